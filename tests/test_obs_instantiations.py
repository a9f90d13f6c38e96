"""Every reachable observation-kernel instantiation (obs_instantiations.py: variant x output type x observations
per env) on the GPU against the C oracle, bit-exact, with guard bands round the observation buffer.

include/zombsole_mi355x.h states no alignment for obs_dev beyond its element type, so each case writes into
three buffers: one at a 16-B boundary, one an element past one, and one 16 B and an element past one.  Each lies
inside a byte tensor filled with 0x5A, 64 B or more before it and after it, and has three padding rows
(eng.outputs(rows=N + 3)); after every launch the bytes before the N envs' blocks, the padding rows and the bytes
after must still be 0x5A.  (0x5A5A = 23 130 is no value an observation holds: codes and weapons are small, a
life is at most 200.)
"""
import numpy as np
import pytest

import obs_instantiations as I
from libzombsole_amd import _abi
from test_obstacle_hp import _poke_all

pytestmark = pytest.mark.gpu

FILL, GUARD, PAD_ROWS, STEPS = 0x5A, 64, 3, 24


class Guarded(object):
    """rows x obs_shape of the engine's dtype at byte `offset` of a 0x5A-filled byte tensor."""

    def __init__(self, eng, offset):
        import torch
        self.n, self.offset = eng.N, offset
        self.ts = torch.empty((), dtype=eng.obs_dtype).element_size()
        self.blk = int(np.prod(eng.obs_shape)) * self.ts
        rows = eng.N + PAD_ROWS
        self.raw = torch.empty(offset + rows * self.blk + GUARD + 16, dtype=torch.uint8, device=eng.device)
        assert self.raw.data_ptr() % 16 == 0 and offset >= GUARD and offset % self.ts == 0
        self.fill()
        self.view = self.raw[offset:offset + rows * self.blk].view(eng.obs_dtype).view((rows,) + tuple(eng.obs_shape))
        assert self.view.data_ptr() == self.raw.data_ptr() + offset
        self.out = eng.outputs(rows=rows, obs=self.view)

    def fill(self):
        self.raw.fill_(FILL)

    def check_guards(self, what):
        end = self.offset + self.n * self.blk
        before, after = self.raw[:self.offset].cpu().numpy(), self.raw[end:].cpu().numpy()
        assert (before == FILL).all(), ("bytes before the buffer written", what, np.nonzero(before != FILL)[0][:8] - self.offset)
        assert (after == FILL).all(), ("padding rows or bytes after the buffer written", what, np.nonzero(after != FILL)[0][:8])

    def obs(self):
        return self.view[:self.n].cpu().numpy()

    def untouched(self):
        return bool((self.raw == FILL).all())


def _into(eng, call, g, mask=None):
    """eng.reset / eng.observe into g's buffer."""
    own = eng.obs
    eng.obs = g.view
    try:
        call(mask)
    finally:
        eng.obs = own
    eng.torch.cuda.synchronize()


def _poke(eng, refs, rng, obstacles):
    """Dead bodies (some under map obstacles), damaged and cleaned-up obstacles, one obstacle in agent 0's window
    (where there is one) far below the int16 range: the same pokes through zs_set_state and the oracle."""
    for e, o in enumerate(refs):
        st = eng.get_state(e)
        W, cells, O = st.W, st.W * st.H, st.O
        dw = st.dead_words.view(np.uint32)  # writes through to the record
        dead = [int(c) for c in rng.choice(cells, size=min(cells // 2, (3, 40, 300)[e % 3]), replace=False)]
        dead += [obstacles[i][1] * W + obstacles[i][0] for i in rng.choice(O, size=3, replace=False)]
        for c in dead:
            dw[c >> 5] |= np.uint32(1 << (c & 31))
            o.poke_dead(c % W, c // W)
        ax, ay = int(st.ent[0][2]), int(st.ent[0][3])
        here = [i for i in range(1, O) if st.obst_present[i]]  # still in the world (a cleaned-up one stays out)
        near = [i for i in here if abs(obstacles[i][0] - ax) <= 10 and abs(obstacles[i][1] - ay) <= 10]
        low = near[len(near) // 2] if near else here[0]
        for i in rng.choice(np.arange(1, O), size=min(O - 1, 12), replace=False):
            if i == low:
                continue
            st.obst_life[i] = int(rng.integers(-32000, 199))
            o.poke_obstacle(int(i), int(st.obst_life[i]))
            if st.obst_life[i] <= 0 and rng.integers(2):
                st.obst_present[i] = 0
                o.poke_obstacle_gone(int(i))
        st.obst_life[low] = -40000
        o.poke_obstacle(low, -40000)
        eng.set_state(e, st)


@pytest.mark.parametrize("row", I.ROWS, ids=[r.id for r in I.ROWS])
def test_instantiation(row):
    """One instantiation: describe() names it; a seeded trajectory of STEPS steps of the discrete action stream
    (episodes of 12 steps on bridge64, of one step on the wall map, so autoresets happen) with every env's
    observation against OracleEnv at every step, the steps writing in turn into the three guarded buffers;
    then poked states (dead bodies, some under obstacles; damaged and cleaned-up obstacles; lives below
    -32 768, which int16 saturates with ZS_OVF_INT16 raised) observed into each buffer; then the plan's masked
    kernel under four masks (none, env 0, the last env, every third): masked blocks equal the oracle, every other
    byte keeps 0x5A."""
    import torch
    from libzombsole_amd.engine import Engine
    from oracle.oracle import OracleEnv

    n = row.n
    eng = Engine(row.builder().set_launch(row.launch))
    desc = eng.describe()
    assert (desc["obs_kernel"], desc["obs_kernel_masked"], desc["obs_encoders"]) == \
        (row.obs_kernel, row.obs_kernel_masked, row.obs_encoders), desc
    assert eng.obs_shape == (row.agents, 3, 21, 21)
    ts = torch.empty((), dtype=eng.obs_dtype).element_size()
    bufs = [Guarded(eng, off) for off in (GUARD, GUARD + ts, GUARD + 16 + ts)]
    assert [g.view.data_ptr() % 16 for g in bufs] == [0, ts, ts]

    # -- trajectory ------------------------------------------------------------------------------------------
    seeds = [7000 + 13 * i for i in range(n)]
    eng.seed(seeds)
    _into(eng, eng.reset, bufs[0])
    obs0 = bufs[0].obs()
    bufs[0].check_guards("reset")
    refs = []
    for k, s in enumerate(seeds):
        o = OracleEnv(row.builder(1))
        o.seed(s)
        assert np.array_equal(obs0[k], o.reset()), ("reset obs", k)
        refs.append(o)
    need = [False] * n
    resets = 0
    for t in range(1, STEPS + 1):
        g = bufs[t % 3]
        eng.gen_actions(t, 7)
        acts = eng.actions.cpu().numpy()
        eng.step(out=g.out)
        torch.cuda.synchronize()
        g.check_guards(("step", t))
        obs, rew = g.obs(), g.out.rewards[:n].cpu().numpy()
        done, trunc, was_reset = (x[:n].cpu().numpy() for x in (g.out.done, g.out.trunc, g.out.was_reset))
        for k, o in enumerate(refs):
            if need[k]:
                assert was_reset[k], ("expected autoreset", k, t)
                exp = o.reset()
                need[k] = False
                resets += 1
            else:
                assert not was_reset[k], ("unexpected reset", k, t)
                exp, r, d, tr, lb = o.step(acts[k])
                assert bool(done[k]) == d and bool(trunc[k]) == tr, ("flags", k, t)
                assert np.array_equal(rew[k][lb], r[:eng.A][lb]), ("rew", k, t)
                need[k] = d or tr
            assert np.array_equal(obs[k], exp), ("obs", k, t)
    assert resets >= n  # every env went through an autoreset

    # -- poked states ----------------------------------------------------------------------------------------
    assert not eng.overflow() & _abi.OVF_INT32
    _poke_all(eng, [(0, -32769)])
    for o in refs:
        o.poke_obstacle(0, -32769)
    _poke(eng, refs, np.random.default_rng(57), eng.builder.map.obstacles)
    want = np.stack([o.obs() for o in refs])
    if row.dtype == _abi.DTYPE_I16:  # the lives below the range are in view, saturated
        assert want.min() == -32768
    else:
        assert want.min() == -40000
    for g in bufs:
        g.fill()
        _into(eng, eng.observe, g)
        g.check_guards("observe")
        got = g.obs()
        for k in range(n):
            assert np.array_equal(got[k], want[k]), ("poked obs", k, g.offset)
    assert eng.overflow() == _abi.OVF_INT16
    if row.dtype == _abi.DTYPE_I16:
        with pytest.raises(OverflowError):
            eng.check_lossless()
    else:
        eng.check_lossless()

    # -- masked launches -------------------------------------------------------------------------------------
    idx = torch.arange(n, device=eng.device)
    masks = {"none": idx < 0, "first": idx == 0, "last": idx == n - 1, "every third": idx % 3 == 0}
    for name, m in masks.items():
        mask, on = m.to(torch.uint8), m.cpu().numpy()
        for g in bufs:
            g.fill()
            _into(eng, eng.observe, g, mask)
            if name == "none":
                assert g.untouched(), ("an all-zero mask wrote", g.offset)
                continue
            g.check_guards(("masked observe", name))
            got = g.obs()
            raw = got.view(np.uint8).reshape(n, -1)
            for k in range(n):
                if on[k]:
                    assert np.array_equal(got[k], want[k]), ("masked obs", name, k, g.offset)
                else:
                    assert (raw[k] == FILL).all(), ("unmasked env written", name, k, g.offset)
    eng.close()
