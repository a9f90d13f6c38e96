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
from obs_guard import FILL, GUARD, PAD_ROWS, Guarded, _into, _poke  # noqa: F401 (step_runner.py takes FILL, GUARD from here)
from test_obstacle_hp import _poke_all

pytestmark = pytest.mark.gpu

STEPS = 24


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
