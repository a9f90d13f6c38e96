"""Every row of obs_shapes.py on the GPU against the C oracle, bit-exact, in test_obs_instantiations.py's harness:
three guarded observation buffers (at 16 B, one element past, 16 B and one element past; three padding rows; 0x5A
round them), a seeded trajectory with autoresets, poked states, the masked launches, and the step's other outputs
inside step_runner.GuardedStep's bands.  Then the life edges of the simple encoding, and the plan's refusal."""
import numpy as np
import pytest

import obs_shapes as S
from libzombsole_amd import _abi
from obs_guard import FILL, GUARD, Guarded, _into

pytestmark = pytest.mark.gpu


def _buffers(eng):
    import torch
    ts = torch.empty((), dtype=eng.obs_dtype).element_size()
    bufs = [Guarded(eng, off) for off in (GUARD, GUARD + ts, GUARD + 16 + ts)]
    assert [g.view.data_ptr() % 16 for g in bufs] == [0, ts, ts]
    return bufs


def _masks(eng):
    import torch
    idx = torch.arange(eng.N, device=eng.device)
    return {"none": idx < 0, "first": idx == 0, "last": idx == eng.N - 1, "every third": idx % 3 == 0}


def _check_masked(g, name, on, want, what):
    if name == "none":
        assert g.untouched(), ("an all-zero mask wrote", what, g.offset)
        return
    g.check_guards((what, name))
    got = g.obs()
    raw = got.view(np.uint8).reshape(len(on), -1)
    for k in range(len(on)):
        if on[k]:
            assert np.array_equal(got[k], want[k]), (what, name, k, g.offset)
        else:
            assert (raw[k] == FILL).all(), ("unmasked env written", what, name, k, g.offset)


@pytest.mark.parametrize("row", S.ROWS, ids=[r.id for r in S.ROWS])
def test_row(row):
    """describe() names the row's kernels; the trajectory (row.steps steps of the discrete stream, episodes of
    five steps, so every env autoresets) with every env's observation, rewards, flags and `listed` against OracleEnv
    at every step, the steps writing in turn into the three guarded buffers, and the canonical state of every env
    at the end; poked states (obs_shapes.poke_plan: bodies, one under an obstacle in view; damaged and cleaned-up
    obstacles in view; lives below the int16 range) observed into each buffer; zs_observe under four masks (none, env 0, the last env,
    every third), every unmasked byte still 0x5A; for the `where` rows zs_reset under the same masks."""
    import torch
    from libzombsole_amd.engine import Engine
    from oracle.oracle import OracleEnv
    from step_runner import GuardedStep

    n = row.n
    eng = Engine(row.builder())
    desc = eng.describe()
    assert (desc["obs_kernel"], desc["obs_kernel_masked"], desc["obs_encoders"]) == (row.plan[0], row.plan[1], ""), desc
    if row.lanes:
        assert desc["lanes_per_env"] == row.lanes, desc
    if row.step_kernel:
        assert desc["step_kernel"] == row.step_kernel, desc
    assert eng.obs_shape == row.builder(1).obs_shape()
    bufs = _buffers(eng)
    out = GuardedStep(eng)
    kinds = [o[2] for o in eng.builder.map.obstacles]

    # -- trajectory ------------------------------------------------------------------------------------------
    seeds = row.seeds()
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
    for t in range(1, row.steps + 1):
        g = bufs[t % 3]
        acts = S.actions(seeds, t, eng.A)
        out.clear()
        out.obs = g.view
        out.actions.copy_(torch.from_numpy(acts))
        eng.step(actions=out.actions, out=out)
        torch.cuda.synchronize()
        g.check_guards(("step", t))
        out.check(t)
        obs, rew = g.obs(), out.rewards.cpu().numpy()
        done, trunc, was_reset, listed = (getattr(out, x).cpu().numpy() for x in ("done", "trunc", "was_reset", "listed"))
        for k, o in enumerate(refs):
            if need[k]:
                assert was_reset[k], ("expected autoreset", k, t)
                assert not rew[k].any(), ("rewards of a reset", k, t)
                exp = o.reset()
                need[k] = False
                resets += 1
            else:
                assert not was_reset[k], ("unexpected reset", k, t)
                exp, r, d, tr, lb = o.step(acts[k])
                assert bool(done[k]) == d and bool(trunc[k]) == tr, ("flags", k, t)
                assert np.array_equal(listed[k].astype(bool), lb), ("listed", k, t)
                assert np.array_equal(rew[k][lb[:rew.shape[1]]].view(np.uint64),
                                      r[:rew.shape[1]][lb[:rew.shape[1]]].view(np.uint64)), ("rew", k, t)
                need[k] = d or tr
            assert np.array_equal(obs[k], exp), ("obs", k, t)
    assert resets >= n  # every env went through an autoreset
    for k, o in enumerate(refs):
        assert eng.get_state(k).canonical(kinds) == o.state(), ("state", k)

    # -- poked states ----------------------------------------------------------------------------------------
    assert not eng.overflow() & _abi.OVF_INT32
    rng = np.random.default_rng(57)
    for k, o in enumerate(refs):  # the pokes test_obs_shapes_plan.py counts the classes of, from the oracle's state
        plan = S.poke_plan(eng.builder, o.state(), rng, k)
        S.poke_oracle(o, plan, eng.builder.map.size[0])
        S.poke_engine(eng, k, plan)
    want = np.stack([o.obs() for o in refs])
    for g in bufs:
        g.fill()
        _into(eng, eng.observe, g)
        g.check_guards("observe")
        got = g.obs()
        for k in range(n):
            assert np.array_equal(got[k], want[k]), ("poked obs", k, g.offset)
    assert eng.overflow() == _abi.OVF_INT16
    if row.dt == "i16":
        with pytest.raises(OverflowError):
            eng.check_lossless()
    else:
        eng.check_lossless()

    # -- masked launches -------------------------------------------------------------------------------------
    for name, m in _masks(eng).items():
        mask, on = m.to(torch.uint8), m.cpu().numpy()
        for g in bufs:
            g.fill()
            _into(eng, eng.observe, g, mask)
            _check_masked(g, name, on, want, "masked observe")
    if row in S.WHERE_ROWS:
        for i, (name, m) in enumerate(_masks(eng).items()):
            mask, on = m.to(torch.uint8), m.cpu().numpy()
            want = [refs[k].reset() if on[k] else want[k] for k in range(n)]
            g = bufs[i % 3]
            g.fill()
            _into(eng, eng.reset, g, mask)
            _check_masked(g, name, on, want, "masked reset")
    eng.close()


LIFE_MAP = "wwwwwww\nwp.b.pw\nw.b.b.w\nwwwwwww\n"  # 7 x 4: 18 walls and three boxes round two spawn cells


@pytest.mark.parametrize("dt", S.DTS)
def test_simple_life_edges(dt):
    """Obstacle lives round every edge of 15 * min(life, 100) // 100 (obs_shapes.OBSTACLE_LIVES) and one entity life
    above the cap, poked through zs_set_state and the oracle, on a map whose every cell is inside the agent's window:
    k_obs_pipe (the default), k_obs_gather and k_obs, each into the three guarded buffers.  int16 saturates the cells
    whose value leaves its range and ZS_OVF_INT16 is raised; ZS_OVF_INT32 is not."""
    import obs_model
    from libzombsole_amd.engine import Engine
    from libzombsole_amd.maps import Map
    from oracle.oracle import OracleEnv

    def make(n):
        return _abi.multi_env_config(n, "extermination", [], Map.from_text(LIFE_MAP, name="life_edges"), ["0", "1"],
                                     initial_zombies=0, minimum_zombies=0, observation_position_encoding_style="simple",
                                     obs_dtype=S.DT[dt])
    n = 5
    for lo, kernel in (({}, "k_obs_pipe"), ({"fobs": -1, "obs_pipe": -1, "obs_ring": -1}, "k_obs_gather"),
                       ({"fobs": -1, "obs_pipe": -1, "obs_gather": -1}, "k_obs")):
        eng = Engine(make(n).set_launch(lo))
        assert eng.describe()["obs_kernel"] == kernel
        seeds = [4100 + k for k in range(n)]
        eng.seed(seeds)
        eng.reset()
        refs = []
        O = len(eng.builder.map.obstacles)
        assert O >= len(S.OBSTACLE_LIVES)
        for k, s in enumerate(seeds):
            o = OracleEnv(make(1))
            o.seed(s)
            o.reset()
            st = eng.get_state(k)
            for j, life in enumerate(S.OBSTACLE_LIVES):
                i = (j + 5 * k) % O  # another obstacle (wall or box) takes each life in every env
                st.obst_life[i] = life
                o.poke_obstacle(i, life)
            st.ent[1, 4] = S.ENTITY_LIFE
            o.poke_life(0, 1, S.ENTITY_LIFE)
            eng.set_state(k, st)
            refs.append(o)
        want = np.stack([o.obs() for o in refs])
        agent = 256 * _abi.THING_AGENT + 16 * int(eng.get_state(0).ent[1, 5]) + 15  # the life above 100 shows as 15
        for k, o in enumerate(refs):  # the model's Python ints say the same, and the poked lives are in view
            assert np.array_equal(want[k], obs_model.observe(make(1), o.state(), [0, 1]))
            assert (want[k] == agent).any(), k
        lowest = [256 * kind + (15 * -2147483647) // 100 for kind in (_abi.THING_BOX, _abi.THING_WALL)]
        assert want.min() == -32768 if dt == "i16" else want.min() in lowest
        for g in _buffers(eng):
            _into(eng, eng.observe, g)
            g.check_guards("observe")
            got = g.obs()
            for k in range(n):
                assert np.array_equal(got[k], want[k]), ("life edges", kernel, k, g.offset)
        assert eng.overflow() == _abi.OVF_INT16
        eng.close()


def test_refused_then_created():
    """zs_create refuses a config none of whose image tiers fits 64 KiB with the plan's message, and the next
    zs_create succeeds."""
    from libzombsole_amd.engine import Engine, EngineError
    make, msg, _ = S.REFUSED
    with pytest.raises((EngineError, ValueError)) as err:
        Engine(make(13))
    assert msg in str(err.value)
    row = S.ROWS[0]
    eng = Engine(row.builder())
    eng.seed(row.seeds())
    eng.reset()
    eng.close()
