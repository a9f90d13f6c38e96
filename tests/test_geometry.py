"""The geometry table (geometry_shapes.py) on the GPU: every accepted row at 13 and 37 envs for 24 steps of the far
action stream in episodes of five, at the requested G = 1, 8 and 64, on k_step and k_tick, with the lanes'
execution and the leader's, eager and through step_graph, every env and step against the oracle inside guard bands
(step_runner.py): the reset observation and the observations, rewards bit-exact, flags and `listed`, the full state
at every terminal step, after every autoreset and at the end, the RNG stream at the end; k_action_mask against
mask_model.py after every step; on the observation rows the plan's masked kernel under two masks; and what
zs_create refuses."""
import numpy as np
import pytest

import geometry_shapes as G
import mask_model as M
from step_runner import run_engines
from test_obs_instantiations import FILL, Guarded, _into

pytestmark = pytest.mark.gpu

CASES = [(r.id, v[0], n, graph) for r in G.ROWS for v in r.variants for n in G.ENVS for graph in (False, True)]


def _describe(row, n, g, kernel, par, vname):
    d = {"envs": n, "lanes_per_env": row.G[g], "step_kernel": kernel, "par_exec": 1 if par >= 0 else 0,
         "respawn": "k_respawn" if vname == "k_respawn" else "tick"}
    if row.obs:
        d["obs_kernel"], d["obs_kernel_masked"], d["obs_encoders"] = row.obs
    return d


@pytest.mark.parametrize("rid,vname,n,graph", CASES, ids=["%s-%s-%d-%s" % (c[0], c[1], c[2], "graph" if c[3] else "eager")
                                                          for c in CASES])
def test_row(rid, vname, n, graph):
    """Twelve engines of one row and respawn variant in lock step (G x kernel x par_exec) against one oracle per
    env; describe() against the row's claims; the masks of a k_step and a k_tick engine against the model on the
    oracle's state after the reset and after every step."""
    row = G.BY_ID[rid]
    combos = [(g, k, p) for g in G.GS for k in ("k_step", "k_tick") for p in (1, -1)]
    assert combos[0][1] == "k_step" and combos[2][1] == "k_tick"
    builders = [row.builder(n, g, k, p, vname) for g, k, p in combos]
    mp = M.MapInfo(builders[0].map)

    def masks(t, engs, refs):
        want = [np.array(M.masks(o.state(), mp, engs[0].A, engs[0].n_discrete), dtype=np.uint8) for o in refs]
        for i in (0, 2):  # a k_step and a k_tick engine (combos): the fused and the unfused launch store the state
            got = engs[i].action_mask().cpu().numpy()
            for k in range(len(refs)):
                assert np.array_equal(got[k], want[k]), ("action mask", i, k, t, got[k].tolist(), want[k].tolist())

    resets, respawns = run_engines(builders, row.make, row.seeds(n), G.STEPS, row, graph=graph, states_at=(G.STEPS,),
                                   expect=[_describe(row, n, g, k, p, vname) for g, k, p in combos], terminal=True,
                                   after_step=masks)
    assert sum(resets) >= 3 * n and sum(respawns) >= 3


OBS_ROWS = [r for r in G.ROWS if r.obs]


@pytest.mark.parametrize("row", OBS_ROWS, ids=[r.id for r in OBS_ROWS])
def test_masked_observe(row):
    """The plan's masked kernel on the observation rows after five steps, under two masks (the last env, every
    third): masked blocks equal the oracle's, every other byte keeps its fill, the guards hold."""
    import torch
    from libzombsole_amd.engine import Engine
    from oracle.oracle import OracleEnv
    n = 13
    eng = Engine(row.builder(n, 0, "k_tick", 1, row.variants[0][0]))
    assert eng.describe()["obs_kernel_masked"] == row.obs[1]
    seeds = row.seeds(n)
    eng.seed(seeds)
    eng.reset()
    refs = []
    for s in seeds:
        o = OracleEnv(row.make(1))
        o.seed(s)
        o.reset()
        refs.append(o)
    for t in range(1, 5):  # no episode ends before step 5
        acts = row.actions(seeds, t, eng.A)
        eng.actions.copy_(torch.from_numpy(acts))
        eng.step()
        for k, o in enumerate(refs):
            o.step(acts[k])
    want = np.stack([o.obs() for o in refs])
    ts = torch.empty((), dtype=eng.obs_dtype).element_size()
    idx = torch.arange(n, device=eng.device)
    for name, m in (("last", idx == n - 1), ("every third", idx % 3 == 0)):
        g = Guarded(eng, 64 + ts)
        _into(eng, eng.observe, g, m.to(torch.uint8))
        g.check_guards(("masked observe", name))
        got, on = g.obs(), m.cpu().numpy()
        raw = got.view(np.uint8).reshape(n, -1)
        for k in range(n):
            if on[k]:
                assert np.array_equal(got[k], want[k]), ("masked obs", name, k)
            else:
                assert (raw[k] == FILL).all(), ("unmasked env written", name, k)
    eng.close()


@pytest.mark.parametrize("rid", sorted(G.REFUSED))
def test_refused(rid):
    """zs_create returns ZS_EINVAL (ValueError) with the message the table names, and the next zs_create of a small
    config succeeds."""
    from libzombsole_amd.engine import Engine
    make, msg, _ = G.REFUSED[rid]
    with pytest.raises(ValueError) as e:
        Engine(make(13))
    assert msg in str(e.value), str(e.value)
    small = G.BY_ID["c256x2"]
    eng = Engine(small.builder(3))
    eng.seed(small.seeds(3))
    eng.reset()
    eng.close()
