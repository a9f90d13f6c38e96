"""Every row and launch variant of reset_shapes.py on the GPU against the oracle's run of the row (computed once a
row, shared by its variants): the reset observation; at every step every env's observations, rewards (bit-exact,
the listed agents'), done, truncated, the autoreset flag and `listed`; after the first reset and after the last
step every env's full state (dict order included, the spawn serials consistent) and its stream.  Eager
launches, and for the rows with autoresets the replayed step graphs too."""
import numpy as np
import pytest

import reset_shapes as R
import step_plan_table as T

pytestmark = pytest.mark.gpu

_runs = {}


def reference(row):
    if row.id not in _runs:
        _runs[row.id] = R.oracle_run(row)
    return _runs[row.id]


def plan_of(row, ov):
    launch = dict(ov, fobs=-1)
    launch.pop("lanes_per_env", None)
    return T.plans([(row.builder(ov), launch)])[0]


def check_states(eng, expect, where, fresh=False):
    """Every env's canonical state and stream against the oracle's; the spawn serials of the things in the dict
    are distinct and at or below the env's counter (a move re-inserts a thing, so they rise along the dict order
    only after a reset: 1 .. n after a new handle's first one)."""
    kinds = [o[2] for o in eng.builder.map.obstacles]
    for k, (state, rng) in enumerate(expect):
        sv = eng.get_state(k)
        assert sv.canonical(kinds) == state, ("state", where, k)
        ser = [int(sv.ent[int(s)][7]) for s in sv.order[:sv.n_order]]
        assert len(set(ser)) == len(ser) and all(0 < v <= int(sv.buf[12]) for v in ser), ("serials", where, k, ser)
        if fresh:
            assert ser == list(range(1, sv.n_order + 1)), ("first serials", where, k, ser)
        assert R.same_stream(eng.get_rng(k), rng), ("stream", where, k)


def run_variant(row, ov, graph):
    import torch
    from libzombsole_amd.engine import Engine
    census, final, traces, obs0, after0 = reference(row)
    p = plan_of(row, ov)
    eng = Engine(row.builder(ov))
    try:
        desc = eng.describe()
        assert desc["step_kernel"] == ("k_step" if p["fused"] else "k_tick"), desc
        assert desc["respawn"] == ("k_respawn" if p["defer_respawn"] else "tick"), desc
        assert desc["lanes_per_env"] == p["G"] and desc["reset_lds"] == p["reset_lds"], (desc, p)
        seeds = row.seeds()
        eng.seed(seeds)
        got0 = eng.reset().cpu().numpy()
        for k in range(row.n):
            assert np.array_equal(got0[k], obs0[k]), ("reset obs", k)
        check_states(eng, after0, "reset", fresh=True)
        if row.setup == "walls":
            for k in range(row.n):
                sv = eng.get_state(k)
                sv.obst_present[4096:] = 0
                eng.set_state(k, sv)
        A = eng.A
        for t in range(1, row.steps + 1):
            if graph:
                eng.step_graph(t, 7)
            else:
                eng.gen_actions(t, 7)
                eng.step()
            torch.cuda.synchronize()
            g = {k: getattr(eng, k).cpu().numpy() for k in ("obs", "rewards", "done", "trunc", "listed", "was_reset")}
            if t == 1:
                assert np.array_equal(eng.actions.cpu().numpy(), row.actions(seeds, t, A)), "action stream"
            for k in range(row.n):
                exp, r, d, tr, lb, was = traces[k][t - 1]
                assert bool(g["was_reset"][k]) == was, ("autoreset flag", k, t)
                assert bool(g["done"][k]) == d and bool(g["trunc"][k]) == tr, ("flags", k, t)
                assert np.array_equal(g["listed"][k].astype(bool), lb), ("listed", k, t)
                if was:
                    assert not g["rewards"][k].any(), ("rewards of a reset", k, t)
                elif eng.multi:
                    assert np.array_equal(g["rewards"][k][lb].view(np.uint64), r[:A][lb].view(np.uint64)), ("rew", k, t)
                else:
                    assert np.array_equal(g["rewards"][k].view(np.uint64), r[:1].view(np.uint64)), ("rew", k, t)
                assert np.array_equal(g["obs"][k], exp), ("obs", k, t)
        check_states(eng, final, "last step")
        assert eng.overflow() == 0
    finally:
        eng.close()


CASES = [(r, vid, ov) for r in R.ROWS for vid, ov in r.variants]
GRAPH_CASES = [c for c in CASES if "autoresets" in c[0].claims]


@pytest.mark.parametrize("row,vid,ov", CASES, ids=["%s-%s" % (r.id, v) for r, v, _ in CASES])
def test_shape(row, vid, ov):
    run_variant(row, ov, graph=False)


@pytest.mark.parametrize("row,vid,ov", GRAPH_CASES, ids=["%s-%s" % (r.id, v) for r, v, _ in GRAPH_CASES])
def test_shape_graph(row, vid, ov):
    run_variant(row, ov, graph=True)
