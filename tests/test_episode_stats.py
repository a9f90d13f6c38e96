"""Per-env episode statistics (ZS_FLAG_EPISODE_STATS) on the GPU.  Expected values come from the oracle's per-step
rewards, done, truncated and states run through episode_model.py (episode_cases.trace: computed once per row, shared,
never modified), never from the engine's own outputs; floats are compared as hex strings.  The table:
episode_cases.py, shown by the oracle alone in test_episode_stats_plan.py."""
import ctypes as C

import numpy as np
import pytest

import env_params_cases as EP
import episode_cases as EC
import episode_model as EM
from libzombsole_amd import _abi

pytestmark = pytest.mark.gpu

FILL, PAD = 0x5A, 3  # guard bands: the get outputs start PAD (odd) elements into 0x5A-filled byte tensors
KEYS = ("run_ret", "last_ret", "sum_ret", "last", "tot")
M32 = 0xffffffff


@pytest.fixture(scope="module")
def torch():
    import torch
    return torch


def engine_of(row, **flags):
    from libzombsole_amd.engine import Engine
    eng = Engine(row.builder(**flags))
    eng.seed(row.seeds())
    eng.reset()
    return eng


def fetch(eng, mask=None):
    """zs_episode_stats_get into guarded tensors: the five arrays on the host; guards and masked-out rows checked."""
    t = eng.torch
    R = eng.episode_stats_layout()["R"]
    raws, out = {}, {}
    for k in KEYS:
        dt, w, isz = (t.float64, R, 8) if k.endswith("ret") else (t.int32, 8, 4)
        raw = t.full(((2 * PAD + eng.N * w) * isz,), FILL, dtype=t.uint8, device=eng.device)
        raws[k] = raw
        out[k] = raw[PAD * isz:(PAD + eng.N * w) * isz].view(dt).view(eng.N, w)
    eng.episode_stats(mask, out=out)
    t.cuda.synchronize()
    keep = None if mask is None else (mask.cpu().numpy() == 0)
    got = {}
    for k in KEYS:
        isz = out[k].element_size()
        b = raws[k].cpu().numpy()
        assert (b[:PAD * isz] == FILL).all() and (b[-PAD * isz:] == FILL).all(), ("guard", k)
        if keep is not None:
            rows = b[PAD * isz:-PAD * isz].reshape(eng.N, -1)
            assert (rows[keep] == FILL).all(), ("masked-out rows", k)
        got[k] = out[k].cpu().numpy()
    return got


def check(got, snap, envs=None, what=None):
    for e in (range(len(snap["tot"])) if envs is None else envs):
        for k in ("run_ret", "last_ret", "sum_ret"):
            assert EM.hexes(got[k][e]) == snap[k][e], (k, e, what)
        assert [int(v) for v in got["last"][e]] == snap["last"][e], ("last", e, what)
        assert [int(v) & M32 for v in got["tot"][e]] == snap["tot"][e], ("tot", e, what)


def acts(eng, row, t):
    return eng.torch.from_numpy(row.actions(row.seeds(), t, eng.A)).to(eng.device)


# -- 1, 2: eager and graph replay, every step ---------------------------------------------------------------------------
@pytest.mark.parametrize("graph", (False, True), ids=("eager", "graph"))
@pytest.mark.parametrize("row", EC.ROWS, ids=lambda r: r.id)
def test_every_step_equals_the_model(row, graph, torch):
    snaps, ends = EC.trace(row.id)
    eng = engine_of(row)
    d = eng.describe()
    assert d["episode_stats"] == 1 and d["step_kernel"] == row.step_kernel and d["envs"] == row.n
    assert eng.episode_stats_layout()["R"] == row.R
    check(fetch(eng), snaps[0], what="reset")
    for t in range(1, EC.STEPS + 1):
        if graph:
            eng.actions.copy_(acts(eng, row, t))
            eng.step_graphed()
        else:
            eng.step(acts(eng, row, t))
        if t % 5 == 2:  # a masked get: the other rows stay 0x5A
            mask = (torch.arange(row.n, device=eng.device) % 3 == 1).to(torch.uint8)
            check(fetch(eng, mask), snaps[t], envs=range(1, row.n, 3), what=t)
        check(fetch(eng), snaps[t], what=t)
    assert len(ends) >= 3
    eng.close()


# -- 3: multi-step launches ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("row", [r for r in EC.ROWS if r.config in EC.MULTI_STEP], ids=lambda r: r.id)
def test_sixteen_steps_per_launch(row, torch):
    snaps, _ = EC.trace(row.id, 48)
    eng = engine_of(row)
    for k in (1, 2, 3):
        eng.step_graph(1, 7, steps=16)  # the device policy is the row's discrete stream
        check(fetch(eng), snaps[16 * k], what=16 * k)
    eng.close()


# -- 4: reset_dev omitted -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("row", [EC.ROWS[0], EC.ROWS[3], EC.ROWS[13]], ids=lambda r: r.id)
def test_step_without_listed_and_reset_outputs(row, torch):
    snaps, _ = EC.trace(row.id)
    eng = engine_of(row)
    p = lambda x: C.c_void_p(x.data_ptr())  # noqa: E731
    for t in range(1, EC.STEPS + 1):
        a = acts(eng, row, t)
        rc = eng.L.zs_step(eng.h, p(a), p(eng.obs), p(eng.rewards), p(eng.done), p(eng.trunc), None, None, eng._stream())
        assert rc == 0
        check(fetch(eng), snaps[t], what=t)
    eng.close()


# -- 5, 6: masked zs_reset mid-episode; no autoreset ----------------------------------------------------------------------
@pytest.mark.parametrize("row", [EC.ROWS[2], EC.ROWS[7]], ids=lambda r: r.id)
def test_masked_reset_mid_episode(row, torch):
    eng = engine_of(row)
    tracks = [EC.Track(row, s) for s in row.seeds()]

    def step(t):
        eng.step(acts(eng, row, t))
        for k in tracks:
            k.step(t)
        return fetch(eng)
    for t in (1, 2, 3):
        before = step(t)
    third = list(range(0, row.n, 3))
    mask = torch.zeros(row.n, dtype=torch.uint8, device=eng.device)
    mask[third] = 1
    eng.reset(mask)
    for e in third:
        tracks[e].reset()
    got = fetch(eng)
    assert not got["run_ret"][third].any() and any(float.fromhex(h) != 0.0 for e in third for h in EM.hexes(before["run_ret"][e]))
    for k in KEYS:
        others = [e for e in range(row.n) if e % 3]
        assert np.array_equal(got[k][others], before[k][others]), k
        if k != "run_ret":
            assert np.array_equal(got[k], before[k]), k  # an abandoned episode is not counted
    check(got, EM.snapshot([k.m for k in tracks]), what="after the masked reset")
    for t in range(4, 16):
        check(step(t), EM.snapshot([k.m for k in tracks]), what=t)
    eng.close()


def test_without_autoreset_an_env_is_counted_once(torch):
    row = [r for r in EC.ROWS if r.config == "surv_melee"][1]
    eng = engine_of(row, autoreset=False)
    tracks = [EC.Track(row, s, autoreset=False) for s in row.seeds()]
    ended = {}
    for t in range(1, 17):
        eng.step(acts(eng, row, t))
        for e, k in enumerate(tracks):  # an ended env keeps ticking on both sides (its stream moves on); the model is closed
            k.step(t)
            if k.need and e not in ended:
                ended[e] = t
        got = fetch(eng)
        done = eng.done.cpu().numpy()
        for e in ended:
            assert done[e] == 1, (e, t)  # it goes on reporting done
        check(got, EM.snapshot([k.m for k in tracks]), what=t)
        assert all(int(got["tot"][e][0]) == 1 for e in ended)
    assert len(ended) >= 3
    mask = torch.zeros(row.n, dtype=torch.uint8, device=eng.device)
    mask[sorted(ended)] = 1
    eng.reset(mask)
    for e in ended:
        tracks[e].reset()
    got = fetch(eng)
    assert not got["run_ret"][sorted(ended)].any()
    check(got, EM.snapshot([k.m for k in tracks]), what="masked reset")
    eng.step(acts(eng, row, 17))
    for k in tracks:
        k.step(17)
    check(fetch(eng), EM.snapshot([k.m for k in tracks]), what=17)
    eng.close()


# -- 7: snapshot, restore, clone, checkpoints ---------------------------------------------------------------------------
def test_clone_carries_the_running_return_only(torch):
    from libzombsole_amd.engine import Engine
    row = EC.ROWS[1]  # evac_tiny, unfused
    seeds = row.seeds()
    aseeds = list(seeds)  # whose action stream every env follows: after the clone env 2 follows env 1's
    eng = engine_of(row)
    tracks = [EC.Track(row, s) for s in seeds]

    def step(t):
        eng.step(torch.from_numpy(row.actions(aseeds, t, eng.A)).to(eng.device))
        for k in tracks:
            k.step(t)
    for t in (1, 2, 3, 4, 5, 6, 7, 8):
        step(t)
    before = fetch(eng)
    check(before, EM.snapshot([k.m for k in tracks]), what="before the clone")
    L, EL = eng.snapshot_layout(), eng.episode_stats_layout()
    rec = eng.snapshot()
    torch.cuda.synchronize()
    # the record's ep_run section: run_ret, run_flags, four zero bytes, 8-byte aligned
    assert EL["ep_run"] % 8 == 0 and EL["ep_bytes"] == 8 * row.R + 8 and L["weapon"] == EL["ep_run"] + EL["ep_bytes"]
    sec = np.ascontiguousarray(rec.cpu().numpy()[:, EL["ep_run"]:EL["ep_run"] + EL["ep_bytes"]])
    assert [EM.hexes(x) for x in sec[:, :8 * row.R].copy().view(np.float64)] == [EM.hexes(k.m.run) for k in tracks]
    assert sec[:, 8 * row.R:].copy().view(np.int32).tolist() == [[k.m.closed, 0] for k in tracks]
    # the fork: env 2 becomes env 1; its last episode and totals stay its own
    idx = lambda v: torch.tensor(v, dtype=torch.int32, device=eng.device)  # noqa: E731
    eng.restore(eng.snapshot(idx([1])), None, idx([2]))
    fork = EC.Track(row, seeds[1])
    for t in range(1, 9):
        fork.step(t)
    fork.m.last_ret, fork.m.last, fork.m.tot, fork.m.sum_ret = tracks[2].m.last_ret, tracks[2].m.last, tracks[2].m.tot, tracks[2].m.sum_ret
    tracks[2] = fork
    aseeds[2] = seeds[1]
    got = fetch(eng)
    assert EM.hexes(got["run_ret"][2]) == EM.hexes(before["run_ret"][1])
    for k in ("last_ret", "sum_ret", "last", "tot"):
        assert np.array_equal(got[k], before[k]), k
    check(got, EM.snapshot([k.m for k in tracks]), what="after the clone")
    for t in range(9, 20):
        step(t)
        check(fetch(eng), EM.snapshot([k.m for k in tracks]), what=t)
    # flagged and unflagged handles refuse each other's records
    plain = Engine(row.plain_builder())
    assert plain.snapshot_layout()["fingerprint"] != L["fingerprint"] and plain.describe()["episode_stats"] == 0
    with pytest.raises(ValueError):
        plain.restore(rec)
    with pytest.raises(ValueError):
        eng.restore(plain.snapshot())
    plain.close()
    eng.close()


def test_checkpoint_round_trip_and_refusal(torch, tmp_path):
    from libzombsole_amd.vector import BatchedZombsole
    m = EC.ROWS[0].make(1).map  # evac_tiny: lives change from the first steps on, so the running returns are not zero
    kw = dict(agent_ids=["0", "1", "2", "3"], initial_zombies=2, minimum_zombies=2, max_episode_steps=6, base_seed=900,
              observation_surroundings_width=7)
    v = BatchedZombsole("multi", 13, "evacuation", [], m, episode_stats=True, **kw)
    v.reset()
    for t in range(1, 10):
        v.step(v.sample_actions(t).clone(), graph=False)
    saved = {k: x.clone() for k, x in v.episode_stats().items()}
    assert int(saved["tot"][:, 0].sum()) >= 13 and bool(saved["run_ret"].any())
    path = str(tmp_path / "run.ckpt")
    v.save_checkpoint(path)
    for t in range(10, 14):
        v.step(v.sample_actions(t).clone(), graph=False)
    w = BatchedZombsole("multi", 13, "evacuation", [], m, episode_stats=True, lanes_per_env=8, **kw)
    w.load_checkpoint(path)
    got = w.episode_stats()
    assert torch.equal(got["run_ret"].view(torch.int64), saved["run_ret"].view(torch.int64))
    assert not got["tot"].any() and not got["last"].any()  # the slot's own: a record does not carry them
    for t in range(10, 14):
        w.step(w.sample_actions(t).clone(), graph=False)
    a, b = v.episode_stats(), w.episode_stats()
    assert torch.equal(a["run_ret"].view(torch.int64), b["run_ret"].view(torch.int64))
    assert torch.equal(a["tot"] - saved["tot"], b["tot"])
    assert torch.equal(a["last"][:, :7][b["tot"][:, 0] > 0], b["last"][:, :7][b["tot"][:, 0] > 0])
    plain = BatchedZombsole("multi", 13, "evacuation", [], m, **kw)
    with pytest.raises(ValueError, match="fingerprint"):
        plain.load_checkpoint(path)
    with pytest.raises(RuntimeError):
        plain.episode_stats()
    for x in (v, w, plain):
        x.close()


# -- 8: with env_params ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("row", [EP.ROWS[1], EP.ROWS[4]], ids=lambda r: r.id)
def test_last_holds_the_finished_episodes_own_triple(row, torch):
    from libzombsole_amd.engine import Engine
    b = row.builder()
    b.cfg.flags |= _abi.FLAG_EPISODE_STATS
    eng = Engine(b)
    seeds, trip = row.seeds(), row.triples()
    eng.seed(seeds)
    eng.set_env_params(torch.tensor(trip, dtype=torch.int32))
    tracks = [EP.Track(row, s, t) for s, t in zip(seeds, trip)]
    R = 1 if row.config == "melee_single" else eng.A
    models = [EM.EnvModel(R, int(b.cfg.rules)) for _ in seeds]
    eng.reset()
    for k in tracks:
        k.reset()
    differ = 0
    for t in range(1, EP.STEPS + 1):
        if t == EP.CHANGE_AFTER + 1:
            new = row.changed()
            eng.set_env_params(torch.tensor([new[e] for e in sorted(new)], dtype=torch.int32), envs=sorted(new))
            for e, v in new.items():
                tracks[e].pending = v
        eng.gen_actions(t, row.nd)
        eng.step()
        for k, m in zip(tracks, models):
            cur = k.triple  # the triple the step runs under (a reset step takes up the pending one)
            _, r, d, tr, _ = k.step(t)
            if r is None:
                m.reset()
            else:
                m.step(r, d, tr, k.o.state(), cur)
                differ += (d or tr) and k.pending is not None and tuple(k.pending) != tuple(cur)
        check(fetch(eng), EM.snapshot(models), what=t)
    assert differ >= 3  # episodes that ended with another triple already waiting
    eng.close()


# -- 9: with action masks -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("graph", (False, True), ids=("eager", "graph"))
def test_with_bound_action_masks(graph, torch):
    row = EC.ROWS[0]
    snaps, _ = EC.trace(row.id)
    eng = engine_of(row)
    eng.bind_action_masks()
    for t in range(1, 13):
        if graph:
            eng.actions.copy_(acts(eng, row, t))
            eng.step_graphed()
        else:
            eng.step(acts(eng, row, t))
        bound = eng.masks.clone()
        fresh = eng.action_mask(out=torch.zeros_like(bound))  # the masks of the state the step left, on their own
        assert torch.equal(bound, fresh), t
        check(fetch(eng), snaps[t], what=t)
    assert bool(eng.masks.any())
    eng.close()


# -- 10: clear --------------------------------------------------------------------------------------------------------------
def test_clear_keeps_the_running_part(torch):
    row = EC.ROWS[12]  # single_duel
    eng = engine_of(row)
    tracks = [EC.Track(row, s) for s in row.seeds()]
    for t in range(1, 12):
        eng.step(acts(eng, row, t))
        for k in tracks:
            k.step(t)
    assert sum(k.m.tot[0] for k in tracks) >= 3
    mask = (torch.arange(row.n, device=eng.device) % 2 == 0).to(torch.uint8)
    eng.clear_episode_stats(mask)
    for k in tracks[::2]:
        k.m.clear()
    got = fetch(eng)
    assert not got["tot"][::2].any() and not got["last"][::2].any() and not got["last_ret"][::2].any()
    check(got, EM.snapshot([k.m for k in tracks]), what="cleared")
    first = set()
    for t in range(12, 25):
        eng.step(acts(eng, row, t))
        for e, k in enumerate(tracks):
            k.step(t)
            if k.terminal and e % 2 == 0 and e not in first:
                first.add(e)
                assert k.m.last[7] == 1
        check(fetch(eng), EM.snapshot([k.m for k in tracks]), what=t)
    assert len(first) >= 3
    eng.close()


# -- 11: refusals -------------------------------------------------------------------------------------------------------------
def test_refusals(torch):
    from libzombsole_amd.engine import Engine, EngineError
    row = EC.ROWS[0]
    eng = Engine(row.plain_builder())
    buf = torch.zeros(row.n * 8 * 8, dtype=torch.uint8, device=eng.device)
    p, s = C.c_void_p(buf.data_ptr()), eng._stream()
    out = (C.c_int32 * 8)()
    assert eng.L.zs_episode_stats_layout(eng.h, out) == _abi.ZS_ESTATE
    assert eng.L.zs_episode_stats_get(eng.h, None, p, None, None, None, None, s) == _abi.ZS_ESTATE
    assert eng.L.zs_episode_stats_clear(eng.h, None, s) == _abi.ZS_ESTATE
    torch.cuda.synchronize()
    assert not buf.any() and eng.describe()["episode_stats"] == 0
    eng.close()
    b = row.builder()
    b.cfg.flags |= _abi.FLAG_VIEWER
    with pytest.raises(EngineError, match="viewer"):
        Engine(b)
    eng = Engine(row.builder())
    assert eng.describe()["episode_stats"] == 1
    eng.close()


# -- 12: episode_totals -------------------------------------------------------------------------------------------------------
def test_episode_totals_by_group(torch):
    import math
    from libzombsole_amd.vector import BatchedZombsole
    row = EC.ROWS[0]  # evac_tiny, 13 envs: built here through the batched front end, its seeds the row's
    snaps, _ = EC.trace(row.id)
    v = BatchedZombsole("multi", row.n, "evacuation", [], row.make(1).map, agent_ids=["0", "1", "2", "3"], initial_zombies=2,
                        minimum_zombies=2, max_episode_steps=6, observation_surroundings_width=7, base_seed=row.seed0,
                        episode_stats=True)
    v.reset()
    for t in range(1, EC.STEPS + 1):
        v.step(acts(v.engine, row, t), graph=False)
    check({k: x.cpu().numpy() for k, x in v.episode_stats().items()}, snaps[-1], what="front end")
    groups = np.arange(row.n) % 3
    got = v.episode_totals(torch.from_numpy(groups), 3)
    tot = np.array(snaps[-1]["tot"], dtype=np.int64)
    for k in range(8):
        assert got["tot"][:, k].cpu().tolist() == np.bincount(groups, weights=tot[:, k], minlength=3).astype(np.int64).tolist()
    ret = [[float.fromhex(h) for h in env] for env in snaps[-1]["sum_ret"]]
    for g in range(3):
        envs = [e for e in range(row.n) if groups[e] == g]
        for r in range(row.R):
            xs = [ret[e][r] for e in envs]
            bound = len(envs) * 2.0 ** -53 * math.fsum(abs(x) for x in xs)
            assert abs(float(got["sum_ret"][g, r]) - math.fsum(xs)) <= bound, (g, r)
    one = v.episode_totals()
    assert one["tot"].cpu().tolist() == [tot.sum(axis=0).tolist()]
    v.close()
