"""Per-env zombie counts and time limits (ZS_FLAG_ENV_PARAMS) on the GPU: every env of a mixed batch at every step,
bit-exact against an oracle env of its own config (env_params_cases.run; the table: env_params_cases.py, shown by
the oracle alone in test_env_params_plan.py), the unset flagged handle against the unflagged one, the refusals, the
snapshot record's extra section and the guard bands round the two calls' buffers."""
import ctypes as C

import numpy as np
import pytest

import env_params_cases as EP
from libzombsole_amd import _abi
from test_obs_instantiations import FILL, GUARD

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def torch():
    import torch
    return torch


# -- 1: heterogeneous from the start --------------------------------------------------------------------------------
@pytest.mark.parametrize("row", EP.ROWS, ids=lambda r: r.id)
def test_mixed_batch_against_per_env_oracles(row):
    assert EP.run(row) >= 3  # autoresets happened: the next -> current copy ran in the row's kind of reset


# -- 2: changed mid-run ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("row", EP.CHANGE_ROWS, ids=lambda r: r.id)
def test_changed_mid_run(row):
    EP.run(row, change=True)


def test_vector_surfaces_set_and_read(torch):
    """BatchedZombsole(env_params=True) on both surfaces: a dict of three tensors, the two properties, one step."""
    from libzombsole_amd.vector import BatchedZombsole
    for surface, kw in (("multi", dict(agent_ids=["0", "1"])), ("single", dict(agent_id=0))):
        v = BatchedZombsole(surface, 13, "extermination", [], "bridge64", initial_zombies=4, minimum_zombies=2,
                            max_episode_steps=5, env_params=True, **kw)
        dev = v.engine.device
        p = {"initial_zombies": torch.arange(13, device=dev) % 5, "minimum_zombies": torch.arange(13, device=dev) % 3,
             "max_episode_steps": torch.arange(13, device=dev)}
        v.set_env_params(p)
        want = torch.stack([p[k] for k in _abi.ENV_PARAMS], dim=1).to(torch.int32)
        assert torch.equal(v.env_params, want) and torch.equal(v.env_params_current.cpu(), torch.tensor([[4, 2, 5]] * 13, dtype=torch.int32))
        v.step(v.sample_actions(1).clone())  # the implicit first reset
        assert torch.equal(v.env_params_current, want)
        st = [v.engine.get_state(e) for e in range(13)]
        assert [int(s.ent[v.engine.A:, 1].sum()) for s in st] == [e % 5 for e in range(13)]  # initial_e zombies each
        v.close()
        plain = BatchedZombsole(surface, 13, "extermination", [], "bridge64", initial_zombies=4, **kw)
        with pytest.raises(RuntimeError):
            plain.set_env_params(want)
        plain.close()


# -- 3: the unset flagged handle is the unflagged handle ---------------------------------------------------------------
def _run_plain(builder, seeds, steps, nd, torch):
    from libzombsole_amd.engine import Engine
    eng = Engine(builder)
    eng.seed(seeds)
    trace = [eng.reset().cpu().numpy().copy()]
    for t in range(1, steps + 1):
        eng.gen_actions(t, nd)
        eng.step()
        torch.cuda.synchronize()
        trace.append([x.cpu().numpy().copy() for x in (eng.obs, eng.rewards.view(torch.int64), eng.done, eng.trunc,
                                                        eng.listed, eng.was_reset)])
    states = [eng.get_state(k).buf.copy() for k in range(eng.N)]
    rngs = [eng.get_rng(k) for k in range(eng.N)]
    return eng, trace, states, rngs


@pytest.mark.parametrize("row", [EP.ROWS[1], EP.ROWS[4]], ids=lambda r: r.id)
def test_unflagged_handle_against_the_oracle(row, torch):
    """The unflagged side of the comparison below, held to the oracle of the caps' config."""
    from oracle.oracle import OracleEnv
    eng, trace, _, rngs = _run_plain(row.builder(env_params=False), row.seeds(), EP.STEPS, row.nd, torch)
    assert eng.describe()["env_params"] == 0
    for k in range(0, row.n, 5):
        o = OracleEnv(row.make(1, *row.caps))
        o.seed(row.seeds()[k])
        assert np.array_equal(trace[0][k], o.reset())
        need = False
        for t in range(1, EP.STEPS + 1):
            if need:
                exp, need = o.reset(), False
            else:
                exp, r, d, tr, lb = o.step(row.actions([row.seeds()[k]], t, o.A)[0])
                need = d or tr
                assert bool(trace[t][2][k]) == d and bool(trace[t][3][k]) == tr
            assert np.array_equal(trace[t][0][k], exp), (k, t)
        assert np.array_equal(rngs[k], o.get_rng())
    eng.close()


@pytest.mark.parametrize("row", [EP.ROWS[1], EP.ROWS[4]], ids=lambda r: r.id)
def test_unset_flagged_equals_unflagged(row, torch):
    a, ta, sa, ra = _run_plain(row.builder(env_params=False), row.seeds(), EP.STEPS, row.nd, torch)
    b, tb, sb, rb = _run_plain(row.builder(env_params=True), row.seeds(), EP.STEPS, row.nd, torch)
    assert b.describe()["env_params"] == 1
    assert np.array_equal(ta[0], tb[0])
    for t in range(1, EP.STEPS + 1):
        for x, y, name in zip(ta[t], tb[t], ("obs", "rewards", "done", "trunc", "listed", "was_reset")):
            assert np.array_equal(x, y), (name, t)
    assert all(np.array_equal(x, y) for x, y in zip(sa, sb)) and all(np.array_equal(x, y) for x, y in zip(ra, rb))
    caps = torch.tensor([list(row.caps)] * row.n, dtype=torch.int32)
    assert torch.equal(b.env_params().cpu(), caps) and torch.equal(b.env_params(current=True).cpu(), caps)
    # the unflagged record is byte for byte the flagged one without its extra section
    La, Lb = a.snapshot_layout(), b.snapshot_layout()
    sna, snb = a.snapshot().cpu().numpy(), b.snapshot().cpu().numpy()
    o = Lb["env_params"]
    assert o == La["weapon"] and np.array_equal(sna[:, :o], snb[:, :o])
    assert np.array_equal(sna[:, o:La["pad"]], snb[:, o + 24:Lb["pad"]])
    assert np.array_equal(np.ascontiguousarray(snb[:, o:o + 24]).view(np.int32), np.array([list(row.caps) * 2] * row.n, dtype=np.int32))
    a.close()
    b.close()


# -- 4: refusals ------------------------------------------------------------------------------------------------------
@pytest.fixture()
def eng13(torch):
    from libzombsole_amd.engine import Engine
    eng = Engine(_abi.multi_env_config(13, "extermination", [], "bridge64", ["0", "1"], initial_zombies=6, minimum_zombies=3,
                                       max_episode_steps=5, env_params=True))
    yield eng
    eng.close()


def test_out_of_range_entries_are_not_applied(eng13, torch):
    eng = eng13
    idx = [0, 1, 2, 3, -1, 13, 4, 5, 6]
    par = [[1, 1, 1], [7, 0, 0], [0, 4, 0], [2, 2, -1], [1, 1, 1], [1, 1, 1], [-1, 0, 0], [6, 3, 2 ** 31 - 1], [0, -2, 3]]
    want = [[6, 3, 5]] * 13
    want[0], want[5] = [1, 1, 1], [6, 3, 2 ** 31 - 1]
    eng.set_env_params(torch.tensor(par, dtype=torch.int32), envs=idx, check=False)
    assert eng.env_params().cpu().tolist() == want
    assert eng.overflow() & _abi.OVF_PARAM_RANGE  # sticky until cleared
    with pytest.raises(ValueError, match="range"):  # check=True reads the flag, raises and clears that bit only
        eng.set_env_params(torch.tensor([[0, 0, 0]], dtype=torch.int32), envs=[2])
    assert eng.overflow() == 0 and eng.env_params().cpu().tolist()[2] == [0, 0, 0]
    eng.set_env_params(torch.tensor([[3, 3, 3]], dtype=torch.int32), envs=[12])  # in range: no error
    with pytest.raises(ValueError, match="range"):
        eng.set_env_params(torch.tensor([[3, 3, 3]], dtype=torch.int32), envs=[13])
    assert eng.env_params().cpu().tolist()[12] == [3, 3, 3] and eng.overflow() == 0
    # a value or an index that int32 does not hold is refused, not wrapped into range (2 ** 32 + 1 -> 1)
    before = eng.env_params().cpu().tolist()
    with pytest.raises(ValueError, match="range"):
        eng.set_env_params(torch.tensor([[2 ** 32 + 1, 0, 0], [2, 2, 2]], dtype=torch.int64), envs=[3, 2 ** 32 + 4])
    assert eng.env_params().cpu().tolist() == before and eng.overflow() == 0
    # one env named twice: one of the two triples, whole
    eng.set_env_params(torch.tensor([[1, 2, 3], [4, 0, 9]] * 40, dtype=torch.int32), envs=[7] * 80)
    assert eng.env_params().cpu().tolist()[7] in ([1, 2, 3], [4, 0, 9])
    assert torch.equal(eng.env_params(current=True).cpu(), torch.tensor([[6, 3, 5]] * 13, dtype=torch.int32))
    with pytest.raises(ValueError):
        eng.set_env_params(torch.zeros((2, 3), dtype=torch.int32), envs=[1])
    with pytest.raises(ValueError):
        eng.set_env_params(torch.zeros((2, 2), dtype=torch.int32))


def test_unflagged_handle_and_viewer_refuse(torch):
    from libzombsole_amd.engine import Engine, EngineError
    mk = lambda **kw: _abi.multi_env_config(13, "extermination", [], "bridge64", ["0", "1"], initial_zombies=6,  # noqa: E731
                                            minimum_zombies=3, **kw)
    eng = Engine(mk())
    buf = torch.zeros((13, 3), dtype=torch.int32, device=eng.device)
    s = eng._stream()
    assert eng.L.zs_env_params_set(eng.h, None, 13, C.c_void_p(buf.data_ptr()), s) == _abi.ZS_ESTATE
    assert eng.L.zs_env_params_get(eng.h, 0, C.c_void_p(buf.data_ptr()), s) == _abi.ZS_ESTATE
    assert eng.L.zs_env_params_get(eng.h, 1, C.c_void_p(buf.data_ptr()), s) == _abi.ZS_ESTATE
    assert eng.describe()["env_params"] == 0 and "env_params" not in eng.snapshot_layout()
    eng.close()
    with pytest.raises(EngineError, match="viewer"):
        Engine(mk(env_params=True, viewer=True))


# -- 5: snapshot ------------------------------------------------------------------------------------------------------
def test_clone_carries_both_triples(torch):
    """Env 1 (mid-episode) cloned onto env 2, whose triples differ: both then step identically (same actions: the
    policy's seed is set alike) to the episode's end and reset into the same next triple."""
    from libzombsole_amd.vector import BatchedZombsole
    v = BatchedZombsole("multi", 5, "extermination", [], "bridge64", agent_ids=["0", "1"], initial_zombies=6,
                        minimum_zombies=3, max_episode_steps=6, env_params=True, base_seed=700)
    eng = v.engine
    eng.seed([700, 701, 701, 703, 704])  # envs 1 and 2 draw the same actions
    v.set_env_params(torch.tensor([[6, 3, 6], [2, 1, 4], [5, 3, 6], [0, 0, 0], [6, 0, 3]], dtype=torch.int32))
    v.reset()
    for t in (1, 2):
        v.step(v.sample_actions(t).clone(), graph=False)
    v.set_env_params(torch.tensor([[3, 2, 5]], dtype=torch.int32), envs=[1])  # env 1's next episode
    v.clone([1], [2])
    assert eng.env_params(current=True).cpu().tolist()[1:3] == [[2, 1, 4]] * 2
    assert eng.env_params().cpu().tolist()[1:3] == [[3, 2, 5]] * 2
    assert np.array_equal(eng.get_state(1).buf, eng.get_state(2).buf)
    reset_seen = False
    for t in range(3, 9):
        v.step(v.sample_actions(t).clone(), graph=False)
        torch.cuda.synchronize()
        assert np.array_equal(eng.get_state(1).buf, eng.get_state(2).buf), t
        assert torch.equal(eng.obs[1], eng.obs[2]) and torch.equal(eng.rewards[1], eng.rewards[2])
        assert int(eng.trunc[1]) == int(eng.trunc[2]) == (t == 4)  # the clone's TimeLimit is env 1's: 4 steps
        if int(eng.was_reset[1]):
            reset_seen = True
            assert int(eng.was_reset[2]) and eng.env_params(current=True).cpu().tolist()[1:3] == [[3, 2, 5]] * 2
            assert int(eng.get_state(2).ent[eng.A:, 1].sum()) == 3
    assert reset_seen
    v.close()


def test_checkpoint_round_trip_and_refusals(torch, tmp_path):
    from libzombsole_amd.vector import BatchedZombsole
    kw = dict(agent_ids=["0", "1"], initial_zombies=6, minimum_zombies=3, max_episode_steps=6, base_seed=900)
    v = BatchedZombsole("multi", 13, "extermination", [], "bridge64", env_params=True, **kw)
    trip = torch.tensor([EP.TRIPLES(6, 3)[e] for e in range(13)], dtype=torch.int32)
    v.set_env_params(trip)
    v.reset()
    for t in (1, 2, 3):
        v.step(v.sample_actions(t).clone(), graph=False)
    v.set_env_params(torch.tensor([[1, 1, 1]] * 6, dtype=torch.int32), envs=list(range(0, 12, 2)))
    nxt, cur = v.env_params.clone(), v.env_params_current.clone()
    path = str(tmp_path / "run.ckpt")
    v.save_checkpoint(path)
    trace = []
    for t in (4, 5, 6, 7):
        v.step(v.sample_actions(t).clone(), graph=False)
        trace.append((v.obs.clone(), v.engine.rewards.clone(), v.engine.done.clone(), v.engine.trunc.clone(),
                      v.env_params_current.clone()))
    w = BatchedZombsole("multi", 13, "extermination", [], "bridge64", env_params=True, lanes_per_env=8, **kw)
    w.load_checkpoint(path)
    assert torch.equal(w.env_params, nxt) and torch.equal(w.env_params_current, cur)
    for k, t in enumerate((4, 5, 6, 7)):
        w.step(w.sample_actions(t).clone(), graph=False)
        got = (w.obs, w.engine.rewards, w.engine.done, w.engine.trunc, w.env_params_current)
        assert all(torch.equal(x, y) for x, y in zip(trace[k], got)), t
    # a flagged record and an unflagged handle: refused on the fingerprint (checkpoint) and on rec_bytes (zs_restore)
    plain = BatchedZombsole("multi", 13, "extermination", [], "bridge64", **kw)
    Lp, Lf = plain.engine.snapshot_layout(), v.engine.snapshot_layout()
    assert Lp["fingerprint"] != Lf["fingerprint"] == w.engine.snapshot_layout()["fingerprint"]
    assert Lf["rec_bytes"] != Lp["rec_bytes"] and Lf["pad"] == Lp["pad"] + 24
    with pytest.raises(ValueError, match="fingerprint"):
        plain.load_checkpoint(path)
    rec = v.snapshot()
    assert plain.engine.L.zs_restore(plain.engine.h, C.c_void_p(rec.data_ptr()), int(rec.shape[1]), 13, None, None, 13,
                                     plain.engine._stream()) == _abi.ZS_EINVAL
    with pytest.raises(ValueError):
        plain.restore(rec)
    for x in (v, w, plain):
        x.close()


# -- 6: guard bands ---------------------------------------------------------------------------------------------------
def test_guard_bands(eng13, torch):
    """zs_env_params_get's [N][3] output and zs_env_params_set's inputs inside 0x5A-filled byte tensors: every output
    word written, no guard byte touched, the inputs left as they were."""
    eng, N = eng13, 13

    def band(nbytes):
        raw = torch.full((GUARD + nbytes + GUARD,), FILL, dtype=torch.uint8, device=eng.device)
        assert raw.data_ptr() % 16 == 0
        return raw, raw[GUARD:GUARD + nbytes].view(torch.int32)

    praw, par = band(N * 12)
    iraw, idx = band(N * 4)
    trip = torch.tensor([EP.TRIPLES(6, 3)[e] for e in range(N)], dtype=torch.int32)
    par.view(N, 3).copy_(trip)
    idx.copy_(torch.arange(N - 1, -1, -1, dtype=torch.int32))  # env N - 1 - k takes triple k
    before = (praw.clone(), iraw.clone())
    eng.set_env_params(par.view(N, 3), envs=idx, check=False)
    for which in (False, True):
        oraw, out = band(N * 12)
        eng.env_params(current=which, out=out.view(N, 3))
        torch.cuda.synchronize()
        o = oraw.cpu().numpy()
        assert (o[:GUARD] == FILL).all() and (o[GUARD + N * 12:] == FILL).all()
        want = trip.flip(0) if not which else torch.tensor([[6, 3, 5]] * N, dtype=torch.int32)
        assert torch.equal(out.view(N, 3).cpu(), want)
    assert torch.equal(praw, before[0]) and torch.equal(iraw, before[1])
    assert eng.overflow() == 0
    # n smaller than the buffers: only the first n entries are read (the rest would be out of range: 0x5A5A5A5A)
    rc = eng.L.zs_env_params_set(eng.h, C.c_void_p(iraw.data_ptr() + GUARD - 8), 2, C.c_void_p(praw.data_ptr() + GUARD - 24),
                                 eng._stream())
    assert rc == 0 and eng.overflow(clear=True) == _abi.OVF_PARAM_RANGE  # the two entries lie in the guard: refused
    assert torch.equal(eng.env_params().cpu(), trip.flip(0))
