"""k_nav (csrc/zs_nav.hpp) through the C ABI and the Python layers: word for word against libzombsole_amd/nav.py's
encode and field of states that equal the oracle's, on every row of nav_cases at 13 and 37 envs; as a step's bound last
launch under both step kernels, three lane counts and graphed steps; both fields together against each alone; masked
and inside guard bands; on a viewer; after restore and clone; the refusals; BatchedZombsole(nav=...), the drop-ins'
path_distances() and the two loops of INTEGRATION.md.

The expected rows are the model's of the engine's state record (Engine.get_state) after that record's things and
obstacles have been held equal to the oracle's state of the same env and step (the first 13 envs)."""
import ctypes as C

import numpy as np
import pytest

import mask_model as M
import nav_cases as NC
from libzombsole_amd import _abi
from libzombsole_amd import nav as NV
from libzombsole_amd.entity_obs import Static

pytestmark = pytest.mark.gpu
CAP = NV.MAX_DIST


def _engine(b, **kw):
    from libzombsole_amd.engine import Engine
    return Engine(b, **kw)


def _row_engine(row, n, launch=None, **over):
    """The engine of a row's n envs, seeded and poked as the oracle's run of it (nav_cases.oracle_trace), reset."""
    b = NC.builder(row, n, **over)
    if launch:
        b.set_launch(launch)
    eng = _engine(b)
    eng.seed([NC.SEED0 + k for k in range(n)])
    for k in range(n if NC.pokes_of(row) else 0):
        st = eng.get_state(k)
        for i, life in NC.pokes_of(row):
            if i < len(st.obst_life):
                st.obst_life[i] = life
        eng.set_state(k, st)
    eng.reset()
    return eng


def _views(eng, mp, oracle_states=None):
    """Every env's state record, the first len(oracle_states) held to the oracle's."""
    views = [eng.get_state(k) for k in range(eng.N)]
    for k, ref in enumerate(oracle_states or []):
        mine = M.state_of(views[k], mp)
        assert mine["dyn"] == ref["dyn"] and mine["obst"] == ref["obst"], ("state differs from the oracle's", k)
    return views


def _model(views, static, fields, cap):
    return np.stack([NV.encode(v, static, fields, cap) for v in views])


def _same(got, want, what):
    assert got.shape == want.shape and np.array_equal(got, want), (what, np.argwhere(got != want)[:5].tolist())


# ---- 1. every row, eagerly, against the oracle --------------------------------------------------------------------------
@pytest.mark.parametrize("n", [13, 37])
@pytest.mark.parametrize("row", sorted(NC.ROWS))
def test_rows_and_fields_equal_the_model_of_the_oracles_state(row, n):
    """After the reset and after every step: zs_nav_obs of both fields at every cap of the row, each field alone, and
    (at the reset, the middle and the last step) zs_nav_field for a shuffled index list with a repeated and an
    out-of-range entry."""
    import torch
    _views_o, states, _census = NC.oracle_trace(row, 13)
    eng = _row_engine(row, n)
    mp, static = M.MapInfo(eng.builder.map), Static.of_map(eng.builder.map)
    steps = NC.steps_of(row)
    idx = [n - 1, 0, n, 5 % n, 0, -1, n // 2]  # env 0 twice; n and -1 out of range
    for t in range(steps + 1):
        if t:
            eng.gen_actions(t, 7)
            eng.step()
        views = _views(eng, mp, states[t])
        for cap in NC.caps_of(row):
            want = _model(views, static, 3, cap)
            _same(eng.nav_obs(fields=3, max_dist=cap).cpu().numpy(), want, (row, n, t, cap))
            if cap == min(NC.caps_of(row)):
                _same(eng.nav_obs(fields="objective", max_dist=cap).cpu().numpy(), want[:, :, :1], (row, n, t, cap, 1))
                _same(eng.nav_obs(fields="zombies", max_dist=cap).cpu().numpy(), want[:, :, 1:], (row, n, t, cap, 2))
        if t in (0, steps // 2, steps):
            for which in (NV.OBJECTIVE, NV.ZOMBIES):
                for cap in NC.caps_of(row):
                    out = torch.full((len(idx), static.H, static.W), 0x5A5A, dtype=torch.int16, device=eng.device).view(torch.uint16)
                    got = eng.nav_field(which, idx, out=out, max_dist=cap).cpu().numpy()
                    for j, e in enumerate(idx):
                        want = NV.field(views[e], static, which, cap) if 0 <= e < n else np.full((static.H, static.W), 0x5A5A)
                        assert np.array_equal(got[j], want), (row, n, t, which, cap, j, e)
    eng.close()


def test_a_cleared_obstacle_in_one_env_changes_that_env_alone():
    """set_state clears an obstacle of one env of the batch: the field is per env."""
    row, n = "wall5x4", 13
    eng = _row_engine(row, n)
    static = Static.of_map(eng.builder.map)
    before = eng.nav_obs(fields=3).cpu().numpy().copy()
    f_before = eng.nav_field("zombies").cpu().numpy().copy()
    st = eng.get_state(4)
    assert st.obst_present[8] == 1
    st.obst_present[8] = 0  # the wall left of the room's lower row
    eng.set_state(4, st)
    after, f_after = eng.nav_obs(fields=3).cpu().numpy(), eng.nav_field("zombies").cpu().numpy()
    others = np.arange(n) != 4
    assert np.array_equal(after[others], before[others]) and np.array_equal(f_after[others], f_before[others])
    assert not np.array_equal(f_after[4], f_before[4]) and f_before[4][2, 0] == 0xFFFF and f_after[4][2, 0] != 0xFFFF
    view = eng.get_state(4)
    _same(after[4], NV.encode(view, static, 3), "poked")
    assert np.array_equal(f_after[4], NV.field(view, static, "zombies"))
    eng.close()


# ---- 2. the bound launch under every step shape ---------------------------------------------------------------------------
@pytest.mark.parametrize("fused", [1, -1], ids=["k_step", "k_tick"])
@pytest.mark.parametrize("lanes", [1, 16, 64])
@pytest.mark.parametrize("mode", ["eager", "graph", "graph4"])
@pytest.mark.parametrize("row", ["open33x3", "crowd9x7"])
def test_bound_tensor_is_the_last_steps(row, mode, lanes, fused):
    """While a tensor is bound every step ends with the nav launch: after each launch (eager, one or four steps per graph
    launch) the bound tensor equals an eager zs_nav_obs of the same handle and the model of the oracle's state."""
    import torch
    n = 13
    _v, states, _census = NC.oracle_trace(row, n)
    eng = _row_engine(row, n, launch={"fused": fused, "fobs": -1}, lanes_per_env=lanes)
    d = eng.describe()
    assert d["lanes_per_env"] >= lanes and (d["nav_bound"], d["nav_fields"], d["nav_max_dist"]) == (0, 0, 0), d
    assert d["nav_kernel"] == "k_nav" and d["nav_envs_per_wg"] == 4 and d["nav_block"] == 256 and 0 < d["nav_lds_bytes"] <= 65536
    mp, static = M.MapInfo(eng.builder.map), Static.of_map(eng.builder.map)
    cap = min(NC.caps_of(row)) if row == "crowd9x7" else CAP
    bound = eng.nav_bind(True, 3, cap)
    d = eng.describe()
    assert (d["nav_bound"], d["nav_fields"], d["nav_max_dist"]) == (1, 3, cap)
    per = 4 if mode == "graph4" else 1
    assert NC.steps_of(row) % 4 == 0
    for t in range(per, NC.steps_of(row) + 1, per):
        if mode == "eager":
            eng.gen_actions(t, 7)
            eng.step()
        else:
            eng.step_graph(t - per + 1, 7, steps=per)
        got = bound.cpu().numpy()
        _same(got, eng.nav_obs(out=torch.zeros_like(bound)).cpu().numpy(), (row, mode, lanes, fused, t, "eager"))
        _same(got, _model(_views(eng, mp, states[t]), static, 3, cap), (row, mode, lanes, fused, t))
    eng.close()


@pytest.mark.parametrize("row", ["serpentine", "bridge_a4"])
def test_both_fields_bound_equal_each_bound_alone(row):
    """The shared loop's early exit ends no field early: serpentine's zombie queries are answered some 90 levels before
    its objective queries (test_nav_model.py asserts that in the model)."""
    n = 13
    got = {}
    for fields in (3, 1, 2):
        eng = _row_engine(row, n)
        bound = eng.nav_bind(True, fields)
        for t in range(1, 5):
            eng.step_graph(t, 7)
        got[fields] = bound.cpu().numpy().copy()
        if fields == 3:
            static = Static.of_map(eng.builder.map)
            _same(got[3], _model(_views(eng, M.MapInfo(eng.builder.map)), static, 3, CAP), row)
        eng.close()
    assert np.array_equal(got[3][:, :, :1], got[1]) and np.array_equal(got[3][:, :, 1:], got[2])
    if row == "serpentine":
        obj, zom = got[3][:, :, 0, :5].astype(int), got[3][:, :, 1, :5].astype(int)
        assert zom[zom >= 0].max() + 40 <= obj[obj >= 0].min()


def test_rebinding_and_unbinding():
    import torch
    eng = _row_engine("crowd9x7", 13)
    first = eng.nav_bind(True, "objective")
    for t in range(1, 5):
        eng.step_graph(t, 7)
    kept = first.cpu().numpy().copy()
    assert np.array_equal(kept, eng.nav_obs(out=torch.zeros_like(first)).cpu().numpy())
    second = eng.nav_bind(True, 3, 5)  # other fields and cap: the graphs are recaptured
    for t in range(5, 9):
        eng.step_graph(t, 7)
    assert np.array_equal(first.cpu().numpy(), kept)  # the first buffer is no longer written
    assert np.array_equal(second.cpu().numpy(), eng.nav_obs(out=torch.zeros_like(second)).cpu().numpy())
    assert second.shape == (13, 2, 2, 8) and eng.nav_layout() == dict(eng.nav_layout(3), fields=3)
    L = eng.nav_layout()
    assert (L["F"], L["row_words"], L["field0"], L["field1"], L["envs_per_wg"], L["block"]) == (2, 8, 0, 8, 4, 256)
    assert eng.nav_layout(2)["field1"] == -1 and eng.nav_layout(2)["F"] == 1
    eng.nav_bind(None)
    assert eng.nav is None and eng.describe()["nav_bound"] == 0
    kept = second.cpu().numpy().copy()
    for t in range(9, 13):
        eng.step_graph(t, 7)
    assert np.array_equal(second.cpu().numpy(), kept)
    eng.close()


# ---- 3. masked calls, guard bands, refusals -----------------------------------------------------------------------------
@pytest.mark.parametrize("offset", [0, 8], ids=["at16", "at16plus8"])
@pytest.mark.parametrize("fields", [1, 2, 3])
def test_guard_bands_and_masked_calls(fields, offset):
    """The buffer inside a 0x5A-filled byte tensor: nothing outside it is written, an env whose env-mask byte is 0 keeps
    its bytes, an all-zero mask writes nothing."""
    import torch
    row, n = "crowd9x7", 13
    eng = _row_engine(row, n)
    for t in range(1, 9):
        eng.gen_actions(t, 7)
        eng.step()
    F = bin(fields).count("1")
    nb = n * eng.A * F * 16
    raw = torch.full((nb + 256,), 0x5A, dtype=torch.uint8, device=eng.device)
    lo = (-raw.data_ptr()) % 16 + 64 + offset
    view = raw[lo:lo + nb].view(torch.int16).view(n, eng.A, F, 8)
    want = eng.nav_obs(fields=fields).cpu().numpy()
    for m in (torch.zeros(n), torch.ones(n), torch.arange(n) % 2, (torch.arange(n) == n - 1)):
        raw.fill_(0x5A)
        eng.nav_obs(m.to(torch.uint8).to(eng.device), out=view, fields=fields)
        got = raw.cpu().numpy()
        assert (got[:lo] == 0x5A).all() and (got[lo + nb:] == 0x5A).all()
        body = got[lo:lo + nb].view(np.int16).reshape(n, eng.A, F, 8)
        on = m.numpy().astype(bool)
        assert np.array_equal(body[on], want[on]) and (body[~on] == 0x5A5A).all()
    eng.close()


@pytest.mark.parametrize("row", ["open33x3", "crowd9x7"])
def test_full_field_guard_bands(row):
    """Frames inside a 0x5A-filled byte tensor at an odd 2-byte boundary: the bytes before the first frame, of the frames
    of out-of-range entries between the written ones, and after the last are untouched."""
    import torch
    n = 13
    eng = _row_engine(row, n)
    static = Static.of_map(eng.builder.map)
    cells = static.W * static.H
    idx = [3, n, 12, -7, 3]
    raw = torch.full((2 * cells * len(idx) + 256,), 0x5A, dtype=torch.uint8, device=eng.device)
    lo = (-raw.data_ptr()) % 16 + 64 + 2
    view = raw[lo:lo + 2 * cells * len(idx)].view(torch.uint16).view(len(idx), static.H, static.W)
    eng.nav_field("zombies", idx, out=view)
    got = raw.cpu().numpy()
    assert (got[:lo] == 0x5A).all() and (got[lo + 2 * cells * len(idx):] == 0x5A).all()
    frames = got[lo:lo + 2 * cells * len(idx)].view(np.uint16).reshape(len(idx), static.H, static.W)
    for j, e in enumerate(idx):
        want = NV.field(eng.get_state(e), static, "zombies") if 0 <= e < n else np.full((static.H, static.W), 0x5A5A)
        assert np.array_equal(frames[j], want), (row, j, e)
    eng.close()


def _too_large_map():
    """An empty map just past the plan's limit (test_nav_plan.py computes the boundary)."""
    from libzombsole_amd.maps import Map
    from test_nav_plan import env_bytes, first_refused
    W, H = first_refused()
    assert env_bytes(W, H, 1) > 65536 >= env_bytes(W, H - 1, 1)
    mk = lambda h: Map((W, h), [], [(0, 0), (1, 0)], [(5, 0), (6, 0)], [(9, 0)], "tall%d" % h)  # noqa: E731
    return mk(H), mk(H - 1)


def test_refusals():
    import torch
    eng = _row_engine("wall5x4", 5)
    buf = torch.zeros((5, eng.A, 2, 8), dtype=torch.int16, device=eng.device)
    frames = torch.zeros((5, 4, 5), dtype=torch.int16, device=eng.device).view(torch.uint16)
    L, s, p = eng.L, eng._stream(), C.c_void_p(buf.data_ptr())
    for fields in (0, 4, 7, -1):
        assert L.zs_nav_obs(eng.h, None, fields, 10, p, s) == _abi.ZS_EINVAL
        assert L.zs_nav_bind(eng.h, p, fields, 10) == _abi.ZS_EINVAL
        assert L.zs_nav_plan(eng.h, fields, (C.c_int32 * 8)()) == _abi.ZS_EINVAL
        with pytest.raises(ValueError):
            eng.nav_obs(fields=fields)
    for field in (0, 3, 4):
        assert L.zs_nav_field(eng.h, None, 5, field, 10, C.c_void_p(frames.data_ptr()), s) == _abi.ZS_EINVAL
    for cap in (0, -1, 32767, 1 << 20):
        assert L.zs_nav_obs(eng.h, None, 3, cap, p, s) == _abi.ZS_EINVAL
        assert L.zs_nav_bind(eng.h, p, 3, cap) == _abi.ZS_EINVAL
        assert L.zs_nav_field(eng.h, None, 5, 1, cap, C.c_void_p(frames.data_ptr()), s) == _abi.ZS_EINVAL
        with pytest.raises(ValueError):
            eng.nav_obs(fields=3, max_dist=cap)
    for off in (2, 4, 6):
        assert L.zs_nav_obs(eng.h, None, 3, 10, C.c_void_p(buf.data_ptr() + off), s) == _abi.ZS_EINVAL
        assert L.zs_nav_bind(eng.h, C.c_void_p(buf.data_ptr() + off), 3, 10) == _abi.ZS_EINVAL
    assert L.zs_nav_field(eng.h, None, 5, 1, 10, C.c_void_p(frames.data_ptr() + 1), s) == _abi.ZS_EINVAL
    assert L.zs_nav_field(eng.h, None, -1, 1, 10, C.c_void_p(frames.data_ptr()), s) == _abi.ZS_EINVAL
    assert L.zs_nav_obs(eng.h, None, 3, 10, None, s) == _abi.ZS_EINVAL
    assert not buf.any() and not frames.view(torch.int16).any() and eng.describe()["nav_bound"] == 0  # nothing was launched
    assert eng.nav_field("objective", []).shape == (0, 4, 5)
    viewer = _engine(NC.builder("wall5x4", 5, viewer=True))
    with pytest.raises(RuntimeError):
        viewer.nav_bind(True, 3)
    viewer.close()
    eng.close()


def test_a_map_past_the_plans_limit_is_refused_by_the_calls_not_by_create():
    import torch
    big, fits = _too_large_map()
    for mp, ok in ((big, False), (fits, True)):
        b = _abi.multi_env_config(2, "extermination", [], mp, ["0"], initial_zombies=2, minimum_zombies=2,
                                  observation_surroundings_width=5)
        eng = _engine(b)  # zs_create refuses no handle for it
        eng.seed([1, 2])
        eng.reset()
        lay = eng.nav_layout(3)
        assert (lay["envs_per_wg"], lay["block"], lay["lds_bytes"]) == ((1, 64, lay["env_bytes"]) if ok else (0, 0, 0))
        assert (lay["env_bytes"] <= 65536) == ok and eng.describe()["nav_envs_per_wg"] == (1 if ok else 0)
        if ok:
            static = Static.of_map(mp)
            _same(eng.nav_obs(fields=3).cpu().numpy(), _model([eng.get_state(k) for k in range(2)], static, 3, CAP), "fits")
            assert np.array_equal(eng.nav_field("objective", [1]).cpu().numpy()[0], NV.field(eng.get_state(1), static, 1))
        else:
            buf = torch.zeros((2, 1, 2, 8), dtype=torch.int16, device=eng.device)
            for call in (lambda: eng.nav_obs(fields=3, out=buf), lambda: eng.nav_field("objective"), lambda: eng.nav_bind(buf, 3)):
                with pytest.raises(ValueError, match="65536-byte LDS limit"):
                    call()
            assert not buf.any() and eng.nav is None
            eng.gen_actions(1, 7)
            eng.step()  # the handle steps as any other
        eng.close()


# ---- 4. a viewer; snapshot, restore and clone ---------------------------------------------------------------------------
@pytest.mark.parametrize("row", ["bridge_a4", "crowd9x7"])
def test_viewer_gives_the_source_handles_rows(row):
    import torch
    n = 13
    eng = _row_engine(row, n)
    viewer = _engine(NC.builder(row, n, viewer=True))
    for t in range(1, 7):
        eng.gen_actions(t, 7)
        eng.step()
        if t % 3:
            continue
        viewer.unpack_obs_state(eng.pack_obs_state())
        for fields, cap in ((3, CAP), (1, 7), (2, 3)):
            assert torch.equal(viewer.nav_obs(fields=fields, max_dist=cap), eng.nav_obs(fields=fields, max_dist=cap))
        assert np.array_equal(viewer.nav_field("zombies", [0, 7, 12]).cpu().numpy(), eng.nav_field("zombies", [0, 7, 12]).cpu().numpy())
    viewer.close()
    eng.close()


def test_batched_nav_restore_and_clone(tmp_path):
    """BatchedZombsole(nav=...): the tensor is current after reset, a masked reset, eager and graphed steps, restore,
    clone and load_checkpoint; a cloned env's rows equal its source's: the snapshot record holds all the search reads."""
    import torch
    from libzombsole_amd.vector import BatchedZombsole
    n = 13
    venv = BatchedZombsole("multi", n, "extermination", ["terminator"], "bridge", agent_ids=["0", "1"], initial_zombies=10,
                           minimum_zombies=4, max_episode_steps=9, base_seed=3, nav=("objective", "zombies"), nav_max_dist=60)
    eng = venv.engine
    static = Static.of_map(eng.builder.map)

    def check():
        got = venv.nav_obs.cpu().numpy()
        _same(got, _model([eng.get_state(k) for k in range(n)], static, 3, 60), "batched")
        return got

    venv.reset()
    check()
    for t in range(1, 7):
        venv.step(venv.sample_actions(t), graph=bool(t % 2))
        check()
    assert np.array_equal(venv.nav_field("zombies", [2]).cpu().numpy()[0], NV.field(eng.get_state(2), static, 2, 60))
    snap = venv.snapshot()
    ck = str(tmp_path / "ck.pt")
    venv.save_checkpoint(ck)
    at_snap = check()
    for t in range(7, 12):
        venv.step(venv.sample_actions(t))
    venv.restore(snap, src=[0, 1], dst=[4, 5])
    got = check()
    assert np.array_equal(got[[4, 5]], at_snap[[0, 1]])
    venv.clone([0, 3], [7, 8], observe=False)
    got = check()
    assert np.array_equal(got[7], got[0]) and np.array_equal(got[8], got[3])
    venv.load_checkpoint(ck)
    assert np.array_equal(check(), at_snap)
    m = torch.zeros(n, dtype=torch.uint8, device=eng.device)
    m[3] = 1
    venv.reset(m)
    check()
    venv.close()
    one = BatchedZombsole("single", 2, "safehouse", [], "maze_for_safehouse", agent_id=0, initial_zombies=3, nav="objective")
    one.reset()
    assert one.nav_obs.shape == (2, 1, 1, 8) and one.engine.nav_args == (1, 32766)
    _same(one.nav_obs.cpu().numpy(), _model([one.engine.get_state(k) for k in range(2)], Static.of_map("maze_for_safehouse"), 1, CAP),
          "maze")
    one.close()
    plain = BatchedZombsole("single", 2, "extermination", [], "bridge", agent_id=0, initial_zombies=3)
    assert plain.nav_obs is None and plain.engine.nav is None
    plain.close()


def test_drop_ins_path_distances():
    from libzombsole_amd.gym.multiagent_env import MultiagentZombsoleEnvDiscreteAction
    from libzombsole_amd.gym_env import ZombsoleGymEnvDiscreteAction
    env = MultiagentZombsoleEnvDiscreteAction("safehouse", ["terminator"], "city_for_safehouse", ["0", "1"], initial_zombies=5,
                                              device=0)
    static = Static.of_map("city_for_safehouse")
    env.reset()
    for t in range(3):
        got = env.path_distances()
        eng = env.env._core.engine
        assert got.shape == (2, 2, 8) and np.array_equal(got, NV.encode(eng.get_state(0), static, 3))
        assert np.array_equal(env.path_distances("objective", 9), NV.encode(eng.get_state(0), static, 1, 9))
        env.step({"0": int(got[0, 0, 5]) if got[0, 0, 5] >= 0 else 5, "1": 5})
    env.close()
    one = ZombsoleGymEnvDiscreteAction("extermination", [], "bridge", 0, initial_zombies=4, device=0)
    one.reset()
    got = one.path_distances()
    assert got.shape == (2, 8) and np.array_equal(got, NV.encode(one.env._core.engine.get_state(0), Static.of_map("bridge"), 3)[0])
    one.close()


# ---- 5. the two loops of INTEGRATION.md ----------------------------------------------------------------------------------
def test_shaping_and_the_greedy_follower_on_easy_exit():
    """The greedy follower (word 5 through discrete_to_triples while word 0 > 0, else heal): an agent's word 0 never
    increases from one step to the next while its env was not reset and it stays in the world — a move blocked by
    another entity leaves it where it is, which is no increase; and where it fell, it fell by exactly one, by a move the
    action mask had allowed.  easy_exit has no obstacles, so nothing else can change the field.  test_nav_model.py shows on the
    CPU, with the model and the oracle, that these seeds meet the condition and make progress."""
    import torch
    from libzombsole_amd.vector import BatchedZombsole
    n, gamma = 13, 0.99
    venv = BatchedZombsole("multi", n, "extermination", [], "easy_exit", agent_ids=["0", "1"], initial_zombies=4,
                           minimum_zombies=4, base_seed=NC.SEED0, nav="objective", action_masks=True)
    venv.reset()
    fell = 0
    for t in range(8):
        rows = venv.nav_obs[:, :, 0].clone()
        masks = venv.action_masks.clone()
        phi = -rows[:, :, 0].double()
        k = rows[:, :, 5].long()
        ids = torch.where((rows[:, :, 0] > 0) & (k >= 0), k, torch.full_like(k, 5))
        _obs, rew, _done, _trunc = venv.step(ids)
        new = venv.nav_obs[:, :, 0]
        shaped = rew + gamma * (-new[:, :, 0].double()) - phi  # r + gamma * phi(s') - phi(s)
        assert shaped.shape == (n, 2) and torch.isfinite(shaped).all()
        live = (venv.was_reset == 0)[:, None] & (rows[:, :, 7] & 1).bool() & (new[:, :, 7] & 1).bool()
        assert (new[:, :, 0][live] <= rows[:, :, 0][live]).all()
        went = live & (ids < 4) & (new[:, :, 0] < rows[:, :, 0])
        assert (new[:, :, 0][went] == rows[:, :, 0][went] - 1).all()  # one move, one level
        assert (masks.gather(2, ids.clamp(max=3)[:, :, None])[:, :, 0][went] == 1).all()  # and the mask had allowed it
        fell += int(went.sum())
    assert fell >= n
    venv.close()
