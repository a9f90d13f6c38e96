"""k_entity_obs (csrc/zs_entity_obs.hpp) through the C ABI and the Python layers: word for word against
libzombsole_amd/entity_obs.py's encode of states that equal the oracle's, on the maps of render_cases at 13 and 37 envs
and three K pairs; as a step's bound last launch under every lane count, both step kernels and graphed steps; masked,
inside guard bands, on a viewer; against k_action_mask; and the step without grid observations (grid_obs=False) against
a twin that writes them and against the oracle.

The oracle's state has no slot numbers and the key's tie-break is the slot, so the expected rows are encode of the
engine's state record (Engine.get_state) after that record's things and obstacles have been held equal to the oracle's
state of the same env and step: every value is the oracle's, the slot labels alone are the engine's."""
import numpy as np
import pytest

import entity_obs_cases as EC
import mask_model as M
from libzombsole_amd import _abi
from libzombsole_amd import entity_obs as EO

pytestmark = pytest.mark.gpu


def _engine(b, **kw):
    from libzombsole_amd.engine import Engine
    return Engine(b, **kw)


def _row_engine(row, n, launch=None, grid_obs=True, **over):
    """The engine of a row's n envs, seeded and poked as the oracle's run of it (entity_obs_cases.oracle_trace), reset."""
    b = EC.builder(row, n, **over)
    if launch:
        b.set_launch(launch)
    eng = _engine(b, grid_obs=grid_obs)
    eng.seed([EC.SEED0 + k for k in range(n)])
    for k in range(n if EC.RC.POKES.get(row) else 0):
        st = eng.get_state(k)
        for i, life in EC.RC.POKES[row]:
            if i < len(st.obst_life):
                st.obst_life[i] = life
        eng.set_state(k, st)
    eng.reset()
    return eng


def _expected(eng, mp, static, oracle_states=None, envs=None):
    """encode at (16, 16) of every env's state record, each held to the oracle's state first (when given)."""
    rows = []
    for k in (range(eng.N) if envs is None else envs):
        view = eng.get_state(k)
        if oracle_states is not None:
            mine, ref = M.state_of(view, mp), oracle_states[k]
            assert mine["dyn"] == ref["dyn"] and mine["obst"] == ref["obst"], ("state differs from the oracle's", k)
        rows.append(EO.encode(view, static, 16, 16))
    return np.stack(rows)


def _check_all_k(eng, full, what):
    for kz, kp in EC.KS:
        got = eng.entity_obs(kz=kz, kp=kp).cpu().numpy()
        want = EC.slice_rows(full, kz, kp)
        assert got.shape == want.shape and np.array_equal(got, want), (what, kz, kp, np.argwhere(got != want)[:5].tolist())


# ---- 1. every row, eagerly, against the oracle ---------------------------------------------------------------------------
@pytest.mark.parametrize("n", [13, 37])
@pytest.mark.parametrize("row", EC.ROWS)
def test_rows_equal_encode_of_the_oracles_state(row, n):
    """After the reset and after every step, at every K pair.  13 envs: every env's state is the oracle's, and the
    row's census classes are the oracle's own.  37 envs (a partial last wave of a partial last workgroup): the first 13
    are held to the oracle, the rest to the engine's record."""
    states, census = EC.oracle_trace(row, 13)
    for c in EC.REQUIRED[row]:
        assert sum(c in s for s in census) >= 3, (row, c)
    eng = _row_engine(row, n)
    mp, static = M.MapInfo(eng.builder.map), EO.Static.of_map(eng.builder.map)
    steps = EC.steps_of(row)
    for t in range(steps + 1):
        if t:
            eng.gen_actions(t, 7)
            eng.step()
        full = np.concatenate([_expected(eng, mp, static, states[t], range(13)),
                               _expected(eng, mp, static, None, range(13, n))]) if n > 13 else \
            _expected(eng, mp, static, states[t])
        _check_all_k(eng, full, (row, n, t))
    eng.close()


# ---- 2. the bound launch under every step shape -----------------------------------------------------------------------------
BOUND_ROWS = ("field9x7", "fort_e132", "bridge_a4", "wall5x4")  # E <= 64; a second lane pass; 4 agents + 2 bots; `short`


@pytest.mark.parametrize("fused", [1, -1], ids=["k_step", "k_tick"])
@pytest.mark.parametrize("lanes", [1, 16, 64])
@pytest.mark.parametrize("mode", ["eager", "graph", "graph4"])
@pytest.mark.parametrize("kz,kp", EC.KS)
@pytest.mark.parametrize("row", BOUND_ROWS)
def test_bound_tensor_is_the_last_steps(row, kz, kp, mode, lanes, fused):
    """While a tensor is bound every step ends with the entity launch: after each launch of the row's steps (eager,
    one or four steps per graph launch) the bound tensor is encode of the state the oracle has at that step."""
    n = 13
    states, _census = EC.oracle_trace(row, n)
    eng = _row_engine(row, n, launch={"fused": fused, "fobs": -1}, lanes_per_env=lanes)
    d = eng.describe()
    # lanes_per_env is where the planner starts (it doubles G until the envs' LDS images fit, zs_step_plan.hpp
    # step_layout) and a fused launch needs the reset image to fit too: field9x7 (E = 10) takes every requested shape
    # exactly; the larger rows run under the shape the planner grants for the request
    assert d["lanes_per_env"] >= lanes and d["step_kernel"] in ("k_step", "k_tick"), d
    if row == "field9x7":
        assert d["lanes_per_env"] == lanes and d["step_kernel"] == ("k_step" if fused > 0 else "k_tick"), d
    assert d["entity_obs_bound"] == 0 and d["entity_kz"] == 0
    mp, static = M.MapInfo(eng.builder.map), EO.Static.of_map(eng.builder.map)
    bound = eng.bind_entity_obs(True, kz, kp)
    d = eng.describe()
    assert (d["entity_obs_bound"], d["entity_kz"], d["entity_kp"]) == (1, kz, kp)
    per = 4 if mode == "graph4" else 1
    assert EC.steps_of(row) % 4 == 0
    for t in range(per, EC.steps_of(row) + 1, per):
        if mode == "eager":
            eng.gen_actions(t, 7)
            eng.step()
        else:
            eng.step_graph(t - per + 1, 7, steps=per)
        want = EC.slice_rows(_expected(eng, mp, static, states[t]), kz, kp)
        got = bound.cpu().numpy()
        assert np.array_equal(got, want), (row, kz, kp, mode, lanes, fused, t, np.argwhere(got != want)[:5].tolist())
    eng.close()


def test_rebinding_and_unbinding():
    import torch
    row, n = "bridge64", 13
    eng = _row_engine(row, n)
    first = eng.bind_entity_obs(True, 4, 1)
    for t in range(1, 5):
        eng.step_graph(t, 7)
    kept = first.cpu().numpy().copy()
    assert np.array_equal(kept, eng.entity_obs(out=torch.zeros_like(first)).cpu().numpy())
    second = eng.bind_entity_obs(True, 16, 16)  # other K values: the graphs are recaptured
    for t in range(5, 9):
        eng.step_graph(t, 7)
    assert np.array_equal(first.cpu().numpy(), kept)  # the first buffer is no longer written
    assert np.array_equal(second.cpu().numpy(), eng.entity_obs(out=torch.zeros_like(second)).cpu().numpy())
    assert second.shape == (n, 2, 16 + 4 * 32) and eng.entity_layout()["row_bytes"] == 2 * second.shape[2]
    eng.bind_entity_obs(None)
    assert eng.entities is None and eng.describe()["entity_obs_bound"] == 0
    kept = second.cpu().numpy().copy()
    for t in range(9, 13):
        eng.step_graph(t, 7)
    assert np.array_equal(second.cpu().numpy(), kept)
    eng.close()


# ---- 3. masked calls, guard bands, refusals ---------------------------------------------------------------------------------
@pytest.mark.parametrize("offset", [0, 8], ids=["at16", "at16plus8"])
@pytest.mark.parametrize("kz,kp", EC.KS)
def test_guard_bands_and_masked_calls(kz, kp, offset):
    """The buffer inside a 0x5A-filled byte tensor: nothing outside it is written, an env whose env-mask byte is 0
    keeps its bytes, an all-zero mask writes nothing."""
    import torch
    row, n = "crowd9x7", 13
    eng = _row_engine(row, n)
    for t in range(1, 9):
        eng.gen_actions(t, 7)
        eng.step()
    words = 16 + 4 * (kz + kp)
    nb = n * eng.A * words * 2
    raw = torch.full((nb + 256,), 0x5A, dtype=torch.uint8, device=eng.device)
    lo = (-raw.data_ptr()) % 16 + 64 + offset
    view = raw[lo:lo + nb].view(torch.int16).view(n, eng.A, words)
    want = eng.entity_obs(kz=kz, kp=kp).cpu().numpy()
    for m in (torch.zeros(n), torch.ones(n), torch.arange(n) % 2, (torch.arange(n) == n - 1)):
        raw.fill_(0x5A)
        eng.entity_obs(m.to(torch.uint8).to(eng.device), out=view, kz=kz, kp=kp)
        got = raw.cpu().numpy()
        assert (got[:lo] == 0x5A).all() and (got[lo + nb:] == 0x5A).all()
        body = got[lo:lo + nb].view(np.int16).reshape(n, eng.A, words)
        on = m.numpy().astype(bool)
        assert np.array_equal(body[on], want[on]) and (body[~on] == 0x5A5A).all()
    eng.close()


def test_refusals():
    import ctypes as C
    import torch
    eng = _row_engine("wall5x4", 5)
    buf = torch.zeros((5, eng.A, 36), dtype=torch.int16, device=eng.device)
    L, s = eng.L, eng._stream()
    for kz, kp in ((0, 0), (17, 1), (4, -1), (4, 17)):
        assert L.zs_entity_obs(eng.h, None, kz, kp, C.c_void_p(buf.data_ptr()), s) == _abi.ZS_EINVAL
        assert L.zs_entity_obs_bind(eng.h, C.c_void_p(buf.data_ptr()), kz, kp) == _abi.ZS_EINVAL
        assert L.zs_entity_obs_layout(eng.h, kz, kp, (C.c_int32 * 8)()) == _abi.ZS_EINVAL
        with pytest.raises(ValueError):
            eng.entity_obs(kz=kz, kp=kp)
    for off in (2, 4, 6):
        assert L.zs_entity_obs(eng.h, None, 4, 1, C.c_void_p(buf.data_ptr() + off), s) == _abi.ZS_EINVAL
        assert L.zs_entity_obs_bind(eng.h, C.c_void_p(buf.data_ptr() + off), 4, 1) == _abi.ZS_EINVAL
    assert L.zs_entity_obs(eng.h, None, 4, 1, None, s) == _abi.ZS_EINVAL
    with pytest.raises(ValueError):
        eng.entity_obs(out=buf.view(-1)[2:2 + 5 * eng.A * 36 - 4].view(-1), kz=4, kp=1)
    assert eng.describe()["entity_obs_bound"] == 0
    assert eng.entity_layout(4, 1) == dict(_abi.entity_layout(4, 1), kz=4, kp=1)
    viewer = _engine(EC.builder("wall5x4", 5, viewer=True))
    with pytest.raises(RuntimeError):
        viewer.bind_entity_obs(True, 4, 1)
    viewer.close()
    eng.close()


# ---- 4. a viewer, and the action masks --------------------------------------------------------------------------------------
@pytest.mark.parametrize("row", ["bridge_a4", "fort_e132"])
def test_viewer_and_action_mask_cross_check(row):
    """A viewer fed by pack / unpack gives the same tensor; bit 1 of zombie row 0 is action-mask byte 4 of every
    present agent (k_action_mask's range test, written on its own)."""
    import torch
    n = 13
    eng = _row_engine(row, n)
    viewer = _engine(EC.builder(row, n, viewer=True))
    for t in range(1, 11):
        eng.gen_actions(t, 7)
        eng.step()
        if t % 3:
            continue
        viewer.unpack_obs_state(eng.pack_obs_state())
        for kz, kp in EC.KS:
            mine = eng.entity_obs(kz=kz, kp=kp)
            assert torch.equal(viewer.entity_obs(kz=kz, kp=kp), mine)
            masks = eng.action_mask().cpu().numpy()
            rows = mine.cpu().numpy()
            present = rows[:, :, 0] == 1
            assert np.array_equal(((rows[:, :, 8 + 3] >> 1) & 1)[present], masks[:, :, 4][present])
            assert not rows[~present].any() and not masks[~present].any()
    viewer.close()
    eng.close()


# ---- 5. the step without grid observations ----------------------------------------------------------------------------------
NO_GRID = {"fused": {"fused": 1, "fobs": -1}, "side_stream": {"fused": -1, "fobs": -1},
           "fobs": {"fobs": 1}, "deferred_respawn": {"defer_respawn": 1, "fused": -1, "fobs": -1}}


@pytest.mark.parametrize("shape", sorted(NO_GRID))
def test_step_without_grid_observations(shape):
    """grid_obs=False passes a null obs_dev to every step, graphed step and reset: rewards, done, trunc, listed,
    was_reset and the full snapshot records equal a twin's that writes the grid, through autoresets and a masked
    reset, and the states are the oracle's; describe() names the tail as the step's last launch."""
    import torch
    row, n = "field9x7", 13
    states, _census = EC.oracle_trace(row, n)
    launch = NO_GRID[shape]
    twin = _row_engine(row, n, launch=launch)
    eng = _row_engine(row, n, launch=launch, grid_obs=False)
    d, dt = eng.describe(), twin.describe()
    assert d == dt and d["step_tail_launch"] == ""  # the plan does not depend on the buffer; nothing stepped yet
    if shape == "fused":
        assert d["step_kernel"] == "k_step"
    if shape == "side_stream":
        assert d["step_kernel"] == "k_tick" and d["reset_side_stream"] == 1
    if shape == "fobs":
        assert d["obs_kernel"] == "step launch"
    if shape == "deferred_respawn":
        assert d["respawn"] == "k_respawn"
    assert eng.obs is None and eng.out.obs is None and twin.obs is not None
    ent = eng.bind_entity_obs(True, 4, 1)
    mp, static = M.MapInfo(eng.builder.map), EO.Static.of_map(eng.builder.map)

    def same(t):
        for name in ("rewards", "done", "trunc", "listed", "was_reset"):
            assert torch.equal(getattr(eng, name), getattr(twin, name)), (shape, t, name)
        assert torch.equal(eng.snapshot(), twin.snapshot()), (shape, t)

    resets = 0
    for t in range(1, 25):
        for e in (eng, twin):
            if t <= 12:
                e.gen_actions(t, 7)
                e.step()
            else:
                e.step_graph(t, 7)
        same(t)
        resets += int(eng.was_reset.sum())
        want = EC.slice_rows(_expected(eng, mp, static, states[t]), 4, 1)
        assert np.array_equal(ent.cpu().numpy(), want), (shape, t)
    assert resets >= n  # autoresets went through the null-pointer paths
    # the launch that carried the tail, eagerly and as captured: k_tail without a buffer; with one, the observation
    # kernel unless the step launch writes the observations itself
    assert eng.describe()["step_tail_launch"] == "k_tail"
    tail = twin.describe()["step_tail_launch"]
    assert tail == ("k_tail" if shape == "fobs" else twin.describe()["obs_kernel"]) and tail != ""
    assert eng.step()[0] is None
    twin.step()
    same(25)
    m = torch.zeros(n, dtype=torch.uint8, device=eng.device)
    m[[2, 5, 12]] = 1
    assert eng.reset(m) is None
    twin.reset(m)
    assert torch.equal(eng.snapshot(), twin.snapshot())
    for t in range(26, 30):
        for e in (eng, twin):
            e.step_graph(t, 7)
        same(t)
    with pytest.raises(ValueError):
        eng.observe()
    eng.close()
    twin.close()


def test_host_step_ends_with_the_bound_launch():
    """zs_host_step is zs_step: a bound tensor follows the drop-ins' per-call path too."""
    import torch
    eng = _row_engine("wall5x4", 1)
    ent = eng.bind_entity_obs(True, 4, 1)
    rec = eng.host_record()
    from libzombsole_amd.actions import DISCRETE_TRIPLES
    acts = np.stack([DISCRETE_TRIPLES[5]] * eng.A)[None]  # heal
    eng.host_step(acts, None, rec)
    assert torch.equal(ent, eng.entity_obs(out=torch.zeros_like(ent)))
    assert ent[0, 0, 0] == 1
    eng.close()


# ---- 6. the Python layers ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("grid", [True, False], ids=["grid", "no_grid"])
def test_batched_entity_obs(tmp_path, grid):
    """BatchedZombsole(entity_obs=(4, 1)): the tensor is current after reset, a masked reset, eager and graphed steps,
    restore, clone and load_checkpoint; with grid_obs=False it is the observation every call returns."""
    import torch
    from libzombsole_amd.vector import BatchedZombsole
    n = 13
    venv = BatchedZombsole("multi", n, "extermination", [], "bridge", agent_ids=["0", "1"], initial_zombies=10,
                           minimum_zombies=4, max_episode_steps=9, base_seed=3, entity_obs=(4, 1), grid_obs=grid)
    eng = venv.engine
    static = EO.Static.of_map(eng.builder.map)

    def check():
        got = venv.entity_obs.cpu().numpy()
        want = np.stack([EO.encode(eng.get_state(k), static, 4, 1) for k in range(n)])
        assert got.shape == (n, 2, 36) and np.array_equal(got, want)
        return got

    obs = venv.reset()
    assert (obs is venv.entity_obs) == (not grid) and (venv.obs is None) == (not grid)
    check()
    for t in range(1, 7):
        obs = venv.step(venv.sample_actions(t), graph=bool(t % 2))[0]
        assert (obs is venv.entity_obs) == (not grid)
        check()
    snap = venv.snapshot()
    ck = str(tmp_path / "ck.pt")
    venv.save_checkpoint(ck)
    at_snap = check()
    for t in range(7, 12):
        venv.step(venv.sample_actions(t))
    back = venv.restore(snap, src=[0, 1], dst=[4, 5])
    assert (back is venv.entity_obs) == (not grid)
    check()
    venv.clone([0], [7], observe=False)
    check()
    venv.load_checkpoint(ck)
    assert np.array_equal(check(), at_snap)
    m = torch.zeros(n, dtype=torch.uint8, device=eng.device)
    m[3] = 1
    venv.reset(m)
    check()
    venv.close()
    plain = BatchedZombsole("single", 2, "extermination", [], "bridge", agent_id=0, initial_zombies=3)
    assert plain.entity_obs is None and plain.engine.entities is None and plain.obs is not None
    plain.close()
    with pytest.raises(ValueError):
        BatchedZombsole("single", 2, "extermination", [], "bridge", agent_id=0, initial_zombies=3, grid_obs=False)
