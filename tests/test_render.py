"""zs_render on the GPU: the engine replayed through the recorded render_* fixtures (every call's frame hash is the
reference's), k_render and k_render_track against render.compose over steps with autoresets on the maps of
render_cases.ROWS, the index-list and guard-band contract, resets, snapshots, clones, checkpoints, an uploaded atlas,
and the refusals."""
import numpy as np
import pytest

import golden_util as G
import render_cases as RC
from libzombsole_amd import _abi
from libzombsole_amd import render as R

pytestmark = pytest.mark.gpu


def _engine(b):
    from libzombsole_amd.engine import Engine
    return Engine(b)


def _frames(eng, envs=None):
    import torch
    f = eng.render(envs)
    torch.cuda.synchronize()
    return f.cpu().numpy()


@pytest.mark.parametrize("name", RC.FIXTURES)
def test_engine_frames_match_the_reference(name):
    import torch
    fx = G.load_fixture(name)
    runs = fx["runs"]
    b = G.builder_for(fx, num_envs=len(runs))
    b.cfg.flags |= _abi.FLAG_RENDER | _abi.FLAG_DEATH_LOG
    eng = _engine(b)
    eng.seed([r["seed"] for r in runs])
    eng.reset()
    for i in range(len(runs[0]["calls"])):
        if i > 0:
            acts = np.zeros((len(runs), eng.A, 3), dtype=np.int32)
            for k, r in enumerate(runs):
                if r["calls"][i]["kind"] == "step":
                    acts[k] = G.action_triples(fx, r["calls"][i], eng.A)[:eng.A]
            eng.actions.copy_(torch.from_numpy(acts))
            eng.step()
        fr = _frames(eng)
        for k, r in enumerate(runs):
            assert RC.frame_hash(fr[k]) == r["render"][i]["hash"], (name, r["seed"], i)
    eng.close()


class Tracked(object):
    """An engine with the expected body colours kept on the host from its own death logs (test_logs.py holds those to
    the oracle), and the frame compose gives for each env."""

    def __init__(self, b, seeds):
        self.eng = _engine(b)
        self.eng.seed(seeds)
        self.eng.reset()
        W, H = b.map.size
        self.colors = R.slot_colors(b.num_agents, list(b.cfg.bot_types[:b.num_bots]), self.eng.E - b.num_agents - b.num_bots)
        self.bodies = [RC.BodyColors(W, H, self.colors) for _ in seeds]
        self.t = 0

    def step(self):
        import torch
        self.t += 1
        self.eng.gen_actions(self.t, self.eng.n_discrete)
        self.eng.step()
        torch.cuda.synchronize()
        was_reset = self.eng.was_reset.cpu().numpy()
        for k, bc in enumerate(self.bodies):
            if was_reset[k]:
                bc.reset()
            else:
                bc.deaths(self.eng.death_log(k))
        return was_reset

    def expected(self, k, atlas=None):
        return R.compose_state(self.eng.builder.map, self.eng.get_state(k), self.colors, self.bodies[k].row, atlas)

    def check(self, where):
        fr = _frames(self.eng)
        for k in range(self.eng.N):
            assert np.array_equal(fr[k], self.expected(k)), (where, k, self.t)
        return fr


def _row_engine(row, n, **over):
    """The engine of a row's n envs, seeded and poked as the oracle's run of it (render_cases.oracle_trace), reset."""
    launch = over.pop("launch", None)
    b = RC.ROWS[row](n, **over)
    if launch:
        b.set_launch(launch)
    eng = _engine(b)
    eng.seed([RC.SEED0 + k for k in range(n)])
    for k in range(n if RC.POKES.get(row) else 0):
        st = eng.get_state(k)
        for i, life in RC.POKES[row]:
            if i < len(st.obst_life):
                st.obst_life[i] = life
        eng.set_state(k, st)
    eng.reset()
    return eng


def _against_oracle(row, n, per_launch=0, every=1, **over):
    """The row's engine stepped through the oracle's run: per_launch 0 eager steps, else graph launches of that many
    steps; the engine's frames equal the oracle-side frames (state and death log of the oracle alone through compose)
    after the reset and after every `every` steps.  The census says the run holds what the row is relied on for."""
    steps = RC.steps_of(row)
    every = max(every, per_launch, 1)
    assert every % max(per_launch, 1) == 0 and steps % max(per_launch, 1) == 0
    expected, census = RC.oracle_trace(row, n, steps, True, every)
    for c in RC.REQUIRED[row]:
        assert sum(c in s for s in census) >= 3, (row, c)
    eng = _row_engine(row, n, **over)
    t = 0

    def check():
        fr = _frames(eng)
        for k in range(n):
            assert np.array_equal(fr[k], expected[t][k]), (row, n, k, t)
    check()
    while t < steps:
        if per_launch:
            eng.step_graph(t + 1, eng.n_discrete, steps=per_launch)
            t += per_launch
        else:
            t += 1
            eng.gen_actions(t, eng.n_discrete)
            eng.step()
        if expected[t][0] is not None:
            check()
    eng.close()


@pytest.mark.parametrize("n", [13, 37])
@pytest.mark.parametrize("row", ["field9x7", "safe8x5", "strip70x1", "strip1x70", "wall5x4", "crowd9x7"])
def test_kernel_against_oracle_small_maps(row, n):
    _against_oracle(row, n)


@pytest.mark.parametrize("n", [13, 37])
@pytest.mark.parametrize("row", ["bridge64", "fort_e132"])
def test_kernel_against_oracle_large_maps(row, n):
    eng = _row_engine(row, 2)
    d = eng.describe()
    assert d["render"] == 1 and d["render_block"] == 256 and (row != "bridge64" or d["render_grid"] == 16)
    eng.close()
    _against_oracle(row, n, every=6)


@pytest.mark.parametrize("lanes,fused", [(1, 0), (16, 0), (64, 0), (16, 1), (16, -1), (0, -1)])
def test_tracker_under_every_lane_count_and_both_step_kernels(lanes, fused):
    """G = 1, 16, 64 under the plan's own choice of step kernel, and k_step (fused 1) and k_tick (fused -1) forced."""
    _against_oracle("crowd9x7", 13, every=8, lanes_per_env=lanes, launch={"fused": fused} if fused else None)


@pytest.mark.parametrize("row", ["bridge64", "fort_e132"])
def test_unfused_step_on_the_large_maps(row):
    _against_oracle(row, 13, every=12, launch={"fused": -1})


@pytest.mark.parametrize("per_launch", [1, 4])
@pytest.mark.parametrize("row", ["crowd9x7", "bridge64", "fort_e132"])
def test_graph_launches_track_every_step(row, per_launch):
    _against_oracle(row, 13, per_launch=per_launch, every=4)


def test_poked_obstacle_and_poked_body():
    """zs_set_state: a present obstacle with life <= 0 is drawn; a body poked onto a cell without a death is green."""
    eng = _row_engine("field9x7", 3)
    m = eng.builder.map
    W, H = m.size
    colors = R.slot_colors(eng.A, list(eng.builder.cfg.bot_types[:eng.builder.num_bots]), eng.E - eng.A - eng.builder.num_bots)
    for k in range(3):
        st = eng.get_state(k)
        st.obst_life[k] = -3 - k
        taken = {(o[0], o[1]) for o in m.obstacles} | {(int(r[2]), int(r[3])) for r in st.ent if r[1]}
        cell = next(c for c in range(W * H) if (c % W, c // W) not in taken)
        assert cell < 31
        st.dead_words[0] |= 1 << cell
        eng.set_state(k, st)
    fr = _frames(eng)
    for k in range(3):
        st = eng.get_state(k)
        assert st.obst_present[k] and st.obst_life[k] <= 0 and len(st.dead_cells()) == 1
        exp = R.compose_state(m, st, colors)  # no colour recorded: green
        assert np.array_equal(fr[k], exp), k
        x, y = st.dead_cells()[0] % W, st.dead_cells()[0] // W
        assert (fr[k][10 * y + 5, 10 * x + 5] == [0, 128, 0]).all(), "the body's centre pixel (both diagonals) is green"
    eng.close()


def test_index_lists_guard_bands_and_n_zero():
    import torch
    n = 5
    tr = Tracked(RC.ROWS["field9x7"](n), list(range(n)))
    for _ in range(8):
        tr.step()
    full = tr.check("all")
    eng = tr.eng
    fb = eng.render_layout()["frame_bytes"]
    assert fb == full[0].size
    idx = [4, 4, 0, -1, 3, 2, 1, 0, n, 2 ** 30]  # repeats, reversed order, entries that are no env
    got = _frames(eng, idx)
    for k, e in enumerate(idx):
        assert np.array_equal(got[k], full[e] if 0 <= e < n else np.zeros_like(full[0])), (k, e)
    # fewer frames than entries: only the buffer's frames are drawn; every byte around them stays
    for shift in (0, 1, 7):
        buf = torch.full((16 + 3 * fb + 64,), 0x5A, dtype=torch.uint8, device=eng.device)
        base = (-buf.data_ptr()) % 16 + shift
        out = buf[base:base + 3 * fb].view(3, *full[0].shape)
        assert out.data_ptr() % 16 == shift
        eng.render(torch.tensor([2, 99, 1, 0, 3], dtype=torch.int32, device=eng.device), out=out)
        torch.cuda.synchronize()
        h = buf.cpu().numpy()
        assert (h[:base] == 0x5A).all() and (h[base + 3 * fb:] == 0x5A).all(), shift
        fr = h[base:base + 3 * fb].reshape(3, *full[0].shape)
        assert np.array_equal(fr[0], full[2]) and (fr[1] == 0x5A).all() and np.array_equal(fr[2], full[1]), shift
    buf = torch.full((fb,), 0x5A, dtype=torch.uint8, device=eng.device)
    eng.render(torch.zeros(0, dtype=torch.int32, device=eng.device), out=buf.view(1, *full[0].shape))
    rc = eng.L.zs_render(eng.h, None, 0, None, 0, None)
    torch.cuda.synchronize()
    assert rc == 0 and (buf.cpu().numpy() == 0x5A).all()
    eng.close()


def _run_until_bodies(tr, steps=16):
    for _ in range(steps):
        tr.step()
    assert sum(bc.seen for bc in tr.bodies) > 0
    return tr.check("run")


def test_masked_reset_clears_exactly_the_masked_envs():
    import torch
    n = 6
    tr = Tracked(RC.ROWS["safe8x5"](n, max_episode_steps=0, autoreset=False), list(range(30, 30 + n)))
    _run_until_bodies(tr)
    mask = torch.tensor([1, 0, 1, 0, 0, 1], dtype=torch.uint8, device=tr.eng.device)
    tr.eng.reset(mask)
    for k in range(n):
        if mask[k]:
            tr.bodies[k].reset()
    tr.check("masked reset")
    tr.step()
    tr.check("step after")
    tr.eng.close()


def test_snapshot_restore_clone_and_checkpoint(tmp_path):
    import torch
    from libzombsole_amd.vector import BatchedZombsole
    kw = dict(rules_name="extermination", player_names=["sniper", "hamster"], map_name=G.map_path("field9x7"),
              agent_ids=["0", "1"], initial_zombies=6, minimum_zombies=4, max_episode_steps=0, render=True)
    env = BatchedZombsole("multi", 6, base_seed=40, **kw)
    env.reset()
    eng = env.engine
    for t in range(1, 17):  # under these seeds a bot or an agent has died in four of the envs by step 15 (oracle)
        eng.gen_actions(t, 7)
        eng.step()
    before = _frames(eng)
    L = eng.render_layout()
    assert L["body_col"] == eng.builder.snapshot_layout()["body_col"] and L["body_bytes"] == 64
    snap = env.snapshot()
    path = str(tmp_path / "ck.pt")
    env.save_checkpoint(path)
    body = snap.view(torch.uint8).reshape(6, -1)[:, L["body_col"]:L["body_col"] + L["body_bytes"]].cpu().numpy()
    assert body.any(), "the records carry body colours"
    for t in range(17, 29):
        eng.gen_actions(t, 7)
        eng.step()
    assert not np.array_equal(_frames(eng), before)
    env.restore(snap)
    assert np.array_equal(_frames(eng), before)
    # a clone into a handle with another env count: env 4's world and colours in every env of the other
    other = BatchedZombsole("multi", 3, **kw)
    other.reset()
    rec = eng.snapshot(torch.tensor([4], dtype=torch.int32, device=eng.device))
    other.engine.restore(rec, src=torch.zeros(3, dtype=torch.int32, device=eng.device),
                         dst=torch.arange(3, dtype=torch.int32, device=eng.device))
    fo = _frames(other.engine)
    assert all(np.array_equal(fo[k], before[4]) for k in range(3))
    for t in range(30, 36):
        eng.gen_actions(t, 7)
        eng.step()
    env.load_checkpoint(path)
    assert np.array_equal(_frames(eng), before)
    env.close()
    other.close()


def test_uploaded_atlas_changes_exactly_its_colours():
    tr = Tracked(RC.ROWS["field9x7"](4), [1, 2, 3, 4])
    base = _run_until_bodies(tr)
    masks, palette = R.default_atlas()
    swapped = palette.copy()
    swapped[[R.BLUE, R.YELLOW]] = palette[[R.YELLOW, R.BLUE]]
    tr.eng.set_render_atlas(masks, swapped)
    got = _frames(tr.eng)
    for k in range(4):
        assert np.array_equal(got[k], tr.expected(k, (masks, swapped)))
    blue, yellow = (base == palette[R.BLUE]).all(-1), (base == palette[R.YELLOW]).all(-1)
    assert blue.any() and yellow.any()
    assert (got[blue] == palette[R.YELLOW]).all() and (got[yellow] == palette[R.BLUE]).all()
    assert np.array_equal(got[~(blue | yellow)], base[~(blue | yellow)])
    tr.eng.close()


def test_unflagged_steps_equal_flagged_steps():
    import torch
    outs = []
    for render in (False, True):
        eng = _engine(RC.ROWS["field9x7"](13, render=render))
        eng.seed(list(range(13)))
        eng.reset()
        rows = []
        for t in range(1, 25):
            eng.gen_actions(t, 7)
            eng.step()
            torch.cuda.synchronize()
            rows.append([eng.obs.cpu().numpy().copy(), eng.rewards.cpu().numpy().copy(), eng.done.cpu().numpy().copy(),
                         eng.trunc.cpu().numpy().copy(), eng.was_reset.cpu().numpy().copy()])
        outs.append(rows)
        eng.close()
    for a, b in zip(*outs):
        assert all(np.array_equal(x, y) for x, y in zip(a, b))


def test_refusals():
    from libzombsole_amd.engine import Engine, EngineError
    plain = _engine(RC.ROWS["field9x7"](2, render=False))
    for call in (plain.render_layout, plain.render, lambda: plain.set_render_atlas(*R.default_atlas())):
        with pytest.raises(EngineError, match="ZS_FLAG_RENDER"):
            call()
    assert plain.describe()["render"] == 0 and plain.describe()["render_grid"] == 0
    plain.close()
    b = RC.ROWS["field9x7"](2)
    b.cfg.flags &= ~_abi.FLAG_DEATH_LOG
    with pytest.raises(ValueError, match="ZS_FLAG_DEATH_LOG"):
        Engine(b)
    v = RC.ROWS["field9x7"](2, viewer=True)
    with pytest.raises(EngineError, match="viewer"):
        Engine(v)
    viewer = _engine(RC.ROWS["field9x7"](2, render=False, viewer=True))
    with pytest.raises(EngineError, match="ZS_FLAG_RENDER"):
        viewer.render()
    viewer.close()
