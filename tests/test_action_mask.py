"""k_action_mask (csrc/zs_mask.hpp) through the C ABI and the Python layers: against the reference's own masks
(tests/golden/masks_*.json.gz), against the host model (mask_model.py, pinned to those fixtures on the CPU by
test_mask_model.py) on larger shapes, as a step's bound last launch, inside guard bands, and as an addition that
leaves an unbound handle's outputs alone."""
import numpy as np
import pytest

import golden_util as G
import mask_census as C
import mask_model as M
from libzombsole_amd import _abi

pytestmark = pytest.mark.gpu


def _engine(b):
    from libzombsole_amd.engine import Engine
    return Engine(b)


def _model_masks(eng, mp, envs=None):
    nd = eng.n_discrete
    return np.array([M.masks(M.state_of(eng.get_state(k), mp), mp, eng.A, nd)
                     for k in (range(eng.N) if envs is None else envs)], dtype=np.uint8)


# ---- 1. the reference's masks --------------------------------------------------------------------------------
@pytest.mark.parametrize("name", C.mask_fixture_names())
def test_masks_equal_the_reference(name):
    """The engine driven through a mask fixture's calls (every seed one env, next-step autoreset): after every
    call the standalone launch's masks are the reference's."""
    import torch
    fx = G.load_fixture(name)
    runs = fx["runs"]
    n = len(runs)
    eng = _engine(G.builder_for(fx, num_envs=n))
    eng.seed([r["seed"] for r in runs])
    for k in range(n if G.obstacle_pokes(fx) else 0):
        st = eng.get_state(k)
        for i, life in G.obstacle_pokes(fx):
            st.obst_life[i] = life
        eng.set_state(k, st)
    eng.reset()
    for i in range(len(runs[0]["calls"])):
        if i > 0:
            acts = np.stack([G.action_triples(fx, r["calls"][i], eng.A)[:eng.A] if r["calls"][i]["kind"] == "step"
                             else np.zeros((eng.A, 3), np.int32) for r in runs])
            eng.actions.copy_(torch.from_numpy(acts))
            eng.step()
        got = eng.action_mask().cpu().numpy()
        for k, r in enumerate(runs):
            assert got[k].tolist() == r["masks"][i], (name, r["seed"], i, got[k].tolist())
    eng.close()


# ---- 2. the host model on larger shapes -----------------------------------------------------------------------
def _bridge(n):
    return _abi.multi_env_config(n, "extermination", [], "bridge", ["0", "1"], initial_zombies=10, minimum_zombies=4,
                                 max_episode_steps=9)


def _fort(n):  # E = 132 slots: three passes of the wave; A = 32: two ballots of destinations
    return _abi.multi_env_config(n, "extermination", [], "fort", [str(i) for i in range(32)], initial_zombies=100,
                                 minimum_zombies=0, max_episode_steps=10)


def _bridge64(n):
    return _abi.multi_env_config(n, "extermination", [], "bridge64", ["0", "1"], initial_zombies=10,
                                 minimum_zombies=0, max_episode_steps=7)


def _bridge64_respawn(n):  # zombies kept at 6: respawns most steps, resets every sixth
    return _abi.multi_env_config(n, "extermination", [], "bridge64", ["0", "1"], initial_zombies=10,
                                 minimum_zombies=6, max_episode_steps=6)


def _city128(n):
    return _abi.multi_env_config(n, "safehouse", [], "city128", ["0", "1", "2", "3"], initial_zombies=50,
                                 minimum_zombies=50, max_episode_steps=11)


def _wall(n):
    return _abi.multi_env_config(n, "survival", [], G.map_path("wall_hp"), ["0", "1"], initial_zombies=0,
                                 minimum_zombies=0, agent_weapons=["knife", "shotgun"], max_episode_steps=5)


def _single(n):  # six ids: entry 6 stays 0
    return _abi.single_env_config(n, "extermination", ["terminator"], "bridge", 0, initial_zombies=10,
                                  minimum_zombies=6, agent_weapon="shotgun", max_episode_steps=8)


DIFF = {"bridge_13": (_bridge, 13, None), "bridge_37": (_bridge, 37, None),
        "bridge64_37_respawn_fused": (_bridge64_respawn, 37, {"defer_respawn": 1, "fused": 1}),
        "bridge64_13_respawn_unfused": (_bridge64_respawn, 13, {"defer_respawn": 1, "fused": -1}),
        "fort_13": (_fort, 13, None), "bridge64_37": (_bridge64, 37, None), "city128_13": (_city128, 13, None),
        "wall5x4_37": (_wall, 37, None), "single_bridge_13": (_single, 13, None)}


@pytest.mark.parametrize("row", sorted(DIFF))
def test_masks_equal_the_model(row):
    """Seeded runs of 24 steps with autoresets; every env, every step, the reset call included."""
    make, n, launch = DIFF[row]
    b = make(n)
    if launch:
        b.set_launch(dict(launch, fobs=-1))
    eng = _engine(b)
    if launch:
        d = eng.describe()
        assert d["respawn"] == "k_respawn" and d["step_kernel"] == ("k_step" if launch["fused"] > 0 else "k_tick"), d
    mp = M.MapInfo(b.map)
    eng.seed([4000 + i for i in range(n)])
    eng.reset()
    resets = 0
    for t in range(25):
        if t:
            eng.gen_actions(t, eng.n_discrete)
            eng.step()
            resets += int(eng.was_reset.sum())
        got = eng.action_mask().cpu().numpy()
        want = _model_masks(eng, mp)
        assert np.array_equal(got, want), (row, t, np.argwhere(got != want)[:5].tolist())
    assert resets >= n  # every env's masks followed an autoreset on average
    eng.close()


def test_masks_of_poked_states():
    """Obstacles gone and obstacles present with a life below zero, one and all of them, set by zs_set_state: the
    masks against the model, and the wall above agent 0 spelled out."""
    b = _abi.multi_env_config(5, "survival", [], G.map_path("wall_hp"), ["0", "1"], initial_zombies=1,
                              minimum_zombies=1, agent_weapons=["knife", "shotgun"])
    eng = _engine(b)
    mp = M.MapInfo(b.map)
    eng.seed([7, 7, 7, 7, 7])
    eng.reset()
    base = eng.action_mask().cpu().numpy().copy()
    assert (base == base[0]).all()
    st = eng.get_state(0)
    x, y = int(st.ent[0][2]), int(st.ent[0][3])
    up = mp.index[(x, y - 1)]  # wall_hp: a wall above either spawn
    assert base[0, 0, 2] == 0
    st = eng.get_state(1)
    st.obst_life[up] = -7  # present, destroyed: still in World.things
    eng.set_state(1, st)
    st = eng.get_state(2)
    st.obst_present[up] = 0  # cleaned up
    eng.set_state(2, st)
    st = eng.get_state(3)
    st.obst_life[:] = -1  # every obstacle destroyed, all present
    eng.set_state(3, st)
    st = eng.get_state(4)
    st.obst_present[:] = 0  # none left
    eng.set_state(4, st)
    got = eng.action_mask().cpu().numpy()
    assert np.array_equal(got, _model_masks(eng, mp))
    assert got[1, 0, 2] == 0 and got[2, 0, 2] == 1
    assert np.array_equal(got[3], base[3]) and np.array_equal(got[0], base[0])
    assert got[4, 0, 2] == 1 and (got[4] >= base[4]).all()
    assert not got[:, :, 7].any()
    eng.close()


# ---- 3. the bound launch --------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", ["eager", "graph", "graph4"])
def test_bound_masks_are_the_last_steps(mode):
    """While a buffer is bound every step ends with the mask launch: after 12 (eager, one step per graph launch)
    or 3 x 4 steps the bound tensor equals a standalone launch on the same state, which equals the model.
    Rebinding recaptures and writes only the new buffer; unbinding stops the writes."""
    import torch
    n = 37
    eng = _engine(_bridge(n))
    mp = M.MapInfo(eng.builder.map)
    eng.seed([900 + i for i in range(n)])
    eng.reset()
    first = eng.bind_action_masks()
    assert eng.describe()["mask_bound"] == 1

    def advance(t0, steps):
        if mode == "eager":
            for t in range(t0, t0 + steps):
                eng.gen_actions(t, 7)
                eng.step()
        else:
            per = 4 if mode == "graph4" else 1
            for t in range(t0, t0 + steps, per):
                eng.step_graph(t, 7, steps=per)

    advance(1, 12)
    bound = first.cpu().numpy().copy()
    alone = eng.action_mask(out=torch.zeros_like(first)).cpu().numpy()
    assert np.array_equal(bound, alone)
    assert np.array_equal(alone, _model_masks(eng, mp))
    second = eng.bind_action_masks(torch.full_like(first, 0x5A))
    advance(13, 4)
    assert np.array_equal(first.cpu().numpy(), bound)  # the first buffer is no longer written
    assert np.array_equal(second.cpu().numpy(), eng.action_mask(out=torch.zeros_like(first)).cpu().numpy())
    assert not np.array_equal(second.cpu().numpy(), bound)
    eng.bind_action_masks(None)
    assert eng.masks is None and eng.describe()["mask_bound"] == 0
    kept = second.cpu().numpy().copy()
    advance(17, 4)
    assert np.array_equal(second.cpu().numpy(), kept)
    eng.close()


def test_an_unbound_handle_is_unchanged():
    """24 graphed steps of two handles seeded alike, one with a bound buffer: the same observation / reward / flag
    hashes every step, and the unbound handle's launch description names no bound buffer."""
    from parity_hash import StepHasher
    n = 37
    engs = [_engine(_bridge(n)) for _ in range(2)]
    for e in engs:
        e.seed([60 + i for i in range(n)])
        e.reset()
    engs[1].bind_action_masks()
    hs = [StepHasher(e) for e in engs]
    assert engs[0].describe()["mask_bound"] == 0
    for t in range(1, 25):
        for e in engs:
            e.step_graph(t, 7)
        assert bool((hs[0].step_hash() == hs[1].step_hash()).all()), t
    for e in engs:
        e.close()


# ---- 4. guard bands -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("offset", [0, 8], ids=["at16", "at16plus8"])
def test_mask_guard_bands(offset):
    """The mask buffer inside a 0x5A-filled byte tensor, at a 16-byte boundary and 8 bytes past one: nothing
    outside it is written, an env whose env-mask byte is 0 keeps its bytes, an all-zero env mask writes nothing,
    entries past the table are 0."""
    import torch
    n = 13
    for make in (_bridge, _single):
        eng = _engine(make(n))
        eng.seed(range(n))
        eng.reset()
        nb = n * eng.A * 8
        raw = torch.full((nb + 256,), 0x5A, dtype=torch.uint8, device=eng.device)
        lo = (-raw.data_ptr()) % 16 + 64 + offset
        assert (raw.data_ptr() + lo) % 16 == offset
        view = raw[lo:lo + nb].view(n, eng.A, 8)
        want = eng.action_mask().cpu().numpy()
        assert not want[:, :, eng.n_discrete:].any() and want[:, :, 5].all()
        sel = [torch.zeros(n), torch.ones(n), torch.arange(n) % 2, (torch.arange(n) == n - 1)]
        for m in sel:
            raw.fill_(0x5A)
            m8 = m.to(torch.uint8).to(eng.device)
            eng.action_mask(m8, out=view)
            got = raw.cpu().numpy()
            assert (got[:lo] == 0x5A).all() and (got[lo + nb:] == 0x5A).all()
            body = got[lo:lo + nb].reshape(n, eng.A, 8)
            on = m.numpy().astype(bool)
            assert np.array_equal(body[on], want[on]) and (body[~on] == 0x5A).all()
        with pytest.raises(ValueError):
            eng.action_mask(out=raw[lo + 4:lo + 4 + nb].view(n, eng.A, 8))  # not 8-byte aligned
        eng.close()


# ---- 5. the Python layers -------------------------------------------------------------------------------------
def test_batched_action_masks(tmp_path):
    """BatchedZombsole(action_masks=True): the [N, A, n_discrete] view is current after reset, a masked reset,
    eager and graphed steps, restore, clone and load_checkpoint."""
    import torch
    from libzombsole_amd.vector import BatchedZombsole
    n = 13
    venv = BatchedZombsole("multi", n, "extermination", [], "bridge", agent_ids=["0", "1"], initial_zombies=10,
                           minimum_zombies=4, max_episode_steps=9, base_seed=3, action_masks=True)
    eng = venv.engine
    mp = M.MapInfo(eng.builder.map)

    def check():
        got = venv.action_masks.cpu().numpy()
        assert got.shape == (n, 2, 7)
        assert np.array_equal(got, _model_masks(eng, mp)[:, :, :7])
        return got

    venv.reset()
    check()
    for t in range(1, 7):
        venv.step(venv.sample_actions(t), graph=bool(t % 2))
        check()
    snap = venv.snapshot()
    ck = str(tmp_path / "ck.pt")
    venv.save_checkpoint(ck)
    at_snap = check()
    for t in range(7, 12):
        venv.step(venv.sample_actions(t))
    venv.restore(snap, src=[0, 1], dst=[4, 5])
    check()
    venv.clone([0], [7], observe=False)
    check()
    venv.load_checkpoint(ck)
    assert np.array_equal(check(), at_snap)
    m = torch.zeros(n, dtype=torch.uint8, device=eng.device)
    m[3] = 1
    venv.reset(m)
    check()
    plain = BatchedZombsole("single", 2, "extermination", [], "bridge", agent_id=0, initial_zombies=3)
    assert plain.action_masks is None and plain.engine.masks is None
    plain.close()
    venv.close()


def test_dropin_action_masks():
    """The drop-in envs' action_masks(): their one env's rows, by the standalone launch."""
    from libzombsole_amd.gym.multiagent_env import MultiagentZombsoleEnvDiscreteAction
    from libzombsole_amd.gym_env import ZombsoleGymEnvDiscreteAction
    env = MultiagentZombsoleEnvDiscreteAction("extermination", ["terminator"], "bridge", ["0", "1"], initial_zombies=6)
    mp = M.MapInfo(env.env.engine.builder.map)
    env.reset()
    for t in range(4):
        got = env.action_masks()
        assert got.shape == (2, 7) and got.dtype == np.uint8
        assert np.array_equal(got, _model_masks(env.env.engine, mp)[0][:, :7])
        env.step({a: (t + i) % 7 for i, a in enumerate(env.env.agents)})
    env.close()
    one = ZombsoleGymEnvDiscreteAction("extermination", [], "bridge", 0, initial_zombies=6)
    one.reset()
    got = one.action_masks()
    assert got.shape == (6,) and got[5] == 1
    assert np.array_equal(got, _model_masks(one.env.engine, mp)[0][0, :6])
    one.close()


def test_viewer_masks_and_refusals():
    """A viewer handle computes the masks of the envs it unpacked (it holds all the kernel reads) and refuses a
    binding; zs_describe names the launch."""
    import torch
    n = 13
    src = _engine(_bridge(n))
    src.seed(range(n))
    src.reset()
    for t in range(1, 4):
        src.gen_actions(t, 7)
        src.step()
    viewer = _engine(_abi.multi_env_config(n, "extermination", [], "bridge", ["0", "1"], initial_zombies=10,
                                           minimum_zombies=4, viewer=True))
    viewer.unpack_obs_state(src.pack_obs_state())
    assert torch.equal(viewer.action_mask(), src.action_mask())
    with pytest.raises(RuntimeError):
        viewer.bind_action_masks()
    d = src.describe()
    assert d["mask_kernel"] == "k_action_mask" and d["mask_block"] == 256 and d["mask_grid"] == (n + 3) // 4
    viewer.close()
    src.close()
