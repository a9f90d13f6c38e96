"""k_autopilot (csrc/zs_autopilot.hpp) through the C ABI and the Python layers: against the reference's own decisions
(tests/golden/pilot/pilot_*.json.gz), against the host model (libzombsole_amd/autopilot.py, pinned to those fixtures on
the CPU by test_autopilot_model.py) on the shapes where the mapping can break, as the closed loop that plays a
fixture's run, as an addition that leaves everything else alone, and through the batched and drop-in layers."""
import numpy as np
import pytest

import golden_util as G
import pilot_census as PC
from libzombsole_amd import _abi
from libzombsole_amd import autopilot as AP
from libzombsole_amd import entity_obs as EO

pytestmark = pytest.mark.gpu
NAMES = PC.pilot_fixture_names()


def _engine(b):
    from libzombsole_amd.engine import Engine
    return Engine(b)


def _fixture_engine(fx):
    """One env per seed of the fixture, seeded, its obstacle pokes applied, reset."""
    runs = fx["runs"]
    eng = _engine(G.builder_for(fx, num_envs=len(runs)))
    eng.seed([r["seed"] for r in runs])
    for k in range(len(runs) if G.obstacle_pokes(fx) else 0):
        st = eng.get_state(k)
        for i, life in G.obstacle_pokes(fx):
            st.obst_life[i] = life
        eng.set_state(k, st)
    eng.reset()
    return eng


def _poke(eng, k, rank, x, y):
    """make_pilot_golden.py's poke_things on env k: the thing at `rank` of the dict order moved to (x, y) and put
    last, through an edited snapshot record (zs_set_state refuses a position outside the map)."""
    import torch
    L = eng.snapshot_layout()
    n = eng.get_state(k).n_order
    rec = eng.snapshot([k]).cpu().numpy().copy()
    order = rec[0, L["order"]:L["order"] + eng.E]
    slot = int(order[rank])
    rec[0, L["pos"]:L["pos"] + 4 * eng.E].view(np.int32)[slot] = (x & 0xffff) | (y << 16)
    order[:n] = [s for s in order[:n] if s != slot] + [slot]
    eng.restore(torch.from_numpy(rec).to(eng.device), dst=[k])


# ---- 1. the reference's decisions ----------------------------------------------------------------------------
@pytest.mark.parametrize("name", NAMES)
def test_triples_equal_the_reference(name):
    """The engine driven through a fixture's calls (every seed one env, next-step autoreset): after every call the
    standalone launch's triples are the reference's, for all three policies.  A fixture with poke_things is driven up
    to its poked call and checked there: the poke puts a zombie outside the map, where the engine's tick never lets a
    thing go and from where it is not stepped (the calls after it are the CPU model's and the host program's)."""
    import torch
    fx = G.load_fixture(name)
    runs = fx["runs"]
    pokes = (fx.get("extras") or {}).get("poke_things", [])
    eng = _fixture_engine(fx)
    kinds = [o[2] for o in eng.builder.map.obstacles]
    for i in range(len(runs[0]["calls"])):
        if i > 0:
            acts = np.stack([G.action_triples(fx, r["calls"][i], eng.A)[:eng.A] if r["calls"][i]["kind"] == "step"
                             else np.zeros((eng.A, 3), np.int32) for r in runs])
            eng.actions.copy_(torch.from_numpy(acts))
            eng.step()
        poked = [p for p in pokes if p[1] == i]
        for seed, _call, rank, x, y in poked:
            _poke(eng, [r["seed"] for r in runs].index(seed), rank, x, y)
        got = {p: eng.autopilot(p).cpu().numpy() for p in PC.POLICY_NAMES}
        for k, r in enumerate(runs):
            if not poked:
                assert eng.get_state(k).canonical(kinds)["dyn"] == r["calls"][i]["state"]["dyn"], (name, r["seed"], i)
            for p in PC.POLICY_NAMES:
                assert got[p][k].tolist() == r["pilot"][i][p], (name, r["seed"], i, p, got[p][k].tolist())
        if poked:
            assert len(poked) == len(runs) and any(t[0] == AP.ACT.ACT_MOVE for k in range(len(runs))
                                                   for t in got["terminator"][k].tolist())
            break
    eng.close()


# ---- 2. the host model on the shapes where the mapping can break -----------------------------------------------
def _bridge(n):
    return _abi.multi_env_config(n, "extermination", [], "bridge", ["0", "1"], initial_zombies=10, minimum_zombies=4,
                                 max_episode_steps=9, agent_weapons=["knife", "shotgun"])


def _fort(n):  # E = 132 slots: three passes of the wave; A = 32
    return _abi.multi_env_config(n, "extermination", [], "fort", [str(i) for i in range(32)], initial_zombies=100,
                                 minimum_zombies=0, max_episode_steps=10, agent_weapons=["knife", "axe", "shotgun", "gun"])


def _bridge64_respawn(n):
    return _abi.multi_env_config(n, "extermination", [], "bridge64", ["0", "1"], initial_zombies=10,
                                 minimum_zombies=6, max_episode_steps=6, agent_weapons="knife")


def _city128(n):
    return _abi.multi_env_config(n, "safehouse", [], "city128", ["0", "1", "2", "3"], initial_zombies=50,
                                 minimum_zombies=50, max_episode_steps=11, agent_weapons=["knife", "gun", "axe", "shotgun"])


def _wall(n):
    return _abi.multi_env_config(n, "survival", [], G.map_path("wall_hp"), ["0", "1"], initial_zombies=1,
                                 minimum_zombies=1, agent_weapons=["knife", "shotgun"], max_episode_steps=5)


def _single(n):
    return _abi.single_env_config(n, "extermination", ["terminator"], "bridge", 0, initial_zombies=10,
                                  minimum_zombies=6, agent_weapon="knife", max_episode_steps=8)


DIFF = {"bridge_13": (_bridge, 13, None), "bridge_37": (_bridge, 37, None),
        "bridge64_37_respawn_fused": (_bridge64_respawn, 37, {"defer_respawn": 1, "fused": 1}),
        "bridge64_13_respawn_unfused": (_bridge64_respawn, 13, {"defer_respawn": 1, "fused": -1}),
        "fort_13": (_fort, 13, None), "city128_13": (_city128, 13, None), "wall5x4_37": (_wall, 37, None),
        "single_bridge_13": (_single, 13, None)}


def _model(eng, static, policy):
    """autopilot.decide over every env, into 77-filled rows: [N, A, 3]."""
    out = np.full((eng.N, eng.A, 3), 77, dtype=np.int32)
    for k in range(eng.N):
        AP.decide(eng.get_state(k), static, eng.A, policy[k], out=out[k])
    return out


@pytest.mark.parametrize("row", sorted(DIFF))
def test_triples_equal_the_model(row):
    """Seeded runs of 24 steps with autoresets, the even envs driven by the pilot's own triples and the odd ones by
    gen_actions, under a per-agent policy tensor mixing the codes 0..3 (code 0 rows keep the 77 written there): every
    env, every step, the reset call included."""
    import torch
    make, n, launch = DIFF[row]
    b = make(n)
    if launch:
        b.set_launch(dict(launch, fobs=-1))
    eng = _engine(b)
    if launch:
        d = eng.describe()
        assert d["respawn"] == "k_respawn" and d["step_kernel"] == ("k_step" if launch["fused"] > 0 else "k_tick"), d
    static = EO.Static.of_map(b.map)
    eng.seed([5000 + i for i in range(n)])
    eng.reset()
    codes = np.array([[(k + 2 * a + 1) % 4 if k % 3 else AP.TERMINATOR for a in range(eng.A)] for k in range(n)], np.uint8)
    pol = torch.from_numpy(codes).to(eng.device)
    even = (torch.arange(n, device=eng.device) % 2 == 0).view(n, 1, 1)
    seen, resets = set(), 0
    for t in range(25):
        if t:
            rnd = eng.gen_actions(t, eng.n_discrete).clone()
            mine = torch.where(got_dev == 77, torch.zeros_like(got_dev), got_dev)
            eng.actions.copy_(torch.where(even, mine, rnd))
            eng.step()
            resets += int(eng.was_reset.sum())
        got_dev = eng.autopilot(pol, out=torch.full((n, eng.A, 3), 77, dtype=torch.int32, device=eng.device))
        got = got_dev.cpu().numpy()
        want = _model(eng, static, codes)
        assert np.array_equal(got, want), (row, t, np.argwhere(got != want)[:5].tolist())
        seen |= {int(v) for v in got[:, :, 0].ravel()}
    assert resets >= n // 2 and {AP.ACT.ACT_ATTACK_CLOSEST, AP.ACT.ACT_HEAL, AP.ACT.ACT_MOVE, 77} <= seen, (resets, seen)
    assert eng.overflow() == 0
    eng.close()


# ---- 3. the closed loop ---------------------------------------------------------------------------------------
LOOPS = ["pilot/pilot_multi_boxed_a2_knife", "pilot/pilot_multi_open_a4_weapons", "pilot/pilot_single_strip_bot"]


@pytest.mark.parametrize("mode", ["eager", "graph", "graph_n"])
@pytest.mark.parametrize("name", LOOPS)
def test_closed_loop_plays_the_fixture(name, mode):
    """With the autopilot bound into the action buffer nothing is written to the actions after the first launch:
    every step of a terminator-driven fixture run gives the fixture's rewards (float64 hex), flags and observation
    hashes.  graph_n: zs_step_graph_n with its generated policy off (n_discrete = 0), two steps a launch, checked
    after every second call."""
    import torch
    fx = G.load_fixture(name)
    assert fx["extras"]["pilot"] == ["terminator"] * PC.n_agents(fx) and "poke_things" not in fx["extras"]
    runs = fx["runs"]
    eng = _fixture_engine(fx)
    assert eng.bind_autopilot("terminator", into_actions=True) is eng.actions and eng.pilot is eng.actions
    eng.autopilot(eng.pilot_policy, out=eng.actions)  # the reset world's rows; from here on the steps write them
    per = 2 if mode == "graph_n" else 1
    ncalls = len(runs[0]["calls"])
    for i in range(per, ncalls, per):
        if mode == "eager":
            eng.step()
        elif mode == "graph":
            eng.step_graphed()
        else:
            eng.step_graph(0, 0, steps=per)
        torch.cuda.synchronize()
        obs, rew = eng.obs.cpu().numpy(), eng.rewards.cpu().numpy()
        done, trunc = eng.done.cpu().numpy(), eng.trunc.cpu().numpy()
        listed, was_reset = eng.listed.cpu().numpy(), eng.was_reset.cpu().numpy()
        acts = eng.actions.cpu().numpy()
        for k, r in enumerate(runs):
            rec = r["calls"][i]
            where = (name, mode, r["seed"], i)
            assert ("reset" if was_reset[k] else "step") == rec["kind"], where
            lst = listed[k].astype(bool) if rec["kind"] == "step" else np.ones(eng.A, bool)
            if rec["kind"] == "step":
                assert (bool(done[k]), bool(trunc[k])) == (rec["done"], rec["trunc"]), where
                assert G.rewards_record(fx, rew[k], lst) == rec["rew"], where
            assert G.obs_sha(fx, obs[k], lst if fx["surface"] == "multi" else None) == rec["obs_sha"], where
            assert acts[k].tolist() == r["pilot"][i]["terminator"], where
    eng.close()


# ---- 4. an addition -------------------------------------------------------------------------------------------
def test_code_zero_rows_and_guard_bands():
    """The output inside a 0x5A-filled tensor: nothing outside it is written, rows of code 0 and envs whose env-mask
    byte is 0 keep the sentinel, code 9 writes idle and raises OVF_PARAM_RANGE."""
    import torch
    n = 13
    eng = _engine(_bridge(n))
    eng.seed(range(n))
    eng.reset()
    A = eng.A
    nw = n * A * 3
    raw = torch.full((nw + 64,), 0x5A5A5A5A, dtype=torch.int32, device=eng.device)
    view = raw[32:32 + nw].view(n, A, 3)
    codes = torch.tensor([[k % 4, (k + 1) % 2] for k in range(n)], dtype=torch.uint8, device=eng.device)
    want = eng.autopilot(torch.where(codes == 0, torch.ones_like(codes), codes)).cpu().numpy()
    for m in (torch.zeros(n), torch.ones(n), torch.arange(n) % 2, (torch.arange(n) == n - 1)):
        raw.fill_(0x5A5A5A5A)
        eng.autopilot(codes, m.to(torch.uint8).to(eng.device), out=view)
        got = raw.cpu().numpy()
        assert (got[:32] == 0x5A5A5A5A).all() and (got[32 + nw:] == 0x5A5A5A5A).all()
        body = got[32:32 + nw].reshape(n, A, 3)
        on = m.numpy().astype(bool)[:, None] & (codes.cpu().numpy() != 0)
        assert np.array_equal(body[on], want[on]) and (body[~on] == 0x5A5A5A5A).all()
    assert eng.overflow() == 0
    bad = codes.clone()
    bad[5, 0] = 9
    got = eng.autopilot(bad, out=torch.full_like(view, 77)).cpu().numpy()
    assert got[5, 0].tolist() == [0, 0, 0] and eng.overflow(clear=True) == _abi.OVF_PARAM_RANGE
    with pytest.raises(ValueError):
        eng.autopilot(codes, out=raw[:nw].view(n, A, 3)[:, :, :2])
    eng.close()


def test_a_bound_handle_changes_nothing_else():
    """24 graphed steps of two handles seeded alike and given the same actions, one with masks, entity rows and the
    autopilot bound, the other with masks and entity rows: the same observation / reward / flag hashes, masks and
    entity rows every step; the bound triples equal a standalone launch; describe() names the launch."""
    import torch
    from parity_hash import StepHasher
    n = 37
    engs = [_engine(_bridge(n)) for _ in range(2)]
    for e in engs:
        e.seed([60 + i for i in range(n)])
        e.reset()
        e.bind_action_masks()
        e.bind_entity_obs(True, 4, 1)
    assert engs[1].describe()["autopilot_bound"] == 0
    pol = engs[1].policy_tensor("terminator")
    pol[::3, 1] = AP.SNIPER
    out = engs[1].bind_autopilot(pol)
    d = engs[1].describe()
    assert d["autopilot_bound"] == 1 and d["autopilot_kernel"] == "k_autopilot" and d["autopilot_block"] == 256
    assert d["autopilot_grid"] == (n + 3) // 4 and engs[0].describe()["autopilot_bound"] == 0 and engs[0].pilot is None
    hs = [StepHasher(e) for e in engs]
    for t in range(1, 25):
        for e in engs:
            e.step_graph(t, 7)
        assert bool((hs[0].step_hash() == hs[1].step_hash()).all()), t
        assert torch.equal(engs[0].masks, engs[1].masks) and torch.equal(engs[0].entities, engs[1].entities), t
        if t == 12:  # the policy tensor's contents may change between replays
            pol[:, 0] = AP.TROLL
    kinds0 = set(out[:, 0, 0].tolist())  # the trolls heal; an agent that is not in the world idles
    assert torch.equal(out, engs[1].autopilot(pol)) and AP.ACT.ACT_HEAL in kinds0 and kinds0 <= {AP.ACT.ACT_HEAL, AP.ACT.ACT_IDLE}
    engs[1].bind_autopilot(None)
    assert engs[1].pilot is None and engs[1].describe()["autopilot_bound"] == 0
    kept = out.clone()
    engs[1].step_graph(25, 7)
    assert torch.equal(out, kept)
    for e in engs:
        e.close()


# ---- 5. refusals ----------------------------------------------------------------------------------------------
def test_refusals():
    import ctypes
    import torch
    n = 5
    eng = _engine(_bridge(n))
    viewer = _engine(_abi.multi_env_config(n, "extermination", [], "bridge", ["0", "1"], initial_zombies=10,
                                           minimum_zombies=4, viewer=True, agent_weapons=["knife", "shotgun"]))
    pol = torch.ones((n, 2), dtype=torch.uint8, device=eng.device)
    out = torch.zeros((n, 2, 3), dtype=torch.int32, device=eng.device)
    vp = lambda t: ctypes.c_void_p(t.data_ptr())  # noqa: E731
    L = eng.L
    assert L.zs_autopilot(viewer.h, None, vp(pol), vp(out), None) == _abi.ZS_ESTATE
    assert L.zs_autopilot_bind(viewer.h, vp(pol), vp(out)) == _abi.ZS_ESTATE
    with pytest.raises(RuntimeError):
        viewer.autopilot("terminator")
    for args in ((eng.h, None, None, vp(out), None), (eng.h, None, vp(pol), None, None), (None, None, vp(pol), vp(out), None)):
        assert L.zs_autopilot(*args) == _abi.ZS_EINVAL
    for args in ((eng.h, None, vp(out)), (eng.h, vp(pol), None), (None, vp(pol), vp(out))):
        assert L.zs_autopilot_bind(*args) == _abi.ZS_EINVAL
    assert L.zs_autopilot_bind(eng.h, None, None) == _abi.ZS_OK  # nothing bound: unbinding is no error
    viewer.close()
    eng.close()


# ---- 6. the batched layer ---------------------------------------------------------------------------------------
def test_batched_scripted_actions(tmp_path):
    """BatchedZombsole(autopilot=...): scripted_actions is current after reset, a masked reset, eager and graphed
    steps, step_scripted, set_autopilot, restore, clone and load_checkpoint."""
    import torch
    from libzombsole_amd.vector import BatchedZombsole
    n = 13
    kw = dict(agent_ids=["0", "1"], initial_zombies=10, minimum_zombies=4, max_episode_steps=9, base_seed=3,
              agent_weapons=["knife", "shotgun"])
    venv = BatchedZombsole("multi", n, "extermination", [], "bridge", autopilot="terminator", **kw)
    eng = venv.engine
    static = EO.Static.of_map(eng.builder.map)

    def check():
        got = venv.scripted_actions.cpu().numpy()
        codes = eng.pilot_policy.cpu().numpy()
        want = _model(eng, static, codes)
        on = codes != 0
        assert got.shape == (n, 2, 3) and np.array_equal(got[on], want[on])
        return got

    venv.reset()
    check()
    for t in range(1, 7):
        if t % 3:
            venv.step(venv.sample_actions(t), graph=bool(t % 2))
        else:
            venv.step_scripted()
        check()
    venv.set_autopilot(torch.tensor([AP.SNIPER, AP.TERMINATOR], dtype=torch.uint8))
    venv.step_scripted(graph=False)
    kinds0 = set(check()[:, 0, 0].tolist())  # the snipers; an agent that is not in the world idles
    assert AP.ACT.ACT_ATTACK_CLOSEST in kinds0 and kinds0 <= {AP.ACT.ACT_ATTACK_CLOSEST, AP.ACT.ACT_IDLE}
    venv.set_autopilot("terminator")
    venv.step(venv.sample_actions(7))
    snap = venv.snapshot()
    ck = str(tmp_path / "ck.pt")
    venv.save_checkpoint(ck)
    at_snap = check()
    for t in range(8, 13):
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
    venv.close()
    loop = BatchedZombsole("multi", 5, "extermination", [], "bridge", autopilot="troll", autopilot_into_actions=True, **kw)
    assert loop.scripted_actions is loop.actions
    loop.reset()
    loop.step_scripted()
    assert bool((loop.actions[:, :, 0] == AP.ACT.ACT_HEAL).all())
    loop.close()
    plain = BatchedZombsole("single", 2, "extermination", [], "bridge", agent_id=0, initial_zombies=3)
    assert plain.scripted_actions is None and plain.engine.pilot is None
    with pytest.raises(ValueError):
        plain.step_scripted()
    plain.close()


# ---- 7. the drop-ins -------------------------------------------------------------------------------------------
def test_dropin_scripted_actions_equal_the_fixtures():
    """MultiagentZombsoleEnv.scripted_actions / ZombsoleGymEnv.scripted_action, stepped with their own terminator
    dicts as the fixture's run was: every call's dicts are the fixture's triples' dicts."""
    import random
    from libzombsole_amd.gym.multiagent_env import MultiagentZombsoleEnv
    from libzombsole_amd.gym_env import ZombsoleGymEnv
    for name, cls in (("pilot/pilot_multi_boxed_a2_knife", MultiagentZombsoleEnv), ("pilot/pilot_single_strip_bot", ZombsoleGymEnv)):
        fx = G.load_fixture(name)
        multi = fx["surface"] == "multi"
        kw = dict(fx["kwargs"])
        kw["map_name"] = G.map_path(kw["map_name"])
        run = fx["runs"][0]
        env = cls(**kw)
        random.seed(run["seed"])
        env.reset()
        for i in range(12):
            rec, pl = run["calls"][i], run["pilot"][i]
            if i and rec["kind"] == "reset":
                env.reset()
            elif i:
                env.step(act)
            if multi:
                act = env.scripted_actions("terminator")
                assert act == {a: AP.to_action_dict(t) for a, t in zip(kw["agent_ids"], pl["terminator"])}, (name, i)
                assert env.scripted_actions(["sniper", AP.TROLL]) == {
                    "0": AP.to_action_dict(pl["sniper"][0]), "1": AP.to_action_dict(pl["troll"][1])}
            else:
                act = env.scripted_action("terminator")
                assert act == AP.to_action_dict(pl["terminator"][0]), (name, i)
                assert env.scripted_action("sniper") == AP.to_action_dict(pl["sniper"][0])
        env.close()
