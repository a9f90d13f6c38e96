"""Every consumer of the MT19937 stream started at every index of a block.  641 envs on the crowded 12 x 6 map:
env i < 625 starts each call under test at index i of a twisted block (0 .. 624: the consumers' edges at their
window length, the 64-word sub-block, the 256-word register block and the 624-word block with its slot flip, and
rejection chains that straddle them, fall on some env), 16 more envs at states several blocks into a stream.
Before every call the states go into the oracle envs with zo_set_rng and into the engine, all in one call, through
the host path's rng_host (k_host_unpack); after the call every env's observation, rewards, flags, state and stream
are compared with the oracle's.  The calls, per handle: a mask-mode reset (k_reset over every env); step 1, whose
tick respawns (the config keeps more zombies than it starts with); step 2, a plain mid-episode step that ends the
episode (episodes of two steps); step 3, the autoreset (list-mode reset work, fused or on the side stream); step 4,
a respawning step again.  One handle per launch variant, one oracle run per config shared by its variants.  The
spawn lists are in LDS on the 12 x 6 map and in HBM on the `wide` config (more than 4 096 list entries), both
read from the plan."""
import random

import numpy as np
import pytest

from libzombsole_amd import _abi
from libzombsole_amd import actions as A
from libzombsole_amd.maps import Map

import reset_shapes as R
import step_plan_table as T
from stream_util import at_index, record, same_stream

pytestmark = pytest.mark.gpu

N_IDX, N_DEEP = 625, 16
N = N_IDX + N_DEEP
CALLS = 5  # the reset and four steps
HOST_FLAGS, HOST_ERR, HOST_RNG = 0, 1, 4


# the crowded 12 x 6 map (test_conflict_census.py's layout): 4 player and 16 zombie spawn cells
MELEE_MAP = ("wwwwwwwwwwww\n"
             "w..pppp....w\n"
             "w.zzzzzzzz.w\n"
             "w.zzzzzzzz.w\n"
             "w..........w\n"
             "wwwwwwwwwwww\n")


def plain(n):
    """Nothing but the shuffle and the hits draws in a step: the lanes execute it (unless par_exec is off)."""
    return _abi.multi_env_config(n, "survival", ["terminator"], Map.from_text(MELEE_MAP, name="melee"), ["0", "1"],
                                 initial_zombies=4, minimum_zombies=7, observation_surroundings_width=5,
                                 agent_weapons=["random", "shotgun"], max_episode_steps=2)


def draws(n):
    """A hamster and a randoman, whose decisions draw: the leader's serial loop, and 4 players over 4 cells."""
    return _abi.multi_env_config(n, "survival", ["hamster", "randoman"], Map.from_text(MELEE_MAP, name="melee"),
                                 ["0", "1"], initial_zombies=4, minimum_zombies=7, observation_surroundings_width=5,
                                 agent_weapons=["random", "shotgun"], max_episode_steps=2)


def wide(n):
    """reset_shapes' 96 x 64 map with a player spawn list of 4 100 cells and 65 zombie spawn cells: more than
    4 096 list entries, which the plan stages nowhere, so the reset and respawn work and the tick's leader read
    the lists from HBM; a reset's two player shuffles draw 8 000 words and more (thirteen blocks)."""
    return _abi.multi_env_config(n, "survival", ["hamster", "sniper"], R.field(96, 64, 4100, 65, name="wide"),
                                 ["0", "1"], initial_zombies=4, minimum_zombies=7, observation_surroundings_width=5,
                                 agent_weapons=["random", "shotgun"], max_episode_steps=2)


CONFIGS = {"plain": plain, "draws": draws, "wide": wide}
# (config, variant name, overrides, the plan fields the name stands for); "lanes_per_env" is zs_config's field.
# The melee handles stage the spawn lists in LDS, the wide ones read them from HBM, both read from the plan.  The melee map's 16 zombie spawn cells leave the respawn to the tick's leader by default.
VARIANTS = [
    ("plain", "default", {}, {"fused": 1, "G": 16, "defer_respawn": 0, "rw_step": 64}),
    ("plain", "fused", {"fused": 1}, {"fused": 1, "defer_respawn": 0}),
    ("plain", "side_stream", {"fused": -1}, {"fused": 0, "side_stream": 1, "defer_respawn": 0}),
    ("plain", "serial_reset", {"fused": -1, "reset_stream": -1}, {"fused": 0, "side_stream": 0}),
    ("plain", "G1", {"lanes_per_env": 1}, {"G": 1, "defer_respawn": 0}),
    ("plain", "G4", {"lanes_per_env": 4}, {"G": 4, "defer_respawn": 0}),
    ("plain", "G64", {"lanes_per_env": 64}, {"G": 64, "defer_respawn": 0}),
    ("plain", "leader_exec", {"par_exec": -1}, {"G": 16, "defer_respawn": 0}),
    ("plain", "rw32", {"rw_need": 32}, {"rw_step": 32}),
    ("plain", "rw512", {"rw_need": 512}, {"rw_step": 512, "rw_cap": 512}),
    ("plain", "k_respawn", {"defer_respawn": 1}, {"fused": 1, "defer_respawn": 1}),
    ("plain", "k_respawn_unfused", {"defer_respawn": 1, "fused": -1}, {"fused": 0, "side_stream": 1, "defer_respawn": 1}),
    ("draws", "default", {}, {"fused": 1, "G": 16, "defer_respawn": 0}),
    ("draws", "G1_rw32", {"lanes_per_env": 1, "rw_need": 32}, {"G": 1, "rw_step": 32, "defer_respawn": 0}),
    ("draws", "k_respawn_unfused", {"defer_respawn": 1, "fused": -1}, {"fused": 0, "side_stream": 1, "defer_respawn": 1}),
    # the lists in HBM: k_reset and k_respawn on the side stream, the fused launch, and the tick's leader
    ("wide", "hbm_side_stream", {"fused": -1}, {"fused": 0, "side_stream": 1, "defer_respawn": 1}),
    ("wide", "hbm_fused", {"fused": 1}, {"fused": 1, "defer_respawn": 1}),
    ("wide", "hbm_leader", {"fused": -1, "defer_respawn": -1}, {"fused": 0, "defer_respawn": 0}),
]

_states, _refs = {}, {}


def states(call):
    """uint32 [N][625]: the streams every env starts call `call` from."""
    if call not in _states:
        rows = [at_index(7000 + 1000 * call + i, i) for i in range(N_IDX)]
        for j in range(N_DEEP):  # several blocks in, by a different amount per env
            r = random.Random(9000 + 100 * call + j)
            for _ in range(624 * (2 + j % 5) + 37 * j + 1):
                r.getrandbits(32)
            rows.append(record(r))
        _states[call] = np.stack(rows).astype(np.uint32)
    return _states[call]


def actions(t):
    return np.array([[A.DISCRETE_TRIPLES[A.discrete_action_id(50 + i, t, a, 7)] for a in range(2)] for i in range(N)],
                    dtype=np.int32)


def reference(config):
    """Per call, per env: (obs, rewards, done, truncated, listed before, autoreset, state, stream) of the oracle."""
    from oracle.oracle import OracleEnv
    if config in _refs:
        return _refs[config]
    out = [[] for _ in range(CALLS)]
    acts = [None] + [actions(t) for t in range(1, CALLS)]
    n_resp = n_reset = 0
    for i in range(N):
        o = OracleEnv(CONFIGS[config](1))
        need = False
        for c in range(CALLS):
            o.set_rng(states(c)[i])
            if c == 0 or need:
                ob, r, d, tr, lb, was = o.reset(), None, False, False, np.ones(2, bool), c > 0
                need = False
                n_reset += c > 0
            else:
                ob, r, d, tr, lb = o.step(acts[c][i])
                was, need = False, d or tr
            out[c].append((ob, r, d, tr, lb, was, o.state(), o.get_rng()))
        n_resp += o.census()["respawns"]
    # the calls are what the docstring says: every env autoresets at step 3 and respawns at steps 1 and 4
    assert n_reset == N and n_resp >= 2 * N, (n_reset, n_resp)
    _refs[config] = out
    return out


def check(eng, lay, rec, exp, c, kinds):
    from libzombsole_amd.engine import StateView
    shape, dt = eng.obs_shape, _abi.DTYPE_NP[eng.builder.cfg.obs_dtype]
    assert not rec[:, HOST_ERR].any(), c
    for i in range(N):
        ob, r, d, tr, lb, was, state, rng = exp[i]
        q = rec[i]
        assert int(q[HOST_FLAGS]) == int(d) | (int(tr) << 1) | (int(was) << 2), ("flags", c, i)
        got = q[lay["obs"]:].view(np.uint8)[:lay["obs_bytes"]].view(dt).reshape(shape)
        assert np.array_equal(got, ob), ("obs", c, i)
        if r is not None:
            rw = q[lay["rew"]:lay["rew"] + 2 * lay["R"]].view(np.float64)
            assert np.array_equal(rw[lb].view(np.uint64), r[:2][lb].view(np.uint64)), ("rewards", c, i)
        sv = StateView(eng, q[lay["state"]:lay["state"] + eng.state_words])
        assert sv.canonical(kinds) == state, ("state", c, i)
        assert same_stream(q[HOST_RNG:HOST_RNG + 625].view(np.uint32), rng), ("stream", c, i)


@pytest.mark.parametrize("config,vid,ov,named", VARIANTS, ids=["%s-%s" % (v[0], v[1]) for v in VARIANTS])
def test_every_index(config, vid, ov, named):
    from libzombsole_amd.engine import Engine
    ref = reference(config)
    b = CONFIGS[config](N)
    launch = dict(ov, fobs=-1)
    b.cfg.lanes_per_env = launch.pop("lanes_per_env", 0)
    b.set_launch(launch)
    p = T.plans([(b, launch)])[0]
    assert {k: p[k] for k in named} == named, (vid, p)  # the handle is the one its name says
    if config == "wide":
        assert b.cfg.map.n_player_spawns + b.cfg.map.n_zombie_spawns > 4096
        assert p["rlists_cap"] == p["lists_cap"] == 0, p
    else:
        assert p["rlists_cap"] == p["lists_cap"] == 20, p
    eng = Engine(b)
    try:
        desc = eng.describe()
        assert desc["lanes_per_env"] == p["G"] == (ov.get("lanes_per_env") or p["G"]), (desc, p)
        assert desc["step_kernel"] == ("k_step" if p["fused"] else "k_tick"), desc
        assert desc["respawn"] == ("k_respawn" if p["defer_respawn"] else "tick"), desc
        assert desc["reset_side_stream"] == p["side_stream"] and desc["rng_window"] == p["rw_cap"], (desc, p)
        assert desc["par_exec"] == (0 if ov.get("par_exec", 0) < 0 else 1), desc
        assert desc["rng_step"] == p["rw_step"], (desc, p)
        if "rw_need" in ov:
            assert p["rw_step"] == ov["rw_need"], p
        kinds = [o[2] for o in b.map.obstacles]
        lay = eng.host_layout()
        for c in range(CALLS):
            rec = eng.host_record()
            if c == 0:
                eng.host_reset(states(c), rec)
            else:
                eng.host_step(actions(c), states(c), rec)
            check(eng, lay, rec, ref[c], c, kinds)
    finally:
        eng.close()


def test_set_rng_is_the_host_path():
    """A handful of envs through zs_set_rng / zs_get_rng: the record reads back as the same stream, and a reset
    from it leaves the state and stream the oracle's reset leaves from zo_set_rng of the same record."""
    from libzombsole_amd.engine import Engine
    from oracle.oracle import OracleEnv
    idx = [0, 1, 63, 64, 255, 256, 367, 368, 623, 624]
    recs = [states(0)[i] for i in idx] + [states(0)[N_IDX + 3]]
    eng = Engine(draws(len(recs)).set_launch({"fobs": -1}))
    try:
        kinds = [o[2] for o in eng.builder.map.obstacles]
        for k, rec in enumerate(recs):
            eng.set_rng(k, rec)
            assert same_stream(eng.get_rng(k), rec), k
        obs = eng.reset().cpu().numpy()
        for k, rec in enumerate(recs):
            o = OracleEnv(draws(1))
            o.set_rng(rec)
            assert np.array_equal(obs[k], o.reset()), k
            assert eng.get_state(k).canonical(kinds) == o.state(), k
            assert same_stream(eng.get_rng(k), o.get_rng()), k
    finally:
        eng.close()
