"""The (shape, overrides) matrix of the observation plan (libzombsole_amd/csrc/zs_obs_plan.hpp) and the
table of what every pair resolved to before the plan existed (tests/obs_plan_expected.json: the launch
parameters the engine printed on an MI355X, one row per pair).  test_obs_plan.py checks the plan against
the table on the CPU; the GPU tests that name a kernel take the name they assert from it."""
import json
import os

from libzombsole_amd import _abi
from libzombsole_amd.maps import Map

HERE = os.path.dirname(os.path.abspath(__file__))
WALL_HP_MAP = "wwwww\nwpwpw\nw...w\nwwwww\n"  # test_obstacle_hp.py


def c2(n):
    return _abi.multi_env_config(n, "extermination", [], "bridge64", ["0", "1"], initial_zombies=10,
                                 minimum_zombies=0, max_episode_steps=1000)


def c5(n, dtype=_abi.DTYPE_I16):
    return _abi.multi_env_config(n, "extermination", [], "bridge64", ["0", "1", "2", "3"], initial_zombies=20,
                                 obs_dtype=dtype, max_episode_steps=200)


def c4(n, dtype=_abi.DTYPE_I64):
    return _abi.multi_env_config(n, "safehouse", [], "city128", ["0", "1", "2", "3"], initial_zombies=50,
                                 minimum_zombies=50, obs_dtype=dtype)


def bridge64_single_i32(n):
    return _abi.single_env_config(n, "extermination", [], "bridge64", 0, initial_zombies=10,
                                  observation_scope="surroundings:21", observation_position_encoding="channels",
                                  max_episode_steps=200)


def cityfs_world(n):
    return _abi.single_env_config(n, "safehouse", ["terminator"], "city_for_safehouse", "0", initial_zombies=20,
                                  minimum_zombies=20, observation_scope="world",
                                  observation_position_encoding="channels", max_episode_steps=50)


def easy_exit_surr9(n):
    return _abi.single_env_config(n, "evacuation", ["terminator", "randoman", "hamster", "troll"], "easy_exit", "0",
                                  initial_zombies=8, minimum_zombies=6, observation_scope="surroundings:9",
                                  observation_position_encoding="channels", agent_weapon="random",
                                  max_episode_steps=80)


def fort_w11_i16(n):
    return _abi.multi_env_config(n, "survival", ["sniper", "randoman"], "fort", ["0", "1", "2"], initial_zombies=30,
                                 minimum_zombies=20, agent_weapons=["random", "gun"],
                                 observation_surroundings_width=11, obs_dtype=_abi.DTYPE_I16, max_episode_steps=70)


def wall_hp(n, dtype=_abi.DTYPE_I64):
    return _abi.multi_env_config(n, "extermination", [], Map.from_text(WALL_HP_MAP, name="wall_hp"), ["0", "1"],
                                 initial_zombies=0, minimum_zombies=0, obs_dtype=dtype)


# name -> (config builder, env count); "<config>@<envs>"
SHAPES = {}
for _n in (67, 96, 8192, 12287, 12288, 65536):  # the int64 store streams start at 48 * 256 envs
    SHAPES["c2@%d" % _n] = (c2, _n)
for _n in (64, 4097, 65536):
    SHAPES["c5@%d" % _n] = (c5, _n)
SHAPES["c5_i64@64"] = (lambda n: c5(n, _abi.DTYPE_I64), 64)
SHAPES["bridge64_single_i32@64"] = (bridge64_single_i32, 64)
for _n in (9, 24, 16384):
    SHAPES["c4@%d" % _n] = (c4, _n)
SHAPES["cityfs_world@16"] = (cityfs_world, 16)
SHAPES["easy_exit_surr9@32"] = (easy_exit_surr9, 32)
SHAPES["fort_w11_i16@64"] = (fort_w11_i16, 64)
for _name, _dt in (("i64", _abi.DTYPE_I64), ("i32", _abi.DTYPE_I32), ("i16", _abi.DTYPE_I16)):
    SHAPES["wall_hp_%s@64" % _name] = (lambda n, dt=_dt: wall_hp(n, dt), 64)


def overrides():
    """name -> zs_launch overrides: the automatic choice, every observation path the GPU tests force, and
    one that caps the grid and turns the ring off."""
    from tests import test_engine_oracle, test_obstacle_hp
    ov = {"default": {}}
    for name, lo in test_engine_oracle.PATHS.items():
        if any(k.startswith("obs_") or k == "fobs" for k in lo):
            ov["paths:" + name] = lo
    for name, lo in test_engine_oracle.CITY128_OBS.items():
        ov["city128:" + name] = lo
    for name, (lo, _) in test_obstacle_hp.ENCODERS.items():
        ov["encoders:" + name] = lo
    for name, lo in test_obstacle_hp.OBS_PATHS.items():
        ov["hp:" + name] = lo
    for name, lo in test_engine_oracle.STORE_STREAM.items():
        ov["stream:" + name] = lo
    ov["one_wg_no_ring"] = {"obs_wgs": 1, "obs_lds": 1, "obs_ring": -1}
    seen, uniq = set(), {}
    for name, lo in ov.items():  # one row per distinct set of overrides (under its first name)
        if ov_key(lo) not in seen:
            seen.add(ov_key(lo))
            uniq[name] = lo
    return uniq


def ov_key(lo):
    return json.dumps(sorted((lo or {}).items()))


def shape_ints(builder, lo):
    """The ObsShape of a config (zs_create's arithmetic on the config's integers; defer_respawn as the compiled
    step plan decides it), in the struct's order."""
    c, m = builder.cfg, builder.cfg.map
    W, H, O = m.width, m.height, m.n_obstacles
    E = c.num_agents + c.num_bots + max(c.initial_zombies, c.minimum_zombies)
    cells = [m.obstacle_xy[2 * i + 1] * W + m.obstacle_xy[2 * i] for i in range(O)]
    rank_order = all(b > a for a, b in zip(cells, cells[1:]))
    import step_plan_table
    defer = step_plan_table.defer_respawn(builder, lo)  # step_defer_respawn() (zs_step_plan.hpp), compiled
    return [c.num_envs, W, H, O, (O + 31) // 32, (W * H + 31) // 32, E, c.num_agents, c.obs_scope, c.obs_encoding,
            c.obs_width, c.obs_dtype, c.reward_mode, (W + 20) * (H + 20), int(rank_order), int(defer)]


_rows = None


def expected(shape, lo):
    """The table's row for SHAPES[shape] under the overrides lo: {"full": {...}, "masked": {...}, ...}."""
    global _rows
    if _rows is None:
        with open(os.path.join(HERE, "obs_plan_expected.json")) as f:
            _rows = {(r["shape"], ov_key(r["ov"])): r for r in json.load(f)}
    return _rows[(shape, ov_key(lo))]


KERNEL_NAMES = ["k_obs", "k_obs_gather", "k_obs_pipe", "k_obs_patch", "k_obs_ring", "k_obs_pbring"]  # OBSK_*


def expected_describe(shape, lo):
    """(obs_kernel, obs_kernel_masked, obs_encoders) that describe() reports for the pair."""
    r = expected(shape, lo)
    full = KERNEL_NAMES[r["full"]["kind"]]
    enc = ("patched" if r["full"]["patched"] else "select") if full == "k_obs_ring" else ""
    return ("step launch" if r["fobs"] else full), KERNEL_NAMES[r["masked"]["kind"]], enc
