"""ctypes mirror of include/zombsole_mi355x.h (constants, structs) and the
host-side translation of the reference's constructor arguments into a
`zs_config` (rules / weapon / observation / player-name factories).

Pure host code: importable without torch or a GPU.
"""
import ctypes as C

import numpy as np

from .maps import Map, load_map

# status codes
ZS_OK, ZS_EINVAL, ZS_ENOSPACE, ZS_EHIP, ZS_ESTATE = 0, 1, 2, 3, 4
# things
THING_NONE, THING_BOX, THING_DEADBODY, THING_OBJECTIVE, THING_WALL = 0, 1, 2, 3, 4
THING_ZOMBIE, THING_PLAYER, THING_AGENT = 5, 6, 7
# weapons (observation codes, gym/observation.py:27-34)
WEAPON_NONE, WEAPON_CLAWS, WEAPON_KNIFE, WEAPON_AXE = 0, 1, 10, 11
WEAPON_GUN, WEAPON_RIFLE, WEAPON_SHOTGUN, WEAPON_RANDOM = 12, 13, 14, 255
# bots
BOT_TERMINATOR, BOT_SNIPER, BOT_TROLL, BOT_HAMSTER, BOT_RANDOMAN = 1, 2, 3, 4, 5
# rules
RULES_EXTERMINATION, RULES_SURVIVAL, RULES_EVACUATION, RULES_SAFEHOUSE = 0, 1, 2, 3
REWARD_SINGLE, REWARD_MULTI = 0, 1
OBS_WORLD, OBS_SURROUNDINGS = 0, 1
ENC_SIMPLE, ENC_CHANNELS = 0, 1
DTYPE_I32, DTYPE_I64, DTYPE_I16 = 0, 1, 2
FLAG_AUTORESET = 1
FLAG_DEBUG = 2
FLAG_DEATH_LOG = 4  # zs_death_log: the drop-in views' decoration order and removed zombies' final values
FLAG_VIEWER = 8  # a handle that holds other handles' envs for encoding (zs_obs_state_unpack + zs_observe)
FLAG_ENV_PARAMS = 16  # per-env (initial_zombies, minimum_zombies, max_episode_steps): zs_env_params_set / _get
FLAG_EPISODE_STATS = 32  # per-env episode statistics kept on the device: zs_episode_stats_*
FLAG_RENDER = 64  # frames of the envs drawn on the device: zs_render* (the builders set FLAG_DEATH_LOG with it: it needs it)
OVF_INT16, OVF_INT32 = 1, 2  # zs_overflow range flags
OVF_PARAM_RANGE = 4  # zs_env_params_set met an entry it did not apply (env or value out of range)
ENV_PARAMS = ("initial_zombies", "minimum_zombies", "max_episode_steps")  # a per-env triple, in order
STATE_HEADER, STATE_ENTITY_WORDS = 16, 8
# episode statistics (csrc/zs_episode.hpp): the words of `last` and `tot`, the outcome codes of last[1]
EP_LAST = ("length", "outcome", "zombie_deaths", "deaths", "initial_zombies", "minimum_zombies", "max_episode_steps", "serial")
EP_TOT = ("episodes", "won", "lost", "truncated_agents_dead", "truncated_timelimit", "length", "zombie_deaths", "deaths")
EP_WON, EP_LOST, EP_AGENTS_DEAD, EP_TIMELIMIT, EP_DONE_AND_TIMELIMIT = 1, 2, 3, 4, 256

DTYPE_NP = {DTYPE_I32: np.int32, DTYPE_I64: np.int64, DTYPE_I16: np.int16}

_RULES = {"extermination": RULES_EXTERMINATION, "survival": RULES_SURVIVAL,
          "evacuation": RULES_EVACUATION, "safehouse": RULES_SAFEHOUSE}
_WEAPONS = {"knife": WEAPON_KNIFE, "axe": WEAPON_AXE, "gun": WEAPON_GUN, "rifle": WEAPON_RIFLE,
            "shotgun": WEAPON_SHOTGUN, "random": WEAPON_RANDOM}
_BOTS = {"terminator": BOT_TERMINATOR, "sniper": BOT_SNIPER, "troll": BOT_TROLL,
         "hamster": BOT_HAMSTER, "randoman": BOT_RANDOMAN}


class zs_map_desc(C.Structure):
    _fields_ = [("width", C.c_int32), ("height", C.c_int32),
                ("n_obstacles", C.c_int32), ("obstacle_xy", C.POINTER(C.c_int32)),
                ("obstacle_kind", C.POINTER(C.c_uint8)),
                ("n_objectives", C.c_int32), ("objective_xy", C.POINTER(C.c_int32)),
                ("n_player_spawns", C.c_int32), ("player_spawn_xy", C.POINTER(C.c_int32)),
                ("n_zombie_spawns", C.c_int32), ("zombie_spawn_xy", C.POINTER(C.c_int32))]


OBS_STATE_SECTIONS = ("hp_dirty", "dead_dirty", "pos", "life", "dead", "obst_present", "obst_hp", "weapon", "present")


def obs_state_layout(E, O, DW, OW, obs_dtype):
    """Mirror of obs_state_layout() (csrc/zs_obs_state.hpp): the byte offset of every section of an env's
    observation-state record, "pad" (where the zero padding starts), "rec_bytes" (a multiple of 16) and
    "hp_bytes" (2 for DTYPE_I16: the obstacle HP as int16 saturated at -32768, else 4)."""
    hp = 2 if obs_dtype == DTYPE_I16 else 4
    L, o = {}, 0
    for name, nbytes in zip(OBS_STATE_SECTIONS, (4, 4, 4 * E, 4 * E, 4 * DW, 4 * OW, hp * O, E, E)):
        L[name] = o
        o += nbytes
    L["pad"] = o
    L["rec_bytes"] = (o + 15) // 16 * 16
    L["hp_bytes"] = hp
    return L


def obs_state_record_dtype(obs_dtype, obs_encoding):
    """Mirror of obs_state_record_dtype(): an int16 handle with the simple encoding ships int32 HP (that encoding
    folds the unsaturated life into its code)."""
    return DTYPE_I32 if obs_dtype == DTYPE_I16 and obs_encoding != ENC_CHANNELS else obs_dtype


SNAPSHOT_NSCAL, SNAPSHOT_RING = 9, 1248  # the per-env scalar rows, the words of both MT19937 blocks
SNAPSHOT_SECTIONS = ("ring", "dead", "obst_hp", "obst_present", "obst_nonpos", "pos", "life", "serial", "scal", "hp_dirty",
                     "dead_dirty", "rngst", "prev_life", "weapon", "present", "order", "listed")


def snapshot_section_bytes(E, O, DW, OW, A):
    """The size in bytes of every section of a snapshot record, in SNAPSHOT_SECTIONS' order."""
    return (4 * SNAPSHOT_RING, 4 * DW, 4 * O, 4 * OW, 4 * OW, 4 * E, 4 * E, 4 * E, 4 * SNAPSHOT_NSCAL, 4, 4, 4, 4 * A,
            E, E, E, A)


def snapshot_layout(E, O, DW, OW, A, env_params=False, episode_R=0, body_bytes=0):
    """Mirror of snapshot_layout() (csrc/zs_snapshot.hpp): the byte offset of every section of an env's snapshot
    record, "pad" (where the zero padding starts) and "rec_bytes" (a multiple of 16).  env_params: the record of a
    FLAG_ENV_PARAMS handle, with "env_params" (six int32: the current triple, then the next) before the byte rows.
    episode_R > 0: the record of a FLAG_EPISODE_STATS handle with that many reward slots per env, with "ep_run" (8-byte
    aligned: run_ret float64 [R], run_flags int32, 4 zero bytes) behind env_params and "ep_bytes".
    body_bytes > 0: the record of a FLAG_RENDER handle, with "body_col" (that many bytes: W * H rounded up to 16) behind
    "listed", the last byte row, and "body_bytes"."""
    L, o = {}, 0
    for name, nbytes in zip(SNAPSHOT_SECTIONS, snapshot_section_bytes(E, O, DW, OW, A)):
        if env_params and name == "weapon":
            L["env_params"] = o
            o += 4 * 6
        if episode_R and name == "weapon":
            o += o & 4
            L["ep_run"], L["ep_bytes"] = o, 8 * episode_R + 8
            o += 8 * episode_R + 8
        L[name] = o
        o += nbytes
    if body_bytes:
        L["body_col"], L["body_bytes"] = o, body_bytes
        o += body_bytes
    L["pad"] = o
    L["rec_bytes"] = (o + 15) // 16 * 16
    return L


_M64 = (1 << 64) - 1

# The words of the six layout calls' out[] (include/zombsole_mi355x.h), by position: Engine._layout zips them with the
# call's output.  None: a reserved word.  A snapshot record's fingerprint comes as two 32-bit halves.
ENTITY_LAYOUT_KEYS = ("row_words", "self", "zombies", "players", "objective", "rays", "ray_cap", "row_bytes")
LAYOUT_KEYS = {
    "zs_obs_state_layout": ("rec_bytes",) + OBS_STATE_SECTIONS + ("pad", "hp_bytes"),
    "zs_snapshot_layout": ("rec_bytes",) + SNAPSHOT_SECTIONS + ("pad", "fingerprint_lo", "fingerprint_hi", "nscal", "ring_words",
                                                                "env_params"),
    "zs_entity_obs_layout": ENTITY_LAYOUT_KEYS,
    "zs_episode_stats_layout": ("R", "last_words", "tot_words", "ep_run", "ep_bytes", None, None, None),
    "zs_render_layout": ("height", "width", "frame_bytes", "cell", "mask", "palette", "body_bytes", "body_col"),
    "zs_host_layout": ("words", "rew", "alog", "dlog", "state", "obs", "obs_bytes", "R"),
}

ENTITY_KMAX, ENTITY_RAY_CAP = 16, 16
# the entity action table (csrc/zs_entity_act.hpp): the words of zs_entity_act_table's out[] (None: reserved)
ENTITY_ACT_TABLE_KEYS = ("nid", "row_bytes", "attack_dir", "heal_dir", "zombie_rows", "player_rows", "end", None)
# path-distance fields (csrc/zs_nav.hpp): the field bits, the largest cap, the words of zs_nav_plan's out[]
NAV_OBJECTIVE, NAV_ZOMBIES, NAV_MAX_DIST, NAV_ROW_WORDS = 1, 2, 32766, 8
NAV_PLAN_KEYS = ("F", "row_words", "field0", "field1", "envs_per_wg", "block", "lds_bytes", "env_bytes")


def entity_layout(kz, kp):
    """zs_entity_obs_layout on the host: the int16 row of an entity observation with kz zombie rows (1..16) and kp
    player rows (0..16), as a dict of ENTITY_LAYOUT_KEYS (word offsets; "row_bytes" = 2 * "row_words")."""
    kz, kp = int(kz), int(kp)
    if not (1 <= kz <= ENTITY_KMAX and 0 <= kp <= ENTITY_KMAX):
        raise ValueError("entity observation: kz must be in 1..16 and kp in 0..16")
    words = 16 + 4 * (kz + kp)
    return dict(zip(ENTITY_LAYOUT_KEYS, (words, 0, 8, 8 + 4 * kz, 8 + 4 * (kz + kp), 12 + 4 * (kz + kp), ENTITY_RAY_CAP,
                                         2 * words)))


def _fp_add(h, v):
    z = ((h ^ (v & _M64)) + 0x9E3779B97F4A7C15) & _M64
    z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & _M64
    z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & _M64
    return z ^ (z >> 31)


def _fp_table(h, values):
    h = _fp_add(h, len(values))
    for v in values:
        h = _fp_add(h, int(v) & 0xffffffff)
    return h


def snapshot_fingerprint(cfg):
    """Mirror of snapshot_fingerprint() (csrc/zs_snapshot.hpp) over a zs_config: handles whose fingerprints agree
    can exchange snapshot records."""
    m = cfg.map
    Z = max(cfg.initial_zombies, cfg.minimum_zombies)
    h = 0x7A735F736E617031
    h = _fp_table(h, [m.width, m.height, m.n_obstacles, cfg.num_agents + cfg.num_bots + Z, cfg.num_agents, cfg.num_bots,
                      Z, cfg.rules, cfg.reward_mode, cfg.max_episode_steps, cfg.initial_zombies, cfg.minimum_zombies])
    h = _fp_table(h, m.obstacle_xy[:2 * m.n_obstacles])
    h = _fp_table(h, m.obstacle_kind[:m.n_obstacles])
    h = _fp_table(h, m.player_spawn_xy[:2 * m.n_player_spawns])
    h = _fp_table(h, m.zombie_spawn_xy[:2 * m.n_zombie_spawns])
    h = _fp_table(h, m.objective_xy[:2 * m.n_objectives])
    h = _fp_table(h, cfg.agent_weapons[:cfg.num_agents])
    h = _fp_table(h, cfg.bot_types[:cfg.num_bots])
    if cfg.flags & FLAG_ENV_PARAMS:  # the longer record: flagged and unflagged handles do not exchange records
        h = _fp_add(h, FLAG_ENV_PARAMS)
    if cfg.flags & FLAG_EPISODE_STATS:
        h = _fp_add(h, FLAG_EPISODE_STATS)
    if cfg.flags & FLAG_RENDER:
        h = _fp_add(h, FLAG_RENDER)
    return h


LAUNCH_FIELDS = ["fused", "fobs", "tick_waves", "lds_budget", "rw_need", "reset_wgs", "reset_stream", "reset_lists",
                 "reset_grid", "defer_respawn", "respawn_grid", "obs_pipe", "obs_lds", "obs_patch", "obs_ring",
                 "obs_ring_patch", "obs_gather", "obs_gather_stat", "obs_stat", "obs_win", "obs_wgs", "par_exec"]


class zs_launch(C.Structure):
    """Launch overrides (include/zombsole_mi355x.h): 0 = automatic; switches 1 = on, -1 = off."""
    _fields_ = [(f, C.c_int32) for f in LAUNCH_FIELDS] + [("reserved", C.c_int32 * 10)]


class zs_config(C.Structure):
    _fields_ = [("num_envs", C.c_int32), ("map", zs_map_desc), ("rules", C.c_int32),
                ("num_agents", C.c_int32), ("agent_weapons", C.POINTER(C.c_int32)),
                ("agent_codes", C.POINTER(C.c_int32)),
                ("num_bots", C.c_int32), ("bot_types", C.POINTER(C.c_int32)),
                ("initial_zombies", C.c_int32), ("minimum_zombies", C.c_int32),
                ("reward_mode", C.c_int32), ("obs_scope", C.c_int32), ("obs_encoding", C.c_int32),
                ("obs_width", C.c_int32), ("obs_dtype", C.c_int32),
                ("max_episode_steps", C.c_int32), ("flags", C.c_uint32), ("lanes_per_env", C.c_int32),
                ("launch", C.POINTER(zs_launch))]


# Every call of the C ABI (include/zombsole_mi355x.h, in its order) with its argtypes; engine.load_library binds them.
# The restype is c_int (a ZS_* status) for all but zs_last_error, which returns the message as c_char_p.
# tests/test_abi.py holds the names and the parameter counts to the header.
_vp, _i32, _u64 = C.c_void_p, C.c_int32, C.c_uint64
_pi32, _pu32 = C.POINTER(C.c_int32), C.POINTER(C.c_uint32)
ABI = {
    "zs_last_error": [],
    "zs_create": [_vp, C.c_int, C.POINTER(_vp)],
    "zs_destroy": [_vp],
    "zs_obs_shape": [_vp, _pi32],
    "zs_seed": [_vp, _i32, _i32, C.POINTER(_u64), _vp],
    "zs_reset": [_vp, _vp, _vp, _vp],
    "zs_observe": [_vp, _vp, _vp, _vp],
    "zs_step": [_vp] * 9,
    "zs_gen_actions": [_vp, _u64, _i32, _vp, _vp],
    "zs_step_graph": [_vp, _u64, _i32] + [_vp] * 8,
    "zs_step_graph_n": [_vp, _u64, _i32, _i32] + [_vp] * 8,
    "zs_state_size": [_vp, _pi32],
    "zs_get_state": [_vp, _i32, _vp, _vp],
    "zs_set_state": [_vp, _i32, _vp, _vp],
    "zs_get_rng": [_vp, _i32, _vp, _vp],
    "zs_set_rng": [_vp, _i32, _vp, _vp],
    "zs_overflow": [_vp, _pu32, _i32, _vp],
    "zs_obs_state_layout": [_vp, _pi32],
    "zs_obs_state_pack": [_vp, _vp, _vp],
    "zs_obs_state_unpack": [_vp, _vp, _i32, _i32, _i32, _vp],
    "zs_snapshot_layout": [_vp, _pi32],
    "zs_snapshot": [_vp, _vp, _i32, _vp, _vp],
    "zs_restore": [_vp, _vp, _i32, _i32, _vp, _vp, _i32, _vp],
    "zs_action_mask": [_vp, _vp, _vp, _vp],
    "zs_action_mask_bind": [_vp, _vp],
    "zs_entity_obs_layout": [_vp, _i32, _i32, _pi32],
    "zs_entity_obs": [_vp, _vp, _i32, _i32, _vp, _vp],
    "zs_entity_obs_bind": [_vp, _vp, _i32, _i32],
    "zs_entity_act_table": [_vp, _i32, _i32, _pi32],
    "zs_entity_act_decode": [_vp, _vp, _i32, _i32, _vp, _vp, _vp],
    "zs_entity_act_mask": [_vp, _vp, _i32, _i32, _vp, _vp],
    "zs_entity_act_encode": [_vp, _vp, _i32, _i32, _vp, _vp, _vp],
    "zs_entity_act_bind": [_vp, _vp, _vp, _i32, _i32],
    "zs_nav_plan": [_vp, _i32, _pi32],
    "zs_nav_obs": [_vp, _vp, _i32, _i32, _vp, _vp],
    "zs_nav_field": [_vp, _vp, _i32, _i32, _i32, _vp, _vp],
    "zs_nav_bind": [_vp, _vp, _i32, _i32],
    "zs_autopilot": [_vp, _vp, _vp, _vp, _vp],
    "zs_autopilot_bind": [_vp, _vp, _vp],
    "zs_env_params_set": [_vp, _vp, _i32, _vp, _vp],
    "zs_env_params_get": [_vp, _i32, _vp, _vp],
    "zs_env_params_check": [_vp, _pu32, _vp],
    "zs_episode_stats_layout": [_vp, _pi32],
    "zs_episode_stats_get": [_vp] * 8,
    "zs_episode_stats_clear": [_vp, _vp, _vp],
    "zs_render_layout": [_vp, _pi32],
    "zs_render": [_vp, _vp, _i32, _vp, _i32, _vp],
    "zs_render_sprites": [_vp, _vp, _vp],
    "zs_profile": [_vp, _i32],
    "zs_profile_read": [_vp, C.POINTER(C.c_double)],
    "zs_describe": [_vp, C.c_char_p, _i32],
    "zs_debug_lists": [_vp, _pi32, _vp],
    "zs_death_log": [_vp, _i32, _pi32, _i32, _pi32, _vp],
    "zs_action_log": [_vp, _i32, _pi32, _i32, _pi32, _vp],
    "zs_host_layout": [_vp, _pi32],
    "zs_host_step": [_vp, _vp, _vp, _vp, _vp],
    "zs_host_reset": [_vp, _vp, _vp, _vp],
    "zs_host_observe": [_vp, _vp, _vp],
    "zs_debug_stamps": [_vp, _vp, _vp, _i32],
    "zs_debug_timeline": [_vp, _vp, _i32],
    "zs_debug_stamps_wg": [_vp, _vp, _i32, _i32],
}


def rules_id(rules_name):
    """RulesFactory.create_rules (rules/factory.py:9-19)."""
    if rules_name in _RULES:
        return _RULES[rules_name]
    raise ValueError(f"{rules_name} is not a valid rule name.  Valid options are extermination, "
                     "survival, evacuation, and safehouse")


def weapon_id(weapon_name):
    """WeaponFactory.create_player_weapon (weapons.py:28-45)."""
    w = _WEAPONS.get(str(weapon_name).lower())
    if w is None:
        raise ValueError(f"{weapon_name} is not a valid player weapon name.  Valid options are knife, "
                         "axe, gun, rifle, shotgun, and random.")
    return w


def bot_id(name):
    """create_player -> __import__('zombsole.players.' + name) (game.py:17-32)."""
    if name in _BOTS:
        return _BOTS[name]
    if name == "me":
        raise NotImplementedError("the interactive keyboard player 'me' blocks on input() and "
                                  "cannot run in a batched engine (SURVEY.md §2)")
    raise ModuleNotFoundError("No module named 'zombsole.players.%s'" % name)


def expand_weapons(agent_weapons, n_agents):
    """Game.__process_weapon_name_inputs__ (game.py:142-149)."""
    if isinstance(agent_weapons, str):
        names = [agent_weapons] * n_agents
    elif isinstance(agent_weapons, list):
        names = [agent_weapons[i % len(agent_weapons)] for i in range(n_agents)] if agent_weapons else []
        if len(names) < n_agents:
            names = names  # islice(cycle([])) yields nothing; zip() then truncates agents
    else:
        raise ValueError(f"{agent_weapons} is not a valid value for argument agent_weapons.  Value must "
                         "be the weapon name as a string or a list of weapon names.")
    return names


def parse_scope(scope):
    """build_observation scope parsing (gym/observation.py:176-192) -> (OBS_*, width)."""
    lscope = scope.lower()
    if lscope in ["world", "map"]:
        return OBS_WORLD, 0
    if lscope.startswith("surroundings"):
        width = int(lscope[len("surroundings:"):])
        if (width % 2 == 0) or (width <= 1):
            raise ValueError("surroundings width must be an odd number greater than 1")
        return OBS_SURROUNDINGS, width
    raise ValueError(f"{scope} is not a valid observation scope, must be \"world\", \"map\", or of the "
                     "form \"surroundings:i\" where i is an integer")


def parse_encoding(style):
    lpes = style.lower()
    if lpes not in ["simple", "channels"]:
        raise ValueError(f"{lpes} must be \"simple\" or \"channels\"")
    return ENC_SIMPLE if lpes == "simple" else ENC_CHANNELS


def agent_code(agent_id):
    """Channels code of an agent: 8 + int(agent_id) (gym/observation.py:59-60).

    The reference evaluates int(agent_id) lazily in the encoder; ids that do
    not convert get code -1 here and the wrapper raises the reference's
    ValueError when a channels observation is produced."""
    try:
        return 8 + int(agent_id)
    except (TypeError, ValueError):
        return -1


class ConfigBuilder(object):
    """Owns the numpy arrays a zs_config points into."""

    def __init__(self, num_envs, map_, rules, agent_weapons, agent_codes, bot_types, initial_zombies,
                 minimum_zombies, reward_mode, obs_scope, obs_encoding, obs_width, obs_dtype,
                 max_episode_steps=0, autoreset=True, lanes_per_env=0, debug=False, viewer=False, env_params=False,
                 episode_stats=False, render=False):
        m = map_ if isinstance(map_, Map) else load_map(map_)
        self.map = m

        def xy(lst):
            a = np.asarray(lst, dtype=np.int32).reshape(-1, 2)
            return np.ascontiguousarray(a)

        self._obst_xy = xy([o[:2] for o in m.obstacles])
        self._obst_kind = np.ascontiguousarray(np.asarray([o[2] for o in m.obstacles], dtype=np.uint8))
        self._obj = xy(m.objectives)
        self._ps = xy(m.player_spawns)
        self._zs = xy(m.zombie_spawns)
        self._aw = np.ascontiguousarray(np.asarray(agent_weapons, dtype=np.int32))
        self._ac = np.ascontiguousarray(np.asarray(agent_codes, dtype=np.int32))
        self._bt = np.ascontiguousarray(np.asarray(bot_types, dtype=np.int32))
        p32 = lambda a: a.ctypes.data_as(C.POINTER(C.c_int32))  # noqa: E731
        md = zs_map_desc(m.size[0], m.size[1], len(m.obstacles), p32(self._obst_xy),
                         self._obst_kind.ctypes.data_as(C.POINTER(C.c_uint8)),
                         len(m.objectives), p32(self._obj), len(m.player_spawns), p32(self._ps),
                         len(m.zombie_spawns), p32(self._zs))
        self.cfg = zs_config(int(num_envs), md, int(rules), len(self._aw), p32(self._aw), p32(self._ac),
                             len(self._bt), p32(self._bt), int(initial_zombies), int(minimum_zombies),
                             int(reward_mode), int(obs_scope), int(obs_encoding), int(obs_width),
                             int(obs_dtype), int(max_episode_steps),
                             (FLAG_AUTORESET if autoreset else 0) | (FLAG_DEBUG if debug else 0) |
                             (FLAG_VIEWER if viewer else 0) | (FLAG_ENV_PARAMS if env_params else 0) |
                             (FLAG_EPISODE_STATS if episode_stats else 0) |
                             ((FLAG_RENDER | FLAG_DEATH_LOG) if render else 0),
                             int(lanes_per_env))
        self._launch = None

    def set_launch(self, overrides):
        """Force launch alternatives for the handles built from this config: a dict of zs_launch fields
        (LAUNCH_FIELDS), e.g. {"fused": -1, "obs_ring": 1}; None or {} = every choice automatic."""
        if not overrides:
            self._launch = None
            self.cfg.launch = C.POINTER(zs_launch)()
            return self
        unknown = set(overrides) - set(LAUNCH_FIELDS)
        if unknown:
            raise ValueError("unknown launch overrides: %s" % sorted(unknown))
        self._launch = zs_launch(**{k: int(v) for k, v in overrides.items()})
        self.cfg.launch = C.pointer(self._launch)
        return self

    @property
    def launch(self):
        """The overrides set on this config, as a dict of the non-zero fields."""
        if self._launch is None:
            return {}
        return {f: getattr(self._launch, f) for f in LAUNCH_FIELDS if getattr(self._launch, f)}

    def viewer(self, num_envs):
        """The config of a viewer handle (FLAG_VIEWER) for num_envs envs of this config's map, entities and
        observations (it shares this builder's arrays)."""
        import copy
        b = copy.copy(self)
        b.cfg = zs_config.from_buffer_copy(self.cfg)
        b.cfg.num_envs = int(num_envs)
        b.cfg.flags |= FLAG_VIEWER
        return b

    def obs_state_layout(self):
        """The observation-state record of this config's handles (zs_obs_state_layout without a device)."""
        c, m = self.cfg, self.cfg.map
        E = c.num_agents + c.num_bots + max(c.initial_zombies, c.minimum_zombies)
        return obs_state_layout(E, m.n_obstacles, (m.width * m.height + 31) // 32, (m.n_obstacles + 31) // 32,
                                obs_state_record_dtype(c.obs_dtype, c.obs_encoding))

    def snapshot_layout(self):
        """The snapshot record of this config's handles (zs_snapshot_layout without a device), with "fingerprint"."""
        c, m = self.cfg, self.cfg.map
        E = c.num_agents + c.num_bots + max(c.initial_zombies, c.minimum_zombies)
        L = snapshot_layout(E, m.n_obstacles, (m.width * m.height + 31) // 32, (m.n_obstacles + 31) // 32, c.num_agents,
                            bool(c.flags & FLAG_ENV_PARAMS),
                            (c.num_agents if c.reward_mode == REWARD_MULTI else 1) if c.flags & FLAG_EPISODE_STATS else 0,
                            ((m.width * m.height + 15) & ~15) if c.flags & FLAG_RENDER else 0)
        L["fingerprint"] = snapshot_fingerprint(c)
        return L

    @property
    def num_agents(self):
        return len(self._aw)

    @property
    def num_bots(self):
        return len(self._bt)

    def obs_shape(self):
        """(obs per env, C, H, W) — mirrors zs_obs_shape."""
        c = self.cfg
        chans = 3 if c.obs_encoding == ENC_CHANNELS else 1
        if c.obs_scope == OBS_WORLD:
            h, w = c.map.height, c.map.width
        else:
            h = w = c.obs_width
        n = c.num_agents if (c.reward_mode == REWARD_MULTI and c.obs_scope == OBS_SURROUNDINGS) else 1
        return (n, chans, h, w)

    def ptr(self):
        return C.byref(self.cfg)


def single_env_config(num_envs, rules_name, player_names, map_name, agent_id, initial_zombies=0,
                      minimum_zombies=0, observation_scope="world", observation_position_encoding="simple",
                      agent_weapon="rifle", max_episode_steps=0, obs_dtype=DTYPE_I32, autoreset=True,
                      lanes_per_env=0, debug=False, viewer=False, env_params=False, episode_stats=False, render=False):
    """zs_config for the ZombsoleGymEnv surface (gym_env.py:49-83): one agent + bots."""
    m = load_map(map_name)
    rules = rules_id(rules_name)
    bots = [bot_id(n) for n in player_names]
    weapons = [weapon_id(w) for w in expand_weapons([agent_weapon], 1)]
    scope, width = parse_scope(observation_scope)
    enc = parse_encoding(observation_position_encoding)
    return ConfigBuilder(num_envs, m, rules, weapons, [agent_code(agent_id)], bots, initial_zombies,
                         minimum_zombies, REWARD_SINGLE, scope, enc, width, obs_dtype, max_episode_steps,
                         autoreset, lanes_per_env, debug, viewer, env_params, episode_stats, render)


def multi_env_config(num_envs, rules_name, player_names, map_name, agent_ids, initial_zombies=0,
                     minimum_zombies=0, observation_surroundings_width=21,
                     observation_position_encoding_style="channels", agent_weapons="rifle",
                     max_episode_steps=0, obs_dtype=DTYPE_I64, autoreset=True, lanes_per_env=0, debug=False,
                     viewer=False, env_params=False, episode_stats=False, render=False):
    """zs_config for the MultiagentZombsoleEnv surface (gym/multiagent_env.py:25-78)."""
    w = int(observation_surroundings_width)
    if (w % 2 == 0) or (w <= 1):
        raise ValueError("surroundings width must be an odd number greater than 1")
    enc = parse_encoding(observation_position_encoding_style)
    m = load_map(map_name)
    rules = rules_id(rules_name)
    bots = [bot_id(n) for n in player_names]
    names = expand_weapons(agent_weapons, len(agent_ids))
    ids = list(agent_ids)[:len(names)]  # zip(agent_ids, agent_weapons) truncates (game.py:162-163)
    weapons = [weapon_id(n) for n in names]
    return ConfigBuilder(num_envs, m, rules, weapons, [agent_code(a) for a in ids], bots, initial_zombies,
                         minimum_zombies, REWARD_MULTI, OBS_SURROUNDINGS, enc, w, obs_dtype,
                         max_episode_steps, autoreset, lanes_per_env, debug, viewer, env_params, episode_stats, render)
