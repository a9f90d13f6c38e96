"""One case per observation-kernel instantiation (libzombsole_amd/csrc/k_obs_t.hip): six store-stream / gather
variants x three output types x 1, 2 or 4 observations per env, and k_obs x three output types: 57 device
functions.  test_obs_instantiations_plan.py checks on the CPU that every row's (config, overrides) resolves to
the instantiation it claims (obs_plan(), zs_obs_plan.hpp) and that the rows and the UNREACHABLE list together are
the 57; test_obs_instantiations.py runs every row on the GPU.

The names below are written down from reading obs_plan(), not produced by running it:

  * every config here is the registered shape (surroundings of width 21, channels encoding, a small map in
    rank order with obstacles, at most 64 entities), so `pipe` holds unless obs_pipe = -1;
  * obs_lds = 1 takes the staged kernels at any env count; obs_ring = -1 then leaves k_obs_patch, obs_ring = 1
    takes k_obs_ring, with k_obs_patch's encoders ("patched") unless obs_ring_patch = -1 ("select");
    obs_lds = -1 keeps k_obs_pipe.  Their masked launches run k_obs, told the observation count;
  * obs_pipe = -1 takes k_obs_gather (masked launches too), and k_obs_pbring for the unmasked ones unless
    obs_ring = -1; with obs_gather = -1 as well, k_obs (observation count 0: it reads the count from the config);
  * without `pipe` the small image would be written by the step launch itself: fobs = -1 keeps the kernel.
"""
from libzombsole_amd import _abi
from libzombsole_amd.maps import Map

from obs_plan_table import WALL_HP_MAP

DTYPES = {"i64": _abi.DTYPE_I64, "i32": _abi.DTYPE_I32, "i16": _abi.DTYPE_I16}
AGENTS = {1: ["0"], 2: ["0", "1"], 4: ["0", "1", "2", "3"]}

# variant -> (zs_launch overrides, obs_kernel, obs_kernel_masked, obs_encoders, plan kind, patched)
VARIANTS = {
    "ring_patched": ({"obs_lds": 1, "obs_ring": 1}, "k_obs_ring", "k_obs", "patched", 4, 1),
    "ring_select": ({"obs_lds": 1, "obs_ring": 1, "obs_ring_patch": -1}, "k_obs_ring", "k_obs", "select", 4, 0),
    "pbring": ({"fobs": -1, "obs_pipe": -1}, "k_obs_pbring", "k_obs_gather", "", 5, 0),
    "patch": ({"obs_lds": 1, "obs_ring": -1}, "k_obs_patch", "k_obs", "", 3, 0),
    "pipe": ({"obs_lds": -1}, "k_obs_pipe", "k_obs", "", 2, 0),
    "gather": ({"fobs": -1, "obs_pipe": -1, "obs_ring": -1}, "k_obs_gather", "k_obs_gather", "", 1, 0),
    "k_obs": ({"fobs": -1, "obs_pipe": -1, "obs_gather": -1}, "k_obs", "k_obs", "", 0, 0),
}
# the plan's observation count of the masked launch: the config's count, except under k_obs's own overrides (0)
MASKED_KIND = {"k_obs": 0, "k_obs_gather": 1}
# Launch geometry, by hand from the kernels' shape: envs per workgroup and threads.  The rings walk units of one env,
# or of two where one env's block (observations x 1323 elements) ends off a 16-B boundary and two end on one
# (ring_pair): int64 x 1 (10 584 B), int32 x 2 (10 584 B) and int16 x 4 (10 584 B); 12 + 3 and 10 + 2 waves.
# k_obs_patch: eight waves, one env each; the others four.  No row has more than 130 envs, so no grid meets its cap.
UNIT_ENVS = {("i64", 1): 2, ("i32", 2): 2, ("i16", 4): 2}
GEOMETRY = {"ring_patched": (None, 960), "ring_select": (None, 960), "pbring": (None, 768), "patch": (8, 512),
            "pipe": (4, 256), "gather": (4, 256), "k_obs": (4, 256)}


def bridge64(n, dtype, nobs):
    """Real window content: zombies, boxes, dead bodies; episodes of 12 steps, so autoresets happen."""
    return _abi.multi_env_config(n, "extermination", [], "bridge64", AGENTS[nobs], initial_zombies=12,
                                 minimum_zombies=0, obs_dtype=dtype, max_episode_steps=12)


# WALL_HP_MAP has two player spawns; four agents need four (Game.__initialize_world__ raises "Not enough space to
# spawn" otherwise): the same walls with the two floor cells beside the centre one as spawns too
WALL_HP_MAP_4 = "wwwww\nwpwpw\nwp.pw\nwwwww\n"


def wall_hp(n, dtype, nobs):
    """The 5 x 4 map of test_obstacle_hp.py: windows mostly off-map padding, walls the agents damage, every
    episode over at its first step (no zombies)."""
    text, name = (WALL_HP_MAP_4, "wall_hp4") if nobs == 4 else (WALL_HP_MAP, "wall_hp")
    return _abi.multi_env_config(n, "extermination", [], Map.from_text(text, name=name), AGENTS[nobs],
                                 initial_zombies=0, minimum_zombies=0, obs_dtype=dtype)


MAPS = {"bridge64": bridge64, "wall_hp": wall_hp}

# (variant, dtype, observations) -> (map, env count).  Env counts: odd, and no multiple of the four waves of a
# workgroup or of k_obs_patch's eight (67, 37, 129, 13); 130 = 2 x 65 for an even count that is neither.  Where
# two envs make one ring unit (ring_pair = 2: int64 x 1, int32 x 2, int16 x 4) the count is odd, so the last
# unit holds a lone env.  int16 x 1 envs (2 646 B) start at every even 16-B phase from 8 envs on.
_ROWS = {
    # k_obs_ring, padded-table encoders
    ("ring_patched", "i64", 1): ("bridge64", 67), ("ring_patched", "i64", 2): ("wall_hp", 37),
    ("ring_patched", "i32", 1): ("wall_hp", 67), ("ring_patched", "i32", 2): ("bridge64", 37),
    ("ring_patched", "i16", 1): ("bridge64", 67), ("ring_patched", "i16", 2): ("wall_hp", 130),
    ("ring_patched", "i16", 4): ("bridge64", 37),
    # k_obs_ring, select-chain encoders
    ("ring_select", "i64", 1): ("wall_hp", 129), ("ring_select", "i64", 2): ("bridge64", 37),
    ("ring_select", "i32", 1): ("bridge64", 67), ("ring_select", "i32", 2): ("wall_hp", 67),
    ("ring_select", "i16", 1): ("wall_hp", 67), ("ring_select", "i16", 2): ("bridge64", 37),
    ("ring_select", "i16", 4): ("wall_hp", 13),
    # k_obs_pbring
    ("pbring", "i64", 1): ("bridge64", 67), ("pbring", "i64", 2): ("wall_hp", 130), ("pbring", "i64", 4): ("bridge64", 13),
    ("pbring", "i32", 1): ("wall_hp", 67), ("pbring", "i32", 2): ("bridge64", 37), ("pbring", "i32", 4): ("wall_hp", 37),
    ("pbring", "i16", 1): ("bridge64", 67), ("pbring", "i16", 2): ("wall_hp", 67), ("pbring", "i16", 4): ("bridge64", 37),
    # k_obs_patch
    ("patch", "i64", 1): ("wall_hp", 67), ("patch", "i64", 2): ("bridge64", 37), ("patch", "i64", 4): ("wall_hp", 13),
    ("patch", "i32", 1): ("bridge64", 67), ("patch", "i32", 2): ("wall_hp", 130), ("patch", "i32", 4): ("bridge64", 37),
    ("patch", "i16", 1): ("bridge64", 129), ("patch", "i16", 2): ("bridge64", 37), ("patch", "i16", 4): ("wall_hp", 67),
    # k_obs_pipe
    ("pipe", "i64", 1): ("bridge64", 67), ("pipe", "i64", 2): ("wall_hp", 67), ("pipe", "i64", 4): ("bridge64", 13),
    ("pipe", "i32", 1): ("wall_hp", 130), ("pipe", "i32", 2): ("bridge64", 37), ("pipe", "i32", 4): ("bridge64", 37),
    ("pipe", "i16", 1): ("bridge64", 67), ("pipe", "i16", 2): ("wall_hp", 37), ("pipe", "i16", 4): ("bridge64", 37),
    # k_obs_gather
    ("gather", "i64", 1): ("wall_hp", 67), ("gather", "i64", 2): ("bridge64", 37), ("gather", "i64", 4): ("wall_hp", 37),
    ("gather", "i32", 1): ("bridge64", 67), ("gather", "i32", 2): ("wall_hp", 67), ("gather", "i32", 4): ("bridge64", 13),
    ("gather", "i16", 1): ("wall_hp", 129), ("gather", "i16", 2): ("bridge64", 37), ("gather", "i16", 4): ("bridge64", 37),
    # k_obs (one function per output type; the observation count is the config's)
    ("k_obs", "i64", 0): ("bridge64", 37), ("k_obs", "i32", 0): ("wall_hp", 67), ("k_obs", "i16", 0): ("bridge64", 67),
}
# the observations per env of the k_obs rows' configs (their plan count is 0)
K_OBS_AGENTS = {"i64": 4, "i32": 1, "i16": 2}

# Instantiations no config and override reaches, each with the obs_plan() condition that excludes it.
# k_obs_ring's ring is RING_SLOTS / ring_pair unit slots of obs_stage_slot_bytes(ts, nobs * ring_pair) bytes.  Four
# int64 blocks stage as int32: (4 * 1323 + 2) * 4 -> 21 184 B a slot, and four int32 blocks (4 * 1323 + 4) * 4 ->
# 21 184 B; ring_pair is 1 for both (4 * 1323 * ts is a multiple of 16), so the eight slots alone are 169 472 B,
# more than the 160 KiB (163 840 B) the plan allows, whichever encoders the ring has.
_RING_TOO_LARGE = "rb <= 160 * 1024"
UNREACHABLE = {
    ("ring_patched", "i64", 4): _RING_TOO_LARGE, ("ring_select", "i64", 4): _RING_TOO_LARGE,
    ("ring_patched", "i32", 4): _RING_TOO_LARGE, ("ring_select", "i32", 4): _RING_TOO_LARGE,
}


class Row(object):
    def __init__(self, variant, dtype, nobs, map_name, n):
        self.variant, self.dtype_name, self.nobs, self.map_name, self.n = variant, dtype, nobs, map_name, n
        self.dtype = DTYPES[dtype]
        self.launch, self.obs_kernel, self.obs_kernel_masked, self.obs_encoders, self.kind, self.patched = VARIANTS[variant]
        self.agents = nobs or K_OBS_AGENTS[dtype]  # observations per env of the config
        self.masked_kind = MASKED_KIND[self.obs_kernel_masked]
        self.masked_nobs = 0 if variant == "k_obs" else nobs
        per_wg, self.block = GEOMETRY[variant]
        self.envs_per_wg = per_wg or UNIT_ENVS.get((dtype, nobs), 1)
        self.grid = (n + self.envs_per_wg - 1) // self.envs_per_wg
        self.id = "%s-%s-x%d-%s@%d" % (variant, dtype, nobs, map_name, n)

    def builder(self, n=None):
        return MAPS[self.map_name](self.n if n is None else n, self.dtype, self.agents)


ROWS = [Row(v, dt, nobs, m, n) for (v, dt, nobs), (m, n) in _ROWS.items()]


def all_instantiations():
    """The 57 (variant, dtype, observations) of k_obs_t.hip's launch_nb<1|2|4> and k_obs<TT>."""
    keys = [(v, dt, nobs) for v in VARIANTS if v != "k_obs" for dt in DTYPES for nobs in (1, 2, 4)]
    return keys + [("k_obs", dt, 0) for dt in DTYPES]
