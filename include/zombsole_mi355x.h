/*
 * zombsole_mi355x.h — C ABI of the MI355X-native batched zombsole step engine.
 *
 * The reference (jvstinian/libzombsole) has no FFI: its boundary is the Python
 * class surface ZombsoleGymEnv / MultiagentZombsoleEnv, whose per-tick work is
 * `World.step` plus the env glue.  This header is the seam
 * a maintainer binds from that surface (see INTEGRATION.md for the ctypes
 * stub).  Each entry point names the reference code it replaces:
 *
 *   zs_create      <- ZombsoleGymEnv.__init__ / MultiagentZombsoleEnv.__init__
 *                     (zombsole/gym_env.py:49-83, zombsole/gym/multiagent_env.py:25-78)
 *                     + Game.__init__ (zombsole/game.py:115-140), N envs at once
 *   zs_seed        <- random.seed(s) on the process-global CPython MT19937 the
 *                     reference draws from (/usr/lib/python3.10/random.py:128-168);
 *                     here one independent stream per env
 *   zs_reset       <- env.reset() -> Game.__initialize_world__ + reward reset + obs
 *                     (gym_env.py:148-164, gym/multiagent_env.py:173-184, game.py:151-169)
 *   zs_step        <- env.step(action) (gym_env.py:99-145, gym/multiagent_env.py:111-171):
 *                     set_action, World.step (core.py:72-78), rewards (gym/reward.py),
 *                     respawn (game.py:196-201), observation (gym/observation.py),
 *                     rules (zombsole/rules/{...}.py)
 *   zs_get_state / zs_set_state
 *                  <- the test pokes env.game.world.things, env.game.agents[i].life = x
 *                     (tests/test_game.py:55,105, tests/test_multiagent_env.py:108)
 *   zs_observe     <- env.get_observation() (gym_env.py:93-94)
 *   zs_get_rng / zs_set_rng
 *                  <- random.getstate()/setstate(): the process-global stream the
 *                     reference's World/Game draw from (core.py:2, things.py:2, game.py)
 *   zs_gen_actions <- (bench/parity only) the uniform discrete policy of SURVEY.md §8(d)
 *
 * Conventions: plain C types only; device buffers are raw HIP device pointers,
 * `stream` is a hipStream_t passed as void*.  The engine owns its device
 * state; the caller owns every output buffer.  All calls on one handle are
 * serialized on the stream they are given.  Return value 0 = ok, otherwise a
 * ZS_E* code with a message in zs_last_error() (thread-local).
 *
 * Streams.  Every launch, copy and memset of a call goes to the `stream` it is given (the next-step reset
 * work of zs_step may run on a stream of the handle's own, forked from `stream` and joined to it inside the
 * call).  A call that takes device buffers only returns without waiting for the device: zs_observe, zs_step,
 * zs_gen_actions, zs_obs_state_pack / _unpack, zs_snapshot, zs_restore, zs_action_mask, zs_entity_obs,
 * zs_entity_act_decode / _mask / _encode, zs_nav_obs, zs_nav_field, zs_autopilot, zs_env_params_set / _get, zs_episode_stats_get / _clear, zs_render.
 * A call that hands a host value back, or reads a host buffer, waits for `stream` (and for nothing else)
 * before it returns: zs_seed, zs_reset (its error word), zs_get_state / zs_set_state, zs_get_rng / zs_set_rng,
 * zs_overflow, zs_env_params_check, zs_debug_lists, zs_death_log, zs_action_log and the zs_host_* calls.
 * zs_step_graph(_n) waits for `stream` in the call that captures a buffer set, and only launches the graph
 * when it finds the set cached.  The calls without a stream that change what a step launches wait for the
 * whole device: the zs_*_bind calls when the binding changes (none when it is the one in place) and
 * zs_render_sprites; zs_profile_read waits for its own events.
 * The handle's scratch (the state and seed staging rows, the error word, zs_env_params_set's row, the step
 * counter of zs_step_graph) is shared by all its calls: a caller that moves to another stream orders that
 * stream after the previous call with an event of its own, and two calls of one handle in flight on streams
 * that are not ordered are not supported.
 */
#ifndef ZOMBSOLE_MI355X_H
#define ZOMBSOLE_MI355X_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* ---- status codes (mapped to Python exceptions by the wrapper) --------- */
#define ZS_OK 0
#define ZS_EINVAL 1    /* -> ValueError                                   */
#define ZS_ENOSPACE 2  /* -> Exception('Not enough space to spawn ...') core.py:62-64 */
#define ZS_EHIP 3      /* -> RuntimeError (HIP failure)                    */
#define ZS_ESTATE 4    /* -> RuntimeError (bad call order / index)         */

/* ---- thing kinds: the observation codes of gym/observation.py:18-26 ---- */
#define ZS_THING_NONE 0
#define ZS_THING_BOX 1
#define ZS_THING_DEADBODY 2
#define ZS_THING_OBJECTIVE 3
#define ZS_THING_WALL 4
#define ZS_THING_ZOMBIE 5
#define ZS_THING_PLAYER 6 /* scripted bot (players/{...}.py)          */
#define ZS_THING_AGENT 7  /* RL agent (players/agent.py)          */

/* ---- weapons: the codes of gym/observation.py:27-34; table weapons.py:18-25 */
#define ZS_WEAPON_NONE 0
#define ZS_WEAPON_CLAWS 1
#define ZS_WEAPON_KNIFE 10
#define ZS_WEAPON_AXE 11
#define ZS_WEAPON_GUN 12
#define ZS_WEAPON_RIFLE 13
#define ZS_WEAPON_SHOTGUN 14
#define ZS_WEAPON_RANDOM 255 /* WeaponFactory 'random' (weapons.py:43-44) */

/* ---- scripted bots (players/{...}.py) -------------------------------------- */
#define ZS_BOT_TERMINATOR 1 /* players/terminator.py */
#define ZS_BOT_SNIPER 2     /* players/sniper.py     */
#define ZS_BOT_TROLL 3      /* players/troll.py      */
#define ZS_BOT_HAMSTER 4    /* players/hamster.py    */
#define ZS_BOT_RANDOMAN 5   /* players/randoman.py   */

/* ---- rules (rules/factory.py:9-19) -------------------------------------- */
#define ZS_RULES_EXTERMINATION 0
#define ZS_RULES_SURVIVAL 1
#define ZS_RULES_EVACUATION 2
#define ZS_RULES_SAFEHOUSE 3

/* ---- agent action kinds (int32 triple kind,dx,dy per agent) -------------
 * dx and dy may be any int32: the target is the agent's cell plus the offset, taken exactly (an offset
 * beyond the map from any cell of it, +-16 384 or more, names no cell: a move goes nowhere, an attack or
 * heal finds nothing).  A caller whose offsets are wider than int32 saturates them to the int32 range. */
#define ZS_ACT_IDLE 0
#define ZS_ACT_MOVE 1
#define ZS_ACT_ATTACK 2
#define ZS_ACT_ATTACK_CLOSEST 3
#define ZS_ACT_HEAL 4
#define ZS_ACT_HEAL_CLOSEST 5
#define ZS_ACT_CONFUSED 6
/* the agent's next_step raises (a debug=True env, core.py:96-99): World.step has advanced t and
 * taken the decisions of the actors before this one in dict order (their RNG draws included), then
 * stops; the env's state is otherwise unchanged and that step reports reward 0, not done, not
 * truncated (the drop-ins re-raise the agent's exception) */
#define ZS_ACT_RAISE 7

/* ---- env surface / observation ------------------------------------------ */
#define ZS_REWARD_SINGLE 0 /* AgentRewards, include_life_in_reward=True (gym/reward.py:19-47) */
#define ZS_REWARD_MULTI 1  /* MultiAgentRewards (gym/reward.py:67-98)                         */
#define ZS_OBS_WORLD 0
#define ZS_OBS_SURROUNDINGS 1
#define ZS_ENC_SIMPLE 0
#define ZS_ENC_CHANNELS 1
#define ZS_DTYPE_I32 0
#define ZS_DTYPE_I64 1
#define ZS_DTYPE_I16 2 /* compact internal form; values fit int16 */

#define ZS_FLAG_AUTORESET 1u /* next-step autoreset: an env that ended is reset by the next zs_step */
#define ZS_FLAG_DEBUG 2u     /* debug=True envs (core.py:96-99, 115-119): action kind ZS_ACT_RAISE
                              * stops World.step; without the flag kinds >= 7 are unknown (idle) */
#define ZS_FLAG_DEATH_LOG 4u /* keep, per env, the things its last step's clean_dead_things removed, in
                              * removal order (zs_death_log; the drop-in views' decoration order and
                              * the final values of a removed zombie whose slot a respawn reuses), and
                              * the actions it executed, in execution order (zs_action_log; the drop-in
                              * views' World.events) */

#define ZS_FLAG_VIEWER 8u    /* a viewer handle: it holds other handles' envs for encoding (zs_obs_state_unpack,
                              * zs_observe).  zs_create allocates it like any other handle.  zs_seed, zs_reset,
                              * zs_step*, zs_gen_actions, zs_set_state, zs_set_rng, zs_restore and the
                              * zs_host_* calls return ZS_ESTATE on it before any launch; zs_observe,
                              * zs_obs_shape, zs_describe, zs_state_size, zs_get_state, zs_overflow, zs_destroy,
                              * zs_snapshot, zs_snapshot_layout and the zs_obs_state_* calls work on it */
#define ZS_FLAG_ENV_PARAMS 16u /* per-env zombie counts and time limits (zs_env_params_set / _get): every env carries
                                * (initial_zombies, minimum_zombies, max_episode_steps) twice, the triple its next
                                * reset takes up and the triple of its running episode; both start as the config's
                                * values, which are the caps.  zs_create refuses it on a viewer handle (ZS_ESTATE) */
#define ZS_FLAG_EPISODE_STATS 32u /* per-env episode statistics kept on the device (zs_episode_stats_*): every zs_step
                                   * ends with one more small launch (k_episode_stats).  Without the flag nothing is
                                   * allocated and nothing is launched.  zs_create refuses it on a viewer handle
                                   * (ZS_ESTATE) */
#define ZS_FLAG_RENDER 64u /* frames of the envs drawn on the device (zs_render*): the handle keeps a body colour per
                            * cell per env, and every zs_step ends with one more small launch (k_render_track).  Needs
                            * ZS_FLAG_DEATH_LOG (zs_create: ZS_EINVAL without it); refused on a viewer handle
                            * (ZS_ESTATE).  Without the flag nothing is allocated and nothing is launched */

/* ---- range flags (zs_overflow) -------------------------------------------
 * The reference's obstacle life is an unbounded Python int that carries over resets
 * (game.py:151-155) and keeps falling each time a destroyed Box/Wall is hit again before
 * the first cleanup of an episode (core.py:72-78, 168-184).  The engine holds it in int32. */
#define ZS_OVF_INT16 1u /* an obstacle life went below -32768: ZS_DTYPE_I16 observations saturate it */
#define ZS_OVF_INT32 2u /* an obstacle life reached -2147483647 and saturated there: from then on
                         * that env differs from the reference */
#define ZS_OVF_PARAM_RANGE 4u /* zs_env_params_set met an entry it did not apply: an env index outside [0, N), or
                               * a value outside its range (the config's value is the cap) */

/* ---- map description (parsed by the host; zombsole/game.py:45-97) ------- */
typedef struct zs_map_desc {
    int32_t width, height;
    int32_t n_obstacles;          /* boxes+walls in map-file (dict insertion) order */
    const int32_t* obstacle_xy;   /* [n_obstacles][2]                               */
    const uint8_t* obstacle_kind; /* ZS_THING_BOX / ZS_THING_WALL                   */
    int32_t n_objectives;
    const int32_t* objective_xy;  /* [n][2], map-file order                          */
    int32_t n_player_spawns;
    const int32_t* player_spawn_xy;
    int32_t n_zombie_spawns;      /* 0 => every cell, x-major (core.py:44-47)        */
    const int32_t* zombie_spawn_xy;
} zs_map_desc;

/* ---- launch overrides ----------------------------------------------------------
 * zs_create picks every kernel and layout from the config and the env count.  A non-NULL
 * zs_config.launch forces one of the alternatives it would pick elsewhere, or sizes a grid (parity
 * tests run every alternative; A/B measurements compare them).  Every field: 0 = automatic.
 * Switches: 1 = on, -1 = off.  The block is copied into the handle: no process-wide state, and
 * no environment variable selects a kernel. */
typedef struct zs_launch {
    int32_t fused;           /* reset work inside the step launch (k_step) instead of its own launch  */
    int32_t fobs;            /* observations written by the step launch itself (the default for small
                              * images without a store-stream kernel; -1 off, 1 on)                    */
    int32_t tick_waves;      /* k_tick's register budget: 5 or 6 waves per SIMD                        */
    int32_t lds_budget;      /* -1: largest optional LDS copies instead of the most resident workgroups */
    int32_t rw_need;         /* RNG window words a plain step prefetches (32..512)                    */
    int32_t reset_wgs;       /* reset-work workgroups of a fused step launch                          */
    int32_t reset_stream;    /* -1: an unfused reset launch on the caller's stream, not a side stream  */
    int32_t reset_lists;     /* -1: k_reset reads the spawn lists from HBM instead of LDS              */
    int32_t reset_grid;      /* k_reset workgroups (pending-list mode)                                 */
    int32_t defer_respawn;   /* 1: zombie respawn by k_respawn, -1: by the tick's leader               */
    int32_t respawn_grid;    /* k_respawn workgroups                                                   */
    int32_t obs_pipe;        /* -1: no prefetching store-stream observation kernel (k_obs_pipe family) */
    int32_t obs_lds;         /* the LDS-staged 16-B store kernels (k_obs_patch, k_obs_ring): -1 keeps
                              * k_obs_pipe, 1 takes them at any env count                              */
    int32_t obs_patch;       /* -1: no padded-table encoder kernel k_obs_patch                         */
    int32_t obs_ring;        /* encoder / writer waves through an LDS ring (k_obs_ring, k_obs_pbring);
                              * -1 keeps k_obs_patch / k_obs_pipe / k_obs_gather                       */
    int32_t obs_ring_patch;  /* -1: k_obs_ring with the select-chain encoders instead of the
                              * padded-table ones (its fallback when the tables do not fit)            */
    int32_t obs_gather;      /* -1: no k_obs_gather (large maps then use k_obs)                        */
    int32_t obs_gather_stat; /* -1: k_obs_gather reads static words from HBM instead of LDS tables     */
    int32_t obs_stat;        /* -1: per-cell static words instead of LDS bitmaps                       */
    int32_t obs_win;         /* -1: per-cell entity scan instead of the window map                     */
    int32_t obs_wgs;         /* observation workgroups per CU (store-stream kernels)                   */
    int32_t par_exec;        /* -1: the leader lane executes the shuffled actions serially instead of
                              * the env's lanes in parallel (core.py:103-119)                          */
    int32_t reserved[10];    /* zero (round 6 removed four switches of alternatives measured slower:
                              * the one-launch step k_fstep and its shapes, the early RNG window in
                              * k_tick, the policy inside the side-stream tick)          */
} zs_launch;

typedef struct zs_config {
    int32_t num_envs;
    zs_map_desc map;
    int32_t rules;                /* ZS_RULES_*                                     */
    int32_t num_agents;
    const int32_t* agent_weapons; /* [num_agents] ZS_WEAPON_* or ZS_WEAPON_RANDOM    */
    const int32_t* agent_codes;   /* [num_agents] channels code = 8 + int(agent_id)  */
    int32_t num_bots;
    const int32_t* bot_types;     /* [num_bots] ZS_BOT_* in player_names order       */
    int32_t initial_zombies;
    int32_t minimum_zombies;
    int32_t reward_mode;          /* ZS_REWARD_*                                     */
    int32_t obs_scope;            /* ZS_OBS_*                                        */
    int32_t obs_encoding;         /* ZS_ENC_*                                        */
    int32_t obs_width;            /* surroundings width (odd, > 1)                   */
    int32_t obs_dtype;            /* ZS_DTYPE_*                                      */
    int32_t max_episode_steps;    /* 0 = none; else TimeLimit-style truncation       */
    uint32_t flags;               /* ZS_FLAG_*                                       */
    int32_t lanes_per_env;        /* k_tick lanes per env: 1, 2, 4, 8, 16, 32 or 64; 0 = auto.  Any other
                                   * value: zs_create returns ZS_EINVAL.  A workgroup of 64 lanes holds
                                   * 64 / lanes_per_env envs in one LDS image of at most 64 KiB; where the
                                   * image of the requested count does not fit even with the smallest
                                   * optional copies, the count is doubled until it does.  zs_describe's
                                   * "lanes_per_env" is the count the handle runs                        */
    const zs_launch* launch;      /* NULL = every launch choice automatic                 */
} zs_config;

typedef struct zs_handle zs_handle;

/* Thread-local message for the last failing call on this thread. */
const char* zs_last_error(void);

/* Validate `cfg`, allocate device state for cfg->num_envs envs on `device`. */
int zs_create(const zs_config* cfg, int device, zs_handle** out);
int zs_destroy(zs_handle* h);

/* Per-env observation shape: out[0] = observations per env (1 for the single
 * surface, num_agents for the multi surface), out[1..3] = C, H, W. */
int zs_obs_shape(const zs_handle* h, int32_t out[4]);

/* CPython random.seed(int) semantics per env, for envs [env0, env0+n).  Host
 * array of n seeds.  Also records the seed as the env's action-stream seed. */
int zs_seed(zs_handle* h, int32_t env0, int32_t n, const uint64_t* seeds_host, void* stream);

/* Reset the envs whose byte in env_mask_dev is nonzero (NULL = all) and write
 * their reset observations into obs_dev (other envs' slices untouched).  A new
 * handle's envs are all pending reset: the first zs_step resets them if zs_reset
 * was not called.  obs_dev may be NULL: the envs are reset and no grid observation is written. */
int zs_reset(zs_handle* h, const uint8_t* env_mask_dev, void* obs_dev, void* stream);

/* Re-encode the observation of the envs whose mask byte is nonzero (NULL = all)
 * from their current state — env.get_observation() (gym_env.py:93-94,
 * gym/multiagent_env.py:87-96), e.g. after a zs_set_state poke. */
int zs_observe(zs_handle* h, const uint8_t* env_mask_dev, void* obs_dev, void* stream);

/* One lock-step tick for every env.
 *   actions_dev      int32 [N][num_agents][3]  (kind, dx, dy)
 *   obs_dev          [N][obs_per_env][C][H][W] of cfg->obs_dtype
 *   rewards_dev      float64 [N][num_agents]   (single surface: [N][1])
 *   done_dev, trunc_dev   uint8 [N]
 *   listed_dev       uint8 [N][num_agents]: agent was in env.agents before the
 *                    step (multi surface: the keys of the returned dicts)
 *   reset_dev        uint8 [N]: 1 when this call reset the env (autoreset)
 * Any output pointer except rewards/done/trunc may be NULL.  With obs_dev NULL no grid observation is written, by
 * the step launch, the reset work or an observation launch, and the step's last launch of its own is the tail
 * (k_tail); everything else the step computes is what it computes with a buffer.  The same holds for every step of
 * zs_step_graph(_n).  A learner on entity observations (zs_entity_obs_bind) steps this way.
 * zs_step does not report a reset that fails for want of player spawn cells (the implicit first reset, an
 * autoreset): it returns ZS_OK, reports the env as reset, and leaves it as the failing
 * Game.__initialize_world__ left it (the players that fit placed, no zombies, the stream after the draws made).
 * ZS_ENOSPACE then stays in the handle's error word, which zs_step never reads; zs_reset, zs_set_state and the
 * zs_host_* calls clear the word before they use it, so none of them reports that stale error.  A caller that
 * must see the failure calls zs_reset (or zs_host_reset / zs_host_step, whose record carries the error of
 * their own reset work). */
int zs_step(zs_handle* h, const int32_t* actions_dev, void* obs_dev, double* rewards_dev,
            uint8_t* done_dev, uint8_t* trunc_dev, uint8_t* listed_dev, uint8_t* reset_dev,
            void* stream);

/* Bench / parity action stream: actions_dev[e][a] = DISCRETE table entry
 * splitmix64(splitmix64(splitmix64(seed_e) ^ step) ^ a) % n_discrete
 * (libzombsole_amd/actions.py).  n_discrete = 6 or 7. */
int zs_gen_actions(zs_handle* h, uint64_t step, int32_t n_discrete, int32_t* actions_dev,
                   void* stream);

/* The bench loop's step as one replayed hipGraph: zs_gen_actions for step number t, then
 * zs_step (same outputs), where t = step0 on the first call after a (re)capture and advances by
 * one per call on the device.  The launches are captured once per pending-reset-list parity for
 * each set of buffer arguments (the last 4 sets are kept, so double-buffered outputs replay
 * without recapture); results equal zs_gen_actions + zs_step.
 * The step counter is one per handle, shared by all its cached sets: a call that captures a set with a policy
 * (a new key, an evicted one, any key after a zs_*_bind change) writes step0 into it; a call that finds its
 * set cached ignores step0 and plays the counter's step, which every policy step of a graph advances by one.
 * zs_step, and graphs with n_discrete = 0 (captured or replayed), neither read nor move the counter: after k
 * such steps a cached policy graph continues k steps behind the episode's step number.  A caller that mixes
 * them and needs the true step number plays those steps through a policy graph too, or forces a recapture.
 * n_discrete = 0: no policy.  The graph replays zs_step on the caller's actions_dev, which the
 * caller fills on `stream` before each call (a learner's actions, derived from the previous step's
 * observations); results equal zs_step.  This is the graphed form of the reference's per-tick
 * MultiagentZombsoleEnv.step(actions) / ZombsoleGymEnv.step(action) (zombsole/gym/multiagent_env.py:111-171,
 * zombsole/gym_env.py:99-145), one graph launch per step. */
int zs_step_graph(zs_handle* h, uint64_t step0, int32_t n_discrete, int32_t* actions_dev, void* obs_dev,
                  double* rewards_dev, uint8_t* done_dev, uint8_t* trunc_dev, uint8_t* listed_dev,
                  uint8_t* reset_dev, void* stream);
/* n_steps consecutive steps of zs_step_graph in one graph launch (1 <= n_steps <= 64): each step is
 * the same policy launch + zs_step on the same outputs, so the outputs hold the last step's results
 * (a caller that reads every step's outputs takes n_steps = 1).  Saves the per-graph launch gap.
 * With n_discrete = 0 every step of the launch reads the same actions_dev. */
int zs_step_graph_n(zs_handle* h, uint64_t step0, int32_t n_discrete, int32_t n_steps, int32_t* actions_dev,
                    void* obs_dev, double* rewards_dev, uint8_t* done_dev, uint8_t* trunc_dev,
                    uint8_t* listed_dev, uint8_t* reset_dev, void* stream);

/* Host view of one env's state as a flat int32 record (layout below). */
int zs_state_size(const zs_handle* h, int32_t* n_words);
int zs_get_state(zs_handle* h, int32_t env, int32_t* buf_host, void* stream);
int zs_set_state(zs_handle* h, int32_t env, const int32_t* buf_host, void* stream);

/* One env's MT19937 stream in CPython random.getstate() form (625 words: the raw
 * 624-word block being consumed, then the index 0..624 of its next word).  The
 * single-env wrappers move the process-global `random` state through these around
 * every call, so the engine consumes the same global stream the reference draws
 * from (zombsole/core.py:1-2 `import random`; random.py:128-168 getstate/setstate). */
int zs_get_rng(zs_handle* h, int32_t env, uint32_t* state_host, void* stream);
int zs_set_rng(zs_handle* h, int32_t env, const uint32_t* state_host, void* stream);

/* Sticky ZS_OVF_* flags of the handle (everything queued on `stream` included), OR-ed over all
 * envs since zs_create or the last call with clear != 0.  Lossless results need
 * !(flags & ZS_OVF_INT32), and !(flags & ZS_OVF_INT16) for ZS_DTYPE_I16 observations. */
int zs_overflow(zs_handle* h, uint32_t* flags_host, int32_t clear, void* stream);

/* ---- observation-state records ------------------------------------------------------------------
 * An env's observation is a function of nine of its arrays alone: things' positions, lives, weapons and
 * presence, the dead-body bitmap, obstacle presence and life, and the two words that say which chunks of
 * the bitmap and of the lives may differ from a fresh env's.  A record is those arrays of one env in one
 * block of rec_bytes bytes (a multiple of 16), a small fraction of the observations they encode, so a
 * centralised learner can exchange records instead of observations (vector.StepGather(mode="state")):
 * every handle packs its envs, a viewer handle (ZS_FLAG_VIEWER) unpacks all of them and zs_observe on it
 * re-encodes them, bit-identical to the observations the source handles wrote.
 *
 * zs_obs_state_layout: out[0] = rec_bytes; out[1..9] = byte offsets of the sections hp_dirty (u32),
 * dead_dirty (u32), pos (i32 [E], x | y << 16), life (i32 [E]), dead (u32 [ceil(W*H/32)]), obst_present
 * (u32 [ceil(O/32)]), obst_hp ([O]), weapon (u8 [E]), present (u8 [E]); out[10] = offset of the zero
 * padding that ends the record; out[11] = bytes of an obst_hp element: 4 (int32), or 2 for ZS_DTYPE_I16
 * handles with the channels encoding (int16, the life saturated at -32768 as those observations saturate
 * it themselves).
 * zs_obs_state_pack: the records of all N envs into rec_dev, [N][rec_bytes], 16-byte aligned; every byte
 * of every record is written (padding: zeros).  Any handle.
 * zs_obs_state_unpack: records [0, n) of rec_dev into envs [env0, env0 + n) of a viewer handle (any other
 * handle: ZS_ESTATE); its other envs are untouched.  rec_bytes must equal the handle's own and the range
 * lie inside [0, N), else ZS_EINVAL with nothing launched.  The packing and the unpacking handle must share
 * the map and the entity counts (agents, bots, zombie slots), the observation dtype and encoding: nothing in
 * a record says which handle wrote it, and its contents are not validated.  The source's ZS_OVF_* flags do
 * not travel: read zs_overflow on the source handles. */
int zs_obs_state_layout(const zs_handle* h, int32_t out[12]);
int zs_obs_state_pack(zs_handle* h, void* rec_dev, void* stream);
int zs_obs_state_unpack(zs_handle* h, const void* rec_dev, int32_t rec_bytes, int32_t env0, int32_t n, void* stream);

/* ---- snapshot records: batched device snapshot, restore and clone of env state ---------------------
 * A snapshot record is a verbatim copy of everything per-env that a later step, reset, respawn or
 * observation reads, in one block of rec_bytes bytes (a multiple of 16); nothing is narrowed or re-derived.
 * Restoring it and replaying the same actions reproduces the run bit for bit.  Sections, in record order
 * (E entity slots, A agents, O obstacles, DW = ceil(W*H/32), OW = ceil(O/32)):
 *   ring u32 [1248] (two MT19937 blocks), dead u32 [DW], obst_hp i32 [O] (int32 whatever the observation
 *   dtype), obst_present u32 [OW], obst_nonpos u32 [OW], pos i32 [E] (x | y << 16), life i32 [E], serial u32 [E],
 *   scal i32 [9] (t, deaths, zombie_deaths, episode_steps, n_order, needs_reset, reward prev zombie_deaths,
 *   spawn serial counter, obstacle-cleanup flag), hp_dirty u32, dead_dirty u32, rngst u32 (MT19937 ring offset
 *   | slot << 10 | next-block-ready << 11), prev_life i32 [A], weapon u8 [E], present u8 [E], order u8 [E],
 *   listed u8 [A], zero padding.  A ZS_FLAG_ENV_PARAMS handle's record holds one section more, env_params
 *   i32 [6] (the current triple, then the next one), after prev_life and before the byte rows.  A
 *   ZS_FLAG_EPISODE_STATS handle's record holds the section ep_run: run_ret f64 [R], run_flags i32, 4 zero bytes;
 *   8-byte aligned (after 4 zero bytes where needed), behind env_params (if any) and before the byte rows.
 * NOT in a record: the action-stream seed (zs_seed sets it; it belongs to the slot's policy), the death and
 * action logs (a step's outputs: zs_restore empties them for the envs it writes), the handle's sticky
 * ZS_OVF_* word, zs_step_graph's policy step counter, and a ZS_FLAG_EPISODE_STATS handle's last finished episode
 * and totals (last, last_ret, tot, sum_ret: the slot's own, like the action-stream seed; zs_restore leaves them alone).
 *
 * zs_snapshot_layout: out[0] = rec_bytes; out[1..17] = the byte offsets of the 17 sections in the order
 * above; out[18] = offset of the zero padding; out[19], out[20] = low and high word of the handle's 64-bit
 * fingerprint; out[21] = scalar rows (9); out[22] = ring words (1248); out[23] = the byte offset of the
 * env_params section of a ZS_FLAG_ENV_PARAMS handle's record, else 0.  Two handles whose
 * fingerprints agree can exchange records.  The fingerprint covers the map size, the entity counts (agents,
 * bots, zombie slots), rules, reward mode, max_episode_steps, initial and minimum zombies and the static
 * tables (obstacle cells and kinds, spawn lists, objective cells, agent weapons, bot types); not the env
 * count, the observation settings, lanes_per_env, the launch overrides or the flags, except ZS_FLAG_ENV_PARAMS
 * and ZS_FLAG_EPISODE_STATS (their records are longer), which it covers.  The ep_run section's offset is
 * zs_episode_stats_layout's out[3]; zs_snapshot_layout's out[24] is unchanged.
 *
 * zs_snapshot: record k of rec_dev ([n][rec_bytes], 16-byte aligned) = env env_idx_dev[k] (NULL: env k);
 * duplicates allowed.  Every byte of a record is written (padding: zeros), nothing outside the n records.
 * Any handle, viewers included.
 * zs_restore: record src_idx_dev[k] (NULL: k) of the n_records records at rec_dev is written into env
 * dst_idx_dev[k] (NULL: k), k < n.  n_records is the caller's declaration of how many records rec_dev
 * holds: the kernel reads no record at or past it.  Destinations must be distinct (the caller's contract);
 * sources may repeat (fan-out).  Envs that are no destination keep every byte.  After the copy the pending-
 * reset list the next zs_step drains is rebuilt from the needs_reset flags of all N envs: an env restored
 * from a pending record is reset by the next step, exactly once, and reported in reset_dev; a pending env
 * overwritten by a running record is not reset.  The list parity does not change, so zs_step_graph's cached
 * graphs stay valid.  ZS_ESTATE on a viewer handle.
 * Both: asynchronous on `stream` (no host synchronisation, no host staging).  n < 0, n_records < 0, an
 * unaligned rec_dev or a rec_bytes that is not the handle's: ZS_EINVAL before any launch.  Index entries
 * are bounds-checked on the device: an entry whose env is outside [0, N), or whose record is outside
 * [0, n_records), is skipped (nothing read or written for it).  Record contents are not validated.
 * zs_set_state's needs_reset refusal is unchanged. */
int zs_snapshot_layout(const zs_handle* h, int32_t out[24]);
int zs_snapshot(zs_handle* h, const int32_t* env_idx_dev, int32_t n, void* rec_dev, void* stream);
int zs_restore(zs_handle* h, const void* rec_dev, int32_t rec_bytes, int32_t n_records, const int32_t* src_idx_dev,
               const int32_t* dst_idx_dev, int32_t n, void* stream);

/* ---- action masks of the discrete action tables ----------------------------------------------------
 * mask_dev is uint8 [N][num_agents][8], 8-byte aligned (else ZS_EINVAL).  Byte k of agent a is 1 exactly when,
 * on the env's current world (the one its observation shows), the reference would carry out game_actions[k]
 * of the Discrete(6) / Discrete(7) tables (gym_env.py:328-351, gym/multiagent_env.py:259-285) for that agent,
 * were its action the first one executed: Agent.next_step returns an action (players/agent.py:28-96) and
 * World.thing_move / thing_attack / thing_heal log 'moved to', 'injured' or 'healed' (core.py:140-202).
 *   0..3  move (0,1), (-1,0), (0,-1), (1,0): the destination is inside the map and World.things holds nothing
 *         there: a present obstacle blocks whatever its life (one re-spawned destroyed stays until the
 *         episode's first cleanup), so does a present zombie, bot or agent; bodies and objectives do not
 *   4     attack_closest: a zombie is present and the closest one is within the agent's own weapon range
 *   5     heal: 1
 *   6     heal_closest (multi surface; 0 on the single one, whose table has 6 entries): no other bot or agent
 *         is present, or the closest one is within HEALING_RANGE
 *   7     0
 * An agent that is not in the world (dead, or never placed) has eight zero bytes.  An env pending its reset
 * shows the terminal world's masks, as its observation does.
 *
 * zs_action_mask: one launch on `stream` for the envs whose env_mask_dev byte is nonzero (NULL = all); other
 * envs' bytes are untouched.  Any handle: a viewer's envs (zs_obs_state_unpack) hold everything the kernel
 * reads, so it works there at no extra cost.
 * zs_action_mask_bind: while a buffer is bound (non-NULL), every zs_step ends with a mask launch of all envs
 * into it, after the observation / tail launch, so the masks show respawned zombies and a reset env's new
 * world; zs_step_graph(_n) captures that launch with the step.  Binding another buffer or NULL drops the
 * cached graphs (the next zs_step_graph recaptures).  A handle that never binds launches what it did before.
 * The buffer must outlive the binding.  ZS_ESTATE on a viewer handle (nothing steps it). */
int zs_action_mask(zs_handle* h, const uint8_t* env_mask_dev, void* mask_dev, void* stream);
int zs_action_mask_bind(zs_handle* h, void* mask_dev_or_null);

/* ---- entity observations: a few hundred bytes per env instead of the grid ---------------------------------
 * out_dev is int16 [N][num_agents][ROW], ROW = 16 + 4 (kz + kp) words, 8-byte aligned (else ZS_EINVAL), with
 * 1 <= kz <= 16 zombie rows and 0 <= kp <= 16 player rows (else ZS_EINVAL, before any launch).  Every value is an
 * exact integer of the env's current world, the one its grid observation shows (an env pending its reset: the
 * terminal world).  A row, in words (E slots: agents [0,A), bots [A,A+P), zombies [A+P,E)):
 *   self       8  present (1), x, y, life, weapon code (ZS_WEAPON_*), weapon_r2 (the largest integer d2 inside the
 *                 weapon's range: 2, 36, 100, 9), zombies present in the env, other agents and bots present
 *   zombies    kz x {dx, dy, life, flags}: the present zombie slots ascending by (d2, slot), d2 = dx^2 + dy^2 and
 *                 dx, dy the zombie's cell minus the agent's; flags bit 0 valid, bit 1 d2 <= weapon_r2, bit 2
 *                 d2 == 1; rows past the present zombies are zero
 *   players    kp x {dx, dy, life, flags}: the present agent and bot slots other than the agent itself, in the
 *                 same order; flags bit 0 valid, bit 1 d2 <= 9 (HEALING_RANGE), bit 2 an agent and not a bot,
 *                 bits 8..15 its weapon code
 *   objective  4  {dx, dy, flags, n_objectives} of the nearest objective cell by (d2, map-file index); flags bit 0
 *                 valid, bit 1 the agent stands on an objective
 *   rays       4  towards (0,1), (-1,0), (0,-1), (1,0): the consecutive cells, starting next to the agent, that
 *                 are inside the map and hold no present obstacle (whatever its life), at most 16; entities do not
 *                 stop a ray
 * Lives and counts saturate to the int16 range.  An agent that is not in the world has an all-zero row.
 * The tie-break among equidistant slots is the slot number, not the reference's dict order: among equidistant
 * zombies row 0 need not be the one attack_closest hits (bit 1 of row 0 still equals action-mask byte 4).
 *
 * zs_entity_obs_layout: out[0] = ROW in words, out[1..5] = the word offsets of self, zombies, players, objective and
 * rays, out[6] = the ray cap (16), out[7] = the row's bytes.
 * zs_entity_obs: one launch on `stream` for the envs whose env_mask_dev byte is nonzero (NULL = all); other envs'
 * bytes are untouched.  Any handle: a viewer's envs (zs_obs_state_unpack) hold everything the kernel reads.
 * zs_entity_obs_bind: while a buffer is bound (non-NULL), every zs_step ends with a launch of all envs into it, after
 * the observation / tail launch and a bound mask launch, eagerly, for each step of zs_step_graph(_n) and through
 * zs_host_step.  Binding another buffer, other K values or NULL drops the cached graphs.  A handle that never binds
 * launches what it did before.  The buffer must outlive the binding.  ZS_ESTATE on a viewer handle. */
int zs_entity_obs_layout(const zs_handle* h, int32_t kz, int32_t kp, int32_t out[8]);
int zs_entity_obs(zs_handle* h, const uint8_t* env_mask_dev, int32_t kz, int32_t kp, void* out_dev, void* stream);
int zs_entity_obs_bind(zs_handle* h, void* out_dev_or_null, int32_t kz, int32_t kp);

/* ---- entity-targeted actions: a pointer action table over the entity observation's rows ---------------------
 * NID = 15 + kz + kp ids per agent, kz and kp those of the entity observation (1 <= kz <= 16, 0 <= kp <= 16, else
 * ZS_EINVAL before any launch).  Everything is evaluated on the env's current world, the one its observation shows (an
 * env pending its reset: the terminal world).  dir k = (0,1), (-1,0), (0,-1), (1,0).
 *   id                   triple                                  mask bit is 1 exactly when
 *   0..3                 (ZS_ACT_MOVE, dir k)                    as zs_action_mask byte k
 *   4                    (ZS_ACT_ATTACK_CLOSEST, 0, 0)           as zs_action_mask byte 4
 *   5                    (ZS_ACT_HEAL, 0, 0)                     1
 *   6                    (ZS_ACT_HEAL_CLOSEST, 0, 0)             zs_action_mask byte 6 by the multi surface's rule, on both
 *                                                                surfaces (Agent.next_step takes heal_closest on either)
 *   7..10                (ZS_ACT_ATTACK, dir k)                  the adjacent cell is inside the map and World.things holds a
 *                                                                thing there: a present obstacle whatever its life, or a
 *                                                                present zombie, bot or agent (every weapon reaches distance 1)
 *   11..14               (ZS_ACT_HEAL, dir k)                    the adjacent cell holds a present agent or bot or a present
 *                                                                obstacle, not a zombie (players/agent.py:69-75)
 *   15 + j, j < kz       (ZS_ACT_ATTACK, dx_j, dy_j)             zombie row j of the entity observation is valid and its
 *                                                                d2 <= weapon_r2 (the row's bit 1)
 *   15 + kz + j, j < kp  (ZS_ACT_HEAL, dx_j, dy_j)               player row j is valid and its d2 <= 9 (the row's bit 1)
 * Row j is the j-th present zombie, or the j-th other present agent or bot, ascending by (d2, slot): the entity
 * observation's order.  A mask bit means what zs_action_mask's bytes mean: were this the agent's action and the first
 * one executed, Agent.next_step would return an action and World.thing_move / thing_attack / thing_heal would log 'moved
 * to', 'injured' or 'healed'.  Friendly fire is an action the reference carries out, so its bit is 1.
 * Decode: a valid row decodes to its triple whether or not the mask allows it (the tick then reports 'too far', as the
 * reference does); an id whose row is not valid decodes to (ZS_ACT_IDLE, 0, 0); an id outside [0, NID) does too and
 * raises the sticky ZS_OVF_PARAM_RANGE bit of zs_overflow's word; an agent that is not in the world gets (ZS_ACT_IDLE,
 * 0, 0) and an all-zero mask row.
 * Encode: the smallest id of [0, NID) whose decoded triple equals the given triple word for word on the current world,
 * else -1.  Every triple zs_autopilot writes has an id.
 *
 * zs_entity_act_table: out[0] = NID, out[1] = the mask row's bytes (NID rounded up to 8; padding bytes are 0), out[2..6]
 * = the first id of the blocks attack-dir (7), heal-dir (11), zombie rows (15), player rows (15 + kz), end (NID),
 * out[7] = 0.
 * zs_entity_act_decode: ids_dev int32 [N][num_agents] into actions_dev int32 [N][num_agents][3].
 * zs_entity_act_mask: mask_dev uint8 [N][num_agents][row bytes], 8-byte aligned (else ZS_EINVAL).
 * zs_entity_act_encode: triples_dev int32 [N][num_agents][3] into ids_out_dev int32 [N][num_agents].
 * All three: one launch on `hip_stream` (a hipStream_t passed as void*, what the other calls name `stream`), no host
 * synchronisation; envs whose env_mask_dev byte is 0 are untouched (NULL = all).  Any handle: a viewer's envs
 * (zs_obs_state_unpack) hold everything the kernels read, which is what zs_action_mask and zs_entity_obs read.
 * zs_entity_act_bind: while mask_dev is bound (non-NULL), every zs_step launches the masks of all envs into it after a
 * bound entity-observation launch and before a bound path-distance launch.  While ids_dev is bound, every zs_step begins
 * with the decode of all envs from ids_dev into that call's actions_dev, on the caller's stream ahead of the reset
 * work's fork.  Both hold eagerly, for each step of zs_step_graph(_n) (n_steps > 1: each step decodes the same ids
 * against its own world) and through zs_host_step.  While ids_dev is bound, zs_step_graph(_n) with n_discrete != 0 is
 * ZS_EINVAL: the generated policy would overwrite the decoded rows.  Binding other buffers, other K values or NULL drops
 * the cached graphs; unlike the other *_bind calls this one does not wait for the device: it marks the sets, and the
 * next zs_step_graph(_n) waits for its stream and destroys them before it captures anew.  A handle that never binds
 * launches what it did before.  The buffers must outlive the binding.  ZS_ESTATE on a viewer handle. */
int zs_entity_act_table(const zs_handle* h, int32_t kz, int32_t kp, int32_t out[8]);
int zs_entity_act_decode(zs_handle* h, const uint8_t* env_mask_dev, int32_t kz, int32_t kp, const int32_t* ids_dev,
                         int32_t* actions_dev, void* hip_stream);
int zs_entity_act_mask(zs_handle* h, const uint8_t* env_mask_dev, int32_t kz, int32_t kp, void* mask_dev, void* hip_stream);
int zs_entity_act_encode(zs_handle* h, const uint8_t* env_mask_dev, int32_t kz, int32_t kp, const int32_t* triples_dev,
                         int32_t* ids_out_dev, void* hip_stream);
int zs_entity_act_bind(zs_handle* h, const int32_t* ids_dev_or_null, void* mask_dev_or_null, int32_t kz, int32_t kp);

/* ---- path-distance fields: walking distance to the objectives and to the zombies, per env -------------------
 * A cell is free when it is inside the map and holds no present obstacle, whatever the obstacle's life (the rule of
 * the entity observation's rays); entities never block.  A field is the 4-connected breadth-first distance over free
 * cells from a set of source cells, in moves; a source cell that is not free is not a source.  ZS_NAV_OBJECTIVE: the
 * sources are the map's objective cells (there may be none); ZS_NAV_ZOMBIES: the cells of the present zombie slots.
 * `fields` is a bitmask of the two, F its popcount, the fields emitted in ascending bit order.  1 <= max_dist <=
 * ZS_NAV_MAX_DIST: the search stops after that many levels and a cell not reached by then is unreachable, as blocked
 * cells and cells outside the map are.  Every value is of the env's current world, the one its observation shows (an
 * env pending its reset: the terminal world).
 *
 * Rows: out_dev is int16 [N][num_agents][F][8], 8-byte aligned.  Word 0 the distance at the agent's cell; words 1..4
 * the distances at the cells the moves (0,1), (-1,0), (0,-1), (1,0) lead to, -1 where unreachable, blocked or outside
 * the map; word 5 the smallest k whose neighbour distance is the minimum over the reachable neighbours, word 6 the
 * smallest k at their maximum, both -1 when no neighbour is reachable; word 7 flags: bit 0 the agent is present, bit 1
 * its own cell is a source.  An agent that is not in the world has an all-zero row.
 * Full field: out_dev is uint16 [n][H][W], 2-byte aligned, 0xFFFF = unreachable or blocked.
 *
 * The search runs in the workgroup's LDS (csrc/zs_nav.hpp nav_plan): a map whose single-env image is larger than
 * 64 KiB (28 * H * ceil(W / 32) + 8 * 5 * num_agents bytes, rounded up to 16) is refused with ZS_EINVAL by zs_nav_obs,
 * zs_nav_field and zs_nav_bind; zs_create refuses no handle for it.
 *
 * zs_nav_plan: out[0] = F, out[1] = the row's words (8), out[2] = the word offset of field 0's row in an agent's block
 * (0), out[3] = that of field 1's (8 when F = 2, else -1), out[4] = envs per workgroup, out[5] = threads per workgroup,
 * out[6] = the workgroup's LDS bytes, out[7] = one env's image bytes; out[4..6] are 0 where the map is past the limit
 * (the call itself succeeds).
 * zs_nav_obs: one launch on `stream` for the envs whose env_mask_dev byte is nonzero (NULL = all); other envs' rows are
 * untouched.  Any handle: a viewer's envs (zs_obs_state_unpack) hold everything the kernel reads.
 * zs_nav_field: frame k < n of env env_idx_dev[k] (NULL: k) and the one field `field`; an entry outside [0, N) leaves
 * its frame untouched; entries may repeat.  Any handle.
 * zs_nav_bind: while a buffer is bound (non-NULL), every zs_step ends with a launch of all envs into it, after the
 * observation / tail launch and the bound mask and entity launches and before a bound autopilot's, eagerly, for each
 * step of zs_step_graph(_n) and through zs_host_step.  Binding another buffer, other fields, another max_dist or NULL
 * drops the cached graphs.  A handle that never binds launches what it did before.  The buffer must outlive the
 * binding.  ZS_ESTATE on a viewer handle.
 * ZS_EINVAL before any launch: fields zero or with unknown bits, field not exactly one of the two bits, max_dist out of
 * range, a misaligned buffer, n < 0. */
#define ZS_NAV_OBJECTIVE 1
#define ZS_NAV_ZOMBIES 2
#define ZS_NAV_MAX_DIST 32766
int zs_nav_plan(const zs_handle* h, int32_t fields, int32_t out[8]);
int zs_nav_obs(zs_handle* h, const uint8_t* env_mask_dev, int32_t fields, int32_t max_dist, void* out_dev, void* stream);
int zs_nav_field(zs_handle* h, const int32_t* env_idx_dev, int32_t n, int32_t field, int32_t max_dist, void* out_dev,
                 void* stream);
int zs_nav_bind(zs_handle* h, void* out_dev_or_null, int32_t fields, int32_t max_dist);

/* ---- scripted policies for agent slots: a launch that writes the bots' actions as agent triples -------------
 * out_dev is int32 [N][num_agents][3], triples in zs_step's action form (ZS_ACT_*, dx, dy), 4-byte aligned (else
 * ZS_EINVAL); policy_dev is uint8 [N][num_agents], one ZS_PILOT_* code per agent.  Each row is computed from the env's
 * current world, the one its observation shows (an env pending its reset: the terminal world):
 *   ZS_PILOT_NONE        the row is not written: a caller's own triple in it survives
 *   ZS_PILOT_TERMINATOR  players/terminator.py with the agent's own weapon.  z = the closest present zombie, ties
 *                        broken by the reference's dict order.  No zombie: (ZS_ACT_HEAL, 0, 0).  z within the weapon's
 *                        range: (ZS_ACT_ATTACK_CLOSEST, 0, 0).  Else (dx, dy) = the adjacent cell closest to z, the
 *                        first minimum over (0,1), (0,-1), (1,0), (-1,0): (ZS_ACT_HEAL, dx, dy) when an agent or bot
 *                        stands there, (ZS_ACT_ATTACK, dx, dy) when any other thing does (a zombie; an obstacle
 *                        whatever its life), else (ZS_ACT_MOVE, dx, dy), a cell outside the map included
 *   ZS_PILOT_SNIPER      players/sniper.py: (ZS_ACT_ATTACK_CLOSEST, 0, 0)
 *   ZS_PILOT_TROLL       players/troll.py: (ZS_ACT_HEAL, 0, 0)
 *   any other code       (ZS_ACT_IDLE, 0, 0), and the sticky ZS_OVF_PARAM_RANGE bit of zs_overflow's word is raised
 * An agent of nonzero code that is not in the world gets (ZS_ACT_IDLE, 0, 0).  Given such a triple, zs_step does for
 * the agent exactly what the reference's bot of that class does in its place.  No policy draws from the env's stream.
 *
 * zs_autopilot: one launch on `stream` for the envs whose env_mask_dev byte is nonzero (NULL = all); other envs' rows
 * are untouched.
 * zs_autopilot_bind: while a policy and an output are bound (both non-NULL; both NULL unbinds), every zs_step ends with
 * a launch of all envs, after the observation / tail launch and the bound mask and entity launches and before the
 * episode statistics, eagerly and for each step of zs_step_graph(_n).  The policy tensor's contents may change between
 * steps and graph replays.  out_dev may be the action buffer the steps read: step t's last launch then writes the rows
 * step t + 1 takes (the closed loop; with zs_step_graph(_n) pass n_discrete = 0, else the generated policy overwrites
 * them).  Binding other buffers or NULL drops the cached graphs.  The buffers must outlive the binding.
 * Both calls: ZS_EINVAL on a NULL argument, ZS_ESTATE on a viewer handle (its observation-state records carry no dict
 * order, which the closest zombie's tie-break reads). */
#define ZS_PILOT_NONE 0
#define ZS_PILOT_TERMINATOR 1
#define ZS_PILOT_SNIPER 2
#define ZS_PILOT_TROLL 3
int zs_autopilot(zs_handle* h, const uint8_t* env_mask_dev, const uint8_t* policy_dev, int32_t* out_dev, void* stream);
int zs_autopilot_bind(zs_handle* h, const uint8_t* policy_dev_or_null, int32_t* out_dev_or_null);

/* ---- per-env zombie counts and time limits (ZS_FLAG_ENV_PARAMS) ----------------------------------------
 * A flagged handle holds, per env, the triple (initial_zombies, minimum_zombies, max_episode_steps) twice: the
 * NEXT triple and the CURRENT one.  After zs_create both equal the config's values, and until the first
 * zs_env_params_set the handle behaves exactly like one without the flag.  Every reset of env e (the implicit
 * first one, zs_reset, an autoreset, alone or fused into the step launch) copies next -> current and then spawns
 * initial_e zombies; until the env's next reset its zombie respawns (by the tick or by k_respawn) keep minimum_e
 * zombies and its TimeLimit truncates at max_steps_e (0: none), read from the current triple.  So an episode has
 * one difficulty from its first tick to its last.  The config's values are caps: 0 <= initial_e <=
 * cfg.initial_zombies, 0 <= minimum_e <= cfg.minimum_zombies, max_steps_e >= 0; the entity slots, the step plan
 * and the LDS images stay functions of the config alone.  New zombies go into the lowest free zombie slots, so an
 * env with smaller counts is, slot for slot, the env of a handle configured with those counts.
 *
 * zs_env_params_set: two launches of one kernel (k_env_params) on `stream`, the first finding, in a scratch row
 * of the handle, the entry that wins each env, the second storing the winners; entry k, k < n, writes the triple params_dev[k][0..2]
 * into the next triple of env env_idx_dev[k] (NULL: env k).  Indices and values are device memory: nothing is
 * read back, the host is not synchronised.  An entry whose env is outside [0, N) or whose values are outside
 * the ranges above is not applied and raises the sticky ZS_OVF_PARAM_RANGE bit of zs_overflow's word; the other
 * entries are applied.  When one env appears in several entries with different triples, one of the given
 * triples wins whole (its three values are never mixed with another entry's); which one is not specified.
 * n < 0 or n > 2^30: ZS_EINVAL; n == 0: nothing.  Like every call on a handle, set calls are serialised on the
 * stream they are given: two of them in flight on different streams of one handle share the scratch row and may
 * drop or mix entries.
 * zs_env_params_check: *refused_host = 1 when ZS_OVF_PARAM_RANGE is up (everything queued on `stream` included),
 * else 0, and clears that bit alone (the other ZS_OVF_* bits stay); synchronises the stream.
 * zs_env_params_get: the next (which = 0) or current (which = 1) triples of all N envs into out_dev, int32
 * [N][3], one launch on `stream`.  Any other `which`: ZS_EINVAL.
 * All three: ZS_ESTATE on a handle created without ZS_FLAG_ENV_PARAMS.
 * Snapshot records of a flagged handle carry both triples (zs_snapshot_layout's out[23]), and its fingerprint
 * covers the flag: flagged and unflagged handles do not exchange records. */
int zs_env_params_set(zs_handle* h, const int32_t* env_idx_dev, int32_t n, const int32_t* params_dev, void* stream);
int zs_env_params_get(zs_handle* h, int32_t which, int32_t* out_dev, void* stream);
int zs_env_params_check(zs_handle* h, uint32_t* refused_host, void* stream);

/* ---- per-env episode statistics (ZS_FLAG_EPISODE_STATS) --------------------------------------------------
 * A flagged handle keeps, per env (R = 1 with ZS_REWARD_SINGLE, num_agents with ZS_REWARD_MULTI):
 *   running:        run_ret f64 [R], run_flags i32 (bit 0: closed)
 *   last episode:   last_ret f64 [R], last i32 [8] = {length, outcome, zombie_deaths, deaths, initial_zombies,
 *                   minimum_zombies, max_episode_steps, serial}; serial is tot[0] after this episode was counted
 *   totals since zs_create or the last clear: tot u32 [8] = {episodes, won, lost, truncated_agents_dead,
 *                   truncated_timelimit, sum of length, sum of zombie_deaths, sum of deaths} (sums mod 2^32),
 *                   sum_ret f64 [R]
 * Outcome codes (last[1]): 1 won (done and won), 2 lost (done and not won), 3 not done, truncated, no agent alive,
 * 4 not done, truncated, some agent alive (the TimeLimit); 256 is OR-ed in when done and truncated are both set.
 * `won` is the rules' own: 2 * alive players >= players for evacuation, else a player alive.
 * Every zs_step (eager, inside zs_step_graph(_n) for each of its steps, and through zs_host_step) ends with one
 * launch, after a bound mask launch, that applies per env, in this order: the step was the env's reset: run_ret = 0,
 * closed = 0; else, if not closed, run_ret[r] = run_ret[r] + rewards[e][r] (one float64 add per step, in step
 * order); if additionally done | truncated: last_ret = run_ret, last filled (length, zombie_deaths and deaths from the
 * env's terminal world, the triple the episode ran under), tot bumped, sum_ret[r] += run_ret[r], closed = 1.  A closed
 * env is not accumulated and not counted again until its next reset (without ZS_FLAG_AUTORESET an ended env keeps
 * ticking and reporting done).  zs_reset, masked or not, zeroes run_ret and closed of the envs it resets: an
 * abandoned episode is not counted.  A flagged handle's zs_step accepts reset_dev = NULL like any other.
 *
 * zs_episode_stats_layout: out[0] = R, out[1] = words of last (8), out[2] = words of tot (8), out[3] = byte offset
 * of the ep_run section of the handle's snapshot record, out[4] = its bytes (8 R + 8), out[5..7] = 0.
 * zs_episode_stats_get: one launch on `stream`; env-major outputs run_ret, last_ret, sum_ret f64 [N][R], last i32
 * [N][8], tot u32 [N][8].  Any output pointer may be NULL.  The rows of envs whose env_mask_dev byte is 0 are untouched
 * (NULL: all envs).  Nothing is read back and the host is not synchronised.
 * zs_episode_stats_clear: zeroes last, last_ret, tot and sum_ret of the masked envs (NULL: all); the running part
 * stays.  One launch on `stream`.
 * All three: ZS_ESTATE on a handle created without ZS_FLAG_EPISODE_STATS. */
int zs_episode_stats_layout(const zs_handle* h, int32_t out[8]);
int zs_episode_stats_get(zs_handle* h, const uint8_t* env_mask_dev, double* run_ret_dev, double* last_ret_dev,
                         double* sum_ret_dev, int32_t* last_dev, uint32_t* tot_dev, void* stream);
int zs_episode_stats_clear(zs_handle* h, const uint8_t* env_mask_dev, void* stream);

/* ---- frames of the envs, drawn on the device (ZS_FLAG_RENDER) ---------------------------------------------
 * A frame is uint8 [10 H][10 W][3], RGB: the map area (the crop [:10 H, :10 W]) of the image the reference's
 * OpencvRenderer(W, H + 2 + players).render draws (renderer.py:235-277), pixel for pixel.  The lines below the map
 * (ticks, life bars, player text) are not drawn.  Cell size 10 and mask size 11 are the reference's.
 * Per cell, in this order: a present entity draws the disc in its slot's colour (agents blue, zombies green, bots by
 * type: terminator cyan, sniper yellow, hamster white, randoman red, troll blue); else a present obstacle the wall
 * (white) or box (yellow), whatever its life; else a body (the env's dead bit) the body mask in the cell's recorded
 * colour; else an objective the frame (blue).  Every drawn cell paints its 11 x 11 mask at (10 x, 10 y); where the
 * masks of neighbours share a pixel row or column the cell painted later (x outer, y inner) wins, so pixel (px, py)
 * takes the first of cell (px / 10, py / 10), the cell above it when py % 10 == 0, the cell left of it when
 * px % 10 == 0 and the cell above-left when both, whose mask covers it, else black.
 * A flagged handle keeps body_col, one byte per cell per env (a palette index; rows of W H bytes rounded up to 16):
 * every zs_step (eager, inside zs_step_graph(_n) for each of its steps, through zs_host_step) ends with one launch
 * that clears the row of an env the step reset and, for every other env, writes for each entry of the step's death
 * log the colour of its slot at its cell, in removal order (the last body of a cell gives the colour, as
 * World.decoration keeps the last).  zs_reset clears the rows of the envs it resets.  zs_set_state leaves the row
 * alone: a body poked onto a cell without a death this episode has colour 0 and is drawn green.  The flag needs
 * ZS_FLAG_DEATH_LOG (zs_create: ZS_EINVAL without it, and for a map whose frame would reach 2 GiB) and is refused on
 * a viewer handle (ZS_ESTATE).  Snapshot records of a flagged handle carry body_col as their last byte section, and
 * the fingerprint covers the flag.
 *
 * zs_render_layout: out[0] = frame height (10 H), out[1] = frame width (10 W), out[2] = frame bytes, out[3] = cell
 * size (10), out[4] = mask size (11), out[5] = palette entries (8), out[6] = body_col bytes per env, out[7] = byte
 * offset of the body_col section of the handle's snapshot record.
 * zs_render: frame k, k < min(n, n_frames), is env envs_dev[k] (NULL: env k), written at out_dev + k * frame bytes;
 * out_dev is device memory for n_frames frames and needs no alignment.  An entry outside [0, N) is skipped on the
 * device and its frame keeps its bytes; entries at or past n_frames are not drawn.  Envs may repeat.  One launch on
 * `stream`, nothing read back, the host not synchronised.  n < 0 or n_frames < 0: ZS_EINVAL; min(n, n_frames) == 0:
 * nothing.
 * zs_render_sprites: replaces the atlas: masks[5][4] = the 121-bit masks of solid (wall), box, disc, frame
 * (objective), body, bit oy * 11 + ox of a mask in word (bit >> 5); palette[8][3] = RGB of entries 0 green (and "no
 * colour recorded"), 1 blue, 2 cyan, 3 yellow, 4 white, 5 red, 6 and 7 unused.  Waits for the device; later
 * zs_render calls draw with the new atlas.  The default atlas is the reference's shapes and colours.
 * All three: ZS_ESTATE on a handle created without ZS_FLAG_RENDER (a viewer handle cannot have it). */
int zs_render_layout(const zs_handle* h, int32_t out[8]);
int zs_render(zs_handle* h, const int32_t* envs_dev, int32_t n, uint8_t* out_dev, int32_t n_frames, void* stream);
int zs_render_sprites(zs_handle* h, const uint32_t masks[5][4], const uint8_t palette[8][3]);

/* Diagnostics (not part of the reference surface): when enabled, every k_tick
 * (the step kernel), k_obs (the observation kernel) and k_reset (world rebuild)
 * launch is bracketed by HIP events on its stream.  zs_profile_read synchronizes
 * and returns out[0] = total k_tick ms, out[1] = k_tick launches, out[2] = total
 * k_obs ms, out[3] = k_obs launches, out[4] = total k_reset ms, out[5] = k_reset
 * launches, out[6] = total k_respawn ms, out[7] = k_respawn launches (deferred zombie
 * respawns), then clears the record. */
int zs_profile(zs_handle* h, int32_t enable);
int zs_profile_read(zs_handle* h, double out[8]);
/* Diagnostics: the launch configuration the handle chose (lanes per env, LDS images, which
 * observation kernel, fused / side-stream reset work, deferred respawn) as a one-line JSON
 * object, NUL-terminated and truncated to len bytes.  "obs_kernel" names the kernel of a step's
 * and an unmasked zs_reset's observations ("step launch": the step writes them itself),
 * "obs_kernel_masked" that of a zs_reset / zs_observe with an env mask, "obs_encoders"
 * ("patched", "select" or "") the encoders of k_obs_ring; "mask_kernel", "mask_grid", "mask_block" the
 * action-mask launch (zs_action_mask) and "mask_bound" whether a buffer is bound; "env_params" whether the handle
 * carries per-env triples (ZS_FLAG_ENV_PARAMS), "episode_stats" whether it keeps episode statistics
 * (ZS_FLAG_EPISODE_STATS); "render" whether it draws frames (ZS_FLAG_RENDER), "render_grid" k_render's workgroups
 * per frame and "render_block" their threads (0 without the flag); "entity_obs_bound" whether an entity-observation
 * buffer is bound (zs_entity_obs_bind) and "entity_kz", "entity_kp" its K values (0 when none);
 * "autopilot_kernel", "autopilot_grid", "autopilot_block" the scripted-policy launch (zs_autopilot) and
 * "autopilot_bound" whether a policy is bound (zs_autopilot_bind); "nav_kernel", "nav_envs_per_wg", "nav_block",
 * "nav_lds_bytes" the path-distance launch (zs_nav_obs; 0 where the map is past its plan's limit), "nav_bound" whether
 * a buffer is bound (zs_nav_bind) and "nav_fields", "nav_max_dist" its arguments (0 when none);
 * "entity_act_kernel" the entity action table's kernels (zs_entity_act_*), "entity_act_ids_bound" and
 * "entity_act_mask_bound" whether ids and a mask buffer are bound (zs_entity_act_bind);
 * "step_tail_launch" the launch that carried the tail of the last zs_step queued or captured: the observation kernel,
 * or "k_tail" when the step launch wrote the observations itself or obs_dev was NULL ("" before any step);
 * "step_policy" where the last captured zs_step_graph step with a policy takes its actions from: "ahead" (the
 * previous step's observation kernel left them, the tick copies them out: no policy launch), "k_gen_actions_ctr"
 * (a launch of its own) or "step launch" (generated inside it); "" before any such capture.
 * Returns ZS_OK. */
int zs_describe(zs_handle* h, char* buf, int32_t len);
/* Diagnostics: out[0], out[1] = the two pending-reset list counts, out[2] = the deferred-respawn
 * count (after everything queued on stream), out[3] = the list parity the next step drains. */
int zs_debug_lists(zs_handle* h, int32_t out[4], void* stream);
/* The things env's last zs_step removed in World.clean_dead_things (core.py:121-138), in removal order
 * (the dict order at the cleanup): per thing {slot, serial, x, y, life} (its entity record's values at
 * removal), at most cap entries into out_host; *n_out = how many the step removed.  Needs
 * ZS_FLAG_DEATH_LOG; an env reset by that step reports none. */
int zs_death_log(zs_handle* h, int32_t env, int32_t* out_host, int32_t cap, int32_t* n_out, void* stream);
/* The actions env's last zs_step executed, in execution order (World.step's shuffled action list,
 * core.py:76,103-119; replaces reading World.events, core.py:68-70, whose messages the drop-in views
 * derive from it): per action {slot | kind << 8, target} with kind 1 move (target: destination
 * x | y << 16, 16 signed bits each: an agent's offset is clamped to +-16384 before it is added, so a destination
 * off the map stays off the map but a far one is not the cell the caller named; a caller that needs that cell
 * adds its own offset to the actor's position from before the step, as the drop-in envs do), 2 attack, 3 heal
 * (target: an entity slot, or -1 - obstacle index in map order); at most
 * cap entries into out_host (2 int32 each); *n_out = how many.  Needs ZS_FLAG_DEATH_LOG; an env reset by
 * that step reports none.  A step a debug raise stopped (ZS_ACT_RAISE) reports *n_out = -1 - k and, as its
 * k entries, the actors before the raising one in dict order that decided an action (core.py:80-101: the
 * others were idle). */
int zs_action_log(zs_handle* h, int32_t env, int32_t* out_host, int32_t cap, int32_t* n_out, void* stream);

/* ---- the drop-ins' per-call path ----------------------------------------------------------------
 * ZombsoleGymEnv.step / reset / get_observation and the MultiagentZombsoleEnv equivalents
 * (zombsole/gym_env.py:93-164, zombsole/gym/multiagent_env.py:87-184) run one env per Python call and
 * read everything back on the host.  These calls do that in one host->device copy, the engine's
 * launches, one device->host copy and one synchronisation, on engine-owned device outputs:
 *   zs_host_step(h, actions_host [N][A][3], rng_host, rec_host)  = zs_set_rng + zs_step + read-back
 *   zs_host_reset(h, rng_host, rec_host)                         = zs_set_rng + zs_reset (all envs) + read-back
 *   zs_host_observe(h, rec_host)                                 = zs_observe + read-back
 * rng_host: NULL, or [N][625] words of CPython random.getstate() form moved into the envs' streams
 * before the call (the process-global stream the reference draws from).  rec_host: [N][words] int32
 * records, each with the fixed header below and the sections zs_host_layout gives:
 *   out[0] words per record, out[1] rewards (float64 [R]), out[2] action log (2E words, zs_action_log
 *   form), out[3] death log (5E words, zs_death_log form), out[4] state record (zs_get_state form),
 *   out[5] observation (out[6] bytes, zs_obs_shape of the config's dtype), out[7] R (1 single, A multi).
 * The record always holds the env's stream after the call (rng section), so the caller moves it back into
 * `random` even when zs_host_reset fails with ZS_ENOSPACE. */
#define ZS_HOST_FLAGS 0  /* bit 0 done, bit 1 truncated, bit 2 autoreset by this call                 */
#define ZS_HOST_ERR 1    /* the engine's error word for the call (ZS_ENOSPACE: players could not spawn) */
#define ZS_HOST_ALOG_N 2 /* zs_action_log's n                                                           */
#define ZS_HOST_DLOG_N 3 /* zs_death_log's n                                                            */
#define ZS_HOST_RNG 4    /* 625 words: the env's stream in random.getstate() form                        */
int zs_host_layout(zs_handle* h, int32_t out[8]);
int zs_host_step(zs_handle* h, const int32_t* actions_host, const uint32_t* rng_host, int32_t* rec_host, void* stream);
int zs_host_reset(zs_handle* h, const uint32_t* rng_host, int32_t* rec_host, void* stream);
int zs_host_observe(zs_handle* h, int32_t* rec_host, void* stream);
/* Diagnostic builds compiled with -DZS_STAMPS only (the product .so returns ZS_ESTATE):
 * per-phase k_tick cycle sums / maxima over all workgroup launches since the last call. */
int zs_debug_stamps(zs_handle* h, uint64_t* sum_out, uint64_t* max_out, int32_t n);
/* Diagnostic builds only: out[2w], out[2w + 1] = start / end s_memrealtime (100 MHz) of workgroup w
 * of the last fused step launch (k_step), w < n. */
int zs_debug_timeline(zs_handle* h, uint64_t* out, int32_t n);
/* Diagnostic builds only: out[w * n_phase + k] = cycles of phase k of workgroup w of the step launches
 * since the last zs_debug_stamps / zs_debug_stamps_wg call (the step kernel's slots only), w < n_wgs. */
int zs_debug_stamps_wg(zs_handle* h, uint64_t* out, int32_t n_wgs, int32_t n_phase);

/* Flat state record, int32 words:
 *   [0]  t (World.t)          [1] deaths            [2] zombie_deaths
 *   [3]  episode_steps        [4] n_order (things with ask_for_actions + ... present, dict order)
 *   [5]  needs_reset          [6] n_entities (E)    [7] n_obstacles (O)
 *   [8]  width                [9] height            [10] reward prev zombie_deaths
 *   [11] n_zombies_present    [12] spawn serial counter [13..15] reserved
 *   zs_set_state restores every field except the read-only [6..9], [11]; [5] must equal the
 *   engine's own flag for that env (pending resets are the engine's work lists), else ZS_EINVAL;
 *   an obstacle life below -2147483647 is refused (ZS_EINVAL)
 *   [16 .. 16+8E)  entity records: kind, present, x, y, life, weapon, extra, spawn_serial
 *                  (slots: agents [0,A), bots [A,A+P), zombies [A+P,E))
 *   [.. +E)        order: entity slot ids in dict order (first n_order valid)
 *   [.. +O)        obstacle life      [.. +O) obstacle present (0/1)
 *   [.. +A)        reward tracker previous life per agent
 *   [.. +A)        listed (agent in env.agents) per agent
 *   [.. +ceil(W*H/32)) dead-body bitmap, bit (y*W+x)
 */
#define ZS_STATE_HEADER 16
#define ZS_STATE_ENTITY_WORDS 8

#ifdef __cplusplus
}
#endif
#endif /* ZOMBSOLE_MI355X_H */
