// zs_launch.hpp — host launchers of the engine's kernels.
//
// The kernels are compiled in several translation units so the library builds in parallel:
//   k_tick_g.hip  once per lanes-per-env G (-DZS_G=1..64): k_tick<G, 5/6> and the fused k_step<G>
//   k_obs_t.hip   once per observation dtype (-DZS_OBS_T=0/1/2): every observation kernel
//   k_reset.hip   k_reset, k_respawn, k_list_filter
//   k_mask.hip    k_action_mask (zs_mask.hpp)
//   k_autopilot.hip  k_autopilot (zs_autopilot.hpp, with its launcher's declaration)
//   k_entity_act.hip  k_entity_act_decode, k_entity_act_mask, k_entity_act_encode (zs_entity_act.hpp, with their launchers'
//                     declarations)
//   k_nav.hip     k_nav (zs_nav.hpp): path-distance fields
//   k_env_params.hip  k_env_params, k_env_params_get, k_env_params_init, k_env_params_check (ZS_FLAG_ENV_PARAMS)
//   k_episode.hip  k_episode_stats, k_episode_get, k_episode_clear (ZS_FLAG_EPISODE_STATS; zs_episode.hpp)
//   k_render.hip  k_render, k_render_track (ZS_FLAG_RENDER; zs_render.hpp)
//   k_records.hip  the per-env record movers: k_obs_state_pack, k_obs_state_unpack (zs_obs_state.hpp), k_snapshot,
//                  k_restore, k_pending_list (zs_snapshot.hpp, zs_record.hpp)
//   k_state.hip   the small helpers: k_seed, k_gen_actions, k_gen_actions_ctr, k_tail, k_get_state, k_set_state,
//                 k_host_unpack, k_host_pack, k_init_pending, k_init_obstacles
//   engine.hip    the handle and the C ABI, host code only (the launches are planned in zs_obs_plan.hpp, zs_step_plan.hpp)
// Each unit exports plain host functions that launch its kernels, with the launch geometry; nothing but Dev, the
// observation plan's ObsKernel (zs_obs_plan.hpp), plain structs and plain pointers crosses the units.
#pragma once
#include "zs_device.hpp"
#include "zs_render.hpp"  // RenderPlan, RenderAtlas
#include "zs_nav.hpp"     // NavArgs, NavPlan

struct ObsStateLayout;  // zs_obs_state.hpp
struct RecTable;        // zs_record.hpp

// one step launch's arguments (k_tick, or k_step when fused)
struct TickArgs {
    const int32_t* actions;
    double* rew;
    uint8_t* done;
    uint8_t* trunc;
    uint8_t* listed;
    uint8_t* reset_out;
    int* rlist;          // the pending-reset list this step appends to
    int* rcount;
    void* obs;
    int env0, env1;      // k_tick's env range
    int n_reset;         // k_step: reset-work workgroups ahead of the tick workgroups
    const int* cur_list;  // k_step: the pending list this step drains
    const int* cur_count;
    int* err;
};

#define ZS_TICK_DECL(G)                                                                                          \
    hipError_t launch_tick_g##G(int fused, int waves, unsigned grid, size_t lds, hipStream_t s, const Dev& d, \
                                const TickArgs& a);                                                            \
    hipError_t stamps_g##G(unsigned long long* wg, unsigned long long* tl, int clear);
ZS_TICK_DECL(1)
ZS_TICK_DECL(2)
ZS_TICK_DECL(4)
ZS_TICK_DECL(8)
ZS_TICK_DECL(16)
ZS_TICK_DECL(32)
ZS_TICK_DECL(64)
#undef ZS_TICK_DECL

// observation kernels
// one launch: the plan's kernel (zs_obs_plan.hpp) over the caller's buffers and env range
struct ObsLaunch {
    ObsKernel k;
    unsigned grid;
    void* obs;
    const uint8_t* mask;
    int env0, env1;
};
#define ZS_OBS_DECL(T)                                                              \
    hipError_t launch_obs_##T(const ObsLaunch& o, hipStream_t s, const Dev& d); \
    hipError_t obs_lds_attr_##T(int kind, int nobs, int patched, int bytes);
ZS_OBS_DECL(i64)
ZS_OBS_DECL(i32)
ZS_OBS_DECL(i16)
#undef ZS_OBS_DECL

// reset work
hipError_t launch_reset_k(unsigned grid, size_t lds, hipStream_t s, const Dev& d, int list_mode, const int* list,
                          const int* count, const uint8_t* mask, int* err, void* obs);
hipError_t launch_respawn_k(unsigned grid, size_t lds, hipStream_t s, const Dev& d);
hipError_t launch_list_filter(unsigned grid, hipStream_t s, const int* src, const int* src_count, int* dst,
                              int* dst_count, const uint8_t* mask, int N);
hipError_t reset_lds_attr(int bytes);
hipError_t stamps_reset(unsigned long long* wg, int clear);

// action masks (zs_mask.hpp): uint8 [N][A][8] into out, 8-byte aligned, for the envs whose env_mask byte is
// nonzero (null: all)
hipError_t launch_action_mask(hipStream_t s, const Dev& d, const uint8_t* env_mask, void* out);

// path-distance fields (k_nav.hip; zs_nav.hpp).  launch_nav: the rows int16 [N][A][F][8] of the envs whose env_mask byte
// is nonzero (null: all) into out, 8-byte aligned.  launch_nav_field: frame k < n (uint16 [H][W]) of env env_idx[k]
// (null: k) and the one field g.fields into out + k * W * H; an env outside [0, N) leaves its frame untouched
hipError_t launch_nav(hipStream_t s, const Dev& d, const NavArgs& g, const uint8_t* env_mask, void* out);
hipError_t launch_nav_field(hipStream_t s, const Dev& d, const NavArgs& g, const int32_t* env_idx, int n, void* out);

// per-env zombie counts and time limits (k_env_params.hip; ZS_FLAG_ENV_PARAMS handles): entry k
// < n of params ([n][3]) into the next triple of env idx[k] (null: k), two launches (owner: int32 [N] scratch, -1
// between calls); the next or current triples of all envs as [N][3]; both triples = the config's, owner = -1
hipError_t launch_env_params_set(hipStream_t s, const Dev& d, int32_t* owner, const int32_t* idx, int n, const int32_t* params);
hipError_t launch_env_params_get(hipStream_t s, const Dev& d, int current, int32_t* out);
hipError_t launch_env_params_init(hipStream_t s, const Dev& d, int32_t* owner);
hipError_t launch_env_params_check(hipStream_t s, const Dev& d, uint32_t* out);  // *out = the range word; its PARAM_RANGE bit cleared

// per-env episode statistics (k_episode.hip; ZS_FLAG_EPISODE_STATS handles).  The statistics' arrays are the handle's
// own and reach these kernels alone, as their argument: the Dev has no field for them.
struct EpisodeArgs {
    int N, R, A, P, E, rules;
    int initial_zombies, minimum_zombies, max_steps;  // the config's triple (envp null)
    const int32_t* envp;  // ZS_FLAG_ENV_PARAMS: the running episodes' triples, [3][N] (envp_cur()), else null
    const int32_t* scal;  // Dev::scal
    const int32_t* life;  // Dev::life
    uint32_t* run;        // [ZS_EP_RUN_COLS(R)][N] (zs_episode.hpp)
    double* last_ret;     // [R][N]
    double* sum_ret;      // [R][N]
    int32_t* last;        // [8][N]
    uint32_t* tot;        // [8][N]
};
// the step's last launch: the update rule over the step's outputs (was_reset: the tick's reset_out, never null);
// the columns into env-major tensors (any null) for the envs whose mask byte is nonzero (null: all); the masked envs'
// running part (running != 0) or last episode and totals, zeroed
hipError_t launch_episode_stats(hipStream_t s, const EpisodeArgs& a, const double* rew, const uint8_t* done, const uint8_t* trunc,
                                const uint8_t* was_reset);
hipError_t launch_episode_get(hipStream_t s, const EpisodeArgs& a, const uint8_t* mask, double* run_ret, double* last_ret,
                              double* sum_ret, int32_t* last, uint32_t* tot);
hipError_t launch_episode_clear(hipStream_t s, const EpisodeArgs& a, const uint8_t* mask, int running);

// the picture of a ZS_FLAG_RENDER handle's envs (k_render.hip; zs_render.hpp).  Like the statistics' arrays, body_col
// and the atlas are the handle's own and reach these kernels alone, as their argument: the Dev has no field for them.
struct RenderArgs {
    int N, W, H, E, O, OW, DW;
    RenderPlan plan;
    const int32_t* pos;           // Dev::pos
    const uint8_t* present;       // Dev::present
    const int32_t* scell;         // Dev::scell
    const uint32_t* obst_present; // Dev::obst_present
    const uint32_t* dead;         // Dev::dead
    const int32_t* dlog;          // Dev::dlog
    const int32_t* dlog_n;        // Dev::dlog_n
    uint8_t* body_col;            // [N][plan.body_bytes]: per cell the palette index of its last body, 0 = none recorded
    const uint8_t* slot_col;      // [E] static: the palette index of a slot's thing
    RenderAtlas atlas;
};
inline unsigned zs_render_track_grid(int n) { return (unsigned)((n + ZS_RENDER_BLOCK - 1) / ZS_RENDER_BLOCK); }
// mode 0: a step's tracker (flags: the tick's reset_out, never null); mode 1: clear the rows of the envs whose flag
// byte is nonzero (null: all).  launch_render: frames k < min(n, n_frames) of env envs[k] (null: k) into
// out + k * plan.frame_bytes, any alignment; an env outside [0, N) leaves its frame untouched
hipError_t launch_render_track(hipStream_t s, const RenderArgs& a, const uint8_t* flags, int mode);
hipError_t launch_render(hipStream_t s, const RenderArgs& a, const int32_t* envs, int n, uint8_t* out, int n_frames);

// per-env records (k_records.hip).  Observation-state records (zs_obs_state.hpp), rec 16-B aligned: the handle's N
// envs into rec [N][L.rec_bytes]; records [n] into envs env0 .. env0 + n - 1.  Snapshot records (zs_snapshot.hpp) by
// the handle's section table T: record k = env idx[k] (null: k); record src[k] of n_records into env dst[k], the
// written envs' log counts and *list_count zeroed; list = the envs whose needs_reset is set, *count past them
hipError_t launch_obs_state_pack(hipStream_t s, const Dev& d, const ObsStateLayout& L, void* rec);
hipError_t launch_obs_state_unpack(hipStream_t s, const Dev& d, const ObsStateLayout& L, int env0, int n, const void* rec);
hipError_t launch_snapshot(hipStream_t s, const RecTable& T, int N, const int32_t* idx, int n, void* rec);
hipError_t launch_restore(hipStream_t s, const RecTable& T, const Dev& d, const int32_t* src, const int32_t* dst, int n,
                          int n_records, const void* rec, int* list_count);
hipError_t launch_pending_list(hipStream_t s, const int32_t* needs_reset, int N, int* list, int* count);

// Word offsets of a host record's sections (ZS_HOST_* in include/zombsole_mi355x.h, zs_host_layout)
struct HostLayout {
    int words, rew, alog, dlog, state, obs, obs_bytes, R;
};

// the small helpers (k_state.hip)
hipError_t launch_seed(hipStream_t s, const Dev& d, int env0, int n, const uint64_t* seeds);
hipError_t launch_gen_actions(hipStream_t s, const Dev& d, uint64_t step, int n_discrete, int32_t* act);
hipError_t launch_gen_actions_ctr(hipStream_t s, const Dev& d, const uint64_t* ctr, int n_discrete, int32_t* act);
hipError_t launch_tail(hipStream_t s, const Dev& d);  // the step's tail (Dev::tail_*) when no observation launch ends the step
hipError_t launch_get_state(hipStream_t s, const Dev& d, int e, int32_t* buf);
hipError_t launch_set_state(hipStream_t s, const Dev& d, int e, const int32_t* buf, int* err);
hipError_t launch_host_unpack(hipStream_t s, const Dev& d, const uint32_t* rings, const uint32_t* st, int* err);
hipError_t launch_host_pack(hipStream_t s, const Dev& d, const HostLayout& L, const uint8_t* obs, const double* rew,
                            const uint8_t* done, const uint8_t* trunc, const uint8_t* rst, int* err, int32_t* rec);
hipError_t launch_init_pending(hipStream_t s, const Dev& d, int* list, int* count);
hipError_t launch_init_obstacles(hipStream_t s, const Dev& d);
