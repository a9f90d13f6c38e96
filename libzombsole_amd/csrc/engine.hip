// engine.hip — the handle and the C ABI of the MI355X-native batched zombsole step engine (gfx950): host code only.
//
// The kernels live in their own units behind plain launchers (zs_launch.hpp).  A step (zs_step) is: k_reset
// (zs_reset.hpp, one wave per env that ended at the previous step, on a side stream concurrent with the tick, or
// fused with it into k_step), k_tick (zs_tick.hpp, 64/G envs per wave with G lanes per env and the env's hot state
// in LDS), k_respawn (deferred zombie respawns, one wave per env) and the observation kernel (zs_obs.hpp: k_obs_ring /
// k_obs_pipe persistent store streams, k_obs_gather for large maps, k_obs in general), else k_tail, then k_action_mask
// (zs_mask.hpp) when a mask buffer is bound and k_entity_obs (k_entity_obs.hip, zs_entity_obs.hpp) when an entity
// buffer is, then k_entity_act_mask (k_entity_act.hip, zs_entity_act.hpp) when an entity-action mask buffer is (bound
// entity-action ids are decoded into the step's actions by k_entity_act_decode, the step's first launch), then k_nav (k_nav.hip, zs_nav.hpp) when a path-distance buffer is, then k_autopilot (k_autopilot.hip,
// zs_autopilot.hpp) when a policy is bound.  With a null obs_dev no grid
// observation is written and k_tail ends the step.  zs_step_graph replays a step as a hipGraph.  The small helpers behind the
// ABI (seeding, the policy stream, the state views, the drop-ins' per-call records) are k_state.hip's; the per-env
// record movers (observation-state records, zs_obs_state.hpp; snapshot records, zs_snapshot.hpp and zs_record.hpp) are
// k_records.hip's; k_env_params.hip scatters per-env zombie counts and time limits (ZS_FLAG_ENV_PARAMS); a
// ZS_FLAG_EPISODE_STATS handle's step ends with k_episode_stats (k_episode.hip, zs_episode.hpp); a ZS_FLAG_RENDER
// handle's with k_render_track, and zs_render draws its envs (k_render.hip, zs_render.hpp).
//
// Semantics follow the reference exactly (parity: tests/); every sqrt range
// test of the reference is replaced by its exact integer d^2 equivalent.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdio>
#include <cstring>
#include <string>
#include <vector>

#include "zs_launch.hpp"  // zs_device.hpp (Dev), the plans (zs_obs_plan.hpp, zs_step_plan.hpp)
#include "zs_obs_state.hpp"
#include "zs_snapshot.hpp"
#include "zs_record.hpp"
#include "zs_mask.hpp"  // the mask launch's geometry (zs_describe); the kernel is k_mask.hip's
#include "zs_entity_obs.hpp"  // the entity observation's layout and launcher; the kernel is k_entity_obs.hip's
#include "zs_entity_act.hpp"  // the entity action table's layout and launchers; the kernels are k_entity_act.hip's
#include "zs_autopilot.hpp"  // the scripted policies' launcher and geometry; the kernel is k_autopilot.hip's
#include "zs_episode.hpp"  // the running part's columns (ZS_EP_RUN_COLS); the kernels are k_episode.hip's

// ===========================================================================
// host side: C ABI
// ===========================================================================
static thread_local std::string g_err;

static int fail(int code, const std::string& msg) {
    g_err = msg;
    return code;
}

// the observation launcher of the handle's output dtype (k_obs_t.hip)
static hipError_t obs_launch(int dtype, const ObsLaunch& o, hipStream_t s, const Dev& d) {
    return dtype == ZS_DTYPE_I64 ? launch_obs_i64(o, s, d) : dtype == ZS_DTYPE_I32 ? launch_obs_i32(o, s, d) : launch_obs_i16(o, s, d);
}
static hipError_t obs_attr(int dtype, int kind, int nobs, int patched, int bytes) {
    return dtype == ZS_DTYPE_I64   ? obs_lds_attr_i64(kind, nobs, patched, bytes)
           : dtype == ZS_DTYPE_I32 ? obs_lds_attr_i32(kind, nobs, patched, bytes)
                                   : obs_lds_attr_i16(kind, nobs, patched, bytes);
}

#define HIPCHK(x)                                                                              \
    do {                                                                                       \
        hipError_t _e = (x);                                                                   \
        if (_e != hipSuccess) return fail(ZS_EHIP, std::string(#x ": ") + hipGetErrorString(_e)); \
    } while (0)

// a step that returns a ZS_* status and has set the message: a failure is the caller's result
#define TRY(x)             \
    do {                   \
        int _r = (x);      \
        if (_r) return _r; \
    } while (0)

// a kernel launch's status under the kernel's name: "k_x: <hip error string>"
static int launched(const char* name, hipError_t e) {
    return e == hipSuccess ? ZS_OK : fail(ZS_EHIP, std::string(name) + ": " + hipGetErrorString(e));
}
#define LAUNCHCHK(name, x) TRY(launched((name), (x)))

struct zs_handle {
    zs_config cfg;
    zs_launch ov;   // launch overrides (zs_config.launch, zeroed when NULL)
    int device;
    Dev d;
    ObsPlan obs;    // the observation kernels of an unmasked and of a masked launch (zs_obs_plan.hpp)
    StepPlan step;  // the step, reset and respawn launches (zs_step_plan.hpp)
    // zs_step_graph: one captured hipGraph per autoreset-list parity (the step alternates the two
    // pending-reset lists), replayed on the caller's stream; keyed by the caller's buffers
    // a few buffer sets cached (a caller alternating double-buffered outputs, vector.StepGather)
    struct GraphSet {
        hipGraphExec_t g[2] = {nullptr, nullptr};  // per pending-list parity
        const void* key[9] = {};
        uint64_t used = 0;
    };
    static const int kGraphSets = 4;
    GraphSet gsets[kGraphSets];
    uint64_t gclock = 0;
    bool graphs_stale = false;  // zs_entity_act_bind changed what a step launches: the sets are dropped before the next replay
    // the policy step counter's block (GS_*, zs_device.hpp: the step's policy reads the counter, the step's tail advances
    // it) and the policy's triples kept one step ahead, int32 [N][A][3]: the handle's own, since a caller may write
    // into its action buffer between replays
    uint64_t* d_gstep = nullptr;
    int32_t* d_ahead = nullptr;
    int graph_pol = 0;            // zs_step_graph is capturing a step with this policy (n_discrete), else 0
    const char* step_policy = "";  // where the last captured policy step takes its actions from (zs_describe)
    // next-step reset work on a side stream, concurrent with the tick (the two touch disjoint envs);
    // the caller's stream joins it before the observations (step.side_stream, and the stream exists)
    int reset_side = 0;
    hipStream_t s_reset = nullptr;
    hipEvent_t ev_rfork = nullptr, ev_rjoin = nullptr;
    int state_words;
    std::vector<void*> allocs;
    int32_t* d_state;
    uint64_t* d_seedbuf;
    int* d_err;
    // next-step autoreset work lists: k_tick appends to list[1-par], k_reset drains list[par]
    int* d_rlist[2];
    int* d_rcount;  // [2]
    int rpar = 0;
    uint64_t snap_fp = 0;  // snapshot_fingerprint() of the config (zs_snapshot.hpp)
    int32_t* d_envp_owner = nullptr;  // ZS_FLAG_ENV_PARAMS: zs_env_params_set's scratch, int32 [N], -1 between calls
    void* mask_bound = nullptr;  // zs_action_mask_bind: every zs_step ends with a mask launch into it
    // the entity observation (zs_entity_obs.hpp): the objective list its kernel reads, and zs_entity_obs_bind's buffer
    // and K values (every zs_step ends with a launch into it)
    int32_t* d_obj_xy = nullptr;
    void* ent_bound = nullptr;
    int ent_kz = 0, ent_kp = 0;
    // zs_entity_act_bind: every zs_step begins with the decode of these ids (int32 [N][A]) into its actions, and launches
    // the table's masks into this buffer after a bound entity-observation launch
    const int32_t* eact_ids = nullptr;
    void* eact_mask = nullptr;
    int eact_kz = 0, eact_kp = 0;
    // path-distance fields (zs_nav.hpp): the launch plan of the handle's map, and zs_nav_bind's buffer, fields and cap
    // (every zs_step ends with a launch into it)
    NavPlan nav{};
    void* nav_bound = nullptr;
    int nav_fields = 0, nav_max_dist = 0;
    // zs_autopilot_bind: every zs_step ends with an autopilot launch of this policy (uint8 [N][A]) into these triples
    const uint8_t* pilot_policy = nullptr;
    int32_t* pilot_out = nullptr;
    const char* step_last = "";  // the launch that carried the tail of the last zs_step queued or captured (zs_describe)
    // ZS_FLAG_EPISODE_STATS: the statistics' arrays (k_episode.hip's argument; ep.run null without the flag) and the
    // [N] byte row the tick writes its reset flags to when the caller passes no reset_dev
    EpisodeArgs ep{};
    uint8_t* d_ep_reset = nullptr;
    // ZS_FLAG_RENDER: k_render.hip's argument (rn.body_col null without the flag); it shares d_ep_reset
    RenderArgs rn{};
    // the drop-ins' per-call path (zs_host_*), set up by its first call: one pinned, device-mapped input
    // block (actions, then the `random` state as rings + st words) the kernels read in place, one pinned,
    // device-mapped record block k_host_pack writes in place, one synchronisation per call
    HostLayout hl{};
    int32_t* h_hin = nullptr;   // pinned host memory ...
    int32_t* d_hin = nullptr;   // ... and its device address
    int32_t* h_hrec = nullptr;
    int32_t* d_hrec = nullptr;
    uint8_t* d_hobs = nullptr;
    double* d_hrew = nullptr;
    uint8_t* d_hflags = nullptr;  // done [N], trunc [N], listed [N][A], reset [N]
    // diagnostics: HIP events bracketing every k_tick / k_obs launch on its stream
    int prof = 0;
    std::vector<hipEvent_t> ev_pool;
    std::vector<std::pair<int, int>> ev_tick, ev_obs, ev_reset, ev_respawn;  // (start, end) indices into ev_pool (EventList)
    size_t ev_next = 0;
};

static hipEvent_t prof_event(zs_handle* h, int* idx) {
    if (h->ev_next == h->ev_pool.size()) {
        hipEvent_t ev;
        if (hipEventCreate(&ev) != hipSuccess) return nullptr;
        h->ev_pool.push_back(ev);
    }
    *idx = (int)h->ev_next;
    return h->ev_pool[h->ev_next++];
}

typedef std::vector<std::pair<int, int>> EventList;

// launch() (a hipError_t; `what` names it in the error text) on s, between two events of a profiling handle
// (zs_profile), the pair appended to `list`
template <typename F>
static int timed_launch(zs_handle* h, hipStream_t s, EventList& list, const char* what, F launch) {
    int i0 = -1, i1 = -1;
    if (h->prof) HIPCHK(hipEventRecord(prof_event(h, &i0), s));
    LAUNCHCHK(what, launch());
    if (h->prof) {
        HIPCHK(hipEventRecord(prof_event(h, &i1), s));
        list.push_back({i0, i1});
    }
    return ZS_OK;
}

// zs_profile, zs_profile_read: nothing recorded, every pooled event free again
static void prof_clear(zs_handle* h) {
    for (EventList* l : {&h->ev_tick, &h->ev_obs, &h->ev_reset, &h->ev_respawn}) l->clear();
    h->ev_next = 0;
}

// both graphs of a set destroyed (the first failure's status returned, the rest still destroyed)
static hipError_t destroy_graphs(zs_handle::GraphSet& gs) {
    hipError_t first = hipSuccess;
    for (hipGraphExec_t& g : gs.g) {
        const hipError_t e = g ? hipGraphExecDestroy(g) : hipSuccess;
        if (first == hipSuccess) first = e;
        g = nullptr;
    }
    return first;
}

// the error word of the launches queued on s, read back and left clear (every reader leaves it clear); synchronises s
static int read_error_word(zs_handle* h, hipStream_t s, int* err) {
    *err = 0;
    HIPCHK(hipMemcpyAsync(err, h->d_err, sizeof(int), hipMemcpyDeviceToHost, s));
    HIPCHK(hipMemsetAsync(h->d_err, 0, sizeof(int), s));
    HIPCHK(hipStreamSynchronize(s));
    return ZS_OK;
}

// what a reset's error word means to the caller (zs_reset, the drop-ins' per-call path)
static int reset_result(int err) {
    if (err == ZS_ENOSPACE) return fail(ZS_ENOSPACE, "Not enough space to spawn players/agents");
    return err ? fail(err, "reset failed") : ZS_OK;
}

extern "C" const char* zs_last_error(void) { return g_err.c_str(); }

// a viewer handle (ZS_FLAG_VIEWER) holds other handles' envs for encoding: nothing steps, seeds or resets it
static int viewer_refused(const zs_handle* h, const char* call) {
    if (!(h->cfg.flags & ZS_FLAG_VIEWER)) return ZS_OK;
    return fail(ZS_ESTATE, std::string(call) + ": not on a viewer handle (ZS_FLAG_VIEWER)");
}
#define NOT_ON_VIEWER(h, call) TRY(viewer_refused((h), (call)))

// an entry point's prologue: the caller's stream, and the handle's device current
static int enter(const zs_handle* h, void* stream, hipStream_t* s) {
    *s = (hipStream_t)stream;
    HIPCHK(hipSetDevice(h->device));
    return ZS_OK;
}
#define ENTER(h, stream, s) \
    hipStream_t s;          \
    TRY(enter((h), (stream), &s))

// a call of a feature the handle was created without
static int need_flag(const char* call, bool have, const char* flag) {
    if (have) return ZS_OK;
    return fail(ZS_ESTATE, std::string(call) + ": the handle was created without " + flag);
}

// a record buffer (observation-state or snapshot records) starts at a 16-byte boundary
static int rec_aligned(const void* rec_dev) {
    if ((uintptr_t)rec_dev & 15) return fail(ZS_EINVAL, "rec_dev must be 16-byte aligned");
    return ZS_OK;
}

template <typename T>
static int dalloc(zs_handle* h, T** p, size_t count) {
    size_t bytes = std::max<size_t>(count * sizeof(T), 16);
    hipError_t e = hipMalloc((void**)p, bytes);
    if (e != hipSuccess) return fail(ZS_EHIP, std::string("hipMalloc: ") + hipGetErrorString(e));
    h->allocs.push_back(*p);
    e = hipMemset(*p, 0, bytes);
    if (e != hipSuccess) return fail(ZS_EHIP, std::string("hipMemset: ") + hipGetErrorString(e));
    return ZS_OK;
}

template <typename T>
static int dupload(zs_handle* h, T** p, const std::vector<T>& v) {
    TRY(dalloc(h, p, v.size()));
    if (!v.empty()) HIPCHK(hipMemcpy(*p, v.data(), v.size() * sizeof(T), hipMemcpyHostToDevice));
    return ZS_OK;
}

// the same into one of Dev's read-only tables
template <typename T>
static int dupload(zs_handle* h, const T** p, const std::vector<T>& v) {
    T* q = nullptr;
    const int rc = dupload(h, &q, v);
    *p = q;
    return rc;
}

static void free_all(zs_handle* h) {
    for (void* p : h->allocs) (void)hipFree(p);
    h->allocs.clear();
    if (h->h_hin) (void)hipHostFree(h->h_hin);
    if (h->h_hrec) (void)hipHostFree(h->h_hrec);
    h->h_hin = h->h_hrec = nullptr;
    if (h->ev_rfork) (void)hipEventDestroy(h->ev_rfork);
    if (h->ev_rjoin) (void)hipEventDestroy(h->ev_rjoin);
    h->ev_rfork = h->ev_rjoin = nullptr;
    if (h->s_reset) (void)hipStreamDestroy(h->s_reset);
    h->s_reset = nullptr;
    for (auto& gs : h->gsets) (void)destroy_graphs(gs);
    for (hipEvent_t ev : h->ev_pool) (void)hipEventDestroy(ev);
    h->ev_pool.clear();
}

extern "C" int zs_destroy(zs_handle* h) {
    if (!h) return ZS_OK;
    (void)hipSetDevice(h->device);
    free_all(h);
    delete h;
    return ZS_OK;
}

static int validate(const zs_config* c) {
    if (!c || c->num_envs < 1) return fail(ZS_EINVAL, "num_envs must be >= 1");
    const zs_map_desc& m = c->map;
    if (m.width < 1 || m.height < 1 || m.width > 16000 || m.height > 16000 || (long)m.width * m.height > (1L << 24))
        return fail(ZS_EINVAL, "map size out of range");
    if (c->num_agents < 1) return fail(ZS_EINVAL, "at least one agent is required");
    if (c->num_bots < 0 || c->initial_zombies < 0 || c->minimum_zombies < 0) return fail(ZS_EINVAL, "negative count");
    long E = (long)c->num_agents + c->num_bots + std::max(c->initial_zombies, c->minimum_zombies);
    if (E > 254) return fail(ZS_EINVAL, "agents + bots + max(initial, minimum) zombies must be <= 254");
    if (c->rules == ZS_RULES_EVACUATION && c->num_agents + c->num_bots > 64)
        return fail(ZS_EINVAL, "evacuation rules support at most 64 players");
    if (c->rules < 0 || c->rules > 3) return fail(ZS_EINVAL, "bad rules id");
    if (c->obs_scope == ZS_OBS_SURROUNDINGS && (c->obs_width <= 1 || c->obs_width % 2 == 0))
        return fail(ZS_EINVAL, "surroundings width must be an odd number greater than 1");
    if (c->obs_dtype < 0 || c->obs_dtype > 2) return fail(ZS_EINVAL, "bad obs dtype");
    // the step kernels exist for these lane counts only (k_tick_g.hip); any other value would size the launch
    // for 64 / G envs per workgroup and run a kernel that ticks another number
    {
        const int g = c->lanes_per_env;
        if (g != 0 && (g < 1 || g > 64 || (g & (g - 1)) != 0))
            return fail(ZS_EINVAL, "lanes_per_env must be 0 (automatic) or a power of two in 1..64");
    }
    for (int i = 0; i < m.n_obstacles; i++) {
        int x = m.obstacle_xy[2 * i], y = m.obstacle_xy[2 * i + 1];
        if (x < 0 || y < 0 || x >= m.width || y >= m.height) return fail(ZS_EINVAL, "obstacle out of bounds");
        if (m.obstacle_kind[i] != ZS_THING_BOX && m.obstacle_kind[i] != ZS_THING_WALL) return fail(ZS_EINVAL, "bad obstacle kind");
    }
    const int32_t* lists[3] = {m.objective_xy, m.player_spawn_xy, m.zombie_spawn_xy};
    int ns[3] = {m.n_objectives, m.n_player_spawns, m.n_zombie_spawns};
    for (int l = 0; l < 3; l++)
        for (int i = 0; i < ns[l]; i++) {
            int x = lists[l][2 * i], y = lists[l][2 * i + 1];
            if (x < 0 || y < 0 || x >= m.width || y >= m.height) return fail(ZS_EINVAL, "map list entry out of bounds");
        }
    for (int a = 0; a < c->num_agents; a++) {
        int w = c->agent_weapons[a];
        if (!(w == ZS_WEAPON_KNIFE || w == ZS_WEAPON_AXE || w == ZS_WEAPON_GUN || w == ZS_WEAPON_RIFLE ||
              w == ZS_WEAPON_SHOTGUN || w == ZS_WEAPON_RANDOM))
            return fail(ZS_EINVAL, "bad agent weapon");
    }
    for (int p = 0; p < c->num_bots; p++)
        if (c->bot_types[p] < ZS_BOT_TERMINATOR || c->bot_types[p] > ZS_BOT_RANDOMAN) return fail(ZS_EINVAL, "bad bot type");
    return ZS_OK;
}

static int seed_envs(zs_handle* h, int32_t env0, int32_t n, const uint64_t* seeds_host, void* stream);

// zs_create's handle until it succeeds: an early return frees it with everything allocated so far
struct HandleOwner {
    zs_handle* h;
    ~HandleOwner() {
        if (!h) return;
        free_all(h);
        delete h;
    }
};

// zs_create: the static tables of the map and the config, uploaded; *rank_order: the obstacles are in
// row-major order
static int create_static_tables(zs_handle* h, const zs_config* cfg, bool* rank_order) {
    const zs_map_desc& m = cfg->map;
    Dev& d = h->d;
    // static tables
    std::vector<int16_t> cellmap((size_t)d.W * d.H, -1);
    std::vector<int32_t> oxy(d.O);
    std::vector<uint8_t> okind(d.O);
    for (int i = 0; i < d.O; i++) {
        int x = m.obstacle_xy[2 * i], y = m.obstacle_xy[2 * i + 1];
        if (cellmap[(size_t)y * d.W + x] != -1) return fail(ZS_EINVAL, "two obstacles on one cell");
        cellmap[(size_t)y * d.W + x] = (int16_t)i;
        oxy[i] = (int32_t)((uint32_t)x | ((uint32_t)y << 16));
        okind[i] = m.obstacle_kind[i];
    }
    if (d.O > 32767) return fail(ZS_EINVAL, "too many obstacles");
    std::vector<uint32_t> obstbits(d.DW, 0);
    for (int i = 0; i < d.O; i++) {
        int cell = m.obstacle_xy[2 * i + 1] * d.W + m.obstacle_xy[2 * i];
        obstbits[cell >> 5] |= 1u << (cell & 31);
    }
    // the observation store loop finds an obstacle's index as the rank of its cell among obstacle
    // cells (zs_obs.hpp), valid when the obstacles are in row-major order (every map-file parse)
    *rank_order = true;
    for (int i = 1; i < d.O; i++)
        if (m.obstacle_xy[2 * i + 1] * d.W + m.obstacle_xy[2 * i] <=
            m.obstacle_xy[2 * i - 1] * d.W + m.obstacle_xy[2 * i - 2])
            *rank_order = false;
    std::vector<uint32_t> boxbits(d.DW, 0);
    for (int i = 0; i < d.O; i++)
        if (m.obstacle_kind[i] == ZS_THING_BOX) {
            int cell = m.obstacle_xy[2 * i + 1] * d.W + m.obstacle_xy[2 * i];
            boxbits[cell >> 5] |= 1u << (cell & 31);
        }
    std::vector<int32_t> oprefix(d.DW, 0);
    for (int w = 1; w < d.DW; w++) oprefix[w] = oprefix[w - 1] + __builtin_popcount(obstbits[w - 1]);
    std::vector<uint32_t> objbits(d.DW, 0);
    std::vector<int32_t> scell((size_t)d.W * d.H, 0);  // k_obs static per-cell word (zs_obs.hpp)
    for (int i = 0; i < m.n_objectives; i++) {
        int cell = m.objective_xy[2 * i + 1] * d.W + m.objective_xy[2 * i];
        objbits[cell >> 5] |= 1u << (cell & 31);
        scell[cell] |= (int32_t)SC_OBJ_BIT;
    }
    for (int i = 0; i < d.O; i++) {
        int cell = m.obstacle_xy[2 * i + 1] * d.W + m.obstacle_xy[2 * i];
        scell[cell] |= (int32_t)((uint32_t)(i + 1) | ((uint32_t)m.obstacle_kind[i] << SC_KIND_SHIFT));
    }
    auto packlist = [](const int32_t* xy, int n) {
        std::vector<int32_t> v(n);
        for (int i = 0; i < n; i++) v[i] = (int32_t)((uint32_t)xy[2 * i] | ((uint32_t)xy[2 * i + 1] << 16));
        return v;
    };
    std::vector<int32_t> ps = packlist(m.player_spawn_xy, d.nps), zs = packlist(m.zombie_spawn_xy, d.nzs);
    std::vector<int32_t> aw(cfg->agent_weapons, cfg->agent_weapons + d.A);
    std::vector<int32_t> ac(cfg->agent_codes, cfg->agent_codes + d.A);
    std::vector<int32_t> bt(cfg->bot_types, cfg->bot_types + d.P);

    TRY(dupload(h, &d.cellmap, cellmap));
    TRY(dupload(h, &d.objbits, objbits));
    TRY(dupload(h, &d.obstbits, obstbits));
    TRY(dupload(h, &d.scell, scell));
    TRY(dupload(h, &d.boxbits, boxbits));
    TRY(dupload(h, &d.oprefix, oprefix));
    TRY(dupload(h, &d.obst_xy, oxy));
    TRY(dupload(h, &d.obst_kind, okind));
    TRY(dupload(h, &d.pspawn, ps));
    TRY(dupload(h, &d.zspawn, zs));
    TRY(dupload(h, &h->d_obj_xy, packlist(m.objective_xy, m.n_objectives)));
    h->nav = nav_plan(d.W, d.H, d.A);
    TRY(dupload(h, &d.agent_weapons, aw));
    TRY(dupload(h, &d.agent_codes, ac));
    TRY(dupload(h, &d.bot_types, bt));
    {
        // k_obs_patch's tables (zs_obs.hpp): the map padded by half a registered window (21) on every
        // side, each cell the code / life it shows with no thing on it, no body, every obstacle present
        // at MAX_LIFE (out of bounds: Wall 200, gym/observation.py:69-76); per obstacle x | y << 12 |
        // box << 24 | objective-under << 25
        const int half = 10, pw = d.W + 2 * half, ph = d.H + 2 * half;
        std::vector<uint16_t> pad((((size_t)pw * ph + 7) / 8) * 8, 0);
        for (int y = -half; y < d.H + half; y++)
            for (int x = -half; x < d.W + half; x++) {
                uint16_t v = (uint16_t)(ZS_THING_WALL | (200 << 8));
                if (x >= 0 && y >= 0 && x < d.W && y < d.H) {
                    const int c = y * d.W + x;
                    const bool obj = (objbits[c >> 5] >> (c & 31)) & 1u;
                    const int oi = cellmap[c];
                    if (oi >= 0)
                        v = okind[oi] == ZS_THING_BOX ? (uint16_t)(ZS_THING_BOX | (10 << 8)) : (uint16_t)(ZS_THING_WALL | (200 << 8));
                    else
                        v = obj ? ZS_THING_OBJECTIVE : ZS_THING_NONE;
                    if (oi >= 0 && obj) v |= OPAD_OBJ;
                }
                pad[(size_t)(y + half) * pw + x + half] = v;
            }
        std::vector<uint32_t> opk(std::max(d.O, 1), 0u);
        for (int i = 0; i < d.O; i++) {
            const int x = m.obstacle_xy[2 * i], y = m.obstacle_xy[2 * i + 1], c = y * d.W + x;
            opk[i] = (uint32_t)(x & 0xfff) | ((uint32_t)(y & 0xfff) << 12) | ((okind[i] == ZS_THING_BOX ? 1u : 0u) << 24) |
                     (((objbits[c >> 5] >> (c & 31)) & 1u) << 25);
        }
        TRY(dupload(h, &d.opad, pad));
        TRY(dupload(h, &d.opk, opk));
        d.opad_w = pw;
        d.opad_n = pw * ph;
    }
    return ZS_OK;
}

// zs_create: the per-env arrays, zeroed, and the handle's own buffers
static int create_env_arrays(zs_handle* h, const zs_map_desc& m) {
    Dev& d = h->d;
    const size_t N = d.N, E = d.E;
    TRY(dalloc(h, &d.pos, E * N));
    TRY(dalloc(h, &d.life, E * N));
    TRY(dalloc(h, &d.weapon, E * N));
    TRY(dalloc(h, &d.present, E * N));
    TRY(dalloc(h, &d.serial, E * N));
    TRY(dalloc(h, &d.order, E * N));
    // ZS_FLAG_ENV_PARAMS: both triples behind the scalar rows, [6][N] (envp_cur(), envp_next(): zs_device.hpp)
    TRY(dalloc(h, &d.scal, (size_t)(S_NSCAL + ((d.flags & ZS_FLAG_ENV_PARAMS) ? 2 * EP_N : 0)) * N));
    TRY(dalloc(h, &d.prev_life, (size_t)d.A * N));
    TRY(dalloc(h, &d.listed, (size_t)d.A * N));
    TRY(dalloc(h, &d.obst_hp, (size_t)d.O * N));
    TRY(dalloc(h, &d.hp_dirty, N));
    TRY(dalloc(h, &d.ovf, 1));
    {
        std::vector<int32_t> init(std::max(d.O, 1), 0);
        for (int i = 0; i < d.O; i++) init[i] = m.obstacle_kind[i] == ZS_THING_BOX ? 10 : 200;  // Box / Wall MAX_LIFE
        TRY(dupload(h, &d.hp_init, init));
        d.hp_chunk = std::max(1, (d.O + 31) / 32);
        d.hp_chunk_m = (uint32_t)(((1u << 20) + d.hp_chunk - 1) / d.hp_chunk);
        d.hp_chunk_m32 = (uint32_t)(((1ull << 32) + d.hp_chunk - 1) / d.hp_chunk);
        std::vector<uint32_t> full(std::max(d.OW, 1), 0u);
        for (int w = 0; w < d.OW; w++) full[w] = d.O - 32 * w >= 32 ? 0xffffffffu : ((1u << (d.O - 32 * w)) - 1u);
        TRY(dupload(h, &d.opres_full, full));
    }
    TRY(dalloc(h, &d.obst_present, (size_t)d.OW * N));
    TRY(dalloc(h, &d.obst_nonpos, (size_t)d.OW * N));
    TRY(dalloc(h, &d.dead, (size_t)d.DW * N));
    TRY(dalloc(h, &d.dead_dirty, N));
    {
        std::vector<uint32_t> zero(std::max(d.DW, 1), 0u);
        TRY(dupload(h, &d.dead_zero, zero));
        d.dead_chunk = std::max(1, (d.DW + 31) / 32);
        d.dead_chunk_m = (uint32_t)(((1u << 20) + d.dead_chunk - 1) / d.dead_chunk);
        d.dead_chunk_m32 = (uint32_t)(((1ull << 32) + d.dead_chunk - 1) / d.dead_chunk);
        // exact for every cell when cells * (w_m * W - 2^20) < 2^20 (w_m * W - 2^20 < W)
        d.w_m = (long)d.W * d.H * d.W < (1L << 20) ? (uint32_t)(((1u << 20) + d.W - 1) / d.W) : 0u;
    }
    TRY(dalloc(h, &d.ring, (size_t)ZS_RING_WORDS * N));
    TRY(dalloc(h, &d.rngst, N));
    TRY(dalloc(h, &d.seeds, N));
    TRY(dalloc(h, &d.cand, (size_t)d.ncand * N));
    h->state_words = ZS_STATE_HEADER + ZS_STATE_ENTITY_WORDS * d.E + d.E + 2 * d.O + 2 * d.A + d.DW;
    TRY(dalloc(h, &h->d_state, (size_t)h->state_words));
    TRY(dalloc(h, &h->d_seedbuf, N));
    TRY(dalloc(h, &h->d_err, 1));
    TRY(dalloc(h, &h->d_rlist[0], N));
    TRY(dalloc(h, &h->d_rlist[1], N));
    TRY(dalloc(h, &h->d_rcount, 2));
    TRY(dalloc(h, &d.resp_list, N));
    if (d.flags & ZS_FLAG_DEATH_LOG) {
        TRY(dalloc(h, &d.dlog, (size_t)N * E * 5));
        TRY(dalloc(h, &d.dlog_n, N));
        TRY(dalloc(h, &d.alog, (size_t)N * E * 2));
        TRY(dalloc(h, &d.alog_n, N));
    }
    TRY(dalloc(h, &d.resp_count, 1));
    if (d.flags & ZS_FLAG_ENV_PARAMS) {
        TRY(dalloc(h, &h->d_envp_owner, N + 1));  // and, behind the row, zs_env_params_check's word
    }
    if (d.flags & ZS_FLAG_EPISODE_STATS) {
        EpisodeArgs& a = h->ep;
        const size_t R = d.reward_mode == ZS_REWARD_SINGLE ? 1 : d.A;
        a.N = d.N, a.R = (int)R, a.A = d.A, a.P = d.P, a.E = d.E, a.rules = d.rules;
        a.initial_zombies = d.initial_zombies, a.minimum_zombies = d.minimum_zombies, a.max_steps = d.max_steps;
        a.envp = (d.flags & ZS_FLAG_ENV_PARAMS) ? envp_cur(d) : nullptr;
        a.scal = d.scal, a.life = d.life;
        TRY(dalloc(h, &a.run, (size_t)ZS_EP_RUN_COLS(R) * N));
        TRY(dalloc(h, &a.last_ret, R * N));
        TRY(dalloc(h, &a.sum_ret, R * N));
        TRY(dalloc(h, &a.last, (size_t)ZS_EP_LAST * N));
        TRY(dalloc(h, &a.tot, (size_t)ZS_EP_TOT * N));
        TRY(dalloc(h, &h->d_ep_reset, N));
    }
    if (d.flags & ZS_FLAG_RENDER) {
        RenderArgs& a = h->rn;
        a.N = d.N, a.W = d.W, a.H = d.H, a.E = d.E, a.O = d.O, a.OW = d.OW, a.DW = d.DW;
        a.plan = render_plan(d.W, d.H);
        a.pos = d.pos, a.present = d.present, a.scell = d.scell, a.obst_present = d.obst_present, a.dead = d.dead;
        a.dlog = d.dlog, a.dlog_n = d.dlog_n;
        a.atlas = render_default_atlas();
        std::vector<uint8_t> col((size_t)E);
        for (int s = 0; s < E; s++) col[s] = render_slot_col(s, d.A, d.P, h->cfg.bot_types);
        TRY(dupload(h, &a.slot_col, col));
        TRY(dalloc(h, &a.body_col, (size_t)a.plan.body_bytes * N));
        if (!h->d_ep_reset) TRY(dalloc(h, &h->d_ep_reset, N));
    }
    return ZS_OK;
}

// zs_create: the observation kernels of the handle (zs_obs_plan.hpp), their LDS limits raised
static int create_obs_plan(zs_handle* h, bool rank_order) {
    Dev& d = h->d;
    const ObsShape shape = {d.N, d.W, d.H, d.O, d.OW, d.DW, d.E, d.A, d.obs_scope, d.obs_enc, d.obs_w, d.obs_dtype,
                            d.reward_mode, d.opad_n, rank_order,
                            step_defer_respawn(d.minimum_zombies, d.nzs, d.W * d.H, h->ov)};
    auto lds_ok = [](int kind, int nobs, int patched, int bytes, void* dtype) {
        return obs_attr(*(const int*)dtype, kind, nobs, patched, bytes) == hipSuccess;
    };
    h->obs = obs_plan(shape, h->ov, lds_ok, &d.obs_dtype);
    if (h->obs.error) return fail(ZS_EINVAL, h->obs.error);
    d.obs_stat = h->obs.obs_stat;
    d.obsl = h->obs.step_img;
    d.fobs = h->obs.fobs;
    return ZS_OK;
}

// zs_create: the step plan (zs_step_plan.hpp) and what of it needs HIP: k_reset's LDS limit raised, the side
// stream of an unfused step's reset work
static int create_step_plan(zs_handle* h) {
    Dev& d = h->d;
    const StepShape shape = {d.N, d.W, d.H, d.E, d.A, d.DW, d.ncand, d.nps, d.nzs, d.minimum_zombies, h->cfg.lanes_per_env,
                             d.fobs ? d.obsl.bytes + 4 * d.obs_stat : 0};
    const StepPlan& p = h->step = step_plan(shape, h->ov);
    if (p.error) return fail(ZS_EINVAL, p.error);
    if (!tick_lst_is_behind_misc(tick_layout(64 / p.G, d.E, d.DW, p.rw_cap, p.cand_cap, p.lists_cap, d.A), d.A))
        return fail(ZS_ESTATE, "tick_layout(): the lst row is not behind the MISC rows (zs_tick.hpp LEADER_WORD)");
    d.rw_cap = p.rw_cap;
    d.rw_step = p.rw_step;
    d.cand_cap = p.cand_cap;
    d.lists_cap = p.lists_cap;
    d.rlists_cap = p.rlists_cap;
    d.defer_respawn = p.defer_respawn;
    if (p.reset_lds > 160 * 1024) return fail(ZS_EINVAL, "map too large for the reset kernel's LDS image");
    if (p.side_stream) {
        h->reset_side = hipStreamCreateWithFlags(&h->s_reset, hipStreamNonBlocking) == hipSuccess &&
                        hipEventCreateWithFlags(&h->ev_rfork, hipEventDisableTiming) == hipSuccess &&
                        hipEventCreateWithFlags(&h->ev_rjoin, hipEventDisableTiming) == hipSuccess;
    }
    if (p.reset_lds > 64 * 1024 && reset_lds_attr(p.reset_lds) != hipSuccess)
        return fail(ZS_EHIP, "cannot raise k_reset's dynamic LDS limit");
    return ZS_OK;
}

extern "C" int zs_create(const zs_config* cfg, int device, zs_handle** out) {
    if (!cfg || !out) return fail(ZS_EINVAL, "null argument");
    *out = nullptr;
    TRY(validate(cfg));
    if ((cfg->flags & ZS_FLAG_ENV_PARAMS) && (cfg->flags & ZS_FLAG_VIEWER))  // nothing resets or steps a viewer's envs
        return fail(ZS_ESTATE, "zs_create: ZS_FLAG_ENV_PARAMS: not on a viewer handle (ZS_FLAG_VIEWER)");
    if ((cfg->flags & ZS_FLAG_EPISODE_STATS) && (cfg->flags & ZS_FLAG_VIEWER))
        return fail(ZS_ESTATE, "zs_create: ZS_FLAG_EPISODE_STATS: not on a viewer handle (ZS_FLAG_VIEWER)");
    if (cfg->flags & ZS_FLAG_RENDER) {
        if (cfg->flags & ZS_FLAG_VIEWER) return fail(ZS_ESTATE, "zs_create: ZS_FLAG_RENDER: not on a viewer handle (ZS_FLAG_VIEWER)");
        if (!(cfg->flags & ZS_FLAG_DEATH_LOG))
            return fail(ZS_EINVAL, "zs_create: ZS_FLAG_RENDER needs ZS_FLAG_DEATH_LOG (the body colours come from the death log)");
        if (300L * cfg->map.width * cfg->map.height >= (1L << 31))
            return fail(ZS_EINVAL, "zs_create: ZS_FLAG_RENDER: a frame of this map would not be below 2 GiB");
    }
    HIPCHK(hipSetDevice(device));
    HandleOwner owner{new zs_handle()};
    zs_handle* h = owner.h;
    h->cfg = *cfg;
    memset(&h->ov, 0, sizeof(h->ov));
    if (cfg->launch) h->ov = *cfg->launch;
    h->cfg.launch = nullptr;
    h->device = device;
    h->snap_fp = snapshot_fingerprint(cfg);
    const zs_map_desc& m = cfg->map;
    Dev& d = h->d;
    memset(&d, 0, sizeof(d));
    d.N = cfg->num_envs;
    d.W = m.width;
    d.H = m.height;
    d.O = m.n_obstacles;
    d.A = cfg->num_agents;
    d.P = cfg->num_bots;
    d.Z = std::max(cfg->initial_zombies, cfg->minimum_zombies);
    d.E = d.A + d.P + d.Z;
    d.OW = (d.O + 31) / 32;
    d.DW = (d.W * d.H + 31) / 32;
    d.nps = m.n_player_spawns;
    d.nzs = m.n_zombie_spawns;
    d.nobj = m.n_objectives;
    d.ncand = std::max(d.nps ? d.nps : d.W * d.H, d.nzs ? d.nzs : d.W * d.H);
    d.rules = cfg->rules;
    d.reward_mode = cfg->reward_mode;
    d.obs_scope = cfg->obs_scope;
    d.obs_enc = cfg->obs_encoding;
    d.obs_w = cfg->obs_width;
    d.obs_dtype = cfg->obs_dtype;
    d.max_steps = cfg->max_episode_steps;
    d.initial_zombies = cfg->initial_zombies;
    d.minimum_zombies = cfg->minimum_zombies;
    d.flags = cfg->flags;
    // the shuffle and execution of a tick's actions by the env's lanes (zs_tick.hpp grp_execute) instead of
    // its leader lane alone; zs_launch.par_exec = -1 keeps the leader's serial loop (A/B, parity tests)
    d.par_exec = h->ov.par_exec >= 0;
    bool rank_order;
    TRY(create_static_tables(h, cfg, &rank_order));
    TRY(create_env_arrays(h, m));
    TRY(create_obs_plan(h, rank_order));
    TRY(create_step_plan(h));
    const size_t N = d.N;
    if (getenv("ZS_VERBOSE")) {
        const ObsKernel &kf = h->obs.full, &km = h->obs.masked;
        const StepPlan& p = h->step;
        fprintf(stderr, "zs_create: N=%d E=%d G=%d step_lds=%d resident=%d reset_lds=%d rw_cap=%d cand_cap=%d "
                        "lists_cap=%d fused=%d fobs=%d obs_img=%d obs=%s grid=%u block=%d lds=%d masked=%s block=%d lds=%d "
                        "reset_side=%d defer_respawn=%d\n",
                d.N, d.E, p.G, p.lds, p.resident, p.reset_lds, p.rw_cap, p.cand_cap, p.lists_cap, p.fused,
                d.fobs, d.obsl.bytes, obs_kernel_name(kf.kind), obs_grid(kf, d.N), kf.block, kf.lds,
                obs_kernel_name(km.kind), km.block, km.lds, h->reset_side, d.defer_respawn);
    }
    if (d.O > 0) HIPCHK(launch_init_obstacles(0, d));
    // every env starts "pending reset": the first zs_step (or zs_reset) builds its world
    HIPCHK(launch_init_pending(0, d, h->d_rlist[0], h->d_rcount));
    // both triples of every env start as the config's values
    if (d.flags & ZS_FLAG_ENV_PARAMS) HIPCHK(launch_env_params_init(0, d, h->d_envp_owner));
    // default seeds: env index (every env has a valid stream even if never seeded)
    std::vector<uint64_t> seeds(N);
    for (size_t i = 0; i < N; i++) seeds[i] = i;
    TRY(seed_envs(h, 0, (int)N, seeds.data(), nullptr));
    hipError_t se = hipDeviceSynchronize();
    if (se != hipSuccess) return fail(ZS_EHIP, std::string("zs_create sync: ") + hipGetErrorString(se));
    *out = h;
    owner.h = nullptr;
    return ZS_OK;
}

extern "C" int zs_obs_shape(const zs_handle* h, int32_t out[4]) {
    if (!h || !out) return fail(ZS_EINVAL, "null argument");
    const Dev& d = h->d;
    bool world = d.obs_scope == ZS_OBS_WORLD;
    out[0] = world ? 1 : (d.reward_mode == ZS_REWARD_MULTI ? d.A : 1);
    out[1] = d.obs_enc == ZS_ENC_CHANNELS ? 3 : 1;
    out[2] = world ? d.H : d.obs_w;
    out[3] = world ? d.W : d.obs_w;
    return ZS_OK;
}

extern "C" int zs_seed(zs_handle* h, int32_t env0, int32_t n, const uint64_t* seeds_host, void* stream) {
    if (!h || !seeds_host) return fail(ZS_EINVAL, "null argument");
    NOT_ON_VIEWER(h, "zs_seed");
    return seed_envs(h, env0, n, seeds_host, stream);
}

static int seed_envs(zs_handle* h, int32_t env0, int32_t n, const uint64_t* seeds_host, void* stream) {
    if (env0 < 0 || n < 0 || env0 + n > h->d.N) return fail(ZS_EINVAL, "env range out of bounds");
    if (n == 0) return ZS_OK;
    ENTER(h, stream, s);
    HIPCHK(hipMemcpyAsync(h->d_seedbuf, seeds_host, sizeof(uint64_t) * n, hipMemcpyHostToDevice, s));
    HIPCHK(launch_seed(s, h->d, env0, n, h->d_seedbuf));
    // the policy rows kept ahead were generated from the old seeds: no stamp, so the next policy step generates its own
    if (h->d_gstep) HIPCHK(hipMemsetAsync(h->d_gstep + GS_STAMP, 0, 2 * sizeof(uint64_t), s));
    HIPCHK(hipStreamSynchronize(s));  // seeds_host may be freed by the caller on return
    return ZS_OK;
}

// the step-kernel unit (k_tick_g.hip) of G lanes per env, by log2 G
struct TickUnit {
    decltype(&launch_tick_g1) launch;
    decltype(&stamps_g1) stamps;
};
static const TickUnit& tick_unit(int G) {
#define ZS_UNIT(g) {launch_tick_g##g, stamps_g##g}
    static const TickUnit units[7] = {ZS_UNIT(1), ZS_UNIT(2), ZS_UNIT(4), ZS_UNIT(8), ZS_UNIT(16), ZS_UNIT(32), ZS_UNIT(64)};
#undef ZS_UNIT
    return units[__builtin_ctz((unsigned)G)];
}

// The step's launches take the Dev they pass to the kernels: the handle's, or zs_step's copy of it with the policy
// and the tail set (Dev::pol_*, Dev::tail_*).
static int launch_obs(zs_handle* h, const Dev& d, void* obs, const uint8_t* mask, hipStream_t s, int env0 = 0, int env1 = -1) {
    if (!obs) return ZS_OK;
    if (env1 < 0) env1 = d.N;
    const ObsKernel& k = mask ? h->obs.masked : h->obs.full;
    const ObsLaunch o = {k, obs_grid(k, env1 - env0), obs, mask, env0, env1};
    return timed_launch(h, s, h->ev_obs, "observation launch", [&] { return obs_launch(d.obs_dtype, o, s, d); });
}

static int launch_tick(zs_handle* h, const Dev& d, const int32_t* actions, double* rew, uint8_t* done, uint8_t* trunc,
                       uint8_t* listed, uint8_t* reset_out, int* rlist, int* rcount, void* obs, hipStream_t s,
                       int env0 = 0, int env1 = -1) {
    const StepPlan& sp = h->step;
    const int ne = 64 / sp.G;
    if (env1 < 0) env1 = d.N;
    unsigned grid = (unsigned)((env1 - env0 + ne - 1) / ne);
    const int p = h->rpar;
    const TickArgs a = {actions, rew,  done, trunc,      listed,        reset_out,       rlist,   rcount,
                        obs,     env0, env1, sp.n_reset, h->d_rlist[p], h->d_rcount + p, h->d_err};
    return timed_launch(h, s, h->ev_tick, "step launch",
                        [&] { return tick_unit(sp.G).launch(sp.fused, sp.tick_waves, grid, (size_t)sp.lds, s, d, a); });
}

static int launch_reset(zs_handle* h, const Dev& d, int list_mode, const uint8_t* mask, void* obs, hipStream_t s) {
    const unsigned grid = (unsigned)(list_mode ? h->step.reset_grid_list : h->step.reset_grid_mask);
    const int p = h->rpar;
    return timed_launch(h, s, h->ev_reset, "k_reset", [&] {
        return launch_reset_k(grid, (size_t)h->step.reset_lds, s, d, list_mode, h->d_rlist[p], h->d_rcount + p, mask, h->d_err, obs);
    });
}

// the respawns the tick just deferred (k_respawn drains d.resp_list; count zeroed before the tick)
static int launch_respawn(zs_handle* h, const Dev& d, hipStream_t s) {
    return timed_launch(h, s, h->ev_respawn, "k_respawn",
                        [&] { return launch_respawn_k((unsigned)h->step.respawn_grid, (size_t)h->step.reset_lds, s, d); });
}

// zs_reset's launches, queued on s (the caller synchronises and reads h->d_err)
static int queue_reset(zs_handle* h, const uint8_t* env_mask_dev, void* obs_dev, hipStream_t s) {
    HIPCHK(hipMemsetAsync(h->d_err, 0, sizeof(int), s));
    TRY(launch_reset(h, h->d, 0, env_mask_dev, nullptr, s));
    // the pending-reset list must hold exactly the envs still pending: drop the ones just rebuilt
    {
        int p = h->rpar, q = 1 - p;
        if (!env_mask_dev) {
            HIPCHK(hipMemsetAsync(h->d_rcount + p, 0, sizeof(int), s));
        } else {
            HIPCHK(hipMemsetAsync(h->d_rcount + q, 0, sizeof(int), s));
            HIPCHK(launch_list_filter((unsigned)std::min(64, (h->d.N + 255) / 256), s, (const int*)h->d_rlist[p],
                                      (const int*)(h->d_rcount + p), h->d_rlist[q], h->d_rcount + q, env_mask_dev,
                                      h->d.N));
            // the list the next step appends to (list[p] now) starts empty (zs_step's counter protocol)
            HIPCHK(hipMemsetAsync(h->d_rcount + p, 0, sizeof(int), s));
            h->rpar = q;
        }
    }
    // ZS_FLAG_EPISODE_STATS: the reset envs' running return starts over; an abandoned episode is not counted
    if (h->ep.run) HIPCHK(launch_episode_clear(s, h->ep, env_mask_dev, 1));
    // ZS_FLAG_RENDER: the reset envs' worlds have no bodies
    if (h->rn.body_col) HIPCHK(launch_render_track(s, h->rn, env_mask_dev, 1));
    return launch_obs(h, h->d, obs_dev, env_mask_dev, s);
}

extern "C" int zs_reset(zs_handle* h, const uint8_t* env_mask_dev, void* obs_dev, void* stream) {
    if (!h) return fail(ZS_EINVAL, "null handle");
    NOT_ON_VIEWER(h, "zs_reset");
    ENTER(h, stream, s);
    TRY(queue_reset(h, env_mask_dev, obs_dev, s));
    int err;
    TRY(read_error_word(h, s, &err));
    return reset_result(err);
}

// Observation only (the reference's env.get_observation(), gym_env.py:93-94): re-encode the
// current state of the masked envs, e.g. after a zs_set_state poke.
extern "C" int zs_observe(zs_handle* h, const uint8_t* env_mask_dev, void* obs_dev, void* stream) {
    if (!h || !obs_dev) return fail(ZS_EINVAL, "null argument");
    ENTER(h, stream, s);
    return launch_obs(h, h->d, obs_dev, env_mask_dev, s);
}

extern "C" int zs_step(zs_handle* h, const int32_t* actions_dev, void* obs_dev, double* rewards_dev, uint8_t* done_dev,
                       uint8_t* trunc_dev, uint8_t* listed_dev, uint8_t* reset_dev, void* stream) {
    if (!h || !actions_dev || !rewards_dev || !done_dev || !trunc_dev) return fail(ZS_EINVAL, "null argument");
    NOT_ON_VIEWER(h, "zs_step");
    ENTER(h, stream, s);
    // ZS_FLAG_EPISODE_STATS: the update rule reads the tick's reset flags, so a caller that wants none gets the
    // handle's own row (one row whatever the caller's buffers: the step graphs stay keyed on the caller's pointers)
    if ((h->ep.run || h->rn.body_col) && !reset_dev) reset_dev = h->d_ep_reset;
    // 0) bound entity-action ids (zs_entity_act_bind): decoded against the world the last observation showed into the
    //    rows the tick reads, on the caller's stream ahead of the fork, so the side-stream reset work is ordered after it
    if (h->eact_ids)
        LAUNCHCHK("k_entity_act_decode",
                  launch_entity_act_decode(s, h->d, h->eact_kz, h->eact_kp, nullptr, h->eact_ids, const_cast<int32_t*>(actions_dev)));
    // 1) rebuild the envs that ended at the previous call (list[p]); fused into the tick launch
    //    when the LDS images allow, else a k_reset launch first
    int q = 1 - h->rpar, rc = ZS_OK;
    bool side = false, ahead = false;
    if (!h->step.fused) {
        side = h->reset_side != 0;
        hipStream_t rs = s;
        if (side) {  // fork: the reset work sees everything the caller queued before this call
            HIPCHK(hipEventRecord(h->ev_rfork, s));
            HIPCHK(hipStreamWaitEvent(h->s_reset, h->ev_rfork, 0));
            rs = h->s_reset;
        }
        // zs_step_graph's policy: with the reset work beside the tick, its own launch on the caller's
        // stream right after the fork and ahead of the reset launch (captured in that order, the graph
        // starts the policy first: C3 173 M env-steps/s, against 167 with the reset launch captured first
        // and 169 with the policy inside the step launch); otherwise inside the step launch (no launch,
        // no gap: 8 192 envs 110 -> 117 M env-steps/s).
        // Where the step ends in an encoder / writer observation kernel (k_obs_ring, k_obs_pbring), that launch
        // generated this step's triples a step early into the handle's rows, under its store stream, and leaves the
        // next step's (Dev::pol_ahead): no policy launch, the tick copies the rows out (or generates them itself
        // when the stamp does not name this step: the first replay, after zs_seed, another n_discrete)
        ahead = h->graph_pol && side && obs_dev && !h->d.fobs &&
                (h->obs.full.kind == OBSK_RING || h->obs.full.kind == OBSK_BRING);
        if (h->graph_pol && side && !ahead)
            HIPCHK(launch_gen_actions_ctr(s, h->d, (const uint64_t*)h->d_gstep, h->graph_pol, (int32_t*)actions_dev));
        // ... and then the tick is captured ahead of the reset launch (below): the graph starts its nodes in the
        // order of capture, several us apart, and the tick is the longer of the two
        if (!ahead) {
            TRY(launch_reset(h, h->d, 1, nullptr, h->d.fobs ? obs_dev : nullptr, rs));
            if (side) HIPCHK(hipEventRecord(h->ev_rjoin, h->s_reset));
        }
    }
    // this step's Dev: the handle's (whose pol_* and tail_* stay null) with the policy the step launch generates
    // itself, then (below) with the tail the step's last launch carries
    Dev d = h->d;
    d.pol_n = side && !ahead ? 0 : h->graph_pol;
    d.pol_step = side && !ahead ? nullptr : h->d_gstep;
    d.pol_ahead = ahead ? h->d_ahead : nullptr;
    if (h->graph_pol) h->step_policy = ahead ? "ahead" : side ? "k_gen_actions_ctr" : "step launch";
    // 2) tick every other env; envs that end now are queued on list[q] for the next call.
    // Work-list counters: between calls the list the next step appends to (list[1 - rpar]) and the
    // deferred-respawn list are empty.  This step appends to list[q] and resp_list, drains list[p] and
    // resp_list, and its last launch (the observation kernel, else k_tail) empties list[p] and resp_list
    // again (Dev::tail_*), so no launch ahead of the tick is needed.  (Not by captured 4-byte
    // hipMemsetAsync nodes: in this engine's round-2 city128 graph such nodes left byte patterns in the
    // counters, profiles/r02_graph_memset_city128.log; tools/probe/graphprobe.hip replays that node
    // sequence standalone without a fault, profiles/r03_graphprobe_fork.log.)  Every list index is
    // bounds-checked in the kernels.
    const int p = h->rpar;
    TRY(launch_tick(h, d, actions_dev, rewards_dev, done_dev, trunc_dev, listed_dev, reset_dev, h->d_rlist[q],
                    h->d_rcount + q, obs_dev, s));
    if (ahead) {  // the side stream's reset work, forked above (it drains list[p]: before the parity flips)
        TRY(launch_reset(h, h->d, 1, nullptr, nullptr, h->s_reset));
        HIPCHK(hipEventRecord(h->ev_rjoin, h->s_reset));
    }
    h->rpar = q;
    // a launch failing after the tick was queued: the step's tail (the counter protocol above) is done
    // here instead, so the next step does not append after stale counts (not while capturing: a failed
    // capture is discarded, and nothing of it ran)
    auto tail_on_error = [&](int code) {
        hipStreamCaptureStatus cs = hipStreamCaptureStatusNone;
        if (hipStreamIsCapturing(s, &cs) == hipSuccess && cs == hipStreamCaptureStatusNone) {
            (void)hipMemsetAsync(h->d_rcount + p, 0, sizeof(int), s);
            if (h->d.defer_respawn) (void)hipMemsetAsync(h->d.resp_count, 0, sizeof(int), s);
        }
        return code;
    };
    if (h->d.defer_respawn) {
        rc = launch_respawn(h, d, s);
        if (rc) return tail_on_error(rc);
    }
    // join the reset work, then 3) observations of every env (already written by the step launch
    // when fobs), carrying the step's tail
    if (side && hipStreamWaitEvent(s, h->ev_rjoin, 0) != hipSuccess) return tail_on_error(fail(ZS_EHIP, "hipStreamWaitEvent"));
    d.tail_cnt0 = h->d_rcount + p;
    d.tail_cnt1 = d.defer_respawn ? d.resp_count : nullptr;
    d.tail_step = h->graph_pol ? h->d_gstep : nullptr;
    if (d.fobs || !obs_dev) {
        rc = launched("k_tail", launch_tail(s, d));
        if (rc) return tail_on_error(rc);
        h->step_last = "k_tail";
    } else {
        rc = launch_obs(h, d, obs_dev, nullptr, s);
        if (rc) return tail_on_error(rc);
        h->step_last = obs_kernel_name(h->obs.full.kind);
    }
    // 4) a bound mask buffer (zs_action_mask_bind): the masks of the world the observations show, respawned
    //    zombies and reset envs included (the step's tail is done: nothing to undo when this launch fails)
    if (h->mask_bound) LAUNCHCHK("k_action_mask", launch_action_mask(s, d, nullptr, h->mask_bound));
    //    ... and a bound entity-observation buffer (zs_entity_obs_bind), of the same world
    if (h->ent_bound) {
        const EntityArgs g = {h->ent_kz, h->ent_kp, d.nobj, h->d_obj_xy};
        LAUNCHCHK("k_entity_obs", launch_entity_obs(s, d, g, nullptr, h->ent_bound));
    }
    //    ... and a bound entity-action mask buffer (zs_entity_act_bind), of the same world
    if (h->eact_mask) LAUNCHCHK("k_entity_act_mask", launch_entity_act_mask(s, d, h->eact_kz, h->eact_kp, nullptr, h->eact_mask));
    //    ... and a bound path-distance buffer (zs_nav_bind), of the same world
    if (h->nav_bound) {
        const NavArgs g = {h->nav_fields, h->nav_max_dist, d.nobj, h->d_obj_xy, h->nav};
        LAUNCHCHK("k_nav", launch_nav(s, d, g, nullptr, h->nav_bound));
    }
    //    ... and a bound autopilot (zs_autopilot_bind): the scripted triples of that world.  Bound to the caller's action
    //    buffer this is the closed loop: the rows the next step's tick reads
    if (h->pilot_out) LAUNCHCHK("k_autopilot", launch_autopilot(s, d, nullptr, h->pilot_policy, h->pilot_out));
    // 5) ZS_FLAG_EPISODE_STATS: the step's rewards and flags into the running returns, a finished episode latched
    //    and counted (the terminal world stays until the next call's reset work)
    if (h->ep.run) LAUNCHCHK("k_episode_stats", launch_episode_stats(s, h->ep, rewards_dev, done_dev, trunc_dev, reset_dev));
    // 6) ZS_FLAG_RENDER: the step's death log into the body colours; a reset env's row cleared
    if (h->rn.body_col) LAUNCHCHK("k_render_track", launch_render_track(s, h->rn, reset_dev, 0));
    return ZS_OK;
}

// the cached step graphs hold the old launch sequence (a rare call: wait for the ones in flight first)
static int drop_step_graphs(zs_handle* h) {
    HIPCHK(hipSetDevice(h->device));
    HIPCHK(hipDeviceSynchronize());
    for (auto& gs : h->gsets) {
        HIPCHK(destroy_graphs(gs));
        gs.used = 0;
    }
    return ZS_OK;
}

static int mask_buffer_ok(const void* mask_dev) {
    if (((uintptr_t)mask_dev & 7u) != 0) return fail(ZS_EINVAL, "the action-mask buffer must be 8-byte aligned");
    return ZS_OK;
}

// Action masks of the current state (zs_mask.hpp), uint8 [N][A][8].  Viewer handles included: the kernel reads
// what zs_obs_state_unpack fills (pos, present, weapon, obstacle presence) and the static cell map.
extern "C" int zs_action_mask(zs_handle* h, const uint8_t* env_mask_dev, void* mask_dev, void* stream) {
    if (!h || !mask_dev) return fail(ZS_EINVAL, "null argument");
    TRY(mask_buffer_ok(mask_dev));
    ENTER(h, stream, s);
    HIPCHK(launch_action_mask(s, h->d, env_mask_dev, mask_dev));
    return ZS_OK;
}

extern "C" int zs_action_mask_bind(zs_handle* h, void* mask_dev_or_null) {
    if (!h) return fail(ZS_EINVAL, "null handle");
    NOT_ON_VIEWER(h, "zs_action_mask_bind");
    TRY(mask_buffer_ok(mask_dev_or_null));
    if (mask_dev_or_null == h->mask_bound) return ZS_OK;
    TRY(drop_step_graphs(h));
    h->mask_bound = mask_dev_or_null;
    return ZS_OK;
}

static int entity_args_ok(const void* out_dev, int kz, int kp) {
    if (!ent_k_ok(kz, kp)) return fail(ZS_EINVAL, "entity observation: kz must be in 1..16 and kp in 0..16");
    if (((uintptr_t)out_dev & 7u) != 0) return fail(ZS_EINVAL, "the entity-observation buffer must be 8-byte aligned");
    return ZS_OK;
}

extern "C" int zs_entity_obs_layout(const zs_handle* h, int32_t kz, int32_t kp, int32_t out[8]) {
    if (!h || !out) return fail(ZS_EINVAL, "null argument");
    TRY(entity_args_ok(nullptr, kz, kp));
    const EntLayout L = ent_layout(kz, kp);
    const int32_t v[8] = {L.row_words, L.self, L.zombies, L.players, L.objective, L.rays, ZS_ENT_RAY_CAP, 2 * L.row_words};
    std::memcpy(out, v, sizeof(v));
    return ZS_OK;
}

// Entity observations of the current state (zs_entity_obs.hpp), int16 [N][A][ROW].  Viewer handles included: the
// kernel reads what zs_obs_state_unpack fills and the static tables.
extern "C" int zs_entity_obs(zs_handle* h, const uint8_t* env_mask_dev, int32_t kz, int32_t kp, void* out_dev, void* stream) {
    if (!h || !out_dev) return fail(ZS_EINVAL, "null argument");
    TRY(entity_args_ok(out_dev, kz, kp));
    ENTER(h, stream, s);
    const EntityArgs g = {kz, kp, h->d.nobj, h->d_obj_xy};
    HIPCHK(launch_entity_obs(s, h->d, g, env_mask_dev, out_dev));
    return ZS_OK;
}

extern "C" int zs_entity_obs_bind(zs_handle* h, void* out_dev_or_null, int32_t kz, int32_t kp) {
    if (!h) return fail(ZS_EINVAL, "null handle");
    NOT_ON_VIEWER(h, "zs_entity_obs_bind");
    if (out_dev_or_null) {
        TRY(entity_args_ok(out_dev_or_null, kz, kp));
    } else {
        kz = kp = 0;
    }
    if (out_dev_or_null == h->ent_bound && kz == h->ent_kz && kp == h->ent_kp) return ZS_OK;
    TRY(drop_step_graphs(h));
    h->ent_bound = out_dev_or_null;
    h->ent_kz = kz;
    h->ent_kp = kp;
    return ZS_OK;
}

static int eact_k_ok(int kz, int kp) {
    if (!ent_k_ok(kz, kp)) return fail(ZS_EINVAL, "entity actions: kz must be in 1..16 and kp in 0..16");
    return ZS_OK;
}
static int eact_mask_ok(const void* mask_dev) {
    if (((uintptr_t)mask_dev & 7u) != 0) return fail(ZS_EINVAL, "the entity-action mask buffer must be 8-byte aligned");
    return ZS_OK;
}
static int eact_ids_ok(const void* p) {
    if (((uintptr_t)p & 3u) != 0) return fail(ZS_EINVAL, "entity-action ids and triples must be 4-byte aligned");
    return ZS_OK;
}

extern "C" int zs_entity_act_table(const zs_handle* h, int32_t kz, int32_t kp, int32_t out[8]) {
    if (!h || !out) return fail(ZS_EINVAL, "null argument");
    TRY(eact_k_ok(kz, kp));
    const int32_t v[8] = {eact_nid(kz, kp), eact_row_bytes(kz, kp), ZS_EACT_ATTACK_DIR, ZS_EACT_HEAL_DIR, eact_zombie_id(0),
                          eact_player_id(kz, 0), eact_nid(kz, kp), 0};
    std::memcpy(out, v, sizeof(v));
    return ZS_OK;
}

// The entity action table on the current state (zs_entity_act.hpp).  Viewer handles included: the kernels read what
// zs_obs_state_unpack fills (pos, present, weapon, obstacle presence) and the static cell map.
extern "C" int zs_entity_act_decode(zs_handle* h, const uint8_t* env_mask_dev, int32_t kz, int32_t kp, const int32_t* ids_dev,
                                    int32_t* actions_dev, void* stream) {
    if (!h || !ids_dev || !actions_dev) return fail(ZS_EINVAL, "null argument");
    TRY(eact_k_ok(kz, kp));
    TRY(eact_ids_ok(ids_dev));
    TRY(eact_ids_ok(actions_dev));
    ENTER(h, stream, s);
    LAUNCHCHK("k_entity_act_decode", launch_entity_act_decode(s, h->d, kz, kp, env_mask_dev, ids_dev, actions_dev));
    return ZS_OK;
}

extern "C" int zs_entity_act_mask(zs_handle* h, const uint8_t* env_mask_dev, int32_t kz, int32_t kp, void* mask_dev, void* stream) {
    if (!h || !mask_dev) return fail(ZS_EINVAL, "null argument");
    TRY(eact_k_ok(kz, kp));
    TRY(eact_mask_ok(mask_dev));
    ENTER(h, stream, s);
    LAUNCHCHK("k_entity_act_mask", launch_entity_act_mask(s, h->d, kz, kp, env_mask_dev, mask_dev));
    return ZS_OK;
}

extern "C" int zs_entity_act_encode(zs_handle* h, const uint8_t* env_mask_dev, int32_t kz, int32_t kp, const int32_t* triples_dev,
                                    int32_t* ids_out_dev, void* stream) {
    if (!h || !triples_dev || !ids_out_dev) return fail(ZS_EINVAL, "null argument");
    TRY(eact_k_ok(kz, kp));
    TRY(eact_ids_ok(triples_dev));
    TRY(eact_ids_ok(ids_out_dev));
    ENTER(h, stream, s);
    LAUNCHCHK("k_entity_act_encode", launch_entity_act_encode(s, h->d, kz, kp, env_mask_dev, triples_dev, ids_out_dev));
    return ZS_OK;
}

extern "C" int zs_entity_act_bind(zs_handle* h, const int32_t* ids_dev_or_null, void* mask_dev_or_null, int32_t kz, int32_t kp) {
    if (!h) return fail(ZS_EINVAL, "null handle");
    NOT_ON_VIEWER(h, "zs_entity_act_bind");
    if (ids_dev_or_null || mask_dev_or_null) {
        TRY(eact_k_ok(kz, kp));
        TRY(eact_ids_ok(ids_dev_or_null));
        TRY(eact_mask_ok(mask_dev_or_null));
    } else {
        kz = kp = 0;
    }
    if (ids_dev_or_null == h->eact_ids && mask_dev_or_null == h->eact_mask && kz == h->eact_kz && kp == h->eact_kp) return ZS_OK;
    // the cached step graphs hold the old launch sequence: the next zs_step_graph(_n) drops them behind its stream
    // (no wait here: an eager step in flight has read its binding when it was queued)
    h->graphs_stale = true;
    h->eact_ids = ids_dev_or_null;
    h->eact_mask = mask_dev_or_null;
    h->eact_kz = kz;
    h->eact_kp = kp;
    return ZS_OK;
}

// the arguments every path-distance call checks before it launches: the fields (rows: a mask; a frame: one bit), the
// cap, the buffer's alignment, and the plan of the handle's map
static int nav_args_ok(const zs_handle* h, const void* out_dev, int fields, bool one_field, int max_dist, unsigned align) {
    if (one_field ? !nav_field_ok(fields) : !nav_fields_ok(fields))
        return fail(ZS_EINVAL, one_field ? "path distances: field must be ZS_NAV_OBJECTIVE or ZS_NAV_ZOMBIES"
                                         : "path distances: fields must be a non-empty mask of ZS_NAV_OBJECTIVE | ZS_NAV_ZOMBIES");
    if (!nav_max_dist_ok(max_dist)) return fail(ZS_EINVAL, "path distances: max_dist must be in 1..32766");
    if (((uintptr_t)out_dev & (align - 1)) != 0)
        return fail(ZS_EINVAL, "the path-distance buffer must be " + std::to_string(align) + "-byte aligned");
    if (!h->nav.ok)
        return fail(ZS_EINVAL, "path distances: one env's search image (28 * H * ceil(W / 32) + 40 * agents bytes) is past the " +
                                   std::to_string(ZS_NAV_LDS_LIMIT) + "-byte LDS limit of a workgroup");
    return ZS_OK;
}

extern "C" int zs_nav_plan(const zs_handle* h, int32_t fields, int32_t out[8]) {
    if (!h || !out) return fail(ZS_EINVAL, "null argument");
    if (!nav_fields_ok(fields))
        return fail(ZS_EINVAL, "path distances: fields must be a non-empty mask of ZS_NAV_OBJECTIVE | ZS_NAV_ZOMBIES");
    const int F = nav_nfields(fields);
    const NavPlan& p = h->nav;
    const int64_t bytes = nav_env_bytes(h->d.W, h->d.H, h->d.A);
    const int32_t v[8] = {F, ZS_NAV_ROW_WORDS, 0, F == 2 ? ZS_NAV_ROW_WORDS : -1, p.envs_per_wg, p.block, p.lds_bytes,
                          (int32_t)std::min<int64_t>(bytes, 0x7fffffff)};
    std::memcpy(out, v, sizeof(v));
    return ZS_OK;
}

// Path-distance rows of the current state (zs_nav.hpp), int16 [N][A][F][8].  Viewer handles included: the kernel reads
// what zs_obs_state_unpack fills (pos, present, obstacle presence) and the static tables.
extern "C" int zs_nav_obs(zs_handle* h, const uint8_t* env_mask_dev, int32_t fields, int32_t max_dist, void* out_dev, void* stream) {
    if (!h || !out_dev) return fail(ZS_EINVAL, "null argument");
    TRY(nav_args_ok(h, out_dev, fields, false, max_dist, 8));
    ENTER(h, stream, s);
    const NavArgs g = {fields, max_dist, h->d.nobj, h->d_obj_xy, h->nav};
    LAUNCHCHK("k_nav", launch_nav(s, h->d, g, env_mask_dev, out_dev));
    return ZS_OK;
}

// The full field of a list of envs, uint16 [n][H][W] (index handling as zs_render's)
extern "C" int zs_nav_field(zs_handle* h, const int32_t* env_idx_dev, int32_t n, int32_t field, int32_t max_dist, void* out_dev,
                            void* stream) {
    if (!h || !out_dev) return fail(ZS_EINVAL, "null argument");
    if (n < 0) return fail(ZS_EINVAL, "path distances: n must be >= 0");
    TRY(nav_args_ok(h, out_dev, field, true, max_dist, 2));
    ENTER(h, stream, s);
    const NavArgs g = {field, max_dist, h->d.nobj, h->d_obj_xy, h->nav};
    LAUNCHCHK("k_nav", launch_nav_field(s, h->d, g, env_idx_dev, n, out_dev));
    return ZS_OK;
}

extern "C" int zs_nav_bind(zs_handle* h, void* out_dev_or_null, int32_t fields, int32_t max_dist) {
    if (!h) return fail(ZS_EINVAL, "null handle");
    NOT_ON_VIEWER(h, "zs_nav_bind");
    if (out_dev_or_null) {
        TRY(nav_args_ok(h, out_dev_or_null, fields, false, max_dist, 8));
    } else {
        fields = max_dist = 0;
    }
    if (out_dev_or_null == h->nav_bound && fields == h->nav_fields && max_dist == h->nav_max_dist) return ZS_OK;
    TRY(drop_step_graphs(h));
    h->nav_bound = out_dev_or_null;
    h->nav_fields = fields;
    h->nav_max_dist = max_dist;
    return ZS_OK;
}

static int pilot_args_ok(const void* policy_dev, const void* out_dev) {
    if (!policy_dev || !out_dev) return fail(ZS_EINVAL, "null argument");
    if (((uintptr_t)out_dev & 3u) != 0) return fail(ZS_EINVAL, "the autopilot's triples must be 4-byte aligned");
    return ZS_OK;
}

// Scripted triples of the current state (zs_autopilot.hpp), int32 [N][A][3] under the policy codes uint8 [N][A].  Not on
// a viewer handle: the observation-state record carries no order row, which the closest zombie's tie-break reads.
extern "C" int zs_autopilot(zs_handle* h, const uint8_t* env_mask_dev, const uint8_t* policy_dev, int32_t* out_dev, void* stream) {
    if (!h) return fail(ZS_EINVAL, "null handle");
    TRY(pilot_args_ok(policy_dev, out_dev));
    NOT_ON_VIEWER(h, "zs_autopilot");
    ENTER(h, stream, s);
    HIPCHK(launch_autopilot(s, h->d, env_mask_dev, policy_dev, out_dev));
    return ZS_OK;
}

extern "C" int zs_autopilot_bind(zs_handle* h, const uint8_t* policy_dev_or_null, int32_t* out_dev_or_null) {
    if (!h) return fail(ZS_EINVAL, "null handle");
    NOT_ON_VIEWER(h, "zs_autopilot_bind");
    if (policy_dev_or_null || out_dev_or_null) {  // both, or neither (unbind)
        TRY(pilot_args_ok(policy_dev_or_null, out_dev_or_null));
    }
    if (policy_dev_or_null == h->pilot_policy && out_dev_or_null == h->pilot_out) return ZS_OK;
    TRY(drop_step_graphs(h));
    h->pilot_policy = policy_dev_or_null;
    h->pilot_out = out_dev_or_null;
    return ZS_OK;
}

extern "C" int zs_gen_actions(zs_handle* h, uint64_t step, int32_t n_discrete, int32_t* actions_dev, void* stream) {
    if (!h || !actions_dev) return fail(ZS_EINVAL, "null argument");
    NOT_ON_VIEWER(h, "zs_gen_actions");
    if (n_discrete < 1 || n_discrete > 7) return fail(ZS_EINVAL, "n_discrete must be in 1..7");
    ENTER(h, stream, s);
    HIPCHK(launch_gen_actions(s, h->d, step, n_discrete, actions_dev));
    return ZS_OK;
}

// One step of the on-device policy loop (zs_gen_actions for the next step number, then zs_step) as a
// replayed hipGraph: the launches of a step are captured once per pending-list parity and then
// cost one graph launch per step instead of one dispatch each.  step0 is the step number of the
// first call after (re)capture; later calls continue from the device counter.
extern "C" int zs_step_graph(zs_handle* h, uint64_t step0, int32_t n_discrete, int32_t* actions_dev, void* obs_dev,
                             double* rewards_dev, uint8_t* done_dev, uint8_t* trunc_dev, uint8_t* listed_dev,
                             uint8_t* reset_dev, void* stream) {
    return zs_step_graph_n(h, step0, n_discrete, 1, actions_dev, obs_dev, rewards_dev, done_dev, trunc_dev, listed_dev,
                           reset_dev, stream);
}

extern "C" int zs_step_graph_n(zs_handle* h, uint64_t step0, int32_t n_discrete, int32_t n_steps, int32_t* actions_dev,
                               void* obs_dev, double* rewards_dev, uint8_t* done_dev, uint8_t* trunc_dev,
                               uint8_t* listed_dev, uint8_t* reset_dev, void* stream) {
    if (!h || !actions_dev || !rewards_dev || !done_dev || !trunc_dev) return fail(ZS_EINVAL, "null argument");
    NOT_ON_VIEWER(h, "zs_step_graph");
    // n_discrete = 0: the caller's actions (no policy launch; the graph replays zs_step on actions_dev)
    if (n_discrete < 0 || n_discrete > 7) return fail(ZS_EINVAL, "n_discrete must be in 0..7");
    if (n_steps < 1 || n_steps > 64) return fail(ZS_EINVAL, "n_steps must be in 1..64");
    if (n_discrete != 0 && h->eact_ids)
        return fail(ZS_EINVAL, "zs_step_graph: n_discrete must be 0 while entity-action ids are bound (the generated policy "
                               "would overwrite the decoded rows)");
    ENTER(h, stream, s);
    if (h->graphs_stale) {  // a binding changed since the sets were captured: wait for the replays queued on s, drop them
        HIPCHK(hipStreamSynchronize(s));
        for (auto& gs : h->gsets) {
            HIPCHK(destroy_graphs(gs));
            gs.used = 0;
        }
        h->graphs_stale = false;
    }
    const void* key[9] = {actions_dev, obs_dev, rewards_dev, done_dev, trunc_dev, listed_dev, reset_dev,
                          (const void*)(intptr_t)n_discrete, (const void*)(intptr_t)n_steps};
    zs_handle::GraphSet* set = nullptr;
    for (auto& gs : h->gsets) {
        bool same = gs.g[0] && gs.g[1];
        for (int k = 0; k < 9 && same; k++) same = key[k] == gs.key[k];
        if (same) set = &gs;
    }
    if (!set) {  // capture into the least recently used set
        set = &h->gsets[0];
        for (auto& gs : h->gsets)
            if (gs.used < set->used) set = &gs;
        HIPCHK(destroy_graphs(*set));
        if (!h->d_gstep) {
            TRY(dalloc(h, &h->d_gstep, GS_WORDS));
            TRY(dalloc(h, &h->d_ahead, (size_t)h->d.N * h->d.A * 3));
        }
        // the policy step counter is the policy graphs' alone: a set without a policy (n_discrete = 0) neither reads
        // nor advances it, so capturing one in mid-run leaves it where the policy graphs continue from.  The stamp of
        // the rows kept ahead stays: it names the step and n_discrete they were generated for, whatever step0 is
        if (n_discrete > 0) HIPCHK(hipMemcpyAsync(h->d_gstep + GS_STEP, &step0, sizeof(step0), hipMemcpyHostToDevice, s));
        HIPCHK(hipStreamSynchronize(s));
        hipStream_t cs;
        HIPCHK(hipStreamCreateWithFlags(&cs, hipStreamNonBlocking));
        const int prof = h->prof;
        h->prof = 0;  // no timing events inside a graph
        const int p0 = h->rpar;
        int rc = ZS_OK;
        for (int g = 0; g < 2 && rc == ZS_OK; g++) {  // starting parity p0, then 1 - p0 (zs_step flips rpar)
            hipGraph_t graph = nullptr;
            h->rpar = (p0 + g) & 1;
            if (hipStreamBeginCapture(cs, hipStreamCaptureModeThreadLocal) != hipSuccess) {
                rc = fail(ZS_EHIP, "hipStreamBeginCapture failed");
                break;
            }
            // each step's policy reads the step number *d_gstep (zs_step: its own launch, or inside the
            // step launch), the step's tail advances it
            h->graph_pol = n_discrete;
            for (int k = 0; k < n_steps && rc == ZS_OK; k++)
                rc = zs_step(h, actions_dev, obs_dev, rewards_dev, done_dev, trunc_dev, listed_dev, reset_dev, cs);
            h->graph_pol = 0;
            hipError_t ce = hipStreamEndCapture(cs, &graph);
            if (rc == ZS_OK && ce != hipSuccess) rc = fail(ZS_EHIP, std::string("hipStreamEndCapture: ") + hipGetErrorString(ce));
            if (rc == ZS_OK) {
                hipError_t ie = hipGraphInstantiate(&set->g[(p0 + g) & 1], graph, nullptr, nullptr, 0);
                if (ie != hipSuccess) rc = fail(ZS_EHIP, std::string("hipGraphInstantiate: ") + hipGetErrorString(ie));
            }
            if (graph) (void)hipGraphDestroy(graph);
        }
        h->rpar = p0;  // a capture runs no work: the lists are where they were
        h->prof = prof;
        (void)hipStreamDestroy(cs);
        if (rc != ZS_OK) {
            (void)destroy_graphs(*set);
            return rc;
        }
        for (int k = 0; k < 9; k++) set->key[k] = key[k];
    }
    set->used = ++h->gclock;
    // g[p] starts by draining list p (the parity of its first step); each step flips the parity
    HIPCHK(hipGraphLaunch(set->g[h->rpar], s));
    h->rpar ^= n_steps & 1;
    return ZS_OK;
}

extern "C" int zs_state_size(const zs_handle* h, int32_t* n_words) {
    if (!h || !n_words) return fail(ZS_EINVAL, "null argument");
    *n_words = h->state_words;
    return ZS_OK;
}

extern "C" int zs_get_state(zs_handle* h, int32_t env, int32_t* buf_host, void* stream) {
    if (!h || !buf_host) return fail(ZS_EINVAL, "null argument");
    if (env < 0 || env >= h->d.N) return fail(ZS_EINVAL, "env index out of range");
    ENTER(h, stream, s);
    HIPCHK(launch_get_state(s, h->d, env, h->d_state));
    HIPCHK(hipMemcpyAsync(buf_host, h->d_state, sizeof(int32_t) * h->state_words, hipMemcpyDeviceToHost, s));
    HIPCHK(hipStreamSynchronize(s));
    return ZS_OK;
}

extern "C" int zs_set_state(zs_handle* h, int32_t env, const int32_t* buf_host, void* stream) {
    if (!h || !buf_host) return fail(ZS_EINVAL, "null argument");
    NOT_ON_VIEWER(h, "zs_set_state");
    if (env < 0 || env >= h->d.N) return fail(ZS_EINVAL, "env index out of range");
    {  // a present thing stands on a map cell (the occupancy and observation kernels index the map by it)
        const int32_t* r = buf_host + ZS_STATE_HEADER;
        for (int s = 0; s < h->d.E; s++, r += ZS_STATE_ENTITY_WORDS)
            if (r[1] && (r[2] < 0 || r[3] < 0 || r[2] >= h->d.W || r[3] >= h->d.H))
                return fail(ZS_EINVAL, "a present entity's position is outside the map");
    }
    {  // obstacle life is int32 in HBM; INT32_MIN is the observation kernels' absent mark (ZS_HP_FLOOR)
        const int32_t* hp = buf_host + ZS_STATE_HEADER + ZS_STATE_ENTITY_WORDS * h->d.E + h->d.E;
        for (int o = 0; o < h->d.O; o++)
            if (hp[o] < ZS_HP_FLOOR) return fail(ZS_EINVAL, "obstacle life below -2147483647");
    }
    ENTER(h, stream, s);
    HIPCHK(hipMemsetAsync(h->d_err, 0, sizeof(int), s));
    HIPCHK(hipMemcpyAsync(h->d_state, buf_host, sizeof(int32_t) * h->state_words, hipMemcpyHostToDevice, s));
    HIPCHK(launch_set_state(s, h->d, env, h->d_state, h->d_err));
    int err;
    TRY(read_error_word(h, s, &err));
    if (err) return fail(ZS_EINVAL, "state record's needs_reset [5] differs from the engine's (pending resets are not settable)");
    return ZS_OK;
}

extern "C" int zs_overflow(zs_handle* h, uint32_t* flags_host, int32_t clear, void* stream) {
    if (!h || !flags_host) return fail(ZS_EINVAL, "null argument");
    ENTER(h, stream, s);
    uint32_t f = 0;
    HIPCHK(hipMemcpyAsync(&f, h->d.ovf, sizeof(uint32_t), hipMemcpyDeviceToHost, s));
    if (clear) HIPCHK(hipMemsetAsync(h->d.ovf, 0, sizeof(uint32_t), s));
    HIPCHK(hipStreamSynchronize(s));
    *flags_host = f;
    return ZS_OK;
}

// ---------------------------------------------------------------------------
// observation-state records (zs_obs_state.hpp; kernels and launch geometry: k_records.hip)
// ---------------------------------------------------------------------------
static ObsStateLayout handle_obs_state_layout(const zs_handle* h) {
    const Dev& d = h->d;
    return obs_state_layout(d.E, d.O, d.DW, d.OW, obs_state_record_dtype(d.obs_dtype, d.obs_enc));
}

extern "C" int zs_obs_state_layout(const zs_handle* h, int32_t out[12]) {
    if (!h || !out) return fail(ZS_EINVAL, "null argument");
    const ObsStateLayout L = handle_obs_state_layout(h);
    const int32_t v[12] = {L.rec_bytes, L.hp_dirty, L.dead_dirty, L.pos,     L.life, L.dead,
                           L.obst_present, L.obst_hp, L.weapon,     L.present, L.pad,  L.hp_bytes};
    std::memcpy(out, v, sizeof(v));
    return ZS_OK;
}

extern "C" int zs_obs_state_pack(zs_handle* h, void* rec_dev, void* stream) {
    if (!h || !rec_dev) return fail(ZS_EINVAL, "null argument");
    TRY(rec_aligned(rec_dev));
    ENTER(h, stream, s);
    HIPCHK(launch_obs_state_pack(s, h->d, handle_obs_state_layout(h), rec_dev));
    return ZS_OK;
}

extern "C" int zs_obs_state_unpack(zs_handle* h, const void* rec_dev, int32_t rec_bytes, int32_t env0, int32_t n,
                                   void* stream) {
    if (!h || !rec_dev) return fail(ZS_EINVAL, "null argument");
    if (!(h->cfg.flags & ZS_FLAG_VIEWER)) return fail(ZS_ESTATE, "zs_obs_state_unpack: viewer handles only (ZS_FLAG_VIEWER)");
    const ObsStateLayout L = handle_obs_state_layout(h);
    if (rec_bytes != L.rec_bytes) return fail(ZS_EINVAL, "rec_bytes differs from the handle's (zs_obs_state_layout)");
    if (env0 < 0 || n < 0 || (int64_t)env0 + n > h->d.N) return fail(ZS_EINVAL, "env range out of bounds");
    TRY(rec_aligned(rec_dev));
    if (n == 0) return ZS_OK;
    ENTER(h, stream, s);
    HIPCHK(launch_obs_state_unpack(s, h->d, L, env0, n, rec_dev));
    return ZS_OK;
}

// ---------------------------------------------------------------------------
// snapshot records (zs_snapshot.hpp; kernels and launch geometry: k_records.hip): asynchronous, no host staging
// ---------------------------------------------------------------------------
static SnapshotLayout handle_snapshot_layout(const zs_handle* h) {
    const Dev& d = h->d;
    return snapshot_layout(d.E, d.O, d.DW, d.OW, d.A, (d.flags & ZS_FLAG_ENV_PARAMS) != 0, h->ep.run ? h->ep.R : 0,
                           h->rn.body_col ? h->rn.plan.body_bytes : 0);
}

// the engine-side table of a snapshot record (zs_record.hpp): the handle's arrays in record order
static RecTable snapshot_table(const zs_handle* h) {
    const Dev& d = h->d;
    void* const base[SNAP_NSEC] = {d.ring, d.dead, d.obst_hp, d.obst_present, d.obst_nonpos, d.pos, d.life, d.serial,
                                   d.scal, d.hp_dirty, d.dead_dirty, d.rngst, d.prev_life,
                                   d.weapon, d.present, d.order, d.listed};
    return snapshot_rec_table(base, d.E, d.O, d.DW, d.OW, d.A, (size_t)d.N, (d.flags & ZS_FLAG_ENV_PARAMS) ? envp_cur(d) : nullptr,
                              h->ep.run, h->ep.R, h->rn.body_col, h->rn.plan.body_bytes);
}

extern "C" int zs_snapshot_layout(const zs_handle* h, int32_t out[24]) {
    if (!h || !out) return fail(ZS_EINVAL, "null argument");
    const SnapshotLayout L = handle_snapshot_layout(h);
    static_assert(SNAP_NSEC + 7 == 24, "out[24]");
    std::memset(out, 0, 24 * sizeof(int32_t));
    out[0] = L.rec_bytes;
    for (int s = 0; s <= SNAP_NSEC; s++) out[1 + s] = L.off[s];
    out[SNAP_NSEC + 2] = (int32_t)(uint32_t)h->snap_fp;
    out[SNAP_NSEC + 3] = (int32_t)(uint32_t)(h->snap_fp >> 32);
    out[SNAP_NSEC + 4] = ZS_SNAP_NSCAL;
    out[SNAP_NSEC + 5] = ZS_SNAP_RING;
    out[SNAP_NSEC + 6] = L.envp;
    return ZS_OK;
}

extern "C" int zs_snapshot(zs_handle* h, const int32_t* env_idx_dev, int32_t n, void* rec_dev, void* stream) {
    if (!h || !rec_dev) return fail(ZS_EINVAL, "null argument");
    if (n < 0) return fail(ZS_EINVAL, "n must be >= 0");
    TRY(rec_aligned(rec_dev));
    if (n == 0) return ZS_OK;
    ENTER(h, stream, s);
    HIPCHK(launch_snapshot(s, snapshot_table(h), h->d.N, env_idx_dev, n, rec_dev));
    return ZS_OK;
}

extern "C" int zs_restore(zs_handle* h, const void* rec_dev, int32_t rec_bytes, int32_t n_records, const int32_t* src_idx_dev,
                          const int32_t* dst_idx_dev, int32_t n, void* stream) {
    if (!h || !rec_dev) return fail(ZS_EINVAL, "null argument");
    NOT_ON_VIEWER(h, "zs_restore");
    const SnapshotLayout L = handle_snapshot_layout(h);
    if (rec_bytes != L.rec_bytes) return fail(ZS_EINVAL, "rec_bytes differs from the handle's (zs_snapshot_layout)");
    if (n < 0 || n_records < 0) return fail(ZS_EINVAL, "n and n_records must be >= 0");
    TRY(rec_aligned(rec_dev));
    if (n == 0) return ZS_OK;
    ENTER(h, stream, s);
    const Dev& d = h->d;
    // the list the next step drains, rebuilt in place from the restored flags: the copy zeroes its count, the
    // list launch refills it.  rpar stays, the list the next step appends to and the respawn list are empty
    // between calls (zs_step's counter protocol), so cached step graphs stay valid.  No memset nodes (zs_step).
    const int p = h->rpar;
    HIPCHK(launch_restore(s, snapshot_table(h), d, src_idx_dev, dst_idx_dev, n, n_records, rec_dev, h->d_rcount + p));
    HIPCHK(launch_pending_list(s, d.scal + (size_t)S_NEEDRESET * d.N, d.N, h->d_rlist[p], h->d_rcount + p));
    return ZS_OK;
}

// ---------------------------------------------------------------------------
// per-env zombie counts and time limits (ZS_FLAG_ENV_PARAMS; k_env_params.hip): asynchronous, nothing read back
// ---------------------------------------------------------------------------
extern "C" int zs_env_params_set(zs_handle* h, const int32_t* env_idx_dev, int32_t n, const int32_t* params_dev, void* stream) {
    if (!h) return fail(ZS_EINVAL, "null handle");
    TRY(need_flag("zs_env_params_set", (h->d.flags & ZS_FLAG_ENV_PARAMS) != 0, "ZS_FLAG_ENV_PARAMS"));
    if (n < 0) return fail(ZS_EINVAL, "n must be >= 0");
    if (n == 0) return ZS_OK;
    if (n > (1 << 30)) return fail(ZS_EINVAL, "n must be <= 2^30");
    if (!params_dev) return fail(ZS_EINVAL, "null argument");
    ENTER(h, stream, s);
    HIPCHK(launch_env_params_set(s, h->d, h->d_envp_owner, env_idx_dev, n, params_dev));
    return ZS_OK;
}

extern "C" int zs_env_params_check(zs_handle* h, uint32_t* refused_host, void* stream) {
    if (!h || !refused_host) return fail(ZS_EINVAL, "null argument");
    TRY(need_flag("zs_env_params_check", (h->d.flags & ZS_FLAG_ENV_PARAMS) != 0, "ZS_FLAG_ENV_PARAMS"));
    ENTER(h, stream, s);
    uint32_t* word = (uint32_t*)(h->d_envp_owner + h->d.N);
    HIPCHK(launch_env_params_check(s, h->d, word));
    uint32_t f = 0;
    HIPCHK(hipMemcpyAsync(&f, word, sizeof(uint32_t), hipMemcpyDeviceToHost, s));
    HIPCHK(hipStreamSynchronize(s));
    *refused_host = (f & ZS_OVF_PARAM_RANGE) ? 1u : 0u;
    return ZS_OK;
}

extern "C" int zs_env_params_get(zs_handle* h, int32_t which, int32_t* out_dev, void* stream) {
    if (!h || !out_dev) return fail(ZS_EINVAL, "null argument");
    TRY(need_flag("zs_env_params_get", (h->d.flags & ZS_FLAG_ENV_PARAMS) != 0, "ZS_FLAG_ENV_PARAMS"));
    if (which != 0 && which != 1) return fail(ZS_EINVAL, "which must be 0 (next) or 1 (current)");
    ENTER(h, stream, s);
    HIPCHK(launch_env_params_get(s, h->d, which, out_dev));
    return ZS_OK;
}

// ---------------------------------------------------------------------------
// per-env episode statistics (ZS_FLAG_EPISODE_STATS; k_episode.hip): asynchronous, nothing read back
// ---------------------------------------------------------------------------
extern "C" int zs_episode_stats_layout(const zs_handle* h, int32_t out[8]) {
    if (!h || !out) return fail(ZS_EINVAL, "null argument");
    TRY(need_flag("zs_episode_stats_layout", h->ep.run != nullptr, "ZS_FLAG_EPISODE_STATS"));
    const SnapshotLayout L = handle_snapshot_layout(h);
    const int32_t v[8] = {h->ep.R, ZS_EP_LAST, ZS_EP_TOT, L.ep_run, L.ep_bytes, 0, 0, 0};
    std::memcpy(out, v, sizeof(v));
    return ZS_OK;
}

extern "C" int zs_episode_stats_get(zs_handle* h, const uint8_t* env_mask_dev, double* run_ret_dev, double* last_ret_dev,
                                    double* sum_ret_dev, int32_t* last_dev, uint32_t* tot_dev, void* stream) {
    if (!h) return fail(ZS_EINVAL, "null handle");
    TRY(need_flag("zs_episode_stats_get", h->ep.run != nullptr, "ZS_FLAG_EPISODE_STATS"));
    ENTER(h, stream, s);
    HIPCHK(launch_episode_get(s, h->ep, env_mask_dev, run_ret_dev, last_ret_dev, sum_ret_dev, last_dev, tot_dev));
    return ZS_OK;
}

extern "C" int zs_episode_stats_clear(zs_handle* h, const uint8_t* env_mask_dev, void* stream) {
    if (!h) return fail(ZS_EINVAL, "null handle");
    TRY(need_flag("zs_episode_stats_clear", h->ep.run != nullptr, "ZS_FLAG_EPISODE_STATS"));
    ENTER(h, stream, s);
    HIPCHK(launch_episode_clear(s, h->ep, env_mask_dev, 0));
    return ZS_OK;
}

// ---------------------------------------------------------------------------
// the envs' picture (ZS_FLAG_RENDER; k_render.hip, zs_render.hpp)
// ---------------------------------------------------------------------------
extern "C" int zs_render_layout(const zs_handle* h, int32_t out[8]) {
    if (!h || !out) return fail(ZS_EINVAL, "null argument");
    TRY(need_flag("zs_render_layout", h->rn.body_col != nullptr, "ZS_FLAG_RENDER"));
    const RenderPlan& p = h->rn.plan;
    const int32_t v[8] = {p.frame_h, p.frame_w, p.frame_bytes, ZS_RENDER_CELL, ZS_RENDER_MASK, ZS_RENDER_PALETTE, p.body_bytes,
                          handle_snapshot_layout(h).body_col};
    std::memcpy(out, v, sizeof(v));
    return ZS_OK;
}

extern "C" int zs_render(zs_handle* h, const int32_t* envs_dev, int32_t n, uint8_t* out_dev, int32_t n_frames, void* stream) {
    if (!h) return fail(ZS_EINVAL, "null handle");
    TRY(need_flag("zs_render", h->rn.body_col != nullptr, "ZS_FLAG_RENDER"));
    if (n < 0 || n_frames < 0) return fail(ZS_EINVAL, "zs_render: negative count");
    const long frames = std::min(n, n_frames);
    if (frames == 0) return ZS_OK;
    if (!out_dev) return fail(ZS_EINVAL, "zs_render: null output");
    if (frames * h->rn.plan.bands > 0x7fffffffL) return fail(ZS_EINVAL, "zs_render: too many frames for one launch");
    ENTER(h, stream, s);
    LAUNCHCHK("k_render", launch_render(s, h->rn, envs_dev, n, out_dev, n_frames));
    return ZS_OK;
}

extern "C" int zs_render_sprites(zs_handle* h, const uint32_t masks[5][4], const uint8_t palette[8][3]) {
    if (!h || !masks || !palette) return fail(ZS_EINVAL, "null argument");
    TRY(need_flag("zs_render_sprites", h->rn.body_col != nullptr, "ZS_FLAG_RENDER"));
    HIPCHK(hipSetDevice(h->device));
    HIPCHK(hipDeviceSynchronize());  // the atlas is a launch argument: frames already queued keep the one they took
    RenderAtlas& a = h->rn.atlas;
    for (int s = 0; s < RS_NSHAPE - 1; s++)
        for (int w = 0; w < ZS_RENDER_MASK_WORDS; w++) a.mask[s][w] = masks[s][w] & (w == 3 ? 0x01ffffffu : ~0u);  // 121 bits
    for (int i = 0; i < ZS_RENDER_PALETTE; i++)
        a.rgb[i] = (uint32_t)palette[i][0] | ((uint32_t)palette[i][1] << 8) | ((uint32_t)palette[i][2] << 16);
    return ZS_OK;
}

// ---------------------------------------------------------------------------
// An env's MT19937 stream in CPython's random.getstate() form: state[0..623] = the raw
// block being consumed, state[624] = index of the next word (0..624; 624 = exhausted, the
// next draw twists).  The single-env wrappers move the process-global `random` state in
// and out of the engine around every call, so the engine draws from exactly the stream the
// reference's `random` module would (one process-global RNG).
// ---------------------------------------------------------------------------
extern "C" int zs_get_rng(zs_handle* h, int32_t env, uint32_t* state_host, void* stream) {
    if (!h || !state_host) return fail(ZS_EINVAL, "null argument");
    if (env < 0 || env >= h->d.N) return fail(ZS_EINVAL, "env index out of range");
    ENTER(h, stream, s);
    uint32_t st = 0;
    std::vector<uint32_t> ring(ZS_RING_WORDS);
    HIPCHK(hipMemcpyAsync(&st, h->d.rngst + env, sizeof(uint32_t), hipMemcpyDeviceToHost, s));
    HIPCHK(hipMemcpyAsync(ring.data(), h->d.ring + (size_t)env * ZS_RING_WORDS, sizeof(uint32_t) * ZS_RING_WORDS,
                          hipMemcpyDeviceToHost, s));
    HIPCHK(hipStreamSynchronize(s));
    uint32_t off = st & 1023u, slot = (st >> 10) & 1u;
    std::memcpy(state_host, ring.data() + slot * ZS_MT_N, sizeof(uint32_t) * ZS_MT_N);
    state_host[ZS_MT_N] = off;
    return ZS_OK;
}

// a getstate() block as an env's ring: slot 0 = the given block, slot 1 = its successor (x[k+624] = x[k+397] ^
// f(x[k], x[k+1])); returns the env's rngst word (the block's index, slot 0, next block ready)
static uint32_t ring_from_state(uint32_t* ring, const uint32_t* state) {
    std::memcpy(ring, state, sizeof(uint32_t) * ZS_MT_N);
    for (int k = 0; k < ZS_MT_N; k++) {
        uint32_t a = ring[k], b = ring[k + 1], c = ring[k + ZS_MT_M];
        uint32_t y = (a & 0x80000000u) | (b & 0x7fffffffu);
        ring[ZS_MT_N + k] = c ^ (y >> 1) ^ ((y & 1u) ? 0x9908b0dfu : 0u);
    }
    return state[ZS_MT_N] | (0u << 10) | (1u << 11);
}

extern "C" int zs_set_rng(zs_handle* h, int32_t env, const uint32_t* state_host, void* stream) {
    if (!h || !state_host) return fail(ZS_EINVAL, "null argument");
    NOT_ON_VIEWER(h, "zs_set_rng");
    if (env < 0 || env >= h->d.N) return fail(ZS_EINVAL, "env index out of range");
    if (state_host[ZS_MT_N] > ZS_MT_N) return fail(ZS_EINVAL, "MT index out of range (0..624)");
    ENTER(h, stream, s);
    std::vector<uint32_t> ring(ZS_RING_WORDS);
    const uint32_t st = ring_from_state(ring.data(), state_host);
    HIPCHK(hipMemcpyAsync(h->d.ring + (size_t)env * ZS_RING_WORDS, ring.data(), sizeof(uint32_t) * ZS_RING_WORDS,
                          hipMemcpyHostToDevice, s));
    HIPCHK(hipMemcpyAsync(h->d.rngst + env, &st, sizeof(uint32_t), hipMemcpyHostToDevice, s));
    HIPCHK(hipStreamSynchronize(s));
    return ZS_OK;
}

// ---------------------------------------------------------------------------
// diagnostics: per-kernel device time from HIP events recorded on the launch stream
// ---------------------------------------------------------------------------
extern "C" int zs_profile(zs_handle* h, int32_t enable) {
    if (!h) return fail(ZS_EINVAL, "null handle");
    h->prof = enable ? 1 : 0;
    prof_clear(h);
    return ZS_OK;
}

extern "C" int zs_profile_read(zs_handle* h, double* out) {
    if (!h || !out) return fail(ZS_EINVAL, "null argument");
    HIPCHK(hipSetDevice(h->device));
    double tot[4] = {0.0, 0.0, 0.0, 0.0};
    EventList* lists[4] = {&h->ev_tick, &h->ev_obs, &h->ev_reset, &h->ev_respawn};
    for (int k = 0; k < 4; k++)
        for (auto& pr : *lists[k]) {
            HIPCHK(hipEventSynchronize(h->ev_pool[pr.second]));
            float ms = 0.f;
            HIPCHK(hipEventElapsedTime(&ms, h->ev_pool[pr.first], h->ev_pool[pr.second]));
            tot[k] += ms;
        }
    for (int k = 0; k < 4; k++) out[2 * k] = tot[k], out[2 * k + 1] = (double)lists[k]->size();
    prof_clear(h);
    return ZS_OK;
}

extern "C" int zs_describe(zs_handle* h, char* buf, int32_t len) {
    if (!h || !buf || len <= 0) return fail(ZS_EINVAL, "null argument");
    const Dev& d = h->d;
    const ObsKernel& kf = h->obs.full;
    const StepPlan& p = h->step;
    snprintf(buf, (size_t)len,
             "{\"envs\": %d, \"entities\": %d, \"lanes_per_env\": %d, \"step_kernel\": \"%s\", \"step_lds\": %d, "
             "\"step_wgs_per_cu\": %d, \"rng_window\": %d, \"obs_kernel\": \"%s\", \"reset_side_stream\": %d, "
             "\"reset_lds\": %d, \"respawn\": \"%s\", \"tick_waves\": %d, \"rng_step\": %d, \"par_exec\": %d, "
             "\"obs_kernel_masked\": \"%s\", \"obs_encoders\": \"%s\", \"mask_kernel\": \"k_action_mask\", "
             "\"mask_grid\": %u, \"mask_block\": %d, \"mask_bound\": %d, \"env_params\": %d, \"episode_stats\": %d, "
             "\"render\": %d, \"render_grid\": %d, \"render_block\": %d, \"entity_obs_bound\": %d, \"entity_kz\": %d, "
             "\"entity_kp\": %d, \"autopilot_kernel\": \"k_autopilot\", \"autopilot_grid\": %u, \"autopilot_block\": %d, "
             "\"autopilot_bound\": %d, \"nav_bound\": %d, \"nav_fields\": %d, \"nav_max_dist\": %d, \"nav_kernel\": \"k_nav\", "
             "\"nav_envs_per_wg\": %d, \"nav_block\": %d, \"nav_lds_bytes\": %d, \"entity_act_kernel\": \"k_entity_act\", "
             "\"entity_act_ids_bound\": %d, \"entity_act_mask_bound\": %d, \"step_tail_launch\": \"%s\", "
             "\"step_policy\": \"%s\"}",
             d.N, d.E, p.G, p.fused ? "k_step" : "k_tick", p.lds, p.resident, p.rw_cap,
             d.fobs ? "step launch" : obs_kernel_name(kf.kind), h->reset_side,
             p.reset_lds, p.defer_respawn ? "k_respawn" : "tick", p.tick_waves, p.rw_step,
             d.par_exec, obs_kernel_name(h->obs.masked.kind), obs_encoders_name(kf), zs_mask_grid(d.N), ZS_MASK_BLOCK,
             h->mask_bound ? 1 : 0, (d.flags & ZS_FLAG_ENV_PARAMS) ? 1 : 0, h->ep.run ? 1 : 0, h->rn.body_col ? 1 : 0,
             h->rn.body_col ? h->rn.plan.bands : 0, h->rn.body_col ? ZS_RENDER_BLOCK : 0,
             h->ent_bound ? 1 : 0, h->ent_kz, h->ent_kp, zs_pilot_grid(d.N), ZS_PILOT_BLOCK, h->pilot_out ? 1 : 0,
             h->nav_bound ? 1 : 0, h->nav_fields, h->nav_max_dist, h->nav.envs_per_wg, h->nav.block, h->nav.lds_bytes,
             h->eact_ids ? 1 : 0, h->eact_mask ? 1 : 0, h->step_last, h->step_policy);
    return ZS_OK;
}

// One env's log of its last step (ZS_FLAG_DEATH_LOG): `log` [N][E][words] and its counts.  *n_out: the count clamped
// to [lo, E]; out_host: the first min(entries, cap) entries, a count n < 0 standing for -1 - n entries.
static int read_log(zs_handle* h, const int32_t* log, const int32_t* log_n, int words, int lo, int32_t env, int32_t* out_host,
                    int32_t cap, int32_t* n_out, void* stream) {
    if (!h || !n_out || (cap > 0 && !out_host)) return fail(ZS_EINVAL, "null argument");
    if (!log) return fail(ZS_EINVAL, "the handle was created without ZS_FLAG_DEATH_LOG");
    if (env < 0 || env >= h->d.N) return fail(ZS_EINVAL, "env out of range");
    ENTER(h, stream, s);
    int32_t n = 0;
    HIPCHK(hipMemcpyAsync(&n, log_n + env, sizeof(int32_t), hipMemcpyDeviceToHost, s));
    HIPCHK(hipStreamSynchronize(s));
    n = std::max(lo, std::min(n, h->d.E));
    const int k = std::min(n < 0 ? -1 - n : n, std::max(0, (int)cap));
    if (k > 0) {
        HIPCHK(hipMemcpyAsync(out_host, log + (size_t)env * h->d.E * words, sizeof(int32_t) * words * k, hipMemcpyDeviceToHost, s));
        HIPCHK(hipStreamSynchronize(s));
    }
    *n_out = n;
    return ZS_OK;
}

// The actions env's last step executed, in execution order (the shuffled action list of World.step,
// core.py:76,103-119): per action {slot | kind << 8, target}, kind 1 move (target: the destination,
// x | y << 16), 2 attack, 3 heal (target: an entity slot, or -1 - obstacle index).  Needs ZS_FLAG_DEATH_LOG.
// n < 0: a debug raise stopped the step; -1 - n actors before the raising one decided an action
extern "C" int zs_action_log(zs_handle* h, int32_t env, int32_t* out_host, int32_t cap, int32_t* n_out, void* stream) {
    return read_log(h, h ? h->d.alog : nullptr, h ? h->d.alog_n : nullptr, 2, h ? -1 - h->d.E : 0, env, out_host, cap, n_out, stream);
}

// The things env's last tick's cleanup removed, in removal order: {slot, serial, x, y, life} each (Dev::dlog)
extern "C" int zs_death_log(zs_handle* h, int32_t env, int32_t* out_host, int32_t cap, int32_t* n_out, void* stream) {
    return read_log(h, h ? h->d.dlog : nullptr, h ? h->d.dlog_n : nullptr, 5, 0, env, out_host, cap, n_out, stream);
}

// ---------------------------------------------------------------------------
// The drop-ins' per-call path.  The reference's env.step / env.reset / env.get_observation run one env
// per call on the host (gym_env.py:99-164, gym/multiagent_env.py:111-184) and share the process-global
// `random` stream.  Here one call is: the caller's actions and `random` state written into one pinned,
// device-mapped block that the kernels read in place, the engine's launches, k_host_pack writing
// everything the host reads back (outputs, the advanced stream, the action / death logs, the state
// record, the observation) into one pinned, device-mapped record per env, and one synchronisation.
// ---------------------------------------------------------------------------
static int obs_bytes_per_env(const zs_handle* h) {
    int32_t shp[4];
    zs_obs_shape(h, shp);
    return shp[0] * shp[1] * shp[2] * shp[3] * obs_tsize(h->d.obs_dtype);
}

static HostLayout host_layout(const zs_handle* h) {
    const Dev& d = h->d;
    HostLayout L;
    L.R = d.reward_mode == ZS_REWARD_SINGLE ? 1 : d.A;
    L.obs_bytes = obs_bytes_per_env(h);
    L.rew = ZS_HOST_RNG + ZS_MT_N + 2;  // even: the rewards are float64
    L.alog = L.rew + 2 * L.R;
    L.dlog = L.alog + 2 * d.E;
    L.state = L.dlog + 5 * d.E;
    L.obs = (L.state + h->state_words + 3) & ~3;  // 16-byte aligned
    L.words = (L.obs + (L.obs_bytes + 3) / 4 + 3) & ~3;
    return L;
}

static int host_init(zs_handle* h) {
    if (h->d_hrec) return ZS_OK;
    const Dev& d = h->d;
    const size_t N = d.N;
    HostLayout L = host_layout(h);
    const size_t in_words = N * d.A * 3 + N * (ZS_RING_WORDS + 1);
    TRY(dalloc(h, &h->d_hobs, N * L.obs_bytes));
    TRY(dalloc(h, &h->d_hrew, N * L.R));
    TRY(dalloc(h, &h->d_hflags, N * (3 + d.A)));
    // coherent (uncached on the device) so the kernels see this call's input and the host the record
    // without copies; the blocks are a few KB per env
    const unsigned fl = hipHostMallocMapped | hipHostMallocCoherent;
    HIPCHK(hipHostMalloc((void**)&h->h_hin, in_words * sizeof(int32_t), fl));
    HIPCHK(hipHostMalloc((void**)&h->h_hrec, N * L.words * sizeof(int32_t), fl));
    HIPCHK(hipHostGetDevicePointer((void**)&h->d_hin, h->h_hin, 0));
    HIPCHK(hipHostGetDevicePointer((void**)&h->d_hrec, h->h_hrec, 0));
    h->hl = L;
    return ZS_OK;
}

// the `random` states of envs [0, N) (CPython getstate() form, 625 words each) into the pinned input
// block after the actions: per env its ring (the block, then its successor) and its st word
static int host_stage_rng(zs_handle* h, const uint32_t* rng_host) {
    const size_t N = h->d.N;
    uint32_t* rings = (uint32_t*)h->h_hin + N * h->d.A * 3;
    uint32_t* st = rings + N * ZS_RING_WORDS;
    for (size_t e = 0; e < N; e++) {
        const uint32_t* g = rng_host + e * (ZS_MT_N + 1);
        if (g[ZS_MT_N] > ZS_MT_N) return fail(ZS_EINVAL, "MT index out of range (0..624)");
        st[e] = ring_from_state(rings + e * ZS_RING_WORDS, g);
    }
    return ZS_OK;
}

enum { HOST_STEP = 0, HOST_RESET = 1, HOST_OBSERVE = 2 };

static int host_call(zs_handle* h, int op, const int32_t* actions_host, const uint32_t* rng_host, int32_t* rec_host,
                     hipStream_t s) {
    NOT_ON_VIEWER(h, "zs_host_step / zs_host_reset / zs_host_observe");
    HIPCHK(hipSetDevice(h->device));
    int rc = host_init(h);
    if (rc) return rc;
    const Dev& d = h->d;
    const size_t N = d.N;
    const HostLayout& L = h->hl;
    if (op == HOST_STEP) std::memcpy(h->h_hin, actions_host, sizeof(int32_t) * N * d.A * 3);
    if (rng_host && (rc = host_stage_rng(h, rng_host))) return rc;
    if (rng_host) {
        const uint32_t* rings = (const uint32_t*)h->d_hin + N * d.A * 3;
        HIPCHK(launch_host_unpack(s, d, rings, rings + N * ZS_RING_WORDS, h->d_err));
    }
    uint8_t *done = h->d_hflags, *trunc = done + N, *rst = trunc + N, *listed = rst + N;
    // the record's error word is this call's alone: an earlier zs_step whose reset work failed leaves the word
    // set (zs_step never reads it), and so does an earlier host call (k_host_pack only reads it).  Cleared
    // ahead of the call's launches without a launch of its own where one is queued anyway: by k_host_unpack
    // (the drop-ins pass their stream on every call) or by queue_reset; else by a memset
    if (!rng_host && op != HOST_RESET) HIPCHK(hipMemsetAsync(h->d_err, 0, sizeof(int), s));
    if (op == HOST_STEP) {
        rc = zs_step(h, h->d_hin, h->d_hobs, h->d_hrew, done, trunc, listed, rst, s);
    } else if (op == HOST_RESET) {
        HIPCHK(hipMemsetAsync(h->d_hflags, 0, N * 3, s));
        HIPCHK(hipMemsetAsync(h->d_hrew, 0, N * L.R * sizeof(double), s));
        rc = queue_reset(h, nullptr, h->d_hobs, s);
    } else {
        rc = launch_obs(h, d, h->d_hobs, nullptr, s);
    }
    if (rc) return rc;
    HIPCHK(launch_host_pack(s, d, L, h->d_hobs, h->d_hrew, done, trunc, op == HOST_RESET ? nullptr : rst, h->d_err, h->d_hrec));
    HIPCHK(hipStreamSynchronize(s));
    std::memcpy(rec_host, h->h_hrec, N * L.words * sizeof(int32_t));
    return reset_result(h->h_hrec[ZS_HOST_ERR]);
}

extern "C" int zs_host_layout(zs_handle* h, int32_t out[8]) {
    if (!h || !out) return fail(ZS_EINVAL, "null argument");
    NOT_ON_VIEWER(h, "zs_host_layout");
    const HostLayout L = host_layout(h);
    const int32_t v[8] = {L.words, L.rew, L.alog, L.dlog, L.state, L.obs, L.obs_bytes, L.R};
    std::memcpy(out, v, sizeof(v));
    return ZS_OK;
}

extern "C" int zs_host_step(zs_handle* h, const int32_t* actions_host, const uint32_t* rng_host, int32_t* rec_host,
                            void* stream) {
    if (!h || !actions_host || !rec_host) return fail(ZS_EINVAL, "null argument");
    return host_call(h, HOST_STEP, actions_host, rng_host, rec_host, (hipStream_t)stream);
}

extern "C" int zs_host_reset(zs_handle* h, const uint32_t* rng_host, int32_t* rec_host, void* stream) {
    if (!h || !rec_host) return fail(ZS_EINVAL, "null argument");
    return host_call(h, HOST_RESET, nullptr, rng_host, rec_host, (hipStream_t)stream);
}

extern "C" int zs_host_observe(zs_handle* h, int32_t* rec_host, void* stream) {
    if (!h || !rec_host) return fail(ZS_EINVAL, "null argument");
    return host_call(h, HOST_OBSERVE, nullptr, nullptr, rec_host, (hipStream_t)stream);
}

// Diagnostics: the work-list counters as they stand after everything queued on `stream` (out[0..1]
// the two pending-reset list counts, out[2] the deferred-respawn count, out[3] the parity the next
// step drains).
extern "C" int zs_debug_lists(zs_handle* h, int32_t* out, void* stream) {
    if (!h || !out) return fail(ZS_EINVAL, "null argument");
    ENTER(h, stream, s);
    int v[3] = {0, 0, 0};
    HIPCHK(hipMemcpyAsync(v, h->d_rcount, 2 * sizeof(int), hipMemcpyDeviceToHost, s));
    HIPCHK(hipMemcpyAsync(v + 2, h->d.resp_count, sizeof(int), hipMemcpyDeviceToHost, s));
    HIPCHK(hipStreamSynchronize(s));
    out[0] = v[0];
    out[1] = v[1];
    out[2] = v[2];
    out[3] = h->rpar;
    return ZS_OK;
}

// ---------------------------------------------------------------------------
// diagnostic build (-DZS_STAMPS): per-phase k_tick cycle sums since the last read
// ---------------------------------------------------------------------------
// diagnostic build (-DZS_STAMPS): start / end s_memrealtime of the first n workgroups of the last step launch
extern "C" int zs_debug_timeline(zs_handle* h, uint64_t* out, int32_t n) {
#ifdef ZS_STAMPS
    if (!h || !out || n < 0 || n > ZS_STAMP_WGS) return fail(ZS_EINVAL, "bad argument");
    HIPCHK(hipSetDevice(h->device));
    HIPCHK(hipDeviceSynchronize());
    std::vector<unsigned long long> tl((size_t)ZS_STAMP_WGS * 2);
    HIPCHK(tick_unit(h->step.G).stamps(nullptr, tl.data(), 0));
    std::memcpy(out, tl.data(), (size_t)n * 2 * sizeof(unsigned long long));
    return ZS_OK;
#else
    (void)h; (void)out; (void)n;
    return fail(ZS_ESTATE, "not a ZS_STAMPS diagnostic build");
#endif
}

extern "C" int zs_debug_stamps_wg(zs_handle* h, uint64_t* out, int32_t n_wgs, int32_t n_phase) {
#ifdef ZS_STAMPS
    if (!h || !out || n_wgs < 0 || n_wgs > ZS_STAMP_WGS || n_phase < 1 || n_phase > ZS_NPHASE)
        return fail(ZS_EINVAL, "bad argument");
    HIPCHK(hipSetDevice(h->device));
    HIPCHK(hipDeviceSynchronize());
    std::vector<unsigned long long> buf((size_t)ZS_STAMP_WGS * ZS_NPHASE);
    HIPCHK(tick_unit(h->step.G).stamps(buf.data(), nullptr, 1));
    for (int w = 0; w < n_wgs; w++)
        for (int k = 0; k < n_phase; k++) out[(size_t)w * n_phase + k] = buf[(size_t)w * ZS_NPHASE + k];
    return ZS_OK;
#else
    (void)h; (void)out; (void)n_wgs; (void)n_phase;
    return fail(ZS_ESTATE, "not a ZS_STAMPS diagnostic build");
#endif
}

// per-phase sums over the step-kernel unit of this handle's G and the reset unit (k_reset's phases)
extern "C" int zs_debug_stamps(zs_handle* h, uint64_t* sum_out, uint64_t* max_out, int32_t n) {
#ifdef ZS_STAMPS
    if (!h || !sum_out || n > ZS_NPHASE) return fail(ZS_EINVAL, "bad argument");
    HIPCHK(hipSetDevice(h->device));
    HIPCHK(hipDeviceSynchronize());
    std::vector<unsigned long long> buf((size_t)ZS_STAMP_WGS * ZS_NPHASE), rb(buf.size());
    HIPCHK(tick_unit(h->step.G).stamps(buf.data(), nullptr, 1));
    HIPCHK(stamps_reset(rb.data(), 1));
    for (int k = 0; k < n; k++) {
        sum_out[k] = 0;
        if (max_out) max_out[k] = 0;
    }
    for (size_t w = 0; w < (size_t)ZS_STAMP_WGS; w++)
        for (int k = 0; k < n; k++) {
            unsigned long long v = buf[w * ZS_NPHASE + k] + rb[w * ZS_NPHASE + k];
            sum_out[k] += v;
            if (max_out && v > max_out[k]) max_out[k] = v;
        }
    return ZS_OK;
#else
    (void)h; (void)sum_out; (void)max_out; (void)n;
    return fail(ZS_ESTATE, "not a ZS_STAMPS diagnostic build");
#endif
}
