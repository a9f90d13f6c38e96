// zs_step_plan.hpp — how a handle launches its step: lanes per env, fused or not, LDS images, grids.
//
// step_plan() decides, from the config's integers and the zs_launch overrides alone, everything about
// the step launch (k_tick / k_step, zs_tick.hpp), the reset launch (k_reset, zs_reset.hpp) and the
// respawn launch (k_respawn) that does not depend on the caller's buffers.  The LDS images it sizes
// (tick_layout, reset_lds_bytes) are the ones the kernels lay out.  Nothing here needs HIP: the kernels,
// the engine and a plain host compiler (the plan's CPU test, tests/step_plan_dump.cpp) include the same
// file.
#pragma once
#include <stdint.h>

#include <algorithm>

#include "zs_obs_plan.hpp"  // ZS_HD, zs_launch

// minimum waves per SIMD the one-wave step / tick / reset kernels are compiled for (register budget):
// 6 caps k_tick at 80 VGPRs (88 unbounded: 5 waves) for a few dwords of scratch on cold paths;
// measured C3 125 -> 127, C5 109 -> 114 M env-steps/s, C4 unchanged; 8 (64 VGPRs) spills more and
// loses at C4
#ifndef ZS_STEP_WAVES
#define ZS_STEP_WAVES 6
#endif
// The fused step launch (k_step) is chosen only when the whole launch is resident at once (at most
// 4 * ZS_FUSED_WAVES one-wave workgroups per CU), and k_reset runs a few waves per CU beside the tick
// (3.8 measured at C3): neither needs k_tick's occupancy, and at 6 waves both spill (k_step 244,
// k_reset 292 bytes of scratch per lane, on their serial chains).  3 waves: 147 / 151 VGPRs, none.
#ifndef ZS_FUSED_WAVES
#define ZS_FUSED_WAVES 3
#endif

#define ZS_MT_N 624

// ---------------------------------------------------------------------------
// LDS images
// ---------------------------------------------------------------------------
// LDS footprint of one step workgroup (host and device agree on this layout).  The entity columns the
// observations need (pos, life, weapon, present) sit before `region`; everything in `region` is
// dead once the tick's state is stored, so the observation image of the env being encoded and the
// MT twist buffer alias it.
struct TickLayout {
    int ne;                                  // envs per workgroup
    int off_lists;                           // static spawn lists (player then zombie), shared by the WG
    int off_misc;                            // per-env scalars / tracker, [MISC_*][ne] int32
    int off_lst;
    int off_pos, off_life, off_weap, off_pres;
    int off_region;                          // = off_bm
    int off_bm, off_rw, off_cand, off_tgt, off_act, off_order, off_rank, off_kind, off_perm, off_moved, off_xs;
    int bytes;
};

// per-env LDS scalars (MISC rows); rows MISC_N.. hold prev_life[A] then listed[A].  MISC_NMOVED and
// MISC_NORD are scratch rows of the tick's leader / group hand-off (not staged from or to HBM).
enum { MISC_T = 0, MISC_DEATHS, MISC_ZD, MISC_EPSTEPS, MISC_PREVZD, MISC_SERIAL, MISC_ODIRTY, MISC_NMOVED, MISC_NORD, MISC_N };

ZS_HD inline TickLayout tick_layout(int ne, int E, int DW, int rw_cap, int cand_cap, int lists_cap, int A,
                                    int obs_bytes = 0) {
    TickLayout L;
    L.ne = ne;
    int o = 0;
    L.off_lists = o;
    o += lists_cap * 4;
    L.off_misc = o;
    o += (MISC_N + 2 * A) * ne * 4;
    L.off_lst = o;
    o += ne * 4;
    L.off_pos = o;
    o += E * ne * 4;
    L.off_life = o;
    o += E * ne * 4;
    L.off_weap = o;
    o += E * ne;
    L.off_pres = o;
    o += E * ne;
    L.off_order = o;  // the dict order is stored out after the MT refill, whose buffer aliases the region
    o += E * ne;
    o = ((o + 15) / 16) * 16;
    const int region = o;
    L.off_region = L.off_bm = o;
    o += DW * ne * 4;
    L.off_rw = o;
    o += rw_cap * ne * 4;
    L.off_tgt = o;
    o += E * ne * 4;
    L.off_act = o;  // the agents' action triples, loaded with the stage-in round
    o += 3 * A * ne * 4;
    L.off_cand = o;
    o += ((cand_cap * ne * 2 + 3) / 4) * 4;
    L.off_rank = o;
    o += E * ne;
    L.off_kind = o;
    o += E * ne;
    L.off_perm = o;
    o += E * ne;
    L.off_moved = o;
    o += E * ne;
    o = ((o + 15) / 16) * 16;
    L.off_xs = o;  // grp_execute's two tables of 64 words (G per env)
    o += 2 * 64 * 4;
    // the MT twist buffer (2 x 624 words) and one env's observation image alias the region
    if (o - region < 2 * ZS_MT_N * 4) o = region + 2 * ZS_MT_N * 4;
    if (o - region < obs_bytes) o = region + obs_bytes;
    L.bytes = o;
    return L;
}

// the `lst` row (one word per env) lies right behind the MISC rows: the tick reads an env's entry as MISC row
// MISC_N + 2A (zs_tick.hpp LEADER_WORD); zs_create refuses to run on a layout that says otherwise
ZS_HD inline bool tick_lst_is_behind_misc(const TickLayout& L, int A) { return L.off_lst == L.off_misc + (MISC_N + 2 * A) * L.ne * 4; }

// the reset work's image; its twist buffer doubles as the observation image of the env just rebuilt (obs_bytes)
ZS_HD inline int reset_lds_bytes(int E, int DW, int ncand, int lists_cap, int obs_bytes = 0) {
    int o = DW * 4 + ncand * 4 + 2 * E * 4 + 4 * E + lists_cap * 4 + (E + 8) * 4;
    o = ((o + 15) / 16) * 16;
    return o + (obs_bytes > 2 * ZS_MT_N * 4 ? obs_bytes : 2 * ZS_MT_N * 4);
}

// ---------------------------------------------------------------------------
// the plan
// ---------------------------------------------------------------------------
// the integers the choice reads (zs_create fills them from the config; Dev's names)
struct StepShape {
    int N, W, H, E, A, DW, ncand, nps, nzs;
    int minimum_zombies;
    int lanes_per_env;  // zs_config.lanes_per_env: 0 (automatic) or a power of two in 1..64
    int obs_bytes;      // the step launch's observation image: fobs ? obsl.bytes + 4 * obs_stat : 0 (obs_plan)
};

struct StepPlan {
    int G;           // lanes per env in k_tick / k_step
    int fused;       // zs_step runs reset work and the tick in one launch (k_step)
    int tick_waves;  // the step kernel's register budget (waves per SIMD it is compiled for)
    int lds;         // the step launch's dynamic LDS bytes
    int resident;    // step-launch workgroups resident per CU
    int want;        // workgroups per CU the launch has (capped at 32)
    int rw_cap, rw_step, cand_cap, lists_cap, rlists_cap;  // Dev's fields of these names
    int reset_lds;   // k_reset's and k_respawn's dynamic LDS bytes
    int side_stream;  // the reset work of an unfused step wants a side stream (the engine creates it)
    int n_reset;      // reset-work workgroups ahead of the tick workgroups of a fused launch, else 0
    int reset_grid_list, reset_grid_mask;  // k_reset's grid over a pending list / over an env mask
    int respawn_grid;
    int defer_respawn;  // Dev::defer_respawn (step_defer_respawn)
    const char* error;  // non-null: no step image fits
};

// zombie respawn as wave work after the tick (k_respawn) when its shuffle is long: the tick's
// leader would draw one word per candidate serially.  zs_launch.defer_respawn forces either.
inline int step_defer_respawn(int minimum_zombies, int n_zombie_spawns, int cells, const zs_launch& ov) {
    const int cands = n_zombie_spawns ? n_zombie_spawns : cells;
    return minimum_zombies > 0 && (ov.defer_respawn ? ov.defer_respawn > 0 : cands > 64);
}

// reset-work workgroups of a fused step launch (zs_launch.reset_wgs overrides)
inline int step_reset_wgs(const StepShape& s, const zs_launch& ov) { return std::min(s.N, ov.reset_wgs > 0 ? (int)ov.reset_wgs : 256); }

// Layout of the step launch.  Workgroups of the launch resident at once on the 256 CUs decide how
// much LDS one may take: among the layouts that fit 64 KiB, take the one with the most resident
// workgroups (at most 32 one-wave workgroups per CU), then the largest optional LDS copies (RNG
// window beyond 64 words, spawn candidates, spawn lists).  A fused launch (reset work + tick in
// one) allocates max(tick image, reset image) for every workgroup.
struct StepLayout {
    int G;  // 0: no image fits at any G from the first one tried
    int lds, resident, want, rw_cap, rw_step, cand_cap, lists_cap;
    int rounds() const { return (want + resident - 1) / resident; }
};

// the best layout from want_g lanes per env (0: automatic) up
inline StepLayout step_layout(const StepShape& s, const zs_launch& ov, int want_g, bool fused) {
    const int kMax = 64 * 1024;
    // A launch of many resident rounds is bound by the envs it keeps in flight per CU (k_tick at C3:
    // 19 -> 15 resident workgroups of G = 8 took the launch from 121 to 153 us), a one-round launch by
    // the latency of one workgroup.  Measured on one MI355X: G = 8 beats 16 when G = 16 needs more
    // than two rounds (C3, 65536 envs, E = 12: 121 vs 140 us), G = 16 beats 8 at 8192 and 16384 envs
    // and at C5 (E = 24); G = 32 beats 16 at C4 (E = 54: the decisions spread over more lanes).
    // one-wave workgroups per CU the register budget admits (k_step's or k_tick's)
    const int wave_cap = 4 * (fused ? ZS_FUSED_WAVES : ZS_STEP_WAVES);
    int g0 = want_g > 0 ? want_g : (s.E > 32 ? 32 : 16);
    if (want_g <= 0 && s.E <= 16 && (long)s.N > 2L * wave_cap * 256 * (64 / 16)) g0 = 8;
    const int cand_full = (s.W * s.H <= 65535) ? s.ncand : 0;
    // RNG window: a plain step draws about 1.5 words per actor (shuffle) plus one per attack or heal
    // in range; a window that runs dry sends the leader to HBM.  Measured with the oracle (uniform
    // Discrete(7) agents): C3 (E = 12) mean 12, p99 26, max 37 words; C5 (E = 24) mean 23, p99 46,
    // max 63; C4 (E = 54) median 82.  2E + 8 rounded up to a power of two covers them.
    int rw_need = 32;
    while (rw_need < 512 && rw_need < 2 * s.E + 8) rw_need *= 2;
    if (ov.rw_need > 0) rw_need = std::max(32, std::min(512, (int)ov.rw_need));
    const int lists = (s.nps + s.nzs <= 4096) ? s.nps + s.nzs : 0;
    for (int G = g0; G <= 64; G *= 2) {
        const int ne = 64 / G;
        const int wgs = (s.N + ne - 1) / ne + (fused ? step_reset_wgs(s, ov) : 0);
        const int want = ov.lds_budget < 0 ? 1 : std::min(32, std::max(1, (wgs + 255) / 256));
        StepLayout best = {};
        for (int pass = 0; pass < 2 && !best.G; pass++)  // windows below the need only if nothing else fits
        for (int cand : {cand_full, 0})
            for (int lst : {lists, 0})
                for (int rw : {512, 256, 128, 64, 32}) {
                    if (pass == 0 && rw < rw_need) continue;
                    int bytes = tick_layout(ne, s.E, s.DW, rw, cand, lst, s.A, s.obs_bytes).bytes;
                    if (fused) bytes = std::max(bytes, reset_lds_bytes(s.E, s.DW, s.ncand, lst, s.obs_bytes));
                    if (bytes > kMax) continue;
                    const int res = std::min(std::min(want, wave_cap), 160 * 1024 / bytes);  // >= 1
                    if (res > best.resident) best = StepLayout{G, bytes, res, want, rw, std::min(rw, rw_need), cand, lst};
                }
        if (best.G) return best;
    }
    return StepLayout{};
}

// the step launch (fused or not, lanes per env, LDS copies), the reset launch's image and grids, and
// whether an unfused step's reset work goes to a side stream
inline StepPlan step_plan(const StepShape& s, const zs_launch& ov) {
    StepPlan p = {};
    p.defer_respawn = step_defer_respawn(s.minimum_zombies, s.nzs, s.W * s.H, ov);
    // Fused step launch (reset work + tick in one) when the whole launch is resident at once: then
    // the step is one latency-bound round and the reset work hides under the ticks (measured: 8192
    // envs, 1 round, fused 0.097 ms vs 0.13 ms).  With many rounds per CU (65536 envs) the reset
    // image and the reset role's registers cost every tick workgroup occupancy, so the reset work
    // runs as its own short launch (0.54 ms vs 0.59 ms).  zs_launch.fused forces either.
    StepLayout L = step_layout(s, ov, s.lanes_per_env, true);
    // 8 lanes per env when 16 would take the fused launch past one resident round and 8 take fewer rounds
    // (C3 on one MI355X: 16 384 envs, G = 16 two rounds 133.6 M env-steps/s, G = 8 one round 148.8 M;
    // 24 576 envs fused, G = 16 140.3 M, G = 8 143.5 M; 8 192 envs stay at G = 16, one round either way;
    // profiles/r05c_mid_sizes.log)
    if (L.G == 16 && s.lanes_per_env <= 0 && s.E <= 16 && L.resident < L.want) {
        const StepLayout L8 = step_layout(s, ov, 8, true);
        if (L8.rounds() < L.rounds()) L = L8;
    }
    if (L.G) {
        // up to two resident rounds the fused launch still wins: the side-stream reset work outlasts the tick
        // (C3 16 384 envs: k_tick 38 us, k_reset 43 us) and the fused launch hides it under the ticks (C3 on one
        // MI355X, fused against side stream: 12 288 envs 137.2 / 129.5 M, 16 384 133.1 / 123.7, 32 768 155.3 /
        // 153.6, 49 152 165.1 / 165.5, 65 536 172.5 / 182.0; C5 16 384 153.7 / 148.3, 32 768 186.6 / 199.3;
        // profiles/r05c_mid_sizes.log)
        p.fused = ov.fused ? ov.fused > 0 : 2 * L.resident >= L.want;
        p.tick_waves = ZS_FUSED_WAVES;
        // the fused launch loads its window's first 4G words with its first load round (zs_tick.hpp EARLY): a
        // window that size costs no round trip, and the lanes' draws then reload it less often
        if (p.fused && ov.rw_need <= 0) L.rw_step = std::min(L.rw_cap, std::max(L.rw_step, 4 * L.G));
        if (!p.fused) L = step_layout(s, ov, s.lanes_per_env, false);
    }
    if (!L.G) {
        p.error = "entity table / map too large for the LDS image of one env";
        return p;
    }
    if (!p.fused) {
        // k_tick's register budget: 5 waves per SIMD (96 VGPRs, 20 B of scratch per lane) unless 6 (80
        // VGPRs, 52 B of scratch on the leader's paths) saves a round of resident workgroups.  Measured
        // on one MI355X: C3 tick 95.6 -> 91.9 us and C4 185 -> 179 us at 5; C5 (16 384 workgroups:
        // 2.7 rounds at 6 waves, 3.2 at 5) 167 -> 178 us.  zs_launch.tick_waves forces either.
        const int wgs = (s.N + 64 / L.G - 1) / (64 / L.G);
        const int lres = std::max(1, 160 * 1024 / L.lds);
        auto rounds = [&](int w) {
            const int r = std::min(lres, 4 * w);
            return (wgs + 256 * r - 1) / (256 * r);
        };
        p.tick_waves = rounds(5) <= rounds(6) ? 5 : 6;
        if (ov.tick_waves > 0) p.tick_waves = ov.tick_waves == 5 ? 5 : 6;
        L.resident = std::min(L.resident, 4 * p.tick_waves);
    }
    p.G = L.G, p.lds = L.lds, p.resident = L.resident, p.want = L.want;
    p.rw_cap = L.rw_cap, p.rw_step = L.rw_step, p.cand_cap = L.cand_cap, p.lists_cap = L.lists_cap;
    // the reset launch stages the static spawn lists whenever they fit (no serial global loads in
    // its candidate filters); a fused launch shares the tick's choice
    p.rlists_cap = p.lists_cap;
    if (!p.fused && s.nps + s.nzs <= 4096 && reset_lds_bytes(s.E, s.DW, s.ncand, s.nps + s.nzs, s.obs_bytes) <= 64 * 1024 &&
        ov.reset_lists >= 0)
        p.rlists_cap = s.nps + s.nzs;
    p.reset_lds = reset_lds_bytes(s.E, s.DW, s.ncand, p.rlists_cap, s.obs_bytes);
    // side-stream reset work (unfused steps; zs_launch.reset_stream keeps it on the caller's stream)
    p.side_stream = !p.fused && ov.reset_stream >= 0;
    // fused: the first n_reset workgroups rebuild the envs of the pending list (ended at the previous
    // call) while the others tick every other env; the two sets of envs are disjoint
    p.n_reset = p.fused ? step_reset_wgs(s, ov) : 0;
    // enough one-wave workgroups that a step's resets (~850 at 65536 envs, bridge64) run in one round
    p.reset_grid_list = std::min(s.N, ov.reset_grid > 0 ? (int)ov.reset_grid : 2048);
    p.reset_grid_mask = std::min(s.N, 4096);
    // enough one-wave workgroups for a step's respawns in one pass (C4: 2048 -> 8192 took the launch
    // from 88 to 70 us; workgroups past the list's end exit at once)
    p.respawn_grid = std::min(s.N, ov.respawn_grid > 0 ? (int)ov.respawn_grid : 8192);
    return p;
}
