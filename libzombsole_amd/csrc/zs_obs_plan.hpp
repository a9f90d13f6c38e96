// zs_obs_plan.hpp — which observation kernel a handle launches, and with what grid, block and LDS size.
//
// The engine has six observation kernels (zs_obs.hpp).  obs_plan() picks, from the config's integers and
// the zs_launch overrides alone, the kernel of an unmasked launch (a step's, a full reset's) and of a
// masked one (zs_reset / zs_observe with an env mask), together with the LDS byte counts and tunables
// they are sized by.  Nothing here needs HIP: the kernels, the engine and a plain host compiler (the
// plan's CPU test, tests/obs_plan_dump.cpp) include the same file.
#pragma once
#include <stdint.h>

#include "../../include/zombsole_mi355x.h"

#if defined(__HIPCC__)
#define ZS_HD __host__ __device__
#else
#define ZS_HD
#endif

// ---------------------------------------------------------------------------
// tunables of the kernels that their launch geometry and LDS sizes depend on
// ---------------------------------------------------------------------------
#define OBS_PF_D 2   // prefetched dead-body words per lane   (DW <= 128: maps up to 4096 cells)
#define OBS_PF_H 8   // prefetched obstacle HP words per lane (O <= 512)

// k_obs_patch's waves per workgroup: eight share one copy of the static tables (16 KB at bridge64), two
// workgroups per CU
#define PATCH_WPG 8

// k_obs_ring's encoder / writer waves and ring slots
#ifndef RING_ENC
#define RING_ENC 12
#endif
#ifndef RING_WRT
#define RING_WRT 3  // measured on one MI355X at C3 (2 runs each): 3 writers 267.7 / 269.0 us, 4: 273.4 / 274.4, 2: 282.8 / 283.6
#endif
#ifndef RING_SLOTS
#define RING_SLOTS 8
#endif

// k_obs_pbring's encoder / writer waves
// measured at C4 on one MI355X (2 runs each, profiles/r04_ab_c4_*.log): 9 / 3 159.5-159.9 us, 8 / 4 164.5,
// 8 / 3 170, 5 / 3 184-202, 12 / 3 (4 slots) 201; with the 63-lane cell walk 9 / 3 158.3-159.7, 10 / 2
// 153.6-155.0 (profiles/r04_ab_c4_enc.log)
#ifndef BRING_ENC
#define BRING_ENC 10
#endif
#ifndef BRING_WRT
#define BRING_WRT 2
#endif
#define BRING_D 8  // dead-body words per lane (DW <= 512)
#define BRING_O 2  // obstacle-present words per lane (OW <= 128, O <= 4096)

enum { OBSK_OBS = 0, OBSK_GATHER, OBSK_PIPE, OBSK_PATCH, OBSK_RING, OBSK_BRING };

// ---------------------------------------------------------------------------
// sizes
// ---------------------------------------------------------------------------
// bytes of one output element
ZS_HD constexpr int obs_tsize(int dtype) { return dtype == ZS_DTYPE_I64 ? 8 : dtype == ZS_DTYPE_I32 ? 4 : 2; }

// observations per env
ZS_HD inline int obs_count(int scope, int reward_mode, int A) {
    return scope == ZS_OBS_WORLD ? 1 : (reward_mode == ZS_REWARD_MULTI ? A : 1);
}

// one env's observation image in LDS (zs_obs.hpp)
struct ObsLayout {
    int win;     // window-map bytes (0: no window map, entities found by a per-cell scan)
    int off_pos, off_life, off_cw, off_dead, off_opres, off_hp;
    int hp_cap;  // obstacle HP staged in LDS (else read from HBM)
    int bytes;   // one env's image
};

ZS_HD inline ObsLayout obs_layout(int nobs, int plane, int E, int DW, int OW, int O, bool winmap, bool stage_hp) {
    ObsLayout L;
    int o = 0;
    L.win = winmap ? ((nobs * plane + 15) / 16) * 16 : 0;
    o += L.win;
    L.off_pos = o;
    o += E * 4;
    o = ((o + 7) / 8) * 8;  // the store-stream kernels read {code word, life} pairs from off_life as 8 B
    L.off_life = o;
    o += E * 4;
    L.off_cw = o;
    o += E * 4;
    L.off_dead = o;
    o += DW * 4;
    L.off_opres = o;
    o += OW * 4;
    L.off_hp = o;
    L.hp_cap = stage_hp ? O : 0;
    o += L.hp_cap * 4;
    L.bytes = ((o + 15) / 16) * 16;
    return L;
}

// staging bytes: nblk consecutive channels blocks (one agent's, or every agent's of an env), shifted
// by the destination's 16-B phase in elements
ZS_HD constexpr int obs_stage_slot_bytes(int tsize, int nblk = 1) {
    return (((nblk * 3 * 441 + 16 / tsize) * (tsize == 8 ? 4 : tsize) + 15) / 16) * 16;
}

// k_obs_patch
ZS_HD constexpr int patch_list_bytes(int O) { return ((O * 8 + 15) / 16) * 16; }
// static LDS of a workgroup: the padded table and the obstacles' packed cells
ZS_HD constexpr int patch_static_bytes(int opad_n, int O) {
    return ((opad_n * 2 + 15) / 16) * 16 + ((O * 4 + 15) / 16) * 16 + 256;
}
// per-env list of dead-body cells (without a map obstacle) the encoder patches; an env with more takes
// the per-word scan
#define PATCH_DEAD_CAP 256
ZS_HD constexpr int patch_enc_bytes(int DW, int O) {  // dead words, present words, dead list, list
    return ((DW * 4 + 15) / 16) * 16 + 256 + 4 * PATCH_DEAD_CAP + 16 + patch_list_bytes(O);
}
ZS_HD constexpr int patch_wave_bytes(int DW, int O, int slot) { return patch_enc_bytes(DW, O) + slot; }

// k_obs_ring.  Envs per ring unit: two when one env's block ends off a 16-B boundary and two end on one
// (C5's int16 10 584-B envs): a unit is then one aligned, contiguous stream, with no partial 16-B chunk
// shared by two writers.
ZS_HD constexpr int ring_pair(int tsize, int nobs) {
    return (nobs * 3 * 441 * tsize) % 16 != 0 && (2 * nobs * 3 * 441 * tsize) % 16 == 0 ? 2 : 1;
}
ZS_HD constexpr int ring_lds_bytes(int stat_bytes, int img_bytes, int tsize, int nobs) {
    return stat_bytes + RING_ENC * img_bytes +
           (RING_SLOTS / ring_pair(tsize, nobs)) * obs_stage_slot_bytes(tsize, nobs * ring_pair(tsize, nobs)) +
           16 * RING_SLOTS;
}

// k_obs_pbring
ZS_HD constexpr int bring_unit_bytes(int tsize, int nobs) {
    return obs_stage_slot_bytes(tsize, nobs * ring_pair(tsize, nobs));
}
ZS_HD constexpr int pbring_enc_bytes(int DW, int OW) { return ((DW * 4 + 15) / 16) * 16 + ((OW * 4 + 15) / 16) * 16; }
ZS_HD constexpr int pbring_fixed_bytes(int DW, int OW) { return 16 * DW + BRING_ENC * pbring_enc_bytes(DW, OW) + 128; }
ZS_HD constexpr int pbring_slots(int DW, int OW, int tsize, int nobs, int budget) {
    return (budget - pbring_fixed_bytes(DW, OW)) / bring_unit_bytes(tsize, nobs) < 8 / ring_pair(tsize, nobs)
               ? (budget - pbring_fixed_bytes(DW, OW)) / bring_unit_bytes(tsize, nobs)
               : 8 / ring_pair(tsize, nobs);
}

// ---------------------------------------------------------------------------
// the plan
// ---------------------------------------------------------------------------
// the integers the choice reads (zs_create fills them from the config; Dev's names)
struct ObsShape {
    int N, W, H, O, OW, DW, E, A;
    int scope, enc, obs_w, dtype, reward_mode;
    int opad_n;         // cells of k_obs_patch's padded table
    int rank_order;     // the map's obstacles are in row-major order (index = rank of the cell)
    int defer_respawn;  // zombie respawn after the tick (k_respawn)
};

// one resolved launch: everything but the caller's buffers and env range (zs_launch.hpp ObsLaunch)
struct ObsKernel {
    int kind;         // OBSK_*
    int nobs;         // 1, 2 or 4 (k_obs takes any count and ignores this: 0 unless k_obs_pipe's shape applies)
    int patched;      // k_obs_ring: padded-table encoders
    int block;
    int lds;
    ObsLayout L;
    int stat;         // k_obs: static words staged; k_obs_gather: static words from LDS tables
    int us;           // k_obs_pbring: unit slots of the ring
    int envs_per_wg;  // grid = ceil(envs / envs_per_wg) ...
    int max_wgs;      // ... capped at max_wgs (0: uncapped; the persistent kernels walk the rest)
};

struct ObsPlan {
    ObsKernel full;      // every env of the handle (mask == NULL)
    ObsKernel masked;    // the envs of a mask
    int obs_stat;        // Dev::obs_stat
    ObsLayout step_img;  // Dev::obsl
    int fobs;            // Dev::fobs: the step launch writes the observations itself
    const char* error;   // non-null: no observation image fits
};

inline const char* obs_kernel_name(int kind) {
    return kind == OBSK_RING    ? "k_obs_ring"
           : kind == OBSK_PATCH ? "k_obs_patch"
           : kind == OBSK_PIPE  ? "k_obs_pipe"
           : kind == OBSK_BRING ? "k_obs_pbring"
           : kind == OBSK_GATHER ? "k_obs_gather" : "k_obs";
}

// "patched" / "select" for the kernels that have both encoders (k_obs_ring), "" otherwise
inline const char* obs_encoders_name(const ObsKernel& k) { return k.kind != OBSK_RING ? "" : k.patched ? "patched" : "select"; }

inline unsigned obs_grid(const ObsKernel& k, int n_envs) {
    const int g = (n_envs + k.envs_per_wg - 1) / k.envs_per_wg;
    return (unsigned)(k.max_wgs && g > k.max_wgs ? k.max_wgs : g);
}

// lds_ok(kind, nobs, patched, bytes, ctx): the kernel instantiation may be launched with that much
// dynamic LDS (the engine raises the kernel's limit there, k_obs_t.hip obs_lds_attr)
inline ObsPlan obs_plan(const ObsShape& s, const zs_launch& ov, bool (*lds_ok)(int kind, int nobs, int patched, int bytes, void* ctx),
                        void* ctx) {
    ObsPlan p = {};
    // observation images: k_obs (four envs per workgroup when their images fit 64 KiB, else one;
    // window map and staged HP while one image fits 32 KiB) and, when the step launch writes the
    // observations itself (fobs), one env's image inside the tick / reset LDS (HP staged when the
    // image still fits the MT twist buffer it aliases).  zs_launch.obs_win forces the per-cell
    // entity scan (parity tests of that path).
    const bool world = s.scope == ZS_OBS_WORLD;
    const int nobs = obs_count(s.scope, s.reward_mode, s.A);
    const int plane = world ? s.W * s.H : s.obs_w * s.obs_w;
    const int ts = obs_tsize(s.dtype);
    const bool win = ov.obs_win >= 0;
    ObsLayout L = obs_layout(nobs, plane, s.E, s.DW, s.OW, s.O, win, true);
    if (L.bytes > 32 * 1024) L = obs_layout(nobs, plane, s.E, s.DW, s.OW, s.O, win, false);
    if (L.bytes > 32 * 1024) L = obs_layout(nobs, plane, s.E, s.DW, s.OW, s.O, false, false);
    if (L.bytes > 64 * 1024) {
        p.error = "map too large for the observation kernel's LDS image";
        return p;
    }
    // static tables (4 x DW words) beside the images: per k_obs workgroup, and inside the step
    // launch's image region; zs_launch.obs_stat forces the per-cell static words (parity tests)
    const int stat = (s.rank_order && s.DW <= 1024 && ov.obs_stat >= 0) ? 4 * s.DW : 0;
    const int wpg = stat * 4 + 4 * L.bytes <= 64 * 1024 ? 4 : 1;  // k_obs waves (envs) per workgroup
    // k_obs_pipe: surroundings of width 21, 1/2/4 observations, static tables, staged HP, window
    // map, every entity on its own lane, prefetch arrays large enough (zs_launch.obs_pipe disables)
    const bool pipe = !world && s.obs_w == 21 && (nobs == 1 || nobs == 2 || nobs == 4) && stat && L.hp_cap && L.win &&
                      s.O > 0 && s.E <= 64 && s.DW <= 64 * OBS_PF_D && s.O <= 64 * OBS_PF_H && s.OW <= 64 &&
                      stat * 4 + 4 * L.bytes <= 64 * 1024 && ov.obs_pipe >= 0;
    // the general kernel: one env per wave; also every masked launch unless k_obs_gather applies
    p.full = p.masked = ObsKernel{OBSK_OBS, pipe ? nobs : 0, 0, 64 * wpg, stat * 4 + wpg * L.bytes, L, stat, 0, wpg, 0};
    if (pipe) {
        // every env of the range, registered shape: the prefetching store stream.
        // two workgroups (8 waves) per CU: measured at 65536 envs, 0.350 ms per launch against 0.375
        // at 8 and 0.38 at 3-4 (a smaller set of env blocks in flight at once); one contiguous env
        // range per wave instead of the strided walk measured slower (0.383)
        int wgs = 160 * 1024 / (stat * 4 + 4 * L.bytes);
        wgs = wgs < 1 ? 1 : wgs > 2 ? 2 : wgs;
        if (ov.obs_wgs > 0) wgs = ov.obs_wgs < 32 ? (int)ov.obs_wgs : 32;
        p.full = ObsKernel{OBSK_PIPE, nobs, 0, 256, stat * 4 + 4 * L.bytes, L, 0, 0, 4, 256 * wgs};
    }
    // The LDS-staged 16-B store kernels (k_obs_patch, k_obs_ring; zs_obs.hpp) for k_obs_pipe's shape,
    // channels encoding.  They pay when every wave walks several envs (at 8192 envs, one env per wave,
    // k_obs_pipe's per-cell stores measured 33 vs 36 us): int64 blocks from 48 envs per CU (C3 on one
    // MI355X, k_obs_ring against k_obs_pipe: 12 288 envs 129.5 against 117.1 M env-steps/s, 16 384 123.7 /
    // 121.4, 24 576 140.1 / 134.8, 32 768 153.6 / 147.1; 8 192 138.9 against 143.9, 10 240 (fused) 150.9 /
    // 154.9; profiles/r05c_mid_sizes.log), narrower blocks at any count.  zs_launch.obs_lds = -1 keeps
    // k_obs_pipe, 1 takes them at any count.
    const bool staged = pipe && s.enc == ZS_ENC_CHANNELS && ov.obs_lds >= 0 &&
                        (ts < 8 || (long)s.N >= 48L * 256 || ov.obs_lds > 0);
    // k_obs_patch: k_obs_pipe's walk with the padded-table encoder and the staged flush (maps up to
    // 4095 x 4095, rows of the padded table in the workgroup's LDS).  zs_launch.obs_patch = -1 disables.
    bool patch = false;
    if (staged && s.OW <= 64 && (long)(s.W + 20) * 21 < 65536 && s.H < 4096) {
        const long pb = (long)patch_static_bytes(s.opad_n, s.O) +
                        PATCH_WPG * (long)patch_wave_bytes(s.DW, s.O, obs_stage_slot_bytes(ts));
        if (pb <= 160 * 1024 && ov.obs_patch >= 0 && lds_ok(OBSK_PATCH, nobs, 0, (int)pb, ctx)) {
            patch = true;
            int wgs = (int)(160 * 1024 / pb);  // workgroups (PATCH_WPG waves) per CU
            wgs = wgs < 1 ? 1 : wgs;
            if (ov.obs_wgs > 0) wgs = ov.obs_wgs < 32 ? (int)ov.obs_wgs : 32;
            p.full = ObsKernel{OBSK_PATCH, nobs, 0, 64 * PATCH_WPG, (int)pb, L, 0, 0, PATCH_WPG, 256 * wgs};
        }
    }
    // k_obs_ring (zs_obs.hpp): the staged flush with dedicated writer waves, one workgroup per CU.
    // Measured on one MI355X (2 runs each): C3 (int64) observations 292 / 280 -> 285 / 273 us against its
    // predecessor without writer waves; C5 (int16) even.  Default for int64 blocks; zs_launch.obs_ring
    // forces either.
    if (staged) {
        // the ring's encoders are k_obs_patch's when its tables fit (zs_launch.obs_ring_patch forces either)
        const bool patched = patch && ov.obs_ring_patch >= 0;
        const long rb = patched ? (long)ring_lds_bytes(patch_static_bytes(s.opad_n, s.O), patch_enc_bytes(s.DW, s.O), ts, nobs)
                                : (long)ring_lds_bytes(16 * s.DW, L.bytes, ts, nobs);
        const int rg = ov.obs_ring;
        // default for int64 blocks, and for int16 ones with the padded-table encoders (C5 on one MI355X,
        // 2 runs each: 215.2 / 216.5 us against k_obs_patch's 222.7 / 223.0)
        if (rb <= 160 * 1024 && (rg ? rg > 0 : ts == 8 || (patched && ts == 2)) &&
            lds_ok(OBSK_RING, nobs, patched ? 1 : 0, (int)rb, ctx))
            p.full = ObsKernel{OBSK_RING, nobs, patched ? 1 : 0, 64 * (RING_ENC + RING_WRT), (int)rb, L, 0, 0, ring_pair(ts, nobs), 256};
    }
    // k_obs_gather when the store-stream kernel does not apply (e.g. city128's 3689 obstacles): one env
    // per wave, four per workgroup, window-only static words and HP instead of per-env staging; masked
    // launches too.  zs_launch.obs_gather disables.
    if (!pipe && !world && s.obs_w == 21 && (nobs == 1 || nobs == 2 || nobs == 4) && ov.obs_gather >= 0) {
        const ObsLayout G = obs_layout(nobs, plane, s.E, s.DW, s.OW, s.O, true, false);
        if (4 * G.bytes <= 64 * 1024) {
            // static words from the LDS tables (rank order, as obs_stat) instead of a global load
            // round per window cell (zs_launch.obs_gather_stat)
            const int gstat = stat && 4 * G.bytes + 16 * s.DW <= 64 * 1024 && ov.obs_gather_stat >= 0;
            p.full = p.masked = ObsKernel{OBSK_GATHER, nobs, 0, 256, 4 * G.bytes + (gstat ? 16 * s.DW : 0), G, gstat, 0, 4, 0};
            // k_obs_pbring: k_obs_gather's window-only fetches as the encoders of a k_obs_ring-style ring, the
            // things written over the windows (C4 on one MI355X: observations 180-184 us with k_obs_gather, 151 us
            // with k_obs_pbring), when the dead-body and present rows fit the encoders' load rounds and two unit
            // slots fit beside the static tables and the encoder regions.  zs_launch.obs_ring = -1 keeps k_obs_gather.
            if (stat && s.enc == ZS_ENC_CHANNELS && s.E <= 64 && s.DW <= 64 * BRING_D && s.OW <= 64 * BRING_O &&
                ov.obs_ring >= 0) {
                const int usp = pbring_slots(s.DW, s.OW, ts, nobs, 160 * 1024);
                const long pbb = (long)pbring_fixed_bytes(s.DW, s.OW) + (long)usp * bring_unit_bytes(ts, nobs);
                if (usp >= 2 && lds_ok(OBSK_BRING, nobs, 1, (int)pbb, ctx))
                    p.full = ObsKernel{OBSK_BRING, nobs, 0, 64 * (BRING_ENC + BRING_WRT), (int)pbb, G, 0, usp, ring_pair(ts, nobs), 256};
            }
        }
    }
    // with the store-stream kernel available the observations are its job (measured faster than
    // writing them from the tick workgroups at both 8192 and 65536 envs); zs_launch.fobs forces them
    // into the step launch
    p.obs_stat = stat;
    p.step_img = L;
    p.fobs = L.bytes + 4 * stat <= 16 * 1024 && ov.fobs >= 0;
    if (pipe && ov.fobs <= 0) p.fobs = 0;
    if (s.defer_respawn) p.fobs = 0;  // the observations must see k_respawn's zombies
    return p;
}
