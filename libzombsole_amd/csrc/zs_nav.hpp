// zs_nav.hpp — k_nav: path-distance fields, a breadth-first search per env on the device.  The definition is stated
// here once, as rule functions a host compiler builds too (tests/nav_host.cpp); the kernel below them needs HIP.
//
// Free cells and distances.  A cell is free when it is inside the map and holds no present obstacle, whatever the
// obstacle's life (the rule of the entity observation's rays: cellmap[c] < 0, or the obstacle's bit in obst_present is
// clear).  Entities never block.  A field is the 4-connected BFS distance over free cells from a set of source cells,
// counted in moves; a source cell that is not free is not a source.
//
// Fields.  ZS_NAV_OBJECTIVE (bit 0): the sources are the map's objective cells (there may be none).  ZS_NAV_ZOMBIES
// (bit 1): the cells of the present zombie slots (s >= A + P).  `fields` is a bitmask of the two, F its popcount; the
// fields are emitted in ascending bit order.
//
// Distance cap.  1 <= max_dist <= ZS_NAV_MAX_DIST (32766): the search stops after that many levels.  A cell not reached
// within the cap is unreachable, as are blocked cells and cells outside the map.
//
// Per-agent rows: int16 [N][A][F][8], the buffer 8-byte aligned.  Word 0 is the distance at the agent's cell, words
// 1..4 the distances at the cells the discrete moves k = 0..3 lead to ((0,1), (-1,0), (0,-1), (1,0), the order of
// ent_dir_dx/dy), -1 where unreachable, blocked or outside the map.  Word 5 is the smallest k whose neighbour distance
// is the minimum over the reachable neighbours, word 6 the smallest k at their maximum, both -1 when no neighbour is
// reachable.  Word 7 holds flags: bit 0 the agent is present, bit 1 its own cell is a source.  An agent that is not
// present has an all-zero row (flags bit 0 tells it from "distance 0").
//
// Full field: uint16 [n][H][W] for a list of envs and one field, 0xFFFF = unreachable or blocked.
//
// An env pending its reset shows its terminal world, as every other observation does.
//
// Mapping.  One wave per env; 4, 2 or 1 envs per workgroup so that the workgroup's LDS image stays within 64 KiB
// (nav_plan).  An env's image holds row bitmaps of H x WW words, WW = ceil(W / 32), bit x & 31 of word y * WW + x / 32
// being cell (x, y): `free`, and per field `visited` and two `frontier` buffers; there is no per-cell distance array.
// A level is next = (frontier shifted left | shifted right, with the carries across the words of a row | the row above
// | the row below) & free & ~visited.  The lanes stride the image's words (so a 70 x 1 strip's three words and a
// 128 x 128 map's 512 are spread alike); a lane's first word keeps its free and visited bits in registers.  Both fields
// advance in the same loop and share its one wave barrier per level.  The 5 A query cells of the rows (own cell and four
// neighbours per agent) are fixed before the loop; at each level the lane that owns a query tests its bit in `next`
// and records the level.  A field stops when its frontier is empty or (rows only) all its queries are answered; the
// loop ends when every field has stopped, and its trip count is capped in code at min(max_dist, W * H).
// The full field's lanes store the level of each newly visited bit straight to global memory and the cells never
// visited get 0xFFFF after the loop, so every cell of a frame is stored exactly once.
#pragma once
#include <stdint.h>

#include "../../include/zombsole_mi355x.h"
#include "zs_step_plan.hpp"  // ZS_HD

#define ZS_NAV_ROW_WORDS 8
#define ZS_NAV_NFIELDS 2
#define ZS_NAV_LDS_LIMIT 65536  // a workgroup's LDS image, bytes
#define ZS_NAV_UNREACHED 0xFFFFu
// flags of a row (word 7)
#define ZS_NAV_PRESENT 1
#define ZS_NAV_ON_SOURCE 2

ZS_HD inline bool nav_fields_ok(int fields) { return fields >= 1 && fields <= (ZS_NAV_OBJECTIVE | ZS_NAV_ZOMBIES); }
ZS_HD inline bool nav_field_ok(int field) { return field == ZS_NAV_OBJECTIVE || field == ZS_NAV_ZOMBIES; }
ZS_HD inline bool nav_max_dist_ok(int max_dist) { return max_dist >= 1 && max_dist <= ZS_NAV_MAX_DIST; }
ZS_HD inline int nav_nfields(int fields) { return (fields & 1) + ((fields >> 1) & 1); }
// the bit number (0 objective, 1 zombies) of the i-th field emitted
ZS_HD inline int nav_field_bit(int fields, int i) { return (fields & 1) ? i : 1; }

// the row bitmaps: words per row, the word and bit of cell (x, y), the bits of word w of a row that are cells
ZS_HD inline int nav_ww(int W) { return (W + 31) >> 5; }
ZS_HD inline int nav_word(int x, int y, int ww) { return y * ww + (x >> 5); }
ZS_HD inline uint32_t nav_bit(int x) { return 1u << (x & 31); }
ZS_HD inline uint32_t nav_row_mask(int w, int W) { return W - 32 * w >= 32 ? 0xffffffffu : (1u << (W - 32 * w)) - 1u; }
// one word of a level ahead of `& free & ~visited`: c the frontier word, l / r the words left and right of it in its row
// (0 at the row's ends), u / dn the words above and below (0 at the map's edges)
ZS_HD inline uint32_t nav_step_word(uint32_t c, uint32_t l, uint32_t r, uint32_t u, uint32_t dn) {
    return (c << 1) | (l >> 31) | (c >> 1) | (r << 31) | u | dn;
}
// a cell with this word of `free` is a source only when it is free
ZS_HD inline bool nav_source_ok(uint32_t free_word, int x) { return (free_word & nav_bit(x)) != 0; }
// the level loop's trip count: no shortest path has W * H moves
ZS_HD inline int nav_trip_cap(int max_dist, int W, int H) {
    const int64_t cells = (int64_t)W * H;
    return (int64_t)max_dist < cells ? max_dist : (int)cells;
}
ZS_HD inline int nav_dir_dx(int k) { return k == 1 ? -1 : k == 3 ? 1 : 0; }
ZS_HD inline int nav_dir_dy(int k) { return k == 0 ? 1 : k == 2 ? -1 : 0; }
// words 5 and 6 of a row from the four neighbour distances (-1: not reachable)
ZS_HD inline int nav_best_dir(const int d[4], bool want_max) {
    int best = -1;
    for (int k = 0; k < 4; k++)
        if (d[k] >= 0 && (best < 0 || (want_max ? d[k] > d[best] : d[k] < d[best]))) best = k;
    return best;
}
ZS_HD inline int nav_flags(bool present, int d0) { return (present ? ZS_NAV_PRESENT : 0) | (present && d0 == 0 ? ZS_NAV_ON_SOURCE : 0); }
ZS_HD inline uint64_t nav_pack4(int w0, int w1, int w2, int w3) {
    return (uint64_t)(uint16_t)w0 | ((uint64_t)(uint16_t)w1 << 16) | ((uint64_t)(uint16_t)w2 << 32) | ((uint64_t)(uint16_t)w3 << 48);
}
// a row as the 16 bytes stored for it: d0 the distance at the agent's cell, d[k] at the neighbour of move k
ZS_HD inline void nav_row(bool present, int d0, const int d[4], uint64_t out[2]) {
    if (!present) {
        out[0] = out[1] = 0;
        return;
    }
    out[0] = nav_pack4(d0, d[0], d[1], d[2]);
    out[1] = nav_pack4(d[3], nav_best_dir(d, false), nav_best_dir(d, true), nav_flags(true, d0));
}

// The launch plan.  An env's image: 1 + 3 * ZS_NAV_NFIELDS bitmaps of nw words, then the 5 A query cells (int32) and
// their distances (int16, one row per field), rounded up to 16 bytes.  Always planned for both fields, so one plan
// serves every call of a handle.  ok = 0: a single env's image is past ZS_NAV_LDS_LIMIT.
struct NavPlan {
    int ok, ww, nw, nq, env_bytes, envs_per_wg, block, lds_bytes;
};
ZS_HD inline int64_t nav_env_bytes(int W, int H, int A) {
    const int64_t nw = (int64_t)H * nav_ww(W), nq = 5 * (int64_t)A;
    return (4 * nw * (1 + 3 * ZS_NAV_NFIELDS) + (4 + 2 * ZS_NAV_NFIELDS) * nq + 15) & ~(int64_t)15;
}
ZS_HD inline NavPlan nav_plan(int W, int H, int A) {
    NavPlan p = {};
    p.ww = nav_ww(W);
    const int64_t nw = (int64_t)H * p.ww, nq = 5 * (int64_t)A;
    const int64_t bytes = nav_env_bytes(W, H, A);
    if (bytes > ZS_NAV_LDS_LIMIT) return p;
    p.ok = 1;
    p.nw = (int)nw;
    p.nq = (int)nq;
    p.env_bytes = (int)bytes;
    p.envs_per_wg = 4 * bytes <= ZS_NAV_LDS_LIMIT ? 4 : 2 * bytes <= ZS_NAV_LDS_LIMIT ? 2 : 1;
    p.block = 64 * p.envs_per_wg;
    p.lds_bytes = p.envs_per_wg * p.env_bytes;
    return p;
}
// workgroups of a launch over n envs (or n frames)
ZS_HD inline unsigned nav_grid(const NavPlan& p, int n) { return (unsigned)((n + p.envs_per_wg - 1) / p.envs_per_wg); }

// the kernel's own argument beside the Dev (which has no field for the feature)
struct NavArgs {
    int fields, max_dist, nobj;
    const int32_t* obj_xy;  // [nobj] x | y << 16, map-file order (the handle's d_obj_xy)
    NavPlan plan;
};

// the kernel is defined by the unit that sets ZS_DEFINE_NAV_KERNEL (k_nav.hip)
#ifdef ZS_DEFINE_NAV_KERNEL
#include "zs_device.hpp"

// F fields per launch; FULL: frames of the listed envs (one field) instead of the per-agent rows
template <int F, bool FULL>
__global__ __launch_bounds__(256) void k_nav(Dev d, NavArgs g, const uint8_t* __restrict__ env_mask,
                                             const int32_t* __restrict__ env_idx, int n, void* __restrict__ out) {
    extern __shared__ uint32_t nav_lds[];
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    const int k = __builtin_amdgcn_readfirstlane(blockIdx.x * g.plan.envs_per_wg + wv);
    int e = k;
    if (FULL) {
        if (k >= n) return;
        if (env_idx) e = __builtin_amdgcn_readfirstlane(env_idx[k]);
        if (e < 0 || e >= d.N) return;
    } else {
        if (e >= d.N) return;
        if (env_mask && !env_mask[e]) return;
    }
    const int W = d.W, H = d.H, A = d.A, np = d.A + d.P, E = d.E;
    const int WW = g.plan.ww, NW = g.plan.nw, NQ = g.plan.nq;
    const size_t row = (size_t)e * E;
    const int32_t* __restrict__ pos = d.pos + row;
    const uint8_t* __restrict__ present = d.present + row;
    const uint32_t* __restrict__ opres = d.obst_present + (size_t)e * d.OW;
    // the env's image
    uint32_t* img = nav_lds + (size_t)wv * (g.plan.env_bytes >> 2);
    uint32_t* lfree = img;
    uint32_t* lvis[F];
    uint32_t* lfr[F][2];
#pragma unroll
    for (int f = 0; f < F; f++) {
        lvis[f] = img + (size_t)NW * (1 + 3 * f);
        lfr[f][0] = img + (size_t)NW * (2 + 3 * f);
        lfr[f][1] = img + (size_t)NW * (3 + 3 * f);
    }
    int32_t* qcell = (int32_t*)(img + (size_t)NW * (1 + 3 * ZS_NAV_NFIELDS));
    int16_t* qdist = (int16_t*)(qcell + NQ);  // [F][NQ]
    // a lane's words are lane, lane + 64, ...: their (row, word of the row) without a division per word
    const int r0 = lane / WW, w0 = lane - r0 * WW, rstep = 64 / WW, wstep = 64 - rstep * WW;
#define NAV_WORDS(i, r, w) \
    for (int i = lane, r = r0, w = w0; i < NW; i += 64, r += rstep + (w + wstep >= WW ? 1 : 0), w += wstep - (w + wstep >= WW ? WW : 0))
    // 1) every cell of the map free, nothing visited
    NAV_WORDS(i, r, w) {
        lfree[i] = nav_row_mask(w, W);
#pragma unroll
        for (int f = 0; f < F; f++) lfr[f][0][i] = 0;
    }
    wave_sync();
    // 2) the present obstacles' cells are not free
    for (int o = lane; o < d.O; o += 64) {
        if (!((opres[o >> 5] >> (o & 31)) & 1u)) continue;
        const int32_t xy = d.obst_xy[o];
        const int x = unpack_x(xy), y = unpack_y(xy);
        if (x >= 0 && x < W && y >= 0 && y < H) atomicAnd(&lfree[nav_word(x, y, WW)], ~nav_bit(x));
    }
    wave_sync();
    // 3) the sources: level 0 of every field
#pragma unroll
    for (int f = 0; f < F; f++) {
        const bool zombies = nav_field_bit(g.fields, f) == 1;
        const int cnt = zombies ? E - np : g.nobj;
        for (int i = lane; i < cnt; i += 64) {
            if (zombies && !present[np + i]) continue;
            const int32_t xy = zombies ? pos[np + i] : g.obj_xy[i];
            const int x = unpack_x(xy), y = unpack_y(xy);
            if (x < 0 || x >= W || y < 0 || y >= H) continue;
            const int wi = nav_word(x, y, WW);
            if (nav_source_ok(lfree[wi], x)) atomicOr(&lfr[f][0][wi], nav_bit(x));
        }
    }
    wave_sync();
    // a lane's first word keeps its free and visited bits in registers
    const uint32_t free0 = lane < NW ? lfree[lane] : 0u;
    uint32_t vis0[F];
    uint16_t* frame = (uint16_t*)out + (size_t)k * W * H;  // FULL
#pragma unroll
    for (int f = 0; f < F; f++) {
        vis0[f] = lane < NW ? lfr[f][0][lane] : 0u;
        NAV_WORDS(i, r, w) {
            uint32_t m = lfr[f][0][i];
            if (i != lane) lvis[f][i] = m;
            if (FULL)
                for (; m; m &= m - 1) frame[(size_t)r * W + 32 * w + __builtin_ctz(m)] = 0;
        }
    }
    // 4) the rows' queries: own cell and four neighbours per agent; a cell that is not free is answered (-1) already
    int pend[F];
#pragma unroll
    for (int f = 0; f < F; f++) pend[f] = 0;
    if (!FULL) {
        for (int q0 = 0; q0 < NQ; q0 += 64) {
            const int q = q0 + lane;
            int cell = -1;
            if (q < NQ) {
                const int a = q / 5, j = q - 5 * a;
                if (present[a]) {
                    const int32_t ap = pos[a];
                    const int x = unpack_x(ap) + (j ? nav_dir_dx(j - 1) : 0), y = unpack_y(ap) + (j ? nav_dir_dy(j - 1) : 0);
                    if (x >= 0 && x < W && y >= 0 && y < H && (lfree[nav_word(x, y, WW)] & nav_bit(x)))
                        cell = (nav_word(x, y, WW) << 5) | (x & 31);
                }
                qcell[q] = cell;
            }
#pragma unroll
            for (int f = 0; f < F; f++) {
                const bool at0 = cell >= 0 && ((lfr[f][0][cell >> 5] >> (cell & 31)) & 1u);
                if (q < NQ) qdist[f * NQ + q] = at0 ? 0 : -1;
                pend[f] += __popcll(__ballot(cell >= 0 && !at0));
            }
        }
    }
    wave_sync();
    // 5) the levels.  The trip count is bounded by construction, whatever the frontiers do
    bool act[F];
#pragma unroll
    for (int f = 0; f < F; f++) act[f] = FULL || pend[f] > 0;
    const int cap = nav_trip_cap(g.max_dist, W, H);
    int cur = 0;
    for (int level = 1; level <= cap; level++) {
        bool any = false;
#pragma unroll
        for (int f = 0; f < F; f++) any |= act[f];
        if (!any) break;
        uint32_t grew[F];
#pragma unroll
        for (int f = 0; f < F; f++) {
            grew[f] = 0;
            if (!act[f]) continue;  // wave-uniform
            const uint32_t* fr = lfr[f][cur];
            uint32_t* nx = lfr[f][cur ^ 1];
            NAV_WORDS(i, r, w) {
                const uint32_t l = w > 0 ? fr[i - 1] : 0u, rt = w + 1 < WW ? fr[i + 1] : 0u;
                const uint32_t u = r > 0 ? fr[i - WW] : 0u, dn = r + 1 < H ? fr[i + WW] : 0u;
                const uint32_t vw = i == lane ? vis0[f] : lvis[f][i];
                uint32_t m = nav_step_word(fr[i], l, rt, u, dn) & (i == lane ? free0 : lfree[i]) & ~vw;
                nx[i] = m;
                if (i == lane)
                    vis0[f] = vw | m;
                else
                    lvis[f][i] = vw | m;
                grew[f] |= m;
                if (FULL)
                    for (; m; m &= m - 1) frame[(size_t)r * W + 32 * w + __builtin_ctz(m)] = (uint16_t)level;
            }
        }
        wave_sync();
#pragma unroll
        for (int f = 0; f < F; f++) {
            if (!act[f]) continue;
            const bool more = __ballot(grew[f] != 0) != 0;
            if (!FULL) {
                const uint32_t* nx = lfr[f][cur ^ 1];
                for (int q0 = 0; q0 < NQ; q0 += 64) {
                    const int q = q0 + lane;
                    bool found = false;
                    if (q < NQ) {
                        const int cell = qcell[q];
                        if (cell >= 0 && qdist[f * NQ + q] < 0 && ((nx[cell >> 5] >> (cell & 31)) & 1u)) {
                            qdist[f * NQ + q] = (int16_t)level;
                            found = true;
                        }
                    }
                    pend[f] -= __popcll(__ballot(found));
                }
            }
            act[f] = more && (FULL || pend[f] > 0);
        }
        cur ^= 1;
    }
    wave_sync();
    // 6) the output
    if (FULL) {
        NAV_WORDS(i, r, w) {
            uint32_t m = ~(i == lane ? vis0[0] : lvis[0][i]) & nav_row_mask(w, W);
            for (; m; m &= m - 1) frame[(size_t)r * W + 32 * w + __builtin_ctz(m)] = (uint16_t)ZS_NAV_UNREACHED;
        }
    } else {
        uint64_t* __restrict__ orow = (uint64_t*)out + (size_t)e * A * F * 2;
        for (int t = lane; t < A * F; t += 64) {
            const int a = t / F, f = t - a * F;
            const int16_t* qd = qdist + f * NQ + 5 * a;
            const int dd[4] = {qd[1], qd[2], qd[3], qd[4]};
            uint64_t v[2];
            nav_row(present[a] != 0, qd[0], dd, v);
            orow[2 * t] = v[0];
            orow[2 * t + 1] = v[1];
        }
    }
#undef NAV_WORDS
}
#endif
