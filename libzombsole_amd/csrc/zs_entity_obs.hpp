// zs_entity_obs.hpp — k_entity_obs: the compact, per-agent entity observation.  The encoding is stated here once,
// as rule functions a host compiler builds too (tests/entity_obs_host.cpp); the kernel below them needs HIP.
//
// Output: int16 [N][A][ROW], ROW = 16 + 4 (KZ + KP) words (32 + 8 (KZ + KP) bytes), 1 <= KZ <= 16, 0 <= KP <= 16,
// the buffer 8-byte aligned.  Every value is an exact integer of the env's current world (the one its grid
// observation shows; an env pending its reset shows its terminal world).  A row, in words:
//   self       8: present (1), x, y, life, weapon code (ZS_WEAPON_*), weapon_r2, zombies present in the env,
//                 other agents and bots present
//   zombies    KZ x {dx, dy, life, flags}: the present zombie slots, ascending by the key (d2, slot), d2 = dx^2 + dy^2,
//                 dx, dy = the zombie's cell minus the agent's.  flags: bit 0 valid, bit 1 d2 <= weapon_r2 of the
//                 agent's weapon, bit 2 d2 == 1.  Rows past the present zombies are zero
//   players    KP x {dx, dy, life, flags}: the present agent and bot slots other than the agent itself, in the same
//                 order.  flags: bit 0 valid, bit 1 d2 <= 9 (HEALING_RANGE), bit 2 the slot is an agent and not a
//                 bot, bits 8..15 its weapon code
//   objective  4: {dx, dy, flags, n_objectives} of the nearest objective cell by (d2, map-file index).  flags: bit 0
//                 valid, bit 1 the agent stands on an objective
//   rays       4: towards (0,1), (-1,0), (0,-1), (1,0) (the discrete table's moves) the count of consecutive cells,
//                 starting next to the agent, that are inside the map and hold no present obstacle, whatever the
//                 obstacle's life; capped at ZS_ENT_RAY_CAP.  Entities do not stop a ray
// Lives and counts saturate to the int16 range.  An agent that is not present has an all-zero row.
//
// The tie-break among equidistant slots is the slot number, not the dict-order rank closest_in uses (zs_tick.hpp): the
// kernel then reads nothing but the observation-state arrays (pos, life, weapon, present, obstacle presence) and static
// tables, so it runs on a viewer handle after zs_obs_state_unpack, as k_action_mask does.  Among equidistant zombies
// row 0 therefore need not be the one attack_closest hits.
//
// The keys are compared as (d2, slot) pairs of int32: no bound on d2 (up to 2 * 16000^2 on the largest map) or on the
// slot count is assumed; the objective key is d2 << 32 | index in 64 bits.
//
// Mapping (as zs_mask.hpp): one wave per env, four envs per workgroup, lanes striding the E entity slots with pass 0
// in registers.  Per agent the lanes put their slots' d2 into the wave's LDS row (absent slots and the agent itself a
// sentinel); the keys are distinct, so a slot's rank in its class is the count of smaller keys of that class, and a
// lane whose slot ranks below K stores its own 8-byte row at that rank.  Lanes between the class count and K store
// the zero rows.  No sort, no reduction tree; the nearest objective is one wave minimum of 64-bit keys.  The rays run
// ahead of the agent loop, one lane per (agent, direction), sixteen agents a round.
#pragma once
#include <stdint.h>

#include "../../include/zombsole_mi355x.h"
#include "zs_step_plan.hpp"  // ZS_HD

#define ZS_ENT_BLOCK 256
#define ZS_ENT_ENVS (ZS_ENT_BLOCK / 64)
#define ZS_ENT_RAY_CAP 16
#define ZS_ENT_HEAL_R2 9   // HEALING_RANGE = 3 (core.py:8)
#define ZS_ENT_KMAX 16
#define ZS_ENT_SLOTS 256   // the LDS row of a wave: E <= 254 (zs_create)
#define ZS_ENT_ABSENT 0x7fffffff  // the d2 of a slot that takes no part (a real d2 is below 2^30)

// flags of a zombie row, of a player row, of the objective block
#define ZS_ENT_VALID 1
#define ZS_ENT_IN_RANGE 2
#define ZS_ENT_ADJACENT 4   // zombie rows
#define ZS_ENT_IS_AGENT 4   // player rows
#define ZS_ENT_ON_OBJECTIVE 2

// word offsets of a row's blocks
struct EntLayout {
    int row_words, self, zombies, players, objective, rays;
};
ZS_HD inline bool ent_k_ok(int kz, int kp) { return kz >= 1 && kz <= ZS_ENT_KMAX && kp >= 0 && kp <= ZS_ENT_KMAX; }
ZS_HD inline EntLayout ent_layout(int kz, int kp) {
    EntLayout L;
    L.self = 0;
    L.zombies = 8;
    L.players = 8 + 4 * kz;
    L.objective = 8 + 4 * (kz + kp);
    L.rays = L.objective + 4;
    L.row_words = L.rays + 4;
    return L;
}

// workgroups of a launch over n envs
static inline unsigned zs_ent_grid(int n) { return (unsigned)((n + ZS_ENT_ENVS - 1) / ZS_ENT_ENVS); }

ZS_HD inline int ent_sat16(int64_t v) { return v < -32768 ? -32768 : v > 32767 ? 32767 : (int)v; }
// weapons.py:18-25 max_range as the largest integer d2 inside it (zs_device.hpp weapon_r2)
ZS_HD inline int ent_weapon_r2(int w) {
    return w == ZS_WEAPON_GUN ? 36 : w == ZS_WEAPON_RIFLE ? 100 : w == ZS_WEAPON_SHOTGUN ? 9 : 2;
}
ZS_HD inline int32_t ent_d2(int dx, int dy) { return (int32_t)(dx * dx + dy * dy); }
// key (da, sa) sorts before key (db, sb)
ZS_HD inline bool ent_key_less(int32_t da, int sa, int32_t db, int sb) { return da < db || (da == db && sa < sb); }
ZS_HD inline int ent_zombie_flags(int32_t d2, int r2) {
    return ZS_ENT_VALID | (d2 <= r2 ? ZS_ENT_IN_RANGE : 0) | (d2 == 1 ? ZS_ENT_ADJACENT : 0);
}
ZS_HD inline int ent_player_flags(int32_t d2, bool is_agent, int weapon) {
    return ZS_ENT_VALID | (d2 <= ZS_ENT_HEAL_R2 ? ZS_ENT_IN_RANGE : 0) | (is_agent ? ZS_ENT_IS_AGENT : 0) | ((weapon & 0xff) << 8);
}
ZS_HD inline uint64_t ent_obj_key(int32_t d2, int index) { return ((uint64_t)(uint32_t)d2 << 32) | (uint32_t)index; }
// four int16 words as the 8 bytes stored for them (word 0 lowest)
ZS_HD inline uint64_t ent_pack4(int w0, int w1, int w2, int w3) {
    return (uint64_t)(uint16_t)w0 | ((uint64_t)(uint16_t)w1 << 16) | ((uint64_t)(uint16_t)w2 << 32) | ((uint64_t)(uint16_t)w3 << 48);
}
ZS_HD inline int ent_dir_dx(int k) { return k == 1 ? -1 : k == 3 ? 1 : 0; }
ZS_HD inline int ent_dir_dy(int k) { return k == 0 ? 1 : k == 2 ? -1 : 0; }
// the ray of direction k from (x, y): blocked(cx, cy) says whether a cell inside the map holds a present obstacle
template <typename Blocked>
ZS_HD inline int ent_ray(int x, int y, int k, int W, int H, Blocked blocked) {
    const int dx = ent_dir_dx(k), dy = ent_dir_dy(k);
    int n = 0;
    while (n < ZS_ENT_RAY_CAP) {
        const int cx = x + (n + 1) * dx, cy = y + (n + 1) * dy;
        if (cx < 0 || cx >= W || cy < 0 || cy >= H || blocked(cx, cy)) break;
        n++;
    }
    return n;
}
// the row of slot s seen from the agent: zombie (player = false) or player
ZS_HD inline uint64_t ent_slot_row(int dx, int dy, int32_t life, bool player, bool is_agent, int weapon, int r2) {
    const int32_t dd = ent_d2(dx, dy);
    return ent_pack4(dx, dy, ent_sat16(life), player ? ent_player_flags(dd, is_agent, weapon) : ent_zombie_flags(dd, r2));
}

// the kernel's own argument beside the Dev (which has no field for the feature): the handle's objective list
struct EntityArgs {
    int kz, kp, nobj;
    const int32_t* obj_xy;  // [nobj] x | y << 16, map-file order
};

// the launcher (k_entity_obs.hip): rows of the envs whose env_mask byte is nonzero (null: all) into out, 8-byte aligned
#ifdef __HIPCC__
#include <hip/hip_runtime.h>
struct Dev;
hipError_t launch_entity_obs(hipStream_t s, const Dev& d, const EntityArgs& g, const uint8_t* env_mask, void* out);
#endif

// the kernel is defined by the unit that sets ZS_DEFINE_ENTITY_KERNEL (k_entity_obs.hip)
#ifdef ZS_DEFINE_ENTITY_KERNEL
#include "zs_device.hpp"

__global__ __launch_bounds__(ZS_ENT_BLOCK) void k_entity_obs(Dev d, EntityArgs g, const uint8_t* __restrict__ env_mask,
                                                             uint64_t* __restrict__ out) {
    __shared__ int32_t s_d2[ZS_ENT_ENVS][ZS_ENT_SLOTS];
    const int lane = threadIdx.x & 63;
    const int wv = threadIdx.x >> 6;
    const int e = __builtin_amdgcn_readfirstlane(blockIdx.x * ZS_ENT_ENVS + wv);
    if (e >= d.N) return;
    if (env_mask && !env_mask[e]) return;
    const int E = min(d.E, ZS_ENT_SLOTS), A = d.A, np = d.A + d.P, W = d.W, H = d.H;
    const EntLayout L = ent_layout(g.kz, g.kp);
    const int rowq = L.row_words >> 2;  // 8-byte words of a row
    const size_t row = (size_t)e * d.E;
    const int32_t* __restrict__ pos = d.pos + row;
    const int32_t* __restrict__ life = d.life + row;
    const uint8_t* __restrict__ present = d.present + row;
    const uint8_t* __restrict__ weapon = d.weapon + row;
    const uint32_t* __restrict__ opres = d.obst_present + (size_t)e * d.OW;
    uint64_t* __restrict__ orow = out + (size_t)e * A * rowq;
    int32_t* sd = s_d2[wv];
    // pass 0 of the slots stays in registers
    const bool in0 = lane < E;
    const int32_t p0 = in0 ? pos[lane] : 0;
    const int32_t l0 = in0 ? life[lane] : 0;
    const bool h0 = in0 && present[lane] != 0;
    // present zombies and players of the env
    int nz = 0, npl = 0;
    for (int s0 = 0; s0 < E; s0 += 64) {
        const int s = s0 + lane;
        const bool h = s0 == 0 ? h0 : (s < E && present[s] != 0);
        nz += __popcll(__ballot(h && s >= np));
        npl += __popcll(__ballot(h && s < np));
    }
    // rays: lane 4 i + k walks direction k of agent a0 + i; lane 4 i gathers the four counts and stores the block
    for (int a0 = 0; a0 < A; a0 += 16) {
        const int a = a0 + (lane >> 2), k = lane & 3;
        int n = 0;
        bool here = false;
        if (a < A && present[a] != 0) {
            here = true;
            const int32_t ap = pos[a];
            n = ent_ray(unpack_x(ap), unpack_y(ap), k, W, H, [&](int cx, int cy) {
                const int o = d.cellmap[cy * W + cx];
                return o >= 0 && ((opres[o >> 5] >> (o & 31)) & 1u) != 0;
            });
        }
        const int n1 = __shfl(n, (lane & ~3) + 1), n2 = __shfl(n, (lane & ~3) + 2), n3 = __shfl(n, (lane & ~3) + 3);
        if (here && k == 0) orow[(size_t)a * rowq + (L.rays >> 2)] = ent_pack4(n, n1, n2, n3);
    }
    for (int a = 0; a < A; a++) {  // wave-uniform
        uint64_t* __restrict__ r = orow + (size_t)a * rowq;
        if (!__builtin_amdgcn_readfirstlane(present[a])) {
            for (int i = lane; i < rowq; i += 64) r[i] = 0;
            continue;
        }
        const int32_t ap = __builtin_amdgcn_readfirstlane(pos[a]);
        const int ax = unpack_x(ap), ay = unpack_y(ap);
        const int aw = __builtin_amdgcn_readfirstlane(weapon[a]);
        const int r2 = ent_weapon_r2(aw);
        const int32_t al = __builtin_amdgcn_readfirstlane(life[a]);
        // every slot's d2 from the agent into the wave's LDS row
        for (int s = lane; s < E; s += 64) {
            const int32_t sp = s < 64 ? p0 : pos[s];
            const bool h = s < 64 ? h0 : present[s] != 0;
            sd[s] = h && s != a ? ent_d2(unpack_x(sp) - ax, unpack_y(sp) - ay) : ZS_ENT_ABSENT;
        }
        wave_sync();
        // a slot's rank in its class; a rank below K stores the slot's row
        for (int s = lane; s < E; s += 64) {
            const int32_t mine = sd[s];
            if (mine == ZS_ENT_ABSENT) continue;
            const bool player = s < np;
            const int lo = player ? 0 : np, hi = player ? np : E, K = player ? g.kp : g.kz;
            int rank = 0;
            for (int t = lo; t < hi && rank < K; t++) rank += ent_key_less(sd[t], t, mine, s) ? 1 : 0;
            if (rank < K) {
                const int32_t sp = s < 64 ? p0 : pos[s];
                r[((player ? L.players : L.zombies) >> 2) + rank] =
                    ent_slot_row(unpack_x(sp) - ax, unpack_y(sp) - ay, s < 64 ? l0 : life[s], player, s < A, weapon[s], r2);
            }
        }
        // the zero rows past the class counts (the agent itself is a present player)
        if (lane < g.kz && lane >= nz) r[(L.zombies >> 2) + lane] = 0;
        if (lane < g.kp && lane >= npl - 1) r[(L.players >> 2) + lane] = 0;
        // the nearest objective: a wave minimum of (d2, index) keys
        uint64_t key = ~0ull;
        for (int i = lane; i < g.nobj; i += 64) {
            const int32_t op = g.obj_xy[i];
            const uint64_t k2 = ent_obj_key(ent_d2(unpack_x(op) - ax, unpack_y(op) - ay), i);
            key = k2 < key ? k2 : key;
        }
#pragma unroll
        for (int m = 32; m >= 1; m >>= 1) {
            const uint64_t o = __shfl_xor(key, m);
            key = o < key ? o : key;
        }
        if (lane == 0) {
            r[L.self >> 2] = ent_pack4(1, ax, ay, ent_sat16(al));
            r[(L.self >> 2) + 1] = ent_pack4(aw, r2, ent_sat16(nz), ent_sat16(npl - 1));
            uint64_t ob = 0;
            if (g.nobj > 0) {
                const int32_t op = g.obj_xy[(uint32_t)key];
                ob = ent_pack4(unpack_x(op) - ax, unpack_y(op) - ay,
                               ZS_ENT_VALID | ((key >> 32) == 0 ? ZS_ENT_ON_OBJECTIVE : 0), ent_sat16(g.nobj));
            }
            r[L.objective >> 2] = ob;
        }
        wave_sync();  // the next agent rewrites the LDS row
    }
}
#endif
