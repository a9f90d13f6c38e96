// zs_mask.hpp — k_action_mask: per-agent action masks of the Discrete(6) / Discrete(7) tables.
//
// Byte k of agent a says whether the reference would carry out game_actions[k] for a on the env's current
// world, were a's action the first one executed (players/agent.py:28-96, core.py:140-202):
//   0..3  move (0,1) (-1,0) (0,-1) (1,0): the destination is inside the map and World.things holds nothing
//         there — no present obstacle (whatever its life: a destroyed one stays until the first cleanup),
//         no present zombie, bot or agent; bodies and objectives are decoration
//   4     attack_closest: some present zombie stands within the agent's weapon range (the closest one then
//         does: min d2 <= r2 <=> any d2 <= r2, so no minimum and no tie-break is computed)
//   5     heal: the agent heals itself
//   6     heal_closest (multi surface): no other bot or agent is present (the agent heals itself), or one
//         stands within HEALING_RANGE (d2 <= 9)
//   7     always 0, as is 6 on the single surface
// An agent that is not present has all bytes 0.  The range tests are the tick's integer d2 bounds
// (zs_device.hpp weapon_r2).
//
// Mapping: one wave per env, four envs per workgroup.  Lanes stride over the E entity slots (pass 0 stays in
// registers); per agent every lane folds its slots into eight predicate bits and eight ballots make them
// wave-uniform.  The obstacle / bounds test of the four destinations runs ahead of the agent loop with one
// lane per (agent, direction), sixteen agents per ballot.  Lane a & 63 keeps agent a's eight bytes and the
// lanes store them together, 8 bytes each.
#pragma once
#include "zs_device.hpp"

#define ZS_MASK_BLOCK 256
#define ZS_MASK_ENVS (ZS_MASK_BLOCK / 64)
#define ZS_MASK_HEAL_R2 9  // HEALING_RANGE = 3 (core.py:8)

// workgroups of a mask launch over n envs
static inline unsigned zs_mask_grid(int n) { return (unsigned)((n + ZS_MASK_ENVS - 1) / ZS_MASK_ENVS); }

// the predicate bits of slot s against agent a: 0..3 the slot stands on destination k, 4 zombie in range,
// 5 other player present, 6 other player in healing range (k_entity_act folds the same bits: zs_entity_act.hpp)
__device__ __forceinline__ uint32_t mask_slot_bits(int s, int32_t sp, bool here, int a, int32_t ap, int r2, int np) {
    if (!here || s == a) return 0u;
    const int dx = unpack_x(sp) - unpack_x(ap), dy = unpack_y(sp) - unpack_y(ap);
    const int dd = dx * dx + dy * dy;
    uint32_t f = 0;
    if (dd == 1) f = dx == 0 ? (dy == 1 ? 1u : 4u) : (dx == -1 ? 2u : 8u);
    if (s >= np) return f | (dd <= r2 ? 16u : 0u);
    return f | 32u | (dd <= ZS_MASK_HEAL_R2 ? 64u : 0u);
}

// the kernel is defined by the unit that sets ZS_DEFINE_MASK_KERNEL (k_mask.hip); others take the launch geometry
#ifdef ZS_DEFINE_MASK_KERNEL

__global__ __launch_bounds__(ZS_MASK_BLOCK) void k_action_mask(Dev d, const uint8_t* __restrict__ env_mask,
                                                               uint64_t* __restrict__ out) {
    const int lane = threadIdx.x & 63;
    const int e = __builtin_amdgcn_readfirstlane(blockIdx.x * ZS_MASK_ENVS + (threadIdx.x >> 6));
    if (e >= d.N) return;
    if (env_mask && !env_mask[e]) return;
    const int E = d.E, A = d.A, np = d.A + d.P, W = d.W, H = d.H;
    const bool multi = d.reward_mode == ZS_REWARD_MULTI;
    const size_t row = (size_t)e * E;
    const int32_t* __restrict__ pos = d.pos + row;
    const uint8_t* __restrict__ present = d.present + row;
    const uint8_t* __restrict__ weapon = d.weapon + row;
    const uint32_t* __restrict__ opres = d.obst_present + (size_t)e * d.OW;
    uint64_t* __restrict__ orow = out + (size_t)e * A;
    // pass 0 of the slots stays in registers
    const bool in0 = lane < E;
    const int32_t p0 = in0 ? pos[lane] : 0;
    const bool h0 = in0 && present[lane] != 0;
    for (int a0 = 0; a0 < A; a0 += 64) {
        // destinations outside the map or on a present obstacle: bit 4 * (i & 15) + k of blk[i >> 4] for
        // agent a0 + i, direction k
        uint64_t blk[4];
#pragma unroll
        for (int j = 0; j < 4; j++) {
            const int a = a0 + 16 * j + (lane >> 2), k = lane & 3;
            bool b = false;
            if (a < A) {
                const int32_t ap = pos[a];
                const int x = unpack_x(ap) + (k == 1 ? -1 : k == 3 ? 1 : 0);
                const int y = unpack_y(ap) + (k == 0 ? 1 : k == 2 ? -1 : 0);
                b = x < 0 || x >= W || y < 0 || y >= H;
                if (!b) {
                    const int o = d.cellmap[y * W + x];
                    b = o >= 0 && ((opres[o >> 5] >> (o & 31)) & 1u);
                }
            }
            blk[j] = __ballot(b);
        }
        const int na = min(64, A - a0);
        uint64_t mine = 0;
        for (int i = 0; i < na; i++) {
            const int a = a0 + i;  // wave-uniform
            uint64_t v = 0;
            if (__builtin_amdgcn_readfirstlane(present[a])) {
                const int32_t ap = __builtin_amdgcn_readfirstlane(pos[a]);
                const int r2 = weapon_r2(__builtin_amdgcn_readfirstlane(weapon[a]));
                uint32_t f = mask_slot_bits(lane, p0, h0, a, ap, r2, np);
                for (int s = lane + 64; s < E; s += 64) f |= mask_slot_bits(s, pos[s], present[s] != 0, a, ap, r2, np);
                const uint32_t hit = (uint32_t)(blk[i >> 4] >> (4 * (i & 15))) & 15u;
#pragma unroll
                for (int k = 0; k < 4; k++)
                    if (!((hit >> k) & 1u) && __ballot(f & (1u << k)) == 0) v |= 1ull << (8 * k);
                if (__ballot(f & 16u) != 0) v |= 1ull << 32;
                v |= 1ull << 40;
                if (multi && (__ballot(f & 32u) == 0 || __ballot(f & 64u) != 0)) v |= 1ull << 48;
            }
            if (lane == i) mine = v;
        }
        if (lane < na) orow[a0 + lane] = mine;
    }
}
#endif
