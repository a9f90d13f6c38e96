// zs_autopilot.hpp — k_autopilot: scripted policies for agent slots, written as zs_step action triples.  The encoding
// is stated here once, as rule functions a host compiler builds too (tests/autopilot_host.cpp); the kernel below them
// needs HIP.
//
// Output: int32 [N][A][3] triples (ZS_ACT_*, dx, dy), 4-byte aligned; policy: uint8 [N][A], one ZS_PILOT_* code per
// agent.  Every row is computed from the env's current world (the one its observation shows; an env pending its reset
// shows its terminal world):
//   0 none        the row is not written: a caller's own triple in it survives
//   1 terminator  (players/terminator.py:9-37, with the agent's own weapon) z = the closest present zombie by the key
//                 (d2, rank in the env's dict-order list), the order closest() walks World.things in:
//                   no zombie                     (ZS_ACT_HEAL, 0, 0)
//                   d2(agent, z) <= weapon_r2     (ZS_ACT_ATTACK_CLOSEST, 0, 0)
//                   else the adjacent cell of minimal d2 to z, in adjacent_positions order (0,1), (0,-1), (1,0), (-1,0),
//                   first minimum (utils.py:34-44; not the discrete table's order):
//                     a present agent or bot stands there          (ZS_ACT_HEAL, dx, dy)
//                     any other present thing stands there         (ZS_ACT_ATTACK, dx, dy): a zombie, or an obstacle
//                                                                  whatever its life (a destroyed one stays until the cleanup)
//                     nothing there, or the cell is outside the map (ZS_ACT_MOVE, dx, dy)
//   2 sniper      (players/sniper.py:9-19) (ZS_ACT_ATTACK_CLOSEST, 0, 0) always: without zombies the agent idles, as the bot
//   3 troll       (players/troll.py:10-12) (ZS_ACT_HEAL, 0, 0)
//   other codes   (ZS_ACT_IDLE, 0, 0), and ZS_OVF_PARAM_RANGE raised in the handle's overflow word
// An agent of nonzero code that is not present gets (ZS_ACT_IDLE, 0, 0).  Agent.next_step (players/agent.py:28-96)
// resolves each triple to the (action, target) the bot class returns, so the tick is what it was.  The bots that draw
// from the env's stream (hamster, randoman) are left out: a teacher must not move the stream.
//
// Mapping (as zs_mask.hpp): one wave per env, four envs per workgroup, lanes striding the E entity slots with pass 0 in
// registers.  One pass over the env's order row puts every slot's dict-order rank into the wave's LDS row (the only
// LDS).  Per terminator agent the lanes fold their present zombie slots into the 64-bit key d2 << 32 | rank and one
// wave minimum picks z; the rest is wave-uniform: four d2, one cellmap / obst_present lookup, one ballot of
// pos == cell per slot pass.  Lane a & 63 keeps agent a's triple and the lanes store them together, 12 bytes each, none
// for code 0.  No atomics but the overflow word's.
#pragma once
#include <stdint.h>

#include "../../include/zombsole_mi355x.h"
#include "zs_step_plan.hpp"  // ZS_HD

#define ZS_PILOT_BLOCK 256
#define ZS_PILOT_ENVS (ZS_PILOT_BLOCK / 64)
#define ZS_PILOT_SLOTS 256        // the LDS row of a wave: E <= 254 (zs_create)
#define ZS_PILOT_NO_RANK 0xffffu  // the rank of a slot the order row does not list (it is not present)

// workgroups of a launch over n envs
static inline unsigned zs_pilot_grid(int n) { return (unsigned)((n + ZS_PILOT_ENVS - 1) / ZS_PILOT_ENVS); }

struct PilotTriple {
    int32_t kind, dx, dy;
};
// what stands on the terminator's best cell
enum { PILOT_CELL_FREE = 0, PILOT_CELL_PLAYER = 1, PILOT_CELL_OTHER = 2 };

// weapons.py:18-25 max_range as the largest integer d2 inside it (zs_device.hpp weapon_r2)
ZS_HD inline int pilot_weapon_r2(int w) {
    return w == ZS_WEAPON_GUN ? 36 : w == ZS_WEAPON_RIFLE ? 100 : w == ZS_WEAPON_SHOTGUN ? 9 : 2;
}
ZS_HD inline int32_t pilot_d2(int dx, int dy) { return (int32_t)(dx * dx + dy * dy); }
// the closest-zombie key: the minimum is the first minimum of d2 in dict order
ZS_HD inline uint64_t pilot_key(int32_t d2, uint32_t rank) { return ((uint64_t)(uint32_t)d2 << 32) | rank; }
#define ZS_PILOT_NO_KEY (~0ull)
// adjacent_positions order (utils.py:34-44)
ZS_HD inline int pilot_adj_dx(int k) { return k == 2 ? 1 : k == 3 ? -1 : 0; }
ZS_HD inline int pilot_adj_dy(int k) { return k == 0 ? 1 : k == 1 ? -1 : 0; }
// closest(target, adjacent_positions(self)): the first minimum of the four d2 to the zombie
ZS_HD inline int pilot_best_dir(int ax, int ay, int zx, int zy) {
    int bk = 0;
    int32_t bd = pilot_d2(zx - ax - pilot_adj_dx(0), zy - ay - pilot_adj_dy(0));
    for (int k = 1; k < 4; k++) {
        const int32_t dd = pilot_d2(zx - ax - pilot_adj_dx(k), zy - ay - pilot_adj_dy(k));
        if (dd < bd) {
            bk = k;
            bd = dd;
        }
    }
    return bk;
}
ZS_HD inline PilotTriple pilot_triple(int kind, int dx, int dy) {
    PilotTriple t;
    t.kind = kind;
    t.dx = dx;
    t.dy = dy;
    return t;
}
ZS_HD inline bool pilot_in_range(uint64_t key, int r2) { return (int64_t)(key >> 32) <= (int64_t)r2; }
// the terminator out of range of its zombie, towards direction k, with `cell` (PILOT_CELL_*) on the best cell
ZS_HD inline PilotTriple pilot_chase(int k, int cell) {
    const int kind = cell == PILOT_CELL_PLAYER ? ZS_ACT_HEAL : cell == PILOT_CELL_OTHER ? ZS_ACT_ATTACK : ZS_ACT_MOVE;
    return pilot_triple(kind, pilot_adj_dx(k), pilot_adj_dy(k));
}
// every decision that needs no best cell: `code` != 0; key = the closest zombie's (ZS_PILOT_NO_KEY: none).  *chase is
// set when the terminator is out of range and pilot_chase has the answer; *bad when the code is none of the policies
ZS_HD inline PilotTriple pilot_simple(int code, bool present, uint64_t key, int r2, bool* chase, bool* bad) {
    *chase = false;
    *bad = code > ZS_PILOT_TROLL;
    if (!present || *bad) return pilot_triple(ZS_ACT_IDLE, 0, 0);
    if (code == ZS_PILOT_SNIPER) return pilot_triple(ZS_ACT_ATTACK_CLOSEST, 0, 0);
    if (code == ZS_PILOT_TROLL || key == ZS_PILOT_NO_KEY) return pilot_triple(ZS_ACT_HEAL, 0, 0);
    if (pilot_in_range(key, r2)) return pilot_triple(ZS_ACT_ATTACK_CLOSEST, 0, 0);
    *chase = true;
    return pilot_triple(ZS_ACT_IDLE, 0, 0);
}

// the launcher (k_autopilot.hip): rows of the envs whose env_mask byte is nonzero (null: all) into out
#ifdef __HIPCC__
#include <hip/hip_runtime.h>
struct Dev;
hipError_t launch_autopilot(hipStream_t s, const Dev& d, const uint8_t* env_mask, const uint8_t* policy, int32_t* out);
#endif

// the kernel is defined by the unit that sets ZS_DEFINE_PILOT_KERNEL (k_autopilot.hip)
#ifdef ZS_DEFINE_PILOT_KERNEL
#include "zs_device.hpp"

__global__ __launch_bounds__(ZS_PILOT_BLOCK) void k_autopilot(Dev d, const uint8_t* __restrict__ env_mask,
                                                              const uint8_t* __restrict__ policy, int32_t* out) {
    __shared__ uint16_t s_rank[ZS_PILOT_ENVS][ZS_PILOT_SLOTS];
    const int lane = threadIdx.x & 63;
    const int wv = threadIdx.x >> 6;
    const int e = __builtin_amdgcn_readfirstlane(blockIdx.x * ZS_PILOT_ENVS + wv);
    if (e >= d.N) return;
    if (env_mask && !env_mask[e]) return;
    const int E = min(d.E, ZS_PILOT_SLOTS), A = d.A, np = d.A + d.P, W = d.W, H = d.H;
    const size_t row = (size_t)e * d.E;
    const int32_t* __restrict__ pos = d.pos + row;
    const uint8_t* __restrict__ present = d.present + row;
    const uint8_t* __restrict__ weapon = d.weapon + row;
    const uint8_t* __restrict__ order = d.order + row;
    const uint32_t* __restrict__ opres = d.obst_present + (size_t)e * d.OW;
    const uint8_t* __restrict__ pol = policy + (size_t)e * A;
    int32_t* orow = out + (size_t)e * A * 3;
    uint16_t* sr = s_rank[wv];
    // every slot's dict-order rank: one pass over the order row
    const int n_order = min(max(__builtin_amdgcn_readfirstlane(d.scal[(size_t)S_NORDER * d.N + e]), 0), E);
    for (int s = lane; s < E; s += 64) sr[s] = (uint16_t)ZS_PILOT_NO_RANK;
    wave_sync();
    for (int k = lane; k < n_order; k += 64) {
        const int s = order[k];
        if (s < E) sr[s] = (uint16_t)k;
    }
    wave_sync();
    // pass 0 of the slots stays in registers
    const bool in0 = lane < E;
    const int32_t p0 = in0 ? pos[lane] : 0;
    const bool h0 = in0 && present[lane] != 0;
    const uint32_t r0 = in0 ? sr[lane] : ZS_PILOT_NO_RANK;
    bool raise = false;  // wave-uniform
    for (int a0 = 0; a0 < A; a0 += 64) {
        const int na = min(64, A - a0);
        PilotTriple mine = pilot_triple(ZS_ACT_IDLE, 0, 0);
        bool write = false;
        for (int i = 0; i < na; i++) {
            const int a = a0 + i;  // wave-uniform
            const int code = __builtin_amdgcn_readfirstlane(pol[a]);
            if (code == ZS_PILOT_NONE) continue;
            const bool here = __builtin_amdgcn_readfirstlane(present[a]) != 0;
            const int32_t ap = __builtin_amdgcn_readfirstlane(pos[a]);
            const int ax = unpack_x(ap), ay = unpack_y(ap);
            const int r2 = pilot_weapon_r2(__builtin_amdgcn_readfirstlane(weapon[a]));
            uint64_t key = ZS_PILOT_NO_KEY;
            int32_t zp = 0;  // the position behind this lane's key
            if (here && code == ZS_PILOT_TERMINATOR) {
                for (int s = lane; s < E; s += 64) {
                    const int32_t sp = s < 64 ? p0 : pos[s];
                    const bool h = s < 64 ? h0 : present[s] != 0;
                    if (!h || s < np) continue;
                    const uint64_t k2 = pilot_key(pilot_d2(unpack_x(sp) - ax, unpack_y(sp) - ay), s < 64 ? r0 : (uint32_t)sr[s]);
                    if (k2 < key) {
                        key = k2;
                        zp = sp;
                    }
                }
                const uint64_t own = key;
#pragma unroll
                for (int m = 32; m >= 1; m >>= 1) {
                    const uint64_t o = __shfl_xor(key, m);
                    key = o < key ? o : key;
                }
                if (key != ZS_PILOT_NO_KEY) {  // the winning lane's zombie (the ranks are distinct: one lane holds it)
                    const uint64_t who = __ballot(own == key);
                    zp = __shfl(zp, (int)__builtin_ctzll(who));
                }
            }
            bool chase, bad;
            PilotTriple t = pilot_simple(code, here, key, r2, &chase, &bad);
            raise = raise || bad;
            if (chase) {
                const int k = pilot_best_dir(ax, ay, unpack_x(zp), unpack_y(zp));
                const int bx = ax + pilot_adj_dx(k), by = ay + pilot_adj_dy(k);
                int cell = PILOT_CELL_FREE;
                if (bx >= 0 && bx < W && by >= 0 && by < H) {
                    const int o = d.cellmap[by * W + bx];
                    if (o >= 0 && ((opres[o >> 5] >> (o & 31)) & 1u)) {
                        cell = PILOT_CELL_OTHER;
                    } else {
                        const int32_t bp = pack_xy(bx, by);
                        for (int s0 = 0; s0 < E && cell == PILOT_CELL_FREE; s0 += 64) {
                            const int s = s0 + lane;
                            const bool on = s0 == 0 ? (h0 && p0 == bp) : (s < E && present[s] != 0 && pos[s] == bp);
                            const uint64_t hit = __ballot(on);
                            if (hit) cell = s0 + (int)__builtin_ctzll(hit) < np ? PILOT_CELL_PLAYER : PILOT_CELL_OTHER;
                        }
                    }
                }
                t = pilot_chase(k, cell);
            }
            if (lane == i) {
                mine = t;
                write = true;
            }
        }
        if (write) {
            int32_t* o = orow + 3 * (a0 + lane);
            o[0] = mine.kind;
            o[1] = mine.dx;
            o[2] = mine.dy;
        }
    }
    if (raise && lane == 0) {
        const uint32_t f = ZS_OVF_PARAM_RANGE;
        if ((__hip_atomic_load(d.ovf, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) & f) != f) atomicOr(d.ovf, f);
    }
}
#endif
