// zs_entity_act.hpp — k_entity_act_*: the entity action table, NID = 15 + KZ + KP ids per agent with the KZ, KP of
// the entity observation (zs_entity_obs.hpp).  The table is stated here once, as rule functions a host compiler builds
// too (tests/entity_act_host.cpp); the kernels below them need HIP.
//
//   id                    triple                                   mask bit is 1 exactly when
//   0..3                  (MOVE, dir k)                            as zs_action_mask byte k
//   4                     (ATTACK_CLOSEST, 0, 0)                   as zs_action_mask byte 4
//   5                     (HEAL, 0, 0)                             always
//   6                     (HEAL_CLOSEST, 0, 0)                     zs_action_mask byte 6 of the multi surface, on both surfaces
//   7..10                 (ATTACK, dir k)                          the adjacent cell is inside the map and holds a thing: a present
//                                                                  obstacle whatever its life, or a present zombie, bot or agent
//   11..14                (HEAL, dir k)                            the adjacent cell holds a present agent or bot or a present
//                                                                  obstacle, not a zombie (players/agent.py:69-75)
//   15 + j, j < KZ        (ATTACK, dx_j, dy_j) of zombie row j     the row is valid and d2 <= weapon_r2 (its IN_RANGE bit)
//   15 + KZ + j, j < KP   (HEAL, dx_j, dy_j) of player row j       the row is valid and d2 <= 9
// dir k = (0,1), (-1,0), (0,-1), (1,0); row j = the j-th present zombie, or the j-th other present agent or bot, by
// zs_entity_obs.hpp's key (d2, slot).  Everything is of the env's current world (the one its observation shows; an env
// pending its reset shows its terminal world).  A bit says what zs_action_mask's bytes say: were this the agent's
// action and the first one executed, the reference would carry it out ('moved to', 'injured', 'healed').
//
// Decode: a valid row decodes to its triple whatever its mask bit; a row past the class's present slots, and every id
// of an agent that is not present, decodes to (ZS_ACT_IDLE, 0, 0); an id outside [0, NID) does too and raises
// ZS_OVF_PARAM_RANGE.  Mask: uint8 [N][A][RB], RB = NID rounded up to 8, padding bytes 0; an agent that is not present
// has an all-zero row.  Encode: the smallest id of [0, NID) whose decoded triple equals the given one word for word,
// else -1.
//
// Mapping (k_entity_obs's): one wave per env, four envs per workgroup, lanes striding the E slots with pass 0 in
// registers; per agent the slots' d2 go into the wave's LDS row and a slot's rank in its class is the count of smaller
// keys.  Decode ranks only when the id names a row, and the lane whose slot has rank j stores the triple; the mask
// ranks every slot, the lanes below K put their bytes into the wave's LDS byte row beside the fifteen fixed bytes
// (mask_slot_bits' predicates, zs_mask.hpp, folded by ballots) and the row leaves as 8-byte stores; encode ranks the
// one slot that stands at the triple's offset.  The four adjacent cells' bounds / obstacle tests run ahead, one lane
// per (agent, direction), sixteen agents a round.  The kernels read what k_action_mask and k_entity_obs read.
#pragma once
#include <stdint.h>

#include "zs_entity_obs.hpp"  // ent_k_ok, ent_d2, ent_key_less, ent_weapon_r2, ZS_ENT_HEAL_R2, ent_dir_dx / _dy

#define ZS_EACT_FIXED 15       // ids below the rows
#define ZS_EACT_ATTACK_DIR 7   // first id of (ATTACK, dir k)
#define ZS_EACT_HEAL_DIR 11    // first id of (HEAL, dir k)
#define ZS_EACT_ROW_BYTES_MAX 48  // RB at KZ = KP = 16

// the classes of an id
enum { EACT_MOVE = 0, EACT_ATTACK_CLOSEST, EACT_HEAL_SELF, EACT_HEAL_CLOSEST, EACT_ATTACK_DIR, EACT_HEAL_DIR, EACT_ZOMBIE_ROW,
       EACT_PLAYER_ROW, EACT_BAD };

struct EactTriple {
    int32_t kind, dx, dy;
};
ZS_HD inline EactTriple eact_triple(int kind, int dx, int dy) {
    EactTriple t;
    t.kind = kind;
    t.dx = dx;
    t.dy = dy;
    return t;
}
ZS_HD inline bool eact_same(const EactTriple& a, const EactTriple& b) { return a.kind == b.kind && a.dx == b.dx && a.dy == b.dy; }

ZS_HD inline int eact_nid(int kz, int kp) { return ZS_EACT_FIXED + kz + kp; }
ZS_HD inline int eact_row_bytes(int kz, int kp) { return (eact_nid(kz, kp) + 7) & ~7; }
ZS_HD inline int eact_zombie_id(int j) { return ZS_EACT_FIXED + j; }
ZS_HD inline int eact_player_id(int kz, int j) { return ZS_EACT_FIXED + kz + j; }

// an id's class; *k = its direction or row
ZS_HD inline int eact_class(int id, int kz, int kp, int* k) {
    *k = 0;
    if (id < 0 || id >= eact_nid(kz, kp)) return EACT_BAD;
    if (id < 4) return *k = id, EACT_MOVE;
    if (id == 4) return EACT_ATTACK_CLOSEST;
    if (id == 5) return EACT_HEAL_SELF;
    if (id == 6) return EACT_HEAL_CLOSEST;
    if (id < ZS_EACT_HEAL_DIR) return *k = id - ZS_EACT_ATTACK_DIR, EACT_ATTACK_DIR;
    if (id < ZS_EACT_FIXED) return *k = id - ZS_EACT_HEAL_DIR, EACT_HEAL_DIR;
    if (id < ZS_EACT_FIXED + kz) return *k = id - ZS_EACT_FIXED, EACT_ZOMBIE_ROW;
    return *k = id - ZS_EACT_FIXED - kz, EACT_PLAYER_ROW;
}
// the triple of a fixed entry (id < ZS_EACT_FIXED) and of a valid row
ZS_HD inline EactTriple eact_fixed_triple(int id) {
    int k;
    switch (eact_class(id, 1, 0, &k)) {
        case EACT_MOVE: return eact_triple(ZS_ACT_MOVE, ent_dir_dx(k), ent_dir_dy(k));
        case EACT_ATTACK_CLOSEST: return eact_triple(ZS_ACT_ATTACK_CLOSEST, 0, 0);
        case EACT_HEAL_SELF: return eact_triple(ZS_ACT_HEAL, 0, 0);
        case EACT_HEAL_CLOSEST: return eact_triple(ZS_ACT_HEAL_CLOSEST, 0, 0);
        case EACT_ATTACK_DIR: return eact_triple(ZS_ACT_ATTACK, ent_dir_dx(k), ent_dir_dy(k));
        case EACT_HEAL_DIR: return eact_triple(ZS_ACT_HEAL, ent_dir_dx(k), ent_dir_dy(k));
        default: return eact_triple(ZS_ACT_IDLE, 0, 0);
    }
}
ZS_HD inline EactTriple eact_row_triple(bool player, int dx, int dy) { return eact_triple(player ? ZS_ACT_HEAL : ZS_ACT_ATTACK, dx, dy); }

// What the fixed entries' bits read of the agent's surroundings.  Bit k of a 4-bit field speaks of the adjacent cell
// in direction k: `out` it lies outside the map, `obst` a present obstacle stands there, `thing` a present slot other
// than the agent does, `player` that slot is an agent or a bot.  zombie_in_range, other_player, other_in_heal are
// mask_slot_bits' bits 4, 5, 6 over every slot (zs_mask.hpp).
struct EactNear {
    uint32_t out, obst, thing, player;
    bool zombie_in_range, other_player, other_in_heal;
};
// the mask bit of a fixed entry of a present agent
ZS_HD inline int eact_fixed_mask(int id, const EactNear& w) {
    int k;
    switch (eact_class(id, 1, 0, &k)) {
        case EACT_MOVE: return (((w.out | w.obst | w.thing) >> k) & 1u) ? 0 : 1;
        case EACT_ATTACK_CLOSEST: return w.zombie_in_range ? 1 : 0;
        case EACT_HEAL_SELF: return 1;
        case EACT_HEAL_CLOSEST: return (!w.other_player || w.other_in_heal) ? 1 : 0;
        case EACT_ATTACK_DIR: return (((~w.out & (w.obst | w.thing)) >> k) & 1u) ? 1 : 0;
        case EACT_HEAL_DIR: return (((~w.out & (w.obst | w.player)) >> k) & 1u) ? 1 : 0;
        default: return 0;
    }
}
// all fifteen, bit id of the word
ZS_HD inline uint32_t eact_fixed_bits(const EactNear& w) {
    uint32_t b = 0;
    for (int id = 0; id < ZS_EACT_FIXED; id++) b |= (uint32_t)eact_fixed_mask(id, w) << id;
    return b;
}
// the mask bit of a valid row at distance d2; r2 = the weapon's range of the agent
ZS_HD inline int eact_row_mask(bool player, int32_t d2, int r2) { return d2 <= (player ? ZS_ENT_HEAL_R2 : r2) ? 1 : 0; }

// Encode.  The smallest fixed id whose triple is t, else -1
ZS_HD inline int eact_fixed_match(const EactTriple& t) {
    for (int id = 0; id < ZS_EACT_FIXED; id++)
        if (eact_same(eact_fixed_triple(id), t)) return id;
    return -1;
}
// a present slot of the class at offset (dx, dy) decodes to t
ZS_HD inline bool eact_row_match(const EactTriple& t, bool player, int dx, int dy) { return eact_same(eact_row_triple(player, dx, dy), t); }
// the smallest id that decodes to (ZS_ACT_IDLE, 0, 0) for a present agent: the first row past the nz present zombies,
// else the first past the `others` other present players, else -1
ZS_HD inline int eact_idle_id(int nz, int others, int kz, int kp) {
    return nz < kz ? eact_zombie_id(nz) : others < kp ? eact_player_id(kz, others) : -1;
}
// the id of an agent that is not present: every id decodes to idle
ZS_HD inline int eact_absent_id(const EactTriple& t) { return eact_same(t, eact_triple(ZS_ACT_IDLE, 0, 0)) ? 0 : -1; }

// the launchers (k_entity_act.hip), over the envs whose env_mask byte is nonzero (null: all): ids int32 [N][A] into
// triples int32 [N][A][3]; the masks uint8 [N][A][RB], 8-byte aligned; triples into ids
#ifdef __HIPCC__
hipError_t launch_entity_act_decode(hipStream_t s, const Dev& d, int kz, int kp, const uint8_t* env_mask, const int32_t* ids,
                                    int32_t* actions);
hipError_t launch_entity_act_mask(hipStream_t s, const Dev& d, int kz, int kp, const uint8_t* env_mask, void* out);
hipError_t launch_entity_act_encode(hipStream_t s, const Dev& d, int kz, int kp, const uint8_t* env_mask, const int32_t* triples,
                                    int32_t* ids_out);
#endif

// the kernels are defined by the unit that sets ZS_DEFINE_ENTITY_ACT_KERNEL (k_entity_act.hip)
#ifdef ZS_DEFINE_ENTITY_ACT_KERNEL
#include "zs_mask.hpp"  // mask_slot_bits (zs_device.hpp)

// one env's view, shared by the three kernels: the wave's env, its rows, pass 0 of the slots in registers
struct EactEnv {
    int lane, wv, e, E, A, np, W, H;
    const int32_t* __restrict__ pos;
    const uint8_t* __restrict__ present;
    const uint8_t* __restrict__ weapon;
    const uint32_t* __restrict__ opres;
    int32_t p0;
    bool h0;
    int nz, npl;  // present zombies, present agents and bots
};
// false: the wave has no env, or its env-mask byte is 0
__device__ __forceinline__ bool eact_env(const Dev& d, const uint8_t* env_mask, bool count, EactEnv* v) {
    v->lane = threadIdx.x & 63;
    v->wv = threadIdx.x >> 6;
    v->e = __builtin_amdgcn_readfirstlane(blockIdx.x * ZS_ENT_ENVS + v->wv);
    if (v->e >= d.N) return false;
    if (env_mask && !env_mask[v->e]) return false;
    v->E = min(d.E, ZS_ENT_SLOTS);
    v->A = d.A;
    v->np = d.A + d.P;
    v->W = d.W;
    v->H = d.H;
    const size_t row = (size_t)v->e * d.E;
    v->pos = d.pos + row;
    v->present = d.present + row;
    v->weapon = d.weapon + row;
    v->opres = d.obst_present + (size_t)v->e * d.OW;
    const bool in0 = v->lane < v->E;
    v->p0 = in0 ? v->pos[v->lane] : 0;
    v->h0 = in0 && v->present[v->lane] != 0;
    v->nz = v->npl = 0;
    if (count)
        for (int s0 = 0; s0 < v->E; s0 += 64) {
            const int s = s0 + v->lane;
            const bool h = s0 == 0 ? v->h0 : (s < v->E && v->present[s] != 0);
            v->nz += __popcll(__ballot(h && s >= v->np));
            v->npl += __popcll(__ballot(h && s < v->np));
        }
    return true;
}
// slot s = lane + 64 k of the lane's stride: pass 0 from the registers
__device__ __forceinline__ int32_t eact_pos(const EactEnv& v, int s) { return s < 64 ? v.p0 : v.pos[s]; }
__device__ __forceinline__ bool eact_here(const EactEnv& v, int s) { return s < 64 ? v.h0 : v.present[s] != 0; }
// every slot's d2 from the agent at (ax, ay) into the wave's LDS row (absent slots and the agent itself the sentinel)
__device__ __forceinline__ void eact_fill(const EactEnv& v, int a, int ax, int ay, int32_t* sd) {
    for (int s = v.lane; s < v.E; s += 64) {
        const int32_t sp = eact_pos(v, s);
        sd[s] = eact_here(v, s) && s != a ? ent_d2(unpack_x(sp) - ax, unpack_y(sp) - ay) : ZS_ENT_ABSENT;
    }
    wave_sync();
}
// the rank of slot s (its d2 `mine` in the row) in its class, counted up to `cap`
__device__ __forceinline__ int eact_rank(const EactEnv& v, const int32_t* sd, int s, int32_t mine, int cap) {
    const bool player = s < v.np;
    const int lo = player ? 0 : v.np, hi = player ? v.np : v.E;
    int rank = 0;
    for (int t = lo; t < hi && rank < cap; t++) rank += ent_key_less(sd[t], t, mine, s) ? 1 : 0;
    return rank;
}
__device__ __forceinline__ void eact_raise(const Dev& d) {
    const uint32_t f = ZS_OVF_PARAM_RANGE;
    if ((__hip_atomic_load(d.ovf, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) & f) != f) atomicOr(d.ovf, f);
}

__global__ __launch_bounds__(ZS_ENT_BLOCK) void k_entity_act_decode(Dev d, int kz, int kp, const uint8_t* __restrict__ env_mask,
                                                                    const int32_t* __restrict__ ids, int32_t* actions) {
    __shared__ int32_t s_d2[ZS_ENT_ENVS][ZS_ENT_SLOTS];
    EactEnv v;
    if (!eact_env(d, env_mask, true, &v)) return;
    int32_t* sd = s_d2[v.wv];
    const int32_t* __restrict__ idrow = ids + (size_t)v.e * v.A;
    int32_t* orow = actions + (size_t)v.e * v.A * 3;
    bool raise = false;  // wave-uniform
    for (int a = 0; a < v.A; a++) {  // wave-uniform
        int32_t* o = orow + 3 * a;
        const int id = __builtin_amdgcn_readfirstlane(idrow[a]);
        int j;
        const int cls = eact_class(id, kz, kp, &j);
        raise = raise || cls == EACT_BAD;
        const bool here = __builtin_amdgcn_readfirstlane(v.present[a]) != 0;
        const bool row = cls == EACT_ZOMBIE_ROW || cls == EACT_PLAYER_ROW;
        const bool player = cls == EACT_PLAYER_ROW;
        if (!here || !row || j >= (player ? v.npl - 1 : v.nz)) {
            if (v.lane == 0) {
                const EactTriple t = here && !row ? eact_fixed_triple(cls == EACT_BAD ? -1 : id) : eact_triple(ZS_ACT_IDLE, 0, 0);
                o[0] = t.kind;
                o[1] = t.dx;
                o[2] = t.dy;
            }
            continue;
        }
        const int32_t ap = __builtin_amdgcn_readfirstlane(v.pos[a]);
        const int ax = unpack_x(ap), ay = unpack_y(ap);
        eact_fill(v, a, ax, ay, sd);
        // the slot of the class whose rank is j: its lane stores the triple
        for (int s = v.lane; s < v.E; s += 64) {
            const int32_t mine = sd[s];
            if (mine == ZS_ENT_ABSENT || (s < v.np) != player || eact_rank(v, sd, s, mine, j + 1) != j) continue;
            const int32_t sp = eact_pos(v, s);
            const EactTriple t = eact_row_triple(player, unpack_x(sp) - ax, unpack_y(sp) - ay);
            o[0] = t.kind;
            o[1] = t.dx;
            o[2] = t.dy;
        }
        wave_sync();  // the next agent rewrites the LDS row
    }
    if (raise && v.lane == 0) eact_raise(d);
}

// bits 4 i + k of the two words: direction k of agent a0 + i lies outside the map; a present obstacle stands there
__device__ __forceinline__ void eact_adjacent(const Dev& d, const EactEnv& v, int a0, uint64_t* out, uint64_t* obst) {
    const int a = a0 + (v.lane >> 2), k = v.lane & 3;
    bool bo = false, bb = false;
    if (a < v.A) {
        const int32_t ap = v.pos[a];
        const int x = unpack_x(ap) + ent_dir_dx(k), y = unpack_y(ap) + ent_dir_dy(k);
        bo = x < 0 || x >= v.W || y < 0 || y >= v.H;
        if (!bo) {
            const int o = d.cellmap[y * v.W + x];
            bb = o >= 0 && ((v.opres[o >> 5] >> (o & 31)) & 1u) != 0;
        }
    }
    *out = __ballot(bo);
    *obst = __ballot(bb);
}

__global__ __launch_bounds__(ZS_ENT_BLOCK) void k_entity_act_mask(Dev d, int kz, int kp, const uint8_t* __restrict__ env_mask,
                                                                  uint64_t* __restrict__ out) {
    __shared__ int32_t s_d2[ZS_ENT_ENVS][ZS_ENT_SLOTS];
    __shared__ uint64_t s_row[ZS_ENT_ENVS][ZS_EACT_ROW_BYTES_MAX / 8];
    EactEnv v;
    if (!eact_env(d, env_mask, false, &v)) return;
    int32_t* sd = s_d2[v.wv];
    uint8_t* sb = (uint8_t*)s_row[v.wv];
    const int rbq = eact_row_bytes(kz, kp) >> 3;  // 8-byte words of a row
    uint64_t* __restrict__ orow = out + (size_t)v.e * v.A * rbq;
    for (int a0 = 0; a0 < v.A; a0 += 16) {
        uint64_t bout, bobst;
        eact_adjacent(d, v, a0, &bout, &bobst);
        const int na = min(16, v.A - a0);
        for (int i = 0; i < na; i++) {
            const int a = a0 + i;  // wave-uniform
            uint64_t* __restrict__ r = orow + (size_t)a * rbq;
            if (!__builtin_amdgcn_readfirstlane(v.present[a])) {
                if (v.lane < rbq) r[v.lane] = 0;
                continue;
            }
            const int32_t ap = __builtin_amdgcn_readfirstlane(v.pos[a]);
            const int ax = unpack_x(ap), ay = unpack_y(ap);
            const int r2 = ent_weapon_r2(__builtin_amdgcn_readfirstlane(v.weapon[a]));
            // the fixed entries: mask_slot_bits of every slot, the adjacent players apart, made wave-uniform by ballots
            uint32_t f = 0, fp = 0;
            for (int s = v.lane; s < v.E; s += 64) {
                const uint32_t b = mask_slot_bits(s, eact_pos(v, s), eact_here(v, s), a, ap, r2, v.np);
                f |= b;
                if (s < v.np) fp |= b & 15u;
            }
            EactNear w;
            w.out = (uint32_t)(bout >> (4 * i)) & 15u;
            w.obst = (uint32_t)(bobst >> (4 * i)) & 15u;
            w.thing = w.player = 0;
#pragma unroll
            for (int k = 0; k < 4; k++) {
                w.thing |= __ballot(f & (1u << k)) != 0 ? 1u << k : 0u;
                w.player |= __ballot(fp & (1u << k)) != 0 ? 1u << k : 0u;
            }
            w.zombie_in_range = __ballot(f & 16u) != 0;
            w.other_player = __ballot(f & 32u) != 0;
            w.other_in_heal = __ballot(f & 64u) != 0;
            const uint32_t fixed = eact_fixed_bits(w);
            if (v.lane < 8 * rbq) sb[v.lane] = v.lane < ZS_EACT_FIXED ? (uint8_t)((fixed >> v.lane) & 1u) : (uint8_t)0;
            eact_fill(v, a, ax, ay, sd);  // its wave_sync orders the byte row too
            // the rows: a slot that ranks below K puts its bit at that rank
            for (int s = v.lane; s < v.E; s += 64) {
                const int32_t mine = sd[s];
                if (mine == ZS_ENT_ABSENT) continue;
                const bool player = s < v.np;
                const int K = player ? kp : kz;
                const int rank = eact_rank(v, sd, s, mine, K);
                if (rank < K) sb[player ? eact_player_id(kz, rank) : eact_zombie_id(rank)] = (uint8_t)eact_row_mask(player, mine, r2);
            }
            wave_sync();
            if (v.lane < rbq) r[v.lane] = s_row[v.wv][v.lane];
            wave_sync();  // the next agent rewrites both LDS rows
        }
    }
}

__global__ __launch_bounds__(ZS_ENT_BLOCK) void k_entity_act_encode(Dev d, int kz, int kp, const uint8_t* __restrict__ env_mask,
                                                                    const int32_t* __restrict__ triples, int32_t* __restrict__ ids_out) {
    __shared__ int32_t s_d2[ZS_ENT_ENVS][ZS_ENT_SLOTS];
    EactEnv v;
    if (!eact_env(d, env_mask, true, &v)) return;
    int32_t* sd = s_d2[v.wv];
    const int32_t* __restrict__ trow = triples + (size_t)v.e * v.A * 3;
    int32_t* __restrict__ orow = ids_out + (size_t)v.e * v.A;
    for (int a = 0; a < v.A; a++) {  // wave-uniform
        const EactTriple t = eact_triple(__builtin_amdgcn_readfirstlane(trow[3 * a]), __builtin_amdgcn_readfirstlane(trow[3 * a + 1]),
                                         __builtin_amdgcn_readfirstlane(trow[3 * a + 2]));
        int id;
        if (!__builtin_amdgcn_readfirstlane(v.present[a])) {
            id = eact_absent_id(t);
        } else {
            id = eact_fixed_match(t);
            const bool zrows = t.kind == ZS_ACT_ATTACK, prows = t.kind == ZS_ACT_HEAL;
            if (id < 0 && (zrows || prows)) {
                const int32_t ap = __builtin_amdgcn_readfirstlane(v.pos[a]);
                const int ax = unpack_x(ap), ay = unpack_y(ap);
                eact_fill(v, a, ax, ay, sd);
                // the slots of the class at the triple's offset whose rank is below K: the smallest id among them
                int mine_id = 0x7fffffff;
                const int K = prows ? kp : kz;
                for (int s = v.lane; s < v.E; s += 64) {
                    const int32_t mine = sd[s];
                    if (mine == ZS_ENT_ABSENT || (s < v.np) != prows) continue;
                    const int32_t sp = eact_pos(v, s);
                    if (!eact_row_match(t, prows, unpack_x(sp) - ax, unpack_y(sp) - ay)) continue;
                    const int rank = eact_rank(v, sd, s, mine, K);
                    if (rank < K) mine_id = min(mine_id, prows ? eact_player_id(kz, rank) : eact_zombie_id(rank));
                }
#pragma unroll
                for (int m = 32; m >= 1; m >>= 1) mine_id = min(mine_id, __shfl_xor(mine_id, m));
                id = mine_id == 0x7fffffff ? -1 : mine_id;
                wave_sync();  // the next agent rewrites the LDS row
            }
            if (id < 0 && eact_same(t, eact_triple(ZS_ACT_IDLE, 0, 0))) id = eact_idle_id(v.nz, v.npl - 1, kz, kp);
        }
        if (v.lane == 0) orow[a] = id;
    }
}
#endif
