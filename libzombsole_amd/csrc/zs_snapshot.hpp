// zs_snapshot.hpp — the complete per-env record: everything of an env that a later step, reset, respawn or
// observation reads, copied verbatim (nothing narrowed, nothing re-derived).
//
// zs_snapshot packs envs into records, zs_restore writes records back into envs of the same handle or of any
// handle whose fingerprint agrees, and rebuilds the pending-reset list from the restored S_NEEDRESET flags.
// snapshot_layout() is the record: the byte offset of every section and the record's size.  Nothing here needs
// HIP: the engine's kernels and a plain host compiler (tests/snapshot_layout_dump.cpp) include the same file.
//
// The record, in order (E entity slots, A agents, O obstacles, DW dead-body words, OW obstacle bitmap words):
//   the env-major rows of 4-byte elements, the long ones first: the ring is 312 chunks whatever the config, and
//   with DW, O, OW and E multiples of 4 (the workloads' maps) every row below starts at a multiple of 16 both in
//   the record and in the engine's [N][row] array, so it moves as 16-B accesses on both sides (with the ring
//   behind the columns and pos / life / serial it sat at byte 200 at C3, 8 mod 16, and moved as dwords:
//   profiles/snapshot_bench.json):
//     ring         u32 [ZS_SNAP_RING]   both MT19937 blocks (the one being consumed and the next)
//     dead         u32 [DW]
//     obst_hp      i32 [O]              always int32, whatever the observation dtype
//     obst_present u32 [OW]
//     obst_nonpos  u32 [OW]
//     pos          i32 [E]              x | y << 16
//     life         i32 [E]
//     serial       u32 [E]              spawn serials
//   the engine's [k][N] column arrays, together, so one lane group gathers them in one round:
//     scal         i32 [ZS_SNAP_NSCAL]  every per-env scalar row (zs_device.hpp S_*), S_NEEDRESET and S_ODIRTY included
//     hp_dirty     u32                  obstacle-HP chunks that may differ from a fresh env's
//     dead_dirty   u32                  dead-body chunks that may be non-zero
//     rngst        u32                  the MT19937 ring's offset, slot and ready bits
//     prev_life    i32 [A]              the reward tracker's previous life per agent
//   on a ZS_FLAG_ENV_PARAMS handle only:
//     env_params   i32 [6]              the running episode's (initial, minimum, max_steps), then the next reset's
//   on a ZS_FLAG_EPISODE_STATS handle only, 8-byte aligned (4 zero bytes ahead of it where the sections before it end
//   at an odd dword):
//     ep_run       f64 [R], i32, 4 zero bytes   the running episode's return (R = 1 on the single surface, A on the
//                                       multi surface) and run_flags (zs_episode.hpp)
//   the byte rows:
//     weapon, present, order  u8 [E] each
//     listed       u8 [A]               ([a][N] columns in the engine)
//   on a ZS_FLAG_RENDER handle only, the last byte row:
//     body_col     u8 [W H rounded up to 16]   per cell the palette index of its last body (zs_render.hpp)
//   zero bytes up to rec_bytes, a multiple of 16.
// Every 4-byte section is 4-byte aligned in a 16-byte aligned record.
//
// NOT in a record:
//   * the action-stream seed (Dev::seeds): it belongs to the slot's policy and is set by zs_seed;
//   * the death and action logs (ZS_FLAG_DEATH_LOG): they are a step's outputs; zs_restore zeroes the counts
//     (dlog_n, alog_n) of the envs it writes when the handle keeps logs;
//   * the handle's sticky ZS_OVF_* word (zs_overflow);
//   * the policy step counter of zs_step_graph;
//   * the last finished episode and the totals of a ZS_FLAG_EPISODE_STATS handle (last, last_ret, tot, sum_ret): they
//     are the slot's own, like the action-stream seed, and zs_restore leaves them alone.  Only the running part
//     (ep_run) belongs to an env.
#pragma once
#include <stdint.h>

#include "zs_step_plan.hpp"  // ZS_HD, ZS_MT_N, the public header (zs_config)

#define ZS_SNAP_NSCAL 9               // S_NSCAL (zs_device.hpp; k_records.hip asserts the two agree)
#define ZS_SNAP_RING (2 * ZS_MT_N)    // ZS_RING_WORDS

// Sections in record order; SNAP_NSEC of them, then the padding.
enum {
    SNAP_RING = 0, SNAP_DEAD, SNAP_OBST_HP, SNAP_OBST_PRESENT, SNAP_OBST_NONPOS, SNAP_POS, SNAP_LIFE, SNAP_SERIAL,
    SNAP_SCAL, SNAP_HP_DIRTY, SNAP_DEAD_DIRTY, SNAP_RNGST, SNAP_PREV_LIFE,
    SNAP_WEAPON, SNAP_PRESENT, SNAP_ORDER, SNAP_LISTED,
    SNAP_NSEC
};
#define SNAP_NWORD SNAP_WEAPON   // sections [0, SNAP_NWORD) hold 4-byte elements, the rest bytes

#define ZS_SNAP_ENVP 6   // words of the env_params section: the current triple, then the next one

struct SnapshotLayout {
    int off[SNAP_NSEC + 1];  // byte offset of every section; off[SNAP_NSEC] = where the zero padding starts
    int rec_bytes;           // a multiple of 16
    int envp;                // byte offset of the env_params section (ZS_FLAG_ENV_PARAMS handles), else 0
    int ep_run;              // byte offset of the ep_run section (ZS_FLAG_EPISODE_STATS handles), 8-byte aligned, else 0
    int ep_bytes;            // its bytes, 8 R + 8, else 0
    int ep_gap;              // zero bytes ahead of it (0 or 4)
    int body_col;            // byte offset of the body_col section (ZS_FLAG_RENDER handles), else 0
    int body_bytes;          // its bytes, else 0
};

// env_params: the record of a ZS_FLAG_ENV_PARAMS handle, which holds one section more, env_params i32 [ZS_SNAP_ENVP]
// (the engine's [6][N] columns), after prev_life, the last of the 4-byte sections, and before the byte rows
// ep_R: the record of a ZS_FLAG_EPISODE_STATS handle with R reward slots per env (0: none), which holds ep_run behind
// env_params (if any) and before the byte rows
// body_bytes: the record of a ZS_FLAG_RENDER handle (0: none), which holds body_col behind listed, the last byte row
ZS_HD inline SnapshotLayout snapshot_layout(int E, int O, int DW, int OW, int A, bool env_params = false, int ep_R = 0,
                                            int body_bytes = 0) {
    const int bytes[SNAP_NSEC] = {4 * ZS_SNAP_RING, 4 * DW, 4 * O, 4 * OW, 4 * OW, 4 * E, 4 * E, 4 * E,
                                  4 * ZS_SNAP_NSCAL, 4, 4, 4, 4 * A,
                                  E, E, E, A};
    SnapshotLayout L;
    L.envp = L.ep_run = L.ep_bytes = L.ep_gap = L.body_col = L.body_bytes = 0;
    int o = 0;
    for (int s = 0; s < SNAP_NSEC; s++) {
        if (s == SNAP_NWORD && env_params) L.envp = o, o += 4 * ZS_SNAP_ENVP;
        if (s == SNAP_NWORD && ep_R > 0) L.ep_gap = o & 4, L.ep_run = o + L.ep_gap, L.ep_bytes = 8 * ep_R + 8, o = L.ep_run + L.ep_bytes;
        L.off[s] = o, o += bytes[s];
    }
    if (body_bytes > 0) L.body_col = o, L.body_bytes = body_bytes, o += body_bytes;
    L.off[SNAP_NSEC] = o;
    L.rec_bytes = (o + 15) & ~15;
    return L;
}

// ---------------------------------------------------------------------------
// Fingerprint: 64 bits over what gives a record its meaning.  Two handles whose fingerprints agree can exchange
// records.  Covered: W, H, O, E, A, P, Z, the rules, the reward mode, max_episode_steps, the initial and minimum
// zombies, and the static tables: obstacle cells and kinds, player and zombie spawn lists, objective cells, agent
// weapons, bot types (each with its length).  Deliberately not covered: the env count, the observation settings
// (scope, encoding, width, dtype, agent codes), lanes_per_env, the launch overrides and the flags, but for
// ZS_FLAG_ENV_PARAMS, ZS_FLAG_EPISODE_STATS and ZS_FLAG_RENDER: a handle with any of them has a longer record, so the
// flag is hashed in (last, in that order, and only when set: the fingerprints of handles without them are what they were).
// ---------------------------------------------------------------------------
inline uint64_t snapshot_fp_add(uint64_t h, uint64_t v) {  // splitmix64's finaliser over the running value
    uint64_t z = (h ^ v) + 0x9E3779B97F4A7C15ull;
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
    return z ^ (z >> 31);
}

inline uint64_t snapshot_fp_table(uint64_t h, const int32_t* v, int n) {
    h = snapshot_fp_add(h, (uint64_t)(uint32_t)n);
    for (int i = 0; i < n; i++) h = snapshot_fp_add(h, (uint64_t)(uint32_t)v[i]);
    return h;
}

inline uint64_t snapshot_fingerprint(const zs_config* c) {
    const zs_map_desc& m = c->map;
    const int Z = c->initial_zombies > c->minimum_zombies ? c->initial_zombies : c->minimum_zombies;
    const int32_t head[12] = {m.width, m.height, m.n_obstacles, c->num_agents + c->num_bots + Z, c->num_agents,
                              c->num_bots, Z, c->rules, c->reward_mode, c->max_episode_steps,
                              c->initial_zombies, c->minimum_zombies};
    uint64_t h = 0x7A735F736E617031ull;  // "zs_snap1"
    h = snapshot_fp_table(h, head, 12);
    h = snapshot_fp_table(h, m.obstacle_xy, 2 * m.n_obstacles);
    h = snapshot_fp_add(h, (uint64_t)(uint32_t)m.n_obstacles);
    for (int i = 0; i < m.n_obstacles; i++) h = snapshot_fp_add(h, m.obstacle_kind[i]);
    h = snapshot_fp_table(h, m.player_spawn_xy, 2 * m.n_player_spawns);
    h = snapshot_fp_table(h, m.zombie_spawn_xy, 2 * m.n_zombie_spawns);
    h = snapshot_fp_table(h, m.objective_xy, 2 * m.n_objectives);
    h = snapshot_fp_table(h, c->agent_weapons, c->num_agents);
    h = snapshot_fp_table(h, c->bot_types, c->num_bots);
    if (c->flags & ZS_FLAG_ENV_PARAMS) h = snapshot_fp_add(h, (uint64_t)ZS_FLAG_ENV_PARAMS);
    if (c->flags & ZS_FLAG_EPISODE_STATS) h = snapshot_fp_add(h, (uint64_t)ZS_FLAG_EPISODE_STATS);
    if (c->flags & ZS_FLAG_RENDER) h = snapshot_fp_add(h, (uint64_t)ZS_FLAG_RENDER);
    return h;
}
