// zs_obs_state.hpp — the per-env record of everything the observation encoders read.
//
// An env's observation is a pure function of nine per-env arrays (zs_obs.hpp reads nothing else of an
// env): pos, life, weapon, present, hp_dirty, dead_dirty, dead, obst_present, obst_hp.  A handle packs
// them into one record per env (zs_obs_state_pack); a viewer handle of the same map and entity counts
// unpacks records of other handles into its own envs (zs_obs_state_unpack) and re-encodes them with the
// observation kernels it already has.  obs_state_layout() is the record: the byte offset of every
// section and the record's size.  Nothing here needs HIP: the engine's kernels and a plain host compiler
// (tests/obs_state_layout_dump.cpp) include the same file.
#pragma once
#include <stdint.h>

#include "zs_obs_plan.hpp"  // ZS_HD, ZS_DTYPE_*, ZS_ENC_*

// Byte offsets of a record's sections, in record order.  The 4-byte items come first, so every one of them
// is 4-byte aligned in a 16-byte aligned record; the obstacle HP follows (4-byte aligned), then the byte
// rows; zero bytes pad the record to a multiple of 16.
struct ObsStateLayout {
    int hp_dirty;      // u32
    int dead_dirty;    // u32
    int pos;           // i32 [E]  (x | y << 16)
    int life;          // i32 [E]
    int dead;          // u32 [DW]
    int obst_present;  // u32 [OW]
    int obst_hp;       // i32 [O], or i16 [O] saturated at -32768 (hp_bytes 2)
    int weapon;        // u8 [E]
    int present;       // u8 [E]
    int pad;           // zero bytes up to rec_bytes
    int rec_bytes;     // a multiple of 16
    int hp_bytes;      // bytes of an obstacle HP element: 4, or 2 for ZS_DTYPE_I16
};

// The record of a handle with E entity slots, O obstacles, DW dead-body words, OW obstacle-presence words
// and observations of obs_dtype.  int16 observations saturate an obstacle's life at -32768 themselves
// (obs_val<int16_t>), so their records carry it as int16, saturated the same way.
ZS_HD inline ObsStateLayout obs_state_layout(int E, int O, int DW, int OW, int obs_dtype) {
    ObsStateLayout L;
    L.hp_bytes = obs_dtype == ZS_DTYPE_I16 ? 2 : 4;
    int o = 0;
    L.hp_dirty = o, o += 4;
    L.dead_dirty = o, o += 4;
    L.pos = o, o += 4 * E;
    L.life = o, o += 4 * E;
    L.dead = o, o += 4 * DW;
    L.obst_present = o, o += 4 * OW;
    L.obst_hp = o, o += L.hp_bytes * O;
    L.weapon = o, o += E;
    L.present = o, o += E;
    L.pad = o;
    L.rec_bytes = (o + 15) & ~15;
    return L;
}

// The dtype a handle's record is laid out for.  The narrow HP is lossless only where the saturated life is
// the observation's element itself (the channels encoding's life plane); the simple encoding folds the life
// into 256 * code + 16 * weapon + 15 * life // 100, which still fits int16 for lives far below -32768, so
// an int16 handle with that encoding ships the int32 life.
ZS_HD inline int obs_state_record_dtype(int obs_dtype, int obs_encoding) {
    return obs_dtype == ZS_DTYPE_I16 && obs_encoding != ZS_ENC_CHANNELS ? ZS_DTYPE_I32 : obs_dtype;
}
