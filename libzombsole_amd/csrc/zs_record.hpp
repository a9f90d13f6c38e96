// zs_record.hpp — one walker for the per-env records: snapshot records (zs_snapshot.hpp) and observation-state
// records (zs_obs_state.hpp) move between a record and the engine's arrays by the same function.  The engine's
// snapshot kernels run it; its observation-state kernels keep their own ladder over ObsStateLayout, which takes
// everything from scalar registers and measured faster at 8 192 envs than a table staged in LDS, so for that record
// type the walker is, for now, the host-checked statement of the format (tests/test_record_copy.py).
//
// A record is 16-byte aligned and a multiple of 16 bytes; it is walked in 16-B chunks, and the record side of a
// chunk is always one 16-B access.  The engine side is described by a section table (RecTable): element k of a
// section of env e lies at base + e * estride + k * kstride, which covers the env-major rows ([N][row]: estride =
// the row's bytes, kstride = the element's) and the [k][N] columns (estride = the element's bytes, kstride = N of
// them) alike, so the copy has no per-section code.  The engine side is not 16-B aligned in general: a [N][E]
// int32 row starts at byte 4 e E, and a section at any 4-byte offset of the record.  rec_copy_chunk decides:
//   * a chunk inside one row of dwords moves as 16 B when its engine address allows;
//   * eight int16 elements of a narrowed row are 32 B of the env's int32 row: two 16-B accesses when aligned, the
//     loads issued before the conversions;
//   * otherwise a dword of a 4-byte section moves as a dword (the [k][N] columns are dword gathers: they sit
//     together in a record, one round of one lane group), and the rest moves by element: narrowed elements of a
//     chunk that straddles sections or is misaligned, and the u8 rows by byte;
//   * the padding packs as zero and restores nothing.
// Nothing here needs HIP: the engine's kernels and a plain host compiler (tests/record_copy_host.cpp) include the
// same file.
#pragma once
#include <assert.h>
#include <stddef.h>
#include <stdint.h>

#include "zs_obs_state.hpp"  // ZS_HD, ObsStateLayout
#include "zs_snapshot.hpp"   // SnapshotLayout

#if defined(__HIPCC__)
#define ZS_UNROLL _Pragma("unroll")
#else
#define ZS_UNROLL
#endif

// Element kinds.  A section's kinds never decrease along a record (rec_table checks it): dword sections first, so
// every one of them is 4-byte aligned in the record and a dword of the record never straddles two elements; then
// the narrowed ones (2-byte aligned); then the byte rows.
enum {
    REC_DWORD = 0,  // 4 bytes in the record, the same 4 bytes in the engine
    REC_I16 = 1,    // int16 in the record, int32 in the engine: saturated when packed, sign-extended when restored
    REC_BYTE = 2,   // 1 byte in both
};
#define REC_MAX_SEC 20  // SNAP_NSEC + 3 (zs_snapshot.hpp): the longest record, a ZS_FLAG_ENV_PARAMS | ZS_FLAG_EPISODE_STATS | ZS_FLAG_RENDER handle's

// Entry nsec of every array stands for the padding (no base, REC_BYTE), so an index that rec_find returns is
// always inside the arrays.  No section of a table is empty (rec_table leaves empty ones out): the byte after
// an element lies in the element's section or in the next one.
struct RecTable {
    uint8_t* base[REC_MAX_SEC + 1];
    size_t estride[REC_MAX_SEC + 1];  // bytes from env e's first element to env e + 1's
    size_t kstride[REC_MAX_SEC + 1];  // bytes from element k to element k + 1 of one env
    int off[REC_MAX_SEC + 2];         // record offset of section s; off[nsec]: the zero padding; INT32_MAX from there on
    uint8_t kind[REC_MAX_SEC + 1];
    int nsec;
    int rec_bytes;  // a multiple of 16
};

// One engine array of a record: its base, elements per env of an env-major [N][row] array (0: a [k][N] column
// array) and the element kind.
struct RecSection {
    void* base;
    size_t row;
    int kind;
};

// The table of nsec sections (in record order) of a handle of N envs; off[nsec + 1]: the layout's section offsets
// and the padding's.  The asserts are the walker's rules, properties of a layout and its list of kinds: no more
// sections than a table holds, kinds in order, every element aligned in the record, and rec_bytes the sections'
// bytes rounded up to 16.
inline RecTable rec_table(const RecSection* sec, const int* off, int nsec, int rec_bytes, size_t N) {
    assert(nsec >= 0 && nsec <= REC_MAX_SEC && off[nsec] >= 0 && rec_bytes == ((off[nsec] + 15) & ~15));
    RecTable T;
    int n = 0;
    for (int s = 0; s < nsec; s++) {
        const int kind = sec[s].kind;
        const size_t es = kind == REC_BYTE ? 1 : 4;  // the engine's element
        assert(kind >= (s ? sec[s - 1].kind : REC_DWORD) && kind <= REC_BYTE);
        assert((off[s] & (kind == REC_DWORD ? 3 : kind == REC_I16 ? 1 : 0)) == 0 && off[s] <= off[s + 1]);
        if (off[s] == off[s + 1]) continue;  // an empty section (a map without obstacles)
        T.base[n] = (uint8_t*)sec[s].base;
        T.estride[n] = sec[s].row ? sec[s].row * es : es;
        T.kstride[n] = sec[s].row ? es : N * es;
        T.kind[n] = (uint8_t)kind;
        T.off[n++] = off[s];
    }
    for (int s = n; s <= REC_MAX_SEC; s++) T.base[s] = nullptr, T.estride[s] = T.kstride[s] = 1, T.kind[s] = REC_BYTE;
    T.off[n] = off[nsec];
    for (int s = n + 1; s < REC_MAX_SEC + 2; s++) T.off[s] = INT32_MAX;
    T.nsec = n;
    T.rec_bytes = rec_bytes;
    return T;
}

// The record side of a chunk (the kernels cast uint4 records to it) and an aligned 16 B of an engine row: four
// uint32_t, 16-byte aligned (a compiler's vector of them rather than a struct, so that it can be read through
// REC_MEM pointers).
typedef uint32_t RecChunk __attribute__((vector_size(16), may_alias));

// The engine's arrays are global memory.  Saying so on the device keeps the copies off the flat path, where an
// access counts against the LDS reads as well and a chunk's table lookups would wait for the copies before them
// (measured once, when this was introduced: restore of 65 536 C3 envs 302 us through generic pointers, 278 us so).
#if defined(__HIP_DEVICE_COMPILE__)
#define REC_MEM __attribute__((address_space(1)))
#else
#define REC_MEM
#endif

// the section of record byte b (nsec: the padding); sections are in record order.  Unrolled over constant
// indices: on a table that is a kernel's own argument the offsets are scalar registers, the search reads no
// memory, and a wave whose lanes are all in an early section (the MT ring's 312 chunks) leaves after one compare
ZS_HD inline int rec_find(const RecTable& F, int b) {
    int s = 0;
    ZS_UNROLL
    for (int i = 1; i <= REC_MAX_SEC; i++) {
        if (b < F.off[i]) break;
        s = i;
    }
    return s;
}

// the engine-side address of record byte b (the first byte of an element) of section s, env e
ZS_HD inline uint8_t* rec_addr(const RecTable& T, int s, size_t e, int b) {
    const int k = (b - T.off[s]) >> (REC_BYTE - T.kind[s]);
    return T.base[s] + e * T.estride[s] + (size_t)k * T.kstride[s];
}

// an int32 as the record's int16
ZS_HD inline uint32_t rec_narrow(uint32_t v) {
    const int32_t x = (int32_t)v;
    return (uint16_t)(int16_t)(x < -32768 ? -32768 : x > 32767 ? 32767 : x);
}

// Chunk c of the record at row <-> env e.  PACK: engine -> record, else record -> engine.  F and T are two copies
// of one table: F is searched (rec_find), T is indexed by section.  A kernel passes its argument and the copy it
// staged in LDS (a lane cannot index registers); everyone else calls the one-table form below.
template <bool PACK>
ZS_HD inline void rec_copy_chunk(const RecTable& F, const RecTable& T, RecChunk* row, size_t e, int c) {
    const int b0 = c << 4;
    RecChunk w = {0u, 0u, 0u, 0u};
    if (!PACK) w = row[c];
    int s = rec_find(F, b0), end = T.off[s + 1];
    if (b0 + 16 <= end && T.kind[s] != REC_BYTE) {  // inside one section of 4-byte engine elements: one address
        REC_MEM uint8_t* p = (REC_MEM uint8_t*)rec_addr(T, s, e, b0);
        const size_t ks = T.kstride[s];
        const bool wide = ks == 4 && ((uintptr_t)p & 15) == 0;  // a row, 16-B aligned on the engine side
        REC_MEM RecChunk* q = (REC_MEM RecChunk*)p;
        if (T.kind[s] == REC_DWORD) {
            if (wide && PACK) row[c] = q[0];
            else if (wide) q[0] = w;
            else {  // a misaligned row, or a column: four dwords
                ZS_UNROLL
                for (int j = 0; j < 4; j++) {
                    if (PACK) w[j] = *(REC_MEM uint32_t*)(p + j * ks);
                    else *(REC_MEM uint32_t*)(p + j * ks) = w[j];
                }
                if (PACK) row[c] = w;
            }
            return;
        }
        if (wide) {  // eight narrowed elements, 32 B of the engine's row
            if (PACK) {
                const RecChunk v[2] = {q[0], q[1]};
                ZS_UNROLL
                for (int j = 0; j < 4; j++)
                    w[j] = rec_narrow(v[j >> 1][2 * (j & 1)]) | (rec_narrow(v[j >> 1][2 * (j & 1) + 1]) << 16);
                row[c] = w;
            } else {
                RecChunk v[2];
                ZS_UNROLL
                for (int j = 0; j < 4; j++) {
                    v[j >> 1][2 * (j & 1)] = (uint32_t)(int32_t)(int16_t)(w[j] & 0xffffu);
                    v[j >> 1][2 * (j & 1) + 1] = (uint32_t)(int32_t)(int16_t)(w[j] >> 16);
                }
                q[0] = v[0], q[1] = v[1];
            }
            return;
        }
    }
    // A chunk that straddles sections, the byte rows, a misaligned narrowed row: an element at a time.  No section is
    // empty, so the next element is in this section or the next one.
    if (!PACK) {
        ZS_UNROLL
        for (int j = 0; j < 4; j++)
            for (int k = 0; k < 4;) {
                const int b = b0 + 4 * j + k;
                if (b >= end) end = T.off[++s + 1];
                if (s >= F.nsec) return;  // padding, up to the record's end: restores nothing
                REC_MEM uint8_t* p = (REC_MEM uint8_t*)rec_addr(T, s, e, b);
                const int kind = T.kind[s];
                if (kind == REC_DWORD) *(REC_MEM uint32_t*)p = w[j];
                else if (kind == REC_I16) *(REC_MEM int32_t*)p = (int16_t)(w[j] >> (8 * k));
                else *p = (uint8_t)(w[j] >> (8 * k));
                k += 4 >> kind;
            }
        return;
    }
    // Packing: unrolled over the chunk's 16 bytes, and an element is only loaded here (v, by its first byte) and put
    // in place below, so that no load waits for the one before it.
    uint32_t v[16], narrowed = 0;
    int next = 0;  // the first byte past the element being loaded
    ZS_UNROLL
    for (int i = 0; i < 16; i++) {
        v[i] = 0;
        if (i < next) continue;
        if (b0 + i >= end) end = T.off[++s + 1];
        if (s >= F.nsec) {  // padding: packs as zero
            next = 16;
            continue;
        }
        REC_MEM uint8_t* p = (REC_MEM uint8_t*)rec_addr(T, s, e, b0 + i);
        const int kind = T.kind[s];
        next = i + (4 >> kind);
        if (kind == REC_BYTE) v[i] = *p;
        else v[i] = *(REC_MEM uint32_t*)p;
        if (kind == REC_I16) narrowed |= 1u << i;
    }
    ZS_UNROLL
    for (int i = 0; i < 16; i++) w[i >> 2] |= ((narrowed >> i) & 1u ? rec_narrow(v[i]) : v[i]) << (8 * (i & 3));
    row[c] = w;
}

template <bool PACK>
ZS_HD inline void rec_copy_chunk(const RecTable& T, RecChunk* row, size_t e, int c) {
    rec_copy_chunk<PACK>(T, T, row, e, c);
}

// ---------------------------------------------------------------------------
// The tables of the two record types, from the engine's arrays in record order (base[], of a handle of N envs).
// ---------------------------------------------------------------------------
// base: ring, dead, obst_hp, obst_present, obst_nonpos, pos, life, serial, scal, hp_dirty, dead_dirty, rngst,
// prev_life, weapon, present, order, listed (SNAP_*); env_params: the [6][N] columns of a ZS_FLAG_ENV_PARAMS handle
// (current triple, then next), whose record holds them between prev_life and the byte rows, else null; ep_run: the
// [2 R + 3][N] dword columns of a ZS_FLAG_EPISODE_STATS handle's running part (zs_episode.hpp ZS_EP_RUN_COLS: a zero
// column, run_ret as dword pairs, run_flags, a zero column), ep_R its R, else null: the record's ep_run section with
// the alignment gap ahead of it, which the first zero column fills when there is one; body_col: the [N][body_bytes]
// rows of a ZS_FLAG_RENDER handle, the record's last byte section, else null
inline RecTable snapshot_rec_table(void* const base[SNAP_NSEC], int E, int O, int DW, int OW, int A, size_t N,
                                   void* env_params = nullptr, void* ep_run = nullptr, int ep_R = 0,
                                   void* body_col = nullptr, int body_bytes = 0) {
    const size_t rows[SNAP_NSEC] = {ZS_SNAP_RING, (size_t)DW, (size_t)O, (size_t)OW, (size_t)OW, (size_t)E, (size_t)E, (size_t)E,
                                    0, 0, 0, 0, 0, (size_t)E, (size_t)E, (size_t)E, 0};
    const SnapshotLayout L = snapshot_layout(E, O, DW, OW, A, env_params != nullptr, ep_run ? ep_R : 0, body_col ? body_bytes : 0);
    RecSection sec[SNAP_NSEC + 3];
    int off[SNAP_NSEC + 4], n = 0;
    for (int s = 0; s < SNAP_NSEC; s++) {
        if (s == SNAP_NWORD && env_params) sec[n] = RecSection{env_params, 0, REC_DWORD}, off[n++] = L.envp;
        if (s == SNAP_NWORD && ep_run)
            sec[n] = RecSection{(uint32_t*)ep_run + (L.ep_gap ? 0 : N), 0, REC_DWORD}, off[n++] = L.ep_run - L.ep_gap;
        sec[n] = RecSection{base[s], rows[s], s < SNAP_NWORD ? REC_DWORD : REC_BYTE}, off[n++] = L.off[s];
    }
    if (body_col && body_bytes > 0) sec[n] = RecSection{body_col, (size_t)body_bytes, REC_BYTE}, off[n++] = L.body_col;
    off[n] = L.off[SNAP_NSEC];
    return rec_table(sec, off, n, L.rec_bytes, N);
}

// base: hp_dirty, dead_dirty, pos, life, dead, obst_present, obst_hp, weapon, present; L: obs_state_layout()
inline RecTable obs_state_rec_table(void* const base[9], const ObsStateLayout& L, int E, int O, int DW, int OW, size_t N) {
    const size_t rows[9] = {0, 0, (size_t)E, (size_t)E, (size_t)DW, (size_t)OW, (size_t)O, (size_t)E, (size_t)E};
    const int off[10] = {L.hp_dirty, L.dead_dirty, L.pos, L.life, L.dead, L.obst_present, L.obst_hp, L.weapon, L.present, L.pad};
    RecSection sec[9];
    for (int s = 0; s < 9; s++) sec[s] = RecSection{base[s], rows[s], s < 6 ? REC_DWORD : s > 6 ? REC_BYTE : L.hp_bytes == 2 ? REC_I16 : REC_DWORD};
    return rec_table(sec, off, 9, L.rec_bytes, N);
}
