// Host program of tests/test_record_copy.py: the record walker of libzombsole_amd/csrc/zs_record.hpp, compiled with the
// host compiler, on host arrays shaped like the engine's.  One JSON line per input line:
//   "S E O DW OW A N"           the snapshot record (zs_snapshot.hpp)
//   "O E O DW OW A N hp_bytes"  the observation-state record (zs_obs_state.hpp) with 4- or 2-byte obstacle HP
// Per line, four times over (array i of 17 starts 4 * ((i + round) % 4) bytes past a 16-B boundary): every env is
// packed by rec_copy_chunk<true> chunk by chunk and compared byte for byte with a record put together element by
// element from the layout comments of the two headers (not from the table, not by the walker); then the records of
// envs [env0, env0 + n) are unpacked by rec_copy_chunk<false> into arrays filled otherwise, which must equal the
// source inside the range (a narrowed life: max(life, -32768)) and their former selves everywhere else, guard bytes
// included.  -> {"ok": true, "rec_bytes", "chunks", "nsec"} or {"ok": false, "error"}.
#include <stdio.h>
#include <string.h>

#include <string>
#include <vector>

#include "zs_obs_state.hpp"
#include "zs_record.hpp"
#include "zs_snapshot.hpp"

enum { GUARD = 64 };

// one engine array: [N][row] elements (row > 0) or [cols][N] (row == 0), of 4- or 1-byte elements, between guard bytes
struct Arr {
    int id = 0, es = 4;
    size_t row = 0, per_env = 0, N = 0;
    std::vector<uint8_t> buf;
    size_t lead = 0;  // buf[lead]: the array's first byte

    void make(int id_, int es_, size_t row_, size_t cols, size_t N_, int shift, uint8_t guard) {
        id = id_, es = es_, row = row_, per_env = row_ ? row_ : cols, N = N_;
        buf.assign(GUARD + 32 + es * per_env * N + GUARD, guard);
        lead = GUARD;
        while ((uintptr_t)(buf.data() + lead) & 15) lead++;
        lead += shift;
    }
    uint8_t* base() { return buf.data() + lead; }
    uint8_t* at(size_t e, size_t k) { return base() + (row ? e * row + k : k * N + e) * es; }
    uint32_t get(size_t e, size_t k) {
        uint32_t v = 0;
        memcpy(&v, at(e, k), es);  // little-endian host, like the device
        return v;
    }
    void set(size_t e, size_t k, uint32_t v) { memcpy(at(e, k), &v, es); }
};

enum { A_RING, A_DEAD, A_OBST_HP, A_OBST_PRESENT, A_OBST_NONPOS, A_POS, A_LIFE, A_SERIAL, A_SCAL, A_HP_DIRTY, A_DEAD_DIRTY,
       A_RNGST, A_PREV_LIFE, A_WEAPON, A_PRESENT, A_ORDER, A_LISTED, A_COUNT };

struct Shape {
    int E, O, DW, OW, A, N;
};

static uint32_t pattern(uint32_t a, uint32_t e, uint32_t k, uint32_t salt) {
    uint32_t x = (a + 1) * 0x9E3779B1u ^ (e + 1) * 0x85EBCA77u ^ (k + 1) * 0xC2B2AE3Du ^ salt * 0x27D4EB2Fu;
    x ^= x >> 15, x *= 0x2C1B3C6Du, x ^= x >> 12;
    return x;
}

struct Arrays {
    Arr a[A_COUNT];

    Arrays(const Shape& s, int round, uint32_t salt, uint8_t guard) {
        const size_t E = s.E, N = s.N;
        const struct { int es; size_t row, cols; } dims[A_COUNT] = {
            {4, ZS_SNAP_RING, 0}, {4, (size_t)s.DW, 0}, {4, (size_t)s.O, 0}, {4, (size_t)s.OW, 0}, {4, (size_t)s.OW, 0},
            {4, E, 0}, {4, E, 0}, {4, E, 0}, {4, 0, ZS_SNAP_NSCAL}, {4, 0, 1}, {4, 0, 1}, {4, 0, 1}, {4, 0, (size_t)s.A},
            {1, E, 0}, {1, E, 0}, {1, E, 0}, {1, 0, (size_t)s.A}};
        static const int32_t lives[5] = {-32700, -32768, -32769, -40000, -33000};  // tests/test_obs_state.py
        for (int i = 0; i < A_COUNT; i++) {
            Arr& x = a[i];
            x.make(i, dims[i].es, dims[i].row, dims[i].cols, N, 4 * ((i + round) % 4), guard);
            for (size_t e = 0; e < N; e++)
                for (size_t k = 0; k < x.per_env; k++) {
                    uint32_t v = pattern(i, e, k, salt);
                    if (i == A_OBST_HP)  // lives on both sides of the int16 floor, none above its ceiling
                        v = k % 8 < 5 ? (uint32_t)(lives[k % 8] + (k % 8 == 3 ? (int32_t)e : 0)) : (uint32_t)((int32_t)(v % 60000u) - 50000);
                    x.set(e, k, v);
                }
        }
    }
};

static void put32(std::vector<uint8_t>& r, uint32_t v) {
    for (int k = 0; k < 4; k++) r.push_back((uint8_t)(v >> (8 * k)));
}
static void put_row(std::vector<uint8_t>& r, Arr& x, size_t e) {
    for (size_t k = 0; k < x.per_env; k++) {
        if (x.es == 4) put32(r, x.get(e, k));
        else r.push_back((uint8_t)x.get(e, k));
    }
}

// env e's record, element by element, in the order of the header's layout comment; hp_bytes 0: the snapshot record
static std::vector<uint8_t> reference(Arrays& s, size_t e, int hp_bytes) {
    std::vector<uint8_t> r;
    Arr* a = s.a;
    if (hp_bytes == 0) {
        put_row(r, a[A_RING], e), put_row(r, a[A_DEAD], e), put_row(r, a[A_OBST_HP], e), put_row(r, a[A_OBST_PRESENT], e);
        put_row(r, a[A_OBST_NONPOS], e), put_row(r, a[A_POS], e), put_row(r, a[A_LIFE], e), put_row(r, a[A_SERIAL], e);
        put_row(r, a[A_SCAL], e), put_row(r, a[A_HP_DIRTY], e), put_row(r, a[A_DEAD_DIRTY], e), put_row(r, a[A_RNGST], e);
        put_row(r, a[A_PREV_LIFE], e);
        put_row(r, a[A_WEAPON], e), put_row(r, a[A_PRESENT], e), put_row(r, a[A_ORDER], e), put_row(r, a[A_LISTED], e);
    } else {
        put_row(r, a[A_HP_DIRTY], e), put_row(r, a[A_DEAD_DIRTY], e), put_row(r, a[A_POS], e), put_row(r, a[A_LIFE], e);
        put_row(r, a[A_DEAD], e), put_row(r, a[A_OBST_PRESENT], e);
        if (hp_bytes == 4) put_row(r, a[A_OBST_HP], e);
        else
            for (size_t k = 0; k < a[A_OBST_HP].per_env; k++) {
                const int32_t life = (int32_t)a[A_OBST_HP].get(e, k);
                const uint16_t v = (uint16_t)(int16_t)(life < -32768 ? -32768 : life);
                r.push_back((uint8_t)v), r.push_back((uint8_t)(v >> 8));
            }
        put_row(r, a[A_WEAPON], e), put_row(r, a[A_PRESENT], e);
    }
    while (r.size() % 16) r.push_back(0);
    return r;
}

// the table of the arrays `s`, by the helpers the engine builds its own with; members: the arrays of the record
static RecTable table(Arrays& s, const Shape& sh, int hp_bytes, std::vector<int>* members) {
    if (hp_bytes == 0) {
        void* base[SNAP_NSEC];
        for (int i = 0; i < A_COUNT; i++) base[i] = s.a[i].base(), members->push_back(i);
        return snapshot_rec_table(base, sh.E, sh.O, sh.DW, sh.OW, sh.A, (size_t)sh.N);
    }
    static const int ids[9] = {A_HP_DIRTY, A_DEAD_DIRTY, A_POS, A_LIFE, A_DEAD, A_OBST_PRESENT, A_OBST_HP, A_WEAPON, A_PRESENT};
    void* base[9];
    for (int k = 0; k < 9; k++) base[k] = s.a[ids[k]].base(), members->push_back(ids[k]);
    const ObsStateLayout L = obs_state_layout(sh.E, sh.O, sh.DW, sh.OW, hp_bytes == 2 ? ZS_DTYPE_I16 : ZS_DTYPE_I32);
    return obs_state_rec_table(base, L, sh.E, sh.O, sh.DW, sh.OW, (size_t)sh.N);
}

static std::string run(const Shape& sh, int hp_bytes, int round, int* rec_bytes, int* nsec) {
    const size_t N = sh.N;
    Arrays src(sh, round, 1, 0xA5);
    const Arrays src0 = src;
    std::vector<int> members;
    const RecTable T = table(src, sh, hp_bytes, &members);
    *rec_bytes = T.rec_bytes, *nsec = T.nsec;
    const size_t nb = T.rec_bytes, nch = nb / 16;

    std::vector<uint8_t> recbuf(GUARD + 16 + N * nb + GUARD, 0xCC);
    size_t lead = GUARD;
    while ((uintptr_t)(recbuf.data() + lead) & 15) lead++;
    uint8_t* rec = recbuf.data() + lead;
    for (size_t e = 0; e < N; e++)
        for (size_t c = 0; c < nch; c++) rec_copy_chunk<true>(T, (RecChunk*)(rec + e * nb), e, (int)c);
    for (size_t e = 0; e < N; e++) {
        const std::vector<uint8_t> ref = reference(src, e, hp_bytes);
        if (ref.size() != nb) return "the reference record's size differs from rec_bytes";
        for (size_t b = 0; b < nb; b++)
            if (rec[e * nb + b] != ref[b]) return "pack: env " + std::to_string(e) + " byte " + std::to_string(b) + " differs";
        for (size_t b = T.off[T.nsec]; b < nb; b++)
            if (rec[e * nb + b] != 0) return "pack: padding is not zero";
    }
    for (size_t b = 0; b < recbuf.size(); b++)
        if ((b < lead || b >= lead + N * nb) && recbuf[b] != 0xCC) return "pack: wrote outside the records";
    for (int i = 0; i < A_COUNT; i++)
        if (src.a[i].buf != src0.a[i].buf) return "pack: wrote to the engine arrays";

    // records of envs [env0, env0 + n) into arrays filled otherwise
    const size_t env0 = N > 1 ? 1 : 0, n = N > 2 ? N - 2 : 1;
    Arrays dst(sh, round, 2, 0x5A);
    Arrays want = dst;
    for (int i : members)
        for (size_t e = env0; e < env0 + n; e++)
            for (size_t k = 0; k < src.a[i].per_env; k++) {
                uint32_t v = src.a[i].get(e, k);
                if (i == A_OBST_HP && hp_bytes == 2 && (int32_t)v < -32768) v = (uint32_t)-32768;
                want.a[i].set(e, k, v);
            }
    std::vector<int> again;
    const RecTable D = table(dst, sh, hp_bytes, &again);
    const std::vector<uint8_t> recbuf0 = recbuf;
    for (size_t e = env0; e < env0 + n; e++)
        for (size_t c = 0; c < nch; c++) rec_copy_chunk<false>(D, (RecChunk*)(rec + e * nb), e, (int)c);
    if (recbuf != recbuf0) return "unpack: wrote to the records";
    for (int i = 0; i < A_COUNT; i++)
        for (size_t b = 0; b < dst.a[i].buf.size(); b++)
            if (dst.a[i].buf[b] != want.a[i].buf[b])
                return "unpack: array " + std::to_string(i) + " differs at byte " + std::to_string((long)b - (long)dst.a[i].lead) +
                       " of " + std::to_string(dst.a[i].es * dst.a[i].per_env * N);
    return "";
}

int main(void) {
    char kind;
    while (scanf(" %c", &kind) == 1) {
        Shape sh;
        int hp_bytes = 0;
        if (scanf("%d %d %d %d %d %d", &sh.E, &sh.O, &sh.DW, &sh.OW, &sh.A, &sh.N) != 6) return 1;
        if (kind == 'O' && (scanf("%d", &hp_bytes) != 1 || (hp_bytes != 2 && hp_bytes != 4))) return 1;
        if (kind != 'S' && kind != 'O') return 1;
        std::string err;
        int rec_bytes = 0, nsec = 0;
        for (int round = 0; round < 4 && err.empty(); round++) {
            err = run(sh, hp_bytes, round, &rec_bytes, &nsec);
            if (!err.empty()) err = "round " + std::to_string(round) + ": " + err;
        }
        if (err.empty()) printf("{\"ok\": true, \"rec_bytes\": %d, \"chunks\": %d, \"nsec\": %d}\n", rec_bytes, rec_bytes / 16, nsec);
        else printf("{\"ok\": false, \"error\": \"%s\"}\n", err.c_str());
    }
    return 0;
}
