// Host program of tests/test_env_params_plan.py: the snapshot record with and without the env_params section
// (libzombsole_amd/csrc/zs_snapshot.hpp, zs_record.hpp), compiled with the host compiler.  One JSON line per input line:
//   "L E O DW OW A flag"   -> snapshot_layout(E, O, DW, OW, A, flag): every section's offset, "env_params" (0: none),
//                             "pad", "rec_bytes"
//   "W E O DW OW A N"      -> the record walker over a flagged handle's table (snapshot_rec_table with the [6][N]
//                             env_params columns): every env packed chunk by chunk; the six words at the layout's
//                             env_params offset must be the env's column, every other byte what the unflagged table
//                             packs at the offset less 24 (sections behind env_params) or at the same one (before it);
//                             then unpacked into zeroed arrays, which must equal the source.  {"ok", "nsec", "rec_bytes"}
#include <stdio.h>
#include <string.h>

#include <string>
#include <vector>

#include "zs_record.hpp"
#include "zs_snapshot.hpp"

static const char* names[SNAP_NSEC] = {"ring", "dead", "obst_hp", "obst_present", "obst_nonpos", "pos", "life", "serial", "scal",
                                       "hp_dirty", "dead_dirty", "rngst", "prev_life", "weapon", "present", "order", "listed"};

struct Host {
    std::vector<std::vector<uint32_t>> a;  // 16-B aligned enough: vectors of uint32_t, byte rows included
    std::vector<uint32_t> envp;
    void* base[SNAP_NSEC];
    Host(int E, int O, int DW, int OW, int A, int N, uint32_t salt) {
        const size_t words[SNAP_NSEC] = {(size_t)ZS_SNAP_RING * N, (size_t)DW * N, (size_t)O * N, (size_t)OW * N, (size_t)OW * N,
                                         (size_t)E * N, (size_t)E * N, (size_t)E * N, (size_t)ZS_SNAP_NSCAL * N, (size_t)N,
                                         (size_t)N, (size_t)N, (size_t)A * N,
                                         ((size_t)E * N + 3) / 4, ((size_t)E * N + 3) / 4, ((size_t)E * N + 3) / 4, ((size_t)A * N + 3) / 4};
        a.resize(SNAP_NSEC);
        for (int s = 0; s < SNAP_NSEC; s++) {
            a[s].assign(words[s] + 4, 0u);
            if (salt)
                for (size_t k = 0; k < words[s]; k++) a[s][k] = (uint32_t)(s + 1) * 0x9E3779B1u ^ (uint32_t)(k + 1) * 0x85EBCA77u ^ salt;
            base[s] = a[s].data();
        }
        envp.assign((size_t)ZS_SNAP_ENVP * N + 4, 0u);
        if (salt)
            for (size_t k = 0; k < (size_t)ZS_SNAP_ENVP * N; k++) envp[k] = 0xE0000000u + (uint32_t)k * 7u + salt;
    }
};

static std::string walk(int E, int O, int DW, int OW, int A, int N, int* nsec, int* rec_bytes) {
    Host src(E, O, DW, OW, A, N, 1);
    const RecTable T = snapshot_rec_table(src.base, E, O, DW, OW, A, (size_t)N, src.envp.data());
    const RecTable U = snapshot_rec_table(src.base, E, O, DW, OW, A, (size_t)N);
    const SnapshotLayout L = snapshot_layout(E, O, DW, OW, A, true), L0 = snapshot_layout(E, O, DW, OW, A);
    *nsec = T.nsec, *rec_bytes = T.rec_bytes;
    if (T.rec_bytes != L.rec_bytes || U.rec_bytes != L0.rec_bytes) return "table and layout differ in rec_bytes";
    std::vector<uint32_t> rec((size_t)N * T.rec_bytes / 4 + 4, 0xCCCCCCCCu), rec0((size_t)N * U.rec_bytes / 4 + 4, 0xCCCCCCCCu);
    uint8_t *r = (uint8_t*)rec.data(), *r0 = (uint8_t*)rec0.data();
    while ((uintptr_t)r & 15) r++;
    while ((uintptr_t)r0 & 15) r0++;
    for (int e = 0; e < N; e++) {
        for (int c = 0; c < T.rec_bytes / 16; c++) rec_copy_chunk<true>(T, (RecChunk*)(r + (size_t)e * T.rec_bytes), (size_t)e, c);
        for (int c = 0; c < U.rec_bytes / 16; c++) rec_copy_chunk<true>(U, (RecChunk*)(r0 + (size_t)e * U.rec_bytes), (size_t)e, c);
        const uint8_t *p = r + (size_t)e * T.rec_bytes, *p0 = r0 + (size_t)e * U.rec_bytes;
        for (int k = 0; k < ZS_SNAP_ENVP; k++) {
            uint32_t v;
            memcpy(&v, p + L.envp + 4 * k, 4);
            if (v != src.envp[(size_t)k * N + e]) return "env_params word " + std::to_string(k) + " of env " + std::to_string(e);
        }
        if (memcmp(p, p0, L.envp) != 0) return "the sections before env_params differ from the unflagged record";
        if (memcmp(p + L.envp + 4 * ZS_SNAP_ENVP, p0 + L.envp, L0.off[SNAP_NSEC] - L.envp) != 0)
            return "the sections behind env_params differ from the unflagged record";
        for (int b = L.off[SNAP_NSEC]; b < T.rec_bytes; b++)
            if (p[b]) return "padding is not zero";
    }
    Host dst(E, O, DW, OW, A, N, 0);
    const RecTable D = snapshot_rec_table(dst.base, E, O, DW, OW, A, (size_t)N, dst.envp.data());
    for (int e = 0; e < N; e++)
        for (int c = 0; c < D.rec_bytes / 16; c++) rec_copy_chunk<false>(D, (RecChunk*)(r + (size_t)e * D.rec_bytes), (size_t)e, c);
    const size_t used[SNAP_NSEC] = {(size_t)4 * ZS_SNAP_RING * N, (size_t)4 * DW * N, (size_t)4 * O * N, (size_t)4 * OW * N, (size_t)4 * OW * N,
                                    (size_t)4 * E * N, (size_t)4 * E * N, (size_t)4 * E * N, (size_t)4 * ZS_SNAP_NSCAL * N, (size_t)4 * N,
                                    (size_t)4 * N, (size_t)4 * N, (size_t)4 * A * N, (size_t)E * N, (size_t)E * N, (size_t)E * N, (size_t)A * N};
    for (int s = 0; s < SNAP_NSEC; s++)
        if (memcmp(dst.a[s].data(), src.a[s].data(), used[s]) != 0) return std::string("unpack: ") + names[s] + " differs";
    if (memcmp(dst.envp.data(), src.envp.data(), (size_t)4 * ZS_SNAP_ENVP * N) != 0) return "unpack: env_params differs";
    return "";
}

int main(void) {
    char kind;
    while (scanf(" %c", &kind) == 1) {
        int E, O, DW, OW, A, x;
        if (scanf("%d %d %d %d %d %d", &E, &O, &DW, &OW, &A, &x) != 6) return 1;
        if (kind == 'L') {
            const SnapshotLayout L = snapshot_layout(E, O, DW, OW, A, x != 0);
            printf("{");
            for (int s = 0; s < SNAP_NSEC; s++) printf("\"%s\": %d, ", names[s], L.off[s]);
            printf("\"env_params\": %d, \"pad\": %d, \"rec_bytes\": %d}\n", L.envp, L.off[SNAP_NSEC], L.rec_bytes);
        } else if (kind == 'W') {
            int nsec = 0, rec_bytes = 0;
            const std::string err = walk(E, O, DW, OW, A, x, &nsec, &rec_bytes);
            if (err.empty()) printf("{\"ok\": true, \"nsec\": %d, \"rec_bytes\": %d}\n", nsec, rec_bytes);
            else printf("{\"ok\": false, \"error\": \"%s\"}\n", err.c_str());
        } else {
            return 1;
        }
    }
    return 0;
}
