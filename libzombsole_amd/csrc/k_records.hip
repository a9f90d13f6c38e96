// k_records.hip — the per-env record movers: observation-state records (zs_obs_state.hpp: k_obs_state_pack,
// k_obs_state_unpack) and snapshot records (zs_snapshot.hpp, by the record walker of zs_record.hpp: k_snapshot,
// k_restore, k_pending_list).
#include <algorithm>

#include "zs_launch.hpp"
#include "zs_obs_state.hpp"
#include "zs_snapshot.hpp"
#include "zs_record.hpp"

// ---------------------------------------------------------------------------
// observation-state records (zs_obs_state.hpp): k_obs_state_pack copies the nine per-env arrays the
// observation encoders read into one record per env, k_obs_state_unpack copies records into a viewer's envs.
// Both walk a record in 16-B chunks, `wpe` waves of a 256-thread workgroup per env (1: four envs per
// workgroup, 4: one), grid-stride over envs.  The record side is 16-B aligned (one 16-B store / load per
// chunk).  The engine side is not: a [N][E] int32 row starts at byte 4 e E and a section at any 4-B offset
// of the record, so a chunk inside one 4-byte section moves as 16 B when its engine address allows and as
// four dwords otherwise; eight int16 HP elements of a record chunk are 32 B of the env's int32 row (two 16-B
// accesses when aligned, else eight dwords); the u8 rows and a chunk that straddles sections move by element.
// ---------------------------------------------------------------------------
// the engine-side word of the record's dword at byte b (b % 4 == 0, b inside the 4-byte sections); *sec: its section
__device__ __forceinline__ uint32_t* os_word(const Dev& d, const ObsStateLayout& L, size_t e, int b, int* sec) {
    if (b >= L.obst_hp) return *sec = 6, (uint32_t*)d.obst_hp + e * d.O + ((b - L.obst_hp) >> 2);
    if (b >= L.obst_present) return *sec = 5, d.obst_present + e * d.OW + ((b - L.obst_present) >> 2);
    if (b >= L.dead) return *sec = 4, d.dead + e * d.DW + ((b - L.dead) >> 2);
    if (b >= L.life) return *sec = 3, (uint32_t*)d.life + e * d.E + ((b - L.life) >> 2);
    if (b >= L.pos) return *sec = 2, (uint32_t*)d.pos + e * d.E + ((b - L.pos) >> 2);
    if (b >= L.dead_dirty) return *sec = 1, d.dead_dirty + e;
    return *sec = 0, d.hp_dirty + e;
}

// the record's two bytes at p (p % 2 == 0) past the 4-byte sections: an int16 HP element, u8 rows, padding
__device__ __forceinline__ uint32_t os_tail_get(const Dev& d, const ObsStateLayout& L, size_t e, int p) {
    if (p < L.weapon) return (uint16_t)(int16_t)max(-32768, min(d.obst_hp[e * d.O + ((p - L.obst_hp) >> 1)], 32767));
    uint32_t v = 0;
    for (int k = 0; k < 2; k++) {
        const int q = p + k;
        const uint32_t by = q < L.present ? d.weapon[e * d.E + (q - L.weapon)] : q < L.pad ? d.present[e * d.E + (q - L.present)] : 0u;
        v |= by << (8 * k);
    }
    return v;
}
__device__ __forceinline__ void os_tail_put(const Dev& d, const ObsStateLayout& L, size_t e, int p, uint32_t v) {
    if (p < L.weapon) {
        d.obst_hp[e * d.O + ((p - L.obst_hp) >> 1)] = (int32_t)(int16_t)(v & 0xffffu);
        return;
    }
    for (int k = 0; k < 2; k++) {
        const int q = p + k;
        const uint8_t by = (uint8_t)(v >> (8 * k));
        if (q < L.present) d.weapon[e * d.E + (q - L.weapon)] = by;
        else if (q < L.pad) d.present[e * d.E + (q - L.present)] = by;
    }
}

// rec [n][L.rec_bytes]: record r is env env0 + r of the handle; PACK: engine -> record, else record -> engine
template <bool PACK>
__device__ __forceinline__ void obs_state_copy(const Dev& d, const ObsStateLayout& L, int wpe, int env0, int n, uint4* rec) {
    const int team = wpe * 64, per_wg = 256 / team;
    const int t = threadIdx.x % team;
    const int nch = L.rec_bytes >> 4;
    const int words_end = L.hp_bytes == 4 ? L.weapon : L.obst_hp;  // end of the 4-byte sections
    for (int r = blockIdx.x * per_wg + threadIdx.x / team; r < n; r += gridDim.x * per_wg) {
        const size_t e = (size_t)(env0 + r);
        uint4* row = rec + (size_t)r * nch;
        for (int c = t; c < nch; c += team) {
            const int b0 = c << 4;
            uint32_t w[4];
            if (!PACK) {
                const uint4 v = row[c];
                w[0] = v.x, w[1] = v.y, w[2] = v.z, w[3] = v.w;
            }
            if (b0 + 16 <= words_end) {
                int s0, s3;
                uint32_t* p0 = os_word(d, L, e, b0, &s0);
                (void)os_word(d, L, e, b0 + 12, &s3);
                if (s0 == s3 && ((uintptr_t)p0 & 15) == 0) {  // one section, 16-B aligned on the engine side
                    if (PACK) row[c] = *(const uint4*)p0;
                    else *(uint4*)p0 = uint4{w[0], w[1], w[2], w[3]};
                    continue;
                }
            }
            if (L.hp_bytes == 2 && b0 >= L.obst_hp && b0 + 16 <= L.weapon) {
                // eight int16 HP elements of the record = 32 B of the env's int32 row, all loads issued first
                int32_t* p = d.obst_hp + e * d.O + ((b0 - L.obst_hp) >> 1);
                const bool al = ((uintptr_t)p & 15) == 0;
                int v[8];
                if (PACK) {
                    if (al) {
                        const int4 lo = ((const int4*)p)[0], hi = ((const int4*)p)[1];
                        v[0] = lo.x, v[1] = lo.y, v[2] = lo.z, v[3] = lo.w, v[4] = hi.x, v[5] = hi.y, v[6] = hi.z, v[7] = hi.w;
                    } else {
#pragma unroll
                        for (int k = 0; k < 8; k++) v[k] = p[k];
                    }
#pragma unroll
                    for (int j = 0; j < 4; j++)
                        w[j] = (uint32_t)(uint16_t)(int16_t)max(-32768, min(v[2 * j], 32767)) |
                               ((uint32_t)(uint16_t)(int16_t)max(-32768, min(v[2 * j + 1], 32767)) << 16);
                    row[c] = uint4{w[0], w[1], w[2], w[3]};
                } else {
#pragma unroll
                    for (int j = 0; j < 4; j++) v[2 * j] = (int16_t)(w[j] & 0xffffu), v[2 * j + 1] = (int16_t)(w[j] >> 16);
                    if (al) {
                        ((int4*)p)[0] = int4{v[0], v[1], v[2], v[3]};
                        ((int4*)p)[1] = int4{v[4], v[5], v[6], v[7]};
                    } else {
#pragma unroll
                        for (int k = 0; k < 8; k++) p[k] = v[k];
                    }
                }
                continue;
            }
#pragma unroll
            for (int j = 0; j < 4; j++) {
                const int b = b0 + 4 * j;
                if (b < words_end) {
                    int s;
                    uint32_t* p = os_word(d, L, e, b, &s);
                    if (PACK) w[j] = *p;
                    else *p = w[j];
                } else if (PACK) {
                    w[j] = os_tail_get(d, L, e, b) | (os_tail_get(d, L, e, b + 2) << 16);
                } else {
                    os_tail_put(d, L, e, b, w[j]);
                    os_tail_put(d, L, e, b + 2, w[j] >> 16);
                }
            }
            if (PACK) row[c] = uint4{w[0], w[1], w[2], w[3]};
        }
    }
}

__global__ __launch_bounds__(256) void k_obs_state_pack(Dev d, ObsStateLayout L, int wpe, int n, uint4* rec) {
    obs_state_copy<true>(d, L, wpe, 0, n, rec);
}
__global__ __launch_bounds__(256) void k_obs_state_unpack(Dev d, ObsStateLayout L, int wpe, int env0, int n, const uint4* rec) {
    obs_state_copy<false>(d, L, wpe, env0, n, (uint4*)rec);
}

// ---------------------------------------------------------------------------
// snapshot records (zs_snapshot.hpp): k_snapshot copies everything per-env into one record per entry,
// k_restore copies records back into envs, k_pending_list rebuilds the pending-reset list from the flags.
// One 256-thread workgroup per entry (the MT ring alone is 312 chunks), grid-stride over entries; each kernel is a
// loop over (record, 16-B chunk) that calls the record walker (zs_record.hpp: the section table and
// rec_copy_chunk).  The table comes by value (the section search reads it there, in scalar registers) and is
// staged in LDS so a lane can index it by section.
// ---------------------------------------------------------------------------
static_assert(ZS_SNAP_NSCAL == S_NSCAL && ZS_SNAP_RING == ZS_RING_WORDS, "zs_snapshot.hpp mirrors zs_device.hpp");
static_assert(SNAP_NSEC + 3 <= REC_MAX_SEC, "a snapshot record's sections (with env_params, ep_run and body_col) fit a table");
static_assert(ZS_SNAP_ENVP == 2 * EP_N, "the env_params section is both triples");

__device__ __forceinline__ void rec_stage_table(const RecTable& arg, RecTable* lds) {
    static_assert(sizeof(RecTable) % 4 == 0, "dword copy");
    const uint32_t* src = (const uint32_t*)&arg;
    for (int k = threadIdx.x; k < (int)(sizeof(RecTable) / 4); k += blockDim.x) ((uint32_t*)lds)[k] = src[k];
    __syncthreads();
}

// record k = env idx[k] (idx NULL: env k); an index outside [0, N) is skipped
__global__ __launch_bounds__(256) void k_snapshot(RecTable tab, int N, const int32_t* idx, int n, uint4* rec) {
    __shared__ RecTable T;
    rec_stage_table(tab, &T);
    const int nch = tab.rec_bytes >> 4;
    for (int k = blockIdx.x; k < n; k += gridDim.x) {
        const int e = idx ? idx[k] : k;
        if ((unsigned)e >= (unsigned)N) continue;
        RecChunk* row = (RecChunk*)(rec + (size_t)k * nch);
        for (int c = threadIdx.x; c < nch; c += 256) rec_copy_chunk<true>(tab, T, row, (size_t)e, c);
    }
}

// record src[k] (NULL: k) of the n_records at rec into env dst[k] (NULL: k); an entry whose record or env is out
// of range is skipped.  The written envs' log counts are zeroed (the logs are a step's outputs), and *list_count
// for k_pending_list, which follows on the stream.
__global__ __launch_bounds__(256) void k_restore(RecTable tab, int N, int32_t* dlog_n, int32_t* alog_n, const int32_t* src,
                                                 const int32_t* dst, int n, int n_records, const uint4* rec, int* list_count) {
    __shared__ RecTable T;
    rec_stage_table(tab, &T);
    if (blockIdx.x == 0 && threadIdx.x == 0) *list_count = 0;
    const int nch = tab.rec_bytes >> 4;
    for (int k = blockIdx.x; k < n; k += gridDim.x) {
        const int r = src ? src[k] : k, e = dst ? dst[k] : k;
        if ((unsigned)r >= (unsigned)n_records || (unsigned)e >= (unsigned)N) continue;
        RecChunk* row = (RecChunk*)rec + (size_t)r * nch;
        for (int c = threadIdx.x; c < nch; c += 256) rec_copy_chunk<false>(tab, T, row, (size_t)e, c);
        if (threadIdx.x == 0 && dlog_n) dlog_n[e] = 0, alog_n[e] = 0;
    }
}

// list = the envs whose S_NEEDRESET is set, in any order (envs are independent); *count starts at zero
// (k_restore).  One atomic per wave: its flagged lanes take consecutive entries.
__global__ __launch_bounds__(256) void k_pending_list(const int32_t* needs_reset, int N, int* list, int* count) {
    const int lane = threadIdx.x & 63;
    for (int e0 = (blockIdx.x * 256 + threadIdx.x) - lane; e0 < N; e0 += gridDim.x * 256) {
        const int e = e0 + lane;
        const bool f = e < N && needs_reset[e] != 0;
        const unsigned long long m = __ballot(f);
        if (!m) continue;
        int base = 0;
        if (lane == 0) base = atomicAdd(count, __popcll(m));
        base = __shfl(base, 0);
        const int k = base + __popcll(m & ((1ull << lane) - 1ull));
        if (f && (unsigned)k < (unsigned)N) list[k] = e;
    }
}

// ---------------------------------------------------------------------------
// host launchers (zs_launch.hpp)
// ---------------------------------------------------------------------------
// waves of a workgroup per env (one wave walks up to four 16-B chunks per lane) and the launch's workgroups
static void obs_state_geometry(const ObsStateLayout& L, int n, int* wpe, unsigned* grid) {
    *wpe = L.rec_bytes > 4 * 64 * 16 ? 4 : 1;
    const int per_wg = 4 / *wpe;
    *grid = (unsigned)std::min((n + per_wg - 1) / per_wg, 256 * 16);  // grid-stride past 16 workgroups per CU
}

hipError_t launch_obs_state_pack(hipStream_t s, const Dev& d, const ObsStateLayout& L, void* rec) {
    int wpe;
    unsigned grid;
    obs_state_geometry(L, d.N, &wpe, &grid);
    hipLaunchKernelGGL(k_obs_state_pack, dim3(grid), dim3(256), 0, s, d, L, wpe, d.N, (uint4*)rec);
    return hipGetLastError();
}

hipError_t launch_obs_state_unpack(hipStream_t s, const Dev& d, const ObsStateLayout& L, int env0, int n, const void* rec) {
    int wpe;
    unsigned grid;
    obs_state_geometry(L, n, &wpe, &grid);
    hipLaunchKernelGGL(k_obs_state_unpack, dim3(grid), dim3(256), 0, s, d, L, wpe, env0, n, (const uint4*)rec);
    return hipGetLastError();
}

// workgroups of a launch over n entries, one entry per workgroup at a time (grid-stride past 16 per CU)
static unsigned snap_grid(int n) { return (unsigned)std::min(n, 256 * 16); }

hipError_t launch_snapshot(hipStream_t s, const RecTable& T, int N, const int32_t* idx, int n, void* rec) {
    hipLaunchKernelGGL(k_snapshot, dim3(snap_grid(n)), dim3(256), 0, s, T, N, idx, n, (uint4*)rec);
    return hipGetLastError();
}

hipError_t launch_restore(hipStream_t s, const RecTable& T, const Dev& d, const int32_t* src, const int32_t* dst, int n,
                          int n_records, const void* rec, int* list_count) {
    hipLaunchKernelGGL(k_restore, dim3(snap_grid(n)), dim3(256), 0, s, T, d.N, d.dlog_n, d.alog_n, src, dst, n, n_records,
                       (const uint4*)rec, list_count);
    return hipGetLastError();
}

hipError_t launch_pending_list(hipStream_t s, const int32_t* needs_reset, int N, int* list, int* count) {
    hipLaunchKernelGGL(k_pending_list, dim3((unsigned)std::min(64, (N + 255) / 256)), dim3(256), 0, s, needs_reset, N, list, count);
    return hipGetLastError();
}
