// k_state.hip — the small helper kernels behind the ABI: seeding (k_seed), the bench / parity policy stream
// (k_gen_actions, k_gen_actions_ctr), the step's tail on its own (k_tail), the state views (k_get_state, k_set_state),
// the drop-ins' per-call records (k_host_unpack, k_host_pack) and zs_create's two init kernels.
#include "zs_launch.hpp"

// ---------------------------------------------------------------------------
// seeding: random.seed(int) (init_by_array over abs(n) in 32-bit little-endian words)
// ---------------------------------------------------------------------------
__global__ void k_seed(Dev d, int env0, int n, const uint64_t* seeds) {
    int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    int e = env0 + i;
    uint64_t sd = seeds[i];
    d.seeds[e] = sd;
    uint32_t* mt = d.ring + (size_t)e * ZS_RING_WORDS;
    uint32_t key[2] = {(uint32_t)sd, (uint32_t)(sd >> 32)};
    int klen = (sd >> 32) ? 2 : 1;
    mt[0] = 19650218u;
    for (int k = 1; k < ZS_MT_N; k++) mt[k] = 1812433253u * (mt[k - 1] ^ (mt[k - 1] >> 30)) + (uint32_t)k;
    int a = 1, b = 0;
    for (int k = (ZS_MT_N > klen ? ZS_MT_N : klen); k; k--) {
        mt[a] = (mt[a] ^ ((mt[a - 1] ^ (mt[a - 1] >> 30)) * 1664525u)) + key[b] + (uint32_t)b;
        a++;
        b++;
        if (a >= ZS_MT_N) {
            mt[0] = mt[ZS_MT_N - 1];
            a = 1;
        }
        if (b >= klen) b = 0;
    }
    for (int k = ZS_MT_N - 1; k; k--) {
        mt[a] = (mt[a] ^ ((mt[a - 1] ^ (mt[a - 1] >> 30)) * 1566083941u)) - (uint32_t)a;
        a++;
        if (a >= ZS_MT_N) {
            mt[0] = mt[ZS_MT_N - 1];
            a = 1;
        }
    }
    mt[0] = 0x80000000u;
    // the seeded state is x[0..623]; the first draw twists, so the output stream starts at x[624]
    mt_twist_serial(mt + ZS_MT_N, mt);  // block 1 -> slot 1 (current)
    mt_twist_serial(mt, mt + ZS_MT_N);  // block 2 -> slot 0 (next, ready)
    d.rngst[e] = 0u | (1u << 10) | (1u << 11);
}

// ---------------------------------------------------------------------------
// bench / parity action stream (libzombsole_amd/actions.py; policy_action in zs_device.hpp)
// ---------------------------------------------------------------------------
// one thread per (env, agent): its triple
__global__ void k_gen_actions(Dev d, uint64_t step, int n_discrete, int32_t* act) {
    int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= d.N * d.A) return;
    const int e = i / d.A;
    const int id = policy_id(d.seeds[e], step, n_discrete, i - e * d.A);
    act[(size_t)i * 3 + 0] = c_discrete[id][0];
    act[(size_t)i * 3 + 1] = c_discrete[id][1];
    act[(size_t)i * 3 + 2] = c_discrete[id][2];
}

// The same policy for the step number in device memory (zs_step_graph with the reset work on a side
// stream: launched after the reset fork, it gives the reset work a head start on the tick)
__global__ void k_gen_actions_ctr(Dev d, const uint64_t* ctr, int n_discrete, int32_t* act) {
    int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= d.N * d.A) return;
    const int e = i / d.A;
    const int id = policy_id(d.seeds[e], ctr[0], n_discrete, i - e * d.A);
    act[(size_t)i * 3 + 0] = c_discrete[id][0];
    act[(size_t)i * 3 + 1] = c_discrete[id][1];
    act[(size_t)i * 3 + 2] = c_discrete[id][2];
}

// the step's tail when no observation launch ends the step (observations written by the step launch)
__global__ void k_tail(Dev d) {
    if (threadIdx.x == 0) step_tail(d);
}

// ---------------------------------------------------------------------------
// state views (one env, one thread; test pokes)
// ---------------------------------------------------------------------------
// env e's state record (layout: include/zombsole_mi355x.h), written by threads tid = 0..nt-1 of one workgroup
// (every thread of the workgroup calls it)
__device__ void state_record(const Dev& d, int e, int32_t* b, int tid, int nt) {
    const int N = d.N, E = d.E;
    __shared__ int nz;  // present zombies
    if (tid == 0) nz = 0;
    __syncthreads();
    for (int s = d.A + d.P + tid; s < E; s += nt)
        if (d.present[EIX(d, s, e)]) atomicAdd(&nz, 1);
    __syncthreads();
    if (tid == 0) {
        b[0] = d.scal[S_T * N + e];
        b[1] = d.scal[S_DEATHS * N + e];
        b[2] = d.scal[S_ZD * N + e];
        b[3] = d.scal[S_EPSTEPS * N + e];
        b[4] = d.scal[S_NORDER * N + e];
        b[5] = d.scal[S_NEEDRESET * N + e];
        b[6] = E;
        b[7] = d.O;
        b[8] = d.W;
        b[9] = d.H;
        b[10] = d.scal[S_PREVZD * N + e];
        b[11] = nz;
        b[12] = d.scal[S_SERIAL * N + e];
        b[13] = b[14] = b[15] = 0;
    }
    int32_t* r = b + ZS_STATE_HEADER;
    for (int s = tid; s < E; s += nt) {
        int32_t* q = r + s * ZS_STATE_ENTITY_WORDS;
        int32_t p = d.pos[EIX(d, s, e)];
        q[0] = s < d.A ? ZS_THING_AGENT : (s < d.A + d.P ? ZS_THING_PLAYER : ZS_THING_ZOMBIE);
        q[1] = d.present[EIX(d, s, e)];
        q[2] = unpack_x(p);
        q[3] = unpack_y(p);
        q[4] = d.life[EIX(d, s, e)];
        q[5] = d.weapon[EIX(d, s, e)];
        q[6] = s < d.A ? s : (s < d.A + d.P ? s - d.A : 0);
        q[7] = (int32_t)d.serial[EIX(d, s, e)];
    }
    r += ZS_STATE_ENTITY_WORDS * E;
    for (int s = tid; s < E; s += nt) r[s] = d.order[EIX(d, s, e)];
    r += E;
    for (int o = tid; o < d.O; o += nt) r[o] = d.obst_hp[(size_t)e * d.O + o];
    r += d.O;
    for (int o = tid; o < d.O; o += nt) r[o] = (d.obst_present[(size_t)e * d.OW + (o >> 5)] >> (o & 31)) & 1u;
    r += d.O;
    for (int a = tid; a < d.A; a += nt) r[a] = d.prev_life[(size_t)a * N + e];
    r += d.A;
    for (int a = tid; a < d.A; a += nt) r[a] = d.listed[(size_t)a * N + e];
    r += d.A;
    for (int w = tid; w < d.DW; w += nt) r[w] = (int32_t)d.dead[(size_t)e * d.DW + w];
}

__global__ void k_get_state(Dev d, int e, int32_t* buf) { state_record(d, e, buf, threadIdx.x, blockDim.x); }

// ---------------------------------------------------------------------------
// the drop-ins' per-call path (zs_host_step / zs_host_reset / zs_host_observe): one workgroup per env
// ---------------------------------------------------------------------------
// the process-global `random` state moved in (rings[e]: the getstate() block and its successor, st[e])
// (host memory read in place: one round of 16-B loads, 1 248 words = 312 per env)
__global__ void k_host_unpack(Dev d, const uint32_t* rings, const uint32_t* st, int* err) {
    const int e = blockIdx.x, t = threadIdx.x;
    if (e == 0 && t == 0) *err = 0;  // the call's error word starts clear (host_call; no memset launch)
    static_assert(ZS_RING_WORDS % 4 == 0, "16-B copies");
    const uint4* src = (const uint4*)(rings + (size_t)e * ZS_RING_WORDS);
    uint4* dst = (uint4*)(d.ring + (size_t)e * ZS_RING_WORDS);
    const int n4 = ZS_RING_WORDS / 4;  // 312: two per thread at most (blockDim 256)
    uint4 a = t < n4 ? src[t] : uint4{}, b = t + 256 < n4 ? src[t + 256] : uint4{};
    const uint32_t sv = t == 0 ? st[e] : 0u;
    if (t < n4) dst[t] = a;
    if (t + 256 < n4) dst[t + 256] = b;
    if (t == 0) d.rngst[e] = sv;
}

// everything a call returns to the host, for env e: outputs, RNG stream, logs, state record, observation
__global__ void k_host_pack(Dev d, HostLayout L, const uint8_t* obs, const double* rew, const uint8_t* done,
                            const uint8_t* trunc, const uint8_t* rst, int* err, int32_t* rec) {
    const int e = blockIdx.x, tid = threadIdx.x, nt = blockDim.x;
    int32_t* r = rec + (size_t)e * L.words;
    const uint32_t st = d.rngst[e];
    if (tid == 0) {
        r[ZS_HOST_FLAGS] = (done[e] ? 1 : 0) | (trunc[e] ? 2 : 0) | (rst && rst[e] ? 4 : 0);
        // every env's record carries the call's error word; host_call clears it ahead of the call's launches
        // (not here: a block that cleared it would hide it from the blocks that read after it)
        r[ZS_HOST_ERR] = *err;
        r[ZS_HOST_ALOG_N] = d.alog ? d.alog_n[e] : 0;
        r[ZS_HOST_DLOG_N] = d.dlog ? d.dlog_n[e] : 0;
        r[ZS_HOST_RNG + ZS_MT_N] = (int32_t)(st & 1023u);
    }
    const uint32_t* blk = d.ring + (size_t)e * ZS_RING_WORDS + ((st >> 10) & 1u) * ZS_MT_N;
    for (int k = tid; k < ZS_MT_N; k += nt) r[ZS_HOST_RNG + k] = (int32_t)blk[k];
    const int32_t* rw = (const int32_t*)(rew + (size_t)e * L.R);
    for (int k = tid; k < 2 * L.R; k += nt) r[L.rew + k] = rw[k];
    if (d.alog)
        for (int k = tid; k < 2 * d.E; k += nt) r[L.alog + k] = d.alog[(size_t)e * d.E * 2 + k];
    if (d.dlog)
        for (int k = tid; k < 5 * d.E; k += nt) r[L.dlog + k] = d.dlog[(size_t)e * d.E * 5 + k];
    state_record(d, e, r + L.state, tid, nt);
    // the observation: 16-B copies when the env's block allows (L.obs is 16-B aligned), else 2-B ones
    const uint8_t* src = obs + (size_t)e * L.obs_bytes;
    uint8_t* dst = (uint8_t*)(r + L.obs);
    if (L.obs_bytes % 16 == 0 && ((size_t)e * L.obs_bytes) % 16 == 0 && (L.words % 4) == 0) {
        for (int k = tid; k < L.obs_bytes / 16; k += nt) ((uint4*)dst)[k] = ((const uint4*)src)[k];
    } else {
        for (int k = tid; k < L.obs_bytes / 2; k += nt) ((uint16_t*)dst)[k] = ((const uint16_t*)src)[k];
    }
}

__global__ void k_set_state(Dev d, int e, const int32_t* buf, int* err) {
    if (threadIdx.x != 0) return;
    const int N = d.N, E = d.E;
    const int32_t* b = buf;
    // needs_reset (b[5]) is the engine's own: pending resets are its work lists (an env on a list with
    // the flag cleared would be reset and ticked by one call, one off the lists with the flag set would
    // report a reset without a rebuild), so a record that disagrees is refused, nothing written
    if (b[5] != d.scal[S_NEEDRESET * N + e]) {
        *err = ZS_EINVAL;
        return;
    }
    d.scal[S_T * N + e] = b[0];
    d.scal[S_DEATHS * N + e] = b[1];
    d.scal[S_ZD * N + e] = b[2];
    d.scal[S_EPSTEPS * N + e] = b[3];
    d.scal[S_NORDER * N + e] = b[4];
    d.scal[S_PREVZD * N + e] = b[10];
    d.scal[S_SERIAL * N + e] = b[12];
    const int32_t* r = b + ZS_STATE_HEADER;
    for (int s = 0; s < E; s++, r += ZS_STATE_ENTITY_WORDS) {
        d.present[EIX(d, s, e)] = (uint8_t)r[1];
        d.pos[EIX(d, s, e)] = pack_xy(r[2], r[3]);
        d.life[EIX(d, s, e)] = r[4];
        d.weapon[EIX(d, s, e)] = (uint8_t)r[5];
        d.serial[EIX(d, s, e)] = (uint32_t)r[7];
    }
    for (int s = 0; s < E; s++) d.order[EIX(d, s, e)] = (uint8_t)*r++;
    int any_nonpos = 0;
    for (int o = 0; o < d.O; o++) {
        int v = *r++;
        d.obst_hp[(size_t)e * d.O + o] = hp_store_value(d, v);
        d.hp_dirty[e] = 0xffffffffu;
        uint32_t* w = &d.obst_nonpos[(size_t)e * d.OW + (o >> 5)];
        *w = v <= 0 ? (*w | (1u << (o & 31))) : (*w & ~(1u << (o & 31)));
        any_nonpos |= v <= 0;
    }
    for (int o = 0; o < d.O; o++) {
        uint32_t* w = &d.obst_present[(size_t)e * d.OW + (o >> 5)];
        *w = *r++ ? (*w | (1u << (o & 31))) : (*w & ~(1u << (o & 31)));
    }
    d.scal[S_ODIRTY * N + e] = any_nonpos;
    for (int a = 0; a < d.A; a++) d.prev_life[(size_t)a * N + e] = *r++;
    for (int a = 0; a < d.A; a++) d.listed[(size_t)a * N + e] = (uint8_t)*r++;
    for (int w = 0; w < d.DW; w++) d.dead[(size_t)e * d.DW + w] = (uint32_t)*r++;
    d.dead_dirty[e] = 0xffffffffu;
}

__global__ void k_init_pending(Dev d, int* list, int* count) {
    int e = blockIdx.x * blockDim.x + threadIdx.x;
    if (e == 0) {
        count[0] = d.N;
        count[1] = 0;
    }
    if (e >= d.N) return;
    list[e] = e;
    d.scal[S_NEEDRESET * d.N + e] = 1;
}

__global__ void k_init_obstacles(Dev d) {
    size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= (size_t)d.N * d.O) return;
    int o = (int)(i % d.O);
    d.obst_hp[i] = d.obst_kind[o] == ZS_THING_BOX ? 10 : 200;  // Box / Wall MAX_LIFE
}

// ---------------------------------------------------------------------------
// host launchers (zs_launch.hpp)
// ---------------------------------------------------------------------------
static unsigned grid_of(size_t n, int block) { return (unsigned)((n + block - 1) / block); }

hipError_t launch_seed(hipStream_t s, const Dev& d, int env0, int n, const uint64_t* seeds) {
    hipLaunchKernelGGL(k_seed, dim3(grid_of(n, 64)), dim3(64), 0, s, d, env0, n, seeds);
    return hipGetLastError();
}

hipError_t launch_gen_actions(hipStream_t s, const Dev& d, uint64_t step, int n_discrete, int32_t* act) {
    hipLaunchKernelGGL(k_gen_actions, dim3(grid_of(d.N * d.A, 256)), dim3(256), 0, s, d, step, n_discrete, act);
    return hipGetLastError();
}

hipError_t launch_gen_actions_ctr(hipStream_t s, const Dev& d, const uint64_t* ctr, int n_discrete, int32_t* act) {
    hipLaunchKernelGGL(k_gen_actions_ctr, dim3(grid_of(d.N * d.A, 256)), dim3(256), 0, s, d, ctr, n_discrete, act);
    return hipGetLastError();
}

hipError_t launch_tail(hipStream_t s, const Dev& d) {
    hipLaunchKernelGGL(k_tail, dim3(1), dim3(64), 0, s, d);
    return hipGetLastError();
}

hipError_t launch_get_state(hipStream_t s, const Dev& d, int e, int32_t* buf) {
    hipLaunchKernelGGL(k_get_state, dim3(1), dim3(64), 0, s, d, e, buf);
    return hipGetLastError();
}

hipError_t launch_set_state(hipStream_t s, const Dev& d, int e, const int32_t* buf, int* err) {
    hipLaunchKernelGGL(k_set_state, dim3(1), dim3(64), 0, s, d, e, buf, err);
    return hipGetLastError();
}

hipError_t launch_host_unpack(hipStream_t s, const Dev& d, const uint32_t* rings, const uint32_t* st, int* err) {
    hipLaunchKernelGGL(k_host_unpack, dim3((unsigned)d.N), dim3(256), 0, s, d, rings, st, err);
    return hipGetLastError();
}

hipError_t launch_host_pack(hipStream_t s, const Dev& d, const HostLayout& L, const uint8_t* obs, const double* rew,
                            const uint8_t* done, const uint8_t* trunc, const uint8_t* rst, int* err, int32_t* rec) {
    hipLaunchKernelGGL(k_host_pack, dim3((unsigned)d.N), dim3(256), 0, s, d, L, obs, rew, done, trunc, rst, err, rec);
    return hipGetLastError();
}

hipError_t launch_init_pending(hipStream_t s, const Dev& d, int* list, int* count) {
    hipLaunchKernelGGL(k_init_pending, dim3(grid_of(d.N, 256)), dim3(256), 0, s, d, list, count);
    return hipGetLastError();
}

hipError_t launch_init_obstacles(hipStream_t s, const Dev& d) {  // d.O > 0
    hipLaunchKernelGGL(k_init_obstacles, dim3(grid_of((size_t)d.N * d.O, 256)), dim3(256), 0, s, d);
    return hipGetLastError();
}
