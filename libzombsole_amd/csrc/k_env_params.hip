// k_env_params.hip — per-env zombie counts and time limits (ZS_FLAG_ENV_PARAMS): k_env_params scatters the caller's
// triples into the envs' next triples, k_env_params_get gathers a handle's [3][N] rows into [N][3].
#include "zs_launch.hpp"

#define ZS_ENVP_BLOCK 256

// Entry k, k < n: the triple params[k][0..2] into the next triple of env idx[k] (null: env k).  An entry whose env
// is outside [0, N) or whose values are outside their ranges (the config's counts are the caps) is not applied and
// raises ZS_OVF_PARAM_RANGE.  Two launches, so that an env named by several entries ends with one of their triples
// whole: phase 0 leaves in owner[e] the highest valid entry that names env e (owner is -1 between calls), phase 1
// lets that entry alone store its three values and puts owner[e] back.
__global__ void __launch_bounds__(ZS_ENVP_BLOCK) k_env_params(Dev d, int32_t* owner, int phase, const int32_t* idx, int n,
                                                              const int32_t* params) {
    const int k = blockIdx.x * ZS_ENVP_BLOCK + threadIdx.x;
    if (k >= n) return;
    const int e = idx ? idx[k] : k;
    const int32_t v0 = params[(size_t)k * 3 + 0], v1 = params[(size_t)k * 3 + 1], v2 = params[(size_t)k * 3 + 2];
    const bool ok = (unsigned)e < (unsigned)d.N && v0 >= 0 && v0 <= d.initial_zombies && v1 >= 0 && v1 <= d.minimum_zombies && v2 >= 0;
    if (phase == 0) {
        if (ok) atomicMax(&owner[e], k);
        // one flag word for the handle: skip the atomic once the flag is up (hp_store_value)
        else if (!(__hip_atomic_load(d.ovf, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) & ZS_OVF_PARAM_RANGE))
            atomicOr(d.ovf, ZS_OVF_PARAM_RANGE);
        return;
    }
    // (the winner of this launch may be storing -1 to owner[e] meanwhile: neither value is a loser's k)
    if (!ok || __hip_atomic_load(&owner[e], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) != k) return;
    const size_t N = d.N;
    int32_t* next = envp_next(d);
    next[EP_INITIAL * N + e] = v0;
    next[EP_MINIMUM * N + e] = v1;
    next[EP_MAXSTEPS * N + e] = v2;
    __hip_atomic_store(&owner[e], -1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

// out[e][0..2] = rows[0..2][e]
__global__ void __launch_bounds__(ZS_ENVP_BLOCK) k_env_params_get(const int32_t* rows, int N, int32_t* out) {
    const int e = blockIdx.x * ZS_ENVP_BLOCK + threadIdx.x;
    if (e >= N) return;
    const int32_t v0 = rows[e], v1 = rows[(size_t)N + e], v2 = rows[(size_t)2 * N + e];
    out[(size_t)e * 3 + 0] = v0;
    out[(size_t)e * 3 + 1] = v1;
    out[(size_t)e * 3 + 2] = v2;
}

// both triples of every env = the config's values, owner = -1 (zs_create)
__global__ void __launch_bounds__(ZS_ENVP_BLOCK) k_env_params_init(Dev d, int32_t* owner) {
    const int e = blockIdx.x * ZS_ENVP_BLOCK + threadIdx.x;
    if (e >= d.N) return;
    const size_t N = d.N;
    const int32_t v[EP_N] = {d.initial_zombies, d.minimum_zombies, d.max_steps};
    for (int r = 0; r < EP_N; r++) envp_cur(d)[r * N + e] = envp_next(d)[r * N + e] = v[r];
    owner[e] = -1;
}

// *out = the handle's sticky range word, whose ZS_OVF_PARAM_RANGE bit alone is cleared (zs_env_params_check)
__global__ void k_env_params_check(uint32_t* ovf, uint32_t* out) {
    if (blockIdx.x == 0 && threadIdx.x == 0) *out = atomicAnd(ovf, ~(uint32_t)ZS_OVF_PARAM_RANGE);
}

static unsigned envp_grid(int n) { return (unsigned)(((long long)n + ZS_ENVP_BLOCK - 1) / ZS_ENVP_BLOCK); }

hipError_t launch_env_params_set(hipStream_t s, const Dev& d, int32_t* owner, const int32_t* idx, int n, const int32_t* params) {
    for (int phase = 0; phase < 2; phase++) {
        hipLaunchKernelGGL(k_env_params, dim3(envp_grid(n)), dim3(ZS_ENVP_BLOCK), 0, s, d, owner, phase, idx, n, params);
        const hipError_t e = hipGetLastError();
        if (e != hipSuccess) return e;
    }
    return hipSuccess;
}

hipError_t launch_env_params_get(hipStream_t s, const Dev& d, int current, int32_t* out) {
    hipLaunchKernelGGL(k_env_params_get, dim3(envp_grid(d.N)), dim3(ZS_ENVP_BLOCK), 0, s,
                       (const int32_t*)(current ? envp_cur(d) : envp_next(d)), d.N, out);
    return hipGetLastError();
}

hipError_t launch_env_params_check(hipStream_t s, const Dev& d, uint32_t* out) {
    hipLaunchKernelGGL(k_env_params_check, dim3(1), dim3(64), 0, s, d.ovf, out);
    return hipGetLastError();
}

hipError_t launch_env_params_init(hipStream_t s, const Dev& d, int32_t* owner) {
    hipLaunchKernelGGL(k_env_params_init, dim3(envp_grid(d.N)), dim3(ZS_ENVP_BLOCK), 0, s, d, owner);
    return hipGetLastError();
}
