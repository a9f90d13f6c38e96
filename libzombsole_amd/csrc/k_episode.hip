// k_episode.hip — per-env episode statistics (ZS_FLAG_EPISODE_STATS; the rule: zs_episode.hpp): k_episode_stats is the
// last launch of a flagged handle's step, k_episode_get gathers the engine's columns into the caller's env-major
// tensors, k_episode_clear zeroes the running part (zs_reset) or the last episode and the totals (zs_episode_stats_clear).
//
// One lane per env, 256-thread workgroups.  The engine's own rows are [k][N] columns, so a wave's accesses coalesce;
// the env-major entity rows are read only by the lanes whose env ended.  No atomics, no LDS.
#include "zs_launch.hpp"
#include "zs_episode.hpp"

#define ZS_EP_BLOCK 256

static_assert(EP_N == 3, "an episode's triple");

// the env's store (zs_episode.hpp) over the engine's columns and the step's outputs
struct EpStore {
    const EpisodeArgs& a;
    const double* rew_row;
    size_t e, N;
    ZS_HD double rew(int r) const { return rew_row[r]; }
    ZS_HD double run(int r) const {
        const uint32_t lo = a.run[(size_t)ZS_EP_COL_RET(r) * N + e], hi = a.run[((size_t)ZS_EP_COL_RET(r) + 1) * N + e];
        return __builtin_bit_cast(double, ((uint64_t)hi << 32) | lo);
    }
    ZS_HD void set_run(int r, double v) const {
        const uint64_t b = __builtin_bit_cast(uint64_t, v);
        a.run[(size_t)ZS_EP_COL_RET(r) * N + e] = (uint32_t)b;
        a.run[((size_t)ZS_EP_COL_RET(r) + 1) * N + e] = (uint32_t)(b >> 32);
    }
    ZS_HD int32_t flags() const { return (int32_t)a.run[(size_t)ZS_EP_COL_FLAGS(a.R) * N + e]; }
    ZS_HD void set_flags(int32_t v) const { a.run[(size_t)ZS_EP_COL_FLAGS(a.R) * N + e] = (uint32_t)v; }
    ZS_HD void set_last_ret(int r, double v) const { a.last_ret[(size_t)r * N + e] = v; }
    ZS_HD void add_sum_ret(int r, double v) const { a.sum_ret[(size_t)r * N + e] = a.sum_ret[(size_t)r * N + e] + v; }
    ZS_HD void set_last(int k, int32_t v) const { a.last[(size_t)k * N + e] = v; }
    ZS_HD uint32_t tot(int k) const { return a.tot[(size_t)k * N + e]; }
    ZS_HD void set_tot(int k, uint32_t v) const { a.tot[(size_t)k * N + e] = v; }
    ZS_HD EpisodeEnd end() const {
        EpisodeEnd w;
        w.length = a.scal[(size_t)S_EPSTEPS * N + e];
        w.zombie_deaths = a.scal[(size_t)S_ZD * N + e];
        w.deaths = a.scal[(size_t)S_DEATHS * N + e];
        w.alive_players = w.alive_agents = 0;
        const int32_t* life = a.life + e * a.E;
        for (int s = 0; s < a.A + a.P; s++) {
            const int up = life[s] > 0;
            w.alive_players += up;
            if (s < a.A) w.alive_agents += up;
        }
        w.initial_zombies = a.envp ? a.envp[(size_t)EP_INITIAL * N + e] : a.initial_zombies;
        w.minimum_zombies = a.envp ? a.envp[(size_t)EP_MINIMUM * N + e] : a.minimum_zombies;
        w.max_episode_steps = a.envp ? a.envp[(size_t)EP_MAXSTEPS * N + e] : a.max_steps;
        return w;
    }
};

__global__ void __launch_bounds__(ZS_EP_BLOCK) k_episode_stats(EpisodeArgs a, const double* rew, const uint8_t* done,
                                                              const uint8_t* trunc, const uint8_t* was_reset) {
    const int e = blockIdx.x * ZS_EP_BLOCK + threadIdx.x;
    if (e >= a.N) return;
    EpStore s = {a, rew + (size_t)e * a.R, (size_t)e, (size_t)a.N};
    episode_update(s, a.R, a.rules, a.A + a.P, was_reset[e] != 0, done[e] != 0, trunc[e] != 0);
}

// env-major outputs (any of them null): run_ret, last_ret, sum_ret f64 [N][R], last i32 [N][8], tot u32 [N][8]; the
// rows of an env whose mask byte is 0 are untouched (mask null: every env)
__global__ void __launch_bounds__(ZS_EP_BLOCK) k_episode_get(EpisodeArgs a, const uint8_t* mask, double* run_ret, double* last_ret,
                                                            double* sum_ret, int32_t* last, uint32_t* tot) {
    const int e = blockIdx.x * ZS_EP_BLOCK + threadIdx.x;
    if (e >= a.N || (mask && !mask[e])) return;
    const size_t N = a.N;
    const EpStore s = {a, nullptr, (size_t)e, N};
    for (int r = 0; r < a.R; r++) {
        if (run_ret) run_ret[(size_t)e * a.R + r] = s.run(r);
        if (last_ret) last_ret[(size_t)e * a.R + r] = a.last_ret[(size_t)r * N + e];
        if (sum_ret) sum_ret[(size_t)e * a.R + r] = a.sum_ret[(size_t)r * N + e];
    }
    for (int k = 0; k < ZS_EP_LAST; k++)
        if (last) last[(size_t)e * ZS_EP_LAST + k] = a.last[(size_t)k * N + e];
    for (int k = 0; k < ZS_EP_TOT; k++)
        if (tot) tot[(size_t)e * ZS_EP_TOT + k] = a.tot[(size_t)k * N + e];
}

// the masked envs' running part (running != 0: run_ret = 0, closed = 0), else their last episode and totals, zeroed
__global__ void __launch_bounds__(ZS_EP_BLOCK) k_episode_clear(EpisodeArgs a, const uint8_t* mask, int running) {
    const int e = blockIdx.x * ZS_EP_BLOCK + threadIdx.x;
    if (e >= a.N || (mask && !mask[e])) return;
    const size_t N = a.N;
    const EpStore s = {a, nullptr, (size_t)e, N};
    if (running) {
        for (int r = 0; r < a.R; r++) s.set_run(r, 0.0);
        s.set_flags(0);
        return;
    }
    for (int r = 0; r < a.R; r++) a.last_ret[(size_t)r * N + e] = 0.0, a.sum_ret[(size_t)r * N + e] = 0.0;
    for (int k = 0; k < ZS_EP_LAST; k++) a.last[(size_t)k * N + e] = 0;
    for (int k = 0; k < ZS_EP_TOT; k++) a.tot[(size_t)k * N + e] = 0u;
}

static unsigned ep_grid(int n) { return (unsigned)((n + ZS_EP_BLOCK - 1) / ZS_EP_BLOCK); }

hipError_t launch_episode_stats(hipStream_t s, const EpisodeArgs& a, const double* rew, const uint8_t* done, const uint8_t* trunc,
                                const uint8_t* was_reset) {
    hipLaunchKernelGGL(k_episode_stats, dim3(ep_grid(a.N)), dim3(ZS_EP_BLOCK), 0, s, a, rew, done, trunc, was_reset);
    return hipGetLastError();
}

hipError_t launch_episode_get(hipStream_t s, const EpisodeArgs& a, const uint8_t* mask, double* run_ret, double* last_ret,
                              double* sum_ret, int32_t* last, uint32_t* tot) {
    hipLaunchKernelGGL(k_episode_get, dim3(ep_grid(a.N)), dim3(ZS_EP_BLOCK), 0, s, a, mask, run_ret, last_ret, sum_ret, last, tot);
    return hipGetLastError();
}

hipError_t launch_episode_clear(hipStream_t s, const EpisodeArgs& a, const uint8_t* mask, int running) {
    hipLaunchKernelGGL(k_episode_clear, dim3(ep_grid(a.N)), dim3(ZS_EP_BLOCK), 0, s, a, mask, running);
    return hipGetLastError();
}
