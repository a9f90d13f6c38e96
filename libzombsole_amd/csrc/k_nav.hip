// k_nav.hip — the path-distance kernel (zs_nav.hpp): k_nav<F, FULL>, the per-agent rows of one or two fields and the
// full field of a list of envs.
#define ZS_DEFINE_NAV_KERNEL
#include "zs_launch.hpp"
#include "zs_nav.hpp"

hipError_t launch_nav(hipStream_t s, const Dev& d, const NavArgs& g, const uint8_t* env_mask, void* out) {
    const dim3 grid(nav_grid(g.plan, d.N)), block(g.plan.block);
    if (nav_nfields(g.fields) == 2)
        hipLaunchKernelGGL((k_nav<2, false>), grid, block, g.plan.lds_bytes, s, d, g, env_mask, nullptr, d.N, out);
    else
        hipLaunchKernelGGL((k_nav<1, false>), grid, block, g.plan.lds_bytes, s, d, g, env_mask, nullptr, d.N, out);
    return hipGetLastError();
}

hipError_t launch_nav_field(hipStream_t s, const Dev& d, const NavArgs& g, const int32_t* env_idx, int n, void* out) {
    if (n <= 0) return hipSuccess;
    hipLaunchKernelGGL((k_nav<1, true>), dim3(nav_grid(g.plan, n)), dim3(g.plan.block), g.plan.lds_bytes, s, d, g, nullptr,
                       env_idx, n, out);
    return hipGetLastError();
}
