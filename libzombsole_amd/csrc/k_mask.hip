// k_mask.hip — the action-mask kernel (zs_mask.hpp): k_action_mask.
#define ZS_DEFINE_MASK_KERNEL
#include "zs_launch.hpp"
#include "zs_mask.hpp"

hipError_t launch_action_mask(hipStream_t s, const Dev& d, const uint8_t* env_mask, void* out) {
    hipLaunchKernelGGL(k_action_mask, dim3(zs_mask_grid(d.N)), dim3(ZS_MASK_BLOCK), 0, s, d, env_mask, (uint64_t*)out);
    return hipGetLastError();
}
