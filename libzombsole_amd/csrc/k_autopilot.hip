// k_autopilot.hip — the scripted-policy kernel (zs_autopilot.hpp): k_autopilot.
#define ZS_DEFINE_PILOT_KERNEL
#include "zs_launch.hpp"
#include "zs_autopilot.hpp"

hipError_t launch_autopilot(hipStream_t s, const Dev& d, const uint8_t* env_mask, const uint8_t* policy, int32_t* out) {
    hipLaunchKernelGGL(k_autopilot, dim3(zs_pilot_grid(d.N)), dim3(ZS_PILOT_BLOCK), 0, s, d, env_mask, policy, out);
    return hipGetLastError();
}
