// k_entity_obs.hip — the entity-observation kernel (zs_entity_obs.hpp): k_entity_obs.
#define ZS_DEFINE_ENTITY_KERNEL
#include "zs_launch.hpp"
#include "zs_entity_obs.hpp"

hipError_t launch_entity_obs(hipStream_t s, const Dev& d, const EntityArgs& g, const uint8_t* env_mask, void* out) {
    hipLaunchKernelGGL(k_entity_obs, dim3(zs_ent_grid(d.N)), dim3(ZS_ENT_BLOCK), 0, s, d, g, env_mask, (uint64_t*)out);
    return hipGetLastError();
}
