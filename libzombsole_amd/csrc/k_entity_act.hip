// k_entity_act.hip — the entity action table's kernels (zs_entity_act.hpp): k_entity_act_decode, k_entity_act_mask,
// k_entity_act_encode.
#define ZS_DEFINE_ENTITY_ACT_KERNEL
#include "zs_launch.hpp"
#include "zs_entity_act.hpp"

hipError_t launch_entity_act_decode(hipStream_t s, const Dev& d, int kz, int kp, const uint8_t* env_mask, const int32_t* ids,
                                    int32_t* actions) {
    hipLaunchKernelGGL(k_entity_act_decode, dim3(zs_ent_grid(d.N)), dim3(ZS_ENT_BLOCK), 0, s, d, kz, kp, env_mask, ids, actions);
    return hipGetLastError();
}

hipError_t launch_entity_act_mask(hipStream_t s, const Dev& d, int kz, int kp, const uint8_t* env_mask, void* out) {
    hipLaunchKernelGGL(k_entity_act_mask, dim3(zs_ent_grid(d.N)), dim3(ZS_ENT_BLOCK), 0, s, d, kz, kp, env_mask, (uint64_t*)out);
    return hipGetLastError();
}

hipError_t launch_entity_act_encode(hipStream_t s, const Dev& d, int kz, int kp, const uint8_t* env_mask, const int32_t* triples,
                                    int32_t* ids_out) {
    hipLaunchKernelGGL(k_entity_act_encode, dim3(zs_ent_grid(d.N)), dim3(ZS_ENT_BLOCK), 0, s, d, kz, kp, env_mask, triples, ids_out);
    return hipGetLastError();
}
