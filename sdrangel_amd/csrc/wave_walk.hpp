// What the serial walks share (chana_walk_kernel, bfm_walk_kernel, bfm_deemph_kernel): one wave per channel steps through a
// dependent loop, 64 inputs staged one per lane, each step's input taken from its lane's register so that the step's values and
// branches are the wave's.
#pragma once
#include <hip/hip_runtime.h>

namespace sdrx {

__device__ __forceinline__ float walk_lane_value(float v, int lane)
{
    return __int_as_float(__builtin_amdgcn_readlane(__float_as_int(v), lane));
}

// a walk's streams as global memory by name: a generic access would count on the LDS / scalar-memory counter as well, and
// the step's table lookups would then wait for the batch in flight
typedef __attribute__((address_space(1))) unsigned long long walk_global_u64;
typedef __attribute__((address_space(1))) unsigned int walk_global_u32;
__device__ __forceinline__ float2 walk_global_load(const float2* p)
{
    const unsigned long long v = *(const walk_global_u64*)p;
    return make_float2(__int_as_float((int)(unsigned)v), __int_as_float((int)(unsigned)(v >> 32)));
}
__device__ __forceinline__ float walk_global_load(const float* p)
{
    return __int_as_float((int)*(const walk_global_u32*)p);
}
__device__ __forceinline__ void walk_global_store(float2* p, float2 v)
{
    *(walk_global_u64*)p = (unsigned long long)(unsigned)__float_as_int(v.x) | ((unsigned long long)(unsigned)__float_as_int(v.y) << 32);
}
__device__ __forceinline__ void walk_global_store(unsigned int* p, unsigned int v) { *(walk_global_u32*)p = v; }

} // namespace sdrx
