// device helpers shared by the demodulator kernels
#pragma once
#include <hip/hip_runtime.h>

namespace sdrx {

__device__ __forceinline__ int sdrx_to_q16(float v)
{
    // (qint16) of a float as x86-64 does it: cvttss2si (0x80000000 when out of range or NaN), then the low 16 bits
    const int i = (v >= -2147483648.0f && v < 2147483648.0f) ? (int)v : (int)0x80000000u;
    return (int)(short)i;
}

} // namespace sdrx
