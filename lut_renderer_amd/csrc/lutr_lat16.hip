// lutr_lat16.hip -- the lattice of the fast variant: every node as four fp16 {r, g, b, 0} of value * (2^depth - 1),
// round to nearest even.  Pre-multiplying folds FFmpeg's `v * M` (vf_lut3d.c) into the node, so the blend
// of the fast kernels is the output code before truncation.  |fp16(v * M) - v * M| <= 0.25 at 10 bit, 0.0625 at 8 bit
// for v in [0, 1].  Built once per (lattice, depth) by lutr_api.cpp.
// Also the lattice of the fma32 variant: float4 {r * M, g * M, b * M, 0}, each product one fp32 rounding.
#include <hip/hip_fp16.h>

#include "lutr_internal.h"

namespace lutr {

__global__ __launch_bounds__(256) void k_make_lat16(const float4 *__restrict__ lat, uint2 *__restrict__ out, size_t nodes, float m)
{
    const size_t i = blockIdx.x * 256ull + threadIdx.x;
    if (i >= nodes) return;
    const float4 v = lat[i];
    // Two roundings, as the CPU twin has them (oracle/lut3d_oracle.c: f2h_rne(rgb * m) on an fp32 product): the product to fp32,
    // then fp32 to fp16.  Left to itself the compiler fuses `(half)(v * m)` into v_fma_mixlo_f16, which rounds the exact product
    // once -- a different node wherever the fp32 product lands on an fp16 tie (9 of 107,811 values of a 33^3 test lattice), and
    // every pixel blended from such a node can come out one code away from the twin.  The empty asm keeps the product a value
    // of its own.
    float pr = v.x * m, pg = v.y * m, pb = v.z * m;
    asm volatile("" : "+v"(pr), "+v"(pg), "+v"(pb));
    const unsigned r = __half_as_ushort(__float2half_rn(pr)), g = __half_as_ushort(__float2half_rn(pg));
    const unsigned b = __half_as_ushort(__float2half_rn(pb));
    out[i] = make_uint2(r | (g << 16), b);
}

__global__ __launch_bounds__(256) void k_make_latm(const float4 *__restrict__ lat, float4 *__restrict__ out, size_t nodes, float m)
{
    const size_t i = blockIdx.x * 256ull + threadIdx.x;
    if (i >= nodes) return;
    const float4 v = lat[i];
    out[i] = make_float4(v.x * m, v.y * m, v.z * m, 0.0f);
}

void launch_make_lat16(hipStream_t st, const float4 *lat, uint2 *out, size_t nodes, float m)
{
    hipLaunchKernelGGL(k_make_lat16, dim3((unsigned)((nodes + 255) / 256)), dim3(256), 0, st, lat, out, nodes, m);
}

void launch_make_latm(hipStream_t st, const float4 *lat, float4 *out, size_t nodes, float m)
{
    hipLaunchKernelGGL(k_make_latm, dim3((unsigned)((nodes + 255) / 256)), dim3(256), 0, st, lat, out, nodes, m);
}

}  // namespace lutr
