// lutr_pkcodes.h -- where the codes of a packed 4:2:2 row and of a v210 group sit, and the runs of
// whole words their vector kernels move: shared by the single-lut3d kernels (lutr_pkyuv.hip, lutr_v210.hip) and the stage-stack
// kernels on those frames (lutr_pkstack.hip).  Device code only; include it behind lutr_device.h.
#pragma once

#include "lutr_device.h"

namespace lutr {

// ---------------------------------------------------------------- packed 4:2:2
// A packed side moves the thread's luma and chroma of a row in ONE run of 16 bytes (two for the 16-bit side of 16 -> 8).  Group
// order and shift are wave-uniform kernel arguments: they end up in the offset operand of the bit-field extract that unpacks the
// sample anyway.
template <int NW>
__device__ __forceinline__ void ld_run(uint32_t *w, const uint8_t *p)
{
    if constexpr (NW == 8) { ld_words<4>(w, p); ld_words<4>(w + 4, p + 16); }
    else ld_words<NW>(w, p);
}

template <int NW>
__device__ __forceinline__ void st_run(uint8_t *p, const uint32_t *w)
{
    if constexpr (NW == 8) { st_words<4>(p, w); st_words<4>(p + 16, w + 4); }
    else st_words<NW>(p, w);
}

// luma sample dx of group j of a packed row: 8 bit -- byte 2 dx + cf of word j; 16 bit -- half cf of word 2 j + dx
template <int WIDE>
__device__ __forceinline__ float pk_luma(const uint32_t *w, int j, int dx, unsigned cf, unsigned shift)
{
    if constexpr (WIDE) return (float)__builtin_amdgcn_ubfe(w[2 * j + dx], cf * 16u + shift, 16u - shift);
    else return (float)__builtin_amdgcn_ubfe(w[j], (2u * dx + cf) * 8u, 8u);
}

// chroma component k (0: Cb, 1: Cr) of group j: the first or the second chroma sample of the group, by `csw`
template <int WIDE>
__device__ __forceinline__ float pk_chroma(const uint32_t *w, int j, unsigned k, unsigned cf, unsigned csw, unsigned shift)
{
    if constexpr (WIDE) {
        const unsigned off = (1u - cf) * 16u + shift;
        const uint32_t a = __builtin_amdgcn_ubfe(w[2 * j], off, 16u - shift), b = __builtin_amdgcn_ubfe(w[2 * j + 1], off, 16u - shift);
        return (float)((k ^ csw) ? b : a);
    } else {
        return (float)__builtin_amdgcn_ubfe(w[j], ((1u - cf) + 2u * (k ^ csw)) * 8u, 8u);
    }
}

template <int WIDE>
__device__ __forceinline__ void pk_put_luma(uint32_t *w, int j, int dx, unsigned cf, float v)
{
    const uint32_t u = (uint32_t)v;
    if constexpr (WIDE) w[2 * j + dx] |= u << (cf * 16u);
    else w[j] |= u << ((2u * dx + cf) * 8u);
}

template <int WIDE>
__device__ __forceinline__ void pk_put_chroma(uint32_t *w, int j, unsigned cf, unsigned csw, float cb, float cr)
{
    const uint32_t ub = (uint32_t)cb, ur = (uint32_t)cr;
    const uint32_t a = csw ? ur : ub, b = csw ? ub : ur;
    if constexpr (WIDE) {
        w[2 * j] |= a << ((1u - cf) * 16u);
        w[2 * j + 1] |= b << ((1u - cf) * 16u);
    } else {
        w[j] |= (a << ((1u - cf) * 8u)) | (b << ((3u - cf) * 8u));
    }
}

// ---------------------------------------------------------------- v210
// where the samples of a group sit: word and bit offset of luma sample l (0..5) and of Cb / Cr of pair k (0..2)
__device__ constexpr int kV2YW[6] = {0, 1, 1, 2, 3, 3}, kV2YO[6] = {10, 0, 20, 10, 0, 20};
__device__ constexpr int kV2BW[3] = {0, 1, 2}, kV2BO[3] = {0, 10, 20};
__device__ constexpr int kV2RW[3] = {0, 2, 3}, kV2RO[3] = {20, 0, 10};

// one code of a word (a v_bfe_u32 with a compile-time offset once the caller's loop is unrolled); a code into a zeroed word
__device__ __forceinline__ float v2_get(uint32_t w, int off) { return (float)__builtin_amdgcn_ubfe(w, (unsigned)off, 10u); }
__device__ __forceinline__ void v2_put(uint32_t *w, int off, float v) { *w |= (uint32_t)v << off; }

// The planar runs of 6 and 3 words beside a v210 side start on a 4-byte boundary and no better (24 and 12 bytes per thread), so
// they move word by word.
template <int NW>
__device__ __forceinline__ void ld_dwords(uint32_t *w, const uint8_t *p)
{
#pragma unroll
    for (int k = 0; k < NW; k++) ld_words<1>(w + k, p + 4 * k);
}

template <int NW>
__device__ __forceinline__ void st_dwords(uint8_t *p, const uint32_t *w)
{
#pragma unroll
    for (int k = 0; k < NW; k++) st_words<1>(p + 4 * k, w + k);
}

}  // namespace lutr
