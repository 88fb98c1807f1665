// lutr_stack_steps.h -- the per-pixel step functions of a stage stack and the walk of one block of pixels
// through the compiled step list, shared by the YUV stack kernels (lutr_stack.hip), the RGB-source ones (lutr_rgbstack.hip,
// DESIGN.md 3.26) and the YUV -> RGB ones (lutr_y2rstack.hip).  Device code only; include it behind lutr_device.h.
//
// The includer says whether its translation unit holds the matrix steps: with LUTR_SK_MTX defined, SK_MTX_PARAM is
// `, const MtxConsts &X` and stack_block takes the matrix as its last argument; without, SK_MTX_PARAM is empty and the steps are
// not in the text at all (the kernels of 3.21 keep their code).
#pragma once

#include "lutr_device.h"

#ifndef SK_MTX_PARAM
#error "define SK_MTX_PARAM (and LUTR_SK_MTX with it) ahead of lutr_stack_steps.h"
#endif

namespace lutr {

// the 1D lookup of 3.20 on one pixel of codes
__device__ __forceinline__ Rgb stack_l1d_px(const uint16_t *tab, int stride, const Rgb &q)
{
    Rgb t;
    t.r = (float)tab[(int)q.r];
    t.g = (float)tab[stride + (int)q.g];
    t.b = (float)tab[2 * stride + (int)q.b];
    return t;
}

// unit -> codes: the product and the sum each rounded on their own (no contraction); o in [0, 1] gives [0, M] without a clip
__device__ __forceinline__ Rgb stack_round_px(float maxf, const Rgb &o)
{
    Rgb q;
    q.r = (float)(int)(o.r * maxf + 0.5f);
    q.g = (float)(int)(o.g * maxf + 0.5f);
    q.b = (float)(int)(o.b * maxf + 0.5f);
    return q;
}

// The RGB matrix of 3.25 on one pixel: u = p * k (k = 1 / M on codes; 1 on unit floats, where the product is u itself), then per
// row two products summed, the third product added, the offset added -- each rounded on its own -- and the clamp to [0, 1].  The
// host keeps the entries finite and small enough for every sum to be finite.
__device__ __forceinline__ Rgb mtx_px(const MtxConsts &X, float k, const Rgb &p)
{
    const float r = p.r * k, g = p.g * k, b = p.b * k;
    Rgb o;
    o.r = med3(((X.m[0] * r + X.m[1] * g) + X.m[2] * b) + X.off[0], 0.0f, 1.0f);
    o.g = med3(((X.m[3] * r + X.m[4] * g) + X.m[5] * b) + X.off[1], 0.0f, 1.0f);
    o.b = med3(((X.m[6] * r + X.m[7] * g) + X.m[8] * b) + X.off[2], 0.0f, 1.0f);
    return o;
}

template <int INTERP, int N>
__device__ __forceinline__ void stack_lattice(bool unit, const LutConsts &X, const GFetch &fx, Rgb (&px)[N])
{
    if (unit) {
#pragma unroll
        for (int i = 0; i < N; i++) px[i] = lut3d_unit<INTERP>(X, fx, px[i]);
    } else {
#pragma unroll
        for (int i = 0; i < N; i++) px[i] = lut3d_px<INTERP>(X, fx, px[i].r, px[i].g, px[i].b);
    }
}

// The CDL's and the 1D table's words of S into a workgroup's LDS, the CDL's first (stack_in_lds, lutr_launch.h); every thread of the
// workgroup must arrive here
__device__ __forceinline__ void stack_stage_to(uint32_t *lds, const StackConsts &S)
{
    const uint32_t *__restrict__ a = (const uint32_t *)S.cdl_tab;
    const uint32_t *__restrict__ b = (const uint32_t *)S.l1d_tab;
    for (int i = threadIdx.x; i < S.lds_cdl_words; i += 256) lds[i] = a[i];
    for (int i = threadIdx.x; i < S.lds_l1d_words; i += 256) lds[S.lds_cdl_words + i] = b[i];
    __syncthreads();
}

// The pixels of one block through the step list.  Every branch depends on kernel arguments only.
template <bool TRI, int N>
__device__ __forceinline__ void stack_block(const StackConsts &S, const CdlConsts &C, const uint16_t *l1d, const LutConsts &L,
                                            const LutConsts &L2, Rgb (&px)[N] SK_MTX_PARAM)
{
    const bool mix = S.sat != 1.0f;
#pragma nounroll
    for (unsigned long long ops = S.ops; ops & 0xffull; ops >>= 8) {
        const int op = (int)(ops & 15u), mode = (int)((ops >> 4) & 15u);
        if (op == STACK_OP_L1D) {
#pragma unroll
            for (int i = 0; i < N; i++) px[i] = stack_l1d_px(l1d, S.stride, px[i]);
        } else if (op == STACK_OP_CDL) {
#pragma unroll
            for (int i = 0; i < N; i++) px[i] = cdl_px(C, mix, px[i]);
        } else if (op == STACK_OP_ROUND) {
#pragma unroll
            for (int i = 0; i < N; i++) px[i] = stack_round_px(S.maxf, px[i]);
#ifdef LUTR_SK_MTX
        } else if (op == STACK_OP_MTX_CODES || op == STACK_OP_MTX_UNIT) {
            const float k = op == STACK_OP_MTX_CODES ? X.rcp : 1.0f;
#pragma unroll
            for (int i = 0; i < N; i++) px[i] = mtx_px(X, k, px[i]);
#endif
        } else {
            const bool second = op == STACK_OP_LAT2_CODES || op == STACK_OP_LAT2_UNIT;
            const bool unit = op == STACK_OP_LAT_UNIT || op == STACK_OP_LAT2_UNIT;
            const LutConsts X = second ? L2 : L;
            const GFetch fx(X);                                   // each lattice its own fetch; a pixel holds one set of taps
            if (mode == LUTR_INTERP_TETRAHEDRAL) stack_lattice<LUTR_INTERP_TETRAHEDRAL>(unit, X, fx, px);
            else if (TRI && mode == LUTR_INTERP_TRILINEAR) stack_lattice<LUTR_INTERP_TRILINEAR>(unit, X, fx, px);
            else stack_lattice<LUTR_INTERP_NEAREST>(unit, X, fx, px);
        }
    }
}

#ifdef LUTR_SK_MTX
// stack_generic's per-pixel step loop (lutr_stack.hip) on one pixel of codes: the tables read from global memory, all five modes
__device__ __forceinline__ Rgb rsk_steps_px(const LutConsts &L, const LutConsts &L2, const GFetch &f, const GFetch &f2,
                                            const StackConsts &S, const CdlConsts &C, const MtxConsts &X, bool mix, Rgb o)
{
#pragma nounroll
    for (unsigned long long ops = S.ops; ops & 0xffull; ops >>= 8) {
        const int op = (int)(ops & 15u), mode = (int)((ops >> 4) & 15u);
        switch (op) {
        case STACK_OP_L1D:        o = stack_l1d_px(S.l1d_tab, S.stride, o); break;
        case STACK_OP_CDL:        o = cdl_px(C, mix, o); break;
        case STACK_OP_ROUND:      o = stack_round_px(S.maxf, o); break;
        case STACK_OP_LAT_CODES:  o = lut3d_px_rt(mode, L, f, o.r, o.g, o.b); break;
        case STACK_OP_LAT_UNIT:   o = lut3d_unit_rt(mode, L, f, o); break;
        case STACK_OP_LAT2_CODES: o = lut3d_px_rt(mode, L2, f2, o.r, o.g, o.b); break;
        case STACK_OP_MTX_CODES:  o = mtx_px(X, X.rcp, o); break;
        case STACK_OP_MTX_UNIT:   o = mtx_px(X, 1.0f, o); break;
        default:                  o = lut3d_unit_rt(mode, L2, f2, o); break;
        }
    }
    return o;
}
#endif

}  // namespace lutr
