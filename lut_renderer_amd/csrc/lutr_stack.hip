// lutr_stack.hip -- gfx950 kernels of the fused YUV pass with an ordered stack of lut1d / CDL / lut3d stages.
//
// What they compute: between the YUV -> RGB stage (3.2) and the RGB -> YUV stage (3.2 / 3.8) a pixel walks a list of up to four
// stages, each kind at most once: the first lattice, the second lattice (3.17), the per-code 1D table (3.20), the ASC CDL (3.19).
// It travels as integer codes in [0, M] held as floats, or -- behind the CDL only -- as unit floats:
//   lut1d            codes -> codes   q'_c = tab[c][q_c]
//   cdl              codes -> unit    cdl_px (stages A and B of 3.19)
//   lut3d / lut3d2   codes -> codes   lut3d_px (the prelut taken), or unit -> codes: lut3d_unit
//   round            unit -> codes    q_c = (int)(o_c * M + 0.5f), where a unit pixel meets lut1d or the end of the list
// The host compiles the stage list into a word of step bytes (StackConsts::ops): the pixel's state follows from the list, so the
// rounding is a step of its own and a lattice step says which of its two forms it is.  The word is a kernel argument; the kernels
// walk it with wave-uniform branches.  Nothing is templated on the order.
//
// The unit of work is 3.8's union block for every pair of layouts, the equal ones included.  The vector kernels walk their units
// with a grid stride, so that a workgroup can stage the CDL and 1D tables into LDS once (LDS = true); LDS = false reads them from
// global memory through L1.  Both read the same entries: the bits do not depend on the choice.
//
// One source, two kinds of translation unit (Makefile MIX_RULE):
//   without LUTR_SK_WI   the generic kernel and the launcher
//   LUTR_SK_WI / _WO     the vector kernels of one container mix (8 -> 8, 16 -> 16, 16 -> 8): 9 layout pairs x (any stage
//                        trilinear) x 2 placements
//   LUTR_SKM_WI / _WO    the same set in its MIX form: k_yuv_stack_mix_vec
//   LUTR_SKM_GENERIC     the generic kernel in its MIX form: k_yuv_stack_mix_generic
//   LUTR_SKA_WI / _WO / _WM   the vector kernels in their MATTE form, for one container mix and one matte container:
//                        k_yuv_stack_matte_vec
//   LUTR_SKA_GENERIC     the generic kernel in its MATTE form: k_yuv_stack_matte_generic
//   LUTR_SKX_WI / _WO    the vector kernels in their MATRIX form: k_yuv_stack_mtx_vec
//   LUTR_SKX_GENERIC     the generic kernel in its MATRIX form: k_yuv_stack_mtx_generic
//   LUTR_SKS_WI / _WO    the vector kernels in their SEMI form, the eight layout pairs with a 4:2:0 / 4:2:2 side:
//                        k_yuv_stack_semi_vec
//   LUTR_SKS_GENERIC     the generic kernel of the SEMI form: k_yuv_stack_semi_generic
//
// MIX is a form of the same kernel text, with the pixel's codes behind the YUV -> RGB stage (q0) kept across the
// step walk, or evaluated again behind it, and q = (int)((q0 + s * (q1 - q0)) + 0.5f) sent to the RGB -> YUV stage; s is the
// strength of the pixel's frame, clamped to [0, 1].
//
// MATTE is a third form, which implies MIX: the mix form's text with one more argument, a plane of unsigned
// codes at luma resolution.  The strength of a pixel is the frame's times its matte sample: a' = min(a, Mm),
// a'' = invert ? Mm - a' : a', w = s * (a'' * rcp), and w takes the place of s in the mix.  The vector kernels are built per
// matte container (WM) beside the source's and load the thread's matte words at the top of a unit, beside the source words (3.23
// point 5).
//
// MATRIX is a fourth form, without MIX: the plain form's text with one more argument, the twelve numbers of an
// RGB matrix with offset (MtxConsts, wave-uniform: no table, no LDS), and two more steps in the walk, the matrix on codes and on
// unit floats.  Only this form's translation units hold those steps.
//
// SEMI is a fifth form, without MIX and MATRIX: the plain form's text with one more argument, the containers of the
// two sides (SemiArgs: a side's chroma as ONE plane of pairs, Cr first with `swap`, 16-bit codes `shift` bits up in their words),
// handled at run time with wave-uniform branches around the loads and the stores.  The arithmetic between them is untouched.
//
// How the forms are told apart: the generic kernel's body takes the form as a template parameter (StackForm), and the switches
// of its translation units only choose the instantiation.  The vector kernel keeps its own copy of union_vec_unit's structure
// (lutr_device.h) and the preprocessor forms it had, LUTR_SK_MIX and LUTR_SK_MATTE with the SK_* macros below: through the shared
// body mix instances lose a wave and the matte forms run slower.  Either way a translation unit without the MIX
// or MATTE switches holds nothing of them: the kernels of 3.21 keep their code, registers and names.
#if defined(LUTR_SKM_WI)
#define LUTR_SK_WI LUTR_SKM_WI
#define LUTR_SK_WO LUTR_SKM_WO
#endif
#if defined(LUTR_SKA_WI)
#define LUTR_SK_WI LUTR_SKA_WI
#define LUTR_SK_WO LUTR_SKA_WO
#define LUTR_SK_WM LUTR_SKA_WM
#endif
#if defined(LUTR_SKX_WI)
#define LUTR_SK_WI LUTR_SKX_WI
#define LUTR_SK_WO LUTR_SKX_WO
#endif
#if defined(LUTR_SKS_WI)
#define LUTR_SK_WI LUTR_SKS_WI
#define LUTR_SK_WO LUTR_SKS_WO
#endif
#if defined(LUTR_SKX_WI) || defined(LUTR_SKX_GENERIC)
#define LUTR_SK_MTX 1
#define SK_MTX_PARAM , const MtxConsts &X
#define SK_MTX_ARG , X
#else
#define SK_MTX_PARAM
#define SK_MTX_ARG
#endif
#ifdef LUTR_SK_WI                    // the vector kernel's forms
#if defined(LUTR_SKA_WI)
#define LUTR_SK_MATTE 1
#define LUTR_SK_MIX 1
#define SK_MIX_PARAM , MixConsts M, MatteConsts A
#define SK_MIX_ARG , M, A
#define SK_WM_TPARAM int WM,
#define SK_WM_TARG LUTR_SK_WM,
#define SK_WM_NAME LUTR_STR(LUTR_SK_WM) ","
#define SK_VEC k_yuv_stack_matte_vec
#define SK_VEC_NAME "k_yuv_stack_matte_vec<"
#define SK_VEC_LAUNCH_FN LUTR_CAT(LUTR_CAT(LUTR_CAT(launch_yuv_stack_matte_vec_w, LUTR_SK_WI), LUTR_SK_WO), LUTR_SK_WM)
#elif defined(LUTR_SKM_WI)
#define LUTR_SK_MIX 1
#define SK_MIX_PARAM , MixConsts M
#define SK_MIX_ARG , M
#define SK_VEC k_yuv_stack_mix_vec
#define SK_VEC_NAME "k_yuv_stack_mix_vec<"
#define SK_VEC_LAUNCH launch_yuv_stack_mix_vec_w
#elif defined(LUTR_SKX_WI)                 // the matrix form: no mix; its one more argument travels where the mix forms' do
#define SK_MIX_PARAM , MtxConsts X
#define SK_MIX_ARG , X
#define SK_VEC k_yuv_stack_mtx_vec
#define SK_VEC_NAME "k_yuv_stack_mtx_vec<"
#define SK_VEC_LAUNCH launch_yuv_stack_mtx_vec_w
#elif defined(LUTR_SKS_WI)                 // the semi form: no mix; the containers of the two sides travel where the mix forms' argument does
#define LUTR_SK_SEMI 1
#define SK_MIX_PARAM , SemiArgs A
#define SK_MIX_ARG , A
#define SK_VEC k_yuv_stack_semi_vec
#define SK_VEC_NAME "k_yuv_stack_semi_vec<"
#define SK_VEC_LAUNCH launch_yuv_stack_semi_vec_w
#else
#define SK_MIX_PARAM
#define SK_MIX_ARG
#define SK_VEC k_yuv_stack_vec
#define SK_VEC_NAME "k_yuv_stack_vec<"
#define SK_VEC_LAUNCH launch_yuv_stack_vec_w
#endif
#ifndef LUTR_SK_MATTE
#define SK_WM_TPARAM
#define SK_WM_TARG
#define SK_WM_NAME
#define SK_VEC_LAUNCH_FN LUTR_CAT(LUTR_CAT(SK_VEC_LAUNCH, LUTR_SK_WI), LUTR_SK_WO)
#endif
#endif  // LUTR_SK_WI

#include "lutr_device.h"
#include "lutr_launch.h"
#include "lutr_stack_steps.h"   // stack_l1d_px, stack_round_px, mtx_px, stack_lattice, stack_block

namespace lutr {

enum StackForm { SK_PLAIN, SK_MIX, SK_MATTE };

// The strength of frame fr: one dword of the per-frame array, or the call's scalar.  A NaN is 0, found by its bits (the build does
// not honour NaNs in float compares); then the clamp.
__device__ __forceinline__ float mix_strength(const MixConsts &M, long long fr)
{
    float s = M.frame ? M.frame[fr] : M.s;
    if ((__float_as_uint(s) & 0x7fffffffu) > 0x7f800000u) s = 0.0f;
    return fminf(fmaxf(s, 0.0f), 1.0f);
}

// q0 + s * (q1 - q0) rounded to a code: the difference is exact; the product and the two sums are each rounded on their own
__device__ __forceinline__ Rgb mix_px(float s, const Rgb &q0, const Rgb &q1)
{
    Rgb q;
    q.r = (float)(int)((q0.r + s * (q1.r - q0.r)) + 0.5f);
    q.g = (float)(int)((q0.g + s * (q1.g - q0.g)) + 0.5f);
    q.b = (float)(int)((q0.b + s * (q1.b - q0.b)) + 0.5f);
    return q;
}

// The strength of one pixel: the frame's strength s times the matte sample a (a code held as a float).  The clamp and the
// inversion are on integers below 2^16, exact in fp32; then one rounded product each for the normalisation and the scaling.
__device__ __forceinline__ float matte_weight(const MatteConsts &A, float s, float a)
{
    const float c = fminf(a, A.maxf);
    const float v = A.invert ? A.maxf - c : c;
    const float t = v * A.rcp;
    return s * t;
}

#ifdef LUTR_SK_WI
// ================================================================= vector kernel

extern __shared__ uint32_t stack_lds[];                           // the staged tables: the CDL's floats, then the 1D table's uint16

// The tables the stack uses into LDS, once per workgroup, as whole words (3 * stride floats; 3 * stride uint16 = 3 * stride / 2
// words, stride = 2^depth >= 256); the launcher sized the dynamic LDS to that.  Every thread of the workgroup must arrive here.
__device__ __forceinline__ void stack_stage_tables(const StackConsts &S)
{
    const uint32_t *__restrict__ a = (const uint32_t *)S.cdl_tab;
    const uint32_t *__restrict__ b = (const uint32_t *)S.l1d_tab;
    for (int i = threadIdx.x; i < S.lds_cdl_words; i += 256) stack_lds[i] = a[i];
    for (int i = threadIdx.x; i < S.lds_l1d_words; i += 256) stack_lds[S.lds_cdl_words + i] = b[i];
    __syncthreads();
}

#ifdef LUTR_SK_SEMI
// SEMI: a source sample, the container's shift riding in the extract that unpacks it (word_code, lutr_device.h)
#define SK_CODE(w, i) word_code<WIN>(w, i, ish)
// The byte selectors of v_perm_b32 (D = bytes of {first operand: 4..7, second operand: 0..3}) that take a plane of pairs apart and
// put one together.  `swap` exchanges the two selectors: which array a selector feeds is a scalar select.
//   split: from the pair words (w1, w0) the first / second component of their pairs, as one word of a planar plane
//   join:  from the planar words (second, first) the lower / upper pair word
template <int WIDE> struct SemiSel {
    static constexpr uint32_t split0 = WIDE ? 0x05040100u : 0x06040200u, split1 = WIDE ? 0x07060302u : 0x07050301u;
    static constexpr uint32_t join0 = WIDE ? 0x05040100u : 0x05010400u, join1 = WIDE ? 0x07060302u : 0x07030602u;
    static constexpr uint32_t join0s = WIDE ? 0x01000504u : 0x01050004u, join1s = WIDE ? 0x03020706u : 0x03070206u;
};
#else
#define SK_CODE(w, i) word_sample<WIN>(w, i)
#endif

// union_vec_unit's structure (lutr_device.h), as this family's own copy, with the step walk as the per-block middle.  TRI: some
// stage is trilinear (a stack of nearest / tetrahedral stages does not carry trilinear's registers).  No thread leaves before the barrier behind the staging.
template <int WIN, int WOUT, SK_WM_TPARAM int ICSX, int ICSY, int OCSX, int OCSY, bool TRI, bool LDS>
__global__ __launch_bounds__(256) void SK_VEC(LutConsts L, LutConsts L2, StackConsts S, YuvConsts K, PlaneSet P, FrameGeom G SK_MIX_PARAM)
{
    constexpr int VB = vec_bytes<WIN, WOUT>();
    constexpr int PXT = VB / (WIN ? 2 : 1);                       // luma samples per thread per row
    constexpr int YWI = VB / 4, YWO = PXT * (WOUT ? 2 : 1) / 4;   // luma words per thread per row, in / out
    constexpr int CSX = cmax(ICSX, OCSX), CSY = cmax(ICSY, OCSY);
    constexpr int BW = 1 << CSX, BH = 1 << CSY;                   // the union block
    constexpr int NB = PXT / BW;                                  // union blocks per thread
    constexpr int IRH = BH >> ICSY, ORH = BH >> OCSY;             // chroma rows per thread, in / out
    constexpr int IBX = BW >> ICSX, OBX = BW >> OCSX;             // chroma samples per union block and row, in / out
    constexpr int CWI = (PXT >> ICSX) * (WIN ? 2 : 1) / 4, CWO = (PXT >> OCSX) * (WOUT ? 2 : 1) / 4;
    static_assert(NB >= 1 && CWI >= 1 && CWO >= 1 && YWO >= 1, "a thread must own whole words");
#ifdef LUTR_SK_SEMI
    static_assert(ICSX == 1 || OCSX == 1, "a semi-planar side is 4:2:0 or 4:2:2");
    const unsigned ish = (unsigned)A.ishift;
#endif
    CdlConsts C{S.cdl_tab, S.stride, S.sat};
    const uint16_t *l1d = S.l1d_tab;
    if constexpr (LDS) {
        stack_stage_tables(S);
        C.tab = (const float *)stack_lds;
        l1d = (const uint16_t *)(stack_lds + S.lds_cdl_words);
    }
    const unsigned uw = (unsigned)G.w / PXT;
    const unsigned ub = (unsigned)G.rows >> CSY;
    const unsigned total = uw * ub * (unsigned)G.nframes;
    for (unsigned u = blockIdx.x * 256u + threadIdx.x; u < total; u += gridDim.x * 256u) {
        const unsigned xu = u % uw, t = u / uw;
        const int y0 = ((G.row0 >> CSY) + (int)(t % ub)) * BH;    // first luma row of the thread
        const long long fr = t / ub;
        const long long xi = (long long)xu * VB, xo = (long long)xu * (YWO * 4), cxi = (long long)xu * (CWI * 4),
                        cxo = (long long)xu * (CWO * 4);
#ifdef LUTR_SK_MIX
        const float strength = mix_strength(M, fr);
#endif
#ifdef LUTR_SK_MATTE
        // the matte samples of the thread's BH rows x PXT luma samples: whole dwords in every container mix this is built for
        constexpr int MWI = PXT * (WM ? 2 : 1) / 4;
        static_assert(MWI >= 1, "a thread must own whole matte words");
        const uint8_t *mrow = A.data + fr * A.fstride + (long long)y0 * A.stride + (long long)xu * (MWI * 4);
        uint32_t mw[BH][MWI];
#pragma unroll
        for (int dy = 0; dy < BH; dy++) ld_words<MWI>(mw[dy], mrow + dy * A.stride);
#endif

        uint32_t yw[BH][YWI], cbw[IRH][CWI], crw[IRH][CWI];
        uint32_t yo[BH][YWO], cbo[ORH][CWO], cro[ORH][CWO];
#pragma unroll
        for (int dy = 0; dy < BH; dy++) {
            ld_words<YWI>(yw[dy], P.s[0] + fr * P.sfs[0] + (long long)(y0 + dy) * P.ss[0] + xi);
#pragma unroll
            for (int k = 0; k < YWO; k++) yo[dy][k] = 0;
        }
#pragma unroll
        for (int iy = 0; iy < IRH; iy++) {
            const long long r = (long long)((y0 >> ICSY) + iy);
#ifdef LUTR_SK_SEMI
            // a plane of pairs: ONE load of twice the width, then the pairs taken apart in registers
            if (ICSX == 1 && A.isemi) {
                if constexpr (ICSX == 1) {
                    uint32_t pw[2 * CWI];
                    ld_words<2 * CWI>(pw, P.s[1] + fr * P.sfs[1] + r * P.ss[1] + 2 * cxi);
                    const uint32_t scb = A.iswap ? SemiSel<WIN>::split1 : SemiSel<WIN>::split0;
                    const uint32_t scr = A.iswap ? SemiSel<WIN>::split0 : SemiSel<WIN>::split1;
#pragma unroll
                    for (int k = 0; k < CWI; k++) {
                        cbw[iy][k] = __builtin_amdgcn_perm(pw[2 * k + 1], pw[2 * k], scb);
                        crw[iy][k] = __builtin_amdgcn_perm(pw[2 * k + 1], pw[2 * k], scr);
                    }
                }
            } else
#endif
            {
                ld_words<CWI>(cbw[iy], P.s[1] + fr * P.sfs[1] + r * P.ss[1] + cxi);
                ld_words<CWI>(crw[iy], P.s[2] + fr * P.sfs[2] + r * P.ss[2] + cxi);
            }
        }
#pragma unroll
        for (int oy = 0; oy < ORH; oy++)
#pragma unroll
            for (int k = 0; k < CWO; k++) { cbo[oy][k] = 0; cro[oy][k] = 0; }

#pragma unroll
        for (int j = 0; j < NB; j++) {
            Chroma c[IRH][IBX];
#pragma unroll
            for (int iy = 0; iy < IRH; iy++)
#pragma unroll
                for (int ix = 0; ix < IBX; ix++)
                    c[iy][ix] = chroma_terms(K, SK_CODE(cbw[iy], j * IBX + ix), SK_CODE(crw[iy], j * IBX + ix));
            Rgb px[BH * BW];
#pragma unroll
            for (int dy = 0; dy < BH; dy++)
#pragma unroll
                for (int dx = 0; dx < BW; dx++)
                    px[dy * BW + dx] = yuv_to_rgb(K, SK_CODE(yw[dy], j * BW + dx), c[dy >> ICSY][dx >> ICSX]);
#ifdef LUTR_SK_MIX
            // q0 across the step walk.  A copy of the block (Rgb px0[BH * BW]) is 12 VGPRs at 4:2:0 and takes the tetrahedral
            // instances from 4 waves to 3 (DESIGN.md 3.22 point 5).  Where the block's chroma terms are fewer than its pixels, q0 is
            // evaluated again behind the walk instead -- from the luma words, which stay live for the thread's other blocks anyway,
            // and the chroma terms: the same operations on the same inputs, so the same bits.  The fence keeps hipcc from reusing
            // the first evaluation, which would keep the copy alive after all.
            constexpr bool AGAIN = IRH * IBX < BH * BW;
            Rgb px0[AGAIN ? 1 : BH * BW];
            if constexpr (!AGAIN) {
#pragma unroll
                for (int i = 0; i < BH * BW; i++) px0[i] = px[i];
            }
#endif
            stack_block<TRI>(S, C, l1d, L, L2, px SK_MTX_ARG);
#ifdef LUTR_SK_MATTE
            // the block's weights, in the mix's order
            float wgt[BH * BW];
#pragma unroll
            for (int dy = 0; dy < BH; dy++)
#pragma unroll
                for (int dx = 0; dx < BW; dx++) {
                    wgt[dy * BW + dx] = matte_weight(A, strength, word_sample<WM>(mw[dy], j * BW + dx));
                }
#define SK_STRENGTH(i) wgt[i]
#else
#define SK_STRENGTH(i) strength
#endif
#ifdef LUTR_SK_MIX
            if constexpr (AGAIN) {
#pragma unroll
                for (int dy = 0; dy < BH; dy++) {
#pragma unroll
                    for (int k = 0; k < YWI; k++) asm volatile("" : "+v"(yw[dy][k]));
#pragma unroll
                    for (int dx = 0; dx < BW; dx++) {
                        const Rgb q0 = yuv_to_rgb(K, word_sample<WIN>(yw[dy], j * BW + dx), c[dy >> ICSY][dx >> ICSX]);
                        px[dy * BW + dx] = mix_px(SK_STRENGTH(dy * BW + dx), q0, px[dy * BW + dx]);
                    }
                }
            } else {
#pragma unroll
                for (int i = 0; i < BH * BW; i++) px[i] = mix_px(SK_STRENGTH(i), px0[i], px[i]);
            }
#endif
#undef SK_STRENGTH
            float rs[ORH][OBX], gs[ORH][OBX], bs[ORH][OBX];
#pragma unroll
            for (int oy = 0; oy < ORH; oy++)
#pragma unroll
                for (int ox = 0; ox < OBX; ox++) { rs[oy][ox] = 0.f; gs[oy][ox] = 0.f; bs[oy][ox] = 0.f; }
#pragma unroll
            for (int dy = 0; dy < BH; dy++) {
#pragma unroll
                for (int dx = 0; dx < BW; dx++) {
                    const Rgb o = px[dy * BW + dx];
                    rs[dy >> OCSY][dx >> OCSX] += o.r; gs[dy >> OCSY][dx >> OCSX] += o.g; bs[dy >> OCSY][dx >> OCSX] += o.b;
                    word_put<WOUT>(yo[dy], j * BW + dx, rgb_to_y(K, o));
                }
            }
#pragma unroll
            for (int oy = 0; oy < ORH; oy++)
#pragma unroll
                for (int ox = 0; ox < OBX; ox++) {
                    const int i = j * OBX + ox;
                    word_put<WOUT>(cbo[oy], i, rgb_to_cb(K, rs[oy][ox], gs[oy][ox], bs[oy][ox]));
                    word_put<WOUT>(cro[oy], i, rgb_to_cr(K, rs[oy][ox], gs[oy][ox], bs[oy][ox]));
                }
            // Zero-instruction fence (k_yuv_vec's): keeps hipcc from hoisting the coordinates and taps of every union block of the
            // thread to the top; with it the blocks are emitted one after the other.
#pragma unroll
            for (int dy = 0; dy < BH; dy++) {
#pragma unroll
                for (int k = 0; k < YWI; k++) asm volatile("" : "+v"(yw[dy][k]));
#pragma unroll
                for (int k = 0; k < YWO; k++) asm volatile("" : "+v"(yo[dy][k]));
#ifdef LUTR_SK_MATTE
#pragma unroll
                for (int k = 0; k < MWI; k++) asm volatile("" : "+v"(mw[dy][k]));
#endif
            }
#pragma unroll
            for (int iy = 0; iy < IRH; iy++)
#pragma unroll
                for (int k = 0; k < CWI; k++) asm volatile("" : "+v"(cbw[iy][k]), "+v"(crw[iy][k]));
#pragma unroll
            for (int oy = 0; oy < ORH; oy++)
#pragma unroll
                for (int k = 0; k < CWO; k++) asm volatile("" : "+v"(cbo[oy][k]), "+v"(cro[oy][k]));
        }
#ifdef LUTR_SK_SEMI
        // the container's alignment: one shift per packed word -- two codes below 2^depth cannot carry into each other
        if constexpr (WOUT) {
            const unsigned osh = (unsigned)A.oshift;
#pragma unroll
            for (int dy = 0; dy < BH; dy++)
#pragma unroll
                for (int k = 0; k < YWO; k++) yo[dy][k] <<= osh;
#pragma unroll
            for (int oy = 0; oy < ORH; oy++)
#pragma unroll
                for (int k = 0; k < CWO; k++) { cbo[oy][k] <<= osh; cro[oy][k] <<= osh; }
        }
#endif
#pragma unroll
        for (int dy = 0; dy < BH; dy++)
            st_words<YWO>(P.d[0] + fr * P.dfs[0] + (long long)(y0 + dy) * P.ds[0] + xo, yo[dy]);
#pragma unroll
        for (int oy = 0; oy < ORH; oy++) {
            const long long r = (long long)((y0 >> OCSY) + oy);
#ifdef LUTR_SK_SEMI
            // a plane of pairs: the two components put together in registers, then ONE store of twice the width
            if (OCSX == 1 && A.osemi) {
                if constexpr (OCSX == 1) {
                    uint32_t pw[2 * CWO];
                    const uint32_t s0 = A.oswap ? SemiSel<WOUT>::join0s : SemiSel<WOUT>::join0;
                    const uint32_t s1 = A.oswap ? SemiSel<WOUT>::join1s : SemiSel<WOUT>::join1;
#pragma unroll
                    for (int k = 0; k < CWO; k++) {
                        pw[2 * k] = __builtin_amdgcn_perm(cro[oy][k], cbo[oy][k], s0);
                        pw[2 * k + 1] = __builtin_amdgcn_perm(cro[oy][k], cbo[oy][k], s1);
                    }
                    st_words<2 * CWO>(P.d[1] + fr * P.dfs[1] + r * P.ds[1] + 2 * cxo, pw);
                }
            } else
#endif
            {
                st_words<CWO>(P.d[1] + fr * P.dfs[1] + r * P.ds[1] + cxo, cbo[oy]);
                st_words<CWO>(P.d[2] + fr * P.dfs[2] + r * P.ds[2] + cxo, cro[oy]);
            }
        }
    }
}

// The vector kernels of this translation unit's container mix; the layout checks are the caller's (launch_yuv_stack).  The grid:
// with tables in LDS, eight workgroups a CU, each staging once and walking its share of the units; without, the usual cap.
const char *SK_VEC_LAUNCH_FN(hipStream_t st, const LutConsts &L, const LutConsts &L2, const StackConsts &S, const YuvConsts &K,
                             const PlaneSet &P, const FrameGeom &G, int icsx, int icsy, int ocsx, int ocsy, bool tri,
                             bool lds SK_MIX_PARAM)
{
    constexpr int WI = LUTR_SK_WI, WO = LUTR_SK_WO;
    const dim3 grid(stride_grid(LUTR_STR(SK_VEC), union_units<WI, WO>(G, icsy, ocsy), lds ? (unsigned)device_cus() * 8u : kGridStrideCap)), block(256);
    const size_t lds_bytes = lds ? (size_t)(S.lds_cdl_words + S.lds_l1d_words) * sizeof(uint32_t) : 0;
#define SK_CASE(IX, IY, OX, OY, T) \
    if (icsx == IX && icsy == IY && ocsx == OX && ocsy == OY && tri == (T != 0)) { \
        if (lds) hipLaunchKernelGGL((SK_VEC<WI, WO, SK_WM_TARG IX, IY, OX, OY, T != 0, true>), grid, block, lds_bytes, st, L, L2, S, K, P, G SK_MIX_ARG); \
        else hipLaunchKernelGGL((SK_VEC<WI, WO, SK_WM_TARG IX, IY, OX, OY, T != 0, false>), grid, block, 0, st, L, L2, S, K, P, G SK_MIX_ARG); \
        return lds ? SK_VEC_NAME LUTR_STR(LUTR_SK_WI) "," LUTR_STR(LUTR_SK_WO) "," SK_WM_NAME #IX "," #IY "," #OX "," #OY "," #T ",1>" \
                   : SK_VEC_NAME LUTR_STR(LUTR_SK_WI) "," LUTR_STR(LUTR_SK_WO) "," SK_WM_NAME #IX "," #IY "," #OX "," #OY "," #T ",0>"; \
    }
#define SK_PAIR(IX, IY, OX, OY) SK_CASE(IX, IY, OX, OY, 0) SK_CASE(IX, IY, OX, OY, 1)
#ifdef LUTR_SK_SEMI
    // the eight pairs with a 4:2:0 / 4:2:2 side: 4:4:4 -> 4:4:4 has no side a plane of pairs or a shifted container could be
    SK_PAIR(1, 1, 1, 1) SK_PAIR(1, 1, 1, 0) SK_PAIR(1, 1, 0, 0) SK_PAIR(1, 0, 1, 1) SK_PAIR(1, 0, 1, 0) SK_PAIR(1, 0, 0, 0)
    SK_PAIR(0, 0, 1, 1) SK_PAIR(0, 0, 1, 0)
#else
    LUTR_UNION_PAIRS(SK_PAIR)
#endif
#undef SK_PAIR
#undef SK_CASE
    return nullptr;
}

#else  // !LUTR_SK_WI
// ================================================================= generic kernel
// One thread per union block; any depth, stride or alignment, odd sizes, all five modes on either lattice.  xsub_union_block's
// walk (lutr_device.h) with the step list per pixel (the tables read from global memory), then (MIX, MATTE) the mix with the
// pixel's own q; the matte form reads its sample at the pixel's clamped (x, y).  M and A are null in the forms without them, and
// so is X: the matrix form is the plain one with X set, and its steps are in its translation unit only.
// the step list on one pixel, at run-time modes: what every generic kernel of this file runs between the two conversion stages
__device__ __forceinline__ Rgb stack_walk_rt(const LutConsts &L, const GFetch &f, const LutConsts &L2, const GFetch &f2,
                                             const StackConsts &S, const CdlConsts &C, bool mix, const MtxConsts *X, const Rgb &q)
{
    Rgb o = q;
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
#ifdef LUTR_SK_MTX
        case STACK_OP_MTX_CODES:  o = mtx_px(*X, X->rcp, o); break;
        case STACK_OP_MTX_UNIT:   o = mtx_px(*X, 1.0f, o); break;
#endif
        default:                  o = lut3d_unit_rt(mode, L2, f2, o); break;
        }
    }
    return o;
}

template <int FORM>
__device__ __forceinline__ void stack_generic(const LutConsts &L, const LutConsts &L2, const StackConsts &S, const YuvConsts &K,
                                              const PlaneSet &P, const FrameGeom &G, const MixConsts *M, const MatteConsts *A,
                                              const MtxConsts *X, int win, int wout, int icsx, int icsy, int ocsx, int ocsy)
{
    const GFetch f(L), f2(L2);
    PlaneSink sink{K, P, wout};
    const CdlConsts C{S.cdl_tab, S.stride, S.sat};
    const bool mix = S.sat != 1.0f;
    for_each_block(G, cmax(icsx, ocsx), cmax(icsy, ocsy), false, [&](long long fr, int ux, int uy) {
        float strength = 0.0f;
        if constexpr (FORM != SK_PLAIN) strength = mix_strength(*M, fr);
        xsub_union_block(K, P, G, fr, ux, uy, win, icsx, icsy, ocsx, ocsy, sink, [&](long long fr, int x, int y, const Rgb &q) {
            float wgt = strength;
            if constexpr (FORM == SK_MATTE)
                wgt = matte_weight(*A, strength, ld_sample(A->data + fr * A->fstride + (long long)y * A->stride, x, A->wide));
            Rgb o = stack_walk_rt(L, f, L2, f2, S, C, mix, X, q);
            if constexpr (FORM != SK_PLAIN) o = mix_px(wgt, q, o);
            return o;
        });
    });
}

// this translation unit's kernel and its launch: the one place that says which form it holds
#if defined(LUTR_SKS_GENERIC)
// The semi form: one thread per union block, with its own walk of the block, since every sample goes through its
// side's container (ld_code / st_code; chroma sample cx of a plane of pairs is element 2 cx + (swap ? 1 : 0) for Cb and 2 cx +
// (swap ? 0 : 1) for Cr of plane 1).  The arithmetic and the edges are xsub_union_block's: every pixel reads the chroma sample of
// its own input block, a pixel outside the frame is the edge pixel again, the pixels are summed in raster order into the
// accumulators of their output blocks, and only samples inside the planes are written.  All of a block's codes are read before
// anything is stored.
__global__ __launch_bounds__(256) void k_yuv_stack_semi_generic(LutConsts L, LutConsts L2, StackConsts S, YuvConsts K, PlaneSet P,
                                                                FrameGeom G, SemiArgs A, int win, int wout, int icsx, int icsy,
                                                                int ocsx, int ocsy)
{
    const GFetch f(L), f2(L2);
    const CdlConsts C{S.cdl_tab, S.stride, S.sat};
    const bool mix = S.sat != 1.0f;
    const int csx = cmax(icsx, ocsx), csy = cmax(icsy, ocsy), bw = 1 << csx, bh = 1 << csy;
    const int cwo = (G.w + (1 << ocsx) - 1) >> ocsx, cho = (G.h + (1 << ocsy) - 1) >> ocsy;
    // where Cb and Cr of a chroma sample are: plane, elements per sample and the component's element inside a pair
    const int icr = A.isemi ? 1 : 2, ocr = A.osemi ? 1 : 2;
    const int im = A.isemi ? 2 : 1, om = A.osemi ? 2 : 1;
    const int icb0 = A.isemi ? A.iswap : 0, icr0 = A.isemi ? 1 - A.iswap : 0;
    const int ocb0 = A.osemi ? A.oswap : 0, ocr0 = A.osemi ? 1 - A.oswap : 0;
    for_each_block(G, csx, csy, false, [&](long long fr, int ux, int uy) {
        // the block's codes, pixel i = 2 * dy + dx (a union block is at most 2 x 2)
        float yv[4], cbv[4], crv[4];
#pragma unroll
        for (int i = 0; i < 4; i++) {
            const int dy = i >> 1, dx = i & 1;
            yv[i] = 0.f; cbv[i] = 0.f; crv[i] = 0.f;
            if (dy < bh && dx < bw) {
                const int yy = uy * bh + dy, y = yy < G.h ? yy : G.h - 1;
                const int xx = ux * bw + dx, x = xx < G.w ? xx : G.w - 1;
                const long long cx = x >> icsx;
                yv[i] = ld_code(src_row(P, 0, fr, y), x, win, A.ishift);
                cbv[i] = ld_code(src_row(P, 1, fr, y >> icsy), cx * im + icb0, win, A.ishift);
                crv[i] = ld_code(src_row(P, icr, fr, y >> icsy), cx * im + icr0, win, A.ishift);
            }
        }
        // output chroma block k = 2 * (dy >> ocsy) + (dx >> ocsx) of the union block
        float rs[4] = {0.f, 0.f, 0.f, 0.f}, gs[4] = {0.f, 0.f, 0.f, 0.f}, bs[4] = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int i = 0; i < 4; i++) {
            const int dy = i >> 1, dx = i & 1;
            if (dy < bh && dx < bw) {
                const int yy = uy * bh + dy, y = yy < G.h ? yy : G.h - 1;
                const int xx = ux * bw + dx, x = xx < G.w ? xx : G.w - 1;
                const Rgb o = stack_walk_rt(L, f, L2, f2, S, C, mix, nullptr, yuv_to_rgb(K, yv[i], chroma_terms(K, cbv[i], crv[i])));
                const int k = 2 * (dy >> ocsy) + (dx >> ocsx);
#pragma unroll
                for (int kk = 0; kk < 4; kk++)
                    if (k == kk) { rs[kk] += o.r; gs[kk] += o.g; bs[kk] += o.b; }
                if (yy < G.h && xx < G.w) st_code(dst_row(P, 0, fr, y), x, wout, A.oshift, rgb_to_y(K, o));
            }
        }
#pragma unroll
        for (int kk = 0; kk < 4; kk++) {
            const int oy = kk >> 1, ox = kk & 1;
            const long long ocx = ((ux * bw) >> ocsx) + ox;
            const int ocy = ((uy * bh) >> ocsy) + oy;
            if (oy < (bh >> ocsy) && ox < (bw >> ocsx) && ocx < cwo && ocy < cho) {
                st_code(dst_row(P, 1, fr, ocy), ocx * om + ocb0, wout, A.oshift, rgb_to_cb(K, rs[kk], gs[kk], bs[kk]));
                st_code(dst_row(P, ocr, fr, ocy), ocx * om + ocr0, wout, A.oshift, rgb_to_cr(K, rs[kk], gs[kk], bs[kk]));
            }
        }
    });
}

// its launch, for the launcher in the plain translation unit
const char *launch_yuv_stack_semi_generic(hipStream_t st, unsigned grid, const LutConsts &L, const LutConsts &L2, const StackConsts &S,
                                          const YuvConsts &K, const PlaneSet &P, const FrameGeom &G, const SemiArgs &A, int win,
                                          int wout, int icsx, int icsy, int ocsx, int ocsy)
{
    hipLaunchKernelGGL(k_yuv_stack_semi_generic, dim3(grid), dim3(256), 0, st, L, L2, S, K, P, G, A, win, wout, icsx, icsy, ocsx, ocsy);
    return "k_yuv_stack_semi_generic";
}
#elif defined(LUTR_SKA_GENERIC)
__global__ __launch_bounds__(256) void k_yuv_stack_matte_generic(LutConsts L, LutConsts L2, StackConsts S, YuvConsts K, PlaneSet P,
                                                                 FrameGeom G, MixConsts M, MatteConsts A, int win, int wout, int icsx,
                                                                 int icsy, int ocsx, int ocsy)
{
    stack_generic<SK_MATTE>(L, L2, S, K, P, G, &M, &A, nullptr, win, wout, icsx, icsy, ocsx, ocsy);
}

// its launch, for the launcher in the plain translation unit
const char *launch_yuv_stack_matte_generic(hipStream_t st, unsigned grid, const LutConsts &L, const LutConsts &L2, const StackConsts &S,
                                           const YuvConsts &K, const PlaneSet &P, const FrameGeom &G, const MixConsts &M,
                                           const MatteConsts &A, int win, int wout, int icsx, int icsy, int ocsx, int ocsy)
{
    hipLaunchKernelGGL(k_yuv_stack_matte_generic, dim3(grid), dim3(256), 0, st, L, L2, S, K, P, G, M, A, win, wout, icsx, icsy, ocsx,
                       ocsy);
    return "k_yuv_stack_matte_generic";
}
#elif defined(LUTR_SKX_GENERIC)
__global__ __launch_bounds__(256) void k_yuv_stack_mtx_generic(LutConsts L, LutConsts L2, StackConsts S, YuvConsts K, PlaneSet P,
                                                               FrameGeom G, MtxConsts X, int win, int wout, int icsx, int icsy,
                                                               int ocsx, int ocsy)
{
    stack_generic<SK_PLAIN>(L, L2, S, K, P, G, nullptr, nullptr, &X, win, wout, icsx, icsy, ocsx, ocsy);
}

// its launch, for the launcher in the plain translation unit
const char *launch_yuv_stack_mtx_generic(hipStream_t st, unsigned grid, const LutConsts &L, const LutConsts &L2, const StackConsts &S,
                                         const YuvConsts &K, const PlaneSet &P, const FrameGeom &G, const MtxConsts &X, int win,
                                         int wout, int icsx, int icsy, int ocsx, int ocsy)
{
    hipLaunchKernelGGL(k_yuv_stack_mtx_generic, dim3(grid), dim3(256), 0, st, L, L2, S, K, P, G, X, win, wout, icsx, icsy, ocsx, ocsy);
    return "k_yuv_stack_mtx_generic";
}
#elif defined(LUTR_SKM_GENERIC)
__global__ __launch_bounds__(256) void k_yuv_stack_mix_generic(LutConsts L, LutConsts L2, StackConsts S, YuvConsts K, PlaneSet P,
                                                               FrameGeom G, MixConsts M, int win, int wout, int icsx, int icsy,
                                                               int ocsx, int ocsy)
{
    stack_generic<SK_MIX>(L, L2, S, K, P, G, &M, nullptr, nullptr, win, wout, icsx, icsy, ocsx, ocsy);
}

// its launch, for the launcher in the plain translation unit
const char *launch_yuv_stack_mix_generic(hipStream_t st, unsigned grid, const LutConsts &L, const LutConsts &L2, const StackConsts &S,
                                         const YuvConsts &K, const PlaneSet &P, const FrameGeom &G, const MixConsts &M, int win,
                                         int wout, int icsx, int icsy, int ocsx, int ocsy)
{
    hipLaunchKernelGGL(k_yuv_stack_mix_generic, dim3(grid), dim3(256), 0, st, L, L2, S, K, P, G, M, win, wout, icsx, icsy, ocsx, ocsy);
    return "k_yuv_stack_mix_generic";
}
#else
__global__ __launch_bounds__(256) void k_yuv_stack_generic(LutConsts L, LutConsts L2, StackConsts S, YuvConsts K, PlaneSet P, FrameGeom G,
                                                           int win, int wout, int icsx, int icsy, int ocsx, int ocsy)
{
    stack_generic<SK_PLAIN>(L, L2, S, K, P, G, nullptr, nullptr, nullptr, win, wout, icsx, icsy, ocsx, ocsy);
}

// ================================================================= launcher
// (where the vector kernels read the CDL and 1D tables: stack_in_lds, lutr_launch.h; the default follows 3.20's measurement of
// the 1D table)
constexpr bool kStackLdsDefault = true;

const char *launch_yuv_stack(hipStream_t st, int variant, const LutConsts &L, const LutConsts &L2, const StackConsts &S,
                             const YuvConsts &K, const PlaneSet &P, const FrameGeom &G, int din, int dout, int icsx, int icsy,
                             int ocsx, int ocsy, const MixConsts *M, const MatteConsts *A, const MtxConsts *X)
{
    const UnionLaunch U(G, din, dout, icsx, icsy, ocsx, ocsy);
    const bool lds = stack_in_lds(S, kStackLdsDefault);
    // the lattice steps' modes: the vector kernels have nearest / trilinear / tetrahedral
    bool modes_ok = true, tri = false;
    for (unsigned long long ops = S.ops; ops & 0xffull; ops >>= 8) {
        const int op = (int)(ops & 15u), mode = (int)((ops >> 4) & 15u);
        if (op == STACK_OP_L1D || op == STACK_OP_CDL || op == STACK_OP_ROUND || op == STACK_OP_MTX_CODES || op == STACK_OP_MTX_UNIT) continue;
        modes_ok = modes_ok && vec_mode(mode);
        tri = tri || mode == LUTR_INTERP_TRILINEAR;
    }
    // the matte kernels: built for the source's container and for bytes beside a 16-bit source; whole aligned dwords a thread
    const bool matte_ok = !A || (A->wide <= U.win && U.luma_plane_fits(A->data, A->stride, A->fstride, A->wide));
    auto vec = [&](const PlaneSet &Q, const FrameGeom &H) -> const char * {
        if (A) {
            if (U.win && U.wout)
                return A->wide ? launch_yuv_stack_matte_vec_w111(st, L, L2, S, K, Q, H, icsx, icsy, ocsx, ocsy, tri, lds, *M, *A)
                               : launch_yuv_stack_matte_vec_w110(st, L, L2, S, K, Q, H, icsx, icsy, ocsx, ocsy, tri, lds, *M, *A);
            if (U.win)
                return A->wide ? launch_yuv_stack_matte_vec_w101(st, L, L2, S, K, Q, H, icsx, icsy, ocsx, ocsy, tri, lds, *M, *A)
                               : launch_yuv_stack_matte_vec_w100(st, L, L2, S, K, Q, H, icsx, icsy, ocsx, ocsy, tri, lds, *M, *A);
            return launch_yuv_stack_matte_vec_w000(st, L, L2, S, K, Q, H, icsx, icsy, ocsx, ocsy, tri, lds, *M, *A);
        }
        if (M) {
            if (U.win && U.wout) return launch_yuv_stack_mix_vec_w11(st, L, L2, S, K, Q, H, icsx, icsy, ocsx, ocsy, tri, lds, *M);
            if (U.win) return launch_yuv_stack_mix_vec_w10(st, L, L2, S, K, Q, H, icsx, icsy, ocsx, ocsy, tri, lds, *M);
            return launch_yuv_stack_mix_vec_w00(st, L, L2, S, K, Q, H, icsx, icsy, ocsx, ocsy, tri, lds, *M);
        }
        if (X) {
            if (U.win && U.wout) return launch_yuv_stack_mtx_vec_w11(st, L, L2, S, K, Q, H, icsx, icsy, ocsx, ocsy, tri, lds, *X);
            if (U.win) return launch_yuv_stack_mtx_vec_w10(st, L, L2, S, K, Q, H, icsx, icsy, ocsx, ocsy, tri, lds, *X);
            return launch_yuv_stack_mtx_vec_w00(st, L, L2, S, K, Q, H, icsx, icsy, ocsx, ocsy, tri, lds, *X);
        }
        if (U.win && U.wout) return launch_yuv_stack_vec_w11(st, L, L2, S, K, Q, H, icsx, icsy, ocsx, ocsy, tri, lds);
        if (U.win) return launch_yuv_stack_vec_w10(st, L, L2, S, K, Q, H, icsx, icsy, ocsx, ocsy, tri, lds);
        return launch_yuv_stack_vec_w00(st, L, L2, S, K, Q, H, icsx, icsy, ocsx, ocsy, tri, lds);
    };
    const char *const generic_name = A ? "k_yuv_stack_matte_generic" : M ? "k_yuv_stack_mix_generic" : X ? "k_yuv_stack_mtx_generic" : "k_yuv_stack_generic";
    auto generic = [&](const PlaneSet &Q, const FrameGeom &H, int x0) {
        const unsigned grid = U.generic_grid(generic_name, H);
        if (A) {
            // the tail of a column split: the matte moves right with the source's luma plane
            MatteConsts B = *A;
            B.data += (long long)x0 * (A->wide ? 2 : 1);
            return launch_yuv_stack_matte_generic(st, grid, L, L2, S, K, Q, H, *M, B, U.win, U.wout, icsx, icsy, ocsx, ocsy);
        }
        if (M) return launch_yuv_stack_mix_generic(st, grid, L, L2, S, K, Q, H, *M, U.win, U.wout, icsx, icsy, ocsx, ocsy);
        if (X) return launch_yuv_stack_mtx_generic(st, grid, L, L2, S, K, Q, H, *X, U.win, U.wout, icsx, icsy, ocsx, ocsy);
        hipLaunchKernelGGL(k_yuv_stack_generic, dim3(grid), dim3(256), 0, st, L, L2, S, K, Q, H, U.win, U.wout, icsx, icsy, ocsx, ocsy);
        return generic_name;
    };
    return launch_union(variant, P, G, U, modes_ok && matte_ok, vec, generic, generic_name);
}

// The semi form's launcher: launch_yuv_stack's plain route with the containers of the two sides.  The unit and the
// container mixes are UnionLaunch's; its plane checks and the tail of a column split know that a plane of pairs moves twice a planar
// chroma plane's bytes.  No vector kernel for 4:4:4 -> 4:4:4 (neither side can be a plane of pairs).
const char *launch_yuv_stack_semi(hipStream_t st, int variant, const LutConsts &L, const LutConsts &L2, const StackConsts &S,
                                  const YuvConsts &K, const PlaneSet &P, const FrameGeom &G, const SemiArgs &A, int din, int dout,
                                  int icsx, int icsy, int ocsx, int ocsy)
{
    const UnionLaunch U(G, din, dout, icsx, icsy, ocsx, ocsy, A.isemi != 0, A.osemi != 0);
    const bool lds = stack_in_lds(S, kStackLdsDefault);
    bool modes_ok = icsx == 1 || ocsx == 1, tri = false;
    for (unsigned long long ops = S.ops; ops & 0xffull; ops >>= 8) {
        const int op = (int)(ops & 15u), mode = (int)((ops >> 4) & 15u);
        if (op == STACK_OP_L1D || op == STACK_OP_CDL || op == STACK_OP_ROUND) continue;
        modes_ok = modes_ok && vec_mode(mode);
        tri = tri || mode == LUTR_INTERP_TRILINEAR;
    }
    auto vec = [&](const PlaneSet &Q, const FrameGeom &H) -> const char * {
        if (U.win && U.wout) return launch_yuv_stack_semi_vec_w11(st, L, L2, S, K, Q, H, icsx, icsy, ocsx, ocsy, tri, lds, A);
        if (U.win) return launch_yuv_stack_semi_vec_w10(st, L, L2, S, K, Q, H, icsx, icsy, ocsx, ocsy, tri, lds, A);
        return launch_yuv_stack_semi_vec_w00(st, L, L2, S, K, Q, H, icsx, icsy, ocsx, ocsy, tri, lds, A);
    };
    const char *const generic_name = "k_yuv_stack_semi_generic";
    auto generic = [&](const PlaneSet &Q, const FrameGeom &H, int) {
        return launch_yuv_stack_semi_generic(st, U.generic_grid(generic_name, H), L, L2, S, K, Q, H, A, U.win, U.wout, icsx, icsy, ocsx,
                                             ocsy);
    };
    return launch_union(variant, P, G, U, modes_ok, vec, generic, generic_name);
}
#endif  // the generic forms

#endif  // LUTR_SK_WI

}  // namespace lutr
