// lutr_pkstack.hip -- gfx950 kernels of the stage stack on capture frames: packed 4:2:2
// (yuyv422 / uyvy422 / yvyu422, y210le / y212le / y216le; 3.12) and v210 (3.14), on the source side, the destination side or both.
//
// What they replace: the unpacking of a capture card's frame into yuv422p* ahead of lutr_apply_yuv_stack and the packing behind it.
// The arithmetic is that call's, untouched: a packed or v210 frame is the samples of yuv422p* in another container, the unit of
// work is one chroma pair over 2^OCSY rows (the union block of a 4:2:2 source and the destination), and the pixels of a pair walk
// the compiled step list (StackConsts::ops, lutr_stack_steps.h) between the YUV -> RGB stage and the RGB -> YUV stage.  Nothing is
// templated on the order of the list.
//
// The load / store shells are those of k_yuv_pk_vec (lutr_pkyuv.hip) and k_yuv_v210_vec (lutr_v210.hip): whole-word runs, every
// code of the thread loaded before anything is stored -- except that a v210 thread takes ONE group and moves the planar side's
// few codes in narrower accesses (see k_yuv_stack_v210_vec).  The walk is k_yuv_stack_vec's (lutr_stack.hip): a grid stride, so that a
// workgroup stages the CDL and 1D tables into LDS once (LDS = true); LDS = false reads them from global memory through L1.  Both
// read the same entries: the bits do not depend on the choice.
//
// A call has packed 4:2:2 sides or v210 sides, not both kinds: uyvy422 -> v210 would be a third vector family (a thread of whole
// v210 groups, 6 luma samples, against runs of 4 or 8) for a conversion no capture path needs, and is refused by name one layer up.
//
// One source, three kinds of translation unit (Makefile MIX_RULE):
//   without a switch      the two generic kernels and the two launchers
//   LUTR_PKS_WI / _WO     the packed 4:2:2 vector kernels of one container mix (8 -> 8, 16 -> 16, 16 -> 8): 4 side pairs x (any
//                         stage trilinear) x 2 placements
//   LUTR_VKS_WI / _WO     the v210 vector kernels of one container mix, a v210 side counted as 16 bit (w11, w10; lutr_v210.hip)
#define SK_MTX_PARAM
#include "lutr_device.h"
#include "lutr_launch.h"
#include "lutr_pkcodes.h"
#include "lutr_stack_steps.h"   // stack_stage_to, stack_block, the per-pixel steps

namespace lutr {

#if defined(LUTR_PKS_WI) || defined(LUTR_VKS_WI)
extern __shared__ uint32_t pks_lds[];                             // the staged tables: the CDL's floats, then the 1D table's uint16

// the grid of k_yuv_stack_vec: with tables in LDS, eight workgroups a CU, each staging once and walking its share of the units
static dim3 pks_grid(const char *family, long long units, bool lds)
{
    return dim3(stride_grid(family, units, lds ? (unsigned)device_cus() * 8u : kGridStrideCap));
}
static size_t pks_lds_bytes(const StackConsts &S, bool lds)
{
    return lds ? (size_t)(S.lds_cdl_words + S.lds_l1d_words) * sizeof(uint32_t) : 0;
}
#endif

#if defined(LUTR_PKS_WI)
// ================================================================= packed 4:2:2: vector kernel
// k_yuv_pk_vec's shell.  PI / PO: the source / destination is packed.  The source is always 4:2:2; OCSY = 1 is a planar 4:2:0
// destination.  TRI: some stage is trilinear.  No thread leaves before the barrier behind the staging.
template <int WIN, int WOUT, int PI, int PO, int OCSY, bool TRI, bool LDS>
__global__ __launch_bounds__(256) void k_yuv_stack_pk_vec(LutConsts L, LutConsts L2, StackConsts S, YuvConsts K, PlaneSet P,
                                                          FrameGeom G, PkArgs A)
{
    static_assert(PI || PO, "planar on both sides is k_yuv_stack_vec");
    static_assert(!(PO && OCSY), "a packed destination is 4:2:2");
    constexpr int VB = vec_bytes<WIN, WOUT>();
    constexpr int PXT = VB / (WIN ? 2 : 1);                       // luma samples per thread per row
    constexpr int YWI = VB / 4, YWO = PXT * (WOUT ? 2 : 1) / 4;   // luma words per thread per row of a planar side, in / out
    constexpr int BH = 1 << OCSY;                                 // luma rows per thread
    constexpr int NB = PXT / 2;                                   // groups per thread and row
    constexpr int CWI = NB * (WIN ? 2 : 1) / 4, CWO = NB * (WOUT ? 2 : 1) / 4;   // words of ONE chroma component of a planar side
    constexpr int RWI = 2 * YWI, RWO = 2 * YWO;                   // words of one 4:2:2 row, packed or planar
    constexpr int LWO = PO ? RWO : YWO;                           // words of a destination row that hold luma
    static_assert(NB >= 1 && CWI >= 1 && CWO >= 1 && 2 * CWI == YWI && 2 * CWO == YWO, "a thread must own whole words");
    CdlConsts C{S.cdl_tab, S.stride, S.sat};
    const uint16_t *l1d = S.l1d_tab;
    if constexpr (LDS) {
        stack_stage_to(pks_lds, S);
        C.tab = (const float *)pks_lds;
        l1d = (const uint16_t *)(pks_lds + S.lds_cdl_words);
    }
    const unsigned icf = (unsigned)A.icf, icsw = (unsigned)A.icsw, ish = (unsigned)A.ishift;
    const unsigned ocf = (unsigned)A.ocf, ocsw = (unsigned)A.ocsw;
    const unsigned uw = (unsigned)G.w / PXT;
    const unsigned ub = (unsigned)G.rows >> OCSY;
    const unsigned total = uw * ub * (unsigned)G.nframes;
    for (unsigned u = blockIdx.x * 256u + threadIdx.x; u < total; u += gridDim.x * 256u) {
        const unsigned xu = u % uw, t = u / uw;
        const int y0 = ((G.row0 >> OCSY) + (int)(t % ub)) * BH;   // first luma row of the thread
        const long long fr = t / ub;

        // a source row: packed -- RWI words of groups; planar -- luma in [0, YWI), Cb in [YWI, YWI + CWI), Cr behind it.
        // Every code the thread owns is loaded before anything is stored.
        uint32_t in[BH][RWI];
        uint32_t yo[BH][LWO], co[2 * CWO];                        // (co: a planar destination's Cb | Cr row)
#pragma unroll
        for (int dy = 0; dy < BH; dy++) {
            const long long y = (long long)(y0 + dy);
            if constexpr (PI) {
                ld_run<RWI>(in[dy], P.s[0] + fr * P.sfs[0] + y * P.ss[0] + (long long)xu * (RWI * 4));
            } else {
                ld_words<YWI>(in[dy], P.s[0] + fr * P.sfs[0] + y * P.ss[0] + (long long)xu * VB);
                ld_words<CWI>(in[dy] + YWI, P.s[1] + fr * P.sfs[1] + y * P.ss[1] + (long long)xu * (CWI * 4));
                ld_words<CWI>(in[dy] + YWI + CWI, P.s[2] + fr * P.sfs[2] + y * P.ss[2] + (long long)xu * (CWI * 4));
            }
#pragma unroll
            for (int k = 0; k < LWO; k++) yo[dy][k] = 0;
        }
#pragma unroll
        for (int k = 0; k < 2 * CWO; k++) co[k] = 0;

#pragma unroll
        for (int j = 0; j < NB; j++) {
            // the BH x 2 pixels of one chroma pair, in the order the planar stack holds its union block
            Rgb px[BH * 2];
#pragma unroll
            for (int dy = 0; dy < BH; dy++) {
                const float cbv = PI ? pk_chroma<WIN>(in[dy], j, 0u, icf, icsw, ish) : word_sample<WIN>(in[dy] + YWI, j);
                const float crv = PI ? pk_chroma<WIN>(in[dy], j, 1u, icf, icsw, ish) : word_sample<WIN>(in[dy] + YWI + CWI, j);
                const Chroma c = chroma_terms(K, cbv, crv);
#pragma unroll
                for (int dx = 0; dx < 2; dx++) {
                    const float yv = PI ? pk_luma<WIN>(in[dy], j, dx, icf, ish) : word_sample<WIN>(in[dy], 2 * j + dx);
                    px[dy * 2 + dx] = yuv_to_rgb(K, yv, c);
                }
            }
            stack_block<TRI>(S, C, l1d, L, L2, px);
            float rs = 0.f, gs = 0.f, bs = 0.f;
#pragma unroll
            for (int dy = 0; dy < BH; dy++) {
#pragma unroll
                for (int dx = 0; dx < 2; dx++) {
                    const Rgb o = px[dy * 2 + dx];
                    rs += o.r; gs += o.g; bs += o.b;
                    if constexpr (PO) pk_put_luma<WOUT>(yo[dy], j, dx, ocf, rgb_to_y(K, o));
                    else word_put<WOUT>(yo[dy], 2 * j + dx, rgb_to_y(K, o));
                }
            }
            if constexpr (PO) {
                pk_put_chroma<WOUT>(yo[0], j, ocf, ocsw, rgb_to_cb(K, rs, gs, bs), rgb_to_cr(K, rs, gs, bs));
            } else {
                word_put<WOUT>(co, j, rgb_to_cb(K, rs, gs, bs));
                word_put<WOUT>(co + CWO, j, rgb_to_cr(K, rs, gs, bs));
            }
            // Zero-instruction fence (k_yuv_vec's): keeps hipcc from hoisting the coordinates and taps of every group of the
            // thread to the top; with it the groups are emitted one after the other.
#pragma unroll
            for (int dy = 0; dy < BH; dy++) {
#pragma unroll
                for (int k = 0; k < RWI; k++) asm volatile("" : "+v"(in[dy][k]));
#pragma unroll
                for (int k = 0; k < LWO; k++) asm volatile("" : "+v"(yo[dy][k]));
            }
#pragma unroll
            for (int k = 0; k < 2 * CWO; k++) asm volatile("" : "+v"(co[k]));
        }
        if constexpr (PO) {
            // the container's alignment: one shift per packed word -- two codes below 2^depth cannot carry into each other
            if constexpr (WOUT) {
                const unsigned osh = (unsigned)A.oshift;
#pragma unroll
                for (int k = 0; k < RWO; k++) yo[0][k] <<= osh;
            }
            st_run<RWO>(P.d[0] + fr * P.dfs[0] + (long long)y0 * P.ds[0] + (long long)xu * (RWO * 4), yo[0]);
        } else {
#pragma unroll
            for (int dy = 0; dy < BH; dy++)
                st_words<YWO>(P.d[0] + fr * P.dfs[0] + (long long)(y0 + dy) * P.ds[0] + (long long)xu * (YWO * 4), yo[dy]);
            const long long r = (long long)(y0 >> OCSY);
            st_words<CWO>(P.d[1] + fr * P.dfs[1] + r * P.ds[1] + (long long)xu * (CWO * 4), co);
            st_words<CWO>(P.d[2] + fr * P.dfs[2] + r * P.ds[2] + (long long)xu * (CWO * 4), co + CWO);
        }
    }
}

// The vector kernels of this translation unit's container mix; the layout checks are the caller's (launch_yuv_stack_packed).
const char *LUTR_CAT(LUTR_CAT(launch_yuv_stack_pk_vec_w, LUTR_PKS_WI), LUTR_PKS_WO)(hipStream_t st, const LutConsts &L,
                                                                                    const LutConsts &L2, const StackConsts &S,
                                                                                    const YuvConsts &K, const PlaneSet &P,
                                                                                    const FrameGeom &G, const PkArgs &A, int ocsy,
                                                                                    bool tri, bool lds)
{
    constexpr int WI = LUTR_PKS_WI, WO = LUTR_PKS_WO;
    constexpr int PXT = vec_bytes<WI, WO>() / (WI ? 2 : 1);
    const long long units = (long long)(G.w / PXT) * (G.rows >> ocsy) * G.nframes;
    const dim3 grid = pks_grid("k_yuv_stack_pk_vec", units, lds), block(256);
    const size_t lds_bytes = pks_lds_bytes(S, lds);
#define PKS_CASE(PI, PO, Y, T) \
    if (A.ipk == PI && A.opk == PO && ocsy == Y && tri == (T != 0)) { \
        if (lds) hipLaunchKernelGGL((k_yuv_stack_pk_vec<WI, WO, PI, PO, Y, T != 0, true>), grid, block, lds_bytes, st, L, L2, S, K, P, G, A); \
        else hipLaunchKernelGGL((k_yuv_stack_pk_vec<WI, WO, PI, PO, Y, T != 0, false>), grid, block, 0, st, L, L2, S, K, P, G, A); \
        return lds ? "k_yuv_stack_pk_vec<" LUTR_STR(LUTR_PKS_WI) "," LUTR_STR(LUTR_PKS_WO) "," #PI "," #PO "," #Y "," #T ",1>" \
                   : "k_yuv_stack_pk_vec<" LUTR_STR(LUTR_PKS_WI) "," LUTR_STR(LUTR_PKS_WO) "," #PI "," #PO "," #Y "," #T ",0>"; \
    }
#define PKS_SIDES(PI, PO, Y) PKS_CASE(PI, PO, Y, 0) PKS_CASE(PI, PO, Y, 1)
    PKS_SIDES(1, 1, 0) PKS_SIDES(1, 0, 0) PKS_SIDES(0, 1, 0) PKS_SIDES(1, 0, 1)
#undef PKS_SIDES
#undef PKS_CASE
    return nullptr;
}

#elif defined(LUTR_VKS_WI)
// ================================================================= v210: vector kernel
// One v210 group a thread and row: six luma samples, three chroma pairs, 2^OCSY rows; the pairs are walked one after the other.
// WP: the planar side is 16 bit (ignored for v210 -> v210).  VI / VO: the source / destination is v210.  The source is always
// 4:2:2; OCSY = 1 is a planar 4:2:0 destination.
// k_yuv_v210_vec (lutr_v210.hip) gives a thread as many groups as make whole words on the planar side (2 at 16 bit, 4 at 8 bit:
// up to twelve pairs).  With the step walk as the middle that shape fails: hipcc stops unrolling the pair loop of the trilinear
// 4:2:0 instances, their word arrays go to scratch (80 / 144 bytes a lane), and forced through it lands at 178 VGPRs, two waves and
// about 100 KB of code a kernel.  So the v210 side still moves as whole groups of 16 bytes, and the planar side
// moves the six luma / three chroma codes of the group in the widest accesses their offset allows: 16-bit luma as three dwords
// (12 bytes a thread), 16-bit chroma and 8-bit luma as three 16-bit accesses, 8-bit chroma as three bytes.  Consecutive lanes
// still cover consecutive bytes of a row.  Every code of the thread is loaded before anything is stored.
template <int N>
__device__ __forceinline__ void ld_halves(uint32_t *c, const uint8_t *p)          // N 16-bit codes, one a register
{
#pragma unroll
    for (int k = 0; k < N; k++) c[k] = ((const uint16_t *)p)[k];
}

template <int N>
__device__ __forceinline__ void st_halves(uint8_t *p, const uint32_t *c)          // N registers as 16-bit stores
{
#pragma unroll
    for (int k = 0; k < N; k++) ((uint16_t *)p)[k] = (uint16_t)c[k];
}

template <int N>
__device__ __forceinline__ void st_bytes(uint8_t *p, const uint32_t *c)
{
#pragma unroll
    for (int k = 0; k < N; k++) p[k] = (uint8_t)c[k];
}

template <int WP, int VI, int VO, int OCSY, bool TRI, bool LDS>
__global__ __launch_bounds__(256) void k_yuv_stack_v210_vec(LutConsts L, LutConsts L2, StackConsts S, YuvConsts K, PlaneSet P,
                                                            FrameGeom G)
{
    static_assert(VI || VO, "planar on both sides is k_yuv_stack_vec");
    static_assert(!(VO && OCSY), "a v210 destination is 4:2:2");
    static_assert(VI || WP, "a planar source beside a v210 destination is 16 bit");
    constexpr int BH = 1 << OCSY;                                 // luma rows per thread
    constexpr int BS = WP ? 2 : 1;                                // bytes of a planar sample
    // a source row: v210 -- the group's four words; planar (16 bit) -- three luma words, then Cb0..2 and Cr0..2, one a register
    constexpr int RWI = VI ? 4 : 9;
    // a destination row: v210 -- the group's four words; planar -- the luma codes, one a register (the chroma codes: co)
    constexpr int LWO = VO ? 4 : 6;
    CdlConsts C{S.cdl_tab, S.stride, S.sat};
    const uint16_t *l1d = S.l1d_tab;
    if constexpr (LDS) {
        stack_stage_to(pks_lds, S);
        C.tab = (const float *)pks_lds;
        l1d = (const uint16_t *)(pks_lds + S.lds_cdl_words);
    }
    const unsigned uw = (unsigned)G.w / 6;
    const unsigned ub = (unsigned)G.rows >> OCSY;
    const unsigned total = uw * ub * (unsigned)G.nframes;
    for (unsigned u = blockIdx.x * 256u + threadIdx.x; u < total; u += gridDim.x * 256u) {
        const unsigned xu = u % uw, t = u / uw;
        const int y0 = ((G.row0 >> OCSY) + (int)(t % ub)) * BH;   // first luma row of the thread
        const long long fr = t / ub;

        uint32_t in[BH][RWI];
        uint32_t yo[BH][LWO], co[VO ? 1 : 6];                     // (co: a planar destination's Cb0..2, Cr0..2)
#pragma unroll
        for (int dy = 0; dy < BH; dy++) {
            const long long y = (long long)(y0 + dy);
            if constexpr (VI) {
                ld_words<4>(in[dy], P.s[0] + fr * P.sfs[0] + y * P.ss[0] + (long long)xu * 16);
            } else {
                ld_dwords<3>(in[dy], P.s[0] + fr * P.sfs[0] + y * P.ss[0] + (long long)xu * 12);
                ld_halves<3>(in[dy] + 3, P.s[1] + fr * P.sfs[1] + y * P.ss[1] + (long long)xu * 6);
                ld_halves<3>(in[dy] + 6, P.s[2] + fr * P.sfs[2] + y * P.ss[2] + (long long)xu * 6);
            }
#pragma unroll
            for (int k = 0; k < LWO; k++) yo[dy][k] = 0;
        }
#pragma unroll
        for (int k = 0; k < (VO ? 1 : 6); k++) co[k] = 0;

#pragma unroll
        for (int k = 0; k < 3; k++) {                              // pair of the group
            // the BH x 2 pixels of one chroma pair, in the order the planar stack holds its union block
            Rgb px[BH * 2];
#pragma unroll
            for (int dy = 0; dy < BH; dy++) {
                const float cbv = VI ? v2_get(in[dy][kV2BW[k]], kV2BO[k]) : (float)in[dy][3 + k];
                const float crv = VI ? v2_get(in[dy][kV2RW[k]], kV2RO[k]) : (float)in[dy][6 + k];
                const Chroma c = chroma_terms(K, cbv, crv);
#pragma unroll
                for (int dx = 0; dx < 2; dx++) {
                    const int l = 2 * k + dx;                      // luma sample of the group
                    const float yv = VI ? v2_get(in[dy][kV2YW[l]], kV2YO[l]) : word_sample<1>(in[dy], l);
                    px[dy * 2 + dx] = yuv_to_rgb(K, yv, c);
                }
            }
            stack_block<TRI>(S, C, l1d, L, L2, px);
            float rs = 0.f, gs = 0.f, bs = 0.f;
#pragma unroll
            for (int dy = 0; dy < BH; dy++) {
#pragma unroll
                for (int dx = 0; dx < 2; dx++) {
                    const int l = 2 * k + dx;
                    const Rgb o = px[dy * 2 + dx];
                    rs += o.r; gs += o.g; bs += o.b;
                    if constexpr (VO) v2_put(&yo[dy][kV2YW[l]], kV2YO[l], rgb_to_y(K, o));
                    else yo[dy][l] = (uint32_t)rgb_to_y(K, o);
                }
            }
            if constexpr (VO) {
                v2_put(&yo[0][kV2BW[k]], kV2BO[k], rgb_to_cb(K, rs, gs, bs));
                v2_put(&yo[0][kV2RW[k]], kV2RO[k], rgb_to_cr(K, rs, gs, bs));
            } else {
                co[k] = (uint32_t)rgb_to_cb(K, rs, gs, bs);
                co[3 + k] = (uint32_t)rgb_to_cr(K, rs, gs, bs);
            }
            // Zero-instruction fence (k_yuv_vec's): keeps hipcc from hoisting the coordinates and taps of every pair of the
            // thread to the top; with it the pairs are emitted one after the other.
#pragma unroll
            for (int dy = 0; dy < BH; dy++) {
#pragma unroll
                for (int i = 0; i < RWI; i++) asm volatile("" : "+v"(in[dy][i]));
#pragma unroll
                for (int i = 0; i < LWO; i++) asm volatile("" : "+v"(yo[dy][i]));
            }
#pragma unroll
            for (int i = 0; i < (VO ? 1 : 6); i++) asm volatile("" : "+v"(co[i]));
        }
        if constexpr (VO) {
            st_words<4>(P.d[0] + fr * P.dfs[0] + (long long)y0 * P.ds[0] + (long long)xu * 16, yo[0]);
        } else {
#pragma unroll
            for (int dy = 0; dy < BH; dy++) {
                uint8_t *row = P.d[0] + fr * P.dfs[0] + (long long)(y0 + dy) * P.ds[0] + (long long)xu * (6 * BS);
                if constexpr (WP) {
                    // two 16-bit codes a word: three dwords
                    const uint32_t w[3] = {yo[dy][0] | (yo[dy][1] << 16), yo[dy][2] | (yo[dy][3] << 16), yo[dy][4] | (yo[dy][5] << 16)};
                    st_dwords<3>(row, w);
                } else {
                    // two 8-bit codes a 16-bit store
                    const uint32_t w[3] = {yo[dy][0] | (yo[dy][1] << 8), yo[dy][2] | (yo[dy][3] << 8), yo[dy][4] | (yo[dy][5] << 8)};
                    st_halves<3>(row, w);
                }
            }
            const long long r = (long long)(y0 >> OCSY);
            uint8_t *rb = P.d[1] + fr * P.dfs[1] + r * P.ds[1] + (long long)xu * (3 * BS);
            uint8_t *rr = P.d[2] + fr * P.dfs[2] + r * P.ds[2] + (long long)xu * (3 * BS);
            if constexpr (WP) { st_halves<3>(rb, co); st_halves<3>(rr, co + 3); }
            else { st_bytes<3>(rb, co); st_bytes<3>(rr, co + 3); }
        }
    }
}

// The vector kernels of this translation unit's container mix; the layout checks are the caller's (launch_yuv_stack_v210).
const char *LUTR_CAT(LUTR_CAT(launch_yuv_stack_v210_vec_w, LUTR_VKS_WI), LUTR_VKS_WO)(hipStream_t st, const LutConsts &L,
                                                                                      const LutConsts &L2, const StackConsts &S,
                                                                                      const YuvConsts &K, const PlaneSet &P,
                                                                                      const FrameGeom &G, const V210Args &A, int ocsy,
                                                                                      bool tri, bool lds)
{
    constexpr int WP = LUTR_VKS_WO;                               // (w11: every planar side is 16 bit; w10: the planar destination is 8 bit)
    const long long units = (long long)(G.w / 6) * (G.rows >> ocsy) * G.nframes;
    const dim3 grid = pks_grid("k_yuv_stack_v210_vec", units, lds), block(256);
    const size_t lds_bytes = pks_lds_bytes(S, lds);
#define VKS_CASE(VI, VO, Y, T) \
    if (A.iv == VI && A.ov == VO && ocsy == Y && tri == (T != 0)) { \
        if (lds) hipLaunchKernelGGL((k_yuv_stack_v210_vec<WP, VI, VO, Y, T != 0, true>), grid, block, lds_bytes, st, L, L2, S, K, P, G); \
        else hipLaunchKernelGGL((k_yuv_stack_v210_vec<WP, VI, VO, Y, T != 0, false>), grid, block, 0, st, L, L2, S, K, P, G); \
        return lds ? "k_yuv_stack_v210_vec<" LUTR_STR(LUTR_VKS_WO) "," #VI "," #VO "," #Y "," #T ",1>" \
                   : "k_yuv_stack_v210_vec<" LUTR_STR(LUTR_VKS_WO) "," #VI "," #VO "," #Y "," #T ",0>"; \
    }
#define VKS_SIDES(VI, VO, Y) VKS_CASE(VI, VO, Y, 0) VKS_CASE(VI, VO, Y, 1)
    VKS_SIDES(1, 0, 0) VKS_SIDES(1, 0, 1)
#if LUTR_VKS_WO
    VKS_SIDES(1, 1, 0) VKS_SIDES(0, 1, 0)
#endif
#undef VKS_SIDES
#undef VKS_CASE
    return nullptr;
}

#else  // the generic kernels and the launchers
// the step list on one pixel, at run-time modes and with the tables read from global memory: stack_walk_rt's body (lutr_stack.hip)
// without the matrix steps, which no list of these entries holds
__device__ __forceinline__ Rgb pks_walk_rt(const LutConsts &L, const GFetch &f, const LutConsts &L2, const GFetch &f2,
                                           const StackConsts &S, const CdlConsts &C, bool mix, const Rgb &q)
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
        default:                  o = lut3d_unit_rt(mode, L2, f2, o); break;
        }
    }
    return o;
}

// ================================================================= packed 4:2:2: generic kernel
// k_yuv_pk_generic's walk (lutr_pkyuv.hip) with the step list per pixel: one thread per union block, one group wide (two luma
// samples), 2^ocsy rows.  Any depth, stride (negative included) or alignment, odd sizes, all five modes on either lattice, and a
// planar 4:4:4 destination besides 4:2:2 and 4:2:0.  A pixel outside the frame is the edge pixel again, and the second luma sample
// of an odd-width packed row comes out as a copy of the last real one.  The block's codes are all read before anything is stored.
__global__ __launch_bounds__(256) void k_yuv_stack_pk_generic(LutConsts L, LutConsts L2, StackConsts S, YuvConsts K, PlaneSet P,
                                                              FrameGeom G, PkArgs A, int win, int wout, int ocsx, int ocsy)
{
    const GFetch f(L), f2(L2);
    const CdlConsts C{S.cdl_tab, S.stride, S.sat};
    const bool mix = S.sat != 1.0f;
    const int bh = 1 << ocsy;
    const int cwo = (G.w + (1 << ocsx) - 1) >> ocsx, cho = (G.h + bh - 1) >> ocsy;
    const int wl = A.opk ? ((G.w + 1) >> 1) * 2 : G.w;            // luma samples a destination row holds
    // elements of a group's Cb and Cr inside a packed row
    const int icb = (1 - A.icf) + 2 * A.icsw, icr = (1 - A.icf) + 2 * (1 - A.icsw);
    const int ocb = (1 - A.ocf) + 2 * A.ocsw, ocr = (1 - A.ocf) + 2 * (1 - A.ocsw);
    for_each_block(G, 1, ocsy, false, [&](long long fr, int gx, int uy) {
        // (loops of constant length with a guard, so that the block's codes stay in registers)
        float yv[2][2], cbv[2], crv[2];
#pragma unroll
        for (int dy = 0; dy < 2; dy++) {
            if (dy < bh) {
                const int yy = uy * bh + dy, y = yy < G.h ? yy : G.h - 1;
                const uint8_t *row = src_row(P, 0, fr, (long long)y);
#pragma unroll
                for (int dx = 0; dx < 2; dx++) {
                    const int xx = gx * 2 + dx, x = xx < G.w ? xx : G.w - 1;
                    yv[dy][dx] = A.ipk ? ld_code(row, 2ll * x + A.icf, win, A.ishift) : ld_code(row, x, win, 0);
                }
                cbv[dy] = A.ipk ? ld_code(row, 4ll * gx + icb, win, A.ishift) : ld_code(src_row(P, 1, fr, (long long)y), gx, win, 0);
                crv[dy] = A.ipk ? ld_code(row, 4ll * gx + icr, win, A.ishift) : ld_code(src_row(P, 2, fr, (long long)y), gx, win, 0);
            }
        }
        // the output chroma block is the whole union block, or (4:4:4) each of its two pixels
        float rs = 0.f, gs = 0.f, bs = 0.f;
#pragma unroll
        for (int dy = 0; dy < 2; dy++) {
            if (dy < bh) {
                const int yy = uy * bh + dy;
                uint8_t *row = dst_row(P, 0, fr, (long long)(yy < G.h ? yy : G.h - 1));
                const Chroma c = chroma_terms(K, cbv[dy], crv[dy]);
#pragma unroll
                for (int dx = 0; dx < 2; dx++) {
                    const int xx = gx * 2 + dx;
                    const Rgb o = pks_walk_rt(L, f, L2, f2, S, C, mix, yuv_to_rgb(K, yv[dy][dx], c));
                    if (yy < G.h && xx < wl) {
                        if (A.opk) st_code(row, 2ll * xx + A.ocf, wout, A.oshift, rgb_to_y(K, o));
                        else st_code(row, xx, wout, 0, rgb_to_y(K, o));
                    }
                    if (ocsx) {
                        rs += o.r; gs += o.g; bs += o.b;
                    } else if (xx < cwo && uy < cho) {
                        st_code(dst_row(P, 1, fr, (long long)uy), xx, wout, 0, rgb_to_cb(K, 0.f + o.r, 0.f + o.g, 0.f + o.b));
                        st_code(dst_row(P, 2, fr, (long long)uy), xx, wout, 0, rgb_to_cr(K, 0.f + o.r, 0.f + o.g, 0.f + o.b));
                    }
                }
            }
        }
        if (ocsx && gx < cwo && uy < cho) {
            if (A.opk) {                                           // (4:2:2: the group's own row)
                uint8_t *row = dst_row(P, 0, fr, (long long)uy);
                st_code(row, 4ll * gx + ocb, wout, A.oshift, rgb_to_cb(K, rs, gs, bs));
                st_code(row, 4ll * gx + ocr, wout, A.oshift, rgb_to_cr(K, rs, gs, bs));
            } else {
                st_code(dst_row(P, 1, fr, (long long)uy), gx, wout, 0, rgb_to_cb(K, rs, gs, bs));
                st_code(dst_row(P, 2, fr, (long long)uy), gx, wout, 0, rgb_to_cr(K, rs, gs, bs));
            }
        }
    });
}

// ================================================================= v210: generic kernel
// k_yuv_v210_generic's walk (lutr_v210.hip) with the step list per pixel: one thread per group and union block, six luma samples
// (three pairs) wide, 2^ocsy rows high.  Any stride (negative included), any planar depth 8..16 and alignment, odd sizes and the
// partial last group, all five modes on either lattice, and a planar 4:4:4 destination besides 4:2:2 and 4:2:0.  On a v210
// destination a luma slot beyond the frame repeats the last real luma sample of the row and a pair beyond it the last real pair.
// The thread's codes are all read before anything is stored.
__global__ __launch_bounds__(256) void k_yuv_stack_v210_generic(LutConsts L, LutConsts L2, StackConsts S, YuvConsts K, PlaneSet P,
                                                                FrameGeom G, V210Args A, int wp_in, int wp_out, int ocsx, int ocsy)
{
    const GFetch f(L), f2(L2);
    const CdlConsts C{S.cdl_tab, S.stride, S.sat};
    const bool mix = S.sat != 1.0f;
    const int bh = 1 << ocsy;
    const int cwi = (G.w + 1) >> 1;                               // chroma pairs of a source row
    const int cwo = (G.w + (1 << ocsx) - 1) >> ocsx, cho = (G.h + bh - 1) >> ocsy;
    const int gw = (G.w + 5) / 6;
    const int cr0 = G.row0 >> ocsy;
    const int crows = ((G.row0 + G.rows + bh - 1) >> ocsy) - cr0;
    const long long total = (long long)gw * crows * G.nframes;
    for (long long u = blockIdx.x * 256ll + threadIdx.x; u < total; u += (long long)gridDim.x * 256ll) {
        const long long t = u / gw, fr = t / crows;
        const int gx = (int)(u % gw), uy = cr0 + (int)(t % crows);
        // (loops of constant length with a guard, so that the thread's codes stay in registers)
        float yv[2][6], cbv[2][3], crv[2][3];
#pragma unroll
        for (int dy = 0; dy < 2; dy++) {
            if (dy < bh) {
                const int yy = uy * bh + dy, y = yy < G.h ? yy : G.h - 1;
                const uint8_t *row = src_row(P, 0, fr, (long long)y);
                if (A.iv) {
                    uint32_t w[4];
#pragma unroll
                    for (int i = 0; i < 4; i++) w[i] = ((const uint32_t *)row)[4ll * gx + i];
                    // a slot beyond the frame is ignored: the last real sample again (slot 0 of a group is always real)
#pragma unroll
                    for (int l = 0; l < 6; l++)
                        yv[dy][l] = (l > 0 && gx * 6 + l >= G.w) ? yv[dy][l > 0 ? l - 1 : 0] : v2_get(w[kV2YW[l]], kV2YO[l]);
#pragma unroll
                    for (int k = 0; k < 3; k++) {
                        const bool out = k > 0 && gx * 3 + k >= cwi;
                        cbv[dy][k] = out ? cbv[dy][k > 0 ? k - 1 : 0] : v2_get(w[kV2BW[k]], kV2BO[k]);
                        crv[dy][k] = out ? crv[dy][k > 0 ? k - 1 : 0] : v2_get(w[kV2RW[k]], kV2RO[k]);
                    }
                } else {
                    const uint8_t *rb = src_row(P, 1, fr, (long long)y), *rr = src_row(P, 2, fr, (long long)y);
#pragma unroll
                    for (int l = 0; l < 6; l++) {
                        const int xx = gx * 6 + l;
                        yv[dy][l] = ld_sample(row, xx < G.w ? xx : G.w - 1, wp_in);
                    }
#pragma unroll
                    for (int k = 0; k < 3; k++) {
                        const int pp = gx * 3 + k, p = pp < cwi ? pp : cwi - 1;
                        cbv[dy][k] = ld_sample(rb, p, wp_in);
                        crv[dy][k] = ld_sample(rr, p, wp_in);
                    }
                }
            }
        }
        // the codes of a v210 destination's group (ocsy = 0: one row)
        // (the pair loop stays a loop: three pairs x four step walks at five modes is more code than the compiler unrolls; it
        // indexes the thread's codes without scratch)
        float yq[6], bq[3], rq[3];
#pragma nounroll
        for (int k = 0; k < 3; k++) {
            const int px = gx * 3 + k;                             // pair of the row
            // the output chroma block is the pair over the union block's rows, or (4:4:4) each of its pixels
            float rs = 0.f, gs = 0.f, bs = 0.f;
#pragma unroll
            for (int dy = 0; dy < 2; dy++) {
                if (dy < bh) {
                    const int yy = uy * bh + dy;
                    const Chroma c = chroma_terms(K, cbv[dy][k], crv[dy][k]);
#pragma unroll
                    for (int dx = 0; dx < 2; dx++) {
                        const int xx = px * 2 + dx;
                        const Rgb o = pks_walk_rt(L, f, L2, f2, S, C, mix, yuv_to_rgb(K, yv[dy][2 * k + dx], c));
                        const float yo = rgb_to_y(K, o);
                        if (A.ov) yq[2 * k + dx] = yo;
                        else if (yy < G.h && xx < G.w) st_sample(dst_row(P, 0, fr, (long long)yy), xx, wp_out, yo);
                        if (ocsx) {
                            rs += o.r; gs += o.g; bs += o.b;
                        } else if (xx < cwo && uy < cho) {
                            st_sample(dst_row(P, 1, fr, (long long)uy), xx, wp_out, rgb_to_cb(K, 0.f + o.r, 0.f + o.g, 0.f + o.b));
                            st_sample(dst_row(P, 2, fr, (long long)uy), xx, wp_out, rgb_to_cr(K, 0.f + o.r, 0.f + o.g, 0.f + o.b));
                        }
                    }
                }
            }
            if (A.ov) {
                bq[k] = rgb_to_cb(K, rs, gs, bs);
                rq[k] = rgb_to_cr(K, rs, gs, bs);
            } else if (ocsx && px < cwo && uy < cho) {
                st_sample(dst_row(P, 1, fr, (long long)uy), px, wp_out, rgb_to_cb(K, rs, gs, bs));
                st_sample(dst_row(P, 2, fr, (long long)uy), px, wp_out, rgb_to_cr(K, rs, gs, bs));
            }
        }
        if (A.ov && uy < G.h) {
            uint32_t w[4] = {0u, 0u, 0u, 0u};
#pragma unroll
            for (int l = 0; l < 6; l++) {
                if (l > 0 && gx * 6 + l >= G.w) yq[l] = yq[l > 0 ? l - 1 : 0];
                v2_put(&w[kV2YW[l]], kV2YO[l], yq[l]);
            }
#pragma unroll
            for (int k = 0; k < 3; k++) {
                if (k > 0 && gx * 3 + k >= cwi) { bq[k] = bq[k > 0 ? k - 1 : 0]; rq[k] = rq[k > 0 ? k - 1 : 0]; }
                v2_put(&w[kV2BW[k]], kV2BO[k], bq[k]);
                v2_put(&w[kV2RW[k]], kV2RO[k], rq[k]);
            }
            uint32_t *row = (uint32_t *)dst_row(P, 0, fr, (long long)uy) + 4ll * gx;
#pragma unroll
            for (int i = 0; i < 4; i++) row[i] = w[i];
        }
    }
}

// ================================================================= launchers
// (where the vector kernels read the CDL and 1D tables: stack_in_lds, lutr_launch.h; the default is launch_yuv_stack's)
constexpr bool kPkStackLdsDefault = true;

// the lattice steps' modes: the vector kernels have nearest / trilinear / tetrahedral; *tri: some lattice step is trilinear
static bool pks_vec_modes(const StackConsts &S, bool *tri)
{
    bool ok = true;
    *tri = false;
    for (unsigned long long ops = S.ops; ops & 0xffull; ops >>= 8) {
        const int op = (int)(ops & 15u), mode = (int)((ops >> 4) & 15u);
        if (op == STACK_OP_L1D || op == STACK_OP_CDL || op == STACK_OP_ROUND) continue;
        ok = ok && vec_mode(mode);
        *tri = *tri || mode == LUTR_INTERP_TRILINEAR;
    }
    return ok;
}

// launch_vec_or_generic with launch_union's name for a ragged width: "<vector kernel>+<generic kernel>"
template <class Fits, class Vec, class Generic, class Tail>
static const char *pks_launch(int variant, const PlaneSet &P, const FrameGeom &G, int unit_px, Fits vec_fits, Vec vec, Generic generic,
                              Tail tail, const char *generic_name)
{
    int ran = 0;                                 // bit 0: a vector kernel was launched, bit 1: the generic one
    const char *name = launch_vec_or_generic(
        variant, P, G, unit_px, vec_fits, [&](const PlaneSet &Q, const FrameGeom &H) { ran |= 1; return vec(Q, H); },
        [&](const PlaneSet &Q, const FrameGeom &H) { ran |= 2; return generic(Q, H); }, tail);
    if (!name || ran != 3) return name;
    static thread_local std::string both;
    both = std::string(name) + "+" + generic_name;
    return both.c_str();
}

// launch_yuv_packed's routing (lutr_pkyuv.hip) for the stack kernels
const char *launch_yuv_stack_packed(hipStream_t st, int variant, const LutConsts &L, const LutConsts &L2, const StackConsts &S,
                                    const YuvConsts &K, const PlaneSet &P, const FrameGeom &G, const PkArgs &A, int din, int dout,
                                    int ocsx, int ocsy)
{
    const int win = din > 8, wout = dout > 8;
    const int bh = 1 << ocsy;
    bool tri = false;
    const bool modes_ok = pks_vec_modes(S, &tri);
    const bool lds = stack_in_lds(S, kPkStackLdsDefault);
    // the vector kernels' unit: 8 luma samples per row, 4 for 16 -> 16 bit; 8 -> 16 bit has none, nor has a 4:4:4 destination
    const bool mix_ok = (win == wout || (win && !wout)) && ocsx == 1 && (A.ipk || A.opk) && !(A.opk && ocsy);
    const int pxt = (win && !wout) ? 8 : (win ? 4 : 8);
    const long long bsi = win ? 2 : 1, bso = wout ? 2 : 1;
    const bool batch = G.nframes > 1;
    // a packed row moves in runs of 16 bytes (2 pxt samples; two runs for the 16-bit side of 16 -> 8), a planar luma row pxt
    // samples and a planar chroma row pxt / 2 per access
    auto run = [](long long bytes) { return bytes > 16 ? 16ll : bytes; };
    auto vec_fits = [&](const PlaneSet &Q, const FrameGeom &H) {
        if (!mix_ok || !modes_ok) return false;
        if (H.w % pxt || H.row0 % bh || H.rows % bh) return false;
        if (!units_fit((long long)(H.w / pxt) * (H.rows / bh) * H.nframes)) return false;
        if (!plane_ok(Q.s[0], Q.ss[0], Q.sfs[0], A.ipk ? run(2 * pxt * bsi) : pxt * bsi, batch, kStrideAny, false) ||
            !plane_ok(Q.d[0], Q.ds[0], Q.dfs[0], A.opk ? run(2 * pxt * bso) : pxt * bso, batch, kStrideAny, false))
            return false;
        for (int c = 1; c < 3; c++)
            if ((!A.ipk && !plane_ok(Q.s[c], Q.ss[c], Q.sfs[c], (pxt >> 1) * bsi, batch, kStrideAny, false)) ||
                (!A.opk && !plane_ok(Q.d[c], Q.ds[c], Q.dfs[c], (pxt >> 1) * bso, batch, kStrideAny, false)))
                return false;
        return true;
    };
    auto vec = [&](const PlaneSet &Q, const FrameGeom &H) -> const char * {
        if (win && wout) return launch_yuv_stack_pk_vec_w11(st, L, L2, S, K, Q, H, A, ocsy, tri, lds);
        if (win) return launch_yuv_stack_pk_vec_w10(st, L, L2, S, K, Q, H, A, ocsy, tri, lds);
        return launch_yuv_stack_pk_vec_w00(st, L, L2, S, K, Q, H, A, ocsy, tri, lds);
    };
    const char *const generic_name = "k_yuv_stack_pk_generic";
    auto generic = [&](const PlaneSet &Q, const FrameGeom &H) {
        hipLaunchKernelGGL(k_yuv_stack_pk_generic, dim3(block_grid(generic_name, H.w, H.rows, H.nframes, 1, ocsy)), dim3(256), 0, st,
                           L, L2, S, K, Q, H, A, win, wout, ocsx, ocsy);
        return generic_name;
    };
    return pks_launch(variant, P, G, pxt, vec_fits, vec, generic, [&](int wv) {
        return advance_planes(P, (A.ipk ? 2 * wv : wv) * bsi, (wv >> 1) * bsi, (A.opk ? 2 * wv : wv) * bso, (wv >> ocsx) * bso);
    }, generic_name);
}

// launch_yuv_v210's routing (lutr_v210.hip) for the stack kernels
const char *launch_yuv_stack_v210(hipStream_t st, int variant, const LutConsts &L, const LutConsts &L2, const StackConsts &S,
                                  const YuvConsts &K, const PlaneSet &P, const FrameGeom &G, const V210Args &A, int din, int dout,
                                  int ocsx, int ocsy)
{
    const int wp_in = din > 8, wp_out = dout > 8;
    const int bh = 1 << ocsy;
    bool tri = false;
    const bool modes_ok = pks_vec_modes(S, &tri);
    const bool lds = stack_in_lds(S, kPkStackLdsDefault);
    // the planar side's container decides the mix: v210 -> v210, a 16-bit planar side either way, an 8-bit planar destination; an
    // 8-bit planar source and a 4:4:4 destination have no vector kernel
    const bool both = A.iv && A.ov;
    const int wp = both ? 1 : (A.iv ? wp_out : wp_in);
    const bool mix_ok = ocsx == 1 && !(A.ov && ocsy) && (both || wp || A.iv);
    const int pxt = 6;                           // one group a thread, whatever the planar side
    const long long bs = wp ? 2 : 1;
    const bool batch = G.nframes > 1;
    auto vec_fits = [&](const PlaneSet &Q, const FrameGeom &H) {
        if (!mix_ok || !modes_ok) return false;
        if (H.w % pxt || H.row0 % bh || H.rows % bh) return false;
        if (!units_fit((long long)(H.w / pxt) * (H.rows / bh) * H.nframes)) return false;
        // a v210 plane moves in runs of 16 bytes; a planar luma plane in dwords at 16 bit and 16-bit accesses at 8 bit, a planar
        // chroma plane sample by sample
        if (!plane_ok(Q.s[0], Q.ss[0], Q.sfs[0], A.iv ? 16 : 4, batch, kStrideAny, false) ||
            !plane_ok(Q.d[0], Q.ds[0], Q.dfs[0], A.ov ? 16 : 2 * bs, batch, kStrideAny, false))
            return false;
        for (int c = 1; c < 3; c++)
            if ((!A.iv && !plane_ok(Q.s[c], Q.ss[c], Q.sfs[c], 2, batch, kStrideAny, false)) ||
                (!A.ov && !plane_ok(Q.d[c], Q.ds[c], Q.dfs[c], bs, batch, kStrideAny, false)))
                return false;
        return true;
    };
    auto vec = [&](const PlaneSet &Q, const FrameGeom &H) -> const char * {
        return wp ? launch_yuv_stack_v210_vec_w11(st, L, L2, S, K, Q, H, A, ocsy, tri, lds)
                  : launch_yuv_stack_v210_vec_w10(st, L, L2, S, K, Q, H, A, ocsy, tri, lds);
    };
    const char *const generic_name = "k_yuv_stack_v210_generic";
    auto generic = [&](const PlaneSet &Q, const FrameGeom &H) {
        const long long units = ((long long)H.w + 5) / 6 * blocks(H.rows, ocsy) * H.nframes;
        hipLaunchKernelGGL(k_yuv_stack_v210_generic, dim3(stride_grid(generic_name, units, kGridStrideCap)), dim3(256), 0, st, L, L2, S,
                           K, Q, H, A, wp_in, wp_out, ocsx, ocsy);
        return generic_name;
    };
    return pks_launch(variant, P, G, pxt, vec_fits, vec, generic, [&](int wv) {
        return advance_planes(P, A.iv ? wv / 6 * 16ll : wv * bs, (wv >> 1) * bs, A.ov ? wv / 6 * 16ll : wv * bs, (wv >> ocsx) * bs);
    }, generic_name);
}
#endif

}  // namespace lutr
