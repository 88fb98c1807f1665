// lutr_y2rstack.hip -- gfx950 kernels of the fused stage stack from YUV sources into RGB frames.
//
// What they compute: a planar YUV source, read as lutr_yuv2rgb.hip reads it -- each chroma sample replicated over its INPUT block,
// YUV -> integer RGB codes at the destination's depth through chroma_terms / yuv_to_rgb -- walks the step list of 3.21 / 3.25
// through stack_block / the per-pixel step loop, and the list's final codes are stored as they are, as lutr_yuv2rgb.hip stores
// them: three gbrp planes, or one packed image whose fourth component, if any, is written K.max_l (opaque).  yuv_to_rgb clips
// to [0, max_l], so the codes enter the list as lutr_rgbstack.hip's source codes do.  There is no RGB -> YUV stage and no chroma
// mean.  This family is new, so the matrix is an ordinary argument of every kernel: a list without a matrix stage has no matrix step.
//
// One source, two kinds of translation unit (Makefile MIX_RULE), like lutr_rgbstack.hip:
//   without LUTR_YRS_WI   the generic kernel and the launcher
//   LUTR_YRS_WI / _WO     the vector kernels of one container mix (8 -> 8, 16 -> 16, 16 -> 8): 3 layouts x 3 destination kinds x
//                         (any stage trilinear) x 2 table placements
#define LUTR_SK_MTX 1
#define SK_MTX_PARAM , const MtxConsts &X

#include "lutr_device.h"
#include "lutr_launch.h"
#include "lutr_stack_steps.h"

namespace lutr {

#ifdef LUTR_YRS_WI
// ================================================================= vector kernel

extern __shared__ uint32_t yrs_lds[];                             // the staged tables: the CDL's floats, then the 1D table's uint16

// k_yuv2rgb_vec's input side (whole-dword loads, 8 luma samples per thread and row, 2^ICSY rows, chroma_terms once per input
// chroma sample) and output side (y2r_put and the stores; NC = 1 three planes | 3 | 4 one packed image), k_rgb_stack_vec's walk
// and table staging (a grid stride; no thread leaves before the barrier), and stack_block on the input block's 1, 2 or 4 pixels.
template <int WIN, int ICSX, int ICSY, int NC, int WOUT, bool TRI, bool LDS>
__global__ __launch_bounds__(256) void k_yuv2rgb_stack_vec(LutConsts L, LutConsts L2, StackConsts S, MtxConsts X, YuvConsts K, PlaneSet P,
                                                           FrameGeom G, RgbLayout Y)
{
    constexpr int PXT = 8;                                        // luma samples per thread per row
    constexpr int YWI = PXT * (WIN ? 2 : 1) / 4;                  // luma words in per thread per row
    constexpr int CWI = (PXT >> ICSX) * (WIN ? 2 : 1) / 4;        // chroma words in per thread
    constexpr int BW = 1 << ICSX, BH = 1 << ICSY;                 // the input chroma block
    constexpr int NB = PXT / BW;                                  // blocks per thread
    constexpr int SWO = PXT * (WOUT ? 2 : 1) / 4;                 // dwords of 8 samples of one component out
    constexpr int NWO = (NC == 1 ? 3 : NC) * SWO;                 // destination dwords per thread per row
    static_assert(NB >= 1 && CWI >= 1 && YWI >= 1 && SWO >= 1, "a thread must own whole words");
    CdlConsts C{S.cdl_tab, S.stride, S.sat};
    const uint16_t *l1d = S.l1d_tab;
    if constexpr (LDS) {
        stack_stage_to(yrs_lds, S);
        C.tab = (const float *)yrs_lds;
        l1d = (const uint16_t *)(yrs_lds + S.lds_cdl_words);
    }
    const unsigned uw = (unsigned)G.w / PXT;
    const unsigned ub = (unsigned)G.rows >> ICSY;
    const unsigned total = uw * ub * (unsigned)G.nframes;
    const uint32_t amax = (uint32_t)K.max_l;                      // the fourth component of a packed destination: opaque
    for (unsigned u = blockIdx.x * 256u + threadIdx.x; u < total; u += gridDim.x * 256u) {
        const unsigned xu = u % uw, t = u / uw;
        const int y0 = ((G.row0 >> ICSY) + (int)(t % ub)) * BH;   // first luma row of the thread
        const long long fr = t / ub;

        uint32_t yw[BH][YWI], cbw[CWI], crw[CWI];
        uint32_t out[BH][NWO];
#pragma unroll
        for (int dy = 0; dy < BH; dy++) {
            ld_words<YWI>(yw[dy], P.s[0] + fr * P.sfs[0] + (long long)(y0 + dy) * P.ss[0] + (long long)xu * (YWI * 4));
#pragma unroll
            for (int k = 0; k < NWO; k++) out[dy][k] = 0;
        }
        {
            const long long r = (long long)(y0 >> ICSY), cx = (long long)xu * (CWI * 4);
            ld_words<CWI>(cbw, P.s[1] + fr * P.sfs[1] + r * P.ss[1] + cx);
            ld_words<CWI>(crw, P.s[2] + fr * P.sfs[2] + r * P.ss[2] + cx);
        }

#pragma unroll
        for (int j = 0; j < NB; j++) {
            const Chroma c = chroma_terms(K, word_sample<WIN>(cbw, j), word_sample<WIN>(crw, j));
            Rgb px[BH * BW];
#pragma unroll
            for (int dy = 0; dy < BH; dy++)
#pragma unroll
                for (int dx = 0; dx < BW; dx++)
                    px[dy * BW + dx] = yuv_to_rgb(K, word_sample<WIN>(yw[dy], j * BW + dx), c);
            stack_block<TRI>(S, C, l1d, L, L2, px, X);
#pragma unroll
            for (int dy = 0; dy < BH; dy++)
#pragma unroll
                for (int dx = 0; dx < BW; dx++)
                    y2r_put<WOUT, NC>(out[dy], j * BW + dx, px[dy * BW + dx], Y, amax);
            // Zero-instruction fence (k_yuv_vec's): keeps hipcc from hoisting the coordinates and taps of every block of the
            // thread to the top; with it the blocks are emitted one after the other.
#pragma unroll
            for (int dy = 0; dy < BH; dy++) {
#pragma unroll
                for (int k = 0; k < YWI; k++) asm volatile("" : "+v"(yw[dy][k]));
#pragma unroll
                for (int k = 0; k < NWO; k++) asm volatile("" : "+v"(out[dy][k]));
            }
#pragma unroll
            for (int k = 0; k < CWI; k++) asm volatile("" : "+v"(cbw[k]), "+v"(crw[k]));
        }
#pragma unroll
        for (int dy = 0; dy < BH; dy++) {
            if constexpr (NC == 1) {
#pragma unroll
                for (int k = 0; k < 3; k++)
                    st_words<SWO>(P.d[k] + fr * P.dfs[k] + (long long)(y0 + dy) * P.ds[k] + (long long)xu * (SWO * 4), out[dy] + k * SWO);
            } else {
                uint32_t *dp = (uint32_t *)(P.d[0] + fr * P.dfs[0] + (long long)(y0 + dy) * P.ds[0]) + (size_t)xu * NWO;
#pragma unroll
                for (int k = 0; k < NWO; k++) dp[k] = out[dy][k];
            }
        }
    }
}

// The vector kernels of this translation unit's container mix; the layout checks are the caller's (launch_yuv2rgb_stack).  The
// grid: with tables in LDS, eight workgroups a CU, each staging once and walking its share of the units; without, the usual cap.
const char *LUTR_CAT(LUTR_CAT(launch_yuv2rgb_stack_vec_w, LUTR_YRS_WI), LUTR_YRS_WO)(hipStream_t st, const LutConsts &L, const LutConsts &L2,
                                                                                     const StackConsts &S, const MtxConsts &X,
                                                                                     const YuvConsts &K, const PlaneSet &P,
                                                                                     const RgbLayout &Y, const FrameGeom &G, int icsx,
                                                                                     int icsy, bool tri, bool lds)
{
    constexpr int WI = LUTR_YRS_WI, WO = LUTR_YRS_WO;
    const long long units = (long long)(G.w / 8) * (G.rows >> icsy) * G.nframes;
    const dim3 grid(stride_grid("k_yuv2rgb_stack_vec", units, lds ? (unsigned)device_cus() * 8u : kGridStrideCap)), block(256);
    const size_t lds_bytes = lds ? (size_t)(S.lds_cdl_words + S.lds_l1d_words) * sizeof(uint32_t) : 0;
#define YRS_CASE(IX, IY, C, T) \
    if (icsx == IX && icsy == IY && Y.step == C && tri == (T != 0)) { \
        if (lds) hipLaunchKernelGGL((k_yuv2rgb_stack_vec<WI, IX, IY, C, WO, T != 0, true>), grid, block, lds_bytes, st, L, L2, S, X, K, P, G, Y); \
        else hipLaunchKernelGGL((k_yuv2rgb_stack_vec<WI, IX, IY, C, WO, T != 0, false>), grid, block, 0, st, L, L2, S, X, K, P, G, Y); \
        return lds ? "k_yuv2rgb_stack_vec<" LUTR_STR(LUTR_YRS_WI) "," #IX "," #IY "," #C "," LUTR_STR(LUTR_YRS_WO) "," #T ",1>" \
                   : "k_yuv2rgb_stack_vec<" LUTR_STR(LUTR_YRS_WI) "," #IX "," #IY "," #C "," LUTR_STR(LUTR_YRS_WO) "," #T ",0>"; \
    }
#define YRS_DST(IX, IY, C) YRS_CASE(IX, IY, C, 0) YRS_CASE(IX, IY, C, 1)
#define YRS_LAYOUT(IX, IY) YRS_DST(IX, IY, 1) YRS_DST(IX, IY, 3) YRS_DST(IX, IY, 4)
    YRS_LAYOUT(1, 1) YRS_LAYOUT(1, 0) YRS_LAYOUT(0, 0)
#undef YRS_LAYOUT
#undef YRS_DST
#undef YRS_CASE
    return nullptr;
}

#else  // !LUTR_YRS_WI
// ================================================================= generic kernel
// k_yuv2rgb_generic's walk -- one thread per input chroma block, xsub_union_block with a 4:4:4 "output layout" and RgbSink -- with
// the per-pixel step loop of k_rgb_stack_generic as the pixel functor: any depth pair, stride or alignment, odd sizes, all five
// modes.  Only pixels inside the frame are written.
__global__ __launch_bounds__(256) void k_yuv2rgb_stack_generic(LutConsts L, LutConsts L2, StackConsts S, MtxConsts X, YuvConsts K,
                                                               PlaneSet P, FrameGeom G, RgbLayout Y, int win, int icsx, int icsy)
{
    const GFetch f(L), f2(L2);
    RgbSink sink{P, Y, K.max_l};
    const CdlConsts C{S.cdl_tab, S.stride, S.sat};
    const bool mix = S.sat != 1.0f;
    for_each_block(G, icsx, icsy, false, [&](long long fr, int ux, int uy) {
        xsub_union_block(K, P, G, fr, ux, uy, win, icsx, icsy, 0, 0, sink, [&](long long, int, int, const Rgb &q) {
            return rsk_steps_px(L, L2, f, f2, S, C, X, mix, q);
        });
    });
}

// ================================================================= launcher
// Where the vector kernels read the tables when LUTR_STACK_LDS does not say (stack_in_lds, lutr_launch.h): LDS, the faster one on
// every natural row of 64 UHD frames where the tables fit -- [lut1d, cdl, lut3d] from yuv420p10le into gbrp10le takes 0.74 and from
// yuv420p into rgba 0.80 of the global-memory time, [cdl, lut3d] 0.85 and 0.86 (DESIGN.md 3.27 point 9).
constexpr bool kY2rStackLdsDefault = true;

const char *launch_yuv2rgb_stack(hipStream_t st, int variant, const LutConsts &L, const LutConsts &L2, const StackConsts &S,
                                 const MtxConsts &X, const YuvConsts &K, const PlaneSet &P, const RgbLayout &Y, const FrameGeom &G,
                                 int din, int icsx, int icsy)
{
    const int win = din > 8, wout = Y.wide;
    const int bh = 1 << icsy;
    // the vector kernels' unit: 8 luma samples per row; an 8-bit source written as 16 bit has none
    const bool mix_ok = win == wout || (win && !wout);
    const long long bsi = win ? 2 : 1, bso = wout ? 2 : 1;
    const bool batch = G.nframes > 1;
    // the 3-component vector body knows R G B and B G R order only
    const bool order_ok = Y.step != 3 || (Y.go == 1 && ((Y.ro == 0 && Y.bo == 2) || (Y.ro == 2 && Y.bo == 0)));
    const bool lds = stack_in_lds(S, kY2rStackLdsDefault);
    // the lattice steps' modes: the vector kernels have nearest / trilinear / tetrahedral
    bool modes_ok = true, tri = false;
    for (unsigned long long ops = S.ops; ops & 0xffull; ops >>= 8) {
        const int op = (int)(ops & 15u), mode = (int)((ops >> 4) & 15u);
        if (op == STACK_OP_L1D || op == STACK_OP_CDL || op == STACK_OP_ROUND || op == STACK_OP_MTX_CODES || op == STACK_OP_MTX_UNIT) continue;
        modes_ok = modes_ok && vec_mode(mode);
        tri = tri || mode == LUTR_INTERP_TRILINEAR;
    }
    auto vec_fits = [&](const PlaneSet &Q, const FrameGeom &H) {
        if (!mix_ok || !order_ok || !modes_ok) return false;
        if (H.w % 8 || H.row0 % bh || H.rows % bh) return false;
        if (!units_fit((long long)(H.w / 8) * (H.rows / bh) * H.nframes)) return false;
        if (!plane_ok(Q.s[0], Q.ss[0], Q.sfs[0], 8 * bsi, batch, kStrideAny, false)) return false;
        for (int c = 1; c < 3; c++)
            if (!plane_ok(Q.s[c], Q.ss[c], Q.sfs[c], (8 >> icsx) * bsi, batch, kStrideAny, false)) return false;
        if (Y.step == 1) {
            for (int c = 0; c < 3; c++)
                if (!plane_ok(Q.d[c], Q.ds[c], Q.dfs[c], 8 * bso, batch, kStrideAny, false)) return false;
        } else if (!plane_ok(Q.d[0], Q.ds[0], Q.dfs[0], 4, batch, kStrideAny, false)) {
            return false;
        }
        return true;
    };
    int ran = 0;                                         // bit 0: a vector kernel was launched, bit 1: the generic one
    auto vec = [&](const PlaneSet &Q, const FrameGeom &H) -> const char * {
        ran |= 1;
        if (win && wout) return launch_yuv2rgb_stack_vec_w11(st, L, L2, S, X, K, Q, Y, H, icsx, icsy, tri, lds);
        if (win) return launch_yuv2rgb_stack_vec_w10(st, L, L2, S, X, K, Q, Y, H, icsx, icsy, tri, lds);
        return launch_yuv2rgb_stack_vec_w00(st, L, L2, S, X, K, Q, Y, H, icsx, icsy, tri, lds);
    };
    auto generic = [&](const PlaneSet &Q, const FrameGeom &H) {
        ran |= 2;
        hipLaunchKernelGGL(k_yuv2rgb_stack_generic, dim3(block_grid("k_yuv2rgb_stack_generic", H.w, H.rows, H.nframes, icsx, icsy)),
                           dim3(256), 0, st, L, L2, S, X, K, Q, H, Y, win, icsx, icsy);
        return "k_yuv2rgb_stack_generic";
    };
    const char *name = launch_vec_or_generic(variant, P, G, 8, vec_fits, vec, generic, [&](int wv) {
        const long long db = (long long)wv * Y.step * bso;
        return advance_planes(P, wv * bsi, (wv >> icsx) * bsi, db, db);
    });
    if (!name || ran != 3) return name;
    // a ragged width: the vector kernel up to the last whole unit, the generic one for the rest (as launch_rgb_stack reports it)
    static thread_local std::string both;
    both = std::string(name) + "+k_yuv2rgb_stack_generic";
    return both.c_str();
}
#endif  // LUTR_YRS_WI

}  // namespace lutr
