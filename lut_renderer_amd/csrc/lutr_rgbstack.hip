// lutr_rgbstack.hip -- gfx950 kernels of the fused stage stack on RGB sources.
//
// What they compute: an RGB source -- three gbrp planes or one packed image, integer codes at the source's depth, read as
// lutr_rgb2yuv.hip reads them -- enters the step list of 3.21 / 3.25 as codes held as floats (a 16-bit word above M = 2^depth - 1
// acts as M), walks it through stack_block / the per-pixel step loop, and leaves through one of two sinks:
//   SINK_YUV   the output stage of 3.9: Y per pixel, each chroma sample from the sum of the list's final codes over its output
//              block, a partial block at an odd edge taking the edge column / row again
//   SINK_RGB   three planes at the source's depth, the final codes stored as they are (P.d in R, G, B order); a sample is read
//              and written by the same lane, so the planes may be the source's own
// This family is new, so the matrix is an ordinary argument of every kernel: a list without a matrix stage has no matrix step.
//
// One source, two kinds of translation unit (Makefile MIX_RULE), like lutr_rgb2yuv.hip:
//   without LUTR_RSK_WI   the generic kernel and the launcher
//   LUTR_RSK_WI / _WO     the vector kernels of one container mix (8 -> 8, 16 -> 16, 16 -> 8; the RGB sink where the two are
//                         equal): 3 source kinds x (3 layouts + the RGB sink) x (any stage trilinear) x 2 table placements
#define LUTR_SK_MTX 1
#define SK_MTX_PARAM , const MtxConsts &X

#include "lutr_device.h"
#include "lutr_launch.h"
#include "lutr_stack_steps.h"

namespace lutr {

// a source pixel as the list takes it: codes at most M (an 8-bit container cannot hold more)
template <int WIDE>
__device__ __forceinline__ Rgb rsk_enter(float maxf, const Rgb &q)
{
    if constexpr (WIDE) return Rgb{fminf(q.r, maxf), fminf(q.g, maxf), fminf(q.b, maxf)};
    else return q;
}

#ifdef LUTR_RSK_WI
// ================================================================= vector kernel

extern __shared__ uint32_t rsk_lds[];                             // the staged tables: the CDL's floats, then the 1D table's uint16

// stack_stage_tables of lutr_stack.hip on this family's LDS: every thread of the workgroup must arrive here
__device__ __forceinline__ void rsk_stage_tables(const StackConsts &S)
{
    stack_stage_to(rsk_lds, S);
}

// k_rgb2yuv_vec's input side (8 samples per thread and row, 2^OCSY rows, NC = 1 planar | 3 | 4 packed), k_yuv_stack_vec's walk
// and table staging (a grid stride; no thread leaves before the barrier), stack_block on the output block's 1, 2 or 4 pixels, and
// the sink: k_rgb2yuv_vec's YUV tail, or (SINK_RGB: OCSX = OCSY = 0, WOUT = WIN) three whole-word plane stores.
// o0 is Y | R, o1 / o2 are Cb, Cr | G, B.
template <int WIN, int NC, int WOUT, int SINK, int OCSX, int OCSY, bool TRI, bool LDS>
__global__ __launch_bounds__(256) void k_rgb_stack_vec(LutConsts L, LutConsts L2, StackConsts S, MtxConsts X, YuvConsts K, PlaneSet P,
                                                       FrameGeom G, RgbLayout Y)
{
    constexpr int PXT = 8;                                        // samples per thread per row
    constexpr int SW = PXT * (WIN ? 2 : 1) / 4;                   // dwords of 8 samples of one component
    constexpr int NWI = (NC == 1 ? 3 : NC) * SW;                  // source dwords per thread per row
    constexpr int YWO = PXT * (WOUT ? 2 : 1) / 4;                 // words out per thread per row of a full-size plane
    constexpr int BW = 1 << OCSX, BH = 1 << OCSY;                 // the output block
    constexpr int NB = PXT / BW;                                  // blocks per thread
    constexpr int CWO = SINK == SINK_RGB ? YWO : (PXT >> OCSX) * (WOUT ? 2 : 1) / 4;   // words out per thread of planes 1 and 2
    static_assert(NB >= 1 && CWO >= 1 && YWO >= 1, "a thread must own whole words");
    static_assert(SINK == SINK_YUV || (OCSX == 0 && OCSY == 0 && WIN == WOUT), "the RGB sink is full size at the source's depth");
    CdlConsts C{S.cdl_tab, S.stride, S.sat};
    const uint16_t *l1d = S.l1d_tab;
    if constexpr (LDS) {
        rsk_stage_tables(S);
        C.tab = (const float *)rsk_lds;
        l1d = (const uint16_t *)(rsk_lds + S.lds_cdl_words);
    }
    const unsigned uw = (unsigned)G.w / PXT;
    const unsigned ub = (unsigned)G.rows >> OCSY;
    const unsigned total = uw * ub * (unsigned)G.nframes;
    for (unsigned u = blockIdx.x * 256u + threadIdx.x; u < total; u += gridDim.x * 256u) {
        const unsigned xu = u % uw, t = u / uw;
        const int y0 = ((G.row0 >> OCSY) + (int)(t % ub)) * BH;   // first row of the thread
        const long long fr = t / ub;
        const long long xo = (long long)xu * (YWO * 4), cxo = (long long)xu * (CWO * 4);

        uint32_t in[BH][NWI];
        uint32_t o0[BH][YWO], o1[CWO], o2[CWO];
#pragma unroll
        for (int dy = 0; dy < BH; dy++) {
            if constexpr (NC == 1) {
#pragma unroll
                for (int k = 0; k < 3; k++)
                    ld_words<SW>(in[dy] + k * SW, P.s[k] + fr * P.sfs[k] + (long long)(y0 + dy) * P.ss[k] + (long long)xu * (SW * 4));
            } else {
                const uint32_t *sp = (const uint32_t *)(P.s[0] + fr * P.sfs[0] + (long long)(y0 + dy) * P.ss[0]) + (size_t)xu * NWI;
#pragma unroll
                for (int k = 0; k < NWI; k++) in[dy][k] = sp[k];
            }
#pragma unroll
            for (int k = 0; k < YWO; k++) o0[dy][k] = 0;
        }
#pragma unroll
        for (int k = 0; k < CWO; k++) { o1[k] = 0; o2[k] = 0; }

#pragma unroll
        for (int j = 0; j < NB; j++) {
            Rgb px[BH * BW];
#pragma unroll
            for (int dy = 0; dy < BH; dy++)
#pragma unroll
                for (int dx = 0; dx < BW; dx++)
                    px[dy * BW + dx] = rsk_enter<WIN>(S.maxf, r2y_pixel<WIN, NC>(in[dy], j * BW + dx, Y));
            stack_block<TRI>(S, C, l1d, L, L2, px, X);
            if constexpr (SINK == SINK_RGB) {
                word_put<WOUT>(o0[0], j, px[0].r);
                word_put<WOUT>(o1, j, px[0].g);
                word_put<WOUT>(o2, j, px[0].b);
            } else {
                float rs = 0.f, gs = 0.f, bs = 0.f;
#pragma unroll
                for (int dy = 0; dy < BH; dy++) {
#pragma unroll
                    for (int dx = 0; dx < BW; dx++) {
                        const Rgb o = px[dy * BW + dx];
                        rs += o.r; gs += o.g; bs += o.b;
                        word_put<WOUT>(o0[dy], j * BW + dx, rgb_to_y(K, o));
                    }
                }
                word_put<WOUT>(o1, j, rgb_to_cb(K, rs, gs, bs));
                word_put<WOUT>(o2, j, rgb_to_cr(K, rs, gs, bs));
            }
            // Zero-instruction fence (k_yuv_vec's): keeps hipcc from hoisting the coordinates and taps of every block of the
            // thread to the top; with it the blocks are emitted one after the other.
#pragma unroll
            for (int dy = 0; dy < BH; dy++) {
#pragma unroll
                for (int k = 0; k < NWI; k++) asm volatile("" : "+v"(in[dy][k]));
#pragma unroll
                for (int k = 0; k < YWO; k++) asm volatile("" : "+v"(o0[dy][k]));
            }
#pragma unroll
            for (int k = 0; k < CWO; k++) asm volatile("" : "+v"(o1[k]), "+v"(o2[k]));
        }
#pragma unroll
        for (int dy = 0; dy < BH; dy++)
            st_words<YWO>(P.d[0] + fr * P.dfs[0] + (long long)(y0 + dy) * P.ds[0] + xo, o0[dy]);
        const long long r = (long long)(y0 >> OCSY);
        st_words<CWO>(P.d[1] + fr * P.dfs[1] + r * P.ds[1] + cxo, o1);
        st_words<CWO>(P.d[2] + fr * P.dfs[2] + r * P.ds[2] + cxo, o2);
    }
}

// The vector kernels of this translation unit's container mix; the layout checks are the caller's (launch_rgb_stack).  The grid:
// with tables in LDS, eight workgroups a CU, each staging once and walking its share of the units; without, the usual cap.
const char *LUTR_CAT(LUTR_CAT(launch_rgb_stack_vec_w, LUTR_RSK_WI), LUTR_RSK_WO)(hipStream_t st, const LutConsts &L, const LutConsts &L2,
                                                                                 const StackConsts &S, const MtxConsts &X,
                                                                                 const YuvConsts &K, const PlaneSet &P,
                                                                                 const RgbLayout &Y, const FrameGeom &G, int sink,
                                                                                 int ocsx, int ocsy, bool tri, bool lds)
{
    constexpr int WI = LUTR_RSK_WI, WO = LUTR_RSK_WO;
    const long long units = (long long)(G.w / 8) * (G.rows >> ocsy) * G.nframes;
    const dim3 grid(stride_grid("k_rgb_stack_vec", units, lds ? (unsigned)device_cus() * 8u : kGridStrideCap)), block(256);
    const size_t lds_bytes = lds ? (size_t)(S.lds_cdl_words + S.lds_l1d_words) * sizeof(uint32_t) : 0;
#define RSK_CASE(C, SK, OX, OY, T) \
    if (Y.step == C && sink == SK && ocsx == OX && ocsy == OY && tri == (T != 0)) { \
        if (lds) hipLaunchKernelGGL((k_rgb_stack_vec<WI, C, WO, SK, OX, OY, T != 0, true>), grid, block, lds_bytes, st, L, L2, S, X, K, P, G, Y); \
        else hipLaunchKernelGGL((k_rgb_stack_vec<WI, C, WO, SK, OX, OY, T != 0, false>), grid, block, 0, st, L, L2, S, X, K, P, G, Y); \
        return lds ? "k_rgb_stack_vec<" LUTR_STR(LUTR_RSK_WI) "," #C "," LUTR_STR(LUTR_RSK_WO) "," #SK "," #OX "," #OY "," #T ",1>" \
                   : "k_rgb_stack_vec<" LUTR_STR(LUTR_RSK_WI) "," #C "," LUTR_STR(LUTR_RSK_WO) "," #SK "," #OX "," #OY "," #T ",0>"; \
    }
#define RSK_LAYOUT(C, SK, OX, OY) RSK_CASE(C, SK, OX, OY, 0) RSK_CASE(C, SK, OX, OY, 1)
#if LUTR_RSK_WI == LUTR_RSK_WO
#define RSK_SRC(C) RSK_LAYOUT(C, 0, 1, 1) RSK_LAYOUT(C, 0, 1, 0) RSK_LAYOUT(C, 0, 0, 0) RSK_LAYOUT(C, 1, 0, 0)
#else
#define RSK_SRC(C) RSK_LAYOUT(C, 0, 1, 1) RSK_LAYOUT(C, 0, 1, 0) RSK_LAYOUT(C, 0, 0, 0)
#endif
    RSK_SRC(1) RSK_SRC(3) RSK_SRC(4)
#undef RSK_SRC
#undef RSK_LAYOUT
#undef RSK_CASE
    return nullptr;
}

#else  // !LUTR_RSK_WI
// ================================================================= generic kernel
// One thread per output block (r2y_block's walk): any depth mix, stride or alignment, odd sizes, both sinks.  A pixel outside the
// frame is the edge pixel again; only pixels inside the planes are written.  The RGB sink's block is one pixel.
__global__ __launch_bounds__(256) void k_rgb_stack_generic(LutConsts L, LutConsts L2, StackConsts S, MtxConsts X, YuvConsts K, PlaneSet P,
                                                           FrameGeom G, RgbLayout Y, int wout, int sink, int ocsx, int ocsy)
{
    const GFetch f(L), f2(L2);
    PlaneSink yuv{K, P, wout};
    const CdlConsts C{S.cdl_tab, S.stride, S.sat};
    const bool mix = S.sat != 1.0f;
    for_each_block(G, ocsx, ocsy, false, [&](long long fr, int cx, int cy) {
        const int obw = 1 << ocsx, obh = 1 << ocsy;
        float rs = 0.f, gs = 0.f, bs = 0.f;
        for (int dy = 0; dy < obh; dy++) {
            const int yy = cy * obh + dy;
            const int y = yy < G.h ? yy : G.h - 1;
            for (int dx = 0; dx < obw; dx++) {
                const int xx = cx * obw + dx;
                const int x = xx < G.w ? xx : G.w - 1;
                const int e = x * Y.step;
                const Rgb q{fminf(ld_sample(src_row(P, 0, fr, y), e + Y.ro, Y.wide), S.maxf),
                            fminf(ld_sample(src_row(P, 1, fr, y), e + Y.go, Y.wide), S.maxf),
                            fminf(ld_sample(src_row(P, 2, fr, y), e + Y.bo, Y.wide), S.maxf)};
                const Rgb o = rsk_steps_px(L, L2, f, f2, S, C, X, mix, q);
                if (sink == SINK_RGB) {
                    st_sample(dst_row(P, 0, fr, y), x, wout, o.r);
                    st_sample(dst_row(P, 1, fr, y), x, wout, o.g);
                    st_sample(dst_row(P, 2, fr, y), x, wout, o.b);
                } else {
                    rs += o.r; gs += o.g; bs += o.b;
                    if (yy < G.h && xx < G.w) yuv.luma(fr, x, y, o);
                }
            }
        }
        if (sink != SINK_RGB) yuv.chroma(fr, cx, cy, rs, gs, bs);
    });
}

// ================================================================= launcher
// Where the vector kernels read the tables when LUTR_STACK_LDS does not say (stack_in_lds, lutr_launch.h): LDS, the faster one on
// every natural row of 64 UHD frames -- [lut1d, cdl, lut3d] from gbrp10le takes 0.76 (into YUV) and 0.84 (into gbrp) of the
// global-memory time (DESIGN.md 3.26 point 9).
constexpr bool kRgbStackLdsDefault = true;

const char *launch_rgb_stack(hipStream_t st, int variant, const LutConsts &L, const LutConsts &L2, const StackConsts &S,
                             const MtxConsts &X, const YuvConsts &K, const PlaneSet &P, const RgbLayout &Y, const FrameGeom &G,
                             int sink, int dout, int ocsx, int ocsy)
{
    const int win = Y.wide, wout = dout > 8;
    const int bh = 1 << ocsy;
    // the vector kernels' unit: 8 samples per row; an 8-bit source written as 16 bit has none, and the RGB sink keeps the container
    const bool mix_ok = win == wout || (win && !wout && sink == SINK_YUV);
    const long long bsi = win ? 2 : 1, bso = wout ? 2 : 1;
    const bool batch = G.nframes > 1;
    // the 3-component vector body knows R G B and B G R order only
    const bool order_ok = Y.step != 3 || (Y.go == 1 && ((Y.ro == 0 && Y.bo == 2) || (Y.ro == 2 && Y.bo == 0)));
    const bool lds = stack_in_lds(S, kRgbStackLdsDefault);
    // the lattice steps' modes: the vector kernels have nearest / trilinear / tetrahedral
    bool modes_ok = true, tri = false;
    for (unsigned long long ops = S.ops; ops & 0xffull; ops >>= 8) {
        const int op = (int)(ops & 15u), mode = (int)((ops >> 4) & 15u);
        if (op == STACK_OP_L1D || op == STACK_OP_CDL || op == STACK_OP_ROUND || op == STACK_OP_MTX_CODES || op == STACK_OP_MTX_UNIT) continue;
        modes_ok = modes_ok && vec_mode(mode);
        tri = tri || mode == LUTR_INTERP_TRILINEAR;
    }
    const int dcsx = sink == SINK_RGB ? 0 : ocsx;        // planes 1 and 2 of the destination: full size for the RGB sink
    auto vec_fits = [&](const PlaneSet &Q, const FrameGeom &H) {
        if (!mix_ok || !order_ok || !modes_ok) return false;
        if (H.w % 8 || H.row0 % bh || H.rows % bh) return false;
        if (!units_fit((long long)(H.w / 8) * (H.rows / bh) * H.nframes)) return false;
        if (Y.step == 1) {
            for (int c = 0; c < 3; c++)
                if (!plane_ok(Q.s[c], Q.ss[c], Q.sfs[c], 8 * bsi, batch, kStrideAny, false)) return false;
        } else if (!plane_ok(Q.s[0], Q.ss[0], Q.sfs[0], 4, batch, kStrideAny, false)) {
            return false;
        }
        if (!plane_ok(Q.d[0], Q.ds[0], Q.dfs[0], 8 * bso, batch, kStrideAny, false)) return false;
        for (int c = 1; c < 3; c++)
            if (!plane_ok(Q.d[c], Q.ds[c], Q.dfs[c], (8 >> dcsx) * bso, batch, kStrideAny, false)) return false;
        return true;
    };
    int ran = 0;                                         // bit 0: a vector kernel was launched, bit 1: the generic one
    auto vec = [&](const PlaneSet &Q, const FrameGeom &H) -> const char * {
        ran |= 1;
        if (win && wout) return launch_rgb_stack_vec_w11(st, L, L2, S, X, K, Q, Y, H, sink, ocsx, ocsy, tri, lds);
        if (win) return launch_rgb_stack_vec_w10(st, L, L2, S, X, K, Q, Y, H, sink, ocsx, ocsy, tri, lds);
        return launch_rgb_stack_vec_w00(st, L, L2, S, X, K, Q, Y, H, sink, ocsx, ocsy, tri, lds);
    };
    auto generic = [&](const PlaneSet &Q, const FrameGeom &H) {
        ran |= 2;
        hipLaunchKernelGGL(k_rgb_stack_generic, dim3(block_grid("k_rgb_stack_generic", H.w, H.rows, H.nframes, ocsx, ocsy)), dim3(256), 0,
                           st, L, L2, S, X, K, Q, H, Y, wout, sink, ocsx, ocsy);
        return "k_rgb_stack_generic";
    };
    const char *name = launch_vec_or_generic(variant, P, G, 8, vec_fits, vec, generic, [&](int wv) {
        const long long sb = (long long)wv * Y.step * bsi;
        return advance_planes(P, sb, sb, wv * bso, (wv >> dcsx) * bso);
    });
    if (!name || ran != 3) return name;
    // a ragged width: the vector kernel up to the last whole unit, the generic one for the rest (as launch_union reports it)
    static thread_local std::string both;
    both = std::string(name) + "+k_rgb_stack_generic";
    return both.c_str();
}
#endif  // LUTR_RSK_WI

}  // namespace lutr
