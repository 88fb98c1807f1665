// lutr_v210.hip -- gfx950 kernels of the fused YUV pass on v210 frames: the 10-bit 4:2:2 container of SDI capture
// and play-out cards (FourCC 'v210'), on the source side, the destination side or both.
//
// What they replace: the unpacking of a v210 frame into yuv422p10le a caller had to run ahead of lutr_apply_yuv, and the packing
// behind it.  The arithmetic is lutr_apply_yuv's, untouched: a v210 frame is the samples of yuv422p10le in another container.
//   row       ceil(w / 6) groups of four little-endian 32-bit words
//   word      three 10-bit codes: slot a = bits 0-9, b = bits 10-19, c = bits 20-29; bits 30-31 ignored on input, zero on output
//   group     word 0: Cb0 Y0 Cr0   word 1: Y1 Cb1 Y2   word 2: Cr1 Y3 Cb2   word 3: Y4 Cr2 Y5
//             pair k (Cbk, Crk) belongs to luma samples 2k and 2k + 1 of the group
// A v210 side is 10-bit 4:2:2; each side is v210 or planar on its own.  With a v210 source the planar destination may also be
// 4:2:0 or 4:4:4 (lutr_apply_yuv_xsub's contract, 3.8).
//
// One source, two kinds of translation unit (Makefile MIX_RULE):
//   without LUTR_V2_WI   the generic kernel and the launcher
//   LUTR_V2_WI / _WO     the vector kernels of one container mix, a v210 side counted as 16 bit: w11 -- v210 -> v210, v210 ->
//                        planar 16 bit (4:2:2, 4:2:0), planar 16 bit -> v210; w10 -- v210 -> planar 8 bit (4:2:2, 4:2:0)
#include "lutr_device.h"
#include "lutr_launch.h"
#include "lutr_pkcodes.h"

namespace lutr {

// (where the samples of a group sit, v2_get / v2_put and the word-by-word runs: lutr_pkcodes.h)
#ifdef LUTR_V2_WI
// ================================================================= vector kernel, global gather
// k_yuv_pk_vec's structure (lutr_pkyuv.hip): whole-word loads and stores, 2^OCSY luma rows per thread, lattice taps gathered from
// L1/L2, the thread walks its chroma pairs one after the other.  A v210 side moves whole groups, 16 bytes each; the thread takes
// as many groups as make whole words on the planar side: 1 (v210 -> v210), 2 (16-bit planes: 12 luma samples = 6 words, 6 chroma
// samples = 3 words) or 4 (8-bit planes: 24 luma samples = 6 words, 12 chroma samples = 3 words).  The planar runs of 6 and 3
// words start on a 4-byte boundary and no better (24 and 12 bytes per thread), so they move word by word.
// WP: the planar side is 16 bit (ignored for v210 -> v210).  VI / VO: the source / destination is v210.  The source is always
// 4:2:2; OCSY = 1 is a planar 4:2:0 destination.
template <int WP, int VI, int VO, int OCSY, int INTERP>
__global__ __launch_bounds__(256) void k_yuv_v210_vec(LutConsts L, YuvConsts K, PlaneSet P, FrameGeom G)
{
    static_assert(VI || VO, "planar on both sides is k_yuv_vec / k_yuv_xsub_vec");
    static_assert(!(VO && OCSY), "a v210 destination is 4:2:2");
    constexpr int NG = (VI && VO) ? 1 : (WP ? 2 : 4);             // groups per thread and row
    constexpr int PXT = 6 * NG, NP = 3 * NG;                      // luma samples, chroma pairs per thread and row
    constexpr int BH = 1 << OCSY;                                 // luma rows per thread
    constexpr int YW = PXT * (WP ? 2 : 1) / 4, CW = NP * (WP ? 2 : 1) / 4;   // words of a planar luma row / of ONE chroma component
    constexpr int RWI = VI ? 4 * NG : YW + 2 * CW;                // words of a source row
    constexpr int LWO = VO ? 4 * NG : YW;                         // words of a destination row that hold luma
    constexpr int CWO = VO ? 1 : 2 * CW;                          // words of a planar destination's Cb | Cr row
    static_assert((VI && VO) || (YW == 6 && CW == 3), "a thread must own whole words");
    const GFetch f(L);
    const unsigned uw = (unsigned)G.w / PXT;
    const unsigned ub = (unsigned)G.rows >> OCSY;
    const unsigned total = uw * ub * (unsigned)G.nframes;
    const unsigned u = blockIdx.x * 256u + threadIdx.x;
    if (u >= total) return;
    const unsigned xu = u % uw, t = u / uw;
    const int y0 = ((G.row0 >> OCSY) + (int)(t % ub)) * BH;       // first luma row of the thread
    const long long fr = t / ub;

    // a source row: v210 -- NG groups of four words; planar -- luma in [0, YW), Cb in [YW, YW + CW), Cr behind it.
    // Every code the thread owns is loaded before anything is stored: a destination that is the source sees its own input.
    uint32_t in[BH][RWI];
    uint32_t yo[BH][LWO], co[CWO];
#pragma unroll
    for (int dy = 0; dy < BH; dy++) {
        const long long y = (long long)(y0 + dy);
        if constexpr (VI) {
            const uint8_t *row = P.s[0] + fr * P.sfs[0] + y * P.ss[0] + (long long)xu * (16 * NG);
#pragma unroll
            for (int g = 0; g < NG; g++) ld_words<4>(in[dy] + 4 * g, row + 16 * g);
        } else {
            ld_dwords<YW>(in[dy], P.s[0] + fr * P.sfs[0] + y * P.ss[0] + (long long)xu * (YW * 4));
            ld_dwords<CW>(in[dy] + YW, P.s[1] + fr * P.sfs[1] + y * P.ss[1] + (long long)xu * (CW * 4));
            ld_dwords<CW>(in[dy] + YW + CW, P.s[2] + fr * P.sfs[2] + y * P.ss[2] + (long long)xu * (CW * 4));
        }
#pragma unroll
        for (int k = 0; k < LWO; k++) yo[dy][k] = 0;
    }
#pragma unroll
    for (int k = 0; k < CWO; k++) co[k] = 0;

#pragma unroll
    for (int j = 0; j < NP; j++) {
        const int g = j / 3, k = j % 3;                            // group of the thread, pair of the group
        Chroma c[BH];
#pragma unroll
        for (int dy = 0; dy < BH; dy++) {
            const float cbv = VI ? v2_get(in[dy][4 * g + kV2BW[k]], kV2BO[k]) : word_sample<WP>(in[dy] + YW, j);
            const float crv = VI ? v2_get(in[dy][4 * g + kV2RW[k]], kV2RO[k]) : word_sample<WP>(in[dy] + YW + CW, j);
            c[dy] = chroma_terms(K, cbv, crv);
        }
        float rs = 0.f, gs = 0.f, bs = 0.f;
#pragma unroll
        for (int dy = 0; dy < BH; dy++) {
#pragma unroll
            for (int dx = 0; dx < 2; dx++) {
                const int l = 2 * k + dx;                          // luma sample of the group
                const float yv = VI ? v2_get(in[dy][4 * g + kV2YW[l]], kV2YO[l]) : word_sample<WP>(in[dy], 2 * j + dx);
                const Rgb q = yuv_to_rgb(K, yv, c[dy]);
                const Rgb o = lut3d_px<INTERP>(L, f, q.r, q.g, q.b);
                rs += o.r; gs += o.g; bs += o.b;
                if constexpr (VO) v2_put(&yo[dy][4 * g + kV2YW[l]], kV2YO[l], rgb_to_y(K, o));
                else word_put<WP>(yo[dy], 2 * j + dx, rgb_to_y(K, o));
            }
        }
        if constexpr (VO) {
            v2_put(&yo[0][4 * g + kV2BW[k]], kV2BO[k], rgb_to_cb(K, rs, gs, bs));
            v2_put(&yo[0][4 * g + kV2RW[k]], kV2RO[k], rgb_to_cr(K, rs, gs, bs));
        } else {
            word_put<WP>(co, j, rgb_to_cb(K, rs, gs, bs));
            word_put<WP>(co + CW, j, rgb_to_cr(K, rs, gs, bs));
        }
        // Zero-instruction fence (k_yuv_vec's): keeps hipcc from hoisting the coordinates and taps of every pair of the thread to
        // the top; with it the pairs are emitted one after the other.
#pragma unroll
        for (int dy = 0; dy < BH; dy++) {
#pragma unroll
            for (int i = 0; i < RWI; i++) asm volatile("" : "+v"(in[dy][i]));
#pragma unroll
            for (int i = 0; i < LWO; i++) asm volatile("" : "+v"(yo[dy][i]));
        }
#pragma unroll
        for (int i = 0; i < CWO; i++) asm volatile("" : "+v"(co[i]));
    }
    if constexpr (VO) {
        uint8_t *row = P.d[0] + fr * P.dfs[0] + (long long)y0 * P.ds[0] + (long long)xu * (16 * NG);
#pragma unroll
        for (int g = 0; g < NG; g++) st_words<4>(row + 16 * g, yo[0] + 4 * g);
    } else {
#pragma unroll
        for (int dy = 0; dy < BH; dy++)
            st_dwords<YW>(P.d[0] + fr * P.dfs[0] + (long long)(y0 + dy) * P.ds[0] + (long long)xu * (YW * 4), yo[dy]);
        const long long r = (long long)(y0 >> OCSY);
        st_dwords<CW>(P.d[1] + fr * P.dfs[1] + r * P.ds[1] + (long long)xu * (CW * 4), co);
        st_dwords<CW>(P.d[2] + fr * P.dfs[2] + r * P.ds[2] + (long long)xu * (CW * 4), co + CW);
    }
}

// The vector kernels of this translation unit's container mix; the layout checks are the caller's (launch_yuv_v210).
const char *LUTR_CAT(LUTR_CAT(launch_yuv_v210_vec_w, LUTR_V2_WI), LUTR_V2_WO)(hipStream_t st, const LutConsts &L, const YuvConsts &K,
                                                                               const PlaneSet &P, const FrameGeom &G, const V210Args &A,
                                                                               int ocsy, int mode)
{
    constexpr int WP = LUTR_V2_WO;                                // (w11: every planar side is 16 bit; w10: the planar destination is 8 bit)
    const int pxt = v210_unit_px(A, WP);
    const long long units = (long long)(G.w / pxt) * (G.rows >> ocsy) * G.nframes;
    const dim3 grid((unsigned)((units + 255) / 256)), block(256);
#define V2_CASE(VI, VO, Y, I) \
    if (A.iv == VI && A.ov == VO && ocsy == Y && mode == I) { \
        hipLaunchKernelGGL((k_yuv_v210_vec<WP, VI, VO, Y, I>), grid, block, 0, st, L, K, P, G); \
        return "k_yuv_v210_vec<" LUTR_STR(LUTR_V2_WO) "," #VI "," #VO "," #Y "," #I ">"; \
    }
#define V2_SIDES(VI, VO, Y) V2_CASE(VI, VO, Y, 0) V2_CASE(VI, VO, Y, 1) V2_CASE(VI, VO, Y, 2)
    V2_SIDES(1, 0, 0) V2_SIDES(1, 0, 1)
#if LUTR_V2_WO
    V2_SIDES(1, 1, 0) V2_SIDES(0, 1, 0)
#endif
#undef V2_SIDES
#undef V2_CASE
    return nullptr;
}

#else  // !LUTR_V2_WI
// ================================================================= generic kernel
// One thread per group and union block: six luma samples (three pairs) wide, 2^ocsy rows high -- a v210 word holds codes of two
// pairs, so the group is the smallest unit a thread can own for its stores and for a destination that is the source.  Any
// stride (negative included), any planar depth 8..16 and alignment, odd sizes and the partial last group, all five modes, and a
// planar 4:4:4 destination besides 4:2:2 and 4:2:0.  k_yuv_pk_generic's sums with the input layout fixed at 4:2:2: every pixel
// takes the chroma sample of its own row, an output chroma block sums its pixels row by row.  A pixel outside the frame is the
// edge pixel again, so a partial block sums the edge column / row twice, like np.pad(mode="edge").  On a v210 destination a luma
// slot beyond the frame repeats the last real luma sample of the row and a pair beyond it the last real pair.  The thread's codes
// are all read before anything is stored.  v210 words move one at a time: their base is 4-byte aligned and no more.
__global__ __launch_bounds__(256) void k_yuv_v210_generic(LutConsts L, YuvConsts K, PlaneSet P, FrameGeom G, V210Args A, int wp_in,
                                                          int wp_out, int ocsx, int ocsy, int mode)
{
    const GFetch f(L);
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
        float yq[6], bq[3], rq[3];
#pragma unroll
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
                        const Rgb q = yuv_to_rgb(K, yv[dy][2 * k + dx], c);
                        const Rgb o = lut3d_px_rt(mode, L, f, q.r, q.g, q.b);
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

// ================================================================= launcher
const char *launch_yuv_v210(hipStream_t st, int variant, const LutConsts &L, const YuvConsts &K, const PlaneSet &P,
                            const FrameGeom &G, const V210Args &A, int din, int dout, int ocsx, int ocsy, int mode)
{
    const int wp_in = din > 8, wp_out = dout > 8;
    const int bh = 1 << ocsy;
    // the planar side's container decides the mix: v210 -> v210, a 16-bit planar side either way, an 8-bit planar destination; an
    // 8-bit planar source and a 4:4:4 destination have no vector kernel
    const bool both = A.iv && A.ov;
    const int wp = both ? 1 : (A.iv ? wp_out : wp_in);
    const bool mix_ok = ocsx == 1 && !(A.ov && ocsy) && (both || wp || A.iv);
    const int pxt = v210_unit_px(A, wp);
    const long long bs = wp ? 2 : 1;
    const bool batch = G.nframes > 1;
    auto vec_fits = [&](const PlaneSet &Q, const FrameGeom &H) {
        if (!mix_ok || !vec_mode(mode)) return false;
        if (H.w % pxt || H.row0 % bh || H.rows % bh) return false;
        if (!units_fit((long long)(H.w / pxt) * (H.rows / bh) * H.nframes)) return false;
        // a v210 plane moves in runs of 16 bytes, a planar one word by word
        if (!plane_ok(Q.s[0], Q.ss[0], Q.sfs[0], A.iv ? 16 : 4, batch, kStrideAny, false) ||
            !plane_ok(Q.d[0], Q.ds[0], Q.dfs[0], A.ov ? 16 : 4, batch, kStrideAny, false))
            return false;
        for (int c = 1; c < 3; c++)
            if ((!A.iv && !plane_ok(Q.s[c], Q.ss[c], Q.sfs[c], 4, batch, kStrideAny, false)) ||
                (!A.ov && !plane_ok(Q.d[c], Q.ds[c], Q.dfs[c], 4, batch, kStrideAny, false)))
                return false;
        return true;
    };
    auto vec = [&](const PlaneSet &Q, const FrameGeom &H) -> const char * {
        return wp ? launch_yuv_v210_vec_w11(st, L, K, Q, H, A, ocsy, mode) : launch_yuv_v210_vec_w10(st, L, K, Q, H, A, ocsy, mode);
    };
    auto generic = [&](const PlaneSet &Q, const FrameGeom &H) {
        const long long units = ((long long)H.w + 5) / 6 * blocks(H.rows, ocsy) * H.nframes;
        hipLaunchKernelGGL(k_yuv_v210_generic, dim3(stride_grid("k_yuv_v210_generic", units, kGridStrideCap)), dim3(256), 0, st, L, K, Q, H, A,
                           wp_in, wp_out,
                           ocsx, ocsy, mode);
        return "k_yuv_v210_generic";
    };
    // (no LDS-window kernel for v210 frames; the unit is 6, 12 or 24 luma samples wide, whole groups)
    return launch_vec_or_generic(variant, P, G, pxt, vec_fits, vec, generic, [&](int wv) {
        return advance_planes(P, A.iv ? wv / 6 * 16ll : wv * bs, (wv >> 1) * bs, A.ov ? wv / 6 * 16ll : wv * bs, (wv >> ocsx) * bs);
    });
}
#endif  // LUTR_V2_WI

}  // namespace lutr
