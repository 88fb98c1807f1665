// lutr_semi.hip -- gfx950 kernels of the fused YUV pass on semi-planar frames: nv12 / nv21 / nv16 and the
// p010 / p210 family, on the source side, the destination side or both.
//
// What they replace: the de-interleave (and `>> (16 - depth)`) a caller had to run ahead of lutr_apply_yuv on a surface a
// hardware decoder wrote, and the interleave (and `<<`) behind it for a hardware encoder -- swscale's nv12 / p010le
// (un)packers around the reference's filter chain (ffmpeg.py:246, :304-310).  The arithmetic is lutr_apply_yuv's, untouched: a
// semi-planar frame is the same samples in another container.
//   plane 0   luma, one code per sample
//   plane 1   ceil(w / 2) pairs per row, (Cb, Cr) or with `swap` (Cr, Cb); ceil(h / 2) rows for 4:2:0, h rows for 4:2:2
//   shift     16-bit containers may carry the code in their high bits: code = word >> shift on input (low bits ignored), word =
//             code << shift on output (low bits zero)
// Both sides have the same chroma subsampling (csx = 1); each side is planar or semi-planar on its own.
//
// One source, two kinds of translation unit (Makefile MIX_RULE):
//   without LUTR_SM_WI   the generic kernel and the launcher
//   LUTR_SM_WI / _WO     the vector kernels of one container mix (8 -> 8, 16 -> 16, 16 -> 8): 3 side pairs x 2 layouts x 3 modes
#include "lutr_device.h"
#include "lutr_launch.h"

namespace lutr {

#ifdef LUTR_SM_WI
// ================================================================= vector kernel, global gather
// k_yuv_xsub_vec's structure (lutr_xsub.hip): whole-word loads and stores, VB bytes of luma per thread and row, 2^CSY luma rows
// and one chroma row per thread, lattice taps gathered from L1/L2, the thread walks its chroma blocks one after the other.
// A semi-planar side moves the thread's Cb and Cr in ONE access of twice the width; a planar side in two.  (Frame written out: see
// k_yuv_vec.)
// (the shifted codes are unpacked by word_code, lutr_device.h)
// (a, b) <-> (b, a) in every pair of a word: the two halves of a 16-bit pair, the bytes of each of the two 8-bit pairs
template <int WIDE>
__device__ __forceinline__ uint32_t swap_pairs(uint32_t w)
{
    if constexpr (WIDE) return (w >> 16) | (w << 16);
    else return ((w & 0x00ff00ffu) << 8) | ((w >> 8) & 0x00ff00ffu);
}

template <int WIN, int WOUT, int SI, int SO, int CSX, int CSY, int INTERP>
__global__ __launch_bounds__(256) void k_yuv_semi_vec(LutConsts L, YuvConsts K, PlaneSet P, FrameGeom G, SemiArgs A)
{
    static_assert(CSX == 1, "semi-planar formats are 4:2:0 or 4:2:2");
    constexpr int VB = vec_bytes<WIN, WOUT>();
    constexpr int PXT = VB / (WIN ? 2 : 1);                       // luma samples per thread per row
    constexpr int YWI = VB / 4, YWO = PXT * (WOUT ? 2 : 1) / 4;   // luma words per thread per row, in / out
    constexpr int BH = 1 << CSY;                                  // the chroma block is 2 x BH
    constexpr int NB = PXT / 2;                                   // chroma blocks per thread
    constexpr int CWI = NB * (WIN ? 2 : 1) / 4, CWO = NB * (WOUT ? 2 : 1) / 4;   // words of ONE chroma component per thread
    static_assert(NB >= 1 && CWI >= 1 && CWO >= 1 && YWO >= 1, "a thread must own whole words");
    const GFetch f(L);
    const unsigned uw = (unsigned)G.w / PXT;
    const unsigned ub = (unsigned)G.rows >> CSY;
    const unsigned total = uw * ub * (unsigned)G.nframes;
    const unsigned u = blockIdx.x * 256u + threadIdx.x;
    if (u >= total) return;
    const unsigned xu = u % uw, t = u / uw;
    const int y0 = ((G.row0 >> CSY) + (int)(t % ub)) * BH;        // first luma row of the thread
    const long long cr_ = (long long)(y0 >> CSY);                 // its chroma row
    const long long fr = t / ub;
    const long long xi = (long long)xu * VB, xo = (long long)xu * (YWO * 4);
    const unsigned ish = (unsigned)A.ishift;

    // chroma words: a planar side holds Cb in [0, CW) and Cr in [CW, 2 CW); a semi-planar side 2 CW words of pairs, Cb first
    // (a Cr-first plane is turned round once per word)
    uint32_t yw[BH][YWI], ci[2 * CWI];
    uint32_t yo[BH][YWO], co[2 * CWO];
#pragma unroll
    for (int dy = 0; dy < BH; dy++) {
        ld_words<YWI>(yw[dy], P.s[0] + fr * P.sfs[0] + (long long)(y0 + dy) * P.ss[0] + xi);
#pragma unroll
        for (int k = 0; k < YWO; k++) yo[dy][k] = 0;
    }
    if constexpr (SI) {
        ld_words<2 * CWI>(ci, P.s[1] + fr * P.sfs[1] + cr_ * P.ss[1] + (long long)xu * (2 * CWI * 4));
        if (A.iswap) {
#pragma unroll
            for (int k = 0; k < 2 * CWI; k++) ci[k] = swap_pairs<WIN>(ci[k]);
        }
    } else {
        ld_words<CWI>(ci, P.s[1] + fr * P.sfs[1] + cr_ * P.ss[1] + (long long)xu * (CWI * 4));
        ld_words<CWI>(ci + CWI, P.s[2] + fr * P.sfs[2] + cr_ * P.ss[2] + (long long)xu * (CWI * 4));
    }
#pragma unroll
    for (int k = 0; k < 2 * CWO; k++) co[k] = 0;

#pragma unroll
    for (int j = 0; j < NB; j++) {
        const float cbv = SI ? word_code<WIN>(ci, 2 * j, ish) : word_code<WIN>(ci, j, ish);
        const float crv = SI ? word_code<WIN>(ci, 2 * j + 1, ish) : word_code<WIN>(ci + CWI, j, ish);
        const Chroma c = chroma_terms(K, cbv, crv);
        float rs = 0.f, gs = 0.f, bs = 0.f;
#pragma unroll
        for (int dy = 0; dy < BH; dy++) {
#pragma unroll
            for (int dx = 0; dx < 2; dx++) {
                const int i = j * 2 + dx;
                const Rgb q = yuv_to_rgb(K, word_code<WIN>(yw[dy], i, ish), c);
                const Rgb o = lut3d_px<INTERP>(L, f, q.r, q.g, q.b);
                rs += o.r; gs += o.g; bs += o.b;
                word_put<WOUT>(yo[dy], i, rgb_to_y(K, o));
            }
        }
        if constexpr (SO) {
            word_put<WOUT>(co, 2 * j, rgb_to_cb(K, rs, gs, bs));
            word_put<WOUT>(co, 2 * j + 1, rgb_to_cr(K, rs, gs, bs));
        } else {
            word_put<WOUT>(co, j, rgb_to_cb(K, rs, gs, bs));
            word_put<WOUT>(co + CWO, j, rgb_to_cr(K, rs, gs, bs));
        }
        // Zero-instruction fence (k_yuv_vec's): keeps hipcc from hoisting the coordinates and taps of every chroma block of the
        // thread to the top; with it the blocks are emitted one after the other.
#pragma unroll
        for (int dy = 0; dy < BH; dy++) {
#pragma unroll
            for (int k = 0; k < YWI; k++) asm volatile("" : "+v"(yw[dy][k]));
#pragma unroll
            for (int k = 0; k < YWO; k++) asm volatile("" : "+v"(yo[dy][k]));
        }
#pragma unroll
        for (int k = 0; k < 2 * CWI; k++) asm volatile("" : "+v"(ci[k]));
#pragma unroll
        for (int k = 0; k < 2 * CWO; k++) asm volatile("" : "+v"(co[k]));
    }
    // the container's alignment: one shift per packed word -- two codes below 2^depth cannot carry into each other
    if constexpr (WOUT) {
        const unsigned osh = (unsigned)A.oshift;
#pragma unroll
        for (int dy = 0; dy < BH; dy++)
#pragma unroll
            for (int k = 0; k < YWO; k++) yo[dy][k] <<= osh;
#pragma unroll
        for (int k = 0; k < 2 * CWO; k++) co[k] <<= osh;
    }
#pragma unroll
    for (int dy = 0; dy < BH; dy++)
        st_words<YWO>(P.d[0] + fr * P.dfs[0] + (long long)(y0 + dy) * P.ds[0] + xo, yo[dy]);
    if constexpr (SO) {
        if (A.oswap) {
#pragma unroll
            for (int k = 0; k < 2 * CWO; k++) co[k] = swap_pairs<WOUT>(co[k]);
        }
        st_words<2 * CWO>(P.d[1] + fr * P.dfs[1] + cr_ * P.ds[1] + (long long)xu * (2 * CWO * 4), co);
    } else {
        st_words<CWO>(P.d[1] + fr * P.dfs[1] + cr_ * P.ds[1] + (long long)xu * (CWO * 4), co);
        st_words<CWO>(P.d[2] + fr * P.dfs[2] + cr_ * P.ds[2] + (long long)xu * (CWO * 4), co + CWO);
    }
}

// The vector kernels of this translation unit's container mix; the layout checks are the caller's (launch_yuv_semi).
const char *LUTR_CAT(LUTR_CAT(launch_yuv_semi_vec_w, LUTR_SM_WI), LUTR_SM_WO)(hipStream_t st, const LutConsts &L, const YuvConsts &K,
                                                                               const PlaneSet &P, const FrameGeom &G,
                                                                               const SemiArgs &A, int csy, int mode)
{
    constexpr int WI = LUTR_SM_WI, WO = LUTR_SM_WO;
    constexpr int PXT = vec_bytes<WI, WO>() / (WI ? 2 : 1);
    const long long units = (long long)(G.w / PXT) * (G.rows >> csy) * G.nframes;
    const dim3 grid((unsigned)((units + 255) / 256)), block(256);
#define SM_CASE(SI, SO, Y, I) \
    if (A.isemi == SI && A.osemi == SO && csy == Y && mode == I) { \
        hipLaunchKernelGGL((k_yuv_semi_vec<WI, WO, SI, SO, 1, Y, I>), grid, block, 0, st, L, K, P, G, A); \
        return "k_yuv_semi_vec<" LUTR_STR(LUTR_SM_WI) "," LUTR_STR(LUTR_SM_WO) "," #SI "," #SO ",1," #Y "," #I ">"; \
    }
#define SM_SIDES(SI, SO) SM_CASE(SI, SO, 1, 0) SM_CASE(SI, SO, 1, 1) SM_CASE(SI, SO, 1, 2) \
                         SM_CASE(SI, SO, 0, 0) SM_CASE(SI, SO, 0, 1) SM_CASE(SI, SO, 0, 2)
    SM_SIDES(1, 1) SM_SIDES(1, 0) SM_SIDES(0, 1)
#undef SM_SIDES
#undef SM_CASE
    return nullptr;
}

#else  // !LUTR_SM_WI
// ================================================================= generic kernel
// One thread per chroma block (2 x 2^csy luma samples); any depth, stride (negative included) or alignment, odd sizes, all five
// modes.  A pixel outside the frame is the edge pixel again, so a partial block sums the edge column / row twice, like
// np.pad(mode="edge"); only samples inside the planes are written.  The block's codes are all read before anything is stored:
// a destination that is the source plane for plane sees its own input.
// (its own block walk, not for_each_block of lutr_device.h: with the shared walk it takes 73 VGPRs for 72, 6 waves per SIMD for 7)
__global__ __launch_bounds__(256) void k_yuv_semi_generic(LutConsts L, YuvConsts K, PlaneSet P, FrameGeom G, SemiArgs A, int win,
                                                          int wout, int csy, int mode)
{
    const GFetch f(L);
    const int bh = 1 << csy;
    const int cw = (G.w + 1) >> 1;
    const int ur0 = G.row0 >> csy;
    const int urows = ((G.row0 + G.rows + bh - 1) >> csy) - ur0;
    const long long total = (long long)cw * urows * G.nframes;
    // where Cb and Cr of chroma sample cx are: plane, elements per sample and the component's element inside a pair
    const int icr = A.isemi ? 1 : 2, ocr = A.osemi ? 1 : 2;
    const int im = A.isemi ? 2 : 1, om = A.osemi ? 2 : 1;
    const int icb0 = A.isemi ? A.iswap : 0, icr0 = A.isemi ? 1 - A.iswap : 0;
    const int ocb0 = A.osemi ? A.oswap : 0, ocr0 = A.osemi ? 1 - A.oswap : 0;
    for (long long u = blockIdx.x * 256ll + threadIdx.x; u < total; u += (long long)gridDim.x * 256ll) {
        const int cx = (int)(u % cw);
        const long long t = u / cw;
        const int cy = ur0 + (int)(t % urows);
        const long long fr = t / urows;
        float yv[2][2];
        for (int dy = 0; dy < bh; dy++) {
            const int yy = cy * bh + dy, y = yy < G.h ? yy : G.h - 1;
            const uint8_t *row = P.s[0] + fr * P.sfs[0] + (long long)y * P.ss[0];
            for (int dx = 0; dx < 2; dx++) {
                const int xx = cx * 2 + dx;
                yv[dy][dx] = ld_code(row, xx < G.w ? xx : G.w - 1, win, A.ishift);
            }
        }
        const float cbv = ld_code(P.s[1] + fr * P.sfs[1] + (long long)cy * P.ss[1], (long long)cx * im + icb0, win, A.ishift);
        const float crv = ld_code(P.s[icr] + fr * P.sfs[icr] + (long long)cy * P.ss[icr], (long long)cx * im + icr0, win, A.ishift);
        const Chroma c = chroma_terms(K, cbv, crv);
        float rs = 0.f, gs = 0.f, bs = 0.f;
        for (int dy = 0; dy < bh; dy++) {
            const int yy = cy * bh + dy;
            uint8_t *row = P.d[0] + fr * P.dfs[0] + (long long)(yy < G.h ? yy : G.h - 1) * P.ds[0];
            for (int dx = 0; dx < 2; dx++) {
                const int xx = cx * 2 + dx;
                const Rgb q = yuv_to_rgb(K, yv[dy][dx], c);
                const Rgb o = lut3d_px_rt(mode, L, f, q.r, q.g, q.b);
                rs += o.r; gs += o.g; bs += o.b;
                if (yy < G.h && xx < G.w) st_code(row, xx, wout, A.oshift, rgb_to_y(K, o));
            }
        }
        st_code(P.d[1] + fr * P.dfs[1] + (long long)cy * P.ds[1], (long long)cx * om + ocb0, wout, A.oshift, rgb_to_cb(K, rs, gs, bs));
        st_code(P.d[ocr] + fr * P.dfs[ocr] + (long long)cy * P.ds[ocr], (long long)cx * om + ocr0, wout, A.oshift, rgb_to_cr(K, rs, gs, bs));
    }
}

// ================================================================= launcher
const char *launch_yuv_semi(hipStream_t st, int variant, const LutConsts &L, const YuvConsts &K, const PlaneSet &P,
                            const FrameGeom &G, const SemiArgs &A, int din, int dout, int csy, int mode)
{
    const int win = din > 8, wout = dout > 8;
    const int bh = 1 << csy;
    // the vector kernels' unit: 8 bytes of luma per row (16 for a 16-bit source written as 8 bit); 8 -> 16 bit has none, nor has
    // a planar pair (with both sides planar only a shifted container comes here)
    const bool mix_ok = (win == wout || (win && !wout)) && (A.isemi || A.osemi);
    const int pxt = (win && !wout) ? 8 : (win ? 4 : 8);
    const long long bsi = win ? 2 : 1, bso = wout ? 2 : 1;
    const bool batch = G.nframes > 1;
    auto vec_fits = [&](const PlaneSet &Q, const FrameGeom &H) {
        if (!mix_ok || !vec_mode(mode)) return false;
        if (H.w % pxt || H.row0 % bh || H.rows % bh) return false;
        if (!units_fit((long long)(H.w / pxt) * (H.rows / bh) * H.nframes)) return false;
        if (!plane_ok(Q.s[0], Q.ss[0], Q.sfs[0], pxt * bsi, batch, kStrideAny, false) || !plane_ok(Q.d[0], Q.ds[0], Q.dfs[0], pxt * bso, batch, kStrideAny, false))
            return false;
        // a plane of pairs moves pxt / 2 pairs = pxt samples per access, a planar chroma plane pxt / 2 samples
        for (int c = 1; c < (A.isemi ? 2 : 3); c++)
            if (!plane_ok(Q.s[c], Q.ss[c], Q.sfs[c], (A.isemi ? pxt : pxt >> 1) * bsi, batch, kStrideAny, false)) return false;
        for (int c = 1; c < (A.osemi ? 2 : 3); c++)
            if (!plane_ok(Q.d[c], Q.ds[c], Q.dfs[c], (A.osemi ? pxt : pxt >> 1) * bso, batch, kStrideAny, false)) return false;
        return true;
    };
    auto vec = [&](const PlaneSet &Q, const FrameGeom &H) -> const char * {
        if (win && wout) return launch_yuv_semi_vec_w11(st, L, K, Q, H, A, csy, mode);
        if (win) return launch_yuv_semi_vec_w10(st, L, K, Q, H, A, csy, mode);
        return launch_yuv_semi_vec_w00(st, L, K, Q, H, A, csy, mode);
    };
    auto generic = [&](const PlaneSet &Q, const FrameGeom &H) {
        hipLaunchKernelGGL(k_yuv_semi_generic, dim3(block_grid("k_yuv_semi_generic", H.w, H.rows, H.nframes, 1, csy)), dim3(256), 0, st, L, K, Q, H,
                           A, win, wout, csy, mode);
        return "k_yuv_semi_generic";
    };
    // (no LDS-window kernel for semi-planar frames; the unit is 4 or 8 luma samples wide, whole chroma blocks)
    return launch_vec_or_generic(variant, P, G, pxt, vec_fits, vec, generic, [&](int wv) {
        return advance_planes(P, wv * bsi, (A.isemi ? wv : wv >> 1) * bsi, wv * bso, (A.osemi ? wv : wv >> 1) * bso);
    });
}
#endif  // LUTR_SM_WI

}  // namespace lutr
