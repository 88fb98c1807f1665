// lutr_pkyuv.hip -- gfx950 kernels of the fused YUV pass on packed 4:2:2 frames: yuyv422 / uyvy422 / yvyu422 and
// y210le / y212le / y216le, on the source side, the destination side or both.
//
// What they replace: the de-interleave (and `>> (16 - depth)`) a caller had to run ahead of lutr_apply_yuv on a frame a capture
// card or a 4:2:2 hardware decoder wrote, and the interleave (and `<<`) behind it -- swscale's uyvy422 / y210le (un)packers around
// the reference's filter chain (ffmpeg.py:246, :304-310).  The arithmetic is lutr_apply_yuv's, untouched: a packed frame is the
// samples of yuv422p* in another container.
//   row       ceil(w / 2) groups of four samples, two luma and one Cb / Cr pair
//   order     luma first (Y0 C Y1 C: yuyv422, yvyu422, y21x) or chroma first (C Y0 C Y1: uyvy422); Cb first or Cr first (yvyu422)
//   shift     16-bit containers may carry the code in their high bits: code = word >> shift on input (low bits ignored), word =
//             code << shift on output (low bits zero)
// A packed side is 4:2:2; each side is packed or planar on its own.  With a packed source the planar destination may also be
// 4:2:0 or 4:4:4 (lutr_apply_yuv_xsub's contract, 3.8: chroma replicated over the input block, the output sample the mean of the
// LUT's RGB over the OUTPUT block).
//
// One source, two kinds of translation unit (Makefile MIX_RULE):
//   without LUTR_PK_WI   the generic kernel and the launcher
//   LUTR_PK_WI / _WO     the vector kernels of one container mix (8 -> 8, 16 -> 16, 16 -> 8): 4 side pairs x 3 modes
#include "lutr_device.h"
#include "lutr_launch.h"
#include "lutr_pkcodes.h"

namespace lutr {

#ifdef LUTR_PK_WI
// ================================================================= vector kernel, global gather
// k_yuv_semi_vec's structure (lutr_semi.hip): whole-word loads and stores, PXT luma samples per thread and row, 2^OCSY luma rows
// per thread, lattice taps gathered from L1/L2, the thread walks its groups one after the other.  A packed side moves the
// thread's luma and chroma of a row in ONE run of 16 bytes (two for the 16-bit side of 16 -> 8); a planar side in the three
// accesses of k_yuv_vec.  Group order and shift are wave-uniform kernel arguments: they end up in the offset operand of the
// bit-field extract that unpacks the sample anyway.
// (ld_run / st_run and the pk_* code positions: lutr_pkcodes.h)
// PI / PO: the source / destination is packed.  The source is always 4:2:2; OCSY = 1 is a planar 4:2:0 destination.
template <int WIN, int WOUT, int PI, int PO, int OCSY, int INTERP>
__global__ __launch_bounds__(256) void k_yuv_pk_vec(LutConsts L, YuvConsts K, PlaneSet P, FrameGeom G, PkArgs A)
{
    static_assert(PI || PO, "planar on both sides is k_yuv_vec / k_yuv_xsub_vec");
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
    const GFetch f(L);
    const unsigned uw = (unsigned)G.w / PXT;
    const unsigned ub = (unsigned)G.rows >> OCSY;
    const unsigned total = uw * ub * (unsigned)G.nframes;
    const unsigned u = blockIdx.x * 256u + threadIdx.x;
    if (u >= total) return;
    const unsigned xu = u % uw, t = u / uw;
    const int y0 = ((G.row0 >> OCSY) + (int)(t % ub)) * BH;       // first luma row of the thread
    const long long fr = t / ub;
    const unsigned icf = (unsigned)A.icf, icsw = (unsigned)A.icsw, ish = (unsigned)A.ishift;
    const unsigned ocf = (unsigned)A.ocf, ocsw = (unsigned)A.ocsw;

    // a source row: packed -- RWI words of groups; planar -- luma in [0, YWI), Cb in [YWI, YWI + CWI), Cr behind it.
    // Every code the thread owns is loaded before anything is stored: a destination that is the source sees its own input.
    uint32_t in[BH][RWI];
    uint32_t yo[BH][LWO], co[2 * CWO];                            // (co: a planar destination's Cb | Cr row)
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
        Chroma c[BH];
#pragma unroll
        for (int dy = 0; dy < BH; dy++) {
            const float cbv = PI ? pk_chroma<WIN>(in[dy], j, 0u, icf, icsw, ish) : word_sample<WIN>(in[dy] + YWI, j);
            const float crv = PI ? pk_chroma<WIN>(in[dy], j, 1u, icf, icsw, ish) : word_sample<WIN>(in[dy] + YWI + CWI, j);
            c[dy] = chroma_terms(K, cbv, crv);
        }
        float rs = 0.f, gs = 0.f, bs = 0.f;
#pragma unroll
        for (int dy = 0; dy < BH; dy++) {
#pragma unroll
            for (int dx = 0; dx < 2; dx++) {
                const float yv = PI ? pk_luma<WIN>(in[dy], j, dx, icf, ish) : word_sample<WIN>(in[dy], 2 * j + dx);
                const Rgb q = yuv_to_rgb(K, yv, c[dy]);
                const Rgb o = lut3d_px<INTERP>(L, f, q.r, q.g, q.b);
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
        // Zero-instruction fence (k_yuv_vec's): keeps hipcc from hoisting the coordinates and taps of every group of the thread to
        // the top; with it the groups are emitted one after the other.
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

// The vector kernels of this translation unit's container mix; the layout checks are the caller's (launch_yuv_packed).
const char *LUTR_CAT(LUTR_CAT(launch_yuv_pk_vec_w, LUTR_PK_WI), LUTR_PK_WO)(hipStream_t st, const LutConsts &L, const YuvConsts &K,
                                                                             const PlaneSet &P, const FrameGeom &G, const PkArgs &A,
                                                                             int ocsy, int mode)
{
    constexpr int WI = LUTR_PK_WI, WO = LUTR_PK_WO;
    constexpr int PXT = vec_bytes<WI, WO>() / (WI ? 2 : 1);
    const long long units = (long long)(G.w / PXT) * (G.rows >> ocsy) * G.nframes;
    const dim3 grid((unsigned)((units + 255) / 256)), block(256);
#define PK_CASE(PI, PO, Y, I) \
    if (A.ipk == PI && A.opk == PO && ocsy == Y && mode == I) { \
        hipLaunchKernelGGL((k_yuv_pk_vec<WI, WO, PI, PO, Y, I>), grid, block, 0, st, L, K, P, G, A); \
        return "k_yuv_pk_vec<" LUTR_STR(LUTR_PK_WI) "," LUTR_STR(LUTR_PK_WO) "," #PI "," #PO "," #Y "," #I ">"; \
    }
#define PK_SIDES(PI, PO, Y) PK_CASE(PI, PO, Y, 0) PK_CASE(PI, PO, Y, 1) PK_CASE(PI, PO, Y, 2)
    PK_SIDES(1, 1, 0) PK_SIDES(1, 0, 0) PK_SIDES(0, 1, 0) PK_SIDES(1, 0, 1)
#undef PK_SIDES
#undef PK_CASE
    return nullptr;
}

#else  // !LUTR_PK_WI
// ================================================================= generic kernel
// One thread per union block: one group wide (two luma samples), 2^ocsy rows.  Any depth, stride (negative included) or
// alignment, odd sizes, all five modes, and a planar 4:4:4 destination besides 4:2:2 and 4:2:0.  xsub_union_block's sums
// (lutr_xsub.hip) with the input layout fixed at 4:2:2: every pixel takes the chroma sample of its own row, an output chroma block
// sums its pixels row by row.  A pixel outside the frame is the edge pixel again, so a partial block sums the edge column / row twice, like
// np.pad(mode="edge"), and the second luma sample of an odd-width packed row comes out as a copy of the last real one.  The
// block's codes are all read before anything is stored: a destination that is the source sees its own input.
__global__ __launch_bounds__(256) void k_yuv_pk_generic(LutConsts L, YuvConsts K, PlaneSet P, FrameGeom G, PkArgs A, int win,
                                                        int wout, int ocsx, int ocsy, int mode)
{
    const GFetch f(L);
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
                    const Rgb q = yuv_to_rgb(K, yv[dy][dx], c);
                    const Rgb o = lut3d_px_rt(mode, L, f, q.r, q.g, q.b);
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

// ================================================================= launcher
const char *launch_yuv_packed(hipStream_t st, int variant, const LutConsts &L, const YuvConsts &K, const PlaneSet &P,
                              const FrameGeom &G, const PkArgs &A, int din, int dout, int ocsx, int ocsy, int mode)
{
    const int win = din > 8, wout = dout > 8;
    const int bh = 1 << ocsy;
    // the vector kernels' unit: 8 luma samples per row, 4 for 16 -> 16 bit; 8 -> 16 bit has none, nor has a 4:4:4 destination
    const bool mix_ok = (win == wout || (win && !wout)) && ocsx == 1 && (A.ipk || A.opk) && !(A.opk && ocsy);
    const int pxt = (win && !wout) ? 8 : (win ? 4 : 8);
    const long long bsi = win ? 2 : 1, bso = wout ? 2 : 1;
    const bool batch = G.nframes > 1;
    // a packed row moves in runs of 16 bytes (2 pxt samples; two runs for the 16-bit side of 16 -> 8), a planar luma row pxt
    // samples and a planar chroma row pxt / 2 per access
    auto run = [](long long bytes) { return bytes > 16 ? 16ll : bytes; };
    auto vec_fits = [&](const PlaneSet &Q, const FrameGeom &H) {
        if (!mix_ok || !vec_mode(mode)) return false;
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
        if (win && wout) return launch_yuv_pk_vec_w11(st, L, K, Q, H, A, ocsy, mode);
        if (win) return launch_yuv_pk_vec_w10(st, L, K, Q, H, A, ocsy, mode);
        return launch_yuv_pk_vec_w00(st, L, K, Q, H, A, ocsy, mode);
    };
    auto generic = [&](const PlaneSet &Q, const FrameGeom &H) {
        hipLaunchKernelGGL(k_yuv_pk_generic, dim3(block_grid("k_yuv_pk_generic", H.w, H.rows, H.nframes, 1, ocsy)), dim3(256), 0, st, L, K, Q, H, A,
                           win,
                           wout, ocsx, ocsy, mode);
        return "k_yuv_pk_generic";
    };
    // (no LDS-window kernel for packed frames; the unit is 4 or 8 luma samples wide, whole groups)
    return launch_vec_or_generic(variant, P, G, pxt, vec_fits, vec, generic, [&](int wv) {
        return advance_planes(P, (A.ipk ? 2 * wv : wv) * bsi, (wv >> 1) * bsi, (A.opk ? 2 * wv : wv) * bso, (wv >> ocsx) * bso);
    });
}
#endif  // LUTR_PK_WI

}  // namespace lutr
