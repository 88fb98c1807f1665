// lutr_dual.hip -- gfx950 kernels of the fused YUV pass with TWO planar outputs.
//
// What they replace: the two stages of the reference's "pro" mode (ffmpeg.py:417-472): a ProRes 422 HQ master with the LUT
// (yuv422p10le), then the delivery file in the user's pix_fmt.  Both outputs come from the same lut3d result, so one pass reads
// the source once, converts and gathers once per pixel and runs the output stage twice.  The contract is 3.8's per output:
//   up-sampling    each source chroma sample is replicated over its INPUT block
//   down-sampling  each output's chroma sample is the mean of the LUT's integer RGB over that output's OWN block
// The unit of work is the union block of the three layouts, 2^max(csx) x 2^max(csy) luma samples: it holds whole chroma blocks of
// the source and of both outputs.
//
// One source, two kinds of translation unit (Makefile DUAL_RULE):
//   without LUTR_DU_WI        the generic kernel and the launcher
//   LUTR_DU_WI / _WA / _WB    the vector kernels of one container mix (16 -> 16+16, 16 -> 16+8, 8 -> 8+8): 3 input layouts x
//                             3 layouts of output B x 3 modes; output A is 4:2:2
#include "lutr_device.h"
#include "lutr_launch.h"

namespace lutr {

// luma samples per thread and row of the vector kernels: 8 for a mix with an 8-bit side, 4 for 16 -> 16+16, so that every plane
// row of a thread is whole 32-bit words
constexpr int dual_pxt(int win, int wa, int wb) { return (win && wa && wb) ? 4 : 8; }

#ifdef LUTR_DU_WI
// ================================================================= vector kernel, global gather
// k_yuv_xsub_vec's structure (lutr_xsub.hip) with a second set of output registers: whole-word loads and stores, BH luma rows per
// thread, lattice taps gathered from L1/L2; the thread walks its union blocks one after the other.  Output A is 4:2:2, so the union
// block is 2 luma samples wide and 2^max(ICSY, BCSY) rows high.  P.d / KA: output A; B / KB: output B.
template <int WIN, int WA, int WB, int ICSX, int ICSY, int BCSX, int BCSY, int INTERP>
__global__ __launch_bounds__(256) void k_yuv_dual_vec(LutConsts L, YuvConsts KA, YuvConsts KB, PlaneSet P, DstPlanes B, FrameGeom G)
{
    constexpr int PXT = dual_pxt(WIN, WA, WB);                    // luma samples per thread per row
    constexpr int SI = WIN ? 2 : 1, SA = WA ? 2 : 1, SB = WB ? 2 : 1;
    constexpr int YWI = PXT * SI / 4, YWA = PXT * SA / 4, YWB = PXT * SB / 4;   // luma words per thread per row
    constexpr int CSY = cmax(ICSY, BCSY);
    constexpr int BW = 2, BH = 1 << CSY;                          // the union block
    constexpr int NB = PXT / BW;                                  // union blocks per thread
    constexpr int IRH = BH >> ICSY, BRH = BH >> BCSY;             // chroma rows per thread: in, B (A: BH)
    constexpr int IBX = BW >> ICSX, BBX = BW >> BCSX;             // chroma samples per union block and row: in, B (A: 1)
    constexpr int CWI = (PXT >> ICSX) * SI / 4, CWA = (PXT >> 1) * SA / 4, CWB = (PXT >> BCSX) * SB / 4;
    static_assert(NB >= 1 && YWI >= 1 && YWA >= 1 && YWB >= 1 && CWI >= 1 && CWA >= 1 && CWB >= 1, "a thread must own whole words");
    const GFetch f(L);
    const unsigned uw = (unsigned)G.w / PXT;
    const unsigned ub = (unsigned)G.rows >> CSY;
    const unsigned total = uw * ub * (unsigned)G.nframes;
    const unsigned u = blockIdx.x * 256u + threadIdx.x;
    if (u >= total) return;
    const unsigned xu = u % uw, t = u / uw;
    const int y0 = ((G.row0 >> CSY) + (int)(t % ub)) * BH;        // first luma row of the thread
    const long long fr = t / ub;

    uint32_t yw[BH][YWI], cbw[IRH][CWI], crw[IRH][CWI];
    uint32_t ya[BH][YWA], cba[BH][CWA], cra[BH][CWA];
    uint32_t yb[BH][YWB], cbb[BRH][CWB], crb[BRH][CWB];
#pragma unroll
    for (int dy = 0; dy < BH; dy++) {
        ld_words<YWI>(yw[dy], P.s[0] + fr * P.sfs[0] + (long long)(y0 + dy) * P.ss[0] + (long long)xu * (YWI * 4));
#pragma unroll
        for (int k = 0; k < YWA; k++) ya[dy][k] = 0;
#pragma unroll
        for (int k = 0; k < YWB; k++) yb[dy][k] = 0;
#pragma unroll
        for (int k = 0; k < CWA; k++) { cba[dy][k] = 0; cra[dy][k] = 0; }
    }
#pragma unroll
    for (int iy = 0; iy < IRH; iy++) {
        const long long r = (long long)((y0 >> ICSY) + iy);
        ld_words<CWI>(cbw[iy], P.s[1] + fr * P.sfs[1] + r * P.ss[1] + (long long)xu * (CWI * 4));
        ld_words<CWI>(crw[iy], P.s[2] + fr * P.sfs[2] + r * P.ss[2] + (long long)xu * (CWI * 4));
    }
#pragma unroll
    for (int oy = 0; oy < BRH; oy++)
#pragma unroll
        for (int k = 0; k < CWB; k++) { cbb[oy][k] = 0; crb[oy][k] = 0; }

#pragma unroll
    for (int j = 0; j < NB; j++) {
        Chroma c[IRH][IBX];
#pragma unroll
        for (int iy = 0; iy < IRH; iy++)
#pragma unroll
            for (int ix = 0; ix < IBX; ix++)
                c[iy][ix] = chroma_terms(KA, word_sample<WIN>(cbw[iy], j * IBX + ix), word_sample<WIN>(crw[iy], j * IBX + ix));
        float ra[BH], ga[BH], ba[BH];                             // A's sums: one chroma sample per row of the block
        float rb[BRH][BBX], gb[BRH][BBX], bb[BRH][BBX];
#pragma unroll
        for (int dy = 0; dy < BH; dy++) { ra[dy] = 0.f; ga[dy] = 0.f; ba[dy] = 0.f; }
#pragma unroll
        for (int oy = 0; oy < BRH; oy++)
#pragma unroll
            for (int ox = 0; ox < BBX; ox++) { rb[oy][ox] = 0.f; gb[oy][ox] = 0.f; bb[oy][ox] = 0.f; }
#pragma unroll
        for (int dy = 0; dy < BH; dy++) {
#pragma unroll
            for (int dx = 0; dx < BW; dx++) {
                const int i = j * BW + dx;
                const Rgb q = yuv_to_rgb(KA, word_sample<WIN>(yw[dy], i), c[dy >> ICSY][dx >> ICSX]);
                const Rgb o = lut3d_px<INTERP>(L, f, q.r, q.g, q.b);
                ra[dy] += o.r; ga[dy] += o.g; ba[dy] += o.b;
                rb[dy >> BCSY][dx >> BCSX] += o.r; gb[dy >> BCSY][dx >> BCSX] += o.g; bb[dy >> BCSY][dx >> BCSX] += o.b;
                word_put<WA>(ya[dy], i, rgb_to_y(KA, o));
                word_put<WB>(yb[dy], i, rgb_to_y(KB, o));
            }
        }
#pragma unroll
        for (int dy = 0; dy < BH; dy++) {
            word_put<WA>(cba[dy], j, rgb_to_cb(KA, ra[dy], ga[dy], ba[dy]));
            word_put<WA>(cra[dy], j, rgb_to_cr(KA, ra[dy], ga[dy], ba[dy]));
        }
#pragma unroll
        for (int oy = 0; oy < BRH; oy++)
#pragma unroll
            for (int ox = 0; ox < BBX; ox++) {
                word_put<WB>(cbb[oy], j * BBX + ox, rgb_to_cb(KB, rb[oy][ox], gb[oy][ox], bb[oy][ox]));
                word_put<WB>(crb[oy], j * BBX + ox, rgb_to_cr(KB, rb[oy][ox], gb[oy][ox], bb[oy][ox]));
            }
        // Zero-instruction fence (k_yuv_vec's): keeps hipcc from hoisting the coordinates and taps of every union block of the
        // thread to the top; with it the blocks are emitted one after the other.
#pragma unroll
        for (int dy = 0; dy < BH; dy++) {
#pragma unroll
            for (int k = 0; k < YWI; k++) asm volatile("" : "+v"(yw[dy][k]));
#pragma unroll
            for (int k = 0; k < YWA; k++) asm volatile("" : "+v"(ya[dy][k]));
#pragma unroll
            for (int k = 0; k < YWB; k++) asm volatile("" : "+v"(yb[dy][k]));
#pragma unroll
            for (int k = 0; k < CWA; k++) asm volatile("" : "+v"(cba[dy][k]), "+v"(cra[dy][k]));
        }
#pragma unroll
        for (int iy = 0; iy < IRH; iy++)
#pragma unroll
            for (int k = 0; k < CWI; k++) asm volatile("" : "+v"(cbw[iy][k]), "+v"(crw[iy][k]));
#pragma unroll
        for (int oy = 0; oy < BRH; oy++)
#pragma unroll
            for (int k = 0; k < CWB; k++) asm volatile("" : "+v"(cbb[oy][k]), "+v"(crb[oy][k]));
    }
#pragma unroll
    for (int dy = 0; dy < BH; dy++) {
        const long long y = (long long)(y0 + dy);
        st_words<YWA>(P.d[0] + fr * P.dfs[0] + y * P.ds[0] + (long long)xu * (YWA * 4), ya[dy]);
        st_words<CWA>(P.d[1] + fr * P.dfs[1] + y * P.ds[1] + (long long)xu * (CWA * 4), cba[dy]);
        st_words<CWA>(P.d[2] + fr * P.dfs[2] + y * P.ds[2] + (long long)xu * (CWA * 4), cra[dy]);
        st_words<YWB>(B.d[0] + fr * B.dfs[0] + y * B.ds[0] + (long long)xu * (YWB * 4), yb[dy]);
    }
#pragma unroll
    for (int oy = 0; oy < BRH; oy++) {
        const long long r = (long long)((y0 >> BCSY) + oy);
        st_words<CWB>(B.d[1] + fr * B.dfs[1] + r * B.ds[1] + (long long)xu * (CWB * 4), cbb[oy]);
        st_words<CWB>(B.d[2] + fr * B.dfs[2] + r * B.ds[2] + (long long)xu * (CWB * 4), crb[oy]);
    }
}

#define DU_TAG LUTR_CAT(LUTR_CAT(LUTR_CAT(w, LUTR_DU_WI), LUTR_DU_WA), LUTR_DU_WB)
// The vector kernels of this translation unit's container mix; the layout checks are the caller's (launch_yuv_dual).
const char *LUTR_CAT(launch_yuv_dual_vec_, DU_TAG)(hipStream_t st, const LutConsts &L, const YuvConsts &KA, const YuvConsts &KB,
                                                   const PlaneSet &P, const DstPlanes &B, const FrameGeom &G, int icsx, int icsy,
                                                   int bcsx, int bcsy, int mode)
{
    constexpr int WI = LUTR_DU_WI, WA = LUTR_DU_WA, WB = LUTR_DU_WB;
    constexpr int PXT = dual_pxt(WI, WA, WB);
    const int bh = 1 << cmax(icsy, bcsy);
    const long long units = (long long)(G.w / PXT) * (G.rows / bh) * G.nframes;
    const dim3 grid((unsigned)((units + 255) / 256)), block(256);
#define DU_CASE(IX, IY, BX, BY, I) \
    if (icsx == IX && icsy == IY && bcsx == BX && bcsy == BY && mode == I) { \
        hipLaunchKernelGGL((k_yuv_dual_vec<WI, WA, WB, IX, IY, BX, BY, I>), grid, block, 0, st, L, KA, KB, P, B, G); \
        return "k_yuv_dual_vec<" LUTR_STR(LUTR_DU_WI) "," LUTR_STR(LUTR_DU_WA) "," LUTR_STR(LUTR_DU_WB) "," #IX "," #IY "," #BX \
               "," #BY "," #I ">"; \
    }
#define DU_PAIR(IX, IY, BX, BY) DU_CASE(IX, IY, BX, BY, 0) DU_CASE(IX, IY, BX, BY, 1) DU_CASE(IX, IY, BX, BY, 2)
#define DU_IN(IX, IY) DU_PAIR(IX, IY, 1, 1) DU_PAIR(IX, IY, 1, 0) DU_PAIR(IX, IY, 0, 0)
    DU_IN(1, 1) DU_IN(1, 0) DU_IN(0, 0)
#undef DU_IN
#undef DU_PAIR
#undef DU_CASE
    return nullptr;
}

#else  // !LUTR_DU_WI
// ================================================================= generic kernel
// One thread per union block (at most 2 x 2 luma samples); any depth, stride or alignment, odd sizes, all five modes.  The block's
// pixels are evaluated once and their RGB kept in registers; both outputs are formed from them.  A pixel outside the frame is
// the edge pixel again (its luma and its chroma), so a partial output block sums the edge column / row twice, like
// np.pad(mode="edge"); only pixels and chroma samples inside the planes are written.
struct DualSide {
    uint8_t *d[3];
    long long ds[3], dfs[3];
    int csx, csy, wide;
};

__device__ __forceinline__ uint8_t *side_row(const DualSide &S, int c, long long fr, int y)
{
    return S.d[c] + fr * S.dfs[c] + (long long)y * S.ds[c];
}

// one output of a union block at (x0, y0), bw x bh luma samples, from its pixels o[dy][dx] (every index below is a compile-time
// constant after unrolling; what the run-time layout leaves out is predicated off)
__device__ __forceinline__ void dual_side_out(const YuvConsts &K, const DualSide &S, const FrameGeom &G, long long fr, int x0, int y0,
                                              int bw, int bh, const Rgb (&o)[2][2])
{
    const int cwo = (G.w + (1 << S.csx) - 1) >> S.csx, cho = (G.h + (1 << S.csy) - 1) >> S.csy;
#pragma unroll
    for (int dy = 0; dy < 2; dy++)
#pragma unroll
        for (int dx = 0; dx < 2; dx++)
            if (dy < bh && dx < bw && y0 + dy < G.h && x0 + dx < G.w)
                st_sample(side_row(S, 0, fr, y0 + dy), x0 + dx, S.wide, rgb_to_y(K, o[dy][dx]));
    // output chroma block (oy, ox) of the union block: the pixels with (dy >> csy, dx >> csx) == (oy, ox)
#pragma unroll
    for (int oy = 0; oy < 2; oy++)
#pragma unroll
        for (int ox = 0; ox < 2; ox++) {
            if ((oy << S.csy) >= bh || (ox << S.csx) >= bw) continue;
            float rs = 0.f, gs = 0.f, bs = 0.f;
#pragma unroll
            for (int dy = 0; dy < 2; dy++)
#pragma unroll
                for (int dx = 0; dx < 2; dx++)
                    if (dy < bh && dx < bw && (dy >> S.csy) == oy && (dx >> S.csx) == ox) {
                        rs += o[dy][dx].r; gs += o[dy][dx].g; bs += o[dy][dx].b;
                    }
            const int cx = (x0 >> S.csx) + ox, cy = (y0 >> S.csy) + oy;
            if (cx < cwo && cy < cho) {
                st_sample(side_row(S, 1, fr, cy), cx, S.wide, rgb_to_cb(K, rs, gs, bs));
                st_sample(side_row(S, 2, fr, cy), cx, S.wide, rgb_to_cr(K, rs, gs, bs));
            }
        }
}

__global__ __launch_bounds__(256) void k_yuv_dual_generic(LutConsts L, YuvConsts K1, YuvConsts K2, PlaneSet P, DstPlanes B, FrameGeom G,
                                                          int win, int icsx, int icsy, int w1, int csx1, int csy1, int w2,
                                                          int csx2, int csy2, int mode)
{
    const GFetch f(L);
    const int csx = cmax(icsx, cmax(csx1, csx2)), csy = cmax(icsy, cmax(csy1, csy2));
    const int bw = 1 << csx, bh = 1 << csy;
    DualSide S1, S2;
    for (int c = 0; c < 3; c++) {
        S1.d[c] = P.d[c]; S1.ds[c] = P.ds[c]; S1.dfs[c] = P.dfs[c];
        S2.d[c] = B.d[c]; S2.ds[c] = B.ds[c]; S2.dfs[c] = B.dfs[c];
    }
    S1.csx = csx1; S1.csy = csy1; S1.wide = w1;
    S2.csx = csx2; S2.csy = csy2; S2.wide = w2;
    for_each_block(G, csx, csy, false, [&](long long fr, int ux, int uy) {
        const int x0 = ux * bw, y0 = uy * bh;
        Rgb o[2][2];
#pragma unroll
        for (int dy = 0; dy < 2; dy++)
#pragma unroll
            for (int dx = 0; dx < 2; dx++) {
                if (dy >= bh || dx >= bw) { o[dy][dx] = Rgb{0.f, 0.f, 0.f}; continue; }
                const int y = y0 + dy < G.h ? y0 + dy : G.h - 1, x = x0 + dx < G.w ? x0 + dx : G.w - 1;
                const float cbv = ld_sample(src_row(P, 1, fr, y >> icsy), x >> icsx, win);
                const float crv = ld_sample(src_row(P, 2, fr, y >> icsy), x >> icsx, win);
                const Rgb q = yuv_to_rgb(K1, ld_sample(src_row(P, 0, fr, y), x, win), chroma_terms(K1, cbv, crv));
                o[dy][dx] = lut3d_px_rt(mode, L, f, q.r, q.g, q.b);
            }
        dual_side_out(K1, S1, G, fr, x0, y0, bw, bh, o);
        dual_side_out(K2, S2, G, fr, x0, y0, bw, bh, o);
    });
}

// ================================================================= launcher
const char *launch_yuv_dual(hipStream_t st, int variant, const LutConsts &L, const YuvConsts &K1, const YuvConsts &K2,
                            const PlaneSet &P, const DstPlanes &D2, const FrameGeom &G, int din, int dout1, int csx1, int csy1,
                            int dout2, int csx2, int csy2, int icsx, int icsy, int mode)
{
    const int win = din > 8, w1 = dout1 > 8, w2 = dout2 > 8;
    const int csx = cmax(icsx, cmax(csx1, csx2)), csy = cmax(icsy, cmax(csy1, csy2)), bh = 1 << csy;
    const bool batch = G.nframes > 1;
    // The vector kernels' output A is 4:2:2 in the wider container; the mixes built are 16 -> 16+16, 16 -> 16+8 and 8 -> 8+8.
    // swap: the second output takes A's role.
    auto mix_ok = [&](int wa, int wb) { return win ? (wa == 1) : (wa == 0 && wb == 0); };
    const bool a1 = csx1 == 1 && csy1 == 0 && mix_ok(w1, w2), a2 = csx2 == 1 && csy2 == 0 && mix_ok(w2, w1);
    const bool swap = !a1 && a2;
    const int wa = swap ? w2 : w1, wb = swap ? w1 : w2, bcsx = swap ? csx1 : csx2, bcsy = swap ? csy1 : csy2;
    const int pxt = dual_pxt(win, wa, wb);
    const long long bsi = win ? 2 : 1, bs1 = w1 ? 2 : 1, bs2 = w2 ? 2 : 1;
    struct Both { PlaneSet P; DstPlanes B; };
    const Both PB{P, D2};
    auto vec_fits = [&](const Both &Q, const FrameGeom &H) {
        if (!(a1 || a2) || !vec_mode(mode)) return false;
        if (H.w % pxt || H.row0 % bh || H.rows % bh) return false;
        if (!units_fit((long long)(H.w / pxt) * (H.rows / bh) * H.nframes)) return false;
        if (!plane_ok(Q.P.s[0], Q.P.ss[0], Q.P.sfs[0], pxt * bsi, batch, kStrideAny, false) ||
            !plane_ok(Q.P.d[0], Q.P.ds[0], Q.P.dfs[0], pxt * bs1, batch, kStrideAny, false) ||
            !plane_ok(Q.B.d[0], Q.B.ds[0], Q.B.dfs[0], pxt * bs2, batch, kStrideAny, false))
            return false;
        for (int c = 1; c < 3; c++)
            if (!plane_ok(Q.P.s[c], Q.P.ss[c], Q.P.sfs[c], (pxt >> icsx) * bsi, batch, kStrideAny, false) ||
                !plane_ok(Q.P.d[c], Q.P.ds[c], Q.P.dfs[c], (pxt >> csx1) * bs1, batch, kStrideAny, false) ||
                !plane_ok(Q.B.d[c], Q.B.ds[c], Q.B.dfs[c], (pxt >> csx2) * bs2, batch, kStrideAny, false))
                return false;
        return true;
    };
    auto vec = [&](const Both &Q, const FrameGeom &H) -> const char * {
        PlaneSet A = Q.P;
        DstPlanes Bd = Q.B;
        if (swap)
            for (int c = 0; c < 3; c++) {
                A.d[c] = Q.B.d[c]; A.ds[c] = Q.B.ds[c]; A.dfs[c] = Q.B.dfs[c];
                Bd.d[c] = Q.P.d[c]; Bd.ds[c] = Q.P.ds[c]; Bd.dfs[c] = Q.P.dfs[c];
            }
        const YuvConsts &KA = swap ? K2 : K1, &KB = swap ? K1 : K2;
        if (win && wb) return launch_yuv_dual_vec_w111(st, L, KA, KB, A, Bd, H, icsx, icsy, bcsx, bcsy, mode);
        if (win) return launch_yuv_dual_vec_w110(st, L, KA, KB, A, Bd, H, icsx, icsy, bcsx, bcsy, mode);
        return launch_yuv_dual_vec_w000(st, L, KA, KB, A, Bd, H, icsx, icsy, bcsx, bcsy, mode);
    };
    auto generic = [&](const Both &Q, const FrameGeom &H) {
        hipLaunchKernelGGL(k_yuv_dual_generic, dim3(block_grid("k_yuv_dual_generic", H.w, H.rows, H.nframes, csx, csy)), dim3(256), 0, st, L, K1,
                           K2, Q.P,
                           Q.B, H, win, icsx, icsy, w1, csx1, csy1, w2, csx2, csy2, mode);
        return "k_yuv_dual_generic";
    };
    // (no LDS-window kernel for this path; the unit is 4 or 8 luma samples wide, whole union blocks)
    return launch_vec_or_generic(variant, PB, G, pxt, vec_fits, vec, generic, [&](int wv) {
        Both T{advance_planes(P, wv * bsi, (wv >> icsx) * bsi, wv * bs1, (wv >> csx1) * bs1), D2};
        for (int c = 0; c < 3; c++) T.B.d[c] += c ? (wv >> csx2) * bs2 : wv * bs2;
        return T;
    });
}
#endif  // LUTR_DU_WI

}  // namespace lutr
