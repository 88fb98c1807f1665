// lutr_xsub.hip -- gfx950 kernels of the fused YUV pass with a chroma subsampling change.
//
// What they replace: the `format=<pix_fmt>` at the end of the reference's filter chain when the pixel format it picks
// has another subsampling than the source (ffmpeg.py:304-310; the ProRes 422 HQ master of ffmpeg.py:417-433 on a 4:2:0
// source, force_8bit's yuv420p on a 4:2:2 / 4:4:4 source).  The contract is 3.2's with the two chroma stages split:
//   up-sampling    each source chroma sample is replicated over its INPUT block (x >> icsx, y >> icsy)
//   down-sampling  each output chroma sample is the mean of the LUT's integer RGB over its OUTPUT block (1/n in cbr..crb,
//                  n = 2^(ocsx + ocsy); a partial block at an odd edge takes the edge column / row again)
// The unit of work is the union block, 2^max(icsx, ocsx) x 2^max(icsy, ocsy) luma samples: it holds whole input and whole
// output chroma blocks.
//
// One source, two kinds of translation unit (Makefile MIX_RULE):
//   without LUTR_XS_WI   the generic kernel, the unquantised pass of the dither path and the launcher
//   LUTR_XS_WI / _WO     the vector kernels of one container mix (8 -> 8, 16 -> 16, 16 -> 8): 6 layout pairs x 3 modes
#include "lutr_device.h"
#include "lutr_launch.h"

namespace lutr {

#ifdef LUTR_XS_WI
// ================================================================= vector kernel, global gather
// k_yuv_vec's structure (lutr_kernels.hip): whole-word loads and stores, VB bytes of luma per thread and row, BH luma rows per
// thread, lattice taps gathered from L1/L2.  The thread's input chroma rows (BH >> ICSY) and output chroma rows (BH >> OCSY)
// are separate arrays; the thread walks its union blocks one after the other.  (Frame written out: see k_yuv_vec.)
template <int WIN, int WOUT, int ICSX, int ICSY, int OCSX, int OCSY, int INTERP>
__global__ __launch_bounds__(256) void k_yuv_xsub_vec(LutConsts L, YuvConsts K, PlaneSet P, FrameGeom G)
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
    const GFetch f(L);
    const unsigned uw = (unsigned)G.w / PXT;
    const unsigned ub = (unsigned)G.rows >> CSY;
    const unsigned total = uw * ub * (unsigned)G.nframes;
    const unsigned u = blockIdx.x * 256u + threadIdx.x;
    if (u >= total) return;
    const unsigned xu = u % uw, t = u / uw;
    const int y0 = ((G.row0 >> CSY) + (int)(t % ub)) * BH;        // first luma row of the thread
    const long long fr = t / ub;
    const long long xi = (long long)xu * VB, xo = (long long)xu * (YWO * 4), cxi = (long long)xu * (CWI * 4),
                    cxo = (long long)xu * (CWO * 4);

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
        ld_words<CWI>(cbw[iy], P.s[1] + fr * P.sfs[1] + r * P.ss[1] + cxi);
        ld_words<CWI>(crw[iy], P.s[2] + fr * P.sfs[2] + r * P.ss[2] + cxi);
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
                c[iy][ix] = chroma_terms(K, word_sample<WIN>(cbw[iy], j * IBX + ix), word_sample<WIN>(crw[iy], j * IBX + ix));
        float rs[ORH][OBX], gs[ORH][OBX], bs[ORH][OBX];
#pragma unroll
        for (int oy = 0; oy < ORH; oy++)
#pragma unroll
            for (int ox = 0; ox < OBX; ox++) { rs[oy][ox] = 0.f; gs[oy][ox] = 0.f; bs[oy][ox] = 0.f; }
#pragma unroll
        for (int dy = 0; dy < BH; dy++) {
#pragma unroll
            for (int dx = 0; dx < BW; dx++) {
                const int i = j * BW + dx;
                const Rgb q = yuv_to_rgb(K, word_sample<WIN>(yw[dy], i), c[dy >> ICSY][dx >> ICSX]);
                const Rgb o = lut3d_px<INTERP>(L, f, q.r, q.g, q.b);
                rs[dy >> OCSY][dx >> OCSX] += o.r; gs[dy >> OCSY][dx >> OCSX] += o.g; bs[dy >> OCSY][dx >> OCSX] += o.b;
                word_put<WOUT>(yo[dy], i, rgb_to_y(K, o));
            }
        }
#pragma unroll
        for (int oy = 0; oy < ORH; oy++)
#pragma unroll
            for (int ox = 0; ox < OBX; ox++) {
                word_put<WOUT>(cbo[oy], j * OBX + ox, rgb_to_cb(K, rs[oy][ox], gs[oy][ox], bs[oy][ox]));
                word_put<WOUT>(cro[oy], j * OBX + ox, rgb_to_cr(K, rs[oy][ox], gs[oy][ox], bs[oy][ox]));
            }
        // Zero-instruction fence (k_yuv_vec's): keeps hipcc from hoisting the coordinates and taps of every union block of the
        // thread to the top; with it the blocks are emitted one after the other.
#pragma unroll
        for (int dy = 0; dy < BH; dy++) {
#pragma unroll
            for (int k = 0; k < YWI; k++) asm volatile("" : "+v"(yw[dy][k]));
#pragma unroll
            for (int k = 0; k < YWO; k++) asm volatile("" : "+v"(yo[dy][k]));
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
#pragma unroll
    for (int dy = 0; dy < BH; dy++)
        st_words<YWO>(P.d[0] + fr * P.dfs[0] + (long long)(y0 + dy) * P.ds[0] + xo, yo[dy]);
#pragma unroll
    for (int oy = 0; oy < ORH; oy++) {
        const long long r = (long long)((y0 >> OCSY) + oy);
        st_words<CWO>(P.d[1] + fr * P.dfs[1] + r * P.ds[1] + cxo, cbo[oy]);
        st_words<CWO>(P.d[2] + fr * P.dfs[2] + r * P.ds[2] + cxo, cro[oy]);
    }
}

// The vector kernels of this translation unit's container mix; the layout checks are the caller's (launch_yuv_xsub).
const char *LUTR_CAT(LUTR_CAT(launch_yuv_xsub_vec_w, LUTR_XS_WI), LUTR_XS_WO)(hipStream_t st, const LutConsts &L, const YuvConsts &K,
                                                                               const PlaneSet &P, const FrameGeom &G, int icsx,
                                                                               int icsy, int ocsx, int ocsy, int mode)
{
    constexpr int WI = LUTR_XS_WI, WO = LUTR_XS_WO;
    constexpr int PXT = vec_bytes<WI, WO>() / (WI ? 2 : 1);
    const int bh = 1 << cmax(icsy, ocsy);
    const long long units = (long long)(G.w / PXT) * (G.rows / bh) * G.nframes;
    const dim3 grid((unsigned)((units + 255) / 256)), block(256);
#define XS_CASE(IX, IY, OX, OY, I) \
    if (icsx == IX && icsy == IY && ocsx == OX && ocsy == OY && mode == I) { \
        hipLaunchKernelGGL((k_yuv_xsub_vec<WI, WO, IX, IY, OX, OY, I>), grid, block, 0, st, L, K, P, G); \
        return "k_yuv_xsub_vec<" LUTR_STR(LUTR_XS_WI) "," LUTR_STR(LUTR_XS_WO) "," #IX "," #IY "," #OX "," #OY "," #I ">"; \
    }
#define XS_PAIR(IX, IY, OX, OY) XS_CASE(IX, IY, OX, OY, 0) XS_CASE(IX, IY, OX, OY, 1) XS_CASE(IX, IY, OX, OY, 2)
    XS_PAIR(1, 1, 1, 0) XS_PAIR(1, 1, 0, 0)
    XS_PAIR(1, 0, 1, 1) XS_PAIR(1, 0, 0, 0)
    XS_PAIR(0, 0, 1, 1) XS_PAIR(0, 0, 1, 0)
#undef XS_PAIR
#undef XS_CASE
    return nullptr;
}

#else  // !LUTR_XS_WI
// ================================================================= generic kernels
// One thread per union block; any depth, stride or alignment, odd sizes, all five modes.  The block is walked one OUTPUT
// chroma block at a time (its sum is then one set of three accumulators); every pixel reads the input chroma sample of its
// own input block.  A pixel outside the frame is the edge pixel again (its luma and its chroma), so a partial output block
// sums the edge column / row twice, like np.pad(mode="edge"); only pixels and chroma samples inside the planes are written.
template <class Sink>
__device__ __forceinline__ void xsub_union_block(const LutConsts &L, const GFetch &f, const YuvConsts &K, const PlaneSet &P,
                                                 const FrameGeom &G, long long fr, int ux, int uy, int win, int icsx, int icsy,
                                                 int ocsx, int ocsy, int mode, Sink &sink)
{
    const int bw = 1 << cmax(icsx, ocsx), bh = 1 << cmax(icsy, ocsy), obw = 1 << ocsx, obh = 1 << ocsy;
    const int cwo = (G.w + obw - 1) >> ocsx, cho = (G.h + obh - 1) >> ocsy;
    for (int oy = 0; oy < bh; oy += obh) {
        for (int ox = 0; ox < bw; ox += obw) {
            float rs = 0.f, gs = 0.f, bs = 0.f;
            for (int dy = 0; dy < obh; dy++) {
                const int yy = uy * bh + oy + dy;
                const int y = yy < G.h ? yy : G.h - 1;
                for (int dx = 0; dx < obw; dx++) {
                    const int xx = ux * bw + ox + dx;
                    const int x = xx < G.w ? xx : G.w - 1;
                    const float cbv = ld_sample(src_row(P, 1, fr, y >> icsy), x >> icsx, win);
                    const float crv = ld_sample(src_row(P, 2, fr, y >> icsy), x >> icsx, win);
                    const float yv = ld_sample(src_row(P, 0, fr, y), x, win);
                    const Rgb q = yuv_to_rgb(K, yv, chroma_terms(K, cbv, crv));
                    const Rgb o = lut3d_px_rt(mode, L, f, q.r, q.g, q.b);
                    rs += o.r; gs += o.g; bs += o.b;
                    if (yy < G.h && xx < G.w) sink.luma(fr, x, y, o);
                }
            }
            const int ocx = (ux * bw + ox) >> ocsx, ocy = (uy * bh + oy) >> ocsy;
            if (ocx < cwo && ocy < cho) sink.chroma(fr, ocx, ocy, rs, gs, bs);
        }
    }
}

// (the walk over union blocks and the sinks: lutr_device.h)
__global__ __launch_bounds__(256) void k_yuv_xsub_generic(LutConsts L, YuvConsts K, PlaneSet P, FrameGeom G, int win, int wout,
                                                          int icsx, int icsy, int ocsx, int ocsy, int mode)
{
    const GFetch f(L);
    PlaneSink sink{K, P, wout};
    for_each_block(G, cmax(icsx, ocsx), cmax(icsy, ocsy), false, [&](long long fr, int ux, int uy) {
        xsub_union_block(L, f, K, P, G, fr, ux, uy, win, icsx, icsy, ocsx, ocsy, mode, sink);
    });
}

// the dither path's pass 1 (k_yuv_float's values, lutr_dither.hip): whole frames, chroma planes in the output layout
__global__ __launch_bounds__(256) void k_yuv_float_xsub(LutConsts L, YuvConsts K, PlaneSet P, FrameGeom G, FloatPlanes F, int win,
                                                        int icsx, int icsy, int ocsx, int ocsy, int mode)
{
    const GFetch f(L);
    FloatSink sink(K, F, G, ocsx, ocsy);
    for_each_block(G, cmax(icsx, ocsx), cmax(icsy, ocsy), true, [&](long long fr, int ux, int uy) {
        xsub_union_block(L, f, K, P, G, fr, ux, uy, win, icsx, icsy, ocsx, ocsy, mode, sink);
    });
}

void launch_yuv_float_xsub(hipStream_t st, const LutConsts &L, const YuvConsts &K, const PlaneSet &P, const FrameGeom &G,
                           const FloatPlanes &F, int win, int icsx, int icsy, int ocsx, int ocsy, int mode)
{
    hipLaunchKernelGGL(k_yuv_float_xsub, dim3(block_grid(G.w, G.h, G.nframes, cmax(icsx, ocsx), cmax(icsy, ocsy))), dim3(256), 0, st,
                       L, K, P, G, F, win, icsx, icsy, ocsx, ocsy, mode);
}

// ================================================================= launcher
const char *launch_yuv_xsub(hipStream_t st, int variant, const LutConsts &L, const YuvConsts &K, const PlaneSet &P,
                            const FrameGeom &G, int din, int dout, int icsx, int icsy, int ocsx, int ocsy, int mode)
{
    const int win = din > 8, wout = dout > 8;
    const int csx = cmax(icsx, ocsx), csy = cmax(icsy, ocsy), bh = 1 << csy;
    // the vector kernels' unit: 8 bytes of luma per row (16 for a 16-bit source written as 8 bit); 8 -> 16 bit has none
    const bool mix_ok = win == wout || (win && !wout);
    const int pxt = (win && !wout) ? 8 : (win ? 4 : 8);
    const long long bsi = win ? 2 : 1, bso = wout ? 2 : 1;
    const bool batch = G.nframes > 1;
    auto vec_fits = [&](const PlaneSet &Q, const FrameGeom &H) {
        if (!mix_ok || !vec_mode(mode)) return false;
        if (H.w % pxt || H.row0 % bh || H.rows % bh) return false;
        if (!units_fit((long long)(H.w / pxt) * (H.rows / bh) * H.nframes)) return false;
        if (!plane_ok(Q.s[0], Q.ss[0], Q.sfs[0], pxt * bsi, batch, kStrideAny, false) || !plane_ok(Q.d[0], Q.ds[0], Q.dfs[0], pxt * bso, batch, kStrideAny, false))
            return false;
        for (int c = 1; c < 3; c++)
            if (!plane_ok(Q.s[c], Q.ss[c], Q.sfs[c], (pxt >> icsx) * bsi, batch, kStrideAny, false) ||
                !plane_ok(Q.d[c], Q.ds[c], Q.dfs[c], (pxt >> ocsx) * bso, batch, kStrideAny, false))
                return false;
        return true;
    };
    auto vec = [&](const PlaneSet &Q, const FrameGeom &H) -> const char * {
        if (win && wout) return launch_yuv_xsub_vec_w11(st, L, K, Q, H, icsx, icsy, ocsx, ocsy, mode);
        if (win) return launch_yuv_xsub_vec_w10(st, L, K, Q, H, icsx, icsy, ocsx, ocsy, mode);
        return launch_yuv_xsub_vec_w00(st, L, K, Q, H, icsx, icsy, ocsx, ocsy, mode);
    };
    auto generic = [&](const PlaneSet &Q, const FrameGeom &H) {
        hipLaunchKernelGGL(k_yuv_xsub_generic, dim3(block_grid(H.w, H.rows, H.nframes, csx, csy)), dim3(256), 0, st, L, K, Q, H, win,
                           wout, icsx, icsy, ocsx, ocsy, mode);
        return "k_yuv_xsub_generic";
    };
    // (no LDS-window kernel for a subsampling change; the unit is 4, 8 or 16 luma samples wide, whole union blocks)
    return launch_vec_or_generic(variant, P, G, pxt, vec_fits, vec, generic, [&](int wv) {
        return advance_planes(P, wv * bsi, (wv >> icsx) * bsi, wv * bso, (wv >> ocsx) * bso);
    });
}
#endif  // LUTR_XS_WI

}  // namespace lutr
