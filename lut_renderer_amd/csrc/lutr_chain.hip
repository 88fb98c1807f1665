// lutr_chain.hip -- gfx950 kernels of the fused YUV pass with TWO lut3d stages.
//
// What they replace: `lut3d=file=A:interp=ia,lut3d=file=B:interp=ib,format=<pix_fmt>` -- a technical LUT followed by a creative
// look.  Both lut3d instances negotiate the same RGB format, so the frame stays integer RGB at the LUT depth between them:
//   q0  = YUV -> integer RGB at the LUT depth             (3.2; chroma replicated over its INPUT block)
//   q1  = lut3d_A(q0)   truncated and clipped to [0, M]   (3.1; A's prelut, if it has one)
//   q2  = lut3d_B(q1)   B's own size and scale; the codes q1 enter B exactly as source codes enter A
//   out = integer RGB -> YUV from q2                      (3.2 / 3.8; chroma = mean over its OUTPUT block)
// The unit of work is 3.8's union block for every pair of layouts, the equal ones included.
//
// One source, two kinds of translation unit (Makefile MIX_RULE):
//   without LUTR_CH_WI   the generic kernel and the launcher
//   LUTR_CH_WI / _WO     the vector kernels of one container mix (8 -> 8, 16 -> 16, 16 -> 8): 9 layout pairs x 3 modes
#include <string>

#include "lutr_device.h"
#include "lutr_launch.h"

namespace lutr {

#ifdef LUTR_CH_WI
// ================================================================= vector kernel, global gather
// yuv_xsub_vec_body's structure (lutr_device.h) without the dither offsets and with the second lattice behind the first.  The
// second gather's coordinates are computed from the first one's truncated codes, so its taps are fetched after the first one's
// have been blended: a pixel holds one set of taps at a time.  One template mode serves both stages.
template <int WIN, int WOUT, int ICSX, int ICSY, int OCSX, int OCSY, int INTERP>
__global__ __launch_bounds__(256) void k_yuv_chain_vec(LutConsts L, LutConsts L2, YuvConsts K, PlaneSet P, FrameGeom G)
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
    const GFetch f(L), f2(L2);
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
                const Rgb m = lut3d_px<INTERP>(L, f, q.r, q.g, q.b);
                const Rgb o = lut3d_px<INTERP>(L2, f2, m.r, m.g, m.b);
                rs[dy >> OCSY][dx >> OCSX] += o.r; gs[dy >> OCSY][dx >> OCSX] += o.g; bs[dy >> OCSY][dx >> OCSX] += o.b;
                word_put<WOUT>(yo[dy], i, rgb_to_y(K, o));
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

// The vector kernels of this translation unit's container mix; the layout checks are the caller's (launch_yuv_chain).
const char *LUTR_CAT(LUTR_CAT(launch_yuv_chain_vec_w, LUTR_CH_WI), LUTR_CH_WO)(hipStream_t st, const LutConsts &L, const LutConsts &L2,
                                                                                const YuvConsts &K, const PlaneSet &P,
                                                                                const FrameGeom &G, int icsx, int icsy, int ocsx,
                                                                                int ocsy, int mode)
{
    constexpr int WI = LUTR_CH_WI, WO = LUTR_CH_WO;
    constexpr int PXT = vec_bytes<WI, WO>() / (WI ? 2 : 1);
    const int bh = 1 << cmax(icsy, ocsy);
    const long long units = (long long)(G.w / PXT) * (G.rows / bh) * G.nframes;
    const dim3 grid((unsigned)((units + 255) / 256)), block(256);
#define CH_CASE(IX, IY, OX, OY, I) \
    if (icsx == IX && icsy == IY && ocsx == OX && ocsy == OY && mode == I) { \
        hipLaunchKernelGGL((k_yuv_chain_vec<WI, WO, IX, IY, OX, OY, I>), grid, block, 0, st, L, L2, K, P, G); \
        return "k_yuv_chain_vec<" LUTR_STR(LUTR_CH_WI) "," LUTR_STR(LUTR_CH_WO) "," #IX "," #IY "," #OX "," #OY "," #I ">"; \
    }
#define CH_PAIR(IX, IY, OX, OY) CH_CASE(IX, IY, OX, OY, 0) CH_CASE(IX, IY, OX, OY, 1) CH_CASE(IX, IY, OX, OY, 2)
    CH_PAIR(1, 1, 1, 1) CH_PAIR(1, 1, 1, 0) CH_PAIR(1, 1, 0, 0)
    CH_PAIR(1, 0, 1, 1) CH_PAIR(1, 0, 1, 0) CH_PAIR(1, 0, 0, 0)
    CH_PAIR(0, 0, 1, 1) CH_PAIR(0, 0, 1, 0) CH_PAIR(0, 0, 0, 0)
#undef CH_PAIR
#undef CH_CASE
    return nullptr;
}

#else  // !LUTR_CH_WI
// ================================================================= generic kernel
// One thread per union block; any depth, stride or alignment, odd sizes, all five modes on either stage.  xsub_union_block's walk
// (lutr_device.h) with the second lattice behind the first: a pixel outside the frame is the edge pixel again, only pixels and
// chroma samples inside the planes are written.
__global__ __launch_bounds__(256) void k_yuv_chain_generic(LutConsts L, LutConsts L2, YuvConsts K, PlaneSet P, FrameGeom G, int win,
                                                           int wout, int icsx, int icsy, int ocsx, int ocsy, int mode, int mode2)
{
    const GFetch f(L), f2(L2);
    PlaneSink sink{K, P, wout};
    const int csx = cmax(icsx, ocsx), csy = cmax(icsy, ocsy);
    const int bw = 1 << csx, bh = 1 << csy, obw = 1 << ocsx, obh = 1 << ocsy;
    const int cwo = (G.w + obw - 1) >> ocsx, cho = (G.h + obh - 1) >> ocsy;
    for_each_block(G, csx, csy, false, [&](long long fr, int ux, int uy) {
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
                        const Rgb m = lut3d_px_rt(mode, L, f, q.r, q.g, q.b);
                        const Rgb o = lut3d_px_rt(mode2, L2, f2, m.r, m.g, m.b);
                        rs += o.r; gs += o.g; bs += o.b;
                        if (yy < G.h && xx < G.w) sink.luma(fr, x, y, o);
                    }
                }
                const int ocx = (ux * bw + ox) >> ocsx, ocy = (uy * bh + oy) >> ocsy;
                if (ocx < cwo && ocy < cho) sink.chroma(fr, ocx, ocy, rs, gs, bs);
            }
        }
    });
}

// ================================================================= launcher
const char *launch_yuv_chain(hipStream_t st, int variant, const LutConsts &L, const LutConsts &L2, const YuvConsts &K,
                             const PlaneSet &P, const FrameGeom &G, int din, int dout, int icsx, int icsy, int ocsx, int ocsy,
                             int mode, int mode2)
{
    const int win = din > 8, wout = dout > 8;
    const int csx = cmax(icsx, ocsx), csy = cmax(icsy, ocsy), bh = 1 << csy;
    // the vector kernels' unit: 8 bytes of luma per row (16 for a 16-bit source written as 8 bit); 8 -> 16 bit has none, and
    // neither has a pair of different modes
    const bool mix_ok = win == wout || (win && !wout);
    const int pxt = (win && !wout) ? 8 : (win ? 4 : 8);
    const long long bsi = win ? 2 : 1, bso = wout ? 2 : 1;
    const bool batch = G.nframes > 1;
    int ran = 0;                                 // bit 0: a vector kernel was launched, bit 1: the generic one
    auto vec_fits = [&](const PlaneSet &Q, const FrameGeom &H) {
        if (!mix_ok || !vec_mode(mode) || mode2 != mode) return false;
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
        ran |= 1;
        if (win && wout) return launch_yuv_chain_vec_w11(st, L, L2, K, Q, H, icsx, icsy, ocsx, ocsy, mode);
        if (win) return launch_yuv_chain_vec_w10(st, L, L2, K, Q, H, icsx, icsy, ocsx, ocsy, mode);
        return launch_yuv_chain_vec_w00(st, L, L2, K, Q, H, icsx, icsy, ocsx, ocsy, mode);
    };
    auto generic = [&](const PlaneSet &Q, const FrameGeom &H) {
        ran |= 2;
        hipLaunchKernelGGL(k_yuv_chain_generic, dim3(block_grid("k_yuv_chain_generic", H.w, H.rows, H.nframes, csx, csy)), dim3(256), 0, st, L, L2,
                           K, Q, H,
                           win, wout, icsx, icsy, ocsx, ocsy, mode, mode2);
        return "k_yuv_chain_generic";
    };
    const char *name = launch_vec_or_generic(variant, P, G, pxt, vec_fits, vec, generic, [&](int wv) {
        return advance_planes(P, wv * bsi, (wv >> icsx) * bsi, wv * bso, (wv >> ocsx) * bso);
    });
    if (!name || ran != 3) return name;
    // a ragged width split between the two kernels: both are named
    static thread_local std::string both;
    both = std::string(name) + "+k_yuv_chain_generic";
    return both.c_str();
}
#endif  // LUTR_CH_WI

}  // namespace lutr
