// lutr_cdl.hip -- gfx950 kernels of the fused YUV pass with an ASC CDL in front of lut3d.
//
// What they compute: the per-clip colour decision (slope, offset, power, saturation; ASC CDL v1.2) on the integer RGB the YUV ->
// RGB stage hands lut3d, then the shared show LUT, in one pass:
//   q   = YUV -> integer RGB at the LUT depth              (3.2; chroma replicated over its INPUT block)
//   T_c = tab[c][q_c]                                      (A: slope, offset, clamp and power folded per integer code on the host;
//                                                           no pow on the device)
//   o_c = med3(l + sat * (T_c - l), 0, 1)                  (B: l = (0.2126 T_R + 0.7152 T_G) + 0.0722 T_B; skipped when sat == 1)
//   v   = lut3d on the unit floats o, truncated and clipped to [0, M]   (C: 3.1 from the scale step on)
//   out = integer RGB -> YUV from v                        (3.2 / 3.8; chroma = mean over its OUTPUT block)
// The unit of work is 3.8's union block for every pair of layouts, the equal ones included.  The table is read from global memory
// through L1 like LutConsts::pre (12 KB at 10 bit, 768 KB at 16 bit).
//
// One source, two kinds of translation unit (Makefile MIX_RULE):
//   without LUTR_CD_WI   the generic kernel and the launcher
//   LUTR_CD_WI / _WO     the vector kernels of one container mix (8 -> 8, 16 -> 16, 16 -> 8): 9 layout pairs x 3 modes
#include <string>

#include "lutr_device.h"
#include "lutr_launch.h"

namespace lutr {

#ifdef LUTR_CD_WI
// ================================================================= vector kernel, global gather
// k_yuv_chain_vec's structure (lutr_chain.hip) with the table reads and the saturation mix in place of the first lattice: a pixel's
// three table reads are issued together, the lattice taps depend on them.
template <int WIN, int WOUT, int ICSX, int ICSY, int OCSX, int OCSY, int INTERP>
__global__ __launch_bounds__(256) void k_yuv_cdl_vec(LutConsts L, CdlConsts C, YuvConsts K, PlaneSet P, FrameGeom G)
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
    const bool mix = C.sat != 1.0f;                               // a kernel argument: the branch is wave-uniform

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
                const Rgb o = lut3d_unit<INTERP>(L, f, cdl_px(C, mix, q));
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

// The vector kernels of this translation unit's container mix; the layout checks are the caller's (launch_yuv_cdl).
const char *LUTR_CAT(LUTR_CAT(launch_yuv_cdl_vec_w, LUTR_CD_WI), LUTR_CD_WO)(hipStream_t st, const LutConsts &L, const CdlConsts &C,
                                                                              const YuvConsts &K, const PlaneSet &P,
                                                                              const FrameGeom &G, int icsx, int icsy, int ocsx,
                                                                              int ocsy, int mode)
{
    constexpr int WI = LUTR_CD_WI, WO = LUTR_CD_WO;
    constexpr int PXT = vec_bytes<WI, WO>() / (WI ? 2 : 1);
    const int bh = 1 << cmax(icsy, ocsy);
    const long long units = (long long)(G.w / PXT) * (G.rows / bh) * G.nframes;
    const dim3 grid((unsigned)((units + 255) / 256)), block(256);
#define CD_CASE(IX, IY, OX, OY, I) \
    if (icsx == IX && icsy == IY && ocsx == OX && ocsy == OY && mode == I) { \
        hipLaunchKernelGGL((k_yuv_cdl_vec<WI, WO, IX, IY, OX, OY, I>), grid, block, 0, st, L, C, K, P, G); \
        return "k_yuv_cdl_vec<" LUTR_STR(LUTR_CD_WI) "," LUTR_STR(LUTR_CD_WO) "," #IX "," #IY "," #OX "," #OY "," #I ">"; \
    }
#define CD_PAIR(IX, IY, OX, OY) CD_CASE(IX, IY, OX, OY, 0) CD_CASE(IX, IY, OX, OY, 1) CD_CASE(IX, IY, OX, OY, 2)
    CD_PAIR(1, 1, 1, 1) CD_PAIR(1, 1, 1, 0) CD_PAIR(1, 1, 0, 0)
    CD_PAIR(1, 0, 1, 1) CD_PAIR(1, 0, 1, 0) CD_PAIR(1, 0, 0, 0)
    CD_PAIR(0, 0, 1, 1) CD_PAIR(0, 0, 1, 0) CD_PAIR(0, 0, 0, 0)
#undef CD_PAIR
#undef CD_CASE
    return nullptr;
}

#else  // !LUTR_CD_WI
// ================================================================= generic kernel
// One thread per union block; any depth, stride or alignment, odd sizes, all five modes.  xsub_union_block's walk (lutr_device.h)
// with the CDL in front of the lattice: a pixel outside the frame is the edge pixel again, only pixels and chroma samples inside
// the planes are written.
__global__ __launch_bounds__(256) void k_yuv_cdl_generic(LutConsts L, CdlConsts C, YuvConsts K, PlaneSet P, FrameGeom G, int win,
                                                         int wout, int icsx, int icsy, int ocsx, int ocsy, int mode)
{
    const GFetch f(L);
    PlaneSink sink{K, P, wout};
    const bool mix = C.sat != 1.0f;
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
                        const Rgb o = lut3d_unit_rt(mode, L, f, cdl_px(C, mix, q));
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
const char *launch_yuv_cdl(hipStream_t st, int variant, const LutConsts &L, const CdlConsts &C, const YuvConsts &K, const PlaneSet &P,
                           const FrameGeom &G, int din, int dout, int icsx, int icsy, int ocsx, int ocsy, int mode)
{
    const int win = din > 8, wout = dout > 8;
    const int csx = cmax(icsx, ocsx), csy = cmax(icsy, ocsy), bh = 1 << csy;
    // the vector kernels' unit: 8 bytes of luma per row (16 for a 16-bit source written as 8 bit); 8 -> 16 bit has none
    const bool mix_ok = win == wout || (win && !wout);
    const int pxt = (win && !wout) ? 8 : (win ? 4 : 8);
    const long long bsi = win ? 2 : 1, bso = wout ? 2 : 1;
    const bool batch = G.nframes > 1;
    int ran = 0;                                 // bit 0: a vector kernel was launched, bit 1: the generic one
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
        ran |= 1;
        if (win && wout) return launch_yuv_cdl_vec_w11(st, L, C, K, Q, H, icsx, icsy, ocsx, ocsy, mode);
        if (win) return launch_yuv_cdl_vec_w10(st, L, C, K, Q, H, icsx, icsy, ocsx, ocsy, mode);
        return launch_yuv_cdl_vec_w00(st, L, C, K, Q, H, icsx, icsy, ocsx, ocsy, mode);
    };
    auto generic = [&](const PlaneSet &Q, const FrameGeom &H) {
        ran |= 2;
        hipLaunchKernelGGL(k_yuv_cdl_generic, dim3(block_grid("k_yuv_cdl_generic", H.w, H.rows, H.nframes, csx, csy)), dim3(256), 0, st, L, C, K, Q,
                           H, win,
                           wout, icsx, icsy, ocsx, ocsy, mode);
        return "k_yuv_cdl_generic";
    };
    const char *name = launch_vec_or_generic(variant, P, G, pxt, vec_fits, vec, generic, [&](int wv) {
        return advance_planes(P, wv * bsi, (wv >> icsx) * bsi, wv * bso, (wv >> ocsx) * bso);
    });
    if (!name || ran != 3) return name;
    // a ragged width split between the two kernels: both are named
    static thread_local std::string both;
    both = std::string(name) + "+k_yuv_cdl_generic";
    return both.c_str();
}
#endif  // LUTR_CD_WI

}  // namespace lutr
