// lutr_bnd.hip -- gfx950 kernels of the fused YUV pass with blue-noise dither in its output stage.
//
// A threshold dither: every output sample is quantised as clip(floor(c + d)) where c is the value the output stage hands to
// clip_floor without dither (3.2's fma chain, 0.5 included) and d in (-0.5, 0.5) comes from a 64 x 64 void-and-cluster table by the
// sample's position in its plane.  No scratch, no coupling between rows or frames: row shards and batches give the bits of the
// whole call.  Everything ahead of the add is 3.8's contract (lutr_xsub.hip) for all nine layout pairs, the three equal ones
// included, in strict arithmetic.
//
// One source, two kinds of translation unit (Makefile MIX_RULE):
//   without LUTR_BN_WI   the generic kernel and the launcher
//   LUTR_BN_WI / _WO     the vector kernels of one container mix (8 -> 8, 16 -> 16, 16 -> 8): 9 layout pairs x 3 modes
#include "lutr_device.h"
#include "lutr_launch.h"

namespace lutr {

#ifdef LUTR_BN_WI
// ================================================================= vector kernel, global gather
// k_yuv_xsub_vec's body with the offsets (yuv_xsub_vec_body, lutr_device.h)
template <int WIN, int WOUT, int ICSX, int ICSY, int OCSX, int OCSY, int INTERP>
__global__ __launch_bounds__(256) void k_yuv_bn_vec(LutConsts L, YuvConsts K, PlaneSet P, FrameGeom G, const float *__restrict__ bn)
{
    yuv_xsub_vec_body<WIN, WOUT, ICSX, ICSY, OCSX, OCSY, INTERP, true>(L, K, P, G, bn);
}

// The vector kernels of this translation unit's container mix; the layout checks are the caller's (launch_yuv_bn).
const char *LUTR_CAT(LUTR_CAT(launch_yuv_bn_vec_w, LUTR_BN_WI), LUTR_BN_WO)(hipStream_t st, const LutConsts &L, const YuvConsts &K,
                                                                             const PlaneSet &P, const FrameGeom &G, const float *bn,
                                                                             int icsx, int icsy, int ocsx, int ocsy, int mode)
{
    constexpr int WI = LUTR_BN_WI, WO = LUTR_BN_WO;
    constexpr int PXT = vec_bytes<WI, WO>() / (WI ? 2 : 1);
    const int bh = 1 << cmax(icsy, ocsy);
    const long long units = (long long)(G.w / PXT) * (G.rows / bh) * G.nframes;
    const dim3 grid((unsigned)((units + 255) / 256)), block(256);
#define BN_CASE(IX, IY, OX, OY, I) \
    if (icsx == IX && icsy == IY && ocsx == OX && ocsy == OY && mode == I) { \
        hipLaunchKernelGGL((k_yuv_bn_vec<WI, WO, IX, IY, OX, OY, I>), grid, block, 0, st, L, K, P, G, bn); \
        return "k_yuv_bn_vec<" LUTR_STR(LUTR_BN_WI) "," LUTR_STR(LUTR_BN_WO) "," #IX "," #IY "," #OX "," #OY "," #I ">"; \
    }
#define BN_PAIR(IX, IY, OX, OY) BN_CASE(IX, IY, OX, OY, 0) BN_CASE(IX, IY, OX, OY, 1) BN_CASE(IX, IY, OX, OY, 2)
#define BN_FROM(IX, IY) BN_PAIR(IX, IY, 1, 1) BN_PAIR(IX, IY, 1, 0) BN_PAIR(IX, IY, 0, 0)
    BN_FROM(1, 1) BN_FROM(1, 0) BN_FROM(0, 0)
#undef BN_FROM
#undef BN_PAIR
#undef BN_CASE
    return nullptr;
}

#else  // !LUTR_BN_WI
// ================================================================= generic kernel
// k_yuv_xsub_generic's walk and block body (lutr_device.h) with a DitherSink: any depth, stride or alignment, odd sizes, all five
// modes, 8 -> 16 bit.  x0: the frame column of the planes' column 0 (a whole number of union blocks).
__global__ __launch_bounds__(256) void k_yuv_bn_generic(LutConsts L, YuvConsts K, PlaneSet P, FrameGeom G, const float *__restrict__ bn,
                                                        int x0, int win, int wout, int icsx, int icsy, int ocsx, int ocsy, int mode)
{
    const GFetch f(L);
    DitherSink sink{K, P, wout, bn, x0, x0 >> ocsx};
    for_each_block(G, cmax(icsx, ocsx), cmax(icsy, ocsy), false, [&](long long fr, int ux, int uy) {
        xsub_union_block(L, f, K, P, G, fr, ux, uy, win, icsx, icsy, ocsx, ocsy, mode, sink);
    });
}

// ================================================================= launcher
const char *launch_yuv_bn(hipStream_t st, int variant, const LutConsts &L, const YuvConsts &K, const PlaneSet &P, const FrameGeom &G,
                          const float *bn, int din, int dout, int icsx, int icsy, int ocsx, int ocsy, int mode)
{
    const int win = din > 8, wout = dout > 8;
    const int csx = cmax(icsx, ocsx), csy = cmax(icsy, ocsy), bh = 1 << csy;
    // k_yuv_xsub_vec's unit and conditions: 8 bytes of luma per row (16 for a 16-bit source written as 8 bit); 8 -> 16 bit has none
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
        if (win && wout) return launch_yuv_bn_vec_w11(st, L, K, Q, H, bn, icsx, icsy, ocsx, ocsy, mode);
        if (win) return launch_yuv_bn_vec_w10(st, L, K, Q, H, bn, icsx, icsy, ocsx, ocsy, mode);
        return launch_yuv_bn_vec_w00(st, L, K, Q, H, bn, icsx, icsy, ocsx, ocsy, mode);
    };
    // the pattern is anchored to the frame: the tail of a column split tells the generic kernel where its planes begin (tail(wv)
    // runs just ahead of the generic launch it feeds; every other launch starts at column 0)
    int x0 = 0;
    auto generic = [&](const PlaneSet &Q, const FrameGeom &H) {
        hipLaunchKernelGGL(k_yuv_bn_generic, dim3(block_grid("k_yuv_bn_generic", H.w, H.rows, H.nframes, csx, csy)), dim3(256), 0, st, L, K, Q, H,
                           bn, x0,
                           win, wout, icsx, icsy, ocsx, ocsy, mode);
        return "k_yuv_bn_generic";
    };
    return launch_vec_or_generic(variant, P, G, pxt, vec_fits, vec, generic, [&](int wv) {
        x0 = wv;
        return advance_planes(P, wv * bsi, (wv >> icsx) * bsi, wv * bso, (wv >> ocsx) * bso);
    });
}
#endif  // LUTR_BN_WI

}  // namespace lutr
