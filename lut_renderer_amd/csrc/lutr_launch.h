// lutr_launch.h -- host-only helpers shared by the launchers in the .hip files: layout predicates, grid sizing, the
// small-job boundary, the LUTR_RGB2 policy and per-device facts.  No device code.
#pragma once

#include <climits>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <mutex>
#include <set>
#include <string>
#include <utility>

#include "lutr_internal.h"

// names and strings built from a translation unit's -D switches
#define LUTR_CAT2(a, b) a##b
#define LUTR_CAT(a, b) LUTR_CAT2(a, b)
#define LUTR_STR2(x) #x
#define LUTR_STR(x) LUTR_STR2(x)

namespace lutr {

// ---------------------------------------------------------------- plane alignment
// Stride caps of plane_ok.  The fast kernels address rows with 32-bit positive offsets; bottom-up (negative linesize) or huge
// strides go to the generic kernels, which do 64-bit signed arithmetic.
// the global-gather vector kernels of lutr_xsub.hip, lutr_rgb2yuv.hip, lutr_rgbf.hip, lutr_semi.hip and lutr_sited.hip: 64-bit row
// offsets, no cap
constexpr long long kStrideAny = LLONG_MAX;
// k_rgb_tile (lutr_tile.hip) and the k_rgb_vec / k_yuv_vec kernels routed with it: a tile kernel forms
// (row in tile) * stride + 16 * (unit in row) as one unsigned 32-bit offset with up to 31 rows and 63 units of 16 bytes
constexpr long long kStrideTile = (0xffffffffll - 64 * 16) / 32;
// k_yuv_tile2 (lutr_tile2.hip, Planes2's 32-bit strides) and the 16 -> 8 bit k_yuv_vec routed with it: the same offset with
// units of up to 32 bytes
constexpr long long kStrideTile2 = (0xffffffffll - 64 * 32) / 32;

// A plane a kernel can address with `a`-byte accesses: positive stride up to `stride_cap`, base, stride and (batches) frame
// stride aligned; fstride_nonneg also refuses a batch whose frames run backwards.  Every caller passes what its kernels need:
// the caps and the frame-stride test differ on purpose, they decide which kernel a layout is routed to.
inline bool plane_ok(const void *p, long long stride, long long fstride, long long a, bool batch, long long stride_cap,
                     bool fstride_nonneg)
{
    return stride > 0 && stride <= stride_cap && (uintptr_t)p % (uintptr_t)a == 0 && stride % a == 0 &&
           (!batch || ((!fstride_nonneg || fstride >= 0) && fstride % a == 0));
}

// source and destination plane `c` of P against the same unit
inline bool planes_ok(const PlaneSet &P, int c, long long a, bool batch, long long stride_cap, bool fstride_nonneg)
{
    return plane_ok(P.s[c], P.ss[c], P.sfs[c], a, batch, stride_cap, fstride_nonneg) &&
           plane_ok(P.d[c], P.ds[c], P.dfs[c], a, batch, stride_cap, fstride_nonneg);
}

// gbrp planes are (G, B, R); the tube kernels and the RGB -> YUV path take (R, G, B): slot k <- plane kGbrpToRgb[k]
constexpr int kGbrpToRgb[3] = {2, 0, 1};
inline PlaneSet gbrp_to_rgb(const PlaneSet &P)
{
    PlaneSet Q = P;
    for (int k = 0; k < 3; k++) {
        const int f = kGbrpToRgb[k];
        Q.s[k] = P.s[f]; Q.d[k] = P.d[f]; Q.ss[k] = P.ss[f]; Q.ds[k] = P.ds[f]; Q.sfs[k] = P.sfs[f]; Q.dfs[k] = P.dfs[f];
    }
    return Q;
}

// P moved right by s0 / d0 bytes on plane 0 and sc / dc bytes on planes 1 and 2: the planes of the tail of a column split (a plane
// a semi-planar side does not have stays null)
inline PlaneSet advance_planes(PlaneSet P, long long s0, long long sc, long long d0, long long dc)
{
    for (int c = 0; c < 3; c++) {
        if (P.s[c]) P.s[c] += c ? sc : s0;
        if (P.d[c]) P.d[c] += c ? dc : d0;
    }
    return P;
}

// the modes the vector and tile kernels are instantiated for (the generic kernels have all five)
inline bool vec_mode(int mode)
{
    return mode == LUTR_INTERP_NEAREST || mode == LUTR_INTERP_TRILINEAR || mode == LUTR_INTERP_TETRAHEDRAL;
}

// ---------------------------------------------------------------- launch sizing
// Blocks of 256 threads for `units` work items, at least one.  Grid-stride kernels go through stride_grid (below), most with
// kGridStrideCap: enough blocks to fill 256 CUs x 8.
constexpr unsigned kGridStrideCap = 256 * 64;
inline unsigned grid_for(long long units, unsigned cap = 0x7fffffffu)
{
    long long b = (units + 255) / 256;
    if (b < 1) b = 1;
    if (b > (long long)cap) b = cap;
    return (unsigned)b;
}

// the one-thread-per-unit kernels index their units with 32 bits
inline bool units_fit(long long units) { return units < 0x7fffffffll; }

// LUTR_MAX_BLOCKS (tests and tools only): a cap on the workgroups of every grid-stride launch, so that a frame of a few thousand
// units runs each thread of a grid-stride kernel for several trips, the last of them partial, as a UHD frame does under the
// launchers' own caps.  `text` is the variable's value (or null), `cap` the launch site's own cap.  Accepted only as a plain
// positive decimal that fits a grid; the launch then gets min(cap, value) blocks.  Anything else leaves `cap`.
inline unsigned capped_blocks(const char *text, unsigned cap)
{
    if (!text || !*text) return cap;
    long long v = 0;
    for (const char *c = text; *c; c++) {
        if (*c < '0' || *c > '9') return cap;
        v = v * 10 + (*c - '0');
        if (v > 0x7fffffffll) return cap;
    }
    return v > 0 && v < (long long)cap ? (unsigned)v : cap;
}

// The grid of a grid-stride launch (a kernel that walks `for (u = blockIdx.x * 256 + threadIdx.x; u < units; u += gridDim.x *
// 256)`): grid_for under the site's cap and LUTR_MAX_BLOCKS.  Both variables are read once per process.  LUTR_DEBUG: one line
// per launch, `family` names the kernel.  Never for a one-thread-per-unit kernel: a cap would drop its work.
inline unsigned stride_grid(const char *family, long long units, unsigned cap)
{
    struct Env { const char *max_blocks; bool debug; };
    static const Env env = [] {
        static char text[32];
        const char *e = getenv("LUTR_MAX_BLOCKS");
        // a copy (a later setenv may move the value); a value too long for it is no valid grid either
        if (e) snprintf(text, sizeof text, "%s", strlen(e) < sizeof text ? e : "x");
        return Env{e ? text : nullptr, getenv("LUTR_DEBUG") != nullptr};
    }();
    const unsigned b = grid_for(units, capped_blocks(env.max_blocks, cap));
    if (env.debug) fprintf(stderr, "[lutr gs] %s units %lld blocks %u\n", family, units, b);
    return b;
}

// blocks of 2^cs samples that cover n samples, and the grid of a by-block generic kernel (one thread per 2^csx x 2^csy block,
// for_each_block's walk)
inline long long blocks(int n, int cs) { return (n + (1 << cs) - 1) >> cs; }
inline unsigned block_grid(const char *family, int w, int rows, int nframes, int csx, int csy)
{
    return stride_grid(family, blocks(w, csx) * blocks(rows, csy) * nframes, kGridStrideCap);
}

// The launch sequence of a path that has global-gather vector kernels and a generic kernel, no LDS kernel.  vec_fits(P, G): the
// vector kernels can take these planes and this geometry; vec / generic launch and return the kernel's name; tail(wv): the planes
// moved right by wv pixels.  A ragged width on aligned (padded) rows goes to the vector kernel up to the last whole unit of unit_px
// columns and to the generic kernel for the rest (the unit is a whole number of chroma blocks, so the split falls between two).
// Planes: PlaneSet, or whatever a path with more sides hands through to its own callbacks (lutr_dual.hip).
template <class Planes, class Fits, class Vec, class Generic, class Tail>
const char *launch_vec_or_generic(int variant, const Planes &P, const FrameGeom &G, int unit_px, Fits vec_fits, Vec vec,
                                  Generic generic, Tail tail)
{
    if (variant == VAR_VEC_LDS) return nullptr;
    if (variant == VAR_GENERIC) return generic(P, G);
    if (vec_fits(P, G)) return vec(P, G);
    if (variant == VAR_VEC_GLOBAL) return nullptr;
    const int wv = G.w / unit_px * unit_px;
    if (wv > 0 && wv < G.w) {
        FrameGeom Gv = G, Ge = G;
        Gv.w = wv;
        Ge.w = G.w - wv;
        if (vec_fits(P, Gv)) {
            const char *name = vec(P, Gv);
            generic(tail(wv), Ge);
            return name;
        }
    }
    return generic(P, G);
}

// ---------------------------------------------------------------- the paths that work by union blocks
// What the launchers of lutr_xsub.hip, lutr_bnd.hip, lutr_chain.hip, lutr_cdl.hip, lutr_l1d.hip and lutr_stack.hip share: the
// widths and the vector kernels' unit of a call, the plane checks of those kernels and the planes of a column split's tail.
struct UnionLaunch {
    int win, wout;             // 16-bit containers in / out
    int icsx, ocsx, csx, csy;  // the chroma shifts the checks need, and the union block's
    int bh, pxt;               // the unit: bh luma rows of pxt samples, 8 bytes of luma per row (16 for a 16-bit source written as 8 bit)
    long long bsi, bso;        // bytes per sample in / out
    bool mix_ok, batch;        // the container mix has vector kernels (8 -> 16 bit has none); more than one frame
    bool isemi, osemi;         // the side's chroma is ONE plane of (Cb, Cr) pairs in slot 1 (the stack's semi form)

    UnionLaunch(const FrameGeom &G, int din, int dout, int icsx_, int icsy, int ocsx_, int ocsy, bool isemi_ = false,
                bool osemi_ = false)
        : win(din > 8), wout(dout > 8), icsx(icsx_), ocsx(ocsx_), csx(icsx_ > ocsx_ ? icsx_ : ocsx_), csy(icsy > ocsy ? icsy : ocsy),
          bh(1 << csy), pxt((win && !wout) ? 8 : (win ? 4 : 8)), bsi(win ? 2 : 1), bso(wout ? 2 : 1),
          mix_ok(win == wout || (win && !wout)), batch(G.nframes > 1), isemi(isemi_), osemi(osemi_) {}

    // samples of a chroma plane that go with n luma samples of a row: a plane of pairs holds both components of every block
    long long chroma_in(long long n) const { return isemi ? n : n >> icsx; }
    long long chroma_out(long long n) const { return osemi ? n : n >> ocsx; }

    // whole units, 32-bit unit indices, and whole aligned words of every plane per thread
    bool fits(const PlaneSet &Q, const FrameGeom &H) const
    {
        if (!mix_ok) return false;
        if (H.w % pxt || H.row0 % bh || H.rows % bh) return false;
        if (!units_fit((long long)(H.w / pxt) * (H.rows / bh) * H.nframes)) return false;
        if (!plane_ok(Q.s[0], Q.ss[0], Q.sfs[0], pxt * bsi, batch, kStrideAny, false) || !plane_ok(Q.d[0], Q.ds[0], Q.dfs[0], pxt * bso, batch, kStrideAny, false))
            return false;
        for (int c = 1; c < 3; c++)
            if ((!(isemi && c == 2) && !plane_ok(Q.s[c], Q.ss[c], Q.sfs[c], chroma_in(pxt) * bsi, batch, kStrideAny, false)) ||
                (!(osemi && c == 2) && !plane_ok(Q.d[c], Q.ds[c], Q.dfs[c], chroma_out(pxt) * bso, batch, kStrideAny, false)))
                return false;
        return true;
    }
    // a plane at luma resolution beside the source (the stack's matte): whole aligned words per thread
    bool luma_plane_fits(const void *p, long long stride, long long fstride, int wide) const
    {
        return plane_ok(p, stride, fstride, pxt * (wide ? 2 : 1), batch, kStrideAny, false);
    }
    unsigned generic_grid(const char *family, const FrameGeom &H) const { return block_grid(family, H.w, H.rows, H.nframes, csx, csy); }
};

// launch_vec_or_generic for such a path.  extra_ok: what the family's vector kernels ask beyond UnionLaunch::fits (their modes, a
// plane of their own).  vec(Q, H) and generic(Q, H, x0) launch and return the kernel's name; x0 is the frame column of the planes'
// column 0, wv for the tail of a column split and 0 otherwise.  tail_name: the generic kernel's name, for a family that reports
// "<vector kernel>+<tail_name>" on a ragged split; null: the vector kernel's name alone.
template <class Vec, class Generic>
const char *launch_union(int variant, const PlaneSet &P, const FrameGeom &G, const UnionLaunch &U, bool extra_ok, Vec vec,
                         Generic generic, const char *tail_name = nullptr)
{
    int ran = 0, x0 = 0;                         // ran bit 0: a vector kernel was launched, bit 1: the generic one
    const char *name = launch_vec_or_generic(
        variant, P, G, U.pxt, [&](const PlaneSet &Q, const FrameGeom &H) { return extra_ok && U.fits(Q, H); },
        [&](const PlaneSet &Q, const FrameGeom &H) { ran |= 1; return vec(Q, H); },
        [&](const PlaneSet &Q, const FrameGeom &H) { ran |= 2; return generic(Q, H, x0); },
        [&](int wv) {
            x0 = wv;
            return advance_planes(P, wv * U.bsi, U.chroma_in(wv) * U.bsi, wv * U.bso, U.chroma_out(wv) * U.bso);
        });
    if (!name || ran != 3 || !tail_name) return name;
    static thread_local std::string both;
    both = std::string(name) + "+" + tail_name;
    return both.c_str();
}

// Where the vector kernels of a stage stack (lutr_stack.hip, lutr_rgbstack.hip, lutr_y2rstack.hip) read the CDL and 1D tables.
// The tables the stack uses go to LDS together or not at all: above 24 KB in sum they are read from global memory.
// LUTR_STACK_LDS=0 / 1 (tests and tools) says which; unset: the family's own default.
constexpr size_t kStackLdsBytes = 24 * 1024;
inline bool stack_in_lds(const StackConsts &S, bool family_default)
{
    const size_t bytes = (size_t)(S.lds_cdl_words + S.lds_l1d_words) * sizeof(uint32_t);
    if (bytes == 0 || bytes > kStackLdsBytes) return false;
    if (const char *e = getenv("LUTR_STACK_LDS")) {
        if (e[0] == '0' && !e[1]) return false;
        if (e[0] == '1' && !e[1]) return true;
    }
    return family_default;
}

// The persistent tile kernels pay a fixed start-up (coordinate table, tube staging, a wave's first tile at a quarter of the issue
// rate) and end with a tail of partly idle CUs, so they only win on big launches.  Round 3, Gpx/s tile / plain vector kernels (taps
// gathered from L1/L2, 5-8 waves per SIMD; profiles/r03_exp19_small_launches.txt), fused yuv420p10le strict: UHD 1 frame 181 / 272,
// 2 frames 253 / 322, 4 frames 316 / 357, 8 frames 442 / 326, 16 frames 507 / 333, 64 frames 560 / 338; 1080p 8 frames 253 / 326,
// 16 frames 337 / 300, 32 frames 424 / 324, 64 frames 478 / 329 -- the two-level chunk queue and its small chunks moved the
// crossover of the fused kernels and of the RGB tube kernels (8 UHD rgb24 frames: 480 vs 343 Gpx/s) from 70 Mpx (round 2) to
// ~33 Mpx.  The RGB tile kernels keep 70 (their queue is round 1's).  LUTR_SMALL_JOB_MPX moves every boundary (0 = never).
constexpr long long kSmallTileMpx = 70, kSmallQueueMpx = 33;
inline bool small_job(long long px, long long mpx)
{
    if (const char *e = getenv("LUTR_SMALL_JOB_MPX")) { const long long v = atoll(e); if (v >= 0 && v <= 100000) mpx = v; }
    return px < mpx * 1000000ll;
}

// LUTR_RGB2 / LUTR_NO_RGB2: which RGB launches the round-3 tube kernels (lutr_rgb2.hip) take.  LUTR_RGB2=0 or LUTR_NO_RGB2
// set: none; LUTR_RGB2=all: everything they can; else the measured default of each launcher.
enum Rgb2Policy { RGB2_OFF, RGB2_DEFAULT, RGB2_ALL };
inline Rgb2Policy rgb2_policy()
{
    const char *e = getenv("LUTR_RGB2");
    if ((e && e[0] == '0') || getenv("LUTR_NO_RGB2")) return RGB2_OFF;
    return e && e[0] == 'a' ? RGB2_ALL : RGB2_DEFAULT;
}

// ---------------------------------------------------------------- per-device facts
// Launchers may run on several threads at once (one context per thread): process-wide
// state is initialised exactly once (function-local statics, call_once) or guarded by a mutex.
inline int device_cus()
{
    static const int cus = [] {
        int dev = 0, n = 0;
        hipDeviceProp_t prop;
        if (hipGetDevice(&dev) == hipSuccess && hipGetDeviceProperties(&prop, dev) == hipSuccess) n = prop.multiProcessorCount;
        return n > 0 ? n : 256;
    }();
    return cus;
}

// LUTR_MAX_WAVES (tests and tools only): a cap on the waves of a persistent grid, so that a frame of a few megapixels runs as
// many tiles per wave and draws as many tickets per workgroup as a long launch does.  `text` is the variable's value (or null),
// `wpb` the launcher's waves per workgroup, `uncapped` its device_cus() * waves per CU.  Accepted only as a plain positive
// decimal multiple of `wpb` that is not above `uncapped`; anything else leaves `uncapped`.  Everything a launcher derives from
// its wave count (the tube and chunk thresholds, the chunk shrink loop, the grid, qbase) follows from the value returned.
inline int capped_waves(const char *text, int wpb, int uncapped)
{
    if (!text || !*text || wpb < 1) return uncapped;
    long long v = 0;
    for (const char *c = text; *c; c++) {
        if (*c < '0' || *c > '9') return uncapped;
        v = v * 10 + (*c - '0');
        if (v > uncapped) return uncapped;
    }
    return v > 0 && v % wpb == 0 ? (int)v : uncapped;
}

// Blocks of more than 4 waves need more than the default 64 KB of dynamic LDS: allow it once per (device, kernel).
// false: the runtime refused 160 KB of dynamic LDS for this kernel (the launch would fail).
inline bool allow_lds(const void *kernel, size_t bytes)
{
    static std::set<std::pair<int, const void *>> done;      // the attribute is per device
    static std::mutex mu;
    if (bytes <= 65536) return true;
    int dev = 0;
    (void)hipGetDevice(&dev);
    std::lock_guard<std::mutex> lock(mu);
    if (done.count({dev, kernel})) return true;
    if (hipFuncSetAttribute(kernel, hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024) != hipSuccess) return false;
    done.insert({dev, kernel});
    return true;
}

}  // namespace lutr
