// lutr_tile2.hip -- round-2 fused YUV tile kernels: persistent waves, a workgroup-shared GREY TUBE of the lattice in LDS for
// near-neutral content, per-wave LDS lattice windows for the saturated rest, and validity decided in RAW CODE SPACE before
// any pixel is computed.
//
// Replaces the slice-threaded per-row loops of FFmpeg's lut3d + the scalers around it
// (the filters /root/reference/src/lut_renderer/ffmpeg.py:212-247,:304-310 emits).
//
// What changed against round 1's lutr_tile.hip (DESIGN.md "Kernels" has the measurements):
//   * VALIDITY WITHOUT PER-PIXEL WORK.  Round 1 computed a tile optimistically, accumulated min/max of every
//     pixel's lattice cell (6 VALU per pixel), voted, and redid the tile on a miss.  Here a window carries a BOX
//     [y]x[cb]x[cr] of raw input codes with the guarantee that every pixel inside the box only touches staged
//     nodes.  A tile's raw extremes come from v_pk_min/max_u16 on the packed input words (~1.7 VALU per pixel),
//     one saturating-subtract test per plane says whether the lane's unit is inside the box, one vote per tile.
//     No tile is ever computed twice, no address clamp is needed, and the body has no bounds code at all.
//     box -> cells is a conservative map (map_box below) that exploits what the sheared window exploits: in
//     (r, g-r, b-r) coordinates luma cancels out of the two chroma-like axes.
//   * THE GREY TUBE (level 0, tube_lane / tube_holds).  In the sheared coordinates the two difference axes depend on chroma alone, so
//     "all of r, |g - r| and |b - r| up to H cells" can be staged ONCE per workgroup (98 KB as fp16 at 33^3, H = 8) and serves
//     every tile whose chroma stays within +-64 8-bit codes of G-R and B-R whatever its luma does: 95 % of the tiles of the
//     natural test frames, with no window, no raw box, no second level and no restage.  The windows keep the rest.
//   * PADDED PER-CODE TABLE.  The {prev, frac} table covers every index the YUV->RGB sum can reach (negative sums
//     saturate to 0 in v_cvt_u32_f32), so the per-channel v_min_u32 is gone.
//   * OUTPUT PACKING BY SDWA.  v_cvt_u32_f32_sdwa writes a sample straight into its half-word / byte.
//   * FAST VARIANT (V = 3).  LDS nodes are 8-byte {r,g,b,-} fp16 pre-multiplied by 2^depth-1; the blend is an fma chain
//     of v_fma_mix_f32 (fp16 tap x fp32 weight + fp32 accumulator, exact products, one rounding per step): 12 VALU
//     instead of 24 per pixel, a tap is one ds_read_b64, the window holds 2-3x the nodes.  (Measured alternative: fp32
//     float4 nodes pre-multiplied by M with plain v_fma_f32 -- full-rate VALU, but ds_read_b128 taps run into LDS bank
//     conflicts: 403 vs 560 Gpx/s.)  |fast - strict| <= 1 code at 8 and 10 bit (tests/test_fast_variant.py, DESIGN.md
//     3.4); the strict kernels stay bit-identical to the oracle.
//   * FMA32 VARIANT (V = 4).  The strict kernels' nodes, layout and staging, read from a copy of the lattice pre-multiplied
//     by 2^depth-1 in fp32 (LutConsts::latm); the blend is a chain of full-rate v_fma_f32 with no final `* M`.  Each step
//     rounds once, so the value before truncation is within a few ulp of strict's: <= 1 code at every depth.
//   * Input and output depth are independent (10-bit in, 8-bit out is the reference's libx264 default).
//   * SHARED WITH lutr_rgb2.hip (lutr_tube.h): the two-level chunk queue, the tube's axes and the plane strides padded against LDS
//     bank conflicts, the small machine helpers.  Experiment variants that lost their measurement are not in this file: a
//     one-line note stands where each would go, with the number and the profiles/ file or DESIGN.md section that holds it.
//
// Arithmetic of the strict variants: -ffp-contract=off, FFmpeg's scalar C order, bit-identical to the oracle.
#include <cstdio>
#include <cstdlib>
#include <mutex>
#include <set>
#include <type_traits>
#include <utility>

#include "lutr_internal.h"
#include "lutr_launch.h"
#include "lutr_tube.h"

// One translation unit per (input width, output width, chroma layout): the Makefile compiles this file nine times
// (-DLUTR_T2_WI=.. -DLUTR_T2_WO=.. -DLUTR_T2_X=.. -DLUTR_T2_Y=..), in parallel, each defining launch_yuv_tile2_w<WI><WO>_c<X><Y>.
#ifndef LUTR_T2_WI
#define LUTR_T2_WI 1
#define LUTR_T2_WO 1
#define LUTR_T2_X 1
#define LUTR_T2_Y 1
#endif
#define T2_CAT_(a, b, c, d) launch_yuv_tile2_w##a##b##_c##c##d
#define T2_CAT(a, b, c, d) T2_CAT_(a, b, c, d)
#define T2_ENTRY T2_CAT(LUTR_T2_WI, LUTR_T2_WO, LUTR_T2_X, LUTR_T2_Y)

#ifndef LUTR_T2_WPB
#define LUTR_T2_WPB 16            // waves per workgroup: one workgroup per CU shares one coordinate table
#endif
#ifndef LUTR_T2_WAVES_PER_EU
#define LUTR_T2_WAVES_PER_EU 4
#endif

namespace lutr {
namespace t2 {

extern __shared__ __attribute__((aligned(16))) char smem[];

// LDS behind the coordinate table: 64 bytes of scratch per wave (window cell ranges, raw box, counters), then the WORKGROUP's
// chunk allocator (the two-level queue of lutr_tube.h).
constexpr int kWaveScratch = LUTR_T2_WPB * 64;
constexpr int kScratch = kWaveScratch + tube::kQueueLds;

enum { V_GEN = 0, V_TAB = 1, V_UNIT = 2, V_FAST = 3, V_FMA32 = 4 };      // V >= V_UNIT: clip-free

// ---------------------------------------------------------------- small machine helpers (more in lutr_tube.h)
using namespace tube;
DEV float in_vgpr(float s)
{
    float v;
    asm volatile("v_mov_b32 %0, %1" : "=v"(v) : "s"(s));
    return v;
}
DEV uint32_t pk_min(uint32_t a, uint32_t b) { uint32_t o; asm("v_pk_min_u16 %0, %1, %2" : "=v"(o) : "v"(a), "v"(b)); return o; }
DEV uint32_t pk_max(uint32_t a, uint32_t b) { uint32_t o; asm("v_pk_max_u16 %0, %1, %2" : "=v"(o) : "v"(a), "v"(b)); return o; }
// per 16-bit half: max(a - b, 0)
DEV uint32_t pk_subsat_sv(uint32_t a, uint32_t b) { uint32_t o; asm("v_pk_sub_u16 %0, %1, %2 clamp" : "=v"(o) : "s"(a), "v"(b)); return o; }
DEV uint32_t pk_subsat_vs(uint32_t a, uint32_t b) { uint32_t o; asm("v_pk_sub_u16 %0, %1, %2 clamp" : "=v"(o) : "v"(a), "s"(b)); return o; }

// fp32 weight x fp16 tap (+ fp32 accumulator): v_fma_mix_f32, products exact, one rounding (== fmaf(w, (float)h, c))
DEV float mix0_lo(float w, uint32_t h) { float d; asm("v_fma_mix_f32 %0, %1, %2, 0 op_sel_hi:[0,1,0]" : "=v"(d) : "v"(w), "v"(h)); return d; }
DEV float mix0_hi(float w, uint32_t h) { float d; asm("v_fma_mix_f32 %0, %1, %2, 0 op_sel:[0,1,0] op_sel_hi:[0,1,0]" : "=v"(d) : "v"(w), "v"(h)); return d; }
DEV float mix_lo(float w, uint32_t h, float c) { float d; asm("v_fma_mix_f32 %0, %1, %2, %3 op_sel_hi:[0,1,0]" : "=v"(d) : "v"(w), "v"(h), "v"(c)); return d; }
DEV float mix_hi(float w, uint32_t h, float c) { float d; asm("v_fma_mix_f32 %0, %1, %2, %3 op_sel:[0,1,0] op_sel_hi:[0,1,0]" : "=v"(d) : "v"(w), "v"(h), "v"(c)); return d; }
// fp16 - fp16 -> fp32 (one rounding), and f * t + fp16: the two halves of a lerp whose end points are fp16 taps
DEV float hsub_lo(uint32_t a, uint32_t b) { float d; asm("v_fma_mix_f32 %0, %1, 1.0, -%2 op_sel_hi:[1,0,1]" : "=v"(d) : "v"(a), "v"(b)); return d; }
DEV float hsub_hi(uint32_t a, uint32_t b) { float d; asm("v_fma_mix_f32 %0, %1, 1.0, -%2 op_sel:[1,0,1] op_sel_hi:[1,0,1]" : "=v"(d) : "v"(a), "v"(b)); return d; }
DEV float hlerp_lo(float t, float f, uint32_t v0) { float d; asm("v_fma_mix_f32 %0, %1, %2, %3 op_sel_hi:[0,0,1]" : "=v"(d) : "v"(t), "v"(f), "v"(v0)); return d; }
DEV float hlerp_hi(float t, float f, uint32_t v0) { float d; asm("v_fma_mix_f32 %0, %1, %2, %3 op_sel:[0,0,1] op_sel_hi:[0,0,1]" : "=v"(d) : "v"(t), "v"(f), "v"(v0)); return d; }
// fp16 difference * fp32 fraction + fp16 node: D in the low (D_HI = 0) or high half of `dw`, v0 in the low or high half of `vw`
template <int D_HI, int V_HI> DEV float reclerp(uint32_t dw, float f, uint32_t vw)
{
    float d;
    if constexpr (!D_HI && !V_HI) asm("v_fma_mix_f32 %0, %1, %2, %3 op_sel_hi:[1,0,1]" : "=v"(d) : "v"(dw), "v"(f), "v"(vw));
    else if constexpr (!D_HI && V_HI) asm("v_fma_mix_f32 %0, %1, %2, %3 op_sel:[0,0,1] op_sel_hi:[1,0,1]" : "=v"(d) : "v"(dw), "v"(f), "v"(vw));
    else if constexpr (D_HI && !V_HI) asm("v_fma_mix_f32 %0, %1, %2, %3 op_sel:[1,0,0] op_sel_hi:[1,0,1]" : "=v"(d) : "v"(dw), "v"(f), "v"(vw));
    else asm("v_fma_mix_f32 %0, %1, %2, %3 op_sel:[1,0,1] op_sel_hi:[1,0,1]" : "=v"(d) : "v"(dw), "v"(f), "v"(vw));
    return d;
}
DEV uint32_t f2h_bits(float v) { return (uint32_t)__builtin_bit_cast(unsigned short, (_Float16)v); }     // v_cvt_f16_f32, round to nearest even
// the record of a node `a` whose r + 1 neighbour is `b` (both {r | g << 16, b} of fp16): differences exact in fp32, then rounded to fp16
struct u3 { uint32_t x, y, z; };
DEV u3 make_rec(uint2 a, uint2 b)
{
    const uint32_t dr = f2h_bits(hsub_lo(b.x, a.x)), dg = f2h_bits(hsub_hi(b.x, a.x)), db = f2h_bits(hsub_lo(b.y, a.y));
    return u3{a.x, (a.y & 0xffffu) | (dr << 16), dg | (db << 16)};
}

// (Measured and removed: packed fp32 -- v_pk_add/mul_f32 -- for the R,G pair of the strict blends, the luma add, `* M` and the chroma
// sums, behind a build switch: bit-identical, 68.2 -> 58.7 VALU per pixel in the strict body, and 1-2 % SLOWER; part by part 573-594
// against 595 Gpx/s: profiles/r03_exp37_packed_fp32_parts.txt)
DEV int lds_base() { return (int)(unsigned)(uintptr_t)(__attribute__((address_space(3))) char *)smem; }

typedef uint32_t u2 __attribute__((ext_vector_type(2)));

// ---------------------------------------------------------------- geometry shared with the launcher
struct Geom {
    int lw_log2;          // lanes along x per tile row = 1 << lw_log2 (the other lanes go down)
    int uw, urows;        // units per row, unit rows (a unit = PXT px x BH rows)
    int nsx, nry;         // tiles across, tiles down
    int ch, nrc, nchunks; // chunk = `ch` consecutive tile rows of one strip; chunk id = (frame*nrc + rc)*nsx + strip
    int win_nodes;        // LDS window capacity per wave, in nodes
    int tab_entries;      // per-code coordinate table at LDS offset 0 (0 = coordinates are computed)
    int max_raw;          // 2^din - 1: a raw code above it cannot be trusted to stay inside the table
    int whole;            // 1: the WHOLE lattice fits the workgroup's LDS (N <= 21 strict / 25 fast at 10 bit): staged once,
    int whole_a, whole_b; //    node (r, g, b) at index r * whole_a + g * whole_b + b (strides padded against LDS bank conflicts)
                          // per workgroup, shared by its waves, no windows, no validity tests -- content cannot matter
    int tube_h;           // > 0: a workgroup-shared "grey tube" of the lattice is staged once, behind the scratch area: every cell with
                          // |pg - pr| <= tube_h and |pb - pr| <= tube_h, all of r.  Tiles whose chroma keeps them inside it (tube_holds)
                          // need no window at all; the per-wave windows serve the saturated rest.
    int tube_plane;       // nodes from one r plane of the tube to the next: (2 tube_h + 3)^2 plus a few nodes of padding chosen by the
                          // launcher so that cells one step apart on any two axes never share an LDS bank (tube_plane_stride)
    int mix_max;          // a tile with at most this many lanes outside the tube runs as a MIXED tile (tube body, the outliers' taps from the global lattice)
    float tube_t;         // the test: |gv - rv| and |bu - rv| (RGB codes, chroma only) must stay <= tube_t over the lane's unit
    unsigned tube_rlo, tube_rhi;   // a raw chroma interval [lo, hi] (packed like the window boxes) that implies the test for both planes:
                                   // four saturating subtractions instead of ~35 VALU for the tiles that fit it (tube_rlo > tube_rhi: none)
    unsigned *queue;      // device words {claims, waves done}: both 0 between launches -- the last wave to leave resets them (queue_leave),
                          // so a launch needs no memset node in front of it
    unsigned qbase;       // waves in the grid = the first chunk the counter hands out (the waves' ids come before it)
    unsigned *stats;      // optional device counters; nullptr = off
};

struct Planes2 {          // 32-bit strides: the launcher only sends layouts that fit (plane_ok under kStrideTile2)
    const uint8_t *s[3];
    uint8_t       *d[3];
    unsigned ss[3], ds[3];
    unsigned long long sfs[3], dfs[3];
};

// ---------------------------------------------------------------- variant traits
// INTERP as a template argument: lut3d's modes 0 / 1 / 2, and T2_TET16 = tetrahedral on float4 nodes -- the strict kernels' whole-lattice
// mode.  A tap is then one ds_read_b128 (4 LDS-array cycles) instead of ds_read2_b32 + ds_read_b32 (6), and scattered taps collide far
// less: with the whole 17^3 lattice in LDS, uniform-random frames 351 -> 515 Gpx/s, sigma-64 noise 390 -> 524, sigma-16 +3 %, natural
// frames the same (profiles/r03_exp35_whole_lattice_16byte_nodes.txt).  Everywhere else a third more nodes per KB is worth more (5.6).
constexpr int T2_TET16 = 3;
template <int INTERP, int V> struct Node {
    static constexpr bool fast = V == V_FAST;
    // bytes per node in a window: fast = four fp16 {r,g,b,-} (one ds_read_b64 per tap); strict 4-tap modes pack fp32 {r,g,b}
    // (a third more nodes per wave than float4; a tap is ds_read2_b32 + ds_read_b32); strict trilinear reads float4 nodes
    // fast trilinear stages RECORDS: the node plus the fp16 difference to its r + 1 neighbour, {r | g << 16, b | Dr << 16, Dg | Db << 16}
    // -- FFmpeg's first four lerps (along r) then take ONE v_fma_mix_f32 each instead of two, and a pixel reads 4 records instead of
    // 8 nodes.  (The strict kernels cannot afford it: fp32 records are 24 bytes, the tube would shrink to 4 cells and the windows to
    // nothing.)  The gather body rounds its differences to fp16 as well, so both paths compute the same number.
    static constexpr bool rec = fast && INTERP == LUTR_INTERP_TRILINEAR;
    static constexpr int lds = fast ? (rec ? 12 : 8) : ((INTERP == LUTR_INTERP_TRILINEAR || INTERP == T2_TET16) ? 16 : 12);
    static constexpr int glb = fast ? 8 : 16;                                              // bytes per node in HBM/L2
};

// ---------------------------------------------------------------- window (wave-uniform)
// The cells are integers (CrdI), and the tap address is still three full-rate fma -- with NO conversion at either end: the bits of an
// integer 0 <= k < 2^24 read as a float are k * 2^-149 (a denormal, or the first normal binade: the spacing is 2^-149 throughout), the
// kernels run with fp32 denormals on (the compiler's default for gfx9, spelled out in the Makefile: -fno-gpu-flush-denormals-to-zero;
// the code object says .amdhsa_float_denorm_mode_32 3), v_fma_f32 honours them at full rate, the steps fr / fg / fb are ordinary
// floats holding integers, so every product and sum below is an integer multiple of 2^-149 of magnitude below 2^24 * 2^-149, hence
// exact, and the bits of the (non-negative) result are the address.  (Measured instead: three v_mad_u32_u24 -- one instruction
// fewer still, all of them on the quarter-rate unit: 1.0 % slower than the parent, profiles/tile_cuts_ab.txt.)
DEV float as_tiny(int k) { return k >= 0 ? __int_as_float(k) : -__int_as_float(-k); }      // k * 2^-149, |k| < 2^24
struct Win {
    float fr, fg, fb, fc;        // LDS byte address of the c000 tap: bits of fma(tiny(pr), fr, fma(tiny(pg), fg, fma(tiny(pb), fb, fc))), fc = tiny(base)
    int   o_r, o_g;              // byte steps of +1 along r and g (blue is one node)
};
// The raw-code box a window is good for lives in the wave's LDS scratch, not in registers: {ylo, yhi, cblo, cbhi} at +32,
// {crlo, crhi} at +48, each bound replicated in both 16-bit halves (8-bit planes: code << 8, upper bounds | 0xff -- see
// extremes()).  Registers are what this kernel runs out of, and a value spilled to scratch is worse than it looks: a
// scratch_load in the per-tile path makes the wave wait with vmcnt(0), i.e. for the next tile's prefetch it has just issued.
struct Box { uint32_t ylo, yhi, cblo, cbhi, crlo, crhi; };
DEV void box_store(int scratch_off, const Box &b)
{
    *(uint4 *)(smem + scratch_off + 32) = make_uint4(b.ylo, b.yhi, b.cblo, b.cbhi);
    *(uint2 *)(smem + scratch_off + 48) = make_uint2(b.crlo, b.crhi);
}

// packed per-lane extremes of a unit.  yor: the OR of the luma words -- all the legality test wants (or_words); ymin and ymax are
// filled in by the tiles that go on to the window's raw box (luma_min, luma_max)
struct Ext { uint32_t ymin, ymax, cbmin, cbmax, crmin, crmax, yor; };

template <int INTERP>
DEV Crd crd_compute(const LutConsts &L, float code, float sc)
{
    const float x = code * L.scale_f;
    return crd_split<INTERP>(fminf(x * sc, L.lut_max));       // codes and scales are >= 0: only the upper clip can bind
}

// The kernels carry the cell as an integer (CrdI, lutr_tube.h): the table stores it so, the computed coordinates of the general
// variant are converted once, where they are made.
DEV CrdI crd_int(const Crd &c) { return CrdI{(int)c.p, c.d}; }

DEV CrdI crd_table(unsigned idx)
{
    const uint2 e = *(const uint2 *)(smem + idx * 8u);
    return CrdI{(int)e.x, __uint_as_float(e.y)};
}
// The per-pixel paths index the table by BYTE offset: their YUV -> RGB constants are pre-multiplied by 8 (KB in the kernel;
// a power of two commutes with every rounding), so (unsigned)(8 * v) & ~7 == 8 * floor(v): the `* 8` that was a
// quarter-rate v_lshl_add_u32 per channel is a v_and_b32 on the other pipe.
// The table sits at LDS address 0 (checked at kernel start): the offset IS the address (crd_table8, lutr_tube.h).
typedef __attribute__((address_space(3))) const int *lds_ip;        // the cell of an entry alone (tile_bounds)

// Entry i of the table = coordinates of code min(i, M): indices past M are what an out-of-gamut YUV triple produces
// before FFmpeg's clip to the depth; the clip is folded into the table.
template <int INTERP>
DEV void coord_table_fill(const LutConsts &L, int entries)
{
    for (int q = threadIdx.x; q < entries; q += 64 * LUTR_T2_WPB) {
        Crd c;
        if (L.pre) {                 // a shared prelut (LutConsts::pre_shared): the folded coordinate of the code, then prev / frac as ever
            c = crd_split<INTERP>(L.pre[min(q, (int)L.maxf)]);
        } else c = crd_compute<INTERP>(L, fminf((float)q, L.maxf), L.sc[0]);
        *(uint2 *)(smem + q * 8) = make_uint2((unsigned)(int)c.p, __float_as_uint(c.d));      // {int32 prev, float frac}
    }
    __syncthreads();
}

// ---------------------------------------------------------------- tiles
template <int WIN, int WOUT, int CSX, int CSY>
struct Tile {
    static constexpr int PXT = WIN ? 8 : 16;                         // luma samples per unit row (16 bytes in)
    static constexpr int BH = 1 << CSY, BW = 1 << CSX;
    static constexpr int NC = PXT >> CSX;                            // chroma samples per unit
    static constexpr int YWI = 4, YWO = PXT * (WOUT ? 2 : 1) / 4;    // luma words per row, in / out
    static constexpr int CWI = NC * (WIN ? 2 : 1) / 4, CWO = NC * (WOUT ? 2 : 1) / 4;
    static_assert(CWI >= 1 && CWO >= 1, "a unit must own whole chroma words");
};
template <int WIN, int WOUT, int CSX, int CSY> struct TileIn { using T = Tile<WIN, WOUT, CSX, CSY>; uint32_t y[T::BH][T::YWI], cb[T::CWI], cr[T::CWI]; };
template <int WIN, int WOUT, int CSX, int CSY> struct TileOut { using T = Tile<WIN, WOUT, CSX, CSY>; uint32_t y[T::BH][T::YWO], cb[T::CWO], cr[T::CWO]; };

// (wsample and the non-temporal stw: lutr_tube.h)
// floor(v) for v >= 0 (negatives saturate to 0) written into sample i of the word vector: one SDWA conversion
// (v_cvt_u32_f32 truncates) instead of convert + shift-or.  (lutr_rgb2.hip's `put` is the same idea; shared, the two compile to
// differently scheduled code.)
template <int WIDE>
DEV void wput(uint32_t *w, int i, float v)
{
    if constexpr (WIDE) {
        if ((i & 1) == 0) w[i >> 1] = (uint32_t)v;
        else asm("v_cvt_u32_f32_sdwa %0, %1 dst_sel:WORD_1 dst_unused:UNUSED_PRESERVE src0_sel:DWORD" : "+v"(w[i >> 1]) : "v"(v));
    } else {
        uint32_t &d = w[i >> 2];
        switch (i & 3) {
        case 0: d = (uint32_t)v; break;
        case 1: asm("v_cvt_u32_f32_sdwa %0, %1 dst_sel:BYTE_1 dst_unused:UNUSED_PRESERVE src0_sel:DWORD" : "+v"(d) : "v"(v)); break;
        case 2: asm("v_cvt_u32_f32_sdwa %0, %1 dst_sel:BYTE_2 dst_unused:UNUSED_PRESERVE src0_sel:DWORD" : "+v"(d) : "v"(v)); break;
        default: asm("v_cvt_u32_f32_sdwa %0, %1 dst_sel:BYTE_3 dst_unused:UNUSED_PRESERVE src0_sel:DWORD" : "+v"(d) : "v"(v)); break;
        }
    }
}

// Frames are read once and written once: the loads are non-temporal too (+0.9 % / +0.5 % on 4:2:0, +1 % each on 4:4:4 for stores / loads;
// planar RGB loses 2.5 % with non-temporal loads, DESIGN.md 5.2 "Streaming accesses")
template <int NW> DEV void ldw(uint32_t *w, const uint8_t *p)
{
    typedef unsigned nt4 __attribute__((ext_vector_type(4)));
    typedef unsigned nt2 __attribute__((ext_vector_type(2)));
    if constexpr (NW == 4) { const nt4 v = __builtin_nontemporal_load((const nt4 *)p); w[0] = v.x; w[1] = v.y; w[2] = v.z; w[3] = v.w; }
    else if constexpr (NW == 2) { const nt2 v = __builtin_nontemporal_load((const nt2 *)p); w[0] = v.x; w[1] = v.y; }
    else w[0] = __builtin_nontemporal_load((const uint32_t *)p);
}

template <int N> DEV void fence_words(uint32_t *w)
{
    if constexpr (N == 1) asm volatile("" : "+v"(w[0]));
    else if constexpr (N == 2) asm volatile("" : "+v"(w[0]), "+v"(w[1]));
    else if constexpr (N == 4) asm volatile("" : "+v"(w[0]), "+v"(w[1]), "+v"(w[2]), "+v"(w[3]));
    else if constexpr (N == 8) asm volatile("" : "+v"(w[0]), "+v"(w[1]), "+v"(w[2]), "+v"(w[3]), "+v"(w[4]), "+v"(w[5]), "+v"(w[6]), "+v"(w[7]));
}

// ---------------------------------------------------------------- raw extremes of a unit
// 16-bit containers: the words ARE pairs of samples.  8-bit: a word and the word shifted left by 8 are two streams of
// u16 whose HIGH byte is a sample (the low byte only breaks ties), so the same packed min/max yields exact byte
// extremes in the high bytes; bounds are compared as (code << 8) and (code << 8 | 0xff).
template <int WIN, int N>
DEV void ext_words(const uint32_t *w, uint32_t &mn, uint32_t &mx, bool first)
{
#pragma unroll
    for (int k = 0; k < N; k++) {
        if (first && k == 0) { mn = mx = w[0]; }
        else { mn = pk_min(mn, w[k]); mx = pk_max(mx, w[k]); }
        if constexpr (!WIN) { const uint32_t t = w[k] << 8; mn = pk_min(mn, t); mx = pk_max(mx, t); }
    }
}

// max only (the luma minimum is wanted by the window tests alone: tiles the tube takes never compute it)
template <int WIN, int N>
DEV void max_words(const uint32_t *w, uint32_t &mx, bool first)
{
#pragma unroll
    for (int k = 0; k < N; k++) {
        if (first && k == 0) mx = w[0];
        else mx = pk_max(mx, w[k]);
        if constexpr (!WIN) mx = pk_max(mx, w[k] << 8);
    }
}
template <int WIN, int N>
DEV void min_words(const uint32_t *w, uint32_t &mn, bool first)
{
#pragma unroll
    for (int k = 0; k < N; k++) {
        if (first && k == 0) mn = w[0];
        else mn = pk_min(mn, w[k]);
        if constexpr (!WIN) mn = pk_min(mn, w[k] << 8);
    }
}

// "No sample above 2^k - 1" does not need the maximum: it holds exactly when the OR of the words has no bit above k set, i.e. when
// the OR itself, half by half, is not above 2^k - 1 (the launcher checks that max_raw + 1 is a power of two): the OR takes the
// maximum's place in the saturating subtraction.  Three v_or3_b32 and a v_or_b32 instead of seven v_pk_max_u16 per tile.
template <int N>
DEV void or_words(const uint32_t *w, uint32_t &o, bool first)
{
#pragma unroll
    for (int k = 0; k < N; k++) o = (first && k == 0) ? w[0] : (o | w[k]);
}
// non-zero where a luma sample of the unit is above the top code (`top` = pack_hi(max_raw)).  8-bit planes: every byte is a legal
// code, there is no test.
template <int WIN> DEV uint32_t luma_illegal(uint32_t yor, uint32_t top)
{
    if constexpr (WIN) return pk_subsat_vs(yor, top);
    else return 0u;
}

// the chroma extremes and the OR of the luma words; the luma extremes come later, for the tiles that want them (luma_min, luma_max)
template <int WIN, int WOUT, int CSX, int CSY>
DEV Ext extremes(const TileIn<WIN, WOUT, CSX, CSY> &in)
{
    using T = Tile<WIN, WOUT, CSX, CSY>;
    Ext e;
    e.ymin = e.ymax = e.yor = 0u;
    if constexpr (WIN) {
#pragma unroll
        for (int dy = 0; dy < T::BH; dy++) or_words<T::YWI>(in.y[dy], e.yor, dy == 0);
    }
    ext_words<WIN, T::CWI>(in.cb, e.cbmin, e.cbmax, true);
    ext_words<WIN, T::CWI>(in.cr, e.crmin, e.crmax, true);
    return e;
}
template <int WIN, int WOUT, int CSX, int CSY>
DEV uint32_t luma_min(const TileIn<WIN, WOUT, CSX, CSY> &in)
{
    using T = Tile<WIN, WOUT, CSX, CSY>;
    uint32_t mn = 0u;
#pragma unroll
    for (int dy = 0; dy < T::BH; dy++) min_words<WIN, T::YWI>(in.y[dy], mn, dy == 0);
    return mn;
}
template <int WIN, int WOUT, int CSX, int CSY>
DEV uint32_t luma_max(const TileIn<WIN, WOUT, CSX, CSY> &in)
{
    using T = Tile<WIN, WOUT, CSX, CSY>;
    uint32_t mx = 0u;
#pragma unroll
    for (int dy = 0; dy < T::BH; dy++) max_words<WIN, T::YWI>(in.y[dy], mx, dy == 0);
    return mx;
}

DEV uint32_t pk_subsat(uint32_t a, uint32_t b) { uint32_t o; asm("v_pk_sub_u16 %0, %1, %2 clamp" : "=v"(o) : "v"(a), "v"(b)); return o; }

DEV bool box_holds(int scratch_off, const Ext &e)
{
    const uint4 p = *(const uint4 *)(smem + scratch_off + 32);      // ylo, yhi, cblo, cbhi
    const uint2 q = *(const uint2 *)(smem + scratch_off + 48);      // crlo, crhi
    // every half >= lo and <= hi  <=>  all six saturating differences are zero
    const uint32_t a = pk_subsat(p.x, e.ymin) | pk_subsat(e.ymax, p.y) | pk_subsat(p.z, e.cbmin);
    const uint32_t b = pk_subsat(e.cbmax, p.w) | pk_subsat(q.x, e.crmin) | pk_subsat(e.crmax, q.y);
    return __all((a | b) == 0u);
}

// ---------------------------------------------------------------- box -> cells (conservative, wave-uniform)
// Raw box (float codes, inclusive) -> inclusive ranges of the sheared cell coordinates (pr, pg-pr, pb-pr) that any
// pixel inside the box can produce.  Every float op of the pixel pipeline is monotone in its inputs, so per-channel
// cell ranges follow exactly from evaluating the SAME ops at the right corners.  For the two difference axes that would
// throw away the one thing that makes the sheared window small (luma cancels), so they are bounded analytically:
//   pg - pr in (sg - sr - 1, sg - sr + 1),  sg - sr = kappa (qG - qR) +- 2 delta_s,
//   qG - qR in (dG - 1 - eps, dG + 1 + eps) with dG = gv - rv a function of chroma only (monotone in cb and in cr),
// and where FFmpeg's clip to [0, M] can bind inside the box the clipped difference lies between 0 and the unclipped one.
// The result is intersected with plain interval arithmetic on the per-channel ranges (also valid).
struct Cells { int r0, r1, g0, g1, b0, b1; };

template <int INTERP, int PRE, int V>
DEV float cell_of(const LutConsts &L, float q, int ch, int tab_entries)
{
    if constexpr (V >= V_TAB) { (void)ch; (void)tab_entries; return (float)crd_table((unsigned)q).p; }
    else { (void)tab_entries; return crd_compute<INTERP>(L, q, L.sc[ch]).p; }
}

DEV float qclip(float v, float m) { return med3(floorf(v), 0.0f, m); }
DEV float cfloor(float v, float hi) { return med3(floorf(v), 0.0f, hi); }

template <int INTERP, int PRE, int V>
DEV Cells map_box(const LutConsts &L, const YuvConsts &K, const Geom &TG, float y0, float y1, float cb0, float cb1, float cr0, float cr1)
{
    if constexpr (PRE) {       // the range/depth prologue is a monotone map of each plane
        y0 = qclip(fma_(K.py, y0, K.pyb), K.pre_max); y1 = qclip(fma_(K.py, y1, K.pyb), K.pre_max);
        cb0 = qclip(fma_(K.pc, cb0, K.pcb), K.pre_max); cb1 = qclip(fma_(K.pc, cb1, K.pcb), K.pre_max);
        cr0 = qclip(fma_(K.pc, cr0, K.pcb), K.pre_max); cr1 = qclip(fma_(K.pc, cr1, K.pcb), K.pre_max);
    }
    const float yy0 = fma_(K.ky, y0, K.yb), yy1 = fma_(K.ky, y1, K.yb);
    const float cbd0 = cb0 - K.coff, cbd1 = cb1 - K.coff, crd0 = cr0 - K.coff, crd1 = cr1 - K.coff;
    // krv, kbu > 0; kgu, kgv < 0 for every matrix (make_yuv_consts)
    const float rv0 = K.krv * crd0, rv1 = K.krv * crd1, bu0 = K.kbu * cbd0, bu1 = K.kbu * cbd1;
    const float gv0 = fma_(K.kgu, cbd1, K.kgv * crd1), gv1 = fma_(K.kgu, cbd0, K.kgv * crd0);      // min, max
    const float m = K.max_l;
    const float vr0 = yy0 + rv0, vr1 = yy1 + rv1, vg0 = yy0 + gv0, vg1 = yy1 + gv1, vb0 = yy0 + bu0, vb1 = yy1 + bu1;
    const int te = TG.tab_entries;
    const float pr0 = cell_of<INTERP, PRE, V>(L, qclip(vr0, m), 0, te), pr1 = cell_of<INTERP, PRE, V>(L, qclip(vr1, m), 0, te);
    const float pg0 = cell_of<INTERP, PRE, V>(L, qclip(vg0, m), 1, te), pg1 = cell_of<INTERP, PRE, V>(L, qclip(vg1, m), 1, te);
    const float pb0 = cell_of<INTERP, PRE, V>(L, qclip(vb0, m), 2, te), pb1 = cell_of<INTERP, PRE, V>(L, qclip(vb1, m), 2, te);
    Cells c;
    c.r0 = (int)pr0; c.r1 = (int)pr1;
    // the second difference axis is (b - g), as the tube's (lutr_tube.h)
    float g_lo = pg0 - pr1, g_hi = pg1 - pr0;                                                   // interval arithmetic
    float b_lo = pb0 - pg1, b_hi = pb1 - pg0;
    if (L.pre || (L.sc[0] == L.sc[1] && L.sc[1] == L.sc[2])) {
        // chroma-only difference terms at the corners that extremise them: gv - rv falls in cb and in cr;
        // bu - gv rises in both (gv1 = gv at (cb0, cr0), gv0 = gv at (cb1, cr1))
        float dg0 = gv0 - rv1, dg1 = gv1 - rv0;
        float db0 = bu0 - gv1, db1 = bu1 - gv0;
        // (a shared prelut is a monotone map whose slope lies between 0 and pre_kappa cells per code: a code difference d moves the
        // cell by at most pre_kappa |d| and possibly not at all -- the same one-sided form as where the clip can bind)
        const bool clips = L.pre || vr0 < 0.0f || vg0 < 0.0f || vb0 < 0.0f || vr1 >= m + 1.0f || vg1 >= m + 1.0f || vb1 >= m + 1.0f;
        if (clips) { dg0 = fminf(dg0, 0.0f); dg1 = fmaxf(dg1, 0.0f); db0 = fminf(db0, 0.0f); db1 = fmaxf(db1, 0.0f); }
        const float kappa = L.pre ? L.pre_kappa : L.sc[0] * L.scale_f;
        const float eps = m * (1.0f / 2097152.0f) + 1e-3f;                    // float rounding of the sums, and then some
        const float slack = 1.0f + 2.0f * L.lut_max * (1.0f / 2097152.0f) + 2e-3f;
        g_lo = fmaxf(g_lo, floorf(kappa * (dg0 - 1.0f - eps) - slack) + 1.0f);
        g_hi = fminf(g_hi, ceilf(kappa * (dg1 + 1.0f + eps) + slack) - 1.0f);
        b_lo = fmaxf(b_lo, floorf(kappa * (db0 - 1.0f - eps) - slack) + 1.0f);
        b_hi = fminf(b_hi, ceilf(kappa * (db1 + 1.0f + eps) + slack) - 1.0f);
    }
    c.g0 = (int)g_lo; c.g1 = (int)g_hi; c.b0 = (int)b_lo; c.b1 = (int)b_hi;
    return c;
}

// ---------------------------------------------------------------- exact cell bounds of a tile (second-level test)
// When the raw-box test fails the tile is not necessarily outside the window: the box is a conservative, axis-aligned
// description (uncorrelated sensor noise in Cb and Cr spans a box whose corners no pixel reaches).  The second level
// computes what round 1 computed for every tile: the exact cells each pixel touches, min/max per lane, one vote against
// the window's cell ranges.  ~18 VALU per pixel, paid only by the tiles that fail the cheap test.
struct Bnd { int rmin, rmax, gmin, gmax, bmin, bmax; };
constexpr int kBndNone = 1 << 30;       // rmin = ... = kBndNone, rmax = ... = -kBndNone: no cell yet
// (written as asm like the float forms in lutr_tube.h)
DEV int vmin3i(int a, int b, int c) { int o; asm("v_min3_i32 %0, %1, %2, %3" : "=v"(o) : "v"(a), "v"(b), "v"(c)); return o; }
DEV int vmax3i(int a, int b, int c) { int o; asm("v_max3_i32 %0, %1, %2, %3" : "=v"(o) : "v"(a), "v"(b), "v"(c)); return o; }
DEV int wave_min_i(int v)
{
#pragma unroll
    for (int m = 32; m >= 1; m >>= 1) v = min(v, __shfl_xor(v, m, 64));
    return v;
}
DEV int wave_max_i(int v)
{
#pragma unroll
    for (int m = 32; m >= 1; m >>= 1) v = max(v, __shfl_xor(v, m, 64));
    return v;
}

template <int WIN, int WOUT, int CSX, int CSY, int INTERP, int PRE, int V>
DEV Bnd tile_bounds(const LutConsts &L, const YuvConsts &K, const Geom &TG, TileIn<WIN, WOUT, CSX, CSY> &in)
{
    using T = Tile<WIN, WOUT, CSX, CSY>;
    Bnd bn;
    bn.rmin = bn.gmin = bn.bmin = kBndNone;
    bn.rmax = bn.gmax = bn.bmax = -kBndNone;
#pragma unroll
    for (int j = 0; j < T::NC; j++) {
        float cbv = wsample<WIN>(in.cb, j), crv = wsample<WIN>(in.cr, j);
        if constexpr (PRE) {
            cbv = cfloor(fma_(K.pc, cbv, K.pcb), K.pre_max);
            crv = cfloor(fma_(K.pc, crv, K.pcb), K.pre_max);
        }
        const float cbd = cbv - K.coff, crd = crv - K.coff;
        const float rv = K.krv * crd, gv = fma_(K.kgu, cbd, K.kgv * crd), bu = K.kbu * cbd;
        constexpr int NQ = T::BH * T::BW;
        int pr[NQ], pg_[NQ], pb_[NQ], hg[NQ], hb[NQ];
        // all table reads of the chroma block first, then their uses (one LDS round trip per block, not per pixel)
#pragma unroll
        for (int q = 0; q < NQ; q++) {
            const int dy = q / T::BW, dx = q % T::BW;
            float yv = wsample<WIN>(in.y[dy], j * T::BW + dx);
            if constexpr (PRE) yv = cfloor(fma_(K.py, yv, K.pyb), K.pre_max);
            const float yy = fma_(K.ky, yv, K.yb);
            if constexpr (V >= V_TAB) {
                // K is the kernel's KB; the caller has checked that every raw code is legal, so the padded table covers the sums
                pr[q] = *(lds_ip)(uintptr_t)((unsigned)(yy + rv) & ~7u);
                pg_[q] = *(lds_ip)(uintptr_t)((unsigned)(yy + gv) & ~7u);
                pb_[q] = *(lds_ip)(uintptr_t)((unsigned)(yy + bu) & ~7u);
            } else {
                pr[q] = (int)crd_compute<INTERP>(L, cfloor(yy + rv, K.max_l), L.sc[0]).p;
                pg_[q] = (int)crd_compute<INTERP>(L, cfloor(yy + gv, K.max_l), L.sc[1]).p;
                pb_[q] = (int)crd_compute<INTERP>(L, cfloor(yy + bu, K.max_l), L.sc[2]).p;
            }
        }
        __builtin_amdgcn_sched_barrier(0);
#pragma unroll
        for (int q = 0; q < NQ; q++) { hg[q] = pg_[q] - pr[q]; hb[q] = pb_[q] - pg_[q]; }
        if constexpr (T::BH * T::BW >= 2) {
#pragma unroll
            for (int q = 0; q + 1 < T::BH * T::BW; q += 2) {
                bn.rmin = vmin3i(bn.rmin, pr[q], pr[q + 1]); bn.rmax = vmax3i(bn.rmax, pr[q], pr[q + 1]);
                bn.gmin = vmin3i(bn.gmin, hg[q], hg[q + 1]); bn.gmax = vmax3i(bn.gmax, hg[q], hg[q + 1]);
                bn.bmin = vmin3i(bn.bmin, hb[q], hb[q + 1]); bn.bmax = vmax3i(bn.bmax, hb[q], hb[q + 1]);
            }
        } else {
            bn.rmin = min(bn.rmin, pr[0]); bn.rmax = max(bn.rmax, pr[0]);
            bn.gmin = min(bn.gmin, hg[0]); bn.gmax = max(bn.gmax, hg[0]);
            bn.bmin = min(bn.bmin, hb[0]); bn.bmax = max(bn.bmax, hb[0]);
        }
        // keep the blocks in program order (see tile_body): the fences do not change the words
        fence_words<T::YWI * T::BH>(&in.y[0][0]);
        fence_words<T::CWI>(in.cb);
        fence_words<T::CWI>(in.cr);
        asm volatile("" : "+v"(bn.rmin), "+v"(bn.rmax), "+v"(bn.gmin), "+v"(bn.gmax), "+v"(bn.bmin), "+v"(bn.bmax));
    }
    return bn;
}

// the window's cell ranges live in the wave's 64-byte LDS scratch (they are only read on the second-level path)
DEV bool cells_hold(int scratch_off, const Bnd &b)
{
    const int4 lo = *(const int4 *)(smem + scratch_off);            // r_lo, g_lo, b_lo, r_hi
    const int2 hi = *(const int2 *)(smem + scratch_off + 16);       // g_hi, b_hi
    const bool ok = b.rmin >= lo.x && b.rmax <= lo.w && b.gmin >= lo.y && b.gmax <= hi.x && b.bmin >= lo.z && b.bmax <= hi.y;
    return __all(ok);
}

template <int WIN> DEV int lo_of_(uint32_t mn) { const int a = (int)(mn & 0xffffu), b = (int)(mn >> 16); const int v = a < b ? a : b; return WIN ? v : v >> 8; }
template <int WIN> DEV int hi_of_(uint32_t mx) { const int a = (int)(mx & 0xffffu), b = (int)(mx >> 16); const int v = a > b ? a : b; return WIN ? v : v >> 8; }

// ---------------------------------------------------------------- the grey tube
// Is every pixel of the tile inside the tube?  In sheared coordinates luma cancels out of the two difference axes (map_box), so the
// answer depends on chroma alone: with dG = gv - rv and dB = bu - rv (monotone in cb and cr, evaluated at the corners of the lane's
// chroma extremes), every cell has |pg - pr| <= H and |pb - pr| <= H as soon as |dG|, |dB| <= tube_t =
// (H + 1 - slack) / kappa - 1 - eps -- map_box's own bound solved for d.  Where FFmpeg's clip to [0, M] binds, the clipped
// difference lies between 0 and the unclipped one, and 0 is inside.  One vote per tile, ~35 VALU per lane, no luma needed.
template <int WIN, int PRE>
DEV bool tube_holds(const YuvConsts &K, const Geom &TG, const Ext &e)
{
    float cb0 = (float)lo_of_<WIN>(e.cbmin), cb1 = (float)hi_of_<WIN>(e.cbmax);
    float cr0 = (float)lo_of_<WIN>(e.crmin), cr1 = (float)hi_of_<WIN>(e.crmax);
    if constexpr (PRE) {       // the range/depth prologue is a monotone map of each plane
        cb0 = qclip(fma_(K.pc, cb0, K.pcb), K.pre_max); cb1 = qclip(fma_(K.pc, cb1, K.pcb), K.pre_max);
        cr0 = qclip(fma_(K.pc, cr0, K.pcb), K.pre_max); cr1 = qclip(fma_(K.pc, cr1, K.pcb), K.pre_max);
    }
    const float cbd0 = cb0 - K.coff, cbd1 = cb1 - K.coff, crd0 = cr0 - K.coff, crd1 = cr1 - K.coff;
    // krv, kbu > 0; kgu, kgv < 0 for every matrix (make_yuv_consts)
    const float rv0 = K.krv * crd0, rv1 = K.krv * crd1, bu0 = K.kbu * cbd0, bu1 = K.kbu * cbd1;
    const float gv0 = fma_(K.kgu, cbd1, K.kgv * crd1), gv1 = fma_(K.kgu, cbd0, K.kgv * crd0);      // min, max
    // (b - g: bu - gv rises in cb and in cr, its extremes sit at the corners (cb0, cr0) and (cb1, cr1) where gv is gv1 and gv0)
    const float dg0 = gv0 - rv1, dg1 = gv1 - rv0;
    const float db0 = bu0 - gv1, db1 = bu1 - gv0;
    const float worst = vmax3(fmaxf(-dg0, dg1), -db0, db1);
    return worst <= TG.tube_t;          // per lane: the caller votes
}

// The same bound sample by sample, for units with at most four chroma samples (4:2:0 and 4:2:2 at 10 bit): a pixel's chroma IS one
// of them, so no pairing of one sample's Cb with another's Cr inflates the differences.  About the cost of the corner form; under
// per-sample chroma noise it keeps more tiles in the tube (sigma = 16, strict kernels' H = 6: 17 % -> 32 % of the tiles).
// Returns the samples OUTSIDE the bound, bit j = chroma sample j of the lane's unit (0: the lane is inside; the caller votes): a
// mixed tile patches only the pixel groups that own such a sample (tile_body, MIX).
template <int WIN, int WOUT, int CSX, int CSY, int PRE>
DEV unsigned tube_outside_samples(const YuvConsts &K, const Geom &TG, const TileIn<WIN, WOUT, CSX, CSY> &in)
{
    using T = Tile<WIN, WOUT, CSX, CSY>;
    unsigned bad = 0u;
#pragma unroll
    for (int j = 0; j < T::NC; j++) {
        float cbv = wsample<WIN>(in.cb, j), crv = wsample<WIN>(in.cr, j);
        if constexpr (PRE) {
            cbv = cfloor(fma_(K.pc, cbv, K.pcb), K.pre_max);
            crv = cfloor(fma_(K.pc, crv, K.pcb), K.pre_max);
        }
        const float cbd = cbv - K.coff, crd = crv - K.coff;
        const float rv = K.krv * crd, gv = fma_(K.kgu, cbd, K.kgv * crd), bu = K.kbu * cbd;
        if (!(fmaxf(fabsf(gv - rv), fabsf(bu - gv)) <= TG.tube_t)) bad |= 1u << j;
    }
    return bad;
}

// ---------------------------------------------------------------- restage
DEV uint32_t shx(uint32_t v, int m) { return (uint32_t)__shfl_xor((int)v, m, 64); }
template <int WIN> DEV int lo_of(uint32_t mn) { const int a = (int)(mn & 0xffffu), b = (int)(mn >> 16); const int v = a < b ? a : b; return WIN ? v : v >> 8; }
template <int WIN> DEV int hi_of(uint32_t mx) { const int a = (int)(mx & 0xffffu), b = (int)(mx >> 16); const int v = a > b ? a : b; return WIN ? v : v >> 8; }
template <int WIN> DEV uint32_t pack_lo(int v) { const uint32_t h = WIN ? (uint32_t)v : (uint32_t)v << 8; return h | (h << 16); }
template <int WIN> DEV uint32_t pack_hi(int v) { const uint32_t h = WIN ? (uint32_t)v : ((uint32_t)v << 8) | 0xffu; return h | (h << 16); }

// The window holds this tile (second-level test) but its raw box does not -- typically a window that was staged around the
// exact cells of an edge tile and has no box at all.  Try to give it one without staging anything: the largest of a few raw
// boxes around this tile's raw extremes whose conservative cell map lies inside the window's cell ranges.  Called with
// back-off (1st, 4th, 16th consecutive second-level pass), so a wave leaves the expensive mode once it is past the edge.
template <int WIN, int INTERP, int PRE, int V>
DEV bool rebox(const LutConsts &L, const YuvConsts &K, const Geom &TG, const Ext &e_, int scratch_off, int lane)
{
    Ext e = e_;
    asm volatile("" : "+v"(e.ymin), "+v"(e.ymax), "+v"(e.cbmin), "+v"(e.cbmax), "+v"(e.crmin), "+v"(e.crmax));
#pragma unroll
    for (int m = 32; m >= 1; m >>= 1) {
        e.ymin = pk_min(e.ymin, shx(e.ymin, m)); e.ymax = pk_max(e.ymax, shx(e.ymax, m));
        e.cbmin = pk_min(e.cbmin, shx(e.cbmin, m)); e.cbmax = pk_max(e.cbmax, shx(e.cbmax, m));
        e.crmin = pk_min(e.crmin, shx(e.crmin, m)); e.crmax = pk_max(e.crmax, shx(e.crmax, m));
    }
    const int y0 = uni(lo_of<WIN>(e.ymin)), y1 = uni(hi_of<WIN>(e.ymax));
    const int cb0 = uni(lo_of<WIN>(e.cbmin)), cb1 = uni(hi_of<WIN>(e.cbmax));
    const int cr0 = uni(lo_of<WIN>(e.crmin)), cr1 = uni(hi_of<WIN>(e.crmax));
    const int mr = TG.max_raw;
    const int4 lo = *(const int4 *)(smem + scratch_off);            // r_lo, g_lo, b_lo, r_hi
    const int2 hi = *(const int2 *)(smem + scratch_off + 16);       // g_hi, b_hi
    const int wr0 = uni(lo.x), wg0 = uni(lo.y), wb0 = uni(lo.z), wr1 = uni(lo.w), wg1 = uni(hi.x), wb1 = uni(hi.y);
    const float cell_y = L.maxf / (L.lut_max * K.ky * (PRE ? K.py : 1.0f));
    const int unit = (mr + 1) >> 8;
#pragma unroll 1
    for (int t = 0; t < 3; t++) {
        const int mc = t == 0 ? unit : (t == 1 ? (unit + 3) / 4 : 0);
        const int my = t == 2 ? 0 : (int)((t == 0 ? 1.5f : 0.5f) * cell_y);
        const int ty0 = max(y0 - my, 0), ty1 = min(y1 + my, mr);
        const int tcb0 = max(cb0 - mc, 0), tcb1 = min(cb1 + mc, mr), tcr0 = max(cr0 - mc, 0), tcr1 = min(cr1 + mc, mr);
        const Cells c = map_box<INTERP, PRE, V>(L, K, TG, (float)ty0, (float)ty1, (float)tcb0, (float)tcb1, (float)tcr0, (float)tcr1);
        const bool fits = uni((int)(c.r0 >= wr0 && c.r1 <= wr1 && c.g0 >= wg0 && c.g1 <= wg1 && c.b0 >= wb0 && c.b1 <= wb1)) != 0;
        if (fits) {
            if (lane == 0) {
                Box bx;
                bx.ylo = pack_lo<WIN>(ty0); bx.yhi = pack_hi<WIN>(ty1);
                bx.cblo = pack_lo<WIN>(tcb0); bx.cbhi = pack_hi<WIN>(tcb1);
                bx.crlo = pack_lo<WIN>(tcr0); bx.crhi = pack_hi<WIN>(tcr1);
                box_store(scratch_off, bx);
            }
            return true;
        }
    }
    return false;
}

// Neither test vouches for the tile: stage a new window around the tile's EXACT cells (spare cells on the two
// chroma-like axes as capacity allows, the luma-like axis gets the rest), then look for the largest raw box around the
// tile's raw extremes whose conservative cell map (map_box) lies inside what was staged: that box is what the cheap
// first-level test of the following tiles runs against (it may come out empty for very noisy content; those tiles then
// pay the second level).  Returns false (W untouched; the caller runs the global-gather body for this tile) when the
// tile's colours do not fit a window, or a raw code lies above 2^din - 1.
// Plane stride of a window: the smallest stride >= `nodes` for which cells one step apart on any axes never share an LDS bank
// (see tube_plane_stride in lutr_tube.h: node index = pr * A + pg * B + pb, collision when dr A + dg B + db = 0 mod 32, i.e.
// when A mod 32 lies within one of 0, +B or -B).  kGoodA[B mod 32] has bit (A mod 32) set for the strides that are fine; a
// rotate and a find-first-set pick the padding -- this runs in every restage, and every wave starts with one (a search loop
// here cost a short launch 30 us).  (Round 2's `nodes | 1` instead: profiles/r03_exp15_window_shear_padding.txt.)
__constant__ unsigned kGoodA[32] = {
    0x00000000u, 0x00000000u, 0x1ffffff0u, 0x0fffffe0u, 0x47ffffc4u, 0x63ffff8cu, 0x71ffff1cu, 0x78fffe3cu, 0x7c7ffc7cu, 0x7e3ff8fcu,
    0x7f1ff1fcu, 0x7f8fe3fcu, 0x7fc7c7fcu, 0x7fe38ffcu, 0x7ff11ffcu, 0x7ff83ffcu, 0x7ffc7ffcu, 0x7ff83ffcu, 0x7ff11ffcu, 0x7fe38ffcu,
    0x7fc7c7fcu, 0x7f8fe3fcu, 0x7f1ff1fcu, 0x7e3ff8fcu, 0x7c7ffc7cu, 0x78fffe3cu, 0x71ffff1cu, 0x63ffff8cu, 0x47ffffc4u, 0x0fffffe0u,
    0x1ffffff0u, 0x00000000u};
__constant__ unsigned short kGoodA16[16] = {      // the same for 16-byte nodes (ds_read_b128: indices collide mod 16)
    0x0000u, 0x0000u, 0x1ff0u, 0x0fe0u, 0x47c4u, 0x638cu, 0x711cu, 0x783cu, 0x7c7cu, 0x783cu, 0x711cu, 0x638cu, 0x47c4u, 0x0fe0u, 0x1ff0u, 0x0000u};
template <int NODE>
DEV int win_plane_stride(int nodes, int nb)
{
    constexpr int M = NODE == 16 ? 16 : 32;
    const int B = nb - 1, a0 = (nodes - nb) & (M - 1);
    const unsigned m = NODE == 16 ? (unsigned)kGoodA16[B & 15] : kGoodA[B & 31];
    const unsigned r = a0 ? ((m >> a0) | (m << (M - a0))) & (NODE == 16 ? 0xffffu : 0xffffffffu) : m;      // bit k: padding k is fine
    return r ? nodes + __builtin_ctz(r) : (nodes | 1);
}

template <int WIN, int INTERP, int PRE, int V>
DEV bool restage(Win &W, const LutConsts &L, const YuvConsts &K, const Geom &TG, const Ext &e_, const Bnd &bn_, int slice_off,
                 int scratch_off, int lane_)
{
    using N = Node<INTERP, V>;
    constexpr int kLN = N::lds;
    // the lane id, recomputed: kept live from the kernel's start it is the one register the strict trilinear instance spilled to scratch
    (void)lane_;
    const int lane = (int)__builtin_amdgcn_mbcnt_hi(~0u, __builtin_amdgcn_mbcnt_lo(~0u, 0u));
    Ext e = e_;
    Bnd bn = bn_;
    // side-effect free reductions would be hoisted out of the (rare) miss branch into every tile
    asm volatile("" : "+v"(e.ymin), "+v"(e.ymax), "+v"(e.cbmin), "+v"(e.cbmax), "+v"(e.crmin), "+v"(e.crmax));
    asm volatile("" : "+v"(bn.rmin), "+v"(bn.rmax), "+v"(bn.gmin), "+v"(bn.gmax), "+v"(bn.bmin), "+v"(bn.bmax));
#pragma unroll
    for (int m = 32; m >= 1; m >>= 1) {
        e.ymin = pk_min(e.ymin, shx(e.ymin, m)); e.ymax = pk_max(e.ymax, shx(e.ymax, m));
        e.cbmin = pk_min(e.cbmin, shx(e.cbmin, m)); e.cbmax = pk_max(e.cbmax, shx(e.cbmax, m));
        e.crmin = pk_min(e.crmin, shx(e.crmin, m)); e.crmax = pk_max(e.crmax, shx(e.crmax, m));
    }
    const int y0 = uni(lo_of<WIN>(e.ymin)), y1 = uni(hi_of<WIN>(e.ymax));
    const int cb0 = uni(lo_of<WIN>(e.cbmin)), cb1 = uni(hi_of<WIN>(e.cbmax));
    const int cr0 = uni(lo_of<WIN>(e.crmin)), cr1 = uni(hi_of<WIN>(e.crmax));
    const int mr = TG.max_raw;
    if (y1 > mr || cb1 > mr || cr1 > mr) return false;
    const int cap = TG.win_nodes;
    int ng = 0, nb = 0, sr = 1, nr = 0, r0 = 0, g0 = 0, b0 = 0;
    int by0 = 1, by1 = 0, bcb0 = 1, bcb1 = 0, bcr0 = 1, bcr1 = 0;             // raw box of the first-level test; empty so far
    bool placed = false;
    const float cell_y = L.maxf / (L.lut_max * K.ky * (PRE ? K.py : 1.0f));   // raw codes per lattice cell along luma
    const int unit = (mr + 1) >> 8;                                            // one 8-bit code in raw codes
    // (1) A window that covers the conservative image of the tile's raw box plus a margin: the tiles that follow then pass
    //     the cheap first-level test.  Margins from generous to none; the first whose cells fit the capacity wins.
    // (Measured: 95 % of the tiles that leave a raw box leave it through a chroma bound -- vertical colour edges that a
    // 256-px-wide tile straddles for a whole chunk.  Trading luma room for 4-6 codes of chroma margin did not pay: -0.5 %.)
#pragma unroll 1
    for (int t = 0; t < 4 && !placed; t++) {
        const int mc = t == 0 ? 2 * unit : (t == 1 ? unit : (t == 2 ? (unit + 3) / 4 : 0));
        const int my = t == 3 ? 0 : (int)((t == 0 ? 2.0f : (t == 1 ? 1.0f : 0.3f)) * cell_y);
        const int ty0 = max(y0 - my, 0), ty1 = min(y1 + my, mr);
        const int tcb0 = max(cb0 - mc, 0), tcb1 = min(cb1 + mc, mr), tcr0 = max(cr0 - mc, 0), tcr1 = min(cr1 + mc, mr);
        const Cells c = map_box<INTERP, PRE, V>(L, K, TG, (float)ty0, (float)ty1, (float)tcb0, (float)tcb1, (float)tcr0, (float)tcr1);
        // corners: r..r+1, (g-r)-1..(g-r)+1, (b-r)-1..(b-r)+1
        const int need_r = uni(c.r1 - c.r0 + 2), need_g = uni(c.g1 - c.g0 + 3), need_b = uni(c.b1 - c.b0 + 3);
        if (need_r < 2 || need_g < 3 || need_b < 3 || need_g > 128 || need_b > 128) continue;
        // odd row and plane strides: the nodes of neighbouring cells (the ones a wave reads together) differ by +-1, +-nb,
        // +-(sr - nb - 1) and small sums of those -- kept away from multiples of 16 nodes, i.e. from the same LDS banks
        const int nb_ = need_b | 1;
        const int sr_ = win_plane_stride<kLN>(need_g * nb_, nb_), nr_ = cap / sr_;
        if (nr_ < need_r) continue;
        ng = need_g; nb = nb_; sr = sr_; nr = nr_;
        r0 = uni(c.r0) - ((nr - need_r) >> 1); g0 = uni(c.g0) - 1; b0 = uni(c.b0) - 1;
        by0 = ty0; by1 = ty1; bcb0 = tcb0; bcb1 = tcb1; bcr0 = tcr0; bcr1 = tcr1;
        placed = true;
        // the luma-like axis got whatever capacity was left: widen the luma range of the box to match, if the map agrees
        const int room = (nr - need_r) >> 1;
        if (room > 0) {
            const int my2 = my + (int)(0.8f * (float)room * cell_y);
            const int uy0 = max(y0 - my2, 0), uy1 = min(y1 + my2, mr);
            const Cells c2 = map_box<INTERP, PRE, V>(L, K, TG, (float)uy0, (float)uy1, (float)tcb0, (float)tcb1, (float)tcr0, (float)tcr1);
            const bool fits = uni((int)(c2.r0 >= r0 && c2.r1 <= r0 + nr - 2 && c2.g0 >= g0 + 1 && c2.g1 <= g0 + ng - 2 &&
                                        c2.b0 >= b0 + 1 && c2.b1 <= b0 + nb - 2)) != 0;
            if (fits) { by0 = uy0; by1 = uy1; }
        }
    }
    if (!placed) {
        // (2) The raw box is too loose a description of this tile (an edge between two colours: Cb and Cr move together,
        //     the box spans every combination).  Stage around the tile's EXACT cells; the first-level box stays empty and
        //     the tiles that follow are vouched for by the second-level test.
        const int rmin = uni(wave_min_i(bn.rmin)), rmax = uni(wave_max_i(bn.rmax));
        const int gmin = uni(wave_min_i(bn.gmin)), gmax = uni(wave_max_i(bn.gmax));
        const int bmin = uni(wave_min_i(bn.bmin)), bmax = uni(wave_max_i(bn.bmax));
        const int need_r = rmax - rmin + 2, need_g = gmax - gmin + 3, need_b = bmax - bmin + 3;
        int spare = 1;
        for (;;) {                                   // one spare cell on each side of the chroma-like axes if it fits
            ng = need_g + 2 * spare; nb = (need_b + 2 * spare) | 1;
            sr = win_plane_stride<kLN>(ng * nb, nb);
            nr = cap / sr;
            if (nr >= need_r + 2 * spare || spare == 0) break;
            spare--;
        }
        if (need_r > nr || ng > 128 || nb > 128) return false;
        r0 = rmin - ((nr - need_r) >> 1);
        g0 = gmin - 1 - spare;
        b0 = bmin - 1 - spare;
    }
    // cells whose 8 corners are staged
    const int wr0 = r0, wr1 = r0 + nr - 2, wg0 = g0 + 1, wg1 = g0 + ng - 2, wb0 = b0 + 1, wb1 = b0 + nb - 2;

    const int n1 = L.n1, nmax = L.n1 - 1;
    const int plane = ng * nb, total = nr * plane;
    // i -> (ir, ig, ib) by float reciprocals: floor(i / d) == (int)((i + 0.5) * (1 / d)) while the quotient stays below 2^7 and
    // d below 2^12 (error of the product < 2^-16, distance of (i + 0.5) / d from an integer >= 2^-13; d <= window capacity); every product fits 24 bits
    const float rcp_plane = 1.0f / (float)plane, rcp_nb = 1.0f / (float)nb;
    // Batches of kB nodes per lane: all kB global reads are issued before the first LDS write, so a restage costs about
    // one L2 round trip per batch instead of one per node (the wave is stalled meanwhile; 4 waves per SIMD cannot hide it).
    constexpr int kB = 6;          // (9 and 18 for the 8-byte nodes of the fast windows were measured: no difference)
    for (int base = 0; base < total; base += 64 * kB) {
        int dst[kB];
        typename std::conditional<N::fast, uint2, float4>::type val[kB];
        uint2 val1[N::rec ? kB : 1];                                          // records: the r + 1 neighbour
#pragma unroll
        for (int k = 0; k < kB; k++) {
            const int i = min(base + k * 64 + lane, total - 1);              // the last batch re-reads the final node: harmless
            const int ir = (int)(((float)i + 0.5f) * rcp_plane), rem = i - __mul24(ir, plane);
            const int ig = (int)(((float)rem + 0.5f) * rcp_nb), ib = rem - __mul24(ig, nb);
            int r = r0 + ir, g = r + g0 + ig, b = g + b0 + ib;
            // nodes outside the cube are never referenced by a valid pixel: clamp to stay inside the lattice
            r = min(max(r, 0), nmax); g = min(max(g, 0), nmax); b = min(max(b, 0), nmax);
            const int src = __mul24(__mul24(r, n1) + g, n1) + b;
            dst[k] = slice_off + kLN * (__mul24(ir, sr) + __mul24(ig, nb) + ib);
            if constexpr (N::fast) val[k] = L.lat16[src];
            else val[k] = L.lat[src];
            if constexpr (N::rec) val1[k] = L.lat16[__mul24(__mul24(min(r + 1, nmax), n1) + g, n1) + b];
        }
#pragma unroll
        for (int k = 0; k < kB; k++) {
            char *q = smem + dst[k];
            if constexpr (N::rec) { const u3 rc = make_rec(val[k], val1[k]); ((uint32_t *)q)[0] = rc.x; ((uint32_t *)q)[1] = rc.y; ((uint32_t *)q)[2] = rc.z; }
            else if constexpr (N::fast) *(uint2 *)q = val[k];
            else if constexpr (kLN == 16) *(float4 *)q = val[k];
            else { ((float *)q)[0] = val[k].x; ((float *)q)[1] = val[k].y; ((float *)q)[2] = val[k].z; }
        }
    }
    if (lane == 0) {
        *(int4 *)(smem + scratch_off) = make_int4(wr0, wg0, wb0, wr1);
        *(int2 *)(smem + scratch_off + 16) = make_int2(wg1, wb1);
    }
    // node index = (pr-r0)*sr + (pg-pr-g0)*nb + (pb-pg-b0)
    W.o_r = kLN * (sr - nb); W.o_g = kLN * (nb - 1);
    W.fr = (float)W.o_r; W.fg = (float)W.o_g; W.fb = (float)kLN;
    W.fc = as_tiny(lds_base() + slice_off - kLN * (r0 * sr + g0 * nb + b0));
    if (lane == 0) {
        Box bx;
        if (by1 >= by0) {
            bx.ylo = pack_lo<WIN>(by0); bx.yhi = pack_hi<WIN>(by1);
            bx.cblo = pack_lo<WIN>(bcb0); bx.cbhi = pack_hi<WIN>(bcb1);
            bx.crlo = pack_lo<WIN>(bcr0); bx.crhi = pack_hi<WIN>(bcr1);
        } else {
            bx.ylo = bx.cblo = bx.crlo = 0xffffffffu; bx.yhi = bx.cbhi = bx.crhi = 0u;      // empty: lo > hi
        }
        box_store(scratch_off, bx);
    }
    return true;
}

// ---------------------------------------------------------------- one pixel
struct PxC {
    int a;                  // byte address (LDS) or byte offset (global) of the c000 tap
    int oa, oz;             // tetrahedral: byte offsets of the 2nd and 3rd taps
    f2v w01, w23;           // tetrahedral weights {w0, w1}, {w2, w3} as register pairs; trilinear keeps {d.r, d.g}, {d.b, -}
};
struct Rgb3 { float r, g, b; };

template <bool LDS, int INTERP, int V>
DEV PxC px_finish(const LutConsts &L, const Win &W, const CrdI &cr, const CrdI &cg, const CrdI &cb)
{
    using N = Node<INTERP, V>;
    constexpr int nb_ = LDS ? N::lds : N::glb;
    PxC c;
    if constexpr (LDS) {
        // exact (Win): the cells' bits are the operands, the result's bits are the address; the box test guarantees it is inside the slice
        c.a = __float_as_int(fma_(__int_as_float(cr.p), W.fr, fma_(__int_as_float(cg.p), W.fg, fma_(__int_as_float(cb.p), W.fb, W.fc))));
    } else {
        c.a = ((cr.p * L.n1 + cg.p) * L.n1 + cb.p) * nb_;
    }
    c.oa = c.oz = 0;
    c.w01 = f2v{0.0f, 0.0f}; c.w23 = f2v{0.0f, 0.0f};
    if constexpr (INTERP == LUTR_INTERP_TRILINEAR) {
        c.w01.x = cr.d; c.w01.y = cg.d; c.w23.x = cb.d;
    } else if constexpr (INTERP == LUTR_INTERP_TETRAHEDRAL || INTERP == T2_TET16) {
        // FFmpeg's six branches all evaluate (1-x) c000 + (x-y) cA + (y-z) cB + z c111 with (x,y,z) the fractions sorted
        // descending; ties only ever choose between taps whose weight is exactly 0 (finite lattice), so the sorted form is
        // bit-identical.
        const float dr = cr.d, dg = cg.d, db = cb.d;
        const float x = fmaxf(fmaxf(dr, dg), db), y = med3(dr, dg, db), z = fminf(fminf(dr, dg), db);
        const bool rg = dr > dg, gb = dg > db, rb = dr > db;
        const int o_r = LDS ? W.o_r : nb_ * L.n1 * L.n1, o_g = LDS ? W.o_g : nb_ * L.n1, o_b = nb_;
        const int z_r = o_g + o_b, z_g = o_r + o_b, z_b = o_r + o_g;         // o111 minus the step of the smallest fraction
        c.oa = (rg && rb) ? o_r : (gb ? o_g : o_b);
        c.oz = (gb && rb) ? z_b : (rg ? z_g : z_r);
        c.w01.x = 1.0f - x; c.w01.y = x - y; c.w23.x = y - z; c.w23.y = z;
    }
    return c;
}

// strict taps: one node as floats
template <bool LDS, int NB>
DEV f4 tap(const LutConsts &L, int a)
{
    if constexpr (LDS && NB == 16) {
        return *(const __attribute__((address_space(3))) f4 *)(uintptr_t)(unsigned)a;
    } else if constexpr (LDS) {
        const __attribute__((address_space(3))) float *p = (const __attribute__((address_space(3))) float *)(uintptr_t)(unsigned)a;
        f4 v; v.x = p[0]; v.y = p[1]; v.z = p[2]; v.w = 0.0f;
        return v;
    } else {
        return *(const f4 *)((const char *)L.lat + a);
    }
}
// fast taps: one node as two words {r | g << 16, b} of fp16
template <bool LDS>
DEV u2 tap16(const LutConsts &L, int a)
{
    if constexpr (LDS) return *(const __attribute__((address_space(3))) u2 *)(uintptr_t)(unsigned)a;
    else return *(const u2 *)((const char *)L.lat16 + a);
}

// The taps of one pixel, loaded in one go so that several pixels' reads are in flight together (tile_body phases).
template <bool LDS, int INTERP, int V> struct Taps {
    static constexpr bool rec = LDS && Node<INTERP, V>::rec;          // four records instead of eight nodes
    static constexpr int n = rec ? 4 : (INTERP == LUTR_INTERP_TRILINEAR ? 8 : (INTERP == LUTR_INTERP_NEAREST ? 1 : 4));
    typename std::conditional<rec, u3, typename std::conditional<V == V_FAST, u2, f4>::type>::type t[n];
};
DEV u3 tap_rec(int a)
{
    const __attribute__((address_space(3))) uint32_t *p = (const __attribute__((address_space(3))) uint32_t *)(uintptr_t)(unsigned)a;
    return u3{p[0], p[1], p[2]};
}

template <bool LDS, int INTERP, int V>
DEV Taps<LDS, INTERP, V> px_taps(const LutConsts &L, const Win &W, const PxC &c)
{
    using N = Node<INTERP, V>;
    constexpr int nb_ = LDS ? N::lds : N::glb;
    const int o_r = LDS ? W.o_r : nb_ * L.n1 * L.n1, o_g = LDS ? W.o_g : nb_ * L.n1;
    const int a = c.a;
    Taps<LDS, INTERP, V> T;
    if constexpr (Taps<LDS, INTERP, V>::rec) {
        const int ag = a + o_g;
        T.t[0] = tap_rec(a); T.t[1] = tap_rec(a + nb_); T.t[2] = tap_rec(ag); T.t[3] = tap_rec(ag + nb_);      // c00x c01x ... : (g, b) corners
        return T;
    } else {
    auto ld = [&](int addr) {
        if constexpr (N::fast) return tap16<LDS>(L, addr);
        else return tap<LDS, nb_>(L, addr);
    };
    if constexpr (INTERP == LUTR_INTERP_NEAREST) {
        T.t[0] = ld(a);
    } else if constexpr (INTERP == LUTR_INTERP_TRILINEAR) {
        const int ag = a + o_g, ar = a + o_r, arg = ar + o_g;
        T.t[0] = ld(a); T.t[1] = ld(a + nb_); T.t[2] = ld(ag); T.t[3] = ld(ag + nb_);       // c000 c001 c010 c011
        T.t[4] = ld(ar); T.t[5] = ld(ar + nb_); T.t[6] = ld(arg); T.t[7] = ld(arg + nb_);   // c100 c101 c110 c111
    } else {
        T.t[0] = ld(a); T.t[1] = ld(a + c.oa); T.t[2] = ld(a + c.oz); T.t[3] = ld(a + o_r + o_g + nb_);
    }
    return T;
    }
}

// MIXED tiles: a lane outside the tube computed its coordinates, fractions and weights like every other lane -- none of that depends
// on where the nodes live -- but its LDS reads returned whatever its address pointed at.  Fetch the pixel's taps from the global
// lattice (float4 nodes, blue fastest: the gather body's index) over the LDS results; the blend and everything after it run once.
// A and the steps are exact: prev <= N - 1 in the (N + 1)^3 copy, every product below 2^24.  12 bytes per tap: {r, g, b}.
template <int INTERP, int V>
DEV void patch_taps(const LutConsts &L, const CrdI &cr, const CrdI &cg, const CrdI &cb, Taps<true, INTERP, V> &T)
{
    static_assert(V != V_FAST, "the fast kernels have no mixed tiles");
    unsigned n1 = (unsigned)L.n1;
    asm volatile("" : "+s"(n1));      // (opaque: the steps are two scalar instructions here; hoisted out of the tile loop they are spilled SGPRs)
    const unsigned o_g = 16u * n1, o_r = o_g * n1, o_b = 16u;
    const unsigned a = (__umul24(__umul24((unsigned)cr.p, n1) + (unsigned)cg.p, n1) + (unsigned)cb.p) << 4;
    auto ld = [&](unsigned off, f4 &t) {
        const float *p = (const float *)((const char *)L.lat + off);
        t.x = p[0]; t.y = p[1]; t.z = p[2];
    };
    if constexpr (INTERP == LUTR_INTERP_NEAREST) {
        ld(a, T.t[0]);
    } else if constexpr (INTERP == LUTR_INTERP_TRILINEAR) {
        const unsigned ag = a + o_g, ar = a + o_r, arg = ar + o_g;
        ld(a, T.t[0]); ld(a + o_b, T.t[1]); ld(ag, T.t[2]); ld(ag + o_b, T.t[3]);
        ld(ar, T.t[4]); ld(ar + o_b, T.t[5]); ld(arg, T.t[6]); ld(arg + o_b, T.t[7]);
    } else {
        // px_finish's two selects with the global steps
        const float dr = cr.d, dg = cg.d, db = cb.d;
        const bool rg = dr > dg, gb = dg > db, rb = dr > db;
        const unsigned oa = (rg && rb) ? o_r : (gb ? o_g : o_b);
        const unsigned a111 = a + (o_r + o_g + o_b);
        const unsigned az = a111 - ((gb && rb) ? o_b : (rg ? o_g : o_r));       // c111 minus the step of the smallest fraction
        ld(a, T.t[0]); ld(a + oa, T.t[1]); ld(az, T.t[2]); ld(a111, T.t[3]);
    }
}

// lattice value as the integer code it quantises to, held as float
template <bool LDS, int INTERP, int V>
DEV Rgb3 px_blend(const LutConsts &L, const PxC &c, const Taps<LDS, INTERP, V> &T)
{
    Rgb3 v;
    if constexpr (Taps<LDS, INTERP, V>::rec) {
        // records {r | g << 16, b | Dr << 16, Dg | Db << 16} of the (g, b) corners 00, 01 (b + 1), 10 (g + 1), 11
        const float dr = c.w01.x, dg = c.w01.y, db = c.w23.x;
        {
            const float c00 = reclerp<1, 0>(T.t[0].y, dr, T.t[0].x), c01 = reclerp<1, 0>(T.t[1].y, dr, T.t[1].x);
            const float c10 = reclerp<1, 0>(T.t[2].y, dr, T.t[2].x), c11 = reclerp<1, 0>(T.t[3].y, dr, T.t[3].x);
            const float c0 = fma_(c10 - c00, dg, c00), c1 = fma_(c11 - c01, dg, c01);
            v.r = fma_(c1 - c0, db, c0);
        }
        {
            const float c00 = reclerp<0, 1>(T.t[0].z, dr, T.t[0].x), c01 = reclerp<0, 1>(T.t[1].z, dr, T.t[1].x);
            const float c10 = reclerp<0, 1>(T.t[2].z, dr, T.t[2].x), c11 = reclerp<0, 1>(T.t[3].z, dr, T.t[3].x);
            const float c0 = fma_(c10 - c00, dg, c00), c1 = fma_(c11 - c01, dg, c01);
            v.g = fma_(c1 - c0, db, c0);
        }
        {
            const float c00 = reclerp<1, 0>(T.t[0].z, dr, T.t[0].y), c01 = reclerp<1, 0>(T.t[1].z, dr, T.t[1].y);
            const float c10 = reclerp<1, 0>(T.t[2].z, dr, T.t[2].y), c11 = reclerp<1, 0>(T.t[3].z, dr, T.t[3].y);
            const float c0 = fma_(c10 - c00, dg, c00), c1 = fma_(c11 - c01, dg, c01);
            v.b = fma_(c1 - c0, db, c0);
        }
        return v;
    } else
    if constexpr (V == V_FAST) {
        // nodes are fp16 of (lattice * M): the blend IS the code before truncation.  v_fma_mix_f32 takes the fp16 tap as it
        // is (exact conversion inside the instruction), fp32 weight, fp32 accumulator: one rounding per step.
        if constexpr (INTERP == LUTR_INTERP_NEAREST) {
            v.r = mix0_lo(1.0f, T.t[0].x); v.g = mix0_hi(1.0f, T.t[0].x); v.b = mix0_lo(1.0f, T.t[0].y);
        } else if constexpr (INTERP == LUTR_INTERP_TRILINEAR) {
            const float dr = c.w01.x, dg = c.w01.y, db = c.w23.x;
            // (with records in LDS this is the gather body: its differences are rounded to fp16 as the staged ones are)
#define TRI16(SUB_, LERP_, W_, out) \
            { \
                auto SUB = [](uint32_t a_, uint32_t b_) { \
                    const float d_ = SUB_(a_, b_); \
                    if constexpr (Node<INTERP, V>::rec) return (float)(_Float16)d_; else return d_; \
                }; \
                auto LERP = [](float t_, float f_, uint32_t v0_) { return LERP_(t_, f_, v0_); }; \
                const float c00 = LERP(SUB(T.t[4].W_, T.t[0].W_), dr, T.t[0].W_), c10 = LERP(SUB(T.t[6].W_, T.t[2].W_), dr, T.t[2].W_); \
                const float c01 = LERP(SUB(T.t[5].W_, T.t[1].W_), dr, T.t[1].W_), c11 = LERP(SUB(T.t[7].W_, T.t[3].W_), dr, T.t[3].W_); \
                const float c0 = fma_(c10 - c00, dg, c00), c1 = fma_(c11 - c01, dg, c01); \
                out = fma_(c1 - c0, db, c0); \
            }
            TRI16(hsub_lo, hlerp_lo, x, v.r) TRI16(hsub_hi, hlerp_hi, x, v.g) TRI16(hsub_lo, hlerp_lo, y, v.b)
#undef TRI16
        } else {
            const float w0 = c.w01.x, w1 = c.w01.y, w2 = c.w23.x, w3 = c.w23.y;
            v.r = mix_lo(w3, T.t[3].x, mix_lo(w2, T.t[2].x, mix_lo(w1, T.t[1].x, mix0_lo(w0, T.t[0].x))));
            v.g = mix_hi(w3, T.t[3].x, mix_hi(w2, T.t[2].x, mix_hi(w1, T.t[1].x, mix0_hi(w0, T.t[0].x))));
            v.b = mix_lo(w3, T.t[3].y, mix_lo(w2, T.t[2].y, mix_lo(w1, T.t[1].y, mix0_lo(w0, T.t[0].y))));
        }
        return v;
    } else if constexpr (V == V_FMA32) {
        // nodes are fp32 of (lattice * M), each a single rounding: the blend is the code before truncation, one rounding per
        // step.  Same taps and weights as strict; FFmpeg's tetrahedral order w0 c000 + w1 cA + w2 cB + w3 c111, and its
        // trilinear lerps as fma(v1 - v0, f, v0).
        if constexpr (INTERP == LUTR_INTERP_NEAREST) {
            v.r = T.t[0].x; v.g = T.t[0].y; v.b = T.t[0].z;
        } else if constexpr (INTERP == LUTR_INTERP_TRILINEAR) {
            const float dr = c.w01.x, dg = c.w01.y, db = c.w23.x;
            auto lerp = [](float v0, float v1, float f) { return fma_(v1 - v0, f, v0); };
#define TRI(ch, out) \
            { \
                const float c00 = lerp(T.t[0].ch, T.t[4].ch, dr), c10 = lerp(T.t[2].ch, T.t[6].ch, dr); \
                const float c01 = lerp(T.t[1].ch, T.t[5].ch, dr), c11 = lerp(T.t[3].ch, T.t[7].ch, dr); \
                const float c0 = lerp(c00, c10, dg), c1 = lerp(c01, c11, dg); \
                out = lerp(c0, c1, db); \
            }
            // (one channel at a time: interleaved, 8-bit 4:2:0 with the prologue spilled five VGPRs)
            TRI(x, v.r) __builtin_amdgcn_sched_barrier(0); TRI(y, v.g) __builtin_amdgcn_sched_barrier(0); TRI(z, v.b)
#undef TRI
        } else {
            const float w0 = c.w01.x, w1 = c.w01.y, w2 = c.w23.x, w3 = c.w23.y;
            v.r = fma_(w3, T.t[3].x, fma_(w2, T.t[2].x, fma_(w1, T.t[1].x, w0 * T.t[0].x)));
            v.g = fma_(w3, T.t[3].y, fma_(w2, T.t[2].y, fma_(w1, T.t[1].y, w0 * T.t[0].y)));
            v.b = fma_(w3, T.t[3].z, fma_(w2, T.t[2].z, fma_(w1, T.t[1].z, w0 * T.t[0].z)));
        }
        return v;
    } else {
        if constexpr (INTERP == LUTR_INTERP_NEAREST) {
            v.r = T.t[0].x; v.g = T.t[0].y; v.b = T.t[0].z;
        } else if constexpr (INTERP == LUTR_INTERP_TRILINEAR) {
            const float dr = c.w01.x, dg = c.w01.y, db = c.w23.x;
#define TRI(ch, out) \
            { \
                const float c00 = tlerp(T.t[0].ch, T.t[4].ch, dr), c10 = tlerp(T.t[2].ch, T.t[6].ch, dr); \
                const float c01 = tlerp(T.t[1].ch, T.t[5].ch, dr), c11 = tlerp(T.t[3].ch, T.t[7].ch, dr); \
                const float c0 = tlerp(c00, c10, dg), c1 = tlerp(c01, c11, dg); \
                out = tlerp(c0, c1, db); \
            }
            TRI(x, v.r) TRI(y, v.g) TRI(z, v.b)
#undef TRI
        } else {
            const float w0 = c.w01.x, w1 = c.w01.y, w2 = c.w23.x, w3 = c.w23.y;
            v.r = w0 * T.t[0].x + w1 * T.t[1].x + w2 * T.t[2].x + w3 * T.t[3].x;
            v.g = w0 * T.t[0].y + w1 * T.t[1].y + w2 * T.t[2].y + w3 * T.t[3].y;
            v.b = w0 * T.t[0].z + w1 * T.t[1].z + w2 * T.t[2].z + w3 * T.t[3].z;
        }
        v.r *= L.maxf; v.g *= L.maxf; v.b *= L.maxf;
        return v;
    }
}

// (int)(v * M) clipped to [0, M]; V >= V_UNIT: every lattice node lies in [0, 1], the truncation alone lands in [0, M]
// (all weights and nodes >= 0, rounding of products and sums is monotone): the clip is dead code.
template <int INTERP, int V>
DEV Rgb3 px_quant(const LutConsts &L, const Rgb3 &v)
{
    Rgb3 o;
    // (Measured for the fast tetrahedral kernel: rounding by two full-rate adds of 1.5 * 2^23 on a chain started at -0.5 + 2^-12
    // instead of the quarter-rate v_trunc_f32 -- three more instructions per pixel, 3 % slower: instruction issue binds first.)
    if constexpr (V >= V_UNIT) { o.r = truncf(v.r); o.g = truncf(v.g); o.b = truncf(v.b); }
    else { o.r = med3(truncf(v.r), 0.0f, L.maxf); o.g = med3(truncf(v.g), 0.0f, L.maxf); o.b = med3(truncf(v.b), 0.0f, L.maxf); }
    return o;
}

template <bool DEAD> DEV float ofloor(float v, float hi) { if constexpr (DEAD) return v; else return fminf(v, hi); }

// ---------------------------------------------------------------- tile body
// Coordinates of the four pixels of a group (phase A): twelve table reads (or their computed twins) issued back to back.
struct GroupCrd { CrdI r[4], g[4], b[4]; };

template <bool LDS, int WIN, int WOUT, int CSX, int CSY, int INTERP, int PRE, int V>
DEV void group_coords(const LutConsts &L, const YuvConsts &K, const Geom &TG, const TileIn<WIN, WOUT, CSX, CSY> &in, int g, GroupCrd &q)
{
    using T = Tile<WIN, WOUT, CSX, CSY>;
    constexpr int GW = 4 / T::BH, NCG = (GW >> CSX) > 0 ? (GW >> CSX) : 1;
    float rv[NCG], gv[NCG], bu[NCG];
#pragma unroll
    for (int c = 0; c < NCG; c++) {
        const int j = g * NCG + c;
        float cbv = wsample<WIN>(in.cb, j), crv = wsample<WIN>(in.cr, j);
        if constexpr (PRE) {
            cbv = cfloor(fma_(K.pc, cbv, K.pcb), K.pre_max);
            crv = cfloor(fma_(K.pc, crv, K.pcb), K.pre_max);
        }
        const float cbd = cbv - K.coff, crd = crv - K.coff;
        rv[c] = K.krv * crd; gv[c] = fma_(K.kgu, cbd, K.kgv * crd); bu[c] = K.kbu * cbd;
    }
#pragma unroll
    for (int p = 0; p < 4; p++) {
        const int dy = p / GW, i = g * GW + p % GW, c = (p % GW) >> CSX;
        float yv = wsample<WIN>(in.y[dy], i);
        if constexpr (PRE) yv = cfloor(fma_(K.py, yv, K.pyb), K.pre_max);
        const float yy = fma_(K.ky, yv, K.yb);
        if constexpr (V >= V_TAB) {
            // clip(floor(v), 0, M): v_cvt_u32_f32 floors and saturates negatives to 0; the table is padded past M
            // K is the kernel's KB here: sums are 8 x the code, the masked conversion is the table's byte offset
            unsigned ri = (unsigned)(yy + rv[c]) & ~7u, gi = (unsigned)(yy + gv[c]) & ~7u, bi = (unsigned)(yy + bu[c]) & ~7u;
            if constexpr (!LDS) {           // the gather body also serves tiles with raw codes nobody vouched for
                const unsigned top = (unsigned)(TG.tab_entries - 1) * 8u;
                ri = min(ri, top); gi = min(gi, top); bi = min(bi, top);
            }
            q.r[p] = crd_table8i(ri); q.g[p] = crd_table8i(gi); q.b[p] = crd_table8i(bi);
        } else {
            const float rq = cfloor(yy + rv[c], K.max_l), gq = cfloor(yy + gv[c], K.max_l), bq = cfloor(yy + bu[c], K.max_l);
            q.r[p] = crd_int(crd_compute<INTERP>(L, rq, L.sc[0])); q.g[p] = crd_int(crd_compute<INTERP>(L, gq, L.sc[1]));
            q.b[p] = crd_int(crd_compute<INTERP>(L, bq, L.sc[2]));
        }
    }
}

// One tile.  Every LDS result is requested well before it is used, inside the wave: with four waves per SIMD (the
// register budget) the hardware alone cannot hide an LDS round trip per pixel.  Order per group g:
//   A(g)    coordinate reads of the group            (12 ds_read_b64)
//   B(g)    tap addresses + weights, then tap reads  (TB pixels' taps in flight together)
//   C(g)    blends, truncation, RGB -> YUV, packing
// sched_barrier keeps the machine scheduler from sinking the reads back next to their uses; the zero-instruction
// fences at the end of a group keep instruction selection from hoisting every group to the top (> 1000 spilled registers).
// (Measured and removed, each behind a build switch: issuing A(g+1) before C(g) -- +4 % for the strict kernels while they had the
// registers, with the tube state live it spills: -2.7 %, DESIGN.md 5.2 "Scheduling"; fencing every input and output word instead of
// the live ones keeps 2 x 12 registers allocated through the tile; the window's address factors and the chroma rows copied to VGPRs
// per tile: no gain)
// MIX (the LDS body of a mixed tile): `outside` has bit j set when chroma sample j of the lane's unit is outside the tube (all bits where
// the test has the lane's verdict only).  A group whose samples are inside needs nothing; elsewhere the lane re-reads the taps of the
// batch from the global lattice (patch_taps) under a divergent branch the wave skips when no lane wants it.
template <bool LDS, int WIN, int WOUT, int CSX, int CSY, int INTERP, int PRE, int V, bool MIX = false>
DEV void tile_body(const LutConsts &L, const YuvConsts &K_, const Win &W_, const Geom &TG, TileIn<WIN, WOUT, CSX, CSY> &in,
                   TileOut<WIN, WOUT, CSX, CSY> &out, unsigned outside = 0u)
{
    static_assert(LDS || !MIX, "the patch belongs to the LDS body");
    Win W = W_;              // (local copies: through the references alone every instance gets another register allocation)
    YuvConsts K = K_;
    using T = Tile<WIN, WOUT, CSX, CSY>;
    // a group = 4 pixels: all BH rows of GW columns; it owns NCG chroma samples
    constexpr int GW = 4 / T::BH, NG = T::PXT / GW, NCG = (GW >> CSX) > 0 ? (GW >> CSX) : 1;
    constexpr bool kDead = V >= V_UNIT;          // launcher checked the RGB->YUV maxima too (out_clip_dead)
    // tap batches of the fast 4-tap kernels: 4 pixels (2 and 1 were measured behind a build switch)
    constexpr int TB = INTERP == LUTR_INTERP_TRILINEAR ? (V == V_FAST ? 2 : 1) : (INTERP == LUTR_INTERP_NEAREST ? 4 : (V == V_FAST ? 4 : 2));
    // (two slots, one used: the second is what is left of the removed cross-group pipeline.  A single GroupCrd compiles the general
    // 4:2:2 tetrahedral instances to three adds with their operands swapped, and this file's device code is held bit for bit.)
    GroupCrd cq[2];
#pragma unroll
    for (int g = 0; g < NG; g++) {
        GroupCrd &q = cq[0];
        group_coords<LDS, WIN, WOUT, CSX, CSY, INTERP, PRE, V>(L, K, TG, in, g, q);
        __builtin_amdgcn_sched_barrier(0);
        Rgb3 o[4];
#pragma unroll
        for (int qb = 0; qb < 4; qb += TB) {
            PxC pc[TB];
            Taps<LDS, INTERP, V> tp[TB];
#pragma unroll
            for (int t = 0; t < TB; t++) {
                pc[t] = px_finish<LDS, INTERP, V>(L, W, q.r[qb + t], q.g[qb + t], q.b[qb + t]);
                tp[t] = px_taps<LDS, INTERP, V>(L, W, pc[t]);
            }
            if constexpr (MIX) {
                // (opaque per batch: the batches of a group test the same bits, and merged under one branch their taps -- four
                // pixels' -- would all be live at once)
                unsigned want = (outside >> (g * NCG)) & ((1u << NCG) - 1u);
                asm volatile("" : "+v"(want));
                if (want) {
#pragma unroll
                    for (int t = 0; t < TB; t++) patch_taps<INTERP, V>(L, q.r[qb + t], q.g[qb + t], q.b[qb + t], tp[t]);
                }
            }
            __builtin_amdgcn_sched_barrier(0);
#pragma unroll
            for (int t = 0; t < TB; t++) {
                o[qb + t] = px_quant<INTERP, V>(L, px_blend<LDS, INTERP, V>(L, pc[t], tp[t]));
                // (the patch's branch ends a basic block: keep this batch's blend in front of the next one's)
                if constexpr (MIX) asm volatile("" : "+v"(o[qb + t].r), "+v"(o[qb + t].g), "+v"(o[qb + t].b));
            }
        }
        float rs[NCG], gs[NCG], bs[NCG];
#pragma unroll
        for (int p = 0; p < 4; p++) {
            const int dy = p / GW, i = g * GW + p % GW, c = (p % GW) >> CSX;
            if (dy == 0 && ((p % GW) & (T::BW - 1)) == 0) { rs[c] = o[p].r; gs[c] = o[p].g; bs[c] = o[p].b; }
            else { rs[c] += o[p].r; gs[c] += o[p].g; bs[c] += o[p].b; }
            wput<WOUT>(out.y[dy], i, ofloor<kDead>(fma_(K.cyr, o[p].r, fma_(K.cyg, o[p].g, fma_(K.cyb, o[p].b, K.yob))), K.max_o));
        }
#pragma unroll
        for (int c = 0; c < NCG; c++) {
            const int j = g * NCG + c;
            wput<WOUT>(out.cb, j, ofloor<kDead>(fma_(K.cbr, rs[c], fma_(K.cbg, gs[c], fma_(K.cbb, bs[c], K.cob))), K.max_o));
            wput<WOUT>(out.cr, j, ofloor<kDead>(fma_(K.crr, rs[c], fma_(K.crg, gs[c], fma_(K.crb, bs[c], K.cob))), K.max_o));
        }
        // Only what is live anyway: the input words later groups still read (they cannot start before this point) and the
        // output words this group wrote (it cannot finish after it).  Fencing consumed input words or unborn output words
        // would keep 2 x 12 registers allocated through the whole tile.
        if (g + 1 < NG) {
            constexpr int ISH = WIN ? 1 : 2;
            const int y0 = ((g + 1) * GW) >> ISH, c0 = ((g + 1) * NCG) >> ISH;
#pragma unroll
            for (int dy = 0; dy < T::BH; dy++)
#pragma unroll
                for (int k = 0; k < T::YWI; k++) if (k >= y0) fence_words<1>(&in.y[dy][k]);
#pragma unroll
            for (int k = 0; k < T::CWI; k++) if (k >= c0) { fence_words<1>(&in.cb[k]); fence_words<1>(&in.cr[k]); }
        }
        {
            constexpr int OSH = WOUT ? 1 : 2;
            const int y0 = (g * GW) >> OSH, y1 = ((g + 1) * GW - 1) >> OSH, c0 = (g * NCG) >> OSH, c1 = ((g + 1) * NCG - 1) >> OSH;
#pragma unroll
            for (int dy = 0; dy < T::BH; dy++)
#pragma unroll
                for (int k = 0; k < T::YWO; k++) if (k >= y0 && k <= y1) fence_words<1>(&out.y[dy][k]);
#pragma unroll
            for (int k = 0; k < T::CWO; k++) if (k >= c0 && k <= c1) { fence_words<1>(&out.cb[k]); fence_words<1>(&out.cr[k]); }
        }
    }
}

template <int WIN, int WOUT, int CSX, int CSY, int INTERP, int PRE, int V>
__global__ __launch_bounds__(64 * LUTR_T2_WPB, LUTR_T2_WAVES_PER_EU)
void k_yuv_tile2(LutConsts L_, YuvConsts K_, Planes2 P, FrameGeom G, Geom TG)
{
    using T = Tile<WIN, WOUT, CSX, CSY>;
    using N = Node<INTERP, V>;
    // mixed tiles: the strict kernels (see the vote below); not trilinear with the prologue, whose body has no register left for the
    // lanes' verdict (it spilled three VGPRs to scratch inside the body)
    // (likewise 8-bit 4:4:4 trilinear: eight spilled registers, and fma32 trilinear: three in the headline layout)
    // (mixed tiles for the fast kernels too, measured behind a build switch: sigma-16 frames 512 -> 537 Gpx/s, natural 662 -> 655,
    // saturated 530 -> 522, 10 more VGPRs: profiles/r03_exp34_mixed_tiles_fast_kernels.txt)
    // (only the table variants ever stage a tube, and T2_TET16 is the whole-lattice mode: no tube, no mixed tiles)
    constexpr bool kMixed = V != V_FAST && V >= V_TAB && INTERP != T2_TET16 &&
                            !(INTERP == LUTR_INTERP_TRILINEAR && (PRE || (!WIN && !CSX) || V == V_FMA32));
    // A mixed tile runs ONE body: the tube body with the outliers' taps patched from the global lattice (tile_body, MIX).  Not where
    // the patching body spills: 8-bit 4:4:4 (12-22 VGPRs, at one pixel per tap batch too) and 16-bit trilinear in 4:2:0 and 4:4:4
    // (4 and 2) keep the second pass, the gather body under a divergent branch for the outlier lanes.
    constexpr bool kPatch = kMixed && !(!WIN && !CSX) && !(INTERP == LUTR_INTERP_TRILINEAR && WIN && WOUT && CSX == CSY);
    LutConsts L = L_;
    YuvConsts K = K_;
    // a wave-uniform constant used by several VALU ops per pixel is worth a VGPR (an SGPR operand halves the issue rate
    // of plain fp32 ops on gfx950, tools/ubench); the trilinear bodies have no registers to spare
    if constexpr (INTERP != LUTR_INTERP_TRILINEAR) {
        K.cyr = in_vgpr(K_.cyr); K.cyg = in_vgpr(K_.cyg); K.cyb = in_vgpr(K_.cyb);
        K.ky = in_vgpr(K_.ky); K.yb = in_vgpr(K_.yb); K.yob = in_vgpr(K_.yob);
        if constexpr (!N::fast) L.maxf = in_vgpr(L_.maxf);
    }
    if (lds_base() != 0) __builtin_trap();        // crd_table8 addresses the table absolutely
#ifdef __HIP_DEVICE_COMPILE__
    {   // pos_at reads the plane descriptors from the kernel-argument segment at the offset a struct of the parameters gives them:
        // make sure that IS where they are before any address is built from them
        struct KernArgsChk { LutConsts L; YuvConsts K; Planes2 P; FrameGeom G; Geom TG; };
        const __attribute__((address_space(4))) Planes2 *chk = (const __attribute__((address_space(4))) Planes2 *)(
            (const __attribute__((address_space(4))) char *)__builtin_amdgcn_kernarg_segment_ptr() + offsetof(KernArgsChk, P));
        if (chk->s[0] != P.s[0] || chk->d[2] != P.d[2] || chk->ss[1] != P.ss[1] || chk->dfs[2] != P.dfs[2]) __builtin_trap();
    }
#endif
    // the per-pixel constants of the table variants, times 8 (crd_table8); map_box keeps the plain ones
    YuvConsts KB = K;
    if constexpr (V >= V_TAB) {
        KB.ky = K.ky * 8.0f; KB.yb = K.yb * 8.0f;
        KB.krv = K.krv * 8.0f; KB.kgu = K.kgu * 8.0f; KB.kgv = K.kgv * 8.0f; KB.kbu = K.kbu * 8.0f;
    }
    const int tube_nb = 2 * TG.tube_h + 3;                    // nodes across each difference axis: cells -H..H, corners -H-1..H+1
    const int tube_nodes = TG.tube_h > 0 ? L.n1 * TG.tube_plane : 0;
    const int lane = threadIdx.x & 63;
    const int wib = uni(threadIdx.x >> 6);
    const int tab_bytes = TG.tab_entries * 8;
    const int scratch_off = tab_bytes + wib * 64;             // the window's cell ranges (second-level test)
    const int tube_off = tab_bytes + kScratch;
    const int slice_off = tube_off + tube_nodes * N::lds + wib * TG.win_nodes * N::lds;
    Win Wt;                                                   // the tube as a window: same address form as a staged one
    // index = pr * plane + (pg - pr + H + 1) * nb + (pb - pg + H + 1)
    Wt.o_g = N::lds * (tube_nb - 1); Wt.o_r = N::lds * (TG.tube_plane - tube_nb);
    Wt.fr = (float)Wt.o_r; Wt.fg = (float)Wt.o_g; Wt.fb = (float)N::lds;
    Wt.fc = as_tiny(lds_base() + tube_off + N::lds * ((TG.tube_h + 1) * tube_nb + TG.tube_h + 1));
    unsigned st_tube = 0, st_mixed = 0;
    int fr, sx, ry, rem;                                      // the tile being fetched next
    bool first = true;
    const int wgq_off = tab_bytes + kWaveScratch;             // the workgroup's chunk allocator (claim_chunk)
    if (threadIdx.x < 24) ((unsigned *)(smem + wgq_off))[threadIdx.x + (threadIdx.x ? 7 : 0)] = 0u;      // queue words 0, 8..30 (lutr_tube.h)
    const bool have_work = claim_chunk<LUTR_T2_WPB>(TG, lane, lds_base(), wgq_off, fr, sx, ry, rem, first);      // (no atomic: a wave's first chunk is its id)
    const int lw = 1 << TG.lw_log2, lh_log2 = 6 - TG.lw_log2;
    const int lx = lane & (lw - 1), ly = lane >> TG.lw_log2;
    const int cr0 = G.row0 >> CSY;                            // first unit row of this call's row range

    Win W;
    W.fr = W.fg = W.fb = W.fc = 0.0f; W.o_r = W.o_g = 0;
    if (lane == 0) {     // empty box: lo > hi in every plane, so the first tile always restages
        Box bx;
        bx.ylo = bx.cblo = bx.crlo = 0xffffffffu; bx.yhi = bx.cbhi = bx.crhi = 0u;
        box_store(scratch_off, bx);
    }
    if (TG.whole) {
        // lattice layout of the global copy ((N+1)^3 nodes, blue fastest, index N replicates N-1): prev + 1 is always staged
        W.o_r = N::lds * TG.whole_a; W.o_g = N::lds * TG.whole_b;
        W.fr = (float)W.o_r; W.fg = (float)W.o_g; W.fb = (float)N::lds;
        W.fc = as_tiny(lds_base() + tab_bytes + kScratch);
    }
    constexpr int YIB = T::YWI * 4, YOB = T::YWO * 4, CIB = T::CWI * 4, COB = T::CWO * 4;

    // Where a tile lives: wave-uniform strip pointers (frame, strip and unit row folded in) plus the clamps for lanes past
    // the right / bottom edge.  Built from scratch when a chunk is claimed; inside a chunk the next tile is one step down,
    // i.e. six 64-bit scalar adds -- recomputing the 64-bit products per tile cost ~140 scalar instructions per tile and wave.
    struct TilePos { const uint8_t *s0, *s1, *s2; uint8_t *d0, *d1, *d2; int xlim, ylim; };
    const unsigned ystep_s0 = (unsigned)((T::BH << lh_log2) * (int)P.ss[0]), ystep_s1 = (unsigned)((int)P.ss[1] << lh_log2),
                   ystep_s2 = (unsigned)((int)P.ss[2] << lh_log2);
    const unsigned ystep_d0 = (unsigned)((T::BH << lh_log2) * (int)P.ds[0]), ystep_d1 = (unsigned)((int)P.ds[1] << lh_log2),
                   ystep_d2 = (unsigned)((int)P.ds[2] << lh_log2);
    // The plane bases and frame strides (24 SGPRs) are only needed here, once per chunk: read them from the kernel-argument
    // segment when they are, instead of keeping them resident (and spilled to VGPR lanes) through every tile
    // (SGPR spills of the headline kernel 101 -> 82, profiles/r03_exp39_strides_from_kernarg.txt; the layout assumption is checked at
    // kernel start).
    auto pos_at = [&](int f, int tsx, int try_) {
        TilePos q;
#ifdef __HIP_DEVICE_COMPILE__
        struct KernArgs { LutConsts L; YuvConsts K; Planes2 P; FrameGeom G; Geom TG; };   // the kernel's parameter list
        typedef const __attribute__((address_space(4))) Planes2 *PlanesK;
        PlanesK Pk = (PlanesK)((const __attribute__((address_space(4))) char *)__builtin_amdgcn_kernarg_segment_ptr() + offsetof(KernArgs, P));
        asm volatile("" : "+s"(Pk));                                      // opaque: the loads stay here, not hoisted out of the loop
        const Planes2 P = *Pk;
#endif
        const long long urow0 = cr0 + (try_ << lh_log2);                  // wave-uniform
        q.s0 = P.s[0] + f * P.sfs[0] + urow0 * T::BH * (long long)P.ss[0] + (long long)tsx * lw * YIB;
        q.s1 = P.s[1] + f * P.sfs[1] + urow0 * (long long)P.ss[1] + (long long)tsx * lw * CIB;
        q.s2 = P.s[2] + f * P.sfs[2] + urow0 * (long long)P.ss[2] + (long long)tsx * lw * CIB;
        q.d0 = P.d[0] + f * P.dfs[0] + urow0 * T::BH * (long long)P.ds[0] + (long long)tsx * lw * YOB;
        q.d1 = P.d[1] + f * P.dfs[1] + urow0 * (long long)P.ds[1] + (long long)tsx * lw * COB;
        q.d2 = P.d[2] + f * P.dfs[2] + urow0 * (long long)P.ds[2] + (long long)tsx * lw * COB;
        q.xlim = TG.uw - 1 - tsx * lw;
        q.ylim = TG.urows - 1 - (try_ << lh_log2);
        return q;
    };
    auto pos_down = [&](TilePos &q) {
        q.s0 += ystep_s0; q.s1 += ystep_s1; q.s2 += ystep_s2;
        q.d0 += ystep_d0; q.d1 += ystep_d1; q.d2 += ystep_d2;
        q.ylim -= 1 << lh_log2;
    };
    // Input words of a tile.  Idle lanes of edge tiles re-read a valid unit of the same tile.  32-bit lane offsets: the
    // launcher only sends strides below 2^24 (a tile spans at most 128 rows).
    auto load_tile = [&](TileIn<WIN, WOUT, CSX, CSY> &dst, const TilePos &q) {
        const unsigned lxc = (unsigned)min(lx, q.xlim), lyc = (unsigned)min(ly, q.ylim);
        const unsigned y0 = __umul24(lyc * T::BH, P.ss[0]) + lxc * YIB;
#pragma unroll
        for (int dy = 0; dy < T::BH; dy++) ldw<T::YWI>(dst.y[dy], q.s0 + (y0 + dy * P.ss[0]));
        ldw<T::CWI>(dst.cb, q.s1 + (__umul24(lyc, P.ss[1]) + lxc * CIB));
        ldw<T::CWI>(dst.cr, q.s2 + (__umul24(lyc, P.ss[2]) + lxc * CIB));
    };

    bool have_win = false;
    int l2run = 0;                 // consecutive tiles vouched for by the second-level test only
    // event counters (lutr_ctx_tile_stats): kept in the wave's LDS scratch, not in registers (see Box)
    const bool counting = TG.stats != nullptr;
    unsigned *cnt = (unsigned *)(smem + scratch_off + 24);      // [0] second-level tests, [1] restage attempts; +56: [8] gather, [9] staged
    if (lane == 0) { cnt[0] = cnt[1] = 0; cnt[8] = cnt[9] = 0; }
    unsigned st_tiles = 0;
#define T2_COUNT(i) do { if (counting && lane == 0) cnt[i] += 1u; } while (0)
#ifdef LUTR_T2_DEBUG_STATS
    unsigned tk_head = 0, tk_l2 = 0, tk_rest = 0, tk_body = 0, tk_gath = 0, tk_store = 0, tk_wait = 0;
    unsigned long long tk = __builtin_amdgcn_s_memrealtime();
#define TK(acc) { const unsigned long long now_ = __builtin_amdgcn_s_memrealtime(); acc += (unsigned)(now_ - tk); tk = now_; }
#else
#define TK(acc)
#endif
    // The first tile's loads go out BEFORE the workgroup stages its table and tube: a launch of a few frames would otherwise
    // spend its first ~10 us with an idle memory system.
    TilePos np = pos_at(have_work ? fr : 0, have_work ? sx : 0, have_work ? ry : 0);          // the tile being fetched
    TileIn<WIN, WOUT, CSX, CSY> nxt;
    if (have_work) load_tile(nxt, np);
    if constexpr (V >= V_TAB) coord_table_fill<INTERP>(L, TG.tab_entries);     // the kernel's only barrier ...
    if (TG.whole) {                                                             // ... but for this one, in whole-lattice mode
        char *dst = smem + TG.tab_entries * 8 + kScratch;
        const int nodes = L.n1 * L.n1 * L.n1, plane = L.n1 * L.n1;
        for (int i = threadIdx.x; i < nodes; i += 64 * LUTR_T2_WPB) {
            const int r = i / plane, rem = i - r * plane, g = rem / L.n1, b = rem - g * L.n1;
            const int o = r * TG.whole_a + g * TG.whole_b + b;                  // (padded strides: see whole_strides)
            if constexpr (N::rec) {
                const u3 rc = make_rec(L.lat16[i], L.lat16[i + plane < nodes ? i + plane : i]);
                uint32_t *q = (uint32_t *)(dst + 12 * o); q[0] = rc.x; q[1] = rc.y; q[2] = rc.z;
            } else if constexpr (N::fast) ((uint2 *)dst)[o] = L.lat16[i];
            else {
                const float4 v = L.lat[i];
                if constexpr (N::lds == 16) ((float4 *)dst)[o] = v;
                else { float *q = (float *)(dst + 12 * o); q[0] = v.x; q[1] = v.y; q[2] = v.z; }
            }
        }
        __syncthreads();
    }
    if (TG.tube_h > 0) {
        // node (ir, ig, ib) = lattice (r, g = r + ig - H - 1, b = g + ib - H - 1), clamped
        // (a clamped node is never read by a valid pixel)
        char *dst = smem + TG.tab_entries * 8 + kScratch;
        const int plane = TG.tube_plane, nmax = L.n1 - 1;
        // four nodes per thread in flight: the staging is a chain of L2 round trips, and a short launch pays it in full
        constexpr int kSB = 4;
        for (int base = threadIdx.x; base < tube_nodes; base += kSB * 64 * LUTR_T2_WPB) {
            int src[kSB], src1[kSB];
#pragma unroll
            for (int k = 0; k < kSB; k++) {
                const int i = min(base + k * 64 * LUTR_T2_WPB, tube_nodes - 1);
                const int ir = i / plane, rem = i - ir * plane, ig = min(rem / tube_nb, tube_nb - 1), ib = rem - ig * tube_nb;   // (padding: any node)
                const int gq = ir + ig - TG.tube_h - 1;
                const int g = min(max(gq, 0), nmax), b = min(max(gq + ib - TG.tube_h - 1, 0), nmax);
                src[k] = (ir * L.n1 + g) * L.n1 + b;
                src1[k] = (min(ir + 1, nmax) * L.n1 + g) * L.n1 + b;
            }
            typename std::conditional<N::fast, uint2, float4>::type val[kSB];
            uint2 val1[N::rec ? kSB : 1];
#pragma unroll
            for (int k = 0; k < kSB; k++) {
                if constexpr (N::fast) val[k] = L.lat16[src[k]];
                else val[k] = L.lat[src[k]];
                if constexpr (N::rec) val1[k] = L.lat16[src1[k]];
            }
#pragma unroll
            for (int k = 0; k < kSB; k++) {
                const int i = min(base + k * 64 * LUTR_T2_WPB, tube_nodes - 1);      // (the last batch re-writes the final node: harmless)
                if constexpr (N::rec) { const u3 rc = make_rec(val[k], val1[k]); uint32_t *q = (uint32_t *)(dst + 12 * i); q[0] = rc.x; q[1] = rc.y; q[2] = rc.z; }
                else if constexpr (N::fast) ((uint2 *)dst)[i] = val[k];
                else if constexpr (N::lds == 16) ((float4 *)dst)[i] = val[k];
                else { float *q = (float *)(dst + 12 * i); q[0] = val[k].x; q[1] = val[k].y; q[2] = val[k].z; }
            }
        }
        __syncthreads();
    }
    __syncthreads();                          // (the allocator's LDS words are initialised; the general variant has no other barrier)
    if (!have_work) { queue_leave<LUTR_T2_WPB>(TG, lane, lds_base(), wgq_off); return; }      // (after the barriers above: every wave of the workgroup takes part in the staging)

    for (bool more = true; more;) {
        TileIn<WIN, WOUT, CSX, CSY> in = nxt;
        const TilePos cp = np;                // the tile being computed (its store pointers and clamps)
        // Next tile: the one below in this chunk, else the first tile of a newly claimed chunk.  Its loads are issued
        // NOW, before this tile's stores (vmcnt retires in order).  When the queue is drained the current tile is simply
        // fetched again, so every path has the same number of memory operations in flight.
        if (--rem > 0) { ry++; pos_down(np); }
        else {
            more = claim_chunk<LUTR_T2_WPB>(TG, lane, lds_base(), wgq_off, fr, sx, ry, rem, first);
            if (more) np = pos_at(fr, sx, ry);
        }
        load_tile(nxt, np);
        // s_setprio around the phases of a tile: a wave between its body and the next one -- stores, chunk claim, the next tile's
        // loads -- goes first, so memory operations leave as early as they can (strict 587-589 -> 593 Gpx/s, fast +0.1 %; the body
        // first instead: -1.7 %; profiles/r03_exp22_setprio.txt)
        __builtin_amdgcn_s_setprio(0);

#ifdef LUTR_T2_DEBUG_STATS
        TK(tk_store)                 // issuing the next tile's loads counts as store/loop time
        fence_words<T::YWI * T::BH>(&in.y[0][0]); fence_words<T::CWI>(in.cb); fence_words<T::CWI>(in.cr);
        TK(tk_wait)                  // ... and this is the wait for this tile's own loads
#endif
        Ext e = extremes<WIN, WOUT, CSX, CSY>(in);             // without the luma extremes: see below
        bool use_tube = false, mixed = false, lane_in = true;
        unsigned outside = 0u;                 // chroma samples of the lane's unit outside the tube (tile_body, MIX)
        if (TG.tube_h > 0) {
            // level 0: the tile's chroma keeps it inside the workgroup's grey tube (and its raw codes are legal for the clamp-free body)
            const uint32_t top = pack_hi<WIN>(TG.max_raw);
            // one vote for the common case: chroma inside the raw interval (which lies inside the legal codes) and luma legal
            const uint32_t ybits = luma_illegal<WIN>(e.yor, top);
            const uint32_t rbits = pk_subsat_sv(TG.tube_rlo, e.cbmin) | pk_subsat_vs(e.cbmax, TG.tube_rhi) |
                                   pk_subsat_sv(TG.tube_rlo, e.crmin) | pk_subsat_vs(e.crmax, TG.tube_rhi);
            if (__all((ybits | rbits) == 0u)) use_tube = true;
            else if (__all((ybits | pk_subsat_vs(e.cbmax, top) | pk_subsat_vs(e.crmax, top)) == 0u)) {
                // legal, but outside the interval: the bound itself.  Per sample for the strict kernels (their tube is 6 cells wide:
                // sigma = 16 frames +9 %, natural -0.8 %, 3 x chroma -1.5 %); the fast kernels' 8-cell tube gains 1.7 % there and loses
                // 1.4 % on 3 x chroma: corner form
                if constexpr (T::NC <= 4 && V != V_FAST) {
                    outside = tube_outside_samples<WIN, WOUT, CSX, CSY, PRE>(K, TG, in);
                    lane_in = outside == 0u;
                } else {
                    lane_in = tube_holds<WIN, PRE>(K, TG, e);
                    outside = lane_in ? 0u : ~0u;
                }
                use_tube = __all(lane_in);
                // MIXED tile: a few lanes outside the tube (sensor noise: one outlier unit in 64 sends a whole tile away).  Every
                // lane runs the tube body -- an outlier reads wherever its numbers point, LDS reads cannot fault -- and where a
                // sample is outside, the lane fetches those pixels' taps from the global lattice inside the same body: coordinates,
                // weights, blend, RGB -> YUV and packing run once.  (Raw codes are legal here -- the vote above -- so the body's
                // clamp-free table reads hold for the outliers too.)
                // (strict kernels only: with a cheap restage -- win_plane_stride -- the fast kernels' H = 8 tube and 367-node windows do as
                // well or better without it: three times the chroma 540 vs 518 Gpx/s, sigma-16 526 vs 539, profiles/r03_exp16_*.txt)
                if constexpr (kMixed)
                    if (!use_tube) mixed = __popcll(__ballot(!lane_in)) <= TG.mix_max;
            }
        }
        bool use_lds = use_tube || mixed;
        if (!use_lds && !TG.whole) {
            e.ymin = luma_min<WIN, WOUT, CSX, CSY>(in);
            e.ymax = luma_max<WIN, WOUT, CSX, CSY>(in);
            use_lds = box_holds(scratch_off, e);               // first level: raw extremes against the window's raw box
        }
        TK(tk_head)
        st_tiles++;
        if (TG.whole) {
            // every cell is in LDS; only raw codes above 2^din - 1 (which the padded table does not cover) need the clamping body
            const uint32_t top = pack_hi<WIN>(TG.max_raw);
            use_lds = __all((luma_illegal<WIN>(e.yor, top) | pk_subsat_vs(e.cbmax, top) | pk_subsat_vs(e.crmax, top)) == 0u);
        } else if (use_tube) {
            st_tube++;
        } else if (mixed) {
            st_mixed++;
        } else if (use_lds) {
#ifdef LUTR_T2_DEBUG_STATS
            if (l2run > 0 && lane == 0) atomicAdd(&TG.stats[21 + (l2run <= 1 ? 0 : l2run <= 2 ? 1 : l2run <= 4 ? 2 : l2run <= 8 ? 3 : l2run <= 16 ? 4 : 5)], (unsigned)l2run);
#endif
            l2run = 0;
        } else {
            T2_COUNT(0);
#ifdef LUTR_T2_DEBUG_STATS
            {   // which bound of the raw box failed (wave-wide), and was there a box at all
                const uint4 p = *(const uint4 *)(smem + scratch_off + 32);
                const uint2 q = *(const uint2 *)(smem + scratch_off + 48);
                const bool f0 = !__all(pk_subsat(p.x, e.ymin) == 0u), f1 = !__all(pk_subsat(e.ymax, p.y) == 0u);
                const bool f2 = !__all(pk_subsat(p.z, e.cbmin) == 0u), f3 = !__all(pk_subsat(e.cbmax, p.w) == 0u);
                const bool f4 = !__all(pk_subsat(q.x, e.crmin) == 0u), f5 = !__all(pk_subsat(e.crmax, q.y) == 0u);
                if (lane == 0) {
                    if (p.x > p.y) atomicAdd(&TG.stats[18], 1u);          // empty box
                    else {
                        if (f0) atomicAdd(&TG.stats[12], 1u); if (f1) atomicAdd(&TG.stats[13], 1u);
                        if (f2) atomicAdd(&TG.stats[14], 1u); if (f3) atomicAdd(&TG.stats[15], 1u);
                        if (f4) atomicAdd(&TG.stats[16], 1u); if (f5) atomicAdd(&TG.stats[17], 1u);
                        if ((f0 || f1) && !(f2 || f3 || f4 || f5)) atomicAdd(&TG.stats[19], 1u);   // luma only
                        if (!(f0 || f1) && (f2 || f3 || f4 || f5)) atomicAdd(&TG.stats[20], 1u);   // chroma only
                    }
                }
            }
#endif

            // second level: exact cells against the window's cell ranges.  Raw codes must be legal (<= 2^din - 1) for the
            // clamp-free table reads of tile_bounds and of the LDS body; a tile with wild container values takes the gather body.
            const uint32_t top = pack_hi<WIN>(TG.max_raw);
            const bool legal = __all((luma_illegal<WIN>(e.yor, top) | pk_subsat_vs(e.cbmax, top) | pk_subsat_vs(e.crmax, top)) == 0u);
            Bnd bn;
            bn.rmin = bn.gmin = bn.bmin = kBndNone; bn.rmax = bn.gmax = bn.bmax = -kBndNone;
            if (legal) bn = tile_bounds<WIN, WOUT, CSX, CSY, INTERP, PRE, V>(L, KB, TG, in);
            use_lds = have_win && legal && cells_hold(scratch_off, bn);
            TK(tk_l2)
            if (use_lds) {
                l2run++;
                // back-off: the 1st, 4th, 16th consecutive pass tries to give the window a raw box again.  (Staging a boxed window
                // instead when that fails was measured: such streaks sit on vertical colour edges, where no box fits: -0.7 %.)
                if (l2run == 1 || l2run == 4 || l2run == 16) rebox<WIN, INTERP, PRE, V>(L, K, TG, e, scratch_off, lane);
            } else {
#ifdef LUTR_T2_DEBUG_STATS
                if (l2run > 0 && lane == 0) atomicAdd(&TG.stats[21 + (l2run <= 1 ? 0 : l2run <= 2 ? 1 : l2run <= 4 ? 2 : l2run <= 8 ? 3 : l2run <= 16 ? 4 : 5)], (unsigned)l2run);
#endif
                l2run = 0;
            }
            if (!use_lds) {
                T2_COUNT(1);
                use_lds = restage<WIN, INTERP, PRE, V>(W, L, K, TG, e, bn, slice_off, scratch_off, lane);
                if (use_lds) { T2_COUNT(9); have_win = true; }
                TK(tk_rest)
            }
        }
        TileOut<WIN, WOUT, CSX, CSY> out;
        if (use_lds && !(kPatch && mixed)) {
            tile_body<true, WIN, WOUT, CSX, CSY, INTERP, PRE, V>(L, KB, (use_tube || mixed) ? Wt : W, TG, in, out); TK(tk_body)
        }
        bool gather = !use_lds;                      // whole tiles only (wave-uniform)
        if constexpr (kMixed && !kPatch) gather = gather || (mixed && !lane_in);
        if (gather) {
            tile_body<false, WIN, WOUT, CSX, CSY, INTERP, PRE, V>(L, KB, W, TG, in, out); TK(tk_gath)
        }
        if (kPatch && mixed) {
            tile_body<true, WIN, WOUT, CSX, CSY, INTERP, PRE, V, kPatch>(L, KB, Wt, TG, in, out, outside); TK(tk_body)
        }
        if (!use_lds) T2_COUNT(8);
        __builtin_amdgcn_s_setprio(3);      // stores, the queue and the next tile's loads go first
        {
            // Idle lanes of edge tiles processed a duplicate of a valid unit of this tile (load_tile clamps), so they
            // store the same bytes to the same place as its owner: no branch, fixed store count.
            const unsigned lxc = (unsigned)min(lx, cp.xlim), lyc = (unsigned)min(ly, cp.ylim);
            const unsigned y0 = __umul24(lyc * T::BH, P.ds[0]) + lxc * YOB;
#pragma unroll
            for (int dy = 0; dy < T::BH; dy++) stw<T::YWO>(cp.d0 + (y0 + dy * P.ds[0]), out.y[dy]);
            stw<T::CWO>(cp.d1 + (__umul24(lyc, P.ds[1]) + lxc * COB), out.cb);
            stw<T::CWO>(cp.d2 + (__umul24(lyc, P.ds[2]) + lxc * COB), out.cr);
        }
        TK(tk_store)
    }
#ifdef LUTR_T2_DEBUG_STATS
    if (TG.stats && lane == 0) {
        atomicAdd(&TG.stats[4], tk_head >> 4); atomicAdd(&TG.stats[5], tk_l2 >> 4); atomicAdd(&TG.stats[7], tk_rest >> 4);
        atomicAdd(&TG.stats[11], tk_wait >> 4); atomicAdd(&TG.stats[8], tk_body >> 4); atomicAdd(&TG.stats[9], tk_gath >> 4); atomicAdd(&TG.stats[10], tk_store >> 4);
    }
#endif
    queue_leave<LUTR_T2_WPB>(TG, lane, lds_base(), wgq_off);
    if (TG.stats && lane == 0) {
        atomicAdd(&TG.stats[0], st_tiles); atomicAdd(&TG.stats[1], cnt[1]);
        atomicAdd(&TG.stats[2], cnt[8]); atomicAdd(&TG.stats[3], cnt[9]); atomicAdd(&TG.stats[6], cnt[0]);
        atomicAdd(&TG.stats[12], st_tube); atomicAdd(&TG.stats[30], st_mixed);
    }
}

}  // namespace t2

// ================================================================= launcher
namespace {

// Largest index (unsigned)(yy + {rv, gv, bu}) can take for raw codes in [0, 2^din - 1]: each sum is monotone in its inputs.
int table_entries(const YuvConsts &K, int din)
{
    const float mr = (float)((1 << din) - 1);
    auto pre = [&](float v, float a, float b) { return K.pre != 0.0f ? fminf(fmaxf(floorf(fmaf(a, v, b)), 0.0f), K.pre_max) : v; };
    const float y1 = pre(mr, K.py, K.pyb), c0 = pre(0.0f, K.pc, K.pcb), c1 = pre(mr, K.pc, K.pcb);
    const float yy = fmaf(K.ky, y1, K.yb);
    const float r = yy + K.krv * (c1 - K.coff), g = yy + fmaf(K.kgu, c0 - K.coff, K.kgv * (c0 - K.coff)), b = yy + K.kbu * (c1 - K.coff);
    const float top = fmaxf(fmaxf(r, g), fmaxf(b, K.max_l));
    return ((int)top + 3) & ~1;           // even: the window slices behind the table stay 16-byte aligned (ds_read_b128)
}

bool out_clip_dead(const YuvConsts &K, int chroma_n)
{
    const float m = K.max_l, mn = K.max_l * (float)chroma_n;
    auto hi = [](float c, float v) { return c > 0.0f ? v : 0.0f; };
    const float y = fmaf(K.cyr, hi(K.cyr, m), fmaf(K.cyg, hi(K.cyg, m), fmaf(K.cyb, hi(K.cyb, m), K.yob)));
    const float cb = fmaf(K.cbr, hi(K.cbr, mn), fmaf(K.cbg, hi(K.cbg, mn), fmaf(K.cbb, hi(K.cbb, mn), K.cob)));
    const float cr = fmaf(K.crr, hi(K.crr, mn), fmaf(K.crg, hi(K.crg, mn), fmaf(K.crb, hi(K.crb, mn), K.cob)));
    const float lim = K.max_o + 1.0f;
    return y < lim && cb < lim && cr < lim;
}

}  // namespace

// The LUTR_* tuning knobs of this launcher (tools/ only) are read ONCE per process: round 2 called getenv a dozen times per
// launch, which a stream of single-frame applies pays every time (bench.py host_us_per_apply).
namespace {
struct Knob {
    const char *v;
    explicit Knob(const char *name) : v(getenv(name)) {}
    explicit operator bool() const { return v != nullptr; }
    int num() const { return atoi(v); }
};
#define T2_KNOB(NAME) ([]() -> const Knob & { static const Knob k(NAME); return k; }())
}  // namespace

// The tube's chroma bound under a shared prelut (LutConsts::pre_shared).  FFmpeg resamples a cineSpace shaper WITHOUT normalising the
// interpolation weight by the segment width (parse_cinespace: `mix = x - in_prelut[idx]`), so the curve lut3d applies is a staircase:
// nearly flat inside a segment, a jump at every input point -- its largest step between two codes says nothing about the rise over
// 100.  What the tube needs is D(d) = max over x of s(x + d) - s(x), the most the coordinate can rise over d codes: two channel codes at
// most d apart then sit at most floor(D(d)) + 1 cells apart.  Returns the largest d with D(d) <= h - 0.002 (0 if none).
// The scan is O(2^depth * d), so the last result is kept, keyed by the table's number (LutConsts::pre_gen) -- not by its address,
// which a context's next shaper at the same depth, or another context's table, may well reuse.
static int prelut_tube_bound(const float *s, unsigned long long gen, int maxi, int h)
{
    struct Memo { unsigned long long gen; int maxi, h, d; };
    static thread_local Memo memo = {0, 0, 0, 0};
    if (!s || maxi < 1) return 0;
    if (gen && memo.gen == gen && memo.maxi == maxi && memo.h == h) return memo.d;
    const float lim = (float)h - 2e-3f;
    int d = 0;
    for (int cand = 1; cand <= maxi; cand++) {
        float rise = 0.0f;
        for (int x = 0; x + cand <= maxi; x++) rise = fmaxf(rise, s[x + cand] - s[x]);
        if (rise > lim) break;
        d = cand;
    }
    memo = Memo{gen, maxi, h, d};
    return d;
}

// Which variant serves this call?
static int tile2_variant(const LutConsts &L, const YuvConsts &K, int lut_depth, int csx, int csy, bool fast)
{
    const bool eq = L.pre ? L.pre_shared != 0 : (L.sc[0] == L.sc[1] && L.sc[1] == L.sc[2]);      // one coordinate table for R, G and B
    const bool tab = eq && lut_depth <= 10 && (L.pre || !T2_KNOB("LUTR_NO_TAB"));
    const bool unit = L.unit && out_clip_dead(K, 1 << (csx + csy));
    if (fast && tab && unit && L.lat16 && !L.pre) return t2::V_FAST;      // (the fast variant is defined without a prelut: its CPU twin has none)
    if (tab && unit && L.latm && !L.pre) return t2::V_FMA32;              // (likewise; any LUT depth the table serves)
    if (tab && unit) return t2::V_UNIT;
    if (tab) return t2::V_TAB;
    return t2::V_GEN;
}

const char *T2_ENTRY(hipStream_t st, const LutConsts &L, const YuvConsts &K, const PlaneSet &P, const FrameGeom &G,
                             int din, int dout, int lut_depth, int csx, int csy, int mode, bool fast, unsigned *stats, unsigned *queue)
{
    using namespace t2;
    constexpr int win = LUTR_T2_WI, wout = LUTR_T2_WO;
    if ((din > 8) != win || (dout > 8) != wout || csx != LUTR_T2_X || csy != LUTR_T2_Y) return nullptr;
    const int pxt = win ? 8 : 16;
    const bool pre = K.pre != 0.0f;
    const int v = tile2_variant(L, K, lut_depth, csx, csy, fast);
    if (pre && v != V_UNIT && v != V_FAST && v != V_FMA32) return nullptr;
    if (L.pre && v < V_TAB) return nullptr;                   // a prelut lives in the coordinate table: the general variant computes
    // nearest has no blend to speed up and no prologue instances: strict clip-free kernel, or the round-1 path
    if (mode == LUTR_INTERP_NEAREST && pre) return nullptr;
    const int vv = (mode == LUTR_INTERP_NEAREST && (v == V_FAST || v == V_FMA32)) ? V_UNIT : v;      // (c * M rounds once either way)
    for (int i = 0; i < 3; i++)
        if (P.sfs[i] < 0 || P.dfs[i] < 0 || P.ss[i] < 0 || P.ds[i] < 0 || P.ss[i] >= (1 << 24) || P.ds[i] >= (1 << 24)) return nullptr;

    Geom tg;
    const int uw = G.w / pxt, urows = G.rows >> csy;
    // lanes across x: 16 (x 4 down: 128 x 8 px at 10-bit 4:2:0) unless another shape wastes 2 % fewer lanes at the frame's edges.
    // Compact tiles see fewer colours: with the tube, 16 x 4 measures 625 / 564 Gpx/s fast / strict against 607 / 542 for 32 x 2
    // and 615 / 562 for 8 x 8 (UHD).
    // 4:2:2 / 4:4:4 (one row per unit) are on the memory side and want 512-byte runs per tile row: 32 x 2 lanes there
    // (yuv422p10le 489 vs 341 Gpx/s, yuv444p10le 407 vs 332).
    int best = csy ? 4 : 5;
    double best_eff = -1.0;
    const int order[2][5] = {{5, 4, 6, 3, 2}, {4, 5, 3, 6, 2}};
    for (int l : order[csy ? 1 : 0]) {
        const int lw = 1 << l, lh = 64 >> l;
        const double eff = ((double)uw / (((uw + lw - 1) / lw) * lw)) * ((double)urows / (((urows + lh - 1) / lh) * lh));
        if (eff > best_eff + 0.02) { best_eff = eff; best = l; }
    }
    if (const Knob &e = T2_KNOB("LUTR_LW_LOG2")) { const int c = e.num(); if (c >= 2 && c <= 6) best = c; }
    tg.lw_log2 = best; tg.uw = uw; tg.urows = urows;
    tg.nsx = (uw + (1 << best) - 1) >> best;
    tg.nry = (urows + (64 >> best) - 1) / (64 >> best);
    int waves_per_cu = 16;
    if (const Knob &e = T2_KNOB("LUTR_WAVES_PER_CU")) { const int c = e.num(); if (c >= LUTR_T2_WPB && c <= 32 && c % LUTR_T2_WPB == 0) waves_per_cu = c; }
    const int max_waves = capped_waves(T2_KNOB("LUTR_MAX_WAVES").v, LUTR_T2_WPB, device_cus() * waves_per_cu);
    // Chunk = `ch` consecutive tile rows of a strip.  Round 2's single counter capped the claim rate (4096 waves got ~85 M atomic adds
    // per second out of it: UHD 10-bit throughput was proportional to the chunk height up to 7 tiles -- 348 / 434 / 515 / 585 Gpx/s at
    // 4 / 5 / 6 / 7 -- and flat from 8), so chunks were at least 8192 pixels.  With the two-level queue (claim_chunk: one global atomic
    // per 16 claims) small chunks are free -- 256 UHD frames at 8 / 4 / 2 tiles: 581 / 582 / 576 Gpx/s strict -- and they are what a
    // short launch needs for its tail: 8 frames 347 / 361 / 436, 16 frames 438 / 490 / 501, 32 frames 518 / 535 / 536
    // (profiles/r03_exp18_two_level_queue.txt).  4096 pixels per claim, 2048 when a wave gets fewer than 64 tiles.
    const int tile_px = pxt * (1 << csy) * 64;
    int ch = (4096 + tile_px - 1) / tile_px;
    if ((long long)G.nframes * tg.nsx * tg.nry < 64ll * max_waves) ch = (2048 + tile_px - 1) / tile_px;
    if (ch < 1) ch = 1;
    if (const Knob &e = T2_KNOB("LUTR_CHUNK")) { const int c = e.num(); if (c >= 1 && c <= 256) ch = c; }
    while (ch > 1 && (long long)G.nframes * tg.nsx * ((tg.nry + ch - 1) / ch) < max_waves / 4) ch >>= 1;
    tg.ch = ch; tg.nrc = (tg.nry + ch - 1) / ch; tg.nchunks = G.nframes * tg.nrc * tg.nsx;
    tg.tab_entries = vv >= V_TAB ? table_entries(K, din) : 0;
    tg.max_raw = (1 << din) - 1;
    if ((tg.max_raw & (tg.max_raw + 1)) != 0) return nullptr;      // the kernels test legality by OR (or_words): 2^k - 1 only
    const int node_ = vv == V_FAST ? (mode == LUTR_INTERP_TRILINEAR ? 12 : 8) : (mode == LUTR_INTERP_TRILINEAR ? 16 : 12);      // Node::lds
    const int blocks_per_cu = waves_per_cu / LUTR_T2_WPB > 0 ? waves_per_cu / LUTR_T2_WPB : 1;
    const int lds_block = 163840 / blocks_per_cu - tg.tab_entries * 8 - t2::kScratch;
    // whole-lattice mode: (N+1)^3 nodes behind the table in one workgroup's LDS, row and plane strides padded against bank conflicts.
    // The strict tetrahedral kernels stage float4 nodes there when those fit too (T2_TET16; N <= 19 at 10 bit).
    int node = node_;
    long long whole_bytes = 0;
    bool whole16 = false;
    tg.whole = 0; tg.whole_a = L.n1 * L.n1; tg.whole_b = L.n1;
    if (blocks_per_cu == 1 && !T2_KNOB("LUTR_NO_WHOLE")) {
        if (node_ == 12 && mode == LUTR_INTERP_TETRAHEDRAL && vv != V_GEN && !T2_KNOB("LUTR_NO_WHOLE16")) {
            int a, b;
            const long long bytes = whole_strides(L.n1, 16, lds_block, &a, &b);
            if (bytes) { tg.whole = 1; tg.whole_a = a; tg.whole_b = b; whole_bytes = bytes; whole16 = true; node = 16; }
        }
        if (!tg.whole) {
            int a, b;
            const long long bytes = whole_strides(L.n1, node_, lds_block, &a, &b);
            if (bytes) { tg.whole = 1; tg.whole_a = a; tg.whole_b = b; whole_bytes = bytes; }
        }
    }
    // The grey tube (Geom::tube_h): all of r, |g - r| and |b - r| up to H cells.  Needs the table variants (equal channel scales: the
    // chroma-only bound of map_box), a blend (nearest rounds to a node, the bound is for floor), and room left for windows.
    // H: as wide as 70 % of the block's LDS allows while every wave keeps a window of 256 nodes, at most 8 cells of a 33^3 lattice
    // (+-64 8-bit codes of G-R and B-R; 34 x 19 x 19 fp16 nodes = 98 KB, windows of 366 nodes).  Measured, UHD yuv420p10le fast,
    // H = 5 / 7 / 8 / 9: natural frames 611 / 620 / 628 / 636 Gpx/s, three times the chroma 516 / 521 / 530 / 519, sigma = 8 noise
    // 503 / 543 / 550 / 569, sigma = 16 250 / 388 / 481 / 500: the tube, not the windows, is what carries natural content; 9 leaves
    // windows of 197 nodes and starts to cost saturated frames.  The strict kernels (12-byte nodes) get H = 7 (below).
    tg.tube_h = 0; tg.tube_t = 0.0f; tg.tube_plane = 0;
    long long tube_bytes = 0;
    // (65^3: a tube that fits is 5 of ITS cells wide, +-20 8-bit codes -- 497 / 427 Gpx/s with it, 530 / 492 without: off above 40^3)
    if (!tg.whole && vv >= V_TAB && mode != LUTR_INTERP_NEAREST && (L.n1 <= 41 || T2_KNOB("LUTR_TUBE_H"))) {
        int h = (8 * (L.n1 - 2) + 16) / 32;                       // 8 at 33^3
        // a short launch (under ~100 tiles per wave) does not earn back the ~8 us it takes to stage the widest tube: 5 cells there
        // (UHD, 8 / 16 / 32 / 64 frames per launch, Gpx/s at H = 8 | 5: 351 | 369, 445 | 456, 533 | 541, 598 | 595)
        if ((long long)G.nframes * tg.nsx * tg.nry < 100ll * max_waves) h = (5 * (L.n1 - 2) + 16) / 32;
        if (const Knob &e = T2_KNOB("LUTR_TUBE_H")) h = e.num();
        const float kappa = L.pre ? fmaxf(L.pre_kappa, 1e-6f) : L.sc[0] * L.scale_f;   // cells per code, at most (a shared prelut: its largest step)
        const float eps = K.max_l * (1.0f / 2097152.0f) + 1e-3f;                 // as map_box
        const float slack = 1.0f + 2.0f * L.lut_max * (1.0f / 2097152.0f) + 2e-3f;
        // fast (8-byte nodes): at most 70 % of the block's LDS and windows of >= 256 nodes (H = 8 / 366 at 33^3).  The strict 4-tap
        // kernels' 12-byte nodes do not fit that at H = 7; they trade window size for tube width (H = 7, 16 windows of 134 nodes
        // instead of H = 6 / 277): natural +2 %, sigma-8 +0 %, sigma-16 +43 %, three times the chroma -7 % (profiles/r03_exp4.txt)
        int min_win = node == 12 ? 128 : 256, tube_pct = node == 12 ? 85 : 70;
        if (const Knob &e = T2_KNOB("LUTR_MIN_WIN")) { const int c = e.num(); if (c >= 128 && c <= 4096) min_win = c; }
        if (const Knob &e = T2_KNOB("LUTR_TUBE_PCT")) { const int c = e.num(); if (c >= 10 && c <= 95) tube_pct = c; }
        while (h >= 3) {
            const long long nb = 2 * h + 3, plane = T2_KNOB("LUTR_TUBE_NOPAD") ? nb * nb : tube_plane_stride((int)nb, node);
            const long long bytes = (long long)L.n1 * plane * node;
            const bool fits = bytes <= (long long)lds_block * tube_pct / 100 && (lds_block - bytes) / (node * LUTR_T2_WPB) >= min_win;
            float t = ((float)(h + 1) - slack) / kappa - 1.0f - eps;
            if (L.pre) t = fits ? prelut_tube_bound(L.pre_host, L.pre_gen, (int)L.maxf, h) - 0.5f - eps : 0.0f;      // (a scan of the curve: memoised)
            if (fits && t > 0.0f) {
                tg.tube_h = h; tg.tube_t = t; tg.tube_plane = (int)plane; tube_bytes = bytes;
                break;
            }
            h--;
        }
    }
    // 63: whenever at least one lane is inside the tube; a tile with all 64 lanes outside goes to the wave's window as before.
    // Measured for the strict kernels (64 UHD frames, Gpx/s, profiles/r03_exp16_mixed_tiles_cheap_restage.txt): sigma-16 frames
    // 409 without mixed tiles, 423 / 426 / 428 / 435 at 8 / 16 / 32 / 63 lanes; sigma-8 498 -> 510; natural and saturated frames +-1 %.
    // (profiles/r03_exp7_mixed_tiles.txt shows 286 -> 402: that build still paid 30 us of stride search per restage.)
    // With the outliers patched inside the tube body (tile_body, MIX) a mixed tile is cheaper still, and 63 wins everywhere, at
    // 8 / 16 / 32 / 63 lanes: natural 585 / 589 / 598 / 601, sigma-8 512 / 519 / 525 / 548, sigma-16 434 / 443 / 450 / 479, three times
    // the chroma 458 / 460 / 468 / 477 (profiles/mixed_patch_ab.txt).
    tg.mix_max = 63;
    if (const Knob &e = T2_KNOB("LUTR_MIX_MAX")) { const int c = e.num(); if (c >= 0 && c <= 63) tg.mix_max = c; }
    tg.tube_rlo = 0xffffffffu; tg.tube_rhi = 0u;
    if (tg.tube_h > 0) {
        // the square |cb' - coff|, |cr' - coff| <= R (after the prologue) inside the tube's chroma region: both differences are linear in
        // the two offsets, so their worst corners bound them; 1 % and one code of margin absorb the float rounding of the per-lane form
        const float s1 = fabsf(K.kgu) + fabsf(K.kgv - K.krv);
        const float s2 = fabsf(K.kbu - K.kgu) + fabsf(K.kgv);
        const float R = floorf(0.99f * tg.tube_t / fmaxf(s1, s2)) - 1.0f;
        // (one entry of memory: a stream of applies repeats the same constants, and the scan is up to 65,536 codes long)
        struct Memo { float pre, pc, pcb, pre_max, coff, R; int max_raw, lo, hi; };
        static thread_local Memo memo = {0, 0, 0, 0, 0, -1.0f, -1, -1, -1};
        int lo = -1, hi = -1;
        if (memo.pre == K.pre && memo.pc == K.pc && memo.pcb == K.pcb && memo.pre_max == K.pre_max && memo.coff == K.coff &&
            memo.R == R && memo.max_raw == tg.max_raw) { lo = memo.lo; hi = memo.hi; }
        else {
            for (int raw = 0; raw <= tg.max_raw; raw++) {           // the prologue is a monotone map of raw codes
                float c = (float)raw;
                if (K.pre != 0.0f) c = fminf(fmaxf(floorf(fmaf(K.pc, c, K.pcb)), 0.0f), K.pre_max);
                if (fabsf(c - K.coff) <= R) { if (lo < 0) lo = raw; hi = raw; }
            }
            memo = Memo{K.pre, K.pc, K.pcb, K.pre_max, K.coff, R, tg.max_raw, lo, hi};
        }
        if (R >= 1.0f && lo >= 0) {
            auto rep = [&](unsigned v16) { return v16 | (v16 << 16); };
            tg.tube_rlo = win ? rep((unsigned)lo) : rep((unsigned)lo << 8);
            tg.tube_rhi = win ? rep((unsigned)hi) : rep(((unsigned)hi << 8) | 0xffu);
        }
    }
    int cap = (int)((lds_block - tube_bytes) / (node * LUTR_T2_WPB));
    if (const Knob &e = T2_KNOB("LUTR_WIN_NODES")) { const int c = e.num(); if (c >= 64 && c < cap) cap = c; }
    if (!tg.whole && cap < 128) return nullptr;
    tg.win_nodes = tg.whole ? 0 : cap;
    tg.queue = queue; tg.stats = stats;
    const int waves = tg.nchunks < max_waves ? tg.nchunks : max_waves;
    const dim3 grid((waves + LUTR_T2_WPB - 1) / LUTR_T2_WPB), block(64 * LUTR_T2_WPB);
    tg.qbase = grid.x * LUTR_T2_WPB;      // (the counter is at zero: the previous launch left it so)
    const size_t lds = (size_t)tg.tab_entries * 8 + kScratch +
                       (tg.whole ? (size_t)whole_bytes : (size_t)tube_bytes + (size_t)LUTR_T2_WPB * tg.win_nodes * node);
    Planes2 TP;
    for (int i = 0; i < 3; i++) {
        TP.s[i] = P.s[i]; TP.d[i] = P.d[i];
        TP.ss[i] = (unsigned)P.ss[i]; TP.ds[i] = (unsigned)P.ds[i];
        TP.sfs[i] = (unsigned long long)P.sfs[i]; TP.dfs[i] = (unsigned long long)P.dfs[i];
    }
    LutConsts Lm = L;                         // the fma32 kernels read the pre-multiplied copy through the strict kernels' pointer
    Lm.lat = L.latm;
    if (T2_KNOB("LUTR_DEBUG"))
        fprintf(stderr, "[lutr t2] nsx %d nry %d chunk %d chunks %d blocks %u lds/block %zu win_nodes %d tab %d variant %d tube h %d plane %d t %.1f\n",
                tg.nsx, tg.nry, tg.ch, tg.nchunks, grid.x, lds, tg.win_nodes, tg.tab_entries, vv, tg.tube_h, tg.tube_plane, tg.tube_t);

#define T2_LAUNCH(WI, WO, X, Y, I, PR, VV, NAME) \
    do { \
        auto kern = k_yuv_tile2<WI, WO, X, Y, I, PR, VV>; \
        if (!allow_lds((const void *)kern, lds)) return nullptr; \
        hipLaunchKernelGGL(kern, grid, block, lds, st, VV == V_FMA32 ? Lm : L, K, TP, G, tg); \
        return tg.whole ? NAME "+whole-lattice" : (tg.tube_h ? NAME "+tube" : NAME); \
    } while (0)
#define T2_NAME(WI, WO, X, Y, I, SUF) "k_yuv_tile2<" #WI #WO "," #X #Y "," #I SUF ">"
#define T2_CASE(WI, WO, X, Y, I) \
    if (mode == I) { \
        if (I == LUTR_INTERP_TETRAHEDRAL && whole16) {      /* (other I: the template argument falls back to an instance that exists anyway) */ \
            if (pre && vv == V_FMA32) T2_LAUNCH(WI, WO, X, Y, (I == 2 ? T2_TET16 : 2), 1, V_FMA32, T2_NAME(WI, WO, X, Y, I, ",pre,tab,unit,fma32,n16")); \
            if (pre) T2_LAUNCH(WI, WO, X, Y, (I == 2 ? T2_TET16 : 2), 1, V_UNIT, T2_NAME(WI, WO, X, Y, I, ",pre,tab,unit,n16")); \
            if (vv == V_FMA32) T2_LAUNCH(WI, WO, X, Y, (I == 2 ? T2_TET16 : 2), 0, V_FMA32, T2_NAME(WI, WO, X, Y, I, ",tab,unit,fma32,n16")); \
            if (vv == V_UNIT) T2_LAUNCH(WI, WO, X, Y, (I == 2 ? T2_TET16 : 2), 0, V_UNIT, T2_NAME(WI, WO, X, Y, I, ",tab,unit,n16")); \
            if (vv == V_TAB) T2_LAUNCH(WI, WO, X, Y, (I == 2 ? T2_TET16 : 2), 0, V_TAB, T2_NAME(WI, WO, X, Y, I, ",tab,n16")); \
        } \
        if (I != LUTR_INTERP_NEAREST) { \
            if (pre && vv == V_FAST) T2_LAUNCH(WI, WO, X, Y, (I == 0 ? 2 : I), 1, V_FAST, T2_NAME(WI, WO, X, Y, I, ",pre,tab,unit,fast")); \
            if (pre && vv == V_FMA32) T2_LAUNCH(WI, WO, X, Y, (I == 0 ? 2 : I), 1, V_FMA32, T2_NAME(WI, WO, X, Y, I, ",pre,tab,unit,fma32")); \
            if (pre) T2_LAUNCH(WI, WO, X, Y, (I == 0 ? 2 : I), 1, V_UNIT, T2_NAME(WI, WO, X, Y, I, ",pre,tab,unit")); \
            if (vv == V_FAST) T2_LAUNCH(WI, WO, X, Y, (I == 0 ? 2 : I), 0, V_FAST, T2_NAME(WI, WO, X, Y, I, ",tab,unit,fast")); \
            if (vv == V_FMA32) T2_LAUNCH(WI, WO, X, Y, (I == 0 ? 2 : I), 0, V_FMA32, T2_NAME(WI, WO, X, Y, I, ",tab,unit,fma32")); \
        } \
        if (vv == V_UNIT) T2_LAUNCH(WI, WO, X, Y, I, 0, V_UNIT, T2_NAME(WI, WO, X, Y, I, ",tab,unit")); \
        if (vv == V_TAB) T2_LAUNCH(WI, WO, X, Y, I, 0, V_TAB, T2_NAME(WI, WO, X, Y, I, ",tab")); \
        T2_LAUNCH(WI, WO, X, Y, I, 0, V_GEN, T2_NAME(WI, WO, X, Y, I, "")); \
    }
    T2_CASE(LUTR_T2_WI, LUTR_T2_WO, LUTR_T2_X, LUTR_T2_Y, 0)
    T2_CASE(LUTR_T2_WI, LUTR_T2_WO, LUTR_T2_X, LUTR_T2_Y, 1)
    T2_CASE(LUTR_T2_WI, LUTR_T2_WO, LUTR_T2_X, LUTR_T2_Y, 2)
    return nullptr;
}

}  // namespace lutr
