// lutr_internal.h -- structures shared by the C-ABI layer (lutr_api.cpp) and the
// gfx950 kernels (lutr_kernels.hip).  Not part of the public boundary.  The launchers' shared host helpers: lutr_launch.h.
#pragma once

#ifdef LUTR_HOST_ONLY
// Sanitizer build of the two host parsers (oracle/Makefile `asan`: gcc -fsanitize=address,undefined, no HIP):
// they need the public header and set_error only.
#include <stdint.h>

#include "lutr.h"

namespace lutr {
void set_error(const char *fmt, ...);
}
#else

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "lutr.h"

namespace lutr {

// Device lattice: (n+1)^3 nodes of float4 {r,g,b,0}, index ((r*n1+g)*n1+b), blue
// fastest like FFmpeg's lut[r*N*N + g*N + b].  Index n on every axis
// is a replica of node n-1, so NEXT(x) = min(prev+1, n-1) (A.4) becomes prev+1 with
// no clamp in the kernels.
struct LutConsts {
    const float4 *lat;
    const uint2  *lat16;  // fast variant: the same nodes as fp16 {r, g, b, 0} of (value * (2^depth - 1)), or nullptr
    const float4 *latm;   // fma32 variant: the same nodes as fp32 {r, g, b, 0} of (value * (2^depth - 1)), or nullptr
    int   n1;            // n + 1
    float scale_f;       // 1.0f / (2^depth - 1)
    float sc[3];         // scale.{r,g,b} * (n-1)
    float lut_max;       // (float)(n-1)
    float maxf;          // (float)(2^depth - 1)
    int   unit;          // 1 when every lattice node is known to lie in [0, 1] (lets the tile kernels drop the output clip)
    const float *pre;    // lut3d's prelut folded into a per-code table of lattice coordinates (3 x pre_stride floats: the coordinate of
    int   pre_stride;    // integer code i of channel c is pre[c * pre_stride + i]), or nullptr.  The generic / vector kernels and the RGB
                         // tube kernels read it per channel; the fused YUV tile kernels take it when it is `pre_shared`:
    int   pre_shared;    // 1: the three channels' tables are identical and non-decreasing over the codes 0 .. 2^depth - 1 (the usual
    float pre_kappa;     // cineSpace shaper): one coordinate table serves R, G and B; pre_kappa = the largest step between two codes (cells)
    const float *pre_host; // HOST copy of that shared table (2^depth entries; launcher only: the tube's bound is read off the curve itself)
    unsigned long long pre_gen;  // a process-wide number of that table, new for every table built (launcher only: the key of the tube bound's memo)
};

// Constant block of the YUV contract; same fields, same order as the
// oracle's orc_yuv_consts so tests can compare them float for float.
struct YuvConsts {
    float ky, yb, coff, krv, kgu, kgv, kbu, max_l;
    float cyr, cyg, cyb, yob;
    float cbr, cbg, cbb;
    float crr, crg, crb, cob;
    float max_o;
    float pre;                       // 0 or 1
    float py, pyb, pc, pcb, pre_max;
    float pad[6];                    // -> 32 floats
};
static_assert(sizeof(YuvConsts) == 32 * sizeof(float), "YuvConsts is the 32-float block of lutr_yuv_constants");

struct PlaneSet {
    const uint8_t *s[3];
    uint8_t       *d[3];
    long long ss[3], ds[3];          // row strides, bytes
    long long sfs[3], dfs[3];        // frame strides, bytes
};

// the planes of a second destination (lutr_dual.hip)
struct DstPlanes {
    uint8_t  *d[3];
    long long ds[3], dfs[3];         // row / frame strides, bytes
};

// one interleaved image (or batch): component offsets in units of one component
struct PackedSet {
    const uint8_t *s;
    uint8_t       *d;
    long long ss, ds, sfs, dfs;      // row / frame strides, bytes
    int ro, go, bo, ao;              // ao = the fourth slot of 4-component formats (alpha or padding)
};

// unquantised output planes of the dither path (device scratch, densely packed per frame)
struct FloatPlanes {
    float *y, *cb, *cr;
};

struct FrameGeom {
    int w, h, row0, rows, nframes;
};

enum Variant { VAR_AUTO = 0, VAR_GENERIC = 1, VAR_VEC_GLOBAL = 2, VAR_VEC_LDS = 3 };

// launchers (lutr_kernels.hip); return the kernel's name, or nullptr when the variant
// cannot take this layout (caller then falls back to the generic kernel)
const char *launch_rgb(hipStream_t st, int variant, const LutConsts &L, const PlaneSet &P,
                       const FrameGeom &G, int depth, int interp, unsigned *stats, unsigned *queue);
const char *launch_yuv(hipStream_t st, int variant, const LutConsts &L, const YuvConsts &K,
                       const PlaneSet &P, const FrameGeom &G, int din, int dout, int lut_depth, int csx, int csy,
                       int interp, bool fast, unsigned *stats, unsigned *queue);

// packed RGB (lutr_packed.hip)
const char *launch_packed(hipStream_t st, int variant, const LutConsts &L, const PackedSet &P, const FrameGeom &G,
                          int wide, int ncomp, int interp, unsigned *stats, unsigned *queue);

// round-3 RGB tube kernels (lutr_rgb2.hip, one translation unit per layout): planes in SLOT order -- planar callers pass
// (R, G, B), packed callers the one buffer in [0] and rev = 1 for B, G, R memory order; nullptr = cannot take the call
#define LUTR_R2_DECL(ly) \
    const char *launch_rgb_tube_ly##ly(hipStream_t st, const LutConsts &L, const PlaneSet &P, const FrameGeom &G, int depth, \
                                       int mode, int rev, unsigned *stats, unsigned *queue);
LUTR_R2_DECL(0) LUTR_R2_DECL(1) LUTR_R2_DECL(2) LUTR_R2_DECL(3) LUTR_R2_DECL(4) LUTR_R2_DECL(5) LUTR_R2_DECL(6) LUTR_R2_DECL(7)
#undef LUTR_R2_DECL

// error-diffusion dither path (lutr_dither.hip): whole frames, float planes in F (chroma planes in the output layout ocsx, ocsy;
// csx, csy are the input's)
const char *launch_yuv_dither(hipStream_t st, const LutConsts &L, const YuvConsts &K, const PlaneSet &P,
                              const FrameGeom &G, const FloatPlanes &F, int din, int dout, int csx, int csy, int interp,
                              int ocsx, int ocsy);

// chroma subsampling change (lutr_xsub.hip): input layout icsx, icsy, output layout ocsx, ocsy (they differ); K
// carries the output block's 1/n.  nullptr = the variant cannot take the call (vec_lds always; vec_global on layouts the vector
// kernel cannot take)
const char *launch_yuv_xsub(hipStream_t st, int variant, const LutConsts &L, const YuvConsts &K, const PlaneSet &P,
                            const FrameGeom &G, int din, int dout, int icsx, int icsy, int ocsx, int ocsy, int interp);
// its vector kernels, one translation unit per container mix (w<in wide><out wide>): nullptr = not a cross pair / mode it has
#define LUTR_XS_DECL(tag) \
    const char *launch_yuv_xsub_vec_##tag(hipStream_t st, const LutConsts &L, const YuvConsts &K, const PlaneSet &P, \
                                          const FrameGeom &G, int icsx, int icsy, int ocsx, int ocsy, int interp);
LUTR_XS_DECL(w00) LUTR_XS_DECL(w11) LUTR_XS_DECL(w10)
#undef LUTR_XS_DECL
// the dither path's unquantised pass for a subsampling change (k_yuv_float_xsub)
void launch_yuv_float_xsub(hipStream_t st, const LutConsts &L, const YuvConsts &K, const PlaneSet &P, const FrameGeom &G,
                           const FloatPlanes &F, int win, int icsx, int icsy, int ocsx, int ocsy, int interp);

// two lut3d stages in one pass (lutr_chain.hip): launch_yuv_xsub's call for any pair of layouts, the equal ones
// included, with a second lattice L2 (no prelut) and its mode behind the first.  nullptr = the variant cannot take the call
// (vec_lds always; vec_global on layouts the vector kernel cannot take and on a pair of different modes)
const char *launch_yuv_chain(hipStream_t st, int variant, const LutConsts &L, const LutConsts &L2, const YuvConsts &K,
                             const PlaneSet &P, const FrameGeom &G, int din, int dout, int icsx, int icsy, int ocsx, int ocsy,
                             int interp, int interp2);
// its vector kernels, one translation unit per container mix (w<in wide><out wide>): nullptr = not a mode it has
#define LUTR_CH_DECL(tag) \
    const char *launch_yuv_chain_vec_##tag(hipStream_t st, const LutConsts &L, const LutConsts &L2, const YuvConsts &K, \
                                           const PlaneSet &P, const FrameGeom &G, int icsx, int icsy, int ocsx, int ocsy, \
                                           int interp);
LUTR_CH_DECL(w00) LUTR_CH_DECL(w11) LUTR_CH_DECL(w10)
#undef LUTR_CH_DECL

// ASC CDL in front of lut3d (lutr_cdl.hip): the per-code table of slope, offset, clamp and power (device; the
// value of integer code i of channel c is tab[c * stride + i], stride = 2^lut_depth) and the saturation
struct CdlConsts {
    const float *tab;
    int   stride;
    float sat;
};
// launch_yuv_xsub's call for any pair of layouts, the equal ones included, with the CDL between the YUV -> RGB stage and the
// lattice (L.pre is not read).  nullptr = the variant cannot take the call (vec_lds always; vec_global on layouts the vector
// kernel cannot take)
const char *launch_yuv_cdl(hipStream_t st, int variant, const LutConsts &L, const CdlConsts &C, const YuvConsts &K, const PlaneSet &P,
                           const FrameGeom &G, int din, int dout, int icsx, int icsy, int ocsx, int ocsy, int interp);
// its vector kernels, one translation unit per container mix (w<in wide><out wide>): nullptr = not a mode it has
#define LUTR_CD_DECL(tag) \
    const char *launch_yuv_cdl_vec_##tag(hipStream_t st, const LutConsts &L, const CdlConsts &C, const YuvConsts &K, \
                                         const PlaneSet &P, const FrameGeom &G, int icsx, int icsy, int ocsx, int ocsy, int interp);
LUTR_CD_DECL(w00) LUTR_CD_DECL(w11) LUTR_CD_DECL(w10)
#undef LUTR_CD_DECL

// 1D LUT ahead of lut3d (lutr_l1d.hip): the per-code table (device; the output code of integer code i of channel
// c is tab[c * stride + i], stride = 2^lut_depth)
struct L1dConsts {
    const uint16_t *tab;
    int stride;
};
// launch_yuv_cdl's call with the 1D table in the CDL's place; interp LUTR_INTERP_NONE = lut1d alone (L is not read).  nullptr =
// the variant cannot take the call (vec_lds always; vec_global on layouts the vector kernel cannot take)
const char *launch_yuv_l1d(hipStream_t st, int variant, const LutConsts &L, const L1dConsts &C, const YuvConsts &K, const PlaneSet &P,
                           const FrameGeom &G, int din, int dout, int icsx, int icsy, int ocsx, int ocsy, int interp);
// its vector kernels, one translation unit per container mix (w<in wide><out wide>); lds: stage the table per workgroup.
// nullptr = not a mode it has
#define LUTR_L1_DECL(tag) \
    const char *launch_yuv_l1d_vec_##tag(hipStream_t st, const LutConsts &L, const L1dConsts &C, const YuvConsts &K, \
                                         const PlaneSet &P, const FrameGeom &G, int icsx, int icsy, int ocsx, int ocsy, int interp, \
                                         bool lds);
LUTR_L1_DECL(w00) LUTR_L1_DECL(w11) LUTR_L1_DECL(w10)
#undef LUTR_L1_DECL
// lut1d alone on planar RGB: P in gbrp order (G, B, R), planes of `depth` bits.  nullptr as above
const char *launch_rgb_l1d(hipStream_t st, int variant, const L1dConsts &C, const PlaneSet &P, const FrameGeom &G, int depth);

// an ordered stack of lut1d / CDL / lut3d stages (lutr_stack.hip).  The stage list compiled into steps, one byte
// each from the low end of `ops`, a zero byte ends it: bits 0..3 the step, bits 4..7 the interpolation mode of a lattice step.
// A pixel is integer codes held as floats, or unit floats behind the CDL; the list says which at every step.
enum StackOp {
    STACK_OP_END        = 0,
    STACK_OP_LAT_CODES  = 1,     // the first lattice on codes: lut3d_px (prelut taken)
    STACK_OP_LAT_UNIT   = 2,     // the first lattice on unit floats: lut3d_unit
    STACK_OP_LAT2_CODES = 3,     // the second lattice, the same two forms
    STACK_OP_LAT2_UNIT  = 4,
    STACK_OP_L1D        = 5,     // codes -> codes through the 1D table
    STACK_OP_CDL        = 6,     // codes -> unit: cdl_px
    STACK_OP_ROUND      = 7,     // unit -> codes: (int)(o * maxf + 0.5f)
    STACK_OP_MTX_CODES  = 8,     // the RGB matrix on codes (codes -> unit) and on unit floats (unit -> unit): the matrix forms of
    STACK_OP_MTX_UNIT   = 9      // the kernels only
};
struct StackConsts {
    unsigned long long ops;      // at most 6 steps: four stages and two roundings (matrix, cdl, lut1d, lut3d)
    const float    *cdl_tab;     // CdlConsts::tab, or nullptr when no step reads it
    const uint16_t *l1d_tab;     // L1dConsts::tab, likewise
    int   stride;                // 2^lut_depth
    float sat;                   // the CDL's saturation (1 without one)
    float maxf;                  // (float)(2^lut_depth - 1)
    int   lds_cdl_words;         // 32-bit words of the tables the stack uses (0: not used): what an LDS placement stages
    int   lds_l1d_words;
};
// launch_yuv_chain's call with the step list; L / L2 are read by the lattice steps only.  nullptr = the variant cannot take the
// call (vec_lds always; vec_global on layouts the vector kernel cannot take and on pyramid / prism stages)
// The strength mix behind the list: frame f of the call takes frame[f] (device memory, nframes floats) when
// `frame` is set, else the scalar s; the kernels clamp either to [0, 1], NaN to 0.
struct MixConsts {
    const float *frame;
    float s;
};
// The matte behind the list: one plane of unsigned codes at luma resolution, bytes or 16-bit words; `data` is row
// 0 of the first frame, fstride 0 = one matte for every frame.  The strength of a pixel is its frame's times
// (invert ? maxf - min(a, maxf) : min(a, maxf)) * rcp.
struct MatteConsts {
    const uint8_t *data;
    long long stride, fstride;   // bytes
    float maxf;                  // (float)(2^depth - 1)
    float rcp;                   // 1.0f / maxf, formed on the host
    int   invert;
    int   wide;                  // 16-bit words
};
// The RGB matrix of a matrix step: twelve numbers and the host's 1.0f / maxf, passed by value -- wave-uniform, no
// table.  t_r = ((m[0] * u_r + m[1] * u_g) + m[2] * u_b) + off[0], rows 1 and 2 likewise; u = q * rcp on codes.
struct MtxConsts {
    float m[9];
    float off[3];
    float rcp;
};
// M = nullptr: the kernels of 3.21; else their mix forms (k_yuv_stack_mix_vec / k_yuv_stack_mix_generic), whatever the strength;
// A (with M): their matte forms (k_yuv_stack_matte_vec / k_yuv_stack_matte_generic), whatever the matte;
// X (without M and A): the matrix forms (k_yuv_stack_mtx_vec / k_yuv_stack_mtx_generic), the only ones with the matrix steps
const char *launch_yuv_stack(hipStream_t st, int variant, const LutConsts &L, const LutConsts &L2, const StackConsts &S,
                             const YuvConsts &K, const PlaneSet &P, const FrameGeom &G, int din, int dout, int icsx, int icsy,
                             int ocsx, int ocsy, const MixConsts *M, const MatteConsts *A, const MtxConsts *X = nullptr);
const char *launch_yuv_stack_mtx_generic(hipStream_t st, unsigned grid, const LutConsts &L, const LutConsts &L2, const StackConsts &S,
                                         const YuvConsts &K, const PlaneSet &P, const FrameGeom &G, const MtxConsts &X, int win,
                                         int wout, int icsx, int icsy, int ocsx, int ocsy);
// the matrix vector kernels, one translation unit per container mix (w<in wide><out wide>)
#define LUTR_SKX_DECL(tag) \
    const char *launch_yuv_stack_mtx_vec_##tag(hipStream_t st, const LutConsts &L, const LutConsts &L2, const StackConsts &S, \
                                               const YuvConsts &K, const PlaneSet &P, const FrameGeom &G, int icsx, int icsy, \
                                               int ocsx, int ocsy, bool tri, bool lds, MtxConsts X);
LUTR_SKX_DECL(w00) LUTR_SKX_DECL(w11) LUTR_SKX_DECL(w10)
#undef LUTR_SKX_DECL
const char *launch_yuv_stack_matte_generic(hipStream_t st, unsigned grid, const LutConsts &L, const LutConsts &L2, const StackConsts &S,
                                           const YuvConsts &K, const PlaneSet &P, const FrameGeom &G, const MixConsts &M,
                                           const MatteConsts &A, int win, int wout, int icsx, int icsy, int ocsx, int ocsy);
// the matte vector kernels, one translation unit per (w<in wide><out wide><matte wide>)
#define LUTR_SKA_DECL(tag) \
    const char *launch_yuv_stack_matte_vec_##tag(hipStream_t st, const LutConsts &L, const LutConsts &L2, const StackConsts &S, \
                                                 const YuvConsts &K, const PlaneSet &P, const FrameGeom &G, int icsx, int icsy, \
                                                 int ocsx, int ocsy, bool tri, bool lds, MixConsts M, MatteConsts A);
LUTR_SKA_DECL(w000) LUTR_SKA_DECL(w110) LUTR_SKA_DECL(w111) LUTR_SKA_DECL(w100) LUTR_SKA_DECL(w101)
#undef LUTR_SKA_DECL
// its vector kernels, one translation unit per container mix (w<in wide><out wide>) and form; tri: some lattice step is
// trilinear; lds: stage the tables per workgroup
const char *launch_yuv_stack_mix_generic(hipStream_t st, unsigned grid, const LutConsts &L, const LutConsts &L2, const StackConsts &S,
                                         const YuvConsts &K, const PlaneSet &P, const FrameGeom &G, const MixConsts &M, int win,
                                         int wout, int icsx, int icsy, int ocsx, int ocsy);
#define LUTR_SK_DECL(tag) \
    const char *launch_yuv_stack_vec_##tag(hipStream_t st, const LutConsts &L, const LutConsts &L2, const StackConsts &S, \
                                           const YuvConsts &K, const PlaneSet &P, const FrameGeom &G, int icsx, int icsy, int ocsx, \
                                           int ocsy, bool tri, bool lds); \
    const char *launch_yuv_stack_mix_vec_##tag(hipStream_t st, const LutConsts &L, const LutConsts &L2, const StackConsts &S, \
                                               const YuvConsts &K, const PlaneSet &P, const FrameGeom &G, int icsx, int icsy, \
                                               int ocsx, int ocsy, bool tri, bool lds, MixConsts M);
LUTR_SK_DECL(w00) LUTR_SK_DECL(w11) LUTR_SK_DECL(w10)
#undef LUTR_SK_DECL

// blue-noise dither in the output stage (lutr_bnd.hip): launch_yuv_xsub's call for any pair of layouts, the equal
// ones included; bn = the 64 x 64 table of offsets (device).  nullptr = the variant cannot take the call (vec_lds always;
// vec_global on layouts the vector kernel cannot take)
const char *launch_yuv_bn(hipStream_t st, int variant, const LutConsts &L, const YuvConsts &K, const PlaneSet &P, const FrameGeom &G,
                          const float *bn, int din, int dout, int icsx, int icsy, int ocsx, int ocsy, int interp);
// its vector kernels, one translation unit per container mix (w<in wide><out wide>): nullptr = not a mode it has
#define LUTR_BN_DECL(tag) \
    const char *launch_yuv_bn_vec_##tag(hipStream_t st, const LutConsts &L, const YuvConsts &K, const PlaneSet &P, \
                                        const FrameGeom &G, const float *bn, int icsx, int icsy, int ocsx, int ocsy, int interp);
LUTR_BN_DECL(w00) LUTR_BN_DECL(w11) LUTR_BN_DECL(w10)
#undef LUTR_BN_DECL

// two outputs from one pass (lutr_dual.hip): input layout icsx, icsy; output 1 in P.d (depth dout1, layout csx1, csy1,
// constants K1), output 2 in D2 (dout2, csx2, csy2, K2); K1 and K2 share the input stage.  nullptr = the variant cannot take the
// call (vec_lds always; vec_global on layouts the vector kernel cannot take)
const char *launch_yuv_dual(hipStream_t st, int variant, const LutConsts &L, const YuvConsts &K1, const YuvConsts &K2,
                            const PlaneSet &P, const DstPlanes &D2, const FrameGeom &G, int din, int dout1, int csx1, int csy1,
                            int dout2, int csx2, int csy2, int icsx, int icsy, int interp);
// its vector kernels, one translation unit per container mix (w<in wide><A wide><B wide>): output A (P.d, KA) is 4:2:2, output B
// has the layout bcsx, bcsy; nullptr = not a layout / mode it has
#define LUTR_DU_DECL(tag) \
    const char *launch_yuv_dual_vec_##tag(hipStream_t st, const LutConsts &L, const YuvConsts &KA, const YuvConsts &KB, \
                                          const PlaneSet &P, const DstPlanes &B, const FrameGeom &G, int icsx, int icsy, int bcsx, \
                                          int bcsy, int interp);
LUTR_DU_DECL(w111) LUTR_DU_DECL(w110) LUTR_DU_DECL(w000)
#undef LUTR_DU_DECL

// semi-planar frames (lutr_semi.hip): the container of each side -- planar (three planes) or semi-planar (PlaneSet
// slot 1 holds the Cb / Cr pairs, slot 2 is not read), Cr first with `swap`, 16-bit codes `shift` bits up in their words.  Both
// sides are csx = 1 with the same csy.  nullptr = the variant cannot take the call (vec_lds always; vec_global on layouts the
// vector kernel cannot take)
struct SemiArgs {
    int isemi, iswap, ishift;
    int osemi, oswap, oshift;
};
const char *launch_yuv_semi(hipStream_t st, int variant, const LutConsts &L, const YuvConsts &K, const PlaneSet &P,
                            const FrameGeom &G, const SemiArgs &A, int din, int dout, int csy, int interp);
// its vector kernels, one translation unit per container mix (w<in wide><out wide>): nullptr = not a side pair / mode it has
#define LUTR_SM_DECL(tag) \
    const char *launch_yuv_semi_vec_##tag(hipStream_t st, const LutConsts &L, const YuvConsts &K, const PlaneSet &P, \
                                          const FrameGeom &G, const SemiArgs &A, int csy, int interp);
LUTR_SM_DECL(w00) LUTR_SM_DECL(w11) LUTR_SM_DECL(w10)
#undef LUTR_SM_DECL

// the stage stack on semi-planar sides (lutr_stack.hip's SEMI forms): launch_yuv_stack's plain call for the eight
// layout pairs with a 4:2:0 / 4:2:2 side, each side in the container A gives it (as launch_yuv_semi's; any pair, planar both ways
// included, goes to the generic kernel).  nullptr = the variant cannot take the call (vec_lds always; vec_global on layouts the
// vector kernel cannot take)
const char *launch_yuv_stack_semi(hipStream_t st, int variant, const LutConsts &L, const LutConsts &L2, const StackConsts &S,
                                  const YuvConsts &K, const PlaneSet &P, const FrameGeom &G, const SemiArgs &A, int din, int dout,
                                  int icsx, int icsy, int ocsx, int ocsy);
const char *launch_yuv_stack_semi_generic(hipStream_t st, unsigned grid, const LutConsts &L, const LutConsts &L2, const StackConsts &S,
                                          const YuvConsts &K, const PlaneSet &P, const FrameGeom &G, const SemiArgs &A, int win,
                                          int wout, int icsx, int icsy, int ocsx, int ocsy);
// its vector kernels, one translation unit per container mix (w<in wide><out wide>): nullptr = not a layout pair it has
#define LUTR_SKS_DECL(tag) \
    const char *launch_yuv_stack_semi_vec_##tag(hipStream_t st, const LutConsts &L, const LutConsts &L2, const StackConsts &S, \
                                                const YuvConsts &K, const PlaneSet &P, const FrameGeom &G, int icsx, int icsy, \
                                                int ocsx, int ocsy, bool tri, bool lds, SemiArgs A);
LUTR_SKS_DECL(w00) LUTR_SKS_DECL(w11) LUTR_SKS_DECL(w10)
#undef LUTR_SKS_DECL

// packed 4:2:2 frames (lutr_pkyuv.hip): the container of each side -- planar (three planes) or packed (PlaneSet
// slot 0 holds the groups, slots 1 and 2 are not read); cf: chroma first in a group (uyvy422), csw: Cr ahead of Cb (yvyu422),
// 16-bit codes `shift` bits up in their words.  The source is 4:2:2; the destination is 4:2:2, or planar with the layout ocsx,
// ocsy (K then carries the output block's 1/n).  nullptr = the variant cannot take the call (vec_lds always; vec_global on layouts
// the vector kernel cannot take)
struct PkArgs {
    int ipk, icf, icsw, ishift;
    int opk, ocf, ocsw, oshift;
};
const char *launch_yuv_packed(hipStream_t st, int variant, const LutConsts &L, const YuvConsts &K, const PlaneSet &P,
                              const FrameGeom &G, const PkArgs &A, int din, int dout, int ocsx, int ocsy, int interp);
// its vector kernels, one translation unit per container mix (w<in wide><out wide>): nullptr = not a side pair / mode it has
#define LUTR_PK_DECL(tag) \
    const char *launch_yuv_pk_vec_##tag(hipStream_t st, const LutConsts &L, const YuvConsts &K, const PlaneSet &P, \
                                        const FrameGeom &G, const PkArgs &A, int ocsy, int interp);
LUTR_PK_DECL(w00) LUTR_PK_DECL(w11) LUTR_PK_DECL(w10)
#undef LUTR_PK_DECL

// v210 frames (lutr_v210.hip): the container of each side -- planar (three planes) or v210 (PlaneSet slot 0 holds the
// groups of four words, slots 1 and 2 are not read).  A v210 side is 10-bit 4:2:2; the source is 4:2:2; the destination is 4:2:2,
// or planar with the layout ocsx, ocsy (K then carries the output block's 1/n).  din / dout: the depths of the two sides (10 for a
// v210 one).  nullptr = the variant cannot take the call (vec_lds always; vec_global on layouts the vector kernel cannot take)
struct V210Args {
    int iv, ov;
};
// luma samples a thread of the vector kernels takes per row: whole groups that make whole words on the planar side (wp: it is 16 bit)
inline int v210_unit_px(const V210Args &A, int wp) { return (A.iv && A.ov) ? 6 : (wp ? 12 : 24); }
const char *launch_yuv_v210(hipStream_t st, int variant, const LutConsts &L, const YuvConsts &K, const PlaneSet &P,
                            const FrameGeom &G, const V210Args &A, int din, int dout, int ocsx, int ocsy, int interp);
// its vector kernels, one translation unit per container mix (w<in wide><out wide>, a v210 side counted as wide): nullptr = not a
// side pair / mode it has
#define LUTR_V2_DECL(tag) \
    const char *launch_yuv_v210_vec_##tag(hipStream_t st, const LutConsts &L, const YuvConsts &K, const PlaneSet &P, \
                                          const FrameGeom &G, const V210Args &A, int ocsy, int interp);
LUTR_V2_DECL(w11) LUTR_V2_DECL(w10)
#undef LUTR_V2_DECL

// the stage stack on packed 4:2:2 and v210 frames (lutr_pkstack.hip): launch_yuv_packed's / launch_yuv_v210's call
// with launch_yuv_stack's plain step list in place of the one lattice.  nullptr = the variant cannot take the call (vec_lds always;
// vec_global on layouts the vector kernel cannot take and on pyramid / prism stages)
const char *launch_yuv_stack_packed(hipStream_t st, int variant, const LutConsts &L, const LutConsts &L2, const StackConsts &S,
                                    const YuvConsts &K, const PlaneSet &P, const FrameGeom &G, const PkArgs &A, int din, int dout,
                                    int ocsx, int ocsy);
const char *launch_yuv_stack_v210(hipStream_t st, int variant, const LutConsts &L, const LutConsts &L2, const StackConsts &S,
                                  const YuvConsts &K, const PlaneSet &P, const FrameGeom &G, const V210Args &A, int din, int dout,
                                  int ocsx, int ocsy);
// their vector kernels, one translation unit per container mix (w<in wide><out wide>, a v210 side counted as wide); tri: some
// lattice step is trilinear; lds: stage the tables per workgroup; nullptr = not a side pair it has
#define LUTR_PKS_DECL(tag) \
    const char *launch_yuv_stack_pk_vec_##tag(hipStream_t st, const LutConsts &L, const LutConsts &L2, const StackConsts &S, \
                                              const YuvConsts &K, const PlaneSet &P, const FrameGeom &G, const PkArgs &A, int ocsy, \
                                              bool tri, bool lds);
LUTR_PKS_DECL(w00) LUTR_PKS_DECL(w11) LUTR_PKS_DECL(w10)
#undef LUTR_PKS_DECL
#define LUTR_VKS_DECL(tag) \
    const char *launch_yuv_stack_v210_vec_##tag(hipStream_t st, const LutConsts &L, const LutConsts &L2, const StackConsts &S, \
                                                const YuvConsts &K, const PlaneSet &P, const FrameGeom &G, const V210Args &A, \
                                                int ocsy, bool tri, bool lds);
LUTR_VKS_DECL(w11) LUTR_VKS_DECL(w10)
#undef LUTR_VKS_DECL

// pass 2 of the dither path alone (k_dither_ed on the float planes F, chroma planes in the output layout); false = rows too wide
bool launch_dither_ed(hipStream_t st, const YuvConsts &K, const PlaneSet &P, const FrameGeom &G, const FloatPlanes &F, int wout,
                      int ocsx, int ocsy);

// RGB source -> YUV output (lutr_rgb2yuv.hip).  The source travels in PlaneSet::s as three component streams in
// R, G, B order: planar = the three planes (step 1, offsets 0); packed = the image's base three times, `step` components per
// pixel, component index ro / go / bo inside a pixel.  PlaneSet::d is Y, Cb, Cr.
struct RgbLayout {
    int step;          // components per pixel in a stream: 1 planar, 3 | 4 packed
    int wide;          // 16-bit container
    int ro, go, bo;    // component index of R, G, B inside a pixel (0 for planar)
};
// mode: LUTR_INTERP_*, or -1 = no lut3d (the source codes go straight to the output stage).  nullptr = the variant cannot take
// the call (vec_lds always; vec_global on layouts the vector kernel cannot take)
const char *launch_rgb2yuv(hipStream_t st, int variant, const LutConsts &L, const YuvConsts &K, const PlaneSet &P,
                           const RgbLayout &Y, const FrameGeom &G, int dout, int ocsx, int ocsy, int mode);
// its vector kernels, one translation unit per container mix (w<in wide><out wide>): nullptr = not a layout / mode it has
#define LUTR_R2Y_DECL(tag) \
    const char *launch_rgb2yuv_vec_##tag(hipStream_t st, const LutConsts &L, const YuvConsts &K, const PlaneSet &P, \
                                         const RgbLayout &Y, const FrameGeom &G, int ocsx, int ocsy, int mode);
LUTR_R2Y_DECL(w00) LUTR_R2Y_DECL(w11) LUTR_R2Y_DECL(w10)
#undef LUTR_R2Y_DECL
// the dither path: the unquantised pass by output blocks (k_rgb2yuv_float), then k_dither_ed; whole frames
const char *launch_rgb2yuv_dither(hipStream_t st, const LutConsts &L, const YuvConsts &K, const PlaneSet &P, const RgbLayout &Y,
                                  const FrameGeom &G, const FloatPlanes &F, int dout, int ocsx, int ocsy, int mode);

// the stage stack on an RGB source (lutr_rgbstack.hip): launch_rgb2yuv's source (P.s, Y) through the step list S
// (StackConsts, as launch_yuv_stack takes it; X is read by the matrix steps only) into one of two sinks: SINK_YUV = P.d is Y, Cb,
// Cr at depth dout in the layout ocsx, ocsy, through K; SINK_RGB = P.d is three planes in R, G, B order at the source's depth
// (dout is that depth, ocsx = ocsy = 0, K is not read; P.d may be P.s).  nullptr = the variant cannot take the call (vec_lds
// always; vec_global on layouts the vector kernel cannot take and on pyramid / prism stages)
enum RgbStackSink { SINK_YUV = 0, SINK_RGB = 1 };
const char *launch_rgb_stack(hipStream_t st, int variant, const LutConsts &L, const LutConsts &L2, const StackConsts &S,
                             const MtxConsts &X, const YuvConsts &K, const PlaneSet &P, const RgbLayout &Y, const FrameGeom &G,
                             int sink, int dout, int ocsx, int ocsy);
// its vector kernels, one translation unit per container mix (w<in wide><out wide>); tri: some lattice step is trilinear; lds:
// stage the tables per workgroup.  nullptr = not a source kind / sink / layout it has
#define LUTR_RSK_DECL(tag) \
    const char *launch_rgb_stack_vec_##tag(hipStream_t st, const LutConsts &L, const LutConsts &L2, const StackConsts &S, \
                                           const MtxConsts &X, const YuvConsts &K, const PlaneSet &P, const RgbLayout &Y, \
                                           const FrameGeom &G, int sink, int ocsx, int ocsy, bool tri, bool lds);
LUTR_RSK_DECL(w00) LUTR_RSK_DECL(w11) LUTR_RSK_DECL(w10)
#undef LUTR_RSK_DECL

// the blue-noise path: the generic kernel with a DitherSink, row shards allowed; nullptr = a vector variant was
// asked for (this path has no vector kernel yet)
const char *launch_rgb2yuv_bn(hipStream_t st, int variant, const LutConsts &L, const YuvConsts &K, const PlaneSet &P,
                              const RgbLayout &Y, const FrameGeom &G, const float *bn, int dout, int ocsx, int ocsy, int mode);

// YUV source -> RGB output (lutr_yuv2rgb.hip).  PlaneSet::s is Y, Cb, Cr at depth din in the layout icsx, icsy; the
// destination travels in PlaneSet::d as three component streams in R, G, B order, described by Y as the source of launch_rgb2yuv
// is (planar = the three planes; packed = the image's base three times; the fourth component of a 4-component image is written
// K.max_l).  mode: LUTR_INTERP_*, or -1 = no lut3d.  nullptr = the variant cannot take the call (vec_lds always; vec_global on
// layouts the vector kernel cannot take)
const char *launch_yuv2rgb(hipStream_t st, int variant, const LutConsts &L, const YuvConsts &K, const PlaneSet &P,
                           const RgbLayout &Y, const FrameGeom &G, int din, int icsx, int icsy, int mode);
// its vector kernels, one translation unit per container mix (w<in wide><out wide>): nullptr = not a layout / mode it has
#define LUTR_Y2R_DECL(tag) \
    const char *launch_yuv2rgb_vec_##tag(hipStream_t st, const LutConsts &L, const YuvConsts &K, const PlaneSet &P, \
                                         const RgbLayout &Y, const FrameGeom &G, int icsx, int icsy, int mode);
LUTR_Y2R_DECL(w00) LUTR_Y2R_DECL(w11) LUTR_Y2R_DECL(w10)
#undef LUTR_Y2R_DECL

// the stage stack from a YUV source into an RGB frame (lutr_y2rstack.hip): launch_yuv2rgb's source and destination
// (P, Y, din, icsx, icsy) with the step list S of launch_rgb_stack (L2, X likewise) between yuv_to_rgb and the stores.  nullptr =
// the variant cannot take the call (vec_lds always; vec_global on layouts the vector kernel cannot take and on pyramid / prism
// stages)
const char *launch_yuv2rgb_stack(hipStream_t st, int variant, const LutConsts &L, const LutConsts &L2, const StackConsts &S,
                                 const MtxConsts &X, const YuvConsts &K, const PlaneSet &P, const RgbLayout &Y, const FrameGeom &G,
                                 int din, int icsx, int icsy);
// its vector kernels, one translation unit per container mix (w<in wide><out wide>); tri: some lattice step is trilinear; lds:
// stage the tables per workgroup.  nullptr = not a layout / destination kind it has
#define LUTR_YRS_DECL(tag) \
    const char *launch_yuv2rgb_stack_vec_##tag(hipStream_t st, const LutConsts &L, const LutConsts &L2, const StackConsts &S, \
                                               const MtxConsts &X, const YuvConsts &K, const PlaneSet &P, const RgbLayout &Y, \
                                               const FrameGeom &G, int icsx, int icsy, bool tri, bool lds);
LUTR_YRS_DECL(w00) LUTR_YRS_DECL(w11) LUTR_YRS_DECL(w10)
#undef LUTR_YRS_DECL

// planar float RGB sources (lutr_rgbf.hip): gbrpf32 planes in PlaneSet::s in R, G, B order.  No per-code
// coordinate table exists for a float input, so lut3d's prelut travels as the raw table lutr_ctx_set_prelut was given and is
// applied per pixel (FFmpeg's prelut_interp_1d_linear); LutConsts::pre is not read by these kernels.
struct FloatPre {
    const float *tab;  // 3 x size floats (device), or nullptr: no prelut
    int   size;
    float min[3], scale[3];
};
// float in, float out (PlaneSet::d in R, G, B order too; may be the source).  nullptr as for launch_rgb2yuv
const char *launch_rgbf(hipStream_t st, int variant, const LutConsts &L, const FloatPre &Q, const PlaneSet &P, const FrameGeom &G,
                        int mode);
// float in, Y / Cb / Cr out: the lattice's output quantised to 16-bit codes, then 3.9's output stage at lut_depth 16.  mode as for
// launch_rgb2yuv (-1 = no lut3d)
const char *launch_rgbf2yuv(hipStream_t st, int variant, const LutConsts &L, const FloatPre &Q, const YuvConsts &K, const PlaneSet &P,
                            const FrameGeom &G, int dout, int ocsx, int ocsy, int mode);
// its vector kernels, one translation unit per output container (w<out wide>)
#define LUTR_RGBF_DECL(tag) \
    const char *launch_rgbf2yuv_vec_##tag(hipStream_t st, const LutConsts &L, const FloatPre &Q, const YuvConsts &K, \
                                          const PlaneSet &P, const FrameGeom &G, int ocsx, int ocsy, int mode);
LUTR_RGBF_DECL(w0) LUTR_RGBF_DECL(w1)
#undef LUTR_RGBF_DECL
// the dither path: k_rgbf2yuv_float, then k_dither_ed; whole frames
const char *launch_rgbf2yuv_dither(hipStream_t st, const LutConsts &L, const FloatPre &Q, const YuvConsts &K, const PlaneSet &P,
                                   const FrameGeom &G, const FloatPlanes &F, int dout, int ocsx, int ocsy, int mode);

// the blue-noise path: as launch_rgb2yuv_bn
const char *launch_rgbf2yuv_bn(hipStream_t st, int variant, const LutConsts &L, const FloatPre &Q, const YuvConsts &K,
                               const PlaneSet &P, const FrameGeom &G, const float *bn, int dout, int ocsx, int ocsy, int mode);

// the alpha plane of yuva* / gbrap* frames (lutr_alpha.hip): one plane in (none for a fill), one plane out
struct AlphaArgs {
    const uint8_t *s;                // nullptr with kind 0
    uint8_t       *d;
    long long ss, ds, sfs, dfs;      // row / frame strides, bytes
    int kind;                        // LUTR_ALPHA_NONE (fill) | LUTR_ALPHA_INT | LUTR_ALPHA_FLOAT
    int swide, wout;                 // 16-bit words on the integer source / on the destination
    int step, off;                   // source sample of pixel x: element x * step + off of its row (a plane: 1, 0)
    int copy;                        // integer source at the destination's depth: the words are copied
    unsigned mi, mo;                 // 2^din - 1 (integer source), 2^dout - 1
    unsigned long long k;            // a' = (min(word, mi) * k + 2^39) >> 40
    float mof;                       // (float)mo
};
// fills everything of A but the planes and step / off; false = no multiplier passed the host's check of the depth pair
bool alpha_consts(AlphaArgs *A, int kind, int din, int dout);
// nullptr = the variant cannot take the call (vec_lds always; vec_global on layouts the vector kernel cannot take)
const char *launch_alpha(hipStream_t st, int variant, const AlphaArgs &A, const FrameGeom &G);

// premultiplied alpha (lutr_premul.hip): the source's alpha plane beside its colour planes -- luma-sized, one
// element per pixel, at the source's depth (integer YUV) or float32 (float RGB)
struct AlphaIn {
    const uint8_t *a;
    long long as, afs;               // row / frame strides, bytes
};
// the colour planes and the alpha plane of one call: what launch_vec_or_generic hands through to this path's callbacks
struct PremulPlanes {
    PlaneSet p;
    AlphaIn  a;
};
struct PremulConsts {
    uint32_t ma, ml;                 // 2^din - 1 (alpha has the source's depth), 2^lut_depth - 1 (<= ma: the callers keep them equal)
    int      din;                    // the alpha depth: ma = 2^din - 1
};
// launch_yuv_xsub's call for any pair of layouts, the equal ones included, with unpremultiply / premultiply around lut3d.
// nullptr = the variant cannot take the call (vec_lds always; vec_global on layouts the vector kernel cannot take)
const char *launch_yuva_premul(hipStream_t st, int variant, const LutConsts &L, const YuvConsts &K, const PremulPlanes &P,
                               const FrameGeom &G, int din, int dout, int lut_depth, int icsx, int icsy, int ocsx, int ocsy,
                               int interp);
// its vector kernels, one translation unit per container mix (w<in wide><out wide>): nullptr = not a mode it has
#define LUTR_PM_DECL(tag) \
    const char *launch_yuva_premul_vec_##tag(hipStream_t st, const LutConsts &L, const YuvConsts &K, const PremulConsts &M, \
                                             const PremulPlanes &P, const FrameGeom &G, int icsx, int icsy, int ocsx, int ocsy, \
                                             int interp);
LUTR_PM_DECL(w00) LUTR_PM_DECL(w11) LUTR_PM_DECL(w10)
#undef LUTR_PM_DECL
// launch_rgbf's call (planes in R, G, B order, the destination may be the source) with the float alpha plane as a fourth stream
const char *launch_rgbaf_premul(hipStream_t st, int variant, const LutConsts &L, const FloatPre &Q, const PremulPlanes &P,
                                const FrameGeom &G, int interp);

// round-2 tile kernels (lutr_tile2.hip, one translation unit per format: w<in wide><out wide>_c<csx><csy>); nullptr =
// this combination is not built / cannot take the call, the caller falls back
#define LUTR_T2_DECL(tag) \
    const char *launch_yuv_tile2_##tag(hipStream_t st, const LutConsts &L, const YuvConsts &K, const PlaneSet &P, \
                                       const FrameGeom &G, int din, int dout, int lut_depth, int csx, int csy, int mode, \
                                       bool fast, unsigned *stats, unsigned *queue);
LUTR_T2_DECL(w00_c11) LUTR_T2_DECL(w00_c10) LUTR_T2_DECL(w00_c00)
LUTR_T2_DECL(w11_c11) LUTR_T2_DECL(w11_c10) LUTR_T2_DECL(w11_c00)
LUTR_T2_DECL(w10_c11) LUTR_T2_DECL(w10_c10) LUTR_T2_DECL(w10_c00)
#undef LUTR_T2_DECL
// sited chroma resampling (lutr_sited.hip): 4:2:0 / 4:2:2, loc = LUTR_CHROMA_LEFT / CENTER / TOPLEFT; K carries the
// down-sampling's 1/n in cbr..crb (make_yuv_consts_sited); nullptr = the launch is too large
const char *launch_yuv_sited(hipStream_t st, const LutConsts &L, const YuvConsts &K, const PlaneSet &P, const FrameGeom &G,
                             int din, int dout, int csy, int loc, int mode);
// output resize (lutr_resize.hip): one plane's geometry and Q14 tables (device), for a grid of output tiles of
// 64 columns x RzArgs::th rows (64, 32 or 16: the tallest whose LDS fits)
constexpr int kRzTileW = 64, kRzTileHMax = 64;
constexpr int kRzRows = 8, kRzU = 4;     // staged source rows per wave and step (most); samples per lane and row in one load batch
struct RzPlane {
    const uint8_t *s;
    uint8_t *d;
    long long ss, ds, sfs, dfs;      // row / frame strides, bytes
    int sw, sh, dw, dh;              // plane sizes, samples
    const int *xs, *xw;              // per output column: first tap (unclamped), nx weights ([column][tap])
    const int *ys, *yw;              // per output row: first tap, ny weights
    int nx, ny;
    int tiles_x, tile0;              // tile columns of this plane; index of its first tile inside a frame
};
struct RzArgs {
    RzPlane p[3];
    int tiles_per_frame;
    int depth;                       // 8..16 (8: uint8 planes, else uint16)
    int spx, spy;                    // largest footprint of a tile over the three planes: source columns, source rows
    int nx_max, ny_max;
    int th;                          // output rows per tile
    int rows;                        // staged source rows per wave and step, 1..kRzRows (the most whose LDS fits 64 KiB)
};
size_t resize_lds_bytes(const RzArgs &A);
// nullptr = too many tiles, or a footprint that does not fit the workgroup's LDS
const char *launch_resize(hipStream_t st, RzArgs A, int nframes);
// fp16 lattice of the fast variant and fp32 pre-multiplied lattice of the fma32 variant (lutr_lat16.hip)
void launch_make_lat16(hipStream_t st, const float4 *lat, uint2 *out, size_t nodes, float m);
void launch_make_latm(hipStream_t st, const float4 *lat, float4 *out, size_t nodes, float m);

// persistent LDS-window kernels (lutr_tile.hip); layout already checked by launch_rgb/launch_yuv
const char *launch_rgb_tile(hipStream_t st, const LutConsts &L, const PlaneSet &P, const FrameGeom &G,
                            int depth, int interp, unsigned *stats, unsigned *queue);

// host helpers (lutr_api.cpp)
int make_yuv_consts(const lutr_yuv_params &p, YuvConsts *out);
int make_yuv_consts_xsub(const lutr_yuv_params &p, YuvConsts *out);
int make_yuv_consts_sited(const lutr_yuv_params &p, int chroma_loc, YuvConsts *out);
int make_yuv_consts_rgb2yuv(const lutr_yuv_params &p, YuvConsts *out);
int make_yuv_consts_yuv2rgb(const lutr_yuv_params &p, YuvConsts *out);
void set_error(const char *fmt, ...);

}  // namespace lutr
#endif  // LUTR_HOST_ONLY
