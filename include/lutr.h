/*
 * lutr.h -- C-ABI of the MI355X-native 3D-LUT apply engine (liblutr.so).
 *
 * This is the drop-in boundary for ONE path of ionlz/LUT-renderer: the per-pixel
 * work the reference delegates to the external `ffmpeg` process through the
 * filter string it builds at
 *     src/lut_renderer/ffmpeg.py:246   lut3d=file='<cube>':interp=<mode>
 * together with the conversions it (or ffmpeg's filter negotiation) puts around
 * that filter:
 *     src/lut_renderer/ffmpeg.py:212-236   scale=in_range=..:out_range=..:in_color_matrix=..
 *     src/lut_renderer/ffmpeg.py:224,233   format=<8-bit intermediate>
 *     src/lut_renderer/ffmpeg.py:304-310   format=<pix_fmt>
 * The reference has no FFI for this path (it spawns a process,
 * src/lut_renderer/task_manager.py:145-151); these entry points are what a
 * ctypes binding would load instead (INTEGRATION.md shows the stub).
 *
 * Conventions
 *   - plain pointers and sizes only; no torch / HIP types in signatures
 *     (a HIP stream crosses as void*).
 *   - every function returns 0 on success or a negative errno-style code;
 *     lutr_last_error() returns a thread-local message for the last failure.
 *   - pixel-plane pointers handed to lutr_apply_* are DEVICE pointers on the
 *     context's GPU.  The library never falls back to the CPU: with no usable
 *     GPU, lutr_ctx_create fails with LUTR_EIO.
 *   - the caller owns every buffer it passes; the library owns the context,
 *     its stream (unless one is injected) and the device copy of the lattice.
 *   - a context is not shared between threads; different contexts are independent.
 */
#ifndef LUTR_H
#define LUTR_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define LUTR_VERSION_STRING "0.1.0"

/* error codes (negative errno values; mirrors FFmpeg's AVERROR(EINVAL) / AVERROR_INVALIDDATA split) */
#define LUTR_OK        0
#define LUTR_ENOENT   (-2)    /* file not found */
#define LUTR_EIO      (-5)    /* HIP runtime failure / no GPU */
#define LUTR_ENOMEM   (-12)
#define LUTR_EINVAL   (-22)   /* bad argument, unsupported format, LUT_3D_SIZE outside [2,256] */
#define LUTR_EILSEQ   (-84)   /* malformed .cube ("invalid data"), unexpected EOF */

/* interpolation, numbered like FFmpeg's lut3d `interp` option values
 * (replaces the interp= half of ffmpeg.py:242-246) */
enum lutr_interp {
    LUTR_INTERP_NEAREST     = 0,
    LUTR_INTERP_TRILINEAR   = 1,
    LUTR_INTERP_TETRAHEDRAL = 2,
    LUTR_INTERP_PYRAMID     = 3,
    LUTR_INTERP_PRISM       = 4
};

/* YUV<->RGB matrices the reference can name (ffmpeg.py:119-125) */
enum lutr_matrix {
    LUTR_MATRIX_BT709  = 0,
    LUTR_MATRIX_BT601  = 1,   /* smpte170m and bt470bg */
    LUTR_MATRIX_BT2020 = 2    /* bt2020nc; bt2020c uses the same coefficients */
};

/* ranges (in_range=/out_range= at ffmpeg.py:225) */
enum lutr_range { LUTR_RANGE_TV = 0, LUTR_RANGE_PC = 1 };

/* planar YUV formats: depth | csx<<8 | csy<<9  (csx/csy = log2 chroma subsampling) */
#define LUTR_FMT(depth, csx, csy) ((depth) | ((csx) << 8) | ((csy) << 9))
#define LUTR_FMT_DEPTH(f) ((f) & 0xff)
#define LUTR_FMT_CSX(f)   (((f) >> 8) & 1)
#define LUTR_FMT_CSY(f)   (((f) >> 9) & 1)
#define LUTR_FMT_YUV420P     LUTR_FMT(8, 1, 1)
#define LUTR_FMT_YUV422P     LUTR_FMT(8, 1, 0)
#define LUTR_FMT_YUV444P     LUTR_FMT(8, 0, 0)
#define LUTR_FMT_YUV420P10   LUTR_FMT(10, 1, 1)
#define LUTR_FMT_YUV422P10   LUTR_FMT(10, 1, 0)
#define LUTR_FMT_YUV444P10   LUTR_FMT(10, 0, 0)
#define LUTR_FMT_YUV420P12   LUTR_FMT(12, 1, 1)
#define LUTR_FMT_YUV422P12   LUTR_FMT(12, 1, 0)
#define LUTR_FMT_YUV444P12   LUTR_FMT(12, 0, 0)

/* What the filter chain around lut3d does to a YUV frame (ffmpeg.py:212-236, :304-310).
 *   src codes (fmt_in, range_src)
 *     -> optional prologue to (lut_depth, range_in)       scale=in_range=pc:out_range=..,format=yuv4xxp
 *     -> integer RGB at lut_depth via matrix_in           (auto-inserted scaler ahead of lut3d)
 *     -> lut3d                                            ffmpeg.py:246
 *     -> YUV (fmt_out, range_out) via matrix_out          format=<pix_fmt>, ffmpeg.py:309
 * The prologue runs iff range_src != range_in or depth(fmt_in) != lut_depth.
 * fmt_in and fmt_out must have the same chroma subsampling. */
typedef struct lutr_yuv_params {
    int32_t fmt_in;
    int32_t fmt_out;
    int32_t lut_depth;
    int32_t matrix_in;
    int32_t matrix_out;
    int32_t range_src;
    int32_t range_in;
    int32_t range_out;
} lutr_yuv_params;

/* One frame (or a batch of equally laid out frames) of three planes.
 * stride = bytes between rows; frame_stride = bytes between consecutive frames of
 * a batch (ignored when nframes == 1).  Planar RGB uses FFmpeg's gbrp order
 * (plane 0 = G, 1 = B, 2 = R); YUV uses Y, Cb, Cr. */
typedef struct lutr_planes {
    void     *data[3];
    ptrdiff_t stride[3];
    int64_t   frame_stride[3];
} lutr_planes;

/* Packed (interleaved) RGB formats lut3d accepts: bits per component (8|16, 16 = little-endian
 * uint16), components per pixel (3|4) and the component index of R, G, B inside a pixel; the
 * remaining slot of a 4-component format (alpha or padding) is copied from source to destination. */
#define LUTR_PACKED(bits, ncomp, ro, go, bo) ((bits) | ((ncomp) << 8) | ((ro) << 12) | ((go) << 16) | ((bo) << 20))
#define LUTR_PACKED_BITS(f)  ((f) & 0xff)
#define LUTR_PACKED_NCOMP(f) (((f) >> 8) & 0xf)
#define LUTR_PACKED_RO(f)    (((f) >> 12) & 0xf)
#define LUTR_PACKED_GO(f)    (((f) >> 16) & 0xf)
#define LUTR_PACKED_BO(f)    (((f) >> 20) & 0xf)
#define LUTR_PK_RGB24    LUTR_PACKED(8, 3, 0, 1, 2)
#define LUTR_PK_BGR24    LUTR_PACKED(8, 3, 2, 1, 0)
#define LUTR_PK_RGBA     LUTR_PACKED(8, 4, 0, 1, 2)   /* also rgb0 */
#define LUTR_PK_BGRA     LUTR_PACKED(8, 4, 2, 1, 0)   /* also bgr0 */
#define LUTR_PK_ARGB     LUTR_PACKED(8, 4, 1, 2, 3)   /* also 0rgb */
#define LUTR_PK_ABGR     LUTR_PACKED(8, 4, 3, 2, 1)   /* also 0bgr */
#define LUTR_PK_RGB48LE  LUTR_PACKED(16, 3, 0, 1, 2)
#define LUTR_PK_BGR48LE  LUTR_PACKED(16, 3, 2, 1, 0)
#define LUTR_PK_RGBA64LE LUTR_PACKED(16, 4, 0, 1, 2)
#define LUTR_PK_BGRA64LE LUTR_PACKED(16, 4, 2, 1, 0)

/* one interleaved image, or a batch of equally laid out ones */
typedef struct lutr_packed {
    void     *data;
    ptrdiff_t stride;          /* bytes between rows */
    int64_t   frame_stride;    /* bytes between frames of a batch (ignored when nframes == 1) */
} lutr_packed;

typedef struct lutr_ctx lutr_ctx;

const char *lutr_version(void);
const char *lutr_last_error(void);

/* ---- .cube files (host side; what lut3d's file= option does, ffmpeg.py:246) ---- */
/* Parses `path` with FFmpeg's parse_cube semantics.  On success *rgb is a malloc'ed
 * n*n*n*3 float lattice indexed ((r*n+g)*n+b)*3+c (blue fastest), scale[c] =
 * clip(1/(DOMAIN_MAX[c]-DOMAIN_MIN[c]), 0, 1).  Free with lutr_cube_free. */
int  lutr_cube_parse(const char *path, float **rgb, int *n, float scale[3]);
void lutr_cube_free(float *rgb);
/* Any 3D LUT file lut3d's file= option accepts, chosen by extension like FFmpeg does: .cube (as above),
 * .dat, .3dl, .m3d, .csp (cineSpace).  Same outputs as lutr_cube_parse; free with lutr_cube_free.  Unknown extension: LUTR_EINVAL.
 * A .csp file whose three channels carry a pre-LUT (a 1D shaper ahead of the cube, lut3d's `prelut`) needs lutr_lut_parse_ex:
 * lutr_lut_parse returns LUTR_EINVAL for it rather than dropping the shaper. */
int  lutr_lut_parse(const char *path, float **rgb, int *n, float scale[3]);
/* As lutr_lut_parse, plus the file's prelut as lut3d builds it (/root/reference never sees it: FFmpeg's vf_lut3d.c parse_cinespace):
 * *prelut = 3 x *prelut_size floats (channel c at [c * size]; size is 65536) sampled at prelut_min[c] + i / prelut_scale[c],
 * or NULL / 0 when the file has none.  Free *prelut with lutr_cube_free.  Pass it to lutr_ctx_set_prelut after lutr_ctx_set_lut. */
int  lutr_lut_parse_ex(const char *path, float **rgb, int *n, float scale[3], float **prelut, int *prelut_size,
                       float prelut_min[3], float prelut_scale[3]);

/* ---- context ---- */
int  lutr_ctx_create(int device, lutr_ctx **out);
void lutr_ctx_destroy(lutr_ctx *ctx);
/* run on a caller-owned HIP stream (hipStream_t passed as void*); NULL selects HIP's default
 * (null) stream, which is what torch.cuda.current_stream() is unless the caller changed it.
 * Until this is called the context uses a private non-blocking stream.  Launches of one context never
 * overlap: if work issued on the previous stream may still be running, the new stream is made to wait
 * for it (hipStreamWaitEvent) -- the context's work queue and scratch are per context, not per stream. */
int  lutr_ctx_set_stream(lutr_ctx *ctx, void *hip_stream);
int  lutr_ctx_sync(lutr_ctx *ctx);

/* upload a host lattice (layout of lutr_cube_parse); drops a prelut set earlier */
int  lutr_ctx_set_lut(lutr_ctx *ctx, const float *rgb, int n, const float scale[3]);
/* lut3d's prelut for the lattice just set (layout of lutr_lut_parse_ex; size 0 or prelut NULL removes it).  Every sample then goes
 * through FFmpeg's apply_prelut (linear interpolation in the 1D table) before the cube.  With a prelut the calls run on the
 * generic / vector kernels (the LDS tile kernels and the fast precision do not take one). */
int  lutr_ctx_set_prelut(lutr_ctx *ctx, const float *prelut, int size, const float prelut_min[3], const float prelut_scale[3]);
/* the SECOND lattice of lutr_apply_yuv_chain (layout of lutr_cube_parse; finite nodes, like lutr_ctx_set_lut); rgb NULL or n 0
 * removes it.  It lives in a device buffer of its own in the first lattice's layout, (n+1)^3 float4 nodes; it has no prelut.
 * lutr_ctx_set_lut / lutr_ctx_lut_alloc / lutr_lut_broadcast leave it alone, and no other entry point reads it. */
int  lutr_ctx_set_lut2(lutr_ctx *ctx, const float *rgb, int n, const float scale[3]);
/* multi-GPU: a non-root rank allocates the device lattice without filling it, the host
 * broadcasts into the pointer returned by lutr_ctx_lut_device (RCCL, root = the rank that
 * called lutr_ctx_set_lut), then every rank may apply. */
int  lutr_ctx_lut_alloc(lutr_ctx *ctx, int n, const float scale[3]);
int  lutr_ctx_lut_device(lutr_ctx *ctx, void **dptr, size_t *bytes);
/* call after writing the device lattice obtained from lutr_ctx_lut_device (e.g. once the broadcast
 * has landed): checks that every node is finite (LUTR_EINVAL otherwise, like lutr_ctx_set_lut) and
 * records the lattice's value range, which selects clip-free kernels for lattices inside [0, 1].
 * Optional: an unsealed lattice is applied with the general kernels. */
int  lutr_ctx_lut_seal(lutr_ctx *ctx);
/* One process, several GPUs (the reference is one GUI process with a thread pool,
 * src/lut_renderer/task_manager.py:229-235, so it cannot start one rank per GPU): copy the lattice of
 * ctxs[root] into every other context, GPU to GPU over xGMI (hipMemcpyPeerAsync on each receiver's stream;
 * a plain device copy when two contexts share a GPU).  Receivers are allocated as needed and inherit the
 * root's value-range seal.  Asynchronous: each context's later applies are ordered behind its copy.  This
 * is the single-process twin of the RCCL broadcast one-rank-per-GPU hosts do into lutr_ctx_lut_device. */
int  lutr_lut_broadcast(lutr_ctx **ctxs, int nctx, int root);
/* lutr_lut_broadcast with flags.  LUTR_BCAST_FORCE_PEER_COPY: take the cross-device call (hipMemcpyPeerAsync) also between
 * two contexts of ONE GPU (a self-peer copy is legal) -- the test hook that lets a one-GPU box execute what an 8-GPU node
 * runs.  The receiver's copy is recorded on its own event (a later lutr_ctx_set_stream waits for it) and the root waits
 * for outstanding copies before its lattice is overwritten or freed. */
enum { LUTR_BCAST_FORCE_PEER_COPY = 1 };
int  lutr_lut_broadcast_ex(lutr_ctx **ctxs, int nctx, int root, unsigned flags);
/* bytes of the device lattice layout for size n: (n+1)^3 nodes of 16 bytes */
size_t lutr_lattice_bytes(int n);

/* ---- apply (device pointers; asynchronous on the context's stream) ---- */
/* lut3d on planar RGB at `depth` bits (8 -> uint8 planes, 9..16 -> uint16 LE planes),
 * luma rows [row0, row0+rows) of each of nframes frames. */
int lutr_apply_planar_rgb(lutr_ctx *ctx, int depth, int interp, int w, int h, int nframes,
                          const lutr_planes *src, const lutr_planes *dst, int row0, int rows);

/* lut3d on packed RGB (`pfmt` = one of LUTR_PK_* / LUTR_PACKED(...)); M = 255 or 65535.  16-bit
 * formats need 2-byte aligned rows.  src == dst (in place) is allowed. */
int lutr_apply_packed_rgb(lutr_ctx *ctx, int pfmt, int interp, int w, int h, int nframes,
                          const lutr_packed *src, const lutr_packed *dst, int row0, int rows);

/* fused YUV -> RGB -> lut3d -> RGB -> YUV; row0 and rows must be multiples of the
 * chroma block height (2 for 4:2:0) unless row0+rows == h. */
int lutr_apply_yuv(lutr_ctx *ctx, const lutr_yuv_params *p, int interp, int w, int h, int nframes,
                   const lutr_planes *src, const lutr_planes *dst, int row0, int rows);

/* Chroma siting of the resampling around the LUT, named like ffprobe's chroma_location.
 *   REPLICATE: each chroma sample is replicated over its block before the LUT and the block mean is taken after it
 *              (lutr_apply_yuv's contract).
 *   LEFT:      MPEG-2 / H.264 / HEVC default: horizontally co-sited, vertically interstitial.
 *   CENTER:    JPEG / MPEG-1: interstitial on both axes.
 *   TOPLEFT:   HEVC / BT.2020 type 2 (HDR10): co-sited on both axes.
 * "Co-sited": chroma sample k sits on luma sample 2k; "interstitial": halfway between luma samples 2k and 2k+1. */
enum lutr_chroma_loc {
    LUTR_CHROMA_REPLICATE = 0,
    LUTR_CHROMA_LEFT      = 1,
    LUTR_CHROMA_CENTER    = 2,
    LUTR_CHROMA_TOPLEFT   = 3
};

/* lutr_apply_yuv with sited bilinear chroma resampling: before YUV -> RGB each luma pixel takes a weighted sum of the
 * (prologue'd) chroma codes around it, weights in quarters per subsampled axis (co-sited: 4 | 2 2, interstitial: 1 3 | 3 1);
 * after lut3d each chroma sample is a weighted sum of the LUT's RGB output (co-sited axis: taps 2i-1, 2i, 2i+1 weighted
 * 1 2 1; interstitial axis: taps 2i, 2i+1 weighted 1 1).  Every coordinate clamps to its plane.  All sums are exact
 * integers in fp32; the rest is lutr_apply_yuv's arithmetic.  Always strict precision (fast / fma32 run strict here).
 * chroma_loc == LUTR_CHROMA_REPLICATE and 4:4:4 formats are lutr_apply_yuv itself (same kernels, same bits).
 * The up- and down-sampling read source rows and columns around the output region, including rows outside
 * [row0, row0 + rows) of the full frame; only the shard is written.  In-place operation is not supported: the bounding
 * byte range of every source plane (all its rows and frames) must be disjoint from that of every destination plane, else
 * LUTR_EINVAL -- a conservative rule that also refuses planes interleaved row by row in one buffer.  That and an unknown
 * chroma_loc are rejected before anything touches the device.  4:2:0 / 4:2:2 launches with equal input and output widths,
 * a width that is a multiple of 4 and aligned, positive strides run the vector kernel (last kernel "k_yuv_sited_vec<..>"),
 * every other layout the per-sample kernel ("k_yuv_sited<..>"); both compute the same bits. */
int lutr_apply_yuv_sited(lutr_ctx *ctx, const lutr_yuv_params *p, int interp, int chroma_loc, int w, int h, int nframes,
                         const lutr_planes *src, lutr_planes *dst, int row0, int rows);
/* lutr_yuv_constants for lutr_apply_yuv_sited: the same block with the down-sampling's 1/n folded into cbr..crb
 * (n = product of the tap sums of the subsampled axes: 2, 4, 8 or 16; formed in double, rounded once to float) */
int lutr_yuv_constants_sited(const lutr_yuv_params *p, int chroma_loc, float out[32]);

/* ---- output resize (the reference's `-s WxH` after its -vf chain, ffmpeg.py:312-313) ---- */
/* Separable bicubic, B = 0, C = 0.6 (libswscale's SWS_BICUBIC defaults, which the ffmpeg CLI uses for -s; FFmpeg recall, unpinned):
 * k(t) = 1.4|t|^3 - 2.4|t|^2 + 1 (|t| < 1), -0.6|t|^3 + 3|t|^2 - 4.8|t| + 2.4 (1 <= |t| < 2), 0 otherwise.  Per axis, with
 * f = src / dst of the LUMA sizes for every plane and stretch = max(1, f): chroma sample j sits at luma coordinate 2^cs j + o
 * (o = 0 co-sited, (2^cs - 1) / 2 interstitial), is mapped through luma's x -> (x + 0.5) f - 0.5 and back to a source chroma
 * index x; it reads n = 2 ceil(2 stretch) samples floor(x) - n/2 + 1 + k weighted k((x_k - x) / stretch), normalised in double,
 * rounded to Q14 (floor(w 16384 + 0.5)) and the residue added to the largest tap (the first on a tie): every row sums to 16384.
 * Limits per axis: 1/8 <= dst / src <= 16.  Integer arithmetic at output depth d:
 *   t = (sum w s + 2^(d-3)) >> (d-2);  v = sum w t;  out = clamp((v + 2^(29-d)) >> (30-d), 0, 2^d - 1). */

/* Host only (no context, no GPU): the table of one axis of one plane.  src / dst are luma sizes, cs = 0 | 1 the plane's log2
 * subsampling on this axis, cosited = 1 for a co-sited chroma axis (ignored when cs == 0).  *ntaps = n; start (ceil(dst / 2^cs)
 * entries: the first source index, unclamped) and weights (ceil(dst / 2^cs) * n, row-major) are filled when not NULL.
 * LUTR_EINVAL outside the limits. */
int lutr_resize_filter(int src, int dst, int cs, int cosited, int *start, int16_t *weights, int *ntaps);

enum lutr_resize_family { LUTR_RESIZE_YUV = 0, LUTR_RESIZE_GBR = 1 };

/* Resize nframes frames of three planes from sw x sh to dw x dh (luma sizes; chroma planes are ceil(size / 2^cs)) at `depth`
 * (8 -> uint8, 9..16 -> uint16 LE).  family LUTR_RESIZE_YUV: planar 4:2:0 / 4:2:2 / 4:4:4 (csx, csy), chroma siting from
 * chroma_loc per axis as in lutr_apply_yuv_sited (REPLICATE = interstitial on every subsampled axis); LUTR_RESIZE_GBR: gbrp,
 * csx = csy = 0.  Source indices clamp to the plane.  Not in place: the bounding byte range of every source plane must be
 * disjoint from that of every destination plane (the rule of lutr_apply_yuv_sited).  Tables are built on the host once per axis
 * geometry and kept in the context.  Asynchronous on the context's stream; the last kernel is "k_resize<8|16>". */
int lutr_resize_planes(lutr_ctx *ctx, int family, int depth, int csx, int csy, int chroma_loc, int sw, int sh, int dw, int dh,
                       int nframes, const lutr_planes *src, lutr_planes *dst);

/* Host only (no context, no GPU): the launch plan lutr_resize_planes makes for this geometry, by the same function and after the
 * same argument checks (LUTR_EINVAL as there).  out[8] = { th: output rows per tile (64, 32 or 16, the tallest whose LDS stays
 * within 40 KiB with one staged row); rows: staged source rows per wave and step (8 .. 1, the most whose LDS stays within 64 KiB);
 * lds: dynamic LDS bytes of the launch; spx, spy: the largest footprint of a tile over the three planes, source columns (even)
 * and source rows; nx_max, ny_max: the most taps per axis; tiles_per_frame }.  A plan whose lds exceeds 65536 is filled in and
 * refused with LUTR_EINVAL, as lutr_resize_planes refuses the launch. */
int lutr_resize_plan(int family, int depth, int csx, int csy, int chroma_loc, int sw, int sh, int dw, int dh, int *out);

/* zscale_dither of the reference (models.py:46; the filter `zscale=dither=error_diffusion`, ffmpeg.py:305-307) */
enum lutr_dither {
    LUTR_DITHER_NONE = 0,
    LUTR_DITHER_ERROR_DIFFUSION = 1,
    /* An engine setting, not one of the reference's options: a threshold dither with a 64 x 64 void-and-cluster
     * ("blue-noise") mask, fused into the output stage.  Every output sample is q = clip(floor(c + d), 0, max_o): c is the fp32
     * value the output stage floors without dither (its 0.5 included), d = (2 * rank - 4095) / 8192 with rank the mask entry
     * [(y + OY[p]) & 63][(x + OX[p]) & 63], OX = (0, 24, 40), OY = (0, 37, 11) for plane p = Y, Cb, Cr; (x, y) are the sample's
     * coordinates in its own output plane, counted from the top-left of the full frame.  One fp32 add, rounded once.  The same
     * pattern for every frame; no scratch; rows and frames are independent, so row shards and batches give the bits of the whole
     * call.  Always strict arithmetic.  A context's first call in this mode allocates and uploads the 16 KB table of d; later
     * calls only launch. */
    LUTR_DITHER_BLUE_NOISE = 2
};

/* The mask of LUTR_DITHER_BLUE_NOISE: 4096 ranks, a permutation of 0 .. 4095, row-major [y][x].  Host only, no context, no GPU.
 * LUTR_EINVAL for a null pointer. */
int lutr_dither_mask(uint16_t out[4096]);

/* lutr_apply_yuv with the final quantisation dithered: Floyd-Steinberg error diffusion per output plane
 * (rows top to bottom, left to right).  Rows are coupled, so this takes whole frames only;
 * shard a batch over GPUs by frames.  dither == LUTR_DITHER_NONE is lutr_apply_yuv on rows [0, h).
 * Uses context-owned device scratch of 4 bytes per output sample of the batch.
 * dither == LUTR_DITHER_BLUE_NOISE is lutr_apply_yuv_xsub's blue-noise call on rows [0, h): same kernels, no scratch. */
int lutr_apply_yuv_dither(lutr_ctx *ctx, const lutr_yuv_params *p, int interp, int dither, int w, int h, int nframes,
                          const lutr_planes *src, const lutr_planes *dst);

/* ---- chroma subsampling change (the reference's format=<pix_fmt> with another layout, ffmpeg.py:304-310) ---- */
/* lutr_apply_yuv with fmt_in and fmt_out in any two of 4:2:0, 4:2:2 and 4:4:4 (4:4:0 is LUTR_EINVAL on either side), at any
 * depth pair in 8..16.  Each source chroma sample is replicated over its INPUT block (sample x >> icsx, y >> icsy); each output
 * chroma sample is the mean of the LUT's integer RGB over its OUTPUT block, the 1/n (n = 2^(ocsx + ocsy)) folded into cbr..crb
 * (lutr_yuv_constants_xsub).  A partial output block at an odd edge takes the edge column / row again.  Everything else --
 * prologue, matrices, ranges, LUT depth, truncation -- is lutr_apply_yuv's arithmetic.
 * row0 and rows must be multiples of the union block height 2^max(icsy, ocsy) unless row0 + rows == h.
 * dither: LUTR_DITHER_NONE, or LUTR_DITHER_ERROR_DIFFUSION on whole frames only (row0 = 0, rows = h; the scratch of
 * lutr_apply_yuv_dither, sized by the output layout), or LUTR_DITHER_BLUE_NOISE on any row range the block rule allows.
 * Equal layouts are lutr_apply_yuv (or lutr_apply_yuv_dither for error diffusion) itself: same kernels, bits and last kernel.
 * LUTR_DITHER_BLUE_NOISE does not forward: all nine layout pairs, the equal ones included, run "k_yuv_bn_vec<win,wout,icsx,
 * icsy,ocsx,ocsy,interp>" under k_yuv_xsub_vec's conditions and "k_yuv_bn_generic" for everything else (any depth pair, 8 -> 16
 * bit, all five modes), a ragged width split between the two; strict arithmetic, a .csp prelut taken; variants as below.
 * A layout change always runs strict precision (fast / fma32 run strict here, no suffix on the last kernel) and takes a
 * .csp prelut.  Kernels: "k_yuv_xsub_vec<win,wout,icsx,icsy,ocsx,ocsy,interp>" (nearest / trilinear / tetrahedral; 8 -> 8,
 * 16 -> 16 and 16 -> 8 bit containers; width a multiple of 8 luma samples, 4 for 16 -> 16; positive strides aligned to
 * the accesses; row0 / rows multiples of the union block height), "k_yuv_xsub_generic" for everything else; a ragged
 * width on aligned rows is split between the two; dithering runs "k_yuv_float+k_dither_ed".  Variants: auto and generic
 * as for lutr_apply_yuv; vec_global fails with LUTR_EINVAL where the vector kernel cannot take the layout; vec_lds always
 * fails with LUTR_EINVAL on a layout change (there is no LDS-window kernel for it). */
int lutr_apply_yuv_xsub(lutr_ctx *ctx, const lutr_yuv_params *p, int interp, int dither, int w, int h, int nframes,
                        const lutr_planes *src, const lutr_planes *dst, int row0, int rows);
/* lutr_yuv_constants for lutr_apply_yuv_xsub: the down-sampling's n is the OUTPUT block's size.  Same bits as
 * lutr_yuv_constants when fmt_in and fmt_out share the layout.  Host only. */
int lutr_yuv_constants_xsub(const lutr_yuv_params *p, float out[32]);

/* ---- RGB sources with a YUV output (the reference's chain on a PNG / TIFF / DPX sequence or an RGB screen
 *      recording: lut3d directly on the RGB frame, then format=<pix_fmt>, ffmpeg.py:246 and :304-310) ---- */
/* `interp` value of lutr_apply_rgb_to_yuv that leaves lut3d out: the source codes go straight to the RGB -> YUV stage
 * (the range-normalising stage ahead of lut3d that the reference puts in front of full-range sources, ffmpeg.py:212-233). */
#define LUTR_INTERP_NONE (-1)
/* Integer RGB at depth p->lut_depth -> lut3d at that depth (lutr_apply_planar_rgb / lutr_apply_packed_rgb's arithmetic, every
 * interpolation mode, a .csp prelut taken) -> planar YUV p->fmt_out (4:2:0 / 4:2:2 / 4:4:4 at any depth in 8..16; 4:4:0 is
 * LUTR_EINVAL) through the output stage of lutr_apply_yuv: Y per pixel, each chroma sample from the sum of the LUT's integer RGB
 * over its OUTPUT block, 1/n (n = 2^(ocsx + ocsy)) folded into cbr..crb (lutr_yuv_constants_rgb2yuv); a partial block at an odd
 * edge takes the edge column / row again.  Of *p only fmt_out, lut_depth, matrix_out and range_out are read.
 * src_kind == 0: planar gbrp in src_planar (plane 0 = G, 1 = B, 2 = R; uint8 for lut_depth 8, else uint16 LE), src_packed unused.
 * src_kind == LUTR_PK_* / LUTR_PACKED(...): one packed image in src_packed, src_planar unused; lut_depth must be the format's
 *   bits (8 | 16); a fourth component (alpha / padding) is read past and dropped.  16-bit formats need 2-byte aligned rows.
 * row0 and rows must be multiples of the output chroma block height 2^ocsy unless row0 + rows == h.
 * dither: LUTR_DITHER_NONE, or LUTR_DITHER_ERROR_DIFFUSION on whole frames only (the scratch of lutr_apply_yuv_dither, sized by
 * the output layout), or LUTR_DITHER_BLUE_NOISE on any row range the block rule allows: "k_rgb2yuv_bn_generic" (no vector kernel
 * yet: vec_global and vec_lds fail with LUTR_EINVAL).  Always strict precision (fast / fma32 run strict here, no suffix on the
 * last kernel).
 * Not in place: the bounding byte range of every source plane / the source image (all rows and frames) must be disjoint from
 * that of every destination plane (the rule of lutr_apply_yuv_sited), else LUTR_EINVAL before anything touches the device.
 * Kernels: "k_rgb2yuv_vec<win,nc,wout,ocsx,ocsy,interp|nolut>" (nc = 1 planar, 3 | 4 packed components; nearest / trilinear /
 * tetrahedral / no LUT; 8 -> 8, 16 -> 16 and 16 -> 8 bit containers; width a multiple of 8; positive strides; planar source
 * planes aligned to 8 samples, a packed image to 4 bytes, destination planes to the 8 (chroma: 8 >> ocsx) samples a thread
 * stores; 3-component sources in R G B or B G R order; row0 / rows multiples of 2^ocsy), "k_rgb2yuv_generic" for everything
 * else; a ragged width on aligned rows is split between the two; dithering runs "k_rgb2yuv_float+k_dither_ed".  Variants: auto
 * and generic as for lutr_apply_yuv; vec_global fails with LUTR_EINVAL where the vector kernel cannot take the layout; vec_lds
 * always fails with LUTR_EINVAL (there is no LDS kernel for this path).
 * Not covered: chroma siting, a tile (LDS) kernel.  (YUV in with RGB out is lutr_apply_yuv_to_rgb.) */
int lutr_apply_rgb_to_yuv(lutr_ctx *ctx, const lutr_yuv_params *p, int interp, int dither, int src_kind, int w, int h, int nframes,
                          const lutr_planes *src_planar, const lutr_packed *src_packed, const lutr_planes *dst, int row0, int rows);
/* The constant block lutr_apply_rgb_to_yuv uses.  Its output-stage entries (cyr..crb, yob, cob, max_o) equal, bit for bit, those
 * of lutr_yuv_constants_xsub for a 4:4:4 source at depth lut_depth with the same output side; the input-stage entries are not
 * read by the kernels (they are filled from matrix_out / range_out).  Host only. */
int lutr_yuv_constants_rgb2yuv(const lutr_yuv_params *p, float out[32]);

/* ---- YUV sources with an RGB output (ffmpeg's lut3d=...,format=<rgb fmt> on a camera file: a DPX / TIFF / PNG
 *      sequence, a review still, a GUI preview) ---- */
/* Planar YUV p->fmt_in (4:2:0 / 4:2:2 / 4:4:4 at any depth din in 8..16; 4:4:0 is LUTR_EINVAL) -> each chroma sample replicated
 * over its INPUT block (x >> icsx, y >> icsy), as lutr_apply_yuv_xsub -> integer RGB at p->lut_depth through matrix_in (the
 * input stage of lutr_apply_yuv) -> lut3d at that depth (every interpolation mode, a .csp prelut taken; LUTR_INTERP_NONE leaves
 * it out) -> stored as it is.  The LUT runs at the DESTINATION's depth, where ffmpeg's format negotiation puts lut3d when
 * format=<rgb fmt> follows it; there is no depth change behind the LUT.  Of *p only fmt_in, lut_depth, matrix_in, range_src and
 * range_in are read.
 * dst_kind == 0: planar gbrp in dst_planar (plane 0 = G, 1 = B, 2 = R; uint8 for lut_depth 8, else uint16 LE), dst_packed unused.
 * dst_kind == LUTR_PK_* / LUTR_PACKED(...): one packed image in dst_packed, dst_planar unused; lut_depth must be the format's
 *   bits (8 | 16), else LUTR_EINVAL; the fourth component of a 4-component format is written 2^lut_depth - 1 (opaque).  16-bit
 *   formats need 2-byte aligned rows.
 * Depth: with range_src == range_in a source depth other than lut_depth is NOT a prologue here (so a tv source may change depth):
 *   the change is folded into the input-stage constants (lutr_yuv_constants_yuv2rgb).  With range_src != range_in the prologue of
 *   lutr_apply_yuv runs, on its terms (a pc source only), and lands at (lut_depth, range_in).
 * row0 and rows must be multiples of the input chroma block height 2^icsy unless row0 + rows == h.
 * Always strict precision (fast / fma32 run strict here, no suffix on the last kernel).
 * Not in place: the bounding byte range of every source plane (all rows and frames) must be disjoint from that of every
 * destination plane / the destination image (the rule of lutr_apply_yuv_sited), else LUTR_EINVAL before anything touches the device.
 * Kernels: "k_yuv2rgb_vec<win,icsx,icsy,nc,wout,interp|nolut>" (nc = 1 planar, 3 | 4 packed components; nearest / trilinear /
 * tetrahedral / no LUT; 8 -> 8, 16 -> 16 and 16 -> 8 bit containers; width a multiple of 8; positive strides; source planes
 * aligned to the 8 (chroma: 8 >> icsx) samples a thread loads, planar destination planes to 8 samples, a packed image to 4 bytes;
 * 3-component destinations in R G B or B G R order; row0 / rows multiples of 2^icsy), "k_yuv2rgb_generic" for everything else; a
 * ragged width on aligned rows is split between the two.  Variants: auto and generic as for lutr_apply_yuv; vec_global fails with
 * LUTR_EINVAL where the vector kernel cannot take the layout; vec_lds always fails with LUTR_EINVAL (there is no LDS kernel for
 * this path).
 * Not covered: chroma siting, dither, a resize, a float destination, alpha carried into a packed destination, a tile (LDS) kernel. */
int lutr_apply_yuv_to_rgb(lutr_ctx *ctx, const lutr_yuv_params *p, int interp, int dst_kind, int w, int h, int nframes,
                          const lutr_planes *src, const lutr_planes *dst_planar, const lutr_packed *dst_packed, int row0, int rows);
/* The constant block lutr_apply_yuv_to_rgb uses.  With range_src == range_in, for s = 2^(din - 8), Mi = 2^din - 1,
 * Ml = 2^lut_depth - 1 (formed in double, each entry rounded once):
 *   tv: ky = Ml / (219 s), yoff = 16 s, kc = Ml / (224 s)      pc: ky = Ml / Mi, yoff = 0, kc = Ml / Mi
 *   yb = -ky yoff + 0.5, coff = 128 s, krv = 2 (1 - kr) kc, kbu = 2 (1 - kb) kc, kgu = -2 kb (1 - kb) / kg kc,
 *   kgv = -2 kr (1 - kr) / kg kc, max_l = Ml, pre = 0
 * -- for din == lut_depth the input-stage entries of lutr_yuv_constants bit for bit; legal black gives code 0 and legal white Ml
 * for every depth pair.  With range_src != range_in it is the block of lutr_yuv_constants for an output at (lut_depth, 4:4:4,
 * matrix_in, range_in).  The output-stage entries are not read by the kernels.  Host only. */
int lutr_yuv_constants_yuv2rgb(const lutr_yuv_params *p, float out[32]);

/* ---- planar float RGB sources, gbrpf32le (what ffmpeg decodes an OpenEXR sequence to: lut3d's planar-float
 *      path on the frame itself, then format=<pix_fmt>, ffmpeg.py:246 and :304-310) ---- */
/* lut3d on planar float RGB, float in and float out.  src / dst: three planes of 32-bit floats in gbrp order (plane 0 = G,
 * 1 = B, 2 = R); strides in bytes; base pointers, strides and (batches) frame strides must be multiples of 4, else LUTR_EINVAL.
 * Per pixel and channel: the input is sanitised by its bit pattern (NaN -> 0, +inf -> FLT_MAX, -inf -> -FLT_MAX, vf_lut3d.c's
 * sanitizef); a .csp prelut is interpolated PER PIXEL on the table lutr_ctx_set_prelut was given (prelut_interp_1d_linear:
 * t = clip((x - min) * scale, 0, size - 1), lerp of tab[(int)t] and its neighbour); s = clip(x * (scale * (n - 1)), 0, n - 1);
 * interp<mode> (all five modes); the three floats are stored as they are: no clip, no scaling -- values outside [0, 1] survive.
 * Always strict precision (fast / fma32 run strict here, no suffix on the last kernel).  src == dst (in place) is allowed.
 * Kernels: "k_rgbf_vec<interp>" (nearest / trilinear / tetrahedral; width a multiple of 4; positive strides; planes, strides and
 * frame strides 16-byte aligned), "k_rgbf_generic" for everything else; a ragged width on aligned rows is split between the
 * two.  Variants: auto and generic as for lutr_apply_yuv; vec_global fails with LUTR_EINVAL where the vector kernel cannot take
 * the layout; vec_lds always fails with LUTR_EINVAL (there is no LDS kernel for this path). */
int lutr_apply_planar_rgb_f32(lutr_ctx *ctx, int interp, int w, int h, int nframes, const lutr_planes *src, const lutr_planes *dst,
                              int row0, int rows);
/* Planar float RGB (src as for lutr_apply_planar_rgb_f32) -> lut3d as above -> each channel quantised to a 16-bit code,
 * q = clip(rintf(v * 65535), 0, 65535) with round-half-to-even -> planar YUV p->fmt_out through the output stage of
 * lutr_apply_rgb_to_yuv at lut_depth 16 (constants: lutr_yuv_constants_rgb2yuv; chroma from the block sum of q; a partial block
 * takes the edge again; 4:4:0 is LUTR_EINVAL).  Reads of *p what lutr_apply_rgb_to_yuv reads; p->lut_depth must be 16, else
 * LUTR_EINVAL.  interp == LUTR_INTERP_NONE leaves lut3d out: sanitise, quantise, convert.
 * row0 and rows must be multiples of the output chroma block height 2^ocsy unless row0 + rows == h.
 * dither: LUTR_DITHER_NONE, or LUTR_DITHER_ERROR_DIFFUSION on whole frames only (the scratch of lutr_apply_yuv_dither), or
 * LUTR_DITHER_BLUE_NOISE on any row range the block rule allows: "k_rgbf2yuv_bn_generic" (no vector kernel yet: vec_global and
 * vec_lds fail with LUTR_EINVAL).
 * Always strict precision.  Not in place: the byte-range rule of lutr_apply_rgb_to_yuv, checked before anything touches the device.
 * Kernels: "k_rgbf2yuv_vec<wout,ocsx,ocsy,interp|nolut>" (nearest / trilinear / tetrahedral / no LUT; width a multiple of 8;
 * positive strides; source planes 16-byte aligned, destination planes to the 8 (chroma: 8 >> ocsx) samples a thread stores;
 * row0 / rows multiples of 2^ocsy), "k_rgbf2yuv_generic" for everything else; a ragged width on aligned rows is split between
 * the two; dithering runs "k_rgbf2yuv_float+k_dither_ed".  Variants as for lutr_apply_planar_rgb_f32. */
int lutr_apply_rgbf_to_yuv(lutr_ctx *ctx, const lutr_yuv_params *p, int interp, int dither, int w, int h, int nframes,
                           const lutr_planes *src, const lutr_planes *dst, int row0, int rows);

/* ---- semi-planar YUV frames: nv12 / nv21 / nv16 and p010le / p012le / p016le / p210le / p212le / p216le, what
 *      hardware decoders write and hardware encoders read -- the frame the reference's chain (ffmpeg.py:246, :304-310) sees after
 *      FFmpeg's scaler has unpacked it ---- */
/* The container of one side of lutr_apply_yuv_semi.
 *   semi  = 0: three planes, as lutr_apply_yuv takes them.
 *   semi  = 1: data[0] is luma; data[1] holds ceil(w / 2) pairs of chroma samples per row, ceil(h / 2) rows for 4:2:0 and h
 *              rows for 4:2:2, with stride[1] / frame_stride[1] in bytes; data[2] is ignored and may be NULL.
 *   swap  = 1: Cr comes first in a pair (nv21).  Only with semi = 1.
 *   shift    : left shift of the code inside its 16-bit word, 16 - depth (p010le: 6) or 0; always 0 for an 8-bit container.
 *              On input the code is word >> shift whatever the low bits hold; on output the low bits are zero. */
typedef struct lutr_yuv_layout {
    int32_t semi;
    int32_t swap;
    int32_t shift;
} lutr_yuv_layout;

/* lutr_apply_yuv on frames whose source side, destination side or both are semi-planar; each side's container is its own.  The
 * result is bit-identical to lutr_apply_yuv on the same samples held in three planes: everything *p expresses (depth change,
 * the full-range prologue, matrices, ranges, lut_depth) and a .csp prelut are that call's arithmetic unchanged.
 * fmt_in and fmt_out must have the same chroma subsampling, 4:2:0 or 4:2:2 when a side is semi-planar.  Row blocks follow the
 * rule of lutr_apply_yuv.  When both layouts are planar with shift 0 this IS lutr_apply_yuv: same kernels, bits, last kernel.
 * src == dst plane for plane (in place) is allowed when both sides have the same format; nothing else about overlap is checked.
 * Always strict precision otherwise (fast / fma32 run strict here, no suffix on the last kernel).
 * LUTR_EINVAL with a message, before anything touches the device: a shift other than 16 - depth or 0 on a 16-bit container, a
 * non-zero shift on an 8-bit one, swap without semi, semi / swap outside 0 | 1, a semi-planar side that is 4:4:4, a null pointer
 * where a plane is needed, 16-bit planes whose base, stride or (batches) frame stride is odd.
 * Kernels: "k_yuv_semi_vec<win,wout,semi_in,semi_out,csx,csy,interp>" (nearest / trilinear / tetrahedral; 8 -> 8, 16 -> 16 and
 * 16 -> 8 bit containers; at least one side semi-planar; width a multiple of 8 luma samples, 4 for 16 -> 16; positive strides
 * aligned to the accesses -- a plane of pairs moves twice the bytes of a planar chroma plane per access; row0 / rows multiples
 * of the chroma block height), "k_yuv_semi_generic" for everything else (one thread per chroma block; any depth 8..16, stride,
 * alignment or size; all five modes); a ragged width on aligned rows is split between the two.  Variants: auto and generic as
 * for lutr_apply_yuv; vec_global fails with LUTR_EINVAL where the vector kernel cannot take the layout; vec_lds always fails
 * with LUTR_EINVAL (there is no LDS kernel for this path).
 * Not covered: a subsampling change, chroma siting, dither, 4:4:4 semi-planar (nv24, p410le), big-endian containers. */
int lutr_apply_yuv_semi(lutr_ctx *ctx, const lutr_yuv_params *p, int interp, const lutr_yuv_layout *in_layout,
                        const lutr_yuv_layout *out_layout, int w, int h, int nframes, const lutr_planes *src,
                        const lutr_planes *dst, int row0, int rows);

/* ---- packed 4:2:2 YUV frames: yuyv422 / uyvy422 / yvyu422 and y210le / y212le / y216le, what capture cards,
 *      V4L2 devices and 4:2:2 hardware decoders write -- the frame the reference's chain (ffmpeg.py:246, :304-310) sees after
 *      FFmpeg's scaler has unpacked it to yuv422p* ---- */
#define LUTR_PK_YUYV 0   /* Y0 Cb Y1 Cr: yuyv422, y210le, y212le, y216le */
#define LUTR_PK_UYVY 1   /* Cb Y0 Cr Y1: uyvy422 */
#define LUTR_PK_YVYU 2   /* Y0 Cr Y1 Cb: yvyu422 */
/* The container of one side of lutr_apply_yuv_packed.
 *   packed = 0: three planes, as lutr_apply_yuv takes them; order and shift must be 0.
 *   packed = 1: data[0] holds ceil(w / 2) groups of four samples per row (two luma, one Cb / Cr pair), h rows, with stride[0] /
 *               frame_stride[0] in bytes; data[1] and data[2] are ignored and may be NULL.
 *   order     : LUTR_PK_YUYV | LUTR_PK_UYVY | LUTR_PK_YVYU, the samples of a group in memory order.
 *   shift     : left shift of the code inside its 16-bit word, 16 - depth (y210le: 6) or 0; always 0 for an 8-bit container.
 *               On input the code is word >> shift whatever the low bits hold; on output the low bits are zero.
 * Odd width: the second luma sample of the last group is ignored on input and written as a copy of the last real luma sample
 * on output; chroma follows the edge rule of lutr_apply_yuv (the edge column counts twice in the block mean). */
typedef struct lutr_yuv_packing {
    int32_t packed;
    int32_t order;
    int32_t shift;
} lutr_yuv_packing;

/* lutr_apply_yuv on frames whose source side, destination side or both are packed 4:2:2; each side's container is its own.
 * A packed side's format (fmt_in / fmt_out of *p) is 4:2:2.  With 4:2:2 on both sides the result is bit-identical to
 * lutr_apply_yuv on the same samples held in yuv422p* planes: everything *p expresses (depth change, the full-range prologue,
 * matrices, ranges, lut_depth) and a .csp prelut are that call's arithmetic unchanged.  A packed source may also go to a PLANAR
 * 4:2:0 or 4:4:4 destination: bit-identical to lutr_apply_yuv_xsub on the de-interleaved source.  Row blocks follow the rule of
 * those calls (row0 / rows multiples of the destination's chroma block height).  When both sides are planar this IS
 * lutr_apply_yuv / lutr_apply_yuv_xsub: same kernels, bits, last kernel.
 * src == dst (in place) is allowed when both sides are the same packed container with the same strides; any other overlap of
 * the source's and the destination's byte ranges fails.  Always strict precision (fast / fma32 run strict here, no suffix on
 * the last kernel).
 * LUTR_EINVAL with a message, before anything touches the device: packed outside 0 | 1, order outside 0..2, order or shift on a
 * planar side, a shift other than 16 - depth or 0 on a 16-bit container, a non-zero shift on an 8-bit one, a packed side whose
 * format is not 4:2:2, a packed destination whose fmt_in is not 4:2:2, a null pointer where a plane is needed, 16-bit containers
 * whose base, stride or (batches) frame stride is odd, source and destination overlapping other than in place.
 * Kernels: "k_yuv_pk_vec<win,wout,packed_in,packed_out,ocsy,interp>" (nearest / trilinear / tetrahedral; 8 -> 8, 16 -> 16 and
 * 16 -> 8 bit containers; a 4:2:2 or planar 4:2:0 destination; width a multiple of 8 luma samples, 4 for 16 -> 16; positive
 * strides; packed rows 16-byte aligned, planar rows aligned to k_yuv_vec's words; row0 / rows multiples of the destination's
 * chroma block height), "k_yuv_pk_generic" for everything else (one thread per group; any depth 8..16, stride, alignment or
 * size; all five modes; the planar 4:4:4 destination); a ragged width on aligned rows is split between the two.  Variants: auto
 * and generic as for lutr_apply_yuv; vec_global fails with LUTR_EINVAL where the vector kernel cannot take the layout; vec_lds
 * always fails with LUTR_EINVAL (there is no LDS kernel for this path).
 * Not covered: a semi-planar side, a packed destination with a subsampling change, chroma siting, dither, resize, an RGB
 * source, packed 4:4:4 (vuyx, xv30le, ayuv64le), big-endian containers. */
int lutr_apply_yuv_packed(lutr_ctx *ctx, const lutr_yuv_params *p, int interp, const lutr_yuv_packing *in,
                          const lutr_yuv_packing *out, int w, int h, int nframes, const lutr_planes *src,
                          const lutr_planes *dst, int row0, int rows);

/* ---- v210 frames: the 10-bit 4:2:2 container of SDI capture and play-out cards and of QuickTime / AVI files
 *      with FourCC 'v210' -- the frame the reference's chain sees after FFmpeg's v210 decoder has unpacked it to yuv422p10le ---- */
/* lutr_apply_yuv on frames whose source side (in_v210 = 1), destination side (out_v210 = 1) or both are v210; the other side is
 * three planes as lutr_apply_yuv takes them.  Both flags 0 is LUTR_EINVAL (that is lutr_apply_yuv / lutr_apply_yuv_xsub).
 * A v210 side uses data[0] / stride[0] / frame_stride[0] only (data[1], data[2] are ignored and may be NULL) and its format
 * (fmt_in / fmt_out of *p) is LUTR_FMT(10, 1, 0).  A row is ceil(w / 6) groups of four little-endian 32-bit words; a word holds
 * three 10-bit codes, slot a in bits 0-9, b in bits 10-19, c in bits 20-29:
 *      word 0: Cb0 Y0 Cr0    word 1: Y1 Cb1 Y2    word 2: Cr1 Y3 Cb2    word 3: Y4 Cr2 Y5
 * pair k (Cbk, Crk) belongs to luma samples 2k and 2k + 1 of the group.  The usual row stride is 128 * ceil(w / 48) bytes; any
 * stride that is a multiple of 4 and at least 16 * ceil(w / 6) in magnitude is taken.
 * Input: a code is its 10 bits whatever bits 30-31 hold; slots of samples beyond the frame (luma x >= w, pair k >= ceil(w / 2))
 * are ignored.  Output: bits 30-31 are zero; a luma slot beyond the frame repeats the last real luma sample of the row, a pair
 * beyond it the last real pair; bytes of a row past its last group are never written.  Odd w: chroma follows the edge rule of
 * lutr_apply_yuv (the edge column counts twice in the block mean).
 * With 4:2:2 on both sides the result is bit-identical to lutr_apply_yuv on the same codes held in yuv422p10le planes: everything
 * *p expresses (depth change, the full-range prologue, matrices, ranges, lut_depth) and a .csp prelut are that call's arithmetic
 * unchanged.  A v210 source may also go to a PLANAR 4:2:0 or 4:4:4 destination: bit-identical to lutr_apply_yuv_xsub on the
 * unpacked source.  Row blocks follow the rule of those calls (row0 / rows multiples of the destination's chroma block height).
 * src == dst (in place) is allowed when both sides are v210 with the same strides; any other overlap of the source's and the
 * destination's byte ranges fails.  Always strict precision (fast / fma32 run strict here, no suffix on the last kernel).
 * LUTR_EINVAL with a message, before anything touches the device: a flag outside 0 | 1, both flags 0, a v210 side whose format
 * is not 10-bit 4:2:2, a v210 destination whose fmt_in is not 4:2:2, a v210 stride below 16 * ceil(w / 6) or not a multiple of
 * 4, a v210 base that is not 4-byte aligned, a null pointer where a plane is needed, 16-bit planes whose base or stride is odd,
 * overlap other than in place, row0 / rows off the chroma block.
 * Kernels: "k_yuv_v210_vec<planar_wide,v210_in,v210_out,ocsy,interp>" (nearest / trilinear / tetrahedral; v210 -> v210, v210 ->
 * planar 16 or 8 bit 4:2:2 / 4:2:0, planar 16 bit -> v210; 6, 12 (16-bit planes) or 24 (8-bit planes) luma samples per thread;
 * v210 rows 16-byte aligned with positive strides, planar rows 4-byte aligned), "k_yuv_v210_generic" for everything else (one
 * thread per group of six luma samples; any stride, planar depth 8..16 or alignment, any size; all five modes; the planar 4:4:4
 * destination; an 8-bit planar source); a width that is not a whole number of units is split between the two.  Variants: auto
 * and generic as for lutr_apply_yuv; vec_global fails with LUTR_EINVAL where the vector kernel cannot take the layout; vec_lds
 * always fails with LUTR_EINVAL (there is no LDS kernel for this path).
 * Not covered: a semi-planar or packed 4:2:2 side, a subsampling change into v210, chroma siting, dither, resize, the two-output
 * pass, an RGB source, v210x / v410 / r210, big-endian variants. */
int lutr_apply_yuv_v210(lutr_ctx *ctx, const lutr_yuv_params *p, int interp, int in_v210, int out_v210, int w, int h,
                        int nframes, const lutr_planes *src, const lutr_planes *dst, int row0, int rows);

/* ---- two outputs from one pass (the reference's "pro" mode, ffmpeg.py:417-472: a ProRes 422 HQ master with the
 *      LUT in yuv422p10le, then the delivery file in the user's pix_fmt -- both from the same lut3d result) ---- */
/* lutr_apply_yuv_xsub with a second destination: planar YUV in, TWO planar YUV frames out.  fmt_out2 (a LUTR_FMT code) may differ
 * from p->fmt_out in depth (8..16) and chroma subsampling (4:2:0 / 4:2:2 / 4:4:4); both outputs share matrix_out and range_out.
 * dst is bit-identical to what lutr_apply_yuv_xsub(ctx, p, ...) writes (lutr_apply_yuv when fmt_in and fmt_out share the layout),
 * dst2 to the same call with fmt_out2 in place of fmt_out: everything *p expresses on the input side (the full-range prologue,
 * matrices, ranges, lut_depth), a .csp prelut and all five interpolation modes are that call's arithmetic unchanged.  The source
 * is read once and lut3d evaluated once per pixel; the output stage runs twice.  Chroma is replicated over its INPUT block; each
 * output's chroma sample is the mean of the LUT's integer RGB over that output's OWN block (constants: the output-stage entries
 * of lutr_yuv_constants_xsub for fmt_out and for fmt_out2); a partial block at an odd edge takes the edge column / row again.
 * row0 and rows must be multiples of the union block height 2^max(icsy, csy of fmt_out, csy of fmt_out2) unless row0 + rows == h.
 * Always strict precision (fast / fma32 run strict here, no suffix on the last kernel).
 * Not in place: the bounding byte ranges (all rows and frames) of the source planes, of dst's planes and of dst2's planes must
 * all be disjoint from one another (the rule of lutr_apply_yuv_sited).
 * LUTR_EINVAL with a message, before anything touches the device: a bad fmt_out2 (depth outside 8..16, 4:4:0), a null pointer
 * where a plane is needed, 16-bit planes whose base, stride or (batches) frame stride is odd, row0 / rows off the union block,
 * any overlap, variant vec_lds (there is no LDS kernel for this path).  Variant vec_global where the vector kernel cannot take
 * the call is LUTR_EINVAL too, found where the kernel is chosen, as in the sibling entry points: the device is selected and a
 * .csp prelut's table may have been uploaded by then, no kernel has run and nothing is written.
 * Kernels: "k_yuv_dual_vec<win,wa,wb,icsx,icsy,bcsx,bcsy,interp>" (nearest / trilinear / tetrahedral; output A is the 4:2:2 one
 * -- dst2 when only it is 4:2:2 -- and B the other, in the container mixes 16 -> 16+16, 16 -> 16+8 and 8 -> 8+8 bit; width a
 * multiple of 8 luma samples, 4 for 16 -> 16+16; positive strides aligned to the accesses; row0 / rows multiples of the union
 * block height), "k_yuv_dual_generic" for everything else (one thread per union block; any depth 8..16, stride, alignment or
 * size; all five modes; an 8-bit source with a 16-bit output; two outputs of which neither is 4:2:2); a ragged width on aligned
 * rows is split between the two.  Variants: auto and generic as for lutr_apply_yuv.
 * Not covered: dither, chroma siting or a resize on either output, semi-planar / packed / RGB / float sides, different matrices
 * or ranges per output, more than two outputs, a tile (LDS) kernel. */
int lutr_apply_yuv_dual(lutr_ctx *ctx, const lutr_yuv_params *p, int fmt_out2, int interp, int w, int h, int nframes,
                        const lutr_planes *src, const lutr_planes *dst, const lutr_planes *dst2, int row0, int rows);

/* Two lut3d stages in one pass: `lut3d=file=A:interp=ia,lut3d=file=B:interp=ib,format=<pix_fmt>`, a technical
 * LUT followed by a creative look.  Both lut3d instances negotiate the same RGB format, so the frame stays integer RGB at
 * p->lut_depth between them.  Planar YUV in, planar YUV out, any of 4:2:0 / 4:2:2 / 4:4:4 at 8..16 bit on either side:
 *   q0 = YUV -> integer RGB (lutr_apply_yuv's stage 1, the full-range prologue included; chroma replicated over its INPUT block)
 *   q1 = lut3d of the context's first lattice on q0: `interp`, its scale, its .csp prelut if set; clip((int)(v * M), 0, M)
 *   q2 = lut3d of the second lattice (lutr_ctx_set_lut2) on q1: `interp2`, its own n and scale; the codes q1 enter it exactly as
 *        source codes enter the first
 *   out = integer RGB -> YUV from q2 (lutr_apply_yuv_xsub's stage 3: chroma = the mean over its OUTPUT block, a partial block at
 *        an odd edge takes the edge column / row again; constants: lutr_yuv_constants_xsub)
 * row0 and rows must be multiples of the union block height 2^max(icsy, ocsy) unless row0 + rows == h.
 * Always strict precision (fast / fma32 run strict here, no suffix on the last kernel).
 * Not in place: the bounding byte ranges (all rows and frames) of the source planes and of the destination planes must be
 * disjoint (the rule of lutr_apply_yuv_sited).
 * LUTR_EINVAL with a message, before anything touches the device: no first or no second lattice, the format errors of
 * lutr_apply_yuv_xsub (4:4:0, a depth outside 8..16), a null plane, 16-bit planes whose base, stride or (batches) frame stride is
 * odd, row0 / rows off the union block, any overlap, variant vec_lds (there is no LDS kernel for this path).  Variant vec_global
 * where the vector kernel cannot take the call is LUTR_EINVAL too, found where the kernel is chosen, as in the sibling entry
 * points: no kernel has run and nothing is written.
 * Kernels: "k_yuv_chain_vec<win,wout,icsx,icsy,ocsx,ocsy,interp>" (interp == interp2, nearest / trilinear / tetrahedral; the
 * container mixes 8 -> 8, 16 -> 16 and 16 -> 8 bit; width a multiple of 8 luma samples, 4 for 16 -> 16; positive strides aligned to
 * the accesses; row0 / rows multiples of the union block height), "k_yuv_chain_generic" for everything else (one thread per union
 * block; any depth, stride, alignment or size; all five modes and any pair of them; an 8-bit source with a 16-bit output); a
 * ragged width on aligned rows is split between the two and named "<vector kernel>+k_yuv_chain_generic".
 * Not covered: a prelut on the second LUT, more than two LUTs, RGB / float / alpha / semi-planar / packed / v210 sides, dither,
 * chroma siting, a resize, the two-output pass, a tile (LDS) kernel. */
int lutr_apply_yuv_chain(lutr_ctx *ctx, const lutr_yuv_params *p, int interp, int interp2, int w, int h, int nframes,
                         const lutr_planes *src, const lutr_planes *dst, int row0, int rows);

/* ---- ASC CDL in front of lut3d: the per-clip colour decision (slope, offset, power, saturation; ASC CDL v1.2,
 *      the numbers of a .cc / .ccc / .cdl file) on the log image ahead of the shared show LUT, in one pass.  An engine setting:
 *      ffmpeg has no CDL filter. ---- */
typedef struct lutr_cdl {
    float slope[3], offset[3], power[3];   /* R, G, B; identity 1, 0, 1 */
    float saturation;                      /* identity 1 */
} lutr_cdl;

/* Host only, no context and no device: stage A of lutr_apply_yuv_cdl for one channel (0 = R, 1 = G, 2 = B) at `depth` bits
 * (8..16), 2^depth floats into `out`.  With M = 2^depth - 1, for every integer code k = 0 .. M, in double:
 *   x = (double)((float)k * (float)(1 / M))        the float lut3d forms from a code (lutr_apply_planar_rgb)
 *   t = clamp(x * slope + offset, 0, 1)            the product is exact in double, the sum is rounded once
 *   out[k] = (float)(power == 1 ? t : pow(t, power))
 * The identity CDL gives out[k] = (float)k * (float)(1 / M).  LUTR_EINVAL with a message: a null argument, a depth outside 8..16, a
 * channel outside 0..2, or a CDL lutr_apply_yuv_cdl refuses. */
int lutr_cdl_table(const lutr_cdl *cdl, int depth, int channel, float *out);

/* lutr_apply_yuv_xsub's pass (planar YUV in and out, any pair of 4:2:0 / 4:2:2 / 4:4:4, the equal pairs included, 8..16 bit on
 * either side) with the CDL between its YUV -> RGB stage and lut3d.  Per luma position, M = 2^lut_depth - 1:
 *   q   = YUV -> integer RGB (lutr_apply_yuv's stage 1, the full-range prologue included; chroma replicated over its INPUT block)
 *   T_c = lutr_cdl_table(cdl, lut_depth, c)[q_c]: slope, offset, clamp and power, tabulated per code on the host (the device
 *         never calls pow)
 *   o_c = med3(l + sat * (T_c - l), 0, 1) with l = (0.2126f * T_R + 0.7152f * T_G) + 0.0722f * T_B: fp32, every product and sum
 *         rounded on its own; skipped when sat == 1 (o_c = T_c)
 *   v   = lut3d on o: s_c = med3(o_c * scale_c * (n - 1), 0, n - 1), `interp` (all five modes), clip((int)(v * M), 0, M)
 *   out = integer RGB -> YUV from v (lutr_apply_yuv_xsub's stage 3: chroma = the mean over its OUTPUT block, a partial block at an
 *         odd edge takes the edge column / row again; constants: lutr_yuv_constants_xsub)
 * The identity CDL (1, 0, 1, saturation 1) gives lutr_apply_yuv_xsub's bits; saturation 0 feeds the lattice R = G = B; slope 0
 * feeds it the constant clamp(offset)^power.
 * The device table is kept in the context under (slope, offset, power, lut_depth) and rebuilt when they change: the upload is
 * ordered on the context's stream behind the kernels that still read the old table and returns once the host copy is consumed.
 * row0 and rows must be multiples of the union block height 2^max(icsy, ocsy) unless row0 + rows == h.
 * Always strict precision (fast / fma32 run strict here, no suffix on the last kernel).
 * Not in place: the bounding byte ranges (all rows and frames) of the source planes and of the destination planes must be
 * disjoint (the rule of lutr_apply_yuv_sited).
 * LUTR_EINVAL with a message, before anything touches the device: no lattice, a null argument or plane, a CDL with a number that is
 * not finite, a negative slope, a power that is not above 0 or a negative saturation, a .csp prelut on the context (its folded
 * table is per code, and the CDL's output is not a code), the format errors of lutr_apply_yuv_xsub (4:4:0, a depth outside
 * 8..16), 16-bit planes whose base, stride or (batches) frame stride is odd, row0 / rows off the union block, any overlap, variant
 * vec_lds (there is no LDS kernel for this path).  Variant vec_global where the vector kernel cannot take the call is LUTR_EINVAL
 * too, found where the kernel is chosen, as in the sibling entry points: the table may have been uploaded by then, no kernel has
 * run and nothing is written.
 * Kernels: "k_yuv_cdl_vec<win,wout,icsx,icsy,ocsx,ocsy,interp>" (nearest / trilinear / tetrahedral; the container mixes 8 -> 8,
 * 16 -> 16 and 16 -> 8 bit; width a multiple of 8 luma samples, 4 for 16 -> 16; positive strides aligned to the accesses; row0 /
 * rows multiples of the union block height), "k_yuv_cdl_generic" for everything else (one thread per union block; any depth,
 * stride, alignment or size; all five modes; an 8-bit source with a 16-bit output); a ragged width on aligned rows is split
 * between the two and named "<vector kernel>+k_yuv_cdl_generic".
 * Not covered: a prelut, dither, chroma siting, a resize, the two-output pass, premultiplied alpha, RGB / float / semi-planar /
 * packed / v210 sides, a tile (LDS) kernel.  The CDL together with the two-LUT chain or a 1D LUT is lutr_apply_yuv_stack's. */
int lutr_apply_yuv_cdl(lutr_ctx *ctx, const lutr_yuv_params *p, int interp, const lutr_cdl *cdl, int w, int h, int nframes,
                       const lutr_planes *src, const lutr_planes *dst, int row0, int rows);

/* ---- 1D LUT files: ffmpeg's lut1d, alone or ahead of lut3d in the fused pass -- the per-channel transform a
 *      camera vendor or a grading tool exports as a .cube with LUT_1D_SIZE (log to display gamma, legal to full, printer-light
 *      trims): `lut1d=file=tech.cube,lut3d=file=look.cube`.  The semantics restate FFmpeg's published vf_lut3d.c; they are
 *      unpinned, like the other file formats. ---- */
enum lutr_interp1d {
    LUTR_INTERP1D_NEAREST = 0,
    LUTR_INTERP1D_LINEAR  = 1,   /* lut1d's default */
    LUTR_INTERP1D_COSINE  = 2,
    LUTR_INTERP1D_CUBIC   = 3,
    LUTR_INTERP1D_SPLINE  = 4
};

/* Parse a .cube file with LUT_1D_SIZE n, 2 <= n <= 65536, followed by n rows of three floats.  *lut receives 3 x n floats,
 * channel c (0 = R, 1 = G, 2 = B) at [c * n]; free it with lutr_cube_free.  Lines are handled as lutr_cube_parse handles them
 * (comments, blank lines, TITLE, DOMAIN_MIN / DOMAIN_MAX between the size line and the last row, non-finite numbers refused),
 * plus `LUT_1D_INPUT_RANGE a b`, which sets min and max of all three channels.  scale[c] = clip(1 / (max[c] - min[c]), 0, 1), the
 * subtraction in float.  Errors name the file: a file that also carries LUT_3D_SIZE (a shaper ahead of a cube: not supported yet)
 * and a bad size are LUTR_EINVAL; fewer than n rows, a row with fewer than three numbers, no LUT_1D_SIZE are LUTR_EILSEQ.
 * lutr_cube_parse / lutr_lut_parse keep refusing 1D files.  Not covered: 1D .csp. */
int lutr_lut1d_parse(const char *path, float **lut, int *size, float scale[3]);

/* Host only, no context and no device: the per-code table of channel `channel` at `depth` bits (8..16), 2^depth entries into
 * `out`.  M = 2^depth - 1, factor = (float)M, sc = (scale[c] / factor) * (float)(size - 1); every operation rounded to fp32, no
 * contraction.  For every code k = 0 .. M: s = (float)k * sc, prev = (int)s, next = min(prev + 1, size - 1), mu = s - prev, p =
 * lut[c][prev], q = lut[c][next], and v by `interp1d` (FFmpeg's interp_1d_*):
 *   nearest  lut[c][(int)((double)s + .5)]
 *   linear   p + (q - p) * mu
 *   cosine   m = (1.f - cosf((float)(mu * M_PI))) * .5f;  p + (q - p) * m     (the one mode that depends on the C library's cosf)
 *   cubic    y0 = lut[max(prev - 1, 0)], y1 = p, y2 = q, y3 = lut[min(next + 1, size - 1)]; mu2 = mu * mu; a0 = y3 - y2 - y0 + y1,
 *            a1 = y0 - y1 - a0, a2 = y2 - y0, a3 = y1; a0 * mu * mu2 + a1 * mu2 + a2 * mu + a3, left to right
 *   spline   c0 = y1, c1 = .5f * (y2 - y0), c2 = y0 - 2.5f * y1 + 2.f * y2 - .5f * y3, c3 = .5f * (y3 - y0) + 1.5f * (y1 - y2);
 *            ((c3 * mu + c2) * mu + c1) * mu + c0
 * out[k] = (int)med3(v * factor, 0, factor): truncation; the clamp in float ahead of the conversion is the engine's own rule.
 * LUTR_EINVAL with a message: a null argument, size outside 2..65536, an unknown mode, depth outside 8..16, channel outside 0..2,
 * scale[channel] outside [0, 1], a node that is not finite. */
int lutr_lut1d_table(const float *lut, int size, const float scale[3], int interp1d, int depth, int channel, uint16_t *out);

/* The context's 1D LUT (layout of lutr_lut1d_parse) and its mode; lut NULL or size 0 removes it.  It lives beside the lattices:
 * lutr_ctx_set_lut, lutr_ctx_set_lut2, the broadcast and every other entry point leave it alone, and only the two entry points
 * below read it.  The device tables are built per depth at first use and uploaded on the context's stream, behind the kernels that
 * still read the previous one; they are told apart by a generation number taken here, never by the host address. */
int lutr_ctx_set_lut1d(lutr_ctx *ctx, const float *lut, int size, const float scale[3], int interp1d);

/* lutr_apply_yuv_xsub's pass (planar YUV in and out, any pair of 4:2:0 / 4:2:2 / 4:4:4, the equal pairs included, 8..16 bit on
 * either side) with the context's 1D LUT between its YUV -> RGB stage and lut3d.  Per luma position:
 *   q    = YUV -> integer RGB at lut_depth (lutr_apply_yuv's stage 1, the full-range prologue included; chroma replicated over
 *          its INPUT block)
 *   q'_c = lutr_lut1d_table(..., lut_depth, c)[q_c]
 *   v    = lut3d on the codes q' (`interp`, all five modes; a .csp prelut on the lattice is taken: q' is a code), or q' itself
 *          with interp == LUTR_INTERP_NONE (lut1d alone; no lattice needed)
 *   out  = integer RGB -> YUV from v (lutr_apply_yuv_xsub's stage 3; constants: lutr_yuv_constants_xsub)
 * The frame is integer RGB at lut_depth between the two filters, as it is between ffmpeg's lut1d and lut3d.  The identity 1D LUT
 * (lut[c][i] = i / (n - 1), n = 2^lut_depth, linear) gives the bits of the call without it.
 * row0 and rows must be multiples of the union block height 2^max(icsy, ocsy) unless row0 + rows == h.  Always strict precision,
 * no suffix on the last kernel.  Not in place (the overlap rule of lutr_apply_yuv_sited).
 * LUTR_EINVAL with a message, before anything touches the device: no 1D LUT set, no lattice (unless LUTR_INTERP_NONE), a null
 * argument or plane, the format errors of lutr_apply_yuv_xsub, 16-bit planes at odd addresses, row0 / rows off the union block,
 * any overlap, variant vec_lds.  Variant vec_global where the vector kernel cannot take the call is LUTR_EINVAL too, found where
 * the kernel is chosen.
 * Kernels: "k_yuv_l1d_vec<win,wout,icsx,icsy,ocsx,ocsy,interp>" (none (-1) / nearest / trilinear / tetrahedral; 8 -> 8, 16 -> 16
 * and 16 -> 8 bit containers; the layout rules of k_yuv_cdl_vec), a grid-stride walk whose workgroups stage the table into LDS
 * once when 3 * 2^lut_depth * 2 bytes <= 24 KB and LUTR_L1D_LDS is not 0, and read it from global memory otherwise -- the bits do
 * not depend on that; "k_yuv_l1d_generic" for everything else; a ragged width is split and named
 * "<vector kernel>+k_yuv_l1d_generic".
 * Not covered: cosine anywhere but the host table, float sources, the container formats of DESIGN.md 3.11 - 3.14, dither, chroma
 * siting, a resize, two outputs, premultiplied alpha, a tile (LDS window) kernel.  A 1D LUT behind lut3d, or together with a CDL
 * or the chain, is lutr_apply_yuv_stack's. */
int lutr_apply_yuv_lut1d(lutr_ctx *ctx, const lutr_yuv_params *p, int interp, int w, int h, int nframes, const lutr_planes *src,
                         const lutr_planes *dst, int row0, int rows);

/* lut1d alone on planar RGB (gbrp order: plane 0 = G, 1 = B, 2 = R) at `depth` bits (8: uint8, 9..16: uint16 LE):
 * out_c = lutr_lut1d_table(..., depth, c)[min(code_c, 2^depth - 1)] -- the clamp of container values above M is the engine's own
 * rule.  In place is allowed: each sample is read and written by one lane.  Kernels: "k_rgb_l1d<wide>" (whole-dword loads and
 * stores: bases and strides multiples of 4; the table in LDS or global memory on lutr_apply_yuv_lut1d's terms), "k_rgb_l1d_generic"
 * for unaligned planes and the columns past the last whole dword ("k_rgb_l1d<wide>+k_rgb_l1d_generic").  vec_lds is LUTR_EINVAL; vec_global is LUTR_EINVAL where the dword kernel cannot take the
 * whole call. */
int lutr_apply_planar_rgb_lut1d(lutr_ctx *ctx, int depth, int w, int h, int nframes, const lutr_planes *src, const lutr_planes *dst,
                                int row0, int rows);

/* ---- an ordered stack of lut1d / CDL / lut3d stages in one fused pass: what a dailies or finishing pipeline
 *      stacks between decode and encode -- input transform, per-clip CDL, show LUT; grade, technical LUT, look; look, output
 *      curve -- without a trip through YUV between the operators. ---- */
enum lutr_stage_kind {
    LUTR_STAGE_LUT3D   = 1,   /* the context's first lattice (lutr_ctx_set_lut), its .csp prelut taken where the pixel is a code */
    LUTR_STAGE_LUT3D_2 = 2,   /* the second lattice (lutr_ctx_set_lut2); never a prelut */
    LUTR_STAGE_LUT1D   = 3,   /* the context's 1D LUT (lutr_ctx_set_lut1d) */
    LUTR_STAGE_CDL     = 4,   /* the `cdl` argument of the call */
    LUTR_STAGE_MATRIX  = 5    /* the `mtx` argument of lutr_apply_yuv_stack_matrix; the other stack entries refuse it by name */
};
typedef struct lutr_stage {
    int32_t kind;             /* enum lutr_stage_kind */
    int32_t interp;           /* enum lutr_interp of a LUTR_STAGE_LUT3D / _LUT3D_2 stage (all five modes); not read for the others */
} lutr_stage;

/* lutr_apply_yuv_xsub's pass (planar YUV in and out, any pair of 4:2:0 / 4:2:2 / 4:4:4, the equal pairs included, 8..16 bit on
 * either side) with `nstages` stages, 1..4, each kind at most once, in the order given, between its YUV -> RGB stage and its RGB
 * -> YUV stage.  M = 2^lut_depth - 1.  A pixel travels between stages as CODES (integer R, G, B in [0, M] held as floats: what
 * stage 1 of lutr_apply_yuv produces) or as UNIT floats in [0, 1] (what the CDL produces):
 *   LUTR_STAGE_LUT1D     codes -> codes: q'_c = lutr_lut1d_table(..., lut_depth, c)[q_c]
 *   LUTR_STAGE_CDL       codes -> unit: T_c = lutr_cdl_table(cdl, lut_depth, c)[q_c], then the saturation mix of
 *                        lutr_apply_yuv_cdl (skipped when saturation == 1)
 *   LUTR_STAGE_LUT3D(_2) codes -> codes: lut3d as in lutr_apply_yuv (scale, the first lattice's prelut, `interp`, clip((int)(v * M),
 *                        0, M)); unit -> codes: lut3d as in lutr_apply_yuv_cdl (s_c = med3(o_c * scale_c * (n - 1), 0, n - 1), ...)
 *   unit -> codes        where a unit pixel meets LUTR_STAGE_LUT1D or the end of the list: q_c = (int)((o_c * (float)M) + 0.5f),
 *                        fp32, the product and the sum each rounded on their own; o_c in [0, 1] gives [0, M] without a clip
 * The RGB -> YUV stage takes codes (chroma = the mean over its OUTPUT block; constants: lutr_yuv_constants_xsub).
 * Bit for bit: {LUT3D} is lutr_apply_yuv_xsub without dither, {CDL, LUT3D} is lutr_apply_yuv_cdl, {LUT1D, LUT3D} is
 * lutr_apply_yuv_lut1d and {LUT1D} is that call with LUTR_INTERP_NONE, {LUT3D, LUT3D_2} is lutr_apply_yuv_chain.  {CDL} with the
 * identity CDL is the source through the two conversion stages alone at every depth 8..16.
 * The call is asynchronous on the context's stream and reuses the context's resources unchanged: both lattices, the CDL table
 * keyed by (slope, offset, power, lut_depth) with its stream-ordered upload, the 1D tables keyed by generation.
 * row0 and rows must be multiples of the union block height 2^max(icsy, ocsy) unless row0 + rows == h.  Always strict precision
 * (fast / fma32 run strict here, no suffix on the last kernel).  Not in place (the overlap rule of lutr_apply_yuv_sited).
 * LUTR_EINVAL with a message, before anything touches the device: a null argument or plane; nstages outside 1..4, an unknown
 * kind, a kind twice, an unknown mode on a lut3d stage; a stage whose resource is missing (no lattice, no second lattice, no 1D
 * LUT, a CDL stage with cdl == NULL) or a cdl without a CDL stage; a CDL lutr_apply_yuv_cdl refuses; LUTR_STAGE_LUT3D directly
 * behind LUTR_STAGE_CDL on a context with a .csp prelut; the format errors of lutr_apply_yuv_xsub; a lut_depth outside 8..16;
 * 16-bit planes at odd addresses; row0 / rows off the union block; any overlap; variant vec_lds.  Variant vec_global where the
 * vector kernel cannot take the call (layout, 8 -> 16 bit, a pyramid or prism stage) is LUTR_EINVAL too, found where the kernel
 * is chosen: tables may have been uploaded by then, no kernel has run and nothing is written.
 * Kernels, as lutr_ctx_last_kernel names them: "k_yuv_stack_vec<win,wout,icsx,icsy,ocsx,ocsy,tri,lds>[stages]" (nearest / trilinear /
 * tetrahedral stages; tri = 1 when a stage is trilinear, lds = 1 when the tables are staged in LDS; the layout rules of
 * k_yuv_cdl_vec), a grid-stride walk whose workgroups
 * stage the CDL and 1D tables the stack uses into LDS once when they fit 24 KB together (3 * 2^lut_depth * 4 bytes for the CDL, 3 *
 * 2^lut_depth * 2 for the 1D LUT) and LUTR_STACK_LDS is not 0, and read them from global memory otherwise -- the bits do not depend
 * on that; "k_yuv_stack_generic[stages]" for everything else; a ragged width is split and named
 * "<vector kernel>+k_yuv_stack_generic[stages]".  [stages] is the list as given, comma separated: lut3d:<interp>, lut3d2:<interp>,
 * lut1d, cdl -- for example "k_yuv_stack_vec<1,1,1,1,1,0,0,1>[lut1d,cdl,lut3d:2]".
 * Not covered: more than one stage of a kind, a tile (LDS window) kernel, RGB / float / alpha / semi-planar / packed / v210 sides,
 * dither, chroma siting, a resize, the two-output pass, premultiplied alpha. */
int lutr_apply_yuv_stack(lutr_ctx *ctx, const lutr_yuv_params *p, const lutr_stage *stages, int nstages, const lutr_cdl *cdl, int w,
                         int h, int nframes, const lutr_planes *src, const lutr_planes *dst, int row0, int rows);

/* ---- LUT strength: the "intensity" / "opacity" / key-gain control of a grade -- the graded pixel mixed with the
 *      source behind the stage list, in the one place where both are in registers as RGB codes. ----
 * lutr_apply_yuv_stack's pass with one step behind the list.  With M = 2^lut_depth - 1, q0_c the pixel's codes behind the YUV -> RGB
 * stage, q1_c the codes the list ends with (behind the closing unit -> codes rounding) and s the strength of the pixel's frame, in
 * fp32 with every operation rounded on its own:
 *   s'  = fminf(fmaxf(s, 0), 1), a NaN taken as 0
 *   q_c = (int)((q0_c + s' * (q1_c - q0_c)) + 0.5f)        the difference is exact; product, sum, sum: three roundings
 * and q_c feeds the RGB -> YUV stage as q1_c does in lutr_apply_yuv_stack.  q_c lies between q0_c and q1_c: no clip.  s = 1 gives
 * lutr_apply_yuv_stack's output bit for bit, s = 0 gives the source through the two conversion stages alone ({CDL} with the
 * identity CDL).
 * `frame_strength` = NULL: every frame takes `strength`.  Otherwise it points to nframes floats in device memory, read by the
 * kernel on the context's stream (the caller keeps them alive, as it does the planes): frame f of the call takes
 * frame_strength[f], f counted from the first frame of the call whatever row0 / rows are -- row shards give the bits of the whole
 * call -- and `strength` is not read.
 * Every refusal of lutr_apply_yuv_stack, and LUTR_EINVAL for a `strength` that is NaN or outside [0, 1] when frame_strength is
 * NULL (the values of the array cannot be seen from the host: the kernels clamp them).
 * Kernels: always the mix forms, at strength 1 as well -- "k_yuv_stack_mix_vec<win,wout,icsx,icsy,ocsx,ocsy,tri,lds>[stages]",
 * "k_yuv_stack_mix_generic[stages]", "<vector kernel>+k_yuv_stack_mix_generic[stages]" for a ragged width, chosen by the rules of
 * lutr_apply_yuv_stack; both table placements give the same bits.
 * Not covered: what lutr_apply_yuv_stack does not cover; a tile (LDS window) kernel. */
int lutr_apply_yuv_stack_mix(lutr_ctx *ctx, const lutr_yuv_params *p, const lutr_stage *stages, int nstages, const lutr_cdl *cdl,
                             float strength, const float *frame_strength, int w, int h, int nframes, const lutr_planes *src,
                             const lutr_planes *dst, int row0, int rows);

/* ---- a matte plane: a strength per pixel -- the key that holds a look off the skin tones, a power window, a
 *      title-safe area left alone, a wipe between graded and ungraded. ----
 * lutr_apply_yuv_stack_mix's pass with the strength of a pixel scaled by a matte sample.  The matte is one plane at luma
 * resolution of unsigned codes of `depth` bits (8..16), Mm = 2^depth - 1: bytes when depth == 8, little-endian 16-bit words
 * otherwise.  With a the code at the pixel's luma position and s' the clamped strength of the pixel's frame, in fp32 with every
 * operation rounded on its own:
 *   a'  = min(a, Mm)                          a 16-bit container may hold more than `depth` bits
 *   a'' = invert ? Mm - a' : a'
 *   t   = (float)a'' * rcp                    rcp = 1.0f / (float)Mm, formed once on the host
 *   w   = s' * t
 *   q_c = (int)((q0_c + w * (q1_c - q0_c)) + 0.5f)
 * and q_c feeds the RGB -> YUV stage: luma per pixel, chroma from the block sums of the mixed codes, so a matte edge inside a
 * chroma block is handled in RGB ahead of the mean.  t is increasing in a, never above 1 and exactly 1 at Mm: a matte of Mm
 * everywhere (0 everywhere with invert) gives lutr_apply_yuv_stack_mix's output bit for bit, a matte of 0 everywhere that of
 * strength 0.
 * The matte has no chroma plane.  `data` is row 0 of the first frame, as the planes' pointers are; the sample of a pixel is at its
 * absolute luma row and column, so row shards give the bits of the whole call.  frame_stride 0 with nframes > 1 is a still matte:
 * every frame reads the same plane.
 * Every refusal of lutr_apply_yuv_stack_mix, and LUTR_EINVAL before anything touches the device for: a null matte or data, a
 * depth outside 8..16, invert outside 0 | 1, a stride shorter than a row of the matte, an odd base, stride or frame stride on a
 * 16-bit container, a negative frame stride, a matte that overlaps a destination plane.
 * Kernels: always the matte forms, with a constant matte as well --
 * "k_yuv_stack_matte_vec<win,wout,wm,icsx,icsy,ocsx,ocsy,tri,lds>[stages]" (wm: the matte's container; built for wm == win and
 * for bytes beside a 16-bit source; base, stride and frame stride aligned to the thread's 4..16 bytes),
 * "k_yuv_stack_matte_generic[stages]" for everything else, "<vector kernel>+k_yuv_stack_matte_generic[stages]" for a ragged width.
 * Not covered: what lutr_apply_yuv_stack_mix does not cover; a matte at chroma resolution or in floats; feathering or any
 * other processing of the matte. */
typedef struct lutr_matte {
    const void *data;         /* device */
    ptrdiff_t   stride;       /* bytes between rows */
    int64_t     frame_stride; /* bytes between frames; 0 = one matte for every frame */
    int32_t     depth;        /* 8..16 */
    int32_t     invert;       /* 0 | 1 */
} lutr_matte;
int lutr_apply_yuv_stack_matte(lutr_ctx *ctx, const lutr_yuv_params *p, const lutr_stage *stages, int nstages, const lutr_cdl *cdl,
                               float strength, const float *frame_strength, const lutr_matte *matte, int w, int h, int nframes,
                               const lutr_planes *src, const lutr_planes *dst, int row0, int rows);

/* ---- an RGB matrix stage in the stack: the 3x3 matrix with offset of a colour pipeline -- a gamut conversion
 *      between a camera curve and a working space (lut1d, matrix, lut3d), a white-balance or channel-mixer trim ahead of the
 *      show LUT, a channel swap. ----
 * lutr_apply_yuv_stack's pass with one more stage kind, LUTR_STAGE_MATRIX, at most once in the list of 1..4 stages, in any
 * position; its resource is the `mtx` argument of the call, as the CDL is `cdl`.  m is row-major: row 0 gives R', row 1 G', row 2
 * B', from (R, G, B).  The stage takes a pixel in either state and produces UNIT floats.  With M = 2^lut_depth - 1, in fp32 with
 * every operation rounded on its own (no contraction):
 *   u_c = q_c * rcp                           from codes; rcp = 1.0f / (float)M, formed once on the host: the float the identity
 *                                             CDL's table holds for code q_c
 *   u_c = o_c                                 from unit
 *   t_r = ((m[0] * u_r + m[1] * u_g) + m[2] * u_b) + offset[0]        likewise t_g (row 1), t_b (row 2)
 *   o_c = min(max(t_c, 0), 1)
 * Behind it: a lut3d / lut3d2 stage runs in its unit form, as behind the CDL (LUTR_STAGE_LUT3D with a .csp prelut is refused
 * there, as behind the CDL); LUTR_STAGE_LUT1D and the end of the list take the unit -> codes rounding of lutr_apply_yuv_stack; and
 * so does LUTR_STAGE_CDL, whose table is per code: {MATRIX, CDL} quantises to lut_depth bits in between.
 * Bit for bit: {MATRIX} with the identity is {CDL} with the identity CDL, {MATRIX(I), LUT3D} is {CDL(identity), LUT3D},
 * {LUT3D, MATRIX(I)} is {LUT3D} and {MATRIX(I), LUT1D} is {LUT1D}.
 * Everything else -- stages 1 and 3, the prologue, layouts, depths, row rules, the overlap rule, the resources, strict
 * arithmetic -- is lutr_apply_yuv_stack's.
 * LUTR_EINVAL with a message, before anything touches the device: everything lutr_apply_yuv_stack refuses; a matrix stage with
 * mtx == NULL, or mtx without a matrix stage; an entry of m or offset that is not finite or above 65536 in magnitude (which
 * keeps every sum finite: no NaN reaches the clamp).  lutr_apply_yuv_stack, _mix and _matte refuse LUTR_STAGE_MATRIX by name.
 * Kernels: always the matrix forms, whose twelve numbers are kernel arguments --
 * "k_yuv_stack_mtx_vec<win,wout,icsx,icsy,ocsx,ocsy,tri,lds>[stages]", "k_yuv_stack_mtx_generic[stages]",
 * "<vector kernel>+k_yuv_stack_mtx_generic[stages]" for a ragged width, chosen by the rules of lutr_apply_yuv_stack; the stage is
 * "matrix" in [stages].
 * Not covered: what lutr_apply_yuv_stack does not cover; a strength or a matte together with a matrix; a second matrix; a tile
 * (LDS window) kernel; named gamut presets. */
typedef struct lutr_rgb_matrix {
    float m[9];               /* row-major */
    float offset[3];          /* in unit floats */
} lutr_rgb_matrix;
int lutr_apply_yuv_stack_matrix(lutr_ctx *ctx, const lutr_yuv_params *p, const lutr_stage *stages, int nstages, const lutr_cdl *cdl,
                                const lutr_rgb_matrix *mtx, int w, int h, int nframes, const lutr_planes *src,
                                const lutr_planes *dst, int row0, int rows);

/* ---- the stage stack on RGB sources: a DPX / TIFF / PNG sequence through an input transform, a per-shot CDL, a
 *      gamut matrix and the show LUT in one pass, into a YUV master or back into planar RGB ----
 * The source is lutr_apply_rgb_to_yuv's: src_kind == 0 takes gbrp planes in src_planar (plane 0 = G, 1 = B, 2 = R; uint8 at depth 8,
 * else uint16 LE), src_kind == LUTR_PK_* / LUTR_PACKED(...) one packed image in src_packed (a fourth component is read past).  Its
 * integer codes at the depth dl of the list enter the list as codes held as floats -- the state stage 1 of lutr_apply_yuv_stack
 * produces -- and a 16-bit word above M = 2^dl - 1 acts as M.  The list is lutr_apply_yuv_stack_matrix's, unchanged: 1..4 stages out
 * of LUT3D, LUT3D_2, LUT1D, CDL, MATRIX, each at most once, in any order, every lattice stage with its own mode (all five), the
 * first lattice's .csp prelut taken where it is fed codes, the same compiled steps, the same unit -> codes rounding and per-stage
 * arithmetic in strict fp32 without contraction.
 * dst_kind == LUTR_RGB_STACK_YUV: dl = p->lut_depth (a packed source's bits); the list's final codes go through the output stage
 *   of lutr_apply_rgb_to_yuv into planar YUV p->fmt_out (4:2:0 / 4:2:2 / 4:4:4 at 8..16 bit; constants
 *   lutr_yuv_constants_rgb2yuv; each chroma sample from the sum of the final codes over its output block; a partial block takes
 *   the edge column / row again).  Of *p only fmt_out, lut_depth, matrix_out and range_out are read.  Not in place: the byte-range
 *   rule of lutr_apply_rgb_to_yuv.
 * dst_kind == 8..16: dl = dst_kind, which a packed source's bits must equal; the final codes are stored as they are into three
 *   gbrp planes of dl bits in dst (G, B, R).  p is not read and may be NULL.  dst may be a planar source's own planes (the same
 *   base, stride and frame stride plane by plane: a sample is read and written by the same lane); any other overlap is refused.
 * row0 and rows must be multiples of the output chroma block height (1 for a gbrp destination) unless row0 + rows == h.
 * Bit for bit: {LUT3D} into YUV is lutr_apply_rgb_to_yuv; {LUT3D} into gbrp is lutr_apply_planar_rgb; {LUT1D} into gbrp is
 * lutr_apply_planar_rgb_lut1d; {CDL} with the identity CDL and {MATRIX} with the identity matrix into gbrp give the source
 * (codes <= M).
 * LUTR_EINVAL with a message, before anything touches the device: everything lutr_apply_yuv_stack_matrix refuses about the list
 * and its resources; a dst_kind that is neither; a packed source whose bits differ from dl; the format errors of
 * lutr_apply_rgb_to_yuv; variant vec_lds; an overlap as above.
 * Kernels: "k_rgb_stack_vec<win,nc,wout,sink,ocsx,ocsy,tri,lds>[stages]" (nc = 1 planar, 3 | 4 packed; sink 0 = YUV, 1 = gbrp;
 * nearest / trilinear / tetrahedral stages; 8 -> 8, 16 -> 16 and, into YUV, 16 -> 8 bit containers; the layout rules of
 * "k_rgb2yuv_vec"; the tables in LDS when they fit 24 KB, LUTR_STACK_LDS=0 | 1 as for lutr_apply_yuv_stack),
 * "k_rgb_stack_generic[stages]" for everything else, "<vector kernel>+k_rgb_stack_generic[stages]" for a ragged width on aligned
 * rows; [stages] as lutr_apply_yuv_stack writes it.  vec_global fails with LUTR_EINVAL where the vector kernel cannot take the call.
 * Not covered: packed RGB destinations, float sources, a strength or a matte, dither, a resize, semi-planar / packed YUV
 * destinations, a tile (LDS window) kernel. */
#define LUTR_RGB_STACK_YUV 0
int lutr_apply_rgb_stack(lutr_ctx *ctx, const lutr_yuv_params *p, const lutr_stage *stages, int nstages, const lutr_cdl *cdl,
                         const lutr_rgb_matrix *mtx, int src_kind, int w, int h, int nframes, const lutr_planes *src_planar,
                         const lutr_packed *src_packed, int dst_kind, const lutr_planes *dst, int row0, int rows);

/* ---- the stage stack from YUV sources into RGB frames: a camera file (ProRes / HEVC) graded with the per-shot
 *      CDL and the show LUT into a DPX / TIFF / PNG sequence, or with lut1d,matrix,lut3d into rgba / bgra for a viewer ----
 * The source and the destination are lutr_apply_yuv_to_rgb's, and so are dst_kind and the fields of *p that are read (fmt_in,
 * lut_depth, matrix_in, range_src, range_in): planar YUV p->fmt_in (4:2:0 / 4:2:2 / 4:4:4 at any depth din in 8..16; 4:4:0 is
 * LUTR_EINVAL) -> [the prologue only if range_src != range_in, on lutr_apply_yuv_to_rgb's terms] -> each chroma sample replicated
 * over its INPUT block -> integer RGB codes at dl = p->lut_depth, the destination's depth (constants lutr_yuv_constants_yuv2rgb,
 * unchanged) -> the list of lutr_apply_rgb_stack / lutr_apply_yuv_stack_matrix, unchanged: 1..4 stages out of LUT3D, LUT3D_2,
 * LUT1D, CDL, MATRIX, each at most once, in any order, every lattice stage with its own mode (all five), the first lattice's .csp
 * prelut taken where it is fed codes, the same compiled steps, the same unit -> codes rounding and per-stage arithmetic in strict
 * fp32 without contraction -> the final codes stored as they are: gbrp planes at dl in dst_planar (dst_kind == 0; G, B, R), or one
 * packed image in dst_packed (dst_kind == LUTR_PK_* / LUTR_PACKED(...), whose bits dl must be; a fourth component is written
 * 2^dl - 1, opaque; 16-bit formats need 2-byte aligned rows).
 * row0 and rows must be multiples of the input chroma block height 2^icsy unless row0 + rows == h.  Not in place: the byte-range
 * rule of lutr_apply_yuv_to_rgb.
 * Bit for bit: {LUT3D} is lutr_apply_yuv_to_rgb with that mode; {CDL} with the identity CDL and {MATRIX} with the identity matrix
 * are lutr_apply_yuv_to_rgb with LUTR_INTERP_NONE; any list is lutr_apply_rgb_stack from gbrp into gbrp on the planes
 * lutr_apply_yuv_to_rgb with LUTR_INTERP_NONE writes at dl (the conversion clips to [0, 2^dl - 1]), arranged as the destination.
 * LUTR_EINVAL with a message, before anything touches the device: everything lutr_apply_yuv_stack_matrix refuses about the list
 * and its resources; the format errors of lutr_apply_yuv_to_rgb; variant vec_lds; an overlap as above.
 * Kernels: "k_yuv2rgb_stack_vec<win,icsx,icsy,nc,wout,tri,lds>[stages]" (nc = 1 planar, 3 | 4 packed; nearest / trilinear /
 * tetrahedral stages; the layout rules of "k_yuv2rgb_vec"; the tables in LDS when they fit 24 KB, LUTR_STACK_LDS=0 | 1 as for
 * lutr_apply_yuv_stack), "k_yuv2rgb_stack_generic[stages]" for everything else, "<vector kernel>+k_yuv2rgb_stack_generic[stages]"
 * for a ragged width on aligned rows; [stages] as lutr_apply_yuv_stack writes it.  vec_global fails with LUTR_EINVAL where the
 * vector kernel cannot take the call.
 * Not covered: a strength or a matte, dither, a resize, chroma siting, a float destination, semi-planar / packed 4:2:2 / v210
 * sources, alpha carried into a packed destination, a tile (LDS window) kernel. */
int lutr_apply_yuv_stack_to_rgb(lutr_ctx *ctx, const lutr_yuv_params *p, const lutr_stage *stages, int nstages, const lutr_cdl *cdl,
                                const lutr_rgb_matrix *mtx, int dst_kind, int w, int h, int nframes, const lutr_planes *src,
                                const lutr_planes *dst_planar, const lutr_packed *dst_packed, int row0, int rows);

/* ---- the stage stack on semi-planar sides: a hardware-decoded p010le / nv12 file through lut1d,cdl,lut3d into a
 *      yuv422p10le master or back into p010le / nv12 for a hardware encoder, without a de-interleave pass ahead of the stack and
 *      an interleave pass behind it ----
 * lutr_apply_yuv_stack with each side in the container its layout names (lutr_yuv_layout, as lutr_apply_yuv_semi takes it): three
 * planes, or luma and one plane of (Cb, Cr) pairs -- (Cr, Cb) with swap --, 16-bit codes `shift` bits up in their words.  The
 * result is bit-identical to lutr_apply_yuv_stack on the same samples held in three planes, put into the destination's
 * container: the list, its compiled steps, the union block of the two layouts (chroma replicated over its input block, averaged
 * over its output block), the full-range prologue and everything else *p expresses are that call's arithmetic unchanged.  On
 * input the code is word >> shift whatever the low bits hold; on output the word is code << shift, low bits zero.
 * A semi-planar side is 4:2:0 or 4:2:2; the other side may be 4:2:0 / 4:2:2 / 4:4:4, planar or semi-planar, at 8..16 bit: this is
 * the one call that changes the chroma subsampling of a semi-planar frame.  Stages: 1..4 out of LUT3D, LUT3D_2, LUT1D, CDL, each at
 * most once, in any order, on lutr_apply_yuv_stack's terms (a .csp prelut where that call allows it).  row0 and rows must be
 * multiples of the union block height unless row0 + rows == h.  When both layouts are planar with shift 0 this IS
 * lutr_apply_yuv_stack: same kernels, bits, last kernel.  Always strict precision (fast / fma32 run strict here).
 * Not in place: no byte range of a source plane may overlap one of a destination plane, over all rows and frames; a plane of
 * pairs spans 2 * ceil(w / 2) samples a row and a semi-planar side has no plane 2.
 * LUTR_EINVAL with a message, before anything touches the device: a null layout; everything lutr_apply_yuv_stack refuses about the
 * list and its resources -- a MATRIX stage with that call's words; everything lutr_apply_yuv_semi refuses about a layout (a wrong
 * shift, swap without semi, semi / swap outside 0 | 1, a semi-planar side that is 4:4:4, a missing plane, odd 16-bit planes);
 * variant vec_lds; an overlap as above.
 * Kernels: "k_yuv_stack_semi_vec<win,wout,icsx,icsy,ocsx,ocsy,tri,lds>[stages]" (nearest / trilinear / tetrahedral stages; 8 -> 8,
 * 16 -> 16 and 16 -> 8 bit containers; the eight layout pairs with a 4:2:0 / 4:2:2 side; width a multiple of 8 luma samples, 4 for
 * 16 -> 16; positive strides aligned to the accesses -- a plane of pairs moves twice the bytes of a planar chroma plane per
 * access; the tables in LDS when they fit 24 KB, LUTR_STACK_LDS=0 | 1 as for lutr_apply_yuv_stack),
 * "k_yuv_stack_semi_generic[stages]" for everything else (one thread per union block; any depth 8..16, stride, alignment or size;
 * all five modes), "<vector kernel>+k_yuv_stack_semi_generic[stages]" for a ragged width on aligned rows; [stages] as
 * lutr_apply_yuv_stack writes it.  vec_global fails with LUTR_EINVAL where the vector kernel cannot take the layout.
 * Not covered: a matrix stage, a strength or a matte, dither, chroma siting, a resize, a second output, alpha (semi-planar formats
 * carry none), packed 4:2:2 / v210 / RGB sides, 4:4:4 semi-planar (nv24, p410le), big-endian containers, a tile (LDS window)
 * kernel. */
int lutr_apply_yuv_stack_semi(lutr_ctx *ctx, const lutr_yuv_params *p, const lutr_stage *stages, int nstages, const lutr_cdl *cdl,
                              const lutr_yuv_layout *in_layout, const lutr_yuv_layout *out_layout, int w, int h, int nframes,
                              const lutr_planes *src, const lutr_planes *dst, int row0, int rows);

/* ---- the stage stack on capture frames: v210 / uyvy422 from a capture card through lut1d,cdl,lut3d into v210 /
 *      uyvy422 for a play-out card or into a yuv422p10le master, without an unpacking pass ahead of the stack and a packing pass
 *      behind it ----
 * lutr_apply_yuv_stack with each side planar or packed 4:2:2 (lutr_yuv_packing, as lutr_apply_yuv_packed takes it), or with each
 * side planar or v210 (in_v210 / out_v210, as lutr_apply_yuv_v210 takes them).  The result is bit-identical to
 * lutr_apply_yuv_stack on the same samples held in three planes, put into the destination's container: the list, its compiled
 * steps, the full-range prologue, lut_depth and everything else *p expresses are that call's arithmetic unchanged.  The side rules
 * and the container rules are lutr_apply_yuv_packed's and lutr_apply_yuv_v210's: a packed / v210 side is 4:2:2 (v210: 10 bit);
 * with a packed / v210 source the planar destination may be 4:2:2, 4:2:0 or 4:4:4 at 8..16 bit; a packed / v210 destination takes a
 * 4:2:2 source; low bits under a shift and bits 30-31 of a v210 word are ignored on input and zero on output; slots beyond the
 * frame are ignored on input and replicated on output; row bytes past the last group are never written.
 * Stages: 1..4 out of LUT3D, LUT3D_2, LUT1D, CDL, each at most once, in any order, on lutr_apply_yuv_stack's terms.  row0 and rows
 * must be multiples of the destination's chroma block height unless row0 + rows == h.  With both sides planar either call IS
 * lutr_apply_yuv_stack.  Always strict precision.  A packed 4:2:2 side and a v210 side in one call are not supported: each entry
 * takes its own kind.
 * Not in place: no byte range of a source plane may overlap one of a destination plane, over all rows and frames.
 * LUTR_EINVAL with a message, before anything touches the device: a null packing; everything lutr_apply_yuv_stack refuses about the
 * list and its resources -- a MATRIX stage with that call's words; everything lutr_apply_yuv_packed / lutr_apply_yuv_v210 refuses
 * about a side; variant vec_lds; an overlap as above.
 * Kernels: "k_yuv_stack_pk_vec<win,wout,pi,po,ocsy,tri,lds>[stages]" / "k_yuv_stack_v210_vec<wp,vi,vo,ocsy,tri,lds>[stages]" under
 * the layout conditions of k_yuv_pk_vec / k_yuv_v210_vec and nearest / trilinear / tetrahedral stages (the tables in LDS when they
 * fit 24 KB, LUTR_STACK_LDS=0 | 1 as for lutr_apply_yuv_stack), "k_yuv_stack_pk_generic[stages]" /
 * "k_yuv_stack_v210_generic[stages]" for everything else, "<vector kernel>+<generic kernel>[stages]" for a ragged width on aligned
 * rows; [stages] as lutr_apply_yuv_stack writes it.  vec_global fails with LUTR_EINVAL where the vector kernel cannot take the
 * layout.
 * Not covered: a matrix stage, a strength or a matte, dither, chroma siting, a resize, a second output, alpha, semi-planar / RGB
 * sides, v210x / v410 / packed 4:4:4 / big-endian containers, a tile (LDS window) kernel. */
int lutr_apply_yuv_stack_packed(lutr_ctx *ctx, const lutr_yuv_params *p, const lutr_stage *stages, int nstages, const lutr_cdl *cdl,
                                const lutr_yuv_packing *in, const lutr_yuv_packing *out, int w, int h, int nframes,
                                const lutr_planes *src, const lutr_planes *dst, int row0, int rows);
int lutr_apply_yuv_stack_v210(lutr_ctx *ctx, const lutr_yuv_params *p, const lutr_stage *stages, int nstages, const lutr_cdl *cdl,
                              int in_v210, int out_v210, int w, int h, int nframes, const lutr_planes *src, const lutr_planes *dst,
                              int row0, int rows);

/* ---- the alpha plane of yuva* / gbrap* frames: ProRes 4444 (yuva444p10le / 12le), VP8 / VP9 with alpha
 *      (yuva420p), PNG / TIFF / EXR sequences with alpha (rgba, rgba64le, gbrap*, gbrapf32le).  In the reference's chain lut3d
 *      copies the alpha plane through and format=<pix_fmt> keeps, converts, drops or makes it (ffmpeg.py:246, :304-310) ---- */
enum lutr_alpha_kind {
    LUTR_ALPHA_NONE  = 0,    /* the source has no alpha: the destination plane is filled with 2^dout - 1 (opaque) */
    LUTR_ALPHA_INT   = 1,    /* integer samples at `depth` bits: uint8 for depth 8, else uint16 LE */
    LUTR_ALPHA_FLOAT = 2     /* 32-bit float samples, 1.0 = opaque (gbrapf32le) */
};
/* Where the alpha samples of a frame (or a batch) are.  Sample x of row y of frame f is element x * step + offset of the row at
 * data + f * frame_stride + y * stride; an element is 1 byte (LUTR_ALPHA_INT, depth 8), 2 bytes (depth 9..16) or 4 bytes
 * (LUTR_ALPHA_FLOAT).  A plane has step 1, offset 0; the A of a packed rgba / bgra image has step 4, offset 3, of argb / abgr
 * step 4, offset 0, of rgba64le / bgra64le step 4, offset 3 at depth 16.  With LUTR_ALPHA_NONE only `kind` is read. */
typedef struct lutr_alpha_src {
    int32_t     kind;            /* enum lutr_alpha_kind */
    int32_t     depth;           /* LUTR_ALPHA_INT: 8..16 */
    const void *data;
    ptrdiff_t   stride;          /* bytes between rows */
    int64_t     frame_stride;    /* bytes between frames of a batch (ignored when nframes == 1) */
    int32_t     step;            /* elements between two samples of a row, >= 1 */
    int32_t     offset;          /* element index of the sample inside its pixel, 0 .. step - 1 */
} lutr_alpha_src;

/* Writes rows [row0, row0 + rows) of the alpha plane `dst` (w x h samples at `dout` bits, 8 -> uint8, 9..16 -> uint16 LE; dst_stride
 * / dst_frame_stride in bytes) of each of nframes frames; rows outside the range are not written.  Alpha and colour are
 * independent: nothing of a context's lattice, precision, matrices, ranges or dither reaches this call, alpha is never dithered and
 * is treated as straight (a premultiplied source keeps its alpha while the LUT runs on its premultiplied colour, as ffmpeg's
 * chain gives it).  No lattice is needed.
 *   LUTR_ALPHA_INT, depth == dout: the words are copied as they are.
 *   LUTR_ALPHA_INT, depth != dout: with Mi = 2^depth - 1, Mo = 2^dout - 1: a = min(word, Mi), a' = floor((2 a Mo + Mi) / (2 Mi)) --
 *     the nearest code (Mi is odd: no ties); 0 -> 0, Mi -> Mo, monotone, 8 -> 16 bit is a * 257, up then down is the identity.
 *   LUTR_ALPHA_FLOAT: q = clip(rintf(a * (float)Mo), 0, Mo): one fp32 multiply, round half to even, NaN -> 0 by its bit pattern.
 *   LUTR_ALPHA_NONE: every sample is Mo.
 * The source plane as the destination plane (same pointer, strides and depth, step 1) is allowed and does nothing (the last
 * kernel is then "k_alpha_nop").  Any other overlap of the two bounding byte ranges (all rows and frames) is LUTR_EINVAL.
 * LUTR_EINVAL with a message, before anything touches the device: a null context, descriptor or destination, a null source
 * pointer with a kind other than LUTR_ALPHA_NONE, a kind outside 0..2, depth or dout outside 8..16, step < 1 or offset outside
 * 0 .. step - 1, 16-bit samples whose base, stride or (batches) frame stride is odd, float samples not 4-byte aligned, negative
 * sizes or rows outside the frame, overlap other than the no-op.
 * Kernels: "k_alpha_vec<src,wout>" (src 0 = 8-bit, 1 = 16-bit, 2 = float source words, wout = 16-bit destination words; a plane
 * source (step 1); width a multiple of 8 samples, 16 for 8 -> 8 bit; positive strides; both planes aligned to what a thread moves:
 * 16 bytes on a 16-bit or float side, 8 on an 8-bit side next to one of those, 16 for 8 -> 8 bit; fewer than 2^31 units),
 * "k_alpha_generic" for everything else (one sample per thread; any stride, negative included, any alignment allowed above, odd
 * sizes, packed sources); a ragged width on aligned rows is split between the two; "k_alpha_fill" for LUTR_ALPHA_NONE (16-byte
 * stores under the vector kernel's conditions on the destination, one sample per thread otherwise, split likewise).
 * Variants: auto and generic as for lutr_apply_yuv; vec_global fails with LUTR_EINVAL where the vector kernel cannot take the
 * layout; vec_lds always fails with LUTR_EINVAL (there is no LDS kernel for this path).  Asynchronous on the context's stream.
 * Not covered: an alpha resize, alpha inside semi-planar / packed YUV / v210 containers (ayuv64le, vuya), a float alpha
 * destination.  (Premultiplied colour: lutr_apply_yuv_premul / lutr_apply_planar_rgb_f32_premul below; this call is the same.) */
int lutr_alpha_plane(lutr_ctx *ctx, const lutr_alpha_src *src, int dout, void *dst, ptrdiff_t dst_stride, int64_t dst_frame_stride,
                     int w, int h, int nframes, int row0, int rows);

/* ---- premultiplied alpha: unpremultiply, lut3d, premultiply in one pass.  OpenEXR is premultiplied by
 *      specification (gbrapf32le), ProRes 4444 elements (yuva444p10le / 12le) usually are; a non-linear LUT on premultiplied
 *      colour is wrong wherever 0 < alpha < 1.  An engine setting: ffmpeg's chain has no such step. ---- */
/* lutr_apply_yuv_xsub's pass (planar YUV in and out, any pair of 4:2:0 / 4:2:2 / 4:4:4, the equal pairs included, 8..16 bit on
 * either side) on the colour planes `src` -> `dst` of a source whose alpha plane is `alpha`: kind LUTR_ALPHA_INT, depth equal to the
 * depth of p->fmt_in, step 1, offset 0 (a luma-sized plane).  Per luma position, with a = min(alpha word, Ma), Ma = 2^din - 1,
 * Ml = 2^lut_depth - 1:
 *   q   = YUV -> integer RGB (lutr_apply_yuv's stage 1; chroma replicated over its INPUT block)
 *   S   = min(Ml, floor((q * Ma + floor(a / 2)) / a)) per channel for a > 0, S = q for a == 0 (exact integers)
 *   o   = lut3d on S: `interp` (all five modes), the context's scale, its .csp prelut if set; clip((int)(v * Ml), 0, Ml)
 *   P   = floor((o * a + floor(Ma / 2)) / Ma) per channel
 *   out = integer RGB -> YUV from P (lutr_apply_yuv_xsub's stage 3: chroma = the mean over its OUTPUT block, a partial block at an
 *         odd edge takes the edge column / row again; constants: lutr_yuv_constants_xsub)
 * a == Ma makes both steps the identity (the bits of the straight call), a == 0 gives P == 0.  The destination's alpha plane is
 * not written here: lutr_alpha_plane copies or converts it afterwards, as for a straight call.
 * row0 and rows must be multiples of the union block height 2^max(icsy, ocsy) unless row0 + rows == h.
 * Always strict precision (fast / fma32 run strict here, no suffix on the last kernel).
 * Not in place: the bounding byte ranges (all rows and frames) of the source planes and of the alpha source must be disjoint from
 * those of the destination planes (the rule of lutr_apply_rgb_to_yuv; the alpha source is named source plane 3).
 * LUTR_EINVAL with a message, before anything touches the device: no lattice, a null argument or plane, the format errors of
 * lutr_apply_yuv_xsub (4:4:0, a depth outside 8..16), a prologue (range_src != range_in, or lut_depth other than the source's
 * depth: such a call has no alpha to carry), an alpha source of another kind, depth, step or offset, 16-bit planes whose base,
 * stride or (batches) frame stride is odd, row0 / rows off the union block, any overlap, variant vec_lds (there is no LDS kernel
 * for this path).  Variant vec_global where the vector kernel cannot take the call is LUTR_EINVAL too, found where the kernel is
 * chosen, as in the sibling entry points: no kernel has run and nothing is written.
 * Kernels: "k_yuva_premul_vec<win,wout,icsx,icsy,ocsx,ocsy,interp>" (nearest / trilinear / tetrahedral; the container mixes
 * 8 -> 8, 16 -> 16 and 16 -> 8 bit; width a multiple of 8 luma samples, 4 for 16 -> 16; positive strides aligned to the accesses,
 * the alpha plane like luma; row0 / rows multiples of the union block height), "k_yuva_premul_generic" for everything else (one
 * thread per union block; any depth, stride, alignment or size; all five modes; an 8-bit source with a 16-bit output); a ragged
 * width on aligned rows is split between the two and named "<vector kernel>+k_yuva_premul_generic".
 * Not covered: dither, chroma siting, a resize, the two-output pass, the two-LUT chain, integer RGB sources (PNG / TIFF are
 * straight), an RGB source into yuva* (EXR -> yuva444p*), semi-planar / packed / v210 sides, a tile (LDS) kernel. */
int lutr_apply_yuv_premul(lutr_ctx *ctx, const lutr_yuv_params *p, int interp, int w, int h, int nframes, const lutr_planes *src,
                          const lutr_alpha_src *alpha, const lutr_planes *dst, int row0, int rows);

/* lutr_apply_planar_rgb_f32's pass (gbrpf32 planes G, B, R in `src` and `dst`) on the colour planes of a gbrapf32le source whose
 * alpha plane is `alpha`: kind LUTR_ALPHA_FLOAT, step 1, offset 0.  Per pixel, with a the alpha float:
 *   t  = clamp(a, 0, 1); NaN -> 0 by its bit pattern, -0 -> +0
 *   S  = sanitize(c) / t for t > 0, sanitize(c) for t == 0: one IEEE fp32 division (round to nearest even, subnormals kept),
 *        then sanitised again (an overflow to +-inf becomes +-FLT_MAX)
 *   L  = lutr_apply_planar_rgb_f32's lut3d on S (the prelut per pixel, nothing clipped)
 *   out = L * t: one fp32 multiply
 * t == 1 reproduces lutr_apply_planar_rgb_f32 bit for bit.  The alpha plane itself is the caller's to copy.
 * `dst` may be `src` (in place); the alpha source must not overlap a destination plane.  Always strict precision.
 * LUTR_EINVAL with a message, before anything touches the device: what lutr_apply_planar_rgb_f32 refuses, a null alpha
 * descriptor or plane, an alpha source of another kind, step or offset or not 4-byte aligned, the alpha source overlapping a
 * destination plane, variant vec_lds.  Variant vec_global where the vector kernel cannot take the layout is LUTR_EINVAL too.
 * Kernels: "k_rgbaf_premul_vec<interp>" (nearest / trilinear / tetrahedral; width a multiple of 4; the four source planes and
 * the three destination planes 16-byte aligned, positive strides), "k_rgbaf_premul_generic" for everything else (one pixel per
 * thread; all five modes); a ragged width on aligned rows is split between the two and named with both.
 * Not covered: a float source with an integer or YUV output (EXR -> yuva444p*). */
int lutr_apply_planar_rgb_f32_premul(lutr_ctx *ctx, int interp, int w, int h, int nframes, const lutr_planes *src,
                                     const lutr_alpha_src *alpha, const lutr_planes *dst, int row0, int rows);

/* ---- precision ---- */
/* STRICT (default): every kernel is a bit-exact restatement of FFmpeg's scalar C lut3d (vf_lut3d.c order of operations,
 * no fused multiply-add in the blend).  FAST: permission to use the tolerance-bounded tile kernels -- lattice staged as
 * fp16 of value * (2^depth - 1), blend as a fused multiply-add chain with fp32 accumulation, truncation as in FFmpeg.
 * Output differs from STRICT by at most ONE code at 8 and at 10 bit (north_star allows 1 / 2 against FFmpeg).  It is
 * used where it applies (fused YUV launches on the LDS-window kernels, LUT depth 8 or 10, lattice inside [0, 1]);
 * everything else runs the strict kernels.  lutr_ctx_last_kernel() names what ran (",fast").
 * FMA32: the strict kernels' fp32 lattice, coordinates, weights, tap selection, truncation and YUV stages; only the blend
 * rounds differently -- nodes pre-multiplied by 2^depth - 1 in fp32 (one rounding each), tetrahedral as
 * fma(w3,c3, fma(w2,c2, fma(w1,c1, w0*c0))), trilinear lerps as fma(b - a, f, a), no final `* M`.  The value before
 * truncation is within a few fp32 ulp of STRICT's, so output differs from STRICT by at most ONE code at every depth.
 * It is used where it applies (fused YUV launches on the LDS-window kernels, LUT depth 8 or 10, lattice inside [0, 1], no
 * prelut, no dither; nearest is identical to STRICT and runs its kernel); everything else runs the strict kernels.
 * lutr_ctx_last_kernel() names what ran (",fma32"). */
enum lutr_precision { LUTR_PRECISION_STRICT = 0, LUTR_PRECISION_FAST = 1, LUTR_PRECISION_FMA32 = 2 };
int lutr_ctx_set_precision(lutr_ctx *ctx, int precision);

/* ---- tuning / introspection (bench and tests) ---- */
/* kernel variant: 0 = auto, 1 = generic (scalar, any layout), 2 = vector + global gather,
 * 3 = vector + LDS lattice window (persistent tile kernels).  Auto picks 3 for launches of 70 Mpx and more
 * (about 8 UHD frames), 2 below that (lower latency), 1 for layouts the vector kernels cannot take; a ragged
 * width on aligned rows is split between 3 and 1.  2 and 3 fail with LUTR_EINVAL on such layouts. */
int lutr_ctx_set_variant(lutr_ctx *ctx, int variant);
/* name of the kernel variant the last apply call launched ("" before the first) */
const char *lutr_ctx_last_kernel(lutr_ctx *ctx);
/* Statistics of the LDS-window tile kernels, accumulated since the previous call.  out[8] (may be
 * NULL) = { tiles, restage attempts (tiles neither the tube nor the wave's window could take), tiles done by the
 * global-gather body, windows staged, 0, 0, tiles served by the workgroup-shared grey tube (no window needed),
 * tiles that needed the exact (second-level) window test }.
 * Then collection is enabled (and zeroed) or disabled. */
int lutr_ctx_tile_stats(lutr_ctx *ctx, int enable, uint64_t out[8]);
/* the constant block the YUV kernels use, for cross-checking against the oracle: 32 floats */
int lutr_yuv_constants(const lutr_yuv_params *p, float out[32]);
/* Host only, for tests: the wave count a persistent tile launcher works with when the environment variable LUTR_MAX_WAVES
 * holds `text` (NULL = unset), its workgroups have `waves_per_block` waves and the device fits `uncapped` of them.  The
 * launchers call the same function: `text` counts only as a plain positive decimal multiple of waves_per_block that is
 * not above `uncapped`; anything else returns `uncapped`. */
int lutr_max_waves_knob(const char *text, int waves_per_block, int uncapped);
/* Host only, for tests: the most workgroups a grid-stride launch whose own cap is `cap` gets when the environment variable
 * LUTR_MAX_BLOCKS holds `text` (NULL = unset).  The launchers call the same function: `text` counts only as a plain positive
 * decimal that fits 31 bits, and then gives min(cap, value); anything else returns `cap`. */
int lutr_max_blocks_knob(const char *text, int cap);

#ifdef __cplusplus
}
#endif
#endif /* LUTR_H */
