/* C ABI of libdcl_dconv.so: the dilated 3x3 convolution of DeepLabv3 (the ASPP branches and the ResNet layers whose stride was
 * replaced by dilation) on gfx950 kernels: forward, data gradient and weight gradient.
 *
 * A fifth, small library next to the main one, with its own prefix (ddc_) and its own binding module (_lib_dconv.py).
 * Every device entry launches on `stream`, never waits for the device, never reads a result back, uses no floating-point
 * atomics and gives bitwise the same result from run to run.
 *
 * Operator:  y = conv2d(x, w, bias, stride 1, padding d, dilation d), groups 1.  All tensors f32, contiguous:
 *   x [N, Ci, H, W]    w [Co, Ci, 3, 3]    bias [Co] or null    y [N, Co, H, W]
 * Tap (ky, kx) reads x at offset ((ky - 1) d, (kx - 1) d); outside the image it reads zero.
 *
 * Arithmetic: split f16 ("f16x3").  An operand v becomes hi = f16(v s) and lo = f16(v s - hi) with a power-of-two scale s from the
 * tensor's absmax; a product is hi.hi + hi.lo + lo.hi on v_mfma_f32_32x32x16_f16 with f32 accumulation.  The absmax of x, dy and
 * w is computed on the device by this library (a maximum over the bit patterns of non-negative floats, as integer atomics).
 *
 * Live taps: a tap is dead for the whole image when ky != 1 and d >= H, or kx != 1 and d >= W; the host computes the mask once per
 * launch (ddc_live_taps).  Dead taps are never loaded or multiplied; in the weight gradient they get exact zeros.  A wave also
 * skips a live tap whose shifted window lies wholly outside the image for all of its 32 pixels (one ballot: wave-uniform).
 *
 * Forward and data gradient are one kernel, an implicit GEMM per live tap: a workgroup of 4 waves owns DDC_TILE_CO output channels
 * of DDC_TILE_P pixels of one image (a wave: DDC_TILE_CO x 32 pixels), K = input channels in chunks of DDC_CHUNK_CI.  The weights
 * come as fragments written by ddc_pack; every lane loads its own shifted pixel of the chunk's channels (zero outside the image)
 * and splits it in registers.  The data gradient is the same convolution of dy with the transposed, tap-mirrored fragments.
 *
 * Weight gradient: dW[co, ci, tap] = sum over n, p of dy[n, co, p] x[n, ci, p + off(tap)].  A wave owns a DDC_WG_TILE x DDC_WG_TILE
 * tile of (co, ci) for one live tap and one slab; the pixels of all images, in units of DDC_WG_CHUNK_P, are cut into
 * ddc_wgrad_slabs consecutive slabs.  Each slab's partial goes to the workspace; a second kernel adds the slabs in index order. */
#ifndef DDC_DCONV_H
#define DDC_DCONV_H
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define DDC_OK 0
#define DDC_EINVAL 1
#define DDC_TILE_P 128       /* pixels of one workgroup's tile (forward / data gradient) */
#define DDC_TILE_CO 64       /* output channels of one workgroup's tile */
#define DDC_CHUNK_CI 16      /* input channels of one accumulation step */
#define DDC_WG_TILE 32       /* weight gradient: output and input channels of one wave's tile */
#define DDC_WG_CHUNK_P 16    /* weight gradient: pixels of one accumulation step (a "unit") */
#define DDC_MAX_SLABS 64     /* weight gradient: most slabs */
#define DDC_SLAB_MIN_UNITS 32 /* weight gradient: a slab is not planned shorter than this many units */
#define DDC_WG_TARGET 2048   /* weight gradient: waves a launch aims at */
#define DDC_MAX_C 4096
#define DDC_MAX_D 64
#define DDC_MAX_N 65535      /* the batch is a launch's grid y dimension */

#define DDC_OP_FWD 0
#define DDC_OP_DGRAD 1
#define DDC_OP_WGRAD 2

int ddc_version(void);
const char *ddc_last_error(void);

/* Host only (no device is touched): 1 when the kernels take the shape, else 0.  Taken: Ci % 16 == 0 and Co % 16 == 0,
 * 16 <= Ci, Co <= DDC_MAX_C, 1 <= d <= DDC_MAX_D, H, W >= 1, 1 <= N <= DDC_MAX_N, and every tensor (N Ci H W, N Co H W, 9 Co Ci)
 * under 2^31 elements. */
int ddc_supported(int N, int Ci, int Co, int H, int W, int d);

/* Host only.  Bit 3 ky + kx is set when tap (ky, kx) is live: ky == 1 or d < H, and kx == 1 or d < W.  0 for H, W or d < 1. */
unsigned ddc_live_taps(int H, int W, int d);

/* Host only.  The number of slabs of the weight gradient, from the shape alone: with units = N ceil(H W / DDC_WG_CHUNK_P),
 * tiles = ceil(Co / DDC_WG_TILE) ceil(Ci / DDC_WG_TILE) live,
 *   want = min(max(1, ceil(DDC_WG_TARGET / tiles)), DDC_MAX_SLABS, max(1, units / DDC_SLAB_MIN_UNITS)),
 *   per = ceil(units / want),  slabs = ceil(units / per):  none is empty.  0 for a shape ddc_supported refuses. */
int ddc_wgrad_slabs(int N, int Ci, int Co, int H, int W, int d);

/* Host only.  Bytes of workspace of one entry, with r(x) = x rounded up to 256:
 *   DDC_OP_FWD, DDC_OP_DGRAD   256                                   the absmax slot of x / dy
 *   DDC_OP_WGRAD               512 + r(4 slabs live Co Ci)           two absmax slots, then the partial of every slab
 * Returns -1 for an unknown op or a shape ddc_supported refuses. */
int64_t ddc_workspace_bytes(int op, int N, int Ci, int Co, int H, int W, int d);

/* Host only.  Bytes of one orientation of the packed weights: 9 taps x ceil(rows / 32) row tiles x (cols / 16) chunks x {hi, lo} x
 * 64 lanes x 16 bytes = 36 ceil32(rows) cols, with (rows, cols) = (Co, Ci) for the forward and (Ci, Co) for the data gradient
 * (transposed != 0).  -1 unless both are multiples of 16 in [16, DDC_MAX_C]. */
int64_t ddc_packed_bytes(int Co, int Ci, int transposed);

/* Every device entry: the packed fragments 16-byte aligned, every other tensor as any float array (they are read and written one
 * float at a time, so a contiguous view at an odd storage offset is taken); workspace of at least ddc_workspace_bytes(op, ...) bytes, 256-byte aligned, contents
 * on entry do not matter; a smaller one is refused before anything is launched.  Outputs are written completely. */

/* wamax[0] = max|w|, and both orientations of the hi / lo fragments of w scaled by pow2_scale(wamax): wp for ddc_fwd
 * (ddc_packed_bytes(Co, Ci, 0)), wpt for ddc_dgrad (ddc_packed_bytes(Co, Ci, 1); weights transposed, taps mirrored).  All nine
 * taps are packed, so one pack serves every map size and dilation.  Rows past the channel count are written as zeros. */
int ddc_pack(const float *w, int Co, int Ci, float *wamax, void *wp, void *wpt, void *stream);

/* y from x, the forward fragments and their absmax; bias may be null. */
int ddc_fwd(const float *x, const void *wp, const float *wamax, const float *bias, int N, int Ci, int Co, int H, int W, int d,
            void *workspace, int64_t workspace_bytes, float *y, void *stream);

/* dx [N, Ci, H, W] from dy [N, Co, H, W] and the data-gradient fragments; Ci and Co are the forward's. */
int ddc_dgrad(const float *dy, const void *wpt, const float *wamax, int N, int Ci, int Co, int H, int W, int d, void *workspace,
              int64_t workspace_bytes, float *dx, void *stream);

/* dw [Co, Ci, 3, 3] from x and dy. */
int ddc_wgrad(const float *x, const float *dy, int N, int Ci, int Co, int H, int W, int d, void *workspace,
              int64_t workspace_bytes, float *dw, void *stream);

#ifdef __cplusplus
}
#endif
#endif
