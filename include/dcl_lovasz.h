/* C ABI of libdcl_lovasz.so: the Lovasz-Softmax loss (Berman et al., CVPR 2018) on gfx950 kernels.
 *
 * A second, small library next to the main one, with its own prefix (dlv_) and its own binding module
 * (_lib_lovasz.py).  Semantics: losses/LovaszSoftmax.py.  Every device entry launches on `stream`, never waits for
 * the device, uses no float atomics and gives bitwise the same result from run to run.
 *
 * A SEGMENT is one class (per_image = 0: S = C segments of L = N*HW pixels) or one (image, class) pair (per_image = 1:
 * S = N*C segments of L = HW pixels).  Per segment: e = |fg - softmax_k|, sorted descending with a stable LSD radix sort
 * (4 passes of 8 bits over the fp32 bits of e, which are order preserving for e in [0, 1]), an exact integer prefix
 * count of the foreground in sorted order, the Jaccard step in its cancellation-free form (fp64), and the dot product
 * in fp64 partials summed in a fixed order.  Pixels whose label is the ignore id stay in place with e = 0 and fg = 0:
 * they sort last, add nothing, shift no other element's step, and get a zero coefficient. */
#ifndef DLV_LOVASZ_H
#define DLV_LOVASZ_H
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define DLV_OK 0
#define DLV_EINVAL 1
#define DLV_MAX_CLASSES 256
#define DLV_TILE 4096 /* elements of one segment that one workgroup sorts / scans */

int dlv_version(void);
const char *dlv_last_error(void);

/* Host only.  Bytes of workspace dlv_lovasz_fwd needs, with T = N*C*HW elements, S segments of L elements (above),
 * tps = ceil(L / DLV_TILE) tiles per segment and r(x) = x rounded up to 256:
 *
 *   4 * r(4 T)              key and payload, ping and pong           (the 2 x 8 B x T of the sort)
 * + r(4 * 256 * S * tps)    digit histograms of one pass, [S][256][tps]
 * + r(4 * 256 * S)          digit totals per segment
 * + r(4 * S * tps)          foreground counts per tile
 * + r(8 * S * tps)          fp64 partial terms per tile
 * + 3 * r(8 * S)            foreground totals, term weights, weighted terms per segment
 *
 * All classes are sorted at once (no chunking).  Returns -1 on arguments dlv_lovasz_fwd would refuse. */
int64_t dlv_workspace_bytes(int N, int C, int HW, int per_image);

/* Forward.
 *   logits     f32 [N, C, HW] (NCHW contiguous)
 *   labels     int64 | int32 | uint8 [N, HW] (label_bytes = 8 | 4 | 1)
 *   has_ignore / ignore   pixels with label == ignore are dropped (has_ignore = 0: none are)
 *   present_only   1: a class without foreground in its segment's pixels gives no term ('present'); 0: every considered one
 *   consider   uint8 [C] on the device, non-zero = the class is considered; NULL = all classes
 *   workspace  workspace_bytes >= dlv_workspace_bytes(...) bytes, 256-byte aligned; contents on entry do not matter
 *   coef       f32 [N, C, HW] out: d loss / d softmax_k at every pixel (0 at ignored pixels), kept for dlv_lovasz_bwd
 *   loss       f32 [1] out: mean over the terms (per image, then over the N images, with per_image); 0 without terms
 * Requires 1 <= C <= DLV_MAX_CLASSES, N*HW < 2^31, N*C*HW < 2^31. */
int dlv_lovasz_fwd(const float *logits, const void *labels, int label_bytes, int N, int C, int HW, int per_image,
                   int has_ignore, int ignore, int present_only, const uint8_t *consider, void *workspace,
                   int64_t workspace_bytes, float *coef, float *loss, void *stream);

/* Backward: one element-wise pass that recomputes the softmax p,
 *   dlogits[n, j, x] = upstream[0] * p_j * (coef_j - sum_k coef_k p_k).
 *   upstream   f32 [1] on the device        dlogits   f32 [N, C, HW] out */
int dlv_lovasz_bwd(const float *logits, const float *coef, const float *upstream, int N, int C, int HW, float *dlogits,
                   void *stream);

#ifdef __cplusplus
}
#endif
#endif
