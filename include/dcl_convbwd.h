/* dcl_convbwd.h -- C ABI of libdcl_convbwd.so: the backward of a 3x3 / stride 1 / pad 1 convolution y = conv(x, w), x [N, Cin, H, W],
 * y [N, Cout, H, W], as ONE launch.  The grid holds the data-gradient tiles (the interleaved (3, 4) or (3, 2) tile of dcl_conv3x3_f16x3)
 * first and the weight-gradient workgroups (the (3, 1) LDS-DMA kernel of dcl_wgrad3x3_f16x3, flat or wave form) behind them, planned
 * for the compute units the tiles leave free; the slab reduction follows as a second launch.  Both results are those of the separate
 * entries of dcl_hip.h: gx bit for bit, dw bit for bit when the weight gradient is planned for the same workgroup count.
 *
 * Every entry returns 0 on success, a negative DCL_E* code (dcl_hip.h) or a positive hipError_t; dcb_last_error() has the text of
 * the calling thread's last failure.  Tensors are contiguous fp32 NCHW, 16-byte aligned. */
#pragma once
#ifdef __cplusplus
extern "C" {
#endif

int dcb_version(void);
const char *dcb_last_error(void);

/* 1 when the fused launch serves the shape under the automatic plan (host arithmetic only): channel counts in sixteens with
 * Cout % 48 == 0, W % 8 == 0, an automatic data-gradient tile of (3, 4) or (3, 2) whose grid, rounded up to a multiple of 8, leaves
 * at least half of the 256 compute units to the weight gradient.  pre: the weight gradient's operand is relu(x * sc + sh)
 * (dcl_wgrad3x3_pre_f16x3); the shapes served are the same. */
int dcb_supported(int N, int Cin, int Cout, int H, int W, int pre);

/* The plan of a launch, host only.  tile_r / tile_p > 0 force the data-gradient tile (must be (3, 4) or (3, 2)); wg_target: workgroups
 * the weight gradient is planned for -- 0 = automatic (256 - nd8 when that is at least 128, else 256), or a multiple of 8 in
 * [32, 256]; 256 reproduces the plan of dcl_wgrad3x3_f16x3.  out[0 .. 7] = data-gradient workgroups nd, nd rounded up to a multiple
 * of 8 (nd8), weight-gradient workgroups, slabs of `part`, wave form (0 | 1 | 2), tile R, tile P, workgroup target.  Returns 0, or
 * DCL_EUNSUPPORTED for a shape / tile the kernels do not take. */
int dcb_plan(int N, int Cin, int Cout, int H, int W, int tile_r, int tile_p, int wg_target, int *out);

/* slabs of 9 * Cout * Cin floats `part` must hold (0: not served) -- the same plan value the launch uses */
int dcb_wgrad_splits(int N, int Cin, int Cout, int H, int W, int tile_r, int tile_p, int wg_target);

/* gx = data gradient of gy (+ addend, may be NULL), dw = weight gradient.  wpt: w packed for the data gradient (dcl_conv3x3_pack,
 * transposed); gamax / gcount, xamax / xcount: absmax slots of gy and of the weight gradient's operand (x, or relu(x * pre_sc +
 * pre_sh) when pre_sc / pre_sh are given, both or neither); wamax: max |w|. */
int dcb_conv3x3_bwd_f16x3(const float *gy, const void *wpt, const float *x, int N, int Cin, int Cout, int H, int W,
                          const float *gamax, int gcount, const float *wamax, const float *xamax, int xcount,
                          const float *addend, const float *pre_sc, const float *pre_sh, int tile_r, int tile_p, int wg_target,
                          float *gx, float *part, float *dw, void *stream);

#ifdef __cplusplus
}
#endif
