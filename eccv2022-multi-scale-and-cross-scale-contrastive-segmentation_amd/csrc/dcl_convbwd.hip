// dcl_convbwd.hip -- backward of the 3x3 / stride 1 / pad 1 convolution in ONE launch (include/dcl_convbwd.h).
//
// The 192- and 384-channel BasicBlock convolutions of HRNet-W48 run their data gradient as 96 workgroups on 256 compute units by
// choice (DCL_CONV_MIN_WGS, dcl_conv_plan.h: twice the rows per wave, less CU-time) and their weight gradient, from the same autograd
// node and on the same stream, behind it: two independent kernels that both read gy, one after the other.  Here one grid holds both:
// workgroups [0, nd) run the data-gradient tile (conv_body, dcl_conv_body.h), workgroups [nd8, nd8 + G) the weight gradient
// (wgrad3x3d_body, dcl_wgrad3x3d_body.h) with id - nd8 -- nd8 = nd rounded up to a multiple of 8, so that id & 7 is the XCD in both
// decodes; the padding workgroups [nd, nd8) leave at once.  The hardware dispatches in id order: the tiles take their CUs first, the
// weight gradient -- planned for the 256 - nd8 CUs that remain (dcl_convbwd_plan.h) -- fills the rest, and no second queue is
// involved.  Both bodies are the separate kernels' own code, one copy each; they run one workgroup per CU and share one LDS buffer
// of the larger size (120 KiB: the weight gradient's staging rings; the (3, 4) tile's patches take 95.6 KiB).  The slab reduction
// follows as its own launch (dcl_wgrad_reduce.h).
#include "dcl_convbwd_plan.h"
#include "dcl_wgrad3x3d_body.h"
#include "dcl_wgrad_reduce.h"

namespace {

// P: rows per wave of the (3, P) data-gradient tile; WAVE / PRE: the weight gradient's forms (wgrad3x3d_body)
template <int P, bool WAVE, bool PRE>
__global__ __launch_bounds__(256, 1) void k_conv3x3_bwd(ConvArgs c, WgradArgs w, int nd, int nd8)
{
    constexpr int CB = conv_lds_bytes<3, P, 1>(), WB = wgrad3x3d_lds_bytes<3, 1, WAVE>();
    __shared__ __attribute__((aligned(1024))) unsigned char smem[CB > WB ? CB : WB];
    __shared__ float wm[8];
    const int bid = (int)blockIdx.x;
    if (bid < nd)
        conv_body<3, P, 1, 0, true>(c, bid, smem);
    else if (bid >= nd8)
        wgrad3x3d_body<3, 1, WAVE, PRE>(w, (unsigned)(bid - nd8), smem, wm);
}

template <int P>
void launch_bwd(const ConvArgs &c, const WgradArgs &w, const DcbPlan &d, hipStream_t s)
{
    const dim3 grid(d.nd8 + d.w.grid), block(256);
    const int nd = (int)d.nd, nd8 = (int)d.nd8;
    const bool pre = w.pre_sc != nullptr;
    if (d.w.wave_mode) {
        if (pre)
            hipLaunchKernelGGL((k_conv3x3_bwd<P, true, true>), grid, block, 0, s, c, w, nd, nd8);
        else
            hipLaunchKernelGGL((k_conv3x3_bwd<P, true, false>), grid, block, 0, s, c, w, nd, nd8);
    } else {
        if (pre)
            hipLaunchKernelGGL((k_conv3x3_bwd<P, false, true>), grid, block, 0, s, c, w, nd, nd8);
        else
            hipLaunchKernelGGL((k_conv3x3_bwd<P, false, false>), grid, block, 0, s, c, w, nd, nd8);
    }
}

}  // namespace

extern "C" int dcb_conv3x3_bwd_f16x3(const float *gy, const void *wpt, const float *x, int N, int Cin, int Cout, int H, int W,
                                     const float *gamax, int gcount, const float *wamax, const float *xamax, int xcount,
                                     const float *addend, const float *pre_sc, const float *pre_sh, int tile_r, int tile_p, int wg_target,
                                     float *gx, float *part, float *dw, void *stream)
{
    DCL_CHECK_ARG(gy && wpt && x && gamax && wamax && xamax && gx && part && dw, "null pointer");
    DCL_CHECK_ARG(N > 0 && Cin > 0 && Cout > 0 && H > 0 && W > 0 && gcount > 0 && xcount > 0, "bad shape");
    DCL_CHECK_ARG((pre_sc == nullptr) == (pre_sh == nullptr), "pre_sc and pre_sh: both or neither");
    DCL_CHECK_ARG(((((uintptr_t)x) | ((uintptr_t)gy) | ((uintptr_t)wpt)) & 15) == 0, "tensors must be 16-byte aligned");
    DCL_CHECK_ARG(((((uintptr_t)pre_sc) | ((uintptr_t)pre_sh)) & 3) == 0, "tables must be 4-byte aligned");
    const DcbPlan d = dcb_make_plan(N, Cin, Cout, H, W, tile_r, tile_p, wg_target);
    if (!d.ok) {
        dcb_set_error("dcb_conv3x3_bwd_f16x3: shape, tile or workgroup target not taken (dcb_supported, dcb_plan)");
        return DCL_EUNSUPPORTED;
    }
    // data gradient: gx [N, Cin, H, W] = conv3x3(gy [N, Cout, H, W], wpt) + addend
    ConvArgs c;
    conv_fill_args(c, gy, N, Cout, H, W, wpt, Cin, gamax, gcount, wamax, addend, nullptr, gx, nullptr, nullptr);
    if (conv_fill_grid(c, d.R, d.P) != d.nd) {
        dcb_set_error("dcb_conv3x3_bwd_f16x3: plan and tile grid disagree");
        return DCL_EINVAL;
    }
    WgradArgs w;
    wgrad_fill_args(w, d.w, x, gy, part, xamax, xcount, gamax, gcount, N, Cin, Cout, H, W, 1, pre_sc, pre_sh);
    hipStream_t s = (hipStream_t)stream;
    if (d.P == 4)
        launch_bwd<4>(c, w, d, s);
    else
        launch_bwd<2>(c, w, d, s);
    DCL_LAUNCH_CHECK();
    launch_wgrad_reduce(part, d.w.slabs, Cout, Cin, dw, s);
    DCL_LAUNCH_CHECK();
    return 0;
}
