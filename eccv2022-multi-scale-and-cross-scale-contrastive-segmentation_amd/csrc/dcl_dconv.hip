// dcl_dconv.hip -- device half of libdcl_dconv.so (include/dcl_dconv.h): the dilated 3x3 convolution, forward / data gradient (one
// kernel, k_dconv) and weight gradient (k_dwgrad + k_dwgrad_sum), on v_mfma_f32_32x32x16_f16 with split-f16 operands.
//
// Operand layout of the instruction (lane l: r = l & 31, h = l >> 5): A[row r][k = 8 h + j] and B[k = 8 h + j][col r] in element
// j = 0..7 of the lane's fragment; result register g of lane l is C[row (g & 3) + 8 (g >> 2) + 4 h][col r].
//   k_dconv    A = weights (rows: output channels; ddc_pack wrote the fragments lane by lane), B = x (cols: 32 pixels of the wave,
//              k: 16 input channels).  A lane loads the eight channels of ITS pixel, shifted by the tap, zero outside the image:
//              for d > 1 the taps share no halo, so nothing is staged through LDS and the kernel has no barrier.
//   k_dwgrad   A = dy (rows: output channels, k: 16 consecutive pixels), B = x shifted by the tap (cols: input channels).
// No kernel here stores or loads outside the tensors it is given: every load is predicated on its own row / pixel test.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <initializer_list>

#include "dcl_f16x3.h"
#include "dcl_dconv_plan.h"

namespace {

constexpr int NTHR = 256;

#define DMFMA(A, B, C) __builtin_amdgcn_mfma_f32_32x32x16_f16(as_half8(A), as_half8(B), (C), 0, 0, 0)

// max over the bit patterns of |x| (non-negative floats order as unsigned integers; a NaN ends up on top and poisons the scale)
__global__ __launch_bounds__(NTHR) void k_absmax(const float *__restrict__ x, int64_t n, unsigned *slot)
{
    unsigned m = 0;
    for (int64_t i = (int64_t)blockIdx.x * NTHR + threadIdx.x; i < n; i += (int64_t)gridDim.x * NTHR) {
        const unsigned b = __float_as_uint(x[i]) & 0x7fffffffu;
        m = b > m ? b : m;
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        const unsigned t = (unsigned)__shfl_xor((int)m, o, 64);
        m = t > m ? t : m;
    }
    if ((threadIdx.x & 63) == 0 && m != 0)
        atomicMax(slot, m);
}

// one thread per lane of one fragment: [tap][row tile][chunk][hi, lo][lane] x 16 bytes
__global__ __launch_bounds__(NTHR) void k_pack(const float *__restrict__ w, int Co, int Ci, const float *__restrict__ wamax,
                                                u32x4 *__restrict__ wp, int transposed)
{
    const int rows = transposed ? Ci : Co, cols = transposed ? Co : Ci;
    const int RT = (rows + 31) / 32, CH = cols / 16;
    const int64_t total = 9ll * RT * CH * 64;
    const int64_t idx = (int64_t)blockIdx.x * NTHR + threadIdx.x;
    if (idx >= total)
        return;
    const int lane = (int)(idx & 63);
    int64_t f = idx >> 6;
    const int ch = (int)(f % CH);
    f /= CH;
    const int rt = (int)(f % RT), tap = (int)(f / RT);
    const float s = pow2_scale(wamax[0]);
    const int r = lane & 31, h = lane >> 5, row = rt * 32 + r;
    const int src_tap = transposed ? 8 - tap : tap;
    float v[8];
#pragma unroll
    for (int j = 0; j < 8; ++j) {
        const int col = ch * 16 + 8 * h + j;
        const int co = transposed ? col : row, ci = transposed ? row : col;
        v[j] = row < rows ? w[((int64_t)co * Ci + ci) * 9 + src_tap] : 0.f;
    }
    u32x4 hi, lo;
    split8(v, s, hi, lo);
    const size_t o = ((size_t)(tap * RT + rt) * CH + ch) * 128;
    wp[o + lane] = hi;
    wp[o + 64 + lane] = lo;
}

struct ConvArgs {
    const float *x;          // [N, Ci, H, W]  (the data gradient: dy, and Ci / Co swapped by the caller)
    const u32x4 *wp;         // fragments: rows = Co of this launch
    const float *wamax;
    const unsigned *xamax;
    const float *bias;       // [Co] or null
    float *y;                // [N, Co, H, W]
    int Ci, Co, H, W, d;
    unsigned live;
};

__global__ __launch_bounds__(NTHR) void k_dconv(ConvArgs a)
{
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int r = lane & 31, h = lane >> 5;
    const int HW = a.H * a.W;
    const int wp0 = blockIdx.x * DDC_TILE_P + wave * 32;
    if (wp0 >= HW)              // wave-uniform; the kernel has no barrier
        return;
    const int n = blockIdx.y, co0 = blockIdx.z * DDC_TILE_CO;
    const int p = wp0 + r;
    const bool pin = p < HW;
    const int py = pin ? p / a.W : 0, px = pin ? p - py * a.W : 0;
    const int RT = (a.Co + 31) / 32, CH = a.Ci / DDC_CHUNK_CI, rt0 = co0 / 32;
    const bool second = rt0 + 1 < RT;
    const float sx = pow2_scale(__uint_as_float(a.xamax[0])), sw = pow2_scale(a.wamax[0]);
    const float *xn = a.x + (size_t)n * a.Ci * HW;
    f32x16 acc0 = {0}, acc1 = {0};
    for (int tap = 0; tap < 9; ++tap) {
        if (!((a.live >> tap) & 1))
            continue;
        const int yy = py + (tap / 3 - 1) * a.d, xx = px + (tap % 3 - 1) * a.d;
        const bool valid = pin && yy >= 0 && yy < a.H && xx >= 0 && xx < a.W;
        if (__ballot(valid) == 0)       // the wave's shifted window lies wholly outside the image
            continue;
        const int q = valid ? yy * a.W + xx : 0;
        const u32x4 *wt = a.wp + ((size_t)(tap * RT + rt0) * CH) * 128 + lane;
        for (int ch = 0; ch < CH; ++ch) {
            const float *xc = xn + (size_t)(ch * DDC_CHUNK_CI + 8 * h) * HW + q;
            float v[8];
#pragma unroll
            for (int j = 0; j < 8; ++j)
                v[j] = valid ? xc[(size_t)j * HW] : 0.f;
            u32x4 bhi, blo;
            split8(v, sx, bhi, blo);
            split_to_mfma_pad(bhi, blo);
            const u32x4 ahi = wt[(size_t)ch * 128], alo = wt[(size_t)ch * 128 + 64];
            acc0 = DMFMA(ahi, bhi, acc0);
            acc0 = DMFMA(ahi, blo, acc0);
            acc0 = DMFMA(alo, bhi, acc0);
            if (second) {
                const u32x4 chi = wt[(size_t)(CH + ch) * 128], clo = wt[(size_t)(CH + ch) * 128 + 64];
                acc1 = DMFMA(chi, bhi, acc1);
                acc1 = DMFMA(chi, blo, acc1);
                acc1 = DMFMA(clo, bhi, acc1);
            }
        }
    }
    if (!pin)
        return;
    const float isx = 1.f / sx, isw = 1.f / sw;
    float *yn = a.y + (size_t)n * a.Co * HW + p;
#pragma unroll
    for (int g = 0; g < 16; ++g) {
        const int co = co0 + (g & 3) + 8 * (g >> 2) + 4 * h;
        if (co < a.Co)
            yn[(size_t)co * HW] = acc0[g] * isx * isw + (a.bias ? a.bias[co] : 0.f);
        const int c2 = co + 32;
        if (second && c2 < a.Co)
            yn[(size_t)c2 * HW] = acc1[g] * isx * isw + (a.bias ? a.bias[c2] : 0.f);
    }
}

struct WgArgs {
    const float *x, *dy;
    const unsigned *xamax, *dyamax;
    float *part;             // [slabs][live][Co][Ci]
    int Ci, Co, H, W, d;
    unsigned live;
    int nlive, units_per_image;
    long long units, per;    // all units, units of one slab
};

__global__ __launch_bounds__(64) void k_dwgrad(WgArgs a)
{
    const int lane = threadIdx.x, r = lane & 31, h = lane >> 5;
    const int HW = a.H * a.W;
    const int cit = (a.Ci + DDC_WG_TILE - 1) / DDC_WG_TILE;
    const int co0 = (blockIdx.x / cit) * DDC_WG_TILE, ci0 = (blockIdx.x % cit) * DDC_WG_TILE;
    int tap = 0;
    for (int seen = -1; tap < 9; ++tap)
        if ((a.live >> tap) & 1)
            if (++seen == (int)blockIdx.y)
                break;
    const int sy = (tap / 3 - 1) * a.d, sxo = (tap % 3 - 1) * a.d;
    const long long u0 = (long long)blockIdx.z * a.per;
    const long long u1 = u0 + a.per < a.units ? u0 + a.per : a.units;
    const float sdy = pow2_scale(__uint_as_float(a.dyamax[0])), sxs = pow2_scale(__uint_as_float(a.xamax[0]));
    const bool corow = co0 + r < a.Co, cirow = ci0 + r < a.Ci;
    f32x16 acc = {0};
    for (long long u = u0; u < u1; ++u) {
        const int n = (int)(u / a.units_per_image);
        const int pu = (int)(u - (long long)n * a.units_per_image) * DDC_WG_CHUNK_P + 8 * h;
        const float *dyr = a.dy + ((size_t)n * a.Co + (corow ? co0 + r : 0)) * HW;
        const float *xr = a.x + ((size_t)n * a.Ci + (cirow ? ci0 + r : 0)) * HW;
        int y = pu / a.W, xq = pu - y * a.W;
        float va[8], vb[8];
#pragma unroll
        for (int j = 0; j < 8; ++j) {
            const int p = pu + j;
            const bool in = p < HW;
            va[j] = (in && corow) ? dyr[p] : 0.f;
            const int yy = y + sy, xx = xq + sxo;
            const bool ok = in && cirow && yy >= 0 && yy < a.H && xx >= 0 && xx < a.W;
            vb[j] = ok ? xr[yy * a.W + xx] : 0.f;
            if (++xq == a.W) {
                xq = 0;
                ++y;
            }
        }
        u32x4 ahi, alo, bhi, blo;
        split8(va, sdy, ahi, alo);
        split8(vb, sxs, bhi, blo);
        acc = DMFMA(ahi, bhi, acc);
        acc = DMFMA(ahi, blo, acc);
        acc = DMFMA(alo, bhi, acc);
    }
    const int ci = ci0 + r;
    if (ci >= a.Ci)
        return;
    float *out = a.part + ((size_t)blockIdx.z * a.nlive + blockIdx.y) * a.Co * a.Ci + ci;
#pragma unroll
    for (int g = 0; g < 16; ++g) {
        const int co = co0 + (g & 3) + 8 * (g >> 2) + 4 * h;
        if (co < a.Co)
            out[(size_t)co * a.Ci] = acc[g];
    }
}

// dw[co][ci][tap] = the slabs' partials added in index order, unscaled; exact zeros on dead taps
__global__ __launch_bounds__(NTHR) void k_dwgrad_sum(const float *__restrict__ part, const unsigned *xamax, const unsigned *dyamax,
                                                      int CoCi, unsigned live, int nlive, int slabs, float *__restrict__ dw)
{
    const int e = blockIdx.x * NTHR + threadIdx.x;
    if (e >= CoCi * 9)
        return;
    const int tap = e % 9, cc = e / 9;
    if (!((live >> tap) & 1)) {
        dw[e] = 0.f;
        return;
    }
    const int li = __popc(live & ((1u << tap) - 1));
    float s = 0.f;
    for (int k = 0; k < slabs; ++k)
        s += part[((size_t)k * nlive + li) * CoCi + cc];
    const float isx = 1.f / pow2_scale(__uint_as_float(xamax[0])), isd = 1.f / pow2_scale(__uint_as_float(dyamax[0]));
    dw[e] = s * isx * isd;
}

int launched(const char *what)
{
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess) {
        ddc_set_error("%s: launch failed: %s", what, hipGetErrorString(e));
        return (int)e;
    }
    return DDC_OK;
}

bool aligned16(std::initializer_list<const void *> ps)
{
    for (const void *p : ps)
        if (!p || (uintptr_t)p % 16 != 0)
            return false;
    return true;
}

// x, dy, y, dx, dw and the bias are read and written one float at a time: any float tensor will do
bool aligned4(std::initializer_list<const void *> ps)
{
    for (const void *p : ps)
        if (!p || (uintptr_t)p % 4 != 0)
            return false;
    return true;
}

int common_args(int op, int N, int Ci, int Co, int H, int W, int d, const void *ws, int64_t ws_bytes, bool tensors_ok,
                const char *what)
{
    const int64_t need = ddc_ws_bytes(op, N, Ci, Co, H, W, d);
    if (need < 0) {
        ddc_set_error("%s: shape not taken (ddc_supported)", what);
        return DDC_EINVAL;
    }
    if (!tensors_ok) {
        ddc_set_error("%s: a tensor is null, or fragments not 16-byte aligned", what);
        return DDC_EINVAL;
    }
    if (ws_bytes < need) {
        ddc_set_error("%s: workspace of %lld bytes, %lld needed", what, (long long)ws_bytes, (long long)need);
        return DDC_EINVAL;
    }
    if (!ws || (uintptr_t)ws % 256 != 0) {
        ddc_set_error("%s: the workspace must be 256-byte aligned", what);
        return DDC_EINVAL;
    }
    return DDC_OK;
}

// slot[0] = max|x| over n floats (the slot is cleared first, on the stream)
int absmax_into(const float *x, int64_t n, unsigned *slot, hipStream_t st, const char *what)
{
    const hipError_t e = hipMemsetAsync(slot, 0, sizeof(unsigned), st);
    if (e != hipSuccess) {
        ddc_set_error("%s: hipMemsetAsync: %s", what, hipGetErrorString(e));
        return (int)e;
    }
    int64_t blocks = (n + 4 * NTHR - 1) / (4 * NTHR);
    if (blocks > 2048)
        blocks = 2048;
    hipLaunchKernelGGL(k_absmax, dim3((unsigned)blocks), dim3(NTHR), 0, st, x, n, slot);
    return launched(what);
}

// the forward of (x, fragments with `Co` rows): shared by ddc_fwd and ddc_dgrad
int conv_launch(const float *x, const void *wp, const float *wamax, const float *bias, int N, int Ci, int Co, int H, int W, int d,
                void *ws, float *y, hipStream_t st, const char *what)
{
    unsigned *slot = (unsigned *)ws;
    int rc = absmax_into(x, (int64_t)N * Ci * H * W, slot, st, what);
    if (rc != DDC_OK)
        return rc;
    ConvArgs a{x, (const u32x4 *)wp, wamax, slot, bias, y, Ci, Co, H, W, d, ddc_live_mask(H, W, d)};
    const dim3 grid((unsigned)ddc_ceil_div(H * W, DDC_TILE_P), (unsigned)N, (unsigned)ddc_ceil_div(Co, DDC_TILE_CO));
    hipLaunchKernelGGL(k_dconv, grid, dim3(NTHR), 0, st, a);
    return launched(what);
}

}  // namespace

extern "C" int ddc_pack(const float *w, int Co, int Ci, float *wamax, void *wp, void *wpt, void *stream)
{
    if (ddc_pack_bytes(Co, Ci, 0) < 0) {
        ddc_set_error("%s: channel counts not taken (ddc_packed_bytes)", __func__);
        return DDC_EINVAL;
    }
    if (!wamax || !aligned4({w}) || !aligned16({wp, wpt})) {
        ddc_set_error("%s: a tensor is null, or fragments not 16-byte aligned", __func__);
        return DDC_EINVAL;
    }
    hipStream_t st = (hipStream_t)stream;
    int rc = absmax_into(w, 9ll * Co * Ci, (unsigned *)wamax, st, __func__);
    if (rc != DDC_OK)
        return rc;
    for (int tr = 0; tr < 2; ++tr) {
        const int64_t lanes = ddc_pack_bytes(Co, Ci, tr) / 32;      // one thread writes a hi and a lo fragment row: 32 bytes
        hipLaunchKernelGGL(k_pack, dim3((unsigned)((lanes + NTHR - 1) / NTHR)), dim3(NTHR), 0, st, w, Co, Ci, (const float *)wamax,
                           (u32x4 *)(tr ? wpt : wp), tr);
        if ((rc = launched(__func__)) != DDC_OK)
            return rc;
    }
    return DDC_OK;
}

extern "C" int ddc_fwd(const float *x, const void *wp, const float *wamax, const float *bias, int N, int Ci, int Co, int H, int W,
                       int d, void *workspace, int64_t workspace_bytes, float *y, void *stream)
{
    const int rc = common_args(DDC_OP_FWD, N, Ci, Co, H, W, d, workspace, workspace_bytes, wamax && aligned4({x, y}) && aligned16({wp}), __func__);
    if (rc != DDC_OK)
        return rc;
    return conv_launch(x, wp, wamax, bias, N, Ci, Co, H, W, d, workspace, y, (hipStream_t)stream, __func__);
}

extern "C" int ddc_dgrad(const float *dy, const void *wpt, const float *wamax, int N, int Ci, int Co, int H, int W, int d,
                         void *workspace, int64_t workspace_bytes, float *dx, void *stream)
{
    const int rc = common_args(DDC_OP_DGRAD, N, Ci, Co, H, W, d, workspace, workspace_bytes, wamax && aligned4({dy, dx}) && aligned16({wpt}), __func__);
    if (rc != DDC_OK)
        return rc;
    return conv_launch(dy, wpt, wamax, nullptr, N, Co, Ci, H, W, d, workspace, dx, (hipStream_t)stream, __func__);
}

extern "C" int ddc_wgrad(const float *x, const float *dy, int N, int Ci, int Co, int H, int W, int d, void *workspace,
                         int64_t workspace_bytes, float *dw, void *stream)
{
    int rc = common_args(DDC_OP_WGRAD, N, Ci, Co, H, W, d, workspace, workspace_bytes, aligned4({x, dy, dw}), __func__);
    if (rc != DDC_OK)
        return rc;
    hipStream_t st = (hipStream_t)stream;
    unsigned *xslot = (unsigned *)workspace, *dslot = (unsigned *)((char *)workspace + 256);
    float *part = (float *)((char *)workspace + 512);
    if ((rc = absmax_into(x, (int64_t)N * Ci * H * W, xslot, st, __func__)) != DDC_OK)
        return rc;
    if ((rc = absmax_into(dy, (int64_t)N * Co * H * W, dslot, st, __func__)) != DDC_OK)
        return rc;
    const unsigned live = ddc_live_mask(H, W, d);
    const int nlive = ddc_popcount9(live), slabs = ddc_slab_count(N, Ci, Co, H, W, d);
    const long long units = ddc_wgrad_units(N, H, W), per = ddc_slab_units(N, Ci, Co, H, W, d);
    WgArgs a{x, dy, xslot, dslot, part, Ci, Co, H, W, d, live, nlive, (int)(units / N), units, per};
    const dim3 grid((unsigned)(ddc_ceil_div(Co, DDC_WG_TILE) * ddc_ceil_div(Ci, DDC_WG_TILE)), (unsigned)nlive, (unsigned)slabs);
    hipLaunchKernelGGL(k_dwgrad, grid, dim3(64), 0, st, a);
    if ((rc = launched(__func__)) != DDC_OK)
        return rc;
    const int E = 9 * Co * Ci;
    hipLaunchKernelGGL(k_dwgrad_sum, dim3((unsigned)((E + NTHR - 1) / NTHR)), dim3(NTHR), 0, st, (const float *)part,
                       (const unsigned *)xslot, (const unsigned *)dslot, Co * Ci, live, nlive, slabs, dw);
    return launched(__func__);
}
