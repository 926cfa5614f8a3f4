// dcl_tsne.hip -- exact t-SNE on gfx950 (include/dcl_tsne.h): the algorithm of van der Maaten's tsne.py, which the reference's
// demo_tsne mode runs through tsne_torch in eager torch, about ten N x N tensors per iteration.  Here P [N, N] is the only N x N
// buffer, and an iteration reads it once.
//
//   k_cond_p     one workgroup per row: the row's squared distances (difference form, an FMA chain over the dimensions) go to LDS,
//                or above DTS_LDS_ROW points to the row of P itself, where thread t reads back and finally overwrites only the
//                entries t wrote; the search for beta is the workgroup's: two sums per try, every thread takes the same branch.
//   k_sym        a workgroup owns a 32 x 32 tile and its mirror tile (both read into LDS before either is written); run twice:
//                once for the partial sums of P + P^T, once to write (P + P^T) / sum.  a + b == b + a makes the result symmetric
//                bitwise.
//   k_zsum       partial sums of num = 1 / (1 + |y_i - y_j|^2) over a 256-row x 1024-column block, the columns' points in LDS;
//                num is symmetric bitwise, so the blocks below the diagonal are skipped and those above it count twice.
//   k_gradient   a workgroup owns DTS_GRAD_ROWS whole rows of P and streams them, 256 threads x 4 columns at a step (16-byte
//                loads when the rows start on 16 bytes); a step's points y_j are loaded once and serve all the rows.  Whole rows:
//                dY needs no second stage.  With KL the same pass leaves the workgroup's partial of sum p log(p / q).
//   k_update     gains, momentum, step, and the partial column sums of the new Y; block 0 sums the KL partials first.
//   k_center     Y -= column means.
//
// Sums across workgroups: the producer writes one partial per workgroup, the consumer adds them at its head, thread-strided and
// then by the fixed tree of block_sum: the same order in every workgroup and in every run.  No atomics, no flags.
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

#include "dcl_tsne_plan.h"

namespace {

constexpr int NTHR = 256;
constexpr int NWAVE = NTHR / 64;
constexpr int GR = DTS_GRAD_ROWS;

__device__ __forceinline__ float wave_sum(float v)
{
#pragma unroll
    for (int o = 32; o > 0; o >>= 1)
        v += __shfl_down(v, o, 64);
    return v;                                                      // (lane 0)
}

__device__ __forceinline__ float wave_min(float v)
{
#pragma unroll
    for (int o = 32; o > 0; o >>= 1)
        v = fminf(v, __shfl_down(v, o, 64));
    return v;
}

// The workgroup's sum, handed to every thread.  s: NWAVE floats; the caller keeps a barrier between the last read here and the next
// write to the same s (or alternates between two of them).
__device__ __forceinline__ float block_sum(float v, float *s)
{
    v = wave_sum(v);
    if ((threadIdx.x & 63) == 0)
        s[threadIdx.x >> 6] = v;
    __syncthreads();
    return (s[0] + s[1]) + (s[2] + s[3]);
}

// sum of part[0, n) in an order that depends on n alone
__device__ __forceinline__ float sum_parts(const float *__restrict__ part, int n, float *s)
{
    float v = 0.f;
    for (int k = threadIdx.x; k < n; k += NTHR)
        v += part[k];
    return block_sum(v, s);
}

__device__ __forceinline__ float num_of(float dx, float dy) { return __builtin_amdgcn_rcpf(fmaf(dy, dy, fmaf(dx, dx, 1.f))); }

// ---- step 2 ---------------------------------------------------------------------------------------------------------------------
template <bool LDS>
__global__ __launch_bounds__(NTHR) void k_cond_p(const float *__restrict__ X, int N, int D, float log_u, float *P, float *__restrict__ beta_out)
{
    __shared__ float s_x[DTS_MAX_D];
    __shared__ float s_red[2][2][NWAVE];
    __shared__ float s_d[LDS ? DTS_LDS_ROW : 1];
    const int tid = threadIdx.x, i = blockIdx.x;
    if (tid < D)
        s_x[tid] = X[(int64_t)i * D + tid];
    __syncthreads();
    float *row = P + (int64_t)i * N;
    float *d_of = LDS ? s_d : row;                                 // thread t touches the entries j = t (mod NTHR) only
    float dmin = INFINITY;
    for (int j = tid; j < N; j += NTHR) {
        const float *__restrict__ xj = X + (int64_t)j * D;
        float acc = 0.f;
        for (int k = 0; k < D; ++k) {
            const float diff = s_x[k] - xj[k];
            acc = fmaf(diff, diff, acc);
        }
        d_of[j] = acc;
        if (j != i)
            dmin = fminf(dmin, acc);
    }
    dmin = wave_min(dmin);
    if ((tid & 63) == 0)
        s_red[0][0][tid >> 6] = dmin;
    __syncthreads();
    dmin = fminf(fminf(s_red[0][0][0], s_red[0][0][1]), fminf(s_red[0][0][2], s_red[0][0][3]));
    __syncthreads();

    float beta = 1.f, lo = -INFINITY, hi = INFINITY, sum_p = 1.f;
    for (int tries = 0;; ++tries) {
        float a = 0.f, b = 0.f;
        for (int j = tid; j < N; j += NTHR) {
            if (j == i)
                continue;
            const float d = d_of[j] - dmin;
            const float e = expf(-beta * d);
            a += e;
            b = fmaf(d, e, b);
        }
        // (two sums, one barrier: the slots alternate from try to try, so a slot is rewritten only after the barrier of the try
        // in between, which every reader of its previous content has passed)
        float(*s)[NWAVE] = s_red[tries & 1];
        a = wave_sum(a), b = wave_sum(b);
        if ((tid & 63) == 0)
            s[0][tid >> 6] = a, s[1][tid >> 6] = b;
        __syncthreads();
        sum_p = (s[0][0] + s[0][1]) + (s[0][2] + s[0][3]);
        const float sum_dp = (s[1][0] + s[1][1]) + (s[1][2] + s[1][3]);
        const float h_diff = logf(sum_p) + beta * sum_dp / sum_p - log_u;
        if (fabsf(h_diff) <= 1e-5f || tries >= 50)                  // (the same for every thread)
            break;
        if (h_diff > 0.f) {
            lo = beta;
            beta = hi == INFINITY ? beta * 2.f : (beta + hi) * 0.5f;
        } else {
            hi = beta;
            beta = lo == -INFINITY ? beta * 0.5f : (beta + lo) * 0.5f;
        }
    }
    for (int j = tid; j < N; j += NTHR)
        row[j] = j == i ? 0.f : expf(-beta * (d_of[j] - dmin)) / sum_p;
    if (tid == 0)
        beta_out[i] = beta;
}

// ---- step 3 ---------------------------------------------------------------------------------------------------------------------
template <bool APPLY>
__global__ __launch_bounds__(NTHR) void k_sym(float *P, int N, int T, float *part, int nparts)
{
    constexpr int TS = DTS_SYM_TILE;
    __shared__ float a[TS][TS + 1], b[TS][TS + 1];
    __shared__ float s_red[NWAVE];
    const int tid = threadIdx.x, tx = tid & (TS - 1), ty = tid / TS;
    float total = 1.f, acc = 0.f;
    if (APPLY) {
        total = sum_parts(part, nparts, s_red);
        __syncthreads();
    }
    for (int t = blockIdx.x; t < T * T; t += gridDim.x) {
        const int bi = t / T, bj = t - bi * T;
        if (bi > bj)                                               // (the whole workgroup)
            continue;
        const bool diag = bi == bj;
        for (int r = ty; r < TS; r += NTHR / TS) {
            const int gi = bi * TS + r, gj = bj * TS + tx;         // tile A: rows of bi, columns of bj
            a[r][tx] = gi < N && gj < N ? P[(int64_t)gi * N + gj] : 0.f;
            const int hi = bj * TS + r, hj = bi * TS + tx;         // tile B, its mirror
            if (!diag)
                b[r][tx] = hi < N && hj < N ? P[(int64_t)hi * N + hj] : 0.f;
        }
        __syncthreads();
        for (int r = ty; r < TS; r += NTHR / TS) {
            const int gi = bi * TS + r, gj = bj * TS + tx;
            const float sa = a[r][tx] + (diag ? a[tx][r] : b[tx][r]);
            if (APPLY) {
                if (gi < N && gj < N)
                    P[(int64_t)gi * N + gj] = sa / total;
                if (!diag) {
                    const int hi = bj * TS + r, hj = bi * TS + tx;
                    if (hi < N && hj < N)
                        P[(int64_t)hi * N + hj] = (b[r][tx] + a[tx][r]) / total;
                }
            } else {
                acc += diag ? sa : sa + sa;                        // (the mirror tile holds the same sums)
            }
        }
        __syncthreads();
    }
    if (!APPLY) {
        acc = block_sum(acc, s_red);
        if (tid == 0)
            part[blockIdx.x] = acc;
    }
}

// ---- step 5 ---------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(NTHR) void k_zsum(const float *__restrict__ Y, int N, float *__restrict__ zpart)
{
    __shared__ float s_yx[DTS_Z_COLS], s_yy[DTS_Z_COLS];
    __shared__ float s_red[NWAVE];
    const int tid = threadIdx.x;
    const int i = blockIdx.x * DTS_Z_ROWS + tid, c0 = blockIdx.y * DTS_Z_COLS, cn = min(DTS_Z_COLS, N - c0);
    // num_ij == num_ji bitwise: a block below the diagonal is left to its mirror cells, which count twice (dts_z_block_weight)
    const int weight = dts_z_block_weight(blockIdx.x, blockIdx.y);
    if (weight == 0) {                                             // (the whole workgroup)
        if (tid == 0)
            zpart[blockIdx.x * gridDim.y + blockIdx.y] = 0.f;
        return;
    }
    for (int c = tid; c < cn; c += NTHR)
        s_yx[c] = Y[2 * (c0 + c)], s_yy[c] = Y[2 * (c0 + c) + 1];
    __syncthreads();
    float acc = 0.f;
    if (i < N) {
        const float yx = Y[2 * i], yy = Y[2 * i + 1];
        for (int c = 0; c < cn; ++c) {
            const float num = num_of(yx - s_yx[c], yy - s_yy[c]);
            acc += c0 + c != i ? num : 0.f;
        }
    }
    acc = block_sum(acc, s_red);
    if (tid == 0)
        zpart[blockIdx.x * gridDim.y + blockIdx.y] = acc * (float)weight;
}

template <int VEC, bool KL>
__global__ __launch_bounds__(NTHR) void k_gradient(const float *__restrict__ P, const float *__restrict__ Y, int N, float scale,
                                                   const float *__restrict__ zpart, int nz, float *__restrict__ dY,
                                                   float *__restrict__ klpart, float *__restrict__ z_out, int yvec)
{
    __shared__ float s_red[NWAVE];
    __shared__ float s_out[NWAVE][2 * GR + 1];
    const int tid = threadIdx.x;
    const float Z = sum_parts(zpart, nz, s_red);
    if (z_out && blockIdx.x == 0 && tid == 0)
        *z_out = Z;
    const float inv_z = 1.f / Z;
    const int row0 = blockIdx.x * GR;
    int rows[GR];
    float yix[GR], yiy[GR], ax[GR], ay[GR], kl = 0.f;
#pragma unroll
    for (int r = 0; r < GR; ++r) {
        rows[r] = min(row0 + r, N - 1);                            // rows past the end repeat the last one and are not stored
        yix[r] = Y[2 * rows[r]], yiy[r] = Y[2 * rows[r] + 1];
        ax[r] = ay[r] = 0.f;
    }
    for (int c = tid * VEC; c < N; c += NTHR * VEC) {              // VEC == 4: N % 4 == 0, so c + 3 < N
        float yjx[VEC], yjy[VEC];
        bool loaded = false;
        if constexpr (VEC == 4) {
            if (yvec) {                                            // (Y starts on 16 bytes; c is a multiple of 4)
                const float4 u = *reinterpret_cast<const float4 *>(Y + 2 * c), v = *reinterpret_cast<const float4 *>(Y + 2 * c + 4);
                yjx[0] = u.x, yjy[0] = u.y, yjx[1] = u.z, yjy[1] = u.w;
                yjx[2] = v.x, yjy[2] = v.y, yjx[3] = v.z, yjy[3] = v.w;
                loaded = true;
            }
        }
        if (!loaded) {
#pragma unroll
            for (int v = 0; v < VEC; ++v)
                yjx[v] = Y[2 * (c + v)], yjy[v] = Y[2 * (c + v) + 1];
        }
#pragma unroll
        for (int r = 0; r < GR; ++r) {
            const float *__restrict__ src = P + (int64_t)rows[r] * N + c;
            float p[VEC];
            if constexpr (VEC == 4) {
                const float4 u = *reinterpret_cast<const float4 *>(src);
                p[0] = u.x, p[1] = u.y, p[2] = u.z, p[3] = u.w;
            } else {
                p[0] = src[0];
            }
#pragma unroll
            for (int v = 0; v < VEC; ++v) {
                const float dx = yix[r] - yjx[v], dy = yiy[r] - yjy[v];
                const float num = c + v != rows[r] ? num_of(dx, dy) : 0.f;
                const float pe = fmaxf(4.f * p[v], 1e-21f) * scale;
                const float q = fmaxf(num * inv_z, 1e-12f);
                const float w = (pe - q) * num;
                ax[r] = fmaf(w, dx, ax[r]);
                ay[r] = fmaf(w, dy, ay[r]);
                if (KL && row0 + r < N)
                    kl += pe * logf(pe / q);
            }
        }
    }
    const int lane = tid & 63, wave = tid >> 6;
#pragma unroll
    for (int r = 0; r < GR; ++r) {
        const float sx = wave_sum(ax[r]), sy = wave_sum(ay[r]);
        if (lane == 0)
            s_out[wave][2 * r] = sx, s_out[wave][2 * r + 1] = sy;
    }
    if (KL) {
        kl = wave_sum(kl);
        if (lane == 0)
            s_out[wave][2 * GR] = kl;
    }
    __syncthreads();
    if (tid < 2 * GR + (KL ? 1 : 0)) {
        const float v = (s_out[0][tid] + s_out[1][tid]) + (s_out[2][tid] + s_out[3][tid]);
        if (tid == 2 * GR)
            klpart[blockIdx.x] = v;
        else if (row0 + tid / 2 < N)
            dY[2 * row0 + tid] = v;
    }
}

__global__ __launch_bounds__(NTHR) void k_update(const float *__restrict__ dY, float *__restrict__ iY, float *__restrict__ gains,
                                                 float *__restrict__ Y, int N, float momentum, float *__restrict__ colpart,
                                                 const float *__restrict__ klpart, int nkl, float *__restrict__ kl_out)
{
    __shared__ float s_red[3][NWAVE];
    const int tid = threadIdx.x, i = blockIdx.x * DTS_UPD_ROWS + tid;
    if (kl_out && blockIdx.x == 0) {                               // (uniform over the workgroup)
        const float kl = sum_parts(klpart, nkl, s_red[2]);
        if (tid == 0)
            *kl_out = kl;
    }
    float s[2] = {0.f, 0.f};
    if (i < N) {
#pragma unroll
        for (int c = 0; c < 2; ++c) {
            const int e = 2 * i + c;
            const float d = dY[e];
            float v = iY[e], g = gains[e];
            g = (d > 0.f) != (v > 0.f) ? g + 0.2f : g * 0.8f;
            g = fmaxf(g, 0.01f);
            v = momentum * v - 500.f * (g * d);
            const float y = Y[e] + v;
            gains[e] = g, iY[e] = v, Y[e] = y;
            s[c] = y;
        }
    }
    const float sx = block_sum(s[0], s_red[0]), sy = block_sum(s[1], s_red[1]);
    if (tid == 0)
        colpart[2 * blockIdx.x] = sx, colpart[2 * blockIdx.x + 1] = sy;
}

__global__ __launch_bounds__(NTHR) void k_center(float *__restrict__ Y, int N, const float *__restrict__ colpart, int nparts)
{
    __shared__ float s_red[2][NWAVE];
    const int tid = threadIdx.x, i = blockIdx.x * DTS_UPD_ROWS + tid;
    float vx = 0.f, vy = 0.f;
    for (int k = tid; k < nparts; k += NTHR)
        vx += colpart[2 * k], vy += colpart[2 * k + 1];
    const float mx = block_sum(vx, s_red[0]) / (float)N, my = block_sum(vy, s_red[1]) / (float)N;
    if (i < N)
        Y[2 * i] -= mx, Y[2 * i + 1] -= my;
}

int launched(const char *what)
{
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess) {
        dts_set_error("%s: launch failed: %s", what, hipGetErrorString(e));
        return (int)e;
    }
    return DTS_OK;
}

bool n_ok(const char *what, int N)
{
    if (N < 2 || (int64_t)N * N >= (1ll << 31)) {
        dts_set_error("%s: N = %d not taken (2 <= N, N * N < 2^31)", what, N);
        return false;
    }
    return true;
}

void launch_zsum(const float *Y, int N, float *zpart, hipStream_t st)
{
    hipLaunchKernelGGL(k_zsum, dim3(dts_z_row_blocks(N), dts_z_col_chunks(N)), dim3(NTHR), 0, st, Y, N, zpart);
}

void launch_gradient(const float *P, const float *Y, int N, float ex, const float *zpart, float *dY, float *klpart, float *z_out,
                     hipStream_t st)
{
    const dim3 grid(dts_grad_groups(N)), block(NTHR);
    const int nz = dts_z_parts(N), yvec = ((uintptr_t)Y & 15) == 0 ? 1 : 0;
    const float scale = ex * 0.25f;
    const bool vec = dts_grad_vec((uintptr_t)P, N);
    if (vec && klpart)
        hipLaunchKernelGGL((k_gradient<4, true>), grid, block, 0, st, P, Y, N, scale, zpart, nz, dY, klpart, z_out, yvec);
    else if (vec)
        hipLaunchKernelGGL((k_gradient<4, false>), grid, block, 0, st, P, Y, N, scale, zpart, nz, dY, klpart, z_out, yvec);
    else if (klpart)
        hipLaunchKernelGGL((k_gradient<1, true>), grid, block, 0, st, P, Y, N, scale, zpart, nz, dY, klpart, z_out, yvec);
    else
        hipLaunchKernelGGL((k_gradient<1, false>), grid, block, 0, st, P, Y, N, scale, zpart, nz, dY, klpart, z_out, yvec);
}

void launch_update(const float *dY, float *iY, float *gains, float *Y, int N, float momentum, float *colpart, const float *klpart,
                   float *kl_out, hipStream_t st)
{
    const dim3 grid(dts_upd_groups(N)), block(NTHR);
    hipLaunchKernelGGL(k_update, grid, block, 0, st, dY, iY, gains, Y, N, momentum, colpart, klpart, dts_grad_groups(N), kl_out);
    hipLaunchKernelGGL(k_center, grid, block, 0, st, Y, N, (const float *)colpart, dts_upd_groups(N));
}

}  // namespace

extern "C" int dts_cond_p(const float *X, int N, int D, float perplexity, int scratch, float *P, float *beta, void *stream)
{
    if (!dts_shape_ok(N, D, (double)perplexity)) {
        dts_set_error("dts_cond_p: N = %d, D = %d, perplexity = %g not taken (dts_supported)", N, D, (double)perplexity);
        return DTS_EINVAL;
    }
    if (!X || !P || !beta || (scratch != 0 && scratch != 1)) {
        dts_set_error("dts_cond_p: a null pointer, or scratch not 0 or 1");
        return DTS_EINVAL;
    }
    const float log_u = logf(perplexity);
    if (dts_row_in_lds(N) && !scratch)
        hipLaunchKernelGGL((k_cond_p<true>), dim3(N), dim3(NTHR), 0, (hipStream_t)stream, X, N, D, log_u, P, beta);
    else
        hipLaunchKernelGGL((k_cond_p<false>), dim3(N), dim3(NTHR), 0, (hipStream_t)stream, X, N, D, log_u, P, beta);
    return launched("dts_cond_p");
}

extern "C" int dts_symmetrize(float *P, int N, float *part, void *stream)
{
    if (!n_ok("dts_symmetrize", N))
        return DTS_EINVAL;
    if (!P || !part) {
        dts_set_error("dts_symmetrize: a null pointer");
        return DTS_EINVAL;
    }
    const int T = dts_sym_tiles(N), G = dts_sym_groups(N);
    hipLaunchKernelGGL((k_sym<false>), dim3(G), dim3(NTHR), 0, (hipStream_t)stream, P, N, T, part, G);
    hipLaunchKernelGGL((k_sym<true>), dim3(G), dim3(NTHR), 0, (hipStream_t)stream, P, N, T, part, G);
    return launched("dts_symmetrize");
}

extern "C" int dts_zsum(const float *Y, int N, float *zpart, void *stream)
{
    if (!n_ok("dts_zsum", N))
        return DTS_EINVAL;
    if (!Y || !zpart) {
        dts_set_error("dts_zsum: a null pointer");
        return DTS_EINVAL;
    }
    launch_zsum(Y, N, zpart, (hipStream_t)stream);
    return launched("dts_zsum");
}

extern "C" int dts_gradient(const float *P, const float *Y, int N, float exaggeration, const float *zpart, float *dY, float *klpart,
                            float *z_out, void *stream)
{
    if (!n_ok("dts_gradient", N))
        return DTS_EINVAL;
    if (!P || !Y || !zpart || !dY) {
        dts_set_error("dts_gradient: a null pointer");
        return DTS_EINVAL;
    }
    if (!(exaggeration > 0.f)) {
        dts_set_error("dts_gradient: exaggeration must be positive");
        return DTS_EINVAL;
    }
    launch_gradient(P, Y, N, exaggeration, zpart, dY, klpart, z_out, (hipStream_t)stream);
    return launched("dts_gradient");
}

extern "C" int dts_update(const float *dY, float *iY, float *gains, float *Y, int N, float momentum, float *colpart,
                          const float *klpart, float *kl_out, void *stream)
{
    if (!n_ok("dts_update", N))
        return DTS_EINVAL;
    if (!dY || !iY || !gains || !Y || !colpart) {
        dts_set_error("dts_update: a null pointer");
        return DTS_EINVAL;
    }
    if (kl_out && !klpart) {
        dts_set_error("dts_update: kl_out without klpart");
        return DTS_EINVAL;
    }
    launch_update(dY, iY, gains, Y, N, momentum, colpart, klpart, kl_out, (hipStream_t)stream);
    return launched("dts_update");
}

extern "C" int dts_run(const float *P, float *Y, float *iY, float *gains, float *dY, float *ws, int N, int first, int last,
                       float *kl_hist, void *stream)
{
    if (!n_ok("dts_run", N))
        return DTS_EINVAL;
    if (!P || !Y || !iY || !gains || !dY || !ws) {
        dts_set_error("dts_run: a null pointer");
        return DTS_EINVAL;
    }
    if (first < 0 || last < first) {
        dts_set_error("dts_run: iterations [%d, %d) not taken", first, last);
        return DTS_EINVAL;
    }
    hipStream_t st = (hipStream_t)stream;
    float *zpart = ws + dts_ws_z(N), *klpart = ws + dts_ws_kl(N), *colpart = ws + dts_ws_col(N);
    for (int it = first; it < last; ++it) {
        const int slot = kl_hist ? dts_kl_slot(it) : -1;
        launch_zsum(Y, N, zpart, st);
        launch_gradient(P, Y, N, dts_exaggeration(it), zpart, dY, slot >= 0 ? klpart : nullptr, nullptr, st);
        launch_update(dY, iY, gains, Y, N, dts_momentum(it), colpart, klpart, slot >= 0 ? kl_hist + slot : nullptr, st);
        const int rc = launched("dts_run");
        if (rc != DTS_OK)
            return rc;
    }
    return DTS_OK;
}
