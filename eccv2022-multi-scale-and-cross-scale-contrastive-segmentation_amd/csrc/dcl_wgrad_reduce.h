// dcl_wgrad_reduce.h -- the slab reductions of the 3x3 weight gradient, dw = sum of the slabs of `part` in fixed order, for the
// translation units that launch them: dcl_wgrad3x3.hip (dcl_wgrad3x3_f16x3) and dcl_convbwd.hip (the fused backward launch).
#pragma once
#include "dcl_common.h"

namespace {

// dw[co][ci][tap] = sum_s part[s][tap][co][ci].  Block = 32 outputs x 8 slab groups: group g adds slabs g, g+8, ...
// in order, the 8 partial sums are combined in order through LDS -> fixed summation tree, deterministic.
template <int K>
__global__ __launch_bounds__(256) void k_wgrad_reduce_t(const float *__restrict__ part, int S, int Cout, int Cin,
                                                       float *__restrict__ dw)
{
    // K groups of 32 outputs per workgroup: 1 for the narrow layers (many slabs, few outputs: parallelism over the
    // outputs matters), 4 for the wide ones (with one, the 1.3 M outputs of a 384-channel layer were 41 k workgroups of
    // a few loads each -- 16 us, bound by the workgroup dispatch rate)
    __shared__ float sh[K][8][32];
    const int total = 9 * Cout * Cin;
    const int lane = threadIdx.x & 31, g = threadIdx.x >> 5;
#pragma unroll
    for (int k = 0; k < K; ++k) {
        const int idx = (blockIdx.x * K + k) * 32 + lane;       // (tap, co, ci) in slab order
        float s0 = 0.f, s1 = 0.f;
        if (idx < total) {
            int q = g;
            for (; q + 8 < S; q += 16) {
                s0 += part[(size_t)q * total + idx];
                s1 += part[(size_t)(q + 8) * total + idx];
            }
            if (q < S)
                s0 += part[(size_t)q * total + idx];
        }
        sh[k][g][lane] = s0 + s1;
    }
    __syncthreads();
    if (g < K) {
        const int idx = (blockIdx.x * K + g) * 32 + lane;
        if (idx < total) {
            float s = sh[g][0][lane];
#pragma unroll
            for (int q = 1; q < 8; ++q)
                s += sh[g][q][lane];
            const int ci = idx % Cin;
            const int co = (idx / Cin) % Cout;
            const int tap = idx / (Cin * Cout);
            dw[((size_t)co * Cin + ci) * 9 + tap] = s;
        }
    }
}

// Wide layers (few slabs, many outputs): one workgroup per (co, 32 ci), thread = (tap, ci).  The slab layout
// [tap][co][ci] is read in 128-byte runs as before, but dw[co][ci][tap] is written through an LDS tile as ONE contiguous
// 1152-byte run -- the per-output form writes 4 bytes every 36 (a 32-byte sector per value: 42 MB of write traffic for the
// 5 MB gradient of a 384-channel layer).  Same slab order: bitwise the same sums when S <= 8 (one group per output).
__global__ __launch_bounds__(320) void k_wgrad_reduce_wide(const float *__restrict__ part, int S, int Cout, int Cin,
                                                          float *__restrict__ dw)
{
    __shared__ float tile[32 * 9];
    const int co = blockIdx.y, ci0 = blockIdx.x * 32;
    const int t = threadIdx.x, tap = t >> 5, cl = t & 31;
    const size_t total = (size_t)9 * Cout * Cin;
    if (t < 288) {
        float s0 = 0.f;
        if (ci0 + cl < Cin) {
            const float *p = part + ((size_t)tap * Cout + co) * Cin + ci0 + cl;
            for (int q = 0; q < S; ++q)
                s0 += p[(size_t)q * total];
        }
        tile[cl * 9 + tap] = s0;
    }
    __syncthreads();
    const int nci = min(32, Cin - ci0);
    if (t < nci * 9)
        dw[((size_t)co * Cin + ci0) * 9 + t] = tile[t];
}

static void launch_wgrad_reduce(const float *part, int S, int Cout, int Cin, float *dw, hipStream_t st)
{
    const int total = 9 * Cout * Cin;
    if (total >= (1 << 18) && S <= 8)
        hipLaunchKernelGGL(k_wgrad_reduce_wide, dim3((Cin + 31) / 32, Cout), dim3(320), 0, st, part, S, Cout, Cin, dw);
    else if (total >= (1 << 18))
        hipLaunchKernelGGL(k_wgrad_reduce_t<4>, dim3((total + 127) / 128), dim3(256), 0, st, part, S, Cout, Cin, dw);
    else
        hipLaunchKernelGGL(k_wgrad_reduce_t<1>, dim3((total + 31) / 32), dim3(256), 0, st, part, S, Cout, Cin, dw);
}

}  // namespace
