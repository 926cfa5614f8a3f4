// dcl_f16x3.h -- the split-f16 ("f16x3") building blocks, one definition each, for every translation unit that feeds the f16
// matrix pipe with fp32-equivalent operands: an f32 value v becomes hi = f16(v * s) and lo = f16(v * s - hi) for a power-of-two
// scale s, and a product is hi.hi + hi.lo + lo.hi with f32 accumulation.  Also the LDS-DMA pieces the staged kernels share.
//   half8, u32x4, as_half8     fragment types of the f16 MFMAs
//   F16_TARGET, pow2_scale     the operand scale from an absmax
//   split1, split2, split8     1 / 2 / 8 floats -> hi and lo (the only v_fma_mix* in the code base)
//   split_to_mfma_fence, split_to_mfma_pad    the wait states between a split and the MFMA that reads it (the rule is there)
//   uniform_ptr, dma16, vm_wait               LDS-DMA staging
// (the wave maximum that feeds pow2_scale: wave_max in dcl_common.h)
#pragma once
#include "dcl_common.h"

// Bound probe of the weight-gradient kernels (tools/probes/conv_bounds.sh; 0 in the product): 1 = no MFMAs (k_wgrad3x3d,
// k_wgrad1x1d), 2 = no LDS-DMA -- dma16 below, i.e. EVERY kernel that stages through it, k_wgrad3x3_s2d included.  Results are
// wrong.  Defined here because dma16 reads it; the units that issue no dma16 are not affected by it.
#ifndef DCL_WG_PROBE
#define DCL_WG_PROBE 0
#endif

namespace {

typedef _Float16 half8 __attribute__((ext_vector_type(8)));
typedef unsigned u32x4 __attribute__((ext_vector_type(4)));

constexpr float F16_TARGET = 16384.0f;      // operands are scaled so that their absmax lands in (2^13, 2^14]

// power-of-two operand scale from the tensor's absmax (the same expression wherever a scale is formed, so that a packer and its
// consumer see the same one); an all-zero tensor takes 1, inf / nan propagate into the products
__device__ __forceinline__ float pow2_scale(float amax)
{
    return amax == 0.f ? 1.f : exp2f(fminf(fmaxf(floorf(log2f(F16_TARGET / amax)), -100.f), 100.f));
}

// Packed f16 pair (lo half = element 0) of hi = f16(v * s) and of lo = f16(v * s - hi) for two values.  s is a power
// of two (or 0), so v * s is exact and the fused form computes the same value; written as v_fma_mix{lo,hi}_f16
// (f32 / f16 inputs, f32 arithmetic, f16 result into one half of the destination): 2 VALU instructions per value
// and no packing.  The compiler's own lowering of the C expression takes 3+ and a v_pack.
__device__ __forceinline__ void split2(float v0, float v1, float s, unsigned &hi, unsigned &lo)
{
    // (mixlo leaves the upper half of its destination alone; mixhi fills it right after, so no initialisation)
    asm("v_fma_mixlo_f16 %0, %1, %2, 0" : "=v"(hi) : "v"(v0), "v"(s));
    asm("v_fma_mixhi_f16 %0, %1, %2, 0" : "+v"(hi) : "v"(v1), "v"(s));
    asm("v_fma_mixlo_f16 %0, %1, %2, -%3 op_sel_hi:[0,0,1]" : "=&v"(lo) : "v"(v0), "v"(s), "v"(hi));
    asm("v_fma_mixhi_f16 %0, %1, %2, -%3 op_sel:[0,0,1] op_sel_hi:[0,0,1]" : "+v"(lo) : "v"(v1), "v"(s), "v"(hi));
}

// one value: f16 hi / lo in the low halves of hi / lo (upper halves undefined)
__device__ __forceinline__ void split1(float v0, float s, unsigned &hi, unsigned &lo)
{
    asm("v_fma_mixlo_f16 %0, %1, %2, 0" : "=v"(hi) : "v"(v0), "v"(s));
    asm("v_fma_mixlo_f16 %0, %1, %2, -%3 op_sel_hi:[0,0,1]" : "=&v"(lo) : "v"(v0), "v"(s), "v"(hi));
}

// 8 floats -> MFMA operand fragments (hi, lo)
__device__ __forceinline__ void split8(const float (&v)[8], float s, u32x4 &hi, u32x4 &lo)
{
    unsigned h0, h1, h2, h3, l0, l1, l2, l3;
    split2(v[0], v[1], s, h0, l0);
    split2(v[2], v[3], s, h1, l1);
    split2(v[4], v[5], s, h2, l2);
    split2(v[6], v[7], s, h3, l3);
    hi = u32x4{h0, h1, h2, h3};
    lo = u32x4{l0, l1, l2, l3};
}

__device__ __forceinline__ half8 as_half8(u32x4 v) { return __builtin_bit_cast(half8, v); }

// THE RULE: at least two wait states between the last v_fma_mix* of a split and an MFMA that reads the fragment as A or B.
// The splits are inline asm, and the compiler's hazard recognizer does not look inside an asm statement: it sees no VALU write
// there and pads only its one fixed state behind the statement.  The instruction set asks for two between a VALU write of a
// VGPR and an MFMA reading it (the s_nop 1 of the CDNA HIP programming guide, section 5.7 item 2).  With fewer the MFMA can read
// the register before its high half has landed: k_winattn_fwd_mfma showed 1e-4 errors in one of ~10^5 scores, which no small
// test sees.  So every kernel that calls a split puts one of the two forms below -- or real work -- between it and the MFMA, and
// the build checks the distance on the device assembly of every unit (tools/split_wait_states.py, run by the Makefile's
// compile rules): a kernel that falls short does not build.
//
// The fence: nothing moves across it.  For kernels that split a whole batch of fragments and then run their MFMAs.
__device__ __forceinline__ void split_to_mfma_fence()
{
    __builtin_amdgcn_sched_barrier(0);
    asm volatile("s_nop 4");
    __builtin_amdgcn_sched_barrier(0);
}

// The pad: two states tied to one hi / lo pair, which an MFMA can then read only behind them.  Loads, address arithmetic and
// MFMAs on other fragments still move freely: prefer it where a split sits inside a software pipeline the fence would cut.
// (Not volatile: its operands order it, and a volatile statement would also be pinned against dma16 and vm_wait.)
template <typename F>
__device__ __forceinline__ void split_to_mfma_pad(F &hi, F &lo)
{
    asm("s_nop 1" : "+v"(hi), "+v"(lo));
}

// a pointer the compiler knows to be wave-uniform (scalar registers)
__device__ __forceinline__ const float *uniform_ptr(const float *p)
{
    const unsigned long long v = (unsigned long long)(uintptr_t)p;
    const unsigned lo = __builtin_amdgcn_readfirstlane((unsigned)v), hi = __builtin_amdgcn_readfirstlane((unsigned)(v >> 32));
    return (const float *)(uintptr_t)(((unsigned long long)hi << 32) | lo);
}

// One LDS-DMA wave instruction: lane i copies the 16 bytes at gbase + voff(i) to LDS byte address lds_dst + 16 i; gbase and
// lds_dst must be wave-uniform.  (Inline asm: the compiler puts s_waitcnt vmcnt(0) in front of every LDS read that follows the
// builtin; here completion is counted by hand, vm_wait.)
__device__ __forceinline__ void dma16(const void *gbase, unsigned voff, unsigned lds_dst)
{
    if (DCL_WG_PROBE & 2)
        return;
    unsigned keep;
    asm volatile("s_mov_b32 %0, m0\n\ts_mov_b32 m0, %3\n\ts_nop 0\n\tglobal_load_lds_dwordx4 %1, %2\n\ts_mov_b32 m0, %0"
                 : "=&s"(keep)
                 : "v"(voff), "s"(gbase), "s"(lds_dst)
                 : "memory");
}

// wait until at most N of this wave's vector-memory operations are outstanding
template <int N>
__device__ __forceinline__ void vm_wait()
{
    static_assert(N >= 0 && N < 64, "vmcnt immediate");
    asm volatile("s_waitcnt vmcnt(%0)" ::"n"(N) : "memory");
}

}  // namespace
