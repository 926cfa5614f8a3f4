// dcl_ohem_plan.h -- what dcl_ohem.hip, dcl_ohem_capi.cpp and the host tests (tests/ohem_plan_main.cpp) share: the digit split of the
// radix select, the bin picking, the workspace layout and the shape test.  Host-compilable: plain functions, no HIP header
// (DOH_HD is empty unless a HIP compiler reads this, where it lets the kernels call the same code).
#pragma once
#include <stdint.h>

#include "../../include/dcl_ohem.h"

#ifdef __HIPCC__
#define DOH_HD __host__ __device__ __attribute__((always_inline))
#else
#define DOH_HD
#endif

void doh_set_error(const char *fmt, ...);

// ---- the digit split: a key is three digits, most significant first: 11 | 11 | 10 bits
#define DOH_PASSES 3
#define DOH_MAX_BINS 2048
DOH_HD static inline int doh_digit_bits(int pass) { return pass == 2 ? 10 : 11; }
DOH_HD static inline int doh_digit_shift(int pass) { return pass == 0 ? 21 : pass == 1 ? 10 : 0; }
DOH_HD static inline int doh_bins(int pass) { return 1 << doh_digit_bits(pass); }
DOH_HD static inline uint32_t doh_digit(uint32_t key, int pass)
{
    return (key >> doh_digit_shift(pass)) & (uint32_t)(doh_bins(pass) - 1);
}
// whether the digits of `key` above pass `pass` are those of `prefix` (pass 0: every key with the sign bit clear -- a p is never
// negative, and DOH_INVALID_BITS, the only pattern with the sign bit set, is in no histogram)
DOH_HD static inline bool doh_prefix_match(uint32_t key, uint32_t prefix, int pass)
{
    if (pass == 0)
        return (key >> 31) == 0;
    const int sh = doh_digit_shift(pass - 1);
    return (key >> sh) == (prefix >> sh);
}
// the prefix with the digit of pass `pass` set
DOH_HD static inline uint32_t doh_with_digit(uint32_t prefix, int pass, uint32_t digit)
{
    return prefix | (digit << doh_digit_shift(pass));
}

// a NaN takes one bit pattern (above +inf: it orders last); -0 cannot occur (exp), but costs nothing to fold
DOH_HD static inline uint32_t doh_canonical_bits(uint32_t bits)
{
    if ((bits & 0x7fffffffu) > 0x7f800000u)
        return 0x7fc00000u;
    return bits == 0x80000000u ? 0u : bits;
}

// ---- bin picking: the first bin b with  sum(hist[0 .. b]) > rank;  *rem = rank - sum(hist[0 .. b-1]), the rank inside the bin.
// -1 (and *rem untouched) when rank >= the total.
DOH_HD static inline int doh_pick_bin(const uint32_t *hist, int nbins, uint32_t rank, uint32_t *rem)
{
    uint32_t before = 0;
    for (int b = 0; b < nbins; ++b) {
        const uint32_t c = hist[b];
        if (rank - before < c) {          // before <= rank here, so the difference does not wrap
            *rem = rank - before;
            return b;
        }
        before += c;
    }
    return -1;
}

// two levels, as the one-workgroup kernel runs it: sums[j] = sum of the bins [j * chunk, (j + 1) * chunk) (the kernel forms them with
// one thread per chunk), the chunk is picked from the sums and the bin from the chunk.  Equals doh_pick_bin on the whole histogram.
#define DOH_CHUNKS 256
DOH_HD static inline uint32_t doh_chunk_sum(const uint32_t *hist, int chunk, int j)
{
    uint32_t s = 0;
    for (int b = 0; b < chunk; ++b)
        s += hist[j * chunk + b];
    return s;
}
DOH_HD static inline int doh_pick_two_level(const uint32_t *hist, const uint32_t *sums, int nbins, uint32_t rank, uint32_t *rem)
{
    const int chunk = nbins / DOH_CHUNKS;
    uint32_t r1 = 0, r2 = 0;
    const int j = doh_pick_bin(sums, DOH_CHUNKS, rank, &r1);
    if (j < 0)
        return -1;
    const int b = doh_pick_bin(hist + j * chunk, chunk, r1, &r2);
    if (b < 0)
        return -1;                        // (sums that are not the histogram's)
    *rem = r2;
    return j * chunk + b;
}

// k = min(max(min_kept, 1), n - 1) for n >= 1
DOH_HD static inline uint32_t doh_rank(int min_kept, uint32_t n)
{
    const uint32_t mk = min_kept < 1 ? 1u : (uint32_t)min_kept;
    return mk < n - 1 ? mk : n - 1;
}

// ---- the workspace, in 4-byte words: three histograms, the state, the row partials {f32 sum l, u32 count}
#define DOH_WS_HIST0 0
#define DOH_WS_HIST1 (DOH_WS_HIST0 + 2048)
#define DOH_WS_HIST2 (DOH_WS_HIST1 + 2048)
#define DOH_WS_STATE (DOH_WS_HIST2 + 1024)
#define DOH_WS_PART (DOH_WS_STATE + 16)
#define DOH_WS_CLEAR DOH_WS_PART /* words doh_target_prob clears: everything in front of the partials */
// state words
#define DOH_ST_N 0      /* valid pixels (atomic counter) */
#define DOH_ST_PREFIX 1 /* digits fixed so far */
#define DOH_ST_RANK 2   /* rank inside the bins that match the prefix */
#define DOH_ST_EMPTY 3  /* 1 when n == 0 */
#define DOH_ST_V 4      /* bits of v */
#define DOH_ST_THR 5    /* bits of thr */
#define DOH_ST_K 6      /* k */

DOH_HD static inline int doh_ws_hist(int pass) { return pass == 0 ? DOH_WS_HIST0 : pass == 1 ? DOH_WS_HIST1 : DOH_WS_HIST2; }

static inline int64_t doh_ws_bytes(int N, int H)
{
    const int64_t rows = (int64_t)N * H;
    if (N < 1 || H < 1 || rows >= (1ll << 31))
        return -1;
    return (DOH_WS_PART + 2 * rows) * 4;
}

static inline bool doh_shape_ok(int N, int C, int h, int w, int H, int W)
{
    if (N < 1 || C < 1 || C > DOH_MAX_C || h < 1 || w < 1 || H < h || W < w)
        return false;
    const int64_t lim = 1ll << 31;
    if ((int64_t)N * H >= lim || (int64_t)N * H * W >= lim || (int64_t)N * C * h >= lim || (int64_t)N * C * h * w >= lim)
        return false;
    // the limits of dcl_upsample_ce_fwd / dcl_upsample_ce_bwd (csrc/dcl_upce.hip)
    return 2 * (int64_t)w <= 6144 && 3 * (int64_t)w + W <= 36864 && 2 * (((int64_t)H + h - 1) / h) + 8 <= 80;
}
