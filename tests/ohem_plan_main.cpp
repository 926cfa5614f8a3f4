// Stand-alone check of csrc/dcl_ohem_plan.h (built with -fsanitize=address,undefined by tests/test_ohem_host.py): the radix select
// as the kernels run it -- three histograms, a two-level bin pick after each -- against a sorted array, for random and all-equal
// keys, with the rank at 0, at n - 1 and at every bin boundary; the digits reassemble the key; the workspace regions do not overlap.
#include <algorithm>
#include <cstdarg>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "dcl_ohem_plan.h"

void doh_set_error(const char *, ...) {}

static int fails = 0;
#define CHECK(cond, ...)                    \
    do {                                    \
        if (!(cond)) {                      \
            if (++fails < 20) {             \
                printf("FAIL %s: ", #cond); \
                printf(__VA_ARGS__);        \
                printf("\n");               \
            }                               \
        }                                   \
    } while (0)

static uint32_t rng_state = 12345u;
static uint32_t rnd()
{
    rng_state ^= rng_state << 13;
    rng_state ^= rng_state >> 17;
    rng_state ^= rng_state << 5;
    return rng_state;
}

// the select of the device code on the host: keys with the sign bit set are invalid pixels
static uint32_t select_kth(const std::vector<uint32_t> &keys, uint32_t rank, std::vector<uint32_t> *boundaries)
{
    uint32_t prefix = 0;
    for (int pass = 0; pass < DOH_PASSES; ++pass) {
        const int bins = doh_bins(pass);
        std::vector<uint32_t> hist(bins, 0u), sums(DOH_CHUNKS, 0u);
        for (uint32_t k : keys)
            if ((k >> 31) == 0 && doh_prefix_match(k, prefix, pass))
                hist[doh_digit(k, pass)]++;
        for (int j = 0; j < DOH_CHUNKS; ++j)
            sums[j] = doh_chunk_sum(hist.data(), bins / DOH_CHUNKS, j);
        uint32_t rem = 0xdeadbeefu, rem1 = 0xdeadbeefu;
        const int b = doh_pick_two_level(hist.data(), sums.data(), bins, rank, &rem);
        const int b1 = doh_pick_bin(hist.data(), bins, rank, &rem1);
        CHECK(b >= 0 && b == b1 && rem == rem1, "pass %d rank %u: two-level %d/%u one-level %d/%u", pass, rank, b, rem, b1, rem1);
        if (b < 0)
            return 0;
        CHECK(rem < hist[b], "rank inside the bin");
        if (boundaries && pass == 0) {            // ranks at which the first digit changes
            uint32_t c = 0;
            for (int i = 0; i < bins; ++i) {
                if (hist[i]) {
                    boundaries->push_back(c);
                    boundaries->push_back(c + hist[i] - 1);
                }
                c += hist[i];
            }
        }
        prefix = doh_with_digit(prefix, pass, (uint32_t)b);
        rank = rem;
    }
    return prefix;
}

static void run(const std::vector<uint32_t> &keys, const char *what)
{
    std::vector<uint32_t> valid;
    for (uint32_t k : keys)
        if ((k >> 31) == 0)
            valid.push_back(k);
    std::sort(valid.begin(), valid.end());
    const uint32_t n = (uint32_t)valid.size();
    std::vector<uint32_t> ranks = {0u, n - 1, n / 2, n / 3}, bounds;
    select_kth(keys, 0, &bounds);
    ranks.insert(ranks.end(), bounds.begin(), bounds.end());
    for (uint32_t r : ranks) {
        if (r >= n)
            continue;
        const uint32_t got = select_kth(keys, r, nullptr);
        CHECK(got == valid[r], "%s: rank %u of %u: %08x, sorted %08x", what, r, n, got, valid[r]);
    }
    // a rank at or beyond the count is refused, not answered
    std::vector<uint32_t> hist(doh_bins(0), 0u);
    for (uint32_t k : valid)
        hist[doh_digit(k, 0)]++;
    uint32_t rem = 7;
    CHECK(doh_pick_bin(hist.data(), doh_bins(0), n, &rem) == -1 && rem == 7, "%s: rank n refused", what);
}

int main()
{
    // digits reassemble the key; the bins of the passes
    CHECK(doh_digit_bits(0) + doh_digit_bits(1) + doh_digit_bits(2) == 32, "digit bits");
    for (int i = 0; i < 100000; ++i) {
        const uint32_t k = i < 4 ? (i == 0 ? 0u : i == 1 ? 0xffffffffu : i == 2 ? 0x7fc00000u : 0x3f800000u) : rnd();
        uint32_t back = 0;
        for (int pass = 0; pass < DOH_PASSES; ++pass) {
            CHECK(doh_digit(k, pass) < (uint32_t)doh_bins(pass), "digit range");
            back = doh_with_digit(back, pass, doh_digit(k, pass));
            if (pass + 1 < DOH_PASSES)
                CHECK(doh_prefix_match(k, back, pass + 1), "prefix of its own digits");
        }
        CHECK(back == k, "%08x reassembles to %08x", k, back);
    }
    CHECK(!doh_prefix_match(DOH_INVALID_BITS, 0u, 0) && (DOH_INVALID_BITS >> 31) == 1, "the invalid pattern is in no pass");
    CHECK(doh_canonical_bits(0x7f800001u) == 0x7fc00000u && doh_canonical_bits(0xffc00000u) == 0x7fc00000u &&
              doh_canonical_bits(0x7f800000u) == 0x7f800000u && doh_canonical_bits(0x80000000u) == 0u &&
              doh_canonical_bits(0x3f800000u) == 0x3f800000u, "canonical bits");
    // k = min(max(min_kept, 1), n - 1)
    CHECK(doh_rank(0, 10) == 1 && doh_rank(5, 10) == 5 && doh_rank(9, 10) == 9 && doh_rank(10, 10) == 9 && doh_rank(1000000000, 7) == 6 &&
              doh_rank(3, 1) == 0 && doh_rank(2147483647, 2147483647u) == 2147483646u, "rank");

    // random keys: floats in [0, 1] (as probabilities are), full-range positives, a few invalid ones in between
    std::vector<uint32_t> keys;
    for (int i = 0; i < 50000; ++i) {
        float f = (float)(rnd() >> 8) / 16777216.f;
        if (i % 3 == 0)
            f = f * f * f * f;
        uint32_t b;
        memcpy(&b, &f, 4);
        keys.push_back(i % 11 == 0 ? DOH_INVALID_BITS : b);
    }
    run(keys, "probabilities");
    keys.clear();
    for (int i = 0; i < 30000; ++i)
        keys.push_back(rnd() >> 1);
    run(keys, "positive words");
    keys.assign(5000, 0x3e99999au);                  // all equal
    keys.push_back(DOH_INVALID_BITS);
    run(keys, "all equal");
    keys.assign(1, 0x3f000000u);                     // a single key
    run(keys, "single");
    keys.clear();
    for (int i = 0; i < 4096; ++i)                   // one bin of the first two passes: the third decides
        keys.push_back(0x3e99a000u + (rnd() & 1023u));
    run(keys, "third pass");
    keys.clear();
    for (int i = 0; i < 3000; ++i)                   // every bin of the first pass holds one key: every rank is a boundary
        keys.push_back(((uint32_t)(i % 1024) << 21) | (rnd() & 0x1fffffu));
    run(keys, "boundaries");

    // the workspace: regions in order, no overlap, the clear covers everything in front of the partials
    const int off[6] = {DOH_WS_HIST0, DOH_WS_HIST1, DOH_WS_HIST2, DOH_WS_STATE, DOH_WS_PART, 0};
    const int len[4] = {doh_bins(0), doh_bins(1), doh_bins(2), 16};
    for (int i = 0; i < 4; ++i)
        CHECK(off[i] + len[i] <= off[i + 1] && off[i] >= 0, "region %d overlaps the next", i);
    for (int pass = 0; pass < DOH_PASSES; ++pass)
        CHECK(doh_ws_hist(pass) == off[pass] && doh_bins(pass) <= DOH_MAX_BINS && doh_bins(pass) % DOH_CHUNKS == 0, "histogram %d", pass);
    CHECK(DOH_ST_K < 16 && DOH_WS_CLEAR == DOH_WS_PART && DOH_WS_PART % 4 == 0, "state words, clear, alignment");
    CHECK(doh_ws_bytes(2, 28) == (int64_t)(DOH_WS_PART + 2 * 56) * 4 && doh_ws_bytes(0, 5) == -1 && doh_ws_bytes(65536, 32768) == -1,
          "workspace bytes");
    CHECK(doh_shape_ok(12, 19, 128, 256, 512, 1024) && doh_shape_ok(16, 150, 128, 128, 512, 512) && doh_shape_ok(1, 5, 33, 65, 33, 65) &&
              !doh_shape_ok(1, 256, 8, 8, 32, 32) && !doh_shape_ok(1, 19, 8, 8, 4, 32) && !doh_shape_ok(1, 19, 8, 4000, 8, 4000) &&
              !doh_shape_ok(1, 19, 1, 8, 64, 32) && !doh_shape_ok(4, 19, 8, 8, 32768, 32768), "shape test");
    if (fails) {
        printf("%d failures\n", fails);
        return 1;
    }
    printf("ohem plan ok\n");
    return 0;
}
