// Stand-alone host program over csrc/dcl_tta_plan.h (tests/test_tta_host.py compiles it with -fsanitize=address,undefined and runs it
// on the CPU): every plan function on exact-size heap buffers, over a grid of sizes that holds an axis shorter than the crop, one
// equal to it, remainders that shift the last window back, strides above the crop, and degenerate grids.
#include <stdio.h>
#include <stdlib.h>

#include <vector>

#include "dcl_tta_plan.h"

void dtt_set_error(const char *, ...) {}

#define CHECK(c)                                                   \
    do {                                                           \
        if (!(c)) {                                                \
            printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #c);  \
            return 1;                                              \
        }                                                          \
    } while (0)

int main()
{
    long windows = 0;
    for (int n = 1; n <= 80; ++n)
        for (int crop = 1; crop <= 40; crop += 3)
            for (int stride = 1; stride <= 45; stride += 4) {
                const int count = dtt_window_count(n, crop, stride);
                if (count < 1) {
                    CHECK(n - crop <= -stride);
                    continue;
                }
                std::vector<int32_t> cnt(n), ones(n, 0);
                CHECK(dtt_window_counts(n, crop, stride, cnt.data()) == count);
                int prev_lo = -1;
                for (int r = 0; r < count; ++r) {
                    int lo, hi;
                    dtt_window(n, crop, stride, r, &lo, &hi);
                    CHECK(0 <= lo && lo < hi && hi <= n);
                    CHECK(hi - lo == (crop < n ? crop : n));
                    CHECK(lo >= prev_lo);
                    prev_lo = lo;
                    for (int i = lo; i < hi; ++i)
                        ones[i] += 1;
                    ++windows;
                }
                int lo, hi;
                dtt_window(n, crop, stride, count - 1, &lo, &hi);
                CHECK(hi == n);                                 // the last window ends at the end of the axis
                for (int i = 0; i < n; ++i)
                    CHECK(cnt[i] == ones[i]);
                if (stride <= crop)
                    for (int i = 0; i < n; ++i)
                        CHECK(cnt[i] >= 1);
            }
    // the documented cases: 48 columns, crop 24, stride 16 -> the last of 3 windows shifted back to 24
    int lo, hi;
    CHECK(dtt_window_count(48, 24, 16) == 3);
    dtt_window(48, 24, 16, 2, &lo, &hi);
    CHECK(lo == 24 && hi == 48);
    CHECK(dtt_window_count(24, 32, 32) == 1);
    dtt_window(24, 32, 32, 0, &lo, &hi);
    CHECK(lo == 0 && hi == 24);
    CHECK(dtt_window_count(10, 100, 32) < 1);

    int nh, nw;
    dtt_cts_size(1024, 2048, 2048, 0.75, &nh, &nw);
    CHECK(nh == 768 && nw == 1536);
    dtt_cts_size(20, 40, 48, 1.5, &nh, &nw);
    CHECK(nh == 36 && nw == 72);
    dtt_cts_size(40, 20, 48, 0.5, &nh, &nw);
    CHECK(nh == 24 && nw == 12);
    dtt_cts_size(30, 30, 45, 1.0, &nh, &nw);
    CHECK(nh == 45 && nw == 45);

    for (int in = 1; in <= 40; in += 3)
        for (int out = 1; out <= 90; out += 7)
            for (int align = 0; align < 2; ++align) {
                const float scale = dcl_bilinear_scale(in, out, align);
                std::vector<float> row(in, 1.f);
                int last = 0;
                for (int dst = 0; dst < out; ++dst) {
                    int i0, i1;
                    float l0, l1;
                    dcl_bilinear_src_index(scale, align, dst, in, &i0, &i1, &l0, &l1);
                    CHECK(0 <= i0 && i0 <= i1 && i1 <= in - 1 && i1 - i0 <= 1 && i0 >= last);
                    CHECK(l1 >= 0.f && l0 + l1 > 0.999f && l0 + l1 < 1.001f);
                    CHECK(row[i0] * l0 + row[i1] * l1 > 0.999f);
                    last = i0;
                }
            }

    CHECK(dtt_shape_ok(1024, 1, 1, 1, 1, 1, 1) && !dtt_shape_ok(1025, 1, 1, 1, 1, 1, 1) && !dtt_shape_ok(0, 1, 1, 1, 1, 1, 1));
    CHECK(dtt_shape_ok(19, 512, 1024, 2048, 4096, 1024, 2048));
    CHECK(!dtt_shape_ok(1, 1, 1, 1, 1, 1 << 16, 1 << 15) && dtt_shape_ok(1, 1, 1, 1, 1, (1 << 16) - 1, 1 << 15));
    printf("plan ok: %ld windows\n", windows);
    return 0;
}
