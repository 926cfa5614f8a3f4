// Stand-alone host program over csrc/dcl_slide_plan.h (tests/test_slide_host.py compiles it with -fsanitize=address,undefined and
// runs it on the CPU): the PASCAL-Context window grid and the cover count on exact-size heap buffers, over a grid of sizes that
// holds exact fits, partial last windows and strides above the crop, and the shape tests at their limits.
#include <stdio.h>
#include <stdlib.h>

#include <vector>

#include "dcl_slide_plan.h"

void dsw_set_error(const char *, ...) {}

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
    for (int crop = 1; crop <= 40; crop += 3)
        for (int n = crop; n <= 90; ++n)                        // the caller pads a shorter axis to the crop
            for (int stride = 1; stride <= 45; stride += 4) {
                const int count = dsw_pc_window_count(n, crop, stride);
                CHECK(count >= 1);
                if (count > DSW_MAX_WIN)
                    continue;
                std::vector<int> lo(count), hi(count);
                for (int r = 0; r < count; ++r) {
                    dsw_pc_window(n, crop, stride, r, &lo[r], &hi[r]);
                    CHECK(lo[r] == r * stride && hi[r] <= n && hi[r] - lo[r] <= crop);
                    CHECK(hi[r] - lo[r] == crop || hi[r] == n);  // only a window that reaches the end is partial
                    ++windows;
                }
                CHECK(hi[count - 1] == n);                       // the last window reaches the end of the axis
                if (lo[count - 1] >= n)
                    continue;                                    // (stride > crop can start a window at the end: refused below)
                std::vector<int32_t> cnt(n), ones(n, 0);
                const int least = dsw_cover(n, crop, lo.data(), count, cnt.data());
                for (int r = 0; r < count; ++r)
                    for (int i = lo[r]; i < hi[r]; ++i)
                        ones[i] += 1;
                int want = count + 1;
                for (int i = 0; i < n; ++i) {
                    CHECK(cnt[i] == ones[i]);
                    want = ones[i] < want ? ones[i] : want;
                }
                CHECK(least == want);
                if (stride <= crop)
                    CHECK(least >= 1);
                CHECK(dsw_cover(n, crop, lo.data(), count, nullptr) == least);
            }
    // fixture pa at scale 1.5: 44 rows, crop 16, stride 10 -> 4 windows, the last one partial
    int lo, hi;
    CHECK(dsw_pc_window_count(44, 16, 10) == 4);
    dsw_pc_window(44, 16, 10, 3, &lo, &hi);
    CHECK(lo == 30 && hi == 44);
    CHECK(dsw_pc_window_count(24, 24, 16) == 1);
    CHECK(dsw_pc_window_count(10, 100, 32) < 1);

    // cover: a hole, a bad start, too many windows
    const int gap[2] = {0, 9};
    std::vector<int32_t> c12(12);
    CHECK(dsw_cover(12, 4, gap, 2, c12.data()) == 0 && c12[3] == 1 && c12[4] == 0 && c12[9] == 1 && c12[11] == 1);
    const int out_of_range[1] = {12}, negative[1] = {-1};
    CHECK(dsw_cover(12, 4, out_of_range, 1, nullptr) == -1 && dsw_cover(12, 4, negative, 1, nullptr) == -1);
    std::vector<int> many(DSW_MAX_WIN + 1, 0);
    CHECK(dsw_cover(4, 4, many.data(), DSW_MAX_WIN, nullptr) == DSW_MAX_WIN);
    CHECK(dsw_cover(12, 4, many.data(), DSW_MAX_WIN + 1, nullptr) == -1);
    const int far[1] = {2147483000};
    CHECK(dsw_cover(2147483647 / 4, 2147483647, far, 1, nullptr) == -1);

    CHECK(dsw_gather_ok(1024, 1, 1, 1, 1, 1, 1, 1, 1) && !dsw_gather_ok(1025, 1, 1, 1, 1, 1, 1, 1, 1));
    CHECK(!dsw_gather_ok(5, 4, 4, 16, 16, DSW_MAX_WIN + 1, 1, 8, 8) && dsw_gather_ok(5, 4, 4, 16, 16, DSW_MAX_WIN, DSW_MAX_WIN, 8, 8));
    CHECK(!dsw_gather_ok(5, 17, 4, 16, 16, 1, 1, 8, 8));                                  // logits larger than the window
    CHECK(dsw_gather_ok(1, 1, 1, 1, 1, 1, 1, (1 << 16) - 1, 1 << 15) && !dsw_gather_ok(1, 1, 1, 1, 1, 1, 1, 1 << 16, 1 << 15));
    CHECK(!dsw_gather_ok(1024, 1 << 10, 1 << 10, 1 << 10, 1 << 10, 2, 1, 8, 8));          // the batch of logits reaches 2^31
    CHECK(dsw_crops_ok(3, 375, 500, 750, 1000, 3, 3, 512, 512) && !dsw_crops_ok(9, 8, 8, 8, 8, 1, 1, 8, 8));
    CHECK(!dsw_crops_ok(0, 8, 8, 8, 8, 1, 1, 8, 8) && !dsw_crops_ok(3, 8, 8, 8, 8, 0, 1, 8, 8));
    CHECK(!dsw_crops_ok(8, 8, 8, 8, 8, DSW_MAX_WIN, DSW_MAX_WIN, 256, 256));              // 2 * 4096 * 8 * 65536 = 2^32
    CHECK(dsw_below_2_31(1 << 15, (1 << 16) - 1, 1, 1) && !dsw_below_2_31(1 << 15, 1 << 16, 1, 1));
    CHECK(!dsw_below_2_31(2147483647, 2147483647, 2147483647, 2147483647));
    printf("plan ok: %ld windows\n", windows);
    return 0;
}
