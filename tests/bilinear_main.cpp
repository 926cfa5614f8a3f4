// Stand-alone host program over csrc/dcl_bilinear.h (tests/test_bilinear_host.py compiles it with -fsanitize=address,undefined and
// runs it on the CPU).  For every (in, out, align) of a dense grid and of the up- and down-sampling shapes the kernels meet:
//   * the source index pair and weights are well formed and monotonic;
//   * dcl_bilinear_weight is exactly the sum of the weights whose index is the asked one;
//   * dcl_bilinear_out_range covers every output with a non-zero weight.  That is a hard condition: the gather-form backward passes
//     of dcl_resize.hip and dcl_upce.hip sum over that range only, so one output outside it is a gradient term dropped silently.
#include <stdio.h>

#include "dcl_bilinear.h"

#define CHECK(c)                                                                                                 \
    do {                                                                                                         \
        if (!(c)) {                                                                                              \
            printf("FAILED %s:%d: %s (in %d, out %d, align %d)\n", __FILE__, __LINE__, #c, in, out, align);      \
            return 1;                                                                                            \
        }                                                                                                        \
    } while (0)

static long long g_pairs = 0;

static int walk(int in, int out, int align)
{
    const float scale = dcl_bilinear_scale(in, out, align);
    int last = 0;
    for (int dst = 0; dst < out; ++dst) {
        int i0, i1;
        float l0, l1;
        dcl_bilinear_src_index(scale, align, dst, in, &i0, &i1, &l0, &l1);
        CHECK(0 <= i0 && i0 <= i1 && i1 <= in - 1 && i1 - i0 <= 1 && i0 >= last);
        CHECK(l1 >= 0.f && l0 + l1 > 0.999f && l0 + l1 < 1.001f);
        last = i0;
    }
    for (int i = 0; i < in; ++i) {
        int lo, hi;
        dcl_bilinear_out_range(scale, align, i, in, out, &lo, &hi);
        CHECK(0 <= lo && hi <= out - 1);
        for (int o = 0; o < out; ++o) {
            int i0, i1;
            float l0, l1;
            dcl_bilinear_src_index(scale, align, o, in, &i0, &i1, &l0, &l1);
            const float w = dcl_bilinear_weight(scale, align, o, in, i);
            CHECK(w == (i0 == i ? l0 : 0.f) + (i1 == i ? l1 : 0.f));
            if (w != 0.f)
                CHECK(lo <= o && o <= hi);
            ++g_pairs;
        }
    }
    return 0;
}

int main()
{
    for (int align = 0; align < 2; ++align)
        for (int in = 1; in <= 64; ++in)
            for (int out = 1; out <= 200; ++out)
                if (walk(in, out, align))
                    return 1;
    const int shapes[][2] = {{256, 1024}, {512, 2048}, {1024, 2048}, {128, 1024}, {257, 1025}, {1000, 333}, {2048, 512}};
    for (int align = 0; align < 2; ++align)
        for (const auto &s : shapes)
            if (walk(s[0], s[1], align))
                return 1;
    printf("bilinear ok: %lld index pairs\n", g_pairs);
    return 0;
}
