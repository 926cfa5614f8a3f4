// Stand-alone host program over csrc/dcl_pred_plan.h (tests/test_pred_host.py compiles it with -fsanitize=address,undefined and runs it
// on the CPU).  argv[1] names a table that the test wrote from its Python restatement of the source-index rule, one line per
// output index:
//   in out align dst i0 i1 l0 l1        (weights as the hexadecimal bits of their fp32 value)
// Every line is compared exactly with what the header computes.  Then, for every shape of the GPU tests, the walk of dcl_pred.hip's
// threads is repeated on exact-size heap buffers: each run's taps are read from a [C, h, w] map and its bytes written to the three
// outputs, as 4-byte words where the header says so; every output byte must be written exactly once.  Last, the shape tests.
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <vector>

#include "dcl_pred_plan.h"

void dpr_set_error(const char *, ...) {}

#define CHECK(c)                                                   \
    do {                                                           \
        if (!(c)) {                                                \
            printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #c);  \
            return 1;                                              \
        }                                                          \
    } while (0)

static const int SHAPES[][5] = {{1, 3, 5, 9, 11}, {19, 5, 7, 17, 23}, {19, 8, 12, 32, 48}, {150, 13, 9, 50, 33}, {256, 4, 6, 16, 22},
                                {19, 16, 24, 16, 24}, {3, 1, 1, 7, 5}, {2, 6, 9, 1, 1}};

// the walk of k_predict over one image: returns 0 when every byte of the outputs was written exactly once
static int walk(int C, int h, int w, int H, int W, int align, size_t shift)
{
    std::vector<float> z((size_t)C * h * w);
    for (size_t i = 0; i < z.size(); ++i)
        z[i] = (float)((i * 2654435761u) % 1009) - 504.f;
    // `shift` bytes in front of each output take it off the 4-byte boundary (the storage itself is exact: one byte past is an error)
    std::vector<uint8_t> ids_buf(shift + (size_t)H * W), rgb_buf(shift + (size_t)3 * H * W);
    std::vector<uint8_t> cnt1((size_t)H * W, 0), cnt3((size_t)3 * H * W, 0);
    uint8_t *ids = ids_buf.data() + shift, *rgb = rgb_buf.data() + shift;
    const int runs = dpr_runs(W);
    const int v1 = dpr_vec_ok((uint64_t)(uintptr_t)ids, W), v3 = dpr_vec_ok((uint64_t)(uintptr_t)rgb, W);
    CHECK(runs * DPR_RUN >= W && (runs - 1) * DPR_RUN < W);
    if (shift % 4)
        CHECK(!v1 && !v3);
    const float sy = dcl_bilinear_scale(h, H, align), sx = dcl_bilinear_scale(w, W, align);
    for (int64_t item = 0; item < (int64_t)H * runs; ++item) {
        const int Y = (int)(item / runs), X0 = (int)(item - (int64_t)Y * runs) * DPR_RUN;
        const int n = W - X0 < DPR_RUN ? W - X0 : DPR_RUN;
        CHECK(n >= 1);
        int y0, y1;
        float ly0, ly1;
        dcl_bilinear_src_index(sy, align, Y, h, &y0, &y1, &ly0, &ly1);
        CHECK(0 <= y0 && y0 <= y1 && y1 < h && y1 - y0 <= 1 && ly0 >= 0.f && ly1 >= 0.f && ly0 <= 1.f && ly1 <= 1.f);
        int arg[DPR_RUN];
        for (int k = 0; k < DPR_RUN; ++k) {
            const int X = X0 + k < W - 1 ? X0 + k : W - 1;
            int x0, x1;
            float lx0, lx1;
            dcl_bilinear_src_index(sx, align, X, w, &x0, &x1, &lx0, &lx1);
            CHECK(0 <= x0 && x0 <= x1 && x1 < w && x1 - x0 <= 1 && lx0 >= 0.f && lx1 >= 0.f && lx0 <= 1.f && lx1 <= 1.f);
            float best = 0.f;
            arg[k] = 0;
            for (int c = 0; c < C; ++c) {
                const float *zc = z.data() + (size_t)c * h * w;
                const float v = ly0 * (lx0 * zc[y0 * w + x0] + lx1 * zc[y0 * w + x1]) + ly1 * (lx0 * zc[y1 * w + x0] + lx1 * zc[y1 * w + x1]);
                if (c == 0 || v > best)
                    best = v, arg[k] = c;
            }
            CHECK(arg[k] >= 0 && arg[k] < C && arg[k] < 256);
        }
        const int64_t o = (int64_t)Y * W + X0;
        if (v1 && n == DPR_RUN) {
            CHECK(((uintptr_t)(ids + o) & 3) == 0);
            const uint32_t word = (uint32_t)arg[0] | ((uint32_t)arg[1] << 8) | ((uint32_t)arg[2] << 16) | ((uint32_t)arg[3] << 24);
            memcpy(ids + o, &word, 4);
            for (int k = 0; k < 4; ++k)
                cnt1[o + k] += 1;
        } else {
            CHECK(!v1);
            for (int k = 0; k < n; ++k)
                ids[o + k] = (uint8_t)arg[k], cnt1[o + k] += 1;
        }
        if (v3 && n == DPR_RUN) {
            CHECK(((uintptr_t)(rgb + 3 * o) & 3) == 0);
            uint32_t words[3] = {1, 2, 3};
            memcpy(rgb + 3 * o, words, 12);
            for (int k = 0; k < 12; ++k)
                cnt3[3 * o + k] += 1;
        } else {
            CHECK(!v3);
            for (int k = 0; k < 3 * n; ++k)
                rgb[3 * o + k] = 7, cnt3[3 * o + k] += 1;
        }
    }
    for (size_t i = 0; i < cnt1.size(); ++i)
        CHECK(cnt1[i] == 1);
    for (size_t i = 0; i < cnt3.size(); ++i)
        CHECK(cnt3[i] == 1);
    return 0;
}

int main(int argc, char **argv)
{
    CHECK(argc == 2);
    FILE *f = fopen(argv[1], "r");
    CHECK(f != NULL);
    long lines = 0;
    int in, out, align, dst, i0, i1;
    unsigned b0, b1;
    while (fscanf(f, "%d %d %d %d %d %d %x %x", &in, &out, &align, &dst, &i0, &i1, &b0, &b1) == 8) {
        int g0, g1;
        float l0, l1;
        dcl_bilinear_src_index(dcl_bilinear_scale(in, out, align), align, dst, in, &g0, &g1, &l0, &l1);
        unsigned c0, c1;
        memcpy(&c0, &l0, 4);
        memcpy(&c1, &l1, 4);
        if (g0 != i0 || g1 != i1 || c0 != b0 || c1 != b1) {
            printf("FAILED %d -> %d align %d dst %d: (%d, %d, %08x, %08x) != (%d, %d, %08x, %08x)\n", in, out, align, dst, g0, g1, c0, c1,
                   i0, i1, b0, b1);
            return 1;
        }
        ++lines;
    }
    fclose(f);
    CHECK(lines > 0);

    for (size_t s = 0; s < sizeof(SHAPES) / sizeof(SHAPES[0]); ++s)
        for (int align = 0; align < 2; ++align)
            for (size_t shift = 0; shift < 4; shift += 1) {
                const int *q = SHAPES[s];
                CHECK(dpr_shape_ok(1, q[0], q[1], q[2], q[3], q[4], 1) && dpr_shape_ok(3, q[0], q[1], q[2], q[3], q[4], 1));
                if (walk(q[0], q[1], q[2], q[3], q[4], align, shift))
                    return 1;
            }

    // the shape tests
    CHECK(!dpr_shape_ok(1, 0, 4, 4, 8, 8, 1) && !dpr_shape_ok(1, 257, 4, 4, 8, 8, 1) && dpr_shape_ok(1, 256, 4, 4, 8, 8, 1));
    CHECK(!dpr_shape_ok(0, 19, 4, 4, 8, 8, 1) && !dpr_shape_ok(65536, 19, 4, 4, 8, 8, 1) && dpr_shape_ok(65535, 19, 1, 1, 2, 2, 1));
    CHECK(!dpr_shape_ok(1, 19, 0, 4, 8, 8, 1) && !dpr_shape_ok(1, 19, 4, 4, 8, 0, 1));
    CHECK(!dpr_shape_ok(1, 19, 4, 4, 32768, 65536, 0) && dpr_shape_ok(1, 19, 4, 4, 32768, 65535, 0));       // 2^31 output pixels
    CHECK(!dpr_shape_ok(1, 19, 4, 4, 32768, 65535, 1) && dpr_shape_ok(1, 19, 4, 4, 16384, 43690, 1));       // ... times 3 with colours
    CHECK(!dpr_shape_ok(1, 19, 4, 4, 16384, 43691, 1));
    CHECK(!dpr_shape_ok(1, 256, 2048, 4096, 8, 8, 0) && dpr_shape_ok(1, 255, 2048, 4096, 8, 8, 0));           // 2^31 logits
    CHECK(!dpr_shape_ok(2, 19, 4, 4, 32768, 32768, 0) && dpr_shape_ok(2, 19, 4, 4, 32768, 32767, 0));
    CHECK(dpr_shape_ok(1, 1, 46340, 46340, 46340, 46340, 0) && !dpr_shape_ok(1, 1, 46341, 46341, 8, 8, 0));
    CHECK(!dpr_panel_ok(0, 4, 1) && !dpr_panel_ok(4, 4, 2) && dpr_panel_ok(18, 22, 8) && dpr_panel_ok(18, 22, 4));
    CHECK(dpr_panel_ok(15446, 15446, 1) && !dpr_panel_ok(15447, 15447, 1));                                   // 9 H W < 2^31
    CHECK(dpr_vec_ok(64, 24) && !dpr_vec_ok(65, 24) && !dpr_vec_ok(66, 24) && !dpr_vec_ok(64, 22) && dpr_runs(1) == 1 && dpr_runs(4) == 1);
    CHECK(dpr_runs(5) == 2 && dpr_runs(2147483647) == 536870912);
    // the class slices: a power of two up to 8, every slice at least 8 classes and none empty, together the classes once
    for (int C = 1; C <= DPR_MAX_C; ++C)
        for (int64_t items = 1; items <= (1 << 20); items *= 4)
            for (int N = 1; N <= 3; N += 2) {
                const int split = dpr_class_split(items, N, C), chunk = (C + split - 1) / split;
                CHECK(split == 1 || split == 2 || split == 4 || split == 8);
                CHECK(split == 1 || (C / split >= 8 && ((items + 255) / 256) * N * (split / 2) < 2048));
                CHECK((split - 1) * chunk < C && split * chunk >= C);
            }
    CHECK(dpr_class_split(1024 * 512, 1, 19) == 1 && dpr_class_split(512 * 128, 1, 150) == 8 && dpr_class_split(99, 1, 19) == 2);
    CHECK(dpr_class_split(99, 1, 1) == 1 && dpr_class_split(99, 1, 15) == 1 && dpr_class_split(99, 1, 256) == 8);
    printf("plan ok: %ld lines\n", lines);
    return 0;
}
