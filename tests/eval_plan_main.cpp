// Stand-alone host program over csrc/dcl_eval_plan.h and csrc/dcl_eval_capi.cpp (tests/test_eval_host.py compiles it with
// -fsanitize=address,undefined and runs it on the CPU).  argv[1] names a table that the test wrote from its Python restatement of
// the two-stage taps, one line per output index of one axis:
//   in mid crop out align_mid align_out dst j0 j1 m0 m1 i0 i1 i2 i3 l0 l1 l2 l3     (weights as the hexadecimal bits of their fp32 value)
// Every line is compared exactly with what dve_plan_taps computes, and held to the invariants: stage-2 indices inside the crop,
// stage-1 indices inside the input, weights of a pair summing to 1.  Then, for every shape of the GPU tests, the walk of
// dcl_eval.hip's threads is repeated on exact-size heap buffers: each run's taps are read from a [C, h, w] map, its labels from an
// [H0, W0] map, and its bytes written to ids, as 4-byte words where the header says so; every byte must be written exactly once.
// Last, the shape test and the small rules.
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <vector>

#include "dcl_eval_capi.cpp"

#define CHECK(c)                                                   \
    do {                                                           \
        if (!(c)) {                                                \
            printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #c);  \
            return 1;                                              \
        }                                                          \
    } while (0)

//                              C  h  w  a1 Hp  Wp  rh  rw  H0  W0  a2       (h = 0: dense)
static const int CASES[][11] = {{150, 8, 12, 0, 32, 48, 29, 43, 37, 55, 0}, {19, 8, 16, 1, 32, 64, 32, 64, 21, 45, 1},
                                {150, 0, 0, 0, 32, 32, 23, 32, 50, 70, 0},  {256, 4, 6, 1, 16, 24, 13, 21, 16, 22, 0},
                                {1, 3, 5, 0, 12, 20, 9, 17, 11, 19, 0},     {19, 5, 7, 0, 20, 28, 17, 23, 64, 96, 1},
                                {19, 0, 0, 0, 16, 24, 16, 24, 16, 24, 0},   {2, 8, 8, 0, 32, 32, 1, 1, 5, 7, 0},
                                {19, 8, 8, 0, 32, 32, 31, 30, 1, 1, 1}};

static unsigned bits(float v)
{
    unsigned b;
    memcpy(&b, &v, 4);
    return b;
}

// the walk of k_evaluate over one image: returns 0 when every byte of ids was written exactly once and every label read once
static int walk(const int *q, size_t shift)
{
    const int C = q[0] < 3 ? q[0] : 3, a1 = q[3], Hp = q[4], Wp = q[5], rh = q[6], rw = q[7], H0 = q[8], W0 = q[9], a2 = q[10];
    const int h = q[1] ? q[1] : Hp, w = q[2] ? q[2] : Wp;
    std::vector<float> z((size_t)C * h * w);
    for (size_t i = 0; i < z.size(); ++i)
        z[i] = (float)((i * 2654435761u) % 1009) - 504.f;
    std::vector<uint8_t> label((size_t)H0 * W0, 1), ids_buf(shift + (size_t)H0 * W0), cnt((size_t)H0 * W0, 0), seen((size_t)H0 * W0, 0);
    uint8_t *ids = ids_buf.data() + shift;
    const int runs = dve_runs(W0), vec = dve_vec_ok((uint64_t)(uintptr_t)ids, W0);
    CHECK(runs * DVE_RUN >= W0 && (runs - 1) * DVE_RUN < W0);
    if (shift % 4)
        CHECK(!vec);
    const float sy1 = dcl_bilinear_scale(h, Hp, a1), sx1 = dcl_bilinear_scale(w, Wp, a1);
    const float sy2 = dcl_bilinear_scale(rh, H0, a2), sx2 = dcl_bilinear_scale(rw, W0, a2);
    for (int64_t item = 0; item < (int64_t)H0 * runs; ++item) {
        const int Y = (int)(item / runs), X0 = (int)(item - (int64_t)Y * runs) * DVE_RUN;
        const int n = W0 - X0 < DVE_RUN ? W0 - X0 : DVE_RUN;
        CHECK(n >= 1);
        const DveTap ty = dve_tap(rh, H0, sy2, a2, Y);
        CHECK(0 <= ty.i0 && ty.i0 <= ty.i1 && ty.i1 < rh);
        const int rows[2] = {ty.i0, ty.i1};
        int arg[DVE_RUN];
        for (int k = 0; k < DVE_RUN; ++k) {
            const int X = X0 + k < W0 - 1 ? X0 + k : W0 - 1;
            const DveTap tx = dve_tap(rw, W0, sx2, a2, X);
            CHECK(0 <= tx.i0 && tx.i0 <= tx.i1 && tx.i1 < rw);
            const int colsx[2] = {tx.i0, tx.i1};
            float best = 0.f;
            arg[k] = 0;
            for (int c = 0; c < C; ++c) {
                const float *zc = z.data() + (size_t)c * h * w;
                float s[2][2];
                for (int r = 0; r < 2; ++r)
                    for (int j = 0; j < 2; ++j) {
                        const DveTap r1 = dve_tap(h, Hp, sy1, a1, rows[r]), q1 = dve_tap(w, Wp, sx1, a1, colsx[j]);
                        CHECK(0 <= r1.i0 && r1.i0 <= r1.i1 && r1.i1 < h && 0 <= q1.i0 && q1.i0 <= q1.i1 && q1.i1 < w);
                        s[r][j] = r1.l0 * (q1.l0 * zc[r1.i0 * w + q1.i0] + q1.l1 * zc[r1.i0 * w + q1.i1]) +
                                  r1.l1 * (q1.l0 * zc[r1.i1 * w + q1.i0] + q1.l1 * zc[r1.i1 * w + q1.i1]);
                    }
                const float v = ty.l0 * (tx.l0 * s[0][0] + tx.l1 * s[0][1]) + ty.l1 * (tx.l0 * s[1][0] + tx.l1 * s[1][1]);
                if (c == 0 || v > best)
                    best = v, arg[k] = c;
            }
            CHECK(arg[k] >= 0 && arg[k] < C);
        }
        const int64_t o = (int64_t)Y * W0 + X0;
        for (int k = 0; k < n; ++k)
            seen[o + k] += label[o + k];
        if (vec && n == DVE_RUN) {
            CHECK(((uintptr_t)(ids + o) & 3) == 0);
            const uint32_t word = (uint32_t)arg[0] | ((uint32_t)arg[1] << 8) | ((uint32_t)arg[2] << 16) | ((uint32_t)arg[3] << 24);
            memcpy(ids + o, &word, 4);
            for (int k = 0; k < 4; ++k)
                cnt[o + k] += 1;
        } else {
            CHECK(!vec);
            for (int k = 0; k < n; ++k)
                ids[o + k] = (uint8_t)arg[k], cnt[o + k] += 1;
        }
    }
    for (size_t i = 0; i < cnt.size(); ++i)
        CHECK(cnt[i] == 1 && seen[i] == 1);
    return 0;
}

int main(int argc, char **argv)
{
    CHECK(argc == 2);
    FILE *f = fopen(argv[1], "r");
    CHECK(f != NULL);
    long lines = 0;
    int in, mid, crop, out, a1, a2, dst, j[2], i[4];
    unsigned m[2], l[4];
    while (fscanf(f, "%d %d %d %d %d %d %d %d %d %x %x %d %d %d %d %x %x %x %x", &in, &mid, &crop, &out, &a1, &a2, &dst, &j[0], &j[1],
                  &m[0], &m[1], &i[0], &i[1], &i[2], &i[3], &l[0], &l[1], &l[2], &l[3]) == 19) {
        int gj[2], gi[4];
        float gm[2], gl[4];
        CHECK(dve_plan_taps(in, mid, crop, out, a1, a2, dst, gj, gm, gi, gl) == DVE_OK);
        bool same = gj[0] == j[0] && gj[1] == j[1] && bits(gm[0]) == m[0] && bits(gm[1]) == m[1];
        for (int k = 0; k < 4; ++k)
            same = same && gi[k] == i[k] && bits(gl[k]) == l[k];
        if (!same) {
            printf("FAILED %d -> %d, [0, %d) -> %d align %d %d dst %d: (%d %d | %d %d %d %d) != (%d %d | %d %d %d %d) or a weight\n", in,
                   mid, crop, out, a1, a2, dst, gj[0], gj[1], gi[0], gi[1], gi[2], gi[3], j[0], j[1], i[0], i[1], i[2], i[3]);
            return 1;
        }
        // the invariants: stage 2 never leaves the crop (so never touches the padded part of stage 1), stage 1 never the input
        CHECK(0 <= gj[0] && gj[0] <= gj[1] && gj[1] <= crop - 1 && gj[1] - gj[0] <= 1);
        CHECK(fabsf(gm[0] + gm[1] - 1.f) <= 1.2e-7f && gm[0] >= 0.f && gm[1] >= 0.f);
        for (int k = 0; k < 2; ++k) {
            CHECK(0 <= gi[2 * k] && gi[2 * k] <= gi[2 * k + 1] && gi[2 * k + 1] <= in - 1 && gi[2 * k + 1] - gi[2 * k] <= 1);
            CHECK(fabsf(gl[2 * k] + gl[2 * k + 1] - 1.f) <= 1.2e-7f && gl[2 * k] >= 0.f && gl[2 * k + 1] >= 0.f);
        }
        ++lines;
    }
    fclose(f);
    CHECK(lines > 0);
    int gj[2], gi[4];
    float gm[2], gl[4];
    CHECK(dve_plan_taps(4, 16, 17, 8, 0, 0, 0, gj, gm, gi, gl) != 0 && dve_plan_taps(4, 16, 8, 8, 0, 0, 8, gj, gm, gi, gl) != 0);
    CHECK(dve_plan_taps(4, 16, 8, 8, 0, 0, 0, NULL, gm, gi, gl) != 0 && dve_last_error()[0] != 0);

    for (size_t s = 0; s < sizeof(CASES) / sizeof(CASES[0]); ++s)
        for (size_t shift = 0; shift < 4; ++shift) {
            const int *q = CASES[s];
            const int h = q[1] ? q[1] : q[4], w = q[2] ? q[2] : q[5];
            CHECK(dve_supported(q[0], h, w, q[4], q[5], q[6], q[7], q[8], q[9], q[0]) == 1);
            CHECK(dve_supported(q[0], h, w, q[4], q[5], q[6], q[7], q[8], q[9], q[0] + 1) == 1);
            if (walk(q, shift))
                return 1;
        }

    // the shape test, at and beyond each limit
    CHECK(!dve_shape_ok(0, 4, 4, 8, 8, 8, 8, 9, 9, 0) && !dve_shape_ok(257, 4, 4, 8, 8, 8, 8, 9, 9, 257));
    CHECK(dve_shape_ok(256, 4, 4, 8, 8, 8, 8, 9, 9, 256) && dve_shape_ok(256, 4, 4, 8, 8, 8, 8, 9, 9, 257));
    CHECK(!dve_shape_ok(19, 4, 4, 8, 8, 8, 8, 9, 9, 18) && !dve_shape_ok(19, 4, 4, 8, 8, 8, 8, 9, 9, 21));
    CHECK(!dve_shape_ok(19, 0, 4, 8, 8, 8, 8, 9, 9, 19) && !dve_shape_ok(19, 4, 4, 8, 0, 8, 8, 9, 9, 19));
    CHECK(!dve_shape_ok(19, 4, 4, 8, 8, 0, 8, 9, 9, 19) && !dve_shape_ok(19, 4, 4, 8, 8, 8, 8, 9, 0, 19));
    CHECK(!dve_shape_ok(1, 4, 4, 8, 8, 8, 8, 32768, 65536, 1) && dve_shape_ok(1, 4, 4, 8, 8, 8, 8, 32768, 65535, 1));     // H0 * W0
    CHECK(!dve_shape_ok(2, 4, 4, 8, 8, 8, 8, 32768, 32768, 2) && dve_shape_ok(2, 4, 4, 8, 8, 8, 8, 32768, 32767, 2));     // C * H0 * W0
    CHECK(!dve_shape_ok(256, 2048, 4096, 8, 8, 8, 8, 9, 9, 256) && dve_shape_ok(255, 2048, 4096, 8, 8, 8, 8, 9, 9, 255)); // C * h * w
    CHECK(!dve_shape_ok(256, 4, 4, 2048, 4096, 8, 8, 9, 9, 256) && dve_shape_ok(255, 4, 4, 2048, 4096, 8, 8, 9, 9, 255)); // C * Hp * Wp
    CHECK(dve_shape_ok(1, 46340, 46340, 46340, 46340, 1, 1, 46340, 46340, 1) && !dve_shape_ok(1, 46341, 46341, 8, 8, 8, 8, 9, 9, 1));
    CHECK(dve_vec_ok(64, 24) && !dve_vec_ok(65, 24) && !dve_vec_ok(66, 24) && !dve_vec_ok(64, 22) && dve_runs(1) == 1 && dve_runs(4) == 1);
    CHECK(dve_runs(5) == 2 && dve_runs(2147483647) == 536870912);
    CHECK(dve_hist_in_lds(19, 20) && dve_hist_in_lds(64, 64) && !dve_hist_in_lds(64, 65) && !dve_hist_in_lds(150, 151));
    // the class slices: a power of two up to 8, every slice at least 8 classes and none empty, together the classes once
    for (int C = 1; C <= DVE_MAX_C; ++C)
        for (int64_t items = 1; items <= (1 << 20); items *= 4) {
            const int split = dve_class_split(items, C), chunk = (C + split - 1) / split;
            CHECK(split == 1 || split == 2 || split == 4 || split == 8);
            CHECK(split == 1 || (C / split >= 8 && ((items + 255) / 256) * (split / 2) < 2048));
            CHECK((split - 1) * chunk < C && split * chunk >= C);
        }
    printf("plan ok: %ld lines\n", lines);
    return 0;
}
