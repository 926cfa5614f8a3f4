// Stand-alone host program over csrc/dcl_aug_plan.h (tests/test_aug_host.py compiles it with -fsanitize=address,undefined and runs it
// on the CPU).  argv[1] names a table that the test wrote from its Python restatement of the rules, one line per output index:
//   S D o k0 n nearest w[0] .. w[n-1]        (weights as the hexadecimal bits of their fp32 value)
// Every line is compared exactly with what the header computes, on exact-size heap buffers; then the tap rules' invariants over a
// grid of sizes, the pad / crop / flip composition and the plan test.
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <vector>

#include "dcl_aug_plan.h"

void dau_set_error(const char *, ...) {}

#define CHECK(c)                                                   \
    do {                                                           \
        if (!(c)) {                                                \
            printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #c);  \
            return 1;                                              \
        }                                                          \
    } while (0)

static dau_plan base_plan()
{
    dau_plan p;
    memset(&p, 0, sizeof(p));
    p.H = 37, p.W = 53, p.rh = 20, p.rw = 30, p.Hc = 32, p.Wc = 48, p.pt = 5, p.pl = 7, p.h = 16, p.w = 24;
    p.P = 2, p.ci[0] = 0, p.cj[0] = 0, p.ci[1] = 16, p.cj[1] = 24;
    p.ncolor = 4, p.perm[0] = 2, p.perm[1] = 0, p.perm[2] = 1, p.perm[3] = 3;
    p.b = p.c = p.s = 1.f, p.ignore = 19, p.max_ratio = 0.75, p.normalise = 1;
    return p;
}

int main(int argc, char **argv)
{
    CHECK(argc == 2);
    FILE *f = fopen(argv[1], "r");
    CHECK(f != NULL);
    long lines = 0;
    int S, D, o, k0, n, nearest;
    while (fscanf(f, "%d %d %d %d %d %d", &S, &D, &o, &k0, &n, &nearest) == 6) {
        std::vector<unsigned> want(n);
        for (int k = 0; k < n; ++k)
            CHECK(fscanf(f, "%x", &want[k]) == 1);
        const DauAxis a = dau_axis(S, D);
        int lo, hi;
        double centre;
        const double sum = dau_tap_range(a, o, &lo, &hi, &centre);
        CHECK(lo == k0 && hi - lo == n && sum > 0.0);
        for (int k = lo; k < hi; ++k) {
            const float w = dau_tap_weight(a, centre, sum, k);
            unsigned bits;
            memcpy(&bits, &w, 4);
            if (bits != want[k - lo]) {
                printf("FAILED weight %d -> %d, o %d, tap %d: %08x != %08x\n", S, D, o, k, bits, want[k - lo]);
                return 1;
            }
        }
        CHECK(dau_nearest(S, D, o) == nearest);
        ++lines;
    }
    fclose(f);
    CHECK(lines > 0);

    // invariants over every scale the kernels take
    for (int s = 1; s <= 70; s += 3)
        for (int d = 1; d <= 8 * s && d <= 150; d += (d < 12 ? 1 : 7)) {
            if (!dau_scale_ok(s, d))
                continue;
            const DauAxis a = dau_axis(s, d);
            std::vector<float> row(s, 1.f);
            int last_near = 0;
            for (int x = 0; x < d; ++x) {
                int lo, hi;
                double centre;
                const double sum = dau_tap_range(a, x, &lo, &hi, &centre);
                CHECK(0 <= lo && lo < hi && hi <= s && hi - lo <= DAU_MAX_TAPS && sum > 0.0);
                float acc = 0.f;
                for (int k = lo; k < hi; ++k)
                    acc += dau_tap_weight(a, centre, sum, k) * row[k];
                CHECK(acc > 0.9999f && acc < 1.0001f);
                const int nn = dau_nearest(s, d, x);
                CHECK(0 <= nn && nn < s && nn >= last_near);
                last_near = nn;
            }
        }
    CHECK(!dau_scale_ok(9, 1) && dau_scale_ok(8, 1) && dau_scale_ok(1, 8) && !dau_scale_ok(1, 9) && !dau_scale_ok(0, 1));
    // the 64-bit branch of the nearest index agrees with the 32-bit one's rule
    CHECK(dau_nearest(60000, 50000, 49999) == (int)(((2ll * 49999 + 1) * 60000) / (2ll * 50000)));
    CHECK(dau_src_col(0, 53, 1) == 52 && dau_src_col(52, 53, 1) == 0 && dau_src_col(7, 53, 0) == 7);

    // pad / crop composition and the label lookup on exact-size buffers
    dau_plan p = base_plan();
    CHECK(dau_plan_ok(&p));
    std::vector<uint8_t> lbl((size_t)p.H * p.W), lut(256);
    for (size_t i = 0; i < lbl.size(); ++i)
        lbl[i] = (uint8_t)(i % 251);
    for (int i = 0; i < 256; ++i)
        lut[i] = (uint8_t)(255 - i);
    for (int flip = 0; flip < 2; ++flip) {
        p.flip = flip;
        long inside = 0;
        for (int c = 0; c < p.P; ++c)
            for (int y = 0; y < p.h; ++y)
                for (int x = 0; x < p.w; ++x) {
                    int ry, rx;
                    if (!dau_crop_to_resized(p, c, y, x, &ry, &rx))
                        continue;
                    ++inside;
                    const int sy = ((2 * ry + 1) * p.H) / (2 * p.rh), sx = ((2 * rx + 1) * p.W) / (2 * p.rw);
                    CHECK(dau_label_at(lbl.data(), lut.data(), p, ry, rx) == lut[lbl[(size_t)sy * p.W + (flip ? p.W - 1 - sx : sx)]]);
                }
        CHECK(inside == (16 - 5) * (24 - 7) + (25 - 16) * (37 - 24));
    }

    // verdicts and the choice
    CHECK(dau_verdict(2, 2, 4, 0.75) == 1 && dau_verdict(2, 3, 4, 0.75) == 0 && dau_verdict(1, 4, 4, 0.75) == 0);
    CHECK(dau_verdict(0, 0, 0, 0.75) == 0);
    std::vector<int32_t> ws(3 * DAU_MAX_CAND, 0);
    CHECK(dau_chosen(ws.data(), 10) == 9 && dau_chosen(ws.data(), 1) == 0);
    ws[3 * 6] = 1;
    CHECK(dau_chosen(ws.data(), 10) == 6);
    ws[0] = 1;
    CHECK(dau_chosen(ws.data(), 10) == 0);

    // the plan test
    dau_plan q = base_plan();
    q.rh = 4;                                       // 37 -> 4: beyond 1/8
    CHECK(!dau_plan_ok(&q));
    q = base_plan();
    q.h = 33;                                       // crop larger than the canvas
    CHECK(!dau_plan_ok(&q));
    q = base_plan();
    q.P = 11;
    CHECK(!dau_plan_ok(&q));
    q = base_plan();
    q.cj[1] = 25;                                   // candidate outside the canvas
    CHECK(!dau_plan_ok(&q));
    q = base_plan();
    q.pt = 13;                                      // resized image outside the canvas
    CHECK(!dau_plan_ok(&q));
    q = base_plan();
    q.perm[1] = 2;                                  // an operation twice
    CHECK(!dau_plan_ok(&q));
    q = base_plan();
    CHECK(dau_contrast_pos(q) == 2);
    q.ncolor = 2;
    CHECK(dau_plan_ok(&q) && dau_contrast_pos(q) == -1);
    CHECK(!dau_plan_ok(NULL));
    printf("plan ok: %ld lines\n", lines);
    return 0;
}
