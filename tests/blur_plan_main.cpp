// Stand-alone host program over csrc/dcl_blur_plan.h (tests/test_cadis_host.py compiles it with -fsanitize=address,undefined and
// runs it as a program): the box of every radius against the table the test wrote from its own restatement, the tile walk of the
// three passes against the same passes on the whole axis (every staged buffer is a heap array of exactly dbl_ext values, so a tap
// outside a pass's range is an out-of-bounds read or a read of a NaN), and the reflected row against its definition.
//   usage: blur_plan_main <table>     lines of "radius l ww-bits fw-bits" (the floats as hex words)
#include <cmath>
#include <cstdio>
#include <cstring>
#include <vector>

#include "dcl_blur_plan.h"

void dbl_set_error(const char *, ...) {}

static float pass_at(const std::vector<float> &a, int g, int n, int base, int l, float ww, float fw)
{
    float acc = 0.f;
    for (int d = -l; d <= l; ++d)
        acc += a.at(dbl_tap(g, d, n, base));
    const float e = a.at(dbl_tap(g, -l - 1, n, base)) + a.at(dbl_tap(g, l + 1, n, base));
    return ww * acc + fw * e;
}

static int check_tiles(int n, int T, int radius)
{
    const DblBox b = dbl_box_of(radius);
    std::vector<float> whole(n);
    for (int i = 0; i < n; ++i)
        whole[i] = (float)((i * 37 + radius * 11) % 256);
    std::vector<float> ref = whole;
    for (int p = 0; p < 3; ++p) {
        std::vector<float> next(n);
        for (int g = 0; g < n; ++g)
            next[g] = pass_at(ref, g, n, 0, b.l, b.ww, b.fw);
        ref = next;
    }
    for (int t0 = 0; t0 < n; t0 += T) {
        const int ext = dbl_ext(T, b.l), base = t0 - dbl_halo(b.l);
        std::vector<float> cur(ext, NAN);
        for (int j = 0; j < ext; ++j)
            if (base + j >= 0 && base + j < n)
                cur[j] = whole[base + j];
        for (int p = 1; p <= 3; ++p) {
            std::vector<float> next(ext, NAN);
            for (int j = dbl_pass_lo(p, b.l); j < dbl_pass_hi(p, T, b.l); ++j)
                if (base + j >= 0 && base + j < n)
                    next[j] = pass_at(cur, base + j, n, base, b.l, b.ww, b.fw);
            cur = next;
        }
        for (int x = 0; x < T && t0 + x < n; ++x) {
            const float got = cur.at(dbl_halo(b.l) + x);
            if (std::memcmp(&got, &ref[t0 + x], sizeof(float)) != 0) {
                std::printf("tile walk: n %d T %d radius %d index %d: %.9g != %.9g\n", n, T, radius, t0 + x, got, ref[t0 + x]);
                return 1;
            }
        }
    }
    return 0;
}

int main(int argc, char **argv)
{
    if (argc != 2)
        return 2;
    std::FILE *f = std::fopen(argv[1], "r");
    if (!f)
        return 2;
    int radius, l, rows = 0;
    unsigned ww, fw;
    while (std::fscanf(f, "%d %d %x %x", &radius, &l, &ww, &fw) == 4) {
        const DblBox b = dbl_box_of(radius);
        unsigned gw, gf;
        std::memcpy(&gw, &b.ww, 4);
        std::memcpy(&gf, &b.fw, 4);
        if (b.l != l || gw != ww || gf != fw) {
            std::printf("box of radius %d: l %d ww %08x fw %08x, expected %d %08x %08x\n", radius, b.l, gw, gf, l, ww, fw);
            return 1;
        }
        if (2 * b.l + 3 > 17 || !dbl_blur_ok(1, 1, 1, radius))
            return 1;
        ++rows;
    }
    std::fclose(f);
    if (rows != DBL_MAX_RADIUS)
        return 1;
    const int sizes[] = {1, 2, 5, 7, 33, 64, 65, 131, 300};
    const int tiles[] = {4, 64, 256};
    for (int n : sizes)
        for (int T : tiles)
            for (int r = 1; r <= DBL_MAX_RADIUS; ++r)
                if (check_tiles(n, T, r))
                    return 1;
    for (int h = 1; h <= 9; ++h)
        for (int top = 0; top < h; ++top)
            for (int bottom = 0; bottom < h; ++bottom) {
                if (!dbl_pad_ok(3, h, 5, top, bottom))
                    return 1;
                for (int y = 0; y < h + top + bottom; ++y) {
                    const int want = y < top ? top - y : y < top + h ? y - top : 2 * (h - 1) - (y - top);
                    if (dbl_reflect_row(y, top, h) != want || want < 0 || want >= h) {
                        std::printf("reflect: h %d top %d bottom %d row %d\n", h, top, bottom, y);
                        return 1;
                    }
                }
            }
    if (dbl_pad_ok(3, 4, 5, 4, 0) || dbl_pad_ok(3, 4, 5, 0, -1) || dbl_blur_ok(1, 46341, 46341, 3) || dbl_blur_ok(5, 4, 4, 3) ||
        dbl_blur_ok(1, 4, 4, 0) || dbl_blur_ok(1, 4, 4, DBL_MAX_RADIUS + 1) || !dbl_blur_ok(4, 1, 1, 8))
        return 1;
    std::printf("blur plan ok: %d radii\n", rows);
    return 0;
}
