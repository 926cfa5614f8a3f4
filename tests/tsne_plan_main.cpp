// Stand-alone host program over csrc/dcl_tsne_plan.h, built with -fsanitize=address,undefined by tests/test_tsne_host.py: the shape
// rule at each limit, every count covering its N with no workgroup to spare, the workspace regions of dts_run disjoint and inside
// dts_ws_floats, the walk of the symmetrize tile grid visiting every tile pair exactly once, the zsum block weights counting every
// pair once, and tsne.py's schedule.
#include <math.h>
#include <stdio.h>
#include <stdlib.h>
#include <vector>

#include "dcl_tsne_plan.h"

void dts_set_error(const char *, ...) {}

#define CHECK(c)                                                                                                                   \
    do {                                                                                                                           \
        if (!(c)) {                                                                                                                \
            printf("FAILED line %d: %s\n", __LINE__, #c);                                                                          \
            return 1;                                                                                                              \
        }                                                                                                                          \
    } while (0)

int main()
{
    // the shape rule
    CHECK(dts_shape_ok(19000, 50, 30.0) && dts_shape_ok(4000, 50, 30.0) && dts_shape_ok(33, 2, 5.0));
    CHECK(dts_shape_ok(46340, 1, 30.0) && !dts_shape_ok(46341, 1, 30.0) && !dts_shape_ok(1ll << 40, 1, 30.0));
    CHECK(dts_shape_ok(100, DTS_MAX_D, 30.0) && !dts_shape_ok(100, DTS_MAX_D + 1, 30.0) && !dts_shape_ok(100, 0, 30.0));
    CHECK(!dts_shape_ok(32, 2, 31.0) && dts_shape_ok(32, 2, 30.999) && !dts_shape_ok(32, 2, 0.0) && !dts_shape_ok(32, 2, -1.0));
    CHECK(!dts_shape_ok(32, 2, NAN) && !dts_shape_ok(1, 2, 0.5) && !dts_shape_ok(0, 2, 0.5) && !dts_shape_ok(-5, 2, 0.5));

    const int sizes[] = {2, 3, 7, 8, 9, 31, 32, 33, 130, 255, 256, 257, 1023, 1024, 1025, 4000, 8191, 8192, 8193, 19000, 46340};
    for (int N : sizes) {
        CHECK(dts_row_in_lds(N) == (N <= DTS_LDS_ROW));
        const int T = dts_sym_tiles(N), G = dts_sym_groups(N);
        CHECK((int64_t)T * DTS_SYM_TILE >= N && (int64_t)(T - 1) * DTS_SYM_TILE < N);
        CHECK(G >= 1 && G <= DTS_SYM_GROUPS && (int64_t)G <= (int64_t)T * T);
        CHECK((int64_t)T * T < (1ll << 31));
        if (T <= 64) {                                       // the strided walk of k_sym: every pair bi <= bj exactly once
            std::vector<int> seen((size_t)T * T, 0);
            for (int g = 0; g < G; ++g)
                for (int t = g; t < T * T; t += G) {
                    const int bi = t / T, bj = t - bi * T;
                    if (bi > bj)
                        continue;
                    seen[(size_t)bi * T + bj] += 1;
                }
            for (int bi = 0; bi < T; ++bi)
                for (int bj = 0; bj < T; ++bj)
                    CHECK(seen[(size_t)bi * T + bj] == (bi <= bj ? 1 : 0));
        }
        CHECK((int64_t)dts_z_row_blocks(N) * DTS_Z_ROWS >= N && (int64_t)(dts_z_row_blocks(N) - 1) * DTS_Z_ROWS < N);
        CHECK((int64_t)dts_z_col_chunks(N) * DTS_Z_COLS >= N && (int64_t)(dts_z_col_chunks(N) - 1) * DTS_Z_COLS < N);
        CHECK(dts_z_parts(N) == dts_z_row_blocks(N) * dts_z_col_chunks(N) && dts_z_col_chunks(N) <= 65535);
        CHECK((int64_t)dts_grad_groups(N) * DTS_GRAD_ROWS >= N && (int64_t)(dts_grad_groups(N) - 1) * DTS_GRAD_ROWS < N);
        CHECK((int64_t)dts_upd_groups(N) * DTS_UPD_ROWS >= N && (int64_t)(dts_upd_groups(N) - 1) * DTS_UPD_ROWS < N);
        // workspace: zpart | klpart | colpart, back to back
        CHECK(dts_ws_z(N) == 0 && dts_ws_kl(N) == dts_ws_z(N) + dts_z_parts(N));
        CHECK(dts_ws_col(N) == dts_ws_kl(N) + dts_grad_groups(N));
        CHECK(dts_ws_floats(N) == dts_ws_col(N) + 2 * (int64_t)dts_upd_groups(N));
        // 16-byte loads need both the base and every row start on 16 bytes
        for (uint64_t base = 4096; base < 4096 + 32; base += 4)
            CHECK(dts_grad_vec(base, N) == ((base % 16 == 0 && N % 4 == 0) ? 1 : 0));
    }

    // zsum: with the block weights every ordered pair (i, j) is counted once: weight(i, j) + weight(j, i) == 2
    for (int N : {33, 257, 1024, 1025, 1300, 2600}) {
        const int RB = dts_z_row_blocks(N), CB = dts_z_col_chunks(N);
        for (int rb = 0; rb < RB; ++rb)
            for (int cb = 0; cb < CB; ++cb)
                CHECK(dts_z_block_weight(rb, cb) >= 0 && dts_z_block_weight(rb, cb) <= 2);
        for (int i = 0; i < N; ++i)
            for (int j = 0; j < N; ++j)
                CHECK(dts_z_block_weight(i / DTS_Z_ROWS, j / DTS_Z_COLS) + dts_z_block_weight(j / DTS_Z_ROWS, i / DTS_Z_COLS) == 2);
    }

    // tsne.py's schedule
    CHECK(dts_exaggeration(0) == 4.f && dts_exaggeration(100) == 4.f && dts_exaggeration(101) == 1.f);
    CHECK(dts_momentum(0) == 0.5f && dts_momentum(19) == 0.5f && dts_momentum(20) == 0.8f);
    int slots = 0;
    for (int it = 0; it < 2000; ++it) {
        const int s = dts_kl_slot(it);
        CHECK((s >= 0) == ((it + 1) % 10 == 0));
        if (s >= 0) {
            CHECK(s == slots && s < dts_kl_slots(2000));
            ++slots;
        }
    }
    CHECK(slots == dts_kl_slots(2000) && dts_kl_slots(9) == 0 && dts_kl_slots(10) == 1 && dts_kl_slots(-3) == 0);
    printf("plan ok\n");
    return 0;
}
