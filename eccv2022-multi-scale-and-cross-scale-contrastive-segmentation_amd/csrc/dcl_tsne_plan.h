// dcl_tsne_plan.h -- what dcl_tsne.hip, dcl_tsne_capi.cpp and the host tests share: the supported-shape rule, the workgroup and
// partial counts of every launch, the workspace layout of dts_run and the schedule of an iteration.  Host-compilable: no HIP.
#pragma once
#include <stdint.h>

#include "../../include/dcl_tsne.h"

void dts_set_error(const char *fmt, ...);

static inline bool dts_shape_ok(int64_t N, int D, double perplexity)
{
    if (N < 2 || N >= 65536 || D < 1 || D > DTS_MAX_D)
        return false;
    if (!(perplexity > 0.0) || !(perplexity < (double)(N - 1)))
        return false;
    return N * N < (1ll << 31);
}

static inline int dts_ceil_div(int a, int b) { return (a + b - 1) / b; }

static inline int dts_row_in_lds(int N) { return N <= DTS_LDS_ROW ? 1 : 0; }

// symmetrize: tiles per side; the workgroups walk the T * T tile grid with a stride and skip the tiles below the diagonal
static inline int dts_sym_tiles(int N) { return dts_ceil_div(N, DTS_SYM_TILE); }
static inline int dts_sym_groups(int N)
{
    const int64_t t = dts_sym_tiles(N);
    return (int)(t * t < DTS_SYM_GROUPS ? t * t : DTS_SYM_GROUPS);
}

static inline int dts_z_row_blocks(int N) { return dts_ceil_div(N, DTS_Z_ROWS); }
static inline int dts_z_col_chunks(int N) { return dts_ceil_div(N, DTS_Z_COLS); }
static inline int dts_z_parts(int N) { return dts_z_row_blocks(N) * dts_z_col_chunks(N); }

// num_ij == num_ji: a zsum block (row block rb, column chunk cb) whose columns all lie below its rows is skipped (weight 0), its
// mirror cells lie in blocks whose columns all lie above their rows and count twice; a block the diagonal runs through counts
// once.  The two sets are mirror images because a column chunk is a whole number of row blocks.
static_assert(DTS_Z_COLS % DTS_Z_ROWS == 0, "zsum: a column chunk must be a whole number of row blocks");
#ifdef __HIPCC__
#define DTS_HD __host__ __device__
#else
#define DTS_HD
#endif
DTS_HD static inline int dts_z_block_weight(int rb, int cb)
{
    const int64_t r0 = (int64_t)rb * DTS_Z_ROWS, c0 = (int64_t)cb * DTS_Z_COLS;
    return c0 + DTS_Z_COLS <= r0 ? 0 : (c0 >= r0 + DTS_Z_ROWS ? 2 : 1);
}

static inline int dts_grad_groups(int N) { return dts_ceil_div(N, DTS_GRAD_ROWS); }
static inline int dts_upd_groups(int N) { return dts_ceil_div(N, DTS_UPD_ROWS); }

// every row of P starts on 16 bytes when the base does and N is a multiple of 4: then 16-byte loads, else 4-byte ones
static inline int dts_grad_vec(uint64_t p_base, int N) { return (p_base & 15) == 0 && (N % 4) == 0 ? 1 : 0; }

// dts_run's workspace: zpart | klpart | colpart
static inline int64_t dts_ws_z(int N) { (void)N; return 0; }
static inline int64_t dts_ws_kl(int N) { return dts_z_parts(N); }
static inline int64_t dts_ws_col(int N) { return dts_ws_kl(N) + dts_grad_groups(N); }
static inline int64_t dts_ws_floats(int N) { return dts_ws_col(N) + 2 * (int64_t)dts_upd_groups(N); }

// the schedule of iteration it (tsne.py): early exaggeration, momentum switch, KL every tenth iteration
static inline float dts_exaggeration(int it) { return it <= 100 ? 4.f : 1.f; }
static inline float dts_momentum(int it) { return it < 20 ? 0.5f : 0.8f; }
static inline int dts_kl_slot(int it) { return (it + 1) % 10 == 0 ? (it + 1) / 10 - 1 : -1; }
static inline int dts_kl_slots(int n_iter) { return n_iter < 0 ? 0 : n_iter / 10; }
