// dcl_ocr_plan.h -- what dcl_ocr.hip and dcl_ocr_capi.cpp share: the shape test, the split count, the workspace size, the error text.
#pragma once
#include <stdint.h>

#include "../../include/dcl_ocr.h"

void dco_set_error(const char *fmt, ...);

static inline int64_t dco_r256(int64_t x) { return (x + 255) / 256 * 256; }

static inline bool dco_shape_ok(int B, int C, int K, int N)
{
    if (B < 1 || B > DCO_MAX_B || N < 1 || K < 1 || K > DCO_MAX_K || C < 16 || C > DCO_MAX_C || C % 16 != 0)
        return false;
    return (int64_t)B * C * N < (1ll << 31) && (int64_t)B * K * N < (1ll << 31);
}

static inline int dco_tiles(int N) { return (N + DCO_TILE_N - 1) / DCO_TILE_N; }
static inline int dco_chunks(int C) { return (C + DCO_CHUNK_C - 1) / DCO_CHUNK_C; }

static inline int dco_split_count(int B, int C, int N)
{
    if (B < 1 || C < 1 || N < 1)
        return 0;
    const int64_t bc = (int64_t)B * dco_chunks(C);
    int64_t want = (512 + bc - 1) / bc;
    if (want < 1)
        want = 1;
    if (want > DCO_MAX_SPLIT)
        want = DCO_MAX_SPLIT;
    const int64_t tiles = dco_tiles(N);
    if (want > tiles)
        want = tiles;
    const int64_t per = (tiles + want - 1) / want;      // tiles of one split; then no split is left empty
    return (int)((tiles + per - 1) / per);
}

static inline int64_t dco_ws_bytes(int op, int B, int C, int K, int N)
{
    if (!dco_shape_ok(B, C, K, N))
        return -1;
    const int64_t sp = dco_split_count(B, C, N);
    switch (op) {
    case DCO_OP_GATHER_FWD: return dco_r256(4ll * B * sp * K * C);
    case DCO_OP_GATHER_BWD: return 0;
    case DCO_OP_ATTN_FWD: return 0;
    case DCO_OP_ATTN_BWD: return dco_r256(8ll * B * sp * C * K);
    }
    return -1;
}
