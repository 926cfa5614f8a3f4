// dcl_attn_plan.h -- what dcl_attn.hip and dcl_attn_capi.cpp share: the shape test, the workspace layout and the error text.
#pragma once
#include <stdint.h>

#include "../../include/dcl_attn.h"

void dat_set_error(const char *fmt, ...);

#define DAT_CHECK_ARG(cond, msg)                              \
    do {                                                      \
        if (!(cond)) {                                        \
            dat_set_error("%s: %s", __func__, msg);           \
            return DAT_EINVAL;                                \
        }                                                     \
    } while (0)

static inline int64_t dat_r256(int64_t x) { return (x + 255) / 256 * 256; }

static inline bool dat_shape_ok(int B, int N, int heads, int D)
{
    if (B < 1 || N < 1 || heads < 1 || D < 16 || D > DAT_MAX_HEAD_DIM || D % 16 != 0)
        return false;
    if ((int64_t)B * heads > 65535)
        return false;
    return (int64_t)B * N * 3 * heads * D < (1ll << 31);
}

// Byte offsets of the workspace's parts (include/dcl_attn.h, dat_workspace_bytes states the same sum).
struct DatLayout {
    int64_t amax, delta, bytes;
};

static inline bool dat_layout(int B, int N, int heads, int D, int backward, DatLayout *o)
{
    if (!dat_shape_ok(B, N, heads, D))
        return false;
    o->amax = 0;
    o->delta = dat_r256(16ll * B * heads);
    o->bytes = o->delta + (backward ? dat_r256(4ll * B * heads * N) : 0);
    return true;
}
