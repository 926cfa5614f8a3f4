// dcl_lovasz_plan.h -- what dcl_lovasz.hip and dcl_lovasz_capi.cpp share: the workspace layout and the error text.
#pragma once
#include <stdint.h>

#include "../../include/dcl_lovasz.h"

void dlv_set_error(const char *fmt, ...);

#define DLV_CHECK_ARG(cond, msg)                              \
    do {                                                      \
        if (!(cond)) {                                        \
            dlv_set_error("%s: %s", __func__, msg);           \
            return DLV_EINVAL;                                \
        }                                                     \
    } while (0)

#define DLV_RADIX 256

// Byte offsets of the workspace's parts (include/dcl_lovasz.h, dlv_workspace_bytes states the same sum).
struct DlvLayout {
    int64_t T, S, L, tps;
    int64_t key[2], pay[2], hist, tot, fgt, part, G, scale, segterm, bytes;
};

static inline int64_t dlv_r256(int64_t x) { return (x + 255) / 256 * 256; }

// false when the shape is outside what the kernels index
static inline bool dlv_layout(int N, int C, int HW, int per_image, DlvLayout *o)
{
    if (N < 1 || C < 1 || C > DLV_MAX_CLASSES || HW < 1)
        return false;
    int64_t P = (int64_t)N * HW, T = P * C;
    if (P >= (1ll << 31) || T >= (1ll << 31))
        return false;
    o->T = T;
    o->S = per_image ? (int64_t)N * C : C;
    o->L = per_image ? HW : P;
    o->tps = (o->L + DLV_TILE - 1) / DLV_TILE;
    int64_t at = 0;
    auto take = [&](int64_t bytes) { int64_t a = at; at += dlv_r256(bytes); return a; };
    o->key[0] = take(4 * T);
    o->key[1] = take(4 * T);
    o->pay[0] = take(4 * T);
    o->pay[1] = take(4 * T);
    o->hist = take(4 * DLV_RADIX * o->S * o->tps);
    o->tot = take(4 * DLV_RADIX * o->S);
    o->fgt = take(4 * o->S * o->tps);
    o->part = take(8 * o->S * o->tps);
    o->G = take(8 * o->S);
    o->scale = take(8 * o->S);
    o->segterm = take(8 * o->S);
    o->bytes = at;
    return true;
}
