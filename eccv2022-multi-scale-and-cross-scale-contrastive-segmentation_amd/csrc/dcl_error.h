// dcl_error.h -- the error text of a library, written once.  Every library keeps the message of its last failed call per thread;
// its *_capi.cpp instantiates DCL_DEFINE_ERROR_TEXT(prefix) at file scope and gets
//     void prefix_set_error(const char *fmt, ...)        printf-style, truncates at 511 characters
//     extern "C" const char *prefix_last_error(void)     the text of the calling thread ("" before the first error)
// prefix_set_error takes the linkage and visibility of the declaration the library's own header gave it (dcl_common.h, *_plan.h).
#pragma once
#include <stdarg.h>
#include <stdio.h>

#define DCL_DEFINE_ERROR_TEXT(prefix)                                                                                              \
    static thread_local char g_err[512] = "";                                                                                      \
    void prefix##_set_error(const char *fmt, ...)                                                                                  \
    {                                                                                                                              \
        va_list ap;                                                                                                                \
        va_start(ap, fmt);                                                                                                         \
        vsnprintf(g_err, sizeof(g_err), fmt, ap);                                                                                  \
        va_end(ap);                                                                                                                \
    }                                                                                                                              \
    extern "C" const char *prefix##_last_error(void) { return g_err; }
