// HIP call checks of the host files (engine.cpp, forward.cpp, hooks.cpp): report
// through errorf and leave the enclosing function with false (HIP_OK) or -1 (HIP_RC).
#pragma once

#include "host_common.h"

#include <hip/hip_runtime.h>

#define HIP_CHECK_(expr, ret)                                                                            \
    do {                                                                                                 \
        hipError_t e_ = (expr);                                                                          \
        if (e_ != hipSuccess) {                                                                          \
            emb::errorf("libbert: HIP error %s at %s:%d (%s)\n", hipGetErrorString(e_), __FILE__,        \
                        __LINE__, #expr);                                                                \
            return ret;                                                                                  \
        }                                                                                                \
    } while (0)

#define HIP_OK(expr) HIP_CHECK_(expr, false)
#define HIP_RC(expr) HIP_CHECK_(expr, -1)
