/* jx_hip.h -- what only the HIP translation units share (jpgx_plan.cpp is built by plain g++
 * without the HIP headers and does not include this) */
#ifndef JX_HIP_H
#define JX_HIP_H
#include <hip/hip_runtime.h>

#include "../../include/jpgx.h"
#define JX_MAX_DEV 64       /* devices with state of their own (tables uploaded once per device) */
static inline int jx_hip_rc(hipError_t e) { return e == hipSuccess ? JPGX_OK : JPGX_EHIP; }
#endif
