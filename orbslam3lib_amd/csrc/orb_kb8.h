// orb_kb8.h -- the KannalaBrandt8 projection, shared by the fisheye stereo kernel (orb_fisheye.hip)
// and the two-camera motion-model search (orb_track.hip): one definition, so both stay pinned to
// the same libm restatements (orb_math.h; tests/test_host_harness.py).
#pragma once
#include <hip/hip_runtime.h>

#include "orb_math.h"

namespace orbgpu {

// KannalaBrandt8::project(const Eigen::Vector3f&) (KannalaBrandt8.cpp:61-78)
__device__ inline void kb8_project(const float* P, const float x[3], float uv[2]) {
    const float x2_plus_y2 = x[0] * x[0] + x[1] * x[1];
    const float theta = libm_atan2f(sqrtf(x2_plus_y2), x[2]);
    const float psi = libm_atan2f(x[1], x[0]);
    const float theta2 = theta * theta;
    const float theta3 = theta * theta2;
    const float theta5 = theta3 * theta2;
    const float theta7 = theta5 * theta2;
    const float theta9 = theta7 * theta2;
    const float r = theta + P[4] * theta3 + P[5] * theta5 + P[6] * theta7 + P[7] * theta9;
    float sn, cs;
    libm_sincosf(psi, &sn, &cs);
    uv[0] = P[0] * r * cs + P[2];
    uv[1] = P[1] * r * sn + P[3];
}

}  // namespace orbgpu
