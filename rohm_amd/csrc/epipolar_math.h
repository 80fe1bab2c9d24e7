// What rig.hip and sync.hip share of the epipolar geometry of a pair of views: the limits (views_args.h's), the once-per-call undistortion of every
// view's points into the workspace (rule 1 of rohm_multiview.h; the kernel lives in rig.hip, one copy in the library), the pair
// test and the Sampson terms of rule 4 of rohm_rig.h.
#pragma once
#include "common.h"
#include "camera_math.h"
#include "views_args.h"

namespace rohm {

// und [V,P,2] float64 into ws: (a, b) of every detection, NaN where it is unobserved or its undistortion is not finite.  One launch.
int rig_undistort(const float* keypoints, const double* cams, int V, long long P, double conf_min, void* ws, hipStream_t stream);

__device__ __forceinline__ bool rig_pair_ok(int v1, int v2, int V) { return v1 >= 0 && v1 < V && v2 >= 0 && v2 < V && v1 != v2; }

// x2^T E x1 times the pixel scale and the squared gradient norm of rule 4
__device__ __forceinline__ void rig_sampson(const double* E, double a1, double b1, double a2, double b2, double scale, double& ns, double& den) {
    const double l0 = E[0] * a1 + E[1] * b1 + E[2], l1 = E[3] * a1 + E[4] * b1 + E[5], l2 = E[6] * a1 + E[7] * b1 + E[8];
    const double m0 = E[0] * a2 + E[3] * b2 + E[6], m1 = E[1] * a2 + E[4] * b2 + E[7];
    ns = (a2 * l0 + b2 * l1 + l2) * scale;
    den = l0 * l0 + l1 * l1 + m0 * m0 + m1 * m1;
}

}  // namespace rohm
