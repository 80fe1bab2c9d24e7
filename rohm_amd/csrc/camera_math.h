// The camera row of rohm_multiview.h and rohm_fit_views.h and what multiview.hip and fit_views.hip do with it, in float64: what counts
// as observed, the undistortion, the projection with its residual and Jacobian rows, and the symmetric 3 x 3 solve.  Private to csrc.
//
// A row of `cams` has 24 values: R (9, row-major), t (3), fx, fy, cx, cy, k1, k2, p1, p2, k3, three zeros.  The first 14 are all
// the projection needs, so a caller may keep just those.  keypoints_undistort_kernel (clips.hip) keeps its own copy of the iteration:
// it is pinned to cv2's bits, and compiled through cam_undistort its multiply-adds contract in another order.
#pragma once
#include <hip/hip_runtime.h>
#include <math.h>

namespace rohm {

constexpr int kCamRow = 24;
constexpr int kCamPinhole = 14;                      // R, t, fx, fy

// rule 1 of rohm_multiview.h: a detection is observed when it is finite and its confidence is above conf_min
__device__ __forceinline__ bool cam_observed(double x, double y, double c, double conf_min) {
    return isfinite(x) && isfinite(y) && isfinite(c) && c > conf_min;
}

// the pixel (px, py) of a full camera row to undistorted normalised coordinates (a, b): the five fixed-point iterations of
// cv2.undistortPoints, no mirroring
__device__ __forceinline__ void cam_undistort(const double* cam, double px, double py, double& a, double& b) {
    const double k1 = cam[16], k2 = cam[17], p1 = cam[18], p2 = cam[19], k3 = cam[20];
    const double x0 = (px - cam[14]) / cam[12], y0 = (py - cam[15]) / cam[13];
    double x = x0, y = y0;
#pragma unroll 1
    for (int it = 0; it < 5; ++it) {
        const double r2 = x * x + y * y;
        const double icd = 1.0 / (1.0 + ((k3 * r2 + k2) * r2 + k1) * r2);
        const double dx = 2.0 * p1 * x * y + p2 * (r2 + 2.0 * x * x);
        const double dy = p1 * (r2 + 2.0 * y * y) + 2.0 * p2 * x * y;
        x = (x0 - dx) * icd;
        y = (y0 - dy) * icd;
    }
    a = x;
    b = y;
}

// Xc = R X + t
__device__ __forceinline__ void cam_to_view(const double* cam, const double* X, double* Xc) {
    Xc[0] = cam[0] * X[0] + cam[1] * X[1] + cam[2] * X[2] + cam[9];
    Xc[1] = cam[3] * X[0] + cam[4] * X[1] + cam[5] * X[2] + cam[10];
    Xc[2] = cam[6] * X[0] + cam[7] * X[1] + cam[8] * X[2] + cam[11];
}

// the residual r (pixels) of a view at X against the undistorted detection (a, b) and, on request, the rows of its 2 x 3 Jacobian;
// returns |r|^2, infinite when z_c <= 0
template <bool WITH_J>
__device__ __forceinline__ double cam_residual(const double* cam, const double* X, double a, double b, double* r, double* j0, double* j1) {
    double Xc[3];
    cam_to_view(cam, X, Xc);
    const double zc = Xc[2];
    const double u = Xc[0] / zc, v = Xc[1] / zc;
    r[0] = cam[12] * (u - a);
    r[1] = cam[13] * (v - b);
    if (WITH_J) {
#pragma unroll
        for (int k = 0; k < 3; ++k) {
            j0[k] = cam[12] * (cam[k] - u * cam[6 + k]) / zc;
            j1[k] = cam[13] * (cam[3 + k] - v * cam[6 + k]) / zc;
        }
    }
    return zc > 0.0 ? r[0] * r[0] + r[1] * r[1] : (double)INFINITY;
}

// x = A^-1 b through the cofactors of the symmetric A = (a00, a01, a02, a11, a12, a22).  The caller judges singularity: det, and
// the trace of the cofactor matrix (trace(A^-1) = cof_trace / det).
struct CamSolve3 { double det, cof_trace; };
__device__ __forceinline__ CamSolve3 cam_solve3(const double* A, const double* b, double* x) {
    const double c00 = A[3] * A[5] - A[4] * A[4];
    const double c01 = A[2] * A[4] - A[1] * A[5];
    const double c02 = A[1] * A[4] - A[2] * A[3];
    const double c11 = A[0] * A[5] - A[2] * A[2];
    const double c12 = A[1] * A[2] - A[0] * A[4];
    const double c22 = A[0] * A[3] - A[1] * A[1];
    const double det = A[0] * c00 + A[1] * c01 + A[2] * c02;
    x[0] = (c00 * b[0] + c01 * b[1] + c02 * b[2]) / det;
    x[1] = (c01 * b[0] + c11 * b[1] + c12 * b[2]) / det;
    x[2] = (c02 * b[0] + c12 * b[1] + c22 * b[2]) / det;
    return {det, c00 + c11 + c22};
}

}  // namespace rohm
