// Multi-view triangulation: calibrated, synchronised views of 2-D keypoints to a 3-D skeleton (rohm_mv_triangulate) and the
// per-view reprojection residuals of a skeleton (rohm_mv_residuals).  rohm_amd/multiview.py drives them; tests/multiview_ref.py
// restates both in numpy; include/rohm_multiview.h states the rule in full.  There is no counterpart in the reference: its
// EgoBody loader reads the calibration of five Kinects and uses one view.
//
// The camera row (observed, undistortion, projection with residual and Jacobian rows, the 3 x 3 cofactor solve) is camera_math.h's,
// shared with fit_views.hip.  All arithmetic is float64 on the float32 keypoints, as in fit.hip and floor.hip.  No atomics, every sum is taken in a fixed
// order or by a fixed butterfly: the same input gives the same bits.
//
// rohm_mv_triangulate: a group of W lanes per (frame, joint) in workgroups of 256 threads.  W = 64, a wave, serves any V; up to
// V = 6 the 15 pairs fit W = 16, four points per wave, which is what a rig of four or five cameras gets.  Lane v < V of the group
// undistorts its view's detection and puts the ray (o, d) and (a, b, c) into LDS: 9 float64 per view.  The lanes then walk the
// pairs v1 < v2 (lane, lane + W: two rounds at V = 16, 120 pairs); each pair's midpoint is scored against every observed ray,
// whose camera row is a wave-uniform load (the view index is the loop counter).  The winner comes from three reductions over
// the group -- integer max of the inlier count, float64 min of the cost among the lanes at that count, integer min of the pair
// index among the lanes at that cost -- so no order of arrival can change a bit.  The refinement stays in the group: lane v
// holds view v's camera and detection in registers, the 3 x 3 normal equations are 16-lane xor-butterflies, the same at either
// W, so both widths give the same bits.  One thread per point with 16 rays in registers spills; a group per point does not.
#include "common.h"
#include "camera_math.h"
#include "reduce.h"
#include "views_args.h"
#include "../../include/rohm_multiview.h"

#include <limits.h>

namespace rohm {

constexpr int kMvMaxPairs = kViewsMax * (kViewsMax - 1) / 2;
constexpr int kMvThreads = 256;
constexpr int kMvSmallViews = 6;                     // up to this many views the pairs (15) fit a group of 16 lanes
constexpr int kMvRay = 9;                            // o (3), d (3), a, b, c
constexpr int kMvMaxRefine = 64;

struct MvArgs {
    const float* kp;
    const double* cams;
    const double* rigid;
    int V, N, J;
    double conf_min, tau, sin_min;
    int min_views, refine;
    double* joints;
    float* conf;
    double* report;
    uint32_t* inliers;
    float* kp_und;
};

// w (I - d d^T) and w (I - d d^T) o of one ray, the terms of the midpoint system
__device__ __forceinline__ void mv_ray_terms(double w, const double* o, const double* d, double* A, double* b) {
    const double od = d[0] * o[0] + d[1] * o[1] + d[2] * o[2];
    A[0] = w * (1.0 - d[0] * d[0]);
    A[1] = w * (-d[0] * d[1]);
    A[2] = w * (-d[0] * d[2]);
    A[3] = w * (1.0 - d[1] * d[1]);
    A[4] = w * (-d[1] * d[2]);
    A[5] = w * (1.0 - d[2] * d[2]);
    b[0] = w * (o[0] - d[0] * od);
    b[1] = w * (o[1] - d[1] * od);
    b[2] = w * (o[2] - d[2] * od);
}

// W lanes per point: 64 (a wave; any V), or 16 when the pairs fit 16 lanes (V <= 6: four points per wave).  Everything a group of W
// lanes decides is uniform in the group, and every shuffle stays inside it, so the groups of a wave never read one another.
template <int W>
__global__ __launch_bounds__(kMvThreads) void mv_triangulate_kernel(const MvArgs g) {
    constexpr int kPoints = kMvThreads / W;          // points per workgroup
    constexpr int kViews = W == 64 ? kViewsMax : kMvSmallViews;
    __shared__ double rays[kPoints][kViews][kMvRay];
    const int lane = threadIdx.x % W, wave = threadIdx.x / W;      // the lane in its group, the group in its workgroup
    const long long P = (long long)g.N * g.J;
    const long long p = (long long)blockIdx.x * kPoints + wave;
    const bool live = p < P;                         // group-uniform
    const int V = g.V;

    // ---- rule 1: lane v < V takes view v
    bool obs = false;
    double cam[14], o[3] = {0.0, 0.0, 0.0}, d[3] = {0.0, 0.0, 0.0}, a = 0.0, b = 0.0, c = 0.0;
#pragma unroll
    for (int k = 0; k < 14; ++k) cam[k] = 0.0;
    if (live && lane < V) {
        const size_t at = ((size_t)lane * (size_t)P + (size_t)p) * 3;
        const float xf = g.kp[at], yf = g.kp[at + 1], cf = g.kp[at + 2];
        const double* row = g.cams + (size_t)lane * kCamRow;
        float ux = xf, uy = yf;
        obs = cam_observed((double)xf, (double)yf, (double)cf, g.conf_min);
        if (obs) {
#pragma unroll
            for (int k = 0; k < 14; ++k) cam[k] = row[k];
            c = (double)cf;
            cam_undistort(row, (double)xf, (double)yf, a, b);
            ux = (float)(row[12] * a + row[14]);
            uy = (float)(row[13] * b + row[15]);
            double n2 = 0.0;
#pragma unroll
            for (int k = 0; k < 3; ++k) {
                o[k] = -(cam[k] * cam[9] + cam[3 + k] * cam[10] + cam[6 + k] * cam[11]);
                d[k] = cam[k] * a + cam[3 + k] * b + cam[6 + k];
                n2 += d[k] * d[k];
            }
            const double n = sqrt(n2);
            double* ray = rays[wave][lane];
#pragma unroll
            for (int k = 0; k < 3; ++k) {
                d[k] /= n;
                ray[k] = o[k];
                ray[3 + k] = d[k];
            }
            ray[6] = a;
            ray[7] = b;
            ray[8] = c;
        }
        if (g.kp_und) {
            g.kp_und[at] = ux;
            g.kp_und[at + 1] = uy;
            g.kp_und[at + 2] = cf;
        }
    }
    __syncthreads();                                 // the only barrier: every group reaches it, a group past the last point leaves after it
    const unsigned S = (unsigned)(__ballot(obs) >> ((threadIdx.x & 63) - lane)) & 0xffffu;
    if (!live) return;
    const int n_obs = __popc(S);

    // ---- rule 2: the lanes walk the pairs
    int best_n = 0, best_q = INT_MAX;
    double best_cost = (double)INFINITY;
    unsigned best_mask = 0u;
    const int n_pairs = V * (V - 1) / 2;
    for (int q = lane; q < n_pairs; q += W) {
        int v1 = 0, rem = q;
        while (rem >= V - 1 - v1) {
            rem -= V - 1 - v1;
            ++v1;
        }
        const int v2 = v1 + 1 + rem;
        if (!((S >> v1) & 1u) || !((S >> v2) & 1u)) continue;
        const double* r1 = rays[wave][v1];
        const double* r2 = rays[wave][v2];
        const double kx = r1[4] * r2[5] - r1[5] * r2[4], ky = r1[5] * r2[3] - r1[3] * r2[5], kz = r1[3] * r2[4] - r1[4] * r2[3];
        if (sqrt(kx * kx + ky * ky + kz * kz) < g.sin_min) continue;
        double A1[6], b1[3], A2[6], b2[3], X[3];
        mv_ray_terms(1.0, r1, r1 + 3, A1, b1);
        mv_ray_terms(1.0, r2, r2 + 3, A2, b2);
#pragma unroll
        for (int k = 0; k < 6; ++k) A1[k] += A2[k];
#pragma unroll
        for (int k = 0; k < 3; ++k) b1[k] += b2[k];
        cam_solve3(A1, b1, X);
        int n = 0;
        double cost = 0.0;
        unsigned mask = 0u;
        for (int v = 0; v < V; ++v) {                // v is wave-uniform: the camera row is a scalar load, whatever S the groups have
            if (!((S >> v) & 1u)) continue;
            const double* ray = rays[wave][v];
            double r[2];
            const double e2 = cam_residual<false>(g.cams + (size_t)v * kCamRow, X, ray[6], ray[7], r, nullptr, nullptr);
            if (sqrt(e2) <= g.tau) {
                ++n;
                cost += ray[8] * e2;
                mask |= 1u << v;
            }
        }
        if (!((mask >> v1) & 1u) || !((mask >> v2) & 1u)) continue;
        if (n > best_n || (n == best_n && cost < best_cost)) {       // q ascends: a tie keeps the lower pair index
            best_n = n;
            best_cost = cost;
            best_q = q;
            best_mask = mask;
        }
    }
    const int n_max = lanes_reduce<W>(best_n, MaxOp());
    const double c_min = lanes_reduce<W>(best_n == n_max ? best_cost : (double)INFINITY, MinOp());
    const int q_min = lanes_reduce<W>((best_n == n_max && best_cost == c_min) ? best_q : INT_MAX, MinOp());

    // ---- rule 3
    if (n_max < 2 || n_max < g.min_views || q_min == INT_MAX) {
        if (lane == 0) {
            const double nan = (double)NAN;
            g.joints[p * 3] = nan;
            g.joints[p * 3 + 1] = nan;
            g.joints[p * 3 + 2] = nan;
            g.conf[p] = 0.0f;
            g.inliers[p] = 0u;
            g.report[p * 4] = 0.0;
            g.report[p * 4 + 1] = nan;
            g.report[p * 4 + 2] = nan;
            g.report[p * 4 + 3] = (double)n_obs;
        }
        return;
    }
    const unsigned mask = __shfl(best_mask, (int)(threadIdx.x & 63) - lane + q_min % W, 64);

    // ---- rule 4: lanes 0..15 hold the views; what a lane that is no inlier adds is exactly zero
    const bool inl = lane < V && ((mask >> lane) & 1u);
    const double w = inl ? c : 0.0;
    double X0[3], X[3], A[6], t3[3];
    {
        double At[6], bt[3];
        mv_ray_terms(w, o, d, At, bt);
#pragma unroll
        for (int k = 0; k < 6; ++k) A[k] = lanes_sum<16>(inl ? At[k] : 0.0);
#pragma unroll
        for (int k = 0; k < 3; ++k) t3[k] = lanes_sum<16>(inl ? bt[k] : 0.0);
        cam_solve3(A, t3, X0);
    }
    const double sum_c = lanes_sum<16>(w);
#pragma unroll
    for (int k = 0; k < 3; ++k) X[k] = X0[k];
    double E0 = 0.0, E = 0.0;
    for (int it = 0; it <= g.refine; ++it) {
        double r[2], j0[3], j1[3];
        const double e2 = cam_residual<true>(cam, X, a, b, r, j0, j1);
        E = lanes_sum<16>(inl ? w * e2 : 0.0);
        if (it == 0) E0 = E;
        if (it == g.refine) break;
        A[0] = lanes_sum<16>(inl ? w * (j0[0] * j0[0] + j1[0] * j1[0]) : 0.0);
        A[1] = lanes_sum<16>(inl ? w * (j0[0] * j0[1] + j1[0] * j1[1]) : 0.0);
        A[2] = lanes_sum<16>(inl ? w * (j0[0] * j0[2] + j1[0] * j1[2]) : 0.0);
        A[3] = lanes_sum<16>(inl ? w * (j0[1] * j0[1] + j1[1] * j1[1]) : 0.0);
        A[4] = lanes_sum<16>(inl ? w * (j0[1] * j0[2] + j1[1] * j1[2]) : 0.0);
        A[5] = lanes_sum<16>(inl ? w * (j0[2] * j0[2] + j1[2] * j1[2]) : 0.0);
#pragma unroll
        for (int k = 0; k < 3; ++k) t3[k] = lanes_sum<16>(inl ? w * (j0[k] * r[0] + j1[k] * r[1]) : 0.0);
        double dX[3];
        cam_solve3(A, t3, dX);
#pragma unroll
        for (int k = 0; k < 3; ++k) X[k] -= dX[k];
    }
    if (!isfinite(E) || E > E0) {
        E = E0;
#pragma unroll
        for (int k = 0; k < 3; ++k) X[k] = X0[k];
    }
    double sigma;
    {
        double r[2], j0[3], j1[3];
        cam_residual<true>(cam, X, a, b, r, j0, j1);
        A[0] = lanes_sum<16>(inl ? j0[0] * j0[0] + j1[0] * j1[0] : 0.0);
        A[1] = lanes_sum<16>(inl ? j0[0] * j0[1] + j1[0] * j1[1] : 0.0);
        A[2] = lanes_sum<16>(inl ? j0[0] * j0[2] + j1[0] * j1[2] : 0.0);
        A[3] = lanes_sum<16>(inl ? j0[1] * j0[1] + j1[1] * j1[1] : 0.0);
        A[4] = lanes_sum<16>(inl ? j0[1] * j0[2] + j1[1] * j1[2] : 0.0);
        A[5] = lanes_sum<16>(inl ? j0[2] * j0[2] + j1[2] * j1[2] : 0.0);
        t3[0] = t3[1] = t3[2] = 0.0;
        double unused[3];
        const CamSolve3 q = cam_solve3(A, t3, unused);
        sigma = sqrt(q.cof_trace / q.det);                 // trace(A^-1)
    }

    // ---- rule 5
    if (lane == 0) {
        double Y[3] = {X[0], X[1], X[2]};
        if (g.rigid) {
#pragma unroll
            for (int k = 0; k < 3; ++k) Y[k] = g.rigid[k * 3] * X[0] + g.rigid[k * 3 + 1] * X[1] + g.rigid[k * 3 + 2] * X[2] + g.rigid[9 + k];
        }
        g.joints[p * 3] = Y[0];
        g.joints[p * 3 + 1] = Y[1];
        g.joints[p * 3 + 2] = Y[2];
        g.conf[p] = (float)(sum_c / (double)n_max);
        g.inliers[p] = mask;
        g.report[p * 4] = (double)n_max;
        g.report[p * 4 + 1] = sqrt(E / sum_c);
        g.report[p * 4 + 2] = sigma;
        g.report[p * 4 + 3] = (double)n_obs;
    }
}

// one thread per (view, frame, joint): the detection as given against the forward distortion model
__global__ __launch_bounds__(256) void mv_residuals_kernel(const double* __restrict__ joints, const float* __restrict__ kp,
                                                           const double* __restrict__ cams, long long P, long long total, double conf_min,
                                                           double* __restrict__ resid) {
    const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= total) return;
    const long long p = i % P;
    const double* cam = cams + (size_t)(i / P) * kCamRow;
    const double x = (double)kp[i * 3], y = (double)kp[i * 3 + 1], c = (double)kp[i * 3 + 2];
    const double X0 = joints[p * 3], X1 = joints[p * 3 + 1], X2 = joints[p * 3 + 2];
    double out = (double)NAN;
    if (cam_observed(x, y, c, conf_min) && isfinite(X0) && isfinite(X1) && isfinite(X2)) {
        const double X[3] = {X0, X1, X2};
        double Xc[3];
        cam_to_view(cam, X, Xc);
        if (Xc[2] > 0.0) {
            const double k1 = cam[16], k2 = cam[17], p1 = cam[18], p2 = cam[19], k3 = cam[20];
            const double u = Xc[0] / Xc[2], v = Xc[1] / Xc[2], r2 = u * u + v * v;
            const double gr = 1.0 + ((k3 * r2 + k2) * r2 + k1) * r2;
            const double ud = u * gr + 2.0 * p1 * u * v + p2 * (r2 + 2.0 * u * u);
            const double vd = v * gr + p1 * (r2 + 2.0 * v * v) + 2.0 * p2 * u * v;
            const double ex = cam[12] * ud + cam[14] - x, ey = cam[13] * vd + cam[15] - y;
            out = sqrt(ex * ex + ey * ey);
        }
    }
    resid[i] = out;
}

static int mv_check(const char* who, int V, int N, int J, double conf_min) {
    if (int rc = views_check_shape(who, V, 2, N, 0, J)) return rc;
    return views_check_conf(who, conf_min);
}

}  // namespace rohm

using namespace rohm;

extern "C" int rohm_mv_limits(int* max_views, int* max_pairs) {
    if (max_views) *max_views = kViewsMax;
    if (max_pairs) *max_pairs = kMvMaxPairs;
    return ROHM_OK;
}

extern "C" int rohm_mv_triangulate(const float* keypoints, const double* cams, const double* rigid, int V, int N, int J, double conf_min,
                                   double tau_px, double min_angle_rad, int min_views, int refine, double* joints, float* conf,
                                   double* report, uint32_t* inliers, float* keypoints_und, rohm_stream_t stream) {
    if (int rc = mv_check("mv_triangulate", V, N, J, conf_min)) return rc;
    ROHM_ARG_CHECK(isfinite(tau_px) && tau_px > 0.0, "mv_triangulate: tau_px must be finite and > 0, got %g", tau_px);
    ROHM_ARG_CHECK(min_angle_rad >= 0.0 && min_angle_rad <= 1.5707963267948966, "mv_triangulate: min_angle_rad must be in [0, pi / 2], got %g",
                   min_angle_rad);
    ROHM_ARG_CHECK(min_views >= 2 && min_views <= V, "mv_triangulate: min_views must be in [2, V = %d], got %d", V, min_views);
    ROHM_ARG_CHECK(refine >= 0 && refine <= kMvMaxRefine, "mv_triangulate: refine must be in [0, %d], got %d", kMvMaxRefine, refine);
    if (N == 0) return ROHM_OK;
    ROHM_ARG_CHECK(keypoints, "mv_triangulate: keypoints is null");
    ROHM_ARG_CHECK(cams, "mv_triangulate: cams is null");
    ROHM_ARG_CHECK(joints, "mv_triangulate: joints is null");
    ROHM_ARG_CHECK(conf, "mv_triangulate: conf is null");
    ROHM_ARG_CHECK(report, "mv_triangulate: report is null");
    ROHM_ARG_CHECK(inliers, "mv_triangulate: inliers is null");
    MvArgs a;
    a.kp = keypoints; a.cams = cams; a.rigid = rigid; a.V = V; a.N = N; a.J = J; a.conf_min = conf_min; a.tau = tau_px;
    a.sin_min = sin(min_angle_rad); a.min_views = min_views; a.refine = refine; a.joints = joints; a.conf = conf; a.report = report;
    a.inliers = inliers; a.kp_und = keypoints_und;
    const long long P = (long long)N * J;
    const double pairs = 0.5 * V * (V - 1);
    prof::Scope ps("mv_triangulate", (double)P * pairs * (60.0 + 30.0 * V), (double)P * (12.0 * V * (keypoints_und ? 2 : 1) + 64.0), (hipStream_t)stream);
    if (V <= kMvSmallViews) {
        constexpr int kPoints = kMvThreads / 16;
        hipLaunchKernelGGL(mv_triangulate_kernel<16>, dim3((unsigned)((P + kPoints - 1) / kPoints)), dim3(kMvThreads), 0, (hipStream_t)stream, a);
    } else {
        constexpr int kPoints = kMvThreads / 64;
        hipLaunchKernelGGL(mv_triangulate_kernel<64>, dim3((unsigned)((P + kPoints - 1) / kPoints)), dim3(kMvThreads), 0, (hipStream_t)stream, a);
    }
    ROHM_LAUNCH_CHECK();
    return ROHM_OK;
}

extern "C" int rohm_mv_residuals(const double* joints_world, const float* keypoints, const double* cams, int V, int N, int J,
                                 double conf_min, double* resid, rohm_stream_t stream) {
    if (int rc = mv_check("mv_residuals", V, N, J, conf_min)) return rc;
    if (N == 0) return ROHM_OK;
    ROHM_ARG_CHECK(joints_world, "mv_residuals: joints_world is null");
    ROHM_ARG_CHECK(keypoints, "mv_residuals: keypoints is null");
    ROHM_ARG_CHECK(cams, "mv_residuals: cams is null");
    ROHM_ARG_CHECK(resid, "mv_residuals: resid is null");
    const long long P = (long long)N * J, total = P * V;
    prof::Scope ps("mv_residuals", 0.0, (double)total * 20.0 + (double)P * 24.0, (hipStream_t)stream);
    hipLaunchKernelGGL(mv_residuals_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, (hipStream_t)stream, joints_world, keypoints,
                       cams, P, total, conf_min, resid);
    ROHM_LAUNCH_CHECK();
    return ROHM_OK;
}
