// SMPL-X from 2-D keypoints by reprojection, one camera or several: per-frame pose by Levenberg-Marquardt (rohm_fit_views_pose).
// rohm_amd/fit_views.py drives it; tests/fit_views_ref.py restates it in numpy; include/rohm_fit_views.h states the rule in full.
// There is no counterpart in the reference: its recordings come with fitted parameters.
//
// This is rohm_fit_pose (fit.hip) with a symmetric 3 x 3 weight per joint where that kernel has a scalar: the data term's normal
// equations are H = sum_j Jp_j^T W_j Jp_j, g = sum_j Jp_j^T b_j, with W_j = sum_v w_vj A_vj^T A_vj and b_j = sum_v w_vj A_vj^T r_vj
// taken over the views in ascending order by the joint's own lane.  The quadratic forms are formed on the fly from the 66 x 66
// joint Jacobian, so there is no second 66 x 66 array.  Only that data term (FitViewsProblem), the start translation and the report
// are here: the solver (its LDS, the prologue pieces, the prior and smoothing, the walk over H, the Cholesky solve, the
// iteration, the unfitted exit) is fit_math.h's; the camera row (observed, undistortion, projection with
// residual and Jacobian rows, the 3 x 3 solve) is camera_math.h's, shared with multiview.hip.  All arithmetic is float64 on the
// float32 inputs.  No atomics, every sum is taken by one thread in a fixed order: the same input gives the same bits.
//
// One workgroup of 256 threads per frame.  LDS, as float64: fit.hip's 64.9 KiB (H packed, the Jacobian / Cholesky factor, the
// per-joint state) plus the undistorted observations (a, b, c) of every (view, joint), 8.3 KiB at the limit of 16 views, 14 values
// per camera row (1.8 KiB) and the per-joint W_j, b_j and partial sums (2.3 KiB): 76.0 KiB whatever V is, so two workgroups share a
// CU's 160 KiB as in fit.hip.  The undistortion runs once, in the prologue, (view, joint) entries across the threads.
#include "camera_math.h"
#include "fit_math.h"
#include "views_args.h"
#include "../../include/rohm_fit_views.h"

namespace rohm {

constexpr int kFvMaxViews = kViewsMax;               // (of a camera row's 24 values the iteration keeps kCamPinhole = 14: R, t, fx, fy)
constexpr int kFvReport = 8;
constexpr double kFvSingular = 1e-12;                // the start translation's system is singular when det <= this * trace^3

struct FitViewsArgs {
    const float* Jt;              // [J,3]
    const float* Js;              // [J,3,10]
    const int* parents;           // [J]
    const float* kp;              // [V,N,22,3]
    const double* cams;           // [V,24]
    const float* betas;           // [N,10]
    const double* init;           // [N,69]
    const double* prev;           // [N,69] or null
    const double* w_prior;        // [22]
    double w_smooth, w_smooth_t, sigma2, conf_min;
    int iters, min_obs, V, N;
    double* params;               // [N,69]
    double* report;               // [N,8]
    double* resid;                // [V,N,22] or null
    double* normal;               // [N,69,70] or null
};

struct FitViewsShared : FitCore {
    double Wj[NJ * 6], bj[NJ * 3];                   // per joint: W_j as (00, 01, 02, 11, 12, 22) and b_j
    double ej[NJ], ce2[NJ], sc[NJ], zmin[NJ];        // per joint: sum_v c rho(e2) (infinite behind a camera), sum_v c e2, sum_v c, min z_c
    double obs[kFvMaxViews * NJ * 3];                // (a, b, c) per (view, joint); c = 0 where unobserved
    double cam[kFvMaxViews * kCamPinhole];
    int n_obs, solve_t;
#ifdef ROHM_FIT_VIEWS_ONE_WORKGROUP                  // the A/B build of scripts/bench_fit_views.py: past 80 KiB a workgroup has its CU to itself
    double one_workgroup_pad[1024];
#endif
};

__device__ __forceinline__ double fv_sym(const double* Wq, int a, int b) {        // entry (a, b) of (00, 01, 02, 11, 12, 22)
    const int lo = a < b ? a : b, hi = a < b ? b : a;
    return Wq[lo == 0 ? hi : (lo == 1 ? 2 + hi : 5)];
}

// The data term sum_v sum_j c_vj rho(|r_vj|^2) for fit_lm.
struct FitViewsProblem {
    FitViewsShared& s;
    int tid, V;
    double sigma2;

    // R, J_r on 22 lanes, the chain on lane 0.  Ends with a barrier.
    template <bool kJac>
    __device__ __forceinline__ void kinematics(const double* x) const {
        fit_rotations<kJac>(s, x, tid);
        if (tid == 0) chain64(s.R, s.rest, s.parents, s.G, s.P);
        __syncthreads();
    }

    // Joint j against its observations at X = P_j + t, the views in ascending order: e_j, sum c e2, sum c, min z_c and, with kJac, W_j
    // and b_j.  `resid` (this frame's [V][.][22] rows, stride `vstride` between views) receives sqrt(e2), NaN where unobserved.
    template <bool kJac>
    __device__ __forceinline__ void joint(const double* x, int j, double* resid, size_t vstride) const {
        const double X[3] = {s.P[j * 3] + x[kFitRot], s.P[j * 3 + 1] + x[kFitRot + 1], s.P[j * 3 + 2] + x[kFitRot + 2]};
        double e = 0.0, ce2 = 0.0, sc = 0.0, zmin = (double)INFINITY;
        double Wq[6] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0}, bq[3] = {0.0, 0.0, 0.0};
        bool behind = false;
        for (int v = 0; v < V; ++v) {
            const double* o = s.obs + (v * NJ + j) * 3;
            const double c = o[2];
            double out = __longlong_as_double(0x7ff8000000000000ll);
            if (c > 0.0) {
                const double* cam = s.cam + v * kCamPinhole;
                double Xc[3];
                cam_to_view(cam, X, Xc);
                zmin = fmin(zmin, Xc[2]);
                if (Xc[2] > 0.0) {
                    double r[2], j0[3], j1[3];
                    const double e2 = cam_residual<kJac>(cam, X, o[0], o[1], r, j0, j1);
                    double rho = e2, drho = 1.0;
                    if (sigma2 > 0.0) {
                        const double q = sigma2 / (sigma2 + e2);
                        rho = q * e2;
                        drho = q * q;
                    }
                    e += c * rho;
                    ce2 += c * e2;
                    sc += c;
                    out = sqrt(e2);
                    if (kJac) {
                        const double wv = c * drho;
                        Wq[0] += wv * (j0[0] * j0[0] + j1[0] * j1[0]);
                        Wq[1] += wv * (j0[0] * j0[1] + j1[0] * j1[1]);
                        Wq[2] += wv * (j0[0] * j0[2] + j1[0] * j1[2]);
                        Wq[3] += wv * (j0[1] * j0[1] + j1[1] * j1[1]);
                        Wq[4] += wv * (j0[1] * j0[2] + j1[1] * j1[2]);
                        Wq[5] += wv * (j0[2] * j0[2] + j1[2] * j1[2]);
#pragma unroll
                        for (int k = 0; k < 3; ++k) bq[k] += wv * (j0[k] * r[0] + j1[k] * r[1]);
                    }
                } else {
                    behind = true;
                }
            }
            if (resid) resid[(size_t)v * vstride + j] = out;
        }
        s.ej[j] = behind ? (double)INFINITY : e;
        s.ce2[j] = ce2;
        s.sc[j] = sc;
        s.zmin[j] = zmin;
        if (kJac) {
#pragma unroll
            for (int k = 0; k < 6; ++k) s.Wj[j * 6 + k] = Wq[k];
#pragma unroll
            for (int k = 0; k < 3; ++k) s.bj[j * 3 + k] = bq[k];
        }
    }

    // E at x; every thread returns it.  kJac also leaves J_r in M, W_j and b_j for hessian() and gradient().
    template <bool kJac>
    __device__ __forceinline__ double evaluate(const double* x, double* resid = nullptr, size_t vstride = 0) const {
        kinematics<kJac>(x);
        if (tid < NJ) joint<kJac>(x, tid, resid, vstride);
        __syncthreads();
        if (tid == 0) {
            double e = 0.0;
            for (int j = 0; j < NJ; ++j) e += s.ej[j];
            s.E = fit_prior_energy(s, x, e);
        }
        __syncthreads();
        return s.E;
    }

    // the data term's share of H_ij (i >= j) and of g_i: sum_q Jp_q^T W_q Jp_q and sum_q Jp_q^T b_q, the translation's columns of Jp
    // being the identity
    __device__ __forceinline__ double hessian(int i, int j) const {
        double v = 0.0;
        if (i < kFitRot) {
            for (int q = 0; q < NJ; ++q) {
                const double* Wq = s.Wj + q * 6;
                const double* row = s.W + (q * 3) * kFitRot;
                const double a0 = row[i], a1 = row[kFitRot + i], a2 = row[2 * kFitRot + i];
                const double b0 = row[j], b1 = row[kFitRot + j], b2 = row[2 * kFitRot + j];
                v += a0 * (Wq[0] * b0 + Wq[1] * b1 + Wq[2] * b2) + a1 * (Wq[1] * b0 + Wq[3] * b1 + Wq[4] * b2) +
                     a2 * (Wq[2] * b0 + Wq[4] * b1 + Wq[5] * b2);
            }
        } else if (j < kFitRot) {
            const int a = i - kFitRot;
            for (int q = 0; q < NJ; ++q) {
                const double* Wq = s.Wj + q * 6;
                const double* row = s.W + (q * 3) * kFitRot;
                v += fv_sym(Wq, a, 0) * row[j] + fv_sym(Wq, a, 1) * row[kFitRot + j] + fv_sym(Wq, a, 2) * row[2 * kFitRot + j];
            }
        } else {
            for (int q = 0; q < NJ; ++q) v += fv_sym(s.Wj + q * 6, i - kFitRot, j - kFitRot);
        }
        return v;
    }
    __device__ __forceinline__ double gradient(int i) const {
        double v = 0.0;
        if (i < kFitRot) {
            for (int q = 0; q < NJ; ++q) {
                const double* row = s.W + (q * 3) * kFitRot;
                v += row[i] * s.bj[q * 3] + row[kFitRot + i] * s.bj[q * 3 + 1] + row[2 * kFitRot + i] * s.bj[q * 3 + 2];
            }
        } else {
            for (int q = 0; q < NJ; ++q) v += s.bj[q * 3 + i - kFitRot];
        }
        return v;
    }
};

// Two waves per SIMD, as fit_pose_kernel: 76 KiB of LDS lets two workgroups share a CU only if the kernel stays within 256 registers.
// Measured for 3 000 frames of 20 iterations at V = 1 / 4 / 16: 41 / 58 / 60 ms, against 71 / 104 / 107 ms with
// one workgroup per CU (profiles/fit_views_bench.json, profiles/fit_views_bench_one_workgroup_per_cu.json).
__global__ __launch_bounds__(kFitThreads) __attribute__((amdgpu_waves_per_eu(2))) void fit_views_pose_kernel(const FitViewsArgs a) {
    __shared__ FitViewsShared s;
    const int tid = threadIdx.x;
    const size_t f = blockIdx.x;
    const int V = a.V;
    double* params = a.params + f * kFitX;
    double* report = a.report + f * kFvReport;
    double* normal = a.normal ? a.normal + f * kFitX * (kFitX + 1) : nullptr;
    double* resid = a.resid ? a.resid + f * NJ : nullptr;            // view v's row of this frame is at resid + v * N * 22
    const size_t vstride = (size_t)a.N * NJ;
    const double* init = a.init + f * kFitX;
    const FitViewsProblem prob = {s, tid, V, a.sigma2};

    // ---- prologue: observations (undistorted once), camera rows, the body
    for (int e = tid; e < V * NJ; e += kFitThreads) {
        const int v = e / NJ, j = e % NJ;
        const float* k = a.kp + (((size_t)v * a.N + f) * NJ + j) * 3;
        const double px = (double)k[0], py = (double)k[1], c = (double)k[2];
        const bool ok = cam_observed(px, py, c, a.conf_min);
        double ua = 0.0, ub = 0.0;
        if (ok) cam_undistort(a.cams + (size_t)v * kCamRow, px, py, ua, ub);
        s.obs[e * 3] = ua;
        s.obs[e * 3 + 1] = ub;
        s.obs[e * 3 + 2] = ok ? c : 0.0;
    }
    for (int e = tid; e < V * kCamPinhole; e += kFitThreads) s.cam[e] = a.cams[(size_t)(e / kCamPinhole) * kCamRow + e % kCamPinhole];
    fit_load_body(s, a.Jt, a.Js, a.parents, a.betas + f * NBETA, a.w_prior, tid);
    __syncthreads();
    if (tid == 0) {
        int seen = 0;
        for (int e = 0; e < V * NJ; ++e) seen += s.obs[e * 3 + 2] > 0.0 ? 1 : 0;
        s.n_obs = seen;
        bool rot_ok = true;
        for (int i = 0; i < kFitRot; ++i) rot_ok = rot_ok && isfinite(init[i]);
        const double t0 = init[kFitRot], t1 = init[kFitRot + 1], t2 = init[kFitRot + 2];
        const bool t_nan = isnan(t0) && isnan(t1) && isnan(t2);
        const bool t_ok = isfinite(t0) && isfinite(t1) && isfinite(t2);
        int status = 1;
        if (seen < a.min_obs) status = 0;
        else if (!rot_ok || !(t_nan || t_ok)) status = 2;
        s.status = status;
        s.solve_t = t_nan ? 1 : 0;
        for (int i = 0; i < kFitX; ++i) s.x[i] = (status == 1 && !(t_nan && i >= kFitRot)) ? init[i] : 0.0;
        fit_lane0_setup(s, a.prev, f, a.N, a.w_smooth, a.w_smooth_t);        // smoothing: body pose and translation, not the root
    }
    __syncthreads();

    // ---- the start: the translation in closed form where the row asks for it, and every observed joint in front of its camera
    double E = 0.0;
    if (s.status == 1) {                             // (uniform: read after the barrier, written again only behind the next one)
        if (s.solve_t) {
            prob.kinematics<false>(s.x);
            if (tid < NJ) {                          // joint j's share of sum c (n1 n1^T + n2 n2^T) t = -sum c (n1 (n1 . p + d1) + n2 (n2 . p + d2))
                double A[6] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0}, r[3] = {0.0, 0.0, 0.0};
                const double* p = s.P + tid * 3;
                for (int v = 0; v < V; ++v) {
                    const double* o = s.obs + (v * NJ + tid) * 3;
                    const double c = o[2];
                    if (!(c > 0.0)) continue;
                    const double* cam = s.cam + v * kCamPinhole;
#pragma unroll
                    for (int h = 0; h < 2; ++h) {
                        const double n0 = cam[h * 3] - o[h] * cam[6], n1 = cam[h * 3 + 1] - o[h] * cam[7], n2 = cam[h * 3 + 2] - o[h] * cam[8];
                        const double d = (n0 * p[0] + n1 * p[1] + n2 * p[2]) + (cam[9 + h] - o[h] * cam[11]);
                        A[0] += c * (n0 * n0); A[1] += c * (n0 * n1); A[2] += c * (n0 * n2);
                        A[3] += c * (n1 * n1); A[4] += c * (n1 * n2); A[5] += c * (n2 * n2);
                        r[0] -= c * (n0 * d); r[1] -= c * (n1 * d); r[2] -= c * (n2 * d);
                    }
                }
                for (int k = 0; k < 6; ++k) s.Wj[tid * 6 + k] = A[k];
                for (int k = 0; k < 3; ++k) s.bj[tid * 3 + k] = r[k];
            }
            __syncthreads();
            if (tid == 0) {
                double A[6] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0}, b[3] = {0.0, 0.0, 0.0}, t[3];
                for (int j = 0; j < NJ; ++j) {
                    for (int k = 0; k < 6; ++k) A[k] += s.Wj[j * 6 + k];
                    for (int k = 0; k < 3; ++k) b[k] += s.bj[j * 3 + k];
                }
                const double det = cam_solve3(A, b, t).det, tr = A[0] + A[3] + A[5];
                if (det > kFvSingular * (tr * tr * tr)) {
                    for (int k = 0; k < 3; ++k) s.x[kFitRot + k] = t[k];
                } else {
                    s.status = 3;
                }
            }
            __syncthreads();
        }
        if (s.status == 1) {
            E = prob.evaluate<true>(s.x);
            if (!(E < (double)INFINITY)) {           // an observed joint at z_c <= 0 (or a start that is not a number)
                if (tid == 0) s.status = 3;
            }
            __syncthreads();
        }
    }
    const int status = s.status;
    if (status != 1) {
        fit_unfitted(status, params, report, normal, tid);
        const double nan = __longlong_as_double(0x7ff8000000000000ll);
        if (resid)
            for (int e = tid; e < V * NJ; e += kFitThreads) resid[(size_t)(e / NJ) * vstride + e % NJ] = nan;
        if (tid == 0) {
            report[6] = (double)s.n_obs; report[7] = nan;
        }
        return;
    }

    const FitLm lm = fit_lm(s, prob, E, a.iters, normal, tid);
    prob.evaluate<false>(s.x, resid, vstride);       // the residuals at the answer
    if (tid < kFitX) params[tid] = s.x[tid];
    if (tid == 0) {
        double sc = 0.0, sr = 0.0, zmin = (double)INFINITY;
        for (int j = 0; j < NJ; ++j) {
            sc += s.sc[j];
            sr += s.ce2[j];
            zmin = fmin(zmin, s.zmin[j]);
        }
        report[0] = 1.0; report[1] = lm.E0; report[2] = lm.E; report[3] = (double)lm.accepted; report[4] = lm.lambda; report[5] = sqrt(sr / sc);
        report[6] = (double)s.n_obs; report[7] = zmin;
    }
}

}  // namespace rohm

using namespace rohm;

extern "C" int rohm_fit_views_pose(const rohm_smplx_t* h, const float* keypoints, const double* cams, const float* betas, const double* init,
                                   const double* prev, const double* w_prior, double w_smooth, double w_smooth_t, double sigma_px,
                                   double conf_min, int iters, int min_obs, int V, int N, double* params, double* report, double* resid,
                                   double* normal, rohm_stream_t stream) {
    ROHM_ARG_CHECK(V >= 1 && V <= kFvMaxViews, "fit_views_pose: V must be in [1, %d], got %d", kFvMaxViews, V);
    ROHM_ARG_CHECK(N >= 0, "fit_views_pose: N must be >= 0, got %d", N);
    ROHM_ARG_CHECK(iters >= 0, "fit_views_pose: iters must be >= 0, got %d", iters);
    ROHM_ARG_CHECK(isfinite(sigma_px) && sigma_px >= 0.0, "fit_views_pose: sigma_px must be finite and >= 0, got %g", sigma_px);
    ROHM_ARG_CHECK(isfinite(conf_min) && conf_min >= 0.0, "fit_views_pose: conf_min must be finite and >= 0, got %g", conf_min);
    ROHM_ARG_CHECK(isfinite(w_smooth) && w_smooth >= 0.0, "fit_views_pose: w_smooth must be finite and >= 0, got %g", w_smooth);
    ROHM_ARG_CHECK(isfinite(w_smooth_t) && w_smooth_t >= 0.0, "fit_views_pose: w_smooth_t must be finite and >= 0, got %g", w_smooth_t);
    ROHM_ARG_CHECK(min_obs >= 1, "fit_views_pose: min_obs must be >= 1, got %d", min_obs);
    if (N == 0) return ROHM_OK;
    ROHM_ARG_CHECK(h, "fit_views_pose: the body model handle is null");
    ROHM_ARG_CHECK(keypoints, "fit_views_pose: keypoints is null");
    ROHM_ARG_CHECK(cams, "fit_views_pose: cams is null");
    ROHM_ARG_CHECK(betas, "fit_views_pose: betas is null");
    ROHM_ARG_CHECK(init, "fit_views_pose: init is null");
    ROHM_ARG_CHECK(w_prior, "fit_views_pose: w_prior is null");
    ROHM_ARG_CHECK(params, "fit_views_pose: params is null");
    ROHM_ARG_CHECK(report, "fit_views_pose: report is null");
    ROHM_ARG_CHECK(h->J >= NJ, "fit_views_pose: the body model has %d joints, fewer than %d", h->J, NJ);
    FitViewsArgs a;
    a.Jt = h->d_Jt; a.Js = h->d_Js; a.parents = h->d_parents; a.kp = keypoints; a.cams = cams; a.betas = betas; a.init = init; a.prev = prev;
    a.w_prior = w_prior; a.w_smooth = w_smooth; a.w_smooth_t = w_smooth_t; a.sigma2 = sigma_px * sigma_px; a.conf_min = conf_min;
    a.iters = iters; a.min_obs = min_obs; a.V = V; a.N = N; a.params = params; a.report = report; a.resid = resid; a.normal = normal;
    prof::Scope ps("fit_views_pose", (double)N * (iters + 1) * (30.0 * kFitTri * NJ + 80.0 * V * NJ),
                   (double)N * (12.0 * V * NJ + 40.0 + 8.0 * (kFitX * 3 + kFvReport + (resid ? V * NJ : 0))), (hipStream_t)stream);
    hipLaunchKernelGGL(fit_views_pose_kernel, dim3((unsigned)N), dim3(kFitThreads), 0, (hipStream_t)stream, a);
    ROHM_LAUNCH_CHECK();
    return ROHM_OK;
}
