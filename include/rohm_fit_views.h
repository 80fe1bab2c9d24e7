/*
 * rohm_fit_views.h -- C ABI of librohm_hip.so's fit of SMPL-X to 2-D keypoints by reprojection (csrc/fit_views.hip): one
 * calibrated camera or several, straight from the pixels of every view to per-frame pose parameters.  rohm_amd/fit_views.py
 * drives the entry point, tests/fit_views_ref.py restates it in numpy.  No counterpart in the reference: its recordings come
 * with fitted parameters.
 *
 * The functions declared here obey rohm_hip.h's "Conventions" and "Caller-owned memory" word for word: 0 on success, < 0 on
 * error with a thread-local rohm_last_error(); every tensor argument is a DEVICE pointer to contiguous memory owned by the
 * caller and needs the alignment of its element only; a call reads and writes only the operands it is given; every launch
 * goes on the caller-supplied stream with no synchronisation, no allocation and no read-back, so every stream-taking
 * function here may be recorded into a hipGraph (device operands are read at replay time, the scalars travel in the kernel
 * arguments); outputs may hold anything on entry and are written wholly; an optional output passed as NULL is not computed.
 * tests/test_gpu_stale_memory.py, test_gpu_bounds.py, test_gpu_stream_order.py and test_gpu_graph_replay.py hold the functions
 * of this header to those contracts, with the cases of tests/header_cases.py.
 *
 * Cameras.  cams [V,24] float64, the rows of rohm_multiview.h: R (9 values, row-major, world -> camera: x_cam = R X + t), t (3),
 * fx, fy, cx, cy, k1, k2, p1, p2, k3, three zeros.  1 <= V <= 16.  No atomics; every sum is taken in a fixed order: the same
 * input gives the same bits.  All arithmetic is float64 on the float32 keypoints and betas.
 */
#ifndef ROHM_FIT_VIEWS_H
#define ROHM_FIT_VIEWS_H

#include "rohm_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

/* rohm_fit_views_pose: one Levenberg-Marquardt problem per frame, one launch for the recording.  It is rohm_fit_pose with the
 * reprojection error of every view in place of the distance to 3-D joints.
 * h: the body model (rohm_smplx_create; at least 22 joints).  keypoints [V,N,22,3] float32: x, y in pixels as detected
 * (distorted) and a confidence c, SMPL joint order.  betas [N,10] float32.  init [N,69] float64, required: the start, the
 * axis-angles of joints 0..21 then the translation.  prev [N,69] float64 or NULL.  w_prior [22] float64.
 * Outputs, all written wholly: params [N,69] float64; report [N,8] float64; resid [V,N,22] float64 or NULL; normal [N,69,70]
 * float64 or NULL.
 *
 * Observations.  (v, j) is observed when x, y and c are finite and c > conf_min; it is undistorted to normalised (a, b) by
 * rule 1 of rohm_multiview.h (five iterations, no mirroring), once.  n_obs is their number in the frame.
 *
 * Energy.  x = (theta, t).  With X_j = p_j(theta, beta) + t, p_j the joints of rohm_fit_pose, and (x_c, y_c, z_c) = R_v X_j + t_v:
 *     r_vj = (fx (x_c / z_c - a), fy (y_c / z_c - b)),   e2 = |r_vj|^2
 *     E(x) = sum_v sum_j c_vj rho(e2) + sum_k w_prior[k] |theta_k|^2
 *          + w_smooth sum_{k=1..21} |theta_k - m_k|^2 + w_smooth_t |t - m_t|^2
 * over the observed (v, j).  rho(e2) = e2 when sigma_px == 0, else sigma^2 e2 / (sigma^2 + e2) (Geman-McClure: the mis-detection
 * of one view saturates at sigma^2).  m_k is rohm_fit_pose's: the mean of prev's rows f - 1 and f + 1 over those that exist and
 * are wholly finite; m_t is the same mean of their translations; without such a neighbour (or with prev NULL) both smoothing
 * terms are absent.  An observed joint with z_c <= 0 makes E = +inf.
 *
 * Normal equations.  A_vj = diag(fx, fy) [[1 / z_c, 0, -x_c / z_c^2], [0, 1 / z_c, -y_c / z_c^2]] R_v;  w_vj = c_vj rho'(e2),
 * which is c_vj when sigma_px == 0 and c_vj sigma^4 / (sigma^2 + e2)^2 otherwise;  W_j = sum_v w_vj A^T A,
 * b_j = sum_v w_vj A^T r_vj, v ascending.  H = sum_j Jp_j^T W_j Jp_j + diag(w_prior + smoothing weights),
 * g = sum_j Jp_j^T b_j + w_prior theta + w_smooth (theta - m) + w_smooth_t (t - m_t): the gradient of E / 2.  Jp_j is the
 * 3 x 69 block of rohm_fit_pose's joint Jacobian.
 *
 * Iteration.  rohm_fit_pose's, unchanged: lambda starts at 1e-3; up to eight tries per iteration of
 * (H + lambda diag(diag(H) + 1e-9)) d = -g by Cholesky, a pivot that is not positive rejects the try; x + d is accepted when
 * E(x + d) < E(x), so an infinite E is a rejected try; lambda / 10 (at least 1e-9) after an accepted try, lambda * 10 (at most
 * 1e8) after a rejected one.
 *
 * Start and status (report[.,0]), decided in this order:
 *   0  n_obs < min_obs.
 *   2  a rotation entry of the init row is not finite, or its translation is neither three NaN nor three finite values.
 *   3  no usable start, see below.
 *   1  fitted.
 * Where the init row's three translation entries are all NaN the translation is solved in closed form at the row's rotations:
 * every observation gives (R_v[0] - a R_v[2]) . (p_j + t) + (t_v[0] - a t_v[2]) = 0 and the same with b and row 1, linear in t;
 * the 3 x 3 normal equations with weights c_vj are solved through their cofactors.  Status 3 when that system is singular
 * (det <= 1e-12 trace^3) or when, at the start, E is not finite (an observed joint at z_c <= 0).
 *
 * report [N,8]: status; E at the start; E at the end; accepted iterations; final lambda; sqrt(sum c e2 / sum c) in px at the end;
 * n_obs; the smallest z_c over the observations at the end.  resid: sqrt(e2) at the end, NaN where unobserved.  normal: H | g at
 * the start.  Statuses 0, 2 and 3 give a zero params row, a zero normal block, NaN resid and
 * report = (status, NaN, NaN, 0, NaN, NaN, n_obs, NaN).
 *
 * Errors before any launch (ROHM_ERR_ARG, the message names the argument): V outside [1, 16], N < 0, iters < 0, sigma_px,
 * conf_min, w_smooth or w_smooth_t negative or not finite, min_obs < 1, a null h, keypoints, cams, betas, init, w_prior, params
 * or report.  N == 0 returns without a launch.
 * One workgroup of 256 threads per frame, 76 KiB of LDS whatever V is; one launch. */
int rohm_fit_views_pose(const rohm_smplx_t* h, const float* keypoints, const double* cams, const float* betas, const double* init,
                        const double* prev, const double* w_prior, double w_smooth, double w_smooth_t, double sigma_px,
                        double conf_min, int iters, int min_obs, int V, int N, double* params, double* report, double* resid,
                        double* normal, rohm_stream_t stream);

#ifdef __cplusplus
}
#endif
#endif /* ROHM_FIT_VIEWS_H */
