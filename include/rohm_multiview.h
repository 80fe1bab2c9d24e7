/*
 * rohm_multiview.h -- C ABI of librohm_hip.so's multi-view triangulation (csrc/multiview.hip): calibrated, synchronised views
 * of 2-D keypoints to a 3-D skeleton.  rohm_amd/multiview.py drives the entry points, tests/multiview_ref.py restates them in
 * numpy.  No counterpart in the reference: its EgoBody loader reads the calibration chain of five Kinects and uses one view.
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
 * Cameras.  cams [V,24] float64, one row per view: R (9 values, row-major, world -> camera: x_cam = R X + t), t (3), fx, fy,
 * cx, cy, k1, k2, p1, p2, k3, three zeros.  2 <= V <= 16 (rohm_mv_limits).  No atomics; every sum is taken in a fixed order:
 * the same input gives the same bits.  All arithmetic is float64 on the float32 keypoints.
 */
#ifndef ROHM_MULTIVIEW_H
#define ROHM_MULTIVIEW_H

#include "rohm_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

/* Host only, nothing on the device is touched: *max_views = 16, *max_pairs = 120 (= 16 * 15 / 2).  Either pointer may be
 * NULL. */
int rohm_mv_limits(int* max_views, int* max_pairs);

/* rohm_mv_triangulate: one robust triangulation per (frame, joint), one launch for the recording.
 * keypoints [V,N,J,3] float32: x, y in pixels as detected (distorted), confidence c.  rigid [12] float64 or NULL: R (9,
 * row-major) then t, world -> output frame; NULL leaves the result in the world.
 * Outputs, all written wholly: joints [N,J,3] float64; conf [N,J] float32; report [N,J,4] float64 = the number of inliers, the
 * inliers' weighted rms reprojection error in px, sigma_m, the number of observed views; inliers [N,J] uint32, bit v set when
 * view v is an inlier; keypoints_und [V,N,J,3] float32 or NULL.
 *
 * The rule per (frame, joint):
 * 1. Observed views S: x, y and c are finite and c > conf_min.  Normalised coordinates: (a, b) starts from (x0, y0) =
 *    ((x - cx) / fx, (y - cy) / fy); five times: r2 = a^2 + b^2, q = 1 / (1 + ((k3 r2 + k2) r2 + k1) r2),
 *    dx = 2 p1 a b + p2 (r2 + 2 a^2), dy = p1 (r2 + 2 b^2) + 2 p2 a b, (a, b) = ((x0 - dx) q, (y0 - dy) q) -- what
 *    cv2.undistortPoints does, and rohm_keypoints_undistort between its two mirrorings; there is NO mirroring here.
 *    keypoints_und = (fx a + cx, fy b + cy, c); an unobserved entry passes through as given.
 *    Ray of view v: origin o = -R^T t, direction d = R^T (a, b, 1) / |R^T (a, b, 1)|.
 * 2. Hypotheses: every pair v1 < v2 of S in lexicographic order (at most 120).  A pair is skipped when |d1 x d2| <
 *    sin(min_angle_rad).  Its point X solves the 3 x 3 system sum (I - d d^T) X = sum (I - d d^T) o over its two rays (the
 *    midpoint of their common perpendicular).  The error of a view v of S at X: with (x_c, y_c, z_c) = R X + t,
 *    e_v = |(fx (x_c / z_c - a), fy (y_c / z_c - b))|, infinite when z_c <= 0.  The pair is a candidate only if both of its own
 *    views have e <= tau_px.  Its inliers are the views of S with e_v <= tau_px, its cost is sum c_v e_v^2 over them (v
 *    ascending).  The winner is the candidate with the most inliers, then the smaller cost, then the lower pair index.
 * 3. No result: |S| < 2, no candidate, or fewer than min_views inliers.  Then joints = NaN, conf = 0, inliers = 0,
 *    report = (0, NaN, NaN, |S|).
 * 4. Refinement: X0 solves sum c_v (I - d d^T) X = sum c_v (I - d d^T) o over the inliers.  `refine` plain Gauss-Newton steps
 *    on E(X) = sum c_v |r_v|^2, r_v = (fx (x_c / z_c - a), fy (y_c / z_c - b)), with the analytic 2 x 3 Jacobian
 *    J_v = diag(fx, fy) [[1 / z_c, 0, -x_c / z_c^2], [0, 1 / z_c, -y_c / z_c^2]] R: X <- X - (sum c J^T J)^-1 sum c J^T r.
 *    There is no per-step accept / reject.  After the last step X0 is kept if E(X) is not finite or exceeds E(X0).
 *    rms = sqrt(E / sum c_v) at the result.  sigma_m = sqrt(trace((sum J_v^T J_v)^-1)) with unit weights at the result: the
 *    standard deviation in metres for one pixel of noise, so a narrow baseline shows up here.
 *    Every 3 x 3 system is symmetric and is solved through its cofactors.
 * 5. conf = the mean c_v of the inliers; joints = rigid applied to the result.
 *
 * Errors before any launch (ROHM_ERR_ARG, the message names the argument): V outside [2, 16], N < 0, J < 1, N * J above
 * 2^29, conf_min or tau_px not finite, tau_px <= 0, min_angle_rad outside [0, pi / 2], min_views outside [2, V], refine
 * outside [0, 64], a null keypoints, cams, joints, conf, report or inliers.  N == 0 returns without a launch.
 * A group of lanes per point -- 16 lanes up to V = 6 (15 pairs), a 64-lane wave above -- in workgroups of 256 threads; both
 * give the same bits; one launch. */
int rohm_mv_triangulate(const float* keypoints, const double* cams, const double* rigid, int V, int N, int J, double conf_min,
                        double tau_px, double min_angle_rad, int min_views, int refine, double* joints, float* conf,
                        double* report, uint32_t* inliers, float* keypoints_und, rohm_stream_t stream);

/* rohm_mv_residuals: the per-view diagnostic.  joints_world [N,J,3] float64 (world frame, not `rigid`'s), keypoints and cams
 * as above.  resid [V,N,J] float64, written wholly: the pixel distance between the detection as given and the point
 * projected with the FORWARD distortion model -- (x, y) = (x_c / z_c, y_c / z_c), r2 = x^2 + y^2,
 * g = 1 + ((k3 r2 + k2) r2 + k1) r2, (fx (x g + 2 p1 x y + p2 (r2 + 2 x^2)) + cx, fy (y g + p1 (r2 + 2 y^2) + 2 p2 x y) + cy)
 * -- and NaN where the view is unobserved (rule 1 with conf_min), the joint is not finite or the point is behind the camera
 * (z_c <= 0).  It does not share the undistortion iterations, so it checks them.  One thread per entry; one launch; the same
 * argument errors as above; N == 0 returns without a launch. */
int rohm_mv_residuals(const double* joints_world, const float* keypoints, const double* cams, int V, int N, int J,
                      double conf_min, double* resid, rohm_stream_t stream);

#ifdef __cplusplus
}
#endif
#endif /* ROHM_MULTIVIEW_H */
