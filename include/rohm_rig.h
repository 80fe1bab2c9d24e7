/*
 * rohm_rig.h -- C ABI of librohm_hip.so's rig calibration (csrc/rig.hip): the 2-D keypoints of a person seen by several
 * synchronised cameras with known intrinsics to the cameras' extrinsics.  rohm_amd/rig.py drives the entry points (the RANSAC
 * loop, the spanning tree, the Levenberg-Marquardt loop and its Cholesky solve are host logic there), tests/rig_ref.py restates
 * them in numpy.  No counterpart in the reference: its EgoBody loader reads the calibration chain of five Kinects.
 *
 * The functions declared here obey rohm_hip.h's "Conventions" and "Caller-owned memory" word for word: 0 on success, < 0 on
 * error with a thread-local rohm_last_error(); every tensor argument is a DEVICE pointer to contiguous memory owned by the
 * caller and needs the alignment of its element only; a call reads and writes only the operands it is given; every launch
 * goes on the caller-supplied stream with no synchronisation, no allocation and no read-back, so every stream-taking
 * function here may be recorded into a hipGraph (device operands are read at replay time, the scalars travel in the kernel
 * arguments); outputs may hold anything on entry and are written wholly; a workspace may hold anything on entry and holds
 * nothing a later call needs; an optional output passed as NULL is not computed.
 * tests/test_gpu_stale_memory.py, test_gpu_bounds.py, test_gpu_stream_order.py and test_gpu_graph_replay.py hold the functions
 * of this header to those contracts, with the cases of tests/header_cases.py.
 *
 * Cameras.  cams [V,24] float64 are the rows of rohm_multiview.h: R (9, row-major, world -> camera), t (3), fx, fy, cx, cy, k1,
 * k2, p1, p2, k3, three zeros; 2 <= V <= 16.  The pair functions read only the intrinsics (values 12..20).  keypoints [V,N,J,3]
 * float32: x, y in pixels as detected (distorted), confidence c; P = N J points, P <= 2^29.  A detection is observed, and
 * undistorted to normalised coordinates (a, b), by rule 1 of rohm_multiview.h; a detection whose (a, b) is not finite counts as
 * unobserved.  No atomics; every float64 sum is taken in a fixed order that depends on the sizes only: the same input gives the
 * same bits.  All arithmetic is float64 on the float32 keypoints.
 */
#ifndef ROHM_RIG_H
#define ROHM_RIG_H

#include "rohm_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

/* Host only: the bytes of the workspace `ws` of the two pair functions (the undistorted coordinates, V * P * 16) and of
 * rohm_rig_ba_moments (the workgroups' partial sums).  < 0 (ROHM_ERR_ARG) when V is outside [2, 16] or P outside [1, 2^29]. */
long long rohm_rig_pair_ws_bytes(int V, long long P);
long long rohm_rig_ba_ws_bytes(int V, long long P);

/* rohm_rig_pair_hypotheses: epipolar RANSAC for Q pairs of views in one call: K eight-point hypotheses per pair, solved and scored.
 * pairs [Q,2] int32 (v1, v2); samples [Q,K,8] int32, indices into the P points, drawn by the caller and in DEVICE memory --
 * nothing is checked on the host, so the call does not wait (this differs from rohm_floor_hypotheses).
 * Outputs, all written wholly: E [Q,K,9] float64 (row-major 3 x 3); counts [Q,K,2] int64 = (inliers, common points); best [Q]
 * int32.
 *
 * The rule per (pair, hypothesis):
 * 1. A point is common when it is observed in both views; x1 = (a1, b1, 1), x2 = (a2, b2, 1) are its undistorted normalised
 *    coordinates in v1 and v2.  Its row is x2 (x) x1 = (a2 a1, a2 b1, a2, b2 a1, b2 b1, b2, a1, b1, 1), so that x2^T E x1 = row . E.
 * 2. M = sum row^T row (9 x 9) over the eight sampled points, in sample order.  E is the unit eigenvector of M's smallest
 *    eigenvalue (the lowest index among equal ones), signed so that its largest-magnitude entry is positive (the lowest index on
 *    ties).  The eigenvectors come from 10 sweeps of cyclic Jacobi rotations (p, q) in row order, each the textbook rotation
 *    t = sign(theta) / (|theta| + sqrt(theta^2 + 1)), theta = (a_qq - a_pp) / (2 a_pq), skipped when a_pq = 0.
 * 3. The hypothesis is degenerate -- E = NaN, counts = (-1, -1) -- when a pair entry is outside [0, V) or v1 = v2; a sample index
 *    is outside [0, P); a sample index is repeated; a sampled point is not common; or the second-smallest eigenvalue is below
 *    1e-12 of the largest (or M is not finite).
 * 4. The Sampson distance of a common point in pixels: with l = E x1 and m = E^T x2,
 *    d = |x2^T E x1| / sqrt(l0^2 + l1^2 + m0^2 + m1^2) * (fx1 + fy1 + fx2 + fy2) / 4.
 *    The point is an inlier when d <= tau_px, decided without the root as (x2^T E x1 * scale)^2 <= tau_px^2 (l0^2 + l1^2 + m0^2 +
 *    m1^2) with a positive right-hand factor.  counts = (the number of inliers, the number of common points).
 * 5. best = the hypothesis with the most inliers, the lowest index on ties, -1 when every hypothesis is degenerate.  Counts are
 *    integers: no order of a reduction can change a bit.
 *
 * Errors before any launch (ROHM_ERR_ARG, the message names the argument): V outside [2, 16], N < 1, J < 1, N * J above 2^29,
 * Q < 0, K < 1, Q * K above 2^27, conf_min or tau_px not finite, tau_px <= 0, a null keypoints, cams, pairs, samples, ws, E,
 * counts or best.  Q == 0 returns without a launch.
 * Three launches: the undistortion of every view's points into ws, once, not once per pair; 32 hypotheses per workgroup of 256
 * threads -- 16 lanes solve one eigenproblem in LDS, then the pair's points pass through LDS in tiles of 512 and every lane scores
 * its two hypotheses against them; one workgroup per pair for `best`. */
int rohm_rig_pair_hypotheses(const float* keypoints, const double* cams, const int* pairs, const int* samples, int V, int N, int J,
                             int Q, int K, double conf_min, double tau_px, void* ws, double* E, long long* counts, int* best,
                             rohm_stream_t stream);

/* rohm_rig_pair_moments: the sums of the inlier refit.  E [Q,9] float64, one matrix per pair.  moments [Q,47] float64, written
 * wholly: over the pair's common points with d <= tau_px (rule 4 above) the count, sum d^2 (d^2 = (x2^T E x1 * scale)^2 / (l0^2 +
 * l1^2 + m0^2 + m1^2)), and the 45 sums row_i row_j for i <= j in row-major order of the upper triangle.  The caller takes the
 * smallest eigenvector of the 9 x 9 matrix they fill and calls again.  A pair outside [0, V) or with v1 = v2 gives a row of NaN;
 * an E that is not finite has no inliers (zeros).
 * The order of the sums: one workgroup of 256 threads per pair; thread t takes the points t, t + 256, ...; a xor-butterfly per
 * wave (offsets 32, 16, ..., 1); the four wave partials in wave order.
 * Errors as above (without samples, K, counts and best; `moments` for the output).  Two launches. */
int rohm_rig_pair_moments(const float* keypoints, const double* cams, const int* pairs, const double* E, int V, int N, int J, int Q,
                          double conf_min, double tau_px, void* ws, double* moments, rohm_stream_t stream);

/* rohm_rig_ba_moments: the camera system of one Levenberg-Marquardt try of bundle adjustment, the points eliminated.
 * cams [V,24]: the current rig.  points [P,3] float64: the current points; a point is inside the problem when its three
 * coordinates are finite and at least two views observe it.
 * Unknowns: per camera (d omega, d t) with R' = exp([d omega]x) R and t' = t + d t; per point X.
 * Energy: E = sum_v sum_p c_vp rho(|r_vp|^2) over the observed (v, p) of the points inside, r the pixel residual of
 * rohm_multiview.h's rule 4 against the once-undistorted detection, rho of rohm_fit_views.h (Geman-McClure with sigma_px, plain at
 * 0), weights w = c rho'.  An observed (v, p) with z_c <= 0 adds +inf to E, counts as an observation and adds nothing else.
 * Jacobians: J_X = A R and J_c = [-A [R X]x, A] with A the 2 x 3 matrix of rohm_fit_views.h.  With H_pp = sum_v w J_X^T J_X,
 * g_p = sum_v w J_X^T r, H_cp = w J_c^T J_X (6 x 3 per observed (v, p)), U_v = sum_p w J_c^T J_c, g_c = sum_p w J_c^T r and
 * H_pp,d = H_pp + lambda diag(diag H_pp + 1e-9), whose inverse goes through the cofactors:
 *   S [6V,6V] = U + lambda diag(diag U + 1e-9) - sum_p H_cp H_pp,d^-1 H_pc      (symmetric: the lower triangle mirrors the upper)
 *   r [6V]    = g_c - sum_p H_cp H_pp,d^-1 g_p
 *   stats [2] = (E, the number of observations).
 * The caller deletes the rows and columns of the camera it holds fixed, solves S dc = -r and calls rohm_rig_ba_update.
 * The order of the sums: the points go in tiles of 16 to G = ceil(T / ceil(T / 256)) workgroups, T = ceil(P / 16), consecutive
 * tiles to one workgroup; 16 lanes take a point, lane v view v, and sum over the views by a xor-butterfly (offsets 8, 4, 2, 1);
 * every entry of a workgroup's partial of S and r has one thread that adds the workgroup's points in ascending order, skipping a
 * point that one of the entry's two cameras does not see; U, g_c, E and the count are summed per lane over the tiles, then over
 * the 16 lanes of a view in ascending order; a closing launch adds the workgroups' partials in workgroup order.
 * Errors before any launch: V, N, J as above, conf_min not finite, sigma_px or lambda not finite or negative, a null keypoints,
 * cams, points, ws, S, r or stats.  Two launches. */
int rohm_rig_ba_moments(const float* keypoints, const double* cams, const double* points, int V, int N, int J, double conf_min,
                        double sigma_px, double lambda, void* ws, double* S, double* r, double* stats, rohm_stream_t stream);

/* rohm_rig_ba_update: the points of the try.  The operands of rohm_rig_ba_moments and dc [V,6] float64 (d omega, d t per camera;
 * zeros for the fixed one).  points_new [P,3] = X - H_pp,d^-1 (g_p + sum_v H_pc dc_v) for a point inside the problem, the sum over
 * the views by the same butterfly; any other point passes through as given.  cams_new [V,24] or NULL: R' = rodrigues(d omega) R
 * (fit_math.h's: angle = |d omega + 1e-8|), t' = t + d t, the other 12 values copied.
 * Errors as above (`dc`, `points_new`).  One launch. */
int rohm_rig_ba_update(const float* keypoints, const double* cams, const double* points, const double* dc, int V, int N, int J,
                       double conf_min, double sigma_px, double lambda, double* points_new, double* cams_new, rohm_stream_t stream);

#ifdef __cplusplus
}
#endif
#endif /* ROHM_RIG_H */
