/*
 * rohm_sync.h -- C ABI of librohm_hip.so's camera synchronisation (csrc/sync.hip): the 2-D keypoints of a person seen by several
 * cameras that were not triggered together to one constant time offset per camera.  rohm_amd/sync.py drives the entry points (the
 * coarse and fine sweeps, the parabola through the best grid point and the weighted least squares of the offsets are host logic
 * there), tests/sync_ref.py restates them in numpy.  No counterpart in the reference: its EgoBody recordings are synchronised by
 * the Kinects' own cable.
 *
 * Where this header stands.  It is PROVISIONAL: it lives in include/provisional/, is not listed in rohm_amd/_lib.py's HEADERS and
 * its rows are _lib.PROVISIONAL_SIGNATURES, which lib() applies under the same strict rule as SIGNATURES.  The reason: every
 * pointer- or stream-taking declaration of HEADERS must have a case in the contract registries (tests/header_cases.py,
 * tests/stale_memory.py and the four families that read them), and the change that added this header was not one that edits
 * them.  Until a later change moves the header up to include/ and adds its header_cases entry, tests/test_sync_ref.py holds the
 * declarations, the table and the library's exports to each other, and tests/test_gpu_sync.py holds the two stream-taking
 * functions to the contracts itself: the same bits over poisoned memory, operands one element past an aligned boundary between
 * intact canaries, and a graph replay on a side stream.
 *
 * The functions declared here obey rohm_hip.h's "Conventions" and "Caller-owned memory" word for word: 0 on success, < 0 on
 * error with a thread-local rohm_last_error(); every tensor argument is a DEVICE pointer to contiguous memory owned by the
 * caller and needs the alignment of its element only; a call reads and writes only the operands it is given; every launch
 * goes on the caller-supplied stream with no synchronisation, no allocation and no read-back, so every stream-taking
 * function here may be recorded into a hipGraph (device operands are read at replay time, the scalars travel in the kernel
 * arguments); outputs may hold anything on entry and are written wholly; a workspace may hold anything on entry and holds
 * nothing a later call needs; an optional output passed as NULL is not computed.
 *
 * The model.  All V views have N frames at one common, uniform rate fps.  Frame n of view v was exposed at times[n] + offset_v,
 * and offset_ref = 0.  For a pair (v1, v2) the shift s = (offset_v1 - offset_v2) fps is in frames: view 1's frame n shows the
 * instant of view 2's frame n + s.  Only constant offsets are covered: drift, different frame rates, rolling shutter, more than
 * one person and a moving rig are outside the model.
 *
 * Interpolation at a real frame index f (all of it in float64): i0 = floor(f), alpha = f - i0.  alpha == 0 uses frame i0 alone,
 * bit for bit -- frame i0 + 1 need not exist or be usable.  Otherwise both brackets i0 and i0 + 1 must lie in [0, N) and be
 * usable, and the value is (1 - alpha) x(i0) + alpha x(i0 + 1).  f = n + s is one float64 addition.
 *
 * Cameras and keypoints are rohm_rig.h's: cams [V,24] float64 (the pair sweep reads only the intrinsics, values 12..20),
 * keypoints [V,N,J,3] float32 (x, y in pixels as detected, confidence c), P = N J points, P <= 2^29.  No atomics; every float64
 * sum is taken in a fixed order that depends on the sizes only: the same input gives the same bits.  All arithmetic is float64 on
 * the float32 keypoints.
 */
#ifndef ROHM_SYNC_H
#define ROHM_SYNC_H

#include "../rohm_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

/* Host only: the bytes of the workspace `ws` of rohm_sync_pair_sweep (the undistorted coordinates, V * P * 16, as
 * rohm_rig_pair_ws_bytes).  < 0 (ROHM_ERR_ARG) when V is outside [2, 16] or P outside [1, 2^29]. */
long long rohm_sync_ws_bytes(int V, long long P);

/* rohm_sync_pair_sweep: the epipolar cost of Q pairs of views at S time shifts each.  pairs [Q,2] int32 (v1, v2); E [Q,9] float64,
 * one matrix per pair (row-major 3 x 3, x2^T E x1 = 0); shifts [Q,S] float64 in frames.  out [Q,S,4] float64, written wholly.
 *
 * The rule per (pair, shift s):
 * 1. Every view is undistorted once into ws by rule 1 of rohm_multiview.h, as rohm_rig_pair_hypotheses does it (the same device
 *    code): (a, b) per detection, not finite where the detection is unobserved.
 * 2. A point (n, j) is common when view 1's detection (n, j) is observed and view 2's normalised coordinates of joint j can be
 *    interpolated at f = n + s by the rule above (a bracket is usable when it is observed).  x1 = (a1, b1, 1) is view 1's point,
 *    x2 = (a2, b2, 1) view 2's, interpolated in normalised coordinates.
 * 3. d is the Sampson distance in pixels of rule 4 of rohm_rig.h with that rule's scale, d^2 = (x2^T E x1 * scale)^2 / (l0^2 +
 *    l1^2 + m0^2 + m1^2); the point is an inlier when d <= tau_px, decided without the root as there.
 * 4. out[q, s] = (the number of common points; the number of inliers; sum d^2 / (d^2 + sigma_px^2) over the common points -- sum
 *    d^2 at sigma_px = 0; sum d^2 over the inliers).  A common point whose d^2 is not finite or whose gradient norm is not
 *    positive (an E that is not finite) is no inlier and adds the supremum of its term to the third sum: 1, or +inf at
 *    sigma_px = 0.
 * 5. A row of NaN for a pair outside [0, V) or with v1 = v2, and for a shift that is not finite.  Zeros where nothing is common
 *    (a shift beyond +-N among them).  An E that is not finite has no inliers.
 * 6. The order of the sums is that of rohm_rig_pair_moments: one workgroup of 256 threads per (pair, shift); thread t takes the
 *    points p = n J + j = t, t + 256, ...; a xor-butterfly per wave (offsets 32, 16, ..., 1); the four wave partials in wave order.
 *
 * Errors before any launch (ROHM_ERR_ARG, the message names the argument): V outside [2, 16], N < 1, J < 1, N * J above 2^29,
 * Q < 0, S < 1, Q * S above 2^20, conf_min or tau_px or sigma_px not finite, tau_px <= 0, sigma_px < 0, a null keypoints, cams,
 * pairs, E, shifts, ws or out.  Q == 0 returns without a launch.  Two launches. */
int rohm_sync_pair_sweep(const float* keypoints, const double* cams, const int* pairs, const double* E, const double* shifts, int V,
                         int N, int J, int Q, int S, double conf_min, double tau_px, double sigma_px, void* ws, double* out,
                         rohm_stream_t stream);

/* rohm_sync_resample: every view on another clock.  shifts [V] float64 in frames; out [V,N,J,3] float32, written wholly, must not
 * overlap keypoints.  out[v, n] is view v at the frame index f = n + shifts[v], in pixels as detected:
 * - alpha == 0: the three values of frame i0, bit for bit (shifts[v] == 0 copies the view's bits; an integer shift is a slice);
 * - otherwise a bracket has a position when x, y and c are finite and c > 0 (the track resampler's rule).  Both have one: x and
 *   y are (1 - alpha) x(i0) + alpha x(i0 + 1) in float64, rounded once to float32, and the confidence is min(c0, c1).  One has
 *   none: (x, y) of the other bracket and confidence 0.  Neither has: (0, 0, 0);
 * - a frame index whose bracket lies outside [0, N) gives (0, 0, 0); a shift that is not finite gives zeros for that view.
 * Errors before the launch: V outside [1, 16], N < 1, J < 1, N * J above 2^29, a null keypoints, shifts or out.  One launch, one
 * thread per (v, n, j). */
int rohm_sync_resample(const float* keypoints, const double* shifts, int V, int N, int J, float* out, rohm_stream_t stream);

#ifdef __cplusplus
}
#endif
#endif /* ROHM_SYNC_H */
