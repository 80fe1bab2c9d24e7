// Synchronising a rig's cameras from the person: the epipolar cost of a pair of views over a list of time shifts
// (rohm_sync_pair_sweep) and the resampling of every view onto the reference view's clock (rohm_sync_resample).  rohm_amd/sync.py
// drives them (the coarse and fine sweeps, the parabola, the weighted least squares of the per-view offsets are host logic);
// tests/sync_ref.py restates them in numpy; include/provisional/rohm_sync.h states the rule in full.  There is no counterpart in the
// reference.
//
// The undistortion of every view's points (once per call, into the workspace), the pair test and the Sampson terms are rig.hip's,
// through epipolar_math.h.  All arithmetic is float64 on the float32 keypoints.  No atomics: thread t takes the points t, t + 256,
// ... in ascending order, and the threads' sums meet in reduce.h's block_reduce, which fixes the rest of the order.
//
// rohm_sync_pair_sweep is the plain form: one workgroup of 256 threads per (pair, shift).  A ten-minute recording of four views swept
// over +-30 frames is 366 workgroups of 4e5 points each; view 1's point and view 2's two brackets are 48 bytes per point out of L2.
#include "common.h"
#include "camera_math.h"
#include "epipolar_math.h"
#include "reduce.h"
#include "../../include/provisional/rohm_sync.h"

namespace rohm {

constexpr int kSyncThreads = 256;
constexpr long long kSyncMaxCells = 1ll << 20;       // Q * S
constexpr int kSyncOut = 4;                          // common, inliers, the robust sum, sum d^2 over the inliers

struct SyncSweepArgs {
    const double* und;            // [V,P,2]
    const double* cams;
    const int* pairs;             // [Q,2]
    const double* E;              // [Q,9]
    const double* shifts;         // [Q,S]
    int V, N, J, S;
    double tau2, sigma2;
    double* out;                  // [Q,S,4]
};

__global__ __launch_bounds__(kSyncThreads) void sync_sweep_kernel(const SyncSweepArgs g) {
    __shared__ double shm[kSyncThreads / 64][kSyncOut];
    const int tid = threadIdx.x;
    const int cell = blockIdx.x;                     // q * S + s
    const int q = cell / g.S;
    const int v1 = g.pairs[q * 2], v2 = g.pairs[q * 2 + 1];
    const double shift = g.shifts[cell];
    double* out = g.out + (size_t)cell * kSyncOut;
    if (!rig_pair_ok(v1, v2, g.V) || !isfinite(shift)) {       // uniform in the workgroup
        if (tid < kSyncOut) out[tid] = (double)NAN;
        return;
    }
    double E[9];
#pragma unroll
    for (int i = 0; i < 9; ++i) E[i] = g.E[(size_t)q * 9 + i];
    const double* c1 = g.cams + (size_t)v1 * kCamRow;
    const double* c2 = g.cams + (size_t)v2 * kCamRow;
    const double scale = (c1[12] + c1[13] + c2[12] + c2[13]) / 4.0;
    const int N = g.N, J = g.J, P = N * J;
    const double* u1 = g.und + (size_t)v1 * (size_t)P * 2;
    const double* u2 = g.und + (size_t)v2 * (size_t)P * 2;
    double m[kSyncOut] = {0.0, 0.0, 0.0, 0.0};
    for (int p = tid; p < P; p += kSyncThreads) {
        const int n = p / J, j = p - n * J;
        const double a1 = u1[(size_t)p * 2], b1 = u1[(size_t)p * 2 + 1];
        const double f = (double)n + shift;
        const double fl = floor(f);
        const double alpha = f - fl;
        if (!(isfinite(a1) && isfinite(b1)) || !(fl >= 0.0 && fl < (double)N)) continue;
        const int i0 = (int)fl;
        const size_t at = ((size_t)i0 * J + j) * 2;
        double a2 = u2[at], b2 = u2[at + 1];
        if (alpha != 0.0) {                          // both brackets must exist and be observed
            if (i0 + 1 >= N) continue;
            const double a3 = u2[at + (size_t)J * 2], b3 = u2[at + (size_t)J * 2 + 1];
            a2 = (1.0 - alpha) * a2 + alpha * a3;    // NaN when either bracket is unobserved
            b2 = (1.0 - alpha) * b2 + alpha * b3;
        }
        if (!(isfinite(a2) && isfinite(b2))) continue;
        double ns, den;
        rig_sampson(E, a1, b1, a2, b2, scale, ns, den);
        const double d2 = ns * ns / den;
        m[0] += 1.0;
        if (den > 0.0 && isfinite(d2)) {
            m[2] += g.sigma2 > 0.0 ? d2 / (d2 + g.sigma2) : d2;
            if (ns * ns <= g.tau2 * den) {
                m[1] += 1.0;
                m[3] += d2;
            }
        } else {                                     // no distance: the robust function's supremum
            m[2] += g.sigma2 > 0.0 ? 1.0 : (double)INFINITY;
        }
    }
    block_reduce<kSyncThreads, kSyncOut>(m, shm, out, SumOfK());
}

// a bracket that carries a position: finite, with a positive confidence (the track resampler's rule)
__device__ __forceinline__ bool sync_has_position(float x, float y, float c) { return isfinite(x) && isfinite(y) && isfinite(c) && c > 0.0f; }

__global__ __launch_bounds__(256) void sync_resample_kernel(const float* __restrict__ kp, const double* __restrict__ shifts, int N, int J,
                                                            long long total, float* __restrict__ out) {
    const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;       // (v, n, j)
    if (i >= total) return;
    const long long per_view = (long long)N * J;
    const int v = (int)(i / per_view);
    const long long r = i - (long long)v * per_view;
    const int n = (int)(r / J), j = (int)(r - (long long)n * J);
    const double shift = shifts[v];
    const double f = (double)n + shift;
    const double fl = floor(f);
    const double alpha = f - fl;
    float x = 0.0f, y = 0.0f, c = 0.0f;
    if (isfinite(shift) && fl >= 0.0 && fl < (double)N) {
        const int i0 = (int)fl;
        const float* s0 = kp + (((size_t)v * N + i0) * J + j) * 3;
        if (alpha == 0.0) {                          // the frame itself, bit for bit
            const unsigned* b0 = reinterpret_cast<const unsigned*>(s0);
            unsigned* o = reinterpret_cast<unsigned*>(out + (size_t)i * 3);
            o[0] = b0[0]; o[1] = b0[1]; o[2] = b0[2];
            return;
        }
        if (i0 + 1 < N) {
            const float* s1 = s0 + (size_t)J * 3;
            const float x0 = s0[0], y0 = s0[1], c0 = s0[2], x1 = s1[0], y1 = s1[1], c1 = s1[2];
            const bool h0 = sync_has_position(x0, y0, c0), h1 = sync_has_position(x1, y1, c1);
            if (h0 && h1) {
                // two products and one sum, each rounded: no contraction, so that the float32 result is the restatement's bit
                x = (float)__dadd_rn(__dmul_rn(1.0 - alpha, (double)x0), __dmul_rn(alpha, (double)x1));
                y = (float)__dadd_rn(__dmul_rn(1.0 - alpha, (double)y0), __dmul_rn(alpha, (double)y1));
                c = fminf(c0, c1);
            } else if (h0) {
                x = x0; y = y0;
            } else if (h1) {
                x = x1; y = y1;
            }
        }
    }
    out[(size_t)i * 3] = x;
    out[(size_t)i * 3 + 1] = y;
    out[(size_t)i * 3 + 2] = c;
}

}  // namespace rohm

using namespace rohm;

extern "C" long long rohm_sync_ws_bytes(int V, long long P) {
    if (int rc = views_check_ws("sync_ws_bytes", V, P)) return rc;
    return (long long)V * P * 16;
}

extern "C" int rohm_sync_pair_sweep(const float* keypoints, const double* cams, const int* pairs, const double* E, const double* shifts, int V,
                                    int N, int J, int Q, int S, double conf_min, double tau_px, double sigma_px, void* ws, double* out,
                                    rohm_stream_t stream) {
    if (int rc = views_check_shape("sync_pair_sweep", V, 2, N, 1, J)) return rc;
    ROHM_ARG_CHECK(Q >= 0, "sync_pair_sweep: Q must be >= 0, got %d", Q);
    ROHM_ARG_CHECK(S >= 1, "sync_pair_sweep: S must be >= 1, got %d", S);
    ROHM_ARG_CHECK((long long)Q * S <= kSyncMaxCells, "sync_pair_sweep: Q * S must not exceed %lld, got %lld", kSyncMaxCells, (long long)Q * S);
    if (int rc = views_check_conf("sync_pair_sweep", conf_min)) return rc;
    ROHM_ARG_CHECK(isfinite(tau_px) && tau_px > 0.0, "sync_pair_sweep: tau_px must be finite and > 0, got %g", tau_px);
    ROHM_ARG_CHECK(isfinite(sigma_px) && sigma_px >= 0.0, "sync_pair_sweep: sigma_px must be finite and >= 0, got %g", sigma_px);
    if (Q == 0) return ROHM_OK;
    ROHM_ARG_CHECK(keypoints, "sync_pair_sweep: keypoints is null");
    ROHM_ARG_CHECK(cams, "sync_pair_sweep: cams is null");
    ROHM_ARG_CHECK(pairs, "sync_pair_sweep: pairs is null");
    ROHM_ARG_CHECK(E, "sync_pair_sweep: E is null");
    ROHM_ARG_CHECK(shifts, "sync_pair_sweep: shifts is null");
    ROHM_ARG_CHECK(ws, "sync_pair_sweep: ws is null");
    ROHM_ARG_CHECK(out, "sync_pair_sweep: out is null");
    const long long P = (long long)N * J;
    prof::Scope ps("sync_pair_sweep", 45.0 * (double)Q * S * (double)P, 48.0 * (double)Q * S * (double)P, (hipStream_t)stream);
    if (int rc = rig_undistort(keypoints, cams, V, P, conf_min, ws, (hipStream_t)stream)) return rc;
    SyncSweepArgs a;
    a.und = (const double*)ws; a.cams = cams; a.pairs = pairs; a.E = E; a.shifts = shifts; a.V = V; a.N = N; a.J = J; a.S = S;
    a.tau2 = tau_px * tau_px; a.sigma2 = sigma_px * sigma_px; a.out = out;
    hipLaunchKernelGGL(sync_sweep_kernel, dim3((unsigned)(Q * S)), dim3(kSyncThreads), 0, (hipStream_t)stream, a);
    ROHM_LAUNCH_CHECK();
    return ROHM_OK;
}

extern "C" int rohm_sync_resample(const float* keypoints, const double* shifts, int V, int N, int J, float* out, rohm_stream_t stream) {
    if (int rc = views_check_shape("sync_resample", V, 1, N, 1, J)) return rc;
    ROHM_ARG_CHECK(keypoints, "sync_resample: keypoints is null");
    ROHM_ARG_CHECK(shifts, "sync_resample: shifts is null");
    ROHM_ARG_CHECK(out, "sync_resample: out is null");
    const long long total = (long long)V * N * J;
    prof::Scope ps("sync_resample", 6.0 * (double)total, 36.0 * (double)total, (hipStream_t)stream);
    hipLaunchKernelGGL(sync_resample_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, (hipStream_t)stream, keypoints, shifts, N, J, total,
                       out);
    ROHM_LAUNCH_CHECK();
    return ROHM_OK;
}
