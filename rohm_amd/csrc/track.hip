// A generic track (per-frame SMPL-X estimates of one person at any frame rate, with frames the detector missed) put on
// the 30 fps grid the networks were trained on -- or a reconstruction put back onto the source's time stamps.
//
// There is no counterpart in the reference: its loaders assume one fit per frame at exactly 30 fps.  The rule for one
// output time t (tests/track_ref.py restates it in numpy):
//   brackets   i0 = last valid source frame with times_src <= t, i1 = first valid one with times_src >= t; where one side
//              does not exist both are the nearest valid frame (a hold) and gap = 1.  alpha = (t - t0) / (t1 - t0) in
//              float64, 0 when i0 == i1.  gap = 1 also when t1 - t0 > max_gap.
//   alpha == 0 every parameter is the bit pattern of source row i0 (no conversion, no renormalisation) and so are, outside
//              a gap, the keypoints and the mask: a 30 fps track passes through unchanged.
//   parameters are interpolated even inside a gap (the networks need an input; the masks say it is no evidence): the 22
//              rotations by a float64 quaternion slerp (q1 negated when dot < 0, omega = atan2(sqrt(max(1 - d d, 0)), d),
//              lerp weights when sin(omega) < 1e-8, normalised, back through 2 atan2(|v|, w) with w >= 0); transl and
//              betas as a + alpha (b - a).
//   keypoints  outside a gap: confidence min(c0, c1); x, y interpolated in float64 and rounded to float32; a bracket with
//              confidence 0 has no position, x, y then come from the other one.  Inside a gap (holds included): (0, 0, 0).
//   mask       min(m0, m1) outside a gap, 0 inside.
// One thread per (output frame, slot); slots = 22 rotations, 1 for transl + betas, J keypoints, M mask columns.  Every
// thread finds its brackets by a binary search over valid_idx (17 steps for a ten-minute recording).  No atomics, nothing
// written twice: the same input gives the same bits.
#include <vector>
#include "common.h"
#include "rot_priv.h"

namespace rohm {

constexpr int kTrackCols = 79;                 // global_orient 3, transl 3, betas 10, body_pose 63
constexpr int kTrackRot = 22;                  // root + 21 body joints
constexpr int kTrackFixedSlots = kTrackRot + 1;

// (rotvec_to_quat_f64, quat_to_rotvec_f64 and slerp_rotvec_f64 live in rot_priv.h: export.hip blends with them too)
struct TrackArgs {
    const double* times_src;   // [N]
    const int* valid_idx;      // [Nv] ascending, inside [0, N)
    const double* params;      // [N,79]
    const float* keypoints;    // [N,J,3] or null
    const float* mask;         // [N,M] or null
    const double* times_dst;   // [n_out]
    double max_gap;
    int N, Nv, J, M, n_out;
    double* params_out;        // [n_out,79]
    float* keypoints_out;      // [n_out,J,3]
    float* mask_out;           // [n_out,M]
    int* src_index;            // [n_out]
    unsigned char* gap;        // [n_out]
};

__global__ __launch_bounds__(256) void track_resample_kernel(const TrackArgs a) {
    const int slots = kTrackFixedSlots + a.J + a.M;
    const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= (long long)a.n_out * slots) return;
    const int n = (int)(i / slots), slot = (int)(i - (long long)n * slots);
    const double t = a.times_dst[n];
    // a source index outside [0, N) (the host checks them) is clamped: never a read outside the arrays
    auto src = [&](int k) { return min(max(a.valid_idx[k], 0), a.N - 1); };
    int lo = 0, hi = a.Nv;                                   // number of valid frames with times_src <= t
    while (lo < hi) {
        const int mid = (lo + hi) >> 1;
        if (a.times_src[src(mid)] <= t) lo = mid + 1; else hi = mid;
    }
    int k0 = lo - 1, k1 = lo;
    bool gap = false;
    if (k0 < 0) { k0 = k1 = 0; gap = true; }
    else if (a.times_src[src(k0)] == t) k1 = k0;
    else if (k1 >= a.Nv) { k1 = k0; gap = true; }
    const int i0 = src(k0), i1 = src(k1);
    double alpha = 0.0;
    if (i0 != i1) {
        const double t0 = a.times_src[i0], t1 = a.times_src[i1];
        alpha = (t - t0) / (t1 - t0);
        gap = (t1 - t0) > a.max_gap;
    }
    const bool copy = alpha == 0.0;
    const double* p0 = a.params + (size_t)i0 * kTrackCols;
    const double* p1 = a.params + (size_t)i1 * kTrackCols;
    double* po = a.params_out + (size_t)n * kTrackCols;
    if (slot < kTrackRot) {
        const int col = slot == 0 ? 0 : 16 + (slot - 1) * 3;
        if (copy) {
            po[col] = p0[col]; po[col + 1] = p0[col + 1]; po[col + 2] = p0[col + 2];
        } else {
            double rv[3];
            slerp_rotvec_f64(p0 + col, p1 + col, alpha, rv);
            po[col] = rv[0]; po[col + 1] = rv[1]; po[col + 2] = rv[2];
        }
    } else if (slot == kTrackRot) {
#pragma unroll
        for (int c = 3; c < 16; ++c) po[c] = copy ? p0[c] : p0[c] + alpha * (p1[c] - p0[c]);
        a.src_index[n] = i0;
        a.gap[n] = gap ? 1 : 0;
    } else if (slot < kTrackFixedSlots + a.J) {
        const int j = slot - kTrackFixedSlots;
        const float* k0p = a.keypoints + ((size_t)i0 * a.J + j) * 3;
        const float* k1p = a.keypoints + ((size_t)i1 * a.J + j) * 3;
        float* ko = a.keypoints_out + ((size_t)n * a.J + j) * 3;
        if (gap) {
            ko[0] = 0.f; ko[1] = 0.f; ko[2] = 0.f;
        } else if (copy) {
            ko[0] = k0p[0]; ko[1] = k0p[1]; ko[2] = k0p[2];
        } else {
            const float c0 = k0p[2], c1 = k1p[2];
            if (c0 == 0.f) { ko[0] = k1p[0]; ko[1] = k1p[1]; }
            else if (c1 == 0.f) { ko[0] = k0p[0]; ko[1] = k0p[1]; }
            else {
                ko[0] = (float)((double)k0p[0] + alpha * ((double)k1p[0] - (double)k0p[0]));
                ko[1] = (float)((double)k0p[1] + alpha * ((double)k1p[1] - (double)k0p[1]));
            }
            ko[2] = (c0 == 0.f || c1 == 0.f) ? 0.f : fminf(c0, c1);
        }
    } else {
        const int m = slot - kTrackFixedSlots - a.J;
        const float m0 = a.mask[(size_t)i0 * a.M + m], m1 = a.mask[(size_t)i1 * a.M + m];
        a.mask_out[(size_t)n * a.M + m] = gap ? 0.f : (copy ? m0 : fminf(m0, m1));
    }
}

}  // namespace rohm

using namespace rohm;

extern "C" int rohm_track_resample(const double* times_src, const int* valid_idx, const double* params, const float* keypoints,
                                   const float* mask_joint, const double* times_dst, double max_gap, int N, int Nv, int J, int M,
                                   int n_out, double* params_out, float* keypoints_out, float* mask_out, int* src_index,
                                   unsigned char* gap, rohm_stream_t stream) {
    ROHM_ARG_CHECK(N >= 1 && Nv >= 1 && Nv <= N, "track_resample: need 1 <= Nv <= N (got Nv=%d N=%d)", Nv, N);
    ROHM_ARG_CHECK(n_out >= 0 && J >= 0 && M >= 0, "track_resample: negative size (n_out=%d J=%d M=%d)", n_out, J, M);
    ROHM_ARG_CHECK(max_gap >= 0.0, "track_resample: max_gap must be >= 0 (a NaN is refused too)");
    if (n_out == 0) return ROHM_OK;
    ROHM_ARG_CHECK(times_src && valid_idx && params && times_dst && params_out && src_index && gap, "track_resample: null argument");
    ROHM_ARG_CHECK(J == 0 || (keypoints && keypoints_out), "track_resample: J = %d needs keypoints and keypoints_out", J);
    ROHM_ARG_CHECK(M == 0 || (mask_joint && mask_out), "track_resample: M = %d needs mask_joint and mask_out", M);
    const long long total = (long long)n_out * (kTrackFixedSlots + J + M);
    ROHM_ARG_CHECK((total + 255) / 256 <= 0x7fffffffLL, "track_resample: %lld slots are more than one launch takes", total);
    // the valid list is the host's (a few thousand integers): read it back once and check it, the kernel indexes with it.  That read
    // waits for the stream, and a wait on a recording stream invalidates the caller's capture: refuse before anything is issued.
    if (stream_is_capturing((hipStream_t)stream)) {
        set_error("rohm_track_resample waits for its stream (it checks valid_idx on the host) and cannot be recorded into a graph: call it "
                  "outside the capture");
        return ROHM_ERR_UNSUPPORTED;
    }
    std::vector<int> vi((size_t)Nv);
    ROHM_HIP_CHECK(hipMemcpyAsync(vi.data(), valid_idx, sizeof(int) * (size_t)Nv, hipMemcpyDeviceToHost, (hipStream_t)stream));
    ROHM_HIP_CHECK(hipStreamSynchronize((hipStream_t)stream));
    for (int k = 0; k < Nv; ++k) {
        ROHM_ARG_CHECK(vi[k] >= 0 && vi[k] < N, "track_resample: valid_idx[%d] = %d is outside [0, %d)", k, vi[k], N);
        ROHM_ARG_CHECK(k == 0 || vi[k] > vi[k - 1], "track_resample: valid_idx must be ascending (valid_idx[%d] = %d after %d)", k,
                       vi[k], vi[k - 1]);
    }
    TrackArgs a;
    a.times_src = times_src; a.valid_idx = valid_idx; a.params = params; a.keypoints = keypoints; a.mask = mask_joint;
    a.times_dst = times_dst; a.max_gap = max_gap; a.N = N; a.Nv = Nv; a.J = J; a.M = M; a.n_out = n_out;
    a.params_out = params_out; a.keypoints_out = keypoints_out; a.mask_out = mask_out; a.src_index = src_index; a.gap = gap;
    prof::Scope ps("track_resample", 0.0, (double)n_out * (16.0 * kTrackCols + 24.0 * J + 8.0 * M + 13.0), (hipStream_t)stream);
    hipLaunchKernelGGL(track_resample_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, (hipStream_t)stream, a);
    ROHM_LAUNCH_CHECK();
    return ROHM_OK;
}
