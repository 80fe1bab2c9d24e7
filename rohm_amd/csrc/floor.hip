// The floor of an uncalibrated camera-frame track: toe positions at rest (rohm_floor_candidates), K candidate planes through
// triples of them scored in one launch (rohm_floor_hypotheses) and the sums a least-squares refinement needs
// (rohm_floor_moments).  rohm_amd/floor.py drives them (RANSAC, then numpy.linalg.eigh of a 3x3 covariance on the host).  There
// is no counterpart in the reference: its recordings come with a calibrated scene.  tests/floor_ref.py restates the three
// kernels in numpy; include/rohm_hip.h states the rules in full.
//
// All arithmetic is float64 on the float32 positions, as in quality.hip.  Everything that is compared with a threshold ends
// in an integer count, so the order of a reduction cannot change a bit; the float64 sums of rohm_floor_moments are taken in
// a fixed order.  No atomics: the same input gives the same bits.
//
// rohm_floor_hypotheses is the hot one: K x (P + NJ) signed distances, 3e9 for a ten-minute 60 fps track at K = 4096.  A
// workgroup of 256 threads takes 16 hypotheses: lane (tid % 8) keeps two planes (8 float64) in registers, and the 32 groups
// of 8 lanes (tid / 8) deal the positions of a tile among themselves.  A tile of 1024 positions is staged once through LDS
// as float64 (24 KiB, converted while it is staged; the next tile's loads are issued before this one is counted); the 8
// lanes of a group read the same address (a broadcast), a wave reads 8 neighbouring positions per step, and every value
// read serves two planes.  The workgroup walks all joints first (which side is the body on?), flips its planes, then walks
// the points (the support); the partial counts of the 32 groups meet in three shuffles and one LDS exchange.  K = 4096
// makes 256 workgroups of 4 waves, one per CU; a second launch of one workgroup picks the best score.  Measured at that
// size (scripts/bench_floor.py on one MI355X, a run per version, each run's seven windows within 0.5 % of each other): 16
// lanes along the hypotheses (128 workgroups) 4.9 ms, 8 lanes 3.7 ms, 8 lanes with the next tile's loads in flight 2.1 ms
// -- with one wave per SIMD nothing else hides the staging's latency.
#include "common.h"
#include "reduce.h"

#include <limits.h>

#include <vector>

namespace rohm {

constexpr int kFToe0 = 10;                           // toes are joints 10 and 11 of 22
constexpr int kFJoints = 22;
constexpr int kFThreads = 256;
constexpr int kFHypLanes = 8;                        // lanes of a workgroup along the hypotheses (a power of two below 64)
constexpr int kFPlanesPerLane = 2;
constexpr int kFHypPerBlock = kFHypLanes * kFPlanesPerLane;
constexpr int kFGroups = kFThreads / kFHypLanes;     // 32 groups of lanes share a tile's positions
constexpr int kFTile = 1024;                         // positions per staged tile: 3 x 1024 float64 = 24 KiB
static_assert(kFTile * 3 % kFThreads == 0, "a tile is dealt evenly to the threads that stage it");
constexpr int kFBestThreads = 1024;
constexpr int kFMoments = 11;
constexpr int kFMomThreads = 1024;
constexpr double kFDegenerate = 1e-9;

// ---- candidates: one thread per (valid frame, toe) ----
struct FloorCandArgs {
    const float* joints;          // [N,22,3]
    const double* times;          // [N]
    const int* valid_idx;         // [Nv]
    const float* keypoints;       // [N,22,3] or null
    double conf_min, v_max, max_gap;
    int N, Nv;
    unsigned char* flags;         // [N,2]
};

__global__ __launch_bounds__(256) void floor_flags_clear_kernel(unsigned char* flags, long long n) {
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    if (i < n) flags[i] = 0;
}

__global__ __launch_bounds__(256) void floor_candidates_kernel(const FloorCandArgs a) {
    const long long idx = (long long)blockIdx.x * 256 + threadIdx.x;
    const long long v = idx >> 1;
    const int k = (int)(idx & 1);
    if (v >= a.Nv) return;
    const int i = a.valid_idx[v];
    if (i < 0 || i >= a.N) return;                   // an index outside the track marks nothing and reads nothing
    bool rest = false;
    if (v + 1 < a.Nv) {
        const int i2 = a.valid_idx[v + 1];
        if (i2 > i && i2 < a.N) {
            const double dt = a.times[i2] - a.times[i];
            const size_t e0 = ((size_t)i * kFJoints + kFToe0 + k) * 3, e1 = ((size_t)i2 * kFJoints + kFToe0 + k) * 3;
            const double dx = (double)a.joints[e1] - (double)a.joints[e0], dy = (double)a.joints[e1 + 1] - (double)a.joints[e0 + 1],
                         dz = (double)a.joints[e1 + 2] - (double)a.joints[e0 + 2];
            const double speed = sqrt(dx * dx + dy * dy + dz * dz) / dt;
            // every comparison is false for a NaN: a number that is not finite anywhere in the rule leaves the flag 0
            rest = dt > 0.0 && dt <= a.max_gap && speed < a.v_max;
            if (a.keypoints) rest = rest && (double)a.keypoints[e0 + 2] > a.conf_min;
        }
    }
    a.flags[(size_t)i * 2 + k] = rest ? 1 : 0;
}

// ---- hypotheses ----
struct FloorHypArgs {
    const float* points;          // [P,3]
    const float* joints;          // [NJ,3]
    const int* triples;           // [K,3], checked on the host
    double tau, under_tol;
    int P, NJ, K;
    double* planes;               // [K,4]
    long long* scores;            // [K,3]
    int* best;                    // [1]
};

// Walk `n` positions of `src` in tiles through LDS; this thread looks at positions group, group + 16, ... of every tile.
// kSupport: a[q] += |s| <= tol.  Otherwise a[q] += s > tol and b[q] += s < -tol.  s = n . x + d of plane q.  A NaN counts nowhere.
template <bool kSupport>
__device__ __forceinline__ void floor_count(const float* __restrict__ src, int n, const double (&pl)[kFPlanesPerLane][4], double tol,
                                            double* sh, int tid, int (&a)[kFPlanesPerLane], int (&b)[kFPlanesPerLane]) {
    const int group = tid / kFHypLanes;
    constexpr int kPer = kFTile * 3 / kFThreads;     // floats of a tile per thread
    float next[kPer];
    auto fetch = [&](int base) {                     // the tile's floats into registers; zeros past the end are never read
        const int left = (int)min((long long)kFTile * 3, ((long long)n - base) * 3);
        const float* s = src + (size_t)base * 3;
#pragma unroll
        for (int k = 0; k < kPer; ++k) {
            const int e = tid + k * kFThreads;
            next[k] = e < left ? s[e] : 0.0f;
        }
    };
    if (n > 0) fetch(0);
    for (int base = 0; base < n; base += kFTile) {
        const int cnt = min(kFTile, n - base);
#pragma unroll
        for (int k = 0; k < kPer; ++k) sh[tid + k * kFThreads] = (double)next[k];
        __syncthreads();
        if (base + kFTile < n) fetch(base + kFTile);  // the next tile's loads fly while this one is counted
#pragma unroll 4
        for (int i = group; i < cnt; i += kFGroups) {
            const double x = sh[3 * i], y = sh[3 * i + 1], z = sh[3 * i + 2];
#pragma unroll
            for (int q = 0; q < kFPlanesPerLane; ++q) {
                const double d = pl[q][0] * x + pl[q][1] * y + pl[q][2] * z + pl[q][3];
                if (kSupport) {
                    a[q] += fabs(d) <= tol ? 1 : 0;
                } else {
                    a[q] += d > tol ? 1 : 0;
                    b[q] += d < -tol ? 1 : 0;
                }
            }
        }
        __syncthreads();
    }
}

__global__ __launch_bounds__(kFThreads) void floor_hypotheses_kernel(const FloorHypArgs a) {
    __shared__ double sh[kFTile * 3];
    __shared__ int shc[4 * kFHypLanes];
    const int tid = threadIdx.x;
    const double nan = __longlong_as_double(0x7ff8000000000000ll);
    double pl[kFPlanesPerLane][4];
    bool live[kFPlanesPerLane];
    int hyp[kFPlanesPerLane];
#pragma unroll
    for (int q = 0; q < kFPlanesPerLane; ++q) {
        const long long h = (long long)blockIdx.x * kFHypPerBlock + q * kFHypLanes + tid % kFHypLanes;
        hyp[q] = h < a.K ? (int)h : -1;
        live[q] = false;
        pl[q][0] = pl[q][1] = pl[q][2] = pl[q][3] = nan;
        if (h < a.K) {
            double p[3][3];
#pragma unroll
            for (int c = 0; c < 3; ++c) {
                const int i = min(max(a.triples[(size_t)h * 3 + c], 0), a.P - 1);      // the host checked them; never outside the array
#pragma unroll
                for (int k = 0; k < 3; ++k) p[c][k] = (double)a.points[(size_t)i * 3 + k];
            }
            const double ux = p[1][0] - p[0][0], uy = p[1][1] - p[0][1], uz = p[1][2] - p[0][2];
            const double vx = p[2][0] - p[0][0], vy = p[2][1] - p[0][1], vz = p[2][2] - p[0][2];
            const double nx = uy * vz - uz * vy, ny = uz * vx - ux * vz, nz = ux * vy - uy * vx;
            const double len = sqrt(nx * nx + ny * ny + nz * nz);
            if (len >= kFDegenerate && isfinite(len)) {
                pl[q][0] = nx / len;
                pl[q][1] = ny / len;
                pl[q][2] = nz / len;
                pl[q][3] = -(pl[q][0] * p[0][0] + pl[q][1] * p[0][1] + pl[q][2] * p[0][2]);
                live[q] = true;
            }
        }
    }
    int pos[kFPlanesPerLane] = {0, 0}, neg[kFPlanesPerLane] = {0, 0}, sup[kFPlanesPerLane] = {0, 0}, unused[kFPlanesPerLane] = {0, 0};
    floor_count<false>(a.joints, a.NJ, pl, a.under_tol, sh, tid, pos, neg);
#pragma unroll
    for (int q = 0; q < kFPlanesPerLane; ++q) {
        pos[q] = group_sum<kFHypLanes>(pos[q], shc, tid);
        neg[q] = group_sum<kFHypLanes>(neg[q], shc, tid);
        if (neg[q] > pos[q]) {                       // the body is on the other side: turn the plane over; a tie keeps it
#pragma unroll
            for (int k = 0; k < 4; ++k) pl[q][k] = -pl[q][k];
            neg[q] = pos[q];
        }
    }
    floor_count<true>(a.points, a.P, pl, a.tau, sh, tid, sup, unused);
#pragma unroll
    for (int q = 0; q < kFPlanesPerLane; ++q) {
        sup[q] = group_sum<kFHypLanes>(sup[q], shc, tid);
        if (tid < kFHypLanes && hyp[q] >= 0) {
            const size_t h = (size_t)hyp[q];
#pragma unroll
            for (int k = 0; k < 4; ++k) a.planes[h * 4 + k] = pl[q][k];
            a.scores[h * 3] = live[q] ? (long long)sup[q] - (long long)neg[q] : LLONG_MIN;
            a.scores[h * 3 + 1] = live[q] ? (long long)sup[q] : 0;
            a.scores[h * 3 + 2] = live[q] ? (long long)neg[q] : 0;
        }
    }
}

// ---- moments of the inliers ----
struct FloorMomArgs {
    const float* points;          // [P,3]
    const double* plane;          // [4]
    const double* origin;         // [3]
    double tau;
    int P;
    double* out;                  // [11]
};

// One workgroup: thread t takes the points t, t + 1024, ... in ascending order, then reduce.h's block_reduce (a xor-butterfly per
// wave, the 16 wave partials in wave order).  Tens of thousands of contacts are a few dozen points per thread.
__global__ __launch_bounds__(kFMomThreads) void floor_moments_kernel(const FloorMomArgs a) {
    __shared__ double shm[kFMomThreads / 64][kFMoments];
    const int tid = threadIdx.x;
    const double n0 = a.plane[0], n1 = a.plane[1], n2 = a.plane[2], d = a.plane[3];      // wave-uniform: scalar loads
    const double o0 = a.origin[0], o1 = a.origin[1], o2 = a.origin[2];
    double m[kFMoments];
#pragma unroll
    for (int k = 0; k < kFMoments; ++k) m[k] = 0.0;
    for (int i = tid; i < a.P; i += kFMomThreads) {
        const double x = (double)a.points[(size_t)i * 3], y = (double)a.points[(size_t)i * 3 + 1], z = (double)a.points[(size_t)i * 3 + 2];
        const double r = n0 * x + n1 * y + n2 * z + d;
        if (fabs(r) <= a.tau) {                      // false for a NaN
            const double qx = x - o0, qy = y - o1, qz = z - o2;
            m[0] += 1.0;
            m[1] += qx; m[2] += qy; m[3] += qz;
            m[4] += qx * qx; m[5] += qx * qy; m[6] += qx * qz;
            m[7] += qy * qy; m[8] += qy * qz; m[9] += qz * qz;
            m[10] += r * r;
        }
    }
    block_reduce<kFMomThreads, kFMoments>(m, shm, a.out, SumOfK());
}

}  // namespace rohm

using namespace rohm;

extern "C" int rohm_floor_candidates(const float* joints, const double* times, const int* valid_idx, const float* keypoints, int N,
                                     int Nv, float conf_min, double v_max, double max_gap, unsigned char* flags,
                                     rohm_stream_t stream) {
    ROHM_ARG_CHECK(N >= 0 && Nv >= 0 && Nv <= N, "floor_candidates: need 0 <= Nv <= N (got Nv=%d N=%d)", Nv, N);
    ROHM_ARG_CHECK(v_max > 0.0, "floor_candidates: v_max must be positive (a NaN is refused too)");
    ROHM_ARG_CHECK(max_gap >= 0.0, "floor_candidates: max_gap must be >= 0 (a NaN is refused too)");
    ROHM_ARG_CHECK(!keypoints || conf_min == conf_min, "floor_candidates: conf_min is NaN");
    if (N == 0) return ROHM_OK;
    ROHM_ARG_CHECK(joints && times && flags && (valid_idx || Nv == 0), "floor_candidates: null argument");
    FloorCandArgs a;
    a.joints = joints; a.times = times; a.valid_idx = valid_idx; a.keypoints = keypoints;
    a.conf_min = (double)conf_min; a.v_max = v_max; a.max_gap = max_gap; a.N = N; a.Nv = Nv; a.flags = flags;
    prof::Scope ps("floor_candidates", 0.0, (double)Nv * (2.0 * 24.0 + 16.0 + 4.0 + (keypoints ? 8.0 : 0.0)) + 4.0 * N, (hipStream_t)stream);
    const long long n_flags = 2ll * N, n_threads = 2ll * Nv;
    hipLaunchKernelGGL(floor_flags_clear_kernel, dim3((unsigned)((n_flags + 255) / 256)), dim3(256), 0, (hipStream_t)stream, flags, n_flags);
    ROHM_LAUNCH_CHECK();
    if (Nv == 0) return ROHM_OK;
    hipLaunchKernelGGL(floor_candidates_kernel, dim3((unsigned)((n_threads + 255) / 256)), dim3(256), 0, (hipStream_t)stream, a);
    ROHM_LAUNCH_CHECK();
    return ROHM_OK;
}

extern "C" int rohm_floor_hypotheses(const float* points, int P, const float* joints, int NJ, const int* triples, int K, double tau,
                                     double under_tol, double* planes, long long* scores, int* best, rohm_stream_t stream) {
    ROHM_ARG_CHECK(P >= 0 && NJ >= 0 && K >= 0, "floor_hypotheses: negative size (P=%d NJ=%d K=%d)", P, NJ, K);
    ROHM_ARG_CHECK(tau >= 0.0 && under_tol >= 0.0, "floor_hypotheses: tau and under_tol must be >= 0 (a NaN is refused too)");
    if (K == 0) return ROHM_OK;
    ROHM_ARG_CHECK(P >= 3, "floor_hypotheses: a plane needs 3 points, got P=%d with K=%d", P, K);
    ROHM_ARG_CHECK(points && triples && planes && scores && best && (joints || NJ == 0), "floor_hypotheses: null argument");
    ROHM_ARG_CHECK((long long)P * 3 <= INT_MAX && (long long)NJ * 3 <= INT_MAX, "floor_hypotheses: P=%d or NJ=%d is more than one launch takes", P, NJ);
    // the triples are the host's (K x 3 integers): read them back once and check them, the kernel indexes with them.  That read waits
    // for the stream, and a wait on a recording stream invalidates the caller's capture: refuse before anything is issued.
    if (stream_is_capturing((hipStream_t)stream)) {
        set_error("rohm_floor_hypotheses waits for its stream (it checks the triples on the host) and cannot be recorded into a graph: call "
                  "it outside the capture");
        return ROHM_ERR_UNSUPPORTED;
    }
    std::vector<int> tr((size_t)K * 3);
    ROHM_HIP_CHECK(hipMemcpyAsync(tr.data(), triples, sizeof(int) * tr.size(), hipMemcpyDeviceToHost, (hipStream_t)stream));
    ROHM_HIP_CHECK(hipStreamSynchronize((hipStream_t)stream));
    for (size_t k = 0; k < tr.size(); ++k)
        ROHM_ARG_CHECK(tr[k] >= 0 && tr[k] < P, "floor_hypotheses: triples[%d][%d] = %d is outside [0, %d)", (int)(k / 3), (int)(k % 3), tr[k], P);
    FloorHypArgs a;
    a.points = points; a.joints = joints; a.triples = triples; a.tau = tau; a.under_tol = under_tol;
    a.P = P; a.NJ = NJ; a.K = K; a.planes = planes; a.scores = scores; a.best = best;
    const unsigned blocks = (unsigned)(((long long)K + kFHypPerBlock - 1) / kFHypPerBlock);
    prof::Scope ps("floor_hypotheses", 8.0 * (double)K * ((double)P + (double)NJ), (double)blocks * 12.0 * ((double)P + (double)NJ) + 68.0 * K,
                   (hipStream_t)stream);
    hipLaunchKernelGGL(floor_hypotheses_kernel, dim3(blocks), dim3(kFThreads), 0, (hipStream_t)stream, a);
    ROHM_LAUNCH_CHECK();
    // a degenerate triple scores LLONG_MIN, below any live score (support minus under-count may be negative): all of them degenerate gives -1
    hipLaunchKernelGGL((best_score_kernel<kFBestThreads, 3, LLONG_MIN + 1>), dim3(1), dim3(kFBestThreads), 0, (hipStream_t)stream, scores, K, best);
    ROHM_LAUNCH_CHECK();
    return ROHM_OK;
}

extern "C" int rohm_floor_moments(const float* points, int P, const double* plane, const double* origin, double tau, double* out,
                                  rohm_stream_t stream) {
    ROHM_ARG_CHECK(P >= 0, "floor_moments: P must be >= 0, got %d", P);
    ROHM_ARG_CHECK(tau >= 0.0, "floor_moments: tau must be >= 0 (a NaN is refused too)");
    if (P == 0) return ROHM_OK;
    ROHM_ARG_CHECK(points && plane && origin && out, "floor_moments: null argument");
    ROHM_ARG_CHECK((long long)P * 3 <= INT_MAX, "floor_moments: P=%d is more than one launch takes", P);
    FloorMomArgs a;
    a.points = points; a.plane = plane; a.origin = origin; a.tau = tau; a.P = P; a.out = out;
    prof::Scope ps("floor_moments", 0.0, 12.0 * P, (hipStream_t)stream);
    hipLaunchKernelGGL(floor_moments_kernel, dim3(1), dim3(kFMomThreads), 0, (hipStream_t)stream, a);
    ROHM_LAUNCH_CHECK();
    return ROHM_OK;
}
