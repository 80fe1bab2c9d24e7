// Scores of a stitched track that need no ground truth: per 30 fps frame the reprojection residual against the detected
// keypoints, foot skating, acceleration, toe / floor penetration and the distance to the input track, plus their sums
// split into observed and in-filled frames (rohm_track_quality); and the clearance of a whole mesh above the floor
// (rohm_floor_clearance).  There is no counterpart in the reference: its evaluation (eval_prox_egobody.py:172-270,
// csrc/scene_metrics.hip) works per clip in canonical frames against ground truth and counts overlapping frames twice.
// tests/quality_ref.py restates both kernels in numpy.
//
// rohm_track_quality: frames are independent, so one half-wave (32 lanes) takes one frame and lane j < 22 joint j; a
// 256-thread workgroup takes 8 frames.  Flags and counts are ballots, sums and the maximum a xor-butterfly over the 32
// lanes: a fixed order, every lane ends with the same bits.  All arithmetic is float64 on the float32 inputs.  A second
// launch of one workgroup reduces the rows (and the toe heights, which the rows do not hold per toe) to totals [2,15] in a
// fixed order: thread i takes frames i, i + 1024, ..., then reduce.h's block_reduce, with max_nan in column 3.  No
// atomics, no workspace: the same input gives the same bits.
//
// NaN rules (what the tests pin): a value is NaN exactly when a number it reads is.  The thresholds are written so that a
// NaN reaches the result instead of failing a comparison silently: a joint with confidence above conf_min whose camera
// coordinates are not finite makes columns 0 .. 2 NaN; a foot joint with a NaN speed or height makes skate NaN.
#include "common.h"
#include "reduce.h"

namespace rohm {

constexpr int kQJ = 22;
constexpr int kQCols = 10;
constexpr int kQTot = 15;
constexpr int kQFramesPerBlock = 8;                  // 256 threads / 32 lanes
constexpr unsigned kQFootBits = (1u << 7) | (1u << 8) | (1u << 10) | (1u << 11);      // ankles 7, 8 and toes 10, 11
constexpr unsigned kQToeBits = (1u << 10) | (1u << 11);
constexpr int kQTotThreads = 1024;
constexpr int kQShfl = 32;                           // the width a half-wave hands to its shuffles

struct QualityArgs {
    const float* joints;          // [N,22,3]
    const float* keypoints;       // [N,22,3] or null
    const float* joints_ref;      // [N,22,3] or null
    const float* mask_ref;        // [N,22] or null
    const unsigned char* gap;     // [N] or null
    const double* scene2cam;      // [16] row-major or null; rows 0 .. 2 are read
    double fx, fy, cx, cy, fps, ground, conf_min;
    int N, up, has_floor, has_cam;
    double* rows;                 // [N,10]
    double* totals;               // [2,15]
};

__device__ __forceinline__ unsigned half_ballot(bool p, int lane) {
    const unsigned long long b = __ballot(p);
    return (unsigned)((lane & 32) ? (b >> 32) : (b & 0xffffffffull));
}

__device__ __forceinline__ double height_of(const double* p, int up) { return up == 2 ? p[2] : p[1]; }

__global__ __launch_bounds__(256) void track_quality_kernel(const QualityArgs a) {
    const int lane = threadIdx.x & 63, j = threadIdx.x & 31;
    const long long t = (long long)blockIdx.x * kQFramesPerBlock + (threadIdx.x >> 5);
    const bool frame = t < a.N, on = frame && j < kQJ;
    const double nan = __longlong_as_double(0x7ff8000000000000ll);
    const size_t e = ((size_t)(frame ? t : 0) * kQJ + (j < kQJ ? j : 0)) * 3;       // this lane's joint, always inside the arrays
    const size_t fs = (size_t)kQJ * 3;
    const bool has1 = t + 1 < a.N, has2 = t + 2 < a.N;

    double p0[3], p1[3], p2[3];
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        p0[k] = (double)a.joints[e + k];
        p1[k] = has1 ? (double)a.joints[e + fs + k] : 0.0;
        p2[k] = has2 ? (double)a.joints[e + 2 * fs + k] : 0.0;
    }

    // ---- reprojection residual: columns 0 .. 2 ----
    double s_cd = 0.0, s_c = 0.0, d_max = -1.0;
    bool qual = false, bad = false;
    if (a.has_cam && on) {
        double m[12];
#pragma unroll
        for (int k = 0; k < 12; ++k) m[k] = a.scene2cam[k];      // wave-uniform: scalar loads
        const double u = (double)a.keypoints[e], v = (double)a.keypoints[e + 1], c = (double)a.keypoints[e + 2];
        if (c > a.conf_min) {
            const double X = m[0] * p0[0] + m[1] * p0[1] + m[2] * p0[2] + m[3];
            const double Y = m[4] * p0[0] + m[5] * p0[1] + m[6] * p0[2] + m[7];
            const double Z = m[8] * p0[0] + m[9] * p0[1] + m[10] * p0[2] + m[11];
            bad = !(isfinite(X) && isfinite(Y) && isfinite(Z));
            qual = !bad && Z > 0.0;
            if (qual) {
                const double du = a.fx * X / Z + a.cx - u, dv = a.fy * Y / Z + a.cy - v;
                const double d = sqrt(du * du + dv * dv);
                s_cd = c * d;
                s_c = c;
                d_max = d;
            }
        }
    }
    const unsigned qual_bits = half_ballot(qual, lane), bad_bits = half_ballot(bad, lane);
    s_cd = lanes_sum<32, kQShfl>(s_cd);
    s_c = lanes_sum<32, kQShfl>(s_c);
    d_max = lanes_reduce<32, kQShfl>(d_max, MaxNanOp());
    double col0 = nan, col1 = nan, col2 = 0.0;
    if (a.has_cam) {
        const int n = __popc(qual_bits);
        col2 = bad_bits ? nan : (double)n;
        if (!bad_bits && n > 0) {
            col0 = s_cd / s_c;
            col1 = d_max;
        }
    }

    // ---- skating of the pair (t, t + 1): column 3; toe penetration: column 5 ----
    const double h = height_of(p0, a.up) - a.ground;
    const double dx = p1[0] - p0[0], dy = a.up == 2 ? p1[1] - p0[1] : p1[2] - p0[2];
    const double vel = sqrt(dx * dx + dy * dy) * a.fps;
    const bool toe = (kQToeBits >> j) & 1u;
    const bool foot_ok = vel > 0.10 && h < (toe ? 0.10 : 0.15);
    const bool foot_nan = vel != vel || h != h;
    const unsigned ok_bits = half_ballot(on && foot_ok, lane), nan_bits = half_ballot(on && foot_nan, lane);
    double col3 = nan;
    if (a.has_floor && has1) col3 = (nan_bits & kQFootBits) ? nan : ((ok_bits & kQFootBits) == kQFootBits ? 1.0 : 0.0);
    const double pen = h < 0.0 ? h : (h != h ? h : 0.0);      // min(d, 0), a NaN stays
    const double pen10 = __shfl(pen, 10, 32), pen11 = __shfl(pen, 11, 32);
    double col5 = nan;
    if (a.has_floor) col5 = (pen10 != pen10 || pen11 != pen11) ? nan : (pen10 < pen11 ? pen10 : pen11);

    // ---- acceleration of the triple (t, t + 1, t + 2): column 4 ----
    double acc = 0.0;
    if (on && has2) {
        const double ax = (p2[0] - 2.0 * p1[0]) + p0[0], ay = (p2[1] - 2.0 * p1[1]) + p0[1], az = (p2[2] - 2.0 * p1[2]) + p0[2];
        acc = sqrt(ax * ax + ay * ay + az * az) * (a.fps * a.fps);
    }
    acc = lanes_sum<32, kQShfl>(acc);
    const double col4 = has2 ? acc / (double)kQJ : nan;

    // ---- distance to the input track, split by its visibility mask: columns 6 .. 8 ----
    const double mk = (on && a.mask_ref) ? (double)a.mask_ref[(size_t)t * kQJ + j] : 1.0;
    const bool vis = on && mk == 1.0, occ = on && mk == 0.0;
    const int n_vis = __popc(half_ballot(vis, lane)), n_occ = __popc(half_ballot(occ, lane));
    double dev = 0.0;
    if (a.joints_ref && on) {
        const double ex = p0[0] - (double)a.joints_ref[e], ey = p0[1] - (double)a.joints_ref[e + 1],
                     ez = p0[2] - (double)a.joints_ref[e + 2];
        dev = sqrt(ex * ex + ey * ey + ez * ez);
    }
    const double s_vis = lanes_sum<32, kQShfl>(vis ? dev : 0.0), s_occ = lanes_sum<32, kQShfl>(occ ? dev : 0.0);
    const double col6 = (a.joints_ref && n_vis > 0) ? s_vis / (double)n_vis : nan;
    const double col7 = (a.joints_ref && n_occ > 0) ? s_occ / (double)n_occ : nan;

    if (frame && j < kQCols) {
        const double col9 = (a.gap && a.gap[t]) ? 1.0 : 0.0;
        const double vals[kQCols] = {col0, col1, col2, col3, col4, col5, col6, col7, (double)n_vis, col9};
        double v = vals[0];
#pragma unroll
        for (int k = 1; k < kQCols; ++k) v = (j == k) ? vals[k] : v;
        a.rows[(size_t)t * kQCols + j] = v;
    }
}

// rows [N,10] (+ the toe heights) -> totals [2,15]; one workgroup.  acc holds the two groups' 15 values side by side, as totals does.
__global__ __launch_bounds__(kQTotThreads) void track_quality_totals_kernel(const QualityArgs a) {
    __shared__ double sh[kQTotThreads / 64][2 * kQTot];
    const int tid = threadIdx.x;
    const double nan = __longlong_as_double(0x7ff8000000000000ll);
    double acc[2 * kQTot];
#pragma unroll
    for (int k = 0; k < 2 * kQTot; ++k) acc[k] = (k % kQTot == 3) ? -1.0 : 0.0;      // column 3 is a maximum of distances >= 0
    for (int t = tid; t < a.N; t += kQTotThreads) {
        const double* r = a.rows + (size_t)t * kQCols;
        double v[kQTot];
#pragma unroll
        for (int k = 0; k < kQTot; ++k) v[k] = 0.0;
        v[0] = 1.0;
        v[3] = -1.0;
        if (r[0] == r[0]) { v[1] = r[0]; v[2] = 1.0; v[3] = r[1]; }
        if (r[3] == r[3]) { v[4] = r[3]; v[5] = 1.0; }
        if (r[4] == r[4]) { v[6] = r[4]; v[7] = 1.0; }
        if (a.has_floor) {
#pragma unroll
            for (int toe = 10; toe <= 11; ++toe) {
                const double d = (double)a.joints[((size_t)t * kQJ + toe) * 3 + (a.up == 2 ? 2 : 1)] - a.ground;
                if (d == d) {
                    v[8] += d < -0.05 ? 1.0 : 0.0;
                    v[9] += d < 0.0 ? d : 0.0;
                    v[10] += 1.0;
                }
            }
        }
        if (r[6] == r[6]) { v[11] = r[6]; v[12] = 1.0; }
        if (r[7] == r[7]) { v[13] = r[7]; v[14] = 1.0; }
        const bool g1 = r[9] != 0.0;
#pragma unroll
        for (int k = 0; k < kQTot; ++k) {
            if (k == 3) {
                acc[k] = g1 ? acc[k] : max_nan(acc[k], v[k]);
                acc[kQTot + k] = g1 ? max_nan(acc[kQTot + k], v[k]) : acc[kQTot + k];
            } else {
                acc[k] += g1 ? 0.0 : v[k];
                acc[kQTot + k] += g1 ? v[k] : 0.0;
            }
        }
    }
    block_reduce<kQTotThreads, 2 * kQTot>(acc, sh, a.totals, [](int k, double x, double y) { return (k % kQTot == 3) ? max_nan(x, y) : x + y; });
    __syncthreads();
    if (tid < 2) {      // the maximum of a group without a reprojection residual is NaN
        if (a.totals[tid * kQTot + 2] == 0.0) a.totals[tid * kQTot + 3] = nan;
    }
}

// ---- floor clearance of a mesh: one workgroup per frame ----
__global__ __launch_bounds__(256) void floor_clearance_kernel(const float* __restrict__ verts, int V, int up, double ground,
                                                              double below, double* __restrict__ out) {
    __shared__ double sh_h[4];
    __shared__ int sh_i[4];
    __shared__ int sh_n[4];
    const int tid = threadIdx.x;
    const float* v = verts + (size_t)blockIdx.x * V * 3 + (up == 2 ? 2 : 1);
    Scored<double> low = {__longlong_as_double(0x7ff0000000000000ll), 0x7fffffff};      // the lowest vertex; the lower index on ties
    int n_below = 0, not_finite = 0;
    for (int i = tid; i < V; i += 256) {
        const double h = (double)v[(size_t)i * 3] - ground;
        not_finite |= !isfinite(h);
        low = better_of<true>(low, Scored<double>{h, i});
        n_below += h < -below ? 1 : 0;
    }
    n_below = lanes_sum<64>(n_below);
    const int any_bad = __syncthreads_or(not_finite);
    if ((tid & 63) == 0) sh_n[tid >> 6] = n_below;
    low = block_arg_best<256, true>(low, sh_h, sh_i);      // its barrier publishes sh_n too
    if (tid == 0) {
        const int n = sh_n[0] + sh_n[1] + sh_n[2] + sh_n[3];
        const double nan = __longlong_as_double(0x7ff8000000000000ll);
        double* o = out + (size_t)blockIdx.x * 3;
        o[0] = any_bad ? nan : low.s;
        o[1] = any_bad ? -1.0 : (double)low.h;
        o[2] = any_bad ? nan : (double)n;
    }
}

}  // namespace rohm

using namespace rohm;

extern "C" int rohm_track_quality(const float* joints, int N, double fps, int up_axis, int has_floor, float ground_height,
                                  const double* scene2cam, double fx, double fy, double cx, double cy, const float* keypoints,
                                  float conf_min, const float* joints_ref, const float* mask_ref, const unsigned char* gap,
                                  double* rows, double* totals, rohm_stream_t stream) {
    ROHM_ARG_CHECK(N >= 0, "track_quality: N must be >= 0, got %d", N);
    ROHM_ARG_CHECK(up_axis == 1 || up_axis == 2, "track_quality: up_axis must be 1 (y) or 2 (z), got %d", up_axis);
    ROHM_ARG_CHECK(fps > 0.0 && fps < 1e6, "track_quality: fps must be positive and finite");
    ROHM_ARG_CHECK(!has_floor || ground_height == ground_height, "track_quality: ground_height is NaN");
    ROHM_ARG_CHECK((scene2cam != nullptr) == (keypoints != nullptr),
                   "track_quality: scene2cam and keypoints go together (both or neither)");
    ROHM_ARG_CHECK(conf_min == conf_min, "track_quality: conf_min is NaN");
    if (N == 0) return ROHM_OK;
    ROHM_ARG_CHECK(joints && rows && totals, "track_quality: null argument");
    QualityArgs a;
    a.joints = joints; a.keypoints = keypoints; a.joints_ref = joints_ref; a.mask_ref = mask_ref; a.gap = gap;
    a.fx = fx; a.fy = fy; a.cx = cx; a.cy = cy; a.fps = fps; a.ground = has_floor ? (double)ground_height : 0.0;
    a.conf_min = (double)conf_min;
    a.N = N; a.up = up_axis; a.has_floor = has_floor ? 1 : 0; a.has_cam = scene2cam ? 1 : 0;
    a.rows = rows; a.totals = totals;
    a.scene2cam = scene2cam;
    const unsigned blocks = (unsigned)(((long long)N + kQFramesPerBlock - 1) / kQFramesPerBlock);
    const double bytes = (double)N * (4.0 * kQJ * 3 * (3 + (keypoints ? 1 : 0) + (joints_ref ? 1 : 0)) + (mask_ref ? 4.0 * kQJ : 0.0) +
                                      2.0 * 8.0 * kQCols + 1.0);
    prof::Scope ps("track_quality", 0.0, bytes, (hipStream_t)stream);
    hipLaunchKernelGGL(track_quality_kernel, dim3(blocks), dim3(256), 0, (hipStream_t)stream, a);
    ROHM_LAUNCH_CHECK();
    hipLaunchKernelGGL(track_quality_totals_kernel, dim3(1), dim3(kQTotThreads), 0, (hipStream_t)stream, a);
    ROHM_LAUNCH_CHECK();
    return ROHM_OK;
}

extern "C" int rohm_floor_clearance(const float* verts, int n, int V, int up_axis, float ground_height, float below, double* out,
                                    rohm_stream_t stream) {
    ROHM_ARG_CHECK(n >= 0 && V >= 1, "floor_clearance: need n >= 0 and V >= 1 (got n=%d V=%d)", n, V);
    ROHM_ARG_CHECK(up_axis == 1 || up_axis == 2, "floor_clearance: up_axis must be 1 (y) or 2 (z), got %d", up_axis);
    ROHM_ARG_CHECK(ground_height == ground_height && below == below, "floor_clearance: ground_height or below is NaN");
    if (n == 0) return ROHM_OK;
    ROHM_ARG_CHECK(verts && out, "floor_clearance: null argument");
    prof::Scope ps("floor_clearance", 0.0, (double)n * (12.0 * V + 24.0), (hipStream_t)stream);
    hipLaunchKernelGGL(floor_clearance_kernel, dim3((unsigned)n), dim3(256), 0, (hipStream_t)stream, verts, V, up_axis,
                       (double)ground_height, (double)below, out);
    ROHM_LAUNCH_CHECK();
    return ROHM_OK;
}
