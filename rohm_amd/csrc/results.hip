// The result tails of the test drivers on the device: test_amass_full.py:386-396, test_prox_egobody.py:326-336,
// test_posenet.py:185-195, test_trajnet.py:179-181 (de-normalise the representations) and test_trajnet.py:221-263,
// :333-366 (the trajectory report).
//
// The scripts copy every representation to the host, permute it to [bs, T, 294] and de-normalise it in numpy; here one
// launch reads up to three of them in place -- the sampler's [B, C, 1, T] output or the first T rows of a [B, T', C]
// batch entry, given by strides -- and writes contiguous [B, T, C].  The transpose goes through a padded LDS tile so
// that both the T-contiguous reads and the C-contiguous writes coalesce; rows of T = 143 floats are only 4-byte
// aligned, so the accesses are dwords, and the edge tiles (294 and 143 are no multiples of 32) are predicated.
//
// Numerics follow numpy (2.x, NEP 50) on the drivers' float32 arrays: `x * Std + Mean` is a rounded product and a
// rounded sum; the report's differences, the * 27000 scaling and the norm are single float32 operations in the script's
// order; sums are accumulated in float64.  Contraction into fma is switched off for this file: HIP's __fmul_rn /
// __fadd_rn are plain operators that the default -ffp-contract=fast would fuse.
#include "common.h"

#pragma clang fp contract(off)

namespace rohm {

constexpr int kRTile = 32;                 // tile edge (frames x channels)
constexpr int kRPad = kRTile + 1;          // padded LDS row: the 32 lanes of a column write hit 32 distinct banks
constexpr int kRTraj = 22;                 // channels the optional trajectory rows replace (test_amass_full.py:391)
constexpr int kNReport = 15;               // layout documented in include/rohm_hip.h

struct ResultRowsArgs {
    rohm_result_rows_item it[ROHM_RESULT_ROWS_MAX];
};

// grid (ceil(C / 32), ceil(T / 32), n_items * B), block (32, 8)
__global__ __launch_bounds__(256) void result_rows_kernel(ResultRowsArgs a, int B, int T, int C) {
    __shared__ float tile[kRTile][kRPad];      // [t][c]
    const rohm_result_rows_item& it = a.it[blockIdx.z / B];
    const int b = blockIdx.z % B;
    const int c0 = blockIdx.x * kRTile, t0 = blockIdx.y * kRTile;
    const int tx = threadIdx.x, ty = threadIdx.y;
    const float* src = it.src + (long long)b * it.stride_b;
    if (it.stride_t == 1) {
        // channel-major source ([B, C, 1, T]): lanes run along the frames of one channel
#pragma unroll
        for (int k = 0; k < kRTile; k += 8) {
            const int c = c0 + ty + k, t = t0 + tx;
            if (c < C && t < T) tile[tx][ty + k] = src[(long long)c * it.stride_c + t];
        }
    } else {
        // frame-major source ([B, T', C]): lanes run along the channels of one frame
#pragma unroll
        for (int k = 0; k < kRTile; k += 8) {
            const int t = t0 + ty + k, c = c0 + tx;
            if (c < C && t < T) tile[ty + k][tx] = src[(long long)t * it.stride_t + (long long)c * it.stride_c];
        }
    }
    __syncthreads();
    float* out = it.out + (long long)b * T * C;
    const float* traj = it.traj ? it.traj + (long long)b * it.traj_rows * kRTraj : nullptr;
#pragma unroll
    for (int k = 0; k < kRTile; k += 8) {
        const int t = t0 + ty + k, c = c0 + tx;
        if (c >= C || t >= T) continue;
        float v = tile[ty + k][tx];
        if (traj && c < kRTraj) v = traj[(long long)t * kRTraj + c];      // motion_repr_noisy[:, :, 0:22] = traj_noisy_full[:, 0:-1]
        out[(long long)t * C + c] = v * it.std[c] + it.mean[c];           // two rounded operations (contraction is off)
    }
}

// correctly rounded float32 square root, as numpy's (see csrc/scene_metrics.hip: the device sqrt is only guaranteed to
// within an ulp; a midpoint between two floats squares exactly in float64 and never equals a float)
__device__ __forceinline__ float report_sqrt_rn(float x) {
    float r = sqrtf(x);
    const double dx = (double)x;
    const float lo = nextafterf(r, 0.f);
    const double ml = 0.5 * ((double)lo + (double)r);
    if (ml * ml > dx) r = lo;
    const float hi = nextafterf(r, INFINITY);
    const double mh = 0.5 * ((double)r + (double)hi);
    if (mh * mh < dx) r = hi;
    return r;
}

// (p[t+3] - 3 p[t+2] + 3 p[t+1] - p[t]) * fps ** 3, test_trajnet.py:245: numpy evaluates ((a - 3b) + 3c) - d
__device__ __forceinline__ float jerk(float p0, float p1, float p2, float p3) {
    return (((p3 - 3.f * p2) + 3.f * p1) - p0) * 27000.f;
}

// lane l of the returned value holds the sum over the wave, added in the same butterfly order on every call
__device__ __forceinline__ double report_wave_sum(double v) {
#pragma unroll
    for (int o = 32; o; o >>= 1) v += __shfl_xor(v, o);
    return v;
}

struct TrajReportArgs {
    const float* joints[5];      // clean, noisy, from_abs_traj, from_rel_traj, from_smpl
    const float* rot_clean;
    const float* rot_rec;
    long long rot_clean_stride, rot_rec_stride;
};

// one wave per clip; out [B, 15] doubles; elems [B, 15, T] floats or NULL
__global__ __launch_bounds__(64) void traj_report_kernel(TrajReportArgs a, int T, double* __restrict__ out,
                                                         float* __restrict__ elems) {
    const int b = blockIdx.x, lane = threadIdx.x;
    const long long fs = 22 * 3;                    // floats per frame; joint 0 (the pelvis) is its first three
    const float* jt[5];
#pragma unroll
    for (int k = 0; k < 5; ++k) jt[k] = a.joints[k] + (long long)b * T * fs;
    const float* rc = a.rot_clean + (long long)b * T * a.rot_clean_stride;
    const float* rr = a.rot_rec + (long long)b * T * a.rot_rec_stride;
    float* el = elems ? elems + (long long)b * kNReport * T : nullptr;
    double s[kNReport];
#pragma unroll
    for (int k = 0; k < kNReport; ++k) s[k] = 0.0;
    for (int t = lane; t < T; t += 64) {
        // :222-224, :233: |rot_rec * 2 - rot_clean * 2|
        const float e = fabsf(rr[(long long)t * a.rot_rec_stride] * 2.f - rc[(long long)t * a.rot_clean_stride] * 2.f);
        s[0] += (double)e;
        if (el) el[t] = e;
        // :234-242: |pelvis_rec - pelvis_clean| per axis for the three recoveries
#pragma unroll
        for (int r = 0; r < 3; ++r)
#pragma unroll
            for (int x = 0; x < 3; ++x) {
                const float d = fabsf(jt[2 + r][t * fs + x] - jt[0][t * fs + x]);
                s[1 + r * 3 + x] += (double)d;
                if (el) el[(long long)(1 + r * 3 + x) * T + t] = d;
            }
        // :245-263: jitter of the five pelvis tracks
#pragma unroll
        for (int k = 0; k < 5; ++k) {
            float n = 0.f;
            if (t + 3 < T) {
                const float* p = jt[k] + t * fs;
                const float jx = jerk(p[0], p[fs], p[2 * fs], p[3 * fs]);
                const float jy = jerk(p[1], p[fs + 1], p[2 * fs + 1], p[3 * fs + 1]);
                const float jz = jerk(p[2], p[fs + 2], p[2 * fs + 2], p[3 * fs + 2]);
                n = report_sqrt_rn((jx * jx + jy * jy) + jz * jz);      // np.linalg.norm(axis=-1): add.reduce left to right
                s[10 + k] += (double)n;
            }
            if (el) el[(long long)(10 + k) * T + t] = n;                // frames >= T - 3: 0, not part of the report
        }
    }
#pragma unroll
    for (int k = 0; k < kNReport; ++k) {
        const double v = report_wave_sum(s[k]);
        if (lane == 0) out[(long long)b * kNReport + k] = v;
    }
}

}  // namespace rohm

using namespace rohm;

extern "C" int rohm_result_rows(const rohm_result_rows_item* items, int n_items, int B, int T, int C,
                                rohm_stream_t stream) {
    ROHM_ARG_CHECK(items, "result_rows: null argument");
    ROHM_ARG_CHECK(n_items >= 1 && n_items <= ROHM_RESULT_ROWS_MAX, "result_rows: 1 to %d tensors per launch, got %d",
                   ROHM_RESULT_ROWS_MAX, n_items);
    ROHM_ARG_CHECK(B > 0 && T > 0 && C > 0 && (long long)B * n_items <= 65535,
                   "result_rows: need B, T, C > 0 and B * n_items <= 65535 (got B=%d T=%d C=%d)", B, T, C);
    ResultRowsArgs a;
    for (int i = 0; i < n_items; ++i) {
        const rohm_result_rows_item& it = items[i];
        ROHM_ARG_CHECK(it.src && it.mean && it.std && it.out, "result_rows: null pointer in tensor %d", i);
        ROHM_ARG_CHECK(it.stride_b >= 0 && it.stride_t >= 1 && it.stride_c >= 1 && (it.stride_t == 1 || it.stride_c == 1),
                       "result_rows: tensor %d needs positive strides with frames or channels contiguous "
                       "(got b=%lld t=%lld c=%lld)", i, it.stride_b, it.stride_t, it.stride_c);
        ROHM_ARG_CHECK(!it.traj || (C >= kRTraj && it.traj_rows >= T),
                       "result_rows: tensor %d: trajectory rows need C >= 22 and at least T=%d rows (got C=%d rows=%lld)", i,
                       T, C, it.traj_rows);
        a.it[i] = it;
    }
    for (int i = n_items; i < ROHM_RESULT_ROWS_MAX; ++i) a.it[i] = items[0];
    const double bytes = (double)n_items * B * T * C * 8.0;
    prof::Scope ps("result_rows", 2.0 * n_items * B * T * C, bytes, (hipStream_t)stream);
    dim3 grid((C + kRTile - 1) / kRTile, (T + kRTile - 1) / kRTile, n_items * B);
    hipLaunchKernelGGL(result_rows_kernel, grid, dim3(kRTile, 8), 0, (hipStream_t)stream, a, B, T, C);
    ROHM_LAUNCH_CHECK();
    return ROHM_OK;
}

extern "C" int rohm_traj_report(const float* joints_clean, const float* joints_noisy, const float* joints_from_abs_traj,
                                const float* joints_from_rel_traj, const float* joints_from_smpl, const float* rot_clean,
                                long long rot_clean_stride, const float* rot_rec, long long rot_rec_stride, int B, int T,
                                double* out, float* elems, rohm_stream_t stream) {
    ROHM_ARG_CHECK(joints_clean && joints_noisy && joints_from_abs_traj && joints_from_rel_traj && joints_from_smpl &&
                       rot_clean && rot_rec && out, "traj_report: null argument");
    ROHM_ARG_CHECK(B > 0 && T >= 4, "traj_report: need B > 0 and T >= 4 (the jitter spans 4 frames), got B=%d T=%d", B, T);
    ROHM_ARG_CHECK(rot_clean_stride >= 1 && rot_rec_stride >= 1, "traj_report: strides must be positive");
    TrajReportArgs a;
    a.joints[0] = joints_clean; a.joints[1] = joints_noisy; a.joints[2] = joints_from_abs_traj;
    a.joints[3] = joints_from_rel_traj; a.joints[4] = joints_from_smpl;
    a.rot_clean = rot_clean; a.rot_rec = rot_rec;
    a.rot_clean_stride = rot_clean_stride; a.rot_rec_stride = rot_rec_stride;
    prof::Scope ps("traj_report", 0.0, (double)B * T * (5 * 12.0 + 8.0) + 8.0 * B * kNReport, (hipStream_t)stream);
    hipLaunchKernelGGL(traj_report_kernel, dim3(B), dim3(64), 0, (hipStream_t)stream, a, T, out, elems);
    ROHM_LAUNCH_CHECK();
    return ROHM_OK;
}
