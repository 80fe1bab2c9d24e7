// Evaluation metrics of the PROX / EgoBody driver on the device: eval_prox_egobody.py:172-270.
//
// The script maps every clip back to scene coordinates with inv(trans_scene2cano) (utils/other_utils.py:133-143), then
// reduces [clip_len, 22, 3] joint tracks to foot skating, acceleration, (EgoBody) global / root-relative MPJPE split by
// the visibility mask, and toe ground penetration.  One workgroup per clip, no atomics: each clip's sums depend on its
// own data only, whatever the batch holds.  The back-transform is recomputed wherever a joint is read (9 multiply-adds
// against re-reading a staged copy), so nothing is held in LDS beyond the matrix and the reduction buffer.
//
// Numerics follow numpy (2.x, NEP 50) on the driver's float32 arrays: every difference, norm, threshold test and the
// 30 / 900 scalings are single float32 operations with round-to-nearest, in the script's order; thresholds and the
// floor height are rounded to float32; sums are accumulated in float64.  Contraction into fma is switched off for this
// file: HIP's __fmul_rn / __fadd_rn are plain operators that the default -ffp-contract=fast would fuse.
#include "common.h"

#pragma clang fp contract(off)

#include "reduce.h"      // after the pragma: what it adds is compiled under this file's setting

namespace rohm {

constexpr int kSJ = 22;
constexpr int kNScene = 11;      // layout documented in include/rohm_hip.h
constexpr int kSceneMaxT = 800;
__constant__ int kSFoot[4] = {7, 10, 8, 11};      // eval_prox_egobody.py:189

// correctly rounded float32 square root, as numpy's: the device sqrt is only guaranteed to within an ulp, so its
// result is moved to the neighbour on the other side of a rounding midpoint when there is one.  A midpoint between two
// floats has 25 significant bits, its square is exact in float64, and it never equals a float exactly.
__device__ __forceinline__ float sqrt_rn(float x) {
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

// np.linalg.norm(v, axis=-1) of a float32 3-vector: sqrt(add.reduce(v * v)), reduced left to right
__device__ __forceinline__ float norm3(float a, float b, float c) {
    return sqrt_rn((a * a + b * b) + c * c);
}

// points_coord_trans (other_utils.py:139-143): x . M[:3,:3]^T + M[:3,3], float32
__device__ __forceinline__ void to_scene(const float* __restrict__ p, const float* m, float* q) {
    const float x = p[0], y = p[1], z = p[2];
#pragma unroll
    for (int r = 0; r < 3; ++r)
        q[r] = ((x * m[r * 4 + 0] + y * m[r * 4 + 1]) + z * m[r * 4 + 2]) + m[r * 4 + 3];
}

// (x[t+2] - 2 x[t+1] + x[t]) * fps^2, :213
__device__ __forceinline__ float accel(float x0, float x1, float x2) {
    return ((x2 - 2.f * x1) + x0) * 900.f;
}

__global__ __launch_bounds__(256) void scene_metrics_kernel(const float* __restrict__ jr, const float* __restrict__ s2c,
                                                            const float* __restrict__ ground, int up,
                                                            const float* __restrict__ jg, int T_gt,
                                                            const float* __restrict__ mask, float* __restrict__ jscene,
                                                            double* __restrict__ out, int T) {
    __shared__ double sh[256];
    __shared__ float sm[12];
    const int b = blockIdx.x, tid = threadIdx.x;
    if (tid == 0) {
        // inv(trans_scene2cano[b]) in float64 (Gauss-Jordan, partial pivoting; general 4x4), rounded to float32
        double a[4][8];
        for (int r = 0; r < 4; ++r)
            for (int c = 0; c < 4; ++c) {
                a[r][c] = (double)s2c[(size_t)b * 16 + r * 4 + c];
                a[r][4 + c] = (r == c) ? 1.0 : 0.0;
            }
        for (int c = 0; c < 4; ++c) {
            int p = c;
            for (int r = c + 1; r < 4; ++r)
                if (fabs(a[r][c]) > fabs(a[p][c])) p = r;
            if (p != c)
                for (int k = 0; k < 8; ++k) {
                    const double t = a[c][k];
                    a[c][k] = a[p][k];
                    a[p][k] = t;
                }
            const double inv = 1.0 / a[c][c];      // singular matrix: inf / nan propagate into the metrics
            for (int k = 0; k < 8; ++k) a[c][k] *= inv;
            for (int r = 0; r < 4; ++r) {
                if (r == c) continue;
                const double f = a[r][c];
                for (int k = 0; k < 8; ++k) a[r][k] -= f * a[c][k];
            }
        }
        for (int r = 0; r < 3; ++r)
            for (int c = 0; c < 4; ++c) sm[r * 4 + c] = (float)a[r][4 + c];
    }
    __syncthreads();
    float m[12];
#pragma unroll
    for (int k = 0; k < 12; ++k) m[k] = sm[k];

    const float gh = ground[b];
    const bool z_up = (up == 2);                    // PROX: up z, horizontal (x, y); EgoBody: up y, horizontal (x, z) (:190-199)
    const size_t fs = (size_t)kSJ * 3;              // floats per frame
    const float* r = jr + (size_t)b * T * fs;
    const float* g = jg ? jg + (size_t)b * T_gt * fs : nullptr;
    const float* mk = mask ? mask + (size_t)b * T * kSJ : nullptr;
    float* js = jscene ? jscene + (size_t)b * T * fs : nullptr;

    double s_acc = 0, s_acc_err = 0, n_pene = 0, s_pene = 0, s_glob = 0, s_loc = 0, s_loc_vis = 0, s_vis = 0,
           s_loc_occ = 0, s_occ = 0, n_skate = 0;
    for (int i = tid; i < T * kSJ; i += blockDim.x) {
        const int t = i / kSJ, j = i - t * kSJ;
        float p[3];
        to_scene(r + (size_t)i * 3, m, p);
        if (js) {
#pragma unroll
            for (int k = 0; k < 3; ++k) js[(size_t)i * 3 + k] = p[k];
        }
        if (t + 2 < T) {     // :212-216
            float p1[3], p2[3], ar[3];
            to_scene(r + (size_t)i * 3 + fs, m, p1);
            to_scene(r + (size_t)i * 3 + 2 * fs, m, p2);
#pragma unroll
            for (int k = 0; k < 3; ++k) ar[k] = accel(p[k], p1[k], p2[k]);
            s_acc += (double)norm3(ar[0], ar[1], ar[2]);
            if (g) {
                const float* q = g + (size_t)i * 3;
                float e[3];
#pragma unroll
                for (int k = 0; k < 3; ++k) e[k] = ar[k] - accel(q[k], q[fs + k], q[2 * fs + k]);
                s_acc_err += (double)norm3(e[0], e[1], e[2]);
            }
        }
        if (g) {             // :236-240
            const float* q = g + (size_t)i * 3;
            const float* q0 = g + (size_t)t * fs;
            float p0[3];
            to_scene(r + (size_t)t * fs, m, p0);
            s_glob += (double)norm3(q[0] - p[0], q[1] - p[1], q[2] - p[2]);
            float d[3];
#pragma unroll
            for (int k = 0; k < 3; ++k) d[k] = (q[k] - q0[k]) - (p[k] - p0[k]);
            const float loc = norm3(d[0], d[1], d[2]);
            s_loc += (double)loc;
            if (mk) {
                const float v = mk[i], o = 1.f - v;
                s_loc_vis += (double)(loc * v);
                s_vis += (double)v;
                s_loc_occ += (double)(loc * o);
                s_occ += (double)o;
            }
        }
        if (j == 10 || j == 11) {   // toes, :256-262
            const float d = (z_up ? p[2] : p[1]) - gh;
            if (d < -0.05f) n_pene += 1.0;
            if (!(d >= 0.f)) s_pene += (double)d;       // pene_dist[pene_dist >= 0] = 0 (a NaN stays)
        }
    }
    for (int t = tid; t < T - 1; t += blockDim.x) {      // :186-205
        bool ok = true;
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            float a[3], c[3];
            to_scene(r + (size_t)t * fs + kSFoot[k] * 3, m, a);
            to_scene(r + (size_t)(t + 1) * fs + kSFoot[k] * 3, m, c);
            const float dx = c[0] - a[0], dy = z_up ? c[1] - a[1] : c[2] - a[2];
            const float vel = sqrt_rn(dx * dx + dy * dy) * 30.f;
            const float h = (z_up ? a[2] : a[1]) - gh;
            const float hmax = (k & 1) ? 0.10f : (float)(0.10 + 0.05);
            ok = ok && (vel > 0.10f) && (h < hmax);
        }
        if (ok) n_skate += 1.0;
    }
    const double vals[kNScene] = {n_skate, s_acc, s_acc_err, n_pene, s_pene, s_glob, s_loc, s_loc_vis, s_vis, s_loc_occ, s_occ};
    for (int k = 0; k < kNScene; ++k) {
        const double v = block_tree_reduce(vals[k], sh, SumOp());
        if (tid == 0) out[(size_t)b * kNScene + k] = v;
    }
}

}  // namespace rohm

using namespace rohm;

extern "C" int rohm_scene_metrics(const float* joints_rec, const float* trans_scene2cano, const float* ground_height,
                                  int up_axis, const float* joints_gt, int T_gt, const float* mask_vis,
                                  float* joints_scene, int B, int T, double* out, rohm_stream_t stream) {
    ROHM_ARG_CHECK(joints_rec && trans_scene2cano && ground_height && out, "scene_metrics: null argument");
    ROHM_ARG_CHECK(B > 0 && T >= 3 && T <= kSceneMaxT, "scene_metrics: need B > 0 and 3 <= T <= %d (got B=%d T=%d)",
                   kSceneMaxT, B, T);
    ROHM_ARG_CHECK(up_axis == 1 || up_axis == 2, "scene_metrics: up_axis must be 1 (EgoBody, y) or 2 (PROX, z), got %d",
                   up_axis);
    ROHM_ARG_CHECK(!joints_gt || T_gt >= T, "scene_metrics: joints_gt has %d frames, need at least T=%d", T_gt, T);
    ROHM_ARG_CHECK(!mask_vis || joints_gt, "scene_metrics: mask_vis is only used with joints_gt");
    const double bytes = 4.0 * B * T * kSJ * 3 * (1 + (joints_gt ? 1 : 0) + (joints_scene ? 1 : 0)) +
                         (mask_vis ? 4.0 * B * T * kSJ : 0.0) + 8.0 * B * kNScene;
    prof::Scope ps("scene_metrics", 0.0, bytes, (hipStream_t)stream);
    hipLaunchKernelGGL(scene_metrics_kernel, dim3(B), dim3(256), 0, (hipStream_t)stream, joints_rec, trans_scene2cano,
                       ground_height, up_axis, joints_gt, T_gt, mask_vis, joints_scene, out, T);
    ROHM_LAUNCH_CHECK();
    return ROHM_OK;
}
