// Export of a reconstruction: rows of the 294-channel representation -> per-frame SMPL-X parameters in scene or camera
// coordinates, for all frames of a recording in one launch.
//
// Reference: what eval_prox_egobody.py:275-310 does clip by clip on the host for its renderer -- recover_from_repr_smpl
// 'smplx_params' (data_loaders/motion_representation.py:373-388: rot6d_to_rotmat, data_loaders/common/quaternion.py:482-501,
// then rotation_matrix_to_angle_axis) and inv(trans_scene2cano) -- with the frame change applied to the PARAMETERS instead of
// the vertices: update_globalRT_for_smplx with delta_T given (utils/other_utils.py:221-240).
//
// Per output frame n the row (clip frame_clip[n], row frame_t[n]) is gathered (the stitching of overlapping clips is this
// gather), de-normalised in float32 as `x * std + mean` (two rounded operations: what rohm_result_rows and the reference's
// numpy produce), and everything after that is float64:
//   R  = Gram-Schmidt of the interleaved 6-D vector (the network's vectors are not orthonormal), for the root and 21 joints
//   d  = J0(betas): rest-pose pelvis from the folded regressor
//   A  = rigid . inv(transf[clip])          (general affine inverse; either may be absent)
//   R' = A_R R,   t' = A_R (t + d) + A_t - d
//   rotation vectors through the quaternion with the atan2 angle (scipy's from_matrix / as_rotvec: stable at angle 0,
//   |aa| <= pi), for R' and every body joint.
// A frame is 32 lanes: lane j < 22 converts joint j's rotation, lane 22 the translation, lane 23 copies betas and the
// foot-contact channels.  Eight frames per workgroup.  No atomics, no cross-lane traffic: same input, same bits.
//
// rohm_export_smplx_blend is the same export with a cross-fade instead of the gather where two clips share a frame: both
// candidates go through the device functions below (the same arithmetic, so a frame with one candidate is bit for bit
// rohm_export_smplx's), then the rotations are slerped (rot_priv.h, the rule of rohm_track_resample) and the rest is
// a + alpha (b - a), with the same lane roles.  No counterpart in the reference, which never stitches its clips.
#include <math.h>
#include "common.h"
#include "rot_priv.h"
#include "smplx_fk.h"

// HIP's __fmul_rn / __fadd_rn are plain operators that the default -ffp-contract=fast would fuse: contraction is off for
// this file (as in results.hip), so that the de-normalisation is numpy's rounded product and rounded sum.
#pragma clang fp contract(off)

namespace rohm {

constexpr int kExportFrames = 8;       // frames per workgroup (32 lanes each)
constexpr int kExportCols = 79;        // global_orient 3, transl 3, betas 10, body_pose 63 (the smplx_world layout)
constexpr int kExportDisagree = 23;    // 22 geodesic angles and the pelvis distance (the blend's `disagree`)

// interleaved 6-D vector (a1x a2x a1y a2y a1z a2z) -> row-major R with columns b1, b2, b3; F.normalize's eps 1e-12
__device__ __forceinline__ void rot6d_f64(const double* x, double* R) {
    const double a1[3] = {x[0], x[2], x[4]}, a2[3] = {x[1], x[3], x[5]};
    const double n1 = fmax(sqrt(a1[0] * a1[0] + a1[1] * a1[1] + a1[2] * a1[2]), 1e-12);
    const double b1[3] = {a1[0] / n1, a1[1] / n1, a1[2] / n1};
    const double d = b1[0] * a2[0] + b1[1] * a2[1] + b1[2] * a2[2];
    const double u[3] = {a2[0] - d * b1[0], a2[1] - d * b1[1], a2[2] - d * b1[2]};
    const double n2 = fmax(sqrt(u[0] * u[0] + u[1] * u[1] + u[2] * u[2]), 1e-12);
    const double b2[3] = {u[0] / n2, u[1] / n2, u[2] / n2};
    const double b3[3] = {b1[1] * b2[2] - b1[2] * b2[1], b1[2] * b2[0] - b1[0] * b2[2], b1[0] * b2[1] - b1[1] * b2[0]};
#pragma unroll
    for (int i = 0; i < 3; ++i) { R[i * 3] = b1[i]; R[i * 3 + 1] = b2[i]; R[i * 3 + 2] = b3[i]; }
}

// A = rigid . inv(transf) as rotation part AR [9] and translation At [3]; transf is float32 [4,4] whose last row is
// (0, 0, 0, 1), inverted as a general affine map: inv = [M^-1, -M^-1 t].  Null pointers are identities.
__device__ __forceinline__ void export_affine(const float* __restrict__ transf, const double* __restrict__ rigid, double* AR,
                                              double* At) {
    double iR[9] = {1, 0, 0, 0, 1, 0, 0, 0, 1}, it[3] = {0, 0, 0};
    if (transf) {
        const double m[9] = {transf[0], transf[1], transf[2], transf[4], transf[5], transf[6], transf[8], transf[9], transf[10]};
        const double t[3] = {transf[3], transf[7], transf[11]};
        const double c00 = m[4] * m[8] - m[5] * m[7], c01 = m[5] * m[6] - m[3] * m[8], c02 = m[3] * m[7] - m[4] * m[6];
        const double id = 1.0 / (m[0] * c00 + m[1] * c01 + m[2] * c02);
        iR[0] = c00 * id; iR[1] = (m[2] * m[7] - m[1] * m[8]) * id; iR[2] = (m[1] * m[5] - m[2] * m[4]) * id;
        iR[3] = c01 * id; iR[4] = (m[0] * m[8] - m[2] * m[6]) * id; iR[5] = (m[2] * m[3] - m[0] * m[5]) * id;
        iR[6] = c02 * id; iR[7] = (m[1] * m[6] - m[0] * m[7]) * id; iR[8] = (m[0] * m[4] - m[1] * m[3]) * id;
#pragma unroll
        for (int i = 0; i < 3; ++i) it[i] = -(iR[i * 3] * t[0] + iR[i * 3 + 1] * t[1] + iR[i * 3 + 2] * t[2]);
    }
    if (!rigid) {
#pragma unroll
        for (int i = 0; i < 9; ++i) AR[i] = iR[i];
#pragma unroll
        for (int i = 0; i < 3; ++i) At[i] = it[i];
        return;
    }
#pragma unroll
    for (int i = 0; i < 3; ++i) {
#pragma unroll
        for (int j = 0; j < 3; ++j)
            AR[i * 3 + j] = rigid[i * 4] * iR[j] + rigid[i * 4 + 1] * iR[3 + j] + rigid[i * 4 + 2] * iR[6 + j];
        At[i] = rigid[i * 4] * it[0] + rigid[i * 4 + 1] * it[1] + rigid[i * 4 + 2] * it[2] + rigid[i * 4 + 3];
    }
}

// One row of the representation, de-normalised channel by channel (`mean` null: the row is de-normalised already).
struct ExportRow {
    const float* x;
    long long isc;
    const float* mean;
    const float* stdv;
    __device__ __forceinline__ float operator()(int ch) const {
        const float v = x[(size_t)ch * isc];
        return mean ? v * stdv[ch] + mean[ch] : v;                  // x * Std + Mean: two rounded float32 operations
    }
};

// first column of joint j's rotation vector in a [79] row (j = 0: global_orient)
__device__ __forceinline__ int export_rot_col(int j) { return j == 0 ? 0 : 16 + (j - 1) * 3; }

// the rule of rohm_clips_build for an index outside the arrays: NaN outputs, never a read outside them.  lane < 24 as in
// the kernels below; contact may be null.
__device__ __forceinline__ void export_nan_row(int lane, double* o, float* contact4) {
    const double qnan = __longlong_as_double(0x7ff8000000000000LL);
    if (lane < NJ) {
        const int col = export_rot_col(lane);
        o[col] = qnan; o[col + 1] = qnan; o[col + 2] = qnan;
    } else if (lane == NJ) {
        o[3] = qnan; o[4] = qnan; o[5] = qnan;
    } else {
#pragma unroll
        for (int k = 0; k < NBETA; ++k) o[6 + k] = qnan;
        if (contact4)
#pragma unroll
            for (int k = 0; k < 4; ++k) contact4[k] = __int_as_float(0x7fc00000);
    }
}

// joint j's final rotation vector: Gram-Schmidt of its 6-D vector, A_R from the left for the root
__device__ __forceinline__ void export_rotation(const ExportRow& ldc, int j, const float* tf, const double* rigid, double* rv) {
    double x6[6], R[9];
    const int ch0 = j == 0 ? CH_ROT6D : CH_POSE6D + (j - 1) * 6;
#pragma unroll
    for (int k = 0; k < 6; ++k) x6[k] = (double)ldc(ch0 + k);
    rot6d_f64(x6, R);
    if (j == 0 && (tf || rigid)) {
        double AR[9], At[3], Rn[9];
        export_affine(tf, rigid, AR, At);
#pragma unroll
        for (int i = 0; i < 3; ++i)
#pragma unroll
            for (int k = 0; k < 3; ++k) Rn[i * 3 + k] = AR[i * 3] * R[k] + AR[i * 3 + 1] * R[3 + k] + AR[i * 3 + 2] * R[6 + k];
#pragma unroll
        for (int i = 0; i < 9; ++i) R[i] = Rn[i];
    }
    matrix_to_rotvec_f64(R, rv);
}

// the final translation t' = A_R (t + d) + A_t - d and d, the rest-pose pelvis of the row's betas
__device__ __forceinline__ void export_transl(const ExportRow& ldc, const float* tf, const double* rigid, const float* __restrict__ Jt,
                                              const float* __restrict__ Js, double* out, double* d) {
    double beta[NBETA], tr[3], AR[9], At[3];
#pragma unroll
    for (int k = 0; k < NBETA; ++k) beta[k] = (double)ldc(CH_BETAS + k);
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        double v = (double)Jt[k];                              // joint 0 of the folded regressor: the rest-pose pelvis
#pragma unroll
        for (int b = 0; b < NBETA; ++b) v += (double)Js[k * NBETA + b] * beta[b];
        d[k] = v;
        tr[k] = (double)ldc(CH_TRANS + k) + v;
    }
    export_affine(tf, rigid, AR, At);
#pragma unroll
    for (int i = 0; i < 3; ++i) out[i] = AR[i * 3] * tr[0] + AR[i * 3 + 1] * tr[1] + AR[i * 3 + 2] * tr[2] + At[i] - d[i];
}

__global__ __launch_bounds__(kExportFrames * 32) void export_smplx_kernel(
    const float* __restrict__ repr, long long isb, long long ist, long long isc, const float* __restrict__ mean,
    const float* __restrict__ stdv, const float* __restrict__ transf, const double* __restrict__ rigid,
    const float* __restrict__ Jt, const float* __restrict__ Js, const int* __restrict__ frame_clip,
    const int* __restrict__ frame_t, int C, int T, int N, double* __restrict__ params, float* __restrict__ contact) {
    const int n = blockIdx.x * kExportFrames + (threadIdx.x >> 5);
    const int lane = threadIdx.x & 31;
    if (n >= N || lane >= 24) return;
    const int c = frame_clip[n], t = frame_t[n];
    double* o = params + (size_t)n * kExportCols;
    const bool valid = c >= 0 && c < C && t >= 0 && t < T;
    if (!valid) {
        export_nan_row(lane, o, contact ? contact + (size_t)n * 4 : nullptr);
        return;
    }
    const ExportRow ldc = {repr + (size_t)c * isb + (size_t)t * ist, isc, mean, stdv};
    const float* tf = transf ? transf + (size_t)c * 16 : nullptr;
    if (lane < NJ) {
        double rv[3];
        export_rotation(ldc, lane, tf, rigid, rv);
        const int col = export_rot_col(lane);
        o[col] = rv[0]; o[col + 1] = rv[1]; o[col + 2] = rv[2];
    } else if (lane == NJ) {
        double tr[3], d[3];
        export_transl(ldc, tf, rigid, Jt, Js, tr, d);
        o[3] = tr[0]; o[4] = tr[1]; o[5] = tr[2];
    } else {
#pragma unroll
        for (int k = 0; k < NBETA; ++k) o[6 + k] = (double)ldc(CH_BETAS + k);
        if (contact)
#pragma unroll
            for (int k = 0; k < 4; ++k) contact[(size_t)n * 4 + k] = ldc(CH_CONTACT + k);
    }
}

// The export with a cross-fade over the frames two clips share (rohm_export_smplx_blend).  Candidate a = (frame_clip[n],
// frame_t[n]) and, where frame_clip_b[n] >= 0, candidate b go through the device functions above: one candidate, or
// alpha == 0, leaves candidate a's bits.  Otherwise lane j slerps joint j's two final rotation vectors (rot_priv.h, the rule
// of rohm_track_resample), lane 22 fades the translation, lane 23 betas and contact, each as a + alpha (b - a) in float64.
// disagree [N,23]: per joint the geodesic angle between the candidates, column 22 the distance between their pelvis
// positions transl + d(betas); zero where there is one candidate.
__global__ __launch_bounds__(kExportFrames * 32) void export_smplx_blend_kernel(
    const float* __restrict__ repr, long long isb, long long ist, long long isc, const float* __restrict__ mean,
    const float* __restrict__ stdv, const float* __restrict__ transf, const double* __restrict__ rigid,
    const float* __restrict__ Jt, const float* __restrict__ Js, const int* __restrict__ frame_clip,
    const int* __restrict__ frame_t, const int* __restrict__ frame_clip_b, const int* __restrict__ frame_t_b,
    const double* __restrict__ alpha, int C, int T, int N, double* __restrict__ params, float* __restrict__ contact,
    double* __restrict__ disagree) {
    const int n = blockIdx.x * kExportFrames + (threadIdx.x >> 5);
    const int lane = threadIdx.x & 31;
    if (n >= N || lane >= 24) return;
    const int ca = frame_clip[n], ta = frame_t[n], cb = frame_clip_b[n], tb = frame_t_b[n];
    const bool two = cb >= 0;
    double* o = params + (size_t)n * kExportCols;
    float* oc = contact ? contact + (size_t)n * 4 : nullptr;
    double* od = disagree ? disagree + (size_t)n * kExportDisagree : nullptr;
    const bool valid = ca >= 0 && ca < C && ta >= 0 && ta < T && (!two || (cb < C && tb >= 0 && tb < T));
    if (!valid) {
        export_nan_row(lane, o, oc);
        if (od && lane <= NJ) od[lane] = __longlong_as_double(0x7ff8000000000000LL);
        return;
    }
    const double al = alpha[n];
    const ExportRow la = {repr + (size_t)ca * isb + (size_t)ta * ist, isc, mean, stdv};
    const ExportRow lb = {repr + (size_t)(two ? cb : ca) * isb + (size_t)(two ? tb : ta) * ist, isc, mean, stdv};
    const float* tfa = transf ? transf + (size_t)ca * 16 : nullptr;
    const float* tfb = transf && two ? transf + (size_t)cb * 16 : nullptr;
    if (lane < NJ) {
        double rv[3], dis = 0.0;
        export_rotation(la, lane, tfa, rigid, rv);
        if (two) {
            double rb[3];
            export_rotation(lb, lane, tfb, rigid, rb);
            dis = geodesic_rotvec_f64(rv, rb);
            if (al != 0.0) {
                double ra[3] = {rv[0], rv[1], rv[2]};
                slerp_rotvec_f64(ra, rb, al, rv);
            }
        }
        const int col = export_rot_col(lane);
        o[col] = rv[0]; o[col + 1] = rv[1]; o[col + 2] = rv[2];
        if (od) od[lane] = dis;
    } else if (lane == NJ) {
        double tr[3], d[3], dis = 0.0;
        export_transl(la, tfa, rigid, Jt, Js, tr, d);
        if (two) {
            double trb[3], db[3], s = 0.0;
            export_transl(lb, tfb, rigid, Jt, Js, trb, db);
#pragma unroll
            for (int k = 0; k < 3; ++k) {
                const double e = (trb[k] + db[k]) - (tr[k] + d[k]);
                s += e * e;
                if (al != 0.0) tr[k] = tr[k] + al * (trb[k] - tr[k]);
            }
            dis = sqrt(s);
        }
        o[3] = tr[0]; o[4] = tr[1]; o[5] = tr[2];
        if (od) od[NJ] = dis;
    } else {
        const bool fade = two && al != 0.0;
#pragma unroll
        for (int k = 0; k < NBETA; ++k) {
            const double a = (double)la(CH_BETAS + k);
            o[6 + k] = fade ? a + al * ((double)lb(CH_BETAS + k) - a) : a;
        }
        if (oc)
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                const float a = la(CH_CONTACT + k);
                oc[k] = fade ? (float)((double)a + al * ((double)lb(CH_CONTACT + k) - (double)a)) : a;      // rounded once
            }
    }
}

}  // namespace rohm

using namespace rohm;

extern "C" int rohm_export_smplx(const rohm_smplx_t* h, const float* repr, long long in_stride_b, long long in_stride_t,
                                 long long in_stride_c, const float* mean294, const float* std294, const float* transf,
                                 const double* rigid, const int* frame_clip, const int* frame_t, int C, int T, int N,
                                 double* params, float* contact, rohm_stream_t stream) {
    ROHM_ARG_CHECK(N >= 0 && C >= 0 && T >= 0, "export_smplx: negative size (C=%d T=%d N=%d)", C, T, N);
    if (N == 0) return ROHM_OK;
    ROHM_ARG_CHECK(h && repr && frame_clip && frame_t && params, "export_smplx: null argument");
    ROHM_ARG_CHECK((mean294 == nullptr) == (std294 == nullptr), "export_smplx: pass both mean and std or neither");
    prof::Scope ps("export_smplx", 0.0, (double)N * (4.0 * 155 + 8.0 * kExportCols + 16.0), (hipStream_t)stream);
    hipLaunchKernelGGL(export_smplx_kernel, dim3((N + kExportFrames - 1) / kExportFrames), dim3(kExportFrames * 32), 0,
                       (hipStream_t)stream, repr, in_stride_b, in_stride_t, in_stride_c, mean294, std294, transf, rigid, h->d_Jt,
                       h->d_Js, frame_clip, frame_t, C, T, N, params, contact);
    ROHM_LAUNCH_CHECK();
    return ROHM_OK;
}

extern "C" int rohm_export_smplx_blend(const rohm_smplx_t* h, const float* repr, long long in_stride_b, long long in_stride_t,
                                       long long in_stride_c, const float* mean294, const float* std294, const float* transf,
                                       const double* rigid, const int* frame_clip, const int* frame_t, const int* frame_clip_b,
                                       const int* frame_t_b, const double* alpha, int C, int T, int N, double* params,
                                       float* contact, double* disagree, rohm_stream_t stream) {
    ROHM_ARG_CHECK(N >= 0 && C >= 0 && T >= 0, "export_smplx_blend: negative size (C=%d T=%d N=%d)", C, T, N);
    if (N == 0) return ROHM_OK;
    ROHM_ARG_CHECK(h && repr && frame_clip && frame_t && frame_clip_b && frame_t_b && alpha && params,
                   "export_smplx_blend: null argument");
    ROHM_ARG_CHECK((mean294 == nullptr) == (std294 == nullptr), "export_smplx_blend: pass both mean and std or neither");
    prof::Scope ps("export_smplx_blend", 0.0, (double)N * (2.0 * 4.0 * 155 + 8.0 * (kExportCols + kExportDisagree) + 40.0),
                   (hipStream_t)stream);
    hipLaunchKernelGGL(export_smplx_blend_kernel, dim3((N + kExportFrames - 1) / kExportFrames), dim3(kExportFrames * 32), 0,
                       (hipStream_t)stream, repr, in_stride_b, in_stride_t, in_stride_c, mean294, std294, transf, rigid, h->d_Jt,
                       h->d_Js, frame_clip, frame_t, frame_clip_b, frame_t_b, alpha, C, T, N, params, contact, disagree);
    ROHM_LAUNCH_CHECK();
    return ROHM_OK;
}
