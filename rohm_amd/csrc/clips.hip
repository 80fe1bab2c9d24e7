// Test-time clips of a PROX / EgoBody recording on the device.
//
// Reference: data_loaders/dataloader_video.py::create_body_repr (:373-403) and __getitem__ (:421-498), which run per
// clip on the host: cano_seq_smplx / cano_seq_smplx_egobody (data_loaders/motion_representation.py:47-184),
// update_globalRT_for_smplx (utils/other_utils.py:221-240), get_repr_smplx (:187-282), cv2.undistortPoints on the
// OpenPose keypoints and the visibility-mask assembly.  Here: all clips of a recording in one launch, one workgroup
// per clip, windows read in place from the two arrays rohm_smplx_frames_to_world returns.
//
// Dtype flow of the reference (it decides the last bits, cf. rederive.hip):
//   * the floor is the min of the float32 world joints and is subtracted in float32 (a preset floor is rounded to
//     float32 there, but enters transf_matrix unrounded); `if preset_floor_height:` treats 0.0 as "not given";
//   * from the frame-0 translation on the canonical joints are float64 (float32 array minus float32 * int64 array),
//     so are the canonical parameters and transf_matrix;
//   * get_repr_smplx then sees float64 joints: the facing direction, the foot-contact decisions, root position and
//     height, the rotation matrices and the angular velocity are float64; qbetween / qmul / qrot cast their float64
//     arguments to float32 and compute in float32 WITHOUT fma contraction (quaternion.py:21-23,126-135,397-406);
//   * one rounding to float32 at the store, after the optional float64 normalisation.
// cano_seq_smplx unpacks face_joint_indx as r_hip = 2, l_hip = 1; get_repr_smplx unpacks it with the hips swapped.
// No float atomics; the floor is a min-reduction (order-independent), so results are bitwise reproducible.
#include "common.h"
#include "rot_priv.h"
#include "smplx_fk.h"

namespace rohm {

constexpr int kClipThreads = 512;
constexpr int kWorldCols = 79;                 // global_orient 3, transl 3, betas 10, body_pose 63
constexpr int kFrameLds = NJ * 3 * 8;          // float64 canonical joints of one frame
constexpr int kFrameAux = 9 * 8 + 3 * 8 + 4 * 4;   // R (f64), transl (f64), root quaternion (f32)
constexpr int kFixedLds = 64;                  // wave minima + first-NaN index
constexpr int kLdsMax = 160 * 1024;
constexpr int CH_LOCAL_VEL = CH_LOCAL + NJ * 3;

struct ClipArgs {
    const float* joints;      // [N,22,3] world
    const double* world;      // [N,79]
    const int* starts;        // [C] or null
    int step, N, L, up;       // start_c = c * step when starts is null; up = 2 (z) or 1 (y)
    int has_preset;
    double preset;
    double A[9];              // extra axis rotations after the facing rotation (identity for z up)
    const float* mean;        // [294] or null
    const float* stdv;
    float* repr;              // [C,L-1,294]
    float* cano_joints;       // [C,L,22,3]
    float* cano_orient;       // [C,L,3]
    float* cano_transl;       // [C,L,3]
    float* transf;            // [C,4,4]
    double* orient_transl64;  // [C,L,6] canonical global_orient, transl before the float32 store, or null
    double* scratch;          // [C,L,66] when the joints do not fit into LDS, else null
};

__device__ __forceinline__ void mat3_vec(const double* M, const double* v, double* o) {
#pragma unroll
    for (int i = 0; i < 3; ++i) o[i] = M[i * 3] * v[0] + M[i * 3 + 1] * v[1] + M[i * 3 + 2] * v[2];
}

__device__ __forceinline__ double dsq3(double a, double b, double c) {      // x**2 + y**2 + z**2, left to right, no fma
    return __dadd_rn(__dadd_rn(__dmul_rn(a, a), __dmul_rn(b, b)), __dmul_rn(c, c));
}

// get_repr_smplx (:187-282) on canonical joints cj [L,22,3] (float64 storage, LDS or scratch), the rotation matrices sR [L,9]
// and translations sT [L,3] of the canonical global_orient / transl, and parameter rows W [L,79] (betas, body_pose); sQ [L,4]
// and first_nan (== L on entry) are workgroup storage.  All of it must be visible to the workgroup on entry.  F32: the joints
// are float32 values (the noisy joints of the AMASS loader), so what the reference computes in the joints' dtype -- the
// across vector and its normalisation, the differences behind local_positions / local_vel / root_l_vel and the squared
// foot velocities -- is float32 arithmetic without fma contraction.
template <bool F32>
__device__ __forceinline__ void repr_from_canonical(const double* cj, const double* sR, const double* sT, float* sQ, int* first_nan,
                                                    const double* W, int L, const float* mean, const float* stdv, float* o_repr) {
    const int tid = threadIdx.x;
    auto dif = [](double x, double y) -> double { return F32 ? (double)sub((float)x, (float)y) : x - y; };
    auto sq3 = [](double x, double y, double z) -> double {     // x**2 + y**2 + z**2 in the joints' dtype
        if (!F32) return dsq3(x, y, z);
        const float fx = (float)x, fy = (float)y, fz = (float)z;
        return (double)add(add(mul(fx, fx), mul(fy, fy)), mul(fz, fz));
    };
    // ---- root quaternion of every frame from the facing direction --------------------------------------------------------
    for (int f = tid; f < L; f += blockDim.x) {
        const double* p = cj + (size_t)f * NJ * 3;
        double ac[3];                                        // (r_hip - l_hip) + (sdr_r - sdr_l) with r_hip = 1, l_hip = 2
#pragma unroll
        for (int k = 0; k < 3; ++k) {
            if (F32) ac[k] = (double)add(sub((float)p[1 * 3 + k], (float)p[2 * 3 + k]), sub((float)p[17 * 3 + k], (float)p[16 * 3 + k]));
            else ac[k] = (p[1 * 3 + k] - p[2 * 3 + k]) + (p[17 * 3 + k] - p[16 * 3 + k]);
        }
        if (F32) {
            const float an = __fsqrt_rn((float)sq3(ac[0], ac[1], ac[2]));
#pragma unroll
            for (int k = 0; k < 3; ++k) ac[k] = (double)__fdiv_rn((float)ac[k], an);
        } else {
            const double an = sqrt(dsq3(ac[0], ac[1], ac[2]));
#pragma unroll
            for (int k = 0; k < 3; ++k) ac[k] /= an;
        }
        const double fw[3] = {-ac[1], ac[0], 0.0};          // (0,0,1) x across
        const double fn = sqrt(dsq3(fw[0], fw[1], fw[2]));
        const float v0[3] = {(float)(fw[0] / fn), (float)(fw[1] / fn), (float)(fw[2] / fn)};
        float q[4];
        qbetween_y_rn(v0, q);
        if (isnan(q[0]) || isnan(q[1]) || isnan(q[2]) || isnan(q[3])) atomicMin(first_nan, f);
#pragma unroll
        for (int k = 0; k < 4; ++k) sQ[f * 4 + k] = q[k];
    }
    __syncthreads();
    if (tid == 0) {                                          // only the FIRST NaN frame is patched; then frame 0 = identity
        const int k = *first_nan;
        if (k < L) {
            const int src = (k == 0) ? L - 1 : k - 1;
            for (int i = 0; i < 4; ++i) sQ[k * 4 + i] = sQ[src * 4 + i];
        }
        sQ[0] = 1.f; sQ[1] = 0.f; sQ[2] = 0.f; sQ[3] = 0.f;
    }
    __syncthreads();

    // ---- phase 2: the 294 channels of frames 0 .. L-2, one (frame, joint) pair per thread ---------------------------------
    auto put = [&](float* row, int ch, double v) {
        row[ch] = (float)(mean ? (v - (double)mean[ch]) / (double)stdv[ch] : v);
    };
    for (int i = tid; i < (L - 1) * NJ; i += blockDim.x) {
        const int t = i / NJ, j = i - t * NJ;
        float* row = o_repr + (size_t)t * C_TOTAL;
        const double* p = cj + (size_t)t * NJ * 3;
        const double* pn = p + NJ * 3;
        const float* q = sQ + t * 4;
        const float* qn = q + 4;
        const float lp[3] = {(float)dif(p[j * 3], p[0]), (float)dif(p[j * 3 + 1], p[1]), (float)p[j * 3 + 2]};
        const float dv[3] = {(float)dif(pn[j * 3], p[j * 3]), (float)dif(pn[j * 3 + 1], p[j * 3 + 1]), (float)dif(pn[j * 3 + 2], p[j * 3 + 2])};
        float r[3];
        qrot_rn(q, lp, r);
#pragma unroll
        for (int k = 0; k < 3; ++k) put(row, CH_LOCAL + j * 3 + k, r[k]);
        qrot_rn(q, dv, r);
#pragma unroll
        for (int k = 0; k < 3; ++k) put(row, CH_LOCAL_VEL + j * 3 + k, r[k]);
        const double* w = W + (size_t)t * kWorldCols;
        if (j > 0) {
            double M[9];
            rotvec_to_matrix_f64(w + 16 + (j - 1) * 3, M);
            const int o = CH_POSE6D + (j - 1) * 6;
            put(row, o, M[0]); put(row, o + 1, M[1]); put(row, o + 2, M[3]); put(row, o + 3, M[4]); put(row, o + 4, M[6]);
            put(row, o + 5, M[7]);
            continue;
        }
        put(row, 0, (double)atan2f(q[3], q[0]));                                   // root_rot_angle
        float vw, vz;
        qmul_inv_wz_rn(qn, q, vw, vz);
        put(row, 1, (double)atan2f(vz, vw));                                       // root_rot_angle_vel
        put(row, 2, p[0]); put(row, 3, p[1]);                                      // root_l_pos
        qrot_rn(qn, dv, r);                                                        // rotated by the NEXT frame's q
        put(row, 4, r[0]); put(row, 5, r[1]);                                      // root_l_vel
        put(row, 6, p[2]);                                                         // root_height
        const double* R = sR + (size_t)t * 9;
        const double* Rn = R + 9;
        put(row, 7, R[0]); put(row, 8, R[1]); put(row, 9, R[3]); put(row, 10, R[4]); put(row, 11, R[6]); put(row, 12, R[7]);
        double dR[9], Wm[9];
#pragma unroll
        for (int k = 0; k < 9; ++k) dR[k] = Rn[k] - R[k];
#pragma unroll
        for (int x = 0; x < 3; ++x)
#pragma unroll
            for (int y = 0; y < 3; ++y) Wm[x * 3 + y] = dR[x * 3] * R[y * 3] + dR[x * 3 + 1] * R[y * 3 + 1] + dR[x * 3 + 2] * R[y * 3 + 2];
        put(row, 13, (-Wm[5] + Wm[7]) / 2.0); put(row, 14, (Wm[2] - Wm[6]) / 2.0); put(row, 15, (-Wm[1] + Wm[3]) / 2.0);
#pragma unroll
        for (int k = 0; k < 3; ++k) { put(row, 16 + k, sT[t * 3 + k]); put(row, 19 + k, sT[(t + 1) * 3 + k] - sT[t * 3 + k]); }
#pragma unroll
        for (int k = 0; k < NBETA; ++k) put(row, CH_BETAS + k, w[6 + k]);
        // foot contact (foot_detect, :23-44, up_axis 'z'): slow AND low, columns left 7, 10 then right 8, 11
        const int fj[4] = {7, 10, 8, 11};
        const double hthr[4] = {0.18, 0.15, 0.18, 0.15};
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            const double* u = p + fj[k] * 3;
            const double* un = pn + fj[k] * 3;
            const double sq = sq3(dif(un[0], u[0]), dif(un[1], u[1]), dif(un[2], u[2]));
            put(row, CH_CONTACT + k, (sq < 5e-5 && u[2] < hthr[k]) ? 1.0 : 0.0);
        }
    }
}

__global__ __launch_bounds__(kClipThreads) void clips_build_kernel(const ClipArgs a) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem_raw[];
    const int L = a.L, c = blockIdx.x, tid = threadIdx.x, up = a.up;
    double* cj = a.scratch ? a.scratch + (size_t)c * L * NJ * 3 : reinterpret_cast<double*>(smem_raw);
    unsigned char* aux = smem_raw + (a.scratch ? 0 : (size_t)L * kFrameLds);
    double* sR = reinterpret_cast<double*>(aux);
    double* sT = sR + (size_t)L * 9;
    float* sQ = reinterpret_cast<float*>(sT + (size_t)L * 3);
    float* sMin = sQ + (size_t)L * 4;                       // [8]
    int* first_nan = reinterpret_cast<int*>(sMin + 8);

    const long long s0 = a.starts ? (long long)a.starts[c] : (long long)c * a.step;
    float* o_repr = a.repr + (size_t)c * (L - 1) * C_TOTAL;
    float* o_cj = a.cano_joints + (size_t)c * L * NJ * 3;
    float* o_go = a.cano_orient + (size_t)c * L * 3;
    float* o_tr = a.cano_transl + (size_t)c * L * 3;
    float* o_tm = a.transf + (size_t)c * 16;
    if (s0 < 0 || s0 + L > a.N) {                           // a window outside the recording: NaN, never an out-of-bounds read
        const float nanv = __builtin_nanf("");
        for (int i = tid; i < (L - 1) * C_TOTAL; i += blockDim.x) o_repr[i] = nanv;
        for (int i = tid; i < L * NJ * 3; i += blockDim.x) o_cj[i] = nanv;
        for (int i = tid; i < L * 3; i += blockDim.x) { o_go[i] = nanv; o_tr[i] = nanv; }
        if (tid < 16) o_tm[tid] = nanv;
        if (a.orient_transl64)
            for (int i = tid; i < L * 6; i += blockDim.x) a.orient_transl64[(size_t)c * L * 6 + i] = __builtin_nan("");
        return;
    }
    const float* J = a.joints + (size_t)s0 * NJ * 3;
    const double* W = a.world + (size_t)s0 * kWorldCols;

    // ---- floor: min of the up coordinate over the clip (float32), or the preset ------------------------------------
    if (tid == 0) *first_nan = L;
    const bool preset = a.has_preset && a.preset != 0.0;
    float floor32;
    double floor64;
    if (preset) {
        floor32 = (float)a.preset;
        floor64 = a.preset;
        __syncthreads();
    } else {
        float m = INFINITY;
        for (int i = tid; i < L * NJ; i += blockDim.x) m = fminf(m, J[(size_t)i * 3 + up]);
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) m = fminf(m, __shfl_xor(m, o));
        if ((tid & 63) == 0) sMin[tid >> 6] = m;
        __syncthreads();
        m = sMin[0];
        for (int w = 1; w < (int)(blockDim.x >> 6); ++w) m = fminf(m, sMin[w]);
        floor32 = m;
        floor64 = (double)m;
    }

    // ---- canonical frame from frame 0 (every thread computes it: 5 joints) ------------------------------------------
    double root[3], rot[9], tvec[3];
    {
        auto ld = [&](int j, double* p) {
#pragma unroll
            for (int k = 0; k < 3; ++k) p[k] = (double)(k == up ? sub(J[j * 3 + k], floor32) : J[j * 3 + k]);
        };
        double p0[3], p1[3], p2[3], p16[3], p17[3];
        ld(0, p0); ld(1, p1); ld(2, p2); ld(16, p16); ld(17, p17);
#pragma unroll
        for (int k = 0; k < 3; ++k) root[k] = (k == up) ? 0.0 : p0[k];
        double x[3];
#pragma unroll
        for (int k = 0; k < 3; ++k) x[k] = ((p2[k] - root[k]) - (p1[k] - root[k])) + ((p17[k] - root[k]) - (p16[k] - root[k]));
        x[up] = 0.0;
        const double xn = sqrt(dsq3(x[0], x[1], x[2]));
#pragma unroll
        for (int k = 0; k < 3; ++k) x[k] /= xn;
        double Q[9];                                         // transf_rotmat^T
        if (up == 2) {
            double y[3] = {-x[1], x[0], 0.0};               // z_axis x x_axis
            const double yn = sqrt(dsq3(y[0], y[1], y[2]));
            Q[0] = x[0]; Q[1] = x[1]; Q[2] = x[2];
            Q[3] = y[0] / yn; Q[4] = y[1] / yn; Q[5] = y[2] / yn;
            Q[6] = 0.0; Q[7] = 0.0; Q[8] = 1.0;
        } else {
            double y[3] = {x[2], 0.0, -x[0]};               // (0,1,0) x x_axis
            const double yn = sqrt(dsq3(y[0], y[1], y[2]));
            Q[0] = -x[0]; Q[1] = -x[1]; Q[2] = -x[2];
            Q[3] = -0.0; Q[4] = -1.0; Q[5] = -0.0;
            Q[6] = -(y[0] / yn); Q[7] = -(y[1] / yn); Q[8] = -(y[2] / yn);
        }
#pragma unroll
        for (int i = 0; i < 3; ++i)
#pragma unroll
            for (int j = 0; j < 3; ++j) rot[i * 3 + j] = a.A[i * 3] * Q[j] + a.A[i * 3 + 1] * Q[3 + j] + a.A[i * 3 + 2] * Q[6 + j];
        double m1[3];
#pragma unroll
        for (int k = 0; k < 3; ++k) m1[k] = (k == up) ? -floor64 : -root[k];
        mat3_vec(rot, m1, tvec);
        if (tid < 16) {
            const int i = tid >> 2, j = tid & 3;
            o_tm[tid] = (float)(i == 3 ? (j == 3 ? 1.0 : 0.0) : (j == 3 ? tvec[i] : rot[i * 3 + j]));
        }
    }

    // ---- phase 1: canonical joints (float64, kept for phase 2) and canonical parameters --------------------------------
    for (int i = tid; i < L * NJ; i += blockDim.x) {
        double p[3], q[3];
#pragma unroll
        for (int k = 0; k < 3; ++k) {
            const float v = J[(size_t)i * 3 + k];
            p[k] = (double)(k == up ? sub(v, floor32) : v) - root[k];
        }
        mat3_vec(rot, p, q);
#pragma unroll
        for (int k = 0; k < 3; ++k) { cj[(size_t)i * 3 + k] = q[k]; o_cj[(size_t)i * 3 + k] = (float)q[k]; }
    }
    for (int f = tid; f < L; f += blockDim.x) {
        const double* w = W + (size_t)f * kWorldCols;
        const double go[3] = {w[0], w[1], w[2]};
        double dT[3], tp[3], Rb[9], Rn[9], rvn[3], tn[3];
#pragma unroll
        for (int k = 0; k < 3; ++k) { dT[k] = (double)J[(size_t)f * NJ * 3 + k] - w[3 + k]; tp[k] = w[3 + k] + dT[k]; }
        rotvec_to_matrix_f64(go, Rb);
#pragma unroll
        for (int i = 0; i < 3; ++i)
#pragma unroll
            for (int j = 0; j < 3; ++j) Rn[i * 3 + j] = rot[i * 3] * Rb[j] + rot[i * 3 + 1] * Rb[3 + j] + rot[i * 3 + 2] * Rb[6 + j];
        matrix_to_rotvec_f64(Rn, rvn);
        mat3_vec(rot, tp, tn);
        rotvec_to_matrix_f64(rvn, sR + (size_t)f * 9);      // get_repr_smplx starts again from the rotation vector
#pragma unroll
        for (int k = 0; k < 3; ++k) {
            const double t = (tn[k] + tvec[k]) - dT[k];
            sT[f * 3 + k] = t;
            o_go[f * 3 + k] = (float)rvn[k];
            o_tr[f * 3 + k] = (float)t;
            if (a.orient_transl64) {
                double* o64 = a.orient_transl64 + ((size_t)c * L + f) * 6;
                o64[k] = rvn[k];
                o64[3 + k] = t;
            }
        }
    }
    __syncthreads();

    repr_from_canonical<false>(cj, sR, sT, sQ, first_nan, W, L, a.mean, a.stdv, o_repr);
}

// get_repr_smplx on joints that are canonical already (the noisy clips of dataloader_amass.py:213-215 and the sep_noise
// items of :298-309): positions [C,L,22,3] float32 or float64, params [C,L,79] float64 (global_orient, transl, betas,
// body_pose).  With joint_noise [C,L,22,3] (float64) the joints become float32(positions + noise) first (:305-307).
struct ReprArgs {
    const float* pos32;
    const double* pos64;
    const double* params;
    const double* joint_noise;
    int L;
    const float* mean;
    const float* stdv;
    float* repr;              // [C,L-1,294]
    float* joints_out;        // [C,L,22,3] the joints the representation was computed from, or null
    double* scratch;
};

template <bool F32>
__global__ __launch_bounds__(kClipThreads) void clips_repr_kernel(const ReprArgs a) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem_raw[];
    const int L = a.L, c = blockIdx.x, tid = threadIdx.x;
    double* cj = a.scratch ? a.scratch + (size_t)c * L * NJ * 3 : reinterpret_cast<double*>(smem_raw);
    unsigned char* aux = smem_raw + (a.scratch ? 0 : (size_t)L * kFrameLds);
    double* sR = reinterpret_cast<double*>(aux);
    double* sT = sR + (size_t)L * 9;
    float* sQ = reinterpret_cast<float*>(sT + (size_t)L * 3);
    int* first_nan = reinterpret_cast<int*>(sQ + (size_t)L * 4 + 8);
    const size_t base = (size_t)c * L * NJ * 3;
    const double* W = a.params + (size_t)c * L * kWorldCols;
    if (tid == 0) *first_nan = L;
    for (int i = tid; i < L * NJ * 3; i += blockDim.x) {
        double v = a.pos64 ? a.pos64[base + i] : (double)a.pos32[base + i];
        if (a.joint_noise) v = (double)(float)(v + a.joint_noise[base + i]);
        cj[i] = v;
        if (a.joints_out) a.joints_out[base + i] = (float)v;
    }
    for (int f = tid; f < L; f += blockDim.x) {
        const double* w = W + (size_t)f * kWorldCols;
        rotvec_to_matrix_f64(w, sR + (size_t)f * 9);
#pragma unroll
        for (int k = 0; k < 3; ++k) sT[f * 3 + k] = w[3 + k];
    }
    __syncthreads();
    repr_from_canonical<F32>(cj, sR, sT, sQ, first_nan, W, L, a.mean, a.stdv, a.repr + (size_t)c * (L - 1) * C_TOTAL);
}

// dataloader_video.py:441-458: flip x, cv2.undistortPoints(src, K, dist, P = K) (five fixed-point iterations of the inverse of
// the k1 k2 p1 p2 k3 model), flip x back; the confidence passes through.  float64 arithmetic, float32 store.
struct UndistortArgs { double K[9]; double k[5]; double width; };

__global__ __launch_bounds__(256) void keypoints_undistort_kernel(const float* __restrict__ kp, float* __restrict__ out, long long M,
                                                                  const UndistortArgs u) {
    const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= M) return;
    const double fx = u.K[0], fy = u.K[4], cx = u.K[2], cy = u.K[5];
    const double k1 = u.k[0], k2 = u.k[1], p1 = u.k[2], p2 = u.k[3], k3 = u.k[4];
    const double px = u.width - 1.0 - (double)kp[i * 3], py = (double)kp[i * 3 + 1];
    const double x0 = (px - cx) / fx, y0 = (py - cy) / fy;
    double x = x0, y = y0;
#pragma unroll 1
    for (int it = 0; it < 5; ++it) {
        const double r2 = x * x + y * y;
        const double icd = 1.0 / (1.0 + ((k3 * r2 + k2) * r2 + k1) * r2);
        const double dx = 2.0 * p1 * x * y + p2 * (r2 + 2.0 * x * x);
        const double dy = p1 * (r2 + 2.0 * y * y) + 2.0 * p2 * x * y;
        x = (x0 - dx) * icd;
        y = (y0 - dy) * icd;
    }
    const double xx = u.K[0] * x + u.K[1] * y + u.K[2], yy = u.K[3] * x + u.K[4] * y + u.K[5];
    const double ww = 1.0 / (u.K[6] * x + u.K[7] * y + u.K[8]);
    out[i * 3] = (float)(u.width - 1.0 - xx * ww);
    out[i * 3 + 1] = (float)(yy * ww);
    out[i * 3 + 2] = kp[i * 3 + 2];
}

// dataloader_video.py:462-484, windows read in place.  One thread per (clip, frame, channel).
__global__ __launch_bounds__(256) void visibility_masks_kernel(const float* __restrict__ kp, const float* __restrict__ mask_joint,
                                                               int mask_cols, const int* __restrict__ starts, int step, int N,
                                                               int C, int L, float* __restrict__ joint_vis,
                                                               float* __restrict__ vec_vis) {
    const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= (long long)C * L * C_TOTAL) return;
    const int ch = (int)(i % C_TOTAL);
    const long long cf = i / C_TOTAL;
    const int f = (int)(cf % L), c = (int)(cf / L);
    const long long n = (starts ? (long long)starts[c] : (long long)c * step) + f;
    const bool inside = n >= 0 && n < N;
    auto vis = [&](int j) -> float {
        if (!inside) return __builtin_nanf("");
        return ((double)kp[(n * NJ + j) * 3 + 2] > 0.2) ? mask_joint[n * mask_cols + j] : 0.f;
    };
    if (ch < NJ) joint_vis[cf * NJ + ch] = vis(ch);
    float v;
    if (ch < CH_LOCAL) v = 1.f;
    else if (ch < CH_LOCAL_VEL) v = vis((ch - CH_LOCAL) / 3);
    else if (ch < CH_POSE6D) v = vis((ch - CH_LOCAL_VEL) / 3);
    else if (ch < CH_BETAS) v = vis(1 + (ch - CH_POSE6D) / 6);
    else if (ch < CH_CONTACT) v = 1.f;
    else {
        const int k = ch - CH_CONTACT;                       // 0, 1: left foot (7 & 10); 2, 3: right foot (8 & 11)
        v = (vis(k < 2 ? 7 : 8) == 1.f && vis(k < 2 ? 10 : 11) == 1.f) ? 1.f : 0.f;
    }
    vec_vis[i] = v;
}

static size_t clip_lds_bytes(int L, bool joints_in_lds) {
    return (size_t)L * (kFrameAux + (joints_in_lds ? kFrameLds : 0)) + kFixedLds;
}

}  // namespace rohm

using namespace rohm;

extern "C" size_t rohm_clips_scratch_bytes(int C, int L) {
    if (C <= 0 || L < 2) return 0;
    return clip_lds_bytes(L, true) <= (size_t)kLdsMax ? 0 : (size_t)C * L * NJ * 3 * sizeof(double);
}

extern "C" int rohm_clips_build_f64(const float* joints_world, const double* smplx_world, int N, const int* starts, int C,
                                    int clip_len, int overlap, int up_axis, int has_preset_floor, double preset_floor,
                                    const float* mean294, const float* std294, float* repr, float* cano_joints,
                                    float* cano_orient, float* cano_transl, float* transf, double* orient_transl64,
                                    void* scratch, size_t scratch_bytes, rohm_stream_t stream) {
    ROHM_ARG_CHECK(clip_len >= 2 && clip_len <= 800, "clips_build: need 2 <= clip_len <= 800 (got %d)", clip_len);
    ROHM_ARG_CHECK(C >= 0 && N >= 0, "clips_build: negative size (C=%d N=%d)", C, N);
    ROHM_ARG_CHECK(up_axis == 1 || up_axis == 2, "clips_build: up_axis must be 1 (y) or 2 (z)");
    ROHM_ARG_CHECK((mean294 == nullptr) == (std294 == nullptr), "clips_build: pass both mean and std or neither");
    if (C == 0) return ROHM_OK;
    ROHM_ARG_CHECK(joints_world && smplx_world && repr && cano_joints && cano_orient && cano_transl && transf,
                   "clips_build: null argument");
    const int step = clip_len - overlap;
    if (!starts)
        ROHM_ARG_CHECK(overlap >= 0 && overlap < clip_len && (long long)(C - 1) * step + clip_len <= N,
                       "clips_build: %d clips of %d frames with overlap %d do not fit into %d frames", C, clip_len, overlap, N);
    const size_t need = rohm_clips_scratch_bytes(C, clip_len);
    ROHM_ARG_CHECK(need == 0 || (scratch && scratch_bytes >= need), "clips_build: scratch too small (%zu < %zu)", scratch_bytes, need);
    ClipArgs a;
    a.joints = joints_world; a.world = smplx_world; a.starts = starts; a.step = step; a.N = N; a.L = clip_len; a.up = up_axis;
    a.has_preset = has_preset_floor; a.preset = preset_floor;
    for (int i = 0; i < 9; ++i) a.A[i] = (i % 4 == 0) ? 1.0 : 0.0;
    if (up_axis == 1) {     // trans_rot_z(pi) . trans_rot_x(-pi/2) with the reference's own libm values (:157-164)
        const double cx = cos(-M_PI / 2), sx = sin(-M_PI / 2), cz = cos(M_PI), sz = sin(M_PI);
        const double rx[9] = {1, 0, 0, 0, cx, -sx, 0, sx, cx}, rz[9] = {cz, -sz, 0, sz, cz, 0, 0, 0, 1};
        for (int i = 0; i < 3; ++i)
            for (int j = 0; j < 3; ++j) a.A[i * 3 + j] = rz[i * 3] * rx[j] + rz[i * 3 + 1] * rx[3 + j] + rz[i * 3 + 2] * rx[6 + j];
    }
    a.mean = mean294; a.stdv = std294; a.repr = repr; a.cano_joints = cano_joints; a.cano_orient = cano_orient;
    a.cano_transl = cano_transl; a.transf = transf; a.orient_transl64 = orient_transl64;
    a.scratch = need ? static_cast<double*>(scratch) : nullptr;
    const size_t lds = clip_lds_bytes(clip_len, need == 0);
    static int lds_set = 0;
    if ((int)lds > lds_set) {
        ROHM_HIP_CHECK(hipFuncSetAttribute(reinterpret_cast<const void*>(&clips_build_kernel),
                                           hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
        lds_set = (int)lds;
    }
    prof::Scope ps("clips_build", 0.0, (double)C * clip_len * (4.0 * 66 * 2 + 8.0 * kWorldCols + 4.0 * C_TOTAL), (hipStream_t)stream);
    hipLaunchKernelGGL(clips_build_kernel, dim3(C), dim3(kClipThreads), lds, (hipStream_t)stream, a);
    ROHM_LAUNCH_CHECK();
    return ROHM_OK;
}

extern "C" int rohm_clips_build(const float* joints_world, const double* smplx_world, int N, const int* starts, int C,
                                int clip_len, int overlap, int up_axis, int has_preset_floor, double preset_floor,
                                const float* mean294, const float* std294, float* repr, float* cano_joints,
                                float* cano_orient, float* cano_transl, float* transf, void* scratch, size_t scratch_bytes,
                                rohm_stream_t stream) {
    return rohm_clips_build_f64(joints_world, smplx_world, N, starts, C, clip_len, overlap, up_axis, has_preset_floor,
                                preset_floor, mean294, std294, repr, cano_joints, cano_orient, cano_transl, transf, nullptr,
                                scratch, scratch_bytes, stream);
}

extern "C" int rohm_clips_repr(const void* positions, int positions_f64, const double* params, const double* joint_noise, int C,
                               int clip_len, const float* mean294, const float* std294, float* repr, float* joints_out,
                               void* scratch, size_t scratch_bytes, rohm_stream_t stream) {
    ROHM_ARG_CHECK(clip_len >= 2 && clip_len <= 800, "clips_repr: need 2 <= clip_len <= 800 (got %d)", clip_len);
    ROHM_ARG_CHECK(C >= 0, "clips_repr: negative size (C=%d)", C);
    ROHM_ARG_CHECK((mean294 == nullptr) == (std294 == nullptr), "clips_repr: pass both mean and std or neither");
    if (C == 0) return ROHM_OK;
    ROHM_ARG_CHECK(positions && params && repr, "clips_repr: null argument");
    const size_t need = rohm_clips_scratch_bytes(C, clip_len);
    ROHM_ARG_CHECK(need == 0 || (scratch && scratch_bytes >= need), "clips_repr: scratch too small (%zu < %zu)", scratch_bytes, need);
    ReprArgs a;
    a.pos32 = positions_f64 ? nullptr : static_cast<const float*>(positions);
    a.pos64 = positions_f64 ? static_cast<const double*>(positions) : nullptr;
    a.params = params; a.joint_noise = joint_noise; a.L = clip_len; a.mean = mean294; a.stdv = std294; a.repr = repr;
    a.joints_out = joints_out; a.scratch = need ? static_cast<double*>(scratch) : nullptr;
    const bool f32 = !positions_f64 || joint_noise;            // the dtype get_repr_smplx sees
    const size_t lds = clip_lds_bytes(clip_len, need == 0);
    static int lds_set[2] = {0, 0};
    if ((int)lds > lds_set[f32]) {
        const void* fn = f32 ? reinterpret_cast<const void*>(&clips_repr_kernel<true>)
                             : reinterpret_cast<const void*>(&clips_repr_kernel<false>);
        ROHM_HIP_CHECK(hipFuncSetAttribute(fn, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
        lds_set[f32] = (int)lds;
    }
    prof::Scope ps("clips_repr", 0.0, (double)C * clip_len * (8.0 * 66 + 8.0 * kWorldCols + 4.0 * C_TOTAL), (hipStream_t)stream);
    if (f32) hipLaunchKernelGGL(clips_repr_kernel<true>, dim3(C), dim3(kClipThreads), lds, (hipStream_t)stream, a);
    else hipLaunchKernelGGL(clips_repr_kernel<false>, dim3(C), dim3(kClipThreads), lds, (hipStream_t)stream, a);
    ROHM_LAUNCH_CHECK();
    return ROHM_OK;
}

extern "C" int rohm_keypoints_undistort(const float* keypoints, long long M, const double* camera_mtx9, const double* dist5,
                                        double image_width, float* out, rohm_stream_t stream) {
    ROHM_ARG_CHECK(M >= 0, "keypoints_undistort: negative count");
    if (M == 0) return ROHM_OK;
    ROHM_ARG_CHECK(keypoints && camera_mtx9 && dist5 && out, "keypoints_undistort: null argument");
    ROHM_ARG_CHECK(camera_mtx9[0] != 0.0 && camera_mtx9[4] != 0.0, "keypoints_undistort: zero focal length");
    UndistortArgs u;
    for (int i = 0; i < 9; ++i) u.K[i] = camera_mtx9[i];
    for (int i = 0; i < 5; ++i) u.k[i] = dist5[i];
    u.width = image_width;
    prof::Scope ps("keypoints_undistort", 0.0, 24.0 * M, (hipStream_t)stream);
    hipLaunchKernelGGL(keypoints_undistort_kernel, dim3((unsigned)((M + 255) / 256)), dim3(256), 0, (hipStream_t)stream, keypoints,
                       out, M, u);
    ROHM_LAUNCH_CHECK();
    return ROHM_OK;
}

extern "C" int rohm_visibility_masks(const float* keypoints, const float* mask_joint, int mask_cols, int N, const int* starts,
                                     int C, int clip_len, int overlap, float* mask_joint_vis, float* mask_vec_vis,
                                     rohm_stream_t stream) {
    ROHM_ARG_CHECK(clip_len >= 1 && C >= 0 && N >= 0, "visibility_masks: bad sizes (C=%d L=%d N=%d)", C, clip_len, N);
    ROHM_ARG_CHECK(mask_cols >= NJ, "visibility_masks: mask_joint needs at least 22 columns (got %d)", mask_cols);
    if (C == 0) return ROHM_OK;
    ROHM_ARG_CHECK(keypoints && mask_joint && mask_joint_vis && mask_vec_vis, "visibility_masks: null argument");
    const int step = clip_len - overlap;
    if (!starts)
        ROHM_ARG_CHECK(overlap >= 0 && overlap < clip_len && (long long)(C - 1) * step + clip_len <= N,
                       "visibility_masks: %d clips of %d frames with overlap %d do not fit into %d frames", C, clip_len, overlap, N);
    const long long total = (long long)C * clip_len * C_TOTAL;
    prof::Scope ps("visibility_masks", 0.0, 4.0 * total, (hipStream_t)stream);
    hipLaunchKernelGGL(visibility_masks_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, (hipStream_t)stream, keypoints,
                       mask_joint, mask_cols, starts, step, N, C, clip_len, mask_joint_vis, mask_vec_vis);
    ROHM_LAUNCH_CHECK();
    return ROHM_OK;
}
