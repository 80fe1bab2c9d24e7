// Vector-Jacobian product of the repr -> joints recovery (rohm_repr_joints, rederive.hip): given d_joints [B,T,22,3]
// (dL/djoints), write dL/drepr for all 294 channels of every frame (zero on the channels the recovery does not read).
// This is what makes the joint terms of PoseNet.compute_losses_with_smpl (model/posenet.py:98-194) differentiable with
// respect to the network output.
//
// mode 0 'smplx_params': joints = FK(rot6d -> R, betas) + transl.  The reference's R -> axis-angle -> Rodrigues round
//   trip is the identity on SO(3), so the gradient is taken through the Gram-Schmidt matrices directly, as the forward
//   does: fk_backward<true> (incl. the global orientation) + rot6d_bwd + the betas' rest-joint regressor.
// mode 1 'joint_abs_traj': j >= 1 = Rz(2a) v_j + (x, y, 0), joint 0 = (x, y, h).
// mode 2 'joint_rel_traj': as mode 1 with a_t = sum_{s<t} angvel_s and (x, y)_t = sum_{s<=t} Rz(2a_s) v_{s-1}; the
//   VJP runs the two running sums backwards over the frames (one workgroup per clip, thread 0 scans).
//
// Every output element is written by exactly one thread and every sum has a fixed order: no atomics, so the result is
// bitwise reproducible.  With mean/std the forward de-normalises repr * std + mean, so the VJP scales by std.
#include "common.h"
#include "smplx_fk.h"

namespace rohm {

namespace {

constexpr int CH_ANG_VEL = 1, CH_L_VEL = 4;   // root_rot_angle_vel, root_l_vel (motion_representation.py:312-329)

struct Grad294 {
    float* o;
    long long sc;
    const float* stdv;
    __device__ __forceinline__ void put(int c, float v) const { o[(size_t)c * sc] = stdv ? v * stdv[c] : v; }
};

// Rz(2a) v for the (x, y) part, the rotation abs_joint applies: returns (r0, r1) with o = r + pos.
__device__ __forceinline__ void rot_xy(float ang, float v0, float v1, float& r0, float& r1) {
    float o[3];
    const float v[3] = {v0, v1, 0.f}, zero[3] = {0.f, 0.f, 0.f};
    abs_joint(ang, zero, v, o);
    r0 = o[0];
    r1 = o[1];
}

// Per-frame part shared by modes 1 and 2: the local joints' gradient (written), and the frame's direct dL/dangle and
// dL/d(x, y) (returned).  d(Rz(2a) v)/da = 2 (r1, -r0).
__device__ __forceinline__ void traj_frame(const float* x, long long isc, const float* mean, const float* stdv,
                                           const float* g, float ang, const Grad294& out, float& gang, float& gx,
                                           float& gy) {
    auto ldc = [&](int c) {
        const float v = x[(size_t)c * isc];
        return mean ? __fadd_rn(__fmul_rn(v, stdv[c]), mean[c]) : v;   // as the forward, no fma
    };
    gang = 0.f;
    gx = g[0];
    gy = g[1];
    for (int j = 1; j < NJ; ++j) {
        const float* gj = g + j * 3;
        const float v[3] = {ldc(CH_LOCAL + 3 * j), ldc(CH_LOCAL + 3 * j + 1), ldc(CH_LOCAL + 3 * j + 2)};
        float r0, r1, dv[3];
        rot_xy(ang, v[0], v[1], r0, r1);
        gang += 2.f * (gj[0] * r1 - gj[1] * r0);
        gx += gj[0];
        gy += gj[1];
        abs_joint_T(ang, gj, dv);
#pragma unroll
        for (int c = 0; c < 3; ++c) out.put(CH_LOCAL + 3 * j + c, dv[c]);
    }
    out.put(CH_ROOT_H, g[2]);
}

__global__ __launch_bounds__(64) void repr_joints_vjp_kernel(const float* __restrict__ repr, long long isb,
                                                             long long ist, long long isc, const float* __restrict__ mean,
                                                             const float* __restrict__ stdv, const float* __restrict__ Jt,
                                                             const float* __restrict__ Js, const int* __restrict__ parents,
                                                             const float* __restrict__ dj, float* __restrict__ drepr,
                                                             long long osb, long long ost, long long osc, int mode, int B,
                                                             int T) {
    const int idx = blockIdx.x * blockDim.x + threadIdx.x;
    if (idx >= B * T) return;
    const int b = idx / T, t = idx % T;
    const float* x = repr + (size_t)b * isb + (size_t)t * ist;
    const float* g = dj + (size_t)idx * NJ * 3;
    const Grad294 out{drepr + (size_t)b * osb + (size_t)t * ost, osc, mean ? stdv : nullptr};
    auto ldc = [&](int c) {
        const float v = x[(size_t)c * isc];
        return mean ? __fadd_rn(__fmul_rn(v, stdv[c]), mean[c]) : v;   // as the forward, no fma
    };
    for (int c = 0; c < C_TOTAL; ++c) out.o[(size_t)c * osc] = 0.f;
    if (mode == 0) {
        FrameIn in;
#pragma unroll
        for (int k = 0; k < 6; ++k) in.x6[0][k] = ldc(CH_ROT6D + k);
        for (int j = 1; j < NJ; ++j)
#pragma unroll
            for (int k = 0; k < 6; ++k) in.x6[j][k] = ldc(CH_POSE6D + (j - 1) * 6 + k);
#pragma unroll
        for (int k = 0; k < NBETA; ++k) in.beta[k] = ldc(CH_BETAS + k);
        FkCtx f;
        smplx_fk(in, Jt, Js, parents, f);
        float gP[NJ][3], dR[NJ][9], dJr[NJ][3], dtr[3] = {0.f, 0.f, 0.f};
        for (int j = 0; j < NJ; ++j)
#pragma unroll
            for (int c = 0; c < 3; ++c) {
                gP[j][c] = g[j * 3 + c];
                dtr[c] += gP[j][c];
            }
        fk_backward<true>(f, parents, gP, dR, dJr);
        for (int j = 0; j < NJ; ++j) {
            float dx[6];
            rot6d_bwd(in.x6[j], dR[j], dx);
            const int c0 = j == 0 ? CH_ROT6D : CH_POSE6D + (j - 1) * 6;
#pragma unroll
            for (int k = 0; k < 6; ++k) out.put(c0 + k, dx[k]);
        }
#pragma unroll
        for (int k = 0; k < NBETA; ++k) {      // Jr[j][c] = Jt + sum_k Js[j,c,k] beta_k
            float s = 0.f;
            for (int j = 0; j < NJ; ++j)
#pragma unroll
                for (int c = 0; c < 3; ++c) s = fmaf(Js[(j * 3 + c) * NBETA + k], dJr[j][c], s);
            out.put(CH_BETAS + k, s);
        }
#pragma unroll
        for (int c = 0; c < 3; ++c) out.put(CH_TRANS + c, dtr[c]);
    } else {
        float gang, gx, gy;
        traj_frame(x, isc, mean, stdv, g, ldc(CH_ROOT_ANG), out, gang, gx, gy);
        out.put(CH_ROOT_ANG, gang);
        out.put(CH_ROOT_POS, gx);
        out.put(CH_ROOT_POS + 1, gy);
    }
}

// mode 2.  LDS per frame: [0] angle a_t, [1..3] direct dL/da_t, dL/dx_t, dL/dy_t; [4..6] the scanned gradients of
// frame t's angvel and (vx, vy) channels.
__global__ __launch_bounds__(256) void repr_joints_rel_vjp_kernel(const float* __restrict__ repr, long long isb,
                                                                  long long ist, long long isc,
                                                                  const float* __restrict__ mean,
                                                                  const float* __restrict__ stdv,
                                                                  const float* __restrict__ dj, float* __restrict__ drepr,
                                                                  long long osb, long long ost, long long osc, int T) {
    extern __shared__ __attribute__((aligned(16))) float sf[];     // [T][8]
    const int b = blockIdx.x;
    const float* xb = repr + (size_t)b * isb;
    auto ldc = [&](int t, int c) {
        const float v = xb[(size_t)t * ist + (size_t)c * isc];
        return mean ? __fadd_rn(__fmul_rn(v, stdv[c]), mean[c]) : v;   // as the forward, no fma
    };
    if (threadIdx.x == 0) {    // the forward's angle scan, same order (repr_joints_rel_kernel)
        float ang = 0.f;
        for (int t = 0; t < T; ++t) {
            if (t > 0) ang = __fadd_rn(ang, ldc(t - 1, CH_ANG_VEL));
            sf[t * 8] = ang;
        }
    }
    __syncthreads();
    for (int t = threadIdx.x; t < T; t += blockDim.x) {
        float* o = drepr + (size_t)b * osb + (size_t)t * ost;
        for (int c = 0; c < C_TOTAL; ++c) o[(size_t)c * osc] = 0.f;
        const Grad294 out{o, osc, mean ? stdv : nullptr};
        float gang, gx, gy;
        traj_frame(xb + (size_t)t * ist, isc, mean, stdv, dj + ((size_t)b * T + t) * NJ * 3, sf[t * 8], out, gang, gx, gy);
        sf[t * 8 + 1] = gang; sf[t * 8 + 2] = gx; sf[t * 8 + 3] = gy;
        sf[t * 8 + 4] = 0.f; sf[t * 8 + 5] = 0.f; sf[t * 8 + 6] = 0.f;
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        // (x, y)_t = sum_{s<=t} r_s, r_s = Rz(2 a_s) v_{s-1} (r_0 = 0): dL/dr_s = Gx, Gy = sum_{t>=s} dL/d(x, y)_t.
        // a_t = sum_{s<t} angvel_s: dL/dangvel_{t-1} = sum_{t'>=t} dL/da_t' (incl. the a_t' in r_t').
        float Gx = 0.f, Gy = 0.f, Ga = 0.f;
        for (int t = T - 1; t >= 1; --t) {
            const float a = sf[t * 8];
            Gx += sf[t * 8 + 2];
            Gy += sf[t * 8 + 3];
            float r0, r1;
            rot_xy(a, ldc(t - 1, CH_L_VEL), ldc(t - 1, CH_L_VEL + 1), r0, r1);
            Ga += sf[t * 8 + 1] + 2.f * (Gx * r1 - Gy * r0);
            const float G[3] = {Gx, Gy, 0.f};
            float dv[3];
            abs_joint_T(a, G, dv);
            sf[(t - 1) * 8 + 4] = Ga;
            sf[(t - 1) * 8 + 5] = dv[0];
            sf[(t - 1) * 8 + 6] = dv[1];
        }
    }
    __syncthreads();
    for (int t = threadIdx.x; t < T; t += blockDim.x) {
        const Grad294 out{drepr + (size_t)b * osb + (size_t)t * ost, osc, mean ? stdv : nullptr};
        out.put(CH_ANG_VEL, sf[t * 8 + 4]);
        out.put(CH_L_VEL, sf[t * 8 + 5]);
        out.put(CH_L_VEL + 1, sf[t * 8 + 6]);
    }
}

}  // namespace

}  // namespace rohm

using namespace rohm;

extern "C" int rohm_repr_joints_vjp(const rohm_smplx_t* h, const float* repr, long long in_stride_b,
                                    long long in_stride_t, long long in_stride_c, const float* mean294,
                                    const float* std294, int B, int T, int mode, const float* d_joints, float* d_repr,
                                    long long out_stride_b, long long out_stride_t, long long out_stride_c,
                                    rohm_stream_t stream) {
    ROHM_ARG_CHECK(repr && d_joints && d_repr, "repr_joints_vjp: null argument");
    ROHM_ARG_CHECK(mode != 0 || h, "repr_joints_vjp: mode 0 ('smplx_params') needs a body-model handle");
    ROHM_ARG_CHECK(mode >= 0 && mode <= 2, "repr_joints_vjp: mode must be 0 (smplx_params), 1 (joint_abs_traj) or 2 (joint_rel_traj)");
    ROHM_ARG_CHECK((mean294 == nullptr) == (std294 == nullptr), "repr_joints_vjp: pass both mean and std or neither");
    if (B <= 0 || T <= 0) return ROHM_OK;
    const int n = B * T;
    prof::Scope ps("repr_joints_vjp", 0.0, 4.0 * n * (155 + 66 + 2 * C_TOTAL), (hipStream_t)stream);
    if (mode == 2) {
        ROHM_ARG_CHECK(T <= 2048, "repr_joints_vjp: 'joint_rel_traj' supports T <= 2048");
        hipLaunchKernelGGL(repr_joints_rel_vjp_kernel, dim3(B), dim3(256), (size_t)T * 8 * sizeof(float),
                           (hipStream_t)stream, repr, in_stride_b, in_stride_t, in_stride_c, mean294, std294, d_joints,
                           d_repr, out_stride_b, out_stride_t, out_stride_c, T);
        ROHM_LAUNCH_CHECK();
        return ROHM_OK;
    }
    hipLaunchKernelGGL(repr_joints_vjp_kernel, dim3((n + 63) / 64), dim3(64), 0, (hipStream_t)stream, repr, in_stride_b,
                       in_stride_t, in_stride_c, mean294, std294, h ? h->d_Jt : nullptr, h ? h->d_Js : nullptr,
                       h ? h->d_parents : nullptr, d_joints, d_repr, out_stride_b, out_stride_t, out_stride_c, mode, B, T);
    ROHM_LAUNCH_CHECK();
    return ROHM_OK;
}
