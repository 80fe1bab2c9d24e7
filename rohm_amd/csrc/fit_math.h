// The float64 pieces that the Levenberg-Marquardt kernels of fit.hip (SMPL-X from 3-D joints) and fit_views.hip (SMPL-X from 2-D
// keypoints) share: Rodrigues and the right Jacobian of SO(3), the logarithm, the kinematic chain, the Jacobian of the 66 joint
// coordinates against the 66 rotation unknowns, and the damped Cholesky solve.  The float32 helpers of smplx_fk.h cannot serve a
// float64 solver; these are their float64 siblings (the same Rodrigues convention, the same chain).  Private to csrc.
//
// The two templates take the kernel's LDS struct S.  fit_jacobian needs G, M, P [NJ x 9 / 9 / 3], anc [NJ] and W [66 x 66];
// fit_solve needs H (packed lower triangle), W (at least kFitTri values), g, dg, rhs, sol [69].
#pragma once
#include "smplx_fk.h"

namespace rohm {

constexpr int kFitThreads = 256;
constexpr int kFitRot = 66;                          // rotation unknowns (22 joints x 3)
constexpr int kFitX = 69;                            // unknowns: rotations, then the translation
constexpr int kFitTri = kFitX * (kFitX + 1) / 2;     // packed lower triangle of H
constexpr int kFitTries = 8;
constexpr double kFitLambda0 = 1e-3, kFitLambdaMin = 1e-9, kFitLambdaMax = 1e8, kFitDiagEps = 1e-9, kFitDegenerate = 1e-9;

__device__ __forceinline__ int tri(int i, int j) { return i * (i + 1) / 2 + j; }   // i >= j

__device__ __forceinline__ void mat_mul64(const double* a, const double* b, double* c) {
#pragma unroll
    for (int i = 0; i < 3; ++i)
#pragma unroll
        for (int j = 0; j < 3; ++j) c[i * 3 + j] = a[i * 3] * b[j] + a[i * 3 + 1] * b[3 + j] + a[i * 3 + 2] * b[6 + j];
}

// rodrigues of smplx_fk.h in float64: angle = |r + 1e-8|, axis = r / angle, R = I + sin K + (1 - cos) K^2
__device__ __forceinline__ void rodrigues64(const double* r, double* R) {
    const double ex = r[0] + 1e-8, ey = r[1] + 1e-8, ez = r[2] + 1e-8;
    const double ang = sqrt(ex * ex + ey * ey + ez * ez);
    const double x = r[0] / ang, y = r[1] / ang, z = r[2] / ang;
    const double s = sin(ang), c1 = 1.0 - cos(ang);
    const double K[9] = {0.0, -z, y, z, 0.0, -x, -y, x, 0.0};
    double K2[9];
    mat_mul64(K, K, K2);
#pragma unroll
    for (int i = 0; i < 9; ++i) R[i] = ((i % 4 == 0) ? 1.0 : 0.0) + s * K[i] + c1 * K2[i];
}

// the right Jacobian of SO(3): I - (1 - cos a) / a^2 K + (a - sin a) / a^3 K^2, K = [r]x, a = |r|; its series below 1e-6
__device__ __forceinline__ void right_jacobian64(const double* r, double* Jr) {
    const double a2 = r[0] * r[0] + r[1] * r[1] + r[2] * r[2];
    const double a = sqrt(a2);
    double p, q;
    if (a < 1e-6) {
        p = 0.5 - a2 / 24.0;
        q = 1.0 / 6.0 - a2 / 120.0;
    } else {
        p = (1.0 - cos(a)) / a2;
        q = (a - sin(a)) / (a2 * a);
    }
    const double K[9] = {0.0, -r[2], r[1], r[2], 0.0, -r[0], -r[1], r[0], 0.0};
    double K2[9];
    mat_mul64(K, K, K2);
#pragma unroll
    for (int i = 0; i < 9; ++i) Jr[i] = ((i % 4 == 0) ? 1.0 : 0.0) - p * K[i] + q * K2[i];
}

// rotation matrix -> axis-angle.  c = (tr R - 1) / 2, v = (R21 - R12, R02 - R20, R10 - R01), s = |v| / 2, angle = atan2(s, c).
// s >= 1e-6 and c > -0.99: v / (2 s) angle.  Else c > 0: v / 2.  Else (near a half turn) the axis comes from B = (R + R^T) / 2:
// i = the largest B_ii (the first on ties), n_i = sqrt(max((B_ii - c) / (1 - c), 0)), n_j = B_ij / ((1 - c) n_i), normalised,
// signed to agree with v.
__device__ __forceinline__ void log_map64(const double* R, double* aa) {
    const double c = (R[0] + R[4] + R[8] - 1.0) * 0.5;
    const double v[3] = {R[7] - R[5], R[2] - R[6], R[3] - R[1]};
    const double s = 0.5 * sqrt(v[0] * v[0] + v[1] * v[1] + v[2] * v[2]);
    const double ang = atan2(s, c);
    if (s >= 1e-6 && c > -0.99) {
        const double f = ang / (2.0 * s);
        aa[0] = v[0] * f; aa[1] = v[1] * f; aa[2] = v[2] * f;
    } else if (c > 0.0) {
        aa[0] = 0.5 * v[0]; aa[1] = 0.5 * v[1]; aa[2] = 0.5 * v[2];
    } else {
        int i = 0;
        if (R[4] > R[i * 4]) i = 1;
        if (R[8] > R[i * 4]) i = 2;
        double n[3];
        n[i] = sqrt(fmax((R[i * 4] - c) / (1.0 - c), 0.0));
        for (int j = 0; j < 3; ++j)
            if (j != i) n[j] = 0.5 * (R[i * 3 + j] + R[j * 3 + i]) / ((1.0 - c) * n[i]);
        const double len = sqrt(n[0] * n[0] + n[1] * n[1] + n[2] * n[2]);
        const double sign = (v[0] * n[0] + v[1] * n[1] + v[2] * n[2]) < 0.0 ? -1.0 : 1.0;
        for (int j = 0; j < 3; ++j) aa[j] = sign * n[j] / len * ang;
    }
}

// fk_forward of smplx_fk.h in float64 on LDS arrays: G[0] = R[0], P[0] = rest[0], G[j] = G[p] R[j], P[j] = P[p] + G[p] (rest[j] - rest[p])
__device__ __forceinline__ void chain64(const double* R, const double* rest, const int* parents, double* G, double* P) {
    for (int i = 0; i < 9; ++i) G[i] = R[i];
    if (P)
        for (int c = 0; c < 3; ++c) P[c] = rest[c];
    for (int j = 1; j < NJ; ++j) {
        const int p = parents[j];
        mat_mul64(G + p * 9, R + j * 9, G + j * 9);
        if (P) {
            const double off[3] = {rest[j * 3] - rest[p * 3], rest[j * 3 + 1] - rest[p * 3 + 1], rest[j * 3 + 2] - rest[p * 3 + 2]};
            for (int c = 0; c < 3; ++c)
                P[j * 3 + c] = P[p * 3 + c] + (G[p * 9 + c * 3] * off[0] + G[p * 9 + c * 3 + 1] * off[1] + G[p * 9 + c * 3 + 2] * off[2]);
        }
    }
}

// The Jacobian of the 66 joint coordinates against the 66 rotation unknowns into s.W [66 rows][66 columns], from G, P and the J_r that
// an evaluation left in M (turned into G J_r here).  Ends with a barrier.
template <class S>
__device__ __forceinline__ void fit_jacobian(S& s, int tid) {
    if (tid < NJ) {                                  // M = G J_r
        double m[9];
        mat_mul64(s.G + tid * 9, s.M + tid * 9, m);
        for (int i = 0; i < 9; ++i) s.M[tid * 9 + i] = m[i];
    }
    __syncthreads();
    for (int e = tid; e < NJ * NJ; e += kFitThreads) {       // block (j, k): -[p_j - p_k]x M_k for k a strict ancestor of j, else 0
        const int j = e / NJ, k = e % NJ;
        const bool on = (s.anc[j] >> k) & 1u;
        const double d[3] = {s.P[j * 3] - s.P[k * 3], s.P[j * 3 + 1] - s.P[k * 3 + 1], s.P[j * 3 + 2] - s.P[k * 3 + 2]};
#pragma unroll
        for (int b = 0; b < 3; ++b) {
            const double m0 = s.M[k * 9 + b], m1 = s.M[k * 9 + 3 + b], m2 = s.M[k * 9 + 6 + b];
            s.W[(j * 3) * kFitRot + k * 3 + b] = on ? m1 * d[2] - m2 * d[1] : 0.0;
            s.W[(j * 3 + 1) * kFitRot + k * 3 + b] = on ? m2 * d[0] - m0 * d[2] : 0.0;
            s.W[(j * 3 + 2) * kFitRot + k * 3 + b] = on ? m0 * d[1] - m1 * d[0] : 0.0;
        }
    }
    __syncthreads();
}

// (H + lambda diag(diag(H) + 1e-9)) sol = -g by Cholesky over W.  false on a pivot that is not positive.
template <class S>
__device__ __forceinline__ bool fit_solve(S& s, double lambda, int tid) {
    double* L = s.W;
    __syncthreads();                                 // a try that ended on a bad pivot left without one: nobody still reads L
    for (int e = tid; e < kFitTri; e += kFitThreads) L[e] = s.H[e];
    if (tid < kFitX) s.rhs[tid] = -s.g[tid];
    __syncthreads();
    if (tid < kFitX) L[tri(tid, tid)] += lambda * (s.H[tri(tid, tid)] + kFitDiagEps);
    __syncthreads();
    const int ti = tid / 16, tj = tid % 16;
    for (int k = 0; k < kFitX; ++k) {
        const double piv = L[tri(k, k)];             // final since the barrier that closed step k - 1; not written in step k
        if (!(piv > 0.0)) return false;              // the same value in every thread
        const double d = sqrt(piv);
        for (int i = k + 1 + tid; i < kFitX; i += kFitThreads) L[tri(i, k)] /= d;
        if (tid == 0) s.dg[k] = d;
        __syncthreads();
        for (int i = k + 1 + ti; i < kFitX; i += 16) {
            const double lik = L[tri(i, k)];
            for (int j = k + 1 + tj; j <= i; j += 16) L[tri(i, j)] -= lik * L[tri(j, k)];
        }
        __syncthreads();
    }
    for (int k = 0; k < kFitX; ++k) {                // L z = rhs; z ends in rhs
        const double z = s.rhs[k] / s.dg[k];
        for (int i = k + 1 + tid; i < kFitX; i += kFitThreads) s.rhs[i] -= L[tri(i, k)] * z;
        if (tid == 0) s.sol[k] = z;
        __syncthreads();
    }
    for (int k = kFitX - 1; k >= 0; --k) {           // L^T d = z; z is in sol, d ends in rhs
        const double d = s.sol[k] / s.dg[k];
        for (int i = tid; i < k; i += kFitThreads) s.sol[i] -= L[tri(k, i)] * d;
        if (tid == 0) s.rhs[k] = d;
        __syncthreads();
    }
    return true;
}

}  // namespace rohm
