// The float64 pieces of the Levenberg-Marquardt kernels of fit.hip (SMPL-X from 3-D joints) and fit_views.hip (SMPL-X from 2-D
// keypoints).  Both use: Rodrigues, the right Jacobian of SO(3), the logarithm and the kinematic chain (the siblings of smplx_fk.h's
// float32 helpers: the same Rodrigues convention, the same chain), the Jacobian of the 66 joint coordinates against the 66
// rotation unknowns, the damped Cholesky solve, the `normal` dump and the "not fitted" exit.  The rest is the solver as
// fit_views.hip runs it, everything but a data term: the LDS it keeps (FitCore), the prologue pieces, the prior and smoothing
// part of the energy and of the gradient, the walk over the packed triangle of H and the iteration itself (fit_lm).  fit.hip
// still writes those out for itself (its header says why); a solver to come takes them from here.  Private to csrc.
//
// The templates take the kernel's LDS struct S (fit_jacobian, fit_solve, fit_dump_normal: any struct with the members they name;
// the others: one that extends FitCore).  A kernel hands fit_lm a "problem" p: p.evaluate<kJac>(x) is the energy at x, the same
// value in every thread, behind a barrier (kJac also leaves J_r in M and whatever the next two need); p.hessian(i, j) and
// p.gradient(i) are the data term's share of H and g at s.x.
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

// What a solver keeps in LDS whatever its data term; FitViewsShared (fit_views.hip) extends it with its data term's members.
struct FitCore {
    double H[kFitTri];            // packed lower triangle
    double W[kFitRot * kFitRot];  // the Jacobian [66 rows][66 columns]; then the packed Cholesky factor (strictly lower part)
    double g[kFitX], dg[kFitX], rhs[kFitX], sol[kFitX];
    double x[kFitX], xt[kFitX];
    double R[NJ * 9], G[NJ * 9], M[NJ * 9];          // local and world rotations; M = G J_r
    double P[NJ * 3], rest[NJ * 3];
    double mean[kFitX], wdiag[kFitX], wsm[kFitX], wp[NJ];    // (the translation's three entries carry the smoothing only)
    double E;
    int parents[NJ];
    unsigned anc[NJ];             // bit k: joint k is a strict ancestor
    int status;
};

// prologue, all lanes: parents and prior weights on 22 lanes, the rest joints Jt + Js betas on 66.  The caller's barrier follows.
template <class S>
__device__ __forceinline__ void fit_load_body(S& s, const float* __restrict__ Jt, const float* __restrict__ Js, const int* __restrict__ parents,
                                              const float* __restrict__ betas, const double* __restrict__ w_prior, int tid) {
    if (tid < NJ) {
        s.parents[tid] = parents[tid];
        s.wp[tid] = w_prior[tid];
    }
    if (tid < kFitRot) {
        double v = (double)Jt[tid];
        for (int k = 0; k < NBETA; ++k) v += (double)Js[tid * NBETA + k] * (double)betas[k];
        s.rest[tid] = v;
    }
}

// prologue, lane 0, behind fit_load_body's barrier: the ancestor masks and the smoothing set-up.  Smoothing: the mean of prev over
// the neighbours of frame f that exist and are finite; the body pose and the translation (weight w_smooth_t), never
// the root.  wdiag is what the prior and the smoothing add to H's diagonal.
template <class S>
__device__ __forceinline__ void fit_lane0_setup(S& s, const double* __restrict__ prev, size_t f, int N, double w_smooth, double w_smooth_t) {
    s.anc[0] = 0u;
    for (int j = 1; j < NJ; ++j) s.anc[j] = s.anc[s.parents[j]] | (1u << s.parents[j]);
    int cnt = 0;
    bool use[2] = {false, false};
    if (prev) {
        for (int q = 0; q < 2; ++q) {
            const long long g = (long long)f + (q == 0 ? -1 : 1);
            if (g < 0 || g >= N) continue;
            bool fin = true;
            for (int i = 0; i < kFitX; ++i) fin = fin && isfinite(prev[(size_t)g * kFitX + i]);
            use[q] = fin;
            cnt += fin ? 1 : 0;
        }
    }
    for (int i = 0; i < kFitX; ++i) {
        const bool on = i >= 3 && cnt > 0;
        double m = 0.0;
        if (on) {
            if (use[0]) m += prev[(f - 1) * kFitX + i];
            if (use[1]) m += prev[(f + 1) * kFitX + i];
            m /= (double)cnt;
        }
        s.mean[i] = m;
        s.wsm[i] = on ? (i < kFitRot ? w_smooth : w_smooth_t) : 0.0;
        s.wdiag[i] = (i < kFitRot ? s.wp[i / 3] : 0.0) + s.wsm[i];
    }
}

// R of all joints on 22 lanes; kJac also leaves J_r in M (turned into G J_r by fit_jacobian).  Ends with a barrier.
template <bool kJac, class S>
__device__ __forceinline__ void fit_rotations(S& s, const double* x, int tid) {
    if (tid < NJ) {
        rodrigues64(x + tid * 3, s.R + tid * 9);
        if (kJac) right_jacobian64(x + tid * 3, s.M + tid * 9);
    }
    __syncthreads();
}

// lane 0: the data term's energy e plus the prior and the smoothing at x
template <class S>
__device__ __forceinline__ double fit_prior_energy(const S& s, const double* x, double e) {
    for (int k = 0; k < NJ; ++k) {
        double q = 0.0, m = 0.0;
        for (int c = 0; c < 3; ++c) {
            const double th = x[k * 3 + c], d = th - s.mean[k * 3 + c];
            q += th * th;
            m += s.wsm[k * 3 + c] * (d * d);
        }
        e += s.wp[k] * q + m;
    }
    double m = 0.0;
    for (int c = 0; c < 3; ++c) {
        const double d = x[kFitRot + c] - s.mean[kFitRot + c];
        m += s.wsm[kFitRot + c] * (d * d);
    }
    return e + m;
}

// entry i of g at s.x: the data term's v plus the prior and the smoothing
template <class S>
__device__ __forceinline__ double fit_prior_gradient(const S& s, int i, double v) {
    if (i < kFitRot) return v + s.wp[i / 3] * s.x[i] + s.wsm[i] * (s.x[i] - s.mean[i]);
    return v + s.wsm[i] * (s.x[i] - s.mean[i]);
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

// H (packed) and g at s.x from the state p.evaluate<true> left: p.hessian(i, j) is the data term's share of H_ij (i >= j),
// p.gradient(i) its share of g_i.  Ends with a barrier.
template <class S, class Problem>
__device__ __forceinline__ void fit_normal(S& s, const Problem& p, int tid) {
    fit_jacobian(s, tid);
    int i = 0, base = 0;                             // this thread's first packed index is tid: walk (i, j) along with it
    for (int e = tid; e < kFitTri; e += kFitThreads) {
        while (base + i + 1 <= e) { base += i + 1; ++i; }
        const int j = e - base;
        double v = p.hessian(i, j);
        if (i == j) v += s.wdiag[i];
        s.H[e] = v;
    }
    if (tid < kFitX) s.g[tid] = fit_prior_gradient(s, tid, p.gradient(tid));
    __syncthreads();
}

// H and g as the rows of normal[69][70]
template <class S>
__device__ __forceinline__ void fit_dump_normal(const S& s, double* __restrict__ normal, int tid) {
    for (int e = tid; e < kFitX * (kFitX + 1); e += kFitThreads) {
        const int i = e / (kFitX + 1), j = e % (kFitX + 1);
        normal[e] = j == kFitX ? s.g[i] : s.H[i >= j ? tri(i, j) : tri(j, i)];
    }
}

// A frame that is not fitted: zeros, the status and NaN in the six report columns both kernels have.  The caller adds its own
// columns and returns: the whole block leaves.
__device__ __forceinline__ void fit_unfitted(int status, double* __restrict__ params, double* __restrict__ report, double* __restrict__ normal,
                                             int tid) {
    const double nan = __longlong_as_double(0x7ff8000000000000ll);
    for (int i = tid; i < kFitX; i += kFitThreads) params[i] = 0.0;
    if (normal)
        for (int i = tid; i < kFitX * (kFitX + 1); i += kFitThreads) normal[i] = 0.0;
    if (tid == 0) {
        report[0] = (double)status; report[1] = nan; report[2] = nan; report[3] = 0.0; report[4] = nan; report[5] = nan;
    }
}

struct FitLm { double E0, E, lambda; int accepted; };     // the energy at the start and at the answer, the last damping, the accepted tries

// Levenberg-Marquardt from s.x, where E = p.evaluate<true>(s.x) has just been taken: up to `iters` iterations of up to eight tries,
// lambda / 10 (not below 1e-9) after an accepted try and * 10 (not above 1e8) after a rejected one.  `normal`, if asked for, is H and g
// at the start.  The answer is in s.x; the state of the last evaluation is that of the last try, not of s.x.
template <class S, class Problem>
__device__ __forceinline__ FitLm fit_lm(S& s, const Problem& p, double E, int iters, double* __restrict__ normal, int tid) {
    const double E0 = E;
    double lambda = kFitLambda0;
    int accepted = 0;
    bool fresh = false;                              // H and g belong to the current x
    if (normal || iters > 0) {
        fit_normal(s, p, tid);
        fresh = true;
    }
    if (normal) fit_dump_normal(s, normal, tid);
    for (int it = 0; it < iters; ++it) {
        if (!fresh) {
            E = p.template evaluate<true>(s.x);
            fit_normal(s, p, tid);
            fresh = true;
        }
        for (int tr = 0; tr < kFitTries; ++tr) {
            bool ok = fit_solve(s, lambda, tid);
            if (ok) {
                if (tid < kFitX) s.xt[tid] = s.x[tid] + s.rhs[tid];
                __syncthreads();
                const double Et = p.template evaluate<false>(s.xt);
                ok = Et < E;                         // an infinite (or NaN) energy is a rejected try
                if (ok) {
                    if (tid < kFitX) s.x[tid] = s.xt[tid];
                    E = Et;
                    __syncthreads();
                }
            }
            if (ok) {
                lambda = fmax(lambda / 10.0, kFitLambdaMin);
                ++accepted;
                fresh = false;
                break;
            }
            lambda = fmin(lambda * 10.0, kFitLambdaMax);
        }
    }
    return {E0, E, lambda, accepted};
}

}  // namespace rohm
