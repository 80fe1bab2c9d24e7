// SMPL-X from 3-D joints: per-frame pose by Levenberg-Marquardt (rohm_fit_pose) and the sums one shared shape needs
// (rohm_fit_shape_moments).  rohm_amd/fit.py drives them; tests/fit_ref.py restates both in numpy; include/rohm_hip.h states
// the rules in full.  There is no counterpart in the reference: its recordings come with fitted parameters.
//
// All arithmetic is float64 on the float32 inputs, as in floor.hip.  No atomics, every sum is taken by one thread in a fixed
// order or by a fixed butterfly: the same input gives the same bits.  The float64 helpers, the Jacobian, the Cholesky solve, the
// `normal` dump and the unfitted exit are fit_math.h's, shared with fit_views.hip.  The prologue, the smoothing set-up and the
// Levenberg-Marquardt loop are written out here although fit_math.h has them for fit_views.hip (fit_lm and its pieces): with
// 256 registers and spills this kernel is at the edge, and every way of taking them from there moved it off its instruction
// stream and cost 0.7 to 2.6 % (profiles/fit_core_resources.md).  A rule changed there is changed here too.
//
// rohm_fit_pose: one workgroup of 256 threads per frame.  In LDS, as float64: the normal matrix H as a packed lower triangle
// (2415 values, 19 KiB), the Jacobian of the 66 joint coordinates against the 66 rotation unknowns (34 KiB; the translation's
// columns are the identity and are never stored) and 11 KiB of per-joint state: 64.9 KiB, so two workgroups share a CU's
// 160 KiB (and the kernel is held to the 256 registers that lets them, see fit_pose_kernel).  The Jacobian is dead once H and g are built, so the Cholesky factor of H + lambda diag(H) (packed again) is
// written over it; H itself survives the tries of one iteration.  Rodrigues and the right Jacobian of the 22 joints go to
// 22 lanes, the kinematic chain is serial on lane 0 (21 small products), and the lanes go to J^T C J (2415 dot products of 66
// terms per iteration) and to the factorisation (69 steps, two barriers each; the triangular solves take one barrier per
// step).
#include "fit_math.h"
#include "reduce.h"

#include <limits.h>

namespace rohm {

constexpr int kFitMomThreads = 128;
constexpr int kFitMom = 66;                          // 55 + 10 + 1
constexpr int kFitTotThreads = 256;

// the torso triad of the issue: columns x^ = norm(v1 - v2), u^ = norm of the part of v12 - (v1 + v2) / 2 orthogonal to x^,
// z^ = x^ x u^.  F is row-major with those columns.  false when a norm is below 1e-9 (or not a number).
__device__ __forceinline__ bool triad64(const double* v1, const double* v2, const double* v12, double* F) {
    double x[3], u[3];
    for (int c = 0; c < 3; ++c) x[c] = v1[c] - v2[c];
    const double nx = sqrt(x[0] * x[0] + x[1] * x[1] + x[2] * x[2]);
    if (!(nx >= kFitDegenerate)) return false;
    for (int c = 0; c < 3; ++c) x[c] /= nx;
    for (int c = 0; c < 3; ++c) u[c] = v12[c] - 0.5 * (v1[c] + v2[c]);
    const double d = u[0] * x[0] + u[1] * x[1] + u[2] * x[2];
    for (int c = 0; c < 3; ++c) u[c] -= d * x[c];
    const double nu = sqrt(u[0] * u[0] + u[1] * u[1] + u[2] * u[2]);
    if (!(nu >= kFitDegenerate)) return false;
    for (int c = 0; c < 3; ++c) u[c] /= nu;
    const double z[3] = {x[1] * u[2] - x[2] * u[1], x[2] * u[0] - x[0] * u[2], x[0] * u[1] - x[1] * u[0]};
    for (int c = 0; c < 3; ++c) { F[c * 3] = x[c]; F[c * 3 + 1] = u[c]; F[c * 3 + 2] = z[c]; }
    return true;
}

// c_j and y_j of a frame: a non-finite target or confidence, or a confidence <= 0, gives c = 0 (and y = 0, so that it is never a NaN)
__device__ __forceinline__ void load_observation(const float* __restrict__ targets, const float* __restrict__ conf, size_t frame, int j,
                                                 double* c, double* y) {
    const float* t = targets + (frame * NJ + j) * 3;
    const double y0 = (double)t[0], y1 = (double)t[1], y2 = (double)t[2];
    const double cj = conf ? (double)conf[frame * NJ + j] : 1.0;
    const bool ok = isfinite(y0) && isfinite(y1) && isfinite(y2) && isfinite(cj) && cj > 0.0;
    c[j] = ok ? cj : 0.0;
    y[j * 3] = ok ? y0 : 0.0; y[j * 3 + 1] = ok ? y1 : 0.0; y[j * 3 + 2] = ok ? y2 : 0.0;
}

struct FitPoseArgs {
    const float* Jt;              // [J,3]
    const float* Js;              // [J,3,10]
    const int* parents;           // [J]
    const float* targets;         // [N,22,3]
    const float* conf;            // [N,22] or null
    const float* betas;           // [N,10]
    const double* init;           // [N,69] or null
    const double* prev;           // [N,69] or null
    const double* w_prior;        // [22]
    double w_smooth;
    int iters, min_joints, N;
    double* params;               // [N,69]
    double* report;               // [N,6]
    double* normal;               // [N,69,70] or null
};

struct FitShared {
    double H[kFitTri];            // packed lower triangle
    double W[kFitRot * kFitRot];  // the Jacobian [66 rows][66 columns]; then the packed Cholesky factor (strictly lower part)
    double g[kFitX], dg[kFitX], rhs[kFitX], sol[kFitX];
    double x[kFitX], xt[kFitX];
    double R[NJ * 9], G[NJ * 9], M[NJ * 9];          // local and world rotations; M = G J_r
    double P[NJ * 3], rest[NJ * 3], y[NJ * 3], res[NJ * 3], c[NJ];
    double mean[kFitRot], wdiag[kFitRot], wsm[kFitRot], wp[NJ];
    double E;
    int parents[NJ];
    unsigned anc[NJ];             // bit k: joint k is a strict ancestor
    int status;
};

// R (and M's first factor) of all joints on 22 lanes, the chain and the energy on lane 0; every thread returns E.
// res = P + t - y afterwards.  kJac also leaves J_r in M (turned into G J_r by the caller).
template <bool kJac>
__device__ __forceinline__ double fit_evaluate(FitShared& s, const double* x, int tid) {
    if (tid < NJ) {
        rodrigues64(x + tid * 3, s.R + tid * 9);
        if (kJac) right_jacobian64(x + tid * 3, s.M + tid * 9);
    }
    __syncthreads();
    if (tid == 0) {
        chain64(s.R, s.rest, s.parents, s.G, s.P);
        double e = 0.0;
        for (int j = 0; j < NJ; ++j) {
            double q = 0.0;
            for (int c = 0; c < 3; ++c) {
                const double r = s.P[j * 3 + c] + x[kFitRot + c] - s.y[j * 3 + c];
                s.res[j * 3 + c] = r;
                q += r * r;
            }
            e += s.c[j] * q;
        }
        for (int k = 0; k < NJ; ++k) {
            double q = 0.0, m = 0.0;
            for (int c = 0; c < 3; ++c) {
                const double th = x[k * 3 + c], d = th - s.mean[k * 3 + c];
                q += th * th;
                m += s.wsm[k * 3 + c] * (d * d);
            }
            e += s.wp[k] * q + m;
        }
        s.E = e;
    }
    __syncthreads();
    return s.E;
}

// H (packed) and g at s.x from the state fit_evaluate<true> left
__device__ __forceinline__ void fit_normal(FitShared& s, int tid) {
    fit_jacobian(s, tid);
    int i = 0, base = 0;                            // this thread's first packed index is tid: walk (i, j) along with it
    for (int e = tid; e < kFitTri; e += kFitThreads) {
        while (base + i + 1 <= e) { base += i + 1; ++i; }
        const int j = e - base;
        double v = 0.0;
        if (i < kFitRot) {
            for (int r = 0; r < kFitRot; ++r) v += s.c[r / 3] * (s.W[r * kFitRot + i] * s.W[r * kFitRot + j]);
            if (i == j) v += s.wdiag[i];
        } else if (j < kFitRot) {
            const int a = i - kFitRot;
            for (int q = 0; q < NJ; ++q) v += s.c[q] * s.W[(q * 3 + a) * kFitRot + j];
        } else if (i == j) {
            for (int q = 0; q < NJ; ++q) v += s.c[q];
        }
        s.H[e] = v;
    }
    if (tid < kFitRot) {
        double v = 0.0;
        for (int r = 0; r < kFitRot; ++r) v += s.c[r / 3] * (s.res[r] * s.W[r * kFitRot + tid]);
        s.g[tid] = v + s.wp[tid / 3] * s.x[tid] + s.wsm[tid] * (s.x[tid] - s.mean[tid]);
    } else if (tid < kFitX) {
        const int a = tid - kFitRot;
        double v = 0.0;
        for (int q = 0; q < NJ; ++q) v += s.c[q] * s.res[q * 3 + a];
        s.g[tid] = v;
    }
    __syncthreads();
}

// Two waves per SIMD: without the attribute the compiler takes 262 registers and one workgroup has a CU to itself; held to 256 it
// spills 25 of them (40 B of scratch per lane, in the serial start-up code) and two workgroups share the CU: 58 ms instead of 108 ms
// for 3 000 frames of 20 iterations (profiles/fit_bench.json).
__global__ __launch_bounds__(kFitThreads) __attribute__((amdgpu_waves_per_eu(2))) void fit_pose_kernel(const FitPoseArgs a) {
    __shared__ FitShared s;
    const int tid = threadIdx.x;
    const size_t f = blockIdx.x;
    double* params = a.params + f * kFitX;
    double* report = a.report + f * 6;
    double* normal = a.normal ? a.normal + f * kFitX * (kFitX + 1) : nullptr;

    if (tid < NJ) {
        load_observation(a.targets, a.conf, f, tid, s.c, s.y);
        s.parents[tid] = a.parents[tid];
        s.wp[tid] = a.w_prior[tid];
    }
    if (tid < kFitRot) {
        double v = (double)a.Jt[tid];
        for (int k = 0; k < NBETA; ++k) v += (double)a.Js[tid * NBETA + k] * (double)a.betas[f * NBETA + k];
        s.rest[tid] = v;
    }
    __syncthreads();
    if (tid == 0) {
        s.anc[0] = 0u;
        for (int j = 1; j < NJ; ++j) s.anc[j] = s.anc[s.parents[j]] | (1u << s.parents[j]);
        int seen = 0;
        for (int j = 0; j < NJ; ++j) seen += s.c[j] > 0.0 ? 1 : 0;
        bool from_init = a.init != nullptr;
        if (from_init)
            for (int i = 0; i < kFitX; ++i) from_init = from_init && isfinite(a.init[f * kFitX + i]);
        int status = 1;
        if (seen < a.min_joints) {
            status = 0;
        } else if (from_init) {
            for (int i = 0; i < kFitX; ++i) s.x[i] = a.init[f * kFitX + i];
        } else {
            double Fy[9], Fr[9];
            const bool ok = s.c[1] > 0.0 && s.c[2] > 0.0 && s.c[12] > 0.0 && triad64(s.y + 3, s.y + 6, s.y + 36, Fy) &&
                            triad64(s.rest + 3, s.rest + 6, s.rest + 36, Fr);
            if (!ok) {
                status = 2;
            } else {
                double R0[9];
                for (int i = 0; i < 3; ++i)
                    for (int j = 0; j < 3; ++j) R0[i * 3 + j] = Fy[i * 3] * Fr[j * 3] + Fy[i * 3 + 1] * Fr[j * 3 + 1] + Fy[i * 3 + 2] * Fr[j * 3 + 2];
                for (int i = 0; i < kFitX; ++i) s.x[i] = 0.0;
                log_map64(R0, s.x);
            }
        }
        s.status = status;
        // smoothing: the mean of prev over the neighbours that exist and are finite; body pose only
        int cnt = 0;
        bool use[2] = {false, false};
        if (a.prev) {
            for (int q = 0; q < 2; ++q) {
                const long long g = (long long)f + (q == 0 ? -1 : 1);
                if (g < 0 || g >= a.N) continue;
                bool fin = true;
                for (int i = 0; i < kFitX; ++i) fin = fin && isfinite(a.prev[(size_t)g * kFitX + i]);
                use[q] = fin;
                cnt += fin ? 1 : 0;
            }
        }
        for (int i = 0; i < kFitRot; ++i) {
            double m = 0.0;
            if (i >= 3 && cnt > 0) {
                if (use[0]) m += a.prev[(f - 1) * kFitX + i];
                if (use[1]) m += a.prev[(f + 1) * kFitX + i];
                m /= (double)cnt;
            }
            s.mean[i] = m;
            s.wsm[i] = (i >= 3 && cnt > 0) ? a.w_smooth : 0.0;
            s.wdiag[i] = s.wp[i / 3] + s.wsm[i];
        }
    }
    __syncthreads();
    const int status = s.status;
    if (status != 1) {                               // skipped, or needs a start: zeros and NaN energies; the whole block leaves
        fit_unfitted(status, params, report, normal, tid);
        return;
    }
    bool from_init = a.init != nullptr;              // (uniform: every thread reads the same row)
    if (from_init)
        for (int i = 0; i < kFitX; ++i) from_init = from_init && isfinite(a.init[f * kFitX + i]);
    if (!from_init) {                                // t = sum c (y - p) / sum c at the triad's rotation
        fit_evaluate<false>(s, s.x, tid);            // x's translation is 0 here: res = p - y
        if (tid == 0) {
            double sc = 0.0, t[3] = {0.0, 0.0, 0.0};
            for (int j = 0; j < NJ; ++j) {
                sc += s.c[j];
                for (int c = 0; c < 3; ++c) t[c] -= s.c[j] * s.res[j * 3 + c];
            }
            for (int c = 0; c < 3; ++c) s.x[kFitRot + c] = t[c] / sc;
        }
        __syncthreads();
    }

    double E = fit_evaluate<true>(s, s.x, tid);
    const double E0 = E;
    double lambda = kFitLambda0;
    int accepted = 0;
    bool fresh = false;                              // H and g belong to the current x
    if (normal || a.iters > 0) {
        fit_normal(s, tid);
        fresh = true;
    }
    if (normal) fit_dump_normal(s, normal, tid);
    for (int it = 0; it < a.iters; ++it) {
        if (!fresh) {
            E = fit_evaluate<true>(s, s.x, tid);
            fit_normal(s, tid);
            fresh = true;
        }
        for (int tr = 0; tr < kFitTries; ++tr) {
            bool ok = fit_solve(s, lambda, tid);
            if (ok) {
                if (tid < kFitX) s.xt[tid] = s.x[tid] + s.rhs[tid];
                __syncthreads();
                const double Et = fit_evaluate<false>(s, s.xt, tid);
                ok = Et < E;
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
    fit_evaluate<false>(s, s.x, tid);                // the residuals at the answer
    if (tid < kFitX) params[tid] = s.x[tid];
    if (tid == 0) {
        double sc = 0.0, sr = 0.0;
        for (int j = 0; j < NJ; ++j) {
            sc += s.c[j];
            sr += s.c[j] * (s.res[j * 3] * s.res[j * 3] + s.res[j * 3 + 1] * s.res[j * 3 + 1] + s.res[j * 3 + 2] * s.res[j * 3 + 2]);
        }
        report[0] = 1.0; report[1] = E0; report[2] = E; report[3] = (double)accepted; report[4] = lambda; report[5] = sqrt(sr / sc);
    }
}

// ---- the sums one shared shape needs ----
struct FitMomArgs {
    const float* Jt;
    const float* Js;
    const int* parents;
    const float* targets;         // [N,22,3]
    const float* conf;            // [N,22] or null
    const double* params;         // [N,69]
    const unsigned char* use;     // [N]
    int N;
    double* per_frame;            // [N,66]
    double* out;                  // [66]
};

// One workgroup of 128 threads per frame.  With the pose fixed p_j + t = a_j + A_j beta: A_0 = Js_0, A_j = A_p + G_p (Js_j - Js_p),
// a_j the same chain on Jt, plus t.  22 lanes take Rodrigues, lane 0 the chain of G, 33 lanes a column of A (10) or a (1) each
// along the tree, 66 lanes one sum each over the joints in joint order.
__global__ __launch_bounds__(kFitMomThreads) void fit_shape_moments_kernel(const FitMomArgs a) {
    __shared__ double R[NJ * 9], G[NJ * 9], A[NJ * 3 * 11], y[NJ * 3], c[NJ];
    __shared__ int parents[NJ];
    const int tid = threadIdx.x;
    const size_t f = blockIdx.x;
    double* row = a.per_frame + f * kFitMom;
    if (!a.use[f]) {
        if (tid < kFitMom) row[tid] = 0.0;
        return;
    }
    const double* x = a.params + f * kFitX;
    if (tid < NJ) {
        load_observation(a.targets, a.conf, f, tid, c, y);
        parents[tid] = a.parents[tid];
        const double r[3] = {x[tid * 3], x[tid * 3 + 1], x[tid * 3 + 2]};
        rodrigues64(r, R + tid * 9);
    }
    __syncthreads();
    if (tid == 0) chain64(R, nullptr, parents, G, nullptr);
    __syncthreads();
    if (tid < 33) {
        const int cc = tid / 11, k = tid % 11;
        auto basis = [&](int j, int b) { return k < NBETA ? (double)a.Js[(j * 3 + b) * NBETA + k] : (double)a.Jt[j * 3 + b]; };
        A[cc * 11 + k] = basis(0, cc);
        for (int j = 1; j < NJ; ++j) {
            const int p = parents[j];
            double v = 0.0;
            for (int b = 0; b < 3; ++b) v += G[p * 9 + cc * 3 + b] * (basis(j, b) - basis(p, b));
            A[(j * 3 + cc) * 11 + k] = A[(p * 3 + cc) * 11 + k] + v;
        }
    }
    __syncthreads();
    if (tid < kFitMom) {
        double v = 0.0;
        if (tid < 55) {                              // the upper triangle of sum c A^T A, row-major
            int i = 0, left = tid;
            while (left >= NBETA - i) { left -= NBETA - i; ++i; }
            const int k = i + left;
            for (int j = 0; j < NJ; ++j) {
                double q = 0.0;
                for (int cc = 0; cc < 3; ++cc) q += A[(j * 3 + cc) * 11 + i] * A[(j * 3 + cc) * 11 + k];
                v += c[j] * q;
            }
        } else {
            const int i = tid - 55;                  // 0..9: sum c A^T (y - a); 10: sum c |y - a|^2
            for (int j = 0; j < NJ; ++j) {
                double q = 0.0;
                for (int cc = 0; cc < 3; ++cc) {
                    const double e = y[j * 3 + cc] - (A[(j * 3 + cc) * 11 + NBETA] + x[kFitRot + cc]);
                    q += (i < NBETA ? A[(j * 3 + cc) * 11 + i] : e) * e;
                }
                v += c[j] * q;
            }
        }
        row[tid] = v;
    }
}

// out[k] = sum over the frames of per_frame[., k]: one workgroup per k, thread t takes the frames t, t + 256, ... in ascending order,
// then reduce.h's block_reduce of one value (a xor-butterfly per wave, the 4 wave partials in wave order)
__global__ __launch_bounds__(kFitTotThreads) void fit_shape_total_kernel(const double* __restrict__ per_frame, int N, double* __restrict__ out) {
    __shared__ double sh[kFitTotThreads / 64][1];
    const int tid = threadIdx.x, k = blockIdx.x;
    double v[1] = {0.0};
    for (int i = tid; i < N; i += kFitTotThreads) v[0] += per_frame[(size_t)i * kFitMom + k];
    block_reduce<kFitTotThreads, 1>(v, sh, out + k, SumOfK());
}

}  // namespace rohm

using namespace rohm;

extern "C" int rohm_fit_pose(const rohm_smplx_t* h, const float* targets, const float* conf, const float* betas, const double* init,
                             const double* prev, const double* w_prior, double w_smooth, int iters, int min_joints, int N, double* params,
                             double* report, double* normal, rohm_stream_t stream) {
    ROHM_ARG_CHECK(N >= 0, "fit_pose: N must be >= 0, got %d", N);
    ROHM_ARG_CHECK(iters >= 0 && min_joints >= 1 && min_joints <= NJ, "fit_pose: need iters >= 0 and 1 <= min_joints <= %d (got iters=%d min_joints=%d)",
                   NJ, iters, min_joints);
    ROHM_ARG_CHECK(w_smooth >= 0.0, "fit_pose: w_smooth must be >= 0 (a NaN is refused too)");
    if (N == 0) return ROHM_OK;
    ROHM_ARG_CHECK(h && targets && betas && w_prior && params && report, "fit_pose: null argument");
    ROHM_ARG_CHECK(h->J >= NJ, "fit_pose: the body model has %d joints, fewer than %d", h->J, NJ);
    FitPoseArgs a;
    a.Jt = h->d_Jt; a.Js = h->d_Js; a.parents = h->d_parents; a.targets = targets; a.conf = conf; a.betas = betas; a.init = init; a.prev = prev;
    a.w_prior = w_prior; a.w_smooth = w_smooth; a.iters = iters; a.min_joints = min_joints; a.N = N; a.params = params; a.report = report;
    a.normal = normal;
    prof::Scope ps("fit_pose", (double)N * (iters + 1) * 2.0 * kFitTri * kFitRot, (double)N * (4.0 * 98 + 8.0 * (kFitX * 3 + 6)), (hipStream_t)stream);
    hipLaunchKernelGGL(fit_pose_kernel, dim3((unsigned)N), dim3(kFitThreads), 0, (hipStream_t)stream, a);
    ROHM_LAUNCH_CHECK();
    return ROHM_OK;
}

extern "C" int rohm_fit_shape_moments(const rohm_smplx_t* h, const float* targets, const float* conf, const double* params,
                                      const unsigned char* use, int N, double* per_frame, double* out, rohm_stream_t stream) {
    ROHM_ARG_CHECK(N >= 0, "fit_shape_moments: N must be >= 0, got %d", N);
    if (N == 0) return ROHM_OK;
    ROHM_ARG_CHECK(h && targets && params && use && per_frame && out, "fit_shape_moments: null argument");
    ROHM_ARG_CHECK(h->J >= NJ, "fit_shape_moments: the body model has %d joints, fewer than %d", h->J, NJ);
    FitMomArgs a;
    a.Jt = h->d_Jt; a.Js = h->d_Js; a.parents = h->d_parents; a.targets = targets; a.conf = conf; a.params = params; a.use = use; a.N = N;
    a.per_frame = per_frame; a.out = out;
    prof::Scope ps("fit_shape_moments", 0.0, (double)N * (4.0 * 88 + 8.0 * (kFitX + 2 * kFitMom)), (hipStream_t)stream);
    hipLaunchKernelGGL(fit_shape_moments_kernel, dim3((unsigned)N), dim3(kFitMomThreads), 0, (hipStream_t)stream, a);
    ROHM_LAUNCH_CHECK();
    hipLaunchKernelGGL(fit_shape_total_kernel, dim3(kFitMom), dim3(kFitTotThreads), 0, (hipStream_t)stream, per_frame, N, out);
    ROHM_LAUNCH_CHECK();
    return ROHM_OK;
}
