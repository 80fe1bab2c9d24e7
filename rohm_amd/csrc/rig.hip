// Rig calibration from the person's own 2-D keypoints: epipolar RANSAC for all pairs of views in one call
// (rohm_rig_pair_hypotheses), the sums of the inlier refit (rohm_rig_pair_moments) and one Levenberg-Marquardt try of bundle
// adjustment with the points eliminated (rohm_rig_ba_moments, rohm_rig_ba_update).  rohm_amd/rig.py drives them (the sampling, the
// spanning tree, the LM schedule and the Cholesky solve of the 6 V camera unknowns are host logic); tests/rig_ref.py restates them
// in numpy; include/rohm_rig.h states the rule in full.  There is no counterpart in the reference.
//
// The camera row is camera_math.h's, shared with multiview.hip and fit_views.hip; epipolar_math.h holds what sync.hip shares; the rotation update is fit_math.h's rodrigues64.
// All arithmetic is float64 on the float32 keypoints.  No atomics: the scores are integer counts, and every float64 sum has one owner
// that adds in a fixed order, or is a fixed butterfly: the same input gives the same bits.
//
// rohm_rig_pair_hypotheses is the hot one: pairs x hypotheses x points Sampson distances, 1e11 for 16 views, 1024 hypotheses per
// pair and a ten-minute recording.  As in floor.hip a workgroup holds a handful of hypotheses -- 32: 16 lanes by two -- and the pair's
// points pass through LDS once per tile of 512 for all of them; a wave reads four points per step, each broadcast to 16 lanes.  A
// leading launch undistorts every view's points once into the workspace (NaN where unobserved), not once per pair.  The 9 x 9
// eigenproblem of a hypothesis (45 + 81 float64) does not fit a thread's registers: 16 lanes share it in LDS, lane k turning row k,
// then column k, of every Jacobi rotation; the 32 hypotheses of a workgroup take two rounds of 16.  The inlier test needs neither
// the root nor the division of the Sampson distance.
//
// rohm_rig_ba_moments: 16 lanes per point as in multiview.hip, lane v view v; a tile of 16 points leaves H_cp (6 x 3 per view),
// H_pp,d^-1 and g_p in LDS, then every thread owns up to four (camera row, camera) strips of six entries of S, in registers, and
// adds the tile's points to them in order, touching only the points both cameras see.  Blocks (v1, v2) with v1 <= v2 only; the
// closing launch mirrors.
#include "common.h"
#include "camera_math.h"
#include "epipolar_math.h"
#include "fit_math.h"
#include "reduce.h"
#include "../../include/rohm_rig.h"

#include <limits.h>

namespace rohm {

constexpr long long kRigMaxHyp = 1ll << 27;
constexpr int kRigThreads = 256;
constexpr int kRigHypLanes = 16;                     // lanes that share an eigenproblem; hypotheses side by side in the scoring
constexpr int kRigHypPerLane = 2;
constexpr int kRigHypPerBlock = kRigHypLanes * kRigHypPerLane;
constexpr int kRigGroups = kRigThreads / kRigHypLanes;
constexpr int kRigTile = 512;                        // points per LDS tile: 4 float64 each
constexpr int kRigSweeps = 10;
constexpr double kRigGapMin = 1e-12;
constexpr int kRigMoments = 47;
constexpr int kRigMomThreads = 256;
constexpr int kRigPickThreads = 256;
constexpr int kBaPts = 16;                           // points per tile, 16 lanes each
constexpr int kBaMaxGroups = 256;
constexpr int kBaSlots = 4;                          // strips of S per thread: 6 * 136 = 816 <= 4 * 256
constexpr int kBaCam = 29;                           // per view: U (21), g_c (6), E, the count
constexpr double kBaDiagEps = 1e-9;

// ---- the undistorted coordinates of every view, once (sync.hip launches it too, through epipolar_math.h's rig_undistort) ----
__global__ __launch_bounds__(256) void rig_undistort_kernel(const float* __restrict__ kp, const double* __restrict__ cams, long long P,
                                                            long long total, double conf_min, double* __restrict__ und) {
    const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= total) return;
    const double* cam = cams + (size_t)(i / P) * kCamRow;
    const double x = (double)kp[i * 3], y = (double)kp[i * 3 + 1], c = (double)kp[i * 3 + 2];
    double a = (double)NAN, b = (double)NAN;
    if (cam_observed(x, y, c, conf_min)) {
        cam_undistort(cam, x, y, a, b);
        if (!(isfinite(a) && isfinite(b))) a = b = (double)NAN;
    }
    und[i * 2] = a;
    und[i * 2 + 1] = b;
}

struct RigHypArgs {
    const double* und;            // [V,P,2]
    const double* cams;
    const int* pairs;             // [Q,2]
    const int* samples;           // [Q,K,8]
    int V, K;
    long long P;
    double tau2;
    double* E;                    // [Q,K,9]
    long long* counts;            // [Q,K,2]
};

__global__ __launch_bounds__(kRigThreads) void rig_hypotheses_kernel(const RigHypArgs g) {
    // phase 1: A [16][81], Vm [16][81], rows [16][8][9]; phase 2: the tile [512][4]
    __shared__ double sh[kRigHypLanes * (81 + 81 + 72)];
    __shared__ double Esh[kRigHypPerBlock][9];
    __shared__ int sidx[kRigHypLanes][8];
    __shared__ int shc[4 * kRigHypLanes];
    double* const A = sh;
    double* const Vm = sh + kRigHypLanes * 81;
    double* const rows = sh + kRigHypLanes * 162;
    const int tid = threadIdx.x;
    const int q = blockIdx.y;
    const int v1 = g.pairs[q * 2], v2 = g.pairs[q * 2 + 1];
    const bool pair_ok = rig_pair_ok(v1, v2, g.V);   // uniform in the workgroup
    const long long P = g.P;
    const double nan = (double)NAN;
    const double* u1 = g.und + (size_t)(pair_ok ? v1 : 0) * (size_t)P * 2;
    const double* u2 = g.und + (size_t)(pair_ok ? v2 : 0) * (size_t)P * 2;

    // ---- rules 1 to 3: two rounds of 16 eigenproblems, 16 lanes each
    const int hl = tid / kRigHypLanes, l = tid % kRigHypLanes;
    for (int round = 0; round < kRigHypPerLane; ++round) {
        const int slot = round * kRigHypLanes + hl;
        const long long h = (long long)blockIdx.x * kRigHypPerBlock + slot;
        bool bad = false;
        int idx = -1;
        if (l < 8) {
            double a1 = 0.0, b1 = 0.0, a2 = 0.0, b2 = 0.0;
            bad = true;
            if (h < g.K && pair_ok) {
                idx = g.samples[((size_t)q * g.K + (size_t)h) * 8 + l];
                if (idx >= 0 && idx < P) {
                    a1 = u1[(size_t)idx * 2]; b1 = u1[(size_t)idx * 2 + 1];
                    a2 = u2[(size_t)idx * 2]; b2 = u2[(size_t)idx * 2 + 1];
                    bad = !(isfinite(a1) && isfinite(b1) && isfinite(a2) && isfinite(b2));
                }
            }
            if (bad) a1 = b1 = a2 = b2 = 0.0;
            sidx[hl][l] = idx;
            double* row = rows + (hl * 8 + l) * 9;
            row[0] = a2 * a1; row[1] = a2 * b1; row[2] = a2;
            row[3] = b2 * a1; row[4] = b2 * b1; row[5] = b2;
            row[6] = a1;      row[7] = b1;      row[8] = 1.0;
        }
        __syncthreads();
        if (l < 8 && !bad)
            for (int m = 0; m < l; ++m) bad = bad || sidx[hl][m] == idx;      // a repeated index
        const unsigned long long ballot = __ballot(bad);
        bool dead = ((ballot >> ((tid & 63) - l)) & 0xffffull) != 0ull;    // uniform in the 16 lanes
        for (int e = l; e < 81; e += kRigHypLanes) {
            const int i = e / 9, j = e % 9;
            double s = 0.0;
#pragma unroll
            for (int k = 0; k < 8; ++k) s += rows[(hl * 8 + k) * 9 + i] * rows[(hl * 8 + k) * 9 + j];      // in sample order
            A[hl * 81 + e] = s;
            Vm[hl * 81 + e] = i == j ? 1.0 : 0.0;
        }
        __syncthreads();
        double* a = A + hl * 81;
        double* vm = Vm + hl * 81;
        for (int sweep = 0; sweep < kRigSweeps; ++sweep)
            for (int p = 0; p < 8; ++p)
                for (int r = p + 1; r < 9; ++r) {
                    const double app = a[p * 9 + p], arr = a[r * 9 + r], apr = a[p * 9 + r];
                    double c = 1.0, s = 0.0;
                    if (apr != 0.0) {
                        const double theta = (arr - app) / (2.0 * apr);
                        const double t = (theta >= 0.0 ? 1.0 : -1.0) / (fabs(theta) + sqrt(theta * theta + 1.0));
                        c = 1.0 / sqrt(t * t + 1.0);
                        s = t * c;
                    }
                    __syncthreads();                 // everyone has read the three entries
                    if (l < 9) {                     // A J and V J: row l, columns p and r
                        const double x = a[l * 9 + p], y = a[l * 9 + r];
                        a[l * 9 + p] = c * x - s * y;
                        a[l * 9 + r] = s * x + c * y;
                        const double vx = vm[l * 9 + p], vy = vm[l * 9 + r];
                        vm[l * 9 + p] = c * vx - s * vy;
                        vm[l * 9 + r] = s * vx + c * vy;
                    }
                    __syncthreads();
                    if (l < 9) {                     // J^T (A J): column l, rows p and r
                        const double x = a[p * 9 + l], y = a[r * 9 + l];
                        a[p * 9 + l] = c * x - s * y;
                        a[r * 9 + l] = s * x + c * y;
                    }
                    __syncthreads();
                }
        double lmin = (double)INFINITY, l2 = (double)INFINITY, lmax = -(double)INFINITY;
        int i0 = 0;
        bool finite = true;
        for (int k = 0; k < 9; ++k) {
            const double d = a[k * 9 + k];
            finite = finite && isfinite(d);
            if (d < lmin) { l2 = lmin; lmin = d; i0 = k; }
            else if (d < l2) l2 = d;
            if (d > lmax) lmax = d;
        }
        dead = dead || !finite || !(l2 >= kRigGapMin * lmax);
        double top = 0.0, sign = 1.0;
        for (int k = 0; k < 9; ++k) {
            const double e = vm[k * 9 + i0];
            if (fabs(e) > top) { top = fabs(e); sign = e < 0.0 ? -1.0 : 1.0; }
        }
        if (l < 9) {
            const double e = dead ? nan : sign * vm[l * 9 + i0];
            Esh[slot][l] = e;
            if (h < g.K) g.E[((size_t)q * g.K + (size_t)h) * 9 + l] = e;
        }
        __syncthreads();                             // the next round, and the tiles, write over A, Vm and rows
    }

    // ---- rule 4: lane h2 of every group scores its two hypotheses against the group's share of each tile
    const int h2 = tid % kRigHypLanes, grp = tid / kRigHypLanes;
    double E[kRigHypPerLane][9];
#pragma unroll
    for (int k = 0; k < kRigHypPerLane; ++k)
#pragma unroll
        for (int i = 0; i < 9; ++i) E[k][i] = Esh[k * kRigHypLanes + h2][i];
    int inl[kRigHypPerLane] = {0, 0}, common = 0;
    if (pair_ok) {
        const double* c1 = g.cams + (size_t)v1 * kCamRow;
        const double* c2 = g.cams + (size_t)v2 * kCamRow;
        const double scale = (c1[12] + c1[13] + c2[12] + c2[13]) / 4.0;
        double* tile = sh;
        for (long long base = 0; base < P; base += kRigTile) {
            const int cnt = (int)min((long long)kRigTile, P - base);
            for (int i = tid; i < cnt; i += kRigThreads) {
                tile[i * 4] = u1[(size_t)(base + i) * 2];
                tile[i * 4 + 1] = u1[(size_t)(base + i) * 2 + 1];
                tile[i * 4 + 2] = u2[(size_t)(base + i) * 2];
                tile[i * 4 + 3] = u2[(size_t)(base + i) * 2 + 1];
            }
            __syncthreads();
#pragma unroll 2
            for (int i = grp; i < cnt; i += kRigGroups) {
                const double a1 = tile[i * 4], b1 = tile[i * 4 + 1], a2 = tile[i * 4 + 2], b2 = tile[i * 4 + 3];
                const bool both = isfinite(a1) && isfinite(b1) && isfinite(a2) && isfinite(b2);
                common += both ? 1 : 0;
#pragma unroll
                for (int k = 0; k < kRigHypPerLane; ++k) {
                    double ns, den;
                    rig_sampson(E[k], a1, b1, a2, b2, scale, ns, den);
                    inl[k] += (both && den > 0.0 && ns * ns <= g.tau2 * den) ? 1 : 0;      // false for a NaN
                }
            }
            __syncthreads();
        }
    }
    common = group_sum<kRigHypLanes>(common, shc, tid);
#pragma unroll
    for (int k = 0; k < kRigHypPerLane; ++k) {
        const int n = group_sum<kRigHypLanes>(inl[k], shc, tid);
        const long long h = (long long)blockIdx.x * kRigHypPerBlock + k * kRigHypLanes + tid;
        if (tid < kRigHypLanes && h < g.K) {
            const bool live = E[k][0] == E[k][0];    // a degenerate hypothesis is all NaN
            g.counts[((size_t)q * g.K + (size_t)h) * 2] = live ? (long long)n : -1;
            g.counts[((size_t)q * g.K + (size_t)h) * 2 + 1] = live ? (long long)common : -1;
        }
    }
}

// ---- the sums of the inlier refit: one workgroup per pair; thread t takes the points t, t + 256, ... in ascending order ----
__global__ __launch_bounds__(kRigMomThreads) void rig_moments_kernel(const double* __restrict__ und, const double* __restrict__ cams,
                                                                     const int* __restrict__ pairs, const double* __restrict__ Es, int V,
                                                                     long long P, double tau2, double* __restrict__ out) {
    __shared__ double shm[kRigMomThreads / 64][kRigMoments];
    const int tid = threadIdx.x, q = blockIdx.x;
    const int v1 = pairs[q * 2], v2 = pairs[q * 2 + 1];
    if (!rig_pair_ok(v1, v2, V)) {                   // uniform in the workgroup
        if (tid < kRigMoments) out[(size_t)q * kRigMoments + tid] = (double)NAN;
        return;
    }
    double E[9];
#pragma unroll
    for (int i = 0; i < 9; ++i) E[i] = Es[(size_t)q * 9 + i];
    const double* c1 = cams + (size_t)v1 * kCamRow;
    const double* c2 = cams + (size_t)v2 * kCamRow;
    const double scale = (c1[12] + c1[13] + c2[12] + c2[13]) / 4.0;
    const double* u1 = und + (size_t)v1 * (size_t)P * 2;
    const double* u2 = und + (size_t)v2 * (size_t)P * 2;
    double m[kRigMoments];
#pragma unroll
    for (int k = 0; k < kRigMoments; ++k) m[k] = 0.0;
    for (long long p = tid; p < P; p += kRigMomThreads) {
        const double a1 = u1[p * 2], b1 = u1[p * 2 + 1], a2 = u2[p * 2], b2 = u2[p * 2 + 1];
        double ns, den;
        rig_sampson(E, a1, b1, a2, b2, scale, ns, den);
        if (isfinite(a1) && isfinite(b1) && isfinite(a2) && isfinite(b2) && den > 0.0 && ns * ns <= tau2 * den) {
            const double row[9] = {a2 * a1, a2 * b1, a2, b2 * a1, b2 * b1, b2, a1, b1, 1.0};
            m[0] += 1.0;
            m[1] += ns * ns / den;
            int k = 2;
#pragma unroll
            for (int i = 0; i < 9; ++i)
#pragma unroll
                for (int j = i; j < 9; ++j) m[k++] += row[i] * row[j];
        }
    }
    block_reduce<kRigMomThreads, kRigMoments>(m, shm, out + (size_t)q * kRigMoments, SumOfK());
}

// ---- bundle adjustment ----
struct BaArgs {
    const float* kp;
    const double* cams;
    const double* points;
    const double* dc;
    int V;
    long long P;
    double conf_min, sigma2, lambda;
    double* ws;
    int tiles, tiles_per_group, n_tasks, stride;
    double* points_new;
    double* cams_new;
};

// What lane v holds of point p: the weight w = c rho' (0 when the lane adds nothing), the residual, the rows of J_X and J_c, its share
// e of the energy and whether it is an observation; and, the same in all 16 lanes, whether the point is inside the problem, H_pp,d
// (packed) and g_p.
struct BaLane {
    double w, r[2], jx[2][3], jc[2][6], e;
    bool counted, inside;
    unsigned seen;                // bit v: view v adds to the sums of this point
    double Hd[6], gp[3], X[3];
};

__device__ __forceinline__ void ba_lane(const BaArgs& g, long long p, int lane, BaLane& o) {
    const bool live = p < g.P;
    bool obs = false;
    double a = 0.0, b = 0.0, c = 0.0;
    o.X[0] = o.X[1] = o.X[2] = 0.0;
    bool fin = false;
    if (live) {
#pragma unroll
        for (int k = 0; k < 3; ++k) o.X[k] = g.points[(size_t)p * 3 + k];
        fin = isfinite(o.X[0]) && isfinite(o.X[1]) && isfinite(o.X[2]);
    }
    const double* cam = g.cams + (size_t)(lane < g.V ? lane : 0) * kCamRow;
    if (live && fin && lane < g.V) {
        const size_t at = ((size_t)lane * (size_t)g.P + (size_t)p) * 3;
        const double x = (double)g.kp[at], y = (double)g.kp[at + 1];
        c = (double)g.kp[at + 2];
        if (cam_observed(x, y, c, g.conf_min)) {
            cam_undistort(cam, x, y, a, b);
            obs = isfinite(a) && isfinite(b);
        }
    }
    const unsigned S = (unsigned)(__ballot(obs) >> ((threadIdx.x & 63) - lane)) & 0xffffu;
    o.inside = __popc(S) >= 2;
    o.counted = obs && o.inside;
    o.w = 0.0;
    o.e = 0.0;
    o.r[0] = o.r[1] = 0.0;
#pragma unroll
    for (int k = 0; k < 3; ++k) o.jx[0][k] = o.jx[1][k] = 0.0;
#pragma unroll
    for (int k = 0; k < 6; ++k) o.jc[0][k] = o.jc[1][k] = 0.0;
    bool adds = false;
    if (o.counted) {
        double Xc[3];
        cam_to_view(cam, o.X, Xc);
        if (Xc[2] > 0.0) {
            const double e2 = cam_residual<true>(cam, o.X, a, b, o.r, o.jx[0], o.jx[1]);
            double rho = e2, drho = 1.0;
            if (g.sigma2 > 0.0) {
                const double qq = g.sigma2 / (g.sigma2 + e2);
                rho = qq * e2;
                drho = qq * qq;
            }
            o.e = c * rho;
            o.w = c * drho;
            adds = true;
            const double u = Xc[0] / Xc[2], v = Xc[1] / Xc[2];
            const double A[2][3] = {{cam[12] / Xc[2], 0.0, -cam[12] * u / Xc[2]}, {0.0, cam[13] / Xc[2], -cam[13] * v / Xc[2]}};
            const double Y[3] = {Xc[0] - cam[9], Xc[1] - cam[10], Xc[2] - cam[11]};     // R X
#pragma unroll
            for (int k = 0; k < 2; ++k) {            // -A [Y]x: row k is Y x A_k
                o.jc[k][0] = Y[1] * A[k][2] - Y[2] * A[k][1];
                o.jc[k][1] = Y[2] * A[k][0] - Y[0] * A[k][2];
                o.jc[k][2] = Y[0] * A[k][1] - Y[1] * A[k][0];
                o.jc[k][3] = A[k][0];
                o.jc[k][4] = A[k][1];
                o.jc[k][5] = A[k][2];
            }
        } else {
            o.e = (double)INFINITY;                  // behind the camera: the try is lost, the sums go on without it
        }
    }
    o.seen = (unsigned)(__ballot(adds) >> ((threadIdx.x & 63) - lane)) & 0xffffu;
    const double w = o.w;
    o.Hd[0] = lanes_sum<16>(w * (o.jx[0][0] * o.jx[0][0] + o.jx[1][0] * o.jx[1][0]));
    o.Hd[1] = lanes_sum<16>(w * (o.jx[0][0] * o.jx[0][1] + o.jx[1][0] * o.jx[1][1]));
    o.Hd[2] = lanes_sum<16>(w * (o.jx[0][0] * o.jx[0][2] + o.jx[1][0] * o.jx[1][2]));
    o.Hd[3] = lanes_sum<16>(w * (o.jx[0][1] * o.jx[0][1] + o.jx[1][1] * o.jx[1][1]));
    o.Hd[4] = lanes_sum<16>(w * (o.jx[0][1] * o.jx[0][2] + o.jx[1][1] * o.jx[1][2]));
    o.Hd[5] = lanes_sum<16>(w * (o.jx[0][2] * o.jx[0][2] + o.jx[1][2] * o.jx[1][2]));
#pragma unroll
    for (int k = 0; k < 3; ++k) o.gp[k] = lanes_sum<16>(w * (o.jx[0][k] * o.r[0] + o.jx[1][k] * o.r[1]));
    o.Hd[0] += g.lambda * (o.Hd[0] + kBaDiagEps);
    o.Hd[3] += g.lambda * (o.Hd[3] + kBaDiagEps);
    o.Hd[5] += g.lambda * (o.Hd[5] + kBaDiagEps);
}

// the strip (v1, i, v2) of a task: row i of camera v1 against the six columns of camera v2 >= v1
__device__ __forceinline__ void ba_task(int task, int V, int& v1, int& i, int& v2) {
    int blk = task / 6;
    i = task % 6;
    v1 = 0;
    while (blk >= V - v1) {
        blk -= V - v1;
        ++v1;
    }
    v2 = v1 + blk;
}

__global__ __launch_bounds__(kRigThreads) void rig_ba_moments_kernel(const BaArgs g) {
    __shared__ double Ysh[kBaPts * kViewsMax * 18];          // H_cp of the tile: [point][view][6][3]
    __shared__ double Hish[kBaPts][9];                           // H_pp,d^-1, column by column
    __shared__ double gpsh[kBaPts][3];
    __shared__ unsigned seensh[kBaPts];
    const int tid = threadIdx.x, pt = tid / 16, lane = tid % 16, V = g.V;
    int tv1[kBaSlots], ti[kBaSlots], tv2[kBaSlots];
    double acc[kBaSlots][6], racc[kBaSlots];
#pragma unroll
    for (int s = 0; s < kBaSlots; ++s) {
        const int task = tid + s * kRigThreads;
        tv1[s] = -1; ti[s] = 0; tv2[s] = 0;
        if (task < g.n_tasks) ba_task(task, V, tv1[s], ti[s], tv2[s]);
        racc[s] = 0.0;
#pragma unroll
        for (int j = 0; j < 6; ++j) acc[s][j] = 0.0;
    }
    double U[21], gc[6], Esum = 0.0, nsum = 0.0;
#pragma unroll
    for (int k = 0; k < 21; ++k) U[k] = 0.0;
#pragma unroll
    for (int k = 0; k < 6; ++k) gc[k] = 0.0;

    const int t0 = blockIdx.x * g.tiles_per_group, t1 = min(t0 + g.tiles_per_group, g.tiles);
    for (int t = t0; t < t1; ++t) {
        BaLane o;
        ba_lane(g, (long long)t * kBaPts + pt, lane, o);
        {
            int k = 0;
#pragma unroll
            for (int i = 0; i < 6; ++i) {
#pragma unroll
                for (int j = i; j < 6; ++j) U[k++] += o.w * (o.jc[0][i] * o.jc[0][j] + o.jc[1][i] * o.jc[1][j]);
                gc[i] += o.w * (o.jc[0][i] * o.r[0] + o.jc[1][i] * o.r[1]);
            }
            Esum += o.e;
            nsum += o.counted ? 1.0 : 0.0;
        }
        double* Y = Ysh + (pt * kViewsMax + lane) * 18;
#pragma unroll
        for (int i = 0; i < 6; ++i)
#pragma unroll
            for (int a = 0; a < 3; ++a) Y[i * 3 + a] = o.w * (o.jc[0][i] * o.jx[0][a] + o.jc[1][i] * o.jx[1][a]);
        if (lane < 3) {                              // column `lane` of the inverse
            double col[3] = {0.0, 0.0, 0.0};
            if (o.inside && o.seen) {
                const double unit[3] = {lane == 0 ? 1.0 : 0.0, lane == 1 ? 1.0 : 0.0, lane == 2 ? 1.0 : 0.0};
                cam_solve3(o.Hd, unit, col);
            }
            Hish[pt][lane] = col[0];
            Hish[pt][3 + lane] = col[1];
            Hish[pt][6 + lane] = col[2];
        }
        if (lane == 3) {
            gpsh[pt][0] = o.gp[0];
            gpsh[pt][1] = o.gp[1];
            gpsh[pt][2] = o.gp[2];
            seensh[pt] = o.inside ? o.seen : 0u;
        }
        __syncthreads();
#pragma unroll
        for (int s = 0; s < kBaSlots; ++s) {
            if (tv1[s] < 0) continue;
            const unsigned need = (1u << tv1[s]) | (1u << tv2[s]);
            for (int q = 0; q < kBaPts; ++q) {       // the tile's points in ascending order
                if ((seensh[q] & need) != need) continue;
                const double* y1 = Ysh + (q * kViewsMax + tv1[s]) * 18 + ti[s] * 3;
                const double* y2 = Ysh + (q * kViewsMax + tv2[s]) * 18;
                const double* Hi = Hish[q];
                const double z0 = y1[0] * Hi[0] + y1[1] * Hi[3] + y1[2] * Hi[6];
                const double z1 = y1[0] * Hi[1] + y1[1] * Hi[4] + y1[2] * Hi[7];
                const double z2 = y1[0] * Hi[2] + y1[1] * Hi[5] + y1[2] * Hi[8];
#pragma unroll
                for (int j = 0; j < 6; ++j) acc[s][j] -= z0 * y2[j * 3] + z1 * y2[j * 3 + 1] + z2 * y2[j * 3 + 2];
                if (tv1[s] == tv2[s]) racc[s] -= z0 * gpsh[q][0] + z1 * gpsh[q][1] + z2 * gpsh[q][2];
            }
        }
        __syncthreads();
    }

    double* part = g.ws + (size_t)blockIdx.x * (size_t)g.stride;
#pragma unroll
    for (int s = 0; s < kBaSlots; ++s) {
        if (tv1[s] < 0) continue;
        const int task = tid + s * kRigThreads;
#pragma unroll
        for (int j = 0; j < 6; ++j) part[(size_t)task * 6 + j] = acc[s][j];
        if (tv1[s] == tv2[s]) part[(size_t)g.n_tasks * 6 + tv1[s] * 6 + ti[s]] = racc[s];
    }
    // U, g_c, E and the count: per lane over the tiles above, now over the 16 lanes of a view in ascending order, 18 and 11 values at a time
    double* cam_part = part + (size_t)g.n_tasks * 6 + 6 * V;
#pragma unroll
    for (int k = 0; k < 18; ++k) Ysh[tid * 18 + k] = U[k];
    __syncthreads();
    for (int e = tid; e < V * 18; e += kRigThreads) {
        const int v = e / 18, k = e % 18;
        double s = 0.0;
        for (int q = 0; q < kBaPts; ++q) s += Ysh[(q * 16 + v) * 18 + k];
        cam_part[v * kBaCam + k] = s;
    }
    __syncthreads();
    Ysh[tid * 18] = U[18]; Ysh[tid * 18 + 1] = U[19]; Ysh[tid * 18 + 2] = U[20];
#pragma unroll
    for (int k = 0; k < 6; ++k) Ysh[tid * 18 + 3 + k] = gc[k];
    Ysh[tid * 18 + 9] = Esum;
    Ysh[tid * 18 + 10] = nsum;
    __syncthreads();
    for (int e = tid; e < V * 11; e += kRigThreads) {
        const int v = e / 11, k = e % 11;
        double s = 0.0;
        for (int q = 0; q < kBaPts; ++q) s += Ysh[(q * 16 + v) * 18 + k];
        cam_part[v * kBaCam + 18 + k] = s;
    }
}

// S, r and stats from the workgroups' partials, added in workgroup order; the lower triangle mirrors the upper
__global__ __launch_bounds__(256) void rig_ba_close_kernel(const double* __restrict__ ws, int G, int stride, int n_tasks, int V, double lambda,
                                                           double* __restrict__ S, double* __restrict__ r, double* __restrict__ stats) {
    const int n = 6 * V;
    const int e = blockIdx.x * 256 + threadIdx.x;
    const int off_r = n_tasks * 6, off_c = n_tasks * 6 + n;
    if (e < n * n) {
        int row = e / n, col = e % n;
        if (row > col) { const int t = row; row = col; col = t; }
        const int v1 = row / 6, i = row % 6, v2 = col / 6, j = col % 6;
        const int blk = v1 * V - v1 * (v1 - 1) / 2 + (v2 - v1);
        double s = 0.0;
        for (int w = 0; w < G; ++w) s += ws[(size_t)w * stride + (size_t)(blk * 6 + i) * 6 + j];
        if (v1 == v2) {
            const int k = i * 6 - i * (i - 1) / 2 + (j - i);
            double u = 0.0;
            for (int w = 0; w < G; ++w) u += ws[(size_t)w * stride + off_c + v1 * kBaCam + k];
            if (i == j) u += lambda * (u + kBaDiagEps);
            s = u + s;
        }
        S[e] = s;
    } else if (e < n * n + n) {
        const int row = e - n * n;
        double gcs = 0.0, s = 0.0;
        for (int w = 0; w < G; ++w) gcs += ws[(size_t)w * stride + off_c + (row / 6) * kBaCam + 21 + row % 6];
        for (int w = 0; w < G; ++w) s += ws[(size_t)w * stride + off_r + row];
        r[row] = gcs + s;
    } else if (e < n * n + n + 2) {
        const int k = e - n * n - n;                 // 0: E, 1: the count
        double s = 0.0;
        for (int w = 0; w < G; ++w)
            for (int v = 0; v < V; ++v) s += ws[(size_t)w * stride + off_c + v * kBaCam + 27 + k];
        stats[k] = s;
    }
}

__global__ __launch_bounds__(kRigThreads) void rig_ba_update_kernel(const BaArgs g) {
    const int tid = threadIdx.x, pt = tid / 16, lane = tid % 16, V = g.V;
    const long long p = (long long)blockIdx.x * kBaPts + pt;
    if (g.cams_new && blockIdx.x == 0 && tid < V) {
        const double* cam = g.cams + (size_t)tid * kCamRow;
        const double* d = g.dc + (size_t)tid * 6;
        double* out = g.cams_new + (size_t)tid * kCamRow;
        double dR[9], Rn[9];
        rodrigues64(d, dR);
        mat_mul64(dR, cam, Rn);
        for (int k = 0; k < 9; ++k) out[k] = Rn[k];
        for (int k = 0; k < 3; ++k) out[9 + k] = cam[9 + k] + d[3 + k];
        for (int k = 12; k < kCamRow; ++k) out[k] = cam[k];
    }
    BaLane o;
    ba_lane(g, p, lane, o);
    double rhs[3];
    const double* d = g.dc + (size_t)(lane < V ? lane : 0) * 6;
#pragma unroll
    for (int a = 0; a < 3; ++a) {
        double s = 0.0;
#pragma unroll
        for (int i = 0; i < 6; ++i) s += o.w * (o.jc[0][i] * o.jx[0][a] + o.jc[1][i] * o.jx[1][a]) * d[i];
        rhs[a] = o.gp[a] + lanes_sum<16>(s);
    }
    if (lane == 0 && p < g.P) {
        const bool moves = o.inside && o.seen;       // any other point passes through as given
        double dX[3] = {0.0, 0.0, 0.0};
        if (moves) cam_solve3(o.Hd, rhs, dX);
#pragma unroll
        for (int k = 0; k < 3; ++k) {
            const double x = g.points[(size_t)p * 3 + k];
            g.points_new[(size_t)p * 3 + k] = moves ? x - dX[k] : x;
        }
    }
}

static int rig_check(const char* who, int V, int N, int J, double conf_min) {
    if (int rc = views_check_shape(who, V, 2, N, 1, J)) return rc;
    return views_check_conf(who, conf_min);
}

struct BaPlan { int tiles, tiles_per_group, groups, n_tasks, stride; };

static BaPlan ba_plan(int V, long long P) {
    BaPlan b;
    b.tiles = (int)((P + kBaPts - 1) / kBaPts);
    b.tiles_per_group = (b.tiles + kBaMaxGroups - 1) / kBaMaxGroups;
    b.groups = (b.tiles + b.tiles_per_group - 1) / b.tiles_per_group;
    b.n_tasks = 6 * (V * (V + 1) / 2);
    b.stride = b.n_tasks * 6 + 6 * V + kBaCam * V;
    return b;
}

int rig_undistort(const float* keypoints, const double* cams, int V, long long P, double conf_min, void* ws, hipStream_t stream) {
    const long long total = (long long)V * P;
    hipLaunchKernelGGL(rig_undistort_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, stream, keypoints, cams, P, total, conf_min,
                       (double*)ws);
    ROHM_LAUNCH_CHECK();
    return ROHM_OK;
}

}  // namespace rohm

using namespace rohm;

extern "C" long long rohm_rig_pair_ws_bytes(int V, long long P) {
    if (int rc = views_check_ws("rig_pair_ws_bytes", V, P)) return rc;
    return (long long)V * P * 16;
}

extern "C" long long rohm_rig_ba_ws_bytes(int V, long long P) {
    if (int rc = views_check_ws("rig_ba_ws_bytes", V, P)) return rc;
    const BaPlan b = ba_plan(V, P);
    return (long long)b.groups * b.stride * 8;
}

extern "C" int rohm_rig_pair_hypotheses(const float* keypoints, const double* cams, const int* pairs, const int* samples, int V, int N, int J,
                                        int Q, int K, double conf_min, double tau_px, void* ws, double* E, long long* counts, int* best,
                                        rohm_stream_t stream) {
    if (int rc = rig_check("rig_pair_hypotheses", V, N, J, conf_min)) return rc;
    ROHM_ARG_CHECK(Q >= 0, "rig_pair_hypotheses: Q must be >= 0, got %d", Q);
    ROHM_ARG_CHECK(K >= 1, "rig_pair_hypotheses: K must be >= 1, got %d", K);
    ROHM_ARG_CHECK((long long)Q * K <= kRigMaxHyp, "rig_pair_hypotheses: Q * K must not exceed %lld, got %lld", kRigMaxHyp, (long long)Q * K);
    ROHM_ARG_CHECK(Q <= 65535, "rig_pair_hypotheses: Q must not exceed 65535, got %d", Q);
    ROHM_ARG_CHECK(isfinite(tau_px) && tau_px > 0.0, "rig_pair_hypotheses: tau_px must be finite and > 0, got %g", tau_px);
    if (Q == 0) return ROHM_OK;
    ROHM_ARG_CHECK(keypoints, "rig_pair_hypotheses: keypoints is null");
    ROHM_ARG_CHECK(cams, "rig_pair_hypotheses: cams is null");
    ROHM_ARG_CHECK(pairs, "rig_pair_hypotheses: pairs is null");
    ROHM_ARG_CHECK(samples, "rig_pair_hypotheses: samples is null");
    ROHM_ARG_CHECK(ws, "rig_pair_hypotheses: ws is null");
    ROHM_ARG_CHECK(E, "rig_pair_hypotheses: E is null");
    ROHM_ARG_CHECK(counts, "rig_pair_hypotheses: counts is null");
    ROHM_ARG_CHECK(best, "rig_pair_hypotheses: best is null");
    const long long P = (long long)N * J;
    prof::Scope ps("rig_pair_hypotheses", 40.0 * (double)Q * K * (double)P, 32.0 * (double)Q * ((K + kRigHypPerBlock - 1) / kRigHypPerBlock) * (double)P,
                   (hipStream_t)stream);
    if (int rc = rig_undistort(keypoints, cams, V, P, conf_min, ws, (hipStream_t)stream)) return rc;
    RigHypArgs a;
    a.und = (const double*)ws; a.cams = cams; a.pairs = pairs; a.samples = samples; a.V = V; a.K = K; a.P = P; a.tau2 = tau_px * tau_px;
    a.E = E; a.counts = counts;
    hipLaunchKernelGGL(rig_hypotheses_kernel, dim3((unsigned)((K + kRigHypPerBlock - 1) / kRigHypPerBlock), (unsigned)Q), dim3(kRigThreads), 0,
                       (hipStream_t)stream, a);
    ROHM_LAUNCH_CHECK();
    // a degenerate hypothesis counts -1: all of a pair's degenerate gives -1
    hipLaunchKernelGGL((best_score_kernel<kRigPickThreads, 2, 0ll>), dim3((unsigned)Q), dim3(kRigPickThreads), 0, (hipStream_t)stream, counts, K, best);
    ROHM_LAUNCH_CHECK();
    return ROHM_OK;
}

extern "C" int rohm_rig_pair_moments(const float* keypoints, const double* cams, const int* pairs, const double* E, int V, int N, int J, int Q,
                                     double conf_min, double tau_px, void* ws, double* moments, rohm_stream_t stream) {
    if (int rc = rig_check("rig_pair_moments", V, N, J, conf_min)) return rc;
    ROHM_ARG_CHECK(Q >= 0, "rig_pair_moments: Q must be >= 0, got %d", Q);
    ROHM_ARG_CHECK(isfinite(tau_px) && tau_px > 0.0, "rig_pair_moments: tau_px must be finite and > 0, got %g", tau_px);
    if (Q == 0) return ROHM_OK;
    ROHM_ARG_CHECK(keypoints, "rig_pair_moments: keypoints is null");
    ROHM_ARG_CHECK(cams, "rig_pair_moments: cams is null");
    ROHM_ARG_CHECK(pairs, "rig_pair_moments: pairs is null");
    ROHM_ARG_CHECK(E, "rig_pair_moments: E is null");
    ROHM_ARG_CHECK(ws, "rig_pair_moments: ws is null");
    ROHM_ARG_CHECK(moments, "rig_pair_moments: moments is null");
    const long long P = (long long)N * J;
    prof::Scope ps("rig_pair_moments", 0.0, 32.0 * (double)Q * (double)P, (hipStream_t)stream);
    if (int rc = rig_undistort(keypoints, cams, V, P, conf_min, ws, (hipStream_t)stream)) return rc;
    hipLaunchKernelGGL(rig_moments_kernel, dim3((unsigned)Q), dim3(kRigMomThreads), 0, (hipStream_t)stream, (const double*)ws, cams, pairs, E, V, P,
                       tau_px * tau_px, moments);
    ROHM_LAUNCH_CHECK();
    return ROHM_OK;
}

static int ba_check(const char* who, int V, int N, int J, double conf_min, double sigma_px, double lambda) {
    if (int rc = rig_check(who, V, N, J, conf_min)) return rc;
    ROHM_ARG_CHECK(isfinite(sigma_px) && sigma_px >= 0.0, "%s: sigma_px must be finite and >= 0, got %g", who, sigma_px);
    ROHM_ARG_CHECK(isfinite(lambda) && lambda >= 0.0, "%s: lambda must be finite and >= 0, got %g", who, lambda);
    return ROHM_OK;
}

extern "C" int rohm_rig_ba_moments(const float* keypoints, const double* cams, const double* points, int V, int N, int J, double conf_min,
                                   double sigma_px, double lambda, void* ws, double* S, double* r, double* stats, rohm_stream_t stream) {
    if (int rc = ba_check("rig_ba_moments", V, N, J, conf_min, sigma_px, lambda)) return rc;
    ROHM_ARG_CHECK(keypoints, "rig_ba_moments: keypoints is null");
    ROHM_ARG_CHECK(cams, "rig_ba_moments: cams is null");
    ROHM_ARG_CHECK(points, "rig_ba_moments: points is null");
    ROHM_ARG_CHECK(ws, "rig_ba_moments: ws is null");
    ROHM_ARG_CHECK(S, "rig_ba_moments: S is null");
    ROHM_ARG_CHECK(r, "rig_ba_moments: r is null");
    ROHM_ARG_CHECK(stats, "rig_ba_moments: stats is null");
    const long long P = (long long)N * J;
    const BaPlan b = ba_plan(V, P);
    BaArgs a = {};
    a.kp = keypoints; a.cams = cams; a.points = points; a.V = V; a.P = P; a.conf_min = conf_min; a.sigma2 = sigma_px * sigma_px; a.lambda = lambda;
    a.ws = (double*)ws; a.tiles = b.tiles; a.tiles_per_group = b.tiles_per_group; a.n_tasks = b.n_tasks; a.stride = b.stride;
    prof::Scope ps("rig_ba_moments", (double)P * (300.0 * V + 27.0 * b.n_tasks), (double)P * (12.0 * V + 24.0), (hipStream_t)stream);
    hipLaunchKernelGGL(rig_ba_moments_kernel, dim3((unsigned)b.groups), dim3(kRigThreads), 0, (hipStream_t)stream, a);
    ROHM_LAUNCH_CHECK();
    const int outputs = 36 * V * V + 6 * V + 2;
    hipLaunchKernelGGL(rig_ba_close_kernel, dim3((unsigned)((outputs + 255) / 256)), dim3(256), 0, (hipStream_t)stream, (const double*)ws, b.groups,
                       b.stride, b.n_tasks, V, lambda, S, r, stats);
    ROHM_LAUNCH_CHECK();
    return ROHM_OK;
}

extern "C" int rohm_rig_ba_update(const float* keypoints, const double* cams, const double* points, const double* dc, int V, int N, int J,
                                  double conf_min, double sigma_px, double lambda, double* points_new, double* cams_new, rohm_stream_t stream) {
    if (int rc = ba_check("rig_ba_update", V, N, J, conf_min, sigma_px, lambda)) return rc;
    ROHM_ARG_CHECK(keypoints, "rig_ba_update: keypoints is null");
    ROHM_ARG_CHECK(cams, "rig_ba_update: cams is null");
    ROHM_ARG_CHECK(points, "rig_ba_update: points is null");
    ROHM_ARG_CHECK(dc, "rig_ba_update: dc is null");
    ROHM_ARG_CHECK(points_new, "rig_ba_update: points_new is null");
    const long long P = (long long)N * J;
    BaArgs a = {};
    a.kp = keypoints; a.cams = cams; a.points = points; a.dc = dc; a.V = V; a.P = P; a.conf_min = conf_min; a.sigma2 = sigma_px * sigma_px;
    a.lambda = lambda; a.points_new = points_new; a.cams_new = cams_new;
    prof::Scope ps("rig_ba_update", (double)P * 300.0 * V, (double)P * (12.0 * V + 48.0), (hipStream_t)stream);
    hipLaunchKernelGGL(rig_ba_update_kernel, dim3((unsigned)((P + kBaPts - 1) / kBaPts)), dim3(kRigThreads), 0, (hipStream_t)stream, a);
    ROHM_LAUNCH_CHECK();
    return ROHM_OK;
}
