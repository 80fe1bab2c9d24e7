// The AMASS training loader's own arithmetic on the device (data_loaders/dataloader_amass.py), next to clips.hip, which
// canonicalises the clips and computes their motion representation:
//   * rohm_smplx_param_noise: the SMPL-X parameter noise of :156-192 (Euler 'zxy' space for the 22 rotations) and the
//     plain additive noise of the sep_noise items (:298-303), float64 throughout like the reference's numpy / scipy;
//   * rohm_repr_stats: per-channel mean and population std of the clean representation (:254-258), float64 accumulation
//     in two deterministic stages;
//   * rohm_amass_batch: the item assembly of __getitem__ (:317-339) for a vector of item indices;
//   * rohm_amass_preprocess: the per-frame work of preprocessing_amass.py:47-69 (float32 cast, the 178-column parameter row
//     and joints 0..24 by joints-only FK) for the frames of many recordings in one launch.
// No float atomics anywhere: results are bitwise reproducible.
#include "common.h"
#include "rot_priv.h"
#include "smplx_fk.h"

namespace rohm {

constexpr int kParamCols = 79;                 // global_orient 3, transl 3, betas 10, body_pose 63
constexpr int kRots = 22;                      // global_orient + 21 body rotations
constexpr int kStatThreads = 320;              // >= C_TOTAL, a multiple of the wave size
constexpr int kStatMaxGroups = 1024;

// One thread per (frame, rotation); the thread of rotation 0 also adds the transl and betas noise of its frame.
__global__ __launch_bounds__(256) void param_noise_kernel(const double* __restrict__ params, const double* __restrict__ n_orient,
                                                          const double* __restrict__ n_transl, const double* __restrict__ n_betas,
                                                          const double* __restrict__ n_pose, long long M, int additive,
                                                          double* __restrict__ out) {
    const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= M * kRots) return;
    const long long m = i / kRots;
    const int r = (int)(i - m * kRots);
    const double* w = params + m * kParamCols;
    double* o = out + m * kParamCols;
    const int col = r == 0 ? 0 : 16 + (r - 1) * 3;
    const double* nz = r == 0 ? n_orient + m * 3 : n_pose + m * 63 + (r - 1) * 3;
    if (additive) {
#pragma unroll
        for (int k = 0; k < 3; ++k) o[col + k] = w[col + k] + nz[k];
    } else {
        double e[3], rv[3];
        rotvec_to_euler_zxy_deg_f64(w + col, e);
#pragma unroll
        for (int k = 0; k < 3; ++k) e[k] += nz[k];
        euler_zxy_deg_to_rotvec_f64(e, rv);
#pragma unroll
        for (int k = 0; k < 3; ++k) o[col + k] = rv[k];
    }
    if (r == 0) {
#pragma unroll
        for (int k = 0; k < 3; ++k) o[3 + k] = w[3 + k] + n_transl[m * 3 + k];
#pragma unroll
        for (int k = 0; k < NBETA; ++k) o[6 + k] = w[6 + k] + n_betas[m * NBETA + k];
    }
}

// Stage 1: workgroup g takes rows [g * per, min(rows, (g + 1) * per)), thread ch one channel: the mean of its rows, then the
// sum of squared deviations from that mean.  partial [G, 2, 294].
__global__ __launch_bounds__(kStatThreads) void repr_stats_partial_kernel(const float* __restrict__ x, long long rows, long long per,
                                                                          double* __restrict__ partial) {
    const int ch = threadIdx.x;
    if (ch >= C_TOTAL) return;
    const long long r0 = (long long)blockIdx.x * per, r1 = (r0 + per < rows) ? r0 + per : rows;
    double s = 0.0;
    for (long long r = r0; r < r1; ++r) s += (double)x[r * C_TOTAL + ch];
    const double mean = s / (double)(r1 - r0);
    double m2 = 0.0;
    for (long long r = r0; r < r1; ++r) {
        const double d = (double)x[r * C_TOTAL + ch] - mean;
        m2 += d * d;
    }
    partial[((size_t)blockIdx.x * 2) * C_TOTAL + ch] = mean;
    partial[((size_t)blockIdx.x * 2 + 1) * C_TOTAL + ch] = m2;
}

// Stage 2: one workgroup folds the partials in their order (Chan et al.'s pairwise update).
__global__ __launch_bounds__(kStatThreads) void repr_stats_combine_kernel(const double* __restrict__ partial, int G, long long rows,
                                                                          long long per, double* __restrict__ mean_out,
                                                                          double* __restrict__ std_out) {
    const int ch = threadIdx.x;
    if (ch >= C_TOTAL) return;
    double n = 0.0, mean = 0.0, m2 = 0.0;
    for (int g = 0; g < G; ++g) {
        const long long e = (long long)(g + 1) * per;
        const double nb = (double)((e < rows ? e : rows) - (long long)g * per);
        const double mb = partial[((size_t)g * 2) * C_TOTAL + ch], m2b = partial[((size_t)g * 2 + 1) * C_TOTAL + ch];
        const double d = mb - mean, nn = n + nb;
        mean += d * (nb / nn);
        m2 += m2b + d * d * (n * nb / nn);
        n = nn;
    }
    mean_out[ch] = mean;
    std_out[ch] = sqrt(m2 / n);
}

struct BatchArgs {
    const float* clean;       // [n, R, 294]
    const float* noisy;       // [n, R, 294] ([B, R, 294] with noisy_per_batch) or null (input_noise = False)
    const long long* index;   // [B]
    long long n;
    int R, B;
    const float* mean;
    const float* stdv;
    int overwrite;            // task 'pose': the first `overwrite` noisy channels are the clean ones
    int noisy_per_batch;      // row b of `noisy` belongs to batch entry b (the sep_noise items, made per batch)
    int cond_kind;            // 0: none, 1: the first 22 channels, 2: the 13 absolute trajectory channels
    float* out_clean;         // [B, R, 294]
    float* out_noisy;         // [B, R, 294]
    float* cond;              // [B, R, 22 | 13] or null
    float* control;           // [B, R, 272] or null
};

__constant__ int kAbsTrajCh[13] = {0, 2, 3, 6, 7, 8, 9, 10, 11, 12, 16, 17, 18};

// One thread per (item, frame, channel).  An index outside [0, n) gives NaN rows, never a read outside the arrays.
__global__ __launch_bounds__(256) void amass_batch_kernel(const BatchArgs a) {
    const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= (long long)a.B * a.R * C_TOTAL) return;
    const int ch = (int)(i % C_TOTAL);
    const long long bt = i / C_TOTAL;
    const long long b = bt / a.R, t = bt - b * a.R;
    const long long src = a.index[b];
    float vc, vn;
    if (src < 0 || src >= a.n) {
        vc = vn = __builtin_nanf("");
    } else {
        const long long at = (src * a.R + t) * C_TOTAL + ch;
        const double m = (double)a.mean[ch], s = (double)a.stdv[ch];
        const float c = a.clean[at];
        const float z = (a.noisy && ch >= a.overwrite) ? a.noisy[a.noisy_per_batch ? i : at] : c;
        vc = (float)(((double)c - m) / s);
        vn = (float)(((double)z - m) / s);
    }
    a.out_clean[i] = vc;
    a.out_noisy[i] = vn;
    if (a.cond_kind == 1) {
        if (ch < 22) a.cond[bt * 22 + ch] = vn;
    } else if (a.cond_kind == 2) {
#pragma unroll
        for (int k = 0; k < 13; ++k)
            if (kAbsTrajCh[k] == ch) a.cond[bt * 13 + k] = vn;
    }
    if (a.control && ch >= C_TOTAL - 272) a.control[bt * 272 + (ch - (C_TOTAL - 272))] = vc;
}

static int stat_groups(long long rows, long long* per) {
    long long p = 64;                                         // rows per workgroup, grown until the groups fit
    while ((rows + p - 1) / p > kStatMaxGroups) p *= 2;
    *per = p;
    return (int)((rows + p - 1) / p);
}

// ---- raw AMASS -> the 30 fps trees (preprocessing_amass.py:47-69) -----------------------------------------------------
constexpr int kRawCols = 178;                  // root_orient 3, trans 3, betas 10, pose_body 63, pose_hand 90, pose_jaw 3, eye 3, eye 3
constexpr int kRawJoints = 25;                 // 22 body joints + jaw, left eye, right eye (leaves: positions from the parent's transform)
constexpr int kRawFrames = 128;                // frames per workgroup = one lane each for the FK

struct RawArgs {
    const double *root_orient, *trans, *pose_body, *pose_hand, *pose_jaw, *pose_eye, *betas;
    const int32_t* rec_of_frame;
    int N, R;
    const float *Jt, *Js;
    const int* parents;
    float *joints, *params;
};

// The eight runs of columns of a parameter row: source array, its row length, the run's first column (both eye runs are
// pose_eye[:, 0:3], preprocessing_amass.py:54-55).  Kept in LDS and indexed per element, so that the copy loop has no branch
// between its loads.
typedef const double __attribute__((address_space(1))) * RawPtr;      // still a global-memory pointer after a trip through LDS
struct RawSeg { RawPtr base; int width, col0; };

__device__ __forceinline__ void raw_segments(const RawArgs& a, RawSeg* s) {
    s[0] = {(RawPtr)a.root_orient, 3, 0};
    s[1] = {(RawPtr)a.trans, 3, 3};
    s[2] = {(RawPtr)a.betas, NBETA, 6};
    s[3] = {(RawPtr)a.pose_body, 63, 16};
    s[4] = {(RawPtr)a.pose_hand, 90, 79};
    s[5] = {(RawPtr)a.pose_jaw, 3, 169};
    s[6] = {(RawPtr)a.pose_eye, 6, 172};
    s[7] = {(RawPtr)a.pose_eye, 6, 175};
}

// Address of column c of the parameter row of frame n, whose recording is `rec`.  An index outside [0, R) reads betas[0] and is
// replaced by NaN afterwards (`bad`): never a read outside the arrays.
__device__ __forceinline__ RawPtr raw_source(const RawSeg* segs, int R, size_t n, int c, int rec, bool& bad) {
    const int k = (c >= 3) + (c >= 6) + (c >= 16) + (c >= 79) + (c >= 169) + (c >= 172) + (c >= 175);
    const RawSeg s = segs[k];
    bad = k == 2 && (rec < 0 || rec >= R);
    const size_t row = k == 2 ? (size_t)(bad ? 0 : rec) : n;
    return s.base + row * s.width + (c - s.col0);
}

constexpr int kRawBatch = 8;                   // loads a lane has in flight in the copy phase

// One workgroup = two waves = 128 consecutive frames.  Phase 1: the lanes walk the workgroup's [frames, 178] block of the row-major
// output in order (consecutive lanes on consecutive floats: whole-line stores, and loads that are consecutive within each source
// array), eight elements per lane at a time, cast float64 -> float32 (round to nearest even, as torch.Tensor(ndarray)) and keep the
// 79 columns the FK reads in LDS (row stride 79, odd: lane-per-row reads are conflict free).  Phase 2: one lane per frame runs the
// chain of rohm_smplx_joints (the same device functions) on the cast values and adds the three leaf joints.
__global__ __launch_bounds__(kRawFrames) void amass_preprocess_kernel(const RawArgs a) {
    __shared__ float rows[kRawFrames * kParamCols];
    __shared__ int recs[kRawFrames];
    __shared__ RawSeg segs[8];
    if (threadIdx.x == 0) raw_segments(a, segs);
    const size_t n0 = (size_t)blockIdx.x * kRawFrames;
    const int nf = (a.N - (long long)n0 < kRawFrames) ? (int)(a.N - (long long)n0) : kRawFrames;
    if ((int)threadIdx.x < nf) recs[threadIdx.x] = a.rec_of_frame[n0 + threadIdx.x];
    __syncthreads();
    const int total = nf * kRawCols;
    for (int base = threadIdx.x; base < total; base += kRawBatch * kRawFrames) {
        double v[kRawBatch];
        bool bad[kRawBatch];
#pragma unroll
        for (int u = 0; u < kRawBatch; ++u) {
            const int idx = min(base + u * kRawFrames, total - 1);      // past the end: a valid address, the value is dropped
            const int fl = idx / kRawCols;
            v[u] = *raw_source(segs, a.R, n0 + fl, idx - fl * kRawCols, recs[fl], bad[u]);
        }
#pragma unroll
        for (int u = 0; u < kRawBatch; ++u) {
            const int idx = base + u * kRawFrames;
            if (idx < total) {
                const int fl = idx / kRawCols, c = idx - fl * kRawCols;
                const float x = bad[u] ? __builtin_nanf("") : (float)v[u];
                a.params[n0 * kRawCols + idx] = x;
                if (c < kParamCols) rows[fl * kParamCols + c] = x;
            }
        }
    }
    __syncthreads();
    if ((int)threadIdx.x >= nf) return;
    const float* w = rows + threadIdx.x * kParamCols;
    const size_t n = n0 + threadIdx.x;
    FkCtx f;
    for (int j = 0; j < NJ; ++j) {
        const int col = j == 0 ? 0 : 16 + (j - 1) * 3;
        const float r[3] = {w[col], w[col + 1], w[col + 2]};
        rodrigues(r, f.R[j]);
    }
    float beta[NBETA];
    for (int k = 0; k < NBETA; ++k) beta[k] = w[6 + k];
    rest_joints(a.Jt, a.Js, beta, f.Jr);
    fk_forward(f, a.parents);
    const float t[3] = {w[3], w[4], w[5]};
    float* out = a.joints + n * kRawJoints * 3;
    for (int j = 0; j < NJ; ++j)
#pragma unroll
        for (int c = 0; c < 3; ++c) out[j * 3 + c] = f.P[j][c] + t[c];
    // joints 22..24: P[j] = P[p] + G[p] (Jr[j] - Jr[p]); their own rotations turn nothing that is read
    for (int j = NJ; j < kRawJoints; ++j) {
        const int p = a.parents[j];
        float off[3], wv[3];
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            float v = a.Jt[j * 3 + c];
#pragma unroll
            for (int k = 0; k < NBETA; ++k) v = fmaf(a.Js[(j * 3 + c) * NBETA + k], beta[k], v);
            off[c] = v - f.Jr[p][c];
        }
        mat_vec(f.G[p], off, wv);
#pragma unroll
        for (int c = 0; c < 3; ++c) out[j * 3 + c] = f.P[p][c] + wv[c] + t[c];
    }
}

}  // namespace rohm

using namespace rohm;

extern "C" int rohm_smplx_param_noise(const double* params, const double* noise_orient, const double* noise_transl,
                                      const double* noise_betas, const double* noise_pose, long long M, int additive,
                                      double* out, rohm_stream_t stream) {
    ROHM_ARG_CHECK(M >= 0 && M <= (1ll << 40), "smplx_param_noise: bad frame count");
    if (M == 0) return ROHM_OK;
    ROHM_ARG_CHECK(params && noise_orient && noise_transl && noise_betas && noise_pose && out, "smplx_param_noise: null argument");
    ROHM_ARG_CHECK(params != out, "smplx_param_noise: out must not alias params");
    const long long total = M * kRots;
    ROHM_ARG_CHECK((total + 255) / 256 <= 0x7fffffffll, "smplx_param_noise: too many frames for one launch");
    prof::Scope ps("smplx_param_noise", 0.0, 8.0 * 3 * kParamCols * (double)M, (hipStream_t)stream);
    hipLaunchKernelGGL(param_noise_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, (hipStream_t)stream, params,
                       noise_orient, noise_transl, noise_betas, noise_pose, M, additive, out);
    ROHM_LAUNCH_CHECK();
    return ROHM_OK;
}

extern "C" size_t rohm_repr_stats_scratch_bytes(long long rows) {
    if (rows <= 0) return 0;
    long long per;
    return (size_t)stat_groups(rows, &per) * 2 * C_TOTAL * sizeof(double);
}

extern "C" int rohm_repr_stats(const float* repr, long long rows, double* mean294, double* std294, void* scratch,
                               size_t scratch_bytes, rohm_stream_t stream) {
    ROHM_ARG_CHECK(rows >= 1, "repr_stats: need at least one row (got %lld)", rows);
    ROHM_ARG_CHECK(repr && mean294 && std294, "repr_stats: null argument");
    const size_t need = rohm_repr_stats_scratch_bytes(rows);
    ROHM_ARG_CHECK(scratch && scratch_bytes >= need, "repr_stats: scratch too small (%zu < %zu)", scratch_bytes, need);
    long long per;
    const int G = stat_groups(rows, &per);
    prof::Scope ps("repr_stats", 0.0, 8.0 * C_TOTAL * (double)rows, (hipStream_t)stream);
    hipLaunchKernelGGL(repr_stats_partial_kernel, dim3(G), dim3(kStatThreads), 0, (hipStream_t)stream, repr, rows, per,
                       static_cast<double*>(scratch));
    ROHM_LAUNCH_CHECK();
    hipLaunchKernelGGL(repr_stats_combine_kernel, dim3(1), dim3(kStatThreads), 0, (hipStream_t)stream,
                       static_cast<const double*>(scratch), G, rows, per, mean294, std294);
    ROHM_LAUNCH_CHECK();
    return ROHM_OK;
}

extern "C" int rohm_amass_batch(const float* repr_clean, const float* repr_noisy, long long n_items, int rows_per_item,
                                const long long* index, int B, const float* mean294, const float* std294, int overwrite_channels,
                                int noisy_per_batch, int cond_kind, float* out_clean, float* out_noisy, float* cond, float* control_cond,
                                rohm_stream_t stream) {
    ROHM_ARG_CHECK(B >= 0 && n_items >= 0 && rows_per_item >= 1, "amass_batch: bad sizes (B=%d n=%lld rows=%d)", B, n_items,
                   rows_per_item);
    ROHM_ARG_CHECK(overwrite_channels >= 0 && overwrite_channels <= C_TOTAL, "amass_batch: overwrite_channels outside [0, 294]");
    ROHM_ARG_CHECK(cond_kind >= 0 && cond_kind <= 2, "amass_batch: cond_kind must be 0, 1 or 2");
    if (B == 0) return ROHM_OK;
    ROHM_ARG_CHECK(repr_clean && index && mean294 && std294 && out_clean && out_noisy, "amass_batch: null argument");
    ROHM_ARG_CHECK(cond_kind == 0 || cond, "amass_batch: cond_kind %d needs a cond buffer", cond_kind);
    const long long total = (long long)B * rows_per_item * C_TOTAL;
    ROHM_ARG_CHECK((total + 255) / 256 <= 0x7fffffffll, "amass_batch: batch too large for one launch");
    BatchArgs a;
    a.clean = repr_clean; a.noisy = repr_noisy; a.index = index; a.n = n_items; a.R = rows_per_item; a.B = B;
    a.mean = mean294; a.stdv = std294; a.overwrite = overwrite_channels; a.noisy_per_batch = noisy_per_batch; a.cond_kind = cond_kind;
    a.out_clean = out_clean; a.out_noisy = out_noisy; a.cond = cond; a.control = control_cond;
    prof::Scope ps("amass_batch", 0.0, 16.0 * (double)total, (hipStream_t)stream);
    hipLaunchKernelGGL(amass_batch_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, (hipStream_t)stream, a);
    ROHM_LAUNCH_CHECK();
    return ROHM_OK;
}

extern "C" int rohm_amass_preprocess(const rohm_smplx_t* h, const double* root_orient, const double* trans, const double* pose_body,
                                     const double* pose_hand, const double* pose_jaw, const double* pose_eye, const double* betas,
                                     const int32_t* rec_of_frame, int N, int R, float* joints, float* params, rohm_stream_t stream) {
    ROHM_ARG_CHECK(h, "amass_preprocess: null handle");
    ROHM_ARG_CHECK(h->J >= kRawJoints, "amass_preprocess: the body model has %d joints, joints 0..%d are needed", h->J, kRawJoints - 1);
    for (int j = NJ; j < kRawJoints; ++j)
        ROHM_ARG_CHECK(h->parents[j] >= 0 && h->parents[j] < NJ, "amass_preprocess: parents[%d] = %d is not one of the %d body joints", j,
                       h->parents[j], NJ);
    ROHM_ARG_CHECK(N >= 0 && R >= 0, "amass_preprocess: bad sizes (N=%d R=%d)", N, R);
    if (N == 0) return ROHM_OK;
    ROHM_ARG_CHECK(R >= 1, "amass_preprocess: %d frames but no recording", N);
    ROHM_ARG_CHECK(root_orient && trans && pose_body && pose_hand && pose_jaw && pose_eye && betas && rec_of_frame && joints && params,
                   "amass_preprocess: null argument");
    RawArgs a;
    a.root_orient = root_orient; a.trans = trans; a.pose_body = pose_body; a.pose_hand = pose_hand; a.pose_jaw = pose_jaw;
    a.pose_eye = pose_eye; a.betas = betas; a.rec_of_frame = rec_of_frame; a.N = N; a.R = R;
    a.Jt = h->d_Jt; a.Js = h->d_Js; a.parents = h->d_parents; a.joints = joints; a.params = params;
    prof::Scope ps("amass_preprocess", 0.0, (8.0 * 168 + 4.0 * (kRawCols + kRawJoints * 3 + 1)) * (double)N, (hipStream_t)stream);
    hipLaunchKernelGGL(amass_preprocess_kernel, dim3((unsigned)((N + kRawFrames - 1) / kRawFrames)), dim3(kRawFrames), 0,
                       (hipStream_t)stream, a);
    ROHM_LAUNCH_CHECK();
    return ROHM_OK;
}
