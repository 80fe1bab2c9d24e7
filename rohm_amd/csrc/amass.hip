// The AMASS training loader's own arithmetic on the device (data_loaders/dataloader_amass.py), next to clips.hip, which
// canonicalises the clips and computes their motion representation:
//   * rohm_smplx_param_noise: the SMPL-X parameter noise of :156-192 (Euler 'zxy' space for the 22 rotations) and the
//     plain additive noise of the sep_noise items (:298-303), float64 throughout like the reference's numpy / scipy;
//   * rohm_repr_stats: per-channel mean and population std of the clean representation (:254-258), float64 accumulation
//     in two deterministic stages;
//   * rohm_amass_batch: the item assembly of __getitem__ (:317-339) for a vector of item indices.
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
