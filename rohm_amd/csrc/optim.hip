// The optimiser step of the training loops (train/training_loop_posenet.py:52-54,278: AdamW(...), self.opt.step()) and the global
// gradient norm / clip coefficient the reference lacks.
//   * rohm_adamw_step: torch.optim.AdamW (decoupled weight decay, no amsgrad; torch/optim/adam.py _single_tensor_adam, the
//     non-capturable branch, in its operation order) over a LIST of tensors.  The table (param, grad, exp_avg, exp_avg_sq, numel per
//     tensor) travels BY VALUE as the kernel argument, kChunk tensors per launch, so nothing the host rewrites next step is read by
//     a kernel still in flight.  A tensor is cut into blocks of kElems elements; the chunk carries the prefix sums of its tensors'
//     block counts and a block finds its tensor by bisection.
//   * rohm_grad_norm: sum of squares in double, two levels in a fixed order (thread -> block tree -> scratch; one finishing block
//     adds the scratch slots by index).  No atomics: the same inputs give the same bits.
// Streaming kernels: 16-byte loads and stores on the body of a block when every pointer of the tensor sits at the same offset from
// a 16-byte boundary (<= 3 scalar head elements bring them all onto it), scalar otherwise and on tails.  Vector stores only; nothing
// is allocated or synchronised; everything goes on the caller's stream.
#include <math.h>
#include "common.h"

namespace rohm {

constexpr int kChunk = 64;              // tensors per launch: 64 x (4 pointers + numel) + 65 prefix words = 2.8 KB of the 4 KB kernarg
constexpr int kThreads = 256;
constexpr int kElems = 4096;            // elements per block: 256 threads x 4 iterations x 16 bytes

struct AdamTable {
    float* p[kChunk]; const float* g[kChunk]; float* m[kChunk]; float* v[kChunk];
    long long numel[kChunk];
    int first_block[kChunk + 1];        // prefix sums of the tensors' block counts; first_block[n] = blocks of the launch
    int n;
    int has_decay;
    float decay, w1, beta2, w2, bc2_sqrt, step_size, eps;
    const float* coef;                  // device: the clip coefficient, or null
};

struct NormTable {
    const float* g[kChunk];
    long long numel[kChunk];
    int first_block[kChunk + 1];
    int n;
    double* partial;                    // this launch's first slot
};

// The tensor of block b: the last t with first_block[t] <= b.
template <typename Table>
__device__ __forceinline__ int find_tensor(const Table& a, int b) {
    int lo = 0, hi = a.n - 1;
    while (lo < hi) {
        const int mid = (lo + hi + 1) >> 1;
        if (a.first_block[mid] <= b) lo = mid; else hi = mid - 1;
    }
    return lo;
}

__device__ __forceinline__ unsigned quad_offset(const void* p) { return (unsigned)(((uintptr_t)p >> 2) & 3u); }

struct AdamScalars { float decay, w1, beta2, w2, bc2_sqrt, step_size, eps, coef; bool has_decay, has_coef; };

__device__ __forceinline__ void adam_one(const AdamScalars& s, float& p, float g, float& m, float& v) {
    if (s.has_decay) p *= s.decay;                            // param.mul_(1 - lr * weight_decay)
    if (s.has_coef) g = __fmul_rn(g, s.coef);                 // rounded on its own: a coefficient of 1 leaves the step's bits alone
    m = m + s.w1 * (g - m);                                   // exp_avg.lerp_(grad, 1 - beta1), weight < 0.5
    v = v * s.beta2 + s.w2 * g * g;                           // exp_avg_sq.mul_(beta2).addcmul_(grad, grad, value=1 - beta2)
    const float denom = sqrtf(v) / s.bc2_sqrt + s.eps;        // (exp_avg_sq.sqrt() / bias_correction2_sqrt).add_(eps)
    p = p - s.step_size * m / denom;                          // param.addcdiv_(exp_avg, denom, value=-step_size)
}

__global__ __launch_bounds__(kThreads) void adamw_kernel(AdamTable a) {
    const int b = blockIdx.x;
    const int t = find_tensor(a, b);
    const long long start = (long long)(b - a.first_block[t]) * kElems;
    const long long left = a.numel[t] - start;
    const int len = left < kElems ? (int)left : kElems;
    float* __restrict__ p = a.p[t] + start;
    const float* __restrict__ g = a.g[t] + start;
    float* __restrict__ m = a.m[t] + start;
    float* __restrict__ v = a.v[t] + start;

    AdamScalars s;
    s.decay = a.decay; s.w1 = a.w1; s.beta2 = a.beta2; s.w2 = a.w2; s.bc2_sqrt = a.bc2_sqrt; s.step_size = a.step_size; s.eps = a.eps;
    s.has_decay = a.has_decay != 0; s.has_coef = a.coef != nullptr;
    s.coef = s.has_coef ? *a.coef : 1.0f;

    // kElems is a multiple of 4, so a block's pointers keep their tensor's offsets from a 16-byte boundary
    const unsigned off = quad_offset(p);
    const bool vec = off == quad_offset(g) && off == quad_offset(m) && off == quad_offset(v);
    int head = vec ? (int)((4u - off) & 3u) : len;
    if (head > len) head = len;
    const int nvec = (len - head) >> 2;
    const int tail0 = head + (nvec << 2);

    f32x4* __restrict__ p4 = reinterpret_cast<f32x4*>(p + head);
    const f32x4* __restrict__ g4 = reinterpret_cast<const f32x4*>(g + head);
    f32x4* __restrict__ m4 = reinterpret_cast<f32x4*>(m + head);
    f32x4* __restrict__ v4 = reinterpret_cast<f32x4*>(v + head);
#pragma unroll 4
    for (int i = threadIdx.x; i < nvec; i += kThreads) {
        f32x4 pp = p4[i], mm = m4[i], vv = v4[i];
        const f32x4 gg = g4[i];
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            float pk = pp[k], mk = mm[k], vk = vv[k];
            adam_one(s, pk, gg[k], mk, vk);
            pp[k] = pk; mm[k] = mk; vv[k] = vk;
        }
        p4[i] = pp; m4[i] = mm; v4[i] = vv;
    }
    // scalar head [0, head) and tail [tail0, len): at most 3 + 3 elements of a vector block, the whole block of a scalar one
    for (int i = threadIdx.x; i < head + (len - tail0); i += kThreads) {
        const int e = i < head ? i : tail0 + (i - head);
        float pk = p[e], mk = m[e], vk = v[e];
        adam_one(s, pk, g[e], mk, vk);
        p[e] = pk; m[e] = mk; v[e] = vk;
    }
}

// Sum over the block, every thread contributing `x`; the result is valid in thread 0.  A fixed tree: lanes by shuffle, waves in order.
__device__ __forceinline__ double block_sum(double x) {
    __shared__ double wave_part[kThreads / 64];
    for (int o = 32; o; o >>= 1) x += __shfl_down(x, o, 64);
    if ((threadIdx.x & 63) == 0) wave_part[threadIdx.x >> 6] = x;
    __syncthreads();
    double sum = 0.0;
    if (threadIdx.x == 0)
        for (int w = 0; w < kThreads / 64; ++w) sum += wave_part[w];
    return sum;
}

__global__ __launch_bounds__(kThreads) void grad_sumsq_kernel(NormTable a) {
    const int b = blockIdx.x;
    const int t = find_tensor(a, b);
    const long long start = (long long)(b - a.first_block[t]) * kElems;
    const long long left = a.numel[t] - start;
    const int len = left < kElems ? (int)left : kElems;
    const float* __restrict__ g = a.g[t] + start;
    int head = (int)((4u - quad_offset(g)) & 3u);
    if (head > len) head = len;
    const int nvec = (len - head) >> 2;
    const int tail0 = head + (nvec << 2);
    const f32x4* __restrict__ g4 = reinterpret_cast<const f32x4*>(g + head);
    double acc = 0.0;
#pragma unroll 4
    for (int i = threadIdx.x; i < nvec; i += kThreads) {
        const f32x4 gg = g4[i];
#pragma unroll
        for (int k = 0; k < 4; ++k) acc += (double)gg[k] * (double)gg[k];
    }
    for (int i = threadIdx.x; i < head + (len - tail0); i += kThreads) {
        const int e = i < head ? i : tail0 + (i - head);
        acc += (double)g[e] * (double)g[e];
    }
    const double sum = block_sum(acc);
    if (threadIdx.x == 0) a.partial[b] = sum;
}

// out[0] = total_norm, out[1] = min(1, max_norm / (total_norm + 1e-6)): torch.nn.utils.clip_grad_norm_'s coefficient (a NaN norm
// gives a NaN coefficient, an infinite one 0, as torch's clamp does with error_if_nonfinite=False).
__global__ __launch_bounds__(kThreads) void grad_norm_finish_kernel(const double* __restrict__ partial, int n, float max_norm,
                                                                    float* __restrict__ out) {
    double acc = 0.0;
    for (int i = threadIdx.x; i < n; i += kThreads) acc += partial[i];
    const double sum = block_sum(acc);
    if (threadIdx.x == 0) {
        const float norm = (float)sqrt(sum);
        const float c = max_norm / (norm + 1e-6f);
        f32x2 r;
        r[0] = norm;
        r[1] = c > 1.0f ? 1.0f : c;
        *reinterpret_cast<f32x2*>(out) = r;
    }
}

constexpr long long kMaxBlocks = 1ll << 24;      // per launch: HIP refuses a grid of 2^32 threads or more
static long long blocks_of(long long numel) { return (numel + kElems - 1) / kElems; }

}  // namespace rohm

using namespace rohm;

extern "C" int rohm_adamw_limits(int* tensors_per_launch, int* elems_per_block) {
    if (tensors_per_launch) *tensors_per_launch = kChunk;
    if (elems_per_block) *elems_per_block = kElems;
    return ROHM_OK;
}

extern "C" int rohm_adamw_step(float* const* params, const float* const* grads, float* const* exp_avg, float* const* exp_avg_sq,
                               const long long* numel, int n_tensors, double lr, double beta1, double beta2, double eps,
                               double weight_decay, long long step, const float* clip_coef, rohm_stream_t stream) {
    static_assert(sizeof(AdamTable) <= 4096, "the table must fit the kernel argument segment");
    ROHM_ARG_CHECK(n_tensors >= 0, "adamw_step: negative tensor count (%d)", n_tensors);
    ROHM_ARG_CHECK(step >= 1, "adamw_step: step=%lld, the first step is 1", step);
    ROHM_ARG_CHECK(lr >= 0.0 && eps >= 0.0 && weight_decay >= 0.0, "adamw_step: lr, eps and weight_decay must not be negative");
    ROHM_ARG_CHECK(beta1 >= 0.0 && beta1 < 1.0 && beta2 >= 0.0 && beta2 < 1.0, "adamw_step: betas must lie in [0, 1)");
    // the lerp form below is torch's for a weight under 0.5
    ROHM_ARG_CHECK(1.0 - beta1 < 0.5, "adamw_step: beta1=%g: only beta1 > 0.5 is supported", beta1);
    if (n_tensors == 0) return ROHM_OK;
    ROHM_ARG_CHECK(params && grads && exp_avg && exp_avg_sq && numel, "adamw_step: null table");
    for (int i = 0; i < n_tensors; ++i) {
        ROHM_ARG_CHECK(numel[i] >= 0, "adamw_step: tensor %d has numel %lld", i, numel[i]);
        ROHM_ARG_CHECK(numel[i] == 0 || (params[i] && grads[i] && exp_avg[i] && exp_avg_sq[i]), "adamw_step: tensor %d has a null pointer", i);
        ROHM_ARG_CHECK(((uintptr_t)params[i] | (uintptr_t)grads[i] | (uintptr_t)exp_avg[i] | (uintptr_t)exp_avg_sq[i]) % 4 == 0,
                       "adamw_step: tensor %d is not 4-byte aligned", i);
    }
    AdamTable a;
    // the scalars in double, converted to float once, as torch passes its Python floats to the fp32 kernels
    a.has_decay = weight_decay != 0.0;
    a.decay = (float)(1.0 - lr * weight_decay);
    a.w1 = (float)(1.0 - beta1);
    a.beta2 = (float)beta2;
    a.w2 = (float)(1.0 - beta2);
    a.bc2_sqrt = (float)sqrt(1.0 - pow(beta2, (double)step));
    a.step_size = (float)(lr / (1.0 - pow(beta1, (double)step)));
    a.eps = (float)eps;
    a.coef = clip_coef;
    int i = 0;
    while (i < n_tensors) {
        long long blocks = 0;
        int n = 0;
        for (; i < n_tensors && n < kChunk; ++i) {
            if (numel[i] == 0) continue;
            const long long nb = blocks_of(numel[i]);
            if (blocks + nb > kMaxBlocks) {
                ROHM_ARG_CHECK(n > 0, "adamw_step: tensor %d is too large for one launch", i);
                break;
            }
            a.p[n] = params[i]; a.g[n] = grads[i]; a.m[n] = exp_avg[i]; a.v[n] = exp_avg_sq[i]; a.numel[n] = numel[i];
            a.first_block[n] = (int)blocks;
            blocks += nb;
            ++n;
        }
        if (n == 0) continue;
        a.first_block[n] = (int)blocks;
        a.n = n;
        long long elems = 0;
        for (int k = 0; k < n; ++k) elems += a.numel[k];
        prof::Scope ps("adamw_step", 12.0 * (double)elems, 28.0 * (double)elems, (hipStream_t)stream);
        hipLaunchKernelGGL(adamw_kernel, dim3((unsigned)blocks), dim3(kThreads), 0, (hipStream_t)stream, a);
        ROHM_LAUNCH_CHECK();
    }
    return ROHM_OK;
}

extern "C" size_t rohm_grad_norm_scratch_bytes(long long total_elems, int n_tensors) {
    if (total_elems < 0 || n_tensors < 0) return 0;
    // every tensor rounds its block count up at most once
    return (size_t)(total_elems / kElems + n_tensors + 1) * sizeof(double);
}

extern "C" int rohm_grad_norm(const float* const* grads, const long long* numel, int n_tensors, float max_norm, float* out,
                              void* scratch, size_t scratch_bytes, rohm_stream_t stream) {
    static_assert(sizeof(NormTable) <= 4096, "the table must fit the kernel argument segment");
    ROHM_ARG_CHECK(n_tensors >= 0, "grad_norm: negative tensor count (%d)", n_tensors);
    ROHM_ARG_CHECK(out && (uintptr_t)out % 8 == 0, "grad_norm: out must be an 8-byte aligned device pointer to two floats");
    ROHM_ARG_CHECK(max_norm >= 0.0f || max_norm != max_norm, "grad_norm: max_norm=%g is negative", (double)max_norm);
    ROHM_ARG_CHECK(n_tensors == 0 || (grads && numel), "grad_norm: null table");
    long long total_blocks = 0;
    for (int i = 0; i < n_tensors; ++i) {
        ROHM_ARG_CHECK(numel[i] >= 0, "grad_norm: tensor %d has numel %lld", i, numel[i]);
        ROHM_ARG_CHECK(numel[i] == 0 || grads[i], "grad_norm: tensor %d has a null pointer", i);
        ROHM_ARG_CHECK((uintptr_t)grads[i] % 4 == 0, "grad_norm: tensor %d is not 4-byte aligned", i);
        total_blocks += blocks_of(numel[i]);
    }
    ROHM_ARG_CHECK(total_blocks <= 0x7fffffffll, "grad_norm: too many elements for one call");
    if (total_blocks > 0) {
        ROHM_ARG_CHECK(scratch && (uintptr_t)scratch % 8 == 0, "grad_norm: scratch must be an 8-byte aligned device pointer");
        if (scratch_bytes < (size_t)total_blocks * sizeof(double)) {
            set_error("grad_norm: scratch of %zu bytes, %zu needed", scratch_bytes, (size_t)total_blocks * sizeof(double));
            return ROHM_ERR_WORKSPACE;
        }
    }
    double* partial = static_cast<double*>(scratch);
    NormTable a;
    long long done = 0;
    int i = 0;
    while (i < n_tensors) {
        long long blocks = 0, elems = 0;
        int n = 0;
        for (; i < n_tensors && n < kChunk; ++i) {
            if (numel[i] == 0) continue;
            const long long nb = blocks_of(numel[i]);
            if (blocks + nb > kMaxBlocks) {
                ROHM_ARG_CHECK(n > 0, "grad_norm: tensor %d is too large for one launch", i);
                break;
            }
            a.g[n] = grads[i]; a.numel[n] = numel[i];
            a.first_block[n] = (int)blocks;
            blocks += nb;
            elems += numel[i];
            ++n;
        }
        if (n == 0) continue;
        a.first_block[n] = (int)blocks;
        a.n = n;
        a.partial = partial + done;
        prof::Scope ps("grad_norm", 2.0 * (double)elems, 4.0 * (double)elems, (hipStream_t)stream);
        hipLaunchKernelGGL(grad_sumsq_kernel, dim3((unsigned)blocks), dim3(kThreads), 0, (hipStream_t)stream, a);
        ROHM_LAUNCH_CHECK();
        done += blocks;
    }
    prof::Scope ps("grad_norm_finish", 0.0, 8.0 * (double)done, (hipStream_t)stream);
    hipLaunchKernelGGL(grad_norm_finish_kernel, dim3(1), dim3(kThreads), 0, (hipStream_t)stream, partial, (int)done, max_norm, out);
    ROHM_LAUNCH_CHECK();
    return ROHM_OK;
}
