// The ordered reductions under the geometry and metric kernels (floor, rig, sync, multiview, quality, the shape totals of fit.hip, the
// AMASS and scene metrics).  Every one of those kernels promises "the same input, the same bits", so the order of a reduction is part
// of what its entry point computes: it is stated here, once, in the comment of the function that fixes it.  Device code only; the one
// kernel is the arg-max of the RANSAC scores.  Nothing here multiplies: the helpers add, compare and move, so a caller's
// floating-point contraction setting (scene_metrics.hip switches it off) has nothing to act on.
//
// Not here: common.h's wave_sum64 (float, on the VALU) and the reductions of the inference and training kernels; the fixed-order LDS
// sums inside rig_ba_moments_kernel, rig_ba_close_kernel and fit_math.h's solver, which have owners, not butterflies.
#pragma once
#include "common.h"

#include <limits.h>

namespace rohm {

// ---- the operations: op(a, b) with a the value held and b the value that arrives ----
struct SumOp {
    template <class T> __device__ __forceinline__ T operator()(T a, T b) const { return a + b; }
};
struct MaxOp {
    __device__ __forceinline__ int operator()(int a, int b) const { return max(a, b); }
};
struct MinOp {
    __device__ __forceinline__ int operator()(int a, int b) const { return min(a, b); }
    __device__ __forceinline__ float operator()(float a, float b) const { return fminf(a, b); }
    __device__ __forceinline__ double operator()(double a, double b) const { return fmin(a, b); }
};

// the larger of two, a NaN wins
__device__ __forceinline__ double max_nan(double a, double b) { return (a > b || a != a) ? a : b; }
struct MaxNanOp {
    __device__ __forceinline__ double operator()(double a, double b) const { return max_nan(a, b); }
};

// a value with the index it came from, and the better of two: the larger value (kLower: the lower value); the lower index on ties
template <class T>
struct Scored {
    T s;
    int h;
};

template <bool kLower = false, class T>
__device__ __forceinline__ Scored<T> better_of(Scored<T> a, Scored<T> b) {
    return ((kLower ? b.s < a.s : b.s > a.s) || (b.s == a.s && b.h < a.h)) ? b : a;
}

template <class T>
__device__ __forceinline__ T lane_xor(T v, int o, int width) {
    return __shfl_xor(v, o, width);
}
template <class T>
__device__ __forceinline__ Scored<T> lane_xor(Scored<T> v, int o, int width) {
    return Scored<T>{__shfl_xor(v.s, o, width), __shfl_xor(v.h, o, width)};
}

// The xor butterfly over the W lanes (16, 32 or 64) that share lane / W: v = op(v, v of lane ^ o) for o = W / 2, W / 4, ..., 1.  Every
// one of the W lanes ends with the same bits.  kWidth is the width handed to the shuffle: 64 everywhere but in track_quality_kernel,
// whose half-waves have always passed 32.
template <int W, int kWidth = 64, class T, class Op>
__device__ __forceinline__ T lanes_reduce(T v, Op op) {
    static_assert(W == 16 || W == 32 || W == 64, "a group of lanes is 16, 32 or 64 wide");
#pragma unroll
    for (int o = W / 2; o > 0; o >>= 1) v = op(v, lane_xor(v, o, kWidth));
    return v;
}

// the sum over the W lanes of a group (the 16 lanes of a point in multiview.hip and rig.hip's bundle adjustment), in every one of them
template <int W, int kWidth = 64, class T>
__device__ __forceinline__ T lanes_sum(T v) {
    return lanes_reduce<W, kWidth>(v, SumOp());
}

// K values per thread of a workgroup of Threads to K results, out[k] = op(k, ., .) over all threads: per k the 64-lane butterfly of
// lanes_reduce, lane 0 of wave w stores to shm[w][k], one barrier, then thread k folds the wave partials in wave order, ((w0 op w1)
// op w2) ..., and writes out[k].  op(k, a, b) may depend on k (the quality totals keep a maximum in one column).  Every thread of the
// workgroup must call it; out is written by threads 0 .. K - 1 and is not ordered against anything after the call.
template <int Threads, int K, class Op>
__device__ __forceinline__ void block_reduce(const double (&m)[K], double (*shm)[K], double* out, Op op) {
    static_assert(Threads % 64 == 0 && K <= Threads, "whole waves, and a thread per result");
    const int tid = threadIdx.x;
#pragma unroll
    for (int k = 0; k < K; ++k) {
        const double v = lanes_reduce<64>(m[k], [&](double a, double b) { return op(k, a, b); });
        if ((tid & 63) == 0) shm[tid >> 6][k] = v;
    }
    __syncthreads();
    if (tid < K) {
        double v = shm[0][tid];
        for (int w = 1; w < Threads / 64; ++w) v = op(tid, v, shm[w][tid]);
        out[tid] = v;
    }
}

// op(k, a, b) of a plain sum
struct SumOfK {
    __device__ __forceinline__ double operator()(int, double a, double b) const { return a + b; }
};

// The RANSAC kernels' counts: a workgroup of 256 threads holds Lanes hypotheses side by side (thread tid serves hypothesis lane
// tid % Lanes) and 256 / Lanes groups of lanes that dealt the points among themselves.  The sum of v over the groups that share a
// hypothesis lane, in every thread: shuffles over the offsets Lanes, 2 Lanes, ..., 32, then the four waves' partials through shc
// [4 * Lanes] in wave order.  Integer counts: no order could change a bit.  Two barriers; shc is free again on return.
template <int Lanes>
__device__ __forceinline__ int group_sum(int v, int* shc, int tid) {
#pragma unroll
    for (int o = Lanes; o < 64; o <<= 1) v += __shfl_xor(v, o, 64);
    const int l = tid % Lanes;
    if ((tid & 63) < Lanes) shc[(tid >> 6) * Lanes + l] = v;
    __syncthreads();
    const int r = shc[l] + shc[Lanes + l] + shc[2 * Lanes + l] + shc[3 * Lanes + l];
    __syncthreads();
    return r;
}

// The best of a workgroup's (value, index) pairs, in thread 0 (the other threads get their own wave's): the 64-lane butterfly of
// better_of, lane 0 of wave w stores to sh_s[w], sh_h[w], one barrier, thread 0 folds waves 1, 2, ... into its own.  better_of is
// associative and commutative, ties included, so the order cannot change the winner.  Part of the contract: exactly one barrier,
// after the wave partials are stored and before thread 0 reads them, so what a caller stored to LDS before the call is published by
// it too (floor_clearance_kernel's per-wave counts are).
template <int Threads, bool kLower, class T>
__device__ __forceinline__ Scored<T> block_arg_best(Scored<T> b, T* sh_s, int* sh_h) {
    const int tid = threadIdx.x;
    b = lanes_reduce<64>(b, [](Scored<T> x, Scored<T> y) { return better_of<kLower>(x, y); });
    if ((tid & 63) == 0) {
        sh_s[tid >> 6] = b.s;
        sh_h[tid >> 6] = b.h;
    }
    __syncthreads();
    if (tid == 0)
        for (int w = 1; w < Threads / 64; ++w) b = better_of<kLower>(b, Scored<T>{sh_s[w], sh_h[w]});
    return b;
}

// best[r] = the index of the largest of the K scores scores[(r K + h) kStride], h < K, the lower index on ties; -1 when even the
// winner is below kNoneBelow, which is how the RANSAC kernels mark a degenerate hypothesis.  One workgroup per row r of best.  The
// stride and the bound are template arguments, not kernel arguments: the address of a score stays a constant multiple, as in the two
// kernels this one replaced.
template <int Threads, int kStride, long long kNoneBelow>
__global__ __launch_bounds__(Threads) void best_score_kernel(const long long* __restrict__ scores, int K, int* __restrict__ best) {
    __shared__ long long sh_s[Threads / 64];
    __shared__ int sh_h[Threads / 64];
    const long long* c = scores + (size_t)blockIdx.x * (size_t)K * kStride;
    Scored<long long> b = {kNoneBelow - 1, INT_MAX};
    for (int h = threadIdx.x; h < K; h += Threads) b = better_of(b, Scored<long long>{c[(size_t)h * kStride], h});
    b = block_arg_best<Threads, false>(b, sh_s, sh_h);
    if (threadIdx.x == 0) best[blockIdx.x] = b.s < kNoneBelow ? -1 : b.h;
}

// The LDS tree over a workgroup of blockDim.x threads (a power of two), sh [blockDim.x]: sh[t] = op(sh[t], sh[t + o]) for t < o, o =
// blockDim.x / 2, ..., 1, a barrier after each level; every thread gets sh[0].  A leading barrier frees sh from the call before.
template <class T, class Op>
__device__ __forceinline__ T block_tree_reduce(T v, T* sh, Op op) {
    const int tid = threadIdx.x;
    __syncthreads();
    sh[tid] = v;
    __syncthreads();
    for (int o = blockDim.x / 2; o > 0; o >>= 1) {
        if (tid < o) sh[tid] = op(sh[tid], sh[tid + o]);
        __syncthreads();
    }
    return sh[0];
}

}  // namespace rohm
