// Deterministic reductions shared by the two training sources (posenet_train.hip, trajnet_train.hip): column sums in row chunks and
// the in-order sum of partial slabs (slab_sum).  No float atomics: a gradient summed here is bitwise reproducible.  Included inside each
// source's anonymous namespace.
#pragma once

constexpr int kColRows = 256;           // rows per column-sum chunk

inline unsigned blocks(long long n, int per) { return (unsigned)((n + per - 1) / per); }

// Column sums, first pass: part[chunk][n] = sum over rows r of the chunk of X(r, n), X(r, n) = X[(r / inner) outer_stride +
// (r % inner) inner_stride + n col_stride]; 64 columns x 4 row phases per workgroup, the phases added in a fixed order.
__global__ __launch_bounds__(256) void colsum_kernel(const float* __restrict__ X, long long outer_stride, int inner,
                                                     long long inner_stride, long long col_stride, int rows, int N,
                                                     float* __restrict__ part) {
    __shared__ float red[4][64];
    const int c = threadIdx.x & 63, ph = threadIdx.x >> 6;
    const int n = blockIdx.x * 64 + c;
    const int r0 = blockIdx.y * kColRows;
    float s = 0.f;
    if (n < N)
        for (int r = r0 + ph; r < r0 + kColRows && r < rows; r += 4)
            s += X[(long long)(r / inner) * outer_stride + (long long)(r % inner) * inner_stride + n * col_stride];
    red[ph][c] = s;
    __syncthreads();
    if (ph == 0 && n < N) part[(long long)blockIdx.y * N + n] = ((red[0][c] + red[1][c]) + red[2][c]) + red[3][c];
}

// out[i] = sum_s part[s][i], slabs added in index order; out2 (optional) receives the same values
__global__ void reduce_slabs_kernel(const float* __restrict__ part, int S, long long n, float* __restrict__ out, float* __restrict__ out2) {
    const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    float s = part[i];
    for (int k = 1; k < S; ++k) s += part[(long long)k * n + i];
    out[i] = s;
    if (out2) out2[i] = s;
}

// A product split into ns partial slabs of n floats each, then summed in slab order into out: product(dst) launches the GEMM that
// writes slab s at dst + s n.  A single slab is written straight to out, with no second launch.
template <class Product>
inline int slab_sum(int ns, long long n, float* part, float* out, hipStream_t s, Product product) {
    const int rc = product(ns > 1 ? part : out);
    if (rc || ns <= 1) return rc;
    hipLaunchKernelGGL(reduce_slabs_kernel, dim3(blocks(n, 256)), dim3(256), 0, s, part, ns, n, out, (float*)nullptr);
    ROHM_LAUNCH_CHECK();
    return ROHM_OK;
}

inline int colsum(const float* X, long long outer_stride, int inner, long long inner_stride, long long col_stride, int rows, int N,
                  float* out, float* out2, float* part, hipStream_t s) {
    const int chunks = (rows + kColRows - 1) / kColRows;
    hipLaunchKernelGGL(colsum_kernel, dim3((N + 63) / 64, chunks), dim3(256), 0, s, X, outer_stride, inner, inner_stride, col_stride,
                       rows, N, part);
    ROHM_LAUNCH_CHECK();
    hipLaunchKernelGGL(reduce_slabs_kernel, dim3(blocks(N, 256)), dim3(256), 0, s, part, chunks, (long long)N, out, out2);
    ROHM_LAUNCH_CHECK();
    return ROHM_OK;
}
