// PoseNet training: a train-mode forward that keeps what the backward needs, and the backward of the whole network
// (model/posenet.py:75-96, model/heads.py:112-176, nn.TransformerEncoderLayer post-norm = oracle/nets.py:41-57) for
// `train/training_loop_posenet.py`.  Stateless with respect to the weights: every call takes device pointers to the live
// parameters, so an optimiser step needs no rebuild of anything.
//
// All products run on one strided, batched fp32-MFMA GEMM (v_mfma_f32_16x16x4_f32, exact fp32 fma chains like the rest of the
// library; the tile and its pipeline are train_tile.h).  Its operands are addressed through (row, column, batch) strides, so the transposed operands of the backward -- the
// reduction axis of a weight gradient is the token axis, the attention's dK / dV contract over queries -- are staged through LDS
// transposed instead of being materialised, and the [B, C, 1, T] channel-major tensors of the embeds and the output head are read
// and written in place.  Weight gradients split their token axis into slices of kRowsPerSplit rows that go to their own
// partial slab, and a second kernel adds the slabs in index order: no float atomics anywhere, so every gradient is bitwise reproducible.
//
// Dropout (train mode, keep-scale 1 / (1 - p)) at the reference's five sites: 0 PositionalEncoding (model/heads.py:126-129) on the
// [B, S, D] token sequence, 1 the attention probabilities inside nn.MultiheadAttention [B, H, S, S], 2 dropout1 on the attention
// output [B, S, D], 3 the FF inner activation after GELU [B, S, F], 4 dropout2 on the FF2 output [B, S, D].  Element e of site s of
// layer l is kept iff  hash(seed, 8 l + s, e) < (1 - p) 2^32  (a counter-based splitmix64 hash): the backward regenerates the masks
// instead of storing them, and rohm_posenet_dropout_mask materialises any of them.
#include <string.h>
#include "common.h"

namespace rohm {
namespace {

#include "train_reduce.h"
#include "train_tile.h"

constexpr int kD = 512, kH = 4, kF = 1024, kDh = 128, kMaxS = 145;
constexpr int kRowsPerSplit = 576;      // token rows per weight-gradient slice: 4 clips of 144 tokens, but any M goes -- a slice may cut a
                                        // clip (S = 145), and the last one is short: tgemm_kernel's k_total remainder bounds its K loop

// ---------------------------------------------------------------------------------------------------------------- dropout
__device__ __forceinline__ unsigned long long mix64(unsigned long long z) {
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
    return z ^ (z >> 31);
}
__device__ __forceinline__ bool drop_keep(unsigned long long seed, unsigned key, unsigned long long idx, unsigned thr) {
    const unsigned long long k = mix64(seed ^ (0x9E3779B97F4A7C15ull * (unsigned long long)(key + 1)));
    return (unsigned)(mix64(k + 0xD1B54A32D192ED03ull * (idx + 1)) >> 32) < thr;
}
struct Drop {
    unsigned long long seed;
    unsigned key, thr;
    float scale;
    int on;
};
__host__ __device__ inline unsigned drop_key(int layer, int site) { return (unsigned)(layer * 8 + site); }

// ---------------------------------------------------------------------------------------------------------------- GEMM
// C(z; m, n) = epi(alpha * sum_k A(z; m, k) B(z; k, n)), z = z1 * nb2 + z2, with
//   A(z; m, k) = A[z1 a_b1 + z2 a_b2 + m a_rs + k a_cs],  B(z; k, n) = B[z1 b_b1 + z2 b_b2 + k b_rs + n b_cs],
//   C(z; m, n) = C[z1 c_b1 + z2 c_b2 + m c_rs + n c_cs]   (pre / gz / R are indexed like C).
// k_total > 0: batch z1 is the slice [z1 K, z1 K + K) of a k_total-long reduction (weight-gradient splits; K = rows per split).
// Epilogue, in this order: * alpha, + bias[n], * qscale for n < qcols, pre := v, act (1 GELU, 2 SiLU), dropout (element m N + n),
// * act'(gz) (1 GELU', 2 SiLU'), + R, + C (accumulate), store.
struct TG {
    const float* A; long long a_rs, a_cs, a_b1, a_b2;
    const float* B; long long b_rs, b_cs, b_b1, b_b2;
    float* C; long long c_rs, c_cs, c_b1, c_b2;
    int M, N, K, nb1, nb2, k_total;
    float alpha;
    const float* bias;
    int qcols; float qscale;
    float* pre;
    int act;
    const float* gz; int gact;
    const float* R;
    int accumulate;
    Drop drop;
};

__device__ __forceinline__ float silu_f(float x) { return x / (1.0f + expf(-x)); }
__device__ __forceinline__ float silu_grad(float x) {
    const float s = 1.0f / (1.0f + expf(-x));
    return s * (1.0f + x * (1.0f - s));
}
__device__ __forceinline__ float gelu_grad(float x) {      // d/dx 0.5 x (1 + erf(x / sqrt 2))
    return 0.5f * (1.0f + erff(x * 0.70710678118654752440f)) + x * 0.39894228040143267794f * expf(-0.5f * x * x);
}

__global__ __launch_bounds__(256) void tgemm_kernel(TG p) {
    __shared__ float As[kStageFloats];      // [k][m]
    __shared__ float Bs[kStageFloats];      // [k][n]
    const int n0 = blockIdx.x * TBN, m0 = blockIdx.y * TBM;
    const int z1 = blockIdx.z / p.nb2, z2 = blockIdx.z % p.nb2;
    const float* A = p.A + z1 * p.a_b1 + z2 * p.a_b2;
    const float* Bp = p.B + z1 * p.b_b1 + z2 * p.b_b2;
    int kend = p.K;
    if (p.k_total > 0) {
        const int rem = p.k_total - z1 * p.K;
        kend = rem < p.K ? rem : p.K;
    }
    // global -> register staging: threads run along whichever axis of the operand is contiguous
    const bool a_kc = (p.a_cs == 1), b_nc = (p.b_cs == 1);
    float ra[8], rb[8];
    Tile t;
    t.run<TBK>(As, Bs, 0, kend,
        [&](int k0) __attribute__((always_inline)) {
#pragma unroll
            for (int e = 0; e < 8; ++e) {
                int m, k, kb, n;
                stage_map(!a_kc, e, k, m);
                stage_map(b_nc, e, kb, n);
                const int gm = m0 + m, gk = k0 + k, gn = n0 + n, gkb = k0 + kb;
                ra[e] = (gm < p.M && gk < kend) ? A[gm * p.a_rs + gk * p.a_cs] : 0.f;
                rb[e] = (gn < p.N && gkb < kend) ? Bp[gkb * p.b_rs + gn * p.b_cs] : 0.f;
            }
        },
        [&]() __attribute__((always_inline)) {
#pragma unroll
            for (int e = 0; e < 8; ++e) {
                int m, k, kb, n;
                stage_map(!a_kc, e, k, m);
                stage_map(b_nc, e, kb, n);
                As[stage_at(k, m)] = ra[e];
                Bs[stage_at(kb, n)] = rb[e];
            }
        });
    const auto& acc = t.acc;
    const long long cbase = z1 * p.c_b1 + z2 * p.c_b2;
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int j = 0; j < 2; ++j)
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const int m = m0 + t.row(i, r), n = n0 + t.col(j);
                if (m >= p.M || n >= p.N) continue;
                float v = acc[i][j][r] * p.alpha;
                if (p.bias) v += p.bias[n];
                if (n < p.qcols) v *= p.qscale;
                const long long ci = cbase + m * p.c_rs + n * p.c_cs;
                if (p.pre) p.pre[ci] = v;
                if (p.act == 1) v = gelu_erf(v);
                else if (p.act == 2) v = silu_f(v);
                if (p.drop.on)
                    v = drop_keep(p.drop.seed, p.drop.key, (unsigned long long)m * p.N + n, p.drop.thr) ? v * p.drop.scale : 0.f;
                if (p.gz) v *= (p.gact == 1) ? gelu_grad(p.gz[ci]) : silu_grad(p.gz[ci]);
                if (p.R) v += p.R[ci];
                if (p.accumulate) v += p.C[ci];
                p.C[ci] = v;
            }
}

// ---------------------------------------------------------------------------------------------------------------- row kernels
// Four floats of a caller's LIVE parameter (gamma, beta): the ABI asks only 4-byte alignment of a parameter (it may be a view into
// a flat buffer), so the 16-byte load is taken only where the address allows it.  `saved` and `scratch` are 16-byte aligned by contract.
__device__ __forceinline__ f32x4 param4(const float* p) {
    if ((reinterpret_cast<uintptr_t>(p) & 15) == 0) return *reinterpret_cast<const f32x4*>(p);
    return f32x4{p[0], p[1], p[2], p[3]};
}

// LayerNorm over D = 512 (one wave per row, 8 columns per lane): y = (x - mu) rstd g + b, stats[row] = (mu, rstd).
__global__ __launch_bounds__(256) void ln_fwd_kernel(const float* __restrict__ x, const float* __restrict__ g,
                                                     const float* __restrict__ b, float* __restrict__ y, float* __restrict__ stats,
                                                     int M, float eps) {
    const int row = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
    if (row >= M) return;
    const float* xr = x + (long long)row * kD;
    f32x4 v0 = *reinterpret_cast<const f32x4*>(xr + 4 * lane), v1 = *reinterpret_cast<const f32x4*>(xr + 256 + 4 * lane);
    float s = 0.f;
#pragma unroll
    for (int q = 0; q < 4; ++q) s += v0[q] + v1[q];
    const float mu = wave_sum64(s) * (1.0f / kD);
    float ss = 0.f;
#pragma unroll
    for (int q = 0; q < 4; ++q) ss += (v0[q] - mu) * (v0[q] - mu) + (v1[q] - mu) * (v1[q] - mu);
    const float rstd = 1.0f / sqrtf(wave_sum64(ss) * (1.0f / kD) + eps);
    const f32x4 g0 = param4(g + 4 * lane), g1 = param4(g + 256 + 4 * lane);
    const f32x4 b0 = param4(b + 4 * lane), b1 = param4(b + 256 + 4 * lane);
    f32x4 o0, o1;
#pragma unroll
    for (int q = 0; q < 4; ++q) {
        o0[q] = (v0[q] - mu) * rstd * g0[q] + b0[q];
        o1[q] = (v1[q] - mu) * rstd * g1[q] + b1[q];
    }
    *reinterpret_cast<f32x4*>(y + (long long)row * kD + 4 * lane) = o0;
    *reinterpret_cast<f32x4*>(y + (long long)row * kD + 256 + 4 * lane) = o1;
    if (lane == 0) { stats[2 * row] = mu; stats[2 * row + 1] = rstd; }
}

// LayerNorm backward: ds = rstd (dxh - mean(dxh) - xhat mean(dxh xhat)), dxh = dy g; gx = dy xhat (the gamma gradient's summand,
// column-summed afterwards); dd = dropout(ds) when the dropout is on (the sub-layer's gradient, model/posenet.py:63-69).
__global__ __launch_bounds__(256) void ln_bwd_kernel(const float* __restrict__ dy, const float* __restrict__ x,
                                                     const float* __restrict__ stats, const float* __restrict__ g,
                                                     float* __restrict__ ds, float* __restrict__ gx, float* __restrict__ dd, Drop drop,
                                                     int M) {
    const int row = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
    if (row >= M) return;
    const long long o = (long long)row * kD;
    const float mu = stats[2 * row], rstd = stats[2 * row + 1];
    float xh[8], dh[8], gy[8];
    float s1 = 0.f, s2 = 0.f;
#pragma unroll
    for (int h = 0; h < 2; ++h) {
        const f32x4 xv = *reinterpret_cast<const f32x4*>(x + o + 256 * h + 4 * lane);
        const f32x4 dv = *reinterpret_cast<const f32x4*>(dy + o + 256 * h + 4 * lane);
        const f32x4 gv = param4(g + 256 * h + 4 * lane);
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            xh[4 * h + q] = (xv[q] - mu) * rstd;
            gy[4 * h + q] = dv[q];
            dh[4 * h + q] = dv[q] * gv[q];
            s1 += dh[4 * h + q];
            s2 += dh[4 * h + q] * xh[4 * h + q];
        }
    }
    const float a = wave_sum64(s1) * (1.0f / kD), c = wave_sum64(s2) * (1.0f / kD);
#pragma unroll
    for (int h = 0; h < 2; ++h) {
        f32x4 dsv, gxv, ddv;
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            const int e = 4 * h + q;
            dsv[q] = rstd * (dh[e] - a - xh[e] * c);
            gxv[q] = gy[e] * xh[e];
            if (drop.on) {
                const unsigned long long idx = (unsigned long long)o + 256 * h + 4 * lane + q;
                ddv[q] = drop_keep(drop.seed, drop.key, idx, drop.thr) ? dsv[q] * drop.scale : 0.f;
            } else {
                ddv[q] = dsv[q];
            }
        }
        *reinterpret_cast<f32x4*>(ds + o + 256 * h + 4 * lane) = dsv;
        *reinterpret_cast<f32x4*>(gx + o + 256 * h + 4 * lane) = gxv;
        *reinterpret_cast<f32x4*>(dd + o + 256 * h + 4 * lane) = ddv;
    }
}

__device__ __forceinline__ float wave_max64(float v) {
#pragma unroll
    for (int o = 32; o; o >>= 1) v = fmaxf(v, __shfl_xor(v, o));
    return v;
}

// Softmax over the S <= 145 keys (three 64-key chunks: up to 192) of a row (one wave per row): P (saved) and, when the dropout is on, Pd = dropout(P).
__global__ __launch_bounds__(256) void softmax_fwd_kernel(const float* sc, float* P, float* __restrict__ Pd,
                                                          Drop drop, int rows, int S) {
    const int row = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
    if (row >= rows) return;
    const long long o = (long long)row * S;
    float v[3];
#pragma unroll
    for (int q = 0; q < 3; ++q) {
        const int j = lane + 64 * q;
        v[q] = j < S ? sc[o + j] : -INFINITY;
    }
    const float mx = wave_max64(fmaxf(fmaxf(v[0], v[1]), v[2]));
    float s = 0.f;
#pragma unroll
    for (int q = 0; q < 3; ++q) {
        const int j = lane + 64 * q;
        v[q] = j < S ? expf(v[q] - mx) : 0.f;
        s += v[q];
    }
    const float inv = 1.0f / wave_sum64(s);
#pragma unroll
    for (int q = 0; q < 3; ++q) {
        const int j = lane + 64 * q;
        if (j >= S) continue;
        const float pv = v[q] * inv;
        P[o + j] = pv;
        if (drop.on) Pd[o + j] = drop_keep(drop.seed, drop.key, (unsigned long long)(o + j), drop.thr) ? pv * drop.scale : 0.f;
    }
}

// Softmax backward in place: dP = dropout'(dPd); dS = P (dP - sum_j P dP)  (sum_j P dP = rowsum(dO o O) under the dropout).
__global__ __launch_bounds__(256) void softmax_bwd_kernel(const float* __restrict__ P, float* __restrict__ dP, Drop drop, int rows,
                                                          int S) {
    const int row = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
    if (row >= rows) return;
    const long long o = (long long)row * S;
    float pv[3], dv[3], s = 0.f;
#pragma unroll
    for (int q = 0; q < 3; ++q) {
        const int j = lane + 64 * q;
        pv[q] = j < S ? P[o + j] : 0.f;
        dv[q] = j < S ? dP[o + j] : 0.f;
        if (drop.on && j < S) dv[q] = drop_keep(drop.seed, drop.key, (unsigned long long)(o + j), drop.thr) ? dv[q] * drop.scale : 0.f;
        s += pv[q] * dv[q];
    }
    const float D = wave_sum64(s);
#pragma unroll
    for (int q = 0; q < 3; ++q) {
        const int j = lane + 64 * q;
        if (j < S) dP[o + j] = pv[q] * (dv[q] - D);
    }
}

// ---------------------------------------------------------------------------------------------------------------- elementwise
__global__ void dropout_apply_kernel(const float* x, float* y, Drop drop, long long n) {
    const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    y[i] = drop_keep(drop.seed, drop.key, (unsigned long long)i, drop.thr) ? x[i] * drop.scale : 0.f;
}

__global__ void dropout_mask_kernel(uint8_t* __restrict__ keep, Drop drop, long long n) {
    const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    keep[i] = drop_keep(drop.seed, drop.key, (unsigned long long)i, drop.thr) ? 1 : 0;
}

// pe[t] rows of the timestep embedding (model/heads.py:145): e0[b] = pe[clamp(t[b])]
__global__ void gather_pe_kernel(const float* __restrict__ pe, int pe_len, const int64_t* __restrict__ t, float* __restrict__ e0, int B) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= B * kD) return;
    long long tb = t[i / kD];
    tb = tb < 0 ? 0 : (tb >= pe_len ? pe_len - 1 : tb);
    e0[i] = pe[tb * kD + i % kD];
}

// h0 = dropout(cat(temb, x.Wx^T + bx + c.Wc^T + bc) + pe[:S]) in place (model/posenet.py:85-91): rows >= 1 hold the two GEMMs' sum
__global__ void embed_finish_kernel(float* __restrict__ h, const float* __restrict__ temb, const float* __restrict__ bx,
                                    const float* __restrict__ bc, const float* __restrict__ pe, Drop drop, int B, int S) {
    const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= (long long)B * S * kD) return;
    const int d = (int)(i % kD);
    const long long r = i / kD;
    const int s = (int)(r % S), b = (int)(r / S);
    float v = (s == 0) ? temb[(long long)b * kD + d] + pe[d] : h[i] + bx[d] + bc[d] + pe[(long long)s * kD + d];
    if (drop.on) v = drop_keep(drop.seed, drop.key, (unsigned long long)i, drop.thr) ? v * drop.scale : 0.f;
    h[i] = v;
}

// out[b][c][0][t] (+)= src[b][c][0][t] for c < traj (the trajectory channels copied from cond, model/posenet.py:94-95)
__global__ void traj_copy_kernel(const float* __restrict__ src, float* __restrict__ dst, int B, int C, int T, int traj, int add) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= B * traj * T) return;
    const int b = i / (traj * T), r = i % (traj * T);
    const long long o = (long long)b * C * T + r;
    dst[o] = add ? dst[o] + src[o] : src[o];
}

__global__ void q_sample_kernel(const float* __restrict__ x0, const float* __restrict__ noise, const float* __restrict__ sa,
                                const float* __restrict__ sb, const int64_t* __restrict__ t, int n_steps, int B, long long row,
                                float* __restrict__ out) {
    const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= (long long)B * row) return;
    long long tb = t[i / row];
    tb = tb < 0 ? 0 : (tb >= n_steps ? n_steps - 1 : tb);
    out[i] = sa[tb] * x0[i] + sb[tb] * noise[i];
}

// ---------------------------------------------------------------------------------------------------------------- host side
TG tg_plain() {
    TG p;
    memset(&p, 0, sizeof(p));
    p.alpha = 1.f;
    p.nb1 = p.nb2 = 1;
    return p;
}

int launch_tg(const TG& p, const char* label, hipStream_t s) {
    if (p.M <= 0 || p.N <= 0) return ROHM_OK;
    prof::Scope ps(label, 2.0 * p.M * p.N * (double)p.K * p.nb1 * p.nb2, 0.0, s);
    dim3 grid((p.N + TBN - 1) / TBN, (p.M + TBM - 1) / TBM, p.nb1 * p.nb2);
    hipLaunchKernelGGL(tgemm_kernel, grid, dim3(256), 0, s, p);
    ROHM_LAUNCH_CHECK();
    return ROHM_OK;
}

// Y[M, N] = X[M, K] . W[N, K]^T (+ epilogue) on token-major activations
TG tg_nt(const float* X, const float* W, float* Y, int M, int N, int K) {
    TG p = tg_plain();
    p.A = X; p.a_rs = K; p.a_cs = 1;
    p.B = W; p.b_rs = 1; p.b_cs = K;
    p.C = Y; p.c_rs = N; p.c_cs = 1;
    p.M = M; p.N = N; p.K = K;
    return p;
}
// dX[M, K] = dY[M, N] . W[N, K]
TG tg_nn(const float* dY, const float* W, float* dX, int M, int N, int K) {
    TG p = tg_plain();
    p.A = dY; p.a_rs = N; p.a_cs = 1;
    p.B = W; p.b_rs = K; p.b_cs = 1;
    p.C = dX; p.c_rs = K; p.c_cs = 1;
    p.M = M; p.N = K; p.K = N;
    return p;
}

Drop make_drop(float p, unsigned long long seed, int layer, int site) {
    Drop d;
    d.seed = seed;
    d.key = drop_key(layer, site);
    d.on = p > 0.f;
    const double keep = 1.0 - (double)p;
    const double thr = keep * 4294967296.0;
    d.thr = thr >= 4294967295.0 ? 0xFFFFFFFFu : (unsigned)thr;
    d.scale = (float)(1.0 / keep);
    return d;
}

struct Dims {
    int D, H, F, L, c_in, c_out, traj, B, T, S, M;
};

// Saved buffer (floats): per layer l  x, qkv, P, ctx, s1, st1, y, z, g, s2, st2;  then h_L, pd (forward's dropped-P slab), e0, u, su,
// temb.  x of layer 0 is the embedded, dropped token sequence; x of layer l + 1 is layer l's output.
struct SavedLayout {
    long long x, qkv, P, ctx, s1, st1, y, z, g, s2, st2, layer;
    long long hL, pd, e0, u, su, temb, total;
};
SavedLayout saved_layout(const Dims& d) {
    SavedLayout o;
    const long long M = d.M, D = d.D, F = d.F, PS = (long long)d.B * d.H * d.S * d.S;
    long long q = 0;
    auto take = [&](long long n) { const long long at = q; q += (n + 63) / 64 * 64; return at; };
    o.x = take(M * D); o.qkv = take(M * 3 * D); o.P = take(PS); o.ctx = take(M * D); o.s1 = take(M * D); o.st1 = take(2 * M);
    o.y = take(M * D); o.z = take(M * F); o.g = take(M * F); o.s2 = take(M * D); o.st2 = take(2 * M);
    o.layer = q;
    q = o.layer * d.L;
    o.hL = take(M * D); o.pd = take(PS); o.e0 = take((long long)d.B * D); o.u = take((long long)d.B * D);
    o.su = take((long long)d.B * D); o.temb = take((long long)d.B * D);
    o.total = q;
    return o;
}

struct ScratchLayout {
    long long dh, ds, dd, gx, dz, dy, dctx, dqkv, dP, pd, du, part, cpart, total;
};
int n_splits(const Dims& d) { return (d.M + kRowsPerSplit - 1) / kRowsPerSplit; }
ScratchLayout scratch_layout(const Dims& d) {
    ScratchLayout o;
    const long long M = d.M, D = d.D, F = d.F, PS = (long long)d.B * d.H * d.S * d.S;
    long long q = 0;
    auto take = [&](long long n) { const long long at = q; q += (n + 63) / 64 * 64; return at; };
    o.dh = take(M * D); o.ds = take(M * D); o.dd = take(M * D); o.gx = take(M * D); o.dz = take(M * F); o.dy = take(M * D);
    o.dctx = take(M * D); o.dqkv = take(M * 3 * D); o.dP = take(PS); o.pd = take(PS); o.du = take((long long)d.B * D);
    long long part = (long long)n_splits(d) * 3 * D * D;
    const long long pe = (long long)d.B * D * (d.c_in > d.c_out ? d.c_in : d.c_out);
    if (pe > part) part = pe;
    o.part = take(part);
    o.cpart = take((long long)((M + kColRows - 1) / kColRows) * 3 * D);
    o.total = q;
    return o;
}

int check_dims(int d_model, int n_head, int d_ff, int n_layer, int c_in, int c_out, int traj, int B, int T, Dims* out) {
    if (d_model != kD || n_head != kH || d_ff != kF || n_layer < 1 || c_in < 1 || c_out < 1 || traj < 0 || c_out + traj != c_in ||
        B < 1 || B > 16383 || T < 1 || T + 1 > kMaxS) {
        set_error("posenet training: unsupported shape d_model=%d n_head=%d d_ff=%d n_layer=%d c_in=%d c_out=%d traj=%d B=%d T=%d "
                  "(supported: d_model 512, 4 heads, d_ff 1024, n_layer >= 1, c_out + traj == c_in, 1 <= B <= 16383, 1 <= T <= 144)",
                  d_model, n_head, d_ff, n_layer, c_in, c_out, traj, B, T);
        return ROHM_ERR_UNSUPPORTED;
    }
    Dims& d = *out;
    d.D = d_model; d.H = n_head; d.F = d_ff; d.L = n_layer; d.c_in = c_in; d.c_out = c_out; d.traj = traj; d.B = B; d.T = T;
    d.S = T + 1; d.M = B * d.S;
    return ROHM_OK;
}

// dW[N, K] = dY^T . X over the M token rows (dY [M, N] row stride ldy, X [M, K] row stride ldx), split into row slices, and the
// bias gradient db[N] = column sums of dY.
int weight_grad(const float* dY, long long ldy, const float* X, long long ldx, int M, int N, int K, float* dW, float* db, float* part,
                float* cpart, hipStream_t s) {
    const int ns = (M + kRowsPerSplit - 1) / kRowsPerSplit;
    TG p = tg_plain();
    p.A = dY; p.a_rs = 1; p.a_cs = ldy; p.a_b1 = (long long)kRowsPerSplit * ldy;
    p.B = X; p.b_rs = ldx; p.b_cs = 1; p.b_b1 = (long long)kRowsPerSplit * ldx;
    p.c_rs = K; p.c_cs = 1; p.c_b1 = (long long)N * K;
    p.M = N; p.N = K; p.K = kRowsPerSplit; p.k_total = M; p.nb1 = ns;
    int rc = slab_sum(ns, p.c_b1, part, dW, s, [&](float* dst) { p.C = dst; return launch_tg(p, "train_wgrad", s); });
    if (rc) return rc;
    if (db) return colsum(dY, 0, M, ldy, 1, M, N, db, nullptr, cpart, s);
    return ROHM_OK;
}

// attention batched GEMM over (clip, head): z1 = clip, z2 = head
TG tg_heads(const Dims& d) {
    TG p = tg_plain();
    p.nb1 = d.B;
    p.nb2 = d.H;
    return p;
}

}  // namespace

// ================================================================================================================ forward
static int train_forward(const rohm_posenet_weights* w, const Dims& d, const float* x_t, const float* cond, const int64_t* t,
                         float dropout_p, unsigned long long seed, float* out, float* sv, hipStream_t s) {
    const SavedLayout o = saved_layout(d);
    const int D = d.D, F = d.F, M = d.M, S = d.S, T = d.T, B = d.B, H = d.H;
    const long long CT = (long long)d.c_in * T;
    const float qscale = 1.0f / sqrtf((float)kDh);
    int rc;
    // ---- timestep token: pe[t] -> Linear -> SiLU -> Linear (model/heads.py:140-146)
    hipLaunchKernelGGL(gather_pe_kernel, dim3(blocks((long long)B * D, 256)), dim3(256), 0, s, w->pe, w->pe_len, t, sv + o.e0, B);
    ROHM_LAUNCH_CHECK();
    TG p = tg_nt(sv + o.e0, w->t_w0, sv + o.su, B, D, D);
    p.bias = w->t_b0; p.pre = sv + o.u; p.act = 2;
    if ((rc = launch_tg(p, "train_time_mlp", s))) return rc;
    p = tg_nt(sv + o.su, w->t_w2, sv + o.temb, B, D, D);
    p.bias = w->t_b2;
    if ((rc = launch_tg(p, "train_time_mlp", s))) return rc;
    // ---- InputProcess of x_t and cond into rows 1..T of every clip (model/heads.py:154-160), then + biases, pe, token 0, dropout
    float* h0 = sv + o.x;
    for (int half = 0; half < 2; ++half) {
        p = tg_plain();
        p.A = half ? cond : x_t; p.a_rs = 1; p.a_cs = T; p.a_b1 = CT;
        p.B = half ? w->in_c_w : w->in_x_w; p.b_rs = 1; p.b_cs = d.c_in;
        p.C = h0 + D; p.c_rs = D; p.c_cs = 1; p.c_b1 = (long long)S * D;
        p.M = T; p.N = D; p.K = d.c_in; p.nb1 = B; p.accumulate = half;
        if ((rc = launch_tg(p, "train_embed", s))) return rc;
    }
    hipLaunchKernelGGL(embed_finish_kernel, dim3(blocks((long long)M * D, 256)), dim3(256), 0, s, h0, sv + o.temb, w->in_x_b, w->in_c_b,
                       w->pe, make_drop(dropout_p, seed, 0, 0), B, S);
    ROHM_LAUNCH_CHECK();
    // ---- encoder layers
    for (int l = 0; l < d.L; ++l) {
        const rohm_posenet_layer_weights& lw = w->layers[l];
        float* L0 = sv + (long long)l * o.layer;
        const float* x = L0 + o.x;
        float* qkv = L0 + o.qkv;
        float* P = L0 + o.P;
        float* ctx = L0 + o.ctx;
        float* xo = (l + 1 < d.L) ? sv + (long long)(l + 1) * o.layer + o.x : sv + o.hL;
        // in-projection, q pre-scaled by 1 / sqrt(dh)
        p = tg_nt(x, lw.in_proj_w, qkv, M, 3 * D, D);
        p.bias = lw.in_proj_b; p.qcols = D; p.qscale = qscale;
        if ((rc = launch_tg(p, "train_qkv", s))) return rc;
        // scores = q k^T per (clip, head) into P, softmax in place (P saved), Pd = dropout(P)
        p = tg_heads(d);
        p.A = qkv; p.a_rs = 3 * D; p.a_cs = 1; p.a_b1 = (long long)S * 3 * D; p.a_b2 = kDh;
        p.B = qkv + D; p.b_rs = 1; p.b_cs = 3 * D; p.b_b1 = (long long)S * 3 * D; p.b_b2 = kDh;
        p.C = P; p.c_rs = S; p.c_cs = 1; p.c_b1 = (long long)H * S * S; p.c_b2 = (long long)S * S;
        p.M = S; p.N = S; p.K = kDh;
        if ((rc = launch_tg(p, "train_attn_scores", s))) return rc;
        const Drop dp = make_drop(dropout_p, seed, l, 1);
        hipLaunchKernelGGL(softmax_fwd_kernel, dim3(blocks((long long)B * H * S, 4)), dim3(256), 0, s, P, P, sv + o.pd, dp, B * H * S, S);
        ROHM_LAUNCH_CHECK();
        // ctx = Pd v
        p = tg_heads(d);
        p.A = dp.on ? sv + o.pd : P; p.a_rs = S; p.a_cs = 1; p.a_b1 = (long long)H * S * S; p.a_b2 = (long long)S * S;
        p.B = qkv + 2 * D; p.b_rs = 3 * D; p.b_cs = 1; p.b_b1 = (long long)S * 3 * D; p.b_b2 = kDh;
        p.C = ctx; p.c_rs = D; p.c_cs = 1; p.c_b1 = (long long)S * D; p.c_b2 = kDh;
        p.M = S; p.N = kDh; p.K = S;
        if ((rc = launch_tg(p, "train_attn_pv", s))) return rc;
        // s1 = x + dropout1(out_proj(ctx)); y = norm1(s1)
        p = tg_nt(ctx, lw.out_proj_w, L0 + o.s1, M, D, D);
        p.bias = lw.out_proj_b; p.drop = make_drop(dropout_p, seed, l, 2); p.R = x;
        if ((rc = launch_tg(p, "train_out_proj", s))) return rc;
        hipLaunchKernelGGL(ln_fwd_kernel, dim3(blocks(M, 4)), dim3(256), 0, s, L0 + o.s1, lw.norm1_w, lw.norm1_b, L0 + o.y, L0 + o.st1, M,
                           1e-5f);
        ROHM_LAUNCH_CHECK();
        // z = linear1(y) (saved), g = dropout(gelu(z)); s2 = y + dropout2(linear2(g)); out = norm2(s2)
        p = tg_nt(L0 + o.y, lw.lin1_w, L0 + o.g, M, F, D);
        p.bias = lw.lin1_b; p.pre = L0 + o.z; p.act = 1; p.drop = make_drop(dropout_p, seed, l, 3);
        if ((rc = launch_tg(p, "train_ff1", s))) return rc;
        p = tg_nt(L0 + o.g, lw.lin2_w, L0 + o.s2, M, D, F);
        p.bias = lw.lin2_b; p.drop = make_drop(dropout_p, seed, l, 4); p.R = L0 + o.y;
        if ((rc = launch_tg(p, "train_ff2", s))) return rc;
        hipLaunchKernelGGL(ln_fwd_kernel, dim3(blocks(M, 4)), dim3(256), 0, s, L0 + o.s2, lw.norm2_w, lw.norm2_b, xo, L0 + o.st2, M, 1e-5f);
        ROHM_LAUNCH_CHECK();
    }
    // ---- OutputProcess on tokens 1..T into channels traj.. of [B, C_in, 1, T]; channels < traj from cond (model/heads.py:171-176)
    p = tg_plain();
    p.A = sv + o.hL + D; p.a_rs = D; p.a_cs = 1; p.a_b1 = (long long)S * D;
    p.B = w->out_w; p.b_rs = 1; p.b_cs = D;
    p.C = out + (long long)d.traj * T; p.c_rs = 1; p.c_cs = T; p.c_b1 = CT;
    p.M = T; p.N = d.c_out; p.K = D; p.nb1 = B; p.bias = w->out_b;
    if ((rc = launch_tg(p, "train_out_head", s))) return rc;
    if (d.traj > 0) {
        hipLaunchKernelGGL(traj_copy_kernel, dim3(blocks((long long)B * d.traj * T, 256)), dim3(256), 0, s, cond, out, B, d.c_in, T, d.traj, 0);
        ROHM_LAUNCH_CHECK();
    }
    return ROHM_OK;
}

// ================================================================================================================ backward
static int train_backward(const rohm_posenet_weights* w, const Dims& d, const float* x_t, const float* cond, float dropout_p,
                          unsigned long long seed, const float* sv, const float* d_out, const rohm_posenet_grads* g, float* d_x_t,
                          float* d_cond, float* sc, hipStream_t s) {
    const SavedLayout o = saved_layout(d);
    const ScratchLayout k = scratch_layout(d);
    const int D = d.D, F = d.F, M = d.M, S = d.S, T = d.T, B = d.B, H = d.H;
    const long long CT = (long long)d.c_in * T, PS = (long long)B * H * S * S;
    const float qscale = 1.0f / sqrtf((float)kDh);
    float *dh = sc + k.dh, *ds = sc + k.ds, *dd = sc + k.dd, *gx = sc + k.gx, *dz = sc + k.dz, *dy = sc + k.dy, *dctx = sc + k.dctx,
          *dqkv = sc + k.dqkv, *dP = sc + k.dP, *pd = sc + k.pd, *du = sc + k.du, *part = sc + k.part, *cpart = sc + k.cpart;
    int rc;
    // ---- output head: dh (tokens 1..T) = dOut^T-slices . Wout; dWout, dbout
    ROHM_HIP_CHECK(hipMemsetAsync(dh, 0, sizeof(float) * (size_t)M * D, s));
    TG p = tg_plain();
    p.A = d_out + (long long)d.traj * T; p.a_rs = 1; p.a_cs = T; p.a_b1 = CT;
    p.B = w->out_w; p.b_rs = D; p.b_cs = 1;
    p.C = dh + D; p.c_rs = D; p.c_cs = 1; p.c_b1 = (long long)S * D;
    p.M = T; p.N = D; p.K = d.c_out; p.nb1 = B;
    if ((rc = launch_tg(p, "train_bwd_head_dx", s))) return rc;
    p = tg_plain();
    p.A = d_out + (long long)d.traj * T; p.a_rs = T; p.a_cs = 1; p.a_b1 = CT;
    p.B = sv + o.hL + D; p.b_rs = D; p.b_cs = 1; p.b_b1 = (long long)S * D;
    p.c_rs = D; p.c_cs = 1; p.c_b1 = (long long)d.c_out * D;
    p.M = d.c_out; p.N = D; p.K = T; p.nb1 = B;      // one slab per clip
    if ((rc = slab_sum(B, p.c_b1, part, g->out_w, s, [&](float* dst) { p.C = dst; return launch_tg(p, "train_wgrad_head", s); }))) return rc;
    if ((rc = colsum(d_out + (long long)d.traj * T, CT, T, 1, T, B * T, d.c_out, g->out_b, nullptr, cpart, s))) return rc;
    // ---- encoder layers, last to first; dh = gradient of the layer's output
    for (int l = d.L - 1; l >= 0; --l) {
        const rohm_posenet_layer_weights& lw = w->layers[l];
        const rohm_posenet_layer_grads& lg = g->layers[l];
        const float* L0 = sv + (long long)l * o.layer;
        const float *x = L0 + o.x, *qkv = L0 + o.qkv, *P = L0 + o.P, *ctx = L0 + o.ctx, *y = L0 + o.y, *z = L0 + o.z, *gg = L0 + o.g;
        // norm2: ds = d s2 (the residual's gradient), dd = dropout2'(ds) (FF2's output gradient)
        hipLaunchKernelGGL(ln_bwd_kernel, dim3(blocks(M, 4)), dim3(256), 0, s, dh, L0 + o.s2, L0 + o.st2, lw.norm2_w, ds, gx, dd,
                           make_drop(dropout_p, seed, l, 4), M);
        ROHM_LAUNCH_CHECK();
        if ((rc = colsum(dh, 0, M, D, 1, M, D, lg.norm2_b, nullptr, cpart, s))) return rc;
        if ((rc = colsum(gx, 0, M, D, 1, M, D, lg.norm2_w, nullptr, cpart, s))) return rc;
        // linear2
        if ((rc = weight_grad(dd, D, gg, F, M, D, F, lg.lin2_w, lg.lin2_b, part, cpart, s))) return rc;
        p = tg_nn(dd, lw.lin2_w, dz, M, D, F);
        p.drop = make_drop(dropout_p, seed, l, 3); p.gz = z; p.gact = 1;
        if ((rc = launch_tg(p, "train_bwd_ff2_dx", s))) return rc;
        // linear1; dy = dz . W1 + ds
        if ((rc = weight_grad(dz, F, y, D, M, F, D, lg.lin1_w, lg.lin1_b, part, cpart, s))) return rc;
        p = tg_nn(dz, lw.lin1_w, dy, M, F, D);
        p.R = ds;
        if ((rc = launch_tg(p, "train_bwd_ff1_dx", s))) return rc;
        // norm1
        hipLaunchKernelGGL(ln_bwd_kernel, dim3(blocks(M, 4)), dim3(256), 0, s, dy, L0 + o.s1, L0 + o.st1, lw.norm1_w, ds, gx, dd,
                           make_drop(dropout_p, seed, l, 2), M);
        ROHM_LAUNCH_CHECK();
        if ((rc = colsum(dy, 0, M, D, 1, M, D, lg.norm1_b, nullptr, cpart, s))) return rc;
        if ((rc = colsum(gx, 0, M, D, 1, M, D, lg.norm1_w, nullptr, cpart, s))) return rc;
        // out-projection
        if ((rc = weight_grad(dd, D, ctx, D, M, D, D, lg.out_proj_w, lg.out_proj_b, part, cpart, s))) return rc;
        p = tg_nn(dd, lw.out_proj_w, dctx, M, D, D);
        if ((rc = launch_tg(p, "train_bwd_out_proj_dx", s))) return rc;
        // attention, per (clip, head)
        const Drop dp = make_drop(dropout_p, seed, l, 1);
        if (dp.on) {
            hipLaunchKernelGGL(dropout_apply_kernel, dim3(blocks(PS, 256)), dim3(256), 0, s, P, pd, dp, PS);
            ROHM_LAUNCH_CHECK();
        }
        // dV = Pd^T dO
        p = tg_heads(d);
        p.A = dp.on ? pd : P; p.a_rs = 1; p.a_cs = S; p.a_b1 = (long long)H * S * S; p.a_b2 = (long long)S * S;
        p.B = dctx; p.b_rs = D; p.b_cs = 1; p.b_b1 = (long long)S * D; p.b_b2 = kDh;
        p.C = dqkv + 2 * D; p.c_rs = 3 * D; p.c_cs = 1; p.c_b1 = (long long)S * 3 * D; p.c_b2 = kDh;
        p.M = S; p.N = kDh; p.K = S;
        if ((rc = launch_tg(p, "train_bwd_attn_dv", s))) return rc;
        // dPd = dO V^T, then dS in place
        p = tg_heads(d);
        p.A = dctx; p.a_rs = D; p.a_cs = 1; p.a_b1 = (long long)S * D; p.a_b2 = kDh;
        p.B = qkv + 2 * D; p.b_rs = 1; p.b_cs = 3 * D; p.b_b1 = (long long)S * 3 * D; p.b_b2 = kDh;
        p.C = dP; p.c_rs = S; p.c_cs = 1; p.c_b1 = (long long)H * S * S; p.c_b2 = (long long)S * S;
        p.M = S; p.N = S; p.K = kDh;
        if ((rc = launch_tg(p, "train_bwd_attn_dp", s))) return rc;
        hipLaunchKernelGGL(softmax_bwd_kernel, dim3(blocks((long long)B * H * S, 4)), dim3(256), 0, s, P, dP, dp, B * H * S, S);
        ROHM_LAUNCH_CHECK();
        // dQ = dS K scale (q was pre-scaled), dK = dS^T q_scaled
        p = tg_heads(d);
        p.A = dP; p.a_rs = S; p.a_cs = 1; p.a_b1 = (long long)H * S * S; p.a_b2 = (long long)S * S;
        p.B = qkv + D; p.b_rs = 3 * D; p.b_cs = 1; p.b_b1 = (long long)S * 3 * D; p.b_b2 = kDh;
        p.C = dqkv; p.c_rs = 3 * D; p.c_cs = 1; p.c_b1 = (long long)S * 3 * D; p.c_b2 = kDh;
        p.M = S; p.N = kDh; p.K = S; p.alpha = qscale;
        if ((rc = launch_tg(p, "train_bwd_attn_dq", s))) return rc;
        p = tg_heads(d);
        p.A = dP; p.a_rs = 1; p.a_cs = S; p.a_b1 = (long long)H * S * S; p.a_b2 = (long long)S * S;
        p.B = qkv; p.b_rs = 3 * D; p.b_cs = 1; p.b_b1 = (long long)S * 3 * D; p.b_b2 = kDh;
        p.C = dqkv + D; p.c_rs = 3 * D; p.c_cs = 1; p.c_b1 = (long long)S * 3 * D; p.c_b2 = kDh;
        p.M = S; p.N = kDh; p.K = S;
        if ((rc = launch_tg(p, "train_bwd_attn_dk", s))) return rc;
        // in-projection; dx = dqkv . W_in + d s1 -> the previous layer's output gradient
        if ((rc = weight_grad(dqkv, 3 * D, x, D, M, 3 * D, D, lg.in_proj_w, lg.in_proj_b, part, cpart, s))) return rc;
        p = tg_nn(dqkv, lw.in_proj_w, dh, M, 3 * D, D);
        p.R = ds;
        if ((rc = launch_tg(p, "train_bwd_qkv_dx", s))) return rc;
    }
    // ---- embedding: dh -> gradient before the PositionalEncoding dropout
    const Drop d0 = make_drop(dropout_p, seed, 0, 0);
    if (d0.on) {
        hipLaunchKernelGGL(dropout_apply_kernel, dim3(blocks((long long)M * D, 256)), dim3(256), 0, s, dh, dh, d0, (long long)M * D);
        ROHM_LAUNCH_CHECK();
    }
    // time MLP from token 0
    p = tg_plain();
    p.A = dh; p.a_rs = 1; p.a_cs = (long long)S * D;
    p.B = sv + o.su; p.b_rs = D; p.b_cs = 1;
    p.C = g->t_w2; p.c_rs = D; p.c_cs = 1;
    p.M = D; p.N = D; p.K = B;
    if ((rc = launch_tg(p, "train_wgrad_time", s))) return rc;
    if ((rc = colsum(dh, (long long)S * D, 1, 0, 1, B, D, g->t_b2, nullptr, cpart, s))) return rc;
    p = tg_plain();
    p.A = dh; p.a_rs = (long long)S * D; p.a_cs = 1;
    p.B = w->t_w2; p.b_rs = D; p.b_cs = 1;
    p.C = du; p.c_rs = D; p.c_cs = 1;
    p.M = B; p.N = D; p.K = D; p.gz = sv + o.u; p.gact = 2;
    if ((rc = launch_tg(p, "train_bwd_time_dx", s))) return rc;
    p = tg_plain();
    p.A = du; p.a_rs = 1; p.a_cs = D;
    p.B = sv + o.e0; p.b_rs = D; p.b_cs = 1;
    p.C = g->t_w0; p.c_rs = D; p.c_cs = 1;
    p.M = D; p.N = D; p.K = B;
    if ((rc = launch_tg(p, "train_wgrad_time", s))) return rc;
    if ((rc = colsum(du, D, 1, 0, 1, B, D, g->t_b0, nullptr, cpart, s))) return rc;
    // the two InputProcess Linears: both biases get the column sums over tokens >= 1
    if ((rc = colsum(dh + D, (long long)S * D, T, D, 1, B * T, D, g->in_x_b, g->in_c_b, cpart, s))) return rc;
    for (int half = 0; half < 2; ++half) {
        const float* src = half ? cond : x_t;
        p = tg_plain();
        p.A = dh + D; p.a_rs = 1; p.a_cs = D; p.a_b1 = (long long)S * D;
        p.B = src; p.b_rs = 1; p.b_cs = T; p.b_b1 = CT;
        p.c_rs = d.c_in; p.c_cs = 1; p.c_b1 = (long long)D * d.c_in;
        p.M = D; p.N = d.c_in; p.K = T; p.nb1 = B;      // one slab per clip
        rc = slab_sum(B, p.c_b1, part, half ? g->in_c_w : g->in_x_w, s,
                      [&](float* slabs) { p.C = slabs; return launch_tg(p, "train_wgrad_embed", s); });
        if (rc) return rc;
        float* dst = half ? d_cond : d_x_t;
        if (!dst) continue;
        p = tg_plain();
        p.A = dh + D; p.a_rs = D; p.a_cs = 1; p.a_b1 = (long long)S * D;
        p.B = half ? w->in_c_w : w->in_x_w; p.b_rs = d.c_in; p.b_cs = 1;
        p.C = dst; p.c_rs = 1; p.c_cs = T; p.c_b1 = CT;
        p.M = T; p.N = d.c_in; p.K = D; p.nb1 = B;
        if ((rc = launch_tg(p, "train_bwd_embed_dx", s))) return rc;
    }
    if (d_cond && d.traj > 0) {      // the trajectory channels of the output are cond's own
        hipLaunchKernelGGL(traj_copy_kernel, dim3(blocks((long long)B * d.traj * T, 256)), dim3(256), 0, s, d_out, d_cond, B, d.c_in, T,
                           d.traj, 1);
        ROHM_LAUNCH_CHECK();
    }
    return ROHM_OK;
}

}  // namespace rohm

using namespace rohm;

extern "C" size_t rohm_posenet_train_saved_bytes(int d_model, int n_head, int d_ff, int n_layer, int c_in, int c_out, int B, int T) {
    Dims d;
    if (check_dims(d_model, n_head, d_ff, n_layer, c_in, c_out, c_in - c_out, B, T, &d)) return 0;
    return (size_t)saved_layout(d).total * sizeof(float);
}

extern "C" size_t rohm_posenet_train_scratch_bytes(int d_model, int n_head, int d_ff, int n_layer, int c_in, int c_out, int B, int T) {
    Dims d;
    if (check_dims(d_model, n_head, d_ff, n_layer, c_in, c_out, c_in - c_out, B, T, &d)) return 0;
    return (size_t)scratch_layout(d).total * sizeof(float);
}

extern "C" int rohm_posenet_train_forward(const rohm_posenet_weights* w, int d_model, int n_head, int d_ff, int n_layer, int c_in,
                                          int c_out, int traj_dim, const float* x_t, const float* cond, const int64_t* t, int B, int T,
                                          float dropout_p, unsigned long long seed, float* out, void* saved, size_t saved_bytes,
                                          rohm_stream_t stream) {
    Dims d;
    int rc = check_dims(d_model, n_head, d_ff, n_layer, c_in, c_out, traj_dim, B, T, &d);
    if (rc) return rc;
    ROHM_ARG_CHECK(w && w->layers && x_t && cond && t && out && saved, "rohm_posenet_train_forward: null argument");
    ROHM_ARG_CHECK(w->pe && w->pe_len >= T + 1, "rohm_posenet_train_forward: pe must have >= T + 1 = %d rows", T + 1);
    ROHM_ARG_CHECK(dropout_p >= 0.f && dropout_p < 1.f, "rohm_posenet_train_forward: dropout_p=%g must be in [0, 1)", (double)dropout_p);
    ROHM_ARG_CHECK(aligned16(saved), "rohm_posenet_train_forward: saved must be 16-byte aligned");
    ROHM_ARG_CHECK(saved_bytes >= (size_t)saved_layout(d).total * sizeof(float), "rohm_posenet_train_forward: saved buffer too small");
    return train_forward(w, d, x_t, cond, t, dropout_p, seed, out, static_cast<float*>(saved), static_cast<hipStream_t>(stream));
}

extern "C" int rohm_posenet_train_backward(const rohm_posenet_weights* w, int d_model, int n_head, int d_ff, int n_layer, int c_in,
                                           int c_out, int traj_dim, const float* x_t, const float* cond, int B, int T, float dropout_p,
                                           unsigned long long seed, const void* saved, size_t saved_bytes, const float* d_out,
                                           const rohm_posenet_grads* grads, float* d_x_t, float* d_cond, void* scratch,
                                           size_t scratch_bytes, rohm_stream_t stream) {
    Dims d;
    int rc = check_dims(d_model, n_head, d_ff, n_layer, c_in, c_out, traj_dim, B, T, &d);
    if (rc) return rc;
    ROHM_ARG_CHECK(w && w->layers && grads && grads->layers && x_t && cond && saved && d_out && scratch,
                   "rohm_posenet_train_backward: null argument");
    ROHM_ARG_CHECK(dropout_p >= 0.f && dropout_p < 1.f, "rohm_posenet_train_backward: dropout_p=%g must be in [0, 1)", (double)dropout_p);
    ROHM_ARG_CHECK(aligned16(saved) && aligned16(scratch), "rohm_posenet_train_backward: saved / scratch must be 16-byte aligned");
    ROHM_ARG_CHECK(saved_bytes >= (size_t)saved_layout(d).total * sizeof(float), "rohm_posenet_train_backward: saved buffer too small");
    ROHM_ARG_CHECK(scratch_bytes >= (size_t)scratch_layout(d).total * sizeof(float), "rohm_posenet_train_backward: scratch too small");
    return train_backward(w, d, x_t, cond, dropout_p, seed, static_cast<const float*>(saved), d_out, grads, d_x_t, d_cond,
                          static_cast<float*>(scratch), static_cast<hipStream_t>(stream));
}

extern "C" int rohm_posenet_dropout_mask(unsigned long long seed, int layer, int site, float dropout_p, long long n, uint8_t* keep,
                                         rohm_stream_t stream) {
    ROHM_ARG_CHECK(keep && n >= 0 && layer >= 0 && site >= 0 && site <= 4 && (site != 0 || layer == 0),
                   "rohm_posenet_dropout_mask: bad arguments (layer=%d site=%d n=%lld)", layer, site, n);
    ROHM_ARG_CHECK(dropout_p >= 0.f && dropout_p < 1.f, "rohm_posenet_dropout_mask: dropout_p=%g must be in [0, 1)", (double)dropout_p);
    if (n == 0) return ROHM_OK;
    hipLaunchKernelGGL(dropout_mask_kernel, dim3(blocks(n, 256)), dim3(256), 0, static_cast<hipStream_t>(stream), keep,
                       make_drop(dropout_p, seed, layer, site), n);
    ROHM_LAUNCH_CHECK();
    return ROHM_OK;
}

extern "C" int rohm_q_sample(const float* x0, const float* noise, const float* sqrt_ac, const float* sqrt_1m_ac, const int64_t* t,
                             int n_steps, int B, long long row_len, float* out, rohm_stream_t stream) {
    ROHM_ARG_CHECK(x0 && noise && sqrt_ac && sqrt_1m_ac && t && out && n_steps > 0 && B >= 0 && row_len >= 0,
                   "rohm_q_sample: bad arguments");
    if ((long long)B * row_len == 0) return ROHM_OK;
    hipLaunchKernelGGL(q_sample_kernel, dim3(blocks((long long)B * row_len, 256)), dim3(256), 0, static_cast<hipStream_t>(stream), x0,
                       noise, sqrt_ac, sqrt_1m_ac, t, n_steps, B, row_len, out);
    ROHM_LAUNCH_CHECK();
    return ROHM_OK;
}
