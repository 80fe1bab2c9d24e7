// TrajNet / TrajControl training: a train-mode forward that keeps what the backward needs, and the backward of the whole conv U-Net
// (model/trajnet.py:177-275 with the blocks of model/heads.py:12-106 and the ControlNet of model/trajnet.py:10-75) for
// `train/training_loop_trajnet.py`.  Stateless with respect to the weights like posenet_train.hip: every call takes device pointers
// to the live parameters in the reference's layouts (Conv1d [C_out, C_in, k], ConvTranspose1d [C_in, C_out, k]) in the order of
// the state_dict, and gradients are written in those layouts.  TrajNet has no dropout and GroupNorm no running statistics, so this
// forward computes the function of the inference forward.
//
// Activations are channels-last with two zero halo rows on either side of every clip: [B, T_l + 4, C] at U-Net level l
// (T_l = T >> l).  A convolution is then a GEMM over the flattened rows whose A operand is read at a row offset per tap -- no
// gather and no boundary predicate inside a clip -- and whose epilogue stores zeros on the halo rows, so every buffer is written
// whole by the kernel that produces it.  The stride-2 convs map output rows to input rows with a factor of two (the transposed
// conv as two phases).  Two kernels carry all products, on the tile of train_tile.h (v_mfma_f32_16x16x4_f32, exact fp32 fma chains):
//   cgemm_kernel  Y = taps(X) . W    forward convs, data gradients (taps mirrored / phases swapped), the Linears of the time path;
//                 the weights are read in place through (tap, k, n) strides;
//   wgemm_kernel  dW = dY^T . taps(X) over a slab of whole clips, one tap per grid slice; slabs are added in index order afterwards.
// GroupNorm's d gamma / d beta and the time-bias gradients are per-sample partials summed in sample order.  No float atomics.
#include <string.h>
#include <atomic>
#include "trajnet_priv.h"

namespace rohm {
namespace {

#include "train_reduce.h"
#include "train_tile.h"

constexpr int kGroups = 8, kHalo = 2, kTdim = 32, kMid = 512;
constexpr int kSlabRows = 512;          // rows per weight-gradient slab (rounded down to whole clips, at least one)

// d/dx mish(x) from the e = exp(min(x, 20)), n = e (e + 2) form of mishf: mish = x n / (n + 2), (n / (n + 2))' = 4 e (e + 1) / (n + 2)^2
__device__ __forceinline__ float mish_grad(float x) {
    const float e = __expf(fminf(x, 20.f));
    const float n = e * (e + 2.f), d = n + 2.f;
    const float g = n / d + x * (4.f * e * (e + 1.f)) / (d * d);
    return (x > 20.f) ? 1.f : g;
}

// ---------------------------------------------------------------------------------------------------------------- conv GEMM
// Row m of the flattened problem is (clip cb = m / mdiv, position q = m % mdiv).
//   A(m, tap, k) = A[(cb a_tp + q a_qm + a_qo + tap a_qt) lda + k]      (rows outside [0, a_rows) read as zero)
//   B(tap, k, n) = B[tap b_ts + k b_rs + n b_cs]
//   C(m, n)      = C[(cb c_tp + oq) ldc + n],  oq = q c_qm + c_qo;  rows with oq outside [0, c_tp) are not stored, rows within
//                  c_halo of either end of the clip are stored as zero.
// Epilogue: + bias[n], pre := v, act (1 Mish), * Mish'(gz), + C (accumulate).
struct CG {
    const float* A; int lda, a_tp, a_qm, a_qo, a_qt; long long a_rows;
    const float* B; long long b_ts, b_rs, b_cs;
    float* C; int ldc, c_tp, c_qm, c_qo, c_halo;
    int M, N, K, ntap, mdiv;
    const float* bias;
    float* pre;
    int act;
    const float* gz;
    int accumulate;
};

__global__ __launch_bounds__(256) void cgemm_kernel(CG p) {
    __shared__ float As[kStageFloats];      // [k][m]
    __shared__ float Bs[kStageFloats];      // [k][n]
    const int tid = threadIdx.x;
    const int n0 = blockIdx.x * TBN, m0 = blockIdx.y * TBM;
    // A: threads run along k (contiguous); each thread owns 8 rows whose clip-mapped row index is fixed across the reduction
    const int ak = tid & 31;
    long long arow[8];
#pragma unroll
    for (int e = 0; e < 8; ++e) {
        const int m = m0 + e * 8 + (tid >> 5);
        arow[e] = (m < p.M) ? (long long)(m / p.mdiv) * p.a_tp + (long long)(m % p.mdiv) * p.a_qm + p.a_qo : -(1ll << 40);
    }
    // B: threads run along whichever of (k, n) has the smaller stride in the weight tensor
    const bool b_nfast = p.b_cs <= p.b_rs;
    const int kchunks = (p.K + TBK - 1) / TBK, iters = p.ntap * kchunks;
    float ra[8], rb[8];
    Tile t;
    t.run<1>(As, Bs, 0, iters,
        [&](int it) __attribute__((always_inline)) {
            const int tap = it / kchunks, k0 = (it - tap * kchunks) * TBK;
            const float* Bt = p.B + tap * p.b_ts;
            const long long roff = (long long)tap * p.a_qt;
            const int gk = k0 + ak;
#pragma unroll
            for (int e = 0; e < 8; ++e) {
                const long long r = arow[e] + roff;
                ra[e] = (gk < p.K && r >= 0 && r < p.a_rows) ? p.A[r * p.lda + gk] : 0.f;
                int kb, n;
                stage_map(b_nfast, e, kb, n);
                const int gkb = k0 + kb, gn = n0 + n;
                rb[e] = (gkb < p.K && gn < p.N) ? Bt[gkb * p.b_rs + gn * p.b_cs] : 0.f;
            }
        },
        [&]() __attribute__((always_inline)) {
#pragma unroll
            for (int e = 0; e < 8; ++e) {
                int kb, n;
                stage_map(b_nfast, e, kb, n);
                As[stage_at(ak, e * 8 + (tid >> 5))] = ra[e];
                Bs[stage_at(kb, n)] = rb[e];
            }
        });
    const auto& acc = t.acc;
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const int m = m0 + t.row(i, r);
            if (m >= p.M) continue;
            const int oq = (m % p.mdiv) * p.c_qm + p.c_qo;
            if (oq < 0 || oq >= p.c_tp) continue;
            const bool halo = oq < p.c_halo || oq >= p.c_tp - p.c_halo;
            const long long crow = ((long long)(m / p.mdiv) * p.c_tp + oq) * p.ldc;
#pragma unroll
            for (int j = 0; j < 2; ++j) {
                const int n = n0 + t.col(j);
                if (n >= p.N) continue;
                const long long ci = crow + n;
                float v = acc[i][j][r];
                if (p.bias) v += p.bias[n];
                if (p.pre) p.pre[ci] = v;
                if (p.act == 1) v = mishf(v);
                if (p.gz) v *= mish_grad(p.gz[ci]);
                if (p.accumulate) v += p.C[ci];
                p.C[ci] = halo ? 0.f : v;
            }
        }
}

// ---------------------------------------------------------------------------------------------------------------- weight-gradient GEMM
// G[i g_is + j g_js + tap] = sum over the slab's rows m = (cb, q) of  L[(cb l_tp + q + l_qo) ldl + i] . P[(cb p_tp + q p_qm + p_qo + tap) ldp + j]
// (rows outside [0, l_rows) / [0, p_rows) read as zero).  blockIdx.z = slab * ntap + tap; slab s covers rows [s ms, (s + 1) ms) and
// writes G + s g_slab.
struct WG {
    const float* L; int ldl, l_tp, l_qo; long long l_rows;
    const float* P; int ldp, p_tp, p_qm, p_qo; long long p_rows;
    float* G; long long g_is, g_js, g_slab;
    int I, J, M, mdiv, ntap, ms;
};

__global__ __launch_bounds__(256) void wgemm_kernel(WG p) {
    __shared__ float As[kStageFloats];      // [row][i]
    __shared__ float Bs[kStageFloats];      // [row][j]
    const int tid = threadIdx.x;
    const int j0 = blockIdx.x * TBN, i0 = blockIdx.y * TBM;
    const int slab = blockIdx.z / p.ntap, tap = blockIdx.z % p.ntap;
    const int mbeg = slab * p.ms, mend = (mbeg + p.ms < p.M) ? mbeg + p.ms : p.M;
    const int c = tid & 63, kr = tid >> 6;      // threads run along the channels (contiguous); 4 rows per pass, 8 passes per chunk
    float ra[8], rb[8];
    Tile t;
    t.run<TBK>(As, Bs, mbeg, mend,
        [&](int mb) __attribute__((always_inline)) {
#pragma unroll
            for (int e = 0; e < 8; ++e) {
                const int m = mb + e * 4 + kr;
                float a = 0.f, b = 0.f;
                if (m < mend) {
                    const int cb = m / p.mdiv, q = m - cb * p.mdiv;
                    const long long rl = (long long)cb * p.l_tp + q + p.l_qo;
                    const long long rp = (long long)cb * p.p_tp + (long long)q * p.p_qm + p.p_qo + tap;
                    if (i0 + c < p.I && rl >= 0 && rl < p.l_rows) a = p.L[rl * p.ldl + i0 + c];
                    if (j0 + c < p.J && rp >= 0 && rp < p.p_rows) b = p.P[rp * p.ldp + j0 + c];
                }
                ra[e] = a;
                rb[e] = b;
            }
        },
        [&]() __attribute__((always_inline)) {
#pragma unroll
            for (int e = 0; e < 8; ++e) {
                As[stage_at(e * 4 + kr, c)] = ra[e];
                Bs[stage_at(e * 4 + kr, c)] = rb[e];
            }
        });
    const auto& acc = t.acc;
    float* G = p.G + (long long)slab * p.g_slab + tap;
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int j = 0; j < 2; ++j)
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const int gi = i0 + t.row(i, r), gj = j0 + t.col(j);
                if (gi < p.I && gj < p.J) G[gi * p.g_is + gj * p.g_js] = acc[i][j][r];
            }
}

// ---------------------------------------------------------------------------------------------------------------- GroupNorm + Mish
// All-threads sum of a 256-thread workgroup, the four wave sums added in wave order.
__device__ __forceinline__ float block_sum(float v, float* red) {
    v = wave_sum64(v);
    __syncthreads();
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
    __syncthreads();
    return ((red[0] + red[1]) + red[2]) + red[3];
}

// One workgroup per (group, sample): y = Mish(GroupNorm(x)) [+ tb[b][c]] [+ add], halo rows of y stored as zero; stats[b][g] = (mean, rstd).
// x: conv output [B, Tp, C]; y / add: row strides ldy / ldadd (add may alias y).
__global__ __launch_bounds__(256) void gn_mish_fwd_kernel(const float* __restrict__ x, const float* __restrict__ gam,
                                                          const float* __restrict__ bet, const float* __restrict__ tb, const float* add,
                                                          int ldadd, float* y, int ldy, float* __restrict__ stats, int C, int Tl,
                                                          float eps) {
    __shared__ float red[4];
    const int g = blockIdx.x, b = blockIdx.y, cpg = C / kGroups, Tp = Tl + 2 * kHalo;
    const int cl = threadIdx.x % cpg, ph = threadIdx.x / cpg, nph = 256 / cpg, ch = g * cpg + cl;
    const float* xb = x + ((long long)b * Tp + kHalo) * C + ch;
    float s = 0.f;
    for (int t = ph; t < Tl; t += nph) s += xb[(long long)t * C];
    const float inv_n = 1.0f / (float)(Tl * cpg);
    const float mean = block_sum(s, red) * inv_n;
    float ss = 0.f;
    for (int t = ph; t < Tl; t += nph) {
        const float d = xb[(long long)t * C] - mean;
        ss += d * d;
    }
    const float rstd = 1.0f / sqrtf(block_sum(ss, red) * inv_n + eps);
    if (threadIdx.x == 0) {
        stats[2 * (b * kGroups + g)] = mean;
        stats[2 * (b * kGroups + g) + 1] = rstd;
    }
    const float ga = gam[ch], be = bet[ch], tbv = tb ? tb[(long long)b * C + ch] : 0.f;
    for (int q = ph; q < Tp; q += nph) {
        const long long row = (long long)b * Tp + q;
        float v = 0.f;
        if (q >= kHalo && q < Tp - kHalo) {
            v = mishf((x[row * C + ch] - mean) * rstd * ga + be) + tbv;
            if (add) v += add[row * ldadd + ch];
        }
        y[row * ldy + ch] = v;
    }
}

// Backward of y = Mish(GroupNorm(x)) [+ tb]: dx (halo rows zero, row stride C) from dy (row stride ldy), the saved x and (mean, rstd);
// per-sample partials pg[b][c] = sum_t dz xhat, pb[b][c] = sum_t dz (z = xhat gamma + beta, dz = dy Mish'(z)) and, when ptb is given,
// ptb[b][c] = sum_t dy (the time bias' gradient).  Sums over t run per thread in t order and over the threads of a channel in thread order.
__global__ __launch_bounds__(256) void gn_mish_bwd_kernel(const float* __restrict__ dy, int ldy, const float* __restrict__ x,
                                                          const float* __restrict__ stats, const float* __restrict__ gam,
                                                          const float* __restrict__ bet, float* __restrict__ dx, float* __restrict__ pg,
                                                          float* __restrict__ pb, float* __restrict__ ptb, int C, int Tl) {
    __shared__ float red[4];
    __shared__ float ch_red[3][256];
    const int g = blockIdx.x, b = blockIdx.y, cpg = C / kGroups, Tp = Tl + 2 * kHalo;
    const int cl = threadIdx.x % cpg, ph = threadIdx.x / cpg, nph = 256 / cpg, ch = g * cpg + cl;
    const float mean = stats[2 * (b * kGroups + g)], rstd = stats[2 * (b * kGroups + g) + 1];
    const float ga = gam[ch], be = bet[ch];
    float sg = 0.f, sb = 0.f, st = 0.f;
    for (int t = ph; t < Tl; t += nph) {
        const long long row = (long long)b * Tp + kHalo + t;
        const float xh = (x[row * C + ch] - mean) * rstd;
        const float d = dy[row * ldy + ch];
        const float dz = d * mish_grad(xh * ga + be);
        sg += dz * xh;
        sb += dz;
        st += d;
    }
    const float inv_n = 1.0f / (float)(Tl * cpg);
    const float m1 = block_sum(sb * ga, red) * inv_n;      // mean of d xhat
    const float m2 = block_sum(sg * ga, red) * inv_n;      // mean of d xhat . xhat
    ch_red[0][threadIdx.x] = sg;
    ch_red[1][threadIdx.x] = sb;
    ch_red[2][threadIdx.x] = st;
    __syncthreads();
    if (ph == 0) {
        float a0 = sg, a1 = sb, a2 = st;
        for (int k = 1; k < nph; ++k) {
            a0 += ch_red[0][k * cpg + cl];
            a1 += ch_red[1][k * cpg + cl];
            a2 += ch_red[2][k * cpg + cl];
        }
        pg[(long long)b * C + ch] = a0;
        pb[(long long)b * C + ch] = a1;
        if (ptb) ptb[(long long)b * C + ch] = a2;
    }
    for (int q = ph; q < Tp; q += nph) {
        const long long row = (long long)b * Tp + q;
        float v = 0.f;
        if (q >= kHalo && q < Tp - kHalo) {
            const float xh = (x[row * C + ch] - mean) * rstd;
            const float dz = dy[row * ldy + ch] * mish_grad(xh * ga + be);
            v = rstd * (dz * ga - m1 - xh * m2);
        }
        dx[row * C + ch] = v;
    }
}

// ---------------------------------------------------------------------------------------------------------------- elementwise
// dst[r][c] (+)= src[r][c] for c < cols (row strides ldd / lds)
__global__ void copy_cols_kernel(const float* __restrict__ src, int lds, float* dst, int ldd, long long rows, int cols, int add) {
    const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= rows * cols) return;
    const long long r = i / cols;
    const int c = (int)(i % cols);
    const float v = src[r * lds + c];
    dst[r * ldd + c] = add ? dst[r * ldd + c] + v : v;
}

// [B, T, C] -> [B, T + 4, C] with zero halo rows
__global__ void pad_rows_kernel(const float* __restrict__ src, float* __restrict__ dst, int B, int Tl, int C) {
    const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    const int Tp = Tl + 2 * kHalo;
    if (i >= (long long)B * Tp * C) return;
    const int c = (int)(i % C);
    const long long r = i / C;
    const int q = (int)(r % Tp), b = (int)(r / Tp);
    dst[i] = (q >= kHalo && q < Tp - kHalo) ? src[((long long)b * Tl + q - kHalo) * C + c] : 0.f;
}

// SinusoidalPosEmb (model/heads.py:57-69): e[b] = (sin(t f_i), cos(t f_i)), f_i = exp(-i log(10000) / (half - 1))
__global__ void sinusoid_kernel(const int64_t* __restrict__ t, float* __restrict__ e, int B) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= B * kTdim) return;
    const int b = i / kTdim, j = i % kTdim, half = kTdim / 2;
    const float f = expf((float)(j % half) * -(logf(10000.f) / (float)(half - 1)));
    const float a = (float)t[b] * f;
    e[i] = j < half ? sinf(a) : cosf(a);
}

__global__ void mish_kernel(const float* __restrict__ x, float* __restrict__ y, long long n) {
    const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) y[i] = mishf(x[i]);
}
__global__ void mul_mish_grad_kernel(float* __restrict__ d, const float* __restrict__ z, long long n) {
    const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) d[i] *= mish_grad(z[i]);
}

// ---------------------------------------------------------------------------------------------------------------- network description
struct Par { const float* w = nullptr; float* g = nullptr; };
struct ConvP { Par w, b; int cin = 0, cout = 0, k = 0; };
struct BlkP { ConvP conv; Par gam, bet; };
struct ResP {
    BlkP b0, b1;
    Par tw, tb;
    ConvP res;
    bool has_t = false, has_res = false;
    int cin = 0, cout = 0;
};
struct Net {
    ConvP zc0, k_zero[4], k_down[4], k_zero_mid;
    ResP k_enc[4], k_mid[2];
    Par t_w1, t_b1, t_w3, t_b3;
    ResP d_enc[4], d_mid[2], dec[4], c_enc[4];
    ConvP d_down[4], up[4], c_down[4], fin1;
    BlkP fin;
};
struct Dims { int m, ct, cc, control, B, T; };

inline bool conv_g(const ConvP& c) { return c.w.g || c.b.g; }
inline bool blk_g(const BlkP& b) { return conv_g(b.conv) || b.gam.g || b.bet.g; }
inline bool res_g(const ResP& r) { return blk_g(r.b0) || blk_g(r.b1) || r.tw.g || r.tb.g || (r.has_res && conv_g(r.res)); }

// Walks the tensor table in the order of weight_order() (rohm_amd/model/trajnet.py); grads may be null (forward).
int parse_net(const rohm_trajnet_weights* wts, float* const* grads, const Dims& d, Net* net) {
    int cursor = 0;
    bool ok = true;
    auto next = [&](size_t n) -> Par {
        Par p;
        if (cursor >= wts->n_tensors) { ok = false; return p; }
        const rohm_tensor_ref& t = wts->tensors[cursor];
        if (t.numel != n || !t.data) { ok = false; return p; }
        p.w = t.data;
        p.g = grads ? grads[cursor] : nullptr;
        ++cursor;
        return p;
    };
    auto conv = [&](ConvP& c, int cout, int cin, int k) {
        c.cin = cin; c.cout = cout; c.k = k;
        c.w = next((size_t)cout * cin * k);
        c.b = next(cout);
    };
    auto blk = [&](BlkP& b, int cin, int cout) {
        conv(b.conv, cout, cin, 5);
        b.gam = next(cout);
        b.bet = next(cout);
    };
    auto res = [&](ResP& r, int cin, int cout, bool has_t) {
        r.cin = cin; r.cout = cout; r.has_t = has_t; r.has_res = cin != cout;
        blk(r.b0, cin, cout);
        blk(r.b1, cout, cout);
        if (has_t) { r.tw = next((size_t)cout * kTdim); r.tb = next(cout); }
        if (r.has_res) conv(r.res, cout, cin, 1);
    };
    const int m = d.m, ch[4] = {m / 8, m / 4, m / 2, m}, zo[4] = {32, m / 8, m / 4, m / 2};
    if (d.control) {
        conv(net->zc0, d.ct, d.cc, 1);
        int cin = d.ct;
        for (int i = 0; i < 4; ++i) {
            res(net->k_enc[i], cin, ch[i], true);
            conv(net->k_zero[i], zo[i], ch[i], 1);
            conv(net->k_down[i], 2 * ch[i], 2 * ch[i], 3);
            cin = 2 * ch[i];
        }
        res(net->k_mid[0], 2 * m, m, true);
        res(net->k_mid[1], m, m, true);
        conv(net->k_zero_mid, m, m, 1);
    }
    net->t_w1 = next((size_t)4 * kTdim * kTdim); net->t_b1 = next(4 * kTdim);
    net->t_w3 = next((size_t)4 * kTdim * kTdim); net->t_b3 = next(kTdim);
    int cin = d.ct;
    for (int i = 0; i < 4; ++i) {
        res(net->d_enc[i], cin, ch[i], true);
        conv(net->d_down[i], 2 * ch[i], 2 * ch[i], 3);
        cin = 2 * ch[i];
    }
    res(net->d_mid[0], 2 * m, m, true);
    res(net->d_mid[1], m, m, true);
    for (int i = 3; i >= 0; --i) {
        conv(net->up[i], ch[i], ch[i], 4);      // ConvTranspose1d [C_in, C_out, 4], C_in == C_out
        res(net->dec[i], 2 * ch[i], zo[i], true);
    }
    blk(net->fin, 32, 32);
    conv(net->fin1, d.ct, 32, 1);
    cin = d.ct;
    for (int i = 0; i < 4; ++i) {
        res(net->c_enc[i], cin, ch[i], false);
        conv(net->c_down[i], ch[i], ch[i], 3);      // cond_downsample4 is built but never called (model/trajnet.py:174)
        cin = ch[i];
    }
    if (!ok || cursor != wts->n_tensors) {
        set_error("trajnet training: the weight table does not match the architecture at tensor %d of %d (mid_dim=%d traj_feat_dim=%d "
                  "control_cond_dim=%d trajcontrol=%d)", cursor, wts->n_tensors, d.m, d.ct, d.cc, d.control);
        return ROHM_ERR_ARG;
    }
    return ROHM_OK;
}

int check_dims(int mid_dim, int time_dim, int c_traj, int c_ctrl, int trajcontrol, int B, int T, Dims* d) {
    if (mid_dim != kMid || time_dim != kTdim || c_traj < 1 || c_traj > 32 || c_ctrl < 1 || c_ctrl > kPadCtl || B < 1 || B > 16383 ||
        T < 16 || T % 16 != 0 || (long long)T * (mid_dim / 64) > 4096) {
        set_error("trajnet training: unsupported shape mid_dim=%d time_dim=%d traj_feat_dim=%d control_cond_dim=%d B=%d T=%d "
                  "(supported: mid_dim 512, time_dim 32, 1 <= traj_feat_dim <= 32, control_cond_dim <= %d, 1 <= B <= 16383, "
                  "T a multiple of 16 with T <= 512)", mid_dim, time_dim, c_traj, c_ctrl, B, T, kPadCtl);
        return ROHM_ERR_UNSUPPORTED;
    }
    d->m = mid_dim; d->ct = c_traj; d->cc = c_ctrl; d->control = trajcontrol ? 1 : 0; d->B = B; d->T = T;
    return ROHM_OK;
}

// ---------------------------------------------------------------------------------------------------------------- buffers
struct Geo {      // per level l = 0..4: T_l, padded rows per clip, rows in all; channel widths
    int Tl[5], Tp[5], ch[4], zo[4];
    long long R[5];
};
Geo geo(const Dims& d) {
    Geo g;
    for (int l = 0; l < 5; ++l) { g.Tl[l] = d.T >> l; g.Tp[l] = g.Tl[l] + 2 * kHalo; g.R[l] = (long long)d.B * g.Tp[l]; }
    const int m = d.m;
    g.ch[0] = m / 8; g.ch[1] = m / 4; g.ch[2] = m / 2; g.ch[3] = m;
    g.zo[0] = 32; g.zo[1] = m / 8; g.zo[2] = m / 4; g.zo[3] = m / 2;
    return g;
}

struct ResS { float *c0, *st0, *a0, *c1, *st1; };      // saved per residual block: both conv outputs with their statistics, block 0's activation
struct Saved {
    float *xin, *cin, *ctl;
    float *semb, *h1pre, *h1, *temb, *mt, *tbv;
    float *hc[4], *cdn[3];
    float *kz0, *kcat[4], *kz[4], *kdn[4], *kmid1, *kmid2, *kzmid;
    float *dcat[4], *ddn[4], *mid1, *mids;
    float *ucat[4], *dd[4];
    float *fc0, *fst, *fa;
    ResS r_c[4], r_k[4], r_km[2], r_d[4], r_dm[2], r_u[4];
    long long total;
};
struct Bump {
    float* base;
    long long q = 0;
    float* take(long long n) {
        float* p = base ? base + q : nullptr;
        q += (n + 63) / 64 * 64;
        return p;
    }
};
Saved map_saved(const Dims& d, float* base) {
    const Geo g = geo(d);
    Saved s;
    Bump b{base};
    const long long B = d.B;
    auto rs = [&](ResS& r, int l, int cout) {
        r.c0 = b.take(g.R[l] * cout); r.st0 = b.take(B * kGroups * 2); r.a0 = b.take(g.R[l] * cout);
        r.c1 = b.take(g.R[l] * cout); r.st1 = b.take(B * kGroups * 2);
    };
    s.xin = b.take(g.R[0] * d.ct); s.cin = b.take(g.R[0] * d.ct);
    s.ctl = d.control ? b.take(g.R[0] * d.cc) : nullptr;
    s.semb = b.take(B * kTdim); s.h1pre = b.take(B * 4 * kTdim); s.h1 = b.take(B * 4 * kTdim); s.temb = b.take(B * kTdim);
    s.mt = b.take(B * kTdim); s.tbv = b.take(B * d.m);
    for (int l = 0; l < 4; ++l) {
        s.hc[l] = b.take(g.R[l] * g.ch[l]);
        if (l < 3) s.cdn[l] = b.take(g.R[l + 1] * g.ch[l]);
        rs(s.r_c[l], l, g.ch[l]);
        s.dcat[l] = b.take(g.R[l] * 2 * g.ch[l]); s.ddn[l] = b.take(g.R[l + 1] * 2 * g.ch[l]);
        rs(s.r_d[l], l, g.ch[l]);
        s.ucat[l] = b.take(g.R[l] * 2 * g.ch[l]); s.dd[l] = b.take(g.R[l] * g.zo[l]);
        rs(s.r_u[l], l, g.zo[l]);
        if (d.control) {
            s.kcat[l] = b.take(g.R[l] * 2 * g.ch[l]); s.kz[l] = b.take(g.R[l] * g.zo[l]); s.kdn[l] = b.take(g.R[l + 1] * 2 * g.ch[l]);
            rs(s.r_k[l], l, g.ch[l]);
        }
    }
    s.mid1 = b.take(g.R[4] * d.m); s.mids = b.take(g.R[4] * d.m);
    rs(s.r_dm[0], 4, d.m); rs(s.r_dm[1], 4, d.m);
    if (d.control) {
        s.kz0 = b.take(g.R[0] * d.ct);
        s.kmid1 = b.take(g.R[4] * d.m); s.kmid2 = b.take(g.R[4] * d.m); s.kzmid = b.take(g.R[4] * d.m);
        rs(s.r_km[0], 4, d.m); rs(s.r_km[1], 4, d.m);
    }
    s.fc0 = b.take(g.R[0] * 32); s.fst = b.take(B * kGroups * 2); s.fa = b.take(g.R[0] * 32);
    s.total = b.q;
    return s;
}

int slab_clips(int mdiv) { const int c = kSlabRows / mdiv; return c < 1 ? 1 : c; }
int n_slabs(int B, int mdiv) { const int c = slab_clips(mdiv); return (B + c - 1) / c; }

struct GradBufs {
    float *t1, *t2;                          // block temporaries [R_l, C_out]
    float *pg, *pb, *ptb;                    // per-sample partials [B, C]
    float *part, *cpart;                     // weight-gradient slabs, column-sum chunks
    long long part_cap;
    float *g_s[4], *g_mid, *g_ucat[4];       // gradients at the decoder outputs (= at the control residuals), at the mid sum, at the decoder concats
    float *g_dcat[4], *g_ddn[4], *g_m1;      // diffusion encoder
    float *g_kcat[4], *g_kdn[4], *g_k5a, *g_k5b, *g_kz0;      // ControlNet
    float *g_hc[4], *g_cdn[3];               // cond encoder
    float *dmt, *dh1;                        // time path
    long long total;
};
GradBufs map_scratch(const Dims& d, float* base) {
    const Geo g = geo(d);
    GradBufs s;
    Bump b{base};
    const long long B = d.B;
    long long rc = g.R[4] * d.m, part = 0, rows = g.R[0];
    for (int l = 0; l < 5; ++l) {
        const long long w = g.ch[l < 4 ? l : 3];
        if (g.R[l] * w > rc) rc = g.R[l] * w;
        const long long need = (long long)n_slabs(d.B, g.Tp[l]) * 12 * w * w;      // the largest weight at a level is its down conv's
        if (need > part) part = need;
    }
    const long long zc = (long long)n_slabs(d.B, g.Tl[0]) * 64 * (d.cc > 64 * 5 ? d.cc : 64 * 5);      // 13-channel first convs, zero conv 0
    if (zc > part) part = zc;
    s.t1 = b.take(rc); s.t2 = b.take(rc);
    s.pg = b.take(B * d.m); s.pb = b.take(B * d.m); s.ptb = b.take(B * d.m);
    s.part = b.take(part); s.part_cap = part;
    s.cpart = b.take(((rows + kColRows - 1) / kColRows + 1) * 2 * d.m);
    for (int l = 0; l < 4; ++l) {
        s.g_s[l] = b.take(g.R[l] * g.zo[l]); s.g_ucat[l] = b.take(g.R[l] * 2 * g.ch[l]);
        s.g_dcat[l] = b.take(g.R[l] * 2 * g.ch[l]); s.g_ddn[l] = b.take(g.R[l + 1] * 2 * g.ch[l]);
        s.g_hc[l] = b.take(g.R[l] * g.ch[l]);
        if (l < 3) s.g_cdn[l] = b.take(g.R[l + 1] * g.ch[l]);
        if (d.control) { s.g_kcat[l] = b.take(g.R[l] * 2 * g.ch[l]); s.g_kdn[l] = b.take(g.R[l + 1] * 2 * g.ch[l]); }
    }
    s.g_mid = b.take(g.R[4] * d.m); s.g_m1 = b.take(g.R[4] * d.m);
    if (d.control) { s.g_k5a = b.take(g.R[4] * d.m); s.g_k5b = b.take(g.R[4] * d.m); s.g_kz0 = b.take(g.R[0] * d.ct); }
    s.dmt = b.take(B * kTdim); s.dh1 = b.take(B * 4 * kTdim);
    s.total = b.q;
    return s;
}

// ---------------------------------------------------------------------------------------------------------------- launches
// A padded activation [B, Tp, ld] (p already offset to its first channel), or, with unpadded set, a caller tensor [B, T, ld].
struct View { float* p; int ld; bool unpadded; };
inline View V(float* p, int ld) { return View{p, ld, false}; }
inline View VU(float* p, int ld) { return View{p, ld, true}; }

struct Ctx {
    Dims d;
    Geo g;
    hipStream_t s;
    GradBufs* sc = nullptr;      // backward only
    int gemms = 0;
};

int launch_cg(Ctx& c, const CG& p, const char* label) {
    if (p.M <= 0 || p.N <= 0) return ROHM_OK;
    prof::Scope ps(label, 2.0 * p.M * p.N * (double)p.K * p.ntap, 0.0, c.s);
    hipLaunchKernelGGL(cgemm_kernel, dim3((p.N + TBN - 1) / TBN, (p.M + TBM - 1) / TBM), dim3(256), 0, c.s, p);
    ROHM_LAUNCH_CHECK();
    ++c.gemms;
    return ROHM_OK;
}

CG cg_base(Ctx& c, View a, int la, int K, View out, int lo, int N) {      // A at level la, C at level lo
    CG p;
    memset(&p, 0, sizeof(p));
    p.A = a.p; p.lda = a.ld; p.a_tp = a.unpadded ? c.g.Tl[la] : c.g.Tp[la]; p.a_qm = 1; p.a_qo = a.unpadded ? -kHalo : 0; p.a_qt = 1;
    p.a_rows = (long long)c.d.B * p.a_tp;
    p.C = out.p; p.ldc = out.ld; p.c_tp = out.unpadded ? c.g.Tl[lo] : c.g.Tp[lo]; p.c_qm = 1; p.c_qo = out.unpadded ? -kHalo : 0;
    p.c_halo = out.unpadded ? 0 : kHalo;
    p.K = K; p.N = N; p.ntap = 1;
    return p;
}

// Y = conv(X) for a Conv1d(k in {1, 5}, stride 1, pad k / 2) at level l
int conv_fwd(Ctx& c, const ConvP& w, View x, View y, int l) {
    CG p = cg_base(c, x, l, w.cin, y, l, w.cout);
    p.M = (int)c.g.R[l]; p.mdiv = c.g.Tp[l];
    p.a_qo += -(w.k / 2);
    p.B = w.w.w; p.b_ts = 1; p.b_rs = w.k; p.b_cs = (long long)w.cin * w.k; p.ntap = w.k;
    p.bias = w.b.w;
    return launch_cg(c, p, "traj_train_conv");
}
// dX[:, :ncols] (+)= the data gradient of that conv: the same conv of dY with the taps mirrored
int conv_dgrad(Ctx& c, const ConvP& w, View dy, View dx, int ncols, int l, bool accumulate) {
    CG p = cg_base(c, dy, l, w.cout, dx, l, ncols);
    p.M = (int)c.g.R[l]; p.mdiv = c.g.Tp[l];
    p.a_qo += w.k / 2; p.a_qt = -1;
    p.B = w.w.w; p.b_ts = 1; p.b_rs = (long long)w.cin * w.k; p.b_cs = w.k; p.ntap = w.k;
    p.accumulate = accumulate ? 1 : 0;
    return launch_cg(c, p, "traj_train_conv_dx");
}
// Downsample1d = Conv1d(k3, s2, p1): level l -> l + 1
int down_fwd(Ctx& c, const ConvP& w, View x, View y, int l) {
    CG p = cg_base(c, x, l, w.cin, y, l + 1, w.cout);
    p.M = (int)c.g.R[l + 1]; p.mdiv = c.g.Tp[l + 1];
    p.a_qm = 2; p.a_qo = -3;
    p.B = w.w.w; p.b_ts = 1; p.b_rs = 3; p.b_cs = (long long)w.cin * 3; p.ntap = 3;
    p.bias = w.b.w;
    return launch_cg(c, p, "traj_train_down");
}
// its data gradient is a two-phase transposed conv: even input rows take tap 1, odd ones taps 0 and 2
int down_dgrad(Ctx& c, const ConvP& w, View dy, View dx, int ncols, int l) {
    for (int phase = 0; phase < 2; ++phase) {
        CG p = cg_base(c, dy, l + 1, w.cout, dx, l, ncols);
        p.M = (int)c.g.R[l + 1]; p.mdiv = c.g.Tp[l + 1];
        p.b_rs = (long long)w.cin * 3; p.b_cs = 3;
        if (phase == 0) { p.ntap = 1; p.a_qo = 0; p.B = w.w.w + 1; p.b_ts = 0; }
        else { p.ntap = 2; p.a_qo = 1; p.a_qt = -1; p.B = w.w.w; p.b_ts = 2; }
        p.c_qm = 2; p.c_qo = -2 + phase;
        int rc = launch_cg(c, p, "traj_train_down_dx");
        if (rc) return rc;
    }
    return ROHM_OK;
}
// Upsample1d = ConvTranspose1d(k4, s2, p1), weight [C_in, C_out, 4]: level l + 1 -> l, as two 2-tap phases
// (Y[2u] = X[u] W1 + X[u - 1] W3, Y[2u + 1] = X[u + 1] W0 + X[u] W2)
int up_fwd(Ctx& c, const ConvP& w, View x, View y, int l) {
    for (int phase = 0; phase < 2; ++phase) {
        CG p = cg_base(c, x, l + 1, w.cin, y, l, w.cout);
        p.M = (int)c.g.R[l + 1]; p.mdiv = c.g.Tp[l + 1];
        p.ntap = 2; p.a_qt = -1; p.a_qo = phase;
        p.B = w.w.w + (phase ? 0 : 1); p.b_ts = 2; p.b_rs = (long long)w.cout * 4; p.b_cs = 4;
        p.c_qm = 2; p.c_qo = -2 + phase;
        p.bias = w.b.w;
        int rc = launch_cg(c, p, "traj_train_up");
        if (rc) return rc;
    }
    return ROHM_OK;
}
// its data gradient is a stride-2 conv with four taps
int up_dgrad(Ctx& c, const ConvP& w, View dy, View dx, int l) {
    CG p = cg_base(c, dy, l, w.cout, dx, l + 1, w.cin);
    p.M = (int)c.g.R[l + 1]; p.mdiv = c.g.Tp[l + 1];
    p.a_qm = 2; p.a_qo = -3; p.ntap = 4;
    p.B = w.w.w; p.b_ts = 1; p.b_rs = 4; p.b_cs = (long long)w.cout * 4;
    return launch_cg(c, p, "traj_train_up_dx");
}
// plain [B, K] . W[N, K]^T (+ bias) on matrices without clips (the time path)
int lin_fwd(Ctx& c, const float* X, int K, const float* W, const float* bias, float* Y, int N, float* pre, int act) {
    CG p;
    memset(&p, 0, sizeof(p));
    p.A = X; p.lda = K; p.a_tp = c.d.B; p.a_qm = 1; p.a_qt = 1; p.a_rows = c.d.B;
    p.B = W; p.b_rs = 1; p.b_cs = K;
    p.C = Y; p.ldc = N; p.c_tp = c.d.B; p.c_qm = 1;
    p.M = c.d.B; p.mdiv = c.d.B; p.N = N; p.K = K; p.ntap = 1;
    p.bias = bias; p.pre = pre; p.act = act;
    return launch_cg(c, p, "traj_train_linear");
}
// dX[B, K] (+)= dY[B, N] . W[N, K], optionally * Mish'(gz)
int lin_dgrad(Ctx& c, const float* dY, int N, const float* W, float* dX, int K, const float* gz, bool accumulate) {
    CG p;
    memset(&p, 0, sizeof(p));
    p.A = dY; p.lda = N; p.a_tp = c.d.B; p.a_qm = 1; p.a_qt = 1; p.a_rows = c.d.B;
    p.B = W; p.b_rs = K; p.b_cs = 1;
    p.C = dX; p.ldc = K; p.c_tp = c.d.B; p.c_qm = 1;
    p.M = c.d.B; p.mdiv = c.d.B; p.N = K; p.K = N; p.ntap = 1;
    p.gz = gz; p.accumulate = accumulate ? 1 : 0;
    return launch_cg(c, p, "traj_train_linear_dx");
}

int launch_wg(Ctx& c, WG p, float* dW, long long wsize, int nclips, const char* label) {
    const int cps = slab_clips(p.mdiv), ns = (nclips + cps - 1) / cps;
    p.ms = cps * p.mdiv;
    p.g_slab = wsize;
    if (ns > 1 && (long long)ns * wsize > c.sc->part_cap) {
        set_error("trajnet training: weight-gradient slabs exceed the scratch plan (%d x %lld floats)", ns, wsize);
        return ROHM_ERR_ARG;
    }
    return slab_sum(ns, wsize, c.sc->part, dW, c.s, [&](float* dst) -> int {
        p.G = dst;
        prof::Scope ps(label, 2.0 * p.I * p.J * (double)p.M * p.ntap, 0.0, c.s);
        hipLaunchKernelGGL(wgemm_kernel, dim3((p.J + TBN - 1) / TBN, (p.I + TBM - 1) / TBM, ns * p.ntap), dim3(256), 0, c.s, p);
        ROHM_LAUNCH_CHECK();
        ++c.gemms;
        return ROHM_OK;
    });
}
// Gradients of a Conv1d's weight [C_out, C_in, k] and bias: dy at level ly (rows of the reduction), x at level lx; stride = 1 or 2
int conv_wgrad(Ctx& c, const ConvP& w, View dy, int ly, View x, int lx, int stride) {
    const int tpy = dy.unpadded ? c.g.Tl[ly] : c.g.Tp[ly];
    const long long rows = (long long)c.d.B * tpy;
    if (w.w.g) {
        WG p;
        memset(&p, 0, sizeof(p));
        p.L = dy.p; p.ldl = dy.ld; p.l_tp = tpy; p.l_qo = 0; p.l_rows = rows;
        p.P = x.p; p.ldp = x.ld; p.p_tp = c.g.Tp[lx]; p.p_qm = stride; p.p_rows = c.g.R[lx];
        p.p_qo = (stride == 2 ? -3 : -(w.k / 2)) + (dy.unpadded ? kHalo : 0);
        p.g_is = (long long)w.cin * w.k; p.g_js = w.k;
        p.I = w.cout; p.J = w.cin; p.M = (int)rows; p.mdiv = tpy; p.ntap = w.k;
        int rc = launch_wg(c, p, w.w.g, (long long)w.cout * w.cin * w.k, c.d.B, "traj_train_wgrad");
        if (rc) return rc;
    }
    if (w.b.g) return colsum(dy.p, 0, (int)rows, dy.ld, 1, (int)rows, w.cout, w.b.g, nullptr, c.sc->cpart, c.s);
    return ROHM_OK;
}
// ... of the ConvTranspose1d's weight [C_in, C_out, 4]: x at level l + 1 carries the reduction rows, dy at level l is read at 2 q - 3 + tap
int up_wgrad(Ctx& c, const ConvP& w, View dy, View x, int l) {
    if (w.w.g) {
        WG p;
        memset(&p, 0, sizeof(p));
        p.L = x.p; p.ldl = x.ld; p.l_tp = c.g.Tp[l + 1]; p.l_rows = c.g.R[l + 1];
        p.P = dy.p; p.ldp = dy.ld; p.p_tp = c.g.Tp[l]; p.p_qm = 2; p.p_qo = -3; p.p_rows = c.g.R[l];
        p.g_is = (long long)w.cout * 4; p.g_js = 4;
        p.I = w.cin; p.J = w.cout; p.M = (int)c.g.R[l + 1]; p.mdiv = c.g.Tp[l + 1]; p.ntap = 4;
        int rc = launch_wg(c, p, w.w.g, (long long)w.cin * w.cout * 4, c.d.B, "traj_train_wgrad");
        if (rc) return rc;
    }
    if (w.b.g) return colsum(dy.p, 0, (int)c.g.R[l], dy.ld, 1, (int)c.g.R[l], w.cout, w.b.g, nullptr, c.sc->cpart, c.s);
    return ROHM_OK;
}
// dW[N, K] = dY[B, N]^T . X[B, K] and db = column sums of dY over the samples (Linears of the time path)
int lin_wgrad(Ctx& c, const float* dY, int N, const float* X, int K, float* dW, float* db) {
    if (dW) {
        WG p;
        memset(&p, 0, sizeof(p));
        p.L = dY; p.ldl = N; p.l_tp = c.d.B; p.l_rows = c.d.B;
        p.P = X; p.ldp = K; p.p_tp = c.d.B; p.p_qm = 1; p.p_rows = c.d.B;
        p.g_is = K; p.g_js = 1;
        p.I = N; p.J = K; p.M = c.d.B; p.mdiv = c.d.B; p.ntap = 1;
        int rc = launch_wg(c, p, dW, (long long)N * K, 1, "traj_train_wgrad");
        if (rc) return rc;
    }
    if (db) return colsum(dY, 0, c.d.B, N, 1, c.d.B, N, db, nullptr, c.sc->cpart, c.s);
    return ROHM_OK;
}

int copy_cols(Ctx& c, const float* src, int lds, float* dst, int ldd, long long rows, int cols, bool add) {
    hipLaunchKernelGGL(copy_cols_kernel, dim3(blocks(rows * cols, 256)), dim3(256), 0, c.s, src, lds, dst, ldd, rows, cols, add ? 1 : 0);
    ROHM_LAUNCH_CHECK();
    return ROHM_OK;
}

int gn_fwd(Ctx& c, const BlkP& b, const float* x, const float* tb, const float* add, int ldadd, View y, float* stats, int l) {
    const int C = b.conv.cout;
    prof::Scope ps("traj_train_gn_mish", 0.0, 0.0, c.s);
    hipLaunchKernelGGL(gn_mish_fwd_kernel, dim3(kGroups, c.d.B), dim3(256), 0, c.s, x, b.gam.w, b.bet.w, tb, add, ldadd, y.p, y.ld, stats,
                       C, c.g.Tl[l], 1e-5f);
    ROHM_LAUNCH_CHECK();
    return ROHM_OK;
}
// dx (contiguous [R_l, C]) and the GroupNorm parameter gradients; ptb (optional) receives the per-sample sums of dy
int gn_bwd(Ctx& c, const BlkP& b, View dy, const float* x, const float* stats, float* dx, float* ptb, int l) {
    const int C = b.conv.cout;
    {
        prof::Scope ps("traj_train_gn_mish_bwd", 0.0, 0.0, c.s);
        hipLaunchKernelGGL(gn_mish_bwd_kernel, dim3(kGroups, c.d.B), dim3(256), 0, c.s, dy.p, dy.ld, x, stats, b.gam.w, b.bet.w, dx,
                           c.sc->pg, c.sc->pb, ptb, C, c.g.Tl[l]);
        ROHM_LAUNCH_CHECK();
    }
    int rc;
    if (b.gam.g && (rc = colsum(c.sc->pg, 0, c.d.B, C, 1, c.d.B, C, b.gam.g, nullptr, c.sc->cpart, c.s))) return rc;
    if (b.bet.g && (rc = colsum(c.sc->pb, 0, c.d.B, C, 1, c.d.B, C, b.bet.g, nullptr, c.sc->cpart, c.s))) return rc;
    return ROHM_OK;
}

// ResidualTemporalBlock (model/heads.py:12-54) at level l: out = block1(block0(x) + time_mlp(temb)) + residual(x)
int res_fwd(Ctx& c, const ResP& r, View x, View out, const ResS& sv, const Saved& S, int l) {
    int rc;
    if ((rc = conv_fwd(c, r.b0.conv, x, V(sv.c0, r.cout), l))) return rc;
    if (r.has_t && (rc = lin_fwd(c, S.mt, kTdim, r.tw.w, r.tb.w, S.tbv, r.cout, nullptr, 0))) return rc;
    if ((rc = gn_fwd(c, r.b0, sv.c0, r.has_t ? S.tbv : nullptr, nullptr, 0, V(sv.a0, r.cout), sv.st0, l))) return rc;
    if ((rc = conv_fwd(c, r.b1.conv, V(sv.a0, r.cout), V(sv.c1, r.cout), l))) return rc;
    if (r.has_res) {
        if ((rc = conv_fwd(c, r.res, x, out, l))) return rc;
        return gn_fwd(c, r.b1, sv.c1, nullptr, out.p, out.ld, out, sv.st1, l);
    }
    return gn_fwd(c, r.b1, sv.c1, nullptr, x.p, x.ld, out, sv.st1, l);
}

// Its backward.  d_out: gradient at the block's output; when want_dx, dx[:, :dx_cols] receives the input's gradient (dx_cols <
// C_in: only the leading channels of a concat are wanted).  want_t: the time embedding's gradient is wanted (accumulated into dmt).
int res_bwd(Ctx& c, const ResP& r, View x, View d_out, const ResS& sv, const Saved& S, int l, bool want_dx, View dx, int dx_cols,
            bool want_t) {
    int rc;
    GradBufs& k = *c.sc;
    const bool time_g = r.has_t && (r.tw.g || r.tb.g || want_t);
    const bool up0 = want_dx || blk_g(r.b0) || time_g;
    if (up0 || blk_g(r.b1)) {
        if ((rc = gn_bwd(c, r.b1, d_out, sv.c1, sv.st1, k.t1, nullptr, l))) return rc;
        if ((rc = conv_wgrad(c, r.b1.conv, V(k.t1, r.cout), l, V(sv.a0, r.cout), l, 1))) return rc;
    }
    if (up0) {
        if ((rc = conv_dgrad(c, r.b1.conv, V(k.t1, r.cout), V(k.t2, r.cout), r.cout, l, false))) return rc;
        if ((rc = gn_bwd(c, r.b0, V(k.t2, r.cout), sv.c0, sv.st0, k.t1, time_g ? k.ptb : nullptr, l))) return rc;
        if (time_g) {
            if ((rc = lin_wgrad(c, k.ptb, r.cout, S.mt, kTdim, r.tw.g, r.tb.g))) return rc;
            if (want_t && (rc = lin_dgrad(c, k.ptb, r.cout, r.tw.w, k.dmt, kTdim, nullptr, true))) return rc;
        }
        if ((rc = conv_wgrad(c, r.b0.conv, V(k.t1, r.cout), l, x, l, 1))) return rc;
        if (want_dx && (rc = conv_dgrad(c, r.b0.conv, V(k.t1, r.cout), dx, dx_cols, l, false))) return rc;
    }
    if (r.has_res) {
        if ((rc = conv_wgrad(c, r.res, d_out, l, x, l, 1))) return rc;
        if (want_dx && (rc = conv_dgrad(c, r.res, d_out, dx, dx_cols, l, true))) return rc;
    } else if (want_dx) {
        if ((rc = copy_cols(c, d_out.p, d_out.ld, dx.p, dx.ld, c.g.R[l], dx_cols, true))) return rc;
    }
    return ROHM_OK;
}

// ================================================================================================================ forward
int train_forward(Ctx& c, const Net& n, const float* x_t, const float* cond, const float* ctl, const int64_t* t, float* out,
                  const Saved& S) {
    const Dims& d = c.d;
    const Geo& g = c.g;
    const int B = d.B;
    int rc;
    auto pad = [&](const float* src, float* dst, int C) {
        hipLaunchKernelGGL(pad_rows_kernel, dim3(blocks(g.R[0] * C, 256)), dim3(256), 0, c.s, src, dst, B, d.T, C);
    };
    pad(x_t, S.xin, d.ct);
    pad(cond, S.cin, d.ct);
    if (d.control) pad(ctl, S.ctl, d.cc);
    ROHM_LAUNCH_CHECK();
    // ---- time path (model/trajnet.py:120-125): sinusoid -> Linear -> Mish -> Linear; every block applies Mish to it first
    hipLaunchKernelGGL(sinusoid_kernel, dim3(blocks((long long)B * kTdim, 256)), dim3(256), 0, c.s, t, S.semb, B);
    ROHM_LAUNCH_CHECK();
    if ((rc = lin_fwd(c, S.semb, kTdim, n.t_w1.w, n.t_b1.w, S.h1, 4 * kTdim, S.h1pre, 1))) return rc;
    if ((rc = lin_fwd(c, S.h1, 4 * kTdim, n.t_w3.w, n.t_b3.w, S.temb, kTdim, nullptr, 0))) return rc;
    hipLaunchKernelGGL(mish_kernel, dim3(blocks((long long)B * kTdim, 256)), dim3(256), 0, c.s, S.temb, S.mt, (long long)B * kTdim);
    ROHM_LAUNCH_CHECK();
    // ---- cond encoder (model/trajnet.py:192-208); h_cond[l] also goes into the concat inputs of the two down-conv chains
    for (int l = 0; l < 4; ++l) {
        const int w = g.ch[l];
        if ((rc = res_fwd(c, n.c_enc[l], l == 0 ? V(S.cin, d.ct) : V(S.cdn[l - 1], g.ch[l - 1]), V(S.hc[l], w), S.r_c[l], S, l))) return rc;
        if ((rc = copy_cols(c, S.hc[l], w, S.dcat[l] + w, 2 * w, g.R[l], w, false))) return rc;
        if (d.control && (rc = copy_cols(c, S.hc[l], w, S.kcat[l] + w, 2 * w, g.R[l], w, false))) return rc;
        if (l < 3 && (rc = down_fwd(c, n.c_down[l], V(S.hc[l], w), V(S.cdn[l], w), l))) return rc;
    }
    // ---- ControlNet (model/trajnet.py:43-75)
    if (d.control) {
        if ((rc = conv_fwd(c, n.zc0, V(S.ctl, d.cc), V(S.kz0, d.ct), 0))) return rc;
        for (int l = 0; l < 4; ++l) {
            const int w = g.ch[l];
            if ((rc = res_fwd(c, n.k_enc[l], l == 0 ? V(S.kz0, d.ct) : V(S.kdn[l - 1], 2 * g.ch[l - 1]), V(S.kcat[l], 2 * w), S.r_k[l], S, l)))
                return rc;
            if ((rc = conv_fwd(c, n.k_zero[l], V(S.kcat[l], 2 * w), V(S.kz[l], g.zo[l]), l))) return rc;
            if ((rc = down_fwd(c, n.k_down[l], V(S.kcat[l], 2 * w), V(S.kdn[l], 2 * w), l))) return rc;
        }
        if ((rc = res_fwd(c, n.k_mid[0], V(S.kdn[3], 2 * d.m), V(S.kmid1, d.m), S.r_km[0], S, 4))) return rc;
        if ((rc = res_fwd(c, n.k_mid[1], V(S.kmid1, d.m), V(S.kmid2, d.m), S.r_km[1], S, 4))) return rc;
        if ((rc = conv_fwd(c, n.k_zero_mid, V(S.kmid2, d.m), V(S.kzmid, d.m), 4))) return rc;
    }
    // ---- diffusion encoder and mid blocks (model/trajnet.py:220-240)
    for (int l = 0; l < 4; ++l) {
        const int w = g.ch[l];
        if ((rc = res_fwd(c, n.d_enc[l], l == 0 ? V(S.xin, d.ct) : V(S.ddn[l - 1], 2 * g.ch[l - 1]), V(S.dcat[l], 2 * w), S.r_d[l], S, l)))
            return rc;
        if ((rc = copy_cols(c, S.dcat[l], 2 * w, S.ucat[l] + w, 2 * w, g.R[l], w, false))) return rc;      // the decoder's skip half
        if ((rc = down_fwd(c, n.d_down[l], V(S.dcat[l], 2 * w), V(S.ddn[l], 2 * w), l))) return rc;
    }
    if ((rc = res_fwd(c, n.d_mid[0], V(S.ddn[3], 2 * d.m), V(S.mid1, d.m), S.r_dm[0], S, 4))) return rc;
    if ((rc = res_fwd(c, n.d_mid[1], V(S.mid1, d.m), V(S.mids, d.m), S.r_dm[1], S, 4))) return rc;
    if (d.control && (rc = copy_cols(c, S.kzmid, d.m, S.mids, d.m, g.R[4], d.m, true))) return rc;
    // ---- decoder (model/trajnet.py:243-271)
    for (int l = 3; l >= 0; --l) {
        const int w = g.ch[l];
        if ((rc = up_fwd(c, n.up[l], l == 3 ? V(S.mids, d.m) : V(S.dd[l + 1], g.zo[l + 1]), V(S.ucat[l], 2 * w), l))) return rc;
        if ((rc = res_fwd(c, n.dec[l], V(S.ucat[l], 2 * w), V(S.dd[l], g.zo[l]), S.r_u[l], S, l))) return rc;
        if (d.control && (rc = copy_cols(c, S.kz[l], g.zo[l], S.dd[l], g.zo[l], g.R[l], g.zo[l], true))) return rc;
    }
    // ---- final Conv1dBlock(32, 32) + 1x1 conv (model/trajnet.py:273-275)
    if ((rc = conv_fwd(c, n.fin.conv, V(S.dd[0], 32), V(S.fc0, 32), 0))) return rc;
    if ((rc = gn_fwd(c, n.fin, S.fc0, nullptr, nullptr, 0, V(S.fa, 32), S.fst, 0))) return rc;
    return conv_fwd(c, n.fin1, V(S.fa, 32), VU(out, d.ct), 0);
}

// ================================================================================================================ backward
int train_backward(Ctx& c, const Net& n, const Saved& S, const float* d_out, float* d_x_t, float* d_cond, float* d_ctl) {
    const Dims& d = c.d;
    const Geo& g = c.g;
    GradBufs& k = *c.sc;
    const int B = d.B;
    int rc;
    // ---- what lies upstream of each tensor: a data gradient is propagated only where a trainable parameter or a wanted input is
    const bool Ut = n.t_w1.g || n.t_b1.g || n.t_w3.g || n.t_b3.g;
    bool Uhc[4], Uke[4] = {false, false, false, false}, Ukin[5] = {false, false, false, false, false};
    bool Uco[5] = {false, false, false, false, false}, Ude[4], Udin[5], Us[4], Uup[4];
    bool Ukz0 = false, Ukm1 = false, Ukm2 = false;
    bool u = d_cond != nullptr;
    for (int l = 0; l < 4; ++l) {
        if (l > 0) u = u || conv_g(n.c_down[l - 1]);
        u = u || res_g(n.c_enc[l]);
        Uhc[l] = u;
    }
    if (d.control) {
        Ukz0 = d_ctl != nullptr || conv_g(n.zc0);
        Ukin[0] = Ukz0;
        for (int l = 0; l < 4; ++l) {
            Uke[l] = Ukin[l] || res_g(n.k_enc[l]) || Ut;
            Uco[l] = Uke[l] || conv_g(n.k_zero[l]);
            Ukin[l + 1] = Uke[l] || Uhc[l] || conv_g(n.k_down[l]);
        }
        Ukm1 = Ukin[4] || res_g(n.k_mid[0]) || Ut;
        Ukm2 = Ukm1 || res_g(n.k_mid[1]) || Ut;
        Uco[4] = Ukm2 || conv_g(n.k_zero_mid);
    }
    Udin[0] = d_x_t != nullptr;
    for (int l = 0; l < 4; ++l) {
        Ude[l] = Udin[l] || res_g(n.d_enc[l]) || Ut;
        Udin[l + 1] = Ude[l] || Uhc[l] || conv_g(n.d_down[l]);
    }
    const bool Um1 = Udin[4] || res_g(n.d_mid[0]) || Ut, Um2 = Um1 || res_g(n.d_mid[1]) || Ut;
    const bool Umid = Um2 || Uco[4];
    for (int l = 3; l >= 0; --l) {
        Uup[l] = (l == 3 ? Umid : Us[l + 1]) || conv_g(n.up[l]);
        Us[l] = Uup[l] || Ude[l] || res_g(n.dec[l]) || Ut || Uco[l];
    }
    if (Ut) ROHM_HIP_CHECK(hipMemsetAsync(k.dmt, 0, sizeof(float) * (size_t)B * kTdim, c.s));
    // ---- final 1x1 conv and Conv1dBlock
    const View dov = VU(const_cast<float*>(d_out), d.ct);
    if ((rc = conv_wgrad(c, n.fin1, dov, 0, V(S.fa, 32), 0, 1))) return rc;
    if (!(Us[0] || blk_g(n.fin))) return ROHM_OK;
    if ((rc = conv_dgrad(c, n.fin1, dov, V(k.t2, 32), 32, 0, false))) return rc;
    if ((rc = gn_bwd(c, n.fin, V(k.t2, 32), S.fc0, S.fst, k.t1, nullptr, 0))) return rc;
    if ((rc = conv_wgrad(c, n.fin.conv, V(k.t1, 32), 0, V(S.dd[0], 32), 0, 1))) return rc;
    if (!Us[0]) return ROHM_OK;
    if ((rc = conv_dgrad(c, n.fin.conv, V(k.t1, 32), V(k.g_s[0], 32), 32, 0, false))) return rc;
    // ---- decoder, level 1 to 4: g_s[l] is the gradient at dec_l's output and at the control residual added to it
    for (int l = 0; l < 4; ++l) {
        if (!Us[l]) break;
        const int w = g.ch[l];
        const bool want = Uup[l] || Ude[l];
        if ((rc = res_bwd(c, n.dec[l], V(S.ucat[l], 2 * w), V(k.g_s[l], g.zo[l]), S.r_u[l], S, l, want, V(k.g_ucat[l], 2 * w),
                          Ude[l] ? 2 * w : w, Ut)))
            return rc;
        if (!Uup[l]) break;
        const View xin = l == 3 ? V(S.mids, d.m) : V(S.dd[l + 1], g.zo[l + 1]);
        if ((rc = up_wgrad(c, n.up[l], V(k.g_ucat[l], 2 * w), xin, l))) return rc;
        const bool want_in = l == 3 ? Umid : Us[l + 1];
        if (want_in && (rc = up_dgrad(c, n.up[l], V(k.g_ucat[l], 2 * w), l == 3 ? V(k.g_mid, d.m) : V(k.g_s[l + 1], g.zo[l + 1]), l)))
            return rc;
    }
    // ---- ControlNet: the gradient at control residual l is g_s[l] (g_mid for the mid one)
    if (d.control) {
        if (Uco[4]) {
            if ((rc = conv_wgrad(c, n.k_zero_mid, V(k.g_mid, d.m), 4, V(S.kmid2, d.m), 4, 1))) return rc;
            if (Ukm2) {
                if ((rc = conv_dgrad(c, n.k_zero_mid, V(k.g_mid, d.m), V(k.g_k5a, d.m), d.m, 4, false))) return rc;
                if ((rc = res_bwd(c, n.k_mid[1], V(S.kmid1, d.m), V(k.g_k5a, d.m), S.r_km[1], S, 4, Ukm1, V(k.g_k5b, d.m), d.m, Ut)))
                    return rc;
                if (Ukm1 && (rc = res_bwd(c, n.k_mid[0], V(S.kdn[3], 2 * d.m), V(k.g_k5b, d.m), S.r_km[0], S, 4, Ukin[4],
                                          V(k.g_kdn[3], 2 * d.m), 2 * d.m, Ut)))
                    return rc;
            }
        }
        for (int l = 3; l >= 0; --l) {
            const int w = g.ch[l];
            bool written = false;      // g_kcat[l][:, :w], the gradient at control_enc_l's output
            if (Ukin[l + 1]) {
                if ((rc = conv_wgrad(c, n.k_down[l], V(k.g_kdn[l], 2 * w), l + 1, V(S.kcat[l], 2 * w), l, 2))) return rc;
                if (Uke[l] || Uhc[l]) {
                    if ((rc = down_dgrad(c, n.k_down[l], V(k.g_kdn[l], 2 * w), V(k.g_kcat[l], 2 * w), Uhc[l] ? 2 * w : w, l))) return rc;
                    written = true;
                }
            }
            if (Uco[l]) {
                if ((rc = conv_wgrad(c, n.k_zero[l], V(k.g_s[l], g.zo[l]), l, V(S.kcat[l], 2 * w), l, 1))) return rc;
                if (Uke[l]) {
                    if ((rc = conv_dgrad(c, n.k_zero[l], V(k.g_s[l], g.zo[l]), V(k.g_kcat[l], 2 * w), w, l, written))) return rc;
                    written = true;
                }
            }
            if (Uke[l] && written) {
                const View xin = l == 0 ? V(S.kz0, d.ct) : V(S.kdn[l - 1], 2 * g.ch[l - 1]);
                const View dxv = l == 0 ? V(k.g_kz0, d.ct) : V(k.g_kdn[l - 1], 2 * g.ch[l - 1]);
                if ((rc = res_bwd(c, n.k_enc[l], xin, V(k.g_kcat[l], 2 * w), S.r_k[l], S, l, Ukin[l], dxv, n.k_enc[l].cin, Ut))) return rc;
            }
        }
        if (Ukz0) {
            if ((rc = conv_wgrad(c, n.zc0, V(k.g_kz0, d.ct), 0, V(S.ctl, d.cc), 0, 1))) return rc;
            if (d_ctl && (rc = conv_dgrad(c, n.zc0, V(k.g_kz0, d.ct), VU(d_ctl, d.cc), d.cc, 0, false))) return rc;
        }
    }
    // ---- diffusion mid blocks and encoder
    if (Um2) {
        if ((rc = res_bwd(c, n.d_mid[1], V(S.mid1, d.m), V(k.g_mid, d.m), S.r_dm[1], S, 4, Um1, V(k.g_m1, d.m), d.m, Ut))) return rc;
        if (Um1 && (rc = res_bwd(c, n.d_mid[0], V(S.ddn[3], 2 * d.m), V(k.g_m1, d.m), S.r_dm[0], S, 4, Udin[4], V(k.g_ddn[3], 2 * d.m),
                                 2 * d.m, Ut)))
            return rc;
    }
    for (int l = 3; l >= 0; --l) {
        const int w = g.ch[l];
        if (Udin[l + 1]) {
            if ((rc = conv_wgrad(c, n.d_down[l], V(k.g_ddn[l], 2 * w), l + 1, V(S.dcat[l], 2 * w), l, 2))) return rc;
            if ((Ude[l] || Uhc[l]) && (rc = down_dgrad(c, n.d_down[l], V(k.g_ddn[l], 2 * w), V(k.g_dcat[l], 2 * w), Uhc[l] ? 2 * w : w, l)))
                return rc;
        }
        if (!Ude[l]) continue;
        // Ude[l] implies Udin[l + 1] and Us[l]: both halves of the encoder output's gradient exist
        if ((rc = copy_cols(c, k.g_ucat[l] + w, 2 * w, k.g_dcat[l], 2 * w, g.R[l], w, true))) return rc;
        const View xin = l == 0 ? V(S.xin, d.ct) : V(S.ddn[l - 1], 2 * g.ch[l - 1]);
        const View dxv = l == 0 ? VU(d_x_t, d.ct) : V(k.g_ddn[l - 1], 2 * g.ch[l - 1]);
        if ((rc = res_bwd(c, n.d_enc[l], xin, V(k.g_dcat[l], 2 * w), S.r_d[l], S, l, Udin[l], dxv, n.d_enc[l].cin, Ut))) return rc;
    }
    // ---- cond encoder: h_cond[l] feeds the diffusion down conv, the control down conv and the next cond level
    for (int l = 3; l >= 0; --l) {
        if (!Uhc[l]) continue;
        const int w = g.ch[l];
        bool written = false;
        if (l < 3) {      // Uhc[l] implies Uhc[l + 1]: g_cdn[l] exists
            if ((rc = conv_wgrad(c, n.c_down[l], V(k.g_cdn[l], w), l + 1, V(S.hc[l], w), l, 2))) return rc;
            if ((rc = down_dgrad(c, n.c_down[l], V(k.g_cdn[l], w), V(k.g_hc[l], w), w, l))) return rc;
            written = true;
        }
        if ((rc = copy_cols(c, k.g_dcat[l] + w, 2 * w, k.g_hc[l], w, g.R[l], w, written))) return rc;
        if (d.control && (rc = copy_cols(c, k.g_kcat[l] + w, 2 * w, k.g_hc[l], w, g.R[l], w, true))) return rc;
        const View xin = l == 0 ? V(S.cin, d.ct) : V(S.cdn[l - 1], g.ch[l - 1]);
        const bool want = l == 0 ? d_cond != nullptr : Uhc[l - 1];
        const View dxv = l == 0 ? VU(d_cond, d.ct) : V(k.g_cdn[l - 1], g.ch[l - 1]);
        if ((rc = res_bwd(c, n.c_enc[l], xin, V(k.g_hc[l], w), S.r_c[l], S, l, want, dxv, n.c_enc[l].cin, false))) return rc;
    }
    // ---- time MLP: dmt holds the gradient at Mish(temb) summed over the blocks
    if (Ut) {
        hipLaunchKernelGGL(mul_mish_grad_kernel, dim3(blocks((long long)B * kTdim, 256)), dim3(256), 0, c.s, k.dmt, S.temb,
                           (long long)B * kTdim);
        ROHM_LAUNCH_CHECK();
        if ((rc = lin_wgrad(c, k.dmt, kTdim, S.h1, 4 * kTdim, n.t_w3.g, n.t_b3.g))) return rc;
        if (n.t_w1.g || n.t_b1.g) {
            if ((rc = lin_dgrad(c, k.dmt, kTdim, n.t_w3.w, k.dh1, 4 * kTdim, S.h1pre, false))) return rc;
            if ((rc = lin_wgrad(c, k.dh1, 4 * kTdim, S.semb, kTdim, n.t_w1.g, n.t_b1.g))) return rc;
        }
    }
    return ROHM_OK;
}

std::atomic<int> g_last_gemms{0};      // autograd runs the backward on a thread of its own: process-wide

}  // namespace
}  // namespace rohm

using namespace rohm;

extern "C" size_t rohm_trajnet_train_saved_bytes(int mid_dim, int time_dim, int c_traj, int c_ctrl, int trajcontrol, int B, int T) {
    Dims d;
    if (check_dims(mid_dim, time_dim, c_traj, c_ctrl, trajcontrol, B, T, &d)) return 0;
    return (size_t)map_saved(d, nullptr).total * sizeof(float);
}

extern "C" size_t rohm_trajnet_train_scratch_bytes(int mid_dim, int time_dim, int c_traj, int c_ctrl, int trajcontrol, int B, int T) {
    Dims d;
    if (check_dims(mid_dim, time_dim, c_traj, c_ctrl, trajcontrol, B, T, &d)) return 0;
    return (size_t)map_scratch(d, nullptr).total * sizeof(float);
}

extern "C" int rohm_trajnet_train_forward(const rohm_trajnet_weights* w, int mid_dim, int time_dim, int c_traj, int c_ctrl,
                                          int trajcontrol, const float* x_t, const float* cond, const float* control_cond,
                                          const int64_t* t, int B, int T, float* out, void* saved, size_t saved_bytes,
                                          rohm_stream_t stream) {
    Ctx c;
    int rc = check_dims(mid_dim, time_dim, c_traj, c_ctrl, trajcontrol, B, T, &c.d);
    if (rc) return rc;
    ROHM_ARG_CHECK(w && w->tensors && x_t && cond && t && out && saved, "rohm_trajnet_train_forward: null argument");
    ROHM_ARG_CHECK(!trajcontrol || control_cond, "rohm_trajnet_train_forward: TrajControl needs control_cond");
    ROHM_ARG_CHECK(aligned16(saved), "rohm_trajnet_train_forward: saved must be 16-byte aligned");
    const Saved S = map_saved(c.d, static_cast<float*>(saved));
    ROHM_ARG_CHECK(saved_bytes >= (size_t)S.total * sizeof(float), "rohm_trajnet_train_forward: saved buffer too small");
    Net net;
    if ((rc = parse_net(w, nullptr, c.d, &net))) return rc;
    c.g = geo(c.d);
    c.s = static_cast<hipStream_t>(stream);
    return train_forward(c, net, x_t, cond, control_cond, t, out, S);
}

extern "C" int rohm_trajnet_train_backward(const rohm_trajnet_weights* w, int mid_dim, int time_dim, int c_traj, int c_ctrl,
                                           int trajcontrol, int B, int T, const void* saved, size_t saved_bytes, const float* d_out,
                                           float* const* grads, float* d_x_t, float* d_cond, float* d_control_cond, void* scratch,
                                           size_t scratch_bytes, rohm_stream_t stream) {
    Ctx c;
    int rc = check_dims(mid_dim, time_dim, c_traj, c_ctrl, trajcontrol, B, T, &c.d);
    if (rc) return rc;
    ROHM_ARG_CHECK(w && w->tensors && grads && saved && d_out && scratch, "rohm_trajnet_train_backward: null argument");
    ROHM_ARG_CHECK(trajcontrol || !d_control_cond, "rohm_trajnet_train_backward: d_control_cond without TrajControl");
    ROHM_ARG_CHECK(aligned16(saved) && aligned16(scratch), "rohm_trajnet_train_backward: saved / scratch must be 16-byte aligned");
    const Saved S = map_saved(c.d, static_cast<float*>(const_cast<void*>(saved)));
    GradBufs sc = map_scratch(c.d, static_cast<float*>(scratch));
    ROHM_ARG_CHECK(saved_bytes >= (size_t)S.total * sizeof(float), "rohm_trajnet_train_backward: saved buffer too small");
    ROHM_ARG_CHECK(scratch_bytes >= (size_t)sc.total * sizeof(float), "rohm_trajnet_train_backward: scratch too small");
    Net net;
    if ((rc = parse_net(w, grads, c.d, &net))) return rc;
    ROHM_ARG_CHECK(!net.c_down[3].w.g && !net.c_down[3].b.g,
                   "rohm_trajnet_train_backward: cond_downsample4 is never called and has no gradient (pass NULL)");
    c.g = geo(c.d);
    c.s = static_cast<hipStream_t>(stream);
    c.sc = &sc;
    rc = train_backward(c, net, S, d_out, d_x_t, d_cond, d_control_cond);
    g_last_gemms.store(c.gemms);
    return rc;
}

extern "C" int rohm_trajnet_train_last_gemms(void) { return g_last_gemms.load(); }
