// The condition masks of the training loops on the device (train/training_loop_posenet.py:107-205 and :221-248,
// train/training_loop_trajnet.py:72-82).  The loops decide on the host WHAT to hide (a handful of integers per item); these
// kernels apply the decision to the batch:
//   * rohm_train_cond: cond [B, 294, 1, T] = mask(src [B, T, 294]) and, optionally, clean_t = clean transposed -- the masks and the
//     two permute(0, 2, 1) copies of a PoseNet step as ONE launch.  A 64 frame x 64 channel tile goes through LDS: rows of src are
//     read along channels (a wave reads 256 consecutive bytes), columns are stored along frames (a wave stores 256 consecutive
//     bytes).  The tile's rows are padded to 65 floats: the write of lane l goes to bank (65 f + l) % 32 and the transposed read to
//     bank (65 l + c) % 32 = (l + c) % 32, both distinct within a 32-lane half, so neither side has a bank conflict.
//   * rohm_train_traj_window: the in-place trajectory window of a TrajNet step.
// Plain vector loads and stores only; no atomics; nothing is allocated or synchronised.
#include "common.h"

namespace rohm {

constexpr int kCh = 294;                // body_feat_dim: REPR_LIST in order
constexpr int kTraj = 22;               // trajectory channels: never masked
constexpr int kPos0 = 22, kVel0 = 88, kPose0 = 154, kBetas0 = 280, kContact0 = 290;
constexpr int kTile = 64;               // frames and channels of one tile
constexpr int kPad = kTile + 1;
constexpr int kChTiles = (kCh + kTile - 1) / kTile;
constexpr int kMaxT = 512;

struct CondArgs {
    const float* src; const float* clean;
    const unsigned* joint_bits; const int* window; const unsigned* vis_bits; const long long* vis_index;
    float* cond; float* clean_t;
    int B, T, n_vis, vis_rows, zero_contact, f_tiles;
};

// Bits of the joints whose state decides channel c (0: no joint does); for a contact channel the two foot joints.
__device__ __forceinline__ unsigned channel_joints(int c) {
    if (c < kPos0) return 0u;
    if (c < kVel0) return 1u << ((c - kPos0) / 3);
    if (c < kPose0) return 1u << ((c - kVel0) / 3);
    if (c < kBetas0) return 1u << (1 + (c - kPose0) / 6);
    if (c < kContact0) return 0u;
    return c < kContact0 + 2 ? (1u << 7 | 1u << 10) : (1u << 8 | 1u << 11);
}

__global__ __launch_bounds__(256) void train_cond_kernel(CondArgs a) {
    __shared__ float tile_s[kTile * kPad];
    __shared__ float tile_c[kTile * kPad];
    const int per_item = a.f_tiles * kChTiles;
    const int b = blockIdx.x / per_item, r = blockIdx.x - b * per_item;
    const int f0 = (r / kChTiles) * kTile, c0 = (r % kChTiles) * kTile;
    const int lane = threadIdx.x & 63, grp = threadIdx.x >> 6;
    const size_t item = (size_t)b * a.T;

    // in: lane = channel
    if (c0 + lane < kCh) {
#pragma unroll 4
        for (int f = grp; f < kTile; f += 4) {
            if (f0 + f >= a.T) break;
            const size_t g = (item + f0 + f) * kCh + c0 + lane;
            tile_s[f * kPad + lane] = a.src[g];
            if (a.clean) tile_c[f * kPad + lane] = a.clean[g];
        }
    }
    __syncthreads();

    // out: lane = frame
    const int f = f0 + lane;
    if (f >= a.T) return;
    const unsigned hidden = a.joint_bits ? a.joint_bits[b] : 0u;
    const bool in_window = a.window && f >= a.window[2 * b] && f < a.window[2 * b + 1];
    unsigned visible = 0xffffffffu;
    bool bad_clip = false;
    if (a.vis_bits) {
        const long long clip = a.vis_index[b];
        bad_clip = clip < 0 || clip >= a.n_vis;
        if (!bad_clip) visible = a.vis_bits[(size_t)clip * a.vis_rows + f];
    }
    for (int c = grp; c < kTile; c += 4) {
        const int ch = c0 + c;
        if (ch >= kCh) break;
        const size_t o = ((size_t)b * kCh + ch) * a.T + f;
        float v = tile_s[lane * kPad + c];
        const unsigned j = channel_joints(ch);
        if (a.vis_bits) v *= ((visible & j) == j) ? 1.0f : 0.0f;         // the reference multiplies by its 0/1 mask
        if ((hidden & j) || (in_window && ch >= kTraj) || (a.zero_contact && ch >= kContact0)) v = 0.0f;
        if (bad_clip) v = __int_as_float(0x7fc00000);
        a.cond[o] = v;
        if (a.clean) a.clean_t[o] = tile_c[lane * kPad + c];
    }
}

__global__ __launch_bounds__(256) void traj_window_kernel(float* __restrict__ cond, const int* __restrict__ window, long long total,
                                                          int T, int C, int n_ch) {
    const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= total) return;
    const int ch = (int)(i % n_ch);
    const long long row = i / n_ch;
    const int t = (int)(row % T), b = (int)(row / T);
    if (t >= window[2 * b] && t < window[2 * b + 1]) cond[row * C + ch] *= 0.0f;      // x * 0 inside, x * 1 (= x) outside
}

}  // namespace rohm

using namespace rohm;

extern "C" int rohm_train_cond(const float* src, const float* clean, int B, int T, const unsigned* joint_bits, const int* window,
                               const unsigned* vis_bits, int n_vis, int vis_rows, const long long* vis_index,
                               const long long* vis_index_host, int zero_contact, float* cond, float* clean_t,
                               rohm_stream_t stream) {
    ROHM_ARG_CHECK(B >= 0, "train_cond: negative batch size (B=%d)", B);
    ROHM_ARG_CHECK(T >= 1 && T <= kMaxT, "train_cond: T=%d outside [1, %d]", T, kMaxT);
    if (vis_bits) {
        ROHM_ARG_CHECK(n_vis >= 1, "train_cond: vis_bits needs n_vis >= 1 (got %d)", n_vis);
        ROHM_ARG_CHECK(vis_rows >= T, "train_cond: vis_rows=%d is less than T=%d", vis_rows, T);
        ROHM_ARG_CHECK(B == 0 || vis_index, "train_cond: vis_bits needs vis_index");
        if (vis_index_host)
            for (int b = 0; b < B; ++b)
                ROHM_ARG_CHECK(vis_index_host[b] >= 0 && vis_index_host[b] < n_vis,
                               "train_cond: vis_index[%d]=%lld outside [0, %d)", b, vis_index_host[b], n_vis);
    }
    if (B == 0) return ROHM_OK;
    ROHM_ARG_CHECK(src && cond, "train_cond: null argument");
    ROHM_ARG_CHECK(!clean == !clean_t, "train_cond: clean and clean_t go together");
    ROHM_ARG_CHECK(src != cond && clean != cond && src != clean_t, "train_cond: outputs must not alias inputs");
    CondArgs a;
    a.src = src; a.clean = clean; a.joint_bits = joint_bits; a.window = window; a.vis_bits = vis_bits; a.vis_index = vis_index;
    a.cond = cond; a.clean_t = clean_t;
    a.B = B; a.T = T; a.n_vis = n_vis; a.vis_rows = vis_rows; a.zero_contact = zero_contact != 0;
    a.f_tiles = (T + kTile - 1) / kTile;
    const long long blocks = (long long)B * a.f_tiles * kChTiles;
    ROHM_ARG_CHECK(blocks <= 0x7fffffffll, "train_cond: batch too large for one launch");
    prof::Scope ps("train_cond", 0.0, 8.0 * (clean ? 2 : 1) * (double)B * T * kCh, (hipStream_t)stream);
    hipLaunchKernelGGL(train_cond_kernel, dim3((unsigned)blocks), dim3(256), 0, (hipStream_t)stream, a);
    ROHM_LAUNCH_CHECK();
    return ROHM_OK;
}

extern "C" int rohm_train_traj_window(float* cond, int B, int T, int C, int n_ch, const int* window, rohm_stream_t stream) {
    ROHM_ARG_CHECK(B >= 0 && T >= 1 && C >= 1, "train_traj_window: bad sizes (B=%d T=%d C=%d)", B, T, C);
    ROHM_ARG_CHECK(n_ch >= 0 && n_ch <= C, "train_traj_window: n_ch=%d outside [0, %d]", n_ch, C);
    if (B == 0 || n_ch == 0) return ROHM_OK;
    ROHM_ARG_CHECK(cond && window, "train_traj_window: null argument");
    const long long total = (long long)B * T * n_ch;
    ROHM_ARG_CHECK((total + 255) / 256 <= 0x7fffffffll, "train_traj_window: batch too large for one launch");
    prof::Scope ps("train_traj_window", 0.0, 8.0 * (double)total, (hipStream_t)stream);
    hipLaunchKernelGGL(traj_window_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, (hipStream_t)stream, cond, window,
                       total, T, C, n_ch);
    ROHM_LAUNCH_CHECK();
    return ROHM_OK;
}
