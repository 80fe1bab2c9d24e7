// The MFMA tile under the three training GEMMs (tgemm_kernel in posenet_train.hip, cgemm_kernel and wgemm_kernel in
// trajnet_train.hip): a 64 x 64 output tile per 256-thread workgroup, the reduction staged through LDS in chunks of 32, on
// v_mfma_f32_16x16x4_f32 (exact fp32 fma chains).  The kernels keep their operand addressing and their epilogues; the tile shape,
// the LDS layout, the fragment mapping and the pipeline order live here, once.  Device code only; included inside each source's
// anonymous namespace like train_reduce.h.
#pragma once

constexpr int TBM = 64, TBN = 64, TBK = 32;
constexpr int LDP = TBM + 16;               // +16: the 4 k-rows of a fragment read hit distinct bank groups
constexpr int kStageFloats = TBK * LDP;     // one staged operand block, [k][m or n]: each kernel declares two in LDS

__device__ __forceinline__ int stage_at(int k, int x) { return k * LDP + x; }      // LDS index of reduction row k, tile row / column x

// Which (k, x) of a TBK x 64 operand block element e = 0..7 of this thread stages: threads run along whichever axis of the operand
// is contiguous in memory, x (the tile's 64 rows / columns) or k.
__device__ __forceinline__ void stage_map(bool along_x, int e, int& k, int& x) {
    const int lin = e * 256 + threadIdx.x;
    if (along_x) { x = lin & 63; k = lin >> 6; } else { k = lin & 31; x = lin >> 5; }
}

// Four waves as 2 x 2 sub-tiles of 32 x 32, each two by two 16 x 16 MFMA blocks: acc[i][j][r] is the tile's element (row(i, r), col(j)).
struct Tile {
    f32x4 acc[2][2];
    int wm, wn, li, lk;      // the wave's sub-tile origin; the lane's index within a 16-wide block and its k-row group
    __device__ __forceinline__ Tile() {
#pragma unroll
        for (int i = 0; i < 2; ++i)
#pragma unroll
            for (int j = 0; j < 2; ++j) acc[i][j] = f32x4{0.f, 0.f, 0.f, 0.f};
        const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
        wm = (wave >> 1) * 32, wn = (wave & 1) * 32;
        li = lane & 15, lk = lane >> 4;
    }
    __device__ __forceinline__ int row(int i, int r) const { return wm + 16 * i + 4 * lk + r; }
    __device__ __forceinline__ int col(int j) const { return wn + 16 * j + li; }

    // acc += A . B over one staged block: sixteen MFMAs, each lane group lk feeding k-row kk + lk
    __device__ __forceinline__ void mfma_chunk(const float* As, const float* Bs) {
#pragma unroll
        for (int kk = 0; kk < TBK; kk += 4) {
            const float* ar = As + (kk + lk) * LDP;
            const float* br = Bs + (kk + lk) * LDP;
            const float a0 = ar[wm + li], a1 = ar[wm + 16 + li];
            const float b0 = br[wn + li], b1 = br[wn + 16 + li];
            acc[0][0] = __builtin_amdgcn_mfma_f32_16x16x4f32(a0, b0, acc[0][0], 0, 0, 0);
            acc[0][1] = __builtin_amdgcn_mfma_f32_16x16x4f32(a0, b1, acc[0][1], 0, 0, 0);
            acc[1][0] = __builtin_amdgcn_mfma_f32_16x16x4f32(a1, b0, acc[1][0], 0, 0, 0);
            acc[1][1] = __builtin_amdgcn_mfma_f32_16x16x4f32(a1, b1, acc[1][1], 0, 0, 0);
        }
    }

    // The register-staged pipeline over the kernel's own loop variable it = begin, begin + STEP, ... < end:  load(it) reads chunk it
    // from global memory into the kernel's registers, store() writes those registers to As / Bs.  The load of chunk it + STEP is
    // issued after the barrier that publishes chunk it, so it lands under that chunk's MFMAs.
    // The wave barrier emits no instruction.  It keeps the compiler from merging the first load's guard with the loop's entry test:
    // merged, the loop-invariant 64-bit row strides of the kernels' address arithmetic end up as phis over the divergent bounds
    // checks of that load, in VGPRs: tgemm_kernel then compiles to 116 VGPRs instead of 103 (3 waves per SIMD instead of 4) and
    // wgemm_kernel to 56 instead of 41 (7 instead of 8).  profiles/train_tile_resources.md has the table.
    template <int STEP, class Load, class Store>
    __device__ __forceinline__ void run(const float* As, const float* Bs, int begin, int end, const Load& load, const Store& store) {
        if (begin < end) load(begin);
        __builtin_amdgcn_wave_barrier();
        for (int it = begin; it < end; it += STEP) {
            __syncthreads();
            store();
            __syncthreads();
            if (it + STEP < end) load(it + STEP);
            mfma_chunk(As, Bs);
        }
    }
};
