// What the fp32-MFMA inference GEMMs share: gemm_f32_kernel (gemm_f32.hip, one launch per GEMM), the phases of encoder_chain_kernel /
// encoder_stack_kernel (encoder_chain.hip), and for the first and last item lbs.hip / trajnet_resident.hip / exchange.hip.  The
// swizzled LDS image and the scheduling groups of the K loops; the XCD-id read and the turn policy of the bounded waits; the tile
// constants, the unit -> slot map and dummy-zone rule of the LDS-DMA staging, the 16x16x4 fragment and its MFMA half, the column operands
// and the embed-table row, Chan's merges of row statistics.  Not here, on measurements (profiles/gemm_tile_resources.md): gemm_phase
// and prefetch_w write the staging map out, both GEMMs their fragment read, and each its LayerNorm tail; the K-loop pipelines stay
// with their kernels on purpose (see the comments there).
#pragma once
#include "common.h"

namespace rohm {

constexpr int kGemmBK = 32;      // K chunk

__device__ __forceinline__ int lds_off(int row, int slot) {   // float index inside a [rows][32] tile
    return row * kGemmBK + ((slot ^ ((row >> 1) & 7)) << 2);
}

// compile-time repetition of sched_group_barrier triples (the builtin needs literal arguments) that pins the [LDS read | DMA | MFMA]
// interleave of a K loop.
// VAL > 0 (conv gather): the per-chunk address arithmetic of the gathered operand (VALU) is dealt out between the MFMA
// groups as well -- left alone the scheduler hoists all of it in front of the half's first MFMA.
template <int I, int N, int MF, int DS_TOTAL, int VM_TOTAL, int ID, int VAL = 0>
struct SchedGroups {
    static __device__ __forceinline__ void run() {
        constexpr int kValu = 0x002, kMfma = 0x008, kVmem = 0x010, kDsRead = 0x100;
        __builtin_amdgcn_sched_group_barrier(kMfma, MF, ID);
        __builtin_amdgcn_sched_group_barrier(kDsRead, DS_TOTAL / N + (I < DS_TOTAL % N ? 1 : 0), ID);
        if constexpr (VAL > 0) __builtin_amdgcn_sched_group_barrier(kValu, VAL, ID);
        __builtin_amdgcn_sched_group_barrier(kVmem, VM_TOTAL / N + (I < VM_TOTAL % N ? 1 : 0), ID);
        SchedGroups<I + 1, N, MF, DS_TOTAL, VM_TOTAL, ID, VAL>::run();
    }
};
template <int N, int MF, int DS_TOTAL, int VM_TOTAL, int ID, int VAL>
struct SchedGroups<N, N, MF, DS_TOTAL, VM_TOTAL, ID, VAL> {
    static __device__ __forceinline__ void run() {}
};

// ---- exchanges through the L2 of one XCD ------------------------------------------------------------------------------------------
// which XCD this workgroup runs on, + 1 (1 .. 8: never 0, so zeroed memory is stale).  Part of every exchange tag: a partner that
// publishes from another XCD is reported (status 2), not trusted silently
__device__ __forceinline__ unsigned xcd_id1() { return 1u + (unsigned)__builtin_amdgcn_s_getreg((3 << 11) | 20); }

// The turn policy of the bounded waits on exchange words (the layout probe of exchange.hip has its own, shorter bound).  A wait loop polls, and between two polls asks give_up(): s_sleep 1; a wait that another workgroup of the pass
// already lost (the error word is looked at every 128 turns) is not worth 0.2 s again: the results since the last status check are
// void anyway, the host falls back and re-runs (rohm_amd/diffusion/ddpm.py); after 2^19 turns (~0.2 s: never on a healthy device, the
// partners are co-resident) `code` goes into the error word: do not hang the device; the host reads the word.
struct WaitTurns {
    int it = 0;
    __device__ __forceinline__ bool give_up(unsigned* err, unsigned code) {
        __builtin_amdgcn_s_sleep(1);
        if ((it & 127) == 127 && __hip_atomic_load(err, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) != 0u) return true;
        if (it > (1 << 19)) {
            __hip_atomic_store(err, code, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            return true;
        }
        ++it;
        return false;
    }
};
// ... for ONE 8-byte word (relaxed, agent scope: past the L1, the partner's store went to L2): until pred(word); false = given up.
// pred may act on the word it accepts: the callers' predicates report a partner on another XCD (status 2) before they return true
template <typename Pred>
__device__ __forceinline__ bool wait_word(const unsigned long long* addr, Pred&& pred, unsigned* err, unsigned code) {
    for (WaitTurns w;;) {
        if (pred(__hip_atomic_load(addr, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT))) return true;
        if (w.give_up(err, code)) return false;
    }
}

namespace gemm_tile {

constexpr int BM = 144;
constexpr int BK = kGemmBK;
constexpr int NRB = BM / 16;        // 9 row blocks of 16
constexpr int A_UNITS = BM * 8;     // 16-byte units per A chunk (1152)
constexpr int A_ITERS = (A_UNITS + 255) / 256;  // 5 (the last pass is half populated)

// ---- staging geometry: LDS-DMA of a [rows][32] chunk image by 256 threads, pass i moves the 16-byte units u = tid + 256 i ----------
// unit -> (row, slot): the XOR swizzle that makes every ds_read_b128 conflict-free is applied to the per-lane SOURCE address (the
// DMA writes LDS linearly): unit u of row `row` (= u / 8; row 0 for the units past the image, the tail of a half-populated last pass)
// fetches the 16 bytes at slot unit_slot(u, row) of that row's K chunk.
__device__ __forceinline__ int unit_slot(int u, int row) { return (u & 7) ^ ((row >> 1) & 7); }
// where pass `pass` of wave (wave_u / 64) lands in an image of UNITS units.  A half-populated last pass: the waves past the image fetch
// a (valid) dummy row into the landing zone instead of being predicated off -- a branch here would split the block the scheduler
// interleaves
template <int UNITS>
__device__ __forceinline__ float* unit_dst(float* img, int pass, int wave_u, float* lds_dummy) {
    float* dst = img + (pass * 256 + wave_u) * 4;
    if (pass == (UNITS + 255) / 256 - 1 && UNITS % 256 != 0)
        dst = (wave_u < UNITS - pass * 256) ? dst : lds_dummy + (wave_u & 64) * 4;
    return dst;
}

// ---- 16x16x4 fragments: 9 row blocks x NCB column blocks per wave -------------------------------------------------------------------
// lane (li = l & 15, lg = l >> 4) holds X[16 b + li][16 s + 4 lg + j], j = 0..3, of block b: ONE ds_read_b128; MFMA j contracts
// k = {4 lg + j}: a fixed permutation of k, identical for both operands.
template <int NCB>
struct Frag16 { f32x4 a[NRB]; f32x4 b[NCB]; };
// one k16 half of a chunk.  SWAP: weights on the MFMA "A" side, so a lane ends with 4 consecutive output columns of one row
template <int NCB, bool SWAP = true>
__device__ __forceinline__ void mma_half16(f32x4 (&acc16)[NRB * NCB], const Frag16<NCB>& f) {
#pragma unroll
    for (int r = 0; r < NRB; ++r)
#pragma unroll
        for (int c = 0; c < NCB; ++c)
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                if constexpr (SWAP)
                    acc16[r * NCB + c] = __builtin_amdgcn_mfma_f32_16x16x4f32(f.b[c][j], f.a[r][j], acc16[r * NCB + c], 0, 0, 0);
                else
                    acc16[r * NCB + c] = __builtin_amdgcn_mfma_f32_16x16x4f32(f.a[r][j], f.b[c][j], acc16[r * NCB + c], 0, 0, 0);
            }
}

// ---- epilogue operands ------------------------------------------------------------------------------------------------------------
struct ColOps { f32x4 bias, g4, b4; };          // what depends on the column group only: bias, LayerNorm gamma and beta
// EPI_EMBED: the row of the positional / timestep table that output row m adds: the timestep token's row for token 0, else the
// positional (or per-row) table.  P: GemmParams, or a phase's copy of its S / tab* members
template <typename P>
__device__ __forceinline__ const float* embed_table_row(const P& p, int m, int nb) {
    const int bidx = m / p.S, tok = m % p.S;
    return (tok == 0) ? p.tab0 + (size_t)bidx * p.ldtab0 + nb : p.tab + (size_t)(p.tab_by_row ? m : tok) * p.ldtab + nb;
}

// ---- row statistics of the LayerNorm epilogues ------------------------------------------------------------------------------------
// Chan's update of two equal-sized parts of n elements each, (mean, M2 = sum of squares about that mean):
//     mean = (m_a + m_b) / 2,   M2 = M2_a + M2_b + n (m_b - m_a)^2 / 2
__device__ __forceinline__ void merge_stats(float ma, float qa, float mb, float qb, float n, float& m, float& q2) {
    const float d = mb - ma;
    m = 0.5f * (ma + mb);
    q2 = (qa + qb) + 0.5f * n * d * d;
}
// ... of this lane's part and lane l ^ 32's (far) or l ^ 16's: a lane swap on the VALU
__device__ __forceinline__ void merge_stats_swap(float& m, float& q2, float n, bool far) {
    typedef unsigned rohm_u2 __attribute__((ext_vector_type(2)));
    rohm_u2 tm, tq;
    if (far) { tm = __builtin_amdgcn_permlane32_swap(__float_as_uint(m), __float_as_uint(m), false, false);
               tq = __builtin_amdgcn_permlane32_swap(__float_as_uint(q2), __float_as_uint(q2), false, false); }
    else     { tm = __builtin_amdgcn_permlane16_swap(__float_as_uint(m), __float_as_uint(m), false, false);
               tq = __builtin_amdgcn_permlane16_swap(__float_as_uint(q2), __float_as_uint(q2), false, false); }
    merge_stats(__uint_as_float(tm[0]), __uint_as_float(tq[0]), __uint_as_float(tm[1]), __uint_as_float(tq[1]), n, m, q2);
}

}  // namespace gemm_tile
}  // namespace rohm
