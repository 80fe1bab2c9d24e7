/*
 * rohm_hip.h -- C ABI of librohm_hip.so, the MI355X (gfx950) native library behind
 * RoHM's iterative-denoising hot path.
 *
 * The reference (sanweiliti/RoHM) is pure Python/PyTorch and has no FFI of its own
 * (SURVEY.md §8b); each entry point below names the reference function (file:line
 * under the RoHM tree) whose arithmetic it replaces.  The Python host side
 * (rohm_amd/) binds these through ctypes and mirrors the reference's classes.
 *
 * Conventions
 *   - every function returns 0 on success, <0 on error; rohm_last_error() returns a
 *     thread-local message.  Nothing throws or aborts across the boundary.
 *   - all tensor arguments are DEVICE pointers to contiguous fp32 (int64 for
 *     timesteps) owned by the caller; the library never allocates inside a
 *     forward/step call: scratch comes from the caller's workspace
 *     (*_workspace_bytes).  Weights are copied and re-laid-out at *_create time, so
 *     the caller may free its copies afterwards.
 *     The training entry points (rohm_posenet_train_*, rohm_trajnet_train_*) have no handle: they read the
 *     caller's LIVE parameters in the reference's layouts on every call and keep their state in caller-owned
 *     `saved` / `scratch` buffers (*_saved_bytes, *_scratch_bytes).
 *   - alignment: x_t, cond, noise, x, t, d_out and the outputs of rohm_posenet_forward / _sample_loop / _train_*,
 *     rohm_ddpm_step[_table], rohm_q_sample and rohm_guidance_* need the alignment of their element only: they may be a batch
 *     slice of a larger tensor (8 bytes past a 16-byte boundary for [B, 294, 1, 143]).  So do the LIVE parameter and gradient
 *     pointers of rohm_posenet_train_* (views into a flat buffer): a kernel takes a 16-byte access through such a pointer only
 *     where the address allows it.  tests/test_gpu_bounds.py runs these calls on batch slices and compares bit for bit.  Other
 *     entry points state what they need (the GEMM building blocks' A / W, every `ws` / `scratch` / `saved`).
 *   - a call reads and writes only the operands it is given, and of `ws` / `scratch` / `saved` only the first *_bytes bytes
 *     (tests/test_gpu_bounds.py: guard bands around every buffer).
 *   - every launch goes on the caller-supplied hipStream_t (passed as void*);
 *     no hidden device synchronisation in forward / step / loop calls.  Set-up calls say so where they
 *     synchronise: *_create, rohm_exchange_probe, rohm_posenet_set_exchange(h, 1), the status read
 *     rohm_posenet_exchange_status; the stand-alone rohm_gemm_res_layernorm_f32 / rohm_output_process_f32
 *     probe an un-probed device on their FIRST call unless the stream records a graph (see there).
 *     One loop call does wait: rohm_trajnet_sample_loop in its clip-resident form (TrajNet's default, see rohm_trajnet_loop_mode)
 *     synchronises `stream` once at its end to read the in-kernel meetings' error word (ROHM_TRAJ_RESIDENT=0 keeps it wait-free).
 *     tests/test_gpu_stream_order.py holds every entry point to this (inputs that arrive late on a side stream, a call log).
 *   - recordable calls: every entry point that takes a rohm_stream_t and is not named below as waiting may be called on a stream
 *     that records a hipGraph.  A replay does exactly what the recorded call would do if it were made again with the same argument
 *     values: device operands are read at replay time; host scalars (step, seed, coefficients, sizes) and host arrays (t_model,
 *     coef, pointer and numel tables, camera matrices, rohm_result_rows_item lists) are read at the call and travel in the kernel
 *     arguments, so the caller may rewrite or free host arrays as soon as the call returns -- no recorded node points at caller host
 *     memory.  A replay therefore repeats the recorded `step` of rohm_adamw_step and the recorded `seed` of
 *     rohm_posenet_train_forward: a caller that wants them to move records one graph per value or passes them through device
 *     memory of its own design (rohm_amd.optim.AdamW.step() and PoseNet.forward in train mode with dropout > 0 raise while the
 *     current stream records, because they would freeze them silently).  Process-wide read-outs describe the recording call, not
 *     the replays: rohm_trajnet_loop_mode, rohm_trajnet_train_last_gemms, rohm_last_error.
 *     Waiting calls cannot be recorded.  rohm_track_resample waits for its stream to check valid_idx on the host and is refused
 *     on a recording stream.  rohm_floor_hypotheses waits for its stream to check the triples on the host and is refused on a
 *     recording stream.  rohm_posenet_exchange_status waits for its stream to read the status word and is refused on a recording
 *     stream.  Refused means: the call returns ROHM_ERR_UNSUPPORTED with a rohm_last_error that names the function, before it issues
 *     or synchronises anything, so the caller's capture stays valid.  rohm_trajnet_sample_loop steps aside instead: on a recording
 *     stream it takes its launch-per-layer form, which does not wait (rohm_trajnet_loop_mode() reports 0 for that call).
 *     Warm-up: none is required for correctness.  Two first-call decisions are taken differently while recording, neither changes
 *     a result: on a device that has not been probed (rohm_exchange_probe) rohm_gemm_res_layernorm_f32 refuses and
 *     rohm_output_process_f32 uses plain tiles (see there); and a host thread whose FIRST TrajControl loop call is recorded gets
 *     the one-stream order in that graph, because the control stream and its events are not created under a capture -- one eager
 *     rohm_trajnet_sample_loop call on that thread before the capture gives the graph its parallel branch (bit-identical either
 *     way; that branch needs the runtime's default of four hardware queues to replay).  The Python wrappers allocate workspaces
 *     per call or cache them per handle and shape: under torch.cuda.graph an allocation made while recording belongs to the graph's
 *     pool, so call a wrapper once eagerly first, as torch asks for any captured code.
 *     The launch profiler (rohm_profile_start) is outside this contract: it records events of its own around every launch; record
 *     with it off.
 *     tests/test_gpu_graph_replay.py records every such entry point on one set of values, replays it over poisoned outputs and
 *     workspaces on a second set and on the first again, with the host arrays it can reach rewritten after the capture, and
 *     compares bit for bit with eager calls; the three waiting calls are refused there with the capture left valid.
 *   - handles are immutable after create (documented exceptions, all control calls that must not race with
 *     launches of the same handle: rohm_posenet_set_exchange, rohm_posenet_inject_exchange_fault,
 *     rohm_posenet_set_stack_timeline); calls are re-entrant across streams given distinct workspaces.
 *     Every Python binding that keeps a workspace hands out one per HIP stream (PoseNet, TrajNet, and the SMPL-X layer's guidance
 *     and skinning scratch); every other wrapper allocates per call.  One limit: the stream-K output head and the clip-resident
 *     TrajNet step launch 256 one-per-CU workgroups that meet through L2, so two of them in flight on two streams cannot both be
 *     resident and one may report an expired wait (ROHM_ERR_EXCHANGE; the loop falls back to its launch-per-layer form) -- run
 *     those launches one at a time per device.  tests/test_gpu_reentrancy.py holds every entry point to this (a ledger of who was
 *     handed which memory; two streams released together; two host threads on one handle).
 *     One handle per device.
 *
 * Caller-owned memory
 *   Every buffer the caller hands in to be written -- `ws`, `scratch`, `saved`, `buf` and every output tensor -- may hold
 *   ANYTHING on entry: uninitialised memory, NaN, the remains of an earlier call of another shape at the same address
 *   (a caching allocator returns the block it was just given back).  Results do not depend on those contents: what a
 *   kernel reads it, or an earlier launch of the same call, has written; pad rows and pad columns that feed a GEMM are
 *   cleared by the call; an exchange header without the magic word (memory the library has not armed at THAT offset) makes
 *   the call zero the header, its statistics slots and its flags before the first launch.  tests/test_gpu_stale_memory.py
 *   holds every entry point to this, bit for bit.  Two things are state by purpose: *_train_backward reads the `saved`
 *   buffer *_train_forward wrote, and an armed exchange header (error word, pass counter) lives on in a workspace from
 *   call to call.
 *   Regions a call leaves UNWRITTEN (the caller's to initialise if it reads them):
 *     - rohm_output_process_f32: channels outside [ch_off, ch_off + C_out) of `out`;
 *     - rohm_traj_rederive and rohm_repr_joints_vjp address their output through strides: only the elements they name (channels
 *       0..21 of frames 0..T-2; all 294 channels) are written, what lies between them in the caller's tensor is not touched;
 *     - optional outputs passed as NULL are not computed; nothing else of an output tensor is skipped;
 *     - of a workspace nothing may be read back by the caller, except where an entry point says so
 *       (rohm_posenet_status_offset, the header words of rohm_gemm_res_layernorm_f32 / rohm_output_process_f32).
 */
#ifndef ROHM_HIP_H
#define ROHM_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define ROHM_OK 0
#define ROHM_ERR_ARG (-1)
#define ROHM_ERR_HIP (-2)
#define ROHM_ERR_WORKSPACE (-3)
#define ROHM_ERR_UNSUPPORTED (-4)
#define ROHM_ERR_EXCHANGE (-5)   /* an in-kernel exchange between workgroups failed: results since the last status check are invalid */

typedef void* rohm_stream_t; /* hipStream_t */

const char* rohm_last_error(void);
int rohm_version(void);

/* ------------------------------------------------------------------ launch profiler
 * Measurement aid for bench.py: while active, every instrumented kernel launch is bracketed by a
 * pair of HIP events recorded ON THE LAUNCH STREAM (so it sees the library's launches whatever
 * torch's current stream is).  Inside *_sample_loop only every `step_stride`-th denoising step is
 * bracketed, which keeps the timed region's perturbation negligible.  Not thread-safe.
 * rohm_profile_stop synchronises the recorded events and aggregates per kernel label:
 * launches, summed duration, summed algorithmic flops / bytes (as priced in DESIGN.md). */
typedef struct {
    char name[48];
    uint64_t launches;
    double total_ms;
    double flops;
    double bytes;
} rohm_profile_row;
/* The profiler is one process-wide recorder: start / stop / detail must not overlap launches issued by other host threads. */
int rohm_profile_start(int step_stride);
int rohm_profile_stop(rohm_profile_row* rows, int max_rows, int* n_rows);
/* on != 0: GEMM / conv-GEMM / GroupNorm launches are recorded under a label that carries their shape ("conv_gemm/64 M576
 * N512 K2560 S8"), one row per distinct shape -- per-launch-shape timing of the TrajNet step (scripts/bench_trajnet.py). */
int rohm_profile_detail(int on);

/* ------------------------------------------------------------------ building blocks
 * Exposed so that each kernel can be parity-tested and profiled on its own.        */

/* C[M,N] = epi(A[M,K] . W[N,K]^T): the fp32-MFMA GEMM every Linear of the path runs
 * on (nn.Linear in model/heads.py:154,169, nn.TransformerEncoderLayer in
 * model/posenet.py:63-69).  A, W row-major with K contiguous (lda/ldw in floats,
 * multiples of 4, 16-byte aligned); K a multiple of 32; M, N arbitrary.
 * epi: 0 = +bias, 1 = +bias, erf-form GELU (erf via A&S 7.1.26, abs err 1.5e-7), 2 = +bias +R[M,N](ldr).
 * bias may be NULL.  Leading dimensions are in floats and may exceed the row length (views into larger matrices):
 * lda >= K, ldw >= K, ldc >= N and, for epi 2, ldr >= N -- a shorter one would overlap rows and is refused with
 * ROHM_ERR_ARG.  C, bias and R need no alignment and ldc / ldr no multiple (16-byte aligned ones with ldc, ldr
 * multiples of 4 take the vector epilogue). */
int rohm_gemm_f32(const float* A, int lda, const float* W, int ldw, float* C, int ldc, int M, int N,
                  int K, const float* bias, const float* R, int ldr, int epi, rohm_stream_t stream);

/* In-place LayerNorm over the last dimension of x[M,D] (D == 256, 512 or 1024), eps 1e-5, biased
 * variance, affine -- nn.LayerNorm inside nn.TransformerEncoderLayer (model/posenet.py:63-69). */
int rohm_layernorm_f32(float* x, const float* gamma, const float* beta, int M, int D,
                       rohm_stream_t stream);

/* C = LayerNorm(A . W^T + bias + R) * gamma + beta in ONE launch -- the post-norm sublayer tail of nn.TransformerEncoderLayer
 * (model/posenet.py:63-69: x = norm1(x + out_proj(attn)), x = norm2(x + linear2(...)); `norm_first=False`), eps inside the root,
 * biased variance over the N columns.  The N / 64 or N / 128 column tiles of a 144-row tile exchange their per-row (mean, M2)
 * (merged pairwise by Chan's update: two-pass stability) through L2 while the kernel runs (they are dispatched back to back onto one XCD), so LN(x) is stored once and the raw
 * sum never reaches HBM.  Shapes: M % 144 == 0, K % 32 == 0, N / 64 or N / 128 in {1, 2, 4, 8} (else ROHM_ERR_UNSUPPORTED:
 * use rohm_gemm_f32(epi 2) + rohm_layernorm_f32).  `scratch`: rohm_gemm_res_layernorm_scratch_bytes(M, N) bytes, 64-byte aligned,
 * owned by the caller for the duration of the launch.  Its first 64 bytes are the exchange header: [0] the error word (0 = fine, 1 a
 * bounded wait expired, 2 partners on different XCDs; sticky -- the caller clears it), [1] a magic once armed, [2] a pass counter
 * this call advances on the device.  A scratch the library has not seen (no magic: uninitialised or recycled memory) is zeroed by the
 * call itself.  The slots are tagged with that device-side counter, so the launch may be recorded into a hipGraph: every replay
 * draws a fresh tag.  The partner tiles must be co-resident on one XCD: on a device that is not a whole MI355X (partitioned, CU
 * mask, probe launch failed -- see rohm_posenet_exchange_mode) the call returns ROHM_ERR_UNSUPPORTED.
 * The device in question is the one that owns `scratch`.  Its layout verdict comes from rohm_exchange_probe (below) or from an
 * earlier rohm_posenet_create on that device; on a device nobody has probed yet, the FIRST call of this function (and of
 * rohm_output_process_f32 with a scratch) runs the probe itself -- a hipMalloc, a null-stream launch and a device synchronisation,
 * once -- unless `stream` is recording a graph: then nothing is probed or cached, this call returns ROHM_ERR_UNSUPPORTED and
 * rohm_output_process_f32 uses plain tiles.  Call rohm_exchange_probe(device) before a capture (or before a latency-critical first
 * call) and these entry points never synchronise. */
/* Layout probe of `device`, always run afresh: properties, the CU-mask environment, 256 one-per-CU workgroups that must be resident
 * together with block b on XCD b % 8.  Returns 1 if the exchanging launches may be used there, 0 if not; `why` (optional) receives a
 * static string.  Allocates, launches on the null stream and synchronises the device: a set-up call.  A verdict about the device is
 * cached for the later launch calls; "the probe could not run" (set-up / launch failed) is returned but never cached.  Probes are
 * serialised across the processes of a host (advisory file lock), so the ranks of a node do not time each other out. */
int rohm_exchange_probe(int device, const char** why);
size_t rohm_gemm_res_layernorm_scratch_bytes(int M, int N);
int rohm_gemm_res_layernorm_f32(const float* A, int lda, const float* W, int ldw, float* C, int ldc, int M, int N, int K,
                                const float* bias, const float* R, int ldr, const float* gamma, const float* beta, float eps,
                                void* scratch, size_t scratch_bytes, rohm_stream_t stream);

/* Multi-head self-attention over n_tok tokens, head dim 64 or 128, for n_seq sequences:
 * qkv[n_seq*n_tok, 3*n_head*head_dim] (q | k | v blocks, q already scaled by head_dim^-1/2)
 * -> ctx[n_seq*n_tok, n_head*head_dim].  Replaces the scaled-dot-product inside
 * nn.MultiheadAttention (model/posenet.py:63-69).  n_tok = 144, head_dim = 128 (every released
 * configuration) runs the specialised kernel; other shapes the general one. */
int rohm_attention_f32(const float* qkv, float* ctx, int n_seq, int n_head, int n_tok, int head_dim,
                       rohm_stream_t stream);

/* ---- opt-in precision ladder: split GEMMs on 16-bit PLANES of the fp32 operands ----
 * The same Linears as rohm_gemm_f32 (model/posenet.py:63-69), each fp32 product a.w emulated by bf16 / fp16 MFMA products of
 * planes.  `nplane` is the MODE everywhere:  3 = bf16x6 (three bf16 planes cut by truncation, x = h + m + l exactly, six products,
 * fp32-class accuracy),  2 = bf16x3 (two bf16 planes, three products, ~2^-16),  16 = fp16x3 (two FP16 planes h = fp16(x),
 * l' = fp16((x - h) 2^11): x = h + 2^-11 l' to 2^-24 for 6e-5 <= |x| <= 65504; three products, the two cross terms in a second
 * accumulator of weight 2^-11: ~2^-22 per product).  A plane tensor of X[rows][K] (rows % 16 == 0, K % 32 == 0) is
 * rohm_planes_bytes(rows, K, mode) bytes in the fragment-major layout of rohm_amd/csrc/planes.h; producers write it (LayerNorm,
 * attention, the GELU GEMM) or rohm_planes_split cuts it from scale * X (scale: a power of two, 1 for activations; fp16 weight
 * planes are cut from 2^8 W and the GEMM is given acc_scale = 2^-8).  Never the default: rohm_posenet_create selects a mode only
 * under ROHM_GEMM_PRECISION=bf16x6 | bf16x3 | fp16x3. */
size_t rohm_planes_bytes(int rows, int K, int nplane);
int rohm_planes_split(const float* X, int ldx, int rows, int K, int nplane, float scale, void* planes, rohm_stream_t stream);
/* C[M,N] = epi(A . W^T) from the planes of A [M][K] and W [N][K]; M % 144 == 0, N % 64 == 0, K % 32 == 0.
 * epi: 0 = +bias, 1 = +bias, erf GELU, 2 = +bias +R, 3 = (+bias) * (n < qcols ? qscale : 1).  C (fp32, ldc) and / or
 * Cp (planes of the result over [M][N]) receive the result; the accumulator is multiplied by acc_scale first (0 = 1).
 * flags bit 0: plane output through 8-byte stores. */
int rohm_gemm_planes(const void* Ap, const void* Wp, float* C, int ldc, void* Cp, int M, int N, int K,
                     const float* bias, const float* R, int ldr, int qcols, float qscale, float acc_scale, int epi,
                     int nplane, int flags, rohm_stream_t stream);
/* rohm_gemm_planes with nn.LayerNorm (model/posenet.py:60-69 norm1 / norm2 of nn.TransformerEncoderLayer, post-norm) FOLDED into
 * the GEMMs around it (two-plane modes, K >= 192): the normalised tensor is never stored.  Row statistics travel as partial
 * (sum, sum of squares) pairs per 16 columns, row-block major: stats[row / 16][ln_dim / 16][row % 16][2] floats.
 *   out_stats (epi 2, ln_dim == N): receives the statistics of the result rows.
 *   ln_stats (epi 1 / 3, ln_dim == K): Ap are the planes of the RAW tensor x, Wp those of W[n][k] gamma[k], bias holds
 *     d[n] = b[n] + sum_k beta[k] W[n][k], ln_c holds c[n] = sum_k gamma[k] W[n][k]; the epilogue computes
 *     (acc - mu c) rstd + d = LN(x) W^T + b.
 *   r_stats (epi 2, ln_dim == N): R is raw as well; LN(R) = (R - mu) rstd r_gamma + r_beta is what is added.
 * Any of the three may be null. */
int rohm_gemm_planes_ln(const void* Ap, const void* Wp, float* C, int ldc, void* Cp, int M, int N, int K,
                        const float* bias, const float* R, int ldr, int qcols, float qscale, float acc_scale, int epi,
                        int nplane, const float* ln_stats, const float* ln_c, const float* r_stats, const float* r_gamma,
                        const float* r_beta, float* out_stats, int ln_dim, float ln_eps, rohm_stream_t stream);
/* rohm_layernorm_f32 that also writes the planes of its result (M % 16 == 0); the fp32 result is bit-identical. */
int rohm_layernorm_planes_f32(float* x, const float* gamma, const float* beta, int M, int D, int nplane,
                              void* planes, rohm_stream_t stream);
/* rohm_attention_f32 (n_tok = 144, head_dim = 128 only) writing the planes of ctx instead of fp32 ctx. */
int rohm_attention_planes_f32(const float* qkv, void* ctx_planes, int n_seq, int n_head, int nplane,
                              rohm_stream_t stream);

/* One DDPM ancestral update, elementwise over n floats:
 *   x_prev = c1*x0 + c2*x_t + guid_scale*guid_grad + sigma*noise
 * = q_posterior_mean_variance + p_sample[_with_grad]
 * (diffusion/gaussian_diffusion_posenet.py:212-234,426-434,466-479).  guid_grad may be NULL;
 * noise may be NULL when sigma == 0 (t == 0).  x_prev may alias x_t. */
int rohm_ddpm_step(const float* x_t, const float* x0, const float* noise, const float* guid_grad,
                   float c1, float c2, float sigma, float guid_scale, float* x_prev, size_t n,
                   rohm_stream_t stream);

/* Same update with per-sample timesteps and device-resident schedule tables (no host sync):
 *   tables [n_steps, 4] fp32 rows = {posterior_mean_coef1, posterior_mean_coef2,
 *                                     posterior_variance, posterior_log_variance_clipped}
 *   t      int64[B]   timestep of each sample (row of `tables`)
 *   x_prev[b] = c1*x0 + c2*x_t + var*(w_a*grad_a + w_b*grad_b) + [t_b != 0]*exp(0.5*logvar)*noise
 * over `row_len` floats per sample.  grad_a / grad_b may be NULL.  This is exactly
 * p_sample_with_grad (diffusion/gaussian_diffusion_posenet.py:436-480) after the network call. */
int rohm_ddpm_step_table(const float* x_t, const float* x0, const float* noise, const float* grad_a,
                         float w_a, const float* grad_b, float w_b, const float* tables,
                         const int64_t* t, int n_steps, float* x_prev, int B, size_t row_len,
                         rohm_stream_t stream);

/* ------------------------------------------------------------------------- PoseNet
 * model/posenet.py:12-96 + model/heads.py:112-176.                                   */
typedef struct rohm_posenet rohm_posenet_t;

typedef struct {
    const float *in_proj_w, *in_proj_b;   /* [3D, D], [3D]   self_attn.in_proj_*      */
    const float *out_proj_w, *out_proj_b; /* [D, D], [D]     self_attn.out_proj.*     */
    const float *lin1_w, *lin1_b;         /* [F, D], [F]     linear1.*                */
    const float *lin2_w, *lin2_b;         /* [D, F], [D]     linear2.*                */
    const float *norm1_w, *norm1_b;       /* [D]             norm1.*                  */
    const float *norm2_w, *norm2_b;       /* [D]             norm2.*                  */
} rohm_posenet_layer_weights;

typedef struct {
    const float *in_x_w, *in_x_b; /* [D, C_in], [D]  input_process.poseEmbedding.*         */
    const float *in_c_w, *in_c_b; /* [D, C_in], [D]  input_process_cond.poseEmbedding.*    */
    const float* pe;              /* [pe_len, D]     sequence_pos_encoder.pe (squeezed)    */
    int pe_len;
    const float *t_w0, *t_b0;     /* [D, D], [D]     embed_timestep.time_embed.0.*         */
    const float *t_w2, *t_b2;     /* [D, D], [D]     embed_timestep.time_embed.2.*         */
    const float *out_w, *out_b;   /* [C_out, D], [C_out]  output_process.poseFinal.*       */
    const rohm_posenet_layer_weights* layers; /* [n_layer] */
} rohm_posenet_weights;

/* OutputProcess.forward (model/heads.py:171-176): poseFinal Linear D -> C_out of every token, stored the way PoseNet.forward returns
 * it (model/posenet.py:94-96).  h [B * (T + 1), D] token-major (row b * (T + 1) + tok; the reference's [T + 1, B, D] with the two
 * leading axes exchanged; token 0 is the timestep token and has no output), w [C_out, D], b [C_out] ->
 * out[b][ch_off + c][0][tok - 1] of a [B, C_total, 1, T] tensor (the other channels are not touched).
 * `scratch` (optional, rohm_output_process_scratch_bytes() bytes, 256-byte aligned): lets shapes whose 144 x 64 tiles would need a
 * part-filled extra round of the 256 CUs (B = 64: 288 tiles) run as a stream-K launch -- the (tile, K chunk) units are dealt out
 * evenly, a tile cut in two is finished by the workgroup holding its tail.  It starts with the same exchange header as above ([0] the
 * error word, sticky).  NULL, or a device that fails the layout guard: plain tiling.  Recordable into a hipGraph.  D % 32 == 0. */
size_t rohm_output_process_scratch_bytes(void);
/* Host-only: the launch plan rohm_output_process_f32 (with scratch) uses for this shape.  Returns 1 for a stream-K launch -- 256
 * workgroups, 32 per XCD; XCD x owns tiles [x * tiles_per_xcd, (x + 1) * tiles_per_xcd) of the 144 x 64 tiling (row tiles of one column
 * tile adjacent), its j-th workgroup (block 8 j + x) the (tile, 32-wide K chunk) units [j u, (j + 1) u) of them in tile-major order,
 * u = units_per_workgroup -- and 0 for plain tiles (outputs set to 0).  tests/test_host_logic.py walks this schedule. */
int rohm_output_process_plan(int B, int T, int D, int C_out, int* units_per_workgroup, int* tiles_per_xcd);
int rohm_output_process_f32(const float* h, const float* w, const float* b, float* out, int B, int T, int D, int C_out,
                            int ch_off, int C_total, void* scratch, size_t scratch_bytes, rohm_stream_t stream);

/* Weight pointers may be host or device memory (copied with hipMemcpyDefault). */
int rohm_posenet_create(rohm_posenet_t** out, const rohm_posenet_weights* w, int d_model, int n_head,
                        int d_ff, int n_layer, int c_in, int c_out, int traj_dim, int device);
void rohm_posenet_destroy(rohm_posenet_t* h);
/* Bytes of caller-owned scratch one forward / sampling call on B clips of T frames needs (ROHM_ERR_WORKSPACE below it).  Besides the
 * activations it holds, per sampling call, the loop-invariant cond half of the input embedding [B (T + 1), D] and -- for handles
 * that fold layer 0's in-projection onto the packed input (d_model 512, d_ff 1024, 4 heads, <= 8 layers, T = 143; default on,
 * ROHM_POSENET_INPROJ_FOLD=0 at create) -- that half pushed through the in-projection, [B (T + 1), 3 D]: 56.6 MB at B = 64.
 * Such a handle itself holds, besides the weights, the folded weight [3 D, 320] and one in-projected timestep token per row of the
 * positional table, [pe_len, 3 D]: 30.7 MB of device memory at pe_len = 5000. */
size_t rohm_posenet_workspace_bytes(const rohm_posenet_t* h, int B, int T);
/* 0: exact fp32 MFMA GEMMs (default); 3 / 2 / 16: the handle was created under ROHM_GEMM_PRECISION=bf16x6 / bf16x3 / fp16x3 and runs
 * the four Linears of every encoder layer (model/posenet.py:63-69) as split-bf16 GEMMs on planes. */
int rohm_posenet_precision(const rohm_posenet_t* h);

/* PoseNet.forward (model/posenet.py:75-96): x_t, cond [B, C_in, 1, T] contiguous, t int64[B]
 * -> x0_out [B, C_in, 1, T] (channels < traj_dim copied from cond, the C_out others predicted). */
int rohm_posenet_forward(const rohm_posenet_t* h, const float* x_t, const float* cond, const int64_t* t,
                         float* x0_out, int B, int T, void* ws, size_t ws_bytes, rohm_stream_t stream);

/* Status of the in-kernel exchanges of the forwards / loops run on workspace `ws` since the last call of this function.  Two of
 * PoseNet's kernels let workgroups of ONE launch hand data to each other through L2 (the LayerNorm inside the out-projection / FF2
 * GEMMs: rohm_gemm_res_layernorm_f32 above; the stream-K output head: rohm_output_process_f32 below).  Their waits are bounded; a
 * wait that runs into its bound (or partners found on different XCDs) sets a word in `ws` that stays set.  This call
 * synchronises `stream`, returns ROHM_ERR_EXCHANGE (and clears the word) if it is set, ROHM_OK otherwise.  Never expected on a
 * whole, exclusively owned MI355X -- the partner workgroups are co-resident by construction, and rohm_posenet_create checks the
 * device before it uses these launches -- but another tenant's long kernels can delay a partner past the bound, and a wrong result
 * must not pass silently: the Python loops call it after every fused chunk of steps (one synchronisation per <= 50 steps) and after
 * every step-wise forward, switch the handle to the exchange-free launches (rohm_posenet_set_exchange) and RE-RUN the chunk.
 * Direct callers of rohm_posenet_forward must call it before they trust the output. */
int rohm_posenet_exchange_status(const rohm_posenet_t* h, int B, int T, void* ws, size_t ws_bytes, rohm_stream_t stream);
/* Byte offset of the exchange header inside a workspace of this shape: [0] the error word (0 fine, 1 a bounded wait expired,
 * 2 partners on different XCDs), [1] 0x524f484d once a call has armed the workspace, [2] the pass counter (advanced on the device by
 * the first kernel of every network pass; the tags of a pass's exchanging launches derive from it).  Diagnostics and tests. */
size_t rohm_posenet_status_offset(const rohm_posenet_t* h, int B, int T);
/* Which launch forms this handle uses for the post-norm tails (model/posenet.py:63-69) and OutputProcess (model/heads.py:171-176):
 * bit 0 LayerNorm inside the out-projection / FF2 GEMMs, bit 1 stream-K output head; bit 2: the environment asked for them but the
 * layout guard refused at create (rohm_posenet_exchange_guard says why: < 256 CUs = a partitioned device, HSA_CU_MASK /
 * ROC_GLOBAL_CU_MASK set, or the probe launch -- 256 one-per-CU workgroups that must be resident together, block b on XCD b % 8 --
 * failed); bit 3: switched off after a failed exchange (rohm_posenet_set_exchange(h, 0)); bit 4: where the shape allows it (whole
 * 144-token clips, d_model 512, d_ff 1024) the four GEMMs between two attention launches -- out-projection + norm1, linear1 + GELU,
 * linear2 + norm2, the next layer's in-projection -- run as ONE launch whose workgroups hand tiles to each other per clip
 * (ROHM_POSENET_CHAIN=0: one launch per GEMM); bit 5: ... and attention too -- the whole encoder stack of a forward is one launch
 * (`encoder_stack_kernel`, the default from 32 clips on; ROHM_POSENET_CHAIN=layer keeps bit 4 without bit 5).  Bits 4 / 5 say what
 * the handle WOULD launch where the shape qualifies (whole clips, B >= 32 or ROHM_POSENET_CHAIN_ANY=1); they need bit 0.
 * ROHM_EXCHANGE_GUARD=off skips the guard, =probe skips its environment shortcut.
 * The chain and the stack address every operand as a scalar base plus a 32-bit byte offset per lane, so they run only where each
 * operand of the call -- activations of M = B * (T + 1) rows and up to 3 * d_model columns, the packed input, the weights -- is
 * smaller than 2^31 bytes; rohm_posenet_stack_addressable is that predicate (1 = fits).  A larger call runs one launch per GEMM.
 * At B = 128 the largest operand is 113 MB, so no supported batch size comes near the bound. */
int rohm_posenet_exchange_mode(const rohm_posenet_t* h);
int rohm_posenet_stack_addressable(long long M, int d_model, int d_ff, int k_pack);
const char* rohm_posenet_exchange_guard(const rohm_posenet_t* h);
/* on = 0: from now on this handle runs the exchange-free launches (GEMM + LayerNorm kernel pair, plain output-head tiles) -- what the
 * sampling loops do, before re-running the chunk, when rohm_posenet_exchange_status reports a failure.  on = 1: back to what the
 * environment asked for and the guard allows -- the guard is asked AGAIN if it had refused at create or the handle had fallen back
 * (a tenant that was resident then may have gone): that re-probe synchronises the device, so on = 1 is a control call between runs.
 * Not to be called while launches of this handle are being issued by another thread. */
int rohm_posenet_set_exchange(rohm_posenet_t* h, int on);
/* Test hook: the next `n_launches` LayerNorm-carrying GEMM launches of this handle publish one column tile's statistics under a
 * wrong tag, so its partners' waits expire (~0.2 s, once) and the error word is set -- a real failed exchange for the fallback tests. */
int rohm_posenet_inject_exchange_fault(rohm_posenet_t* h, int n_launches);
/* Diagnostics: phase timeline of the encoder stack (the one launch that carries nn.TransformerEncoder, model/posenet.py:63-69,92, from
 * 32 clips on).  With a device buffer of rohm_posenet_stack_timeline_bytes(B) bytes set, lane 0 of every workgroup of the following
 * stack launches of this handle (forwards / loop steps at batch size <= B) writes the 100 MHz wall clock at the seams of its phases:
 * buf[(block * 9 + layer) * 12 + k], k = 0 layer entered, 1 qkv of the clip complete (attention starts), 2 attention done, 3 ctx
 * complete, 4 out-projection + norm1 done, 5 met, 6 linear1 + GELU done, 7 met, 8 linear2 + norm2 done, 9 met, 10 next layer's
 * in-projection done; layer 8 = the leading phases (0 entered, 1 embedding done, 2 met, 3 in-projection of layer 0 done, 4 met).
 * Every launch overwrites the stamps.  buf = NULL switches it off (the default; the kernels then pay one scalar test per seam).
 * scripts/stack_timeline.py turns the stamps into per-phase spans and the in-stack attention rate (bench.py roofline.attention). */
size_t rohm_posenet_stack_timeline_bytes(int B);
int rohm_posenet_set_stack_timeline(rohm_posenet_t* h, void* buf, size_t bytes, int B);

/* Device-resident DDPM loop without guidance: p_sample_loop over `n_steps` descending timesteps
 * (diffusion/gaussian_diffusion_posenet.py:578-662, 388-434).
 *   x        [B, C_in, 1, T]  in: x_T, out: final sample (x_{-1})
 *   cond     [B, C_in, 1, T]
 *   t_model  int64[n_steps]   timestep fed to the network at loop step i (after timestep_map)
 *   coef     float[n_steps*3] per loop step: posterior_mean_coef1, posterior_mean_coef2,
 *                             sigma = exp(0.5*posterior_log_variance_clipped) (0 when t == 0)
 *   noise    [n_steps, B, C_in, 1, T] injected Gaussian noise (row i used at loop step i)
 *   x0_last  optional [B, C_in, 1, T]: pred_xstart of the last executed step (early_stop result)
 *   x_in_last optional [B, C_in, 1, T]: the INPUT x_t of the last executed step -- what the reference leaves in
 *            batch['x_t'] after a run (p_mean_variance, gaussian_diffusion_posenet.py:264)
 * All per-step scalars are host arrays (the loop is driven from the host, kernels stay async). */
int rohm_posenet_sample_loop(const rohm_posenet_t* h, float* x, const float* cond, const int64_t* t_model,
                             const float* coef, const float* noise, float* x0_last, float* x_in_last, int n_steps,
                             int B, int T, void* ws, size_t ws_bytes, rohm_stream_t stream);

/* ------------------------------------------------------------------------- PoseNet training
 * train/training_loop_posenet.py: the train-mode forward of PoseNet (model/posenet.py:75-96 with the five dropouts of
 * model/heads.py:126-129 and nn.TransformerEncoderLayer) and its backward.  No handle: `w` holds device pointers to the LIVE
 * parameters on every call (an optimiser step needs no rebuild).  Shapes: d_model 512, 4 heads, d_ff 1024, any n_layer >= 1,
 * c_out + traj_dim == c_in, 1 <= B <= 16383, 1 <= T <= 144; anything else returns ROHM_ERR_UNSUPPORTED (rohm_last_error names
 * the shape).  Exact fp32 (fp32 MFMA), no atomics (bitwise reproducible), no host synchronisation.
 * Dropout (keep-scale 1 / (1 - p), 0 <= p < 1): element e of site s of layer l is kept iff a counter-based hash of (seed, 8 l + s, e)
 * falls below (1 - p) 2^32.  Sites and the flat shapes their e indexes: 0 the PositionalEncoding dropout on the token sequence
 * [B, T + 1, D] (layer 0 only), 1 attention probabilities [B, H, T + 1, T + 1], 2 dropout1 [B, T + 1, D], 3 FF inner after GELU
 * [B, T + 1, F], 4 dropout2 [B, T + 1, D]; token 0 is the timestep token.  The backward regenerates the masks from (seed, p). */
typedef struct {
    float *in_proj_w, *in_proj_b, *out_proj_w, *out_proj_b, *lin1_w, *lin1_b, *lin2_w, *lin2_b;
    float *norm1_w, *norm1_b, *norm2_w, *norm2_b;
} rohm_posenet_layer_grads;

typedef struct {       /* mirrors the weights struct: pe is a buffer and gets no gradient */
    float *in_x_w, *in_x_b, *in_c_w, *in_c_b;
    float *t_w0, *t_b0, *t_w2, *t_b2;
    float *out_w, *out_b;
    const rohm_posenet_layer_grads* layers; /* [n_layer], host array of device pointers */
} rohm_posenet_grads;

/* Bytes of the caller-owned `saved` buffer of rohm_posenet_train_forward (0 for an unsupported shape).  Per layer it keeps the
 * layer input, qkv (q pre-scaled), the softmax probabilities, ctx, both pre-norm sums with their (mean, rstd), norm1's output, the
 * FF1 pre-activation and the dropped GELU output; about 250 MB per layer at B = 64, T = 143. */
size_t rohm_posenet_train_saved_bytes(int d_model, int n_head, int d_ff, int n_layer, int c_in, int c_out, int B, int T);
/* Bytes of the `scratch` of rohm_posenet_train_backward (0 for an unsupported shape). */
size_t rohm_posenet_train_scratch_bytes(int d_model, int n_head, int d_ff, int n_layer, int c_in, int c_out, int B, int T);
/* PoseNet.forward in train mode (model/posenet.py:75-96): x_t, cond [B, c_in, 1, T], t int64 [B] -> out [B, c_in, 1, T] (channels
 * < traj_dim copied from cond), and `saved` for the backward.  The timestep token is computed per sample from pe[t] (Linear -> SiLU
 * -> Linear, model/heads.py:140-146).  saved: 16-byte aligned. */
int rohm_posenet_train_forward(const rohm_posenet_weights* w, int d_model, int n_head, int d_ff, int n_layer, int c_in, int c_out,
                               int traj_dim, const float* x_t, const float* cond, const int64_t* t, int B, int T, float dropout_p,
                               unsigned long long seed, float* out, void* saved, size_t saved_bytes, rohm_stream_t stream);
/* The backward of that forward for d_out = dL/d out [B, c_in, 1, T]: OVERWRITES every gradient in `grads` (108 state-dict
 * tensors), and d_x_t / d_cond (nullable) with dL/dx_t, dL/dcond (d_cond includes the pass-through of the traj_dim channels).
 * Same weights, inputs, dropout_p and seed as the forward that filled `saved` (read only: the call may be repeated). */
int rohm_posenet_train_backward(const rohm_posenet_weights* w, int d_model, int n_head, int d_ff, int n_layer, int c_in, int c_out,
                                int traj_dim, const float* x_t, const float* cond, int B, int T, float dropout_p,
                                unsigned long long seed, const void* saved, size_t saved_bytes, const float* d_out,
                                const rohm_posenet_grads* grads, float* d_x_t, float* d_cond, void* scratch, size_t scratch_bytes,
                                rohm_stream_t stream);
/* keep[e] = 1 if element e < n of dropout site `site` of layer `layer` is kept by the training forward with (seed, dropout_p). */
int rohm_posenet_dropout_mask(unsigned long long seed, int layer, int site, float dropout_p, long long n, uint8_t* keep,
                              rohm_stream_t stream);
/* q_sample (gaussian_diffusion_posenet.py:192-210): out = sqrt_ac[t[b]] x0 + sqrt_1m_ac[t[b]] noise over row_len floats per
 * sample; sqrt_ac / sqrt_1m_ac are device float tables of n_steps entries. */
int rohm_q_sample(const float* x0, const float* noise, const float* sqrt_ac, const float* sqrt_1m_ac, const int64_t* t, int n_steps,
                  int B, long long row_len, float* out, rohm_stream_t stream);

/* ------------------------------------------------------------------------- TrajNet / TrajControl
 * model/trajnet.py:10-275 + model/heads.py:12-106: conv U-Net x0-predictor of the 13-channel trajectory,
 * optional ControlNet branch conditioned on PoseNet's 272-channel local pose. */
typedef struct rohm_trajnet rohm_trajnet_t;
typedef struct {
    const float* data; /* host or device */
    size_t numel;
} rohm_tensor_ref;
/* The parameter tensors in the reference's state_dict order (model/trajnet.py; `controlnet.*` first when
 * trajcontrol): every `weight` immediately followed by its `bias`; 186 tensors, +84 with TrajControl.
 * Conv weights are [C_out, C_in, k] (ConvTranspose1d: [C_in, C_out, k]) exactly as stored in a checkpoint. */
typedef struct {
    const rohm_tensor_ref* tensors;
    int n_tensors;
} rohm_trajnet_weights;

int rohm_trajnet_create(rohm_trajnet_t** out, const rohm_trajnet_weights* w, int mid_dim, int time_dim,
                        int c_traj, int c_ctrl, int trajcontrol, int device);
void rohm_trajnet_destroy(rohm_trajnet_t* h);
size_t rohm_trajnet_workspace_bytes(const rohm_trajnet_t* h, int B, int T);
/* Launch shape of TrajNet's latency-bound convolutions (process-wide; no counterpart in the reference, whose convs are
 * torch's): conv_wg_per_cu = workgroups of a conv GEMM that may share a CU (1 or 2; a 144x64 tile needs 60 KB of the 160 KB
 * LDS), split_min_chunks = fewest 32-wide K chunks a split-K slice may get, split_pow2 != 0 rounds split counts down to
 * powers of two (workgroup b computes split b % S and runs on XCD b % 8: with S a power of two an XCD's L2 holds only its
 * own K slices of the weights).  Results do not depend on them beyond the fp32 summation order of split-K.  The defaults are the measured optimum on MI355X. */
int rohm_trajnet_tune(int conv_wg_per_cu, int split_min_chunks, int split_pow2);

/* TrajNet.forward (model/trajnet.py:177-275): x_t, cond [B, T, c_traj], control_cond [B, T, c_ctrl] (NULL
 * without TrajControl), t int64[B] -> x0_out [B, T, c_traj].  T must be a multiple of 16 with (mid_dim / 64) * T <= 4096, the
 * largest GroupNorm group (T <= 512 at mid_dim 512); a longer clip returns ROHM_ERR_UNSUPPORTED before anything is launched. */
int rohm_trajnet_forward(const rohm_trajnet_t* h, const float* x_t, const float* cond, const float* control_cond,
                         const int64_t* t, float* x0_out, int B, int T, void* ws, size_t ws_bytes,
                         rohm_stream_t stream);

/* Device-resident DDPM loop (diffusion/gaussian_diffusion_trajnet.py:559-627, 440-466); arguments as
 * rohm_posenet_sample_loop with tensors of shape [B, T, c_traj] (x0_last / x_in_last optional, as there). */
int rohm_trajnet_sample_loop(const rohm_trajnet_t* h, float* x, const float* cond, const float* control_cond,
                             const int64_t* t_model, const float* coef, const float* noise, float* x0_last,
                             float* x_in_last, int n_steps, int B, int T, void* ws, size_t ws_bytes,
                             rohm_stream_t stream);

/* Which form the last rohm_trajnet_sample_loop of the calling host thread ran in: 0 one launch per layer, 1 the clip-resident step (one
 * launch per denoising step, an XCD's workgroups stay with its clips and meet through its L2 between the layers -- csrc/trajnet_resident.hip:
 * the default for TrajNet at B <= 64 on a device that passed the exchange probe, opt-in ROHM_TRAJ_RESIDENT=1 for TrajControl, off with
 * ROHM_TRAJ_RESIDENT=0; when it runs, rohm_trajnet_sample_loop waits for the stream once at its end to read the exchange's error word, and
 * a wait that expired hands the call back to form 0 with x restored).  No counterpart in the reference. */
int rohm_trajnet_loop_mode(void);

/* ------------------------------------------------------------------------- TrajNet / TrajControl training
 * train/training_loop_trajnet.py: the train-mode forward of TrajNet (model/trajnet.py:177-275; no dropout, GroupNorm without
 * running statistics: the function of rohm_trajnet_forward) and the backward of the whole conv U-Net with its ControlNet branch.
 * No handle: `w` lists device pointers to the LIVE parameters in the reference's layouts (Conv1d [C_out, C_in, k],
 * ConvTranspose1d [C_in, C_out, k]) in state_dict order, as for rohm_trajnet_create; gradients are written in those layouts.
 * Shapes: mid_dim 512, time_dim 32, 1 <= c_traj <= 32, c_ctrl <= 320, 1 <= B <= 16383, T a multiple of 16 with T <= 512 (the
 * GroupNorm group limit of the inference forward); anything else returns ROHM_ERR_UNSUPPORTED (rohm_last_error names the shape).
 * Exact fp32 (fp32 MFMA), no atomics (bitwise reproducible), no host synchronisation. */
/* Bytes of the caller-owned `saved` buffer of rohm_trajnet_train_forward (0 for an unsupported shape): the zero-haloed inputs, per
 * Conv1dBlock the conv output and the group statistics, per residual block its block-0 activation and output, the concat buffers. */
size_t rohm_trajnet_train_saved_bytes(int mid_dim, int time_dim, int c_traj, int c_ctrl, int trajcontrol, int B, int T);
/* Bytes of the `scratch` of rohm_trajnet_train_backward (0 for an unsupported shape). */
size_t rohm_trajnet_train_scratch_bytes(int mid_dim, int time_dim, int c_traj, int c_ctrl, int trajcontrol, int B, int T);
/* TrajNet.forward in train mode: x_t, cond [B, T, c_traj], control_cond [B, T, c_ctrl] (NULL without TrajControl), t int64 [B]
 * -> out [B, T, c_traj], and `saved` (16-byte aligned) for the backward. */
int rohm_trajnet_train_forward(const rohm_trajnet_weights* w, int mid_dim, int time_dim, int c_traj, int c_ctrl, int trajcontrol,
                               const float* x_t, const float* cond, const float* control_cond, const int64_t* t, int B, int T,
                               float* out, void* saved, size_t saved_bytes, rohm_stream_t stream);
/* The backward of that forward for d_out = dL/d out [B, T, c_traj].  grads: host array of w->n_tensors device pointers, one per
 * parameter in the order of `w`; a NULL entry means the parameter is frozen: its weight-gradient product is not launched, and data
 * gradients are propagated only as far as a non-NULL entry or a wanted input gradient lies upstream.  Every non-NULL gradient
 * is OVERWRITTEN.  cond_downsample4 is never called by the reference and must be NULL.  d_x_t / d_cond / d_control_cond (each
 * nullable) receive dL/dx_t, dL/dcond, dL/dcontrol_cond.  `saved` is read only: the call may be repeated. */
int rohm_trajnet_train_backward(const rohm_trajnet_weights* w, int mid_dim, int time_dim, int c_traj, int c_ctrl, int trajcontrol,
                                int B, int T, const void* saved, size_t saved_bytes, const float* d_out, float* const* grads,
                                float* d_x_t, float* d_cond, float* d_control_cond, void* scratch, size_t scratch_bytes,
                                rohm_stream_t stream);
/* GEMM launches (conv, data-gradient and weight-gradient products) of the process's last rohm_trajnet_train_backward:
 * a frozen backbone launches fewer than an all-trainable step. */
int rohm_trajnet_train_last_gemms(void);

/* ------------------------------------------------------------------------- SMPL-X + guidance
 * Joints-only SMPL-X (third-party smplx==0.1.28 `SMPLX.forward` / `lbs`, called from
 * data_loaders/motion_representation.py:389) and the two test-time guidance gradients of
 * model/posenet.py:196-317.  The hot path reads only joints[:, 0:22]; those depend on
 * J_regressor.(v_template + shapedirs.beta) and the kinematic chain, never on vertices, so the
 * regressor is folded once at create time (fp64 accumulation) and a step is O(22) 3x3 products
 * per frame instead of full linear blend skinning. */
typedef struct rohm_smplx rohm_smplx_t;

/* v_template [V,3], shapedirs [V,3,n_shape_total] (first 10 = betas), J_regressor [J,V], parents int32[J];
 * pointers may be host or device memory. */
int rohm_smplx_create(rohm_smplx_t** out, const float* v_template, const float* shapedirs, int n_shape_total,
                      const float* J_regressor, const int32_t* parents, int V, int J, int device);
void rohm_smplx_destroy(rohm_smplx_t* h);

/* joints[N, n_out, 3] (n_out <= 22) from axis-angle pose [N, n_pose, 3] (global orient first; joints beyond
 * n_pose are unrotated), betas [N,10], transl [N,3]: Rodrigues (angle = |r + 1e-8|) + forward kinematics. */
int rohm_smplx_joints(const rohm_smplx_t* h, const float* pose, int n_pose, const float* betas,
                      const float* transl, int N, float* joints, int n_out, rohm_stream_t stream);

/* Dataset-side per-frame SMPL-X work, batched over the frames of a recording (data_loaders/dataloader_video.py:121-142,
 * :282-300 -- one smplx call, one cam2world transform and one update_globalRT_for_smplx (utils/other_utils.py:189-240)
 * PER FRAME there): axis-angle global_orient [N,3], body_pose [N,63], betas [N,10], transl [N,3] (device, float32),
 * rigid = cam2world [4,4] row-major (device float32) -> joints_world [N,22,3] (float32) and orient_transl_world [N,6]
 * (float64: new global_orient, new transl -- the two entries of the parameter dict the function rewrites). */
int rohm_smplx_frames_to_world(const rohm_smplx_t* h, const float* global_orient, const float* body_pose,
                               const float* betas, const float* transl, const float* rigid, int N, float* joints_world,
                               double* orient_transl_world, rohm_stream_t stream);

size_t rohm_guidance_workspace_bytes(int B, int T);

/* guide_skating_with_smpl (model/posenet.py:196-257, compute_grad='x_0'): x0 [B,294,1,T] normalised
 * prediction, mean294/std294 the dataset statistics -> grad_out [B,294,1,T] = d(-loss)/dx0 with channels
 * [0,22) and [290,294) zeroed.  counts2 (device float[2]) receives the two skating-mask counts
 * (abs-trajectory, SMPL-X recovery); both zero <=> the reference returns a 0-d zero, and grad_out is
 * then all zeros. */
int rohm_guidance_skating_grad(const rohm_smplx_t* h, const float* x0, const float* mean294, const float* std294,
                               int B, int T, float* grad_out, float* counts2, void* ws, size_t ws_bytes,
                               rohm_stream_t stream);

/* The two halves of rohm_guidance_skating_grad, for clip sharding with GLOBAL-batch semantics:
 * the loss normalises by mask counts over the whole batch (model/posenet.py:231,243), so each rank runs `prepare`
 * (local counts -> counts2), the host all-reduces the 2 floats (RCCL), and `apply` uses the summed counts.  `apply`
 * must follow `prepare` on the same x0 / workspace. */
int rohm_guidance_skating_prepare(const rohm_smplx_t* h, const float* x0, const float* mean294, const float* std294,
                                  int B, int T, float* counts2, void* ws, size_t ws_bytes, rohm_stream_t stream);
int rohm_guidance_skating_apply(const rohm_smplx_t* h, const float* x0, const float* mean294, const float* std294,
                                int B, int T, const float* counts2, float* grad_out, void* ws, size_t ws_bytes,
                                rohm_stream_t stream);

/* guide_2d_projection_with_smpl (model/posenet.py:260-317): transf_matrix [B,4,4] (affine, inverted on the
 * device), cam_R [3,3], cam_t [3], focal / center [B,2], kp2d [B, kp_frames, 22, 3] (u, v, confidence). */
int rohm_guidance_proj2d_grad(const rohm_smplx_t* h, const float* x0, const float* mean294, const float* std294,
                              const float* transf_matrix, const float* cam_R, const float* cam_t,
                              const float* focal, const float* center, const float* kp2d, int kp_frames, int B,
                              int T, float* grad_out, void* ws, size_t ws_bytes, rohm_stream_t stream);

/* Full linear blend skinning (smplx==0.1.28 `lbs`, as called with return_verts=True from
 * data_loaders/motion_representation.py:389-396; the post-loop meshes of test_amass_full.py:405-425).  Optional:
 * rohm_smplx_set_skinning uploads what the joints-only path does not need -- posedirs [(J-1)*9, V*3] (pose_feature
 * @ posedirs layout of smplx), lbs_weights [V, J] (+ v_template, shapedirs again) -- after which
 * rohm_smplx_forward produces joints [N, n_joints_out, 3] (may be NULL) and verts [N, V, 3] (may be NULL: joints only)
 * from poses pose [N, n_pose, 3] (pose_kind 0: axis-angle) or [N, n_pose, 6] (pose_kind 1: the interleaved 6-D vectors
 * of the motion representation, quaternion.py:482-501); global orient first; joints >= n_pose unrotated; expression = 0;
 * betas [N,10], transl [N,3].  ws: rohm_smplx_lbs_workspace_bytes(h, N), 256-byte aligned.  N <= 65535 per call.
 * The shape and pose blendshapes are one fp32-MFMA GEMM; the skinning blend T = W . A runs on the matrix core too when
 * lbs_weights is dense (mode 0), and over per-vertex ELL rows of the non-zero weights when >= 75 % of it is zero and no vertex
 * has more than 16 non-zero joints -- what a released SMPLX_*.npz looks like (mode 1).  rohm_smplx_skinning_mode reports the
 * choice made at rohm_smplx_set_skinning (-1: not set; 2: ELL rows of all joints, ROHM_LBS_SKIN=ell). */
int rohm_smplx_skinning_mode(const rohm_smplx_t* h);
int rohm_smplx_set_skinning(rohm_smplx_t* h, const float* v_template, const float* shapedirs, int n_shape_total,
                            const float* posedirs, int n_pose_feat, const float* lbs_weights);
size_t rohm_smplx_lbs_workspace_bytes(const rohm_smplx_t* h, int N);
int rohm_smplx_forward(const rohm_smplx_t* h, const float* pose, int n_pose, int pose_kind, const float* betas, const float* transl,
                       int N, float* joints, int n_joints_out, float* verts, void* ws, size_t ws_bytes,
                       rohm_stream_t stream);

/* recover_from_repr_smpl (data_loaders/motion_representation.py:332-398) straight from the 294-channel
 * representation: joints [B,T,22,3].  mode 0 = 'smplx_params' (:373-398, joints[:, 0:22] of the body model incl.
 * transl; h required), mode 1 = 'joint_abs_traj' (:349-371; h may be NULL), mode 2 = 'joint_rel_traj' (:312-329: root
 * angle / position as running sums of the per-frame velocities; h may be NULL).  repr is addressed with strides as in
 * rohm_traj_rederive; mean294/std294 de-normalise on the fly (both NULL = repr is already de-normalised). */
int rohm_repr_joints(const rohm_smplx_t* h, const float* repr, long long in_stride_b, long long in_stride_t,
                     long long in_stride_c, const float* mean294, const float* std294, int B, int T, int mode,
                     float* joints, rohm_stream_t stream);

/* Vector-Jacobian product of rohm_repr_joints: the same recovery arguments, plus d_joints [B,T,22,3] (dL/djoints,
 * contiguous).  Writes dL/drepr into d_repr, element (b, t, c) at d_repr[b*out_stride_b + t*out_stride_t +
 * c*out_stride_c], for all 294 channels (0 on those the mode does not read); with mean294/std294 this is the gradient
 * with respect to the NORMALISED input (the de-normalisation's factor std included).  Used to backpropagate the joint
 * terms of PoseNet.compute_losses_with_smpl (model/posenet.py:98-194) into the network output.  mode 0 differentiates
 * the Gram-Schmidt matrices directly: the reference's R -> axis-angle -> Rodrigues round trip is the identity on SO(3).
 * mode 2 runs the running sums over frames backwards (T <= 2048).  No atomics: bitwise reproducible.  d_repr must not
 * overlap repr. */
int rohm_repr_joints_vjp(const rohm_smplx_t* h, const float* repr, long long in_stride_b, long long in_stride_t,
                         long long in_stride_c, const float* mean294, const float* std294, int B, int T, int mode,
                         const float* d_joints, float* d_repr, long long out_stride_b, long long out_stride_t,
                         long long out_stride_c, rohm_stream_t stream);

/* Between-stage trajectory re-derivation: replaces the drivers' host round trip
 * test_amass_full.py:262-311 / test_prox_egobody.py:238-287 -- de-normalise TrajNet's representation,
 * recover_from_repr_smpl('smplx_params') (data_loaders/motion_representation.py:373-398), per-sequence
 * get_repr_smplx (:187-282), re-normalise, keep the 22 trajectory channels.
 * repr: element (b, t, c) at repr[b*in_stride_b + t*in_stride_t + c*in_stride_c] (floats), c < 294, t < T, normalised
 * with (mean_in, std_in); out: element (b, t, c), t < T-1, c < 22, at out[b*out_stride_b + t*out_stride_t +
 * c*out_stride_c], normalised with (mean_out, std_out) -- so the result can be written straight into channels 0..21
 * of PoseNet's `cond` in either layout.  2 <= T <= 800.  Degenerate facing directions reproduce the reference's NaN
 * handling (only the first NaN frame of a clip is patched with its predecessor, :212-215). */
int rohm_traj_rederive(const rohm_smplx_t* h, const float* repr, long long in_stride_b, long long in_stride_t,
                       long long in_stride_c, const float* mean_in, const float* std_in, const float* mean_out,
                       const float* std_out, int B, int T, float* out, long long out_stride_b,
                       long long out_stride_t, long long out_stride_c, rohm_stream_t stream);

/* Test-time clips of a PROX / EgoBody recording (data_loaders/dataloader_video.py:373-403): for every clip
 * cano_seq_smplx (up_axis 2 = z; data_loaders/motion_representation.py:47-110) or cano_seq_smplx_egobody (up_axis 1 = y;
 * :113-184), update_globalRT_for_smplx with delta_T = positions[:,0] - transl, and the full 294-channel get_repr_smplx
 * (:187-282, feet_vel_thre 5e-5), one workgroup per clip on `stream`, no host synchronisation.
 * joints_world [N,22,3] float32 and smplx_world [N,79] float64 are what rohm_smplx_frames_to_world produces (+ betas,
 * body_pose); clip c covers frames starts[c] .. starts[c] + clip_len - 1 (device int32 [C]) or, with starts == NULL,
 * starts at c * (clip_len - overlap).  A window that leaves [0, N) yields NaN outputs for that clip, never a read
 * outside the arrays.  2 <= clip_len <= 800; C == 0 returns without a launch.
 * has_preset_floor != 0 uses preset_floor instead of the clip's lowest joint, except that 0.0 counts as "not given"
 * (`if preset_floor_height:`).  mean294 / std294 (both or neither) normalise the representation.
 * Outputs (float32): repr [C, clip_len-1, 294], cano_joints [C, clip_len, 22, 3], cano_orient / cano_transl
 * [C, clip_len, 3], transf [C, 4, 4] (scene -> canonical).  scratch: rohm_clips_scratch_bytes(C, clip_len) bytes, 0
 * while the float64 canonical joints of a clip fit into LDS (clip_len <= 255). */
size_t rohm_clips_scratch_bytes(int C, int clip_len);
int rohm_clips_build(const float* joints_world, const double* smplx_world, int N, const int* starts, int C,
                     int clip_len, int overlap, int up_axis, int has_preset_floor, double preset_floor,
                     const float* mean294, const float* std294, float* repr, float* cano_joints, float* cano_orient,
                     float* cano_transl, float* transf, void* scratch, size_t scratch_bytes, rohm_stream_t stream);

/* rohm_clips_build with one more output: orient_transl64 [C, clip_len, 6] (float64; may be NULL), the canonical
 * global_orient and transl before their float32 store -- data_loaders/dataloader_amass.py keeps them in float64 up to the
 * body-model call (:152-197).  Same kernel; every other output is bit-identical to rohm_clips_build's. */
int rohm_clips_build_f64(const float* joints_world, const double* smplx_world, int N, const int* starts, int C,
                         int clip_len, int overlap, int up_axis, int has_preset_floor, double preset_floor,
                         const float* mean294, const float* std294, float* repr, float* cano_joints, float* cano_orient,
                         float* cano_transl, float* transf, double* orient_transl64, void* scratch, size_t scratch_bytes,
                         rohm_stream_t stream);

/* get_repr_smplx (data_loaders/motion_representation.py:187-282, feet_vel_thre 5e-5) on clips that are canonical already
 * -- the second half of rohm_clips_build: positions [C, clip_len, 22, 3] (float32, or float64 with positions_f64 != 0),
 * params [C, clip_len, 79] float64 (global_orient, transl, betas, body_pose) -> repr [C, clip_len-1, 294] float32.  What
 * the reference computes in the joints' dtype (across vector, position differences, squared foot velocities) is float32
 * arithmetic for float32 positions and float64 arithmetic for float64 ones; NaN handling, mean294 / std294, the LDS /
 * scratch rule (rohm_clips_scratch_bytes) and the limits on clip_len are those of rohm_clips_build.
 * joint_noise [C, clip_len, 22, 3] (float64; may be NULL): the joints become float32(positions + joint_noise) first
 * (dataloader_amass.py:305-307).  joints_out (float32; may be NULL) receives the joints the representation was made of. */
int rohm_clips_repr(const void* positions, int positions_f64, const double* params, const double* joint_noise, int C,
                    int clip_len, const float* mean294, const float* std294, float* repr, float* joints_out, void* scratch,
                    size_t scratch_bytes, rohm_stream_t stream);

/* SMPL-X parameter noise of the AMASS loader (dataloader_amass.py:156-192), float64 throughout, one thread per rotation:
 * params / out [M,79] rows (global_orient, transl, betas, body_pose); noise_orient [M,3] and noise_pose [M,63] are in
 * degrees and are added to the 'zxy' Euler angles scipy's lowercase (extrinsic) as_euler gives, the result going back
 * through from_euler(...).as_rotvec() (rotation angle in [0, pi]); noise_transl [M,3] and noise_betas [M,10] are added.
 * additive != 0 adds all four arrays to the parameters as they are (the sep_noise items, :298-303).  The kernel draws
 * nothing; out must not alias params. */
int rohm_smplx_param_noise(const double* params, const double* noise_orient, const double* noise_transl,
                           const double* noise_betas, const double* noise_pose, long long M, int additive, double* out,
                           rohm_stream_t stream);

/* Per-channel mean and population standard deviation of repr [rows, 294] (float32; dataloader_amass.py:254-258) into
 * mean294 / std294 (device float64 [294]).  float64 accumulation in two stages -- per-workgroup (mean, sum of squared
 * deviations) of a block of rows, then one workgroup that folds them in order -- so the result is bitwise reproducible.
 * scratch: rohm_repr_stats_scratch_bytes(rows) bytes. */
size_t rohm_repr_stats_scratch_bytes(long long rows);
int rohm_repr_stats(const float* repr, long long rows, double* mean294, double* std294, void* scratch, size_t scratch_bytes,
                    rohm_stream_t stream);

/* dataloader_amass.py:317-339 for the B items index[b] (device int64; an index outside [0, n_items) gives NaN rows):
 * repr_clean / repr_noisy [n_items, rows_per_item, 294] de-normalised (repr_noisy NULL: input_noise = False, the noisy
 * item is the clean one; with noisy_per_batch != 0 it is [B, rows_per_item, 294], row b for batch entry b: the sep_noise
 * items, which are made per batch) -> out_clean, out_noisy [B, rows_per_item, 294] = (x - mean) / std in float64, rounded once.
 * The first overwrite_channels noisy channels are taken from the clean item before normalising (task 'pose', :324).
 * cond_kind 1: cond [B, rows, 22] = the first 22 noisy channels; 2: cond [B, rows, 13] = channels 0, 2, 3, 6, 7..12,
 * 16..18 (:337); 0: none.  control_cond [B, rows, 272] (may be NULL) = the last 272 clean channels. */
int rohm_amass_batch(const float* repr_clean, const float* repr_noisy, long long n_items, int rows_per_item,
                     const long long* index, int B, const float* mean294, const float* std294, int overwrite_channels,
                     int noisy_per_batch, int cond_kind, float* out_clean, float* out_noisy, float* cond, float* control_cond,
                     rohm_stream_t stream);

/* The per-frame work of preprocessing_amass.py:47-69 for N frames of R recordings that lie back to back (all device pointers):
 * every input is cast float64 -> float32 with round-to-nearest-even, as torch.Tensor(ndarray) does (:48-55); params [N,178] is
 * the row of :68 -- root_orient 3, trans 3, betas 10, pose_body 63, pose_hand 90, pose_jaw 3, pose_eye[:, 0:3] and
 * pose_eye[:, 0:3] AGAIN (:54-55 read the left eye twice; the script's comment says 169, the row has 178 columns) -- and
 * joints [N,25,3] is smplx_output.joints[:, 0:25] of :65-66 in float32 from the cast values: Rodrigues (angle = |r + 1e-8|) and
 * the chain of rohm_smplx_joints for joints 0..21, P[j] = P[p] + G[p] (Jrest[j] - Jrest[p]), p = parents[j], for the leaves
 * 22..24 (jaw, eyes), plus trans.  Those joints depend on betas, root_orient, pose_body and trans only (hand_pose is no argument
 * of SMPLX.forward, and the jaw / eye rotations turn nothing that is read), so no vertices are computed.  betas [R,10] holds
 * bdata['betas'][:10] of each recording (:50); rec_of_frame [N] in [0, R) picks a frame's row (a value outside gives NaN betas).
 * The handle needs J >= 25 and parents[22..24] among the 22 body joints (argument error otherwise).  Runs on `stream` without
 * synchronising; N == 0 returns without a launch. */
int rohm_amass_preprocess(const rohm_smplx_t* h, const double* root_orient, const double* trans, const double* pose_body,
                          const double* pose_hand, const double* pose_jaw, const double* pose_eye, const double* betas,
                          const int32_t* rec_of_frame, int N, int R, float* joints, float* params, rohm_stream_t stream);

/* dataloader_video.py:441-458 for M keypoints [M,3] (x, y, confidence; device float32): x -> image_width - 1 - x,
 * cv2.undistortPoints(src, camera_mtx, dist, P = camera_mtx) (five fixed-point iterations of the inverse of the
 * k1 k2 p1 p2 k3 model), x flipped back; the confidence passes through.  camera_mtx9 (row-major 3x3) and dist5 are HOST
 * arrays; float64 arithmetic, float32 store.  out may alias keypoints. */
int rohm_keypoints_undistort(const float* keypoints, long long M, const double* camera_mtx9, const double* dist5,
                             double image_width, float* out, rohm_stream_t stream);

/* dataloader_video.py:462-484 with the windows of rohm_clips_build read in place: keypoints [N,22,3] (confidence in
 * column 2), mask_joint [N, mask_cols >= 22] (device float32) -> mask_joint_vis [C, clip_len, 22] =
 * (conf > 0.2) * mask_joint and mask_vec_vis [C, clip_len, 294]: ones on the trajectory channels and the betas, the joint
 * masks x3 on local_positions / local_vel and x6 on smplx_body_pose_6d (joints 1..21), and on the contact channels 1
 * where both foot joints (7 & 10 left, 8 & 11 right) are visible. */
int rohm_visibility_masks(const float* keypoints, const float* mask_joint, int mask_cols, int N, const int* starts,
                          int C, int clip_len, int overlap, float* mask_joint_vis, float* mask_vec_vis,
                          rohm_stream_t stream);

/* AMASS evaluation metrics (eval_amass_full.py:67-147) as per-clip partial sums.  joints_clean / joints_rec
 * [B,T,22,3]; contact_* point at the 4 contact channels of the de-normalised clean / reconstructed representation
 * of frame (b, t) = contact[(b*T + t)*stride + k].  A (frame, joint) counts as occluded if bit `joint` of
 * occ_joint_mask is set (mask_scheme 'lower': joints 1,2,4,5,7,8,10,11, :76) or occ_start <= frame < occ_end
 * ('full': [65, 65 + int(ratio*145)), :84-87).  out [B,10] doubles:
 *   0 sum |clean - rec| over T*22        1 the same over occluded entries      2 number of occluded entries
 *   3 matching contact labels (of T*4)   4 skating frames, clean (of T-1)      5 skating frames, rec
 *   6 sum |accel_rec - accel_clean| over (T-2)*22    7 toe entries below -0.05 m (of T*2)
 *   8 sum of negative toe heights        9 min height of the clean clip (the ground reference, :105)
 * The script's numbers are sums over clips divided by the counts in brackets. */
int rohm_amass_metrics(const float* joints_clean, const float* joints_rec, const float* contact_clean,
                       long long contact_clean_stride, const float* contact_rec, long long contact_rec_stride,
                       unsigned occ_joint_mask, int occ_start, int occ_end, int B, int T, double* out,
                       rohm_stream_t stream);

/* PROX / EgoBody evaluation metrics (eval_prox_egobody.py:172-270) as per-clip partial sums, one workgroup per clip.
 * joints_rec [B,T,22,3] in canonical coordinates; each clip is mapped back to scene coordinates with
 * inv(trans_scene2cano[b]) ([B,4,4], a general matrix inverted in float64, rounded to float32, then applied as
 * points_coord_trans, utils/other_utils.py:139-143).  ground_height [B] (floats: a batch may mix recordings);
 * up_axis 2 = PROX (z up, horizontal x/y), 1 = EgoBody (y up, horizontal x/z).  joints_gt [B,T_gt,22,3] (scene
 * coordinates, first T frames used, T_gt >= T) and mask_vis [B,T,22] (1 = visible; only with joints_gt) may be NULL.
 * joints_scene [B,T,22,3] receives the back-transformed joints when non-NULL.  3 <= T <= 800.  out [B,11] doubles:
 *   0 skating frames (of T-1)             1 sum |acc_rec| (of (T-2)*22)     2 sum |acc_rec - acc_gt| (of (T-2)*22)
 *   3 toe entries with d < -0.05 (of 2T)  4 sum min(d, 0) over toes (of 2T)  5 sum global error (of 22T)
 *   6 sum local (root-relative) error (of 22T)   7 sum local*mask   8 sum mask   9 sum local*(1-mask)   10 sum (1-mask)
 * with d = toe height - ground_height; 2 and 5-10 are 0 without joints_gt, 7-10 without mask_vis.  The script's
 * numbers are sums over clips divided by the counts in brackets (vis / occ: 7 / 8 and 9 / 10).  No allocation, no
 * synchronisation. */
int rohm_scene_metrics(const float* joints_rec, const float* trans_scene2cano, const float* ground_height, int up_axis,
                       const float* joints_gt, int T_gt, const float* mask_vis, float* joints_scene, int B, int T,
                       double* out, rohm_stream_t stream);

/* Depth rendering and PROX joint-occlusion masks (csrc/raster.hip): utils/get_occlusion_mask.py without pyrender, trimesh or
 * OpenCV.  One coverage rule everywhere: a pinhole camera in OpenCV axes (x right, y down, z forward: pyrender's
 * IntrinsicsCamera under the script's diag(1, -1, -1, 1) pose, get_occlusion_mask.py:64-69); pixel (x, y) samples the ray
 * through u = x + 0.5, v = y + 0.5; its depth is the smallest camera-space z, znear <= z <= zfar, at which that ray meets
 * any triangle, 0 where it meets none (pyrender's znear / zfar defaults are 0.05 / 100).  Meshes are two-sided unless
 * cull_backfaces != 0, which drops triangles that run clockwise as seen from the camera (OpenGL's default under pyrender;
 * scene scans are open surfaces, so the two differ where a surface is seen from behind).  Triangles may cross z = 0 or lie
 * behind the camera: the test uses homogeneous edge functions in fp64 and needs no clipper; depths are fp32.
 *
 * rohm_depth_render replaces the two r.render calls (get_occlusion_mask.py:82-88 for the scene, :122-129 per body):
 * verts [n_mesh, V, 3] fp32 and faces [F, 3] int32 (one face list for all meshes) on the device; transform: 16 floats in
 * HOST memory, a row-major 4 x 4 rigid transform applied to every vertex on the device (the script's
 * apply_transform(inv(cam2world)), :77-78), or NULL for vertices already in camera space.  depth [n_mesh, H, W] fp32.
 * Faces with an index outside [0, V) are skipped.  ws: rohm_depth_workspace_bytes(n_mesh, F, W, H) bytes, 256-byte
 * aligned (about 108 bytes per triangle); nothing is allocated, the stream is the caller's and is never synchronised.
 * Depths are merged with an unsigned min on the float's bit pattern: the image is bitwise reproducible.
 *
 * rohm_depth_probe is the same rule at listed pixels only: pixels [n_mesh, P, 2] int32 (x, y) in, depth [n_mesh, P] out;
 * a pixel outside the image yields 0.  It agrees bit for bit with the rendered image at those pixels and is what the
 * mask needs (25 pixels of every frame's body, :138-143) without one 8 MB image per frame.  No workspace. */
size_t rohm_depth_workspace_bytes(int n_mesh, int F, int W, int H);
int rohm_depth_render(const float* verts, const int* faces, int n_mesh, int V, int F, const float* transform, double fx,
                      double fy, double cx, double cy, int W, int H, double znear, double zfar, int cull_backfaces,
                      float* depth, void* ws, size_t ws_bytes, rohm_stream_t stream);
int rohm_depth_probe(const float* verts, const int* faces, int n_mesh, int V, int F, const float* transform, double fx,
                     double fy, double cx, double cy, int W, int H, double znear, double zfar, int cull_backfaces,
                     const int* pixels, int P, float* depth, rohm_stream_t stream);

/* cv2.projectPoints with zero rotation and translation (get_occlusion_mask.py:43-46, :133-136): joints [N, J, 3] fp32 in
 * camera space on the device; camera_mtx (9 doubles, row-major 3 x 3) and dist (k1, k2, p1, p2, k3) in HOST memory.
 * OpenCV's published model in fp64: x' = X / Z, y' = Y / Z (Z == 0 divides by 1), r2 = x'^2 + y'^2,
 * x" = x' (1 + k1 r2 + k2 r2^2 + k3 r2^3) + 2 p1 x' y' + p2 (r2 + 2 x'^2), y" = y' (...) + p1 (r2 + 2 y'^2) + 2 p2 x' y',
 * u = fx x" + cx, v = fy y" + cy; then astype(int), i.e. truncation toward zero.  pixels [N, J, 2] int32 (x, y), the
 * input of the probe; a value beyond the int range becomes INT_MIN, outside every image. */
int rohm_project_pixels(const float* joints, const double* camera_mtx, const double* dist, int N, int J, int* pixels,
                        rohm_stream_t stream);

/* The mask decision, get_occlusion_mask.py:138-143: projects as rohm_project_pixels does, then a joint is occluded
 * (mask 0) iff its pixel lies inside the W x H image, scene_depth there is not 0 and body_depth - scene_depth > thr
 * (a float32 difference, as on the script's float32 images; thr is 0.1 there); every other joint is visible (mask 1).
 * scene_depth [H, W] from the renderer, body_depth [N, J] from the probe at the projected pixels, mask [N, J] fp32. */
int rohm_joint_occlusion_mask(const float* joints, const double* camera_mtx, const double* dist, const float* scene_depth,
                              int W, int H, const float* body_depth, float thr, int N, int J, float* mask,
                              rohm_stream_t stream);

/* Evaluation pictures (csrc/shade.hip): the render path of eval_amass_full.py:277-395, eval_prox_egobody.py:373-451 and
 * utils/render_util.py without pyrender, trimesh, an OpenGL context or PIL.  Device pointers, the caller's stream, never
 * synchronised, nothing allocated.
 *
 * rohm_vertex_normals: smooth normals in gather form (no float atomics, hence the same bits on every call).  verts
 * [n_mesh, V, 3] fp32, faces [F, 3] int32 and the vertex -> face adjacency in CSR form, offsets [V + 1] and face_ids [3F]
 * int32 (the faces of vertex v are face_ids[offsets[v] .. offsets[v + 1])).  Thread (mesh, vertex) sums the un-normalised
 * (p1 - p0) x (p2 - p0) of its faces in list order, which weights by area, and normalises, in fp32.  A vertex with no
 * face, or with a zero sum, gets (0, 0, 0).  normals [n_mesh, V, 3] fp32.
 *
 * rohm_color_render: mesh, camera, transform and workspace arguments are those of rohm_depth_render (the workspace size
 * comes from rohm_color_workspace_bytes).  normals [n_mesh, V, 3] fp32 in the vertices' coordinates, or NULL for flat
 * shading with the face normal; colors uint8 [n_mesh, V, 4] (colors_per_mesh != 0) or [1, V, 4] (== 0) RGBA; outputs rgba
 * uint8 [n_mesh, H, W, 4] and, when not NULL, depth fp32 [n_mesh, H, W] and face_id int32 [n_mesh, H, W] (-1: nothing hit).
 * The rule:
 *   - Coverage and depth are exactly the rule above; the depth output equals rohm_depth_render's image bit for bit.
 *   - Winner of a pixel: the smallest fp32 depth pattern; among equal patterns the smallest face index.  The tile's LDS
 *     z-buffer holds a 64-bit key (depth bits << 32) | face per pixel, merged with an unsigned 64-bit atomic min:
 *     order-independent, hence bitwise reproducible.
 *   - Resolve, once per covered pixel after the tile's triangles are merged.  Weights l_i = e_i / (e_0 + e_1 + e_2) from
 *     the winner's edge functions in fp64: the perspective-correct barycentrics of the hit point.  Normal
 *     n = normalise(sum l_i n_i), the n_i taken to camera space by the call's rotation; the normalised face normal
 *     (p1 - p0) x (p2 - p0) when normals is NULL.  Without the cull flag a normal facing away from the eye (n . d > 0, d the
 *     pixel's ray) is negated.  One directional light along the viewing axis (the reference places its light at the camera
 *     pose): lambert = max(0, -n_z) in the OpenCV axes.  Colour c_k = sum l_i C_ik / 255, alpha a = sum l_i A_i / 255;
 *     out_k = floor(255 min(1, c_k (ambient + diffuse lambert)) + 0.5), out_a = floor(255 a + 0.5); a missed pixel is
 *     (0, 0, 0, 0).  Shading arithmetic is fp32.
 *   - The reference's scene has ambient 0.3; its intensity-3 light on a non-metallic material gives diffuse 3 / pi.  No
 *     specular term, no sRGB curve, and nothing behind a translucent surface is blended: the nearest surface is drawn and
 *     its alpha written.  These are stated differences from pyrender; nothing is pinned to it, as for depth.
 *
 * rohm_skeleton_mesh: create_pyrender_skel's geometry (render_util.py:119-158), batched.  joints [N, J, 3]; a unit sphere
 * template [Vs, 3] and a unit cylinder template [Vc, 3] (axis z, from 0 to 1); limbs [L, 2] int32 joint pairs; hide
 * [N, J + L] bytes (or NULL).  verts [N, J Vs + L Vc, 3]: sphere j is joint j + r_joint x template; cylinder l runs from
 * p1 = joint limbs[l][0] to p2 = joint limbs[l][1] in the frame a = (p2 - p1) / |p2 - p1|, u = normalise(a x e) with e the
 * coordinate axis of smallest |a . e| (ties: the lowest index), w = a x u: p1 + r_limb (x u + y w) + z |p2 - p1| a.  A
 * hidden primitive, or a limb of zero length, collapses onto its first joint; the renderer drops zero-area triangles, so
 * one face list serves the whole batch.
 *
 * The scripts' image arithmetic on uint8 images, elementwise and bit for bit:
 *   rohm_image_requantize  render_img: every RGBA channel x -> float32(x) / 255, alpha times `alpha`, then (x * 255)
 *                          truncated to uint8 (the colour channels take the same round trip).
 *   rohm_image_paste       Image.paste(src, (0, 0), src) in place on an RGB or RGBA destination: with a = src alpha,
 *                          t = src a + dst (255 - a) + 128, out = (t + (t >> 8)) >> 8 on every destination channel.
 *   rohm_image_overlay     render_img_overlay: src's rgb where src alpha > 0, dst_rgb elsewhere -> out [.., 3].
 *   rohm_image_flip_lr     Image.FLIP_LEFT_RIGHT on rows x W pixels of `channels` bytes; in and out must differ. */
int rohm_vertex_normals(const float* verts, const int* faces, const int* offsets, const int* face_ids, int n_mesh, int V,
                        int F, float* normals, rohm_stream_t stream);
size_t rohm_color_workspace_bytes(int n_mesh, int F, int W, int H);
int rohm_color_render(const float* verts, const int* faces, int n_mesh, int V, int F, const float* transform, double fx,
                      double fy, double cx, double cy, int W, int H, double znear, double zfar, int cull_backfaces,
                      const float* normals, const unsigned char* colors, int colors_per_mesh, float ambient, float diffuse,
                      unsigned char* rgba, float* depth, int* face_id, void* ws, size_t ws_bytes, rohm_stream_t stream);
int rohm_skeleton_mesh(const float* joints, int N, int J, const float* sphere, int Vs, const float* cylinder, int Vc,
                       const int* limbs, int L, float r_joint, float r_limb, const unsigned char* hide, float* verts,
                       rohm_stream_t stream);
int rohm_image_requantize(const unsigned char* rgba, float alpha, long long n_pixels, unsigned char* out,
                          rohm_stream_t stream);
int rohm_image_paste(unsigned char* dst, int dst_channels, const unsigned char* src_rgba, long long n_pixels,
                     rohm_stream_t stream);
int rohm_image_overlay(const unsigned char* dst_rgb, const unsigned char* src_rgba, long long n_pixels, unsigned char* out,
                       rohm_stream_t stream);
int rohm_image_flip_lr(const unsigned char* in, long long rows, int W, int channels, unsigned char* out,
                       rohm_stream_t stream);

/* The condition masks of the training loops (csrc/train_masks.hip).  The loop decides on the host what to hide; the device
 * applies it.  Device pointers unless stated, the caller's stream, never synchronised, nothing allocated.
 *
 * rohm_train_cond: PoseNet's training condition of a batch, training_loop_posenet.py:107-205 (and :221-248 of the eval block), in
 * one launch.  src [B, T, 294] float32 (the batch's normalised motion_repr_noisy or motion_repr_clean rows) ->
 * cond [B, 294, 1, T]; with clean [B, T, 294] also clean_t [B, 294, 1, T] = clean transposed, bit for bit (the loop's two
 * permute(0, 2, 1).unsqueeze(-2) copies).  1 <= T <= 512.  Per item, each NULL or present:
 *   joint_bits [B] uint32   bit j set: joint j is hidden in every frame (stored as 0).
 *   window [B, 2] int32     (start, end): frames start <= f < end lose every channel from 22 on (stored as 0).
 *   vis_bits [n_vis, vis_rows] uint32 with vis_index [B] int64: bit j of row f of clip vis_index[b] set: joint j is visible
 *                           at frame f; the value is MULTIPLIED by the 0 / 1 mask, as the PROX branch does (:157).  Rows
 *                           0 .. T-1 of a clip are used (vis_rows >= T).  vis_index_host, when not NULL, is a HOST copy of
 *                           vis_index that is range-checked before the launch; on the device an index outside [0, n_vis)
 *                           reads nothing and gives NaN rows.
 * zero_contact != 0 stores 0 in the four contact channels.  Channels in REPR_LIST order: 0..21 trajectory, never masked;
 * 22..87 local positions, joint (c-22)/3; 88..153 local velocities, joint (c-88)/3; 154..279 body pose 6d, joint
 * 1 + (c-154)/6; 280..289 betas, never masked by joints; 290, 291 left and 292, 293 right foot contact: hidden with
 * joint_bits when bit 7 or 10 (left) / 8 or 11 (right) is set, visible with vis_bits only when joints 7 and 10 (left) / 8 and
 * 11 (right) are both visible.  The multiplication comes first, then the stores of 0.  The outputs must not alias the inputs.
 * Errors before any launch (ROHM_ERR_ARG): B < 0, T outside [1, 512], vis_rows < T, a vis_index_host entry outside [0, n_vis).
 *
 * rohm_train_traj_window: training_loop_trajnet.py:72-82 in place on cond [B, T, C]: the first n_ch channels of frames
 * window[b][0] <= t < window[b][1] (window [B, 2] int32) are multiplied by 0, everything else by 1 (left as it is). */
int rohm_train_cond(const float* src, const float* clean, int B, int T, const unsigned* joint_bits, const int* window,
                    const unsigned* vis_bits, int n_vis, int vis_rows, const long long* vis_index,
                    const long long* vis_index_host, int zero_contact, float* cond, float* clean_t, rohm_stream_t stream);
int rohm_train_traj_window(float* cond, int B, int T, int C, int n_ch, const int* window, rohm_stream_t stream);

/* The optimiser step of the training loops (csrc/optim.hip): train/training_loop_posenet.py:52-54,278 and
 * train/training_loop_trajnet.py hold a torch.optim.AdamW and call its step(); the reference has no gradient clipping.
 * The tables (params, grads, exp_avg, exp_avg_sq, numel) are HOST arrays of n_tensors entries whose pointer entries are DEVICE
 * pointers to contiguous fp32 (4-byte aligned; they need not be 16-byte aligned: a parameter may be a view into a larger
 * buffer).  The library copies the entries into the kernel arguments before it returns, so the caller may rewrite or free the
 * arrays at once, and gradient pointers may differ from step to step.  Tensors of 0 elements are skipped.  The caller's stream,
 * never synchronised, nothing allocated, no atomics.
 *
 * rohm_adamw_step: one AdamW update of every listed tensor with the same hyper-parameters and the same step count `step` (>= 1,
 * the count AFTER this step, as torch's state['step']): torch.optim.AdamW with decoupled weight decay and without amsgrad,
 * in the operation order of torch/optim/adam.py _single_tensor_adam (non-capturable branch).  The scalars are derived in double
 * and converted to float once: decay = 1 - lr weight_decay, w1 = 1 - beta1, w2 = 1 - beta2, bc2_sqrt = sqrt(1 - beta2^step),
 * step_size = lr / (1 - beta1^step).  Per element in fp32:
 *     p *= decay                       (skipped when weight_decay == 0)
 *     g' = g * *clip_coef              (skipped when clip_coef is NULL)
 *     m += w1 (g' - m);   v = v beta2 + w2 g' g';   p -= step_size m / (sqrt(v) / bc2_sqrt + eps)
 * clip_coef, when not NULL, is a device pointer to one float, typically out + 1 of rohm_grad_norm on the same stream.  The
 * gradients themselves are only read: unlike torch.nn.utils.clip_grad_norm_, clipping does NOT rescale the stored gradients.
 * beta1 must exceed 0.5 (torch's lerp takes another form below that).  Launches: one per rohm_adamw_limits' tensors_per_launch
 * tensors; a tensor is cut into blocks of elems_per_block elements.
 *
 * rohm_grad_norm: out[0] = the L2 norm over all listed gradients, out[1] = min(1, max_norm / (out[0] + 1e-6)), the coefficient
 * of torch.nn.utils.clip_grad_norm_ (error_if_nonfinite=False: a NaN norm gives a NaN coefficient, an infinite norm 0; nothing
 * is raised).  out: device, 2 floats, 8-byte aligned.  Squares are summed in double, per block into `scratch`
 * (rohm_grad_norm_scratch_bytes for the total element count and the tensor count; 8-byte aligned), then by one finishing
 * block in slot order: the same inputs give the same bits on every call.  ROHM_ERR_WORKSPACE when scratch is too small. */
int rohm_adamw_limits(int* tensors_per_launch, int* elems_per_block);
int rohm_adamw_step(float* const* params, const float* const* grads, float* const* exp_avg, float* const* exp_avg_sq,
                    const long long* numel, int n_tensors, double lr, double beta1, double beta2, double eps,
                    double weight_decay, long long step, const float* clip_coef, rohm_stream_t stream);
size_t rohm_grad_norm_scratch_bytes(long long total_elems, int n_tensors);
int rohm_grad_norm(const float* const* grads, const long long* numel, int n_tensors, float max_norm, float* out,
                   void* scratch, size_t scratch_bytes, rohm_stream_t stream);

/* The result tails of the test drivers (csrc/results.hip).
 *
 * rohm_result_rows de-normalises up to ROHM_RESULT_ROWS_MAX representations in one launch (test_amass_full.py:387-396 and
 * the same lines of the other drivers): out[b, t, c] = src[b stride_b + t stride_t + c stride_c] * std[c] + mean[c] for
 * b < B, t < T, c < C, as a rounded float32 product followed by a rounded float32 sum (numpy's two operations: the result
 * equals the scripts' bit for bit).  Strides are in elements; either the frames (stride_t == 1: the samplers'
 * [B, C, 1, T] output) or the channels (stride_c == 1: the first T rows of a [B, T', C] tensor) must be contiguous.
 * traj, when not NULL, is a contiguous [B, traj_rows, 22] tensor (traj_rows >= T, C >= 22) whose rows replace channels
 * 0..21 BEFORE de-normalisation (`motion_repr_noisy[:, :, 0:22] = traj_noisy_full[:, 0:-1, :]`, test_amass_full.py:391).
 * out is contiguous [B, T, C] and must not overlap a source.  `items` is read on the host during the call.  Errors before
 * any launch (ROHM_ERR_ARG): a null pointer, n_items outside [1, ROHM_RESULT_ROWS_MAX], traj_rows < T, neither axis
 * contiguous, B * n_items > 65535.
 *
 * rohm_traj_report: the report of test_trajnet.py:221-263, :333-366 as per-clip sums, one wave per clip, no atomics (lanes
 * stride over frames, accumulate in double, one butterfly reduction: the same bits on every call).  The five joint tensors
 * are contiguous [B, T, 22, 3]; only joint 0 (the pelvis) is read.  rot_clean / rot_rec point at channel 0 of the
 * de-normalised clean / reconstructed representation of clip 0, frame (b, t) at [(b T + t) stride].  out [B, 15] doubles:
 *   0        sum_t |2 rot_rec - 2 rot_clean|                                                          (of T)
 *   1 + 3r+x sum_t |pelvis_r[t, x] - pelvis_clean[t, x]|, r = 0 from_abs_traj, 1 from_rel_traj, 2 from_smpl   (of T)
 *   10 + k   sum_t ||(p[t+3] - 3 p[t+2] + 3 p[t+1] - p[t]) * 30^3||, k = clean, noisy, from_abs_traj, from_rel_traj, from_smpl
 *            (of T - 3), every operation a rounded float32 one in numpy's order, the square root correctly rounded
 * elems, when not NULL, receives the float32 terms of these sums as [B, 15, T] (rows 10..14: frames >= T - 3 are 0).
 * T < 4 is ROHM_ERR_ARG. */
#define ROHM_RESULT_ROWS_MAX 3
typedef struct {
    const float* src;
    long long stride_b, stride_t, stride_c;
    const float* mean;
    const float* std;
    const float* traj;
    long long traj_rows;
    float* out;
} rohm_result_rows_item;
int rohm_result_rows(const rohm_result_rows_item* items, int n_items, int B, int T, int C, rohm_stream_t stream);
int rohm_traj_report(const float* joints_clean, const float* joints_noisy, const float* joints_from_abs_traj,
                     const float* joints_from_rel_traj, const float* joints_from_smpl, const float* rot_clean,
                     long long rot_clean_stride, const float* rot_rec, long long rot_rec_stride, int B, int T,
                     double* out, float* elems, rohm_stream_t stream);

/* Export of a reconstruction (csrc/export.hip): rows of the 294-channel representation -> per-frame SMPL-X parameters in
 * scene or camera coordinates, one launch for all N frames of a recording.  The inverse of rohm_smplx_frames_to_world +
 * rohm_clips_build; what eval_prox_egobody.py:275-310 does per clip on the host (recover_from_repr_smpl 'smplx_params',
 * inv(trans_scene2cano)), applied to the parameters as update_globalRT_for_smplx with delta_T given
 * (utils/other_utils.py:221-240).
 * repr is addressed as in rohm_repr_joints: element (c, t, ch) at repr[c*in_stride_b + t*in_stride_t + ch*in_stride_c],
 * c < C, t < T, ch < 294; mean294 / std294 (both or neither) de-normalise in float32 as x * std + mean, two rounded
 * operations.  transf [C,4,4] float32 (scene -> canonical; NULL = identity) is inverted in float64 as a general affine map;
 * rigid [4,4] float64 (NULL = identity) is applied after that inverse: A = rigid . inv(transf[c]).  Output frame n is
 * taken from clip frame_clip[n], row frame_t[n] (device int32 [N]); an index outside [0, C) x [0, T) yields a NaN row,
 * never a read outside the arrays.  Per frame, float64 after the de-normalisation: R = Gram-Schmidt of smplx_rot_6d
 * (quaternion.py:482-501) and of the 21 body joints; d = rest-pose pelvis of the frame's betas (folded regressor of h);
 * R' = A_R R, t' = A_R (t + d) + A_t - d; rotation vectors through the quaternion with an atan2 angle (|aa| <= pi).
 * params [N,79] float64 = global_orient 3, transl 3, betas 10, body_pose 63 (the smplx_world layout rohm_clips_build
 * reads); contact [N,4] float32 (may be NULL) = the foot-contact channels.  No atomics: the same input gives the same
 * bits.  N == 0 returns without a launch. */
int rohm_export_smplx(const rohm_smplx_t* h, const float* repr, long long in_stride_b, long long in_stride_t,
                      long long in_stride_c, const float* mean294, const float* std294, const float* transf,
                      const double* rigid, const int* frame_clip, const int* frame_t, int C, int T, int N,
                      double* params, float* contact, rohm_stream_t stream);

/* rohm_export_smplx with a cross-fade over the frames two clips share (csrc/export.hip), one launch for all N frames.
 * Every clip is denoised on its own, so at a window boundary the plain gather jumps in position, heading and pose; here
 * output frame n has candidate a = (frame_clip[n], frame_t[n]) and, where frame_clip_b[n] >= 0, candidate b =
 * (frame_clip_b[n], frame_t_b[n]) (device int32 [N]) with the weight alpha[n] of b (device float64 [N];
 * rohm_amd.export.plan_blend makes the five arrays: a linear ramp strictly inside (0, 1) over the shared frames).  repr,
 * strides, mean294 / std294, transf, rigid, C, T as in rohm_export_smplx.  Both candidates go through exactly the arithmetic
 * of rohm_export_smplx (its device functions), each with its own clip's transf and its own betas' pelvis offset.
 * One candidate (frame_clip_b[n] < 0), or alpha[n] == 0: the row is candidate a's bits, what rohm_export_smplx writes for
 * (frame_clip[n], frame_t[n]).  Otherwise, in float64: the 22 rotations are the shortest-arc quaternion slerp of the two
 * candidates' final rotation vectors by the rule of rohm_track_resample (lerp weights when sin(omega) < 1e-8, |rotation
 * vector| <= pi through the atan2 angle); transl, betas and the four contact channels are a + alpha (b - a), contact
 * rounded to float32 once.
 * params [N,79] float64 (the smplx_world layout); contact [N,4] float32 (may be NULL); disagree [N,23] float64 (may be
 * NULL): what the two candidates disagreed by -- columns 0..21 the geodesic angle (rad) between their rotations per joint,
 * column 22 the distance (m) between their pelvis positions transl + d(betas) -- whatever alpha is, and zero where there
 * is one candidate.  An index pair outside [0, C) x [0, T) on the a side, or on the b side when frame_clip_b[n] >= 0, gives
 * a NaN row in all three outputs, never a read outside the arrays.  Every output element is written.  No atomics: the
 * same input gives the same bits.  N == 0 returns without a launch. */
int rohm_export_smplx_blend(const rohm_smplx_t* h, const float* repr, long long in_stride_b, long long in_stride_t,
                            long long in_stride_c, const float* mean294, const float* std294, const float* transf,
                            const double* rigid, const int* frame_clip, const int* frame_t, const int* frame_clip_b,
                            const int* frame_t_b, const double* alpha, int C, int T, int N, double* params, float* contact,
                            double* disagree, rohm_stream_t stream);

/* A track of per-frame SMPL-X estimates at any frame rate, with frames that have no fit, resampled to the times
 * times_dst [n_out] (the 30 fps grid of the networks, or a reconstruction back onto the source's time stamps).  No
 * counterpart in the reference.  All arrays are device memory: times_src [N] float64 seconds, strictly increasing;
 * valid_idx [Nv] int32, the ascending indices of the source frames that have a fit (read back and checked here: one stream
 * synchronisation per call); params [N,79] float64 (global_orient 3, transl 3, betas 10, body_pose 63); keypoints [N,J,3]
 * float32 (x, y, confidence; J = 0 and NULL allowed); mask_joint [N,M] float32 (M = 0 and NULL allowed).
 * For an output time t: i0 = last valid frame with times_src <= t, i1 = first valid frame with times_src >= t; where one
 * side does not exist both are the nearest valid frame and gap = 1; alpha = (t - t0) / (t1 - t0) in float64, 0 when
 * i0 == i1; gap = 1 also when t1 - t0 > max_gap (seconds).  alpha == 0 copies the bits of source row i0.  Otherwise the 22
 * rotations are float64 quaternion slerps (shortest arc, lerp weights when sin(omega) < 1e-8, |rotation vector| <= pi),
 * transl and betas are a + alpha (b - a) -- inside a gap too.  Keypoints outside a gap: confidence min(c0, c1), x / y
 * interpolated in float64 and stored as float32, taken from the other bracket where one confidence is 0; mask min(m0, m1).
 * Inside a gap keypoints and mask are 0.  src_index [n_out] = i0, gap [n_out] uint8.  No atomics: the same input gives
 * the same bits.  n_out == 0 returns without a launch. */
int rohm_track_resample(const double* times_src, const int32_t* valid_idx, const double* params, const float* keypoints,
                        const float* mask_joint, const double* times_dst, double max_gap, int N, int Nv, int J, int M,
                        int n_out, double* params_out, float* keypoints_out, float* mask_out, int32_t* src_index,
                        unsigned char* gap, rohm_stream_t stream);

/* Scores of a stitched track that need no ground truth (csrc/quality.hip; tests/quality_ref.py restates it).  One row per
 * frame of the stitched track, every frame counted once.  All arrays are device memory.  joints [N,22,3] float32 in scene
 * coordinates (ExportResult.joints with frame='scene'); up_axis 2 = z, 1 = y as in rohm_scene_metrics; has_floor /
 * ground_height: the floor's height along up_axis; scene2cam [16] float64, row-major, with the intrinsics fx, fy, cx, cy and
 * keypoints [N,22,3] float32 (u, v, confidence, SMPL order) -- scene2cam and keypoints are both given or both NULL;
 * joints_ref [N,22,3] float32 (the input track in scene coordinates; may be NULL); mask_ref [N,22] float32 (1 = the joint
 * was observed; NULL = all ones); gap [N] uint8 (NULL = all zero).  All arithmetic is float64 on the float32 inputs.
 * rows [N,10] float64, every element written:
 *   0 reproj_px = sum c d / sum c over the joints with c > conf_min and camera depth Z > 0, d the pixel distance between
 *     the keypoint and (fx X / Z + cx, fy Y / Z + cy) of scene2cam . joint; NaN when no joint qualifies or without keypoints
 *   1 reproj_max_px, the largest d over the same joints (NaN likewise)      2 the number of those joints
 *   3 skate of the pair (t, t+1), 1 or 0: all of ankles 7, 8 and toes 10, 11 have horizontal speed > 0.10 m/s and a height
 *     above the floor at t below 0.15 m (ankles) / 0.10 m (toes), the rule of csrc/scene_metrics.hip; NaN at the last frame
 *     and without a floor
 *   4 accel = mean over the 22 joints of |x[t+2] - 2 x[t+1] + x[t]| fps^2; NaN at the last two frames
 *   5 pene = min over the two toes of min(d, 0), d = height - ground_height; NaN without a floor
 *   6 dev_vis = mean |joints - joints_ref| over the joints with mask_ref == 1; NaN when there are none or without joints_ref
 *   7 dev_occ, the same over mask_ref == 0      8 the number of joints with mask_ref == 1      9 gap[t] as 0 / 1
 * A value is NaN exactly when a number it reads is not finite: a joint with c > conf_min whose camera coordinates are not
 * finite makes 0 .. 2 NaN, a foot joint with a NaN speed or height makes 3 NaN, and so on; nothing else changes.
 * totals [2,15] float64: the sums of group g = gap[t] (0 observed, 1 in-filled; a pair or triple belongs to the group of its
 * first frame), NaN per-frame values left out of sums and counts:
 *   0 frames      1 sum reproj_px      2 frames with a reproj_px      3 max reproj_max_px (NaN when 2 is 0)
 *   4 skating pairs      5 pairs scored      6 sum accel      7 frames with an accel
 *   8 toe entries with d < -0.05      9 sum min(d, 0) over toe entries      10 toe entries scored (a NaN d is left out)
 *   11 sum dev_vis      12 frames with dev_vis      13 sum dev_occ      14 frames with dev_occ
 * Two launches: half a wave per frame, then one workgroup that reduces the rows in a fixed order.  No atomics (the same
 * input gives the same bits), no allocation, no synchronisation.  N == 0 returns without a launch. */
int rohm_track_quality(const float* joints, int N, double fps, int up_axis, int has_floor, float ground_height,
                       const double* scene2cam, double fx, double fy, double cx, double cy, const float* keypoints,
                       float conf_min, const float* joints_ref, const float* mask_ref, const unsigned char* gap,
                       double* rows, double* totals, rohm_stream_t stream);

/* How far a mesh track reaches under the floor (csrc/quality.hip): toes alone miss a knee or a hand.  verts [n,V,3]
 * float32 device memory in scene coordinates, up_axis as above.  out [n,3] float64 per frame: the lowest vertex height
 * above the floor (height - ground_height, float64 on the float32 values), the index of that vertex (the lowest index on
 * ties) and the number of vertices with height - ground_height < -below.  A frame with a vertex height that is not finite
 * gets (NaN, -1, NaN).  One workgroup per frame, a fixed-order reduction; no atomics, no allocation, no synchronisation.
 * n == 0 returns without a launch. */
int rohm_floor_clearance(const float* verts, int n, int V, int up_axis, float ground_height, float below, double* out,
                         rohm_stream_t stream);

/* The floor of an uncalibrated camera-frame track (csrc/floor.hip; rohm_amd/floor.py drives the three entry points,
 * tests/floor_ref.py restates them).  No counterpart in the reference.  All arrays are device memory, all arithmetic is
 * float64 on the float32 positions, no atomics (the same input gives the same bits), no allocation.
 *
 * rohm_floor_candidates: which toe positions are at rest.  joints [N,22,3] float32 in the camera frame, times [N] float64
 * seconds (strictly increasing), valid_idx [Nv] int32, the ascending indices of the frames that have a fit, keypoints
 * [N,22,3] float32 (x, y, confidence; may be NULL).  flags [N,2] uint8 for the toes (joints 10 and 11), every element
 * written: flags[i][k] = 1 exactly when frame i is in valid_idx and has a successor i' there with
 * 0 < dt = times[i'] - times[i] <= max_gap, |p[i'] - p[i]| / dt < v_max (p the toe's position) and, with keypoints, the
 * toe's confidence at i > conf_min.  A number that is not finite anywhere in the rule gives 0.  An entry of valid_idx
 * outside [0, N), or one whose successor is not larger, marks nothing and reads nothing.  Two launches, no
 * synchronisation.  N == 0 returns without a launch. */
int rohm_floor_candidates(const float* joints, const double* times, const int32_t* valid_idx, const float* keypoints, int N,
                          int Nv, float conf_min, double v_max, double max_gap, unsigned char* flags, rohm_stream_t stream);

/* rohm_floor_hypotheses: K candidate planes scored in one launch.  points [P,3] float32 (the resting toe positions), joints
 * [NJ,3] float32 (every joint of every valid frame), triples [K,3] int32 indices into points (read back and checked here:
 * one stream synchronisation per call; an index outside [0, P) is refused by name).  For hypothesis h with the points p0,
 * p1, p2 of its triple: n = (p1 - p0) x (p2 - p0); the triple is degenerate unless 1e-9 <= |n| < inf; n /= |n|,
 * d = -n . p0.  pos = #(n . q + d > under_tol) and neg = #(n . q + d < -under_tol) over the joints q; if neg > pos the plane
 * is turned over (n, d -> -n, -d) and the counts change places, a tie keeps it.  under = neg, support =
 * #(|n . p + d| <= tau) over the points, score = support - under.  planes [K,4] float64 (n, d); scores [K,3] int64 (score,
 * support, under); a degenerate triple gets a NaN plane and (INT64_MIN, 0, 0).  best [1] int32: the hypothesis with the
 * largest score, the lowest index on ties, -1 when every triple is degenerate.  A NaN position fails every comparison and
 * so is in no count.  All counts are integers: no reduction order can change a bit.  Two launches (16 hypotheses per
 * workgroup, positions tiled through LDS; then one workgroup for best).  K == 0 returns without a launch; K > 0 needs
 * P >= 3. */
int rohm_floor_hypotheses(const float* points, int P, const float* joints, int NJ, const int32_t* triples, int K, double tau,
                          double under_tol, double* planes, long long* scores, int32_t* best, rohm_stream_t stream);

/* rohm_floor_moments: the sums a least-squares plane through the inliers needs.  points [P,3] float32, plane [4] float64
 * (n, d), origin [3] float64 (any point near the inliers; it keeps the products small).  Over the points with
 * |r| <= tau, r = n . p + d, and q = p - origin: out [11] float64 = count, sum q (x, y, z), sum of the products xx, xy, xz,
 * yy, yz, zz of q, sum r^2.  A NaN position is no inlier.  One workgroup of 1024 threads, a fixed order (as the totals of
 * rohm_track_quality): thread t takes the points t, t + 1024, ..., a xor-butterfly per wave, then the 16 wave partials in
 * wave order.  No workspace, no synchronisation.  P == 0 returns without a launch and leaves out alone. */
int rohm_floor_moments(const float* points, int P, const double* plane, const double* origin, double tau, double* out,
                       rohm_stream_t stream);

/* SMPL-X from 3-D joints (csrc/fit.hip; rohm_amd/fit.py drives the two entry points, tests/fit_ref.py restates them).  No
 * counterpart in the reference.  All arrays are device memory; the inputs are float32 where the project's forward
 * kinematics takes float32, all arithmetic is float64; no atomics (the same input gives the same bits), no allocation, no
 * synchronisation.
 *
 * rohm_fit_pose: one Levenberg-Marquardt problem per frame.  targets [N,22,3] float32 in SMPL joint order, any frame of
 * reference; conf [N,22] float32 or NULL (ones); betas [N,10] float32; init, prev [N,69] float64 or NULL; w_prior [22]
 * float64.  c_j = conf_j, or 0 for a target or confidence that is not finite or a confidence <= 0.  Unknowns x [69]: the
 * axis-angles of joints 0..21, then the translation t.
 *   E(x) = sum_j c_j |p_j + t - y_j|^2 + sum_k w_prior[k] |theta_k|^2 + w_smooth sum_{k=1..21} |theta_k - m_k|^2
 * p_j: rohm_smplx_joints' joints (angle |r + 1e-8|, axis r / angle, rest joints Jt + Js beta, the forward chain) in float64.
 * m_k: the mean of prev's theta_k over those of the frames i - 1, i + 1 that exist and whose whole prev row is finite; with
 * prev NULL or no such neighbour the smoothing term is absent (the root, k = 0, is never smoothed).
 * Jacobian: d p_j / d theta_k = -[p_j - p_k]x G_k J_r(theta_k) for k a strict ancestor of j (G_k the world rotation,
 * J_r = I - (1 - cos a) / a^2 K + (a - sin a) / a^3 K^2 with K = [theta_k]x, a = |theta_k|; below a = 1e-6 the factors are
 * 1/2 - a^2/24 and 1/6 - a^2/120), d / dt = I.  H = J^T C J + diag(w_prior + smoothing), g = J^T C r + w_prior theta +
 * w_smooth (theta - m): half the gradient of E.
 * Start: the init row when init is given and that row is finite.  Else theta = 0 but for the root, R_0 = F(y) F(rest)^T with
 * F(v) = [x^ u^ z^], x^ = norm(v_1 - v_2), u^ = norm of the part of v_12 - (v_1 + v_2) / 2 orthogonal to x^, z^ = x^ x u^,
 * turned into an axis-angle (c = (tr R - 1) / 2, v = (R21 - R12, R02 - R20, R10 - R01), s = |v| / 2, angle = atan2(s, c);
 * v angle / (2 s) when s >= 1e-6 and c > -0.99, v / 2 when c > 0 otherwise, else the axis from the largest diagonal element
 * of (R + R^T) / 2, signed to agree with v), and t = sum c (y - p) / sum c.
 * report [N,6]: status, E at the start, E at the end, accepted iterations, the final lambda, sqrt(sum c |r|^2 / sum c).
 * Status 0: fewer than min_joints joints have c > 0.  Status 2: no usable init row and joint 1, 2 or 12 has c = 0 or a norm
 * of a triad (of the targets or of the rest joints) is below 1e-9.  Both give a zero params row, NaN for report 1, 2, 4, 5,
 * 0 accepted and a zero normal block.  Status 1 otherwise.
 * Iteration: lambda starts at 1e-3.  Each of the `iters` iterations builds H and g and makes up to 8 tries: solve
 * (H + lambda diag(diag(H) + 1e-9)) d = -g by Cholesky (a pivot that is not positive is a rejected try); accept when
 * E(x + d) < E(x), then lambda = max(lambda / 10, 1e-9) and the iteration ends; otherwise lambda = min(10 lambda, 1e8).
 * Eight rejections leave x alone.  iters == 0 evaluates only: params is the start.  normal [N,69,70] (may be NULL) receives
 * H (columns 0..68) and g (column 69) at the start.  params [N,69], report and normal are written wholly.
 * One workgroup of 256 threads per frame, H (packed), the Jacobian and the Cholesky factor in 65 KiB of LDS.  N == 0
 * returns without a launch. */
int rohm_fit_pose(const rohm_smplx_t* h, const float* targets, const float* conf, const float* betas, const double* init,
                  const double* prev, const double* w_prior, double w_smooth, int iters, int min_joints, int N,
                  double* params, double* report, double* normal, rohm_stream_t stream);

/* rohm_fit_shape_moments: with the pose fixed the joints are linear in the shape, p_j + t = a_j + A_j beta: A_0 = Js_0,
 * A_j = A_parent + G_parent (Js_j - Js_parent) (Js [3,10] per joint: the handle's joint shape directions), a_j the same chain
 * on Jt, plus t.  targets, conf as above; params [N,69] float64; use [N] uint8.  per_frame [N,66] float64, every row
 * written (zeros where use == 0): the upper triangle of sum_j c_j A_j^T A_j (55 values, row-major, i <= j), sum_j c_j
 * A_j^T (y_j - a_j) (10 values), sum_j c_j |y_j - a_j|^2.  out [66]: the sum of the rows in a fixed order (one workgroup
 * per value: thread t takes the frames t, t + 256, ..., a xor-butterfly per wave, then the 4 wave partials in wave order).
 * Two launches.  N == 0 returns without a launch and leaves out alone. */
int rohm_fit_shape_moments(const rohm_smplx_t* h, const float* targets, const float* conf, const double* params,
                           const unsigned char* use, int N, double* per_frame, double* out, rohm_stream_t stream);

#ifdef __cplusplus
}
#endif
#endif /* ROHM_HIP_H */
