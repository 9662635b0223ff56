/*
 * gdm.h -- C ABI of libgdm_hip.so: the MI355X (gfx950) kernels under the GAN training hot path of
 * marja-w/gan-des-midi-music-gen (GAN_DES/SIMNN.py, MMGAN_MIDI_DES/network_tests.py).
 *
 * The reference has no native/FFI boundary of its own: everything below its Python classes is
 * PyTorch/ATen.  Each entry point here therefore names the ATen dispatch (and the reference call site) it replaces.
 *
 * Contract (all entry points):
 *   - plain C: device pointers + sizes, no torch types; `stream` is a hipStream_t passed as void*.
 *   - caller owns all memory; nothing is allocated, freed or synchronised here; work is only enqueued on `stream`.
 *   - returns 0 on success, a negative GDM_E* code otherwise; gdm_last_error() gives the thread-local message.
 *   - re-entrant across host threads (autograd runs backward on its own thread); no global mutable state.
 *   - `dtype` arguments: GDM_F32 (exact-fp32 mode, v_mfma_f32_16x16x4_f32) or GDM_BF16 (bf16 storage/MFMA operands,
 *     v_mfma_f32_16x16x32_bf16, fp32 accumulation).  Parameters, gradients of parameters, optimizer state, batch-norm
 *     statistics and losses are always fp32.
 */
#ifndef GDM_H
#define GDM_H
#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

enum { GDM_F32 = 0, GDM_BF16 = 1 };
enum { GDM_ACT_NONE = 0, GDM_ACT_RELU = 1, GDM_ACT_LEAKY = 2, GDM_ACT_SIGMOID = 3 };
enum { GDM_OK = 0, GDM_EINVAL = -1, GDM_ELAUNCH = -2, GDM_EWORKSPACE = -3 };
/* the three criteria of model 2's training loop (network_tests.py:248-250: BCEWithLogitsLoss, MSELoss, L1Loss) */
enum { GDM_CRIT_BCE_LOGITS = 0, GDM_CRIT_MSE = 1, GDM_CRIT_L1 = 2 };

/* ---- probes -------------------------------------------------------------------------------------------------- */
const char* gdm_last_error(void);
int gdm_version(void);          /* 1000*major + minor */
const char* gdm_arch(void);     /* "gfx950" */
int gdm_build_flavor(void);     /* 0 = shipped flags; 1 = built with experiment switches (GDM_HIPCC_FLAGS): not benchable */

/* ---- dense layers (aten::addmm / aten::mm: nn.Linear fwd, dX, dW; ConvTranspose2d as GEMM) ---------------------
 * C[m,n] = act( sum_k A[m,k]*B[k,n] + bias_n[n] + bias_m[m] ), arbitrary element strides (transposes are free).
 * Replaces F.linear at SIMNN.py:140-141, network_tests.py:77,112,139,160 and their autograd mm's.
 * compute_dtype selects the MFMA; operands of the other type are converted while staged into LDS.
 * split_k > 1 partitions K over blockIdx.z into fp32 slabs in `workspace` (>= split_k*M*N*4 bytes) that a second
 * kernel sums in fixed order (deterministic) before bias/activation.                                              */
int gdm_gemm(const void* A, int a_dtype, int64_t sam, int64_t sak,
             const void* B, int b_dtype, int64_t sbk, int64_t sbn,
             void* C, int c_dtype, int64_t scm, int64_t scn,
             int M, int N, int K,
             const float* bias_n, const float* bias_m, int act, float slope,
             int compute_dtype, int split_k, void* workspace, size_t workspace_bytes, void* stream);

/* The path gdm_gemm takes for one operand description, from the same host function gdm_gemm launches from.  Nothing is
 * launched and the GPU is not touched: the pointers count for their alignment only and are never dereferenced.  Fills
 * plan[GDM_GEMM_PLAN_FIELDS]: the kernel (GDM_GEMM_KERNEL_*), whether A and B are read K-major (fast kernels; 0 on the
 * generic path), the effective split_k (clamped so that no slab is empty), the slab width k_per_split, the reduce
 * kernel (GDM_GEMM_REDUCE_*) and the workspace bytes gdm_gemm will ask for.  Argument errors are gdm_gemm's.         */
enum { GDM_GEMM_KERNEL_F32 = 0, GDM_GEMM_KERNEL_BF16 = 1, GDM_GEMM_KERNEL_FAST_K32 = 2, GDM_GEMM_KERNEL_FAST_K64 = 3 };
enum { GDM_GEMM_REDUCE_NONE = 0, GDM_GEMM_REDUCE_VECTOR = 1, GDM_GEMM_REDUCE_SCALAR = 2 };
enum { GDM_GEMM_PLAN_KERNEL = 0, GDM_GEMM_PLAN_A_KMAJOR = 1, GDM_GEMM_PLAN_B_KMAJOR = 2, GDM_GEMM_PLAN_SPLIT_K = 3,
       GDM_GEMM_PLAN_K_PER_SPLIT = 4, GDM_GEMM_PLAN_REDUCE = 5, GDM_GEMM_PLAN_WORKSPACE_BYTES = 6,
       GDM_GEMM_PLAN_FIELDS = 7 };
int gdm_gemm_plan(const void* A, int a_dtype, int64_t sam, int64_t sak,
                  const void* B, int b_dtype, int64_t sbk, int64_t sbn,
                  const void* C, int c_dtype, int64_t scm, int64_t scn,
                  int M, int N, int K, const float* bias_n, int compute_dtype, int split_k, int64_t* plan);

/* ---- loss (aten::binary_cross_entropy_with_logits, mean) --------------------------------------------------------
 * x: n fp32 values fed to BCEWithLogitsLoss (for model 1 these are already sigmoid outputs: SIMNN.py:141 + 289),
 * target: one label value for the whole batch (0.9/0.1/1.0 at SIMNN.py:284,308,326; 1/0 at network_tests.py:286-287).
 * Writes loss[0] (mean) and, if dx != NULL, dx[i] = grad_scale * (sigmoid(x[i]) - target) / n.
 * If fuse_sigmoid_backward the chain through model 1's final sigmoid is fused: x[i] is sigmoid(z[i]) and dx[i] is
 * d loss / d z[i].  accumulate_loss adds the mean to loss[0] instead of overwriting it (disc_loss = fake + real,
 * SIMNN.py:314).  n <= 65536 (one workgroup, fixed-order reduction => deterministic).                              */
int gdm_bce_with_logits(const float* x, float target, int n, float grad_scale, float* loss, float* dx,
                        int fuse_sigmoid_backward, int accumulate_loss, void* stream);

/* The criterion of model 2's loop as a choice (network_tests.py:248-250, applied at 304-305 and 313; aten::mse_loss /
 * aten::l1_loss, mean): the contract of gdm_bce_with_logits without the sigmoid-fusion flag.  On n logits x and one
 * label y:  GDM_CRIT_MSE  loss = mean((x-y)^2), dx[i] = grad_scale * 2 (x[i]-y) / n;
 *           GDM_CRIT_L1   loss = mean(|x-y|),   dx[i] = grad_scale * sign(x[i]-y) / n, sign(0) = 0 as torch;
 *           GDM_CRIT_BCE_LOGITS  bit-identical to gdm_bce_with_logits(..., fuse_sigmoid_backward = 0, ...).
 * One workgroup, fixed-order reduction, n <= 65536; an unknown criterion is GDM_EINVAL.                             */
int gdm_criterion_loss(const float* x, float target, int n, int criterion, float grad_scale, float* loss, float* dx,
                       int accumulate_loss, void* stream);

/* ---- optimizer (torch.optim.Adam single-tensor step, SIMNN.py:258-259,316; network_tests.py:253-254,308) -------
 * One flat fp32 range: p, g, m (exp_avg), v (exp_avg_sq) of n elements; `step` is the 1-based step count.
 * bias corrections are computed on the host in double like torch does.  grad_scale multiplies g on the fly
 * (1/world_size after a summed gradient all-reduce; 1 otherwise).                                                  */
int gdm_adam_step(float* p, const float* g, float* m, float* v, int64_t n, int step, float lr, float beta1,
                  float beta2, float eps, float grad_scale, void* stream);

/* the same update with the step counter and hyper-parameters resident on the device, so that a captured hipGraph can
 * be replayed: hyper = 8 floats {step (int32 bits), lr, beta1, beta2, eps, grad_scale, -, -}; every call increments
 * the step and recomputes the bias corrections on the device (in double), then updates the flat range.             */
int gdm_adam_step_dev(float* p, const float* g, float* m, float* v, int64_t n, float* hyper, void* stream);
/* The same update for ONE parameter viewed as (N, C, P) whose gradient g_pc is laid out (N, P, C) -- model 1's
 * fc1.weight (128, 32, H2*W2): its weight-gradient GEMM produces the channels-last flatten order -- and whose updated
 * value is also written to shadow_pc (N, P, C) in shadow_dtype, the operand copy the forward / dX GEMMs read.  p, m, v
 * keep the reference's (N, C, P) order.  Replaces two gdm_permute_pc passes around the optimizer.  advance_step: 1 =
 * increment the step and recompute the bias corrections first (like gdm_adam_step_dev); 0 = use the record as it is
 * (a second range of the same optimizer step).                                                                      */
int gdm_adam_step_dev_pc(float* p, const float* g_pc, float* m, float* v, int N, int C, int P, void* shadow_pc,
                         int shadow_dtype, float* hyper, int advance_step, void* stream);

/* ---- batch norm, training mode, rows x channels matrices (aten::native_batch_norm + activation) ----------------
 * y: (rows, channels) fp32 pre-norm values (row-major).  Computes per-channel batch mean / biased variance with a
 * fixed-order Welford merge, updates running_mean/var (momentum, unbiased var) and num_batches_tracked, and writes
 * out = act(gamma*(y-mean)*invstd + beta) in `out_dtype`.  save_mean/save_invstd (channels) are kept for backward.
 * Covers BatchNorm1d+Sigmoid (network_tests.py:78-79,113-114; rows=B) and BatchNorm2d+ReLU on channels-last
 * activations (SIMNN.py:105-108; rows=B*H*W).  workspace >= gdm_bn_workspace_bytes(rows, channels).
 * training=0 normalises with the running statistics instead and leaves them untouched.                            */
size_t gdm_bn_workspace_bytes(int rows, int channels);
int gdm_bn_act_fwd(const float* y, int rows, int channels, const float* gamma, const float* beta,
                   float* running_mean, float* running_var, int64_t* num_batches_tracked, float momentum, float eps,
                   int act, void* out, int out_dtype, float* save_mean, float* save_invstd, int training,
                   void* workspace, size_t workspace_bytes, void* stream);
/* dout: gradient w.r.t. `out` (out_dtype); out: the forward's output (used for act'); y: the pre-norm input.
 * Writes dy (rows,channels) fp32 and dgamma/dbeta (channels).                                                     */
int gdm_bn_act_bwd(const void* dout, const void* out, int out_dtype, const float* y, int rows, int channels,
                   const float* gamma, const float* save_mean, const float* save_invstd, int act, float* dy,
                   float* dgamma, float* dbeta, void* workspace, size_t workspace_bytes, void* stream);
/* The statistics half of gdm_bn_act_fwd alone (training mode): per-channel batch mean / 1/sqrt(var+eps) into save_*,
 * running statistics and num_batches_tracked updated; the consumer applies the normalisation itself (the fused generator
 * kernels below do it while they load their input).  gdm_bn_finalize merges `chunks` x channels (n, mean, M2) partials
 * laid out [chunk][channel][3] -- what gdm_simnn_gen_convt_bn leaves -- in chunk order.                              */
int gdm_bn_stats(const float* y, int rows, int channels, float* running_mean, float* running_var,
                 int64_t* num_batches_tracked, float momentum, float eps, float* save_mean, float* save_invstd,
                 void* workspace, size_t workspace_bytes, void* stream);
/* Batch statistics that span several calls (data-parallel ranks, SURVEY.md 8e "exact mode"): gdm_bn_partials writes the
 * per-row-chunk Welford triples (n, mean, M2) of y (rows, channels) into partials (gdm_bn_partial_chunks(rows) x channels
 * x 3 floats); the partials of all ranks, concatenated along the chunk axis (all-gather), go through gdm_bn_finalize with
 * the GLOBAL row count; gdm_bn_apply = act((y - mean) * invstd * gamma + beta). */
int gdm_bn_partial_chunks(int rows);
int gdm_bn_partials(const float* y, int rows, int channels, float* partials, void* stream);
int gdm_bn_apply(const float* y, int rows, int channels, const float* gamma, const float* beta, const float* mean,
                 const float* invstd, int act, void* out, int out_dtype, void* stream);
int gdm_bn_finalize(const float* ws, int chunks, int rows, int channels, float momentum, float eps, float* running_mean,
                    float* running_var, int64_t* num_batches_tracked, float* save_mean, float* save_invstd, void* stream);

/* ---- model 1 generator, layers 2..4 fused (GAN_DES/SIMNN.py:105-110; forward only, training-mode BatchNorm, the
 * reference's default geometry: 128 -> 64 -> 32 -> 1 channels, 4x4 -> 8x8 -> 16x16 -> 20x20).  Activations are
 * channels-last fp32 row matrices (B*H*W, C) holding the PRE-normalisation convolution outputs.
 * gdm_simnn_gen_pack: conv1.weight (noise_dim,128,4,4), conv2.weight (128,64,4,4), conv3.weight (64,32,4,4) -> bf16
 *   GEMM images (conv1: [pos*128+co][k], conv2/3: parity classes).
 * gdm_simnn_gen_first: ConvTranspose2d(noise_dim -> 128, k4) on the 1x1 noise = a GEMM, y1 (B*16, 128), plus the exact
 *   training-mode BatchNorm statistics of its 128 channels (save_mean / save_invstd, running statistics,
 *   num_batches_tracked) in the same launch: a workgroup owns 16 channels for the whole batch (2 <= B <= 256).
 * gdm_simnn_gen_convt_bn(layer 2|3): BatchNorm(mean, invstd, gamma, beta) + ReLU applied to yin while it is staged,
 *   ConvTranspose2d(k4,s2,p1) as four 2x2-tap implicit GEMMs on bf16 MFMA -> yout, plus one (n, mean, M2) partial per
 *   workgroup and output channel in ws_partials (gdm_simnn_gen_convt_chunks(layer, B) x Cout x 3 floats) for
 *   gdm_bn_finalize.
 * gdm_simnn_gen_last: BatchNorm + ReLU on load, ConvTranspose2d(32 -> 1, k5, s1, p0), sigmoid -> out (B, 20*20).     */
size_t gdm_simnn_gen_pack_bytes(void);
int gdm_simnn_gen_pack(const float* w1, int noise_dim, const float* w2, const float* w3, void* pack, void* stream);
int gdm_simnn_gen_first(const float* noise, int B, int noise_dim, const void* pack, float* y1, float momentum, float eps,
                        float* running_mean, float* running_var, int64_t* num_batches_tracked, float* save_mean,
                        float* save_invstd, void* stream);
int gdm_simnn_gen_convt_chunks(int layer, int B);
int gdm_simnn_gen_convt_bn(int layer, const float* yin, const float* mean, const float* invstd, const float* gamma,
                           const float* beta, int B, const void* pack, float* yout, float* ws_partials, void* stream);
int gdm_simnn_gen_last(const float* yin, const float* mean, const float* invstd, const float* gamma, const float* beta,
                       const float* w4, int B, float* out, void* stream);
/* The whole generator in eval mode, one launch (GAN_DES/SIMNN.py:201-216, generate_song: gen.eval(), gen(noise); the
 * ATen chain of SIMNN.py:97-112 with BatchNorm on its running statistics).  Reference geometry, noise (B, noise_dim)
 * fp32 with 1 <= noise_dim <= 128, any B >= 1; `pack` is gdm_simnn_gen_pack's image.  A workgroup carries one sample
 * through all four layers with its activations in LDS; the rounding points are those of the three training-mode calls
 * above (bf16 noise, weights of layers 1..3 and staged operands bf16(max(fma(x - running_mean, invstd * gamma, beta), 0)),
 * fp32 MFMA accumulation, layer 4 and the sigmoid in fp32), invstd = 1 / sqrtf(running_var + eps) computed in the kernel.
 * Running statistics are only read.  A sample's result does not depend on B or on its row.  Optional taps (NULL = off,
 * a kernel variant without them is launched when all four are NULL): the raw pre-BatchNorm accumulators tap_y1
 * (B*16, 128), tap_y2 (B*64, 64), tap_y3 (B*256, 32), channels-last fp32, and tap_invstd (128 + 64 + 32 floats).
 * pack, out and the y taps are 16-byte aligned.                                                                      */
int gdm_simnn_gen_eval(const float* noise, int B, int noise_dim, const void* pack, const float* w4,
                       const float* gamma1, const float* beta1, const float* rmean1, const float* rvar1,
                       const float* gamma2, const float* beta2, const float* rmean2, const float* rvar2,
                       const float* gamma3, const float* beta3, const float* rmean3, const float* rvar3,
                       float eps, float* out, float* tap_y1, float* tap_y2, float* tap_y3, float* tap_invstd,
                       void* stream);


/* ---- elementwise helpers ---------------------------------------------------------------------------------------*/
/* out = act(x + bias[col]) and its backward dx = dout * act'(out); (rows, cols) row-major. */
int gdm_bias_act_fwd(const float* x, const float* bias, int rows, int cols, int act, float slope, void* out,
                     int out_dtype, void* stream);
int gdm_act_bwd(const void* dout, const void* out, int dtype, int64_t n, int act, float slope, void* dx, void* stream);
/* column sums of a (rows, cols) matrix: out[c] = sum_r x[r,c] (bias gradients). deterministic two-stage. */
int gdm_colsum(const void* x, int dtype, int rows, int cols, float* out, void* workspace, size_t workspace_bytes,
               void* stream);
int gdm_cast(const void* src, int src_dtype, void* dst, int dst_dtype, int64_t n, void* stream);
/* counter[0] (device int) += number of NaN / +-Inf elements of x (bit test: the library's arithmetic is compiled
 * without NaN semantics).  What torch.autograd.set_detect_anomaly(True) (network_tests.py:211) turns into an exception
 * in the reference is found with this: the host side checks inputs, parameters, losses and gradients when anomaly
 * mode is on, or on request (check_finite()). */
int gdm_nonfinite_count(const void* x, int dtype, int64_t n, int* counter, void* stream);

/* ---- model 1 discriminator, convolution trunk (SIMNN.py:123-125,136-139) ---------------------------------------
 * conv1: Conv2d(1,16,k2,s1,p1)+ReLU+MaxPool2 fused (aten::convolution/relu/max_pool2d_with_indices):
 *   x (B,H,W) fp32 -> p1 (B,H1,W1,16) channels-last `dtype`, code1 = B*H1*4*Q1 uint64 (Q1 = ceil(W1/4); 8 bytes per
 *   pooled pixel, rows padded to whole quads of four pixels), an opaque image of 16-bit fields, one per (pixel, channel
 *   group g of four): nibble k of a field belongs to channel 4g+k, bits [1:0] = argmax position (dy*2+dx, first maximum in
 *   scan order), bit 2 = that channel passes gradient (pooled value > 0); fields are ordered
 *   [image][pooled row][quad = pw/4][g][pw%4], pixels >= W1 of a row's last quad hold 0; H1=(H+1)/2, W1=(W+1)/2.
 *   code1 is only ever read back by gdm_simnn_conv1_bwd_weight / _bwd_data / gdm_simnn_conv2_bwd_fused.
 * conv2: Conv2d(16,32,k3,s1,p1)+ReLU+MaxPool2 fused, implicit GEMM on MFMA:
 *   p1 -> p2 (B,H2,W2,32) channels-last, code2 (B,H2,W2,16) uint8: one byte per channel pair (2j, 2j+1) =
 *   8 * (c_even + 5 * c_odd), c = 0..3 argmax position in scan order, 4 = ReLU-dead; H2=H1/2, W2=W1/2.  The reference flattens channel-major (x.view(-1, 32*32*54), SIMNN.py:139);
 *   the host keeps fc1's weight permuted to the channels-last order instead (gdm_permute_pc), which is the same
 *   linear map.
 * conv2 weights are consumed from a packed image built by gdm_simnn_conv2_pack (forward and flipped-backward MFMA
 * operand layouts, in `dtype`); rebuild it whenever the weights change.                                            */
int gdm_simnn_conv1_fwd(const float* x, const float* w, const float* bias, int B, int H, int W, void* p1,
                        uint64_t* code1, int dtype, void* stream);
/* the same for a batch that is the concatenation of two input tensors, images 0 .. bsplit-1 from x0 and bsplit .. B-1
 * from x1 (the discriminator step's [real ; generated] batch, SIMNN.py:306-310, in one launch, without a torch.cat) */
int gdm_simnn_conv1_fwd_pair(const float* x0, const float* x1, int bsplit, const float* w, const float* bias, int B,
                             int H, int W, void* p1, uint64_t* code1, int dtype, void* stream);
size_t gdm_simnn_conv2_pack_bytes(int dtype);
int gdm_simnn_conv2_pack(const float* w, int dtype, void* pack, void* stream);
int gdm_simnn_conv2_fwd(const void* p1, const void* pack, const float* bias, int B, int H1, int W1, void* p2,
                        uint8_t* code2, int dtype, void* stream);
/* backward of the conv2 block w.r.t. its input: dp2 (B,H2,W2,32) + code2 -> dp1 (B,H1,W1,16).  conv1's ReLU/pool
 * routing is not applied here; gdm_simnn_conv1_bwd_weight applies it through code1. */
int gdm_simnn_conv2_bwd_data(const void* dp2, const uint8_t* code2, const void* pack, int B, int H1, int W1, void* dp1,
                             int dtype, void* stream);
/* the same data gradient with conv1's weight gradient fused into its epilogue: dp1 is routed through code1 and
 * contracted with the input windows while it is still in registers, so it never goes to HBM (dp1_or_null = NULL).
 * Samples [0,bsplit) read their input from x0, samples [bsplit,B) from x1 (the 2B batch [real ; fake]).
 * The kernel leaves one slab of 80 partial sums per workgroup in `workspace`
 * (>= gdm_simnn_conv2_bwd_fused_workspace_bytes(B,H1,W1)); gdm_simnn_conv2_bwd_fused_finish (same B,H1,W1,workspace)
 * adds the slabs in fixed order into dw1 (16,1,2,2), db1 (16).                                                      */
size_t gdm_simnn_conv2_bwd_fused_workspace_bytes(int B, int H1, int W1);
int gdm_simnn_conv2_bwd_fused(const void* dp2, const uint8_t* code2, const void* pack, int B, int H1, int W1,
                              const uint64_t* code1, const float* x0, const float* x1, int bsplit, int H, int W,
                              void* dp1_or_null, int dtype, void* workspace, size_t workspace_bytes, void* stream);
int gdm_simnn_conv2_bwd_fused_finish(int B, int H1, int W1, float* dw1, float* db1, void* workspace,
                                     size_t workspace_bytes, void* stream);
/* dW2 (32,16,3,3), db2 (32): deterministic slab reduction; workspace >= gdm_simnn_conv2_bwd_weight_workspace_bytes */
size_t gdm_simnn_conv2_bwd_weight_workspace_bytes(int B, int H1, int W1);
int gdm_simnn_conv2_bwd_weight(const void* dp2, const uint8_t* code2, const void* p1, int B, int H1, int W1,
                               float* dw, float* db, int dtype, void* workspace, size_t workspace_bytes, void* stream);
/* dW1 (16,1,2,2), db1 (16) from dp1 routed through code1 (pool argmax + ReLU mask) and the input x. */
size_t gdm_simnn_conv1_bwd_weight_workspace_bytes(int B, int H, int W);
int gdm_simnn_conv1_bwd_weight(const void* dp1, const uint64_t* code1, const float* x, int B, int H, int W,
                               float* dw, float* db, int dtype, int accumulate, void* workspace, size_t workspace_bytes,
                               void* stream);
/* dx (B,H,W) fp32 = gradient w.r.t. the discriminator's spectrogram input (aten::convolution_backward's input
 * gradient of SIMNN.py:136 behind the ReLU/pool routing of code1); dp1 (B,H1,W1,16) as written by
 * gdm_simnn_conv2_bwd_fused(dp1_or_null != NULL) or gdm_simnn_conv2_bwd_data; w = conv1.weight (16,1,2,2). */
int gdm_simnn_conv1_bwd_data(const void* dp1, const uint64_t* code1, const float* w, int B, int H, int W, float* dx,
                             int dtype, void* stream);

/* disc_opt.step() of model 1 (SIMNN.py:316) in ONE launch: Adam on fc1.weight with the two layout changes of
 * gdm_adam_step_dev_pc (gradient and operand copy in (N,P,C) order) + Adam on the n_small remaining parameters (one
 * contiguous range p_small / g_small / m_small / v_small that contains conv2.weight) + the rebuild of conv2's packed
 * images (gdm_simnn_conv2_pack) from the updated weights.  hyper: the 8-float device record of gdm_adam_step_dev (its
 * step counter is advanced); done: a device record of GDM_SIMNN_ADAM_RECORD_INTS ints owned by this optimizer (two-level
 * completion counters and the cached bias-correction terms of the next step), zero before the first launch and to be
 * zeroed again whenever the host rewrites `hyper`.  Bit-identical to the sequence gdm_adam_step_dev(small) +
 * gdm_adam_step_dev_pc(big) + gdm_simnn_conv2_pack. */
#define GDM_SIMNN_ADAM_RECORD_INTS 1056
int gdm_simnn_adam_step(float* p_big, const float* g_big_pc, float* m_big, float* v_big, int N, int C, int P,
                        void* shadow_pc, float* p_small, const float* g_small, float* m_small, float* v_small,
                        int n_small, const float* conv2_weight, void* pack, int dtype, float* hyper, int* done,
                        void* stream);

/* head of model 1's discriminator, forward + loss + backward in one launch (SIMNN.py:140-141, 289/311/329):
 * h1 (n,128) fp32 = relu(fc1) -> prob (n) = sigmoid(fc2), loss[0] (+)= sum over the two label halves of the batch
 * means of BCEWithLogits(prob, y) (rows [0,n0) label y0, rows [n0,n) label y1; the sigmoid OUTPUT is fed to the
 * logits loss exactly like the reference does), and if dh1 != NULL the gradients dh1 (n,128) (already through fc1's
 * ReLU), dw2 (128), db2 (1), db1 (128 = column sums of dh1).  Row slices of 32 are reduced per workgroup, slices are
 * summed in order by a second launch.  workspace >= gdm_simnn_head_workspace_bytes(n).                              */
size_t gdm_simnn_head_workspace_bytes(int n);
int gdm_simnn_head(const float* h1, const float* w2, const float* b2, int n, int n0, float y0, float y1, float* prob,
                   float* loss, int accumulate_loss, void* dh1, int dh1_dtype /* GDM_F32 | GDM_BF16: the fc1 GEMMs' operand */,
                   float* dw2, float* db2, float* db1, void* workspace, size_t workspace_bytes, void* stream);

/* ---- model 2 -----------------------------------------------------------------------------------------------------
 * One generator block in one launch: out = act(BatchNorm1d(x W^T + b)) for up to gdm_linear_bn_act_max_rows() rows
 * (network_tests.py:75-80,110-115: aten::addmm + native_batch_norm + sigmoid).  x (M,K), w (N,K) fp32 row-major;
 * bf16 MFMA operands, fp32 accumulation, exact two-pass batch statistics kept inside the workgroup that owns the
 * columns; running statistics / num_batches_tracked updated in training mode.  y_out (M,N) = pre-norm values,
 * optional (backward needs them).
 * groups >= 1: x, y_out, out hold `groups` batches of M rows one after the other (save_mean / save_invstd: groups x N);
 * every batch is normalised with its own statistics and the running statistics take the updates in batch order -- the
 * two forwards a generator makes per training iteration (network_tests.py:294, 312) in one launch.  stat_repeats >= 1
 * applies each running-statistics update that many times (a forward repeated on identical inputs).  act: NONE, RELU or
 * SIGMOID (LEAKY is not offered here: there is no slope argument; GDM_EINVAL).                                       */
typedef struct gdm_linear_bn_job {      /* the arguments of gdm_linear_bn_act_fwd that differ between blocks */
  const float *x, *w, *bias, *gamma, *beta;
  float *running_mean, *running_var;
  int64_t* num_batches_tracked;
  float *y_out, *out, *save_mean, *save_invstd;
  int M, N, K, groups, stat_repeats;
} gdm_linear_bn_job;
int gdm_linear_bn_act_max_rows(void);
/* 1 or 2 independent blocks in ONE launch (the k-th blocks of model 2's two generators, network_tests.py:186-187: the
 * generators have the same depth and do not depend on each other).  Same arithmetic per job as gdm_linear_bn_act_fwd. */
int gdm_linear_bn_act_fwd_multi(const gdm_linear_bn_job* jobs, int n_jobs, float momentum, float eps, int act,
                                int training, void* stream);
/* out_j (M_j, Ka_j + Kb_j) = [a_j | b_j] row by row for up to four jobs in one launch (torch.cat(dim=1) of the
 * generators' inputs, network_tests.py:87, 119: noise next to the conditioning vector).  b_j may be NULL (copy).   */
typedef struct gdm_concat_job {
  const float *a, *b;
  float* out;
  int M, Ka, Kb;
} gdm_concat_job;
int gdm_concat_cols_multi(const gdm_concat_job* jobs, int n_jobs, void* stream);
int gdm_linear_bn_act_fwd(const float* x, const float* w, const float* bias, const float* gamma, const float* beta,
                          float* running_mean, float* running_var, int64_t* num_batches_tracked, float momentum,
                          float eps, int act, int training, int M, int N, int K, float* y_out, float* out,
                          float* save_mean, float* save_invstd, int groups, int stat_repeats, void* stream);
/* DiscriminatorCNN(roll_size=(2,128,T)) forward + BCE-with-logits loss + full backward as one persistent kernel that
 * keeps a whole sample and its activations in LDS (network_tests.py:147-160 and the criterion calls at 304-305, 313;
 * replaces aten::convolution x2, leaky_relu x2, addmm, binary_cross_entropy_with_logits and their backwards).
 * Samples [0,bsplit) are read from xa (bsplit,2,128,T) with label ya; samples [bsplit,B) from the two planes p0, p1
 * (B-bsplit,128,T) (piano_roll, durations: the reference's stack().permute() view, network_tests.py:290) with label
 * yb.  loss[0] (+)= mean_a + mean_b; logits (B).  want_grad: dw1 (16,2,4,4), db1, dw2 (32,16,4,4), db2, dwfc (1,K),
 * dbfc.  Weights come from gdm_dcnn_pack (bf16 MFMA images + permuted fc weight + biases; rebuild after every update).
 * bf16 only; gdm_dcnn_fused_supported(T) tells whether the roll length fits (T = 50: yes).
 * The last 16 of the gdm_dcnn_pack_bytes(T) bytes are padding behind the biases: no kernel reads or writes them.        */
int gdm_dcnn_fused_supported(int T);
size_t gdm_dcnn_pack_bytes(int T);
int gdm_dcnn_pack(const float* w1, const float* b1, const float* w2, const float* b2, const float* wfc,
                  const float* bfc, int T, void* pack, void* stream);
size_t gdm_dcnn_fused_workspace_bytes(int B, int T, int want_grad);
int gdm_dcnn_fused(const float* xa, int bsplit, const float* p0, const float* p1, int B, int T, float ya, float yb,
                   const void* pack, float* logits, float* loss, int accumulate_loss, int want_grad, float* dw1,
                   float* db1, float* dw2, float* db2, float* dwfc, float* dbfc, void* workspace,
                   size_t workspace_bytes, void* stream);
/* The same pass with the optimizer step fused into the gradient's final summation (one rank: nothing to exchange between
 * gradient and update): disc_opt.step() (network_tests.py:308, torch.optim.Adam) is applied by the threads that finish
 * the gradient elements, and the updated weights are written straight into `pack` (in place: the next launch reads
 * them).  param / exp_avg / exp_avg_sq: w1, b1, w2, b2, wfc, bfc; hyper = the 8-float device record of
 * gdm_adam_step_dev (its step counter is advanced); done = one device int, zero before the first launch. */
typedef struct gdm_dcnn_adam {
  float* param[6];
  float* exp_avg[6];
  float* exp_avg_sq[6];
  float* hyper;
  int* done;
} gdm_dcnn_adam;
int gdm_dcnn_fused_adam(const float* xa, int bsplit, const float* p0, const float* p1, int B, int T, float ya, float yb,
                        void* pack, float* logits, float* loss, int accumulate_loss, float* dw1, float* db1, float* dw2,
                        float* db2, float* dwfc, float* dbfc, const gdm_dcnn_adam* opt, void* workspace,
                        size_t workspace_bytes, void* stream);
/* Both passes with the criterion of network_tests.py:248-250 as an argument (GDM_CRIT_*; applied to each label half
 * at 304-305 and to the generator step's logits at 313): per half of n logits with label y, MSE is mean((z-y)^2) with
 * dz = 2 (z-y) / n, L1 is mean(|z-y|) with dz = sign(z-y) / n (sign(0) = 0 as torch).  gdm_dcnn_fused and
 * gdm_dcnn_fused_adam are these with GDM_CRIT_BCE_LOGITS; an unknown criterion is GDM_EINVAL.                        */
int gdm_dcnn_fused_crit(const float* xa, int bsplit, const float* p0, const float* p1, int B, int T, float ya, float yb,
                        const void* pack, float* logits, float* loss, int accumulate_loss, int want_grad, float* dw1,
                        float* db1, float* dw2, float* db2, float* dwfc, float* dbfc, int criterion, void* workspace,
                        size_t workspace_bytes, void* stream);
int gdm_dcnn_fused_adam_crit(const float* xa, int bsplit, const float* p0, const float* p1, int B, int T, float ya,
                             float yb, void* pack, float* logits, float* loss, int accumulate_loss, float* dw1,
                             float* db1, float* dw2, float* db2, float* dwfc, float* dbfc, const gdm_dcnn_adam* opt,
                             int criterion, void* workspace, size_t workspace_bytes, void* stream);
/* Both generators in eval mode, one launch for any batch (network_tests.py:58-123: Generator and BeatGenerator, four
 * blocks Linear -> BatchNorm1d -> Sigmoid each; generate_midi, :199-206, calls them after .eval()).  BatchNorm on the
 * running statistics is a per-column affine map, so rows are independent: a workgroup carries 16 rows through layers
 * 1-3 in LDS and computes one slab of layer 4's columns.  A job is one generator; with two jobs the second one's
 * workgroups ride in the same grid.  x = cat(noise (B, z), input (B, in)) is read from the two pointers (:87, :119);
 * input_stride is the second one's row stride in floats, 0 = one vector for every row.  K1 = z + in.
 * Arithmetic per layer as gdm_linear_bn_act_fwd in eval mode: split operands x = xh + xl, W = wh + wl in bf16, three
 * MFMA products, fp32 accumulation and bias, (y - running_mean) * (invstd * gamma) + beta with invstd =
 * 1 / sqrtf(running_var + eps), sigmoid; activations stay fp32 between layers.  A row's bits depend on neither B nor
 * the row's position.  Only `out` (B, N4) and the taps are written: the running statistics and num_batches_tracked
 * are not even passed.
 * gdm_mmgan_gen_eval_supported: 1 <= K1 <= 512, hidden widths (256, 128, 64), 1 <= N4 <= 2^20.
 * gdm_mmgan_gen_eval_pack: w, bias, gamma, beta, running_mean, running_var are HOST arrays of the four layers' device
 * pointers (w[l] (N_l, K_l) fp32 row-major); the pack (16-byte aligned, gdm_mmgan_gen_eval_pack_bytes bytes, 0 for an
 * unsupported geometry) receives hi/lo bf16 weight images in MFMA fragment order, zero-padded, and per column bias,
 * invstd, gamma, beta, running_mean.  It is a copy: rebuild it when a parameter or a buffer changes.
 * Taps (NULL = off; a kernel instance without them is launched when all are NULL): tap_y[l] the fp32 pre-BatchNorm
 * values y_{l+1} (B, N_l) of the four layers, tap_a[l] the activations a_{l+1} of the three hidden ones.            */
typedef struct gdm_mmgan_gen_eval_job {
  const float *noise, *input;
  const void* pack;
  size_t pack_bytes;
  float* out;
  float* tap_y[4];
  float* tap_a[3];
  int B, z, in, input_stride, n4;
} gdm_mmgan_gen_eval_job;
int gdm_mmgan_gen_eval_supported(int k1, int h1, int h2, int h3, int n4);
size_t gdm_mmgan_gen_eval_pack_bytes(int k1, int h1, int h2, int h3, int n4);
int gdm_mmgan_gen_eval_pack(const float* const* w, const float* const* bias, const float* const* gamma,
                            const float* const* beta, const float* const* running_mean, const float* const* running_var,
                            int k1, int h1, int h2, int h3, int n4, float eps, void* pack, size_t pack_bytes,
                            void* stream);
int gdm_mmgan_gen_eval(const gdm_mmgan_gen_eval_job* jobs, int n_jobs, int h1, int h2, int h3, void* stream);

/* ---- deterministic discrete-event simulator core (host code; SIMULATOR/simulation_v3.py:25-74, 426-743) -------------
 * One run of Sim(adj, distributions, queue_list, seeds=[seed], logging_mode='Music').run(number_of_customers) for 'normal'
 * distributions (loc[i], scale[i] per node; what both bridges construct, matrix_sim_process.py:72-74 / 50-54) and
 * probability routing.  adj (dim,dim) row-major float64: diagonal > 0 marks a source, <= 0 a server; queue_cap[i] =
 * queue_list[i].  The per-node generators are numpy legacy RandomStates seeded from RandomState(seed).randint(3, 9999999)
 * like the reference's; routing draws come from the GLOBAL numpy stream, whose state travels in and out through
 * mt_key[624] / mt_pos / has_gauss / cached_gauss (np.random.get_state() / set_state()).  The run ends when the event
 * list is empty, when number_of_customers customers have been generated (stop_reason 1), or after max_events processed
 * events (stop_reason 2; the reference stops on a wall-clock limit instead, simulation_v3.py:496-499; 0 = no cap).
 * out[0..n_out) = the 'Music' log records in order: kind 0 arrival / 1 departure (value = clock), 2 processing (value =
 * service time).  GDM_EWORKSPACE when out_capacity is too small (n_out then holds the count needed). */
typedef struct gdm_des_event {
  double value;
  int64_t event_id;
  int32_t node;
  int32_t kind;
} gdm_des_event;
int gdm_des_run(const double* adj, int dim, const double* loc, const double* scale, const int32_t* queue_cap, int64_t seed,
                int64_t number_of_customers, int64_t max_events, uint32_t* mt_key, int* mt_pos, int* has_gauss,
                double* cached_gauss, gdm_des_event* out, int64_t out_capacity, int64_t* n_out, int* stop_reason);

/* ---- the same simulator for a batch of B specs of one dim (csrc/des_sim.h is the one source of the event logic) -------
 * Sample b is simulated exactly as gdm_des_run simulates it FROM ITS OWN generator state (mt_key (B,624), mt_pos,
 * has_gauss, cached_gauss (B): in and out per sample): nothing is handed from one sample to the next.  All arrays have a
 * leading B: adj (B,dim,dim) -- what gdm_des_routing writes --, loc, scale (B,dim) f64, queue_cap (B,dim) i32, seed,
 * number_of_customers (B) i64.  max_queue_cap = the ring capacity per server (a sample with a larger queue_cap errors).
 * max_events >= 1 caps the processed events; every generator draw counts against a budget of
 * 64 * (max_events + dim + 1) 32-bit words per sample (stop reason 5: a service distribution that never turns positive
 * ends there instead of spinning).  max_records: the sample stops (reason 4) as soon as that many records are written,
 * a prefix of the uncapped log; 0 = no cap (host only).
 * Records come out in the CSR layout gdm_des_log_to_roll / gdm_des_log_to_notes take: value, event_id, node, kind
 * (n_records_cap entries each) and rec_ptr (B + 1); n_records (B) i64, stop_reason (B) i32 = GDM_DES_STOP_*.  A sample
 * that errors (reason 3: bad spec, no destination, a customer routed to a source, a capacity overrun) has an empty log
 * and leaves its neighbours alone.
 * gdm_des_run_batch_host: host arrays, dim <= GDM_DES_BATCH_HOST_MAX_DIM; math 0 = libm's log / sqrt (numpy's bits, as gdm_des_run), 1 = the portable
 *   log / sqrt of des_sim.h.  GDM_EWORKSPACE when n_records_cap is too small (rec_ptr[B] then holds the count needed).
 * gdm_des_run_batch: device arrays, always portable math: bit-identical to the host entry with math = 1.  One wave per
 *   sample + a one-workgroup pack step.  max_records >= 1 is required and n_records_cap >= B * max_records (the bound
 *   the consumers are given as n_records: nothing is read back in between).  workspace: 16-byte aligned device memory
 *   of gdm_des_batch_workspace_bytes(B, dim, max_queue_cap) bytes (generator states, rings, routing tables; -1 for
 *   arguments out of range).
 * gdm_des_pack: the pack step of gdm_des_run_batch on its own (device arrays): records of sample b at b * max_records,
 *   n_records (B) counts (clamped to 0..max_records) -> rec_ptr (B + 1) and the records closed up in place.
 * gdm_des_math_probe[_host]: log_out[i] = des_log(x[i]), factor_out[i] = sqrt(-2 des_log(x[i]) / x[i]) -- the portable
 *   math of the polar method on its own, device and host form (they must agree bit for bit).                         */
#define GDM_DES_STOP_EMPTY 0
#define GDM_DES_STOP_CUSTOMERS 1
#define GDM_DES_STOP_EVENTS 2
#define GDM_DES_STOP_ERROR 3
#define GDM_DES_STOP_RECORDS 4
#define GDM_DES_STOP_BUDGET 5
#define GDM_DES_BATCH_MAX_DIM 128
#define GDM_DES_BATCH_HOST_MAX_DIM 4096 /* gdm_des_run_batch_host only (gdm_des_run's bound): its tables are on the heap */
#define GDM_DES_BATCH_MAX_QUEUE_CAP 65536
#define GDM_DES_BATCH_MAX_EVENTS ((int64_t)1 << 40)
int gdm_des_run_batch_host(const double* adj, int B, int dim, const double* loc, const double* scale,
                           const int32_t* queue_cap, const int64_t* seed, const int64_t* number_of_customers,
                           int max_queue_cap, int math, int64_t max_events, int64_t max_records, uint32_t* mt_key,
                           int32_t* mt_pos, int32_t* has_gauss, double* cached_gauss, double* value, int64_t* event_id,
                           int32_t* node, int32_t* kind, int64_t n_records_cap, int64_t* rec_ptr, int64_t* n_records,
                           int32_t* stop_reason);
int64_t gdm_des_batch_workspace_bytes(int B, int dim, int max_queue_cap);
int gdm_des_run_batch(const double* adj, int B, int dim, const double* loc, const double* scale,
                      const int32_t* queue_cap, const int64_t* seed, const int64_t* number_of_customers,
                      int max_queue_cap, int64_t max_events, int64_t max_records, uint32_t* mt_key, int32_t* mt_pos,
                      int32_t* has_gauss, double* cached_gauss, double* value, int64_t* event_id, int32_t* node,
                      int32_t* kind, int64_t n_records_cap, int64_t* rec_ptr, int64_t* n_records, int32_t* stop_reason,
                      void* workspace, size_t workspace_bytes, void* stream);
int gdm_des_pack(int B, int64_t max_records, const int64_t* n_records, int64_t* rec_ptr, double* value,
                 int64_t* event_id, int32_t* node, int32_t* kind, void* stream);
int gdm_des_math_probe_host(const double* x, int64_t n, double* log_out, double* factor_out);
int gdm_des_math_probe(const double* x, int64_t n, double* log_out, double* factor_out, void* stream);

/* ---- the batched simulator WITHOUT a log: per-node queueing statistics (csrc/des_stats.hip, csrc/des_sim.h) ----------
 * The same event chain as gdm_des_run_batch[_host] -- same inputs, same generator states in and out, same stop reasons
 * (never GDM_DES_STOP_RECORDS: there is no record cap) -- that writes no records and returns the accumulators the
 * reference's Server / Source objects carry after Sim.run (SIMULATOR/simulation_v3.py:207-217, 280-281), the inputs of
 * Sim.calculate_metrics (752-824).  (B, dim) arrays, a server's entries zero on a source row and the other way round:
 *   served          i64  total_customers_served, ScheduleDeparture :596
 *   time_in_service f64  total_time_in_service, += service in event order, :606
 *   reneges         i64  the else branch of ProcessArrival, :564
 *   max_queue       i32  max_queue_length, the queue size after an enqueue, :560-561
 *   time_in_queue   f64  total_time_in_queue, += Clock - arrival_time at the dequeue in event order, :641 (:558)
 *   arrival_time    f64  Source.arrival_times, Initialization :526 and ProcessArrival :578
 *   generated       i64  Source.customers_generated, :530 and :579
 *   queue_area      f64  sum over k of k * queue_length_times[k] (:768 before the division by Clock)
 * and optionally queue_time (B, dim, max_queue_cap + 1) f64 = queue_length_times as a dense array (NULL: skipped).
 * The reference adds evt.time - previous_time to queue_length_times[queue.size()] of EVERY server on every popped
 * event (:472-484); here a server's share is added when its queue length changes and once at the end, so queue_area
 * and queue_time are the same sums rounded differently; the other arrays are accumulated in the reference's order.
 * (B) arrays: clock f64 = the reference's Clock and end_time f64 = its previous_time -- the event that triggers the
 * number_of_customers stop is popped and counted in the time integration (:472-484 run before the break at :486) but
 * Clock is not advanced to it; the final flush goes to end_time --; total_customers, events (processed), n_records
 * (the records the logging entries would have written, uncapped) i64; stop_reason i32.
 * A sample that stops with GDM_DES_STOP_ERROR returns zeros in every statistic and keeps the generator state it came
 * with.
 * gdm_des_stats_batch_host: host arrays, dim <= GDM_DES_BATCH_HOST_MAX_DIM, math 0 = libm, 1 = portable.
 * gdm_des_stats_batch: device arrays, portable math, bit-identical to the host entry with math = 1; one wave per
 *   sample, accumulators in LDS, one launch.  dim <= GDM_DES_BATCH_MAX_DIM; arrays aligned to their element size;
 *   workspace: 16-byte aligned device memory of gdm_des_stats_workspace_bytes(B, dim, max_queue_cap) bytes (the layout
 *   of gdm_des_batch_workspace_bytes plus the ring of arrival times; -1 for arguments out of range).  Everything is
 *   validated on the host before the launch (GDM_EINVAL, no launch).                                                 */
int gdm_des_stats_batch_host(const double* adj, int B, int dim, const double* loc, const double* scale,
                             const int32_t* queue_cap, const int64_t* seed, const int64_t* number_of_customers,
                             int max_queue_cap, int math, int64_t max_events, uint32_t* mt_key, int32_t* mt_pos,
                             int32_t* has_gauss, double* cached_gauss, int64_t* served, int64_t* reneges,
                             int64_t* generated, int32_t* max_queue, double* time_in_service, double* time_in_queue,
                             double* queue_area, double* arrival_time, double* clock, double* end_time,
                             int64_t* total_customers, int64_t* events, int64_t* n_records, int32_t* stop_reason,
                             double* queue_time);
int64_t gdm_des_stats_workspace_bytes(int B, int dim, int max_queue_cap);
int gdm_des_stats_batch(const double* adj, int B, int dim, const double* loc, const double* scale,
                        const int32_t* queue_cap, const int64_t* seed, const int64_t* number_of_customers,
                        int max_queue_cap, int64_t max_events, uint32_t* mt_key, int32_t* mt_pos, int32_t* has_gauss,
                        double* cached_gauss, int64_t* served, int64_t* reneges, int64_t* generated,
                        int32_t* max_queue, double* time_in_service, double* time_in_queue, double* queue_area,
                        double* arrival_time, double* clock, double* end_time, int64_t* total_customers,
                        int64_t* events, int64_t* n_records, int32_t* stop_reason, double* queue_time, void* workspace,
                        size_t workspace_bytes, void* stream);

/* ---- the same statistics with a distribution KIND per node (csrc/des_stats.hip: des_stats_dist_kernel; des::AnyDist in
 * csrc/des_sim.h) ------------------------------------------------------------------------------------------------------
 * The argument lists of gdm_des_stats_batch[_host] with `kind` (B, dim) i32 after `scale`; same outputs, stop reasons,
 * generator-state contract and workspace (gdm_des_stats_workspace_bytes).  A node draws its service / inter-arrival
 * time from its own legacy stream as the reference's Server / Source do (SIMULATOR/simulation_v3.py:181-192, 263-274):
 *   GDM_DES_DIST_NORMAL       ['normal', loc, scale]   rng.standard_normal() * scale + loc  (what the entries above do)
 *   GDM_DES_DIST_EXPONENTIAL  ['exponential', scale]   (-log(1.0 - rng.random_sample())) * scale + 0.0; loc is not read
 *   GDM_DES_DIST_UNIFORM      ['uniform', loc, scale]  rng.random_sample() * scale + loc
 * -- scipy's rvs, operation for operation; scale == 0 returns loc (0.0 for the exponential) and draws nothing.  With
 * every kind 0 the results are the bytes of gdm_des_stats_batch[_host].
 * Refused per sample (GDM_DES_STOP_ERROR, zeros, generator state kept), besides what the entries above refuse: a
 * server that can never draw a positive service time without consuming draws -- an exponential with scale 0, a
 * uniform with scale 0 and loc <= 0 (the reference's `while service <= 0` never ends).  A uniform that draws but whose
 * support is <= 0 ends on the draw budget (GDM_DES_STOP_BUDGET), like a normal far below zero.
 * A kind outside 0..2: the host entry reads its array and refuses the call (GDM_EINVAL, nothing runs); the device
 * entry cannot, there the sample stops with GDM_DES_STOP_ERROR like any refused spec.  Everything else is validated on
 * the host before the launch.  gdm_des_stats_batch_dist_host: math 0 = libm, 1 = portable, the device's bits.        */
#define GDM_DES_DIST_NORMAL 0
#define GDM_DES_DIST_EXPONENTIAL 1
#define GDM_DES_DIST_UNIFORM 2
int gdm_des_stats_batch_dist_host(const double* adj, int B, int dim, const double* loc, const double* scale,
                                  const int32_t* kind, const int32_t* queue_cap, const int64_t* seed,
                                  const int64_t* number_of_customers, int max_queue_cap, int math, int64_t max_events,
                                  uint32_t* mt_key, int32_t* mt_pos, int32_t* has_gauss, double* cached_gauss,
                                  int64_t* served, int64_t* reneges, int64_t* generated, int32_t* max_queue,
                                  double* time_in_service, double* time_in_queue, double* queue_area,
                                  double* arrival_time, double* clock, double* end_time, int64_t* total_customers,
                                  int64_t* events, int64_t* n_records, int32_t* stop_reason, double* queue_time);
int gdm_des_stats_batch_dist(const double* adj, int B, int dim, const double* loc, const double* scale,
                             const int32_t* kind, const int32_t* queue_cap, const int64_t* seed,
                             const int64_t* number_of_customers, int max_queue_cap, int64_t max_events,
                             uint32_t* mt_key, int32_t* mt_pos, int32_t* has_gauss, double* cached_gauss,
                             int64_t* served, int64_t* reneges, int64_t* generated, int32_t* max_queue,
                             double* time_in_service, double* time_in_queue, double* queue_area, double* arrival_time,
                             double* clock, double* end_time, int64_t* total_customers, int64_t* events,
                             int64_t* n_records, int32_t* stop_reason, double* queue_time, void* workspace,
                             size_t workspace_bytes, void* stream);

/* ---- the LOGGING simulator with a distribution KIND per node (csrc/des_batch.hip: des_batch_dist_kernel; des::AnyDist in
 * csrc/des_sim.h) ------------------------------------------------------------------------------------------------------
 * The argument lists of gdm_des_run_batch[_host] with `dist_kind` (B, dim) i32 of GDM_DES_DIST_* between `scale` and
 * `queue_cap`, as the two statistics entries above order them (the records' own `kind` output keeps its place); same
 * records, CSR layout, stop reasons, workspace (gdm_des_batch_workspace_bytes) and pack step.  The draws are those of
 * gdm_des_stats_batch_dist[_host], so the log is the one whose statistics those entries return.
 * A sample that stops with GDM_DES_STOP_ERROR has an empty log and KEEPS the generator state it came with (the rule of
 * the statistics entries; gdm_des_run_batch[_host] write the state back after an error inside the chain).  With every
 * kind 0 and no such sample the results are the bytes of gdm_des_run_batch[_host].
 * Refused per sample, besides what the entries without kinds refuse: an exponential server with scale 0 and a uniform
 * server with scale 0 and loc <= 0, when a customer reaches it.  A kind outside 0..2: the host entry reads its array
 * and refuses the call (GDM_EINVAL, nothing runs); the device entry cannot, there the sample stops with
 * GDM_DES_STOP_ERROR.  gdm_des_run_batch_dist_host: math 0 = libm (the reference's bits), 1 = portable, the device's. */
int gdm_des_run_batch_dist_host(const double* adj, int B, int dim, const double* loc, const double* scale,
                                const int32_t* dist_kind, const int32_t* queue_cap, const int64_t* seed,
                                const int64_t* number_of_customers, int max_queue_cap, int math, int64_t max_events,
                                int64_t max_records, uint32_t* mt_key, int32_t* mt_pos, int32_t* has_gauss,
                                double* cached_gauss, double* value, int64_t* event_id, int32_t* node, int32_t* kind,
                                int64_t n_records_cap, int64_t* rec_ptr, int64_t* n_records, int32_t* stop_reason);
int gdm_des_run_batch_dist(const double* adj, int B, int dim, const double* loc, const double* scale,
                           const int32_t* dist_kind, const int32_t* queue_cap, const int64_t* seed,
                           const int64_t* number_of_customers, int max_queue_cap, int64_t max_events,
                           int64_t max_records, uint32_t* mt_key, int32_t* mt_pos, int32_t* has_gauss,
                           double* cached_gauss, double* value, int64_t* event_id, int32_t* node, int32_t* kind,
                           int64_t n_records_cap, int64_t* rec_ptr, int64_t* n_records, int32_t* stop_reason,
                           void* workspace, size_t workspace_bytes, void* stream);

/* ---- the simulator with the reference's 'queue' and 'branch' NODES (csrc/des_sim.h: des::AnyNode; des_stats_net_kernel,
 * des_batch_net_kernel) ------------------------------------------------------------------------------------------------
 * The argument lists, outputs, stop reasons, generator-state contract, workspaces (gdm_des_stats_workspace_bytes,
 * gdm_des_batch_workspace_bytes) and pack step of the four _dist entries above; `kind` may also be
 *   GDM_DES_DIST_QUEUE   ['queue']   a waiting room in front of several servers (Server.__init__, simulation_v3.py:196):
 *                        service time 0 without a draw; its departure takes no routing draw but the first idle child
 *                        that is a server, and while there is none it is scheduled again at the earliest next departure
 *                        among the children (ProcessDeparture 656-673, schedule_delayed_departure 679-697)
 *   GDM_DES_DIST_BRANCH  ['branch']  a router: service time 0 without a draw, routed like any server
 * loc and scale of such a node are not read.  Each is a server with a FIFO and queue_cap; a queue node's delayed
 * departure counts as a waiting customer in the admission test and in queue_area / queue_time (not in max_queue), and
 * adds its delay to time_in_queue.  Every pop of a delayed departure is a processed event and a 'departure' record.
 * (queue_time has max_queue_cap + 1 columns as ever: queue + delayed departure beyond max_queue_cap, which only tied
 * arrivals at a full queue node can reach, has no column there and still counts in queue_area.)
 * With every kind in 0..2 the results are the bytes of the _dist entries.
 * Refused per sample (GDM_DES_STOP_ERROR), besides what those refuse: a SOURCE of either kind (the reference raises
 * "Distribution not supported"), and a queue node that must wait while none of its children has ever scheduled a
 * departure (every child a source: the delayed time is +inf).  A kind outside 0..4: the host entries refuse the call
 * by message, the device entries stop that sample with GDM_DES_STOP_ERROR.                                           */
#define GDM_DES_DIST_QUEUE 3
#define GDM_DES_DIST_BRANCH 4
int gdm_des_stats_batch_net_host(const double* adj, int B, int dim, const double* loc, const double* scale,
                                 const int32_t* kind, const int32_t* queue_cap, const int64_t* seed,
                                 const int64_t* number_of_customers, int max_queue_cap, int math, int64_t max_events,
                                 uint32_t* mt_key, int32_t* mt_pos, int32_t* has_gauss, double* cached_gauss,
                                 int64_t* served, int64_t* reneges, int64_t* generated, int32_t* max_queue,
                                 double* time_in_service, double* time_in_queue, double* queue_area,
                                 double* arrival_time, double* clock, double* end_time, int64_t* total_customers,
                                 int64_t* events, int64_t* n_records, int32_t* stop_reason, double* queue_time);
int gdm_des_stats_batch_net(const double* adj, int B, int dim, const double* loc, const double* scale,
                            const int32_t* kind, const int32_t* queue_cap, const int64_t* seed,
                            const int64_t* number_of_customers, int max_queue_cap, int64_t max_events,
                            uint32_t* mt_key, int32_t* mt_pos, int32_t* has_gauss, double* cached_gauss,
                            int64_t* served, int64_t* reneges, int64_t* generated, int32_t* max_queue,
                            double* time_in_service, double* time_in_queue, double* queue_area, double* arrival_time,
                            double* clock, double* end_time, int64_t* total_customers, int64_t* events,
                            int64_t* n_records, int32_t* stop_reason, double* queue_time, void* workspace,
                            size_t workspace_bytes, void* stream);
int gdm_des_run_batch_net_host(const double* adj, int B, int dim, const double* loc, const double* scale,
                               const int32_t* node_kind, const int32_t* queue_cap, const int64_t* seed,
                               const int64_t* number_of_customers, int max_queue_cap, int math, int64_t max_events,
                               int64_t max_records, uint32_t* mt_key, int32_t* mt_pos, int32_t* has_gauss,
                               double* cached_gauss, double* value, int64_t* event_id, int32_t* node, int32_t* kind,
                               int64_t n_records_cap, int64_t* rec_ptr, int64_t* n_records, int32_t* stop_reason);
int gdm_des_run_batch_net(const double* adj, int B, int dim, const double* loc, const double* scale,
                          const int32_t* node_kind, const int32_t* queue_cap, const int64_t* seed,
                          const int64_t* number_of_customers, int max_queue_cap, int64_t max_events,
                          int64_t max_records, uint32_t* mt_key, int32_t* mt_pos, int32_t* has_gauss,
                          double* cached_gauss, double* value, int64_t* event_id, int32_t* node, int32_t* kind,
                          int64_t n_records_cap, int64_t* rec_ptr, int64_t* n_records, int32_t* stop_reason,
                          void* workspace, size_t workspace_bytes, void* stream);

/* ---- the statistics at S customer counts of ONE run: snapshots (csrc/des_sim.h: des::SnapStats) -- HOST entry only ------
 * number_of_customers enters a run only in its stop test, so the run of n1 customers is a prefix of the run of n2 > n1
 * under the same seeds.  This entry runs gdm_des_stats_batch_net_host (des::AnyNode, the superset of the node kinds; an
 * all-normal net passes kind = 0 everywhere) ONCE per sample, to the sample's last checkpoint, and writes at every
 * checkpoint what the run of that many customers returns:
 *   snap_customers (B, S) i64, 1 <= S <= GDM_DES_SNAP_MAX, every row strictly ascending with values >= 1; the run's
 *   number_of_customers is the row's last entry (there is no other customers array).
 * Outputs: the arrays of gdm_des_stats_batch_net_host with S between B and the rest -- (B, S, dim), (B, S), snap_stop
 * (B, S) i32 and the optional queue_time (B, S, dim, max_queue_cap + 1) -- and the generator state after the run, (B).
 * INVARIANT: snapshot s of sample b is, field for field and bit for bit, what gdm_des_stats_batch_net_host returns for
 * that sample with number_of_customers = snap_customers[b, s] and the same max_events and math; the generator state is
 * that of the run to the last checkpoint.  A checkpoint's stop test fires at a pop (several at one pop: all at or below
 * the number of sources fire at the first); such a snapshot has GDM_DES_STOP_CUSTOMERS and its time-at-queue-length
 * terms closed up to that pop on a copy, the running sums untouched.  When the run ends for another reason (event list
 * empty, max_events, draw budget) every checkpoint not reached receives the final state and that reason.  A sample
 * that ends in GDM_DES_STOP_ERROR keeps the generator state it came with and returns zeros and reason 3 in every
 * checkpoint it had not reached (the ones before are the shorter runs', which ended well; a spec refused before anything
 * runs has reached none).  A bad snap_customers row refuses the call by message (GDM_EINVAL, nothing runs).
 * There is NO device entry: the one-wave-per-sample kernel over this policy is not part of the library (DESIGN.md
 * section 7, f20).                                                                                                     */
#define GDM_DES_SNAP_MAX 256
int gdm_des_stats_batch_snap_host(const double* adj, int B, int dim, const double* loc, const double* scale,
                                  const int32_t* kind, const int32_t* queue_cap, const int64_t* seed,
                                  const int64_t* snap_customers, int S, int max_queue_cap, int math, int64_t max_events,
                                  uint32_t* mt_key, int32_t* mt_pos, int32_t* has_gauss, double* cached_gauss,
                                  int64_t* served, int64_t* reneges, int64_t* generated, int32_t* max_queue,
                                  double* time_in_service, double* time_in_queue, double* queue_area,
                                  double* arrival_time, double* clock, double* end_time, int64_t* total_customers,
                                  int64_t* events, int64_t* n_records, int32_t* snap_stop, double* queue_time);

/* ---- log -> queue tracks (csrc/des_tracks.hip; the reference's MMGAN_MIDI_DES/simlog_to_vid.ipynb, first cell) --------
 * Per sample b, over the first max_lines records of its log [rec_ptr[b], rec_ptr[b + 1]) ('processing' records count
 * towards max_lines and change nothing): an arrival (kind 0) at node n adds 1 to n's counter, a departure (kind 1)
 * subtracts 1; after each of the two, if the sum of all counters is > 0, a row with the counters of the tracked nodes
 * is appended; row 0 is a row of zeros.  col_of_node (B, dim) i32: the column of a node, -1 = not tracked; S columns.
 * A reneged arrival is never subtracted: the numbers are arrivals minus departures, not queue lengths (the notebook's
 * behaviour, kept).  Unlike the notebook, whose regular expression drops a line whose clock prints in exponent
 * notation, every record counts.
 * status (B) i32: 0, GDM_DES_TRACKS_ENODE (an arrival or departure at a node that is not tracked: the notebook's
 * KeyError) or GDM_DES_TRACKS_EPTR (offsets outside the record arrays); such a sample has ZERO rows.
 * gdm_des_log_tracks_count: device arrays -> n_rows (B) i64 and row_ptr (B + 1) i64, their exclusive scan.
 * gdm_des_log_tracks: device arrays, row_ptr as the count wrote it -> tracks (n_rows_cap >= row_ptr[B] rows, S) i32,
 *   sample b's rows at row_ptr[b]; one workgroup per sample, a kept row written as S consecutive int32.
 * gdm_des_log_tracks_host: both steps on host arrays, the device's oracle; also checks col_of_node (inside -1..S-1, no
 *   column twice).  tracks NULL with n_rows_cap 0 only counts; GDM_EWORKSPACE when n_rows_cap is too small (row_ptr[B]
 *   then holds the count needed).                                                                                     */
#define GDM_DES_TRACKS_ENODE 1
#define GDM_DES_TRACKS_EPTR 2
#define GDM_DES_TRACKS_MAX_DIM 4096
#define GDM_DES_TRACKS_MAX_LINES ((int64_t)1 << 30)
int gdm_des_log_tracks_count(const int32_t* node, const int32_t* kind, const int64_t* rec_ptr, int64_t n_records, int B,
                             int dim, const int32_t* col_of_node, int64_t max_lines, int64_t* n_rows, int64_t* row_ptr,
                             int32_t* status, void* stream);
int gdm_des_log_tracks(const int32_t* node, const int32_t* kind, const int64_t* rec_ptr, int64_t n_records, int B,
                       int dim, const int32_t* col_of_node, int S, int64_t max_lines, const int64_t* row_ptr,
                       int64_t n_rows_cap, int32_t* tracks, void* stream);
int gdm_des_log_tracks_host(const int32_t* node, const int32_t* kind, const int64_t* rec_ptr, int64_t n_records, int B,
                            int dim, const int32_t* col_of_node, int S, int64_t max_lines, int64_t* n_rows,
                            int64_t* row_ptr, int32_t* status, int32_t* tracks, int64_t n_rows_cap);

/* ---- log -> per-visit and per-customer tables (csrc/des_visits.hip, the walk in csrc/des_visits.h; host code only) ----
 * An event_id is a customer and keeps its id from node to node.  Per sample b, over its records [rec_ptr[b],
 * rec_ptr[b + 1]), with i the index of a record relative to the sample's first:
 *   arrival (kind 0) at node n, id e, value t: opens visit v (node, event_id, rec_arrival = i, t_arrival = t); prev_visit
 *     = the customer's visit before (-1: none), whose next_visit becomes v; a customer's OPEN visit is its latest one;
 *   processing (kind 2) at n, e, value s: starts e's open visit, which must be at n and not started: rec_start = i,
 *     service = s, t_start = the value of the latest arrival or departure record before it;
 *   departure (kind 1) at n, e, value t: ends e's open visit, which must be at n and started: n_departures + 1; the first
 *     one sets rec_first_depart / t_first_depart, every one rec_depart / t_depart -- the last one wins (a 'queue' node's
 *     delayed departures are several departure records of one visit).
 * Visit rows, CSR over samples by visit_ptr (B + 1), indices relative to the sample; column k of a block of n_visits_cap
 * rows starts at k * n_visits_cap; -1 / NaN = none; the doubles are copies of log values:
 *   visit_i32 (3, cap): node, n_departures, outcome (GDM_DES_VISIT_DEPARTED: a departure was logged; _IN_SERVICE:
 *     started, no departure; _UNSERVED: never started -- turned away, or still waiting when the log ended: the log alone
 *     cannot tell.  A queue node's customer whose last logged departure was a delayed one reads as DEPARTED at that
 *     clock: at most one per queue node and log)
 *   visit_i64 (7, cap): event_id, rec_arrival, rec_start, rec_first_depart, rec_depart, prev_visit, next_visit
 *   visit_f64 (5, cap): t_arrival, t_start, service, t_first_depart, t_depart
 * Customer rows, CSR by cust_ptr (B + 1); row = event id, 0 .. the largest id seen; blocks of n_customers_cap rows:
 *   cust_i32 (2, cap): n_visits (0: the id has no record; then outcome GDM_DES_CUST_ABSENT, visits -1, times NaN, sums
 *     0), outcome (from the last visit: GDM_DES_CUST_EXITED, _IN_NET or _UNSERVED; EXITED means no later arrival was
 *     logged)
 *   cust_i64 (2, cap): first_visit, last_visit
 *   cust_f64 (4, cap): t_enter (t_arrival of the first visit), t_exit (t_depart of the last visit when it DEPARTED, else
 *     NaN), service_sum and wait_sum: the sums of service and of (t_start - t_arrival) over the customer's started
 *     visits, from 0.0 in visit order (first_visit, then next_visit)
 * status (B) i32; a refused sample has ZERO visits and ZERO customers and its neighbours are what they are without it:
 *   GDM_DES_VISITS_ERECORD  a kind outside 0..2; a node outside 0..dim-1; an event_id < 0 or > n + dim, n the sample's
 *     record count (an id is handed out at the latest when an earlier arrival of its source is processed); a processing
 *     or departure record whose customer has no open visit at that node; a second processing for one visit; a departure
 *     before its processing; a processing record with no clock record before it (which the open visit's arrival rules out)
 *   GDM_DES_VISITS_EPTR     offsets outside the record arrays
 * The six tables NULL with both caps 0 only counts (visit_ptr, cust_ptr, status); GDM_EWORKSPACE when a cap is too
 * small: visit_ptr[B] / cust_ptr[B] then hold the counts needed and the tables' contents are not defined.
 * There is NO device entry and no kernel: a log on the device is read back once.           */
#define GDM_DES_VISITS_ERECORD 1
#define GDM_DES_VISITS_EPTR 2
#define GDM_DES_VISIT_UNSERVED 0
#define GDM_DES_VISIT_IN_SERVICE 1
#define GDM_DES_VISIT_DEPARTED 2
#define GDM_DES_CUST_ABSENT (-1)
#define GDM_DES_CUST_UNSERVED 0
#define GDM_DES_CUST_IN_NET 1
#define GDM_DES_CUST_EXITED 2
#define GDM_DES_VISITS_MAX_DIM 4096
#define GDM_DES_VISITS_MAX_RECORDS ((int64_t)1 << 40)
int gdm_des_log_visits_host(const double* value, const int64_t* event_id, const int32_t* node, const int32_t* kind,
                            const int64_t* rec_ptr, int64_t n_records, int B, int dim, int64_t* visit_ptr,
                            int64_t* cust_ptr, int32_t* status, int32_t* visit_i32, int64_t* visit_i64,
                            double* visit_f64, int64_t n_visits_cap, int32_t* cust_i32, int64_t* cust_i64,
                            double* cust_f64, int64_t n_customers_cap);

/* ---- generic convolution lowering helpers (model 2 discriminator, model 1 generator) ----------------------------
 * im2col for Conv2d fwd / dW and col2im (gather form, deterministic) for Conv2d dX and ConvTranspose2d fwd.
 * Activations are channels-last (B,H,W,C) unless `src_planar` (NCHW fp32 input planes, e.g. the piano-roll).
 * cols: (B*OH*OW, C*KH*KW) row-major with k = (c*KH + kh)*KW + kw -- torch's weight order, so Conv2d weights
 * (Cout, Cin*KH*KW) and ConvTranspose2d weights (Cin, Cout*KH*KW) are GEMM operands in place.                       */
int gdm_im2col(const void* src, int src_dtype, int src_planar, int B, int H, int W, int C, int KH, int KW,
               int stride, int pad, int OH, int OW, void* cols, int cols_dtype, void* stream);
/* dst[b,h,w,c] = sum over (oh,ow,kh,kw) with oh*stride-pad+kh==h, ow*stride-pad+kw==w of cols[(b,oh,ow),(c,kh,kw)].
 * dst_planar: bit 0 = write (B,C,H,W) instead of channels-last; bit 1 = the columns of `cols` are ordered (kh,kw,c)
 * (tap-major: what a GEMM with the weight permuted to (Cin, KH, KW, Cout) produces -- coalesced reads) instead of
 * torch's (c,kh,kw); bits 4-5 = GDM_ACT_* applied to the sum (RELU / SIGMOID; LEAKY is not offered here).            */
int gdm_col2im(const void* cols, int cols_dtype, int B, int H, int W, int C, int KH, int KW, int stride, int pad,
               int OH, int OW, void* dst, int dst_dtype, int dst_planar, void* stream);

/* dst (B,C,P) = src (B,P,C) transposed per batch element, with dtype conversion (channels-last <-> channel-major
 * flatten order: activations, and fc1's weight / weight gradient viewed as (128, 32, H2*W2) <-> (128, H2*W2, 32)). */
int gdm_permute_pc(const void* src, int src_dtype, int B, int P, int C, void* dst, int dst_dtype, void* stream);

/* aten::max_pool2d_with_indices / its backward, kernel 2 stride 2 (floor), channels-last (B,H,W,C) -> (B,H/2,W/2,C)
 * (F.max_pool2d(x, 2, 2) of the SimNN branch, GAN_DES/SIMNN.py:156,158).  idx: window position 0..3 of the first
 * maximum in scan order, one byte per output element (NULL: forward only).  dst holds that very element, bit for bit
 * (a window of -0.0 and +0.0 gives whichever comes first, like ATen).                                                */
int gdm_maxpool2_fwd(const void* src, int dtype, int B, int H, int W, int C, void* dst, uint8_t* idx_or_null,
                     void* stream);
int gdm_maxpool2_bwd(const void* dout, int dtype, const uint8_t* idx, int B, int H, int W, int C, void* dx,
                     void* stream);

/* ---- batched DES-matrix prologue (numpy head of matrix_to_midi, MMGAN_MIDI_DES/matrix_sim_process.py:33-117, and of
 * matrix_to_wav, GAN_DES/matrix_sim_process.py:21-95): generated matrix -> what simulation_v3.Sim is constructed from.
 * g: B samples of an (S,S) fp32 matrix, sample_stride floats apart (the generator output in place); dim = number of
 * DES nodes (S - 3 / S - 5); rows dim.. are parameter rows.  The reference interleaves this arithmetic with draws from
 * numpy's global RNG whose consumption depends on the data, so the host advances the stream between the two calls:
 * gdm_des_scan    |m| -> thr_mask (B,S) u8 = |m[dim][x]| > threshold (NULL: skip); instruments (B,dim) i32 =
 *                 int(|m[dim+1][i]| * 126); note_levels (B,dim) i32 = int(|m[dim+2][i]| * 126), with note_mod:
 *                 max(0, . % 128); zero_mask (B,dim) u64, bit x of row i set iff |m[i][x]| == 0 (x < dim);
 *                 norm_aux: aux (B,2,dim) fp32 = rows dim+3, dim+4 divided by their sequential float32 sum over all S
 *                 entries (model 1's distribution rows); flags (B) i32, bit 0 = the sample holds a non-finite value or
 *                 an instrument / note-level product |m| * 126 that is not below 2^31 (stored as INT32_MAX; Python's
 *                 int() upstream has no such limit).
 * gdm_des_routing src_mask (B,dim) u8 (1 = source node), residue_col (B,dim) i32 (column that absorbs 1 - sum(row);
 *                 < 0: none) -> out (B,dim,dim) fp64: source columns and diagonal zeroed, rows divided by their
 *                 float64 sum in numpy's pairwise order (0/0 -> 0), residue added, diagonal +1 (source) / -1 (server).
 * S <= 64.  Results are bit-identical to numpy's on finite inputs (tests/golden/des_prologue.npz).                  */
int gdm_des_scan(const float* g, int64_t sample_stride, int B, int S, int dim, float threshold, int note_mod,
                 int norm_aux, uint8_t* thr_mask_or_null, int32_t* instruments, int32_t* note_levels,
                 uint64_t* zero_mask, float* aux_or_null, int32_t* flags, void* stream);
int gdm_des_routing(const float* g, int64_t sample_stride, int B, int S, int dim, const uint8_t* src_mask,
                    const int32_t* residue_col, double* out, void* stream);

/* ---- the draws between the two, per sample on a stream of its own ("des_device"; csrc/des_draws.h is the one source):
 * sample b's stream is numpy's RandomState(base[b]) (init_genrand, position 624, no cached gauss).  On it, in the
 * reference's order: the random sources np.random.choice(dim, size=k, replace=False) (MMGAN_MIDI_DES/
 * matrix_sim_process.py:44, k = dim / 4; GAN_DES/matrix_sim_process.py:28, k = S / 8, drawn only when no column of
 * thr_mask passes, :25-30), one np.random.choice(candidates) per row for the column that takes the rounding residue
 * (:102 / :87; candidates = columns not zero in zero_mask, not sources, not the row itself), then the reseed pair
 * np.random.seed(np.random.randint(0, 99999, size=1)); seeds = np.random.randint(0, 99999, size=1) (:114-115 / :105-106).
 * route 0 (midi): params = gen2_output (B, n_params >= 7) fp32: loc / scale = |p[1] * 50|, |p[2] * 50| for a source and
 *   |p[3] * 10|, |p[4] * 10| for a server (:72-74), customers = max(200, max(1000, int(3000 * p[6]))) (:13, :151-163).
 * route 1 (wav): params = gdm_des_scan's aux (B, 2, dim), n_params = 2 dim: 30 r3, 15 r4 / 5 r3, 3 r4 (:57-59),
 *   customers = 1000 (:110); needs thr_mask (B,S) and 1 <= S / 8 <= dim.
 * All arithmetic is float32 widened to float64, as numpy's.  instrument_override (B) i32 or NULL: a program for every
 * node of the sample, INT32_MIN = none (the scan's instruments).  Outputs: src (B,dim) u8, cols (B,dim) i32 -- what
 * gdm_des_routing takes --, seed, customers (B) i64, loc, scale (B,dim) f64, queue_cap (B,dim) i32 = 254, instruments,
 * note_levels (B,dim) i32, the stream after the last draw (mt_key (B,624), mt_pos, has_gauss (B) i32, cached_gauss (B)
 * f64) -- what gdm_des_run_batch takes --, status (B) i32: 0 ok, 1 empty candidate list (ValueError upstream), 2 more
 * than one thresholded source (ValueError, GAN_DES :30), 3 thresholded column >= dim (IndexError, :67), 4 draw budget
 * exhausted, 5 int(3000 * p[6]) undefined (NaN, inf, beyond int64).  A sample with status != 0 has zero src / cols /
 * seed, the stream of RandomState(base[b]) untouched, and scale -1, which makes gdm_des_run_batch end it with
 * GDM_DES_STOP_ERROR and no records.  dim <= S <= 64.  gdm_des_draws: device arrays, one wave per sample;
 * gdm_des_draws_host: host arrays, the same source, the same bits.                                                   */
int gdm_des_draws(int route, int B, int S, int dim, const uint32_t* base, const uint64_t* zero_mask,
                  const uint8_t* thr_mask_or_null, const int32_t* scan_instruments, const int32_t* scan_note_levels,
                  const float* params, int n_params, const int32_t* instrument_override_or_null, uint8_t* src,
                  int32_t* cols, int64_t* seed, int64_t* customers, double* loc, double* scale, int32_t* queue_cap,
                  int32_t* instruments, int32_t* note_levels, uint32_t* mt_key, int32_t* mt_pos, int32_t* has_gauss,
                  double* cached_gauss, int32_t* status, void* stream);
int gdm_des_draws_host(int route, int B, int S, int dim, const uint32_t* base, const uint64_t* zero_mask,
                       const uint8_t* thr_mask_or_null, const int32_t* scan_instruments,
                       const int32_t* scan_note_levels, const float* params, int n_params,
                       const int32_t* instrument_override_or_null, uint8_t* src, int32_t* cols, int64_t* seed,
                       int64_t* customers, double* loc, double* scale, int32_t* queue_cap, int32_t* instruments,
                       int32_t* note_levels, uint32_t* mt_key, int32_t* mt_pos, int32_t* has_gauss,
                       double* cached_gauss, int32_t* status);

/* ---- piano-roll rasteriser (the scatter of generate_piano_roll, MMGAN_MIDI_DES/datasets.py:29-45), batched over files.
 * Messages of row r = file * 128 + note are ev_*[row_ptr[r] .. row_ptr[r+1]) in file order; ev_step = one-second time
 * step of the message, ev_vel = velocity of a note_on (0..127) or -1 for a note_off.  Writes roll, dur (n_files,128,W)
 * fp32: roll[note][step] = last note_on velocity, dur[note][on:off] = off - on of the note_off that closed it.
 * The host has already cut each file's list where the reference's loop stops.                                        */
int gdm_piano_roll_raster(const int32_t* row_ptr, const int32_t* ev_step, const int32_t* ev_vel, int n_files, int W,
                          float* roll, float* dur, void* stream);

/* ---- windowed piano-roll rasteriser: the planes of generate_piano_roll(midi, sample_size, beats_length) of
 * data_viewing_and_processing.ipynb cell 10 (the event loop of MMGAN_MIDI_DES/datasets.py:29-45 on (128, sample_size)
 * planes) cut into windows of L steps as cell 11 cuts them, without building the full-width planes.
 * row_ptr / ev_step / ev_vel are gdm_piano_roll_raster's CSR arrays.  Window n < n_windows is (win_file[n], win_s0[n]):
 * roll, dur (n_windows,128,L) fp32 receive columns [s0, s0 + L) of that file's planes -- a duration written by a
 * note_off keeps its full-length value off - on in every window it crosses, note_on_time carries over from earlier
 * windows, later messages overwrite earlier ones, and what no message writes is zero.  Any window list is allowed (any
 * first step, overlaps, window 0); which windows a dataset keeps is the caller's policy.  One launch, one workgroup per
 * window, both planes built in LDS and stored with 16-byte stores: L <= 160 (2 * 128 * L floats <= 160 KB), roll and
 * dur 16-byte aligned, win_s0[n] >= 0 and win_s0[n] + L <= INT32_MAX, win_file[n] a file of row_ptr (the caller's
 * statement about device arrays: the Python wrapper checks it).                                                     */
int gdm_piano_roll_windows(const int32_t* row_ptr, const int32_t* ev_step, const int32_t* ev_vel,
                           const int32_t* win_file, const int32_t* win_s0, int n_windows, int L, float* roll,
                           float* dur, void* stream);

/* ---- DES log -> MIDI track -> piano-roll planes, batched over samples (process_adjsim_log / MidiGenerator,
 * MMGAN_MIDI_DES/sim_log_to_midi.py:14-277, then generate_piano_roll on the file it builds, datasets.py:13-54).
 * One launch, one workgroup per sample.  Records of sample s are value/event_id/node/kind[rec_ptr[s] .. rec_ptr[s+1])
 * (the fields of the DES core's event log, gdm_des_run; rec_ptr has B + 1 entries, all clamped to [0, n_records]);
 * only the first 5000 are looked at, as the reference's reader does.  tails (B, tail_stride) fp32: gen2_output[10:],
 * six values used; instruments, note_levels (B, dim) i32; save (B) i32: non-zero = save_midi runs for this sample
 * (the caller decides: `generate` or a line count that is a multiple of 100) -- otherwise the reference's MidiFile
 * has no track and the planes stay zero.  start / end / sequence_length are generate_piano_roll's.
 * Outputs (planes and track 16-byte aligned: checked): planes (B, 2, 128, W) fp32 = [roll, durations] with W = the width the reference's final slice leaves
 * (checked); track (B, track_cap, 4) i32 = (kind, a, b, time) quadruples, kind one of GDM_MIDI_*, a/b = tempo,0 |
 * numerator,denominator | key index,0 | program,0 | note,velocity | 0,0; track_len (B) i32; status (B) i32:
 * bit 0 = the track is the saved one (after save_midi), bits 8.. = 0 or a GDM_DES_MIDI_E* code (the reference raises
 * for such a sample; its track is empty and its planes are zero).                                                  */
#define GDM_MIDI_SET_TEMPO 0
#define GDM_MIDI_TIME_SIGNATURE 1
#define GDM_MIDI_KEY_SIGNATURE 2
#define GDM_MIDI_PROGRAM_CHANGE 3
#define GDM_MIDI_NOTE_ON 4
#define GDM_MIDI_NOTE_OFF 5
#define GDM_MIDI_END_OF_TRACK 6
#define GDM_DES_MIDI_TRACK_CAP 512 /* the reference stops appending at 500 messages (+ 1 + end_of_track) */
#define GDM_DES_MIDI_MAX_NODES 256
#define GDM_DES_MIDI_EPARAMS 1 /* a tail value is not finite, beyond int32 after scaling, or gives a negative tempo */
#define GDM_DES_MIDI_ENODE 2   /* an arrival at a node without instrument / note level (KeyError upstream) */
#define GDM_DES_MIDI_ERANGE 3  /* program or note outside 0..127 (mido refuses the message) */
#define GDM_DES_MIDI_EMODULO 4 /* base + var == 0: customer_id % 0 */
int gdm_des_log_to_roll(const double* value, const int64_t* event_id, const int32_t* node, const int32_t* kind,
                        const int64_t* rec_ptr, int64_t n_records, const float* tails, int tail_stride,
                        const int32_t* instruments, const int32_t* note_levels, int dim, const int32_t* save, int B,
                        int start, int end, int sequence_length, float* planes, int W, int32_t* track, int track_cap,
                        int32_t* track_len, int32_t* status, void* stream);

/* ---- mel-spectrogram featuriser (GAN_DES/util.py:37-61: torchaudio MelSpectrogram + AmplitudeToDB) --------------
 * The producer of model 1's discriminator input.  DFT and mel filter bank are gdm_gemm calls in exact fp32 (window
 * folded into the [cos | sin] matrix); these three functions are the kernels around them.
 * gdm_stft_frames: x (B windows of L samples, x_stride apart) -> out (B*frames, n_fft) centred frames, reflect padding
 *   (torch.stft center=True, pad_mode="reflect"; frames = 1 + L / hop).
 * gdm_power_spectrum: c (rows, 2*nfreq) = [re | im] -> p (rows, ldp) = re^2 + im^2 (Spectrogram power=2); columns
 *   nfreq..ldp-1 are zero padding for the following GEMM.
 * gdm_power_to_db: mel (B, frames, n_mels) -> out (B, n_mels, frames) = max(10 log10(max(mel, amin)),
 *   window max - top_db)  (AmplitudeToDB(stype="power", top_db); top_db < 0 = no floor).                             */
int gdm_stft_frames(const float* x, int B, int64_t L, int64_t x_stride, int hop, int n_fft, int frames, float* out,
                    void* stream);
int gdm_power_spectrum(const float* c, int64_t rows, int nfreq, int ldp, float* p, void* stream);
int gdm_power_to_db(const float* mel, int B, int frames, int n_mels, float top_db, float amin, float* out, void* stream);

/* ---- PCM front end of the featuriser (GAN_DES/datasets.py:26-43, GAN_DES/util.py:89-119) ---------------------------
 * What torchaudio.load(normalize=True), the channel rule and the window loops of InputSong / split_audio_data /
 * get_melspectrogram_db_tensor_from_file produce, read straight from a WAV file's sample bytes on the device: `pcm` is
 * the data chunk (little-endian, interleaved, n_samples sample frames of `channels` = 1..8 samples, aligned to the
 * element size: 1 byte for U8 and S24, 2 for S16, 4 for S32 and F32).  Each stored sample becomes one fp32 first:
 *   U8  (v - 128) * 2^-7        S16  v * 2^-15        S24 (3 bytes)  v * 2^-23
 *   S32 (float)v, rounded to nearest even, then * 2^-31              F32  the float as stored
 * These are the values torchaudio documents for normalize=True.  PINNED: S16 only (every step is exact in fp32, and the
 * three 16-bit files the reference ships are fixtures); the other formats follow the formula above and nothing else,
 * because torchaudio is not available to compare with.
 * mix = c >= 0: channel c (InputSong's `channel = 0`).  mix = -1: waveform.mean(dim=0) = the decoded channels added left
 * to right in fp32, then one correctly rounded division by `channels` (S32 therefore rounds per sample and per sum;
 * S16 and S24 means are exact).  No multiply-add is contracted.
 * gdm_pcm_to_float: out[t] = mono(first + t), t < count; requires 0 <= first, count > 0, first + count <= n_samples.
 * gdm_pcm_stft_frames: gdm_stft_frames over windows of the song that are never materialised.  Window w < n_regular
 *   starts at start0 + w * stride; if tail_start >= 0 one more window starts there (InputSong's last window, taken from
 *   the end).  All windows are win_len samples long.
 *   out[((w * frames + f) * n_fft) + j] = mono(start_w + reflect(f * hop + j - n_fft / 2, win_len)), the reflection
 *   (s < 0 -> -s, s >= win_len -> 2 (win_len - 1) - s) staying inside the window: no neighbour's sample is read.
 *   Checked before the launch: every start >= 0 and start + win_len <= n_samples, win_len > n_fft / 2,
 *   (frames - 1) * hop <= win_len, n_fft % 4 == 0, out 16-byte aligned.  A bad table is GDM_EINVAL, never a read
 *   outside the buffer (whose size, n_samples * channels * bytes per sample, is the caller's statement).            */
#define GDM_PCM_U8 0
#define GDM_PCM_S16 1
#define GDM_PCM_S24 2
#define GDM_PCM_S32 3
#define GDM_PCM_F32 4
int gdm_pcm_to_float(const void* pcm, int fmt, int channels, int mix, int64_t n_samples, int64_t first, int64_t count,
                     float* out, void* stream);
int gdm_pcm_stft_frames(const void* pcm, int fmt, int channels, int mix, int64_t n_samples, int64_t start0,
                        int64_t stride, int n_regular, int64_t tail_start, int64_t win_len, int hop, int n_fft,
                        int frames, float* out, void* stream);

/* ---- model 1's DES bridge: DES log -> notes -> integer synth -> STFT frames / PCM --------------------------------
 * What the reference does per generated sample between Sim.run and the mel featuriser (GAN_DES/matrix_sim_process.py:
 * 112-129): process_adjsim_log builds a MIDI file from the log, FluidSynth renders it, the WAV is loaded again.
 *
 * gdm_des_log_to_notes (GAN_DES/sim_log_process_music.py:65-133 MidiGenerator.process_line, :159-185 the reader):
 *   one launch, one workgroup per sample; records in the CSR layout of gdm_des_log_to_roll, only the first 5000 of a
 *   sample are looked at; note_levels (B, dim) i32.  Outputs: notes (B, notes_cap, 4) i64 = (on_tick, off_tick, pitch,
 *   velocity) -- the ticks are the cumulative delta times of the strictly sequential note_on / note_off track, as mido
 *   reads it --, n_notes (B) i32 <= 5000, clip_len (B) i64 = sample(last off_tick) + GDM_SYNTH_RELEASE (0: no notes),
 *   status (B) i32 = 0 or a GDM_DES_NOTES_E* code; a sample with a code has n_notes = clip_len = 0.
 *   sample(tick) = (tick * 735) >> 3: 1/480 s per tick (set_tempo 1 000 000, 480 ticks per beat) at 44 100 Hz.
 *
 * The synth (defined HERE: FluidSynth's sound font is not imitated).  Integer only.  Tables: wave[2048] i16 (default
 * round(32767 sin(2 pi i / 2048))), inc[128] u32 = round(2^32 * 440 * 2^((p - 69) / 12) / 44100), both built by the
 * host in float64.  A voice with s_on = sample(on_tick), s_off = sample(off_tick), pitch p and velocity v (both taken
 * & 127) contributes at sample s in [s_on, s_off + R):
 *     phase = (uint32)(inc[p] * (s - s_on))            e_att = min(s - s_on + 1, A)
 *     e_rel = s < s_off ? R : R - (s - s_off)          voice = ((int64)wave[phase >> 21] * v * e_att * e_rel) >> SHIFT
 *   (arithmetic shift: -8128 <= voice <= 8127).  A sample is the int32 sum of its voices clamped to [-32768, 32767];
 *   5000 voices stay below 2^26.
 * gdm_synth_frames: frames (B * 216, 2048) fp32, the matrix gdm_stft_frames would cut from the rendered clips: with
 *   hop = clip_len / 215, element (b, f, n) = sample(reflect(f * hop + n - 1024, clip_len)) * 2^-15, reflect as in
 *   gdm_pcm_stft_frames.  A clip with n_notes = 0 (or clip_len <= 1024) gives zero frames.  One workgroup per (b, f).
 * gdm_synth_pcm: out[i] = sample(first + i), i < count, of ONE clip (notes, n_notes point at it), as 16-bit PCM.
 * Checked before the launch: notes_cap <= 5000 (the voice list in LDS), alignment (frames / out: 16 bytes), the sample
 * range.  n_notes is clamped to [0, notes_cap] on the device; no other device value forms an address.
 *
 * gdm_synth_windows: W windows of F clips of any length as 16-bit PCM, one launch (a MIDI performance rendered for the
 *   mel featuriser: datasets.MaestroDataset, datasets.midi_to_wav).  notes (n_total, 4) i64 = (s_on, s_off, pitch,
 *   velocity) with the times IN SAMPLES at 44 100 Hz, the rows of the F clips back to back, note_ptr (F + 1) i64 the
 *   offset of each clip's rows; within a clip the rows ascend in s_on, and off_max[k] is the maximum of s_off over the
 *   clip's rows up to and including k (non-decreasing within a clip).  Window w is samples [win_start[w], win_start[w]
 *   + win_len) of clip win_clip[w] (i32):
 *     out[w * out_stride + i] = the int32 sum over the clip's voices of the formula above at s = win_start[w] + i,
 *     clamped to [-32768, 32767], for i < win_len; out[w * out_stride + win_len ..] is not written.
 *   A sample where no voice sounds (before the first note, beyond the clip's end, a clip without rows) is 0.
 *   One workgroup per (2048 samples, window).  It does not scan the clip: rows from the first with s_on > hi on, and
 *   rows before the first with off_max + R > lo, cannot sound in its samples [lo, hi]; two binary searches find both,
 *   and the rows between are taken in tiles of GDM_SYNTH_TILE, each filtered into a fixed list in LDS.  No limit on
 *   the rows of a clip or on simultaneous voices; the integer sum does not depend on the order, so every bit is defined.
 *   The int32 sum is the caller's to keep: fewer than 2^18 voices at one sample cannot overflow it (2^18 * 8128 < 2^31).
 *   Checked before the launch: null pointers (notes / off_max may be null iff n_total = 0), alignment (out: 16 bytes,
 *   every table: its element), 1 <= F, 1 <= W <= 65535, 1 <= win_len <= 2^30, out_stride >= win_len and
 *   out_stride % 8 == 0, n_total >= 0.  On the device win_clip is clamped to [0, F), both ends of a clip's row range
 *   to [0, n_total] with start <= end, the searches stay inside that range, and win_start is taken within +-2^62; no
 *   other value read from device memory forms an address.  If the rows do not ascend or off_max is not the running
 *   maximum, voices may be missed, nothing else.
 *
 * A Standard MIDI File -> those rows (datasets.midi_notes; host, exact integer arithmetic):
 *   time: tracks merged stably by absolute tick; with U = the running sum of delta_ticks * tempo in force (us per beat;
 *     500 000 until the first set_tempo; a set_tempo applies to the messages after it), a message sounds at sample
 *     U * 441 / (ticks_per_beat * 10000), rounded down.  Tempo 1 000 000 at 480 ticks per beat gives sample(tick) above.
 *   pairing: a note_on with velocity > 0 opens a note on its (channel, pitch); a note_off, or a note_on with velocity
 *     0, closes the OLDEST open note of that (channel, pitch) and is ignored when there is none; notes still open at
 *     the end close at the file's last message (the end_of_track with the largest tick included).
 *   sustain pedal (controller 64 per channel, value >= 64 = down): a close that arrives while the pedal is down is
 *     deferred; the note ends at the earliest of the pedal's release on its channel, the next note_on of its
 *     (channel, pitch), and the file's last message.
 *   All channels sound the one voice, program changes are ignored, pitch and velocity are kept as stored.
 *   clip_len = max(s_off) + GDM_SYNTH_RELEASE, or 5 * 44100 for a file without notes; refused: U * 441 >= 2^63,
 *   clip_len > 2^40, 2^18 notes or more.                                                                           */
#define GDM_DES_NOTES_MAX 5000
#define GDM_DES_NOTES_ENODE 1  /* a note for a node without note level (KeyError upstream) */
#define GDM_DES_NOTES_EPITCH 2 /* note outside 0..127 (mido refuses the message) */
#define GDM_DES_NOTES_ELONG 3  /* the clip would pass 2^40 samples: left blank, nothing is raised */
#define GDM_DES_NOTES_EPROGRAM 4 /* gdm_des_log_to_notes_pc: program outside 0..127 (mido refuses the message) */
#define GDM_SYNTH_ATTACK 256
#define GDM_SYNTH_RELEASE 8192
#define GDM_SYNTH_SHIFT 30
#define GDM_SYNTH_WAVE 2048
#define GDM_SYNTH_FRAMES 216
#define GDM_SYNTH_NFFT 2048
#define GDM_SYNTH_TILE 1024 /* rows a gdm_synth_windows workgroup filters at a time (16 KB of LDS) */
int gdm_des_log_to_notes(const double* value, const int64_t* event_id, const int32_t* node, const int32_t* kind,
                         const int64_t* rec_ptr, int64_t n_records, const int32_t* note_levels, int dim, int B,
                         int64_t* notes, int notes_cap, int32_t* n_notes, int64_t* clip_len, int32_t* status,
                         void* stream);
int gdm_synth_frames(const int64_t* notes, int notes_cap, const int32_t* n_notes, const int64_t* clip_len, int B,
                     const int16_t* wave, const uint32_t* inc, float* frames, void* stream);
int gdm_synth_pcm(const int64_t* notes, int notes_cap, const int32_t* n_notes, const int16_t* wave, const uint32_t* inc,
                  int64_t first, int64_t count, int16_t* out, void* stream);
int gdm_synth_windows(const int64_t* notes, const int64_t* off_max, int64_t n_total, const int64_t* note_ptr, int F,
                      const int32_t* win_clip, const int64_t* win_start, int W, int64_t win_len, int64_t out_stride,
                      const int16_t* wave, const uint32_t* inc, int16_t* out, void* stream);

/* ---- the stand-alone demo: random (or given) matrix -> DES -> MIDI -> WAV (SIMULATOR/simulation_to_wav.py) ------------
 * gdm_s2w_prologue (:25-71): m (B, S, S) float64 device matrices, read and not modified; dim = S - 5 nodes, rows dim ..
 *   dim + 4 are the parameter rows.  One launch, one workgroup per sample.  Outputs, bit for bit what the reference's
 *   numpy float64 code computes: src (B,dim) u8 = m[dim][i] > 0.75 (false for a NaN); instruments, note_levels (B,dim)
 *   i32 = (int)(m[dim+1][i] * 127), (int)(m[dim+2][i] * 127) (truncation; no abs and no 126 as in gdm_des_scan);
 *   instrument_override (B) i32 or NULL puts one program on every node of a sample, INT32_MIN = none, as in
 *   gdm_des_draws; loc, scale (B,dim) f64 = 10 r3, 5 r4 for a source and 3 r3, 2 r4 for a server (r3, r4 = rows dim+3,
 *   dim+4); queue_cap (B,dim) i32 = 127; adj (B,dim,dim) f64: EVERY column c < S with m[dim][c] > 0.75 is zeroed (a
 *   given matrix may mark parameter columns), the diagonal is zeroed, each row i < dim is divided (IEEE) by Python's
 *   sum() of it -- the strictly sequential left-to-right float64 sum over all S entries, parameter columns included --,
 *   then the diagonal is +1 for a source and -1 for a server and the first dim columns are kept.  Nothing is drawn and
 *   no NaN is repaired: status (B) i32 = 1 when a row sum is zero or not finite (0 otherwise); such a sample has scale
 *   -1 on every node -- gdm_des_run_batch ends it with GDM_DES_STOP_ERROR and no records -- and an adj of zeros around
 *   its diagonal; its neighbours are untouched.  Checked before the launch: null pointers, GDM_S2W_MIN_SIZE <= S <=
 *   GDM_S2W_MAX_SIZE, B >= 1, every array aligned to its elements.  No value read from device memory forms an address.
 *
 * gdm_des_log_to_notes_pc (:162-214, the demo's own MidiGenerator): gdm_des_log_to_notes -- same records, same reader,
 *   same replay, one source -- for the copy whose program_change lines are live: the track receives program_change(on),
 *   note_on(on), program_change(off), note_off(off), so on_tick = ticks + 2 on and off_tick = on_tick + 2 off, and a
 *   note row has FIVE columns (on_tick, off_tick, pitch, velocity, program) with program = instruments[node]
 *   (instruments (B,dim) i32).  A program outside 0..127 is GDM_DES_NOTES_EPROGRAM (tested before the pitch: the
 *   program_change is built first).  The demo never calls generate_midi, so its file has no set_tempo; the tick ->
 *   sample rule is therefore not fixed here but passed: sample(tick) = tick * tick_mul / tick_div (integers, rounded
 *   down; 735 / 16 for the default tempo 500 000 at 480 ticks per beat -- the rule datasets.midi_notes applies to the
 *   written file), clip_len = sample(last off_tick) + tail (0: no notes).  GDM_DES_NOTES_ELONG when sample + tail would
 *   pass 2^40, tested against the doubled steps before they are added.  1 <= tick_mul, tick_div <= 2^20, 0 <= tail <=
 *   2^30, every array aligned to its elements.
 *
 * gdm_synth_windows_gm: gdm_synth_windows with a timbre per General MIDI family.  Same windows, tiles, searches and
 *   checks; note rows are (n_total, 5) i64 (s_on, s_off, pitch, velocity, program) and the family is f = (program & 127)
 *   >> 3.  Tables from the caller: waves (16, 2048) i16, env (16, 2) i32 = (A_f, R_f), clamped on the device to 1 ..
 *   2^21 each.  With the tables ops.synth_gm_tables builds, A_f * R_f = 2^21 = GDM_SYNTH_ATTACK * GDM_SYNTH_RELEASE
 *   for every family, so the voice bound and the int32-sum argument above carry over.  A voice contributes at s in
 *   [s_on, s_off + R_f):
 *     phase = (uint32)(inc[p] * (s - s_on))            e_att = min(s - s_on + 1, A_f)
 *     e_rel = s < s_off ? R_f : R_f - (s - s_off)      voice = ((int64)waves[f][phase >> 21] * v * e_att * e_rel) >> 30
 *   end_max[k] = the running maximum of s_off + R_f(row) over the clip's rows up to k (the release varies per row; it
 *   stands where off_max stands).  The 64 KB of wave tables and the 16 envelopes are staged in LDS by every workgroup:
 *   the inner loop reads one table entry per voice and sample at a data-dependent index, which LDS serves per lane and
 *   a global load would serve per cache line.  waves and out 16-byte aligned.                                         */
#define GDM_S2W_MIN_SIZE 6
#define GDM_S2W_MAX_SIZE 256
#define GDM_SYNTH_GM_FAMILIES 16
#define GDM_SYNTH_GM_ENV_MAX (1 << 21)
int gdm_s2w_prologue(const double* m, int B, int S, const int32_t* instrument_override_or_null, uint8_t* src,
                     int32_t* instruments, int32_t* note_levels, double* loc, double* scale, int32_t* queue_cap,
                     double* adj, int32_t* status, void* stream);
int gdm_des_log_to_notes_pc(const double* value, const int64_t* event_id, const int32_t* node, const int32_t* kind,
                            const int64_t* rec_ptr, int64_t n_records, const int32_t* instruments,
                            const int32_t* note_levels, int dim, int B, int64_t tick_mul, int64_t tick_div, int64_t tail,
                            int64_t* notes, int notes_cap, int32_t* n_notes, int64_t* clip_len, int32_t* status,
                            void* stream);
int gdm_synth_windows_gm(const int64_t* notes, const int64_t* end_max, int64_t n_total, const int64_t* note_ptr, int F,
                         const int32_t* win_clip, const int64_t* win_start, int W, int64_t win_len, int64_t out_stride,
                         const int16_t* waves, const int32_t* env, const uint32_t* inc, int16_t* out, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* GDM_H */
