/* agent0_hip.h — C-ABI of libagent0_hip.so: the MI355X (gfx950) hot path of agent0's deepq actor-learner loop.
 *
 * The reference (zhoubin-me/agent0) is pure Python and defines no FFI; each entry point below names the reference
 * code it replaces (paths relative to the reference repo).  INTEGRATION.md shows the ctypes binding a maintainer
 * of the reference would add.  Conventions:
 *   - every function returns int: 0 = A0_OK, < 0 = error (A0_E*), message via a0_last_error() (thread-local);
 *   - all pointers are DEVICE pointers unless a parameter is named host_*; buffers are owned by the caller and
 *     only borrowed for the duration of the call (the library keeps no reference, a0_net tables excepted);
 *   - `stream` is a hipStream_t passed as void*; calls are asynchronous w.r.t. the host, never synchronise,
 *     never allocate (except a0_net_create) and are safe to capture into a hipGraph;
 *   - fp32 everywhere the reference is fp32; u8 frames; int32 actions/slots; int64 replay indices.
 */
#ifndef AGENT0_HIP_H
#define AGENT0_HIP_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define A0_ABI_VERSION 1

/* Control block (device int64[A0_CTRL_WORDS], optional): lets a sequence of launches be captured ONCE into a hipGraph and replayed
 * while counters keep advancing — each kernel adds ctrl[index] to the corresponding immediate argument.  NULL = no adjustment. */
#define A0_CTRL_ENV_STEP 0      /* a0_env_synth_step: g            */
#define A0_CTRL_ACTOR_STEPS 1   /* a0_actor_nstep: steps           */
#define A0_CTRL_RNG_ACTION 2    /* a0_actor_egreedy_rng: off_a     */
#define A0_CTRL_RNG_UNIFORM 3   /* a0_actor_egreedy_rng: off_u     */
#define A0_CTRL_REPLAY_SLOT 4   /* a0_replay_insert: start_slot    */
#define A0_CTRL_RNG_TAUS 5      /* a0_rng_uniform_ctrl (IQN taus)  */
#define A0_CTRL_RNG_NOISE 6     /* a0_rng_normal_ctrl (NoisyNet)   */
#define A0_CTRL_WORDS 8

const char* a0_last_error(void);
int a0_abi_version(void);
/* "default" for the product build; a tuning build (tools/build_variant.sh) reports its name and -D flags, and the product loader refuses it. */
const char* a0_build_info(void);
int a0_device_info(int* cu_count, long long* hbm_bytes, char* arch_name64);

/* ---------------------------------------------------------------- network geometry (agent0/deepq/model.py:90-105) */
typedef struct a0_net_desc {
    int C, H, W;          /* observation shape, cfg.obs_shape (agent0/deepq/main.py:31) */
} a0_net_desc;

typedef struct a0_net a0_net;

/* where a batch of u8 observations lives: frames[(slot ? slot[b] : b) * sample_stride + chan_off + c*H*W + y*W + x] */
typedef struct a0_frames_arg {
    const uint8_t* frames;
    const int* slot;            /* optional gather indices (replay sample), NULL = dense batch */
    long long sample_stride;    /* bytes between samples: 8*H*W for replay rows, 4*H*W for actor observations */
    int chan_off;               /* 0 = st, 4*H*W = st_next half of a replay row (agent0/deepq/agent.py:132-135) */
} a0_frames_arg;

/* one pending slab reduction of a weight gradient (loss.backward(), agent.py:153-155): out[i] = sum_z slabs[z * slab_stride + i], i < count (z ascending: deterministic) */
typedef struct a0_reduce_seg { const float* slabs; long long slab_stride; int nslab; float* out; long long count; } a0_reduce_seg;
typedef struct a0_pending_reduce { a0_reduce_seg seg[4]; int n; } a0_pending_reduce;

/* packed conv weights: w1 [32][C*8*8] in (c,kh,kw) order, w2 [64][4*4*32] and w3 [64][3*3*64] in (kh,kw,c) order */
typedef struct a0_encoder_weights {
    const float *w1, *b1, *w2, *b2, *w3, *b3;
} a0_encoder_weights;

/* one forward pass of a0_net_encoder_fwd_fused_multi: fragment-major weight copies (a0_net_conv_wt_refresh), biases (w->b1 .. b3), frames, observations, outputs */
typedef struct a0_encoder_pass {
    const float* wt; const a0_encoder_weights* w; const a0_frames_arg* f; int B;
    float *act1, *act2, *act3;      /* act1 / act2 optional (a pass that is differentiated keeps them) */
} a0_encoder_pass;

int a0_net_create(const a0_net_desc* desc, a0_net** out);
int a0_net_destroy(a0_net* net);
int a0_net_geometry(const a0_net* net, int* out8);  /* H1,W1,H2,W2,H3,W3,feat_dim,K1 */

/* ConvEncoder.forward (model.py:104-105) with the uint8->fp32 /255 of agent.py:27 / agent.py:129-134 fused into conv1.
 * Outputs are NHWC: act1 [B][H1][W1][32], act2 [B][H2][W2][64], act3 [B][H3][W3][64] (= features in (h,w,c) order). */
int a0_net_encoder_fwd(const a0_net* net, const a0_encoder_weights* w, const a0_frames_arg* frames, int B,
                       float* act1, float* act2, float* act3, void* stream);

/* Fused variant of a0_net_encoder_fwd: one workgroup per observation, activations resident in LDS, bit-identical outputs.
 * wt = k-major copies of the three conv weight matrices (a0_net_conv_wt_floats(C) floats, refreshed by a0_net_conv_wt_refresh
 * whenever the packed weights change); act1 / act2 may be NULL when no backward pass follows. */
int a0_net_encoder_fused_supported(int C, int H, int W);
long long a0_net_conv_wt_floats(int C);
int a0_net_conv_wt_refresh(const a0_encoder_weights* w, int C, float* wt, void* stream);
/* the online network's copies after an optimizer step, mirrored into the target network's copies when that step triggered a target sync
 * (state[4] of a0_adam_step_sync): one launch per update instead of one refresh per network */
int a0_net_conv_wt_refresh_sync(const a0_encoder_weights* w, int C, float* wt, float* wt_target, const int* state, void* stream);
int a0_net_encoder_fwd_fused(int C, int H, int W, const float* wt, const a0_encoder_weights* w, const a0_frames_arg* frames, int B,
                             float* act1, float* act2, float* act3, void* stream);
/* Up to three passes of a0_net_encoder_fwd_fused in ONE launch (the learner's target / online passes over one batch — reference agent.py:176-181 / 222-231 evaluate
 * model_target(next_obs), model(next_obs), model(obs) one after the other; they are independent): bit-identical outputs, 4 x 84 x 84 observations only. */
int a0_net_encoder_fwd_fused_multi(int C, int H, int W, int n, const a0_encoder_pass* pass, void* stream);

/* Fused conv3 + conv2 data gradients per observation (84x84 geometry), the backward-data half of ConvEncoder (model.py:93-105 under
 * autograd, agent.py:136-141): d3 [B][7][7][64] -> d2 [B][9][9][64] and d1 [B][20][20][32], masked by act2 / act1 > 0.  wt = the
 * buffer a0_net_conv_wt_refresh fills (it also holds the flipped / phase-split weight matrices this kernel streams). */
int a0_net_encoder_dgrad_fused_supported(int C, int H, int W);
int a0_net_encoder_dgrad_fused(int C, int H, int W, const float* wt, const float* d3, const float* act1, const float* act2, int B, float* d2,
                               float* d1, void* stream);

/* autograd backward of the encoder (agent.py:153-155).  d3 = dL/d(conv3 pre-activation), already ReLU-masked.
 * g1,g2,g3 receive [dW | db] of each conv in the packed layout.  slabs: a0_net_encoder_bwd_scratch() floats. */
long long a0_net_encoder_bwd_scratch(const a0_net* net, int B);
int a0_net_encoder_bwd(const a0_net* net, const a0_encoder_weights* w, const a0_frames_arg* frames, int B,
                       const float* act1, const float* act2, const float* d3, float* d2, float* d1,
                       float* g1, float* g2, float* g3, float* slabs, void* stream);

/* the three weight-gradient GEMMs of a0_net_encoder_bwd alone: d2 / d1 are inputs (from a0_net_encoder_dgrad_fused) */
int a0_net_encoder_wgrad(const a0_net* net, const a0_encoder_weights* w, const a0_frames_arg* frames, int B, const float* act1, const float* act2,
                         const float* d3, const float* d2, const float* d1, float* g1, float* g2, float* g3, float* slabs, const a0_pending_reduce* pend,
                         void* stream);

/* The update tail in one launch (loss.backward()'s last sums + optimizer.step() + the target copy, agent.py:153-161).  a0_net_encoder_wgrad_tail is a0_net_encoder_wgrad
 * WITHOUT its slab-reduction launch: the reductions (pend's first, then the encoder's) are filed in *plan, and the step's one-thread bookkeeping — NaN skip, step count, bias
 * corrections, "sync now": state[0..5] and scalars2 exactly as a0_adam_step_sync_wt leaves them — rides in the last weight-gradient launch (a launch of its own where that
 * is not the per-observation conv1 kernel).  Until a0_update_tail has run the gradients of the planned segments are not final and their slabs must stay untouched. */
typedef struct a0_update_tail_plan { a0_reduce_seg seg[8]; int n; } a0_update_tail_plan;
int a0_net_encoder_wgrad_tail(const a0_net* net, const a0_encoder_weights* w, const a0_frames_arg* frames, int B, const float* act1, const float* act2,
                              const float* d3, const float* d2, const float* d1, float* g1, float* g2, float* g3, float* slabs, const a0_pending_reduce* pend,
                              a0_update_tail_plan* plan, int* state, float* scalars2, double lr, double beta1, double beta2, int target_update_freq, void* stream);

/* nn.Linear / NoisyLinear forward+backward (model.py:54-62,112-114): Y = act(X W^T + b), W [N][K] row-major.
 * N, K, ldx multiples of 4.  scratch sizes from the *_scratch functions (0 => may pass NULL). */
long long a0_dense_fwd_scratch(int R, int N, int K);
int a0_dense_fwd(const float* X, int ldx, const float* W, const float* b, float* Y, int R, int N, int K, int relu,
                 float* scratch, void* stream);
/* a0_dense_fwd with the split-K count given by the caller (1 = unsplit; scratch: splits * R * N floats when splits > 1).  A grouped actor step runs every group's layers
 * with the count of the full batch's launch (a0_dense_fwd_splits), so each row's sum is formed in the same order as in a one-group step. */
int a0_dense_fwd_splits(int R, int N, int K);
int a0_dense_fwd_n(const float* X, int ldx, const float* W, const float* b, float* Y, int R, int N, int K, int relu, int splits, float* scratch, void* stream);
int a0_dense_dgrad(const float* dY, const float* W, const float* act_mask, float* dX, int R, int N, int K, void* stream);
/* (round 4) a0_dense_dgrad with the ReLU mask X and the unsplit a0_dense_wgrad of ONE layer (loss.backward() through first_dense, agent.py:153-155) as one launch: the two
 * GEMMs have the same number of 64 x 64 tiles (R == N) and together keep the chip's workgroup slots filled; bit-identical to the two calls.  Shapes: _ok (fc1 of a 512-row batch) */
int a0_dense_dgrad_wgrad_ok(int R, int N, int K);
int a0_dense_dgrad_wgrad_ok2(int R, int N, int K);      /* (round 5) _ok, or a SMALL layer whose two gradients together fit one round of 64 x 64 tiles (a distributional head at a
                                                         * 512-row batch): side by side in one launch; the weight gradient is then an unsplit sum (a0_dense_wgrad's up to the association order) */
int a0_dense_dgrad_wgrad(const float* dY, const float* W, const float* X, int ldx, float* dX, float* grad_w_b, int R, int N, int K, void* stream);
/* (round 5) the same launch also carries the NEXT layer's weight gradient: dW2 = dY2^T X2 (+ bias row sums) into grad2 [N2 x K2 | N2], an unsplit sum over the R rows
 * (what a0_dense_wgrad(dY2, X2, ldx2, grad2, R, N2, K2) computes, up to the association order of the fp32 additions).  fc1's two gradients and the head's weight gradient
 * of a learner's backward pass (agent.py:153-155) are independent once the loss kernel has written dY and dY2.  N2 x K2 must have no more 128 x 64 tiles than R x K. */
int a0_dense_dgrad_wgrad2_ok(int R, int N, int K, int N2, int K2);      /* where the library's own learners use it: heads of at most eight such tiles (scalar heads) */
int a0_dense_dgrad_wgrad2(const float* dY, const float* W, const float* X, int ldx, float* dX, float* grad, int R, int N, int K,
                          const float* dY2, const float* X2, int ldx2, float* grad2, int N2, int K2, void* stream);
long long a0_dense_wgrad_scratch(int R, int N, int K);
int a0_dense_wgrad(const float* dY, const float* X, int ldx, float* grad_w_b, int R, int N, int K, float* slabs, void* stream);
/* n <= 4 dense weight gradients (the head's and fc1's, + the cosine embedding's) whose slab reductions share one launch; layer i reduces in
 * slabs + slab_off[i] (a0_dense_wgrad_scratch floats each, disjoint).  The pointer / shape arrays are host arrays. */
int a0_dense_wgrad_multi(int n, const float* const* dY, const float* const* X, const int* ldx, float* const* grad_w_b, const int* R, const int* N, const int* K,
                         float* slabs, const long long* slab_off, a0_pending_reduce* pend, void* stream);
/* (round 4) pend != NULL: the slab reductions are NOT launched but appended to *pend (set pend->n = 0 before the first call); the next
 * a0_net_encoder_wgrad(..., pend, ...) adds them to its own reduction launch — one launch less per update.  Until then the gradients of the deferred layers are
 * not final and their slabs (slabs + slab_off[i]) must stay untouched: give the encoder a slab region of its own. */

/* Y[r] = act(X[r] W^T + b) * M[r / group]: the IQN / FQF embedding relu(cosine_emb(...)) times the state features (model.py:244-247) in the
 * GEMM's epilogue, for passes that are not differentiated; only when a0_dense_fwd_scratch(R, N, K) == 0 (unsplit GEMM) */
int a0_dense_fwd_mul(const float* X, int ldx, const float* W, const float* b, const float* M, int group, float* Y, int R, int N, int K, int relu, void* stream);

/* the same for a pass that IS differentiated: E[r] = act(X[r] W^T + b) is kept for a0_hadamard_bwd and Y[r] = E[r] * M[r / group] is written in
 * the same launch (replaces a0_dense_fwd + a0_hadamard_fwd on model.py:244-247).  Only for the shapes of the short-reduction kernel
 * (K = 64, R >= 256, N >= 64): a0_dense_fwd_mul_keep_ok returns 1 for them, a0_dense_fwd_mul_keep fails with A0_EINVAL otherwise */
int a0_dense_fwd_mul_keep_ok(int R, int N, int K, int ldx);
int a0_dense_fwd_mul_keep(const float* X, int ldx, const float* W, const float* b, const float* M, int group, float* E, float* Y, int R, int N, int K, int relu, void* stream);

/* a0_dense_fwd without its slab reduction: slab z of [R][N] at stride R*N holds X W^T over the z-th k range; the consumer kernel sums the
 * a0_dense_fwd_partial_slabs(R, N, K) slabs in order, adds the bias and applies the activation (a0_dqn_head_loss_slabs) */
int a0_dense_fwd_partial_slabs(int R, int N, int K);
int a0_dense_fwd_partial(const float* X, int ldx, const float* W, int R, int N, int K, float* slabs, void* stream);
/* the same with the slab count given by the caller (slabs: splits * R * N floats) — see a0_dense_fwd_n */
int a0_dense_fwd_partial_n(const float* X, int ldx, const float* W, int R, int N, int K, int splits, float* slabs, void* stream);
/* (round 4) n = 2 or 3 passes of ONE layer shape with their own inputs, weights and slab buffers — the target / online fc1 passes of an update (agent.py:176-181) — in one
 * launch: fewer, deeper splits per pass (a0_dense_fwd_partial_multi_slabs of them; the partial sums associate differently from a0_dense_fwd_partial's) because the passes
 * fill the chip together.  Host arrays of device pointers; shapes: a0_dense_fwd_partial_multi_ok */
int a0_dense_fwd_partial_multi_ok(int n, int R, int N, int K);
int a0_dense_fwd_partial_multi_slabs(int n, int R, int N, int K);
int a0_dense_fwd_partial_multi(int n, const float* const* X, int ldx, const float* const* W, int R, int N, int K, float* const* slabs, const long long* slab_stride,
                               void* stream);      /* slab_stride (optional, per pass): floats between consecutive slabs, default R * N — passes may share one [splits][2R][N] buffer */
/* The reduction a0_dense_fwd performs behind its split-K GEMM, for up to four layers of the same width N in ONE launch: out[i] = act(sum_z slabs[i][z] + bias[i])
 * (slabs added in slab order: bit-identical to a0_dense_fwd).  The three fc1 passes of a distributional update (agent.py:219-231: online on s, online on s',
 * target on s') finish in one launch instead of three.  Host arrays of n entries; every buffer 16-byte aligned, slab strides multiples of 4 floats. */
int a0_reduce_bias_act_multi(int n, const float* const* slabs, const long long* slab_stride, const int* nslab, const float* const* bias, float* const* out,
                             const int* rows, int N, int relu, void* stream);

/* measurement hook for bench.py: HIP events around every launch of the GEMM tagged `tag` (1 conv1 fwd, 2 conv2 fwd, 3 conv3 fwd,
 * 4 dense fwd, 5 dense dgrad, 6 dense wgrad, 7/8 conv3 wgrad/dgrad, 9/10 conv2 wgrad/dgrad, 11 conv1 wgrad, 12 fused encoder, 13 fused encoder dgrad,
 * 14 the actor step's tail + env step + encoder kernel of a0_actor_qhead_env_step_enc), recorded on the
 * launch stream.  a0_probe_end writes host_out3 = {launches, total ms, total algorithmic FLOP (2*M*N*K)}. */
int a0_probe_begin(int tag, int max_launches);
int a0_probe_end(double* host_out3);

/* Named host-side ranges for rocprofv3 --marker-trace (roctx; SURVEY.md §5 — the reference has wall-clock timing only, trainer.py:176-180).  Active only when the
 * process was started with A0_ROCTX=1 and librocprofiler-sdk-roctx.so can be loaded (a0_trace_enabled); otherwise every call is a branch.  The library's own
 * handles open ranges `rollout` (a0_actor_rollout), `update` (a0_learner_update), `exchange` (the gradient all-reduce's enqueue), `sample` (a0_rbuf_sample*);
 * a host adds its own around them (the Python Trainer: `iteration`, `update_block`).  a0_trace_rank(r) prefixes every name with "r<r>:" (r < 0: no prefix).
 * A range brackets the ENQUEUE on the host; the kernels it launched are in the kernel trace of the same run. */
int a0_trace_enabled(void);
int a0_trace_rank(int rank);
int a0_trace_push(const char* name);
int a0_trace_pop(void);

/* Weights as term planes (round 6): a0_split_planes writes the three exact bf16 terms of W [N][K] (K % 4 == 0) into `planes` (a0_weight_planes_words(N, K) 32-bit words) once
 * per change of W; a0_dense_fwd_wplanes is a0_dense_fwd (model.py:112-114) for the shapes a0_dense_fwd_wplanes_ok accepts (unsplit, K % 32 == 0, R >= 2048, N >= 128) reading them —
 * the same products, the same result bit for bit, without the weight operand's split instructions in the GEMM. */
long long a0_weight_planes_words(int N, int K);
int a0_split_planes(const float* W, unsigned int* planes, int N, int K, void* stream);
int a0_dense_fwd_wplanes_ok(int R, int N, int K);
int a0_dense_fwd_wplanes(const float* X, int ldx, const unsigned int* Wplanes, const float* b, float* Y, int R, int N, int K, int relu, void* stream);

/* The actor's per-step fc1 GEMM as a kernel of its own (actor_fc1.hip): a0_actor_fc1_n writes exactly the split-K slabs a0_dense_fwd_partial_n(X, ldx, W, R, N, K, splits,
 * slabs) writes — same k ranges, same products in the same order: the same bits — for the shapes a0_actor_fc1_ok accepts (N = 512, K % 32 == 0, 1 <= R <= 256, the
 * six-product split-operand GEMM), reading W as bf16 term planes in MFMA-fragment order: a0_actor_fc1_planes writes them (a0_actor_fc1_planes_words(N, K) 32-bit words;
 * N % 32 == 0, K % 16 == 0) once per change of W.  splits = a0_dense_fwd_partial_slabs(R, N, K): the scalar-head actors' slabs (a0_actor_qhead*).
 * a0_actor_fc1_dense: a0_dense_fwd(X, ldx, W, b, Y, R, N, K, relu, scratch) — the c51 / qr actors' fc1 — for the shapes a0_actor_fc1_dense_ok accepts (those of
 * a0_actor_fc1_ok that a0_dense_fwd runs split): the same slabs into `scratch`, the same reduction launch behind them, the same Y bit for bit. */
long long a0_actor_fc1_planes_words(int N, int K);
int a0_actor_fc1_planes(const float* W, unsigned int* planes, int N, int K, void* stream);
int a0_actor_fc1_ok(int R, int N, int K);
int a0_actor_fc1_dense_ok(int R, int N, int K);
int a0_actor_fc1_dense(const float* X, int ldx, const unsigned int* planes, const float* b, float* Y, int R, int N, int K, int relu, float* scratch, void* stream);
int a0_actor_fc1_n(const float* X, int ldx, const unsigned int* planes, int R, int N, int K, int splits, float* slabs, void* stream);

/* Matrix pipe used by every fp32-operand GEMM above (dense layers, conv2/conv3 weight gradients, unfused conv layers):
 * 1 (default) = bf16 MFMA with both operands split exactly into three bf16 terms, nine products, fp32 accumulation (igemm_x9.h);
 * 0 = fp32 MFMA fmaf chain (igemm.h).  Same results up to the association order of the fp32 additions.  Returns the previous mode;
 * mode < 0 only queries.  Process-wide, not a per-stream setting: change it between launches, never during graph capture. */
int a0_gemm_mode(int mode);

/* Cross products the split-operand kernels form per multiply (the x9 GEMM family, the fused encoder's conv2 / conv3 and their data gradients, the fused conv2 / conv3
 * weight gradient): with a = a0 + a1 + a2, b = b0 + b1 + b2 (exact bf16 terms, |a1| <= 2^-8 |a|, |a2| <= 2^-16 |a|)
 *   9 = all of them: every partial product of the fp32 fmaf chain, exactly (the strict mode);
 *   6 = those with i + j <= 2 (default): a1*b2, a2*b1, a2*b2 — each below 2^-24 of a*b, below the rounding the fp32 chain applies to every partial sum — are not
 *       formed; against fp64 its rms error is within 0.6 % of the nine-product result's and 0.88 - 1.38 x the sequential fp32 fmaf chain's, with a small
 *       negative bias that grows with the reduction length (profiles/r06_x6_accuracy.txt).
 * n = 6 or 9 sets it, anything else only queries; returns the previous value.  Environment: A0_X9_PRODUCTS=9.  Process-wide: change it between launches, never
 * during graph capture (captured graphs keep the kernels they were captured with).  conv1 (bytes x three weight terms) always forms all three. */
int a0_x9_products(int n);

/* ---------------------------------------------------------------- heads and losses */
/* dueling combine (model.py:127-130,168-172,228-231): raw [R][ld] = [A*T advantages | T values | pad] -> q [R][A][T] */
int a0_dueling_fwd(const float* raw, int ld, float* q, int R, int A, int T, int dueling, void* stream);
int a0_dueling_bwd(const float* dq, float* draw, int ld, int R, int A, int T, int dueling, void* stream);

/* head.qval + argmax (model.py:133,176-177,190-192,253-257,280-284; agent.py:32,177-180,224-227,277-280).
 * x(b,a,t) = x[b*sb + a*sa + t*st]; mode 0 identity, 1 mean over t, 2 C51 expectation (aux = atoms[T]),
 * 3 FQF sum (tau[t+1]-tau[t]) x (aux = taus [B][T+1]).  Outputs optional. */
int a0_select_action(const float* x, long long sb, long long sa, long long st, int B, int A, int T, int mode,
                     const float* aux, int* a_star, float* qsel, float* qmax, void* stream);
/* Actor.act's tail for distributional heads (c51: mode 2 with atoms [T]; qr: mode 1) in one launch: head slabs (a0_dense_fwd_partial) ->
 * slab sum + bias -> dueling combine -> expectation -> first-max argmax -> epsilon-greedy draw from the actor's Philox streams.  Same
 * arithmetic as a0_dense_fwd's reduction + a0_dueling_fwd + a0_select_action + a0_actor_egreedy_rng. */
int a0_actor_dist_tail(const float* slabs, long long slab_stride, int nslab, const float* bias, int ld, int A, int T, int dueling, int mode,
                       const float* atoms, int E, unsigned long long seed, unsigned int stream_a, unsigned int stream_u, unsigned long long off_a,
                       unsigned long long off_u, float eps, const long long* ctrl, const float* eps_ptr, int* action, float* qmax, void* stream);
/* the quantile networks' tail (iqn: mode 1; fqf: mode 3 with taus [E][T + 1]) without the env step: a0_actor_quantile_tail_env_step's arguments up to `qmax` — for actor
 * steps on host environments and test rollouts.  Same arithmetic, hence the same action and qmax, as the merged kernel and as a0_reduce_bias_act + a0_dueling_fwd +
 * a0_select_action + a0_actor_egreedy_rng. */
int a0_actor_quantile_tail(const float* slabs, long long slab_stride, int nslab, const float* bias, int ld, int A, int T, int dueling, int mode,
                           const float* taus, int E, unsigned long long seed, unsigned int stream_a, unsigned int stream_u, unsigned long long off_a,
                           unsigned long long off_u, float eps, const long long* ctrl, const float* eps_ptr, int* action, float* qmax, void* stream);
/* a0_actor_dist_tail + a0_env_synth_step_commit in ONE launch (a workgroup per env; the distributional counterpart of a0_actor_qhead_env_step):
 * arguments of a0_actor_dist_tail, then those of a0_env_synth_step_commit (the action is taken from, and written to, `action`). */
int a0_actor_dist_tail_env_step(const float* slabs, long long slab_stride, int nslab, const float* bias, int ld, int A, int T, int dueling, int mode,
                                const float* atoms, int E, unsigned long long seed, unsigned int stream_a, unsigned int stream_u, unsigned long long off_a,
                                unsigned long long off_u, float eps, const long long* ctrl, const float* eps_ptr, int* action, float* qmax,
                                unsigned long long env_seed, unsigned int rank, unsigned int g, const uint8_t* obs_in, uint8_t* obs_out, float* ep_ret,
                                float* final_mask, float* final_ret, int n, long long steps, double gamma, int* ring_act, float* ring_rew, float* ring_done,
                                const uint8_t* obs0, uint8_t* frames, long long cap, long long start_slot, int* r_act, float* r_rew, float* r_done, int task, void* stream);

/* the quantile networks' counterpart (iqn: mode 1, mean over the T = K sampled quantiles; fqf: mode 3, sum over the T = F fractions weighted by their widths,
 * taus [E][T + 1]): `slabs` are the split-K slabs [nslab][E * T][ld] of the head GEMM over (env, quantile) rows (a0_dense_fwd_partial), columns = actions
 * (+ the dueling value); replaces a0_reduce_bias_act + a0_dueling_fwd + a0_select_action + a0_actor_egreedy_rng + a0_env_synth_step_commit of one actor
 * step (reference agent.py:25-39 with model.py:253-257 / 280-284 behind it, and agent.py:44-90's per-step work), same arithmetic statement for statement */
int a0_actor_quantile_tail_env_step(const float* slabs, long long slab_stride, int nslab, const float* bias, int ld, int A, int T, int dueling, int mode,
                                    const float* taus, int E, unsigned long long seed, unsigned int stream_a, unsigned int stream_u, unsigned long long off_a,
                                    unsigned long long off_u, float eps, const long long* ctrl, const float* eps_ptr, int* action, float* qmax,
                                    unsigned long long env_seed, unsigned int rank, unsigned int g, const uint8_t* obs_in, uint8_t* obs_out, float* ep_ret,
                                    float* final_mask, float* final_ret, int n, long long steps, double gamma, int* ring_act, float* ring_rew, float* ring_done,
                                    const uint8_t* obs0, uint8_t* frames, long long cap, long long start_slot, int* r_act, float* r_rew, float* r_done, int task, void* stream);

/* DQNLearner.train_step (agent.py:173-190): loss [B], dq [B][A] = d(sum_b w_b loss_b)/dq */
int a0_loss_dqn(const float* q, const float* q_next, int A, const int* act, const int* a_star, const float* rew,
                const float* done, const float* wgt, float gamma_n, int B, float* loss, float* dq, int* nan_flag, void* stream);
/* DQNLearner.train_step (agent.py:173-190) from the fc1 activations on, one launch: q heads (online on h(s), target on h'(s'), online on
 * h(s') when h_sel != NULL = double-Q), dueling combine (model.py:123-131), argmax, smooth-L1 loss, and the gradient w.r.t. the raw head
 * outputs draw [B][ld] (dueling backward applied).  W_* [A(+1)][512] + b_*; q_on_out [B][A] (q_tg_out optional) for inspection. */
int a0_dqn_head_loss(const float* h_on, const float* h_tg, const float* h_sel, const float* W_on, const float* b_on, const float* W_tg,
                     const float* b_tg, int A, int dueling, int ld, const int* act, const float* rew, const float* done, const float* wgt,
                     float gamma_n, int B, float* loss, float* q_on_out, float* q_tg_out, float* draw, int* nan_flag, void* stream);
/* a0_dqn_head_loss that also finishes the three fc1 layers from their split-K slabs (a0_dense_fwd_partial): slab sum in order + bias + ReLU,
 * bit-identical to a0_dense_fwd; writes the online activations h(s) [B][512] for the backward pass.  slabs_sel = NULL without double-Q.
 * dh_out (optional, [B][512]): the gradient w.r.t. h(s), i.e. draw times the online head's rows masked by h > 0 — what a0_dense_dgrad would
 * compute from draw (the head's backward-data pass, agent.py:153-155), produced here where all of its operands already are. */
int a0_dqn_head_loss_slabs(const float* slabs_on, const float* slabs_tg, const float* slabs_sel, long long slab_stride, int nslab, const float* b1_on,
                           const float* b1_tg, float* h_on_out, const float* W_on, const float* b_on, const float* W_tg, const float* b_tg, int A,
                           int dueling, int ld, const int* act, const float* rew, const float* done, const float* wgt, float gamma_n, int B, float* loss,
                           float* q_on_out, float* q_tg_out, float* draw, int* nan_flag, float* dh_out, void* stream);

/* MDQNLearner.train_step (agent.py:194-215): q_next = target(next_obs), q_cur_tgt = target(obs), both [B][A] */
int a0_loss_mdqn(const float* q, const float* q_next, const float* q_cur_tgt, int A, const int* act, const float* rew, const float* done,
                 const float* wgt, float gamma_n, float tau, float lo, int B, float* loss, float* dq, int* nan_flag, void* stream);
/* (round 5) MDQNLearner.train_step (agent.py:193-215) from the fc1 GEMMs' split-K slabs on, one launch — a0_dqn_head_loss_slabs with the Munchausen target: slabs_cur are
 * the TARGET network's fc1 slabs on the CURRENT observation (agent.py:202-204; finished with the target's fc1 bias, evaluated with the target's head), tau / lo as in
 * a0_loss_mdqn.  q_cur_out (optional, [B][A]) receives target(obs).  Given the q values it writes, loss and draw equal a0_loss_mdqn + a0_dueling_bwd bit for bit. */
int a0_mdqn_head_loss_slabs(const float* slabs_on, const float* slabs_tg, const float* slabs_cur, long long slab_stride, int nslab, const float* b1_on,
                            const float* b1_tg, float* h_on_out, const float* W_on, const float* b_on, const float* W_tg, const float* b_tg, int A,
                            int dueling, int ld, const int* act, const float* rew, const float* done, const float* wgt, float gamma_n, float tau, float lo,
                            int B, float* loss, float* q_on_out, float* q_tg_out, float* q_cur_out, float* draw, int* nan_flag, float* dh_out, void* stream);
/* C51Learner.train_step (agent.py:219-269) from the head GEMMs' split-K slabs on, one launch: slab sums + bias (a0_dense_fwd's reduction), dueling combine per
 * atom (model.py:163-177), greedy next action from the expectation under softmax (agent.py:225-231), projection of the target distribution and cross entropy
 * (a0_loss_c51), d loss / d logits carried back through the dueling combine into `draw` [B][ld] — the gradient w.r.t. the online head GEMM's output on s.
 * slabs_on [nslab_on][rows_on][ld]: the ONLINE head over rows [0, B) = s and, under double-Q, rows [sel_off, sel_off + B) = s' (one GEMM over both, they share
 * the weights); sel_off < 0: no double-Q, the target's own expectation selects.  slabs_tg [nslab_tg][B][ld]: the target head on s'.  Optional outputs:
 * q_on_out / q_tg_out [B][A][T] (the combined logits), m_out [B][T] (projected target), a_star_out [B].  Same arithmetic, statement for statement, as
 * a0_dense_fwd's reduction + a0_dueling_fwd + a0_select_action + a0_loss_c51 + a0_dueling_bwd. */
int a0_c51_head_loss_slabs(const float* slabs_on, long long stride_on, int nslab_on, int rows_on, const float* slabs_tg, long long stride_tg, int nslab_tg,
                           int sel_off, const float* bias_on, const float* bias_tg, int ld, int A, int T, int dueling, const int* act, const float* rew,
                           const float* done, const float* wgt, const float* atoms, float gamma_n, float vmin, float vmax, int B, float* loss, float* draw,
                           float* q_on_out, float* q_tg_out, float* m_out, int* a_star_out, int* nan_flag, void* stream);
/* (round 5) QRLearner.train_step (agent.py:272-293 with huber_qr_loss 110-114) from the head GEMMs' split-K slabs on, one launch — the quantile-regression counterpart
 * of a0_c51_head_loss_slabs, same slab layout and the same meaning of rows_on / sel_off: slab sums + bias, dueling combine per quantile (model.py:163-177 through QRHead
 * 180-192), greedy next action from the mean over the T quantiles (agent.py:277-280), target quantiles r + gamma^n (1 - d) q'(a*), the T x T pairwise quantile Huber loss
 * with fractions taus [T] (the fixed midpoints, agent.py:274), d loss / d q carried back through the dueling combine into `draw` [B][ld].  One workgroup per sample, the
 * staged head outputs and the targets in LDS, the B x T x T pair tensor never materialised.  Optional outputs: q_on_out / q_tg_out [B][A][T], a_star_out [B].  Same
 * arithmetic, statement for statement, as a0_dense_fwd's reduction + a0_dueling_fwd + a0_select_action(mode 1) + a0_quantile_target + a0_loss_quantile_huber +
 * a0_dueling_bwd. */
int a0_qr_head_loss_slabs(const float* slabs_on, long long stride_on, int nslab_on, int rows_on, const float* slabs_tg, long long stride_tg, int nslab_tg,
                          int sel_off, const float* bias_on, const float* bias_tg, int ld, int A, int T, int dueling, const int* act, const float* rew,
                          const float* done, const float* wgt, const float* taus, float gamma_n, int B, float* loss, float* draw, float* q_on_out,
                          float* q_tg_out, int* a_star_out, int* nan_flag, void* stream);
/* C51Learner.train_step (agent.py:219-269): logits / tgt_logits [B][A][T]; m_out (optional) = projected target [B][T] */
int a0_loss_c51(const float* logits, const float* tgt_logits, int A, int T, const int* act, const int* a_star,
                const float* rew, const float* done, const float* wgt, const float* atoms, float gamma_n,
                float vmin, float vmax, int B, float* loss, float* dlogits, float* m_out, int* nan_flag, void* stream);
/* learner.c51.hl_gauss: the HL-Gauss classification target (Farebrother et al. 2024, "Stop Regressing: Training Value Functions via Classification for Scalable
 * Deep RL") in the projected distribution's place — a0_loss_c51's arguments plus sigma, one wave per sample, one lane per bin.  The atoms z_t = vmin + t Delta,
 * Delta = (vmax - vmin) / (T - 1), are bin CENTRES; the T + 1 edges are e_k = vmin - Delta / 2 + k Delta.  Per sample, in fp32 and in this order:
 * p' = softmax(tgt_logits at a_star), v' = (sum_t e'_t z_t) / (sum_t e'_t) with the wave sums of a0_select_action's mode 2, y = rew + (gamma_n (1 - done)) v',
 * y clamped to [vmin, vmax] by comparisons (a NaN reward stays NaN and reaches the loss and the flag).  Then in DOUBLE on the device, rounded to fp32 once:
 *   m_t = [Phi((e_{t+1} - y) / sigma) - Phi((e_t - y) / sigma)] / [Phi((e_T - y) / sigma) - Phi((e_0 - y) / sigma)],  Phi(u) = (1 + erf(u / sqrt 2)) / 2,
 * each lane evaluating its own two edges and the two outer ones (equal inputs give equal bytes), Delta the double quotient of the fp32 vmin and vmax.  sigma =
 * rho * Delta is handed over AS A DOUBLE and used as one; it must still be a normal fp32 number once rounded.  Loss and dlogits are a0_loss_c51's cross
 * entropy against m unchanged; m_out (optional) receives m.  A0_EINVAL, with the number named: a0_loss_c51's conditions, a sigma that is NaN, infinite, <= 0,
 * not a normal fp32 number, or above T * Delta (rho > num_atoms). */
int a0_loss_c51_hl_gauss(const float* logits, const float* tgt_logits, int A, int T, const int* act, const int* a_star,
                         const float* rew, const float* done, const float* wgt, const float* atoms, float gamma_n,
                         float vmin, float vmax, double sigma, int B, float* loss, float* dlogits, float* m_out, int* nan_flag, void* stream);
/* learner.c51.hl_gauss from the head GEMMs' split-K slabs on, one launch: a0_c51_head_loss_slabs with the Gaussian histogram of a0_loss_c51_hl_gauss in the
 * projection's place (no gather tables) — same slab layout, same meaning of rows_on / sel_off, same optional outputs; m_out receives the histogram.  The
 * expectation v' at a* is taken from the TARGET's logits also under double-Q, where a* is the online network's choice.  Given the q values it writes, loss, m_out
 * and a_star equal a0_loss_c51_hl_gauss and draw equals a0_dueling_bwd of its dlogits, bit for bit.  sigma and its refusals as there. */
int a0_c51_hl_gauss_head_loss_slabs(const float* slabs_on, long long stride_on, int nslab_on, int rows_on, const float* slabs_tg, long long stride_tg, int nslab_tg,
                                    int sel_off, const float* bias_on, const float* bias_tg, int ld, int A, int T, int dueling, const int* act, const float* rew,
                                    const float* done, const float* wgt, const float* atoms, float gamma_n, float vmin, float vmax, double sigma, int B, float* loss,
                                    float* draw, float* q_on_out, float* q_tg_out, float* m_out, int* a_star_out, int* nan_flag, void* stream);
/* quantile target r + gamma^n (1-d) q_next[a*] (agent.py:281-286,313-318,358-364) and BaseLearner.huber_qr_loss
 * (agent.py:110-114) with its gradient; strides let QR ([B][A][N]) and IQN/FQF ([B][N][A]) share the kernels. */
int a0_quantile_target(const float* q_next, long long sb, long long sj, long long sa, const int* a_star, const float* rew,
                       const float* done, float gamma_n, int B, int Nd, float* y, void* stream);
int a0_loss_quantile_huber(const float* q, long long sb, long long si, long long sa, const float* y, const float* taus,
                           long long tb, const int* act, const float* wgt, int B, int N, int Nd, float* loss, float* dq,
                           int* nan_flag, void* stream);
/* learner.iqn.munchausen: the Munchausen-IQN quantile targets (Vieillard, Pietquin, Geist 2020, section 5 and appendix B) in one launch.  q_next / q_cur: the TARGET
 * network's quantiles on s' / on s at the same Nd fractions, element (b, j, a) at b*sb + j*sj + a*sa of either (the strides of a0_quantile_target).  Per sample, with
 * Qm' / Qm the means over j (summed in j order), lp(x)_a = (x_a - max x) - tau log sum_k exp((x_k - max x) / tau) and pi' = softmax(Qm' / tau):
 *   y[b][j] = rew + alpha clamp(lp(Qm)[act], lo, 0) + gamma_n (1 - done) sum_a pi'_a (q_next(b, j, a) - lp(Qm')_a),  j < Nd.
 * The softmax is at temperature tau and the bonus is scaled by alpha, as in the paper: a0_loss_mdqn's temperature-1 softmax and its tau in alpha's place (quirk
 * Q17) are the reference's and stay that entry point's own.  No atomics: equal inputs give equal bytes.  A NaN or an infinity among a sample's inputs makes all Nd
 * targets of that sample NaN and no other's.  A0_EINVAL: a null pointer, B < 1, Nd outside [1, 8192], A outside [1, 32], tau <= 0, alpha < 0, lo > 0, or one of
 * the three not finite. */
int a0_miqn_target(const float* q_next, const float* q_cur, long long sb, long long sj, long long sa, const int* act, const float* rew, const float* done,
                   float gamma_n, float tau, float alpha, float lo, int B, int Nd, int A, float* y, void* stream);

/* IQN / FQF head pieces (model.py:235-251, 268-278; agent.py:371-387) */
int a0_cos_features(const float* taus, float* out, long long R, int D, void* stream);
/* (round 6) the actor's IQN step: taus[r] = element offset + r of the Philox uniform stream (== a0_rng_uniform / a0_rng_uniform_ctrl: ctrl, when given, adds
 * ctrl[ctrl_idx] to the offset) and out = a0_cos_features(taus) in ONE launch; the same bits as the two calls (model.py:238-241) */
int a0_tau_cos_features(unsigned long long seed, unsigned int stream, unsigned long long offset, const long long* ctrl, int ctrl_idx, float* taus, float* out,
                        long long R, int D, void* stream_h);
/* learner.iqn.risk: risk-sensitive IQN policies (Dabney et al. 2018, section 4).  The policy evaluates the network at tau' = beta(tau) instead of the uniform draw tau:
 *   A0_RISK_CVAR   eta tau                                                                  0 < eta <= 1          (the paper: 0.25, 0.1)
 *   A0_RISK_POW    eta >= 0: tau^(1 / (1 + |eta|)); eta < 0: 1 - (1 - tau)^(1 / (1 + |eta|))    finite, |eta| <= 64   (the paper: -2)
 *   A0_RISK_CPW    tau^eta / (tau^eta + (1 - tau)^eta)^(1 / eta)                            0 < eta <= 1          (the paper: 0.71)
 *   A0_RISK_WANG   Phi(Phi^-1(tau) + eta), beta(0) = 0                                      finite, |eta| <= 8    (the paper: 0.75, -0.75)
 * A0_RISK_NEUTRAL is the identity and ignores eta.  Arithmetic: tau is the fp32 draw k * 2^-24; cvar is ONE fp32 multiply by eta rounded to fp32 (numpy float32's
 * bits); the other three are formed in double from (double)tau and the double eta — pow(), normcdfinv(), Phi(u) = erfc(-u / sqrt 2) / 2 — and rounded to fp32 once,
 * so they lie within one fp32 spacing of the exact value.  tau = 0 gives 0 for every kind; a result above 1 becomes 1; a NaN stays a NaN.  One device function
 * states the formula for both entry points below.
 * a0_risk_distort: out[i] = beta(taus[i]), i < n, elementwise; out may equal taus; 16-byte loads and stores where both pointers are 16-byte aligned (the ragged
 * last chunk of n % 256 elements and unaligned buffers go element by element); neutral copies.  Equal inputs give equal bytes.
 * a0_tau_cos_features_risk: a0_tau_cos_features's arguments (the ctrl word included, so a captured rollout works) plus (kind, eta); draw, distortion and the D cosine
 * features stay ONE launch, taus receives tau', and the bytes are those of a0_rng_uniform(_ctrl) -> a0_risk_distort -> a0_cos_features.  The double-precision chain
 * runs once per fraction (one lane draws and distorts it and leaves it in LDS for the fraction's D cosine lanes), not once per (fraction, cosine) pair.
 * A0_EINVAL, under the entry point's name with the setting and the number named: a null pointer, n < 1 (R < 1, D < 1, a ctrl index outside the control block), a kind
 * that is none of the five, an eta outside the kind's range, NaN or infinite. */
#define A0_RISK_NEUTRAL 0
#define A0_RISK_CVAR 1
#define A0_RISK_POW 2
#define A0_RISK_CPW 3
#define A0_RISK_WANG 4
int a0_risk_distort(const float* taus, float* out, long long n, int kind, double eta, void* stream);
int a0_tau_cos_features_risk(unsigned long long seed, unsigned int stream, unsigned long long offset, const long long* ctrl, int ctrl_idx, float* taus, float* out,
                             long long R, int D, int kind, double eta, void* stream_h);
int a0_hadamard_fwd(const float* emb, const float* feat, float* x, int B, int n, int D, void* stream);
int a0_hadamard_bwd(const float* dx, const float* emb, const float* feat, float* demb, float* d3, int B, int n, int D, void* stream);
/* (round 6) a0_dense_dgrad(dY [R][N], W [N][K], no mask) + a0_hadamard_bwd in one launch for R = B * n rows, n = 32 or 64: dx = dY W is consumed in the GEMM's epilogue and never
 * reaches HBM.  demb [R][K] is bit-identical to the two calls'; d3 [R / n][K] sums a sample's n rows in another order (fp32 rounding).  Shapes: a0_dense_dgrad_hadamard_ok. */
int a0_dense_dgrad_hadamard_ok(int R, int N, int K, int n);
int a0_dense_dgrad_hadamard(const float* dY, const float* W, const float* emb, const float* feat, float* demb, float* d3, int R, int N, int K, int n, void* stream);
int a0_fqf_taus(const float* logits, int ld, float* taus, float* tau_hat, int B, int F, void* stream);
/* (round 6) a0_fqf_taus + a0_cos_features(tau_hat) -> cos_out [B * F][D] in one launch (the actor's FQF step); the same bits as the two calls */
int a0_fqf_taus_cos(const float* logits, int ld, float* taus, float* tau_hat, float* cos_out, int D, int B, int F, void* stream);
int a0_fqf_inner_taus(const float* taus, float* out, int B, int F, void* stream);
int a0_fqf_fraction_loss(const float* q, const float* qh, const float* taus, const int* act, const float* wgt, int B, int F, int A,
                         int ldl, float* loss, float* dlogits, const float* logits, void* stream);

/* ---------------------------------------------------------------- optimizer / target sync (agent.py:102-106,152-161,333-338) */
/* state: int[8] device block: [0] nan flag (set by losses) [1] update_steps [2] skipped [3] skip_now [4] sync_now [5] scratch of a0_adam_step_sync_wt (the new
 * count between its two launches; a0_net_encoder_wgrad_tail leaves the same word)
 * [6] calls of a0_adam_step_sync_wt with a loss ring (free-running: the ring slot of the next call is state[6] % ring_cap)
 * [7] update_steps at the last network reset (written by a0_net_reset alone; 0 in every run without learner.net_reset_freq).  Every Adam form derives its bias
 *     corrections from t = max(1, update_steps - state[7]): with the word at 0 that is the update count, as it always was.
 * Every Adam form below takes the step's decisions — NaN skip, new count, the two bias-correction scalars, "sync now" — from ONE device function
 * (a0_step_decide, csrc/update_tail.h) and steps a parameter with one of TWO written-out element forms (a0_adam_wide / a0_adam_scalar, csrc/optim.hip): groups of
 * four that move as 16 bytes take the first, everything stepped element by element — all of a0_adam_step included — the second. */
int a0_adam_step(float* params, const float* grads, float* exp_avg, float* exp_avg_sq, long long n, int* state,
                 float* scalars2, double lr, double beta1, double beta2, double eps, int target_update_freq, void* stream);
/* a0_adam_step with the target copy of agent.py:160-161 folded into the same pass: when update_steps % target_update_freq == 0 after this
 * update, target[0, n_total) receives the new parameters (n_total >= n also covers blocks Adam does not own).  == a0_adam_step +
 * a0_target_sync(force = 0), two launches instead of three. */
int a0_adam_step_sync(float* params, const float* grads, float* exp_avg, float* exp_avg_sq, long long n, int* state, float* scalars2, double lr,
                      double beta1, double beta2, double eps, int target_update_freq, float* target, long long n_total, const float* extra_nan_flag,
                      void* stream);
/* The optimizer tail of a network whose convolutions run in the fused kernels, two launches instead of three: a0_adam_step_sync with the step's
 * bookkeeping (NaN skip, step count, bias corrections, "sync now": agent.py:152-161) derived inside the Adam kernel, then
 * a0_net_conv_wt_refresh_sync of the online copies `wt` (mirrored into `wt_target` on a sync step), which also commits the step count.
 * state[5] is scratch.  Same results as the two calls it replaces.  loss (optional, [loss_n]): the update's per-sample losses; their batch mean — the Trainer's
 * `loss` statistic, trainer.py:99,111-113, == a0_mean_rows — is written to loss_ring[state[6] % ring_cap] by the Adam launch itself (one launch per update less). */
int a0_adam_step_sync_wt(float* params, const float* grads, float* exp_avg, float* exp_avg_sq, long long n, int* state, float* scalars2, double lr,
                         double beta1, double beta2, double eps, int target_update_freq, float* target, long long n_total, const float* extra_nan_flag,
                         const a0_encoder_weights* w, int C, float* wt, float* wt_target, const float* loss, int loss_n, float* loss_ring, int ring_cap, void* stream);
/* Global gradient-norm clipping in front of Adam (learner.clip_grad_norm; torch.nn.utils.clip_grad_norm_ with its defaults), two stages and ONE extra launch per update.
 * Stage 1, a0_grad_norm_partials: the sum of squares of grads[0, n) as A0_GRAD_NORM_PARTIALS doubles (squares and sums in double; a fixed split of the range that
 * depends on n alone, plain stores, unused partials zero: the same bits on every run).  grads 16-byte aligned: 16-byte loads; otherwise element by element.
 * Stage 2 rides in the Adam launch of the _clip entry points — the two above plus (partials, max_norm > 0, norm_ring, norm_ring_cap): every workgroup sums the partials
 * in the same order, rounds ||g|| = sqrt(sum) to fp32, forms c = max_norm / (||g|| + 1e-6f), coef = c < 1 ? c : 1 in fp32 and steps on g[i] * coef — bit for bit the
 * unclipped entry point on a buffer holding g * coef.  The pre-clip norm is written to norm_ring[state[6] % norm_ring_cap] (the slot of the same update's loss mean;
 * a0_adam_step_sync_clip does not advance state[6]), on NaN-skipped steps too. */
#define A0_GRAD_NORM_PARTIALS 256
int a0_grad_norm_partials(const float* grads, long long n, double* partials, void* stream);
/* Decoupled weight decay in front of Adam (learner.weight_decay; torch.optim.AdamW's p <- p * (1 - lr * lambda)), ONE launch of A0_GRAD_NORM_PARTIALS workgroups,
 * which decides for itself: the update counts as skipped when state[0] != 0 (the NaN flag, still up: issue this IN FRONT of the update's Adam form — a0_adam_step_sync
 * or a0_adam_step_sync_wt, with or without _clip; not in front of a0_update_tail, whose bookkeeping has lowered the flag a launch earlier) or when extra_nan_flag
 * (optional, as the Adam forms take it) is nonzero.  Not skipped: every params[i], i in [0, n), becomes fl32(p - fl32(c32 * p)), c32 = (float)c — one rounded
 * product, one rounded subtraction, no contraction — so that the Adam form behind steps, and files in the weight copies and the target, the shrunk values.  Skipped:
 * no parameter is stored.  Either way partials[b] (A0_GRAD_NORM_PARTIALS doubles, 8-byte aligned, a0_grad_norm_partials' split of the range, plain stores, 0 for an
 * empty range) receives the sum of squares, in double, of the values workgroup b READ: sqrt of their sum is the parameter norm in front of the decay.  params 16-byte
 * aligned: 16-byte loads and stores; otherwise element by element.  c = lr * lambda formed in double by the caller; A0_EINVAL unless 2^-24 <= c32 < 1 (a smaller
 * coefficient moves no fp32 value).  No state word is written, no scratch, no atomics. */
int a0_weight_decay(float* params, long long n, double c, const int* state, const float* extra_nan_flag, double* partials, void* stream);
int a0_adam_step_sync_clip(float* params, const float* grads, float* exp_avg, float* exp_avg_sq, long long n, int* state, float* scalars2, double lr,
                           double beta1, double beta2, double eps, int target_update_freq, float* target, long long n_total, const float* extra_nan_flag,
                           const double* partials, float max_norm, float* norm_ring, int norm_ring_cap, void* stream);
int a0_adam_step_sync_wt_clip(float* params, const float* grads, float* exp_avg, float* exp_avg_sq, long long n, int* state, float* scalars2, double lr,
                              double beta1, double beta2, double eps, int target_update_freq, float* target, long long n_total, const float* extra_nan_flag,
                              const a0_encoder_weights* w, int C, float* wt, float* wt_target, const float* loss, int loss_n, float* loss_ring, int ring_cap,
                              const double* partials, float max_norm, float* norm_ring, int norm_ring_cap, void* stream);
/* ONE launch for what a0_net_encoder_wgrad's reduction launch and the two launches of a0_adam_step_sync_wt do, bit for bit: every planned slab sum is formed in
 * a0_net_encoder_wgrad's order by the workgroup that owns those parameters, written to grads and stepped on at once; every other parameter takes the Adam path of
 * a0_adam_step_sync; target copy on a sync step and loss-mean ring slot as in a0_adam_step_sync_wt; and the lane that holds a new convolution weight writes it to every
 * place of `wt` (and, on a sync step, of `wt_target`) that a0_net_conv_wt_refresh would copy it to.  Call it behind a0_net_encoder_wgrad_tail, which has already derived
 * the step's decisions into state / scalars2; here state[3], state[4] and the scalars are only read (state[6], the ring counter, advances as before).
 * plan->seg[k].out must lie inside grads[0, n_total), the segments must not overlap; w->w1 / w2 / w3 must lie inside params; `wt` must hold the copies of the weights
 * as they are before the call (a NaN-skipped step leaves it alone).  No data-parallel flag and no clipping: those paths keep the three-launch chain. */
int a0_update_tail(float* params, float* grads, float* exp_avg, float* exp_avg_sq, long long n, int* state, const float* scalars2, double beta1, double beta2, double eps,
                   float* target, long long n_total, const a0_update_tail_plan* plan, const a0_encoder_weights* w, int C, float* wt, float* wt_target,
                   const float* loss, int loss_n, float* loss_ring, int ring_cap, void* stream);
/* Soft (Polyak) target updates (learner.target_tau): target[i] <- fmaf(tau32, fl32(online[i] - target[i]), target[i]) over [0, n_total), tau32 = tau rounded to fp32 once
 * (0 < tau < 1; tau >= 1 is the hard copy a0_target_sync gives and is refused) — one rounded subtraction and one fused multiply-add, the same bits on every path.
 * ONE launch, which decides for itself: it blends when force != 0, or when target_update_freq > 0 and state[1] % target_update_freq == 0, and returns at once
 * otherwise (state may be NULL with force).  Issue it behind an update's Adam form — a0_adam_step_sync, a0_adam_step_sync_wt (with or without _clip) or
 * a0_net_encoder_wgrad_tail + a0_update_tail — called with target_update_freq = 0: those then never hard-copy, state[4] stays 0 while tau is on, and state[1]
 * holds the new step count by the time this launch reads it; like the hard copy, the blend also follows a NaN-skipped update whose count is a multiple of the period.
 * Buffers 16-byte aligned: 16 bytes per lane and a scalar tail of n_total % 4 floats; 4-byte aligned: element by element.  wt_target (optional, 16-byte aligned,
 * a0_net_conv_wt_floats(C) floats) with w_target, the target's convolution weights inside target[0, n_total): after a blend wt_target holds the bytes
 * a0_net_conv_wt_refresh would build from the blended target; when the launch does not blend it is not touched.  No scratch, no atomics. */
int a0_target_blend(float* target, const float* online, long long n_total, double tau, const int* state, int target_update_freq, int force,
                    const a0_encoder_weights* w_target, int C, float* wt_target, void* stream);
/* Periodic shrink-and-perturb network resets (learner.net_reset_freq / learner.net_reset_shrink; Nikishin et al. 2022, D'Oro et al. 2023, Schwarzer et al. 2023).
 * ONE launch, which decides for itself: it resets when force != 0 (reset number k = k_host >= 0), or when state[3] == 0 (the update was not NaN-skipped), freq > 0,
 * state[1] > 0 and state[1] % freq == 0 (k = state[1] / freq); otherwise every workgroup returns after reading those two words (state may be NULL with force).
 * Issue it behind an update's Adam form — any of those above — and behind a0_target_blend where that is used.  A reset:
 *  - walks the rule table `segs` (n_segs <= A0_NET_RESET_MAX_SEGS, ascending, disjoint, inside [0, n_adam); passed to the kernel by value).  Element i of a segment
 *    gets the fresh value phi: kind CONST: `scale`; NORMAL: what a0_rng_normal(seed32, 8, k * n_total + i, scale, ..) writes for that position; UNIFORM:
 *    scale * (2 u - 1), u what a0_rng_uniform(seed32, 8, k * n_total + i, ..) writes (2 u - 1 is exact, one rounded multiply).  seed32 = seed & 0xFFFFFFFF.  A draw is a
 *    function of (seed32, k, i) alone: nothing advances, nothing new belongs in a snapshot.
 *  - keep == 0: params[i] <- phi.  keep == 1: the segment keeps the share alpha (0 <= alpha <= 1, rounded to fp32 once): alpha == 1 leaves the element unread and
 *    unwritten and draws nothing, alpha == 0 is params[i] <- phi, anything else params[i] <- fmaf(alpha32, fl32(params[i] - phi), phi) (a0_target_blend's arithmetic).
 *    Elements of [0, n_total) outside every segment (the fqf fraction net behind n_adam) are left alone.
 *  - exp_avg and exp_avg_sq <- 0 over [0, n_adam); state[7] <- state[1], so that Adam's bias corrections restart at t = 1 with the next update (state != NULL).
 *  - target[i] <- params[i] over [0, n_total), the hard copy of construction time; with wt / wt_target (both or neither; 16-byte aligned, a0_net_conv_wt_floats(C)
 *    floats) and w, the ONLINE network's convolution weights inside params[0, n_total), the lane that holds a convolution weight files it in both copies: afterwards
 *    each holds the bytes a0_net_conv_wt_refresh builds from the new parameters.
 * All four buffers 16-byte aligned: 16 bytes per lane where four elements lie inside one segment, element by element at a boundary and in the tail of n_total % 4
 * floats; 4-byte aligned buffers: element by element.  No scratch, no LDS, no atomics. */
#define A0_NET_RESET_MAX_SEGS 32
enum { A0_NET_RESET_CONST = 0, A0_NET_RESET_NORMAL = 1, A0_NET_RESET_UNIFORM = 2 };
typedef struct a0_net_reset_seg {
    long long offset, count; /* [offset, offset + count) of the flat parameter buffer */
    int kind;                /* A0_NET_RESET_CONST / _NORMAL / _UNIFORM */
    float scale;             /* the constant, the standard deviation, the bound */
    int keep;                /* 1: the segment keeps the share alpha of its values (the encoder); 0: it is replaced */
} a0_net_reset_seg;
int a0_net_reset(float* params, float* target, float* exp_avg, float* exp_avg_sq, long long n_adam, long long n_total, const a0_net_reset_seg* segs, int n_segs,
                 double alpha, unsigned long long seed, int* state, int freq, int force, long long k_host, const a0_encoder_weights* w, int C, float* wt,
                 float* wt_target, void* stream);
/* Dormant neurons and ReDo recycling (learner.redo_freq / learner.redo_tau / learner.redo_recycle; Sokar et al. 2023, "The Dormant Neuron Phenomenon in Deep RL").
 * The 672 hidden neurons of the network, in this order: conv1's 32 output channels [0, 32), conv2's 64 [32, 96), conv3's 64 [96, 160), fc1's 512 units [160, 672).
 * Both entry points decide for themselves, like a0_net_reset: they act when force != 0, or when state[3] == 0 (the update was not NaN-skipped), freq > 0, state[1] > 0
 * and state[1] % freq == 0; otherwise every workgroup returns after reading those two words (state may be NULL with force).  Issue them behind an update's Adam form
 * and behind a0_target_blend, in front of a0_net_reset.
 *
 * a0_redo_score (two launches: partial sums, finish): act1 [rows1][32], act2 [rows2][64], act3 [rows3][64], fc1 [rows4][512], fp32, channel-fastest, 16-byte aligned,
 * rows >= 1 — the activations of the online, differentiated pass (A0_PEEK_ACT1 / 2 / 3 / FC1).  For layer l with n_l neurons: m_i = (1 / rows) sum_r |X[r][i]|,
 * s_i = m_i / ((1 / n_l) sum_j m_j), a layer whose mean is 0 has s_i = 0; neuron i is dormant iff s_i <= tau (0 <= tau < 1), compared in double.  All sums are
 * accumulated in double in a fixed order: workgroup g of the (at most A0_REDO_PARTIALS) workgroups a layer's row count names owns a range of rows that depends on that count alone, its lanes' sums are added in
 * index order into partials[g][672] (plain stores, no atomics), and one workgroup adds the partials of a neuron in index order, in eight slices whose sums it then adds in index order.  partials: A0_REDO_PARTIALS * A0_REDO_NEURONS
 * doubles of scratch.  Outputs: scores float[672] (the double rounded once), mask int[672] (1 = dormant), counts int[8]: [0..3] dormant per layer, [4] their sum,
 * [5] state[1] of the evaluation (0 with a NULL state; the caller initialises it to -1 = "never evaluated"), [6], [7] spare and not written.
 *
 * a0_redo_recycle (one launch): for every neuron i of layer l with mask != 0,
 *  - incoming: row i of the layer's W block and bias i get the fresh value the rule table `segs` (a0_net_reset's table; `keep` is ignored: a recycled row is
 *    replaced, not shrunk) gives element e: kind CONST: `scale`; NORMAL / UNIFORM: what a0_rng_normal / a0_rng_uniform (as scale * (2 u - 1)) write at position
 *    k * n_total + e of Philox stream 9 of seed & 0xFFFFFFFF, k = state[1] / freq (k_host with force) — a function of (seed, k, e) alone;
 *  - outgoing: every weight of the next block that reads neuron i becomes 0.0f: conv1 -> conv2 columns with col % 32 == i, conv2 -> conv3 col % 64 == i,
 *    conv3 -> fc1 col % 64 == i in all 512 rows, fc1 -> head column i in all Npad rows (an element that is both ends at 0); the head's bias, the cosine embedding and
 *    everything behind n_adam are left alone;
 *  - exp_avg and exp_avg_sq of every touched element become 0; state is only read (Adam's bias correction is not restarted);
 *  - with wt (16-byte aligned, a0_net_conv_wt_floats(C) floats) and w, the ONLINE network's convolution weights inside params — the blocks `blocks` names — the lane
 *    that writes a convolution weight files it in wt: afterwards wt holds the bytes a0_net_conv_wt_refresh builds from the new parameters.
 * Every other byte is left unread or unwritten; the target network and its weight copy are not arguments.  `blocks`: the offsets of the blocks [W (N x K) | b (N)]
 * in the flat buffer (agent0_amd/deepq/layout.py), ascending: conv1 32 x K1, conv2 64 x 512, conv3 64 x 576, fc1 512 x feat, head Npad x 512.  Buffers 4-byte
 * aligned; element by element, stores only where an element is touched; the mask is read into LDS once per workgroup.  No scratch, no atomics. */
#define A0_REDO_NEURONS 672
#define A0_REDO_PARTIALS 512
typedef struct a0_redo_blocks {
    long long conv1, conv2, conv3, fc1, head; /* first element of each block in the flat parameter buffer */
    int K1, feat, Npad;                       /* conv1's row length C * 64, fc1's row length 64 * H3 * W3, the head's padded rows */
} a0_redo_blocks;
int a0_redo_score(const float* act1, long long rows1, const float* act2, long long rows2, const float* act3, long long rows3, const float* fc1, long long rows4,
                  double tau, const int* state, int freq, int force, double* partials, float* scores, int* mask, int* counts, void* stream);
int a0_redo_recycle(float* params, float* exp_avg, float* exp_avg_sq, long long n_adam, long long n_total, const a0_net_reset_seg* segs, int n_segs,
                    const a0_redo_blocks* blocks, const int* mask, unsigned long long seed, const int* state, int freq, int force, long long k_host,
                    const a0_encoder_weights* w, int C, float* wt, void* stream);
/* Feature rank (learner.rank_freq / learner.rank_delta): srank_delta of Kumar et al. 2021, "Implicit Under-Parameterization Inhibits Data-Efficient Deep RL", for the
 * fc1 activations of an update's differentiated pass — fc1 [rows][512], fp32, 16-byte aligned, rows >= 1: the buffer A0_PEEK_FC1 names, exactly what a0_redo_score is
 * given as its fourth layer.  Two launches that decide for themselves like a0_redo_score: they act when force != 0, or when state[3] == 0, freq > 0, state[1] > 0 and
 * state[1] % freq == 0; otherwise every workgroup returns after reading those two words (state may be NULL with force).  Issue them behind an update's Adam form and
 * a0_target_blend, in front of a0_redo_score and a0_net_reset.  The activations are only read.
 *  1. G = X^T X (512 x 512) on the fp64 matrix pipe: every lane converts its fp32 element to double, so every product is exact and only the additions round; one
 *     workgroup owns a 64 x 64 tile and walks all rows in order (rows past `rows` count as zeros), an element [i][j], j >= i, is stored at [i][j] and [j][i]: G is
 *     bitwise symmetric and the same from run to run.  No atomics.
 *  2. One workgroup: the eigenvalues l_1 >= ... >= l_512 of G in double (Householder tridiagonalisation of a copy, Sturm bisection with LAPACK dstebz's pivot
 *     safeguard until the interval is two neighbouring doubles); s_i = sqrt(l_i), and s_i = 0 where l_i <= 512 * 2^-52 * l_1 (the floor: the Gram route cannot
 *     resolve singular values below about 3e-7 * s_1, and tiny negative eigenvalues fall under it too);
 *     feature_rank = min { k : (s_1 + ... + s_k) / (s_1 + ... + s_512) >= 1 - delta }, the sums taken in index order in double; 0 if every s_i is 0; -1 if a diagonal
 *     element of G is not finite (the spectrum is then written as zeros).
 * gram: A0_RANK_GRAM_DOUBLES doubles of work space, 8-byte aligned: [0, 512 * 512) holds G afterwards, the second half is the copy the eigenvalue stage destroys.
 * Outputs: spectrum double[A0_RANK_FEATURES] (the s_i, descending), result int[8]: [0] feature_rank, [1] the number of s_i > 0, [2] state[1] of the evaluation (0
 * with a NULL state; the caller initialises it to -1 = "never evaluated"), the rest spare and not written.
 * A0_EINVAL, each with the argument named: a NULL fc1 / gram / spectrum / result, a NULL state without force, rows < 1, freq < 0, delta not in the open interval
 * (0, 1) (NaN included; the number is named), misaligned buffers.  No scratch, no allocation, no host sync: capturable in a hipGraph. */
#define A0_RANK_FEATURES 512
#define A0_RANK_GRAM_DOUBLES (2 * A0_RANK_FEATURES * A0_RANK_FEATURES)
int a0_feature_rank(const float* fc1, long long rows, double delta, const int* state, int freq, int force, double* gram, double* spectrum, int* result, void* stream);
/* ---------------------------------------------------------------- a whole learner behind one handle (opaque handles, library-owned HBM)
 * BaseLearner (agent.py:97-169) with DQNLearner.train_step (173-190) for scalar heads on 4 x 84 x 84 observations — BASELINE configs[1]: online + target parameters
 * in the packed layout (agent0_amd/deepq/layout.py: conv1 | conv2 | conv3 | fc1 | head, each [W (N x K) | b (N)], head rows padded to a multiple of 32), gradients,
 * Adam moments, status words and every workspace live in HBM that a0_learner_create allocates and a0_learner_destroy frees; a0_learner_update is BaseLearner.train —
 * forward passes, loss, backward, Adam(lr, eps = adam_eps or 1e-2 / B), NaN guard, update counter, target copy every target_update_freq updates — as ONE call that
 * enqueues the same launches, in the same order, as the per-kernel entry points above (bit-identical results), never allocates and never synchronises.
 * algo = A0_ALGO_C51 (round 4): C51Learner.train_step (agent.py:218-268) — BASELINE configs[2], with NoisyLinear layers (model.py:28-87; packed as fc1.mu | fc1.sigma |
 * head.mu | head.sigma, composed weights and the noise vectors in HBM of the handle, both networks' noise redrawn per update from Philox stream 4 of `seed` exactly
 * as BaseLearner.train does, agent.py:125-127), dueling, double-Q and n-step.  algo = A0_ALGO_IQN / A0_ALGO_FQF: BASELINE configs[3] / [4]; A0_ALGO_QR / A0_ALGO_MDQN: the reference's remaining learners
 * (num_atoms quantiles per action for qr; NoisyNet allowed for both). */
#define A0_ALGO_DQN 0
#define A0_ALGO_C51 1
#define A0_ALGO_QR 4    /* QRLearner.train_step (agent.py:272-293): num_atoms fixed quantiles per action, quantile Huber loss at the midpoints (2 i + 1) / (2 T) */
#define A0_ALGO_MDQN 5  /* MDQNLearner.train_step (agent.py:194-215): Munchausen DQN, the target network also evaluated on the current observation */
#define A0_ALGO_FQF 3   /* FQFLearner.train_step (agent.py:334-388) with the fraction proposal network (model.py:260-284; its own RMSprop step, agent.py:139-148): packed layout
                         * conv1 | conv2 | conv3 | fc1 | head | cos | frac, Adam over everything before frac; BASELINE configs[4] */
#define A0_ALGO_IQN 2   /* IQNLearner.train_step (agent.py:296-331) with the cosine-embedding head (model.py:203-257): packed layout conv1 | conv2 | conv3 | fc1 | head | cos;
                         * the three tau draws of an update (K, N', N per sample, in that order) come from Philox stream 3 of `seed` as BaseLearner's do */
typedef struct a0_learner a0_learner;
typedef struct a0_learner_desc {
    int A, dueling, double_q;         /* cfg.action_dim, learner.dueling_head, learner.double_q (config.py:72-95) */
    int B, n_step;                    /* learner.batch_size, learner.n_step_q */
    double discount, lr, adam_eps;    /* learner.discount, learner.learning_rate; adam_eps <= 0: the reference's 1e-2 / B (agent.py:105) */
    int target_update_freq;           /* learner.target_update_freq (agent.py:160-161) */
    int algo;                         /* A0_ALGO_* */
    int num_atoms; double vmin, vmax; /* c51: learner.c51.num_atoms / vmin / vmax (config.py:97-101); the support is torch.linspace(vmin, vmax, num_atoms) */
    int noisy;                        /* learner.noisy_net */
    unsigned long long seed;          /* the learner's Philox seed (the Python classes use cfg.seed + 15485863): noise and tau draws */
    int iqn_K, iqn_N, iqn_N_dash;     /* iqn: learner.iqn.K / N / N_dash (config.py:103-109); 64 cosines */
    int fqf_F;                        /* fqf: learner.iqn.F fractions (<= 32) */
    double mdqn_tau, mdqn_lo;         /* mdqn: learner.mdqn.tau / lo (config.py:88-92) */
    double max_grad_norm;             /* (round 5) learner.max_grad_norm: > 0 clips the fqf fraction net's gradient to this L2 norm before its RMSprop step, the only
                                       * place the reference clips (agent.py:143-147); <= 0 (and a zero-initialised trailing field): no clipping */
} a0_learner_desc;
int a0_learner_create(const a0_learner_desc* desc, a0_learner** out);
/* BaseLearner.__init__ (agent.py:97-110) over HBM the CALLER already holds (each pointer may be NULL: the library allocates that buffer): what lets a host that keeps its own views of the
 * parameters — the Python classes' flat tensors, a checkpointing layer — hand the update loop to the library without copies (agent0_amd/deepq/native_loop.py).  Sizes:
 * online / target / adam_m / adam_v a0_learner_param_floats floats (known from a throw-away handle or deepq/layout.py), grads 4 more, state 8 ints, scalars 4,
 * loss_ring loss_ring_cap floats (the per-update batch-mean loss lands in slot state[6] % cap), wt_* a0_net_conv_wt_floats(4), eff_* the composed NoisyNet weights
 * [fc1 | head] and noise [online | target] the noise vectors (layout: a0_learner_desc above).  Borrowed buffers are used as they are: no initial noise is drawn into a
 * borrowed `noise` (a0_learner_set_rng tells the handle where the caller's stream stands).  The library cannot measure a borrowed buffer: `grads` MUST hold
 * a0_learner_param_floats + 4 floats (the NaN flag of a data-parallel update rides behind the parameters), every other size is exactly as listed, all 16-byte aligned. */
typedef struct a0_learner_buffers {
    float *online, *target, *grads, *adam_m, *adam_v;
    int* state;
    float* scalars;
    float* loss_ring; int loss_ring_cap;
    float *wt_online, *wt_target;
    float *eff_online, *eff_target, *noise;
    float* rms_sq;                    /* fqf: the fraction net's RMSprop state, 32 * feat + 32 floats */
} a0_learner_buffers;
int a0_learner_create_on(const a0_learner_desc* desc, const a0_learner_buffers* buffers, a0_learner** out);
/* the next draw offset of one of the learner's Philox streams (3 = the quantile fractions of agent.py:300-310, 4 = NoisyNet's reset_noise of agent.py:125-127) */
int a0_learner_set_rng(a0_learner* learner, int stream_id, unsigned long long offset);
/* the handle's Philox state, for resumable runs: words[0] = seed, words[1 .. 8] = the running offsets of streams 0 .. 7; set != 0 writes them into the handle, 0 reads them */
int a0_learner_rng_state(a0_learner* learner, unsigned long long* words, int set);
int a0_learner_destroy(a0_learner* learner);
long long a0_learner_param_floats(const a0_learner* learner);
/* Data parallelism through the handle (one process per GPU, the reference itself has no multi-GPU learner — launch.py:30-61's actor processes
 * are its only parallelism): with `comm` from a0_dp_init every a0_learner_update SUMs its gradients over the ranks between backward and Adam — the dense blocks
 * (plus the NaN flag behind them) on a side stream while the encoder backward runs, then the convolution blocks, then the join; Adam skips the step on every rank
 * if any rank saw a NaN.  Same buckets and order as agent0_amd/deepq/dist.py::RcclGradAllReduce, issued eagerly.  Collective: every rank sets it before its first
 * update and calls a0_learner_update the same number of times.  comm = 0 switches the exchange off; the caller keeps ownership of the communicator. */
int a0_learner_set_exchange(a0_learner* learner, long long comm);
/* learner.clip_grad_norm through the handle: with max_norm > 0 every a0_learner_update scales the gradient Adam steps on — [0, n_adam) of the flat buffer, i.e.
 * everything but the fqf fraction net, whose own max_grad_norm clip and RMSprop step stay as they are — by min(1, max_norm / (||g|| + 1e-6)), ||g|| taken after the
 * data-parallel exchange has summed both buckets (a0_grad_norm_partials behind the join, then a0_adam_step_sync_wt_clip), and files the pre-clip norm in
 * norm_ring_dev[state[6] % ring_cap] (ring_cap floats the caller owns; NULL: the handle allocates ring_cap slots, 1024 when ring_cap < 1; A0_PEEK_GRAD_NORM_RING
 * returns the ring either way).  max_norm <= 0 switches clipping off again.  Call it between updates, not while one is being captured. */
int a0_learner_set_grad_clip(a0_learner* learner, double max_norm, float* norm_ring_dev, int ring_cap);
/* learner.target_tau through the handle: with 0 < tau < 1 every a0_learner_update passes the period 0 to its Adam form and issues a0_target_blend (the handle's
 * target, its weight copies, desc.target_update_freq) behind it, so the target moves by tau at the updates where it used to be overwritten.  tau <= 0: off, the
 * update issues what it always did.  tau >= 1: A0_EINVAL.  Accepted before the handle's first update only (A0_EINVAL afterwards); descriptor structs are unchanged.
 * The forced copies of a0_learner_create* and a0_learner_set_params stay hard copies. */
int a0_learner_set_target_tau(a0_learner* learner, double tau);
/* learner.weight_decay through the handle: with lambda > 0 every a0_learner_update issues a0_weight_decay — the handle's online parameters [0, n_adam), i.e.
 * everything but the fqf fraction net, c = desc.lr * lambda, the data-parallel NaN flag where an exchange is set — behind the fqf RMSprop step and in front of its
 * Adam form, and takes the three-launch tail as under a0_learner_set_grad_clip.  partials_dev: A0_GRAD_NORM_PARTIALS doubles the caller owns (8-byte aligned), which
 * receive every update's sums of squares; NULL: the handle allocates them (a0_learner_weight_decay_partials returns the pointer either way, NULL while off).
 * lambda <= 0: off, the update issues what it always did.  A0_EINVAL: NaN, fl32(lr * lambda) >= 1 or below 2^-24, a misaligned buffer.  Accepted before the
 * handle's first update only (A0_EINVAL afterwards); descriptor structs are unchanged. */
int a0_learner_set_weight_decay(a0_learner* learner, double lambda, double* partials_dev);
int a0_learner_weight_decay_partials(const a0_learner* learner, double** partials_dev);
/* learner.net_reset_freq / learner.net_reset_shrink through the handle: with freq > 0 every a0_learner_update issues a0_net_reset (the handle's buffers, the rule
 * table built from its own block descriptors — the one agent0_amd/deepq/layout.py::NetLayout.reset_segments builds — alpha = shrink, the low 32 bits of `seed`) as
 * its last launch.  freq == 0: off, the update issues what it always did.  freq < 0, or shrink outside [0, 1] (NaN included): A0_EINVAL.  Accepted before the
 * handle's first update only (A0_EINVAL afterwards); descriptor structs are unchanged.  a0_learner_net_reset_segs copies the table out and returns
 * the number of entries; a `cap` smaller than that is A0_EINVAL (A0_NET_RESET_MAX_SEGS entries always fit). */
int a0_learner_set_net_reset(a0_learner* learner, int freq, double shrink, unsigned long long seed);
int a0_learner_net_reset_segs(const a0_learner* learner, a0_net_reset_seg* out, int cap);
/* learner.redo_freq / learner.redo_tau / learner.redo_recycle through the handle: with freq > 0 every a0_learner_update issues a0_redo_score on the buffers
 * A0_PEEK_ACT1 / 2 / 3 / FC1 name and, with recycle != 0, a0_redo_recycle (the handle's rule table and block descriptors, the low 32 bits of `seed`) behind its Adam
 * form and the blend, in front of a0_net_reset.  freq == 0: off, nothing is allocated and the update issues what it always did.  A0_EINVAL: freq < 0, tau not a
 * finite number in [0, 1), recycle != 0 on a NoisyNet handle (ReDo is undefined for mu / sigma pairs; measuring is allowed), a handle with a data-parallel exchange
 * (the ranks see different batches and would draw different masks; a0_learner_set_exchange refuses the other order), a call after the handle's first update.
 * a0_learner_redo_buffers: the handle's scores float[672], mask int[672], counts int[8] on the device (NULL each while the setting is off); counts[5] is -1 until
 * the first evaluation.  Descriptor structs are unchanged. */
int a0_learner_set_redo(a0_learner* learner, int freq, double tau, int recycle, unsigned long long seed);
int a0_learner_redo_buffers(const a0_learner* learner, float** scores_dev, int** mask_dev, int** counts_dev);
/* learner.rank_freq / learner.rank_delta through the handle: with freq > 0 every a0_learner_update issues a0_feature_rank on the buffer A0_PEEK_FC1 names (for iqn /
 * fqf the B * N rows of the differentiated pass, as a0_redo_score gets them) behind its Adam form and the blend, in front of the ReDo launches and a0_net_reset.
 * freq == 0: off, nothing is allocated and the update issues what it always did.  A0_EINVAL: freq < 0, delta not in the open interval (0, 1) (the number is named), a
 * call after the handle's first update.  The launches modify nothing the update uses, so a handle with a data-parallel exchange is allowed: every rank evaluates its
 * own batch.  a0_learner_feature_rank_buffers: the handle's spectrum double[512] and result int[8] on the device (NULL each while the setting is off); result[2] is
 * -1 until the first evaluation.  Descriptor structs are unchanged. */
int a0_learner_set_feature_rank(a0_learner* learner, int freq, double delta);
int a0_learner_feature_rank_buffers(const a0_learner* learner, double** spectrum_dev, int** result_dev);
/* learner.aug_shift through the handle: with pad > 0 every a0_learner_update first issues a0_augment_shift (the caller's frames / slot / row_bytes, the handle's seed
 * and state words, so u = state[6]) into a stage buffer of B * 2 * C * H * W bytes that the handle allocates on the first such call, and then runs every pass — the
 * target and double-Q passes on st_next, the online pass and mdqn's target pass on st, conv1's weight gradient — on that buffer with a NULL slot; the caller's ring is
 * only read.  pad == 0: off again, the update issues what it always did.  The range checks are a0_augment_shift's, made here against the handle's geometry
 * (A0_EINVAL); with the setting on, a0_learner_update refuses a row_bytes other than 2 * C * H * W.  Call it between updates, not while one is being captured;
 * descriptor structs are unchanged, and nothing is added to a snapshot: the update count travels in the state words. */
int a0_learner_set_aug_shift(a0_learner* learner, int pad);
/* learner.iqn.munchausen through the handle (iqn handles only): with on != 0 every a0_learner_update builds its quantile targets with a0_miqn_target instead of the
 * greedy a0_quantile_target.  The three fraction draws stay as they are (the K draw is made and left unused, so the Philox position is a plain iqn handle's); the
 * encoder launch gets the passes {target, s'}, {target, s}, {online, s}; the target head runs on both target passes at the N' target fractions; the selection pass
 * and a0_select_action are not run.  The first call that switches it on allocates the second target pass's buffers (features of B observations, a head workspace of
 * B * N' rows without gradients).  on == 0: off again, the update issues what it always did (tau, alpha and lo are still checked).  A0_EINVAL, each with the setting
 * and the number named: a handle of another algo, a double-Q handle (there is no argmax to decouple), tau <= 0, alpha < 0, lo > 0, one of the three NaN or
 * infinite (as given or once rounded to float), a call after the handle's first update.  Descriptor structs are unchanged and nothing is added to a snapshot. */
int a0_learner_set_munchausen(a0_learner* learner, int on, double tau, double alpha, double lo);
/* learner.iqn.risk through the learner handle (iqn handles only): with a kind other than A0_RISK_NEUTRAL every a0_learner_update distorts the K SELECTION fractions —
 * those of the greedy next action, of the target network or, under double-Q, of the online network — with one a0_risk_distort launch behind the three draws, into
 * a buffer of B * K floats that the first such call allocates; the selection pass reads that buffer.  The draws, the N' target fractions, the N online fractions,
 * the loss and everything behind it are a neutral handle's, and so is the Philox position: the distortion draws nothing.  A0_RISK_NEUTRAL: off again, the update
 * issues what it always did (eta is ignored).  A0_EINVAL, with the setting and the number named: a kind or an eta a0_risk_distort refuses, a handle of another algo
 * (fqf included: its fractions are proposed, not drawn), a handle with learner.iqn.munchausen on (its target's policy is the softmax of the risk-neutral mean), a
 * call after the handle's first update.  Descriptor structs are unchanged and nothing is added to a snapshot. */
int a0_learner_set_risk(a0_learner* learner, int kind, double eta);
/* learner.c51.hl_gauss through the handle (c51 handles only): with ratio > 0 every a0_learner_update ends its forward half with a0_c51_hl_gauss_head_loss_slabs
 * instead of a0_c51_head_loss_slabs, sigma = ratio * Delta formed in double from the handle's fp32 vmin and vmax, Delta = (vmax - vmin) / (num_atoms - 1).
 * ratio <= 0: off again, the update issues what it always did (on a handle of any algo).  A0_EINVAL, each with the setting and the number named: a ratio that is
 * NaN or infinite, and with ratio > 0 a handle of another algo, ratio > num_atoms, a sigma that is not a normal fp32 number.  Call it between updates, not while
 * one is being captured; nothing is allocated, descriptor structs are unchanged, and nothing is added to a snapshot. */
int a0_learner_set_hl_gauss(a0_learner* learner, double ratio);
/* parameters in the packed layout (device pointers, a0_learner_param_floats floats each); target_packed = NULL: target = copy of online (agent.py:100) */
int a0_learner_set_params(a0_learner* learner, const float* online_packed, const float* target_packed, void* stream);
/* copies of what the handle holds (any pointer may be NULL): parameters, target parameters, Adam moments (param_floats each), the eight status words */
int a0_learner_get(const a0_learner* learner, float* online_out, float* target_out, float* adam_m_out, float* adam_v_out, int* state_out8, void* stream);
/* the handle's own buffer of per-sample losses [B] of the last update — BaseLearner.train's return value (agent.py:163-169) — as a device pointer valid for the
 * handle's lifetime: what a0_rbuf_update_priority (trainer.py:103-104) takes without the copy a non-NULL loss_out of a0_learner_update costs */
int a0_learner_loss_buffer(const a0_learner* learner, float** loss_dev);
/* (round 5) borrowed views of the handle's HBM for inspection — the flat gradient buffer (layout of the parameters) and the differentiated pass's activations
 * (NHWC; their signs are the ReLU decisions of the last update), which a0_learner_get does not copy out: *dev_ptr / *count (floats).  Valid until the next call on
 * the handle.  tests/test_gpu_trace.py walks the handle path against the CPU oracle with them. */
enum { A0_PEEK_GRADS = 0, A0_PEEK_ACT1 = 1, A0_PEEK_ACT2 = 2, A0_PEEK_ACT3 = 3, A0_PEEK_FC1 = 4, A0_PEEK_LOSS = 5, A0_PEEK_GRAD_NORM_RING = 6 /* a0_learner_set_grad_clip */ };
int a0_learner_peek(const a0_learner* learner, int what, float** dev_ptr, long long* count);
/* fqf: a copy of the per-sample fraction losses [B] of the last update (the `fraction_loss` statistic, trainer.py:99-101) into out_dev */
int a0_learner_get_frac_loss(const a0_learner* learner, float* out_dev, void* stream);
/* c51: the support atoms [num_atoms] from HOST memory, for a caller that holds the exact values its reference run used (default: linspace in fp32, torch's formula) */
int a0_learner_set_support(a0_learner* learner, const float* atoms_host);
/* frames: u8 replay rows st || st_next of row_bytes bytes, read through slot [B] (ring slots of the sampled batch; NULL = rows 0 .. B-1); act int32, rew / done /
 * wgt fp32 [B]; loss_out (optional, [B]): the per-sample losses, i.e. what update_priority takes (trainer.py:103-104) */
int a0_learner_update(a0_learner* learner, const uint8_t* frames, const int* slot, long long row_bytes, const int* act, const float* rew, const float* done,
                      const float* wgt, float* loss_out, void* stream);

/* ---------------------------------------------------------------- the rest of the loop behind handles: replay ring and actor (csrc/runtime.hip)
 * a0_rbuf = ReplayDataset (replay.py:14-59) + the sampling of trainer.py:63-72,91-96: the HBM ring of st || st_next rows (2 * obs_bytes each) with its metadata,
 * uniform sampling (the DataLoader's shuffled epochs as a Feistel permutation, last batch of an epoch never returned: utils.py:51-56) or, prioritize != 0,
 * prioritize == 1, proportional sampling from the sum-tree with importance weights and the beta schedule, or, prioritize == 2 (round 6), the reference's prioritized
 * mode TO THE LETTER (replay.sumtree=false; replay.py:45-59, trainer.py:91-104, quirks Q1 / Q2 / Q7): uniform permutation batches, a flat priority vector [size]
 * whose TAIL takes max_p^alpha on every extend, importance weights from priority[idx] / the sum over the WHOLE capacity, priority[ids] = (loss + eps)^alpha.
 * `seed` is the sampler's Philox seed (the Python classes use cfg.seed + 104729). */
typedef struct a0_rbuf a0_rbuf;
typedef struct a0_rbuf_desc {
    long long size; int obs_bytes, B, prioritize;      /* replay.size, C*H*W, learner.batch_size, 0 = uniform / 1 = prioritized, sum-tree / 2 = prioritized, the reference's flat vector */
    double alpha, eps, beta0; long long total_steps;   /* replay.alpha / eps / beta0 (config.py:118-124), trainer.total_steps (the beta schedule's length) */
    unsigned long long seed;
} a0_rbuf_desc;
typedef struct a0_batch { const long long* idx; const int* slot; const int* act; const float* rew; const float* done; const float* prio; const float* weights; } a0_batch;
int a0_rbuf_create(const a0_rbuf_desc* desc, a0_rbuf** out);
/* ReplayDataset.__init__ (replay.py:14-30) over ring buffers the caller already holds (each may be NULL: library-owned): frames [size * 2 * obs_bytes] u8, act i32 / rew / done f32 [size], tree f32
 * [2 * 2^ceil(log2 size)] (prioritize == 1; with prioritize == 2 this argument is the flat priority vector f32 [size], all ones for an empty ring), max_p f32 [1] (must hold the
 * caller's current max priority: 1 for an empty ring) */
int a0_rbuf_create_on(const a0_rbuf_desc* desc, uint8_t* frames, int* act, float* rew, float* done, float* tree, float* max_p, a0_rbuf** out);
int a0_rbuf_destroy(a0_rbuf* replay);
long long a0_rbuf_len(const a0_rbuf* replay);
long long a0_rbuf_write_cursor(const a0_rbuf* replay);
int a0_rbuf_info(const a0_rbuf* replay, long long* top, long long* written, double* beta);
/* the ring's device buffers (any pointer may be NULL): frames [size][2 * obs_bytes] u8, act int32 / rew / done fp32 [size], the sum-tree [2 * cap2] and max_p [1] */
int a0_rbuf_buffers(a0_rbuf* replay, uint8_t** frames, int** act, float** rew, float** done, float** tree, float** max_p);
/* copies into caller buffers (device pointers, any may be NULL): rows [0, rows) of frames / act / rew / done, the sum-tree (2 * cap2 floats), max_p */
int a0_rbuf_read(const a0_rbuf* replay, long long rows, uint8_t* frames_out, int* act_out, float* rew_out, float* done_out, float* tree_out, float* max_p_out, void* stream);
/* ReplayDataset.extend for n transitions already written into the ring at the write cursor (a0_actor_rollout does that) */
int a0_rbuf_commit(a0_rbuf* replay, long long n, void* stream);
/* (round 5) ReplayDataset.extend for a rollout that an asynchronous actor wrote into ANOTHER ring (`stage`: an a0_rbuf of a few rollouts' rows; the launch schedule,
 * launch.py:47-62): rows [start_row, start_row + n) of `stage` are copied to this ring's write cursor and committed like a0_rbuf_commit.  The caller orders the call
 * behind the rollout's end. */
int a0_rbuf_extend_from(a0_rbuf* replay, const a0_rbuf* stage, long long start_row, long long n, void* stream);
/* one batch into the handle's persistent batch buffers (device pointers in *out, valid until the next sample) */
int a0_rbuf_sample(a0_rbuf* replay, a0_batch* out, void* stream);
/* uniform replay: the next n <= 32 batches — exactly the batches n consecutive a0_rbuf_sample calls would return (trainer.py:63-72: they do not depend on the updates
 * between them) — drawn by ONE launch into n persistent batch buffers (valid until the next sample call of either kind).  Prioritized replay: A0_EINVAL. */
int a0_rbuf_sample_block(a0_rbuf* replay, int n, a0_batch* out, void* stream);
/* ReplayDataset.update_priority with the last batch's indices and the learner's per-sample losses; learner_state: a0_learner_get's status words or NULL */
int a0_rbuf_update_priority(a0_rbuf* replay, const float* loss, const int* learner_state, void* stream);

/* a0_actor = Actor (agent.py:19-90) on the device-resident synthetic env for the heads a0_learner covers (scalar; categorical with or without NoisyNet; implicit quantile; fully parameterised quantile): observations, epsilon-greedy Philox streams (seed, rank), n-step ring,
 * episode statistics.  a0_actor_rollout = Actor.sample: T steps acting with the learner's online network, transitions written into the replay ring at its write
 * cursor (then a0_rbuf_commit(replay, T * E)); a0_actor_collect waits for the stream and returns qs [T] and the finished episodes' returns (host memory). */
typedef struct a0_actor a0_actor;
typedef struct a0_actor_desc {
    int E, T, A, dueling, n_step;                      /* actor.num_envs, actor.sample_steps, cfg.action_dim, learner.dueling_head, learner.n_step_q */
    double discount;                                   /* learner.discount */
    unsigned long long seed; unsigned int rank;        /* cfg.seed, this process's rank */
    int env_task;                                      /* A0_ENV_TASK_* */
    int reset_noise_freq;                              /* learner.reset_noise_freq (NoisyNet learners; 0 = the reference's default 4) */
} a0_actor_desc;
int a0_actor_create(const a0_actor_desc* desc, a0_actor** out);
int a0_actor_destroy(a0_actor* actor);
/* (round 5) every workspace a rollout with `learner` needs, allocated at set-up (a0_actor_rollout on an unbound actor binds it first — the one call after create that
 * allocates); own_network != 0: the actor also gets its OWN copy of the network (parameters, weight copies, NoisyNet noise and composed weights), which
 * a0_actor_snapshot refreshes from the learner — the launch schedule's actor.futures.sample(eps, state_dict) (launch.py:34-36,58-62).  Without it the actor acts with
 * the learner's online network, NoisyNet buffers included, like the reference's train actor on the main schedule (trainer.py:41-44: the SAME module). */
int a0_actor_bind(a0_actor* actor, const a0_learner* learner, int own_network);
int a0_actor_snapshot(a0_actor* actor, const a0_learner* learner, void* stream);
/* (the learner is not const: like the reference's single-process main, the actor acts with the learner's own network object — a NoisyNet actor redraws that
 * network's noise every reset_noise_freq steps from ITS Philox stream 4 and recomposes the effective weights, agent.py:52-53) */
int a0_actor_rollout(a0_actor* actor, a0_learner* learner, a0_rbuf* replay, float epsilon, void* stream);
/* actor.eps_ladder for the handle: from now on a0_actor_rollout launches a0_eps_ladder(epsilon, NULL, alpha, E, i0, n_total, vec) once, ahead of its first step, into
 * an [E] vector the handle owns (allocated by the first call with alpha > 0) and every step's tail reads its env's own entry (A0_EPS_PER_ENV) — device env,
 * attached pool and the launch schedule's actor stream alike.  alpha <= 0 switches it off again: the rollout's launches and their arguments are those of a handle
 * that never heard of it.  Derived from `epsilon` every rollout, so no part of a0_actor_state_save. */
int a0_actor_set_eps_ladder(a0_actor* actor, float alpha, long long i0, long long n_total);
/* learner.iqn.risk for the actor handle: with a kind other than A0_RISK_NEUTRAL every step of a0_actor_rollout with an iqn learner draws its E * K fractions with
 * a0_tau_cos_features_risk(kind, eta) in a0_tau_cos_features's place — one launch, as before; the tail kernels and their arguments are untouched — device env and
 * attached pool alike.  A0_RISK_NEUTRAL: the rollout calls what it always called.  No state of its own: nothing in a0_actor_state_save.  A0_EINVAL: a kind or an
 * eta a0_risk_distort refuses, a call after the handle's first rollout; a0_actor_rollout then refuses, before anything is launched, a learner of any algo but iqn. */
int a0_actor_set_risk(a0_actor* actor, int kind, double eta);
/* where a quantile actor's steps leave their E * nt fractions on the device (iqn: the draws, distorted under learner.iqn.risk; fqf: the tau-hats): the handle's own
 * buffer, overwritten by every step; NULL until the actor is bound to a quantile learner.  For inspection (tests); nothing reads it between steps. */
int a0_actor_fractions(const a0_actor* actor, float** taus_dev);
/* Scalar heads and c51 / qr: a0_actor_rollout over the device env lays fc1's weights out once per rollout (and after every noise reset) with a0_actor_fc1_planes and runs the steps'
 * fc1 through a0_actor_fc1 where a0_actor_fc1_ok accepts the shape.  on = 0: the handle keeps the general GEMM in every step — the same bytes (for comparisons). */
int a0_actor_set_fc1_planes(a0_actor* actor, int on);
/* steps whose fc1 a0_actor_rollout has run as a0_actor_fc1_kernel since the handle was created */
long long a0_actor_fc1_launches(const a0_actor* actor);
int a0_actor_collect(a0_actor* actor, float* qs_host, float* returns_host, int max_returns, int* n_returns, void* stream);
/* Host environments stepped by worker processes (agent0_amd/common/env_pool.py HostEnvPool): while a pool is attached, a0_actor_rollout steps IT instead of the
 * device env.  Per step t: encoder, fc1 + head + the head's tail (a0_actor_qhead / a0_actor_dist_tail / a0_actor_quantile_tail, the full batch's split counts),
 * a0_env_pool_send of the actions and the step word, a host-side wait for every worker's done word, the DMA-only a0_env_pool_upload, then a0_host_step_ingest
 * (frame stack, n-step window, replay row, statistics).  The rows, parameters and statistics equal those of Actor._rollout_host.
 *
 * The shared page-locked block (host_envs.block_layout; one half per step parity h = seq & 1):
 *   obs_host[h]   [E][nstack * frame_bytes] u8  whole stacks, read for the envs whose advance scalar is 0
 *   scal_host[h]  [7][E] f32                    reward, terminated, truncated, life_loss, final mask, final return, advance (1: the stack moved on by one frame)
 *   new_host[h]   [E][frame_bytes] u8           the newest frame of every env
 *   actions       [E] i32                       written by the device through act_dev before the step word
 *   control       i64 words: [0] the step word (step_word | (seq & seq_mask): host_envs.ctl_word(CMD_STEP, seq)), written through ctl_dev; [1] a reset's
 *                 argument; [2 + w] the last sequence number worker w has completed (done_host points at [2]); a worker that dies stores -1 there.
 * A worker polls word [0] for seq + 1, steps its envs with the actions, writes its envs' rows of half (seq + 1) & 1, then stores seq + 1 into its done word.
 * obs_dev[2] is the device observation double buffer: the observation of sequence number s lives in obs_dev[s & 1].  `seq` is the pool's current sequence
 * number at attach time; a0_actor_pool_seq reads it back after a rollout and sets it after the host has stepped or reset the pool itself.  The wait gives up
 * with an error when a done word is negative or after timeout_s seconds; after 2 ms it sleeps between polls. */
typedef struct a0_env_pool_desc {
    int E, nstack, W, use_life_loss;                   /* envs, frames per stack, worker processes (>= 1), 0: ignore the life_loss row */
    long long frame_bytes;                             /* bytes per frame (a multiple of 16) */
    void* new_host[2]; void* scal_host[2]; void* obs_host[2];      /* page-locked host halves (host addresses) */
    void* act_dev; void* ctl_dev;                      /* device addresses of the action slot and of control word 0 (a0_host_device_pointer) */
    long long* done_host;                              /* host address of the W done words */
    void* obs_dev[2]; void* scal_dev[2]; void* new_dev;   /* device buffers: observations, scalars per half, newest frames */
    long long step_word, seq_mask;                     /* CMD_STEP << CMD_SHIFT, (1 << CMD_SHIFT) - 1 */
    long long seq;                                     /* the pool's sequence number now */
    double timeout_s;                                  /* give up waiting for the workers after this long */
} a0_env_pool_desc;
int a0_actor_attach_pool(a0_actor* actor, const a0_env_pool_desc* desc);
int a0_actor_detach_pool(a0_actor* actor);
/* *seq_out (optional) := the attached pool's sequence number, *whole_out (optional) := stacks uploaded whole since attach; then, set_seq >= 0: the sequence
 * number := set_seq (the host stepped or reset the pool itself) */
int a0_actor_pool_seq(a0_actor* actor, long long* seq_out, long long* whole_out, long long set_seq);
/* a0_actor_collect (the rs / qs of Actor.sample, agent.py:85-90) in two halves, so that the next rollout can be enqueued before the host waits: _begin enqueues the copies of the statistics into page-locked
 * buffers of the handle and records an event (call it BEFORE the next a0_actor_rollout, which reuses the device buffers); _end waits for that event only */
int a0_actor_collect_begin(a0_actor* actor, void* stream);
int a0_actor_collect_end(a0_actor* actor, float* qs_host, float* returns_host, int max_returns, int* n_returns);

/* ---------------------------------------------------------------- resumable runs (Trainer.save_snapshot / load_snapshot; csrc/runtime.hip, csrc/snapshot.hip)
 * What the handles own and no caller-visible buffer holds, as versioned flat blobs in HOST memory: 32 little-endian 8-byte words (doubles as their bit patterns),
 * for the actor followed by copies of its device arrays.  _save waits for `stream`; _load refuses a blob whose description differs from the handle's, with a message.
 * The seeds are state: a blob loaded into a handle created with another seed continues the saved run.
 *   replay  0 magic, 1 version (1), 2 size, 3 obs_bytes, 4 B, 5 prioritize, 6 top, 7 written, 8 epoch open, 9 epoch top, 10 epoch batches, 11 epoch position,
 *           12 epoch seed, 13..20 Philox offsets, 21 beta in use, 22 beta schedule, 23 max_p, 24 Philox seed, 25 alpha, 26 eps, 27 beta0, 28 total_steps.
 *           _save brings the sum-tree's top levels up to date first (like a0_rbuf_read), so that the caller can save the tree from its own buffer.
 *   actor   0 magic, 1 version (1), 2 E, 3 T, 4 A, 5 dueling, 6 n_step, 7 env_task, 8 reset_noise_freq, 9 discount, 10 observation buffers K, 11 current buffer,
 *           12 env step counter, 13 actor step counter, 14 Philox seed, 15..22 Philox offsets, 23 env seed, 24 rank; then obs [K][E][obs_bytes] u8, ep_ret [E] f32,
 *           ring_act [n][E] i32, ring_rew, ring_done [n][E] f32, qs [T], stat_mask [T][E], stat_ret [T][E] f32 (the last rollout's statistics: a rollout issued ahead
 *           and not yet collected is collected after the load).  An actor with an attached host pool has no saveable env state: A0_ESTATE. */
long long a0_rbuf_state_size(const a0_rbuf* replay);
int a0_rbuf_state_save(a0_rbuf* replay, void* blob_host, long long capacity, void* stream);
int a0_rbuf_state_load(a0_rbuf* replay, const void* blob_host, long long bytes, void* stream);
long long a0_actor_state_size(const a0_actor* actor);
int a0_actor_state_save(a0_actor* actor, void* blob_host, long long capacity, void* stream);
int a0_actor_state_load(a0_actor* actor, const void* blob_host, long long bytes, void* stream);
/* Frame deduplication of ring rows on the way to a snapshot file and back (csrc/snapshot.hip).  A chunk is `rows` consecutive ring rows of frames_per_row frames of
 * frame_bytes bytes (a multiple of 16), at most 32 768 frames.  a0_snapshot_pack looks, for every frame in row order, for the first byte-identical frame among the
 * earlier frames of its row and then the frames of the row `stride` earlier in the chunk (stride = num_envs: the same env's previous step; 0: same row only), by
 * comparing bytes, and writes
 *     u32 lit_id[rows * frames_per_row] | u32 n_lit | pad to 16 B | u8 literals[n_lit][frame_bytes]        (literals at a0_snapshot_literal_offset)
 * to `packed` (a0_snapshot_pack_bound bytes: every frame a literal); lit_id names each frame's literal with reference chains resolved, literals are in row order, and
 * the bytes are a function of the chunk's bytes alone.  `work`: rows * frames_per_row u32 of device scratch.  a0_snapshot_unpack writes frame (r, j) =
 * literals[lit_id[r][j]] into `rows_out`; an id >= n_lit (a damaged file) writes nothing and sets *bad_flag (device int, may be NULL) to 1.  Device pointers, 16-byte aligned. */
long long a0_snapshot_pack_bound(long long rows, int frames_per_row, int frame_bytes);
long long a0_snapshot_literal_offset(long long rows, int frames_per_row);
int a0_snapshot_pack(const uint8_t* rows, long long n_rows, int frames_per_row, int frame_bytes, long long stride, uint8_t* packed, unsigned int* work, void* stream);
int a0_snapshot_unpack(const uint8_t* packed, long long n_rows, int frames_per_row, int frame_bytes, uint8_t* rows_out, int* bad_flag, void* stream);

/* data parallelism: this rank's NaN flag as a float (1.0 / 0.0) that rides at the tail of a SUM-reduced gradient bucket; the reduced value
 * comes back through extra_nan_flag (nonzero = some rank saw a NaN: every rank skips the step), NULL on one GPU */
int a0_nan_flag_export(const int* state, float* out, void* stream);
int a0_rmsprop_step(float* params, const float* grads, float* square_avg, long long n, double lr, double alpha, double eps,
                    double max_grad_norm, float* clip_scratch, void* stream);
int a0_target_sync(float* target, const float* online, long long n, const int* state, int force, void* stream);
/* NoisyLinear.reset_noise / forward weight composition and its gradient fan-out (model.py:54-62,73-87) */
int a0_noisy_compose(const float* mu, const float* sigma, float* eff, int N, int K, int r0, int r1, const float* noise_in,
                     const float* noise_out_w, const float* noise_out_b, void* stream);
int a0_noisy_grad_sigma(const float* gmu, float* gsigma, int N, int K, int r0, int r1, const float* noise_in,
                        const float* noise_out_w, const float* noise_out_b, void* stream);
/* up to three NoisyLinear modules (first_dense, q_head, value_head) in one launch; host arrays of per-module arguments.
 * grad = 0: a0_noisy_compose per module; grad = 1: a0_noisy_grad_sigma per module (mu = gmu, eff = gsigma, sigma unused) */
int a0_noisy_multi(int grad, int nmod, const float* const* mu, const float* const* sigma, float* const* eff, const int* N, const int* K, const int* r0,
                   const int* r1, const float* const* noise_in, const float* const* noise_out_w, const float* const* noise_out_b, void* stream);

/* ---------------------------------------------------------------- replay (agent0/deepq/replay.py:14-59, trainer.py:63-72,91-96) */
int a0_replay_insert(uint8_t* frames, long long cap, int obs_bytes, long long start_slot, int n, const uint8_t* obs,
                     const uint8_t* obs_next, const int* act, const float* rew, const float* done, int* r_act,
                     float* r_rew, float* r_done, const long long* ctrl, void* stream);
int a0_replay_lookup(const long long* idx, int B, long long top, long long head, long long cap, int* slot, const int* r_act,
                     const float* r_rew, const float* r_done, const float* priority, int* act, float* rew, float* done,
                     float* prio, long long* idx_out, void* stream);
int a0_replay_gather(const uint8_t* frames, int row_bytes, const int* slot, int B, uint8_t* out, void* stream);
/* index generation + metadata lookup + row gather in ONE launch (trainer.py:63-72 + replay.py:32-37): mode 0 = element start+b of the
 * epoch's Feistel permutation of [0, n_perm), mode 1 = stratified sum-tree draw with xi[b] */
int a0_replay_sample_gather(int mode, unsigned long long start, unsigned long long n_perm, unsigned int seed, const float* tree, long long cap2,
                            const float* xi, long long top, long long head, long long cap, const uint8_t* frames, int row_bytes, const int* r_act,
                            const float* r_rew, const float* r_done, const float* priority, int B, uint8_t* out, long long* idx_out, int* slot_out,
                            int* act, float* rew, float* done, float* prio, void* stream);
/* uniform sampling without the row copy (the learner's conv1 reads ring rows through slot_out): == a0_perm_batch + a0_replay_lookup */
int a0_replay_sample_slots(unsigned long long start, unsigned long long n_perm, unsigned int seed, long long top, long long head, long long cap,
                           const int* r_act, const float* r_rew, const float* r_done, const float* priority, int B, long long* idx_out, int* slot_out,
                           int* act, float* rew, float* done, float* prio, void* stream);
/* n <= 32 such batches in ONE launch (host arrays start / n_perm / seed [n]; outputs [n][B]): uniform replay's batches do not depend on the updates between them
 * (the DataLoader's shuffled epochs, trainer.py:63-72), so a whole update block's sampling is one launch */
int a0_replay_sample_slots_multi(int n, const unsigned long long* start, const unsigned long long* n_perm, const unsigned int* seed, long long top, long long head, long long cap,
                                 const int* r_act, const float* r_rew, const float* r_done, int B, long long* idx_out, int* slot_out, int* act, float* rew, float* done,
                                 float* prio, void* stream);
int a0_fill_f32(float* p, long long n, float v, void* stream);
int a0_priority_update(float* priority, const long long* ids, const float* loss, int B, float eps, float alpha,
                       float* pstate, const int* state, void* stream);
int a0_priority_tail(float* priority, long long size, long long n, const float* pstate, float alpha, void* stream);
int a0_sum_f32(const float* x, long long n, float* scratch256, float* out, void* stream);
int a0_is_weights(const float* prio, int B, const float* psum, long long top, float beta, float* w, void* stream);
int a0_perm_batch(unsigned long long start, int count, unsigned long long n, unsigned int seed, long long* out, void* stream);
/* sum-tree (new component, contract in oracle/sumtree.c): tree float[2*cap2] */
/* n <= 1024 leaves per call (larger batches: consecutive calls in batch order, so that a later duplicate still wins).  state (optional,
 * the learner's status words): the call is a no-op when state[3] != 0, i.e. when the update was skipped on a NaN loss (agent.py:152-158) */
int a0_sumtree_set(float* tree, long long cap2, const long long* idx, const float* val, int n, const int* state, void* stream);
/* leaves (start + i) % size, i < n, all set to val[0] (device scalar) and their ancestors recomputed: the rollout's new transitions enter at
 * max_p^alpha (replay.py:45-53) in one launch; same tree as a0_sumtree_set on those pairs */
int a0_sumtree_set_range(float* tree, long long cap2, long long start, long long n, long long size, const float* val, void* stream);
int a0_sumtree_rebuild(float* tree, long long cap2, void* stream);
int a0_sumtree_sample(const float* tree, long long cap2, const float* xi, int B, long long* out_idx, float* out_p, void* stream);
/* one prioritized batch in one launch: stratified uniforms from the sampler's Philox stream, sum-tree descent, slot + metadata lookup and
 * importance weights (trainer.py:91-94); == a0_rng_uniform + a0_sumtree_sample + a0_replay_lookup + a0_is_weights.  B <= 1024. */
int a0_sumtree_sample_batch(unsigned long long seed, unsigned int stream, unsigned long long offset, float* tree, long long cap2, int B, long long top,
                            long long cap, float beta, const int* r_act, const float* r_rew, const float* r_done, long long* idx_out, int* slot_out,
                            int* act, float* rew, float* done, float* prio, float* w, int rebuild_top, void* stream_h);
/* (round 4) the kernel stages the levels with <= 2048 nodes in LDS — recomputed from level 2048 (or the leaves of a smaller tree) — and walks them there;
 * rebuild_top = 1 also writes them back: the launch a0_sumtree_set_from_loss(defer_top = 1) left out, so that replay.py:55-59 followed by the next
 * trainer.py:63-72 batch is two launches */
/* val = (loss + eps)^alpha, pstate[0] = max(pstate[0], max loss) (replay.py:55-59); no-op when state && state[3] (NaN-skipped update) */
int a0_priority_from_loss(const float* loss, int n, float eps, float alpha, float* val, float* pstate, const int* state, void* stream);
/* a0_priority_from_loss + a0_sumtree_set in two launches instead of three (replay.py:55-59 on the sum-tree): the per-subtree kernel forms (loss + eps)^alpha while it
 * stages the batch and keeps pstate[0] = max_p; n <= 1024; for trees with a0_sumtree_set_from_loss_ok(cap2) == 1 (64 ... 1024 leaves per subtree below the top 2048 nodes) */
int a0_sumtree_set_from_loss_ok(long long cap2);
int a0_sumtree_set_from_loss(float* tree, long long cap2, const long long* idx, const float* loss, int n, float eps, float alpha, float* pstate, const int* state,
                             int defer_top, void* stream);
/* defer_top = 1 (replay.py:55-59 followed by the next batch of trainer.py:63-72 in two launches): leaves and subtrees only (one launch); tree[1 .. 2047] are stale until a0_sumtree_sample_batch(rebuild_top = 1), a0_sumtree_set_range (which
 * recomputes the top from level 2048 anyway) or a0_sumtree_top_rebuild has run — every other reader of the top levels must be preceded by one of them */
int a0_sumtree_top_rebuild(float* tree, long long cap2, void* stream);

/* ---------------------------------------------------------------- actor (agent0/deepq/agent.py:25-39,57-73) */
/* Epsilon of the action-selection entry points below (every one that takes `eps_ptr`): eps_ptr == NULL: the scalar argument `eps`; eps_ptr != NULL: eps_ptr[0], a
 * device scalar (a captured rollout's epsilon), and `eps` is ignored — unless `eps` is A0_EPS_PER_ENV: then env e of the launch acts with its OWN eps_ptr[e]
 * (eps_ptr: [E] floats; the index is relative to the pointer, so a launch over envs [off, off + k) of a vector passes vec + off).  What actor.eps_ladder hands in.
 * CAUTION: beside a device scalar `eps` is therefore no longer a don't-care.  A caller who passes -1.0f there with a one-float eps_ptr makes the kernel read
 * eps_ptr[1 .. E - 1], past that buffer; the entry points cannot see its length.  Pass any other value (0 will do) beside a device scalar. */
#define A0_EPS_PER_ENV (-1.0f)
/* The Ape-X epsilon ladder (actor.eps_ladder = alpha > 0): eps_vec[e] = ladder(eps, i0 + e, n_total) for e < E, where
 *   ladder(eps, i, N) = eps^(1 + alpha * i / (N - 1))   formed as pow((double)eps, 1.0 + (double)alpha * i / (N - 1)) and rounded to fp32 once,
 *   = eps, bit for bit, where eps >= 1 (the schedule's all-random warm-up), i == 0 or N <= 1;  = 0 where eps <= 0.
 * i0 / n_total: the launch's first env in, and the size of, the GLOBAL vector of environments (data parallel: rank * E of world * E).  eps = eps_ptr[0] when
 * eps_ptr is given (a captured rollout).  One small launch per rollout; alpha <= 0, E < 1, i0 < 0 or i0 + E > n_total: A0_EINVAL. */
int a0_eps_ladder(float eps, const float* eps_ptr, float alpha, int E, long long i0, long long n_total, float* eps_vec, void* stream);
int a0_actor_egreedy(const int* greedy, const int* rand_action, const float* u, float eps, int E, int* action,
                     const float* qmax, float* qs_out, void* stream);
/* Fused actor tail for scalar heads (dqn / mdqn), Actor.act (agent.py:25-39) after the encoder: fc1 (split-K GEMM into `scratch`,
 * a0_actor_qhead_scratch(E, K) floats) + bias + ReLU, q head (W2 [A(+1)][512], b2), dueling combine (model.py:123-131), first-max
 * argmax, epsilon-greedy draw from the Philox streams (same draws as a0_actor_egreedy_rng).  qmax[e] = max_a q(e, a). */
long long a0_actor_qhead_scratch(int E, int K);
int a0_actor_qhead(const float* feat, int E, int K, const float* W1, const float* b1, const float* W2, const float* b2, int A, int dueling,
                   float* scratch, unsigned long long seed, unsigned int stream_a, unsigned int stream_u, unsigned long long off_a,
                   unsigned long long off_u, float eps, const long long* ctrl, const float* eps_ptr, int* action, float* qmax, void* stream);
/* a0_actor_qhead with the fc1 GEMM's split count given by the caller (scratch: splits * E * 512 floats) — see a0_dense_fwd_n; a0_actor_qhead uses
 * a0_dense_fwd_partial_slabs(E, 512, K) */
int a0_actor_qhead_n(const float* feat, int E, int K, int splits, const float* W1, const float* b1, const float* W2, const float* b2, int A, int dueling,
                     float* scratch, unsigned long long seed, unsigned int stream_a, unsigned int stream_u, unsigned long long off_a,
                     unsigned long long off_u, float eps, const long long* ctrl, const float* eps_ptr, int* action, float* qmax, void* stream);
/* a0_actor_qhead + a0_env_synth_step_commit in two launches instead of three (the fc1 GEMM, then ONE kernel with a workgroup per env: one
 * wave runs the tail and the env's scalar work with the chosen action while the others already write the new frame / stack / replay row).
 * Arguments: those of a0_actor_qhead, then those of a0_env_synth_step_commit (the action is taken from, and written to, `action`). */
int a0_actor_qhead_env_step(const float* feat, int E, int K, const float* W1, const float* b1, const float* W2, const float* b2, int A, int dueling,
                            float* scratch, unsigned long long seed, unsigned int stream_a, unsigned int stream_u, unsigned long long off_a,
                            unsigned long long off_u, float eps, const long long* ctrl, const float* eps_ptr, int* action, float* qmax,
                            unsigned long long env_seed, unsigned int rank, unsigned int g, const uint8_t* obs_in, uint8_t* obs_out, float* ep_ret,
                            float* final_mask, float* final_ret, int n, long long steps, double gamma, int* ring_act, float* ring_rew, float* ring_done,
                            const uint8_t* obs0, uint8_t* frames, long long cap, long long start_slot, int* r_act, float* r_rew, float* r_done, int task, void* stream);
/* ... with fc1 taken from pre-split weights where a0_actor_fc1_ok accepts the step (w1_planes = a0_actor_fc1_planes of W1, or NULL: the call above): the same bytes */
int a0_actor_qhead_env_step_wp(const float* feat, int E, int K, const float* W1, const float* b1, const float* W2, const float* b2, int A, int dueling,
                            float* scratch, unsigned long long seed, unsigned int stream_a, unsigned int stream_u, unsigned long long off_a,
                            unsigned long long off_u, float eps, const long long* ctrl, const float* eps_ptr, int* action, float* qmax,
                            unsigned long long env_seed, unsigned int rank, unsigned int g, const uint8_t* obs_in, uint8_t* obs_out, float* ep_ret,
                            float* final_mask, float* final_ret, int n, long long steps, double gamma, int* ring_act, float* ring_rew, float* ring_done,
                            const uint8_t* obs0, uint8_t* frames, long long cap, long long start_slot, int* r_act, float* r_rew, float* r_done, int task, const unsigned int* w1_planes, void* stream);
/* out[t] = mean over e of x[t][e] (per-step mean max-Q of a rollout, agent.py:38,88) */
int a0_mean_rows(const float* x, int T, int E, float* out, void* stream);

/* the same with both draws generated in-kernel from Philox streams (bit-identical to a0_rng_randint + a0_rng_uniform + a0_actor_egreedy) */
/* (round 5) a0_actor_qhead_env_step whose second launch goes on to ENCODE the env's new observation: fc1 GEMM over `feat`, then ONE launch per env for tail + env
 * step + the fused encoder over obs_out into act3_next [E][3136] (may be `feat`) — the next actor step's features, so that a step is two launches instead of three
 * (agent.py:25-39,52-81 and model.py:90-105 for the next observation).  wt / w: the acting network's weight copies and encoder weights as for
 * a0_net_encoder_fwd_fused (4 x 84 x 84 observations only).  Same bytes and features as a0_actor_qhead_env_step + a0_net_encoder_fwd_fused. */
int a0_actor_qhead_env_step_enc(const float* feat, int E, int K, const float* W1, const float* b1, const float* W2, const float* b2, int A, int dueling,
                                float* scratch, unsigned long long seed, unsigned int stream_a, unsigned int stream_u, unsigned long long off_a,
                                unsigned long long off_u, float eps, const long long* ctrl, const float* eps_ptr, int* action, float* qmax,
                                unsigned long long env_seed, unsigned int rank, unsigned int g, const uint8_t* obs_in, uint8_t* obs_out, float* ep_ret,
                                float* final_mask, float* final_ret, int n, long long steps, double gamma, int* ring_act, float* ring_rew, float* ring_done,
                                const uint8_t* obs0, uint8_t* frames, long long cap, long long start_slot, int* r_act, float* r_rew, float* r_done, int task,
                                const float* wt, const a0_encoder_weights* w, float* act3_next, void* stream);
/* ... with fc1 taken from pre-split weights where a0_actor_fc1_ok accepts the step (w1_planes = a0_actor_fc1_planes of W1, or NULL: the call above): the same bytes */
int a0_actor_qhead_env_step_enc_wp(const float* feat, int E, int K, const float* W1, const float* b1, const float* W2, const float* b2, int A, int dueling,
                                float* scratch, unsigned long long seed, unsigned int stream_a, unsigned int stream_u, unsigned long long off_a,
                                unsigned long long off_u, float eps, const long long* ctrl, const float* eps_ptr, int* action, float* qmax,
                                unsigned long long env_seed, unsigned int rank, unsigned int g, const uint8_t* obs_in, uint8_t* obs_out, float* ep_ret,
                                float* final_mask, float* final_ret, int n, long long steps, double gamma, int* ring_act, float* ring_rew, float* ring_done,
                                const uint8_t* obs0, uint8_t* frames, long long cap, long long start_slot, int* r_act, float* r_rew, float* r_done, int task,
                                const float* wt, const a0_encoder_weights* w, float* act3_next, const unsigned int* w1_planes, void* stream);
/* (round 5) a0_actor_dist_tail_env_step (c51 / qr) whose kernel goes on to encode the env's new observation into act3_next [E][3136], as a0_actor_qhead_env_step_enc
 * does for scalar heads: the same bytes and features as a0_actor_dist_tail_env_step + a0_net_encoder_fwd_fused, one launch and one kernel boundary less per step. */
int a0_actor_dist_tail_env_step_enc(const float* slabs, long long slab_stride, int nslab, const float* bias, int ld, int A, int T, int dueling, int mode,
                                    const float* atoms, int E, unsigned long long seed, unsigned int stream_a, unsigned int stream_u, unsigned long long off_a,
                                    unsigned long long off_u, float eps, const long long* ctrl, const float* eps_ptr, int* action, float* qmax,
                                    unsigned long long env_seed, unsigned int rank, unsigned int g, const uint8_t* obs_in, uint8_t* obs_out, float* ep_ret,
                                    float* final_mask, float* final_ret, int n, long long steps, double gamma, int* ring_act, float* ring_rew, float* ring_done,
                                    const uint8_t* obs0, uint8_t* frames, long long cap, long long start_slot, int* r_act, float* r_rew, float* r_done, int task,
                                    const float* wt, const a0_encoder_weights* w, float* act3_next, void* stream);
/* (round 6) the same for the quantile networks' tail (a0_actor_quantile_tail_env_step: iqn mode 1, fqf mode 3 with `taus` [E][T + 1]): tail + env step + replay row +
 * the new observation's encoder in one launch — an iqn actor step is then a0_tau_cos_features | embedding GEMM | fc1 GEMM | head GEMM | this. */
int a0_actor_quantile_tail_env_step_enc(const float* slabs, long long slab_stride, int nslab, const float* bias, int ld, int A, int T, int dueling, int mode,
                                        const float* taus, int E, unsigned long long seed, unsigned int stream_a, unsigned int stream_u, unsigned long long off_a,
                                        unsigned long long off_u, float eps, const long long* ctrl, const float* eps_ptr, int* action, float* qmax,
                                        unsigned long long env_seed, unsigned int rank, unsigned int g, const uint8_t* obs_in, uint8_t* obs_out, float* ep_ret,
                                        float* final_mask, float* final_ret, int n, long long steps, double gamma, int* ring_act, float* ring_rew, float* ring_done,
                                        const uint8_t* obs0, uint8_t* frames, long long cap, long long start_slot, int* r_act, float* r_rew, float* r_done, int task,
                                        const float* wt, const a0_encoder_weights* w, float* act3_next, void* stream);
int a0_actor_egreedy_rng(const int* greedy, unsigned long long seed, unsigned int stream_a, unsigned int stream_u, unsigned long long off_a,
                         unsigned long long off_u, int A, float eps, int E, int* action, const float* qmax, float* qs_out,
                         const long long* ctrl, const float* eps_ptr, void* stream);
int a0_actor_nstep(int E, int n, long long steps, double gamma, const int* action, const float* reward, const float* terminal,
                   const float* truncated, const float* life_loss, int* ring_act, float* ring_rew, float* ring_done,
                   int* out_act, float* out_rew, float* out_done, const long long* ctrl, void* stream);

/* Device frame stack for host environments.  Replaces gymnasium FrameStack's host-side stacking plus the
 * per-step upload of the whole (E, nstack, H, W) batch (atari_wrappers.py:63, agent.py:27): out[e] = prev[e][1:] || newest[e] for envs
 * with advance[e] != 0 (their stack moved on by exactly one frame); rows with advance[e] == 0 are left untouched (uploaded whole).
 * prev / out: [E][nstack][frame_bytes] u8, newest: [E][frame_bytes]; frame_bytes a multiple of 16, pointers 16-byte aligned. */
int a0_env_frame_stack(const uint8_t* prev, const uint8_t* newest, const float* advance, uint8_t* out, int E, int nstack, long long frame_bytes,
                       void* stream);

/* The two PCIe legs of a host-environment step as one call each (the host thread's enqueue time is on the critical path between "the
 * workers have finished" and "the workers see the next actions").
 * a0_env_pool_upload: agent.py:27 `torch.from_numpy(obs).to(device)` — newest frames [E][frame_bytes] and scalars [n_scal][E] host -> device,
 *   whole stacks (obs_host rows [E][nstack][frame_bytes]) for the envs whose row `advance_row` of the HOST scalars is 0, then a0_env_frame_stack
 *   into `out` from `prev`.  Host pointers must be page-locked; *n_whole (optional) receives the number of whole stacks uploaded.
 * a0_env_pool_send: the direction AsyncVectorEnv.step_async pickles through pipes (atari_wrappers.py:59-69) — E actions, then the 8-byte step
 *   word, stored into page-locked host memory through its DEVICE address (a0_host_device_pointer) by two kernels in stream order: a worker that
 *   reads the new word reads the new actions.  No host-side wait in either call. */
int a0_host_device_pointer(void* host, void** dev);
int a0_env_pool_upload(const uint8_t* new_host, uint8_t* new_dev, const float* scal_host, float* scal_dev, int n_scal, int advance_row,
                       const uint8_t* obs_host, const uint8_t* prev, uint8_t* out, int E, int nstack, long long frame_bytes, int* n_whole,
                       void* stream);
int a0_env_pool_send(const int* action, int* act_host_dev, int E, long long* ctl_host_dev, long long word, void* stream);
/* a0_env_pool_upload with prev = NULL is its DMA-only form: the newest frames, the scalars and the whole stacks (into `out`) are copied, and the frame stack
 * is left to a0_host_step_ingest.  (prev, not out, marks it: out stays the destination of the whole stacks.)
 * a0_host_step_ingest: the ingest half of a host-env step in ONE launch, after the DMA-only upload of the step — what a0_env_frame_stack + a0_actor_nstep +
 *   a0_replay_insert + the two statistics copies leave, bit for bit:
 *   - out[e] = prev[e][1:] || newest[e] where scal[6][e] != 0 (rows with advance 0 were uploaded whole into out and are only read);
 *   - the n-step window of a0_actor_nstep (reward, terminal, truncated, life_loss = scal rows 0 - 3; life_loss ignored when use_life_loss == 0);
 *   - n > 1: ring_obs[steps % ring_len][e] = prev[e] (ring_obs: [ring_len][E][nstack * frame_bytes] u8, ring_len >= n);
 *   - the replay row at slot (start_slot + e) % cap: st = prev[e] (n = 1) or ring_obs[oldest][e], oldest = (steps - min(steps + 1, n) + 1) % ring_len
 *     (n > 1), st_next = out[e]; r_act / r_rew / r_done[slot] = the emitted n-step transition;
 *   - stat_mask[e] = scal[4][e], stat_ret[e] = scal[5][e] (pass the step's rows of the rollout's statistics).
 *   scal: [7][E] f32 in env_pool's N_SCAL order (reward, terminated, truncated, life_loss, final mask, final return, advance); frames: [cap][2][obs] u8;
 *   cap >= E.  ctrl adds its ACTOR_STEPS word to steps and its REPLAY_SLOT word to start_slot. */
int a0_host_step_ingest(const uint8_t* prev, const uint8_t* newest, const float* scal, uint8_t* out, int E, int nstack, long long frame_bytes,
                        int use_life_loss, const int* action, int n, int ring_len, long long steps, double gamma, int* ring_act, float* ring_rew,
                        float* ring_done, uint8_t* ring_obs, uint8_t* frames, long long cap, long long start_slot, int* r_act, float* r_rew,
                        float* r_done, float* stat_mask, float* stat_ret, const long long* ctrl, void* stream);

/* ---------------------------------------------------------------- device RNG + synthetic env (no reference counterpart) */
int a0_rng_u32(unsigned long long seed, unsigned int stream_id, unsigned long long offset, unsigned int* out, long long n, void* stream);
int a0_rng_uniform(unsigned long long seed, unsigned int stream_id, unsigned long long offset, float* out, long long n, void* stream);
int a0_rng_randint(unsigned long long seed, unsigned int stream_id, unsigned long long offset, int hi, int* out, long long n, void* stream);
int a0_rng_normal(unsigned long long seed, unsigned int stream_id, unsigned long long offset, float stdv, float* out, long long n, void* stream);
int a0_rng_uniform_ctrl(unsigned long long seed, unsigned int stream_id, unsigned long long offset, float* out, long long n, const long long* ctrl,
                        int ctrl_idx, void* stream);
int a0_rng_normal_ctrl(unsigned long long seed, unsigned int stream_id, unsigned long long offset, float stdv, float* out, long long n,
                       const long long* ctrl, int ctrl_idx, void* stream);
/* learner.aug_shift: DrQ's random shift of a sampled batch, in one launch.  frames / slot / row_bytes as in a0_learner_update (slot == NULL: rows 0 .. B - 1), a row
 * being st || st_next of C * H * W bytes each and nothing else (row_bytes == 2 * C * H * W); out: a dense [B][row_bytes] batch.  Every observation is shifted on its
 * own, all C planes alike: out[c][y][x] = in[c][clamp(y + dy, 0, H - 1)][clamp(x + dx, 0, W - 1)] — a replicate pad by `pad` and a crop at (dy + pad, dx + pad).
 * The draw: sample b of update u owns words 4 (u B + b) .. + 3 of Philox stream 7 of `seed` (a0_rng_u32's numbering, 64-bit positions): dy(st), dx(st), dy(st_next),
 * dx(st_next), each word % (2 pad + 1) - pad.  u = state[6] read on the device when state != NULL (the learner's status words: the update count its Adam launch
 * advances, so a replayed hipGraph moves on by itself), else u_host (>= 0).  A0_EINVAL: pad < 1, pad >= min(H, W), pad > 16, row_bytes != 2 * C * H * W,
 * C * H * W % 16 != 0 or >= 2^30, frames or out not 16-byte aligned.  `out` must not overlap the rows of `frames` the launch reads: the library cannot detect that,
 * and the result would depend on the order the workgroups run in.  slot values are not checked either (they index rows of `frames`, as in a0_learner_update). */
int a0_augment_shift(const uint8_t* frames, const int* slot, long long row_bytes, int C, int H, int W, int pad, int B, unsigned long long seed, const int* state,
                     long long u_host, uint8_t* out, void* stream);
/* Synthetic env (oracle/synth_env.c defines it).  `task` selects the reward: A0_ENV_TASK_STREAM = an action-independent stream (P(-1, +1, 0) = .05, .05, .9:
 * the bench workload), A0_ENV_TASK_BLOCK = learnable: +1 when the action equals the quadrant (mod A) of the bright 8x8 block in the newest frame of the
 * observation it was chosen on, -1 for the next class, 0 otherwise (chance level 0, optimum +1 per step).  Terminals / life losses do not depend on it. */
#define A0_ENV_TASK_STREAM 0
#define A0_ENV_TASK_BLOCK 1
/* (round 5) A0_ENV_TASK_CHASE = a task with TEMPORAL credit: the action MOVES the block on a 4 x 4 lattice (a % 4: up, down, left, right), +1 only on arrival at the
 * bottom-right cell, then a respawn three to six moves away; the env reads its state back from the newest frame of the observation (csrc/synth_env.h).  In the kernels
 * that merge the actor's tail with the env step the frame waves wait at a workgroup barrier for the action under this task (the other tasks' frames do not depend on
 * it and keep the barrier-free overlap). */
#define A0_ENV_TASK_CHASE 2
int a0_env_synth_reset(unsigned long long seed, unsigned int rank, int E, uint8_t* obs, float* ep_ret, void* stream);
int a0_env_synth_reset_task(unsigned long long seed, unsigned int rank, int E, uint8_t* obs, float* ep_ret, int task, void* stream);      /* (round 5) a0_env_synth_reset for `task`: the chase task's first frame shows the block at the env's start cell */
int a0_env_synth_step(unsigned long long seed, unsigned int rank, int E, unsigned int g, const uint8_t* obs_in, uint8_t* obs_out,
                      float* ep_ret, float* reward, float* terminal, float* truncated, float* life_loss, float* final_mask,
                      float* final_ret, const int* action, int A, int task, const long long* ctrl, void* stream);
/* a0_env_synth_step + a0_actor_nstep (agent.py:57-73) + a0_replay_insert (agent.py:78-81, replay.py:45-53) in one launch for rollouts
 * driven by the synthetic env: obs0 = first observation of the emitted transition (obs_in for n = 1).  ctrl adds its ENV_STEP,
 * ACTOR_STEPS and REPLAY_SLOT words to g, steps and start_slot. */
int a0_env_synth_step_commit(unsigned long long seed, unsigned int rank, int E, unsigned int g, const uint8_t* obs_in, uint8_t* obs_out, float* ep_ret,
                             float* final_mask, float* final_ret, int n, long long steps, double gamma, const int* action, int* ring_act,
                             float* ring_rew, float* ring_done, const uint8_t* obs0, uint8_t* frames, long long cap, long long start_slot, int* r_act,
                             float* r_rew, float* r_done, int A, int task, const long long* ctrl, void* stream);

/* ---------------------------------------------------------------- data-parallel gradient exchange (no reference counterpart)
 * One process per GPU; every rank holds a full replica and SUM-reduces its flat fp32 gradient buffer once per update over RCCL/xGMI.  The
 * reference reduces its loss by SUM (agent.py:154), so a SUM all-reduce with Adam eps = 1e-2/(world*B) is one reference step on the global
 * batch.  a0_dp_allreduce is enqueued on the caller's stream (in place, asynchronous, capturable into the update's hipGraph).  Rendezvous:
 * rank 0 fills a 128-byte HOST blob with a0_dp_unique_id and hands it to the other ranks by its own means; every rank then calls a0_dp_init
 * (collective; binds to the calling thread's current device) and gets an opaque communicator handle, 0 on error. */
int a0_dp_unique_id(void* host_id128);
long long a0_dp_init(const void* host_id128, int rank, int world);
int a0_dp_allreduce(long long comm, float* buf, long long n, void* stream);
int a0_dp_destroy(long long comm);
/* (round 5) what RCCL reports for the communicator: host_out3 = {ncclCommCount, ncclCommUserRank, ncclCommCuDevice}; bench.py prints it beside an all-reduce of ones */
int a0_dp_info(long long comm, int* host_out3);

#ifdef __cplusplus
}
#endif
#endif /* AGENT0_HIP_H */
