// Optimizer, NaN guard and target-network sync over the flat parameter buffer (gfx950).
// Restates reference agent0/deepq/agent.py:102-106 (Adam lr 5e-4, eps 1e-2/B), :333-338 (RMSprop for the FQF
// fraction net), :152-158 (skip the step when any per-sample loss is NaN) and :160-161 (target <- online every
// target_update_freq successful updates) without the two host syncs per update the reference pays (quirk Q14):
// the NaN flag, the step counter and the "sync now" decision all live in a small device-side state block.
// Resets and ReDo recycling of the same buffer: net_reset.hip.  NoisyNet: noisy.hip.
#include "a0_internal.h"
#include "update_tail.h"

#include <algorithm>
#include <type_traits>

// state block (ints): see a0_learner_state in include/agent0_hip.h
//   [0] nan_flag      set by the loss kernels (atomicOr) when a per-sample loss is NaN
//   [1] update_steps  successful optimizer steps so far (reference BaseLearner.update_steps)
//   [2] skipped       number of updates skipped because of NaN
//   [3] skip_now      decision for the update in flight (1 = NaN seen, leave the parameters alone)
//   [4] sync_now      1 if update_steps % target_update_freq == 0 after this update
//   [7] reset_steps   update_steps at the last network reset (a0_net_reset); Adam's bias corrections count t = max(1, update_steps - reset_steps)
// scalars (floats): [0] step_size = lr / (1 - b1^t), [1] bc2_sqrt = sqrt(1 - b2^t)
// extra_flag (optional): a float that is nonzero when ANY data-parallel rank saw a NaN — the sum over ranks of a0_nan_flag_export's
// output, which travels at the tail of the dense gradient bucket instead of in an all-reduce of its own.
// The decisions themselves: a0_step_decide / a0_step_publish (update_tail.h).
__global__ void a0_adam_prep_kernel(int* __restrict__ state, float* __restrict__ scal, double lr, double b1, double b2, int target_freq,
                                    const float* __restrict__ extra_flag) {
    if (threadIdx.x != 0 || blockIdx.x != 0) return;
    a0_step_publish(a0_step_decide(state, extra_flag, lr, b1, b2, target_freq), state, scal, true);
}

// ---- Adam's element.  The library steps a parameter in exactly TWO arithmetic forms, each written out here — fused where __builtin_fmaf says so, rounded products
// everywhere else — so that no choice of the compiler's contraction can part two kernels that must agree bit for bit (the one-launch tail against the three-launch
// chain, tests/test_gpu_update_tail.py; a0_adam_step against a0_adam_step_sync, tests/test_gpu_adam_forms.py):
//   * a0_adam_wide: both moments and the step fused.  Every group of four parameters that moves as 16 bytes: n, n_total multiples of four, every buffer 16-byte aligned.
//   * a0_adam_scalar: both moments from rounded products plus an add, the step fused.  Everything stepped element by element, and all of a0_adam_step.
// They differ because that is how the two paths were first compiled, and a buffer's bits must not depend on which kernel steps it; making them one form would
// change the results of the scalar path.
struct a0_adam_hyper { float w1, b2, w2, eps; };
static a0_adam_hyper a0_adam_hyper_of(double beta1, double beta2, double eps) { return a0_adam_hyper{(float)(1.0 - beta1), (float)beta2, (float)(1.0 - beta2), (float)eps}; }

A0_D void a0_adam_wide(float& p, float& m, float& v, float gi, const a0_adam_hyper& H, const a0_step& S) {
#pragma clang fp contract(off)
    const float w1 = H.w1, b2 = H.b2, w2 = H.w2;
    float mi = m, vi = v;
    mi = __builtin_fmaf(gi - mi, w1, mi);
    vi = __builtin_fmaf(w2 * gi, gi, vi * b2);
    const float denom = sqrtf(vi) / S.bc2_sqrt + H.eps;
    p = __builtin_fmaf(-S.step_size, mi / denom, p);
    m = mi; v = vi;
}
A0_D void a0_adam_scalar(float& p, float& m, float& v, float gi, const a0_adam_hyper& H, const a0_step& S) {
#pragma clang fp contract(off)
    const float w1 = H.w1, b2 = H.b2, w2 = H.w2;
    float mi = m, vi = v;
    mi = mi + (gi - mi) * w1;
    vi = vi * b2 + (w2 * gi) * gi;
    const float denom = sqrtf(vi) / S.bc2_sqrt + H.eps;
    p = __builtin_fmaf(-S.step_size, mi / denom, p);
    m = mi; v = vi;
}

// the 16-byte path of the Adam forms: n, n_total multiples of four and every buffer 16-byte aligned
static int a0_adam_vec4(const float* params, const float* grads, const float* exp_avg, const float* exp_avg_sq, const float* target, long long n, long long n_total) {
    return ((n | n_total) % 4 == 0) && a0_aligned(16, params, grads, exp_avg, exp_avg_sq, target);
}

// The sum of 256 lanes' values through LDS: store, then the tree o = 128 ... 1 with a barrier per step; the result is red[0], in the one order every sum here has
template <class T>
A0_D void a0_block_sum256(T* red, T v) {
    red[threadIdx.x] = v;
    __syncthreads();
    for (int o = 128; o > 0; o >>= 1) { if ((int)threadIdx.x < o) red[threadIdx.x] += red[threadIdx.x + o]; __syncthreads(); }
}

__global__ void a0_adam_kernel(float* __restrict__ p, const float* __restrict__ g, float* __restrict__ m, float* __restrict__ v,
                               long long n, const int* __restrict__ state, const float* __restrict__ scal, a0_adam_hyper H) {
    const a0_step S = a0_step_published(state, scal);
    if (S.skip) return;
    long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    const long long stride = (long long)gridDim.x * blockDim.x;
    for (; i < n; i += stride) a0_adam_scalar(p[i], m[i], v[i], g[i], H, S);
}

extern "C" int a0_adam_step(float* params, const float* grads, float* exp_avg, float* exp_avg_sq, long long n, int* state, float* scalars,
                            double lr, double beta1, double beta2, double eps, int target_update_freq, void* stream) {
    if (!params || !grads || !exp_avg || !exp_avg_sq || !state || !scalars || n < 1) return a0_fail(A0_EINVAL, "a0_adam_step: bad argument");
    hipStream_t st = (hipStream_t)stream;
    hipLaunchKernelGGL(a0_adam_prep_kernel, dim3(1), dim3(1), 0, st, state, scalars, lr, beta1, beta2, target_update_freq, (const float*)nullptr);
    hipLaunchKernelGGL(a0_adam_kernel, dim3(a0_grid_256(n)), dim3(256), 0, st, params, grads, exp_avg, exp_avg_sq, n, state, scalars, a0_adam_hyper_of(beta1, beta2, eps));
    return a0_fail_hip((int)hipGetLastError(), "a0_adam_step");
}

// Adam with the target copy folded in: when the step's decision says "sync now" (update_steps % target_update_freq == 0, agent.py:160-161) every element's NEW
// value is also written to the target buffer, over [0, n_total) — n_total > n covers blocks Adam does not own (FQF's fraction net).  A skipped (NaN) step leaves the
// parameters alone but still syncs, like the reference.
// FOLD: no a0_adam_prep_kernel in front.  Every workgroup derives the step's decisions and scalars itself — from words nobody writes during this kernel — and
// workgroup 0 publishes them without committing (a0_step_publish).
struct a0_adam_fold { double lr, b1, b2; int target_freq; const float* extra_flag; int* state_w; float* scal_w; const float* loss; int loss_n; float* loss_ring; int ring_cap; };

// Global gradient-norm clipping (learner.clip_grad_norm; torch.nn.utils.clip_grad_norm_ with its defaults), stage 1: the sum of squares of g[0, n) as
// A0_GRAD_NORM_PARTIALS partial sums.  Workgroup b owns the elements [b * chunk, (b + 1) * chunk) — chunk a multiple of four, a function of n alone — and writes
// partials[b] with a plain store (0 when its range is empty): no atomics, no "last workgroup" counter, and the same bits on every run.  Squares and sums are doubles:
// the square of a float is exact in double, so the only rounding of the norm that matters is stage 2's final cast.  vec4: g is 16-byte aligned (16-byte loads, a
// scalar tail); otherwise element by element.
// The walk itself, for every kernel of this shape.  T: float or const float; `each(at, x)` sees every value x the walk has read at `at` (an a0_f4 on the 16-byte
// path) once its squares are added, and stores there what it likes.
template <class T, class F>
A0_D void a0_chunk_sumsq(T* __restrict__ x, long long n, long long chunk, int vec4, double* __restrict__ partials, F each) {
    using T4 = std::conditional_t<std::is_const_v<T>, const a0_f4, a0_f4>;
    __shared__ double red[256];
    const long long lo = (long long)blockIdx.x * chunk;
    const long long hi = lo + chunk < n ? lo + chunk : n;
    double s = 0.0;
    if (lo < hi) {
        long long done = 0;
        if (vec4) {
            const long long n4 = (hi - lo) >> 2;
            T4* x4 = (T4*)(x + lo);
            for (long long j = threadIdx.x; j < n4; j += 256) {
                const a0_f4 v = x4[j];
                s += (double)v.x * (double)v.x; s += (double)v.y * (double)v.y; s += (double)v.z * (double)v.z; s += (double)v.w * (double)v.w;
                each(x4 + j, v);
            }
            done = n4 << 2;
        }
        for (long long i = lo + done + threadIdx.x; i < hi; i += 256) {
            const float v = x[i];
            s += (double)v * (double)v;
            each(x + i, v);
        }
    }
    a0_block_sum256(red, s);
    if (threadIdx.x == 0) partials[blockIdx.x] = red[0];
}
// ... and its launch: A0_GRAD_NORM_PARTIALS workgroups of 256, chunk from n alone, the 16-byte path for a 16-byte aligned buffer; `rest`: the kernel's own arguments
template <class K, class T, class... A>
static void a0_chunk_sumsq_launch(K kernel, T* x, long long n, void* stream, A... rest) {
    const long long chunk = ((n + A0_GRAD_NORM_PARTIALS - 1) / A0_GRAD_NORM_PARTIALS + 3) / 4 * 4;
    hipLaunchKernelGGL(kernel, dim3(A0_GRAD_NORM_PARTIALS), dim3(256), 0, (hipStream_t)stream, x, n, chunk, a0_aligned(16, x) ? 1 : 0, rest...);
}

__global__ __launch_bounds__(256) void a0_grad_sumsq_kernel(const float* __restrict__ g, long long n, long long chunk, int vec4, double* __restrict__ partials) {
    a0_chunk_sumsq(g, n, chunk, vec4, partials, [](const void*, const auto&) {});      // the sums alone: nothing to store
}

extern "C" int a0_grad_norm_partials(const float* grads, long long n, double* partials, void* stream) {
    if (!grads || !partials || n < 1 || !a0_aligned(4, grads) || !a0_aligned(8, partials)) return a0_fail(A0_EINVAL, "a0_grad_norm_partials: bad argument");
    a0_chunk_sumsq_launch(a0_grad_sumsq_kernel, grads, n, stream, partials);
    return a0_fail_hip((int)hipGetLastError(), "a0_grad_norm_partials");
}

// Decoupled weight decay (learner.weight_decay; torch.optim.AdamW's p <- p * (1 - lr * lambda) in front of its Adam step), ONE launch in front of the update's Adam
// form, in a0_grad_sumsq_kernel's shape: workgroup b owns [b * chunk, (b + 1) * chunk) of p[0, n), shrinks it by c = fl32(lr * lambda) — t = fl32(c * p), then
// p <- fl32(p - t): one rounded product (a0_mul_rounded) and one rounded subtraction — and writes the sum of the squares of the values it READ to partials[b]
// (doubles, plain stores, 0 for an empty range): the parameter norm in front of the decay, finished on the host.  The kernel decides "skipped" for itself as
// a0_step_decide does, from words nobody writes while it runs: the NaN flag state[0], which the Adam form behind lowers, and the optional data-parallel flag.  A
// skipped update stores no parameter; its partials are written all the same.
A0_D float a0_decay1(float p, float c) {
    const float t = a0_mul_rounded(c, p);
    float r;
    {
#pragma clang fp contract(off)
        r = p - t;
    }
    return r;
}
struct a0_decay_each {
    float c; bool skip;
    A0_D void operator()(float* at, float x) const { if (!skip) *at = a0_decay1(x, c); }
    A0_D void operator()(a0_f4* at, a0_f4 x) const {
        if (!skip) { x.x = a0_decay1(x.x, c); x.y = a0_decay1(x.y, c); x.z = a0_decay1(x.z, c); x.w = a0_decay1(x.w, c); *at = x; }
    }
};
__global__ __launch_bounds__(256) void a0_weight_decay_kernel(float* __restrict__ p, long long n, long long chunk, int vec4, float c, const int* __restrict__ state,
                                                              const float* __restrict__ extra_flag, double* __restrict__ partials) {
    const bool skip = (state[0] != 0) || (extra_flag && extra_flag[0] != 0.f);
    a0_chunk_sumsq(p, n, chunk, vec4, partials, a0_decay_each{c, skip});
}

// c: lr * lambda as the caller formed it in double; rounded to fp32 once here.  2^-24 <= fl32(c) < 1: a smaller c moves no fp32 value, c >= 1 is no decay
extern "C" int a0_weight_decay(float* params, long long n, double c, const int* state, const float* extra_nan_flag, double* partials, void* stream) {
    if (!params || !state || !partials || n < 1 || !a0_aligned(4, params) || !a0_aligned(8, partials)) return a0_fail(A0_EINVAL, "a0_weight_decay: bad argument");
    const float c32 = (float)c;
    if (!(c32 >= 0x1p-24f) || !(c32 < 1.f)) return a0_fail(A0_EINVAL, "a0_weight_decay: c = lr * lambda must lie in [2^-24, 1) as an fp32 number");
    a0_chunk_sumsq_launch(a0_weight_decay_kernel, params, n, stream, c32, state, extra_nan_flag, partials);
    return a0_fail_hip((int)hipGetLastError(), "a0_weight_decay");
}

// The batch mean of this update's per-sample losses (the Trainer's `loss` statistic, trainer.py:99,111-113) into the ring slot of the free-running call counter
// state[6], by ONE workgroup of 256 lanes — the same reduction, statement for statement, as a0_mean_rows_kernel, whose launch per update (4.8 us of pure latency)
// it replaces.  Skipped steps are recorded too (their mean is whatever the loss kernel wrote, NaN included).
A0_D void a0_loss_mean_to_ring(const float* loss, int loss_n, float* loss_ring, int ring_cap, int* state_w) {
    __shared__ float red[256];
    float s = 0.f;
    for (int e = threadIdx.x; e < loss_n; e += 256) s += loss[e];
    a0_block_sum256(red, s);
    if (threadIdx.x == 0) { const int c = state_w[6]; loss_ring[c % ring_cap] = red[0] / (float)loss_n; state_w[6] = c + 1; }
}

// stage 2 (CLIP): every workgroup sums the partials in the same order, so all of them step on the same coefficient; workgroup 0 files the norm
struct a0_adam_clip { const double* partials; float max_norm; float* norm_ring; int ring_cap; };
template <bool FOLD, bool CLIP>
__global__ void a0_adam_sync_kernel(float* __restrict__ p, const float* __restrict__ g, float* __restrict__ m, float* __restrict__ v,
                                    long long n, const int* __restrict__ state, const float* __restrict__ scal,
                                    a0_adam_hyper H, float* __restrict__ target, long long n_total, int vec4, a0_adam_fold F, a0_adam_clip K) {
    a0_step S;
    float coef = 1.f;
    if constexpr (CLIP) {
        // ||g|| = sqrt(sum of the partials), rounded to fp32 once; coef = min(1, max_norm / (||g|| + 1e-6)) in fp32.  The pre-clip norm goes to ring slot
        // state[6] % cap — the slot of this update's loss mean, read before workgroup 0 advances the counter below — on skipped (NaN) steps too.
        static_assert(A0_GRAD_NORM_PARTIALS == 256, "one partial per lane of the 256-lane workgroup");
        __shared__ double cred[256];
        a0_block_sum256(cred, K.partials[threadIdx.x]);
        const float norm = (float)sqrt(cred[0]);
        if (blockIdx.x == 0 && threadIdx.x == 0) K.norm_ring[(FOLD ? F.state_w[6] : state[6]) % K.ring_cap] = norm;
        const float c = K.max_norm / (norm + 1e-6f);
        coef = c < 1.f ? c : 1.f;
    }
    if constexpr (FOLD) {
        __shared__ a0_step sh;
        if (blockIdx.x == 0 && F.loss) a0_loss_mean_to_ring(F.loss, F.loss_n, F.loss_ring, F.ring_cap, F.state_w);
        if (threadIdx.x == 0) {
            sh = a0_step_decide(state, F.extra_flag, F.lr, F.b1, F.b2, F.target_freq);
            if (blockIdx.x == 0) a0_step_publish(sh, F.state_w, F.scal_w, false);
        }
        __syncthreads();
        S = sh;
    } else {
        S = a0_step_published(state, scal);
    }
    const bool skip = S.skip != 0, sync = S.sync != 0;
    if (skip && !sync) return;
    long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    const long long stride = (long long)gridDim.x * blockDim.x;
    const long long end = sync ? n_total : n;
    if (vec4) {                     // 16 bytes per lane (a0_adam_vec4)
        const long long n4 = n >> 2, end4 = end >> 2;
        for (; i < end4; i += stride) {
            a0_f4 pv = ((a0_f4*)p)[i];
            if (i < n4 && !skip) {
                const a0_f4 gv = ((const a0_f4*)g)[i];
                a0_f4 mv = ((a0_f4*)m)[i], vv = ((a0_f4*)v)[i];
                float* pp = &pv.x; const float* gp = &gv.x; float* mp = &mv.x; float* vp = &vv.x;
#pragma unroll
                for (int e = 0; e < 4; ++e) a0_adam_wide(pp[e], mp[e], vp[e], CLIP ? a0_mul_rounded(gp[e], coef) : gp[e], H, S);
                ((a0_f4*)p)[i] = pv; ((a0_f4*)m)[i] = mv; ((a0_f4*)v)[i] = vv;
            }
            if (sync) ((a0_f4*)target)[i] = pv;
        }
        return;
    }
    for (; i < end; i += stride) {
        float pi = p[i];
        if (i < n && !skip) {
            a0_adam_scalar(pi, m[i], v[i], CLIP ? a0_mul_rounded(g[i], coef) : g[i], H, S);
            p[i] = pi;
        }
        if (sync) target[i] = pi;
    }
}

static bool a0_clip_args_ok(const double* partials, float max_norm, const float* norm_ring, int norm_ring_cap) {
    return partials && a0_aligned(8, partials) && max_norm > 0.f && norm_ring && norm_ring_cap >= 1;
}

// The one launcher of the four instantiations.  Plain (wt == nullptr): the one-thread prep kernel in front, == a0_adam_step + a0_target_sync.  Folded (the optimizer
// tail of a network with fused-kernel weight copies, in TWO launches): Adam with the step's bookkeeping and the loss mean folded in, then the refresh of the online
// net's weight copies (mirrored into the target's on a sync step), which also commits the step counter; == a0_adam_step_sync + a0_net_conv_wt_refresh_sync.
// clip (optional): a0_adam_step_sync on g * min(1, max_norm / (||g|| + 1e-6)), ||g|| from the partials a0_grad_norm_partials left for this gradient buffer.
int a0_conv_wt_refresh_commit(const a0_encoder_weights* w, int C, float* wt, float* wt_target, int* state, hipStream_t st);      // encoder_fused.hip
struct a0_adam_wt { const a0_encoder_weights* w; int C; float *wt, *wt_target; const float* loss; int loss_n; float* loss_ring; int ring_cap; };
static int a0_adam_sync_launch(const char* who, float* params, const float* grads, float* exp_avg, float* exp_avg_sq, long long n, int* state, float* scalars,
                               double lr, double beta1, double beta2, double eps, int target_update_freq, float* target, long long n_total,
                               const float* extra_nan_flag, const a0_adam_wt* wt, const a0_adam_clip* clip, void* stream) {
    if (!params || !grads || !exp_avg || !exp_avg_sq || !state || !scalars || !target || n < 1 || n_total < n || (wt && (!wt->w || !wt->wt || !wt->wt_target || wt->C < 1)))
        return a0_fail(A0_EINVAL, who);
    if (wt && wt->loss && (!wt->loss_ring || wt->loss_n < 1 || wt->ring_cap < 1)) return a0_fail(A0_EINVAL, "a0_adam_step_sync_wt: loss statistics need a ring of at least one slot");
    hipStream_t st = (hipStream_t)stream;
    a0_adam_fold F{0.0, 0.0, 0.0, 0, nullptr, nullptr, nullptr, nullptr, 0, nullptr, 1};
    if (wt) F = a0_adam_fold{lr, beta1, beta2, target_update_freq, extra_nan_flag, state, scalars, wt->loss, wt->loss_n, wt->loss_ring, wt->ring_cap > 0 ? wt->ring_cap : 1};
    else hipLaunchKernelGGL(a0_adam_prep_kernel, dim3(1), dim3(1), 0, st, state, scalars, lr, beta1, beta2, target_update_freq, extra_nan_flag);
    const int vec4 = a0_adam_vec4(params, grads, exp_avg, exp_avg_sq, target, n, n_total);
    const auto kernel = wt ? (clip ? a0_adam_sync_kernel<true, true> : a0_adam_sync_kernel<true, false>) : (clip ? a0_adam_sync_kernel<false, true> : a0_adam_sync_kernel<false, false>);
    hipLaunchKernelGGL(kernel, dim3(a0_grid_256(vec4 ? n_total / 4 : n_total)), dim3(256), 0, st, params, grads, exp_avg, exp_avg_sq, n, (const int*)state, (const float*)scalars,
                       a0_adam_hyper_of(beta1, beta2, eps), target, n_total, vec4, F, clip ? *clip : a0_adam_clip{nullptr, 0.f, nullptr, 1});
    const int e = a0_fail_hip((int)hipGetLastError(), who);
    return (e != A0_OK || !wt) ? e : a0_conv_wt_refresh_commit(wt->w, wt->C, wt->wt, wt->wt_target, state, st);
}

extern "C" int a0_adam_step_sync(float* params, const float* grads, float* exp_avg, float* exp_avg_sq, long long n, int* state, float* scalars,
                                 double lr, double beta1, double beta2, double eps, int target_update_freq, float* target, long long n_total,
                                 const float* extra_nan_flag, void* stream) {
    return a0_adam_sync_launch("a0_adam_step_sync: bad argument", params, grads, exp_avg, exp_avg_sq, n, state, scalars, lr, beta1, beta2, eps, target_update_freq, target, n_total,
                               extra_nan_flag, nullptr, nullptr, stream);
}

extern "C" int a0_adam_step_sync_clip(float* params, const float* grads, float* exp_avg, float* exp_avg_sq, long long n, int* state, float* scalars,
                                      double lr, double beta1, double beta2, double eps, int target_update_freq, float* target, long long n_total,
                                      const float* extra_nan_flag, const double* partials, float max_norm, float* norm_ring, int norm_ring_cap, void* stream) {
    if (!a0_clip_args_ok(partials, max_norm, norm_ring, norm_ring_cap)) return a0_fail(A0_EINVAL, "a0_adam_step_sync_clip: partials, max_norm > 0 and a norm ring of at least one slot");
    const a0_adam_clip clip{partials, max_norm, norm_ring, norm_ring_cap};
    return a0_adam_sync_launch("a0_adam_step_sync_clip: bad argument", params, grads, exp_avg, exp_avg_sq, n, state, scalars, lr, beta1, beta2, eps, target_update_freq, target, n_total,
                               extra_nan_flag, nullptr, &clip, stream);
}

extern "C" int a0_adam_step_sync_wt(float* params, const float* grads, float* exp_avg, float* exp_avg_sq, long long n, int* state, float* scalars,
                                    double lr, double beta1, double beta2, double eps, int target_update_freq, float* target, long long n_total,
                                    const float* extra_nan_flag, const a0_encoder_weights* w, int C, float* wt, float* wt_target, const float* loss, int loss_n,
                                    float* loss_ring, int ring_cap, void* stream) {
    const a0_adam_wt fold{w, C, wt, wt_target, loss, loss_n, loss_ring, ring_cap};
    return a0_adam_sync_launch("a0_adam_step_sync_wt: bad argument", params, grads, exp_avg, exp_avg_sq, n, state, scalars, lr, beta1, beta2, eps, target_update_freq, target, n_total,
                               extra_nan_flag, &fold, nullptr, stream);
}

// the norm goes to norm_ring[state[6] % norm_ring_cap], beside the loss mean's slot
extern "C" int a0_adam_step_sync_wt_clip(float* params, const float* grads, float* exp_avg, float* exp_avg_sq, long long n, int* state, float* scalars,
                                         double lr, double beta1, double beta2, double eps, int target_update_freq, float* target, long long n_total,
                                         const float* extra_nan_flag, const a0_encoder_weights* w, int C, float* wt, float* wt_target, const float* loss, int loss_n,
                                         float* loss_ring, int ring_cap, const double* partials, float max_norm, float* norm_ring, int norm_ring_cap, void* stream) {
    if (!a0_clip_args_ok(partials, max_norm, norm_ring, norm_ring_cap)) return a0_fail(A0_EINVAL, "a0_adam_step_sync_wt_clip: partials, max_norm > 0 and a norm ring of at least one slot");
    const a0_adam_wt fold{w, C, wt, wt_target, loss, loss_n, loss_ring, ring_cap};
    const a0_adam_clip clip{partials, max_norm, norm_ring, norm_ring_cap};
    return a0_adam_sync_launch("a0_adam_step_sync_wt_clip: bad argument", params, grads, exp_avg, exp_avg_sq, n, state, scalars, lr, beta1, beta2, eps, target_update_freq, target, n_total,
                               extra_nan_flag, &fold, &clip, stream);
}

// ------------------------------------------------------------------------------------------------ the update tail in one launch
// a0_reduce_segments_kernel + a0_adam_sync_kernel<true, false> + a0_conv_wt_kernel as ONE kernel without a second pass over anything: [0, n_total) is cut into
// regions — the planned slab segments, and the ranges between them — and every workgroup serves one piece of one region:
//   * segment, 16-byte path: 128 parameters — eight row groups x 32 lanes form the sums as a0_reduce_segments_kernel does, row group 0 adds the eight partial sums
//     0..7 from zero, writes the gradient and steps its four parameters on it; scalar path: 32 parameters likewise;
//   * between segments: a0_adam_sync_kernel's body, 1024 parameters per workgroup on the 16-byte path, 256 on the scalar path.
// The step's decisions were derived one launch earlier (a0_tail_prep_run): state[3], state[4] and the scalars are only read here, so there is nothing to commit and
// no workgroup waits for another.  The lane that holds a new convolution weight also files it in the fused kernels' copies (a0_wt_sink and a0_tail_wt*: update_tail.h).
struct a0_tail_region { long long lo, hi; int first_block, seg, vec, pad_; };      // [lo, hi) of the flat buffer; seg < 0: not a slab segment
struct a0_tail_args {
    float *p, *g, *m, *v, *target;
    long long n, n_total;
    const int* state; const float* scal;
    a0_adam_hyper H;
    int vec4;                                   // a0_adam_vec4
    a0_reduce_seg seg[8];
    a0_tail_region reg[17];
    int nreg;
    const float* loss; int loss_n; float* loss_ring; int ring_cap; int* state_w;
    a0_wt_sink W;
};

// a0_adam_sync_kernel's body for float4 i of the flat buffer; HAVE_G: the gradient is the sum this lane has just formed
template <bool HAVE_G>
A0_D void a0_tail_adam4(const a0_tail_args& A, const a0_step& S, long long i, a0_f4 gsum) {
    const long long n4 = A.n >> 2, end4 = (S.sync ? A.n_total : A.n) >> 2;
    if ((S.skip && !S.sync) || i >= end4) return;
    a0_f4 pv = ((a0_f4*)A.p)[i];
    if (i < n4 && !S.skip) {
        a0_f4 gv;
        if constexpr (HAVE_G) gv = gsum; else gv = ((const a0_f4*)A.g)[i];
        a0_f4 mv = ((a0_f4*)A.m)[i], vv = ((a0_f4*)A.v)[i];
        float* pp = &pv.x; const float* gp = &gv.x; float* mp = &mv.x; float* vp = &vv.x;
#pragma unroll
        for (int e = 0; e < 4; ++e) a0_adam_wide(pp[e], mp[e], vp[e], gp[e], A.H, S);
        ((a0_f4*)A.p)[i] = pv; ((a0_f4*)A.m)[i] = mv; ((a0_f4*)A.v)[i] = vv;
    }
    if (S.sync) ((a0_f4*)A.target)[i] = pv;
    a0_tail_wt_f4(A.W, !S.skip, S.sync, 4 * i, pv);
}
// ... and for one float
template <bool HAVE_G>
A0_D void a0_tail_adam1(const a0_tail_args& A, const a0_step& S, long long i, float gsum) {
    const long long end = S.sync ? A.n_total : A.n;
    if ((S.skip && !S.sync) || i >= end) return;
    float pi = A.p[i];
    if (i < A.n && !S.skip) {
        a0_adam_scalar(pi, A.m[i], A.v[i], HAVE_G ? gsum : A.g[i], A.H, S);
        A.p[i] = pi;
    }
    if (S.sync) A.target[i] = pi;
    a0_tail_wt1(A.W, !S.skip, S.sync, i, pi);
}
// a sum leaves as a plain register value, as a loaded gradient would arrive
A0_D float a0_tail_settle(float r) { asm volatile("" : "+v"(r)); return r; }

__global__ __launch_bounds__(256) void a0_update_tail_kernel(a0_tail_args A) {
    __shared__ a0_f4 red4[8][33];
    if (blockIdx.x == 0 && A.loss) a0_loss_mean_to_ring(A.loss, A.loss_n, A.loss_ring, A.ring_cap, A.state_w);
    const a0_step S = a0_step_published(A.state, A.scal);
    int ri = 0;
    for (int k = 1; k < A.nreg; ++k) ri += ((int)blockIdx.x >= A.reg[k].first_block) ? 1 : 0;
    const a0_tail_region R = A.reg[ri];
    const long long blk = (long long)((int)blockIdx.x - R.first_block);
    if (R.seg < 0) {           // between the segments
        if (R.vec) {
            const long long i4 = (R.lo >> 2) + blk * 256 + threadIdx.x;
            if (i4 < (R.hi >> 2)) a0_tail_adam4<false>(A, S, i4, a0_zero4());
        } else {
            const long long i = R.lo + blk * 256 + threadIdx.x;
            if (i < R.hi) a0_tail_adam1<false>(A, S, i, 0.f);
        }
        return;
    }
    const a0_reduce_seg G = A.seg[R.seg];
    const int c = threadIdx.x & 31, g = threadIdx.x >> 5;
    if (R.vec) {
        const long long i4 = blk * 32 + c;                    // float4 index in the segment
        const long long n4 = G.count >> 2, st4 = G.slab_stride >> 2;
        red4[g][c] = i4 < n4 ? a0_rowgroup_sum4((const a0_f4*)G.slabs + i4, st4, g, G.nslab) : a0_zero4();
        __syncthreads();
        if (g == 0 && i4 < n4) {
            a0_f4 t = a0_zero4();
#pragma unroll
            for (int j = 0; j < 8; ++j) { const a0_f4 v = red4[j][c]; t.x += v.x; t.y += v.y; t.z += v.z; t.w += v.w; }
            ((a0_f4*)G.out)[i4] = t;
            t.x = a0_tail_settle(t.x); t.y = a0_tail_settle(t.y); t.z = a0_tail_settle(t.z); t.w = a0_tail_settle(t.w);
            if (A.vec4) a0_tail_adam4<true>(A, S, (R.lo >> 2) + i4, t);
            else {
                const long long i = R.lo + 4 * i4;
                a0_tail_adam1<true>(A, S, i, t.x); a0_tail_adam1<true>(A, S, i + 1, t.y); a0_tail_adam1<true>(A, S, i + 2, t.z); a0_tail_adam1<true>(A, S, i + 3, t.w);
            }
        }
        return;
    }
    // scalar path: 32 flat indices per workgroup from R.lo on — the segment's first float, rounded down to a multiple of four where Adam takes its 16-byte form, so
    // that every aligned group of four parameters is stepped by ONE lane with a0_adam_wide, as a0_adam_sync_kernel would step it; which lane forms an
    // output's sum does not change the sum
    float* red = (float*)red4;                                 // [8][33] floats
    const long long F = R.lo + blk * 32 + c, i = F - (G.out - A.g);
    const bool in = i >= 0 && i < G.count;
    red[g * 33 + c] = in ? a0_rowgroup_sum1(G.slabs + i, G.slab_stride, g, G.nslab) : 0.f;
    __syncthreads();
    float t = 0.f;
    if (g == 0 && in) {
#pragma unroll
        for (int j = 0; j < 8; ++j) t += red[j * 33 + c];
        G.out[i] = t;
        t = a0_tail_settle(t);
        if (!A.vec4) a0_tail_adam1<true>(A, S, F, t);
    }
    if (!A.vec4) return;
    __syncthreads();
    if (g == 0 && F < R.hi) red[c] = in ? t : A.g[F];          // a neighbour outside the segment: its gradient is final in memory
    __syncthreads();
    if (g == 0 && (c & 3) == 0 && F < R.hi) a0_tail_adam4<true>(A, S, F >> 2, a0_f4{red[c], red[c + 1], red[c + 2], red[c + 3]});
}

extern "C" int a0_update_tail(float* params, float* grads, float* exp_avg, float* exp_avg_sq, long long n, int* state, const float* scalars, double beta1, double beta2,
                              double eps, float* target, long long n_total, const a0_update_tail_plan* plan, const a0_encoder_weights* w, int C, float* wt, float* wt_target,
                              const float* loss, int loss_n, float* loss_ring, int ring_cap, void* stream) {
    if (!params || !grads || !exp_avg || !exp_avg_sq || !state || !scalars || !target || n < 1 || n_total < n || !plan || plan->n < 0 || plan->n > 8 || !wt)
        return a0_fail(A0_EINVAL, "a0_update_tail: bad argument");
    if (loss && (!loss_ring || loss_n < 1 || ring_cap < 1)) return a0_fail(A0_EINVAL, "a0_update_tail: loss statistics need a ring of at least one slot");
    a0_tail_args A;
    A.p = params; A.g = grads; A.m = exp_avg; A.v = exp_avg_sq; A.target = target; A.n = n; A.n_total = n_total;
    A.state = state; A.scal = scalars; A.H = a0_adam_hyper_of(beta1, beta2, eps);
    A.vec4 = a0_adam_vec4(params, grads, exp_avg, exp_avg_sq, target, n, n_total);
    A.loss = loss; A.loss_n = loss_n; A.loss_ring = loss_ring; A.ring_cap = ring_cap > 0 ? ring_cap : 1; A.state_w = state;
    if (int e = a0_wt_sink_make(&A.W, "a0_update_tail", "params", params, n_total, w, C, wt, wt_target)) return e;
    // the segments in the order of their place in the flat buffer, the ranges between them, and each region's share of the grid
    int order[8];
    for (int k = 0; k < plan->n; ++k) {
        const a0_reduce_seg& s = plan->seg[k];
        if (!s.slabs || !s.out || s.nslab < 1 || s.count < 1 || s.out < grads || (s.out - grads) + s.count > n_total) return a0_fail(A0_EINVAL, "a0_update_tail: a segment outside grads[0, n_total)");
        A.seg[k] = s; order[k] = k;
    }
    for (int k = plan->n; k < 8; ++k) A.seg[k] = a0_reduce_seg{nullptr, 0, 0, nullptr, 0};
    std::sort(order, order + plan->n, [&](int a, int b) { return plan->seg[a].out < plan->seg[b].out; });
    long long at = 0, blocks = 0;
    int nreg = 0;
    auto gap = [&](long long lo, long long hi) {
        if (lo >= hi) return;
        const int vec = A.vec4 && lo % 4 == 0 && hi % 4 == 0;
        A.reg[nreg++] = a0_tail_region{lo, hi, (int)blocks, -1, vec, 0};
        blocks += vec ? ((hi - lo) / 4 + 255) / 256 : (hi - lo + 255) / 256;
    };
    for (int j = 0; j < plan->n; ++j) {
        const a0_reduce_seg& s = plan->seg[order[j]];
        long long lo = s.out - grads, hi = lo + s.count;
        // a0_reduce_segments_kernel's choice of path
        const int vec = ((s.count | s.slab_stride) % 4 == 0) && a0_aligned(16, s.slabs, s.out);
        if (!vec && A.vec4) { lo = lo / 4 * 4; hi = (hi + 3) / 4 * 4; }       // 16-byte Adam: a scalar segment's region grows to whole groups of four (see the kernel)
        if (lo < at) return a0_fail(A0_EINVAL, "a0_update_tail: segments overlap or share a 16-byte group of parameters");
        gap(at, lo);
        A.reg[nreg++] = a0_tail_region{lo, hi, (int)blocks, order[j], vec, 0};
        blocks += vec ? (s.count / 4 + 31) / 32 : (hi - lo + 31) / 32;
        at = hi;
    }
    gap(at, n_total);
    A.nreg = nreg;
    for (int k = nreg; k < 17; ++k) A.reg[k] = a0_tail_region{0, 0, 0x7fffffff, -1, 0, 0};
    if (blocks < 1 || blocks > 0x7fffffffLL) return a0_fail(A0_EINVAL, "a0_update_tail: grid");
    hipLaunchKernelGGL(a0_update_tail_kernel, dim3((unsigned)blocks), dim3(256), 0, (hipStream_t)stream, A);
    return a0_fail_hip((int)hipGetLastError(), "a0_update_tail");
}

// out[0] = 1.0f if this rank's NaN flag (state[0], set by the loss kernels) is up, else 0.0f — a float so that it can ride along in
// the SUM all-reduce of a gradient bucket (dist.GradAllReduce)
__global__ void a0_nan_flag_export_kernel(const int* __restrict__ state, float* __restrict__ out) { out[0] = state[0] != 0 ? 1.f : 0.f; }

extern "C" int a0_nan_flag_export(const int* state, float* out, void* stream) {
    if (!state || !out) return a0_fail(A0_EINVAL, "a0_nan_flag_export: bad argument");
    hipLaunchKernelGGL(a0_nan_flag_export_kernel, dim3(1), dim3(1), 0, (hipStream_t)stream, state, out);
    return a0_fail_hip((int)hipGetLastError(), "a0_nan_flag_export");
}

// RMSprop(lr, alpha, eps), no momentum, not centered (torch.optim.RMSprop defaults otherwise) — runs unconditionally,
// like the reference's fqf_optimizer.step() which sits before the NaN guard (agent.py:139-148).
__global__ void a0_rmsprop_kernel(float* __restrict__ p, const float* __restrict__ g, float* __restrict__ sq, long long n,
                                  float lr, float alpha, float w, float eps, const float* __restrict__ clip_coef) {
    const float c = clip_coef ? clip_coef[0] : 1.f;
    long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    const long long stride = (long long)gridDim.x * blockDim.x;
    for (; i < n; i += stride) {
        const float gi = g[i] * c;
        float s = sq[i] * alpha + (w * gi) * gi;
        sq[i] = s;
        p[i] = p[i] - lr * (gi / (sqrtf(s) + eps));
    }
}

// clip_coef[0] = min(1, max_norm / (||g|| + 1e-6))   (torch.nn.utils.clip_grad_norm_), single workgroup
__global__ __launch_bounds__(256) void a0_clip_coef_kernel(const float* __restrict__ g, long long n, float max_norm, float* __restrict__ coef) {
    __shared__ float red[256];
    float s = 0.f;
    for (long long i = threadIdx.x; i < n; i += 256) s += g[i] * g[i];
    a0_block_sum256(red, s);
    if (threadIdx.x == 0) {
        float c = max_norm / (sqrtf(red[0]) + 1e-6f);
        coef[0] = c < 1.f ? c : 1.f;
    }
}

extern "C" int a0_rmsprop_step(float* params, const float* grads, float* square_avg, long long n, double lr, double alpha, double eps,
                               double max_grad_norm, float* clip_scratch, void* stream) {
    if (!params || !grads || !square_avg || n < 1) return a0_fail(A0_EINVAL, "a0_rmsprop_step: bad argument");
    hipStream_t st = (hipStream_t)stream;
    const float* coef = nullptr;
    if (max_grad_norm > 0) {
        if (!clip_scratch) return a0_fail(A0_EINVAL, "a0_rmsprop_step: clipping needs a 1-float scratch");
        hipLaunchKernelGGL(a0_clip_coef_kernel, dim3(1), dim3(256), 0, st, grads, n, (float)max_grad_norm, clip_scratch);
        coef = clip_scratch;
    }
    hipLaunchKernelGGL(a0_rmsprop_kernel, dim3(a0_grid_256(n)), dim3(256), 0, st, params, grads, square_avg, n, (float)lr, (float)alpha,
                       (float)(1.0 - alpha), (float)eps, coef);
    return a0_fail_hip((int)hipGetLastError(), "a0_rmsprop_step");
}

// target <- online when state[4] says so (agent.py:160-161: deepcopy of the whole module, buffers included)
__global__ void a0_target_sync_kernel(float* __restrict__ dst, const float* __restrict__ src, long long n, const int* __restrict__ state, int force) {
    if (!force && !state[4]) return;
    long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    const long long stride = (long long)gridDim.x * blockDim.x;
    const long long n4 = n >> 2;
    const a0_f4* s4 = (const a0_f4*)src;
    a0_f4* d4 = (a0_f4*)dst;
    for (long long j = i; j < n4; j += stride) d4[j] = s4[j];
    for (long long j = (n4 << 2) + i; j < n; j += stride) dst[j] = src[j];
}

extern "C" int a0_target_sync(float* target, const float* online, long long n, const int* state, int force, void* stream) {
    if (!target || !online || n < 1 || (!force && !state)) return a0_fail(A0_EINVAL, "a0_target_sync: bad argument");
    if (!a0_aligned(16, target, online)) return a0_fail(A0_EINVAL, "a0_target_sync: buffers must be 16-byte aligned");
    hipLaunchKernelGGL(a0_target_sync_kernel, dim3(a0_grid_256(n >> 2)), dim3(256), 0, (hipStream_t)stream, target, online, n, state, force);
    return a0_fail_hip((int)hipGetLastError(), "a0_target_sync");
}

// ------------------------------------------------------------------------------------------------ soft target updates
// learner.target_tau: target <- target + tau * (online - target) over [0, n_total) — the whole module, as the hard copy takes it — at the updates where the hard copy
// would have happened.  The Adam forms in front are called with a target period of 0 ("never sync"), so this launch decides for itself from the step count they have
// committed by now: state[1] holds the NEW count behind all three tail forms.  When it does not blend, every workgroup returns at once.
// The element: a0_blend1 (a0_defs.h).  The firing rule is on purpose not net_reset.hip's a0_period_fires: no skip test, and at count 0 it blends only under `force`.

// W: the target's fused-kernel weight copies follow.  The lane that holds a blended convolution weight files it through the update tail's helpers, on the target
// side only — a0_wt_layout stays the only description of the copy layout.
template <bool W>
__global__ __launch_bounds__(256) void a0_target_blend_kernel(float* __restrict__ target, const float* __restrict__ online, long long n_total, float tau,
                                                              const int* __restrict__ state, int freq, int force, int vec4, a0_wt_sink B) {
    if (!force && !(freq > 0 && state[1] % freq == 0)) return;
    const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    const long long stride = (long long)gridDim.x * blockDim.x;
    long long done = 0;
    if (vec4) {                     // both buffers 16-byte aligned: 16 bytes per lane, the same arithmetic per element, and a scalar tail of n_total % 4 floats
        const long long n4 = n_total >> 2;
        for (long long j = i; j < n4; j += stride) {
            a0_f4 tv = ((a0_f4*)target)[j];
            const a0_f4 pv = ((const a0_f4*)online)[j];
            tv.x = a0_blend1(tv.x, pv.x, tau); tv.y = a0_blend1(tv.y, pv.y, tau); tv.z = a0_blend1(tv.z, pv.z, tau); tv.w = a0_blend1(tv.w, pv.w, tau);
            ((a0_f4*)target)[j] = tv;
            if constexpr (W) a0_tail_wt_f4(B, false, true, 4 * j, tv);
        }
        done = n4 << 2;
    }
    for (long long j = done + i; j < n_total; j += stride) {
        const float t = a0_blend1(target[j], online[j], tau);
        target[j] = t;
        if constexpr (W) a0_tail_wt1(B, false, true, j, t);
    }
}

extern "C" int a0_target_blend(float* target, const float* online, long long n_total, double tau, const int* state, int target_update_freq, int force,
                               const a0_encoder_weights* w_target, int C, float* wt_target, void* stream) {
    if (!target || !online || n_total < 1 || (!force && !state) || !a0_aligned(4, target, online))
        return a0_fail(A0_EINVAL, "a0_target_blend: bad argument");
    const float tau32 = (float)tau;       // rounded to fp32 once
    if (!(tau > 0.0) || !(tau < 1.0) || !(tau32 > 0.f) || !(tau32 < 1.f)) return a0_fail(A0_EINVAL, "a0_target_blend: tau must lie in (0, 1); tau >= 1 is the hard copy (a0_target_sync)");
    a0_wt_sink B{0, 0, 0, 0, 0, nullptr, nullptr};
    if (wt_target)
        if (int e = a0_wt_sink_make(&B, "a0_target_blend", "target", target, n_total, w_target, C, nullptr, wt_target)) return e;
    const int vec4 = a0_aligned(16, target, online) ? 1 : 0;
    hipLaunchKernelGGL(wt_target ? a0_target_blend_kernel<true> : a0_target_blend_kernel<false>, dim3(a0_grid_256(vec4 ? (n_total + 3) / 4 : n_total)), dim3(256), 0, (hipStream_t)stream,
                       target, online, n_total, tau32, state, target_update_freq, force, vec4, B);
    return a0_fail_hip((int)hipGetLastError(), "a0_target_blend");
}
