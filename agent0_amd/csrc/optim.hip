// Optimizer, NaN guard and target-network sync over the flat parameter buffer (gfx950).
// Restates reference agent0/deepq/agent.py:102-106 (Adam lr 5e-4, eps 1e-2/B), :333-338 (RMSprop for the FQF
// fraction net), :152-158 (skip the step when any per-sample loss is NaN) and :160-161 (target <- online every
// target_update_freq successful updates) without the two host syncs per update the reference pays (quirk Q14):
// the NaN flag, the step counter and the "sync now" decision all live in a small device-side state block.
#include "a0_internal.h"
#include "rng_elem.h"
#include "update_tail.h"

#include <algorithm>

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

// at most 2048 workgroups of 256 lanes, grid-stride behind that
static unsigned a0_grid_256(long long items) { const long long b = (items + 255) / 256; return (unsigned)(b > 2048 ? 2048 : b < 1 ? 1 : b); }
// the 16-byte path of the Adam forms: n, n_total multiples of four and every buffer 16-byte aligned
static int a0_adam_vec4(const float* params, const float* grads, const float* exp_avg, const float* exp_avg_sq, const float* target, long long n, long long n_total) {
    return ((n | n_total) % 4 == 0) && ((((uintptr_t)params) | ((uintptr_t)grads) | ((uintptr_t)exp_avg) | ((uintptr_t)exp_avg_sq) | ((uintptr_t)target)) % 16 == 0);
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
__global__ __launch_bounds__(256) void a0_grad_sumsq_kernel(const float* __restrict__ g, long long n, long long chunk, int vec4, double* __restrict__ partials) {
    __shared__ double red[256];
    const long long lo = (long long)blockIdx.x * chunk;
    const long long hi = lo + chunk < n ? lo + chunk : n;
    double s = 0.0;
    if (lo < hi) {
        long long done = 0;
        if (vec4) {
            const long long n4 = (hi - lo) >> 2;
            const a0_f4* g4 = (const a0_f4*)(g + lo);
            for (long long j = threadIdx.x; j < n4; j += 256) {
                const a0_f4 x = g4[j];
                s += (double)x.x * (double)x.x; s += (double)x.y * (double)x.y; s += (double)x.z * (double)x.z; s += (double)x.w * (double)x.w;
            }
            done = n4 << 2;
        }
        for (long long i = lo + done + threadIdx.x; i < hi; i += 256) s += (double)g[i] * (double)g[i];
    }
    red[threadIdx.x] = s;
    __syncthreads();
    for (int o = 128; o > 0; o >>= 1) { if ((int)threadIdx.x < o) red[threadIdx.x] += red[threadIdx.x + o]; __syncthreads(); }
    if (threadIdx.x == 0) partials[blockIdx.x] = red[0];
}

extern "C" int a0_grad_norm_partials(const float* grads, long long n, double* partials, void* stream) {
    if (!grads || !partials || n < 1 || (((uintptr_t)grads) & 3) || (((uintptr_t)partials) & 7)) return a0_fail(A0_EINVAL, "a0_grad_norm_partials: bad argument");
    const long long chunk = ((n + A0_GRAD_NORM_PARTIALS - 1) / A0_GRAD_NORM_PARTIALS + 3) / 4 * 4;
    hipLaunchKernelGGL(a0_grad_sumsq_kernel, dim3(A0_GRAD_NORM_PARTIALS), dim3(256), 0, (hipStream_t)stream, grads, n, chunk, (((uintptr_t)grads) & 15) == 0 ? 1 : 0, partials);
    return a0_fail_hip((int)hipGetLastError(), "a0_grad_norm_partials");
}

// the product alone, rounded to fp32: never contracted into the subtraction or the multiply-add that consumes it, so that stepping on g * coef gives the bits of
// a0_adam_step_sync on a gradient buffer multiplied by coef beforehand
A0_D float a0_mul_rounded(float a, float b) {
    float r;
    {
#pragma clang fp contract(off)
        r = a * b;
    }
    asm volatile("" : "+v"(r));      // the Adam arithmetic behind it sees a plain register value, as it sees a loaded gradient
    return r;
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
__global__ __launch_bounds__(256) void a0_weight_decay_kernel(float* __restrict__ p, long long n, long long chunk, int vec4, float c, const int* __restrict__ state,
                                                              const float* __restrict__ extra_flag, double* __restrict__ partials) {
    __shared__ double red[256];
    const bool skip = (state[0] != 0) || (extra_flag && extra_flag[0] != 0.f);
    const long long lo = (long long)blockIdx.x * chunk;
    const long long hi = lo + chunk < n ? lo + chunk : n;
    double s = 0.0;
    if (lo < hi) {
        long long done = 0;
        if (vec4) {
            const long long n4 = (hi - lo) >> 2;
            a0_f4* p4 = (a0_f4*)(p + lo);
            for (long long j = threadIdx.x; j < n4; j += 256) {
                a0_f4 x = p4[j];
                s += (double)x.x * (double)x.x; s += (double)x.y * (double)x.y; s += (double)x.z * (double)x.z; s += (double)x.w * (double)x.w;
                if (!skip) { x.x = a0_decay1(x.x, c); x.y = a0_decay1(x.y, c); x.z = a0_decay1(x.z, c); x.w = a0_decay1(x.w, c); p4[j] = x; }
            }
            done = n4 << 2;
        }
        for (long long i = lo + done + threadIdx.x; i < hi; i += 256) {
            const float x = p[i];
            s += (double)x * (double)x;
            if (!skip) p[i] = a0_decay1(x, c);
        }
    }
    red[threadIdx.x] = s;
    __syncthreads();
    for (int o = 128; o > 0; o >>= 1) { if ((int)threadIdx.x < o) red[threadIdx.x] += red[threadIdx.x + o]; __syncthreads(); }
    if (threadIdx.x == 0) partials[blockIdx.x] = red[0];
}

// c: lr * lambda as the caller formed it in double; rounded to fp32 once here.  2^-24 <= fl32(c) < 1: a smaller c moves no fp32 value, c >= 1 is no decay
extern "C" int a0_weight_decay(float* params, long long n, double c, const int* state, const float* extra_nan_flag, double* partials, void* stream) {
    if (!params || !state || !partials || n < 1 || (((uintptr_t)params) & 3) || (((uintptr_t)partials) & 7)) return a0_fail(A0_EINVAL, "a0_weight_decay: bad argument");
    const float c32 = (float)c;
    if (!(c32 >= 0x1p-24f) || !(c32 < 1.f)) return a0_fail(A0_EINVAL, "a0_weight_decay: c = lr * lambda must lie in [2^-24, 1) as an fp32 number");
    const long long chunk = ((n + A0_GRAD_NORM_PARTIALS - 1) / A0_GRAD_NORM_PARTIALS + 3) / 4 * 4;
    hipLaunchKernelGGL(a0_weight_decay_kernel, dim3(A0_GRAD_NORM_PARTIALS), dim3(256), 0, (hipStream_t)stream, params, n, chunk, (((uintptr_t)params) & 15) == 0 ? 1 : 0, c32, state,
                       extra_nan_flag, partials);
    return a0_fail_hip((int)hipGetLastError(), "a0_weight_decay");
}

// The batch mean of this update's per-sample losses (the Trainer's `loss` statistic, trainer.py:99,111-113) into the ring slot of the free-running call counter
// state[6], by ONE workgroup of 256 lanes — the same reduction, statement for statement, as a0_mean_rows_kernel, whose launch per update (4.8 us of pure latency)
// it replaces.  Skipped steps are recorded too (their mean is whatever the loss kernel wrote, NaN included).
A0_D void a0_loss_mean_to_ring(const float* loss, int loss_n, float* loss_ring, int ring_cap, int* state_w) {
    __shared__ float red[256];
    float s = 0.f;
    for (int e = threadIdx.x; e < loss_n; e += 256) s += loss[e];
    red[threadIdx.x] = s;
    __syncthreads();
    for (int o = 128; o > 0; o >>= 1) { if ((int)threadIdx.x < o) red[threadIdx.x] += red[threadIdx.x + o]; __syncthreads(); }
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
        cred[threadIdx.x] = K.partials[threadIdx.x];
        __syncthreads();
        for (int o = 128; o > 0; o >>= 1) { if ((int)threadIdx.x < o) cred[threadIdx.x] += cred[threadIdx.x + o]; __syncthreads(); }
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
    return partials && (((uintptr_t)partials) & 7) == 0 && max_norm > 0.f && norm_ring && norm_ring_cap >= 1;
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
// no workgroup waits for another.  The lane that holds a new convolution weight also files it in the fused kernels' copies (the inverse of a0_conv_wt_kernel's gather).

// Where a new convolution weight goes in the fused kernels' copies `wt` (online) / `wt_t` (target): the one description the tail, the blend and the reset share.
struct a0_wt_sink {
    long long o1, o2, o3;                       // first weight of conv1 / conv2 / conv3 in the flat buffer
    int K1, wt4;                                // wt4: o1, o2, o3 multiples of four (four consecutive k of one row per 16-byte lane)
    float *wt, *wt_t;
};
// w: the convolution weights inside base[0, n_total) (`what`: the buffer's name in who's error text); wt may be NULL for a caller that files the target side only
static int a0_wt_sink_make(a0_wt_sink* S, const char* who, const char* what, const float* base, long long n_total, const a0_encoder_weights* w, int C, float* wt, float* wt_target) {
    const std::string name(who);
    if (!w || !w->w1 || !w->w2 || !w->w3 || C < 1 || !wt_target) return a0_fail(A0_EINVAL, (name + ": weight copies need the encoder weights, C >= 1 and the copies' buffers").c_str());
    if ((((uintptr_t)wt) | ((uintptr_t)wt_target)) & 15) return a0_fail(A0_EINVAL, (name + ": the weight copies must be 16-byte aligned").c_str());
    *S = a0_wt_sink{w->w1 - base, w->w2 - base, w->w3 - base, C * 64, 0, wt, wt_target};
    if (S->o1 < 0 || S->o1 + 32LL * S->K1 > n_total || S->o2 < 0 || S->o2 + 64 * 512 > n_total || S->o3 < 0 || S->o3 + 64 * 576 > n_total)
        return a0_fail(A0_EINVAL, (name + ": the convolution weights must lie inside " + what + "[0, n_total)").c_str());
    S->wt4 = ((S->o1 | S->o2 | S->o3) % 4 == 0) ? 1 : 0;
    return A0_OK;
}

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

A0_D void a0_tail_put16(const a0_wt_sink& A, bool to_online, bool to_target, long long u16, uint32_t bits) {
    if (to_online) ((uint16_t*)A.wt)[u16] = (uint16_t)bits;
    if (to_target) ((uint16_t*)A.wt_t)[u16] = (uint16_t)bits;
}
A0_D void a0_tail_put32(const a0_wt_sink& A, bool to_online, bool to_target, int dw, uint32_t bits) {
    if (to_online) ((uint32_t*)A.wt)[dw] = bits;
    if (to_target) ((uint32_t*)A.wt_t)[dw] = bits;
}
// dword of term s of weight (n, k) in an a0_wring1 / a0_wring9 segment of N columns: uint4 ((t*N + n)*4 + q)*3 + s holds k = 32t + 8q .. +7; a dword is two consecutive k
A0_D int a0_tail_term_dword(int N, int n, int k, int s) { return ((((k >> 5) * N + n) * 4 + ((k >> 3) & 3)) * 3 + s) * 4 + ((k >> 1) & 3); }
// the data-gradient copies of one weight: conv3's flipped taps, conv2's stride phases (see a0_conv_wt_kernel)
A0_D void a0_tail_wt_dgrad(const a0_wt_sink& A, bool to_online, bool to_target, const a0_wt_layout& T, bool c3, int co, int k, float w) {
    int base, N, n, kk;
    if (c3) {              // k = (kh*3 + kw)*64 + ci  ->  n = ci, k' = ((2-kh)*3 + (2-kw))*64 + co
        const int cell = k >> 6;
        n = k & 63; kk = (8 - cell) * 64 + co; base = T.dgrad3x(); N = 64;
    } else {               // k = (kh*4 + kw)*32 + ci  ->  phase (kh & 1, kw & 1), n = ci, k' = ((1 - kh/2)*2 + (1 - kw/2))*64 + co
        const int tap = k >> 5, kh = tap >> 2, kw = tap & 3;
        n = k & 31; kk = ((1 - (kh >> 1)) * 2 + (1 - (kw >> 1))) * 64 + co; base = T.dgrad2x() + ((kh & 1) * 2 + (kw & 1)) * T.n_dgrad2x_phase; N = 32;
    }
#pragma unroll
    for (int s = 0; s < 3; ++s) a0_tail_put16(A, to_online, to_target, 2LL * (base + a0_tail_term_dword(N, n, kk, s)) + (kk & 1), a0_bf16_term(w, s));
}
// every copy of the weight at flat index idx (new value w): nothing to do outside the three convolution weight blocks
A0_D void a0_tail_wt1(const a0_wt_sink& A, bool to_online, bool to_target, long long idx, float w) {
    const a0_wt_layout T{A.K1 / 64};
    if (idx >= A.o1 && idx < A.o1 + 32LL * A.K1) {
        const int e = (int)(idx - A.o1), n = e / A.K1, k = e - n * A.K1;
        const float x = w / 255.0f;             // conv1 multiplies raw bytes: the reference's /255 is folded in here
#pragma unroll
        for (int s = 0; s < 3; ++s) a0_tail_put16(A, to_online, to_target, 2LL * (T.conv1x() + a0_tail_term_dword(32, n, k, s)) + (k & 1), a0_bf16_term(x, s));
    } else if ((idx >= A.o2 && idx < A.o2 + 64 * 512) || (idx >= A.o3 && idx < A.o3 + 64 * 576)) {
        const bool c3 = idx >= A.o3 && idx < A.o3 + 64 * 576;
        const int K = c3 ? 576 : 512, e = (int)(idx - (c3 ? A.o3 : A.o2)), n = e / K, k = e - n * K;
        // fp32, a0_wring layout: float ((c*64 + n)*4 + q)*4 + j holds W[n][k = 16c + 4j + q]
        a0_tail_put32(A, to_online, to_target, (c3 ? T.conv3() : T.conv2()) + (((k >> 4) * 64 + n) * 4 + (k & 3)) * 4 + ((k >> 2) & 3), __float_as_uint(w));
#pragma unroll
        for (int s = 0; s < 3; ++s) a0_tail_put16(A, to_online, to_target, 2LL * ((c3 ? T.conv3x() : T.conv2x()) + a0_tail_term_dword(64, n, k, s)) + (k & 1), a0_bf16_term(w, s));
        a0_tail_wt_dgrad(A, to_online, to_target, T, c3, n, k, w);
    }
}
// four consecutive weights idx .. idx + 3 of one row (idx a multiple of four floats behind its block's start): the terms of four k are 8 adjacent bytes
A0_D void a0_tail_wt4(const a0_wt_sink& A, bool to_online, bool to_target, long long idx, const a0_f4& pv) {
    const a0_wt_layout T{A.K1 / 64};
    const float w[4] = {pv.x, pv.y, pv.z, pv.w};
    int base, N, n, k;
    bool c1 = false, c3 = false;
    if (idx >= A.o1 && idx < A.o1 + 32LL * A.K1) { const int e = (int)(idx - A.o1); n = e / A.K1; k = e - n * A.K1; base = T.conv1x(); N = 32; c1 = true; }
    else if (idx >= A.o2 && idx < A.o2 + 64 * 512) { const int e = (int)(idx - A.o2); n = e >> 9; k = e & 511; base = T.conv2x(); N = 64; }
    else if (idx >= A.o3 && idx < A.o3 + 64 * 576) { const int e = (int)(idx - A.o3); n = e / 576; k = e - n * 576; base = T.conv3x(); N = 64; c3 = true; }
    else return;
    float x[4];
#pragma unroll
    for (int e = 0; e < 4; ++e) x[e] = c1 ? w[e] / 255.0f : w[e];
#pragma unroll
    for (int s = 0; s < 3; ++s) {
        const uint2 t{a0_bf16_term(x[0], s) | (a0_bf16_term(x[1], s) << 16), a0_bf16_term(x[2], s) | (a0_bf16_term(x[3], s) << 16)};
        const int dw = base + a0_tail_term_dword(N, n, k, s);          // k a multiple of four: an even dword
        if (to_online) *(uint2*)((uint32_t*)A.wt + dw) = t;
        if (to_target) *(uint2*)((uint32_t*)A.wt_t + dw) = t;
    }
    if (c1) return;
    const int ring = (c3 ? T.conv3() : T.conv2()) + (((k >> 4) * 64 + n) * 4) * 4 + ((k >> 2) & 3);
#pragma unroll
    for (int e = 0; e < 4; ++e) {
        a0_tail_put32(A, to_online, to_target, ring + 4 * e, __float_as_uint(w[e]));
        a0_tail_wt_dgrad(A, to_online, to_target, T, c3, n, k + e, w[e]);
    }
}

// four consecutive weights held by one lane
A0_D void a0_tail_wt_f4(const a0_wt_sink& A, bool to_online, bool to_target, long long idx, const a0_f4& pv) {
    if (A.wt4) a0_tail_wt4(A, to_online, to_target, idx, pv);
    else { a0_tail_wt1(A, to_online, to_target, idx, pv.x); a0_tail_wt1(A, to_online, to_target, idx + 1, pv.y); a0_tail_wt1(A, to_online, to_target, idx + 2, pv.z); a0_tail_wt1(A, to_online, to_target, idx + 3, pv.w); }
}

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
        const int vec = ((s.count | s.slab_stride) % 4 == 0) && ((((uintptr_t)s.slabs) | ((uintptr_t)s.out)) % 16 == 0);
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
    red[threadIdx.x] = s;
    __syncthreads();
    for (int o = 128; o > 0; o >>= 1) {
        if ((int)threadIdx.x < o) red[threadIdx.x] += red[threadIdx.x + o];
        __syncthreads();
    }
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
    long long blocks = (n + 255) / 256;
    if (blocks > 2048) blocks = 2048;
    hipLaunchKernelGGL(a0_rmsprop_kernel, dim3((unsigned)blocks), dim3(256), 0, st, params, grads, square_avg, n, (float)lr, (float)alpha,
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
    if ((((uintptr_t)target) | ((uintptr_t)online)) & 15) return a0_fail(A0_EINVAL, "a0_target_sync: buffers must be 16-byte aligned");
    long long blocks = ((n >> 2) + 255) / 256;
    if (blocks > 2048) blocks = 2048;
    if (blocks < 1) blocks = 1;
    hipLaunchKernelGGL(a0_target_sync_kernel, dim3((unsigned)blocks), dim3(256), 0, (hipStream_t)stream, target, online, n, state, force);
    return a0_fail_hip((int)hipGetLastError(), "a0_target_sync");
}

// ------------------------------------------------------------------------------------------------ soft target updates
// learner.target_tau: target <- target + tau * (online - target) over [0, n_total) — the whole module, as the hard copy takes it — at the updates where the hard copy
// would have happened.  The Adam forms in front are called with a target period of 0 ("never sync"), so this launch decides for itself from the step count they have
// committed by now: state[1] holds the NEW count behind all three tail forms.  When it does not blend, every workgroup returns at once.
// One rounded subtraction and one fused multiply-add per element, kept out of the compiler's contraction choices (see a0_mul_rounded).
A0_D float a0_blend1(float t, float p, float tau) {
    float d;
    {
#pragma clang fp contract(off)
        d = p - t;
    }
    asm volatile("" : "+v"(d));
    return __builtin_fmaf(tau, d, t);
}

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
    if (!target || !online || n_total < 1 || (!force && !state) || ((((uintptr_t)target) | ((uintptr_t)online)) & 3))
        return a0_fail(A0_EINVAL, "a0_target_blend: bad argument");
    const float tau32 = (float)tau;       // rounded to fp32 once
    if (!(tau > 0.0) || !(tau < 1.0) || !(tau32 > 0.f) || !(tau32 < 1.f)) return a0_fail(A0_EINVAL, "a0_target_blend: tau must lie in (0, 1); tau >= 1 is the hard copy (a0_target_sync)");
    a0_wt_sink B{0, 0, 0, 0, 0, nullptr, nullptr};
    if (wt_target)
        if (int e = a0_wt_sink_make(&B, "a0_target_blend", "target", target, n_total, w_target, C, nullptr, wt_target)) return e;
    const int vec4 = ((((uintptr_t)target) | ((uintptr_t)online)) % 16 == 0) ? 1 : 0;
    hipLaunchKernelGGL(wt_target ? a0_target_blend_kernel<true> : a0_target_blend_kernel<false>, dim3(a0_grid_256(vec4 ? (n_total + 3) / 4 : n_total)), dim3(256), 0, (hipStream_t)stream,
                       target, online, n_total, tau32, state, target_update_freq, force, vec4, B);
    return a0_fail_hip((int)hipGetLastError(), "a0_target_blend");
}

// ------------------------------------------------------------------------------------------------ periodic network resets
// learner.net_reset_freq = N: after an update that was not NaN-skipped and left update_steps a positive multiple of N, the Q-network is re-initialised in ONE launch
// behind the update's Adam form (and behind a0_target_blend): the head blocks are replaced by fresh values, the encoder blocks keep the share alpha of theirs
// (shrink and perturb), Adam's moments are zeroed, its bias correction restarts (state[7] <- state[1]), the target becomes a copy of the online network and the
// lane that holds a convolution weight files it in both networks' weight copies.  On every other update all workgroups return after reading state[1] and state[3].
// Fresh values: element i at reset k = update_steps / N draws from Philox stream A0_STREAM_RESET of the seed at position k * n_total + i — a function of
// (seed, k, i) alone; a normal element is a0_rng_normal's value there, a uniform one bound * (2 u - 1) with u a0_rng_uniform's (rng_elem.h).
struct a0_reset_table { a0_net_reset_seg s[A0_NET_RESET_MAX_SEGS]; int n; };
// the rule of one flat index: kind < 0 outside every segment; keep is the share that survives (alpha32 or 0); end: one past the segment's last index
struct a0_reset_rule { long long end; int kind; float scale, keep; };

// every lane walks the table in the same order (uniform loads of the by-value table, no indexed access to it); outside every segment `end` is where the next one starts
A0_D a0_reset_rule a0_reset_find(const a0_reset_table& T, float alpha, long long i, long long n_total) {
    a0_reset_rule R{n_total, -1, 0.f, 1.f};
#pragma nounroll
    for (int s = 0; s < T.n; ++s) {
        const long long lo = T.s[s].offset, hi = lo + T.s[s].count;
        if (i >= lo && i < hi) { R.end = hi; R.kind = T.s[s].kind; R.scale = T.s[s].scale; R.keep = T.s[s].keep ? alpha : 0.f; }
        else if (lo > i && lo < R.end && R.kind < 0) R.end = lo;
    }
    return R;
}
// 2u - 1 is exact in fp32 (u is a multiple of 2^-24 below 1), then one rounded multiply
A0_D float a0_reset_uniform(float bound, float u) {
#pragma clang fp contract(off)
    return bound * (2.0f * u - 1.0f);
}
A0_D float a0_reset_fresh1(const a0_reset_rule& R, unsigned long long seed, unsigned long long pos, uint32_t stream = A0_STREAM_RESET) {
    if (R.kind == A0_NET_RESET_NORMAL) return a0_rng_normal_at(seed, stream, pos, R.scale);
    if (R.kind == A0_NET_RESET_UNIFORM) return a0_reset_uniform(R.scale, a0_rng_uniform_at(seed, stream, pos));
    return R.scale;
}
// four consecutive positions that share one Philox block (pos0 a multiple of four): one block, two Box-Muller pairs — the words a0_philox_word would pick
A0_D a0_f4 a0_reset_fresh4(const a0_reset_rule& R, unsigned long long seed, unsigned long long pos0) {
    a0_f4 f;
    if (R.kind == A0_NET_RESET_CONST) { f.x = f.y = f.z = f.w = R.scale; return f; }
    const unsigned long long blk = pos0 >> 2;
    const a0_u4 o = a0_philox4x32_10((uint32_t)blk, (uint32_t)(blk >> 32), A0_STREAM_RESET, 0u, (uint32_t)seed, (uint32_t)(seed >> 32));
    if (R.kind == A0_NET_RESET_NORMAL) {
        f.x = a0_rng_normal_words(o.x, o.y, false, R.scale); f.y = a0_rng_normal_words(o.x, o.y, true, R.scale);
        f.z = a0_rng_normal_words(o.z, o.w, false, R.scale); f.w = a0_rng_normal_words(o.z, o.w, true, R.scale);
    } else {
        f.x = a0_reset_uniform(R.scale, a0_rng_uniform_word(o.x)); f.y = a0_reset_uniform(R.scale, a0_rng_uniform_word(o.y));
        f.z = a0_reset_uniform(R.scale, a0_rng_uniform_word(o.z)); f.w = a0_reset_uniform(R.scale, a0_rng_uniform_word(o.w));
    }
    return f;
}
// keep == 0: the fresh value itself; otherwise fmaf(keep, fl32(p - phi), phi) — a0_blend1's form with the fresh value in the target's place
A0_D float a0_reset_mix(const a0_reset_rule& R, float p, float phi) { return R.keep == 0.f ? phi : a0_blend1(phi, p, R.keep); }

template <bool W>
__global__ __launch_bounds__(256) void a0_net_reset_kernel(float* __restrict__ p, float* __restrict__ target, float* __restrict__ m, float* __restrict__ v, long long n_adam,
                                                           long long n_total, a0_reset_table T, float alpha, unsigned long long seed_arg, int* __restrict__ state, int freq,
                                                           int force, long long k_host, int vec4, a0_wt_sink B) {
    long long k = k_host;
    if (!force) {
        const int steps = state[1];
        if (state[3] != 0 || !(freq > 0 && steps > 0 && steps % freq == 0)) return;
        k = steps / freq;
    }
    // a fresh optimizer: a0_step_decide counts t from here (nobody reads state[7] during this launch)
    if (state && blockIdx.x == 0 && threadIdx.x == 0) state[7] = state[1];
    // the seed (32 bits) travels in a vector register: Philox's key schedule of a uniform seed would be hoisted into twenty scalar registers for the whole loop
    uint32_t seed_v = (uint32_t)seed_arg;
    asm volatile("" : "+v"(seed_v));
    const unsigned long long seed = seed_v;
    const unsigned long long base = (unsigned long long)k * (unsigned long long)n_total;
    const long long stride = (long long)gridDim.x * blockDim.x;
    const long long groups = (n_total + 3) >> 2;
    // a lane owns four consecutive elements.  `wide`: the buffers are 16-byte aligned, the four share a Philox block and, with weight copies, a row of a convolution
    // matrix; where they also lie inside one segment (or between two) they move as 16 bytes.  Everything else — a segment boundary inside the four (the real / pad
    // boundary of a noisy bias), the tail of n_total % 4 floats, 4-byte-aligned buffers — goes element by element through the same arithmetic.
    const bool wide = vec4 && (base & 3) == 0 && (!W || B.wt4);
    for (long long j = (long long)blockIdx.x * blockDim.x + threadIdx.x; j < groups; j += stride) {
        const long long e0 = 4 * j;
        const a0_reset_rule R = a0_reset_find(T, alpha, e0, n_total);
        if (wide && e0 + 4 <= R.end) {
            a0_f4 pv = ((a0_f4*)p)[j];
            if (R.kind >= 0 && R.keep != 1.f) {
                const a0_f4 f = a0_reset_fresh4(R, seed, base + (unsigned long long)e0);
                pv.x = a0_reset_mix(R, pv.x, f.x); pv.y = a0_reset_mix(R, pv.y, f.y); pv.z = a0_reset_mix(R, pv.z, f.z); pv.w = a0_reset_mix(R, pv.w, f.w);
                ((a0_f4*)p)[j] = pv;
            }
            ((a0_f4*)target)[j] = pv;
            if (e0 + 4 <= n_adam) { ((a0_f4*)m)[j] = a0_zero4(); ((a0_f4*)v)[j] = a0_zero4(); }
            else {
#pragma unroll
                for (int e = 0; e < 4; ++e) if (e0 + e < n_adam) { m[e0 + e] = 0.f; v[e0 + e] = 0.f; }
            }
            continue;
        }
#pragma nounroll
        for (long long idx = e0; idx < e0 + 4 && idx < n_total; ++idx) {
            const a0_reset_rule Re = a0_reset_find(T, alpha, idx, n_total);
            float x = p[idx];
            if (Re.kind >= 0 && Re.keep != 1.f) { x = a0_reset_mix(Re, x, a0_reset_fresh1(Re, seed, base + (unsigned long long)idx)); p[idx] = x; }
            target[idx] = x;
            if (idx < n_adam) { m[idx] = 0.f; v[idx] = 0.f; }
        }
    }
    // the weight copies of BOTH networks (the target is the online network after a reset), in a pass of their own over the convolution blocks: every lane files the
    // parameters it has just written itself (the same lane-to-element map)
    if constexpr (W) {
        const long long c_lo = (B.o1 < B.o2 ? (B.o1 < B.o3 ? B.o1 : B.o3) : (B.o2 < B.o3 ? B.o2 : B.o3)) >> 2;
        long long c_hi = B.o1 + 32LL * B.K1;
        if (B.o2 + 64 * 512 > c_hi) c_hi = B.o2 + 64 * 512;
        if (B.o3 + 64 * 576 > c_hi) c_hi = B.o3 + 64 * 576;
        c_hi = (c_hi + 3) >> 2;
        for (long long j = (long long)blockIdx.x * blockDim.x + threadIdx.x; j < c_hi && j < groups; j += stride) {      // the first pass's groups, lane for lane
            if (j < c_lo) continue;
            const long long e0 = 4 * j;
            if (wide && e0 + 4 <= n_total) a0_tail_wt4(B, true, true, e0, ((const a0_f4*)p)[j]);
            else {
#pragma nounroll
                for (long long idx = e0; idx < e0 + 4 && idx < n_total; ++idx) a0_tail_wt1(B, true, true, idx, p[idx]);
            }
        }
    }
}

// the by-value table of a launch from the caller's rules, checked (`who`: the entry point's name in the error text)
static int a0_reset_table_make(a0_reset_table* T, const char* who, const a0_net_reset_seg* segs, int n_segs, long long n_adam) {
    const std::string name(who);
    if (n_segs < 0 || n_segs > A0_NET_RESET_MAX_SEGS || (n_segs > 0 && !segs)) return a0_fail(A0_EINVAL, (name + ": between 0 and A0_NET_RESET_MAX_SEGS segments").c_str());
    T->n = n_segs;
    long long at = 0;
    for (int s = 0; s < A0_NET_RESET_MAX_SEGS; ++s) {
        if (s >= n_segs) { T->s[s] = a0_net_reset_seg{0, 0, A0_NET_RESET_CONST, 0.f, 0}; continue; }
        const a0_net_reset_seg& g = segs[s];
        if (g.offset < at || g.count < 1 || g.offset + g.count > n_adam) return a0_fail(A0_EINVAL, (name + ": the segments must be ascending, disjoint and inside [0, n_adam)").c_str());
        if (g.kind != A0_NET_RESET_CONST && g.kind != A0_NET_RESET_NORMAL && g.kind != A0_NET_RESET_UNIFORM) return a0_fail(A0_EINVAL, (name + ": unknown segment kind").c_str());
        if (!(g.scale == g.scale) || g.scale - g.scale != 0.f || (g.keep != 0 && g.keep != 1)) return a0_fail(A0_EINVAL, (name + ": a segment's scale must be finite and its keep flag 0 or 1").c_str());
        at = g.offset + g.count;
        T->s[s] = g;
    }
    return A0_OK;
}

extern "C" int a0_net_reset(float* params, float* target, float* exp_avg, float* exp_avg_sq, long long n_adam, long long n_total, const a0_net_reset_seg* segs, int n_segs,
                            double alpha, unsigned long long seed, int* state, int freq, int force, long long k_host, const a0_encoder_weights* w, int C, float* wt,
                            float* wt_target, void* stream) {
    if (!params || !target || !exp_avg || !exp_avg_sq || n_adam < 1 || n_total < n_adam || (!force && !state) || freq < 0 || (force && k_host < 0) ||
        ((((uintptr_t)params) | ((uintptr_t)target) | ((uintptr_t)exp_avg) | ((uintptr_t)exp_avg_sq)) & 3))
        return a0_fail(A0_EINVAL, "a0_net_reset: bad argument");
    if (!(alpha >= 0.0) || !(alpha <= 1.0)) return a0_fail(A0_EINVAL, "a0_net_reset: alpha must lie in [0, 1]");
    a0_reset_table T;
    if (int e = a0_reset_table_make(&T, "a0_net_reset", segs, n_segs, n_adam)) return e;
    a0_wt_sink B{0, 0, 0, 0, 0, nullptr, nullptr};
    if (wt || wt_target) {
        if (!wt) return a0_fail(A0_EINVAL, "a0_net_reset: weight copies need wt and wt_target, both or neither");
        if (int e = a0_wt_sink_make(&B, "a0_net_reset", "params", params, n_total, w, C, wt, wt_target)) return e;
    }
    const int vec4 = ((((uintptr_t)params) | ((uintptr_t)target) | ((uintptr_t)exp_avg) | ((uintptr_t)exp_avg_sq)) % 16 == 0) ? 1 : 0;
    const float alpha32 = (float)alpha;       // rounded to fp32 once
    const unsigned long long seed32 = seed & 0xFFFFFFFFull;
    hipLaunchKernelGGL(wt ? a0_net_reset_kernel<true> : a0_net_reset_kernel<false>, dim3(a0_grid_256((n_total + 3) / 4)), dim3(256), 0, (hipStream_t)stream,
                       params, target, exp_avg, exp_avg_sq, n_adam, n_total, T, alpha32, seed32, state, freq, force, k_host, vec4, B);
    return a0_fail_hip((int)hipGetLastError(), "a0_net_reset");
}

// ------------------------------------------------------------------------------------------------ dormant neurons and ReDo
// learner.redo_freq = N (Sokar et al. 2023): after an update that was not NaN-skipped and left update_steps a positive multiple of N, three launches behind the
// update's Adam form (and a0_target_blend), in front of a0_net_reset: (1) per-workgroup sums of |activation| per neuron over the differentiated pass's four buffers,
// (2) one workgroup finishes them into the scores s_i = m_i / mean_j(m_j), the mask s_i <= tau and the counts, (3) the dormant neurons are recycled.  On every other
// update each launch returns after reading state[1] and state[3].  Everything is summed in double in a fixed order (the rows of a workgroup by the geometry alone,
// the lanes of a channel and the workgroups in index order; no atomics), so a run is reproducible.
A0_D bool a0_redo_fires(const int* __restrict__ state, int freq, int force) {
    if (force) return true;
    const int steps = state[1];
    return state[3] == 0 && freq > 0 && steps > 0 && steps % freq == 0;
}

// The workgroups that take part in a layer of `rows` rows when one workgroup step covers `rps` rows: about eight steps each, at most all of them — a function of
// the row count alone.  A short layer (fc1: B rows of 512) leaves few partials for the finish to read.
A0_D int a0_redo_groups(long long rows, int rps) {
    const long long g = ((rows + rps - 1) / rps + 7) / 8;
    return (int)(g < 1 ? 1 : g > A0_REDO_PARTIALS ? A0_REDO_PARTIALS : g);
}

// One layer of N channels, channel-fastest: a lane owns four channels (one 16-byte load per row) of every (256 / (N / 4))-th row of its workgroup's rows, four
// loads in flight; one exchange through LDS per layer, after which lane ch adds its channel's lanes in index order.  out: this workgroup's N partial sums.
template <int N>
A0_D void a0_redo_layer_sums(const float* __restrict__ X, long long rows, double* __restrict__ out, double (*sh)[4]) {
    constexpr int N4 = N / 4, RPS = 256 / N4;
    const int tid = threadIdx.x, r = tid / N4, c = tid % N4, G = a0_redo_groups(rows, RPS);
    if ((int)blockIdx.x >= G) return;          // the whole workgroup: nobody waits at the barriers below
    const long long steps = (rows + RPS - 1) / RPS, per = (steps + G - 1) / G;
    const long long s0 = (long long)blockIdx.x * per, s1 = s0 + per < steps ? s0 + per : steps;
    const a0_f4* __restrict__ X4 = (const a0_f4*)X;
    double a[4] = {0.0, 0.0, 0.0, 0.0};
    long long s = s0;
    for (; s + 4 <= s1; s += 4) {
        a0_f4 x[4];
#pragma unroll
        for (int u = 0; u < 4; ++u) { const long long row = (s + u) * RPS + r; x[u] = row < rows ? X4[row * N4 + c] : a0_zero4(); }
#pragma unroll
        for (int u = 0; u < 4; ++u) { a[0] += (double)fabsf(x[u].x); a[1] += (double)fabsf(x[u].y); a[2] += (double)fabsf(x[u].z); a[3] += (double)fabsf(x[u].w); }
    }
    for (; s < s1; ++s) {
        const long long row = s * RPS + r;
        const a0_f4 x = row < rows ? X4[row * N4 + c] : a0_zero4();
        a[0] += (double)fabsf(x.x); a[1] += (double)fabsf(x.y); a[2] += (double)fabsf(x.z); a[3] += (double)fabsf(x.w);
    }
#pragma unroll
    for (int e = 0; e < 4; ++e) sh[tid][e] = a[e];
    __syncthreads();
    for (int ch = tid; ch < N; ch += 256) {
        double t = 0.0;
#pragma unroll
        for (int rr = 0; rr < RPS; ++rr) t += sh[rr * N4 + (ch >> 2)][ch & 3];
        out[ch] = t;
    }
    __syncthreads();
}

__global__ __launch_bounds__(256) void a0_redo_sums_kernel(const float* __restrict__ act1, long long rows1, const float* __restrict__ act2, long long rows2,
                                                           const float* __restrict__ act3, long long rows3, const float* __restrict__ fc1, long long rows4,
                                                           const int* __restrict__ state, int freq, int force, double* __restrict__ partials) {
    if (!a0_redo_fires(state, freq, force)) return;
    __shared__ double sh[256][4];
    double* out = partials + (long long)blockIdx.x * A0_REDO_NEURONS;
    a0_redo_layer_sums<32>(act1, rows1, out, sh);
    a0_redo_layer_sums<64>(act2, rows2, out + 32, sh);
    a0_redo_layer_sums<64>(act3, rows3, out + 96, sh);
    a0_redo_layer_sums<512>(fc1, rows4, out + 160, sh);
}

// layer of neuron i: 0 conv1 [0, 32), 1 conv2 [32, 96), 2 conv3 [96, 160), 3 fc1 [160, 672)
A0_D int a0_redo_layer_of(int i) { return i < 32 ? 0 : i < 96 ? 1 : i < 160 ? 2 : 3; }

// One workgroup of 1024 lanes.  The partials of a neuron — those of the workgroups that took part in its layer — are added in index order in two steps, so that
// up to 512 dependent additions do not wait for as many loads one after the other: lane (slice s, neuron i) adds the s-th eighth of them (independent loads), then
// lane i adds its eight slice sums in index order.
__global__ __launch_bounds__(1024) void a0_redo_finish_kernel(const double* __restrict__ partials, long long rows1, long long rows2, long long rows3, long long rows4,
                                                              double tau, const int* __restrict__ state, int freq, int force, float* __restrict__ scores, int* __restrict__ mask,
                                                              int* __restrict__ counts) {
    if (!a0_redo_fires(state, freq, force)) return;
    constexpr int SLICES = 8;
    __shared__ double part[SLICES][A0_REDO_NEURONS];
    __shared__ double m[A0_REDO_NEURONS];
    __shared__ double mean[4];
    __shared__ int dorm[A0_REDO_NEURONS];
    __shared__ int cnt[4];
    const int i = threadIdx.x, lay = a0_redo_layer_of(i);
    const int lo = i == 0 ? 0 : i == 1 ? 32 : i == 2 ? 96 : 160, width = i == 0 ? 32 : i == 3 ? 512 : 64;      // of layer i, for the lanes i < 4
    for (int item = threadIdx.x; item < SLICES * A0_REDO_NEURONS; item += 1024) {
        const int sl = item / A0_REDO_NEURONS, n = item - sl * A0_REDO_NEURONS, ln = a0_redo_layer_of(n);
        const int G = ln == 0 ? a0_redo_groups(rows1, 32) : ln == 1 ? a0_redo_groups(rows2, 16) : ln == 2 ? a0_redo_groups(rows3, 16) : a0_redo_groups(rows4, 2);
        const int per = (G + SLICES - 1) / SLICES, g0 = sl * per, g1 = g0 + per < G ? g0 + per : G;
        double t = 0.0;
#pragma unroll 8
        for (int g = g0; g < g1; ++g) t += partials[(long long)g * A0_REDO_NEURONS + n];
        part[sl][n] = t;
    }
    __syncthreads();
    if (i < A0_REDO_NEURONS) {
        const long long rows = lay == 0 ? rows1 : lay == 1 ? rows2 : lay == 2 ? rows3 : rows4;
        double t = 0.0;
#pragma unroll
        for (int sl = 0; sl < SLICES; ++sl) t += part[sl][i];
        m[i] = t / (double)rows;
    }
    __syncthreads();
    if (i < 4) {
        double t = 0.0;
        for (int j = 0; j < width; ++j) t += m[lo + j];
        mean[i] = t / (double)width;
    }
    __syncthreads();
    if (i < A0_REDO_NEURONS) {
        const double s = mean[lay] > 0.0 ? m[i] / mean[lay] : 0.0;
        const int d = s <= tau ? 1 : 0;
        scores[i] = (float)s; mask[i] = d; dorm[i] = d;
    }
    __syncthreads();
    if (i < 4) {
        int c = 0;
        for (int j = 0; j < width; ++j) c += dorm[lo + j];
        cnt[i] = c; counts[i] = c;
    }
    __syncthreads();
    if (i == 0) { counts[4] = cnt[0] + cnt[1] + cnt[2] + cnt[3]; counts[5] = state ? state[1] : 0; }
}

extern "C" int a0_redo_score(const float* act1, long long rows1, const float* act2, long long rows2, const float* act3, long long rows3, const float* fc1, long long rows4,
                             double tau, const int* state, int freq, int force, double* partials, float* scores, int* mask, int* counts, void* stream) {
    if (!act1 || !act2 || !act3 || !fc1 || !partials || !scores || !mask || !counts || rows1 < 1 || rows2 < 1 || rows3 < 1 || rows4 < 1 || (!force && !state) || freq < 0)
        return a0_fail(A0_EINVAL, "a0_redo_score: bad argument");
    if (!(tau >= 0.0) || !(tau < 1.0)) return a0_fail(A0_EINVAL, "a0_redo_score: tau must lie in [0, 1)");
    if ((((uintptr_t)act1) | ((uintptr_t)act2) | ((uintptr_t)act3) | ((uintptr_t)fc1)) & 15) return a0_fail(A0_EINVAL, "a0_redo_score: the activation buffers must be 16-byte aligned");
    if ((((uintptr_t)partials) & 7) || ((((uintptr_t)scores) | ((uintptr_t)mask) | ((uintptr_t)counts)) & 3)) return a0_fail(A0_EINVAL, "a0_redo_score: misaligned output");
    hipLaunchKernelGGL(a0_redo_sums_kernel, dim3(A0_REDO_PARTIALS), dim3(256), 0, (hipStream_t)stream, act1, rows1, act2, rows2, act3, rows3, fc1, rows4, state, freq, force, partials);
    hipLaunchKernelGGL(a0_redo_finish_kernel, dim3(1), dim3(1024), 0, (hipStream_t)stream, (const double*)partials, rows1, rows2, rows3, rows4, tau, state, freq, force,
                       scores, mask, counts);
    return a0_fail_hip((int)hipGetLastError(), "a0_redo_score");
}

// The recycle launch.  Blocks in flat order conv1, conv2, conv3, fc1, head; block b is [W (N x K) | bias (N)] at `off`; `in`: where its rows' neurons start in the
// mask (-1: the head, whose rows are no hidden neurons), `out`: where the neurons its columns read start (-1: conv1 reads pixels), column k reads neuron k % mod.
struct a0_redo_map { long long off[5]; int N[5], K[5], in[5], out[5], mod[5]; };

template <bool W>
__global__ __launch_bounds__(256) void a0_redo_recycle_kernel(float* __restrict__ p, float* __restrict__ m, float* __restrict__ v, long long n_adam, long long n_total, a0_reset_table T,
                                                              a0_redo_map D, const int* __restrict__ mask, unsigned long long seed_arg, const int* __restrict__ state, int freq,
                                                              int force, long long k_host, a0_wt_sink B) {
    if (!a0_redo_fires(state, freq, force)) return;
    const long long k = force ? k_host : (long long)(state[1] / freq);
    __shared__ unsigned char dm[A0_REDO_NEURONS];
    for (int i = threadIdx.x; i < A0_REDO_NEURONS; i += 256) dm[i] = mask[i] != 0 ? 1 : 0;
    __syncthreads();
    // the seed in a vector register, as in a0_net_reset_kernel
    uint32_t seed_v = (uint32_t)seed_arg;
    asm volatile("" : "+v"(seed_v));
    const unsigned long long seed = seed_v;
    const unsigned long long base = (unsigned long long)k * (unsigned long long)n_total;
    const long long stride = (long long)gridDim.x * blockDim.x;
    for (long long e = (long long)blockIdx.x * blockDim.x + threadIdx.x; e < n_adam; e += stride) {
        bool incoming = false, outgoing = false;
#pragma nounroll
        for (int b = 0; b < 5; ++b) {      // uniform loads of the by-value map, as a0_reset_find walks its table
            const long long nw = (long long)D.N[b] * D.K[b], r = e - D.off[b];
            if (r < 0 || r >= nw + D.N[b]) continue;
            if (r >= nw) { incoming = D.in[b] >= 0 && dm[D.in[b] + (int)(r - nw)]; continue; }      // a bias: incoming only
            const int n = (int)((unsigned)r / (unsigned)D.K[b]), kk = (int)r - n * D.K[b];
            incoming = D.in[b] >= 0 && dm[D.in[b] + n];
            outgoing = D.out[b] >= 0 && dm[D.out[b] + kk % D.mod[b]];
        }
        if (!incoming && !outgoing) continue;
        // an element that is both (the weight from a dormant neuron into a dormant neuron) ends at zero: the outgoing rule is applied last, as in ReDo's published code
        float x = 0.f;
        if (!outgoing) {
            const a0_reset_rule R = a0_reset_find(T, 0.f, e, n_total);
            if (R.kind < 0) continue;                  // the table has no rule for it: left alone
            x = a0_reset_fresh1(R, seed, base + (unsigned long long)e, A0_STREAM_REDO);
        }
        p[e] = x; m[e] = 0.f; v[e] = 0.f;
        if constexpr (W) a0_tail_wt1(B, true, false, e, x);
    }
}

extern "C" int a0_redo_recycle(float* params, float* exp_avg, float* exp_avg_sq, long long n_adam, long long n_total, const a0_net_reset_seg* segs, int n_segs,
                               const a0_redo_blocks* blocks, const int* mask, unsigned long long seed, const int* state, int freq, int force, long long k_host,
                               const a0_encoder_weights* w, int C, float* wt, void* stream) {
    if (!params || !exp_avg || !exp_avg_sq || !blocks || !mask || n_adam < 1 || n_total < n_adam || (!force && !state) || freq < 0 || (force && k_host < 0) ||
        ((((uintptr_t)params) | ((uintptr_t)exp_avg) | ((uintptr_t)exp_avg_sq) | ((uintptr_t)mask)) & 3))
        return a0_fail(A0_EINVAL, "a0_redo_recycle: bad argument");
    a0_reset_table T;
    if (int e = a0_reset_table_make(&T, "a0_redo_recycle", segs, n_segs, n_adam)) return e;
    if (blocks->K1 < 1 || blocks->feat < 64 || blocks->feat % 64 != 0 || blocks->Npad < 1) return a0_fail(A0_EINVAL, "a0_redo_recycle: K1 >= 1, feat a positive multiple of 64, Npad >= 1");
    a0_redo_map D;
    const long long off[5] = {blocks->conv1, blocks->conv2, blocks->conv3, blocks->fc1, blocks->head};
    const int N[5] = {32, 64, 64, 512, blocks->Npad}, K[5] = {blocks->K1, 512, 576, blocks->feat, 512};
    const int in[5] = {0, 32, 96, 160, -1}, out[5] = {-1, 0, 32, 96, 160}, mod[5] = {1, 32, 64, 64, 512};
    long long at = 0;
    for (int b = 0; b < 5; ++b) {
        if (off[b] < at || off[b] + (long long)N[b] * K[b] + N[b] > n_adam) return a0_fail(A0_EINVAL, "a0_redo_recycle: the blocks conv1, conv2, conv3, fc1, head must be ascending, disjoint and inside [0, n_adam)");
        at = off[b] + (long long)N[b] * K[b] + N[b];
        D.off[b] = off[b]; D.N[b] = N[b]; D.K[b] = K[b]; D.in[b] = in[b]; D.out[b] = out[b]; D.mod[b] = mod[b];
    }
    a0_wt_sink B{0, 0, 0, 0, 0, nullptr, nullptr};
    if (wt) {
        if (int e = a0_wt_sink_make(&B, "a0_redo_recycle", "params", params, n_total, w, C, nullptr, wt)) return e;
        if (B.o1 != blocks->conv1 || B.o2 != blocks->conv2 || B.o3 != blocks->conv3 || B.K1 != blocks->K1)
            return a0_fail(A0_EINVAL, "a0_redo_recycle: the encoder weights and the block descriptors name different convolution blocks");
        B.wt = wt; B.wt_t = nullptr;                   // the online copy alone: the target follows at its next sync or blend
    }
    const unsigned long long seed32 = seed & 0xFFFFFFFFull;
    hipLaunchKernelGGL(wt ? a0_redo_recycle_kernel<true> : a0_redo_recycle_kernel<false>, dim3(a0_grid_256(n_adam)), dim3(256), 0, (hipStream_t)stream, params, exp_avg, exp_avg_sq, n_adam,
                       n_total, T, D, mask, seed32, state, freq, force, k_host, B);
    return a0_fail_hip((int)hipGetLastError(), "a0_redo_recycle");
}

// ------------------------------------------------------------------------------------------------ NoisyNet
// W = mu + sigma * (f(eps_out) x f(eps_in)),  b = mu_b + sigma_b * f(eps_b),  f(x) = sign(x) sqrt|x|
// (reference agent0/deepq/model.py:54-62,73-87).  Blocks are [W (N*K) | b (N)]; one call handles the rows [r0, r1) that
// belong to one NoisyLinear module (q_head and value_head share a packed block but have their own noise vectors).
A0_D float a0_noise_f(float x) { return (x > 0.f ? 1.f : (x < 0.f ? -1.f : 0.f)) * sqrtf(fabsf(x)); }

__global__ void a0_noisy_compose_kernel(const float* __restrict__ mu, const float* __restrict__ sigma, float* __restrict__ eff, int N, int K,
                                        int r0, int r1, const float* __restrict__ noise_in, const float* __restrict__ noise_out_w,
                                        const float* __restrict__ noise_out_b) {
    const long long rows = r1 - r0;
    const long long total = rows * K + rows;
    long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    const long long stride = (long long)gridDim.x * blockDim.x;
    for (; i < total; i += stride) {
        long long off; float e;
        if (i < rows * K) {
            const int n = (int)(i / K), k = (int)(i % K);
            off = (long long)(r0 + n) * K + k;
            e = a0_noise_f(noise_out_w[n]) * a0_noise_f(noise_in[k]);
        } else {
            const int n = (int)(i - rows * K);
            off = (long long)N * K + r0 + n;
            e = a0_noise_f(noise_out_b[n]);
        }
        eff[off] = mu[off] + sigma[off] * e;
    }
}

// gradient fan-out: the weight-gradient kernels write d(eff) into the mu block (d mu = d eff); d sigma = d eff * eps
__global__ void a0_noisy_grad_sigma_kernel(const float* __restrict__ gmu, float* __restrict__ gsigma, int N, int K, int r0, int r1,
                                           const float* __restrict__ noise_in, const float* __restrict__ noise_out_w,
                                           const float* __restrict__ noise_out_b) {
    const long long rows = r1 - r0;
    const long long total = rows * K + rows;
    long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    const long long stride = (long long)gridDim.x * blockDim.x;
    for (; i < total; i += stride) {
        long long off; float e;
        if (i < rows * K) {
            const int n = (int)(i / K), k = (int)(i % K);
            off = (long long)(r0 + n) * K + k;
            e = a0_noise_f(noise_out_w[n]) * a0_noise_f(noise_in[k]);
        } else {
            const int n = (int)(i - rows * K);
            off = (long long)N * K + r0 + n;
            e = a0_noise_f(noise_out_b[n]);
        }
        gsigma[off] = gmu[off] * e;
    }
}

// Up to six NoisyLinear modules (first_dense, q_head, value_head of the online AND the target network: round 4) in one launch: workgroups [first_block[m], first_block[m+1]) serve module m.
struct a0_noisy_mod { const float* mu; const float* sigma; float* out; int N, K, r0, r1; const float* noise_in; const float* noise_out_w; const float* noise_out_b; };
struct a0_noisy_multi_args { a0_noisy_mod mod[6]; int first_block[7]; };

template <bool GRAD>
__global__ void a0_noisy_multi_kernel(a0_noisy_multi_args A) {
    int mi = 0;
#pragma unroll
    for (int k = 1; k < 6; ++k) mi += ((int)blockIdx.x >= A.first_block[k]) ? 1 : 0;
    const a0_noisy_mod M = A.mod[mi];
    const int nblk = A.first_block[mi + 1] - A.first_block[mi];
    const long long rows = M.r1 - M.r0;
    const long long total = rows * M.K + rows;
    long long i = (long long)((int)blockIdx.x - A.first_block[mi]) * blockDim.x + threadIdx.x;
    const long long stride = (long long)nblk * blockDim.x;
    for (; i < total; i += stride) {
        long long off; float e;
        if (i < rows * M.K) {
            const int n = (int)(i / M.K), k = (int)(i % M.K);
            off = (long long)(M.r0 + n) * M.K + k;
            e = a0_noise_f(M.noise_out_w[n]) * a0_noise_f(M.noise_in[k]);
        } else {
            const int n = (int)(i - rows * M.K);
            off = (long long)M.N * M.K + M.r0 + n;
            e = a0_noise_f(M.noise_out_b[n]);
        }
        if (GRAD) M.out[off] = M.mu[off] * e;                 // d sigma = d eff * eps (mu = the gradient written into the mu block)
        else M.out[off] = M.mu[off] + M.sigma[off] * e;       // eff = mu + sigma * eps
    }
}

// The same, four k per lane: 16-byte loads and stores, 32-bit index arithmetic (the element-wise kernel spends its time in a 64-bit division per element; this one
// runs at the HBM rate).  Every element is formed by the same expression as above; needs K % 4 == 0 and 16-byte aligned blocks / noise vectors (the packed layout's).
template <bool GRAD>
__global__ __launch_bounds__(256) void a0_noisy_multi_v4_kernel(a0_noisy_multi_args A) {
    int mi = 0;
#pragma unroll
    for (int k = 1; k < 6; ++k) mi += ((int)blockIdx.x >= A.first_block[k]) ? 1 : 0;
    const a0_noisy_mod M = A.mod[mi];
    const unsigned nblk = (unsigned)(A.first_block[mi + 1] - A.first_block[mi]);
    const unsigned rows = (unsigned)(M.r1 - M.r0), K4 = (unsigned)M.K >> 2, nw = rows * K4, total = nw + rows;
    const unsigned stride = nblk * 256u;
    for (unsigned i = ((unsigned)blockIdx.x - (unsigned)A.first_block[mi]) * 256u + threadIdx.x; i < total; i += stride) {
        if (i < nw) {
            const unsigned n = i / K4, k4 = i - n * K4;
            const long long off = (long long)(M.r0 + (int)n) * M.K + 4 * k4;
            const float eo = a0_noise_f(M.noise_out_w[n]);
            const a0_f4 ni = *(const a0_f4*)(M.noise_in + 4 * k4);
            const float e0 = eo * a0_noise_f(ni.x), e1 = eo * a0_noise_f(ni.y), e2 = eo * a0_noise_f(ni.z), e3 = eo * a0_noise_f(ni.w);
            const a0_f4 mu = *(const a0_f4*)(M.mu + off);
            a0_f4 o;
            if (GRAD) { o.x = mu.x * e0; o.y = mu.y * e1; o.z = mu.z * e2; o.w = mu.w * e3; }
            else {
                const a0_f4 sg = *(const a0_f4*)(M.sigma + off);
                o.x = mu.x + sg.x * e0; o.y = mu.y + sg.y * e1; o.z = mu.z + sg.z * e2; o.w = mu.w + sg.w * e3;
            }
            *(a0_f4*)(M.out + off) = o;
        } else {
            const unsigned n = i - nw;
            const long long off = (long long)M.N * M.K + M.r0 + (int)n;
            const float e = a0_noise_f(M.noise_out_b[n]);
            if (GRAD) M.out[off] = M.mu[off] * e;
            else M.out[off] = M.mu[off] + M.sigma[off] * e;
        }
    }
}

// nmod <= 6 modules; arrays are host arrays.  grad = 0: eff[m] = mu[m] + sigma[m] * eps (a0_noisy_compose per module);
// grad = 1: gsigma[m] (passed as eff) = gmu[m] (passed as mu) * eps (a0_noisy_grad_sigma per module; sigma unused).
extern "C" int a0_noisy_multi(int grad, int nmod, const float* const* mu, const float* const* sigma, float* const* eff, const int* N, const int* K, const int* r0,
                              const int* r1, const float* const* noise_in, const float* const* noise_out_w, const float* const* noise_out_b, void* stream) {
    if (nmod < 1 || nmod > 6 || !mu || !eff || !N || !K || !r0 || !r1 || !noise_in || !noise_out_w || !noise_out_b || (!grad && !sigma))
        return a0_fail(A0_EINVAL, "a0_noisy_multi: bad argument");
    a0_noisy_multi_args A;
    int blocks = 0;
    bool v4 = true;      // the four-wide kernel, unless an operand is unaligned or K not a multiple of 4
    for (int m = 0; m < nmod && v4; ++m)
        v4 = mu[m] && eff[m] && noise_in[m] && K[m] % 4 == 0 && (long long)N[m] * K[m] < (1LL << 31) &&
             (((uintptr_t)mu[m] | (uintptr_t)eff[m] | (uintptr_t)noise_in[m] | (grad ? 0 : (uintptr_t)sigma[m])) & 15) == 0;
    for (int m = 0; m < 6; ++m) {
        A.first_block[m] = blocks;
        if (m < nmod) {
            if (!mu[m] || !eff[m] || (!grad && !sigma[m]) || !noise_in[m] || !noise_out_w[m] || !noise_out_b[m] || N[m] < 1 || K[m] < 1 || r0[m] < 0 || r1[m] <= r0[m] || r1[m] > N[m])
                return a0_fail(A0_EINVAL, "a0_noisy_multi: bad module");
            A.mod[m] = a0_noisy_mod{mu[m], grad ? nullptr : sigma[m], eff[m], N[m], K[m], r0[m], r1[m], noise_in[m], noise_out_w[m], noise_out_b[m]};
            long long b = v4 ? ((long long)(r1[m] - r0[m]) * (K[m] / 4 + 1) + 255) / 256 : ((long long)(r1[m] - r0[m]) * (K[m] + 1) + 255) / 256;
            if (b > 2048) b = 2048;
            blocks += (int)b;
        } else {
            A.mod[m] = a0_noisy_mod{nullptr, nullptr, nullptr, 1, 1, 0, 0, nullptr, nullptr, nullptr};
        }
    }
    for (int m = nmod + 1; m <= 6; ++m) A.first_block[m] = 0x7fffffff;       // unused modules are never selected
    A.first_block[nmod] = blocks;                                              // end of the last real module
    if (v4 && grad) hipLaunchKernelGGL(a0_noisy_multi_v4_kernel<true>, dim3((unsigned)blocks), dim3(256), 0, (hipStream_t)stream, A);
    else if (v4) hipLaunchKernelGGL(a0_noisy_multi_v4_kernel<false>, dim3((unsigned)blocks), dim3(256), 0, (hipStream_t)stream, A);
    else if (grad) hipLaunchKernelGGL(a0_noisy_multi_kernel<true>, dim3((unsigned)blocks), dim3(256), 0, (hipStream_t)stream, A);
    else hipLaunchKernelGGL(a0_noisy_multi_kernel<false>, dim3((unsigned)blocks), dim3(256), 0, (hipStream_t)stream, A);
    return a0_fail_hip((int)hipGetLastError(), "a0_noisy_multi");
}

extern "C" int a0_noisy_compose(const float* mu, const float* sigma, float* eff, int N, int K, int r0, int r1, const float* noise_in,
                                const float* noise_out_w, const float* noise_out_b, void* stream) {
    if (!mu || !sigma || !eff || !noise_in || !noise_out_w || !noise_out_b || N < 1 || K < 1 || r0 < 0 || r1 <= r0 || r1 > N) return a0_fail(A0_EINVAL, "a0_noisy_compose: bad argument");
    long long total = (long long)(r1 - r0) * (K + 1), blocks = (total + 255) / 256;
    if (blocks > 2048) blocks = 2048;
    hipLaunchKernelGGL(a0_noisy_compose_kernel, dim3((unsigned)blocks), dim3(256), 0, (hipStream_t)stream, mu, sigma, eff, N, K, r0, r1, noise_in, noise_out_w, noise_out_b);
    return a0_fail_hip((int)hipGetLastError(), "a0_noisy_compose");
}

extern "C" int a0_noisy_grad_sigma(const float* gmu, float* gsigma, int N, int K, int r0, int r1, const float* noise_in,
                                   const float* noise_out_w, const float* noise_out_b, void* stream) {
    if (!gmu || !gsigma || !noise_in || !noise_out_w || !noise_out_b || N < 1 || K < 1 || r0 < 0 || r1 <= r0 || r1 > N) return a0_fail(A0_EINVAL, "a0_noisy_grad_sigma: bad argument");
    long long total = (long long)(r1 - r0) * (K + 1), blocks = (total + 255) / 256;
    if (blocks > 2048) blocks = 2048;
    hipLaunchKernelGGL(a0_noisy_grad_sigma_kernel, dim3((unsigned)blocks), dim3(256), 0, (hipStream_t)stream, gmu, gsigma, N, K, r0, r1, noise_in, noise_out_w, noise_out_b);
    return a0_fail_hip((int)hipGetLastError(), "a0_noisy_grad_sigma");
}
