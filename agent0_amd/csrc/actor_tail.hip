// Every actor tail, alone and merged with the synthetic env's step, and their launchers: the scalar heads' (dqn / mdqn), which start with their fc1 (a0_actor_fc1_slabs,
// dense.hip), and those over the head GEMM's split-K slabs — c51 / qr (one row per env) and iqn / fqf (a row per env and fraction).  No file-scope contraction pragma
// here: the tails' multiply-adds fuse as the compiler's default has them.
#include "a0_internal.h"
#include "actor_step.h"
#include "actor_tail.h"      // a0_wave_sum / a0_wave_max, the actor tails' device functions

// ------------------------------------------------------------------------------------------------ actor tail for distributional heads
// Everything between the head GEMM and the chosen action of Actor.act (reference agent.py:25-39 with model.py:163-177 / 190-192
// behind it) for c51 and qr: the head GEMM leaves its split-K slabs (a0_dense_fwd_partial) and this kernel sums them in slab order and
// adds the bias (== a0_reduce_bias_act_kernel), applies the dueling combine per atom (== a0_dueling_fwd_kernel), takes the expectation
// (c51: softmax over atoms x support; qr: mean over quantiles) and the first maximum (== a0_select_action_kernel) and makes the
// epsilon-greedy draw from the actor's Philox streams (== a0_egreedy_rng_kernel).  Same arithmetic, statement for statement, as the four
// kernels it replaces; one wave per environment, the row's head outputs live in LDS.
#include "philox.h"
__global__ __launch_bounds__(256) void a0_actor_dist_tail_kernel(const float* __restrict__ slabs, long long slab_stride, int nslab, const float* __restrict__ bias,
                                                                 int ld, int A, int T, int dueling, int mode, const float* __restrict__ atoms, int E,
                                                                 unsigned long long seed, uint32_t stream_a, uint32_t stream_u, unsigned long long off_a,
                                                                 unsigned long long off_u, float eps, const long long* __restrict__ ctrl,
                                                                 const float* __restrict__ eps_ptr, int* __restrict__ action, float* __restrict__ qmax) {
    extern __shared__ float xs_all[];                    // [4 waves][A*T + T]
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int e = blockIdx.x * 4 + wave;
    const int er = e < E ? e : E - 1;
    const int NC = A * T + (dueling ? T : 0);
    float* xs = xs_all + (size_t)wave * (A * T + T);
    // head output = slab sum in slab order + bias
    const float* sp = slabs + (long long)er * ld;
    for (int c0 = lane; c0 < NC; c0 += 256) {          // four columns x eight slabs requested before any is added; additions in slab order
        float acc[4] = {0.f, 0.f, 0.f, 0.f};
        for (int z = 0; z < nslab; z += 8) {
            float t[8][4];
#pragma unroll
            for (int zz = 0; zz < 8; ++zz)
#pragma unroll
                for (int j = 0; j < 4; ++j) {
                    const int c = c0 + 64 * j;
                    t[zz][j] = (z + zz < nslab && c < NC) ? sp[(long long)(z + zz) * slab_stride + c] : 0.f;
                }
#pragma unroll
            for (int zz = 0; zz < 8; ++zz)
                if (z + zz < nslab) {
#pragma unroll
                    for (int j = 0; j < 4; ++j) acc[j] += t[zz][j];
                }
        }
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const int c = c0 + 64 * j;
            if (c < NC) xs[c] = acc[j] + bias[c];
        }
    }
    __syncthreads();
    if (dueling) {
        for (int t = lane; t < T; t += 64) {
            float s = 0.f;
            for (int a = 0; a < A; ++a) s += xs[a * T + t];
            const float mean = s / (float)A;
            const float v = xs[A * T + t];
            for (int a = 0; a < A; ++a) xs[a * T + t] = v + (xs[a * T + t] - mean);
        }
    }
    __syncthreads();
    float best = 0.f;
    int besta = 0;
    for (int a = 0; a < A; ++a) {
        const float* p = xs + a * T;
        float v;
        if (mode == 1) {
            float s = 0.f;
            for (int t = lane; t < T; t += 64) s += p[t];
            v = a0_wave_sum(s) / (float)T;
        } else {
            float mx = -INFINITY;
            for (int t = lane; t < T; t += 64) mx = fmaxf(mx, p[t]);
            mx = a0_wave_max(mx);
            float se = 0.f, sz = 0.f;
            for (int t = lane; t < T; t += 64) {
                float ex = expf(p[t] - mx);
                se += ex;
                sz += ex * atoms[t];
            }
            se = a0_wave_sum(se);
            sz = a0_wave_sum(sz);
            v = sz / se;
        }
        if (a == 0 || v > best) { best = v; besta = a; }   // first maximum wins, like torch.argmax on CPU
    }
    if (lane != 0 || e >= E) return;
    if (ctrl) { off_a += (unsigned long long)ctrl[A0_CTRL_RNG_ACTION]; off_u += (unsigned long long)ctrl[A0_CTRL_RNG_UNIFORM]; }
    eps = a0_env_eps(eps, eps_ptr, (uint32_t)__builtin_amdgcn_readfirstlane(e));      // one env per wave
    const int ra = (int)(a0_philox_word(seed, stream_a, off_a + (unsigned long long)e) % (uint32_t)A);
    const float u = (float)(a0_philox_word(seed, stream_u, off_u + (unsigned long long)e) >> 8) * 0x1.0p-24f;
    action[e] = (u > eps) ? besta : ra;
    qmax[e] = best;
}

// ---- the same tail AND the synthetic env's step in one launch, a workgroup per env (the distributional counterpart of
// a0_actor_qhead_env_kernel, below): all four waves sum the head's slabs into LDS (one column per thread: the same slab-order additions),
// then wave 0 alone applies the dueling combine, takes the expectation and the first maximum, draws the action and does the env's scalar work
// with it, while waves 1-3 already write the new frame, the shifted stack and the replay row.  Same bytes as a0_actor_dist_tail +
// a0_env_synth_step_commit.
// (a0_dtenv_args + a0_actor_dist_tail_env_body live in actor_tail.h: shared with the kernel that goes on to encode the next observation, encoder_fused.hip)
__global__ __launch_bounds__(512) void a0_actor_dist_tail_env_kernel(a0_dtenv_args P) {
    extern __shared__ float xs[];                        // [max(A*T + T, ld)] head outputs of this env
    __shared__ int s_chase_cell;
    a0_actor_dist_tail_env_body(P, xs, &s_chase_cell);
}

// the head and draw arguments every slab tail takes, with or without the env step: pointers, ranges, the row width and slab stride of its layout, its two modes
static bool a0_slab_head_ok(const a0_slab_head& h, int E, const a0_step_draw& draw) {
    const int A = h.A, T = h.T, other = h.kt ? 3 : 2;
    return !(!h.slabs || !h.bias || !draw.action || !draw.qmax || E < 1 || A < 1 || T < 1 || h.nslab < 1 ||
             (h.kt ? h.ld < A + (h.dueling ? 1 : 0) || h.slab_stride < (long long)E * T * h.ld : h.ld < A * T + (h.dueling ? T : 0) || h.slab_stride < (long long)E * h.ld) ||
             (h.mode != 1 && h.mode != other) || (h.mode == other && !(h.kt ? h.taus : h.atoms)));
}

// The launcher of the merged step for both slab layouts (a0_internal.h).  head.kt = 0 — c51 / qr: the head GEMM leaves [nslab][E][ld], 160 KB of LDS at most, its width
// the padded row's where the slab sum runs 16 bytes wide; head.kt = 1 — the quantile networks (iqn: mean over the K sampled quantiles, mode 1; fqf: sum over the F
// fractions weighted by their widths, mode 3): the head GEMM over E * T rows leaves [nslab][E * T][ld] (a0_dense_fwd_partial), 64 KB at most.  Per env one workgroup sums
// the slabs in slab order and adds the bias (== a0_reduce_bias_act), applies the dueling combine (== a0_dueling_fwd), takes the action values and the first maximum (==
// a0_select_action), draws epsilon-greedy (== a0_egreedy_rng) and steps the env (== a0_env_synth_step_commit): five launches of reference agent.py:25-39 / 44-90's
// per-step work become one.  With `next` the workgroups go on to encode their env's new observation (a0_actor_dist_step_enc_kernel, encoder_fused.hip; rounds 5 / 6):
// an actor step is encoder-less between a rollout's first and last step.
int a0_actor_slab_tail_env_launch(const a0_slab_head& h, int E, const a0_step_draw& draw, const a0_env_commit& env, const a0_next_enc* next, hipStream_t st) {
    const std::string who = std::string(h.kt ? "a0_actor_quantile_tail_env_step" : "a0_actor_dist_tail_env_step") + (next ? "_enc" : "");
    const int A = h.A, T = h.T;
    if (!a0_slab_head_ok(h, E, draw)) return a0_fail(A0_EINVAL, (who + ": bad argument").c_str());
    { const int rc = a0_env_commit_check(env, E, A, who.c_str()); if (rc != A0_OK) return rc; }
    const bool vec4 = !(h.ld & 3) && !(h.slab_stride & 3) && !((((uintptr_t)h.slabs) | ((uintptr_t)h.bias)) & 15);
    const size_t lds = (size_t)(h.kt || (A * T + T) > h.ld || !vec4 ? (A * T + T) : h.ld) * sizeof(float);
    if (lds > (size_t)(h.kt ? 64 : 160) * 1024) return a0_fail(A0_EINVAL, (who + ": head too wide for LDS").c_str());
    if (!h.kt && !next) {
        static size_t configured = 0;
        if (lds > configured) {
            if (hipFuncSetAttribute((const void*)a0_actor_dist_tail_env_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds) != hipSuccess)
                return a0_fail(A0_EINVAL, (who + ": LDS").c_str());
            configured = lds;
        }
    }
    a0_dtenv_args P;
    P.slabs = h.slabs; P.slab_stride = h.slab_stride; P.nslab = h.nslab; P.bias = h.bias; P.ld = h.ld; P.A = A; P.T = T; P.dueling = h.dueling; P.mode = h.mode; P.atoms = h.atoms; P.E = E;
    a0_step_fill(P, draw, env);
    P.kt = h.kt; P.taus = h.taus; P.vec4 = vec4 ? 1 : 0;
    if (next) return a0_actor_dist_step_enc_launch(P, lds, next->wt, next->w, next->act3_next, st);
    hipLaunchKernelGGL(a0_actor_dist_tail_env_kernel, dim3(E), dim3(512), lds, st, P);
    return a0_fail_hip((int)hipGetLastError(), who.c_str());
}

extern "C" int a0_actor_dist_tail_env_step(const float* slabs, long long slab_stride, int nslab, const float* bias, int ld, int A, int T, int dueling, int mode,
                                           const float* atoms, int E, unsigned long long seed, unsigned int stream_a, unsigned int stream_u, unsigned long long off_a,
                                           unsigned long long off_u, float eps, const long long* ctrl, const float* eps_ptr, int* action, float* qmax,
                                           unsigned long long env_seed, unsigned int rank, unsigned int g, const uint8_t* obs_in, uint8_t* obs_out, float* ep_ret,
                                           float* final_mask, float* final_ret, int n, long long steps, double gamma, int* ring_act, float* ring_rew, float* ring_done,
                                           const uint8_t* obs0, uint8_t* frames, long long cap, long long start_slot, int* r_act, float* r_rew, float* r_done, int task, void* stream) {
    const a0_slab_head head{slabs, slab_stride, nslab, bias, ld, A, T, dueling, mode, atoms, nullptr, 0};
    const a0_step_draw draw{seed, stream_a, stream_u, off_a, off_u, eps, ctrl, eps_ptr, action, qmax};
    const a0_env_commit env{env_seed, rank, g, obs_in, obs_out, ep_ret, final_mask, final_ret, n, steps, gamma, ring_act, ring_rew, ring_done, obs0, frames, cap, start_slot, r_act, r_rew, r_done, task};
    return a0_actor_slab_tail_env_launch(head, E, draw, env, nullptr, (hipStream_t)stream);
}

extern "C" int a0_actor_dist_tail_env_step_enc(const float* slabs, long long slab_stride, int nslab, const float* bias, int ld, int A, int T, int dueling, int mode,
                                           const float* atoms, int E, unsigned long long seed, unsigned int stream_a, unsigned int stream_u, unsigned long long off_a,
                                           unsigned long long off_u, float eps, const long long* ctrl, const float* eps_ptr, int* action, float* qmax,
                                           unsigned long long env_seed, unsigned int rank, unsigned int g, const uint8_t* obs_in, uint8_t* obs_out, float* ep_ret,
                                           float* final_mask, float* final_ret, int n, long long steps, double gamma, int* ring_act, float* ring_rew, float* ring_done,
                                           const uint8_t* obs0, uint8_t* frames, long long cap, long long start_slot, int* r_act, float* r_rew, float* r_done, int task,
                                               const float* wt, const a0_encoder_weights* w, float* act3_next, void* stream) {
    const a0_slab_head head{slabs, slab_stride, nslab, bias, ld, A, T, dueling, mode, atoms, nullptr, 0};
    const a0_step_draw draw{seed, stream_a, stream_u, off_a, off_u, eps, ctrl, eps_ptr, action, qmax};
    const a0_env_commit env{env_seed, rank, g, obs_in, obs_out, ep_ret, final_mask, final_ret, n, steps, gamma, ring_act, ring_rew, ring_done, obs0, frames, cap, start_slot, r_act, r_rew, r_done, task};
    const a0_next_enc next{wt, w, act3_next};
    return a0_actor_slab_tail_env_launch(head, E, draw, env, &next, (hipStream_t)stream);
}

// mode 1: mean over the T sampled quantiles (iqn); mode 3: the fractions' widths from `taus` [E][T + 1] (fqf)
extern "C" int a0_actor_quantile_tail_env_step(const float* slabs, long long slab_stride, int nslab, const float* bias, int ld, int A, int T, int dueling, int mode,
                                               const float* taus, int E, unsigned long long seed, unsigned int stream_a, unsigned int stream_u, unsigned long long off_a,
                                               unsigned long long off_u, float eps, const long long* ctrl, const float* eps_ptr, int* action, float* qmax,
                                               unsigned long long env_seed, unsigned int rank, unsigned int g, const uint8_t* obs_in, uint8_t* obs_out, float* ep_ret,
                                               float* final_mask, float* final_ret, int n, long long steps, double gamma, int* ring_act, float* ring_rew, float* ring_done,
                                               const uint8_t* obs0, uint8_t* frames, long long cap, long long start_slot, int* r_act, float* r_rew, float* r_done, int task, void* stream) {
    const a0_slab_head head{slabs, slab_stride, nslab, bias, ld, A, T, dueling, mode, nullptr, taus, 1};
    const a0_step_draw draw{seed, stream_a, stream_u, off_a, off_u, eps, ctrl, eps_ptr, action, qmax};
    const a0_env_commit env{env_seed, rank, g, obs_in, obs_out, ep_ret, final_mask, final_ret, n, steps, gamma, ring_act, ring_rew, ring_done, obs0, frames, cap, start_slot, r_act, r_rew, r_done, task};
    return a0_actor_slab_tail_env_launch(head, E, draw, env, nullptr, (hipStream_t)stream);
}

extern "C" int a0_actor_quantile_tail_env_step_enc(const float* slabs, long long slab_stride, int nslab, const float* bias, int ld, int A, int T, int dueling, int mode,
                                                   const float* taus, int E, unsigned long long seed, unsigned int stream_a, unsigned int stream_u, unsigned long long off_a,
                                                   unsigned long long off_u, float eps, const long long* ctrl, const float* eps_ptr, int* action, float* qmax,
                                                   unsigned long long env_seed, unsigned int rank, unsigned int g, const uint8_t* obs_in, uint8_t* obs_out, float* ep_ret,
                                                   float* final_mask, float* final_ret, int n, long long steps, double gamma, int* ring_act, float* ring_rew, float* ring_done,
                                                   const uint8_t* obs0, uint8_t* frames, long long cap, long long start_slot, int* r_act, float* r_rew, float* r_done, int task,
                                                   const float* wt, const a0_encoder_weights* w, float* act3_next, void* stream) {
    const a0_slab_head head{slabs, slab_stride, nslab, bias, ld, A, T, dueling, mode, nullptr, taus, 1};
    const a0_step_draw draw{seed, stream_a, stream_u, off_a, off_u, eps, ctrl, eps_ptr, action, qmax};
    const a0_env_commit env{env_seed, rank, g, obs_in, obs_out, ep_ret, final_mask, final_ret, n, steps, gamma, ring_act, ring_rew, ring_done, obs0, frames, cap, start_slot, r_act, r_rew, r_done, task};
    const a0_next_enc next{wt, w, act3_next};
    return a0_actor_slab_tail_env_launch(head, E, draw, env, &next, (hipStream_t)stream);
}

// The same quantile tail WITHOUT the env step, for every actor step that has no device env to merge it with: host environments (one group or several,
// Actor._rollout_host / _rollout_groups) and test rollouts.  One wave per env runs wave 0 of a0_actor_dist_tail_env_kernel with the env's work compiled out
// (a0_actor_dist_tail_wave0<false>): slab sum in slab order + bias, dueling combine per quantile, action values (modes 1 / 3), first maximum, epsilon-greedy
// draw — the same bytes as the merged kernel and as the four launches it replaces (a0_reduce_bias_act, a0_dueling_fwd, a0_select_action, a0_actor_egreedy_rng).
__global__ __launch_bounds__(64) void a0_actor_quantile_tail_kernel(a0_dtenv_args P) {
    extern __shared__ float xs[];                        // [A*T + T] head outputs of this env
    a0_actor_dist_tail_wave0<false>(P, xs, nullptr, 0u, 0, a0_u4{0u, 0u, 0u, 0u});
}

// The launcher of both slab tails WITHOUT an env step (a0_internal.h): head.kt = 0 — a0_actor_dist_tail_kernel, four envs per workgroup, 160 KB of LDS at most; head.kt = 1 —
// a0_actor_quantile_tail_kernel, an env per workgroup, 64 KB at most.  The exported a0_actor_dist_tail / a0_actor_quantile_tail pack into it, under whose names its errors
// read; the actor handle's rollout over a host-env pool calls it with the descriptors it fills for the merged step.
int a0_actor_slab_tail_launch(const a0_slab_head& h, int E, const a0_step_draw& d, hipStream_t st) {
    static const char* const MSG[2][4] = {
        {"a0_actor_dist_tail: bad argument", "a0_actor_dist_tail: head too wide for LDS", "a0_actor_dist_tail: LDS", "a0_actor_dist_tail"},
        {"a0_actor_quantile_tail: bad argument", "a0_actor_quantile_tail: head too wide for LDS", "a0_actor_quantile_tail: LDS", "a0_actor_quantile_tail"}};
    const char* const* msg = MSG[h.kt ? 1 : 0];
    if (!a0_slab_head_ok(h, E, d)) return a0_fail(A0_EINVAL, msg[0]);
    const int A = h.A, T = h.T;
    const size_t lds = (size_t)(h.kt ? 1 : 4) * (A * T + T) * sizeof(float);
    if (lds > (size_t)(h.kt ? 64 : 160) * 1024) return a0_fail(A0_EINVAL, msg[1]);
    if (h.kt) {
        a0_dtenv_args P = {};
        P.slabs = h.slabs; P.slab_stride = h.slab_stride; P.nslab = h.nslab; P.bias = h.bias; P.ld = h.ld; P.A = A; P.T = T; P.dueling = h.dueling; P.mode = h.mode; P.atoms = nullptr; P.E = E;
        P.rng_seed = d.seed; P.stream_a = d.stream_a; P.stream_u = d.stream_u; P.off_a = d.off_a; P.off_u = d.off_u; P.eps = d.eps; P.ctrl = d.ctrl; P.eps_ptr = d.eps_ptr;
        P.action = d.action; P.qmax = d.qmax;
        P.task = A0_ENV_TASK_STREAM;
        P.kt = 1; P.taus = h.taus;
        P.vec4 = (!(h.ld & 3) && !(h.slab_stride & 3) && !((((uintptr_t)h.slabs) | ((uintptr_t)h.bias)) & 15)) ? 1 : 0;
        hipLaunchKernelGGL(a0_actor_quantile_tail_kernel, dim3(E), dim3(64), lds, st, P);
        return a0_fail_hip((int)hipGetLastError(), msg[3]);
    }
    static size_t configured = 0;
    if (lds > configured) {
        if (hipFuncSetAttribute((const void*)a0_actor_dist_tail_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds) != hipSuccess) return a0_fail(A0_EINVAL, msg[2]);
        configured = lds;
    }
    hipLaunchKernelGGL(a0_actor_dist_tail_kernel, dim3((E + 3) / 4), dim3(256), lds, st, h.slabs, h.slab_stride, h.nslab, h.bias, h.ld, A, T, h.dueling, h.mode, h.atoms, E,
                       d.seed, d.stream_a, d.stream_u, d.off_a, d.off_u, d.eps, d.ctrl, d.eps_ptr, d.action, d.qmax);
    return a0_fail_hip((int)hipGetLastError(), msg[3]);
}

// mode 1: mean over the T sampled quantiles (iqn); mode 3: the fractions' widths from `taus` [E][T + 1] (fqf)
extern "C" int a0_actor_quantile_tail(const float* slabs, long long slab_stride, int nslab, const float* bias, int ld, int A, int T, int dueling, int mode,
                                      const float* taus, int E, unsigned long long seed, unsigned int stream_a, unsigned int stream_u, unsigned long long off_a,
                                      unsigned long long off_u, float eps, const long long* ctrl, const float* eps_ptr, int* action, float* qmax, void* stream) {
    const a0_slab_head head{slabs, slab_stride, nslab, bias, ld, A, T, dueling, mode, nullptr, taus, 1};
    const a0_step_draw draw{seed, stream_a, stream_u, off_a, off_u, eps, ctrl, eps_ptr, action, qmax};
    return a0_actor_slab_tail_launch(head, E, draw, (hipStream_t)stream);
}

// mode 1: mean over the T quantiles (qr); mode 2: C51 expectation with `atoms` [T]
extern "C" int a0_actor_dist_tail(const float* slabs, long long slab_stride, int nslab, const float* bias, int ld, int A, int T, int dueling, int mode,
                                  const float* atoms, int E, unsigned long long seed, unsigned int stream_a, unsigned int stream_u, unsigned long long off_a,
                                  unsigned long long off_u, float eps, const long long* ctrl, const float* eps_ptr, int* action, float* qmax, void* stream) {
    const a0_slab_head head{slabs, slab_stride, nslab, bias, ld, A, T, dueling, mode, atoms, nullptr, 0};
    const a0_step_draw draw{seed, stream_a, stream_u, off_a, off_u, eps, ctrl, eps_ptr, action, qmax};
    return a0_actor_slab_tail_launch(head, E, draw, (hipStream_t)stream);
}

// ------------------------------------------------------------------------------------------------ fused actor tail (dqn / mdqn)
// Everything between the conv features and the chosen action of Actor.act (reference agent.py:25-39 with model.py:108-131 behind it), for scalar-valued heads: fc1 runs as
// the usual split-K implicit GEMM (a0_actor_fc1_slabs), but its slabs are consumed directly by ONE kernel that finishes fc1 (slab sum + bias + ReLU), evaluates the q head (A or
// A+1 rows of 512), applies the dueling combine, takes the first maximum and makes the epsilon-greedy draw from the actor's Philox streams.  One wave per environment; replaces
// six launches (reduce, head GEMM, reduce, dueling, select, egreedy) on the actor's critical path.
__global__ __launch_bounds__(256) void a0_actor_qhead_kernel(const float* __restrict__ slabs, long long slab_stride, int nslab, const float* __restrict__ b1,
                                                             const float* __restrict__ W2, const float* __restrict__ b2, int A, int dueling, int E,
                                                             unsigned long long seed, uint32_t stream_a, uint32_t stream_u, unsigned long long off_a,
                                                             unsigned long long off_u, float eps, const long long* __restrict__ ctrl,
                                                             const float* __restrict__ eps_ptr, int* __restrict__ action, float* __restrict__ qmax) {
    __shared__ float raw[4][64];
    extern __shared__ float w2s[];                       // the head's A(+1) rows of 512, staged once per workgroup
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int e = blockIdx.x * 4 + wave;
    const int NQ = A + (dueling ? 1 : 0);
    for (int i = threadIdx.x; i < NQ * 128; i += 256) ((a0_f4*)w2s)[i] = ((const a0_f4*)W2)[i];
    __syncthreads();
    if (e >= E) return;
    if (ctrl) { off_a += (unsigned long long)ctrl[A0_CTRL_RNG_ACTION]; off_u += (unsigned long long)ctrl[A0_CTRL_RNG_UNIFORM]; }
    eps = a0_env_eps(eps, eps_ptr, (uint32_t)__builtin_amdgcn_readfirstlane(e));      // one env per wave
    int act = 0; float best = 0.f;
    a0_qhead_wave(slabs, slab_stride, nslab, b1, w2s, b2, A, dueling, e, lane, raw[wave], seed, stream_a, stream_u, off_a, off_u, eps, act, best);
    if (lane == 0) { action[e] = act; qmax[e] = best; }
}

__global__ __launch_bounds__(512) void a0_actor_qhead_env_kernel(a0_qenv_args P) {
    __shared__ float raw[64];
    __shared__ int s_chase_cell;
    extern __shared__ float w2s[];
    a0_actor_qhead_env_body(P, raw, w2s, &s_chase_cell);
}

// (the fc1's own split count: a0_dense_fwd_partial's at N = 512)
extern "C" long long a0_actor_qhead_scratch(int E, int K) { return (long long)a0_dense_fwd_partial_slabs(E, 512, K) * E * 512; }

extern "C" int a0_actor_qhead_n(const float* feat, int E, int K, int splits, const float* W1, const float* b1, const float* W2, const float* b2, int A, int dueling,
                                float* scratch, unsigned long long seed, unsigned int stream_a, unsigned int stream_u, unsigned long long off_a,
                                unsigned long long off_u, float eps, const long long* ctrl, const float* eps_ptr, int* action, float* qmax, void* stream) {
    A0_TRY
    if (!feat || !W1 || !b1 || !W2 || !b2 || !scratch || !action || !qmax || E < 1 || K < 4 || (K & 3) || A < 1 || A + (dueling ? 1 : 0) > 24)
        return a0_fail(A0_EINVAL, "a0_actor_qhead: bad argument (A + dueling <= 24: the head rows are staged in 48 KB of LDS)");
    if (const int rc = a0_splits_check("a0_actor_qhead_n", splits, K)) return rc;
    if (const int rc = a0_actor_fc1_slabs(feat, K, W1, nullptr, E, splits, scratch, (hipStream_t)stream)) return rc;
    hipLaunchKernelGGL(a0_actor_qhead_kernel, dim3((E + 3) / 4), dim3(256), (size_t)(A + (dueling ? 1 : 0)) * 512 * sizeof(float), (hipStream_t)stream, scratch, (long long)E * 512, splits, b1, W2, b2, A, dueling, E,
                       seed, stream_a, stream_u, off_a, off_u, eps, ctrl, eps_ptr, action, qmax);
    A0_HIP_THROW(hipGetLastError());
    return A0_OK;
    A0_CATCH
}

extern "C" int a0_actor_qhead(const float* feat, int E, int K, const float* W1, const float* b1, const float* W2, const float* b2, int A, int dueling,
                              float* scratch, unsigned long long seed, unsigned int stream_a, unsigned int stream_u, unsigned long long off_a,
                              unsigned long long off_u, float eps, const long long* ctrl, const float* eps_ptr, int* action, float* qmax, void* stream) {
    return a0_actor_qhead_n(feat, E, K, a0_dense_fwd_partial_slabs(E, 512, K), W1, b1, W2, b2, A, dueling, scratch, seed, stream_a, stream_u, off_a, off_u, eps, ctrl, eps_ptr, action,
                            qmax, stream);
}

// a0_actor_qhead + a0_env_synth_step_commit: fc1 GEMM over `feat` (this step's features), then ONE launch per env for tail + env step — with `next`, the launch goes on
// to encode the env's NEW observation (round 5, a0_actor_step_enc2_kernel in encoder_fused.hip) into next->act3_next, which may be `feat` itself: the GEMM has read it
int a0_actor_qhead_env_launch(const float* feat, int E, int K, const float* W1, const float* b1, const float* W2, const float* b2, int A, int dueling, float* scratch,
                              const a0_step_draw& draw, const a0_env_commit& env, const a0_next_enc* next, const unsigned int* w1_planes, hipStream_t st) {
    A0_TRY
    if (!feat || !W1 || !b1 || !W2 || !b2 || !scratch || !draw.action || !draw.qmax || E < 1 || (next ? K != 3136 : (K < 4 || (K & 3))) || A < 1 || A + (dueling ? 1 : 0) > 24)
        return a0_fail(A0_EINVAL, next ? "a0_actor_qhead_env_step_enc: bad argument (4 x 84 x 84 observations, A + dueling <= 24)"
                                       : "a0_actor_qhead_env_step: bad argument (A + dueling <= 24: the head rows are staged in 48 KB of LDS)");
    { const int rc = a0_env_commit_check(env, E, A, next ? "a0_actor_qhead_env_step_enc" : "a0_actor_qhead_env_step"); if (rc != A0_OK) return rc; }
    const int splits = a0_dense_fwd_partial_slabs(E, 512, K);
    { const int rc = a0_actor_fc1_slabs(feat, K, W1, w1_planes, E, splits, scratch, st); if (rc != A0_OK) return rc; }
    a0_qenv_args P;
    P.slabs = scratch; P.slab_stride = (long long)E * 512; P.nslab = splits; P.b1 = b1; P.W2 = W2; P.b2 = b2; P.A = A; P.dueling = dueling; P.E = E;
    a0_step_fill(P, draw, env);
    if (next) return a0_actor_step_enc_launch(P, next->wt, next->w, next->act3_next, st);
    hipLaunchKernelGGL(a0_actor_qhead_env_kernel, dim3(E), dim3(512), (size_t)(A + (dueling ? 1 : 0)) * 512 * sizeof(float), st, P);
    A0_HIP_THROW(hipGetLastError());
    return A0_OK;
    A0_CATCH
}

// (w1_planes: a0_actor_fc1_planes of W1 — fc1 then runs as a0_actor_fc1_kernel where a0_actor_fc1_ok accepts the step; the plain forms pass none)
extern "C" int a0_actor_qhead_env_step_wp(const float* feat, int E, int K, const float* W1, const float* b1, const float* W2, const float* b2, int A, int dueling,
                                       float* scratch, unsigned long long seed, unsigned int stream_a, unsigned int stream_u, unsigned long long off_a,
                                       unsigned long long off_u, float eps, const long long* ctrl, const float* eps_ptr, int* action, float* qmax,
                                       unsigned long long env_seed, unsigned int rank, unsigned int g, const uint8_t* obs_in, uint8_t* obs_out, float* ep_ret,
                                       float* final_mask, float* final_ret, int n, long long steps, double gamma, int* ring_act, float* ring_rew, float* ring_done,
                                       const uint8_t* obs0, uint8_t* frames, long long cap, long long start_slot, int* r_act, float* r_rew, float* r_done, int task, const unsigned int* w1_planes, void* stream) {
    const a0_step_draw draw{seed, stream_a, stream_u, off_a, off_u, eps, ctrl, eps_ptr, action, qmax};
    const a0_env_commit env{env_seed, rank, g, obs_in, obs_out, ep_ret, final_mask, final_ret, n, steps, gamma, ring_act, ring_rew, ring_done, obs0, frames, cap, start_slot, r_act, r_rew, r_done, task};
    return a0_actor_qhead_env_launch(feat, E, K, W1, b1, W2, b2, A, dueling, scratch, draw, env, nullptr, w1_planes, (hipStream_t)stream);
}
extern "C" int a0_actor_qhead_env_step(const float* feat, int E, int K, const float* W1, const float* b1, const float* W2, const float* b2, int A, int dueling,
                                       float* scratch, unsigned long long seed, unsigned int stream_a, unsigned int stream_u, unsigned long long off_a,
                                       unsigned long long off_u, float eps, const long long* ctrl, const float* eps_ptr, int* action, float* qmax,
                                       unsigned long long env_seed, unsigned int rank, unsigned int g, const uint8_t* obs_in, uint8_t* obs_out, float* ep_ret,
                                       float* final_mask, float* final_ret, int n, long long steps, double gamma, int* ring_act, float* ring_rew, float* ring_done,
                                       const uint8_t* obs0, uint8_t* frames, long long cap, long long start_slot, int* r_act, float* r_rew, float* r_done, int task, void* stream) {
    const a0_step_draw draw{seed, stream_a, stream_u, off_a, off_u, eps, ctrl, eps_ptr, action, qmax};
    const a0_env_commit env{env_seed, rank, g, obs_in, obs_out, ep_ret, final_mask, final_ret, n, steps, gamma, ring_act, ring_rew, ring_done, obs0, frames, cap, start_slot, r_act, r_rew, r_done, task};
    return a0_actor_qhead_env_launch(feat, E, K, W1, b1, W2, b2, A, dueling, scratch, draw, env, nullptr, nullptr, (hipStream_t)stream);
}

extern "C" int a0_actor_qhead_env_step_enc_wp(const float* feat, int E, int K, const float* W1, const float* b1, const float* W2, const float* b2, int A, int dueling,
                                           float* scratch, unsigned long long seed, unsigned int stream_a, unsigned int stream_u, unsigned long long off_a,
                                           unsigned long long off_u, float eps, const long long* ctrl, const float* eps_ptr, int* action, float* qmax,
                                           unsigned long long env_seed, unsigned int rank, unsigned int g, const uint8_t* obs_in, uint8_t* obs_out, float* ep_ret,
                                           float* final_mask, float* final_ret, int n, long long steps, double gamma, int* ring_act, float* ring_rew, float* ring_done,
                                           const uint8_t* obs0, uint8_t* frames, long long cap, long long start_slot, int* r_act, float* r_rew, float* r_done, int task,
                                           const float* wt, const a0_encoder_weights* w, float* act3_next, const unsigned int* w1_planes, void* stream) {
    const a0_step_draw draw{seed, stream_a, stream_u, off_a, off_u, eps, ctrl, eps_ptr, action, qmax};
    const a0_env_commit env{env_seed, rank, g, obs_in, obs_out, ep_ret, final_mask, final_ret, n, steps, gamma, ring_act, ring_rew, ring_done, obs0, frames, cap, start_slot, r_act, r_rew, r_done, task};
    const a0_next_enc next{wt, w, act3_next};
    return a0_actor_qhead_env_launch(feat, E, K, W1, b1, W2, b2, A, dueling, scratch, draw, env, &next, w1_planes, (hipStream_t)stream);
}
extern "C" int a0_actor_qhead_env_step_enc(const float* feat, int E, int K, const float* W1, const float* b1, const float* W2, const float* b2, int A, int dueling,
                                           float* scratch, unsigned long long seed, unsigned int stream_a, unsigned int stream_u, unsigned long long off_a,
                                           unsigned long long off_u, float eps, const long long* ctrl, const float* eps_ptr, int* action, float* qmax,
                                           unsigned long long env_seed, unsigned int rank, unsigned int g, const uint8_t* obs_in, uint8_t* obs_out, float* ep_ret,
                                           float* final_mask, float* final_ret, int n, long long steps, double gamma, int* ring_act, float* ring_rew, float* ring_done,
                                           const uint8_t* obs0, uint8_t* frames, long long cap, long long start_slot, int* r_act, float* r_rew, float* r_done, int task,
                                           const float* wt, const a0_encoder_weights* w, float* act3_next, void* stream) {
    const a0_step_draw draw{seed, stream_a, stream_u, off_a, off_u, eps, ctrl, eps_ptr, action, qmax};
    const a0_env_commit env{env_seed, rank, g, obs_in, obs_out, ep_ret, final_mask, final_ret, n, steps, gamma, ring_act, ring_rew, ring_done, obs0, frames, cap, start_slot, r_act, r_rew, r_done, task};
    const a0_next_enc next{wt, w, act3_next};
    return a0_actor_qhead_env_launch(feat, E, K, W1, b1, W2, b2, A, dueling, scratch, draw, env, &next, nullptr, (hipStream_t)stream);
}
