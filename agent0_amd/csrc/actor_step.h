// What one merged actor step (tail + synthetic env step in ONE launch) carries besides its head, as two host descriptors, with the one copy of their argument
// check and of their way into the kernels' argument structs.  Host code only: the exported entry points (include/agent0_hip.h) keep their flat argument lists and
// pack these; a0_actor_rollout (runtime.hip) fills them once per step.  A new per-step field goes into the descriptor, a0_step_fill and the exported wrappers.
#pragma once
#include "a0_internal.h"

#include <cstdint>
#include <string>

// the epsilon-greedy draw: the actor's Philox streams and where the action and max_a q go
struct a0_step_draw {
    unsigned long long seed; unsigned int stream_a, stream_u; unsigned long long off_a, off_u; float eps; const long long* ctrl; const float* eps_ptr;
    int* action; float* qmax;
};
// the env step, the n-step bookkeeping and the replay row (a0_env_synth_step_commit's arguments)
struct a0_env_commit {
    unsigned long long env_seed; unsigned int rank, g; const uint8_t* obs_in; uint8_t* obs_out; float *ep_ret, *final_mask, *final_ret;
    int n; long long steps; double gamma; int* ring_act; float *ring_rew, *ring_done; const uint8_t* obs0; uint8_t* frames; long long cap, start_slot;
    int* r_act; float *r_rew, *r_done; int task;
};
// where a step's kernel goes on to encode the env's new observation (encoder_fused.hip): the NEXT step's features into act3_next [E][3136]
struct a0_next_enc { const float* wt; const a0_encoder_weights* w; float* act3_next; };
// the head GEMM's split-K slabs for the distributional (kt = 0: c51 mode 2 with atoms, qr mode 1) and quantile (kt = 1: iqn mode 1, fqf mode 3 with taus) tails
struct a0_slab_head {
    const float* slabs; long long slab_stride; int nslab; const float* bias; int ld, A, T, dueling, mode; const float *atoms, *taus; int kt;
};

// A0_OK, or A0_EINVAL behind a message that starts with `who`: null / range / task tests, then the 16-byte alignment of the observation buffers
inline int a0_env_commit_check(const a0_env_commit& c, int E, int A, const char* who) {
    if (!c.obs_in || !c.obs_out || c.obs_in == c.obs_out || !c.ep_ret || !c.final_mask || !c.final_ret || !c.ring_act || !c.ring_rew || !c.ring_done || !c.obs0 || !c.frames ||
        !c.r_act || !c.r_rew || !c.r_done || c.n < 1 || c.steps < 0 || c.cap < E || c.start_slot < 0 || c.task < A0_ENV_TASK_STREAM || c.task > A0_ENV_TASK_CHASE ||
        (c.task == A0_ENV_TASK_CHASE && A < 4))
        return a0_fail(A0_EINVAL, (std::string(who) + ": bad env argument (obs_in and obs_out must differ; the chase task needs at least four actions)").c_str());
    if ((((uintptr_t)c.obs_in) | ((uintptr_t)c.obs_out) | ((uintptr_t)c.obs0) | ((uintptr_t)c.frames)) & 15)
        return a0_fail(A0_EINVAL, (std::string(who) + ": buffers must be 16-byte aligned").c_str());
    return A0_OK;
}

// Args: a0_qenv_args or a0_dtenv_args (actor_tail.h), which name these fields alike
template <class Args>
inline void a0_step_fill(Args& P, const a0_step_draw& d, const a0_env_commit& c) {
    P.rng_seed = d.seed; P.stream_a = d.stream_a; P.stream_u = d.stream_u; P.off_a = d.off_a; P.off_u = d.off_u; P.eps = d.eps; P.ctrl = d.ctrl; P.eps_ptr = d.eps_ptr;
    P.action = d.action; P.qmax = d.qmax;
    P.env_seed = c.env_seed; P.rank = c.rank; P.g = c.g; P.obs_in = c.obs_in; P.obs_out = c.obs_out; P.ep_ret = c.ep_ret; P.final_mask = c.final_mask; P.final_ret = c.final_ret;
    P.n = c.n; P.steps = c.steps; P.gamma = c.gamma; P.ring_act = c.ring_act; P.ring_rew = c.ring_rew; P.ring_done = c.ring_done; P.obs0 = c.obs0; P.frames = c.frames;
    P.cap = c.cap; P.start = c.start_slot % c.cap; P.r_act = c.r_act; P.r_rew = c.r_rew; P.r_done = c.r_done; P.task = c.task;
}
