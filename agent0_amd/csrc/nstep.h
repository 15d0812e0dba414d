// The n-step window of ONE env at one step (agent.py:57-73): shared by a0_nstep_kernel (actor.hip) and the host-step ingest kernel (host_step.hip), so that
// both emit the same bits.
//   done_t = (terminal | life_loss) & ~truncated                      agent.py:57-62
//   R = 0; D = 0; for k = newest .. oldest: D |= d_k; R = R*gamma*(1-d_k) + r_k      agent.py:64-69, in fp64, rounded to fp32 once
//   emitted action = action of the oldest entry                       agent.py:70-71
// steps = number of env steps taken BEFORE this one (so this step is written at steps % n).  The emitted transition goes to *o_act / *o_rew / *o_done.
#pragma once
#include "a0_defs.h"

A0_D void a0_nstep_env(int e, int E, int n, long long steps, double gamma, int a_now, float reward, float terminal, float truncated, float life_loss,
                       int* __restrict__ ring_act, float* __restrict__ ring_rew, float* __restrict__ ring_done, int* __restrict__ o_act, float* __restrict__ o_rew,
                       float* __restrict__ o_done) {
#pragma clang fp contract(off)
    const bool done = ((terminal != 0.f) || (life_loss != 0.f)) && !(truncated != 0.f);
    const int cur = (int)(steps % n);
    ring_act[(long long)cur * E + e] = a_now;
    ring_rew[(long long)cur * E + e] = reward;
    ring_done[(long long)cur * E + e] = done ? 1.f : 0.f;
    const long long have = steps + 1;
    const int count = have < n ? (int)have : n;
    double R = 0.0;
    bool D = false;
    for (int k = 0; k < count; ++k) {
        const int idx = (int)(((steps - k) % n + n) % n);
        const float dk = (k == 0) ? (done ? 1.f : 0.f) : ring_done[(long long)idx * E + e];
        const float rk = (k == 0) ? reward : ring_rew[(long long)idx * E + e];
        D = D || (dk != 0.f);
        R = R * gamma * (double)(1 - (dk != 0.f ? 1 : 0)) + (double)rk;
    }
    const int oldest = (int)(((steps - (count - 1)) % n + n) % n);
    *o_act = (count == 1) ? a_now : ring_act[(long long)oldest * E + e];
    *o_rew = (float)R;
    *o_done = D ? 1.f : 0.f;
}
