// What every head family shares: the dueling combine and its backward, and greedy-action selection.  The TD losses live by family in loss_value.hip (scalar
// heads: DQN, Munchausen DQN), loss_c51.hip and loss_quantile.hip (QR / IQN / FQF); head_loss.h holds the pieces those share.
// Restates the dueling / qval arithmetic of reference agent0/deepq/model.py:123-131, 163-177, 190-192, 219-233, 253-257, 280-284.
#include "head_loss.h"

// ------------------------------------------------------------------------------------------------ dueling combine
// raw [R][ld]: columns [0, A*T) advantage / plain q (action-major), [A*T, A*T+T) value stream when dueling.
__global__ void a0_dueling_fwd_kernel(const float* __restrict__ raw, int ld, float* __restrict__ q, int R, int A, int T, int dueling) {
    long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= (long long)R * T) return;
    const int r = (int)(i / T), t = (int)(i % T);
    const float* x = raw + (long long)r * ld;
    float* o = q + (long long)r * A * T;
    if (!dueling) {
        for (int a = 0; a < A; ++a) o[a * T + t] = x[a * T + t];
        return;
    }
    float s = 0.f;
    for (int a = 0; a < A; ++a) s += x[a * T + t];
    const float mean = s / (float)A;
    const float v = x[A * T + t];
    for (int a = 0; a < A; ++a) o[a * T + t] = v + (x[a * T + t] - mean);
}

__global__ void a0_dueling_bwd_kernel(const float* __restrict__ dq, float* __restrict__ draw, int ld, int R, int A, int T, int dueling) {
    long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= (long long)R * ld) return;
    const int r = (int)(i / ld), c = (int)(i % ld);
    const float* g = dq + (long long)r * A * T;
    float out = 0.f;
    if (c < A * T) {
        out = g[c];
        if (dueling) {
            const int t = c % T;
            float s = 0.f;
            for (int a = 0; a < A; ++a) s += g[a * T + t];
            out -= s / (float)A;
        }
    } else if (dueling && c < A * T + T) {
        const int t = c - A * T;
        float s = 0.f;
        for (int a = 0; a < A; ++a) s += g[a * T + t];
        out = s;
    }
    draw[i] = out;
}

extern "C" int a0_dueling_fwd(const float* raw, int ld, float* q, int R, int A, int T, int dueling, void* stream) {
    if (!raw || !q || R < 1 || A < 1 || T < 1 || ld < A * T + (dueling ? T : 0)) return a0_fail(A0_EINVAL, "a0_dueling_fwd: bad argument");
    long long n = (long long)R * T;
    hipLaunchKernelGGL(a0_dueling_fwd_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, (hipStream_t)stream, raw, ld, q, R, A, T, dueling);
    return a0_fail_hip((int)hipGetLastError(), "a0_dueling_fwd");
}

extern "C" int a0_dueling_bwd(const float* dq, float* draw, int ld, int R, int A, int T, int dueling, void* stream) {
    if (!dq || !draw || R < 1 || A < 1 || T < 1 || ld < A * T + (dueling ? T : 0)) return a0_fail(A0_EINVAL, "a0_dueling_bwd: bad argument");
    long long n = (long long)R * ld;
    hipLaunchKernelGGL(a0_dueling_bwd_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, (hipStream_t)stream, dq, draw, ld, R, A, T, dueling);
    return a0_fail_hip((int)hipGetLastError(), "a0_dueling_bwd");
}

// ------------------------------------------------------------------------------------------------ action values + argmax
// One wave per sample.  x(b,a,t) = x[b*sb + a*sa + t*st].  mode: 0 identity (T=1), 1 mean over t (QR atoms / IQN taus),
// 2 C51 expectation sum_t softmax_t * atoms[t], 3 FQF sum_t (tau[b][t+1]-tau[b][t]) * x.
__global__ __launch_bounds__(64) void a0_select_action_kernel(const float* __restrict__ x, long long sb, long long sa, long long st,
                                                               int B, int A, int T, int mode, const float* __restrict__ aux,
                                                               int* __restrict__ a_star, float* __restrict__ qsel, float* __restrict__ qmax) {
    const int b = blockIdx.x, lane = threadIdx.x;
    if (b >= B) return;
    float best = 0.f;
    int besta = 0;
    for (int a = 0; a < A; ++a) {
        const float* p = x + (long long)b * sb + (long long)a * sa;
        float v;
        if (mode == 0) {
            v = p[0];
        } else if (mode == 1) {
            float s = 0.f;
            for (int t = lane; t < T; t += 64) s += p[(long long)t * st];
            v = a0_wave_sum(s) / (float)T;
        } else if (mode == 2) {
            float mx = -INFINITY;
            for (int t = lane; t < T; t += 64) mx = fmaxf(mx, p[(long long)t * st]);
            mx = a0_wave_max(mx);
            float se = 0.f, sz = 0.f;
            for (int t = lane; t < T; t += 64) {
                float e = expf(p[(long long)t * st] - mx);
                se += e;
                sz += e * aux[t];
            }
            se = a0_wave_sum(se);
            sz = a0_wave_sum(sz);
            v = sz / se;
        } else {
            const float* tau = aux + (long long)b * (T + 1);
            float s = 0.f;
            for (int t = lane; t < T; t += 64) s += (tau[t + 1] - tau[t]) * p[(long long)t * st];
            v = a0_wave_sum(s);
        }
        if (qsel && lane == 0) qsel[(long long)b * A + a] = v;
        a0_first_max(a, v, best, besta);
    }
    if (lane == 0) {
        if (a_star) a_star[b] = besta;
        if (qmax) qmax[b] = best;
    }
}

extern "C" int a0_select_action(const float* x, long long sb, long long sa, long long st, int B, int A, int T, int mode,
                                const float* aux, int* a_star, float* qsel, float* qmax, void* stream) {
    if (!x || B < 1 || A < 1 || T < 1 || mode < 0 || mode > 3 || ((mode == 2 || mode == 3) && !aux)) return a0_fail(A0_EINVAL, "a0_select_action: bad argument");
    hipLaunchKernelGGL(a0_select_action_kernel, dim3(B), dim3(64), 0, (hipStream_t)stream, x, sb, sa, st, B, A, T, mode, aux, a_star, qsel, qmax);
    return a0_fail_hip((int)hipGetLastError(), "a0_select_action");
}
