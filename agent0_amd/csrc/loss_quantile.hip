// Quantile-Huber loss (QR / IQN / FQF): target quantiles, the pairwise sweep, stand-alone and — QR — fused with the head tail; forward value and gradient w.r.t.
// the quantiles in one pass; and the Munchausen-IQN targets (a0_miqn_target), which have no reference counterpart.  Restates reference agent0/deepq/agent.py:110-114 (the loss), 273-293 (QRLearner.train_step) and 297-327 (the IQN / FQF targets) with
// the dueling arithmetic of agent0/deepq/model.py:163-177, 180-192.
#include "head_loss.h"
#include "store_policy.h"

// ------------------------------------------------------------------------------------------------ quantile Huber
// y[b][j] = r + gamma_n*(1-d) * qn(b, j, a*_b),  qn(b,j,a) = q_next[b*sb + j*sj + a*sa]
__global__ void a0_quantile_target_kernel(const float* __restrict__ q_next, long long sb, long long sj, long long sa,
                                          const int* __restrict__ a_star, const float* __restrict__ rew, const float* __restrict__ done,
                                          float gamma_n, int B, int Nd, float* __restrict__ y) {
    long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= (long long)B * Nd) return;
    const int b = (int)(i / Nd), j = (int)(i % Nd);
    y[i] = rew[b] + (gamma_n * (1.f - done[b])) * q_next[(long long)b * sb + (long long)j * sj + (long long)a_star[b] * sa];
}

extern "C" int a0_quantile_target(const float* q_next, long long sb, long long sj, long long sa, const int* a_star, const float* rew,
                                  const float* done, float gamma_n, int B, int Nd, float* y, void* stream) {
    if (!q_next || !a_star || !rew || !done || !y || B < 1 || Nd < 1) return a0_fail(A0_EINVAL, "a0_quantile_target: bad argument");
    long long n = (long long)B * Nd;
    hipLaunchKernelGGL(a0_quantile_target_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, (hipStream_t)stream, q_next, sb, sj, sa, a_star, rew, done, gamma_n, B, Nd, y);
    return a0_fail_hip((int)hipGetLastError(), "a0_quantile_target");
}

// ------------------------------------------------------------------------------------------------ Munchausen-IQN targets (learner.iqn.munchausen)
// Vieillard, Pietquin, Geist 2020, section 5 and appendix B; no reference counterpart (the reference has Munchausen targets for its scalar head only).  Per sample b, with
// z'_j(a) = q_next(b, j, a), z_j(a) = q_cur(b, j, a) — the TARGET network on s' and on s at the same N' fractions —, element (b, j, a) at b*sb + j*sj + a*sa:
//   Qm'(a) = (sum_j z'_j(a)) / N',  Qm(a) = (sum_j z_j(a)) / N'                       (each sum taken serially in j order by one lane)
//   lp(x)_a = (x_a - max x) - tau log sum_k exp((x_k - max x) / tau)                   (tau log pi_tau(a): log_softmax_stable at temperature tau)
//   pi'_a   = exp((Qm'_a - max) / tau) / sum_k exp((Qm'_k - max) / tau)                (the softmax at temperature tau, as in the paper; mdqn's is at temperature 1)
//   m       = alpha clamp(lp(Qm)_{a_b}, lo, 0)                                         (alpha is the paper's; mdqn multiplies by tau instead, quirk Q17)
//   y_j     = r + m + gamma_n (1 - d) sum_a pi'_a (z'_j(a) - lp(Qm')_a)
// One wave per sample.  Lane l < 32 owns action l of the next-state values, lane 32 + l action l of the current-state values: its serial sum over j, then — inside
// the wave's 32-lane half, by a five-stage butterfly — the maximum, the sum of exponentials and the log-policy.  pi' and lp(Qm') go to LDS, the taken action's
// log-policy comes from its lane; then lanes stride over j for y_j, the A products added in action order.  No atomics: the bytes are a function of the inputs.
// A sum that is not finite (a NaN or an infinity among the sample's 2 N' A inputs) makes s - s a NaN in its lane; the wave's sum of those joins every y_j of the
// sample, so the quantile Huber kernel behind raises the flag and the update is skipped.  The clamp is two comparisons, not fminf / fmaxf, which would drop a NaN.
// y is read by the next launch alone: written through (store_policy.h), like the GEMMs' slabs.
using a0_miqn_y_store = a0_st_wt;
__global__ __launch_bounds__(64) void a0_miqn_target_kernel(const float* __restrict__ q_next, const float* __restrict__ q_cur, long long sb, long long sj, long long sa,
                                                            const int* __restrict__ act, const float* __restrict__ rew, const float* __restrict__ done, float gamma_n,
                                                            float tau, float alpha, float lo, int Nd, int A, float* __restrict__ y) {
    __shared__ float s_pi[32], s_lp[32];
    const int b = blockIdx.x, lane = threadIdx.x, half = lane >> 5, a = lane & 31;
    const bool on = a < A;
    const int act_b = act[b];
    const float rew_b = rew[b], done_b = done[b];
    const float* qn_b = q_next + (long long)b * sb;
    const float* mine = (half ? q_cur + (long long)b * sb : qn_b) + (long long)(on ? a : 0) * sa;
    float s = 0.f;
#pragma unroll 8
    for (int j = 0; j < Nd; ++j) s += mine[(long long)j * sj];
    const float x = s / (float)Nd;
    const float poison = a0_wave_sum(on ? s - s : 0.f);      // +0, or NaN when an input of the sample is not finite
    float mx = on ? x : -INFINITY;
#pragma unroll
    for (int o = 16; o > 0; o >>= 1) mx = fmaxf(mx, __shfl_xor(mx, o, 64));
    const float z = x - mx;
    const float e = on ? expf(z / tau) : 0.f;
    float se = e;
#pragma unroll
    for (int o = 16; o > 0; o >>= 1) se += __shfl_xor(se, o, 64);
    const float lp = z - tau * logf(se);
    if (!half && on) { s_pi[a] = e / se; s_lp[a] = lp; }
    float bonus = __shfl(lp, 32 + (act_b & 31), 64);
    bonus = bonus < lo ? lo : bonus;
    bonus = bonus > 0.f ? 0.f : bonus;
    const float head = rew_b + alpha * bonus + poison;
    const float g = gamma_n * (1.f - done_b);
    __syncthreads();
    for (int j = lane; j < Nd; j += 64) {
        const float* p = qn_b + (long long)j * sj;
        float acc = 0.f;
        for (int k = 0; k < A; ++k) acc += s_pi[k] * (p[(long long)k * sa] - s_lp[k]);
        a0_put_f32<a0_miqn_y_store>(y + (long long)b * Nd + j, head + g * acc);
    }
}

extern "C" int a0_miqn_target(const float* q_next, const float* q_cur, long long sb, long long sj, long long sa, const int* act, const float* rew, const float* done,
                              float gamma_n, float tau, float alpha, float lo, int B, int Nd, int A, float* y, void* stream) {
    if (!q_next || !q_cur || !act || !rew || !done || !y || B < 1 || Nd < 1 || Nd > 8192 || A < 1 || A > 32)
        return a0_fail(A0_EINVAL, "a0_miqn_target: bad argument (null pointer, or outside B >= 1, 1 <= Nd <= 8192, 1 <= A <= 32)");
    if (!(tau > 0.f) || !(alpha >= 0.f) || !(lo <= 0.f) || !(tau - tau == 0.f) || !(alpha - alpha == 0.f) || !(lo - lo == 0.f))
        return a0_fail(A0_EINVAL, "a0_miqn_target: tau > 0, alpha >= 0 and lo <= 0, all finite");
    hipLaunchKernelGGL(a0_miqn_target_kernel, dim3(B), dim3(64), 0, (hipStream_t)stream, q_next, q_cur, sb, sj, sa, act, rew, done, gamma_n, tau, alpha, lo, Nd, A, y);
    return a0_fail_hip((int)hipGetLastError(), "a0_miqn_target");
}

// One online quantile q_i against the N' targets held in LDS (16-byte aligned), in target order: al = sum_j huber(q_i - T_j) |tau_i - 1{T_j < q_i}| and
// ag = sum_j clamp(q_i - T_j, -1, 1) |tau_i - 1{T_j < q_i}| (reference agent.py:110-114 and its derivative w.r.t. q_i).  Shared by the stand-alone loss kernel and
// by the kernel that runs QRLearner.train_step from the head GEMMs' slabs, so the two cannot differ.  Four targets per LDS read (every lane reads the same address: a
// broadcast).  Eight vector instructions per pair, none of them changing a rounding:
//   * the two values |tau - 1| and |tau - 0| the weight can take are formed once per quantile (kept out of the loop by an empty asm: the compiler would otherwise
//     sink the abs behind the select and pay it per pair);
//   * with c = min(|d|, 1) the Huber value (|d| < 1 ? 0.5 d d : |d| - 0.5) is c * (|d| - 0.5 c): for |d| < 1 the bracket is |d| - 0.5 |d| = 0.5 |d| exactly (an
//     exponent step) and the product |d| * (0.5 |d|) is the same correctly rounded product as (0.5 d) * d; for |d| >= 1 it is 1 * (|d| - 0.5);
//   * both sums advance in one packed fma.
A0_D void a0_qh_sweep(float qi, float tau, const float* __restrict__ s_t, int Nd, float& al, float& ag) {
    float w_lt = fabsf(tau - 1.f), w_ge = fabsf(tau - 0.f);
    asm volatile("" : "+v"(w_lt), "+v"(w_ge));
    float l = 0.f, g = 0.f;
    auto pair = [&](float tj) {
        const float d = qi - tj;
        const float ad = fabsf(d);
        const float c = fminf(ad, 1.f);
        const float h = c * __builtin_fmaf(-0.5f, c, ad);
        const float wq = (tj < qi) ? w_lt : w_ge;
        l += h * wq;
        g += fminf(fmaxf(d, -1.f), 1.f) * wq;
    };
    int j = 0;
    for (; j + 4 <= Nd; j += 4) {
        const a0_f4 t = *(const a0_f4*)(s_t + j);
        pair(t.x); pair(t.y); pair(t.z); pair(t.w);
    }
    for (; j < Nd; ++j) pair(s_t[j]);
    al = l; ag = g;
}

// One workgroup per sample; thread i owns online quantile i and sweeps the N' targets held in LDS, so the
// B x N' x N pairwise tensor of the reference (agent.py:110-114) is never materialised.
// q(b,i,a) = q[b*sb + i*si + a*sa]; taus[b*tb + i] (tb = 0: shared fixed midpoints).
// dq gets w_b/N' * sum_j clamp(q_i - T_j, -1, 1) * |tau_i - 1{T_j < q_i}| at the taken action (dq pre-zeroed by caller).
__global__ __launch_bounds__(256) void a0_quantile_huber_kernel(const float* __restrict__ q, long long sb, long long si, long long sa,
                                                                 const float* __restrict__ y, const float* __restrict__ taus, long long tb,
                                                                 const int* __restrict__ act, const float* __restrict__ wgt,
                                                                 int B, int N, int Nd, float* __restrict__ loss, float* __restrict__ dq,
                                                                 int* __restrict__ nan_flag) {
    extern __shared__ __attribute__((aligned(16))) float s_t[];       // Nd targets
    __shared__ float s_part[4];
    const int b = blockIdx.x, tid = threadIdx.x;
    for (int j = tid; j < Nd; j += blockDim.x) s_t[j] = y[(long long)b * Nd + j];
    __syncthreads();
    const int a = act[b];
    float total = 0.f;
    for (int i = tid; i < N; i += blockDim.x) {
        const long long qi_off = (long long)b * sb + (long long)i * si + (long long)a * sa;
        float al, ag;
        a0_qh_sweep(q[qi_off], taus[(long long)b * tb + i], s_t, Nd, al, ag);
        total += al;
        dq[qi_off] = wgt[b] * ag / (float)Nd;
    }
    total = a0_wave_sum(total);
    if ((tid & 63) == 0) s_part[tid >> 6] = total;
    __syncthreads();
    if (tid == 0) {
        float s = 0.f;
        for (int w = 0; w < (int)(blockDim.x >> 6); ++w) s += s_part[w];
        const float l = s / (float)Nd;
        loss[b] = l;
        if (l != l) atomicOr(nan_flag, 1);
    }
}

extern "C" int a0_loss_quantile_huber(const float* q, long long sb, long long si, long long sa, const float* y, const float* taus,
                                      long long tb, const int* act, const float* wgt, int B, int N, int Nd, float* loss, float* dq,
                                      int* nan_flag, void* stream) {
    if (!q || !y || !taus || !act || !wgt || !loss || !dq || !nan_flag || B < 1 || N < 1 || Nd < 1 || Nd > 8192) return a0_fail(A0_EINVAL, "a0_loss_quantile_huber: bad argument");
    int threads = ((N + 63) / 64) * 64;
    if (threads > 256) threads = 256;
    hipLaunchKernelGGL(a0_quantile_huber_kernel, dim3(B), dim3(threads), (size_t)Nd * sizeof(float), (hipStream_t)stream, q, sb, si, sa, y, taus, tb, act, wgt, B, N, Nd, loss, dq, nan_flag);
    return a0_fail_hip((int)hipGetLastError(), "a0_loss_quantile_huber");
}

// ------------------------------------------------------------------------------------------------ QR: head tail + loss from the head GEMMs' slabs
// QRLearner.train_step (reference agent.py:272-293) from the head GEMMs on, in ONE launch — the quantile-regression counterpart of
// a0_c51_head_loss_slabs_kernel, same slab layout: the online head GEMM over [s ; s'] rows (s' only under double-Q) and the target head GEMM over s' leave their
// split-K slabs; per sample one workgroup of four waves
//   sums them in slab order and adds the bias                                    (== a0_reduce_bias_act_kernel, three times)
//   applies the dueling combine per quantile                                     (== a0_dueling_fwd_kernel, three times; model.py:163-177 through QRHead 180-192)
//   takes the mean over the quantiles and its first maximum                      (== a0_select_action_kernel mode 1; agent.py:277-280)
//   forms the target quantiles r + gamma^n (1 - d) q'(a*)                        (== a0_quantile_target_kernel; agent.py:281-286)
//   sweeps the N x N pairs of the quantile Huber loss                            (== a0_quantile_huber_kernel; agent.py:110-114,288-292)
//   and carries d loss / d q back through the dueling combine                    (== the dq memset + a0_dueling_bwd_kernel)
// — eleven launches of ~5 us of latency each around a 10 us loss kernel — statement for statement the same arithmetic, so the update's numbers do not change.
// The staged head outputs (3 passes x ld floats) and the N targets live in LDS; thread i owns online quantile i (strided when N > 256).
struct a0_qrhl_args : a0_hl_slabs {
    const float* taus;
};
__global__ __launch_bounds__(256) void a0_qr_head_loss_slabs_kernel(a0_qrhl_args P) {
    extern __shared__ __attribute__((aligned(16))) float xq[];     // [3 passes: online(s), target(s'), online(s')][ld], then the T targets (padded to 4)
    __shared__ float s_val[32];
    __shared__ float s_part[4];
    const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int A = P.A, T = P.T, NQ = A + (P.dueling ? 1 : 0), NC = NQ * T, ld = P.ld;
    const float fA = (float)A;
    const int b = blockIdx.x;
    // the sample's scalars are requested before the staging loads
    const int act_b = P.act[b];
    const float rew_b = P.rew[b], done_b = P.done[b], wgt_b = P.wgt[b];
    float* s_y = xq + 3 * ld;
    // staging: 16 bytes per lane and slab over the padded row (the pad columns are summed too and never read); a pass at a time, so that the slab addresses are
    // wave-uniform offsets from one base; all slabs of a piece (at most eight) requested before any is added, additions in slab order
    const int npass = P.sel_off < 0 ? 2 : 3;
    const int ld4 = ld >> 2;
    for (int p = 0; p < npass; ++p) {
        const float* base = (p == 1) ? P.s_tg : P.s_on;
        const long long st4 = ((p == 1) ? P.stride_tg : P.stride_on) >> 2;
        const int ns = (p == 1) ? P.nslab_tg : P.nslab_on;
        const a0_f4* row = (const a0_f4*)(base + (long long)(((p == 2) ? P.sel_off : 0) + b) * ld);
        const a0_f4* bias4 = (const a0_f4*)((p == 1) ? P.bias_tg : P.bias_on);
        for (int c4 = tid; c4 < ld4; c4 += 256) {
            a0_f4 t[8];
#pragma unroll
            for (int zz = 0; zz < 8; ++zz) t[zz] = (zz < ns) ? row[(long long)zz * st4 + c4] : a0_zero4();
            *(a0_f4*)(xq + p * ld + 4 * c4) = a0_slab_sum4(t, ns, bias4 + c4);
        }
    }
    __syncthreads();
    // dueling combine per quantile: thread t owns column t of every action in every pass (it reads back only what it wrote itself)
    for (int t = tid; t < T; t += 256) {
        if (P.dueling)
            for (int p = 0; p < npass; ++p) a0_dueling_combine_col(xq + p * ld, A, fA, T, t);
        if (P.q_on_out) for (int a = 0; a < A; ++a) P.q_on_out[((long long)b * A + a) * T + t] = xq[a * T + t];
        if (P.q_tg_out) for (int a = 0; a < A; ++a) P.q_tg_out[((long long)b * A + a) * T + t] = xq[ld + a * T + t];
    }
    __syncthreads();
    // greedy next action: mean over the quantiles of the selecting network's values, first maximum (a0_select_action_kernel, mode 1: lane-strided partial sums,
    // then the wave's butterfly) — wave w takes actions w, w + 4, ...
    const float* xsel = xq + (P.sel_off < 0 ? 1 : 2) * ld;
    for (int a = wave; a < A; a += 4) {
        const float* p = xsel + a * T;
        float s = 0.f;
        for (int t = lane; t < T; t += 64) s += p[t];
        const float v = a0_wave_sum(s) / (float)T;
        if (lane == 0) s_val[a] = v;
    }
    __syncthreads();
    float best = 0.f;
    int a_star = 0;
    for (int a = 0; a < A; ++a) a0_first_max(a, s_val[a], best, a_star);
    if (P.a_star_out && tid == 0) P.a_star_out[b] = a_star;
    // target quantiles (a0_quantile_target_kernel)
    for (int j = tid; j < T; j += 256) s_y[j] = rew_b + (P.gamma_n * (1.f - done_b)) * xq[ld + a_star * T + j];
    __syncthreads();
    // the pairwise sweep (a0_quantile_huber_kernel) and, with each quantile's gradient at hand, its way back through the dueling combine (a0_dueling_bwd_kernel on a dq
    // that is zero outside the taken action) straight into the head GEMM's output gradient
    float* o = P.draw + (long long)b * ld;
    float tot = 0.f;
    for (int i = tid; i < T; i += 256) {
        float al, ag;
        a0_qh_sweep(xq[act_b * T + i], P.taus[i], s_y, T, al, ag);
        tot += al;
        const float g = wgt_b * ag / (float)T;
        float sdl = 0.f;
        for (int k = 0; k < A; ++k) sdl += (k == act_b) ? g : 0.f;
        for (int k = 0; k < A; ++k) {
            float out = (k == act_b) ? g : 0.f;
            if (P.dueling) out -= sdl / (float)A;
            o[k * T + i] = out;
        }
        if (P.dueling) o[A * T + i] = sdl;
    }
    for (int c = NC + tid; c < ld; c += 256) o[c] = 0.f;
    tot = a0_wave_sum(tot);
    if (lane == 0) s_part[wave] = tot;
    __syncthreads();
    if (tid == 0) {
        float s = 0.f;
        for (int w = 0; w < 4; ++w) s += s_part[w];
        const float l = s / (float)T;
        P.loss[b] = l;
        if (l != l) atomicOr(P.nan_flag, 1);
    }
}

extern "C" int a0_qr_head_loss_slabs(const float* slabs_on, long long stride_on, int nslab_on, int rows_on, const float* slabs_tg, long long stride_tg, int nslab_tg,
                                     int sel_off, const float* bias_on, const float* bias_tg, int ld, int A, int T, int dueling, const int* act, const float* rew,
                                     const float* done, const float* wgt, const float* taus, float gamma_n, int B, float* loss, float* draw, float* q_on_out,
                                     float* q_tg_out, int* a_star_out, int* nan_flag, void* stream) {
    const size_t lds = ((size_t)3 * ld + (size_t)((T + 3) / 4 * 4)) * sizeof(float);
    a0_qrhl_args P;
    if (int rc = a0_hl_slabs_fill(P, "a0_qr_head_loss_slabs", taus && A <= 32 && T >= 1 && nslab_on <= 8 && nslab_tg <= 8, "A <= 32; at most 8 slabs per head", lds, slabs_on,
                                  stride_on, nslab_on, rows_on, slabs_tg, stride_tg, nslab_tg, sel_off, bias_on, bias_tg, ld, A, T, dueling, act, rew, done, wgt, gamma_n, B,
                                  loss, draw, q_on_out, q_tg_out, a_star_out, nan_flag))
        return rc;
    if (!a0_grant_dynamic_lds<a0_qr_head_loss_slabs_kernel>(lds)) return a0_fail(A0_EINVAL, "a0_qr_head_loss_slabs: LDS");
    P.taus = taus;
    hipLaunchKernelGGL(a0_qr_head_loss_slabs_kernel, dim3(B), dim3(256), lds, (hipStream_t)stream, P);
    return a0_fail_hip((int)hipGetLastError(), "a0_qr_head_loss_slabs");
}
