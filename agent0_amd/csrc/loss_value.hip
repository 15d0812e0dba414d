// TD losses of the scalar heads: DQN smooth-L1 and Munchausen DQN, stand-alone and fused with the heads — forward value and gradient w.r.t. the head output in one
// pass.  Restates reference agent0/deepq/agent.py:173-190 (DQNLearner.train_step) and 193-215 (MDQNLearner.train_step, log_softmax_stable 116-119) with the q head
// and dueling arithmetic of agent0/deepq/model.py:108-131 behind them.
#include "head_loss.h"

// ------------------------------------------------------------------------------------------------ DQN
// loss[b] = smooth_l1(q[b][a_b] - y_b), y_b = r + gamma_n*(1-d)*q_next[b][a*_b];  dq = w * clamp(q - y, -1, 1) at a_b.
__global__ void a0_dqn_loss_kernel(const float* __restrict__ q, const float* __restrict__ q_next, int A, const int* __restrict__ act,
                                   const int* __restrict__ a_star, const float* __restrict__ rew, const float* __restrict__ done,
                                   const float* __restrict__ wgt, float gamma_n, int B, float* __restrict__ loss, float* __restrict__ dq,
                                   int* __restrict__ nan_flag) {
    const int b = blockIdx.x * blockDim.x + threadIdx.x;
    if (b >= B) return;
    const float qn = q_next[(long long)b * A + a_star[b]];
    const float y = rew[b] + (gamma_n * (1.f - done[b])) * qn;
    const int a = act[b];
    const float g = a0_td_tail(q[(long long)b * A + a] - y, wgt[b], loss + b, nan_flag);
    for (int k = 0; k < A; ++k) dq[(long long)b * A + k] = (k == a) ? g : 0.f;
}

extern "C" int a0_loss_dqn(const float* q, const float* q_next, int A, const int* act, const int* a_star, const float* rew,
                           const float* done, const float* wgt, float gamma_n, int B, float* loss, float* dq, int* nan_flag, void* stream) {
    if (!q || !q_next || !act || !a_star || !rew || !done || !wgt || !loss || !dq || !nan_flag || B < 1 || A < 1) return a0_fail(A0_EINVAL, "a0_loss_dqn: bad argument");
    hipLaunchKernelGGL(a0_dqn_loss_kernel, dim3((B + 127) / 128), dim3(128), 0, (hipStream_t)stream, q, q_next, A, act, a_star, rew, done, wgt, gamma_n, B, loss, dq, nan_flag);
    return a0_fail_hip((int)hipGetLastError(), "a0_loss_dqn");
}

// ------------------------------------------------------------------------------------------------ Munchausen DQN
// MDQNLearner.train_step (reference agent.py:194-215, log_softmax_stable 116-119), per sample:
//   lp(x)  = z - tau * logsumexp(z / tau),  z = x - max(x)
//   v_next = sum_a softmax(q')_a * (q'_a - lp(q')_a)            (softmax at temperature 1, as the reference has it)
//   y      = r + tau * clamp(lp(q_tgt(obs))[a], lo, 0) + gamma_n * (1 - d) * v_next        (alpha is unused in the reference, Q17)
template <class QN, class QC>
A0_D float a0_mdqn_target(QN qn, QC qc, int A, int a, float rew, float done, float gamma_n, float tau, float lo) {
    float mx = qn(0), mc = qc(0);
    for (int k = 1; k < A; ++k) { mx = fmaxf(mx, qn(k)); mc = fmaxf(mc, qc(k)); }
    float se_t = 0.f, se_1 = 0.f, sc_t = 0.f;
    for (int k = 0; k < A; ++k) { se_t += expf((qn(k) - mx) / tau); se_1 += expf(qn(k) - mx); sc_t += expf((qc(k) - mc) / tau); }
    const float lse_t = logf(se_t), lsc_t = logf(sc_t);
    float v_next = 0.f;
    for (int k = 0; k < A; ++k) {
        const float lp = (qn(k) - mx) - tau * lse_t;
        v_next += (expf(qn(k) - mx) / se_1) * (qn(k) - lp);
    }
    float add_on = (qc(a) - mc) - tau * lsc_t;
    add_on = fminf(fmaxf(add_on, lo), 0.f);
    return rew + tau * add_on + (gamma_n * (1.f - done)) * v_next;
}

__global__ void a0_mdqn_loss_kernel(const float* __restrict__ q, const float* __restrict__ q_next, const float* __restrict__ q_cur_tgt, int A,
                                    const int* __restrict__ act, const float* __restrict__ rew, const float* __restrict__ done, const float* __restrict__ wgt,
                                    float gamma_n, float tau, float lo, int B, float* __restrict__ loss, float* __restrict__ dq, int* __restrict__ nan_flag) {
    const int b = blockIdx.x * blockDim.x + threadIdx.x;
    if (b >= B) return;
    const float* qn = q_next + (long long)b * A;
    const float* qc = q_cur_tgt + (long long)b * A;
    const int a = act[b];
    const float y = a0_mdqn_target([&](int k) { return qn[k]; }, [&](int k) { return qc[k]; }, A, a, rew[b], done[b], gamma_n, tau, lo);
    const float g = a0_td_tail(q[(long long)b * A + a] - y, wgt[b], loss + b, nan_flag);
    for (int k = 0; k < A; ++k) dq[(long long)b * A + k] = (k == a) ? g : 0.f;
}

extern "C" int a0_loss_mdqn(const float* q, const float* q_next, const float* q_cur_tgt, int A, const int* act, const float* rew, const float* done,
                            const float* wgt, float gamma_n, float tau, float lo, int B, float* loss, float* dq, int* nan_flag, void* stream) {
    if (!q || !q_next || !q_cur_tgt || !act || !rew || !done || !wgt || !loss || !dq || !nan_flag || B < 1 || A < 1 || !(tau > 0.f)) return a0_fail(A0_EINVAL, "a0_loss_mdqn: bad argument");
    hipLaunchKernelGGL(a0_mdqn_loss_kernel, dim3((B + 127) / 128), dim3(128), 0, (hipStream_t)stream, q, q_next, q_cur_tgt, A, act, rew, done, wgt, gamma_n, tau, lo, B, loss, dq, nan_flag);
    return a0_fail_hip((int)hipGetLastError(), "a0_loss_mdqn");
}

// ------------------------------------------------------------------------------------------------ DQN: heads + loss + head gradient
// Everything between the fc1 activations and the gradient w.r.t. the raw head outputs of DQNLearner.train_step (reference
// agent.py:173-190 with model.py:108-131 behind it) in one kernel, one wave per sample: q head of the online net on h(s), of the
// target net on h'(s') and — double-Q — of the online net on h(s'); dueling combine; first-max argmax; smooth-L1 against
// y = r + gamma^n (1-d) q'(s', a*); dq; dueling backward into draw [B][ld].  Replaces nine launches (2 x (GEMM, reduce, dueling),
// select, loss, dueling backward) that together move a few hundred kilobytes.
__global__ __launch_bounds__(256) void a0_dqn_head_loss_kernel(const float* __restrict__ h_on, const float* __restrict__ h_tg, const float* __restrict__ h_sel,
                                                               const float* __restrict__ W_on, const float* __restrict__ b_on, const float* __restrict__ W_tg,
                                                               const float* __restrict__ b_tg, int A, int dueling, int ld, const int* __restrict__ act,
                                                               const float* __restrict__ rew, const float* __restrict__ done, const float* __restrict__ wgt,
                                                               float gamma_n, int B, float* __restrict__ loss, float* __restrict__ q_on_out,
                                                               float* __restrict__ q_tg_out, float* __restrict__ draw, int* __restrict__ nan_flag) {
    extern __shared__ float wsm[];                 // [online rows | target rows], NQ x 512 each
    __shared__ float raw[4][3][32];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int NQ = A + (dueling ? 1 : 0);
    for (int i = threadIdx.x; i < NQ * 128; i += 256) { ((a0_f4*)wsm)[i] = ((const a0_f4*)W_on)[i]; ((a0_f4*)wsm)[NQ * 128 + i] = ((const a0_f4*)W_tg)[i]; }
    const int b = blockIdx.x * 4 + wave;
    const int br = b < B ? b : B - 1;
    float ho[8], ht[8], hs[8];
#pragma unroll
    for (int i = 0; i < 8; ++i) {
        ho[i] = h_on[(long long)br * 512 + lane + 64 * i];
        ht[i] = h_tg[(long long)br * 512 + lane + 64 * i];
        hs[i] = h_sel ? h_sel[(long long)br * 512 + lane + 64 * i] : 0.f;
    }
    __syncthreads();
    if (b >= B) return;
    for (int a = 0; a < NQ; ++a) {
        const float* wo = wsm + a * 512;
        const float* wt = wsm + (NQ + a) * 512;
        float so = 0.f, st = 0.f, ss = 0.f;
#pragma unroll
        for (int i = 0; i < 8; ++i) {
            const float w1 = wo[lane + 64 * i];
            so = fmaf(ho[i], w1, so);
            ss = fmaf(hs[i], w1, ss);
            st = fmaf(ht[i], wt[lane + 64 * i], st);
        }
        so = a0_wave_sum(so); st = a0_wave_sum(st); ss = a0_wave_sum(ss);
        if (lane == 0) { raw[wave][0][a] = so + b_on[a]; raw[wave][1][a] = st + b_tg[a]; raw[wave][2][a] = ss + b_on[a]; }
    }
    if (lane != 0) return;
    // lane 0's tail: dueling means, q of each pass, the first maximum of the selecting pass, the q outputs, the target, the TD tail, the dueling backward into draw
    const int nsel = h_sel ? 2 : 1;
    float mean[3] = {0.f, 0.f, 0.f}, v[3] = {0.f, 0.f, 0.f};
    if (dueling)
        for (int s3 = 0; s3 < 3; ++s3) {
            float t = 0.f;
            for (int a = 0; a < A; ++a) t += raw[wave][s3][a];
            mean[s3] = t / (float)A;
            v[s3] = raw[wave][s3][A];
        }
    auto q = [&](int s3, int a) { return dueling ? v[s3] + (raw[wave][s3][a] - mean[s3]) : raw[wave][s3][a]; };
    float best = 0.f;
    int a_star = 0;
    for (int a = 0; a < A; ++a) {
        a0_first_max(a, q(nsel, a), best, a_star);
        q_on_out[(long long)b * A + a] = q(0, a);
        if (q_tg_out) q_tg_out[(long long)b * A + a] = q(1, a);
    }
    const float qn = q(1, a_star);
    const float y = rew[b] + (gamma_n * (1.f - done[b])) * qn;
    const int ab = act[b];
    const float g = a0_td_tail(q(0, ab) - y, wgt[b], loss + b, nan_flag);
    a0_onehot_dueling_bwd(draw + (long long)b * ld, A, dueling, ld, ab, g, nullptr);
}

extern "C" int a0_dqn_head_loss(const float* h_on, const float* h_tg, const float* h_sel, const float* W_on, const float* b_on, const float* W_tg,
                                const float* b_tg, int A, int dueling, int ld, const int* act, const float* rew, const float* done, const float* wgt,
                                float gamma_n, int B, float* loss, float* q_on_out, float* q_tg_out, float* draw, int* nan_flag, void* stream) {
    const int NQ = A + (dueling ? 1 : 0);
    if (!h_on || !h_tg || !W_on || !b_on || !W_tg || !b_tg || !act || !rew || !done || !wgt || !loss || !q_on_out || !draw || !nan_flag || B < 1 || A < 1 || NQ > 24 ||
        ld < NQ)
        return a0_fail(A0_EINVAL, "a0_dqn_head_loss: bad argument (A + dueling <= 24)");
    const size_t lds = (size_t)2 * NQ * 512 * sizeof(float);
    if (!a0_grant_dynamic_lds<a0_dqn_head_loss_kernel>(lds)) return a0_fail(A0_EINVAL, "a0_dqn_head_loss: LDS");
    hipLaunchKernelGGL(a0_dqn_head_loss_kernel, dim3((B + 3) / 4), dim3(256), lds, (hipStream_t)stream, h_on, h_tg, h_sel, W_on, b_on, W_tg, b_tg, A, dueling, ld, act,
                       rew, done, wgt, gamma_n, B, loss, q_on_out, q_tg_out, draw, nan_flag);
    return a0_fail_hip((int)hipGetLastError(), "a0_dqn_head_loss");
}

// Variant that also finishes fc1: the three fc1 GEMMs (online on s, target on s', online on s' for double-Q) leave their split-K slabs
// behind (a0_dense_fwd_partial) and this kernel sums them in slab order, adds the bias and applies the ReLU exactly like
// a0_reduce_bias_act_kernel would (bit-identical), writing only the online activations h(s) that the backward pass needs.  Two or three
// reduction launches per update disappear.
// MDQN = true: MDQNLearner.train_step (agent.py:193-215) through the same kernel — the third pass is the TARGET network on the current observation
// (its fc1 bias and head rows are the target's), and the loss is the Munchausen one (a0_mdqn_target, shared with a0_mdqn_loss_kernel); q_sel_out receives it.
struct a0_mdqn_par { float tau, lo; float* q_sel_out; };
template <bool MDQN>
__global__ __launch_bounds__(256) void a0_dqn_head_loss_slabs_kernel(const float* __restrict__ s_on, const float* __restrict__ s_tg, const float* __restrict__ s_sel,
                                                                     long long slab_stride, int nslab, const float* __restrict__ b1_on,
                                                                     const float* __restrict__ b1_tg, float* __restrict__ h_on_out,
                                                                     const float* __restrict__ W_on, const float* __restrict__ b_on, const float* __restrict__ W_tg,
                                                                     const float* __restrict__ b_tg, int A, int dueling, int ld, const int* __restrict__ act,
                                                                     const float* __restrict__ rew, const float* __restrict__ done, const float* __restrict__ wgt,
                                                                     float gamma_n, int B, float* __restrict__ loss, float* __restrict__ q_on_out,
                                                                     float* __restrict__ q_tg_out, float* __restrict__ draw, int* __restrict__ nan_flag,
                                                                     float* __restrict__ dh_out, a0_mdqn_par M) {
    extern __shared__ float wsm[];                 // [online rows | target rows], NQ x 512 each
    __shared__ float raw[4][3][32];
    __shared__ float dsh[4][32];                   // this row's head gradient (draw), for the fused head data gradient
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int NQ = A + (dueling ? 1 : 0);
    const int b = blockIdx.x * 4 + wave;
    const int br = b < B ? b : B - 1;
    // everything the tail of the kernel reads is requested here, in front of the slab loads, so that no load waits behind the head reductions: the sample's scalars
    // (every lane holds them; lane 0 uses them), the head biases (lane a holds row a's) and fc1's bias columns
    const int ab = act[br];
    const float rew_b = rew[br], done_b = done[br], wgt_b = wgt[br];
    const float hb_on = lane < NQ ? b_on[lane] : 0.f, hb_tg = lane < NQ ? b_tg[lane] : 0.f;
    float b1o[8], b1t[8];
#pragma unroll
    for (int i = 0; i < 8; ++i) { b1o[i] = b1_on[lane + 64 * i]; b1t[i] = b1_tg[lane + 64 * i]; }
    float ho[8], ht[8], hs[8];
#pragma unroll
    for (int i = 0; i < 8; ++i) { ho[i] = 0.f; ht[i] = 0.f; hs[i] = 0.f; }
    const long long ro = (long long)br * 512 + lane;
    // four slabs per trip: every column of the trip is requested before any is added, so 64 (96) loads overlap instead of queueing;
    // the additions stay in slab order
    auto sum4 = [&](const float* __restrict__ sp, float (&h)[8], int z) {
        for (; z + 4 <= nslab; z += 4) {
            float t[4][8];
#pragma unroll
            for (int zz = 0; zz < 4; ++zz)
#pragma unroll
                for (int i = 0; i < 8; ++i) t[zz][i] = sp[(long long)(z + zz) * slab_stride + ro + 64 * i];
#pragma unroll
            for (int zz = 0; zz < 4; ++zz)
#pragma unroll
                for (int i = 0; i < 8; ++i) h[i] += t[zz][i];
        }
        for (; z < nslab; ++z) {
            float t[8];
#pragma unroll
            for (int i = 0; i < 8; ++i) t[i] = sp[(long long)z * slab_stride + ro + 64 * i];
#pragma unroll
            for (int i = 0; i < 8; ++i) h[i] += t[i];
        }
    };
    // the first four slabs of all three passes are requested together, then the head weights are staged while they are in flight
    const int z0 = nslab >= 4 ? 4 : 0;
    float t_on[4][8], t_tg[4][8], t_sel[4][8];
    if (z0) {
#pragma unroll
        for (int zz = 0; zz < 4; ++zz)
#pragma unroll
            for (int i = 0; i < 8; ++i) {
                t_on[zz][i] = s_on[(long long)zz * slab_stride + ro + 64 * i];
                t_tg[zz][i] = s_tg[(long long)zz * slab_stride + ro + 64 * i];
            }
        if (s_sel) {
#pragma unroll
            for (int zz = 0; zz < 4; ++zz)
#pragma unroll
                for (int i = 0; i < 8; ++i) t_sel[zz][i] = s_sel[(long long)zz * slab_stride + ro + 64 * i];
        }
    }
    for (int i = threadIdx.x; i < NQ * 128; i += 256) { ((a0_f4*)wsm)[i] = ((const a0_f4*)W_on)[i]; ((a0_f4*)wsm)[NQ * 128 + i] = ((const a0_f4*)W_tg)[i]; }
    if (z0) {
#pragma unroll
        for (int zz = 0; zz < 4; ++zz)
#pragma unroll
            for (int i = 0; i < 8; ++i) { ho[i] += t_on[zz][i]; ht[i] += t_tg[zz][i]; }
        if (s_sel) {
#pragma unroll
            for (int zz = 0; zz < 4; ++zz)
#pragma unroll
                for (int i = 0; i < 8; ++i) hs[i] += t_sel[zz][i];
        }
    }
    sum4(s_on, ho, z0);
    sum4(s_tg, ht, z0);
    if (s_sel) sum4(s_sel, hs, z0);
#pragma unroll
    for (int i = 0; i < 8; ++i) {
        const float bo = b1o[i], bt = b1t[i];
        float v = ho[i] + bo; ho[i] = v < 0.f ? 0.f : v;
        v = ht[i] + bt; ht[i] = v < 0.f ? 0.f : v;
        v = hs[i] + (MDQN ? bt : bo); hs[i] = v < 0.f ? 0.f : v;
    }
    __syncthreads();
    if (b >= B) return;
#pragma unroll
    for (int i = 0; i < 8; ++i) h_on_out[(long long)b * 512 + lane + 64 * i] = ho[i];
    for (int a = 0; a < NQ; ++a) {
        const float* wo = wsm + a * 512;
        const float* wt = wsm + (NQ + a) * 512;
        float so = 0.f, st = 0.f, ss = 0.f;
#pragma unroll
        for (int i = 0; i < 8; ++i) {
            const float w1 = wo[lane + 64 * i], w2 = wt[lane + 64 * i];
            so = fmaf(ho[i], w1, so);
            ss = fmaf(hs[i], MDQN ? w2 : w1, ss);
            st = fmaf(ht[i], w2, st);
        }
        so = a0_wave_sum(so); st = a0_wave_sum(st); ss = a0_wave_sum(ss);
        const float bo_a = __int_as_float(__builtin_amdgcn_readlane(__float_as_int(hb_on), a)), bt_a = __int_as_float(__builtin_amdgcn_readlane(__float_as_int(hb_tg), a));
        if (lane == 0) { raw[wave][0][a] = so + bo_a; raw[wave][1][a] = st + bt_a; raw[wave][2][a] = ss + (MDQN ? bt_a : bo_a); }
    }
    // lane 0's tail, the text of a0_dqn_head_loss_kernel's but for the Munchausen target and the copy of draw in dsh (why it is written out twice:
    // profiles/r33_loss_split.md)
    if (lane == 0) {
    const int nsel = (s_sel && !MDQN) ? 2 : 1;
    float mean[3] = {0.f, 0.f, 0.f}, v[3] = {0.f, 0.f, 0.f};
    if (dueling)
        for (int s3 = 0; s3 < 3; ++s3) {
            float t = 0.f;
            for (int a = 0; a < A; ++a) t += raw[wave][s3][a];
            mean[s3] = t / (float)A;
            v[s3] = raw[wave][s3][A];
        }
    auto q = [&](int s3, int a) { return dueling ? v[s3] + (raw[wave][s3][a] - mean[s3]) : raw[wave][s3][a]; };
    float best = 0.f;
    int a_star = 0;
    for (int a = 0; a < A; ++a) {
        a0_first_max(a, q(nsel, a), best, a_star);
        q_on_out[(long long)b * A + a] = q(0, a);
        if (q_tg_out) q_tg_out[(long long)b * A + a] = q(1, a);
        if (MDQN && M.q_sel_out) M.q_sel_out[(long long)b * A + a] = q(2, a);
    }
    float y;
    if (MDQN) {
        y = a0_mdqn_target([&](int k) { return q(1, k); }, [&](int k) { return q(2, k); }, A, ab, rew_b, done_b, gamma_n, M.tau, M.lo);
    } else {
        const float qn = q(1, a_star);
        y = rew_b + (gamma_n * (1.f - done_b)) * qn;
    }
    const float g = a0_td_tail(q(0, ab) - y, wgt_b, loss + b, nan_flag);
    a0_onehot_dueling_bwd(draw + (long long)b * ld, A, dueling, ld, ab, g, dsh[wave]);
    }
    // head data gradient, fused: dh[k] = (h[k] > 0) * sum_c draw[c] * W_on[c][k] over the head's rows (what a0_dense_dgrad computes from
    // draw, W_on and the ReLU mask h) — the row's draw values come from lane 0 through LDS, the weights are already staged, h is in registers
    if (dh_out) {
        __builtin_amdgcn_s_waitcnt(0xc07f);      // lgkmcnt(0): lane 0's LDS stores of dsh have landed (one wave: lock step, LDS in order)
        __builtin_amdgcn_wave_barrier();
#pragma unroll
        for (int i = 0; i < 8; ++i) {
            float acc = 0.f;
            for (int c = 0; c < NQ; ++c) acc = fmaf(dsh[wave][c], wsm[c * 512 + lane + 64 * i], acc);
            dh_out[(long long)b * 512 + lane + 64 * i] = ho[i] > 0.f ? acc : 0.f;
        }
    }
}

// The one launcher behind a0_dqn_head_loss_slabs and a0_mdqn_head_loss_slabs (MDQN: slabs_sel is required, M carries tau > 0).
template <bool MDQN>
static int a0_scalar_head_loss_slabs(const float* slabs_on, const float* slabs_tg, const float* slabs_sel, long long slab_stride, int nslab, const float* b1_on,
                                     const float* b1_tg, float* h_on_out, const float* W_on, const float* b_on, const float* W_tg, const float* b_tg, int A, int dueling,
                                     int ld, const int* act, const float* rew, const float* done, const float* wgt, float gamma_n, int B, float* loss, float* q_on_out,
                                     float* q_tg_out, float* draw, int* nan_flag, float* dh_out, const a0_mdqn_par& M, void* stream) {
    const int NQ = A + (dueling ? 1 : 0);
    if (!slabs_on || !slabs_tg || (MDQN && !slabs_sel) || !b1_on || !b1_tg || !h_on_out || !W_on || !b_on || !W_tg || !b_tg || !act || !rew || !done || !wgt || !loss ||
        !q_on_out || !draw || !nan_flag || B < 1 || A < 1 || NQ > 24 || ld < NQ || nslab < 1 || slab_stride < (long long)B * 512 || (MDQN && !(M.tau > 0.f)))
        return a0_fail(A0_EINVAL, MDQN ? "a0_mdqn_head_loss_slabs: bad argument (A + dueling <= 24, tau > 0)" : "a0_dqn_head_loss_slabs: bad argument (A + dueling <= 24)");
    const size_t lds = (size_t)2 * NQ * 512 * sizeof(float);
    if (!a0_grant_dynamic_lds<a0_dqn_head_loss_slabs_kernel<MDQN>>(lds)) return a0_fail(A0_EINVAL, MDQN ? "a0_mdqn_head_loss_slabs: LDS" : "a0_dqn_head_loss_slabs: LDS");
    hipLaunchKernelGGL(a0_dqn_head_loss_slabs_kernel<MDQN>, dim3((B + 3) / 4), dim3(256), lds, (hipStream_t)stream, slabs_on, slabs_tg, slabs_sel, slab_stride, nslab, b1_on,
                       b1_tg, h_on_out, W_on, b_on, W_tg, b_tg, A, dueling, ld, act, rew, done, wgt, gamma_n, B, loss, q_on_out, q_tg_out, draw, nan_flag, dh_out, M);
    return a0_fail_hip((int)hipGetLastError(), MDQN ? "a0_mdqn_head_loss_slabs" : "a0_dqn_head_loss_slabs");
}

extern "C" int a0_dqn_head_loss_slabs(const float* slabs_on, const float* slabs_tg, const float* slabs_sel, long long slab_stride, int nslab, const float* b1_on,
                                      const float* b1_tg, float* h_on_out, const float* W_on, const float* b_on, const float* W_tg, const float* b_tg, int A,
                                      int dueling, int ld, const int* act, const float* rew, const float* done, const float* wgt, float gamma_n, int B, float* loss,
                                      float* q_on_out, float* q_tg_out, float* draw, int* nan_flag, float* dh_out, void* stream) {
    return a0_scalar_head_loss_slabs<false>(slabs_on, slabs_tg, slabs_sel, slab_stride, nslab, b1_on, b1_tg, h_on_out, W_on, b_on, W_tg, b_tg, A, dueling, ld, act, rew,
                                            done, wgt, gamma_n, B, loss, q_on_out, q_tg_out, draw, nan_flag, dh_out, a0_mdqn_par{0.f, 0.f, nullptr}, stream);
}

extern "C" int a0_mdqn_head_loss_slabs(const float* slabs_on, const float* slabs_tg, const float* slabs_cur, long long slab_stride, int nslab, const float* b1_on,
                                       const float* b1_tg, float* h_on_out, const float* W_on, const float* b_on, const float* W_tg, const float* b_tg, int A,
                                       int dueling, int ld, const int* act, const float* rew, const float* done, const float* wgt, float gamma_n, float tau, float lo,
                                       int B, float* loss, float* q_on_out, float* q_tg_out, float* q_cur_out, float* draw, int* nan_flag, float* dh_out, void* stream) {
    return a0_scalar_head_loss_slabs<true>(slabs_on, slabs_tg, slabs_cur, slab_stride, nslab, b1_on, b1_tg, h_on_out, W_on, b_on, W_tg, b_tg, A, dueling, ld, act, rew,
                                           done, wgt, gamma_n, B, loss, q_on_out, q_tg_out, draw, nan_flag, dh_out, a0_mdqn_par{tau, lo, q_cur_out}, stream);
}
