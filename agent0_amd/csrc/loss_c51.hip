// C51: projection of the Bellman-shifted target distribution + cross entropy, stand-alone and fused with the head tail — forward value and gradient w.r.t. the
// logits in one pass.  Restates reference agent0/deepq/agent.py:219-269 (C51Learner.train_step) with the dueling arithmetic of agent0/deepq/model.py:163-177.
#include "head_loss.h"
#include <type_traits>

// ------------------------------------------------------------------------------------------------ C51
// One wave per sample, one lane per atom (T <= 64).  The projection is computed in gather form — bin j sums the
// contributions of the atoms whose lo (then up) index equals j, in ascending atom order — which is the order the
// reference's two index_add_ calls produce on the CPU, so the result is deterministic (quirk Q20 resolved).
__global__ __launch_bounds__(64) void a0_c51_loss_kernel(const float* __restrict__ logits, const float* __restrict__ tgt_logits,
                                                          int A, int T, const int* __restrict__ act, const int* __restrict__ a_star,
                                                          const float* __restrict__ rew, const float* __restrict__ done,
                                                          const float* __restrict__ wgt, const float* __restrict__ atoms,
                                                          float gamma_n, float vmin, float vmax, float delta, int B,
                                                          float* __restrict__ loss, float* __restrict__ dlogits, float* __restrict__ m_out,
                                                          int* __restrict__ nan_flag) {
    __shared__ int s_lo[64], s_up[64];
    __shared__ float s_wl[64], s_wu[64];
    const int b = blockIdx.x, t = threadIdx.x;
    const bool on = t < T;
    // softmax of the target net's logits at the greedy next action
    const float* tp = tgt_logits + ((long long)b * A + a_star[b]) * T;
    const float xt = on ? tp[t] : -INFINITY;
    const float mxt = a0_wave_max(xt);
    const float et = on ? expf(xt - mxt) : 0.f;
    const float p = et / a0_wave_sum(et);
    // Bellman-shifted, clamped support and its fractional bin position
    a0_c51_bin(rew[b], done[b], gamma_n, on ? atoms[t] : 0.f, p, vmin, vmax, delta, T, on, &s_lo[t], &s_up[t], &s_wl[t], &s_wu[t]);
    __syncthreads();
    float m = 0.f;
    if (on) {
        for (int k = 0; k < T; ++k) if (s_lo[k] == t) m += s_wl[k];
        for (int k = 0; k < T; ++k) if (s_up[k] == t) m += s_wu[k];
    }
    if (m_out && on) m_out[(long long)b * T + t] = m;
    // cross entropy against the online net's log-softmax at the taken action
    const int a = act[b];
    const float* op = logits + ((long long)b * A + a) * T;
    a0_c51_xent(on ? op[t] : -INFINITY, m, on, wgt[b], t, loss + b, nan_flag, [&](float g) {
        for (int k = 0; k < A; ++k) dlogits[((long long)b * A + k) * T + t] = (k == a) ? g : 0.f;
    });
}

extern "C" int a0_loss_c51(const float* logits, const float* tgt_logits, int A, int T, const int* act, const int* a_star,
                           const float* rew, const float* done, const float* wgt, const float* atoms, float gamma_n,
                           float vmin, float vmax, int B, float* loss, float* dlogits, float* m_out, int* nan_flag, void* stream) {
    if (!logits || !tgt_logits || !act || !a_star || !rew || !done || !wgt || !atoms || !loss || !dlogits || !nan_flag || B < 1 || A < 1 || T < 2 || T > 64)
        return a0_fail(A0_EINVAL, "a0_loss_c51: bad argument (2 <= num_atoms <= 64)");
    const float delta = (float)(((double)vmax - (double)vmin) / (double)(T - 1));
    hipLaunchKernelGGL(a0_c51_loss_kernel, dim3(B), dim3(64), 0, (hipStream_t)stream, logits, tgt_logits, A, T, act, a_star, rew, done, wgt,
                       atoms, gamma_n, vmin, vmax, delta, B, loss, dlogits, m_out, nan_flag);
    return a0_fail_hip((int)hipGetLastError(), "a0_loss_c51");
}

// ------------------------------------------------------------------------------------------------ C51 with the HL-Gauss target (learner.c51.hl_gauss)
// a0_c51_loss_kernel with the Gaussian histogram of the clamped scalar target (a0_hl_gauss_mass) in the projection's place: one wave per sample, one lane per bin,
// no LDS.  sigma and delta are doubles (include/agent0_hip.h says why).
__global__ __launch_bounds__(64) void a0_c51_hl_gauss_loss_kernel(const float* __restrict__ logits, const float* __restrict__ tgt_logits, int A, int T,
                                                                   const int* __restrict__ act, const int* __restrict__ a_star, const float* __restrict__ rew,
                                                                   const float* __restrict__ done, const float* __restrict__ wgt, const float* __restrict__ atoms,
                                                                   float gamma_n, float vmin, float vmax, double delta, double sigma, int B, float* __restrict__ loss,
                                                                   float* __restrict__ dlogits, float* __restrict__ m_out, int* __restrict__ nan_flag) {
    const int b = blockIdx.x, t = threadIdx.x;
    const bool on = t < T;
    const float* tp = tgt_logits + ((long long)b * A + a_star[b]) * T;
    const float m = a0_hl_gauss_mass(on ? tp[t] : -INFINITY, on, on ? atoms[t] : 0.f, rew[b], done[b], gamma_n, vmin, vmax, delta, sigma, T, t);
    if (m_out && on) m_out[(long long)b * T + t] = m;
    const int a = act[b];
    const float* op = logits + ((long long)b * A + a) * T;
    a0_c51_xent(on ? op[t] : -INFINITY, m, on, wgt[b], t, loss + b, nan_flag, [&](float g) {
        for (int k = 0; k < A; ++k) dlogits[((long long)b * A + k) * T + t] = (k == a) ? g : 0.f;
    });
}

extern "C" int a0_loss_c51_hl_gauss(const float* logits, const float* tgt_logits, int A, int T, const int* act, const int* a_star, const float* rew, const float* done,
                                    const float* wgt, const float* atoms, float gamma_n, float vmin, float vmax, double sigma, int B, float* loss, float* dlogits,
                                    float* m_out, int* nan_flag, void* stream) {
    if (!logits || !tgt_logits || !act || !a_star || !rew || !done || !wgt || !atoms || !loss || !dlogits || !nan_flag || B < 1 || A < 1 || T < 2 || T > 64)
        return a0_fail(A0_EINVAL, "a0_loss_c51_hl_gauss: bad argument (2 <= num_atoms <= 64)");
    const double delta = ((double)vmax - (double)vmin) / (double)(T - 1);
    if (int rc = a0_hl_gauss_check("a0_loss_c51_hl_gauss", sigma, delta, T)) return rc;
    hipLaunchKernelGGL(a0_c51_hl_gauss_loss_kernel, dim3(B), dim3(64), 0, (hipStream_t)stream, logits, tgt_logits, A, T, act, a_star, rew, done, wgt, atoms, gamma_n,
                       vmin, vmax, delta, sigma, B, loss, dlogits, m_out, nan_flag);
    return a0_fail_hip((int)hipGetLastError(), "a0_loss_c51_hl_gauss");
}

// ------------------------------------------------------------------------------------------------ C51: head tail + loss from the head GEMMs' slabs
// C51Learner.train_step (reference agent.py:219-269) from the head GEMMs on, in ONE launch: the online head GEMM over [s ; s'] rows (s' only
// under double-Q) and the target head GEMM over s' leave their split-K slabs (a0_dense_fwd_partial); per sample one wave
//   sums them in slab order and adds the bias                                    (== a0_reduce_bias_act_kernel, three times)
//   applies the dueling combine per atom                                         (== a0_dueling_fwd_kernel, three times; model.py:163-177)
//   takes the expectation under softmax and its first maximum                    (== a0_select_action_kernel mode 2; agent.py:225-231)
//   projects the target distribution at that action and takes the cross entropy  (== a0_c51_loss_kernel; agent.py:233-267)
//   forms d loss / d logits and carries it back through the dueling combine      (== a0_dueling_bwd_kernel)
// — nine launches of ~5 us of latency each — statement for statement the same arithmetic, so the update's numbers do not change.  Four samples per
// workgroup; the workgroup first stages the 3 x (A + 1) x T head outputs of its samples in LDS (every thread a few columns, all slabs of a column
// requested before any is added), then each wave works on its sample with one lane per atom.
//
// learner.c51.hl_gauss: the same body with the projection block replaced by a0_hl_gauss_mass on the target's logits at a* (also under double-Q, where the selection
// loop's `best` is the online network's) — no tables, no gather loops.  One kernel template, two instantiations: HLG = false is the kernel as it was, instruction for
// instruction; HLG = true is what a0_c51_hl_gauss_head_loss_slabs launches, and its descriptor adds the double delta and sigma.
struct a0_c51hl_args : a0_hl_slabs {
    const float* atoms; float vmin, vmax, delta; float* m_out;
};
struct a0_c51hlg_args : a0_c51hl_args {
    double delta_d, sigma;
};
template <bool HLG> using a0_c51hl_args_t = std::conditional_t<HLG, a0_c51hlg_args, a0_c51hl_args>;
template <bool HLG>
__global__ __launch_bounds__(256) void a0_c51_head_loss_slabs_kernel(a0_c51hl_args_t<HLG> P) {
    extern __shared__ float xs[];                  // [4 samples][3 passes: online(s), target(s'), online(s')][ld]
    const int lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int A = P.A, T = P.T, NQ = A + (P.dueling ? 1 : 0), NC = NQ * T, ld = P.ld;
    const float fA = (float)A;
    const int b0 = blockIdx.x * 4;
    // this wave's sample: its scalars are requested before the staging loads, so that nothing in the arithmetic below waits for memory again
    const int bme = (b0 + wave) < P.B ? b0 + wave : P.B - 1;
    const int act_b = P.act[bme];
    const float rew_b = P.rew[bme], done_b = P.done[bme], wgt_b = P.wgt[bme];
    const float atom = lane < T ? P.atoms[lane] : 0.f;
    // staging: 16 bytes per lane and slab over the padded row (ld columns: the pad columns are summed too and never read), two row pieces x eight slabs
    // requested before anything is added — ~2 us of L2 / MALL latency per dependent batch is what this phase costs, so it is cut to two or three batches
    const int npass = P.sel_off < 0 ? 2 : 3;
    const int ld4 = ld >> 2, per = 4 * ld4, total = npass * per;
    for (int it0 = threadIdx.x; it0 < total; it0 += 512) {
        a0_f4 t[2][8];
        int ns[2], dst[2];
        const a0_f4* bp[2];
#pragma unroll
        for (int u = 0; u < 2; ++u) {
            const int it = it0 + 256 * u;
            const bool valid = it < total;
            const int p = valid ? it / per : 0, r = valid ? it - p * per : 0;
            const int sidx = r / ld4, c4 = r - sidx * ld4;
            int b = b0 + sidx;
            b = b < P.B ? b : P.B - 1;
            const float* base = (p == 1) ? P.s_tg : P.s_on;
            const long long st4 = ((p == 1) ? P.stride_tg : P.stride_on) >> 2;
            ns[u] = valid ? ((p == 1) ? P.nslab_tg : P.nslab_on) : 0;
            const a0_f4* sp = (const a0_f4*)(base + (long long)(((p == 2) ? P.sel_off : 0) + b) * ld) + c4;
            bp[u] = (const a0_f4*)((p == 1) ? P.bias_tg : P.bias_on) + c4;
            dst[u] = (sidx * 3 + p) * ld + 4 * c4;
#pragma unroll
            for (int zz = 0; zz < 8; ++zz) t[u][zz] = (zz < ns[u]) ? sp[(long long)zz * st4] : a0_zero4();
            // more than eight slabs (never the case for a 512-deep head): the rest joins slab by slab below
            if (ns[u] > 8) {
                a0_f4 acc = a0_zero4();
#pragma unroll
                for (int zz = 0; zz < 8; ++zz) a0_add4(acc, t[u][zz]);
                for (int z = 8; z < ns[u]; ++z) a0_add4(acc, sp[(long long)z * st4]);
                t[u][0] = acc;
                ns[u] = 1;
            }
        }
#pragma unroll
        for (int u = 0; u < 2; ++u) {
            if (it0 + 256 * u >= total) continue;
            *(a0_f4*)(xs + dst[u]) = a0_slab_sum4(t[u], ns[u], bp[u]);
        }
    }
    __syncthreads();
    const int b = b0 + wave;
    if (b >= P.B) return;
    float* X = xs + (long long)wave * 3 * ld;      // pass p of this wave's sample at X + p * ld
    const int t = lane;
    const bool on = t < T;
    // dueling combine per atom: each lane reads back only what it wrote itself (column t of every action), so no fence is needed up to the outputs
    if (P.dueling && on)
        for (int p = 0; p < npass; ++p) a0_dueling_combine_col(X + p * ld, A, fA, T, t);
    if (on) {
        if (P.q_on_out) for (int a = 0; a < A; ++a) P.q_on_out[((long long)b * A + a) * T + t] = X[a * T + t];
        if (P.q_tg_out) for (int a = 0; a < A; ++a) P.q_tg_out[((long long)b * A + a) * T + t] = X[ld + a * T + t];
    }
    // greedy next action: expectation of the selecting network's distribution, first maximum (a0_select_action_kernel, mode 2)
    const float* xsel = X + (P.sel_off < 0 ? 1 : 2) * ld;
    float best = 0.f;
    int a_star = 0;
    for (int a = 0; a < A; ++a) {
        const float xv = on ? xsel[a * T + t] : -INFINITY;
        const float mx = a0_wave_max(xv);
        float se = 0.f, sz = 0.f;
        if (on) {
            const float ex = expf(xv - mx);
            se += ex;
            sz += ex * atom;
        }
        se = a0_wave_sum(se);
        sz = a0_wave_sum(sz);
        a0_first_max(a, sz / se, best, a_star);
    }
    if (P.a_star_out && lane == 0) P.a_star_out[b] = a_star;
    float m = 0.f;
    if constexpr (HLG) {
        // the Gaussian histogram of the clamped scalar target, from the target's logits at a* (a0_c51_hl_gauss_loss_kernel)
        m = a0_hl_gauss_mass(on ? X[ld + a_star * T + t] : -INFINITY, on, atom, rew_b, done_b, P.gamma_n, P.vmin, P.vmax, P.delta_d, P.sigma, T, t);
    } else {
        // projection of the target distribution at a* (a0_c51_loss_kernel)
        __shared__ __attribute__((aligned(16))) int s_lo[4][64], s_up[4][64];
        __shared__ __attribute__((aligned(16))) float s_wl[4][64], s_wu[4][64];
        const float xt = on ? X[ld + a_star * T + t] : -INFINITY;
        const float mxt = a0_wave_max(xt);
        const float et = on ? expf(xt - mxt) : 0.f;
        const float pr = et / a0_wave_sum(et);
        a0_c51_bin(rew_b, done_b, P.gamma_n, atom, pr, P.vmin, P.vmax, P.delta, T, on, &s_lo[wave][t], &s_up[wave][t], &s_wl[wave][t], &s_wu[wave][t]);
        // one wave: its LDS writes above are ordered before its LDS reads below (in-order LDS queue); the fences keep the compiler from moving them
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
        __builtin_amdgcn_wave_barrier();
        __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
        if (on) {
            // ascending atom order, as in a0_c51_loss_kernel; four table entries per LDS read (entries k >= T hold -1 and never match)
            const int4* lo4 = (const int4*)s_lo[wave];
            const int4* up4 = (const int4*)s_up[wave];
            const a0_f4* wl4 = (const a0_f4*)s_wl[wave];
            const a0_f4* wu4 = (const a0_f4*)s_wu[wave];
#pragma unroll
            for (int k4 = 0; k4 < 16; ++k4)
                if (4 * k4 < T) {
                    const int4 L = lo4[k4]; const a0_f4 Wv = wl4[k4];
                    if (L.x == t) m += Wv.x;
                    if (L.y == t) m += Wv.y;
                    if (L.z == t) m += Wv.z;
                    if (L.w == t) m += Wv.w;
                }
#pragma unroll
            for (int k4 = 0; k4 < 16; ++k4)
                if (4 * k4 < T) {
                    const int4 U = up4[k4]; const a0_f4 Wv = wu4[k4];
                    if (U.x == t) m += Wv.x;
                    if (U.y == t) m += Wv.y;
                    if (U.z == t) m += Wv.z;
                    if (U.w == t) m += Wv.w;
                }
        }
    }
    if (P.m_out && on) P.m_out[(long long)b * T + t] = m;
    // cross entropy at the taken action (a0_c51_loss_kernel); d loss / d logits goes back through the dueling combine (a0_dueling_bwd_kernel on a dq that is zero outside
    // the taken action: the sum over all A entries from +0 as that kernel's, which is what a -0 or NaN g needs), straight into the head GEMM's output gradient
    float* o = P.draw + (long long)b * ld;
    a0_c51_xent(on ? X[act_b * T + t] : -INFINITY, m, on, wgt_b, lane, P.loss + b, P.nan_flag, [&](float g) {
        float sdl = 0.f;
        for (int k = 0; k < A; ++k) sdl += (k == act_b) ? g : 0.f;
        for (int k = 0; k < A; ++k) {
            float out = (k == act_b) ? g : 0.f;
            if (P.dueling) out -= sdl / (float)A;
            o[k * T + t] = out;
        }
        if (P.dueling) o[A * T + t] = sdl;
    });
    for (int c = NC + lane; c < ld; c += 64) o[c] = 0.f;
}

extern "C" int a0_c51_head_loss_slabs(const float* slabs_on, long long stride_on, int nslab_on, int rows_on, const float* slabs_tg, long long stride_tg, int nslab_tg,
                                      int sel_off, const float* bias_on, const float* bias_tg, int ld, int A, int T, int dueling, const int* act, const float* rew,
                                      const float* done, const float* wgt, const float* atoms, float gamma_n, float vmin, float vmax, int B, float* loss, float* draw,
                                      float* q_on_out, float* q_tg_out, float* m_out, int* a_star_out, int* nan_flag, void* stream) {
    const size_t lds = (size_t)4 * 3 * ld * sizeof(float);
    a0_c51hl_args P;
    if (int rc = a0_hl_slabs_fill(P, "a0_c51_head_loss_slabs", atoms && T >= 2 && T <= 64, "2 <= num_atoms <= 64", lds, slabs_on, stride_on, nslab_on, rows_on, slabs_tg,
                                  stride_tg, nslab_tg, sel_off, bias_on, bias_tg, ld, A, T, dueling, act, rew, done, wgt, gamma_n, B, loss, draw, q_on_out, q_tg_out,
                                  a_star_out, nan_flag))
        return rc;
    if (!a0_grant_dynamic_lds<a0_c51_head_loss_slabs_kernel<false>>(lds)) return a0_fail(A0_EINVAL, "a0_c51_head_loss_slabs: LDS");
    P.atoms = atoms; P.vmin = vmin; P.vmax = vmax; P.delta = (float)(((double)vmax - (double)vmin) / (double)(T - 1)); P.m_out = m_out;
    hipLaunchKernelGGL(a0_c51_head_loss_slabs_kernel<false>, dim3((B + 3) / 4), dim3(256), lds, (hipStream_t)stream, P);
    return a0_fail_hip((int)hipGetLastError(), "a0_c51_head_loss_slabs");
}

extern "C" int a0_c51_hl_gauss_head_loss_slabs(const float* slabs_on, long long stride_on, int nslab_on, int rows_on, const float* slabs_tg, long long stride_tg,
                                               int nslab_tg, int sel_off, const float* bias_on, const float* bias_tg, int ld, int A, int T, int dueling, const int* act,
                                               const float* rew, const float* done, const float* wgt, const float* atoms, float gamma_n, float vmin, float vmax,
                                               double sigma, int B, float* loss, float* draw, float* q_on_out, float* q_tg_out, float* m_out, int* a_star_out,
                                               int* nan_flag, void* stream) {
    const size_t lds = (size_t)4 * 3 * ld * sizeof(float);
    a0_c51hlg_args P;
    if (int rc = a0_hl_slabs_fill(P, "a0_c51_hl_gauss_head_loss_slabs", atoms && T >= 2 && T <= 64, "2 <= num_atoms <= 64", lds, slabs_on, stride_on, nslab_on, rows_on,
                                  slabs_tg, stride_tg, nslab_tg, sel_off, bias_on, bias_tg, ld, A, T, dueling, act, rew, done, wgt, gamma_n, B, loss, draw, q_on_out,
                                  q_tg_out, a_star_out, nan_flag))
        return rc;
    P.delta_d = ((double)vmax - (double)vmin) / (double)(T - 1);
    if (int rc = a0_hl_gauss_check("a0_c51_hl_gauss_head_loss_slabs", sigma, P.delta_d, T)) return rc;
    if (!a0_grant_dynamic_lds<a0_c51_head_loss_slabs_kernel<true>>(lds)) return a0_fail(A0_EINVAL, "a0_c51_hl_gauss_head_loss_slabs: LDS");
    P.atoms = atoms; P.vmin = vmin; P.vmax = vmax; P.delta = (float)P.delta_d; P.m_out = m_out; P.sigma = sigma;
    hipLaunchKernelGGL(a0_c51_head_loss_slabs_kernel<true>, dim3((B + 3) / 4), dim3(256), lds, (hipStream_t)stream, P);
    return a0_fail_hip((int)hipGetLastError(), "a0_c51_hl_gauss_head_loss_slabs");
}
