// What the head epilogues and TD losses of loss.hip, loss_value.hip, loss_c51.hip and loss_quantile.hip share, each piece stated once: the first-maximum rule, the
// smooth-L1 tail and the one-hot dueling backward of the scalar heads, the ordered slab sum and the per-column dueling combine of the C51 / QR slab kernels, the C51
// projection's bin position and cross entropy, the HL-Gauss histogram that may stand in the projection's place, and on the host the dynamic-LDS limit and the
// descriptor of the kernels that work from the head GEMMs' slabs.  The fused kernels are held bit for bit to the launches they replace (tests/test_gpu_head_loss_chain.py, tests/test_gpu_engine.py): the arithmetic here is that of
// those launches, statement for statement.  What stays written out in its kernels and why: profiles/r33_loss_split.md.
#pragma once
#include "a0_internal.h"
#include <string>

// ------------------------------------------------------------------------------------------------ device pieces
// first maximum wins, like torch.argmax on CPU: candidates arrive in ascending a
A0_D void a0_first_max(int a, float v, float& best, int& besta) {
    if (a == 0 || v > best) { best = v; besta = a; }
}

// The tail of a scalar head's TD error d = q(s, a) - y: loss[b] = smooth_l1(d), the NaN flag, and the returned gradient w * clamp(d, -1, 1) w.r.t. q(s, a).
A0_D float a0_td_tail(float d, float w, float* loss_b, int* nan_flag) {
    const float ad = fabsf(d);
    const float l = (ad < 1.f) ? 0.5f * d * d : ad - 0.5f;
    *loss_b = l;
    if (l != l) atomicOr(nan_flag, 1);
    return w * fminf(fmaxf(d, -1.f), 1.f);
}

// Dueling backward of the scalar heads' dq = g * e_ab (a0_dueling_bwd_kernel) into row o [ld] of the head GEMM's output gradient: advantage column c gets
// dq[c] - sum(dq) / A, the value column sum(dq), the pad columns zero.  The sums run over all A entries from +0 as that kernel's do, which is what a -0 or NaN g needs to
// come out the same.  dsh (optional): a copy of the first 32 columns in LDS.
A0_D void a0_onehot_dueling_bwd(float* o, int A, int dueling, int ld, int ab, float g, float* dsh) {
    for (int c = 0; c < ld; ++c) {
        float out = 0.f;
        if (c < A) {
            out = (c == ab) ? g : 0.f;
            if (dueling) {
                float s = 0.f;
                for (int a = 0; a < A; ++a) s += (a == ab) ? g : 0.f;
                out -= s / (float)A;
            }
        } else if (dueling && c == A) {
            float s = 0.f;
            for (int a = 0; a < A; ++a) s += (a == ab) ? g : 0.f;
            out = s;
        }
        o[c] = out;
        if (dsh && c < 32) dsh[c] = out;
    }
}

A0_D void a0_add4(a0_f4& acc, const a0_f4& v) { acc.x += v.x; acc.y += v.y; acc.z += v.z; acc.w += v.w; }
// The rule of a0_reduce_bias_act_kernel, four columns wide: the sum of the first ns (<= 8) slabs in slab order, from zero, then the bias (read once the sum stands).
A0_D a0_f4 a0_slab_sum4(const a0_f4 (&t)[8], int ns, const a0_f4* bias) {
    a0_f4 acc = a0_zero4();
#pragma unroll
    for (int zz = 0; zz < 8; ++zz)
        if (zz < ns) a0_add4(acc, t[zz]);
    a0_add4(acc, *bias);
    return acc;
}

// Dueling combine of column t of one pass's head outputs x [A + 1][T] in LDS, in place (== a0_dueling_fwd_kernel; reference model.py:163-177): the caller's lane owns
// the column, it reads back only what it wrote itself.  fA = (float)A, formed by the kernel (why: profiles/r33_loss_split.md).
A0_D void a0_dueling_combine_col(float* x, int A, float fA, int T, int t) {
    float s = 0.f;
#pragma unroll 4
    for (int a = 0; a < A; ++a) s += x[a * T + t];
    const float mean = s / fA;
    const float v = x[A * T + t];
#pragma unroll 4
    for (int a = 0; a < A; ++a) x[a * T + t] = v + (x[a * T + t] - mean);
}
// C51 projection, one atom (reference agent.py:233-262): the Bellman-shifted, clamped support point of an atom of probability p, its fractional bin position, and
// the table entry of the gather form — bins lo and up and the mass each receives.  `on` false (a lane past the last atom): bins -1, which no lane number matches.
A0_D void a0_c51_bin(float rew, float done, float gamma_n, float atom, float p, float vmin, float vmax, float delta, int T, bool on,
                     int* lo_t, int* up_t, float* wl_t, float* wu_t) {
    float tz = rew + (gamma_n * (1.f - done)) * atom;
    tz = tz < vmin ? vmin : tz;                          // comparisons, not fminf / fmaxf: a NaN reward stays NaN and reaches the loss and the flag
    tz = tz > vmax ? vmax : tz;
    float bp = (tz - vmin) / delta;
    bp = bp > (float)(T - 1) ? (float)(T - 1) : bp;      // fl32(delta) may lie below the exact width: vmax itself then lands just above T - 1 and its bin would be T
    // (a NaN reward: bp is NaN and so are both weights below, which is what carries it to the loss and the flag; the indices then come from the device's
    // float -> int conversion of NaN, 0, and whatever they were the gather forms only compare them with lane numbers: nothing is addressed by them)
    int lo = (int)floorf(bp), up = (int)ceilf(bp);
    if (up > 0 && lo == up) lo -= 1;
    if (lo < T - 1 && lo == up) up += 1;
    *lo_t = on ? lo : -1;
    *up_t = on ? up : -1;
    *wl_t = p * ((float)up - bp);
    *wu_t = p * (bp - (float)lo);
}
// C51 cross entropy of the projected mass m (lane t: bin t) against the online net's log-softmax at the taken action, xo its logit (-inf past the last atom;
// agent.py:264-267).  All 64 lanes call; lane 0 stores the loss and raises the flag; a lane that holds an atom hands w * d loss / d logit of it to store_g.
template <class StoreG>
A0_D void a0_c51_xent(float xo, float m, bool on, float w, int lane, float* loss_b, int* nan_flag, StoreG&& store_g) {
    const float mxo = a0_wave_max(xo);
    const float eo = on ? expf(xo - mxo) : 0.f;
    const float so = a0_wave_sum(eo);
    const float logp = xo - mxo - logf(so);
    const float l = -a0_wave_sum(on ? m * logp : 0.f);
    const float msum = a0_wave_sum(m);
    if (lane == 0) {
        *loss_b = l;
        if (l != l) atomicOr(nan_flag, 1);
    }
    if (on) store_g(w * ((eo / so) * msum - m));
}
// HL-Gauss (learner.c51.hl_gauss; Farebrother et al. 2024): the mass of bin t — lane t's — of the Gaussian histogram of the clamped scalar target, from the target
// net's logit xt of atom t at the greedy next action (-inf past the last atom) and the atom itself, the bin's centre.  All 64 lanes call.  fp32, in the order of the
// selection step and of a0_c51_bin: v' = (sum e z) / (sum e) by a0_wave_sum, y = rew + (gamma_n (1 - done)) v', clamped by comparisons (a NaN reward stays NaN).
// Then in double: the edges e_k = vmin - delta / 2 + k delta, erf((e - y) / sigma / sqrt 2) at the lane's own two edges and at the two outer ones — the halves and
// the ones of Phi cancel in the quotient — and one rounding to fp32.  delta and sigma are doubles formed on the host.  Equal inputs give equal bytes.
A0_D float a0_hl_gauss_mass(float xt, bool on, float atom, float rew, float done, float gamma_n, float vmin, float vmax, double delta, double sigma, int T, int t) {
    const float mx = a0_wave_max(xt);
    float se = 0.f, sz = 0.f;
    if (on) {
        const float ex = expf(xt - mx);
        se += ex;
        sz += ex * atom;
    }
    se = a0_wave_sum(se);
    sz = a0_wave_sum(sz);
    float y = rew + (gamma_n * (1.f - done)) * (sz / se);
    y = y < vmin ? vmin : y;
    y = y > vmax ? vmax : y;
    const double yd = (double)y, e0 = (double)vmin - 0.5 * delta;
    auto erf_at = [&](int k) { return erf((e0 + (double)k * delta - yd) / sigma * 0.70710678118654752440); };
    const double q = (erf_at(t + 1) - erf_at(t)) / (erf_at(T) - erf_at(0));
    return on ? (float)q : 0.f;
}

// ------------------------------------------------------------------------------------------------ host pieces
// What the two HL-Gauss entry points and a0_learner_set_hl_gauss refuse of sigma = rho * delta (delta > 0 the double bin width, T bins): NaN, infinite, <= 0, not a
// normal fp32 number once rounded, above T * delta (rho > num_atoms: a sanity limit).  Returns A0_OK or the recorded error with the numbers named.
static int a0_hl_gauss_check(const char* who, double sigma, double delta, int T) {
    const float s32 = (float)sigma;
    const bool ok = sigma > 0.0 && sigma - sigma == 0.0 && s32 - s32 == 0.f && s32 >= 1.17549435e-38f && delta > 0.0 && sigma <= (double)T * delta;
    if (ok) return A0_OK;
    char msg[320];
    snprintf(msg, sizeof msg, "%s: learner.c51.hl_gauss: sigma = %g (ratio sigma / Delta = %g, Delta = %g) must be a normal fp32 number above 0 and at most "
                              "num_atoms * Delta = %g (ratio <= num_atoms = %d)", who, sigma, sigma / delta, delta, (double)T * delta, T);
    return a0_fail(A0_EINVAL, msg);
}

// Raises Kernel's dynamic-LDS limit to `lds` bytes where it is above what the kernel was last granted (one high-water mark per kernel); false: HIP refused.
template <auto Kernel>
static bool a0_grant_dynamic_lds(size_t lds) {
    static size_t configured = 0;
    if (lds <= configured) return true;
    if (hipFuncSetAttribute((const void*)Kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds) != hipSuccess) return false;
    configured = lds;
    return true;
}

// What a0_c51_head_loss_slabs_kernel and a0_qr_head_loss_slabs_kernel work from: the split-K slabs (a0_dense_fwd_partial) of the online head GEMM over [s ; s'] rows
// (s' only under double-Q) and of the target head GEMM over s', the head biases, the sample scalars and the outputs.  C51 adds atoms and support, QR its taus.
struct a0_hl_slabs {
    const float* s_on; long long stride_on; int nslab_on;      // online head slabs [nslab_on][R_on][ld]: rows [0, B) = s, rows [sel_off, sel_off + B) = s'
    const float* s_tg; long long stride_tg; int nslab_tg;      // target head slabs [nslab_tg][B][ld] on s'
    int sel_off;                                               // < 0: no double-Q (the greedy next action comes from the target's own values)
    const float *bias_on, *bias_tg; int ld, A, T, dueling;
    const int* act; const float *rew, *done, *wgt; float gamma_n; int B;
    float *loss, *draw, *q_on_out, *q_tg_out; int* a_star_out; int* nan_flag;
};
// Checks the arguments both entry points share and fills H.  `ok`: the family's own conditions; `limits`: what its message says about them, in brackets; lds: the
// launch's dynamic LDS.  Returns A0_OK or the recorded error, under the name `who`.
static int a0_hl_slabs_fill(a0_hl_slabs& H, const char* who, bool ok, const char* limits, size_t lds, const float* slabs_on, long long stride_on, int nslab_on,
                              int rows_on, const float* slabs_tg, long long stride_tg, int nslab_tg, int sel_off, const float* bias_on, const float* bias_tg, int ld,
                              int A, int T, int dueling, const int* act, const float* rew, const float* done, const float* wgt, float gamma_n, int B, float* loss,
                              float* draw, float* q_on_out, float* q_tg_out, int* a_star_out, int* nan_flag) {
    const int NQ = A + (dueling ? 1 : 0);
    auto fail = [&](const std::string& what) { return a0_fail(A0_EINVAL, (std::string(who) + what).c_str()); };      // the text is built only on the way out
    if (!ok || !slabs_on || !slabs_tg || !bias_on || !bias_tg || !act || !rew || !done || !wgt || !loss || !draw || !nan_flag || B < 1 || A < 1 || ld < NQ * T ||
        nslab_on < 1 || nslab_tg < 1 || rows_on < B || stride_on < (long long)rows_on * ld || stride_tg < (long long)B * ld ||
        (sel_off >= 0 && (sel_off < B || sel_off + B > rows_on)))
        return fail(std::string(": bad argument (") + limits + "; the s' rows of the online slabs must lie behind the s rows)");
    if (lds > 150 * 1024) return fail(": head too wide for LDS");
    if ((ld & 3) || (stride_on & 3) || (stride_tg & 3) || !a0_aligned(16, slabs_on, slabs_tg, bias_on, bias_tg))
        return fail(": slabs and biases must be 16-byte aligned, ld and the slab strides multiples of 4 floats");
    H = a0_hl_slabs{slabs_on, stride_on, nslab_on, slabs_tg, stride_tg, nslab_tg, sel_off, bias_on, bias_tg, ld, A, T, dueling, act, rew, done, wgt, gamma_n, B,
                      loss, draw, q_on_out, q_tg_out, a_star_out, nan_flag};
    return A0_OK;
}
