// What the one-launch update tail (optim.hip: a0_update_tail_kernel) shares with the kernels it replaces per update: the row-group sums of
// a0_reduce_segments_kernel (reduce.hip), the weight-copy layout and the bf16 terms of a0_conv_wt_kernel (encoder_fused.hip), and the one-thread
// bookkeeping of an optimizer step (a0_step_decide / a0_step_publish), which every Adam form runs and the tail has run in the launch in front of it.
// The scatter of a new weight into the weight copies is shared further: the soft target update (optim.hip), the reset and the recycle (net_reset.hip) use it too.
#pragma once
#include "a0_internal.h"

#include <cstdint>

// ---- slab sums: row group g of a workgroup adds the slabs z = g, g + 8, ... in increasing z; the eight partial sums meet in LDS and are added 0..7 from zero
// four of this row group's slabs requested before any is added (same order of additions): the loads of a 72-slab segment overlap instead of queueing
A0_D a0_f4 a0_rowgroup_sum4(const a0_f4* p, long long st4, int g, int nslab) {
    a0_f4 s = a0_zero4();
    for (int z = g; z < nslab; z += 32) {
        a0_f4 v[4];
#pragma unroll
        for (int u = 0; u < 4; ++u) v[u] = (z + 8 * u < nslab) ? p[(long long)(z + 8 * u) * st4] : a0_zero4();
#pragma unroll
        for (int u = 0; u < 4; ++u)
            if (z + 8 * u < nslab) { s.x += v[u].x; s.y += v[u].y; s.z += v[u].z; s.w += v[u].w; }
    }
    return s;
}
A0_D float a0_rowgroup_sum1(const float* p, long long slab_stride, int g, int nslab) {
    float s = 0.f;
    for (int z = g; z < nslab; z += 8) s += p[(long long)z * slab_stride];
    return s;
}

// ---- The weight-copy buffer `wt` that a0_conv_wt_kernel fills from the packed [N][K] weights and every fused kernel reads: the length of each
// segment and its offset, in floats, for C input channels.  This is the only description of the layout in the library.
struct a0_wt_layout {
    int C;
    constexpr int n_conv1x() const { return 48 * 64 * C; }      // conv1: fl(w/255) as three exact bf16 terms, a0_wring1 layout (32 x 64 C x 3 x 2 bytes)
    static constexpr int n_conv2 = 64 * 512;                    // conv2 fp32, fragment-major (a0_wring layout)
    static constexpr int n_conv3 = 64 * 576;                    // conv3 fp32, fragment-major
    static constexpr int n_conv2x = 96 * 512;                   // conv2 as three exact bf16 terms (a0_wring9 layout, N = 64): 64 x K x 3 x 2 bytes
    static constexpr int n_conv3x = 96 * 576;                   // conv3 likewise
    static constexpr int n_dgrad3x = 96 * 576;                  // conv3's data-gradient matrix (flipped taps) [576][64] as three bf16 terms, a0_wring9 layout, N = 64
    static constexpr int n_dgrad2x_phase = 48 * 256;            // conv2's data-gradient matrix of one stride phase [256][32], a0_wring9 layout, N = 32; four of them
    constexpr int conv1x() const { return 0; }
    constexpr int conv2() const { return n_conv1x(); }
    constexpr int conv3() const { return conv2() + n_conv2; }
    constexpr int conv2x() const { return conv3() + n_conv3; }
    constexpr int conv3x() const { return conv2x() + n_conv2x; }
    constexpr int dgrad3x() const { return conv3x() + n_conv3x; }
    constexpr int dgrad2x() const { return dgrad3x() + n_dgrad3x; }
    constexpr int total() const { return dgrad2x() + 4 * n_dgrad2x_phase; }
};

#if defined(__HIPCC__)
A0_HD uint32_t a0_bf16_trunc(float f) { return __float_as_uint(f) >> 16; }
A0_HD float a0_bf16_up(uint32_t h) { return __uint_as_float(h << 16); }
// w = hi + mid + lo EXACTLY, three bf16 terms of 8 significant bits each: term s (0 = hi, 1 = mid, 2 = lo) as bf16 bits
A0_HD uint32_t a0_bf16_term(float w, int s) {
    const uint32_t hi = a0_bf16_trunc(w);
    const float r1 = w - a0_bf16_up(hi);              // exact: at most 16 significant bits left
    const uint32_t mid = a0_bf16_trunc(r1);
    const float r2 = r1 - a0_bf16_up(mid);            // exact: at most 8 significant bits left
    return s == 0 ? hi : s == 1 ? mid : a0_bf16_trunc(r2);
}

// ---- the scatter into that layout (the inverse of a0_conv_wt_kernel's gather): the lane that holds a new convolution weight files it in the copies itself.
// Where a new convolution weight goes in the fused kernels' copies `wt` (online) / `wt_t` (target): the one description the tail, the blend, the reset and the
// recycle share.
struct a0_wt_sink {
    long long o1, o2, o3;                       // first weight of conv1 / conv2 / conv3 in the flat buffer
    int K1, wt4;                                // wt4: o1, o2, o3 multiples of four (four consecutive k of one row per 16-byte lane)
    float *wt, *wt_t;
};
// w: the convolution weights inside base[0, n_total) (`what`: the buffer's name in who's error text); wt may be NULL for a caller that files the target side only
static int a0_wt_sink_make(a0_wt_sink* S, const char* who, const char* what, const float* base, long long n_total, const a0_encoder_weights* w, int C, float* wt, float* wt_target) {
    const std::string name(who);
    if (!w || !w->w1 || !w->w2 || !w->w3 || C < 1 || !wt_target) return a0_fail(A0_EINVAL, (name + ": weight copies need the encoder weights, C >= 1 and the copies' buffers").c_str());
    if (!a0_aligned(16, wt, wt_target)) return a0_fail(A0_EINVAL, (name + ": the weight copies must be 16-byte aligned").c_str());
    *S = a0_wt_sink{w->w1 - base, w->w2 - base, w->w3 - base, C * 64, 0, wt, wt_target};
    if (S->o1 < 0 || S->o1 + 32LL * S->K1 > n_total || S->o2 < 0 || S->o2 + 64 * 512 > n_total || S->o3 < 0 || S->o3 + 64 * 576 > n_total)
        return a0_fail(A0_EINVAL, (name + ": the convolution weights must lie inside " + what + "[0, n_total)").c_str());
    S->wt4 = ((S->o1 | S->o2 | S->o3) % 4 == 0) ? 1 : 0;
    return A0_OK;
}

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

// ---- an optimizer step's bookkeeping, one thread: NaN skip, step count, bias corrections, "sync now".  a0_step_decide is the only place that derives them; it reads
// state[0] (NaN flag), state[1] (update_steps BEFORE this step), state[7] (the count at the last network reset, 0 without one) and the optional data-parallel flag.
struct a0_step { int skip, steps, sync; float step_size, bc2_sqrt; };
A0_D a0_step a0_step_decide(const int* state, const float* extra_flag, double lr, double b1, double b2, int target_freq) {
    a0_step S;
    S.skip = (state[0] != 0) || (extra_flag && extra_flag[0] != 0.f);
    S.steps = state[1] + (S.skip ? 0 : 1);
    const int since = S.steps - state[7];
    const int t = since > 0 ? since : 1;
    S.step_size = (float)(lr / (1.0 - pow(b1, (double)t)));
    S.bc2_sqrt = (float)sqrt(1.0 - pow(b2, (double)t));
    S.sync = (target_freq > 0 && (S.steps % target_freq) == 0) ? 1 : 0;      // evaluated even after a skipped step, like the reference
    return S;
}
// commit: state[1] <- the new count and the NaN flag down.  Without it the new count waits in state[5] for the next kernel on the stream to commit
// (a0_conv_wt_kernel): the folded Adam kernel publishes while its other workgroups are still reading state[0] and state[1].
A0_D void a0_step_publish(const a0_step& S, int* state, float* scal, bool commit) {
    if (S.skip) state[2] += 1;
    state[3] = S.skip; state[4] = S.sync;
    scal[0] = S.step_size; scal[1] = S.bc2_sqrt;
    if (commit) { state[1] = S.steps; state[0] = 0; }
    else state[5] = S.steps;
}
// what a kernel behind a publish steps with: words nobody writes while it runs
A0_D a0_step a0_step_published(const int* state, const float* scal) { return a0_step{state[3], 0, state[4], scal[0], scal[1]}; }

// The bookkeeping of the one-launch tail needs the NaN flag to be final — the loss kernel ran — and nothing else, so it rides in the last launch in front of the
// tail (conv1_wgrad.hip, or a launch of its own: net.hip).  It leaves state[5] as the folded form's commit does, so that both tails leave the same status block.
struct a0_tail_prep { int* state; float* scal; double lr, b1, b2; int target_freq; };
A0_D void a0_tail_prep_run(const a0_tail_prep& P) {
    const a0_step S = a0_step_decide(P.state, nullptr, P.lr, P.b1, P.b2, P.target_freq);
    P.state[5] = S.steps;
    a0_step_publish(S, P.state, P.scal, true);
}
#endif
