// What the one-launch update tail (optim.hip: a0_update_tail_kernel) shares with the kernels it replaces per update: the row-group sums of
// a0_reduce_segments_kernel (net.hip), the weight-copy layout and the bf16 terms of a0_conv_wt_kernel (encoder_fused.hip), and the one-thread
// bookkeeping of an optimizer step (a0_step_decide / a0_step_publish), which every Adam form runs and the tail has run in the launch in front of it.
#pragma once
#include "a0_defs.h"

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
