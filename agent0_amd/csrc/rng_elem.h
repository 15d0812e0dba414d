// One element of the Philox fills (rng.hip), as device functions: what a0_rng_uniform_kernel and a0_rng_normal_kernel write at position `pos` of stream
// (seed, stream).  rng.hip's kernels and the network reset (net_reset.hip: a0_net_reset_kernel) both call these, so a reset's fresh values are bit for bit the values
// a fill at the same positions gives.  Every product here is rounded on its own (no contraction), as in the kernels these formulas were moved out of.
#pragma once
#include "philox.h"

// u in [0, 1): the word's top 24 bits
A0_D float a0_rng_uniform_word(uint32_t w) {
#pragma clang fp contract(off)
    return (float)(w >> 8) * 0x1.0p-24f;
}
A0_D float a0_rng_uniform_at(unsigned long long seed, uint32_t stream, unsigned long long pos) { return a0_rng_uniform_word(a0_philox_word(seed, stream, pos)); }

// Box-Muller on the pair of words at positions (pos & ~1, pos | 1): the even position takes the cosine, the odd one the sine
A0_D float a0_rng_normal_words(uint32_t w_even, uint32_t w_odd, bool odd, float stdv) {
#pragma clang fp contract(off)
    const float u1 = (float)((w_even >> 8) + 1u) * 0x1.0p-24f;
    const float u2 = (float)(w_odd >> 8) * 0x1.0p-24f;
    const float rad = sqrtf(-2.0f * logf(u1));
    const float ang = 6.283185307179586f * u2;
    return stdv * rad * (odd ? sinf(ang) : cosf(ang));
}
A0_D float a0_rng_normal_at(unsigned long long seed, uint32_t stream, unsigned long long pos, float stdv) {
    const unsigned long long pair = pos & ~1ull;
    return a0_rng_normal_words(a0_philox_word(seed, stream, pair), a0_philox_word(seed, stream, pair + 1), (pos & 1) != 0, stdv);
}
