// Common definitions for the agent0_amd HIP library (gfx950 only).
#pragma once
#include <stdint.h>
#include <stddef.h>

#if defined(__HIPCC__)
#include <hip/hip_runtime.h>
#define A0_HD __host__ __device__ __forceinline__
#define A0_D __device__ __forceinline__
#else
#define A0_HD inline
#define A0_D inline
#endif

// 16-byte vector types usable from both hipcc and plain g++ (host emulation of the index math)
struct __attribute__((aligned(16))) a0_f4 { float x, y, z, w; };
struct __attribute__((aligned(16))) a0_i4 { int x, y, z, w; };

A0_HD a0_f4 a0_zero4() { a0_f4 v; v.x = 0.f; v.y = 0.f; v.z = 0.f; v.w = 0.f; return v; }

#if defined(__HIPCC__)
// the product alone, rounded to fp32: never contracted into the subtraction or the multiply-add that consumes it, so that stepping on g * coef gives the bits of
// a0_adam_step_sync on a gradient buffer multiplied by coef beforehand
A0_D float a0_mul_rounded(float a, float b) {
    float r;
    {
#pragma clang fp contract(off)
        r = a * b;
    }
    asm volatile("" : "+v"(r));      // the Adam arithmetic behind it sees a plain register value, as it sees a loaded gradient
    return r;
}
// One rounded subtraction and one fused multiply-add per element, kept out of the compiler's contraction choices (see a0_mul_rounded).
A0_D float a0_blend1(float t, float p, float tau) {
    float d;
    {
#pragma clang fp contract(off)
        d = p - t;
    }
    asm volatile("" : "+v"(d));
    return __builtin_fmaf(tau, d, t);
}
// "This update fires" for an action of period freq (net_reset.hip, feature_rank.hip): it was not NaN-skipped (state[3]) and left update_steps (state[1]) a positive
// multiple of freq; or `force`.  On every other update such a kernel returns after reading these two words.
A0_D bool a0_period_fires(const int* __restrict__ state, int freq, int force) {
    if (force) return true;
    const int steps = state[1];
    return state[3] == 0 && freq > 0 && steps > 0 && steps % freq == 0;
}
// butterfly reductions over the 64 lanes of a wave: every lane ends with the result
A0_D float a0_wave_sum(float v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    return v;
}
A0_D float a0_wave_max(float v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v = fmaxf(v, __shfl_xor(v, o, 64));
    return v;
}
#endif

// status codes returned by every exported function (include/agent0_hip.h)
enum {
    A0_OK = 0,
    A0_EINVAL = -1,   // bad argument (shape/alignment/null)
    A0_EHIP = -2,     // HIP runtime error, see a0_last_error()
    A0_ENOMEM = -3,
    A0_ESTATE = -4,   // call not valid in the current state
};

// launch families of the profiler probe (probe.hip; ops.py's PROBE_TAGS and bench.py's roofline use the numbers).  1 - 11: set on the backend before each GEMM of net_impl.h;
// 12 - 14: the fused kernels (14: the actor step's tail + env step + next observation's encoder in one kernel, a family of its own: the encoder's roofline keeps the pure launches)
enum { A0_TAG_NONE = 0, A0_TAG_CONV1_FWD = 1, A0_TAG_CONV2_FWD = 2, A0_TAG_CONV3_FWD = 3, A0_TAG_DENSE_FWD = 4, A0_TAG_DENSE_DGRAD = 5,
       A0_TAG_DENSE_WGRAD = 6, A0_TAG_CONV3_WGRAD = 7, A0_TAG_CONV3_DGRAD = 8, A0_TAG_CONV2_WGRAD = 9, A0_TAG_CONV2_DGRAD = 10, A0_TAG_CONV1_WGRAD = 11,
       A0_TAG_ENCODER_FUSED = 12, A0_TAG_ENCODER_DGRAD_FUSED = 13, A0_TAG_ACTOR_STEP_ENC = 14 };

// Geometry of a "virtual convolution": row m = (b, oh, ow) reads
//   in[b][oh*stride - pad + kh][ow*stride - pad + kw][c]
// Used for forward im2col (pad = 0) and for gather-form data gradients (stride = 1, pad > 0).
struct a0_geom {
    int Hin, Win, C;          // input spatial size and channels
    int Hout, Wout;           // rows per sample = Hout*Wout
    int stride, pad;
    int HWout;
    long long sample_stride;  // elements (bytes for u8) between consecutive samples of the input
    unsigned hw_magic, w_magic;   // ceil(2^32 / HWout), ceil(2^32 / Wout): row index -> (sample, oh, ow) without integer division (a0_udiv)
};

// floor(m / d) for any 32-bit m, given magic = ceil(2^32 / d), d >= 2: the multiply-high overestimates by at most one.
A0_HD unsigned a0_udiv_magic(unsigned d) { return d > 1 ? (unsigned)((0x100000000ull + d - 1) / d) : 0u; }
A0_HD int a0_udiv(int m, int d, unsigned magic) {
    if (d <= 1) return m;
    unsigned q = (unsigned)(((unsigned long long)(unsigned)m * magic) >> 32);
    if (q * (unsigned)d > (unsigned)m) --q;
    return (int)q;
}
