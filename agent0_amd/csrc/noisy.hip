// NoisyNet (gfx950): the effective weights of NoisyLinear modules and the fan-out of their gradients to sigma.
// W = mu + sigma * (f(eps_out) x f(eps_in)),  b = mu_b + sigma_b * f(eps_b),  f(x) = sign(x) sqrt|x|
// (reference agent0/deepq/model.py:54-62,73-87).  Blocks are [W (N*K) | b (N)]; a module is the rows [r0, r1) that
// belong to one NoisyLinear (q_head and value_head share a packed block but have their own noise vectors).
// Gradient fan-out: the weight-gradient kernels write d(eff) into the mu block (d mu = d eff); d sigma = d eff * eps.
#include "a0_internal.h"

A0_D float a0_noise_f(float x) { return (x > 0.f ? 1.f : (x < 0.f ? -1.f : 0.f)) * sqrtf(fabsf(x)); }

// Up to six NoisyLinear modules (first_dense, q_head, value_head of the online AND the target network: round 4) in one launch: workgroups [first_block[m], first_block[m+1]) serve module m.
struct a0_noisy_mod { const float* mu; const float* sigma; float* out; int N, K, r0, r1; const float* noise_in; const float* noise_out_w; const float* noise_out_b; };
struct a0_noisy_multi_args { a0_noisy_mod mod[6]; int first_block[7]; };

// element i of a module's rows * K weights and rows biases: its place in the block and its eps
struct a0_noisy_elem { long long off; float eps; };
A0_D a0_noisy_elem a0_noisy_elem_of(const a0_noisy_mod& M, long long i) {
    const long long rows = M.r1 - M.r0;
    if (i < rows * M.K) {
        const int n = (int)(i / M.K), k = (int)(i % M.K);
        return a0_noisy_elem{(long long)(M.r0 + n) * M.K + k, a0_noise_f(M.noise_out_w[n]) * a0_noise_f(M.noise_in[k])};
    }
    const int n = (int)(i - rows * M.K);
    return a0_noisy_elem{(long long)M.N * M.K + M.r0 + n, a0_noise_f(M.noise_out_b[n])};
}

template <bool GRAD>
__global__ void a0_noisy_multi_kernel(a0_noisy_multi_args A) {
    int mi = 0;
#pragma unroll
    for (int k = 1; k < 6; ++k) mi += ((int)blockIdx.x >= A.first_block[k]) ? 1 : 0;
    const a0_noisy_mod M = A.mod[mi];
    const int nblk = A.first_block[mi + 1] - A.first_block[mi];
    const long long rows = M.r1 - M.r0;
    const long long total = rows * M.K + rows;
    long long i = (long long)((int)blockIdx.x - A.first_block[mi]) * blockDim.x + threadIdx.x;
    const long long stride = (long long)nblk * blockDim.x;
    for (; i < total; i += stride) {
        const a0_noisy_elem E = a0_noisy_elem_of(M, i);
        if (GRAD) M.out[E.off] = M.mu[E.off] * E.eps;                 // d sigma = d eff * eps (mu = the gradient written into the mu block)
        else M.out[E.off] = M.mu[E.off] + M.sigma[E.off] * E.eps;     // eff = mu + sigma * eps
    }
}

// The same, four k per lane: 16-byte loads and stores, 32-bit index arithmetic (the element-wise kernel spends its time in a 64-bit division per element; this one
// runs at the HBM rate).  Every element is formed by the same expression as above; needs K % 4 == 0 and 16-byte aligned blocks / noise vectors (the packed layout's).
template <bool GRAD>
__global__ __launch_bounds__(256) void a0_noisy_multi_v4_kernel(a0_noisy_multi_args A) {
    int mi = 0;
#pragma unroll
    for (int k = 1; k < 6; ++k) mi += ((int)blockIdx.x >= A.first_block[k]) ? 1 : 0;
    const a0_noisy_mod M = A.mod[mi];
    const unsigned nblk = (unsigned)(A.first_block[mi + 1] - A.first_block[mi]);
    const unsigned rows = (unsigned)(M.r1 - M.r0), K4 = (unsigned)M.K >> 2, nw = rows * K4, total = nw + rows;
    const unsigned stride = nblk * 256u;
    for (unsigned i = ((unsigned)blockIdx.x - (unsigned)A.first_block[mi]) * 256u + threadIdx.x; i < total; i += stride) {
        if (i < nw) {
            const unsigned n = i / K4, k4 = i - n * K4;
            const long long off = (long long)(M.r0 + (int)n) * M.K + 4 * k4;
            const float eo = a0_noise_f(M.noise_out_w[n]);
            const a0_f4 ni = *(const a0_f4*)(M.noise_in + 4 * k4);
            const float e0 = eo * a0_noise_f(ni.x), e1 = eo * a0_noise_f(ni.y), e2 = eo * a0_noise_f(ni.z), e3 = eo * a0_noise_f(ni.w);
            const a0_f4 mu = *(const a0_f4*)(M.mu + off);
            a0_f4 o;
            if (GRAD) { o.x = mu.x * e0; o.y = mu.y * e1; o.z = mu.z * e2; o.w = mu.w * e3; }
            else {
                const a0_f4 sg = *(const a0_f4*)(M.sigma + off);
                o.x = mu.x + sg.x * e0; o.y = mu.y + sg.y * e1; o.z = mu.z + sg.z * e2; o.w = mu.w + sg.w * e3;
            }
            *(a0_f4*)(M.out + off) = o;
        } else {
            const unsigned n = i - nw;
            const long long off = (long long)M.N * M.K + M.r0 + (int)n;
            const float e = a0_noise_f(M.noise_out_b[n]);
            if (GRAD) M.out[off] = M.mu[off] * e;
            else M.out[off] = M.mu[off] + M.sigma[off] * e;
        }
    }
}

// The one launcher: nmod <= 6 checked modules (sigma unused under grad).  wide: the four-wide kernel, where every module allows it — no operand unaligned, no K
// that is not a multiple of 4; without it (the per-module entry points) always the element-wise kernel.
static int a0_noisy_launch(const char* who, bool grad, bool wide, int nmod, const a0_noisy_mod* mods, void* stream) {
    a0_noisy_multi_args A;
    int blocks = 0;
    bool v4 = wide;
    for (int m = 0; m < nmod && v4; ++m) {
        const a0_noisy_mod& M = mods[m];
        v4 = M.K % 4 == 0 && (long long)M.N * M.K < (1LL << 31) && a0_aligned(16, M.mu, M.out, M.noise_in, M.sigma);
    }
    for (int m = 0; m < 6; ++m) {
        A.first_block[m] = blocks;
        A.mod[m] = m < nmod ? mods[m] : a0_noisy_mod{nullptr, nullptr, nullptr, 1, 1, 0, 0, nullptr, nullptr, nullptr};
        if (m < nmod) blocks += (int)a0_grid_256((long long)(mods[m].r1 - mods[m].r0) * (v4 ? mods[m].K / 4 + 1 : mods[m].K + 1));
    }
    for (int m = nmod + 1; m <= 6; ++m) A.first_block[m] = 0x7fffffff;       // unused modules are never selected
    A.first_block[nmod] = blocks;                                              // end of the last real module
    const auto kernel = v4 ? (grad ? a0_noisy_multi_v4_kernel<true> : a0_noisy_multi_v4_kernel<false>) : (grad ? a0_noisy_multi_kernel<true> : a0_noisy_multi_kernel<false>);
    hipLaunchKernelGGL(kernel, dim3((unsigned)blocks), dim3(256), 0, (hipStream_t)stream, A);
    return a0_fail_hip((int)hipGetLastError(), who);
}

// nmod <= 6 modules; arrays are host arrays.  grad = 0: eff[m] = mu[m] + sigma[m] * eps (a0_noisy_compose per module);
// grad = 1: gsigma[m] (passed as eff) = gmu[m] (passed as mu) * eps (a0_noisy_grad_sigma per module; sigma unused).
extern "C" int a0_noisy_multi(int grad, int nmod, const float* const* mu, const float* const* sigma, float* const* eff, const int* N, const int* K, const int* r0,
                              const int* r1, const float* const* noise_in, const float* const* noise_out_w, const float* const* noise_out_b, void* stream) {
    if (nmod < 1 || nmod > 6 || !mu || !eff || !N || !K || !r0 || !r1 || !noise_in || !noise_out_w || !noise_out_b || (!grad && !sigma))
        return a0_fail(A0_EINVAL, "a0_noisy_multi: bad argument");
    a0_noisy_mod mods[6];
    for (int m = 0; m < nmod; ++m) {
        if (!mu[m] || !eff[m] || (!grad && !sigma[m]) || !noise_in[m] || !noise_out_w[m] || !noise_out_b[m] || N[m] < 1 || K[m] < 1 || r0[m] < 0 || r1[m] <= r0[m] || r1[m] > N[m])
            return a0_fail(A0_EINVAL, "a0_noisy_multi: bad module");
        mods[m] = a0_noisy_mod{mu[m], grad ? nullptr : sigma[m], eff[m], N[m], K[m], r0[m], r1[m], noise_in[m], noise_out_w[m], noise_out_b[m]};
    }
    return a0_noisy_launch("a0_noisy_multi", grad != 0, true, nmod, mods, stream);
}

// One module through the element-wise kernel, also for aligned operands: tests/test_gpu_kernels.py holds the four-wide kernel to it bit for bit.
extern "C" int a0_noisy_compose(const float* mu, const float* sigma, float* eff, int N, int K, int r0, int r1, const float* noise_in,
                                const float* noise_out_w, const float* noise_out_b, void* stream) {
    if (!mu || !sigma || !eff || !noise_in || !noise_out_w || !noise_out_b || N < 1 || K < 1 || r0 < 0 || r1 <= r0 || r1 > N) return a0_fail(A0_EINVAL, "a0_noisy_compose: bad argument");
    const a0_noisy_mod M{mu, sigma, eff, N, K, r0, r1, noise_in, noise_out_w, noise_out_b};
    return a0_noisy_launch("a0_noisy_compose", false, false, 1, &M, stream);
}

extern "C" int a0_noisy_grad_sigma(const float* gmu, float* gsigma, int N, int K, int r0, int r1, const float* noise_in,
                                   const float* noise_out_w, const float* noise_out_b, void* stream) {
    if (!gmu || !gsigma || !noise_in || !noise_out_w || !noise_out_b || N < 1 || K < 1 || r0 < 0 || r1 <= r0 || r1 > N) return a0_fail(A0_EINVAL, "a0_noisy_grad_sigma: bad argument");
    const a0_noisy_mod M{gmu, nullptr, gsigma, N, K, r0, r1, noise_in, noise_out_w, noise_out_b};
    return a0_noisy_launch("a0_noisy_grad_sigma", true, false, 1, &M, stream);
}
