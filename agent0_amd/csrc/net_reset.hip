// Periodic re-initialisation of the Q-network over the flat parameter buffer (gfx950): shrink-and-perturb resets (learner.net_reset_freq) and dormant-neuron
// scoring with ReDo recycling (learner.redo_freq).  Both run behind the update's Adam form (optim.hip), decide for themselves on the device whether this update is
// one of theirs, draw their fresh values from the rule table of a0_net_reset_seg and file new convolution weights through update_tail.h's scatter.
#include "a0_internal.h"
#include "rng_elem.h"
#include "update_tail.h"

// a0_period_fires ("this update fires" for an action of period freq): a0_defs.h, shared with feature_rank.hip.
// ... and which one it is: k = update_steps / freq, or the caller's under `force`.  Fresh values are positioned by (k, flat index).
A0_D long long a0_period_index(const int* __restrict__ state, int freq, int force, long long k_host) { return force ? k_host : (long long)(state[1] / freq); }
// the seed (32 bits) travels in a vector register: Philox's key schedule of a uniform seed would be hoisted into twenty scalar registers for the whole loop
A0_D unsigned long long a0_seed_vgpr(unsigned long long seed_arg) {
    uint32_t seed_v = (uint32_t)seed_arg;
    asm volatile("" : "+v"(seed_v));
    return seed_v;
}

// ------------------------------------------------------------------------------------------------ periodic network resets
// learner.net_reset_freq = N: after an update that was not NaN-skipped and left update_steps a positive multiple of N, the Q-network is re-initialised in ONE launch
// behind the update's Adam form (and behind a0_target_blend): the head blocks are replaced by fresh values, the encoder blocks keep the share alpha of theirs
// (shrink and perturb), Adam's moments are zeroed, its bias correction restarts (state[7] <- state[1]), the target becomes a copy of the online network and the
// lane that holds a convolution weight files it in both networks' weight copies.
// Fresh values: element i at reset k = update_steps / N draws from Philox stream A0_STREAM_RESET of the seed at position k * n_total + i — a function of
// (seed, k, i) alone; a normal element is a0_rng_normal's value there, a uniform one bound * (2 u - 1) with u a0_rng_uniform's (rng_elem.h).
struct a0_reset_table { a0_net_reset_seg s[A0_NET_RESET_MAX_SEGS]; int n; };
// the rule of one flat index: kind < 0 outside every segment; keep is the share that survives (alpha32 or 0); end: one past the segment's last index
struct a0_reset_rule { long long end; int kind; float scale, keep; };

// every lane walks the table in the same order (uniform loads of the by-value table, no indexed access to it); outside every segment `end` is where the next one starts
A0_D a0_reset_rule a0_reset_find(const a0_reset_table& T, float alpha, long long i, long long n_total) {
    a0_reset_rule R{n_total, -1, 0.f, 1.f};
#pragma nounroll
    for (int s = 0; s < T.n; ++s) {
        const long long lo = T.s[s].offset, hi = lo + T.s[s].count;
        if (i >= lo && i < hi) { R.end = hi; R.kind = T.s[s].kind; R.scale = T.s[s].scale; R.keep = T.s[s].keep ? alpha : 0.f; }
        else if (lo > i && lo < R.end && R.kind < 0) R.end = lo;
    }
    return R;
}
// 2u - 1 is exact in fp32 (u is a multiple of 2^-24 below 1), then one rounded multiply
A0_D float a0_reset_uniform(float bound, float u) {
#pragma clang fp contract(off)
    return bound * (2.0f * u - 1.0f);
}
A0_D float a0_reset_fresh1(const a0_reset_rule& R, unsigned long long seed, unsigned long long pos, uint32_t stream = A0_STREAM_RESET) {
    if (R.kind == A0_NET_RESET_NORMAL) return a0_rng_normal_at(seed, stream, pos, R.scale);
    if (R.kind == A0_NET_RESET_UNIFORM) return a0_reset_uniform(R.scale, a0_rng_uniform_at(seed, stream, pos));
    return R.scale;
}
// four consecutive positions that share one Philox block (pos0 a multiple of four): one block, two Box-Muller pairs — the words a0_philox_word would pick
A0_D a0_f4 a0_reset_fresh4(const a0_reset_rule& R, unsigned long long seed, unsigned long long pos0) {
    a0_f4 f;
    if (R.kind == A0_NET_RESET_CONST) { f.x = f.y = f.z = f.w = R.scale; return f; }
    const unsigned long long blk = pos0 >> 2;
    const a0_u4 o = a0_philox4x32_10((uint32_t)blk, (uint32_t)(blk >> 32), A0_STREAM_RESET, 0u, (uint32_t)seed, (uint32_t)(seed >> 32));
    if (R.kind == A0_NET_RESET_NORMAL) {
        f.x = a0_rng_normal_words(o.x, o.y, false, R.scale); f.y = a0_rng_normal_words(o.x, o.y, true, R.scale);
        f.z = a0_rng_normal_words(o.z, o.w, false, R.scale); f.w = a0_rng_normal_words(o.z, o.w, true, R.scale);
    } else {
        f.x = a0_reset_uniform(R.scale, a0_rng_uniform_word(o.x)); f.y = a0_reset_uniform(R.scale, a0_rng_uniform_word(o.y));
        f.z = a0_reset_uniform(R.scale, a0_rng_uniform_word(o.z)); f.w = a0_reset_uniform(R.scale, a0_rng_uniform_word(o.w));
    }
    return f;
}
// keep == 0: the fresh value itself; otherwise fmaf(keep, fl32(p - phi), phi) — a0_blend1's form with the fresh value in the target's place
A0_D float a0_reset_mix(const a0_reset_rule& R, float p, float phi) { return R.keep == 0.f ? phi : a0_blend1(phi, p, R.keep); }

template <bool W>
__global__ __launch_bounds__(256) void a0_net_reset_kernel(float* __restrict__ p, float* __restrict__ target, float* __restrict__ m, float* __restrict__ v, long long n_adam,
                                                           long long n_total, a0_reset_table T, float alpha, unsigned long long seed_arg, int* __restrict__ state, int freq,
                                                           int force, long long k_host, int vec4, a0_wt_sink B) {
    if (!a0_period_fires(state, freq, force)) return;
    const long long k = a0_period_index(state, freq, force, k_host);
    // a fresh optimizer: a0_step_decide counts t from here (nobody reads state[7] during this launch)
    if (state && blockIdx.x == 0 && threadIdx.x == 0) state[7] = state[1];
    const unsigned long long seed = a0_seed_vgpr(seed_arg);
    const unsigned long long base = (unsigned long long)k * (unsigned long long)n_total;
    const long long stride = (long long)gridDim.x * blockDim.x;
    const long long groups = (n_total + 3) >> 2;
    // a lane owns four consecutive elements.  `wide`: the buffers are 16-byte aligned, the four share a Philox block and, with weight copies, a row of a convolution
    // matrix; where they also lie inside one segment (or between two) they move as 16 bytes.  Everything else — a segment boundary inside the four (the real / pad
    // boundary of a noisy bias), the tail of n_total % 4 floats, 4-byte-aligned buffers — goes element by element through the same arithmetic.
    const bool wide = vec4 && (base & 3) == 0 && (!W || B.wt4);
    for (long long j = (long long)blockIdx.x * blockDim.x + threadIdx.x; j < groups; j += stride) {
        const long long e0 = 4 * j;
        const a0_reset_rule R = a0_reset_find(T, alpha, e0, n_total);
        if (wide && e0 + 4 <= R.end) {
            a0_f4 pv = ((a0_f4*)p)[j];
            if (R.kind >= 0 && R.keep != 1.f) {
                const a0_f4 f = a0_reset_fresh4(R, seed, base + (unsigned long long)e0);
                pv.x = a0_reset_mix(R, pv.x, f.x); pv.y = a0_reset_mix(R, pv.y, f.y); pv.z = a0_reset_mix(R, pv.z, f.z); pv.w = a0_reset_mix(R, pv.w, f.w);
                ((a0_f4*)p)[j] = pv;
            }
            ((a0_f4*)target)[j] = pv;
            if (e0 + 4 <= n_adam) { ((a0_f4*)m)[j] = a0_zero4(); ((a0_f4*)v)[j] = a0_zero4(); }
            else {
#pragma unroll
                for (int e = 0; e < 4; ++e) if (e0 + e < n_adam) { m[e0 + e] = 0.f; v[e0 + e] = 0.f; }
            }
            continue;
        }
#pragma nounroll
        for (long long idx = e0; idx < e0 + 4 && idx < n_total; ++idx) {
            const a0_reset_rule Re = a0_reset_find(T, alpha, idx, n_total);
            float x = p[idx];
            if (Re.kind >= 0 && Re.keep != 1.f) { x = a0_reset_mix(Re, x, a0_reset_fresh1(Re, seed, base + (unsigned long long)idx)); p[idx] = x; }
            target[idx] = x;
            if (idx < n_adam) { m[idx] = 0.f; v[idx] = 0.f; }
        }
    }
    // the weight copies of BOTH networks (the target is the online network after a reset), in a pass of their own over the convolution blocks: every lane files the
    // parameters it has just written itself (the same lane-to-element map)
    if constexpr (W) {
        const long long c_lo = (B.o1 < B.o2 ? (B.o1 < B.o3 ? B.o1 : B.o3) : (B.o2 < B.o3 ? B.o2 : B.o3)) >> 2;
        long long c_hi = B.o1 + 32LL * B.K1;
        if (B.o2 + 64 * 512 > c_hi) c_hi = B.o2 + 64 * 512;
        if (B.o3 + 64 * 576 > c_hi) c_hi = B.o3 + 64 * 576;
        c_hi = (c_hi + 3) >> 2;
        for (long long j = (long long)blockIdx.x * blockDim.x + threadIdx.x; j < c_hi && j < groups; j += stride) {      // the first pass's groups, lane for lane
            if (j < c_lo) continue;
            const long long e0 = 4 * j;
            if (wide && e0 + 4 <= n_total) a0_tail_wt4(B, true, true, e0, ((const a0_f4*)p)[j]);
            else {
#pragma nounroll
                for (long long idx = e0; idx < e0 + 4 && idx < n_total; ++idx) a0_tail_wt1(B, true, true, idx, p[idx]);
            }
        }
    }
}

// the by-value table of a launch from the caller's rules, checked (`who`: the entry point's name in the error text)
static int a0_reset_table_make(a0_reset_table* T, const char* who, const a0_net_reset_seg* segs, int n_segs, long long n_adam) {
    const std::string name(who);
    if (n_segs < 0 || n_segs > A0_NET_RESET_MAX_SEGS || (n_segs > 0 && !segs)) return a0_fail(A0_EINVAL, (name + ": between 0 and A0_NET_RESET_MAX_SEGS segments").c_str());
    T->n = n_segs;
    long long at = 0;
    for (int s = 0; s < A0_NET_RESET_MAX_SEGS; ++s) {
        if (s >= n_segs) { T->s[s] = a0_net_reset_seg{0, 0, A0_NET_RESET_CONST, 0.f, 0}; continue; }
        const a0_net_reset_seg& g = segs[s];
        if (g.offset < at || g.count < 1 || g.offset + g.count > n_adam) return a0_fail(A0_EINVAL, (name + ": the segments must be ascending, disjoint and inside [0, n_adam)").c_str());
        if (g.kind != A0_NET_RESET_CONST && g.kind != A0_NET_RESET_NORMAL && g.kind != A0_NET_RESET_UNIFORM) return a0_fail(A0_EINVAL, (name + ": unknown segment kind").c_str());
        if (!(g.scale == g.scale) || g.scale - g.scale != 0.f || (g.keep != 0 && g.keep != 1)) return a0_fail(A0_EINVAL, (name + ": a segment's scale must be finite and its keep flag 0 or 1").c_str());
        at = g.offset + g.count;
        T->s[s] = g;
    }
    return A0_OK;
}

extern "C" int a0_net_reset(float* params, float* target, float* exp_avg, float* exp_avg_sq, long long n_adam, long long n_total, const a0_net_reset_seg* segs, int n_segs,
                            double alpha, unsigned long long seed, int* state, int freq, int force, long long k_host, const a0_encoder_weights* w, int C, float* wt,
                            float* wt_target, void* stream) {
    if (!params || !target || !exp_avg || !exp_avg_sq || n_adam < 1 || n_total < n_adam || (!force && !state) || freq < 0 || (force && k_host < 0) ||
        !a0_aligned(4, params, target, exp_avg, exp_avg_sq))
        return a0_fail(A0_EINVAL, "a0_net_reset: bad argument");
    if (!(alpha >= 0.0) || !(alpha <= 1.0)) return a0_fail(A0_EINVAL, "a0_net_reset: alpha must lie in [0, 1]");
    a0_reset_table T;
    if (int e = a0_reset_table_make(&T, "a0_net_reset", segs, n_segs, n_adam)) return e;
    a0_wt_sink B{0, 0, 0, 0, 0, nullptr, nullptr};
    if (wt || wt_target) {
        if (!wt) return a0_fail(A0_EINVAL, "a0_net_reset: weight copies need wt and wt_target, both or neither");
        if (int e = a0_wt_sink_make(&B, "a0_net_reset", "params", params, n_total, w, C, wt, wt_target)) return e;
    }
    const int vec4 = a0_aligned(16, params, target, exp_avg, exp_avg_sq) ? 1 : 0;
    const float alpha32 = (float)alpha;       // rounded to fp32 once
    const unsigned long long seed32 = seed & 0xFFFFFFFFull;
    hipLaunchKernelGGL(wt ? a0_net_reset_kernel<true> : a0_net_reset_kernel<false>, dim3(a0_grid_256((n_total + 3) / 4)), dim3(256), 0, (hipStream_t)stream,
                       params, target, exp_avg, exp_avg_sq, n_adam, n_total, T, alpha32, seed32, state, freq, force, k_host, vec4, B);
    return a0_fail_hip((int)hipGetLastError(), "a0_net_reset");
}

// ------------------------------------------------------------------------------------------------ dormant neurons and ReDo
// learner.redo_freq = N (Sokar et al. 2023): after an update that was not NaN-skipped and left update_steps a positive multiple of N, three launches behind the
// update's Adam form (and a0_target_blend), in front of a0_net_reset: (1) per-workgroup sums of |activation| per neuron over the differentiated pass's four buffers,
// (2) one workgroup finishes them into the scores s_i = m_i / mean_j(m_j), the mask s_i <= tau and the counts, (3) the dormant neurons are recycled.
// Everything is summed in double in a fixed order (the rows of a workgroup by the geometry alone, the lanes of a channel and the workgroups in index order; no
// atomics), so a run is reproducible.

// The four scored layers conv1, conv2, conv3, fc1 — the only statement of their geometry: first neuron in the mask, width, and the rows one workgroup step of the
// sums kernel covers (256 lanes, four channels per lane).  Selects, not a table: a lane-dependent l costs compares, never an indexed load of a by-value array.
struct a0_redo_layer { int lo, width, rps; };
A0_HD constexpr a0_redo_layer a0_redo_layer_at(int l) {
    return l == 0 ? a0_redo_layer{0, 32, 32} : l == 1 ? a0_redo_layer{32, 64, 16} : l == 2 ? a0_redo_layer{96, 64, 16} : a0_redo_layer{160, 512, 2};
}
static_assert(a0_redo_layer_at(3).lo + a0_redo_layer_at(3).width == A0_REDO_NEURONS, "the four layers fill the mask");
A0_D int a0_redo_layer_of(int i) { return i < a0_redo_layer_at(1).lo ? 0 : i < a0_redo_layer_at(2).lo ? 1 : i < a0_redo_layer_at(3).lo ? 2 : 3; }

// The workgroups that take part in a layer of `rows` rows when one workgroup step covers `rps` rows: about eight steps each, at most all of them — a function of
// the row count alone.  A short layer (fc1: B rows of 512) leaves few partials for the finish to read.
A0_D int a0_redo_groups(long long rows, int rps) {
    const long long g = ((rows + rps - 1) / rps + 7) / 8;
    return (int)(g < 1 ? 1 : g > A0_REDO_PARTIALS ? A0_REDO_PARTIALS : g);
}

// Layer L of N channels, channel-fastest: a lane owns four channels (one 16-byte load per row) of every (256 / (N / 4))-th row of its workgroup's rows, four
// loads in flight; one exchange through LDS per layer, after which lane ch adds its channel's lanes in index order.  out: this workgroup's A0_REDO_NEURONS partial sums.
template <int L>
A0_D void a0_redo_layer_sums(const float* __restrict__ X, long long rows, double* __restrict__ out, double (*sh)[4]) {
    constexpr int N = a0_redo_layer_at(L).width, N4 = N / 4, RPS = a0_redo_layer_at(L).rps;
    static_assert(RPS * N4 == 256, "a workgroup step is 256 lanes of four channels");
    const int tid = threadIdx.x, r = tid / N4, c = tid % N4, G = a0_redo_groups(rows, RPS);
    if ((int)blockIdx.x >= G) return;          // the whole workgroup: nobody waits at the barriers below
    const long long steps = (rows + RPS - 1) / RPS, per = (steps + G - 1) / G;
    const long long s0 = (long long)blockIdx.x * per, s1 = s0 + per < steps ? s0 + per : steps;
    const a0_f4* __restrict__ X4 = (const a0_f4*)X;
    double a[4] = {0.0, 0.0, 0.0, 0.0};
    long long s = s0;
    for (; s + 4 <= s1; s += 4) {
        a0_f4 x[4];
#pragma unroll
        for (int u = 0; u < 4; ++u) { const long long row = (s + u) * RPS + r; x[u] = row < rows ? X4[row * N4 + c] : a0_zero4(); }
#pragma unroll
        for (int u = 0; u < 4; ++u) { a[0] += (double)fabsf(x[u].x); a[1] += (double)fabsf(x[u].y); a[2] += (double)fabsf(x[u].z); a[3] += (double)fabsf(x[u].w); }
    }
    for (; s < s1; ++s) {
        const long long row = s * RPS + r;
        const a0_f4 x = row < rows ? X4[row * N4 + c] : a0_zero4();
        a[0] += (double)fabsf(x.x); a[1] += (double)fabsf(x.y); a[2] += (double)fabsf(x.z); a[3] += (double)fabsf(x.w);
    }
#pragma unroll
    for (int e = 0; e < 4; ++e) sh[tid][e] = a[e];
    __syncthreads();
    for (int ch = tid; ch < N; ch += 256) {
        double t = 0.0;
#pragma unroll
        for (int rr = 0; rr < RPS; ++rr) t += sh[rr * N4 + (ch >> 2)][ch & 3];
        out[a0_redo_layer_at(L).lo + ch] = t;
    }
    __syncthreads();
}

__global__ __launch_bounds__(256) void a0_redo_sums_kernel(const float* __restrict__ act1, long long rows1, const float* __restrict__ act2, long long rows2,
                                                           const float* __restrict__ act3, long long rows3, const float* __restrict__ fc1, long long rows4,
                                                           const int* __restrict__ state, int freq, int force, double* __restrict__ partials) {
    if (!a0_period_fires(state, freq, force)) return;
    __shared__ double sh[256][4];
    double* out = partials + (long long)blockIdx.x * A0_REDO_NEURONS;
    a0_redo_layer_sums<0>(act1, rows1, out, sh);
    a0_redo_layer_sums<1>(act2, rows2, out, sh);
    a0_redo_layer_sums<2>(act3, rows3, out, sh);
    a0_redo_layer_sums<3>(fc1, rows4, out, sh);
}

// One workgroup of 1024 lanes.  The partials of a neuron — those of the workgroups that took part in its layer — are added in index order in two steps, so that
// up to 512 dependent additions do not wait for as many loads one after the other: lane (slice s, neuron i) adds the s-th eighth of them (independent loads), then
// lane i adds its eight slice sums in index order.
__global__ __launch_bounds__(1024) void a0_redo_finish_kernel(const double* __restrict__ partials, long long rows1, long long rows2, long long rows3, long long rows4,
                                                              double tau, const int* __restrict__ state, int freq, int force, float* __restrict__ scores, int* __restrict__ mask,
                                                              int* __restrict__ counts) {
    if (!a0_period_fires(state, freq, force)) return;
    constexpr int SLICES = 8;
    __shared__ double part[SLICES][A0_REDO_NEURONS];
    __shared__ double m[A0_REDO_NEURONS];
    __shared__ double mean[4];
    __shared__ int dorm[A0_REDO_NEURONS];
    __shared__ int cnt[4];
    const int i = threadIdx.x, lay = a0_redo_layer_of(i);
    const int lo = a0_redo_layer_at(i).lo, width = a0_redo_layer_at(i).width;      // of layer i, for the lanes i < 4
    for (int item = threadIdx.x; item < SLICES * A0_REDO_NEURONS; item += 1024) {
        const int sl = item / A0_REDO_NEURONS, n = item - sl * A0_REDO_NEURONS, ln = a0_redo_layer_of(n);
        const int G = ln == 0 ? a0_redo_groups(rows1, a0_redo_layer_at(0).rps) : ln == 1 ? a0_redo_groups(rows2, a0_redo_layer_at(1).rps)
                    : ln == 2 ? a0_redo_groups(rows3, a0_redo_layer_at(2).rps) : a0_redo_groups(rows4, a0_redo_layer_at(3).rps);
        const int per = (G + SLICES - 1) / SLICES, g0 = sl * per, g1 = g0 + per < G ? g0 + per : G;
        double t = 0.0;
#pragma unroll 8
        for (int g = g0; g < g1; ++g) t += partials[(long long)g * A0_REDO_NEURONS + n];
        part[sl][n] = t;
    }
    __syncthreads();
    if (i < A0_REDO_NEURONS) {
        const long long rows = lay == 0 ? rows1 : lay == 1 ? rows2 : lay == 2 ? rows3 : rows4;
        double t = 0.0;
#pragma unroll
        for (int sl = 0; sl < SLICES; ++sl) t += part[sl][i];
        m[i] = t / (double)rows;
    }
    __syncthreads();
    if (i < 4) {
        double t = 0.0;
        for (int j = 0; j < width; ++j) t += m[lo + j];
        mean[i] = t / (double)width;
    }
    __syncthreads();
    if (i < A0_REDO_NEURONS) {
        const double s = mean[lay] > 0.0 ? m[i] / mean[lay] : 0.0;
        const int d = s <= tau ? 1 : 0;
        scores[i] = (float)s; mask[i] = d; dorm[i] = d;
    }
    __syncthreads();
    if (i < 4) {
        int c = 0;
        for (int j = 0; j < width; ++j) c += dorm[lo + j];
        cnt[i] = c; counts[i] = c;
    }
    __syncthreads();
    if (i == 0) { counts[4] = cnt[0] + cnt[1] + cnt[2] + cnt[3]; counts[5] = state ? state[1] : 0; }
}

extern "C" int a0_redo_score(const float* act1, long long rows1, const float* act2, long long rows2, const float* act3, long long rows3, const float* fc1, long long rows4,
                             double tau, const int* state, int freq, int force, double* partials, float* scores, int* mask, int* counts, void* stream) {
    if (!act1 || !act2 || !act3 || !fc1 || !partials || !scores || !mask || !counts || rows1 < 1 || rows2 < 1 || rows3 < 1 || rows4 < 1 || (!force && !state) || freq < 0)
        return a0_fail(A0_EINVAL, "a0_redo_score: bad argument");
    if (!(tau >= 0.0) || !(tau < 1.0)) return a0_fail(A0_EINVAL, "a0_redo_score: tau must lie in [0, 1)");
    if (!a0_aligned(16, act1, act2, act3, fc1)) return a0_fail(A0_EINVAL, "a0_redo_score: the activation buffers must be 16-byte aligned");
    if (!a0_aligned(8, partials) || !a0_aligned(4, scores, mask, counts)) return a0_fail(A0_EINVAL, "a0_redo_score: misaligned output");
    hipLaunchKernelGGL(a0_redo_sums_kernel, dim3(A0_REDO_PARTIALS), dim3(256), 0, (hipStream_t)stream, act1, rows1, act2, rows2, act3, rows3, fc1, rows4, state, freq, force, partials);
    hipLaunchKernelGGL(a0_redo_finish_kernel, dim3(1), dim3(1024), 0, (hipStream_t)stream, (const double*)partials, rows1, rows2, rows3, rows4, tau, state, freq, force,
                       scores, mask, counts);
    return a0_fail_hip((int)hipGetLastError(), "a0_redo_score");
}

// The recycle launch.  Blocks in flat order conv1, conv2, conv3, fc1, head; block b is [W (N x K) | bias (N)] at `off`; `in`: where its rows' neurons start in the
// mask (-1: the head, whose rows are no hidden neurons), `out`: where the neurons its columns read start (-1: conv1 reads pixels), column k reads neuron k % mod.
struct a0_redo_map { long long off[5]; int N[5], K[5], in[5], out[5], mod[5]; };

template <bool W>
__global__ __launch_bounds__(256) void a0_redo_recycle_kernel(float* __restrict__ p, float* __restrict__ m, float* __restrict__ v, long long n_adam, long long n_total, a0_reset_table T,
                                                              a0_redo_map D, const int* __restrict__ mask, unsigned long long seed_arg, const int* __restrict__ state, int freq,
                                                              int force, long long k_host, a0_wt_sink B) {
    if (!a0_period_fires(state, freq, force)) return;
    const long long k = a0_period_index(state, freq, force, k_host);
    __shared__ unsigned char dm[A0_REDO_NEURONS];
    for (int i = threadIdx.x; i < A0_REDO_NEURONS; i += 256) dm[i] = mask[i] != 0 ? 1 : 0;
    __syncthreads();
    const unsigned long long seed = a0_seed_vgpr(seed_arg);
    const unsigned long long base = (unsigned long long)k * (unsigned long long)n_total;
    const long long stride = (long long)gridDim.x * blockDim.x;
    for (long long e = (long long)blockIdx.x * blockDim.x + threadIdx.x; e < n_adam; e += stride) {
        bool incoming = false, outgoing = false;
#pragma nounroll
        for (int b = 0; b < 5; ++b) {      // uniform loads of the by-value map, as a0_reset_find walks its table
            const long long nw = (long long)D.N[b] * D.K[b], r = e - D.off[b];
            if (r < 0 || r >= nw + D.N[b]) continue;
            if (r >= nw) { incoming = D.in[b] >= 0 && dm[D.in[b] + (int)(r - nw)]; continue; }      // a bias: incoming only
            const int n = (int)((unsigned)r / (unsigned)D.K[b]), kk = (int)r - n * D.K[b];
            incoming = D.in[b] >= 0 && dm[D.in[b] + n];
            outgoing = D.out[b] >= 0 && dm[D.out[b] + kk % D.mod[b]];
        }
        if (!incoming && !outgoing) continue;
        // an element that is both (the weight from a dormant neuron into a dormant neuron) ends at zero: the outgoing rule is applied last, as in ReDo's published code
        float x = 0.f;
        if (!outgoing) {
            const a0_reset_rule R = a0_reset_find(T, 0.f, e, n_total);
            if (R.kind < 0) continue;                  // the table has no rule for it: left alone
            x = a0_reset_fresh1(R, seed, base + (unsigned long long)e, A0_STREAM_REDO);
        }
        p[e] = x; m[e] = 0.f; v[e] = 0.f;
        if constexpr (W) a0_tail_wt1(B, true, false, e, x);
    }
}

extern "C" int a0_redo_recycle(float* params, float* exp_avg, float* exp_avg_sq, long long n_adam, long long n_total, const a0_net_reset_seg* segs, int n_segs,
                               const a0_redo_blocks* blocks, const int* mask, unsigned long long seed, const int* state, int freq, int force, long long k_host,
                               const a0_encoder_weights* w, int C, float* wt, void* stream) {
    if (!params || !exp_avg || !exp_avg_sq || !blocks || !mask || n_adam < 1 || n_total < n_adam || (!force && !state) || freq < 0 || (force && k_host < 0) ||
        !a0_aligned(4, params, exp_avg, exp_avg_sq, mask))
        return a0_fail(A0_EINVAL, "a0_redo_recycle: bad argument");
    a0_reset_table T;
    if (int e = a0_reset_table_make(&T, "a0_redo_recycle", segs, n_segs, n_adam)) return e;
    if (blocks->K1 < 1 || blocks->feat < 64 || blocks->feat % 64 != 0 || blocks->Npad < 1) return a0_fail(A0_EINVAL, "a0_redo_recycle: K1 >= 1, feat a positive multiple of 64, Npad >= 1");
    a0_redo_map D;
    const long long off[5] = {blocks->conv1, blocks->conv2, blocks->conv3, blocks->fc1, blocks->head};
    const int K[5] = {blocks->K1, 512, 576, blocks->feat, 512};
    long long at = 0;
    for (int b = 0; b < 5; ++b) {      // block b < 4 holds layer b's neurons as rows; block b > 0 reads layer b - 1's as columns
        const int N = b < 4 ? a0_redo_layer_at(b).width : blocks->Npad;
        if (off[b] < at || off[b] + (long long)N * K[b] + N > n_adam) return a0_fail(A0_EINVAL, "a0_redo_recycle: the blocks conv1, conv2, conv3, fc1, head must be ascending, disjoint and inside [0, n_adam)");
        at = off[b] + (long long)N * K[b] + N;
        D.off[b] = off[b]; D.N[b] = N; D.K[b] = K[b];
        D.in[b] = b < 4 ? a0_redo_layer_at(b).lo : -1;
        D.out[b] = b > 0 ? a0_redo_layer_at(b - 1).lo : -1;
        D.mod[b] = b > 0 ? a0_redo_layer_at(b - 1).width : 1;
    }
    a0_wt_sink B{0, 0, 0, 0, 0, nullptr, nullptr};
    if (wt) {
        if (int e = a0_wt_sink_make(&B, "a0_redo_recycle", "params", params, n_total, w, C, nullptr, wt)) return e;
        if (B.o1 != blocks->conv1 || B.o2 != blocks->conv2 || B.o3 != blocks->conv3 || B.K1 != blocks->K1)
            return a0_fail(A0_EINVAL, "a0_redo_recycle: the encoder weights and the block descriptors name different convolution blocks");
        B.wt = wt; B.wt_t = nullptr;                   // the online copy alone: the target follows at its next sync or blend
    }
    const unsigned long long seed32 = seed & 0xFFFFFFFFull;
    hipLaunchKernelGGL(wt ? a0_redo_recycle_kernel<true> : a0_redo_recycle_kernel<false>, dim3(a0_grid_256(n_adam)), dim3(256), 0, (hipStream_t)stream, params, exp_avg, exp_avg_sq, n_adam,
                       n_total, T, D, mask, seed32, state, freq, force, k_host, B);
    return a0_fail_hip((int)hipGetLastError(), "a0_redo_recycle");
}
