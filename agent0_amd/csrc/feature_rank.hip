// Feature rank (learner.rank_freq; gfx950): srank_delta of Kumar et al. 2021 for the fc1 activations X [rows][512] of an update's differentiated pass, in two
// launches that decide for themselves as the ReDo launches do (a0_period_fires).  (1) G = X^T X on the fp64 matrix pipe, one 64 x 64 tile per workgroup, every
// product exact and every sum in a fixed order; (2) one workgroup: Householder tridiagonalisation of a copy of G, Sturm bisection for the 512 eigenvalues, the
// floor, the square roots, the ordered sums and the rank.  No atomics, no allocation, no host sync: the same bytes from run to run.
#include "a0_internal.h"

#include <cstdio>

#define A0_RANK_TILE 64                                      // a workgroup's tile of G
#define A0_RANK_TILES (A0_RANK_FEATURES / A0_RANK_TILE)      // 8 tile rows; the 36 tiles J >= I are computed, the rest is their mirror
#define A0_RANK_CHUNK 16                                     // rows of X staged per step
#define A0_RANK_LDS_STRIDE 80                                // floats between two staged rows: the four rows an MFMA operand reads fall into different banks

typedef double a0_d4 __attribute__((ext_vector_type(4)));

// ------------------------------------------------------------------------------------------------ launch 1: the Gram matrix
// 256 lanes = 2 x 2 waves, wave (wr, wc) owns the 32 x 32 quarter of tile (I, J) as 2 x 2 v_mfma_f64_16x16x4_f64 accumulators.  A step stages 16 rows of the tile's
// two column panels (one 16-byte load per lane and panel, rows past `rows` as zeros; the next step's loads are in flight during the MFMAs), then four MFMA rounds of
// four rows each: lane l feeds A[i = l & 15][k = l >> 4] = X[r + k][I-panel column i] and B[k][j = l & 15] = X[r + k][J-panel column j], converted to double.  A
// product of two fp32 values is exact in double; the additions happen in row order inside one accumulator.  An element (i, j) with j >= i is stored at [i][j] and
// [j][i] of both halves of `gram` (G, and the copy the second launch works in), so G is bitwise symmetric by construction.
__global__ __launch_bounds__(256) void a0_feature_gram_kernel(const float* __restrict__ X, long long rows, const int* __restrict__ state, int freq, int force,
                                                              double* __restrict__ gram) {
    if (!a0_period_fires(state, freq, force)) return;
    __shared__ float sA[A0_RANK_CHUNK * A0_RANK_LDS_STRIDE], sB[A0_RANK_CHUNK * A0_RANK_LDS_STRIDE];
    int I = 0, J = (int)blockIdx.x;
    while (J >= A0_RANK_TILES - I) { J -= A0_RANK_TILES - I; ++I; }      // the blockIdx.x-th pair of the upper triangle, row by row
    J += I;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, wr = wave >> 1, wc = wave & 1;
    const int srow = tid >> 4, scol = (tid & 15) * 4;                      // what this lane stages: 16 rows x 16 lanes x 4 floats per panel
    const float* __restrict__ XA = X + I * A0_RANK_TILE + scol;
    const float* __restrict__ XB = X + J * A0_RANK_TILE + scol;
    a0_d4 acc[2][2];
#pragma unroll
    for (int s = 0; s < 2; ++s)
#pragma unroll
        for (int t = 0; t < 2; ++t) acc[s][t] = a0_d4{0.0, 0.0, 0.0, 0.0};
    const long long chunks = (rows + A0_RANK_CHUNK - 1) / A0_RANK_CHUNK;
    a0_f4 ga = srow < rows ? *(const a0_f4*)(XA + (long long)srow * A0_RANK_FEATURES) : a0_zero4();
    a0_f4 gb = srow < rows ? *(const a0_f4*)(XB + (long long)srow * A0_RANK_FEATURES) : a0_zero4();
    const int k = lane >> 4, c = lane & 15;
    for (long long ch = 0; ch < chunks; ++ch) {
        __syncthreads();                                                   // the previous step's reads are done
        *(a0_f4*)(sA + srow * A0_RANK_LDS_STRIDE + scol) = ga;
        *(a0_f4*)(sB + srow * A0_RANK_LDS_STRIDE + scol) = gb;
        __syncthreads();
        const long long nr = (ch + 1) * A0_RANK_CHUNK + srow;
        ga = nr < rows ? *(const a0_f4*)(XA + nr * A0_RANK_FEATURES) : a0_zero4();
        gb = nr < rows ? *(const a0_f4*)(XB + nr * A0_RANK_FEATURES) : a0_zero4();
#pragma unroll
        for (int kk = 0; kk < A0_RANK_CHUNK / 4; ++kk) {
            const float* pa = sA + (kk * 4 + k) * A0_RANK_LDS_STRIDE + wr * 32 + c;
            const float* pb = sB + (kk * 4 + k) * A0_RANK_LDS_STRIDE + wc * 32 + c;
            const double a0 = (double)pa[0], a1 = (double)pa[16], b0 = (double)pb[0], b1 = (double)pb[16];
            acc[0][0] = __builtin_amdgcn_mfma_f64_16x16x4f64(a0, b0, acc[0][0], 0, 0, 0);
            acc[0][1] = __builtin_amdgcn_mfma_f64_16x16x4f64(a0, b1, acc[0][1], 0, 0, 0);
            acc[1][0] = __builtin_amdgcn_mfma_f64_16x16x4f64(a1, b0, acc[1][0], 0, 0, 0);
            acc[1][1] = __builtin_amdgcn_mfma_f64_16x16x4f64(a1, b1, acc[1][1], 0, 0, 0);
        }
    }
    // C/D of the f64 form: column = lane & 15, row = (lane >> 4) + 4 * reg
    double* __restrict__ work = gram + (long long)A0_RANK_FEATURES * A0_RANK_FEATURES;
#pragma unroll
    for (int s = 0; s < 2; ++s)
#pragma unroll
        for (int t = 0; t < 2; ++t)
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const int gi = I * A0_RANK_TILE + wr * 32 + s * 16 + k + 4 * r, gj = J * A0_RANK_TILE + wc * 32 + t * 16 + c;
                if (gj < gi) continue;                                     // the diagonal tiles' lower halves: written by their mirror elements
                const double g = acc[s][t][r];
                gram[gi * A0_RANK_FEATURES + gj] = g; gram[gj * A0_RANK_FEATURES + gi] = g;
                work[gi * A0_RANK_FEATURES + gj] = g; work[gj * A0_RANK_FEATURES + gi] = g;
            }
}

// ------------------------------------------------------------------------------------------------ launch 2: eigenvalues, floor, rank
#define A0_RANK_N A0_RANK_FEATURES
#define A0_RANK_BISECT_MAX 192      // a bisection ends when its interval is two neighbouring doubles, at the latest here (the Gershgorin interval halves to a denormal width long before)

// the sum of one double per lane over the 1024 lanes in a fixed order: xor-shuffles inside a wave, then the sixteen wave sums in index order (every lane gets it)
A0_D double a0_rank_block_sum(double x, double* red) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) x += __shfl_xor(x, o);
    __syncthreads();                                                       // red is free again
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = x;
    __syncthreads();
    double t = 0.0;
#pragma unroll
    for (int w = 0; w < 16; ++w) t += red[w];
    return t;
}

// Number of eigenvalues of the tridiagonal (d, e2 = e^2) below or at x: the Sturm sequence with LAPACK dstebz's safeguarded pivot.
A0_D int a0_rank_sturm(const double* d, const double* e2, double x, double pivmin) {
    double q = d[0] - x;
    if (fabs(q) < pivmin) q = -pivmin;
    int cnt = q <= 0.0 ? 1 : 0;
#pragma unroll 4
    for (int j = 1; j < A0_RANK_N; ++j) {
        q = d[j] - e2[j - 1] / q - x;
        if (fabs(q) < pivmin) q = -pivmin;
        cnt += q <= 0.0 ? 1 : 0;
    }
    return cnt;
}

// One workgroup of 1024 lanes; lane (h = tid >> 9, j = tid & 511) owns column j of the rows of parity h.  T = Q^T G Q by 510 Householder reflectors (LAPACK dsytd2's
// arithmetic on the full symmetric matrix, which stays in HBM / L2): step k has v (v[k + 1] = 1, zero up to k), tau and the raw product A v; it forms
// w = p - (tau / 2)(p . v) v, takes row k + 1 of A - v w^T - w v^T for the NEXT reflector, and then makes one pass over the rows behind k that applies the rank-2
// update and accumulates the next step's A v from the new values: the matrix is read and written once per step.  A lane only ever touches its own column, and its
// own parity's rows, except for that one row, which is read behind a barrier.  Bound (profiles/r29_feature_rank.md): the 2 MB matrix does not fit one CU's LDS, so
// the stage moves about 1.4 MB per step through one CU's path to L2 — 12.6 ms; more loads in flight per lane change nothing.  The bisection (3.7 - 5.7 ms) is
// bound by the latency of 511 dependent divisions per Sturm count.
__global__ __launch_bounds__(1024) void a0_feature_rank_kernel(double* __restrict__ gram, double delta, const int* __restrict__ state, int freq, int force,
                                                               double* __restrict__ spectrum, int* __restrict__ result) {
    if (!a0_period_fires(state, freq, force)) return;
    constexpr int N = A0_RANK_N;
    __shared__ double v[N], w[N], vn[N], pp[2][N], dd[N], ee[N], red[16];
    __shared__ double sh_scal[4], sh_alpha;
    __shared__ int sh_bad;
    const int tid = threadIdx.x, h = tid >> 9, j = tid & (N - 1);
    double* __restrict__ A = gram + (long long)N * N;
    // a diagonal element that is not finite: feature_rank = -1, nothing else is computed
    if (tid == 0) sh_bad = 0;
    __syncthreads();
    if (h == 0) { const double g = gram[j * N + j]; if (!(fabs(g) <= 1.79769313486231570815e308)) sh_bad = 1; }
    __syncthreads();
    if (sh_bad) {
        if (h == 0) spectrum[j] = 0.0;
        if (tid == 0) { result[0] = -1; result[1] = 0; result[2] = state ? state[1] : 0; }
        return;
    }

    // the reflector of step k from x = (row k of A behind the diagonal), LAPACK dlarfg: lanes h == 0 hold x_j (0 for j <= k); leaves v = vn, tau, e[k]
    auto reflector = [&](int k, double xj) -> double {
        const double xr = (h == 0 && j > k + 1) ? xj : 0.0;
        if (h == 0 && j == k + 1) sh_alpha = xj;                           // published by the barriers of the sum below
        const double xn2 = a0_rank_block_sum(xr * xr, red), alpha = sh_alpha;
        double tau = 0.0, scale = 0.0, beta = alpha;
        if (xn2 > 0.0) {
            const double nrm = sqrt(alpha * alpha + xn2);
            beta = alpha >= 0.0 ? -nrm : nrm;
            tau = (beta - alpha) / beta;
            scale = 1.0 / (alpha - beta);
        }
        if (h == 0) vn[j] = j <= k ? 0.0 : j == k + 1 ? 1.0 : xr * scale;
        if (tid == 0) ee[k] = beta;
        return tau;
    };

    // step 0's reflector and raw product
    if (tid == 0) dd[0] = A[0];
    double tau = reflector(0, h == 0 && j > 0 ? A[j] : 0.0);
    __syncthreads();
    {
        double acc = 0.0;
#pragma unroll 8
        for (int i = 1 + ((1 + h) & 1); i < N; i += 2) acc += A[i * N + j] * vn[i];      // rows of parity h behind row 0
        pp[h][j] = acc;
    }
    for (int k = 0; k < N - 2; ++k) {
        __syncthreads();                                                   // pp and vn of step k are complete
        const double vj = vn[j], pj = tau * (pp[0][j] + pp[1][j]);
        const double pv = a0_rank_block_sum(h == 0 ? pj * vj : 0.0, red);  // its barriers: every lane has read vn and pp
        const double a2 = -0.5 * tau * pv, wj = pj + a2 * vj;
        if (h == 0) { v[j] = vj; w[j] = wj; }
        __syncthreads();
        // row k + 1 of the updated matrix: the next diagonal element and the next reflector's x
        double xj = 0.0;
        if (h == 0 && j > k) {
#pragma clang fp contract(off)
            xj = A[(k + 1) * N + j] - (v[k + 1] * w[j] + w[k + 1] * v[j]);
        }
        if (h == 0 && j == k + 1) dd[k + 1] = xj;
        double tau_n = 0.0;
        if (k + 1 < N - 2) tau_n = reflector(k + 1, xj);
        else if (h == 0 && j == N - 1) ee[N - 2] = xj;                     // the last off-diagonal element
        __syncthreads();
        // the pass: rows i > k of parity h, column j > k; vn is zero up to row k + 1
        double acc = 0.0;
        if (j > k) {
            // per row: the rank-2 update with both products rounded (the two triangles stay mirror images), then the next step's product
#pragma unroll 8
            for (int i = k + 1 + ((k + 1 + h) & 1); i < N; i += 2) {
                double a;
                {
#pragma clang fp contract(off)
                    a = A[i * N + j] - (v[i] * wj + w[i] * vj);
                }
                A[i * N + j] = a;
                acc += a * vn[i];
            }
        }
        pp[h][j] = acc;
        tau = tau_n;
    }
    __syncthreads();
    if (tid == 0) dd[N - 1] = A[(N - 1) * N + (N - 1)];
    __syncthreads();

    // ---- bisection: lane i < 512 finds the i-th largest eigenvalue of (dd, ee)
    double* e2 = pp[0];
    double* lam = pp[1];
    if (h == 0) e2[j] = j < N - 1 ? ee[j] * ee[j] : 0.0;
    __syncthreads();
    if (tid == 0) {
        double gl = dd[0] - fabs(ee[0]), gu = dd[0] + fabs(ee[0]), emax = 0.0;
        for (int i = 1; i < N; ++i) {
            const double r = fabs(ee[i - 1]) + (i < N - 1 ? fabs(ee[i]) : 0.0);
            gl = fmin(gl, dd[i] - r); gu = fmax(gu, dd[i] + r);
        }
        for (int i = 0; i < N - 1; ++i) emax = fmax(emax, e2[i]);
        const double pivmin = 2.2250738585072014e-308 * fmax(1.0, emax), tnorm = fmax(fabs(gl), fabs(gu));
        const double widen = 2.1 * tnorm * 2.220446049250313e-16 * N + 4.2 * pivmin;
        sh_scal[0] = gl - widen; sh_scal[1] = gu + widen; sh_scal[2] = pivmin; sh_scal[3] = tnorm;
    }
    __syncthreads();
    if (h == 0) {
        double lo = sh_scal[0], hi = sh_scal[1];
        const double pivmin = sh_scal[2];
        const int want = N - j;                                            // the j-th largest: the smallest x with at least N - j eigenvalues at or below it
        if (sh_scal[3] == 0.0) lo = hi = 0.0;                              // the zero matrix: every eigenvalue is exactly 0
        for (int it = 0; it < A0_RANK_BISECT_MAX; ++it) {
            const double mid = lo + 0.5 * (hi - lo);
            if (!(mid > lo && mid < hi)) break;
            if (a0_rank_sturm(dd, e2, mid, pivmin) >= want) hi = mid; else lo = mid;
        }
        lam[j] = hi;
    }
    __syncthreads();
    // ---- floor, square roots, ordered sums, rank
    double* sg = v;
    if (h == 0) {
        const double l1 = lam[0], l = lam[j];
        const double s = (l > 0.0 && l > 0x1p-43 * l1) ? sqrt(l) : 0.0;      // 512 * 2^-52 = 2^-43
        sg[j] = s; spectrum[j] = s;
    }
    __syncthreads();
    if (tid == 0) {
        double total = 0.0;
        int pos = 0;
        for (int i = 0; i < N; ++i) { total += sg[i]; pos += sg[i] > 0.0 ? 1 : 0; }
        int rank = 0;
        if (total > 0.0) {
            const double need = 1.0 - delta;
            double part = 0.0;
            rank = N;
            for (int i = 0; i < N; ++i) {
                part += sg[i];
                if (part / total >= need) { rank = i + 1; break; }
            }
        }
        result[0] = rank; result[1] = pos; result[2] = state ? state[1] : 0;
    }
}

extern "C" int a0_feature_rank(const float* fc1, long long rows, double delta, const int* state, int freq, int force, double* gram, double* spectrum, int* result,
                               void* stream) {
    if (!fc1) return a0_fail(A0_EINVAL, "a0_feature_rank: fc1 is NULL");
    if (!gram) return a0_fail(A0_EINVAL, "a0_feature_rank: gram is NULL");
    if (!spectrum) return a0_fail(A0_EINVAL, "a0_feature_rank: spectrum is NULL");
    if (!result) return a0_fail(A0_EINVAL, "a0_feature_rank: result is NULL");
    if (!force && !state) return a0_fail(A0_EINVAL, "a0_feature_rank: state is NULL without force");
    if (rows < 1) return a0_fail(A0_EINVAL, "a0_feature_rank: rows < 1");
    if (freq < 0) return a0_fail(A0_EINVAL, "a0_feature_rank: freq < 0");
    if (!(delta > 0.0) || !(delta < 1.0)) {
        char msg[160];
        snprintf(msg, sizeof msg, "a0_feature_rank: delta = %g must lie in the open interval (0, 1)", delta);
        return a0_fail(A0_EINVAL, msg);
    }
    if (!a0_aligned(16, fc1)) return a0_fail(A0_EINVAL, "a0_feature_rank: fc1 must be 16-byte aligned");
    if (!a0_aligned(8, gram, spectrum)) return a0_fail(A0_EINVAL, "a0_feature_rank: gram and spectrum must be 8-byte aligned");
    if (!a0_aligned(4, result, state)) return a0_fail(A0_EINVAL, "a0_feature_rank: result and state must be 4-byte aligned");
    hipLaunchKernelGGL(a0_feature_gram_kernel, dim3(A0_RANK_TILES * (A0_RANK_TILES + 1) / 2), dim3(256), 0, (hipStream_t)stream, fc1, rows, state, freq, force, gram);
    hipLaunchKernelGGL(a0_feature_rank_kernel, dim3(1), dim3(1024), 0, (hipStream_t)stream, gram, delta, state, freq, force, spectrum, result);
    return a0_fail_hip((int)hipGetLastError(), "a0_feature_rank");
}
