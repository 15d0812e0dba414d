// Dense layers on gfx950: the exported a0_dense_* entry points over the HIP backend of net_impl.h, the weights-as-term-planes forms, and the split-K fc1 whose slabs a consumer
// kernel finishes (actor tails, head + loss kernels).  Every matrix-operand GEMM of the library is instantiated here.  Replaces the ATen -> cuBLAS dispatches behind reference
// agent0/deepq/model.py:112-114 / 144-146 / 203-216 (dense layers of the heads) and their autograd backward (agent.py:153-155).
#include "hip_backend.h"
#include "short_k_fwd.h"

void a0_hip_backend::short_k_fwd(const float* X, int ldx, const float* W, const float* b, const float* M, int group, float* Y, float* Y2, int R, int N, int relu) {
    A0_HIP_THROW(a0_short_k_fwd_launch(st, X, ldx, W, b, M, group, Y, Y2, R, N, relu));
}

// ------------------------------------------------------------------------------------------------ argument checks
// A0_OK, or A0_EINVAL behind "<who>: bad shape": R >= 1 and N, K, ldx multiples of 4 (an entry point without one passes 0); ok: the entry point's own tests; multiples: the message names the rule
static int a0_dense_shape_check(const char* who, bool ok, int R, int N, int K, int ldx, bool multiples = true) {
    if (ok && R >= 1 && !(N & 3) && !(K & 3) && !(ldx & 3)) return A0_OK;
    return a0_fail(A0_EINVAL, (std::string(who) + (multiples ? ": bad shape (N, K, ldx must be multiples of 4)" : ": bad shape")).c_str());
}
int a0_splits_check(const char* who, int splits, int K) {
    if (splits >= 1 && splits <= 64 && splits <= (K + 31) / 32) return A0_OK;
    return a0_fail(A0_EINVAL, (std::string(who) + ": splits must lie in [1, min(64, ceil(K / 32))]").c_str());
}

// ------------------------------------------------------------------------------------------------ forward
extern "C" long long a0_dense_fwd_scratch(int R, int N, int K) { return a0_dense_fwd_scratch_impl(R, N, K); }

extern "C" int a0_dense_fwd(const float* X, int ldx, const float* W, const float* b, float* Y, int R, int N, int K, int relu,
                            float* scratch, void* stream) {
    A0_TRY
    if (const int rc = a0_dense_shape_check("a0_dense_fwd", X && W && b && Y && N >= 4, R, N, K, ldx)) return rc;
    if (a0_dense_fwd_scratch_impl(R, N, K) > 0 && !scratch) return a0_fail(A0_EINVAL, "a0_dense_fwd: split-K needs scratch");
    a0_hip_backend bk{(hipStream_t)stream};
    a0_dense_fwd_impl(bk, X, ldx, W, b, Y, R, N, K, relu, scratch);
    return A0_OK;
    A0_CATCH
}

// a0_dense_fwd with the split count given by the caller (1 = unsplit): a grouped actor step runs each group's layers with the split count of the full batch's launch, so
// every row's sum is formed in the same order as in a one-group step.  a0_dense_fwd_splits tells the count a0_dense_fwd itself would use.
extern "C" int a0_dense_fwd_splits(int R, int N, int K) { return R < 1 ? 1 : a0_dense_fwd_splits_impl(R, N, K); }
extern "C" int a0_dense_fwd_n(const float* X, int ldx, const float* W, const float* b, float* Y, int R, int N, int K, int relu, int splits, float* scratch, void* stream) {
    A0_TRY
    if (const int rc = a0_dense_shape_check("a0_dense_fwd_n", X && W && b && Y && N >= 4, R, N, K, ldx)) return rc;
    if (const int rc = a0_splits_check("a0_dense_fwd_n", splits, K)) return rc;
    if (splits > 1 && !scratch) return a0_fail(A0_EINVAL, "a0_dense_fwd_n: split-K needs scratch (splits * R * N floats)");
    a0_hip_backend bk{(hipStream_t)stream};
    a0_dense_fwd_impl(bk, X, ldx, W, b, Y, R, N, K, relu, scratch, splits);
    return A0_OK;
    A0_CATCH
}

// ---- weights as term planes (round 6): W [N][K] fp32 -> the three bf16 term planes in OpPlanesKC's layout (igemm_x9.h), once per change of W; a0_dense_fwd_wplanes
// is a0_dense_fwd for unsplit shapes (a0_dense_fwd_scratch == 0) with whole k tiles (K % 32 == 0) reading them: the same exact terms, so the same result bit for bit.
__global__ void a0_split_planes_kernel(const a0_f4* __restrict__ W, uint32_t* __restrict__ planes, long long groups) {
    const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= groups) return;
    a0_x9_piece pc;
    pc.v = W[i];
#pragma unroll
    for (int e = 0; e < 4; ++e) pc.split(e);
    a0_u32x2g hi, mid, lo;
    pc.pack(hi, mid, lo);
    a0_u32x2g* o = (a0_u32x2g*)(planes + i * 6);
    o[0] = hi; o[1] = mid; o[2] = lo;
}
extern "C" long long a0_weight_planes_words(int N, int K) { return (long long)N * (K / 4) * 6; }
extern "C" int a0_split_planes(const float* W, unsigned int* planes, int N, int K, void* stream) {
    if (!W || !planes || N < 1 || K < 4 || (K & 3)) return a0_fail(A0_EINVAL, "a0_split_planes: bad argument (K a multiple of 4)");
    const long long groups = (long long)N * (K / 4);
    hipLaunchKernelGGL(a0_split_planes_kernel, dim3((unsigned)((groups + 255) / 256)), dim3(256), 0, (hipStream_t)stream, (const a0_f4*)W, planes, groups);
    return a0_fail_hip((int)hipGetLastError(), "a0_split_planes");
}
extern "C" int a0_dense_fwd_wplanes_ok(int R, int N, int K) {
    return (R >= 2048 && N >= 128 && !(N & 3) && !(K & 31) && a0_dense_fwd_splits_impl(R, N, K) == 1 && a0_gemm_mode(-1) != 0) ? 1 : 0;
}
extern "C" int a0_dense_fwd_wplanes(const float* X, int ldx, const unsigned int* Wplanes, const float* b, float* Y, int R, int N, int K, int relu, void* stream) {
    A0_TRY
    if (!X || !Wplanes || !b || !Y || (ldx & 3) || !a0_dense_fwd_wplanes_ok(R, N, K)) return a0_fail(A0_EINVAL, "a0_dense_fwd_wplanes: shapes a0_dense_fwd_wplanes_ok accepts");
    hipStream_t st = (hipStream_t)stream;
    const a0_mat_src a{X, ldx};
    const a0_planes_src bw{Wplanes, K / 4};
    const EpiBiasAct::Params e{Y, b, N, relu};
    // unsplit matrix operands; its own tile is the 128 x 128 one, whatever the count of tiles
    switch (a0_gemm_tile_class(R, N, K, 1, true, true, false, false)) {
    case A0_TILE_HUGE: a0_x9_probed<OpMatKC, OpPlanesKC, EpiBiasAct, 4, 2, 2, 2, 1>(st, A0_TAG_DENSE_FWD, a, bw, e, R, N, K, 1); break;
    case A0_TILE_BIG: case A0_TILE_OWN: a0_x9_probed<OpMatKC, OpPlanesKC, EpiBiasAct, 4, 2, 1, 2>(st, A0_TAG_DENSE_FWD, a, bw, e, R, N, K, 1); break;
    case A0_TILE_FP32: break;      // a0_dense_fwd_wplanes_ok: the split-operand mode only
    }
    return A0_OK;
    A0_CATCH
}

// Y[r][:] = act(X[r] W^T + b) * M[r / group][:] — the quantile networks' embedding times the state features in the GEMM's epilogue
// (reference model.py:244-247: relu(cosine_emb(cos(pi i tau))) * features), for passes that are not differentiated: the embedding never
// goes to HBM and the Hadamard pass disappears.  Only for shapes whose forward GEMM is not split (a0_dense_fwd_scratch == 0).
extern "C" int a0_dense_fwd_mul(const float* X, int ldx, const float* W, const float* b, const float* M, int group, float* Y, int R, int N, int K, int relu, void* stream) {
    A0_TRY
    if (const int rc = a0_dense_shape_check("a0_dense_fwd_mul", X && W && b && M && Y && group >= 1, R, N, K, ldx)) return rc;
    if (a0_dense_fwd_splits_impl(R, N, K) != 1) return a0_fail(A0_EINVAL, "a0_dense_fwd_mul: this shape runs as a split GEMM; use a0_dense_fwd + a0_hadamard_fwd");
    a0_hip_backend bk{(hipStream_t)stream};
    bk.tag = A0_TAG_DENSE_FWD;
    if (a0_short_k_shape(R, N, K, ldx)) { bk.short_k_fwd(X, ldx, W, b, M, group, Y, nullptr, R, N, relu); return A0_OK; }
    a0_mat_src a{X, ldx};
    a0_mat_src bw{W, K};
    EpiBiasActMul::Params e{Y, b, N, relu, M, group, a0_udiv_magic((unsigned)group)};
    if (N <= 32) bk.template igemm<OpMatKC, OpMatKC, EpiBiasActMul, 4, 1, 1, 1>(a, bw, e, R, N, K, 1);
    else bk.template igemm<OpMatKC, OpMatKC, EpiBiasActMul, 4, 1, 1, 2>(a, bw, e, R, N, K, 1);
    return A0_OK;
    A0_CATCH
}

// The same for a pass that IS differentiated: E = act(X W^T + b) is kept for the backward pass (a0_hadamard_bwd) and Y = E * M[r / group] is
// written beside it in the same launch (a0_dense_fwd + a0_hadamard_fwd without re-reading E).  Only for the shapes of the short-reduction
// kernel: a0_dense_fwd_mul_keep_ok tells.
extern "C" int a0_dense_fwd_mul_keep_ok(int R, int N, int K, int ldx) { return a0_short_k_shape(R, N, K, ldx) ? 1 : 0; }

extern "C" int a0_dense_fwd_mul_keep(const float* X, int ldx, const float* W, const float* b, const float* M, int group, float* E, float* Y, int R, int N, int K, int relu, void* stream) {
    A0_TRY
    if (const int rc = a0_dense_shape_check("a0_dense_fwd_mul_keep", X && W && b && M && E && Y && group >= 1, R, N, 0, 0, false)) return rc;      // (K, ldx: below)
    if (!a0_short_k_shape(R, N, K, ldx)) return a0_fail(A0_EINVAL, "a0_dense_fwd_mul_keep: not a short-reduction shape (a0_dense_fwd_mul_keep_ok); use a0_dense_fwd + a0_hadamard_fwd");
    a0_hip_backend bk{(hipStream_t)stream};
    bk.tag = A0_TAG_DENSE_FWD;
    bk.short_k_fwd(X, ldx, W, b, M, group, E, Y, R, N, relu);
    return A0_OK;
    A0_CATCH
}

// The split-K GEMM of a0_dense_fwd WITHOUT its reduction: slab z = X W^T over the z-th k range, [R][N] each at stride R*N; the caller's
// next kernel sums the slabs (a0_dqn_head_loss_slabs, a0_actor_qhead).  Returns the slab count.
// Tile of the split-K fc1 GEMM whose slabs a consumer kernel finishes (actor tail, DQN head + loss): 64 x 64 up to 256 rows (the actor's
// batch: 8 slabs instead of 16 for the tail kernel to sum, GEMM + tail 19.9 vs 22.3 us at 256 rows; the eight-wave tiles need 16 slabs
// there and lose), 128 x 64 on EIGHT waves above (two per SIMD: one wave's staging work in the shadow of the other's MFMAs; 512 rows: GEMM + tail
// 26.5 vs 27.8 us on four waves, whole B = 512 update 380 vs 385 us) — profiles/r02_encoder_experiments.md.
static inline bool a0_fc1_small(int R) { return R <= 256; }
static inline int a0_fc1_splits(int R, int N, int K) {
    const int bx = a0_fc1_small(R) ? 64 : 128, by = 64;
    const int blocks = ((R + bx - 1) / bx) * ((N + by - 1) / by);
    int splits = blocks < 256 ? 256 / blocks : 1;      // about 256 workgroups
    const int maxs = (K / 32) / 2;
    if (splits > maxs) splits = maxs;
    if (splits > 64) splits = 64;
    return splits < 1 ? 1 : splits;
}

extern "C" int a0_dense_fwd_partial_slabs(int R, int N, int K) {
    const int s = N <= 32 ? a0_dense_fwd_splits_impl(R, N, K) : a0_fc1_splits(R, N, K);
    return s < 1 ? 1 : s;
}

static int a0_dense_fwd_partial_run(const float* X, int ldx, const float* W, int R, int N, int K, int splits, float* slabs, hipStream_t st) {
    a0_hip_backend bk{st};
    a0_mat_src a{X, ldx};
    a0_mat_src bw{W, K};
    EpiSlab::Params ep{slabs, (long long)R * N, N};
    bk.tag = A0_TAG_DENSE_FWD;
    if (N <= 32) bk.igemm<OpMatKC, OpMatKC, EpiSlab, 4, 1, 1, 1>(a, bw, ep, R, N, K, splits);
    else if (a0_fc1_small(R)) bk.igemm<OpMatKC, OpMatKC, EpiSlab, 2, 2, 1, 1>(a, bw, ep, R, N, K, splits);      // 64 x 64
    else bk.igemm<OpMatKC, OpMatKC, EpiSlab, 4, 2, 1, 1>(a, bw, ep, R, N, K, splits);                           // 128 x 64, eight waves
    return A0_OK;
}

// (no range check on its own count: a0_fc1_splits' exceeds ceil(K / 32) for small K)
extern "C" int a0_dense_fwd_partial(const float* X, int ldx, const float* W, int R, int N, int K, float* slabs, void* stream) {
    A0_TRY
    if (const int rc = a0_dense_shape_check("a0_dense_fwd_partial", X && W && slabs, R, N, K, ldx)) return rc;
    return a0_dense_fwd_partial_run(X, ldx, W, R, N, K, a0_dense_fwd_partial_slabs(R, N, K), slabs, (hipStream_t)stream);
    A0_CATCH
}

// a0_dense_fwd_partial with the split count given by the caller (the slab buffer holds splits * R * N floats): see a0_dense_fwd_n
extern "C" int a0_dense_fwd_partial_n(const float* X, int ldx, const float* W, int R, int N, int K, int splits, float* slabs, void* stream) {
    A0_TRY
    if (const int rc = a0_dense_shape_check("a0_dense_fwd_partial_n", X && W && slabs, R, N, K, ldx)) return rc;
    if (const int rc = a0_splits_check("a0_dense_fwd_partial_n", splits, K)) return rc;
    return a0_dense_fwd_partial_run(X, ldx, W, R, N, K, splits, slabs, (hipStream_t)stream);
    A0_CATCH
}

// n = 2 or 3 passes of one dense layer shape — X[i] [R][ldx] x W[i]^T [N][K] -> slabs[i] [splits][R][N] — as ONE launch (a0_igemm_x9_group_kernel): the chip is
// filled with a half / a third of the splits a single pass needs, so every workgroup's k loop is that much longer and the fixed cost of a launch is paid once.  The
// slabs differ from a0_dense_fwd_partial's (fewer, deeper partial sums: another association of the same fp32 additions); a0_dense_fwd_partial_multi_slabs tells the
// consumer how many there are.  Split-operand GEMM mode only.
static int a0_fwd_multi_splits(int n, int R, int N, int K) {
    const int blocks = n * ((R + 127) / 128) * ((N + 63) / 64);
    int splits = blocks < 256 ? 256 / blocks : 1;
    const int maxs = (K / 32) / 2;
    if (splits > maxs) splits = maxs;
    return splits < 1 ? 1 : splits;
}
extern "C" int a0_dense_fwd_partial_multi_ok(int n, int R, int N, int K) {
    return (a0_gemm_mode(-1) != 0 && (n == 2 || n == 3) && R >= 257 && R <= 4096 && N > 32 && !(N & 3) && !(K & 3)) ? 1 : 0;
}
extern "C" int a0_dense_fwd_partial_multi_slabs(int n, int R, int N, int K) { return a0_fwd_multi_splits(n, R, N, K); }

extern "C" int a0_dense_fwd_partial_multi(int n, const float* const* X, int ldx, const float* const* W, int R, int N, int K, float* const* slabs, const long long* slab_stride,
                                          void* stream) {
    A0_TRY
    if (!X || !W || !slabs || (ldx & 3) || !a0_dense_fwd_partial_multi_ok(n, R, N, K)) return a0_fail(A0_EINVAL, "a0_dense_fwd_partial_multi: shapes a0_dense_fwd_partial_multi_ok accepts");
    a0_x9_group<OpMatKC, OpMatKC, EpiSlab> grp;
    for (int i = 0; i < 3; ++i) {
        const int j = i < n ? i : 0;
        if (!X[j] || !W[j] || !slabs[j]) return a0_fail(A0_EINVAL, "a0_dense_fwd_partial_multi: null operand");
        grp.pa[i] = a0_mat_src{X[j], ldx};
        grp.pb[i] = a0_mat_src{W[j], K};
        // slab_stride (optional): floats between a pass's consecutive slabs — two passes may interleave their rows in one buffer [splits][2R][N] (stride 2 R N, bases R N apart)
        const long long stride = slab_stride ? slab_stride[j] : (long long)R * N;
        if (stride < (long long)R * N || (stride & 3)) return a0_fail(A0_EINVAL, "a0_dense_fwd_partial_multi: slab stride");
        grp.pe[i] = EpiSlab::Params{slabs[j], stride, N};
    }
    const int splits = a0_fwd_multi_splits(n, R, N, K);
    hipEvent_t e0 = nullptr, e1 = nullptr;
    const bool probe = a0_probe_events(A0_TAG_DENSE_FWD, &e0, &e1);
    A0_HIP_THROW((a0_igemm_x9_group_launch<OpMatKC, OpMatKC, EpiSlab, 4, 2, 1, 1>((hipStream_t)stream, n, grp, R, N, K, splits, e0, e1)));      // 128 x 64 tiles, eight waves
    if (probe) a0_probe_commit(2.0 * n * (double)R * (double)N * (double)K);
    return A0_OK;
    A0_CATCH
}

// a0_dense_fwd for the c51 / qr actors' fc1 over pre-split weights: the split GEMM's slabs from a0_actor_fc1_n (the split count a0_dense_fwd takes), then a0_dense_fwd's own
// reduction launch (slab sum in order + bias + ReLU)
extern "C" int a0_actor_fc1_dense_ok(int R, int N, int K) {
    return (a0_actor_fc1_ok(R, N, K) && a0_dense_fwd_splits_impl(R, N, K) > 1) ? 1 : 0;
}
extern "C" int a0_actor_fc1_dense(const float* X, int ldx, const unsigned int* planes, const float* b, float* Y, int R, int N, int K, int relu, float* scratch, void* stream) {
    A0_TRY
    if (!b || !Y || !scratch || !a0_actor_fc1_dense_ok(R, N, K)) return a0_fail(A0_EINVAL, "a0_actor_fc1_dense: shapes a0_actor_fc1_dense_ok accepts");
    const int splits = a0_dense_fwd_splits_impl(R, N, K);
    const int rc = a0_actor_fc1_n(X, ldx, planes, R, N, K, splits, scratch, stream);
    if (rc != A0_OK) return rc;
    a0_reduce_bias_act_launch((hipStream_t)stream, scratch, (long long)R * N, splits, b, Y, R, N, relu);
    return A0_OK;
    A0_CATCH
}

// fc1 of a scalar-head actor step (a0_internal.h)
int a0_actor_fc1_slabs(const float* feat, int K, const float* W1, const unsigned int* w1_planes, int E, int splits, float* scratch, hipStream_t st) {
    if (w1_planes && a0_actor_fc1_ok(E, 512, K)) return a0_actor_fc1_n(feat, K, w1_planes, E, 512, K, splits, scratch, (void*)st);
    return a0_dense_fwd_partial_run(feat, K, W1, E, 512, K, splits, scratch, st);
}

// ------------------------------------------------------------------------------------------------ backward
extern "C" int a0_dense_dgrad(const float* dY, const float* W, const float* act_mask, float* dX, int R, int N, int K, void* stream) {
    A0_TRY
    if (const int rc = a0_dense_shape_check("a0_dense_dgrad", dY && W && dX, R, N, K, 0, false)) return rc;      // (no ldx: dY and W are packed)
    a0_hip_backend bk{(hipStream_t)stream};
    a0_dense_dgrad_impl(bk, dY, W, act_mask, dX, R, N, K);
    return A0_OK;
    A0_CATCH
}

// a0_dense_dgrad(dY, W, no mask) + a0_hadamard_bwd in ONE launch (round 6): dx = dY W [R][K] is consumed in the GEMM's epilogue (EpiHadamard) and never written — R = B * n rows,
// n = 32 or 64 fractions per sample, R a multiple of 256 (whole 256 x 128 tiles along the rows: a wave's 64 rows are whole samples), N (the reduction, fc1's 512) a multiple of 16.
// demb is bit-identical to the two calls' (the same accumulators times the same features); d3 sums the sample's rows in the tile's register order instead of row by row
// (fp32 rounding: 1e-7 of the accumulated magnitude).
extern "C" int a0_dense_dgrad_hadamard_ok(int R, int N, int K, int n) {
    return (a0_gemm_mode(-1) != 0 && (n == 32 || n == 64) && R >= 4096 && !(R & 255) && !(R % n) && !(N & 15) && N >= 64 && !(K & 3) && K >= 128) ? 1 : 0;
}
extern "C" int a0_dense_dgrad_hadamard(const float* dY, const float* W, const float* emb, const float* feat, float* demb, float* d3, int R, int N, int K, int n, void* stream) {
    A0_TRY
    if (!dY || !W || !emb || !feat || !demb || !d3 || !a0_dense_dgrad_hadamard_ok(R, N, K, n)) return a0_fail(A0_EINVAL, "a0_dense_dgrad_hadamard: shapes a0_dense_dgrad_hadamard_ok accepts");
    const a0_mat_src a{dY, N};
    const a0_mat_src bw{W, K};
    const EpiHadamard::Params e{emb, feat, demb, d3, K, n};
    a0_x9_probed<OpMatKC, OpMatXC, EpiHadamard, 4, 2, 2, 2, 1>((hipStream_t)stream, A0_TAG_DENSE_DGRAD, a, bw, e, R, K, N, 1);
    return A0_OK;
    A0_CATCH
}

// a0_dense_dgrad (with the ReLU mask) and the unsplit a0_dense_wgrad of ONE layer — same dY, R x N x K with as many 64 x 64 tiles in the data gradient (R x K) as in the
// weight gradient (N x K): N == R — as one launch (a0_igemm_x9_pair_kernel).  fc1 of a 512-row batch: dX = (dY W) * (X > 0) into dX, dW = dY^T X (+ bias row sums) into grad.
// Bit-identical to the two calls.  Shapes: a0_dense_dgrad_wgrad_ok.
// (the class is stated in the tiles of the single-problem paths it must equal: fewer than 256 tiles of 128 x 64 in the data gradient, so that a0_dense_dgrad runs 64 x 64
// tiles, and at least 256 tiles of 64 x 64 in the weight gradient, so that a0_dense_wgrad is unsplit; within it the launch's own 128 x 128 tiles number at most
// 2 x 128 + the head's, and 2 x 100 + 4 for fc1)
// the tile of the fc1 backward launches (pair and trio): four by two waves of A0_FC1_MT x A0_FC1_NT blocks of 32 x 32
static constexpr int A0_FC1_MT = 1, A0_FC1_NT = 2;
static constexpr int A0_FC1_BX = 128 * A0_FC1_MT, A0_FC1_BY = 64 * A0_FC1_NT;
extern "C" int a0_dense_dgrad_wgrad_ok(int R, int N, int K) {
    const long long b128 = (long long)((R + 127) / 128) * ((K + 63) / 64), b64 = (long long)((N + 63) / 64) * ((K + 63) / 64);
    return (a0_gemm_mode(-1) != 0 && !a0_probe_active() && R == N && R >= 1 && R <= 1024 && !(N & 3) && !(K & 3) && b128 < 256 && b64 >= 256 && N >= 512 &&
            !a0_x9_big_round((long long)((R + 127) / 128) * ((K + 127) / 128))) ? 1 : 0;
}
// (round 5) a second class of shapes: SMALL layers whose two gradients together fit one round of 64 x 64 tiles — the head of a distributional learner at a 512-row batch
// (c51: 64 + 32 tiles, qr: 64 + 104).  Alone, the data gradient occupies a quarter of the chip for its whole k loop and the weight gradient follows it; side by side
// the launch lasts as long as the longer of the two.  The weight gradient is then an UNSPLIT sum on the bf16 pipe (a0_dense_wgrad: slabs on the fp32 pipe).
static int a0_dense_dgrad_wgrad_small_ok(int R, int N, int K) {
    const long long t1 = (long long)((R + 63) / 64) * ((K + 63) / 64), t2 = (long long)((N + 63) / 64) * ((K + 63) / 64);
    return (a0_gemm_mode(-1) != 0 && !a0_probe_active() && R >= 64 && R <= 1024 && N >= 64 && !(N & 3) && !(K & 3) && t1 + t2 <= 256 && t2 >= 16) ? 1 : 0;
}
extern "C" int a0_dense_dgrad_wgrad_ok2(int R, int N, int K) { return (a0_dense_dgrad_wgrad_ok(R, N, K) || a0_dense_dgrad_wgrad_small_ok(R, N, K)) ? 1 : 0; }
extern "C" int a0_dense_dgrad_wgrad(const float* dY, const float* W, const float* X, int ldx, float* dX, float* grad, int R, int N, int K, void* stream) {
    A0_TRY
    if (!dY || !W || !X || !dX || !grad || ldx < K || (ldx & 3) || !a0_dense_dgrad_wgrad_ok2(R, N, K)) return a0_fail(A0_EINVAL, "a0_dense_dgrad_wgrad: shapes a0_dense_dgrad_wgrad_ok2 accepts");
    a0_mat_src a1{dY, N}, b1{W, K};                          // data gradient: rows r, reduction over n
    EpiMaskMat::Params e1{dX, X, K};
    a0_mat_src a2{dY, N}, b2{X, ldx};                        // weight gradient: rows n, reduction over r
    EpiWgradSlab::Params e2{grad, 0, K, (long long)N * K};
    if (!a0_dense_dgrad_wgrad_ok(R, N, K)) {                 // the small class: 64 x 64 tiles, four waves, unequal tile counts
        A0_HIP_THROW((a0_igemm_x9_pair_launch<OpMatKC, OpMatXC, EpiMaskMat, OpMatXC, OpMatXC, EpiWgradSlab, 2, 2, 1, 1>((hipStream_t)stream, a1, b1, e1, R, K, N, a2, b2, e2, N, K, R)));
        return A0_OK;
    }
    // 128 x 128 tiles on eight waves, two 32 x 32 blocks per wave (A0_FC1_MT x A0_FC1_NT): fc1 of a 512-row batch is 100 + 100 workgroups of 120 KB of LDS, one per CU, ALL
    // resident at once — the 128 x 64 tile before it needed two rounds of workgroups (196 + 196 on 256 CUs, the second 56 % full) and paid ramp, prologue and epilogue twice
    // (profiles/r17_fc1_backward.md; the 256 x 64 tile was measured too and is slower).  The same sums as the 64 x 64 tiles of the separate calls: every output element's k
    // loop is the same sequence of MFMAs, and the bias gradient's 16 partial sums have the same members (BX = 128 on 512 threads, as before).
    A0_HIP_THROW((a0_igemm_x9_pair_launch<OpMatKC, OpMatXC, EpiMaskMat, OpMatXC, OpMatXC, EpiWgradSlab, 4, 2, A0_FC1_MT, A0_FC1_NT>((hipStream_t)stream, a1, b1, e1, R, K, N, a2, b2, e2, N, K, R)));
    return A0_OK;
    A0_CATCH
}

// a0_dense_dgrad_wgrad plus the NEXT layer's weight gradient in the same launch (round 5): with dY = d loss / d fc1's output and dY2 = d loss / d head's output both
// final (the head / loss kernel writes them), fc1's data gradient, fc1's weight gradient and the head's weight gradient dW2 = dY2^T X2 (+ bias row sums) into grad2
// [N2 x K2 | N2] are independent; the head's few tiles ride in the pair's launch (a0_igemm_x9_trio_kernel).  grad2 gets an UNSPLIT sum over the R rows on the bf16 pipe
// (a0_dense_wgrad splits it into slabs on the fp32 pipe: the same sum up to the association order).  Shapes: a0_dense_dgrad_wgrad_ok(R, N, K), X2 rows of R, ldx2 >= K2.
// where it pays: heads of at most 128 rows over at most 512 columns (scalar heads: four of the launch's 128 x 128 tiles).  Measured with wider heads in the launch
// (same box, alternating, 128 x 64 tiles): c51's 16 tiles
// 14.47 - 14.50 -> 14.57 ms, qr's 56 tiles 12.13 -> 12.16 ms — there the fp32-pipe split launch of its own stays; dqn 9.97 -> 9.85 ms, mdqn 11.69 -> 11.60.
extern "C" int a0_dense_dgrad_wgrad2_ok(int R, int N, int K, int N2, int K2) {
    return (a0_dense_dgrad_wgrad_ok(R, N, K) && N2 >= 4 && !(N2 & 3) && N2 <= 128 && K2 >= 4 && !(K2 & 3) && K2 <= 512) ? 1 : 0;
}
extern "C" int a0_dense_dgrad_wgrad2(const float* dY, const float* W, const float* X, int ldx, float* dX, float* grad, int R, int N, int K,
                                     const float* dY2, const float* X2, int ldx2, float* grad2, int N2, int K2, void* stream) {
    A0_TRY
    if (!dY || !W || !X || !dX || !grad || ldx < K || (ldx & 3) || !a0_dense_dgrad_wgrad_ok(R, N, K)) return a0_fail(A0_EINVAL, "a0_dense_dgrad_wgrad2: shapes a0_dense_dgrad_wgrad_ok accepts");
    if (!dY2 || !X2 || !grad2 || N2 < 4 || (N2 & 3) || K2 < 4 || (K2 & 3) || ldx2 < K2 || (ldx2 & 3) ||
        (long long)((N2 + A0_FC1_BX - 1) / A0_FC1_BX) * ((K2 + A0_FC1_BY - 1) / A0_FC1_BY) > (long long)((R + A0_FC1_BX - 1) / A0_FC1_BX) * ((K + A0_FC1_BY - 1) / A0_FC1_BY))
        return a0_fail(A0_EINVAL, "a0_dense_dgrad_wgrad2: the second layer's weight gradient must have no more tiles than the first layer's data gradient");
    a0_mat_src a1{dY, N}, b1{W, K};
    EpiMaskMat::Params e1{dX, X, K};
    a0_mat_src a2{dY, N}, b2{X, ldx};
    EpiWgradSlab::Params e2{grad, 0, K, (long long)N * K};
    a0_mat_src a3{dY2, N2}, b3{X2, ldx2};
    EpiWgradSlab::Params e3{grad2, 0, K2, (long long)N2 * K2};
    A0_HIP_THROW((a0_igemm_x9_trio_launch<OpMatKC, OpMatXC, EpiMaskMat, OpMatXC, OpMatXC, EpiWgradSlab, 4, 2, A0_FC1_MT, A0_FC1_NT>((hipStream_t)stream, a1, b1, e1, R, K, N, a2, b2, e2, N, K, R,
                                                                                                                  a3, b3, e3, N2, K2, R)));
    return A0_OK;
    A0_CATCH
}

extern "C" long long a0_dense_wgrad_scratch(int R, int N, int K) { return a0_dense_wgrad_scratch_impl(R, N, K); }

extern "C" int a0_dense_wgrad(const float* dY, const float* X, int ldx, float* grad, int R, int N, int K, float* slabs, void* stream) {
    A0_TRY
    if (const int rc = a0_dense_shape_check("a0_dense_wgrad", dY && X && grad, R, N, K, ldx, false)) return rc;
    if (a0_dense_wgrad_scratch_impl(R, N, K) > 0 && !slabs) return a0_fail(A0_EINVAL, "a0_dense_wgrad: needs slab scratch");
    a0_hip_backend bk{(hipStream_t)stream};
    a0_dense_wgrad_impl(bk, dY, X, ldx, grad, R, N, K, slabs);
    return A0_OK;
    A0_CATCH
}

// Up to four dense weight gradients whose slab reductions share ONE launch (head + fc1 [+ cosine embedding]): layer i uses
// slabs + slab_off[i] (a0_dense_wgrad_scratch(R[i], N[i], K[i]) floats each).  Same results as four a0_dense_wgrad calls.
extern "C" int a0_dense_wgrad_multi(int n, const float* const* dY, const float* const* X, const int* ldx, float* const* grad, const int* R, const int* N, const int* K,
                                    float* slabs, const long long* slab_off, a0_pending_reduce* pend, void* stream) {
    A0_TRY
    if (n < 1 || n > 4 || !dY || !X || !ldx || !grad || !R || !N || !K || !slab_off) return a0_fail(A0_EINVAL, "a0_dense_wgrad_multi: 1..4 layers");
    a0_hip_backend bk{(hipStream_t)stream};
    a0_reduce_seg segs[4];
    int nseg = 0;
    for (int i = 0; i < n; ++i) {
        if (const int rc = a0_dense_shape_check("a0_dense_wgrad_multi", dY[i] && X[i] && grad[i], R[i], N[i], K[i], ldx[i], false)) return rc;
        if (a0_dense_wgrad_scratch_impl(R[i], N[i], K[i]) > 0 && !slabs) return a0_fail(A0_EINVAL, "a0_dense_wgrad_multi: needs slab scratch");
        a0_reduce_seg seg;
        a0_dense_wgrad_impl(bk, dY[i], X[i], ldx[i], grad[i], R[i], N[i], K[i], slabs ? slabs + slab_off[i] : nullptr, &seg);
        if (seg.nslab > 0) segs[nseg++] = seg;
    }
    if (pend) {        // left to the next a0_net_encoder_wgrad(..., pend, ...)
        if (pend->n < 0 || pend->n + nseg > 4) return a0_fail(A0_EINVAL, "a0_dense_wgrad_multi: more than four pending reductions");
        for (int k = 0; k < nseg; ++k) pend->seg[pend->n++] = segs[k];
    } else if (nseg > 0) bk.reduce_segments(segs, nseg);
    return A0_OK;
    A0_CATCH
}
