// The HIP backend of net_impl.h: which kernel one implicit GEMM runs on, the probe around it, and the launchers of the fused weight gradients and the slab
// reductions.  net.hip instantiates it over the encoder's operands, dense.hip over matrix operands: no instantiation is shared, and nothing here is a kernel.
#pragma once
#include "igemm_x9.h"
#include "a0_internal.h"
#include "net_impl.h"

// reduce.hip: the slab reductions behind the backend's members of the same names
void a0_reduce_slabs_launch(hipStream_t st, const float* slabs, long long slab_stride, int nslab, float* out, long long count);
void a0_reduce_segments_launch(hipStream_t st, const a0_reduce_seg* segs, int nseg);
void a0_reduce_bias_act_launch(hipStream_t st, const float* slabs, long long slab_stride, int nslab, const float* bias, float* out, int rows, int N, int relu);

template <class OP> struct a0_is_mat { static constexpr bool value = false; };
template <> struct a0_is_mat<OpMatKC> { static constexpr bool value = true; };
template <> struct a0_is_mat<OpMatXC> { static constexpr bool value = true; };
// im2col-gathered B operands (conv weight gradients): their address arithmetic already fills the issue slots the splits would need
template <class OP> struct a0_is_gather { static constexpr bool value = false; };
template <> struct a0_is_gather<OpActXC> { static constexpr bool value = true; };

// The launch an X x Y x K problem in `splits` gets: 256 x 128 tiles, 128 x 128 tiles, the caller's own tile — all on the split-operand kernel of the bf16 matrix
// pipe (igemm_x9.h) — or the fmaf-chain kernel (igemm.h).  x9_ok: both operands are fp32 (a0_x9_ok); mats: both are plain matrices, unsplit or as term planes;
// wgrad_family: an x-contiguous A operand (weight gradients); gather: an im2col-gathered B operand.
enum a0_tile_class { A0_TILE_HUGE, A0_TILE_BIG, A0_TILE_OWN, A0_TILE_FP32 };
// 128 x 128 tiles (times splits) from which the eight-wave tile takes a problem
static inline bool a0_x9_big_round(long long tiles128) { constexpr long long A0_X9_BIG_TILES = 256; return tiles128 >= A0_X9_BIG_TILES; }
static inline a0_tile_class a0_gemm_tile_class(int X, int Y, int K, int splits, bool x9_ok, bool mats, bool wgrad_family, bool gather) {
    constexpr long long A0_X9_HUGE_TILES = 250;      // 256 x 128 tiles (times splits) from which that tile takes a problem
    // fp32 operands: the split-operand kernel; A0_GEMM=fp32 keeps the fmaf-chain kernel
    if (!x9_ok || a0_gemm_mode(-1) == 0) return A0_TILE_FP32;
    // large problems: 128 x 128 tiles on eight waves (two per SIMD: the splits of one wave issue in the shadow of the other's MFMAs)
    const int sp = splits < 1 ? 1 : splits;
    const long long big = (long long)((X + 127) / 128) * ((Y + 127) / 128) * sp;
    // weight gradients (x-contiguous A): the short, heavily split reductions of a 512-row batch are staging-bound, and there
    // the fp32 kernel's plain 16-byte LDS commits win (conv2/conv3 36 vs 44 us, fc1 17.7 vs 19.4 us); the split kernel takes
    // them only when each split is at least 512 deep (the quantile networks' B*N-row reductions: fc1 1.12 vs 1.34 ms)
    const bool deep = K / sp >= 512;
    // very large dense problems (the quantile networks' 32 768-row layers): 256 x 128 tiles of 16 k on eight waves, 64 x 64 per wave — a quarter less
    // staging and a third fewer LDS fragment reads per MFMA than the 128 x 128 x 32 tile, the same 36 MFMAs per wave between barriers; taken when
    // there is about a full round of such tiles (the actor's 8 192 rows would fill half the CUs and keep the smaller tile)
    const long long huge = (long long)((X + 255) / 256) * ((Y + 127) / 128) * sp;
    // ... and when they fill their rounds of 256 workgroups about as well as the smaller tiles fill theirs (the tile is worth ~5 %; relaxing this for
    // fqf's 16 384-row data gradient, 1600 tiles = 6.25 rounds, or its 15 872-row pass, 248 tiles, gained nothing: 384.7 vs 385.3 us, 347.9 vs 342.8 us)
    const double fill_huge = (double)huge / (256.0 * (double)((huge + 255) / 256)), fill_big = (double)big / (256.0 * (double)((big + 255) / 256));
    if (mats && X >= 256 && Y >= 128 && huge >= A0_X9_HUGE_TILES && fill_huge >= 0.93 * fill_big && (deep || !wgrad_family)) return A0_TILE_HUGE;
    // (round 6, six products: the same 128 x 128 tile on FOUR waves of 64 x 64 — a third fewer LDS fragment reads per MFMA, one wave per SIMD — measured 139.9 vs
    // 137.7 us on the actor's 8 192-row fc1, iqn 86.4 vs 85.9 ms: not kept, profiles/r06_experiments.md)
    // (round 6: TWO four-wave workgroups per CU on 128 x 64 x 16 tiles — independent barriers, so the SIMD partners are not in lockstep — measured 211 vs 177 us at
    // 8 192 rows, 319 vs 322 at 16 384: not kept, profiles/r06_experiments.md)
    if (X >= 128 && Y >= 128 && a0_x9_big_round(big) && (deep || !wgrad_family)) return A0_TILE_BIG;
    return (!wgrad_family || (deep && !gather)) ? A0_TILE_OWN : A0_TILE_FP32;
}

// one split-operand launch with the probe's event pair travelling IN it (the dispatch's own timestamps, as for the fused kernels)
template <class OA, class OB, class EP, int... TILE>
static void a0_x9_probed(hipStream_t st, int tag, const typename OA::Params& pa, const typename OB::Params& pb, const typename EP::Params& pe, int X, int Y, int K, int splits) {
    hipEvent_t e0 = nullptr, e1 = nullptr;
    const bool probe = a0_probe_events(tag, &e0, &e1);
    A0_HIP_THROW((a0_igemm_x9_launch<OA, OB, EP, TILE...>(st, pa, pb, pe, X, Y, K, splits, e0, e1)));
    if (probe) a0_probe_commit(2.0 * (double)X * (double)Y * (double)K);
}

struct a0_hip_backend {
    hipStream_t st;
    int tag = 0;
    const a0_tail_prep* prep = nullptr;      // a0_net_encoder_wgrad_tail: bookkeeping to ride in the per-observation conv1 launch; prep_done: it did
    bool prep_done = false;
    template <class OA, class OB, class EP, int WM, int WN, int MT, int NT>
    void igemm(const typename OA::Params& pa, const typename OB::Params& pb, const typename EP::Params& pe, int X, int Y, int K, int splits) {
        constexpr bool x9_ok = a0_x9_ok<OA>::value && a0_x9_ok<OB>::value, mats = a0_is_mat<OA>::value && a0_is_mat<OB>::value;
        switch (a0_gemm_tile_class(X, Y, K, splits, x9_ok, mats, OA::MODE == A0_XC, a0_is_gather<OB>::value)) {
        case A0_TILE_HUGE: if constexpr (x9_ok && mats) a0_x9_probed<OA, OB, EP, 4, 2, 2, 2, 1>(st, tag, pa, pb, pe, X, Y, K, splits); return;
        case A0_TILE_BIG: if constexpr (x9_ok) a0_x9_probed<OA, OB, EP, 4, 2, 1, 2>(st, tag, pa, pb, pe, X, Y, K, splits); return;
        case A0_TILE_OWN: if constexpr (x9_ok) a0_x9_probed<OA, OB, EP, WM, WN, MT, NT>(st, tag, pa, pb, pe, X, Y, K, splits); return;
        case A0_TILE_FP32: break;
        }
        // the fmaf-chain kernel has four waves: an eight-wave tile shape falls back to the same tile on four (twice the blocks per wave along N); bracketed
        constexpr bool eight = WM * WN == 8;
        constexpr int FWN = eight ? WN / 2 : WN, FNT = eight ? NT * 2 : NT;
        static_assert(!eight || (WN % 2) == 0, "eight-wave shapes: even wave count along N");
        a0_probe_bracket pb_(tag, st);
        A0_HIP_THROW((a0_igemm_launch<OA, OB, EP, WM, FWN, MT, FNT>(st, pa, pb, pe, X, Y, K, splits)));
        pb_.stop(2.0 * (double)X * (double)Y * (double)K);
    }
    // (not part of the timing probe's dense_fwd family: bound by its output stream, not by the matrix pipe)   dense.hip defines it: the kernel is its unit's
    void short_k_fwd(const float* X, int ldx, const float* W, const float* b, const float* M, int group, float* Y, float* Y2, int R, int N, int relu);
    // the fused per-observation weight gradients commit nothing when their launcher returns 0 (unsupported shape: the GEMM path follows)
    int conv1_wgrad_fused(const a0_net_core& n, const a0_frames_arg& f, int B, const float* d1, float* slabs) {
        if (!slabs) return 0;
        a0_probe_bracket pb(tag, st);
        const int g = a0_conv1_wgrad_fused_launch(&f, n.C, n.H, n.W, B, d1, slabs, prep, st);
        if (g > 0 && prep) prep_done = true;
        if (g > 0) pb.stop(2.0 * 32.0 * (double)n.K1 * (double)B * n.H1 * n.W1);
        return g;
    }
    bool conv23_wgrad_fused(const a0_net_core& n, int B, const float* act1, const float* act2, const float* d2, const float* d3, float* slab2, float* slab3) {
        a0_probe_bracket pb(A0_TAG_CONV2_WGRAD, st);
        const int ran = a0_conv23_wgrad_fused_launch(n, B, act1, act2, d2, d3, slab2, slab3, st);
        if (ran) pb.stop(2.0 * 64.0 * ((double)n.K2 * n.H2 * n.W2 + (double)n.K3 * n.H3 * n.W3) * B);
        return ran != 0;
    }
    void reduce_slabs(const float* slabs, long long slab_stride, int nslab, float* out, long long count) { a0_reduce_slabs_launch(st, slabs, slab_stride, nslab, out, count); }
    void reduce_segments(const a0_reduce_seg* segs, int nseg) { a0_reduce_segments_launch(st, segs, nseg); }
    void reduce_bias_act(const float* slabs, long long slab_stride, int nslab, const float* bias, float* out, int rows, int N, int relu) {
        a0_reduce_bias_act_launch(st, slabs, slab_stride, nslab, bias, out, rows, N, relu);
    }
};
