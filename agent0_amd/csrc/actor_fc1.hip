// The actor's per-step fc1 GEMM (model.py:112-114 under Actor.act, agent.py:25-39) as a kernel of its own: up to 256 rows x 512 x K, written as the split-K slabs of
// a0_dense_fwd_partial — the same slab count, the same k range per slab, the same six v_mfma_f32_32x32x16_bf16 products per 16 k in the same order into the same
// accumulator, so every slab element has the bits the general kernel (igemm_x9.h, <OpMatKC, OpMatKC, EpiSlab, 2, 2, 1, 1, 2>, six products) gives it.
//
// What differs is the weight operand.  W does not change inside a rollout, yet the general kernel re-reads its fp32 tile in each of the 80 launches, splits it into the
// three bf16 terms in every workgroup (four row tiles share one W tile), writes the terms to LDS and holds them behind the k tile's barrier.  Here
// a0_actor_fc1_planes_kernel splits W ONCE per change of W and lays the terms out in MFMA-fragment order (the scheme of the fused encoder's weights, encoder_fused.hip):
//   uint4 index ((nb * K/16 + ks) * 3 + term) * 64 + lane  holds the eight k = 16 ks + 8 (lane >> 5) .. + 7 of row n = 32 nb + (lane & 31), term 0 / 1 / 2 = hi / mid / lo
// — the B fragment of `lane` for k-step ks of column block nb.  A wave's load of one term of one k-step is 1 KB of consecutive memory; each lane streams its own fragments
// with 16-byte global loads through a register ring A0_FC1_RING k tiles deep.  W uses no LDS and no barrier; the k tile's barrier covers the features alone, whose staging
// (fetch, split on the fly, three 8-byte LDS writes per float4) is the general kernel's own code (a0_x9_stager<OpMatKC>, unmasked as in its FULL launches).
//
// Global traffic inside the k loop is loads only (the features' and the ring's), which return in order: the waits in the loop over whole groups of ring tiles are
// counted (vmcnt(24) and up); vmcnt(0) stands in the prologue (the first feature tile), in the last nt % 4 tiles behind the loop, where nothing is refilled, and in front
// of the slab stores.
#include "igemm_x9.h"
#include "a0_internal.h"
#include "net_impl.h"
#include "store_policy.h"
// the eight split-K slabs of a step (store_policy.h): read by the step kernel behind this launch; a lane holds 4 bytes per element
typedef a0_st_wt a0_fc1_store;       // measured: 0.3 - 0.4 us per launch (profiles/r20_store_policy.md)

constexpr int A0_FC1_RING = 4;      // k tiles (32 k = six fragments per lane) in flight per lane; even: LDS buffer and register slot of a tile follow its ring slot's parity

__global__ __launch_bounds__(256) void a0_actor_fc1_kernel(const float* __restrict__ X, int ldx, const uint4* __restrict__ Wp, float* __restrict__ slabs, int R, int N, int K,
                                                           int kchunk, int gx, int gy) {
    typedef a0_x9_stager<OpMatKC, 64, 256, 2> SA;
    constexpr int APL = SA::IM::PLANE, ABYTES = 3 * APL, D = A0_FC1_RING;
    static_assert(SA::R == 2 && (D % 2) == 0, "two feature pieces per thread and tile");
    __shared__ __attribute__((aligned(16))) char As[2 * ABYTES];      // [2 buffers][3 planes][64 rows][80 B]

    const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int wm = wave >> 1, wn = wave & 1;
    // the general kernel's XCD-aware tile order (igemm_x9.h): an XCD walks a contiguous range of logical tiles
    int bx, by, bz;
    {
        const int n = gridDim.x, id = blockIdx.x, per = n >> 3;
        const int L = (id < (per << 3)) ? (id & 7) * per + (id >> 3) : id;
        if (gy <= gx) { by = L % gy; const int t = L / gy; bx = t % gx; bz = t / gx; }
        else          { bx = L % gx; const int t = L / gx; by = t % gy; bz = t / gy; }
    }
    const int x0 = bx * 64, y0 = by * 64;
    const int kb = bz * kchunk;
    const int ke = (K < kb + kchunk) ? K : (kb + kchunk);
    const int nt = ke > kb ? (ke - kb) >> 5 : 0;
    // C/D layout of v_mfma_f32_32x32x16_bf16: column = lane & 31, row = (r & 3) + 8 * (r >> 2) + 4 * (lane >> 5)
    float* const out = slabs + (long long)bz * R * N + (y0 + wn * 32 + (lane & 31));
    if (nt < 1) {      // a slab whose k range is empty is written as zeros, as the general kernel writes it.  (Leaving here also tells the compiler that the k loop below
                       // runs at least once: with a guard around it, it moves the ring's first loads behind the first barrier, one more latency in front of the first MFMA)
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            const int x = x0 + wm * 32 + (r & 3) + 8 * (r >> 2) + 4 * (lane >> 5);
            if (x < R) out[(long long)x * N] = 0.f;
        }
        return;
    }

    const a0_mat_src pa{X, ldx};
    SA sa;
    sa.init(pa, x0, R, kb, ke, tid);

    // the ring: tile t of this workgroup is k tile kb / 32 + t of W; tiles past the end of W re-read the last one and are never multiplied
    const int T = K >> 5, t0 = kb >> 5;
    const uint4* const wbase = Wp + (long long)((y0 >> 5) + wn) * (K >> 4) * (3 * 64) + lane;
    a0_u32x4g ring[D][6];
    auto fill = [&](int slot, int tile) {
        const int tt = tile < T ? tile : T - 1;
        const a0_u32x4g* p = (const a0_u32x4g*)(wbase + (long long)tt * (6 * 64));
#pragma unroll
        for (int i = 0; i < 6; ++i) ring[slot][i] = p[i * 64];
    };

    a0_acc16 acc;
#pragma unroll
    for (int r = 0; r < 16; ++r) acc[r] = 0.f;

    // features: tiles 0 and 1 into the two register slots (the first thing requested: tile 0 is what the first barrier waits for), then the ring's D tiles
    typename SA::Slot s0, s1;
    s0.okmask = s1.okmask = 0u;
#pragma unroll
    for (int p = 0; p < 2; ++p) sa.template fetch_piece<true>(pa, s0, p, kb, ke, tid);
#pragma unroll
    for (int p = 0; p < 2; ++p) sa.template fetch_piece<true>(pa, s1, p, kb + 32, ke, tid);
#pragma unroll
    for (int d = 0; d < D; ++d) fill(d, t0 + d);

    // micro-step u of a feature tile's staging (the general kernel's): piece u / 6, step u % 6 = take | split e0..e3 | pack + store + refetch
    a0_x9_piece pc;
    a0_f4 unused = a0_zero4();
    auto micro = [&](int u, typename SA::Slot& s, char* a_dst, int k_fetch) {
        const int p = u / 6, st = u % 6;
        if (st == 0) pc.v = sa.template value<false, true>(s, p, unused);
        else if (st <= 4) pc.split(st - 1);
        else { sa.store(pc, p, a_dst, tid); sa.template fetch_piece<true>(pa, s, p, k_fetch, ke, tid); }
    };
    const int abase = SA::frag_base(lane, wm * 32);

    // One tile: multiply LDS buffer `buf` by ring slot `b` while the next tile (slot s) is split and written into the other buffer and the tile after the
    // next-but-one is requested into the registers each piece frees; one micro-step behind each of the twelve MFMAs, pinned there
    auto mma_tile = [&](int buf, typename SA::Slot& s, const a0_u32x4g (&b)[6], int k_fetch) {
        const char* ap = As + buf * ABYTES;
        char* a_dst = As + (buf ^ 1) * ABYTES;
        a0_u32x4g a[2][3];
#pragma unroll
        for (int ks = 0; ks < 2; ++ks)
#pragma unroll
            for (int t = 2; t >= 0; --t) a[ks][t] = SA::frag(ap + t * APL, abase, 0, ks);
        __builtin_amdgcn_sched_barrier(0);
#pragma unroll
        for (int n = 0; n < 12; ++n) {
            // the six products of a0_igemm_x9_body (NPR = 6) in its order: lo*hi, mid*mid, hi*lo, mid*hi, hi*mid, hi*hi (features x weights), k-step 0 then 1
            constexpr int TA[6] = {2, 1, 0, 1, 0, 0};
            constexpr int TB[6] = {0, 1, 2, 0, 1, 0};
            const int ks = n / 6, q = n % 6;
            acc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(__builtin_bit_cast(a0_bf16x8g, a[ks][TA[q]]), __builtin_bit_cast(a0_bf16x8g, b[ks * 3 + TB[q]]), acc, 0, 0, 0);
            micro(n, s, a_dst, k_fetch);
            __builtin_amdgcn_sched_barrier(0);
        }
    };

    // tile 0 into LDS buffer 0, tile 2 into the freed slot
#pragma unroll
    for (int u = 0; u < 12; ++u) micro(u, s0, As, kb + 64);
    __syncthreads();
    // whole groups of D tiles in a loop without an exit in its body (an exit between two tiles joins the loop's head, and the head's first wait — is ring slot 0
    // here? — would then answer for a slot filled one tile ago instead of D tiles ago: vmcnt(5) instead of vmcnt(24)); the last nt % D tiles follow, without refills
    int tb = 0;
#pragma unroll 1
    for (; tb + D <= nt; tb += D) {
#pragma unroll
        for (int u = 0; u < D; ++u) {
            mma_tile(u & 1, (u & 1) ? s0 : s1, ring[u], kb + 32 * (tb + u + 3));
            fill(u, t0 + tb + u + D);
            __builtin_amdgcn_sched_barrier(0);
            __syncthreads();
        }
    }
#pragma unroll
    for (int u = 0; u < D - 1; ++u) {
        if (tb + u < nt) {
            mma_tile(u & 1, (u & 1) ? s0 : s1, ring[u], kb + 32 * (tb + u + 3));
            __syncthreads();
        }
    }

#pragma unroll
    for (int r = 0; r < 16; ++r) {
        const int x = x0 + wm * 32 + (r & 3) + 8 * (r >> 2) + 4 * (lane >> 5);
        if (x < R) a0_store4<a0_fc1_store>(&out[(long long)x * N], __float_as_uint(acc[r]));
    }
}

// W [N][K] fp32 -> the fragment-ordered term planes above: one thread per (column block, k-step, lane) reads its eight k (32 B) and writes its three fragments, a wave
// 1 KB of consecutive memory per term.  The exact truncation split the GEMM forms per tile (a0_x9_piece, as a0_split_planes_kernel).
__global__ __launch_bounds__(256) void a0_actor_fc1_planes_kernel(const float* __restrict__ W, uint4* __restrict__ planes, int K, long long count) {
    const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= count) return;
    const int lane = (int)(i & 63), K16 = K >> 4;
    const long long g = i >> 6;                       // nb * K16 + ks
    const int nb = (int)(g / K16), ks = (int)(g - (long long)nb * K16);
    const a0_f4* src = (const a0_f4*)(W + (long long)(nb * 32 + (lane & 31)) * K + ks * 16 + 8 * (lane >> 5));
    a0_u32x2g hi[2], mid[2], lo[2];
#pragma unroll
    for (int h = 0; h < 2; ++h) {
        a0_x9_piece pc;
        pc.v = src[h];
#pragma unroll
        for (int e = 0; e < 4; ++e) pc.split(e);
        pc.pack(hi[h], mid[h], lo[h]);
    }
    uint4* o = planes + g * (3 * 64) + lane;
    o[0] = uint4{hi[0].x, hi[0].y, hi[1].x, hi[1].y};
    o[64] = uint4{mid[0].x, mid[0].y, mid[1].x, mid[1].y};
    o[128] = uint4{lo[0].x, lo[0].y, lo[1].x, lo[1].y};
}

extern "C" long long a0_actor_fc1_planes_words(int N, int K) { return (N < 1 || K < 1) ? 0 : (long long)N * (K / 8) * 12; }

extern "C" int a0_actor_fc1_planes(const float* W, unsigned int* planes, int N, int K, void* stream) {
    if (!W || !planes || N < 32 || (N & 31) || K < 16 || (K & 15) || ((((uintptr_t)W) | ((uintptr_t)planes)) & 15))
        return a0_fail(A0_EINVAL, "a0_actor_fc1_planes: bad argument (N a multiple of 32, K a multiple of 16, 16-byte aligned buffers)");
    const long long count = (long long)(N / 32) * (K / 16) * 64;
    hipLaunchKernelGGL(a0_actor_fc1_planes_kernel, dim3((unsigned)((count + 255) / 256)), dim3(256), 0, (hipStream_t)stream, W, (uint4*)planes, K, count);
    return a0_fail_hip((int)hipGetLastError(), "a0_actor_fc1_planes");
}

// The shapes the kernel takes: fc1's 512 columns, whole k tiles, the rows for which a0_dense_fwd_partial runs its 64 x 64 tile, and the split-operand GEMM in its
// six-product form (what the slabs are bit-identical to).  Elsewhere callers keep a0_dense_fwd_partial.
extern "C" int a0_actor_fc1_ok(int R, int N, int K) {
    return (R >= 1 && R <= 256 && N == 512 && K >= 32 && !(K & 31) && a0_gemm_mode(-1) != 0 && a0_x9_products_now() == 6) ? 1 : 0;
}

extern "C" int a0_actor_fc1_n(const float* X, int ldx, const unsigned int* planes, int R, int N, int K, int splits, float* slabs, void* stream) {
    if (!X || !planes || !slabs || (ldx & 3) || ldx < K || !a0_actor_fc1_ok(R, N, K) || ((((uintptr_t)X) | ((uintptr_t)planes)) & 15))
        return a0_fail(A0_EINVAL, "a0_actor_fc1_n: shapes a0_actor_fc1_ok accepts (16-byte aligned rows)");
    if (const int rc = a0_splits_check("a0_actor_fc1_n", splits, K)) return rc;
    const int ktiles = K / 32;
    const int kchunk = ((ktiles + splits - 1) / splits) * 32;         // a0_igemm_x9_launch's
    const int gx = (R + 63) / 64, gy = N / 64;
    A0_LAUNCH_PROBED(A0_TAG_DENSE_FWD, 2.0 * (double)R * (double)N * (double)K, a0_actor_fc1_kernel, dim3((unsigned)(gx * gy * splits)), dim3(256), 0, (hipStream_t)stream, X, ldx,
                     (const uint4*)planes, slabs, R, N, K, kchunk, gx, gy);
    return a0_fail_hip((int)hipGetLastError(), "a0_actor_fc1_n");
}
