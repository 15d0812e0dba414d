// The slab reductions behind the split-K GEMMs — plain, with bias and activation (one layer or up to four), up to eight segments in one launch — with their
// launchers (hip_backend.h: a0_hip_backend's reduction members), and the row mean of a rollout's max-Q.  Every sum is formed in a fixed order: deterministic.
#include "hip_backend.h"
#include "update_tail.h"      // a0_rowgroup_sum1 / a0_rowgroup_sum4

// the eight row groups' partial sums of 32 columns meet in LDS (red: [8][33] floats) and row group 0 adds them 0..7 from zero
A0_D void a0_rowgroups_combine1(float* red, int g, int c, float s, bool in, float* out) {
    red[g * 33 + c] = s;
    __syncthreads();
    if (g == 0 && in) {
        float t = 0.f;
#pragma unroll
        for (int j = 0; j < 8; ++j) t += red[j * 33 + c];
        *out = t;
    }
}

// out[i] = sum_z slabs[z][i].  One workgroup per 32 consecutive outputs; its 8 row groups stride over z and are combined as above: 8 slab rows in flight per output column.
__global__ __launch_bounds__(256) void a0_reduce_slabs_kernel(const float* __restrict__ slabs, long long slab_stride, int nslab,
                                                               float* __restrict__ out, long long count) {
    __shared__ float red[8 * 33];
    const int c = threadIdx.x & 31, g = threadIdx.x >> 5;
    const long long i = (long long)blockIdx.x * 32 + c;
    a0_rowgroups_combine1(red, g, c, i < count ? a0_rowgroup_sum1(slabs + i, slab_stride, g, nslab) : 0.f, i < count, out + i);
}

__global__ void a0_reduce_bias_act_kernel(const float* __restrict__ slabs, long long slab_stride, int nslab,
                                          const float* __restrict__ bias, float* __restrict__ out, int rows, int N, int relu) {
    long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    const long long count = (long long)rows * N;
    const long long stride = (long long)gridDim.x * blockDim.x;
    for (; i < count; i += stride) {
        float s = 0.f;
        // eight slabs requested before any is added (additions still in slab order): 32 dependent-looking loads in a row cost a short, wide reduction 10 us
        for (int z = 0; z < nslab; z += 8) {
            float t[8];
#pragma unroll
            for (int zz = 0; zz < 8; ++zz) t[zz] = (z + zz < nslab) ? slabs[(long long)(z + zz) * slab_stride + i] : 0.f;
#pragma unroll
            for (int zz = 0; zz < 8; ++zz)
                if (z + zz < nslab) s += t[zz];
        }
        s += bias[i % N];
        if (relu) s = (s < 0.f) ? 0.f : s;
        out[i] = s;
    }
}

// a0_reduce_bias_act_kernel for up to four layers of the same width in ONE launch (round 4: the three fc1 passes of a distributional update — online on s, online on s', target
// on s' — each leave their own split-K slabs; their reductions are independent and each is a 4.7 us launch of pure latency on its own).  Same arithmetic per element as the
// single-layer kernel: slabs added in slab order, eight requested at a time, then the bias, then the ReLU.
struct a0_rba_seg { const float* slabs; long long slab_stride; int nslab; const float* bias; float* out; int rows; };
struct a0_rba_multi_args { a0_rba_seg seg[4]; int n, N, relu; };
__global__ __launch_bounds__(256) void a0_reduce_bias_act_multi_kernel(a0_rba_multi_args A) {
    const int si = blockIdx.y;
    const a0_rba_seg S = A.seg[si];
    const int N4 = A.N >> 2;
    const long long count4 = (long long)S.rows * N4, st4 = S.slab_stride >> 2;
    const long long stride = (long long)gridDim.x * blockDim.x;
    for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < count4; i += stride) {
        a0_f4 s = a0_zero4();
        const a0_f4* p = (const a0_f4*)S.slabs + i;
        for (int z = 0; z < S.nslab; z += 8) {
            a0_f4 t[8];
#pragma unroll
            for (int zz = 0; zz < 8; ++zz) t[zz] = (z + zz < S.nslab) ? p[(long long)(z + zz) * st4] : a0_zero4();
#pragma unroll
            for (int zz = 0; zz < 8; ++zz)
                if (z + zz < S.nslab) { s.x += t[zz].x; s.y += t[zz].y; s.z += t[zz].z; s.w += t[zz].w; }
        }
        const a0_f4 b = ((const a0_f4*)S.bias)[i % N4];
        s.x += b.x; s.y += b.y; s.z += b.z; s.w += b.w;
        if (A.relu) { s.x = s.x < 0.f ? 0.f : s.x; s.y = s.y < 0.f ? 0.f : s.y; s.z = s.z < 0.f ? 0.f : s.z; s.w = s.w < 0.f ? 0.f : s.w; }
        ((a0_f4*)S.out)[i] = s;
    }
}

// Up to eight slab reductions in one launch: workgroup g serves 128 outputs of the segment its index falls into — 32 lanes x 16 bytes wide, eight row groups striding over the
// slabs and combined in a fixed order through LDS; a segment whose base, stride or count is not a multiple of four floats takes the scalar path (32 outputs per workgroup).
struct a0_reduce_multi_args { a0_reduce_seg seg[8]; int first_block[9]; int vec[8]; };
__global__ __launch_bounds__(256) void a0_reduce_segments_kernel(a0_reduce_multi_args A) {
    __shared__ a0_f4 red4[8][33];
    int si = 0;
#pragma unroll
    for (int k = 1; k < 8; ++k) si += ((int)blockIdx.x >= A.first_block[k]) ? 1 : 0;
    const a0_reduce_seg S = A.seg[si];
    const int c = threadIdx.x & 31, g = threadIdx.x >> 5;
    const long long blk = (long long)((int)blockIdx.x - A.first_block[si]);
    if (A.vec[si]) {
        const long long i4 = blk * 32 + c;                    // float4 index
        const long long n4 = S.count >> 2, st4 = S.slab_stride >> 2;
        red4[g][c] = i4 < n4 ? a0_rowgroup_sum4((const a0_f4*)S.slabs + i4, st4, g, S.nslab) : a0_zero4();
        __syncthreads();
        if (g == 0 && i4 < n4) {
            a0_f4 t = a0_zero4();
#pragma unroll
            for (int j = 0; j < 8; ++j) { const a0_f4 v = red4[j][c]; t.x += v.x; t.y += v.y; t.z += v.z; t.w += v.w; }
            ((a0_f4*)S.out)[i4] = t;
        }
        return;
    }
    const long long i = blk * 32 + c;
    a0_rowgroups_combine1((float*)red4, g, c, i < S.count ? a0_rowgroup_sum1(S.slabs + i, S.slab_stride, g, S.nslab) : 0.f, i < S.count, S.out + i);
}

void a0_reduce_slabs_launch(hipStream_t st, const float* slabs, long long slab_stride, int nslab, float* out, long long count) {
    hipLaunchKernelGGL(a0_reduce_slabs_kernel, dim3((unsigned)((count + 31) / 32)), dim3(256), 0, st, slabs, slab_stride, nslab, out, count);
    A0_HIP_THROW(hipGetLastError());
}
void a0_reduce_segments_launch(hipStream_t st, const a0_reduce_seg* segs, int nseg) {
    if (nseg < 1 || nseg > 8) throw std::runtime_error("reduce_segments: 1..8 segments");
    a0_reduce_multi_args A;
    int blocks = 0;
    for (int k = 0; k < 8; ++k) {
        A.first_block[k] = blocks;
        A.vec[k] = 0;
        if (k < nseg) {
            A.seg[k] = segs[k];
            A.vec[k] = ((segs[k].count | segs[k].slab_stride) % 4 == 0) && a0_aligned(16, segs[k].slabs, segs[k].out);
            blocks += A.vec[k] ? (int)((segs[k].count / 4 + 31) / 32) : (int)((segs[k].count + 31) / 32);
        } else {
            A.seg[k] = a0_reduce_seg{nullptr, 0, 0, nullptr, 0};
        }
    }
    A.first_block[8] = blocks;
    for (int k = nseg; k < 8; ++k) A.first_block[k] = 0x7fffffff;        // unused segments are never selected
    hipLaunchKernelGGL(a0_reduce_segments_kernel, dim3((unsigned)blocks), dim3(256), 0, st, A);
    A0_HIP_THROW(hipGetLastError());
}
void a0_reduce_bias_act_launch(hipStream_t st, const float* slabs, long long slab_stride, int nslab, const float* bias, float* out, int rows, int N, int relu) {
    hipLaunchKernelGGL(a0_reduce_bias_act_kernel, dim3(a0_grid_256((long long)rows * N)), dim3(256), 0, st, slabs, slab_stride, nslab, bias, out, rows, N, relu);
    A0_HIP_THROW(hipGetLastError());
}

extern "C" int a0_reduce_bias_act_multi(int n, const float* const* slabs, const long long* slab_stride, const int* nslab, const float* const* bias, float* const* out,
                                       const int* rows, int N, int relu, void* stream) {
    if (n < 1 || n > 4 || !slabs || !slab_stride || !nslab || !bias || !out || !rows || N < 4 || (N & 3)) return a0_fail(A0_EINVAL, "a0_reduce_bias_act_multi: bad argument (1..4 layers, N a multiple of 4)");
    a0_rba_multi_args A;
    A.n = n; A.N = N; A.relu = relu;
    int maxrows = 0;
    for (int i = 0; i < n; ++i) {
        if (!slabs[i] || !bias[i] || !out[i] || rows[i] < 1 || nslab[i] < 1 || (slab_stride[i] & 3) || slab_stride[i] < (long long)rows[i] * N ||
            !a0_aligned(16, slabs[i], bias[i], out[i]))
            return a0_fail(A0_EINVAL, "a0_reduce_bias_act_multi: bad layer (16-byte aligned buffers, slab stride a multiple of 4 floats)");
        A.seg[i] = a0_rba_seg{slabs[i], slab_stride[i], nslab[i], bias[i], out[i], rows[i]};
        if (rows[i] > maxrows) maxrows = rows[i];
    }
    for (int i = n; i < 4; ++i) A.seg[i] = A.seg[0];
    hipLaunchKernelGGL(a0_reduce_bias_act_multi_kernel, dim3(a0_grid_256((long long)maxrows * (N >> 2)), n), dim3(256), 0, (hipStream_t)stream, A);
    return a0_fail_hip((int)hipGetLastError(), "a0_reduce_bias_act_multi");
}

// out[t] = mean_e x[t][e]: the per-step mean max-Q of a rollout (agent.py:38,88), all T steps in one launch
__global__ __launch_bounds__(256) void a0_mean_rows_kernel(const float* __restrict__ x, int E, float* __restrict__ out) {
    __shared__ float red[256];
    const float* p = x + (long long)blockIdx.x * E;
    float s = 0.f;
    for (int e = threadIdx.x; e < E; e += 256) s += p[e];
    red[threadIdx.x] = s;
    __syncthreads();
    for (int o = 128; o > 0; o >>= 1) { if ((int)threadIdx.x < o) red[threadIdx.x] += red[threadIdx.x + o]; __syncthreads(); }
    if (threadIdx.x == 0) out[blockIdx.x] = red[0] / (float)E;
}

extern "C" int a0_mean_rows(const float* x, int T, int E, float* out, void* stream) {
    if (!x || !out || T < 1 || E < 1) return a0_fail(A0_EINVAL, "a0_mean_rows: bad argument");
    hipLaunchKernelGGL(a0_mean_rows_kernel, dim3(T), dim3(256), 0, (hipStream_t)stream, x, E, out);
    return a0_fail_hip((int)hipGetLastError(), "a0_mean_rows");
}
