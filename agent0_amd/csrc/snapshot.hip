// Replay snapshots (Trainer.save_snapshot / load_snapshot): lossless, content-verified frame deduplication of ring rows on their way to a file, and back.
//
// A ring row is st || st_next, two sliding windows of 4 frames: every frame an env emits is stored about eight times.  The ring keeps that layout;
// these kernels remove the repeats from a CHUNK of rows (at most 32 768 frames: 4 096 rows of 8) and put them back:
//
//   pack    for every frame (r, j) of the chunk, in row order: the first byte-identical frame among a fixed candidate set — the frames (r, 0 .. j - 1) of the same
//           row, then the frames (r - stride, 0 .. F - 1) of the row `stride` earlier in the chunk (the same env's previous step when stride = num_envs) — or none:
//           the frame is a literal.  References are followed to their literal (a chain runs back through the chunk), literals are numbered in row order, and the
//           packed chunk is
//               u32 lit_id[rows * F] | u32 n_lit | pad to 16 B | u8 literals[n_lit][frame_bytes]
//           Matching compares bytes, 16 B per lane with an exit at the first differing 1 KiB; nothing is assumed about how the rows were made, so n-step rows, resets,
//           a wrong stride or rows written by host envs lower the ratio and never change a byte.  No reference leaves the chunk.
//   unpack  frame(r, j) = literals[lit_id[r][j]]: a pure gather straight into ring rows.
//
// The same ring packs to the same bytes: every choice above is a function of the chunk's bytes alone (first match in a fixed order, literals in row order).
// The numpy restatement the tests compare against is tests/snapshot_ref.py.
#include "a0_internal.h"

namespace {

constexpr int SNAP_MAX_FRAMES = 32768;      // frames per chunk: the resolve / scan kernel is ONE workgroup of 1024 lanes with 32 frames each

// does frame `a` equal frame `b`?  One wavefront; nvec 16-byte vectors; every lane returns the same answer
__device__ __forceinline__ bool snap_equal(const uint4* __restrict__ a, const uint4* __restrict__ b, int nvec, int lane) {
    for (int v0 = 0; v0 < nvec; v0 += 64) {
        const int v = v0 + lane;
        bool diff = false;
        if (v < nvec) {
            const uint4 x = a[v], y = b[v];
            diff = (x.x != y.x) | (x.y != y.y) | (x.z != y.z) | (x.w != y.w);
        }
        if (__ballot(diff) != 0ull) return false;
    }
    return true;
}

// one wavefront per frame: ref[i] = the chunk-wide index of the first identical candidate, or i itself (a literal)
__global__ __launch_bounds__(256) void a0_snapshot_match_kernel(const uint8_t* __restrict__ rows, int n_rows, int F, int frame_bytes, int stride, unsigned int* __restrict__ ref) {
    const int lane = threadIdx.x & 63;
    const int i = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (i >= n_rows * F) return;
    const int r = i / F, j = i - r * F, nvec = frame_bytes >> 4;
    const uint4* me = (const uint4*)(rows + (long long)i * frame_bytes);
    unsigned int found = (unsigned int)i;
    for (int c = 0; c < j; ++c) {
        const int k = r * F + c;
        if (snap_equal(me, (const uint4*)(rows + (long long)k * frame_bytes), nvec, lane)) { found = (unsigned int)k; break; }
    }
    if (found == (unsigned int)i && stride > 0 && r >= stride) {
        for (int c = 0; c < F; ++c) {
            const int k = (r - stride) * F + c;
            if (snap_equal(me, (const uint4*)(rows + (long long)k * frame_bytes), nvec, lane)) { found = (unsigned int)k; break; }
        }
    }
    if (lane == 0) ref[i] = found;
}

// ONE workgroup: follow every reference to its literal (pointer jumping: a reference always points to an earlier frame, so 15 doublings cover 32 768 frames), number
// the literals in frame order (exclusive scan of the literal flags), lit_id[i] = number of i's literal.  ref[] ends up holding every frame's literal frame.
__global__ __launch_bounds__(1024) void a0_snapshot_resolve_kernel(unsigned int* __restrict__ ref, int n, unsigned int* __restrict__ lit_id, unsigned int* __restrict__ n_lit) {
    __shared__ unsigned int part[1024];
    const int t = threadIdx.x;
    const int per = (n + 1023) / 1024, lo = t * per, hi = lo + per < n ? lo + per : n;
    // loads and stores of ref[] that other lanes' passes depend on go through the device-scope cache level, ordered by the barrier between the passes
    for (int pass = 0; pass < 16; ++pass) {
        for (int i = lo; i < hi; ++i) {
            const unsigned int p = __hip_atomic_load(ref + i, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            const unsigned int g = __hip_atomic_load(ref + p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            if (g != p) __hip_atomic_store(ref + i, g, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        }
        __threadfence();
        __syncthreads();
    }
    unsigned int cnt = 0;
    for (int i = lo; i < hi; ++i) cnt += __hip_atomic_load(ref + i, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) == (unsigned int)i ? 1u : 0u;
    part[t] = cnt;
    __syncthreads();
    for (int d = 1; d < 1024; d <<= 1) {          // inclusive scan of the per-lane counts
        const unsigned int add = t >= d ? part[t - d] : 0u;
        __syncthreads();
        part[t] += add;
        __syncthreads();
    }
    unsigned int base = part[t] - cnt;
    if (t == 1023) n_lit[0] = part[1023];
    for (int i = lo; i < hi; ++i)
        if (__hip_atomic_load(ref + i, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) == (unsigned int)i) __hip_atomic_store(lit_id + i, base++, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    __threadfence();
    __syncthreads();
    for (int i = lo; i < hi; ++i) {
        const unsigned int p = __hip_atomic_load(ref + i, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        if (p != (unsigned int)i) lit_id[i] = __hip_atomic_load(lit_id + p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
}

// one wavefront per frame: a literal goes to its place in the compacted array
__global__ __launch_bounds__(256) void a0_snapshot_scatter_kernel(const uint8_t* __restrict__ rows, int n, int frame_bytes, const unsigned int* __restrict__ ref,
                                                                  const unsigned int* __restrict__ lit_id, uint8_t* __restrict__ literals) {
    const int lane = threadIdx.x & 63;
    const int i = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (i >= n || ref[i] != (unsigned int)i) return;
    const int nvec = frame_bytes >> 4;
    const uint4* s = (const uint4*)(rows + (long long)i * frame_bytes);
    uint4* d = (uint4*)(literals + (long long)lit_id[i] * frame_bytes);
    for (int v = lane; v < nvec; v += 64) d[v] = s[v];
}

// one workgroup per row: every frame from its literal.  An id outside [0, n_lit) — a damaged file — writes nothing and raises the flag word behind n_lit's pad
__global__ __launch_bounds__(256) void a0_snapshot_unpack_kernel(const unsigned int* __restrict__ lit_id, const unsigned int* __restrict__ n_lit, const uint8_t* __restrict__ literals,
                                                                 int F, int frame_bytes, uint8_t* __restrict__ rows, int* __restrict__ bad) {
    const int r = blockIdx.x, nvec = frame_bytes >> 4;
    const unsigned int nl = n_lit[0];
    for (int j = 0; j < F; ++j) {
        const unsigned int id = lit_id[r * F + j];
        if (id >= nl) { if (threadIdx.x == 0 && bad) bad[0] = 1; continue; }
        const uint4* s = (const uint4*)(literals + (long long)id * frame_bytes);
        uint4* d = (uint4*)(rows + ((long long)r * F + j) * frame_bytes);
        for (int v = threadIdx.x; v < nvec; v += 256) d[v] = s[v];
    }
}

inline long long snap_lit_off(long long frames) { return (frames * 4 + 4 + 15) / 16 * 16; }

bool snap_shape_ok(long long n_rows, int F, int frame_bytes) {
    return n_rows >= 1 && F >= 1 && F <= 64 && frame_bytes >= 16 && (frame_bytes % 16) == 0 && n_rows * F <= SNAP_MAX_FRAMES;
}

}  // namespace

extern "C" long long a0_snapshot_pack_bound(long long rows, int frames_per_row, int frame_bytes) {
    if (!snap_shape_ok(rows, frames_per_row, frame_bytes)) { a0_fail(A0_EINVAL, "a0_snapshot_pack_bound: 1 .. 32768 frames per chunk, frame bytes a multiple of 16"); return -1; }
    return snap_lit_off(rows * frames_per_row) + rows * frames_per_row * (long long)frame_bytes;
}

extern "C" long long a0_snapshot_literal_offset(long long rows, int frames_per_row) { return rows >= 1 && frames_per_row >= 1 ? snap_lit_off(rows * frames_per_row) : -1; }

extern "C" int a0_snapshot_pack(const uint8_t* rows, long long n_rows, int frames_per_row, int frame_bytes, long long stride, uint8_t* packed, unsigned int* work, void* stream) {
    if (!rows || !packed || !work || !snap_shape_ok(n_rows, frames_per_row, frame_bytes) || stride < 0)
        return a0_fail(A0_EINVAL, "a0_snapshot_pack: bad argument (1 .. 32768 frames per chunk, frame bytes a multiple of 16, stride >= 0)");
    if ((((uintptr_t)rows) | ((uintptr_t)packed)) & 15) return a0_fail(A0_EINVAL, "a0_snapshot_pack: buffers must be 16-byte aligned");
    const int n = (int)(n_rows * frames_per_row);
    const int st = stride > n_rows ? (int)n_rows : (int)stride;       // a row `stride` earlier than any row of the chunk does not exist
    unsigned int* lit_id = (unsigned int*)packed;
    unsigned int* n_lit = lit_id + n;
    uint8_t* literals = packed + snap_lit_off(n);
    hipStream_t s = (hipStream_t)stream;
    hipLaunchKernelGGL(a0_snapshot_match_kernel, dim3((n + 3) / 4), dim3(256), 0, s, rows, (int)n_rows, frames_per_row, frame_bytes, st, work);
    hipLaunchKernelGGL(a0_snapshot_resolve_kernel, dim3(1), dim3(1024), 0, s, work, n, lit_id, n_lit);
    hipLaunchKernelGGL(a0_snapshot_scatter_kernel, dim3((n + 3) / 4), dim3(256), 0, s, rows, n, frame_bytes, (const unsigned int*)work, (const unsigned int*)lit_id, literals);
    return a0_fail_hip((int)hipGetLastError(), "a0_snapshot_pack");
}

extern "C" int a0_snapshot_unpack(const uint8_t* packed, long long n_rows, int frames_per_row, int frame_bytes, uint8_t* rows, int* bad_flag, void* stream) {
    if (!rows || !packed || !snap_shape_ok(n_rows, frames_per_row, frame_bytes)) return a0_fail(A0_EINVAL, "a0_snapshot_unpack: bad argument (1 .. 32768 frames per chunk, frame bytes a multiple of 16)");
    if ((((uintptr_t)rows) | ((uintptr_t)packed)) & 15) return a0_fail(A0_EINVAL, "a0_snapshot_unpack: buffers must be 16-byte aligned");
    const long long n = n_rows * frames_per_row;
    const unsigned int* lit_id = (const unsigned int*)packed;
    hipLaunchKernelGGL(a0_snapshot_unpack_kernel, dim3((unsigned)n_rows), dim3(256), 0, (hipStream_t)stream, lit_id, lit_id + n, packed + snap_lit_off(n), frames_per_row, frame_bytes, rows, bad_flag);
    return a0_fail_hip((int)hipGetLastError(), "a0_snapshot_unpack");
}
