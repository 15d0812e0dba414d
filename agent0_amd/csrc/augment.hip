// learner.aug_shift: DrQ's random shift of a sampled batch (gfx950).  No reference counterpart: the reference trains on the frames as they were stored.
// Every observation of the batch — C planes of H x W bytes, st and st_next of a replay row each on its own — is padded by `pad` pixels with edge replication and
// cropped back at a random offset, i.e. out[c][y][x] = in[c][clamp(y + dy, 0, H - 1)][clamp(x + dx, 0, W - 1)] with one (dy, dx) in [-pad, pad]^2 for all C planes.
// The draw: Philox stream 7 of the learner's seed; sample b of update u owns the block at counter u * B + b (the stream's words 4 (u B + b) ... + 3, as
// a0_rng_u32 numbers them): words 0 / 1 = dy / dx of st, words 2 / 3 = dy / dx of st_next, each `word % (2 pad + 1) - pad` (a0_rng_randint's reduction).  u is the
// free-running update count the Adam launches keep in state[6], read on the device: a replayed hipGraph moves on by itself and a resumed run continues the sequence.
// Pure byte movement: B * row_bytes read (through `slot`, never written), as much written to the dense batch the encoder kernels then read with slot == NULL.
#include "a0_internal.h"
#include "philox.h"

// One 256-lane workgroup per (sample, observation).  STAGED: the source observation goes to LDS with 16-byte loads and the lanes pick their bytes from there;
// otherwise (an observation above A0_AUG_LDS_BYTES) they pick them from global memory.  Either way a lane assembles 16 consecutive output bytes — the flat
// offset is cut into (plane, row, column) once and carried from byte to byte — and writes them with one 16-byte store.
#define A0_AUG_LDS_BYTES (64 * 1024)

template <bool STAGED>
__global__ __launch_bounds__(256) void a0_augment_shift_kernel(const uint8_t* __restrict__ frames, const int* __restrict__ slot, long long row_bytes, int C, int H, int W,
                                                               int pad, int B, unsigned long long seed, const int* __restrict__ state, unsigned long long u_host,
                                                               uint8_t* __restrict__ out) {
    extern __shared__ __attribute__((aligned(16))) uint8_t a0_aug_lds[];
    const int b = (int)(blockIdx.x >> 1), o = (int)(blockIdx.x & 1);
    const int HW = H * W, obs = C * HW, n16 = obs >> 4;
    const unsigned long long u = state ? (unsigned long long)(unsigned)state[6] : u_host;
    const unsigned long long blk = u * (unsigned long long)B + (unsigned long long)b;
    const a0_u4 r = a0_philox4x32_10((uint32_t)blk, (uint32_t)(blk >> 32), A0_STREAM_AUG, 0u, (uint32_t)seed, (uint32_t)(seed >> 32));
    const uint32_t span = 2u * (uint32_t)pad + 1u;
    const int dy = (int)((o ? r.z : r.x) % span) - pad, dx = (int)((o ? r.w : r.y) % span) - pad;
    const long long row = slot ? (long long)slot[b] : (long long)b;
    const uint8_t* src = frames + row * row_bytes + (long long)o * obs;
    uint8_t* dst = out + (long long)b * row_bytes + (long long)o * obs;
    if constexpr (STAGED) {
        for (int j = threadIdx.x; j < n16; j += 256) ((uint4*)a0_aug_lds)[j] = ((const uint4*)src)[j];
        __syncthreads();
    }
    const uint8_t* in = STAGED ? (const uint8_t*)a0_aug_lds : src;
    for (int j = threadIdx.x; j < n16; j += 256) {
        const int e = j << 4;
        int c = e / HW;
        const int rem = e - c * HW;
        int y = rem / W, x = rem - y * W;
        int base = c * HW + min(max(y + dy, 0), H - 1) * W;
        uint32_t w[4] = {0u, 0u, 0u, 0u};
#pragma unroll
        for (int k = 0; k < 16; ++k) {
            w[k >> 2] |= (uint32_t)in[base + min(max(x + dx, 0), W - 1)] << (8 * (k & 3));
            if (++x == W) {      // the next byte opens a row, possibly a plane (the last byte of the observation opens nothing: its base is not read)
                x = 0;
                if (++y == H) { y = 0; ++c; }
                base = c * HW + min(max(y + dy, 0), H - 1) * W;
            }
        }
        ((uint4*)dst)[j] = make_uint4(w[0], w[1], w[2], w[3]);
    }
}

// the range checks of a0_augment_shift, shared with a0_learner_set_aug_shift (learner.hip), which makes them at set time against the handle's geometry
int a0_augment_shift_check(const char* who, int C, int H, int W, int pad, long long row_bytes) {
    const std::string w(who);
    if (C < 1 || H < 1 || W < 1) return a0_fail(A0_EINVAL, (w + ": C, H, W >= 1").c_str());
    if (pad < 1) return a0_fail(A0_EINVAL, (w + ": pad < 1 (a shift of zero pixels is the setting switched off)").c_str());
    if (pad >= (H < W ? H : W)) return a0_fail(A0_EINVAL, (w + ": pad >= min(H, W)").c_str());
    if (pad > 16) return a0_fail(A0_EINVAL, (w + ": pad > 16").c_str());
    const long long obs = (long long)C * H * W;
    if (obs >= (1LL << 30)) return a0_fail(A0_EINVAL, (w + ": an observation of 2^30 bytes or more").c_str());
    if (obs % 16 != 0) return a0_fail(A0_EINVAL, (w + ": C * H * W must be a multiple of 16 (16-byte loads and stores)").c_str());
    if (row_bytes != 2 * obs) return a0_fail(A0_EINVAL, (w + ": row_bytes != 2 * C * H * W (a row holds st || st_next and nothing else)").c_str());
    return A0_OK;
}

extern "C" int a0_augment_shift(const uint8_t* frames, const int* slot, long long row_bytes, int C, int H, int W, int pad, int B, unsigned long long seed,
                                const int* state, long long u_host, uint8_t* out, void* stream) {
    if (!frames || !out || B < 1) return a0_fail(A0_EINVAL, "a0_augment_shift: frames, out and B >= 1");
    const int rc = a0_augment_shift_check("a0_augment_shift", C, H, W, pad, row_bytes);
    if (rc != A0_OK) return rc;
    if ((((uintptr_t)frames) | ((uintptr_t)out)) & 15) return a0_fail(A0_EINVAL, "a0_augment_shift: frames and out must be 16-byte aligned");
    if (!state && u_host < 0) return a0_fail(A0_EINVAL, "a0_augment_shift: u_host < 0");
    const int obs = C * H * W;
    const dim3 grid(2u * (unsigned)B), block(256);
    hipStream_t st = (hipStream_t)stream;
    if (obs <= A0_AUG_LDS_BYTES)
        hipLaunchKernelGGL((a0_augment_shift_kernel<true>), grid, block, (size_t)obs, st, frames, slot, row_bytes, C, H, W, pad, B, seed, state, (unsigned long long)u_host, out);
    else
        hipLaunchKernelGGL((a0_augment_shift_kernel<false>), grid, block, 0, st, frames, slot, row_bytes, C, H, W, pad, B, seed, state, (unsigned long long)u_host, out);
    return a0_fail_hip((int)hipGetLastError(), "a0_augment_shift");
}
