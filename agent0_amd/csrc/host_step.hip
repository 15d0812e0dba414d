// The ingest half of a host-environment step in ONE launch (gfx950).  Once a step's newest frames, scalars and whole stacks have been
// DMA'd to the device (a0_env_pool_upload with prev = NULL), this kernel does what Actor._rollout_host / HostEnvPool._upload issue as about six launches and copies:
//   frame stack      out[e] = prev[e][1:] ‖ newest[e] where advance[e] != 0 (a0_frame_stack_kernel's rule; rows with advance 0 were uploaded whole into out)
//   n-step window    nstep.h, the body a0_nstep_kernel runs (fp64 R, done = (terminal | life_loss) & ~truncated, ring entry at steps % n)
//   replay row       slot (start + e) % cap: st = prev[e] (n = 1) or the observation ring's oldest entry (n > 1), st_next = out[e]; act / rew / done
//   observation ring (n > 1) ring_obs[steps % ring_len][e] = prev[e]   (agent.py keeps the last n observations for the n-step transition's st)
//   statistics       stat_mask[e] / stat_ret[e] = the step's final-mask and final-return scalars
// The new stack goes to the observation buffer and to the row's st_next half from the same registers; nothing is read back.  Pure data movement: per env it
// reads prev (+ the ring's oldest entry for n > 1) and the newest frame, and writes out, the 2 x obs_bytes row (and the ring entry for n > 1).
#include "a0_internal.h"
#include "nstep.h"

#pragma clang fp contract(off)

// scalar rows of a host step (env_pool.N_SCAL = 7): reward, terminated, truncated, life_loss, final mask, final return, advance
enum { A0_SCAL_REW = 0, A0_SCAL_TERM, A0_SCAL_TRUNC, A0_SCAL_LIFE, A0_SCAL_FMASK, A0_SCAL_FRET, A0_SCAL_ADV, A0_N_SCAL };

// grid (columns, E): one workgroup row per env, 16 bytes per lane; blockIdx.x splits the stack into columns so that small batches still spread over the CUs
__global__ __launch_bounds__(256) void a0_host_step_ingest_kernel(const uint4* __restrict__ prev, const uint4* __restrict__ newest, const float* __restrict__ scal,
                                                                   uint4* __restrict__ out, int E, int nstack, int fv, int use_life, const int* __restrict__ action,
                                                                   int n, int ring_len, long long steps, double gamma, int* __restrict__ ring_act,
                                                                   float* __restrict__ ring_rew, float* __restrict__ ring_done, uint4* __restrict__ ring_obs,
                                                                   uint4* __restrict__ frames, long long cap, long long start, int* __restrict__ r_act,
                                                                   float* __restrict__ r_rew, float* __restrict__ r_done, float* __restrict__ stat_mask,
                                                                   float* __restrict__ stat_ret, const long long* __restrict__ ctrl) {
    const int e = blockIdx.y;
    if (ctrl) { steps += ctrl[A0_CTRL_ACTOR_STEPS]; start += ctrl[A0_CTRL_REPLAY_SLOT]; }
    const long long slot = (start + e) % cap;
    const bool adv = scal[(long long)A0_SCAL_ADV * E + e] != 0.f;
    const int total = nstack * fv, keep = (nstack - 1) * fv;
    const uint4* p = prev + (long long)e * total;
    const uint4* nw = newest + (long long)e * fv;
    uint4* o = out + (long long)e * total;
    uint4* row = frames + slot * 2 * total;
    // n > 1: this step's observation enters the ring at steps % ring_len; st is the entry of the transition's first step (this very observation while the
    // window holds one step)
    uint4* ring_w = nullptr;
    const uint4* st = p;
    if (n > 1) {
        const long long count = steps + 1 < n ? steps + 1 : n;
        const long long rs = steps % ring_len, oldest = (steps - (count - 1)) % ring_len;
        ring_w = ring_obs + (rs * E + e) * total;
        if (oldest != rs) st = ring_obs + (oldest * E + e) * total;
    }
    for (int i = blockIdx.x * 256 + threadIdx.x; i < total; i += gridDim.x * 256) {
        const uint4 c = p[i];
        uint4 v;
        if (adv) {
            v = i < keep ? p[i + fv] : nw[i - keep];
            o[i] = v;
        } else {
            v = o[i];
        }
        row[total + i] = v;
        if (ring_w) ring_w[i] = c;
        row[i] = st[i];      // (a select between c and st[i] here makes the compiler spill c to scratch to load it through a pointer)
    }
    if (blockIdx.x == 0 && threadIdx.x == 0) {
        a0_nstep_env(e, E, n, steps, gamma, action[e], scal[(long long)A0_SCAL_REW * E + e], scal[(long long)A0_SCAL_TERM * E + e],
                     scal[(long long)A0_SCAL_TRUNC * E + e], use_life ? scal[(long long)A0_SCAL_LIFE * E + e] : 0.f, ring_act, ring_rew, ring_done,
                     r_act + slot, r_rew + slot, r_done + slot);
        stat_mask[e] = scal[(long long)A0_SCAL_FMASK * E + e];
        stat_ret[e] = scal[(long long)A0_SCAL_FRET * E + e];
    }
}

extern "C" int a0_host_step_ingest(const uint8_t* prev, const uint8_t* newest, const float* scal, uint8_t* out, int E, int nstack, long long frame_bytes,
                                   int use_life_loss, const int* action, int n, int ring_len, long long steps, double gamma, int* ring_act, float* ring_rew,
                                   float* ring_done, uint8_t* ring_obs, uint8_t* frames, long long cap, long long start_slot, int* r_act, float* r_rew,
                                   float* r_done, float* stat_mask, float* stat_ret, const long long* ctrl, void* stream) {
    if (!prev || !newest || !scal || !out || prev == out || !action || !ring_act || !ring_rew || !ring_done || !frames || !r_act || !r_rew || !r_done ||
        !stat_mask || !stat_ret || E < 1 || nstack < 2 || frame_bytes < 16 || (frame_bytes % 16) || n < 1 || steps < 0 || cap < E || start_slot < 0 ||
        (n > 1 && (!ring_obs || ring_len < n)) || ((long long)nstack * frame_bytes) / 16 > 0x7fffffffLL ||
        ((((uintptr_t)prev) | ((uintptr_t)newest) | ((uintptr_t)out) | ((uintptr_t)frames) | ((uintptr_t)ring_obs)) % 16))
        return a0_fail(A0_EINVAL, "a0_host_step_ingest: bad argument (frames of a multiple of 16 bytes, 16-byte aligned, out != prev, cap >= E, ring_len >= n > 1 with a ring)");
    const int fv = (int)(frame_bytes / 16), total = nstack * fv;
    int gx = (total + 255) / 256; if (gx > 8) gx = 8;
    hipLaunchKernelGGL(a0_host_step_ingest_kernel, dim3(gx, E), dim3(256), 0, (hipStream_t)stream, (const uint4*)prev, (const uint4*)newest, scal, (uint4*)out, E,
                       nstack, fv, use_life_loss ? 1 : 0, action, n, n > 1 ? ring_len : 1, steps, gamma, ring_act, ring_rew, ring_done, (uint4*)ring_obs, (uint4*)frames,
                       cap, start_slot % cap, r_act, r_rew, r_done, stat_mask, stat_ret, ctrl);
    return a0_fail_hip((int)hipGetLastError(), "a0_host_step_ingest");
}
