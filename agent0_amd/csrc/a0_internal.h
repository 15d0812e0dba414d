// Internal helpers shared by the .hip translation units: error plumbing for the C-ABI.
#pragma once
#include "../../include/agent0_hip.h"
#include "a0_defs.h"

#include <exception>
#if defined(__HIPCC__)
#include <hip/hip_ext.h>
#endif
#include <stdexcept>
#include <string>

int a0_fail(int code, const char* msg);          // records the thread-local message, returns code
int a0_fail_hip(int hip_error, const char* what);

struct a0_hip_error : std::runtime_error {
    int err;
    a0_hip_error(int e, const std::string& w) : std::runtime_error(w), err(e) {}
};

#define A0_STR2(x) #x
#define A0_STR(x) A0_STR2(x)
#define A0_HIP_THROW(expr)                                                                                  \
    do {                                                                                                    \
        hipError_t a0_e_ = (expr);                                                                          \
        if (a0_e_ != hipSuccess) throw a0_hip_error((int)a0_e_, std::string(__FILE__ ":" A0_STR(__LINE__) ": ") + hipGetErrorString(a0_e_)); \
    } while (0)

#define A0_TRY try {
#define A0_CATCH                                                   \
    }                                                              \
    catch (const a0_hip_error& e) { return a0_fail_hip(e.err, e.what()); } \
    catch (const std::exception& e) { return a0_fail(A0_EINVAL, e.what()); } \
    catch (...) { return a0_fail(A0_EINVAL, "unknown C++ exception"); }

// at most 2048 workgroups of 256 lanes, grid-stride behind that
static inline unsigned a0_grid_256(long long items) { const long long b = (items + 255) / 256; return (unsigned)(b > 2048 ? 2048 : b < 1 ? 1 : b); }
// every one of these pointers is a multiple of `bytes` (a power of two); a null pointer counts as aligned
template <class... P>
static inline bool a0_aligned(unsigned bytes, const P*... p) { return ((((uintptr_t)p) | ... | (uintptr_t)0) & (bytes - 1)) == 0; }

// Philox stream ids (agent0_amd/common/utils.py DeviceRng: 1 / 2 epsilon-greedy, 3 quantile fractions, 4 NoisyNet, 5 sum-tree, 6 permutation seeds); 7 = the
// random shifts of learner.aug_shift (augment.hip), positioned by the update count alone: no running offset, nothing to snapshot
#define A0_STREAM_AUG 7
// 8 = the fresh values of learner.net_reset_freq (net_reset.hip: a0_net_reset), positioned by (reset number, flat index): no running offset either
#define A0_STREAM_RESET 8
// 9 = the fresh values of learner.redo_freq (net_reset.hip: a0_redo_recycle), positioned by (recycle number, flat index): no running offset
#define A0_STREAM_REDO 9
// augment.hip: the range checks of a0_augment_shift (A0_EINVAL with a message that starts with `who`)
int a0_augment_shift_check(const char* who, int C, int H, int W, int pad, long long row_bytes);
// quantile.hip: learner.iqn.risk's (kind, eta) as every entry point and both handles' setters check them (A0_EINVAL with a message that starts with `who`)
int a0_risk_check(const char* who, int kind, double eta);

// roctx ranges (core.hip): no-ops unless A0_ROCTX=1
void a0_trace_push_internal(const char* name);
void a0_trace_pop_internal();
struct a0_trace_scope {
    explicit a0_trace_scope(const char* name) { a0_trace_push_internal(name); }
    ~a0_trace_scope() { a0_trace_pop_internal(); }
    a0_trace_scope(const a0_trace_scope&) = delete;
    a0_trace_scope& operator=(const a0_trace_scope&) = delete;
};

#if defined(__HIPCC__)
// ---- core.hip: the process-wide GEMM switches (a0_gemm_mode(-1) reads the mode: 1 = split-operand kernels, 0 = fp32 chain)
int a0_x9_products_now();      // 6 or 9 cross products in the split-operand kernels (a0_x9_products)
// ---- probe.hip: the profiler probe, HIP events on launches tagged `tag` (A0_TAG_*, a0_defs.h).  Two forms.
// Carried, for launches of ONE kernel: the probe hands out its next event pair and the launch carries it (hipExtLaunchKernelGGL: the events take the
// dispatch's own begin / end timestamps, what rocprofv3's kernel trace reports) — an event recorded in front of a launch also counts the ~2.5 us between the
// previous kernel's end and this one's first wave.
bool a0_probe_events(int tag, hipEvent_t* start, hipEvent_t* stop);
void a0_probe_commit(double flops);
bool a0_probe_active();        // a probe is armed, whatever its tag
#define A0_LAUNCH_PROBED(tag, flops, kern, grid, block, lds, st, ...)                                                              \
    do {                                                                                                                           \
        hipEvent_t a0_e0_ = nullptr, a0_e1_ = nullptr;                                                                             \
        if (a0_probe_events((tag), &a0_e0_, &a0_e1_)) {                                                                            \
            hipExtLaunchKernelGGL(kern, grid, block, (uint32_t)(lds), st, a0_e0_, a0_e1_, 0, __VA_ARGS__);                         \
            a0_probe_commit(flops);                                                                                                \
        } else                                                                                                                     \
            hipLaunchKernelGGL(kern, grid, block, lds, st, __VA_ARGS__);                                                           \
    } while (0)
// Bracket, for launchers that cannot carry the pair: made in front of the launch (start event), stop(flops) behind it (stop event, commit); never stopped: nothing committed
struct a0_probe_bracket {
    hipStream_t st; hipEvent_t e0 = nullptr, e1 = nullptr; bool on;
    a0_probe_bracket(int tag, hipStream_t s) : st(s), on(a0_probe_events(tag, &e0, &e1)) { if (on) A0_HIP_THROW(hipEventRecord(e0, st)); }
    void stop(double flops) { if (on) { A0_HIP_THROW(hipEventRecord(e1, st)); a0_probe_commit(flops); } }
};
// ---- conv1_wgrad.hip: per-observation conv1 weight gradient on the bf16 pipe; returns the slab count (0 = unsupported shape)
// prep (optional, update_tail.h): the optimizer step's one-thread bookkeeping, done by the launch's first workgroup when its slab is written
struct a0_tail_prep; struct a0_net_core;
int a0_conv1_wgrad_fused_launch(const a0_frames_arg* f, int C, int H, int W, int B, const float* d1, float* slabs, const a0_tail_prep* prep, hipStream_t st);
// ---- conv23_wgrad.hip: per-observation conv2 + conv3 weight gradients on the bf16 pipe (one launch); returns 1 if it ran, 0 = unsupported shape
int a0_conv23_wgrad_fused_launch(const a0_net_core& n, int B, const float* act1, const float* act2, const float* d2, const float* d3, float* slab2, float* slab3,
                                 hipStream_t st);
// ---- dense.hip: fc1 of a scalar-head actor step, [splits][E][512] slabs into scratch — the dedicated kernel over pre-split, fragment-ordered weights (actor_fc1.hip;
// w1_planes = a0_actor_fc1_planes of W1, or null) where it applies, the same slabs bit for bit, else the general split-K GEMM
int a0_actor_fc1_slabs(const float* feat, int K, const float* W1, const unsigned int* w1_planes, int E, int splits, float* scratch, hipStream_t st);
int a0_splits_check(const char* who, int splits, int K);      // a caller-given split count: A0_OK, or A0_EINVAL behind a message that starts with `who`
// ---- actor_tail.hip: one actor step's tail + synthetic env step in ONE launch, behind the descriptors of actor_step.h (the exported a0_actor_*_env_step* pack them,
// a0_actor_rollout fills them once per step).  next (optional): the kernel goes on to encode the env's new observation; the *_enc entry points, whose names the errors then take.
struct a0_step_draw; struct a0_env_commit; struct a0_next_enc; struct a0_slab_head;
// scalar heads (dqn / mdqn): fc1 over `feat` (a0_actor_fc1_slabs), then the tail kernel
int a0_actor_qhead_env_launch(const float* feat, int E, int K, const float* W1, const float* b1, const float* W2, const float* b2, int A, int dueling, float* scratch,
                              const a0_step_draw& draw, const a0_env_commit& env, const a0_next_enc* next, const unsigned int* w1_planes, hipStream_t st);
// the tails over the head GEMM's slabs (c51 / qr: head.kt = 0, iqn / fqf: head.kt = 1)
int a0_actor_slab_tail_env_launch(const a0_slab_head& head, int E, const a0_step_draw& draw, const a0_env_commit& env, const a0_next_enc* next, hipStream_t st);
// the same tails without the env step (actor steps over host environments): a0_actor_dist_tail / a0_actor_quantile_tail behind the descriptors
int a0_actor_slab_tail_launch(const a0_slab_head& head, int E, const a0_step_draw& draw, hipStream_t st);
#endif
