// Nature-CNN encoder on gfx950: the a0_net object (geometry and gather tables) and the exported encoder entry points over the HIP backend of net_impl.h.  Every
// encoder-operand GEMM of the library is instantiated here; the dense layers are dense.hip's.
// Replaces the ATen -> cuDNN dispatches behind reference agent0/deepq/model.py:93-101 (ConvEncoder) and their autograd backward (agent.py:153-155).
#include "hip_backend.h"
#include "update_tail.h"

#include <vector>

// ------------------------------------------------------------------------------------------------ net object
struct a0_net {
    a0_net_core core;
    std::vector<void*> owned;
    ~a0_net() { for (void* p : owned) (void)hipFree(p); }
    template <class T> const T* upload(const std::vector<T>& v) {
        void* d = nullptr;
        A0_HIP_THROW(hipMalloc(&d, v.size() * sizeof(T)));
        owned.push_back(d);
        A0_HIP_THROW(hipMemcpy(d, v.data(), v.size() * sizeof(T), hipMemcpyHostToDevice));
        return (const T*)d;
    }
};

extern "C" int a0_net_create(const a0_net_desc* d, a0_net** out) {
    A0_TRY
    if (!d || !out) return a0_fail(A0_EINVAL, "a0_net_create: null argument");
    a0_net* n = new a0_net();
    if (!a0_net_core_init(n->core, d->C, d->H, d->W)) { delete n; return a0_fail(A0_EINVAL, "a0_net_create: observation too small for the 8/4, 4/2, 3/1 conv stack"); }
    a0_net_tables t;
    a0_net_build_tables(n->core, t);
    try {
        n->core.ktab1 = n->upload(t.ktab1); n->core.ktab2 = n->upload(t.ktab2); n->core.ktab3 = n->upload(t.ktab3);
        n->core.ktab_d3 = n->upload(t.ktab_d3); n->core.ktab_d2 = n->upload(t.ktab_d2);
        n->core.wtab_d3 = n->upload(t.wtab_d3);
        for (int i = 0; i < 4; ++i) n->core.wtab_d2[i] = n->upload(t.wtab_d2[i]);
    } catch (...) { delete n; throw; }
    *out = n;
    return A0_OK;
    A0_CATCH
}

extern "C" int a0_net_destroy(a0_net* n) { delete n; return A0_OK; }

extern "C" int a0_net_geometry(const a0_net* n, int* out8) {
    if (!n || !out8) return a0_fail(A0_EINVAL, "a0_net_geometry: null");
    const a0_net_core& c = n->core;
    out8[0] = c.H1; out8[1] = c.W1; out8[2] = c.H2; out8[3] = c.W2; out8[4] = c.H3; out8[5] = c.W3; out8[6] = c.feat; out8[7] = c.K1;
    return A0_OK;
}

extern "C" int a0_net_encoder_fwd(const a0_net* n, const a0_encoder_weights* w, const a0_frames_arg* f, int B,
                                  float* act1, float* act2, float* act3, void* stream) {
    A0_TRY
    if (!n || !w || !f || !f->frames || !act1 || !act2 || !act3 || B < 1) return a0_fail(A0_EINVAL, "a0_net_encoder_fwd: bad argument");
    a0_hip_backend bk{(hipStream_t)stream};
    a0_encoder_fwd_impl(bk, n->core, *w, *f, B, act1, act2, act3);
    return A0_OK;
    A0_CATCH
}

// the arguments the three backward entry points share; `who`: the entry point, under whose name the errors read
static int a0_encoder_bwd_check(const char* who, const a0_net* n, const a0_encoder_weights* w, const a0_frames_arg* f, int B, const float* act1, const float* act2, const float* d3,
                                const float* d2, const float* d1, const float* g1, const float* g2, const float* g3, bool more_ok, const float* slabs, const a0_pending_reduce* pend) {
    if (!n || !w || !f || !f->frames || !act1 || !act2 || !d3 || !d2 || !d1 || !g1 || !g2 || !g3 || B < 1 || !more_ok) return a0_fail(A0_EINVAL, (std::string(who) + ": null argument").c_str());
    if (a0_encoder_bwd_scratch_impl(n->core, B) > 0 && !slabs) return a0_fail(A0_EINVAL, (std::string(who) + ": needs slab scratch").c_str());
    if (pend && (pend->n < 0 || pend->n > 4)) return a0_fail(A0_EINVAL, (std::string(who) + ": bad pending reductions").c_str());
    return A0_OK;
}

extern "C" int a0_net_encoder_wgrad(const a0_net* n, const a0_encoder_weights* w, const a0_frames_arg* f, int B, const float* act1, const float* act2,
                                    const float* d3, const float* d2, const float* d1, float* g1, float* g2, float* g3, float* slabs, const a0_pending_reduce* pend,
                                    void* stream) {
    A0_TRY
    if (const int rc = a0_encoder_bwd_check("a0_net_encoder_wgrad", n, w, f, B, act1, act2, d3, d2, d1, g1, g2, g3, true, slabs, pend)) return rc;
    a0_hip_backend bk{(hipStream_t)stream};
    a0_encoder_bwd_impl(bk, n->core, *w, *f, B, act1, act2, d3, const_cast<float*>(d2), const_cast<float*>(d1), g1, g2, g3, slabs, false, pend);
    return A0_OK;
    A0_CATCH
}

__global__ void a0_tail_prep_kernel(a0_tail_prep P) {
    if (threadIdx.x == 0 && blockIdx.x == 0) a0_tail_prep_run(P);
}

extern "C" int a0_net_encoder_wgrad_tail(const a0_net* n, const a0_encoder_weights* w, const a0_frames_arg* f, int B, const float* act1, const float* act2,
                                         const float* d3, const float* d2, const float* d1, float* g1, float* g2, float* g3, float* slabs, const a0_pending_reduce* pend,
                                         a0_update_tail_plan* plan, int* state, float* scalars, double lr, double beta1, double beta2, int target_update_freq, void* stream) {
    A0_TRY
    if (const int rc = a0_encoder_bwd_check("a0_net_encoder_wgrad_tail", n, w, f, B, act1, act2, d3, d2, d1, g1, g2, g3, plan && state && scalars, slabs, pend)) return rc;
    const a0_tail_prep prep{state, scalars, lr, beta1, beta2, target_update_freq};
    a0_hip_backend bk{(hipStream_t)stream};
    bk.prep = &prep;
    a0_encoder_bwd_impl(bk, n->core, *w, *f, B, act1, act2, d3, const_cast<float*>(d2), const_cast<float*>(d1), g1, g2, g3, slabs, false, pend, plan);
    if (!bk.prep_done) {       // conv1's weight gradient was a GEMM launch: the bookkeeping goes out on its own
        hipLaunchKernelGGL(a0_tail_prep_kernel, dim3(1), dim3(1), 0, (hipStream_t)stream, prep);
        A0_HIP_THROW(hipGetLastError());
    }
    return A0_OK;
    A0_CATCH
}

extern "C" long long a0_net_encoder_bwd_scratch(const a0_net* n, int B) { return n ? a0_encoder_bwd_scratch_impl(n->core, B) : 0; }

extern "C" int a0_net_encoder_bwd(const a0_net* n, const a0_encoder_weights* w, const a0_frames_arg* f, int B,
                                  const float* act1, const float* act2, const float* d3, float* d2, float* d1,
                                  float* g1, float* g2, float* g3, float* slabs, void* stream) {
    A0_TRY
    if (const int rc = a0_encoder_bwd_check("a0_net_encoder_bwd", n, w, f, B, act1, act2, d3, d2, d1, g1, g2, g3, true, slabs, nullptr)) return rc;
    a0_hip_backend bk{(hipStream_t)stream};
    a0_encoder_bwd_impl(bk, n->core, *w, *f, B, act1, act2, d3, d2, d1, g1, g2, g3, slabs);
    return A0_OK;
    A0_CATCH
}
