// The profiler probe: bench.py times every launch of ONE tagged family (A0_TAG_*, a0_defs.h) with HIP events on the stream the kernel runs on, so that its
// average duration (and hence achieved FLOP/s against the fp32 MFMA roofline) is measured live inside the timed region.  The launch sites reach it through
// a0_probe_events / a0_probe_commit (the pair travels in the launch), a0_probe_bracket (the pair is recorded around it) and a0_probe_active: a0_internal.h.
#include "a0_internal.h"

#include <vector>

struct a0_probe_t {
    int tag = 0;
    std::vector<hipEvent_t> ev;     // pairs: start, stop
    size_t used = 0;
    double flops = 0.0;
};
static a0_probe_t g_probe;

bool a0_probe_active() { return g_probe.tag != 0; }

bool a0_probe_events(int tag, hipEvent_t* start, hipEvent_t* stop) {
    if (g_probe.tag == 0 || g_probe.tag != tag || g_probe.used + 2 > g_probe.ev.size()) return false;
    *start = g_probe.ev[g_probe.used]; *stop = g_probe.ev[g_probe.used + 1];
    return true;
}
void a0_probe_commit(double flops) { g_probe.used += 2; g_probe.flops += flops; }

extern "C" int a0_probe_begin(int tag, int max_launches) {
    A0_TRY
    for (hipEvent_t e : g_probe.ev) (void)hipEventDestroy(e);
    g_probe.ev.clear();
    g_probe.used = 0; g_probe.flops = 0.0; g_probe.tag = 0;
    if (tag <= 0 || max_launches <= 0) return A0_OK;
    g_probe.ev.resize(2 * (size_t)max_launches);
    for (auto& e : g_probe.ev) A0_HIP_THROW(hipEventCreate(&e));
    g_probe.tag = tag;
    return A0_OK;
    A0_CATCH
}

// host_out3: [launches, total milliseconds, total algorithmic FLOP]; synchronises on the recorded events
extern "C" int a0_probe_end(double* host_out3) {
    A0_TRY
    if (!host_out3) return a0_fail(A0_EINVAL, "a0_probe_end: null");
    double ms = 0.0;
    for (size_t i = 0; i + 1 < g_probe.used; i += 2) {
        A0_HIP_THROW(hipEventSynchronize(g_probe.ev[i + 1]));
        float t = 0.f;
        A0_HIP_THROW(hipEventElapsedTime(&t, g_probe.ev[i], g_probe.ev[i + 1]));
        ms += t;
    }
    host_out3[0] = (double)(g_probe.used / 2); host_out3[1] = ms; host_out3[2] = g_probe.flops;
    g_probe.tag = 0;
    return A0_OK;
    A0_CATCH
}
