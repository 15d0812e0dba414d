// a0_learner: one DQN-family learner — online + target parameters, gradients, Adam moments and every workspace — as ONE opaque handle whose HBM the
// library owns, and BaseLearner.train (reference agent0/deepq/agent.py:124-169 with DQNLearner.train_step 173-190 behind it) as ONE C call per update.
//
// Everything a0_learner_update does is a sequence of the entry points declared above it in include/agent0_hip.h, in exactly the order
// agent0_amd/deepq/engine.py issues them for the same configuration (so the two are bit-identical: tests/test_gpu_engine.py::test_native_learner_...);
// what this file adds is the part a non-Python host would otherwise have to re-implement: the packed parameter layout (deepq/layout.py), buffer
// sizes, split-K slab bookkeeping and the call order.  SURVEY.md §8(b) "ownership": opaque handle, library-owned HBM, caller passes borrowed device
// pointers valid for the call, no allocation and no host synchronisation after a0_learner_create.
//
// Scope: on 4 x 84 x 84 observations, the scalar-head learners (dqn; dueling; double-Q; n-step through discount^n) — BASELINE configs[1], the bench line — and
// the categorical one (c51, also with NoisyLinear layers: BASELINE configs[2], rainbow-lite), the implicit quantile network (configs[3]) and the fully
// parameterised quantile function (configs[4]), plus qr and mdqn: the reference's six learners.
//
// The update's stages are named after the methods of engine.py::DeviceLearner they mirror; the family (a0_family, learner_state.h) is decided once, in a0_learner_layout.
#include "learner_state.h"
#include "head_loss.h"      // a0_hl_gauss_check

extern "C" int a0_learner_create(const a0_learner_desc* d, a0_learner** out) { return a0_learner_create_on(d, nullptr, out); }

extern "C" int a0_learner_set_rng(a0_learner* L, int stream_id, unsigned long long offset) {
    if (!L || stream_id < 0 || stream_id > 7 || (offset & 3)) return a0_fail(A0_EINVAL, "a0_learner_set_rng: stream 0..7, offset a multiple of four");
    L->rng.off[stream_id] = offset;
    return A0_OK;
}

// the learner's Philox state for resumable runs: words[0] = seed, words[1 .. 8] = the running offsets of streams 0 .. 7; set != 0 writes it into the handle
extern "C" int a0_learner_rng_state(a0_learner* L, unsigned long long* words, int set) {
    if (!L || !words) return a0_fail(A0_EINVAL, "a0_learner_rng_state: null argument");
    if (set) {
        for (int i = 0; i < 8; ++i) if (words[1 + i] & 3) return a0_fail(A0_EINVAL, "a0_learner_rng_state: offsets are multiples of four");
        L->rng.seed = words[0];
        for (int i = 0; i < 8; ++i) L->rng.off[i] = words[1 + i];
    } else {
        words[0] = L->rng.seed;
        for (int i = 0; i < 8; ++i) words[1 + i] = L->rng.off[i];
    }
    return A0_OK;
}

// ---- a0_learner_create_on, part 1: what a description is refused for, before anything is allocated
static int a0_learner_desc_check(const a0_learner_desc* d, const a0_learner_buffers* bufs, a0_learner** out) {
    if (!d || !out) return a0_fail(A0_EINVAL, "a0_learner_create: null argument");
    if (bufs && bufs->loss_ring && bufs->loss_ring_cap < 1) return a0_fail(A0_EINVAL, "a0_learner_create_on: loss_ring_cap");
    if (d->A < 1 || d->B < 1 || d->n_step < 1 || !(d->discount > 0.0) || !(d->lr >= 0.0) || d->target_update_freq < 1 ||
        (d->algo != A0_ALGO_DQN && d->algo != A0_ALGO_C51 && d->algo != A0_ALGO_IQN && d->algo != A0_ALGO_FQF && d->algo != A0_ALGO_QR && d->algo != A0_ALGO_MDQN))
        return a0_fail(A0_EINVAL, "a0_learner_create: bad description");
    if (d->algo == A0_ALGO_QR && (d->num_atoms < 1 || d->num_atoms > 1024)) return a0_fail(A0_EINVAL, "a0_learner_create: qr needs 1 <= num_atoms <= 1024");
    if (d->algo == A0_ALGO_MDQN && !(d->mdqn_tau > 0.0)) return a0_fail(A0_EINVAL, "a0_learner_create: mdqn needs tau > 0");
    if (d->algo == A0_ALGO_FQF && (d->fqf_F < 2 || d->fqf_F > 32 || d->A + (d->dueling ? 1 : 0) > 32)) return a0_fail(A0_EINVAL, "a0_learner_create: fqf needs 2 <= F <= 32, A + dueling <= 32");
    if (d->algo == A0_ALGO_IQN && (d->iqn_K < 1 || d->iqn_N < 1 || d->iqn_N_dash < 1 || d->A + (d->dueling ? 1 : 0) > 32)) return a0_fail(A0_EINVAL, "a0_learner_create: iqn needs K, N, N' >= 1, A + dueling <= 32");
    if (d->algo == A0_ALGO_DQN && d->A + (d->dueling ? 1 : 0) > 24) return a0_fail(A0_EINVAL, "a0_learner_create: the dqn handle covers scalar heads with A + dueling <= 24 actions");
    if (d->algo == A0_ALGO_C51 && (d->num_atoms < 2 || d->num_atoms > 64 || !(d->vmax > d->vmin))) return a0_fail(A0_EINVAL, "a0_learner_create: c51 needs 2 <= num_atoms <= 64 and vmin < vmax");
    return A0_OK;
}

// ---- part 2: the head's dimensions, the family, the packed parameter layout (deepq/layout.py) and NoisyNet's noise modules
static void a0_learner_layout(a0_learner* L) {
    const a0_learner_desc* d = &L->d;
    L->T = (d->algo == A0_ALGO_C51 || d->algo == A0_ALGO_QR) ? d->num_atoms : 1;
    L->Nq = d->A * L->T; L->V = d->dueling ? L->T : 0; L->NQ = d->A + (d->dueling ? 1 : 0);
    L->Npad = (int)ceil_to(L->Nq + L->V, 32);
    L->gamma_n = (float)std::pow(d->discount, (double)d->n_step);
    const int Ron = d->double_q ? 2 * d->B : d->B;
    switch (d->algo) {
        case A0_ALGO_C51: L->fam = A0_FAM_DIST; break;
        case A0_ALGO_QR:       // c51's layer structure when a sample's staged head outputs fit in LDS (engine.py::_qr_fused_ok)
            L->fam = d->A <= 32 && (3LL * L->Npad + ceil_to(L->T, 4)) * 4 <= 150 * 1024 &&
                     std::max(a0_dense_fwd_partial_slabs(Ron, L->Npad, 512), a0_dense_fwd_partial_slabs(d->B, L->Npad, 512)) <= 8 ? A0_FAM_DIST : A0_FAM_LAYERWISE;
            break;
        case A0_ALGO_MDQN: L->fam = L->NQ <= 24 ? A0_FAM_SCALAR : A0_FAM_LAYERWISE; break;      // dqn's structure when the scalar-head kernel covers the action set
        case A0_ALGO_IQN: L->fam = A0_FAM_IQN; break; case A0_ALGO_FQF: L->fam = A0_FAM_FQF; break;
        default: L->fam = A0_FAM_SCALAR;
    }
    long long off = 0;
    auto add = [&](Blk& b, int N, int K) { b = Blk{off, N, K}; off += b.size(); };
    add(L->conv1, 32, L->C * 64); add(L->conv2, 64, 512); add(L->conv3, 64, 576);
    if (d->noisy) { add(L->fc1, 512, L->feat); add(L->fc1_sigma, 512, L->feat); add(L->head, L->Npad, 512); add(L->head_sigma, L->Npad, 512); }
    else { add(L->fc1, 512, L->feat); add(L->head, L->Npad, 512); }
    if (L->fam == A0_FAM_IQN || L->fam == A0_FAM_FQF) add(L->cos, L->feat, 64);      // the quantile family: cosine-embedding heads over B * n_tau rows
    L->n_adam = off;
    if (L->fam == A0_FAM_FQF) { add(L->frac, 32, L->feat); L->F = d->fqf_F; }  // behind the Adam range: its own RMSprop step (agent.py:139-148)
    L->n_pad = ceil_to(off, 4);
    if (!d->noisy) return;
    // composed weights [fc1 | head] per network; noise vectors per NoisyLinear module in the reference's module order (first_dense, q_head, value_head), each
    // (noise_in, noise_out_weight, noise_out_bias) padded to four floats — the layout one Philox fill of the whole buffer reproduces (engine.py DeviceNet)
    L->eff_fc1 = Blk{0, 512, L->feat}; L->eff_head = Blk{L->eff_fc1.size(), L->Npad, 512};
    L->n_eff = L->eff_fc1.size() + L->eff_head.size();
    long long no = 0;
    auto mod = [&](int block, int r0, int r1, int in_f) {
        a0_noise_mod m{block, r0, r1, in_f, 0, 0, 0};
        m.off_in = no; no += ceil_to(in_f, 4); m.off_w = no; no += ceil_to(r1 - r0, 4); m.off_b = no; no += ceil_to(r1 - r0, 4);
        L->mods[L->n_mods++] = m;
    };
    mod(0, 0, 512, L->feat); mod(1, 0, L->Nq, 512);
    if (d->dueling) mod(1, L->Nq, L->Nq + L->V, 512);
    L->noise_len = no;
}

// ---- part 3: the workspaces.  What every family has: parameters and optimizer state (the caller's where given), activations, gradients, slab scratch, NoisyNet's buffers
static int a0_ws_common(a0_learner* L, const a0_learner_buffers& U) {
    const a0_learner_desc* d = &L->d; const int B = d->B;
    const bool fqf = L->fam == A0_FAM_FQF, quantile = fqf || L->fam == A0_FAM_IQN;
    L->wt_floats = a0_net_conv_wt_floats(L->C);
    L->online = U.online ? U.online : L->alloc<float>(L->n_pad, true); L->target = U.target ? U.target : L->alloc<float>(L->n_pad, true);
    L->grads = U.grads ? U.grads : L->alloc<float>(L->n_pad + 4, true);
    L->m = U.adam_m ? U.adam_m : L->alloc<float>(L->n_pad, true); L->v = U.adam_v ? U.adam_v : L->alloc<float>(L->n_pad, true);
    L->state = U.state ? U.state : L->alloc<int>(8, true); L->scalars = U.scalars ? U.scalars : L->alloc<float>(4, true);
    L->loss_ring = U.loss_ring ? U.loss_ring : L->alloc<float>(1024, true); L->loss_ring_cap = U.loss_ring ? U.loss_ring_cap : 1024;
    L->wt_on = U.wt_online ? U.wt_online : L->alloc<float>(L->wt_floats, true); L->wt_tg = U.wt_target ? U.wt_target : L->alloc<float>(L->wt_floats, true);
    L->act1 = L->alloc<float>((long long)B * L->H1 * L->W1 * 32); L->act2 = L->alloc<float>((long long)B * L->H2 * L->W2 * 64);
    L->act3_t = L->alloc<float>((long long)B * L->feat); L->ns_fc1 = a0_dense_fwd_partial_slabs(B, 512, L->feat);
    if (L->fam != A0_FAM_DIST) {
        // the passes' features kept apart: online on s, and a third pass's (online on s' under double-Q; the target network's on the CURRENT observation for mdqn
        // from the fc1 slabs) — with the passes' fc1 slabs, h(s) of the online network and (mdqn) target(obs).  a0_ws_dist has its own, back to back
        const bool mdqn = L->fam == A0_FAM_SCALAR && d->algo == A0_ALGO_MDQN, third = d->double_q || mdqn;
        L->act3_o = L->alloc<float>((long long)B * L->feat);
        if (third) L->act3_s = L->alloc<float>((long long)B * L->feat);
        for (int i = 0; i < (third ? 3 : 2); ++i) L->fc1_slabs[i] = L->alloc<float>((long long)L->ns_fc1 * B * 512);
        L->h = L->alloc<float>((long long)B * 512);
        if (mdqn) L->q_cur = L->alloc<float>((long long)B * d->A);
    }
    L->q_o = L->alloc<float>((long long)B * d->A * L->T); L->q_t = L->alloc<float>((long long)B * d->A * L->T);
    const long long Rg = fqf ? (long long)B * d->fqf_F : (quantile ? (long long)B * d->iqn_N : (long long)B);           // rows of the differentiated pass
    L->draw = L->alloc<float>(Rg * L->Npad); L->dh = L->alloc<float>(Rg * 512); L->d3 = L->alloc<float>((long long)B * L->feat);
    L->d2 = L->alloc<float>((long long)B * L->H2 * L->W2 * 64); L->d1 = L->alloc<float>((long long)B * L->H1 * L->W1 * 32); L->loss = L->alloc<float>(B);
    // one slab scratch for the dense weight gradients (disjoint regions, one reduction launch) and, after them, the encoder's
    const long long s_head = ceil_to(a0_dense_wgrad_scratch((int)Rg, L->Npad, 512), 4), s_fc1 = ceil_to(a0_dense_wgrad_scratch((int)Rg, 512, L->feat), 4);
    const long long s_cos = quantile ? ceil_to(a0_dense_wgrad_scratch((int)Rg, L->feat, 64), 4) : 0;
    L->slab_off[0] = 0; L->slab_off[1] = s_head;
    L->slab_off3[0] = 0; L->slab_off3[1] = s_head; L->slab_off3[2] = s_head + s_fc1;
    // (the dense layers' slab reductions ride in the encoder's reduction launch, a0_pending_reduce: the encoder's slabs start behind theirs)
    L->enc_slab_off = s_head + s_fc1 + s_cos;
    long long n_slab = L->enc_slab_off + a0_net_encoder_bwd_scratch(L->net, B);
    if (fqf && a0_dense_wgrad_scratch(B, 32, L->feat) > n_slab) n_slab = a0_dense_wgrad_scratch(B, 32, L->feat);
    L->slabs = L->alloc<float>(n_slab > 4 ? n_slab : 4);
    if (!d->noisy) return A0_OK;
    L->eff_on = U.eff_online ? U.eff_online : L->alloc<float>(L->n_eff, true); L->eff_tg = U.eff_target ? U.eff_target : L->alloc<float>(L->n_eff, true);
    if (U.noise) { L->noise = U.noise; return A0_OK; }      // the caller's vectors as they are; its stream position comes through a0_learner_set_rng
    L->noise = L->alloc<float>(2 * L->noise_len, true);
    // BaseLearner.__init__ builds the online and the target network, and a NoisyLinear draws its first noise when it is built (model.py:44-52): the two
    // networks' first draws come off the learner's stream here, so that the updates' draws continue where the Python classes' do
    const unsigned long long o = L->rng.reserve(STREAM_NOISE, L->noise_len);
    (void)L->rng.reserve(STREAM_NOISE, L->noise_len);
    A0_CHECK(a0_rng_normal(L->rng.seed, 4, o, 0.1f, L->noise, 2 * L->noise_len, nullptr));
    A0_HIP_THROW(hipDeviceSynchronize());
    return A0_OK;
}

static void a0_ws_qr_taus(a0_learner* L) {      // agent.py:274: the quantile midpoints
    std::vector<float> t((size_t)L->T);
    for (int i = 0; i < L->T; ++i) t[(size_t)i] = (2.0f * (float)i + 1.0f) / (2.0f * (float)L->T);
    A0_HIP_THROW(hipMemcpy(L->qr_taus = L->alloc<float>(L->T), t.data(), (size_t)L->T * 4, hipMemcpyHostToDevice));
}

// c51, and qr from the head slabs: the online network's features of s and (double-Q) of s' back to back — fc1 and the head run over both as ONE GEMM each (same weights)
static void a0_ws_dist(a0_learner* L) {
    const a0_learner_desc* d = &L->d; const int B = d->B;
    L->R_on = d->double_q ? 2 * B : B;
    L->ns_on = a0_dense_fwd_partial_slabs(L->R_on, 512, L->feat); L->nh_on = a0_dense_fwd_partial_slabs(L->R_on, L->Npad, 512);
    L->nh_tg = a0_dense_fwd_partial_slabs(B, L->Npad, 512);
    L->act3_o = L->act3_on = L->alloc<float>((long long)L->R_on * L->feat);
    if (d->double_q) L->act3_s = L->act3_on + (long long)B * L->feat;
    L->fc1_on = L->alloc<float>((long long)L->ns_on * L->R_on * 512); L->fc1_tg = L->alloc<float>((long long)L->ns_fc1 * B * 512);
    L->h_on = L->alloc<float>((long long)L->R_on * 512); L->h_tg = L->alloc<float>((long long)B * 512);
    L->h = L->h_on;                                  // h(s) of the online network: what the backward pass reads
    L->hs_on = L->alloc<float>((long long)L->nh_on * L->R_on * L->Npad); L->hs_tg = L->alloc<float>((long long)L->nh_tg * B * L->Npad);
    L->a_star = L->alloc<int>(B, true);
    if (d->algo == A0_ALGO_QR) { a0_ws_qr_taus(L); return; }
    L->atoms = L->alloc<float>(L->T); L->m_proj = L->alloc<float>((long long)B * L->T);
    // torch.linspace(vmin, vmax, T) in fp32 as ATen's vectorised CPU kernel computes it (RangeFactories: step = (end - start) / (steps - 1); fma(step, i, start)
    // below the middle, fma(-step, steps - 1 - i, end) above).  A host whose torch build rounds differently hands its own values to a0_learner_set_support.
    std::vector<float> at((size_t)L->T);
    const float lo = (float)d->vmin, hi = (float)d->vmax, step = (hi - lo) / (float)(L->T - 1);
    for (int i = 0; i < L->T; ++i) at[(size_t)i] = i < L->T / 2 ? std::fmaf(step, (float)i, lo) : std::fmaf(-step, (float)(L->T - 1 - i), hi);
    A0_HIP_THROW(hipMemcpy(L->atoms, at.data(), (size_t)L->T * 4, hipMemcpyHostToDevice));
}

// qr and mdqn head by head: per pass fc1 output, raw head output and combined head output, over the common buffers where one exists
static void a0_ws_layerwise(a0_learner* L) {
    const a0_learner_desc* d = &L->d; const int B = d->B;
    const long long nq = (long long)B * d->A * L->T;
    auto gw = [&](a0_learner::DWs& w, float* act3, float* h, float* q) { w.act3 = act3; w.h = h ? h : L->alloc<float>((long long)B * 512); w.raw = L->alloc<float>((long long)B * L->Npad); w.q = q ? q : L->alloc<float>(nq); };
    gw(L->go, L->act3_o, L->h, L->q_o);
    gw(L->gt, L->act3_t, nullptr, L->q_t);
    if (d->double_q && d->algo == A0_ALGO_QR) gw(L->gs, L->act3_s, nullptr, nullptr);
    if (d->algo == A0_ALGO_MDQN) gw(L->gm, L->alloc<float>((long long)B * L->feat), nullptr, nullptr);
    L->g_dq = L->alloc<float>(nq, true); L->a_star = L->alloc<int>(B, true);
    L->fwd_scratch = L->alloc<float>(std::max(4LL, std::max((long long)a0_dense_fwd_scratch(B, 512, L->feat), (long long)a0_dense_fwd_scratch(B, L->Npad, 512))));
    if (d->algo == A0_ALGO_QR) { L->y = L->alloc<float>((long long)B * L->T); a0_ws_qr_taus(L); }
}

// one pass's cosine-embedding head workspace over B * n_tau rows (a0_ws_quantile; a0_learner_set_munchausen for the pass it adds)
static void a0_qws_buffers(a0_learner* L, a0_learner::QWs& w, int n_tau, float* act3, bool grads) {
    const int A = L->d.A;
    w.n_tau = n_tau; w.R = (long long)L->d.B * n_tau; w.act3 = act3;
    w.h = L->alloc<float>(w.R * 512); w.raw = L->alloc<float>(w.R * L->Npad); w.q = L->alloc<float>(w.R * A);
    w.cosx = L->alloc<float>(w.R * 64); w.emb = L->alloc<float>(w.R * L->feat); w.x = L->alloc<float>(w.R * L->feat);
    if (grads) { w.dq = L->alloc<float>(w.R * A, true); w.dx = L->alloc<float>(w.R * L->feat); w.demb = L->alloc<float>(w.R * L->feat); }
}

// iqn and fqf (K = N = N' = F, and the fraction net's buffers): the cosine-embedding head's workspaces per pass, the fraction draws, the quantile target
static void a0_ws_quantile(a0_learner* L, const a0_learner_buffers& U) {
    const a0_learner_desc* d = &L->d; const int B = d->B;
    const bool fqf = L->fam == A0_FAM_FQF;
    const int K = fqf ? d->fqf_F : d->iqn_K, N = fqf ? d->fqf_F : d->iqn_N, Nd = fqf ? d->fqf_F : d->iqn_N_dash;
    L->a_star = L->alloc<int>(B, true);
    long long sc = 4;
    auto ws = [&](a0_learner::QWs& w, int n_tau, float* act3, bool grads) {
        a0_qws_buffers(L, w, n_tau, act3, grads);
        for (int r : {B * K, B * Nd, B * N, B * (N - 1)}) {
            if (r > w.R || r < 1) continue;
            const long long a = a0_dense_fwd_scratch(r, L->feat, 64), b2 = a0_dense_fwd_scratch(r, 512, L->feat), c = a0_dense_fwd_scratch(r, L->Npad, 512);
            sc = std::max(sc, std::max(a, std::max(b2, c)));
        }
    };
    ws(L->qo, N, L->act3_o, true);
    ws(L->qt, Nd > K ? Nd : K, L->act3_t, false);
    if (d->double_q) ws(L->qs, K, L->act3_s, false);
    L->t_sel = L->alloc<float>(ceil_to((long long)B * K, 4)); L->t_tgt = L->alloc<float>(ceil_to((long long)B * Nd, 4)); L->t_on = L->alloc<float>(ceil_to((long long)B * N, 4));
    L->y = L->alloc<float>((long long)B * Nd);
    if (fqf) {
        const int F = d->fqf_F;
        auto fw = [&](a0_learner::FWs& w) { w.logits = L->alloc<float>((long long)B * 32, true); w.tau_all = L->alloc<float>((long long)B * (F + 1)); w.tau_hat = L->alloc<float>((long long)B * F); };
        fw(L->fo); fw(L->ft);
        if (d->double_q) fw(L->fs);
        ws(L->qf, F, L->act3_o, false);
        sc = std::max(sc, (long long)a0_dense_fwd_scratch(B, 32, L->feat));
        L->inner_taus = L->alloc<float>((long long)B * F);
        L->rms_sq = U.rms_sq ? U.rms_sq : L->alloc<float>(L->frac.size(), true);
        L->frac_loss = L->alloc<float>(B, true); L->dfrac = L->alloc<float>((long long)B * 32, true); L->clip = L->alloc<float>(4, true);
    }
    L->fwd_scratch = L->alloc<float>(sc);
}

extern "C" int a0_learner_create_on(const a0_learner_desc* d, const a0_learner_buffers* bufs, a0_learner** out) {
    A0_TRY
    A0_CHECK(a0_learner_desc_check(d, bufs, out));
    const a0_learner_buffers none{}, &U = bufs ? *bufs : none;
    std::unique_ptr<a0_learner> L(new a0_learner());
    L->d = *d;
    L->rng.init(d->seed, 0);      // every learner: learner.aug_shift, NoisyNet and the quantile fractions draw from the seed
    a0_net_desc nd{4, 84, 84};
    if (a0_net_create(&nd, &L->net) != A0_OK) return A0_EINVAL;
    a0_learner_layout(L.get());
    if (a0_ws_common(L.get(), U) != A0_OK) return A0_EINVAL;
    switch (L->fam) {
        case A0_FAM_SCALAR: break;      // the common buffers are all it has
        case A0_FAM_DIST: a0_ws_dist(L.get()); break;
        case A0_FAM_LAYERWISE: a0_ws_layerwise(L.get()); break;
        case A0_FAM_IQN: case A0_FAM_FQF: a0_ws_quantile(L.get(), U); break;
    }
    *out = L.release();
    return A0_OK;
    A0_CATCH
}

// DeepQHead.forward (model.py:108-131; the distributional variants 137-177): relu(first_dense(x)), the q / value heads, the dueling combine — DeviceNet.head, dense branch
static int a0_dense_head(a0_learner* L, bool target, a0_learner::DWs& w, void* stream) {
    const int B = L->d.B;
    A0_CHECK(a0_dense_fwd(w.act3, L->feat, L->Wf(target), L->bf(target), w.h, B, 512, L->feat, 1, L->fwd_scratch, stream));
    A0_CHECK(a0_dense_fwd(w.h, 512, L->Wh(target), L->bh(target), w.raw, B, L->Npad, 512, 0, L->fwd_scratch, stream));
    return a0_dueling_fwd(w.raw, L->Npad, w.q, B, L->d.A, L->T, L->d.dueling ? 1 : 0, stream);
}

// IQNHead.forward (model.py:235-251) for `n_tau` fractions per sample: cosine features, the embedding times the state features (in the embedding GEMM's epilogue where the
// shape allows; kept for the backward pass when the pass is differentiated), fc1, the head, the dueling combine — DeviceNet.head of agent0_amd/deepq/engine.py
static int a0_iqn_head(a0_learner* L, bool target, a0_learner::QWs& w, const float* taus, int n_tau, bool grads, void* stream) {
    const int B = L->d.B, A = L->d.A;
    const int R = B * n_tau;
    const float* flat = target ? L->target : L->online;
    // (fc1 and the heads are NoisyLinear layers under NoisyNet — their composed weights; the cosine embedding is a plain Linear: model.py:204-217)
    const float *Wc = flat + L->cos.w(), *bc = flat + L->cos.b(), *Wf = L->Wf(target), *bf = L->bf(target), *Wh = L->Wh(target), *bh = L->bh(target);
    A0_CHECK(a0_cos_features(taus, w.cosx, R, 64, stream));
    if (!grads && a0_dense_fwd_scratch(R, L->feat, 64) == 0) A0_CHECK(a0_dense_fwd_mul(w.cosx, 64, Wc, bc, w.act3, n_tau, w.x, R, L->feat, 64, 1, stream));
    else if (grads && a0_dense_fwd_mul_keep_ok(R, L->feat, 64, 64)) A0_CHECK(a0_dense_fwd_mul_keep(w.cosx, 64, Wc, bc, w.act3, n_tau, w.emb, w.x, R, L->feat, 64, 1, stream));
    else {
        A0_CHECK(a0_dense_fwd(w.cosx, 64, Wc, bc, w.emb, R, L->feat, 64, 1, L->fwd_scratch, stream));
        A0_CHECK(a0_hadamard_fwd(w.emb, w.act3, w.x, B, n_tau, L->feat, stream));
    }
    A0_CHECK(a0_dense_fwd(w.x, L->feat, Wf, bf, w.h, R, 512, L->feat, 1, L->fwd_scratch, stream));
    A0_CHECK(a0_dense_fwd(w.h, 512, Wh, bh, w.raw, R, L->Npad, 512, 0, L->fwd_scratch, stream));
    return a0_dueling_fwd(w.raw, L->Npad, w.q, R, A, 1, L->d.dueling ? 1 : 0, stream);
}

extern "C" int a0_learner_destroy(a0_learner* L) { delete L; return A0_OK; }

extern "C" long long a0_learner_param_floats(const a0_learner* L) { return L ? L->n_pad : 0; }

// Data parallelism through the handle (the reference has no multi-GPU learner: launch.py's actors are its only parallelism): `comm` from
// a0_dp_init makes every a0_learner_update SUM its gradients over the ranks between backward and Adam — the two buckets, the side stream and the order of
// agent0_amd/deepq/dist.py::RcclGradAllReduce, issued eagerly.  comm = 0 switches the exchange off again.  The caller owns the communicator.
extern "C" int a0_learner_set_exchange(a0_learner* L, long long comm) {
    A0_TRY
    if (!L) return a0_fail(A0_EINVAL, "a0_learner_set_exchange: null handle");
    if (comm && !L->dp_side) {
        A0_HIP_THROW(hipStreamCreateWithFlags(&L->dp_side, hipStreamNonBlocking));
        for (hipEvent_t& e : L->dp_ev) A0_HIP_THROW(hipEventCreateWithFlags(&e, hipEventDisableTiming));
    }
    if (comm && L->redo_freq > 0) return a0_fail(A0_EINVAL, "a0_learner_set_exchange: not together with a0_learner_set_redo (the ranks would draw different masks)");
    L->dp_comm = comm;
    L->dp_one_rank = false;
    if (comm) {       // a one-rank group (a rehearsal, or a job of one GPU): nothing to overlap, so both all-reduces go on the update's own stream
        int info[3] = {0, 0, 0};
        if (a0_dp_info(comm, info) == A0_OK) L->dp_one_rank = info[0] == 1;
    }
    return A0_OK;
    A0_CATCH
}

extern "C" int a0_learner_set_grad_clip(a0_learner* L, double max_norm, float* norm_ring_dev, int ring_cap) {
    A0_TRY
    if (!L) return a0_fail(A0_EINVAL, "a0_learner_set_grad_clip: null handle");
    if (!(max_norm > 0.0)) { L->clip_max_norm = 0.f; return A0_OK; }
    if (norm_ring_dev && ring_cap < 1) return a0_fail(A0_EINVAL, "a0_learner_set_grad_clip: a caller's ring needs ring_cap >= 1");
    if (!L->gnorm_partials) L->gnorm_partials = L->alloc<double>(A0_GRAD_NORM_PARTIALS, true);
    if (norm_ring_dev) { L->gnorm_ring = norm_ring_dev; L->gnorm_ring_cap = ring_cap; }
    else { L->gnorm_ring_cap = ring_cap > 0 ? ring_cap : 1024; L->gnorm_ring = L->alloc<float>(L->gnorm_ring_cap, true); }
    L->clip_max_norm = (float)max_norm;
    return A0_OK;
    A0_CATCH
}

extern "C" int a0_learner_set_target_tau(a0_learner* L, double tau) {
    if (!L) return a0_fail(A0_EINVAL, "a0_learner_set_target_tau: null handle");
    if (L->updated) return a0_fail(A0_EINVAL, "a0_learner_set_target_tau: the setting is fixed once the handle has run an update");
    if (!(tau < 1.0) || !((float)tau < 1.f)) return a0_fail(A0_EINVAL, "a0_learner_set_target_tau: tau >= 1 is the hard copy, which learner.target_update_freq alone gives");
    L->target_tau = tau > 0.0 && (float)tau > 0.f ? tau : 0.0;
    return A0_OK;
}

extern "C" int a0_learner_set_weight_decay(a0_learner* L, double lambda, double* partials_dev) {
    A0_TRY
    if (!L) return a0_fail(A0_EINVAL, "a0_learner_set_weight_decay: null handle");
    if (L->updated) return a0_fail(A0_EINVAL, "a0_learner_set_weight_decay: the setting is fixed once the handle has run an update");
    if (lambda != lambda) return a0_fail(A0_EINVAL, "a0_learner_set_weight_decay: lambda is NaN");
    if (!(lambda > 0.0)) { L->decay_c = 0.0; return A0_OK; }
    const double c = L->d.lr * lambda;
    const float c32 = (float)c;
    char msg[256];
    if (!(c32 < 1.f)) {
        snprintf(msg, sizeof msg, "a0_learner_set_weight_decay: lr * lambda = %g * %g = %g must be below 1", L->d.lr, lambda, c);
        return a0_fail(A0_EINVAL, msg);
    }
    if (!(c32 >= 0x1p-24f)) {
        snprintf(msg, sizeof msg, "a0_learner_set_weight_decay: lr * lambda = %g * %g = %g is below 2^-24 = %g and would move no fp32 parameter", L->d.lr, lambda, c, 0x1p-24);
        return a0_fail(A0_EINVAL, msg);
    }
    if (((uintptr_t)partials_dev) & 7) return a0_fail(A0_EINVAL, "a0_learner_set_weight_decay: partials_dev must be 8-byte aligned");
    if (!partials_dev && !L->decay_own) L->decay_own = L->alloc<double>(A0_GRAD_NORM_PARTIALS, true);
    L->decay_partials = partials_dev ? partials_dev : L->decay_own;
    L->decay_c = c;
    return A0_OK;
    A0_CATCH
}

extern "C" int a0_learner_weight_decay_partials(const a0_learner* L, double** partials_dev) {
    if (!L || !partials_dev) return a0_fail(A0_EINVAL, "a0_learner_weight_decay_partials: null argument");
    *partials_dev = L->decay_c > 0.0 ? L->decay_partials : nullptr;
    return A0_OK;
}

// The rule table of a network reset from the handle's block descriptors: NetLayout.reset_segments (agent0_amd/deepq/layout.py), entry for entry.  A fresh weight has
// the constructor's per-element scale (agent0_amd/deepq/model.py): an orthogonal matrix of gain g has element RMS g / sqrt(max(rows, cols)); a NoisyLinear's mu is
// uniform in +-1 / sqrt(in), its sigma 0.4 / sqrt(in) (weights) and 0.4 / sqrt(out) (bias).  Returns the number of entries.
static int a0_learner_reset_table(const a0_learner* L, a0_net_reset_seg* out) {
    int n = 0;
    auto add = [&](long long off, long long cnt, int kind, double scale, int keep) { if (cnt > 0) out[n++] = a0_net_reset_seg{off, cnt, kind, (float)scale, keep}; };
    auto orth = [](double gain, long long rows, long long cols) { return gain / std::sqrt((double)std::max(rows, cols)); };
    const double g_relu = std::sqrt(2.0);
    for (const Blk* b : {&L->conv1, &L->conv2, &L->conv3}) {
        add(b->w(), (long long)b->N * b->K, A0_NET_RESET_NORMAL, orth(g_relu, b->N, b->K), 1);
        add(b->b(), b->N, A0_NET_RESET_CONST, 0.0, 1);
    }
    const long long real = L->Nq + L->V, pad = L->Npad - real;
    if (L->d.noisy) {
        const double bf = 1.0 / std::sqrt((double)L->feat), bh = 1.0 / std::sqrt(512.0);
        add(L->fc1.w(), 512LL * L->feat, A0_NET_RESET_UNIFORM, bf, 0);
        add(L->fc1.b(), 512, A0_NET_RESET_UNIFORM, bf, 0);
        add(L->fc1_sigma.w(), 512LL * L->feat, A0_NET_RESET_CONST, 0.4 * bf, 0);
        add(L->fc1_sigma.b(), 512, A0_NET_RESET_CONST, 0.4 / std::sqrt(512.0), 0);
        add(L->head.w(), real * 512, A0_NET_RESET_UNIFORM, bh, 0);
        add(L->head.w() + real * 512, pad * 512, A0_NET_RESET_CONST, 0.0, 0);
        add(L->head.b(), real, A0_NET_RESET_UNIFORM, bh, 0);
        add(L->head.b() + real, pad, A0_NET_RESET_CONST, 0.0, 0);
        add(L->head_sigma.w(), real * 512, A0_NET_RESET_CONST, 0.4 * bh, 0);
        add(L->head_sigma.w() + real * 512, pad * 512, A0_NET_RESET_CONST, 0.0, 0);
        add(L->head_sigma.b(), L->Nq, A0_NET_RESET_CONST, 0.4 / std::sqrt((double)L->Nq), 0);
        add(L->head_sigma.b() + L->Nq, L->V, A0_NET_RESET_CONST, L->V > 0 ? 0.4 / std::sqrt((double)L->V) : 0.0, 0);
        add(L->head_sigma.b() + real, pad, A0_NET_RESET_CONST, 0.0, 0);
    } else {
        add(L->fc1.w(), 512LL * L->feat, A0_NET_RESET_NORMAL, orth(g_relu, 512, L->feat), 0);
        add(L->fc1.b(), 512, A0_NET_RESET_CONST, 0.0, 0);
        add(L->head.w(), (long long)L->Nq * 512, A0_NET_RESET_NORMAL, orth(0.01, L->Nq, 512), 0);
        add(L->head.w() + (long long)L->Nq * 512, (long long)L->V * 512, A0_NET_RESET_NORMAL, orth(1.0, L->V, 512), 0);
        add(L->head.w() + real * 512, pad * 512, A0_NET_RESET_CONST, 0.0, 0);
        add(L->head.b(), L->Npad, A0_NET_RESET_CONST, 0.0, 0);
    }
    if (L->d.algo == A0_ALGO_IQN || L->d.algo == A0_ALGO_FQF) {
        add(L->cos.w(), (long long)L->feat * 64, A0_NET_RESET_NORMAL, orth(g_relu, L->feat, 64), 0);
        add(L->cos.b(), L->feat, A0_NET_RESET_CONST, 0.0, 0);
    }
    return n;
}

extern "C" int a0_learner_set_net_reset(a0_learner* L, int freq, double shrink, unsigned long long seed) {
    if (!L) return a0_fail(A0_EINVAL, "a0_learner_set_net_reset: null handle");
    if (L->updated) return a0_fail(A0_EINVAL, "a0_learner_set_net_reset: the setting is fixed once the handle has run an update");
    if (freq < 0) return a0_fail(A0_EINVAL, "a0_learner_set_net_reset: freq < 0 (0 is off)");
    if (!(shrink >= 0.0) || !(shrink <= 1.0)) return a0_fail(A0_EINVAL, "a0_learner_set_net_reset: shrink must lie in [0, 1]");
    L->reset_freq = freq; L->reset_shrink = shrink; L->reset_seed = seed & 0xFFFFFFFFull;
    L->n_reset_segs = freq > 0 ? a0_learner_reset_table(L, L->reset_segs) : 0;
    return A0_OK;
}

extern "C" int a0_learner_net_reset_segs(const a0_learner* L, a0_net_reset_seg* out, int cap) {
    if (!L || !out || cap < 0) return a0_fail(A0_EINVAL, "a0_learner_net_reset_segs: null argument");
    a0_net_reset_seg tab[A0_NET_RESET_MAX_SEGS];
    const int n = a0_learner_reset_table(L, tab);
    if (n > cap) return a0_fail(A0_EINVAL, "a0_learner_net_reset_segs: cap is smaller than the table (A0_NET_RESET_MAX_SEGS entries always fit)");
    for (int i = 0; i < n; ++i) out[i] = tab[i];
    return n;
}

extern "C" int a0_learner_set_redo(a0_learner* L, int freq, double tau, int recycle, unsigned long long seed) {
    A0_TRY
    if (!L) return a0_fail(A0_EINVAL, "a0_learner_set_redo: null handle");
    if (L->updated) return a0_fail(A0_EINVAL, "a0_learner_set_redo: the setting is fixed once the handle has run an update");
    if (freq < 0) return a0_fail(A0_EINVAL, "a0_learner_set_redo: freq < 0 (0 is off)");
    if (!(tau >= 0.0) || !(tau < 1.0)) {
        char msg[160];
        snprintf(msg, sizeof msg, "a0_learner_set_redo: tau = %g must be a finite number in [0, 1)", tau);
        return a0_fail(A0_EINVAL, msg);
    }
    if (freq > 0 && recycle && L->d.noisy) return a0_fail(A0_EINVAL, "a0_learner_set_redo: recycle is undefined for NoisyNet's mu / sigma pairs (recycle = 0 measures only)");
    if (freq > 0 && L->dp_comm) return a0_fail(A0_EINVAL, "a0_learner_set_redo: not on a handle with a data-parallel exchange (the ranks would draw different masks)");
    L->redo_freq = freq; L->redo_tau = tau; L->redo_recycle = recycle ? 1 : 0; L->redo_seed = seed & 0xFFFFFFFFull;
    L->n_redo_segs = freq > 0 && recycle ? a0_learner_reset_table(L, L->redo_segs) : 0;
    if (freq > 0 && !L->redo_partials) {
        L->redo_partials = L->alloc<double>((long long)A0_REDO_PARTIALS * A0_REDO_NEURONS);
        L->redo_scores = L->alloc<float>(A0_REDO_NEURONS, true); L->redo_mask = L->alloc<int>(A0_REDO_NEURONS, true); L->redo_counts = L->alloc<int>(8, true);
        const int never = -1;
        A0_HIP_THROW(hipMemcpy(L->redo_counts + 5, &never, sizeof never, hipMemcpyHostToDevice));
    }
    return A0_OK;
    A0_CATCH
}

extern "C" int a0_learner_redo_buffers(const a0_learner* L, float** scores_dev, int** mask_dev, int** counts_dev) {
    if (!L || !scores_dev || !mask_dev || !counts_dev) return a0_fail(A0_EINVAL, "a0_learner_redo_buffers: null argument");
    const bool on = L->redo_freq > 0;
    *scores_dev = on ? L->redo_scores : nullptr; *mask_dev = on ? L->redo_mask : nullptr; *counts_dev = on ? L->redo_counts : nullptr;
    return A0_OK;
}

extern "C" int a0_learner_set_feature_rank(a0_learner* L, int freq, double delta) {
    A0_TRY
    if (!L) return a0_fail(A0_EINVAL, "a0_learner_set_feature_rank: null handle");
    if (L->updated) return a0_fail(A0_EINVAL, "a0_learner_set_feature_rank: the setting is fixed once the handle has run an update");
    if (freq < 0) return a0_fail(A0_EINVAL, "a0_learner_set_feature_rank: freq < 0 (0 is off)");
    if (!(delta > 0.0) || !(delta < 1.0)) {
        char msg[160];
        snprintf(msg, sizeof msg, "a0_learner_set_feature_rank: delta = %g must lie in the open interval (0, 1)", delta);
        return a0_fail(A0_EINVAL, msg);
    }
    L->rank_freq = freq; L->rank_delta = delta;
    if (freq > 0 && !L->rank_gram) {
        L->rank_gram = L->alloc<double>((long long)A0_RANK_GRAM_DOUBLES);
        L->rank_spectrum = L->alloc<double>(A0_RANK_FEATURES, true); L->rank_result = L->alloc<int>(8, true);
        const int never = -1;
        A0_HIP_THROW(hipMemcpy(L->rank_result + 2, &never, sizeof never, hipMemcpyHostToDevice));
    }
    return A0_OK;
    A0_CATCH
}

extern "C" int a0_learner_feature_rank_buffers(const a0_learner* L, double** spectrum_dev, int** result_dev) {
    if (!L || !spectrum_dev || !result_dev) return a0_fail(A0_EINVAL, "a0_learner_feature_rank_buffers: null argument");
    const bool on = L->rank_freq > 0;
    *spectrum_dev = on ? L->rank_spectrum : nullptr; *result_dev = on ? L->rank_result : nullptr;
    return A0_OK;
}

extern "C" int a0_learner_set_aug_shift(a0_learner* L, int pad) {
    A0_TRY
    if (!L) return a0_fail(A0_EINVAL, "a0_learner_set_aug_shift: null handle");
    if (pad == 0) { L->aug_pad = 0; return A0_OK; }
    const long long row = 2LL * L->C * L->H * L->W;
    A0_CHECK(a0_augment_shift_check("a0_learner_set_aug_shift", L->C, L->H, L->W, pad, row));
    if (!L->aug_stage) L->aug_stage = L->alloc<uint8_t>((long long)L->d.B * row);
    L->aug_pad = pad;
    return A0_OK;
    A0_CATCH
}

// learner.iqn.munchausen (DeviceLearner: munchausen_value + the constructor's refusals).  The new pass's rows, B * N', are rows a0_ws_quantile has sized fwd_scratch for (qt has at least as many)
extern "C" int a0_learner_set_munchausen(a0_learner* L, int on, double tau, double alpha, double lo) {
    A0_TRY
    if (!L) return a0_fail(A0_EINVAL, "a0_learner_set_munchausen: null handle");
    if (L->updated) return a0_fail(A0_EINVAL, "a0_learner_set_munchausen: the setting is fixed once the handle has run an update");
    char msg[256];
    const float t32 = (float)tau, a32 = (float)alpha, l32 = (float)lo;
    if (!(tau > 0.0) || !(t32 > 0.f) || !(t32 - t32 == 0.f)) {
        snprintf(msg, sizeof msg, "a0_learner_set_munchausen: learner.mdqn.tau = %g must be a finite number above 0 (as a float too)", tau);
        return a0_fail(A0_EINVAL, msg);
    }
    if (!(alpha >= 0.0) || !(a32 - a32 == 0.f)) {
        snprintf(msg, sizeof msg, "a0_learner_set_munchausen: learner.mdqn.alpha = %g must be a finite number >= 0", alpha);
        return a0_fail(A0_EINVAL, msg);
    }
    if (!(lo <= 0.0) || !(l32 - l32 == 0.f)) {
        snprintf(msg, sizeof msg, "a0_learner_set_munchausen: learner.mdqn.lo = %g must be a finite number <= 0", lo);
        return a0_fail(A0_EINVAL, msg);
    }
    if (!on) { L->miqn = false; return A0_OK; }
    if (L->d.algo != A0_ALGO_IQN) {
        snprintf(msg, sizeof msg, "a0_learner_set_munchausen: learner.iqn.munchausen is for iqn handles only (this handle's algo is %d)", L->d.algo);
        return a0_fail(A0_EINVAL, msg);
    }
    if (L->d.double_q) return a0_fail(A0_EINVAL, "a0_learner_set_munchausen: learner.iqn.munchausen not together with double_q = 1 (the target has no argmax to decouple)");
    if (L->risk_kind != A0_RISK_NEUTRAL) return a0_fail(A0_EINVAL, "a0_learner_set_munchausen: learner.iqn.munchausen not together with learner.iqn.risk (a0_learner_set_risk: the target's policy is the softmax of the risk-neutral mean)");
    if (!L->act3_m) {
        L->act3_m = L->alloc<float>((long long)L->d.B * L->feat);
        a0_qws_buffers(L, L->qm, L->d.iqn_N_dash, L->act3_m, false);
    }
    L->miqn = true; L->miqn_tau = t32; L->miqn_alpha = a32; L->miqn_lo = l32;
    return A0_OK;
    A0_CATCH
}

// learner.iqn.risk (DeviceLearner: risk_value + the constructor's refusals)
extern "C" int a0_learner_set_risk(a0_learner* L, int kind, double eta) {
    A0_TRY
    if (!L) return a0_fail(A0_EINVAL, "a0_learner_set_risk: null handle");
    if (L->updated) return a0_fail(A0_EINVAL, "a0_learner_set_risk: learner.iqn.risk is fixed once the handle has run an update");
    A0_CHECK(a0_risk_check("a0_learner_set_risk", kind, eta));
    if (kind == A0_RISK_NEUTRAL) { L->risk_kind = A0_RISK_NEUTRAL; L->risk_eta = 0.0; return A0_OK; }
    if (L->d.algo != A0_ALGO_IQN) {
        char msg[256];
        snprintf(msg, sizeof msg, "a0_learner_set_risk: learner.iqn.risk = %d is for iqn handles only (this handle's algo is %d; fqf proposes its fractions, it does not draw them)", kind, L->d.algo);
        return a0_fail(A0_EINVAL, msg);
    }
    if (L->miqn) return a0_fail(A0_EINVAL, "a0_learner_set_risk: learner.iqn.risk not together with learner.iqn.munchausen (its target's policy is the softmax of the risk-neutral mean)");
    if (!L->t_risk) L->t_risk = L->alloc<float>(ceil_to((long long)L->d.B * L->d.iqn_K, 4));
    L->risk_kind = kind; L->risk_eta = eta;
    return A0_OK;
    A0_CATCH
}

// learner.c51.hl_gauss (DeviceLearner: hl_gauss_value).  sigma from the fp32 vmin and vmax the loss kernels receive, in double
extern "C" int a0_learner_set_hl_gauss(a0_learner* L, double ratio) {
    A0_TRY
    if (!L) return a0_fail(A0_EINVAL, "a0_learner_set_hl_gauss: null handle");
    char msg[256];
    if (!(ratio - ratio == 0.0)) {
        snprintf(msg, sizeof msg, "a0_learner_set_hl_gauss: learner.c51.hl_gauss = %g must be a finite number (<= 0 is off)", ratio);
        return a0_fail(A0_EINVAL, msg);
    }
    if (!(ratio > 0.0)) { L->hlg_sigma = 0.0; return A0_OK; }
    if (L->d.algo != A0_ALGO_C51) {
        snprintf(msg, sizeof msg, "a0_learner_set_hl_gauss: learner.c51.hl_gauss = %g is for c51 handles only (this handle's algo is %d)", ratio, L->d.algo);
        return a0_fail(A0_EINVAL, msg);
    }
    const double delta = ((double)(float)L->d.vmax - (double)(float)L->d.vmin) / (double)(L->T - 1), sigma = ratio * delta;
    A0_CHECK(a0_hl_gauss_check("a0_learner_set_hl_gauss", sigma, delta, L->T));
    L->hlg_sigma = sigma;
    return A0_OK;
    A0_CATCH
}

extern "C" int a0_learner_set_params(a0_learner* L, const float* online_packed, const float* target_packed, void* stream) {
    A0_TRY
    if (!L || !online_packed) return a0_fail(A0_EINVAL, "a0_learner_set_params: null argument");
    hipStream_t st = (hipStream_t)stream;
    A0_HIP_THROW(hipMemcpyAsync(L->online, online_packed, (size_t)L->n_pad * 4, hipMemcpyDeviceToDevice, st));
    A0_HIP_THROW(hipMemcpyAsync(L->target, target_packed ? target_packed : online_packed, (size_t)L->n_pad * 4, hipMemcpyDeviceToDevice, st));      // target = deepcopy(model), agent.py:100
    a0_encoder_weights wo = L->enc(L->online), wtg = L->enc(L->target);
    A0_CHECK(a0_net_conv_wt_refresh(&wo, L->C, L->wt_on, stream));
    A0_CHECK(a0_net_conv_wt_refresh(&wtg, L->C, L->wt_tg, stream));
    return A0_OK;
    A0_CATCH
}

extern "C" int a0_learner_loss_buffer(const a0_learner* L, float** loss_dev) {
    if (!L || !loss_dev) return a0_fail(A0_EINVAL, "a0_learner_loss_buffer: null argument");
    *loss_dev = L->loss;
    return A0_OK;
}

// Borrowed views of the handle's own HBM for inspection (parity harnesses walking the handle path link by link against the CPU oracle need the gradients and the
// differentiated pass's activations — the ReLU decisions — that a0_learner_get does not copy out).  Valid until the next call on the handle / a0_learner_destroy.
extern "C" int a0_learner_peek(const a0_learner* L, int what, float** dev_ptr, long long* count) {
    if (!L || !dev_ptr || !count) return a0_fail(A0_EINVAL, "a0_learner_peek: null argument");
    const long long B = L->d.B;
    switch (what) {
        case A0_PEEK_GRADS: *dev_ptr = L->grads; *count = L->n_pad; break;
        case A0_PEEK_ACT1: *dev_ptr = L->act1; *count = B * L->H1 * L->W1 * 32; break;
        case A0_PEEK_ACT2: *dev_ptr = L->act2; *count = B * L->H2 * L->W2 * 64; break;
        case A0_PEEK_ACT3: *dev_ptr = L->act3_o; *count = B * L->feat; break;
        case A0_PEEK_FC1: *dev_ptr = (L->d.algo == A0_ALGO_IQN || L->d.algo == A0_ALGO_FQF) ? L->qo.h : L->h; *count = ((L->d.algo == A0_ALGO_IQN || L->d.algo == A0_ALGO_FQF) ? L->qo.R : B) * 512; break;
        case A0_PEEK_LOSS: *dev_ptr = L->loss; *count = B; break;
        case A0_PEEK_GRAD_NORM_RING: *dev_ptr = L->gnorm_ring; *count = L->gnorm_ring_cap; break;
        default: return a0_fail(A0_EINVAL, "a0_learner_peek: unknown buffer");
    }
    if (!*dev_ptr) return a0_fail(A0_ESTATE, "a0_learner_peek: this learner does not keep that buffer");
    return A0_OK;
}

extern "C" int a0_learner_get_frac_loss(const a0_learner* L, float* out_dev, void* stream) {
    A0_TRY
    if (!L || !out_dev || !L->frac_loss) return a0_fail(A0_EINVAL, "a0_learner_get_frac_loss: an fqf handle and an output buffer");
    A0_HIP_THROW(hipMemcpyAsync(out_dev, L->frac_loss, (size_t)L->d.B * 4, hipMemcpyDeviceToDevice, (hipStream_t)stream));
    return A0_OK;
    A0_CATCH
}

extern "C" int a0_learner_set_support(a0_learner* L, const float* atoms_host) {
    A0_TRY
    if (!L || !atoms_host || !L->atoms) return a0_fail(A0_EINVAL, "a0_learner_set_support: a c51 handle and a host array of num_atoms floats");
    A0_HIP_THROW(hipMemcpy(L->atoms, atoms_host, (size_t)L->T * 4, hipMemcpyHostToDevice));
    return A0_OK;
    A0_CATCH
}

extern "C" int a0_learner_get(const a0_learner* L, float* online_out, float* target_out, float* adam_m_out, float* adam_v_out, int* state_out8, void* stream) {
    A0_TRY
    if (!L) return a0_fail(A0_EINVAL, "a0_learner_get: null handle");
    hipStream_t st = (hipStream_t)stream;
    if (online_out) A0_HIP_THROW(hipMemcpyAsync(online_out, L->online, (size_t)L->n_pad * 4, hipMemcpyDeviceToDevice, st));
    if (target_out) A0_HIP_THROW(hipMemcpyAsync(target_out, L->target, (size_t)L->n_pad * 4, hipMemcpyDeviceToDevice, st));
    if (adam_m_out) A0_HIP_THROW(hipMemcpyAsync(adam_m_out, L->m, (size_t)L->n_pad * 4, hipMemcpyDeviceToDevice, st));
    if (adam_v_out) A0_HIP_THROW(hipMemcpyAsync(adam_v_out, L->v, (size_t)L->n_pad * 4, hipMemcpyDeviceToDevice, st));
    if (state_out8) A0_HIP_THROW(hipMemcpyAsync(state_out8, L->state, 8 * sizeof(int), hipMemcpyDeviceToDevice, st));
    return A0_OK;
    A0_CATCH
}

// ---- a0_learner_update: what the stages of one update share.  Filled by a0_learner_update and a0_upd_prepare; the stages below write pend, head_wgrad_done, fuse_tail and tail
struct a0_upd {
    a0_learner* L; void* stream;
    const int* act; const float *rew, *done, *wgt;      // the batch [B], on the device
    a0_encoder_weights w_on, w_tg;
    a0_frames_arg f_obs, f_next;        // s and s' of the batch's rows (of the stage buffer under learner.aug_shift)
    a0_pending_reduce pend;             // dense slab sums that ride in the encoder's reduction launch ...
    a0_pending_reduce* pp;              // ... unless this is null: under data parallelism the dense range is exchanged right after the dense backward (engine.py::_backward_dense)
    bool head_wgrad_done;               // a distributional head's weight gradient rode in its data gradient's launch (a0_dense_dgrad_wgrad, small class)
    bool dp, dp_inline;                 // data parallelism; both all-reduces on the update's own stream
    int hard_freq;                      // the Adam forms' target period: 0 — never a hard copy — under learner.target_tau
    bool fuse_tail; a0_update_tail_plan tail;      // the update's tail as one launch (a0_backward_encoder decides), by this plan
};

// NoisyNet's modules in one launch.  Forward: both networks' effective weights mu + sigma * eps.  sigma_grads: d sigma = d eff * eps of the online network, from the
// reduced gradients in the mu blocks (model.py:78-87 differentiated)
static int a0_noisy(a0_upd& u, bool sigma_grads) {
    a0_learner* L = u.L;
    const float *mu[6], *sg[6], *nin[6], *nw[6], *nb[6];
    float* out[6]; int N[6], K[6], r0[6], r1[6], nm = 0;
    for (int net = 0; net < (sigma_grads ? 1 : 2); ++net) {
        const float* flat = net ? L->target : L->online; float* e = net ? L->eff_tg : L->eff_on;
        const float* nz = L->noise + (net ? L->noise_len : 0);
        for (int k = 0; k < L->n_mods; ++k, ++nm) {
            const a0_noise_mod& m = L->mods[k];
            const Blk &bm = m.block ? L->head : L->fc1, &bs = m.block ? L->head_sigma : L->fc1_sigma, &be = m.block ? L->eff_head : L->eff_fc1;
            mu[nm] = (sigma_grads ? L->grads : flat) + bm.off; sg[nm] = flat + bs.off; out[nm] = sigma_grads ? L->grads + bs.off : e + be.off;
            N[nm] = bm.N; K[nm] = bm.K; r0[nm] = m.r0; r1[nm] = m.r1;
            nin[nm] = nz + m.off_in; nw[nm] = nz + m.off_w; nb[nm] = nz + m.off_b;
        }
    }
    return a0_noisy_multi(sigma_grads ? 1 : 0, nm, mu, sigma_grads ? nullptr : sg, out, N, K, r0, r1, nin, nw, nb, u.stream);
}
static int a0_sigma_grads(a0_upd& u) { return a0_noisy(u, true); }

// DeviceLearner._upd_prepare, in front of every family's forward.  learner.aug_shift: the batch is shifted into the stage buffer first, by the draws of update state[6], and every pass reads
// that dense batch; the ring is only read.  NoisyNet, BaseLearner.train (agent.py:125-127): reset_noise of the online, then of the target network — ONE Philox fill of
// the joint buffer (the same draws as two fills: every vector is padded to the offsets' stride of four) — and both networks' effective weights in one launch
static int a0_upd_prepare(a0_upd& u, const uint8_t* frames, const int* slot, long long row_bytes) {
    a0_learner* L = u.L; const int obs = L->C * L->H * L->W;
    if (L->aug_pad > 0) {
        A0_CHECK(a0_augment_shift(frames, slot, row_bytes, L->C, L->H, L->W, L->aug_pad, L->d.B, L->rng.seed, L->state, 0, L->aug_stage, u.stream));
        frames = L->aug_stage; slot = nullptr; row_bytes = 2LL * obs;
    }
    u.f_next = a0_frames_arg{frames, slot, row_bytes, obs}; u.f_obs = a0_frames_arg{frames, slot, row_bytes, 0};
    if (!L->d.noisy) return A0_OK;
    const long long nn = 2 * L->noise_len;
    A0_CHECK(a0_rng_normal(L->rng.seed, STREAM_NOISE, L->rng.reserve(STREAM_NOISE, nn), 0.1f, L->noise, nn, u.stream));
    return a0_noisy(u, false);
}

// DeviceLearner._upd_encode: the passes' encoders as ONE launch in the order given (a pass without act3 is left out); `keep`: the differentiated pass, whose act1 / act2 the encoder backward reads
struct a0_enc_sel { bool target, next; float* act3; bool keep; };
static int a0_upd_encode(a0_upd& u, const a0_enc_sel (&sel)[3]) {
    a0_learner* L = u.L;
    a0_encoder_pass passes[3]; int np = 0;
    for (const a0_enc_sel& s : sel)
        if (s.act3) passes[np++] = a0_encoder_pass{s.target ? L->wt_tg : L->wt_on, s.target ? &u.w_tg : &u.w_on, s.next ? &u.f_next : &u.f_obs, L->d.B,
                                                   s.keep ? L->act1 : nullptr, s.keep ? L->act2 : nullptr, s.act3};
    return a0_net_encoder_fwd_fused_multi(L->C, L->H, L->W, np, passes, u.stream);
}

// DeviceLearner._fwd_layerwise (qr, mdqn; the Python side also takes the wide dqn head there, which this handle refuses): the passes' encoders in one launch, then per pass fc1, head, dueling combine; the loss leaves dq in g_dq
static int a0_fwd_layerwise(a0_upd& u) {
    a0_learner* L = u.L; void* stream = u.stream; const int B = L->d.B, A = L->d.A, T = L->T, dq = L->d.double_q ? 1 : 0;
    if (L->d.algo == A0_ALGO_MDQN) {       // the third pass is the target network on the CURRENT observation (agent.py:202-204)
        A0_CHECK(a0_upd_encode(u, {{true, true, L->gt.act3, false}, {true, false, L->gm.act3, false}, {false, false, L->go.act3, true}}));
        A0_CHECK(a0_dense_head(L, true, L->gt, stream));
        A0_CHECK(a0_dense_head(L, true, L->gm, stream));
        A0_CHECK(a0_dense_head(L, false, L->go, stream));
        return a0_loss_mdqn(L->go.q, L->gt.q, L->gm.q, A, u.act, u.rew, u.done, u.wgt, L->gamma_n, (float)L->d.mdqn_tau, (float)L->d.mdqn_lo, B, L->loss, L->g_dq, L->state, stream);
    }
    A0_CHECK(a0_upd_encode(u, {{true, true, L->gt.act3, false}, {false, true, dq ? L->gs.act3 : nullptr, false}, {false, false, L->go.act3, true}}));
    A0_CHECK(a0_dense_head(L, true, L->gt, stream));
    if (dq) A0_CHECK(a0_dense_head(L, false, L->gs, stream));
    A0_CHECK(a0_select_action(dq ? L->gs.q : L->gt.q, (long long)A * T, T, 1, B, A, T, 1, nullptr, L->a_star, nullptr, nullptr, stream));
    A0_CHECK(a0_dense_head(L, false, L->go, stream));
    A0_CHECK(a0_quantile_target(L->gt.q, (long long)A * T, 1, T, L->a_star, u.rew, u.done, L->gamma_n, B, T, L->y, stream));
    A0_HIP_THROW(hipMemsetAsync(L->g_dq, 0, (size_t)B * A * T * 4, (hipStream_t)stream));
    return a0_loss_quantile_huber(L->go.q, (long long)A * T, 1, T, L->y, L->qr_taus, 0, u.act, u.wgt, B, T, T, L->loss, L->g_dq, L->state, stream);
}

// FQFLearner.train_step (agent.py:334-388) in the order of DeviceLearner._fwd_fqf (agent0_amd/deepq/engine.py)
static int a0_fwd_fqf(a0_upd& u) {
    a0_learner* L = u.L; void* stream = u.stream; const int B = L->d.B, A = L->d.A, F = L->F, dq = L->d.double_q ? 1 : 0;
    A0_CHECK(a0_upd_encode(u, {{false, false, L->act3_o, true}, {true, true, L->act3_t, false}, {false, true, dq ? L->act3_s : nullptr, false}}));
    // FQFHead.prop_taus (model.py:268-278): the fraction net on the (detached) features -> taus, tau_hats
    auto taus = [&](const float* flat, const float* act3, a0_learner::FWs& w) -> int {
        A0_CHECK(a0_dense_fwd(act3, L->feat, flat + L->frac.w(), flat + L->frac.b(), w.logits, B, 32, L->feat, 0, L->fwd_scratch, stream));
        return a0_fqf_taus(w.logits, 32, w.tau_all, w.tau_hat, B, F, stream);
    };
    A0_CHECK(taus(L->online, L->act3_o, L->fo));
    A0_CHECK(a0_iqn_head(L, false, L->qo, L->fo.tau_hat, F, true, stream));
    // greedy next action at the selecting network's own fractions: the online network on s' under double-Q, else the target
    a0_learner::FWs& fsel = dq ? L->fs : L->ft; a0_learner::QWs& qsel = dq ? L->qs : L->qt;
    A0_CHECK(taus(dq ? L->online : L->target, qsel.act3, fsel));
    A0_CHECK(a0_iqn_head(L, !dq, qsel, fsel.tau_hat, F, false, stream));
    A0_CHECK(a0_select_action(qsel.q, (long long)F * A, 1, A, B, A, F, 3, fsel.tau_all, L->a_star, nullptr, nullptr, stream));
    A0_CHECK(a0_iqn_head(L, true, L->qt, L->fo.tau_hat, F, false, stream));                      // quirk Q16: the target evaluated at the ONLINE tau-hats
    A0_CHECK(a0_quantile_target(L->qt.q, (long long)F * A, A, 1, L->a_star, u.rew, u.done, L->gamma_n, B, F, L->y, stream));
    A0_HIP_THROW(hipMemsetAsync(L->qo.dq, 0, (size_t)L->qo.R * A * 4, (hipStream_t)stream));
    A0_CHECK(a0_loss_quantile_huber(L->qo.q, (long long)F * A, A, 1, L->y, L->fo.tau_hat, F, u.act, u.wgt, B, F, F, L->loss, L->qo.dq, L->state, stream));
    // fraction loss: q at the interior taus (no grad), its gradient w.r.t. the fraction logits; the fraction net's RMSprop step follows the backward pass
    A0_CHECK(a0_fqf_inner_taus(L->fo.tau_all, L->inner_taus, B, F, stream));
    A0_CHECK(a0_iqn_head(L, false, L->qf, L->inner_taus, F - 1, false, stream));
    A0_CHECK(a0_fqf_fraction_loss(L->qf.q, L->qo.q, L->fo.tau_all, u.act, u.wgt, B, F, A, 32, L->frac_loss, L->dfrac, L->fo.logits, stream));
    return a0_dense_wgrad(L->dfrac, L->act3_o, L->feat, L->grads + L->frac.off, B, 32, L->feat, L->slabs, stream);
}

// IQNLearner.train_step (agent.py:296-331) in the order of DeviceLearner._fwd_iqn (agent0_amd/deepq/engine.py).  The update's three tau draws first (BaseLearner.train_batch:
// K, N', N fractions per sample, Philox stream 3)
static int a0_fwd_iqn(a0_upd& u) {
    a0_learner* L = u.L; void* stream = u.stream; const int B = L->d.B, A = L->d.A, dq = L->d.double_q ? 1 : 0, K = L->d.iqn_K, N = L->d.iqn_N, Nd = L->d.iqn_N_dash;
    A0_CHECK(a0_rng_uniform(L->rng.seed, STREAM_TAUS, L->rng.reserve(STREAM_TAUS, (long long)B * K), L->t_sel, (long long)B * K, stream));
    A0_CHECK(a0_rng_uniform(L->rng.seed, STREAM_TAUS, L->rng.reserve(STREAM_TAUS, (long long)B * Nd), L->t_tgt, (long long)B * Nd, stream));
    A0_CHECK(a0_rng_uniform(L->rng.seed, STREAM_TAUS, L->rng.reserve(STREAM_TAUS, (long long)B * N), L->t_on, (long long)B * N, stream));
    if (L->miqn) {      // learner.iqn.munchausen: the target network on s' and on s at the same N' fractions; no greedy next action (the K draw above is made and left unused)
        A0_CHECK(a0_upd_encode(u, {{true, true, L->act3_t, false}, {true, false, L->act3_m, false}, {false, false, L->act3_o, true}}));
        A0_CHECK(a0_iqn_head(L, true, L->qt, L->t_tgt, Nd, false, stream));
        A0_CHECK(a0_iqn_head(L, true, L->qm, L->t_tgt, Nd, false, stream));
        A0_CHECK(a0_miqn_target(L->qt.q, L->qm.q, (long long)Nd * A, A, 1, u.act, u.rew, u.done, L->gamma_n, L->miqn_tau, L->miqn_alpha, L->miqn_lo, B, Nd, A, L->y, stream));
    } else {
        A0_CHECK(a0_upd_encode(u, {{true, true, L->act3_t, false}, {false, true, dq ? L->act3_s : nullptr, false}, {false, false, L->act3_o, true}}));
        // greedy next action from the K-sample mean, of the online network under double-Q (agent.py:303-306)
        a0_learner::QWs& sel = dq ? L->qs : L->qt;
        const float* t_sel = L->t_sel;
        if (L->risk_kind != A0_RISK_NEUTRAL) {      // learner.iqn.risk: the policy's K fractions distorted into the handle's own buffer; the draws stay what they are
            A0_CHECK(a0_risk_distort(L->t_sel, L->t_risk, (long long)B * K, L->risk_kind, L->risk_eta, stream));
            t_sel = L->t_risk;
        }
        A0_CHECK(a0_iqn_head(L, !dq, sel, t_sel, K, false, stream));
        A0_CHECK(a0_select_action(sel.q, (long long)K * A, 1, A, B, A, K, 1, nullptr, L->a_star, nullptr, nullptr, stream));
        A0_CHECK(a0_iqn_head(L, true, L->qt, L->t_tgt, Nd, false, stream));
        A0_CHECK(a0_quantile_target(L->qt.q, (long long)Nd * A, A, 1, L->a_star, u.rew, u.done, L->gamma_n, B, Nd, L->y, stream));
    }
    A0_CHECK(a0_iqn_head(L, false, L->qo, L->t_on, N, true, stream));
    A0_HIP_THROW(hipMemsetAsync(L->qo.dq, 0, (size_t)L->qo.R * A * 4, (hipStream_t)stream));
    return a0_loss_quantile_huber(L->qo.q, (long long)N * A, A, 1, L->y, L->t_on, N, u.act, u.wgt, B, N, Nd, L->loss, L->qo.dq, L->state, stream);
}

// C51Learner.train_step (agent.py:218-268) / QRLearner.train_step (agent.py:272-293), in the order of DeviceLearner._fwd_dist (agent0_amd/deepq/engine.py): the three encoder
// passes in one launch; the online fc1 over [s ; s'] rows as ONE GEMM and the target's, their slabs finished by one reduction launch; the two head GEMMs; and one
// launch for everything behind them (slab sums, dueling, greedy next action, projection, cross entropy, head gradient)
static int a0_fwd_dist(a0_upd& u) {
    a0_learner* L = u.L; void* stream = u.stream; const int B = L->d.B, A = L->d.A, dq = L->d.double_q ? 1 : 0;
    A0_CHECK(a0_upd_encode(u, {{true, true, L->act3_t, false}, {false, true, dq ? L->act3_s : nullptr, false}, {false, false, L->act3_o, true}}));
    // the passes (online on s, online on s' under double-Q, target on s') are GEMMs of one shape each for fc1 and for the head: one grouped launch per layer, the
    // online passes' rows interleaved into the [splits][R_on][N] buffers the reduction and the loss kernel read
    const int npass = dq ? 3 : 2;
    int ns_on = L->ns_on, ns_tg = L->ns_fc1, nh_on = L->nh_on, nh_tg = L->nh_tg;
    const bool grouped = a0_dense_fwd_partial_multi_ok(npass, B, 512, L->feat) && a0_dense_fwd_partial_multi_ok(npass, B, L->Npad, 512);
    if (grouped) {
        const float* Xs[3] = {L->act3_on, dq ? L->act3_s : L->act3_t, L->act3_t};
        const float* Ws[3] = {L->Wf(false), dq ? L->Wf(false) : L->Wf(true), L->Wf(true)};
        float* sl[3] = {L->fc1_on, dq ? L->fc1_on + (long long)B * 512 : L->fc1_tg, L->fc1_tg};
        const long long st[3] = {(long long)L->R_on * 512, dq ? (long long)L->R_on * 512 : (long long)B * 512, (long long)B * 512};
        A0_CHECK(a0_dense_fwd_partial_multi(npass, Xs, L->feat, Ws, B, 512, L->feat, sl, st, stream));
        ns_on = ns_tg = a0_dense_fwd_partial_multi_slabs(npass, B, 512, L->feat);
    } else {
        A0_CHECK(a0_dense_fwd_partial(L->act3_t, L->feat, L->Wf(true), B, 512, L->feat, L->fc1_tg, stream));
        A0_CHECK(a0_dense_fwd_partial(L->act3_on, L->feat, L->Wf(false), L->R_on, 512, L->feat, L->fc1_on, stream));
    }
    const float* rsl[2] = {L->fc1_on, L->fc1_tg};
    const long long rst[2] = {(long long)L->R_on * 512, (long long)B * 512};
    const int ns[2] = {ns_on, ns_tg}, rows[2] = {L->R_on, B};
    const float* bias[2] = {L->bf(false), L->bf(true)};
    float* out[2] = {L->h_on, L->h_tg};
    A0_CHECK(a0_reduce_bias_act_multi(2, rsl, rst, ns, bias, out, rows, 512, 1, stream));
    if (grouped) {
        const float* Xs[3] = {L->h_on, dq ? L->h_on + (long long)B * 512 : L->h_tg, L->h_tg};
        const float* Ws[3] = {L->Wh(false), dq ? L->Wh(false) : L->Wh(true), L->Wh(true)};
        float* sl[3] = {L->hs_on, dq ? L->hs_on + (long long)B * L->Npad : L->hs_tg, L->hs_tg};
        const long long st[3] = {(long long)L->R_on * L->Npad, dq ? (long long)L->R_on * L->Npad : (long long)B * L->Npad, (long long)B * L->Npad};
        A0_CHECK(a0_dense_fwd_partial_multi(npass, Xs, 512, Ws, B, L->Npad, 512, sl, st, stream));
        nh_on = nh_tg = a0_dense_fwd_partial_multi_slabs(npass, B, L->Npad, 512);
    } else {
        A0_CHECK(a0_dense_fwd_partial(L->h_on, 512, L->Wh(false), L->R_on, L->Npad, 512, L->hs_on, stream));
        A0_CHECK(a0_dense_fwd_partial(L->h_tg, 512, L->Wh(true), B, L->Npad, 512, L->hs_tg, stream));
    }
    if (L->d.algo == A0_ALGO_QR)
        return a0_qr_head_loss_slabs(L->hs_on, (long long)L->R_on * L->Npad, nh_on, L->R_on, L->hs_tg, (long long)B * L->Npad, nh_tg, dq ? B : -1, L->bh(false), L->bh(true),
                                     L->Npad, A, L->T, L->d.dueling ? 1 : 0, u.act, u.rew, u.done, u.wgt, L->qr_taus, L->gamma_n, B, L->loss, L->draw, L->q_o, L->q_t, L->a_star,
                                     L->state, stream);
    if (L->hlg_sigma > 0.0)      // learner.c51.hl_gauss: the same launch with the Gaussian histogram of the scalar target in the projection's place
        return a0_c51_hl_gauss_head_loss_slabs(L->hs_on, (long long)L->R_on * L->Npad, nh_on, L->R_on, L->hs_tg, (long long)B * L->Npad, nh_tg, dq ? B : -1, L->bh(false),
                                               L->bh(true), L->Npad, A, L->T, L->d.dueling ? 1 : 0, u.act, u.rew, u.done, u.wgt, L->atoms, L->gamma_n, (float)L->d.vmin,
                                               (float)L->d.vmax, L->hlg_sigma, B, L->loss, L->draw, L->q_o, L->q_t, L->m_proj, L->a_star, L->state, stream);
    return a0_c51_head_loss_slabs(L->hs_on, (long long)L->R_on * L->Npad, nh_on, L->R_on, L->hs_tg, (long long)B * L->Npad, nh_tg, dq ? B : -1, L->bh(false), L->bh(true),
                                  L->Npad, A, L->T, L->d.dueling ? 1 : 0, u.act, u.rew, u.done, u.wgt, L->atoms, L->gamma_n, (float)L->d.vmin, (float)L->d.vmax, B, L->loss, L->draw,
                                  L->q_o, L->q_t, L->m_proj, L->a_star, L->state, stream);
}

// DeviceLearner._fwd_scalar — dqn (agent.py:173-190) and mdqn from the fc1 slabs (193-215): the target pass on s', a third pass (the online network on s' under double-Q; mdqn: the TARGET network
// on the CURRENT observation, agent.py:202-204) and the online pass on s as ONE encoder launch, their fc1 GEMMs (split-K slabs), then the heads of both networks,
// dueling, argmax, Huber loss, head gradient and the head's backward-data pass in one launch
static int a0_fwd_scalar(a0_upd& u) {
    a0_learner* L = u.L; void* stream = u.stream; const int B = L->d.B, A = L->d.A, dq = L->d.double_q ? 1 : 0;
    const bool mdqn = L->d.algo == A0_ALGO_MDQN, third = mdqn || dq;
    A0_CHECK(a0_upd_encode(u, {{true, true, L->act3_t, false}, {mdqn, !mdqn, third ? L->act3_s : nullptr, false}, {false, false, L->act3_o, true}}));
    int ns = L->ns_fc1; const int n_fc1 = third ? 3 : 2;
    const float* W3 = mdqn ? L->Wf(true) : L->Wf(false);
    if (a0_dense_fwd_partial_multi_ok(n_fc1, B, 512, L->feat)) {      // the passes' fc1 GEMMs as one launch (fewer, deeper splits each)
        const float* Xs[3] = {L->act3_o, L->act3_t, L->act3_s};
        const float* Ws[3] = {L->Wf(false), L->Wf(true), W3};
        A0_CHECK(a0_dense_fwd_partial_multi(n_fc1, Xs, L->feat, Ws, B, 512, L->feat, L->fc1_slabs, nullptr, stream));
        ns = a0_dense_fwd_partial_multi_slabs(n_fc1, B, 512, L->feat);
    } else {
        A0_CHECK(a0_dense_fwd_partial(L->act3_t, L->feat, L->Wf(true), B, 512, L->feat, L->fc1_slabs[1], stream));
        if (third) A0_CHECK(a0_dense_fwd_partial(L->act3_s, L->feat, W3, B, 512, L->feat, L->fc1_slabs[2], stream));
        A0_CHECK(a0_dense_fwd_partial(L->act3_o, L->feat, L->Wf(false), B, 512, L->feat, L->fc1_slabs[0], stream));
    }
    if (mdqn)
        return a0_mdqn_head_loss_slabs(L->fc1_slabs[0], L->fc1_slabs[1], L->fc1_slabs[2], (long long)B * 512, ns, L->bf(false), L->bf(true), L->h, L->Wh(false), L->bh(false),
                                       L->Wh(true), L->bh(true), A, L->d.dueling ? 1 : 0, L->Npad, u.act, u.rew, u.done, u.wgt, L->gamma_n, (float)L->d.mdqn_tau, (float)L->d.mdqn_lo, B,
                                       L->loss, L->q_o, L->q_t, L->q_cur, L->draw, L->state, L->dh, stream);
    return a0_dqn_head_loss_slabs(L->fc1_slabs[0], L->fc1_slabs[1], dq ? L->fc1_slabs[2] : nullptr, (long long)B * 512, ns, L->bf(false), L->bf(true), L->h,
                                  L->Wh(false), L->bh(false), L->Wh(true), L->bh(true), A, L->d.dueling ? 1 : 0, L->Npad, u.act, u.rew, u.done, u.wgt, L->gamma_n, B,
                                  L->loss, L->q_o, L->q_t, L->draw, L->state, L->dh, stream);
}

// the head's data gradient where the loss launch does not fold it in (dist, layerwise) — side by side with the head's weight gradient where the shape allows
static int a0_head_dgrad(a0_upd& u) {
    a0_learner* L = u.L; const int B = L->d.B;
    if (!a0_dense_dgrad_wgrad_ok2(B, L->Npad, 512)) return a0_dense_dgrad(L->draw, L->Wh(false), L->h, L->dh, B, L->Npad, 512, u.stream);
    u.head_wgrad_done = true;
    return a0_dense_dgrad_wgrad(L->draw, L->Wh(false), L->h, 512, L->dh, L->grads + L->head.off, B, L->Npad, 512, u.stream);
}

// DeviceLearner._backward_dense (agent.py:153-155): from the loss's gradient down to d3, the gradient of the online features of s, with the dense weight gradients
static int a0_backward_dense(a0_upd& u) {
    a0_learner* L = u.L; void* stream = u.stream; const int B = L->d.B, A = L->d.A;
    if (L->fam == A0_FAM_IQN || L->fam == A0_FAM_FQF) {      // the quantile branch: over the B * n_tau rows of the differentiated pass
        const int N = L->qo.n_tau, R = (int)L->qo.R;
        A0_CHECK(a0_dueling_bwd(L->qo.dq, L->draw, L->Npad, R, A, 1, L->d.dueling ? 1 : 0, stream));
        A0_CHECK(a0_dense_dgrad(L->draw, L->Wh(false), L->qo.h, L->dh, R, L->Npad, 512, stream));
        if (a0_dense_dgrad_hadamard_ok(R, 512, L->feat, N))      // round 6: dx = dh W never reaches HBM (DeviceLearner._backward_dense takes the same branch)
            A0_CHECK(a0_dense_dgrad_hadamard(L->dh, L->Wf(false), L->qo.emb, L->act3_o, L->qo.demb, L->d3, R, 512, L->feat, N, stream));
        else {
            A0_CHECK(a0_dense_dgrad(L->dh, L->Wf(false), nullptr, L->qo.dx, R, 512, L->feat, stream));
            A0_CHECK(a0_hadamard_bwd(L->qo.dx, L->qo.emb, L->act3_o, L->qo.demb, L->d3, B, N, L->feat, stream));
        }
        const float* dY[3] = {L->draw, L->dh, L->qo.demb};
        const float* X[3] = {L->qo.h, L->qo.x, L->qo.cosx};
        const int ldx[3] = {512, L->feat, 64}, Rr[3] = {R, R, R}, Nn[3] = {L->Npad, 512, L->feat}, Kk[3] = {512, L->feat, 64};
        float* G[3] = {L->grads + L->head.off, L->grads + L->fc1.off, L->grads + L->cos.off};
        return a0_dense_wgrad_multi(3, dY, X, ldx, G, Rr, Nn, Kk, L->slabs, L->slab_off3, u.pp, stream);
    }
    // the dueling combine's backward (layerwise; the fused loss launches write draw themselves) and the head's data gradient (the scalar-head launch writes dh as well)
    if (L->fam == A0_FAM_LAYERWISE) A0_CHECK(a0_dueling_bwd(L->g_dq, L->draw, L->Npad, B, A, L->T, L->d.dueling ? 1 : 0, stream));
    if (L->fam != A0_FAM_SCALAR) A0_CHECK(a0_head_dgrad(u));
    // fc1's data gradient and the dense weight gradients with one slab reduction
    const float* dY[2] = {L->draw, L->dh};
    const float* X[2] = {L->h, L->act3_o};
    const int ldx[2] = {512, L->feat}, R[2] = {B, B}, N[2] = {L->Npad, 512}, K[2] = {512, L->feat};
    float* G[2] = {L->grads + L->head.off, L->grads + L->fc1.off};
    if (u.head_wgrad_done) {
        if (a0_dense_dgrad_wgrad_ok(B, 512, L->feat)) return a0_dense_dgrad_wgrad(L->dh, L->Wf(false), L->act3_o, L->feat, L->d3, G[1], B, 512, L->feat, stream);
        A0_CHECK(a0_dense_dgrad(L->dh, L->Wf(false), L->act3_o, L->d3, B, 512, L->feat, stream));
        return a0_dense_wgrad_multi(1, dY + 1, X + 1, ldx + 1, G + 1, R + 1, N + 1, K + 1, L->slabs, L->slab_off + 1, u.pp, stream);
    }
    // fc1's data gradient, fc1's weight gradient and the head's weight gradient — all three wait for the loss kernel only — as ONE launch (DeviceLearner._backward_dense)
    if (a0_dense_dgrad_wgrad2_ok(B, 512, L->feat, L->Npad, 512))
        return a0_dense_dgrad_wgrad2(L->dh, L->Wf(false), L->act3_o, L->feat, L->d3, G[1], B, 512, L->feat, L->draw, L->h, 512, G[0], L->Npad, 512, stream);
    if (a0_dense_dgrad_wgrad_ok(B, 512, L->feat)) {      // fc1's data gradient and weight gradient as one launch; the head's weight gradient alone
        A0_CHECK(a0_dense_dgrad_wgrad(L->dh, L->Wf(false), L->act3_o, L->feat, L->d3, G[1], B, 512, L->feat, stream));
        return a0_dense_wgrad_multi(1, dY, X, ldx, G, R, N, K, L->slabs, L->slab_off, u.pp, stream);
    }
    A0_CHECK(a0_dense_dgrad(L->dh, L->Wf(false), L->act3_o, L->d3, B, 512, L->feat, stream));
    return a0_dense_wgrad_multi(2, dY, X, ldx, G, R, N, K, L->slabs, L->slab_off, u.pp, stream);
}

// one bucket's all-reduce: on the update's own stream, or on the side stream behind what the update has issued so far
static int a0_dp_bucket(a0_upd& u, int ev, float* g, long long n) {
    a0_learner* L = u.L;
    if (u.dp_inline) return a0_dp_allreduce(L->dp_comm, g, n, u.stream);
    A0_HIP_THROW(hipEventRecord(L->dp_ev[ev], (hipStream_t)u.stream));
    A0_HIP_THROW(hipStreamWaitEvent(L->dp_side, L->dp_ev[ev], 0));
    return a0_dp_allreduce(L->dp_comm, g, n, L->dp_side);
}

// DeviceLearner.exchange_begin: every dense gradient (and the NaN flag riding behind them) is final here; their SUM over the ranks runs on the side stream while the encoder backward computes the
// convolution gradients on the update's.  The two buckets of dist.RcclGradAllReduce (layout.py): [0, fc1.off) the convolution blocks, [fc1.off, n_pad] the dense blocks + the NaN flag
static int a0_exchange_begin(a0_upd& u) {
    a0_learner* L = u.L;
    if (!u.dp) return A0_OK;
    if (L->d.noisy) A0_CHECK(a0_sigma_grads(u));
    A0_CHECK(a0_nan_flag_export(L->state, L->grads + L->n_pad, u.stream));
    return a0_dp_bucket(u, 0, L->grads + L->fc1.off, L->n_pad + 1 - L->fc1.off);
}

// DeviceLearner.backward_encoder(fuse_tail).  The update's tail as one launch: the slab sums wait for the Adam launch — not under data parallelism or clipping, which
// need the summed gradient first, nor under weight decay, whose launch reads the NaN flag the one-launch tail's bookkeeping lowers a launch early, nor when NoisyNet's
// sigma gradients wait for deferred dense sums
static int a0_backward_encoder(a0_upd& u) {
    a0_learner* L = u.L; const int B = L->d.B;
    A0_CHECK(a0_net_encoder_dgrad_fused(L->C, L->H, L->W, L->wt_on, L->d3, L->act1, L->act2, B, L->d2, L->d1, u.stream));
    u.fuse_tail = !u.dp && L->clip_max_norm <= 0.f && L->decay_c <= 0.0 && !(L->d.noisy && u.pend.n > 0);
    if (u.fuse_tail)
        return a0_net_encoder_wgrad_tail(L->net, &u.w_on, &u.f_obs, B, L->act1, L->act2, L->d3, L->d2, L->d1, L->grads + L->conv1.off, L->grads + L->conv2.off,
                                         L->grads + L->conv3.off, L->slabs + L->enc_slab_off, &u.pend, &u.tail, L->state, L->scalars, L->d.lr, 0.9, 0.999, u.hard_freq, u.stream);
    return a0_net_encoder_wgrad(L->net, &u.w_on, &u.f_obs, B, L->act1, L->act2, L->d3, L->d2, L->d1, L->grads + L->conv1.off, L->grads + L->conv2.off, L->grads + L->conv3.off,
                                L->slabs + L->enc_slab_off, &u.pend, u.stream);
}

// DeviceLearner.exchange_end: the convolution bucket behind the dense one on the same communicator and stream (one total order on every rank), then the join.
// Without data parallelism: NoisyNet's sigma gradients, now that the dense sums are reduced
static int a0_exchange_end(a0_upd& u) {
    a0_learner* L = u.L;
    if (!u.dp) return L->d.noisy ? a0_sigma_grads(u) : A0_OK;
    A0_CHECK(a0_dp_bucket(u, 1, L->grads, L->fc1.off));
    if (u.dp_inline) return A0_OK;
    A0_HIP_THROW(hipEventRecord(L->dp_ev[2], L->dp_side));
    A0_HIP_THROW(hipStreamWaitEvent((hipStream_t)u.stream, L->dp_ev[2], 0));
    return A0_OK;
}

// DeviceLearner.apply: Adam (eps = 1e-2 / B unless given), NaN guard, update counter, target copy every target_update_freq updates, weight-copy refresh
// (agent.py:102-106,152-161) in one of three forms, behind learner.weight_decay's launch; then learner.target_tau's blend, which follows whichever form the update took, and learner.net_reset_freq's
// reset, the update's last launch, which returns at once unless this update's count names a reset
static int a0_apply(a0_upd& u, float* loss_out) {
    a0_learner* L = u.L; void* stream = u.stream; const int B = L->d.B; float *on = L->online, *tg = L->target;
    if (loss_out) A0_HIP_THROW(hipMemcpyAsync(loss_out, L->loss, (size_t)B * 4, hipMemcpyDeviceToDevice, (hipStream_t)stream));
    if (L->fam == A0_FAM_FQF)      // unconditional, like the reference's fqf_optimizer.step() in front of the NaN guard (agent.py:139-148); lr / 2e4, alpha 0.95, eps 1e-5
        A0_CHECK(a0_rmsprop_step(on + L->frac.off, L->grads + L->frac.off, L->rms_sq, L->frac.size(), L->d.lr / 2e4, 0.95, 1e-5, L->d.max_grad_norm > 0.0 ? L->d.max_grad_norm : -1.0, L->clip, stream));
    const double eps = L->d.adam_eps > 0.0 ? L->d.adam_eps : 1e-2 / (double)B; const float* dp_flag = u.dp ? L->grads + L->n_pad : nullptr;
    // learner.weight_decay: everything Adam owns shrinks first, unless this update is NaN-skipped; the Adam form behind files the shrunk values' successors
    if (L->decay_c > 0.0) A0_CHECK(a0_weight_decay(on, L->n_adam, L->decay_c, L->state, dp_flag, L->decay_partials, stream));
    if (u.fuse_tail) {
        A0_CHECK(a0_update_tail(on, L->grads, L->m, L->v, L->n_adam, L->state, L->scalars, 0.9, 0.999, eps, tg, L->n_pad, &u.tail, &u.w_on, L->C, L->wt_on, L->wt_tg, L->loss, B,
                                L->loss_ring, L->loss_ring_cap, stream));
    } else if (L->clip_max_norm > 0.f) {
        // learner.clip_grad_norm: every gradient Adam owns is final here — summed over the ranks behind the join — so one launch takes its sum of squares and the Adam
        // launch turns it into the norm, the coefficient and the ring entry
        A0_CHECK(a0_grad_norm_partials(L->grads, L->n_adam, L->gnorm_partials, stream));
        A0_CHECK(a0_adam_step_sync_wt_clip(on, L->grads, L->m, L->v, L->n_adam, L->state, L->scalars, L->d.lr, 0.9, 0.999, eps, u.hard_freq, tg, L->n_pad, dp_flag, &u.w_on, L->C,
                                           L->wt_on, L->wt_tg, L->loss, B, L->loss_ring, L->loss_ring_cap, L->gnorm_partials, L->clip_max_norm, L->gnorm_ring, L->gnorm_ring_cap, stream));
    } else {
        A0_CHECK(a0_adam_step_sync_wt(on, L->grads, L->m, L->v, L->n_adam, L->state, L->scalars, L->d.lr, 0.9, 0.999, eps, u.hard_freq, tg, L->n_pad, dp_flag, &u.w_on, L->C,
                                      L->wt_on, L->wt_tg, L->loss, B, L->loss_ring, L->loss_ring_cap, stream));
    }
    if (L->target_tau > 0.0) A0_CHECK(a0_target_blend(tg, on, L->n_pad, L->target_tau, L->state, L->d.target_update_freq, 0, &u.w_tg, L->C, L->wt_tg, stream));
    // learner.rank_freq: the feature rank of the differentiated pass's fc1 activations (the rows a0_redo_score gets); both launches return at once on other updates
    if (L->rank_freq > 0) {
        const bool quantile = L->fam == A0_FAM_IQN || L->fam == A0_FAM_FQF;
        A0_CHECK(a0_feature_rank(quantile ? L->qo.h : L->h, quantile ? L->qo.R : (long long)B, L->rank_delta, L->state, L->rank_freq, 0, L->rank_gram, L->rank_spectrum, L->rank_result,
                                 stream));
    }
    // learner.redo_freq: scores, mask and counts from the differentiated pass's activations, then the recycle launch; all three return at once on other updates
    if (L->redo_freq > 0) {
        const bool quantile = L->fam == A0_FAM_IQN || L->fam == A0_FAM_FQF;
        const int H3 = L->feat / 64;      // H3 * W3
        A0_CHECK(a0_redo_score(L->act1, (long long)B * L->H1 * L->W1, L->act2, (long long)B * L->H2 * L->W2, L->act3_o, (long long)B * H3, quantile ? L->qo.h : L->h, quantile ? L->qo.R : (long long)B,
                               L->redo_tau, L->state, L->redo_freq, 0, L->redo_partials, L->redo_scores, L->redo_mask, L->redo_counts, stream));
        if (L->redo_recycle) {
            const a0_redo_blocks blk{L->conv1.off, L->conv2.off, L->conv3.off, L->fc1.off, L->head.off, L->conv1.K, L->feat, L->Npad};
            A0_CHECK(a0_redo_recycle(on, L->m, L->v, L->n_adam, L->n_pad, L->redo_segs, L->n_redo_segs, &blk, L->redo_mask, L->redo_seed, L->state, L->redo_freq, 0, 0, &u.w_on, L->C,
                                     L->wt_on, stream));
        }
    }
    return L->reset_freq > 0 ? a0_net_reset(on, tg, L->m, L->v, L->n_adam, L->n_pad, L->reset_segs, L->n_reset_segs, L->reset_shrink, L->reset_seed, L->state, L->reset_freq, 0, 0,
                                            &u.w_on, L->C, L->wt_on, L->wt_tg, stream) : A0_OK;
}

// BaseLearner.train (agent.py:124-169): frames = u8 replay rows st || st_next of `row_bytes` bytes each, addressed through `slot` (ring slots of the sampled
// batch; NULL = dense batch), act / rew / done / wgt [B] on the device.  loss_out (optional) receives the per-sample losses [B] (what the caller feeds to
// update_priority, trainer.py:103-104).  NaN skip, step counter and target sync are decided on the device (state words as in a0_adam_step_sync_wt).
extern "C" int a0_learner_update(a0_learner* L, const uint8_t* frames, const int* slot, long long row_bytes, const int* act, const float* rew, const float* done,
                                 const float* wgt, float* loss_out, void* stream) {
    A0_TRY
    a0_trace_scope range("update");
    if (!L || !frames || !act || !rew || !done || !wgt) return a0_fail(A0_EINVAL, "a0_learner_update: null argument");
    if (row_bytes < 2LL * L->C * L->H * L->W) return a0_fail(A0_EINVAL, "a0_learner_update: a replay row holds st || st_next (2 x C x H x W bytes)");
    L->updated = true;
    // A0_DP_ONE_STREAM=1 (the same on every rank; a tuning aid): both all-reduces on the caller's stream — no overlap with the encoder backward, but none of the three
    // cross-stream hand-offs either, which cost an eager host ~10 us each (profiles/r04_experiments.md)
    // Default (round 6): the side stream when the group has more than one rank (the dense bucket, 95 % of the bytes, travels beside the encoder backward — what the
    // captured form does), the caller's stream in a one-rank group (+0.1 ms per iteration instead of +0.65, profiles/r04_native_dp_one_rank_ab.txt); A0_DP_ONE_STREAM=0 / 1 forces either.
    static const int dp_force = getenv("A0_DP_ONE_STREAM") != nullptr ? (atoi(getenv("A0_DP_ONE_STREAM")) != 0 ? 1 : 0) : -1;
    a0_upd u;
    u.L = L; u.stream = stream; u.act = act; u.rew = rew; u.done = done; u.wgt = wgt;
    u.w_on = L->enc(L->online); u.w_tg = L->enc(L->target);
    u.dp = L->dp_comm != 0; u.dp_inline = dp_force >= 0 ? dp_force == 1 : L->dp_one_rank;
    u.pend.n = 0; u.pp = u.dp ? nullptr : &u.pend; u.head_wgrad_done = u.fuse_tail = false;
    u.hard_freq = L->target_tau > 0.0 ? 0 : L->d.target_update_freq;
    A0_CHECK(a0_upd_prepare(u, frames, slot, row_bytes));
    switch (L->fam) {
        case A0_FAM_SCALAR: A0_CHECK(a0_fwd_scalar(u)); break;
        case A0_FAM_DIST: A0_CHECK(a0_fwd_dist(u)); break;
        case A0_FAM_LAYERWISE: A0_CHECK(a0_fwd_layerwise(u)); break;
        case A0_FAM_IQN: A0_CHECK(a0_fwd_iqn(u)); break;
        case A0_FAM_FQF: A0_CHECK(a0_fwd_fqf(u)); break;
    }
    A0_CHECK(a0_backward_dense(u));
    A0_CHECK(a0_exchange_begin(u));
    A0_CHECK(a0_backward_encoder(u));
    A0_CHECK(a0_exchange_end(u));
    return a0_apply(u, loss_out);
    A0_CATCH
}
