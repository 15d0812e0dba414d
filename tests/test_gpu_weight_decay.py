"""GPU (MI355X): ``learner.weight_decay`` — decoupled (AdamW) weight decay, a0_weight_decay in front of the update's Adam form.

1. the kernel against numpy float32 (tests/weight_decay_ref.py), byte for byte, at the work-split edges, aligned and offset by four bytes; the partial sums against
   float64 within chunk * 2^-53; guard bands around the range.
2. a skipped update (the NaN flag, the data-parallel flag): no parameter byte moves, the partials are written, the status words stay.
3. decay + each non-tail Adam form == the form on host-decayed parameters, on every buffer (tests/test_gpu_update_tail.py's _World).
4. DeviceLearner and the a0_learner handle for every learner of tests/test_gpu_grad_clip.py, plain and clipped.
5. dqn against the oracle's learner whose Adam step is preceded by the decay, free-running, inside tests/test_gpu_trace.py's FREE_BOUNDS.
6. the Trainer: handles == Python classes on main, launch and one-rank data parallelism; ``param_norm``; snapshots; the setting off.
7. bad arguments.
"""
import csv
import math

import numpy as np
import pytest
import torch

import recipe
import weight_decay_ref as R

pytestmark = pytest.mark.gpu

P = R.P


@pytest.fixture(scope="module")
def hip():
    from agent0_amd.ops import HipOps
    ops = HipOps()
    assert "gfx950" in ops.device_info()[2] and hasattr(ops, "weight_decay")
    return ops


def _gc():
    import test_gpu_grad_clip as GC
    return GC


def _bits(t):
    return t.view(torch.int32) if t.dtype == torch.float32 else t


# ------------------------------------------------------------------------------------------------ 1. the kernel
GUARD = 64
SPECIAL = np.array([0.0, -0.0, 1e-45, -1e-45, 1e-39, -3e-42, 1.1754944e-38, 3e38, -3e38, 1.7e38, 1.0, -1.0], np.float32)
_INPUT = {}


def _input(n):
    """n floats: normals of mixed scale with zeros of both signs, denormals and large values spread over the range (the first element and the last among them)."""
    if n not in _INPUT:
        g = recipe.gen(900 + n)
        x = (g.standard_normal(n) * np.exp(g.uniform(-20.0, 20.0, n))).astype(np.float32)
        at = np.unique(np.concatenate([[0, n - 1], g.integers(0, n, 4 * len(SPECIAL))]))
        x[at] = SPECIAL[np.arange(at.size) % len(SPECIAL)]
        x.setflags(write=False)
        _INPUT[n] = x
    return _INPUT[n]


def _banded(hip, x, off):
    """x on the device at a 16-byte boundary plus ``off`` floats, with GUARD floats of a known pattern on both sides -> (whole buffer, view of x)."""
    whole = hip.empty(GUARD + 4 + x.size + GUARD)
    assert whole.data_ptr() % 16 == 0
    whole.fill_(-7.25)
    lo = GUARD + off
    whole[lo:lo + x.size].copy_(torch.from_numpy(np.array(x)))
    view = whole[lo:lo + x.size]
    assert view.data_ptr() % 16 == 4 * off
    return whole, view


def _guards_intact(whole, off, n):
    lo = GUARD + off
    return bool((whole[:lo] == -7.25).all()) and bool((whole[lo + n:] == -7.25).all())


@pytest.mark.parametrize("off", [0, 1], ids=["aligned", "offset-4-bytes"])
@pytest.mark.parametrize("n", [5, 1025, 77824 + 37])
def test_kernel_against_numpy(hip, n, off):
    x = _input(n)
    ch = R.chunk_of(n)
    want_parts = R.partials_f64(x)
    state = torch.zeros(8, dtype=torch.int32, device=hip.device)
    for c in (2.0 ** -24, 5e-5, 0.5):
        whole, view = _banded(hip, x, off)
        parts = torch.full((P + 8,), -3.0, dtype=torch.float64, device=hip.device)
        hip.weight_decay(view, n, c, state, None, parts[:P])
        torch.cuda.synchronize()
        got = view.cpu().numpy()
        want = R.decay(x, c)
        bad = np.nonzero(got.view(np.uint32) != want.view(np.uint32))[0]
        assert bad.size == 0, f"n {n} off {off} c {c}: {bad.size} elements differ, first {bad[:8].tolist()}: in {x[bad[:4]].tolist()} got {got[bad[:4]].tolist()} want {want[bad[:4]].tolist()}"
        assert _guards_intact(whole, off, n), "a float outside [0, n) was written"
        gp = parts.cpu().numpy()
        assert bool((gp[P:] == -3.0).all()), "a partial past the last workgroup's"
        rel = np.abs(gp[:P] - want_parts) / np.where(want_parts > 0, want_parts, 1.0)
        print(f"n {n} off {off} c {c}: chunk {ch}, worst partial rel {rel.max():.3e} (bound {ch * 2.0 ** -53:.3e})")
        assert bool((rel <= ch * 2.0 ** -53).all()) and bool((gp[:P][want_parts == 0.0] == 0.0).all())
        assert state.tolist() == [0] * 8
    # 2^-24 is not a no-op
    assert not np.array_equal(R.decay(x, 2.0 ** -24).view(np.uint32), x.view(np.uint32))


# ------------------------------------------------------------------------------------------------ 2. a skipped update
@pytest.mark.parametrize("off", [0, 1], ids=["aligned", "offset-4-bytes"])
@pytest.mark.parametrize("how", ["nan-flag", "extra-flag"])
def test_a_skipped_update_stores_no_parameter(hip, how, off):
    n = 1025
    x = _input(n)
    whole, view = _banded(hip, x, off)
    before = whole.clone()
    state = torch.tensor([1 if how == "nan-flag" else 0, 5, 2, 0, 1, 0, 9, 3], dtype=torch.int32, device=hip.device)
    st0 = state.clone()
    flag = torch.tensor([2.0 if how == "extra-flag" else 0.0], device=hip.device)
    parts = torch.full((P,), -3.0, dtype=torch.float64, device=hip.device)
    hip.weight_decay(view, n, 0.5, state, flag, parts)
    torch.cuda.synchronize()
    assert torch.equal(_bits(whole), _bits(before)), "a skipped update moved a parameter"
    assert torch.equal(state, st0) and flag.item() == (2.0 if how == "extra-flag" else 0.0)
    want = R.partials_f64(x)
    gp = parts.cpu().numpy()
    assert bool((np.abs(gp - want) <= R.chunk_of(n) * 2.0 ** -53 * want).all()), "the partials are written on a skipped update too"
    # ... and with both flags down the same call decays
    state[0] = 0
    flag.zero_()
    hip.weight_decay(view, n, 0.5, state, flag, parts)
    torch.cuda.synchronize()
    assert np.array_equal(view.cpu().numpy().view(np.uint32), R.decay(x, 0.5).view(np.uint32))


# ------------------------------------------------------------------------------------------------ 3. in front of each non-tail Adam form
FORMS3 = ["adam_step_sync", "adam_step_sync_clip", "adam_step_sync_wt", "adam_step_sync_wt_clip"]


@pytest.mark.parametrize("aligned", [True, False], ids=["n%4==0,n_total>n", "n%4!=0"])
@pytest.mark.parametrize("form", FORMS3)
def test_decay_then_the_form_equals_the_form_on_decayed_parameters(hip, form, aligned):
    """Four updates at target_update_freq = 2 — first, sync, NaN-skipped (+ sync), ordinary.  World A: a0_weight_decay, then the form.  World B: the host replaces
    params[:n] by the numpy reference's (nothing on the skipped update), then the same form."""
    import test_gpu_update_tail as UT
    HP = UT.HP
    C_, c = 4, 5e-5
    conv_end = 32 * 64 * C_ + 32 + 64 * 512 + 64 + 64 * 576 + 64
    n_dense, extra = (1700, 260) if aligned else (1701, 3)
    n, n_total = conv_end + n_dense, conv_end + n_dense + extra
    A, Bw = UT._World(hip, C_, n, n_total, 31), UT._World(hip, C_, n, n_total, 31)
    gen = recipe.gen(32)
    fold, clip = "_wt" in form, form.endswith("_clip")
    extra_bufs = {}
    for w in (A, Bw):
        extra_bufs[id(w)] = dict(partials=hip.zeros(P, dtype=torch.float64), gring=hip.zeros(7), wd=hip.zeros(P, dtype=torch.float64))
    for u, kind in enumerate(["first", "sync", "nan+sync", "ordinary"]):
        g = torch.from_numpy((gen.standard_normal(n_total + 4) * 0.1).astype(np.float32)).to(hip.device)
        loss = torch.from_numpy(gen.standard_normal(8).astype(np.float32)).to(hip.device)
        for w in (A, Bw):
            E = extra_bufs[id(w)]
            w.g.copy_(g)
            w.loss.copy_(loss)
            if kind.startswith("nan"):
                w.state[0] = 1
            if w is A:
                hip.weight_decay(w.p, n, c, w.state, None, E["wd"])
            elif not kind.startswith("nan"):
                host = w.p.cpu().numpy()
                host[:n] = R.decay(host[:n], c)
                w.p.copy_(torch.from_numpy(host))
            adam = (w.p, w.g, w.m, w.v, n, w.state, w.scal, HP["lr"], HP["b1"], HP["b2"], HP["eps"], HP["tf"], w.t, n_total, None)
            wt = (w.weights(w.p), C_, w.wt, w.wt_t, w.loss, 8, w.ring) if fold else ()
            if clip:
                hip.grad_norm_partials(w.g, n, E["partials"])
                getattr(hip, form)(*adam, *wt, E["partials"], 0.5, E["gring"])
            else:
                getattr(hip, form)(*adam, *wt)
        torch.cuda.synchronize()
        a, b = A.everything(), Bw.everything()
        a["norm_ring"], b["norm_ring"] = extra_bufs[id(A)]["gring"], extra_bufs[id(Bw)]["gring"]
        for k in a:
            assert torch.equal(_bits(a[k]), _bits(b[k])), f"{form}, update {u} ({kind}): {k}"
        st = A.state.tolist()
        want = {"first": (1, 0, 0), "sync": (2, 0, 1), "nan+sync": (2, 1, 1), "ordinary": (3, 0, 0)}[kind]
        assert (st[1], st[3], st[4]) == want and st[0] == 0, f"{form}, update {u} ({kind}): status words {st}"
        if kind.endswith("sync"):
            assert torch.equal(_bits(A.t), _bits(A.p))
    if fold:      # the copies are what a refresh from the final weights gives
        fresh = hip.empty(hip.conv_wt_floats(C_))
        hip.conv_wt_refresh(A.weights(A.p), C_, fresh)
        torch.cuda.synchronize()
        assert torch.equal(_bits(fresh), _bits(A.wt))


# ------------------------------------------------------------------------------------------------ 4. learners
LAMBDA4 = 20.0          # lr 5e-4: c = fl32(0.01)


def _engine4(cs, clip=-1.0, **kw):
    """tests/test_gpu_grad_clip.py's _Case.engine with further constructor arguments."""
    from agent0_amd.common.utils import DeviceRng
    from agent0_amd.deepq.engine import DeviceLearner
    GC = _gc()
    c = cs.c
    dev = DeviceLearner(cs.hip, cs.L, GC.B, double_q=c.get("double_q", False), target_update_freq=3, K=cs.K, N=cs.N, N_dash=cs.Nd,
                        max_grad_norm=c.get("max_grad_norm", -1.0), clip_grad_norm=clip, **kw)
    dev.online.load_state_dict(recipe.make_state_dict(cs.spec, 11))
    dev.target.load_state_dict(recipe.make_state_dict(cs.spec, 12))
    rng = DeviceRng(cs.hip, GC.SEED)
    if cs.L.noisy:
        rng.reserve(rng.STREAM_NOISE, dev.online.noise_len); rng.reserve(rng.STREAM_NOISE, dev.target.noise_len)
    dev._test_rng = rng
    dev._test_taus = [cs.hip.empty(GC.B * k) for k in (cs.K, cs.Nd, cs.N)] if cs.L.algo == "iqn" else None
    return dev


def _fresh_copies_equal(hip, dev, what):
    for net, name in ((dev.online, "online"), (dev.target, "target")):
        if not net.fused:
            continue
        fresh = hip.empty(net.wt.numel())
        hip.conv_wt_refresh(net.encoder_weights(), dev.L.C, fresh)
        torch.cuda.synchronize()
        assert torch.equal(_bits(fresh), _bits(net.wt)), f"{what}: the {name} network's weight copies"


@pytest.mark.parametrize("clipped", [False, True], ids=["plain", "clipped"])
@pytest.mark.parametrize("name", ["dqn", "rainbow-lite", "iqn", "fqf-fraction-clip"])
def test_learner_with_decay_equals_the_learner_decayed_by_hand(hip, name, clipped):
    GC = _gc()
    cs = GC._Case(hip, name)
    L = cs.L
    clip = -1.0
    if clipped:      # half the first update's norm: the first update clips
        probe = _engine4(cs)
        probe.forward_backward(*cs.batch(0), rand=cs.draws(probe))
        torch.cuda.synchronize()
        clip = float(np.float32(0.5 * float(probe.grads[:L.n_adam].double().square().sum().sqrt())))
    wd, hand, plain = _engine4(cs, clip, weight_decay=LAMBDA4), _engine4(cs, clip), _engine4(cs, clip)
    assert wd.wd_coef == float(np.float32(0.01)) and wd.wd_partials is not None and hand.wd_partials is None and hand.wd_coef == 0.0
    nat = cs.handle(wd, clip)
    nat.set_weight_decay(LAMBDA4)
    frac = L.blocks.get("frac")
    pad = ~cs.real_mask()
    for s in range(4):
        before = wd.online.flat[:L.n_adam].cpu().numpy()
        wd.update(*cs.batch(s), rand=cs.draws(wd))
        # the same update with the decay applied by hand between the backward pass and apply()
        hand.forward_backward(*cs.batch(s), rand=cs.draws(hand))
        host = hand.online.flat.cpu().numpy()
        host[:L.n_adam] = R.decay(host[:L.n_adam], wd.wd_coef)
        hand.online.flat.copy_(torch.from_numpy(host))
        hand.apply()
        nat.update(*cs.batch(s))
        if s == 0:
            plain.update(*cs.batch(s), rand=cs.draws(plain))
        torch.cuda.synchronize()
        GC._same(GC._everything(wd), GC._everything(hand), f"{name}, update {s}: weight_decay vs decayed by hand")
        o, t, m, v, st = nat.get()
        GC._same(dict(online=o, target=t, moment1=m, moment2=v, state=st), GC._everything(wd), f"{name}, update {s}: the handle")
        _fresh_copies_equal(hip, wd, f"{name}, update {s}")
        assert wd.state[1].item() == s + 1 and wd.state[0].item() == 0
        if frac is not None:
            assert torch.equal(wd.online.flat[frac.all], hand.online.flat[frac.all]) and torch.equal(wd.rms_sq, hand.rms_sq), "the fraction net is left alone"
            if s == 0:
                assert torch.equal(wd.online.flat[frac.all], plain.online.flat[frac.all]), "the fraction net equals the undecayed run's"
        if s == 0:
            assert not torch.equal(wd.online.flat[:L.n_adam], plain.online.flat[:L.n_adam]), "the setting changes the parameters"
        assert float(wd.online.flat[:L.n_adam].cpu()[pad].abs().max()) == 0.0, "padded head rows stay zero"
        # the statistic: the norm in front of this update's decay, in both buffers
        want = math.sqrt(math.fsum((before.astype(np.float64) ** 2).tolist()))
        got = R.norm_of(wd.wd_partials.cpu().numpy())
        assert abs(got - want) <= (L.n_adam * 2.0 ** -53 + 2.0 ** -53) * want and torch.equal(nat.weight_decay_partials(), wd.wd_partials)
    nat.close()


@pytest.mark.parametrize("value", [0.0, -1.0])
def test_the_off_values_change_nothing_and_keep_the_one_launch_tail(hip, value):
    GC = _gc()
    cs = GC._Case(hip, "dqn")
    off, none = _engine4(cs, weight_decay=value), _engine4(cs)
    assert off.wd_partials is None and off.wd_coef == 0.0 and off.weight_decay == 0.0
    nat = cs.handle(off, -1.0)
    nat.set_weight_decay(value)
    assert nat.weight_decay_partials() is None
    planned = []
    for s in range(3):
        for dev in (off, none):
            dev.forward_dense(*cs.batch(s))
            dev.exchange_begin()
            dev.backward_encoder(fuse_tail=True)
            planned.append(dev._tail_plan is not None)
            dev.exchange_end()
            dev.apply()
        nat.update(*cs.batch(s))
    torch.cuda.synchronize()
    assert all(planned), "the one-launch tail stays selected"
    for k, x in dict(GC._everything(off), grads=off.grads, wt=off.online.wt, wt_target=off.target.wt, scalars=off.scalars, ring=off.loss_ring).items():
        y = dict(GC._everything(none), grads=none.grads, wt=none.online.wt, wt_target=none.target.wt, scalars=none.scalars, ring=none.loss_ring)[k]
        assert torch.equal(_bits(x), _bits(y)), k
    o, t, m, v, st = nat.get()
    GC._same(dict(online=o, target=t, moment1=m, moment2=v, state=st), GC._everything(none), "the handle with the setting off")
    nat.close()
    # ... and on, the three-launch tail
    on = _engine4(cs, weight_decay=LAMBDA4)
    on.forward_dense(*cs.batch(0))
    on.backward_encoder(fuse_tail=True)
    assert on._tail_plan is None
    on.apply()
    torch.cuda.synchronize()


def test_a_nan_skipped_update_decays_nothing_in_the_learner(hip):
    """The loss kernel raises the flag itself (a NaN reward); engine and handle leave every parameter where it was and count the skip."""
    GC = _gc()
    cs = GC._Case(hip, "dqn")
    wd = _engine4(cs, weight_decay=LAMBDA4)
    nat = cs.handle(wd, -1.0)
    nat.set_weight_decay(LAMBDA4)
    batch = list(cs.batch(0))
    batch[4] = batch[4].clone()
    batch[4][0] = float("nan")
    before = wd.online.flat.clone()
    wd.update(*batch)
    nat.update(*batch)
    torch.cuda.synchronize()
    assert torch.equal(_bits(wd.online.flat), _bits(before)) and wd.state.tolist()[:4] == [0, 0, 1, 1]
    o, t, m, v, st = nat.get()
    assert torch.equal(_bits(o), _bits(before)) and torch.equal(st, wd.state)
    want = math.sqrt(math.fsum((before[:cs.L.n_adam].cpu().numpy().astype(np.float64) ** 2).tolist()))
    assert abs(R.norm_of(wd.wd_partials.cpu().numpy()) - want) <= (cs.L.n_adam * 2.0 ** -53 + 2.0 ** -53) * want
    nat.close()


# ------------------------------------------------------------------------------------------------ 5. the reference walk
def test_dqn_walks_with_the_oracle_that_decays_in_front_of_adam(hip):
    """dqn at tests/test_gpu_trace.py's smallest batch (32), four free-running updates, lambda = 20 at lr 5e-4 (c = 0.01), against oracle.learner.OracleLearner with
    p <- p * (1 - c) in front of its Adam step (tests/weight_decay_ref.py).  Bounds: that file's FREE_BOUNDS (18 free-running updates) — loss_rel and param_abs."""
    from agent0_amd.deepq.engine import DeviceLearner
    from agent0_amd.deepq.layout import NetLayout
    from oracle import learner as olearner
    from oracle.losses import Hyper
    import test_gpu_trace as TR
    Bw, lam = TR.SMALL.B, 20.0
    spec = recipe.NetSpec("dqn", 4)
    L = NetLayout.from_spec(spec)
    dev = DeviceLearner(hip, L, Bw, target_update_freq=2, weight_decay=lam)
    c = dev.wd_coef
    assert c == float(np.float32(0.01)) and dev.lr == 5e-4      # the oracle's default learning rate
    sd_o, sd_t = recipe.make_state_dict(spec, 11), recipe.make_state_dict(spec, 12)
    dev.online.load_state_dict(sd_o)
    dev.target.load_state_dict(sd_t)
    ora = R.decayed_oracle(olearner.OracleLearner)(spec, sd_o, sd_t, Hyper(), batch_size=Bw, target_update_freq=2, c=c)
    plain = olearner.OracleLearner(spec, sd_o, sd_t, Hyper(), batch_size=Bw, target_update_freq=2)
    D = lambda x: torch.from_numpy(x).to(hip.device)
    for s in range(4):
        frames = recipe.make_frames(Bw, 61 + s, spec.obs_shape)
        a, r, d, w = recipe.make_transitions(Bw, spec.action_dim, 62 + s)
        loss = dev.update(D(frames.reshape(-1)), None, 2 * 4 * 84 * 84, D(a.astype(np.int32)), D(r), D(d.astype(np.float32)), D(w))
        torch.cuda.synchronize()
        res = ora.train(frames.reshape(Bw, -1), a, r, d.astype(np.float32), w, np.arange(Bw))
        plain.train(frames.reshape(Bw, -1), a, r, d.astype(np.float32), w, np.arange(Bw))
        loss_rel = float(((loss[:Bw].cpu() - res["q_loss"]).abs() / (res["q_loss"].abs() + 1e-3)).max())
        got, got_t = dev.online.state_dict(), dev.target.state_dict()
        param_abs = max(float((got[k].cpu() - ora.po[k].detach()).abs().max()) for k in ora.q_keys)
        target_abs = max(float((got_t[k].cpu() - ora.pt[k].detach()).abs().max()) for k in ora.q_keys)
        print(f"update {s + 1}: loss_rel {loss_rel:.3e} param_abs {param_abs:.3e} target_abs {target_abs:.3e}")
        assert loss_rel <= TR.FREE_BOUNDS["loss_rel"] and param_abs <= TR.FREE_BOUNDS["param_abs"] and target_abs <= TR.FREE_BOUNDS["param_abs"]
    assert ora.update_steps == 4 == dev.state[1].item()
    # the walk has teeth: the undecayed oracle ends far (in units of the bound) from the decayed one
    far = max(float((ora.po[k].detach() - plain.po[k].detach()).abs().max()) for k in ora.q_keys)
    print(f"decayed vs undecayed oracle: {far:.3e}")
    assert far > 1e3 * TR.FREE_BOUNDS["param_abs"]


# ------------------------------------------------------------------------------------------------ 6. the Trainer
LAMBDA6 = 20.0


def _el():
    import test_gpu_eps_ladder as EL
    return EL


def _trainer(tmp_path, monkeypatch, native, algo, extra, use_lp, tag, lam=LAMBDA6, seed=42):
    from agent0_amd.deepq.config import parse_overrides
    from agent0_amd.deepq.trainer import Trainer
    monkeypatch.setenv("A0_NATIVE_LOOP", "1" if native else "0")
    cfg = parse_overrides([f"learner.algo={algo}", f"seed={seed}", f"logdir={tmp_path / tag}"] + ([f"learner.weight_decay={lam}"] if lam is not None else []) + _el().BASE5 + list(extra))
    return Trainer(cfg, use_lp=use_lp)


def _state(tr):
    eng = tr.learner.engine
    return _el()._state(tr) + [eng.online.wt.clone(), eng.target.wt.clone()] + ([eng.wd_partials.clone()] if eng.wd_partials is not None else [])


def _run(tmp_path, monkeypatch, native, algo, extra, use_lp, tag, lam=LAMBDA6, iters=6, dp=False):
    from agent0_amd.deepq.native_loop import NativeLoop
    EL = _el()
    tr = _trainer(tmp_path, monkeypatch, native, algo, extra, use_lp, tag, lam)
    hook = EL._install_exchange(tr) if dp else None
    res = [{k: v for k, v in tr.run_iteration().items() if k != "fps"} for _ in range(iters)]
    assert isinstance(tr._nl, NativeLoop) if native else tr._nl is False, getattr(tr, "native_loop_reason", None)
    out = _state(tr), res, list(tr.Qs), list(tr.Rs), tr.frame_count
    assert res[-1]["loss"] is not None, "updates ran"
    EL._close_exchange(tr, hook) if dp else EL._close(tr)
    return out


@pytest.mark.parametrize("mode,algo,extra", [("main", "dqn", []), ("launch", "dqn", []), ("dp", "dqn", []),
                                             ("main", "c51", ["learner.noisy_net=true", "learner.dueling_head=true", "learner.n_step_q=3"])],
                         ids=["main-dqn", "launch-dqn", "dp-dqn", "main-c51-noisy-duel-n3"])
def test_handles_and_python_classes_end_on_the_same_state(mode, algo, extra, tmp_path, monkeypatch):
    """Six iterations, three updates each once training has started.  ``dp``: a one-rank RCCL group (A0_DP_FORCE=1).  The result dictionaries are compared too, so
    ``param_norm`` is the same number under both host loops."""
    import torch.distributed as dist
    EL = _el()
    dp = mode == "dp"
    if dp:
        EL._one_rank_group(monkeypatch)
    try:
        a = _run(tmp_path, monkeypatch, False, algo, extra, mode == "launch", "py", dp=dp)
        b = _run(tmp_path, monkeypatch, True, algo, extra, mode == "launch", "nat", dp=dp)
    finally:
        if dp:
            dist.destroy_process_group()
    EL._assert_same_run(a, b)
    state, res = a[0][4], a[1]
    assert state[1].item() >= 8
    norms = [r.get("param_norm") for r in res]
    print("param_norm per iteration:", norms)
    assert all("param_norm" in r for r in res) and norms[-1] is not None and math.isfinite(norms[-1]) and norms[-1] > 0.0
    assert norms[-1] == R.norm_of(a[0][-1].cpu().numpy()), "the statistic is the partials' sum in index order, square-rooted in double"
    if mode == "main" and algo == "dqn":
        off = _run(tmp_path, monkeypatch, True, algo, extra, False, "off", lam=None)
        assert off[0][4][1].item() == state[1].item() and not torch.equal(off[0][0], a[0][0]), "the setting changes the parameters"
        assert all("param_norm" not in r for r in off[1])


def test_param_norm_is_the_norm_in_front_of_the_last_update(tmp_path, monkeypatch):
    """The Python classes with ``train_batch`` wrapped on the instance: the parameters in front of every update are captured on the device; the reported number is
    their float64 norm within n_adam * 2^-53 (non-negative terms, exact in double) plus one rounding of the square root."""
    EL = _el()
    tr = _trainer(tmp_path, monkeypatch, False, "dqn", [], False, "cap")
    eng = tr.learner.engine
    n_adam = eng.L.n_adam
    seen = []
    inner = tr.learner.train_batch

    def capture(*a, **kw):
        seen.append(eng.online.flat[:n_adam].clone())
        return inner(*a, **kw)
    tr.learner.train_batch = capture
    res = None
    for _ in range(5):
        res = tr.run_iteration()
        tr.logging(res)
    torch.cuda.synchronize()
    assert len(seen) >= 3 and res["loss"] is not None
    want = math.sqrt(math.fsum((seen[-1].cpu().numpy().astype(np.float64) ** 2).tolist()))
    got = res["param_norm"]
    print(f"param_norm {got!r} float64 {want!r} rel {abs(got - want) / want:.3e}")
    assert math.isfinite(got) and abs(got - want) <= (n_adam * 2.0 ** -53 + 2.0 ** -53) * want
    later = math.sqrt(math.fsum((eng.online.flat[:n_adam].cpu().numpy().astype(np.float64) ** 2).tolist()))
    assert abs(got - later) > (n_adam * 2.0 ** -53 + 2.0 ** -53) * want, "in front of the last update, not behind it"
    EL._close(tr)
    GC = _gc()
    with open(tmp_path / "cap" / "progress.csv") as f:
        rows = list(csv.DictReader(f))
    assert list(rows[0].keys()) == GC.TODAYS_HEADER + ["param_norm"] and float(rows[-1]["param_norm"]) == got
    assert "param_norm" in open(tmp_path / "cap" / "msg.log").read()


@pytest.mark.parametrize("native", [True, False], ids=["handles", "python-classes"])
def test_a_snapshot_taken_mid_run_resumes_bit_for_bit(native, tmp_path, monkeypatch):
    EL = _el()
    want = _run(tmp_path, monkeypatch, native, "dqn", [], False, "a")
    tr = _trainer(tmp_path, monkeypatch, native, "dqn", [], False, "b")
    for _ in range(3):
        tr.run_iteration()
    assert tr.learner.engine.state[1].item() > 0, "updates ran in front of the snapshot"
    snap_dir = tr.save_snapshot(str(tmp_path / "snap"))
    EL._close(tr)
    tr = _trainer(tmp_path, monkeypatch, native, "dqn", [], False, "c", seed=7)
    tr.load_snapshot(snap_dir)
    res = [{k: v for k, v in tr.run_iteration().items() if k != "fps"} for _ in range(3)]
    got = _state(tr)
    EL._close(tr)
    for i, (x, y) in enumerate(zip(got, want[0])):
        assert torch.equal(_bits(x), _bits(y)), f"state item {i}"
    assert res == want[1][3:]


def test_setting_off_changes_no_key_no_header_and_no_log_line(tmp_path, monkeypatch):
    GC = _gc()
    tr = GC._trainer(tmp_path, monkeypatch, True, "off")
    eng = tr.learner.engine
    assert eng.weight_decay == 0.0 and eng.wd_coef == 0.0 and eng.wd_partials is None
    for i in range(2):
        res = tr.run_iteration()
        tr.logging(res)
    assert list(res.keys()) == GC.TODAYS_HEADER[:-1] + ["fps"] and res["loss"] is not None
    GC._close(tr)
    with open(tmp_path / "off" / "progress.csv") as f:
        rows = list(csv.reader(f))
    assert rows[0] == GC.TODAYS_HEADER and len(rows) == 3
    log = open(tmp_path / "off" / "msg.log").read()
    assert "param_norm" not in log and "weight_decay" not in log


def test_the_learner_refuses_bad_settings(hip):
    cs = _gc()._Case(hip, "dqn")
    for lam in (float("nan"), 2000.0, 1e-4):
        with pytest.raises(ValueError, match=r"learner\.weight_decay"):
            _engine4(cs, weight_decay=lam)


# ------------------------------------------------------------------------------------------------ 7. bad arguments
def test_bad_arguments_are_refused(hip):
    from agent0_amd import _abi
    from agent0_amd._abi import A0Error
    lib, EINVAL = hip.lib, -1
    p = hip.zeros(1024)
    state = torch.zeros(8, dtype=torch.int32, device=hip.device)
    parts = hip.zeros(P + 2, dtype=torch.float64)
    pp, sp, dp = p.data_ptr(), state.data_ptr(), parts.data_ptr()
    for args in ((None, 64, 0.5, sp, None, dp), (pp, 64, 0.5, None, None, dp), (pp, 64, 0.5, sp, None, None), (pp, 0, 0.5, sp, None, dp), (pp, -1, 0.5, sp, None, dp),
                 (pp, 64, 0.5, sp, None, dp + 4), (pp + 2, 64, 0.5, sp, None, dp)):
        assert lib.a0_weight_decay(*args, None) == EINVAL and "a0_weight_decay" in _abi.last_error(), args
    for c in (1.0, 1.5, 0.0, -0.5, float("nan"), float("inf"), 2.0 ** -25, 1.0 - 2.0 ** -30):
        assert lib.a0_weight_decay(pp, 64, c, sp, None, dp, None) == EINVAL and "a0_weight_decay" in _abi.last_error() and "2^-24" in _abi.last_error(), c
        with pytest.raises(A0Error, match="a0_weight_decay"):
            hip.weight_decay(p, 64, c, state, None, parts[:P])
    with pytest.raises(A0Error):
        hip.weight_decay(p, 64, 0.5, state, None, parts[:P - 1])
    torch.cuda.synchronize()
    assert float(p.abs().max()) == 0.0 and float(parts.abs().max()) == 0.0, "a refused call launches nothing"
    # the handle's setter: the numbers are named, a misaligned buffer is refused, and the setting is fixed once an update has run
    GC = _gc()
    cs = GC._Case(hip, "dqn")
    dev = cs.engine()
    nat = cs.handle(dev, -1.0)
    h = nat.h
    assert lib.a0_learner_set_weight_decay(None, 0.1, None) == EINVAL and "a0_learner_set_weight_decay" in _abi.last_error()
    assert lib.a0_learner_set_weight_decay(h, float("nan"), None) == EINVAL and "a0_learner_set_weight_decay" in _abi.last_error() and "NaN" in _abi.last_error()
    assert lib.a0_learner_set_weight_decay(h, 2000.0, None) == EINVAL and "2000" in _abi.last_error() and "0.0005" in _abi.last_error() and "below 1" in _abi.last_error()
    assert lib.a0_learner_set_weight_decay(h, 1e-4, None) == EINVAL and "0.0001" in _abi.last_error() and "0.0005" in _abi.last_error() and "2^-24" in _abi.last_error()
    assert lib.a0_learner_set_weight_decay(h, 0.1, dp + 4) == EINVAL and "8-byte aligned" in _abi.last_error()
    assert nat.weight_decay_partials() is None
    nat.set_weight_decay(0.1)
    own = nat.weight_decay_partials()
    assert own is not None and float(own.abs().max()) == 0.0, "NULL: the handle allocates"
    nat.set_weight_decay(0.0)
    assert nat.weight_decay_partials() is None
    nat.set_weight_decay(0.1, parts[:P])
    nat.update(*cs.batch(0))
    torch.cuda.synchronize()
    assert float(parts[:P].sum()) > 0.0 and float(parts[P:].abs().max()) == 0.0 and torch.equal(nat.weight_decay_partials(), parts[:P]), "the caller's buffer receives the sums"
    for lam in (0.1, 0.0, 0.2):
        assert lib.a0_learner_set_weight_decay(h, lam, None) == EINVAL and "a0_learner_set_weight_decay" in _abi.last_error() and "fixed once" in _abi.last_error()
    nat.close()
