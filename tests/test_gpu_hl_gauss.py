"""GPU (MI355X): the HL-Gauss classification target for C51 (``learner.c51.hl_gauss``): a0_loss_c51_hl_gauss against float64, the fused
a0_c51_hl_gauss_head_loss_slabs against it, and the update that issues the fused kernel.

1. The stand-alone kernel against tests/hl_gauss_ref.py (whose bound tests/test_hl_gauss_reference_helpers.py fixes before any device run): T = 2, 51, 64 bins,
   A = 1, 4, 18 actions, B = 1 and 5 samples, rho = 0.05 (a near one-hot histogram), 0.75 (the paper's) and T (the setting's limit), with samples whose target lies
   on vmin, on vmax, beyond either before the clamp, on a bin edge, on a centre, terminals, and logits spread over +-30.  m is judged per element against e_m, loss
   and dlogits against the bound carried through the cross entropy; the largest share of each bound is printed and recorded.  Two runs give equal bytes; guard words
   around the outputs stay.  A NaN reward: that sample's loss is NaN and the flag is raised, every other sample's bytes are those of a run without it.
   Work split (csrc/loss_c51.hip): one wave per sample, lane t owns bin t and evaluates its own two edges and the two outer ones in double.
2. The fused kernel: on slabs built as tests/test_gpu_value_loss_reference.py builds them for a0_c51_head_loss_slabs — dueling on and off, double-Q on and off,
   B = 5 and 6 (the tail workgroup of the four-samples-per-workgroup split holds one sample, then two) — loss, m_out and a_star equal the stand-alone kernel on
   the fused kernel's own q_on_out / q_tg_out bit for bit and draw equals a0_dueling_bwd of its dlogits.  Under double-Q a* is the online network's choice and
   the expectation the target's.
3. The update, on a c51 learner of 6 actions and 32 samples: the handle (a0_learner_set_hl_gauss), DeviceLearner.update and C51Learner with its hipGraph agree bit
   for bit after each of five updates — also with a separately staged target pass (tstage), which the setting allows; the Trainer under the handles and under the
   Python classes ends on the same parameters, moments, target, loss ring and priorities with NoisyNet + dueling + double-Q + 3-step + sum-tree, and with
   learner.aug_shift, where a snapshot taken mid-run resumes to the uninterrupted run's bytes.  Off (0.0) is the run that never mentions the setting, byte for
   byte; on differs from plain c51 after one update.  The refusals that need a device."""
import numpy as np
import pytest
import torch

import hl_gauss_ref as H
import recipe
from util import record_stats

pytestmark = pytest.mark.gpu

GUARD = 12345.0
RHO = 0.75


@pytest.fixture(scope="module")
def hip():
    from agent0_amd.ops import HipOps
    ops = HipOps()
    assert "gfx950" in ops.device_info()[2]
    assert hasattr(ops, "loss_c51_hl_gauss") and hasattr(ops, "c51_hl_gauss_head_loss_slabs")
    return ops


def _bits(t):
    return t.view(torch.int32) if t.dtype == torch.float32 else t


def _dev(hip, x):
    return torch.from_numpy(np.ascontiguousarray(x)).to(hip.device)


def _guarded(hip, n):
    buf = torch.full((16 + n + 16,), GUARD, device=hip.device)
    return buf, buf[16:16 + n]


def _untouched(buf, n):
    return bool((buf[:16] == GUARD).all()) and bool((buf[16 + n:] == GUARD).all())


def _sigma(rho, T, vmin=H.VMIN, vmax=H.VMAX):
    from agent0_amd.deepq.engine import hl_gauss_value
    return hl_gauss_value(rho, vmin, vmax, T)[1]


# ------------------------------------------------------------------------------------------------ 1. the stand-alone kernel against float64
def _launch(hip, c, T, A, B, rho, rew=None):
    lb, loss = _guarded(hip, B)
    db, dl = _guarded(hip, B * A * T)
    mb, m = _guarded(hip, B * T)
    st = hip.zeros(8, dtype=torch.int32)
    hip.loss_c51_hl_gauss(_dev(hip, c["logits"].reshape(-1)), _dev(hip, c["tgt_logits"].reshape(-1)), A, T, _dev(hip, c["act"]), _dev(hip, c["a_star"]),
                          _dev(hip, c["rew"] if rew is None else rew), _dev(hip, c["done"]), _dev(hip, c["wgt"]), _dev(hip, c["atoms"]), H.GAMMA, c["vmin"], c["vmax"],
                          _sigma(rho, T, c["vmin"], c["vmax"]), B, loss, dl, m, st)
    torch.cuda.synchronize()
    assert _untouched(lb, B) and _untouched(db, B * A * T) and _untouched(mb, B * T), "nothing outside the outputs is written"
    return loss.clone(), dl.clone(), m.clone(), st.cpu().numpy()


def _ref(c, T, A, B, rho, rew=None):
    return H.hl_gauss_loss64(c["logits"], c["tgt_logits"], A, T, c["act"], c["a_star"], c["rew"] if rew is None else rew, c["done"], c["wgt"], c["atoms"], H.GAMMA,
                             c["vmin"], c["vmax"], rho, B)


def _shares(got, ref, act, T, A, B, rows=None):
    """Largest |kernel - reference| / bound of m, the loss and dlogits over ``rows``; outside the taken action dlogits is exactly 0."""
    loss, dl, m = (x.cpu().numpy().astype(np.float64) for x in got[:3])
    rows = np.arange(B) if rows is None else np.asarray(rows, np.int64)
    m, dl = m.reshape(B, T), dl.reshape(B, A, T)
    assert np.isfinite(m[rows]).all() and np.isfinite(loss[rows]).all() and np.isfinite(dl[rows]).all()
    act = np.asarray(act, np.int64)
    g = dl[np.arange(B), act]
    rest = dl.copy()
    rest[np.arange(B), act] = 0.0
    assert not rest[rows].any(), "dlogits is zero outside the taken action"
    return (float((np.abs(m - ref["m"]) / ref["e_m"])[rows].max()), float((np.abs(loss - ref["loss"]) / ref["tol_loss"])[rows].max()),
            float((np.abs(g - ref["g"]) / ref["tol_g"])[rows].max()))


@pytest.mark.parametrize("A", H.AS)
@pytest.mark.parametrize("T", H.TS)
def test_kernel_against_float64(hip, T, A):
    worst = {}
    kinds = set()
    for rho in H.rhos(T):
        w = np.zeros(3)
        for B, shift in H.launches(T, A):
            c = H.case(T, A, B, shift)
            kinds |= set(c["kinds"])
            got = _launch(hip, c, T, A, B, rho)
            ref = _ref(c, T, A, B, rho)
            assert not got[3].any(), f"status words {got[3]}"
            w = np.maximum(w, _shares(got, ref, c["act"], T, A, B))
            again = _launch(hip, c, T, A, B, rho)
            assert all(torch.equal(_bits(x), _bits(y)) for x, y in zip(got[:3], again[:3])), "two runs give equal bytes"
            msum = got[2].cpu().numpy().astype(np.float64).reshape(B, T).sum(-1)
            assert np.abs(msum - 1.0).max() <= 64 * 2.0 ** -24, "the histogram is normalised"
        worst[f"rho{rho:g}"] = dict(m=float(w[0]), loss=float(w[1]), dlogits=float(w[2]))
    assert kinds == set(H.KINDS)
    print(f"T={T} A={A}: largest share of the bound " + ", ".join(f"{k}: m {v['m']:.3f} loss {v['loss']:.3f} dlogits {v['dlogits']:.3f}" for k, v in worst.items()))
    record_stats(f"hl_gauss_t{T}_a{A}", {"largest_error_over_bound": worst})
    assert max(max(v.values()) for v in worst.values()) <= 1.0, worst


@pytest.mark.parametrize("T,A", [(51, 4), (2, 1), (64, 18)])
def test_a_nan_reward_sets_the_flag_and_stays_in_its_sample(hip, T, A):
    B = 5
    c = H.case(T, A, B, 5)
    clean = _launch(hip, c, T, A, B, RHO)
    assert not clean[3].any()
    for b in (0, 2, B - 1):
        rew = c["rew"].copy()
        rew[b] = np.nan
        loss, dl, m, st = _launch(hip, c, T, A, B, RHO, rew=rew)
        assert int(st[0]) == 1 and not st[1:].any(), f"status words {st}"
        l = loss.cpu().numpy()
        assert np.isnan(l[b]) and int(np.isnan(l).sum()) == 1, "the NaN stays in its sample's loss"
        assert bool(torch.isnan(m.reshape(B, T)[b]).all()) and bool(torch.isnan(dl.reshape(B, A, T)[b, int(c["act"][b])]).all())
        keep = [i for i in range(B) if i != b]
        for got, want, n in ((loss, clean[0], 1), (dl, clean[1], A * T), (m, clean[2], T)):
            assert torch.equal(_bits(got.reshape(B, n)[keep]), _bits(want.reshape(B, n)[keep])), "every other sample's bytes are those of a run without the NaN"


# ------------------------------------------------------------------------------------------------ 2. the fused kernel against the stand-alone one
@pytest.mark.parametrize("double_q", [False, True], ids=["targetQ", "doubleQ"])
@pytest.mark.parametrize("dueling", [False, True], ids=["plain", "dueling"])
@pytest.mark.parametrize("B", [5, 6])
def test_fused_kernel_equals_the_stand_alone_kernel_on_its_own_logits(hip, B, dueling, double_q):
    for T, A, rho in ((51, 4, RHO), (64, 18, 0.05), (2, 1, 2.0)):
        NQ = A + (1 if dueling else 0)
        ld = (NQ * T + 31) // 32 * 32
        atoms = torch.linspace(H.VMIN, H.VMAX, T).to(hip.device)
        sigma = _sigma(rho, T)
        for ns_on, ns_tg in ((1, 4), (5, 1)):
            g = recipe.gen(3500 + 1000 * A + 10 * T + B + ns_on)
            R_on = 2 * B if double_q else B
            s_on = _dev(hip, g.standard_normal((ns_on, R_on, ld)).astype(np.float32))
            s_tg = _dev(hip, g.standard_normal((ns_tg, B, ld)).astype(np.float32))
            b_on, b_tg = _dev(hip, g.standard_normal(ld).astype(np.float32)), _dev(hip, g.standard_normal(ld).astype(np.float32))
            a, r, d, w = recipe.make_transitions(B, A, 5 + B)
            r = (r * np.float32(4.0)).astype(np.float32)                 # some targets beyond the support
            act, rew, done, wgt = _dev(hip, a.astype(np.int32)), _dev(hip, r), _dev(hip, d.astype(np.float32)), _dev(hip, w)
            st = hip.zeros(8, dtype=torch.int32)
            (lb, loss), (db, draw), (qb, q_on), (tb, q_tg), (mb, m_out) = (_guarded(hip, n) for n in (B, B * ld, B * A * T, B * A * T, B * T))
            a_star = torch.full((B,), -1, dtype=torch.int32, device=hip.device)
            hip.c51_hl_gauss_head_loss_slabs(s_on.reshape(-1), ns_on, R_on, s_tg.reshape(-1), ns_tg, B if double_q else -1, b_on, b_tg, ld, A, T, dueling, act, rew, done, wgt,
                                             atoms, 0.97, H.VMIN, H.VMAX, sigma, B, loss, draw, st, q_on=q_on, q_tg=q_tg, m_out=m_out, a_star=a_star)
            torch.cuda.synchronize()
            assert all(_untouched(buf, n) for buf, n in ((lb, B), (db, B * ld), (qb, B * A * T), (tb, B * A * T), (mb, B * T))), "nothing outside the outputs is written"
            # the greedy next action: a0_select_action on the selecting network's combined logits
            a2 = hip.zeros(B, dtype=torch.int32)
            if double_q:
                acc = torch.zeros_like(s_on[0])
                for z in range(ns_on):
                    acc = acc + s_on[z]
                q3 = hip.empty(B * A * T)
                hip.dueling_fwd((acc + b_on)[B:].reshape(-1).contiguous(), ld, q3, B, A, T, dueling)
                hip.select_action(q3, A * T, T, 1, B, A, T, 2, atoms, a2, None, None)
            else:
                hip.select_action(q_tg.contiguous(), A * T, T, 1, B, A, T, 2, atoms, a2, None, None)
            loss2, dq2, m2, draw2, st2 = hip.empty(B), hip.zeros(B * A * T), hip.empty(B * T), hip.empty(B * ld), hip.zeros(8, dtype=torch.int32)
            hip.loss_c51_hl_gauss(q_on.contiguous(), q_tg.contiguous(), A, T, act, a2, rew, done, wgt, atoms, 0.97, H.VMIN, H.VMAX, sigma, B, loss2, dq2, m2, st2)
            hip.dueling_bwd(dq2, draw2, ld, B, A, T, dueling)
            torch.cuda.synchronize()
            what = f"T={T} A={A} B={B} slabs={ns_on}/{ns_tg} dueling={dueling} double_q={double_q}"
            assert torch.equal(a_star, a2), f"greedy next action, {what}"
            assert torch.equal(_bits(m_out), _bits(m2)), f"histogram, {what}"
            assert torch.equal(_bits(loss), _bits(loss2)), f"loss, {what}"
            assert torch.equal(_bits(draw), _bits(draw2)), f"draw, {what}"
            assert not st.any() and not st2.any() and bool(torch.isfinite(loss).all())
            assert float((m_out.reshape(B, T).sum(-1) - 1).abs().max()) < 1e-5


# ------------------------------------------------------------------------------------------------ 3. the update
ACTIONS, BATCH, RING, UPDATES = 6, 32, 64, 5
SHAPE = (4, 84, 84)
ROW = 2 * 4 * 84 * 84
SEED = 42 + 15485863            # BaseLearner's Philox seed for cfg.seed = 42
_WORLD = {}


def _world():
    if not _WORLD:
        _WORLD["ring"] = recipe.make_frames(RING, 79, SHAPE).reshape(RING, 2, *SHAPE)
        for s in range(UPDATES):
            a, r, d, w = recipe.make_transitions(BATCH, ACTIONS, 800 + s)
            _WORLD[s] = (recipe.gen(650 + s).integers(0, RING, BATCH).astype(np.int32), a.astype(np.int32), r, d.astype(np.float32), w)
    return _WORLD


def _spec():
    return recipe.NetSpec("c51", ACTIONS, obs_shape=SHAPE)


def _load(dev):
    dev.online.load_state_dict(recipe.make_state_dict(_spec(), 11))
    dev.target.load_state_dict(recipe.make_state_dict(_spec(), 12))


def _engine(hip, hl_gauss=RHO, **kw):
    from agent0_amd.deepq.engine import DeviceLearner
    from agent0_amd.deepq.layout import NetLayout
    dev = DeviceLearner(hip, NetLayout.from_spec(_spec()), BATCH, target_update_freq=2, **({} if hl_gauss is None else dict(hl_gauss=hl_gauss)), **kw)
    _load(dev)
    return dev


def _snap(dev, loss):
    torch.cuda.synchronize()
    return dict(online=dev.online.flat.clone(), target=dev.target.flat.clone(), moment1=dev.adam_m.clone(), moment2=dev.adam_v.clone(), loss=loss[:BATCH].clone(),
                ring=dev.loss_ring.clone())


def _same(got, want, what):
    for k in want:
        if k in got:
            assert torch.equal(_bits(got[k]), _bits(want[k])), f"{what}: {k}"


_REFS = {}


def _eager(hip, hl_gauss, staged=False):
    """Five eager updates of DeviceLearner -> the state after every update, the engine.  ``hl_gauss`` None: a learner that never mentions the setting.  ``staged``: the
    target pass of every update runs as a separate stage first (tstage)."""
    key = (hl_gauss, staged)
    if key not in _REFS:
        w = _world()
        dev = _engine(hip, hl_gauss)
        ring = _dev(hip, w["ring"].reshape(-1))
        out = []
        for s in range(UPDATES):
            slots, a, r, d, wg = w[s]
            if staged:
                dev.target_stage(ring, _dev(hip, slots), ROW, s & 1)
            loss = dev.update(ring, _dev(hip, slots), ROW, _dev(hip, a), _dev(hip, r), _dev(hip, d), _dev(hip, wg), **(dict(tstage=s & 1) if staged else {}))
            out.append(_snap(dev, loss))
        assert int(dev.state[6]) == UPDATES and int(dev.state[1]) == UPDATES, "no update was NaN-skipped"
        _REFS[key] = (out, dev)
    return _REFS[key]


def test_the_update_issues_the_fused_kernel_and_off_is_plain_c51(hip):
    out, dev = _eager(hip, RHO)
    assert dev.hl_gauss == RHO and dev.hl_gauss_sigma == RHO * (20.0 / 50)
    T = dev.L.T
    # m_proj holds the Gaussian histogram: the stand-alone kernel on the engine's own logits of the last update reproduces it and the loss
    w = _world()
    _, a, r, d, wg = w[UPDATES - 1]
    loss2, dq2, m2, st2 = hip.empty(BATCH), hip.zeros(BATCH * ACTIONS * T), hip.empty(BATCH * T), hip.zeros(8, dtype=torch.int32)
    hip.loss_c51_hl_gauss(dev.ws_o.q, dev.ws_t.q, ACTIONS, T, _dev(hip, a), dev.a_star, _dev(hip, r), _dev(hip, d), _dev(hip, wg), dev.atoms, dev.gamma_n, dev.vmin, dev.vmax,
                          dev.hl_gauss_sigma, BATCH, loss2, dq2, m2, st2)
    torch.cuda.synchronize()
    assert torch.equal(_bits(m2), _bits(dev.m_proj[: BATCH * T])) and torch.equal(_bits(loss2), _bits(out[-1]["loss"]))
    assert float((m2.reshape(BATCH, T).sum(-1) - 1).abs().max()) < 1e-5
    plain, pdev = _eager(hip, None)
    off, odev = _eager(hip, 0.0)
    neg, _ = _eager(hip, -1.0)
    assert pdev.hl_gauss == odev.hl_gauss == 0.0
    for s in range(UPDATES):
        _same(off[s], plain[s], f"hl_gauss=0.0 against a learner that never mentions it, update {s + 1}")
        _same(neg[s], plain[s], f"hl_gauss=-1 against a learner that never mentions it, update {s + 1}")
    assert not torch.equal(out[0]["loss"], plain[0]["loss"]) and not torch.equal(out[0]["online"], plain[0]["online"]), "on differs from plain c51 after one update"


def test_a_staged_target_pass_gives_the_same_update(hip):
    """c51 allows tstage (DeviceLearner.target_stage_supported) and so does the setting: the stage ends at the target's fc1 slabs."""
    want, dev = _eager(hip, RHO)
    assert dev.target_stage_supported
    got, _ = _eager(hip, RHO, staged=True)
    for s in range(UPDATES):
        _same(got[s], want[s], f"staged target pass, update {s + 1}")


def test_graph_replays_equal_the_eager_updates(hip):
    from agent0_amd.deepq import agent
    from agent0_amd.deepq.config import parse_overrides
    want = _eager(hip, RHO)[0]
    cfg = parse_overrides(["learner.algo=c51", "seed=42", f"learner.batch_size={BATCH}", "learner.target_update_freq=2", f"action_dim={ACTIONS}", "obs_shape=(4,84,84)",
                           f"learner.c51.hl_gauss={RHO}"])
    ln = agent.C51Learner(cfg, ops=hip)
    assert ln.use_graph and ln.engine.hl_gauss == RHO
    _load(ln.engine)
    w = _world()
    ring = _dev(hip, w["ring"].reshape(-1))
    bufs = [_dev(hip, x) for x in w[0]]
    for s in range(UPDATES):
        for t, x in zip(bufs, w[s]):
            t.copy_(_dev(hip, x))
        loss, _ = ln.train_batch(ring, bufs[0], ROW, *bufs[1:])
        _same(_snap(ln.engine, loss), want[s], f"update {s + 1}")
    assert len(ln._graphs) == 1, "the last updates were replays of one captured graph"


def _handle(hip, **kw):
    return hip.native_learner(A=ACTIONS, dueling=False, double_q=kw.pop("double_q", False), B=BATCH, discount=0.99, lr=5e-4, target_update_freq=2, algo=kw.pop("algo", "c51"),
                              seed=SEED, **kw)


def test_handle_equals_the_eager_updates(hip):
    src = _engine(hip, None)
    w = _world()
    ring = _dev(hip, w["ring"].reshape(-1))
    for mode in ("on", "on-off", "never"):
        nat = _handle(hip)
        nat.set_params(src.online.flat, src.target.flat)
        if mode != "never":
            nat.set_hl_gauss(RHO)
        if mode == "on-off":
            nat.set_hl_gauss(0.0)                                  # on and off again: plain c51
        ref = _eager(hip, RHO if mode == "on" else None)[0]
        loss = hip.empty(BATCH)
        for s in range(UPDATES):
            slots, a, r, d, wg = w[s]
            nat.update(ring, _dev(hip, slots), ROW, _dev(hip, a), _dev(hip, r), _dev(hip, d), _dev(hip, wg), loss_out=loss)
            torch.cuda.synchronize()
            o, t, m, v, st = nat.get()
            _same(dict(online=o, target=t, moment1=m, moment2=v, loss=loss), ref[s], f"handle ({mode}), update {s + 1}")
            if mode == "never" and s == 1:
                nat.set_hl_gauss(-3.0)                             # between updates, off stays off
        nat.close()


def test_refusals(hip):
    from agent0_amd._abi import A0Error
    nat = _handle(hip)
    for ratio, word in ((float("nan"), r"hl_gauss = nan"), (float("inf"), r"hl_gauss = inf"), (float("-inf"), r"hl_gauss = -inf")):
        with pytest.raises(A0Error, match="a0_learner_set_hl_gauss.*learner.c51." + word):
            nat.set_hl_gauss(ratio)
    for ratio, word in ((51.5, r"ratio sigma / Delta = 51\.5"), (1e-45, r"sigma = 4e-46"), (1e300, r"ratio sigma / Delta = 1e\+300")):
        with pytest.raises(A0Error, match=r"a0_learner_set_hl_gauss.*learner\.c51\.hl_gauss.*" + word):
            nat.set_hl_gauss(ratio)
    nat.set_hl_gauss(51.0)                                         # the limit itself
    nat.set_hl_gauss(0.0)
    nat.close()
    for algo, code in (("dqn", 0), ("qr", 4), ("iqn", 2)):
        nat = _handle(hip, algo=algo, **(dict(K=4, N=8, N_dash=6) if algo == "iqn" else {}))
        with pytest.raises(A0Error, match=rf"a0_learner_set_hl_gauss.*hl_gauss = 0\.75 is for c51 handles only.*algo is {code}"):
            nat.set_hl_gauss(RHO)
        nat.set_hl_gauss(0.0)
        nat.set_hl_gauss(-1.0)
        nat.close()
    B, A, T = 3, 4, 51
    q, f, i = hip.zeros(B * A * T), hip.zeros(B), hip.zeros(B, dtype=torch.int32)
    out = torch.full((B * A * T,), GUARD, device=hip.device)
    st = hip.zeros(8, dtype=torch.int32)
    for sigma in (0.0, -0.3, float("nan"), float("inf"), 1e-40, 0.4 * 51.01):
        with pytest.raises(A0Error, match=r"a0_loss_c51_hl_gauss.*learner\.c51\.hl_gauss.*sigma = "):
            hip.loss_c51_hl_gauss(q, q, A, T, i, i, f, f, f, hip.zeros(T), 0.99, -10.0, 10.0, sigma, B, out, out, out, st)
    torch.cuda.synchronize()
    assert bool((out == GUARD).all()), "a refused call launches nothing"


# ------------------------------------------------------------------------------------------------ the Trainer: handles == Python classes, snapshots
BASE = ["learner.algo=c51", "actor.num_envs=16", "actor.sample_steps=8", "learner.batch_size=32", "learner.learner_steps=3", "replay.size=2000",
        "trainer.training_start_steps=200", "trainer.exploration_steps=512", "actor.min_eps=0.4", "learner.target_update_freq=4", "trainer.test_episodes=2", "wandb=false",
        "tb=false"]
CONFIGS = {"rainbow": ["learner.noisy_net=true", "learner.dueling_head=true", "learner.double_q=true", "learner.n_step_q=3", "replay.policy=prioritize"],
           "aug": ["learner.aug_shift=4"]}


def _trainer(tmp_path, monkeypatch, native, tag, config, rho=RHO, seed=42):
    from agent0_amd.deepq.config import parse_overrides
    from agent0_amd.deepq.trainer import Trainer
    monkeypatch.setenv("A0_NATIVE_LOOP", "1" if native else "0")
    return Trainer(parse_overrides(BASE + CONFIGS[config] + ([] if rho is None else [f"learner.c51.hl_gauss={rho}"]) + [f"seed={seed}", f"logdir={tmp_path / tag}"]))


def _state(tr):
    torch.cuda.synchronize()
    eng, rp = tr.learner.engine, tr.replay
    n = len(rp)                                       # the ring does not wrap in these runs
    out = [eng.online.flat.clone(), eng.target.flat.clone(), eng.adam_m.clone(), eng.adam_v.clone(), eng.state.clone(), eng.loss_ring.clone(), eng.online.wt.clone(),
           eng.target.wt.clone(), rp.frames[: n * rp.row_bytes].clone(), rp.act[:n].clone(), rp.rew[:n].clone(), rp.done[:n].clone(), rp._pstate.clone()]
    if rp.use_sumtree:
        out.append(rp._tree.clone())                  # the priorities
    return out


def _close(tr):
    tr.test = lambda: None
    tr.final(save=False)


_RUNS = {}


def _whole_run(tmp_path, monkeypatch, native, config, rho=RHO, iters=6):
    from agent0_amd.deepq.native_loop import NativeLoop
    key = (native, config, rho)
    if key not in _RUNS:
        tr = _trainer(tmp_path, monkeypatch, native, f"whole-{native}-{config}-{rho}", config, rho)
        assert tr.learner.engine.hl_gauss == (rho if rho and rho > 0 else 0.0)
        res = [{k: v for k, v in tr.run_iteration().items() if k != "fps"} for _ in range(iters)]
        assert isinstance(tr._nl, NativeLoop) if native else tr._nl is False, getattr(tr, "native_loop_reason", None)
        assert res[-1]["loss"] is not None, "updates ran"
        _RUNS[key] = (_state(tr), res, list(tr.Qs), list(tr.Rs), tr.frame_count)
        _close(tr)
    return _RUNS[key]


@pytest.mark.parametrize("config", list(CONFIGS))
def test_handles_and_python_classes_end_on_the_same_state(config, tmp_path, monkeypatch):
    """Six iterations of 128 transitions, three updates each once 200 are in the ring; the Python classes' last updates are replays of the hipGraph."""
    a, b = _whole_run(tmp_path, monkeypatch, False, config), _whole_run(tmp_path, monkeypatch, True, config)
    for i, (x, y) in enumerate(zip(a[0], b[0])):
        assert torch.equal(_bits(x), _bits(y)), f"{config}: state item {i}"
    assert a[1:5] == b[1:5]
    assert a[0][4][6].item() >= 9 and a[0][4][3].item() == 0, "updates ran, none NaN-skipped"
    if config == "aug":
        never, off = _whole_run(tmp_path, monkeypatch, True, config, rho=None), _whole_run(tmp_path, monkeypatch, True, config, rho=0.0)
        for i, (x, y) in enumerate(zip(never[0], off[0])):
            assert torch.equal(_bits(x), _bits(y)), f"off against a run that never mentions the setting: state item {i}"
        assert never[1:5] == off[1:5]
        assert never[0][4][1].item() == a[0][4][1].item() and not torch.equal(never[0][0], a[0][0]), "the setting changes the run"


@pytest.mark.parametrize("native", [True, False], ids=["handles", "python-classes"])
def test_a_snapshot_taken_mid_run_resumes_bit_for_bit(native, tmp_path, monkeypatch):
    want = _whole_run(tmp_path, monkeypatch, native, "aug")
    tr = _trainer(tmp_path, monkeypatch, native, "b", "aug")
    for _ in range(4):
        tr.run_iteration()
    assert tr.learner.engine.state[6].item() > 0, "updates have run"
    snap_dir = tr.save_snapshot(str(tmp_path / "snap"))
    _close(tr)
    tr = _trainer(tmp_path, monkeypatch, native, "c", "aug", seed=7)           # another seed: the snapshot's is the run's
    tr.load_snapshot(snap_dir)
    res = [{k: v for k, v in tr.run_iteration().items() if k != "fps"} for _ in range(2)]
    got = _state(tr)
    _close(tr)
    for i, (x, y) in enumerate(zip(got, want[0])):
        assert torch.equal(_bits(x), _bits(y)), f"state item {i}"
    assert res == want[1][4:]
