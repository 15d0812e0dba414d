"""GPU (MI355X): Munchausen-IQN targets (``learner.iqn.munchausen``): a0_miqn_target against float64, and the update that issues it.

1. The kernel against tests/miqn_ref.py (whose bound tests/test_miqn_reference_helpers.py fixes before any device run): (B, N', A) from one sample of one fraction and
   one action to 200 fractions (four rounds of the 64 lanes, the last ragged) and 32 actions (every lane of both half-waves), both layouts, tau = 0.03 and 1, with
   planted ties, an action gap of 10 (pi' one-hot in fp32 at tau = 0.03), the bonus at both seams of its clamp, done = 1, and alpha = 0.  Judged per element against
   e_y; the largest share of the bound is printed and recorded.  A NaN in one sample's q_next, then q_cur: that sample's targets are NaN, the others within bound.  Two
   runs give equal bytes, guard words around y stay, bad arguments are refused under the entry point's name.
   Work split (csrc/loss_quantile.hip): one wave per sample; lane l < 32 sums action l of q_next over j, lane 32 + l action l of q_cur; lanes stride over j for y.
2. The update, on a learner of 6 actions, 32 samples, K = 4, N = 8, N' = 6: (a) engine.y is ops.miqn_target of the engine's own two target passes, bit for bit; (b) on
   a batch whose st_next frames are copies of its st frames the new pass equals the target pass on s'; (c) the handle, DeviceLearner.update and IQNLearner with its
   hipGraph agree bit for bit after each of five updates, and the Trainer under the handles and under the Python classes ends on the same parameters, moments, target,
   loss ring and priorities — also with NoisyNet + dueling + 3-step + sum-tree, and with learner.aug_shift; (d) a snapshot taken mid-run resumes to the uninterrupted
   run's bytes under both loops; (e) the run differs from plain iqn from the first update on; (f) its Philox stream-3 position equals plain iqn's; (g) the refusals."""
import numpy as np
import pytest
import torch

import miqn_ref as M
import recipe
from util import record_stats

pytestmark = pytest.mark.gpu

GUARD = 12345.0


@pytest.fixture(scope="module")
def hip():
    from agent0_amd.ops import HipOps
    ops = HipOps()
    assert "gfx950" in ops.device_info()[2]
    assert hasattr(ops, "miqn_target")
    return ops


def _bits(t):
    return t.view(torch.int32) if t.dtype == torch.float32 else t


def _dev(hip, x):
    return torch.from_numpy(np.ascontiguousarray(x)).to(hip.device)


# ------------------------------------------------------------------------------------------------ 1. the kernel against float64
def _launch(hip, c, B, Nd, A, tau, layout, alpha=M.ALPHA, lo=M.LO, q_next=None, q_cur=None):
    sb, sj, sa = M.strides(layout, Nd, A)
    qn, qc = M.laid_out(c["q_next"] if q_next is None else q_next, layout), M.laid_out(c["q_cur"] if q_cur is None else q_cur, layout)
    buf = torch.full((16 + B * Nd + 16,), GUARD, device=hip.device)
    y = buf[16:16 + B * Nd]
    hip.miqn_target(_dev(hip, qn), _dev(hip, qc), sb, sj, sa, _dev(hip, c["act"]), _dev(hip, c["rew"]), _dev(hip, c["done"]), M.GAMMA, tau, alpha, lo, B, Nd, A, y)
    torch.cuda.synchronize()
    assert bool((buf[:16] == GUARD).all()) and bool((buf[16 + B * Nd:] == GUARD).all()), "nothing outside y is written"
    ref = M.miqn_target64(qn, qc, sb, sj, sa, c["act"], c["rew"], c["done"], M.GAMMA, tau, alpha, lo, B, Nd, A)
    return y.clone(), ref


def _share(got, ref, rows=None):
    g = got.cpu().numpy().astype(np.float64).reshape(ref["y"].shape)
    rows = np.arange(g.shape[0]) if rows is None else np.asarray(rows, np.int64)
    if len(rows) == 0:
        return 0.0
    assert np.isfinite(g[rows]).all()
    return float((np.abs(g[rows] - ref["y"][rows]) / ref["e_y"][rows]).max())


@pytest.mark.parametrize("tau", M.TAUS)
@pytest.mark.parametrize("layout", M.LAYOUTS)
@pytest.mark.parametrize("B,Nd,A", M.SHAPES, ids=str)
def test_kernel_against_float64(hip, B, Nd, A, layout, tau):
    c = M.case(B, Nd, A, tau)
    worst = {}
    for name, kw in (("alpha0.9", {}), ("alpha0", dict(alpha=0.0)), ("lo0", dict(lo=0.0))):
        got, ref = _launch(hip, c, B, Nd, A, tau, layout, **kw)
        worst[name] = _share(got, ref)
        again, _ = _launch(hip, c, B, Nd, A, tau, layout, **kw)
        assert torch.equal(_bits(got), _bits(again)), "two runs give equal bytes"
        if name != "alpha0.9":
            assert (ref["m"] == 0).all()
    print(f"(B, N', A)={(B, Nd, A)} {layout} tau={tau} planted={sorted(set(c['planted'].values()))}: largest share of the bound " +
          ", ".join(f"{k} {v:.3f}" for k, v in worst.items()))
    record_stats(f"miqn_target_b{B}_n{Nd}_a{A}_{layout}_tau{tau}", {"largest_error_over_bound": worst})
    assert max(worst.values()) <= 1.0, worst


@pytest.mark.parametrize("layout", M.LAYOUTS)
@pytest.mark.parametrize("B,Nd,A,tau", [(4, 64, 18, 0.03), (3, 200, 6, 1.0), (5, 7, 3, 0.03)], ids=str)
def test_a_nan_poisons_its_own_sample_only(hip, B, Nd, A, tau, layout):
    c = M.case(B, Nd, A, tau)
    for which in ("q_next", "q_cur"):
        for b, bad in ((B - 2, np.nan), (0, np.inf), (B - 1, -np.inf)):
            z = c[which].copy()
            z[b, Nd // 2, (int(c["act"][b]) + 1) % A] = bad             # not the taken action: the bonus's own lane never sees it
            got, ref = _launch(hip, c, B, Nd, A, tau, layout, **{which: z})
            g = got.cpu().numpy().reshape(B, Nd)
            assert ref["nan_rows"].tolist() == [i == b for i in range(B)]
            assert np.isnan(g[b]).all(), f"{which}: {bad} in sample {b} leaves finite targets {g[b]}"
            share = _share(got, ref, [i for i in range(B) if i != b])
            assert share <= 1.0, f"{which}: {bad} in sample {b} moved another sample to {share} bounds"


def test_argument_refusals(hip):
    from agent0_amd._abi import A0Error
    B, Nd, A = 3, 8, 4
    q = hip.zeros(B * Nd * A)
    act, f = hip.zeros(B, dtype=torch.int32), hip.zeros(B)
    y = torch.full((B * Nd,), GUARD, device=hip.device)
    ok = dict(tau=0.03, alpha=0.9, lo=-1.0, B=B, Nd=Nd, A=A)
    call = lambda **kw: (lambda a: hip.miqn_target(q, q, a["Nd"] * a["A"], a["A"], 1, act, f, f, 0.99, a["tau"], a["alpha"], a["lo"], a["B"], a["Nd"], a["A"], y))({**ok, **kw})
    for kw in (dict(tau=0.0), dict(tau=-1.0), dict(tau=float("nan")), dict(tau=float("inf")), dict(alpha=-0.1), dict(alpha=float("nan")), dict(lo=0.5),
               dict(lo=float("-inf")), dict(B=0), dict(Nd=0), dict(A=0)):
        with pytest.raises(A0Error, match="a0_miqn_target"):
            call(**kw)
    lib = hip.lib
    for nd, a in ((8193, 4), (8, 33)):
        assert lib.a0_miqn_target(q.data_ptr(), q.data_ptr(), nd * a, a, 1, act.data_ptr(), f.data_ptr(), f.data_ptr(), 0.99, 0.03, 0.9, -1.0, 1, nd, a, y.data_ptr(), None) == -1
    with pytest.raises(A0Error, match="q_cur"):      # the binding's own size check: the span of the strides
        hip.miqn_target(q, q[: B * Nd * A - 1], Nd * A, A, 1, act, f, f, 0.99, 0.03, 0.9, -1.0, B, Nd, A, y)
    torch.cuda.synchronize()
    assert bool((y == GUARD).all()), "a refused call launches nothing"


# ------------------------------------------------------------------------------------------------ 2. the update
ACTIONS, BATCH, RING, UPDATES = 6, 32, 64, 5
K, N, ND = 4, 8, 6
SHAPE = (4, 84, 84)
ROW = 2 * 4 * 84 * 84
SEED = 42 + 15485863            # BaseLearner's Philox seed for cfg.seed = 42
TAU, ALPHA, LO = 0.03, 0.9, -1.0
_WORLD = {}


def _world():
    if not _WORLD:
        _WORLD["ring"] = recipe.make_frames(RING, 78, SHAPE).reshape(RING, 2, *SHAPE)
        for s in range(UPDATES):
            a, r, d, w = recipe.make_transitions(BATCH, ACTIONS, 700 + s)
            _WORLD[s] = (recipe.gen(550 + s).integers(0, RING, BATCH).astype(np.int32), a.astype(np.int32), r, d.astype(np.float32), w)
    return _WORLD


def _spec():
    return recipe.NetSpec("iqn", ACTIONS, obs_shape=SHAPE)


def _engine(hip, munchausen=True, **kw):
    from agent0_amd.deepq.engine import DeviceLearner
    from agent0_amd.deepq.layout import NetLayout
    dev = DeviceLearner(hip, NetLayout.from_spec(_spec()), BATCH, target_update_freq=2, K=K, N=N, N_dash=ND, munchausen=munchausen, mdqn_tau=TAU, mdqn_alpha=ALPHA,
                        mdqn_lo=LO, **kw)
    _load(dev)
    return dev


def _load(dev):
    dev.online.load_state_dict(recipe.make_state_dict(_spec(), 11))
    dev.target.load_state_dict(recipe.make_state_dict(_spec(), 12))


def _snap(dev, loss):
    torch.cuda.synchronize()
    return dict(online=dev.online.flat.clone(), target=dev.target.flat.clone(), moment1=dev.adam_m.clone(), moment2=dev.adam_v.clone(), loss=loss[:BATCH].clone(),
                ring=dev.loss_ring.clone())


def _same(got, want, what):
    for k in want:
        if k in got:
            assert torch.equal(_bits(got[k]), _bits(want[k])), f"{what}: {k}"


_REFS = {}


def _eager(hip, munchausen):
    """Five eager updates of DeviceLearner with the fractions DeviceRng draws as BaseLearner.train_batch does -> the state after every update, the engine, the rng."""
    if munchausen not in _REFS:
        from agent0_amd.common.utils import DeviceRng
        w = _world()
        dev, rng = _engine(hip, munchausen), DeviceRng(hip, SEED)
        ring = _dev(hip, w["ring"].reshape(-1))
        taus = [hip.empty(BATCH * n) for n in (K, ND, N)]
        out = []
        for s in range(UPDATES):
            slots, a, r, d, wg = w[s]
            for t in taus:
                rng.uniform(rng.STREAM_TAUS, t, t.numel())
            loss = dev.update(ring, _dev(hip, slots), ROW, _dev(hip, a), _dev(hip, r), _dev(hip, d), _dev(hip, wg), rand=taus)
            out.append(_snap(dev, loss))
        assert int(dev.state[6]) == UPDATES and int(dev.state[1]) == UPDATES, "no update was NaN-skipped"
        _REFS[munchausen] = (out, dev, rng, taus)
    return _REFS[munchausen]


def test_engine_targets_are_the_kernel_on_its_own_passes(hip):
    """(a) and (e): after the last eager update engine.y is miqn_target of ws_t.q and ws_m.q; and the run is not plain iqn's."""
    out, dev, rng, taus = _eager(hip, True)
    assert dev.munchausen and dev.ws_m is not None and dev.ws_m.q.numel() == BATCH * ND * ACTIONS and (dev.mdqn_tau, dev.mdqn_alpha, dev.mdqn_lo) == (TAU, ALPHA, LO)
    w = _world()
    _, a, r, d, _ = w[UPDATES - 1]
    y = hip.empty(BATCH * ND)
    hip.miqn_target(dev.ws_t.q, dev.ws_m.q, ND * ACTIONS, ACTIONS, 1, _dev(hip, a), _dev(hip, r), _dev(hip, d), dev.gamma_n, TAU, ALPHA, LO, BATCH, ND, ACTIONS, y)
    torch.cuda.synchronize()
    assert torch.equal(_bits(y), _bits(dev.y[: BATCH * ND])) and bool(torch.isfinite(y).all())
    plain, pdev, prng, _ = _eager(hip, False)
    assert pdev.munchausen is False and pdev.ws_m is None, "off: no buffer"
    assert not torch.equal(out[0]["loss"], plain[0]["loss"]) and not torch.equal(out[0]["online"], plain[0]["online"]), "differs from plain iqn from the first update on"
    # (f) the stream position: the K draw is made and left unused
    assert rng.offsets[rng.STREAM_TAUS] == prng.offsets[prng.STREAM_TAUS] == UPDATES * sum((BATCH * n + 3) // 4 * 4 for n in (K, ND, N))


def test_the_new_pass_is_the_target_network_on_the_current_observation(hip):
    """(b): st_next := st makes the pass on s the pass on s'."""
    w = _world()
    dev = _engine(hip)
    slots, a, r, d, wg = w[0]
    batch = w["ring"][slots].copy()
    batch[:, 1] = batch[:, 0]
    taus = [torch.rand(BATCH * n, device=hip.device) for n in (K, ND, N)]
    dev.forward_dense(_dev(hip, batch.reshape(-1)), None, ROW, _dev(hip, a), _dev(hip, r), _dev(hip, d), _dev(hip, wg), rand=taus)
    torch.cuda.synchronize()
    n = BATCH * ND * ACTIONS
    assert torch.equal(_bits(dev.ws_m.q[:n]), _bits(dev.ws_t.q[:n])) and torch.equal(_bits(dev.ws_m.act3), _bits(dev.ws_t.act3))
    assert float(dev.ws_m.q[:n].abs().max()) > 0
    dev2 = _engine(hip)
    dev2.forward_dense(_dev(hip, w["ring"].reshape(-1)), _dev(hip, slots), ROW, _dev(hip, a), _dev(hip, r), _dev(hip, d), _dev(hip, wg), rand=taus)
    torch.cuda.synchronize()
    assert not torch.equal(dev2.ws_m.q[:n], dev2.ws_t.q[:n]), "on the ring's own rows s and s' differ, and so do the passes"
    assert torch.equal(_bits(dev2.ws_m.q[:n]), _bits(dev.ws_m.q[:n])), "the new pass reads st: changing st_next does not move it"


def test_graph_replays_equal_the_eager_updates(hip):
    """(c), Python classes: IQNLearner.train_batch draws the fractions and replays the update from its hipGraph from the third update on."""
    from agent0_amd.deepq import agent
    from agent0_amd.deepq.config import parse_overrides
    want = _eager(hip, True)[0]
    cfg = parse_overrides(["learner.algo=iqn", "seed=42", f"learner.batch_size={BATCH}", "learner.target_update_freq=2", f"action_dim={ACTIONS}", "obs_shape=(4,84,84)",
                           "learner.iqn.munchausen=true", f"learner.iqn.K={K}", f"learner.iqn.N={N}", f"learner.iqn.N_dash={ND}"])
    ln = agent.IQNLearner(cfg, ops=hip)
    assert ln.use_graph and ln.rng.seed == SEED and ln.engine.munchausen and ln.engine.mdqn_alpha == 0.9
    _load(ln.engine)
    w = _world()
    ring = _dev(hip, w["ring"].reshape(-1))
    bufs = [_dev(hip, x) for x in w[0]]
    for s in range(UPDATES):
        for t, x in zip(bufs, w[s]):
            t.copy_(_dev(hip, x))
        loss, _ = ln.train_batch(ring, bufs[0], ROW, *bufs[1:])
        _same(_snap(ln.engine, loss), want[s], f"update {s + 1}")
    assert len(ln._graphs) == 1, "the last three updates were replays of one captured graph"
    assert ln.rng.offsets[ln.rng.STREAM_TAUS] == _eager(hip, True)[2].offsets[3]


def _handle(hip, **kw):
    return hip.native_learner(A=ACTIONS, dueling=False, double_q=kw.pop("double_q", False), B=BATCH, discount=0.99, lr=5e-4, target_update_freq=2, algo=kw.pop("algo", "iqn"),
                              seed=SEED, K=K, N=N, N_dash=ND, **kw)


def test_handle_equals_the_eager_updates(hip):
    """(c), the handle; (f) its stream position; (g) the setter after the first update."""
    import ctypes as C
    from agent0_amd._abi import A0Error
    want, dev, _, _ = _eager(hip, True)
    src = _engine(hip, False)
    w = _world()
    ring = _dev(hip, w["ring"].reshape(-1))
    pos = {}
    for on in (True, False):
        nat = _handle(hip)
        nat.set_params(src.online.flat, src.target.flat)
        if on:
            nat.set_munchausen(True, TAU, ALPHA, LO)
        else:
            nat.set_munchausen(True, TAU, ALPHA, LO)
            nat.set_munchausen(False, TAU, ALPHA, LO)              # on and off again: plain iqn
        loss = hip.empty(BATCH)
        ref = want if on else _eager(hip, False)[0]
        for s in range(UPDATES):
            slots, a, r, d, wg = w[s]
            nat.update(ring, _dev(hip, slots), ROW, _dev(hip, a), _dev(hip, r), _dev(hip, d), _dev(hip, wg), loss_out=loss)
            torch.cuda.synchronize()
            o, t, m, v, st = nat.get()
            _same(dict(online=o, target=t, moment1=m, moment2=v, loss=loss), ref[s], f"handle (munchausen={on}), update {s + 1}")
        words = (C.c_ulonglong * 9)()
        assert hip.lib.a0_learner_rng_state(nat.h, words, 0) == 0
        pos[on] = int(words[1 + 3])
        with pytest.raises(A0Error, match="a0_learner_set_munchausen.*fixed once the handle has run an update"):
            nat.set_munchausen(not on, TAU, ALPHA, LO)
        nat.close()
    assert pos[True] == pos[False] == UPDATES * sum((BATCH * n + 3) // 4 * 4 for n in (K, ND, N))


def test_refusals(hip, monkeypatch):
    """(g)"""
    from agent0_amd._abi import A0Error
    from agent0_amd.deepq.engine import DeviceLearner
    from agent0_amd.deepq.layout import NetLayout
    nat = _handle(hip)
    for kw, word in ((dict(tau=0.0), r"mdqn\.tau = 0"), (dict(tau=float("nan")), r"mdqn\.tau = nan"), (dict(tau=1e-60), r"mdqn\.tau = 1e-60"), (dict(alpha=-0.5), r"mdqn\.alpha = -0\.5"),
                     (dict(alpha=float("inf")), r"mdqn\.alpha = inf"), (dict(lo=0.25), r"mdqn\.lo = 0\.25"), (dict(lo=float("-inf")), r"mdqn\.lo = -inf")):
        for on in (True, False):
            with pytest.raises(A0Error, match="a0_learner_set_munchausen.*" + word):
                nat.set_munchausen(on, **{**dict(tau=TAU, alpha=ALPHA, lo=LO), **kw})
    nat.close()
    nat = _handle(hip, double_q=True)
    with pytest.raises(A0Error, match="a0_learner_set_munchausen.*double_q"):
        nat.set_munchausen(True)
    nat.close()
    for algo, code in (("fqf", 3), ("dqn", 0)):
        nat = _handle(hip, algo=algo, **(dict(F=8) if algo == "fqf" else {}))
        with pytest.raises(A0Error, match=f"a0_learner_set_munchausen.*iqn handles only.*algo is {code}"):
            nat.set_munchausen(True)
        nat.set_munchausen(False)
        nat.close()
    L = NetLayout.from_spec(_spec())
    with pytest.raises(ValueError, match=r"learner\.iqn\.munchausen.*learner\.double_q"):
        DeviceLearner(hip, L, BATCH, K=K, N=N, N_dash=ND, munchausen=True, double_q=True)
    for algo in ("fqf", "dqn"):
        with pytest.raises(ValueError, match=rf"learner\.iqn\.munchausen.*learner\.algo={algo}"):
            DeviceLearner(hip, NetLayout.from_spec(recipe.NetSpec(algo, ACTIONS, obs_shape=SHAPE)), BATCH, munchausen=True)
    for kw, key in ((dict(mdqn_tau=0.0), "tau"), (dict(mdqn_alpha=-1.0), "alpha"), (dict(mdqn_lo=0.5), "lo"), (dict(mdqn_tau=float("nan")), "tau")):
        with pytest.raises(ValueError, match=rf"learner\.iqn\.munchausen.*learner\.mdqn\.{key}="):
            DeviceLearner(hip, L, BATCH, K=K, N=N, N_dash=ND, munchausen=True, **kw)
    monkeypatch.setenv("A0_PIPELINE_TARGET", "1")
    with pytest.raises(ValueError, match=r"learner\.iqn\.munchausen.*A0_PIPELINE_TARGET"):
        DeviceLearner(hip, L, BATCH, K=K, N=N, N_dash=ND, munchausen=True)
    monkeypatch.setenv("A0_PIPELINE_TARGET", "0")
    dev, w = _engine(hip), _world()
    slots, a, r, d, wg = w[0]
    with pytest.raises(ValueError, match="tstage"):
        dev.forward_dense(_dev(hip, w["ring"].reshape(-1)), _dev(hip, slots), ROW, _dev(hip, a), _dev(hip, r), _dev(hip, d), _dev(hip, wg),
                          rand=[hip.zeros(BATCH * n) for n in (K, ND, N)], tstage=0)


# ------------------------------------------------------------------------------------------------ the Trainer: handles == Python classes, snapshots
BASE = ["learner.algo=iqn", f"learner.iqn.K={K}", f"learner.iqn.N={N}", f"learner.iqn.N_dash={ND}", "actor.num_envs=16", "actor.sample_steps=8", "learner.batch_size=32",
        "learner.learner_steps=3", "replay.size=2000", "trainer.training_start_steps=200", "trainer.exploration_steps=512", "actor.min_eps=0.4",
        "learner.target_update_freq=4", "trainer.test_episodes=2", "wandb=false", "tb=false"]
CONFIGS = {"plain": [],
           "rainbow": ["learner.noisy_net=true", "learner.dueling_head=true", "learner.n_step_q=3", "replay.policy=prioritize"],
           "aug": ["learner.aug_shift=4"]}


def _trainer(tmp_path, monkeypatch, native, tag, config, on=True, seed=42):
    from agent0_amd.deepq.config import parse_overrides
    from agent0_amd.deepq.trainer import Trainer
    monkeypatch.setenv("A0_NATIVE_LOOP", "1" if native else "0")
    return Trainer(parse_overrides(BASE + CONFIGS[config] + [f"learner.iqn.munchausen={'true' if on else 'false'}", f"seed={seed}", f"logdir={tmp_path / tag}"]))


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


def _whole_run(tmp_path, monkeypatch, native, config, on=True, iters=6):
    from agent0_amd.deepq.native_loop import NativeLoop
    key = (native, config, on)
    if key not in _RUNS:
        tr = _trainer(tmp_path, monkeypatch, native, f"whole-{native}-{config}-{on}", config, on)
        assert tr.learner.engine.munchausen is on
        res = [{k: v for k, v in tr.run_iteration().items() if k != "fps"} for _ in range(iters)]
        assert isinstance(tr._nl, NativeLoop) if native else tr._nl is False, getattr(tr, "native_loop_reason", None)
        assert res[-1]["loss"] is not None, "updates ran"
        _RUNS[key] = (_state(tr), res, list(tr.Qs), list(tr.Rs), tr.frame_count, int(tr.learner.rng.offsets.get(3, 0)))
        _close(tr)
    return _RUNS[key]


@pytest.mark.parametrize("config", list(CONFIGS))
def test_handles_and_python_classes_end_on_the_same_state(config, tmp_path, monkeypatch):
    """(c): six iterations of 128 transitions, three updates each once 200 are in the ring; the Python classes' last updates are replays of the hipGraph."""
    a, b = _whole_run(tmp_path, monkeypatch, False, config), _whole_run(tmp_path, monkeypatch, True, config)
    for i, (x, y) in enumerate(zip(a[0], b[0])):
        assert torch.equal(_bits(x), _bits(y)), f"{config}: state item {i}"
    assert a[1:5] == b[1:5]
    assert a[0][4][6].item() >= 9 and a[0][4][3].item() == 0, "updates ran, none NaN-skipped"
    if config == "plain":
        off = _whole_run(tmp_path, monkeypatch, True, config, on=False)
        assert off[0][4][1].item() == a[0][4][1].item() and not torch.equal(off[0][0], a[0][0]), "(e) the setting changes the run"
        assert off[1][1]["loss"] != a[1][1]["loss"], "(e) from the first update block on"
        assert _whole_run(tmp_path, monkeypatch, False, config, on=False)[5] == a[5] > 0, "(f) the Python classes' stream-3 position is plain iqn's"


@pytest.mark.parametrize("native", [True, False], ids=["handles", "python-classes"])
def test_a_snapshot_taken_mid_run_resumes_bit_for_bit(native, tmp_path, monkeypatch):
    """(d)"""
    want = _whole_run(tmp_path, monkeypatch, native, "plain")
    tr = _trainer(tmp_path, monkeypatch, native, "b", "plain")
    for _ in range(4):
        tr.run_iteration()
    assert tr.learner.engine.state[6].item() > 0, "updates have run"
    snap_dir = tr.save_snapshot(str(tmp_path / "snap"))
    _close(tr)
    tr = _trainer(tmp_path, monkeypatch, native, "c", "plain", seed=7)           # another seed: the snapshot's is the run's
    tr.load_snapshot(snap_dir)
    res = [{k: v for k, v in tr.run_iteration().items() if k != "fps"} for _ in range(2)]
    got = _state(tr)
    _close(tr)
    for i, (x, y) in enumerate(zip(got, want[0])):
        assert torch.equal(_bits(x), _bits(y)), f"state item {i}"
    assert res == want[1][4:]
