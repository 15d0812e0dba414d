"""GPU (MI355X): ``learner.iqn.risk`` — a0_risk_distort against the float64 restatement (tests/iqn_risk_ref.py), the fused draw + distortion + cosine launch
against the three-launch chain, the update's selection fractions, the actor's fractions, and whole Trainer runs under the handles and the Python classes."""
import numpy as np
import pytest
import torch

import iqn_risk_ref as R
import recipe
from util import record_stats

pytestmark = pytest.mark.gpu

GUARD = 12345.0
KINDS = R.KINDS
CASES = [(k, e) for k in ("cvar", "pow", "cpw", "wang") for e in dict.fromkeys(R.PAPER_ETA[k] + R.RANGE_ENDS[k])]


@pytest.fixture(scope="module")
def hip():
    from agent0_amd.ops import HipOps
    ops = HipOps()
    assert "gfx950" in ops.device_info()[2]
    assert hasattr(ops, "risk_distort") and hasattr(ops, "tau_cos_features_risk")
    return ops


def _bits(t):
    return t.view(torch.int32) if t.dtype == torch.float32 else t


def _dev(hip, x):
    return torch.from_numpy(np.ascontiguousarray(x)).to(hip.device)


_REF = {}


def _ref(kind, eta):
    """The float64 values over the 4 + 4096 fractions, computed once per (kind, eta)."""
    if (kind, eta) not in _REF:
        _REF[kind, eta] = R.beta_array(kind, eta, R.fractions(4100))
    return _REF[kind, eta]


# ------------------------------------------------------------------------------------------------ 1. a0_risk_distort against float64
def _distort(hip, taus, kind, eta, in_place, head=0):
    """``head``: floats by which both buffers start behind a 16-byte boundary (0: the 16-byte path, else element by element)."""
    n = taus.size
    buf = torch.full((16 + head + n + 16,), GUARD, device=hip.device)
    out = buf[16 + head:16 + head + n]
    if in_place:
        out.copy_(_dev(hip, taus))
        hip.risk_distort(out, out, n, KINDS[kind], eta)
    else:
        src = torch.zeros(16 + head + n, device=hip.device)[16 + head:]
        src.copy_(_dev(hip, taus))
        hip.risk_distort(src, out, n, KINDS[kind], eta)
        torch.cuda.synchronize()
        assert torch.equal(_bits(src), _bits(_dev(hip, taus))), "the input is only read"
    torch.cuda.synchronize()
    assert bool((buf[:16 + head] == GUARD).all()) and bool((buf[16 + head + n:] == GUARD).all()), "nothing outside out is written"
    return out.clone()


@pytest.mark.parametrize("kind,eta", CASES, ids=str)
def test_distort_against_float64(hip, kind, eta):
    """Every kind at the paper's eta and at the ends of its range; n = 1, 3, 257, 4099 and all 4100; in place and out of place; aligned and unaligned heads.
    cvar: numpy float32's bits.  The others: one fp32 spacing at the float64 value (derived in iqn_risk_ref)."""
    taus, ref = R.fractions(4100), _ref(kind, eta)
    worst, differ = 0.0, 0.0
    for n, head, in_place in ((1, 0, False), (1, 0, True), (1, 1, True), (3, 1, True), (3, 0, False), (3, 1, False), (257, 0, True), (257, 3, False), (4099, 0, False), (4099, 2, True), (4100, 0, False), (4100, 0, True)):
        got = _distort(hip, taus[:n], kind, eta, in_place, head).cpu().numpy()
        again = _distort(hip, taus[:n], kind, eta, in_place, head).cpu().numpy()
        assert np.array_equal(got.view(np.int32), again.view(np.int32)), "two runs give equal bytes"
        assert got[0] == 0.0 and np.all(got >= 0.0) and np.all(got <= 1.0)
        if kind == "cvar":
            assert np.array_equal(got.view(np.int32), R.cvar_f32(eta, taus[:n]).view(np.int32)), (n, head, in_place)
            continue
        err = np.abs(got.astype(np.float64) - ref[:n]) / R.spacing32(ref[:n])
        worst = max(worst, float(err.max()))
        differ = max(differ, float((got != ref[:n].astype(np.float32)).mean()))
        print(f"risk_distort {kind} eta={eta} n={n} head={head} in_place={in_place}: largest deviation {err.max():.4f} spacings, "
              f"{(got != ref[:n].astype(np.float32)).mean():.5f} of the elements differ from fl32(ref)")
        assert err.max() <= 1.0, (n, head, in_place, float(err.max()))
    record_stats(f"iqn_risk_distort_{kind}_eta{eta}", {"largest_deviation_in_fp32_spacings": worst, "largest_share_differing_from_fl32_ref": differ})


def test_identities_and_neutral(hip):
    taus = R.fractions(4100)
    for kind, eta in (("neutral", 0.0), ("neutral", 3.5), ("cvar", 1.0), ("pow", 0.0), ("cpw", 1.0)):
        for head in (0, 1):
            assert np.array_equal(_distort(hip, taus, kind, eta, False, head).cpu().numpy().view(np.int32), taus.view(np.int32)), (kind, eta, head)
    nan = np.array([np.nan, 0.25, 0.0, 0.5, np.nan], dtype=np.float32)
    for kind, eta in (("cvar", 0.25), ("pow", -2.0), ("cpw", 0.71), ("wang", 0.75)):
        got = _distort(hip, nan, kind, eta, False).cpu().numpy()
        assert np.isnan(got[[0, 4]]).all() and np.isfinite(got[1:4]).all() and got[2] == 0.0, "a NaN stays a NaN, and its own"


def test_distort_refusals(hip):
    from agent0_amd._abi import A0Error
    t = torch.full((8,), GUARD, device=hip.device)
    for kind, eta, word in ((1, 0.0, "risk_eta = 0 "), (1, 1.5, "risk_eta = 1.5"), (1, float("nan"), "risk_eta = nan"), (2, 65.0, "risk_eta = 65"), (3, 0.0, "0.71"),
                            (3, -1.0, "risk_eta = -1"), (4, float("inf"), "risk_eta = inf"), (4, -8.5, "risk_eta = -8.5"), (5, 0.5, "learner.iqn.risk = 5"), (-1, 0.5, "learner.iqn.risk = -1")):
        with pytest.raises(A0Error, match="a0_risk_distort: .*" + word.replace(".", r"\.")):
            hip.risk_distort(t, t, 8, kind, eta)
        with pytest.raises(A0Error, match="a0_tau_cos_features_risk: .*" + word.replace(".", r"\.")):
            hip.tau_cos_features_risk(1, 3, 0, t, hip.zeros(8 * 64), 8, 64, kind, eta)
    assert hip.lib.a0_risk_distort(t.data_ptr(), t.data_ptr(), 0, 1, 0.25, None) == -1 and hip.lib.a0_risk_distort(None, t.data_ptr(), 8, 1, 0.25, None) == -1
    torch.cuda.synchronize()
    assert bool((t == GUARD).all()), "a refused call launches nothing"


# ------------------------------------------------------------------------------------------------ 2. the fused launch equals the chain
@pytest.mark.parametrize("with_ctrl", [False, True], ids=["no-ctrl", "ctrl"])
@pytest.mark.parametrize("kind,eta", [("neutral", 0.0), ("cvar", 0.25), ("pow", -2.0), ("cpw", 0.71), ("wang", 0.75), ("wang", -0.75)], ids=str)
def test_fused_launch_equals_the_three_launch_chain(hip, kind, eta, with_ctrl):
    seed, stream, D = (7 << 32) | 99, 3, 64
    for Rr, offset, D in ((1, 0, 64), (15, 1, 64), (4 * 5 + 3, 6, 64), (23, 4 * 1000 + 3, 64), (300, 2, 64), (9, 5, 7), (700, 3, 1)):
        ctrl = hip.zeros(8, dtype=torch.int64) if with_ctrl else None
        delta = 0
        if with_ctrl:
            delta = 4 * 3 + 1
            ctrl[5] = delta
        tb, cb = torch.full((8 + Rr + 8,), GUARD, device=hip.device), torch.full((8 + Rr * D + 8,), GUARD, device=hip.device)
        taus, cosx = tb[8:8 + Rr], cb[8:8 + Rr * D]
        hip.tau_cos_features_risk(seed, stream, offset, taus, cosx, Rr, D, KINDS[kind], eta, ctrl=ctrl, ctrl_idx=5)
        u, t2, c2 = hip.empty(Rr), hip.empty(Rr), hip.empty(Rr * D)
        hip.rng_uniform(seed, stream, offset + delta, u, Rr)
        hip.risk_distort(u, t2, Rr, KINDS[kind], eta)
        hip.cos_features(t2, c2, Rr, D)
        torch.cuda.synchronize()
        assert torch.equal(_bits(taus), _bits(t2)), (Rr, offset, D, "taus")
        assert torch.equal(_bits(cosx), _bits(c2)), (Rr, offset, D, "cosines")
        assert bool((tb[:8] == GUARD).all()) and bool((tb[8 + Rr:] == GUARD).all()) and bool((cb[:8] == GUARD).all()) and bool((cb[8 + Rr * D:] == GUARD).all())
        if kind == "neutral":
            t3, c3 = hip.empty(Rr), hip.empty(Rr * D)
            hip.tau_cos_features(seed, stream, offset, t3, c3, Rr, D, ctrl=ctrl, ctrl_idx=5)
            torch.cuda.synchronize()
            assert torch.equal(_bits(taus), _bits(t3)) and torch.equal(_bits(cosx), _bits(c3)), "neutral equals a0_tau_cos_features"


# ------------------------------------------------------------------------------------------------ 3. the update
ACTIONS, BATCH, RING, UPDATES = 6, 32, 64, 5
K, N, ND = 4, 8, 6
SHAPE = (4, 84, 84)
ROW = 2 * 4 * 84 * 84
SEED = 42 + 15485863            # BaseLearner's Philox seed for cfg.seed = 42
_WORLD = {}


def _world():
    if not _WORLD:
        _WORLD["ring"] = recipe.make_frames(RING, 78, SHAPE).reshape(RING, 2, *SHAPE)
        for s in range(UPDATES):
            a, r, d, w = recipe.make_transitions(BATCH, ACTIONS, 700 + s)
            _WORLD[s] = (recipe.gen(550 + s).integers(0, RING, BATCH).astype(np.int32), a.astype(np.int32), r, d.astype(np.float32), w)
    return _WORLD


def _spec(**kw):
    return recipe.NetSpec("iqn", ACTIONS, obs_shape=SHAPE, **kw)


def _load(dev, **kw):
    dev.online.load_state_dict(recipe.make_state_dict(_spec(**kw), 11))
    dev.target.load_state_dict(recipe.make_state_dict(_spec(**kw), 12))


def _engine(hip, risk="neutral", eta=0.0, **kw):
    from agent0_amd.deepq.engine import DeviceLearner
    from agent0_amd.deepq.layout import NetLayout
    dev = DeviceLearner(hip, NetLayout.from_spec(_spec()), BATCH, target_update_freq=2, K=K, N=N, N_dash=ND, risk=risk, risk_eta=eta, **kw)
    _load(dev)
    return dev


def _snap(dev, loss):
    torch.cuda.synchronize()
    return dict(online=dev.online.flat.clone(), target=dev.target.flat.clone(), moment1=dev.adam_m.clone(), moment2=dev.adam_v.clone(), loss=loss[:BATCH].clone(),
                ring=dev.loss_ring.clone(), a_star=dev.a_star.clone())


def _same(got, want, what):
    for k in want:
        if k in got:
            assert torch.equal(_bits(got[k]), _bits(want[k])), f"{what}: {k}"


_EAGER = {}


def _eager(hip, risk, eta, feed=None, double_q=False):
    """Five eager updates of DeviceLearner with the fractions DeviceRng draws as BaseLearner.train_batch does.  ``feed``: a NEUTRAL engine whose K fractions are
    replaced, through the ``rand`` hook, by ``feed(draws)``.  -> the state after every update, the engine, the rng, the fraction buffers as last drawn."""
    key = (risk, eta, feed is not None, double_q)
    if key not in _EAGER:
        from agent0_amd.common.utils import DeviceRng
        w = _world()
        dev, rng = _engine(hip, "neutral" if feed else risk, 0.0 if feed else eta, double_q=double_q), DeviceRng(hip, SEED)
        ring = _dev(hip, w["ring"].reshape(-1))
        taus = [hip.empty(BATCH * n) for n in (K, ND, N)]
        out = []
        for s in range(UPDATES):
            slots, a, r, d, wg = w[s]
            for t in taus:
                rng.uniform(rng.STREAM_TAUS, t, t.numel())
            drawn = taus[0].clone()
            rand = [feed(taus[0]), taus[1], taus[2]] if feed else taus
            loss = dev.update(ring, _dev(hip, slots), ROW, _dev(hip, a), _dev(hip, r), _dev(hip, d), _dev(hip, wg), rand=rand)
            torch.cuda.synchronize()
            assert torch.equal(_bits(taus[0]), _bits(drawn)), "the caller's fractions are only read"
            out.append(_snap(dev, loss))
        assert int(dev.state[6]) == UPDATES and int(dev.state[1]) == UPDATES, "no update was NaN-skipped"
        _EAGER[key] = (out, dev, rng, taus)
    return _EAGER[key]


@pytest.mark.parametrize("double_q", [False, True], ids=["target-selects", "double-q"])
@pytest.mark.parametrize("kind,eta", [("cvar", 0.25), ("pow", -2.0), ("cpw", 0.71), ("wang", -0.75)], ids=str)
def test_update_selects_with_the_distorted_fractions_only(hip, kind, eta, double_q):
    """a_star — and with it everything behind it — equals a neutral update fed, through the rand hook, the K fractions distorted by the float64 reference (cvar) or
    by a0_risk_distort (the other kinds); the N' and N fractions and the Philox position are a neutral run's."""
    def feed(t):
        if kind == "cvar":
            return _dev(hip, R.cvar_f32(eta, t.cpu().numpy()))
        out = hip.empty(t.numel())
        hip.risk_distort(t, out, t.numel(), KINDS[kind], eta)
        return out
    got, dev, rng, taus = _eager(hip, kind, eta, double_q=double_q)
    want, ndev, nrng, ntaus = _eager(hip, kind, eta, feed=feed, double_q=double_q)
    assert dev.risk_kind == KINDS[kind] and dev.t_risk.numel() == BATCH * K and ndev.risk_kind == 0 and ndev.t_risk is None
    for s in range(UPDATES):
        _same(got[s], want[s], f"{kind} update {s + 1}")
    assert torch.equal(_bits(dev.t_risk), _bits(feed(taus[0])))
    for a, b in zip(taus, ntaus):
        assert torch.equal(_bits(a), _bits(b)), "all three draws are a neutral run's"
    assert rng.offsets[rng.STREAM_TAUS] == nrng.offsets[nrng.STREAM_TAUS] == UPDATES * sum((BATCH * n + 3) // 4 * 4 for n in (K, ND, N))
    plain = _eager(hip, "neutral", 0.0, double_q=double_q)[0]
    assert any(not torch.equal(got[s]["a_star"], plain[s]["a_star"]) for s in range(UPDATES)), "the distortion moves the greedy next action"


HANDLE_CONFIGS = {"plain": dict(), "double-dueling-3step": dict(double_q=True, dueling=True, n_step=3),
                  "double-dueling-noisy-3step-sumtree": dict(double_q=True, dueling=True, n_step=3, noisy=True)}


@pytest.mark.parametrize("config", list(HANDLE_CONFIGS))
def test_handle_engine_and_graphed_learner_agree_after_every_update(hip, config):
    """The handle, DeviceLearner.update (IQNLearner, eager) and IQNLearner under its hipGraph, bit for bit after each of five updates — in every configuration,
    NoisyNet included: the handle draws both networks' noise per update from Philox stream 4 of the same seed, from the offset the Python learner starts at.
    (The batches carry importance weights, as a sum-tree batch does; the tree itself belongs to the replay and is held by the Trainer runs below.)"""
    import ctypes as C
    from agent0_amd._abi import A0Error
    from agent0_amd.deepq import agent
    from agent0_amd.deepq.config import parse_overrides
    kind, eta = "wang", -0.75
    hc = HANDLE_CONFIGS[config]
    dq, duel, nstep, noisy = hc.get("double_q", False), hc.get("dueling", False), hc.get("n_step", 1), hc.get("noisy", False)
    over = ["learner.algo=iqn", "seed=42", f"learner.batch_size={BATCH}", "learner.target_update_freq=2", f"action_dim={ACTIONS}", "obs_shape=(4,84,84)",
            f"learner.iqn.risk={kind}", f"learner.iqn.risk_eta={eta}", f"learner.iqn.K={K}", f"learner.iqn.N={N}", f"learner.iqn.N_dash={ND}",
            f"learner.double_q={str(dq).lower()}", f"learner.dueling_head={str(duel).lower()}", f"learner.noisy_net={str(noisy).lower()}", f"learner.n_step_q={nstep}"]
    if noisy:
        over.append("replay.policy=prioritize")
    kw = dict(dueling=duel, noisy=noisy)
    w = _world()
    ring = _dev(hip, w["ring"].reshape(-1))
    runs, start = {}, None
    for graph in (False, True):
        ln = agent.IQNLearner(parse_overrides(list(over)), ops=hip)
        ln.use_graph = graph
        assert ln.engine.risk_kind == KINDS[kind] and ln.engine.risk_eta == eta and ln.engine.double_q is dq
        _load(ln.engine, **kw)
        torch.cuda.synchronize()
        if start is None:      # what the handle starts from: the parameters and the position of the noise stream
            start = (ln.engine.online.flat.clone(), ln.engine.target.flat.clone(), int(ln.rng.offsets.get(ln.rng.STREAM_NOISE, 0)))
        bufs = [_dev(hip, x) for x in w[0]]
        out = []
        for s in range(UPDATES):
            for t, x in zip(bufs, w[s]):
                t.copy_(_dev(hip, x))
            loss, _ = ln.train_batch(ring, bufs[0], ROW, *bufs[1:])
            out.append(_snap(ln.engine, loss))
        assert (len(ln._graphs) == 1) is graph
        runs[graph] = out
    for s in range(UPDATES):
        _same(runs[True][s], runs[False][s], f"hipGraph against eager, update {s + 1}")
    # the handle: its own draws from the same seed
    nat = hip.native_learner(A=ACTIONS, dueling=duel, double_q=dq, B=BATCH, n_step=nstep, discount=0.99, lr=5e-4, target_update_freq=2, algo="iqn", noisy=noisy, seed=SEED,
                             K=K, N=N, N_dash=ND)
    nat.set_params(start[0], start[1])
    if noisy:
        assert hip.lib.a0_learner_set_rng(nat.h, 4, C.c_ulonglong(start[2])) == 0
    nat.set_risk(kind, eta)
    loss = hip.empty(BATCH)
    for s in range(UPDATES):
        slots, a, r, d, wg = w[s]
        nat.update(ring, _dev(hip, slots), ROW, _dev(hip, a), _dev(hip, r), _dev(hip, d), _dev(hip, wg), loss_out=loss)
        torch.cuda.synchronize()
        o, t, m, v, st = nat.get()
        _same(dict(online=o, target=t, moment1=m, moment2=v, loss=loss), runs[False][s], f"handle ({config}), update {s + 1}")
    words = (C.c_ulonglong * 9)()
    assert hip.lib.a0_learner_rng_state(nat.h, words, 0) == 0
    assert int(words[1 + 3]) == UPDATES * sum((BATCH * n + 3) // 4 * 4 for n in (K, ND, N)), "the Philox position is a neutral handle's"
    with pytest.raises(A0Error, match="a0_learner_set_risk.*fixed once the handle has run an update"):
        nat.set_risk("neutral")
    nat.close()


# ------------------------------------------------------------------------------------------------ 4. the actor
E, T = 8, 6


def _actor(logdir, risk, eta, bound=True, groups=0, extra=()):
    import host_slices
    from agent0_amd.common.env_pool import HostEnvGroups
    from agent0_amd.deepq.agent import Actor
    from agent0_amd.deepq.config import parse_overrides
    from agent0_amd.deepq.model import DeepQNet
    from agent0_amd.deepq.replay import ReplayDataset
    cfg = parse_overrides(["learner.algo=iqn", f"actor.num_envs={E}", f"actor.sample_steps={T}", "replay.size=96", "learner.batch_size=8", f"learner.iqn.K={K}",
                           f"learner.iqn.risk={risk}", f"learner.iqn.risk_eta={eta}", "wandb=false", "tb=false", f"logdir={logdir}"] + list(extra))
    cfg.obs_shape, cfg.action_dim = (4, 84, 84), 4
    model = DeepQNet(cfg)
    model.load_state_dict({k: torch.from_numpy(v) for k, v in recipe.make_state_dict(recipe.NetSpec("iqn", 4), 11).items()})
    replay = ReplayDataset(cfg, ops=model.ops) if bound else None
    envs = HostEnvGroups(host_slices.synth_slice(cfg.seed, 0), E, groups=groups, obs_shape=(4, 84, 84), action_dim=4, num_workers=0, ops=model.ops) if groups else None
    return Actor(cfg, model, replay=replay, rank=0, envs=envs)


def _expected_taus(hip, actor, offset, n, kind, eta):
    u, out = hip.empty(n), hip.empty(n)
    hip.rng_uniform(actor.rng.seed, actor.rng.STREAM_TAUS, offset, u, n)
    hip.risk_distort(u, out, n, KINDS[kind], eta)
    torch.cuda.synchronize()
    return out


@pytest.mark.parametrize("kind,eta", [("cvar", 0.25), ("wang", 0.75)], ids=str)
def test_actor_paths_leave_the_distorted_draws_and_agree_on_the_actions(hip, kind, eta, tmp_path):
    """Actor.act through the one-launch path (``_roll_head``) and through the generic chain (the ``rng.uniform`` branch of ``_act_device``: the existing head and
    selection ops on those fractions): the fractions either leaves are a0_risk_distort of the uniform draws at the same offsets, and the greedy actions agree."""
    n = E * K
    a = _actor(tmp_path / "a", kind, eta)
    assert a.one_tail and a.risk_kind == KINDS[kind]
    act_a, q_a = a.act(0.0)
    want = _expected_taus(hip, a, 0, n, kind, eta)
    assert torch.equal(_bits(a.ws.taus[:n]), _bits(want))
    b = _actor(tmp_path / "b", kind, eta)
    b.one_tail = b.quant_slabs = False       # the generic chain, which draws the fractions itself
    act_b, q_b = b.act(0.0)
    assert torch.equal(_bits(b.taus[:n]), _bits(want))
    assert np.array_equal(act_a, act_b) and q_a == pytest.approx(q_b, rel=1e-5)
    neutral = _actor(tmp_path / "n", "neutral", 0.0)
    neutral.act(0.0)
    u = hip.empty(n)
    hip.rng_uniform(a.rng.seed, 3, 0, u, n)
    torch.cuda.synchronize()
    assert torch.equal(_bits(neutral.ws.taus[:n]), _bits(u)) and not torch.equal(want, u)
    assert a.rng.offsets[3] == b.rng.offsets[3] == neutral.rng.offsets[3] == n
    for x in (a, b, neutral):
        x.close()


@pytest.mark.parametrize("mode", ["train-eager", "train-graph", "test", "host-groups"])
def test_rollouts_leave_the_distorted_draws_of_their_last_step(hip, mode, tmp_path):
    kind, eta, n = "pow", -2.0, E * K
    a = _actor(tmp_path / "a", kind, eta, groups=2 if mode == "host-groups" else 0)
    a.use_graph = mode == "train-graph"
    for _ in range(4 if mode == "train-graph" else 2):      # the third rollout is captured, the fourth replayed
        a.sample(0.3, test=mode == "test")
    torch.cuda.synchronize()
    assert (a._graph is not None) is (mode == "train-graph")
    pos = a.rng.offsets[3]
    assert pos == (4 if mode == "train-graph" else 2) * T * n, "the Philox position is a neutral actor's"
    want = _expected_taus(hip, a, pos - n, n, kind, eta)
    if mode == "host-groups":
        for g in a.groups:
            assert torch.equal(_bits(g.ws.taus[: g.E * K]), _bits(want[g.off * K:(g.off + g.E) * K]))
    else:
        assert torch.equal(_bits(a.ws.taus[:n]), _bits(want))
    a.close()


def test_test_rollout_actions_are_the_existing_head_and_selection_ops_on_the_distorted_fractions(hip, tmp_path):
    """Every step of two test rollouts: an actor on the one-launch path (a0_tau_cos_features_risk + the untouched tail kernel) and an actor on the generic chain
    (draw, a0_risk_distort, then the existing head, first-max selection and epsilon-greedy ops on those fractions) act from the same seeds, so equal actions at
    every step give equal frames and returns; one differing action would change the env's next observation and everything behind it."""
    kind, eta, n = "wang", -0.75, E * K
    a, b = _actor(tmp_path / "a", kind, eta), _actor(tmp_path / "b", kind, eta)
    b.one_tail = b.quant_slabs = b.quant_tail = False       # the generic chain, which draws the fractions itself
    outs = {name: [x.sample(0.3, test=True) for _ in range(2)] for name, x in (("a", a), ("b", b))}
    assert a.rng.offsets[3] == b.rng.offsets[3] == 2 * T * n and a.rng.offsets[1] == b.rng.offsets[1]
    for (fa, ra, qa), (fb, rb, qb) in zip(outs["a"], outs["b"]):
        assert len(fa) == len(fb) == T and all(np.array_equal(x, y) for x, y in zip(fa, fb)) and ra == rb
        assert qa == pytest.approx(qb, rel=1e-5)
    assert torch.equal(_bits(b.taus[:n]), _bits(_expected_taus(hip, b, 2 * T * n - n, n, kind, eta)))
    a.close(); b.close()


@pytest.mark.parametrize("mode", ["train-eager", "train-graph", "host-groups"])
def test_training_rollout_actions_are_the_existing_ops_on_the_fractions_it_left(hip, mode, tmp_path):
    """A greedy training rollout (epsilon 0) on the one-launch path — merged with the env step on the device env, eager and replayed from its hipGraph; the tail
    without the env step over a grouped host synthetic env.  The ring's last E rows hold the last step's observations and actions, the workspaces its fractions:
    the existing encoder, head and first-max selection ops on those observations and fractions give those actions."""
    from agent0_amd.deepq.engine import Workspace
    kind, eta, n = "cpw", 0.71, E * K
    rolls = 4 if mode == "train-graph" else 2
    a = _actor(tmp_path / "a", kind, eta, groups=2 if mode == "host-groups" else 0)
    a.use_graph = mode == "train-graph"
    for _ in range(rolls):
        a.sample(0.0)
    torch.cuda.synchronize()
    assert (a._graph is not None) is (mode == "train-graph")
    rows, rp, ops, dev = T * E, a.replay, a.ops, a.model._dev      # nobody extends the replay here: every rollout writes the rows [0, T E)
    taus = torch.cat([g.ws.taus[: g.E * K] for g in a.groups]) if mode == "host-groups" else a.ws.taus[:n].clone()
    assert torch.equal(_bits(taus), _bits(_expected_taus(hip, a, rolls * T * n - n, n, kind, eta)))
    obs = rp.frames[: rows * rp.row_bytes].view(rows, 2, a.obs_bytes)[rows - E:, 0].contiguous().view(-1)
    ws = Workspace(ops, a.L, E, K)
    greedy, qmax = ops.zeros(E, dtype=torch.int32), ops.zeros(E)
    dev.encode(ws, obs, None, a.obs_bytes, 0, E, keep=False)
    dev.head(ws, E, taus.contiguous(), K)
    dev.select(ws, E, K, greedy, qmax=qmax)
    torch.cuda.synchronize()
    assert torch.equal(greedy, rp.act[rows - E:rows]), (greedy.tolist(), rp.act[rows - E:rows].tolist())
    a.close()


def test_actor_handle_leaves_the_distorted_draws_and_its_setter_is_fixed_by_a_rollout(hip, tmp_path, monkeypatch):
    """a0_roll_head: after some iterations under the handles, the fraction buffer of the actor handle holds a0_risk_distort of the uniform draws of its last step
    (its actions are the Python classes': the runs below end on the same ring).  Then the setter is refused."""
    from agent0_amd._abi import A0Error
    from agent0_amd.deepq.native_loop import NativeLoop
    tr = _trainer(tmp_path, monkeypatch, True, "h", "cvar", 0.25)
    iters, Eh, Th = 3, 16, 8
    for _ in range(iters):
        tr.run_iteration()
    assert isinstance(tr._nl, NativeLoop), getattr(tr, "native_loop_reason", None)
    torch.cuda.synchronize()
    n = Eh * K
    got = hip.actor_fractions(tr._nl.actor, n).clone()
    actor = tr.actors[1]
    issued = iters + int(bool(tr._nl._pending_rollout))      # the loop issues the next iteration's rollout ahead and says so
    last = (issued * Th - 1) * n
    want = _expected_taus(hip, actor, last, n, "cvar", 0.25)
    assert torch.equal(_bits(got), _bits(want)), f"the last step of rollout {issued}"
    u = hip.empty(n)
    hip.rng_uniform(actor.rng.seed, 3, last, u, n)
    torch.cuda.synchronize()
    assert not torch.equal(want, u) and not torch.equal(got, u)
    for kind, eta in ((0, 0.0), (1, 0.25), (4, 0.75)):
        with pytest.raises(A0Error, match="a0_actor_set_risk: learner.iqn.risk is fixed once the handle has run a rollout"):
            hip.actor_set_risk(tr._nl.actor, kind, eta)
    _close(tr)


def test_actor_handle_with_a_risk_refuses_a_learner_that_is_not_iqn(hip, tmp_path, monkeypatch):
    """The actor handle learns the algo at the rollout: a0_roll_begin refuses before anything is launched."""
    from agent0_amd._abi import A0Error
    from agent0_amd.deepq.config import parse_overrides
    from agent0_amd.deepq.native_loop import NativeLoop
    from agent0_amd.deepq.trainer import Trainer
    monkeypatch.setenv("A0_NATIVE_LOOP", "1")
    tr = Trainer(parse_overrides(["learner.algo=dqn"] + BASE[1:] + ["seed=42", f"logdir={tmp_path / 'd'}"]))
    nl = tr._native_loop()
    assert isinstance(nl, NativeLoop), getattr(tr, "native_loop_reason", None)
    hip.actor_set_risk(nl.actor, 1, 0.25)
    with pytest.raises(A0Error, match=r"a0_actor_rollout: learner\.iqn\.risk .*iqn learners only"):
        nl._rollout(None)
    hip.actor_set_risk(nl.actor, 0, 0.0)                     # the refused rollout does not count as one
    res = tr.run_iteration()
    assert res is not None and tr.frame_count == 16 * 8
    _close(tr)


# ------------------------------------------------------------------------------------------------ 4 / 5. the Trainer
BASE = ["learner.algo=iqn", f"learner.iqn.K={K}", f"learner.iqn.N={N}", f"learner.iqn.N_dash={ND}", "actor.num_envs=16", "actor.sample_steps=8", "learner.batch_size=32",
        "learner.learner_steps=3", "replay.size=2000", "trainer.training_start_steps=200", "trainer.exploration_steps=512", "actor.min_eps=0.4",
        "learner.target_update_freq=4", "trainer.test_episodes=2", "wandb=false", "tb=false"]
RAINBOW_CFG = ["learner.noisy_net=true", "learner.dueling_head=true", "learner.double_q=true", "learner.n_step_q=3", "replay.policy=prioritize"]


def _trainer(tmp_path, monkeypatch, native, tag, risk, eta, extra=(), seed=42):
    from agent0_amd.deepq.config import parse_overrides
    from agent0_amd.deepq.trainer import Trainer
    monkeypatch.setenv("A0_NATIVE_LOOP", "1" if native else "0")
    return Trainer(parse_overrides(BASE + list(extra) + [f"learner.iqn.risk={risk}", f"learner.iqn.risk_eta={eta}", f"seed={seed}", f"logdir={tmp_path / tag}"]))


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


def _whole_run(tmp_path, monkeypatch, native, risk, eta, extra=(), iters=6):
    from agent0_amd.deepq.native_loop import NativeLoop
    key = (native, risk, eta, tuple(extra))
    if key not in _RUNS:
        tr = _trainer(tmp_path, monkeypatch, native, f"whole-{len(_RUNS)}", risk, eta, extra)
        assert tr.learner.engine.risk_kind == KINDS[risk] and tr.actors[1].risk_kind == KINDS[risk]
        res = [{k: v for k, v in tr.run_iteration().items() if k != "fps"} for _ in range(iters)]
        assert isinstance(tr._nl, NativeLoop) if native else tr._nl is False, getattr(tr, "native_loop_reason", None)
        assert res[-1]["loss"] is not None, "updates ran"
        _RUNS[key] = (_state(tr), res, list(tr.Qs), list(tr.Rs), tr.frame_count, int(tr.learner.rng.offsets.get(3, 0)))
        _close(tr)
    return _RUNS[key]


def _equal(a, b, what):
    for i, (x, y) in enumerate(zip(a[0], b[0])):
        assert torch.equal(_bits(x), _bits(y)), f"{what}: state item {i}"
    assert a[1:5] == b[1:5], what


@pytest.mark.parametrize("extra", [(), tuple(RAINBOW_CFG)], ids=["plain", "rainbow"])
def test_handles_and_python_classes_end_on_the_same_bytes(extra, tmp_path, monkeypatch):
    a, b = _whole_run(tmp_path, monkeypatch, False, "cvar", 0.25, extra), _whole_run(tmp_path, monkeypatch, True, "cvar", 0.25, extra)
    _equal(a, b, "cvar 0.25")
    assert a[0][4][6].item() >= 9 and a[0][4][3].item() == 0, "updates ran, none NaN-skipped"


@pytest.mark.parametrize("native", [True, False], ids=["handles", "python-classes"])
def test_identity_distortions_are_the_neutral_run_and_cvar_is_not(native, tmp_path, monkeypatch):
    """risk=cvar eta=1 and risk=pow eta=0 run the risk launches and end byte-equal to risk=neutral: nothing else moved.  cvar 0.25 differs from the first
    post-warm-up rollout on (its fractions act from the first greedy step; the warm-up's epsilon is 1)."""
    neutral = _whole_run(tmp_path, monkeypatch, native, "neutral", 0.0)
    _equal(_whole_run(tmp_path, monkeypatch, native, "cvar", 1.0), neutral, "cvar 1.0")
    _equal(_whole_run(tmp_path, monkeypatch, native, "pow", 0.0), neutral, "pow 0")
    cvar = _whole_run(tmp_path, monkeypatch, native, "cvar", 0.25)
    assert cvar[5] == neutral[5] and cvar[4] == neutral[4], "the same Philox position and frame count"
    assert not torch.equal(cvar[0][0], neutral[0][0]), "the parameters differ"
    first = next(i for i, (x, y) in enumerate(zip(cvar[1], neutral[1])) if x != y)
    warm = next(i for i, x in enumerate(neutral[1]) if x["loss"] is not None)
    assert first <= warm + 1, (first, warm)


@pytest.mark.parametrize("native", [True, False], ids=["handles", "python-classes"])
def test_a_snapshot_taken_mid_run_resumes_to_the_same_bytes(native, tmp_path, monkeypatch):
    want = _whole_run(tmp_path, monkeypatch, native, "cvar", 0.25)
    tr = _trainer(tmp_path, monkeypatch, native, "b", "cvar", 0.25)
    for _ in range(4):
        tr.run_iteration()
    snap_dir = tr.save_snapshot(str(tmp_path / "snap"))
    _close(tr)
    tr = _trainer(tmp_path, monkeypatch, native, "c", "cvar", 0.25, seed=7)           # another seed: the snapshot's is the run's
    tr.load_snapshot(snap_dir)
    res = [{k: v for k, v in tr.run_iteration().items() if k != "fps"} for _ in range(2)]
    got = _state(tr)
    _close(tr)
    for i, (x, y) in enumerate(zip(got, want[0])):
        assert torch.equal(_bits(x), _bits(y)), f"state item {i}"
    assert res == want[1][4:]


# ------------------------------------------------------------------------------------------------ 6. the refusals
def test_refusals_through_the_constructors_and_both_setters(hip, tmp_path):
    import ctypes as C
    from agent0_amd import _abi
    from agent0_amd._abi import A0Error
    from agent0_amd.deepq.engine import DeviceLearner
    from agent0_amd.deepq.layout import NetLayout
    mk = lambda **kw: hip.native_learner(A=ACTIONS, dueling=False, double_q=False, B=BATCH, discount=0.99, lr=5e-4, target_update_freq=2, algo=kw.pop("algo", "iqn"),
                                         seed=SEED, K=K, N=N, N_dash=ND, **kw)
    nat = mk()
    for kind, eta, word in (("cvar", 0.0, r"risk_eta = 0 .*0\.25"), ("cvar", 2.0, "risk_eta = 2"), ("cpw", 0.0, r"0\.71"), ("pow", 100.0, "risk_eta = 100"),
                            ("wang", float("nan"), "risk_eta = nan"), (7, 0.5, r"learner\.iqn\.risk = 7")):
        with pytest.raises(A0Error, match="a0_learner_set_risk: .*" + word):
            nat.set_risk(kind, eta)
    nat.set_risk("cvar", 0.25)
    with pytest.raises(A0Error, match="a0_learner_set_munchausen.*learner.iqn.risk"):
        nat.set_munchausen(True)
    nat.set_risk("neutral", float("nan"))                      # neutral ignores eta
    nat.set_munchausen(True)
    with pytest.raises(A0Error, match="a0_learner_set_risk.*learner.iqn.munchausen"):
        nat.set_risk("wang", 0.75)
    nat.close()
    for algo, code in (("fqf", 3), ("dqn", 0)):
        nat = mk(algo=algo, **(dict(F=8) if algo == "fqf" else {}))
        with pytest.raises(A0Error, match=f"a0_learner_set_risk.*iqn handles only.*algo is {code}"):
            nat.set_risk("cvar", 0.25)
        nat.set_risk("neutral")
        nat.close()
    L = NetLayout.from_spec(_spec())
    with pytest.raises(ValueError, match=r"learner\.iqn\.risk=cvar.*learner\.iqn\.munchausen"):
        DeviceLearner(hip, L, BATCH, K=K, N=N, N_dash=ND, munchausen=True, risk="cvar", risk_eta=0.25)
    for algo in ("fqf", "dqn"):
        with pytest.raises(ValueError, match=rf"learner\.iqn\.risk=wang.*learner\.algo={algo}"):
            DeviceLearner(hip, NetLayout.from_spec(recipe.NetSpec(algo, ACTIONS, obs_shape=SHAPE)), BATCH, risk="wang", risk_eta=0.75)
    with pytest.raises(ValueError, match=r"learner\.iqn\.risk='norm'"):
        DeviceLearner(hip, L, BATCH, K=K, N=N, N_dash=ND, risk="norm")
    with pytest.raises(ValueError, match=r"learner\.iqn\.risk=cvar: learner\.iqn\.risk_eta=0\.0.*0\.25"):
        _actor(tmp_path / "x", "cvar", 0.0)
    with pytest.raises(ValueError, match=r"learner\.iqn\.risk=cpw.*learner\.iqn\.munchausen"):
        _actor(tmp_path / "y", "cpw", 0.71, extra=["learner.iqn.munchausen=true"])
    dev = _eager(hip, "cvar", 0.25)[1]
    with pytest.raises(ValueError, match=r"learner\.iqn\.risk.*fixed once the learner has run an update"):
        dev.set_risk("neutral")
    # the actor handle: its setter's own checks (after a rollout, and the rollout's refusal of another algo: the two tests of the handle above)
    ad = _abi_actor_desc()
    actor = C.c_void_p()
    _abi.check(hip.lib.a0_actor_create(C.addressof(ad), C.addressof(actor)), "a0_actor_create")
    for kind, eta, word in ((1, 0.0, r"risk_eta = 0 .*0\.25"), (3, 1.5, r"risk_eta = 1\.5"), (4, 9.0, "risk_eta = 9"), (9, 0.5, r"learner\.iqn\.risk = 9")):
        with pytest.raises(A0Error, match="a0_actor_set_risk: .*" + word):
            hip.actor_set_risk(actor, kind, eta)
    hip.actor_set_risk(actor, 1, 0.25)
    hip.actor_set_risk(actor, 0, float("nan"))
    _abi.check(hip.lib.a0_actor_destroy(actor), "a0_actor_destroy")


def _abi_actor_desc():
    from agent0_amd.deepq.native_loop import _ActorDesc
    return _ActorDesc(E, T, 4, 0, 1, 0.99, 42, 0, 0, 4)
