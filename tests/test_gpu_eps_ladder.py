"""GPU (MI355X): ``actor.eps_ladder`` — one epsilon per environment, eps_i = eps^(1 + alpha i / (N - 1)).

1. a0_eps_ladder against the float64 restatement (tests/eps_ladder_ref.py) rounded to fp32: within 1 ulp (double pow is good to a few double ulps, so the two can
   only part at an fp32 rounding boundary), bit-exact on the three edges, a slice equal to the whole's slice.
2. Every action-selection kernel reads its own env's epsilon under A0_EPS_PER_ENV: actions against the oracle's Philox draws compared with the VECTOR
   (actor_tail_cases.egreedy_expected broadcasts), at offsets where a kernel that read entry 0 for everyone would give other ACTIONS (asserted per case).
3. Rollouts byte for byte against the oracle's actor, which takes the vector read back from the device, on four hosts: the eager Python classes, the captured
   rollout (a replay with a new epsilon), the library's actor handle, and that handle in a one-rank data-parallel group (RCCL exchange installed).
4. Host envs: groups and the pool attached to the actor handle give the bytes of the one-group Python rollout.
5. Trainer: the library's handles and the Python classes end on the same state on the main and the launch schedule and in a one-rank data-parallel group; a ladder
   run is the plain run while the scheduled epsilon is >= 1 and another one afterwards; a snapshot resumes bit for bit; test rollouts do not change."""
import ctypes as C
import os

import numpy as np
import pytest
import torch

import actor_tail_cases as TC
import eps_ladder_ref as ref
import recipe

pytestmark = pytest.mark.gpu

EPS_PER_ENV = -1.0


@pytest.fixture(scope="module")
def hip():
    from agent0_amd.ops import HipOps
    ops = HipOps()
    assert "gfx950" in ops.device_info()[2] and ops.__class__.__module__ == "agent0_amd.ops"
    from agent0_amd import ops as opsmod
    assert opsmod.EPS_PER_ENV == EPS_PER_ENV
    return ops


def _dev(hip, a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(hip.device)


# ------------------------------------------------------------------------------------------------ 1. the ladder kernel
LADDER_EPS = (0.0, 1e-3, 0.01, 0.4, 1 - 2.0 ** -24, 1.0, 1.01)
GUARD = 64


def _ladder(hip, eps, alpha, E, i0, n_total, through_ptr):
    out = hip.empty(E + GUARD)
    out.fill_(-7.0)
    if through_ptr:
        hip.eps_ladder(0.123, _dev(hip, np.array([eps], np.float32)), alpha, E, i0, n_total, out)       # the scalar argument is ignored
    else:
        hip.eps_ladder(eps, None, alpha, E, i0, n_total, out)
    torch.cuda.synchronize()
    got = out.cpu().numpy()
    assert (got[E:] == -7.0).all(), "write past the end"
    return got[:E]


@pytest.mark.parametrize("through_ptr", [False, True], ids=["scalar", "eps_ptr"])
@pytest.mark.parametrize("E", [1, 2, 5, 64, 65, 256, 300])
def test_ladder_kernel_against_float64(hip, E, through_ptr):
    worst = 0
    for alpha in (0.5, 7.0):
        for eps in LADDER_EPS:
            got = _ladder(hip, eps, alpha, E, 0, E, through_ptr)
            want = ref.ladder32(eps, alpha, 0, E, E)
            d = int(ref.ulp_distance(got, want).max())
            worst = max(worst, d)
            print(f"E={E} alpha={alpha} eps={eps!r}: worst distance {d} ulp")
            assert d <= 1, f"E={E} alpha={alpha} eps={eps}: {d} ulp from the float64 ladder"
            e32 = np.float32(eps)
            assert got[0].view(np.int32) == (e32 if eps > 0 else np.float32(0)).view(np.int32), "env 0 keeps eps, bit for bit"
            if eps >= 1:
                assert np.array_equal(got.view(np.int32), np.full(E, e32).view(np.int32)), "eps >= 1 stays eps, bit for bit"
            if eps <= 0:
                assert np.array_equal(got.view(np.int32), np.zeros(E, np.int32)), "eps <= 0 gives 0"
            assert (np.diff(got) <= 0).all()
    print("worst", worst)


@pytest.mark.parametrize("through_ptr", [False, True], ids=["scalar", "eps_ptr"])
def test_ladder_slice_is_the_slice_of_the_whole(hip, through_ptr):
    for alpha in (0.5, 7.0):
        for eps in (1e-3, 0.4, 1 - 2.0 ** -24, -0.5, 1.3):
            whole = _ladder(hip, eps, alpha, 300, 0, 300, through_ptr)
            part = _ladder(hip, eps, alpha, 5, 3, 300, through_ptr)
            assert np.array_equal(part.view(np.int32), whole[3:8].view(np.int32))


def test_ladder_refuses_bad_arguments(hip):
    from agent0_amd._abi import A0Error
    out = hip.empty(8)
    for args in ((0.4, None, 0.0, 8, 0, 8), (0.4, None, 7.0, 8, 1, 8), (0.4, None, 7.0, 8, -1, 8), (0.4, None, -1.0, 8, 0, 8)):
        with pytest.raises(A0Error):
            hip.eps_ladder(*args, out)


# ------------------------------------------------------------------------------------------------ 2. the tails read their own epsilon
EPS_MIX = np.array([0.35, 0.0, 1.0, 0.7, 0.15, 0.55, 0.9, 0.25, 0.45], np.float32)       # env 0 fractional; zeros, ones and fractions behind it


def _eps_vector(E):
    return np.array([0.4], np.float32) if E == 1 else EPS_MIX[:E].copy()


def _offsets(E, vec, A, greedy):
    """(off_a, off_u) at which the oracle's draws alone, compared with the VECTOR, send fractional envs down both branches and give at least one env e > 0 another
    ACTION than entry 0 would: its mask differs ((u_e > eps_e) != (u_e > eps_0)) and its random action is not its greedy one (``greedy``: the launch with eps = 0,
    which no offset changes).  A kernel that reads eps_ptr[0] for everyone fails there."""
    from oracle import core
    frac = (vec > 0) & (vec < 1)
    greedy = np.asarray(greedy, np.int64)
    for k in range(4096):
        off_a, off_u = 40 + 3 * k, 44 + 5 * k
        if E == 1:
            return off_a, off_u
        u = core.rng_uniform(TC.RNG_SEED, TC.STREAM_U, off_u, E)
        ra = (core.rng_u32(TC.RNG_SEED, TC.STREAM_A, off_a, E) % np.uint32(A)).astype(np.int64)
        keep = u > vec
        told = (keep != (u > vec[0])) & (ra != greedy)
        if keep[frac].any() and not keep[frac].all() and told[1:].any():
            return off_a, off_u
    raise AssertionError("no offsets found")


def _ctrl(hip, da, du):
    ctrl = hip.zeros(8, dtype=torch.int64)
    ctrl[2], ctrl[3] = da, du
    return ctrl


def _out(hip, E):
    act, q = hip.empty(E + GUARD, dtype=torch.int32), hip.empty(E + GUARD)
    act.fill_(-1); q.fill_(float("nan"))
    act[E:].fill_(0x5A5A5A5A); q[E:].fill_(-1.25e38)
    return act, q


def _get(act, q, E):
    torch.cuda.synchronize()
    assert bool((act[E:] == 0x5A5A5A5A).all()) and bool((q[E:] == -1.25e38).all()), "write past the end"
    return act[:E].cpu().numpy(), q[:E].cpu().numpy()


def _judge_per_env(hip, forms, E, A, what):
    """``forms``: name -> launch(eps, off_a, off_u, ctrl, eps_ptr, action, qmax)."""
    vec = _eps_vector(E)
    vec_dev = _dev(hip, vec)
    for name, launch in forms.items():
        act, q = _out(hip, E)
        launch(0.0, 40, 44, None, None, act, q)                    # the greedy action and max-Q: the same launch with the scalar eps = 0, whatever the offsets
        a_g, q_g = _get(act, q, E)
        off_a, off_u = _offsets(E, vec, A, a_g)
        want, keep = TC.egreedy_expected(TC.RNG_SEED, TC.STREAM_A, TC.STREAM_U, off_a, off_u, vec, A, a_g)
        want0, _ = TC.egreedy_expected(TC.RNG_SEED, TC.STREAM_A, TC.STREAM_U, off_a, off_u, vec[0], A, a_g)      # what reading entry 0 for every env gives
        if E > 1:
            assert set(keep[(vec > 0) & (vec < 1)].tolist()) == {False, True}
            assert not np.array_equal(want[1:], want0[1:]), "the offsets tell a kernel that reads entry 0 from one that reads its own"
        for through_ctrl in (False, True):
            act, q = _out(hip, E)
            if through_ctrl:
                launch(EPS_PER_ENV, off_a - 8, off_u - 20, _ctrl(hip, 8, 20), vec_dev, act, q)
            else:
                launch(EPS_PER_ENV, off_a, off_u, None, vec_dev, act, q)
            a_e, q_e = _get(act, q, E)
            assert np.array_equal(a_e, want), f"{what} {name} (ctrl={through_ctrl}): {a_e} vs the oracle's draws against the vector {want}"
            assert np.array_equal(q_e.view(np.int32), q_g.view(np.int32)), f"{what} {name}: max-Q is that of the scalar launch"
        # any other scalar beside a pointer keeps reading entry 0 (a captured rollout's device scalar)
        act, q = _out(hip, E)
        launch(0.9, off_a, off_u, None, vec_dev, act, q)
        a_0, _ = _get(act, q, E)
        assert np.array_equal(a_0, want0), f"{what} {name}: without the sentinel eps_ptr[0] holds for every env"
    return vec, vec_dev, off_a, off_u


_NET = {}


def _enc(hip):
    if not _NET:
        from agent0_amd.deepq.engine import DeviceNet
        from agent0_amd.deepq.layout import NetLayout
        spec = recipe.NetSpec("dqn", 4, obs_shape=(4, 84, 84))
        net = DeviceNet(hip, NetLayout.from_spec(spec), hip.net(4, 84, 84))
        net.load_state_dict(recipe.make_state_dict(spec, 11))
        _NET["net"] = net
    return _NET["net"]


def _throwaway_env(hip, E):
    z = lambda n, dt=torch.float32: hip.zeros(n, dtype=dt)
    obs_in = _dev(hip, recipe.gen(77).integers(0, 256, E * 4 * 84 * 84, dtype=np.uint8))
    return (4321, 0, 1, obs_in, z(E * 4 * 84 * 84, torch.uint8), z(E), z(E), z(E), 1, 0, 0.99, z(E, torch.int32), z(E), z(E), obs_in,
            z(E * 8 * 84 * 84, torch.uint8), E, 0, z(E, torch.int32), z(E), z(E))


@pytest.mark.parametrize("E", [1, 5, 9])
@pytest.mark.parametrize("A,dueling", [(4, False), (18, True)])
def test_scalar_head_forms_read_their_own_epsilon(hip, A, dueling, E):
    K = TC.QHEAD_ENV_K
    r = TC.qhead_reference(E, K, A, dueling)
    feat, W1, b1, W2, b2 = (_dev(hip, r[k].reshape(-1)) for k in ("feat", "W1", "b1", "W2", "b2"))
    ns = TC.fc1_splits(E, K)
    need = hip.actor_qhead_scratch(E, K)
    env, net = _throwaway_env(hip, E), _enc(hip)
    enc = dict(task=0, wt=net.wt, enc_w=net.encoder_weights(), act3_next=hip.empty(E * K))

    def form(k):
        def launch(eps, off_a, off_u, ctrl, eps_ptr, act, q):
            args = (feat, E, K, W1, b1, W2, b2, A, dueling, hip.empty(need), TC.RNG_SEED, TC.STREAM_A, TC.STREAM_U, off_a, off_u, eps, act, q, ctrl, eps_ptr)
            (hip.actor_qhead, hip.actor_qhead_env_step, hip.actor_qhead_env_step_enc)[k](*args, *((), env, env)[k], **({}, {}, enc)[k])
        return launch

    names = ("actor_qhead", "actor_qhead_env_step", "actor_qhead_env_step_enc")
    vec, vec_dev, off_a, off_u = _judge_per_env(hip, {n: form(k) for k, n in enumerate(names)}, E, A, f"qhead A={A} duel={dueling} E={E}")
    if E > 2:      # a group's launch: envs 2.. with the vector's slice, the batch's split count and the envs' own draws
        act, q = _out(hip, E)
        form(0)(EPS_PER_ENV, off_a, off_u, None, vec_dev, act, q)
        a_w, q_w = _get(act, q, E)
        k = E - 2
        act, q = _out(hip, k)
        hip.actor_qhead_n(feat[2 * K:], k, K, ns, W1, b1, W2, b2, A, dueling, hip.empty(ns * k * 512), TC.RNG_SEED, TC.STREAM_A, TC.STREAM_U, off_a + 2, off_u + 2, EPS_PER_ENV,
                          act, q, None, vec_dev[2:])
        a_p, q_p = _get(act, q, k)
        assert np.array_equal(a_p, a_w[2:]) and np.array_equal(q_p.view(np.int32), q_w[2:].view(np.int32))


def _tail_forms(hip, case, kt, slabs_np, bias_np, aux_np, E):
    A, T, dueling, mode, ld, nslab = case[:6]
    slabs, bias = _dev(hip, slabs_np.reshape(-1)), _dev(hip, bias_np)
    aux = None if aux_np is None else _dev(hip, aux_np.reshape(-1))
    env, net = _throwaway_env(hip, E), _enc(hip)
    enc = dict(task=0, wt=net.wt, enc_w=net.encoder_weights(), act3_next=hip.empty(E * 3136))
    fn = (("actor_dist_tail", "actor_dist_tail_env_step", "actor_dist_tail_env_step_enc"),
          ("actor_quantile_tail", "actor_quantile_tail_env_step", "actor_quantile_tail_env_step_enc"))[kt]

    def form(k):
        def launch(eps, off_a, off_u, ctrl, eps_ptr, act, q):
            args = (slabs, nslab, bias, ld, A, T, dueling, mode, aux, E, TC.RNG_SEED, TC.STREAM_A, TC.STREAM_U, off_a, off_u, eps, act, q, ctrl, eps_ptr)
            getattr(hip, fn[k])(*args, *((), env, env)[k], **({}, {}, enc)[k])
        return launch
    return {fn[k]: form(k) for k in range(3)}


@pytest.mark.parametrize("kt,idx", [(0, 0), (0, 1), (0, 4), (1, 0), (1, 1)], ids=["dist0", "dist1", "dist4", "quantile0", "quantile1"])
def test_distributional_and_quantile_forms_read_their_own_epsilon(hip, kt, idx):
    case = (TC.DIST_CASES, TC.QUANTILE_CASES)[kt][idx]
    A, T, dueling, mode, ld, nslab, E = case[:7]
    r = TC.tail_reference(case, kt)
    forms = _tail_forms(hip, case, kt, r["slabs"], r["bias"], r["aux"], E)
    vec, vec_dev, off_a, off_u = _judge_per_env(hip, forms, E, A, ("dist ", "quantile ")[kt] + TC.case_id(case))
    if E > 2:
        first = next(iter(forms))
        act, q = _out(hip, E)
        forms[first](EPS_PER_ENV, off_a, off_u, None, vec_dev, act, q)
        a_w, q_w = _get(act, q, E)
        k, rows = E - 2, (T if kt else 1)
        sub = np.ascontiguousarray(r["slabs"][:, 2 * rows:])
        aux = r["aux"][2:] if mode == 3 else r["aux"]
        part = _tail_forms(hip, case, kt, sub, r["bias"], aux, k)[first]
        act, q = _out(hip, k)
        part(EPS_PER_ENV, off_a + 2, off_u + 2, None, vec_dev[2:], act, q)
        a_p, q_p = _get(act, q, k)
        assert np.array_equal(a_p, a_w[2:]) and np.array_equal(q_p.view(np.int32), q_w[2:].view(np.int32))


@pytest.mark.parametrize("E", [1, 5, 300])
def test_egreedy_rng_reads_its_own_epsilon(hip, E):
    """As for the tails: offsets searched over all E envs at which reading entry 0 gives other actions, plain and through ``ctrl``, and entry 0 for every env
    beside any other scalar."""
    A = 6
    vec = np.resize(EPS_MIX, E).astype(np.float32) if E > 1 else _eps_vector(1)
    vec_dev = _dev(hip, vec)
    greedy = (np.arange(E) % A).astype(np.int32)
    greedy_dev = _dev(hip, greedy)
    off_a, off_u = _offsets(E, vec, A, greedy)
    want, _ = TC.egreedy_expected(TC.RNG_SEED, TC.STREAM_A, TC.STREAM_U, off_a, off_u, vec, A, greedy)
    want0, _ = TC.egreedy_expected(TC.RNG_SEED, TC.STREAM_A, TC.STREAM_U, off_a, off_u, vec[0], A, greedy)
    if E > 1:
        assert not np.array_equal(want[1:], want0[1:]), "the offsets tell a kernel that reads entry 0 from one that reads its own"

    def launch(eps, da, du, ctrl):
        act, _ = _out(hip, E)
        hip.actor_egreedy_rng(greedy_dev, TC.RNG_SEED, TC.STREAM_A, TC.STREAM_U, off_a - da, off_u - du, A, eps, E, act, None, None, ctrl, vec_dev)
        torch.cuda.synchronize()
        assert bool((act[E:] == 0x5A5A5A5A).all()), "write past the end"
        return act[:E].cpu().numpy()

    assert np.array_equal(launch(EPS_PER_ENV, 0, 0, None), want)
    assert np.array_equal(launch(EPS_PER_ENV, 8, 20, _ctrl(hip, 8, 20)), want), "through ctrl offsets"
    assert np.array_equal(launch(0.9, 0, 0, None), want0), "without the sentinel eps_ptr[0] holds for every env"


# ------------------------------------------------------------------------------------------------ 3. rollouts against the oracle
def make_cfg(algo, E, logdir, **kw):
    from agent0_amd.deepq.config import parse_overrides
    cfg = parse_overrides([f"learner.algo={algo}", f"actor.num_envs={E}", "wandb=false", "tb=false", f"logdir={logdir}"] + [f"{k}={v}" for k, v in kw.items()])
    cfg.obs_shape = (4, 84, 84)
    cfg.action_dim = 4
    return cfg


def _noise_list(L, buf):
    """A noise buffer in the device's layout as the oracle takes it (tests/test_gpu_trace.py)."""
    out, off = [], 0
    for prefix, block, r0, r1, in_f in L.noise_modules:
        for leaf, n in (("noise_in", in_f), ("noise_out_weight", r1 - r0), ("noise_out_bias", r1 - r0)):
            v = buf[off:off + n]
            out.append((L.noise_in_from_kernel(prefix, v) if leaf == "noise_in" else v).clone().cpu().numpy())
            off += (n + 3) // 4 * 4
    return out


ROLLOUT_SPECS = {"dqn": recipe.SPECS["dqn"], "c51": recipe.SPECS["c51_duel_noisy"], "iqn": recipe.SPECS["iqn_duel"]}
ALPHA = 7.0


ROLLOUT_EPS = (0.35, 0.6, 0.2, 0.8, 0.05)              # a new epsilon every rollout


def _oracle_actor(cfg, spec, model, E, T, n_step):
    """The oracle's actor over the oracle's env, fed the device's random numbers as tests/test_gpu_trainer.py::test_actor_rollout_matches_oracle feeds them: Philox
    draws at the offsets the device reserves, NoisyNet noise in the device's layout."""
    from agent0_amd.common.utils import DeviceRng
    from oracle import actor as oactor
    from oracle import core, learner as olearner, nets
    seed64 = cfg.seed & 0xFFFFFFFF
    calls = {"draw": 0, "tau": 0, "noise": 0}
    K = int(cfg.learner.iqn.K)

    def draw(E_):
        off = calls["draw"] * ((E_ + 3) // 4) * 4
        calls["draw"] += 1
        return (core.rng_u32(seed64, DeviceRng.STREAM_EGREEDY_A, off, E_) % 4).astype(np.int64), core.rng_uniform(seed64, DeviceRng.STREAM_EGREEDY_U, off, E_)

    def taus_fn(E_):
        n = E_ * K
        off = calls["tau"] * ((n + 3) // 4) * 4
        calls["tau"] += 1
        return torch.from_numpy(core.rng_uniform(seed64, DeviceRng.STREAM_TAUS, off, n).reshape(E_, K, 1))

    def noisy_reset(p):
        n = model._dev.noise_len
        buf = torch.from_numpy(core.rng_normal(seed64, DeviceRng.STREAM_NOISE, calls["noise"] * ((n + 3) // 4) * 4, 0.1, n))
        calls["noise"] += 1
        it = iter(_noise_list(model.L, buf))
        with torch.no_grad():
            for prefix in nets.dense_prefixes(spec):
                for leaf in ("noise_in", "noise_out_weight", "noise_out_bias"):
                    p[f"{prefix}.{leaf}"] = torch.from_numpy(np.array(next(it), dtype=np.float32))
                nets.compose_noise(p, prefix)

    env = core.SynthVecEnv(E, seed=cfg.seed, rank=0, action_dim=4, task="stream")
    return oactor.OracleActor(env, olearner.to_params(recipe.make_state_dict(spec, 11)), spec, n_step=n_step, sample_steps=T, draw=draw,
                              taus_fn=taus_fn if spec.algo == "iqn" else None, noisy_reset=noisy_reset if spec.noisy else None, reset_noise_freq=3)


def _assert_rollout_is_the_oracles(replay, call, odata, rs, ors, qs, oqs):
    """Rollout ``call``'s ring rows, actions, n-step rewards and dones are the oracle's, byte for byte; so are the episode returns; max-Q to float tolerance."""
    assert [float(x) for x in rs] == [float(x) for x in ors]
    assert np.allclose(qs, oqs, rtol=5e-5, atol=5e-6), "mean max-Q per step"
    n = len(odata)
    base = call * n
    rows = replay.frames.view(replay.size, -1)[base:base + n].cpu().numpy()
    act, rew, done = replay.act[base:base + n].cpu().numpy(), replay.rew[base:base + n].cpu().numpy(), replay.done[base:base + n].cpu().numpy()
    for i, (fr, at, rt, dt) in enumerate(odata):
        assert np.array_equal(rows[i], fr.reshape(-1)), f"transition {base + i}: packed st||st_next bytes"
        assert int(act[i]) == int(at) and float(rew[i]) == np.float32(rt) and bool(done[i] != 0) == bool(dt), f"transition {base + i}"


def _rollout_overrides(spec, n_step, T):
    return {"learner.n_step_q": n_step, "actor.sample_steps": T, "replay.size": 400, "learner.batch_size": 8, "actor.eps_ladder": ALPHA,
            "learner.dueling_head": str(bool(spec.dueling)).lower(), "learner.noisy_net": str(bool(spec.noisy)).lower(), "learner.reset_noise_freq": 3}


@pytest.mark.parametrize("graphed", [False, True], ids=["eager", "graphed"])
@pytest.mark.parametrize("n_step", [1, 3])
@pytest.mark.parametrize("name", sorted(ROLLOUT_SPECS))
def test_rollouts_match_the_oracle_acting_with_the_vector(name, n_step, graphed, tmp_path):
    """The set-up of tests/test_gpu_trainer.py::test_actor_rollout_matches_oracle with E = 8 and the ladder on; the oracle's Actor.sample takes the vector read back
    from the device, a new epsilon every call.  Graphed: calls 0-1 run eagerly, call 2 captures (the ladder launch inside the graph, reading eps_dev), 3-4 replay."""
    from agent0_amd.deepq.agent import Actor
    from agent0_amd.deepq.model import DeepQNet
    from agent0_amd.deepq.replay import ReplayDataset
    E, T = 8, 6
    spec = ROLLOUT_SPECS[name]
    cfg = make_cfg(spec.algo, E, tmp_path, **_rollout_overrides(spec, n_step, T))
    model = DeepQNet(cfg)
    model.load_state_dict({k: torch.from_numpy(v) for k, v in recipe.make_state_dict(spec, 11).items()})
    replay = ReplayDataset(cfg, ops=model.ops)
    actor = Actor(cfg, model, replay=replay, rank=0)
    actor.use_graph = graphed
    ora = _oracle_actor(cfg, spec, model, E, T, n_step)
    for call, eps in enumerate(ROLLOUT_EPS):
        data, rs, qs = actor.sample(float(eps))
        replay.extend(data)
        vec = actor.eps_vec.cpu().numpy()
        assert int(ref.ulp_distance(vec, ref.ladder32(eps, ALPHA, 0, E, E)).max()) <= 1
        assert vec[0] == np.float32(eps) and vec[-1] < vec[0]
        odata, ors, oqs = ora.sample(vec)
        _assert_rollout_is_the_oracles(replay, call, odata, rs, ors, qs, oqs)
    assert (actor._graph is not None) == graphed, "the rollout should have been captured"
    actor.close()


def _one_rank_group(monkeypatch):
    """A one-rank RCCL group (A0_DP_FORCE=1); the caller destroys it."""
    import socket
    from agent0_amd.deepq.dist import init_process_group
    with socket.socket() as sk:
        sk.bind(("127.0.0.1", 0))
        port = str(sk.getsockname()[1])
    for k, v in (("A0_DP_FORCE", "1"), ("RANK", "0"), ("LOCAL_RANK", "0"), ("WORLD_SIZE", "1"), ("MASTER_ADDR", "127.0.0.1"), ("MASTER_PORT", port)):
        monkeypatch.setenv(k, v)
    init_process_group()


def _install_exchange(tr):
    """What bench.py and launch.py do for a data-parallel job: the RCCL gradient exchange on the learner's engine."""
    from agent0_amd.deepq.dist import make_grad_hook
    eng = tr.learner.engine
    hook = eng.grad_hook = make_grad_hook(tr.ops, eng.L.n_adam)
    assert type(hook).__name__ == "RcclGradAllReduce" and hook.active
    return hook


def _close_exchange(tr, hook):
    if getattr(tr, "_nl", None):
        tr._nl.detach_exchange()
    _close(tr)
    hook.close()


@pytest.mark.parametrize("dp", [False, True], ids=["handle", "handle-dp"])
@pytest.mark.parametrize("n_step", [1, 3])
@pytest.mark.parametrize("name", sorted(ROLLOUT_SPECS))
def test_handle_rollouts_match_the_oracle_acting_with_the_vector(name, n_step, dp, tmp_path, monkeypatch):
    """The same comparison for the library's actor handle (a0_actor_set_eps_ladder + a0_actor_rollout), alone and in a one-rank data-parallel group: a Trainer on the
    native loop whose ring never reaches training_start_steps, so that nothing but rollouts runs and the weights stay the recipe's.  The handle keeps its vector to
    itself; the oracle takes what a0_eps_ladder gives on the device for the same (epsilon, alpha, i0 = 0, n_total = E) — a handle that filled its vector with
    another span, or whose tails did not read it, would part from the oracle's bytes."""
    import torch.distributed as dist
    from agent0_amd.deepq.config import parse_overrides
    from agent0_amd.deepq.native_loop import NativeLoop
    from agent0_amd.deepq.trainer import Trainer
    E, T = 8, 6
    spec = ROLLOUT_SPECS[name]
    monkeypatch.setenv("A0_NATIVE_LOOP", "1")
    if dp:
        _one_rank_group(monkeypatch)
    try:
        over = dict(_rollout_overrides(spec, n_step, T), **{"trainer.training_start_steps": 390, "learner.learner_steps": 1, "trainer.test_episodes": 2})
        cfg = parse_overrides([f"learner.algo={spec.algo}", f"actor.num_envs={E}", "wandb=false", "tb=false", f"logdir={tmp_path}"] + [f"{k}={v}" for k, v in over.items()])
        tr = Trainer(cfg)
        tr.learner.model.load_state_dict({k: torch.from_numpy(v) for k, v in recipe.make_state_dict(spec, 11).items()})
        tr.learner.engine.sync_target(force=True)
        hook = _install_exchange(tr) if dp else None
        assert tuple(cfg.obs_shape) == (4, 84, 84) and cfg.action_dim == 4
        tr.epsilon_fn = lambda frames: ROLLOUT_EPS[min(frames // (E * T), len(ROLLOUT_EPS) - 1)]
        ora = _oracle_actor(cfg, spec, tr.learner.model, E, T, n_step)
        vec_dev = tr.ops.zeros(E)
        for call, eps in enumerate(ROLLOUT_EPS):
            nq, nr = len(tr.Qs), len(tr.Rs)
            out = tr.run_iteration()
            assert isinstance(tr._nl, NativeLoop), getattr(tr, "native_loop_reason", None)
            assert out["loss"] is None, "no update ran"
            tr.ops.eps_ladder(eps, None, ALPHA, E, 0, E, vec_dev)
            vec = vec_dev.cpu().numpy()
            assert vec[0] == np.float32(eps) and vec[-1] < vec[0]
            odata, ors, oqs = ora.sample(vec)
            _assert_rollout_is_the_oracles(tr.replay, call, odata, list(tr.Rs)[nr:], ors, list(tr.Qs)[nq:], oqs)
        _close_exchange(tr, hook) if dp else _close(tr)
    finally:
        if dp:
            dist.destroy_process_group()


# ------------------------------------------------------------------------------------------------ 4. grouped and host envs
def _host_rollouts(logdir, algo, E, groups, workers, n_step, T, rollouts, ladder=ALPHA):
    import host_slices
    from agent0_amd.common.env_pool import HostEnvGroups, HostEnvPool
    from agent0_amd.deepq.agent import Actor
    from agent0_amd.deepq.model import DeepQNet
    from agent0_amd.deepq.replay import ReplayDataset
    spec = recipe.NetSpec(algo, 4, num_atoms=51)
    cfg = make_cfg(algo, E, logdir, **{"learner.n_step_q": n_step, "actor.sample_steps": T, "replay.size": 300, "learner.batch_size": 8, "actor.eps_ladder": ladder})
    model = DeepQNet(cfg)
    model.load_state_dict({k: torch.from_numpy(v) for k, v in recipe.make_state_dict(spec, 11).items()})
    replay = ReplayDataset(cfg, ops=model.ops)
    kw = dict(obs_shape=(4, 84, 84), action_dim=4, num_workers=workers, ops=model.ops)
    envs = (HostEnvGroups(host_slices.synth_slice(cfg.seed, 0), E, groups=groups, **kw) if groups > 1 else HostEnvPool(host_slices.synth_slice(cfg.seed, 0), E, **kw))
    actor = Actor(cfg, model, replay=replay, rank=0, envs=envs)
    try:
        assert (actor.groups is not None) == (groups > 1)
        rs_all, qs_all = [], []
        for eps in (0.3, 0.7, 0.1, 0.5)[:rollouts]:
            data, rs, qs = actor.sample(eps)
            replay.extend(data)
            rs_all += rs
            qs_all += qs
        n = rollouts * T * E
        return (replay.frames[: n * replay.row_bytes].clone(), replay.act[:n].clone(), replay.rew[:n].clone(), replay.done[:n].clone(), rs_all, qs_all)
    finally:
        actor.close()


@pytest.mark.parametrize("algo,n_step,workers", [("dqn", 1, 0), ("c51", 3, 2), ("iqn", 1, 2), ("dqn", 3, 2)])
def test_two_groups_give_the_bytes_of_one_group(algo, n_step, workers, tmp_path):
    """A group's launch reads its envs' part of the vector: index in the whole vector env, not in the group."""
    one = _host_rollouts(tmp_path / "one", algo, 8, 1, workers, n_step, 6, 4)
    two = _host_rollouts(tmp_path / "two", algo, 8, 2, workers, n_step, 6, 4)
    plain = _host_rollouts(tmp_path / "off", algo, 8, 1, workers, n_step, 6, 4, ladder=0.0)
    for x, y in zip(one[:4], two[:4]):
        assert torch.equal(x, y)
    assert one[4] == two[4] and one[5] == two[5]
    assert not torch.equal(one[1], plain[1]), "the ladder changes the actions"


# ------------------------------------------------------------------------------------------------ 5. Trainer
E5, T5 = 16, 8
# eps(frames) = 1 - frames / 512 + 0.4: 1.4 and 1.15 for the first two rollouts (frames 0, 128), 0.9 at frames 256, then falling to 0.4
BASE5 = [f"actor.num_envs={E5}", f"actor.sample_steps={T5}", "learner.batch_size=32", "learner.learner_steps=3", "replay.size=2000", "trainer.training_start_steps=200",
         "trainer.exploration_steps=512", "actor.min_eps=0.4", "learner.target_update_freq=4", "trainer.test_episodes=2", "wandb=false", "tb=false"]


def _trainer(tmp_path, monkeypatch, native, algo, extra, use_lp, tag, ladder=ALPHA, seed=42):
    """(In a data-parallel group the caller installs the exchange: ``_install_exchange``.)"""
    from agent0_amd.deepq.config import parse_overrides
    from agent0_amd.deepq.trainer import Trainer
    monkeypatch.setenv("A0_NATIVE_LOOP", "1" if native else "0")
    cfg = parse_overrides([f"learner.algo={algo}", f"actor.eps_ladder={ladder}", f"seed={seed}", f"logdir={tmp_path / tag}"] + BASE5 + list(extra))
    return Trainer(cfg, use_lp=use_lp)


def _state(tr):
    torch.cuda.synchronize()
    eng, rp = tr.learner.engine, tr.replay
    n = len(rp)                                       # the ring does not wrap in these runs: the rows written so far (the rest was never initialised)
    return [eng.online.flat.clone(), eng.target.flat.clone(), eng.adam_m.clone(), eng.adam_v.clone(), eng.state.clone(), rp.frames[: n * rp.row_bytes].clone(), rp.act[:n].clone(),
            rp.rew[:n].clone(), rp.done[:n].clone()]


def _close(tr):
    tr.test = lambda: None
    tr.final(save=False)


def _run(tmp_path, monkeypatch, native, algo, extra, use_lp, tag, ladder=ALPHA, iters=6, dp=False):
    from agent0_amd.deepq.native_loop import NativeLoop
    tr = _trainer(tmp_path, monkeypatch, native, algo, extra, use_lp, tag, ladder)
    hook = _install_exchange(tr) if dp else None
    res = [{k: v for k, v in tr.run_iteration().items() if k != "fps"} for _ in range(iters)]
    assert isinstance(tr._nl, NativeLoop) if native else tr._nl is False, getattr(tr, "native_loop_reason", None)
    out = _state(tr), res, list(tr.Qs), list(tr.Rs), tr.frame_count
    assert res[-1]["loss"] is not None, "updates ran"
    _close_exchange(tr, hook) if dp else _close(tr)
    return out


def _assert_same_run(a, b):
    for i, (x, y) in enumerate(zip(a[0], b[0])):
        assert torch.equal(x, y), f"state item {i}"
    assert a[1:] == b[1:]


@pytest.mark.parametrize("mode", ["main", "launch", "dp"])
@pytest.mark.parametrize("algo,extra", [("dqn", []), ("c51", ["learner.noisy_net=true", "learner.dueling_head=true", "learner.n_step_q=3"])], ids=["dqn", "c51-noisy-duel-n3"])
def test_handles_and_python_classes_end_on_the_same_state(algo, extra, mode, tmp_path, monkeypatch):
    """Three iterations past training_start_steps, the scheduled epsilon below 1 from the third rollout on.  ``dp``: a one-rank RCCL group (A0_DP_FORCE=1)."""
    dp = mode == "dp"
    import torch.distributed as dist
    if dp:
        _one_rank_group(monkeypatch)
    try:
        a = _run(tmp_path, monkeypatch, False, algo, extra, mode == "launch", "py", dp=dp)
        b = _run(tmp_path, monkeypatch, True, algo, extra, mode == "launch", "nat", dp=dp)
    finally:
        if dp:
            dist.destroy_process_group()
    _assert_same_run(a, b)
    assert a[4] == 6 * E5 * T5


@pytest.mark.parametrize("native", [True, False], ids=["handles", "python-classes"])
def test_a_ladder_run_is_the_plain_run_until_epsilon_drops_below_one(native, tmp_path, monkeypatch):
    on = _run(tmp_path, monkeypatch, native, "dqn", [], False, "on")
    off = _run(tmp_path, monkeypatch, native, "dqn", [], False, "off", ladder=0.0)
    n, rb = E5 * T5, 2 * 4 * 84 * 84
    warm = 2 * n                                      # the rollouts at frames 0 and 128: eps = 1.4 and 1.15
    for k in (5, 6, 7, 8):                            # frames, act, rew, done
        per = rb if k == 5 else 1
        assert torch.equal(on[0][k][: warm * per], off[0][k][: warm * per]), "byte-identical while the scheduled epsilon is >= 1"
    assert not torch.equal(on[0][6][warm: 6 * n], off[0][6][warm: 6 * n]), "once epsilon is below 1 the envs explore differently"
    assert on[1][0] == off[1][0] and on[1][1] == off[1][1]


@pytest.mark.parametrize("native", [True, False], ids=["handles", "python-classes"])
def test_a_snapshot_taken_mid_run_resumes_bit_for_bit(native, tmp_path, monkeypatch):
    want = _run(tmp_path, monkeypatch, native, "dqn", [], False, "a")
    tr = _trainer(tmp_path, monkeypatch, native, "dqn", [], False, "b")
    for _ in range(3):
        tr.run_iteration()
    snap_dir = tr.save_snapshot(str(tmp_path / "snap"))
    _close(tr)
    tr = _trainer(tmp_path, monkeypatch, native, "dqn", [], False, "c", seed=7)
    tr.load_snapshot(snap_dir)
    res = [{k: v for k, v in tr.run_iteration().items() if k != "fps"} for _ in range(3)]
    got = _state(tr)
    _close(tr)
    for i, (x, y) in enumerate(zip(got, want[0])):
        assert torch.equal(x, y), f"state item {i}"
    assert res == want[1][3:]


def test_test_rollouts_keep_the_scalar(tmp_path):
    from agent0_amd.deepq.agent import Actor
    from agent0_amd.deepq.model import DeepQNet
    outs = []
    for ladder in (ALPHA, 0.0):
        cfg = make_cfg("dqn", 8, tmp_path, **{"actor.sample_steps": 6, "actor.eps_ladder": ladder})
        model = DeepQNet(cfg)
        model.load_state_dict({k: torch.from_numpy(v) for k, v in recipe.make_state_dict(recipe.SPECS["dqn"], 11).items()})
        actor = Actor(cfg, model, replay=None, rank=1000)          # the Trainer's test actor
        frames, rs, qs = actor.sample(0.3, test=True)
        a, q = actor.act(0.3)
        assert actor.eps_vec is None, "a test actor allocates no vector"
        outs.append((np.concatenate(frames), rs, qs, a.tolist(), q))
        actor.close()
    assert np.array_equal(outs[0][0], outs[1][0]) and outs[0][1:] == outs[1][1:]


def test_the_attached_pool_gives_the_bytes_of_the_python_host_rollout(tmp_path, monkeypatch):
    """A main-schedule Trainer over one HostEnvPool with worker processes: the actor handle steps the pool (a0_actor_attach_pool) with its own vector."""
    import host_slices
    from agent0_amd.common import atari_wrappers
    from agent0_amd.deepq.native_loop import NativeLoop
    monkeypatch.setattr(atari_wrappers, "real_atari_available", lambda: True)
    monkeypatch.setattr(atari_wrappers, "AtariSlice", lambda env_id, episode_life, seed: host_slices.synth_slice(seed, 0))
    res = []
    for native in (True, False):
        tr = _trainer(tmp_path, monkeypatch, native, "dqn", [], False, f"pool{int(native)}")
        out = [tr.run_iteration() for _ in range(5)]
        assert isinstance(tr._nl, NativeLoop) if native else tr._nl is False, getattr(tr, "native_loop_reason", None)
        assert hasattr(tr.actors[1].envs, "step_send") and tr.actors[1].ladder_alpha == ALPHA
        res.append((_state(tr), [o["loss"] for o in out], [o["qmax"] for o in out], tr.frame_count))
        _close(tr)
    for x, y in zip(res[0][0], res[1][0]):
        assert torch.equal(x, y)
    assert res[0][1:] == res[1][1:]
