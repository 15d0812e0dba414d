"""CPU: the yardstick of tests/test_gpu_optim_reference.py (tests/optim_ref.py) against what the project already trusts.

  * adam64 against torch.optim.Adam in float64 over several steps, and against the oracle's Adam (fp32: within half of the bounds);
  * rmsprop64 against torch.optim.RMSprop in float64 and the oracle's RMSprop; clip_coef64 against torch.nn.utils.clip_grad_norm_ in float64;
  * the bookkeeping model against a hand-written table of twelve updates, and against CpuOps.adam_step_sync's status words;
  * an fp32 restatement of both Adam forms and of RMSprop in both contractions within HALF of every bound, on every case the GPU test runs;
  * eight deliberately wrong computations, each rejected by the bounds on the case table."""
import math

import numpy as np
import pytest
import torch

import optim_ref as R
import recipe

F32 = np.float32
LR, B1, B2 = R.HP["lr"], R.HP["b1"], R.HP["b2"]
COEFS = (None,) + tuple(R.clip_coef32(s, R.CLIP_MAX_NORM)[0] for s in R.CLIP_SUMSQ.values())


def _scalars(tname):
    S = R.step_decide([0, R.T_CASES[tname][0], 0, 0, 0, 0, 0, R.T_CASES[tname][1]], None, LR, B1, B2, 2)
    return S["step_size"], S["bc2_sqrt"], S["t"]


# ------------------------------------------------------------------------------------------------ the references
def test_adam64_is_torch_adam_in_float64():
    g = recipe.gen(1)
    p0 = g.standard_normal(257) * 0.05
    P = torch.tensor(p0, dtype=torch.float64, requires_grad=True)
    opt = torch.optim.Adam([P], lr=LR, betas=(B1, B2), eps=1e-2 / 32)
    p, m, v = p0.copy(), np.zeros(257), np.zeros(257)
    H = R.hyper(B1, B2, 1e-2 / 32, exact=True)
    for t in range(1, 8):
        gr = g.standard_normal(257) * (0.1 if t != 4 else 1e-9)
        P.grad = torch.tensor(gr, dtype=torch.float64)
        opt.step()
        ref = R.adam64(p, m, v, gr, H, LR / (1.0 - B1 ** t), math.sqrt(1.0 - B2 ** t))
        p, m, v = ref["p"], ref["m"], ref["v"]
        st = opt.state[P]
        np.testing.assert_allclose(p, P.detach().numpy(), rtol=1e-13, atol=1e-16)
        np.testing.assert_allclose(m, st["exp_avg"].numpy(), rtol=1e-13, atol=1e-18)
        np.testing.assert_allclose(v, st["exp_avg_sq"].numpy(), rtol=1e-13, atol=1e-30)


def test_the_oracles_adam_stays_within_half_of_the_bounds():
    from oracle.learner import Adam
    g = recipe.gen(2)
    for eps in R.EPS_VALUES:
        params = {"w": torch.from_numpy((g.standard_normal(513) * 0.05).astype(F32))}
        opt = Adam(LR, eps, B1, B2)
        H = R.hyper(B1, B2, eps)
        state = [0] * 8
        for t in range(1, 7):
            gr = (g.standard_normal(513) * 0.1).astype(F32)
            p0 = params["w"].numpy().copy()
            m0 = opt.m["w"].numpy().copy() if opt.m else np.zeros(513, F32)
            v0 = opt.v["w"].numpy().copy() if opt.v else np.zeros(513, F32)
            opt.step(params, {"w": torch.from_numpy(gr)})
            S = R.step_update(state, None, LR, B1, B2, 0, "plain")
            assert S["t"] == t == opt.t
            ref = R.adam64(p0, m0, v0, gr, H, S["step_size"], S["bc2_sqrt"])
            for name, got, key in (("p", params["w"], "p"), ("m", opt.m["w"], "m"), ("v", opt.v["w"], "v")):
                frac, msg = R.worst(name, got.numpy(), ref[key], ref["e_" + key], dict(p=p0, m=m0, v=v0, g=gr))
                assert frac <= 0.5, f"eps {eps} t {t}: {msg}"


def test_rmsprop64_is_torch_rmsprop_in_float64_and_the_oracles_in_fp32():
    from oracle.learner import RMSprop
    g = recipe.gen(3)
    p0 = g.standard_normal(300) * 0.05
    P = torch.tensor(p0, dtype=torch.float64, requires_grad=True)
    opt = torch.optim.RMSprop([P], lr=R.RMS["lr"], alpha=R.RMS["alpha"], eps=R.RMS["eps"])
    orc = RMSprop(R.RMS["lr"], R.RMS["alpha"], R.RMS["eps"])
    params = {"w": torch.from_numpy(p0.astype(F32))}
    p, sq = p0.copy(), np.zeros(300)
    for _ in range(4):
        gr = (g.standard_normal(300) * 0.1).astype(F32)
        P.grad = torch.tensor(gr, dtype=torch.float64)
        opt.step()
        ref = R.rmsprop64(p, sq, gr, **R.RMS, exact=True)
        p, sq = ref["p"], ref["sq"]
        np.testing.assert_allclose(p, P.detach().numpy(), rtol=1e-13, atol=1e-16)
        np.testing.assert_allclose(sq, opt.state[P]["square_avg"].numpy(), rtol=1e-13, atol=1e-30)
        q0, s0 = params["w"].numpy().copy(), orc.sq["w"].numpy().copy() if orc.sq else np.zeros(300, F32)
        orc.step(params, {"w": torch.from_numpy(gr)})
        r32 = R.rmsprop64(q0, s0, gr, R.RMS["lr"], R.RMS["alpha"], R.RMS["eps"])
        for name, got, key in (("p", params["w"], "p"), ("sq", orc.sq["w"], "sq")):
            frac, msg = R.worst(name, got.numpy(), r32[key], r32["e_" + key], dict(p=q0, sq=s0, g=gr))
            assert frac <= 0.5, msg


@pytest.mark.parametrize("n", [1, 257, 100384])
def test_clip_coef64_is_clip_grad_norm_in_float64(n):
    g = (recipe.gen(4 + n).standard_normal(n) * 0.1).astype(F32)
    for scale in (0.25, 2.0):
        P = torch.zeros(n, dtype=torch.float64, requires_grad=True)
        P.grad = torch.tensor(g, dtype=torch.float64)
        max_norm = R.f32(scale * float(np.linalg.norm(g.astype(np.float64))))
        total = torch.nn.utils.clip_grad_norm_([P], max_norm)
        coef, norm, rel, _ = R.clip_coef64(g, max_norm)
        assert abs(norm - float(total)) <= 1e-13 * norm
        np.testing.assert_allclose(P.grad.numpy(), g.astype(np.float64) * coef, rtol=1e-12)
        assert (coef == 1.0) == (scale > 1) and 0 < rel < 1e-3


def test_loss_mean64():
    x = (recipe.gen(5).standard_normal(257)).astype(F32)
    mean, tol = R.loss_mean64(x)
    assert abs(mean - float(torch.from_numpy(x).double().mean())) < 1e-15 and abs(float(x.mean()) - mean) <= tol


# ------------------------------------------------------------------------------------------------ the bookkeeping
# state[0..5] after each of SCHEDULE's twelve updates for the committing forms, and t; the pending forms hold the step count in state[5] too
HAND = (
    ([0, 1, 0, 0, 0, 0], 1), ([0, 2, 0, 0, 0, 0], 2), ([0, 3, 0, 0, 1, 0], 3), ([0, 3, 1, 1, 1, 0], 3), ([0, 4, 1, 0, 0, 0], 4), ([0, 4, 2, 1, 1, 0], 4),
    ([0, 5, 2, 0, 1, 0], 5), ([0, 6, 2, 0, 1, 0], 1), ([0, 7, 2, 0, 0, 0], 2), ([0, 8, 2, 0, 0, 0], 1), ([0, 8, 3, 1, 0, 0], 1), ([0, 9, 3, 0, 1, 0], 1),
)


@pytest.mark.parametrize("form", ["plain", "folded", "tail"])
@pytest.mark.parametrize("has_extra", [True, False])
def test_bookkeeping_model_against_the_hand_written_table(form, has_extra):
    state = [0] * 8
    for u, ((kind, reset, tf), (words, t)) in enumerate(zip(R.SCHEDULE, HAND)):
        up, extra = R.schedule_flags(kind, has_extra)
        if up:
            state[0] = 1
        if reset is not None:
            state[7] = reset
        S = R.step_update(state, extra, LR, B1, B2, tf, form)
        want = list(words)
        if form != "plain":
            want[5] = want[1]
        assert state[:6] == want and S["t"] == t, f"update {u}: {state} {S}"
        assert S["step_size"] == R.f32(LR / (1.0 - B1 ** t)) and S["bc2_sqrt"] == R.f32(math.sqrt(1.0 - B2 ** t))
        assert state[6] == 0 and state[7] == (0 if u < 7 else 5 if u < 9 else 9)


def test_saturated_and_clamped_step_counts():
    S = R.step_decide([0, 10 ** 7 - 1, 0, 0, 0, 0, 0, 0], None, LR, B1, B2, 0)
    assert S["t"] == 10 ** 7 and S["step_size"] == R.f32(LR) and R.within_one_ulp(S["bc2_sqrt"], 1.0)
    for name in ("steps==reset", "steps==reset-1"):
        assert _scalars(name)[2] == 1
    assert _scalars("reset+2")[2] == 2
    assert R.within_one_ulp(1.0, np.nextafter(F32(1), F32(2))) and not R.within_one_ulp(1.0, 1.0 + 3e-7)


def test_cpu_ops_status_words_follow_the_model():
    from cpu_ops import CpuOps
    ops = CpuOps()
    n = 8
    p, m, v, t = (torch.zeros(n) for _ in range(4))
    state = torch.zeros(8, dtype=torch.int32)
    scal = torch.zeros(2)
    model = [0] * 8
    for u, (kind, _, tf) in enumerate(R.SCHEDULE):          # CpuOps keeps no reset count: the status words do not depend on it
        up, extra = R.schedule_flags(kind, True)
        if up:
            state[0], model[0] = 1, 1
        ops.adam_step_sync(p, torch.ones(n), m, v, n, state, scal, LR, B1, B2, 1e-3, tf, t, n, torch.tensor([extra]))
        R.step_update(model, extra, LR, B1, B2, tf, "plain")
        assert state[:5].tolist() == model[:5], f"update {u}"


# ------------------------------------------------------------------------------------------------ the fp32 restatements and the wrong computations
def _adam_cases():
    for tname in R.T_CASES:
        for eps in R.EPS_VALUES:
            for coef in COEFS:
                yield tname, eps, coef


def test_fp32_restatements_of_adam_stay_within_half_of_every_bound():
    T = R.adam_table()
    worst_frac = 0.0
    for tname, eps, coef in _adam_cases():
        ss, bc2, _ = _scalars(tname)
        H = R.hyper(B1, B2, eps)
        ref = R.adam64(T["p"], T["m"], T["v"], T["g"], H, ss, bc2, coef=coef, coef_roundings=R.CLIP_ROUNDINGS)
        assert all(np.isfinite(ref[k]).all() for k in ("p", "m", "v", "e_p", "e_m", "e_v")), "the table needs no exclusions"
        for form in ("wide", "scalar"):
            got = dict(zip("pmv", R.adam32(T["p"], T["m"], T["v"], T["g"], H, ss, bc2, form, coef)))
            for k in "pmv":
                frac, msg = R.worst(k, got[k], ref[k], ref["e_" + k], dict(p=T["p"], m=T["m"], v=T["v"], g=T["g"]))
                assert frac <= 0.5, f"{tname} eps {eps} coef {coef} {form}: {msg}"
                worst_frac = max(worst_frac, frac)
    assert worst_frac > 0.1, f"bounds far wider than an fp32 evaluation needs: worst fraction {worst_frac}"


def test_the_square_root_term_and_the_underflow_allowance_are_needed():
    """At a denormal v the kernel's v' is off by an absolute amount; the bound on p' must carry its square root, and the bound on v' its allowance."""
    T = R.adam_table()
    ss, bc2, _ = _scalars("t=1")
    H = R.hyper(B1, B2, 1e-8)
    ref = R.adam64(T["p"], T["m"], T["v"], T["g"], H, ss, bc2)
    _, _, v32 = R.adam32(T["p"], T["m"], T["v"], T["g"], H, ss, bc2, "scalar")
    small = ref["v"] < 2.0 ** -120
    assert small.sum() > 100
    err = np.abs(v32.astype(np.float64) - ref["v"])[small]
    assert (err > 3 * R.U * ref["v"][small]).any(), "some v' misses a purely relative bound"


@pytest.mark.parametrize("name", list(R.WRONG_ADAM))
def test_wrong_adam_computations_are_rejected(name):
    T = R.adam_table()
    for tname in ("t=2", "t=10"):
        for eps in R.EPS_VALUES:
            ss, bc2, t = _scalars(tname)
            H = R.hyper(B1, B2, eps)
            coef = COEFS[1] if name == "step_on_unclipped" else None
            ref = R.adam64(T["p"], T["m"], T["v"], T["g"], H, ss, bc2, coef=coef, coef_roundings=R.CLIP_ROUNDINGS)
            got = dict(zip("pmv", R.WRONG_ADAM[name](T["p"], T["m"], T["v"], T["g"], H, ss, bc2, t, coef)))
            fracs = [R.worst(k, got[k], ref[k], ref["e_" + k], {})[0] for k in "pmv"]
            assert max(fracs) > 10.0, f"{name} at {tname}, eps {eps}: passes the bounds ({fracs})"


def _rms_cases(ns=R.RMSPROP_NS):
    """Every (p, sq, g, coefficient) the GPU test's RMSprop cases start a step from: the fp32 coefficient formed as a0_clip_coef_kernel's would be."""
    for n in ns:
        for zero_p in (True, False):
            for zero_sq in (True, False):
                for clip in R.RMSPROP_CLIPS:
                    p, sq, gs = R.rmsprop_case(n, zero_p, zero_sq)
                    for gr in gs:
                        coef = None if clip == "off" else F32(R.clip_coef64(gr, R.rmsprop_max_norm(gr, clip))[0])
                        assert (clip != "inactive" or coef == 1.0) and (clip != "active" or coef < 0.5)
                        yield p, sq, gr, coef
                        p, sq = R.rmsprop32(p, sq, gr, **R.RMS, contract=False, coef=coef)


def test_fp32_restatements_of_rmsprop_stay_within_half_of_every_bound():
    worst_frac = 0.0
    for p, sq, gr, coef in _rms_cases():
        ref = R.rmsprop64(p, sq, gr, **R.RMS, coef=coef)
        for contract in (False, True):
            gp, gs = R.rmsprop32(p, sq, gr, **R.RMS, contract=contract, coef=coef)
            for name, got, key in (("p", gp, "p"), ("sq", gs, "sq")):
                frac, msg = R.worst(name, got, ref[key], ref["e_" + key], dict(p=p, sq=sq, g=gr))
                assert frac <= 0.5, f"contract {contract}: {msg}"
                worst_frac = max(worst_frac, frac)
    assert worst_frac > 0.1, f"bounds far wider than an fp32 evaluation needs: worst fraction {worst_frac}"


@pytest.mark.parametrize("name", list(R.WRONG_RMSPROP))
def test_wrong_rmsprop_computations_are_rejected(name):
    """lr = 2.5e-8: against the one rounding of a parameter of 0.05 scale no bound can see a step that is off by a fraction of itself — which is why the cases
    hold p = 0, where the step is tested at its own precision.  Every such case must reject the mistake."""
    seen = 0
    for p, sq, gr, coef in _rms_cases((255, 257, 100384)):
        if coef is not None or p.any():
            continue
        ref = R.rmsprop64(p, sq, gr, **R.RMS)
        gp, gs = R.WRONG_RMSPROP[name](p, sq, gr, **R.RMS)
        frac = R.worst("p", gp, ref["p"], ref["e_p"], {})[0]
        assert frac > 10.0, f"{name}: passes the bounds ({frac})"
        seen += 1
    assert seen == 6


def test_the_tables():
    T = R.adam_table()
    assert T["p"].size == R.TABLE_N and len(T["kinds"]) == R.TABLE_N and R.TABLE_N % 4 == 0
    assert R.adam_table() is T and not T["p"].flags.writeable
    kinds = T["kinds"]
    for kd in R.TABLE_KINDS:
        groups = [kinds[i:i + 4] for i in range(0, R.TABLE_N, 4)]
        assert any(gr.count(kd) == 1 and gr.count(R.ORDINARY) == 3 for gr in groups) and any(gr.count(kd) == 4 for gr in groups), kd
    v, g = T["v"], T["g"]
    assert (v == 0).any() and ((v > 0) & (v < 2.0 ** -126)).any() and (v == F32(2.0 ** -126)).any() and v.max() > 2.0 ** 100
    assert (np.signbit(g) & (g == 0)).any() and (np.abs(g) == F32(2.0 ** -70)).any() and np.abs(g).max() > 2.0 ** 50
    idx = [i for i, _ in R.NONFINITE]
    assert len(set(idx)) == 12 and {i % 4 for i in idx} == {0, 1, 2, 3} and len({i // 4 for i in idx}) == 12 and max(idx) < 64
