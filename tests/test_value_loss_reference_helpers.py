"""CPU: the float64 references of tests/value_loss_ref.py (the yardstick of tests/test_gpu_value_loss_reference.py) against what the project already trusts —
the G4 fixture (the reference's projected distribution and loss, both n), oracle.losses.c51_project and log_softmax_tau run in float64, F.smooth_l1_loss,
torch.autograd of sum_b w_b loss_b and a central finite difference — and the bounds of value_loss_ref.py against an fp32 restatement of the kernels'
arithmetic (tests/cpu_ops.py's torch fp32 losses and a lane-by-lane head row: eight fused multiply-adds, a six-stage butterfly, the bias), which must stay
within HALF of every bound at every case the GPU test runs, and against seven deliberately wrong computations, each of which the bounds must reject.  It
also shows that no sample of any head case needs excluding: the float64 gap between the two best selecting values exceeds four bounds everywhere but at
the planted tie."""
import dataclasses

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import actor_tail_cases as C
import recipe
import value_loss_ref as V
from cpu_ops import CpuOps
from oracle import losses, nets
from util import golden, greedy_check

SPARE = 2.0
OPS = object.__new__(CpuOps)             # the torch restatements of the losses need none of the emulation library's state


def _t(a, dtype=None):
    t = torch.from_numpy(np.ascontiguousarray(a))
    return t if dtype is None else t.to(dtype)


def _frac(got, want, tol):
    got, want, tol = (np.asarray(x, np.float64) for x in (got, want, tol))
    err = np.abs(got - want)
    return float(np.max(np.where(tol > 0, err / np.where(tol > 0, tol, 1.0), np.where(err == 0, 0.0, np.inf))))


# ------------------------------------------------------------------------------------------------ against the fixture and the oracle
@pytest.mark.parametrize("n", [1, 3])
def test_projection_and_loss_against_the_reference_fixture(n):
    """G4: target_prob is the reference's fp32 projection of the fixture's selected target distribution, so it lies within the bound an fp32 projection is held
    to (c51_projection_bounds) and, away from the positions' rounding, within 1e-6 relative + 1e-7 (what tests/test_oracle_golden.py holds the oracle to) on all
    but the rows whose positions are integers; the loss from the oracle's fp32 online logits (5e-5 + 5e-6)."""
    g = golden(f"g4_c51_projection_n{n}")
    spec = recipe.SPECS["c51"]
    atoms = nets.c51_atoms(spec).numpy()
    p = g["prob_next_sel"].astype(np.float64)
    m, b, delta = V.c51_project64(p, g["rewards"], g["terminals"], atoms, 0.99 ** n, -10.0, 10.0, with_parts=True)
    _, tol_m, tol_mass = V.c51_projection_bounds(p, np.log(p), m, b, delta, g["rewards"], atoms, 0.99 ** n, -10.0)
    assert _frac(g["target_prob"], m, tol_m) <= 1.0
    assert _frac(g["target_prob"].astype(np.float64).sum(-1), p.sum(-1), tol_mass + 51 * V.U) <= 1.0          # (+ the fp32 sum of the fixture's p itself)
    assert np.abs(m - g["target_prob"]).max() < 5e-6 and np.abs(m.sum(-1) - p.sum(-1)).max() < 1e-12
    po = {k: _t(np.asarray(v)) for k, v in recipe.make_state_dict(spec, 11).items()}
    ft = nets.normalize(_t(recipe.make_frames(len(g["rewards"]), seed=41)))
    obs, _ = torch.split(ft, 4, 1)
    with torch.no_grad():
        x = nets.forward(po, spec, obs).numpy()
    loss, _, _ = V.c51_loss64(x[np.arange(len(m)), g["actions"]], m)
    assert (np.abs(loss - g["loss"]) <= 5e-6 + 5e-5 * np.abs(g["loss"])).all()


@pytest.mark.parametrize("T,vmin,vmax,n", [(51, -10.0, 10.0, 1), (51, -10.0, 10.0, 3), (7, 0.0, 200.0, 3), (64, -5.0, 5.0, 1), (2, -10.0, 10.0, 1)])
def test_projection_against_the_oracle_in_float64(T, vmin, vmax, n):
    """oracle.losses.c51_project on float64 tensors: random rewards, clamping rewards, terminals and integer positions (both fix-ups), 1e-12."""
    g = recipe.gen(T + n)
    B = 12
    atoms = V.c51_atoms(vmin, vmax, T)
    p = V.softmax64(g.standard_normal((B, T)).astype(np.float32) * 2)
    rew = (vmin + (vmax - vmin) * g.random(B)).astype(np.float32)
    done = (np.arange(B) % 3 == 0).astype(np.float32)
    rew[0], rew[3], rew[6] = vmin, vmax, atoms[T // 2]                                   # done rows: b = 0, T - 1 and an interior integer
    rew[1], rew[2] = vmax + 3 * (vmax - vmin), vmin - 3 * (vmax - vmin)
    hp = losses.Hyper(discount=float(np.float32(0.99 ** n)), n_step=1, vmin=vmin, vmax=vmax)
    want = losses.c51_project(_t(p), _t(rew, torch.float64), _t(done, torch.float64), _t(atoms, torch.float64), hp, (vmax - vmin) / (T - 1)).numpy()
    m, b, _ = V.c51_project64(p, rew, done, atoms, 0.99 ** n, vmin, vmax, with_parts=True)
    assert np.abs(m - want).max() < 1e-12
    assert (b[0] == 0).all() and (b[3] == T - 1).all() and (b == np.round(b)).any()
    assert np.abs(m.sum(-1) - 1).max() < 1e-12 and (m >= 0).all()


@pytest.mark.parametrize("tau", V.MDQN_TAUS)
def test_log_policy_and_target_against_the_oracle_in_float64(tau):
    g = recipe.gen(17)
    B, A = 9, 6
    x = (g.standard_normal((B, A)) * 3).astype(np.float32)
    x[1] = 0.5
    x[2] += 100
    t32 = float(np.float32(tau))
    assert np.abs(V.log_softmax_tau64(x, t32) - losses.log_softmax_tau(_t(x, torch.float64), t32).numpy()).max() < 1e-12
    c = V.mdqn_case(128, 4, tau)
    ref = V.mdqn64(c["q"], c["q_next"], c["q_cur"], 4, c["act"], c["rew"], c["done"], c["wgt"], V.GAMMA, tau, c["lo"], 128)
    ql, qc = _t(c["q_next"], torch.float64), _t(c["q_cur"], torch.float64)
    lo, gam = float(np.float32(c["lo"])), float(np.float32(V.GAMMA))
    v_next = (ql.softmax(dim=-1) * (ql - losses.log_softmax_tau(ql, t32))).sum(dim=-1)
    add_on = losses.log_softmax_tau(qc, t32)[torch.arange(128), _t(c["act"]).long()].clamp(lo, 0)
    y = _t(c["rew"], torch.float64) + t32 * add_on + gam * (1 - _t(c["done"], torch.float64)) * v_next
    assert np.abs(ref["y"] - y.numpy()).max() < 1e-11 * max(1.0, float(np.abs(ref["y"]).max()))
    p = c["planted"]
    assert ref["add_on"][p["lo_active"]] == lo and lo < ref["add_on"][p["lo_inactive"]] < 0 and abs(ref["add_on"][p["argmax"]]) < 1e-6
    assert abs(abs(ref["d"][p["seam"]]) - 1) < 1e-5 and np.abs(c["q_next"][p["big"]]).min() > 99


def test_smooth_l1_against_torch():
    d = np.concatenate((recipe.gen(1).standard_normal(200) * 2, [0.0, 1.0, -1.0, float(V.ONE_UP), -float(V.ONE_DOWN)]))
    loss, slope = V.smooth_l1(d, d.astype(np.float32))
    x = _t(d).requires_grad_(True)
    want = F.smooth_l1_loss(x, torch.zeros_like(x), reduction="none")
    want.sum().backward()
    assert np.abs(loss - want.detach().numpy()).max() < 1e-15 and np.abs(slope - x.grad.numpy()).max() < 1e-7           # (the two slopes meet at the seam)


# ------------------------------------------------------------------------------------------------ gradients: autograd and a central difference
def _dqn_total(q, c, A, B):
    y = torch.from_numpy(V.dqn64(c["q"], c["q_next"], A, c["act"], c["a_star"], c["rew"], c["done"], c["wgt"], V.GAMMA, B)["y"])
    l = F.smooth_l1_loss(q[torch.arange(B), _t(c["act"]).long()], y, reduction="none")
    return (l * _t(c["wgt"], torch.float64)).sum()


def _mdqn_total(q, c, A, B):
    y = torch.from_numpy(V.mdqn64(c["q"], c["q_next"], c["q_cur"], A, c["act"], c["rew"], c["done"], c["wgt"], V.GAMMA, c["tau"], c["lo"], B)["y"])
    l = F.smooth_l1_loss(q[torch.arange(B), _t(c["act"]).long()], y, reduction="none")
    return (l * _t(c["wgt"], torch.float64)).sum()


def _c51_total(x, r, A, B):
    m = torch.from_numpy(r["m"])
    logp = x[torch.arange(B), _t(r["act"]).long()].log_softmax(dim=-1)
    return (-(m * logp).sum(-1) * torch.from_numpy(r["w"][:, 0])).sum()


def _central(fn, x, h=1e-6):
    fd = np.zeros(x.shape)
    it = np.nditer(x, flags=["multi_index"])
    for _ in it:
        i = it.multi_index
        xp, xm = x.copy(), x.copy()
        xp[i] += h
        xm[i] -= h
        fd[i] = (float(fn(torch.from_numpy(xp))) - float(fn(torch.from_numpy(xm)))) / (2 * h)
    return fd


def test_value_gradients_against_autograd_and_a_central_difference():
    """dq of the DQN and the Munchausen loss: autograd of sum_b w_b loss_b on F.smooth_l1_loss at B = 128 (the planted seams differ by what the slopes differ
    there: nothing), a central difference at B = 1 on a row away from the seam."""
    B, A = 128, 4
    for total, c, ref in ((_dqn_total, V.dqn_case(B, A), None), (_mdqn_total, V.mdqn_case(B, A, 0.03), None)):
        r = (V.dqn64(c["q"], c["q_next"], A, c["act"], c["a_star"], c["rew"], c["done"], c["wgt"], V.GAMMA, B) if total is _dqn_total else
             V.mdqn64(c["q"], c["q_next"], c["q_cur"], A, c["act"], c["rew"], c["done"], c["wgt"], V.GAMMA, c["tau"], c["lo"], B))
        q = _t(c["q"], torch.float64).requires_grad_(True)
        total(q, c, A, B).backward()
        assert np.abs(r["dq"] - q.grad.numpy()).max() < 1e-6          # at a planted seam d32 and d may sit on different sides: the slopes differ by |d| - 1
        off = np.ones((B, A), bool)
        off[np.arange(B), c["act"]] = False
        assert (r["dq"][off] == 0).all()
    for total, c in ((_dqn_total, V.dqn_case(1, 4, 5)), (_mdqn_total, V.mdqn_case(1, 4, 0.03, 0))):
        r = (V.dqn64(c["q"], c["q_next"], 4, c["act"], c["a_star"], c["rew"], c["done"], c["wgt"], V.GAMMA, 1) if total is _dqn_total else
             V.mdqn64(c["q"], c["q_next"], c["q_cur"], 4, c["act"], c["rew"], c["done"], c["wgt"], V.GAMMA, c["tau"], c["lo"], 1))
        assert abs(abs(r["d"][0]) - 1) > 1e-3
        fd = _central(lambda q: total(q, c, 4, 1), c["q"].astype(np.float64))
        assert np.abs(r["dq"] - fd).max() < 1e-8 * max(1.0, np.abs(fd).max()) and np.abs(fd).max() > 1e-3


def _c51_ref(rows, A, T, vmin, vmax, gam):
    B = len(rows["kinds"])
    r = V.c51_64(rows["logits"], rows["tgt_logits"], A, T, rows["act"], rows["a_star"], rows["rew"], rows["done"], rows["wgt"], rows["atoms"], gam, vmin, vmax, B)
    r["act"] = rows["act"]
    return r


def test_categorical_gradient_against_autograd_and_a_central_difference():
    A, T, vmin, vmax, gam = 3, 7, -10.0, 10.0, 0.99
    rows = V.c51_rows(V.C51_KINDS, T, A, vmin, vmax, 5)
    B = len(rows["kinds"])
    r = _c51_ref(rows, A, T, vmin, vmax, gam)
    x = _t(rows["logits"], torch.float64).requires_grad_(True)
    _c51_total(x, r, A, B).backward()
    assert np.abs(r["dlogits"] - x.grad.numpy()).max() < 1e-12 * max(1.0, np.abs(r["dlogits"]).max())
    rows = V.c51_rows(("random", "terminal"), T, A, vmin, vmax, 6)
    r = _c51_ref(rows, A, T, vmin, vmax, gam)
    fd = _central(lambda x: _c51_total(x, r, A, 2), rows["logits"].astype(np.float64))
    assert np.abs(r["dlogits"] - fd).max() < 1e-8 * max(1.0, np.abs(fd).max()) and np.abs(fd).max() > 1e-3


# ------------------------------------------------------------------------------------------------ the fp32 restatement stays inside the bounds
def _cpu_dqn(c, A, B):
    loss, dq, st = torch.empty(B), torch.empty(B * A), torch.zeros(8, dtype=torch.int32)
    OPS.loss_dqn(_t(c["q"]).reshape(-1), _t(c["q_next"]).reshape(-1), A, _t(c["act"]), _t(c["a_star"]), _t(c["rew"]), _t(c["done"]), _t(c["wgt"]),
                 float(np.float32(V.GAMMA)), B, loss, dq, st)
    return loss.numpy(), dq.numpy().reshape(B, A), int(st[0])


def _cpu_mdqn(c, A, B):
    loss, dq, st = torch.empty(B), torch.empty(B * A), torch.zeros(8, dtype=torch.int32)
    OPS.loss_mdqn(_t(c["q"]).reshape(-1), _t(c["q_next"]).reshape(-1), _t(c["q_cur"]).reshape(-1), A, _t(c["act"]), _t(c["rew"]), _t(c["done"]), _t(c["wgt"]),
                  float(np.float32(V.GAMMA)), float(np.float32(c["tau"])), float(np.float32(c["lo"])), B, loss, dq, st)
    return loss.numpy(), dq.numpy().reshape(B, A), int(st[0])


def _cpu_c51(rows, A, T, vmin, vmax, gam):
    B = len(rows["kinds"])
    loss, dl, m, st = torch.empty(B), torch.empty(B * A * T), torch.empty(B * T), torch.zeros(8, dtype=torch.int32)
    OPS.loss_c51(_t(rows["logits"]).reshape(-1), _t(rows["tgt_logits"]).reshape(-1), A, T, _t(rows["act"]), _t(rows["a_star"]), _t(rows["rew"]), _t(rows["done"]),
                 _t(rows["wgt"]), _t(rows["atoms"]), float(np.float32(gam)), vmin, vmax, B, loss, dl, m, st)
    return loss.numpy(), dl.numpy().reshape(B, A, T), m.numpy().reshape(B, T), int(st[0])


@pytest.mark.parametrize("A", V.DQN_AS)
@pytest.mark.parametrize("B", V.LOSS_BS)
def test_fp32_restatement_of_the_dqn_loss_stays_inside_the_bound(B, A):
    for variant in range(len(V.DQN_PLAN) if B == 1 else 1):
        c = V.dqn_case(B, A, variant)
        ref = V.dqn64(c["q"], c["q_next"], A, c["act"], c["a_star"], c["rew"], c["done"], c["wgt"], V.GAMMA, B)
        tl, tg = V.dqn_bounds(ref, c["wgt"])
        loss, dq, flag = _cpu_dqn(c, A, B)
        rows = np.arange(B)
        assert _frac(loss, ref["loss"], tl) * SPARE <= 1 and _frac(dq[rows, c["act"]], ref["dq"][rows, c["act"]], tg) * SPARE <= 1 and flag == 0
        assert B == 1 or set(c["planted"]) == {p[0] for p in V.DQN_PLAN}
        assert {0, A - 1} <= set(c["act"].tolist()) | ({0, A - 1} if B == 1 else set()) and (B == 1 or {0, A - 1} <= set(c["a_star"].tolist()))


@pytest.mark.parametrize("tau", V.MDQN_TAUS)
@pytest.mark.parametrize("A", V.MDQN_AS)
@pytest.mark.parametrize("B", V.LOSS_BS)
def test_fp32_restatement_of_the_munchausen_loss_stays_inside_the_bound(B, A, tau):
    for variant in range(7 if B == 1 else 1):
        c = V.mdqn_case(B, A, tau, variant)
        ref = V.mdqn64(c["q"], c["q_next"], c["q_cur"], A, c["act"], c["rew"], c["done"], c["wgt"], V.GAMMA, tau, c["lo"], B)
        tl, tg = V.mdqn_bounds(ref, c["wgt"])
        loss, dq, flag = _cpu_mdqn(c, A, B)
        rows = np.arange(B)
        assert _frac(loss, ref["loss"], tl) * SPARE <= 1 and _frac(dq[rows, c["act"]], ref["dq"][rows, c["act"]], tg) * SPARE <= 1 and flag == 0
        if A == 1:
            assert (ref["lp_next"] == 0).all() and np.array_equal(ref["v_next"], c["q_next"][:, 0].astype(np.float64))


@pytest.mark.parametrize("A", V.C51_AS)
@pytest.mark.parametrize("T", V.C51_TS)
def test_fp32_restatement_of_the_categorical_loss_stays_inside_the_bound(T, A):
    seen = set()
    for vmin, vmax, gam, _, rows in V.c51_launches(T, A):
        ref = _c51_ref(rows, A, T, vmin, vmax, gam)
        loss, dl, m, flag = _cpu_c51(rows, A, T, vmin, vmax, gam)
        B = len(rows["kinds"])
        got_g = dl[np.arange(B), rows["act"]]
        fr = [_frac(m, ref["m"], ref["tol_m"]), _frac(m.astype(np.float64).sum(-1), ref["mass"], ref["tol_mass"]), _frac(loss, ref["loss"], ref["tol_loss"]),
              _frac(got_g, ref["g"], ref["tol_g"])]
        assert max(fr) * SPARE <= 1 and flag == 0, (rows["kinds"], vmin, vmax, gam, fr)
        seen |= set(rows["kinds"])
    assert seen == set(V.C51_KINDS)


def _head32(c, k, h):
    """The head row lane by lane (actor_tail_cases.qhead32 with fc1 the identity in one slab: h passes through bit for bit)."""
    return C.qhead32(h, np.eye(512, dtype=np.float32), np.zeros(512, np.float32), c["W_" + k], c["b_" + k], c["A"], c["dueling"], 1)


@pytest.mark.parametrize("with_sel", [0, 1])
@pytest.mark.parametrize("A,dueling", V.HEAD_HEADS)
def test_fp32_restatement_of_the_head_stays_inside_the_bound_and_no_sample_is_excluded(A, dueling, with_sel):
    for B in V.HEAD_BS:
        c = dict(V.head_case(B, A, dueling, with_sel), ld=32)
        ref = V.head_loss64(c)
        q_on, q_tg = _head32(c, "on", c["h_on"]), _head32(c, "tg", c["h_tg"])
        q_sel = _head32(c, "on", c["h_sel"]) if with_sel else q_tg
        assert _frac(q_on, ref["q_on"], ref["t_on"]) * SPARE <= 1 and _frac(q_tg, ref["q_tg"], ref["t_tg"]) * SPARE <= 1
        assert (c["h_on"] == 0).mean() > 0.3
        a, qm = C.first_max(q_sel)
        tied = c["tied"]
        if A >= 2:
            assert tied[0] and (a[tied] == c["tie"][0]).all()
            if A > 2 and B > 2:
                C.check_spread(ref["q_sel"], tied, A, f"head A={A} B={B}")
        # the share of samples whose greedy action the bound leaves open, the planted pair aside: zero, at twice the bound too
        share = greedy_check(ref["q_sel"], 2 * ref["t_sel"], a, qm, exclude=tied, tie=c["tie"], allow_empty=True) if A > 1 else 0.0
        assert share == 0.0 and np.array_equal(a, ref["a_star"])
        if with_sel and A >= 2:
            # the later of the two equal maxima would show: the target's rows are not tied, and the loss moves by more than its bound
            j = c["tie"][1]
            d_j = ref["q_on"][0, c["act"][0]] - (c["rew"][0] + float(np.float32(c["gamma_n"])) * (1 - c["done"][0]) * ref["q_tg"][0, j])
            assert abs(V.smooth_l1(d_j, np.float32(d_j))[0] - ref["loss"][0]) > 100 * ref["tol_loss"][0]
        # the loss and draw of the restated q values
        y = (c["rew"] + (np.float32(c["gamma_n"]) * (1 - c["done"])).astype(np.float32) * q_tg[np.arange(B), a]).astype(np.float32)
        d = (q_on[np.arange(B), c["act"]] - y).astype(np.float32)
        loss = np.where(np.abs(d) < 1, np.float32(0.5) * d * d, np.abs(d) - np.float32(0.5))
        assert _frac(loss, ref["loss"], ref["tol_loss"]) * SPARE <= 1
        assert _frac(c["wgt"] * np.clip(d, -1, 1), ref["g"], ref["tol_g"]) * SPARE <= 1


# ------------------------------------------------------------------------------------------------ wrong computations are rejected
def _rejected(got, want, tol, what):
    assert _frac(got, want, tol) > 1.0, f"negative control {what}: the bound does not reject it ({_frac(got, want, tol):.3f} of it)"


def test_the_bounds_reject_wrong_computations():
    # 1. the last maximum instead of the first on a planted tie: the loss takes the other target value
    c = dict(V.head_case(5, 4, 1, 1), ld=32)
    ref = V.head_loss64(c)
    i, j = c["tie"]
    assert ref["a_star"][0] == i and ref["q_tg"][0, i] != ref["q_tg"][0, j]
    y = c["rew"][0] + float(np.float32(c["gamma_n"])) * (1 - c["done"][0]) * ref["q_tg"][0, j]
    d = ref["q_on"][0, c["act"][0]] - y
    _rejected(V.smooth_l1(d, np.float32(d))[0], ref["loss"][0], ref["tol_loss"][0], "last maximum on the planted tie")
    with pytest.raises(AssertionError, match="the later one was chosen"):
        a = ref["a_star"].copy()
        a[0] = j
        greedy_check(ref["q_sel"], ref["t_sel"], a, ref["q_sel"][np.arange(5), a], tie=c["tie"])
    # 2., 3. a projection fix-up dropped: an integer position keeps lo == up, (up - b) = (b - lo) = 0 and the atom's mass is lost
    T, A, vmin, vmax, gam = 51, 4, -10.0, 10.0, 0.99
    rows = V.c51_rows(V.C51_KINDS[0:5], T, A, vmin, vmax, 3)
    ref = _c51_ref(rows, A, T, vmin, vmax, gam)
    for kw, what, row in ((dict(fixup1=False), "first fix-up dropped", 3), (dict(fixup2=False), "second fix-up dropped", 2)):
        m = V.c51_project64(ref["p"], rows["rew"], rows["done"], rows["atoms"], gam, vmin, vmax, **kw)
        _rejected(m[row], ref["m"][row], ref["tol_m"][row], what)
        _rejected(m.sum(-1), ref["mass"], ref["tol_mass"], what + " (mass)")
    # 4. v_next with the softmax at temperature tau; 5. the add-on clamped only below; 6. gamma_n applied on terminal rows; 7. w multiplied into the loss
    B, A, tau = 128, 4, 0.03
    c = V.mdqn_case(B, A, tau)
    ref = V.mdqn64(c["q"], c["q_next"], c["q_cur"], A, c["act"], c["rew"], c["done"], c["wgt"], V.GAMMA, tau, c["lo"], B)
    tl, tg = V.mdqn_bounds(ref, c["wgt"])
    t32, lo, gam32 = float(np.float32(tau)), float(np.float32(c["lo"])), float(np.float32(V.GAMMA))
    qn, r, dn, rows_ = c["q_next"].astype(np.float64), c["rew"].astype(np.float64), c["done"].astype(np.float64), np.arange(B)
    qa = c["q"][rows_, c["act"]].astype(np.float64)

    def loss_of(y):
        d = qa - y
        return V.smooth_l1(d, d.astype(np.float32))[0]

    # q' - lp(q') = max q' + tau logsumexp is the same for every action, so ANY weights that sum to one give the same v_next; what a kernel can get wrong is
    # the normalisation: the temperature-1 exponentials over the temperature-tau sum
    zn = qn - qn.max(-1, keepdims=True)
    v_tau = (np.exp(zn) / np.exp(zn / t32).sum(-1, keepdims=True) * (qn - ref["lp_next"])).sum(-1)
    assert np.abs((V.softmax64(qn / t32) * (qn - ref["lp_next"])).sum(-1) - ref["v_next"]).max() < 1e-12
    _rejected(loss_of(r + t32 * ref["add_on"] + gam32 * (1 - dn) * v_tau), ref["loss"], tl, "v_next at temperature tau")
    raw_add = ref["lp_cur"][rows_, c["act"]]
    assert (raw_add < lo).any()
    _rejected(loss_of(r + t32 * np.minimum(raw_add, 0.0) + gam32 * (1 - dn) * ref["v_next"]), ref["loss"], tl, "add-on without the clamp at lo")
    assert dn.any()
    _rejected(loss_of(r + t32 * ref["add_on"] + gam32 * ref["v_next"]), ref["loss"], tl, "gamma_n on terminal rows (mdqn)")
    cd = V.dqn_case(B, A)
    rd = V.dqn64(cd["q"], cd["q_next"], A, cd["act"], cd["a_star"], cd["rew"], cd["done"], cd["wgt"], V.GAMMA, B)
    tld, tgd = V.dqn_bounds(rd, cd["wgt"])
    yd = cd["rew"].astype(np.float64) + gam32 * cd["q_next"][rows_, cd["a_star"]].astype(np.float64)
    dd = cd["q"][rows_, cd["act"]].astype(np.float64) - yd
    _rejected(V.smooth_l1(dd, dd.astype(np.float32))[0], rd["loss"], tld, "gamma_n on terminal rows (dqn)")
    w = cd["wgt"].astype(np.float64)
    _rejected(w * rd["loss"], rd["loss"], tld, "w multiplied into the loss")
    _rejected(rd["slope"], rd["dq"][rows_, cd["act"]], tgd, "w left out of the gradient")
    rows = V.c51_rows(V.C51_KINDS[5:10], T, 4, vmin, vmax, 4)
    ref = _c51_ref(rows, 4, T, vmin, vmax, 0.99)
    _rejected(ref["w"][:, 0] * ref["loss"], ref["loss"], ref["tol_loss"], "w multiplied into the categorical loss")


def test_the_finding_rows_ask_for_a_bin_above_the_last_in_fp32():
    """The four supports of the issue's table: the fp32 position of vmax, (vmax - vmin) / fl32(delta), exceeds T - 1; bounded by T - 1 (tests/cpu_ops.py, the
    kernels) the restatement conserves the mass, unbounded it asks scatter_add_ for index T."""
    for vmin, vmax, T in V.FINDING:
        delta = np.float32((vmax - vmin) / (T - 1))
        assert np.float32(np.float32(vmax - vmin) / delta) > T - 1
        rows = V.c51_rows(("clamp_high", "tgt_peak", "binlast"), T, 2, vmin, vmax, 9)
        rows["rew"][1] = vmax + 2 * (vmax - vmin)                    # clamps every atom, like row 0
        ref = _c51_ref(rows, 2, T, vmin, vmax, 0.99)
        loss, dl, m, flag = _cpu_c51(rows, 2, T, vmin, vmax, 0.99)
        assert _frac(m.astype(np.float64).sum(-1), ref["mass"], ref["tol_mass"]) <= 1 and _frac(m, ref["m"], ref["tol_m"]) <= 1 and flag == 0
        # what the unbounded position loses at the peaked row is more than the mass bound allows
        lost = float(np.float32(vmax - vmin) / delta) - (T - 1)
        assert lost * ref["p"][1].max() > ref["tol_mass"][1]


def test_the_emulation_carries_a_nan_reward_to_the_loss_and_the_flag_like_the_kernels():
    """tests/cpu_ops.py::loss_c51 with a NaN reward in sample 2: the flag is set, the NaN stays in that sample, the others stay within half their bounds."""
    T, A, vmin, vmax, gam = 51, 4, -10.0, 10.0, 0.99
    rows = V.c51_rows(V.C51_KINDS[7:12], T, A, vmin, vmax, 21)
    keep = np.arange(5) != 2
    ref = _c51_ref(rows, A, T, vmin, vmax, gam)
    rows["rew"][2] = np.nan
    loss, dl, m, flag = _cpu_c51(rows, A, T, vmin, vmax, gam)
    assert flag == 1 and np.isnan(loss[2]) and int(np.isnan(loss).sum()) == 1 and np.isfinite(m[keep]).all() and np.isfinite(dl[keep]).all()
    assert _frac(m[keep], ref["m"][keep], ref["tol_m"][keep]) * SPARE <= 1 and _frac(loss[keep], ref["loss"][keep], ref["tol_loss"][keep]) * SPARE <= 1
