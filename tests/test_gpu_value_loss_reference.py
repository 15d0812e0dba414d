"""GPU (MI355X): the value and categorical losses against float64, each on its own, at the edges of its work split.

Kernels (agent0_amd/csrc/loss_value.hip, loss_c51.hip): a0_loss_dqn, a0_dqn_head_loss, a0_loss_mdqn and a0_loss_c51 — the yardsticks the bit-identity tests of the fused
a0_dqn_ / a0_mdqn_ / a0_c51_head_loss_slabs kernels compare against (tests/test_gpu_head_loss_chain.py, tests/test_gpu_engine.py), which therefore cannot see
an error the yardstick shares.  References, bounds and cases: tests/value_loss_ref.py, held on the CPU to the G4 fixture, the oracle in float64,
F.smooth_l1_loss, torch.autograd, a finite difference, an fp32 restatement and seven wrong computations by tests/test_value_loss_reference_helpers.py.
Shapes: B around the 128 samples of a block (a0_loss_dqn, a0_loss_mdqn) and the four samples of a workgroup (a0_dqn_head_loss), one action and the widest head
(NQ = 24), T from 2 to the 64 lanes of the wave that holds a sample's atoms.  Last come the fused C51 kernel against its separate launches at T, A, B and slab
counts the existing test skips (the DQN / Munchausen fused kernels at NQ = 24 are added parameters of tests/test_gpu_head_loss_chain.py), and the entry
points' argument checks.

Every output is prefilled with NaN and followed by 64 sentinel elements; columns the contract says are zero are checked bit for bit; the NaN flag is checked
in every case.  Seams (|d| = 1), exact ties and integer bin positions are planted, not avoided, and no sample is excluded anywhere.

Tolerances.  u = 2^-24; an fp32 operation moves its result by at most u of the magnitude it works at, and an element is held to c u SCALE, SCALE the same
computation on absolute values and c the roundings on its longest path (value_loss_ref.py computes them):
  d = q - y         DQN: 5 u S, S = |q| + |r| + gamma_n |q'| (1 - done, its product with gamma_n, the product with q', the sum with r, the difference; one
                    less where the compiler fuses a product and a sum).  done = 1: y is the reward, loss and dq are the fp32 formulas bit for bit
  loss              e_d max(|d|, 1) + 2 u loss (the loss's own product or difference); dq  |w| (e_d + u |clamp d|), exactly 0 away from the taken action
  head row          15 u (sum |h| |w| + |b|): eight fused multiply-adds per lane, six butterfly stages, the bias; the combine adds A + 3
                    (actor_tail_cases.head_roundings).  d then carries both heads' bounds and 5 u S on the heads' magnitudes; draw = the dueling backward of
                    dq: (1 + 1/A at the taken action, 1/A elsewhere) (e_g + 2 u |g|), the value column e_g, pad columns exactly 0
  log-policy        z = x - max rounds by u |z| (the inputs are exact), z / tau once more; logsumexp: EXPF_REL + 2 u sum_k pi_k |z_k / tau| + (A - 1) u +
                    LOGF_BOUND; lp = z - tau lse: u |z| + tau e_lse + 2 u (|z| + tau lse)
  v_next            sum_k p_k (q'_k - lp_k): p_k relative 2 EXPF_REL + u (|z_k| + sum_j p_j |z_j|) + A u, the term e_lp + u (|q'_k| + |lp_k|), A + 1 roundings of
                    the sum; y = r + tau add_on + gamma_n (1 - done) v_next: tau e_lp(a) + gamma_n (1 - done) e_v + 5 u (|r| + tau |add_on| + gamma_n sum p |term|)
  softmax (C51)     one lane per atom: p_k relative 2 EXPF_REL + u (|x_k - max| + sum_j p_j |x_j - max|) + 7 u (butterfly 6, division 1)
  projection        the bin position is off by at most E_k = 6 u (|r| + gamma_n |z_k| + |vmin|) / delta (gamma_n (1 - done), the product, the sum — or one fused
                    multiply-add —, tz - vmin, the division, fl32(delta)).  The projection is 1-Lipschitz in the position, so bin j is held to the sum of p_k E_k
                    over the atoms whose float64 position lies within 1 + E_k of j, plus m_j (rel_p + 2 u) and one u m_j per further non-zero term added into it.
                    The mass sum_j m_j does not see E_k at all ((up - b) + (b - lo) = 1): sum_k p_k (rel_p + 2 u) + the additions.  No row is excluded
  cross entropy     logp_t = x_t - max - logf(sum): 2 u |x_t - max| + EXPF_REL + u sum_j p_j |x_j - max| + 6 u + LOGF_BOUND + u log(sum); loss: sum_t (tol_m |logp| + m
                    tol_logp) + 7 u sum_t m |logp|; dlogits = w (p sum(m) - m): |w| (p msum (rel_p + 2 u) + p tol_msum + tol_m + u (p msum + m))
  expf              EXPF_REL of tests/actor_tail_cases.py (twice the measured 9.1e-8)
  logf              measured here: test_logf_error_stays_within_the_recorded_figure reads logf(s) itself out of a0_loss_c51 (a one-hot target and a one-hot
                    projected distribution make the loss exactly logf of the online softmax's denominator s, which the gradient outputs pin down) for 1e5 values
                    of s in [1, 64] against the float64 logarithm of the same fp32 s.  LOGF_MEASURED (value_loss_ref.py) is the largest deviation on an MI355X,
                    LOGF_BOUND twice it rounded up to a power of two; the test asserts LOGF_BOUND and every bound above uses it.
Each test prints its largest error as a fraction of its tolerance (and records it with util.record_stats)."""
import numpy as np
import pytest
import torch

import actor_tail_cases as C
import recipe
import value_loss_ref as V
from util import record_stats

pytestmark = pytest.mark.gpu

U = V.U
GUARD = 64
SENT = -1.25e38                          # exact in fp32
NAN = float("nan")
LOGF_MEASURED, LOGF_BOUND = V.LOGF_MEASURED, V.LOGF_BOUND


@pytest.fixture(scope="module")
def hip():
    from agent0_amd.ops import HipOps
    ops = HipOps()
    assert "gfx950" in ops.device_info()[2]
    return ops


# ------------------------------------------------------------------------------------------------ helpers
def _dev(hip, a):
    return torch.from_numpy(np.ascontiguousarray(a).reshape(-1)).to(hip.device)


def _out(hip, n, fill=NAN, dtype=torch.float32):
    """n elements of ``fill`` followed by GUARD sentinels."""
    buf = hip.empty(n + GUARD, dtype=dtype)
    buf[:n].fill_(fill)
    buf[n:].fill_(SENT if dtype == torch.float32 else 0x5A5A5A5A)
    return buf


def _flag(hip):
    return _out(hip, 8, fill=0, dtype=torch.int32)


def _take(buf, n, what):
    torch.cuda.synchronize()
    guard = SENT if buf.dtype == torch.float32 else 0x5A5A5A5A
    assert bool((buf[n:] == guard).all()), f"{what}: write past the end"
    return buf[:n].cpu().numpy()


def _bits(a):
    return np.ascontiguousarray(np.asarray(a, np.float32)).view(np.uint32)


def _same_bits(got, want, what):
    got, want = _bits(got).reshape(-1), _bits(want).reshape(-1)
    assert got.shape == want.shape, f"{what}: {got.shape} vs {want.shape}"
    bad = np.nonzero(got != want)[0]
    assert bad.size == 0, f"{what}: {bad.size} of {got.size} elements differ in their bits, first at {bad[:5]}"


def _zero_bits(got, what):
    assert (_bits(got) == 0).all(), f"{what}: must be +0 bit for bit"


class Worst:
    """The largest error over tolerance of a test, per quantity; printed and recorded at the end of the test."""

    def __init__(self, name):
        self.name, self.w = name, {}

    def judge(self, key, got, want, tol, what):
        got, want, tol = (np.asarray(x, np.float64) for x in (got, want, tol))
        assert got.shape == want.shape == tol.shape, (what, got.shape, want.shape, tol.shape)
        assert np.isfinite(got).all(), f"{what}: {int((~np.isfinite(got)).sum())} of {got.size} elements unwritten or not finite"
        err = np.abs(got - want)
        ratio = np.where(tol > 0, err / np.where(tol > 0, tol, 1.0), np.where(err == 0, 0.0, np.inf))
        worst = float(ratio.max()) if ratio.size else 0.0
        self.w[key] = max(self.w.get(key, 0.0), worst)
        if worst > 1.0:
            print(f"{self.name} {what}: largest error {worst:.3f} of its tolerance")
        i = np.unravel_index(int(np.argmax(ratio)), ratio.shape)
        assert worst <= 1.0, f"{what}: element {i} off by {err[i]:.3e}, tolerance {tol[i]:.3e} (got {got[i]!r}, float64 {want[i]!r})"

    def done(self):
        print(f"{self.name}: largest error over tolerance " + ", ".join(f"{k} {v:.3f}" for k, v in self.w.items()))
        record_stats(f"value_loss_{self.name}", {"worst_error_over_tolerance": self.w})


def _smooth32(d):
    """The kernels' fp32 loss and clamp of an fp32 d, operation by operation."""
    d = np.asarray(d, np.float32)
    ad = np.abs(d)
    return np.where(ad < 1, (np.float32(0.5) * d) * d, ad - np.float32(0.5)).astype(np.float32), np.clip(d, np.float32(-1), np.float32(1))


# ------------------------------------------------------------------------------------------------ a0_loss_dqn
@pytest.mark.parametrize("A", V.DQN_AS)
@pytest.mark.parametrize("B", V.LOSS_BS)
def test_dqn_loss_against_float64(hip, B, A):
    W = Worst(f"dqn_b{B}_a{A}")
    rows = np.arange(B)
    for variant in range(len(V.DQN_PLAN) if B == 1 else 1):
        c = V.dqn_case(B, A, variant)
        loss, dq, st = _out(hip, B), _out(hip, B * A), _flag(hip)
        hip.loss_dqn(_dev(hip, c["q"]), _dev(hip, c["q_next"]), A, _dev(hip, c["act"]), _dev(hip, c["a_star"]), _dev(hip, c["rew"]), _dev(hip, c["done"]),
                     _dev(hip, c["wgt"]), V.GAMMA, B, loss, dq, st)
        got_l, got_g, flag = _take(loss, B, "loss"), _take(dq, B * A, "dq").reshape(B, A), _take(st, 8, "state")
        ref = V.dqn64(c["q"], c["q_next"], A, c["act"], c["a_star"], c["rew"], c["done"], c["wgt"], V.GAMMA, B)
        tl, tg = V.dqn_bounds(ref, c["wgt"])
        W.judge("loss", got_l, ref["loss"], tl, "loss")
        W.judge("dq", got_g[rows, c["act"]], ref["dq"][rows, c["act"]], tg, "dq at the taken action")
        off = np.ones((B, A), bool)
        off[rows, c["act"]] = False
        _zero_bits(got_g[off], "dq away from the taken action")
        assert not flag.any(), f"status words {flag}"
        # done = 1: y is the reward bit for bit, so loss and dq are the fp32 formulas of q - r
        on = c["done"] == 1
        if on.any():
            l32, s32 = _smooth32(c["q"][rows, c["act"]][on] - c["rew"][on])
            _same_bits(got_l[on], l32, "loss of done rows")
            _same_bits(got_g[rows, c["act"]][on], c["wgt"][on] * s32, "dq of done rows")
        w0 = c["wgt"] == 0
        assert (got_g[w0] == 0).all()
    W.done()


# ------------------------------------------------------------------------------------------------ a0_dqn_head_loss
def _run_head(hip, c, ld, with_q_tg):
    B, A, NQ = c["B"], c["A"], c["NQ"]
    loss, q_on, draw, st = _out(hip, B), _out(hip, B * A), _out(hip, B * ld), _flag(hip)
    q_tg = _out(hip, B * A) if with_q_tg else None
    hip.dqn_head_loss(_dev(hip, c["h_on"]), _dev(hip, c["h_tg"]), None if c["h_sel"] is None else _dev(hip, c["h_sel"]), _dev(hip, c["W_on"]), _dev(hip, c["b_on"]),
                      _dev(hip, c["W_tg"]), _dev(hip, c["b_tg"]), A, c["dueling"], ld, _dev(hip, c["act"]), _dev(hip, c["rew"]), _dev(hip, c["done"]), _dev(hip, c["wgt"]),
                      c["gamma_n"], B, loss, q_on, q_tg, draw, st)
    return (_take(loss, B, "loss"), _take(q_on, B * A, "q_on").reshape(B, A), _take(q_tg, B * A, "q_tg").reshape(B, A) if with_q_tg else None,
            _take(draw, B * ld, "draw").reshape(B, ld), _take(st, 8, "state"))


@pytest.mark.parametrize("with_sel", [0, 1], ids=["single_q", "double_q"])
@pytest.mark.parametrize("A,dueling", V.HEAD_HEADS)
def test_dqn_head_loss_against_float64(hip, A, dueling, with_sel):
    """q_on, q_tg, loss and draw against util.qhead64 and the reference loss.  The greedy action shows in the loss: where the online network selects (double-Q)
    its rows tie_pair(A) are bit-identical and the target's are not, so the later of the two equal maxima would bring another target value."""
    W = Worst(f"head_a{A}_d{dueling}_sel{with_sel}")
    NQ = A + dueling
    for B in V.HEAD_BS:
        c0 = V.head_case(B, A, dueling, with_sel)
        for ld, with_q_tg in ((NQ, True), (32, False)) + (((32, True), (NQ, False)) if B == 5 else ()):
            c = dict(c0, ld=ld)
            ref = V.head_loss64(c)
            got_l, got_qo, got_qt, got_d, flag = _run_head(hip, c, ld, with_q_tg)
            what = f"B={B} ld={ld}"
            W.judge("q_on", got_qo, ref["q_on"], ref["t_on"], f"q_on, {what}")
            if with_q_tg:
                W.judge("q_tg", got_qt, ref["q_tg"], ref["t_tg"], f"q_tg, {what}")
            W.judge("loss", got_l, ref["loss"], ref["tol_loss"], f"loss, {what}")
            W.judge("draw", got_d, ref["draw"], ref["tol_draw"], f"draw, {what}")
            _zero_bits(got_d[:, NQ:], "draw's pad columns")
            rows = np.arange(B)
            if not dueling:
                off = np.ones((B, A), bool)
                off[rows, c["act"]] = False
                _zero_bits(got_d[:, :A][off], "draw away from the taken action")
            else:
                # <combine(raw), dq> = <raw, draw>: the value column holds g itself (the sum of g and zeros); raw in float64
                g = got_d[:, A].astype(np.float64)
                raw, _ = V.head64(c["h_on"], c["W_on"], c["b_on"], NQ, 0)
                lhs = got_qo[rows, c["act"]].astype(np.float64) * g
                rhs = (raw * got_d[:, :NQ].astype(np.float64)).sum(1)
                share = np.full((B, A), 1.0 / A)
                share[rows, c["act"]] += 1.0
                bound = ref["t_on"][rows, c["act"]] * np.abs(g) + 2 * U * np.abs(g) * (share * np.abs(raw[:, :A])).sum(1) + 1e-300
                W.w["transpose"] = max(W.w.get("transpose", 0.0), float((np.abs(lhs - rhs) / bound).max()))
                assert (np.abs(lhs - rhs) <= bound).all(), f"<fwd(x), g> = {lhs}, <x, bwd(g)> = {rhs}, bound {bound}"
            assert (got_d[c["wgt"] == 0] == 0).all()
            assert not flag.any(), f"status words {flag}"
    W.done()


# ------------------------------------------------------------------------------------------------ a0_loss_mdqn
@pytest.mark.parametrize("tau", V.MDQN_TAUS)
@pytest.mark.parametrize("A", V.MDQN_AS)
@pytest.mark.parametrize("B", V.LOSS_BS)
def test_munchausen_loss_against_float64(hip, B, A, tau):
    W = Worst(f"mdqn_b{B}_a{A}_tau{tau}")
    rows = np.arange(B)
    for variant in range(7 if B == 1 else 1):
        c = V.mdqn_case(B, A, tau, variant)
        loss, dq, st = _out(hip, B), _out(hip, B * A), _flag(hip)
        hip.loss_mdqn(_dev(hip, c["q"]), _dev(hip, c["q_next"]), _dev(hip, c["q_cur"]), A, _dev(hip, c["act"]), _dev(hip, c["rew"]), _dev(hip, c["done"]),
                      _dev(hip, c["wgt"]), V.GAMMA, tau, c["lo"], B, loss, dq, st)
        got_l, got_g, flag = _take(loss, B, "loss"), _take(dq, B * A, "dq").reshape(B, A), _take(st, 8, "state")
        ref = V.mdqn64(c["q"], c["q_next"], c["q_cur"], A, c["act"], c["rew"], c["done"], c["wgt"], V.GAMMA, tau, c["lo"], B)
        tl, tg = V.mdqn_bounds(ref, c["wgt"])
        W.judge("loss", got_l, ref["loss"], tl, "loss")
        W.judge("dq", got_g[rows, c["act"]], ref["dq"][rows, c["act"]], tg, "dq at the taken action")
        off = np.ones((B, A), bool)
        off[rows, c["act"]] = False
        _zero_bits(got_g[off], "dq away from the taken action")
        assert not flag.any(), f"status words {flag}"
    W.done()


# ------------------------------------------------------------------------------------------------ a0_loss_c51
def _run_c51(hip, rows, A, T, vmin, vmax, gam, with_m):
    B = len(rows["kinds"])
    loss, dl, st = _out(hip, B), _out(hip, B * A * T), _flag(hip)
    m = _out(hip, B * T) if with_m else None
    hip.loss_c51(_dev(hip, rows["logits"]), _dev(hip, rows["tgt_logits"]), A, T, _dev(hip, rows["act"]), _dev(hip, rows["a_star"]), _dev(hip, rows["rew"]),
                 _dev(hip, rows["done"]), _dev(hip, rows["wgt"]), _dev(hip, rows["atoms"]), gam, vmin, vmax, B, loss, dl, m, st)
    return _take(loss, B, "loss"), _take(dl, B * A * T, "dlogits").reshape(B, A, T), _take(m, B * T, "m").reshape(B, T) if with_m else None, _take(st, 8, "state")


def _ref_c51(rows, A, T, vmin, vmax, gam):
    return V.c51_64(rows["logits"], rows["tgt_logits"], A, T, rows["act"], rows["a_star"], rows["rew"], rows["done"], rows["wgt"], rows["atoms"], gam, vmin, vmax,
                    len(rows["kinds"]))


def _judge_c51(W, rows, ref, got_l, got_dl, got_m, A, keep=None):
    B = len(rows["kinds"])
    keep = np.ones(B, bool) if keep is None else keep
    r = np.arange(B)
    if got_m is not None:
        W.judge("m", got_m[keep], ref["m"][keep], ref["tol_m"][keep], f"projected distribution {rows['kinds']}")
        W.judge("mass", got_m[keep].astype(np.float64).sum(-1), ref["mass"][keep], ref["tol_mass"][keep], f"mass {rows['kinds']}")
        assert (got_m[keep] >= 0).all()
    W.judge("loss", got_l[keep], ref["loss"][keep], ref["tol_loss"][keep], f"loss {rows['kinds']}")
    W.judge("dlogits", got_dl[r, rows["act"]][keep], ref["g"][keep], ref["tol_g"][keep], f"dlogits at the taken action {rows['kinds']}")
    off = np.ones(got_dl.shape[:2], bool)
    off[r, rows["act"]] = False
    _zero_bits(got_dl[off], "dlogits away from the taken action")
    assert (got_dl[(rows["wgt"] == 0) & keep] == 0).all()


@pytest.mark.parametrize("A", V.C51_AS)
@pytest.mark.parametrize("T", V.C51_TS)
def test_categorical_loss_against_float64(hip, T, A):
    """Every support and gamma_n, B = 5 and 1, the twelve kinds of row of value_loss_ref.C51_KINDS, m_out given and null."""
    W = Worst(f"c51_t{T}_a{A}")
    for vmin, vmax, gam, with_m, rows in V.c51_launches(T, A):
        got_l, got_dl, got_m, flag = _run_c51(hip, rows, A, T, vmin, vmax, gam, with_m)
        _judge_c51(W, rows, _ref_c51(rows, A, T, vmin, vmax, gam), got_l, got_dl, got_m, A)
        assert not flag.any(), f"status words {flag}"
    W.done()


@pytest.mark.parametrize("vmin,vmax,T", V.FINDING)
def test_projection_keeps_its_mass_where_the_rounded_delta_puts_vmax_above_the_last_bin(hip, vmin, vmax, T):
    """fl32(delta) lies below the exact width at these supports: (vmax - vmin) / fl32(delta) = T - 1 + an ulp, and floor / ceil of it would send the atom's upper
    share to bin T, which no lane gathers: that share of the mass (4e-6 of p) used to vanish.  Row 1's target is one atom at probability 1, where the bound on
    the mass is 1e-6.  The position is held to T - 1: every index lies in [0, T) and the mass is whole."""
    W = Worst(f"c51_finding_t{T}_{vmin}_{vmax}")
    A = 2
    rows = V.c51_rows(("clamp_high", "tgt_peak", "binlast"), T, A, vmin, vmax, 9)
    rows["rew"][1] = vmax + 2 * (vmax - vmin)                    # clamps every atom, like row 0
    got_l, got_dl, got_m, flag = _run_c51(hip, rows, A, T, vmin, vmax, 0.99, True)
    ref = _ref_c51(rows, A, T, vmin, vmax, 0.99)
    _judge_c51(W, rows, ref, got_l, got_dl, got_m, A)
    assert (got_m[:, :T - 1] == 0).all() and (got_m[:, T - 1] > 0).all(), "every atom of these rows lands in the last bin"
    assert not flag.any()
    W.done()


def test_a_nan_reward_sets_the_flag_and_stays_in_its_sample(hip):
    T, A, vmin, vmax, gam = 51, 4, -10.0, 10.0, 0.99
    W = Worst("c51_nan")
    rows = V.c51_rows(V.C51_KINDS[7:12], T, A, vmin, vmax, 21)
    rows["rew"][2] = np.nan
    got_l, got_dl, got_m, flag = _run_c51(hip, rows, A, T, vmin, vmax, gam, True)
    assert int(flag[0]) == 1 and not flag[1:].any(), f"status words {flag}"
    assert np.isnan(got_l[2]) and int(np.isnan(got_l).sum()) == 1, "the NaN stays in its sample's loss"
    keep = np.arange(5) != 2
    assert np.isfinite(got_m[keep]).all() and np.isfinite(got_dl[keep]).all()
    clean = dict(rows, rew=np.where(keep, rows["rew"], 0).astype(np.float32))
    _judge_c51(W, rows, _ref_c51(clean, A, T, vmin, vmax, gam), got_l, got_dl, got_m, A, keep=keep)
    W.done()


# ------------------------------------------------------------------------------------------------ logf
def test_logf_error_stays_within_the_recorded_figure(hip):
    """logf alone, read out of a0_loss_c51.  T = n + 1 atoms, online logits (0, ..., 0, -c): the softmax's denominator is s = n + expf(-c) summed by the
    butterfly, anywhere in [n, n + 1].  The target is one-hot at atom 0 (logits 0 and -200: probabilities exactly 1 and 0) and the sample terminal with
    r = vmin, so the projected distribution is exactly (1, 0, ..., 0) and the loss exactly logf(s).  s itself is pinned down by the gradient: with w = 1,
    dlogits[1] = fl(1 / s) and dlogits[n] = fl(expf(-c) / s) (n = 1: dlogits[0] = fl(1 / s) - 1); of the fp32 neighbours of exp(-c) those are kept that
    reproduce both, in the butterfly's order of additions, and an argument is used if they agree on s (nearly all do).  n = 1 ... 63, 1600 values of c each:
    1e5 arguments over [1, 64].  Measured on an MI355X: 6.187e-7 at s = 62.238 (1.3 ulp of log s) over the 99 700 of 100 800 arguments whose s is pinned down,
    recorded as LOGF_MEASURED = 6.2e-7 (value_loss_ref.py, profiles/r12_value_loss_accuracy.md); asserted: LOGF_BOUND = 2^-19 (1.9e-6), twice the figure (1.24e-6)
    rounded up to a power of two."""
    vmin, vmax, Bn = -10.0, 10.0, 1600
    g = recipe.gen(12)
    worst, used, total, where = 0.0, 0, 0, None
    for n in range(1, 64):
        T = n + 1
        c = (-np.log(g.uniform(2e-7, 1.0, Bn))).astype(np.float32)
        x = np.zeros((Bn, 1, T), np.float32)
        x[:, 0, n] = -c
        xt = np.full((Bn, 1, T), -200.0, np.float32)
        xt[:, 0, 0] = 0.0
        rows = dict(logits=x, tgt_logits=xt, act=np.zeros(Bn, np.int32), a_star=np.zeros(Bn, np.int32), rew=np.full(Bn, vmin, np.float32), done=np.ones(Bn, np.float32),
                    wgt=np.ones(Bn, np.float32), atoms=V.c51_atoms(vmin, vmax, T), kinds=(None,) * Bn)
        got_l, got_dl, got_m, flag = _run_c51(hip, rows, 1, T, vmin, vmax, 0.99, True)
        assert not flag.any()
        onehot = np.zeros((Bn, T), np.float32)
        onehot[:, 0] = 1.0
        _same_bits(got_m, onehot, "the projected distribution of a one-hot target at a terminal with r = vmin")
        gl = got_dl[:, 0]
        # candidates for expf(-c): the fp32 neighbours of exp(-c), four either side
        e1 = np.exp(-c.astype(np.float64)).astype(np.float32)
        cand = [e1]
        for _ in range(4):
            cand = [np.nextafter(cand[0], np.float32(0))] + cand + [np.nextafter(cand[-1], np.float32(2))]
        cand = np.stack(cand, 1)                                                   # [Bn][9]
        lanes = np.zeros((Bn, cand.shape[1], 64), np.float32)
        lanes[:, :, :n] = 1.0
        lanes[:, :, n] = cand
        s = C._butterfly(lanes)                                                    # [Bn][9], the wave sum in its order of additions
        inv = (np.float32(1) / s).astype(np.float32)
        ok = (cand / s).astype(np.float32) == gl[:, n:n + 1]
        ok &= (inv == gl[:, 1:2]) if n > 1 else ((inv - np.float32(1)).astype(np.float32) == gl[:, 0:1])
        assert ok.any(1).all(), f"n = {n}: no neighbour of exp(-c) reproduces the gradient of {int((~ok.any(1)).sum())} samples"
        s_lo, s_hi = np.where(ok, s, np.inf).min(1), np.where(ok, s, -np.inf).max(1)
        sure = s_lo == s_hi
        err = np.abs(got_l.astype(np.float64) - np.log(s_lo.astype(np.float64)))[sure]
        total, used = total + Bn, used + int(sure.sum())
        if err.size and err.max() > worst:
            worst, where = float(err.max()), float(s_lo[sure][int(err.argmax())])
    print(f"logf: largest |logf(s) - log(s)| {worst:.4e} at s = {where!r} over {used} of {total} arguments in [1, 64]; recorded {LOGF_MEASURED:.2e}, "
          f"bound {LOGF_BOUND:.4e}: {worst / LOGF_BOUND:.3f} of its tolerance")
    record_stats("value_loss_logf", {"largest_abs_error": worst, "at": where, "arguments_used": used, "arguments": total, "recorded": LOGF_MEASURED, "bound": LOGF_BOUND})
    assert used >= 0.95 * total, f"only {used} of {total} arguments pinned down"
    assert worst <= LOGF_BOUND, f"logf deviates by {worst:.3e} from the float64 logarithm of its fp32 argument (bound {LOGF_BOUND:.3e})"


# ------------------------------------------------------------------------------------------------ the fused C51 kernel at the new edges
@pytest.mark.parametrize("A", [1, 18])
@pytest.mark.parametrize("T", [2, 33, 64])
def test_c51_head_loss_from_slabs_equals_the_separate_kernels_at_the_edges(hip, T, A):
    """a0_c51_head_loss_slabs against slab sums in slab order + bias, a0_dueling_fwd x3, a0_select_action, a0_loss_c51, a0_dueling_bwd, every output bit for bit
    (tests/test_gpu_engine.py::test_c51_head_loss_from_slabs_equals_the_separate_kernels at T = 51, 11, 64 and B >= 9): T = 2, 33, 64, one action and eighteen
    (dueling), B around the four samples of a workgroup, 1, 4 and 5 slabs, with and without the online network's s' rows (double-Q)."""
    dueling = A == 18
    NQ = A + (1 if dueling else 0)
    ld = (NQ * T + 31) // 32 * 32
    atoms = torch.linspace(-10.0, 10.0, T).to(hip.device)
    for B in (1, 3, 4, 5):
        for ns_on, ns_tg in ((1, 4), (4, 5), (5, 1)):
            for double_q in (False, True):
                g = recipe.gen(1000 * A + 10 * T + B + ns_on)
                R_on = 2 * B if double_q else B
                s_on = _dev(hip, g.standard_normal((ns_on, R_on, ld)).astype(np.float32)).reshape(ns_on, R_on, ld)
                s_tg = _dev(hip, g.standard_normal((ns_tg, B, ld)).astype(np.float32)).reshape(ns_tg, B, ld)
                b_on, b_tg = _dev(hip, g.standard_normal(ld).astype(np.float32)), _dev(hip, g.standard_normal(ld).astype(np.float32))
                a, r, d, w = recipe.make_transitions(B, A, 5 + B)
                act, rew, done, wgt = _dev(hip, a.astype(np.int32)), _dev(hip, r), _dev(hip, d.astype(np.float32)), _dev(hip, w)
                st = _flag(hip)
                loss, draw = _out(hip, B), _out(hip, B * ld)
                q_on, q_tg, m_out, a_star = _out(hip, B * A * T), _out(hip, B * A * T), _out(hip, B * T), _out(hip, B, fill=-1, dtype=torch.int32)
                hip.c51_head_loss_slabs(s_on.reshape(-1), ns_on, R_on, s_tg.reshape(-1), ns_tg, B if double_q else -1, b_on, b_tg, ld, A, T, dueling, act, rew, done, wgt,
                                        atoms, 0.97, -10.0, 10.0, B, loss, draw, st, q_on=q_on, q_tg=q_tg, m_out=m_out, a_star=a_star)

                def reduce(slabs, bias):
                    acc = torch.zeros_like(slabs[0])
                    for z in range(slabs.shape[0]):
                        acc = acc + slabs[z]                # slab order
                    return (acc + bias).contiguous()

                raw_on, raw_tg = reduce(s_on, b_on), reduce(s_tg, b_tg)
                q1, q2, q3 = hip.empty(B * A * T), hip.empty(B * A * T), hip.empty(B * A * T)
                hip.dueling_fwd(raw_on[:B].reshape(-1), ld, q1, B, A, T, dueling)
                hip.dueling_fwd(raw_tg.reshape(-1), ld, q2, B, A, T, dueling)
                a2 = hip.zeros(B, dtype=torch.int32)
                if double_q:
                    hip.dueling_fwd(raw_on[B:].reshape(-1).contiguous(), ld, q3, B, A, T, dueling)
                    hip.select_action(q3, A * T, T, 1, B, A, T, 2, atoms, a2, None, None)
                else:
                    hip.select_action(q2, A * T, T, 1, B, A, T, 2, atoms, a2, None, None)
                loss2, dq2, m2, draw2, st2 = hip.empty(B), hip.zeros(B * A * T), hip.empty(B * T), hip.empty(B * ld), hip.zeros(8, dtype=torch.int32)
                hip.loss_c51(q1, q2, A, T, act, a2, rew, done, wgt, atoms, 0.97, -10.0, 10.0, B, loss2, dq2, m2, st2)
                hip.dueling_bwd(dq2, draw2, ld, B, A, T, dueling)
                what = f"B={B} slabs={ns_on}/{ns_tg} double_q={double_q}"
                _same_bits(_take(q_on, B * A * T, "q_on"), q1.cpu().numpy(), f"online logits, {what}")
                _same_bits(_take(q_tg, B * A * T, "q_tg"), q2.cpu().numpy(), f"target logits, {what}")
                assert np.array_equal(_take(a_star, B, "a_star"), a2.cpu().numpy()), f"greedy next action, {what}"
                _same_bits(_take(m_out, B * T, "m_out"), m2.cpu().numpy(), f"projected distribution, {what}")
                _same_bits(_take(loss, B, "loss"), loss2.cpu().numpy(), f"loss, {what}")
                _same_bits(_take(draw, B * ld, "draw"), draw2.cpu().numpy(), f"draw, {what}")
                assert not _take(st, 8, "state").any() and int(st2[0]) == 0


# ------------------------------------------------------------------------------------------------ argument checks
def _untouched(bufs):
    torch.cuda.synchronize()
    for name, (buf, n) in bufs.items():
        got = _take(buf, n, name)
        assert np.isnan(got).all() if buf.dtype == torch.float32 else not got.any(), f"{name} was written by a call that returned an error"


def test_bad_arguments_return_their_error_and_write_nothing(hip):
    from agent0_amd._abi import A0Error
    g = recipe.gen(3)
    B, A = 3, 2
    z = lambda n: _dev(hip, g.standard_normal(n).astype(np.float32))
    iz = lambda n: hip.zeros(n, dtype=torch.int32)
    for T in (1, 65):
        n = B * A * 65
        bufs = dict(loss=(_out(hip, B), B), dlogits=(_out(hip, n), n), m=(_out(hip, B * 65), B * 65), state=(_flag(hip), 8))
        with pytest.raises(A0Error, match="a0_loss_c51"):
            hip.loss_c51(z(n), z(n), A, T, iz(B), iz(B), z(B), iz(B).float(), z(B), z(65), 0.99, -10.0, 10.0, B, bufs["loss"][0], bufs["dlogits"][0], bufs["m"][0],
                         bufs["state"][0])
        _untouched(bufs)
    for A_, dueling, ld in ((25, 0, 32), (24, 1, 32), (4, 1, 4), (4, 0, 3)):          # NQ = 25 both ways; ld < NQ both ways
        nq = A_ + dueling
        bufs = dict(loss=(_out(hip, B), B), q_on=(_out(hip, B * A_), B * A_), q_tg=(_out(hip, B * A_), B * A_), draw=(_out(hip, B * 32), B * 32), state=(_flag(hip), 8))
        with pytest.raises(A0Error, match="a0_dqn_head_loss"):
            hip.dqn_head_loss(z(B * 512), z(B * 512), None, z(nq * 512), z(nq), z(nq * 512), z(nq), A_, dueling, ld, iz(B), z(B), iz(B).float(), z(B), 0.99, B,
                              bufs["loss"][0], bufs["q_on"][0], bufs["q_tg"][0], bufs["draw"][0], bufs["state"][0])
        _untouched(bufs)
    bufs = dict(loss=(_out(hip, B), B), dq=(_out(hip, B * A), B * A), state=(_flag(hip), 8))
    with pytest.raises(A0Error, match="a0_loss_mdqn"):
        hip.loss_mdqn(z(B * A), z(B * A), z(B * A), A, iz(B), z(B), iz(B).float(), z(B), 0.99, 0.0, -1.0, B, bufs["loss"][0], bufs["dq"][0], bufs["state"][0])
    _untouched(bufs)
