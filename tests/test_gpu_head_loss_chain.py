"""GPU (MI355X): a0_dqn_head_loss_slabs / a0_mdqn_head_loss_slabs (one launch from fc1's split-K slabs to the loss, the head gradient and the head's data gradient)
against the launches it stands for, every output buffer as bit patterns:

    a0_reduce_bias_act (slab sums in slab order + bias + ReLU)  ->  h
    a0_dqn_head_loss (the same fmaf chain over 512 columns, a0_wave_sum, first maximum, dueling arithmetic)  ->  q, loss, draw, the NaN flag
    a0_dense_dgrad with the ReLU mask h  ->  dh, on the fp32 fmaf-chain GEMM (a0_gemm_mode 0): dh[k] = fmaf chain over the head's rows in ascending order, which is
    what the fused kernel computes; the split-operand GEMM of the default mode sums six bf16 cross products and agrees to rounding only

at the edges of the kernel's work split: B around its four samples per workgroup, slab counts around its trips of four slabs, one action, the widest head
(A + dueling = 24 both ways: 23 actions with the value stream, 24 without)."""
import numpy as np
import pytest
import torch

import recipe

pytestmark = pytest.mark.gpu

BS = [1, 3, 4, 5, 9]
NSLABS = [1, 3, 4, 5, 8]
LD = 32
GAMMA = 0.97


@pytest.fixture(scope="module")
def hip():
    from agent0_amd.ops import HipOps
    return HipOps()


def D(hip, x):
    return torch.from_numpy(np.ascontiguousarray(x)).to(hip.device)


def bits(t):
    return t.contiguous().view(torch.int32)


def same(a, b):
    return torch.equal(bits(a), bits(b))


def inputs(hip, A, B, ns, seed):
    g = recipe.gen(seed)
    s = [D(hip, (g.standard_normal((ns, B, 512)) * 0.5).astype(np.float32)).reshape(-1) for _ in range(3)]
    b1 = [D(hip, (g.standard_normal(512) * 0.3).astype(np.float32)) for _ in range(2)]
    W = [D(hip, (g.standard_normal((LD, 512)) * 0.05).astype(np.float32)).reshape(-1) for _ in range(2)]
    b = [D(hip, (g.standard_normal(LD) * 0.1).astype(np.float32)) for _ in range(2)]
    a, r, d, w = recipe.make_transitions(B, A, seed + 1)
    return s, b1, W, b, a.astype(np.int32), r, d.astype(np.float32), w


def fc1(hip, slabs, ns, bias, B):
    out = hip.empty(B * 512)
    hip.reduce_bias_act_multi([(slabs, ns, bias, out, B)], 512, True)
    return out


def dgrad_chain(hip, draw, W_on, h, B):
    """a0_dense_dgrad with the ReLU mask on the fp32 fmaf-chain GEMM; also the default mode's largest difference, for the record."""
    dh, dh_x = hip.empty(B * 512), hip.empty(B * 512)
    hip.dense_dgrad(draw, W_on, h, dh_x, B, LD, 512)
    prev = hip.gemm_mode(0)
    try:
        hip.dense_dgrad(draw, W_on, h, dh, B, LD, 512)
    finally:
        hip.gemm_mode(prev)
    return dh, dh_x


@pytest.mark.parametrize("A,dueling", [(1, False), (1, True), (4, False), (4, True), (18, False), (18, True), (23, True), (24, False)])
def test_dqn_head_loss_from_slabs_is_the_unfused_composition_bit_for_bit(hip, A, dueling):
    worst = 0.0
    for B in BS:
        for ns in NSLABS:
            for double_q in (False, True):
                s, b1, W, b, a, r, d, w = inputs(hip, A, B, ns, 31 * A + 7 * B + ns)
                act, rew, done, wgt = D(hip, a), D(hip, r), D(hip, d), D(hip, w)
                st1, st2 = hip.zeros(8, dtype=torch.int32), hip.zeros(8, dtype=torch.int32)
                nan = float("nan")
                loss, q_on, q_tg = hip.empty(B).fill_(nan), hip.empty(B * A).fill_(nan), hip.empty(B * A).fill_(nan)
                draw, dh, h = hip.empty(B * LD).fill_(nan), hip.empty(B * 512).fill_(nan), hip.empty(B * 512).fill_(nan)
                hip.dqn_head_loss_slabs(s[0], s[1], s[2] if double_q else None, ns, b1[0], b1[1], h, W[0], b[0], W[1], b[1], A, dueling, LD, act, rew, done, wgt, GAMMA, B,
                                        loss, q_on, q_tg, draw, st1, dh)
                h_on, h_tg = fc1(hip, s[0], ns, b1[0], B), fc1(hip, s[1], ns, b1[1], B)
                h_sel = fc1(hip, s[2], ns, b1[0], B) if double_q else None
                loss2, q_on2, q_tg2, draw2 = hip.empty(B), hip.empty(B * A), hip.empty(B * A), hip.empty(B * LD)
                hip.dqn_head_loss(h_on, h_tg, h_sel, W[0], b[0], W[1], b[1], A, dueling, LD, act, rew, done, wgt, GAMMA, B, loss2, q_on2, q_tg2, draw2, st2)
                dh2, dh_x = dgrad_chain(hip, draw2, W[0], h_on, B)
                what = f"B={B} nslab={ns} double_q={double_q}"
                worst = max(worst, float((dh - dh_x).abs().max()) / max(float(dh_x.abs().max()), 1e-30))
                assert same(h, h_on), f"h, {what}"
                assert same(q_on, q_on2) and same(q_tg, q_tg2), f"q, {what}"
                assert same(loss, loss2), f"loss, {what}"
                assert same(draw, draw2), f"draw, {what}"
                assert same(dh, dh2), f"dh, {what}: {int((bits(dh) != bits(dh2)).sum())} of {B * 512} differ, max {float((dh - dh2).abs().max())}"
                assert int(st1[0]) == 0 and int(st2[0]) == 0, f"NaN flag, {what}"
    print(f"A={A} dueling={dueling}: dh against the split-operand a0_dense_dgrad differs by at most {worst:.2e} of its scale")


@pytest.mark.parametrize("A,dueling", [(1, False), (1, True), (4, False), (4, True), (18, False), (18, True), (23, True), (24, False)])
def test_mdqn_head_loss_from_slabs_is_the_unfused_composition_bit_for_bit(hip, A, dueling):
    """The Munchausen form: the third pass is the TARGET network on the current observation.  h, and the three heads' q values against a0_dqn_head_loss's (the same
    chain); loss and draw against a0_loss_mdqn + a0_dueling_bwd on those q values; dh against a0_dense_dgrad."""
    tau, lo = 0.03, -1.0
    for B in BS:
        for ns in NSLABS:
            s, b1, W, b, a, r, d, w = inputs(hip, A, B, ns, 57 * A + 5 * B + ns)
            act, rew, done, wgt = D(hip, a), D(hip, r), D(hip, d), D(hip, w)
            st1, st2 = hip.zeros(8, dtype=torch.int32), hip.zeros(8, dtype=torch.int32)
            nan = float("nan")
            loss, draw, dh, h = hip.empty(B).fill_(nan), hip.empty(B * LD).fill_(nan), hip.empty(B * 512).fill_(nan), hip.empty(B * 512).fill_(nan)
            q_on, q_tg, q_cur = hip.empty(B * A).fill_(nan), hip.empty(B * A).fill_(nan), hip.empty(B * A).fill_(nan)
            hip.mdqn_head_loss_slabs(s[0], s[1], s[2], ns, b1[0], b1[1], h, W[0], b[0], W[1], b[1], A, dueling, LD, act, rew, done, wgt, GAMMA, tau, lo, B, loss, q_on, q_tg,
                                     q_cur, draw, st1, dh)
            h_on, h_tg, h_cur = fc1(hip, s[0], ns, b1[0], B), fc1(hip, s[1], ns, b1[1], B), fc1(hip, s[2], ns, b1[1], B)
            scr_l, scr_d, scr_q = hip.empty(B), hip.empty(B * LD), hip.empty(B * A)
            q_on2, q_tg2, q_cur2 = hip.empty(B * A), hip.empty(B * A), hip.empty(B * A)
            hip.dqn_head_loss(h_on, h_tg, None, W[0], b[0], W[1], b[1], A, dueling, LD, act, rew, done, wgt, GAMMA, B, scr_l, q_on2, q_tg2, scr_d, st2)
            hip.dqn_head_loss(h_on, h_cur, None, W[0], b[0], W[1], b[1], A, dueling, LD, act, rew, done, wgt, GAMMA, B, scr_l, scr_q, q_cur2, scr_d, st2)
            loss2, dq2, draw2 = hip.empty(B), hip.zeros(B * A), hip.empty(B * LD)
            st3 = hip.zeros(8, dtype=torch.int32)
            hip.loss_mdqn(q_on2, q_tg2, q_cur2, A, act, rew, done, wgt, GAMMA, tau, lo, B, loss2, dq2, st3)
            hip.dueling_bwd(dq2, draw2, LD, B, A, 1, dueling)
            dh2, _ = dgrad_chain(hip, draw2, W[0], h_on, B)
            what = f"B={B} nslab={ns}"
            assert same(h, h_on), f"h, {what}"
            assert same(q_on, q_on2) and same(q_tg, q_tg2) and same(q_cur, q_cur2), f"q, {what}"
            assert same(loss, loss2), f"loss, {what}"
            assert same(draw, draw2), f"draw, {what}"
            assert same(dh, dh2), f"dh, {what}: {int((bits(dh) != bits(dh2)).sum())} of {B * 512} differ, max {float((dh - dh2).abs().max())}"
            assert int(st1[0]) == 0 and int(st3[0]) == 0, f"NaN flag, {what}"


@pytest.mark.parametrize("dueling", [False, True])
def test_a_nan_reward_sets_the_flag_and_stays_in_its_sample(hip, dueling):
    A, B, ns = 4, 5, 4
    s, b1, W, b, a, r, d, w = inputs(hip, A, B, ns, 99)
    r[2] = np.nan
    act, rew, done, wgt = D(hip, a), D(hip, r), D(hip, d), D(hip, w)
    st1, st2 = hip.zeros(8, dtype=torch.int32), hip.zeros(8, dtype=torch.int32)
    loss, q_on, q_tg, draw, dh, h = hip.empty(B), hip.empty(B * A), hip.empty(B * A), hip.empty(B * LD), hip.empty(B * 512), hip.empty(B * 512)
    hip.dqn_head_loss_slabs(s[0], s[1], s[2], ns, b1[0], b1[1], h, W[0], b[0], W[1], b[1], A, dueling, LD, act, rew, done, wgt, GAMMA, B, loss, q_on, q_tg, draw, st1, dh)
    h_on, h_tg, h_sel = fc1(hip, s[0], ns, b1[0], B), fc1(hip, s[1], ns, b1[1], B), fc1(hip, s[2], ns, b1[0], B)
    loss2, q_on2, q_tg2, draw2 = hip.empty(B), hip.empty(B * A), hip.empty(B * A), hip.empty(B * LD)
    hip.dqn_head_loss(h_on, h_tg, h_sel, W[0], b[0], W[1], b[1], A, dueling, LD, act, rew, done, wgt, GAMMA, B, loss2, q_on2, q_tg2, draw2, st2)
    dh2, _ = dgrad_chain(hip, draw2, W[0], h_on, B)
    assert int(st1[0]) == 1 and int(st2[0]) == 1, "the NaN flag"
    assert same(h, h_on) and same(q_on, q_on2) and same(q_tg, q_tg2)
    # (a NaN's sign and payload are not part of the contract: NaN in the same places, every other value bit for bit)
    for got, want, name in ((loss, loss2, "loss"), (draw, draw2, "draw"), (dh, dh2, "dh")):
        assert torch.equal(torch.isnan(got), torch.isnan(want)), name
        assert torch.equal(bits(torch.nan_to_num(got, nan=0.0)), bits(torch.nan_to_num(want, nan=0.0))), name
    assert bool(torch.isnan(loss[2])) and int(torch.isnan(loss).sum()) == 1, "the NaN stays in its sample's loss"


@pytest.mark.parametrize("dueling", [False, True])
def test_a_nan_reward_sets_the_flag_in_the_munchausen_form(hip, dueling):
    A, B, ns, tau, lo = 4, 5, 4, 0.03, -1.0
    s, b1, W, b, a, r, d, w = inputs(hip, A, B, ns, 101)
    r[3] = np.nan
    act, rew, done, wgt = D(hip, a), D(hip, r), D(hip, d), D(hip, w)
    st1, st2, st3 = (hip.zeros(8, dtype=torch.int32) for _ in range(3))
    loss, draw, dh, h = hip.empty(B), hip.empty(B * LD), hip.empty(B * 512), hip.empty(B * 512)
    q_on, q_tg, q_cur = hip.empty(B * A), hip.empty(B * A), hip.empty(B * A)
    hip.mdqn_head_loss_slabs(s[0], s[1], s[2], ns, b1[0], b1[1], h, W[0], b[0], W[1], b[1], A, dueling, LD, act, rew, done, wgt, GAMMA, tau, lo, B, loss, q_on, q_tg, q_cur,
                             draw, st1, dh)
    h_on, h_tg, h_cur = fc1(hip, s[0], ns, b1[0], B), fc1(hip, s[1], ns, b1[1], B), fc1(hip, s[2], ns, b1[1], B)
    scr_l, scr_d, scr_q = hip.empty(B), hip.empty(B * LD), hip.empty(B * A)
    q_on2, q_tg2, q_cur2 = hip.empty(B * A), hip.empty(B * A), hip.empty(B * A)
    hip.dqn_head_loss(h_on, h_tg, None, W[0], b[0], W[1], b[1], A, dueling, LD, act, rew, done, wgt, GAMMA, B, scr_l, q_on2, q_tg2, scr_d, st2)
    hip.dqn_head_loss(h_on, h_cur, None, W[0], b[0], W[1], b[1], A, dueling, LD, act, rew, done, wgt, GAMMA, B, scr_l, scr_q, q_cur2, scr_d, st2)
    loss2, dq2, draw2 = hip.empty(B), hip.zeros(B * A), hip.empty(B * LD)
    hip.loss_mdqn(q_on2, q_tg2, q_cur2, A, act, rew, done, wgt, GAMMA, tau, lo, B, loss2, dq2, st3)
    hip.dueling_bwd(dq2, draw2, LD, B, A, 1, dueling)
    dh2, _ = dgrad_chain(hip, draw2, W[0], h_on, B)
    assert int(st1[0]) == 1 and int(st3[0]) == 1, "the NaN flag"
    assert same(h, h_on) and same(q_on, q_on2) and same(q_tg, q_tg2) and same(q_cur, q_cur2)
    for got, want, name in ((loss, loss2, "loss"), (draw, draw2, "draw"), (dh, dh2, "dh")):
        assert torch.equal(torch.isnan(got), torch.isnan(want)), name
        assert torch.equal(bits(torch.nan_to_num(got, nan=0.0)), bits(torch.nan_to_num(want, nan=0.0))), name
    assert bool(torch.isnan(loss[3])) and int(torch.isnan(loss).sum()) == 1, "the NaN stays in its sample's loss"
