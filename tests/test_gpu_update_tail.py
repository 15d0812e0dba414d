"""GPU (MI355X): the update's tail as one launch (a0_net_encoder_wgrad_tail + a0_update_tail) against today's chain, bit for bit.

Today's chain: a0_net_encoder_wgrad with pending reductions (its last launch sums the slabs into the gradient), then a0_adam_step_sync_wt (Adam with the
bookkeeping folded in, then the weight-copy refresh that commits the step count).  Both worlds start from the same bytes and run five consecutive updates with
target_update_freq = 2 — first step, sync, NaN-skipped + sync, ordinary, NaN-skipped — the NaN flag raised by the loss kernel from a NaN in its input.  After every
update g, the parameters, both moments, the target, every byte of wt and wt_target, the status words, the scalars and the loss ring are compared as bit patterns.

Work split (csrc/optim.hip): a slab segment is served 128 outputs per workgroup on the 16-byte path (eight row groups of slabs z = g, g + 8, ..., four loads in
flight, a 32-stride loop) and 32 outputs on the scalar path; the ranges between segments 1024 / 256 parameters per workgroup.  Edges: slab counts 1, 7, 8, 9, 31,
32, 33, 72, each on both paths; segments that are scalar because of their base, their count or their stride; segment lengths (148, 45) that end inside a workgroup,
so the next workgroup starts on the first float outside; an Adam range with n % 4 != 0 (every path scalar) and one with n_total > n."""
import ctypes as C

import numpy as np
import pytest
import torch

import recipe

pytestmark = pytest.mark.gpu

HP = dict(lr=5e-4, b1=0.9, b2=0.999, eps=1e-2 / 32, tf=2)
KINDS = ["first", "sync", "nan+sync", "ordinary", "nan"]        # what five consecutive updates are with target_update_freq = 2 and the flag up on the 3rd and 5th
# (off, count, slab_stride) inside a 400-float slot of the dense range: 16-byte path, and scalar because of the base, the count, the stride
FORMS = {"vec": (8, 148, 152), "base": (201, 148, 152), "count": (100, 45, 48), "stride": (4, 148, 149)}
CASES = {
    "1v-7b-8v-9c": [(1, "vec"), (7, "base"), (8, "vec"), (9, "count")],
    "1s-7v-8c-9v": [(1, "stride"), (7, "vec"), (8, "count"), (9, "vec")],
    "31v-32s-33v-72b": [(31, "vec"), (32, "stride"), (33, "vec"), (72, "base")],
    "31c-32v-33b-72v": [(31, "count"), (32, "vec"), (33, "base"), (72, "vec")],
}


@pytest.fixture(scope="module")
def hip():
    from agent0_amd.ops import HipOps
    ops = HipOps()
    assert "gfx950" in ops.device_info()[2]
    assert hasattr(ops, "update_tail")
    return ops


def _bits(t):
    return t.view(torch.int32) if t.dtype == torch.float32 else t


class _World:
    """One copy of everything an update's tail touches, laid out conv1 | conv2 | conv3 | dense range | blocks Adam does not own."""

    def __init__(self, hip, C_, n, n_total, seed):
        g = recipe.gen(seed)
        dev = hip.device
        f = lambda k, scale=1.0: torch.from_numpy((g.standard_normal(k) * scale).astype(np.float32)).to(dev)
        self.C, self.n, self.n_total = C_, n, n_total
        self.p, self.t = f(n_total, 0.05), f(n_total, 0.05)
        self.m, self.v = f(n, 1e-3), f(n, 1e-3).abs()
        self.g = hip.empty(n_total + 4)
        self.state = torch.zeros(8, dtype=torch.int32, device=dev)
        self.scal = hip.zeros(4)
        self.ring = hip.zeros(7)
        self.loss = hip.zeros(8)
        self.dq = hip.zeros(8 * 4)
        K1 = 64 * C_
        self.off = [0, 32 * K1 + 32, 32 * K1 + 32 + 64 * 512 + 64]
        self.conv_end = self.off[2] + 64 * 576 + 64
        self.wt, self.wt_t = hip.empty(hip.conv_wt_floats(C_)), hip.empty(hip.conv_wt_floats(C_))
        hip.conv_wt_refresh(self.weights(self.p), C_, self.wt)
        hip.conv_wt_refresh(self.weights(self.t), C_, self.wt_t)

    def weights(self, flat):
        K1, o = 64 * self.C, self.off
        return dict(w1=flat[o[0]:o[0] + 32 * K1], b1=flat[o[0] + 32 * K1:o[1]], w2=flat[o[1]:o[1] + 64 * 512], b2=flat[o[1] + 64 * 512:o[2]],
                    w3=flat[o[2]:o[2] + 64 * 576], b3=flat[o[2] + 64 * 576:self.conv_end])

    def everything(self):
        return dict(g=self.g[:self.n_total], params=self.p, exp_avg=self.m, exp_avg_sq=self.v, target=self.t, wt=self.wt, wt_target=self.wt_t, state=self.state,
                    scalars=self.scal, loss_ring=self.ring)


def _pend(world, segs, slabs):
    from agent0_amd._abi import PendingReduce
    p = PendingReduce()
    p.n = len(segs)
    at = 0
    for k, (nslab, form) in enumerate(segs):
        off, count, stride = FORMS[form]
        s = p.seg[k]
        s.slabs = slabs.data_ptr() + 4 * at
        s.slab_stride, s.nslab, s.count = stride, nslab, count
        s.out = world.g.data_ptr() + 4 * (world.conv_end + 400 * k + off)
        at += (nslab * stride + 3) // 4 * 4
    return p


def _compare_five_updates(hip, shape, B, segs, n_dense, extra, seed):
    C_, H, W = shape
    net = hip.net(C_, H, W)
    dev = hip.device
    gen = recipe.gen(seed)
    f = lambda k: torch.from_numpy(gen.standard_normal(k).astype(np.float32)).to(dev)
    conv_end = 32 * 64 * C_ + 32 + 64 * 512 + 64 + 64 * 576 + 64
    n, n_total = conv_end + n_dense, conv_end + n_dense + extra
    old, new = _World(hip, C_, n, n_total, seed + 1), _World(hip, C_, n, n_total, seed + 1)
    frames = torch.from_numpy(recipe.make_frames(B, 5, shape)).to(dev).reshape(-1).contiguous()
    stride = frames.numel() // B
    act1, act2 = f(B * net.H1 * net.W1 * 32).abs(), f(B * net.H2 * net.W2 * 64).abs()
    d3, d2, d1 = f(B * net.feat), f(B * net.H2 * net.W2 * 64), f(B * net.H1 * net.W1 * 32)
    pend_slabs = f(sum((ns * FORMS[fm][2] + 3) // 4 * 4 for ns, fm in segs) + 4)
    need = hip.encoder_bwd_scratch(net, B)
    act = torch.zeros(8, dtype=torch.int32, device=dev)
    ones = torch.ones(8, device=dev)
    paths = set()
    for u, kind in enumerate(KINDS):
        q, qn = f(32), f(32)
        if kind.startswith("nan"):
            q[4] = float("nan")         # sample 1, the action taken: the loss kernel raises state[0] itself
        for w in (old, new):
            w.g.fill_(float("nan"))
            slabs = hip.empty(max(need, 4))
            hip.loss_dqn(q, qn, 4, act, act, ones, 0 * ones, ones, 0.99, 8, w.loss, w.dq, w.state)
            o = w.off
            gs = (w.g[o[0]:o[1]], w.g[o[1]:o[2]], w.g[o[2]:w.conv_end])
            pend = _pend(w, segs, pend_slabs)
            if w is old:
                hip.encoder_wgrad(net, w.weights(w.p), frames, None, stride, 0, B, act1, act2, d3, d2, d1, *gs, slabs, pend=pend)
                hip.adam_step_sync_wt(w.p, w.g, w.m, w.v, n, w.state, w.scal, HP["lr"], HP["b1"], HP["b2"], HP["eps"], HP["tf"], w.t, n_total, None, w.weights(w.p), C_,
                                      w.wt, w.wt_t, w.loss, 8, w.ring)
            else:
                plan = hip.encoder_wgrad_tail(net, w.weights(w.p), frames, None, stride, 0, B, act1, act2, d3, d2, d1, *gs, slabs, pend, w.state, w.scal, HP["lr"], HP["b1"],
                                              HP["b2"], HP["tf"])
                assert plan.n >= len(segs)
                for k in range(plan.n):
                    s = plan.seg[k]
                    paths.add("vec" if (s.count | s.slab_stride) % 4 == 0 and (s.slabs | s.out) % 16 == 0 else "scalar")
                hip.update_tail(w.p, w.g, w.m, w.v, n, w.state, w.scal, HP["b1"], HP["b2"], HP["eps"], w.t, n_total, plan, w.weights(w.p), C_, w.wt, w.wt_t, w.loss, 8, w.ring)
        torch.cuda.synchronize()
        a, b = old.everything(), new.everything()
        for k in a:
            if not torch.equal(_bits(a[k]), _bits(b[k])):
                bad = (_bits(a[k]) != _bits(b[k])).nonzero().flatten().tolist()
                print(f"update {u} ({kind}): {k}: {len(bad)} of {a[k].numel()} words differ, conv_end {conv_end}, first {bad[:12]}, last {bad[-4:]}, "
                      f"old {a[k][bad[:4]].tolist()} new {b[k][bad[:4]].tolist()}")
            assert torch.equal(_bits(a[k]), _bits(b[k])), f"update {u} ({kind}): {k}"
        st = old.state.tolist()
        want = {"first": (1, 0, 0), "sync": (2, 0, 1), "nan+sync": (2, 1, 1), "ordinary": (3, 0, 0), "nan": (3, 1, 0)}[kind]
        assert (st[1], st[3], st[4]) == want and st[0] == 0 and st[6] == u + 1, f"update {u} ({kind}): status words {st}"
        if kind.endswith("sync"):
            assert torch.equal(_bits(new.wt_t), _bits(new.wt)) and torch.equal(_bits(new.t), _bits(new.p))
    # the copies are what a refresh from the final weights gives
    fresh = hip.empty(hip.conv_wt_floats(C_))
    hip.conv_wt_refresh(new.weights(new.p), C_, fresh)
    torch.cuda.synchronize()
    assert torch.equal(_bits(fresh), _bits(new.wt))
    return paths


@pytest.mark.parametrize("aligned", [True, False], ids=["n%4==0,n_total>n", "n%4!=0"])
@pytest.mark.parametrize("case", list(CASES))
def test_small_geometry_every_slab_count_on_both_paths(hip, case, aligned):
    n_dense, extra = (1700, 260) if aligned else (1701, 3)
    paths = _compare_five_updates(hip, (4, 36, 36), 8, CASES[case], n_dense, extra, 500 + len(case))
    assert paths == {"vec", "scalar"}


def test_the_real_geometry(hip):
    """C = 4 at 84 x 84: the per-observation weight-gradient kernels (the bookkeeping rides in conv1's), their slab segments beside four pending ones."""
    _compare_five_updates(hip, (4, 84, 84), 8, CASES["31v-32s-33v-72b"], 1700, 260, 77)


def test_bad_plans_are_refused(hip):
    from agent0_amd._abi import A0Error, UpdateTailPlan
    w = _World(hip, 4, 80000, 80000, 3)
    plan = UpdateTailPlan()
    plan.n = 2
    for k in range(2):      # two segments over the same outputs
        s = plan.seg[k]
        s.slabs, s.slab_stride, s.nslab, s.out, s.count = w.m.data_ptr(), 8, 2, w.g.data_ptr() + 4 * w.conv_end, 8
    with pytest.raises(A0Error):
        hip.update_tail(w.p, w.g, w.m, w.v, w.n, w.state, w.scal, 0.9, 0.999, 1e-3, w.t, w.n_total, plan, w.weights(w.p), 4, w.wt, w.wt_t)
    plan.n = 1
    plan.seg[0].out = w.g.data_ptr() + 4 * (w.n_total - 4)      # runs past n_total
    with pytest.raises(A0Error):
        hip.update_tail(w.p, w.g, w.m, w.v, w.n, w.state, w.scal, 0.9, 0.999, 1e-3, w.t, w.n_total, plan, w.weights(w.p), 4, w.wt, w.wt_t)
    with pytest.raises(A0Error):      # convolution weights that are not part of params
        hip.update_tail(w.p, w.g, w.m, w.v, w.n, w.state, w.scal, 0.9, 0.999, 1e-3, w.t, w.n_total, plan, w.weights(w.t), 4, w.wt, w.wt_t)


# ------------------------------------------------------------------------------------------------ the engine: the fused tail, and where it is not used
B = 8
SEED = 42 + 15485863


def _engine(hip, algo, clip=-1.0, **kw):
    from agent0_amd.deepq.engine import DeviceLearner
    from agent0_amd.deepq.layout import NetLayout
    spec = recipe.NetSpec(algo, 4, **kw)
    L = NetLayout.from_spec(spec)
    dev = DeviceLearner(hip, L, B, target_update_freq=2, clip_grad_norm=clip)
    dev.online.load_state_dict(recipe.make_state_dict(spec, 11))
    dev.target.load_state_dict(recipe.make_state_dict(spec, 12))
    return dev, spec


def _batch(hip, spec, ring, s):
    slot = torch.from_numpy(recipe.gen(40 + s).permutation(64)[:B].astype(np.int32)).to(hip.device)
    a, r, d, w = recipe.make_transitions(B, 4, 70 + s)
    return (ring, slot, 2 * 28224) + tuple(torch.from_numpy(x).to(hip.device) for x in (a.astype(np.int32), r, d.astype(np.float32), w))


def _state_of(dev):
    return dict(online=dev.online.flat, target=dev.target.flat, m=dev.adam_m, v=dev.adam_v, grads=dev.grads[:dev.L.n_params_padded], wt=dev.online.wt, wt_target=dev.target.wt,
                state=dev.state, scalars=dev.scalars, ring=dev.loss_ring)


def _three_updates(hip, make):
    """Two engines from the same bytes, the second composing today's three launches; -> (did the first one ever plan a fused tail, both final states)."""
    one, spec = make()
    two, _ = make()
    two.fused_tail = False
    ring = torch.from_numpy(recipe.make_frames(64, 5, spec.obs_shape)).to(hip.device).reshape(-1).contiguous()
    planned = False
    for s in range(3):
        for dev in (one, two):
            dev.forward_dense(*_batch(hip, spec, ring, s))
            dev.exchange_begin()
            dev.backward_encoder(fuse_tail=True)
            planned = planned or dev._tail_plan is not None
            assert dev is one or dev._tail_plan is None
            dev.exchange_end()
            dev.apply()
    torch.cuda.synchronize()
    a, b = _state_of(one), _state_of(two)
    for k in a:
        assert torch.equal(_bits(a[k]), _bits(b[k])), k
    assert one.state[1].item() == 3
    return planned


def test_engine_fused_tail_equals_the_three_launch_chain(hip):
    assert _three_updates(hip, lambda: _engine(hip, "dqn"))
    assert _three_updates(hip, lambda: _engine(hip, "c51"))


def test_clipping_keeps_the_three_launch_chain(hip):
    assert not _three_updates(hip, lambda: _engine(hip, "dqn", clip=0.05))


def test_a_gradient_hook_keeps_the_three_launch_chain(hip):
    def make():
        dev, spec = _engine(hip, "dqn")
        dev.grad_hook = lambda grads, state: None
        return dev, spec
    assert not _three_updates(hip, make)
