"""GPU (MI355X): the one equality between Adam's forms that no other suite pins — a0_adam_step against a0_adam_step_sync on the scalar path, bit for bit.

csrc/optim.hip steps a parameter in two arithmetic forms (a0_adam_wide, a0_adam_scalar).  tests/test_gpu_update_tail.py holds the one-launch tail to the
three-launch chain on both; this file holds a0_adam_step, which always steps element by element, to the scalar path of a0_adam_step_sync.

Geometries (256 lanes per workgroup, at most 2048 workgroups, grid-stride behind that):
  * n = 1027, n_total = 1030: n % 4 = 3, so every path is scalar; more than four workgroups; and a range behind n that only the sync form touches;
  * n = n_total = 2048 * 256 + 5: the smallest size at which the cap of 2048 workgroups makes a lane take a second grid-stride trip.
Both worlds start from the same bytes and run five consecutive updates with target_update_freq = 2 — first step, sync, NaN-skipped + sync, ordinary, NaN-skipped —
the flag raised by setting state[0] before the call.  After every update the parameters over [0, n), both moments, state[0..4] and the scalars are compared as bit
patterns; on the sync updates the sync form's target equals its parameters over [0, n_total)."""
import numpy as np
import pytest
import torch

import recipe

pytestmark = pytest.mark.gpu

HP = dict(lr=5e-4, b1=0.9, b2=0.999, eps=1e-2 / 32, tf=2)
KINDS = ["first", "sync", "nan+sync", "ordinary", "nan"]


@pytest.fixture(scope="module")
def hip():
    from agent0_amd.ops import HipOps
    ops = HipOps()
    assert "gfx950" in ops.device_info()[2]
    return ops


def _bits(t):
    return t.view(torch.int32) if t.dtype == torch.float32 else t


class _World:
    def __init__(self, hip, n, n_total, seed):
        g = recipe.gen(seed)
        f = lambda k, scale: torch.from_numpy((g.standard_normal(k) * scale).astype(np.float32)).to(hip.device)
        self.p, self.t = f(n_total, 0.05), f(n_total, 0.05)
        self.m, self.v = f(n, 1e-3), f(n, 1e-3).abs()
        self.state = torch.zeros(8, dtype=torch.int32, device=hip.device)
        self.scal = hip.zeros(2)


@pytest.mark.parametrize("n,n_total", [(1027, 1030), (2048 * 256 + 5, 2048 * 256 + 5)], ids=["n=1027,n_total=1030", "n=2048*256+5"])
def test_adam_step_equals_adam_step_sync_on_the_scalar_path(hip, n, n_total):
    assert n % 4 != 0, "every path scalar"
    plain, sync = _World(hip, n, n_total, 900), _World(hip, n, n_total, 900)
    gen = recipe.gen(901)
    args = (HP["lr"], HP["b1"], HP["b2"], HP["eps"], HP["tf"])
    for u, kind in enumerate(KINDS):
        g = torch.from_numpy((gen.standard_normal(n) * 0.1).astype(np.float32)).to(hip.device)
        for w in (plain, sync):
            if kind.startswith("nan"):
                w.state[0] = 1
        before = sync.p.clone()
        hip.adam_step(plain.p, g, plain.m, plain.v, n, plain.state, plain.scal, *args)
        hip.adam_step_sync(sync.p, g, sync.m, sync.v, n, sync.state, sync.scal, *args, sync.t, n_total)
        torch.cuda.synchronize()
        for name, a, b in (("params", plain.p[:n], sync.p[:n]), ("exp_avg", plain.m, sync.m), ("exp_avg_sq", plain.v, sync.v), ("state[0..4]", plain.state[:5], sync.state[:5]),
                           ("scalars", plain.scal, sync.scal)):
            same = torch.equal(_bits(a), _bits(b))
            if not same:
                bad = (_bits(a) != _bits(b)).nonzero().flatten().tolist()
                print(f"update {u} ({kind}): {name}: {len(bad)} of {a.numel()} words differ, first {bad[:12]}, adam_step {a[bad[:4]].tolist()} adam_step_sync {b[bad[:4]].tolist()}")
            assert same, f"update {u} ({kind}): {name}"
        st = sync.state.tolist()
        want = {"first": (1, 0, 0), "sync": (2, 0, 1), "nan+sync": (2, 1, 1), "ordinary": (3, 0, 0), "nan": (3, 1, 0)}[kind]
        assert (st[1], st[3], st[4]) == want and st[0] == 0, f"update {u} ({kind}): status words {st}"
        assert torch.equal(_bits(sync.p[n:]), _bits(before[n:])), f"update {u} ({kind}): Adam does not own [n, n_total)"
        assert torch.equal(_bits(sync.p), _bits(before)) == kind.startswith("nan"), f"update {u} ({kind}): a step moves the parameters, a skipped one leaves them alone"
        if kind.endswith("sync"):
            assert torch.equal(_bits(sync.t), _bits(sync.p)), f"update {u} ({kind}): the sync form's target over [0, n_total)"
