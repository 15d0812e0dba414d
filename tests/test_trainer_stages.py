"""The host loop's pieces that need no GPU: the statistics record of an update block (agent0_amd/deepq/trainer.py::_BlockStats) on host tensors, against values worked
out by hand here, and the rule by which the Trainer tells a test harness from its own instance-level callables (native_loop._wrapped)."""
import types

import pytest
import torch

from agent0_amd.deepq.native_loop import _wrapped
from agent0_amd.deepq.trainer import _BlockStats


def _tr(**kw):
    return types.SimpleNamespace(**{"Ls": [], "FLs": [], "GNs": [], "PN": None, **kw})


RING = torch.arange(8, dtype=torch.float32) * 1.5            # slot s holds 1.5 s
NORMS = torch.tensor([10.0, 11.0, 12.0, 13.0])               # slot s holds 10 + s


def test_loss_ring_window_across_the_wrap():
    """Update counts 1030 .. 1033 on a ring of 8: slots 6, 7, 0, 1 (ring0 % cap + n_upd = 10 > cap)."""
    tr = _tr(Ls=[0.125])
    _BlockStats(n_upd=4, ring0=1030, loss=RING).finish(tr)
    assert tr.Ls == [0.125, 9.0, 10.5, 0.0, 1.5] and tr.FLs == [] and tr.GNs == [] and tr.PN is None


def test_means_and_the_fraction_loss_slice():
    """Without the ring the means lie from index 0; of both buffers only the block's n_upd entries count."""
    tr = _tr(FLs=[3.0])
    _BlockStats(n_upd=3, has_frac=True, loss=torch.tensor([0.5, 0.25, 2.0, 9.0, 9.0]), floss=torch.tensor([4.0, 5.0, 6.0, 7.0, 8.0])).finish(tr)
    assert tr.Ls == [0.5, 0.25, 2.0] and tr.FLs == [3.0, 4.0, 5.0, 6.0]


def test_grad_norms_of_a_block_longer_than_the_ring():
    """Six updates from count 9 on a ring of 4: counts 9 .. 14, of which the ring still holds the newest four, 11 .. 14 = slots 3, 0, 1, 2, in that order."""
    tr = _tr(GNs=[99.0])
    _BlockStats(n_upd=6, ring0=9, gn0=9, loss=torch.zeros(8), gnorm=NORMS).finish(tr)
    assert tr.GNs == [13.0, 10.0, 11.0, 12.0]


def test_grad_norms_of_a_block_that_fits():
    tr = _tr()
    _BlockStats(n_upd=2, ring0=9, gn0=9, loss=torch.zeros(8), gnorm=NORMS).finish(tr)       # counts 9, 10 = slots 1, 2
    assert tr.GNs == [11.0, 12.0]


def test_grad_norm_of_the_unfused_tail():
    """The unfused optimizer tail does not advance the slot counter: one value, from slot state[6] % cap = 13 % 4 = 1."""
    state = torch.zeros(8, dtype=torch.int64)
    state[6] = 13
    tr = _tr()
    _BlockStats(n_upd=3, gn0=9, state=state, loss=torch.zeros(3), gnorm=NORMS).finish(tr)
    assert tr.GNs == [11.0]


def test_param_norm_is_the_index_order_double_sum():
    tr = _tr()
    _BlockStats(n_upd=1, loss=torch.zeros(1), wd_partials=torch.tensor([9.0, 16.0, 0.0, 144.0], dtype=torch.float64)).finish(tr)
    assert tr.PN == 13.0                                     # sqrt(169)
    # in index order each 1.0 is lost against 1e16 (spacing 2): the sum is 1e16 and the root 1e8 exactly; a pairwise or compensated sum gives 1e16 + 2, whose
    # root rounds to the next double above 1e8
    _BlockStats(n_upd=1, loss=torch.zeros(1), wd_partials=torch.tensor([1e16, 1.0, 1.0], dtype=torch.float64)).finish(tr)
    assert tr.PN == 1e8


def test_every_statistic_of_one_block():
    tr = _tr()
    _BlockStats(n_upd=2, ring0=1030, gn0=9, has_frac=True, loss=RING, floss=torch.tensor([4.0, 5.0, 6.0]), gnorm=NORMS,
                wd_partials=torch.tensor([9.0, 16.0], dtype=torch.float64)).finish(tr)
    assert (tr.Ls, tr.FLs, tr.GNs, tr.PN) == ([9.0, 10.5], [4.0, 5.0], [11.0, 12.0], 5.0)


def test_a_block_without_updates_touches_nothing():
    tr = _tr(Ls=[1.0], GNs=[7.0], PN=2.0)
    _BlockStats(n_upd=0, ring0=3, gn0=9, loss=RING, floss=RING, gnorm=NORMS, wd_partials=NORMS.double()).finish(tr)
    assert (tr.Ls, tr.FLs, tr.GNs, tr.PN) == ([1.0], [], [7.0], 2.0)


@pytest.mark.parametrize("name", ["on_snapshot_loaded", "epsilon_fn"])
def test_the_trainers_own_callables_are_no_wrappers(name):
    """launch.TrainerNode installs ``on_snapshot_loaded`` on its Trainer, the Trainer its own ``epsilon_fn``: neither is a harness around the hot loop."""
    obj = types.SimpleNamespace(steps=0, name="x")
    setattr(obj, name, lambda: None)
    assert not _wrapped(obj)


@pytest.mark.parametrize("name", ["sample", "train_batch", "extend", "update_priority", "anything_else"])
def test_any_other_instance_level_function_is_a_wrapper(name):
    obj = types.SimpleNamespace(steps=0, epsilon_fn=lambda s: 0.0, on_snapshot_loaded=lambda: None)
    assert not _wrapped(obj)
    setattr(obj, name, lambda *a, **k: None)
    assert _wrapped(obj)
    bound = types.SimpleNamespace()
    setattr(bound, name, types.MethodType(lambda self: None, bound))      # a bound method counts like a function
    assert _wrapped(bound)
