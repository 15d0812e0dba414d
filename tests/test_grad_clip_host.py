"""CPU: the host side of ``learner.clip_grad_norm`` — the config key, and the C-ABI of the clip path (declared, exported, bound with matching argument counts,
argument validation in front of any HIP call).  The kernels themselves are tested on the GPU (tests/test_gpu_grad_clip.py)."""
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_default_override_and_round_trip():
    from agent0_amd.deepq.config import ExpConfig, from_dict, parse_overrides, to_dict
    cfg = ExpConfig()
    assert cfg.learner.clip_grad_norm == -1.0 and isinstance(cfg.learner.clip_grad_norm, float)
    assert cfg.learner.max_grad_norm == -1.0, "the fqf fraction net's own setting is another key"
    cfg = parse_overrides(["learner.clip_grad_norm=5120", "learner.max_grad_norm=0.05"])
    assert cfg.learner.clip_grad_norm == 5120.0 and isinstance(cfg.learner.clip_grad_norm, float) and cfg.learner.max_grad_norm == 0.05
    assert parse_overrides(["learner.clip_grad_norm=2.5e3"]).learner.clip_grad_norm == 2500.0
    with pytest.raises(ValueError):
        parse_overrides(["learner.clip_grad_norm=ten"])
    d = to_dict(cfg)
    assert d["learner"]["clip_grad_norm"] == 5120.0
    back = from_dict(d)
    assert back.learner.clip_grad_norm == 5120.0 and to_dict(back) == d
    assert from_dict({"learner": {"algo": "dqn"}}).learner.clip_grad_norm == -1.0, "a dictionary written before the key existed"
    import agent0_amd.deepq.config as config
    doc = config.__doc__
    assert "learner.clip_grad_norm" in doc and "batch-SUM" in doc and "batch_size" in doc and "world size" in doc


@pytest.mark.parametrize("value,on", [(-1.0, False), (0.0, False), (-0.0, False), (-5, False), (None, False), (1e-3, True), (5120, True)])
def test_a_non_positive_value_means_off(value, on):
    """DeviceLearner normalises the setting as the handle does (a0_learner_set_grad_clip: max_norm <= 0 switches clipping off): off is -1.0, and then the learner
    holds neither partials nor a ring (tests/test_gpu_grad_clip.py::test_setting_off_changes_no_key_and_no_header)."""
    import inspect
    from agent0_amd.deepq import engine
    got = engine.clip_limit(value)
    assert isinstance(got, float) and (got > 0) == on and (got == float(value) if on else got == -1.0)
    assert inspect.signature(engine.DeviceLearner.__init__).parameters["clip_grad_norm"].default == -1.0


def test_the_header_declares_and_the_binding_matches():
    from agent0_amd import _abi
    protos = {n: (r, t) for r, n, t in _abi.parse_header()}
    base, base_wt = protos["a0_adam_step_sync"][1], protos["a0_adam_step_sync_wt"][1]
    extra = ["ptr", "float", "ptr", "int"]                   # partials, max_norm, norm_ring, norm_ring_cap — in front of the stream
    assert protos["a0_grad_norm_partials"] == ("int", ["ptr", "long long", "ptr", "ptr"])
    assert protos["a0_adam_step_sync_clip"] == ("int", base[:-1] + extra + base[-1:]) and len(protos["a0_adam_step_sync_clip"][1]) == 20
    assert protos["a0_adam_step_sync_wt_clip"] == ("int", base_wt[:-1] + extra + base_wt[-1:]) and len(protos["a0_adam_step_sync_wt_clip"][1]) == 28
    assert protos["a0_learner_set_grad_clip"] == ("int", ["ptr", "double", "ptr", "int"])
    # the existing exports are what they were
    assert len(base) == 16 and len(base_wt) == 24 and protos["a0_learner_peek"] == ("int", ["ptr", "int", "ptr", "ptr"])
    header = open(_abi.HEADER).read()
    assert re.search(r"#define\s+A0_GRAD_NORM_PARTIALS\s+256\b", header) and "A0_PEEK_GRAD_NORM_RING = 6" in header
    lib = _abi.load()
    for name in ("a0_grad_norm_partials", "a0_adam_step_sync_clip", "a0_adam_step_sync_wt_clip", "a0_learner_set_grad_clip"):
        fn = getattr(lib, name)
        assert len(fn.argtypes) == len(protos[name][1]), name
    from agent0_amd.ops import HipOps, NativeLearner
    assert HipOps.GRAD_NORM_PARTIALS == 256
    for cls, names in ((HipOps, ("grad_norm_partials", "adam_step_sync_clip", "adam_step_sync_wt_clip")), (NativeLearner, ("set_grad_clip", "grad_norm_ring"))):
        for n in names:
            assert callable(getattr(cls, n))


def test_arguments_are_checked_before_any_launch():
    """Validation happens in front of every HIP call, so it runs here: null pointers, a non-positive limit, a ring without slots, a null handle."""
    import ctypes as C
    from agent0_amd import _abi
    lib = _abi.load()
    assert lib.a0_grad_norm_partials(None, 8, None, None) == -1 and "a0_grad_norm_partials" in _abi.last_error()
    buf = (C.c_double * 256)()
    p = C.addressof(buf)
    assert lib.a0_grad_norm_partials(p, 0, p, None) == -1
    assert lib.a0_grad_norm_partials(p + 2, 8, p, None) == -1, "a gradient pointer that is not float-aligned"
    sync = lambda max_norm, ring, cap, partials=p: lib.a0_adam_step_sync_clip(p, p, p, p, 8, p, p, 5e-4, 0.9, 0.999, 1e-3, 3, p, 8, None, partials, max_norm, ring, cap, None)
    assert sync(0.0, p, 4) == -1 and "max_norm > 0" in _abi.last_error()
    assert sync(-1.0, p, 4) == -1 and sync(1.0, None, 4) == -1 and sync(1.0, p, 0) == -1 and sync(1.0, p, 4, None) == -1
    wt = lambda max_norm: lib.a0_adam_step_sync_wt_clip(p, p, p, p, 8, p, p, 5e-4, 0.9, 0.999, 1e-3, 3, p, 8, None, p, 4, p, p, None, 0, None, 0, p, max_norm, p, 4, None)
    assert wt(0.0) == -1 and "a0_adam_step_sync_wt_clip" in _abi.last_error()
    assert lib.a0_learner_set_grad_clip(None, 1.0, None, 0) == -1 and "a0_learner_set_grad_clip" in _abi.last_error()
    h = C.c_void_p()
    assert lib.a0_learner_peek(None, 6, C.addressof(h), C.addressof(h)) == -1
