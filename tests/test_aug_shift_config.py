"""CPU: the host side of ``learner.aug_shift`` — the config key, the value helper and its refusals, the declarations in the binding table, and the numpy reference
(tests/aug_shift_ref.py) against hand-written cases and against itself.  The GPU side is tests/test_gpu_aug_shift.py."""
import ctypes as C
import os

import numpy as np
import pytest

import aug_shift_ref as R

SEED = 42 + 15485863


def test_config_key_parses_and_round_trips():
    from agent0_amd.deepq import config
    from agent0_amd.deepq.config import from_dict, parse_overrides, to_dict
    cfg = parse_overrides([])
    assert cfg.learner.aug_shift == 0 and isinstance(cfg.learner.aug_shift, int)
    cfg = parse_overrides(["learner.aug_shift=4"])
    assert cfg.learner.aug_shift == 4 and isinstance(cfg.learner.aug_shift, int)
    with pytest.raises(Exception):
        parse_overrides(["learner.aug_shift=wide"])
    d = to_dict(cfg)
    assert d["learner"]["aug_shift"] == 4
    back = from_dict(d)
    assert back.learner.aug_shift == 4 and to_dict(back) == d
    assert from_dict({"learner": {"algo": "dqn"}}).learner.aug_shift == 0, "a dictionary written before the key existed"
    from agent0.deepq import config as alias
    assert alias.parse_overrides(["learner.aug_shift=2"]).learner.aug_shift == 2 and alias.LearnerConfig().aug_shift == 0
    doc = config.__doc__
    assert "learner.aug_shift" in doc and "DrQ" in doc and "mode=play" in doc and "chase" in doc


@pytest.mark.parametrize("value,want", [(0, 0), (None, 0), (0.0, 0), (1, 1), (4, 4), (4.0, 4), (16, 16)])
def test_the_value_helper(value, want):
    import inspect
    from agent0_amd.deepq import engine
    got = engine.aug_shift_value(value, (4, 84, 84), pipeline_target=False)
    assert isinstance(got, int) and got == want
    p = inspect.signature(engine.DeviceLearner.__init__).parameters
    assert p["aug_shift"].default == 0 and p["aug_rng"].default is None


@pytest.mark.parametrize("value,shape", [(-1, (4, 84, 84)), (-4, (4, 84, 84)), (2.5, (4, 84, 84)), (17, (4, 84, 84)), (84, (4, 84, 84)), (12, (4, 12, 20)),
                                         (13, (4, 20, 12)), (4, (1, 4, 4)), (16, (4, 16, 84))])
def test_the_value_helper_refuses_with_the_key_named(value, shape):
    from agent0_amd.deepq import engine
    with pytest.raises(ValueError, match=r"learner\.aug_shift"):
        engine.aug_shift_value(value, shape, pipeline_target=False)


def test_the_value_helper_refuses_the_pipelined_target_pass(monkeypatch):
    from agent0_amd.deepq import engine
    with pytest.raises(ValueError, match=r"learner\.aug_shift.*A0_PIPELINE_TARGET"):
        engine.aug_shift_value(4, (4, 84, 84), pipeline_target=True)
    monkeypatch.setenv("A0_PIPELINE_TARGET", "1")
    with pytest.raises(ValueError, match=r"learner\.aug_shift.*A0_PIPELINE_TARGET"):
        engine.aug_shift_value(4, (4, 84, 84))
    assert engine.aug_shift_value(0, (4, 84, 84)) == 0, "off is off whatever the environment says"
    monkeypatch.setenv("A0_PIPELINE_TARGET", "0")
    assert engine.aug_shift_value(4, (4, 84, 84)) == 4


def test_stream_constant_and_declarations():
    from agent0_amd import _abi
    from agent0_amd.common.utils import DeviceRng
    assert DeviceRng.STREAM_AUG == R.STREAM_AUG == 7
    assert len({DeviceRng.STREAM_EGREEDY_U, DeviceRng.STREAM_EGREEDY_A, DeviceRng.STREAM_TAUS, DeviceRng.STREAM_NOISE, DeviceRng.STREAM_SUMTREE, DeviceRng.STREAM_PERM,
                DeviceRng.STREAM_AUG}) == 7
    protos = {name: (ret, types) for ret, name, types in _abi.parse_header()}
    assert protos["a0_augment_shift"] == ("int", ["ptr", "ptr", "long long", "int", "int", "int", "int", "int", "unsigned long long", "ptr", "long long", "ptr", "ptr"])
    assert protos["a0_learner_set_aug_shift"] == ("int", ["ptr", "int"])
    assert os.path.exists(_abi.LIB_PATH), "build the library first: python -c 'import __graft_entry__ as g; g.build()'"
    lib = _abi.load()
    assert lib.a0_learner_set_aug_shift.argtypes == [C.c_void_p, C.c_int] and lib.a0_augment_shift.restype == C.c_int
    from agent0_amd import ops
    assert hasattr(ops.HipOps, "augment_shift") and hasattr(ops.NativeLearner, "set_aug_shift")


def test_range_checks_are_made_in_front_of_any_launch():
    """The library's checks need no device: every refusal returns A0_EINVAL with a message before a pointer is used (the pointers here are never dereferenced)."""
    from agent0_amd import _abi
    lib = _abi.load()
    fake, EINVAL = 1 << 20, -1
    call = lambda C_, H, W, pad, row, frames=fake, out=fake << 1: lib.a0_augment_shift(frames, None, row, C_, H, W, pad, 2, 1, None, 0, out, None)
    for args in [(4, 84, 84, 0, 2 * 28224), (4, 84, 84, -1, 2 * 28224), (4, 84, 84, 84, 2 * 28224), (4, 12, 20, 12, 1920), (4, 84, 84, 17, 2 * 28224),
                 (4, 84, 84, 4, 2 * 28224 + 16), (1, 3, 3, 1, 18), (4, 84, 84, 4, 2 * 28224, fake + 4), (4, 84, 84, 4, 2 * 28224, fake, fake + 8), (4, 84, 84, 4, 2 * 28224, None)]:
        assert call(*args) == EINVAL and "a0_augment_shift" in _abi.last_error(), args
    assert lib.a0_learner_set_aug_shift(None, 4) == EINVAL and "a0_learner_set_aug_shift" in _abi.last_error()


# ----------------------------------------------------------------------------------------------------------- the reference
def test_zero_draws_are_the_identity():
    g = np.random.default_rng(1)
    rows = g.integers(0, 256, (3, 2, 4, 12, 20), dtype=np.uint8)
    assert np.array_equal(R.shift_rows(rows, np.zeros((3, 4), dtype=np.int64)), rows)


def test_a_hand_written_plane():
    plane = np.array([[1, 2, 3, 4],
                      [5, 6, 7, 8],
                      [9, 10, 11, 12]], dtype=np.uint8)
    # (dy, dx) = (1, -1): out[y][x] = in[min(y + 1, 2)][max(x - 1, 0)]
    want = np.array([[5, 5, 6, 7],
                     [9, 9, 10, 11],
                     [9, 9, 10, 11]], dtype=np.uint8)
    rows = np.stack([plane, plane])[None, :, None]                     # [1, 2, 1, 3, 4]
    out = R.shift_rows(rows, np.array([[1, -1, 0, 0]]))
    assert np.array_equal(out[0, 0, 0], want) and np.array_equal(out[0, 1, 0], plane), "st is shifted, st_next has its own pair"
    out = R.shift_rows(rows, np.array([[0, 0, 1, -1]]))
    assert np.array_equal(out[0, 1, 0], want) and np.array_equal(out[0, 0, 0], plane)
    # replicate pad by p, crop at (dy + p, dx + p)
    p = 2
    padded = np.pad(plane, p, mode="edge")
    for dy in range(-p, p + 1):
        for dx in range(-p, p + 1):
            got = R.shift_rows(rows, np.array([[dy, dx, 0, 0]]))[0, 0, 0]
            assert np.array_equal(got, padded[dy + p:dy + p + 3, dx + p:dx + p + 4]), (dy, dx)


def test_the_largest_shift_repeats_the_edge_row():
    g = np.random.default_rng(2)
    H, W = 12, 20
    rows = g.integers(0, 256, (1, 2, 4, H, W), dtype=np.uint8)
    down = R.shift_rows(rows, np.array([[H - 1, 0, -(H - 1), 0]]))
    assert all(np.array_equal(down[0, 0, :, y], rows[0, 0, :, H - 1]) for y in range(H)), "dy = H - 1: every row is the last input row"
    assert all(np.array_equal(down[0, 1, :, y], rows[0, 1, :, 0]) for y in range(H)), "dy = -(H - 1): every row is the first"


def test_draws_stay_in_range_and_hit_every_value():
    for pad in (1, 3, 4, 11, 16):
        d = R.draws(SEED, 3, 512, pad)
        assert d.shape == (512, 4) and d.min() >= -pad and d.max() <= pad
    d = R.draws(SEED, 0, 512, 4)
    for col in range(4):
        assert set(d[:, col].tolist()) == set(range(-4, 5)), f"column {col}"
    assert not np.array_equal(d[:, 0], d[:, 2]) and not np.array_equal(d[:, 1], d[:, 3]), "st and st_next are drawn independently"


def test_draws_of_an_update_are_a_window_of_the_stream():
    B, pad = 32, 4
    for u in (0, 1, 5):
        assert np.array_equal(R.draws(SEED, u, B, pad), R.draws(SEED, 0, B * (u + 1), pad)[B * u:B * u + B])
    big = 2 ** 33 + 5
    from oracle.core import rng_u32
    words = rng_u32(SEED, 7, 4 * big * B, 4 * B).reshape(B, 4)
    assert np.array_equal(R.draws(SEED, big, B, pad), words.astype(np.int64) % 9 - 4), "positions are 64-bit"
    assert not np.array_equal(R.draws(SEED, big, B, pad), R.draws(SEED, 5, B, pad))
