"""GPU (MI355X): DrQ's random shift of the replay batch (``learner.aug_shift``): a0_augment_shift and everything that issues it.  Byte-exact throughout.

1. the kernel against tests/aug_shift_ref.py: ring rows through a slot vector (non-monotonic, one entry repeated) and dense, the update count from the host (0, 1 and
   2^33 + 5: 64-bit positions) and from a device state block; guard bytes around the output, the ring unchanged, the refusals.
2. five updates with the setting on == five updates with it off on batches the test shifted on the CPU, after every update — through DeviceLearner.update, through
   BaseLearner.train_batch with its hipGraph (two warm-ups, the capture, two replays) and through the a0_learner handle.
3. off is off: aug_shift=0, and a handle switched on and off again, are the untouched learner; the engine holds no stage buffer.
4. the Trainer: handles == Python classes; a snapshot taken mid-run resumes bit for bit.

Work split of the kernel (csrc/augment.hip): one 256-lane workgroup per (sample, observation), 16 output bytes per lane and step; the source observation staged in LDS up
to 64 KiB, read from global memory above.  Shapes: 4 x 84 x 84 (the learner's; 1764 chunks: seven steps, the last one ragged), 4 x 12 x 20 (60 chunks: one step, lanes
idle; chunks that cross rows, 20 not being a multiple of 16), 1 x 4 x 4 (ONE chunk holding four rows), 1 x 260 x 256 (66 560 bytes: the unstaged path)."""
import numpy as np
import pytest
import torch

import aug_shift_ref as R
import recipe

pytestmark = pytest.mark.gpu

SEED = 42 + 15485863            # BaseLearner's Philox seed for cfg.seed = 42
EINVAL = -1
GUARD = 0xA5


@pytest.fixture(scope="module")
def hip():
    from agent0_amd.ops import HipOps
    ops = HipOps()
    assert "gfx950" in ops.device_info()[2]
    assert hasattr(ops, "augment_shift")
    return ops


def _bits(t):
    return t.view(torch.int32) if t.dtype == torch.float32 else t


# ------------------------------------------------------------------------------------------------ 1. the kernel against the reference
CASES = [(5, 4, 84, 84, 4), (3, 4, 12, 20, 1), (3, 4, 12, 20, 3), (3, 4, 12, 20, 11), (2, 1, 4, 4, 3), (2, 4, 20, 36, 16), (2, 1, 260, 256, 5)]
RING_ROWS = 11
SLOTS = [7, 2, 9, 2, 0]         # non-monotonic, 2 twice


@pytest.mark.parametrize("B,C_,H,W,pad", CASES, ids=lambda v: str(v))
def test_kernel_against_reference(hip, B, C_, H, W, pad):
    obs = C_ * H * W
    row = 2 * obs
    ring_np = recipe.gen(900 + obs + pad).integers(0, 256, (RING_ROWS, 2, C_, H, W), dtype=np.uint8)
    ring = torch.from_numpy(ring_np).to(hip.device).reshape(-1).contiguous()
    slots_np = np.array(SLOTS[:B], dtype=np.int32)
    slot = torch.from_numpy(slots_np).to(hip.device)
    state = torch.tensor([0, 3, 0, 0, 0, 3, 7, 0], dtype=torch.int32, device=hip.device)
    for use_slot in (True, False):
        rows = ring_np[slots_np] if use_slot else ring_np[:B]
        for u, from_state in ((0, False), (1, False), (2 ** 33 + 5, False), (7, True)):
            want = R.shift_rows(rows, R.draws(SEED, u, B, pad))
            buf = torch.full((64 + B * row + 64,), GUARD, dtype=torch.uint8, device=hip.device)
            out = buf[64:64 + B * row]
            assert out.data_ptr() % 16 == 0
            hip.augment_shift(ring, slot if use_slot else None, row, C_, H, W, pad, B, SEED, state if from_state else None, 0 if from_state else u, out)
            torch.cuda.synchronize()
            got = out.cpu().numpy().reshape(want.shape)
            bad = int((got != want).sum())
            print(f"B={B} {C_}x{H}x{W} pad={pad} slot={use_slot} u={u} state={from_state}: {bad} of {want.size} bytes differ")
            assert bad == 0
            assert bool((buf[:64] == GUARD).all()) and bool((buf[64 + B * row:] == GUARD).all()), "nothing outside the batch is written"
            if u == 0:
                assert not np.array_equal(got, rows), "the shift moves bytes"
    assert torch.equal(ring.cpu(), torch.from_numpy(ring_np).reshape(-1)), "the ring is only read"
    assert state.tolist() == [0, 3, 0, 0, 0, 3, 7, 0], "the state block is only read"
    # refusals: A0_EINVAL with a message, nothing launched
    from agent0_amd import _abi
    lib = hip.lib
    sentinel = torch.full((B * row,), GUARD, dtype=torch.uint8, device=hip.device)
    rp, op = ring.data_ptr(), sentinel.data_ptr()
    bad_args = [(C_, H, W, 0, row), (C_, H, W, -2, row), (C_, H, W, min(H, W), row), (C_, H, W, 17, row), (C_, H, W, pad, row + 16), (C_, H, W, pad, row - 16)]
    for c, h, w, p, rb in bad_args:
        assert lib.a0_augment_shift(rp, None, rb, c, h, w, p, B, SEED, None, 0, op, None) == EINVAL and _abi.last_error(), (c, h, w, p, rb)
    assert lib.a0_augment_shift(rp, None, 18, 1, 3, 3, 1, B, SEED, None, 0, op, None) == EINVAL and "multiple of 16" in _abi.last_error()
    assert lib.a0_augment_shift(rp, None, row, C_, H, W, pad, B, SEED, None, 0, op + 4, None) == EINVAL and "aligned" in _abi.last_error()
    assert lib.a0_augment_shift(None, None, row, C_, H, W, pad, B, SEED, None, 0, op, None) == EINVAL and _abi.last_error()
    torch.cuda.synchronize()
    assert bool((sentinel == GUARD).all()), "a refused call launches nothing"


# ------------------------------------------------------------------------------------------------ 2. the update on the shifted batch
A, BATCH, RING2, PAD, UPDATES = 6, 32, 64, 4, 5
SHAPE = (4, 84, 84)
ROW = 2 * 4 * 84 * 84
ALGOS = {"dqn": dict(spec=dict(algo="dqn"), double_q=False, cfg=[]),
         "c51-double-duel": dict(spec=dict(algo="c51", dueling=True), double_q=True, cfg=["learner.double_q=true", "learner.dueling_head=true"])}
_WORLD = {}


def _world():
    """The ring and five updates' inputs (numpy; never modified)."""
    if not _WORLD:
        _WORLD["ring"] = recipe.make_frames(RING2, 77, SHAPE).reshape(RING2, 2, *SHAPE)
        for s in range(UPDATES):
            a, r, d, w = recipe.make_transitions(BATCH, A, 600 + s)
            _WORLD[s] = (recipe.gen(500 + s).integers(0, RING2, BATCH).astype(np.int32), a.astype(np.int32), r, d.astype(np.float32), w)
    return _WORLD


def _spec(name):
    return recipe.NetSpec(action_dim=A, obs_shape=SHAPE, **ALGOS[name]["spec"])


def _engine(hip, name, **kw):
    from agent0_amd.deepq.engine import DeviceLearner
    from agent0_amd.deepq.layout import NetLayout
    dev = DeviceLearner(hip, NetLayout.from_spec(_spec(name)), BATCH, double_q=ALGOS[name]["double_q"], target_update_freq=2, **kw)
    _load(dev, name)
    return dev


def _load(dev, name):
    dev.online.load_state_dict(recipe.make_state_dict(_spec(name), 11))
    dev.target.load_state_dict(recipe.make_state_dict(_spec(name), 12))


def _snap(dev, loss):
    torch.cuda.synchronize()
    return dict(online=dev.online.flat.clone(), target=dev.target.flat.clone(), moment1=dev.adam_m.clone(), moment2=dev.adam_v.clone(), loss=loss[:BATCH].clone())


_REFS = {}


def _reference(hip, name, pad):
    """Five updates of a learner WITHOUT the setting; pad > 0: on dense batches shifted on the CPU with the draws of updates 0 .. 4; pad == 0: on the ring through the
    slot vector, as it always ran.  -> the state after every update (computed once per learner and pad)."""
    if (name, pad) not in _REFS:
        w, D = _world(), lambda x: torch.from_numpy(np.ascontiguousarray(x)).to(hip.device)
        dev = _engine(hip, name)
        assert dev.aug_shift == 0 and dev.aug_stage is None
        ring = D(w["ring"].reshape(-1))
        out = []
        for s in range(UPDATES):
            slots, a, r, d, wg = w[s]
            if pad > 0:
                batch = R.shift_rows(w["ring"][slots], R.draws(SEED, s, BATCH, pad))
                loss = dev.update(D(batch.reshape(-1)), None, ROW, D(a), D(r), D(d), D(wg))
            else:
                loss = dev.update(ring, D(slots), ROW, D(a), D(r), D(d), D(wg))
            out.append(_snap(dev, loss))
        assert int(dev.state[6]) == UPDATES and int(dev.state[1]) == UPDATES
        _REFS[(name, pad)] = out
    return _REFS[(name, pad)]


def _same(got, want, what):
    for k in want:
        assert torch.equal(_bits(got[k]), _bits(want[k])), f"{what}: {k}"


@pytest.mark.parametrize("name", list(ALGOS))
def test_eager_update_equals_the_update_on_shifted_batches(hip, name):
    from agent0_amd.common.utils import DeviceRng
    want = _reference(hip, name, PAD)
    w, D = _world(), lambda x: torch.from_numpy(np.ascontiguousarray(x)).to(hip.device)
    dev = _engine(hip, name, aug_shift=PAD, aug_rng=DeviceRng(hip, SEED))
    assert dev.aug_shift == PAD and dev.aug_stage.numel() == BATCH * ROW and dev.aug_stage.dtype == torch.uint8
    ring = D(w["ring"].reshape(-1))
    ring0 = ring.clone()
    for s in range(UPDATES):
        slots, a, r, d, wg = w[s]
        loss = dev.update(ring, D(slots), ROW, D(a), D(r), D(d), D(wg))
        _same(_snap(dev, loss), want[s], f"{name}: update {s + 1}")
    assert torch.equal(ring, ring0), "the ring is never written"
    plain = _reference(hip, name, 0)
    assert not torch.equal(want[0]["loss"], plain[0]["loss"]) and not torch.equal(want[-1]["online"], plain[-1]["online"]), "the shift changes the update"
    with pytest.raises(ValueError, match="tstage"):
        dev.forward_dense(ring, D(w[0][0]), ROW, D(w[0][1]), D(w[0][2]), D(w[0][3]), D(w[0][4]), tstage=0)


@pytest.mark.parametrize("name", list(ALGOS))
def test_graph_replays_advance_the_update_count(hip, name):
    """BaseLearner.train_batch with graphs on: updates 1 and 2 run eagerly, update 3 is the capture's first replay, 4 and 5 replay it — a replay that shifted by the
    draws of the update it was captured at would part from the reference at update 4."""
    from agent0_amd.deepq import agent
    from agent0_amd.deepq.config import parse_overrides
    want = _reference(hip, name, PAD)
    algo = ALGOS[name]["spec"]["algo"]
    cfg = parse_overrides([f"learner.algo={algo}", "seed=42", f"learner.batch_size={BATCH}", "learner.target_update_freq=2", f"action_dim={A}", "obs_shape=(4,84,84)",
                           f"learner.aug_shift={PAD}"] + ALGOS[name]["cfg"])
    ln = {"dqn": agent.DQNLearner, "c51": agent.C51Learner}[algo](cfg, ops=hip)
    assert ln.use_graph and ln.rng.seed == SEED and ln.engine.aug_shift == PAD and ln.engine.aug_rng is ln.rng
    _load(ln.engine, name)
    w, D = _world(), lambda x: torch.from_numpy(np.ascontiguousarray(x)).to(hip.device)
    ring = D(w["ring"].reshape(-1))
    bufs = [D(x) for x in w[0]]                                       # persistent device tensors: the graph holds their addresses
    for s in range(UPDATES):
        for t, x in zip(bufs, w[s]):
            t.copy_(D(x))
        loss, _ = ln.train_batch(ring, bufs[0], ROW, *bufs[1:])
        _same(_snap(ln.engine, loss), want[s], f"{name}: update {s + 1}")
    assert len(ln._graphs) == 1, "the last three updates were replays of one captured graph"
    assert int(ln.engine.state[6]) == UPDATES


@pytest.mark.parametrize("name", list(ALGOS))
def test_handle_equals_the_update_on_shifted_batches(hip, name):
    from agent0_amd._abi import A0Error
    want = _reference(hip, name, PAD)
    c = ALGOS[name]
    src = _engine(hip, name)
    nat = hip.native_learner(A=A, dueling=c["spec"].get("dueling", False), double_q=c["double_q"], B=BATCH, discount=0.99, lr=5e-4, target_update_freq=2,
                             algo=c["spec"]["algo"], num_atoms=51, vmin=-10.0, vmax=10.0, seed=SEED)
    nat.set_params(src.online.flat, src.target.flat)
    for bad in (-1, 17, 84):
        with pytest.raises(A0Error, match="a0_learner_set_aug_shift"):
            nat.set_aug_shift(bad)
    nat.set_aug_shift(PAD)
    w, D = _world(), lambda x: torch.from_numpy(np.ascontiguousarray(x)).to(hip.device)
    ring = D(w["ring"].reshape(-1))
    ring0 = ring.clone()
    loss = hip.empty(BATCH)
    for s in range(UPDATES):
        slots, a, r, d, wg = w[s]
        nat.update(ring, D(slots), ROW, D(a), D(r), D(d), D(wg), loss_out=loss)
        torch.cuda.synchronize()
        o, t, m, v, st = nat.get()
        _same(dict(online=o, target=t, moment1=m, moment2=v, loss=loss), want[s], f"{name}: handle, update {s + 1}")
    assert torch.equal(ring, ring0)
    with pytest.raises(A0Error, match="row_bytes"):      # with the setting on a row holds st || st_next and nothing else
        nat.update(torch.cat([ring, ring[:64]]), D(w[0][0]), ROW + 16, D(w[0][1]), D(w[0][2]), D(w[0][3]), D(w[0][4]))
    nat.close()


# ------------------------------------------------------------------------------------------------ 3. off is off
@pytest.mark.parametrize("name", list(ALGOS))
def test_off_is_the_untouched_learner(hip, name):
    want = _reference(hip, name, 0)
    w, D = _world(), lambda x: torch.from_numpy(np.ascontiguousarray(x)).to(hip.device)
    ring = D(w["ring"].reshape(-1))
    dev = _engine(hip, name, aug_shift=0)
    assert dev.aug_shift == 0 and dev.aug_stage is None, "no stage buffer"
    c = ALGOS[name]
    nat = hip.native_learner(A=A, dueling=c["spec"].get("dueling", False), double_q=c["double_q"], B=BATCH, discount=0.99, lr=5e-4, target_update_freq=2,
                             algo=c["spec"]["algo"], num_atoms=51, vmin=-10.0, vmax=10.0, seed=SEED)
    nat.set_params(dev.online.flat, dev.target.flat)
    nat.set_aug_shift(PAD)
    nat.set_aug_shift(0)
    loss_n = hip.empty(BATCH)
    for s in range(UPDATES):
        slots, a, r, d, wg = w[s]
        loss = dev.update(ring, D(slots), ROW, D(a), D(r), D(d), D(wg))
        _same(_snap(dev, loss), want[s], f"{name}: aug_shift=0, update {s + 1}")
        nat.update(ring, D(slots), ROW, D(a), D(r), D(d), D(wg), loss_out=loss_n)
        torch.cuda.synchronize()
        o, t, m, v, st = nat.get()
        _same(dict(online=o, target=t, moment1=m, moment2=v, loss=loss_n), want[s], f"{name}: handle on then off, update {s + 1}")
    nat.close()


# ------------------------------------------------------------------------------------------------ 4. the Trainer
BASE = ["actor.num_envs=16", "actor.sample_steps=8", "learner.batch_size=32", "learner.learner_steps=3", "replay.size=2000", "trainer.training_start_steps=200",
        "trainer.exploration_steps=512", "actor.min_eps=0.4", "learner.target_update_freq=4", "trainer.test_episodes=2", "wandb=false", "tb=false"]


def _trainer(tmp_path, monkeypatch, native, tag, pad=PAD, seed=42):
    from agent0_amd.deepq.config import parse_overrides
    from agent0_amd.deepq.trainer import Trainer
    monkeypatch.setenv("A0_NATIVE_LOOP", "1" if native else "0")
    return Trainer(parse_overrides(["learner.algo=dqn", f"learner.aug_shift={pad}", f"seed={seed}", f"logdir={tmp_path / tag}"] + BASE))


def _state(tr):
    torch.cuda.synchronize()
    eng, rp = tr.learner.engine, tr.replay
    n = len(rp)                                       # the ring does not wrap in these runs
    return [eng.online.flat.clone(), eng.target.flat.clone(), eng.adam_m.clone(), eng.adam_v.clone(), eng.state.clone(), eng.online.wt.clone(), eng.target.wt.clone(),
            rp.frames[: n * rp.row_bytes].clone(), rp.act[:n].clone(), rp.rew[:n].clone(), rp.done[:n].clone()]


def _close(tr):
    tr.test = lambda: None
    tr.final(save=False)


def _run(tmp_path, monkeypatch, native, tag, pad=PAD, iters=6):
    from agent0_amd.deepq.native_loop import NativeLoop
    tr = _trainer(tmp_path, monkeypatch, native, tag, pad)
    assert tr.learner.engine.aug_shift == pad
    res = [{k: v for k, v in tr.run_iteration().items() if k != "fps"} for _ in range(iters)]
    assert isinstance(tr._nl, NativeLoop) if native else tr._nl is False, getattr(tr, "native_loop_reason", None)
    out = _state(tr), res, list(tr.Qs), list(tr.Rs), tr.frame_count
    assert res[-1]["loss"] is not None, "updates ran"
    _close(tr)
    return out


_RUNS = {}


def _whole_run(tmp_path, monkeypatch, native):
    if native not in _RUNS:
        _RUNS[native] = _run(tmp_path, monkeypatch, native, "whole-nat" if native else "whole-py")
    return _RUNS[native]


def test_handles_and_python_classes_end_on_the_same_state(tmp_path, monkeypatch):
    """Six iterations of 128 transitions, three updates each once 200 are in the ring: twelve updates, the Python classes' last ones replayed from the hipGraph."""
    a, b = _whole_run(tmp_path, monkeypatch, False), _whole_run(tmp_path, monkeypatch, True)
    for i, (x, y) in enumerate(zip(a[0], b[0])):
        assert torch.equal(_bits(x), _bits(y)), f"state item {i}"
    assert a[1:] == b[1:]
    assert a[0][4][6].item() >= 9, "updates ran"
    plain = _run(tmp_path, monkeypatch, True, "plain", pad=0)
    assert plain[0][4][1].item() == a[0][4][1].item() and not torch.equal(plain[0][0], a[0][0]), "the setting changes the run"


@pytest.mark.parametrize("native", [True, False], ids=["handles", "python-classes"])
def test_a_snapshot_taken_mid_run_resumes_bit_for_bit(native, tmp_path, monkeypatch):
    want = _whole_run(tmp_path, monkeypatch, native)
    tr = _trainer(tmp_path, monkeypatch, native, "b")
    for _ in range(4):
        tr.run_iteration()
    assert tr.learner.engine.state[6].item() > 0, "updates have run: the resumed run must continue the sequence of shifts, not restart it"
    snap_dir = tr.save_snapshot(str(tmp_path / "snap"))
    _close(tr)
    tr = _trainer(tmp_path, monkeypatch, native, "c", seed=7)           # another seed: the snapshot's is the run's
    tr.load_snapshot(snap_dir)
    res = [{k: v for k, v in tr.run_iteration().items() if k != "fps"} for _ in range(2)]
    got = _state(tr)
    _close(tr)
    for i, (x, y) in enumerate(zip(got, want[0])):
        assert torch.equal(_bits(x), _bits(y)), f"state item {i}"
    assert res == want[1][4:]
