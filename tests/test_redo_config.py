"""CPU: the host side of ``learner.redo_freq`` / ``learner.redo_tau`` / ``learner.redo_recycle`` — the config keys, the value helper and its refusals, the index maps
of the restatement tests/redo_ref.py against ``NetLayout`` (a marked channel, packed and unpacked), the declarations in the binding table, the library's argument
checks (made in front of any launch), and the statistics' columns, which appear only with the setting on.  The GPU side is tests/test_gpu_redo.py."""
import csv
import ctypes as C
import logging
import math
import types

import numpy as np
import pytest
import torch

import net_reset_ref as R
import redo_ref as RD

LAYOUTS = [("dqn", 4, False, (4, 84, 84)), ("dqn", 18, True, (4, 84, 84)), ("c51", 6, True, (4, 84, 84)), ("iqn", 9, True, (4, 84, 84)), ("fqf", 3, False, (4, 84, 84)),
           ("dqn", 4, False, (1, 84, 84)), ("dqn", 5, False, (4, 52, 60))]
IDS = ["dqn-4", "dqn-duel-18", "c51-duel-6", "iqn-duel-9", "fqf-3", "dqn-C1", "dqn-52x60"]


def _layout(algo, A, dueling, obs, noisy=False):
    from agent0_amd.deepq.layout import NetLayout
    return NetLayout(algo, A, dueling, noisy, 51, obs)


# ----------------------------------------------------------------------------------------------------------- settings
def test_config_keys_parse_and_round_trip():
    from agent0_amd.deepq import config
    from agent0_amd.deepq.config import from_dict, parse_overrides, to_dict
    lc = parse_overrides([]).learner
    assert lc.redo_freq == 0 and isinstance(lc.redo_freq, int) and lc.redo_tau == 0.1 and isinstance(lc.redo_tau, float) and lc.redo_recycle is True
    cfg = parse_overrides(["learner.redo_freq=1000", "learner.redo_tau=0.025", "learner.redo_recycle=false"])
    assert cfg.learner.redo_freq == 1000 and cfg.learner.redo_tau == 0.025 and cfg.learner.redo_recycle is False
    assert parse_overrides(["learner.redo_tau=0"]).learner.redo_tau == 0.0
    for bad in ("learner.redo_freq=often", "learner.redo_tau=low"):
        with pytest.raises(Exception):
            parse_overrides([bad])
    d = to_dict(cfg)
    assert d["learner"]["redo_freq"] == 1000 and d["learner"]["redo_tau"] == 0.025 and d["learner"]["redo_recycle"] is False
    back = from_dict(d)
    assert (back.learner.redo_freq, back.learner.redo_tau, back.learner.redo_recycle) == (1000, 0.025, False) and to_dict(back) == d
    old = from_dict({"learner": {"algo": "dqn"}}).learner
    assert (old.redo_freq, old.redo_tau, old.redo_recycle) == (0, 0.1, True), "a dictionary written before the keys existed"
    from agent0.deepq import config as alias
    assert alias.LearnerConfig().redo_freq == 0 and alias.parse_overrides(["learner.redo_freq=7"]).learner.redo_freq == 7
    doc = " ".join(config.__doc__.split())
    for words in ("learner.redo_freq", "learner.redo_tau", "learner.redo_recycle", "Sokar et al. 2023", "dormant_frac", "A0_DP_FORCE=1", "learner.noisy_net"):
        assert words in doc, words


@pytest.mark.parametrize("args,want", [((0,), (0, 0.1, True)), ((None, None), (0, 0.1, True)), ((3, 0.025, False), (3, 0.025, False)), ((5.0, 0, True), (5, 0.0, True)),
                                       ((1, 0.999999), (1, 0.999999, True))])
def test_the_value_helper(args, want):
    import inspect
    from agent0_amd.deepq import engine
    got = engine.redo_value(*args, data_parallel=False)
    assert got == want and isinstance(got[0], int) and isinstance(got[1], float) and isinstance(got[2], bool)
    p = inspect.signature(engine.DeviceLearner.__init__).parameters
    assert p["redo_freq"].default == 0 and p["redo_tau"].default == 0.1 and p["redo_recycle"].default is True


@pytest.mark.parametrize("freq", [-1, -1000, 2.5, True])
def test_a_bad_period_is_refused_by_name(freq):
    from agent0_amd.deepq import engine
    with pytest.raises(ValueError, match=r"learner\.redo_freq"):
        engine.redo_value(freq, 0.1, data_parallel=False)


@pytest.mark.parametrize("tau", [-0.1, 1.0, 1.5, float("nan"), float("inf"), -float("inf")])
@pytest.mark.parametrize("freq", [0, 3])
def test_a_bad_threshold_is_refused_with_the_number_named(freq, tau):
    from agent0_amd.deepq import engine
    with pytest.raises(ValueError, match=r"learner\.redo_tau") as e:
        engine.redo_value(freq, tau, data_parallel=False)
    assert repr(tau) in str(e.value)


def test_recycling_is_refused_under_noisy_net_and_measuring_is_not():
    from agent0_amd.deepq import engine
    with pytest.raises(ValueError, match=r"learner\.redo_freq.*learner\.redo_recycle.*learner\.noisy_net"):
        engine.redo_value(3, 0.1, True, noisy=True, data_parallel=False)
    assert engine.redo_value(3, 0.1, False, noisy=True, data_parallel=False) == (3, 0.1, False)
    assert engine.redo_value(0, 0.1, True, noisy=True, data_parallel=False) == (0, 0.1, True), "off is off"
    with pytest.raises(ValueError, match="NoisyNet"):
        _layout("c51", 4, True, (4, 84, 84), noisy=True).redo_blocks()


def test_the_data_parallel_path_is_refused(monkeypatch):
    from agent0_amd.deepq import engine
    monkeypatch.delenv("A0_DP_FORCE", raising=False)
    monkeypatch.delenv("WORLD_SIZE", raising=False)
    assert engine.redo_value(3, 0.1, True) == (3, 0.1, True)
    for recycle in (True, False):
        with pytest.raises(ValueError, match=r"learner\.redo_freq.*data-parallel"):
            engine.redo_value(3, 0.1, recycle, data_parallel=True)
    monkeypatch.setenv("A0_DP_FORCE", "1")
    with pytest.raises(ValueError, match=r"learner\.redo_freq.*A0_DP_FORCE=1"):
        engine.redo_value(3, 0.1, False)
    assert engine.redo_value(0, 0.1, True) == (0, 0.1, True), "off is off whatever the environment says"
    monkeypatch.delenv("A0_DP_FORCE")
    monkeypatch.setenv("WORLD_SIZE", "2")
    with pytest.raises(ValueError, match=r"learner\.redo_freq.*data-parallel"):
        engine.redo_value(3, 0.1, True)
    # a gradient exchange installed later (launch.TrainerNode) is met by the launch itself
    eng = types.SimpleNamespace(redo_freq=3, grad_hook=lambda g, s: None)
    with pytest.raises(ValueError, match=r"learner\.redo_freq=3.*gradient exchange"):
        engine.DeviceLearner._redo(eng)


# ----------------------------------------------------------------------------------------------------------- the restatement
def test_scores_mask_and_counts_of_the_restatement():
    g = np.random.default_rng(2)
    acts = [np.abs(g.standard_normal((7, n))) + 0.5 for n in (32, 64, 64, 512)]
    acts[0][:, 3] = 0.0                                   # silent
    acts[1] = -acts[1]                                    # |.|
    acts[1][:, 10] *= 1e-3
    acts[2][:] = 0.0                                      # a layer whose mean is 0: every score 0, every neuron dormant
    s, mask, counts = RD.evaluate(acts, 0.1)
    assert s.dtype == np.float64 and s.shape == (672,) and mask.dtype == np.int32
    for (name, lo, n), X in zip(RD.LAYERS, acts):
        if name != "conv3":
            assert s[lo:lo + n].mean() == pytest.approx(1.0, rel=1e-12), "scores of a layer average 1"
    assert s[3] == 0.0 and s[32 + 10] < 2e-3 and not s[96:160].any()
    assert counts == [1, 1, 64, 0, 66] and mask[3] == 1 and mask[42] == 1 and mask[96:160].all() and mask.sum() == 66
    assert RD.evaluate(acts, 0.0)[2] == [1, 0, 64, 0, 65]
    m = np.abs(acts[3]).sum(0) / 7
    assert np.allclose(s[160:], m / m.mean(), rtol=1e-14, atol=0)
    assert RD.margin(s, 0.1) > 1e-6 and RD.margin(s, 0.0) == math.inf


@pytest.mark.parametrize("spec", LAYOUTS, ids=IDS)
def test_index_maps_against_the_layout(spec):
    """One neuron per layer at a time: the touched elements, marked in a flat buffer and unpacked into the reference's shapes, are exactly that channel's incoming
    filter and bias and the next layer's input slice — conv weights [out][in][kh][kw], fc1's columns in (c, h, w) order."""
    algo, A, dueling, obs = spec
    L = _layout(algo, A, dueling, obs)
    blocks = RD.blocks_of(L)
    assert L.redo_blocks() == tuple(blocks[n][0] for n in ("conv1", "conv2", "conv3", "fc1", "head")) + (L.C * 64, L.feat, L.Npad)
    assert [(n, lo, w) for n, lo, w in L.REDO_LAYERS] == list(RD.LAYERS)
    keys = {"conv1": "encoder.convs.0", "conv2": "encoder.convs.2", "conv3": "encoder.convs.4", "fc1": "head.first_dense"}
    heads = ["head.q_head"] + (["head.value_head"] if dueling else [])
    for (name, lo, n), i in zip(RD.LAYERS, (5, 63, 0, 511)):
        mask = np.zeros(672, np.int32)
        mask[lo + i] = 1
        inc, out = RD.touched(blocks, mask)
        assert not np.intersect1d(inc, out).size and inc.max() < L.n_adam and out.max() < L.n_adam
        nxt = RD.NEXT[name][0]
        assert inc.size == blocks[name][2] + 1 and out.size == blocks[nxt][1] * blocks[nxt][2] // n
        flat = torch.zeros(L.n_params_padded)
        flat[torch.from_numpy(inc)] = 1.0
        flat[torch.from_numpy(out)] = 2.0
        sd = L.unpack(flat)
        want = {k: torch.zeros_like(v) for k, v in sd.items()}
        want[keys[name] + ".weight"][i] = 1.0
        want[keys[name] + ".bias"][i] = 1.0
        if name == "conv3":
            want["head.first_dense.weight"].reshape(512, 64, L.H3, L.W3)[:, i] = 2.0
        elif name == "fc1":
            for h in heads:
                want[h + ".weight"][:, i] = 2.0
        else:
            want[keys[nxt] + ".weight"][:, i] = 2.0
        for k in sd:
            assert torch.equal(sd[k], want[k]), f"{name}[{i}]: {k}"
        # the head's padded rows, which no reference tensor shows, are zeroed too: column i of all Npad rows
        if name == "fc1":
            off, N, K = blocks["head"]
            assert N == L.Npad and np.array_equal(out, off + np.arange(N) * K + i)
        # and packing the marked state_dict back gives the same flat buffer (pad rows aside)
        again = torch.zeros(L.n_params_padded)
        L.pack(sd, again)
        if name != "fc1":
            assert torch.equal(again, flat)
    # every neuron at once: every element of conv1 .. fc1 and every head weight is touched; head biases, the cosine embedding and the fraction net never are
    inc, out = RD.touched(blocks, np.ones(672, np.int32))
    both = np.union1d(inc, out)
    hoff, hN, hK = blocks["head"]
    assert np.array_equal(both, np.arange(hoff + hN * hK)), "conv1 .. fc1 with their biases and the head's weights"
    assert np.array_equal(np.intersect1d(inc, out), np.concatenate([blocks[n][0] + np.arange(blocks[n][1] * blocks[n][2]) for n in ("conv2", "conv3", "fc1")]))


def test_fresh_values_and_moments_of_the_restatement():
    L = _layout("dqn", 4, False, (4, 84, 84))
    blocks, segs = RD.blocks_of(L), R.segments(L)
    n = L.n_params_padded
    g = np.random.default_rng(3)
    p, m, v = (g.standard_normal(n).astype(np.float32) for _ in range(3))
    phi = g.standard_normal(n).astype(np.float32)
    mask = np.zeros(672, np.int32)
    mask[[0, 31, 32 + 7, 96 + 63, 160, 671]] = 1
    p1, m1, v1, both = RD.expect(p, m, v, blocks, segs, mask, phi)
    inc, out = RD.touched(blocks, mask)
    only_in = np.setdiff1d(inc, out)
    kind, scale = RD.rule_of(segs, n)
    w = only_in[kind[only_in] == R.NORMAL]
    b = only_in[kind[only_in] == R.CONST]
    assert w.size and b.size == 6 and np.array_equal(p1[w], phi[w]) and not p1[b].any() and not p1[out].any(), "weights drawn, biases 0, outgoing 0 (also where both)"
    rest = np.setdiff1d(np.arange(n), both)
    assert np.array_equal(p1[rest], p[rest]) and np.array_equal(m1[rest], m[rest]) and np.array_equal(v1[rest], v[rest])
    assert not m1[both].any() and not v1[both].any() and m[both].all()
    assert RD.STREAM_REDO == 9


# ----------------------------------------------------------------------------------------------------------- the binding table and the library's checks
def test_stream_constant_and_declarations():
    from agent0_amd import _abi, ops
    from agent0_amd.common.utils import DeviceRng
    assert DeviceRng.STREAM_REDO == RD.STREAM_REDO == 9 and DeviceRng.STREAM_RESET == 8
    protos = {name: (ret, types) for ret, name, types in _abi.parse_header()}
    assert protos["a0_redo_score"] == ("int", ["ptr", "long long", "ptr", "long long", "ptr", "long long", "ptr", "long long", "double", "ptr", "int", "int", "ptr", "ptr", "ptr",
                                               "ptr", "ptr"])
    assert protos["a0_redo_recycle"] == ("int", ["ptr", "ptr", "ptr", "long long", "long long", "ptr", "int", "ptr", "ptr", "unsigned long long", "ptr", "int", "int", "long long",
                                                 "ptr", "int", "ptr", "ptr"])
    assert protos["a0_learner_set_redo"] == ("int", ["ptr", "int", "double", "int", "unsigned long long"]) and protos["a0_learner_redo_buffers"] == ("int", ["ptr"] * 4)
    assert len(protos["a0_net_reset"][1]) == 19 and protos["a0_learner_set_net_reset"] == ("int", ["ptr", "int", "double", "unsigned long long"]), "existing exports are what they were"
    lib = _abi.load()
    assert lib.a0_learner_set_redo.argtypes == [C.c_void_p, C.c_int, C.c_double, C.c_int, C.c_ulonglong]
    assert C.sizeof(_abi.RedoBlocks) == 56
    assert ops.HipOps.REDO_NEURONS == 672 and ops.HipOps.REDO_PARTIALS == 512
    for name in ("redo_score", "redo_recycle"):
        assert hasattr(ops.HipOps, name)
    assert hasattr(ops.NativeLearner, "set_redo") and hasattr(ops.NativeLearner, "redo_buffers")


def test_arguments_are_checked_before_any_launch():
    """Every refusal returns A0_EINVAL with a message before a pointer is used (the pointers here are never dereferenced on the device)."""
    from agent0_amd import _abi
    lib = _abi.load()
    buf = (C.c_float * 8192)()
    p = (C.addressof(buf) + 15) // 16 * 16
    q = [p + 4 * 512 * i for i in range(12)]

    def score(**kw):
        a = dict(a1=q[0], r1=1, a2=q[1], r2=1, a3=q[2], r3=1, h=q[3], r4=1, tau=0.1, state=q[4], freq=3, force=1, part=q[5], sc=q[6], mk=q[7], ct=q[8])
        a.update(kw)
        return lib.a0_redo_score(a["a1"], a["r1"], a["a2"], a["r2"], a["a3"], a["r3"], a["h"], a["r4"], a["tau"], a["state"], a["freq"], a["force"], a["part"], a["sc"], a["mk"],
                                 a["ct"], None)

    for bad in (dict(a1=None), dict(a2=None), dict(a3=None), dict(h=None), dict(part=None), dict(sc=None), dict(mk=None), dict(ct=None), dict(r1=0), dict(r4=-1),
                dict(state=None, force=0), dict(freq=-1)):
        assert score(**bad) == -1 and "a0_redo_score" in _abi.last_error(), bad
    for tau in (-0.1, 1.0, float("nan"), float("inf")):
        assert score(tau=tau) == -1 and "tau" in _abi.last_error(), tau
    assert score(a2=q[1] + 4) == -1 and "16-byte aligned" in _abi.last_error()
    assert score(part=q[5] + 4) == -1 and score(mk=q[7] + 2) == -1

    Seg, Blk = _abi.NetResetSeg, _abi.RedoBlocks
    good_blocks = (0, 32 * 64 + 32, 32 * 64 + 32 + 64 * 512 + 64, 100000, 200000, 64, 64, 32)

    def recycle(segs=((0, 64, 1, 0.1, 1),), blocks=good_blocks, **kw):
        a = dict(params=q[0], m=q[1], v=q[2], n_adam=300000, n_total=300004, mask=q[3], seed=1, state=q[4], freq=3, force=1, k=0, w=None, C=0, wt=None, blk=True)
        a.update(kw)
        tab = (Seg * max(1, len(segs)))(*[Seg(*s) for s in segs])
        b = Blk(*blocks)
        return lib.a0_redo_recycle(a["params"], a["m"], a["v"], a["n_adam"], a["n_total"], C.addressof(tab), len(segs), C.addressof(b) if a["blk"] else None, a["mask"], a["seed"],
                                   a["state"], a["freq"], a["force"], a["k"], a["w"], a["C"], a["wt"], None)

    for bad in (dict(params=None), dict(m=None), dict(v=None), dict(mask=None), dict(blk=False), dict(n_adam=0), dict(n_total=299999), dict(state=None, force=0), dict(freq=-1),
                dict(k=-1), dict(params=q[0] + 2), dict(mask=q[3] + 1)):
        assert recycle(**bad) == -1 and "a0_redo_recycle" in _abi.last_error(), bad
    assert recycle(segs=((0, 64, 1, 0.1, 1), (60, 32, 0, 0.0, 0))) == -1 and "a0_redo_recycle" in _abi.last_error() and "ascending" in _abi.last_error()
    assert recycle(segs=((0, 64, 3, 0.1, 1),)) == -1 and "kind" in _abi.last_error()
    for blocks in ((0, 0, 40000, 100000, 200000, 64, 64, 32),                 # conv2 on top of conv1
                   (0, 2080, 34912, 100000, 299000, 64, 64, 32),              # the head runs past n_adam
                   (0, 2080, 34912, 100000, 200000, 0, 64, 32), (0, 2080, 34912, 100000, 200000, 64, 65, 32), (0, 2080, 34912, 100000, 200000, 64, 64, 0)):
        assert recycle(blocks=blocks) == -1 and "a0_redo_recycle" in _abi.last_error(), blocks
    ew = _abi.EncoderWeights(q[0], q[0], q[0], q[0], q[0], q[0])
    assert recycle(wt=q[5], w=None, C=1) == -1 and recycle(wt=q[5] + 4, w=C.addressof(ew), C=1) == -1 and "16-byte aligned" in _abi.last_error()
    assert recycle(wt=q[5], w=C.addressof(ew), C=1) == -1 and "different convolution blocks" in _abi.last_error()
    assert lib.a0_learner_set_redo(None, 3, 0.1, 1, 1) == -1 and "a0_learner_set_redo" in _abi.last_error()
    assert lib.a0_learner_redo_buffers(None, None, None, None) == -1


# ----------------------------------------------------------------------------------------------------------- the statistics
TODAYS_HEADER = ["frames", "fraction_loss", "loss", "return_train", "return_train_max", "qmax", "fps"]
REDO_KEYS = ["dormant_frac", "dormant_frac_conv1", "dormant_frac_conv2", "dormant_frac_conv3", "dormant_frac_fc1"]


def _stub_trainer(tmp_path, tag, **eng):
    from agent0_amd.deepq.trainer import Trainer
    tr = Trainer.__new__(Trainer)
    e = dict(gnorm_ring=None, net_reset_freq=0, wd_partials=None, redo_freq=0, redo_counts=None, state=torch.tensor([0, 6, 0, 0, 0, 0, 6, 0], dtype=torch.int32))
    e.update(eng)
    tr.learner = types.SimpleNamespace(engine=types.SimpleNamespace(**e))
    tr.cfg = types.SimpleNamespace(logdir=str(tmp_path / tag))
    (tmp_path / tag).mkdir()
    tr.frame_count, tr.Ls, tr.FLs, tr.Rs, tr.Qs, tr.GNs, tr.PN, tr._nl = 64, [0.5], [], [1.0], [2.0], [], None, False
    tr.primary, tr.writer, tr._wandb = True, None, None
    tr.logger = logging.getLogger(f"redo-test-{tag}")
    tr.logger.setLevel(logging.INFO)
    tr.logger.addHandler(logging.FileHandler(tmp_path / tag / "msg.log"))
    return tr


def _logged(tr, tmp_path, tag):
    res = dict(tr._result(), fps=100.0)
    tr.logging(res)
    for h in tr.logger.handlers:
        h.flush()
    with open(tmp_path / tag / "progress.csv") as f:
        rows = list(csv.reader(f))
    return res, rows, open(tmp_path / tag / "msg.log").read()


def test_the_statistics_appear_only_with_the_setting_on(tmp_path):
    res, rows, log = _logged(_stub_trainer(tmp_path, "off"), tmp_path, "off")
    assert list(res) == TODAYS_HEADER and rows[0] == TODAYS_HEADER and "dormant" not in log

    counts = torch.tensor([0, 0, 0, 0, 0, -1, 0, 0], dtype=torch.int32)
    tr = _stub_trainer(tmp_path, "on", redo_freq=3, redo_counts=counts)
    res, rows, log = _logged(tr, tmp_path, "on")
    assert list(res) == TODAYS_HEADER[:-1] + REDO_KEYS + ["fps"] and all(math.isnan(res[k]) for k in REDO_KEYS), "NaN until the first evaluation"
    assert rows[0] == TODAYS_HEADER + REDO_KEYS
    counts.copy_(torch.tensor([2, 16, 0, 128, 146, 6, 0, 0], dtype=torch.int32))
    res, rows, log = _logged(tr, tmp_path, "on")
    assert [res[k] for k in REDO_KEYS] == [146 / 672, 2 / 32, 16 / 64, 0.0, 128 / 512]
    assert len(rows) == 3 and [float(x) for x in rows[2][-5:]] == [res[k] for k in REDO_KEYS]
    assert "dormant_frac: 0.217 | dormant_frac_conv1: 0.062 | dormant_frac_conv2: 0.250 | dormant_frac_conv3: 0.000 | dormant_frac_fc1: 0.250" in log

    # behind the other optional columns
    tr = _stub_trainer(tmp_path, "all", redo_freq=3, redo_counts=counts, net_reset_freq=3, wd_partials=torch.zeros(1), gnorm_ring=torch.zeros(1))
    res, rows, log = _logged(tr, tmp_path, "all")
    assert rows[0] == TODAYS_HEADER + ["grad_norm", "net_resets", "param_norm"] + REDO_KEYS
