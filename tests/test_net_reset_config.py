"""CPU: the host side of ``learner.net_reset_freq`` / ``learner.net_reset_shrink`` — the config keys, the value helper and its refusals, the rule table of
``NetLayout.reset_segments`` against the restatement in tests/net_reset_ref.py and against freshly constructed torch modules, the declarations in the binding
table, the library's argument checks (made in front of any launch), and the seed broadcast over a two-rank gloo group.  The GPU side is tests/test_gpu_net_reset.py."""
import ctypes as C
import math
import os
import sys
import types

import numpy as np
import pytest
import torch
import torch.multiprocessing as mp

import net_reset_ref as R

HERE = os.path.dirname(os.path.abspath(__file__))
LAYOUTS = [("dqn", 4, False, False), ("dqn", 18, True, False), ("c51", 4, True, True), ("c51", 6, True, True), ("iqn", 4, False, False), ("iqn", 9, True, False),
           ("fqf", 4, False, False), ("fqf", 3, True, False)]
IDS = ["dqn-4", "dqn-duel-18", "rainbow-lite-4", "rainbow-lite-6", "iqn-4", "iqn-duel-9", "fqf-4", "fqf-duel-3"]


def _layout(algo, A, dueling, noisy):
    from agent0_amd.deepq.layout import NetLayout
    return NetLayout(algo, A, dueling, noisy, 51, (4, 84, 84))


def test_config_keys_parse_and_round_trip():
    from agent0_amd.deepq import config
    from agent0_amd.deepq.config import from_dict, parse_overrides, to_dict
    cfg = parse_overrides([])
    assert cfg.learner.net_reset_freq == 0 and isinstance(cfg.learner.net_reset_freq, int)
    assert cfg.learner.net_reset_shrink == 1.0 and isinstance(cfg.learner.net_reset_shrink, float)
    cfg = parse_overrides(["learner.net_reset_freq=40000", "learner.net_reset_shrink=0.5"])
    assert cfg.learner.net_reset_freq == 40000 and cfg.learner.net_reset_shrink == 0.5
    with pytest.raises(Exception):
        parse_overrides(["learner.net_reset_freq=often"])
    with pytest.raises(Exception):
        parse_overrides(["learner.net_reset_shrink=half"])
    d = to_dict(cfg)
    assert d["learner"]["net_reset_freq"] == 40000 and d["learner"]["net_reset_shrink"] == 0.5
    back = from_dict(d)
    assert back.learner.net_reset_freq == 40000 and back.learner.net_reset_shrink == 0.5 and to_dict(back) == d
    old = from_dict({"learner": {"algo": "dqn"}}).learner
    assert old.net_reset_freq == 0 and old.net_reset_shrink == 1.0, "a dictionary written before the keys existed"
    from agent0.deepq import config as alias
    assert alias.LearnerConfig().net_reset_freq == 0 and alias.parse_overrides(["learner.net_reset_freq=7"]).learner.net_reset_freq == 7
    doc = config.__doc__
    assert "learner.net_reset_freq" in doc and "learner.net_reset_shrink" in doc and "reset_noise_freq" in doc and "40000" in doc


@pytest.mark.parametrize("freq,shrink,want", [(0, 1.0, (0, 1.0)), (None, None, (0, 1.0)), (0, 0.5, (0, 0.5)), (3, 0.5, (3, 0.5)), (40000, 0, (40000, 0.0)), (1, 1, (1, 1.0)),
                                              (5.0, 0.2, (5, 0.2))])
def test_the_value_helper(freq, shrink, want):
    import inspect
    from agent0_amd.deepq import engine
    got = engine.net_reset_value(freq, shrink, pipeline_target=False)
    assert got == want and isinstance(got[0], int) and isinstance(got[1], float)
    p = inspect.signature(engine.DeviceLearner.__init__).parameters
    assert p["net_reset_freq"].default == 0 and p["net_reset_shrink"].default == 1.0


@pytest.mark.parametrize("freq", [-1, -40000, 2.5, True])
def test_the_value_helper_refuses_a_bad_period_by_name(freq):
    from agent0_amd.deepq import engine
    with pytest.raises(ValueError, match=r"learner\.net_reset_freq"):
        engine.net_reset_value(freq, 0.5, pipeline_target=False)


@pytest.mark.parametrize("shrink", [-0.1, 1.0000001, 2, float("nan"), float("inf"), -float("inf")])
@pytest.mark.parametrize("freq", [0, 3])
def test_the_value_helper_refuses_a_bad_share_by_name(freq, shrink):
    from agent0_amd.deepq import engine
    with pytest.raises(ValueError, match=r"learner\.net_reset_shrink"):
        engine.net_reset_value(freq, shrink, pipeline_target=False)


def test_the_value_helper_refuses_the_pipelined_target_pass(monkeypatch):
    from agent0_amd.deepq import engine
    with pytest.raises(ValueError, match=r"learner\.net_reset_freq.*A0_PIPELINE_TARGET"):
        engine.net_reset_value(3, 0.5, pipeline_target=True)
    monkeypatch.setenv("A0_PIPELINE_TARGET", "1")
    with pytest.raises(ValueError, match=r"learner\.net_reset_freq.*A0_PIPELINE_TARGET"):
        engine.net_reset_value(3, 0.5)
    assert engine.net_reset_value(0, 0.5) == (0, 0.5), "off is off whatever the environment says"
    monkeypatch.setenv("A0_PIPELINE_TARGET", "0")
    assert engine.net_reset_value(3, 0.5) == (3, 0.5)


# ----------------------------------------------------------------------------------------------------------- the rule table
@pytest.mark.parametrize("spec", LAYOUTS, ids=IDS)
def test_segments_tile_the_adam_range_once(spec):
    L = _layout(*spec)
    segs = L.reset_segments()
    assert len(segs) <= 32
    at = 0
    for off, cnt, kind, scale, keep in segs:
        assert off == at and cnt > 0 and kind in (0, 1, 2) and keep in (0, 1) and math.isfinite(scale) and scale >= 0.0
        at = off + cnt
    assert at == L.n_adam, "exactly [0, n_adam): the fqf fraction net lies behind it"
    if L.algo == "fqf":
        assert L.blocks["frac"].offset == L.n_adam and all(off + cnt <= L.blocks["frac"].offset for off, cnt, *_ in segs)
    assert [(o, c, k, np.float32(s), kp) for o, c, k, s, kp in segs] == [(o, c, k, np.float32(s), kp) for o, c, k, s, kp in R.segments(L)], "the restatement agrees"
    # the encoder, and only the encoder, keeps a share
    assert all((keep == 1) == (off < L.conv_end) for off, cnt, kind, scale, keep in segs)
    # pad rows of the head blocks (weights and biases) are zero segments
    rule = np.full(L.n_adam, -1, np.int64)
    scale_of = np.zeros(L.n_adam)
    for off, cnt, kind, scale, keep in segs:
        rule[off:off + cnt] = kind
        scale_of[off:off + cnt] = scale
    for name, blk in L.blocks.items():
        if name.startswith("head"):
            real, N, K = blk.n_real, blk.N, blk.K
            pad_w = slice(blk.offset + real * K, blk.offset + N * K)
            pad_b = slice(blk.offset + N * K + real, blk.offset + N * K + N)
            for sl in (pad_w, pad_b):
                assert (rule[sl] == R.CONST).all() and (scale_of[sl] == 0.0).all(), name
            assert N > real, "these layouts all have padded head rows"
    # all block boundaries are multiples of four; only the real / pad boundary of noisy biases is not
    odd = [off for off, *_ in segs if off % 4]
    if L.noisy:
        assert odd and all(rule[off - 1] in (R.UNIFORM, R.CONST) for off in odd)
    else:
        assert not odd or all(off >= L.blocks["head"].offset + L.blocks["head"].N * 512 for off in odd)


@pytest.mark.parametrize("spec", LAYOUTS, ids=IDS)
def test_scales_are_those_of_a_freshly_constructed_network(spec):
    """Every normal segment's std == the RMS of the corresponding tensor of a new ConvEncoder / _Head (orthogonal initialisation fixes that RMS exactly): rtol 1e-3.
    Uniform bounds and sigma constants == NoisyLinear's."""
    from agent0_amd.deepq.config import parse_overrides
    from agent0_amd.deepq.model import ConvEncoder, NoisyLinear, _Head
    algo, A, dueling, noisy = spec
    L = _layout(*spec)
    torch.manual_seed(5)
    cfg = parse_overrides([f"learner.algo={algo}"])
    enc, head = ConvEncoder(L.C), _Head(L, cfg)
    rms = lambda t: float(t.detach().double().pow(2).mean().sqrt())
    by_off = {off: (cnt, kind, scale) for off, cnt, kind, scale, keep in L.reset_segments()}
    B = L.blocks
    checked = 0
    for name, conv in (("conv1", enc.convs[0]), ("conv2", enc.convs[2]), ("conv3", enc.convs[4])):
        cnt, kind, scale = by_off[B[name].offset]
        assert kind == R.NORMAL and cnt == conv.weight.numel() and scale == pytest.approx(rms(conv.weight), rel=1e-3), name
        assert by_off[B[name].offset + cnt] == (B[name].N, R.CONST, 0.0) and not conv.bias.detach().any()
        checked += 1
    if not noisy:
        want = [(B["fc1"].offset, head.first_dense.weight), (B["head"].offset, head.q_head.weight)]
        if dueling:
            want.append((B["head"].offset + L.Nq * 512, head.value_head.weight))
        if L.quantile:
            want.append((B["cos"].offset, head.cosine_emb[0].weight))
        for off, w in want:
            cnt, kind, scale = by_off[off]
            assert kind == R.NORMAL and cnt == w.numel() and scale == pytest.approx(rms(w), rel=1e-3), off
            checked += 1
        assert sum(1 for c, k, s in by_off.values() if k == R.NORMAL) == checked, "no normal segment without a tensor behind it"
        assert not any(k == R.UNIFORM for c, k, s in by_off.values())
    else:
        mods = [("fc1", 0, 512, head.first_dense), ("head", 0, L.Nq, head.q_head)] + ([("head", L.Nq, L.V, head.value_head)] if dueling else [])
        for blk, r0, rows, m in mods:
            assert isinstance(m, NoisyLinear)
            mu, sg = B[blk + ".mu"], B[blk + ".sigma"]
            bound = 1.0 / np.sqrt(m.in_features)
            cover = lambda off: next((c, k, s) for o, (c, k, s) in by_off.items() if o <= off < o + c)
            for off in (mu.offset + r0 * mu.K, mu.offset + mu.N * mu.K + r0):          # weight_mu, bias_mu: uniform in +-1 / sqrt(in)
                c, k, s = cover(off)
                assert k == R.UNIFORM and np.float32(s) == np.float32(bound)
            assert float(m.weight_mu.detach().abs().max()) <= bound and float(m.bias_mu.detach().abs().max()) <= bound
            c, k, s = cover(sg.offset + r0 * sg.K)
            assert k == R.CONST and np.float32(s) == m.weight_sigma.detach()[0, 0].numpy() and bool((m.weight_sigma == m.weight_sigma[0, 0]).all())
            c, k, s = cover(sg.offset + sg.N * sg.K + r0)
            assert k == R.CONST and np.float32(s) == m.bias_sigma.detach()[0].numpy() and c == rows, "0.4 / sqrt(out), out the module's own width"
        assert not any(k == R.NORMAL and o >= L.conv_end for o, (c, k, s) in by_off.items()), "under NoisyNet fc1 and the heads are NoisyLinear: no orthogonal draw"


def test_the_reference_blend_and_uniform():
    g = np.random.default_rng(4)
    n = 4096
    p = (g.standard_normal(n) * 0.05).astype(np.float32)
    phi = (g.standard_normal(n) * 0.025).astype(np.float32)
    segs = [(0, 1000, R.NORMAL, 0.025, 1), (1000, 24, R.CONST, 0.0, 1), (1024, 2000, R.NORMAL, 0.025, 0), (3024, 1000, R.CONST, 0.125, 0)]      # [4024, 4096): no rule
    for alpha in (0.0, 0.2, 0.5, 0.8, 1.0):
        want, exact, suspects = R.expect(p, phi, segs, alpha)
        assert np.array_equal(want[1024:3024], phi[1024:3024]) and (want[3024:4024] == np.float32(0.125)).all() and np.array_equal(want[4024:], p[4024:])
        if alpha == 1.0:
            assert np.array_equal(want[:1024], p[:1024]) and exact.all()
        elif alpha == 0.0:
            assert np.array_equal(want[:1000], phi[:1000]) and not want[1000:1024].any() and exact.all()
        else:
            f64 = phi[:1000].astype(np.float64) + np.float64(np.float32(alpha)) * (p[:1000] - phi[:1000]).astype(np.float32).astype(np.float64)
            assert np.array_equal(want[:1000], f64.astype(np.float32)) and not exact[:1024].any() and exact[1024:].all()
            lo, hi = np.minimum(p[:1000], phi[:1000]), np.maximum(p[:1000], phi[:1000])
            assert ((want[:1000] >= lo) & (want[:1000] <= hi)).all() and int(suspects.sum()) <= 2
    u = np.array([0.0, 0.5, 1.0 - 2.0 ** -24, 2.0 ** -24], np.float32)
    assert np.array_equal(R.uniform_fresh(0.25, u), np.array([-0.25, 0.0, 0.25 * (1.0 - 2.0 ** -23), 0.25 * (2.0 ** -23 - 1.0)], np.float32))


# ----------------------------------------------------------------------------------------------------------- the binding table and the library's checks
def test_stream_constant_and_declarations():
    from agent0_amd import _abi
    from agent0_amd.common.utils import DeviceRng
    assert DeviceRng.STREAM_RESET == R.STREAM_RESET == 8 and DeviceRng.STREAM_AUG == 7
    protos = {name: (ret, types) for ret, name, types in _abi.parse_header()}
    assert protos["a0_net_reset"] == ("int", ["ptr", "ptr", "ptr", "ptr", "long long", "long long", "ptr", "int", "double", "unsigned long long", "ptr", "int", "int",
                                              "long long", "ptr", "int", "ptr", "ptr", "ptr"])
    assert protos["a0_learner_set_net_reset"] == ("int", ["ptr", "int", "double", "unsigned long long"])
    # the existing exports are what they were
    assert len(protos["a0_adam_step_sync"][1]) == 16 and len(protos["a0_adam_step_sync_wt"][1]) == 24 and len(protos["a0_update_tail"][1]) == 22
    assert len(protos["a0_target_blend"][1]) == 11 and protos["a0_learner_set_target_tau"] == ("int", ["ptr", "double"])
    header = " ".join(open(_abi.HEADER).read().split())
    assert "[7] update_steps at the last network reset" in header and "t = max(1, update_steps - state[7])" in header
    assert os.path.exists(_abi.LIB_PATH), "build the library first: python -c 'import __graft_entry__ as g; g.build()'"
    lib = _abi.load()
    assert lib.a0_learner_set_net_reset.argtypes == [C.c_void_p, C.c_int, C.c_double, C.c_ulonglong] and len(lib.a0_net_reset.argtypes) == 19
    assert C.sizeof(_abi.NetResetSeg) == 32
    from agent0_amd import ops
    assert hasattr(ops.HipOps, "net_reset") and hasattr(ops.NativeLearner, "set_net_reset") and ops.HipOps.NET_RESET_MAX_SEGS == 32


def test_arguments_are_checked_before_any_launch():
    """Every refusal returns A0_EINVAL with a message before a pointer is used (the pointers here are never dereferenced on the device)."""
    from agent0_amd import _abi
    lib = _abi.load()
    buf = (C.c_float * 4096)()
    p = (C.addressof(buf) + 15) // 16 * 16
    t, m, v, st = p + 4 * 512, p + 4 * 1024, p + 4 * 1536, p + 4 * 2048
    Seg = _abi.NetResetSeg

    def call(segs=((0, 64, 1, 0.1, 1), (64, 32, 0, 0.0, 0)), **kw):
        a = dict(params=p, target=t, m=m, v=v, n_adam=100, n_total=128, alpha=0.5, seed=1, state=st, freq=3, force=1, k=0, w=None, C=0, wt=None, wt_t=None, n_segs=None)
        a.update(kw)
        tab = (Seg * max(1, len(segs)))(*[Seg(*s) for s in segs])
        n = len(segs) if a["n_segs"] is None else a["n_segs"]
        return lib.a0_net_reset(a["params"], a["target"], a["m"], a["v"], a["n_adam"], a["n_total"], C.addressof(tab), n, a["alpha"], a["seed"], a["state"], a["freq"],
                                a["force"], a["k"], a["w"], a["C"], a["wt"], a["wt_t"], None)

    for bad in (dict(params=None), dict(target=None), dict(m=None), dict(v=None), dict(n_adam=0), dict(n_total=99), dict(state=None, force=0), dict(freq=-1), dict(k=-1),
                dict(params=p + 2), dict(v=v + 1)):
        assert call(**bad) == -1 and "a0_net_reset" in _abi.last_error(), bad
    for alpha in (-0.1, 1.5, float("nan"), float("inf")):
        assert call(alpha=alpha) == -1 and "alpha" in _abi.last_error(), alpha
    assert call(n_segs=33) == -1 and call(n_segs=-1) == -1
    for segs in (((0, 64, 1, 0.1, 1), (60, 32, 0, 0.0, 0)),          # overlap
                 ((64, 32, 0, 0.0, 0), (0, 64, 1, 0.1, 1)),          # not ascending
                 ((0, 101, 1, 0.1, 1),),                             # past n_adam
                 ((0, 0, 1, 0.1, 1),), ((-4, 8, 1, 0.1, 1),)):
        assert call(segs=segs) == -1 and "ascending" in _abi.last_error(), segs
    assert call(segs=((0, 64, 3, 0.1, 1),)) == -1 and "kind" in _abi.last_error()
    assert call(segs=((0, 64, 1, float("nan"), 1),)) == -1 and call(segs=((0, 64, 1, float("inf"), 1),)) == -1 and call(segs=((0, 64, 1, 0.1, 2),)) == -1
    ew = _abi.EncoderWeights(p, p, p, p, p, p)
    assert call(wt=m, wt_t=None, w=C.addressof(ew), C=4) == -1 and call(wt=m, wt_t=v, w=None, C=4) == -1 and call(wt=m, wt_t=v, w=C.addressof(ew), C=0) == -1
    assert call(wt=m + 4, wt_t=v, w=C.addressof(ew), C=4) == -1 and "16-byte aligned" in _abi.last_error()
    assert call(wt=m, wt_t=v, w=C.addressof(ew), C=4) == -1 and "inside params" in _abi.last_error()
    assert lib.a0_learner_set_net_reset(None, 3, 0.5, 1) == -1 and "a0_learner_set_net_reset" in _abi.last_error()


# ----------------------------------------------------------------------------------------------------------- the seed under data parallelism
def _engine_stub(seed):
    from agent0_amd.deepq.engine import DeviceLearner
    eng = types.SimpleNamespace(net_reset_freq=3, net_reset_seed=None, aug_rng=types.SimpleNamespace(seed=seed))
    eng.reset_seed = types.MethodType(DeviceLearner.reset_seed, eng)
    return eng


def _seed_worker(rank, world, port, out):
    sys.path.insert(0, os.path.dirname(HERE))
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), RANK=str(rank), WORLD_SIZE=str(world), LOCAL_RANK=str(rank))
    import torch.distributed as dist
    from agent0_amd.deepq.dist import init_process_group
    from agent0_amd.deepq.launch import TrainerNode

    init_process_group(backend="gloo")
    # launch.py: cfg.seed + 1000003 * rank per rank; BaseLearner: DeviceRng(cfg.seed + 15485863), whose seed keeps the low 32 bits
    own = ((42 + 1000003 * rank) + 15485863) & 0xFFFFFFFF
    node = TrainerNode.__new__(TrainerNode)
    eng = _engine_stub(own | (7 << 32))                      # bits above 32 never travel
    node.trainer = types.SimpleNamespace(learner=types.SimpleNamespace(engine=eng))
    first_own = eng.reset_seed()
    node.share_reset_seed(world)
    first = eng.reset_seed()
    eng.aug_rng.seed = (1234 + 99 * rank) | (3 << 32)        # load_snapshot brings another seed; the hook shares rank 0's again
    node.share_reset_seed(world)
    off = _engine_stub(own)
    off.net_reset_freq = 0
    node.trainer.learner.engine = off
    node.share_reset_seed(world)                             # setting off: no collective, nothing set
    out[rank] = (own, first_own, first, eng.reset_seed(), off.net_reset_seed)
    dist.barrier()
    dist.destroy_process_group()


def test_two_ranks_end_with_rank_zeros_reset_seed():
    import socket
    with socket.socket() as sk:
        sk.bind(("127.0.0.1", 0))
        port = sk.getsockname()[1]
    mgr = mp.Manager()
    out = mgr.dict()
    mp.spawn(_seed_worker, args=(2, port, out), nprocs=2, join=True)
    res = dict(out)
    assert res[0][0] != res[1][0] and res[0][1] == res[0][0] and res[1][1] == res[1][0], "every rank starts on its own seed, 32 bits of it"
    assert res[0][2] == res[1][2] == res[0][0], "rank 0's seed on both"
    assert res[0][3] == res[1][3] == 1234, "and again after a load"
    assert res[0][4] is None and res[1][4] is None
    from agent0_amd.deepq.launch import broadcast_reset_seed
    assert broadcast_reset_seed((5 << 32) | 17, 1) == 17, "one rank: no process group needed"
