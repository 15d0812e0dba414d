"""GPU (MI355X): the actor's dedicated fc1 kernel (agent0_amd/csrc/actor_fc1.hip) against the general split-K GEMM it stands in for.

a0_actor_fc1 forms, per slab element, the same six bf16 products per 16 k in the same order into the same fp32 accumulator as a0_dense_fwd_partial: every comparison
here is ``torch.equal`` — there is no tolerance to choose.  The weights reach it as three bf16 term planes in MFMA-fragment order (a0_actor_fc1_planes):
int32 [N / 32][K / 16][3 terms][64 lanes][4 words], word w of lane l = the bf16 pair k = 16 ks + 8 (l >> 5) + 2 w, + 1 (low half first) of row 32 nb + (l & 31)."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

N = 512
ROWS = [1, 63, 64, 65, 96, 256]      # one row; the 64-row tile's edge from both sides; two tiles, one ragged; the actor's batch (1 / 1 / 1 / 2 / 2 / 4 row tiles, 32 / 16 / 8 slabs)
KS = [3136, 64]                      # 84 x 84 and 36 x 36 observations (98 k tiles over 8 - 32 slabs with empty ones at 64 and 96 rows; 2 k tiles in one slab)


@pytest.fixture(scope="module")
def hip():
    from agent0_amd.ops import HipOps
    return HipOps()


def _weights(hip, K, seed):
    """W [512][K]: normal values scaled over 24 binades per row block, a block of rows around 2^-120 (the third term of those is a bf16 denormal) and exact zeros."""
    g = torch.Generator(device="cpu").manual_seed(seed)
    W = torch.randn(N, K, generator=g)
    W *= torch.exp2(torch.randint(-20, 5, (N, 1), generator=g).float())
    W[96:128] *= 2.0 ** -120
    W[torch.rand(N, K, generator=g) < 0.02] = 0.0
    return W.to(hip.device).contiguous()


def _features(hip, R, K, kind, seed):
    g = torch.Generator(device="cpu").manual_seed(seed)
    X = torch.randn(R, K, generator=g) * torch.exp2(torch.randint(-6, 7, (R, K), generator=g).float())
    if kind == "relu":
        X = torch.relu(X - 0.5)       # about two thirds exact zeros, the rest positive: what the encoder's last ReLU hands fc1
    return X.to(hip.device).contiguous()


def _planes(hip, W, K):
    planes = torch.empty(hip.actor_fc1_planes_words(N, K), dtype=torch.int32, device=hip.device)
    hip.actor_fc1_planes(W, planes, N, K)
    return planes


def _terms(planes, K):
    """The fragment-ordered buffer back as three fp32 matrices [3][512][K]."""
    p = planes.view(N // 32, K // 16, 3, 64, 4).cpu().numpy().astype(np.int64) & 0xFFFFFFFF
    halves = np.stack([p & 0xFFFF, p >> 16], axis=-1)                                   # [nb][ks][term][lane][word][half]
    bits = (halves << 16).astype(np.uint32).view(np.float32)
    out = np.zeros((3, N, K), dtype=np.float32)
    for lane in range(64):
        n = np.arange(N // 32) * 32 + (lane & 31)
        for ks in range(K // 16):
            k0 = ks * 16 + 8 * (lane >> 5)
            out[:, n, k0:k0 + 8] = bits[:, ks, :, lane].reshape(N // 32, 3, 8).transpose(1, 0, 2)
    return out


@pytest.mark.parametrize("K", KS)
@pytest.mark.parametrize("R", ROWS)
def test_slabs_equal_the_general_kernels(hip, R, K):
    assert hip.actor_fc1_ok(R, N, K)
    W = _weights(hip, K, 7 * K + 1)
    planes = _planes(hip, W, K)
    ns = hip.dense_fwd_partial_slabs(R, N, K)
    for kind in ("signed", "relu"):
        X = _features(hip, R, K, kind, 31 * R + K)
        want = torch.full((ns, R, N), float("nan"), device=hip.device)
        got = torch.full((ns, R, N), float("nan"), device=hip.device)
        assert hip.dense_fwd_partial(X, K, W, R, N, K, want) == ns
        assert hip.actor_fc1(X, K, planes, R, N, K, got) == ns
        assert not torch.isnan(got).any(), "every slab element is written (empty k ranges as zeros)"
        assert torch.equal(got, want), f"R={R} K={K} {kind}: {(got != want).sum().item()} of {got.numel()} slab elements differ"
        assert (want[:, :, 96:128] != 0).any(), "the tiny rows of W reach the slabs"


def test_slabs_equal_at_a_callers_split_count(hip):
    """a0_actor_fc1_n: 16 slabs over 256 rows, the split the distributional actors' a0_dense_fwd forms."""
    R, K = 256, 3136
    W, X = _weights(hip, K, 5), _features(hip, R, K, "relu", 6)
    planes = _planes(hip, W, K)
    want = torch.empty(16, R, N, device=hip.device)
    got = torch.empty(16, R, N, device=hip.device)
    hip.dense_fwd_partial_n(X, K, W, R, N, K, 16, want)
    hip.actor_fc1(X, K, planes, R, N, K, got, splits=16)
    assert torch.equal(got, want)


@pytest.mark.parametrize("K", KS)
def test_planes_are_the_exact_terms(hip, K):
    g = torch.Generator(device="cpu").manual_seed(K)
    W = (torch.randn(N, K, generator=g) * torch.exp2(torch.randint(-20, 5, (N, K), generator=g).float())).to(hip.device).contiguous()
    planes = _planes(hip, W, K)
    t = _terms(planes, K)
    w = W.cpu().numpy()
    assert np.array_equal((t[0] + t[1]) + t[2], w), "hi + mid + lo == W in fp32, every element"
    assert np.all(np.abs(t[1]) <= np.abs(t[0]) * 2.0 ** -7) and np.all(np.abs(t[2]) <= np.abs(t[0]) * 2.0 ** -15)
    # the same terms a0_split_planes writes in its own layout [n][K / 4][hi hi | mid mid | lo lo]
    flat = torch.empty(hip.weight_planes_words(N, K), dtype=torch.int32, device=hip.device)
    hip.split_planes(W, flat, N, K)
    q = flat.view(N, K // 4, 3, 2).cpu().numpy().astype(np.int64) & 0xFFFFFFFF
    ref = (np.stack([q & 0xFFFF, q >> 16], axis=-1) << 16).astype(np.uint32).view(np.float32)      # [n][k4][term][word][half]
    assert np.array_equal(ref.transpose(2, 0, 1, 3, 4).reshape(3, N, K), t)
    # one changed element changes the planes after a refresh — and nothing before it
    before = planes.clone()
    W[300, K - 3] = 1.2345
    assert torch.equal(planes, before)
    hip.actor_fc1_planes(W, planes, N, K)
    changed = (planes != before).nonzero().flatten()
    assert 1 <= changed.numel() <= 3
    assert _terms(planes, K)[:, 300, K - 3].astype(np.float64).sum() == float(np.float32(1.2345))


@pytest.mark.parametrize("R,n,K", [(257, 512, 3136), (256, 256, 3136), (256, 512, 3120), (0, 512, 3136)])
def test_rejected_shapes_are_refused(hip, R, n, K):
    """What a0_actor_fc1_ok rejects the kernel does not run: the entry point fails instead of writing anything (callers keep a0_dense_fwd_partial there)."""
    from agent0_amd._abi import A0Error
    assert not hip.actor_fc1_ok(R, n, K)
    if R < 1:
        return
    X = torch.zeros(R, K, device=hip.device)
    planes = torch.zeros(max(1, hip.actor_fc1_planes_words(n, K)), dtype=torch.int32, device=hip.device)
    slabs = torch.full((hip.dense_fwd_partial_slabs(R, n, K), R, n), 3.0, device=hip.device)
    with pytest.raises(A0Error):
        hip.actor_fc1(X, K, planes, R, n, K, slabs)
    assert (slabs == 3.0).all()


def test_rejected_modes(hip):
    """The strict nine-product form and the fp32-chain kernel are other sums: not this kernel's."""
    prev = hip.lib.a0_x9_products(9)
    try:
        assert not hip.actor_fc1_ok(256, N, 3136)
    finally:
        hip.lib.a0_x9_products(prev)
    prev = hip.gemm_mode(0)
    try:
        assert not hip.actor_fc1_ok(256, N, 3136)
    finally:
        hip.gemm_mode(prev)
    assert hip.actor_fc1_ok(256, N, 3136)


def _make_cfg(algo, E, logdir, **kw):
    from agent0_amd.deepq.config import parse_overrides
    cfg = parse_overrides([f"learner.algo={algo}", f"actor.num_envs={E}", "wandb=false", "tb=false", f"logdir={logdir}"] + [f"{k}={v}" for k, v in kw.items()])
    cfg.obs_shape = (4, 84, 84)
    cfg.action_dim = 4
    return cfg


def _rollouts(algo, fc1_planes, native, monkeypatch, logdir, launch=False, **extra):
    """Three iterations (rollouts of 96 envs x 6 steps, updates between them, so the weights change from rollout to rollout) through the library's actor handle
    (``native``) or the Python classes' Actor, with fc1 on a0_actor_fc1_kernel or (``Actor.fc1_planes = False``) on the general GEMM: everything a rollout writes, and
    the number of steps whose fc1 took the kernel."""
    from agent0_amd.deepq.native_loop import NativeLoop
    from agent0_amd.deepq.trainer import Trainer
    monkeypatch.setenv("A0_NATIVE_LOOP", "1" if native else "0")
    cfg = _make_cfg(algo, 96, logdir, **{"actor.sample_steps": 6, "replay.size": 2304, "learner.batch_size": 32, "learner.learner_steps": 3, "trainer.training_start_steps": 500,
                                         "learner.target_update_freq": 4, "trainer.exploration_steps": 3000, **extra})
    tr = Trainer(cfg, use_lp=launch)
    tr.actors[1].fc1_planes = fc1_planes
    res = [{k: v for k, v in tr.run_iteration(prefetch=(i % 2 == 0)).items() if k != "fps"} for i in range(3)]
    if native:
        assert isinstance(tr._nl, NativeLoop), getattr(tr, "native_loop_reason", None)
        launches = int(tr._nl.lib.a0_actor_fc1_launches(tr._nl.actor))
    else:
        assert tr._nl is False
        launches = int(tr.actors[1].fc1_launches)
    tr.test = lambda: None
    tr.final(save=False)
    torch.cuda.synchronize()
    eng, rp = tr.learner.engine, tr.replay
    return (res, list(tr.Qs), list(tr.Rs), [t.clone() for t in (rp.frames, rp.act, rp.rew, rp.done, eng.online.flat, eng.adam_m)]), launches


def _lib():
    from agent0_amd import _abi
    return _abi.load()


def _same(a, b):
    assert a[0] == b[0] and a[1] == b[1] and a[2] == b[2]
    for i, (x, y) in enumerate(zip(a[3], b[3])):
        assert torch.equal(x, y), f"tensor {i}"


CASES = [("dqn", {}), ("c51", {}), ("qr", {}), ("mdqn", {"learner.dueling_head": "true"}), ("dqn", {"learner.noisy_net": "true", "learner.reset_noise_freq": 4}),
         ("c51", {"learner.noisy_net": "true", "learner.reset_noise_freq": 4}), ("dqn", {"_launch": True}), ("c51", {"_launch": True})]
IDS = ["dqn", "c51", "qr", "mdqn-dueling", "dqn-noisy", "c51-noisy", "dqn-launch", "c51-launch"]


@pytest.mark.parametrize("native", [True, False], ids=["handle", "classes"])
@pytest.mark.parametrize("algo,extra", CASES, ids=IDS)
def test_rollouts_equal_with_and_without_the_kernel(algo, extra, native, monkeypatch, tmp_path):
    """Both host paths — the library's actor handle and the Python classes' Actor — with fc1 on a0_actor_fc1_kernel (planes laid out at every rollout start, and after
    every noise reset: 6 steps at a reset every 4 cross one inside a rollout and start the next off a reset) against the same rollouts on the general GEMM: replay
    ring, statistics, parameters byte for byte.  A stale plane — a missed refresh after an update, a weight snapshot (launch schedule) or a noise reset — acts on other
    weights and shows in the ring.  The run with the kernel must have taken it in every step of its rollouts, the other in none."""
    extra = dict(extra)
    launch = bool(extra.pop("_launch", False))
    on, n_on = _rollouts(algo, True, native, monkeypatch, tmp_path / "on", launch, **extra)
    off, n_off = _rollouts(algo, False, native, monkeypatch, tmp_path / "off", launch, **extra)
    assert n_on >= 6 and n_on % 6 == 0 and n_off == 0, (n_on, n_off)      # (the classes replay a captured rollout: its steps are counted once)
    _same(on, off)


@pytest.mark.parametrize("native", [True, False], ids=["handle", "classes"])
@pytest.mark.parametrize("algo", ["dqn", "c51"])
def test_rollouts_fall_back_where_the_kernel_does_not_apply(algo, native, monkeypatch, tmp_path):
    """Fallback: under the strict nine-product GEMM a0_actor_fc1_ok rejects every shape — a rollout that was offered the planes keeps the general GEMM in every step
    and equals the rollout that was not, byte for byte (planes read under nine products would be a six-product sum: other bits)."""
    lib = _lib()
    prev = lib.a0_x9_products(9)
    try:
        on, n_on = _rollouts(algo, True, native, monkeypatch, tmp_path / "on")
        off, n_off = _rollouts(algo, False, native, monkeypatch, tmp_path / "off")
    finally:
        lib.a0_x9_products(prev)
    assert n_on == 0 and n_off == 0
    _same(on, off)
    six, n_six = _rollouts(algo, True, native, monkeypatch, tmp_path / "six")
    assert n_six > 0
    assert not all(torch.equal(x, y) for x, y in zip(six[3], on[3])), "nine and six products are different sums: the comparison above can tell them apart"
