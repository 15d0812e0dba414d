"""GPU (MI355X): the two pairs of entry points that run ONE body with their own or a caller's split count (agent0_amd/csrc/dense.hip, actor_tail.hip).

a0_dense_fwd_partial is a0_dense_fwd_partial_n at the count a0_dense_fwd_partial_slabs tells, and a0_actor_qhead is a0_actor_qhead_n at the count its scratch size
tells: the same launches on the same arguments, so every comparison is ``torch.equal`` on the slab buffers, pre-filled with NaN so that an unwritten element shows.
Shapes: the smallest at which each arm is taken — R = 3 / 256 / 257 (the 64 x 64 fc1 tile, its last row count, the 128 x 64 tile), N = 8 (the narrow tile, a0_dense_fwd's
split rule) and 64 (the fc1 split rule), K = 136 (a ragged last k tile, at most 2 slabs), rows of X four floats apart from packed."""
import pytest
import torch

import recipe

pytestmark = pytest.mark.gpu

K = 136


@pytest.fixture(scope="module")
def hip():
    from agent0_amd.ops import HipOps
    return HipOps()


def _normal(hip, seed, *shape):
    return torch.from_numpy(recipe.gen(seed).standard_normal(shape, dtype="float32")).to(hip.device)


@pytest.mark.parametrize("N", [8, 64])
@pytest.mark.parametrize("R", [3, 256, 257])
def test_partial_is_partial_n_at_its_own_count(hip, R, N):
    ldx = K + 4
    X, W = _normal(hip, 1000 * R + N, R, ldx), _normal(hip, 1000 * R + N + 1, N, K)
    ns = hip.dense_fwd_partial_slabs(R, N, K)
    assert 1 <= ns <= 2
    own = torch.full((ns, R, N), float("nan"), device=hip.device)
    given = torch.full((ns, R, N), float("nan"), device=hip.device)
    assert hip.dense_fwd_partial(X, ldx, W, R, N, K, own) == ns
    assert hip.dense_fwd_partial_n(X, ldx, W, R, N, K, ns, given) == ns
    assert not torch.isnan(own).any() and not torch.isnan(given).any(), "every slab element is written"
    assert torch.equal(own, given), f"R={R} N={N}: {(own != given).sum().item()} of {own.numel()} slab elements differ"


@pytest.mark.parametrize("A,dueling", [(3, False), (24, False), (23, True)])
def test_qhead_is_qhead_n_at_its_own_count(hip, A, dueling):
    E, nq = 5, A + (1 if dueling else 0)
    feat, W1, b1 = _normal(hip, 7000 + A, E, K), _normal(hip, 7100 + A, 512, K), _normal(hip, 7200 + A, 512)
    W2, b2 = _normal(hip, 7300 + A, nq, 512), _normal(hip, 7400 + A, nq)
    words = hip.actor_qhead_scratch(E, K)
    splits = words // (E * 512)
    assert splits >= 1 and splits * E * 512 == words
    out = []
    for form in ("own", "given"):
        scratch = torch.full((words,), float("nan"), device=hip.device)
        action = torch.full((E,), -1, dtype=torch.int32, device=hip.device)
        qmax = torch.full((E,), float("nan"), device=hip.device)
        draw = (11, 1, 2, 0, 0, 0.0, action, qmax)      # eps = 0: no draw decides
        if form == "own":
            hip.actor_qhead(feat, E, K, W1, b1, W2, b2, A, dueling, scratch, *draw)
        else:
            hip.actor_qhead_n(feat, E, K, splits, W1, b1, W2, b2, A, dueling, scratch, *draw)
        assert not torch.isnan(scratch).any() and not torch.isnan(qmax).any() and (action >= 0).all() and (action < A).all()
        out.append((scratch, action, qmax))
    for name, own, given in zip(("fc1 slabs", "action", "qmax"), *out):
        assert torch.equal(own, given), f"A={A} dueling={dueling}: {name} differ"
