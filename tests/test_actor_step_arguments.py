"""CPU: the eight merged actor-step entry points (tail + env step in one launch, csrc/actor_step.h) refuse bad arguments with A0_EINVAL and a message that starts with
the function's reporting name, before any HIP call: the pointers here are small fake integers that nothing may read.

The two `_wp` forms report under the names of the plain forms they serve.  Check order: head arguments, then the env commit, then the 16-byte alignment of the
observation buffers, then the head's width against LDS.  The env commit has thirteen pointers (obs_in, obs_out, ep_ret, final_mask, final_ret, the three n-step
rings, obs0, frames and the replay row's three arrays); each is tried null.

The three tails WITHOUT an env step (a0_actor_dist_tail, a0_actor_quantile_tail, a0_actor_qhead: the actor steps over host environments) take the head and the draw
alone and are held to the same: every pointer null, every range at its edge, the head's width against LDS, each under the function's own name."""
import pytest

EINVAL = -1
TASK_STREAM, TASK_CHASE = 0, 2
P = 0x10000                                           # 16-byte aligned stand-ins

DRAW = dict(seed=7, stream_a=1, stream_u=2, off_a=0, off_u=0, eps=0.1, ctrl=None, eps_ptr=None, action=20 * P, qmax=21 * P)
ENV = dict(env_seed=11, rank=0, g=1, obs_in=30 * P, obs_out=31 * P, ep_ret=32 * P, final_mask=33 * P, final_ret=34 * P, n=3, steps=0, gamma=0.99, ring_act=35 * P,
           ring_rew=36 * P, ring_done=37 * P, obs0=38 * P, frames=39 * P, cap=8, start_slot=0, r_act=40 * P, r_rew=41 * P, r_done=42 * P, task=TASK_STREAM)
ENV_POINTERS = ["obs_in", "obs_out", "ep_ret", "final_mask", "final_ret", "ring_act", "ring_rew", "ring_done", "obs0", "frames", "r_act", "r_rew", "r_done"]
NEXT_ENC = dict(wt=50 * P, w=51 * P, act3_next=52 * P)


def _slab_head(quantile):
    # E = 3, A = 4, T = 5, ld = 24, nslab = 2; c51 form: one row per env (mode 2 with atoms), iqn / fqf form: T rows per env (mode 3 with taus)
    return dict(slabs=1 * P, slab_stride=3 * 5 * 24 if quantile else 3 * 24, nslab=2, bias=2 * P, ld=24, A=4, T=5, dueling=0, mode=3 if quantile else 2, aux=3 * P, E=3)


def _scalar_head():
    return dict(feat=1 * P, E=3, K=3136, W1=2 * P, b1=3 * P, W2=4 * P, b2=5 * P, A=4, dueling=0, scratch=6 * P)


# name -> (reporting name, family, extra trailing arguments)
FUNCS = {
    "a0_actor_dist_tail_env_step": ("a0_actor_dist_tail_env_step", "dist", {}),
    "a0_actor_dist_tail_env_step_enc": ("a0_actor_dist_tail_env_step_enc", "dist", NEXT_ENC),
    "a0_actor_quantile_tail_env_step": ("a0_actor_quantile_tail_env_step", "quantile", {}),
    "a0_actor_quantile_tail_env_step_enc": ("a0_actor_quantile_tail_env_step_enc", "quantile", NEXT_ENC),
    "a0_actor_qhead_env_step": ("a0_actor_qhead_env_step", "scalar", {}),
    "a0_actor_qhead_env_step_wp": ("a0_actor_qhead_env_step", "scalar", dict(w1_planes=None)),
    "a0_actor_qhead_env_step_enc": ("a0_actor_qhead_env_step_enc", "scalar", NEXT_ENC),
    "a0_actor_qhead_env_step_enc_wp": ("a0_actor_qhead_env_step_enc", "scalar", dict(NEXT_ENC, w1_planes=None)),
}
SLAB = [f for f, v in FUNCS.items() if v[1] != "scalar"]
SCALAR = [f for f, v in FUNCS.items() if v[1] == "scalar"]


@pytest.fixture(scope="module")
def lib():
    from agent0_amd import _abi
    return _abi.load()


def _refused(lib, fn, **bad):
    """Calls `fn` with its valid arguments overridden by `bad`; asserts A0_EINVAL under the reporting name and returns the message."""
    from agent0_amd import _abi
    who, family, extra = FUNCS[fn]
    a = dict(_scalar_head() if family == "scalar" else _slab_head(family == "quantile"))
    a.update(DRAW)
    a.update(ENV)
    a.update(extra)
    a["stream"] = None
    assert set(bad) <= set(a), bad
    a.update(bad)
    assert getattr(lib, fn)(*a.values()) == EINVAL, (fn, bad)
    msg = _abi.last_error()
    assert msg.startswith(who + ":"), (fn, bad, msg)
    return msg


ENV_CASES = [{p: None} for p in ENV_POINTERS] + [dict(obs_out=ENV["obs_in"]), dict(n=0), dict(steps=-1), dict(cap=3 - 1), dict(start_slot=-1), dict(task=TASK_STREAM - 1),
                                                 dict(task=TASK_CHASE + 1), dict(task=TASK_CHASE, A=3)]


@pytest.mark.parametrize("bad", ENV_CASES, ids=lambda b: ",".join(f"{k}={v}" for k, v in b.items()))
@pytest.mark.parametrize("fn", list(FUNCS))
def test_env_commit_arguments(lib, fn, bad):
    assert "env argument" in _refused(lib, fn, **bad)


@pytest.mark.parametrize("buf", ["obs_in", "obs_out", "obs0", "frames"])
@pytest.mark.parametrize("fn", list(FUNCS))
def test_observation_buffers_must_be_16_byte_aligned(lib, fn, buf):
    assert "16-byte aligned" in _refused(lib, fn, **{buf: ENV[buf] + 4})


def _slab_head_cases(fn):
    q = FUNCS[fn][1] == "quantile"
    ld_min, ld_min_duel = (4, 5) if q else (20, 25)                      # A (+ 1) columns per (env, quantile) row, or A * T (+ T) per env row
    return [dict(nslab=0), dict(ld=ld_min - 1, dueling=0), dict(ld=ld_min_duel - 1, dueling=1), dict(slab_stride=(3 * 5 * 24 if q else 3 * 24) - 1),
            dict(mode=2 if q else 3), dict(aux=None)]                    # a mode of the other family; mode 3 without taus / mode 2 without atoms


@pytest.mark.parametrize("fn,bad", [(f, b) for f in SLAB for b in _slab_head_cases(f)], ids=lambda v: v if isinstance(v, str) else ",".join(f"{k}={x}" for k, x in v.items()))
def test_slab_head_arguments(lib, fn, bad):
    msg = _refused(lib, fn, **bad)
    assert "bad argument" in msg and "env argument" not in msg


@pytest.mark.parametrize("bad", [dict(K=6), dict(A=24, dueling=1), dict(A=25, dueling=0)], ids=lambda b: ",".join(f"{k}={v}" for k, v in b.items()))
@pytest.mark.parametrize("fn", SCALAR)
def test_scalar_head_arguments(lib, fn, bad):
    msg = _refused(lib, fn, **bad)
    assert "bad argument" in msg and "env argument" not in msg


@pytest.mark.parametrize("fn", [f for f in SCALAR if "_enc" in f])
def test_next_encode_needs_the_atari_feature_width(lib, fn):
    msg = _refused(lib, fn, K=3140)                                      # a multiple of 4: the plain forms take it
    assert "bad argument" in msg and "env argument" not in msg


@pytest.mark.parametrize("fn", SLAB)
def test_head_too_wide_for_lds(lib, fn):
    if FUNCS[fn][1] == "quantile":
        bad = dict(A=4, T=4096, slab_stride=3 * 4096 * 24)             # (A * T + T) * 4 bytes = 80 KB > 64 KB
    else:
        bad = dict(A=4, T=8200, ld=4 * 8200, slab_stride=3 * 4 * 8200)   # (A * T + T) * 4 bytes = 164000 > 160 KB
    assert "too wide" in _refused(lib, fn, **bad)


@pytest.mark.parametrize("fn", list(FUNCS))
def test_head_argument_is_reported_before_env_argument(lib, fn):
    head = dict(K=6) if FUNCS[fn][1] == "scalar" else dict(nslab=0)
    msg = _refused(lib, fn, obs_in=None, n=0, **head)
    assert "bad argument" in msg and "env argument" not in msg


# ---------------------------------------------------------------------------------------------- the tails without an env step
TAILS = {"a0_actor_dist_tail": "dist", "a0_actor_quantile_tail": "quantile", "a0_actor_qhead": "scalar"}
SLAB_TAILS = [f for f, v in TAILS.items() if v != "scalar"]


def _tail_refused(lib, fn, **bad):
    """Calls the tail `fn` (head arguments, the draw, the stream) with its valid arguments overridden by `bad`; asserts A0_EINVAL under its own name and returns the message."""
    from agent0_amd import _abi
    family = TAILS[fn]
    a = dict(_scalar_head() if family == "scalar" else _slab_head(family == "quantile"))
    a.update(DRAW)
    a["stream"] = None
    assert set(bad) <= set(a), bad
    a.update(bad)
    assert getattr(lib, fn)(*a.values()) == EINVAL, (fn, bad)
    msg = _abi.last_error()
    assert msg.startswith(fn + ":"), (fn, bad, msg)
    return msg


def _tail_cases(fn):
    if TAILS[fn] == "scalar":      # K: a multiple of 4; A + dueling rows of 512 floats in 48 KB of LDS  (E and K below 1 are not tried: a0_actor_qhead sizes fc1's split from
        # them in front of a0_actor_qhead_n's check)
        return [{p: None} for p in ("feat", "W1", "b1", "W2", "b2", "scratch", "action", "qmax")] + [dict(K=6), dict(A=0), dict(A=24, dueling=1), dict(A=25, dueling=0)]
    q = TAILS[fn] == "quantile"
    ld_min, ld_min_duel = (4, 5) if q else (20, 25)
    return [{p: None} for p in ("slabs", "bias", "action", "qmax")] + [dict(E=0), dict(A=0), dict(T=0), dict(nslab=0), dict(ld=ld_min - 1, dueling=0),
                                                                          dict(ld=ld_min_duel - 1, dueling=1), dict(slab_stride=(3 * 5 * 24 if q else 3 * 24) - 1), dict(mode=0),
                                                                          dict(mode=2 if q else 3), dict(mode=4), dict(aux=None)]


@pytest.mark.parametrize("fn,bad", [(f, b) for f in TAILS for b in _tail_cases(f)], ids=lambda v: v if isinstance(v, str) else ",".join(f"{k}={x}" for k, x in v.items()))
def test_tail_without_env_step_arguments(lib, fn, bad):
    assert "bad argument" in _tail_refused(lib, fn, **bad)


@pytest.mark.parametrize("fn", SLAB_TAILS)
def test_tail_without_env_step_takes_the_other_mode_without_its_table(lib, fn):
    """mode 1 (qr, iqn: a plain mean) needs neither atoms nor taus: with them null the call gets past the argument check and is refused for its width"""
    wide = dict(T=3277, slab_stride=3 * 3277 * 24) if TAILS[fn] == "quantile" else dict(T=2049, ld=4 * 2049, slab_stride=3 * 4 * 2049)
    assert _tail_refused(lib, fn, mode=1, aux=None, **wide) == fn + ": head too wide for LDS"


@pytest.mark.parametrize("fn", SLAB_TAILS)
def test_tail_without_env_step_head_too_wide_for_lds(lib, fn):
    if TAILS[fn] == "quantile":
        bad = dict(A=4, T=3277, slab_stride=3 * 3277 * 24)                 # a workgroup per env: (A * T + T) * 4 bytes = 65 540 > 64 KiB
    else:
        bad = dict(A=4, T=2049, ld=4 * 2049, slab_stride=3 * 4 * 2049)     # four envs per workgroup: 4 * (A * T + T) * 4 bytes = 163 920 > 160 KiB
    assert _tail_refused(lib, fn, **bad) == fn + ": head too wide for LDS"


@pytest.mark.parametrize("fn", SLAB_TAILS)
def test_tail_without_env_step_reports_an_argument_before_the_width(lib, fn):
    wide = dict(T=3277, slab_stride=3 * 3277 * 24) if TAILS[fn] == "quantile" else dict(T=2049, ld=4 * 2049, slab_stride=3 * 4 * 2049)
    assert _tail_refused(lib, fn, nslab=0, **wide) == fn + ": bad argument"
