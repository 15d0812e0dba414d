"""GPU (MI355X): the ingest half of a host-env step in one launch (a0_host_step_ingest) and the DMA-only form of a0_env_pool_upload.

The kernel must leave, byte for byte, what the launches Actor._rollout_host composes today leave: a0_env_frame_stack, the observation ring copy (n > 1),
a0_actor_nstep, a0_replay_insert and the two statistics copies — over consecutive steps, so that the n-step window and the observation ring carry history."""
import ctypes as C

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

N_SCAL, ADV = 7, 6


@pytest.fixture(scope="module")
def hip():
    from agent0_amd.ops import HipOps
    return HipOps()


def _scalars(g, E, adv_p=0.7):
    """[N_SCAL][E] f32 in env_pool's order, every terminal / truncated / life-loss combination likely at E >= 16."""
    s = np.zeros((N_SCAL, E), np.float32)
    s[0] = np.where(g.random(E) < 0.5, g.integers(-1, 2, E), g.standard_normal(E))
    s[1] = g.random(E) < 0.3
    s[2] = g.random(E) < 0.3
    s[3] = g.random(E) < 0.3
    s[4] = g.random(E) < 0.2
    s[5] = g.standard_normal(E) * s[4]
    s[ADV] = g.random(E) < adv_p
    s[ADV, 0] = 0.0
    s[ADV, -1] = 1.0
    return s


def _state(hip, E, n, R, ob, cap):
    z = lambda *a, **k: torch.zeros(*a, device=hip.device, **k)
    return dict(ring_act=z(n * E, dtype=torch.int32), ring_rew=z(n * E), ring_done=z(n * E), ring_obs=z(R * E * ob, dtype=torch.uint8),
                frames=z(cap * 2 * ob, dtype=torch.uint8), r_act=z(cap, dtype=torch.int32), r_rew=z(cap), r_done=z(cap), stat_mask=z(E), stat_ret=z(E))


@pytest.mark.parametrize("E,n,life,fb,use_ctrl", [(16, 1, True, 7056, False), (16, 3, True, 7056, False), (37, 3, False, 64, False), (256, 1, False, 7056, False),
                                                  (16, 3, True, 7056, True)])
def test_ingest_equals_the_composed_launches(hip, E, n, life, fb, use_ctrl):
    g = np.random.default_rng(E * 7 + n + fb)
    nstack, gamma = 4, 0.99
    ob = nstack * fb
    R = n + 1 if n > 1 else 1                       # Actor.ring_len for a rollout length that n + 1 divides
    cap = 3 * E + 5                                 # rows of step 2 wrap the ring
    steps0 = 0
    ctrl = None
    if use_ctrl:                                    # a captured sequence: steps and the replay slot advance through the control block
        ctrl = torch.zeros(8, dtype=torch.int64, device=hip.device)
        ctrl[1], ctrl[4] = 4, 2 * E
    a, b = _state(hip, E, n, R, ob, cap), _state(hip, E, n, R, ob, cap)
    obs = [torch.from_numpy(g.integers(0, 256, E * ob, dtype=np.uint8)).to(hip.device), None]
    obs_a, obs_b = obs[0].clone(), obs[0].clone()
    start = cap - E // 2
    for t in range(5):
        newest = torch.from_numpy(g.integers(0, 256, E * fb, dtype=np.uint8)).to(hip.device)
        scal = torch.from_numpy(_scalars(g, E)).to(hip.device)
        action = torch.from_numpy(g.integers(0, 18, E, dtype=np.int32)).to(hip.device)
        whole = torch.from_numpy(g.integers(0, 256, E * ob, dtype=np.uint8)).to(hip.device)     # what the DMA put into the rows uploaded whole
        keep = (scal[ADV] == 0).repeat_interleave(ob)
        nxt_a = torch.where(keep, whole, torch.full_like(whole, 3))
        nxt_b = nxt_a.clone()
        steps = steps0 + t
        slot = (start + t * E) % cap
        # the ingest launch
        hip.host_step_ingest(obs_a, newest, scal, nxt_a, E, nstack, fb, life, action, n, R, steps, gamma, a["ring_act"], a["ring_rew"], a["ring_done"],
                             a["ring_obs"] if n > 1 else None, a["frames"], cap, slot, a["r_act"], a["r_rew"], a["r_done"], a["stat_mask"], a["stat_ret"], ctrl)
        # the composition of Actor._rollout_host / HostEnvPool._upload
        hip.env_frame_stack(obs_b, newest, scal[ADV], nxt_b, E, nstack, fb)
        b["stat_mask"].copy_(scal[4])
        b["stat_ret"].copy_(scal[5])
        s_eff = steps + (4 if use_ctrl else 0)
        if n > 1:
            rs = s_eff % R
            b["ring_obs"][rs * E * ob:(rs + 1) * E * ob].copy_(obs_b)
            oldest = (s_eff - (min(s_eff + 1, n) - 1)) % R
            obs0 = b["ring_obs"][oldest * E * ob:(oldest + 1) * E * ob]
        else:
            obs0 = obs_b
        out_act, out_rew, out_done = torch.zeros(E, dtype=torch.int32, device=hip.device), torch.zeros(E, device=hip.device), torch.zeros(E, device=hip.device)
        hip.actor_nstep(E, n, steps, gamma, action, scal[0], scal[1], scal[2], scal[3] if life else None, b["ring_act"], b["ring_rew"], b["ring_done"],
                        out_act, out_rew, out_done, ctrl)
        hip.replay_insert(b["frames"], cap, ob, slot, E, obs0, nxt_b, out_act, out_rew, out_done, b["r_act"], b["r_rew"], b["r_done"], ctrl)
        torch.cuda.synchronize()
        assert torch.equal(nxt_a, nxt_b), f"step {t}: observation"
        for k in a:
            if k == "ring_obs" and n == 1:
                continue
            assert torch.equal(a[k], b[k]), f"step {t}: {k}"
        obs_a, obs_b = nxt_a, nxt_b
    assert int(a["r_done"].sum()) > 0 and int((a["r_act"] != 0).sum()) > 0          # the window emitted dones and actions, not only zeros


def test_pool_upload_dma_only(hip):
    """prev = NULL: newest frames, scalars and the whole stacks arrive; the advanced rows of `out` are left for the ingest kernel."""
    from agent0_amd._abi import A0Error, check
    from agent0_amd.ops import _stream
    g = np.random.default_rng(5)
    E, nstack, fb = 24, 4, 7056
    ob = nstack * fb
    scal = _scalars(g, E)
    newest, host_obs = g.integers(0, 256, (E, fb), dtype=np.uint8), g.integers(0, 256, (E, ob), dtype=np.uint8)
    pin = lambda x: torch.from_numpy(np.ascontiguousarray(x)).pin_memory()
    new_h, scal_h, obs_h = pin(newest), pin(scal), pin(host_obs)
    new_d, scal_d = torch.zeros(E * fb, dtype=torch.uint8, device=hip.device), torch.zeros(N_SCAL, E, device=hip.device)
    out = torch.full((E, ob), 5, dtype=torch.uint8, device=hip.device)
    n_whole = C.c_int(-1)
    check(hip.lib.a0_env_pool_upload(new_h.data_ptr(), new_d.data_ptr(), scal_h.data_ptr(), scal_d.data_ptr(), N_SCAL, ADV, obs_h.data_ptr(), None, out.data_ptr(),
                                     E, nstack, fb, C.byref(n_whole), _stream()), "a0_env_pool_upload")
    torch.cuda.synchronize()
    adv = scal[ADV] != 0
    assert n_whole.value == int((~adv).sum())
    assert np.array_equal(new_d.cpu().numpy().reshape(E, fb), newest) and np.array_equal(scal_d.cpu().numpy(), scal)
    got = out.cpu().numpy()
    assert np.array_equal(got[~adv], host_obs[~adv]) and (got[adv] == 5).all()
    with pytest.raises(A0Error):       # out stays required
        check(hip.lib.a0_env_pool_upload(new_h.data_ptr(), new_d.data_ptr(), scal_h.data_ptr(), scal_d.data_ptr(), N_SCAL, ADV, obs_h.data_ptr(), None, None,
                                         E, nstack, fb, None, _stream()), "a0_env_pool_upload")


def test_ingest_rejects_bad_arguments(hip):
    from agent0_amd._abi import A0Error
    E, fb = 8, 64
    ob = 4 * fb
    st = _state(hip, E, 3, 4, ob, E)
    u8 = lambda k: torch.zeros(k, dtype=torch.uint8, device=hip.device)
    prev, out, newest = u8(E * ob), u8(E * ob), u8(E * fb)
    scal, action = torch.zeros(N_SCAL * E, device=hip.device), torch.zeros(E, dtype=torch.int32, device=hip.device)
    args = lambda **kw: dict(dict(prev=prev, newest=newest, scal=scal, out=out, E=E, nstack=4, frame_bytes=fb, use_life_loss=True, action=action, n=3, ring_len=4,
                                  steps=0, gamma=0.99, ring_act=st["ring_act"], ring_rew=st["ring_rew"], ring_done=st["ring_done"], ring_obs=st["ring_obs"],
                                  frames=st["frames"], cap=E, start_slot=0, r_act=st["r_act"], r_rew=st["r_rew"], r_done=st["r_done"], stat_mask=st["stat_mask"],
                                  stat_ret=st["stat_ret"]), **kw)
    hip.host_step_ingest(**args())
    torch.cuda.synchronize()
    for bad in (dict(out=prev), dict(ring_len=2), dict(ring_obs=None), dict(frame_bytes=24), dict(cap=E - 1)):
        with pytest.raises(A0Error):
            hip.host_step_ingest(**args(**bad))
