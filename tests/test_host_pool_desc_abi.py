"""CPU: the ctypes mirror of a0_env_pool_desc (agent0_amd/deepq/native_loop.py) has the header's layout — sizeof and every offsetof, from the header compiled the way a
plain C host compiles it — and the pool calls and a0_host_step_ingest refuse bad arguments before any HIP call."""
import ctypes as C
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_pool_descriptor_mirror_matches_the_header(tmp_path):
    from agent0_amd.deepq.native_loop import _PoolDesc
    gcc = shutil.which("gcc")
    if gcc is None or not os.path.exists("/opt/rocm/include/hip/hip_runtime_api.h"):
        pytest.fail("gcc and the ROCm headers are part of the build image")
    names = [f[0] for f in _PoolDesc._fields_]
    src = tmp_path / "pool_desc.c"
    src.write_text("#include <stdio.h>\n#include <stddef.h>\n#include \"agent0_hip.h\"\nint main(void) {\n  printf(\"%zu\\n\", sizeof(a0_env_pool_desc));\n"
                   + "".join(f"  printf(\"%zu\\n\", offsetof(a0_env_pool_desc, {n}));\n" for n in names) + "  return 0;\n}\n")
    exe = tmp_path / "pool_desc"
    subprocess.run([gcc, "-std=gnu99", "-Wall", "-D__HIP_PLATFORM_AMD__", "-I/opt/rocm/include", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)],
                   check=True, capture_output=True, text=True)
    got = [int(x) for x in subprocess.check_output([str(exe)]).split()]
    assert got[0] == C.sizeof(_PoolDesc)
    assert got[1:] == [getattr(_PoolDesc, n).offset for n in names]


@pytest.fixture(scope="module")
def lib():
    from agent0_amd import _abi
    return _abi.load()


def test_pool_calls_refuse_a_missing_handle(lib):
    from agent0_amd import _abi
    from agent0_amd.deepq.native_loop import _PoolDesc
    d = _PoolDesc()
    assert lib.a0_actor_attach_pool(None, C.addressof(d)) == -1 and "a0_actor_attach_pool" in _abi.last_error()
    assert lib.a0_actor_detach_pool(None) == -1
    assert lib.a0_actor_pool_seq(None, None, None, -1) != 0 and "a0_actor_pool_seq" in _abi.last_error()


def _ingest_args(**kw):
    P = 0x10000                                       # 16-byte aligned stand-ins; validation must refuse the call before anything reads them
    a = dict(prev=P, newest=2 * P, scal=3 * P, out=4 * P, E=8, nstack=4, frame_bytes=64, use_life_loss=1, action=5 * P, n=3, ring_len=4, steps=0, gamma=0.99,
             ring_act=6 * P, ring_rew=7 * P, ring_done=8 * P, ring_obs=9 * P, frames=10 * P, cap=8, start_slot=0, r_act=11 * P, r_rew=12 * P, r_done=13 * P,
             stat_mask=14 * P, stat_ret=15 * P, ctrl=None, stream=None)
    a.update(kw)
    return list(a.values())


@pytest.mark.parametrize("bad", [dict(out=0x10000), dict(prev=None), dict(cap=7), dict(ring_len=2), dict(ring_obs=None), dict(frame_bytes=24), dict(frames=0x10008),
                                 dict(nstack=1), dict(n=0), dict(steps=-1), dict(start_slot=-1), dict(stat_ret=None)])
def test_ingest_validates_its_arguments(lib, bad):
    from agent0_amd import _abi
    assert lib.a0_host_step_ingest(*_ingest_args(**bad)) == -1
    assert "a0_host_step_ingest" in _abi.last_error()
