"""CPU: the C-ABI library loads and exports every symbol include/agent0_hip.h declares (no compute without a GPU); host-side
logic of the product (config overrides, schedules, layout maths); isolation of the oracle from the product path."""
import ast
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_library_exports_every_declared_symbol():
    from agent0_amd import _abi
    protos = _abi.parse_header()
    names = [n for _, n, _ in protos]
    assert len(names) == len(set(names)) and len(names) >= 55
    assert os.path.exists(_abi.LIB_PATH), "build the library first: python -c 'import __graft_entry__ as g; g.build()'"
    out = subprocess.check_output(["nm", "-D", "--defined-only", _abi.LIB_PATH]).decode()
    exported = {line.split()[-1] for line in out.splitlines() if line.strip()}
    missing = [n for n in names if n not in exported]
    assert not missing, f"declared in the header but not exported: {missing}"
    lib = _abi.load()                       # dlopen + argtypes for every prototype; works without a GPU
    assert lib.a0_abi_version() == 1
    # argument validation happens before any HIP call, so it is testable here
    assert lib.a0_dense_fwd(None, 4, None, None, None, 1, 4, 4, 0, None, None) == -1
    assert "a0_dense_fwd" in _abi.last_error()
    assert lib.a0_sumtree_set(None, 3, None, None, 1, None, None) == -1 and "power of two" in _abi.last_error()


def test_product_loader_refuses_a_tuning_build(tmp_path):
    """A library stamped by tools/build_variant.sh (extra -D flags, possibly timing-only code) must never be loaded by the product:
    the loader takes one fixed path (no environment override) and only a build that reports "default"."""
    from agent0_amd import _abi
    assert "A0_LIB" not in open(os.path.join(ROOT, "agent0_amd", "_abi.py")).read()
    assert _abi.load().a0_build_info() == b"default"
    assert not os.path.exists(os.path.join(ROOT, "agent0_amd", "lib", "variants"))
    assert "A0_EXP" not in open(os.path.join(ROOT, "agent0_amd", "csrc", "encoder_fused.hip")).read()
    # the same library with core.hip re-stamped, in a fresh interpreter (the loader caches its handle)
    csrc = os.path.join(ROOT, "agent0_amd", "csrc")
    objs = [os.path.join(csrc, "_obj", f) for f in sorted(os.listdir(os.path.join(csrc, "_obj"))) if f.endswith(".o") and f != "core.o"]
    core = str(tmp_path / "core.o")
    subprocess.check_call(["/opt/rocm/bin/hipcc", "-O1", "--offload-arch=gfx950", "-fPIC", "-std=c++17", "-I" + os.path.join(ROOT, "include"),
                           '-DA0_BUILD_VARIANT="x6: -DA0_X9_MAXORD=2"', "-c", os.path.join(csrc, "core.hip"), "-o", core])
    lib = str(tmp_path / "libagent0_hip_x6.so")
    subprocess.check_call(["/opt/rocm/bin/hipcc", "--offload-arch=gfx950", "-shared", "-fPIC", "-o", lib, core] + objs + ["-ldl"])
    code = ("import sys; sys.path.insert(0, %r)\nfrom agent0_amd import _abi\n"
            "try:\n    _abi.load(%r)\n    print('LOADED')\nexcept _abi.A0Error as e:\n    print('REFUSED', e)\n"
            "print(_abi.load(%r, allow_variant=True).a0_build_info().decode())\n" % (ROOT, lib, lib))
    out = subprocess.check_output([sys.executable, "-c", code]).decode()
    assert "REFUSED" in out and "tuning build (x6: -DA0_X9_MAXORD=2)" in out and "LOADED" not in out
    assert out.strip().splitlines()[-1] == "x6: -DA0_X9_MAXORD=2"


def test_gfx950_code_object_only():
    from agent0_amd import _abi
    blob = open(_abi.LIB_PATH, "rb").read()
    assert b"gfx950" in blob and b"gfx942" not in blob and b"gfx90a" not in blob and b"sm_" not in blob


def test_product_fails_loudly_without_gpu():
    import torch
    if torch.cuda.is_available():
        pytest.skip("GPU present")
    from agent0_amd._abi import A0Error
    from agent0_amd.ops import HipOps
    with pytest.raises(A0Error, match="needs an AMD GPU"):
        HipOps()
    from agent0_amd.deepq.config import parse_overrides
    from agent0_amd.deepq.trainer import Trainer
    cfg = parse_overrides(["device=cpu", "wandb=false", "tb=false"])
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        Trainer(cfg)


def test_config_overrides_and_aliases():
    from agent0_amd.deepq import config as C
    cfg = C.parse_overrides(["env_id=Enduro", "learner.algo=iqr", "learner.double_q=true", "learner.dueling_head=True", "learner.noisy_net=1",
                             "learner.n_step_q=3", "replay.policy=prioritize", "actor.num_envs=256", "replay.size=1000000", "device=cuda",
                             "wandb=false", "tb=false", "trainer.total_steps=1e6", "learner.c51.vmax=20", "learner.iqn.N=32", "seed=7"])
    assert cfg.env_id == "Enduro" and cfg.learner.algo is C.AlgoEnum.iqn and cfg.learner.double_q and cfg.learner.dueling_head and cfg.learner.noisy_net
    assert cfg.learner.n_step_q == 3 and cfg.replay.policy is C.ReplayEnum.prioritize and cfg.actor.num_envs == 256 and cfg.replay.size == 10**6
    assert cfg.trainer.total_steps == 10**6 and cfg.learner.c51.vmax == 20.0 and cfg.learner.iqn.N == 32 and cfg.seed == 7 and not cfg.wandb
    with pytest.raises(KeyError):
        C.parse_overrides(["learner.nope=1"])
    with pytest.raises(ValueError):
        C.parse_overrides(["learner.algo=sarsa"])
    # reference defaults, field for field (agent0/deepq/config.py:72-145)
    d = C.ExpConfig()
    assert (d.learner.discount, d.learner.batch_size, d.learner.learning_rate, d.learner.target_update_freq, d.learner.learner_steps) == (0.99, 512, 5e-4, 500, 20)
    assert (d.trainer.total_steps, d.trainer.training_start_steps, d.trainer.exploration_steps) == (10**7, 10**5, 10**6)
    assert (d.actor.num_envs, d.actor.sample_steps, d.actor.min_eps, d.actor.test_eps) == (16, 80, 0.01, 0.001)
    assert (d.replay.size, d.replay.beta0, d.replay.alpha, d.replay.eps) == (10**6, 0.4, 0.5, 0.01)
    assert (d.learner.iqn.K, d.learner.iqn.N, d.learner.iqn.N_dash, d.learner.iqn.num_cosines, d.learner.iqn.F) == (32, 64, 64, 64, 32)
    assert d.num_actors == 3 and d.seed == 42 and d.env_id == "Breakout"
    rt = C.from_dict(C.to_dict(cfg))
    assert C.to_dict(rt) == C.to_dict(cfg)


def test_schedules_match_golden():
    from agent0_amd.common.utils import LinearSchedule
    from agent0_amd.deepq.config import ExpConfig
    from agent0_amd.deepq.trainer import epsilon_schedule
    from util import golden
    g = golden("g9_schedules")
    s = LinearSchedule(0.4, 1.0, 1e7)
    assert np.array_equal(np.array([s(1280) for _ in range(6)]), g["lin_a"])
    s = LinearSchedule(1.0, 0.1, 10)
    assert np.array_equal(np.array([s() for _ in range(14)]), g["lin_c"])
    eps = epsilon_schedule(ExpConfig())
    assert np.array_equal(np.array([eps(int(t)) for t in g["eps_steps"]]), g["eps"])


def _imports(path):
    tree = ast.parse(open(path).read(), path)
    for node in ast.walk(tree):
        if isinstance(node, ast.Import):
            for a in node.names:
                yield a.name
        elif isinstance(node, ast.ImportFrom) and node.module:
            yield ("." * node.level) + node.module


def test_product_never_imports_the_oracle_or_the_emulation():
    bad = []
    for pkg in ("agent0_amd", "agent0"):
        for dirpath, _, files in os.walk(os.path.join(ROOT, pkg)):
            for f in files:
                if f.endswith(".py"):
                    p = os.path.join(dirpath, f)
                    src = open(p).read()
                    for mod in _imports(p):
                        if mod.split(".")[0] in ("oracle", "cpu_ops", "tests", "recipe"):
                            bad.append((p, mod))
                    assert "liba0oracle" not in src and "host_emul" not in src, p
    assert not bad, f"product code must not import test infrastructure: {bad}"
    # nothing at run time reads the reference tree
    for rel in ("bench.py", "__graft_entry__.py"):
        assert "/root/reference" not in open(os.path.join(ROOT, rel)).read()
    for dirpath, _, files in os.walk(os.path.join(ROOT, "agent0_amd")):
        for f in files:
            if f.endswith((".py", ".hip", ".h", ".sh")):
                src = open(os.path.join(dirpath, f)).read()
                assert "sys.path.insert(0, \"/root/reference\")" not in src and "import_reference" not in src


def test_u8_division_shortcut_is_exact():
    """x/255 via one Newton correction (operands.h a0_div255) equals the fp32 division for every byte value."""
    x = np.arange(256, dtype=np.float32)
    r = np.float32(1.0) / np.float32(255.0)
    q0 = x * r
    e = np.float32(x.astype(np.float64) - q0.astype(np.float64) * 255.0)          # fma(-q0, 255, x): exact in fp64, then one rounding
    q = (q0.astype(np.float64) + e.astype(np.float64) * np.float64(r)).astype(np.float32)
    assert np.array_equal(q, x / np.float32(255.0))


def test_bench_starts_its_own_launcher_as_a_child(monkeypatch, capsys):
    """``python bench.py --gpus N`` with no launcher environment (the way the driver may call it): bench.py must start
    ``python -m torch.distributed.run --nnodes=1 --nproc-per-node N --master-addr 127.0.0.1 --master-port <free> bench.py <same flags>`` as a CHILD
    process — never an exec, and before anything in this process imports the GPU stack — relay rank 0's JSON line on stdout and return the
    child's exit code."""
    import io
    import json
    import subprocess
    import sys

    ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    sys.path.insert(0, ROOT)
    import bench

    seen = {}

    class FakeProc:
        def __init__(self, cmd, stdout=None, text=None, env=None):
            seen["cmd"], seen["env"] = cmd, env
            self.stdout = io.StringIO('some library banner\n{"metric": "env-frames/sec", "value": 1.0, "n_gpus": 4}\n')

        def wait(self):
            return 0

    monkeypatch.setattr(subprocess, "Popen", FakeProc)
    monkeypatch.delenv("WORLD_SIZE", raising=False)
    monkeypatch.setattr(sys, "argv", ["bench.py", "--gpus", "4", "--steps", "3", "--warmup", "1", "--self-launch"])
    monkeypatch.setattr(os, "execv", lambda *a, **k: (_ for _ in ()).throw(AssertionError("bench.py must never exec")))
    gpu_stack = [m for m in ("agent0_amd.ops", "agent0_amd.deepq.trainer") if m in sys.modules]
    with pytest.raises(SystemExit) as e:
        bench.main()
    assert e.value.code == 0
    cmd = seen["cmd"]
    assert cmd[:3] == [sys.executable, "-m", "torch.distributed.run"] and "--nnodes=1" in cmd and "--nproc-per-node=4" in cmd
    assert cmd[cmd.index("--master-addr") + 1] == "127.0.0.1" and int(cmd[cmd.index("--master-port") + 1]) > 0
    i = cmd.index(os.path.join(ROOT, "bench.py"))
    assert cmd[i + 1:] == ["--gpus", "4", "--steps", "3", "--warmup", "1"], "the child gets the same flags, minus --self-launch"
    assert seen["env"]["HSA_ENABLE_IPC_MODE_LEGACY"] == "0"
    out = capsys.readouterr()
    assert json.loads(out.out.strip())["n_gpus"] == 4 and "banner" in out.err, "exactly the JSON line on stdout, everything else on stderr"
    assert [m for m in ("agent0_amd.ops", "agent0_amd.deepq.trainer") if m in sys.modules] == gpu_stack, "the parent did not load the GPU stack"


def test_bench_extra_measurements_need_full(monkeypatch):
    """A plain bench run measures the headline figure only; the probe, replay GB/s, learner_steps=320, other entry point and CPU baseline
    run behind ``--full``, and the ``--no-*`` switches still leave parts of a ``--full`` run out."""
    import sys

    ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    sys.path.insert(0, ROOT)
    import bench

    monkeypatch.setattr(sys, "argv", ["bench.py", "--gpus", "1", "--steps", "3", "--warmup", "1"])
    assert bench.parse().full is False
    monkeypatch.setattr(sys, "argv", ["bench.py", "--steps", "3", "--full", "--no-cpu-baseline"])
    a = bench.parse()
    assert a.full is True and a.no_cpu_baseline is True and a.no_ratio320 is False and a.no_other_entry is False


def test_no_kernel_of_the_library_uses_scratch_memory():
    """build.sh records the compiler's per-kernel resource remarks (agent0_amd/lib/kernel_resources.txt).  A kernel that spills registers
    to scratch still computes the right thing — only slower, with HBM traffic nobody asked for (round 2: ten spilled VGPRs of the fused
    encoder showed up as 8.45 MB written per launch instead of 3.21 MB) — so nothing else would notice."""
    import os
    from agent0_amd import _abi
    path = os.path.join(os.path.dirname(_abi.LIB_PATH), "kernel_resources.txt")
    assert os.path.exists(path), "agent0_amd/csrc/build.sh writes the report next to the library"
    rows = [dict(kv.split("=") for kv in line.split()[2:]) | {"name": line.split()[1]} for line in open(path) if line.strip()]
    assert len(rows) > 100 and any("a0_encoder_fused_kernel" in r["name"] for r in rows)
    bad = [r for r in rows if int(r["scratch"]) or int(r["vgpr_spill"]) or int(r["sgpr_spill"])]
    assert not bad, f"kernels with scratch / spills: {[(r['name'], r['scratch'], r['vgpr_spill'], r['sgpr_spill']) for r in bad]}"


def test_plain_c_hosts_compile_against_the_header():
    """include/agent0_hip.h is a C header: tests/c_host_demo.c and tests/c_host_loop.c (the non-Python hosts of the handle API; run on the GPU box by
    tests/test_gpu_engine.py / test_gpu_trainer.py) must compile as C — syntax and types only, no GPU needed."""
    import shutil
    import subprocess
    gcc = shutil.which("gcc")
    if gcc is None or not os.path.exists("/opt/rocm/include/hip/hip_runtime_api.h"):
        pytest.skip("no C compiler / ROCm headers here")
    for src in ("c_host_demo.c", "c_host_loop.c"):
        r = subprocess.run([gcc, "-std=gnu99", "-Wall", "-fsyntax-only", "-D__HIP_PLATFORM_AMD__", "-I/opt/rocm/include", "-I", os.path.join(ROOT, "include"),
                            os.path.join(ROOT, "tests", src)], capture_output=True, text=True, timeout=300)
        assert r.returncode == 0, src + ":\n" + r.stderr[-3000:]
