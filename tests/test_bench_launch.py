"""bench.py --gpus N as the driver may invoke it: plain `python bench.py --gpus N ...` with no launcher and no WORLD_SIZE.  It must be its
own launcher -- N ranks, one per GPU, RANK / LOCAL_RANK / WORLD_SIZE / MASTER_* as torch.distributed.run sets them, rank 0's JSON line
relayed -- and keep working under torch.distributed.run (WORLD_SIZE set: no second spawn).  CPU tests: the spawn itself (process
creation mocked), and the real thing down to the first GPU call, which must fail loudly here and stop the other rank."""
import importlib
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _bench():
    if ROOT not in sys.path:
        sys.path.insert(0, ROOT)
    return importlib.import_module("bench")


class _FakeProc:
    def __init__(self, line):
        self._line, self.returncode = line, None

    def communicate(self, timeout=None):
        self.returncode = 0
        return self._line, None

    def wait(self, timeout=None):
        self.returncode = 0
        return 0

    def terminate(self):
        self.returncode = -15


def test_gpus_n_without_world_size_spawns_n_ranks(monkeypatch, capsys):
    bench = _bench()
    spawned = []

    def fake_popen(cmd, env=None, stdout=None, **kw):
        spawned.append((cmd, env, stdout))
        return _FakeProc(b'{"n_gpus": 2, "value": 1.0}\n' if env["RANK"] == "0" else b"")

    monkeypatch.setattr(subprocess, "Popen", fake_popen)
    monkeypatch.setattr(sys, "argv", ["bench.py", "--gpus", "2", "--steps", "3", "--warmup", "1"])
    for v in ("WORLD_SIZE", "RANK", "LOCAL_RANK"):
        monkeypatch.delenv(v, raising=False)
    try:
        bench.main()
        rc = 0
    except SystemExit as e:
        rc = e.code
    assert rc == 0
    assert len(spawned) == 2
    ports = set()
    for r, (cmd, env, stdout) in enumerate(spawned):
        assert cmd[0] == sys.executable and os.path.basename(cmd[1]) == "bench.py" and cmd[2:] == ["--gpus", "2", "--steps", "3", "--warmup", "1"]
        assert (env["RANK"], env["LOCAL_RANK"], env["WORLD_SIZE"], env["MASTER_ADDR"]) == (str(r), str(r), "2", "127.0.0.1")
        assert env["HSA_ENABLE_IPC_MODE_LEGACY"] == "0"
        ports.add(env["MASTER_PORT"])
        assert (stdout == subprocess.PIPE) == (r == 0)  # only rank 0's stdout carries the line
    assert len(ports) == 1 and 1024 < int(ports.pop()) < 65536
    line = capsys.readouterr().out.strip().splitlines()
    assert len(line) == 1 and json.loads(line[0])["n_gpus"] == 2


def test_a_launcher_s_world_size_is_respected(monkeypatch):
    """Under torch.distributed.run (WORLD_SIZE in the environment) bench.py is a rank, never a launcher."""
    bench = _bench()
    called = []
    monkeypatch.setattr(bench, "self_launch", lambda n: called.append(n) or 0)
    monkeypatch.setattr(sys, "argv", ["bench.py", "--gpus", "2", "--call-probe", "f32", "--size", "8,6,2"])
    monkeypatch.setenv("WORLD_SIZE", "2")
    try:
        bench.main()  # (--call-probe returns before anything else; here it fails at the first GPU call -- after the launch decision)
    except BaseException:
        pass
    assert called == []


def test_plain_invocation_reaches_the_gpu_call_and_fails_loudly_without_one(gpu_available):
    """The real spawn on this CPU box: both ranks start, rendezvous over gloo, and die at nnlm_create (no HIP device); the parent reports
    the failing rank, stops the other one and returns ITS exit code -- not the `launch with torch.distributed.run` exit 2 of round 4."""
    if gpu_available:
        import pytest
        pytest.skip("GPU present: covered by the -m gpu suite")
    env = {k: v for k, v in os.environ.items() if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK")}
    p = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "2", "--steps", "2", "--warmup", "1", "--size", "64,48,4",
                        "--cpu-iters", "0", "--others", "0"], env=env, capture_output=True, text=True, timeout=300)
    assert p.returncode not in (0, 2), (p.returncode, p.stderr[-400:])
    assert "no HIP device" in p.stderr and "exited with" in p.stderr, p.stderr[-600:]
    assert p.stdout.strip() == ""


def test_roofline_block_is_the_dominant_kernel_with_a_real_bound():
    """The contract reserves `roofline` for the dominant kernel and its HBM / MFMA bound.  The two half-steps' plain cross products are
    launches of one kernel (the first row of rocprofv3's summary), so they rank as one class: with the per-kernel times of a committed
    bench line (profiles/r05_cfg2_bench_steps20.json) the block must be the A-streaming cross product, HBM bound, at achieved =
    algorithmic bytes / average launch time, and the persistent sweep (no roofline: a loop-carried recurrence) must be the secondary."""
    bench = _bench()
    d = json.load(open(os.path.join(ROOT, "profiles", "r05_cfg2_bench_steps20.json")))
    kern = d["kernels"]
    roof, sec, blocks, shares = bench.analyse(bench.CONFIGS[2], 2, kern, 20000, 10000, 50, 4, 1, {"sweep_w": 1, "sweep_h": 0})
    assert roof["bound"] == "hbm" and "xprod16_tn_kernel" in roof["kernel"] and roof["unit"] == "GB/s" and roof["peak"] == 8000.0
    n_l = kern["xprod_h"]["launches"] + kern["xprod_w"]["launches"]
    ms = (kern["xprod_h"]["total_ms"] + kern["xprod_w"]["total_ms"]) / n_l
    by = ((20000 * 10000 * 4 + 50 * 20000 * 4 + 50 * 10000 * 8) * kern["xprod_h"]["launches"] +
          (20000 * 10000 * 4 + 50 * 10000 * 4 + 50 * 20000 * 8) * kern["xprod_w"]["launches"]) / n_l
    assert abs(roof["achieved"] - by / (ms * 1e-3) / 1e9) < 1e-6 * roof["achieved"]
    assert 0.5 < roof["frac"] < 0.8 and abs(roof["frac"] - roof["achieved"] / roof["peak"]) < 1e-12
    assert roof["traffic"] is not None and 0.9 < roof["traffic"] / by < 1.3  # (PMC bytes per launch from the committed summaries)
    assert sec["bound"] == "latency" and "sweep_scd_qw_kernel" in sec["kernel"]
    assert {"xprod_h", "xprod_w", "xprod_w_err", "sweep_h", "sweep_w"} <= set(blocks)


def test_dump_outputs_writes_fp64_within_the_limit_and_samples_the_same_entries_every_time(tmp_path, monkeypatch):
    """--dump-outputs: every array as fp64 <name>.npy; under the limit whole, beyond it each array over 1 MB as the same fixed seeded
    sample of its entries in every run (so two builds' dumps compare entry for entry), small arrays (the traces) still whole."""
    import numpy as np
    bench = _bench()
    rng = np.random.default_rng(3)
    arrays = dict(W=rng.random((500, 300)).astype(np.float32), H=rng.random((300, 600)), mse_error=np.arange(5.0))
    bench.dump_outputs(str(tmp_path / "whole"), arrays)
    for nm, a in arrays.items():
        got = np.load(tmp_path / "whole" / f"{nm}.npy")
        assert got.dtype == np.float64 and np.array_equal(got, a)
    limit = 1_500_000
    monkeypatch.setattr(bench, "DUMP_LIMIT", limit)
    bench.dump_outputs(str(tmp_path / "a"), arrays)
    bench.dump_outputs(str(tmp_path / "b"), arrays)
    data = 0
    for nm, a in arrays.items():
        got, again = np.load(tmp_path / "a" / f"{nm}.npy"), np.load(tmp_path / "b" / f"{nm}.npy")
        assert got.dtype == np.float64 and np.array_equal(got, again)
        if nm == "mse_error":
            assert np.array_equal(got, a)
        else:
            idx = np.sort(np.random.default_rng(0).choice(a.size, got.size, replace=False))
            assert 0 < got.size < a.size and np.array_equal(got, a.ravel()[idx].astype(np.float64))
        data += got.nbytes
    assert data <= limit
