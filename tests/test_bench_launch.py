"""CPU tests of bench.py's launch decision for `--gpus N` (made before anything touches the GPU): N > 1
without a launcher spawns N ranks (torch.distributed.run) or fails when fewer GPUs are visible -- it
never measures one GPU and reports it as N; under a launcher N must equal WORLD_SIZE and the RCCL path
needs one GPU per rank.  Reference: the multi-worker run, src/bin/mrworker.rs:43-149."""
import os
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def plan(gpus, env, n_dev, backend="nccl"):
    import bench
    return bench.launch_plan(gpus, backend, env, n_dev)


def test_single_gpu_default():
    assert plan(1, {}, 1) == "single"
    assert plan(1, {}, 0) == "single"           # no device: the library's own error says so later
    assert plan(1, {"WORLD_SIZE": "1"}, 8) == "single"


def test_spawn_when_no_launcher():
    assert plan(8, {}, 8) == "spawn"
    assert plan(2, {}, 8) == "spawn"
    assert plan(2, {}, 1, backend="gloo") == "spawn"   # the gloo rehearsal may share one GPU


@pytest.mark.parametrize("gpus,n_dev", [(2, 1), (8, 4), (4, 0)])
def test_more_gpus_than_visible_is_an_error(gpus, n_dev):
    with pytest.raises(SystemExit, match="visible"):
        plan(gpus, {}, n_dev)


def test_under_a_launcher():
    env = {"WORLD_SIZE": "4", "LOCAL_WORLD_SIZE": "4", "RANK": "1", "LOCAL_RANK": "1"}
    assert plan(4, env, 8) == "rank"
    with pytest.raises(SystemExit, match="WORLD_SIZE"):
        plan(2, env, 8)
    with pytest.raises(SystemExit, match="WORLD_SIZE"):
        plan(2, {"WORLD_SIZE": "1"}, 8)
    with pytest.raises(SystemExit, match="one GPU per rank"):
        plan(4, env, 2)
    assert plan(4, env, 1, backend="gloo") == "rank"
    with pytest.raises(SystemExit):
        plan(0, {}, 1)


def test_cli_exits_nonzero_without_enough_gpus():
    """`python bench.py --gpus 2` on a host with no GPU (this container): exits non-zero at once with the
    reason, instead of running and reporting one device."""
    env = dict(os.environ)
    for k in ("WORLD_SIZE", "RANK", "LOCAL_RANK", "LOCAL_WORLD_SIZE"):
        env.pop(k, None)
    import torch
    if torch.cuda.device_count() >= 2:
        pytest.skip("two GPUs are visible")
    p = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "2", "--quick"], env=env,
                       capture_output=True, text=True, timeout=300)
    assert p.returncode != 0 and "visible" in p.stderr, p.stderr[-2000:]


# ---- the plain run, --full and --dump-outputs

def _parse(argv, monkeypatch):
    import bench
    monkeypatch.setattr(sys, "argv", ["bench.py"] + argv)
    return bench.parse()


def test_full_is_off_by_default(monkeypatch):
    a = _parse(["--gpus", "1", "--steps", "4", "--warmup", "2"], monkeypatch)
    assert a.full is False and a.dump_outputs is None and (a.steps, a.warmup) == (4, 2)
    a = _parse(["--full", "--dump-outputs", "d"], monkeypatch)
    assert a.full is True and a.dump_outputs == "d"


class _FakeCtx:
    """A context whose job output is `data` cut at `off` (the two calls dump_outputs makes)."""

    def __init__(self, data, off):
        self.data, self.off = data, off

    def output(self):
        return 0, list(self.off)

    def copy_output_to(self, host_ptr, n):
        import ctypes
        ctypes.memmove(host_ptr, self.data, n)


@pytest.mark.parametrize("cap", [1 << 20, 1000])  # the whole output / the seeded sample of a larger one
def test_dump_outputs_arrays(tmp_path, monkeypatch, cap):
    import numpy as np

    import bench
    monkeypatch.setattr(bench, "DUMP_MAX_BYTES", cap)
    rng = np.random.default_rng(7)
    data = rng.integers(0, 256, 5003, dtype=np.uint8).tobytes()
    off = [0, 17, 17, 2900, 5003]
    st = {"tokens": 11, "map_records": 7, "distinct_keys": 5, "output_bytes": 5003}
    for d in ("a", "b"):
        bench.dump_outputs(_FakeCtx(data, off), st, str(tmp_path / d), 0, 1)
    got = {n: np.load(tmp_path / "a" / f"{n}.npy") for n in
           ("output_bytes", "partition_offsets", "partition_byte_sums", "counters")}
    assert sorted(p.name for p in (tmp_path / "a").iterdir()) == sorted(f"{n}.npy" for n in got)
    assert got["output_bytes"].dtype == np.float32
    assert all(got[n].dtype == np.float64 for n in got if n != "output_bytes")
    raw = np.frombuffer(data, dtype=np.uint8)
    assert got["output_bytes"].size == min(cap, len(data))
    if cap >= len(data):
        assert np.array_equal(got["output_bytes"], raw.astype(np.float32))
    else:
        assert set(got["output_bytes"].tolist()) <= set(raw.astype(np.float32).tolist())
    assert got["partition_offsets"].tolist() == off
    assert got["partition_byte_sums"].tolist() == [float(raw[off[r]:off[r + 1]].sum(dtype=np.uint64)) for r in range(4)]
    assert got["counters"].tolist() == [11, 5, 5003]
    assert sum(v.nbytes for v in got.values()) <= 64e6
    for n in got:  # the same arguments give the same arrays
        assert np.array_equal(got[n], np.load(tmp_path / "b" / f"{n}.npy"))
    # a rank of a multi-GPU run writes its own files
    bench.dump_outputs(_FakeCtx(data, off), st, str(tmp_path / "c"), 1, 2)
    assert sorted(p.name for p in (tmp_path / "c").iterdir()) == sorted(f"{n}_rank1.npy" for n in got)


@pytest.mark.gpu
def test_plain_run_times_the_steps_and_dumps_the_output(tmp_path):
    """A plain `bench.py --gpus 1 --steps K --warmup W` on a small input: K timed steps, the headline
    fields, none of the --full legs, and --dump-outputs arrays that equal the oracle's mr-{r}.txt bytes
    of the same input (the generator is a function of the arguments)."""
    import json

    import numpy as np
    import torch

    import mapreduce_rust_amd as M
    import oracle_lib as O
    env = dict(os.environ)
    for k in ("WORLD_SIZE", "RANK", "LOCAL_RANK", "LOCAL_WORLD_SIZE"):
        env.pop(k, None)
    args = ["--gpus", "1", "--steps", "3", "--warmup", "1", "--files-per-gpu", "3", "--file-mib", "1",
            "--reduce", "5", "--vocab", "4096"]
    p = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py")] + args + ["--dump-outputs", str(tmp_path)],
                       env=env, capture_output=True, text=True, timeout=120)
    assert p.returncode == 0, p.stderr[-2000:]
    lines = p.stdout.strip().splitlines()
    assert len(lines) == 1
    j = json.loads(lines[0])
    assert j["steps"] == 3 and j["warmup"] == 1 and len(j["job"]["map_launches"]) == 3
    assert j["unit"] == "GB/s" and j["higher_is_better"] is True and j["dtype"] == "u8" and j["ms_per_step"] > 0
    assert j["value"] == pytest.approx(3 * (1 << 20) / (j["ms_per_step"] / 1e3) / 1e9, rel=1e-2)
    assert not {"cold", "end_to_end", "zipf_u", "c5", "c2", "cpu_baseline"} & set(j)

    # the same input, generated again, through the oracle
    fb = 1 << 20
    buf = torch.empty(3 * fb + 64, dtype=torch.uint8, device="cuda:0")
    with M.Context(0) as ctx:
        for i in range(3):
            ctx.gen_zipf(buf.data_ptr() + i * fb, fb, 0x5EED2026, i, 4096, 1.1)
        torch.cuda.synchronize()
    host = buf[:3 * fb].cpu().numpy().tobytes()
    exp = O.wc([host[i * fb:(i + 1) * fb] for i in range(3)], 5, O.FAST)
    off = np.load(tmp_path / "partition_offsets.npy")
    assert off.tolist() == np.cumsum([0] + [len(e) for e in exp]).tolist()
    got = np.load(tmp_path / "output_bytes.npy")
    assert got.dtype == np.float32
    assert got.astype(np.uint8).tobytes() == b"".join(exp)
    assert np.load(tmp_path / "partition_byte_sums.npy").tolist() == [float(sum(e)) for e in exp]
    assert np.load(tmp_path / "counters.npy")[2] == len(b"".join(exp))
