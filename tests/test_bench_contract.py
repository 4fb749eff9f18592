"""bench.py's driver contract around the N > 1 path.

CPU: `python bench.py --gpus 2` without a launcher starts two ranks itself; with no GPU both ranks refuse to run (the hot path has
no CPU fallback) and the parent must relay the failure instead of hanging or printing a line.
GPU (-m gpu): BASELINE configs[3]'s frames (4928x3264, K = 32, quality 3.5, seeds 12345 + f) through the striped path at full size:
two ranks (gloo, both on device 0: a one-GPU box cannot run two RCCL ranks) stripe both frames, exchange the stripes, and each
produces its frame's container -- whose sha256 must equal the oracle's whole-frame golden (tests/golden/frames.json:
raise_k32_q3.5 and batch_frame1_k32_q3.5; the golden check is part of --full).  A plain one-GPU run prints the headline fields
only, and --dump-outputs writes the last timed step's container as float32 byte values."""
import hashlib
import json
import os
import subprocess
import sys

import pytest

from conftest import ROOT


def test_self_launch_relays_a_failing_rank():
    env = dict(os.environ)
    env.pop("RANK", None)
    env["HIP_VISIBLE_DEVICES"] = ""                           # no GPU for the children wherever this runs
    env["CUDA_VISIBLE_DEVICES"] = ""
    p = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "2", "--steps", "1", "--warmup", "0", "--no-cpu",
                        "--backend", "gloo", "--share-device"], env=env, capture_output=True, text=True, timeout=600)
    assert p.returncode != 0
    assert "needs a GPU" in p.stderr
    assert not p.stdout.strip().startswith("{")



def test_dump_outputs_samples_a_large_container_within_64_mb(tmp_path):
    """a container whose float32 copy would pass the budget is written as a fixed seeded sample with its positions"""
    import numpy as np
    from bench import dump_outputs
    blob = (np.arange(20_000_000, dtype=np.int64) * 7919 % 251).astype(np.uint8)      # 80 MB as float32
    for d in ("a", "b"):
        dump_outputs(str(tmp_path / d), blob, 1, 0)
    files = sorted(os.listdir(tmp_path / "a"))
    assert files == ["container.npy", "container_index.npy"]
    assert sum(os.path.getsize(tmp_path / "a" / f) for f in files) <= 64_000_000
    vals, idx = np.load(tmp_path / "a" / "container.npy"), np.load(tmp_path / "a" / "container_index.npy")
    assert vals.dtype == np.float32 and idx.dtype == np.float64 and vals.size == idx.size > 1_000_000
    assert (np.diff(idx) > 0).all() and idx[-1] < blob.size
    assert (vals == blob[idx.astype(np.int64)]).all()
    assert (np.load(tmp_path / "b" / "container_index.npy") == idx).all()                # the same positions every run
    small = blob[:1000]
    dump_outputs(str(tmp_path / "c"), small, 1, 0)
    assert sorted(os.listdir(tmp_path / "c")) == ["container.npy"]
    assert (np.load(tmp_path / "c" / "container.npy") == small).all()

@pytest.mark.gpu
def test_striped_path_at_full_size_reproduces_the_golden_containers():
    import torch
    if not torch.cuda.is_available():
        pytest.fail("no GPU visible: the gpu-marked tests need a real MI355X")
    env = dict(os.environ)
    for k in ("RANK", "LOCAL_RANK", "WORLD_SIZE", "MASTER_PORT"):
        env.pop(k, None)
    p = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "2", "--backend", "gloo", "--share-device", "--steps", "3",
                        "--warmup", "1", "--full", "--no-cpu"], env=env, capture_output=True, text=True, timeout=900)
    assert p.returncode == 0, p.stderr[-2000:]
    line = json.loads([ln for ln in p.stdout.splitlines() if ln.startswith("{")][-1])
    assert line["n_gpus"] == 2 and line["steps"] == 3
    assert line["golden_containers_checked"] == 2             # rank 0: seed 12345, rank 1: seed 12346
    assert line["bytes_match_golden"] is True
    assert line["config"]["container_bytes"] == 6631961       # rank 0's frame


@pytest.mark.gpu
def test_plain_run_dumps_the_last_steps_container(tmp_path):
    import numpy as np
    import torch
    if not torch.cuda.is_available():
        pytest.fail("no GPU visible: the gpu-marked tests need a real MI355X")
    with open(os.path.join(ROOT, "tests", "golden", "frames.json")) as f:
        gold = json.load(f)["1080p_k8_q3.5"]                   # seed 12345: the one frame of a one-step run
    env = dict(os.environ)
    for k in ("RANK", "LOCAL_RANK", "WORLD_SIZE", "MASTER_PORT"):
        env.pop(k, None)
    p = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--workload", "1080p", "--steps", "1", "--warmup", "1",
                        "--dump-outputs", str(tmp_path)], env=env, capture_output=True, text=True, timeout=600)
    assert p.returncode == 0, p.stderr[-2000:]
    line = json.loads([ln for ln in p.stdout.splitlines() if ln.startswith("{")][-1])
    assert line["steps"] == 1 and line["ms_per_step"] > 0 and line["value"] > 0
    assert line["dtype"] == "f64" and line["unit"] == "Mpixels/s" and line["higher_is_better"] is True
    assert "roofline" not in line and "cpu_baseline" not in line and "bytes_match_golden" not in line
    assert sorted(os.listdir(tmp_path)) == ["container.npy"]
    dumped = np.load(tmp_path / "container.npy")
    assert dumped.dtype == np.float32 and dumped.size == gold["container_bytes"] == line["config"]["container_bytes"]
    assert hashlib.sha256(dumped.astype(np.uint8).tobytes()).hexdigest() == gold["container_sha256"]
