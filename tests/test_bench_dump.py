"""bench.py --dump-outputs: the sample it takes of a large output (CPU), and a plain run's dump
on the GPU against the oracle (a small frame size, so the whole output is written)."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_dump_outputs_sample_is_fixed(tmp_path):
    """More blocks than DUMP_MAX_BLOCKS: the same ascending sample of whole blocks every time."""
    import torch

    import bench
    n = bench.DUMP_MAX_BLOCKS + 1000
    assert bench.DUMP_MAX_BLOCKS * 64 * 4 <= 64 * 2 ** 20
    d_out = (torch.arange(n * 64, dtype=torch.int32) % 32003 - 16000).to(torch.int16).view(2, -1, 64)
    bench.dump_outputs(str(tmp_path / "a"), d_out, "coefficients")
    bench.dump_outputs(str(tmp_path / "b"), d_out.clone(), "coefficients")
    a = np.load(tmp_path / "a" / "coefficients.npy")
    b = np.load(tmp_path / "b" / "coefficients.npy")
    assert a.dtype == np.float32 and a.shape == (bench.DUMP_MAX_BLOCKS, 64)
    assert np.array_equal(a, b)
    # every row is one whole block of the source, rows in the source's order, none twice
    flat = d_out.view(-1, 64).numpy()
    idx = np.sort(np.random.default_rng(0).choice(n, bench.DUMP_MAX_BLOCKS, replace=False))
    assert len(np.unique(idx)) == len(idx)
    assert np.array_equal(a, flat[idx].astype(np.float32))
    # one of 8 ranks: an eighth of the blocks, so that all ranks' files stay within the limit
    bench.dump_outputs(str(tmp_path / "c"), d_out, "coefficients_rank3", bench.DUMP_MAX_BLOCKS // 8)
    c = np.load(tmp_path / "c" / "coefficients_rank3.npy")
    assert c.shape == (bench.DUMP_MAX_BLOCKS // 8, 64) and np.isin(c[:, 0], flat[:, 0]).all()


def test_dump_outputs_small_output_is_whole(tmp_path):
    import torch

    import bench
    d_out = torch.arange(3 * 5 * 64, dtype=torch.int16).view(3, 5, 64) - 400
    bench.dump_outputs(str(tmp_path), d_out, "coefficients")
    a = np.load(tmp_path / "coefficients.npy")
    assert a.dtype == np.float32 and np.array_equal(a, d_out.view(-1, 64).numpy())


@pytest.mark.gpu
def test_bench_plain_run_dumps_last_step_output(tmp_path):
    """A plain run (no --full): no CPU baseline, no output check, and the dumped coefficients
    are the oracle's for the frames the bench generates (seeds 1000 + f)."""
    import oracle as O
    W, H, q, frames = 256, 128, 90, 2
    r = subprocess.run([sys.executable, "bench.py", "--steps", "3", "--warmup", "1", "--settle-ms", "0",
                        "--width", str(W), "--height", str(H), "--quality", str(q),
                        "--frames-per-gpu", str(frames), "--dump-outputs", str(tmp_path)],
                       cwd=REPO, capture_output=True, text=True, timeout=240)
    assert r.returncode == 0, r.stderr[-2000:]
    lines = [ln for ln in r.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1, r.stdout
    d = json.loads(lines[0])
    assert d["steps"] == 3 and d["ms_per_step"] > 0
    assert d["cpu_baseline"] is None and d["output_check"] is None
    assert 0 < d["roofline"]["frac"] < 1
    got = np.load(tmp_path / "coefficients.npy")
    ref = np.stack([O.blocks(O.gen_splitmix(1000 + f, W, H), q) for f in range(frames)])
    assert got.dtype == np.float32 and got.shape == (frames * 3 * (W // 8) * (H // 8), 64)
    assert np.array_equal(got, ref.reshape(-1, 64).astype(np.float32))
