"""bench.py command line: the result line, --dump-outputs and --full."""

import io
import json
import os
import sys
from contextlib import redirect_stdout

import numpy as np
import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)


def _run_bench(argv):
    import bench

    old = sys.argv
    sys.argv = ["bench.py"] + argv
    buf = io.StringIO()
    try:
        with redirect_stdout(buf):
            bench.main()
    finally:
        sys.argv = old
    lines = [l for l in buf.getvalue().splitlines() if l.startswith("{")]
    assert len(lines) == 1
    return json.loads(lines[0])


def test_bench_dump_outputs_reproducible(tmp_path):
    """Two runs with the same arguments dump identical float arrays, and
    the result line carries the requested step count and ms_per_step."""
    argv = ["--gpus", "1", "--steps", "3", "--warmup", "1", "--batch", "16"]
    recs, dumps = [], []
    for sub in ("a", "b"):
        d = tmp_path / sub
        recs.append(_run_bench(argv + ["--dump-outputs", str(d)]))
        dumps.append({f: np.load(d / f) for f in sorted(os.listdir(d))})

    rec = recs[0]
    assert rec["steps"] == 3 and rec["warmup"] == 1
    assert rec["ms_per_step"] > 0
    assert rec["unit"] == "images/sec" and rec["higher_is_better"] is True
    # value and ms_per_step describe the same timed window
    assert rec["value"] == pytest.approx(16 / rec["ms_per_step"] * 1000.0,
                                         rel=1e-3)
    assert "top1" not in rec

    a, b = dumps
    assert a.keys() == b.keys()
    assert "loss.npy" in a
    assert any(k.startswith("param.") for k in a)
    assert any(k.startswith("grad.") for k in a)
    assert sum(v.nbytes for v in a.values()) <= 64 << 20
    # Same seeded inputs both times, and every cross-block reduction that
    # feeds the update has a fixed order, so all arrays match bit for bit.
    # Only the GPU's scalar mean of the 16 per-sample fp32 losses is summed
    # in varying order: at most 16 roundings of 2**-24 relative each.
    import torch
    loss_tol = 16 * 2.0 ** -24 if torch.cuda.is_available() else 0.0
    for k in a:
        assert a[k].dtype in (np.float32, np.float64), k
        assert a[k].shape == b[k].shape, k
        if k == "loss.npy":
            assert abs(float(a[k]) - float(b[k])) <= loss_tol * abs(float(a[k]))
        else:
            assert np.array_equal(a[k], b[k]), k
    assert np.isfinite(a["loss.npy"]).all()


def test_bench_top1_needs_full():
    """The accuracy run belongs to --full; a plain run refuses it."""
    with pytest.raises(SystemExit):
        _run_bench(["--steps", "1", "--warmup", "0", "--batch", "16",
                    "--top1", "1"])
