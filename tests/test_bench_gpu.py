"""bench.py as the driver runs it: a plain run prints the headline line only, and --dump-outputs writes what the
timed step computed -- checked here against the C oracle on the same synthetic columns."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

from tests import helpers as H


@pytest.mark.gpu
def test_plain_run_dumps_what_the_last_timed_step_computed(tmp_path):
    sys.path.insert(0, H.REPO)
    import bench
    import torch
    from xenomapper_amd import _ffi, synth
    pairs, steps = 1_000_000, 3
    proc = subprocess.run([sys.executable, os.path.join(H.REPO, "bench.py"), "--gpus", "1", "--steps", str(steps), "--warmup", "1",
                           "--pairs", str(pairs), "--dump-outputs", str(tmp_path)], capture_output=True, text=True, timeout=600)
    assert proc.returncode == 0, proc.stderr[-2000:]
    lines = [l for l in proc.stdout.splitlines() if l.strip()]
    assert len(lines) == 1, proc.stdout[-2000:]
    rec = json.loads(lines[0])
    assert rec["steps"] == steps and rec["dtype"] == "int32" and rec["higher_is_better"] is True
    assert abs(rec["value"] - pairs * steps / (rec["ms_per_step"] * steps * 1e-3)) / rec["value"] < 1e-4
    assert not {"kernel_ms", "roofline_step", "cpu_baseline", "e2e", "workloads", "full_record"} & set(rec)

    # the same columns (synth.score_columns_torch, seed 2002 for rank 0), the C oracle on them
    cols = {k: v.cpu().numpy() for k, v in synth.score_columns_torch(pairs, seed=2002, device=torch.device("cuda:0")).items()}
    mode = _ffi.MODE_PE_LIBERAL
    code, counts = H.c_classify(mode, cols["as1"], cols["xs1"], cols["as2"], cols["xs2"], cols["unit_bits"].view(np.uint64), _ffi.ABSENT)
    idx, off = H.c_compact(mode, code)
    bins = np.full(code.shape[0], 7, dtype=np.uint8)
    for b in range(7):
        bins[idx[int(off[b]):int(off[b + 1])]] = b

    def sampled(a):
        if a.shape[0] > bench.DUMP_SAMPLE:
            a = a[np.unique(np.random.default_rng(bench.DUMP_SEED).integers(0, a.shape[0], bench.DUMP_SAMPLE))]
        return a.astype(np.float64)
    got = {k: np.load(tmp_path / (k + ".npy")) for k in ("idx", "off", "bins", "counts", "job_counts")}
    assert np.array_equal(got["off"], off.astype(np.float64))
    assert np.array_equal(got["idx"], sampled(idx[:int(off[7])]))
    assert np.array_equal(got["bins"], sampled(bins))
    assert np.array_equal(got["counts"], counts.astype(np.float64))
    assert np.array_equal(got["job_counts"], steps * counts.astype(np.float64))
