#!/usr/bin/env python3
"""Throughput of single_end_mappability_from_sam (xenomappability step 3, 8f-4) with and without on_device=True, on one synthetic
name-sorted SAM of simulated 100 bp reads: two chromosomes, a stretch of unmapped reads at the start of each.

    python tools/bench_mappability.py [--lines 2000000] [--rounds 5] [--file reads.sam]

One warm-up of each route, then `rounds` alternations device / host on the same file in one process; prints one JSON line with
the median and the spread of each route's seconds, lines/s and GB/s of text, the device time per window (HIP events) and where
the device route's wall time goes (reading windows, inside xm_mapp_run, walking segments, writing the wiggle text)."""
import argparse
import json
import os
import statistics
import sys
import tempfile
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from xenomapper_amd import mappability as mp, synth  # noqa: E402


def write_sam(path, n_lines, seed=11, unmapped=2000, read_len=100):
    """Reads chrN_1 .. of two chromosomes in name order: the first `unmapped` of each not mapped at all (RNAME '*'), of the rest
    nine in ten back where they came from with MAPQ 42, the others somewhere else with a low MAPQ."""
    rng = np.random.default_rng(seed)
    pool = [(synth._rand_seq(rng, read_len), synth._rand_qual(rng, read_len)) for _ in range(512)]
    with open(path, "w") as fh:
        fh.write("@HD\tVN:1.0\tSO:queryname\n@SQ\tSN:chr1\tLN:%d\n@SQ\tSN:chr2\tLN:%d\n" % (n_lines, n_lines))
        for chrom, other, count in (("chr1", "chr2", n_lines // 2), ("chr2", "chr1", n_lines - n_lines // 2)):
            home = rng.random(count) < 0.9
            pick = rng.integers(0, len(pool), count)
            away = rng.integers(1, count + 1, count)
            for start in range(0, count, 1 << 16):
                rows = []
                for k in range(start, min(count, start + (1 << 16))):
                    seq, qual = pool[pick[k]]
                    if k < unmapped:
                        rows.append("%s_%d\t4\t*\t0\t0\t*\t*\t0\t0\t%s\t%s\tYT:Z:UU\n" % (chrom, k + 1, seq, qual))
                    elif home[k]:
                        rows.append("%s_%d\t0\t%s\t%d\t42\t%dM\t*\t0\t0\t%s\t%s\tAS:i:0\tXN:i:0\tNM:i:0\tYT:Z:UU\n"
                                    % (chrom, k + 1, chrom, k + 1, read_len, seq, qual))
                    else:
                        rows.append("%s_%d\t16\t%s\t%d\t1\t%dM\t*\t0\t0\t%s\t%s\tAS:i:-12\tXS:i:-12\tNM:i:2\tYT:Z:UU\n"
                                    % (chrom, k + 1, other, away[k], read_len, seq, qual))
                fh.write("".join(rows))


def once(path, on_device):
    with open(path) as fh, open(os.devnull, "w") as out:
        t0 = time.perf_counter()
        mp.single_end_mappability_from_sam(fh, outfile=out, on_device=on_device)
        return time.perf_counter() - t0


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--lines", type=int, default=2_000_000)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--file", help="keep the synthetic SAM here (made when missing)")
    args = ap.parse_args()
    path = args.file or os.path.join(tempfile.mkdtemp(prefix="xm_mapp_"), "reads.sam")
    if not os.path.exists(path):
        write_sam(path, args.lines)
    size = os.path.getsize(path)
    once(path, True), once(path, False)                                # warm-up: buffers allocated and page-locked, the file cached
    seconds = {True: [], False: []}
    runs = []
    for _ in range(args.rounds):
        for on_device in (True, False):
            seconds[on_device].append(once(path, on_device))
            if on_device:
                runs.append(dict(mp.last_run))
    lines = runs[-1]["lines"]

    def summary(values):
        med = statistics.median(values)
        return dict(median_s=med, min_s=min(values), max_s=max(values), lines_per_s=lines / med, GB_per_s=size / med / 1e9)
    windows = max(1, runs[-1]["windows_device"] + runs[-1]["windows_host"])
    med = {k: statistics.median(r[k] for r in runs) for k in ("ms_upload", "ms_kernels", "s_read", "s_device", "s_walk")}
    device_s = statistics.median(seconds[True])
    print(json.dumps(dict(
        bench="single_end_mappability_from_sam", lines=lines, bytes=size, rounds=args.rounds, window_bytes=mp._window_bytes(),
        windows_device=runs[-1]["windows_device"], windows_host=runs[-1]["windows_host"], reasons=runs[-1]["reasons"],
        on_device=summary(seconds[True]), host=summary(seconds[False]),
        speedup=statistics.median(seconds[False]) / device_s,
        ms_upload_per_window=med["ms_upload"] / windows, ms_kernels_per_window=med["ms_kernels"] / windows,
        upload_GB_per_s=size / max(med["ms_upload"], 1e-9) / 1e6, kernels_GB_per_s=size / max(med["ms_kernels"], 1e-9) / 1e6,
        share=dict(read=med["s_read"] / device_s, xm_mapp_run=med["s_device"] / device_s, walk=med["s_walk"] / device_s,
                   write_and_rest=1.0 - (med["s_read"] + med["s_device"] + med["s_walk"]) / device_s))))
    if not args.file:
        os.remove(path)
        os.rmdir(os.path.dirname(path))


if __name__ == "__main__":
    main()
