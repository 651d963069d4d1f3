#!/usr/bin/env python3
"""SAM lines encoded as BAM records on the device (xm_strip_fetch_bins_bam) beside the text gather (xm_strip_fetch_bins) of the same
classified block: bytes of both streams and the time of both calls, on one GPU, in one process, alternating.

    python tools/bench_samenc.py --window-mb 64 --reps 5

Input: the synthetic 2 x 150 bp paired SAM text twin tools/bench_e2e.py uses (50 k pairs, seed 2002), its body tiled to the window
size, one window per slot; the reference names come from its @SQ lines.  A time is a host clock around the call and the
xm_strip_out_wait behind it, which ends in a device synchronisation: it holds the kernels (E1, the scan, E2, F, CRC, frames -- or G1,
the scan, G2) AND the stream's copy to page-locked host memory.  The kernels' own shares are not split here: take them from a
kernel trace of this program run on its own (the kernels have stable names: sam_enc_size_kernel, sam_enc_write_kernel,
sam_enc_frame_copy_kernel, sam_unit_size_kernel, sam_line_copy_kernel).  No pass mark; prints one JSON line.  Needs a GPU."""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)


def window_texts(window_bytes):
    from xenomapper_amd import synth
    t1, t2, _ = synth.sam_text_pair(n_pairs=50_000, seed=2002, profile="bowtie2", paired=True, read_len=150)
    out, names = [], []
    for text in (t1, t2):
        head_end = 0
        while text[head_end] == "@":
            head_end = text.index("\n", head_end) + 1
        names.append([ln.split("\t")[1][3:].encode() for ln in text[:head_end].split("\n") if ln.startswith("@SQ")])
        body = text[head_end:].encode("ascii")
        out.append(body * max(1, window_bytes // len(body)))
    return out, names


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--window-mb", type=int, default=64)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--block-payload", type=int, default=0)
    args = ap.parse_args()
    from xenomapper_amd import _ffi
    from xenomapper_amd.xenomapper import default_context
    (b1, b2), names = window_texts(args.window_mb << 20)
    s = _ffi.Stripper(default_context())
    try:
        for f in (0, 1):
            s.set_refs(f, names[f])
        max_records = max(b1.count(b"\n"), b2.count(b"\n")) + 16
        result = {"metric": "SAM window -> six outputs on the device: BAM records (stored members) beside text", "window_bytes": [len(b1), len(b2)],
                  "block_payload": args.block_payload or 65280, "slots": []}
        for slot in (0, 1):
            s.reserve(slot, max(len(b1), len(b2)), max_records)
            for f, b in enumerate((b1, b2)):
                s.staging(slot, f)[:len(b)] = np.frombuffer(b, dtype=np.uint8)
            got = s.run(slot, len(b1), True, len(b2), True, 0, True, False, False, max_records)
            s.classify(slot, 1, got.n, -2 ** 31)
            times = {"text": [], "bam": []}
            sizes = {}
            for rep in range(args.reps + 1):                                # (the first round warms both calls up and is dropped)
                for kind in ("text", "bam"):
                    t0 = time.perf_counter()
                    if kind == "text":
                        status, _stream, boff = s.fetch_bins(slot, got.n, True, 0b111111)
                    else:
                        status, _stream, boff, declined = s.fetch_bins_bam(slot, got.n, True, 0b111111, args.block_payload, len(names[0]))
                    if status != 0:
                        raise RuntimeError("%s fetch: status %d" % (kind, status))
                    s.out_wait(slot)
                    if rep:
                        times[kind].append(time.perf_counter() - t0)
                    sizes[kind] = boff[7]
            result["slots"].append({"records": got.n, "text_bytes": sizes["text"], "bam_bytes": sizes["bam"],
                                    "bam_over_text": round(sizes["bam"] / max(sizes["text"], 1), 4),
                                    "text_ms_median": round(1e3 * statistics.median(times["text"]), 3),
                                    "bam_ms_median": round(1e3 * statistics.median(times["bam"]), 3),
                                    "text_ms": [round(1e3 * t, 3) for t in times["text"]], "bam_ms": [round(1e3 * t, 3) for t in times["bam"]]})
        print(json.dumps(result))
    finally:
        s.close()


if __name__ == "__main__":
    main()
