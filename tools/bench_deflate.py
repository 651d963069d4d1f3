#!/usr/bin/env python3
"""GB/s of input of the GPU BGZF encoder on the inflated bytes of a tiled BAM fixture -- one BAM-out window, ~0.5 GB:
xm_bgzf_deflate_dev alone (payload, slots and scratch resident in HBM, HIP events on the launch stream) and xm_bgzf_compress
(host buffer in, BGZF members out, wall clock: the copies over the link are in it), the ratio, and beside them on the same
payload zlib level 1 on one core of this box (x the 16 CPUs a job gets) and libdeflate level 1 where the library is installed.
Every stream's CRC is checked by inflating a sample with zlib, and the members of xm_bgzf_compress by gzip.

    python tools/bench_deflate.py --in-gb 0.5
"""
import argparse
import ctypes
import gzip
import json
import os
import sys
import time
import zlib

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.join(REPO, "tools"))
DATA = os.path.join(REPO, "tests", "golden", "ref_data")
PAYLOAD = 65280
CPUS = 16                                                   # what a job gets on the pool's machines
WINDOW_MS = 19.0                                            # what a BAM-out window's copy home takes today


def spread(ms):
    s = sorted(ms)
    return {"median": s[len(s) // 2], "min": s[0], "max": s[-1], "all": [round(x, 3) for x in ms]}


def libdeflate_rate(sample, level=1):
    """GB/s of libdeflate's raw-deflate compressor on one core, or None when the shared library is not installed"""
    try:
        L = ctypes.CDLL("libdeflate.so.0")
    except OSError:
        return None
    L.libdeflate_alloc_compressor.restype = ctypes.c_void_p
    L.libdeflate_deflate_compress.restype = ctypes.c_size_t
    L.libdeflate_deflate_compress.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_size_t, ctypes.c_void_p, ctypes.c_size_t]
    c = L.libdeflate_alloc_compressor(level)
    out = np.empty(PAYLOAD + 1024, dtype=np.uint8)
    t0, done, comp = time.perf_counter(), 0, 0
    for at in range(0, sample.shape[0], PAYLOAD):
        piece = sample[at:at + PAYLOAD]
        comp += L.libdeflate_deflate_compress(c, piece.ctypes.data, piece.shape[0], out.ctypes.data, out.shape[0])
        done += piece.shape[0]
    dt = time.perf_counter() - t0
    L.libdeflate_free_compressor.argtypes = [ctypes.c_void_p]
    L.libdeflate_free_compressor(c)
    return {"GBps_one_core": done / dt / 1e9, "ratio": comp / done}


def run(in_gb=0.5, reps=7, warmup=2, host_reps=3, workdir=None):
    import torch
    import bench_bam
    from xenomapper_amd import _ffi
    workdir = workdir or ("/dev/shm" if os.path.isdir("/dev/shm") else "/tmp")
    path = os.path.join(workdir, "xm_deflate_%d.bam" % os.getpid())
    copies = max(1, int(in_gb * 1e9 / 119_000))
    bench_bam.tiled_bam(os.path.join(DATA, "paired_end_testdata_human.bam"), path, copies, level=0)
    payload = np.frombuffer(gzip.decompress(open(path, "rb").read()), dtype=np.uint8)
    os.unlink(path)
    n = payload.shape[0]
    nb = (n + PAYLOAD - 1) // PAYLOAD
    slot = (PAYLOAD + 5 + 15) & ~15
    blocks = np.zeros(nb, dtype=_ffi.BGZF_BLOCK)
    blocks["cdata_off"] = np.arange(nb, dtype=np.uint64) * slot
    blocks["cdata_len"] = slot
    blocks["out_off"] = np.arange(nb, dtype=np.uint64) * PAYLOAD
    blocks["isize"] = np.minimum(PAYLOAD, n - np.arange(nb, dtype=np.int64) * PAYLOAD)
    dev = torch.device("cuda:0")
    ctx = _ffi.Context(0)
    d_in = torch.zeros(n + 16, dtype=torch.uint8, device=dev)
    d_in[:n] = torch.from_numpy(payload).to(dev)
    d_blocks = torch.from_numpy(blocks.view(np.uint8)).to(dev)
    comp = torch.empty(nb * slot, dtype=torch.uint8, device=dev)
    clen = torch.zeros(nb, dtype=torch.int32, device=dev)
    status = torch.zeros(nb, dtype=torch.int32, device=dev)
    work = torch.empty(_ffi.bgzf_deflate_work_bytes(), dtype=torch.uint8, device=dev)
    ms = []
    for it in range(warmup + reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        ctx.bgzf_deflate_dev(d_in, d_blocks, comp, clen, status, work)
        e1.record()
        torch.cuda.synchronize()
        if it >= warmup:
            ms.append(e0.elapsed_time(e1))
    h_clen, h_status = clen.cpu().numpy(), status.cpu().numpy()
    ok = bool((h_status == 0).all())
    h_comp = comp.cpu().numpy()
    for b in np.linspace(0, nb - 1, 64).astype(int):
        o, c = int(blocks["cdata_off"][b]), int(h_clen[b])
        p0, pn = int(blocks["out_off"][b]), int(blocks["isize"][b])
        ok &= zlib.decompress(h_comp[o:o + c].tobytes(), -15) == payload[p0:p0 + pn].tobytes()
    del comp, h_comp, d_in, work
    torch.cuda.empty_cache()
    dev_ms = spread(ms)
    # the host-buffer call: wall clock
    wall = []
    members = None
    for it in range(1 + host_reps):
        t0 = time.perf_counter()
        members = ctx.bgzf_compress(payload)
        if it:
            wall.append((time.perf_counter() - t0) * 1e3)
    ok &= gzip.decompress(members.tobytes() + _ffi.BGZF_EOF) == payload.tobytes()
    host_ms = spread(wall)
    ctx.close()
    # the host alternative, same payload (a 64 MB slice of it), one core
    sample = payload[:64 << 20]
    t0, zc = time.perf_counter(), 0
    for at in range(0, sample.shape[0], PAYLOAD):
        c = zlib.compressobj(1, zlib.DEFLATED, -15)
        zc += len(c.compress(sample[at:at + PAYLOAD]) + c.flush())
    z_rate = sample.shape[0] / (time.perf_counter() - t0) / 1e9
    ld = libdeflate_rate(sample)
    rate = n / (dev_ms["median"] * 1e-3) / 1e9
    host_best = max(z_rate, ld["GBps_one_core"] if ld else 0.0) * CPUS
    return {"metric": "GB/s of input (BGZF blocks deflated on the GPU)", "value": rate, "ms": dev_ms,
            "window_ms_at_0.55GB": 0.55e9 / (rate * 1e9) * 1e3,
            "compress_GBps": n / (host_ms["median"] * 1e-3) / 1e9, "compress_ms": host_ms,
            "input_bytes": int(n), "blocks": int(nb), "stream_bytes": int(h_clen.sum()), "ratio": float(h_clen.sum()) / n,
            "members_bytes": int(members.shape[0]), "verified": ok,
            "zlib_level1": {"GBps_one_core": z_rate, "GBps_x%d" % CPUS: z_rate * CPUS, "ratio": zc / sample.shape[0]},
            "libdeflate_level1": ld and dict(ld, **{"GBps_x%d" % CPUS: ld["GBps_one_core"] * CPUS}),
            "faster_than_host_x%d" % CPUS: bool(rate > host_best),
            "inside_the_window_copy": bool(0.55e9 / (rate * 1e9) * 1e3 < WINDOW_MS),
            "what": "xm_bgzf_deflate_dev on the inflated bytes of the human BAM fixture tiled to ~%.2f GB, cut every 65280 bytes, all "
                    "buffers resident in HBM, HIP events, %d warm-up launches, median / min / max of %d; xm_bgzf_compress on the same bytes "
                    "from pageable host memory, wall clock, median of %d; 64 streams and all members inflated by zlib"
                    % (in_gb, warmup, reps, host_reps)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--in-gb", type=float, default=0.5, help="payload bytes per launch")
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--dir", default=None)
    a = ap.parse_args()
    print(json.dumps(run(a.in_gb, a.reps, a.warmup, workdir=a.dir)))


if __name__ == "__main__":
    main()
