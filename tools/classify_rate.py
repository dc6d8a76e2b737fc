#!/usr/bin/env python3
"""Time of the classify tail (mars_hip_classify_device: the pooling launch + the finishing launch) on the shipped tiny_160_int8.mars at batch
1 024: 1 024 output maps (64 x 154 x 154 int8, what its three unpadded convolutions leave of 160 x 160) in HBM -> top-K entries per frame.  The tail runs on the library's auxiliary stream, which no
caller can put events on, so the figure is host wall time from the call to the end of mars_hip_sync() on an otherwise idle device, median
of --runs after --warmup, with the same measurement around an empty mars_hip_sync() beside it (the part that is not device time).
Beside it: the bytes-read floor (the maps' bytes) at this box's copy rate, measured in the same process by bench.py's probe
(a 1 GiB device copy, read + write bytes over time), and the wall time of the path the tail replaces, measured once in the same run:
mars_hip_read_tensor of every frame plus the numpy pooling and ranking.  One JSON line; kept in profiles/classify_tail.json.  For the split
between the two launches run it under `rocprofv3 --kernel-trace --stats -- python ...`.

usage: tools/classify_rate.py [--batch 1024] [--top-k 3] [--runs 30] [--warmup 5]
"""
import argparse
import ctypes as C
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "thingino-accel_amd"))

import marsfile  # noqa: E402
import marsrt  # noqa: E402
from conftest import lcg_frame  # noqa: E402


def wall_ms(fn, runs, warmup):
    L = marsrt.lib()
    for _ in range(warmup):
        fn()
        L.mars_hip_sync()
    t = []
    for _ in range(runs):
        L.mars_hip_sync()
        t0 = time.perf_counter()
        fn()
        L.mars_hip_sync()
        t.append((time.perf_counter() - t0) * 1e3)
    return float(np.median(t)), float(min(t)), float(max(t))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=1024)
    ap.add_argument("--top-k", type=int, default=3)
    ap.add_argument("--runs", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    a = ap.parse_args()
    marsrt.nna_init()
    with open(os.path.join(ROOT, "tests", "golden", "models", "tiny_160_int8.mars"), "rb") as fh:
        d = fh.read()
    hdr, tensors, _ = marsfile.parse(d)
    tout = hdr["outputs"][0]
    t = tensors[tout]
    nhwc = t["fmt"] == marsfile.NHWC
    Cc, H, W = (t["shape"][3], t["shape"][1], t["shape"][2]) if nhwc else tuple(t["shape"][1:])
    m = marsrt.Model(d, batch=a.batch)
    shots = [lcg_frame(0xC1A50000 + k, m.input_view(0).shape[1]) for k in range(8)]
    for f in range(a.batch):
        m.input_view(0)[f] = shots[f % 8]
    m.upload()
    m.run_device()
    o = marsrt.cls_opts(top_k=a.top_k)
    tail = wall_ms(lambda: m.classify_device(o), a.runs, a.warmup)
    empty = wall_ms(lambda: None, a.runs, a.warmup)
    top, sums = m.classify_results(a.top_k)
    read_b = a.batch * Cc * H * W
    probe = C.CDLL(os.path.join(ROOT, "thingino-accel_amd", "lib", "libmars_probe.so"))
    probe.mars_probe_copy_rate_gbs.restype = C.c_double
    probe.mars_probe_copy_rate_gbs.argtypes = [C.c_size_t, C.c_int]
    copy_gbs = float(probe.mars_probe_copy_rate_gbs(1 << 30, 10))
    floor_ms = read_b / (copy_gbs * 1e9) * 1e3 if copy_gbs > 0 else None
    # the path the tail replaces: every frame over the host link, pooled and ranked there
    t0 = time.perf_counter()
    host_sums = np.empty((a.batch, Cc), dtype=np.int64)
    for f in range(a.batch):
        x = m.read_tensor(tout, frame=f).view(np.int8)
        host_sums[f] = (x.reshape(H * W, Cc) if nhwc else x.reshape(Cc, H * W).T).sum(axis=0, dtype=np.int64)
    order = np.argsort(-host_sums, axis=1, kind="stable")[:, :a.top_k]
    host_ms = (time.perf_counter() - t0) * 1e3
    assert np.array_equal(host_sums.astype(np.int32), sums) and np.array_equal(order, top["cls"])
    out = {"tool": "tools/classify_rate.py", "model": "tiny_160_int8.mars", "batch": a.batch, "map": "%dx%dx%d int8, %s" % (Cc, H, W, "pixel rows" if nhwc else "planes"),
           "top_k": a.top_k, "runs": a.runs, "warmup": a.warmup,
           "classify_wall_ms_median": round(tail[0], 4), "classify_wall_ms_min_max": [round(tail[1], 4), round(tail[2], 4)],
           "empty_sync_wall_ms_median": round(empty[0], 4),
           "bytes_read": read_b, "copy_rate_GBs_measured": round(copy_gbs, 1), "floor_ms_at_copy_rate": round(floor_ms, 4) if floor_ms else None,
           "floor_over_classify_wall": round(floor_ms / tail[0], 4) if floor_ms else None,
           "floor_over_classify_wall_less_empty_sync": round(floor_ms / max(tail[0] - empty[0], 1e-6), 4) if floor_ms else None,
           "effective_read_GBs": round(read_b / (tail[0] * 1e-3) / 1e9, 1),
           "host_path_wall_ms": round(host_ms, 1), "host_path": "read_tensor of every frame + numpy sum and stable argsort",
           "host_path_over_classify": round(host_ms / tail[0], 1)}
    m.close()
    print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
