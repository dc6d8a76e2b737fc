#!/usr/bin/env python3
"""Cost of the best-shots stage (mars_hip_shots_device / mars_yolo_shot_lists: the three launches of csrc/hip/shots.hip) beside the device
copy rate of the same machine.

One workload: 256 crops of 160 x 160 x 3 int8, [th][tw][3], over 64 camera streams, one step per call (4 tracked crops per frame), 16
table slots per stream.  The crops are random textures, every other one blurred; the confidences are drawn anew for every call, so the
winners change and the copy kernel has work.  Reported per call, median (min .. max) over --runs calls after --warmup:
  shots_device_ms       mars_hip_shots_ms: the three kernels (metrics, walk, copy) between two events on their stream;
  shots_lists_wall_ms   host wall time of mars_yolo_shot_lists: upload of 19.7 MB of crops and the lists, the launches, the download, the waits.
  metrics_read_gbs      the bytes the metrics kernel must read (256 x 76 800) over the device time of all three kernels: a lower bound of
                        that kernel's own rate, since the walk and the copy are inside the interval;
  copy_rate_gbs         what bench.py's probe (libmars_probe.so: a 1 GiB device-to-device copy, read + write bytes over time) reaches here;
  frac_of_copy_rate     metrics_read_gbs / copy_rate_gbs.
The counters of the run are printed beside them: the workload is not an idle one.  No target is set for any of these figures.

One JSON line; kept in profiles/shots_rate.json.

usage: tools/shots_rate.py [--runs 20] [--warmup 4] [--out FILE]
"""
import argparse
import ctypes as C
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "thingino-accel_amd"))

import marsrt  # noqa: E402

TW, TH, S, PER_FRAME, SLOTS = 160, 160, 64, 4, 16
N = S * PER_FRAME


def stats(v):
    return dict(median=round(float(np.median(v)), 4), min=round(min(v), 4), max=round(max(v), 4))


def copy_rate():
    L = C.CDLL(os.path.join(ROOT, "thingino-accel_amd", "lib", "libmars_probe.so"))
    L.mars_probe_copy_rate_gbs.restype = C.c_double
    L.mars_probe_copy_rate_gbs.argtypes = [C.c_size_t, C.c_int]
    return float(L.mars_probe_copy_rate_gbs(1 << 30, 10))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--runs", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=4)
    ap.add_argument("--out")
    a = ap.parse_args()
    marsrt.nna_init()
    rng = np.random.default_rng(0x5407)
    u = rng.integers(0, 256, (N, TH, TW, 3), dtype=np.uint8)
    soft = (u[1::2].astype(np.uint16) + np.roll(u[1::2], 1, axis=1) + np.roll(u[1::2], 1, axis=2) + np.roll(u[1::2], (1, 1), axis=(1, 2))) // 4
    u[1::2] = soft.astype(np.uint8)
    crops = (u.astype(np.int16) - 128).astype(np.int8).reshape(N, -1)
    rois = np.zeros(N, dtype=marsrt.ROI_DTYPE)
    rois["frame"] = np.arange(N) % S
    rois["x0"], rois["y0"] = rng.integers(0, 1000, N), rng.integers(0, 500, N)
    rois["x1"], rois["y1"] = rois["x0"] + rng.integers(40, 280, N), rois["y0"] + rng.integers(40, 220, N)
    tracks = np.zeros(N, dtype=marsrt.TRACK_DTYPE)
    tracks["id"] = 1 + np.arange(N) // S
    cls = np.zeros(N, dtype=np.int32)
    sh = marsrt.Shots(S, SLOTS, TW, TH, True)
    opts = marsrt.shot_opts()
    dev, wall = [], []
    L = marsrt.lib()
    for k in range(a.warmup + a.runs):
        confs = rng.uniform(0.3, 1.0, N).astype(np.float32)
        tracks["hits"] = k + 1
        L.mars_hip_sync()
        t0 = time.perf_counter()
        rec = marsrt.shot_lists(sh, crops, rois, confs, cls, tracks, S, opts)
        t1 = time.perf_counter()
        if k >= a.warmup:
            wall.append((t1 - t0) * 1e3)
            dev.append(sh.ms())
    cnt = np.zeros(6, dtype=np.int64)
    live = 0
    for b in range(S):
        c, lv, _, _ = sh.read(b)
        cnt += c
        live += lv
    sh.close()
    nbytes = N * TW * TH * 3
    gbs = nbytes / (float(np.median(dev)) * 1e-3) / 1e9
    cp = copy_rate()
    res = {"tool": "tools/shots_rate.py", "streams": S, "steps_per_call": 1, "crops": N, "crop": [TW, TH, 3], "layout": "nhwc", "slots": SLOTS,
           "calls": a.warmup + a.runs, "runs": a.runs, "warmup": a.warmup, "crop_bytes_per_call": nbytes,
           "shots_device_ms": stats(dev), "shots_lists_wall_ms": stats(wall),
           "metrics_read_gbs": round(gbs, 1), "copy_rate_gbs": round(cp, 1), "frac_of_copy_rate": round(gbs / cp, 4) if cp > 0 else None,
           "taken_last_call": int(rec["taken"].sum()), "mean_sharp_last_call": round(float(rec["sharp"].mean()), 1),
           "counters": dict(zip(("finished", "lost", "dropped", "overflow", "duplicates", "taken"), (int(v) for v in cnt))), "live_slots": live}
    line = json.dumps(res)
    print(line, flush=True)
    if a.out:
        with open(a.out, "w") as fh:
            fh.write(line + "\n")


if __name__ == "__main__":
    main()
