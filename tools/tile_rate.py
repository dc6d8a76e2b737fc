#!/usr/bin/env python3
"""Time of the tiled-inference stages (include/mars_hip.h, "Tiled inference") on the 640 x 640 DFL twin: 16 camera frames of 1920 x 1080, each
cut into the 8 tiles of mars_tile_grid(1920, 1080, 640, 640, 128, 128) plus one whole-frame tile -- 9 tiles, batch 144 (not bench.py's 256:
the nearest batch that is a multiple of 9 tiles x 16 frames).
  front-end  mars_hip_preprocess_tiles_device (tile_rois_kernel + roi_crop_kernel) from frames in HBM: DEVICE time between two HIP events this
             tool records around the call on the library's stream (mars_hip_stream), and the wall time -- a host clock from the call to the
             return of mars_hip_sync on an otherwise idle device;
  merge      mars_hip_merge_tiles_device (tile_merge_kernel): DEVICE time between two events the library records around it on the auxiliary
             stream (mars_hip_tile_ms), median of --runs after --warmup, and the same wall time;
  DFL tail   mars_hip_detect_dfl_device on the same batch in the same process, wall time, alternating with the merge, so that the two can
             be compared like for like.
One JSON line; kept in profiles/tile_merge.json (--out writes it there).

usage: tools/tile_rate.py [--cams 16] [--conf 0.25] [--runs 20] [--warmup 3] [--out FILE]
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

import marsrt  # noqa: E402
from conftest import lcg_frame  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--cams", type=int, default=16)
    ap.add_argument("--conf", type=float, default=0.25)
    ap.add_argument("--runs", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--input", type=int, default=640)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    marsrt.nna_init()
    L = marsrt.lib()
    S, W, H = a.input, 1920, 1080
    tiles = np.concatenate([marsrt.tile_grid(W, H, S, S, S // 5, S // 5), np.array([(0, 0, W, H)], dtype=marsrt.TILE_DTYPE)])
    T, B = len(tiles), len(tiles) * a.cams
    o = marsrt.tile_opts(W, H, tiles, keep_aspect=True)
    d = marsrt.synth_model(width_x16=4, input_hw=S, seed=1, head="dfl")
    m = marsrt.Model(d, batch=B)
    shots = [lcg_frame(0x5EED0000 + k, W * H * 3) for k in range(4)]
    buf = marsrt.DeviceBuffer(np.stack([shots[c % 4] for c in range(a.cams)]))
    hip, stream = buf._hip, C.c_void_p(L.mars_hip_stream())
    ev = [C.c_void_p(), C.c_void_p()]
    for e in ev:
        if hip.hipEventCreate(C.byref(e)) != 0:
            raise RuntimeError("hipEventCreate")
    front, front_dev, wall_dfl, wall_merge, stage = [], [], [], [], []
    for k in range(a.warmup + a.runs):
        L.mars_hip_sync()
        t0 = time.perf_counter()
        hip.hipEventRecord(ev[0], stream)
        m.preprocess_tiles(buf.ptr, o, device=True)
        hip.hipEventRecord(ev[1], stream)
        L.mars_hip_sync()
        t1 = time.perf_counter()
        ms = C.c_float(-1.0)
        if hip.hipEventElapsedTime(C.byref(ms), ev[0], ev[1]) != 0:
            raise RuntimeError("hipEventElapsedTime")
        if k == 0:
            m.run_device()
        L.mars_hip_sync()
        t2 = time.perf_counter()
        m.detect_dfl_device(conf=a.conf)
        L.mars_hip_sync()
        t3 = time.perf_counter()
        m.merge_tiles(o)
        L.mars_hip_sync()
        t4 = time.perf_counter()
        if k >= a.warmup:
            front.append((t1 - t0) * 1e3)
            front_dev.append(float(ms.value))
            wall_dfl.append((t3 - t2) * 1e3)
            wall_merge.append((t4 - t3) * 1e3)
            stage.append(m.tile_ms())
    lists = m.detect_results()
    _, counts, _, stats = m.tile_results()
    for e in ev:
        hip.hipEventDestroy(e)
    buf.free()

    def mm(v):
        return [round(min(v), 4), round(max(v), 4)]

    med_merge, med_dfl = float(np.median(wall_merge)), float(np.median(wall_dfl))
    out = {"tool": "tools/tile_rate.py", "model": "synthetic DFL twin, width_x16 4, %dx%d" % (S, S), "camera_frames": a.cams, "frame": [W, H],
           "tiles_per_frame": T, "batch": B, "conf": a.conf, "runs": a.runs, "warmup": a.warmup,
           "per_tile_boxes": int(sum(len(x) for x in lists)), "candidates": int(stats["candidates"].sum()), "overflow": int(stats["overflow"].sum()),
           "suppressed": int(stats["suppressed"].sum()), "truncated": int(stats["truncated"].sum()), "merged_boxes": int(counts.sum()),
           "front_end_device_ms_median": round(float(np.median(front_dev)), 4), "front_end_device_ms_min_max": mm(front_dev),
           "front_end_wall_ms_median": round(float(np.median(front)), 4), "front_end_wall_ms_min_max": mm(front),
           "merge_device_ms_median": round(float(np.median(stage)), 4), "merge_device_ms_min_max": mm(stage),
           "merge_wall_ms_median": round(med_merge, 4), "merge_wall_ms_min_max": mm(wall_merge),
           "dfl_tail_wall_ms_median": round(med_dfl, 4), "dfl_tail_wall_ms_min_max": mm(wall_dfl),
           "merge_longer_than_dfl_tail": bool(med_merge > med_dfl),
           "wall_times": "host clock from the call to the return of mars_hip_sync, on an idle device; the device time is between the library's events"}
    m.close()
    line = json.dumps(out)
    print(line, flush=True)
    if a.out:
        with open(a.out, "w") as fh:
            fh.write(line + "\n")


if __name__ == "__main__":
    main()
