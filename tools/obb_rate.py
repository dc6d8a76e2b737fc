#!/usr/bin/env python3
"""Time of the oriented tail (mars_hip_detect_obb_device: obb_decode_kernel + obb_sort_nms_kernel of csrc/hip/obb.hip) on the 640 x 640 obb
twin at batch 256 (bench.py's batch), beside the DFL tail's (mars_hip_detect_dfl_device: decode, sort + upright NMS) on the same batch in
the same process.  The oriented tail's figure is DEVICE time between two events the library records around it on the auxiliary stream
(mars_hip_obb_ms), median of --runs after --warmup on an otherwise idle device.  Beside it the wall time of either tail -- a host clock from
the call to the return of mars_hip_sync, work that ends in a device synchronise -- alternating the two, so that the two tails can be
compared like for like.  One JSON line; kept in profiles/obb_tail.json.

usage: tools/obb_rate.py [--batch 256] [--conf 0.25] [--runs 20] [--warmup 3]
"""
import argparse
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
    ap.add_argument("--batch", type=int, default=256)
    ap.add_argument("--conf", type=float, default=0.25)
    ap.add_argument("--runs", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--input", type=int, default=640)
    a = ap.parse_args()
    marsrt.nna_init()
    L = marsrt.lib()
    S, B = a.input, a.batch
    d = marsrt.synth_model(width_x16=4, input_hw=S, seed=1, head="obb")
    angs = marsrt.obb_twin_tensors(d)
    m = marsrt.Model(d, batch=B)
    shots = [lcg_frame(0x5EED0000 + k, m.input_view(0).shape[1]) for k in range(8)]
    for f in range(B):
        m.input_view(0)[f] = shots[f % 8]
    m.upload()
    m.run_device()
    o = marsrt.obb_opts(angs)
    stage, wall_dfl, wall_obb = [], [], []
    for k in range(a.warmup + a.runs):
        L.mars_hip_sync()
        t0 = time.perf_counter()
        m.detect_dfl_device(conf=a.conf)
        L.mars_hip_sync()
        t1 = time.perf_counter()
        m.detect_obb_device(o, conf=a.conf)
        L.mars_hip_sync()
        t2 = time.perf_counter()
        if k >= a.warmup:
            wall_dfl.append((t1 - t0) * 1e3)
            wall_obb.append((t2 - t1) * 1e3)
            stage.append(m.obb_ms())
    boxes = m.obb_results()
    m.detect_dfl_device(conf=a.conf)
    upright = m.detect_results()
    med = float(np.median(stage))
    out = {"tool": "tools/obb_rate.py", "model": "synthetic obb twin, width_x16 4, %dx%d" % (S, S), "batch": B, "conf": a.conf, "runs": a.runs,
           "warmup": a.warmup, "oriented_boxes_kept": int(sum(len(x) for x in boxes)), "upright_boxes_kept": int(sum(len(x) for x in upright)),
           "obb_tail_device_ms_median": round(med, 4), "obb_tail_device_ms_min_max": [round(min(stage), 4), round(max(stage), 4)],
           "obb_tail_wall_ms_median": round(float(np.median(wall_obb)), 4), "obb_tail_wall_ms_min_max": [round(min(wall_obb), 4), round(max(wall_obb), 4)],
           "dfl_tail_wall_ms_median": round(float(np.median(wall_dfl)), 4), "dfl_tail_wall_ms_min_max": [round(min(wall_dfl), 4), round(max(wall_dfl), 4)],
           "wall_times": "host clock from the call to the return of mars_hip_sync, on an idle device; the device time is between the library's events"}
    m.close()
    print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
