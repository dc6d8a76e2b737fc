#!/usr/bin/env python3
"""Time of the keypoint stage (mars_hip_detect_pose_device: the selection launch + the gather launch of csrc/hip/pose.hip, behind the DFL
tail) on the 640 x 640 pose twin at batch 256 (bench.py's batch), max_per_frame 32.  The stage's figure is DEVICE time between two events
the library records around it on the auxiliary stream (mars_hip_pose_ms), median of --runs after --warmup on an otherwise idle device.
Beside it, for the same batch in the same process: the wall time of the DFL tail alone (mars_hip_detect_dfl_device to mars_hip_sync, a host
clock around work that ends in a device synchronise) and of the pose call (DFL tail + keypoint stage) measured the same way, alternating
the two, so that the stage's share of the tail can be read off; and the stage's algorithmic bytes (the selected cells' keypoint rows and
confidences read, the records and keypoints written).  One JSON line; kept in profiles/pose_tail.json.

usage: tools/pose_rate.py [--batch 256] [--max-per-frame 32] [--runs 20] [--warmup 3]
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
    ap.add_argument("--max-per-frame", type=int, default=32)
    ap.add_argument("--runs", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--input", type=int, default=640)
    a = ap.parse_args()
    marsrt.nna_init()
    L = marsrt.lib()
    S, B, M, K, D = a.input, a.batch, a.max_per_frame, 17, 3
    d = marsrt.synth_model(width_x16=4, input_hw=S, seed=1, head="pose")
    kpts = marsrt.pose_twin_tensors(d)
    m = marsrt.Model(d, batch=B)
    shots = [lcg_frame(0x5EED0000 + k, m.input_view(0).shape[1]) for k in range(8)]
    for f in range(B):
        m.input_view(0)[f] = shots[f % 8]
    m.upload()
    m.run_device()
    o = marsrt.pose_opts(kpts, num_kpt=K, kpt_dim=D, max_per_frame=M)
    stage, wall_dfl, wall_pose = [], [], []
    for k in range(a.warmup + a.runs):
        L.mars_hip_sync()
        t0 = time.perf_counter()
        m.detect_dfl_device()
        L.mars_hip_sync()
        t1 = time.perf_counter()
        m.detect_pose_device(o)
        L.mars_hip_sync()
        t2 = time.perf_counter()
        if k >= a.warmup:
            wall_dfl.append((t1 - t0) * 1e3)
            wall_pose.append((t2 - t1) * 1e3)
            stage.append(m.pose_ms())
    dets = m.detect_results()
    recs, kp = m.pose_results()
    taken = int((recs["det"] >= 0).sum())
    algo_b = taken * (K * D + 4 + 4) + recs.nbytes + kp.nbytes
    med = float(np.median(stage))
    out = {"tool": "tools/pose_rate.py", "model": "synthetic pose twin, width_x16 4, %dx%d" % (S, S), "batch": B, "max_per_frame": M,
           "keypoints": "%d x %d int8 per cell" % (K, D), "runs": a.runs, "warmup": a.warmup,
           "detections_kept": int(sum(len(x) for x in dets)), "poses_taken": taken,
           "pose_stage_device_ms_median": round(med, 4), "pose_stage_device_ms_min_max": [round(min(stage), 4), round(max(stage), 4)],
           "dfl_tail_wall_ms_median": round(float(np.median(wall_dfl)), 4), "dfl_tail_wall_ms_min_max": [round(min(wall_dfl), 4), round(max(wall_dfl), 4)],
           "pose_call_wall_ms_median": round(float(np.median(wall_pose)), 4), "pose_call_wall_ms_min_max": [round(min(wall_pose), 4), round(max(wall_pose), 4)],
           "wall_times": "host clock from the call to the return of mars_hip_sync; the pose call is the DFL tail + the keypoint stage",
           "algorithmic_bytes": int(algo_b), "implied_GBs": round(algo_b / (med * 1e-3) / 1e9, 2)}
    m.close()
    print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
