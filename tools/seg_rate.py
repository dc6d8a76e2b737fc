#!/usr/bin/env python3
"""Time of the mask stage (mars_hip_detect_seg_device: the selection launch + the mask launch of csrc/hip/seg.hip, behind the DFL tail) on the
640 x 640 seg twin at batch 256, max_per_frame 16.  The figure is DEVICE time between two events the library records around the stage on the
auxiliary stream (mars_hip_mask_ms), median of --runs after --warmup on an otherwise idle device.  Beside it: the stage's algorithmic bytes
(prototypes read once + the selected cells' coefficient rows + the mask words and records written) and the fraction of the 8 TB/s HBM roof
that this time implies, and the wall time of the path the stage replaces, measured once in the same run with the calls the library had
before it: mars_hip_detect_dfl, then mars_hip_read_tensor of the prototype and coefficient tensors of every frame and the masks in numpy
(tests/segref.py; the origin of each box, which those calls do not report, is GUESSED from the box's centre and size, so the host path's
masks are not compared: only its time is reported).  One JSON line; kept in profiles/seg_tail.json.

usage: tools/seg_rate.py [--batch 256] [--max-per-frame 16] [--runs 20] [--warmup 3]
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

import marsfile  # noqa: E402
import marsrt  # noqa: E402
import segref  # noqa: E402
from conftest import lcg_frame  # noqa: E402

HBM_ROOF_GBS = 8000.0


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=256)
    ap.add_argument("--max-per-frame", type=int, default=16)
    ap.add_argument("--runs", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--input", type=int, default=640)
    a = ap.parse_args()
    marsrt.nna_init()
    L = marsrt.lib()
    S, B, M = a.input, a.batch, a.max_per_frame
    d = marsrt.synth_model(width_x16=4, input_hw=S, seed=1, head="seg")
    hdr, tensors, _ = marsfile.parse(d)
    coefs, pr = marsrt.seg_twin_tensors(d)
    heads = marsrt.find_yolo_dfl_heads(d)[0]
    m = marsrt.Model(d, batch=B)
    shots = [lcg_frame(0x5EED0000 + k, m.input_view(0).shape[1]) for k in range(8)]
    for f in range(B):
        m.input_view(0)[f] = shots[f % 8]
    m.upload()
    m.run_device()
    o = marsrt.seg_opts(coefs, pr, max_per_frame=M)
    ms = []
    for k in range(a.warmup + a.runs):
        m.detect_seg_device(o)
        t = float(L.mars_hip_mask_ms(m.p))
        if k >= a.warmup:
            ms.append(t)
    dets = m.detect_results()
    recs, words, pw = m.mask_results()
    nm, ph = tensors[pr]["shape"][3], tensors[pr]["shape"][1]
    taken = int((recs["det"] >= 0).sum())
    algo_b = B * nm * ph * pw + taken * nm + recs.nbytes + words.nbytes
    med = float(np.median(ms))
    # the path the stage replaces
    t0 = time.perf_counter()
    host_dets = m.detect_dfl()
    ps = tensors[pr]["scale"]
    for f in range(B):
        P = m.read_tensor(pr, f).view(np.int8).reshape(ph, pw, nm).transpose(2, 0, 1)
        ca = [m.read_tensor(t, f).view(np.int8).reshape(-1, nm) for t in coefs]
        for i in segref.select(host_dets[f]["conf"], 0.0, M):
            b = host_dets[f][i]
            # the origin those calls do not report: guessed as the cell under the box centre on the grid whose stride suits the box size
            k = int(np.argmin([abs(max(b["w"], b["h"]) - 4 * s) for _, _, s in heads]))
            g = S // heads[k][2]
            cell = min(max(int(b["y"] / heads[k][2]), 0), g - 1) * g + min(max(int(b["x"] / heads[k][2]), 0), g - 1)
            segref.mask_array(ca[k][cell], P, (b["x"], b["y"], b["w"], b["h"]), S, S, np.float32(tensors[coefs[k]]["scale"]) * np.float32(ps))
    host_ms = (time.perf_counter() - t0) * 1e3
    out = {"tool": "tools/seg_rate.py", "model": "synthetic seg twin, width_x16 4, %dx%d" % (S, S), "batch": B, "max_per_frame": M,
           "prototypes": "%dx%dx%d int8" % (nm, ph, pw), "runs": a.runs, "warmup": a.warmup,
           "detections_kept": int(sum(len(x) for x in dets)), "masks_taken": taken,
           "mask_stage_device_ms_median": round(med, 4), "mask_stage_device_ms_min_max": [round(min(ms), 4), round(max(ms), 4)],
           "algorithmic_bytes": int(algo_b), "implied_GBs": round(algo_b / (med * 1e-3) / 1e9, 1),
           "fraction_of_8TBs_roof": round(algo_b / (med * 1e-3) / 1e9 / HBM_ROOF_GBS, 4),
           "host_path_wall_ms": round(host_ms, 1),
           "host_path": "detect_dfl + read_tensor of the prototype and coefficient tensors of every frame + numpy masks (origin by a centre-cell search)",
           "host_path_over_mask_stage": round(host_ms / med, 1)}
    m.close()
    print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
