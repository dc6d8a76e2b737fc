#!/usr/bin/env python3
"""Time of the frame-pixel mask stage (mars_hip_detect_seg_native_device: the selection launch + the mask launch of csrc/hip/seg_native.hip,
behind the DFL tail) on the 640 x 640 seg twin fed from 1280 x 720 frames: masks on the 1280 x 720 grid, max_per_frame 16, batch 256.  The
figure is DEVICE time between two events the library records around the stage on the auxiliary stream (mars_hip_mask_native_ms), median of
--runs after --warmup on an otherwise idle device.  Beside it: the bytes the stage must move -- every mask word and record written once, the
prototypes read once per frame, the selected cells' coefficient rows, the tap tables -- and the fraction of the 8 TB/s HBM roof that this
time implies.  The parent of this stage has no counterpart to compare against: the traffic is the yardstick.  One JSON line; kept in
profiles/mask_native.json.

usage: tools/mask_native_rate.py [--batch 256] [--max-per-frame 16] [--src 1280x720] [--runs 20] [--warmup 3]
"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "thingino-accel_amd"))

import marsfile  # noqa: E402
import marsrt  # noqa: E402
from conftest import lcg_frame  # noqa: E402

HBM_ROOF_GBS = 8000.0


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=256)
    ap.add_argument("--max-per-frame", type=int, default=16)
    ap.add_argument("--src", default="1280x720")
    ap.add_argument("--runs", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--input", type=int, default=640)
    a = ap.parse_args()
    W, H = (int(v) for v in a.src.split("x"))
    marsrt.nna_init()
    L = marsrt.lib()
    S, B, M = a.input, a.batch, a.max_per_frame
    d = marsrt.synth_model(width_x16=4, input_hw=S, seed=1, head="seg")
    hdr, tensors, _ = marsfile.parse(d)
    coefs, pr = marsrt.seg_twin_tensors(d)
    m = marsrt.Model(d, batch=B)
    shots = [lcg_frame(0x5EED0000 + k, m.input_view(0).shape[1]) for k in range(8)]
    for f in range(B):
        m.input_view(0)[f] = shots[f % 8]
    m.upload()
    m.run_device()
    o = marsrt.seg_opts(coefs, pr, max_per_frame=M)
    ms = []
    for k in range(a.warmup + a.runs):
        m.detect_seg_native_device(o, None, src=(W, H))
        t = float(L.mars_hip_mask_native_ms(m.p))
        if k >= a.warmup:
            ms.append(t)
    dets = m.detect_results()
    recs = np.zeros((B, M), dtype=marsrt.MASK_DTYPE)  # the words stay on the device: half a gigabyte at the default sizes
    rc = L.mars_hip_mask_native_results(m.p, recs.ctypes.data, None, None, None, None)
    if rc != marsrt.MARS_OK:
        raise marsrt.MarsError(rc, "mars_hip_mask_native_results")
    nm, ph, pw = tensors[pr]["shape"][3], tensors[pr]["shape"][1], tensors[pr]["shape"][2]
    pitch = (W + 31) // 32
    taken = int((recs["det"] >= 0).sum())
    word_b = B * M * H * pitch * 4
    proto_b = B * nm * ph * pw
    algo_b = word_b + proto_b + taken * nm + recs.nbytes + 3 * (W + H) * 4
    box_px = int(((recs["x1"] - recs["x0"]).clip(0) * (recs["y1"] - recs["y0"]).clip(0)).sum())
    med = float(np.median(ms))
    out = {"tool": "tools/mask_native_rate.py", "model": "synthetic seg twin, width_x16 4, %dx%d" % (S, S), "frames": "%dx%d" % (W, H),
           "output_grid": "%dx%d" % (W, H), "batch": B, "max_per_frame": M, "prototypes": "%dx%dx%d int8" % (nm, ph, pw),
           "runs": a.runs, "warmup": a.warmup, "detections_kept": int(sum(len(x) for x in dets)), "masks_taken": taken,
           "rectangle_pixels": box_px, "mask_pixels_set": int(recs["area"].sum()),
           "mask_stage_device_ms_median": round(med, 4), "mask_stage_device_ms_min_max": [round(min(ms), 4), round(max(ms), 4)],
           "bytes_words_written": int(word_b), "bytes_prototypes_read": int(proto_b), "algorithmic_bytes": int(algo_b),
           "implied_GBs": round(algo_b / (med * 1e-3) / 1e9, 1), "fraction_of_8TBs_roof": round(algo_b / (med * 1e-3) / 1e9 / HBM_ROOF_GBS, 4),
           "note": "measured once, on one machine"}
    m.close()
    print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
