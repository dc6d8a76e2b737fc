#!/usr/bin/env python3
"""The camera leg of bench.py (--io camera) fed RGB frames and fed NV12 frames made from the same frames, in one process: yolov5s int8 twin at
640 x 640, batch 256, 1280 x 720 frames from pinned host memory, the four staging slots filled once, then the steady-state wait / submit loop
with three batches in flight.  The two formats alternate, --legs times each; the medians, every leg's rate and the spread are printed as one
JSON line, with the medians of mars_hip_pipe_camera_ms (device time of the front-end of one batch).

usage: tools/camera_rate.py [--batch 256] [--legs 5] [--batches 12] [--hw 640] [--width 8]
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
from conftest import lcg_frame  # noqa: E402

CW, CH = 1280, 720


def rgb_to_nv12(rgb):
    """BT.601 limited range, chroma of a 2 x 2 block from its mean colour: what a camera ISP would have delivered for this picture"""
    p = rgb.astype(np.int32)
    r, g, b = p[..., 0], p[..., 1], p[..., 2]
    y = ((66 * r + 129 * g + 25 * b + 128) >> 8) + 16
    m = (p[0::2, 0::2] + p[0::2, 1::2] + p[1::2, 0::2] + p[1::2, 1::2] + 2) >> 2
    r, g, b = m[..., 0], m[..., 1], m[..., 2]
    u = ((-38 * r - 74 * g + 112 * b + 128) >> 8) + 128
    v = ((112 * r - 94 * g - 18 * b + 128) >> 8) + 128
    return np.concatenate([np.clip(y, 0, 255).astype(np.uint8).reshape(-1), np.clip(np.stack([u, v], -1), 0, 255).astype(np.uint8).reshape(-1)])


def leg(model, outputs, shots, nv12, batch, nb):
    """bench.py's camera loop: -> (images/s, median front-end ms, detections of the last batch)"""
    kw = dict(camera_format=marsrt.CAMERA_NV12) if nv12 else {}
    model.pipe_open(download_outputs=False, detect=True, det_outputs=outputs, thresh=0.45, camera=(CW, CH), **kw)
    for k in range(4):  # fill the four staging slots once (a camera would DMA into them), untimed
        v = model.pipe_input_view(0)
        for f in range(batch):
            v[f] = shots[(f + k) % len(shots)]
        model.pipe_submit()
        if k >= 2:
            model.pipe_wait(copy=False)
    for _ in range(2):
        model.pipe_wait(copy=False)
    pre_ms = []
    marsrt.lib().mars_hip_sync()
    t1 = time.perf_counter()
    for k in range(3):
        model.pipe_submit()
    for _ in range(nb):
        model.pipe_wait(copy=False)
        pre_ms.append(float(marsrt.lib().mars_hip_pipe_camera_ms(model.p)))
        model.pipe_submit()
    kept = 0
    for _ in range(3):
        _, (d, c) = model.pipe_wait(copy=False)
        kept = int(c.sum())
    dt = time.perf_counter() - t1
    model.pipe_close()
    return (nb + 3) * batch / dt, float(np.median([x for x in pre_ms if x > 0])), kept


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=256)
    ap.add_argument("--legs", type=int, default=5)
    ap.add_argument("--batches", type=int, default=12, help="batches of the steady-state loop (bench.py: 12; + 3 to fill and drain)")
    ap.add_argument("--hw", type=int, default=640)
    ap.add_argument("--width", type=int, default=8)
    a = ap.parse_args()
    marsrt.nna_init()
    d = marsrt.synth_model(width_x16=a.width, input_hw=a.hw, seed=1)
    outputs = tuple(range(len(marsfile.parse(d)[0]["outputs"])))
    model = marsrt.Model(d, batch=a.batch)
    rgb = [lcg_frame(0xCA3E0000 + k, CW * CH * 3) for k in range(8)]
    nv12 = [rgb_to_nv12(x.reshape(CH, CW, 3)) for x in rgb]
    res = {"rgb": [], "nv12": []}
    for fmt in ("rgb", "nv12"):  # warm-up: one leg each (code objects, tables, allocations)
        leg(model, outputs, nv12 if fmt == "nv12" else rgb, fmt == "nv12", a.batch, 3)
    for _ in range(a.legs):  # alternating, so that drift of the host or the link hits both alike
        for fmt in ("rgb", "nv12"):
            res[fmt].append(leg(model, outputs, nv12 if fmt == "nv12" else rgb, fmt == "nv12", a.batch, a.batches))
    model.close()
    out = {"tool": "tools/camera_rate.py", "model": "synthetic yolov5 int8 twin, width_x16=%d, %dx%d" % (a.width, a.hw, a.hw), "batch": a.batch,
           "frame": "%dx%d" % (CW, CH), "batches_per_leg": a.batches + 3, "legs": a.legs}
    for fmt in ("rgb", "nv12"):
        rates = [r[0] for r in res[fmt]]
        med = float(np.median(rates))
        out[fmt] = {"host_to_device_bytes_per_batch": a.batch * (CW * CH * 3 // (2 if fmt == "nv12" else 1)),
                    "images_per_s_median": round(med, 1), "images_per_s_legs": [round(x, 1) for x in rates],
                    "spread_pct": round(100 * (max(rates) - min(rates)) / med, 2),
                    "camera_ms_median": round(float(np.median([r[1] for r in res[fmt]])), 4), "camera_ms_legs": [round(r[1], 4) for r in res[fmt]],
                    "detections_last_batch": res[fmt][-1][2]}
    out["nv12_over_rgb"] = round(out["nv12"]["images_per_s_median"] / out["rgb"]["images_per_s_median"], 4)
    print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
