#!/usr/bin/env python3
"""Device time of the ROI crops (mars_hip_crop_detections_device: the select launches + the crop kernel) by HIP events on the library's
stream: 256 frames of 1280 x 720 in HBM, RGB and NV12, a 320 x 320 anchor twin's detections with boxes in frame pixels, four boxes per
frame = 1 024 crops into the shipped tiny_160_int8.mars at batch 1 024.  Median of --runs calls after --warmup.  Beside it: the bytes-moved
floor (the source bytes the kept rectangles' taps touch + the bytes written, at the 8 TB/s peak and the 6.3 TB/s achievable rate bench.py
uses) and the letterbox front-end's time on the same frames (the only comparable kernel in the tree).  One JSON line; kept in
profiles/roi_crop.json.  For the split between the select and the crop kernel run it under `rocprofv3 --kernel-trace --stats -- python ...`.

usage: tools/roi_rate.py [--frames 256] [--slots 1024] [--runs 30] [--warmup 5]
"""
import argparse
import ctypes as C
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "thingino-accel_amd"))

import marsrt  # noqa: E402
from conftest import lcg_frame  # noqa: E402
from test_roi_cpu import roi_axis_np  # noqa: E402

CW, CH = 1280, 720


class Events:
    """elapsed device time between two points of the library's stream"""

    def __init__(self):
        self.hip = C.CDLL("libamdhip64.so", mode=os.RTLD_GLOBAL)
        self.stream = C.c_void_p(marsrt.lib().mars_hip_stream())
        self.e0, self.e1 = C.c_void_p(), C.c_void_p()
        assert self.hip.hipEventCreate(C.byref(self.e0)) == 0 and self.hip.hipEventCreate(C.byref(self.e1)) == 0

    def time(self, fn):
        assert self.hip.hipEventRecord(self.e0, self.stream) == 0
        fn()
        assert self.hip.hipEventRecord(self.e1, self.stream) == 0
        assert self.hip.hipEventSynchronize(self.e1) == 0
        ms = C.c_float()
        assert self.hip.hipEventElapsedTime(C.byref(ms), self.e0, self.e1) == 0
        return ms.value

    def median(self, fn, runs, warmup):
        for _ in range(warmup):
            self.time(fn)
        t = [self.time(fn) for _ in range(runs)]
        return float(np.median(t)), float(min(t)), float(max(t))


def touched_bytes(rois, nv12, tw, th):
    """source bytes the taps of the kept rectangles read: the rows j0, j1 of every output row, cw pixels each (NV12: + half a chroma row per row)"""
    total = 0
    for r in rois:
        cw, ch = int(r["x1"] - r["x0"]), int(r["y1"] - r["y0"])
        j0, j1, _ = roi_axis_np(ch, th)
        rows = len(np.union1d(j0, j1))
        total += rows * cw * 3 // 2 if nv12 else rows * cw * 3
    return total


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=256)
    ap.add_argument("--slots", type=int, default=1024)
    ap.add_argument("--runs", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    a = ap.parse_args()
    marsrt.nna_init()
    ev = Events()
    det = marsrt.Model(marsrt.synth_model(width_x16=4, input_hw=320, seed=3), batch=a.frames)
    with open(os.path.join(ROOT, "tests", "golden", "models", "tiny_160_int8.mars"), "rb") as fh:
        dst = marsrt.Model(fh.read(), batch=a.slots)
    per = a.slots // a.frames
    out = {"tool": "tools/roi_rate.py", "frames": a.frames, "frame": "%dx%d" % (CW, CH), "crops": a.slots, "target": "160x160 planar int8",
           "boxes_per_frame": per, "runs": a.runs, "warmup": a.warmup, "written_bytes": a.slots * 160 * 160 * 3}
    for fmt in ("rgb", "nv12"):
        nv12 = fmt == "nv12"
        fb = CW * CH * 3 // 2 if nv12 else CW * CH * 3
        shots = [lcg_frame(0xCA3E0000 + k, fb) for k in range(8)]
        buf = marsrt.DeviceBuffer(np.stack([shots[f % 8] for f in range(a.frames)]))
        pre = (lambda: det.preprocess_nv12_device(buf.ptr, CW, CH, a.frames)) if nv12 else (lambda: det.preprocess_device(buf.ptr, CW, CH, a.frames))
        lb = ev.median(pre, a.runs, a.warmup)
        det.run_device(sync=False)
        det.detect_heads_device(conf=0.25, src=(CW, CH))
        n_det = sum(len(x) for x in det.detect_results())
        o = marsrt.roi_opts(CW, CH, fmt=marsrt.CAMERA_NV12 if nv12 else marsrt.CAMERA_RGB, max_per_frame=per)
        t = ev.median(lambda: dst.crop_detections(det, buf.ptr, o, device=True), a.runs, a.warmup)
        rois, dropped = dst.roi_results()
        src_b = touched_bytes(rois, nv12, 160, 160)
        moved = src_b + out["written_bytes"]
        out[fmt] = {"detections": n_det, "kept": len(rois), "dropped": dropped,
                    "mean_box": [round(float(np.mean(rois["x1"] - rois["x0"])), 1), round(float(np.mean(rois["y1"] - rois["y0"])), 1)],
                    "select_plus_crop_ms_median": round(t[0], 4), "select_plus_crop_ms_min_max": [round(t[1], 4), round(t[2], 4)],
                    "touched_source_bytes": src_b, "floor_ms_at_8TBs": round(moved / 8e12 * 1e3, 5), "floor_ms_at_6.3TBs": round(moved / 6.3e12 * 1e3, 5),
                    "fraction_of_floor_6.3TBs": round(moved / 6.3e12 * 1e3 / t[0], 4), "effective_GBs": round(moved / (t[0] * 1e-3) / 1e9, 1),
                    "letterbox_320_ms_median": round(lb[0], 4), "letterbox_source_bytes": fb * a.frames}
        buf.free()
    det.close()
    dst.close()
    print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
