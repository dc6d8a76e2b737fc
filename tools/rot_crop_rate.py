#!/usr/bin/env python3
"""Device time of the rotated crop kernel (roi_rot_crop_kernel) beside the upright one (roi_crop_kernel) on the workload of
profiles/roi_crop.json: 1 024 crops of 160 x 160 (planar int8) out of 256 NV12 frames of 1280 x 720 in HBM, four boxes per frame.  The same
seeded boxes go through three kernels, each timed by HIP events on the library's stream (median of --runs launches after --warmup):
  upright   mhip_roi_rects + mhip_roi_crop over the boxes as mars_det_t (the yardstick: run it with --tree on a built checkout of the parent
            commit too);
  rot_0     mhip_roi_rot_rects + mhip_roi_rot_crop over the same boxes as mars_obb_t at angle 0 (the same source pixels, up to the clamp);
  rot_rand  ... at angles drawn over the obb rule's interval [-pi / 4, 3 pi / 4).
The kernels are launched through the library's internal launch record (csrc/mhip.h, mhip_roi_t, restated below), because the public device
chain takes its boxes from a detector.  One JSON line; kept in profiles/rot_crop.json.

usage: tools/rot_crop_rate.py [--frames 256] [--per-frame 4] [--runs 30] [--warmup 5] [--tree PATH] [--upright-only]
"""
import argparse
import ctypes as C
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
# --tree PATH: the library and its marsrt.py of another built checkout (before the imports below: marsrt declares the prototypes of its own library)
TREE = os.path.abspath(sys.argv[sys.argv.index("--tree") + 1]) if "--tree" in sys.argv[1:-1] else ROOT
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(TREE, "thingino-accel_amd"))

import marsrt  # noqa: E402
from conftest import lcg_frame  # noqa: E402
from roi_rate import Events  # noqa: E402

CW, CH, TW, TH = 1280, 720, 160, 160


class RoiLaunch(C.Structure):  # mhip_roi_t (csrc/mhip.h); `csn` and `area` are the last fields, so a library without them reads a prefix
    _fields_ = [("frames", C.c_void_p), ("frame_stride", C.c_size_t), ("n_frames", C.c_int), ("w", C.c_int), ("h", C.c_int), ("fmt", C.c_int),
                ("nv12_flags", C.c_uint), ("dets", C.c_void_p), ("counts", C.c_void_p), ("det_cap", C.c_int),
                ("boxes", C.c_void_p), ("frame_of_box", C.c_void_p), ("n_boxes", C.c_int), ("expand", C.c_float), ("min_conf", C.c_float),
                ("min_size", C.c_int), ("cls_first", C.c_int), ("cls_count", C.c_int), ("max_per_frame", C.c_int), ("keep_aspect", C.c_int),
                ("out", C.c_void_p), ("out_stride", C.c_size_t), ("slots", C.c_int), ("tw", C.c_int), ("th", C.c_int), ("nhwc", C.c_int),
                ("rois", C.c_void_p), ("n_out", C.c_void_p), ("frame_kept", C.c_void_p), ("csn", C.c_void_p),
                ("area", C.c_int)]


def seeded_boxes(frames, per, seed=0x0B0C):
    """per boxes per frame: sides of 60 .. 320 pixels (the spread of the detections behind profiles/roi_crop.json), centres so that the upright
    box lies inside the frame; angles over [-pi / 4, 3 pi / 4)"""
    rng = np.random.default_rng(seed)
    n = frames * per
    w, h = rng.uniform(60, 220, n), rng.uniform(80, 320, n)
    x, y = rng.uniform(w / 2, CW - w / 2), rng.uniform(h / 2, CH - h / 2)
    return x, y, w, h, rng.uniform(-np.pi / 4, 3 * np.pi / 4, n)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=256)
    ap.add_argument("--per-frame", type=int, default=4)
    ap.add_argument("--runs", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--tree", help="another built checkout (the parent commit's, for the yardstick)")
    ap.add_argument("--upright-only", action="store_true")
    a = ap.parse_args()
    marsrt.nna_init()
    L = marsrt.lib()
    ev = Events()
    n = a.frames * a.per_frame
    x, y, w, h, ang = seeded_boxes(a.frames, a.per_frame)
    fb = CW * CH * 3 // 2
    shots = [lcg_frame(0xCA3E0000 + k, fb) for k in range(8)]
    frames = marsrt.DeviceBuffer(np.stack([shots[f % 8] for f in range(a.frames)]))
    fo = marsrt.DeviceBuffer(np.repeat(np.arange(a.frames, dtype=np.int32), a.per_frame).view(np.uint8))
    out = marsrt.DeviceBuffer(np.zeros(n * TW * TH * 3, dtype=np.uint8))
    rois = marsrt.DeviceBuffer(np.zeros(n * 24, dtype=np.uint8))
    n_out = marsrt.DeviceBuffer(np.zeros(16, dtype=np.uint8))
    res = {"tool": "tools/rot_crop_rate.py", "library": "another checkout's" if a.tree else "this tree's", "frames": a.frames, "frame": "%dx%d nv12" % (CW, CH), "crops": n,
           "target": "%dx%d planar int8" % (TW, TH), "runs": a.runs, "warmup": a.warmup, "mean_box": [round(float(w.mean()), 1), round(float(h.mean()), 1)],
           "written_bytes": n * TW * TH * 3}

    def record(boxes_dev, csn_dev):
        p = RoiLaunch()
        p.frames, p.frame_stride, p.n_frames, p.w, p.h, p.fmt = frames.ptr, fb, a.frames, CW, CH, 1
        p.boxes, p.frame_of_box, p.n_boxes = boxes_dev.ptr, fo.ptr, n
        p.expand, p.min_size = 1.0, 2
        p.out, p.out_stride, p.slots, p.tw, p.th, p.nhwc = out.ptr, TW * TH * 3, n, TW, TH, 0
        p.rois, p.n_out, p.csn = rois.ptr, n_out.ptr, csn_dev.ptr if csn_dev else None
        return p

    def timed(name, rects, crop, p):
        def go():
            assert rects(C.byref(p)) == 0 and crop(C.byref(p)) == 0
        t = ev.median(go, a.runs, a.warmup)
        kept = np.zeros(4, dtype=np.int32)
        assert ev.hip.hipMemcpy(C.c_void_p(kept.ctypes.data), C.c_void_p(n_out.ptr), C.c_size_t(16), 2) == 0  # device to host
        r = np.zeros(n, dtype=marsrt.ROI_DTYPE)
        assert ev.hip.hipMemcpy(C.c_void_p(r.ctypes.data), C.c_void_p(rois.ptr), C.c_size_t(n * 24), 2) == 0
        res[name] = {"rects_plus_crop_ms_median": round(t[0], 4), "rects_plus_crop_ms_min_max": [round(t[1], 4), round(t[2], 4)],
                     "crops_cut": int((r["x1"] > r["x0"]).sum()), "slots": int(kept[0])}

    det = np.zeros(n, dtype=marsrt.DET_DTYPE)
    det["x"], det["y"], det["w"], det["h"], det["conf"] = x, y, w, h, 0.9
    up = marsrt.DeviceBuffer(det.view(np.uint8))
    timed("upright", L.mhip_roi_rects, L.mhip_roi_crop, record(up, None))
    if not a.upright_only:
        for name, angles in (("rot_0", np.zeros(n)), ("rot_rand", ang)):
            b = np.zeros(n, dtype=marsrt.OBB_DTYPE)
            b["x"], b["y"], b["w"], b["h"], b["conf"], b["angle"] = x, y, w, h, 0.9, angles
            csn = np.stack([np.cos(b["angle"].astype(np.float64)), np.sin(b["angle"].astype(np.float64))], axis=1).astype(np.float32)
            bd, cd = marsrt.DeviceBuffer(b.view(np.uint8)), marsrt.DeviceBuffer(csn.view(np.uint8))
            timed(name, L.mhip_roi_rot_rects, L.mhip_roi_rot_crop, record(bd, cd))
            bd.free()
            cd.free()
        for k in ("rot_0", "rot_rand"):
            res[k]["over_upright"] = round(res[k]["rects_plus_crop_ms_median"] / res["upright"]["rects_plus_crop_ms_median"], 3)
    for d in (up, frames, fo, out, rois, n_out):
        d.free()
    print(json.dumps(res), flush=True)


if __name__ == "__main__":
    main()
