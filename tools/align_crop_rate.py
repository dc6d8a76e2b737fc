#!/usr/bin/env python3
"""Device time of the aligned crop ("Aligned crops" in include/mars_hip.h) beside the rotated one it shares its sampler with: 1 024 crops of
112 x 112 (planar int8) out of 256 NV12 frames of 1280 x 720 in HBM, four per frame.  The seeded boxes are those of tools/rot_crop_rate.py
(profiles/rot_crop.json): every box gives an oriented box of its centre, its width as both sides and its angle, and a keypoint set -- the
5-point face template under the similarity with that centre, scale width / 112 and angle.  So both paths sample the same source pixels:
  aligned   fit  = mhip_roi_align_rects (one fit per keypoint set: the same device function the device chain's select launch runs),
            crop = mhip_roi_align_crop  (roi_rot_crop_kernel reading its six integers from the fit table);
  rotated   rects = mhip_roi_rot_rects, crop = mhip_roi_rot_crop (the same kernel reading the obb record and its (cos, sin) pair).
Every launch is timed on its own by HIP events on the library's stream (median of --runs launches after --warmup); the whole measurement is
repeated --repeats times and the spread of the repeats' medians is reported next to them.  With --tree PATH the rotated half runs on the
library of another built checkout (the parent commit's): its sampler is the yardstick the new instantiation must have cost nothing.
The kernels are launched through the library's internal launch record (csrc/mhip.h, mhip_roi_t, restated below).  One JSON line; kept in
profiles/align_crop.json.

usage: tools/align_crop_rate.py [--frames 256] [--per-frame 4] [--runs 30] [--warmup 5] [--repeats 5] [--tree PATH]
"""
import argparse
import ctypes as C
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TREE = os.path.abspath(sys.argv[sys.argv.index("--tree") + 1]) if "--tree" in sys.argv[1:-1] else ROOT
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "tools"))
sys.path.insert(0, os.path.join(TREE, "thingino-accel_amd"))

import marsrt  # noqa: E402
from conftest import lcg_frame  # noqa: E402
from roi_rate import Events  # noqa: E402
from rot_crop_rate import CH, CW, RoiLaunch, seeded_boxes  # noqa: E402

TW = TH = 112
FACE5 = [(38.2946, 51.6963), (73.5318, 51.5014), (56.0252, 71.7366), (41.5493, 92.3655), (70.7299, 92.2041)]


class AlignLaunch(C.Structure):  # mhip_roi_t with the fields of the align calls behind those of RoiLaunch
    _fields_ = RoiLaunch._fields_ + [("fits", C.c_void_p), ("pose_recs", C.c_void_p), ("pose_kpts", C.c_void_p), ("pose_max", C.c_int),
                                     ("num_kpt", C.c_int), ("use", C.c_uint), ("min_vis", C.c_float), ("tmpl", (C.c_float * 2) * 32)]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=256)
    ap.add_argument("--per-frame", type=int, default=4)
    ap.add_argument("--runs", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--tree", help="another built checkout (the parent commit's): the rotated half only")
    a = ap.parse_args()
    marsrt.nna_init()
    L = marsrt.lib()
    ev = Events()
    n = a.frames * a.per_frame
    x, y, w, _h, ang = seeded_boxes(a.frames, a.per_frame)
    fb = CW * CH * 3 // 2
    shots = [lcg_frame(0xCA3E0000 + k, fb) for k in range(8)]
    frames = marsrt.DeviceBuffer(np.stack([shots[f % 8] for f in range(a.frames)]))
    fo = marsrt.DeviceBuffer(np.repeat(np.arange(a.frames, dtype=np.int32), a.per_frame).view(np.uint8))
    out = marsrt.DeviceBuffer(np.zeros(n * TW * TH * 3, dtype=np.uint8))
    rois = marsrt.DeviceBuffer(np.zeros(n * 24, dtype=np.uint8))
    fits = marsrt.DeviceBuffer(np.zeros(n * 32, dtype=np.uint8))
    n_out = marsrt.DeviceBuffer(np.zeros(16, dtype=np.uint8))
    res = {"tool": "tools/align_crop_rate.py", "library": "another checkout's" if a.tree else "this tree's", "frames": a.frames,
           "frame": "%dx%d nv12" % (CW, CH), "crops": n, "target": "%dx%d planar int8" % (TW, TH), "runs": a.runs, "warmup": a.warmup,
           "repeats": a.repeats, "mean_side": round(float(w.mean()), 1), "written_bytes": n * TW * TH * 3}

    def record(kind, boxes_dev, csn_dev=None):
        p = kind()
        p.frames, p.frame_stride, p.n_frames, p.w, p.h, p.fmt = frames.ptr, fb, a.frames, CW, CH, 1
        p.boxes, p.frame_of_box, p.n_boxes = boxes_dev.ptr, fo.ptr, n
        p.expand, p.min_size = 1.0, 2
        p.out, p.out_stride, p.slots, p.tw, p.th, p.nhwc = out.ptr, TW * TH * 3, n, TW, TH, 0
        p.rois, p.n_out, p.csn = rois.ptr, n_out.ptr, csn_dev.ptr if csn_dev else None
        return p

    def timed(name, first, crop, p, first_name):
        def launch(f):
            def go():
                assert f(C.byref(p)) == 0
            return go
        reps = {first_name: [], "crop": []}
        for _ in range(a.repeats):
            reps[first_name].append(ev.median(launch(first), a.runs, a.warmup)[0])
            reps["crop"].append(ev.median(launch(crop), a.runs, a.warmup)[0])
        r = np.zeros(n, dtype=marsrt.ROI_DTYPE)
        assert ev.hip.hipMemcpy(C.c_void_p(r.ctypes.data), C.c_void_p(rois.ptr), C.c_size_t(n * 24), 2) == 0  # device to host
        res[name] = {"crops_cut": int((r["x1"] > r["x0"]).sum())}
        for k, t in reps.items():
            res[name][k + "_ms_median_of_repeats"] = round(float(np.median(t)), 4)
            res[name][k + "_ms_repeats"] = [round(v, 4) for v in t]
            res[name][k + "_ms_spread"] = round(max(t) - min(t), 4)

    b = np.zeros(n, dtype=marsrt.OBB_DTYPE)
    b["x"], b["y"], b["w"], b["h"], b["conf"], b["angle"] = x, y, w, w, 0.9, ang
    csn = np.stack([np.cos(b["angle"].astype(np.float64)), np.sin(b["angle"].astype(np.float64))], axis=1).astype(np.float32)
    bd, cd = marsrt.DeviceBuffer(b.view(np.uint8)), marsrt.DeviceBuffer(csn.view(np.uint8))
    timed("rotated", L.mhip_roi_rot_rects, L.mhip_roi_rot_crop, record(RoiLaunch, bd, cd), "rects")
    if not a.tree:
        d = np.array(FACE5) - (TW / 2, TH / 2)
        angle = b["angle"].astype(np.float64)
        c, s = (np.cos(angle) * w / TW)[:, None], (np.sin(angle) * w / TW)[:, None]
        kp = np.zeros((n, 5), dtype=marsrt.KPT_DTYPE)
        kp["x"], kp["y"], kp["v"] = x[:, None] + c * d[:, 0] - s * d[:, 1], y[:, None] + s * d[:, 0] + c * d[:, 1], 1.0
        kd = marsrt.DeviceBuffer(kp.view(np.uint8))
        p = record(AlignLaunch, kd)
        p.fits, p.num_kpt, p.use, p.min_vis = fits.ptr, 5, 31, 0.0
        for j in range(5):
            p.tmpl[j][0], p.tmpl[j][1] = FACE5[j]
        timed("aligned", L.mhip_roi_align_rects, L.mhip_roi_align_crop, p, "fit")
        res["aligned_crop_over_rotated_crop"] = round(res["aligned"]["crop_ms_median_of_repeats"] / res["rotated"]["crop_ms_median_of_repeats"], 3)
        kd.free()
    for dev in (bd, cd, frames, fo, out, rois, fits, n_out):
        dev.free()
    print(json.dumps(res), flush=True)


if __name__ == "__main__":
    main()
