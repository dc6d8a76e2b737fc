#!/usr/bin/env python3
"""Device time of the area-averaging crop kernel (roi_area_crop_kernel) beside the bilinear one (roi_crop_kernel), by HIP events on the
library's stream (median of --runs launches after --warmup), on two workloads:
  crops   the workload of profiles/roi_crop.json and profiles/rot_crop.json: the 1 024 seeded boxes of tools/rot_crop_rate.py out of 256 NV12
          frames of 1280 x 720 into 160 x 160 (planar int8); mhip_roi_rects + mhip_roi_crop with area = 0 (the yardstick: run it with --tree
          on a built checkout of the parent commit too) and with area = 1;
  tiles   16 NV12 frames of 1920 x 1080 as the 9 tiles of INTEGRATION.md (the 8 tiles of mars_tile_grid(1920, 1080, 640, 640, 128, 128) and the
          whole frame), batch 144 into 640 x 640 with keep-aspect; mhip_roi_crop alone over a ROI table written by the host, area = 0 and 1.
Beside each time stands its byte floor: the source bytes of every rectangle (NV12: 1.5 bytes a pixel) plus the bytes written, at 8 TB/s.
The kernels are launched through the library's internal launch record (csrc/mhip.h, mhip_roi_t, restated in tools/rot_crop_rate.py); a
library without the `area` field reads a prefix of it.  One JSON line; kept in profiles/area_crop.json.

usage: tools/area_crop_rate.py [--runs 30] [--warmup 5] [--tree PATH] [--unflagged-only]
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
sys.path.insert(0, os.path.join(ROOT, "tools"))

import marsrt  # noqa: E402
from conftest import lcg_frame  # noqa: E402
from roi_rate import Events  # noqa: E402
from rot_crop_rate import RoiLaunch, seeded_boxes  # noqa: E402

TBS = 8e12


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--runs", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--tree", help="another built checkout (the parent commit's, for the yardstick)")
    ap.add_argument("--unflagged-only", action="store_true", help="area = 0 only (a library from before the flag knows nothing else)")
    a = ap.parse_args()
    marsrt.nna_init()
    L = marsrt.lib()
    ev = Events()
    res = {"tool": "tools/area_crop_rate.py", "library": "another checkout's" if a.tree else "this tree's", "runs": a.runs, "warmup": a.warmup}
    modes = (0,) if a.unflagged_only else (0, 1)

    def workload(name, cw, ch, n_frames, tw, th, keep, table, boxes, fo):
        """table: ROI records written by the host (the crop launch alone is timed); else boxes + fo through mhip_roi_rects"""
        fb = cw * ch * 3 // 2
        n = len(table) if table is not None else len(boxes)
        shots = [lcg_frame(0xCA3E0000 + k, fb) for k in range(8)]
        frames = marsrt.DeviceBuffer(np.stack([shots[f % 8] for f in range(n_frames)]))
        out = marsrt.DeviceBuffer(np.zeros(n * tw * th * 3, dtype=np.uint8))
        rois = marsrt.DeviceBuffer(table.view(np.uint8) if table is not None else np.zeros(n * 24, dtype=np.uint8))
        cnt = np.zeros(4, dtype=np.int32)
        cnt[0] = n
        n_out = marsrt.DeviceBuffer(cnt.view(np.uint8))
        bx = marsrt.DeviceBuffer(boxes.view(np.uint8)) if boxes is not None else None
        fod = marsrt.DeviceBuffer(fo.view(np.uint8)) if fo is not None else None
        p = RoiLaunch()
        p.frames, p.frame_stride, p.n_frames, p.w, p.h, p.fmt = frames.ptr, fb, n_frames, cw, ch, 1
        if bx:
            p.boxes, p.frame_of_box, p.n_boxes = bx.ptr, fod.ptr, n
        p.expand, p.min_size, p.keep_aspect = 1.0, 1 if table is not None else 2, keep
        p.out, p.out_stride, p.slots, p.tw, p.th, p.nhwc = out.ptr, tw * th * 3, n, tw, th, 0
        p.rois, p.n_out = rois.ptr, n_out.ptr
        w = {"frames": n_frames, "frame": "%dx%d nv12" % (cw, ch), "crops": n, "target": "%dx%d planar int8%s" % (tw, th, ", keep-aspect" if keep else ""),
             "timed": "mhip_roi_crop" if table is not None else "mhip_roi_rects + mhip_roi_crop", "written_bytes": n * tw * th * 3}
        for area in modes:
            p.area = area

            def go():
                assert (table is not None or L.mhip_roi_rects(C.byref(p)) == 0) and L.mhip_roi_crop(C.byref(p)) == 0
            t = ev.median(go, a.runs, a.warmup)
            r = np.zeros(n, dtype=marsrt.ROI_DTYPE)
            assert ev.hip.hipMemcpy(C.c_void_p(r.ctypes.data), C.c_void_p(rois.ptr), C.c_size_t(n * 24), 2) == 0  # device to host
            rw, rh = (r["x1"] - r["x0"]).astype(np.int64), (r["y1"] - r["y0"]).astype(np.int64)
            src = int((rw * rh * 3 // 2).sum())
            w["area" if area else "unflagged"] = {"ms_median": round(t[0], 4), "ms_min_max": [round(t[1], 4), round(t[2], 4)], "crops_cut": int((rw > 0).sum())}
            w["mean_rect"] = [round(float(rw.mean()), 1), round(float(rh.mean()), 1)]
            w["source_bytes"] = src
            w["floor_ms_at_8TBs"] = round((src + n * tw * th * 3) / TBS * 1e3, 4)
        if "area" in w:
            w["area"]["over_unflagged"] = round(w["area"]["ms_median"] / w["unflagged"]["ms_median"], 3)
            w["area"]["over_floor"] = round(w["area"]["ms_median"] / w["floor_ms_at_8TBs"], 2)
        res[name] = w
        for d in (frames, out, rois, n_out, bx, fod):
            if d:
                d.free()

    # crops: the boxes of tools/rot_crop_rate.py
    x, y, bw, bh, _ = seeded_boxes(256, 4)
    det = np.zeros(1024, dtype=marsrt.DET_DTYPE)
    det["x"], det["y"], det["w"], det["h"], det["conf"] = x, y, bw, bh, 0.9
    workload("crops", 1280, 720, 256, 160, 160, 0, None, det, np.repeat(np.arange(256, dtype=np.int32), 4))
    # tiles: the table of INTEGRATION.md, "Tiled inference"
    grid = [tuple(t) for t in marsrt.tile_grid(1920, 1080, 640, 640, 128, 128)] + [(0, 0, 1920, 1080)]
    assert len(grid) == 9
    table = np.zeros(16 * 9, dtype=marsrt.ROI_DTYPE)
    for c in range(16):
        for t, (x0, y0, x1, y1) in enumerate(grid):
            table[c * 9 + t] = (c, -1, x0, y0, x1, y1)
    workload("tiles", 1920, 1080, 16, 640, 640, 1, table, None, None)
    print(json.dumps(res), flush=True)


if __name__ == "__main__":
    main()
