#!/usr/bin/env python3
"""Cost of the appearance term in the track tail (mars_yolo_track_lists_app: csrc/hip/track_app.hip) against the plain call
(mars_yolo_track_lists: csrc/hip/track.hip) on the same lists.

The kernels run on streams no caller can put events on, so the tool's own figures are host wall time of the list forms -- upload, the
launches, download of the ids, the waits -- on an otherwise idle device, median of --runs after --warmup.  The scene: 256 streams x 1 step,
16 boxes per frame on a grid, the same in every frame, every box with an embedding of its own direction; the trackers already hold the
scene's tracks, so every box matches its track and, in the appearance call, 16 x 16 cosines per stream are computed and read.  Per C in
(64, 512):
  app         mars_yolo_track_lists_app on a tracker with a plane: upload of the 4096 vectors, the quantise launch, the tracking launch
  app_smooth  the same with MARS_TRACK_APP_SMOOTH (every matched slot blends and re-quantises its row)
  plane       mars_yolo_track_lists on the tracker with a plane (the appearance kernel with nothing to compare)
and once:
  plain       mars_yolo_track_lists on a tracker without a plane: the kernel of the commit before this feature
  empty       the plain call with every count zero: the copies and a launch that finds nothing to do
DEVICE time of the kernels alone comes from a profiler: run one case at a time under `rocprofv3 --kernel-trace --stats --output-format
csv -d DIR -o NAME -- python tools/track_app_rate.py --case plain` (then app64, app512: each runs its warm-up and timed calls and nothing
else), and then the whole tool with --kernel-stats plain=FILE --kernel-stats app64=FILE ...: the kernels' durations in those
*_kernel_stats.csv files are added to the line under "kernel_us" (one call in every profiled run is the births that set the scene up).

One JSON line; kept in profiles/track_app.json.

usage: tools/track_app_rate.py [--runs 30] [--warmup 5] [--case all|plain|app64|app512] [--kernel-stats CASE=FILE.csv ...]
"""
import argparse
import csv
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
from test_track_cpu import box, frames  # noqa: E402

STREAMS, BOXES, MAX_DET = 256, 16, 16
KERNELS = ("track_kernel", "track_app_kernel", "ta_quantise_kernel")


def scene():
    rows = [box(40.0 * (k % 4), y=40.0 * (k // 4), w=30.0, h=30.0, cls=k % 3) for k in range(BOXES)]
    return frames(*([rows] * STREAMS), max_det=MAX_DET)


def wall_ms(fn, runs, warmup):
    t = []
    for k in range(warmup + runs):
        marsrt.lib().mars_hip_sync()
        t0 = time.perf_counter()
        fn()
        if k >= warmup:
            t.append((time.perf_counter() - t0) * 1e3)
    return dict(median=round(float(np.median(t)), 4), min=round(min(t), 4), max=round(max(t), 4))


def kernel_stats(path):
    out = {}
    with open(path, newline="") as fh:
        for row in csv.DictReader(fh):
            for k in KERNELS:
                if row.get("Name", "").split("(")[0].split()[-1:] == [k]:
                    out[k] = dict(calls=int(row["Calls"]), avg_us=round(float(row["AverageNs"]) / 1e3, 2), min_us=round(float(row["MinNs"]) / 1e3, 2),
                                  max_us=round(float(row["MaxNs"]) / 1e3, 2))
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--runs", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--case", default="all", choices=["all", "plain", "app64", "app512"])
    ap.add_argument("--kernel-stats", action="append", default=[])
    a = ap.parse_args()
    marsrt.nna_init()
    d, n = scene()
    o = marsrt.track_opts()
    out = {"tool": "tools/track_app_rate.py", "runs": a.runs, "warmup": a.warmup, "streams": STREAMS, "steps": 1, "boxes_per_frame": BOXES,
           "timing": "host wall ms of the list forms (copies and waits included)", "cases": []}
    if a.case in ("all", "plain"):
        plain = marsrt.Tracker(STREAMS)
        marsrt.track_lists(plain, d, n, o)
        out["plain_no_plane_wall_ms"] = wall_ms(lambda: marsrt.track_lists(plain, d, n, o), a.runs, a.warmup)
        if a.case == "all":
            out["empty_lists_wall_ms"] = wall_ms(lambda: marsrt.track_lists(plain, d, n * 0, o), a.runs, a.warmup)
        plain.close()
    for c in (64, 512):
        if a.case not in ("all", "app%d" % c):
            continue
        base = (lcg_frame(0x7A9E0000 + c, STREAMS * BOXES * c * 4).view(np.int32) >> 14).reshape(STREAMS * BOXES, c)
        index = np.arange(STREAMS * MAX_DET, dtype=np.int32).reshape(STREAMS, MAX_DET)
        res = dict(channels=c, vectors=int(base.shape[0]))
        for name, smooth in (("app", False), ("app_smooth", True))[:2 if a.case == "all" else 1]:
            trk = marsrt.Tracker(STREAMS, c)
            app = marsrt.track_app_opts(smooth=smooth)
            marsrt.track_lists_app(trk, d, n, base, index, o, app)
            res[name + "_wall_ms"] = wall_ms(lambda: marsrt.track_lists_app(trk, d, n, base, index, o, app), a.runs, a.warmup)
            live = sum(int((trk.read_embeddings(b)[1] > 0).sum()) for b in (0, STREAMS - 1))
            assert live == 2 * BOXES, live  # every track holds an embedding: the cosines were computed
            if not smooth and a.case == "all":
                res["plane_wall_ms"] = wall_ms(lambda: marsrt.track_lists(trk, d, n, o), a.runs, a.warmup)
            trk.close()
        out["cases"].append(res)
    if a.kernel_stats:
        out["kernel_us"] = {x.split("=", 1)[0]: kernel_stats(x.split("=", 1)[1]) for x in a.kernel_stats}
    print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
