#!/usr/bin/env python3
"""Cost of the events stage (mars_hip_events_device / mars_yolo_event_lists: one launch of csrc/hip/events.hip) beside the tracker's on the
same lists.

One workload: 256 camera streams, one step per call (a batch of 256 frames), about 50 boxes per frame on seeded random walks over a
1280 x 720 plane, 4 lines and 4 zones per stream (two of the zones with a dwell).  Every batch goes through mars_yolo_track_lists and the ids
it gives, with the same lists, through mars_yolo_event_lists.  Reported per call, median (min .. max) over --runs batches after --warmup:
  events_device_ms       mars_hip_events_ms: the kernel alone, between two events on its stream;
  events_lists_wall_ms   host wall time of mars_yolo_event_lists: upload of lists and ids, the launch, download of records and counts, the waits;
  track_lists_wall_ms    host wall time of mars_yolo_track_lists on the same lists (the tracker has no device timer: tools/track_rate.py says
                         why), so the two wall times are the like-for-like pair and the device time shows what of the first is the kernel.
The totals of the run (crossings, entries, exits, dwell events) are printed beside them: the workload is not an idle one.  No target is set
for any of these figures.

One JSON line; kept in profiles/events_rate.json.

usage: tools/events_rate.py [--runs 20] [--warmup 4] [--out FILE]
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "thingino-accel_amd"))

import marsrt  # noqa: E402

W, H, S, BOXES, MAX_DET = 1280, 720, 256, 50, 64


def rules():
    lines = [(W // 2, 0, W // 2, H), (0, H // 2, W, H // 2), (0, 0, W, H), (W // 4, H, 3 * W // 4, 0)]
    zones = [([(100, 100), (500, 100), (500, 400), (100, 400)], 3),
             ([(700, 80), (1200, 80), (1200, 640), (950, 360), (700, 640), (700, 300)], 0),
             ([(400, 420), (900, 420), (650, 700)], 5),
             ([(560, 280), (640, 240), (720, 280), (760, 360), (720, 440), (640, 480), (560, 440), (520, 360)], 0)]
    return marsrt.event_rules(lines, zones)


def stats(v):
    return dict(median=round(float(np.median(v)), 4), min=round(min(v), 4), max=round(max(v), 4))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--runs", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=4)
    ap.add_argument("--out")
    a = ap.parse_args()
    marsrt.nna_init()
    rng = np.random.default_rng(0xE7E57)
    pos = np.stack([rng.uniform(0, W, (S, BOXES)), rng.uniform(0, H, (S, BOXES))], axis=-1)
    vel = rng.uniform(-40, 40, pos.shape)
    trk, ev = marsrt.Tracker(S), marsrt.Events(S)
    ev.set_rules(rules())
    topts, eopts = marsrt.track_opts(iou_thresh=0.1), marsrt.event_opts(anchor_bottom=True)
    counts = np.full(S, BOXES, dtype=np.int32)
    dev, ewall, twall = [], [], []
    L = marsrt.lib()
    for k in range(a.warmup + a.runs):
        pos += vel
        for ax, hi in ((0, W), (1, H)):  # bounce off the plane's edges
            out = (pos[..., ax] < 0) | (pos[..., ax] > hi)
            vel[..., ax][out] *= -1
        d = np.zeros((S, MAX_DET), dtype=marsrt.DET_DTYPE)
        d["x"][:, :BOXES], d["y"][:, :BOXES] = pos[..., 0], pos[..., 1]
        d["w"][:, :BOXES], d["h"][:, :BOXES], d["conf"][:, :BOXES] = 120.0, 200.0, 0.9
        L.mars_hip_sync()
        t0 = time.perf_counter()
        tracks = marsrt.track_lists(trk, d, counts, topts)
        t1 = time.perf_counter()
        rec, lc, zc = marsrt.event_lists(ev, d, tracks, counts, eopts)
        t2 = time.perf_counter()
        if k >= a.warmup:
            twall.append((t1 - t0) * 1e3)
            ewall.append((t2 - t1) * 1e3)
            dev.append(ev.ms())
    tot = np.zeros(6, dtype=np.int64)
    cnt = np.zeros(5, dtype=np.int64)
    used = 0
    for b in range(S):
        lt, zt, c, u, _ = ev.read(b)
        tot += [lt[:, 0].sum(), lt[:, 1].sum(), zt[:, 0].sum(), zt[:, 1].sum(), zt[:, 2].sum(), zt[:, 3].sum()]
        cnt += c
        used += u
    res = {"tool": "tools/events_rate.py", "streams": S, "steps_per_call": 1, "boxes_per_frame": BOXES, "max_det": MAX_DET, "lines": 4, "zones": 4,
           "calls": a.warmup + a.runs, "runs": a.runs, "warmup": a.warmup,
           "tracked_per_frame_last_call": round(float((tracks["id"] >= 1).sum()) / S, 1),
           "events_device_ms": stats(dev), "events_lists_wall_ms": stats(ewall), "track_lists_wall_ms": stats(twall),
           "totals": dict(zip(("lines_in", "lines_out", "entered", "exited", "dwelled", "lost"), (int(v) for v in tot))),
           "counters": dict(zip(("first", "expired", "overflow", "dropped", "duplicates"), (int(v) for v in cnt))), "used_slots": used}
    ev.close()
    trk.close()
    line = json.dumps(res)
    print(line, flush=True)
    if a.out:
        with open(a.out, "w") as fh:
            fh.write(line + "\n")


if __name__ == "__main__":
    main()
