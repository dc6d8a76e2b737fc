#!/usr/bin/env python3
"""Cost of the track tail (mars_hip_track_device / mars_yolo_track_lists: one launch of csrc/hip/track.hip).

(a) The tail alone.  The kernel runs on streams no caller can put events on, so the figure is host wall time of mars_yolo_track_lists -- upload
    of the lists, the launch, download of the ids, the waits -- on an otherwise idle device, median of --runs after --warmup, on a tracker
    that already holds the scene's tracks (every call is one more batch of the same scene, so every box matches its track).  Beside it the
    same call with every count zero (the copies, the launch and a kernel that finds nothing to do: what is not association work), and the
    host alternative measured once in the same process: mars_hip_detect_results of a batch-256 detector (the 6 MB a deployment would have
    to fetch every batch) plus the numpy restatement of tests/test_track_cpu.py on the same lists.  Cases: 256 streams x 1 step and
    1 stream x 256 steps at 20 boxes per frame; 256 streams x 1 step at 256 boxes per frame; the 256-round staircase of
    tests/test_gpu_track.py on one stream.  For the kernel's own time run this under `rocprofv3 --kernel-trace --stats -- python ...`.
(b) The chain.  The second-stage loop of INTEGRATION.md section 3 (front-end -> detector at batch 256 -> raw-head tail -> crops -> second
    model -> classify -> match -> labels and identities), nothing waiting inside a window, frames per second over --iters iterations ending
    in mars_hip_sync(); three windows without the track call and three with it (256 streams x 1 step, identities carried), alternating.
    Without the call the loop runs exactly the code of the commit before this feature (the feature adds a call, it changes none), so its
    median and window-to-window spread stand for the parent's.

One JSON line; kept in profiles/track_tail.json.

usage: tools/track_rate.py [--runs 30] [--warmup 5] [--iters 40] [--skip-chain]
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
from test_track_cpu import SLOTS, F, TrackerNp, box, frames, track_np  # noqa: E402

CW, CH = 320, 240


def static_scene(streams, steps, boxes, max_det):
    """`boxes` boxes of 30 x 30 on a grid, the same in every frame"""
    rows = [box(40.0 * (k % 16), y=40.0 * (k // 16), w=30.0, h=30.0, cls=k % 3) for k in range(boxes)]
    return frames(*([rows] * (streams * steps)), max_det=max_det)


def staircase():
    gap = F(40) - np.arange(2 * SLOTS, dtype=F) * F(0.05)
    x = np.concatenate([[F(0)], np.cumsum(gap[:-1], dtype=F)]).astype(F)
    return [frames([box(float(v), w=100.0, h=100.0) for v in x[k::2]], max_det=SLOTS) for k in (0, 1)]


def wall_ms(fn, runs, warmup, before=None):
    t = []
    for k in range(warmup + runs):
        if before:
            before()
        marsrt.lib().mars_hip_sync()
        t0 = time.perf_counter()
        fn()
        if k >= warmup:
            t.append((time.perf_counter() - t0) * 1e3)
    return dict(median=round(float(np.median(t)), 4), min=round(min(t), 4), max=round(max(t), 4))


def tail_case(name, streams, steps, boxes, max_det, a, major=False):
    d, n = static_scene(streams, steps, boxes, max_det)
    o = marsrt.track_opts(stream_major=major)
    trk = marsrt.Tracker(streams)
    marsrt.track_lists(trk, d, n, o)
    res = dict(case=name, streams=streams, steps=steps, boxes_per_frame=boxes, max_det=max_det,
               track_lists_wall_ms=wall_ms(lambda: marsrt.track_lists(trk, d, n, o), a.runs, a.warmup),
               empty_lists_wall_ms=wall_ms(lambda: marsrt.track_lists(trk, d, n * 0, o), a.runs, a.warmup))
    trk.close()
    ref = TrackerNp(streams)
    track_np(ref, d, n, stream_major=major)
    t0 = time.perf_counter()
    track_np(ref, d, n, stream_major=major)
    res["numpy_restatement_wall_ms"] = round((time.perf_counter() - t0) * 1e3, 1)
    return res


def tail(a):
    out = [tail_case("256 streams x 1 step, 20 boxes", 256, 1, 20, 32, a),
           tail_case("1 stream x 256 steps, 20 boxes (serial by definition)", 1, 256, 20, 32, a, major=True),
           tail_case("256 streams x 1 step, 256 boxes", 256, 1, 256, 256, a)]
    (d0, n0), (d1, n1) = staircase()
    trk = marsrt.Tracker(1)

    def births():
        trk.reset()
        marsrt.track_lists(trk, d0, n0)

    out.append(dict(case="staircase: 256 tracks x 256 detections on one stream, one pair per round", streams=1, steps=1, boxes_per_frame=256,
                    track_lists_wall_ms=wall_ms(lambda: marsrt.track_lists(trk, d1, n1), a.runs, a.warmup, before=births)))
    trk.close()
    return out


class Loop:
    """the second-stage loop of INTEGRATION.md section 3 at detector batch 256"""

    def __init__(self, batch=256, second=64):
        self.B = batch
        self.det = marsrt.Model(marsrt.synth_model(width_x16=4, input_hw=320, seed=3), batch=batch)
        with open(os.path.join(ROOT, "tests", "golden", "models", "tiny_160_int8.mars"), "rb") as fh:
            self.dst = marsrt.Model(fh.read(), batch=second)
        shots = [lcg_frame(0x5EC0000 + f, CW * CH * 3 // 2) for f in range(8)]
        self.buf = marsrt.DeviceBuffer(np.stack([shots[f % 8] for f in range(batch)]))
        self.gal = marsrt.Gallery(64, 64)
        rows = (np.stack([lcg_frame(0x6A190000 + k, 64).view(np.int8).astype(np.int32) for k in range(50)]) << 9) + 40000
        self.gal.add(rows, np.arange(50) + 1000)
        self.trk = marsrt.Tracker(batch)
        self.roi = marsrt.roi_opts(CW, CH, fmt=marsrt.CAMERA_NV12)
        self.track_opts = marsrt.track_opts(min_conf=0.3, carry_identity=True)

    def once(self, track):
        det, dst = self.det, self.dst
        det.preprocess_nv12_device(self.buf.ptr, CW, CH, self.B)
        det.run_device(sync=False)
        det.detect_heads_device(conf=0.25, src=(CW, CH))
        dst.crop_detections(det, self.buf.ptr, self.roi, device=True)
        dst.run_device(sync=False)
        dst.classify_device(top_k=3)
        dst.match_device(self.gal, top_k=3)
        det.label_detections(dst)
        det.identify_detections(dst)
        if track:
            det.track_device(self.trk, self.track_opts)

    def window(self, iters, track):
        L = marsrt.lib()
        L.mars_hip_sync()
        t0 = time.perf_counter()
        for _ in range(iters):
            self.once(track)
        L.mars_hip_sync()
        return self.B * iters / (time.perf_counter() - t0)

    def close(self):
        self.trk.close()
        self.gal.close()
        self.dst.close()
        self.det.close()
        self.buf.free()


def chain(a):
    lp = Loop()
    for track in (False, True):  # every shape of the timed windows, warm
        lp.window(max(a.iters // 4, 3), track)
    # what the loop leaves per batch, and what fetching it costs the host
    t0 = time.perf_counter()
    dets = lp.det.detect_results()
    fetch_ms = (time.perf_counter() - t0) * 1e3
    t0 = time.perf_counter()
    lp.det.detect_results()
    fetch_ms = min(fetch_ms, (time.perf_counter() - t0) * 1e3)
    live = [len(lp.trk.read(b)[0]) for b in range(0, lp.B, 37)]
    rates = {False: [], True: []}
    for _ in range(3):
        for track in (False, True):
            rates[track].append(lp.window(a.iters, track))
    lp.close()
    base, with_t = rates[False], rates[True]
    mb, mt = float(np.median(base)), float(np.median(with_t))
    spread = max(base) - min(base)
    return dict(loop="INTEGRATION.md section 3, second stage: detector 320x320 twin at batch 256 from NV12 320x240, tiny_160_int8.mars at batch 64, gallery of 50 rows",
                iters_per_window=a.iters, frames_per_window=lp.B * a.iters,
                boxes_per_frame_mean=round(float(np.mean([len(x) for x in dets])), 1), live_tracks_sampled_streams=live,
                detect_results_fetch_wall_ms=round(fetch_ms, 3),
                without_track_fps_windows=[round(x, 1) for x in base], without_track_fps_median=round(mb, 1),
                without_track_fps_spread_max_minus_min=round(spread, 1),
                with_track_fps_windows=[round(x, 1) for x in with_t], with_track_fps_median=round(mt, 1),
                drop_fps=round(mb - mt, 1), drop_within_spread=bool(mb - mt <= spread))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--runs", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--iters", type=int, default=40)
    ap.add_argument("--skip-chain", action="store_true")
    a = ap.parse_args()
    marsrt.nna_init()
    out = {"tool": "tools/track_rate.py", "runs": a.runs, "warmup": a.warmup, "tail": tail(a)}
    if not a.skip_chain:
        out["chain"] = chain(a)
    print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
