#!/usr/bin/env python3
"""Images/s of a resident loop (inputs uploaded once, run_device_async back to back) with the raw-head detection tail switched on against the
graph alone, for the DFL path and, as the yardstick, the anchor path at the same input sizes.  One JSON line per model.

usage: tools/dfl_tail_rate.py [--batch 256] [--steps 30] [--warmup 5] [--only NAME]
"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "thingino-accel_amd"))

import marsrt  # noqa: E402
from conftest import lcg_frame  # noqa: E402


def models():
    with open(os.path.join(ROOT, "tests", "golden", "models", "yolov5nu.mars"), "rb") as fh:
        yield "yolov5nu (DFL, scales 0.1)", fh.read(), lambda m: m.detect_dfl_device(box_scales=0.1, cls_scales=0.1)
    yield "dfl twin 640", marsrt.synth_model(width_x16=4, input_hw=640, seed=1, head="dfl"), lambda m: m.detect_dfl_device()
    yield "dfl twin 320", marsrt.synth_model(width_x16=4, input_hw=320, seed=1, head="dfl"), lambda m: m.detect_dfl_device()
    yield "anchor twin 320", marsrt.synth_model(width_x16=4, input_hw=320, seed=1), lambda m: m.detect_heads_device()
    yield "anchor twin 640", marsrt.synth_model(width_x16=4, input_hw=640, seed=1), lambda m: m.detect_heads_device()


def rate(m, tail, steps, warmup):
    for k in range(warmup + steps):
        if k == warmup:
            marsrt.lib().mars_hip_sync()
            t0 = time.perf_counter()
        m.run_device(sync=False)
        if tail:
            tail(m)
    marsrt.lib().mars_hip_sync()
    return m.batch * steps / (time.perf_counter() - t0)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=256)
    ap.add_argument("--steps", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--only", default="")
    a = ap.parse_args()
    marsrt.nna_init()
    for name, d, tail in models():
        if a.only and a.only not in name:
            continue
        m = marsrt.Model(d, batch=a.batch)
        nb = m.input_view(0).shape[1]
        for f in range(a.batch):
            m.input_view(0)[f] = lcg_frame(0x5EED0000 + f % 16, nb)
        m.upload()
        g = [rate(m, None, a.steps, a.warmup) for _ in range(3)]
        t = [rate(m, tail, a.steps, a.warmup) for _ in range(3)]
        kept = sum(len(x) for x in m.detect_results()) / a.batch
        print(json.dumps({"model": name, "batch": a.batch, "graph_only_img_s": round(max(g)), "with_tail_img_s": round(max(t)),
                          "loss_pct": round(100 * (1 - max(t) / max(g)), 2), "kept_boxes_per_frame": round(kept, 1)}), flush=True)
        m.close()


if __name__ == "__main__":
    main()
