#!/usr/bin/env python3
"""Time of the overlay (csrc/hip/overlay.hip: the selection launch + the pixel launch) on 256 camera frames of 1280 x 720, RGB and NV12, 8
boxes per frame that cover about a tenth of the frame together, each with its label: boxes and labels in place and out of place, and boxes,
labels and mask tints in place.  The figure is DEVICE time between two events recorded around the two launches, as mars_hip_overlay_ms
brackets them in the device form; the launchers are called directly (mhip_overlay_select, mhip_overlay) because the workload fixes the
boxes.  Median of --runs after --warmup, min and max beside it, on an otherwise idle device.  The yardstick, in the same run and under the
same events: the device-to-device copy of the same frames (mhip_d2d_async).  Beside it the same boxes through the in-place fill redaction
(mhip_redact_select, mhip_redact; the method of tools/redact_rate.py).  The first and the last frame of every form are compared with the
restatement (tests/overlayref.py).  One JSON line, kept in profiles/overlay.json (--out).

usage: tools/overlay_rate.py [--frames 256] [--src 1280x720] [--boxes 8] [--runs 20] [--warmup 3] [--out profiles/overlay.json]
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
sys.path.insert(0, os.path.join(ROOT, "tools"))

import marsrt  # noqa: E402
import overlayref as O  # noqa: E402
import redact_rate as RR  # noqa: E402
from test_gpu_overlay import LaunchRec, packed  # noqa: E402  (mhip_overlay_t and a colour as the kernels take it)


def declare(L):
    RR.declare(L)
    for n in ("mhip_overlay_select", "mhip_overlay"):
        f = getattr(L, n)
        f.restype, f.argtypes = C.c_int, [C.POINTER(LaunchRec)]
    return L


def measure(L, a, fmt, W, H):
    F, n = a.frames, a.boxes
    rng = np.random.default_rng(0x0FE21A + fmt)
    fb = O.frame_bytes(W, H, fmt)
    shots = rng.integers(0, 256, (8, fb), dtype=np.uint8)  # eight different frames, repeated
    boxes = RR.boxes_for(rng, F, n, W, H, a.share)
    boxes["cls"] = rng.integers(0, 80, (F, n))
    boxes["conf"] = rng.uniform(0.3, 1.0, (F, n))
    counts = np.full(F, n, dtype=np.int32)
    list_off = (np.arange(F) * n).astype(np.int32)
    pitch = (W + 31) // 32
    mw = rng.integers(0, 1 << 32, (n, H, pitch), dtype=np.uint64).astype(np.uint32)  # eight masks, shared by the frames
    mask_of = np.tile(np.arange(n, dtype=np.int32), F)
    pal = np.array([packed(rgb, fmt) for rgb in O.PALETTE], dtype=np.uint32)
    sizes = (("src", F * fb), ("dst", F * fb), ("keep", F * fb), ("boxes", boxes.nbytes), ("counts", 4 * F), ("off", 4 * F), ("mw", mw.nbytes),
             ("mask_of", mask_of.nbytes), ("pal", pal.nbytes), ("table", 48 * F * n), ("table_n", 4 * F), ("marks", 16 * F * n), ("marks_n", 4 * F),
             ("stats", 24 * F), ("rtable", 20 * F * n), ("rstats", 16 * F))
    dev = {k: L.mhip_malloc(v) for k, v in sizes}
    assert all(dev.values()), "mhip_malloc"
    for f in range(F):
        assert L.mhip_h2d_async(dev["keep"] + f * fb, shots[f % 8].ctypes.data, fb) == 0
    for k, arr in (("boxes", boxes), ("counts", counts), ("off", list_off), ("mw", mw), ("mask_of", mask_of), ("pal", pal)):
        assert L.mhip_h2d_async(dev[k], arr.ctypes.data, arr.nbytes) == 0
    assert L.mhip_sync() == 0
    ev = [L.mhip_event_create(), L.mhip_event_create()]

    def rec(dst, layers):
        return LaunchRec(frames=dev["src"], dst=dst, frame_stride=fb, n_frames=F, w=W, h=H, fmt=fmt, dets=dev["boxes"], counts=dev["counts"],
                         list_off=dev["off"], select_all=1, min_hits=1, text=5, mask_of=dev["mask_of"] if layers & O.MASKS else None,
                         mask_words=dev["mw"] if layers & O.MASKS else None, num_kpt=1, kpt_min_v=0.5, layers=layers, thick=2, radius=2, scale=2,
                         alpha=96, palette=dev["pal"], n_palette=16, no_key=packed((0, 0, 0), fmt),
                         text_col=(C.c_uint32 * 2)(packed((0, 0, 0), fmt), packed((255, 255, 255), fmt)), table=dev["table"], table_n=dev["table_n"],
                         marks=dev["marks"], marks_n=dev["marks_n"], stats=dev["stats"])

    def overlay(p):
        return L.mhip_overlay_select(C.byref(p)) or L.mhip_overlay(C.byref(p))

    rp = RR.LaunchRec(dev["src"], dev["src"], fb, F, W, H, fmt, 0, dev["boxes"], dev["counts"], dev["off"], 0, 1, 1.0, 0.0, 0.0, 0, 0, None, None, 0,
                      None, None, 1, 4, (C.c_ubyte * 3)(0, 0, 0), dev["rtable"], dev["table_n"], dev["rstats"])
    restore = lambda: L.mhip_d2d_async(dev["src"], dev["keep"], F * fb)  # noqa: E731

    def timed_in_place(fn):  # every run starts from the original frames: the restore is outside the events
        ms = []
        for k in range(a.warmup + a.runs):
            assert restore() == 0 and L.mhip_event_record(ev[0]) == 0 and fn() == 0 and L.mhip_event_record(ev[1]) == 0
            t = float(L.mhip_event_elapsed_ms(ev[0], ev[1]))
            if k >= a.warmup:
                ms.append(t)
        return {"median": round(float(np.median(ms)), 4), "min_max": [round(min(ms), 4), round(max(ms), 4)]}

    def check(layers, where):  # the first and the last frame against the restatement, and the statistics
        stats = np.zeros(F, dtype=O.STATS)
        assert L.mhip_d2h_async(stats.ctypes.data, dev["stats"], stats.nbytes) == 0 and L.mhip_sync() == 0
        for f in (0, F - 1):
            want, wst, _ = O.overlay_frames_np(shots[f % 8], boxes[f], np.zeros(n, dtype=np.int32), W, H, fmt, mask_words=mw,
                                               mask_of_box=np.arange(n) if layers & O.MASKS else None, layers=layers)
            got = np.empty(fb, dtype=np.uint8)
            assert L.mhip_d2h_async(got.ctypes.data, dev[where] + f * fb, fb) == 0 and L.mhip_sync() == 0
            assert np.array_equal(got, want[0]), "frame %d (layers %d, %s) differs from the restatement" % (f, layers, where)
            assert stats[f].tobytes() == wst[0].tobytes()
        return int(stats["pixels"].sum())

    BL, MBL = O.BOXES | O.LABELS, O.MASKS | O.BOXES | O.LABELS
    out = {"copy_ms": RR.timed(L, ev, a.runs, a.warmup, restore)}
    p = rec(dev["dst"], BL)
    out["out_of_place_ms"] = RR.timed(L, ev, a.runs, a.warmup, lambda: overlay(p))
    px = check(BL, "dst")
    p_in = rec(dev["src"], BL)
    out["in_place_ms"] = timed_in_place(lambda: overlay(p_in))
    assert check(BL, "src") == px
    p_m = rec(dev["src"], MBL)
    out["in_place_masks_ms"] = timed_in_place(lambda: overlay(p_m))
    px_m = check(MBL, "src")
    out["redact_fill_in_place_ms"] = timed_in_place(lambda: L.mhip_redact_select(C.byref(rp)) or L.mhip_redact(C.byref(rp)))
    copy = out["copy_ms"]["median"]
    out.update({"format": "nv12" if fmt else "rgb", "frames": F, "size": "%dx%d" % (W, H), "boxes_per_frame": n,
                "painted_share": round(px / (F * W * H), 4), "painted_share_with_masks": round(px_m / (F * W * H), 4), "bytes_frames": F * fb,
                "bytes_copy": 2 * F * fb, "copy_GBs": round(2 * F * fb / (copy * 1e-3) / 1e9, 1),
                "out_of_place_vs_copy": round(out["out_of_place_ms"]["median"] / copy, 3),
                "in_place_vs_copy": round(out["in_place_ms"]["median"] / copy, 3),
                "in_place_masks_vs_copy": round(out["in_place_masks_ms"]["median"] / copy, 3),
                "redact_fill_in_place_vs_copy": round(out["redact_fill_in_place_ms"]["median"] / copy, 3)})
    for e in ev:
        L.mhip_event_destroy(e)
    for v in dev.values():
        L.mhip_free(v)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=256)
    ap.add_argument("--src", default="1280x720")
    ap.add_argument("--boxes", type=int, default=8)
    ap.add_argument("--share", type=float, default=0.1)
    ap.add_argument("--runs", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--resources", default="", help="the kernels' VGPR / LDS / scratch use from the compiler's resource listing, recorded as given")
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    W, H = (int(v) for v in a.src.split("x"))
    marsrt.nna_init()
    L = declare(marsrt.lib())
    O.bind(marsrt)
    res = {"tool": "tools/overlay_rate.py", "layers": "boxes + labels (scale 2, thickness 2); the masks form adds tints (alpha 96)", "runs": a.runs,
           "warmup": a.warmup, "timing": "device ms between two events", "yardstick": "mhip_d2d_async of the same frames under the same events",
           "kernel_resources": a.resources, "results": [measure(L, a, fmt, W, H) for fmt in (O.RGB, O.NV12)],
           "note": "measured once, on one machine"}
    line = json.dumps(res)
    print(line, flush=True)
    if a.out:
        with open(a.out, "w") as fh:
            fh.write(line + "\n")


if __name__ == "__main__":
    main()
