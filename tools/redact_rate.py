#!/usr/bin/env python3
"""Time of the redaction (csrc/hip/redact.hip: the selection launch + the pixel launch) on 256 camera frames of 1280 x 720, RGB and NV12,
mosaic with cell 16, 8 boxes per frame that cover about a tenth of the frame together, in place and out of place.  The figure is DEVICE time
between two events recorded around the two launches, as mars_hip_redact_ms brackets them in the device form; the launchers are called
directly (mhip_redact_select, mhip_redact) because the workload fixes the boxes, and the device form takes its boxes from a detection tail.
Median of --runs after --warmup, min and max beside it, on an otherwise idle device.  The yardstick, in the same run and under the same
events: the device-to-device copy of the same frames (mhip_d2d_async).  Beside the times: the bytes each form touches algorithmically -- out
of place every byte once each way; in place the cells that meet a region read once and the redacted samples written once.  One JSON line
per format, all of them kept in profiles/redact.json (--out).

usage: tools/redact_rate.py [--frames 256] [--src 1280x720] [--cell 16] [--boxes 8] [--runs 20] [--warmup 3] [--out profiles/redact.json]
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
import redactref as R  # noqa: E402


class LaunchRec(C.Structure):  # mhip_redact_t of csrc/mhip.h
    _fields_ = [("frames", C.c_void_p), ("dst", C.c_void_p), ("frame_stride", C.c_size_t), ("n_frames", C.c_int), ("w", C.c_int), ("h", C.c_int),
                ("fmt", C.c_int), ("nv12_flags", C.c_uint), ("dets", C.c_void_p), ("counts", C.c_void_p), ("list_off", C.c_void_p),
                ("det_cap", C.c_int), ("select_all", C.c_int), ("expand", C.c_float), ("min_conf", C.c_float), ("ident_min", C.c_float),
                ("cls_first", C.c_int), ("cls_count", C.c_int), ("idents", C.c_void_p), ("mask_recs", C.c_void_p), ("mask_max", C.c_int),
                ("mask_of", C.c_void_p), ("mask_words", C.c_void_p), ("mode", C.c_int), ("cell_log2", C.c_int), ("fill", C.c_ubyte * 3),
                ("table", C.c_void_p), ("table_n", C.c_void_p), ("stats", C.c_void_p)]


def declare(L):
    P, Z, I = C.c_void_p, C.c_size_t, C.c_int
    L.mhip_malloc.restype, L.mhip_malloc.argtypes = P, [Z]
    L.mhip_free.restype, L.mhip_free.argtypes = None, [P]
    L.mhip_event_create.restype, L.mhip_event_create.argtypes = P, []
    L.mhip_event_destroy.restype, L.mhip_event_destroy.argtypes = None, [P]
    L.mhip_event_elapsed_ms.restype, L.mhip_event_elapsed_ms.argtypes = C.c_float, [P, P]
    for n, a in (("mhip_h2d_async", [P, P, Z]), ("mhip_d2h_async", [P, P, Z]), ("mhip_d2d_async", [P, P, Z]), ("mhip_sync", []),
                 ("mhip_event_record", [P]), ("mhip_redact_select", [C.POINTER(LaunchRec)]), ("mhip_redact", [C.POINTER(LaunchRec)])):
        f = getattr(L, n)
        f.restype, f.argtypes = I, a
    return L


def boxes_for(rng, F, n, W, H, share):
    """n boxes a frame, 16 : 9 like the frame, share / n of its area each, anywhere inside it"""
    bw, bh = W * np.sqrt(share / n), H * np.sqrt(share / n)
    b = np.zeros((F, n), dtype=marsrt.DET_DTYPE)
    b["x"], b["y"] = rng.uniform(bw / 2, W - bw / 2, (F, n)), rng.uniform(bh / 2, H - bh / 2, (F, n))
    b["w"], b["h"], b["conf"] = bw, bh, 0.9
    return b


def touched(boxes, W, H, cell, fmt):
    """(|U|, bytes of the cells that meet U, bytes of the redacted samples) over all frames, by the restatement's union"""
    px = cells = 0
    ys, xs = np.arange(0, H, cell), np.arange(0, W, cell)
    for f in range(len(boxes)):
        U, st = R.union_np(boxes[f], W, H)
        px += st[3]
        k = np.add.reduceat(np.add.reduceat(U.astype(np.int64), ys, axis=0), xs, axis=1)
        n = (np.minimum(ys + cell, H) - ys)[:, None] * (np.minimum(xs + cell, W) - xs)[None, :]
        cells += int(n[k > 0].sum())
    per = 1.5 if fmt else 3.0  # bytes a pixel (NV12: the chroma sample of four pixels is two bytes)
    return px, int(cells * per), int(px * per)


def timed(L, ev, runs, warmup, fn):
    ms = []
    for k in range(warmup + runs):
        assert L.mhip_event_record(ev[0]) == 0 and fn() == 0 and L.mhip_event_record(ev[1]) == 0
        t = float(L.mhip_event_elapsed_ms(ev[0], ev[1]))
        if k >= warmup:
            ms.append(t)
    return {"median": round(float(np.median(ms)), 4), "min_max": [round(min(ms), 4), round(max(ms), 4)]}


def measure(L, a, fmt, W, H):
    F, n = a.frames, a.boxes
    rng = np.random.default_rng(0x5EDAC7 + fmt)
    fb = R.frame_bytes(W, H, fmt)
    shots = rng.integers(0, 256, (8, fb), dtype=np.uint8)  # eight different frames, repeated
    boxes = boxes_for(rng, F, n, W, H, a.share)
    counts = np.full(F, n, dtype=np.int32)
    list_off = (np.arange(F) * n).astype(np.int32)
    dev = {k: L.mhip_malloc(v) for k, v in (("src", F * fb), ("dst", F * fb), ("keep", F * fb), ("boxes", boxes.nbytes), ("counts", 4 * F), ("off", 4 * F),
                                            ("table", 20 * F * n), ("table_n", 4 * F), ("stats", 16 * F))}
    assert all(dev.values()), "mhip_malloc"
    for f in range(F):
        assert L.mhip_h2d_async(dev["keep"] + f * fb, shots[f % 8].ctypes.data, fb) == 0
    for k, arr in (("boxes", boxes), ("counts", counts), ("off", list_off)):
        assert L.mhip_h2d_async(dev[k], arr.ctypes.data, arr.nbytes) == 0
    assert L.mhip_sync() == 0
    ev = [L.mhip_event_create(), L.mhip_event_create()]

    def rec(dst):
        return LaunchRec(dev["src"], dst, fb, F, W, H, fmt, 0, dev["boxes"], dev["counts"], dev["off"], 0, 1, 1.0, 0.0, 0.0, 0, 0, None, None, 0,
                         None, None, R.MOSAIC, a.cell.bit_length() - 1, (C.c_ubyte * 3)(0, 0, 0), dev["table"], dev["table_n"], dev["stats"])

    def redact(p):
        return L.mhip_redact_select(C.byref(p)) or L.mhip_redact(C.byref(p))

    restore = lambda: L.mhip_d2d_async(dev["src"], dev["keep"], F * fb)  # noqa: E731
    out = {"copy_ms": timed(L, ev, a.runs, a.warmup, restore)}
    p_out, p_in = rec(dev["dst"]), rec(dev["src"])
    out["out_of_place_ms"] = timed(L, ev, a.runs, a.warmup, lambda: redact(p_out))

    def in_place():  # every run starts from the original frames: the restore is outside the events
        return redact(p_in)
    ms = []
    for k in range(a.warmup + a.runs):
        assert restore() == 0 and L.mhip_event_record(ev[0]) == 0 and in_place() == 0 and L.mhip_event_record(ev[1]) == 0
        t = float(L.mhip_event_elapsed_ms(ev[0], ev[1]))
        if k >= a.warmup:
            ms.append(t)
    out["in_place_ms"] = {"median": round(float(np.median(ms)), 4), "min_max": [round(min(ms), 4), round(max(ms), 4)]}
    # both forms against the restatement on the first and the last frame, and the statistics
    stats = np.zeros(F, dtype=marsrt.REDACT_STATS_DTYPE)
    assert L.mhip_d2h_async(stats.ctypes.data, dev["stats"], stats.nbytes) == 0 and L.mhip_sync() == 0
    for f in (0, F - 1):
        U, st = R.union_np(boxes[f], W, H)
        want = R.redact_frame_np(shots[f % 8], W, H, fmt, U, R.MOSAIC, a.cell)
        for k in ("dst", "src"):
            got = np.empty(fb, dtype=np.uint8)
            assert L.mhip_d2h_async(got.ctypes.data, dev[k] + f * fb, fb) == 0 and L.mhip_sync() == 0
            assert np.array_equal(got, want), "frame %d of %s differs from the restatement" % (f, k)
        assert tuple(stats[f]) == st
    px, cell_b, red_b = touched(boxes, W, H, a.cell, fmt)
    assert px == int(stats["pixels"].sum())
    copy = out["copy_ms"]["median"]
    out.update({"format": "nv12" if fmt else "rgb", "frames": F, "size": "%dx%d" % (W, H), "cell": a.cell, "boxes_per_frame": n,
                "redacted_share": round(px / (F * W * H), 4), "bytes_frames": F * fb, "bytes_out_of_place": 2 * F * fb,
                "bytes_in_place": cell_b + red_b, "bytes_copy": 2 * F * fb,
                "out_of_place_vs_copy": round(out["out_of_place_ms"]["median"] / copy, 3),
                "in_place_vs_copy": round(out["in_place_ms"]["median"] / copy, 3),
                "copy_GBs": round(2 * F * fb / (copy * 1e-3) / 1e9, 1),
                "out_of_place_GBs": round(2 * F * fb / (out["out_of_place_ms"]["median"] * 1e-3) / 1e9, 1),
                "in_place_GBs": round((cell_b + red_b) / (out["in_place_ms"]["median"] * 1e-3) / 1e9, 1)})
    for e in ev:
        L.mhip_event_destroy(e)
    for v in dev.values():
        L.mhip_free(v)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=256)
    ap.add_argument("--src", default="1280x720")
    ap.add_argument("--cell", type=int, default=16)
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
    res = {"tool": "tools/redact_rate.py", "mode": "mosaic", "runs": a.runs, "warmup": a.warmup, "timing": "device ms between two events",
           "yardstick": "mhip_d2d_async of the same frames under the same events", "kernel_resources": a.resources,
           "results": [measure(L, a, fmt, W, H) for fmt in (R.RGB, R.NV12)], "note": "measured once, on one machine"}
    line = json.dumps(res)
    print(line, flush=True)
    if a.out:
        with open(a.out, "w") as fh:
            fh.write(line + "\n")


if __name__ == "__main__":
    main()
