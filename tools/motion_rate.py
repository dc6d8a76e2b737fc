#!/usr/bin/env python3
"""Time of the motion stage (csrc/hip/motion.hip: the cells launch + the map launch) on 256 camera frames of 1280 x 720, RGB and NV12, cell 16,
in two configurations: 256 streams of one step each, and 16 streams of sixteen steps each (fewer workgroups, each with a serial step loop).
The figure is DEVICE time between two events recorded around mars_hip_motion_device, which enqueues the two launches; mars_hip_motion_ms,
the stage's own bracket, is kept beside it.  Median of --runs after --warmup, min and max beside it, on an otherwise idle device.  The runs
alternate between two sets of frames that differ by a bright block over about a tenth of the frame, so every timed call finds those cells
active.  The yardstick, in the same run and under the same events: the device-to-device copy of the same frame bytes (mhip_d2d_async).
Beside the times: the bytes the stage reads algorithmically -- every frame byte of RGB, the Y plane of NV12 -- against the copy's two
passes over every byte.  The second call behind a reset is compared with tests/motionref.py on the first and the last stream.  One JSON line,
kept in profiles/motion.json (--out).

usage: tools/motion_rate.py [--frames 256] [--src 1280x720] [--cell 16] [--runs 20] [--warmup 3] [--out profiles/motion.json]
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
import motionref as R  # noqa: E402


def declare(L):
    P, Z, I = C.c_void_p, C.c_size_t, C.c_int
    L.mhip_malloc.restype, L.mhip_malloc.argtypes = P, [Z]
    L.mhip_free.restype, L.mhip_free.argtypes = None, [P]
    L.mhip_event_create.restype, L.mhip_event_create.argtypes = P, []
    L.mhip_event_destroy.restype, L.mhip_event_destroy.argtypes = None, [P]
    L.mhip_event_elapsed_ms.restype, L.mhip_event_elapsed_ms.argtypes = C.c_float, [P, P]
    for n, a in (("mhip_h2d_async", [P, P, Z]), ("mhip_d2d_async", [P, P, Z]), ("mhip_sync", []), ("mhip_event_record", [P])):
        f = getattr(L, n)
        f.restype, f.argtypes = I, a
    return L


def summary(ms):
    return {"median": round(float(np.median(ms)), 4), "min_max": [round(min(ms), 4), round(max(ms), 4)]}


def shots_for(rng, W, H, fmt):
    """eight different frames, and the same with a bright block over a tenth of the frame"""
    fb = R.frame_bytes(W, H, fmt)
    a = rng.integers(0, 256, (8, fb), dtype=np.uint8)
    b = a.copy()
    bw, bh = int(W * 0.4), int(H * 0.25)
    for k in range(8):
        x0, y0 = int(rng.integers(0, W - bw)), int(rng.integers(0, H - bh))
        if fmt:
            b[k, :W * H].reshape(H, W)[y0:y0 + bh, x0:x0 + bw] = 255
        else:
            b[k].reshape(H, W, 3)[y0:y0 + bh, x0:x0 + bw] = 255
    return a, b


def measure(L, a, fmt, W, H, S):
    F, T = a.frames, a.frames // S
    rng = np.random.default_rng(0x307109 + fmt)
    fb = R.frame_bytes(W, H, fmt)
    shots = shots_for(rng, W, H, fmt)
    dev = [L.mhip_malloc(F * fb) for _ in range(3)]  # the two sets and the copy's destination
    assert all(dev), "mhip_malloc"
    for k in (0, 1):
        for f in range(F):
            assert L.mhip_h2d_async(dev[k] + f * fb, shots[k][f % 8].ctypes.data, fb) == 0
    assert L.mhip_sync() == 0
    ev = [L.mhip_event_create(), L.mhip_event_create()]
    mo = marsrt.Motion(S, W, H, fmt, a.cell)
    opts = marsrt.motion_opts(min_neighbors=1)
    # behind a reset: set 0 is the background, set 1 moves; the first and the last stream against the restatement
    mo.device(dev[0], F, opts)
    mo.device(dev[1], F, opts)
    maps, stats, _ = mo.results()
    for s in (0, S - 1):
        ref = R.Detector(1, W, H, fmt, a.cell)
        idx = [t * S + s for t in range(T)]
        ref.run(np.stack([shots[0][f % 8] for f in idx]), min_neighbors=1)
        wm, ws, _ = ref.run(np.stack([shots[1][f % 8] for f in idx]), min_neighbors=1)
        assert np.array_equal(maps[idx], wm) and stats[idx].tobytes() == ws.tobytes(), "stream %d differs from the restatement" % s
        assert np.array_equal(mo.read(s)[0], ref.bg[0].astype(np.uint16)), "bg of stream %d differs from the restatement" % s
    active = float(stats["active"].sum()) / (F * mo.gw * mo.gh)
    copy_ms, ms, stage_ms = [], [], []
    for k in range(a.warmup + a.runs):
        assert L.mhip_event_record(ev[0]) == 0 and L.mhip_d2d_async(dev[2], dev[k & 1], F * fb) == 0 and L.mhip_event_record(ev[1]) == 0
        tc = float(L.mhip_event_elapsed_ms(ev[0], ev[1]))
        assert L.mhip_event_record(ev[0]) == 0
        mo.device(dev[k & 1], F, opts)
        assert L.mhip_event_record(ev[1]) == 0
        tm = float(L.mhip_event_elapsed_ms(ev[0], ev[1]))
        if k >= a.warmup:
            copy_ms.append(tc)
            ms.append(tm)
            stage_ms.append(mo.ms())
    read_b = F * (W * H if fmt else fb)
    out = {"format": "nv12" if fmt else "rgb", "frames": F, "size": "%dx%d" % (W, H), "cell": a.cell, "streams": S, "steps": T,
           "active_share": round(active, 4), "copy_ms": summary(copy_ms), "motion_ms": summary(ms), "stage_ms": summary(stage_ms),
           "bytes_frames": F * fb, "bytes_read": read_b, "bytes_copy": 2 * F * fb}
    out["motion_vs_copy"] = round(out["motion_ms"]["median"] / out["copy_ms"]["median"], 3)
    out["copy_GBs"] = round(2 * F * fb / (out["copy_ms"]["median"] * 1e-3) / 1e9, 1)
    out["motion_GBs"] = round(read_b / (out["motion_ms"]["median"] * 1e-3) / 1e9, 1)
    mo.close()
    for e in ev:
        L.mhip_event_destroy(e)
    for v in dev:
        L.mhip_free(v)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=256)
    ap.add_argument("--src", default="1280x720")
    ap.add_argument("--cell", type=int, default=16)
    ap.add_argument("--runs", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--resources", default="", help="the kernels' VGPR / LDS / scratch use from the compiler's resource listing, recorded as given")
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    W, H = (int(v) for v in a.src.split("x"))
    marsrt.nna_init()
    L = declare(marsrt.lib())
    res = {"tool": "tools/motion_rate.py", "runs": a.runs, "warmup": a.warmup, "timing": "device ms between two events",
           "yardstick": "mhip_d2d_async of the same frames under the same events", "kernel_resources": a.resources,
           "results": [measure(L, a, fmt, W, H, S) for fmt in (R.RGB, R.NV12) for S in (a.frames, max(a.frames // 16, 1))],
           "note": "measured once, on one machine"}
    line = json.dumps(res)
    print(line, flush=True)
    if a.out:
        with open(a.out, "w") as fh:
            fh.write(line + "\n")


if __name__ == "__main__":
    main()
