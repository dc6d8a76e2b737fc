"""Best shots on the device (include/mars_hip.h, "Best shots"): mars_yolo_shot_lists over the stream and step counts of tests/shotref.py
in both frame orders, split invariance, reset, flush and collect, the case tables (table pressure, overflow, duplicates, ties, the gates),
the geometry table in both layouts with and without MARS_SHOT_KEEP_ASPECT, the refusals that need a device, and the chain detector ->
crop_detections_device -> track_device -> shots_device over two batches with its ordering.  The expected values come from the restatement
in Python integers of tests/shotref.py (checked by hand in tests/test_shot_cpu.py); every comparison -- records, table, counters, step and
plane pixels -- is byte for byte."""
import numpy as np
import pytest

import shotref as R
from test_gpu_roi import FRAME_SEED, Chain, second_stage

pytestmark = pytest.mark.gpu


def same_state(sh, ref, what):
    for b in range(ref.S):
        got, want = sh.read(b), ref.read(b)
        assert got[0].dtype == want[0].dtype and got[0].tobytes() == want[0].tobytes(), (what, b, got[0], want[0])
        assert got[1:] == want[1:], (what, b, got[1:], want[1:])
        slots, wslots = sh.read_slots(b), ref.read_slots(b)
        assert slots.dtype == wslots.dtype and slots.tobytes() == wslots.tobytes(), (what, b, np.flatnonzero(slots != wslots)[:4])
        for s in np.flatnonzero(wslots["state"] != R.FREE):
            px = sh.pixels(b, int(s))
            assert px.dtype == np.uint8 and px.tobytes() == ref.pixels(b, int(s)).tobytes(), (what, b, int(s))


def both(gpu, sh, ref, call, what, **kw):
    """the same crops through the device and through the restatement: records and state agree to the byte"""
    crops, rois, confs, cls, tracks, frames = call[:6]
    out = gpu.shot_lists(sh, crops, rois, confs, cls, tracks, frames, gpu.shot_opts(**kw))
    want = ref.run(crops, rois, confs, cls, tracks, frames, **kw)
    assert out.dtype == want.dtype and out.shape == want.shape, what
    assert out.tobytes() == want.tobytes(), (what, np.flatnonzero(out != want)[:4], out[out != want][:2], want[out != want][:2])
    same_state(sh, ref, what)
    return out


def pair(gpu, S, slots, tw, th, nhwc=True):
    return gpu.Shots(S, slots, tw, th, nhwc), R.ShotsNp(S, slots, tw, th, nhwc)


@pytest.mark.parametrize("shape", R.SHAPES, ids=["S%d-T%d%s" % (s, t, "-major" if m else "") for s, t, m in R.SHAPES])
def test_shot_lists(gpu, shape):
    S, T, major = shape
    name, S_, slots, tw, th, nhwc, calls = [x for x in R.gpu_scenes() if x[0] == "lists-S%d-T%d%s" % (S, T, "-major" if major else "")][0]
    sh, ref = pair(gpu, S, slots, tw, th, nhwc)
    both(gpu, sh, ref, calls[0], shape, **calls[0][6])
    assert sh.ms() > 0
    sh.close()
    sh.close()


def test_split_invariance_reset_flush_and_collect(gpu):
    """one call over 6 steps == three calls over 2 steps, byte for byte, under both maps; a reset of one stream starts that stream over;
    flush finishes what is live; collect hands over by ascending slot up to cap and frees exactly what it copied"""
    S, T, tw, th = 2, 6, 10, 9
    for major in (False, True):
        a = R.scene(0x5402000, S, T, 5, tw, th, True, major)
        kw = dict(max_gap=1, stream_major=major)
        one, ref = pair(gpu, S, 3, tw, th)
        whole = both(gpu, one, ref, a, ("whole", major), **kw)
        three, ref3 = pair(gpu, S, 3, tw, th)
        got = np.zeros_like(whole)
        got["slot"] = -1
        last = None
        for c in range(3):
            # the frames of steps 2 c and 2 c + 1, renumbered for a call over 2 steps
            fr = a[1]["frame"]
            step, stream = (fr % T, fr // T) if major else (fr // S, fr % S)
            sel = np.flatnonzero((fr >= 0) & (fr < S * T) & (step // 2 == c))
            rois = a[1][sel].copy()
            rois["frame"] = (stream[sel] * 2 + step[sel] % 2) if major else ((step[sel] % 2) * S + stream[sel])
            last = (a[0][sel], rois, a[2][sel], a[3][sel], a[4][sel], 2 * S)
            got[sel] = both(gpu, three, ref3, last, ("part", major, c), **kw)
        assert got.tobytes() == whole.tobytes()
        same_state(three, ref, ("parts against the whole", major))
        # stream 1 reset: the last part again, stream 0 going on and stream 1 on an empty table
        three.reset(1)
        ref3.reset(1)
        assert three.read(1)[1:] == (0, 0, 0) and not three.read(1)[0].any() and three.read(0)[3] == T
        same_state(three, ref3, "after reset")
        both(gpu, three, ref3, last, ("after reset", major), **kw)
        assert three.read(1)[3] == 2 and three.read(0)[3] == T + 2
        # flush, then collect below and above the DONE count
        three.flush(0)
        ref3.flush(0)
        same_state(three, ref3, "flush of one stream")
        three.flush()
        ref3.flush()
        same_state(three, ref3, "flush")
        for b in range(S):
            _, live, done, _ = three.read(b)
            assert live == 0 and done >= 2
            before = three.read_slots(b)
            slots, rgb, n = three.collect(b, 1)
            wslots, wrgb, wn = ref3.collect(b, 1)
            assert n == wn == done and slots.tobytes() == wslots.tobytes() and rgb.tobytes() == wrgb.tobytes() and len(slots) == 1
            after = three.read_slots(b)
            first = int(np.flatnonzero(before["state"] == R.DONE)[0])
            assert after[first]["state"] == R.FREE and not after[first].tobytes().strip(b"\0") and (after["state"] == R.DONE).sum() == done - 1
            same_state(three, ref3, ("collect 1", b))
            slots, rgb, n = three.collect(b, 0)
            assert n == done - 1 and len(slots) == 0
            slots, rgb, n = three.collect(b, 100)
            wslots, wrgb, wn = ref3.collect(b, 100)
            assert n == wn == done - 1 and slots.tobytes() == wslots.tobytes() and rgb.tobytes() == wrgb.tobytes()
            assert three.read(b)[1:3] == (0, 0) and not three.read_slots(b).tobytes().strip(b"\0")
        # the emptied tables take new tracks from slot 0 on
        both(gpu, three, ref3, last, ("after collect", major), **kw)
        one.close()
        three.close()


@pytest.mark.parametrize("name", sorted(R.CASES))
def test_case(gpu, name):
    S, slots, tw, th, nhwc, calls, need = R.CASES[name]()
    sh, ref = pair(gpu, S, slots, tw, th, nhwc)
    for c, call in enumerate(calls):
        both(gpu, sh, ref, call, (name, c), **call[6])
    sm = R.summary(ref)  # (of the restatement's state, which is the device's)
    assert all(sm[k] >= 1 for k in need), (name, sm)
    if name == "overflow":
        assert sh.read(0)[0].tolist() == [0, 0, 0, 43, 1, 256]
    sh.close()


@pytest.mark.parametrize("keep", [False, True], ids=["stretch", "keep_aspect"])
@pytest.mark.parametrize("nhwc", [True, False], ids=["nhwc", "nchw"])
@pytest.mark.parametrize("size", R.GEOMETRY, ids=["%dx%d" % s for s in R.GEOMETRY])
def test_geometry(gpu, size, nhwc, keep):
    tw, th = size
    a = R.geometry_scene(tw, th, nhwc)
    sh, ref = pair(gpu, 2, 4, tw, th, nhwc)
    out = both(gpu, sh, ref, a, (size, nhwc, keep), keep_aspect=keep, max_gap=1)
    assert (out["slot"] >= 0).sum() >= 2 and (out["taken"] == 1).sum() >= 2
    if tw >= 3 and th >= 3 and not keep:
        assert (out["sharp"] > 0).any()
    sh.close()


def test_refusals_on_the_device(gpu):
    FILE, TENSOR = gpu.MARS_ERR_INVALID_FILE, gpu.MARS_ERR_INVALID_TENSOR

    def refused(code, fn, *a, **kw):
        with pytest.raises(gpu.MarsError) as ei:
            fn(*a, **kw)
        assert ei.value.code == code

    refused(FILE, gpu.Shots, 0, 4, 8, 8)
    refused(FILE, gpu.Shots, 1, 0, 8, 8)
    refused(FILE, gpu.Shots, 1, 4, 0, 8)
    refused(TENSOR, gpu.Shots, 65536, 4, 8, 8)
    refused(TENSOR, gpu.Shots, 1, 257, 8, 8)
    refused(TENSOR, gpu.Shots, 1, 4, 1281, 8)
    refused(TENSOR, gpu.Shots, 1, 4, 8, 1281)
    sh, ref = pair(gpu, 3, 4, 10, 9)
    a = R.scene(0x5403000, 3, 1, 4, 10, 9)
    both(gpu, sh, ref, a, "before")
    lists = lambda *x, **kw: gpu.shot_lists(sh, *a[:5], *x, **kw)
    refused(TENSOR, lists, 4)                                              # 4 frames, 3 streams
    refused(FILE, lists, 0)
    refused(FILE, lists, 3, gpu.shot_opts(flags=8))
    refused(FILE, lists, 3, gpu.shot_opts(max_gap=-2))
    refused(FILE, lists, 3, gpu.shot_opts(min_sharp=-1))
    refused(FILE, lists, 3, gpu.shot_opts(min_mean=100, max_mean=50))
    refused(FILE, lists, 3, gpu.shot_opts(max_mean=256))
    refused(FILE, lists, 3, gpu.shot_opts(inside=True))                    # no frame size
    refused(TENSOR, sh.read, 3)
    refused(TENSOR, sh.read, -1)
    refused(TENSOR, sh.reset, 3)
    refused(TENSOR, sh.flush, 3)
    refused(TENSOR, sh.read_slots, 3)
    refused(TENSOR, sh.collect, 3, 1)
    refused(FILE, sh.collect, 0, -1)
    refused(TENSOR, sh.pixels, 0, 4)
    free = int(np.flatnonzero(sh.read_slots(0)["state"] == R.FREE)[0])
    refused(TENSOR, sh.pixels, 0, free)                                    # a FREE slot has no picture
    same_state(sh, ref, "nothing moved")
    sh.close()


# ---- the chain ---------------------------------------------------------------------------------------------------------------------------
def test_chain_shots(gpu):
    """detector -> crop_detections_device into tiny_160_int8.mars -> track_device -> shots_device over two batches of the same frames, S =
    the detector's batch: the records and the state equal shot_lists fed the fetched ROI table, detections, tracks and input bytes, and
    the restatement.  Then a crop call into the same model is enqueued straight behind a shots call: the shots call read the crops as
    they were"""
    d2, tin, tout, nhwc = second_stage(gpu, "shipped")
    c = Chain(gpu)
    S = c.det.batch
    dst = gpu.Model(d2, batch=8)
    _, buf = c.frames(FRAME_SEED)
    trk = gpu.Tracker(S)
    sh, ref = pair(gpu, S, 8, 160, 160, nhwc)
    twin = gpu.Shots(S, 8, 160, 160, nhwc)
    TENSOR = gpu.MARS_ERR_INVALID_TENSOR

    def refused(fn, *a, **kw):
        with pytest.raises(gpu.MarsError) as ei:
            fn(*a, **kw)
        assert ei.value.code == TENSOR

    refused(dst.shots_results, sh)                                         # nothing pending
    c.detect(buf)
    refused(dst.shots_device, c.det, sh)                                   # no crop call into dst
    CROP = c.opts(max_per_frame=3)
    dst.crop_detections(c.det, buf.ptr, CROP, device=True)
    refused(dst.shots_device, c.det, sh)                                   # no track results
    TRACK_KW = dict(min_conf=float(min(x["conf"].min() for x in c.det.detect_results())))  # every box is tracked
    c.det.track_device(trk, **TRACK_KW)
    for other in (gpu.Shots(2, 8, 160, 160, nhwc), gpu.Shots(S, 8, 64, 64, nhwc), gpu.Shots(S, 8, 160, 160, not nhwc)):
        refused(dst.shots_device, c.det, other)                            # 3 frames on 2 streams; another size; another layout
        other.close()
    refused(c.det.shots_device, c.det, sh)                                 # det_model == src_model
    trk.reset()

    def fetched():
        """what roi_results, detect_results, track_results and the input tensor's bytes give, one entry per crop"""
        rois, _ = dst.roi_results()
        dets, tracks = c.det.detect_results(), c.det.track_results()
        n, kept = dst.batch, len(rois)
        x = np.stack([dst.read_tensor(tin, frame=k)[:160 * 160 * 3] for k in range(n)]).view(np.int8)
        # the frames behind the kept crops: an empty rectangle each, which is what "k >= kept" comes to
        full = np.zeros(n, dtype=R.ROI)
        full[:kept] = rois
        confs, cls, tr = np.zeros(n, dtype=np.float32), np.zeros(n, dtype=np.int32), np.zeros(n, dtype=R.TRACK)
        tr["id"] = -1
        for k, r in enumerate(rois):
            confs[k], cls[k] = dets[r["frame"]][r["det"]]["conf"], dets[r["frame"]][r["det"]]["cls"]
            tr[k] = tuple(tracks[r["frame"], r["det"]])
        return x, full, confs, cls, tr, S

    KW = dict(max_gap=2)
    got = []
    for r in range(2):
        c.detect(buf)
        dst.crop_detections(c.det, buf.ptr, CROP, device=True)
        c.det.track_device(trk, **TRACK_KW)
        dst.shots_device(c.det, sh, **KW)                                   # nothing has waited since the detector's front-end
        rec = dst.shots_results(sh)
        call = fetched()
        want = both(gpu, twin, ref, call, ("chain", r), **KW)
        assert rec.tobytes() == want.tobytes(), (r, rec, want)
        same_state(sh, ref, ("chain", r))
        got.append(rec)
    assert (got[0]["slot"] >= 0).any() and (got[0]["taken"] == 1).any() and (got[0]["sharp"] > 0).any()
    assert sh.read(0)[3] == 2 and sh.ms() > 0
    # a third batch: the crop call of a fourth comes straight behind the shots call, with other rectangles
    c.detect(buf)
    dst.crop_detections(c.det, buf.ptr, CROP, device=True)
    c.det.track_device(trk, **TRACK_KW)
    call = fetched()
    dst.shots_device(c.det, sh, **KW)
    dst.crop_detections(c.det, buf.ptr, c.opts(max_per_frame=2, expand=1.7), device=True)
    rec = dst.shots_results(sh)
    want = both(gpu, twin, ref, call, "chain 3", **KW)
    assert rec.tobytes() == want.tobytes()
    same_state(sh, ref, "chain 3")
    assert len(dst.roi_results()[0]) == 6 and len(call[1]) == 8             # (the table the shots call read is gone)
    # mars_hip_shots: the enqueue and the fetch in one call, over the new crops; no gates, so every tracked crop takes part
    c.det.track_device(trk, **TRACK_KW)
    rec = dst.shots(c.det, sh, max_gap=2)
    want = both(gpu, twin, ref, fetched(), "chain 4", max_gap=2)                # (6 crops in 8 frames: kept < the batch)
    assert rec.tobytes() == want.tobytes() and sh.read(0)[3] == 4 and [tuple(int(v) for v in r) for r in rec[6:]] == [(0, 0, 0, -1, 0)] * 2
    same_state(sh, ref, "chain 4")
    c.det.pipe_open()
    refused(dst.shots_device, c.det, sh)                                   # an open pipe
    c.det.pipe_close()
    for o in (sh, twin, trk, dst, c):
        o.close()
