"""Tracking on the device (include/mars_hip.h, "Tracking"): mars_yolo_track_lists over stream, step and box counts around the wavefront and the
candidate cap, both frame -> stream maps, the second pass on and off; split invariance; ties; the one-pair-per-round staircase; table
pressure; class gating; the extremes of the arithmetic; and the chain detector -> crops -> classify -> match -> identify -> track over two
batches, with its ordering.  The expected values come from the numpy restatement of tests/test_track_cpu.py (checked there by hand); every
comparison -- outputs, every field of every live state, the four counters -- is bit-exact."""
import numpy as np
import pytest

from test_gpu_gallery import gallery_of, one_round, vectors
from test_gpu_roi import FRAME_SEED, Chain, second_stage
from test_track_cpu import CLS, DET, LOW, SCENE_IDS, SCENE_OPTS, SCENES, SLOTS, F, TrackerNp, box, frames, scene, track_np

pytestmark = pytest.mark.gpu


def same_state(trk, ref, what):
    for b in range(ref.S):
        st, cnt = trk.read(b)
        want, want_cnt = ref.read(b)
        assert cnt.tolist() == want_cnt.tolist(), (what, b, cnt, want_cnt)
        assert st.dtype == want.dtype and st.shape == want.shape, (what, b, st.shape, want.shape)
        assert st.tobytes() == want.tobytes(), (what, b)


def both(gpu, trk, ref, dets, counts, what, idents=None, **kw):
    """the same frames through the device and through the restatement: outputs, states and counters agree to the bit"""
    out = gpu.track_lists(trk, dets, counts, gpu.track_opts(**kw), idents=idents)
    want = track_np(ref, dets, counts, idents=idents, **kw)
    assert out.dtype == want.dtype and out.shape == want.shape, what
    assert out.tobytes() == want.tobytes(), (what, np.argwhere(out != want)[:4])
    same_state(trk, ref, what)
    return out


def pair(gpu, streams):
    return gpu.Tracker(streams), TrackerNp(streams)


@pytest.mark.parametrize("shape", SCENES, ids=SCENE_IDS)
def test_track_lists(gpu, shape):
    streams, steps, boxes, max_det = shape
    for major in (False, True):
        dets, counts = scene(0x7AC0000 + boxes, streams, steps, boxes, max_det, major)
        for low in (LOW, 0.0):
            trk, ref = pair(gpu, streams)
            both(gpu, trk, ref, dets, counts, (shape, major, low), low_conf=low, stream_major=major, **SCENE_OPTS)
            if low and steps >= 3:
                assert min(ref.events.values()) >= 1
            trk.close()


def test_default_options_and_counts_beyond_the_row(gpu):
    """no options at all; a count above max_det is clamped, a negative one reads as an empty frame"""
    dets, counts = scene(0x7AC1000, 2, 3, 7, 8)
    trk, ref = pair(gpu, 2)
    out = gpu.track_lists(trk, dets, counts)
    assert out.tobytes() == track_np(ref, dets, counts).tobytes()
    same_state(trk, ref, "defaults")
    counts = counts.copy()
    counts[0], counts[1] = 1000, -5
    both(gpu, trk, ref, dets, counts, "clamped counts")
    trk.close()


def test_split_invariance_and_reset(gpu):
    """one call over 6 steps == three calls over 2 steps, byte for byte, under both maps; a reset in between starts over"""
    S, T, n = 2, 6, 20
    for major in (False, True):
        dets, counts = scene(0x7AC2000, S, T, n, 32, major)
        kw = dict(low_conf=LOW, stream_major=major, **SCENE_OPTS)
        one, ref = pair(gpu, S)
        whole = both(gpu, one, ref, dets, counts, ("whole", major), **kw)
        three, _ = pair(gpu, S)
        parts = []
        for c in range(3):
            if major:  # a stream's steps 2 c and 2 c + 1, stream by stream
                sel = [b * T + 2 * c + t for b in range(S) for t in range(2)]
            else:
                sel = list(range(2 * c * S, (2 * c + 2) * S))
            parts.append((sel, gpu.track_lists(three, dets[sel], counts[sel], gpu.track_opts(**kw))))
        got = np.zeros_like(whole)
        for sel, o in parts:
            got[sel] = o
        assert got.tobytes() == whole.tobytes()
        for b in range(S):
            assert three.read(b)[0].tobytes() == one.read(b)[0].tobytes() and three.read(b)[1].tolist() == one.read(b)[1].tolist()
        # a reset between the second and the third part: the third part alone on empty tables
        three.reset()
        assert all(len(three.read(b)[0]) == 0 and three.read(b)[1].tolist() == [0, 0, 0, 0] for b in range(S))
        sel = parts[2][0]
        fresh = TrackerNp(S)
        after = gpu.track_lists(three, dets[sel], counts[sel], gpu.track_opts(**kw))
        assert after.tobytes() == track_np(fresh, dets[sel], counts[sel], **kw).tobytes()
        same_state(three, fresh, "after reset")
        assert after.tobytes() != parts[2][1].tobytes() and after["id"].max() < whole["id"].max()  # the ids start over
        one.close()
        three.close()


def test_ties(gpu):
    trk, ref = pair(gpu, 1)
    d, n = frames([box(0)], [box(1), box(1)])
    out = both(gpu, trk, ref, d, n, "duplicate detections")
    assert out[1, :2].tolist() == [(1, 2), (2, 1)]  # the lower index
    trk.reset()
    ref.reset()
    d, n = frames([box(0), box(0)], [box(1)])
    out = both(gpu, trk, ref, d, n, "duplicate tracks")
    assert out[1, 0].tolist() == (1, 2) and trk.read(0)[0]["hits"].tolist() == [2, 1]  # the lower slot
    trk.close()


def test_staircase_one_pair_per_round(gpu):
    """256 tracks and 256 detections on a line, T0 D0 T1 D1 ..., the gaps strictly shrinking: every track prefers the detection on its
    right, every detection the track on ITS right, so only the last pair is mutual -- and once it is gone, only the one before it.  The
    round form resolves one pair per round, 256 rounds; the result is T k <-> D k"""
    gap = F(40) - np.arange(2 * SLOTS, dtype=F) * F(0.05)
    x = np.concatenate([[F(0)], np.cumsum(gap[:-1], dtype=F)]).astype(F)
    d, n = frames([box(float(v), w=100.0, h=100.0) for v in x[0::2]], [box(float(v), w=100.0, h=100.0) for v in x[1::2]], max_det=SLOTS)
    trk, ref = pair(gpu, 1)
    out = both(gpu, trk, ref, d, n, "staircase")
    assert out["id"][1].tolist() == list(range(1, SLOTS + 1)) and (out["hits"][1] == 2).all()
    trk.close()


def test_table_pressure(gpu):
    """300 births into 256 slots: 44 dropped.  After max_miss + 1 empty frames every slot is free and the ids go on from 257"""
    a = [box(20.0 * k, y=0.0) for k in range(150)]
    b = [box(20.0 * k, y=500.0) for k in range(150)]
    d, n = frames(a, b, [], [], [], [box(5.0, y=900.0)], max_det=150)
    trk, ref = pair(gpu, 1)
    both(gpu, trk, ref, d[:2], n[:2], "births", max_miss=2)
    st, cnt = trk.read(0)
    assert len(st) == SLOTS and cnt.tolist() == [256, 0, 0, 44]
    both(gpu, trk, ref, d[2:5], n[2:5], "empty frames", max_miss=2)
    st, cnt = trk.read(0)
    assert len(st) == 0 and cnt.tolist() == [256, 256, 0, 44]
    out = both(gpu, trk, ref, d[5:], n[5:], "the next birth", max_miss=2)
    assert out[0, 0].tolist() == (257, 1) and trk.read(0)[0]["id"].tolist() == [257]
    trk.close()


def test_class_gating(gpu):
    d, n = frames([box(0, cls=1), box(50, cls=2), box(100, cls=4)], [box(1, cls=2), box(51, cls=2), box(101, cls=3)])
    trk, ref = pair(gpu, 1)
    out = both(gpu, trk, ref, d, n, "classes must agree")
    assert out[1, :3].tolist() == [(4, 1), (2, 2), (5, 1)]
    trk.reset()
    ref.reset()
    out = both(gpu, trk, ref, d, n, "any class", any_class=True)
    assert out[1, :3].tolist() == [(1, 2), (2, 2), (3, 2)] and trk.read(0)[0]["cls"].tolist() == [2, 2, 3]
    trk.reset()
    ref.reset()
    out = both(gpu, trk, ref, d, n, "a class window", classes=(2, 2))
    assert out["id"][:, :3].tolist() == [[-1, 1, -1], [2, 1, 3]]
    trk.close()


def test_extremes(gpu):
    """a huge finite box: both areas overflow, uni = inf + inf - inf is a NaN and the comparison fails, so the box never matches its own
    track.  NaN and Inf fields, w <= 0, h <= 0: not a candidate"""
    big = 3e19
    bad = [box(float("nan")), box(0, y=float("inf")), box(0, w=float("-inf")), box(0, w=0.0), box(0, h=-1.0), box(0, conf=float("nan")),
           box(0, conf=float("inf"))]
    d, n = frames([box(0, w=big, h=big), box(7)] + bad, [box(0, w=big, h=big), box(8)] + bad, max_det=16)
    trk, ref = pair(gpu, 1)
    out = both(gpu, trk, ref, d, n, "extremes", low_conf=0.1)
    assert out["id"][0, :9].tolist() == [1, 2] + [-1] * 7 and out[1, :2].tolist() == [(3, 1), (2, 2)]
    # a track whose state leaves the finite range stays harmless: x = 1e38, 2e38 gives vx = 1e38
    wide = dict(w=3e38, h=1e-3)
    d, n = frames([box(1e38, **wide)], [box(2e38, **wide)], [box(3e38, **wide)], [], [box(3e38, **wide)])
    trk.reset()
    ref.reset()
    out = both(gpu, trk, ref, d, n, "overflowing state")
    # (step 2: the prediction 3e38 has the corner 4.5e38 = inf on both boxes, inter = inf, uni = NaN: no match, the track coasts to x = inf)
    assert [out[f, 0].tolist() for f in (0, 1, 2, 4)] == [(1, 1), (1, 2), (2, 1), (3, 1)] and np.isinf(trk.read(0)[0]["x"][0])
    trk.close()


def test_lifecycle_and_refusals_on_the_device(gpu):
    BAD_FILE, BAD_TENSOR = gpu.MARS_ERR_INVALID_FILE, gpu.MARS_ERR_INVALID_TENSOR

    def refused(code, fn, *a, **kw):
        with pytest.raises(gpu.MarsError) as ei:
            fn(*a, **kw)
        assert ei.value.code == code

    trk = gpu.Tracker(3)
    d, n = frames([box(0)], [box(1)], [box(2)], [box(3)])
    refused(BAD_TENSOR, gpu.track_lists, trk, d, n)          # 4 frames, 3 streams
    refused(BAD_TENSOR, trk.read, 3)
    refused(BAD_FILE, gpu.track_lists, trk, d[:3], n[:3], gpu.track_opts(carry_identity=True))
    refused(BAD_FILE, gpu.track_lists, trk, d[:3], n[:3], gpu.track_opts(low_conf=0.5))
    assert all(len(trk.read(b)[0]) == 0 for b in range(3))   # nothing moved
    trk.close()
    trk.close()


# ---- the chain ---------------------------------------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def chain(gpu):
    d2, tin, tout, nhwc = second_stage(gpu, "shipped")
    c = Chain(gpu)
    dst = gpu.Model(d2, batch=8)
    gal = vectors(0x6A190000, 50, 64, shift=9) + 40000
    g, ids = gallery_of(gpu, gal, ids=np.arange(50) + 1000)
    yield c, dst, g
    g.close()
    dst.close()
    c.close()


def lists_of(dets):
    d = np.zeros((len(dets), 1000), dtype=DET)
    for f, x in enumerate(dets):
        d[f, :len(x)] = x
    return d, np.array([len(x) for x in dets], dtype=np.int32)


def test_chain_tracks(gpu, chain):
    """detector -> crops -> classify -> match -> identify -> track_device over two batches of the same frames, S = batch: the second batch's
    boxes keep the ids the first gave them, the carried identities are those of the restatement fed the fetched lists, and the bytes do
    not depend on whether the host waited in between"""
    c, dst, g = chain
    S = c.det.batch
    nv, buf = c.frames(FRAME_SEED)
    trk, ref = gpu.Tracker(S), TrackerNp(S)
    with pytest.raises(gpu.MarsError) as ei:
        c.det.track_results()  # nothing pending
    assert ei.value.code == gpu.MARS_ERR_INVALID_TENSOR
    one_round(c, dst, g, buf)
    with pytest.raises(gpu.MarsError) as ei:
        c.det.track_device(trk, carry_identity=True)  # no identity results yet
    assert ei.value.code == gpu.MARS_ERR_INVALID_TENSOR
    two = gpu.Tracker(2)
    with pytest.raises(gpu.MarsError) as ei:
        c.det.track_device(two)  # 3 frames, 2 streams
    assert ei.value.code == gpu.MARS_ERR_INVALID_TENSOR
    two.close()
    got = []
    for r in range(2):  # with a wait between the detection tail and the tracker
        if r:
            one_round(c, dst, g, buf)
        c.det.identify_detections(dst)
        dets = c.det.detect_results()
        if not r:  # thresholds inside the detector's own confidences: the upper half is the high set, the quarter below it the low set
            conf = np.sort(np.concatenate([x["conf"] for x in dets]))
            TRACK_KW = dict(min_conf=float(conf[len(conf) // 2]), low_conf=float(conf[len(conf) // 4]), carry_identity=True)
            assert 0 < TRACK_KW["low_conf"] < TRACK_KW["min_conf"] <= 1
        c.det.track_device(trk, **TRACK_KW)
        tracks, idents = c.det.track_results(), c.det.identity_results()
        d, n = lists_of(dets)
        want = track_np(ref, d, n, idents=idents, **TRACK_KW)
        assert tracks.tobytes() == want.tobytes(), r
        same_state(trk, ref, ("chain", r))
        got.append((dets, tracks))
    (dets0, t0), (dets1, t1) = got
    assert all(a.tobytes() == b.tobytes() for a, b in zip(dets0, dets1))  # the same frames: every box persists
    born = t0["id"] > 0
    assert born.sum() >= 8 and (t0["hits"][born] == 1).all()
    assert (t1["id"][born] == t0["id"][born]).all() and (t1["hits"][born] == 2).all()  # ... and keeps its id
    states = np.concatenate([trk.read(b)[0] for b in range(S)])
    assert (states["ident"]["cls"] >= 1000).sum() >= 1 and (states["ident"]["cls"] < 0).sum() >= 1  # some tracks carry an identity
    assert ref.events["match2"] >= 0 and ref.events["match1"] >= 8
    mid = [trk.read(b) for b in range(S)]
    # the same two batches with nothing waiting in between
    trk.reset()
    for r in range(2):
        one_round(c, dst, g, buf)
        c.det.identify_detections(dst)
        c.det.track_device(trk, **TRACK_KW)
    assert c.det.track_results().tobytes() == t1.tobytes()
    for b in range(S):
        assert trk.read(b)[0].tobytes() == mid[b][0].tobytes() and trk.read(b)[1].tolist() == mid[b][1].tolist()
    # mars_hip_track: the enqueue and the fetch in one call, a third step of the same boxes
    one_round(c, dst, g, buf)
    c.det.identify_detections(dst)
    t2 = c.det.track(trk, **TRACK_KW)
    assert (t2["id"][born] == t0["id"][born]).all() and (t2["hits"][born] == 3).all()
    c.det.pipe_open()
    with pytest.raises(gpu.MarsError) as ei:
        c.det.track_device(trk)  # an open pipe
    assert ei.value.code == gpu.MARS_ERR_INVALID_TENSOR
    c.det.pipe_close()
    trk.close()
