"""Events on the device (include/mars_hip.h, "Events"): mars_yolo_event_lists over the stream and step counts of tests/eventref.py in both
frame orders, split invariance, reset and a change of rules in mid-stream, the case tables (table pressure, overflow, duplicates, gaps, dwell,
min_hits, 32 lines and 32 zones, entries that take no part), the refusals that need a device, and the chain detector -> track_device ->
events_device over two batches with its ordering.  The expected values come from the restatement in Python integers of tests/eventref.py
(checked by hand in tests/test_events_cpu.py); every comparison -- records, per-frame counts, totals, counters, step and the table -- is
byte for byte."""
import numpy as np
import pytest

import eventref as R
from test_gpu_roi import FRAME_SEED, Chain

pytestmark = pytest.mark.gpu


def same_state(ev, ref, what):
    for b in range(ref.S):
        got, want = ev.read(b), ref.read(b)
        for k in range(3):
            assert got[k].dtype == want[k].dtype and got[k].tobytes() == want[k].tobytes(), (what, b, k, got[k], want[k])
        assert got[3:] == want[3:], (what, b, got[3:], want[3:])
        slots, wslots = ev.read_slots(b), ref.read_slots(b)
        assert slots.dtype == wslots.dtype and slots.tobytes() == wslots.tobytes(), (what, b, np.flatnonzero(slots != wslots)[:4])


def both(gpu, ev, ref, d, t, n, what, **kw):
    """the same frames through the device and through the restatement: records, counts and state agree to the byte"""
    out = gpu.event_lists(ev, d, t, n, gpu.event_opts(**kw))
    want = ref.run(d, t, n, **kw)
    for k in range(3):
        assert out[k].dtype == want[k].dtype and out[k].shape == want[k].shape, (what, k)
        assert out[k].tobytes() == want[k].tobytes(), (what, k, np.argwhere(out[k] != want[k])[:4])
    same_state(ev, ref, what)
    return out


def pair(gpu, streams, rules):
    ev, ref = gpu.Events(streams), R.EventsNp(streams)
    ev.set_rules(gpu.event_rules(rules.lines, rules.zones))
    ref.set_rules(rules)
    return ev, ref


@pytest.mark.parametrize("shape", R.SHAPES, ids=["S%d-T%d%s" % (s, t, "-major" if m else "") for s, t, m in R.SHAPES])
def test_event_lists(gpu, shape):
    S, T, major = shape
    d, t, n = R.scene(0xE7E0000 + 16 * S + T, S, T, 12, 16, major)
    ev, ref = pair(gpu, S, R.RULES3)
    both(gpu, ev, ref, d, t, n, shape, max_gap=1, stream_major=major)
    assert ev.ms() > 0
    ev.close()
    ev.close()


def test_default_options_and_no_rules(gpu):
    """no options and an object without rules: slots are taken and expire, nothing else"""
    d, t, n = R.scene(0xE7E1000, 2, 3, 7, 9)
    ev, ref = gpu.Events(2), R.EventsNp(2)
    out = gpu.event_lists(ev, d, t, n)
    want = ref.run(d, t, n)
    assert all(a.tobytes() == b.tobytes() for a, b in zip(out, want)) and not out[0].view(np.uint32).any()
    same_state(ev, ref, "no rules")
    assert ev.read(0)[2][0] >= 7
    ev.close()


def test_split_invariance_reset_and_new_rules(gpu):
    """one call over 6 steps == three calls over 2 steps, byte for byte, under both maps; a reset of one stream starts that stream over and
    keeps its rules; new rules on one stream reset it and leave the others alone"""
    S, T = 2, 6
    for major in (False, True):
        d, t, n = R.scene(0xE7E2000, S, T, 10, 12, major)
        kw = dict(max_gap=1, stream_major=major)
        one, ref = pair(gpu, S, R.RULES3)
        whole = both(gpu, one, ref, d, t, n, ("whole", major), **kw)
        three, ref3 = pair(gpu, S, R.RULES3)
        got = [np.zeros_like(a) for a in whole]
        sels = []
        for c in range(3):
            sel = [b * T + 2 * c + s for b in range(S) for s in range(2)] if major else list(range(2 * c * S, (2 * c + 2) * S))
            sels.append(sel)
            part = both(gpu, three, ref3, d[sel], t[sel], n[sel], ("part", major, c), **kw)
            for k in range(3):
                got[k][sel] = part[k]
        assert all(a.tobytes() == b.tobytes() for a, b in zip(got, whole))
        for b in range(S):
            assert three.read_slots(b).tobytes() == one.read_slots(b).tobytes()
            assert all(np.array_equal(x, y) for x, y in zip(three.read(b), one.read(b)))
        # stream 1 reset: the last part again, stream 0 going on and stream 1 on an empty table with its rules
        three.reset(1)
        ref3.reset(1)
        assert three.read(1)[3:] == (0, 0) and not three.read(1)[2].any() and three.read(0)[4] == T
        same_state(three, ref3, "after reset")
        both(gpu, three, ref3, d[sels[2]], t[sels[2]], n[sels[2]], ("after reset", major), **kw)
        assert three.read(1)[4] == 2 and three.read(0)[4] == T + 2
        # new rules on stream 0 in mid-stream: it starts over under them, stream 1 keeps table, step and rules
        flipped = R.Rules([(ax, by, bx, ay) for ax, ay, bx, by in R.RULES3.lines], [R.RULES3.zones[1]])
        three.set_rules(gpu.event_rules(flipped.lines, flipped.zones), 0)
        ref3.set_rules(flipped, 0)
        same_state(three, ref3, "new rules")
        assert three.read(0)[3:] == (0, 0) and three.read(1)[4] == 2
        both(gpu, three, ref3, d[sels[0]], t[sels[0]], n[sels[0]], ("new rules", major), **kw)
        one.close()
        three.close()


@pytest.mark.parametrize("name", sorted(R.CASES))
def test_case(gpu, name):
    S, rules, calls, need = R.CASES[name]()
    ev, ref = pair(gpu, S, rules)
    outs = [both(gpu, ev, ref, d, t, n, (name, c), **kw) for c, (d, t, n, kw) in enumerate(calls)]
    sm = R.summary(ref, outs)  # (of the device's outputs and the restatement's state, which are the device's)
    assert all(sm[k] >= 1 for k in need), (name, sm)
    if name == "pressure":
        assert ev.read_slots(0)[0]["id"] == 257 and ev.read(0)[2].tolist() == [257, 1, 0, 1, 0]
    ev.close()


def test_refusals_on_the_device(gpu):
    FILE, TENSOR = gpu.MARS_ERR_INVALID_FILE, gpu.MARS_ERR_INVALID_TENSOR

    def refused(code, fn, *a, **kw):
        with pytest.raises(gpu.MarsError) as ei:
            fn(*a, **kw)
        assert ei.value.code == code

    ev, ref = pair(gpu, 3, R.RULES3)
    d, t, n = R.scene(0xE7E3000, 3, 1, 5, 8)
    both(gpu, ev, ref, d, t, n, "before")
    d4, t4, n4 = R.scene(0xE7E3001, 4, 1, 5, 8)
    refused(TENSOR, gpu.event_lists, ev, d4, t4, n4)                       # 4 frames, 3 streams
    refused(TENSOR, ev.read, 3)
    refused(TENSOR, ev.reset, 3)
    refused(TENSOR, ev.set_rules, gpu.event_rules(), 5)
    refused(FILE, ev.set_rules, gpu.event_rules([(1, 1, 1, 1)]), 0)
    refused(FILE, ev.set_rules, gpu.event_rules(zones=[[(0, 0), (40000, 0), (0, 9)]]), -1)
    refused(FILE, gpu.event_lists, ev, d, t, n, gpu.event_opts(flags=8))
    refused(FILE, gpu.event_lists, ev, d, t, n, gpu.event_opts(max_gap=-2))
    same_state(ev, ref, "nothing moved")
    ev.close()


# ---- the chain ---------------------------------------------------------------------------------------------------------------------------
def lists_of(dets):
    d = np.zeros((len(dets), 1000), dtype=R.DET)
    for f, x in enumerate(dets):
        d[f, :len(x)] = x
    return d, np.array([len(x) for x in dets], dtype=np.int32)


def test_chain_events(gpu):
    """detector -> track_device -> events_device over two batches of the same frames, S = batch: the bytes equal the restatement fed the
    fetched detections and tracks and do not depend on whether the host waited in between.  The rules are placed from the fetched boxes: a
    zone around a tracked box of every frame, a line beside it"""
    c = Chain(gpu)
    S = c.det.batch
    _, buf = c.frames(FRAME_SEED)
    trk, ev = gpu.Tracker(S), gpu.Events(S)
    refused = []
    with pytest.raises(gpu.MarsError) as ei:
        c.det.events_results(ev)  # nothing pending
    refused.append(ei.value.code)
    c.detect(buf)
    with pytest.raises(gpu.MarsError) as ei:
        c.det.events_device(ev)  # no track results yet
    refused.append(ei.value.code)
    dets = c.det.detect_results()
    conf = np.sort(np.concatenate([x["conf"] for x in dets]))
    TRACK_KW = dict(min_conf=float(conf[len(conf) // 2]))
    c.det.track_device(trk, **TRACK_KW)
    two = gpu.Events(2)
    with pytest.raises(gpu.MarsError) as ei:
        c.det.events_device(two)  # 3 frames, 2 streams
    refused.append(ei.value.code)
    two.close()
    assert refused == [gpu.MARS_ERR_INVALID_TENSOR] * 3
    # the rules, per stream, from the first batch's boxes: a square of 17 pixels around the first tracked box (the box sits still, so the
    # zone is occupied in both batches and its dwell of 1 fires in the second), and a gate 3 pixels to its right
    tracks = c.det.track_results()
    d, n = lists_of(dets)
    ref = R.EventsNp(S)
    for b in range(S):
        i = int(np.flatnonzero(tracks[b]["id"] >= 1)[0])
        x, y = int(np.floor(d[b, i]["x"])), int(np.floor(d[b, i]["y"]))
        rules = R.Rules([(x + 3, y - 50, x + 3, y + 50)], [([(x - 8, y - 8), (x + 9, y - 8), (x + 9, y + 9), (x - 8, y + 9)], 1)])
        ev.set_rules(gpu.event_rules(rules.lines, rules.zones), b)
        ref.set_rules(rules, b)
    trk.reset()
    got = []
    for r in range(2):  # with a wait between every stage
        c.detect(buf)
        dets = c.det.detect_results()
        c.det.track_device(trk, **TRACK_KW)
        tracks = c.det.track_results()
        c.det.events_device(ev)
        out = c.det.events_results(ev)
        d, n = lists_of(dets)
        want = ref.run(d, tracks, n)
        assert all(a.tobytes() == w.tobytes() for a, w in zip(out, want)), r
        same_state(ev, ref, ("chain", r))
        got.append(out)
    (rec0, _, zc0), (rec1, _, zc1) = got
    assert (zc0[:, 0, 0] >= 1).all() and (zc1[:, 0, 0] >= 1).all()      # every stream's zone is occupied
    assert (zc1[:, 0, 3] >= 1).all() and not rec0["dwelled"].any()         # ... and its dwell fires in the second batch
    assert ev.read(0)[2][0] >= 3 and ev.read(0)[4] == 2
    mid = [(ev.read(b), ev.read_slots(b)) for b in range(S)]
    # the same two batches with nothing waiting in between
    trk.reset()
    ev.reset()
    for r in range(2):
        c.detect(buf)
        c.det.track_device(trk, **TRACK_KW)
        c.det.events_device(ev)
    out = c.det.events_results(ev)
    assert all(a.tobytes() == w.tobytes() for a, w in zip(out, got[1]))
    for b in range(S):
        assert ev.read_slots(b).tobytes() == mid[b][1].tobytes() and all(np.array_equal(x, y) for x, y in zip(ev.read(b), mid[b][0]))
    # mars_hip_events: the enqueue and the fetch in one call, a third step of the same boxes
    c.detect(buf)
    c.det.track_device(trk, **TRACK_KW)
    rec2, _, zc2 = c.det.events(ev, max_gap=5)
    assert rec2["zones"].tobytes() == rec1["zones"].tobytes() and not rec2["entered"].any() and ev.read(0)[4] == 3
    c.det.pipe_open()
    with pytest.raises(gpu.MarsError) as ei:
        c.det.events_device(ev)  # an open pipe
    assert ei.value.code == gpu.MARS_ERR_INVALID_TENSOR
    c.det.pipe_close()
    ev.close()
    trk.close()
    c.close()
