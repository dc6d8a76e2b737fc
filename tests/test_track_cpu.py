"""Tracking (include/mars_hip.h, "Tracking"), the part that needs no GPU: the entry points are exported, the three structs match their ctypes
mirrors, arguments that can never be valid are refused up front, and the numpy restatement that tests/test_gpu_track.py compares the device
against is itself checked on cases worked out by hand.  The restatement's matching is the literal sorted walk of the header, not the rounds
the kernel runs."""
import ctypes as C
import struct

import numpy as np
import pytest

import cases

F = np.float32
DET = np.dtype([("x", "<f4"), ("y", "<f4"), ("w", "<f4"), ("h", "<f4"), ("conf", "<f4"), ("cls", "<i4")])  # mars_det_t
CLS = np.dtype([("cls", "<i4"), ("score", "<f4")])                                                          # mars_cls_t
TRACK = np.dtype([("id", "<i4"), ("hits", "<i4")])                                                          # mars_track_t
STATE = np.dtype([("id", "<i4"), ("cls", "<i4"), ("hits", "<i4"), ("miss", "<i4"), ("x", "<f4"), ("y", "<f4"), ("w", "<f4"), ("h", "<f4"),
                  ("vx", "<f4"), ("vy", "<f4"), ("ident", CLS)])                                            # mars_track_state_t
SLOTS = MAX_CAND = 256
NEW = ["mars_hip_tracker_create", "mars_hip_tracker_reset", "mars_hip_tracker_free", "mars_hip_tracker_read", "mars_yolo_track_lists",
       "mars_hip_track_device", "mars_hip_track_results", "mars_hip_track"]


# ---- the numpy restatement (Python integers, float32 steps rounded one by one) -----------------------------------------------------------
def iou_np(ax, ay, aw, ah, bx, by, bw, bh):
    """the NMS kernel's expression on float32 scalars or arrays (element by element, every operation rounded on its own); np.fmax and
    np.fmin are C's fmaxf and fminf"""
    with np.errstate(all="ignore"):
        two = F(2)
        ax1, ay1, ax2, ay2 = ax - aw / two, ay - ah / two, ax + aw / two, ay + ah / two
        x1 = np.fmax(ax1, bx - bw / two)
        y1 = np.fmax(ay1, by - bh / two)
        x2 = np.fmin(ax2, bx + bw / two)
        y2 = np.fmin(ay2, by + bh / two)
        iw, ih = np.fmax(F(0), x2 - x1), np.fmax(F(0), y2 - y1)
        inter = iw * ih
        uni = aw * ah + bw * bh
        uni = uni - inter
        uni = uni + F(1e-6)
        return inter / uni


class TrackerNp:
    """the tables of S streams: slots[b][s] = None or a dict of the state's fields (Python ints, np.float32 scalars)"""

    def __init__(self, streams):
        self.S = streams
        self.reset()

    def reset(self):
        self.slots = [[None] * SLOTS for _ in range(self.S)]
        self.next_id = [1] * self.S
        self.counters = [[0, 0, 0, 0] for _ in range(self.S)]  # births, deaths, overflow, dropped
        self.events = dict(match1=0, match2=0, birth=0, death=0, reuse=0)
        self.used = [set() for _ in range(self.S)]

    def read(self, stream):
        live = [t for t in self.slots[stream] if t is not None]
        out = np.zeros(len(live), dtype=STATE)
        for k, t in enumerate(live):
            out[k] = (t["id"], t["cls"], t["hits"], t["miss"], t["x"], t["y"], t["w"], t["h"], t["vx"], t["vy"], (t["icls"], t["iscore"]))
        return out, np.array(self.counters[stream], dtype=np.int64)


def _associate(slots, tracks, cand, d, thresh, any_class, taken):
    """greedy on (iou descending, slot ascending, detection ascending): tracks = free slots, cand = detection indices -> {slot: detection}"""
    if not tracks or not cand:
        return {}
    a = [np.array([slots[s][k] for s in tracks], dtype=F)[:, None] for k in ("px", "py", "w", "h")]
    b = [d[k][cand].astype(F)[None, :] for k in ("x", "y", "w", "h")]
    iou = iou_np(*a, *b)
    pairs = []
    for r, s in enumerate(tracks):
        for c, i in enumerate(cand):
            if (any_class or slots[s]["cls"] == int(d["cls"][i])) and iou[r, c] >= thresh:  # a NaN fails the comparison
                pairs.append((-float(iou[r, c]), s, i))
    got = {}
    for _, s, i in sorted(pairs):
        if s not in got and i not in taken:
            got[s] = i
            taken.add(i)
    return got


def track_np(trk, dets, counts, idents=None, min_conf=0.0, low_conf=0.0, iou_thresh=0.0, iou_thresh_low=0.0, max_miss=0, classes=None,
             any_class=False, carry_identity=False, stream_major=False):
    """dets = DET [F][max_det], counts [F], idents = None or CLS [F][max_det]; moves trk on by these frames -> TRACK [F][max_det]"""
    dets = np.asarray(dets, dtype=DET)
    nf, max_det = dets.shape
    S = trk.S
    assert nf % S == 0
    T = nf // S
    min_conf = F(min_conf) if min_conf else F(0.5)
    low_conf = F(low_conf)
    thr1 = F(iou_thresh) if iou_thresh else F(0.3)
    thr2 = F(iou_thresh_low) if iou_thresh_low else F(0.5)
    max_miss = max_miss if max_miss else 30
    first, count = classes if classes else (0, 0)
    out = np.zeros((nf, max_det), dtype=TRACK)
    out["id"] = -1
    for b in range(S):
        slots = trk.slots[b]
        for t in range(T):
            f = b * T + t if stream_major else t * S + b
            d = dets[f]
            n = min(max(int(counts[f]), 0), max_det)
            H, L = [], []
            for i in range(n):
                v = d[i]
                if not all(np.isfinite(v[k]) for k in ("x", "y", "w", "h", "conf")) or not v["w"] > 0 or not v["h"] > 0:
                    continue
                if count and not first <= int(v["cls"]) < first + count:
                    continue
                if v["conf"] >= min_conf:
                    H.append(i)
                elif low_conf > 0 and v["conf"] >= low_conf:
                    L.append(i)
            trk.counters[b][2] += max(len(H) - MAX_CAND, 0) + max(len(L) - MAX_CAND, 0)
            H, L = H[:MAX_CAND], L[:MAX_CAND]
            live = [s for s in range(SLOTS) if slots[s] is not None]
            with np.errstate(all="ignore"):
                for s in live:
                    slots[s]["px"] = F(slots[s]["x"] + slots[s]["vx"])
                    slots[s]["py"] = F(slots[s]["y"] + slots[s]["vy"])
            taken = set()
            got = _associate(slots, live, H, d, thr1, any_class, taken)
            trk.events["match1"] += len(got)
            if low_conf > 0:
                got2 = _associate(slots, [s for s in live if s not in got], L, d, thr2, any_class, taken)
                trk.events["match2"] += len(got2)
                got.update(got2)
            for s in live:
                k = slots[s]
                if s in got:
                    i = got[s]
                    v = d[i]
                    with np.errstate(all="ignore"):
                        dx, dy = F(v["x"] - k["x"]), F(v["y"] - k["y"])
                        if k["hits"] == 1:
                            k["vx"], k["vy"] = dx, dy
                        else:
                            k["vx"], k["vy"] = F(F(k["vx"] + dx) * F(0.5)), F(F(k["vy"] + dy) * F(0.5))
                    k["x"], k["y"], k["w"], k["h"], k["cls"] = v["x"], v["y"], v["w"], v["h"], int(v["cls"])
                    k["hits"] += 1
                    k["miss"] = 0
                    if carry_identity:
                        e = idents[f][i]
                        if e["cls"] >= 0 and (k["icls"] < 0 or e["score"] >= k["iscore"]):
                            k["icls"], k["iscore"] = int(e["cls"]), e["score"]
                    out[f, i] = (k["id"], k["hits"])
                else:
                    k["x"], k["y"] = k["px"], k["py"]
                    k["miss"] += 1
                    if k["miss"] > max_miss:
                        slots[s] = None
                        trk.counters[b][1] += 1
                        trk.events["death"] += 1
            for i in H:
                if i in taken:
                    continue
                free = [s for s in range(SLOTS) if slots[s] is None]
                if not free:
                    trk.counters[b][3] += 1
                    continue
                v = d[i]
                e = idents[f][i] if carry_identity else (-1, F(0))
                slots[free[0]] = dict(id=trk.next_id[b], cls=int(v["cls"]), hits=1, miss=0, x=v["x"], y=v["y"], w=v["w"], h=v["h"], vx=F(0), vy=F(0),
                                      icls=int(e[0]), iscore=F(e[1]))
                out[f, i] = (trk.next_id[b], 1)
                trk.next_id[b] += 1
                trk.counters[b][0] += 1
                trk.events["birth"] += 1
                trk.events["reuse"] += free[0] in trk.used[b]
                trk.used[b].add(free[0])
    return out


# ---- the scenes the GPU test uses --------------------------------------------------------------------------------------------------------
# (streams, steps, boxes per frame, max_det)
SCENES = [(1, 1, 0, 8), (1, 1, 1, 8), (1, 5, 7, 8), (3, 5, 7, 1000), (3, 4, 65, 300), (1, 3, 257, 300), (2, 3, 300, 1000)]
SCENE_OPTS = dict(max_miss=1)
LOW = 0.2


def scene(seed, streams, steps, boxes, max_det, stream_major=False):
    """boxes on random walks, drawn with cases.f32: -> (DET [streams * steps][max_det], counts).  Step 0 lists all `boxes` objects of the
    stream with a high confidence.  The objects with k % 5 == 0 are missing in step 1 and come back from step 2 on 3000 pixels away: the old
    track coasts and dies (max_miss = 1), the box far away is born into a slot a death freed.  From step 1 on the objects with k % 4 == 2
    come with a confidence between LOW and the default min_conf (pass 2) and those with k % 7 == 3 with one below LOW (not a candidate).
    The list is rotated by 3 places per step"""
    nf = streams * steps
    dets = np.zeros((nf, max_det), dtype=DET)
    counts = np.zeros(nf, dtype=np.int32)
    for b in range(streams):
        s0 = seed + 0x1000 * b
        if boxes == 0:
            continue
        pos = cases.f32(s0 + 1, 2 * boxes, 50.0, 950.0).reshape(boxes, 2).copy()
        size = cases.f32(s0 + 2, 2 * boxes, 40.0, 80.0).reshape(boxes, 2)
        cls = cases.i8(s0 + 3, boxes).astype(np.int32) % 3
        for t in range(steps):
            if t:
                pos = (pos + cases.f32(s0 + 16 + t, 2 * boxes, -3.0, 3.0).reshape(boxes, 2)).astype(F)
            conf = cases.f32(s0 + 64 + t, boxes, 0.6, 1.0)
            rows = []
            for k in range(boxes):
                p = pos[k]
                if k % 5 == 0 and t == 1:
                    continue
                if k % 5 == 0 and t >= 2:
                    p = p + np.array([3000, 0], dtype=F)
                c = conf[k]
                if t >= 1 and k % 4 == 2:
                    c = F(0.25) + (c - F(0.6)) * F(0.5)  # 0.25 .. 0.45
                elif t >= 1 and k % 7 == 3:
                    c = F(0.1)
                rows.append((p[0], p[1], size[k, 0], size[k, 1], c, cls[k]))
            rows = rows[(3 * t) % max(len(rows), 1):] + rows[:(3 * t) % max(len(rows), 1)]
            f = b * steps + t if stream_major else t * streams + b
            assert len(rows) <= max_det
            counts[f] = len(rows)
            dets[f, :len(rows)] = np.array(rows, dtype=DET)
    return dets, counts


SCENE_IDS = ["s%d_t%d_n%d_w%d" % s for s in SCENES]


@pytest.mark.parametrize("shape", SCENES, ids=SCENE_IDS)
def test_scenes_contain_every_event(shape):
    """what keeps the GPU comparison from being vacuous: on the expected output of every scene that runs long enough for it (three steps or
    more) there is a match in pass 1, a match in pass 2, a birth, a death and a slot reused; the scenes above the cap overflow"""
    streams, steps, boxes, max_det = shape
    for major in (False, True):
        dets, counts = scene(0x7AC0000 + boxes, streams, steps, boxes, max_det, major)
        trk = TrackerNp(streams)
        out = track_np(trk, dets, counts, low_conf=LOW, stream_major=major, **SCENE_OPTS)
        assert out.shape == (streams * steps, max_det) and counts[0] == boxes
        assert trk.events["birth"] >= min(boxes, 1) * streams
        if steps >= 3:
            for what in ("match1", "match2", "birth", "death", "reuse"):
                assert trk.events[what] >= 1, (what, trk.events)
            for b in range(streams):
                assert trk.counters[b][0] >= 1 and trk.counters[b][1] >= 1
        if boxes > MAX_CAND:
            assert all(c[2] >= boxes - MAX_CAND for c in trk.counters)
        off = TrackerNp(streams)
        track_np(off, dets, counts, stream_major=major, **SCENE_OPTS)
        assert off.events["match2"] == 0
        if steps >= 3:
            assert off.events["match1"] < trk.events["match1"] + trk.events["match2"]  # the second pass changes the result


# ---- exports, sizes ----------------------------------------------------------------------------------------------------------------------
def test_track_symbols_are_exported(marsrt):
    L = marsrt.lib()
    for n in NEW:
        assert n in marsrt.EXPORTS["mars_hip.h"], n
        assert hasattr(L, n), n
    for f in (marsrt.Tracker, marsrt.Tracker.reset, marsrt.Tracker.read, marsrt.Tracker.close, marsrt.track_lists, marsrt.track_opts,
              marsrt.Model.track_device, marsrt.Model.track_results, marsrt.Model.track):
        assert callable(f)
    assert marsrt.TRACK_DTYPE == TRACK and marsrt.TRACK_STATE_DTYPE == STATE and marsrt.DET_DTYPE == DET and marsrt.CLS_DTYPE == CLS


def test_track_struct_layouts(marsrt, tmp_path):
    import os
    import subprocess
    O, S, T = marsrt.TrackOpts, marsrt.TrackState, marsrt.TrackRec
    of = ["min_conf", "low_conf", "iou_thresh", "iou_thresh_low", "max_miss", "cls_first", "cls_count", "flags"]
    sf = ["id", "cls", "hits", "miss", "x", "y", "w", "h", "vx", "vy", "ident"]
    assert [f[0] for f in O._fields_] == of and [f[0] for f in S._fields_] == sf and [f[0] for f in T._fields_] == ["id", "hits"]
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    items = (["sizeof(mars_hip_track_opts_t)"] + ["offsetof(mars_hip_track_opts_t, %s)" % f for f in of] + ["sizeof(mars_track_state_t)"] +
             ["offsetof(mars_track_state_t, %s)" % f for f in sf] + ["sizeof(mars_track_t)", "offsetof(mars_track_t, id)", "offsetof(mars_track_t, hits)"] +
             ["(size_t)MARS_TRACK_SLOTS", "(size_t)MARS_TRACK_MAX_CAND", "(size_t)MARS_TRACK_ANY_CLASS", "(size_t)MARS_TRACK_CARRY_IDENTITY",
              "(size_t)MARS_TRACK_STREAM_MAJOR"])
    src = tmp_path / "track_abi.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "mars_hip.h"\nint main(void){ size_t v[] = {%s};\n'
                   ' for (size_t i = 0; i < sizeof(v) / sizeof(v[0]); i++) printf("%%zu ", v[i]); return 0; }\n' % ", ".join(items))
    exe = tmp_path / "track_abi"
    subprocess.run(["gcc", "-I", os.path.join(root, "include"), str(src), "-o", str(exe)], check=True)
    got = [int(x) for x in subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.split()]
    want = ([C.sizeof(O)] + [getattr(O, f).offset for f in of] + [C.sizeof(S)] + [getattr(S, f).offset for f in sf] + [C.sizeof(T), T.id.offset, T.hits.offset] +
            [marsrt.TRACK_SLOTS, marsrt.TRACK_MAX_CAND, marsrt.TRACK_ANY_CLASS, marsrt.TRACK_CARRY_IDENTITY, marsrt.TRACK_STREAM_MAJOR])
    assert got == want
    assert C.sizeof(T) == 8 and C.sizeof(S) == 48 and STATE.itemsize == 48 and [STATE.fields[f][1] for f in sf] == [getattr(S, f).offset for f in sf]
    assert (marsrt.TRACK_SLOTS, marsrt.TRACK_MAX_CAND) == (SLOTS, MAX_CAND)


# ---- the restatement itself, by hand -----------------------------------------------------------------------------------------------------
def frames(*lists, max_det=8):
    """lists of (x, y, w, h, conf, cls) -> (DET [len][max_det], counts)"""
    d = np.zeros((len(lists), max_det), dtype=DET)
    for f, rows in enumerate(lists):
        if rows:
            d[f, :len(rows)] = np.array(rows, dtype=DET)
    return d, np.array([len(r) for r in lists], dtype=np.int32)


def box(x, y=0.0, w=10.0, h=10.0, conf=0.9, cls=0):
    return (x, y, w, h, conf, cls)


def test_restated_iou_by_hand():
    # two 10 x 10 boxes 2 apart: inter = 8 * 10, uni = 200 - 80 + 1e-6
    assert iou_np(F(0), F(0), F(10), F(10), F(2), F(0), F(10), F(10)) == F(F(80) / F(F(120) + F(1e-6)))
    assert iou_np(F(0), F(0), F(10), F(10), F(20), F(0), F(10), F(10)) == 0
    big = F(3e19)
    assert np.isnan(iou_np(F(0), F(0), big, big, F(0), F(0), big, big))  # inf + inf - inf


def test_greedy_not_optimal():
    """tracks A at 0 and B at 5; detections D0 at 2 and D1 at -4 (10 x 10 boxes: iou of an offset g is (10 - g) / (10 + g)).  A-D0 8 / 12,
    B-D0 7 / 13, A-D1 6 / 14, B-D1 1 / 19 (below 0.3).  Greedy takes A-D0 first: B stays unmatched and D1 is born.  The optimal assignment
    (A-D1, B-D0) would have matched both"""
    trk = TrackerNp(1)
    d, n = frames([box(0), box(5)], [box(2), box(-4)])
    out = track_np(trk, d, n)
    assert out[0, :2].tolist() == [(1, 1), (2, 1)] and out[1, :2].tolist() == [(1, 2), (3, 1)] and (out["id"][:, 2:] == -1).all() and (out["hits"][:, 2:] == 0).all()
    st, cnt = trk.read(0)
    assert st["id"].tolist() == [1, 2, 3] and st["miss"].tolist() == [0, 1, 0] and st["x"].tolist() == [2, 5, -4] and cnt.tolist() == [3, 0, 0, 0]
    assert st["vx"].tolist() == [2, 0, 0]


def test_exact_ties():
    """two equal detections: the lower index gets the track, the other is born.  Two equal tracks: the lower slot gets the detection"""
    trk = TrackerNp(1)
    d, n = frames([box(0)], [box(1), box(1)])
    out = track_np(trk, d, n)
    assert out[1, :2].tolist() == [(1, 2), (2, 1)]
    trk = TrackerNp(1)
    d, n = frames([box(0), box(0)], [box(1)])
    out = track_np(trk, d, n)
    assert out[0, :2].tolist() == [(1, 1), (2, 1)] and out[1, 0].tolist() == (1, 2)
    st, _ = trk.read(0)
    assert st["hits"].tolist() == [2, 1] and st["miss"].tolist() == [0, 1]


def test_velocity_coast_death_and_slot_reuse():
    """max_miss = 1.  x = 0, 2, 6: vx = 2 at hits == 1, then (2 + 4) / 2 = 3.  Two empty frames: x = 9 with miss 1, then 12 with miss 2 > 1:
    dead, and the box that arrives in that very frame is born into slot 0"""
    trk = TrackerNp(1)
    d, n = frames([box(0)], [box(2)], [box(6)], [])
    out = track_np(trk, d, n, max_miss=1)
    assert [out[f, 0].tolist() for f in range(3)] == [(1, 1), (1, 2), (1, 3)]
    st, cnt = trk.read(0)
    assert (st["x"][0], st["vx"][0], st["hits"][0], st["miss"][0]) == (9, 3, 3, 1) and cnt.tolist() == [1, 0, 0, 0]
    d, n = frames([box(500)])
    out = track_np(trk, d, n, max_miss=1)
    assert out[0, 0].tolist() == (2, 1)
    st, cnt = trk.read(0)
    assert len(st) == 1 and st["id"][0] == 2 and st["x"][0] == 500 and cnt.tolist() == [2, 1, 0, 0]
    assert trk.slots[0][0]["id"] == 2 and trk.events["reuse"] == 1  # slot 0 again
    # after hits == 1 the velocity is averaged with the stored one, and dx is taken from the stored x, not the prediction
    trk = TrackerNp(1)
    d, n = frames([box(0)], [box(2)], [box(3)])
    track_np(trk, d, n)
    assert trk.read(0)[0]["vx"][0] == F(1.5)  # (2 + (3 - 2)) / 2


def test_identity_carry():
    trk = TrackerNp(1)
    d, n = frames([box(0), box(100)], [box(0), box(100)], [box(0), box(100)], [box(0), box(100)])
    ids = np.zeros(d.shape, dtype=CLS)
    ids["cls"] = -1
    ids[0, 0] = (5, 0.7)
    ids[1, 0] = (9, 0.7)   # an equal score replaces (>=)
    ids[1, 1] = (4, -0.5)  # the first identity a track sees is taken whatever its score
    ids[2, 0] = (3, 0.6)   # a lower one does not
    ids[2, 1] = (6, -0.75)
    ids[3, 0] = (-1, 0.99)  # no identity
    track_np(trk, d[:1], n[:1], idents=ids[:1], carry_identity=True)
    assert trk.read(0)[0]["ident"].tolist() == [(5, F(0.7)), (-1, 0)]
    track_np(trk, d[1:2], n[1:2], idents=ids[1:2], carry_identity=True)
    assert trk.read(0)[0]["ident"].tolist() == [(9, F(0.7)), (4, -0.5)]
    track_np(trk, d[2:], n[2:], idents=ids[2:], carry_identity=True)
    assert trk.read(0)[0]["ident"].tolist() == [(9, F(0.7)), (4, -0.5)]
    other = TrackerNp(1)
    track_np(other, d, n, idents=ids)  # without the flag nothing is carried
    assert other.read(0)[0]["ident"].tolist() == [(-1, 0), (-1, 0)]


def test_invalid_boxes_are_ignored():
    bad = [box(float("nan")), box(0, y=float("inf")), box(0, w=float("inf")), box(0, w=0.0), box(0, h=-1.0), box(0, conf=float("nan")),
           box(0, conf=0.4)]
    trk = TrackerNp(1)
    d, n = frames(bad + [box(7)])
    out = track_np(trk, d, n)
    assert out["id"][0].tolist() == [-1] * 7 + [1] and trk.read(0)[1].tolist() == [1, 0, 0, 0]
    # the class window
    d, n = frames([box(0, cls=1), box(50, cls=2), box(100, cls=4)])
    out = track_np(TrackerNp(1), d, n, classes=(2, 2))
    assert out["id"][0, :3].tolist() == [-1, 1, -1]
    # a low set only with low_conf
    d, n = frames([box(0)], [box(9, conf=0.4)])
    assert track_np(TrackerNp(1), d, n)[1, 0].tolist() == (-1, 0)
    assert track_np(TrackerNp(1), d, n, low_conf=0.3)[1, 0].tolist() == (-1, 0)    # iou 1 / 19 < 0.5
    assert track_np(TrackerNp(1), d, n, low_conf=0.3, iou_thresh_low=0.05)[1, 0].tolist() == (1, 2)
    d, n = frames([box(9, conf=0.4)])
    assert track_np(TrackerNp(1), d, n, low_conf=0.3)[0, 0].tolist() == (-1, 0)    # the low set never gives birth


def test_overflow_and_dropped_counters():
    rows = [box(20.0 * k, y=0.0) for k in range(300)]
    d, n = frames(rows, [box(20.0 * k, y=500.0) for k in range(10)], max_det=300)
    trk = TrackerNp(1)
    out = track_np(trk, d[:1], n[:1])
    assert out["id"][0, :256].tolist() == list(range(1, 257)) and (out["id"][0, 256:] == -1).all()
    assert trk.read(0)[1].tolist() == [256, 0, 44, 0]
    out = track_np(trk, d[1:], n[1:])
    assert (out["id"][0] == -1).all() and trk.read(0)[1].tolist() == [256, 0, 44, 10] and trk.next_id[0] == 257


def test_both_frame_to_stream_maps():
    d, n = frames([box(0)], [box(100)], [box(1)], [box(101)])
    trk = TrackerNp(2)
    out = track_np(trk, d, n)  # frames 0 and 2 are stream 0, frames 1 and 3 stream 1
    assert [out[f, 0].tolist() for f in range(4)] == [(1, 1), (1, 1), (1, 2), (1, 2)]
    assert [len(trk.read(b)[0]) for b in range(2)] == [1, 1]
    trk = TrackerNp(2)
    out = track_np(trk, d, n, stream_major=True)  # frames 0 and 1 are stream 0
    assert [out[f, 0].tolist() for f in range(4)] == [(1, 1), (2, 1), (1, 1), (2, 1)]
    assert [trk.read(b)[0]["x"].tolist() for b in range(2)] == [[0, 100], [1, 101]]
    # one call over 2 T steps == two calls over T steps
    one, two = TrackerNp(2), TrackerNp(2)
    a = track_np(one, d, n)
    b = np.concatenate([track_np(two, d[:2], n[:2]), track_np(two, d[2:], n[2:])])
    assert a.tobytes() == b.tobytes() and all(one.read(s)[0].tobytes() == two.read(s)[0].tobytes() for s in range(2))


# ---- refusals ----------------------------------------------------------------------------------------------------------------------------
def test_track_bad_arguments_are_refused_up_front(marsrt):
    L = marsrt.lib()
    BAD_FILE, BAD_TENSOR = marsrt.MARS_ERR_INVALID_FILE, marsrt.MARS_ERR_INVALID_TENSOR
    P = C.POINTER(marsrt.MarsModel)
    a = marsrt.MarsModel()              # never looked into: the refusals come first
    fake = (C.c_char * 256)()           # stands where a tracker would: three streams, no tables
    struct.pack_into("i", fake, 0, 3)
    trk = C.cast(fake, C.c_void_p)
    d, n = frames([box(0)], [box(1)], [box(2)], [box(3)], [box(4)], [box(5)])
    ids = np.zeros(d.shape, dtype=CLS)
    out = np.full(d.shape, 77, dtype=TRACK)
    good = marsrt.track_opts()

    # the lifecycle
    p = C.c_void_p()
    assert L.mars_hip_tracker_create(3, None) == BAD_FILE
    for s, code in ((0, BAD_FILE), (-2, BAD_FILE), (65536, BAD_TENSOR)):
        assert L.mars_hip_tracker_create(s, C.byref(p)) == code and not p.value
    assert L.mars_hip_tracker_reset(None) == BAD_FILE
    L.mars_hip_tracker_free(None)
    st = np.zeros(4, dtype=STATE)
    nl = C.c_int(77)
    assert L.mars_hip_tracker_read(None, 0, st.ctypes.data, 4, C.byref(nl), None) == BAD_FILE
    assert L.mars_hip_tracker_read(trk, 0, None, 4, C.byref(nl), None) == BAD_FILE
    assert L.mars_hip_tracker_read(trk, 0, st.ctypes.data, -1, C.byref(nl), None) == BAD_FILE
    assert L.mars_hip_tracker_read(trk, 3, st.ctypes.data, 4, C.byref(nl), None) == BAD_TENSOR
    assert L.mars_hip_tracker_read(trk, -1, st.ctypes.data, 4, C.byref(nl), None) == BAD_TENSOR
    assert nl.value == 77

    def run(o, t=trk, dd=d, cc=n, ii=None, nf=6, md=8, oo=out):
        return L.mars_yolo_track_lists(t, None if dd is None else dd.ctypes.data, None if cc is None else cc.ctypes.data,
                                       None if ii is None else ii.ctypes.data, nf, md, None if o is None else C.byref(o),
                                       None if oo is None else oo.ctypes.data)

    # options
    nan, inf = float("nan"), float("inf")
    bad = [dict(min_conf=-0.1), dict(min_conf=nan), dict(min_conf=inf), dict(min_conf=1.5), dict(low_conf=-0.1), dict(low_conf=nan),
           dict(low_conf=1.5, min_conf=1.0), dict(iou_thresh=-0.1), dict(iou_thresh=nan), dict(iou_thresh=1.01), dict(iou_thresh_low=-1.0),
           dict(iou_thresh_low=inf), dict(iou_thresh_low=2.0), dict(max_miss=-1), dict(classes=(-1, 2)), dict(classes=(0, -2)),
           dict(low_conf=0.5), dict(low_conf=0.6), dict(min_conf=0.3, low_conf=0.3), dict(min_conf=0.3, low_conf=0.4)]
    bad = [marsrt.track_opts(**kw) for kw in bad]
    for bit in (8, 16, 1 << 31):
        o = marsrt.track_opts()
        o.flags = bit
        bad.append(o)
    for o in bad:
        assert run(o) == BAD_FILE
        assert L.mars_hip_track_device(C.pointer(a), trk, C.byref(o)) == BAD_FILE
        assert L.mars_hip_track(C.pointer(a), trk, C.byref(o), out.ctypes.data) == BAD_FILE
    assert run(None) == BAD_FILE
    for kw in (dict(t=None), dict(dd=None), dict(cc=None), dict(oo=None), dict(nf=0), dict(nf=-3), dict(md=0), dict(md=-1)):
        assert run(good, **kw) == BAD_FILE, kw
    assert run(marsrt.track_opts(carry_identity=True)) == BAD_FILE               # the flag without the array
    assert run(good, md=1001) == BAD_TENSOR
    assert run(good, nf=4) == BAD_TENSOR and run(good, nf=5) == BAD_TENSOR       # F % S != 0
    assert run(marsrt.track_opts(min_conf=0.3, low_conf=0.29, iou_thresh=1.0, iou_thresh_low=1.0, max_miss=5, classes=(3, 4), any_class=True,
                                 carry_identity=True, stream_major=True), ii=ids, nf=4) == BAD_TENSOR  # good options pass the first check
    assert (out["id"] == 77).all() and (out["hits"] == 77).all()                 # nothing was written

    # the model forms
    assert L.mars_hip_track_device(P(), trk, C.byref(good)) == BAD_FILE
    assert L.mars_hip_track_device(C.pointer(a), None, C.byref(good)) == BAD_FILE
    assert L.mars_hip_track_device(C.pointer(a), trk, None) == BAD_FILE
    assert L.mars_hip_track(P(), trk, C.byref(good), out.ctypes.data) == BAD_FILE
    assert L.mars_hip_track(C.pointer(a), None, C.byref(good), out.ctypes.data) == BAD_FILE
    assert L.mars_hip_track(C.pointer(a), trk, None, out.ctypes.data) == BAD_FILE
    assert L.mars_hip_track(C.pointer(a), trk, C.byref(good), None) == BAD_FILE
    assert L.mars_hip_track_results(P(), out.ctypes.data) == BAD_FILE
    assert L.mars_hip_track_results(C.pointer(a), None) == BAD_FILE
