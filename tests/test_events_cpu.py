"""Events (include/mars_hip.h, "Events"), the part that needs no GPU: the entry points are exported, the record sizes are the header's,
arguments that can never be valid are refused up front and leave everything as it was, the restatement tests/test_gpu_events.py compares
the device against (tests/eventref.py) is pinned on cases worked out by hand, and every case table the GPU file uses is shown not to be
vacuous."""
import ctypes as C
import os
import struct
import subprocess

import numpy as np
import pytest

import eventref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ["mars_hip_events_create", "mars_hip_events_free", "mars_hip_events_reset", "mars_hip_events_set_rules", "mars_hip_events_read",
       "mars_hip_events_read_slots", "mars_yolo_event_lists", "mars_hip_events_device", "mars_hip_events_results", "mars_hip_events",
       "mars_hip_events_ms"]
GATE = R.Rules([(48, 0, 48, 64)])  # A -> B points down the y axis: the positive side is x <= 48
Z, EN, EX, DW, LI, LO = range(6)   # the fields of a record


# ---- the library's side that needs no device ------------------------------------------------------------------------------------------------
def test_symbols_and_record_sizes(marsrt, tmp_path):
    L = marsrt.lib()
    for n in NEW:
        assert n in marsrt.EXPORTS["mars_hip.h"] and hasattr(L, n), n
    assert marsrt.EVENT_DTYPE == R.EVENT and marsrt.EVENT_SLOT_DTYPE == R.SLOT
    assert (marsrt.EVENTS_MAX_LINES, marsrt.EVENTS_MAX_ZONES, marsrt.EVENTS_MAX_VERTS) == (R.MAX_LINES, R.MAX_ZONES, R.MAX_VERTS)
    assert (marsrt.EVENTS_STREAM_MAJOR, marsrt.EVENTS_ANCHOR_BOTTOM) == (R.STREAM_MAJOR, R.ANCHOR_BOTTOM)
    src = tmp_path / "sz.c"
    src.write_text('#include <stdio.h>\n#include "mars_hip.h"\nint main(void){printf("%zu %zu %zu %zu %zu %zu %d %d %d %u %u", sizeof(mars_event_t), '
                   'sizeof(mars_event_slot_t), sizeof(mars_event_line_t), sizeof(mars_event_zone_t), sizeof(mars_hip_event_rules_t), '
                   'sizeof(mars_hip_events_opts_t), MARS_EVENTS_MAX_LINES, MARS_EVENTS_MAX_ZONES, MARS_EVENTS_MAX_VERTS, MARS_EVENTS_STREAM_MAJOR, '
                   'MARS_EVENTS_ANCHOR_BOTTOM);return 0;}\n')
    exe = tmp_path / "sz"
    subprocess.check_call(["gcc", "-std=c11", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)])
    want = [R.EVENT.itemsize, R.SLOT.itemsize, C.sizeof(marsrt.EventLine), C.sizeof(marsrt.EventZone), C.sizeof(marsrt.EventRules),
            C.sizeof(marsrt.EventsOpts), R.MAX_LINES, R.MAX_ZONES, R.MAX_VERTS, R.STREAM_MAJOR, R.ANCHOR_BOTTOM]
    assert subprocess.check_output([str(exe)]).decode().split() == [str(v) for v in want]
    assert want[:6] == [24, 152, 16, 72, 2824, 12]


def bad_rules(marsrt):
    tri = [(0, 0), (10, 0), (0, 10)]
    yield "33 lines", _raw(marsrt, n_lines=33)
    yield "-1 lines", _raw(marsrt, n_lines=-1)
    yield "33 zones", _raw(marsrt, n_zones=33)
    yield "-1 zones", _raw(marsrt, n_zones=-1)
    yield "A == B", marsrt.event_rules([(0, 0, 10, 10), (5, 7, 5, 7)])
    for k in range(4):
        for v in (32769, -32769):
            ln = [1, 2, 3, 4]
            ln[k] = v
            yield "line coordinate", marsrt.event_rules([ln])
    yield "2 vertices", marsrt.event_rules(zones=[tri, tri[:2]])
    r = marsrt.event_rules(zones=[tri])
    r.zones[0].n = 9
    yield "9 vertices", r
    yield "negative dwell", marsrt.event_rules(zones=[(tri, -1)])
    yield "zone x", marsrt.event_rules(zones=[[(0, 0), (32769, 0), (0, 10)]])
    yield "zone y", marsrt.event_rules(zones=[[(0, 0), (10, 0), (0, -32769)]])


def _raw(marsrt, **kw):
    r = marsrt.event_rules([(0, 0, 1, 1)], [[(0, 0), (10, 0), (0, 10)]])
    for k, v in kw.items():
        setattr(r, k, v)
    return r


def test_refusals_without_a_device(marsrt):
    FILE, TENSOR = marsrt.MARS_ERR_INVALID_FILE, marsrt.MARS_ERR_INVALID_TENSOR
    L = marsrt.lib()
    p = C.c_void_p()
    for streams, code in ((0, FILE), (-1, FILE), (65536, TENSOR)):
        assert L.mars_hip_events_create(streams, C.byref(p)) == code and not p.value
    assert L.mars_hip_events_create(1, None) == FILE
    fake = (C.c_char * 256)()            # stands where an events object would: three streams, no tables
    struct.pack_into("i", fake, 0, 3)
    before = bytes(fake)
    ev = C.cast(fake, C.c_void_p)
    a = marsrt.MarsModel()               # never looked into: the refusals come first
    good = marsrt.event_rules([(0, 0, 1, 1)], [([(0, 0), (10, 0), (0, 10)], 3)])
    # the rules
    assert L.mars_hip_events_set_rules(None, 0, C.byref(good)) == FILE and L.mars_hip_events_set_rules(ev, 0, None) == FILE
    for what, r in bad_rules(marsrt):
        assert L.mars_hip_events_set_rules(ev, 0, C.byref(r)) == FILE, what
        assert L.mars_hip_events_set_rules(ev, 7, C.byref(r)) == FILE, what  # two faults: the rules before the stream
    for stream in (3, -2):
        assert L.mars_hip_events_set_rules(ev, stream, C.byref(good)) == TENSOR
        assert L.mars_hip_events_reset(ev, stream) == TENSOR
    edge = marsrt.event_rules([(-32768, 32768, 32768, -32768)], [[(-32768, -32768), (32768, -32768), (0, 32768)]])
    assert L.mars_hip_events_set_rules(ev, 9, C.byref(edge)) == TENSOR  # the limits themselves pass the rules' checks
    assert L.mars_hip_events_reset(None, 0) == FILE
    # reading
    assert L.mars_hip_events_read(None, 0, None, None, None, None, None) == FILE and L.mars_hip_events_read_slots(None, 0, None) == FILE
    slots = np.zeros(R.SLOTS, dtype=R.SLOT)
    assert L.mars_hip_events_read_slots(ev, 0, None) == FILE
    for stream in (-1, 3):
        assert L.mars_hip_events_read(ev, stream, None, None, None, None, None) == TENSOR
        assert L.mars_hip_events_read_slots(ev, stream, slots.ctypes.data) == TENSOR
    # the list form
    d, t, n = R.lists([[(1, 1, R.det(1.0, 1.0))]] * 6)
    rec = np.zeros(d.shape, dtype=R.EVENT)
    o = marsrt.event_opts()

    def lists(ev=ev, d=d.ctypes.data, t=t.ctypes.data, n=n.ctypes.data, frames=6, max_det=1, o=o, rec=rec.ctypes.data):
        return L.mars_yolo_event_lists(ev, d, t, n, frames, max_det, C.byref(o) if o is not None else None, rec, None, None)

    for kw in (dict(ev=None), dict(d=None), dict(t=None), dict(n=None), dict(rec=None), dict(o=None), dict(frames=0), dict(frames=-3),
               dict(max_det=0), dict(o=marsrt.event_opts(max_gap=-1)), dict(o=marsrt.event_opts(min_hits=-1)), dict(o=marsrt.event_opts(flags=4)),
               dict(o=marsrt.event_opts(flags=4), max_det=1001)):
        assert lists(**kw) == FILE, kw
    assert lists(max_det=1001) == TENSOR
    for frames in (4, 5, 1):
        assert lists(frames=frames) == TENSOR  # F % S != 0
    assert rec.tobytes() == bytes(rec.nbytes)
    # the device forms
    P = C.POINTER(marsrt.MarsModel)
    assert L.mars_hip_events_device(None, ev, C.byref(o)) == FILE and L.mars_hip_events_device(C.cast(C.pointer(a), P), None, C.byref(o)) == FILE
    assert L.mars_hip_events_device(C.cast(C.pointer(a), P), ev, None) == FILE
    assert L.mars_hip_events_results(None, ev, None, None, None) == FILE and L.mars_hip_events_results(C.cast(C.pointer(a), P), None, None, None, None) == FILE
    assert L.mars_hip_events(None, ev, C.byref(o), None, None, None) == FILE
    assert L.mars_hip_events(C.cast(C.pointer(a), P), ev, None, None, None, None) == FILE
    assert L.mars_hip_events_ms(None) < 0
    L.mars_hip_events_free(None)
    assert bytes(fake) == before         # nothing was touched
    with pytest.raises(ValueError):
        marsrt.event_rules([(0, 0, 1, 1)] * 33)
    with pytest.raises(ValueError):
        marsrt.event_rules(zones=[[(0, 0)] * 9])


# ---- the restatement on hand-computed cases -------------------------------------------------------------------------------------------------
def test_a_straight_walk_over_a_line_in_each_direction():
    # side(X) = cross(B - A, X - A) >= 0 with B - A = (0, 1024): -1024 * (X.x - 768) >= 0, so x <= 48 is the positive side
    rec, ev = R.walk(GATE, [(60, 20), (40, 20), (40, 30), (60, 30)])
    assert rec == [(0,) * 6, (0, 0, 0, 0, 1, 0), (0,) * 6, (0, 0, 0, 0, 0, 1)]  # 0 -> 1 is `in`; along the line nothing; 1 -> 0 is `out`
    lt, _, cnt, used, step = ev.read(0)
    assert lt[0].tolist() == [1, 1] and not lt[1:].any() and cnt.tolist() == [1, 0, 0, 0, 0] and (used, step) == (1, 4)
    # beside the segment's ends: the line is crossed, the segment is not
    short = R.Rules([(48, 10, 48, 20)])
    assert R.walk(short, [(60, 25), (40, 25)])[0][1] == (0,) * 6 and R.walk(short, [(60, 15), (40, 15)])[0][1][LI] == 1
    # the reversed line swaps the directions
    assert R.walk(R.Rules([(48, 64, 48, 0)]), [(60, 20), (40, 20)])[0][1] == (0, 0, 0, 0, 0, 1)


def test_a_path_that_ends_on_the_line():
    # a point on the line is on the positive side: arriving from the negative side counts at once, leaving to the positive side is nothing more
    rec, _ = R.walk(GATE, [(60, 20), (48, 20), (40, 20)])
    assert [r[LI:] for r in rec] == [(0, 0), (1, 0), (0, 0)]
    rec, _ = R.walk(GATE, [(60, 20), (48, 20), (60, 20)])  # ... and back to the negative side is an `out`
    assert [r[LI:] for r in rec] == [(0, 0), (1, 0), (0, 1)]
    rec, _ = R.walk(GATE, [(40, 20), (48, 20), (40, 20)])  # from the positive side onto the line and back: never crossed
    assert [r[LI:] for r in rec] == [(0, 0), (0, 0), (0, 0)]
    rec, _ = R.walk(GATE, [(40, 20), (48, 20), (60, 20)])  # ... and on to the negative side: one `out`, at the step that leaves the line
    assert [r[LI:] for r in rec] == [(0, 0), (0, 0), (0, 1)]
    # one sixteenth short of the line is still the negative side: 48.0625 * 16 = 769
    assert R.quantise(48.0625) == 769 and R.walk(GATE, [(60, 20), (48.0625, 20)])[0][1][LI] == 0


def test_a_path_through_a_shared_end_point_counts_once():
    two = R.Rules([(48, 0, 48, 32), (48, 32, 48, 64)])
    # P = (960, 512), Q = (640, 512), Q - P = (-320, 0).  Segment 0: A - P = (-192, -512) -> cross = 163840 >= 0; B - P = (-192, 0) -> 0 >= 0:
    # equal, not crossed.  Segment 1: A - P = (-192, 0) -> 0 >= 0; B - P = (-192, 512) -> -163840 < 0: crossed
    assert R.cross(-320, 0, -192, -512) == 163840 and R.cross(-320, 0, -192, 512) == -163840
    rec, _ = R.walk(two, [(60, 32), (40, 32)])
    assert rec[1][LI:] == (2, 0)
    # the way back, Q - P = (320, 0): every cross changes its sign but the zero stays >= 0, so now segment 0 takes it.  Exactly one either way
    rec, _ = R.walk(two, [(40, 32), (60, 32)])
    assert rec[1][LI:] == (0, 1)
    # a slanted path through the same point, and one just beside it on either side
    for p, q, want in (((60, 20), (36, 44), 2), ((60, 19), (36, 43), 1), ((60, 21), (36, 45), 2)):
        rec, _ = R.walk(two, [p, q])
        assert rec[1][LI:] == (want, 0), (p, q)
    assert R.walk(two, [(36, 44), (60, 20)])[0][1][LI:] == (0, 1)
    # the outer ends: in this direction the first segment's A belongs to it and the last segment's B does not; the way back swaps them
    assert R.walk(two, [(60, 0), (40, 0)])[0][1][LI:] == (1, 0) and R.walk(two, [(60, 64), (40, 64)])[0][1][LI:] == (0, 0)
    assert R.walk(two, [(40, 0), (60, 0)])[0][1][LI:] == (0, 0) and R.walk(two, [(40, 64), (60, 64)])[0][1][LI:] == (0, 2)


def test_standing_still_crosses_nothing():
    rec, ev = R.walk(R.Rules([(48, 0, 48, 64), (0, 20, 96, 20)], [([(40, 10), (60, 10), (60, 30), (40, 30)], 0)]), [(48, 20), (48, 20), (48, 20)])
    assert rec == [(1, 0, 0, 0, 0, 0)] * 3  # on both lines and inside the zone: P == Q
    assert not ev.read(0)[0].any()


C_ZONE = [(0, 0), (30, 0), (30, 10), (10, 10), (10, 20), (30, 20), (30, 30), (0, 30)]  # a C open to the right: the notch is 10 < x, 10 <= y < 20


def test_a_concave_zone_on_a_vertex_row_and_on_an_edge():
    rules = R.Rules(zones=[(C_ZONE, 0)])

    def inside(x, y):
        return bool(rules.zones_of((16 * x, 16 * y)))

    assert len(C_ZONE) == R.MAX_VERTS
    assert inside(5, 15) and not inside(20, 15) and inside(20, 5) and inside(20, 25) and not inside(40, 5) and not inside(-1, 15)
    # Q = (20, 15): the row meets the edges x = 10 (d = 10: lhs = (20 - 10) * 10 = 100 < rhs = 0 fails) and x = 0 (d = -30: lhs = -600 > 0
    # fails): no toggle.  Q = (5, 15): the first gives lhs = -50 < 0: one toggle
    # on a vertex's row, y = 10: (V.y > 10) != (W.y > 10) holds for the edges that go on above 10 only, so the two vertices are no double count
    assert inside(5, 10) and not inside(20, 10) and not inside(35, 10)
    # y = 20, the notch's lower side: the lower arm begins there
    assert inside(5, 20) and inside(20, 20) and not inside(30, 20)
    # edges: the upper (min y) and the left side belong to the zone, the lower and the right side do not
    assert inside(20, 0) and not inside(20, 30) and inside(0, 15) and not inside(30, 5) and not inside(10, 15)
    # the corners: only the top-left one is inside
    assert inside(0, 0) and not inside(30, 0) and not inside(0, 30) and not inside(30, 30)
    # one sixteenth decides
    assert rules.zones_of((16 * 30 - 1, 16 * 5)) == 1 and rules.zones_of((16 * 20, 16 * 30 - 1)) == 1
    # enter, stay, exit as records: into the spine, down inside it, out through the notch
    rec, ev = R.walk(rules, [(40, 15), (5, 15), (5, 25), (20, 15)])
    assert [r[:3] for r in rec] == [(0, 0, 0), (1, 1, 0), (1, 0, 0), (0, 0, 1)]
    assert ev.read(0)[1][0].tolist() == [1, 1, 0, 0]


def test_the_clamp_and_the_floor():
    assert R.quantise(1e9) == 524288 and R.quantise(-1e9) == -524288 and R.quantise(32768.0) == 524288 and R.quantise(40000.0) == 524288
    assert R.quantise(32767.97) == 524287      # float32(32767.97) = 32767.96875, * 16 = 524287.5
    assert R.quantise(-0.03) == -1 and R.quantise(0.0625) == 1 and R.quantise(0.06) == 0 and R.quantise(-32768.01) == -524288
    assert R.quantise(3.4e38) == 524288 and R.quantise(-3.4e38) == -524288
    # a track far outside still has a side: from the clamp's corner across the gate
    rec, ev = R.walk(GATE, [(1e9, 20), (-1e9, 20)])
    assert rec[1][LI:] == (1, 0) and ev.read_slots(0)[0]["qx"] == -524288
    # the rules' limits are the clamp's: a zone over the whole plane holds every anchor but those on its right and lower side
    whole = R.Rules(zones=[([(-32768, -32768), (32768, -32768), (32768, 32768), (-32768, 32768)], 0)])
    assert whole.zones_of((-524288, -524288)) == 1 and whole.zones_of((524287, 524287)) == 1 and whole.zones_of((524288, 0)) == 0
    # the largest products: 2^20 * 2^20 twice, far inside int64
    assert R.crossing((-524288, -524288, 524288, 524288), (524288, -524288), (-524288, 524288)) == 1


def test_anchor_bottom_rounds_the_sum_in_float32():
    # y = 16384 + 1/16 - 2^-9 has an odd last bit at a spacing of 2^-9; h = 2^-9 gives half = 2^-10, exactly half a spacing: the tie goes to
    # even, up to 16384.0625 -> q = 262145.  In real arithmetic y + h / 2 = 16384.0615234375 -> 262144
    y, h = 16384.060546875, 0.001953125
    assert float(R.F(y)) == y and float(R.F(h)) == h
    assert R.anchor(R.det(3.0, y, 4.0, h), True) == (48, 262145) and R.anchor(R.det(3.0, y, 4.0, h), False) == (48, 262144)
    assert int(np.floor((y + h / 2) * 16)) == 262144
    # y + h * 0.5 beyond the float range is +-inf, which the clamp takes
    assert R.anchor(R.det(0.0, 3e38, 1.0, 3e38), True)[1] == 524288 and R.anchor(R.det(0.0, -3e38, 1.0, -3e38), True)[1] == -524288
    # h * 0.5 of the smallest denormal rounds to zero
    assert R.anchor(R.det(0.0, 2.0, 1.0, 1e-45), True)[1] == 32
    # the foot point enters where the centre does not
    zone = R.Rules(zones=[([(0, 10), (20, 10), (20, 20), (0, 20)], 0)])
    pts = [(5, 4, 2, 4), (5, 4, 2, 12)]
    assert [r[:2] for r in R.walk(zone, pts, anchor_bottom=True)[0]] == [(0, 0), (1, 1)]
    assert [r[:2] for r in R.walk(zone, pts)[0]] == [(0, 0), (0, 0)]


def test_dwell_gap_and_expiry_by_hand():
    zone = R.Rules(zones=[([(0, 0), (20, 0), (20, 20), (0, 20)], 2)])
    IN, OUT = (5, 5), (50, 5)
    # first sight inside: since = 0, no enter event; step 1: 1 - 0 < 2; step 2 fires; step 3 not again
    rec, _ = R.walk(zone, [IN, IN, IN, IN])
    assert [r[:4] for r in rec] == [(1, 0, 0, 0), (1, 0, 0, 0), (1, 0, 0, 1), (1, 0, 0, 0)]
    # entered at step 1, due at step 3, which falls into a gap: fires on return at step 4
    rec, _ = R.walk(zone, [OUT, IN, None, None, IN, IN])
    assert [r and r[:4] for r in rec] == [(0, 0, 0, 0), (1, 1, 0, 0), None, None, (1, 0, 0, 1), (1, 0, 0, 0)]
    # an exit clears the stay: inside 0 .. 1, out at 2, in at 3 (since = 3), fires at 5; a second stay fires again
    rec, ev = R.walk(zone, [IN, IN, OUT, IN, IN, IN])
    assert [r[:4] for r in rec] == [(1, 0, 0, 0), (1, 0, 0, 0), (0, 0, 1, 0), (1, 1, 0, 0), (1, 0, 0, 0), (1, 0, 0, 1)]
    assert ev.read(0)[1][0].tolist() == [1, 1, 1, 0] and ev.read_slots(0)[0]["since"][0] == 3 and ev.read_slots(0)[0]["dwelled"] == 1
    # a gap of exactly max_gap steps is seen again, judged over the whole gap; one more step and the slot is gone
    rec, ev = R.walk(zone, [IN, None, None, OUT], max_gap=3)
    assert rec[3][:3] == (0, 0, 1) and ev.read(0)[2].tolist() == [1, 0, 0, 0, 0]
    rec, ev = R.walk(zone, [IN, None, None, None, OUT], max_gap=3)
    assert rec[4] == (0,) * 6 and ev.read(0)[2].tolist() == [2, 1, 0, 0, 0] and ev.read(0)[1][0].tolist() == [0, 0, 0, 1]  # expired: lost
    # expiry without a return: the step counter alone does it
    rec, ev = R.walk(zone, [IN, None, None], max_gap=1)
    assert ev.read(0)[3:] == (0, 3) and ev.read(0)[1][0, 3] == 1 and not ev.read_slots(0).tobytes().strip(b"\0")


def test_frame_orders_and_split_invariance():
    for S, T in ((3, 4), (2, 6)):
        d, t, n = R.scene(77, S, T, 9, 12, major=False)
        dm, tm, nm = R.scene(77, S, T, 9, 12, major=True)
        one, two, maj = R.EventsNp(S), R.EventsNp(S), R.EventsNp(S)
        for ev in (one, two, maj):
            ev.set_rules(R.RULES3)
        whole = one.run(d, t, n, max_gap=2)
        wm = maj.run(dm, tm, nm, max_gap=2, stream_major=True)
        h = S * T // 2
        parts = [two.run(d[k:k + h], t[k:k + h], n[k:k + h], max_gap=2) for k in (0, h)]
        for k in range(3):
            assert np.array_equal(whole[k], np.concatenate([parts[0][k], parts[1][k]]))
        for f in range(S * T):
            b, s = R.stream_step(f, S * T, S, True)
            assert all(np.array_equal(wm[k][f], whole[k][s * S + b]) for k in range(3))
        for b in range(S):
            assert one.read_slots(b).tobytes() == two.read_slots(b).tobytes() == maj.read_slots(b).tobytes()
            assert all(np.array_equal(x, y) for x, y in zip(one.read(b), two.read(b)))


# ---- no GPU case passes empty -----------------------------------------------------------------------------------------------------------------
def test_the_shape_scenes_are_not_vacuous():
    tot = {}
    for S, T, major in R.SHAPES:
        d, t, n = R.scene(0xE7E0000 + 16 * S + T, S, T, 12, 16, major)
        ev = R.EventsNp(S)
        ev.set_rules(R.RULES3)
        sm = R.summary(ev, [ev.run(d, t, n, max_gap=1, stream_major=major)])
        assert sm["first"] >= S * 6 and sm["used"] >= 1
        if T == 1:  # the first step of a stream only takes slots
            assert not any(sm[k] for k in ("lines_in", "lines_out", "entered", "exited", "dwelled", "expired"))
        else:
            assert min(sm[k] for k in ("lines_in", "lines_out", "entered", "exited")) >= 1, (S, T, sm)
        for k, v in sm.items():
            tot[k] = tot.get(k, 0) + v
    assert min(tot[k] for k in ("lines_in", "lines_out", "entered", "exited", "dwelled", "lost", "expired")) >= 1, tot


@pytest.mark.parametrize("name", sorted(R.CASES))
def test_gpu_cases_are_not_vacuous(name):
    S, rules, calls, need = R.CASES[name]()
    ev = R.EventsNp(S)
    ev.set_rules(rules)
    sm = R.summary(ev, [ev.run(d, t, n, **kw) for d, t, n, kw in calls])
    assert all(sm[k] >= 1 for k in need), (name, sm)
    if name == "pressure":
        assert ev.read(0)[2].tolist() == [257, 1, 0, 1, 0] and ev.read_slots(0)[0]["id"] == 257 and ev.read(0)[3] == 256
    if name == "overflow":
        assert ev.read(0)[2].tolist() == [256, 0, 88, 0, 0]
    if name == "duplicates":
        assert ev.read(0)[2].tolist() == [256, 0, 84, 0, 4]  # 298 participants per frame
    if name == "many_rules":
        assert len(rules.lines) == 32 and len(rules.zones) == 32 and all(len(v) == 8 for v, _ in rules.zones)
    if name == "bad_entries":
        assert ev.read(0)[2].tolist() == [2, 0, 0, 0, 0]  # ids 15 and 16 alone ever take part


def test_the_restatement_writes_what_the_bindings_read(marsrt):
    """the rule record of the bindings holds what the restatement's Rules hold"""
    r = marsrt.event_rules(R.RULES3.lines, R.RULES3.zones)
    assert (r.n_lines, r.n_zones) == (3, 3)
    assert [(ln.ax, ln.ay, ln.bx, ln.by) for ln in r.lines[:3]] == R.RULES3.lines
    for z, (verts, dwell) in enumerate(R.RULES3.zones):
        assert (r.zones[z].n, r.zones[z].dwell) == (len(verts), dwell)
        assert list(zip(r.zones[z].x[:len(verts)], r.zones[z].y[:len(verts)])) == verts
    plain = marsrt.event_rules(zones=[[(0, 0), (10, 0), (0, 10)]])  # a bare vertex list: dwell 0
    assert (plain.zones[0].n, plain.zones[0].dwell) == (3, 0)
