"""The restatement of "Best shots" (tests/shotref.py) pinned on cases worked out by hand: the luma weights, the Laplacian's mean square
on a constant, an impulse and a checkerboard, the confidence factor, the area cap, the keep-aspect rectangle, blur lowering the score, and
the table policy point by point.  Then the condition that keeps tests/test_gpu_shot.py from passing by exercising nothing: over the
scenes that file feeds the device, the restatement's own counters show every path at least once."""
import numpy as np

import shotref as R


def crop_of(Y):
    """a grey crop whose luma is Y: R = G = B = v gives (256 v + 128) >> 8 = v"""
    Y = np.asarray(Y, dtype=np.uint8)
    return np.stack([Y, Y, Y], axis=-1)


def whole(u):
    return (u.shape[1], u.shape[0], 0, 0)


def test_luma_weights():
    assert R.luma(np.array([255, 0, 0])) == (77 * 255 + 128) >> 8 == 77
    assert R.luma(np.array([0, 255, 0])) == (150 * 255 + 128) >> 8 == 149
    assert R.luma(np.array([0, 0, 255])) == (29 * 255 + 128) >> 8 == 29
    assert R.luma(np.array([255, 255, 255])) == 255 and R.luma(np.array([0, 0, 0])) == 0
    assert all(R.luma(np.array([v, v, v])) == v for v in range(256))


def test_constant_crop():
    u = np.zeros((7, 9, 3), dtype=np.uint8)
    u[...] = (200, 100, 50)
    y = (77 * 200 + 150 * 100 + 29 * 50 + 128) >> 8
    assert y == 124 and R.metrics(u, whole(u)) == (124, 0)


def test_impulse():
    """one pixel of height d in the middle of 5 x 5: L = 4 d there, -d at its four neighbours, 0 elsewhere: sum L^2 = 20 d^2 over 9"""
    for d in (1, 10, 255):
        Y = np.zeros((5, 5), dtype=np.uint8)
        Y[2, 2] = d
        mean, sharp = R.metrics(crop_of(Y), (5, 5, 0, 0))
        assert sharp == (20 * d * d) // 9 and mean == d // 25
    # at the border of the interior: the impulse at (1, 1) has only two interior neighbours
    Y = np.zeros((5, 5), dtype=np.uint8)
    Y[1, 1] = 10
    assert R.metrics(crop_of(Y), (5, 5, 0, 0))[1] == (16 * 100 + 2 * 100) // 9


def test_checkerboard():
    Y = (np.indices((6, 8)).sum(axis=0) % 2 * 255).astype(np.uint8)
    L = R.laplacian(Y.astype(np.int64))
    assert L.shape == (4, 6) and set(np.abs(L).reshape(-1).tolist()) == {1020} and L[0, 0] == -1020 and L[0, 1] == 1020
    assert R.metrics(crop_of(Y), (8, 6, 0, 0)) == (127, 1020 * 1020) and 1020 * 1020 == 1040400


def test_small_contents_have_no_interior():
    u = np.random.default_rng(1).integers(0, 256, (4, 6, 3), dtype=np.uint8)
    for nw, nh in [(1, 1), (2, 2), (2, 4), (6, 2)]:
        assert R.metrics(u, (nw, nh, 0, 0))[1] == 0
    # 3 x 3 is the first with an interior pixel
    Y = np.zeros((3, 3), dtype=np.uint8)
    Y[1, 1] = 3
    assert R.metrics(crop_of(Y), (3, 3, 0, 0)) == (0, 144)


def test_confidence_factor():
    assert [R.conf_c(v) for v in (0.0, 1.0, 0.5, float("nan"), -1.0, 2.0)] == [0, 1024, 512, 0, 0, 1024]
    assert R.conf_c(float("inf")) == 0 and R.conf_c(float("-inf")) == 0
    assert R.conf_c(0.3) == int(np.floor(np.float32(0.3) * np.float32(1024))) == 307
    assert R.conf_c(np.nextafter(np.float32(1), np.float32(0))) == 1023


def test_area_cap_and_score():
    assert R.score_of(10, 10, 16, 16, 4, 1.0) == 100 * 5 * 1024
    assert R.score_of(100, 100, 16, 16, 4, 1.0) == 256 * 5 * 1024          # source pixels beyond the target's size add nothing
    assert R.score_of(2 ** 31, 2 ** 31, 16, 16, 0, 0.5) == 256 * 512
    assert R.score_of(1280, 1280, 1280, 1280, 1040400, 1.0) < 2 ** 52


def test_keep_aspect_rectangle():
    assert R.content_rect(10, 40, 16, 16, True) == (4, 16, 6, 0)
    assert R.content_rect(40, 10, 16, 16, True) == (16, 4, 0, 6)
    assert R.content_rect(10, 40, 16, 16, False) == (16, 16, 0, 0)
    assert R.content_rect(1, 1000, 16, 16, True) == (1, 16, 7, 0)            # max(1, ...)
    assert R.content_rect(30, 30, 17, 13, True) == (13, 13, 2, 0)
    # pixels outside the content take no part
    u = np.random.default_rng(2).integers(0, 256, (16, 16, 3), dtype=np.uint8)
    v = u.copy()
    v[:, :6] = 0
    v[:, 10:] = 255
    assert R.metrics(u, (4, 16, 6, 0)) == R.metrics(v, (4, 16, 6, 0))


def test_blur_scores_below_the_original():
    u = np.random.default_rng(3).integers(0, 256, (24, 24, 3), dtype=np.uint8)
    b = R.box_blur(u, 3)
    s0, s1 = R.metrics(u, whole(u))[1], R.metrics(b, whole(b))[1]
    assert 0 < s1 < s0
    assert R.score_of(30, 30, 24, 24, s1, 0.9) < R.score_of(30, 30, 24, 24, s0, 0.9)


def test_layouts_round_trip():
    u = np.random.default_rng(4).integers(0, 256, (5, 7, 3), dtype=np.uint8)
    for nhwc in (True, False):
        x = R.from_u8(u, nhwc)
        assert x.dtype == np.int8 and np.array_equal(R.to_u8(x, 7, 5, nhwc), u)
    assert R.from_u8(u, True)[0] == int(u[0, 0, 0]) - 128 and R.from_u8(u, False)[35] == int(u[0, 0, 1]) - 128


# ---- the table policy, each point by a hand-written sequence ----------------------------------------------------------------------------
TW, TH = 6, 5
SHARP = np.random.default_rng(5).integers(0, 256, (TH, TW, 3), dtype=np.uint8)
SOFT = R.box_blur(SHARP, 3)
RECT = (10, 10, 40, 40)


def run(entries, frames, slots=4, ref=None, **kw):
    ref = ref or R.ShotsNp(1, slots, TW, TH)
    rec = ref.run(*R.pack(entries, TW, TH, True), frames, **kw)
    return rec, ref


def test_tie_keeps_the_older_shot():
    rec, ref = run([(0, 7, 1, 0.5, 1, RECT, SHARP), (1, 7, 2, 0.5, 2, (11, 10, 41, 40), SHARP)], 2)
    s = ref.read_slots(0)[0]
    assert rec["taken"].tolist() == [1, 0] and rec["slot"].tolist() == [0, 0] and rec[0]["score"] == rec[1]["score"]
    assert (s["seen"], s["taken"], s["best_step"], s["last_step"], s["cls"], s["x0"]) == (2, 1, 0, 1, 1, 10) and ref.ties == 1
    # strictly greater replaces: the same crop at a higher confidence
    rec, ref = run([(0, 7, 3, 0.75, 3, RECT, SHARP)], 1, ref=ref)
    s = ref.read_slots(0)[0]
    assert rec["taken"].tolist() == [1] and (s["seen"], s["taken"], s["best_step"], s["cls"]) == (3, 2, 2, 3) and ref.replaced == 1
    assert np.array_equal(ref.pixels(0, 0), SHARP) and ref.read(0)[0].tolist() == [0, 0, 0, 0, 0, 2]
    # ... and a softer one does not
    rec, ref = run([(0, 7, 4, 0.75, 4, RECT, SOFT)], 1, ref=ref)
    assert rec["taken"].tolist() == [0] and 0 < rec[0]["score"] < ref.read_slots(0)[0]["score"] and ref.read_slots(0)[0]["cls"] == 3


def test_expiry_exactly_at_max_gap_plus_one():
    for back, state in ((3, R.LIVE), (4, R.DONE)):  # max_gap 3: seen at 0, back at step 3 (gap 3: alive) or 4 (gap 4: finished)
        rec, ref = run([(0, 1, 1, 0.9, 0, RECT, SHARP), (back, 1, 2, 0.9, 0, RECT, SOFT)], 5, max_gap=3)
        tab = ref.read_slots(0)
        assert tab[0]["state"] == (R.LIVE if back == 3 else R.DONE) and state == tab[0]["state"]
        assert rec["slot"].tolist() == ([0, 0] if back == 3 else [0, 1]) and ref.read(0)[0][0] == (0 if back == 3 else 1)
        assert tab[0]["seen"] == (2 if back == 3 else 1) and ref.read(0)[3] == 5
    # the default is 30
    rec, ref = run([(0, 1, 1, 0.9, 0, RECT, SHARP)], 31)
    assert ref.read(0)[1:3] == (1, 0)
    run([], 1, ref=ref)
    assert ref.read(0)[1:3] == (0, 1) and ref.read(0)[0][0] == 1


def test_free_before_done_then_done_overwritten_then_dropped():
    # 3 slots.  Step 0: ids 1, 2.  max_gap 1: both finished at step 2.  Step 2: ids 3, 4, 5 -> slot 2 (FREE), then slots 0 and 1 (DONE,
    # ascending): two shots lost.  Step 2 has a sixth id: nothing left, dropped
    e = [(0, 1, 1, 0.9, 0, RECT, SHARP), (0, 2, 1, 0.9, 0, RECT, SOFT)] + [(2, i, 1, 0.9, 0, RECT, SHARP) for i in (3, 4, 5, 6)]
    rec, ref = run(e, 3, slots=3, max_gap=1)
    assert rec["slot"].tolist() == [0, 1, 2, 0, 1, -1] and rec["taken"].tolist() == [1, 1, 1, 1, 1, 0]
    assert ref.read(0)[0].tolist() == [2, 2, 1, 0, 0, 5] and ref.read_slots(0)["id"].tolist() == [4, 5, 3]
    assert rec[5]["score"] > 0  # a dropped crop still has its metrics
    # a full LIVE table drops too, and collect frees what it hands over
    rec, ref = run([(0, 9, 1, 0.9, 0, RECT, SHARP)], 1, ref=ref)
    assert rec["slot"].tolist() == [-1] and ref.read(0)[0][2] == 2
    ref.flush()
    assert ref.read(0)[1:3] == (0, 3) and ref.read(0)[0][0] == 5
    slots, rgb, n = ref.collect(0, 2)
    assert n == 3 and slots["id"].tolist() == [4, 5] and rgb.shape == (2, TH, TW, 3) and ref.read_slots(0)["state"].tolist() == [0, 0, 2]
    assert not ref.read_slots(0)[0].tobytes().strip(b"\0")
    slots, rgb, n = ref.collect(0, 5)
    assert n == 1 and slots["id"].tolist() == [3] and ref.read(0)[1:3] == (0, 0)


def test_duplicates_and_overflow():
    rec, ref = run([(0, 5, 1, 0.9, 0, RECT, SOFT), (0, 5, 1, 0.9, 0, RECT, SHARP), (0, 6, 1, 0.9, 0, RECT, SHARP)], 1)
    assert rec["slot"].tolist() == [0, -1, 1] and ref.read(0)[0].tolist() == [0, 0, 0, 0, 1, 2]  # the lower index wins, whatever its score
    S, slots, tw, th, nhwc, calls, _ = R.CASES["overflow"]()
    ref = R.ShotsNp(S, slots, tw, th, nhwc)
    rec = ref.run(*calls[0][:6], **calls[0][6])
    # 300 candidates, one a duplicate: 299 distinct, 256 take part, 43 overflow; index 255 is the last participant, 256 the first left out
    assert ref.read(0)[0].tolist() == [0, 0, 0, 43, 1, 256] and rec[255]["slot"] == 255 and rec[256]["slot"] == -1 and rec[280]["slot"] == -1


def test_min_hits_mean_window_sharpness_and_inside():
    S, slots, tw, th, nhwc, calls, _ = R.CASES["gates"]()
    ref = R.ShotsNp(S, slots, tw, th, nhwc)
    rec = ref.run(*calls[0][:6], **calls[0][6])
    # too few hits, too dark, too flat, touching the left border, touching the bottom border, fine, fine again at a higher confidence
    assert rec["slot"].tolist() == [-1, -1, -1, -1, -1, 0, 0] and rec["taken"].tolist() == [0, 0, 0, 0, 0, 1, 1]
    assert rec[1]["mean"] < 60 and rec[2]["sharp"] == 0 and rec[2]["mean"] == 128 and rec[2]["score"] == 144 * 1 * 921
    # without the gates all six ids take slots
    ref = R.ShotsNp(S, slots, tw, th, nhwc)
    rec = ref.run(*calls[0][:6], stream_major=True)
    assert rec["slot"].tolist() == [0, 1, 2, 3, 4, 5, 5]
    # the window's ends are inside it
    m = int(rec[0]["mean"])
    for lo, hi, ok in ((m, m, True), (m + 1, 255, False), (0, m - 1, False), (1, m, True)):
        ref = R.ShotsNp(1, 2, tw, th, nhwc)
        out = ref.run(*(a[:1] for a in calls[0][:5]), 1, min_mean=lo, max_mean=hi)
        assert (out[0]["slot"] == 0) == ok


def test_records_of_crops_that_take_no_part():
    e = [(0, -1, 5, 0.9, 0, RECT, SHARP), (0, 3, 1, 0.9, 0, (40, 40, 40, 90), SHARP), (7, 3, 1, 0.9, 0, RECT, SHARP), (0, 3, 1, float("nan"), 0, RECT, SHARP)]
    rec, ref = run(e, 1)
    assert rec[0]["score"] > 0 and rec[0]["slot"] == -1                       # untracked: metrics and score, no slot
    assert rec[1].tolist() == (0, 0, 0, -1, 0) and rec[2].tolist() == (0, 0, 0, -1, 0)  # no content: an empty rectangle, a frame outside
    assert rec[3]["score"] == 0 and rec[3]["sharp"] == rec[0]["sharp"] and rec[3]["slot"] == 0 and rec[3]["taken"] == 1  # NaN: c = 0, still a candidate
    out = ref.run(*R.pack(e, TW, TH, True), 1, kept=0)
    assert all(r.tolist() == (0, 0, 0, -1, 0) for r in out) and ref.read(0)[3] == 2


def test_split_invariance_of_the_restatement():
    a = R.scene(0x5401234, 2, 6, 4, TW, TH)
    one = R.ShotsNp(2, 3, TW, TH)
    whole_rec = one.run(*a, max_gap=1)
    three = R.ShotsNp(2, 3, TW, TH)
    got = np.zeros_like(whole_rec)
    for c in range(3):
        sel = np.flatnonzero((a[1]["frame"] >= 4 * c) & (a[1]["frame"] < 4 * c + 4))
        rois = a[1][sel].copy()
        rois["frame"] -= 4 * c
        got[sel] = three.run(a[0][sel], rois, a[2][sel], a[3][sel], a[4][sel], 4, max_gap=1)
    junk = ~((a[1]["frame"] >= 0) & (a[1]["frame"] < 12))
    got["slot"][junk] = -1
    assert got.tobytes() == whole_rec.tobytes() and three.table.tobytes() == one.table.tobytes() and (three.cnt == one.cnt).all()
    live = three.table["state"] != R.FREE
    assert np.array_equal(three.plane[live], one.plane[live])


def test_the_gpu_scenes_exercise_every_path():
    """one further condition, not a measurement: a GPU test cannot pass by exercising nothing"""
    total = {}
    for name, S, slots, tw, th, nhwc, calls in R.gpu_scenes():
        ref = R.ShotsNp(S, slots, tw, th, nhwc)
        for call in calls:
            ref.run(*call[:6], **call[6])
        for k, v in R.summary(ref).items():
            total[k] = total.get(k, 0) + v
        if name in R.CASES:
            need = R.CASES[name]()[6]
            assert all(R.summary(ref)[k] >= 1 for k in need), (name, R.summary(ref))
    assert all(total.get(k, 0) >= 1 for k in ("replaced", "ties", "finished", "lost", "dropped", "duplicates", "overflow")), total
    # ... and the random scenes alone show everything but the overflow, which needs 257 crops in a frame
    total = {}
    for name, S, slots, tw, th, nhwc, calls in R.gpu_scenes():
        if name.startswith("lists-"):
            ref = R.ShotsNp(S, slots, tw, th, nhwc)
            ref.run(*calls[0][:6], **calls[0][6])
            for k, v in R.summary(ref).items():
                total[k] = total.get(k, 0) + v
    assert all(total.get(k, 0) >= 1 for k in ("replaced", "ties", "finished", "lost", "dropped", "duplicates")), total
    for tw, th in R.GEOMETRY:
        a = R.geometry_scene(tw, th, True)
        assert len(a[1]) >= 6 and (a[1]["x1"] > a[1]["x0"]).sum() >= 5
