"""The restatement of include/mars_hip.h, "Events", in Python integers: the literal walk of the header -- float32 only in the anchor,
participants in index order, one step at a time -- and the case tables tests/test_gpu_events.py runs on the device.
tests/test_events_cpu.py pins the restatement on cases worked out by hand and shows that no table is vacuous."""
import numpy as np

F = np.float32
SLOTS, MAX_CAND, MAX_LINES, MAX_ZONES, MAX_VERTS = 256, 256, 32, 32, 8
STREAM_MAJOR, ANCHOR_BOTTOM = 1, 2
DET = np.dtype([("x", "<f4"), ("y", "<f4"), ("w", "<f4"), ("h", "<f4"), ("conf", "<f4"), ("cls", "<i4")])
TRACK = np.dtype([("id", "<i4"), ("hits", "<i4")])
EVENT = np.dtype([("zones", "<u4"), ("entered", "<u4"), ("exited", "<u4"), ("dwelled", "<u4"), ("lines_in", "<u4"), ("lines_out", "<u4")])
SLOT = np.dtype([("id", "<i4"), ("last_step", "<i4"), ("qx", "<i4"), ("qy", "<i4"), ("inside", "<u4"), ("dwelled", "<u4"),
                 ("since", "<i4", (MAX_ZONES,))])
COUNTERS = ("first", "expired", "overflow", "dropped", "duplicates")


# ---- the arithmetic ---------------------------------------------------------------------------------------------------------------------
def quantise(a):
    """float32 -> the anchor's integer: clamp to +-32768, times 16, floor"""
    c = np.minimum(np.maximum(F(a), F(-32768.0)), F(32768.0))
    return int(np.floor(F(c * F(16.0))))


def anchor(d, bottom):
    """(qx, qy) of a DET record; bottom: y + h * 0.5f, the product and the sum rounded on their own"""
    with np.errstate(over="ignore"):
        ay = F(d["y"]) + F(F(d["h"]) * F(0.5)) if bottom else F(d["y"])
    return quantise(d["x"]), quantise(ay)


def cross(ux, uy, vx, vy):
    return ux * vy - uy * vx


def crossing(line, P, Q):
    """line = (ax, ay, bx, by) in sixteenths -> +1: in, -1: out, 0: not crossed"""
    ax, ay, bx, by = line
    sp = cross(bx - ax, by - ay, P[0] - ax, P[1] - ay) >= 0
    sq = cross(bx - ax, by - ay, Q[0] - ax, Q[1] - ay) >= 0
    if sp == sq:
        return 0
    da = cross(Q[0] - P[0], Q[1] - P[1], ax - P[0], ay - P[1]) >= 0
    db = cross(Q[0] - P[0], Q[1] - P[1], bx - P[0], by - P[1]) >= 0
    if da == db:
        return 0
    return 1 if sq else -1


def in_zone(verts, Q):
    """verts in sixteenths, the even-odd crossing number"""
    odd = False
    n = len(verts)
    for e in range(n):
        (vx, vy), (wx, wy) = verts[e], verts[(e + 1) % n]
        if (vy > Q[1]) != (wy > Q[1]):
            d = wy - vy
            lhs, rhs = (Q[0] - vx) * d, (wx - vx) * (Q[1] - vy)
            if (lhs < rhs) if d > 0 else (lhs > rhs):
                odd = not odd
    return odd


def finite(d):
    return bool(np.isfinite(d["x"]) and np.isfinite(d["y"]) and np.isfinite(d["w"]) and np.isfinite(d["h"]))


def stream_step(f, frames, S, major):
    T = frames // S
    return (f // T, f % T) if major else (f % S, f // S)


# ---- the object -------------------------------------------------------------------------------------------------------------------------
class Rules:
    """lines: rows (ax, ay, bx, by) in pixels; zones: pairs (vertices in pixels, dwell)"""

    def __init__(self, lines=(), zones=()):
        self.lines = [tuple(int(v) for v in ln) for ln in lines]
        self.zones = [([(int(x), int(y)) for x, y in verts], int(dwell)) for verts, dwell in zones]
        self.lines16 = [tuple(16 * v for v in ln) for ln in self.lines]
        self.zones16 = [[(16 * x, 16 * y) for x, y in verts] for verts, _ in self.zones]
        self.dwell = [dw for _, dw in self.zones]

    def zones_of(self, Q):
        m = 0
        for z, verts in enumerate(self.zones16):
            if in_zone(verts, Q):
                m |= 1 << z
        return m


class Stream:
    def __init__(self):
        self.slots = [None] * SLOTS  # None, or dict(id, last, q, inside, dwelled, since)
        self.step = 0
        self.line_tot = np.zeros((MAX_LINES, 2), dtype=np.int64)
        self.zone_tot = np.zeros((MAX_ZONES, 4), dtype=np.int64)
        self.cnt = dict.fromkeys(COUNTERS, 0)


class EventsNp:
    def __init__(self, streams):
        self.S = streams
        self.rules = [Rules() for _ in range(streams)]
        self.st = [Stream() for _ in range(streams)]

    def _which(self, stream):
        return range(self.S) if stream < 0 else [stream]

    def reset(self, stream=-1):
        for b in self._which(stream):
            self.st[b] = Stream()

    def set_rules(self, rules, stream=-1):
        for b in self._which(stream):
            self.rules[b] = rules
            self.st[b] = Stream()

    def one_step(self, b, d, tr, n, max_gap, min_hits, bottom, rec, lc, zc):
        """one frame of stream b: d, tr = the frame's rows, rec / lc / zc = the frame's output rows (zero on entry)"""
        s, R = self.st[b], self.rules[b]
        step = s.step
        # 1 expiry
        for k, sl in enumerate(s.slots):
            if sl is not None and step - sl["last"] > max_gap:
                s.cnt["expired"] += 1
                for z in range(MAX_ZONES):
                    if sl["inside"] >> z & 1:
                        s.zone_tot[z, 3] += 1
                s.slots[k] = None
        # participants
        seen, part = set(), []
        for i in range(n):
            if tr[i]["id"] >= 1 and tr[i]["hits"] >= min_hits and finite(d[i]):
                tid = int(tr[i]["id"])
                if tid in seen:
                    s.cnt["duplicates"] += 1
                    continue
                seen.add(tid)
                part.append(i)
        s.cnt["overflow"] += max(0, len(part) - MAX_CAND)
        part = part[:MAX_CAND]
        # 2 lookup
        where = {sl["id"]: k for k, sl in enumerate(s.slots) if sl is not None}
        free = [k for k, sl in enumerate(s.slots) if sl is None]
        for i in part:
            tid = int(tr[i]["id"])
            Q = anchor(d[i], bottom)
            if tid not in where:
                if not free:
                    s.cnt["dropped"] += 1
                    continue
                # 3 first sight
                k = free.pop(0)
                inside = R.zones_of(Q)
                s.slots[k] = dict(id=tid, last=step, q=Q, inside=inside, dwelled=0, since=[0] * MAX_ZONES)
                for z in range(MAX_ZONES):
                    if inside >> z & 1:
                        s.slots[k]["since"][z] = step
                s.cnt["first"] += 1
                rec[i]["zones"] = inside
                continue
            # 4 seen again
            sl = s.slots[where[tid]]
            P = sl["q"]
            lin = lout = 0
            for ln, line in enumerate(R.lines16):
                c = crossing(line, P, Q)
                if c > 0:
                    lin |= 1 << ln
                elif c < 0:
                    lout |= 1 << ln
            now = R.zones_of(Q)
            entered, exited = now & ~sl["inside"], sl["inside"] & ~now
            fired = 0
            for z in range(len(R.zones16)):
                if entered >> z & 1:
                    sl["since"][z] = step
            sl["dwelled"] &= ~(entered | exited)
            for z in range(len(R.zones16)):
                if now >> z & 1 and R.dwell[z] > 0 and step - sl["since"][z] >= R.dwell[z] and not sl["dwelled"] >> z & 1:
                    fired |= 1 << z
                    sl["dwelled"] |= 1 << z
            sl["inside"], sl["q"], sl["last"] = now, Q, step  # 5
            rec[i] = (now, entered, exited, fired, lin, lout)
        # counts and totals
        for i in range(len(rec)):
            r = rec[i]
            if not (r["zones"] | r["entered"] | r["exited"] | r["dwelled"] | r["lines_in"] | r["lines_out"]):
                continue
            for ln in range(MAX_LINES):
                lc[ln, 0] += int(r["lines_in"]) >> ln & 1
                lc[ln, 1] += int(r["lines_out"]) >> ln & 1
            for z in range(MAX_ZONES):
                for j, key in enumerate(("zones", "entered", "exited", "dwelled")):
                    zc[z, j] += int(r[key]) >> z & 1
        s.line_tot += lc
        s.zone_tot[:, :3] += zc[:, 1:]
        s.step += 1

    def run(self, dets, tracks, counts, max_gap=0, min_hits=0, stream_major=False, anchor_bottom=False):
        dets, tracks = np.asarray(dets, dtype=DET), np.asarray(tracks, dtype=TRACK)
        frames, max_det = dets.shape
        assert frames % self.S == 0 and tracks.shape == dets.shape
        rec = np.zeros((frames, max_det), dtype=EVENT)
        lc = np.zeros((frames, MAX_LINES, 2), dtype=np.int32)
        zc = np.zeros((frames, MAX_ZONES, 4), dtype=np.int32)
        T = frames // self.S
        for b in range(self.S):
            for t in range(T):
                f = b * T + t if stream_major else t * self.S + b
                n = min(max(int(counts[f]), 0), max_det)
                self.one_step(b, dets[f], tracks[f], n, max_gap or 30, min_hits or 1, anchor_bottom, rec[f], lc[f], zc[f])
        return rec, lc, zc

    def read(self, b):
        s = self.st[b]
        cnt = np.array([s.cnt[k] for k in COUNTERS], dtype=np.int64)
        return s.line_tot.copy(), s.zone_tot.copy(), cnt, sum(sl is not None for sl in s.slots), s.step

    def read_slots(self, b):
        """canonical: a free slot all zero, since[z] zero for a zone the slot is not inside"""
        out = np.zeros(SLOTS, dtype=SLOT)
        for k, sl in enumerate(self.st[b].slots):
            if sl is None:
                continue
            out[k]["id"], out[k]["last_step"], out[k]["qx"], out[k]["qy"] = sl["id"], sl["last"], sl["q"][0], sl["q"][1]
            out[k]["inside"], out[k]["dwelled"] = sl["inside"], sl["dwelled"]
            for z in range(MAX_ZONES):
                if sl["inside"] >> z & 1:
                    out[k]["since"][z] = sl["since"][z]
        return out


# ---- lists ------------------------------------------------------------------------------------------------------------------------------
def det(x, y, w=8.0, h=8.0, conf=0.9, cls=0):
    return np.array((x, y, w, h, conf, cls), dtype=DET)


def lists(frames, max_det=None):
    """frames: per frame a list of (id, hits, det record) -> (dets, tracks, counts)"""
    width = max_det or max(1, max(len(fr) for fr in frames))
    d = np.zeros((len(frames), width), dtype=DET)
    t = np.zeros((len(frames), width), dtype=TRACK)
    t["id"] = -1
    for f, fr in enumerate(frames):
        for i, (tid, hits, rec) in enumerate(fr):
            d[f, i], t[f, i] = rec, (tid, hits)
    return d, t, np.array([len(fr) for fr in frames], dtype=np.int32)


def walk(rules, points, **kw):
    """one track (id 7) on one stream through `points` ((x, y), (x, y, w, h) or None: not seen in that step) -> (the step's record or
    None, ...), the object"""
    ev = EventsNp(1)
    ev.set_rules(rules)
    frames = [[] if p is None else [(7, 1, det(*p))] for p in points]
    d, t, n = lists(frames, max_det=1)
    rec, _, _ = ev.run(d, t, n, **kw)
    return [None if p is None else tuple(int(v) for v in rec[f, 0]) for f, p in enumerate(points)], ev


# ---- the case tables of the GPU file ----------------------------------------------------------------------------------------------------
# three lines and three zones on a 96 x 64 plane: a vertical gate walked both ways, a diagonal, a short segment most paths miss; a
# rectangle with a dwell of 2 steps, a concave hexagon, a triangle with a dwell of 1
RULES3 = Rules(lines=[(48, 0, 48, 64), (0, 0, 96, 64), (20, 40, 30, 40)],
               zones=[([(10, 10), (40, 10), (40, 30), (10, 30)], 2), ([(50, 5), (90, 5), (90, 60), (70, 30), (50, 60), (50, 40)], 0),
                      ([(30, 35), (60, 35), (45, 60)], 1)])
SHAPES = [(1, 1, False), (1, 5, False), (3, 2, False), (3, 2, True)]  # (S, T, stream major)


def scene(seed, S, T, tracks, max_det, major=False, w=96, h=64, absent=0.15, noise=2):
    """`tracks` ids per stream on random walks over the plane in quarter pixels (so anchors land on rule vertices and lines often), each
    absent from a step now and then; `noise` entries per frame with id -1, too few hits or a non-finite field; the entries shuffled ->
    (dets, tracks, counts) in the call's frame order"""
    rng = np.random.default_rng(seed)
    frames = [None] * (S * T)
    for b in range(S):
        pos = np.stack([rng.integers(0, 4 * w, tracks), rng.integers(0, 4 * h, tracks)], axis=1)
        for t in range(T):
            pos = pos + rng.integers(-60, 61, pos.shape)
            pos[:, 0] = np.clip(pos[:, 0], -8, 4 * w + 8)
            pos[:, 1] = np.clip(pos[:, 1], -8, 4 * h + 8)
            fr = [(k + 1, 1 + t, det(pos[k, 0] / 4.0, pos[k, 1] / 4.0, 6.0 + k % 5, 9.0 + k % 3)) for k in range(tracks) if rng.random() >= absent]
            for k in range(noise):
                kind = (k + t + b) % 3
                fr.append([(-1, 0, det(20.0, 20.0)), (1000 + k, 0, det(20.0, 20.0)), (2000 + k, 3, det(float("nan"), 20.0))][kind])
            fr = [fr[i] for i in rng.permutation(len(fr))]
            frames[b * T + t if major else t * S + b] = fr
    return lists(frames, max_det=max_det)


def many_rules():
    """32 lines and 32 zones of 8 vertices each on the 96 x 64 plane: a fan of gates, and octagons (the odd ones concave) on a grid"""
    lines = [(3 * k, 0, 96 - 3 * k, 64) for k in range(16)] + [(0, 4 * k + 1, 96, 63 - 4 * k) for k in range(16)]
    zones = []
    for k in range(32):
        cx, cy = 6 + 12 * (k % 8), 8 + 16 * (k // 8)
        r, q = 7, (2 if k % 2 else 5)  # q < r / 2: the diagonal vertices pulled in, a concave star
        zones.append(([(cx + r, cy), (cx + q, cy + q), (cx, cy + r), (cx - q, cy + q), (cx - r, cy), (cx - q, cy - q), (cx, cy - r), (cx + q, cy - q)],
                      k % 4))
    return Rules(lines, zones)


def summary(ev, outs):
    """what a run has shown, over every stream: the sums the non-vacuity checks ask about"""
    rec = np.concatenate([o[0].reshape(-1) for o in outs])
    tot = dict(lines_in=int((rec["lines_in"] != 0).sum()), lines_out=int((rec["lines_out"] != 0).sum()), entered=int((rec["entered"] != 0).sum()),
               exited=int((rec["exited"] != 0).sum()), dwelled=int((rec["dwelled"] != 0).sum()), lost=0, used=0)
    for k in COUNTERS:
        tot[k] = 0
    for b in range(ev.S):
        _, zt, cnt, used, _ = ev.read(b)
        tot["lost"] += int(zt[:, 3].sum())
        tot["used"] += used
        for k, v in zip(COUNTERS, cnt):
            tot[k] += int(v)
    return tot


# Every further case: name -> (streams, rules, the calls [(dets, tracks, counts, options)], the summary keys the case is about).  Both test
# files walk this table: the CPU file shows each key non-zero in the restatement, the GPU file compares the device against it.
ZONE_BOX = ([(10, 10), (40, 10), (40, 30), (10, 30)], 2)
GATE = (48, 0, 48, 64)


def case_pressure():
    """256 live ids and one more: dropped; then (max_gap 1) id 1, which sat in the zone, expires out of slot 0 and id 257 takes it"""
    full = [(k, 1, det(20.0 if k == 1 else 60.0, 20.0)) for k in range(1, 257)]
    rest = full[1:] + [(257, 1, det(60.0, 50.0))]
    d, t, n = lists([full, rest, rest], max_det=300)
    return 1, Rules([GATE], [ZONE_BOX]), [(d[:1], t[:1], n[:1], dict(max_gap=1)), (d[1:], t[1:], n[1:], dict(max_gap=1))], ("dropped", "expired", "lost")


def case_overflow():
    """300 tracked entries in one frame: 256 are used"""
    fr = [(k + 1, 2, det(float(k % 96), float(k % 64))) for k in range(300)]
    d, t, n = lists([fr, fr], max_det=300)
    return 1, RULES3, [(d, t, n, {})], ("overflow",)


def case_duplicates():
    """id 5 twice in front of index 256, id 9 at index 1 and again at index 280: the copies do not count towards the cap"""
    fr = [(k + 1, 1, det(float(k % 96), float(k % 64))) for k in range(300)]
    fr[3] = (5, 1, det(90.0, 60.0))
    fr[280] = (9, 1, det(1.0, 1.0))
    moved = [(tid, h, det(float(r["x"]) + 30.0, float(r["y"]))) for tid, h, r in fr]
    d, t, n = lists([fr, moved], max_det=300)
    return 1, RULES3, [(d, t, n, {})], ("duplicates", "overflow", "lines_out")


def case_gap():
    """max_gap 3: id 1 is away for steps 1 and 2 and is judged at step 3 over the whole gap (it crossed the gate and left the zone); id 2
    comes back at step 4, one step too late: expired, lost, a first sight on the far side without a crossing"""
    a0, a1 = (1, 1, det(20.0, 20.0)), (1, 2, det(70.0, 20.0))
    b0, b1 = (2, 1, det(30.0, 25.0)), (2, 2, det(80.0, 25.0))
    d, t, n = lists([[a0, b0], [], [], [a1], [b1]])
    return 1, Rules([GATE], [ZONE_BOX]), [(d, t, n, dict(max_gap=3))], ("lines_out", "exited", "expired", "lost")


def case_dwell():
    """dwell 2: id 1 sits in the zone at step 0, is away and is found there again at step 3: due during the gap, fires on return, once.  id 2
    is inside at 0 and 1, outside at 2, inside from 3 on: the exit clears the stay, the event fires at step 5"""
    a, b_in, b_out = (1, 1, det(20.0, 20.0)), (2, 1, det(30.0, 20.0)), (2, 1, det(60.0, 20.0))
    d, t, n = lists([[a, b_in], [b_in], [b_out], [a, b_in], [a, b_in], [a, b_in], [a, b_in]])
    return 1, Rules([GATE], [ZONE_BOX]), [(d, t, n, {})], ("dwelled", "entered", "exited", "lines_in", "lines_out")


def case_min_hits():
    """min_hits 3: id 1 takes part from its third hit on (x = 50: a first sight, no crossing) and crosses the gate one step later; id 2
    always"""
    frames = [[(1, 1 + s, det(70.0 - 10.0 * s, 20.0)), (2, 5, det(40.0 + 10.0 * s, 40.0))] for s in range(5)]
    d, t, n = lists(frames)
    return 1, Rules([GATE], [ZONE_BOX]), [(d, t, n, dict(min_hits=3))], ("lines_in", "lines_out", "entered")


def case_many_rules():
    d, t, n = scene(0xE7E0321, 2, 6, 40, 48, absent=0.2)
    return 2, many_rules(), [(d, t, n, dict(max_gap=1))], ("lines_in", "lines_out", "entered", "exited", "dwelled", "expired", "lost")


def case_bad_entries():
    """id -1 and 0, NaN and Inf in each of the four fields (conf is not looked at), counts beyond the row and below zero"""
    nan, inf = float("nan"), float("inf")
    bad = [(-1, 1, det(20.0, 20.0)), (0, 1, det(20.0, 20.0)), (11, 1, det(nan, 20.0)), (12, 1, det(20.0, inf)), (13, 1, det(20.0, 20.0, w=-inf)),
           (14, 1, det(20.0, 20.0, h=nan)), (15, 1, det(20.0, 20.0, conf=nan)), (16, 1, det(1e30, -1e30, w=-5.0, h=0.0))]
    moved = [(tid, h, det(60.0, 20.0, float(r["w"]), float(r["h"]), float(r["conf"]))) if tid in (15, 16) else (tid, h, r) for tid, h, r in bad]
    d, t, n = lists([bad, moved, moved, moved], max_det=8)
    n[2], n[3] = 1000, -3
    return 1, Rules([GATE], [ZONE_BOX]), [(d, t, n, {})], ("first", "lines_out", "exited")


def case_anchor_bottom():
    """the foot point: the centre stays above the zone and left of nothing, the bottom edge walks in and out; stream major"""
    frames = [[(1, 1, det(20.0 + 4.0 * s, 4.0, 6.0, 2.0 + 6.0 * (s % 3)))] for s in range(6)]
    d, t, n = lists(frames)
    return 1, Rules([GATE], [([(10, 8), (40, 8), (40, 30), (10, 30)], 1)]), [(d, t, n, dict(anchor_bottom=True, stream_major=True))], ("entered", "exited")


CASES = dict(pressure=case_pressure, overflow=case_overflow, duplicates=case_duplicates, gap=case_gap, dwell=case_dwell, min_hits=case_min_hits,
             many_rules=case_many_rules, bad_entries=case_bad_entries, anchor_bottom=case_anchor_bottom)
