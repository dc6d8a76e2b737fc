"""The restatement of include/mars_hip.h, "Best shots", in Python integers and numpy: the literal walk of the header -- luma, the
Laplacian's mean square, the score, candidates in index order, one step at a time -- and the scenes and case tables
tests/test_gpu_shot.py runs on the device.  tests/test_shot_cpu.py pins the restatement on cases worked out by hand and shows that no
table is vacuous."""
import numpy as np

F = np.float32
MAX_SLOTS, MAX_CAND = 256, 256
STREAM_MAJOR, KEEP_ASPECT, INSIDE = 1, 2, 4
FREE, LIVE, DONE = 0, 1, 2
ROI = np.dtype([("frame", "<i4"), ("det", "<i4"), ("x0", "<i4"), ("y0", "<i4"), ("x1", "<i4"), ("y1", "<i4")])
TRACK = np.dtype([("id", "<i4"), ("hits", "<i4")])
SHOT = np.dtype([("score", "<i8"), ("sharp", "<i4"), ("mean", "<i4"), ("slot", "<i4"), ("taken", "<i4")])
SLOT = np.dtype([("id", "<i4"), ("state", "<i4"), ("first_step", "<i4"), ("last_step", "<i4"), ("best_step", "<i4"), ("seen", "<i4"),
                 ("taken", "<i4"), ("cls", "<i4"), ("conf", "<f4"), ("x0", "<i4"), ("y0", "<i4"), ("x1", "<i4"), ("y1", "<i4"),
                 ("sharp", "<i4"), ("mean", "<i4"), ("pad", "<i4"), ("score", "<i8")])
COUNTERS = ("finished", "lost", "dropped", "overflow", "duplicates", "taken")
SRC_W, SRC_H = 320, 240  # the frames the scenes' rectangles lie in


# ---- the arithmetic ---------------------------------------------------------------------------------------------------------------------
def content_rect(cw, ch, tw, th, keep):
    """-> (nw, nh, px, py): the integer rule of "ROI crops", "Target geometry" """
    if not keep:
        return tw, th, 0, 0
    if cw * th >= ch * tw:
        nw, nh = tw, max(1, (ch * tw + cw // 2) // cw)
    else:
        nw, nh = max(1, (cw * th + ch // 2) // ch), th
    return nw, nh, (tw - nw) // 2, (th - nh) // 2


def luma(u):
    """uint8 [..., 3] -> int64 [...]"""
    u = np.asarray(u).astype(np.int64)
    return (77 * u[..., 0] + 150 * u[..., 1] + 29 * u[..., 2] + 128) >> 8


def laplacian(Y):
    """int64 [h][w] -> L at the pixels with four neighbours, [h - 2][w - 2]"""
    return 4 * Y[1:-1, 1:-1] - Y[1:-1, :-2] - Y[1:-1, 2:] - Y[:-2, 1:-1] - Y[2:, 1:-1]


def metrics(u, rect):
    """u = uint8 [th][tw][3], rect = (nw, nh, px, py) -> (mean, sharp)"""
    nw, nh, px, py = rect
    Y = luma(u)[py:py + nh, px:px + nw]
    mean = int(Y.sum()) // (nw * nh)
    if nw < 3 or nh < 3:
        return mean, 0
    L = laplacian(Y)
    return mean, int((L * L).sum()) // ((nw - 2) * (nh - 2))


def conf_c(conf):
    conf = F(conf)
    if not np.isfinite(conf):
        return 0
    return int(np.floor(F(np.minimum(np.maximum(conf, F(0.0)), F(1.0)) * F(1024.0))))


def score_of(cw, ch, tw, th, sharp, conf):
    return min(cw * ch, tw * th) * (sharp + 1) * conf_c(conf)


def to_u8(crop, tw, th, nhwc):
    """a crop's int8 bytes in its layout -> uint8 [th][tw][3]"""
    x = (np.asarray(crop).reshape(-1).view(np.int8).astype(np.int16) + 128).astype(np.uint8)
    return x.reshape(th, tw, 3) if nhwc else np.ascontiguousarray(x.reshape(3, th, tw).transpose(1, 2, 0))


def from_u8(u, nhwc):
    """uint8 [th][tw][3] -> the crop's int8 bytes in its layout, flat"""
    x = (np.asarray(u).astype(np.int16) - 128).astype(np.int8)
    return x.reshape(-1) if nhwc else np.ascontiguousarray(x.transpose(2, 0, 1)).reshape(-1)


# ---- the object -------------------------------------------------------------------------------------------------------------------------
class ShotsNp:
    def __init__(self, S, slots, tw, th, nhwc=True):
        self.S, self.slots, self.tw, self.th, self.nhwc = S, slots, tw, th, bool(nhwc)
        self.table = np.zeros((S, slots), dtype=SLOT)
        self.plane = np.zeros((S, slots, th, tw, 3), dtype=np.uint8)
        self.step = [0] * S
        self.cnt = np.zeros((S, 6), dtype=np.int64)
        self.replaced = self.ties = 0  # (what the non-vacuity checks ask about; no part of the state)

    def reset(self, b=-1):
        for s in range(self.S) if b < 0 else [b]:
            self.table[s] = np.zeros(self.slots, dtype=SLOT)
            self.step[s] = 0
            self.cnt[s] = 0

    def flush(self, b=-1):
        for s in range(self.S) if b < 0 else [b]:
            live = self.table[s]["state"] == LIVE
            self.table[s]["state"][live] = DONE
            self.cnt[s, 0] += int(live.sum())

    def read(self, b):
        st = self.table[b]["state"]
        return self.cnt[b].copy(), int((st == LIVE).sum()), int((st == DONE).sum()), self.step[b]

    def read_slots(self, b):
        return self.table[b].copy()

    def pixels(self, b, s):
        assert self.table[b, s]["state"] != FREE
        return self.plane[b, s].copy()

    def collect(self, b, cap):
        done = [s for s in range(self.slots) if self.table[b, s]["state"] == DONE]
        take = done[:cap]
        out = (self.table[b, take].copy(), self.plane[b, take].copy(), len(done))
        self.table[b, take] = np.zeros(len(take), dtype=SLOT)
        return out

    def run(self, crops, rois, confs, cls, tracks, frames, max_gap=0, min_hits=0, min_mean=0, max_mean=0, min_sharp=0, src=None,
            stream_major=False, keep_aspect=False, inside=False, kept=None):
        """one entry per crop -> SHOT [n]; the state moves on by `frames` frames"""
        S, tw, th = self.S, self.tw, self.th
        n = len(rois)
        kept = n if kept is None else kept
        assert frames % S == 0
        T = frames // S
        max_gap, min_hits = max_gap or 30, min_hits or 1
        crops = np.asarray(crops).reshape(n, tw * th * 3)
        rec = np.zeros(n, dtype=SHOT)
        rec["slot"] = -1
        info = {}
        for k in range(kept):
            r = rois[k]
            cw, ch = int(r["x1"]) - int(r["x0"]), int(r["y1"]) - int(r["y0"])
            if cw <= 0 or ch <= 0 or not 0 <= int(r["frame"]) < frames:
                continue
            u = to_u8(crops[k], tw, th, self.nhwc)
            mean, sharp = metrics(u, content_rect(cw, ch, tw, th, keep_aspect))
            sc = score_of(cw, ch, tw, th, sharp, confs[k])
            rec[k] = (sc, sharp, mean, -1, 0)
            info[k] = (u, mean, sharp, sc)
        for b in range(S):
            tab = self.table[b]
            for t in range(T):
                f = b * T + t if stream_major else t * S + b
                step = self.step[b]
                for s in range(self.slots):  # 1 expiry
                    if tab[s]["state"] == LIVE and step - int(tab[s]["last_step"]) > max_gap:
                        tab[s]["state"] = DONE
                        self.cnt[b, 0] += 1
                seen_ids, parts = set(), []
                for k in range(kept):
                    if k not in info or int(rois[k]["frame"]) != f:
                        continue
                    _, mean, sharp, _ = info[k]
                    r, tr = rois[k], tracks[k]
                    if int(tr["id"]) < 1 or int(tr["hits"]) < min_hits or sharp < min_sharp:
                        continue
                    if (min_mean or max_mean) and not min_mean <= mean <= max_mean:
                        continue
                    if inside and not (r["x0"] > 0 and r["y0"] > 0 and r["x1"] < src[0] and r["y1"] < src[1]):
                        continue
                    if int(tr["id"]) in seen_ids:
                        self.cnt[b, 4] += 1
                        continue
                    seen_ids.add(int(tr["id"]))
                    parts.append(k)
                self.cnt[b, 3] += max(0, len(parts) - MAX_CAND)
                parts = parts[:MAX_CAND]
                held = {int(tab[s]["id"]): s for s in range(self.slots) if tab[s]["state"] == LIVE}
                free = [s for s in range(self.slots) if tab[s]["state"] == FREE]
                done = [s for s in range(self.slots) if tab[s]["state"] == DONE]
                for k in parts:  # 2 lookup (ascending index)
                    tid = int(tracks[k]["id"])
                    u, mean, sharp, sc = info[k]
                    first = tid not in held
                    if first:
                        if free:
                            s = free.pop(0)
                        elif done:
                            s = done.pop(0)
                            self.cnt[b, 1] += 1
                        else:
                            self.cnt[b, 2] += 1
                            continue
                        tab[s] = np.zeros((), dtype=SLOT)
                        tab[s]["id"], tab[s]["state"], tab[s]["first_step"], tab[s]["seen"], tab[s]["taken"] = tid, LIVE, step, 1, 1
                        store = True
                    else:
                        s = held[tid]
                        tab[s]["seen"] += 1
                        store = sc > int(tab[s]["score"])
                        if store:
                            tab[s]["taken"] += 1
                            self.replaced += 1
                        elif sc == int(tab[s]["score"]):
                            self.ties += 1
                    if store:
                        r = rois[k]
                        for key in ("x0", "y0", "x1", "y1"):
                            tab[s][key] = r[key]
                        tab[s]["cls"], tab[s]["conf"] = cls[k], F(confs[k])
                        tab[s]["sharp"], tab[s]["mean"], tab[s]["score"], tab[s]["best_step"] = sharp, mean, sc, step
                        self.plane[b, s] = u
                        self.cnt[b, 5] += 1
                    tab[s]["last_step"] = step
                    rec[k]["slot"], rec[k]["taken"] = s, int(store)
                self.step[b] = step + 1
        return rec


# ---- scenes -----------------------------------------------------------------------------------------------------------------------------
def box_blur(u, k):
    """uint8 [h][w][3] -> its k x k box mean (edges repeated), k odd"""
    if k <= 1:
        return u.copy()
    h, w, _ = u.shape
    p = np.pad(u.astype(np.int64), ((k // 2, k // 2), (k // 2, k // 2), (0, 0)), mode="edge")
    acc = np.zeros((h, w, 3), dtype=np.int64)
    for dy in range(k):
        for dx in range(k):
            acc += p[dy:dy + h, dx:dx + w]
    return (acc // (k * k)).astype(np.uint8)


def pack(entries, tw, th, nhwc):
    """entries: (frame, id, hits, conf, cls, (x0, y0, x1, y1), uint8 [th][tw][3]) per crop -> (crops, rois, confs, cls, tracks)"""
    n = len(entries)
    crops = np.zeros((n, tw * th * 3), dtype=np.int8)
    rois, tracks = np.zeros(n, dtype=ROI), np.zeros(n, dtype=TRACK)
    confs, cls = np.zeros(n, dtype=np.float32), np.zeros(n, dtype=np.int32)
    for k, (f, tid, hits, conf, c, rect, u) in enumerate(entries):
        crops[k] = from_u8(u, nhwc)
        rois[k] = (f, k % 7, rect[0], rect[1], rect[2], rect[3])
        tracks[k], confs[k], cls[k] = (tid, hits), conf, c
    return crops, rois, confs, cls, tracks


SHAPES = [(1, 1, False), (1, 5, False), (3, 2, False), (3, 2, True)]  # (S, T, stream major)


def scene(seed, S, T, ntracks, tw, th, nhwc=True, major=False, absent=0.25, noise=2, repeat=0.3, dup=0.15):
    """`ntracks` ids per stream, each with a texture of its own that is blurred by a k x k box mean (k drawn per step, so sharpness
    varies), a rectangle that drifts, and a confidence from a short list (so scores tie now and then).  A track is absent from a step
    now and then, ends for good at a step of its own, and now and then shows exactly the crop of its last appearance again (a tie).
    Now and then an id comes twice in a frame.  `noise` crops per frame take no part: id -1, too few hits, an empty rectangle, a frame
    outside the call, a NaN confidence.  The crops are shuffled -> (crops, rois, confs, cls, tracks, frames)"""
    rng = np.random.default_rng(seed)
    entries = []
    for b in range(S):
        tex = rng.integers(0, 256, (ntracks, th, tw, 3), dtype=np.uint8)
        ends = rng.integers(max(1, T // 2), T + 3, ntracks)
        last = [None] * ntracks
        for t in range(T):
            f = b * T + t if major else t * S + b
            for i in range(ntracks):
                if t >= ends[i] or rng.random() < absent:
                    continue
                if last[i] is not None and rng.random() < repeat:
                    conf, rect, u = last[i]
                else:
                    x0, y0 = int(rng.integers(0, SRC_W - 8)), int(rng.integers(0, SRC_H - 8))
                    cw, ch = int(rng.integers(2, 3 * tw + 8)), int(rng.integers(2, 3 * th + 8))
                    rect = (x0, y0, min(x0 + cw, SRC_W), min(y0 + ch, SRC_H))
                    u = box_blur(tex[i], int(rng.choice([1, 1, 3, 5])))
                    u = np.clip(u.astype(np.int64) + int(rng.integers(-40, 41)), 0, 255).astype(np.uint8)
                    conf = float(rng.choice([0.3, 0.5, 0.5, 0.75, 0.9, 1.0]))
                last[i] = (conf, rect, u)
                entries.append((f, 1 + i + 100 * b, 1 + t, conf, i % 5, rect, u))
                if rng.random() < dup:
                    entries.append((f, 1 + i + 100 * b, 1 + t, 0.9, 9, rect, tex[i]))
            flat = rng.integers(0, 256, (th, tw, 3), dtype=np.uint8)
            for k in range(noise):
                kind = (k + t + b) % 5
                entries.append([(f, -1, 0, 0.9, 0, (5, 5, 60, 60), flat), (f, 1000 + k, 0, 0.9, 0, (5, 5, 60, 60), flat),
                                (f, 2000 + k, 3, 0.9, 0, (40, 40, 40, 90), flat), (S * T + k, 3000 + k, 3, 0.9, 0, (5, 5, 60, 60), flat),
                                (f, 4000 + k, 3, float("nan"), 0, (5, 5, 60, 60), flat)][kind])
    entries = [entries[i] for i in rng.permutation(len(entries))]
    return pack(entries, tw, th, nhwc) + (S * T,)


# the targets at which the band cut, the halo, the 16-byte path and the interior rule can each go wrong: (tw, th)
GEOMETRY = [(1, 1), (2, 2), (3, 3), (5, 4), (17, 13), (200, 3), (64, 64), (160, 160)]


def geometry_scene(tw, th, nhwc):
    """two streams, two steps, a few tracks (fewer at the large targets: the restatement is Python)"""
    big = tw * th >= 64 * 64
    return scene(0x5407000 + 1000 * tw + th, 2, 2, 2 if big else 4, tw, th, nhwc, absent=0.1, noise=1)


def summary(ref):
    tot = dict(replaced=ref.replaced, ties=ref.ties)
    for i, k in enumerate(COUNTERS):
        tot[k] = int(ref.cnt[:, i].sum())
    return tot


# ---- the case tables of the GPU file ----------------------------------------------------------------------------------------------------
# name -> (streams, slots, tw, th, nhwc, the calls [(crops, rois, confs, cls, tracks, frames, options)], the summary keys the case is about)
def _tex(seed, tw, th):
    return np.random.default_rng(seed).integers(0, 256, (th, tw, 3), dtype=np.uint8)


def case_pressure():
    """4 slots, 6 ids: two are dropped; then (max_gap 1) everything expires, ids 7 and 8 overwrite the two lowest DONE slots"""
    tw, th = 8, 8
    u = [_tex(0x5408000 + i, tw, th) for i in range(9)]
    e = [(0, i, 1, 0.9, 0, (10, 10, 30, 30), u[i]) for i in range(1, 7)] + [(3, i, 1, 0.9, 0, (10, 10, 30, 30), u[i]) for i in (7, 8)]
    return 1, 4, tw, th, True, [pack(e, tw, th, True) + (4, dict(max_gap=1))], ("dropped", "finished", "lost")


def case_overflow():
    """300 tracked crops of 4 x 4 in one frame: 256 take part; index 280 repeats an id of the first 256 and is a duplicate, no overflow"""
    tw, th = 4, 4
    e = [(0, k + 1, 2, 0.5, 0, (k % 50, k % 40, k % 50 + 6, k % 40 + 7), _tex(0x5409000 + k, tw, th)) for k in range(300)]
    e[280] = (0, 9, 2, 0.5, 0, (1, 1, 9, 9), _tex(0x5409FFF, tw, th))
    return 1, 256, tw, th, False, [pack(e, tw, th, False) + (1, {})], ("overflow", "duplicates")


def case_tie_and_replace():
    """one id over 5 steps: the same crop twice (a tie: the older stays), a blurred one (lower), the sharp one at a higher confidence
    (replaces), and once more the same (a tie again)"""
    tw, th = 16, 12
    u = _tex(0x540A000, tw, th)
    seq = [(u, 0.5), (u, 0.5), (box_blur(u, 3), 0.5), (u, 0.75), (u, 0.75)]
    e = [(t, 7, 1 + t, conf, t, (20 + t, 20, 60 + t, 70), x) for t, (x, conf) in enumerate(seq)]
    return 1, 2, tw, th, True, [pack(e, tw, th, True) + (5, {})], ("ties", "replaced")


def case_gates():
    """min_hits 3, a mean window, min_sharp and MARS_SHOT_INSIDE, one crop failing each, one passing all; stream major"""
    tw, th = 12, 12
    u = _tex(0x540B000, tw, th)
    dark = (u // 8).astype(np.uint8)
    flat = np.full((th, tw, 3), 128, dtype=np.uint8)
    e = [(0, 1, 2, 0.9, 0, (10, 10, 40, 40), u), (0, 2, 3, 0.9, 0, (10, 10, 40, 40), dark), (0, 3, 3, 0.9, 0, (10, 10, 40, 40), flat),
         (0, 4, 3, 0.9, 0, (0, 10, 40, 40), u), (0, 5, 3, 0.9, 0, (10, 10, 40, SRC_H), u), (0, 6, 3, 0.9, 0, (10, 10, 40, 40), u),
         (1, 6, 4, 1.0, 0, (10, 10, 40, 40), u)]
    opts = dict(min_hits=3, min_mean=60, max_mean=200, min_sharp=50, inside=True, src=(SRC_W, SRC_H), stream_major=True)
    return 1, 8, tw, th, False, [pack(e, tw, th, False) + (2, opts)], ("replaced", "taken")


def case_long_gap():
    """max_gap 3: id 1 away for steps 1 .. 3 and back at 4, one step too late: its slot is DONE and a FREE slot is taken before it"""
    tw, th = 6, 5
    u = _tex(0x540C000, tw, th)
    e = [(0, 1, 1, 0.9, 0, (10, 10, 40, 40), u), (4, 1, 2, 0.9, 0, (10, 10, 40, 40), u), (3, 2, 1, 0.9, 0, (10, 10, 40, 40), u)]
    return 1, 3, tw, th, True, [pack(e, tw, th, True) + (6, dict(max_gap=3))], ("finished",)


CASES = dict(pressure=case_pressure, overflow=case_overflow, tie_and_replace=case_tie_and_replace, gates=case_gates, long_gap=case_long_gap)


def gpu_scenes():
    """every (name, streams, slots, tw, th, nhwc, calls) the GPU file feeds the device besides the geometry table: the non-vacuity
    check of tests/test_shot_cpu.py walks the same list"""
    out = []
    for S, T, major in SHAPES:
        out.append(("lists-S%d-T%d%s" % (S, T, "-major" if major else ""), S, 3, 10, 9, True,
                    [scene(0x5400000 + 16 * S + T, S, T, 5, 10, 9, True, major) + (dict(max_gap=1, stream_major=major),)]))
    for name in sorted(CASES):
        S, slots, tw, th, nhwc, calls, _ = CASES[name]()
        out.append((name, S, slots, tw, th, nhwc, calls))
    return out
