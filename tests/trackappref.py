"""The numpy restatement of "Appearance in tracking" (include/mars_hip.h): Python integers for the embeddings, float32 steps rounded one by
one for the cosine, the literal sorted walk for the association -- written from the header, not from the kernel.  It extends the
restatement of tests/test_track_cpu.py (track_np), counts the events a scene shows, and builds the seeded scenes that
tests/test_track_app_cpu.py pins and tests/test_gpu_track_app.py runs on the device."""
import numpy as np

import cases
from conftest import lcg_frame
from test_track_cpu import DET, MAX_CAND, SLOTS, TRACK, F, TrackerNp, iou_np

APP_THRESH, APP_MIN_IOU = F(0.75), F(0.1)
EVENTS = ("app_low_iou", "key_changed", "gated", "below_thresh", "det_none", "track_none", "null_vec", "smooth", "death_clear", "reuse",
          "match1", "match2", "birth", "death")
NONE_VALUES = (-1, -7, 1 << 30, -(1 << 31))  # row indices that mean "no embedding", beside n_vectors itself


# ---- embeddings ----------------------------------------------------------------------------------------------------------------------------
def quantise_np(v):
    """"Gallery match", Quantisation: int32 values -> (int8 [C], qq) in Python integers; a null vector gives zeros and 0"""
    v = [int(x) for x in np.asarray(v).reshape(-1)]
    m = max(abs(x) for x in v)
    if m == 0:
        return np.zeros(len(v), dtype=np.int8), 0
    q = [(-1 if x < 0 else 1) * ((abs(x) * 127 + m // 2) // m) for x in v]
    return np.array(q, dtype=np.int8), sum(x * x for x in q)


def cosine_np(q, qq, e, ee):
    """cos = ((float)dot * einv) * qinv, every operation rounded to float32 on its own"""
    assert qq > 0 and ee > 0
    dot = sum(int(a) * int(b) for a, b in zip(np.asarray(q).reshape(-1), np.asarray(e).reshape(-1)))
    einv = F(F(1) / np.sqrt(F(ee)))
    qinv = F(F(1) / np.sqrt(F(qq)))
    return F(F(F(dot) * einv) * qinv)


def cosine_matrix_np(e, ee, q, qq):
    """cosine_np of every row of e [nt][C] (ee [nt]) with every row of q [nc][C] (qq [nc]) -> float32 [nt][nc], 0 where a side has no
    embedding: exact integer dots, then the two float32 products element by element"""
    ee, qq = np.asarray(ee, dtype=np.int64).reshape(-1), np.asarray(qq, dtype=np.int64).reshape(-1)
    dot = np.asarray(e, dtype=np.int64).reshape(len(ee), -1) @ np.asarray(q, dtype=np.int64).reshape(len(qq), -1).T
    with np.errstate(all="ignore"):
        einv = (F(1) / np.sqrt(ee.astype(F))).astype(F)
        qinv = (F(1) / np.sqrt(qq.astype(F))).astype(F)
        cs = ((dot.astype(F) * einv[:, None]).astype(F) * qinv[None, :]).astype(F)
    cs[ee <= 0, :] = 0
    cs[:, qq <= 0] = 0
    return cs


def blend_np(e, ee, q, qq):
    """the MARS_TRACK_APP_SMOOTH update of a slot (e, ee) matched to a detection (q, qq) -> (int8 [C], ee)"""
    if qq == 0:
        return (np.array(e, dtype=np.int8), ee) if ee else (np.zeros(len(q), dtype=np.int8), 0)
    if ee == 0:
        return np.array(q, dtype=np.int8), qq
    return quantise_np([3 * int(a) + int(b) for a, b in zip(e, q)])


# ---- the tracker ---------------------------------------------------------------------------------------------------------------------------
class TrackerAppNp(TrackerNp):
    """TrackerNp whose slot dicts also hold e (int8 [C]) and ee (0: none)"""

    def __init__(self, streams, channels):
        self.C = channels
        super().__init__(streams)

    def reset(self):
        super().reset()
        self.events = {k: 0 for k in EVENTS}

    def read_embeddings(self, stream):
        live = [t for t in self.slots[stream] if t is not None]
        q = np.zeros((len(live), self.C), dtype=np.int8)
        for k, t in enumerate(live):
            q[k] = t["e"]
        return q, np.array([t["ee"] for t in live], dtype=np.int32)


def _pass1(slots, tracks, cand, d, emb, thr, any_class, app_thresh, app_min_iou, ev):
    """-> ({slot: detection} under the appearance rule, the same under the plain rule); emb[i] = (q, qq) of detection i"""
    if not tracks or not cand:
        return {}, {}
    a = [np.array([slots[s][k] for s in tracks], dtype=F)[:, None] for k in ("px", "py", "w", "h")]
    b = [d[k][cand].astype(F)[None, :] for k in ("x", "y", "w", "h")]
    iou = iou_np(*a, *b)
    cos = cosine_matrix_np([slots[s]["e"] for s in tracks], [slots[s]["ee"] for s in tracks], [emb[i][0] for i in cand], [emb[i][1] for i in cand])
    pairs, plain = [], []
    for r, s in enumerate(tracks):
        for c, i in enumerate(cand):
            if not (any_class or slots[s]["cls"] == int(d["cls"][i])):
                continue
            v = iou[r, c]
            app = False
            if slots[s]["ee"] > 0 and emb[i][1] > 0:
                cs = cos[r, c]  # cosine_np(emb[i][0], emb[i][1], slots[s]["e"], slots[s]["ee"]), all pairs at once
                if not cs >= app_thresh:
                    ev["below_thresh"] += 1
                elif not v >= app_min_iou:
                    ev["gated"] += 1
                else:
                    app = True
            if v >= thr:  # a NaN fails the comparison
                plain.append((-float(v), s, i))
            if v >= thr or app:
                key = np.fmax(v, cs) if app else v
                pairs.append((-float(key), s, i, bool(app and not v >= thr)))
    got, taken, low = {}, set(), {}
    for _, s, i, by_app in sorted(pairs):
        if s not in got and i not in taken:
            got[s] = i
            low[s] = by_app
            taken.add(i)
    ref, taken = {}, set()
    for _, s, i in sorted(plain):
        if s not in ref and i not in taken:
            ref[s] = i
            taken.add(i)
    ev["app_low_iou"] += sum(low.values())
    ev["key_changed"] += sum(1 for s, i in got.items() if not low[s] and ref.get(s) != i)
    return got, ref


def _pass2(slots, tracks, cand, d, thresh, any_class, taken):
    """the plain rule ("Tracking", Association)"""
    if not tracks or not cand:
        return {}
    a = [np.array([slots[s][k] for s in tracks], dtype=F)[:, None] for k in ("px", "py", "w", "h")]
    b = [d[k][cand].astype(F)[None, :] for k in ("x", "y", "w", "h")]
    iou = iou_np(*a, *b)
    pairs = []
    for r, s in enumerate(tracks):
        for c, i in enumerate(cand):
            if (any_class or slots[s]["cls"] == int(d["cls"][i])) and iou[r, c] >= thresh:
                pairs.append((-float(iou[r, c]), s, i))
    got = {}
    for _, s, i in sorted(pairs):
        if s not in got and i not in taken:
            got[s] = i
            taken.add(i)
    return got


def track_app_np(trk, dets, counts, vectors=None, emb_index=None, idents=None, min_conf=0.0, low_conf=0.0, iou_thresh=0.0, iou_thresh_low=0.0,
                 max_miss=0, classes=None, any_class=False, carry_identity=False, stream_major=False, app_thresh=0.0, app_min_iou=0.0,
                 smooth=False):
    """track_np with embeddings: vectors = int32 [n_vectors][C] or None, emb_index = int [F][max_det]; moves trk on -> TRACK [F][max_det]"""
    dets = np.asarray(dets, dtype=DET)
    nf, max_det = dets.shape
    S, T = trk.S, nf // trk.S
    assert nf % S == 0
    nv = 0 if vectors is None else len(vectors)
    quant = [quantise_np(v) for v in vectors] if nv else []
    trk.events["null_vec"] += sum(1 for q in quant if q[1] == 0)
    none = (np.zeros(trk.C, dtype=np.int8), 0)
    min_conf = F(min_conf) if min_conf else F(0.5)
    low_conf = F(low_conf)
    thr1 = F(iou_thresh) if iou_thresh else F(0.3)
    thr2 = F(iou_thresh_low) if iou_thresh_low else F(0.5)
    app_thresh = F(app_thresh) if app_thresh else APP_THRESH
    app_min_iou = F(app_min_iou) if app_min_iou else APP_MIN_IOU
    max_miss = max_miss if max_miss else 30
    first, count = classes if classes else (0, 0)
    ev = trk.events
    out = np.zeros((nf, max_det), dtype=TRACK)
    out["id"] = -1
    for b in range(S):
        slots = trk.slots[b]
        for t in range(T):
            f = b * T + t if stream_major else t * S + b
            d = dets[f]
            n = min(max(int(counts[f]), 0), max_det)

            def emb_of(i):
                r = int(emb_index[f][i]) if nv and emb_index is not None else -1
                return quant[r] if 0 <= r < nv and quant[r][1] > 0 else none

            emb = {i: emb_of(i) for i in range(n)}
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
            ev["det_none"] += sum(1 for i in H if emb[i][1] == 0)
            ev["track_none"] += sum(1 for s in live if slots[s]["ee"] == 0) if H else 0
            got, _ = _pass1(slots, live, H, d, emb, thr1, any_class, app_thresh, app_min_iou, ev)
            ev["match1"] += len(got)
            taken = set(got.values())
            if low_conf > 0:
                got2 = _pass2(slots, [s for s in live if s not in got], L, d, thr2, any_class, taken)
                ev["match2"] += len(got2)
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
                    q, qq = emb[i]
                    if qq > 0:
                        if smooth and k["ee"] > 0:
                            k["e"], k["ee"] = blend_np(k["e"], k["ee"], q, qq)
                            ev["smooth"] += 1
                        else:
                            k["e"], k["ee"] = q.copy(), qq
                    out[f, i] = (k["id"], k["hits"])
                else:
                    k["x"], k["y"] = k["px"], k["py"]
                    k["miss"] += 1
                    if k["miss"] > max_miss:
                        ev["death_clear"] += k["ee"] > 0
                        slots[s] = None
                        trk.counters[b][1] += 1
                        ev["death"] += 1
            for i in H:
                if i in taken:
                    continue
                free = [s for s in range(SLOTS) if slots[s] is None]
                if not free:
                    trk.counters[b][3] += 1
                    continue
                v = d[i]
                e = idents[f][i] if carry_identity else (-1, F(0))
                q, qq = emb[i]
                slots[free[0]] = dict(id=trk.next_id[b], cls=int(v["cls"]), hits=1, miss=0, x=v["x"], y=v["y"], w=v["w"], h=v["h"], vx=F(0), vy=F(0),
                                      icls=int(e[0]), iscore=F(e[1]), e=q.copy(), ee=qq)
                out[f, i] = (trk.next_id[b], 1)
                trk.next_id[b] += 1
                trk.counters[b][0] += 1
                ev["birth"] += 1
                ev["reuse"] += free[0] in trk.used[b]
                trk.used[b].add(free[0])
    return out


# ---- seeded vectors and scenes -------------------------------------------------------------------------------------------------------------
def rand_vectors(seed, n, c, shift=14):
    """[n][c] int32, every row another direction (magnitudes up to 2^(31 - shift))"""
    return (lcg_frame(seed, n * c * 4).view(np.int32) >> shift).astype(np.int32).reshape(n, c)


APP_SCENE_BOXES = 12
APP_SCENE_STEPS = 4
APP_SCENE_OPTS = dict(max_miss=1)
APP_LOW = 0.2
APP_SCENE_C = (1, 63, 64, 65, 200)
APP_SCENE_S = (1, 3)


def app_scene(seed, streams, channels, stream_major=False, steps=APP_SCENE_STEPS):
    """Twelve objects per stream over `steps` steps (four show every event), 60 x 60 boxes 400 pixels apart unless said otherwise.  Every
    object k has a direction base[k]; a step's vector is 16 * base[k] + a little noise, so a track's cosine with its own object is near 1.
      0, 1   stand 30 apart and at step 2 swap sides by 20 and 10 pixels: the IoU prefers the wrong partner (0.714 against 0.5), the
             cosine the right one -- the appearance key changes the outcome.  Their first channels have opposite signs (C = 1 too)
      2      jumps by 44 pixels at step 2: IoU 0.154 < iou_thresh, >= app_min_iou: taken on appearance alone
      3      jumps by 54: IoU 0.053 < app_min_iou: gated out; the old track coasts and dies at step 3 holding its embedding, the jumped box
             is born
      4      never has an embedding (every value that means none in turn)
      5      brings a null vector
      6      turns its embedding round at step 2: a cosine below app_thresh, matched by the IoU
      7      comes with a confidence between APP_LOW and min_conf from step 1 on: pass 2 (or, without a low set, a death)
      8      has no embedding at step 1: the track keeps the one it has
      9, 10  walk at random
      11     appears at step 3 only: born into the slot a death of that step freed
    The list is rotated by 3 places per step.  -> (DET [streams * steps][16], counts, int32 vectors, emb_index)"""
    boxes, max_det = APP_SCENE_BOXES, 16
    nf = streams * steps
    dets = np.zeros((nf, max_det), dtype=DET)
    counts = np.zeros(nf, dtype=np.int32)
    index = np.full((nf, max_det), -1, dtype=np.int32)
    rows = []  # (frame, detection, vector)
    for b in range(streams):
        s0 = seed + 0x1000 * b
        base = rand_vectors(s0 + 1, boxes, channels, shift=18).astype(np.int64)
        base[:, 0] = np.abs(base[:, 0]) + 1024
        base[1::2, 0] *= -1
        jitter = cases.f32(s0 + 2, 2 * boxes, -2.0, 2.0).reshape(boxes, 2)
        pos = np.array([[100.0 + 400.0 * k, 200.0 + 300.0 * b] for k in range(boxes)], dtype=F)
        pos[1, 0] = pos[0, 0] + F(30)
        pos[2:] += jitter[2:]
        cls = cases.i8(s0 + 3, boxes).astype(np.int32) % 3
        cls[1] = cls[0]
        for t in range(steps):
            if t:
                walk = cases.f32(s0 + 16 + t, 2 * boxes, -3.0, 3.0).reshape(boxes, 2)
                pos[9:11] = (pos[9:11] + walk[9:11]).astype(F)
            if t == 2:
                pos[0, 0] += F(20)
                pos[1, 0] -= F(20)
                pos[2, 0] += F(44)
                pos[3, 0] += F(54)
            conf = cases.f32(s0 + 64 + t, boxes, 0.6, 1.0)
            noise = rand_vectors(s0 + 128 + t, boxes, channels, shift=26).astype(np.int64)  # |noise| < 32
            frame = []
            for k in range(boxes):
                if k == 11 and t != 3:
                    continue
                c = conf[k]
                if k == 7 and t >= 1:
                    c = F(0.3)
                vec = base[k] * 16 + noise[k]
                if k == 6 and t >= 2:
                    vec = -vec
                if k == 5:
                    vec = np.zeros(channels, dtype=np.int64)
                if k == 4 or (k == 8 and t == 1):
                    vec = None
                frame.append(((pos[k, 0], pos[k, 1], F(60), F(60), c, cls[k]), k, vec))
            r = (3 * t) % len(frame)
            frame = frame[r:] + frame[:r]
            f = b * steps + t if stream_major else t * streams + b
            counts[f] = len(frame)
            dets[f, :len(frame)] = np.array([x[0] for x in frame], dtype=DET)
            for i, (_, k, vec) in enumerate(frame):
                if vec is not None:
                    rows.append((f, i, vec.astype(np.int32)))
    # the rows in another order than the detections, one unused row in front; a detection without a vector gets one of the values that mean none
    order = np.argsort(lcg_frame(seed + 7, len(rows)), kind="stable")
    vectors = np.zeros((len(rows) + 1, channels), dtype=np.int32)
    vectors[0] = 12345
    for r, j in enumerate(order):
        f, i, vec = rows[j]
        vectors[r + 1] = vec
        index[f, i] = r + 1
    k = 0
    for f in range(nf):
        for i in range(max_det):
            if index[f, i] < 0:
                index[f, i] = (NONE_VALUES + (len(vectors),))[k % (len(NONE_VALUES) + 1)]
                k += 1
    return dets, counts, vectors, index


def app_scene_list():
    """(seed, streams, channels, stream_major, smooth, low_conf) of every seeded scene the GPU test runs"""
    out = []
    n = 0
    for s in APP_SCENE_S:
        for c in APP_SCENE_C:
            for major in (False, True):
                for smooth in (False, True):
                    for low in (APP_LOW, 0.0):
                        out.append((0x7AA0000 + 0x10000 * n, s, c, major, smooth, low))
            n += 1
    return out


SCENE_EVENTS = ("app_low_iou", "key_changed", "gated", "below_thresh", "det_none", "track_none", "null_vec", "death_clear", "reuse")
