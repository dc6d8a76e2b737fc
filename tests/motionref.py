"""The numpy restatement of include/mars_hip.h "Motion" (luma, cell means, the step, the filter, the map words, the statistics, the zones, the
detections), and nothing else: no import from the library.  The rectangle rule is the float32 one restated in tests/test_roi_cpu.py.
tests/test_motion_cpu.py pins it on hand-computed cases; tests/test_gpu_motion.py compares the device against it.  Also the scene generator
and the case tables of the GPU tests, which are functions of their arguments alone, so the CPU file can check that no GPU case is vacuous."""
import numpy as np

from test_roi_cpu import roi_rect_np

RGB, NV12 = 0, 1
STREAM_MAJOR, FRAME_DIFF = 1, 2
MAX_ZONES = 64
STATS = np.dtype([("active", "<i4"), ("x0", "<i4"), ("y0", "<i4"), ("x1", "<i4"), ("y1", "<i4"), ("first", "<i4")])
DET = np.dtype([("active", "<i4"), ("cells", "<i4")])


def frame_bytes(W, H, fmt):
    return W * H * 3 // (2 if fmt == NV12 else 1)


def grid(W, H, B):
    """-> (gw, gh, pitch)"""
    gw, gh = (W + B - 1) // B, (H + B - 1) // B
    return gw, gh, (gw + 31) // 32


def luma_np(frame, W, H, fmt):
    """one frame's bytes -> int64 [H][W]"""
    a = np.asarray(frame, dtype=np.uint8).reshape(-1).astype(np.int64)
    if fmt == NV12:
        return a[:W * H].reshape(H, W)
    p = a.reshape(H, W, 3)
    return (77 * p[..., 0] + 150 * p[..., 1] + 29 * p[..., 2] + 128) >> 8


def cell_count_np(W, H, B):
    ys, xs = np.arange(0, H, B), np.arange(0, W, B)
    return (np.minimum(ys + B, H) - ys)[:, None] * (np.minimum(xs + B, W) - xs)[None, :]


def cell_means_np(luma, B):
    """int64 [H][W] -> the 8.8 means, int64 [gh][gw]"""
    H, W = luma.shape
    S = np.add.reduceat(np.add.reduceat(luma, np.arange(0, H, B), axis=0), np.arange(0, W, B), axis=1)
    n = cell_count_np(W, H, B)
    return (256 * S + n // 2) // n


def step_np(bg, init, m, threshold=0, learn=0, learn_active=0, frame_diff=False):
    """one step of one stream: (bg or None, initialised, the means) -> (raw bool [gh][gw], the new bg)"""
    if not init:
        return np.zeros(m.shape, dtype=bool), m.copy()
    delta = m - bg
    ad = np.abs(delta)
    raw = ad > 256 * (threshold or 8)
    if frame_diff:
        return raw, m.copy()
    k = np.where(raw, learn_active or 8, learn or 4)
    return raw, bg + np.sign(delta) * (ad >> k)


def filter_np(raw, min_neighbors):
    gh, gw = raw.shape
    p = np.zeros((gh + 2, gw + 2), dtype=np.int64)
    p[1:-1, 1:-1] = raw
    nbr = sum(p[1 + dy:1 + dy + gh, 1 + dx:1 + dx + gw] for dy in (-1, 0, 1) for dx in (-1, 0, 1) if (dy, dx) != (0, 0))
    return raw & (nbr >= min_neighbors)


def pack_np(active):
    """bool [gh][gw] -> uint32 [gh][pitch]"""
    gh, gw = active.shape
    pitch = (gw + 31) // 32
    bits = np.zeros((gh, pitch * 32), dtype=np.uint64)
    bits[:, :gw] = active
    return (bits.reshape(gh, pitch, 32) << np.arange(32, dtype=np.uint64)).sum(axis=2).astype(np.uint32)


def unpack_np(words, gw):
    w = np.asarray(words, dtype=np.uint32)
    bits = (w[..., :, None] >> np.arange(32, dtype=np.uint32)) & 1
    return bits.reshape(w.shape[:-1] + (-1,))[..., :gw].astype(bool)


def stats_np(active, W, H, B, first):
    ys, xs = np.nonzero(active)
    if len(xs) == 0:
        return (0, 0, 0, 0, 0, int(first))
    return (len(xs), int(xs.min()) * B, int(ys.min()) * B, min(W, (int(xs.max()) + 1) * B), min(H, (int(ys.max()) + 1) * B), int(first))


def rect_count_np(active, rect, B):
    """(active cells, cells) of the cell range of a half-open pixel rectangle"""
    x0, y0, x1, y1 = (int(v) for v in rect)
    sub = active[y0 // B:(y1 - 1) // B + 1, x0 // B:(x1 - 1) // B + 1]
    return int(sub.sum()), int(sub.size)


def det_np(active, box, W, H, B, expand=0.0):
    r = roi_rect_np(box, W, H, expand, 1)
    return (0, 0) if r is None else rect_count_np(active, r, B)


def stream_step(f, F, S, stream_major):
    T = F // S
    return (f // T, f % T) if stream_major else (f % S, f // S)


class Detector:
    """the state of S streams and the whole call"""

    def __init__(self, S, W, H, fmt, B):
        self.S, self.W, self.H, self.fmt, self.B = S, W, H, fmt, B
        self.gw, self.gh, self.pitch = grid(W, H, B)
        self.bg = np.zeros((S, self.gh, self.gw), dtype=np.int64)
        self.init = np.zeros(S, dtype=bool)
        self.active = self.raw = None

    def reset(self, stream=-1):
        sel = slice(None) if stream < 0 else stream
        self.bg[sel] = 0
        self.init[sel] = False

    def run(self, frames, threshold=0, learn=0, learn_active=0, min_neighbors=0, flags=0, zones=()):
        """frames uint8 [F][frame bytes] -> (maps uint32 [F][gh][pitch], STATS [F], zone counts int32 [F][len(zones)])"""
        frames = np.asarray(frames, dtype=np.uint8).reshape(-1, frame_bytes(self.W, self.H, self.fmt))
        F = len(frames)
        assert F % self.S == 0
        maps = np.zeros((F, self.gh, self.pitch), dtype=np.uint32)
        stats = np.zeros(F, dtype=STATS)
        zc = np.zeros((F, len(zones)), dtype=np.int32)
        self.raw = np.zeros((F, self.gh, self.gw), dtype=bool)
        self.active = np.zeros((F, self.gh, self.gw), dtype=bool)
        order = sorted(range(F), key=lambda f: stream_step(f, F, self.S, bool(flags & STREAM_MAJOR))[::-1])  # by step, then stream
        for f in order:
            s, _ = stream_step(f, F, self.S, bool(flags & STREAM_MAJOR))
            m = cell_means_np(luma_np(frames[f], self.W, self.H, self.fmt), self.B)
            first = not self.init[s]
            raw, self.bg[s] = step_np(self.bg[s], self.init[s], m, threshold, learn, learn_active, bool(flags & FRAME_DIFF))
            self.init[s] = True
            act = filter_np(raw, min_neighbors)
            self.raw[f], self.active[f] = raw, act
            maps[f] = pack_np(act)
            stats[f] = stats_np(act, self.W, self.H, self.B, first)
            zc[f] = [rect_count_np(act, z, self.B)[0] for z in zones]
        return maps, stats, zc

    def boxes(self, boxes, frame_of_box, expand=0.0):
        """against the maps of the last run -> DET [n]"""
        out = np.zeros(len(boxes), dtype=DET)
        for i, (b, f) in enumerate(zip(boxes, frame_of_box)):
            if 0 <= f < len(self.active):
                out[i] = det_np(self.active[f], b, self.W, self.H, self.B, expand)
        return out


# ---- the scenes and cases of the GPU tests ------------------------------------------------------------------------------------------------------
RGB_SIZES = [(2, 2), (31, 17), (33, 45), (65, 66), (257, 130)]    # the redaction tests' lists: rows of no repeating alignment, one pixel past a
NV12_SIZES = [(2, 2), (34, 18), (66, 130), (128, 64), (258, 130)]  # tile, three tile rows, single-cell grids
CELLS = [4, 16, 64]
STREAMS_STEPS = [(1, 1, 0), (1, 5, 0), (3, 2, 0), (3, 2, STREAM_MAJOR)]  # (S, T, flags)


def has_block(W, H, B):
    gw, gh, _ = grid(W, H, B)
    return gw >= 3 and gh >= 3


def case_min_neighbors(W, H, B):
    """grids of at least 3 x 3 cells run with the filter, smaller ones without"""
    return 1 if has_block(W, H, B) else 0


def scene(seed, S, T, W, H, fmt, B):
    """-> uint8 [T][S][frame bytes].  Per stream a fixed random base image of values 1 .. 127; noise of +-1 per step; from step 1 on, on grids of
    at least 3 x 3 cells, a block of about a third of each axis, 120 levels brighter, that hugs the right edge (the clipped column, where
    there is one), moves every step and stays two cell rows above the last one; from step 1 on, on odd steps, a flash of 100 levels confined
    to the last corner cell.  The block never touches a neighbour of that cell, so the filter removes the flash."""
    gw, gh, _ = grid(W, H, B)
    out = np.zeros((T, S, frame_bytes(W, H, fmt)), dtype=np.uint8)
    C = 1 if fmt == NV12 else 3
    bw, bh = max(W // 3, 1), max(min(H // 3, (gh - 2) * B), 1)
    for s in range(S):
        rng = np.random.default_rng([seed, s])
        base = rng.integers(1, 128, (H, W, C)).astype(np.int64)
        chroma = rng.integers(0, 256, W * H // 2, dtype=np.uint8)
        for t in range(T):
            img = base + rng.integers(-1, 2, base.shape)
            if t >= 1 and has_block(W, H, B):
                y0 = min((t - 1) * max(B // 2, 1), (gh - 2) * B - bh)
                x0 = W - bw - (t + 1) % 2
                img[y0:y0 + bh, x0:x0 + bw] += 120
            if t % 2 == 1:
                img[(gh - 1) * B:, (gw - 1) * B:] += 100
            assert img.min() >= 0 and img.max() <= 255
            plane = img.astype(np.uint8).reshape(-1)
            out[t, s] = np.concatenate([plane, chroma]) if fmt == NV12 else plane
    return out


def in_order(scene_ts, stream_major):
    """[T][S][bytes] -> the frames in the order of a call: [F][bytes]"""
    a = scene_ts.transpose(1, 0, 2) if stream_major else scene_ts
    return np.ascontiguousarray(a).reshape(-1, scene_ts.shape[2])


def case_zones(W, H, B, n=MAX_ZONES, seed=0):
    """n zones: a single pixel, the whole frame, one ending on a cell border (where the frame has one), random ones"""
    rng = np.random.default_rng([seed, W, H, B])
    z = [(W - 1, H - 1, W, H), (0, 0, W, H), (0, 0, min(B, W), min(B, H))]
    while len(z) < n:
        x0, y0 = int(rng.integers(0, W)), int(rng.integers(0, H))
        z.append((x0, y0, int(rng.integers(x0 + 1, W + 1)), int(rng.integers(y0 + 1, H + 1))))
    return np.array(z[:n], dtype=np.int32)


def not_vacuous(det, W, H, B, T):
    """det: a Detector after the run of a scene of T >= 2 steps.  Grids of at least 3 x 3 cells: some cell is active, some is inactive, some raw
    cell is removed by the filter, and -- where the grid has a clipped cell at all -- some clipped edge cell is active.  Smaller grids (run
    without the filter): some frame has an active cell and some has none."""
    act, raw = det.active, det.raw
    if not has_block(W, H, B):
        per = act.reshape(len(act), -1).any(axis=1)
        return bool(per.any() and not per.all())
    clipped = cell_count_np(W, H, B) < B * B
    return bool(act.any() and not act.all() and (raw & ~act).any() and (not clipped.any() or (act & clipped).any()))
