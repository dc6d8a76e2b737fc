"""numpy restatement of include/mars_hip.h, "Tiled inference": grid, geometry, map, rules, order, suppression, counters.  float32 arithmetic one
operation at a time (numpy float32 arrays round every operation on its own); the resize itself is roi_crop_np of tests/test_roi_cpu.py.
tests/test_tile_cpu.py checks this file against cases worked out by hand, tests/test_gpu_tile.py compares the device against it byte for byte."""
import numpy as np

from test_roi_cpu import nv12_to_rgb_np, roi_crop_np, roi_target_np

F = np.float32
MAX_DET, MAX_TILES, MAX_CAND = 1000, 64, 2048
KEEP_ASPECT, MATCH_IOS, AGNOSTIC = 1, 2, 4
DET = np.dtype([("x", "<f4"), ("y", "<f4"), ("w", "<f4"), ("h", "<f4"), ("conf", "<f4"), ("cls", "<i4")])
SRC = np.dtype([("tile", "<i4"), ("det", "<i4")])
STATS = np.dtype([("candidates", "<i4"), ("overflow", "<i4"), ("invalid", "<i4"), ("edge", "<i4"), ("suppressed", "<i4"), ("truncated", "<i4")])


def axis(W, tile, overlap):
    """the starts of one axis"""
    if tile >= W:
        return [0]
    step = tile - overlap
    starts, k = [], 0
    while k * step + tile < W:
        starts.append(k * step)
        k += 1
    return starts + [W - tile]


def grid(W, H, tile_w, tile_h, overlap_x=0, overlap_y=0):
    """-> [(x0, y0, x1, y1)] row-major, or -1 where mars_tile_grid returns -1"""
    if W <= 0 or H <= 0 or tile_w <= 0 or tile_h <= 0 or overlap_x < 0 or overlap_y < 0 or overlap_x >= tile_w or overlap_y >= tile_h:
        return -1
    tw, th = min(tile_w, W), min(tile_h, H)
    return [(x, y, x + tw, y + th) for y in axis(H, tile_h, overlap_y) for x in axis(W, tile_w, overlap_x)]


def tile_frames(frames, tiles, tw, th, nhwc=True, keep_aspect=False):
    """uint8 RGB frames [n][H][W][3] -> int8 [n * T][tw * th * 3]: tile t of frame c at row c * T + t"""
    return np.stack([roi_crop_np(f, tuple(int(v) for v in t), tw, th, nhwc, keep_aspect) for f in frames for t in tiles])


def tile_frames_nv12(frames, w, h, flags, tiles, tw, th, nhwc=True, keep_aspect=False):
    """NV12 frames [n][w * h * 3 / 2]: an NV12 tile equals the RGB tile of the converted frame"""
    return tile_frames([nv12_to_rgb_np(f, w, h, flags) for f in frames], tiles, tw, th, nhwc, keep_aspect)


def quota(n_tiles, max_per_tile=0):
    return max_per_tile if max_per_tile else min(MAX_DET, MAX_CAND // n_tiles)


def ord_key(conf):
    """finite float32 -> uint32 in the same order (-0 below +0)"""
    u = np.asarray(conf, dtype=F).view(np.uint32)
    return np.where(u & np.uint32(0x80000000), ~u, u | np.uint32(0x80000000)).astype(np.uint32)


def map_tile(d, tile, tw, th, keep_aspect):
    """entries of one tile (DET records, valid ones) -> X, Y, Wd, Hd as float32 arrays"""
    x0, y0, x1, y1 = (int(v) for v in tile)
    nw, nh, px, py = roi_target_np(x1 - x0, y1 - y0, tw, th, keep_aspect)
    rx, ry = F(x1 - x0) / F(nw), F(y1 - y0) / F(nh)
    with np.errstate(over="ignore", invalid="ignore"):
        X = (d["x"] - F(px)) * rx + F(x0)
        Y = (d["y"] - F(py)) * ry + F(y0)
        return X.astype(F), Y.astype(F), (d["w"] * rx).astype(F), (d["h"] * ry).astype(F)


def match(ax, ay, aw, ah, bx, by, bw, bh, ios):
    """m(a, b) of one box a against arrays b, float32, the expressions of the detection tail"""
    two, eps = F(2), F(1e-6)
    with np.errstate(over="ignore", invalid="ignore", divide="ignore"):
        x1 = np.fmax(ax - aw / two, bx - bw / two)
        y1 = np.fmax(ay - ah / two, by - bh / two)
        x2 = np.fmin(ax + aw / two, bx + bw / two)
        y2 = np.fmin(ay + ah / two, by + bh / two)
        inter = np.fmax(F(0), x2 - x1) * np.fmax(F(0), y2 - y1)
        aarea, barea = aw * ah, bw * bh
        den = np.fmin(aarea, barea) if ios else (aarea + barea) - inter
        return inter / (den + eps)


def merge_one(lists, tiles, src_w, src_h, tw, th, flags=0, merge_thresh=0.0, edge_margin=0.0, max_per_tile=0):
    """lists: T record arrays (the tiles' lists, already cut to their counts) -> (DET [MAX_DET], count, SRC [MAX_DET], STATS scalar)"""
    T = len(tiles)
    assert len(lists) == T and 1 <= T <= MAX_TILES
    q = quota(T, max_per_tile)
    assert T * q <= MAX_CAND
    thresh = F(merge_thresh) if merge_thresh else F(0.5)
    margin = F(edge_margin)
    st = np.zeros((), dtype=STATS)
    cx, cy, cw, ch, cc, ck, ct, ci = [], [], [], [], [], [], [], []
    for t, (d, tile) in enumerate(zip(lists, tiles)):
        d = np.asarray(d, dtype=DET)
        st["overflow"] += max(len(d) - q, 0)
        d = d[:q]
        idx = np.arange(len(d))
        ok = np.isfinite(d["x"]) & np.isfinite(d["y"]) & np.isfinite(d["w"]) & np.isfinite(d["h"]) & np.isfinite(d["conf"]) & (d["w"] > 0) & (d["h"] > 0)
        st["invalid"] += int((~ok).sum())
        d, idx = d[ok], idx[ok]
        X, Y, Wd, Hd = map_tile(d, tile, tw, th, bool(flags & KEEP_ASPECT))
        if margin > 0:
            x0, y0, x1, y1 = (int(v) for v in tile)
            half = F(0.5)
            with np.errstate(over="ignore", invalid="ignore"):
                l, r, tp, bt = X - Wd * half, X + Wd * half, Y - Hd * half, Y + Hd * half
                cut = np.zeros(len(d), dtype=bool)
                if x0 > 0:
                    cut |= (l - F(x0)) < margin
                if x1 < src_w:
                    cut |= (F(x1) - r) < margin
                if y0 > 0:
                    cut |= (tp - F(y0)) < margin
                if y1 < src_h:
                    cut |= (F(y1) - bt) < margin
            st["edge"] += int(cut.sum())
            X, Y, Wd, Hd, d, idx = X[~cut], Y[~cut], Wd[~cut], Hd[~cut], d[~cut], idx[~cut]
        cx.append(X); cy.append(Y); cw.append(Wd); ch.append(Hd); cc.append(d["conf"]); ck.append(d["cls"])
        ct.append(np.full(len(d), t, dtype=np.int32)); ci.append(idx.astype(np.int32))
    X, Y, Wd, Hd, conf = (np.concatenate(v).astype(F) for v in (cx, cy, cw, ch, cc))
    cls, tile_of, det_of = np.concatenate(ck).astype(np.int32), np.concatenate(ct), np.concatenate(ci)
    n = len(X)
    st["candidates"] = n
    order = np.lexsort((np.arange(n), -ord_key(conf).astype(np.int64)))  # confidence descending, then k ascending
    X, Y, Wd, Hd, conf, cls, tile_of, det_of = (v[order] for v in (X, Y, Wd, Hd, conf, cls, tile_of, det_of))
    removed = np.zeros(n, dtype=bool)
    ios, agnostic = bool(flags & MATCH_IOS), bool(flags & AGNOSTIC)
    for a in range(n):
        if removed[a] or a + 1 == n:
            continue
        s = slice(a + 1, n)
        m = match(X[a], Y[a], Wd[a], Hd[a], X[s], Y[s], Wd[s], Hd[s], ios)
        hit = (tile_of[s] != tile_of[a]) & (m > thresh)
        if not agnostic:
            hit &= cls[s] == cls[a]
        removed[s] |= hit
    keep = np.flatnonzero(~removed)
    st["suppressed"] = n - len(keep)
    st["truncated"] = max(len(keep) - MAX_DET, 0)
    keep = keep[:MAX_DET]
    out, org = np.zeros(MAX_DET, dtype=DET), np.zeros(MAX_DET, dtype=SRC)
    k = len(keep)
    out["x"][:k], out["y"][:k], out["w"][:k], out["h"][:k], out["conf"][:k], out["cls"][:k] = X[keep], Y[keep], Wd[keep], Hd[keep], conf[keep], cls[keep]
    org["tile"][:k], org["det"][:k] = tile_of[keep], det_of[keep]
    return out, k, org, st[()]


def merge(dets, counts, tiles, src_w, src_h, tw, th, **kw):
    """dets [n * T][max_det] + counts [n * T] -> (DET [n][MAX_DET], counts [n], SRC [n][MAX_DET], STATS [n]) as mars_yolo_merge_tiles writes them"""
    dets = np.asarray(dets, dtype=DET)
    T = len(tiles)
    n = dets.shape[0] // T
    cnt = np.clip(np.asarray(counts, dtype=np.int64), 0, dets.shape[1])
    res = [merge_one([dets[c * T + t][:cnt[c * T + t]] for t in range(T)], tiles, src_w, src_h, tw, th, **kw) for c in range(n)]
    return (np.stack([r[0] for r in res]), np.array([r[1] for r in res], dtype=np.int32), np.stack([r[2] for r in res]),
            np.array([r[3] for r in res], dtype=STATS))
