"""Tiled inference on the device (include/mars_hip.h, "Tiled inference"): the front-end and the merge, host forms and through a model, against
tests/tileref.py.  Every comparison is byte equality.  The inputs of the merge cases are built and checked (each case must bite) by
merge_case(), which needs no GPU: tileref alone decides what the device has to give."""
import ctypes as C

import numpy as np
import pytest

import marsfile
import tileref
from conftest import lcg_frame
from test_gpu_yolo_dfl import _conv

pytestmark = pytest.mark.gpu

CW, CH = 96, 64  # camera frames of the front-end and model tests
HAND = [(11, 3, 59, 35), (0, 0, 96, 64)]  # a 48 x 32 tile from an odd column, and the whole frame


def camera_frames(n, seed, nv12=False):
    nb = CW * CH * 3 // 2 if nv12 else CW * CH * 3
    a = np.stack([lcg_frame(seed + i, nb) for i in range(n)])
    return a if nv12 else a.reshape(n, CH, CW, 3)


def want_tiles(frames, nv12_flags, tiles, tw, th, nhwc, keep):
    if nv12_flags is None:
        return tileref.tile_frames(frames, tiles, tw, th, nhwc, keep)
    return tileref.tile_frames_nv12(frames, CW, CH, nv12_flags, tiles, tw, th, nhwc, keep)


# ---- front-end, host form ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("nv12_flags", [None, 0, 3])  # RGB; NV12; NV12 with MARS_NV12_VU | MARS_NV12_FULL_RANGE
def test_front_end_host_form(gpu, nv12_flags):
    frames = camera_frames(2, 0x711E0000, nv12_flags is not None)
    grid = tileref.grid(CW, CH, 32, 32, 8, 8)
    assert len(grid) == 12 and [t[0] for t in grid[:4]] == [0, 24, 48, 64] and sorted({t[1] for t in grid}) == [0, 24, 32]
    fmt = dict(fmt=gpu.CAMERA_RGB) if nv12_flags is None else dict(fmt=gpu.CAMERA_NV12, src_flags=nv12_flags)
    for nhwc in (True, False):
        for tiles, tw, th, keep in ((grid, 32, 32, False), (grid, 64, 64, False), (HAND, 64, 64, False), (HAND, 64, 64, True), (HAND, 40, 24, True)):
            o = gpu.tile_opts(CW, CH, tiles, keep_aspect=keep, **fmt)
            got = gpu.tile_frames(frames, o, tw, th, nhwc)
            want = want_tiles(frames, nv12_flags, tiles, tw, th, nhwc, keep)
            assert got.shape == want.shape == (2 * len(tiles), tw * th * 3)
            assert np.array_equal(got, want), (nv12_flags, nhwc, len(tiles), tw, th, keep, int((got != want).sum()))
    if nv12_flags is None:  # an identity tile is a copy
        got = gpu.tile_frames(frames, gpu.tile_opts(CW, CH, grid), 32, 32, True)
        for c in range(2):
            for t, (x0, y0, x1, y1) in enumerate(grid):
                assert np.array_equal(got[c * 12 + t].reshape(32, 32, 3), (frames[c, y0:y1, x0:x1].astype(np.int16) - 128).astype(np.int8))
    # keep-aspect of the 48 x 32 tile in a 64 x 64 input: bands above and below
    band = want_tiles(frames, nv12_flags, HAND[:1], 64, 64, True, True)[0].reshape(64, 64, 3)
    assert (band[:10] == -17).all() and (band[-10:] == -17).all() and not (band[11:53] == -17).all()


# ---- merge, host form: synthetic lists from an LCG ------------------------------------------------------------------------------------------
class Lcg:
    """uniform numbers from the suite's LCG bytes"""

    def __init__(self, seed, n=1 << 16):
        b = lcg_frame(seed, 2 * n).astype(np.uint32)
        self.v, self.i = (b[0::2] << 8 | b[1::2]).astype(np.float64) / 65536.0, 0

    def u(self, lo=0.0, hi=1.0):
        self.i += 1
        return lo + (hi - lo) * float(self.v[(self.i - 1) % len(self.v)])

    def k(self, n):
        return min(int(self.u() * n), n - 1)


TABLES = {
    1: (96, 64, [(0, 0, 96, 64)]),
    2: (96, 64, [(0, 0, 64, 64), (32, 0, 96, 64)]),
    6: (96, 64, tileref.grid(96, 64, 48, 32, 24, 0)),            # 3 x 2: interior and border sides
    16: (256, 256, tileref.grid(256, 256, 80, 80, 21, 21)),      # 4 x 4 overlapping tiles of 80 x 80
    "16d": (256, 256, tileref.grid(256, 256, 64, 64, 0, 0)),     # 4 x 4 disjoint tiles
}
TW = TH = 64


def synth_lists(seed, W, H, tiles, counts, max_det, n_obj, ncls=3, levels=0, keep=False, size=(6.0, 28.0)):
    """one camera frame: n_obj objects in camera pixels, presented by every tile that holds their centre (a jittered copy in that tile's input
    pixels), lists filled up with loose boxes to counts[t] and ordered by confidence.  levels > 0: confidences are multiples of 1 / levels
    (ties across tiles).  -> DET [T][max_det], counts [T]"""
    g = Lcg(seed)
    objs = [(g.u(0, W), g.u(0, H), g.u(*size), g.u(*size), g.k(ncls)) for _ in range(n_obj)]
    dets = np.zeros((len(tiles), max_det), dtype=tileref.DET)
    for t, (x0, y0, x1, y1) in enumerate(tiles):
        nw, nh, px, py = tileref.roi_target_np(x1 - x0, y1 - y0, TW, TH, keep)
        rx, ry = (x1 - x0) / nw, (y1 - y0) / nh
        rows = []
        for X, Y, Wd, Hd, cls in objs:
            if x0 <= X < x1 and y0 <= Y < y1:
                rows.append(((X - x0) / rx + px + g.u(-0.4, 0.4), (Y - y0) / ry + py + g.u(-0.4, 0.4), Wd / rx * g.u(0.95, 1.05), Hd / ry * g.u(0.95, 1.05), cls))
        while len(rows) < counts[t]:
            rows.append((g.u(0, TW), g.u(0, TH), g.u(2, 10), g.u(2, 10), g.k(ncls)))
        rows = rows[:counts[t]]
        conf = [(1 + g.k(levels - 1)) / levels if levels else g.u(0.3, 0.95) for _ in rows]
        for i, j in enumerate(sorted(range(len(rows)), key=lambda j: -conf[j])):
            dets[t, i] = rows[j] [:4] + (conf[j], rows[j][4])
    return dets, np.array(counts, dtype=np.int32)


def disjoint_lists(T, per_tile, max_det):
    """per_tile boxes of 2 x 2 on a 16-column raster of every 64 x 64 tile, confidences all different"""
    dets = np.zeros((T, max_det), dtype=tileref.DET)
    for t in range(T):
        for i in range(per_tile):
            dets[t, i] = (4 * (i % 16) + 2, 8 * (i // 16) + 4, 2, 2, 0.9 - (i * T + t) * 1e-4, i % 3)
    return dets, np.full(T, per_tile, dtype=np.int32)


MERGE_CASES = ["t1", "t2", "t6_counts", "t6_edge0", "t6_edge4", "t6_ios", "t6_iou", "t6_agnostic", "t6_classes", "t6_thresh03", "t6_thresh07",
               "t6_invalid", "t6_keep_aspect", "t16_quota", "t16_full", "t16_ties", "t16_disjoint", "t2_three_frames", "t2_n64", "t2_n65", "t16_n1025"]


def merge_case(name):
    """-> (W, H, tiles, dets [n * T][max_det], counts, options of tileref.merge / gpu.tile_opts, expectation).  Asserts that the case bites."""
    kw, n_frames, bite = {}, 1, True
    if name == "t1":
        W, H, tiles = TABLES[1]
        dets, counts = synth_lists(0x7100, W, H, tiles, [70], 80, 40)
        bite = False
    elif name == "t2" or name == "t2_three_frames":
        W, H, tiles = TABLES[2]
        n_frames = 3 if name.endswith("frames") else 1
        parts = [synth_lists(0x7200 + c, W, H, tiles, [60 + c, 50], 64, 45) for c in range(n_frames)]
        dets, counts = np.concatenate([p[0] for p in parts]), np.concatenate([p[1] for p in parts])
    elif name in ("t2_n64", "t2_n65"):  # candidate counts at the edge of the 64-row chunks of the suppression walk
        W, H, tiles = TABLES[2]
        dets, counts = synth_lists(0x7264, W, H, tiles, [32, int(name[4:]) - 32], 64, 45)
    elif name.startswith("t6"):
        W, H, tiles = TABLES[6]
        cnt = [0, 1, 63, 64, 65, 40] if name == "t6_counts" else [50, 64, 33, 65, 20, 47]
        keep = name == "t6_keep_aspect"
        small = dict(n_obj=150, size=(4.0, 10.0)) if name == "t6_edge4" else dict(n_obj=60)  # boxes that fit between two interior sides
        dets, counts = synth_lists(0x7600, W, H, tiles, cnt, 65, keep=keep, ncls=2 if name in ("t6_agnostic", "t6_classes") else 3, **small)
        kw = {"t6_edge4": dict(edge_margin=4.0), "t6_ios": dict(flags=tileref.MATCH_IOS, merge_thresh=0.6), "t6_iou": dict(merge_thresh=0.6),
              "t6_agnostic": dict(flags=tileref.AGNOSTIC), "t6_thresh03": dict(merge_thresh=0.3), "t6_thresh07": dict(merge_thresh=0.7),
              "t6_keep_aspect": dict(flags=tileref.KEEP_ASPECT)}.get(name, {})
        if name == "t6_invalid":
            dets[1, 3]["x"], dets[2, 0]["w"], dets[2, 5]["w"], dets[3, 7]["h"], dets[5, 2]["conf"] = np.nan, np.inf, 0, -1, np.nan
            dets[1, 9]["y"], dets[3, 8]["h"] = -np.inf, np.nan
        if name in ("t6_agnostic", "t6_classes"):  # one object at camera (36, 16), seen by two tiles under two classes
            dets[0, 0], dets[1, 0] = (48, 32, 12, 16, 0.99, 0), (16, 32, 12, 16, 0.97, 1)
        if name in ("t6_ios", "t6_iou"):  # pieces of boxes cut by a tile edge: inside the full box another tile sees
            dets[0, 0], dets[1, 0] = (30, 20, 40, 12, 0.99, 0), ((24 - 24) / 0.75 + 5, 20, 10, 12, 0.97, 0)
            dets[3, 0], dets[4, 0] = (40, 30, 30, 30, 0.98, 1), (8, 30, 14, 28, 0.96, 1)
    else:
        W, H, tiles = TABLES["16d" if name == "t16_disjoint" else 16]
        if name == "t16_quota":
            cnt = [100] * 16
            cnt[5] = 200
            dets, counts = synth_lists(0x7160, W, H, tiles, cnt, 200, 400)
        elif name == "t16_full":
            dets, counts = synth_lists(0x7161, W, H, tiles, [128] * 16, 128, 700, size=(5.0, 16.0))
        elif name == "t16_ties":
            dets, counts = synth_lists(0x7162, W, H, tiles, [60] * 16, 64, 300, levels=8)
        elif name == "t16_n1025":  # one candidate behind 1024: a last chunk of one row, and the removed set's upper 16 words in use
            dets, counts = synth_lists(0x7163, W, H, tiles, [64] * 15 + [65], 65, 300)
        else:
            dets, counts = disjoint_lists(16, 128, 128)
            bite = False
    want = tileref.merge(dets, counts, tiles, W, H, TW, TH, **kw)
    out, oc, org, st = want
    T = len(tiles)
    for c in range(n_frames):
        s = st[c]
        if bite:
            assert 0 < oc[c] < s["candidates"] and s["suppressed"] > 0, (name, c, tuple(s))
        assert s["candidates"] == s["suppressed"] + s["truncated"] + oc[c]
    if name == "t1":
        cand = dets[0, :counts[0]]
        order = np.lexsort((np.arange(len(cand)), -tileref.ord_key(cand["conf"]).astype(np.int64)))
        assert st[0]["suppressed"] == 0 and oc[0] == 70 and (org[0, :70]["det"] == order).all() and (out[0, :70]["conf"] == cand["conf"][order]).all()
    if name == "t6_counts":
        assert st[0]["candidates"] == sum([0, 1, 63, 64, 65, 40])
    if name in ("t2_n64", "t2_n65", "t16_n1025"):
        assert st[0]["candidates"] == int(name.split("_n")[1])
    if name == "t6_edge0":
        assert st[0]["edge"] == 0
    if name == "t6_edge4":
        assert 0 < st[0]["edge"] < st[0]["candidates"]
    if name == "t6_invalid":
        assert st[0]["invalid"] == 7
    if name in ("t6_ios", "t6_iou"):
        other = tileref.merge(dets, counts, tiles, W, H, TW, TH, flags=0 if name == "t6_ios" else tileref.MATCH_IOS, merge_thresh=0.6)
        assert (oc[0] < other[1][0]) == (name == "t6_ios"), "IOS removes what IoU leaves at the same threshold"
    if name in ("t6_agnostic", "t6_classes"):
        other = tileref.merge(dets, counts, tiles, W, H, TW, TH, flags=0 if name == "t6_agnostic" else tileref.AGNOSTIC)
        assert (oc[0] < other[1][0]) == (name == "t6_agnostic")
    if name == "t6_thresh03":
        assert oc[0] < tileref.merge(dets, counts, tiles, W, H, TW, TH, merge_thresh=0.7)[1][0]
    if name == "t16_quota":
        assert tileref.quota(16) == 128 and st[0]["overflow"] == 72 and st[0]["candidates"] == 15 * 100 + 128
    if name == "t16_full":
        assert st[0]["candidates"] == 2048 and st[0]["overflow"] == 0
    if name == "t16_ties":
        k = oc[0]
        tie = out[0, :k - 1]["conf"] == out[0, 1:k]["conf"]
        assert (tie & (org[0, :k - 1]["tile"] != org[0, 1:k]["tile"])).sum() > 10, "no ties across tiles among the survivors"
    if name == "t16_disjoint":
        assert st[0]["candidates"] == 2048 and st[0]["suppressed"] == 0 and st[0]["truncated"] == 1048 and oc[0] == 1000
    return W, H, tiles, dets, counts, kw, want


def opts_of(gpu, W, H, tiles, kw, **more):
    f = kw.get("flags", 0)
    return gpu.tile_opts(W, H, tiles, keep_aspect=bool(f & tileref.KEEP_ASPECT), ios=bool(f & tileref.MATCH_IOS), agnostic=bool(f & tileref.AGNOSTIC),
                         merge_thresh=kw.get("merge_thresh", 0.0), edge_margin=kw.get("edge_margin", 0.0), max_per_tile=kw.get("max_per_tile", 0), **more)


def same_merge(got, want, what):
    for g, w, n in zip(got, want, ("dets", "counts", "origins", "stats")):
        assert g.shape == w.shape and g.tobytes() == w.tobytes(), (what, n, got[1], want[1], got[3], want[3])


@pytest.mark.parametrize("name", MERGE_CASES)
def test_merge_host_form(gpu, name):
    W, H, tiles, dets, counts, kw, want = merge_case(name)
    same_merge(gpu.merge_tiles(dets, counts, opts_of(gpu, W, H, tiles, kw), TW, TH), want, name)


def test_merge_host_form_clamps_counts_and_takes_max_per_tile(gpu):
    W, H, tiles, dets, counts, kw, _ = merge_case("t6_counts")
    wild = counts.copy()
    wild[0], wild[2] = -5, 9999  # clamped to 0 .. max_det
    kw = dict(max_per_tile=48)
    want = tileref.merge(dets, wild, tiles, W, H, TW, TH, **kw)
    assert want[3][0]["overflow"] == (65 - 48) * 2 + (64 - 48) > 0
    same_merge(gpu.merge_tiles(dets, wild, opts_of(gpu, W, H, tiles, kw), TW, TH), want, "clamped")


# ---- through a model ------------------------------------------------------------------------------------------------------------------------
R, NC, S = 4, 3, 64
DFL_KW = dict(conf=0.6, box_scales=0.05, cls_scales=0.02)


def tile_graph(nchw):
    """3 x 64 x 64 camera input -> a 3x3 stride-2 convolution to 16 channels -> 1x1 stride-2 convolutions down to 4 x 4; DFL heads (box 4 R,
    class NC, concat) at strides 8 and 16; the concats are the outputs.  -> file, input tensor, [(box, class, stride)]"""
    rng = np.random.default_rng(0x711E + nchw)
    G = marsfile.Graph()
    fmt = marsfile.NCHW if nchw else marsfile.NHWC
    shp = (lambda c, h, w: [1, c, h, w]) if nchw else (lambda c, h, w: [1, h, w, c])
    x = G.tensor(shp(3, S, S), fmt=fmt, scale=1.0 / 128)
    t = G.tensor(shp(16, S // 2, S // 2), fmt=fmt, scale=0.05)
    _conv(G, rng, x, t, 16, 3, 3, 2, nchw)
    feat, sc = {}, 0.15
    for s in (4, 8, 16):
        n = G.tensor(shp(16, S // s, S // s), fmt=fmt, scale=sc)
        _conv(G, rng, t, n, 16, 16, 1, 2, nchw)
        feat[s], t, sc = (n, sc), n, sc * 3
    heads, outs = [], []
    for s in (8, 16):
        g, (p, ps) = S // s, feat[s]
        b = G.tensor(shp(4 * R, g, g), fmt=fmt, scale=ps * 3)
        c = G.tensor(shp(NC, g, g), fmt=fmt, scale=ps * 3)
        _conv(G, rng, p, b, 4 * R, 16, 1, 1, nchw)
        _conv(G, rng, p, c, NC, 16, 1, 1, nchw)
        cat = G.tensor(shp(4 * R + NC, g, g), fmt=fmt, scale=ps * 3)
        G.concat([b, c], cat, axis=1 if nchw else 3)
        heads.append((b, c, s))
        outs.append(cat)
    return G.serialise([x], outs), x, heads


def lists_to_arrays(lists):
    dets = np.zeros((len(lists), tileref.MAX_DET), dtype=tileref.DET)
    for f, l in enumerate(lists):
        dets[f, :len(l)] = l
    return dets, np.array([len(l) for l in lists], dtype=np.int32)


def raw_detect_results(gpu, m):
    """mars_hip_detect_results as it is: the whole [batch][MAX_DET] block and the counts, nothing cut"""
    dets = np.zeros((m.batch, tileref.MAX_DET), dtype=tileref.DET)
    counts = np.zeros(m.batch, dtype=np.int32)
    assert gpu.lib().mars_hip_detect_results(m.p, dets.ctypes.data, counts.ctypes.data_as(C.POINTER(C.c_int))) == gpu.MARS_OK
    return dets, counts


MODEL_SHAPES = {6: tileref.grid(CW, CH, 48, 32, 24, 0), 4: [(0, 0, 64, 64), (32, 0, 96, 64)]}  # 1 camera frame x 6 tiles; 2 x 2


@pytest.mark.parametrize("batch", [6, 4])
@pytest.mark.parametrize("nchw", [False, True])
def test_chain_through_a_model(gpu, nchw, batch):
    """preprocess_tiles -> run -> detect_dfl_device (graph-input pixels) -> merge_tiles, twice.  The first round fetches the per-tile lists
    (the whole block and the counts) between the tail and the merge and again after it: the merge leaves them alone, byte for byte.  The second
    round takes its frames from HBM and nothing waits between the calls"""
    tiles = MODEL_SHAPES[batch]
    T, cams = len(tiles), batch // len(tiles)
    nv12 = batch == 4  # the 2 x 2 shape takes NV12 frames
    d, tin, heads = tile_graph(nchw)
    m = gpu.Model(d, batch=batch)
    fmt = dict(fmt=gpu.CAMERA_NV12, src_flags=gpu.NV12_VU) if nv12 else {}
    o = gpu.tile_opts(CW, CH, tiles, merge_thresh=0.4, ios=nchw, edge_margin=2.0 if batch == 6 else 0.0, **fmt)
    kw = dict(flags=tileref.MATCH_IOS if nchw else 0, merge_thresh=0.4, edge_margin=2.0 if batch == 6 else 0.0)
    dfl = dict(heads=[(b, c, s) for b, c, s in heads], reg_max=R, **DFL_KW)
    wants, bufs = [], []
    for rnd in range(2):
        frames = camera_frames(cams, 0x711E1000 + 64 * rnd + batch, nv12)
        if rnd == 0:
            m.preprocess_tiles(frames, o)
        else:
            bufs.append(gpu.DeviceBuffer(frames))
            m.preprocess_tiles(bufs[-1].ptr, o, device=True)
        m.run_device(sync=False)
        m.detect_dfl_device(**dfl)
        before = raw_detect_results(gpu, m) if rnd == 0 else None
        m.merge_tiles(o)
        got = m.tile_results()
        if before is not None:
            after = raw_detect_results(gpu, m)
            assert after[1].tobytes() == before[1].tobytes() and after[0].tobytes() == before[0].tobytes(), "the merge changed the per-tile lists"
        host = gpu.tile_frames(frames, o, S, S, not nchw)
        assert np.array_equal(host, want_tiles(frames, gpu.NV12_VU if nv12 else None, tiles, S, S, not nchw, False))
        for f in range(batch):
            assert np.array_equal(m.read_tensor(tin, frame=f)[:host[f].size].view(np.int8), host[f]), (rnd, f)
        lists = m.detect_results()
        if before is not None:
            assert all(l.tobytes() == before[0][f, :before[1][f]].tobytes() for f, l in enumerate(lists))
        assert sum(len(l) > 0 for l in lists) >= 2 * cams, "the threshold leaves candidates in too few tiles"
        want = tileref.merge(*lists_to_arrays(lists), tiles, CW, CH, S, S, **kw)
        same_merge(got, want, (nchw, batch, rnd))
        assert all(a.tobytes() == b.tobytes() for a, b in zip(m.detect_results(), lists)), "detect_results changed after the merge"
        assert m.tile_ms() >= 0 and gpu.lib().mars_hip_tile_frames(m.p) == cams
        wants.append(want)
    assert wants[0][0].tobytes() != wants[1][0].tobytes(), "both rounds expect the same lists: nothing shows that no stale list is read"
    m.close()
    for b in bufs:
        b.free()


def test_merged_block_follows_the_batch(gpu):
    """one model at batch 2 -> 4 -> 2 over the two-tile table (1, 2, 1 camera frames; mars_hip_set_batch between the calls): the merged
    arrays are there for every batch, every merge is the restatement's, the merge's device time is there after each, and nothing can be
    fetched before the first"""
    tiles = MODEL_SHAPES[4]
    d, tin, heads = tile_graph(False)
    m = gpu.Model(d, batch=2)
    with pytest.raises(gpu.MarsError) as e:
        m.tile_results()
    assert e.value.code == gpu.MARS_ERR_INVALID_TENSOR and m.tile_ms() < 0
    o = gpu.tile_opts(CW, CH, tiles, merge_thresh=0.4)
    dfl = dict(heads=[(b, c, s) for b, c, s in heads], reg_max=R, **DFL_KW)
    for rnd, batch in enumerate((2, 4, 2)):
        m.set_batch(batch)
        cams = batch // len(tiles)
        m.preprocess_tiles(camera_frames(cams, 0x711E3000 + 64 * rnd), o)
        m.run_device(sync=False)
        m.detect_dfl_device(**dfl)
        m.merge_tiles(o)
        got = m.tile_results()
        lists = m.detect_results()
        assert sum(len(l) > 0 for l in lists) >= cams, "the threshold leaves candidates in too few tiles"
        same_merge(got, tileref.merge(*lists_to_arrays(lists), tiles, CW, CH, S, S, merge_thresh=0.4), ("growth", batch))
        assert m.tile_ms() >= 0 and gpu.lib().mars_hip_tile_frames(m.p) == cams
    m.close()


def test_refusals_through_the_model(gpu):
    FILE, TENSOR = gpu.MARS_ERR_INVALID_FILE, gpu.MARS_ERR_INVALID_TENSOR
    d, tin, heads = tile_graph(True)
    m = gpu.Model(d, batch=4)
    two = MODEL_SHAPES[4]
    good = gpu.tile_opts(CW, CH, two)
    frames = camera_frames(2, 0x711E2000)
    dfl = dict(heads=[(b, c, s) for b, c, s in heads], reg_max=R, **DFL_KW)

    def code(f, *a, **k):
        with pytest.raises(gpu.MarsError) as e:
            f(*a, **k)
        return e.value.code

    assert code(m.merge_tiles, good) == TENSOR      # a merge before any detect
    assert code(m.tile_results) == TENSOR and gpu.lib().mars_hip_tile_frames(m.p) == 0  # results before any merge
    three = gpu.tile_opts(CW, CH, two + [(0, 0, 96, 64)])
    assert code(m.preprocess_tiles, np.zeros(CW * CH * 3, dtype=np.uint8), three) == TENSOR  # batch % T != 0
    m.preprocess_tiles(frames, good)
    m.run_device()
    m.detect_dfl_device(src=(CW, CH), **dfl)
    assert code(m.merge_tiles, good) == TENSOR      # lists mapped with src_w > 0
    m.detect_dfl_device(**dfl)
    assert code(m.merge_tiles, three) == TENSOR     # batch % T != 0
    assert code(m.tile_results) == TENSOR
    assert code(m.merge_tiles, gpu.tile_opts(CW, CH, two, flags=8)) == FILE                 # an unknown flag
    assert code(m.merge_tiles, gpu.tile_opts(CW, CH, [(0, 0, 64, 64), (40, 0, 104, 64)])) == FILE  # a tile sticking out of the frame
    assert code(m.preprocess_tiles, frames, gpu.tile_opts(CW, CH, [(0, 0, 64, 64), (32, 8, 96, 72)])) == FILE
    lists = m.detect_results()
    m.merge_tiles(good)
    same_merge(m.tile_results(), tileref.merge(*lists_to_arrays(lists), two, CW, CH, S, S), "after the refusals")
    assert all(a.tobytes() == b.tobytes() for a, b in zip(m.detect_results(), lists)), "detect_results changed after the merge"
    m.pipe_open(download_outputs=False, detect=True, dfl_heads=gpu.yolo_dfl_heads(**dfl))
    assert code(m.merge_tiles, good) == TENSOR      # an open pipe
    assert code(m.preprocess_tiles, frames, good) == TENSOR
    m.pipe_close()
    m.close()
