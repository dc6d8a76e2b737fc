"""Tiled inference (include/mars_hip.h, "Tiled inference"), the part that needs no GPU: the grid rule (pure host code) against its numpy
restatement, the record sizes, the refusals that come before any device work, and the restatement tests/test_gpu_tile.py compares the device
against, checked on cases worked out by hand."""
import ctypes as C

import numpy as np

import tileref
from test_roi_cpu import box

F = np.float32
NEW = ["mars_tile_grid", "mars_hip_preprocess_tiles_device", "mars_hip_preprocess_tiles", "mars_hip_merge_tiles_device", "mars_hip_tile_results",
       "mars_hip_tile_frames", "mars_hip_merge_tiles", "mars_hip_tile_ms", "mars_yolo_tile_frames", "mars_yolo_merge_tiles"]

GRIDS = [(1920, 1080, 640, 640, 128, 128),   # the header's example
         (96, 64, 32, 32, 8, 8),             # the GPU tests' grid
         (96, 64, 200, 100, 0, 0),           # a tile larger than the frame
         (96, 64, 200, 32, 5, 0),            # ... on one axis
         (96, 64, 32, 32, 0, 0),             # overlap 0, W - tile an exact multiple of the step
         (100, 70, 30, 20, 10, 5),           # (100 - 30) = 70 = 3.5 steps; (70 - 20) = 50: not a multiple of 15
         (90, 64, 30, 32, 10, 31),           # W - tile = 60 = 3 * 20 exactly; step 1 on y
         (3840, 2160, 640, 640, 64, 64),
         (33, 1, 32, 1, 31, 0), (2, 2, 1, 1, 0, 0)]


def lib_grid(marsrt, *a, cap=None):
    n = marsrt.lib().mars_tile_grid(*a, None, 0)
    if n < 0:
        return n, None
    cap = n if cap is None else cap
    t = np.full(max(cap, 1) + 1, -7, dtype=np.int32).repeat(4).view(marsrt.TILE_DTYPE)
    assert marsrt.lib().mars_tile_grid(*a, t.ctypes.data, cap) == n
    assert (t[min(cap, n):].view(np.int32) == -7).all()  # nothing behind the cap is written
    return n, [tuple(int(v) for v in r) for r in t[:min(cap, n)]]


def test_tile_symbols_are_exported(marsrt):
    L = marsrt.lib()
    for n in NEW:
        assert n in marsrt.EXPORTS["mars_hip.h"], n
        assert hasattr(L, n), n
    assert (marsrt.TILE_KEEP_ASPECT, marsrt.TILE_MATCH_IOS, marsrt.TILE_AGNOSTIC) == (1, 2, 4)
    assert (marsrt.TILE_MAX_TILES, marsrt.TILE_MAX_CAND) == (tileref.MAX_TILES, tileref.MAX_CAND) == (64, 2048)
    for f in ("tile_grid", "tile_opts", "tile_frames", "merge_tiles"):
        assert callable(getattr(marsrt, f)), f
    for f in ("preprocess_tiles", "merge_tiles", "tile_results"):
        assert callable(getattr(marsrt.Model, f)), f


def test_tile_record_sizes(marsrt, tmp_path):
    import os
    import subprocess
    assert marsrt.TILE_DTYPE == np.dtype([(n, "<i4") for n in ("x0", "y0", "x1", "y1")])
    assert marsrt.TILE_SRC_DTYPE == tileref.SRC and marsrt.TILE_STATS_DTYPE == tileref.STATS and marsrt.DET_DTYPE == tileref.DET
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    src = tmp_path / "tile_abi.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "mars_hip.h"\n'
                   'int main(void){ printf("%zu %zu %zu %zu %zu %zu %zu %zu %u %u %u %d %d", sizeof(mars_tile_t), sizeof(mars_tile_src_t),\n'
                   ' sizeof(mars_tile_stats_t), sizeof(mars_hip_tile_opts_t), offsetof(mars_hip_tile_opts_t, tiles), offsetof(mars_hip_tile_opts_t, flags),\n'
                   ' offsetof(mars_hip_tile_opts_t, max_per_tile), offsetof(mars_tile_stats_t, truncated), MARS_TILE_KEEP_ASPECT, MARS_TILE_MATCH_IOS,\n'
                   ' MARS_TILE_AGNOSTIC, MARS_TILE_MAX_TILES, MARS_TILE_MAX_CAND); return 0; }\n')
    exe = tmp_path / "tile_abi"
    subprocess.run(["gcc", "-I", os.path.join(root, "include"), str(src), "-o", str(exe)], check=True)
    got = subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.split()
    O = marsrt.TileOpts
    assert got == ["16", "8", "24", str(C.sizeof(O)), str(O.tiles.offset), str(O.flags.offset), str(O.max_per_tile.offset), "20", "1", "2", "4", "64", "2048"]


def test_tile_grid_header_example(marsrt):
    n, t = lib_grid(marsrt, 1920, 1080, 640, 640, 128, 128)
    assert n == 8
    assert [r[0] for r in t[:4]] == [0, 512, 1024, 1280] and sorted({r[1] for r in t}) == [0, 440]
    assert tileref.axis(1920, 640, 128) == [0, 512, 1024, 1280] and tileref.axis(1080, 640, 128) == [0, 440]
    assert tileref.axis(96, 32, 8) == [0, 24, 48, 64] and tileref.axis(64, 32, 8) == [0, 24, 32]
    assert tileref.axis(96, 32, 0) == [0, 32, 64] and tileref.axis(90, 30, 10) == [0, 20, 40, 60] and tileref.axis(32, 32, 0) == [0]
    assert [tuple(r) for r in marsrt.tile_grid(96, 64, 32, 32, 8, 8)] == tileref.grid(96, 64, 32, 32, 8, 8)


def test_tile_grid_matches_the_restatement(marsrt):
    for g in GRIDS:
        want = tileref.grid(*g)
        n, t = lib_grid(marsrt, *g)
        assert n == len(want) and t == want, g
        W, H = g[0], g[1]
        # one size, row-major (y outer, x inner), and the frame is covered
        assert len({(r[2] - r[0], r[3] - r[1]) for r in t}) == 1, g
        assert t == sorted(t, key=lambda r: (r[1], r[0])), g
        cover = np.zeros((H, W), dtype=bool)
        for x0, y0, x1, y1 in t:
            assert 0 <= x0 < x1 <= W and 0 <= y0 < y1 <= H
            cover[y0:y1, x0:x1] = True
        assert cover.all(), g


def test_tile_grid_cap_and_refusals(marsrt):
    n, t = lib_grid(marsrt, 96, 64, 32, 32, 8, 8, cap=5)
    assert n == 12 and t == tileref.grid(96, 64, 32, 32, 8, 8)[:5]
    assert lib_grid(marsrt, 96, 64, 32, 32, 8, 8, cap=0)[0] == 12
    for g in [(0, 64, 32, 32, 0, 0), (96, -1, 32, 32, 0, 0), (96, 64, 0, 32, 0, 0), (96, 64, 32, -3, 0, 0), (96, 64, 32, 32, -1, 0),
              (96, 64, 32, 32, 0, -1), (96, 64, 32, 32, 32, 0), (96, 64, 32, 32, 0, 40)]:
        assert lib_grid(marsrt, *g)[0] == -1 and tileref.grid(*g) == -1, g
    try:
        marsrt.tile_grid(96, 64, 32, 32, 32, 0)
        assert False
    except ValueError:
        pass


def test_tile_bad_arguments_are_refused_up_front(marsrt):
    L = marsrt.lib()
    BAD_FILE = marsrt.MARS_ERR_INVALID_FILE
    W, H = 12, 8
    table = [(0, 0, 8, 8), (4, 0, 12, 8)]
    frames = np.zeros(W * H * 3 + 64, dtype=np.uint8)
    out = np.full(2 * 8 * 8 * 3, 77, dtype=np.int8)
    dets = np.zeros((2, 4), dtype=marsrt.DET_DTYPE)
    counts = np.zeros(2, dtype=np.int32)
    mo, mc = np.full(1000, 77, dtype=marsrt.DET_DTYPE), np.full(1, 77, dtype=np.int32)

    def front(o, n=1, tw=8, th=8, fr=frames, dst=out):
        return L.mars_yolo_tile_frames(None if fr is None else fr.ctypes.data, n, None if o is None else C.byref(o), tw, th, 1,
                                       None if dst is None else dst.ctypes.data)

    def merge(o, n=1, max_det=4, tw=8, th=8, d=dets, c=counts, dst=mo):
        return L.mars_yolo_merge_tiles(None if d is None else d.ctypes.data, None if c is None else c.ctypes.data, n, max_det,
                                       None if o is None else C.byref(o), tw, th, None if dst is None else dst.ctypes.data, mc.ctypes.data, None, None)

    mk = marsrt.tile_opts
    good = mk(W, H, table)
    bad = [mk(0, H, table), mk(W, -8, table),                                               # non-positive frame sizes
           mk(W, H, table, fmt=2), mk(W, H, table, fmt=-1),                                 # an unknown format
           mk(W, H, table, src_flags=1),                                                    # an NV12 flag on RGB frames
           mk(W, H, table, fmt=marsrt.CAMERA_NV12, src_flags=4),                            # an unknown NV12 flag bit
           mk(11, 8, [(0, 0, 8, 8)], fmt=marsrt.CAMERA_NV12), mk(12, 7, [(0, 0, 8, 7)], fmt=marsrt.CAMERA_NV12),  # odd NV12 sizes
           mk(W, H, table, flags=8),                                                        # an unknown flag bit
           mk(W, H, table, merge_thresh=-0.1), mk(W, H, table, merge_thresh=1.5), mk(W, H, table, merge_thresh=float("nan")),
           mk(W, H, table, edge_margin=-1.0), mk(W, H, table, edge_margin=float("inf")),
           mk(W, H, table, max_per_tile=-1), mk(W, H, table, max_per_tile=1025),            # 2 * 1025 > 2048
           mk(W, H, [(0, 0, 8, 8), (4, 0, 13, 8)]), mk(W, H, [(0, 0, 8, 9)]), mk(W, H, [(-1, 0, 8, 8)]), mk(W, H, [(0, -2, 8, 8)]),  # sticking out
           mk(W, H, [(4, 0, 4, 8)]), mk(W, H, [(0, 5, 8, 3)]),                              # empty
           mk(W, H, [(0, 0, 8, 8)] * 65)]                                                   # too many tiles
    o = mk(W, H, table)
    o.n_tiles = 0
    bad.append(o)
    o = mk(W, H, table)
    o.tiles = None                                                                          # a NULL table
    bad.append(o)
    assert mk(W, H, [(0, 0, 8, 8)] * 64).n_tiles == 64 and mk(W, H, table, max_per_tile=1024).max_per_tile == 1024
    P = C.POINTER(marsrt.MarsModel)
    a = marsrt.MarsModel()  # never looked into: the refusals come first
    for i, o in enumerate(bad):
        assert front(o) == BAD_FILE, i
        assert merge(o) == BAD_FILE, i
        for f in (L.mars_hip_preprocess_tiles_device, L.mars_hip_preprocess_tiles):
            assert f(C.pointer(a), 0, frames.ctypes.data, C.byref(o)) == BAD_FILE, i
        assert L.mars_hip_merge_tiles_device(C.pointer(a), C.byref(o)) == BAD_FILE, i
        assert L.mars_hip_merge_tiles(C.pointer(a), C.byref(o), None, None, None, None) == BAD_FILE, i
    assert front(None) == BAD_FILE and merge(None) == BAD_FILE
    for kw in (dict(tw=0), dict(th=-8), dict(n=0), dict(fr=None), dict(dst=None)):
        assert front(good, **kw) == BAD_FILE, kw
    for kw in (dict(tw=0), dict(th=-8), dict(n=0), dict(max_det=0), dict(max_det=1001), dict(d=None), dict(c=None), dict(dst=None)):
        assert merge(good, **kw) == BAD_FILE, kw
    assert (out == 77).all() and mo.tobytes() == np.full(1000, 77, dtype=marsrt.DET_DTYPE).tobytes() and mc[0] == 77  # nothing was written
    for f in (L.mars_hip_preprocess_tiles_device, L.mars_hip_preprocess_tiles):
        assert f(P(), 0, frames.ctypes.data, C.byref(good)) == BAD_FILE                     # no model
        assert f(C.pointer(a), 0, None, C.byref(good)) == BAD_FILE                          # no frames
        assert f(C.pointer(a), 0, frames.ctypes.data, None) == BAD_FILE                     # no options
    assert L.mars_hip_merge_tiles_device(P(), C.byref(good)) == BAD_FILE and L.mars_hip_merge_tiles_device(C.pointer(a), None) == BAD_FILE
    assert L.mars_hip_tile_results(P(), None, None, None, None) == BAD_FILE
    assert L.mars_hip_tile_ms(P()) < 0 and L.mars_hip_tile_frames(P()) == 0


# ---- the restatement itself -----------------------------------------------------------------------------------------------------------
def _image(h, w, seed):
    return np.random.default_rng(seed).integers(0, 256, size=(h, w, 3), dtype=np.uint8)


def _lists(*per_tile):
    return [np.array(t, dtype=tileref.DET) if len(t) else np.zeros(0, dtype=tileref.DET) for t in per_tile]


def test_restated_identity_tile_is_a_copy():
    img = _image(64, 96, 3)
    tiles = tileref.grid(96, 64, 32, 32, 8, 8)
    got = tileref.tile_frames([img], tiles, 32, 32)
    planar = tileref.tile_frames([img], tiles, 32, 32, nhwc=False)
    assert got.shape == (12, 32 * 32 * 3)
    for t, (x0, y0, x1, y1) in enumerate(tiles):
        want = (img[y0:y1, x0:x1].astype(np.int16) - 128).astype(np.int8)
        assert np.array_equal(got[t].reshape(32, 32, 3), want)
        assert np.array_equal(planar[t].reshape(3, 32, 32), want.transpose(2, 0, 1))


def test_restated_duplicate_in_the_overlap_comes_out_once():
    # 64 x 32 frame, two 40 x 32 tiles overlapping in x = 24 .. 40, input 40 x 32 (identity map).  One object at camera (32, 16), 10 x 10
    tiles = [(0, 0, 40, 32), (24, 0, 64, 32)]
    lists = _lists([box(32, 16, 10, 10, 0.6, 3)], [box(32 - 24, 16, 10, 10, 0.8, 3)])
    out, n, org, st = tileref.merge_one(lists, tiles, 64, 32, 40, 32)
    assert n == 1 and tuple(out[0]) == (32.0, 16.0, 10.0, 10.0, F(0.8), 3) and tuple(org[0]) == (1, 0)
    assert tuple(st) == (2, 0, 0, 0, 1, 0)
    assert out[1:].tobytes() == bytes(999 * 24) and org[1:].tobytes() == bytes(999 * 8)
    # another class: both stay, unless the merge is class-agnostic
    lists[1]["cls"] = 4
    assert tileref.merge_one(lists, tiles, 64, 32, 40, 32)[1] == 2
    assert tileref.merge_one(lists, tiles, 64, 32, 40, 32, flags=tileref.AGNOSTIC)[1] == 1


def test_restated_boxes_of_one_tile_never_remove_each_other():
    tiles = [(0, 0, 40, 32), (24, 0, 64, 32)]
    lists = _lists([box(20, 16, 10, 10, 0.9, 1), box(21, 16, 10, 10, 0.8, 1)], [])
    out, n, org, st = tileref.merge_one(lists, tiles, 64, 32, 40, 32)
    assert n == 2 and [tuple(o) for o in org[:2]] == [(0, 0), (0, 1)] and st["suppressed"] == 0
    # equal confidences: k decides, tile 0 first
    lists = _lists([box(10, 10, 4, 4, 0.5, 1)], [box(30, 20, 4, 4, 0.5, 1), box(20, 20, 4, 4, 0.75, 1)])
    out, n, org, st = tileref.merge_one(lists, tiles, 64, 32, 40, 32)
    assert [tuple(o) for o in org[:3]] == [(1, 1), (0, 0), (1, 0)]


def test_restated_ios_catches_the_cut_box():
    # a 8 x 8 piece (tile 1) inside its 24 x 8 full version (tile 0): IoU = 1 / 3, IOS = 1
    tiles = [(0, 0, 40, 32), (24, 0, 64, 32)]
    lists = _lists([box(28, 16, 24, 8, 0.9, 0)], [box(28 - 24 + 4, 16, 8, 8, 0.7, 0)])
    assert tileref.merge_one(lists, tiles, 64, 32, 40, 32, merge_thresh=0.5)[1] == 2
    out, n, org, st = tileref.merge_one(lists, tiles, 64, 32, 40, 32, merge_thresh=0.5, flags=tileref.MATCH_IOS)
    assert n == 1 and tuple(org[0]) == (0, 0) and st["suppressed"] == 1
    assert tileref.merge_one(lists, tiles, 64, 32, 40, 32, merge_thresh=0.3)[1] == 1  # 1 / 3 > 0.3


def test_restated_rules_and_counters():
    tiles = [(0, 0, 40, 32), (24, 0, 64, 32)]
    nan, inf = float("nan"), float("inf")
    lists = _lists([box(10, 10, 4, 4, 0.9), box(nan, 10, 4, 4), box(10, 10, 0, 4), box(10, 10, 4, -1), box(10, 10, 4, 4, inf), box(12, 20, 4, 4, 0.8)],
                   [box(30, 10, 6, 6, 0.7)])
    out, n, org, st = tileref.merge_one(lists, tiles, 64, 32, 40, 32)
    assert tuple(st) == (3, 0, 4, 0, 0, 0) and [tuple(o) for o in org[:3]] == [(0, 0), (0, 5), (1, 0)]
    out, n, org, st = tileref.merge_one(lists, tiles, 64, 32, 40, 32, max_per_tile=2)
    assert tuple(st) == (2, 4, 1, 0, 0, 0)
    # the edge rule: tile 0's right side (x = 40) and tile 1's left side (x = 24) are interior, the others lie on the frame border
    lists = _lists([box(37, 16, 4, 4, 0.9), box(2, 2, 4, 4, 0.8), box(34, 16, 4, 4, 0.7)], [box(3, 16, 4, 4, 0.6), box(38, 30, 4, 4, 0.5), box(6, 16, 4, 4, 0.4)])
    out, n, org, st = tileref.merge_one(lists, tiles, 64, 32, 40, 32, edge_margin=4.0)
    # tile 0: r = 39 -> 40 - 39 < 4 cut; the corner box touches only border sides; r = 36 -> 4 < 4 is false.  tile 1: l = 25 -> 1 < 4 cut;
    # the bottom right corner box stays; l = 28 -> 4 < 4 is false
    assert st["edge"] == 2 and [tuple(o) for o in org[:n]] == [(0, 1), (0, 2), (1, 1), (1, 2)]
    assert tileref.merge_one(lists, tiles, 64, 32, 40, 32)[3]["edge"] == 0
    assert tileref.quota(16) == 128 and tileref.quota(1) == 1000 and tileref.quota(2) == 1000 and tileref.quota(3) == 682 and tileref.quota(64) == 32


def test_restated_map_agrees_with_float64():
    rng = np.random.default_rng(5)
    tiles = tileref.grid(96, 64, 32, 32, 8, 8) + [(0, 0, 96, 64), (10, 3, 58, 35)]
    for keep in (False, True):
        for tile in tiles:
            d = np.zeros(200, dtype=tileref.DET)
            d["x"], d["y"] = rng.uniform(0, 64, 200), rng.uniform(0, 64, 200)
            d["w"], d["h"] = rng.uniform(0.5, 40, 200), rng.uniform(0.5, 40, 200)
            X, Y, Wd, Hd = tileref.map_tile(d, tile, 64, 64, keep)
            x0, y0, x1, y1 = tile
            nw, nh, px, py = tileref.roi_target_np(x1 - x0, y1 - y0, 64, 64, keep)
            rx, ry = (x1 - x0) / nw, (y1 - y0) / nh
            for got, want in ((X, (d["x"].astype(np.float64) - px) * rx + x0), (Y, (d["y"].astype(np.float64) - py) * ry + y0),
                              (Wd, d["w"].astype(np.float64) * rx), (Hd, d["h"].astype(np.float64) * ry)):
                assert np.abs(got.astype(np.float64) - want).max() < 1e-3, (tile, keep)


def test_merge_cases_of_the_gpu_tests_bite():
    """the input conditions of tests/test_gpu_tile.py's merge cases (each must bite: 0 < kept < candidates wherever suppression is the point, the
    counters each case is about), against the restatement alone"""
    from test_gpu_tile import MERGE_CASES, merge_case
    for name in MERGE_CASES:
        W, H, tiles, dets, counts, kw, want = merge_case(name)
        assert dets.shape[0] == counts.size and counts.size % len(tiles) == 0 and want[0].shape[0] == counts.size // len(tiles), name


def test_restated_order_key():
    c = np.array([0.0, -0.0, 1e-30, 0.25, 0.5, 1.0, -1.0, 3e38, -3e38], dtype=F)
    k = tileref.ord_key(c).astype(np.int64)
    assert (np.argsort(-k, kind="stable") == [7, 5, 4, 3, 2, 0, 1, 6, 8]).all() and k.min() > 0
