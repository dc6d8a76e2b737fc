"""Redaction (include/mars_hip.h, "Redaction"), the part that needs no GPU: the numpy restatement tests/test_gpu_redact.py compares the device
against (tests/redactref.py) is pinned by a per-pixel loop, by the area-averaging rule it shares its rounding with, by properties and by
cases worked by hand; the entry points are exported, the records have their sizes, and arguments that can never be valid are refused up
front."""
import ctypes as C

import numpy as np
import pytest

import arearef
import redactref as R
from test_roi_cpu import box

DET = box(0, 0, 1, 1).dtype
NEW = ["mars_yolo_redact_frames", "mars_hip_redact_device", "mars_hip_redact_results", "mars_hip_redact", "mars_hip_redact_ms"]


def boxes_of(*b):
    return np.array(list(b), dtype=DET) if b else np.zeros(0, dtype=DET)


def random_frame(rng, W, H, fmt):
    return rng.integers(0, 256, R.frame_bytes(W, H, fmt), dtype=np.uint8)


def random_boxes(rng, n, W, H):
    b = np.zeros(n, dtype=DET)
    b["x"], b["y"] = rng.uniform(-0.1, 1.1, n) * W, rng.uniform(-0.1, 1.1, n) * H
    b["w"], b["h"] = rng.uniform(0, 0.6, n) * W, rng.uniform(0, 0.6, n) * H
    b["conf"] = rng.uniform(0, 1, n)
    return b


# ---- the per-pixel loop: the rule read literally, nothing shared with redactref but the rectangle --------------------------------------------
def loop_plane(src, w, h, ch, cov, mode, B, fill):
    """src: flat list of [h][w][ch] bytes; cov(x, y) -> bool"""
    out = list(src)
    for y in range(h):
        for x in range(w):
            if not cov(x, y):
                continue
            for c in range(ch):
                if mode == R.FILL:
                    out[(y * w + x) * ch + c] = fill[c]
                    continue
                cx, cy = x // B, y // B
                S = n = 0
                for yy in range(cy * B, min(h, (cy + 1) * B)):
                    for xx in range(cx * B, min(w, (cx + 1) * B)):
                        S += src[(yy * w + xx) * ch + c]
                        n += 1
                out[(y * w + x) * ch + c] = (S + n // 2) // n
    return out


def loop_frame(buf, W, H, fmt, U, mode, B, fill, flags=0):
    buf = [int(v) for v in buf]
    if fmt == R.RGB:
        return loop_plane(buf, W, H, 3, lambda x, y: U[y][x], mode, B, fill)
    luma = loop_plane(buf[:W * H], W, H, 1, lambda x, y: U[y][x], mode, B, fill[:1])
    cfill = (fill[2], fill[1]) if flags & R.NV12_VU else (fill[1], fill[2])
    any4 = lambda i, j: U[2 * j][2 * i] or U[2 * j][2 * i + 1] or U[2 * j + 1][2 * i] or U[2 * j + 1][2 * i + 1]  # noqa: E731
    return luma + loop_plane(buf[W * H:], W // 2, H // 2, 2, any4, mode, B // 2, cfill)


@pytest.mark.parametrize("fmt, W, H", [(R.RGB, 13, 9), (R.NV12, 14, 10)])
def test_loop_agrees_with_the_restatement(fmt, W, H):
    rng = np.random.default_rng(W)
    for cell in (2, 4, 8):
        for mode in (R.MOSAIC, R.FILL):
            for flags in ((0, R.NV12_VU) if fmt == R.NV12 else (0,)):
                buf = random_frame(rng, W, H, fmt)
                b = random_boxes(rng, 4, W, H)
                masks = [rng.integers(0, 2, (H, W)).astype(bool) if i % 2 else None for i in range(len(b))]
                U, st = R.union_np(b, W, H, masks=masks)
                assert 0 < st[3] < W * H and st[1] >= 1
                got = R.redact_frame_np(buf, W, H, fmt, U, mode, cell, (7, 99, 201), flags)
                assert got.tolist() == loop_frame(buf, W, H, fmt, U, mode, cell, (7, 99, 201), flags), (cell, mode, flags)


def test_mosaic_of_a_whole_frame_is_the_area_average():
    """W and H multiples of B, one box over everything: the mosaic is the area-averaged W / B x H / B image, every sample repeated B x B"""
    rng = np.random.default_rng(3)
    for W, H, B in [(24, 16, 2), (24, 16, 4), (24, 16, 8), (64, 32, 16), (64, 128, 64)]:
        img = rng.integers(0, 256, (H, W, 3), dtype=np.uint8)
        U, st = R.union_np(boxes_of(box(W / 2, H / 2, W, H)), W, H)
        assert U.all() and st == (1, 0, 0, W * H)
        got = R.redact_frame_np(img, W, H, R.RGB, U, R.MOSAIC, B).reshape(H, W, 3)
        small = arearef.area_resize_np(img, W // B, H // B).astype(np.int16) + 128
        assert np.array_equal(got, np.repeat(np.repeat(small, B, axis=0), B, axis=1))


def test_properties():
    rng = np.random.default_rng(11)
    for fmt, W, H in [(R.RGB, 37, 21), (R.NV12, 38, 22)]:
        buf = random_frame(rng, W, H, fmt)
        b = random_boxes(rng, 6, W, H)
        U, st = R.union_np(b, W, H)
        assert 0 < st[3] < W * H
        for cell in (2, 8, 16):
            # a constant frame stays constant under mosaic
            for v in (0, 1, 200, 255):
                flat = np.full(R.frame_bytes(W, H, fmt), v, dtype=np.uint8)
                assert (R.redact_frame_np(flat, W, H, fmt, U, R.MOSAIC, cell) == v).all()
            # fill is idempotent
            once = R.redact_frame_np(buf, W, H, fmt, U, R.FILL, cell, (9, 8, 7))
            assert np.array_equal(R.redact_frame_np(once, W, H, fmt, U, R.FILL, cell, (9, 8, 7)), once) and not np.array_equal(once, buf)
            # mosaic is idempotent where U is made of whole cells (a partly covered cell mixes its mean with the bytes it kept: {0, 100} with
            # the first pixel redacted gives {50, 100}, and again {75, 100})
            Uc = np.zeros((H, W), dtype=bool)
            Uc[:2 * cell, cell:3 * cell] = True
            Uc[H - H % cell:, :] = True  # the clipped last cell row (empty where H is a multiple)
            once = R.redact_frame_np(buf, W, H, fmt, Uc, R.MOSAIC, cell)
            assert np.array_equal(R.redact_frame_np(once, W, H, fmt, Uc, R.MOSAIC, cell), once) and not np.array_equal(once, buf)
        # the order of the boxes does not matter
        U2, st2 = R.union_np(b[::-1], W, H)
        assert np.array_equal(U, U2) and st == st2
        # a box entirely outside changes nothing and counts as skipped
        far = boxes_of(box(W + 50, H / 2, 10, 10), box(-30, -30, 8, 8))
        U3, st3 = R.union_np(far, W, H)
        assert not U3.any() and st3 == (0, 0, 2, 0)
        assert np.array_equal(R.redact_frame_np(buf, W, H, fmt, U3, R.MOSAIC, 2), buf)
        # a masked region is a subset of the same box unmasked
        masks = [rng.integers(0, 2, (H, W)).astype(bool) for _ in b]
        Um, stm = R.union_np(b, W, H, masks=masks)
        assert not (Um & ~U).any() and 0 < stm[3] < st[3] and stm[1] == stm[0] == st[0]
    one = np.array([[0, 100]], dtype=np.uint8).reshape(1, 2, 1)
    first = np.array([[True, False]])
    a = R.redact_plane_np(one, first, R.MOSAIC, 2, (0,))
    assert a.reshape(-1).tolist() == [50, 100] and R.redact_plane_np(a, first, R.MOSAIC, 2, (0,)).reshape(-1).tolist() == [75, 100]


def test_nv12_chroma_of_a_one_pixel_region():
    W, H = 8, 6
    buf = np.arange(R.frame_bytes(W, H, R.NV12), dtype=np.uint8)
    U, st = R.union_np(boxes_of(box(5.5, 2.5, 1, 1)), W, H)  # pixel (5, 2) alone
    assert st == (1, 0, 0, 1) and U[2, 5]
    got = R.redact_frame_np(buf, W, H, R.NV12, U, R.FILL, 2, (1, 2, 3))
    changed = np.flatnonzero(got != buf).tolist()
    assert changed == [2 * W + 5, W * H + (1 * (W // 2) + 2) * 2, W * H + (1 * (W // 2) + 2) * 2 + 1]  # the pixel, and chroma sample (2, 1): U, V
    assert got[changed].tolist() == [1, 2, 3]
    got = R.redact_frame_np(buf, W, H, R.NV12, U, R.FILL, 2, (1, 2, 3), R.NV12_VU)
    assert got[changed].tolist() == [1, 3, 2]


def test_rgb_5x3_cell_2_by_hand():
    """clipped cells of 1 x 2 (right), 2 x 1 (below) and 1 x 1 (the corner); G = R + 1, B = R + 2, so their means are the red one's + 1, + 2"""
    red = np.array([[12, 20, 30, 40, 50], [60, 70, 80, 90, 100], [110, 120, 130, 140, 150]])
    img = np.stack([red, red + 1, red + 2], axis=-1).astype(np.uint8)
    U, st = R.union_np(boxes_of(box(2.5, 1.5, 5, 3)), 5, 3)
    assert st == (1, 0, 0, 15)
    got = R.redact_frame_np(img, 5, 3, R.RGB, U, R.MOSAIC, 2).reshape(3, 5, 3)
    # (12 + 20 + 60 + 70 + 2) / 4 = 41 (40.5 rounds up); 240 / 4 = 60; (50 + 100 + 1) / 2 = 75; (110 + 120 + 1) / 2 = 115; 135; 150
    want = np.array([[41, 41, 60, 60, 75], [41, 41, 60, 60, 75], [115, 115, 135, 135, 150]])
    assert np.array_equal(got, np.stack([want, want + 1, want + 2], axis=-1))
    # two pixels of the top row: the means are still those of the whole cells, everything else keeps its value
    U, st = R.union_np(boxes_of(box(2, 0.5, 2, 1)), 5, 3)
    assert st == (1, 0, 0, 2) and U[0].tolist() == [False, True, True, False, False]
    got = R.redact_frame_np(img, 5, 3, R.RGB, U, R.MOSAIC, 2).reshape(3, 5, 3)
    want = red.copy()
    want[0, 1], want[0, 2] = 41, 60
    assert np.array_equal(got, np.stack([want, want + 1, want + 2], axis=-1))


def test_nv12_6x4_cell_4_by_hand():
    """Y[y][x] = 10 y + x; U[j][i] = 100 + 10 j + i, V = U + 100.  Luma cells: 4 x 4 and 2 x 4; chroma cells (2 samples a side): 2 x 2 and 1 x 2"""
    W, H = 6, 4
    y = np.array([[10 * r + x for x in range(W)] for r in range(H)])
    u = np.array([[100 + 10 * j + i for i in range(3)] for j in range(2)])
    buf = np.concatenate([y.reshape(-1), np.stack([u, u + 100], axis=-1).reshape(-1)]).astype(np.uint8)
    U, st = R.union_np(boxes_of(box(3.5, 1.5, 1, 1)), W, H)  # pixel (3, 1) alone
    assert st == (1, 0, 0, 1)
    got = R.redact_frame_np(buf, W, H, R.NV12, U, R.MOSAIC, 4)
    want = buf.copy()
    want[1 * W + 3] = 17                     # (264 + 8) / 16
    want[W * H + 2] = 106                    # chroma sample (1, 0): (100 + 101 + 110 + 111 + 2) / 4
    want[W * H + 3] = 206
    assert np.array_equal(got, want)
    U, st = R.union_np(boxes_of(box(3, 2, 6, 4)), W, H)  # everything
    got = R.redact_frame_np(buf, W, H, R.NV12, U, R.MOSAIC, 4)
    assert got[:W * H].reshape(H, W).tolist() == [[17, 17, 17, 17, 20, 20]] * 4    # (156 + 4) / 8 = 20
    assert got[W * H:].reshape(2, 3, 2).tolist() == [[[106, 206], [106, 206], [107, 207]]] * 2  # (102 + 112 + 1) / 2 = 107


def test_restated_selection():
    d = np.array([box(20, 20, 10, 10, 0.9, 1), box(30, 30, 10, 10, 0.8, 2), box(40, 30, 10, 10, 0.2, 1), box(50, 30, 10, 10, 0.7, 1)])
    ident = np.zeros(4, dtype=[("cls", "<i4"), ("score", "<f4")])
    ident["cls"], ident["score"] = [7, -1, 3, 5], [0.9, 0.0, 0.9, 0.3]
    assert R.select_np(d) == [0, 1, 2, 3]
    assert R.select_np(d, min_conf=0.5, classes=(1, 1)) == [0, 3]
    assert R.select_np(d, idents=ident, ident_min=0.5) == [1, 3] and R.select_np(d, idents=ident) == [1]


# ---- exports, record sizes, refusals --------------------------------------------------------------------------------------------------
def test_redact_symbols_are_exported(marsrt):
    L = marsrt.lib()
    for n in NEW:
        assert n in marsrt.EXPORTS["mars_hip.h"], n
        assert hasattr(L, n), n
    assert callable(marsrt.redact_frames) and callable(marsrt.Model.redact) and callable(marsrt.Model.redact_device)
    assert callable(marsrt.Model.redact_results)


def test_redact_record_sizes(marsrt, tmp_path):
    import os
    import subprocess
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    src = tmp_path / "redact_abi.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "mars_hip.h"\n'
                   'int main(void){ printf("%zu %zu %zu %zu %zu %u %u %d", sizeof(mars_redact_stats_t), sizeof(mars_hip_redact_opts_t),\n'
                   ' offsetof(mars_hip_redact_opts_t, fill), offsetof(mars_hip_redact_opts_t, expand), offsetof(mars_hip_redact_opts_t, flags),\n'
                   ' MARS_REDACT_USE_MASKS, MARS_REDACT_SPARE_IDENTIFIED, MARS_REDACT_FILL); return 0; }\n')
    exe = tmp_path / "redact_abi"
    subprocess.run(["gcc", "-I", os.path.join(root, "include"), str(src), "-o", str(exe)], check=True)
    got = subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.split()
    O = marsrt.RedactOpts
    assert got == [str(marsrt.REDACT_STATS_DTYPE.itemsize), str(C.sizeof(O)), str(O.fill.offset), str(O.expand.offset), str(O.flags.offset),
                   str(marsrt.REDACT_USE_MASKS), str(marsrt.REDACT_SPARE_IDENTIFIED), str(marsrt.REDACT_FILL)]
    assert marsrt.REDACT_STATS_DTYPE == R.STATS


def test_redact_bad_arguments_are_refused_up_front(marsrt):
    L = marsrt.lib()
    BAD_FILE, BAD_TENSOR = marsrt.MARS_ERR_INVALID_FILE, marsrt.MARS_ERR_INVALID_TENSOR
    frames = np.zeros(2 * 6 * 4 * 3, dtype=np.uint8)
    boxes = np.zeros(2, dtype=marsrt.DET_DTYPE)
    boxes["x"], boxes["y"], boxes["w"], boxes["h"] = 3, 2, 4, 3
    fo = np.zeros(2, dtype=np.int32)
    mo = np.zeros(2, dtype=np.int32)
    out = np.full(frames.size, 77, dtype=np.uint8)
    stats = np.full(2, 77, dtype=marsrt.REDACT_STATS_DTYPE)

    def call(o, n_frames=2, n_boxes=2, fr=frames, bx=boxes, fob=fo, dst=out, mw=None, mob=None):
        ptr = lambda a: None if a is None else a if isinstance(a, int) else a.ctypes.data  # noqa: E731
        return L.mars_yolo_redact_frames(ptr(fr), n_frames, ptr(bx), ptr(fob), n_boxes, ptr(mw), ptr(mob), None if o is None else C.byref(o),
                                         ptr(dst), stats.ctypes.data)

    good = marsrt.redact_opts(6, 4)
    nv = marsrt.CAMERA_NV12
    bad = [marsrt.redact_opts(0, 4), marsrt.redact_opts(6, -4),                                   # non-positive sizes
           marsrt.redact_opts(6, 4, fmt=2), marsrt.redact_opts(6, 4, fmt=-1),                     # an unknown format
           marsrt.redact_opts(6, 4, src_flags=2),                                                 # an NV12 flag on RGB frames
           marsrt.redact_opts(6, 4, fmt=nv, src_flags=4),                                         # an unknown NV12 flag bit
           marsrt.redact_opts(5, 4, fmt=nv), marsrt.redact_opts(6, 3, fmt=nv),                    # odd NV12 sizes
           marsrt.redact_opts(6, 4, mode=2), marsrt.redact_opts(6, 4, mode=-1),                   # an unknown mode
           marsrt.redact_opts(6, 4, flags=4), marsrt.redact_opts(6, 4, flags=0x80000000),         # an unknown flag bit
           marsrt.redact_opts(6, 4, cell=1), marsrt.redact_opts(6, 4, cell=3), marsrt.redact_opts(6, 4, cell=24),
           marsrt.redact_opts(6, 4, cell=128), marsrt.redact_opts(6, 4, cell=-2),                 # a cell outside the set
           marsrt.redact_opts(6, 4, expand=-1.0), marsrt.redact_opts(6, 4, expand=float("nan")), marsrt.redact_opts(6, 4, expand=float("inf")),
           marsrt.redact_opts(6, 4, min_conf=-0.5), marsrt.redact_opts(6, 4, min_conf=float("nan")),
           marsrt.redact_opts(6, 4, ident_min=-0.5), marsrt.redact_opts(6, 4, ident_min=float("nan")), marsrt.redact_opts(6, 4, ident_min=1.5),
           marsrt.redact_opts(6, 4, classes=(0, -1)),
           marsrt.redact_opts(8193, 3, fmt=nv), marsrt.redact_opts(8193, 4, cell=3)]              # two faults: these come before the size limit
    P = C.POINTER(marsrt.MarsModel)
    a = marsrt.MarsModel()  # never looked into: the refusals come first
    for o in bad:
        assert call(o) == BAD_FILE
        assert L.mars_hip_redact_device(C.pointer(a), frames.ctypes.data, None, C.byref(o)) == BAD_FILE
        assert L.mars_hip_redact(C.pointer(a), frames.ctypes.data, C.byref(o), None) == BAD_FILE
    for o in (marsrt.redact_opts(8193, 4), marsrt.redact_opts(6, 8193), marsrt.redact_opts(8194, 8194, fmt=nv)):  # beyond 8192
        assert call(o) == BAD_TENSOR
        assert L.mars_hip_redact_device(C.pointer(a), frames.ctypes.data, None, C.byref(o)) == BAD_TENSOR
        assert L.mars_hip_redact(C.pointer(a), frames.ctypes.data, C.byref(o), None) == BAD_TENSOR
    assert call(None) == BAD_FILE
    for kw in (dict(n_frames=0), dict(n_frames=-1), dict(n_boxes=-1), dict(fr=None), dict(dst=None), dict(bx=None), dict(fob=None),
               dict(n_frames=65536), dict(n_boxes=65536),
               dict(mob=mo),                                                                      # a mask index without mask words
               dict(dst=frames.ctypes.data + 1), dict(dst=frames.ctypes.data + frames.size - 1),  # a partial overlap, behind the source
               dict(fr=frames.ctypes.data + 36, n_frames=1, dst=frames.ctypes.data)):             # ... in front of it
        assert call(good, **kw) == BAD_FILE, kw
    assert (out == 77).all() and stats.tobytes() == np.full(2, 77, dtype=marsrt.REDACT_STATS_DTYPE).tobytes()  # nothing was written
    assert L.mars_hip_redact_device(P(), frames.ctypes.data, None, C.byref(good)) == BAD_FILE    # no model
    assert L.mars_hip_redact_device(C.pointer(a), None, None, C.byref(good)) == BAD_FILE         # no frames
    assert L.mars_hip_redact_device(C.pointer(a), frames.ctypes.data, None, None) == BAD_FILE    # no options
    assert L.mars_hip_redact(P(), frames.ctypes.data, C.byref(good), None) == BAD_FILE
    assert L.mars_hip_redact(C.pointer(a), None, C.byref(good), None) == BAD_FILE
    assert L.mars_hip_redact(C.pointer(a), frames.ctypes.data, None, None) == BAD_FILE
    assert L.mars_hip_redact_results(P(), None) == BAD_FILE
    assert L.mars_hip_redact_ms(P()) < 0
    for bad_call in (lambda: marsrt.redact_frames(frames[:-1], boxes, fo, good), lambda: marsrt.redact_frames(frames, boxes, fo[:1], good),
                     lambda: marsrt.redact_frames(frames, boxes, fo, good, mask_words=np.zeros((1, 4, 1), np.uint32), mask_of_box=[0, 1])):
        with pytest.raises(ValueError):
            bad_call()
