"""Instance masks in frame pixels on the device (mars_yolo_masks_native, mars_hip_detect_seg_native), bit for bit against the restatement of
include/mars_hip.h "Instance masks in frame pixels" (tests/maskupref.py).  The graphs and the expected detections are those of
tests/test_gpu_yolo_seg.py."""
import numpy as np
import pytest

import maskupref
import segref
from test_gpu_yolo_dfl import decode_dfl, head_bytes
from test_gpu_yolo_heads import letterbox_map, nms
from test_gpu_yolo_seg import DFL_KW, chw_bytes, fill, origins_dfl, seg_graph, sort_nms_idx

pytestmark = pytest.mark.gpu

F32 = np.float32


def geom_of(gpu, g):
    return gpu.mask_geom(g.in_w, g.in_h, g.out_w, g.out_h, nw=g.nw, nh=g.nh, px=g.px, py=g.py, base_w=g.base_w, base_h=g.base_h)


def random_boxes(gpu, rng, n, g):
    """boxes over the base grid, some of them reaching beyond it; box 0 covers everything, with a confidence of 0 (the host form takes all)"""
    b = np.zeros(n, dtype=gpu.DET_DTYPE)
    b["x"], b["y"] = rng.uniform(-0.1, 1.1, n) * g.base_w, rng.uniform(-0.1, 1.1, n) * g.base_h
    b["w"], b["h"] = rng.uniform(0, 1.1, n) * g.base_w, rng.uniform(0, 1.1, n) * g.base_h
    b["conf"] = rng.uniform(0, 1, n)
    if n:
        b[0] = (g.base_w / 2, g.base_h / 2, g.base_w, g.base_h, 0.0, 0)
    return b


def not_vacuous(recs):
    """some mask is neither empty nor its whole rectangle"""
    r = recs[recs["det"] >= 0]
    return bool(((r["area"] > 0) & (r["area"] < (r["x1"] - r["x0"]) * (r["y1"] - r["y0"]))).any())


def run_direct(gpu, coefs, proto, boxes, g, s=0.01, lm=0.0):
    n = len(boxes)
    recs, words = gpu.masks_native(coefs, proto, boxes, geom_of(gpu, g), s, lm)
    assert words.shape == (n, g.out_h, (g.out_w + 31) // 32)
    if n == 0:
        assert recs.shape == (0,)
        return recs, words
    wr, ww = maskupref.mask_frame(boxes, coefs, [s] * n, proto, g, logit_min=lm, max_per_frame=n, take_all=True)
    assert recs.tobytes() == wr.tobytes(), (g, n, lm, recs, wr)
    assert np.array_equal(words, ww), (g, n, lm, np.argwhere(words != ww)[:8])
    return wr, ww


OUT_WIDTHS = (31, 32, 33, 64, 65, 257)   # ragged last words, whole words, one past a word, one past a tile of 8 words
OUT_HEIGHTS = (17, 40, 45, 64, 65, 130)  # short, within one workgroup's span of 64 rows, exactly one span, one row past it, three spans


@pytest.mark.parametrize("nm", [1, 31, 32, 33, 64])
@pytest.mark.parametrize("ph, pw", [(5, 7), (20, 20), (40, 33)])
def test_host_pointer_form(gpu, nm, ph, pw):
    """every legal output width (no down-scaling: out_w >= PW) x n in 0, 1, 17, 64, without a letterbox, the input 4 x the prototypes"""
    rng = np.random.default_rng(nm * 100 + pw)
    proto = rng.integers(-128, 128, (nm, ph, pw), dtype=np.int8)
    proto[:, ph // 2, pw // 2] = 0
    for ow, oh in zip(OUT_WIDTHS, OUT_HEIGHTS):
        if ow < pw:
            continue
        g = maskupref.identity(4 * pw, 4 * ph, ow, max(oh, ph))
        for n in (0, 1, 17, 64):
            coefs = rng.integers(-128, 128, (n, nm), dtype=np.int8)
            wr, _ = run_direct(gpu, coefs, proto, random_boxes(gpu, rng, n, g), g, lm=0.0 if n != 17 else 0.7)
            assert n == 0 or not_vacuous(wr), (ow, n)


GEOMETRIES = [
    ("identity", maskupref.identity(64, 64, 16, 16)),
    ("4x", maskupref.identity(64, 64, 64, 64)),
    ("wide", maskupref.letterbox(100, 56, 64, 64)),
    ("wide, out 77 x 43", maskupref.letterbox(100, 56, 64, 64, 77, 43)),
    ("tall", maskupref.letterbox(56, 100, 64, 64)),
    ("tall, out 300 x 500", maskupref.letterbox(56, 100, 64, 64, 300, 500)),
]


@pytest.mark.parametrize("name, g", GEOMETRIES)
def test_geometries(gpu, name, g):
    """64 x 64 input, 16 x 16 prototypes.  The wide frame: (nw, nh, px, py) = (64, 35, 0, 14)"""
    assert name[:4] != "wide" or g[:6] == (64, 64, 64, 35, 0, 14)
    assert name[:4] != "tall" or g[:6] == (64, 64, 35, 64, 14, 0)
    rng = np.random.default_rng(len(name))
    nm, n = 32, 17
    proto = rng.integers(-128, 128, (nm, 16, 16), dtype=np.int8)
    coefs = rng.integers(-128, 128, (n, nm), dtype=np.int8)
    boxes = random_boxes(gpu, rng, n, g)
    for lm in (0.0, -3.0):
        wr, ww = run_direct(gpu, coefs, proto, boxes, g, lm=lm)
        assert not_vacuous(wr)
    if name == "identity":  # the consequence the header states: word for word the prototype masks
        for lm in (0.0, 0.7):
            recs, words = gpu.masks_native(coefs, proto, boxes, geom_of(gpu, g), 0.01, lm)
            r0, w0 = gpu.masks(coefs, proto, boxes, 64, 64, 0.01, lm)
            assert recs.tobytes() == r0.tobytes() and np.array_equal(words, w0)
            assert not_vacuous(r0)


def test_boxes_at_every_edge(gpu):
    """33 x 40 prototypes, 132 x 160 input, 264 x 80 output: fx = 2, fy = 0.5.  The kernel's fixed split of the grid: tiles of 8 words (256
    pixels) across, so two of them, and workgroup spans of 64 rows down, so rows 0 .. 63 and 64 .. 79; inside a span the bands of 16 rows
    start at the rectangle's own first row"""
    g = maskupref.identity(132, 160, 264, 80)
    rng = np.random.default_rng(5)
    nm = 33
    proto = rng.integers(-128, 128, (nm, 40, 33), dtype=np.int8)

    def box(x0, y0, x1, y1):  # base-grid edges -> (cx, cy, w, h); the halves below are exact in float32
        return ((x0 + x1) / 2, (y0 + y1) / 2, x1 - x0, y1 - y0, 0.5, 0)
    nan, inf = float("nan"), float("inf")
    cases = [
        box(40, 50, 90, 120),                                    # inside
        box(-20, 40, 30, 80), box(100, 40, 150, 80),             # clipped left, right
        box(40, -20, 90, 30), box(40, 140, 90, 200),             # ... above, below
        box(-10, -10, 140, 170), box(0, 0, 132, 160),            # everything
        box(50, 50, 50, 90), box(60, 60, 40, 90), box(200, 40, 260, 80), box(30, 300, 80, 310),  # empty: no width, negative, outside
        (nan, 80, 40, 40, 0.5, 0), (60, nan, 40, 40, 0.5, 0), (60, 80, nan, 40, 0.5, 0), (60, 80, 40, inf, 0.5, 0), (inf, 80, 40, 40, 0.5, 0),
        (60, 80, inf, inf, 0.5, 0), (-inf, -inf, 40, 40, 0.5, 0),
        box(16, 20, 32, 100),                                    # x0 = 32, x1 = 64: one whole word
        box(16, 32, 32, 64), box(128, 32, 132, 64),              # ... 16 rows from y0 = 16: one band; x0 = 256: the second tile column alone
        box(0, 32, 128, 64), box(127.5, 31, 128.5, 65),          # x1 = 256: the first tile column alone; one pixel over each tile edge
        box(15.75, 10, 16.25, 12),                               # x0 = 31, x1 = 33: across the word boundary
        box(20, 100, 60, 128), box(20, 128, 60, 150),            # y1 = 64: ends with the first span; y0 = 64: begins with the second
        box(20, 0, 60, 128), box(20, 127, 60, 129),              # y0 = 0, y1 = 64: the first span alone; one row on each side of the edge
        box(128, 128, 132, 160),                                 # x0 = 256, y0 = 64: the last tile of the last span alone
    ]
    boxes = np.array(cases, dtype=gpu.DET_DTYPE)
    n = len(boxes)
    coefs = rng.integers(-128, 128, (n, nm), dtype=np.int8)
    for lm in (0.0, 1.5):
        wr, ww = run_direct(gpu, coefs, proto, boxes, g, lm=lm)
        assert not_vacuous(wr)
    r = {k: tuple(wr[k][f] for f in ("x0", "y0", "x1", "y1")) for k in range(n)}
    assert r[0] == (80, 25, 180, 60) and r[5] == r[6] == (0, 0, 264, 80) and wr["area"][7:11].tolist() == [0] * 4
    assert r[18] == (32, 10, 64, 50) and r[19] == (32, 16, 64, 32) and r[20] == (256, 16, 264, 32) and r[21] == (0, 16, 256, 32)
    assert r[22] == (255, 15, 257, 33) and r[23] == (31, 5, 33, 6)
    assert r[24] == (40, 50, 120, 64) and r[25] == (40, 64, 120, 75) and r[26] == (40, 0, 120, 64) and r[27] == (40, 63, 120, 65)
    assert r[28] == (256, 64, 264, 80) and all(wr["area"][k] > 0 for k in range(24, 29))


def test_extreme_dot(gpu):
    """all bytes -128 at nm = 64: S = 2^36 at every pixel whatever the weights; (float)S * 2^-16 = 2^20 and the compare is strict"""
    proto = np.full((64, 5, 7), -128, dtype=np.int8)
    coefs = np.full((2, 64), -128, dtype=np.int8)
    g = maskupref.identity(28, 20, 45, 33)
    boxes = np.array([(14, 10, 28, 20, 0.5, 0), (10, 10, 9, 7, 0.5, 0)], dtype=gpu.DET_DTYPE)
    for lm, bit in ((0.0, 1), (1048575.5, 1), (1048576.0, 0)):
        wr, ww = run_direct(gpu, coefs, proto, boxes, g, s=1.0, lm=lm)
        assert wr["area"][0] == 45 * 33 * bit and (0 < wr["area"][1] < 45 * 33) == bool(bit)


def test_every_word_is_rewritten(gpu):
    """the same shapes twice: first every box covers everything with every bit set, then small boxes; the scratch block of the second call
    is, where the allocator hands the same memory out again, the first call's: whatever is not rewritten would show"""
    g = maskupref.letterbox(100, 56, 64, 64, 300, 168)
    rng = np.random.default_rng(9)
    nm, n = 4, 17
    proto = rng.integers(-128, 128, (nm, 16, 16), dtype=np.int8)
    coefs = rng.integers(-128, 128, (n, nm), dtype=np.int8)
    full = np.zeros(n, dtype=gpu.DET_DTYPE)
    full[:] = (50, 28, 200, 200, 0.5, 0)
    for k in range(2):
        wr, ww = run_direct(gpu, coefs, proto, full, g, lm=-1e30)
        assert (wr["area"] == 300 * 168).all()
        small = random_boxes(gpu, rng, n, g)[1:]
        small["w"] *= 0.2
        small["h"] *= 0.2
        wr, ww = run_direct(gpu, coefs[1:], proto, small, g)
        assert not_vacuous(wr) and wr["area"].max() < 300 * 168 // 4


def test_host_pointer_form_refusals(gpu):
    proto = np.zeros((4, 16, 16), np.int8)
    box = np.zeros(1, gpu.DET_DTYPE)
    row = np.zeros((1, 4), np.int8)
    ok = gpu.mask_geom(64, 64, 64, 64)
    gpu.masks_native(row, proto, box, ok, 0.01)
    for g in (gpu.mask_geom(64, 64, 15, 64), gpu.mask_geom(64, 64, 64, 15), gpu.mask_geom(64, 64, 0, 64), gpu.mask_geom(64, 64, 64, 8193),
              gpu.mask_geom(64, 64, 64, 64, base_h=0)):
        with pytest.raises(ValueError):
            gpu.masks_native(row, proto, box, g, 0.01)
    for kw in (dict(s=0.0), dict(s=-1.0), dict(s=float("nan")), dict(lm=float("inf"))):
        with pytest.raises(ValueError):
            gpu.masks_native(row, proto, box, ok, kw.get("s", 0.01), kw.get("lm", 0.0))
    with pytest.raises(ValueError):
        gpu.masks_native(np.zeros((1, 65), np.int8), np.zeros((65, 4, 4), np.int8), box, ok, 0.01)
    with pytest.raises(ValueError):
        gpu.masks_native(np.zeros((65, 4), np.int8), proto, np.zeros(65, gpu.DET_DTYPE), ok, 0.01)


# ---- through a model
def frame_parts(gpu, m, heads, coefs, pr, nchw, f, dfl_kw):
    """frame f of a model that has run -> (kept records in graph-input pixels, their coefficient rows, their product scales, prototypes)"""
    hs = []
    for b, c, cat, _, s in heads:
        bb, cb = head_bytes(gpu, m, f, b, c, cat, nchw)
        hs.append((np.ascontiguousarray(bb), np.ascontiguousarray(cb), dfl_kw["box_scales"], dfl_kw["cls_scales"], s))
    cand, _ = decode_dfl(hs, gpu.DET_DTYPE, dfl_kw["conf"])
    org = origins_dfl(hs, dfl_kw["conf"])
    keep = sort_nms_idx(cand, 0.45)
    kept = cand[keep]
    assert kept.tobytes() == nms(cand.copy(), 0.45).tobytes()
    ca = [np.ascontiguousarray(chw_bytes(m, t, f, nchw)) for t in coefs]
    cells = np.cumsum([0] + [h[1].shape[1] * h[1].shape[2] for h in hs])
    ps = F32(m.tensor_desc(pr).scale)
    rows, scales = [], []
    for o in org[keep]:
        k = int(np.searchsorted(cells, o, side="right")) - 1
        rows.append(ca[k].reshape(ca[k].shape[0], -1)[:, o - cells[k]])
        scales.append(F32(m.tensor_desc(coefs[k]).scale) * ps)
    return kept, rows, scales, np.ascontiguousarray(chw_bytes(m, pr, f, nchw))


@pytest.mark.parametrize("nchw", [False, True])
def test_through_a_model(gpu, nchw):
    """the hand-built seg graph at 64 x 64 (prototypes 16 x 16), batch 3, frame 1 without a detection: with and without a 100 x 56 source
    frame, the default and an explicit output grid, max_per_frame 1 and 16; then a prototype-size call that leaves the native block alone"""
    S, nm, B = 64, 32, 3
    d, heads, coefs, pr = seg_graph(nm, nchw, S)
    m = gpu.Model(d, batch=B)
    fill(m, 0x5E600000 + S, zero_frame=1)
    m.run()
    parts = [frame_parts(gpu, m, heads, coefs, pr, nchw, f, DFL_KW) for f in range(B)]
    assert len(parts[0][0]) > 3 and len(parts[1][0]) == 0
    last = None
    for src in (None, (100, 56)):
        kw = dict(DFL_KW, src=src) if src else DFL_KW
        plain = m.detect_dfl(**kw)
        for out in (None, (77, 43), (65, 70)):
            g = maskupref.letterbox(src[0], src[1], S, S, *(out or (0, 0))) if src else maskupref.identity(S, S, *(out or (S, S)))
            for mpf, lm in ((1, 0.0), (16, 0.0), (16, 5000.0)):
                opts = gpu.seg_opts(coefs, pr, max_per_frame=mpf, logit_min=lm)
                dets, recs, words, ow = m.detect_seg_native(opts, gpu.mask_native_opts(*out) if out else None, **kw)
                assert ow == g.out_w and words.shape == (B, mpf, g.out_h, (g.out_w + 31) // 32) and recs.shape == (B, mpf)
                some = False
                for f, (kept, rows, scales, proto) in enumerate(parts):
                    base = letterbox_map(kept, src[0], src[1], S, S) if src else kept
                    assert dets[f].tobytes() == base.tobytes() == plain[f].tobytes(), (src, out, f)
                    wr, ww = maskupref.mask_frame(base, rows, scales, proto, g, logit_min=lm, max_per_frame=mpf)
                    assert recs[f].tobytes() == wr.tobytes(), (src, out, mpf, lm, f, recs[f], wr)
                    assert np.array_equal(words[f], ww), (src, out, mpf, lm, f)
                    some |= not_vacuous(wr)
                assert (some or lm != 0.0) and (recs[1]["det"] == -1).all() and not words[1].any()
                assert gpu.lib().mars_hip_mask_native_ms(m.p) >= 0
                last = (recs, words, ow)
    # a prototype-size call on the same model: its own block; the native results stay fetchable and unchanged
    got = m.detect_seg(gpu.seg_opts(coefs, pr, max_per_frame=4), **DFL_KW)
    assert got[3] == S // 4 and got[2].shape == (B, 4, S // 4, 1)
    recs, words, ow = m.mask_native_results()
    assert recs.tobytes() == last[0].tobytes() and np.array_equal(words, last[1]) and ow == last[2]
    for f, (kept, rows, scales, proto) in enumerate(parts):
        wr, ww = segref.mask_frame(kept, rows, scales, proto, S, S, max_per_frame=4)
        assert got[1][f].tobytes() == wr.tobytes() and np.array_equal(got[2][f], ww)
    m.close()


def test_model_block_is_rewritten(gpu):
    """the model's result block is reused from call to call, so this is deterministic: first every slot of every frame that has detections
    is taken and every bit of its rectangle set (logit_min far below any value), then, on the same grid and with the same slot count, a
    min_conf that leaves slots unused: whatever the second call did not rewrite -- unused slots, rows and tiles off the rectangles -- would
    still hold the first call's bits"""
    S, nm, B, M = 64, 32, 3, 16
    d, heads, coefs, pr = seg_graph(nm, False, S)
    m = gpu.Model(d, batch=B)
    fill(m, 0x5E600000 + S, zero_frame=1)
    m.run()
    parts = [frame_parts(gpu, m, heads, coefs, pr, False, f, DFL_KW) for f in range(B)]
    levels = np.unique(parts[0][0]["conf"][:M])  # the confidences are table values: ties are common
    assert len(levels) >= 2
    mid = float(levels[-1])  # only the detections at the highest level pass
    kw = dict(DFL_KW, src=(100, 56))
    g = maskupref.letterbox(100, 56, S, S, 300, 170)
    nat = gpu.mask_native_opts(300, 170)
    for seg_kw in (dict(logit_min=-1e30), dict(min_conf=mid)):
        dets, recs, words, ow = m.detect_seg_native(gpu.seg_opts(coefs, pr, max_per_frame=M, **seg_kw), nat, **kw)
        for f, (kept, rows, scales, proto) in enumerate(parts):
            wr, ww = maskupref.mask_frame(letterbox_map(kept, 100, 56, S, S), rows, scales, proto, g, max_per_frame=M, **seg_kw)
            assert recs[f].tobytes() == wr.tobytes() and np.array_equal(words[f], ww), (seg_kw, f)
        taken = (recs[0]["det"] >= 0).sum()
        if "logit_min" in seg_kw:
            full = recs[0][:taken]
            assert taken > 3 and (full["area"] == (full["x1"] - full["x0"]) * (full["y1"] - full["y0"])).all() and full["area"].max() > 0
            first = taken
        else:
            assert 0 < taken < first and not words[0][taken:].any() and not_vacuous(recs[0])
    m.close()


def test_c_entry_point_that_fetches_everything(gpu):
    import ctypes as C
    S, nm, B = 64, 4, 2
    d, heads, coefs, pr = seg_graph(nm, False, S)
    m = gpu.Model(d, batch=B)
    fill(m, 0x5E600000 + S)
    m.run()
    want = m.detect_seg_native(gpu.seg_opts(coefs, pr), None, src=(100, 56), **DFL_KW)
    dets = np.zeros((B, gpu.MAX_DET), dtype=gpu.DET_DTYPE)
    counts = np.zeros(B, dtype=np.int32)
    recs = np.zeros((B, 16), dtype=gpu.MASK_DTYPE)
    words = np.zeros((B, 16, 56, 4), dtype=np.uint32)
    rc = gpu.lib().mars_hip_detect_seg_native(m.p, C.byref(gpu.yolo_dfl_heads(src=(100, 56), **DFL_KW)), C.byref(gpu.seg_opts(coefs, pr)), None,
                                              dets.ctypes.data, counts.ctypes.data_as(C.POINTER(C.c_int)), recs.ctypes.data, words.ctypes.data)
    assert rc == 0 and want[3] == 100
    assert all(dets[f, :counts[f]].tobytes() == want[0][f].tobytes() for f in range(B))
    assert recs.tobytes() == want[1].tobytes() and np.array_equal(words, want[2]) and recs["area"].max() > 0
    m.close()


def test_refusals(gpu):
    INV = gpu.MARS_ERR_INVALID_TENSOR
    S = 64
    d, heads, coefs, pr = seg_graph(4, False, S)
    m = gpu.Model(d, batch=2)
    with pytest.raises(gpu.MarsError) as e:
        m.mask_native_results()  # before any native call
    assert e.value.code == INV and gpu.lib().mars_hip_mask_native_ms(m.p) < 0
    fill(m, 3)
    m.run()
    m.detect_seg(gpu.seg_opts(coefs, pr), **DFL_KW)  # a prototype-size call is none either
    with pytest.raises(gpu.MarsError) as e:
        m.mask_native_results()
    assert e.value.code == INV
    opts = gpu.seg_opts(coefs, pr)
    bad = [
        (dict(out_w=15), {}), (dict(out_h=15), {}),                       # down-scaling: the prototypes are 16 x 16
        (dict(out_w=15, out_h=40), dict(src=(100, 56))),
        (dict(out_w=100, out_h=8), dict(src=(100, 56))),                  # 8 * 64 < 35 * 16: the letterboxed rows
        (dict(out_w=-1), {}), (dict(out_h=-5), {}), (dict(out_w=8193), {}), (dict(out_h=8193), {}),
        (dict(flags=1), {}), (dict(flags=0x80000000), {}),
        ({}, dict(src=(9000, 5000))),                                     # the default grid: the frame, beyond the limit
    ]
    for nat, kw in bad:
        with pytest.raises(gpu.MarsError) as e:
            m.detect_seg_native_device(opts, gpu.mask_native_opts(**nat), **dict(DFL_KW, **kw))
        assert e.value.code == INV, (nat, kw)
    for seg_kw in (dict(max_per_frame=65), dict(proto_scale=-0.5), dict(logit_min=float("nan")), dict(coefs=[coefs[1], coefs[0], coefs[2]])):
        with pytest.raises(gpu.MarsError) as e:  # what mars_hip_detect_seg_device refuses
            m.detect_seg_native_device(gpu.seg_opts(seg_kw.pop("coefs", coefs), pr, **seg_kw), None, **DFL_KW)
        assert e.value.code == INV, seg_kw
    with pytest.raises(gpu.MarsError) as e:
        m.detect_seg_native_device(None, None, **DFL_KW)
    assert e.value.code == INV
    with pytest.raises(gpu.MarsError) as e:
        m.mask_native_results()  # still none
    assert e.value.code == INV
    m.pipe_open(download_outputs=False, detect=True, dfl_heads=gpu.yolo_dfl_heads(**DFL_KW))
    with pytest.raises(gpu.MarsError) as e:
        m.detect_seg_native_device(opts, None, **DFL_KW)
    assert e.value.code == INV
    m.pipe_close()
    m.run()
    good = m.detect_seg_native(opts, gpu.mask_native_opts(16, 16), **DFL_KW)  # and the good configuration passes: the identity
    proto_size = m.detect_seg(opts, **DFL_KW)
    assert good[1].tobytes() == proto_size[1].tobytes() and np.array_equal(good[2], proto_size[2]) and good[1]["area"].max() > 0
    # a refused call leaves the last results fetchable
    with pytest.raises(gpu.MarsError):
        m.detect_seg_native_device(opts, gpu.mask_native_opts(15, 16), **DFL_KW)
    again = m.mask_native_results()
    assert again[0].tobytes() == good[1].tobytes() and np.array_equal(again[1], good[2])
    m.close()
