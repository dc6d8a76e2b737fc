"""The restatement of "Overlay" (tests/overlayref.py) and the library's host functions (the font, the text, the palette, the colour
conversion) on cases worked by hand; the owner maps against the per-pixel rule; and the case generators of tests/test_gpu_overlay.py run
through the restatement: no case may be vacuous.  No GPU."""
import os

import numpy as np
import pytest

import overlayref as O
import test_gpu_overlay as G

HERE = os.path.dirname(os.path.abspath(__file__))


@pytest.fixture(scope="module", autouse=True)
def bound(marsrt):
    O.bind(marsrt)


def one(W, H, boxes, **kw):
    """one RGB frame of zeros with these boxes -> ([H][W][3], the statistics, the info)"""
    b = np.array(boxes, dtype=G.DET)
    extra = {k: kw.pop(k) for k in ("keys", "texts", "mask_words", "mask_of_box", "kpts") if k in kw}
    src = kw.pop("src", np.zeros(W * H * 3, dtype=np.uint8))
    out, st, infos = O.overlay_frames_np(src[None], b, np.zeros(len(b), dtype=np.int32), W, H, O.RGB, **extra, **kw)
    return out[0].reshape(H, W, 3), st[0], infos[0]


# ---- outline ---------------------------------------------------------------------------------------------------------------------------------
def test_outline_of_a_3x3_box_and_a_thickness_above_half_the_box():
    red = [(200, 10, 20)]
    img, st, _ = one(7, 6, [(3.5, 2.5, 3, 3, 0.5, 0)], layers=O.BOXES, thickness=1, palette=red)  # R = (2, 1, 5, 4)
    on = (img == red[0]).all(axis=2)
    want = np.zeros((6, 7), dtype=bool)
    want[1:4, 2:5] = True
    want[2, 3] = False  # the one inner pixel
    assert np.array_equal(on, want) and st["pixels"] == 8 and st["boxes"] == 1 and not img[~want].any()
    for t in (2, 16):  # the inner rectangle is empty: all of R
        img, st, _ = one(7, 6, [(3.5, 2.5, 3, 3, 0.5, 0)], layers=O.BOXES, thickness=t, palette=red)
        want[2, 3] = True
        assert np.array_equal((img == red[0]).all(axis=2), want) and st["pixels"] == 9
    img, st, _ = one(12, 9, [(6, 4, 8, 5, 0.5, 0)], layers=O.BOXES, thickness=2, palette=red)  # R = (2, 1, 10, 7): 8 x 6, inner 4 x 2
    assert st["pixels"] == 48 - 8 and not (img[3:5, 4:8] == red[0]).all(axis=2).any()


# ---- tint ------------------------------------------------------------------------------------------------------------------------------------
def test_tint_blend_at_its_ends():
    mw = np.array([[[0b0110]], [[0b1111]]], dtype=np.uint32)[:1].repeat(2, axis=1)  # a 2-row mask: pixels 1 and 2
    for a, src, col, want in ((1, 0, 255, 1), (1, 255, 0, 254), (256, 0, 255, 255), (256, 255, 0, 0), (1, 255, 255, 255), (256, 7, 7, 7), (0, 0, 255, 96),
                              (128, 255, 0, 128)):
        s = np.full(4 * 2 * 3, src, dtype=np.uint8)
        img, st, _ = one(4, 2, [(2, 1, 4, 2, 0.5, 0)], layers=O.MASKS, alpha=a, palette=[(col,) * 3], mask_words=mw, mask_of_box=[0], src=s)
        assert (img[:, 1:3] == want).all() and (img[:, [0, 3]] == src).all() and st["pixels"] == 4 and st["masked"] == 1, (a, src, col)
    assert (0 * 255 + 255 * 1 + 128) >> 8 == 1 and (255 * 255 + 0 * 1 + 128) >> 8 == 254 and (255 * 160 + 128) >> 8 == 159


# ---- colours ---------------------------------------------------------------------------------------------------------------------------------
YUV = {  # (R, G, B): (limited range, full range), worked by hand from the formulas
    (0, 0, 0): ((16, 128, 128), (0, 128, 128)),
    (255, 255, 255): ((235, 128, 128), (255, 128, 128)),
    (255, 0, 0): ((82, 90, 240), (77, 85, 255)),
    (0, 255, 0): ((144, 54, 34), (149, 43, 21)),
    (0, 0, 255): ((41, 240, 110), (29, 255, 107)),
}


def test_both_yuv_conversions(marsrt):
    for rgb, (lim, full) in YUV.items():
        for flags, want in ((0, lim), (marsrt.NV12_FULL_RANGE, full)):
            assert marsrt.rgb_to_yuv(rgb, flags) == want == O.rgb_to_yuv_np(rgb, flags), (rgb, flags)
            vu = (want[0], want[2], want[1])
            assert marsrt.rgb_to_yuv(rgb, flags | marsrt.NV12_VU) == vu == O.rgb_to_yuv_np(rgb, flags | marsrt.NV12_VU)
    rng = np.random.default_rng(0)
    for rgb in rng.integers(0, 256, (200, 3)):
        for flags in range(4):
            assert marsrt.rgb_to_yuv(rgb, flags) == O.rgb_to_yuv_np(rgb, flags)
    # full range: (128 * 255 + 128) >> 8 = 128, + 128 = 256, clamped; (-43 * 255 + 128) >> 8 = -43 (an arithmetic shift rounds down), + 128 = 85
    assert (128 * 255 + 128) >> 8 == 128 and (-43 * 255 + 128) >> 8 == -43


def test_text_colour_at_luma_127_and_128_and_the_default_palette(marsrt):
    assert O.text_white((127, 127, 127)) and not O.text_white((128, 128, 128))  # (256 * v + 128) >> 8 = v
    for rgb, white in (((127, 127, 127), True), ((128, 128, 128), False)):
        img, _, _ = one(40, 12, [(20, 10.5, 30, 3, 0.5, 0)], layers=O.LABELS, scale=1, palette=[rgb], texts=[b"I"])
        strip = img[0:9, 5:12].reshape(-1, 3)  # R = (5, 9, 35, 12): the strip is 7 x 9 at (5, 0)
        assert {tuple(p) for p in strip} == {rgb, (255, 255, 255) if white else (0, 0, 0)}
    pal = marsrt.overlay_default_palette()
    assert pal.shape == (16, 3) and len({tuple(p) for p in pal}) == 16
    assert {O.text_white(p) for p in pal} == {True, False}  # both text colours occur


# ---- text ------------------------------------------------------------------------------------------------------------------------------------
def test_confidence_percentage(marsrt):
    for conf, want in ((0.005, b"1%"), (0.995, b"100%"), (1.0, b"100%"), (0.0, b"0%"), (0.004, b"0%"), (0.5, b"50%"), (7.0, b"100%"), (-1.0, b"0%"),
                       (float("nan"), b"0%")):
        assert marsrt.overlay_text(0, conf, text=O.TEXT_CONF) == want == O.text_np(0, conf, text=O.TEXT_CONF), conf
    # float32: 0.005 is 0.004999999888..., times 100 rounds to 0.5 exactly, + 0.5 = 1.0: the two roundings are separate (one fused step
    # would give 0.99999998... and 0 %)
    assert float(np.float32(0.005)) * 100 + 0.5 < 1 and np.float32(np.float32(0.005) * np.float32(100)) == 0.5
    rng = np.random.default_rng(3)
    for conf in rng.uniform(0, 1, 2000).astype(np.float32):
        assert marsrt.overlay_text(3, conf) == O.text_np(3, conf)


def test_text_composition(marsrt):
    names = G.names_table()
    t = lambda cls, conf, tid=-1, text=0, nm=names: marsrt.overlay_text(cls, conf, tid, text, nm)
    assert t(0, 0.5) == b"person 50%"
    assert t(1, 0.25) == b"a name of 16 by. 25%"                              # a name of exactly 16 bytes has no NUL
    assert t(2, 0.5) == b"2 50%" and t(6, 0.5) == b"6 50%" and t(3, 0.5, nm=None) == b"3 50%"  # an empty name, no name, no table: the number
    assert t(-7, 0.5) == b"-7 50%" and t(-2147483648, 0.5, text=O.TEXT_CLASS) == b"-2147483648"
    assert t(1, 1.0, 123456, 7) == b"a name of 16 by. #123456"[:24] == b"a name of 16 by. #123456" and len(t(1, 1.0, 1234567, 7)) == 24
    assert t(1, 1.0, 1234567, 7) == b"a name of 16 by. #123456"                 # the 24-byte cut
    assert t(3, 0.5, -1, 7) == b"car 50%" and t(3, 0.5, 0, 7) == b"car #0 50%"  # an untracked detection has no track part
    assert t(3, 0.5, 9, O.TEXT_TRACK) == b"#9" and t(3, 0.5, -1, O.TEXT_TRACK) == b""
    assert t(0, 0.5, 2147483647, O.TEXT_TRACK | O.TEXT_CONF) == b"#2147483647 50%"
    rng = np.random.default_rng(4)
    for _ in range(500):
        cls, tid, text = int(rng.integers(-3, 9)), int(rng.integers(-2, 100000)), int(rng.integers(0, 8))
        conf = np.float32(rng.uniform(0, 1))
        assert marsrt.overlay_text(cls, conf, tid, text, names) == O.text_np(cls, conf, tid, text, names), (cls, tid, text)


# ---- labels ----------------------------------------------------------------------------------------------------------------------------------
def art(img, colour):
    return ["".join("#" if tuple(p) == colour else "." for p in row) for row in img]


def test_label_placement_flip_and_cut():
    c = [(10, 20, 30)]
    # s = 2: Hl = 18, Wl = 2 * 13 = 26.  R = (4, 20, 14, 26): the strip sits above the box at (4, 2)
    img, st, info = one(40, 30, [(9, 23, 10, 6, 0.5, 0)], layers=O.LABELS, palette=c, texts=[b"Hi"])
    cov = info["covered"]
    assert cov[2:20, 4:30].all() and cov.sum() == 18 * 26 and st["labels"] == 1
    # y0 = 17 < Hl: inside the box's top, at (4, 17)
    img, st, info = one(40, 40, [(9, 20, 10, 6, 0.5, 0)], layers=O.LABELS, palette=c, texts=[b"Hi"])
    assert info["covered"][17:35, 4:30].all() and info["covered"].sum() == 18 * 26
    # y0 = 18 = Hl: above, at row 0
    img, st, info = one(40, 40, [(9, 21, 10, 6, 0.5, 0)], layers=O.LABELS, palette=c, texts=[b"Hi"])
    assert info["covered"][0:18, 4:30].all() and info["covered"].sum() == 18 * 26
    # cut at the right edge and at the bottom: x0 = 30 of W = 40, y0 = 0 (inside), H = 10
    img, st, info = one(40, 10, [(35, 2, 10, 4, 0.5, 0)], layers=O.LABELS, palette=c, texts=[b"Hi"])
    assert info["covered"][:, 30:].all() and info["covered"].sum() == 10 * 10
    full, _, _ = one(80, 40, [(35, 21, 10, 6, 0.5, 0)], layers=O.LABELS, palette=c, texts=[b"Hi"])  # the same strip, whole, at (30, 0)
    assert np.array_equal(img[:, 30:], full[:10, 30:40])
    # an empty text: no strip
    img, st, info = one(40, 30, [(9, 23, 10, 6, 0.5, 0)], layers=O.LABELS, palette=c, texts=[b""])
    assert st["labels"] == 0 and st["pixels"] == 0 and st["boxes"] == 1


def test_golden_label(marsrt):
    """one rendered label as ASCII art: '#' text, '+' the strip's colour, '.' the source"""
    c = (10, 20, 30)
    img, _, _ = one(64, 22, [(32, 15, 60, 8, 0.875, 0)], layers=O.LABELS, scale=1, palette=[c], names=G.names_table(), text=7)
    got = ["".join("#" if tuple(p) == (255, 255, 255) else "+" if tuple(p) == c else "." for p in row) for row in img[:12]]
    want = open(os.path.join(HERE, "golden", "overlay_label.txt")).read().split("\n")
    assert got == [w for w in want if w], "\n" + "\n".join(got)


# ---- markers ---------------------------------------------------------------------------------------------------------------------------------
def test_markers_cut_and_dropped():
    kp = np.zeros((1, 6), dtype=G.KPT)
    nan = float("nan")
    kp[0] = [(-0.5, -0.5, 1.0), (-8.5, 5, 1.0), (29.2, 19.9, 0.5), (38.5, 5, 1.0), (5, nan, 1.0), (5, 5, 0.49)]
    pal = [(1, 1, 1), (2, 2, 2), (3, 3, 3), (4, 4, 4)]
    img, st, info = one(30, 20, [(15, 10, 4, 4, 0.5, 0)], layers=O.KEYPOINTS, radius=1, palette=pal, kpts=kp)
    # j = 0: cx = cy = -1, the square [-2, 0]^2 cut to the corner pixel; j = 1: cx = -9 < -8, dropped; j = 2: (29, 19), cut to 2 x 2, colour 2 % 4;
    # j = 3: cx = 38 = W + 8, kept, empty after the cut; j = 4: not finite; j = 5: v below 0.5
    assert st["markers"] == 3 and st["pixels"] == 1 + 4 and tuple(img[0, 0]) == pal[0] and (img[18:, 28:] == pal[2]).all()
    assert [m[1] for m in info["marks"]] == [0, 2, 3]
    kp[0, 3] = (38.5 + 1, 5, 1.0)  # cx = 39 > W + 8: dropped
    _, st, _ = one(30, 20, [(15, 10, 4, 4, 0.5, 0)], layers=O.KEYPOINTS, radius=1, palette=pal, kpts=kp)
    assert st["markers"] == 2
    kp[0, 0] = (-0.5, -0.5, 1.0)
    img, st, _ = one(30, 20, [(15, 10, 4, 4, 0.5, 0)], layers=O.KEYPOINTS, radius=8, palette=pal, kpts=kp)
    assert (img[:8, :8] == pal[0]).all() and not (img[8, :8] == pal[0]).any()  # [-9, 7]^2 cut


# ---- the font --------------------------------------------------------------------------------------------------------------------------------
def test_font(marsrt):
    g = {b: marsrt.overlay_glyph(b) for b in range(-3, 260)}
    assert all(r.shape == (7,) and not (r & 0xE0).any() for r in g.values())  # only the low 5 bits
    assert not g[32].any()
    own = [g[b].tobytes() for b in range(33, 96)]
    assert all(np.frombuffer(r, np.uint8).any() for r in own) and len(set(own)) == 63
    for b in range(96, 127):
        assert g[b].tobytes() == g[b - 32].tobytes()
    for b in list(range(-3, 32)) + list(range(127, 260)):
        assert g[b].tobytes() == g[ord("?")].tobytes()
    assert np.array_equal(O.FONT[ord("a")], g[ord("A")]) and O.FONT.shape == (256, 7)
    assert [format(r, "05b") for r in g[ord("T")]] == ["11111", "00100", "00100", "00100", "00100", "00100", "00100"]  # bit 4 is the left column


# ---- layers and owners -----------------------------------------------------------------------------------------------------------------------
def test_owner_maps_against_the_per_pixel_rule():
    """the restatement's maps and the loop over the elements agree on every pixel of the smallest cases of the GPU file, at every configuration"""
    for what, c, layers, kw, flags, own in G.all_host_cases():
        if (c["W"], c["H"]) not in ((31, 17), (33, 45), (32, 18)):
            continue
        W, H = c["W"], c["H"]
        rgb = dict(c, fmt=O.RGB, frames=c["frames"][:, :W * H * 3] if c["fmt"] == O.RGB else np.zeros((c["F"], W * H * 3), dtype=np.uint8))
        out, st, infos = G.want_host(rgb, layers, kw, 0, own)
        o = O.Opts(layers=layers, no_key=G.NO_KEY, **kw)
        for f, info in enumerate(infos):
            src = rgb["frames"][f].reshape(H, W, 3).astype(np.int64)
            img = out[f].reshape(H, W, 3)
            n = 0
            for y in range(H):
                for x in range(W):
                    kind, col = O.pixel_np(x, y, W, H, info["elems"], info["marks"], o)
                    want = src[y, x] if kind is None else np.array(col) if kind == "opaque" else (src[y, x] * (256 - o.a) + np.array(col) * o.a + 128) >> 8
                    assert tuple(img[y, x]) == tuple(int(v) for v in want), (what, f, x, y, kind)
                    n += kind is not None
            assert n == st[f]["pixels"]


def test_priority_across_layers_and_lowest_index_within_one():
    mw = np.full((2, 12, 1), 0xFFFFFFFF, dtype=np.uint32)
    kp = np.zeros((2, 1), dtype=G.KPT)
    kp[0, 0], kp[1, 0] = (6.5, 6.5, 1.0), (7.5, 6.5, 1.0)
    pal = [(200, 0, 0), (0, 200, 0)]
    img, st, info = one(20, 12, [(6, 6, 8, 8, 0.9, 0), (8, 6, 8, 8, 0.8, 1)], layers=G.ALL, thickness=1, radius=1, scale=1, alpha=256, palette=pal,
                        mask_words=mw, mask_of_box=[0, 1], kpts=kp, texts=[b"", b""])
    # R0 = (2, 2, 10, 10), R1 = (4, 2, 12, 10); no labels.  (5, 5): inside both, tinted by the lower index; (4, 5): R1's outline over R0's tint;
    # (2, 5): R0's outline; the markers [5, 7] and [6, 8] x [5, 7]: keypoint 0 of both, palette[0], over outlines and tints
    assert tuple(img[4, 5]) == pal[0] and tuple(img[5, 4]) == pal[1] and tuple(img[5, 2]) == pal[0] and tuple(img[5, 10]) == pal[1]
    assert (img[5:8, 5:9] == pal[0]).all() and info["opaque_over_tint"] and st["markers"] == 2 and st["masked"] == 2
    assert info["visible"][O.MASKS][4, 5] and not info["visible"][O.MASKS][5, 4] and not info["visible"][O.BOXES][6, 6]


# ---- the GPU file's cases --------------------------------------------------------------------------------------------------------------------
def test_no_gpu_case_is_vacuous():
    n = 0
    for what, c, layers, kw, flags, own in G.all_host_cases():
        out, st, infos = G.want_host(c, layers, kw, flags, own)
        assert not O.not_vacuous(infos, layers, c["W"], c["H"]), what
        assert st["skipped"].sum() >= 2 and np.array_equal(out[-1], c["frames"][-1]) and st["pixels"][0] > 0, what
        if layers == G.ALL and not own:
            assert st["markers"].sum() >= 4 and st["masked"].sum() >= 2 and st["labels"].sum() == st["boxes"].sum(), what
        n += 1
    assert n == 9 * len(G.CONFIGS)
    for W, H, edge in ((66, 130, 32), (128, 66, 64), (257, 130, 128)):  # the first box and its mask span two mask words, two tiles
        c = G.host_case(0, W, H, O.NV12 if W % 2 == 0 else O.RGB)
        e = O.elements_np(c["boxes"][c["fo"] == 0], W, H, O.Opts(layers=G.ALL))[0]
        assert e[0]["rect"][0] < edge < e[0]["rect"][2] and c["mo"][0] == 0, (W, H)
