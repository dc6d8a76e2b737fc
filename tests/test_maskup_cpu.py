"""Instance masks in frame pixels without a device: mars_yolo_mask_taps against the big-integer tables of tests/maskupref.py, its refusals,
the restatement's literal loops against its array form, the consequence the header states (identity geometry: the prototype mask), an
independent pin of the blend against torch's bilinear interpolation where the tap fractions are exact, and the new records' layout."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import maskupref
import segref

F32 = np.float32
INC = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include")

# (out_n, in_n, n_content, pad, P)
NAMED_AXES = [
    (16, 64, 64, 0, 16), (20, 80, 80, 0, 20),       # identity: out = P
    (32, 64, 64, 0, 16), (64, 64, 64, 0, 16), (128, 64, 64, 0, 16),  # 2x, 4x, 8x
    (56, 64, 35, 14, 16), (43, 64, 35, 14, 16),     # a letterboxed axis: content 35 at pad 14 of 64
    (100, 64, 64, 0, 16), (77, 64, 64, 0, 16),
    (1, 64, 64, 0, 1), (1, 64, 3, 30, 16), (8192, 64, 64, 0, 16), (8192, 640, 360, 140, 160),
    (33, 64, 35, 14, 1), (5, 7, 7, 0, 1),           # P = 1: every tap is pixel 0
    (8192, 1 << 20, 1 << 20, 0, 8192), (8192, 1 << 20, 1, (1 << 20) - 1, 1 << 20),  # the largest terms
]


def _check_axis(marsrt, axis):
    ia, ib, w1 = marsrt.mask_taps(*axis)
    ra, rb, rw = maskupref.taps(*axis)
    assert ia.tolist() == ra and ib.tolist() == rb and w1.tolist() == rw, axis
    P = axis[4]
    assert all(0 <= a <= b <= min(a + 1, P - 1) for a, b in zip(ra, rb)) and all(x <= y for x, y in zip(ra, ra[1:])), axis


@pytest.mark.parametrize("axis", NAMED_AXES)
def test_taps_named_axes(marsrt, axis):
    _check_axis(marsrt, axis)


def test_taps_identity_is_the_pixel_itself():
    for P in (1, 16, 33):
        ia, ib, w1 = maskupref.taps(P, 4 * P, 4 * P, 0, P)
        assert ia == list(range(P)) and w1 == [0] * P and ib == [min(i + 1, P - 1) for i in range(P)]


def test_taps_hand_worked():
    """2x over 4 pixels: centres at -0.25, 0.25, 0.75, ... -> floors -1, 0, 0, 1, ...; fractions 0.75, 0.25 in 1/256"""
    ia, ib, w1 = maskupref.taps(8, 16, 16, 0, 4)
    assert ia == [0, 0, 0, 1, 1, 2, 2, 3] and ib == [0, 1, 1, 2, 2, 3, 3, 3] and w1 == [192, 64] * 4
    # content 2 at pad 1 of 4, P = 4, out 2: u = (2X + 1) * 2 * 4 / 16 + 1 - 0.5 = X + 1: pixels 1 and 2 exactly
    assert maskupref.taps(2, 4, 2, 1, 4) == ([1, 2], [2, 3], [0, 0])


def test_taps_random_axes(marsrt):
    rng = np.random.default_rng(2024)
    done = 0
    while done < 300:
        in_n = int(rng.integers(1, 2000))
        n_content = int(rng.integers(1, in_n + 1))
        pad = int(rng.integers(0, in_n - n_content + 1))
        P = int(rng.integers(1, 400))
        lo = -(-n_content * P // in_n)  # the smallest out_n that is no down-scale
        if lo > 1200:
            continue
        out_n = int(rng.integers(max(lo, 1), max(lo, 1) + 300))
        _check_axis(marsrt, (out_n, in_n, n_content, pad, P))
        done += 1


@pytest.mark.parametrize("axis", [
    (15, 64, 64, 0, 16),              # down-scaling by one pixel
    (34, 64, 35, 14, 64),             # ... of the letterboxed content: 34 * 64 < 35 * 64
    (0, 64, 64, 0, 16), (-1, 64, 64, 0, 16), (8193, 64, 64, 0, 16),
    (16, 0, 64, 0, 16), (16, 64, 0, 0, 16), (16, 64, 64, 0, 0), (16, 64, 64, -1, 16),
    (64, 64, 35, 30, 16),             # the content leaves the input
    (8192, (1 << 20) + 1, 64, 0, 16), (8192, 1 << 20, 64, 0, (1 << 20) + 1),
])
def test_taps_refusals(marsrt, axis):
    with pytest.raises(ValueError):
        maskupref.taps(*axis)
    with pytest.raises(ValueError):
        marsrt.mask_taps(*axis)


def test_taps_refuse_null_tables(marsrt):
    a = np.zeros(16, np.int32)
    L = marsrt.lib()
    assert L.mars_yolo_mask_taps(16, 64, 64, 0, 16, a.ctypes.data, a.ctypes.data, a.ctypes.data) == 0
    assert L.mars_yolo_mask_taps(16, 64, 64, 0, 16, None, a.ctypes.data, a.ctypes.data) == -1
    assert L.mars_yolo_mask_taps(16, 64, 64, 0, 16, a.ctypes.data, a.ctypes.data, None) == -1


GEOMS = [
    maskupref.identity(64, 64, 16, 16), maskupref.identity(64, 64, 64, 64), maskupref.identity(64, 48, 37, 29),
    maskupref.letterbox(100, 56, 64, 64), maskupref.letterbox(100, 56, 64, 64, 77, 43), maskupref.letterbox(56, 100, 64, 64),
]


def test_letterbox_geometry():
    assert maskupref.letterbox(100, 56, 64, 64) == (64, 64, 64, 35, 0, 14, 100, 56, 100, 56)
    assert maskupref.letterbox(56, 100, 64, 64, 30, 70) == (64, 64, 35, 64, 14, 0, 56, 100, 30, 70)
    assert maskupref.letterbox(1280, 720, 640, 640)[2:6] == (640, 360, 0, 140)


def test_array_form_equals_the_literal_loops():
    rng = np.random.default_rng(12)
    for k, g in enumerate(GEOMS):
        nm, ph, pw = ((1, 16, 16), (4, 12, 16), (33, 7, 9), (64, 16, 16), (32, 16, 16), (5, 16, 16))[k]
        p = rng.integers(-128, 128, (nm, ph, pw), dtype=np.int8)
        p[:, 1, 3] = 0
        some = 0
        for j in range(3):
            a = rng.integers(-128, 128, nm, dtype=np.int8)
            box = (rng.uniform(0.2, 0.8) * g.base_w, rng.uniform(0.2, 0.8) * g.base_h, rng.uniform(0.1, 1.2) * g.base_w, rng.uniform(0.1, 1.2) * g.base_h)
            lm = (0.0, 2.5, -1.0)[j]
            r0, w0 = maskupref.mask_literal(a, p, box, g, 0.01, lm)
            r1, w1 = maskupref.mask_array(a, p, box, g, 0.01, lm)
            assert r0 == r1 and np.array_equal(w0, w1), (g, j)
            assert w0.shape == (g.out_h, (g.out_w + 31) // 32)
            some += 0 < r0[4] < (r0[2] - r0[0]) * (r0[3] - r0[1])
        assert some, g


def test_identity_geometry_gives_the_prototype_mask():
    """out = PW x PH without a letterbox: w1 = 0, S = 65536 * dot, (float)S * (s * 2^-16) = (float)dot * s"""
    rng = np.random.default_rng(13)
    for nm, ph, pw in ((4, 5, 7), (32, 20, 20), (64, 40, 33)):
        p = rng.integers(-128, 128, (nm, ph, pw), dtype=np.int8)
        g = maskupref.identity(4 * pw, 4 * ph, pw, ph)
        for lm in (0.0, 0.7):
            a = rng.integers(-128, 128, nm, dtype=np.int8)
            box = (2.0 * pw, 2.0 * ph, 3.1 * pw, 2.9 * ph)
            assert maskupref.mask_array(a, p, box, g, 0.01, lm)[0] == segref.mask_array(a, p, box, 4 * pw, 4 * ph, 0.01, lm)[0]
            assert np.array_equal(maskupref.mask_array(a, p, box, g, 0.01, lm)[1], segref.mask_array(a, p, box, 4 * pw, 4 * ph, 0.01, lm)[1])


def test_extreme_value_and_strict_compare():
    """all bytes -128 at nm = 64: every dot is 2^20, S = 2^36 whatever the weights, exact in float32; the compare is strict"""
    p = np.full((64, 3, 5), -128, dtype=np.int8)
    a = np.full(64, -128, dtype=np.int8)
    g = maskupref.identity(20, 12, 20, 12)
    S = maskupref.blend(np.tensordot(a.astype(np.int64), p.astype(np.int64), axes=1), *maskupref.geom_taps(g, 3, 5))
    assert (S == 1 << 36).all()
    for lm, bit in ((0.0, 1), (1048575.5, 1), (1048576.0, 0)):
        (_, _, _, _, area), w = maskupref.mask_literal(a, p, (10, 6, 20, 12), g, 1.0, lm)
        assert area == 240 * bit and (w == 0xFFFFF * bit).all()


@pytest.mark.parametrize("k", [2, 4, 8])
def test_blend_is_torch_bilinear_where_the_fractions_are_exact(k):
    """identity letterbox, integer factor k: the tap fractions are multiples of 1 / (2k), exact in 1/256, and every product and sum below is
    exact in float64, so S / 65536 must be torch's align_corners=False bilinear interpolation of the dots, element for element"""
    import torch
    rng = np.random.default_rng(k)
    for ph, pw in ((5, 7), (16, 16), (1, 9)):
        dots = rng.integers(-(1 << 20), (1 << 20) + 1, (ph, pw), dtype=np.int64)
        g = maskupref.identity(4 * pw, 4 * ph, k * pw, k * ph)
        S = maskupref.blend(dots, *maskupref.geom_taps(g, ph, pw))
        want = torch.nn.functional.interpolate(torch.from_numpy(dots).double()[None, None], size=(k * ph, k * pw), mode="bilinear", align_corners=False)
        assert np.array_equal(S.astype(np.float64) / 65536.0, want[0, 0].numpy()), (k, ph, pw)


def test_record_and_options_layout(marsrt, tmp_path):
    N, G = marsrt.MaskNativeOpts, marsrt.MaskGeom
    got = [C.sizeof(N), C.sizeof(G)] + [getattr(N, f).offset for f, _ in N._fields_] + [getattr(G, f).offset for f, _ in G._fields_]
    assert got == [12, 40, 0, 4, 8] + list(range(0, 40, 4)) and tuple(marsrt.MASK_GEOM_FIELDS) == maskupref.Geom._fields
    src = tmp_path / "abi.c"
    src.write_text("""
#include <stddef.h>
#include <stdio.h>
#include "mars_hip.h"
#define O(f) offsetof(mars_hip_mask_native_opts_t, f)
#define Q(f) offsetof(mars_mask_geom_t, f)
int main(void) {
 printf("%zu %zu %zu %zu %zu ", sizeof(mars_hip_mask_native_opts_t), sizeof(mars_mask_geom_t), O(out_w), O(out_h), O(flags));
 printf("%zu %zu %zu %zu %zu %zu %zu %zu %zu %zu %d\\n", Q(in_w), Q(in_h), Q(nw), Q(nh), Q(px), Q(py), Q(base_w), Q(base_h), Q(out_w), Q(out_h),
        MARS_MASK_NATIVE_MAX);
 return 0;
}
""")
    exe = tmp_path / "abi"
    subprocess.check_call(["gcc", "-std=c11", "-Wall", "-Werror", "-I", INC, str(src), "-o", str(exe)])
    assert [int(v) for v in subprocess.check_output([str(exe)]).split()] == got + [marsrt.MASK_NATIVE_MAX]
    o = marsrt.mask_native_opts(77, 43)
    assert (o.out_w, o.out_h, o.flags) == (77, 43, 0)
    g = marsrt.mask_geom(64, 64, 77, 43, nh=35, py=14, base_w=100, base_h=56)
    assert tuple(getattr(g, f) for f in marsrt.MASK_GEOM_FIELDS) == maskupref.letterbox(100, 56, 64, 64, 77, 43)


def test_host_form_refuses_without_touching_a_device(marsrt):
    """the range checks and the tap tables come before the device: these answer -1 on a machine without one, and n = 0 answers 0"""
    proto = np.zeros((4, 16, 16), np.int8)
    none = np.zeros(0, marsrt.DET_DTYPE)
    recs, words = marsrt.masks_native(np.zeros((0, 4), np.int8), proto, none, marsrt.mask_geom(64, 64, 64, 64), 0.01)
    assert recs.shape == (0,) and words.shape == (0, 64, 2)
    for g in (marsrt.mask_geom(64, 64, 15, 16), marsrt.mask_geom(64, 64, 16, 15), marsrt.mask_geom(64, 64, 8193, 16), marsrt.mask_geom(64, 64, 16, 0),
              marsrt.mask_geom(64, 64, 16, 16, base_w=0), marsrt.mask_geom(64, 64, 16, 16, nw=65)):
        with pytest.raises(ValueError):
            marsrt.masks_native(np.zeros((0, 4), np.int8), proto, none, g, 0.01)
    for kw in (dict(s=0.0), dict(s=float("nan")), dict(logit_min=float("inf"))):
        with pytest.raises(ValueError):
            marsrt.masks_native(np.zeros((0, 4), np.int8), proto, none, marsrt.mask_geom(64, 64, 64, 64), kw.get("s", 0.01), kw.get("logit_min", 0.0))
