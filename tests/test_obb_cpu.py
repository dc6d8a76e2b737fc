"""Oriented boxes without a device: the numpy restatement of include/mars_hip.h "Oriented boxes" (tests/obbref.py) on hand-worked cases, the
records' and options' layout, the synthetic writer's obb head, mars_yolo_obb_corners (pure host code), and the accuracy of the float32
decision against Ultralytics' ProbIoU formula in float64."""
import ctypes as C
import os
import struct
import subprocess

import numpy as np
import pytest

import marsfile
import obbref

F32 = np.float32
INC = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include")


def r32(x):
    """a Python float rounded to float32 (as a Python float): the one rounding of a float32 operation done in double"""
    return struct.unpack("<f", struct.pack("<f", x))[0]


def cov_of(w, h, angle):
    cs, sn = obbref.cosf(F32(angle)), obbref.sinf(F32(angle))
    return obbref.covariance(F32(w), F32(h), cs, sn)


def rel(b1, b2, T):
    """(x, y, w, h, angle) of two boxes -> does the first suppress the second"""
    return bool(obbref.suppresses((b1[0], b1[1]) + cov_of(*b1[2:]), (b2[0], b2[1]) + cov_of(*b2[2:]), T))


def test_identical_boxes_suppress_each_other_for_every_threshold():
    """dx = dy = 0: t1 = t2 = 0 and expf(-0) = 1; den = 4 d up to rounding, so X = 1 up to a few ulp, and E < 1 for T < 1"""
    for box in ((10, 20, 30, 8, 0.3), (0, 0, 2, 2, -0.7), (100.5, 7.25, 60, 2, 2.3), (5, 5, 3, 47, 1.5707964)):
        for T in (0.001, 0.01, 0.1, 0.3, 0.45, 0.5, 0.7, 0.9, 0.99, 0.999):
            assert rel(box, box, T), (box, T)


def test_unit_squares_far_apart_do_not():
    for T in (0.001, 0.3, 0.45, 0.7):
        assert not rel((0, 0, 1, 1, 0.0), (10, 0, 1, 1, 0.0), T)
        assert not rel((0, 0, 1, 1, 0.4), (3, 4, 1, 1, 1.1), T)
    # ... and touching unit squares overlap a little in ProbIoU's Gaussian sense: suppressed at a low threshold only
    assert rel((0, 0, 1, 1, 0.0), (0.5, 0, 1, 1, 0.0), 0.3) and not rel((0, 0, 1, 1, 0.0), (0.5, 0, 1, 1, 0.0), 0.7)


def test_turn_by_pi_gives_the_same_covariance_to_the_bit():
    """cos and sin both change sign: every product of two of them is unchanged"""
    rng = np.random.default_rng(3)
    w, h = rng.uniform(2, 60, 200).astype(F32), rng.uniform(2, 60, 200).astype(F32)
    ang = rng.uniform(-np.pi / 4, 3 * np.pi / 4, 200).astype(F32)
    cs, sn = obbref.cosf(ang), obbref.sinf(ang)
    one, other = obbref.covariance(w, h, cs, sn), obbref.covariance(w, h, -cs, -sn)
    for u, v in zip(one, other):
        assert u.tobytes() == v.tobytes()


def test_a_squares_covariance_is_angle_free_up_to_rounding():
    """w = h: A = B, so c = 0 exactly and a = b = A (cs^2 + sn^2), within a few ulp of A"""
    for side in (2.0, 7.3, 59.9):
        A = F32(side) * F32(side) / F32(12.0)
        for ang in np.linspace(-0.78, 2.35, 23):
            a, b, c, d = cov_of(side, side, ang)
            assert c == 0.0
            assert abs(float(a) - float(A)) <= 4 * float(np.spacing(A)) and abs(float(b) - float(A)) <= 4 * float(np.spacing(A))
            assert abs(float(d) - float(A) ** 2) <= 1e-6 * float(A) ** 2


def test_hand_worked_decode():
    """One cell (gx 2, gy 1) of a 3-wide grid of stride 8; R = 4; box scale 1.0, so that E[0] = 1 and E[255] = expf(-255) = 0: a side whose
    bins hold 127 or -128 has dist = (sum of the indices at 127) / (their number).
      left:   bins {0, 1, 3} -> 4 / 3 = 1.3333334 (rounded up);   top:    bins {1, 2, 3} -> 6 / 3 = 2
      right:  bins {0, 2, 3} -> 5 / 3 = 1.6666666 (rounded down); bottom: bins {0, 1}    -> 1 / 2 = 0.5
    class bytes (-3, 25, 25) at scale 0.07: the first of the largest wins, class 1, conf = 1 / (1 + expf(-1.75)) = 0.85195273
    angle byte 37 at scale 0.03: sg = 1 / (1 + expf(-1.11)) = 0.75212914; ang = (sg - 0.25) * 3.14159265f = 0.50212914 * 3.1415927
      = 1.5774851; cs = cosf(ang) = -0.006688708, sn = sinf(ang) = 0.99997765
    xf = (1.6666666 - 1.3333334) * 0.5 = 0.16666663 (the difference is exact, 0.33333325);  yf = (0.5 - 2) * 0.5 = -0.75
    cx = ((xf cs - yf sn) + 2.5) * 8:  xf cs = -0.0011147845, yf sn = -0.74998325, difference 0.74886847, + 2.5 = 3.2488685, * 8 = 25.990948
    cy = ((xf sn + yf cs) + 1.5) * 8:  xf sn = 0.1666629, yf cs = 0.005016531, sum 0.17167944, + 1.5 = 1.6716795, * 8 = 13.373436
    w = (1.3333334 + 1.6666666) * 8 = 24 (the sum rounds to 3);  h = (2 + 0.5) * 8 = 20
    The test redoes every step in double with one rounding to float32 after each, and compares bits."""
    R, W = 4, 3
    box = np.full((4 * R, 2, W), -128, dtype=np.int8)
    for side, bins in enumerate(((0, 1, 3), (1, 2, 3), (0, 2, 3), (0, 1))):
        for i in bins:
            box[side * R + i, 1, 2] = 127
    cls = np.full((3, 2, W), -128, dtype=np.int8)
    cls[:, 1, 2] = (-3, 25, 25)
    ang = np.zeros((2, W), dtype=np.int8)
    ang[1, 2] = 37
    rec, cs, sn, raw = obbref.decode([(box, cls, ang, 1.0, 0.07, 0.03, 8)], conf=0.25)
    assert raw == 1 and len(rec) == 1 and rec["pred"][0] == 5 and rec["cls"][0] == 1
    dl, dt, dr, db = r32(4 / 3), 2.0, r32(5 / 3), 0.5
    sg = float(obbref.tables(0.03)[0][37 + 128])
    a = r32(r32(sg - 0.25) * float(obbref.PI))
    c, s = float(obbref.cosf(F32(a))), float(obbref.sinf(F32(a)))
    xf, yf = r32(r32(dr - dl) * 0.5), r32(r32(db - dt) * 0.5)
    cx = r32(r32(r32(r32(xf * c) - r32(yf * s)) + 2.5) * 8.0)
    cy = r32(r32(r32(r32(xf * s) + r32(yf * c)) + 1.5) * 8.0)
    want = (cx, cy, r32(r32(dl + dr) * 8.0), r32(r32(dt + db) * 8.0), float(obbref.tables(0.07)[0][25 + 128]), a)
    got = tuple(float(rec[k][0]) for k in ("x", "y", "w", "h", "conf", "angle"))
    assert got == want, (got, want)
    assert (float(cs[0]), float(sn[0])) == (c, s)
    # the figures of the docstring
    assert [float(F32(v)) for v in got] == [float(F32(v)) for v in (25.990948, 13.373436, 24.0, 20.0, 0.85195273, 1.5774851)]
    assert (xf, yf) == (float(F32(0.16666663)), -0.75) and (F32(c), F32(s)) == (F32(-0.006688708), F32(0.99997765))
    # the angle rule's range: [-pi / 4, 3 pi / 4)
    _, at, ct, st = obbref.tables(0.5)
    assert at[0] == F32(F32(-0.25) * obbref.PI) and at[255] == F32(F32(0.75) * obbref.PI) and at[128] == F32(F32(0.25) * obbref.PI)
    assert np.all(np.diff(at.astype(np.float64)) >= 0)


def test_order_greedy_and_letterbox():
    b = np.zeros(5, dtype=obbref.OBB_DTYPE)
    # 0 and 1: the same place, equal confidence (the lower index wins); 2: the same place, higher confidence, another class; 3: elsewhere;
    # 4: the same place and class as 2, lower confidence
    b["x"], b["y"], b["w"], b["h"] = (10, 10, 10, 50, 10), (10, 10, 10, 10, 10), 8, 4
    b["conf"], b["cls"], b["angle"], b["pred"] = (0.5, 0.5, 0.9, 0.5, 0.6), (0, 0, 1, 0, 1), 0.3, (7, 8, 9, 10, 11)
    assert obbref.nms_list(b)["pred"].tolist() == [9, 7, 10]
    assert obbref.nms_list(b, agnostic=True)["pred"].tolist() == [9, 10]
    # a 64 x 64 input fed from 1280 x 720: x' = x * 20, y' = (y - 14) * 20, w and h both * 20
    m = obbref.mapped(b[:1], (1280, 720), (64, 64))
    assert (m["x"][0], m["y"][0], m["w"][0], m["h"][0], m["angle"][0]) == (200.0, -80.0, 160.0, 80.0, b["angle"][0])
    # the enclosing rectangle of an upright box is the box; of one turned by a quarter, the box with its sides swapped (up to cosf(pi / 2))
    e = obbref.enclosing(b[:1], [1.0], [0.0])
    assert (e["w"][0], e["h"][0], e["x"][0], e["conf"][0], e["cls"][0]) == (8.0, 4.0, 10.0, 0.5, 0)
    e = obbref.enclosing(b[:1], [0.0], [-1.0])
    assert (e["w"][0], e["h"][0]) == (4.0, 8.0)


def test_record_and_options_layout(marsrt, tmp_path):
    assert marsrt.OBB_DTYPE == obbref.OBB_DTYPE and marsrt.DET_DTYPE == obbref.DET_DTYPE
    S = marsrt.ObbOpts
    got = [C.sizeof(S)] + [getattr(S, f).offset for f, _ in S._fields_]
    assert got == [36, 0, 16, 32]
    src = tmp_path / "abi.c"
    src.write_text("""
#include <stddef.h>
#include <stdio.h>
#include "mars_hip.h"
int main(void) {
 printf("%zu %zu %zu %zu %zu %zu %zu %zu %zu %u %d\\n", sizeof(mars_obb_t), offsetof(mars_obb_t, conf), offsetof(mars_obb_t, cls),
        offsetof(mars_obb_t, angle), offsetof(mars_obb_t, pred), sizeof(mars_hip_obb_opts_t), offsetof(mars_hip_obb_opts_t, angle_tensors),
        offsetof(mars_hip_obb_opts_t, angle_scales), offsetof(mars_hip_obb_opts_t, flags), MARS_OBB_AGNOSTIC, MARS_SYNTH_HEAD_OBB);
 return 0;
}
""")
    exe = tmp_path / "abi"
    subprocess.check_call(["gcc", "-std=c11", "-Wall", "-Werror", "-I", INC, str(src), "-o", str(exe)])
    d = marsrt.OBB_DTYPE
    want = [d.itemsize] + [d.fields[k][1] for k in ("conf", "cls", "angle", "pred")] + got + [marsrt.OBB_AGNOSTIC, marsrt.SYNTH_HEADS["obb"]]
    assert [int(v) for v in subprocess.check_output([str(exe)]).split()] == want == [32, 16, 20, 24, 28, 36, 0, 16, 32, 1, 4]
    o = marsrt.obb_opts([5, 6, 7], angle_scales=0.5, agnostic=True)
    assert list(o.angle_tensors) == [5, 6, 7, 0] and list(o.angle_scales) == [0.5] * 4 and o.flags == 1
    o = marsrt.obb_opts([1, 2, 3], angle_scales=[0.5, 0.25, 0.125], flags=6)
    assert list(o.angle_scales) == [0.5, 0.25, 0.125, 0.0] and o.flags == 6
    for n in ("mars_hip_detect_obb_device", "mars_hip_obb_results", "mars_hip_detect_obb", "mars_hip_obb_ms", "mars_yolo_obb_nms", "mars_yolo_obb_corners"):
        assert n in marsrt.EXPORTS["mars_hip.h"] and getattr(marsrt.lib(), n)


@pytest.mark.parametrize("nchw", [False, True])
@pytest.mark.parametrize("hw", [64, 160])
def test_synth_obb_head(marsrt, hw, nchw):
    """the DFL twin plus three angle branches behind it: three graph outputs, the angle tensors internal and found by name"""
    d = marsrt.synth_model(width_x16=4, input_hw=hw, nchw_int8=nchw, seed=1, head="obb")
    hdr, tensors, layers = marsfile.parse(d)
    an = marsrt.obb_twin_tensors(d)
    assert len(hdr["outputs"]) == 3 and len(set(an)) == 3 and not set(an) & set(hdr["outputs"])

    def chw(t):
        s = tensors[t]["shape"]
        return (s[1], s[2], s[3]) if nchw else (s[3], s[1], s[2])
    heads, nc, reg_max = marsrt.find_yolo_dfl_heads(d)
    assert (nc, reg_max) == (80, 16) and [s for _, _, s in heads] == [8, 16, 32]
    for k, (b, c, s) in enumerate(heads):
        g = hw // s
        assert chw(hdr["outputs"][k]) == (144, g, g) and chw(b) == (64, g, g) and chw(c) == (80, g, g)
        assert chw(an[k]) == (1, g, g) and tensors[an[k]]["dtype"] == marsfile.I8
        writers = [l for l in layers if an[k] in l["outs"]]
        readers = [l for l in layers if an[k] in l["ins"]]
        assert len(writers) == 1 and writers[0]["type"] == marsfile.CONV2D and [l["type"] for l in readers] == [marsfile.RESHAPE]
    # the trunk and the DFL branches are the dfl twin's, weights included: the obb file only adds tensors and layers behind them
    dd = marsrt.synth_model(width_x16=4, input_hw=hw, nchw_int8=nchw, seed=1, head="dfl")
    hd, td, ld = marsfile.parse(dd)
    assert [t["shape"] for t in tensors[:len(td)]] == [t["shape"] for t in td] and hdr["outputs"] == hd["outputs"]
    assert [(l["type"], l["ins"], l["outs"]) for l in layers[:len(ld)]] == [(l["type"], l["ins"], l["outs"]) for l in ld]
    for bad in (dict(float32=True), dict(tiny=True)):
        with pytest.raises(ValueError):
            marsrt.synth_model(width_x16=4, input_hw=64, head="obb", **bad)
    with pytest.raises(KeyError):
        marsrt.obb_twin_tensors(dd)
    assert marsrt.describe_plan(d)  # the loader and the planner take it


def test_corners_against_the_restatement(marsrt):
    rng = np.random.default_rng(11)
    b = np.zeros(64, dtype=marsrt.OBB_DTYPE)
    b["x"], b["y"] = rng.uniform(-50, 700, 64), rng.uniform(-50, 700, 64)
    b["w"], b["h"] = rng.uniform(0, 300, 64), rng.uniform(0, 300, 64)
    b["angle"] = rng.uniform(-np.pi / 4, 3 * np.pi / 4, 64)
    b["angle"][:3] = (0.0, F32(np.pi / 2), F32(-np.pi / 4))
    got = marsrt.obb_corners(b)
    assert got.shape == (64, 4, 2)
    for i in range(64):
        assert got[i].tobytes() == obbref.corners(b[i]).tobytes(), i
    # an upright 4 x 2 box at (10, 20): corners in the order (-, -), (+, -), (+, +), (-, +) of its own axes
    assert got[0].tolist() == [[b["x"][0] - b["w"][0] / 2, b["y"][0] - b["h"][0] / 2], [b["x"][0] + b["w"][0] / 2, b["y"][0] - b["h"][0] / 2],
                               [b["x"][0] + b["w"][0] / 2, b["y"][0] + b["h"][0] / 2], [b["x"][0] - b["w"][0] / 2, b["y"][0] + b["h"][0] / 2]]
    # the corners' mean is the centre and their spans fit the enclosing rectangle
    e = obbref.enclosing(b, obbref.cosf(b["angle"]), obbref.sinf(b["angle"]))
    assert np.allclose(got.mean(axis=1), np.stack([b["x"], b["y"]], axis=1), atol=1e-3)
    assert np.allclose(np.ptp(got[:, :, 0], axis=1), e["w"], atol=1e-3) and np.allclose(np.ptp(got[:, :, 1], axis=1), e["h"], atol=1e-3)


def probiou64(b1, b2):
    """Ultralytics' probiou in float64 with its eps and clamps; b = (x, y, w, h, angle) arrays"""
    eps = 1e-7

    def cov(w, h, a):
        A, B, c, s = w * w / 12.0, h * h / 12.0, np.cos(a), np.sin(a)
        return A * c * c + B * s * s, A * s * s + B * c * c, (A - B) * c * s
    (x1, y1), (x2, y2) = b1[:2], b2[:2]
    a1, b1_, c1 = cov(*b1[2:])
    a2, b2_, c2 = cov(*b2[2:])
    den = (a1 + a2) * (b1_ + b2_) - (c1 + c2) ** 2
    t1 = ((a1 + a2) * (y1 - y2) ** 2 + (b1_ + b2_) * (x1 - x2) ** 2) / (den + eps) * 0.25
    t2 = ((c1 + c2) * (x2 - x1) * (y1 - y2)) / (den + eps) * 0.5
    t3 = np.log(den / (4 * np.sqrt(np.clip(a1 * b1_ - c1 ** 2, 0, None) * np.clip(a2 * b2_ - c2 ** 2, 0, None)) + eps) + eps) * 0.5
    bd = np.clip(t1 + t2 + t3, eps, 100.0)
    return 1 - np.sqrt(1 - np.exp(-bd) + eps)


def test_decision_against_float64_probiou():
    """400 000 random pairs, boxes of 2 - 60 px, the second a perturbation of the first.  The float64 formula sees the float64 boxes, the
    restatement their float32 roundings (cos and sin: float64's rounded to float32) and the host libm's expf.  Pairs with
    |iou64 - T| < 1e-3 are left out -- at most 1 % of the pairs -- and every other pair must agree, at T = 0.3, 0.45, 0.7.
    Measured with numpy's float32 exp in expf's place: 0 disagreements, 0.14 % / 0.21 % / 0.50 % of the pairs inside the band."""
    rng = np.random.default_rng(1)
    N = 400000
    x1, y1, w1, h1 = rng.uniform(0, 64, N), rng.uniform(0, 64, N), rng.uniform(2, 60, N), rng.uniform(2, 60, N)
    a1 = rng.uniform(-np.pi / 4, 3 * np.pi / 4, N)
    x2, y2 = x1 + rng.normal(0, 6, N), y1 + rng.normal(0, 6, N)
    w2, h2, a2 = w1 * rng.uniform(0.6, 1.6, N), h1 * rng.uniform(0.6, 1.6, N), a1 + rng.normal(0, 0.4, N)
    iou = probiou64((x1, y1, w1, h1, a1), (x2, y2, w2, h2, a2))
    c1 = obbref.covariance(w1.astype(F32), h1.astype(F32), np.cos(a1).astype(F32), np.sin(a1).astype(F32))
    c2 = obbref.covariance(w2.astype(F32), h2.astype(F32), np.cos(a2).astype(F32), np.sin(a2).astype(F32))
    orig = obbref.expf
    cache = {}

    def expf_once(v):  # the exponent does not depend on T: libm is asked once per pair
        key = v.tobytes()
        if key not in cache:
            cache.clear()
            cache[key] = orig(v)
        return cache[key]
    obbref.expf = expf_once
    try:
        for T in (0.3, 0.45, 0.7):
            got = obbref.suppresses((x1.astype(F32), y1.astype(F32)) + c1, (x2.astype(F32), y2.astype(F32)) + c2, T)
            want = iou > T
            band = np.abs(iou - T) < 1e-3
            bad = (got != want) & ~band
            print("T %.2f: suppressed %.4f, inside the band %.4f %%, disagreements outside it %d" % (T, want.mean(), 100 * band.mean(), int(bad.sum())))
            assert band.mean() <= 0.01, (T, band.mean())
            assert not bad.any(), (T, int(bad.sum()), np.abs(iou - T)[bad].max())
    finally:
        obbref.expf = orig
