"""Aligned crops (include/mars_hip.h, "Aligned crops"), the part that needs no GPU: the numpy restatement (tests/alignref.py) on cases worked
out by hand, the host fit mars_yolo_align_fit against it bit for bit, the accuracy of the float32 fit, exports, layouts and the refusals that
come before any device work."""
import ctypes as C
import os
import subprocess

import numpy as np

import alignref
from alignref import FIT_KEYS, align_crop_np, align_fit_np, fit_tuple, geom_of, kpts
from conftest import lcg_frame
from rotref import rot_sample_np

F = np.float32
NEW = ["mars_yolo_align_fit", "mars_yolo_align_template_face5", "mars_yolo_crop_aligned", "mars_hip_crop_pose_device", "mars_hip_crop_pose",
       "mars_hip_align_results"]
FACE5 = [(38.2946, 51.6963), (73.5318, 51.5014), (56.0252, 71.7366), (41.5493, 92.3655), (70.7299, 92.2041)]  # the public ArcFace positions
W, H, TW, TH = 98, 62, 32, 24
QUAD = np.array([(8.25, 6.5), (24.75, 6.5), (10.0, 18.25), (22.5, 17.75)])  # multiples of 1 / 4: every sum below is exact in float32
NAN, INF = float("nan"), float("inf")


def uniforms(seed, n):
    """n numbers of [0, 1) from the suite's LCG, three bytes each"""
    b = lcg_frame(seed, 3 * n).astype(np.uint8).astype(np.float64).reshape(n, 3)
    return (b[:, 0] * 65536 + b[:, 1] * 256 + b[:, 2]) / 16777216.0


def lib_fit(marsrt, kp, tmpl, tw, th, W, H, use=0, min_vis=0.0, expand=0.0, min_size=0):
    """mars_yolo_align_fit -> (kept, the eight integers, the rectangle)"""
    kept, fit, rect = marsrt.align_fit(kp, marsrt.align_opts(tmpl, use, min_vis), marsrt.roi_opts(W, H, expand=expand, min_size=min_size), tw, th)
    return kept, tuple(int(fit[k]) for k in FIT_KEYS), rect


# ---- the two consequences and a fit by hand --------------------------------------------------------------------------------------------
def test_integer_shift_is_an_exact_copy(marsrt):
    """kpt = template + (40, 20): a = 1, b = 0, the centre (56, 32), no fraction anywhere: the crop is frame[20:44, 40:72] - 128"""
    img = lcg_frame(0xA11601, W * H * 3).astype(np.uint8).reshape(H, W, 3)
    kp = kpts(QUAD + (40, 20))
    fit, rect, why = align_fit_np(kp, QUAD, TW, TH, W, H)
    assert why is None and fit["abc"] == (1.0, 0.0, 56.0, 32.0)
    assert fit_tuple(fit) == (int(55.5 * 65536), int(31.5 * 65536), 32768, 0, 0, 32768, 15, 4) and rect == (40, 20, 72, 44)
    got, outside = rot_sample_np(img, geom_of(fit, TW, TH))
    assert outside == 0 and np.array_equal(got, (img[20:44, 40:72].astype(np.int16) - 128).astype(np.int8))
    assert lib_fit(marsrt, kp, QUAD, TW, TH, W, H) == (True, fit_tuple(fit), rect)
    assert np.array_equal(align_crop_np(img, kp, QUAD, TW, TH), got.reshape(-1))


def test_quarter_turn_is_an_exact_transposed_copy(marsrt):
    """the template turned a quarter turn about (50, 30): (du, dv) -> (-dv, du), a = 0, b = 1, Ux = 0, Uy = 32768: output (row j, column i)
    is frame[14 + i][61 - j] -- column i walks down the frame, row j walks left"""
    img = lcg_frame(0xA11602, W * H * 3).astype(np.uint8).reshape(H, W, 3)
    kp = kpts(np.stack([50 - (QUAD[:, 1] - TH / 2), 30 + (QUAD[:, 0] - TW / 2)], axis=1))
    fit, rect, why = align_fit_np(kp, QUAD, TW, TH, W, H)
    assert why is None and fit["abc"] == (0.0, 1.0, 50.0, 30.0)
    assert fit_tuple(fit) == (int(49.5 * 65536), int(29.5 * 65536), 0, 32768, -32768, 0, 15, 4) and rect == (38, 14, 62, 46)
    got, outside = rot_sample_np(img, geom_of(fit, TW, TH))
    want = (img[14:46, 38:62][:, ::-1].transpose(1, 0, 2).astype(np.int16) - 128).astype(np.int8)
    assert outside == 0 and got.shape == (TH, TW, 3) and np.array_equal(got, want)
    assert lib_fit(marsrt, kp, QUAD, TW, TH, W, H) == (True, fit_tuple(fit), rect)


def test_fit_worked_by_hand(marsrt):
    """template (2, 4), (6, 4) in a 10 x 6 target, keypoints (10, 10), (13, 14).  qm = (4, 4), pm = (11.5, 12); dq = (-+2, 0), dp = (-+1.5, -+2):
    A = 3 + 3 = 6, B = 4 + 4 = 8, D = 8, so a = 0.75, b = 1.  ux = 5 - 4 = 1, uy = 3 - 4 = -1: cx = 11.5 + (0.75 + 1) = 13.25,
    cy = 12 + (1 - 0.75) = 12.25.  s = sqrt(0.5625 + 1) = 1.25, we = 12.5, he = 7.5; ha = 0.375, hb = 0.5.  ca = 0.75 / 1.25 and sa = 1 / 1.25
    round to the float32 next to 0.6 and 0.8; 12.5 ca = 7.5 + 2^-21, 7.5 sa = 6 after rounding, their sum ties back to 13.5: ex = 6.75, and
    likewise ey = (10 + 4.5) / 2 = 7.25: the rectangle is [6.5, 20] x [5, 19.5] -> (6, 5, 20, 20)"""
    tmpl, kp = [(2, 4), (6, 4)], kpts([(10, 10), (13, 14)])
    fit, rect, why = align_fit_np(kp, tmpl, 10, 6, W, H)
    assert why is None and fit["abc"] == (0.75, 1.0, 13.25, 12.25)
    assert fit_tuple(fit) == (835584, 770048, 24576, 32768, -32768, 24576, 3, 2) and rect == (6, 5, 20, 20)
    assert lib_fit(marsrt, kp, tmpl, 10, 6, W, H) == (True, fit_tuple(fit), rect)
    # expand scales the crop about its centre: X0, Y0 stay, U and V grow
    fit2, rect2, _ = align_fit_np(kp, tmpl, 10, 6, W, H, expand=2.0)
    assert fit_tuple(fit2) == (835584, 770048, 49152, 65536, -65536, 49152, 3, 2) and rect2 == (0, 0, 27, 27)
    assert lib_fit(marsrt, kp, tmpl, 10, 6, W, H, expand=2.0) == (True, fit_tuple(fit2), rect2)


# ---- the host fit against the restatement ------------------------------------------------------------------------------------------------
FAMILIES = ["plain", "plain", "plain", "plain", "tiny", "huge", "off_frame", "coincident", "not_finite", "few"]
N_CASES = 2400


def seeded_case(i, u):
    """case i from ten uniforms + per-point uniforms -> dict(kp, tmpl, tw, th, W, H, use, min_vis, expand, min_size)"""
    K = (2, 5, 17, 32)[i % 4]
    tw, th = [(112, 112), (32, 24), (64, 96)][(i // 4) % 3]
    fw, fh = [(3840, 2160), (1280, 720), (98, 62), (640, 360)][(i // 12) % 4]
    fam = FAMILIES[(i // 7) % len(FAMILIES)]
    scale = 0.05 * (16 / 0.05) ** u[0]
    if fam == "tiny":
        scale = 0.01 + 0.03 * u[0]
    if fam == "huge":
        scale = 40000.0 / min(tw, th) * (1 + u[0])
    ang = 2 * np.pi * u[1]
    cx, cy = u[2] * fw, u[3] * fh
    if fam == "off_frame":
        cx, cy = [(-1 - 50 * u[2], cy), (fw + 1 + 50 * u[2], cy), (cx, -1 - 50 * u[3]), (cx, fh + 1 + 50 * u[3])][i % 4]
    pts = u[10:10 + 3 * K].reshape(K, 3)
    tmpl = np.stack([pts[:, 0] * tw, pts[:, 1] * th], axis=1).astype(F)
    use = 0 if u[4] < 0.5 else int(u[5] * (1 << K)) & ((1 << K) - 1)
    if fam == "few":
        use = 1 << int(u[5] * K)
    if fam == "coincident":
        tmpl[1] = tmpl[0]
        use = 3
    min_vis = (0.0, 0.0, 0.3, 0.6)[int(u[6] * 4)] if fam in ("plain", "few") else 0.0
    d = tmpl.astype(np.float64) - (tw / 2, th / 2)
    c, s = np.cos(ang) * scale, np.sin(ang) * scale
    xy = np.stack([cx + c * d[:, 0] - s * d[:, 1], cy + s * d[:, 0] + c * d[:, 1]], axis=1) + (pts[:, 2:3] - 0.5) * 0.5 * min(scale, 4)
    kp = kpts(xy, v=u[10 + 3 * K:10 + 4 * K])
    if fam == "coincident":
        kp["v"] = 1.0
    if fam == "not_finite":
        j = int(u[7] * K)
        kp[j][("x", "y", "v")[i % 3]] = (NAN, INF, -INF)[(i // 3) % 3]
        if i % 3 == 2 and (i // 3) % 3 == 2:  # v = -inf never participates: make it x
            kp[j]["v"], kp[j]["x"] = 1.0, -INF
    return dict(kp=kp, tmpl=tmpl, tw=tw, th=th, W=fw, H=fh, use=use, min_vis=min_vis, expand=(0.0, 1.25)[i % 2], min_size=0)


def test_host_fit_equals_the_restatement(marsrt):
    """mars_yolo_align_fit against alignref, all eight integers and the rectangle, over N_CASES seeded cases; every skip reason and the kept
    case must occur, so that nothing is left out silently"""
    per = 10 + 4 * 32
    u = uniforms(0xA116F17, N_CASES * per).reshape(N_CASES, per)
    counts = {}
    for i in range(N_CASES):
        c = seeded_case(i, u[i])
        fit, rect, why = align_fit_np(**c)
        got = lib_fit(marsrt, **c)
        assert got == (why is None, fit_tuple(fit), rect), (i, why, got, fit_tuple(fit), rect)
        counts[why] = counts.get(why, 0) + 1
    for why in (None, alignref.FEW, alignref.NOT_FINITE, alignref.DEGENERATE, alignref.SMALL, alignref.LARGE, alignref.OFF_FRAME):
        assert counts.get(why, 0) > 0, (why, counts)
    assert counts[None] > N_CASES // 4, counts
    assert sum(counts.values()) == N_CASES


def test_nan_outside_the_participating_set_changes_nothing(marsrt):
    u = uniforms(0xA116AA, 40 * 150).reshape(40, 150)
    n = 0
    plain5 = [k for k in range(4000) if k % 4 == 1 and FAMILIES[(k // 7) % len(FAMILIES)] == "plain"][:40]
    for i in range(40):
        c = seeded_case(plain5[i], u[i])  # K = 5, family "plain"
        c["kp"]["v"][:] = 1.0
        c["use"], c["min_vis"] = 0b01111, 0.5
        c["kp"][2]["v"] = 0.25  # masked in, but not visible enough
        zeroed = dict(c, kp=c["kp"].copy())
        for j, field, val in [(4, "x", NAN), (4, "y", INF), (4, "v", NAN), (2, "x", NAN), (2, "y", -INF)]:
            c["kp"][j][field] = val
            zeroed["kp"][j][field] = 0.0
        zeroed["kp"][2]["v"] = 0.25
        a, b = align_fit_np(**c), align_fit_np(**zeroed)
        assert fit_tuple(a[0]) == fit_tuple(b[0]) and a[1:] == b[1:]
        assert lib_fit(marsrt, **c) == lib_fit(marsrt, **zeroed) == (a[2] is None, fit_tuple(a[0]), a[1])
        if a[2] is None:
            assert a[0]["used"] == 0b01011 and a[0]["n_used"] == 3
            n += 1
    assert n >= 20
    # a NaN visibility does not pass min_vis: the point does not participate, the box is not skipped for it
    kp = kpts(QUAD + (40, 20))
    kp[3]["v"], kp[3]["x"] = NAN, NAN
    fit, _, why = align_fit_np(kp, QUAD, TW, TH, W, H)
    assert why is None and fit["used"] == 7 and lib_fit(marsrt, kp, QUAD, TW, TH, W, H)[1] == fit_tuple(fit)


# ---- accuracy ------------------------------------------------------------------------------------------------------------------------------
def fit64(kp, tmpl, tw, th):
    q, p = tmpl.astype(np.float64), np.stack([kp["x"], kp["y"]], axis=1).astype(np.float64)
    dq, dp = q - q.mean(0), p - p.mean(0)
    D = (dq * dq).sum()
    a, b = (dq * dp).sum() / D, (dq[:, 0] * dp[:, 1] - dq[:, 1] * dp[:, 0]).sum() / D
    ux, uy = tw * 0.5 - q.mean(0)[0], th * 0.5 - q.mean(0)[1]
    return a, b, p.mean(0)[0] + (a * ux - b * uy), p.mean(0)[1] + (b * ux + a * uy)


def corners(a, b, cx, cy, tw, th):
    a, b, cx, cy = (np.float64(v) for v in (a, b, cx, cy))
    return np.array([(cx + a * dx - b * dy, cy + b * dx + a * dy) for dx in (-tw / 2, tw / 2) for dy in (-th / 2, th / 2)])


def test_float32_fit_is_close_to_the_float64_fit():
    """The largest displacement of the four crop corners, in source pixels, between the float32 fit and the same closed form in float64 on
    the same float32 inputs: face template at 112 x 112, centres up to 3840 x 2160, scales 0.2 - 8, every angle, 2000 seeded cases.
    Measured on this set: 0.000523 px (an earlier measurement on another seeded set of the same description gave 0.0019 px).  The bound is
    4 x the value measured on this set: the margin covers libm and seed differences."""
    MEASURED = 0.000523
    N = 2000
    u = uniforms(0xA116ACC, N * 16).reshape(N, 16)
    tmpl = np.array(FACE5, dtype=F)
    worst = 0.0
    for i in range(N):
        scale, ang = 0.2 * 40 ** u[i, 0], 2 * np.pi * u[i, 1]
        cx, cy = u[i, 2] * 3840, u[i, 3] * 2160
        d = tmpl.astype(np.float64) - 56
        c, s = np.cos(ang) * scale, np.sin(ang) * scale
        xy = np.stack([cx + c * d[:, 0] - s * d[:, 1], cy + s * d[:, 0] + c * d[:, 1]], axis=1) + (u[i, 4:14].reshape(5, 2) - 0.5) * scale
        kp = kpts(xy)  # rounded to float32 here
        fit, _, why = align_fit_np(kp, tmpl, 112, 112, 3840, 2160, min_size=1)
        assert why is None, (i, why)
        worst = max(worst, float(np.hypot(*(corners(*fit["abc"], 112, 112) - corners(*fit64(kp, tmpl, 112, 112), 112, 112)).T).max()))
    print("largest corner displacement: %.6f px" % worst)
    assert worst < 4 * MEASURED, worst


# ---- exports, layouts, refusals ------------------------------------------------------------------------------------------------------------
def test_align_symbols_are_exported(marsrt):
    L = marsrt.lib()
    for n in NEW:
        assert n in marsrt.EXPORTS["mars_hip.h"], n
        assert hasattr(L, n), n
    for f in (marsrt.align_opts, marsrt.align_fit, marsrt.align_template_face5, marsrt.crop_aligned, marsrt.Model.crop_pose_detections,
              marsrt.Model.crop_pose_detections_device, marsrt.Model.align_results):
        assert callable(f)


def test_align_layouts(marsrt, tmp_path):
    assert marsrt.ALIGN_DTYPE.itemsize == 32 and marsrt.ALIGN_DTYPE.names == FIT_KEYS
    assert [marsrt.ALIGN_DTYPE.fields[k][1] for k in FIT_KEYS] == [0, 4, 8, 12, 16, 20, 24, 28]
    A = marsrt.AlignOpts
    assert [f[0] for f in A._fields_] == ["num_kpt", "tmpl", "use", "min_vis"]
    py = [C.sizeof(A), A.num_kpt.offset, A.tmpl.offset, A.use.offset, A.min_vis.offset]
    assert py == [268, 0, 4, 260, 264]
    inc = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include")
    src = tmp_path / "align_abi.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "mars_hip.h"\n'
                   'int main(void){ printf("%zu %zu %zu %zu %zu %zu %zu %zu %zu", sizeof(mars_hip_align_opts_t), offsetof(mars_hip_align_opts_t, num_kpt),\n'
                   ' offsetof(mars_hip_align_opts_t, tmpl), offsetof(mars_hip_align_opts_t, use), offsetof(mars_hip_align_opts_t, min_vis),\n'
                   ' sizeof(mars_align_t), offsetof(mars_align_t, Ux), offsetof(mars_align_t, used), offsetof(mars_align_t, n_used)); return 0; }\n')
    exe = tmp_path / "align_abi"
    subprocess.run(["gcc", "-I", inc, str(src), "-o", str(exe)], check=True)
    got = [int(v) for v in subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.split()]
    assert got == py + [32, 8, 24, 28]
    proto = tmp_path / "align_proto.c"
    proto.write_text('#include "mars_hip.h"\n'
                     'int (*a)(const mars_kpt_t *, const mars_hip_align_opts_t *, const mars_hip_roi_opts_t *, int, int, mars_align_t *, mars_roi_t *) = mars_yolo_align_fit;\n'
                     'int (*b)(int, int, float [][2]) = mars_yolo_align_template_face5;\n'
                     'mars_error_t (*c)(const unsigned char *, int, const mars_kpt_t *, const int *, int, const mars_hip_align_opts_t *,\n'
                     ' const mars_hip_roi_opts_t *, int, int, int, signed char *, mars_roi_t *, mars_align_t *) = mars_yolo_crop_aligned;\n'
                     'mars_error_t (*d)(mars_model_t *, const void *, mars_model_t *, int, const mars_hip_roi_opts_t *, const mars_hip_align_opts_t *) = mars_hip_crop_pose_device;\n'
                     'mars_error_t (*e)(mars_model_t *, const unsigned char *, mars_model_t *, int, const mars_hip_roi_opts_t *, const mars_hip_align_opts_t *) = mars_hip_crop_pose;\n'
                     'mars_error_t (*f)(mars_model_t *, mars_align_t *, int) = mars_hip_align_results;\n')
    subprocess.run(["gcc", "-Werror", "-I", inc, "-c", str(proto), "-o", str(tmp_path / "align_proto.o")], check=True)


def test_face5_template(marsrt):
    t = marsrt.align_template_face5(112, 112)
    assert t.dtype == np.float32 and np.array_equal(t, np.array(FACE5, dtype=F))
    t2 = marsrt.align_template_face5(224, 112)
    assert np.array_equal(t2[:, 0], t[:, 0] * F(2)) and np.array_equal(t2[:, 1], t[:, 1])
    t3 = marsrt.align_template_face5(112, 56)
    assert np.array_equal(t3[:, 0], t[:, 0]) and np.array_equal(t3[:, 1], t[:, 1] * F(0.5))
    L = marsrt.lib()
    assert L.mars_yolo_align_template_face5(0, 112, t.ctypes.data) == -1 and L.mars_yolo_align_template_face5(112, 112, None) == -1


def test_align_bad_arguments_are_refused_up_front(marsrt):
    L = marsrt.lib()
    BAD_FILE, BAD_TENSOR = marsrt.MARS_ERR_INVALID_FILE, marsrt.MARS_ERR_INVALID_TENSOR
    frames = np.zeros(6 * 4 * 3 + 64, dtype=np.uint8)
    kp = kpts([(1, 1), (4, 1), (1, 3), (4, 3), (2, 2)] * 2)
    fo = np.zeros(2, dtype=np.int32)
    out = np.full(2 * 8 * 8 * 3, 77, dtype=np.int8)
    rois = np.full(2, 77, dtype=marsrt.ROI_DTYPE)
    fits = np.full(2, 77, dtype=marsrt.ALIGN_DTYPE)
    fit1 = np.zeros((), dtype=marsrt.ALIGN_DTYPE)
    tmpl = [(1, 1), (7, 1), (1, 7), (7, 7), (4, 4)]

    def crop(o, a, n_frames=1, n_boxes=2, tw=8, th=8, fr=frames, kp_=kp):
        return L.mars_yolo_crop_aligned(None if fr is None else fr.ctypes.data, n_frames, None if kp_ is None else kp_.ctypes.data, fo.ctypes.data,
                                        n_boxes, None if a is None else C.byref(a), None if o is None else C.byref(o), tw, th, 1, out.ctypes.data,
                                        rois.ctypes.data, fits.ctypes.data)

    def host_fit(o, a, tw=8, th=8):
        return L.mars_yolo_align_fit(kp.ctypes.data, None if a is None else C.byref(a), None if o is None else C.byref(o), tw, th,
                                     fit1.ctypes.data, None)

    good, galign = marsrt.roi_opts(6, 4), marsrt.align_opts(tmpl)
    assert host_fit(good, galign) in (0, 1)
    bad_opts = [marsrt.roi_opts(0, 4), marsrt.roi_opts(6, 4, fmt=2), marsrt.roi_opts(6, 4, src_flags=1),      # what rot_opts refuses
                marsrt.roi_opts(5, 4, fmt=marsrt.CAMERA_NV12), marsrt.roi_opts(6, 4, expand=-1.0), marsrt.roi_opts(6, 4, min_size=-1),
                marsrt.roi_opts(6, 4, max_per_frame=-1), marsrt.roi_opts(6, 4, classes=(0, -1)), marsrt.roi_opts(6, 32768),
                marsrt.roi_opts(6, 4, keep_aspect=True), marsrt.roi_opts(6, 4, area=True)]                      # the two flags
    o = marsrt.roi_opts(6, 4)
    o.flags = 2
    bad_opts.append(o)
    bad_align = [marsrt.align_opts(np.zeros((0, 2))), marsrt.align_opts(np.zeros((33, 2))),                     # num_kpt outside 1 .. 32
                 marsrt.align_opts(tmpl, use=1 << 5), marsrt.align_opts(tmpl, use=1 << 31),                     # a bit at or above num_kpt
                 marsrt.align_opts(tmpl, min_vis=NAN), marsrt.align_opts(tmpl, min_vis=INF),
                 marsrt.align_opts([(1, 1), (7, 1), (1, NAN), (7, 7), (4, 4)]), marsrt.align_opts([(INF, 1), (7, 1), (1, 7), (7, 7), (4, 4)])]
    neg = marsrt.align_opts(tmpl)
    neg.num_kpt = -1
    bad_align.append(neg)
    P = C.POINTER(marsrt.MarsModel)
    a, b = marsrt.MarsModel(), marsrt.MarsModel()  # never looked into: the refusals come first
    for o, al in [(o, galign) for o in bad_opts] + [(good, al) for al in bad_align] + [(good, None), (None, galign)]:
        assert crop(o, al) == BAD_FILE
        assert host_fit(o, al) == -1
        for f in (L.mars_hip_crop_pose_device, L.mars_hip_crop_pose):
            assert f(C.pointer(a), frames.ctypes.data, C.pointer(b), 0, None if o is None else C.byref(o), None if al is None else C.byref(al)) == BAD_FILE
    # a non-finite template value behind num_kpt is not read; all 32 points with every bit of the mask are fine
    tail = marsrt.align_opts(tmpl)
    tail.tmpl[5][0] = NAN
    assert host_fit(good, tail) in (0, 1)
    kp32 = kpts(np.ones((32, 2)))  # (coincident points: skipped, not refused)
    assert L.mars_yolo_align_fit(kp32.ctypes.data, C.byref(marsrt.align_opts(np.ones((32, 2)), use=0xFFFFFFFF)), C.byref(good), 8, 8, fit1.ctypes.data, None) == 0
    for kw in (dict(tw=0), dict(th=-8), dict(n_frames=0), dict(n_boxes=0), dict(n_boxes=65536), dict(fr=None), dict(kp_=None)):
        assert crop(good, galign, **kw) == BAD_FILE, kw
    assert host_fit(good, galign, tw=0) == -1
    assert L.mars_yolo_align_fit(None, C.byref(galign), C.byref(good), 8, 8, fit1.ctypes.data, None) == -1
    assert L.mars_yolo_align_fit(kp.ctypes.data, C.byref(galign), C.byref(good), 8, 8, None, None) == -1
    assert (out == 77).all() and rois.tobytes() == np.full(2, 77, dtype=marsrt.ROI_DTYPE).tobytes() and (fits["n_used"] == 77).all()  # nothing was written
    for f in (L.mars_hip_crop_pose_device, L.mars_hip_crop_pose):
        assert f(P(), frames.ctypes.data, C.pointer(b), 0, C.byref(good), C.byref(galign)) == BAD_FILE       # no model
        assert f(C.pointer(a), None, C.pointer(b), 0, C.byref(good), C.byref(galign)) == BAD_FILE            # no frames
        assert f(C.pointer(a), frames.ctypes.data, C.pointer(a), 0, C.byref(good), C.byref(galign)) == BAD_TENSOR  # det_model == dst_model
    assert L.mars_hip_align_results(P(), fits.ctypes.data, 2) == BAD_FILE
    assert L.mars_hip_align_results(C.pointer(a), None, 2) == BAD_FILE and L.mars_hip_align_results(C.pointer(a), fits.ctypes.data, -1) == BAD_FILE
