"""Second-stage labels (include/mars_hip.h, "Second-stage labels"), the part that needs no GPU: the six entry points are exported, mars_cls_t
is 8 bytes and the options struct matches its ctypes mirror, arguments that can never be valid are refused up front, and the numpy
restatement of the arithmetic that tests/test_gpu_classify.py compares the device against is itself checked on cases worked out by hand."""
import ctypes as C
import ctypes.util

import numpy as np

F = np.float32
MAX_DET = 1000
CLS = np.dtype([("cls", "<i4"), ("score", "<f4")])  # mars_cls_t, restated so that the helpers need no library
NEW = ["mars_yolo_classify_maps", "mars_hip_classify_device", "mars_hip_classify_results", "mars_hip_classify",
       "mars_hip_label_detections_device", "mars_hip_label_results"]

_libm = C.CDLL(ctypes.util.find_library("m") or "libm.so.6")
_libm.expf.restype = C.c_float
_libm.expf.argtypes = [C.c_float]


def expf(x):
    """the host libm's float expf (what csrc/expf_exact.h restates bit for bit: tests/test_expf_exact.py)"""
    return F(_libm.expf(C.c_float(float(x))))


# ---- the numpy restatement (int64 sums, np.float32 scalar steps rounded one by one) ----------------------------------------------------
def classify_np(maps, c, h, w, nhwc, scale, top_k, softmax):
    """int8 bytes of n dense maps ([h][w][c] or [c][h][w]) -> (CLS entries [n][top_k], int32 sums [n][c])"""
    a = np.ascontiguousarray(maps).view(np.int8).reshape(-1)
    a = a.reshape(-1, h * w, c).astype(np.int64).sum(axis=1) if nhwc else a.reshape(-1, c, h * w).astype(np.int64).sum(axis=2)
    assert np.abs(a).max() < 2 ** 31
    n = a.shape[0]
    top = np.zeros((n, top_k), dtype=CLS)
    top["cls"] = -1
    hw, sc = F(h * w), F(scale)
    for f in range(n):
        order = sorted(range(c), key=lambda ch: (-int(a[f, ch]), ch))
        logit = [F(F(F(int(a[f, ch])) / hw) * sc) for ch in range(c)]
        if softmax:
            e = [expf(F(logit[ch] - logit[order[0]])) for ch in range(c)]
            den = e[0]
            for ch in range(1, c):
                den = F(den + e[ch])
        for k, ch in enumerate(order[:top_k]):
            top[f, k] = (ch, F(e[ch] / den) if softmax else logit[ch])
    return top, a.astype(np.int32)


def label_np(rois, top1, counts):
    """ROI records of the kept crops, the top-1 entry of every crop, the detector's list lengths -> labels [frames][MAX_DET]"""
    labels = np.zeros((len(counts), MAX_DET), dtype=CLS)
    labels["cls"] = -1
    for k, r in enumerate(rois):
        assert 0 <= r["det"] < counts[r["frame"]]
        labels[r["frame"], r["det"]] = top1[k]
    return labels


# ---- exports, sizes, refusals -------------------------------------------------------------------------------------------------------------
def test_classify_symbols_are_exported(marsrt):
    L = marsrt.lib()
    for n in NEW:
        assert n in marsrt.EXPORTS["mars_hip.h"], n
        assert hasattr(L, n), n
    assert marsrt.CLS_MAX_TOPK == 8 and marsrt.CLS_SOFTMAX == 1 and marsrt.CLS_DTYPE == CLS
    for f in (marsrt.classify_maps, marsrt.cls_opts, marsrt.Model.classify, marsrt.Model.classify_device, marsrt.Model.classify_results,
              marsrt.Model.label_detections, marsrt.Model.label_results):
        assert callable(f)


def test_classify_record_sizes(marsrt, tmp_path):
    import os
    import subprocess
    assert marsrt.CLS_DTYPE.itemsize == 8
    assert [f[0] for f in marsrt.ClsOpts._fields_] == ["output_index", "tensor", "top_k", "scale", "flags"]
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    src = tmp_path / "cls_abi.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "mars_hip.h"\n'
                   'int main(void){ printf("%zu %zu %zu %zu %zu %zu %d %u", sizeof(mars_cls_t), offsetof(mars_cls_t, score), sizeof(mars_hip_cls_opts_t),\n'
                   ' offsetof(mars_hip_cls_opts_t, top_k), offsetof(mars_hip_cls_opts_t, scale), offsetof(mars_hip_cls_opts_t, flags),\n'
                   ' MARS_CLS_MAX_TOPK, MARS_CLS_SOFTMAX); return 0; }\n')
    exe = tmp_path / "cls_abi"
    subprocess.run(["gcc", "-I", os.path.join(root, "include"), str(src), "-o", str(exe)], check=True)
    got = subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.split()
    O = marsrt.ClsOpts
    assert got == ["8", "4", str(C.sizeof(O)), str(O.top_k.offset), str(O.scale.offset), str(O.flags.offset), "8", "1"]


def test_classify_bad_arguments_are_refused_up_front(marsrt):
    L = marsrt.lib()
    BAD_FILE, BAD_TENSOR = marsrt.MARS_ERR_INVALID_FILE, marsrt.MARS_ERR_INVALID_TENSOR
    maps = np.zeros(2 * 3 * 2 * 2, dtype=np.int8)
    top = np.full(2 * 8, 77, dtype=marsrt.CLS_DTYPE)
    sums = np.full(2 * 3, 77, dtype=np.int32)

    def run(o, n=2, c=3, h=2, w=2, scale=0.5, mp=maps, tp=top):
        return L.mars_yolo_classify_maps(None if mp is None else mp.ctypes.data, n, c, h, w, 1, scale, None if o is None else C.byref(o),
                                         None if tp is None else tp.ctypes.data, sums.ctypes.data)

    good = marsrt.cls_opts(top_k=3)
    bad = [marsrt.cls_opts(top_k=-1), marsrt.cls_opts(top_k=9), marsrt.cls_opts(scale=-0.5), marsrt.cls_opts(scale=float("nan")),
           marsrt.cls_opts(scale=float("inf"))]
    o = marsrt.cls_opts()
    o.flags = 2  # an unknown flag bit
    bad.append(o)
    P = C.POINTER(marsrt.MarsModel)
    a = marsrt.MarsModel()  # never looked into: the refusals come first
    for o in bad:
        assert run(o) == BAD_FILE
        assert L.mars_hip_classify_device(C.pointer(a), C.byref(o)) == BAD_FILE
        assert L.mars_hip_classify(C.pointer(a), C.byref(o), top.ctypes.data, None) == BAD_FILE
    assert run(None) == BAD_FILE
    for kw in (dict(n=0), dict(c=0), dict(h=-2), dict(w=0), dict(mp=None), dict(tp=None)):
        assert run(good, **kw) == BAD_FILE, kw
    for kw in (dict(c=4097), dict(h=4097, w=4096), dict(scale=0.0), dict(scale=-1.0), dict(n=65536)):  # beyond the limits; an effective scale <= 0
        assert run(good, **kw) == BAD_TENSOR, kw
    assert (top["cls"] == 77).all() and (sums == 77).all()  # nothing was written
    assert L.mars_hip_classify_device(P(), C.byref(good)) == BAD_FILE         # no model
    assert L.mars_hip_classify_device(C.pointer(a), None) == BAD_FILE         # no options
    assert L.mars_hip_classify(P(), C.byref(good), top.ctypes.data, None) == BAD_FILE
    assert L.mars_hip_classify(C.pointer(a), None, top.ctypes.data, None) == BAD_FILE
    assert L.mars_hip_classify(C.pointer(a), C.byref(good), None, None) == BAD_FILE
    assert L.mars_hip_classify_results(P(), top.ctypes.data, None, None) == BAD_FILE
    assert L.mars_hip_classify_results(C.pointer(a), None, None, None) == BAD_FILE
    assert L.mars_hip_label_detections_device(P(), C.pointer(a)) == BAD_FILE
    assert L.mars_hip_label_detections_device(C.pointer(a), P()) == BAD_FILE
    assert L.mars_hip_label_detections_device(C.pointer(a), C.pointer(a)) == BAD_TENSOR  # det_model == cls_model
    assert L.mars_hip_label_results(P(), top.ctypes.data) == BAD_FILE
    assert L.mars_hip_label_results(C.pointer(a), None) == BAD_FILE


# ---- the restatement itself ---------------------------------------------------------------------------------------------------------------
def test_restated_tie_by_hand():
    """a 2 x 2 x 3 map: channel sums 3, 3, 7 -> order 2, 0, 1 (the tie goes to the lower channel); logits (sum / 4) * 0.5"""
    px = np.array([[1, 2, 3], [4, -1, 0], [-2, 5, 3], [0, -3, 1]], dtype=np.int8)  # [h * w][c]
    for nhwc, m in ((True, px), (False, px.T.copy())):
        top, sums = classify_np(m, 3, 2, 2, nhwc, 0.5, 3, False)
        assert sums.tolist() == [[3, 3, 7]]
        assert top["cls"].tolist() == [[2, 0, 1]]
        assert top["score"].tolist() == [[0.875, 0.375, 0.375]]
        top, _ = classify_np(m, 3, 2, 2, nhwc, 0.5, 1, False)
        assert top["cls"].tolist() == [[2]] and top["score"].tolist() == [[0.875]]
        top, _ = classify_np(m, 3, 2, 2, nhwc, 0.5, 8, False)  # more entries than channels
        assert top["cls"].tolist() == [[2, 0, 1, -1, -1, -1, -1, -1]] and (top["score"][0, 3:] == 0).all()


def test_restated_softmax_by_hand():
    """three channels on one pixel, bytes 4, 0, 2, scale 0.5: logits 2, 0, 1; best = channel 0;
    e = expf(0), expf(-2), expf(-1); den = (e0 + e1) + e2, left to right; scores e / den in the order 0, 2, 1"""
    top, sums = classify_np(np.array([4, 0, 2], dtype=np.int8), 3, 1, 1, True, 0.5, 3, True)
    e0, e1, e2 = expf(F(0)), expf(F(-2)), expf(F(-1))
    assert e0 == F(1) and abs(float(e1) - 0.1353352832) < 1e-7 and abs(float(e2) - 0.3678794412) < 1e-7
    den = F(F(e0 + e1) + e2)
    assert sums.tolist() == [[4, 0, 2]] and top["cls"].tolist() == [[0, 2, 1]]
    assert top["score"][0].tobytes() == np.array([F(e0 / den), F(e2 / den), F(e1 / den)], dtype=F).tobytes()
    assert abs(float(top["score"][0].sum()) - 1.0) < 1e-6
    # two frames, planar, a scale that is no power of two: the same steps per frame
    m = np.array([[[3]], [[-5]], [[3]], [[9]], [[9]], [[-128]]], dtype=np.int8).reshape(2, 3)  # frame 0: 3, -5, 3; frame 1: 9, 9, -128
    top, sums = classify_np(m, 3, 1, 1, False, 0.3, 2, True)
    assert top["cls"].tolist() == [[0, 2], [0, 1]]
    l0 = [F(F(F(v) / F(1)) * F(0.3)) for v in (3, -5, 3)]
    e = [expf(F(x - l0[0])) for x in l0]
    den = F(F(e[0] + e[1]) + e[2])
    assert top["score"][0].tobytes() == np.array([F(e[0] / den), F(e[2] / den)], dtype=F).tobytes()


def test_restated_labels_by_hand():
    rois = np.zeros(3, dtype=[("frame", "<i4"), ("det", "<i4"), ("x0", "<i4"), ("y0", "<i4"), ("x1", "<i4"), ("y1", "<i4")])
    rois["frame"], rois["det"] = [0, 0, 2], [0, 3, 1]
    top1 = np.array([(5, 0.5), (7, 0.25), (1, 2.0), (9, 9.0)], dtype=CLS)  # a fourth crop slot that was not kept
    lab = label_np(rois, top1, [4, 6, 2])
    assert lab.shape == (3, MAX_DET)
    assert lab[0, 0].tolist() == (5, 0.5) and lab[0, 3].tolist() == (7, 0.25) and lab[2, 1].tolist() == (1, 2.0)
    assert (lab["cls"] != -1).sum() == 3 and (lab["score"] != 0).sum() == 3
