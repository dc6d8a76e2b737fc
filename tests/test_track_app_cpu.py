"""Appearance in tracking (include/mars_hip.h, "Appearance in tracking"), the part that needs no GPU.  Two groups.  The restatement checks
pin tests/trackappref.py -- cosines and a blend worked out by hand, equality with track_np where no detection has an embedding, and every
event in every seeded scene the GPU test runs -- and pass without the feature.  The feature checks compare the two host functions with the
restatement bit for bit, the header with the ctypes mirrors through a compiled probe, and walk the refusals that come before any device
work."""
import ctypes as C
import struct

import numpy as np
import pytest

from test_track_cpu import CLS, LOW, SCENE_IDS, SCENE_OPTS, SCENES, TRACK, F, TrackerNp, box, frames, scene, track_np
from trackappref import (APP_SCENE_OPTS, APP_SCENE_STEPS, SCENE_EVENTS, TrackerAppNp, app_scene, app_scene_list, blend_np, cosine_np,
                         quantise_np, rand_vectors, track_app_np)

NEW = ["mars_yolo_track_cosine", "mars_yolo_embed_blend", "mars_hip_tracker_create_app", "mars_hip_tracker_read_embeddings",
       "mars_yolo_track_lists_app", "mars_hip_track_app_device", "mars_hip_track_app", "mars_yolo_track_cosine_matrix"]
CHANNELS = (1, 63, 64, 65, 4096)
INT32_MIN = -(1 << 31)


# ---- the restatement itself ----------------------------------------------------------------------------------------------------------------
def test_restated_cosine_by_hand():
    # (3, 4) . (4, 3) = 24, both of length 5: 1 / sqrtf(25) is the float32 nearest 0.2, and the two products round one after the other
    fifth = F(1) / F(5)
    assert cosine_np([3, 4], 25, [4, 3], 25) == F(F(F(24) * fifth) * fifth)
    assert abs(float(cosine_np([3, 4], 25, [4, 3], 25)) - 0.96) < 1e-6
    assert cosine_np([3, 4], 25, [-3, -4], 25) == -cosine_np([3, 4], 25, [3, 4], 25)
    assert cosine_np([2, 0], 4, [0, 7], 49) == 0
    # a vector with itself: 127^2 * (1 / 127) * (1 / 127) in float32 -- within an ulp of 1, not clamped
    one = cosine_np([127], 16129, [127], 16129)
    assert one == F(F(F(16129) * (F(1) / F(127))) * (F(1) / F(127))) and abs(float(one) - 1.0) <= 2.0 ** -23


def test_restated_quantiser_and_blend_by_hand():
    q, qq = quantise_np([10, -5, 0])
    assert q.tolist() == [127, -64, 0] and qq == 127 * 127 + 64 * 64  # (5 * 127 + 5) // 10 = 64
    assert quantise_np([0, 0])[1] == 0
    q, qq = quantise_np([INT32_MIN, (1 << 31) - 1])
    assert q.tolist() == [-127, 127] and qq == 2 * 127 * 127
    # e = (127, 0), q = (0, 127): v = (381, 127), m = 381 -> (127, (127 * 127 + 190) // 381 = 42)
    e, ee = blend_np([127, 0], 16129, [0, 127], 16129)
    assert e.tolist() == [127, 42] and ee == 16129 + 1764
    # 3 e + q == 0: the slot is left without an embedding
    e, ee = blend_np([1, -1], 2, [-3, 3], 18)
    assert e.tolist() == [0, 0] and ee == 0
    # a detection without one: the slot keeps its own; a slot without one: it takes the detection's
    assert blend_np([5, 6], 61, [0, 0], 0)[1] == 61 and blend_np([0, 0], 0, [5, 6], 61)[0].tolist() == [5, 6]


def test_appearance_steers_a_crossing_by_hand():
    """two tracks 30 apart swap sides: the IoU alone hands each the other's box, the embeddings keep them apart"""
    d, n = frames([box(100, w=60, h=60), box(130, w=60, h=60)], [box(120, w=60, h=60), box(110, w=60, h=60)])
    vec = np.array([[100, 0], [0, 100], [100, 3], [2, 100]], dtype=np.int32)
    idx = np.full(d.shape, -1, dtype=np.int32)
    idx[0, :2] = [0, 1]
    idx[1, :2] = [2, 3]
    plain = track_np(TrackerNp(1), d, n)
    assert plain[1, :2].tolist() == [(2, 2), (1, 2)]
    trk = TrackerAppNp(1, 2)
    out = track_app_np(trk, d, n, vec, idx)
    assert out[1, :2].tolist() == [(1, 2), (2, 2)] and trk.events["key_changed"] == 2
    q, ee = trk.read_embeddings(0)
    assert q.tolist() == [[127, 4], [3, 127]] and ee.tolist() == [127 * 127 + 16, 127 * 127 + 9]
    # a jump to IoU 16 / 104 < 0.3: lost by the plain rule, kept on appearance; to 6 / 114 < 0.1: gated out
    for jump, ids, what in ((44, (1, 2), "app_low_iou"), (54, (2, 1), "gated")):
        d, n = frames([box(100, w=60, h=60)], [box(100 + jump, w=60, h=60)])
        assert track_np(TrackerNp(1), d, n)[1, 0].tolist() == (2, 1)
        trk = TrackerAppNp(1, 2)
        assert track_app_np(trk, d, n, vec, np.zeros(d.shape, dtype=np.int32))[1, 0].tolist() == ids and trk.events[what] == 1


@pytest.mark.parametrize("shape", SCENES, ids=SCENE_IDS)
def test_without_embeddings_the_restatement_is_track_np(shape):
    streams, steps, boxes, max_det = shape
    dets, counts = scene(0x7AC0000 + boxes, streams, steps, boxes, max_det)
    a, b = TrackerNp(streams), TrackerAppNp(streams, 8)
    want = track_np(a, dets, counts, low_conf=LOW, **SCENE_OPTS)
    none = np.full(dets.shape, 3, dtype=np.int32)
    got = track_app_np(b, dets, counts, np.zeros((3, 8), dtype=np.int32), none, low_conf=LOW, **SCENE_OPTS)  # null vectors only
    assert got.tobytes() == want.tobytes()
    for s in range(streams):
        assert a.read(s)[0].tobytes() == b.read(s)[0].tobytes() and a.read(s)[1].tolist() == b.read(s)[1].tolist()
        assert (b.read_embeddings(s)[1] == 0).all()


@pytest.mark.parametrize("case", app_scene_list(), ids=lambda c: "s%d_c%d_%s%s%s" % (c[1], c[2], "major" if c[3] else "minor", "_smooth" if c[4] else "",
                                                                                   "_low" if c[5] else ""))
def test_seeded_scenes_contain_every_event(case):
    """what keeps the GPU comparison from being vacuous: every scene it runs takes a pair on appearance below iou_thresh, lets the key
    change the outcome, gates a pair out, meets a cosine below the threshold, detections and tracks without an embedding, a null vector,
    a death that clears an embedding and a birth into a freed slot; with the flag, blends"""
    seed, streams, channels, major, smooth, low = case
    dets, counts, vectors, index = app_scene(seed, streams, channels, major)
    assert dets.shape[0] == streams * APP_SCENE_STEPS and counts.max() <= 12
    trk = TrackerAppNp(streams, channels)
    track_app_np(trk, dets, counts, vectors, index, low_conf=low, stream_major=major, smooth=smooth, **APP_SCENE_OPTS)
    for what in SCENE_EVENTS:
        assert trk.events[what] >= streams, (what, trk.events)
    assert (trk.events["smooth"] >= streams) == smooth and (trk.events["match2"] >= 1) == (low > 0)
    plain = TrackerNp(streams)
    track_np(plain, dets, counts, low_conf=low, stream_major=major, **APP_SCENE_OPTS)
    assert any(plain.read(b)[0].tobytes() != trk.read(b)[0].tobytes() for b in range(streams))  # the embeddings change the result


# ---- the feature: host functions -----------------------------------------------------------------------------------------------------------
def seeded_rows(seed, c):
    """int32 rows for the quantiser: random, one holding INT32_MIN and INT32_MAX, one null, one of +-1 only (every byte +-127)"""
    v = rand_vectors(seed, 8, c, shift=0)
    v[1, -1] = (1 << 31) - 1
    v[1, 0] = INT32_MIN  # (with one channel: the only value)
    v[2] = 0
    v[3] = np.where(v[3] < 0, -1, 1)
    v[4] = rand_vectors(seed + 1, 1, c, shift=30)[0]  # tiny values: many zeros
    return v


@pytest.mark.parametrize("c", CHANNELS)
def test_host_cosine_and_blend_match_the_restatement(marsrt, c):
    v = seeded_rows(0x7AB0000 + c, c)
    q, qq = marsrt.embed_quantise(v, c)
    for r in range(len(v)):
        want, wq = quantise_np(v[r])
        assert q[r].tobytes() == want.tobytes() and qq[r] == wq
    assert qq[2] == 0 and (np.abs(q[3]) == 127).all() and q[1, 0] == -127
    for a in range(len(v)):
        for b in range(len(v)):
            if qq[a] == 0 or qq[b] == 0:
                with pytest.raises(marsrt.MarsError) as ei:
                    marsrt.track_cosine(q[a], qq[a], q[b], qq[b])
                assert ei.value.code == marsrt.MARS_ERR_INVALID_TENSOR
            else:
                got = marsrt.track_cosine(q[a], qq[a], q[b], qq[b])
                assert got.tobytes() == cosine_np(q[a], int(qq[a]), q[b], int(qq[b])).tobytes(), (a, b)
            e, ee = marsrt.embed_blend(q[a], qq[a], q[b], qq[b])
            we, wee = blend_np(q[a], int(qq[a]), q[b], int(qq[b]))
            assert e.tobytes() == we.tobytes() and ee == wee, (a, b)
    # e = -q / 3 exactly: the blend is the null vector
    third = np.zeros(c, dtype=np.int8)
    third[0] = 1
    e, ee = marsrt.embed_blend(third, 1, -3 * third, 9)
    assert ee == 0 and not e.any()


# ---- the feature: exports, sizes -----------------------------------------------------------------------------------------------------------
def test_track_app_symbols_are_exported(marsrt):
    L = marsrt.lib()
    for n in NEW:
        assert n in marsrt.EXPORTS["mars_hip.h"], n
        assert hasattr(L, n), n
    for f in (marsrt.Tracker.read_embeddings, marsrt.track_app_opts, marsrt.track_lists_app, marsrt.track_cosine, marsrt.embed_blend,
              marsrt.track_cosine_matrix, marsrt.Model.track_app_device, marsrt.Model.track_app):
        assert callable(f)
    o = marsrt.track_app_opts()
    assert (o.app_thresh, o.app_min_iou, o.flags) == (0, 0, 0) and marsrt.track_app_opts(smooth=True).flags == marsrt.TRACK_APP_SMOOTH


def test_track_app_struct_layouts(marsrt, tmp_path):
    import os
    import subprocess
    A, O = marsrt.TrackAppOpts, marsrt.TrackOpts
    af = ["app_thresh", "app_min_iou", "flags"]
    assert [f[0] for f in A._fields_] == af
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    items = (["sizeof(mars_hip_track_app_opts_t)"] + ["offsetof(mars_hip_track_app_opts_t, %s)" % f for f in af] +
             ["(size_t)MARS_TRACK_APP_SMOOTH", "sizeof(mars_hip_track_opts_t)", "sizeof(mars_track_state_t)", "sizeof(mars_track_t)"])
    protos = ["mars_error_t (*p%d)(%s) = %s;" % (i, sig, name) for i, (name, sig) in enumerate([
        ("mars_yolo_track_cosine", "const signed char *, int, const signed char *, int, int, float *"),
        ("mars_yolo_embed_blend", "const signed char *, int, const signed char *, int, int, signed char *, int *"),
        ("mars_hip_tracker_create_app", "int, int, mars_hip_tracker_t **"),
        ("mars_hip_tracker_read_embeddings", "mars_hip_tracker_t *, int, signed char *, int *, int, int *"),
        ("mars_yolo_track_lists_app", "mars_hip_tracker_t *, const mars_det_t *, const int *, const mars_cls_t *, const int *, int, const int *, int, int, "
                                      "const mars_hip_track_opts_t *, const mars_hip_track_app_opts_t *, mars_track_t *"),
        ("mars_hip_track_app_device", "mars_model_t *, mars_model_t *, mars_hip_tracker_t *, const mars_hip_track_opts_t *, const mars_hip_track_app_opts_t *"),
        ("mars_hip_track_app", "mars_model_t *, mars_model_t *, mars_hip_tracker_t *, const mars_hip_track_opts_t *, const mars_hip_track_app_opts_t *, mars_track_t *"),
        ("mars_yolo_track_cosine_matrix", "const signed char *, const int *, const int *, int, int, int, float *")])]
    src = tmp_path / "track_app_abi.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "mars_hip.h"\n#ifdef PROTOTYPES\n%s\n#endif\nint main(void){ size_t v[] = {%s};\n'
                   ' for (size_t i = 0; i < sizeof(v) / sizeof(v[0]); i++) printf("%%zu ", v[i]); return 0; }\n' % ("\n".join(protos), ", ".join(items)))
    exe = tmp_path / "track_app_abi"
    inc = ["-I", os.path.join(root, "include")]
    subprocess.run(["gcc", "-Werror", "-DPROTOTYPES", "-c"] + inc + [str(src), "-o", str(tmp_path / "track_app_abi.o")], check=True)  # the declared types
    subprocess.run(["gcc"] + inc + [str(src), "-o", str(exe)], check=True)
    got = [int(x) for x in subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.split()]
    assert got == [C.sizeof(A)] + [getattr(A, f).offset for f in af] + [marsrt.TRACK_APP_SMOOTH, C.sizeof(O), 48, 8]
    assert C.sizeof(A) == 12 and C.sizeof(O) == 32


# ---- the feature: refusals -----------------------------------------------------------------------------------------------------------------
def test_track_app_bad_arguments_are_refused_up_front(marsrt):
    L = marsrt.lib()
    BAD_FILE, BAD_TENSOR = marsrt.MARS_ERR_INVALID_FILE, marsrt.MARS_ERR_INVALID_TENSOR
    P = C.POINTER(marsrt.MarsModel)
    a, b = marsrt.MarsModel(), marsrt.MarsModel()  # never looked into: the refusals come first
    fake = (C.c_char * 256)()                      # stands where a tracker would: three streams, no tables, no embedding plane
    struct.pack_into("i", fake, 0, 3)
    trk = C.cast(fake, C.c_void_p)
    d, n = frames([box(0)], [box(1)], [box(2)], [box(3)], [box(4)], [box(5)])
    ids = np.zeros(d.shape, dtype=CLS)
    vec = np.ones((4, 8), dtype=np.int32)
    idx = np.zeros(d.shape, dtype=np.int32)
    out = np.full(d.shape, 77, dtype=TRACK)
    good, app = marsrt.track_opts(), marsrt.track_app_opts()

    # the lifecycle
    p = C.c_void_p()
    assert L.mars_hip_tracker_create_app(3, 8, None) == BAD_FILE
    for s, c, code in ((0, 8, BAD_FILE), (-2, 8, BAD_FILE), (3, 0, BAD_FILE), (3, -1, BAD_FILE), (65536, 8, BAD_TENSOR), (3, 4097, BAD_TENSOR)):
        assert L.mars_hip_tracker_create_app(s, c, C.byref(p)) == code and not p.value
    q = np.zeros((4, 8), dtype=np.int8)
    ee = np.zeros(4, dtype=np.int32)
    nl = C.c_int(77)
    assert L.mars_hip_tracker_read_embeddings(None, 0, q.ctypes.data, ee.ctypes.data, 4, C.byref(nl)) == BAD_FILE
    assert L.mars_hip_tracker_read_embeddings(trk, 0, None, ee.ctypes.data, 4, C.byref(nl)) == BAD_FILE
    assert L.mars_hip_tracker_read_embeddings(trk, 0, q.ctypes.data, None, 4, C.byref(nl)) == BAD_FILE
    assert L.mars_hip_tracker_read_embeddings(trk, 0, q.ctypes.data, ee.ctypes.data, -1, C.byref(nl)) == BAD_FILE
    assert L.mars_hip_tracker_read_embeddings(trk, 3, q.ctypes.data, ee.ctypes.data, 4, C.byref(nl)) == BAD_TENSOR
    assert L.mars_hip_tracker_read_embeddings(trk, 0, q.ctypes.data, ee.ctypes.data, 4, C.byref(nl)) == BAD_TENSOR  # no plane
    assert nl.value == 77

    def ptr(x):
        return None if x is None else x.ctypes.data

    def run(o, ap=app, t=trk, dd=d, cc=n, ii=None, vv=vec, nv=4, ee=idx, nf=6, md=8, oo=out):
        return L.mars_yolo_track_lists_app(t, ptr(dd), ptr(cc), ptr(ii), ptr(vv), nv, ptr(ee), nf, md, None if o is None else C.byref(o),
                                           None if ap is None else C.byref(ap), ptr(oo))

    def dev(o, ap=app, det=C.pointer(a), cls=C.pointer(b), t=trk):
        return L.mars_hip_track_app_device(det, cls, t, None if o is None else C.byref(o), None if ap is None else C.byref(ap))

    def dev_fetch(o, ap=app, det=C.pointer(a), cls=C.pointer(b), t=trk, oo=out):
        return L.mars_hip_track_app(det, cls, t, None if o is None else C.byref(o), None if ap is None else C.byref(ap), ptr(oo))

    # the appearance options
    nan, inf = float("nan"), float("inf")
    bad = [marsrt.track_app_opts(**kw) for kw in (dict(app_thresh=-0.1), dict(app_thresh=nan), dict(app_thresh=inf), dict(app_thresh=1.5),
                                                  dict(app_min_iou=-0.1), dict(app_min_iou=nan), dict(app_min_iou=-inf), dict(app_min_iou=1.01))]
    for bit in (2, 4, 1 << 31):
        o = marsrt.track_app_opts()
        o.flags = bit
        bad.append(o)
    for o in bad:
        assert run(good, ap=o) == BAD_FILE and dev(good, ap=o) == BAD_FILE and dev_fetch(good, ap=o) == BAD_FILE
    assert run(good, ap=None) == BAD_FILE and dev(good, ap=None) == BAD_FILE and dev_fetch(good, ap=None) == BAD_FILE
    # the tracking options, as for the plain calls: flag bits 8 and 16 stay unknown
    worse = [marsrt.track_opts(**kw) for kw in (dict(min_conf=-0.1), dict(low_conf=nan), dict(iou_thresh=1.01), dict(max_miss=-1), dict(low_conf=0.5))]
    for bit in (8, 16, 1 << 31):
        o = marsrt.track_opts()
        o.flags = bit
        worse.append(o)
    for o in worse:
        assert run(o) == BAD_FILE and dev(o) == BAD_FILE and dev_fetch(o) == BAD_FILE
        assert L.mars_yolo_track_lists(trk, d.ctypes.data, n.ctypes.data, None, 6, 8, C.byref(o), out.ctypes.data) == BAD_FILE
    assert run(None) == BAD_FILE and dev(None) == BAD_FILE and dev_fetch(None) == BAD_FILE
    # the arguments of the list form
    for kw in (dict(t=None), dict(dd=None), dict(cc=None), dict(oo=None), dict(nf=0), dict(nf=-3), dict(md=0), dict(md=-1), dict(nv=-1),
               dict(vv=None), dict(ee=None)):
        assert run(good, **kw) == BAD_FILE, kw
    assert run(marsrt.track_opts(carry_identity=True)) == BAD_FILE               # the flag without the array
    assert run(good, md=1001) == BAD_TENSOR
    assert run(good, nf=4) == BAD_TENSOR and run(good, nf=5) == BAD_TENSOR       # F % S != 0
    assert run(good) == BAD_TENSOR                                               # a tracker without a plane
    assert run(good, vv=None, nv=0, ee=None) == BAD_TENSOR                       # ... also with nothing to quantise
    assert run(marsrt.track_opts(carry_identity=True, stream_major=True), ap=marsrt.track_app_opts(1.0, 1.0, True), ii=ids) == BAD_TENSOR
    assert (out["id"] == 77).all() and (out["hits"] == 77).all()                 # nothing was written
    # the model forms
    assert dev(good, det=P()) == BAD_FILE and dev(good, cls=P()) == BAD_FILE and dev(good, t=None) == BAD_FILE
    assert dev_fetch(good, det=P()) == BAD_FILE and dev_fetch(good, cls=P()) == BAD_FILE and dev_fetch(good, t=None) == BAD_FILE
    assert dev_fetch(good, oo=None) == BAD_FILE
    assert dev(good, cls=C.pointer(a)) == BAD_TENSOR                             # det_model == cls_model
    assert dev(good) == BAD_TENSOR and dev_fetch(good) == BAD_TENSOR             # a tracker without a plane, before either model is looked into
    # the host functions and the hook
    f = C.c_float(7)
    i = C.c_int(7)
    q8 = np.ones(8, dtype=np.int8)
    assert L.mars_yolo_track_cosine(None, 8, q8.ctypes.data, 8, 8, C.byref(f)) == BAD_FILE
    assert L.mars_yolo_track_cosine(q8.ctypes.data, 8, None, 8, 8, C.byref(f)) == BAD_FILE
    assert L.mars_yolo_track_cosine(q8.ctypes.data, 8, q8.ctypes.data, 8, 8, None) == BAD_FILE
    assert L.mars_yolo_track_cosine(q8.ctypes.data, 8, q8.ctypes.data, 8, 0, C.byref(f)) == BAD_FILE
    assert L.mars_yolo_track_cosine(q8.ctypes.data, 8, q8.ctypes.data, 8, 4097, C.byref(f)) == BAD_TENSOR
    assert L.mars_yolo_track_cosine(q8.ctypes.data, 0, q8.ctypes.data, 8, 8, C.byref(f)) == BAD_TENSOR
    assert L.mars_yolo_track_cosine(q8.ctypes.data, 8, q8.ctypes.data, 0, 8, C.byref(f)) == BAD_TENSOR
    assert f.value == 7
    assert L.mars_yolo_embed_blend(q8.ctypes.data, 8, q8.ctypes.data, 8, 8, None, C.byref(i)) == BAD_FILE
    assert L.mars_yolo_embed_blend(q8.ctypes.data, 8, q8.ctypes.data, 8, 8, q8.ctypes.data, None) == BAD_FILE
    assert L.mars_yolo_embed_blend(None, 8, q8.ctypes.data, 8, 8, q8.ctypes.data, C.byref(i)) == BAD_FILE
    assert L.mars_yolo_embed_blend(q8.ctypes.data, 8, q8.ctypes.data, -1, 8, q8.ctypes.data, C.byref(i)) == BAD_FILE
    assert L.mars_yolo_embed_blend(q8.ctypes.data, 8, q8.ctypes.data, 8, 0, q8.ctypes.data, C.byref(i)) == BAD_FILE
    assert L.mars_yolo_embed_blend(q8.ctypes.data, 8, q8.ctypes.data, 8, 4097, q8.ctypes.data, C.byref(i)) == BAD_TENSOR
    assert i.value == 7
    m = np.zeros((4, 4), dtype=np.float32)
    tq, te = np.ones((4, 8), dtype=np.int8), np.full(4, 8, dtype=np.int32)

    def hook(a0=tq, a1=te, a2=vec, nt=4, nc=4, c=8, oo=m):
        return L.mars_yolo_track_cosine_matrix(ptr(a0), ptr(a1), ptr(a2), nt, nc, c, ptr(oo))

    for kw in (dict(a0=None), dict(a1=None), dict(a2=None), dict(oo=None), dict(nt=0), dict(nc=0), dict(nc=-1), dict(c=0)):
        assert hook(**kw) == BAD_FILE, kw
    for kw in (dict(nt=257), dict(nc=257), dict(c=4097)):
        assert hook(**kw) == BAD_TENSOR, kw
    assert not m.any()
