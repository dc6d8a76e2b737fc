"""Motion maps on the device (mars_yolo_motion_frames, mars_hip_motion_device, mars_hip_motion_detections_device, mars_yolo_motion_boxes), byte
for byte and count for count against the restatement of include/mars_hip.h "Motion" (tests/motionref.py, pinned by tests/test_motion_cpu.py):
the maps, the statistics, the zone counts and the background of every stream.  tests/test_motion_cpu.py shows on the same scenes that no
case is vacuous; the cases here assert it again on what the restatement gives."""
import ctypes as C

import numpy as np
import pytest

import motionref as R
from test_gpu_move import Dev, hbm, same  # noqa: F401  (hbm: the fixture of guarded allocations)
from test_gpu_redact import FH, FW, Twin, dev_read
from test_gpu_redact import B as TB
from test_gpu_yolo_seg import DFL_KW, seg_graph

pytestmark = pytest.mark.gpu


def check_state(mo, ref, what):
    for s in range(ref.S):
        bg, init = mo.read(s)
        assert init == bool(ref.init[s]), (what, s)
        if init:
            same("%s: bg of stream %d" % (what, s), bg, ref.bg[s].astype(np.uint16))


def check_call(got, want, what):
    for g, w, name in zip(got, want, ("maps", "statistics", "zone counts")):
        assert g.shape == w.shape and g.dtype == w.dtype, (what, name, g.shape, w.shape)
        if name == "statistics":
            assert g.tobytes() == w.tobytes(), (what, g, w)
        else:
            same("%s: %s" % (what, name), g, w)


def both(gpu, S, W, H, fmt, B):
    return gpu.Motion(S, W, H, fmt, B), R.Detector(S, W, H, fmt, B)


def run_both(gpu, mo, ref, frames, what, **kw):
    """the host-pointer form and the restatement over the same frames and options; compares everything the call returns and the state"""
    zones = kw.pop("zones", ())
    flags = kw.pop("flags", 0)
    got = mo.frames(frames, gpu.motion_opts(flags=flags, zones=zones, **kw))
    want = ref.run(frames, flags=flags, zones=zones, **kw)
    check_call(got, want, what)
    check_state(mo, ref, what)
    return want


# ---- the host-pointer form --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("B", R.CELLS)
@pytest.mark.parametrize("fmt", [R.RGB, R.NV12])
def test_host_pointer_form(gpu, fmt, B):
    """every size x (S, T) in {(1, 1), (1, 5), (3, 2)}, the last in both frame orders; three zones ride along"""
    for W, H in (R.NV12_SIZES if fmt else R.RGB_SIZES):
        for S, T, flags in R.STREAMS_STEPS:
            mo, ref = both(gpu, S, W, H, fmt, B)
            frames = R.in_order(R.scene(W * 100 + B, S, T, W, H, fmt, B), bool(flags))
            what = "%d x %d fmt %d cell %d S %d T %d flags %d" % (W, H, fmt, B, S, T, flags)
            _, st, zc = run_both(gpu, mo, ref, frames, what, min_neighbors=R.case_min_neighbors(W, H, B), flags=flags, zones=R.case_zones(W, H, B, 3))
            if T == 1:
                assert st["first"].all() and not st["active"].any()
            else:
                assert R.not_vacuous(ref, W, H, B, T), what
                assert zc[:, 1].tolist() == st["active"].tolist()  # the whole frame
            mo.close()


@pytest.mark.parametrize("fmt, W, H", [(R.RGB, 80, 70), (R.RGB, 65, 66), (R.NV12, 128, 66), (R.NV12, 66, 130)])
def test_guarded_frames_at_every_alignment(hbm, gpu, fmt, W, H):
    """the device form on guarded allocations ([256 guard bytes][frames][256 guard bytes], tests/test_gpu_move.py): the payload offsets give
    every load path -- 16-byte units (80 x 70 and 128 x 66 at offsets 0 and 16), 4-byte units with byte ends -- and nothing is written to
    the frames or around them"""
    S, T = 1, 3
    for B in (4, 16):
        sc = R.in_order(R.scene(W + B, S, T, W, H, fmt, B), False)
        for off in (0, 1, 2, 3, 16):
            mo, ref = both(gpu, S, W, H, fmt, B)
            dev = hbm(sc, off=off, guard=0xA5)
            mo.device(dev.ptr, S * T, min_neighbors=1)
            what = "%d x %d fmt %d cell %d offset %d" % (W, H, fmt, B, off)
            check_call(mo.results(), ref.run(sc, min_neighbors=1), what)
            check_state(mo, ref, what)
            assert ref.active.any() and not ref.active.all() and (ref.raw & ~ref.active).any() and mo.ms() >= 0
            dev.unchanged(what)
            dev.free()
            mo.close()


# ---- the option edges ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("fmt, W, H, B", [(R.RGB, 65, 66, 4), (R.NV12, 66, 130, 16), (R.RGB, 257, 130, 16)])
def test_option_edges(gpu, fmt, W, H, B):
    S, T = 2, 4
    frames = R.in_order(R.scene(5 * W + B, S, T, W, H, fmt, B), False)
    cases = [dict(threshold=1), dict(threshold=255), dict(learn=1, learn_active=1), dict(learn=16, learn_active=16), dict(learn=1, learn_active=16),
             dict(min_neighbors=0), dict(min_neighbors=1), dict(min_neighbors=8), dict(flags=R.FRAME_DIFF, learn=16), dict(flags=R.FRAME_DIFF | R.STREAM_MAJOR),
             dict(min_neighbors=2, zones=R.case_zones(W, H, B))]
    actives = []
    for kw in cases:
        mo, ref = both(gpu, S, W, H, fmt, B)
        _, st, zc = run_both(gpu, mo, ref, frames, "%d x %d cell %d %s" % (W, H, B, sorted(k for k in kw)), **dict(kw))
        actives.append(int(st["active"].sum()))
        if "zones" in kw:
            assert zc.shape[1] == R.MAX_ZONES and zc[:, 1].tolist() == st["active"].tolist() and 0 < zc[:, 3:].sum() < zc.shape[1] * zc[:, 1].sum()
        mo.close()
    assert actives[0] > actives[1] == 0                      # one level catches what 255 levels cannot
    assert actives[5] > actives[6] > actives[7]              # the filter removes more and more
    assert len(set(actives)) >= 5


# ---- state ----------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("stream_major", [False, True])
def test_one_call_over_2T_steps_equals_two_over_T(gpu, stream_major):
    S, T, W, H, B, fmt = 3, 2, 65, 66, 16, R.RGB
    sc = R.scene(21, S, 2 * T, W, H, fmt, B)
    flags = R.STREAM_MAJOR if stream_major else 0
    one, ref1 = both(gpu, S, W, H, fmt, B)
    two, ref2 = both(gpu, S, W, H, fmt, B)
    run_both(gpu, one, ref1, R.in_order(sc, stream_major), "one call", min_neighbors=1, flags=flags)
    for h in (0, 1):
        run_both(gpu, two, ref2, R.in_order(sc[h * T:(h + 1) * T], stream_major), "call %d of two" % h, min_neighbors=1, flags=flags)
    for s in range(S):
        a, b = one.read(s), two.read(s)
        assert a[1] and b[1] and np.array_equal(a[0], b[0])
    assert ref2.active.any()
    one.close()
    two.close()


def test_reset_of_one_stream_and_a_second_detector(gpu):
    S, T, W, H, B, fmt = 3, 2, 34, 18, 4, R.NV12
    sc = R.scene(31, S, 2 * T, W, H, fmt, B)
    mo, ref = both(gpu, S, W, H, fmt, B)
    other, oref = both(gpu, S, W, H, fmt, B)
    run_both(gpu, mo, ref, R.in_order(sc[:T], False), "before the reset", min_neighbors=1)
    run_both(gpu, other, oref, R.in_order(sc[1:1 + T], False), "the second detector", min_neighbors=1)
    check_state(mo, ref, "the first detector behind the second one's call")  # independent
    before = [mo.read(s)[0] for s in range(S)]
    mo.reset(1)
    ref.reset(1)
    assert [mo.read(s)[1] for s in range(S)] == [True, False, True]
    assert np.array_equal(mo.read(0)[0], before[0]) and np.array_equal(mo.read(2)[0], before[2])
    _, st, _ = run_both(gpu, mo, ref, R.in_order(sc[T:], False), "behind the reset", min_neighbors=1)
    assert st["first"].tolist() == [0, 1, 0, 0, 0, 0]
    mo.reset()
    assert not any(mo.read(s)[1] for s in range(S))
    check_state(other, oref, "the second detector behind the first one's reset")
    mo.close()
    other.close()


def test_host_list_of_boxes(gpu):
    W, H, B, fmt, S, T = 257, 130, 16, R.RGB, 1, 3
    mo, ref = both(gpu, S, W, H, fmt, B)
    run_both(gpu, mo, ref, R.in_order(R.scene(41, S, T, W, H, fmt, B), False), "scene", min_neighbors=1)
    rng = np.random.default_rng(8)
    n = 60
    b = np.zeros(n, dtype=gpu.DET_DTYPE)
    b["x"], b["y"] = rng.uniform(-20, W + 20, n), rng.uniform(-20, H + 20, n)
    b["w"], b["h"], b["conf"] = rng.uniform(0.5, W / 2, n), rng.uniform(0.5, H / 2, n), 0.5
    b[0] = (W / 2, H / 2, 2 * W, 2 * H, 0.5, 0)  # the whole frame
    b[1] = (W - 0.5, H - 0.5, 1, 1, 0.5, 0)      # the last pixel
    b["x"][2], b["w"][3], b["h"][4] = np.nan, 0, -1
    fo = rng.integers(0, T, n).astype(np.int32)
    fo[0], fo[1], fo[5], fo[6] = 1, 2, -1, T       # the last two name no frame
    for expand in (0.0, 1.0, 1.7, 0.25):
        got, want = mo.boxes(b, fo, expand), ref.boxes(b, fo, expand)
        assert got.tobytes() == want.tobytes(), (expand, got, want)
    want = ref.boxes(b, fo)
    assert want["cells"][0] == ref.gw * ref.gh and not want[2:7].view(np.int32).any() and (want["active"] > 0).sum() > 3
    assert ((want["active"] < want["cells"]) & (want["active"] > 0)).any()
    assert len(mo.boxes(b[:0], fo[:0])) == 0
    mo.close()


# ---- the device form on the synthetic DFL twin of tests/test_gpu_redact.py --------------------------------------------------------------------
@pytest.fixture(scope="module")
def twin(gpu):
    t = Twin(gpu)
    yield t
    t.close()


def test_device_form_with_detections(gpu, twin):
    """motion -> detect -> motion_detections_device, nothing waiting in between: the counts equal the restatement on mars_hip_detect_results"""
    B = 8
    mo, ref = both(gpu, 1, FW, FH, R.RGB, B)
    sc = R.in_order(R.scene(51, 1, TB + 1, FW, FH, R.RGB, B), False)  # four steps of one stream: the first is the background
    run_both(gpu, mo, ref, sc[:1], "the background")
    sc = sc[1:]
    buf = twin.upload(sc)
    mo.device(buf.ptr, TB, min_neighbors=1)
    twin.m.detect_dfl_device(**dict(DFL_KW, src=(FW, FH)))
    twin.m.motion_detections_device(mo, 0.5)
    got = twin.m.motion_det_results()
    dets = twin.m.detect_results()
    check_call(mo.results(), ref.run(sc, min_neighbors=1), "device form")
    check_state(mo, ref, "device form")
    assert got.shape == (TB, gpu.MAX_DET) and sum(len(d) for d in dets) > 4 and ref.active.any()
    moved = partly = 0
    for f in range(TB):
        want = ref.boxes(dets[f], [f] * len(dets[f]), 0.5)
        assert got[f, :len(want)].tobytes() == want.tobytes(), (f, got[f, :len(want)], want)
        assert not got[f, len(want):].view(np.int32).any()  # behind the list
        moved += int((want["active"] > 0).sum())
        partly += int(((want["active"] > 0) & (want["active"] < want["cells"])).sum())
    assert moved > 0 and partly > 0
    assert mo.boxes(np.concatenate(dets), np.repeat(np.arange(TB), [len(d) for d in dets]), 0.5).tobytes() == \
        np.concatenate([got[f, :len(dets[f])] for f in range(TB)]).tobytes()
    # the refusals of the detection count
    FILE, TENSOR = gpu.MARS_ERR_INVALID_FILE, gpu.MARS_ERR_INVALID_TENSOR
    two, _ = both(gpu, 1, FW, FH, R.RGB, B)
    fresh = gpu.Model(seg_graph(4, False, 64)[0], batch=TB)
    calls = [(twin.m, two, 1.0, TENSOR),                  # no motion call on that detector
             (twin.m, mo, -1.0, FILE), (twin.m, mo, float("nan"), FILE), (fresh, mo, 1.0, TENSOR)]  # ..., no detections in HBM
    two2, _ = both(gpu, 2, FW, FH, R.RGB, B)
    two2.frames(np.concatenate([sc, sc[:1]]))              # F = 4 is not the batch
    calls.append((twin.m, two2, 1.0, TENSOR))
    for model, det, expand, code in calls:
        with pytest.raises(gpu.MarsError) as e:
            model.motion_detections_device(det, expand)
        assert e.value.code == code, (expand, code)
    with pytest.raises(gpu.MarsError) as e:
        fresh.motion_det_results()
    assert e.value.code == TENSOR
    fresh.pipe_open(download_outputs=False, detect=True, dfl_heads=gpu.yolo_dfl_heads(**DFL_KW))
    with pytest.raises(gpu.MarsError) as e:
        fresh.motion_detections_device(mo, 1.0)  # an open pipe
    assert e.value.code == TENSOR
    fresh.pipe_close()
    fresh.close()
    assert twin.m.motion_det_results().tobytes() == got.tobytes()  # no refused call touched the results
    check_state(mo, ref, "behind the refusals")
    for d in (mo, two, two2):
        d.close()


def test_ordering_against_the_redaction(gpu, twin):
    """motion -> redact in place -> motion on the same frames, nothing waiting in between: the first call has read the original pixels, the
    second the redacted ones"""
    B = 8
    frames = R.in_order(R.scene(61, TB, 1, FW, FH, R.RGB, B), False)  # one step of three streams
    first, ref1 = both(gpu, TB, FW, FH, R.RGB, B)
    second, ref2 = both(gpu, TB, FW, FH, R.RGB, B)
    for mo, ref in ((first, ref1), (second, ref2)):
        run_both(gpu, mo, ref, frames, "the background")
    buf = twin.upload(frames)
    dets = twin.detect()[0]
    assert sum(len(d) for d in dets) > 4
    first.device(buf.ptr, TB)
    twin.m.redact_device(buf.ptr, gpu.redact_opts(FW, FH, mode=gpu.REDACT_FILL, fill=(255, 255, 255), expand=0.35))
    second.device(buf.ptr, TB)
    got1, got2 = first.results(), second.results()
    red = dev_read(buf).reshape(frames.shape)
    assert twin.m.redact_results()["pixels"].sum() > 0 and not np.array_equal(red, frames)
    check_call(got1, ref1.run(frames), "motion enqueued before the redaction")
    check_call(got2, ref2.run(red), "motion enqueued behind it")
    assert not got1[1]["active"].any() and got2[1]["active"].sum() > 0
    check_state(first, ref1, "before")
    check_state(second, ref2, "behind")
    first.close()
    second.close()


# ---- refusals -------------------------------------------------------------------------------------------------------------------------------
def test_refusals_leave_the_state_alone(gpu):
    FILE, TENSOR = gpu.MARS_ERR_INVALID_FILE, gpu.MARS_ERR_INVALID_TENSOR
    W, H, B, S = 33, 45, 16, 2
    mo, ref = both(gpu, S, W, H, R.RGB, B)
    fresh, _ = both(gpu, S, W, H, R.RGB, B)
    with pytest.raises(gpu.MarsError) as e:
        fresh.results()  # nothing pending
    assert e.value.code == TENSOR and fresh.ms() < 0
    with pytest.raises(gpu.MarsError) as e:
        fresh.boxes(np.zeros(1, dtype=gpu.DET_DTYPE), [0])  # no maps yet
    assert e.value.code == TENSOR
    frames = R.in_order(R.scene(71, S, 2, W, H, R.RGB, B), False)
    want = run_both(gpu, mo, ref, frames, "the good call", min_neighbors=1)
    buf = gpu.DeviceBuffer(frames)
    L = gpu.lib()
    Z = lambda *rows: dict(zones=np.array(rows, dtype=np.int32))  # noqa: E731
    bad = [(dict(threshold=256), FILE), (dict(threshold=-1), FILE), (dict(learn=17), FILE), (dict(learn=-1), FILE), (dict(learn_active=17), FILE),
           (dict(learn_active=-2), FILE), (dict(min_neighbors=9), FILE), (dict(min_neighbors=-1), FILE), (dict(flags=4), FILE),
           (dict(zones=R.case_zones(W, H, B, 65)), FILE), (Z((0, 0, 0, 5)), FILE), (Z((3, 3, 9, 3)), FILE), (Z((0, 0, W + 1, 5)), FILE),
           (Z((-1, 0, 4, 5)), FILE), (Z((0, 0, 4, H + 1)), FILE)]
    for kw, code in bad:
        o = gpu.motion_opts(**kw)
        assert L.mars_hip_motion_device(mo.p, C.c_void_p(buf.ptr), 4, C.byref(o)) == code, kw
        assert L.mars_yolo_motion_frames(mo.p, frames.ctypes.data, 4, C.byref(o), None, None, None) == code, kw
    o = gpu.motion_opts()
    o.n_zones = 1  # zones without a table
    assert L.mars_hip_motion_device(mo.p, C.c_void_p(buf.ptr), 4, C.byref(o)) == FILE
    o = gpu.motion_opts()
    assert L.mars_hip_motion_device(mo.p, None, 4, C.byref(o)) == FILE and L.mars_hip_motion_device(mo.p, C.c_void_p(buf.ptr), 4, None) == FILE
    assert L.mars_yolo_motion_frames(mo.p, None, 4, C.byref(o), None, None, None) == FILE
    assert L.mars_hip_motion_device(mo.p, C.c_void_p(buf.ptr), 0, C.byref(o)) == FILE
    assert L.mars_hip_motion_device(mo.p, C.c_void_p(buf.ptr), 3, C.byref(o)) == TENSOR  # F % S != 0
    assert L.mars_yolo_motion_frames(mo.p, frames.ctypes.data, 3, C.byref(o), None, None, None) == TENSOR
    for stream in (S, -2, 70000):
        assert L.mars_hip_motion_reset(mo.p, stream) == TENSOR
    for stream in (S, -1):
        assert L.mars_hip_motion_read(mo.p, stream, None, None) == TENSOR
    box = np.zeros(1, dtype=gpu.DET_DTYPE)
    fo = np.zeros(1, dtype=np.int32)
    out = np.zeros(1, dtype=gpu.MOTION_DET_DTYPE)
    for expand in (-0.5, float("nan"), float("inf")):
        assert L.mars_yolo_motion_boxes(mo.p, box.ctypes.data, fo.ctypes.data, 1, expand, out.ctypes.data) == FILE
    assert L.mars_yolo_motion_boxes(mo.p, None, fo.ctypes.data, 1, 1.0, out.ctypes.data) == FILE
    # nothing moved: the state and the pending results are those of the good call
    check_state(mo, ref, "behind the refusals")
    check_call(mo.results(), want, "behind the refusals")
    assert np.array_equal(dev_read(buf), frames.reshape(-1))
    buf.free()
    mo.close()
    fresh.close()
