"""Redaction on the device (mars_yolo_redact_frames, mars_hip_redact_device, mars_hip_redact), byte for byte and count for count against the
restatement of include/mars_hip.h "Redaction" (tests/redactref.py, pinned by tests/test_redact_cpu.py).  Every case checks that it is not
vacuous: some pixel is redacted, some is not, some cell is redacted in part, and `pixels` is the restatement's."""
import ctypes as C
import types

import numpy as np
import pytest

import redactref as R
from test_gpu_maskup import random_boxes
from test_gpu_move import Dev, hbm, same  # noqa: F401  (hbm: the fixture of guarded allocations)
from test_gpu_roi import second_stage
from test_gpu_yolo_seg import DFL_KW, fill, seg_graph
from test_roi_cpu import roi_crop_np, roi_select_np

pytestmark = pytest.mark.gpu

FILL_RGB = (7, 99, 201)
RGB_SIZES = [(2, 2), (31, 17), (33, 45), (65, 66), (257, 130)]   # rows of 93, 99, 195 and 771 bytes: no alignment repeats; one pixel past a
NV12_SIZES = [(2, 2), (34, 18), (66, 130), (128, 64), (258, 130)]  # word and past a tile, clipped edge cells, a ragged last word, three tile rows


# ---- the cases (functions of their arguments alone: tests/test_redact_cpu.py style checks run on them without a device) ----------------------
def case_boxes(dtype_holder, rng, n, F, W, H):
    """random_boxes of tests/test_gpu_maskup.py over the frame, the sizes of all but box 0 scaled down so that n boxes leave pixels free; box 0
    covers the whole frame where there are other frames to stay partly free (n >= 17, F > 1: it goes to frame 0), else the middle of it; from
    17 boxes on one has a NaN and one has w = 0.  A 2 x 2 frame gets the one box that covers pixel (0, 0) alone.  -> (boxes, frame_of_box)"""
    g = types.SimpleNamespace(base_w=W, base_h=H)
    b = random_boxes(dtype_holder, rng, n, g)
    fo = rng.integers(0, F, n).astype(np.int32)
    if n == 0:
        return b, fo
    if W == 2:
        b, fo = b[:1], fo[:1]
        b[0] = (0.5, 0.5, 1, 1, 0.5, 0)
        return b, fo
    f = min(0.5, 1.7 / np.sqrt(max(n / F, 1)))
    b["w"][1:] *= f
    b["h"][1:] *= f
    if n >= 17 and F > 1:
        fo[0] = 0
        fo[1:][fo[1:] == 0] = 1  # frame 0 is all redacted, the others in part
    else:
        b[0] = (W * 0.45, H * 0.55, W * 0.4, H * 0.35, 0.0, 0)
    if n >= 17:
        b["x"][5] = np.nan
        b["w"][6] = 0
    return b, fo


def partly(unions, W, H, B):
    """some cell of some frame is redacted in part"""
    ys, xs = np.arange(0, H, B), np.arange(0, W, B)
    n = (np.minimum(ys + B, H) - ys)[:, None] * (np.minimum(xs + B, W) - xs)[None, :]
    for U in unions:
        k = np.add.reduceat(np.add.reduceat(U.astype(np.int64), ys, axis=0), xs, axis=1)
        if ((k > 0) & (k < n)).any():
            return True
    return False


def not_vacuous(unions, stats, W, H, B):
    return bool(any(U.any() for U in unions) and any((~U).any() for U in unions) and partly(unions, W, H, B) and stats["pixels"].sum() > 0)


def frames_of(rng, F, W, H, fmt):
    return rng.integers(0, 256, (F, R.frame_bytes(W, H, fmt)), dtype=np.uint8)


def gpu_opts(gpu, W, H, fmt, mode, cell, flags=0, **kw):
    return gpu.redact_opts(W, H, fmt=fmt, src_flags=flags, mode=mode, cell=cell, fill=FILL_RGB, **kw)


def check_host(gpu, frames, b, fo, W, H, fmt, mode, cell, flags=0, mw=None, mo=None, inplace=False, expand=0.0):
    got, st = gpu.redact_frames(frames, b, fo, gpu_opts(gpu, W, H, fmt, mode, cell, flags, expand=expand), mask_words=mw, mask_of_box=mo,
                                inplace=inplace)
    want, wst, unions = R.redact_frames_np(frames, b, fo, W, H, fmt, mode, cell, FILL_RGB, expand, flags, mw, mo)
    what = (W, H, fmt, mode, cell, len(b), len(frames), inplace)
    assert st.tobytes() == wst.tobytes(), (what, st, wst)
    same("redacted frames %s" % (what,), got, want)
    return got, wst, unions


# ---- the host-pointer form -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cell", [2, 8, 64])
@pytest.mark.parametrize("mode", [R.MOSAIC, R.FILL])
@pytest.mark.parametrize("fmt", [R.RGB, R.NV12])
def test_host_pointer_form(gpu, fmt, mode, cell):
    """out of place; every size x n_boxes in {0, 1, 17, 300} x F in {1, 3} (257 x 130: one frame); NV12 in both chroma orders"""
    rng = np.random.default_rng(fmt * 100 + mode * 10 + cell)
    for W, H in (NV12_SIZES if fmt else RGB_SIZES):
        for F in ((1,) if W >= 257 else (1, 3)):
            for n in (0, 1, 17, 300):
                frames = frames_of(rng, F, W, H, fmt)
                b, fo = case_boxes(gpu, rng, n, F, W, H)
                flags = (gpu.NV12_VU if n == 17 else gpu.NV12_FULL_RANGE if n == 1 else 0) if fmt else 0
                got, st, unions = check_host(gpu, frames, b, fo, W, H, fmt, mode, cell, flags)
                if n == 0:
                    assert np.array_equal(got, frames) and not st["regions"].any()
                else:
                    assert not_vacuous(unions, st, W, H, cell), (W, H, F, n)
                    assert len(b) < 17 or (st["skipped"].sum() >= 2 and st["regions"].sum() > 0)


def test_every_box_skipped_leaves_the_frames_alone(gpu):
    for fmt, W, H in ((R.RGB, 65, 66), (R.NV12, 66, 130)):
        rng = np.random.default_rng(W)
        frames = frames_of(rng, 3, W, H, fmt)
        nan = float("nan")
        b = np.array([(nan, 5, 4, 4, 0.5, 0), (10, 10, 0, 4, 0.5, 0), (10, 10, 4, -1, 0.5, 0), (W + 40, 10, 8, 8, 0.5, 0), (10, -30, 8, 8, 0.5, 0),
                      (10, 10, 4, 4, nan, 0), (10, 10, float("inf"), 4, 0.5, 0)], dtype=gpu.DET_DTYPE)
        fo = np.array([0, 1, 2, 0, 1, 2, 0], dtype=np.int32)
        for inplace in (False, True):
            got, st, _ = check_host(gpu, frames, b, fo, W, H, fmt, R.MOSAIC, 8, inplace=inplace)
            assert np.array_equal(got, frames) and st["skipped"].tolist() == [3, 2, 2] and not st["regions"].any() and not st["pixels"].any()
        # a frame index that names no frame: the box is left out
        got, st = gpu.redact_frames(frames, b[:1], np.array([7], dtype=np.int32), gpu_opts(gpu, W, H, fmt, R.MOSAIC, 8))
        assert np.array_equal(got, frames) and not st.view(np.int32).any()


# ---- masks -----------------------------------------------------------------------------------------------------------------------------------
def mask_case(rng, n, n_masks, W, H, density):
    """random words (bits outside every rectangle and in the last word's padding included) and a mask_of_box that mixes -1 with repeats"""
    pitch = (W + 31) // 32
    if density == 0:
        mw = np.zeros((n_masks, H, pitch), dtype=np.uint32)
    elif density == 1:
        mw = np.full((n_masks, H, pitch), 0xFFFFFFFF, dtype=np.uint32)
    else:
        mw = rng.integers(0, 1 << 32, (n_masks, H, pitch), dtype=np.uint64).astype(np.uint32)
    mo = rng.integers(-1, n_masks, n).astype(np.int32)
    mo[:3] = (n_masks - 1, -1, n_masks - 1)  # a repeat, and the last mask is addressed
    return mw, mo


@pytest.mark.parametrize("fmt, W, H", [(R.RGB, 31, 17), (R.RGB, 32, 18), (R.RGB, 33, 45), (R.RGB, 65, 66), (R.RGB, 257, 130), (R.NV12, 32, 18),
                                       (R.NV12, 66, 130)])
def test_masks(gpu, fmt, W, H):
    rng = np.random.default_rng(W * 7 + fmt)
    F, n = (1, 9) if W >= 257 else (2, 12)
    frames = frames_of(rng, F, W, H, fmt)
    b, fo = case_boxes(gpu, rng, n, F, W, H)
    b["w"][1:] *= 2
    b["h"][1:] *= 2
    for density in (0, 0.5, 1):
        for mode, cell in ((R.MOSAIC, 2), (R.MOSAIC, 16), (R.FILL, 64)):
            mw, mo = mask_case(rng, n, 4, W, H, density)
            got, st, unions = check_host(gpu, frames, b, fo, W, H, fmt, mode, cell, mw=mw, mo=mo, expand=1.25)
            assert st["masked"].sum() >= 2 and st["regions"].sum() > st["masked"].sum()
            assert not_vacuous(unions, st, W, H, cell), (density, mode, cell)
            if density == 1:  # full masks are the rectangles
                plain = gpu.redact_frames(frames, b, fo, gpu_opts(gpu, W, H, fmt, mode, cell, expand=1.25))
                assert np.array_equal(plain[0], got) and plain[1]["pixels"].tolist() == st["pixels"].tolist()


# ---- in place -------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("fmt", [R.RGB, R.NV12])
def test_in_place_equals_out_of_place(gpu, fmt):
    rng = np.random.default_rng(40 + fmt)
    for W, H in ((NV12_SIZES if fmt else RGB_SIZES)[1:]):
        F = 1 if W >= 257 else 3
        frames = frames_of(rng, F, W, H, fmt)
        b, fo = case_boxes(gpu, rng, 17, F, W, H)
        mw, mo = mask_case(rng, 17, 3, W, H, 0.5)
        for mode, cell in ((R.MOSAIC, 4), (R.MOSAIC, 32), (R.FILL, 16)):
            a, st, unions = check_host(gpu, frames, b, fo, W, H, fmt, mode, cell, mw=mw, mo=mo)
            c, _, _ = check_host(gpu, frames, b, fo, W, H, fmt, mode, cell, mw=mw, mo=mo, inplace=True)
            assert np.array_equal(a, c) and not_vacuous(unions, st, W, H, cell)


class LaunchRec(C.Structure):  # mhip_redact_t of csrc/mhip.h
    _fields_ = [("frames", C.c_void_p), ("dst", C.c_void_p), ("frame_stride", C.c_size_t), ("n_frames", C.c_int), ("w", C.c_int), ("h", C.c_int),
                ("fmt", C.c_int), ("nv12_flags", C.c_uint), ("dets", C.c_void_p), ("counts", C.c_void_p), ("list_off", C.c_void_p),
                ("det_cap", C.c_int), ("select_all", C.c_int), ("expand", C.c_float), ("min_conf", C.c_float), ("ident_min", C.c_float),
                ("cls_first", C.c_int), ("cls_count", C.c_int), ("idents", C.c_void_p), ("mask_recs", C.c_void_p), ("mask_max", C.c_int),
                ("mask_of", C.c_void_p), ("mask_words", C.c_void_p), ("mode", C.c_int), ("cell_log2", C.c_int), ("fill", C.c_ubyte * 3),
                ("table", C.c_void_p), ("table_n", C.c_void_p), ("stats", C.c_void_p)]


@pytest.mark.parametrize("fmt, W, H", [(R.RGB, 80, 70), (R.RGB, 65, 66), (R.NV12, 128, 66), (R.NV12, 66, 130)])
def test_guard_bands_and_every_alignment(hbm, gpu, fmt, W, H):
    """the launchers themselves on guarded allocations ([256 guard bytes][frames][256 guard bytes], tests/test_gpu_move.py): in place the
    guards in front of and behind the frames stay untouched, out of place those of the destination, whose unredacted bytes are copies.  The
    payload offsets give every store path: 16-byte units (80 x 70 and 128 x 66 at offset 0), 4-byte units with byte ends, and bytes alone
    where the two buffers differ in their alignment"""
    L = hbm.L
    for fn in (L.mhip_redact_select, L.mhip_redact):
        fn.restype, fn.argtypes = C.c_int, [C.POINTER(LaunchRec)]
    rng = np.random.default_rng(W + fmt)
    F, n = 2, 10
    frames = frames_of(rng, F, W, H, fmt)
    b, fo = case_boxes(gpu, rng, n, F, W, H)
    order = np.argsort(fo, kind="stable")
    b, fo = b[order], fo[order]
    counts = np.bincount(fo, minlength=F).astype(np.int32)
    list_off = (np.cumsum(counts) - counts).astype(np.int32)
    for mode, cell in ((R.MOSAIC, 8), (R.FILL, 2)):
        want, wst, unions = R.redact_frames_np(frames, b, fo, W, H, fmt, mode, cell, FILL_RGB)
        assert not_vacuous(unions, wst, W, H, cell)
        for src_off, dst_off in ((0, None), (1, None), (2, None), (0, 0), (0, 16), (5, 1), (0, 3), (3, 0)):
            src = hbm(frames, off=src_off, guard=0xA5)
            dst = src if dst_off is None else hbm(np.full(frames.size, 0x3C, dtype=np.uint8), off=dst_off, guard=0xC3)
            side = [hbm(x) for x in (b, counts, list_off, np.zeros(5 * n, np.int32), np.zeros(F, np.int32), np.zeros(4 * F, np.int32))]
            p = LaunchRec(src.ptr, dst.ptr, R.frame_bytes(W, H, fmt), F, W, H, fmt, 0, side[0].ptr, side[1].ptr, side[2].ptr, 0, 1, 1.0, 0.0, 0.0,
                          0, 0, None, None, 0, None, None, mode, cell.bit_length() - 1, (C.c_ubyte * 3)(*FILL_RGB), side[3].ptr, side[4].ptr,
                          side[5].ptr)
            assert L.mhip_redact_select(C.byref(p)) == 0 and L.mhip_redact(C.byref(p)) == 0
            what = "%d x %d fmt %d mode %d cell %d offsets %s %s" % (W, H, fmt, mode, cell, src_off, dst_off)
            same(what, dst.read(what), want)
            if dst is not src:
                src.unchanged(what)
            same(what + ": statistics", side[5].read(what).view(np.int32), wst.view(np.int32))
            for d in [src, dst] + side:
                d.free()


# ---- the device form: the synthetic DFL + seg twin of tests/test_gpu_yolo_seg.py at its smallest size ------------------------------------------
S, NM, B = 64, 4, 3
FW, FH = 100, 56  # the camera frames the detections are mapped into, and the native mask grid


class Twin:
    def __init__(self, gpu):
        self.gpu = gpu
        d, heads, self.coefs, self.pr = seg_graph(NM, False, S)
        self.m = gpu.Model(d, batch=B)
        fill(self.m, 0x5E600000 + S, zero_frame=1)
        self.m.run()
        self.bufs = []

    def detect(self, src=(FW, FH), max_per_frame=2, native=None):
        kw = dict(DFL_KW, src=src)
        return self.m.detect_seg_native(self.gpu.seg_opts(self.coefs, self.pr, max_per_frame=max_per_frame), native, **kw)

    def upload(self, frames):
        self.bufs.append(self.gpu.DeviceBuffer(frames))
        return self.bufs[-1]

    def close(self):
        self.m.close()
        for x in self.bufs:
            x.free()


def dev_read(buf):
    out = np.empty(buf.size, dtype=np.uint8)
    assert buf._hip.hipMemcpy(C.c_void_p(out.ctypes.data), C.c_void_p(buf.ptr), C.c_size_t(buf.size), 2) == 0  # hipMemcpyDeviceToHost
    return out


@pytest.fixture(scope="module")
def twin(gpu):
    t = Twin(gpu)
    yield t
    t.close()


def expected_device(frames, W, H, fmt, dets, mode, cell, masks_of=None, idents=None, **sel):
    """the restatement over fetched detections: masks_of = (records, words) of the native masks or None -> (frames, stats, unions)"""
    expand = sel.pop("expand", 0.0)
    out = np.empty_like(frames)
    stats = np.zeros(len(frames), dtype=R.STATS)
    unions = []
    for f in range(len(frames)):
        keep = R.select_np(dets[f], idents=None if idents is None else idents[f], **sel)
        masks = None
        if masks_of is not None:
            recs, words = masks_of
            slot = {int(r["det"]): j for j, r in enumerate(recs[f]) if r["det"] >= 0}
            masks = [R.unpack_words(words[f][slot[i]], W) if i in slot else None for i in keep]
        U, st = R.union_np(dets[f][np.array(keep, dtype=np.int64)], W, H, expand, masks)
        out[f] = R.redact_frame_np(frames[f], W, H, fmt, U, mode, cell, FILL_RGB)
        stats[f] = st
        unions.append(U)
    return out, stats, unions


def pick_expand(frames, W, H, fmt, dets, mode, cell, start=1.5, **kw):
    """the twin's boxes are many and large: at expand 1 they cover whole frames.  -> the largest expand <= start, of a fixed list, at which the
    RESTATEMENT's union is not vacuous, with the restatement's results at it (the choice looks at nothing the device computed)"""
    for e in (1.5, 1.0, 0.6, 0.35, 0.2, 0.1, 0.05, 0.02):
        if e <= start:
            want, wst, unions = expected_device(frames, W, H, fmt, dets, mode, cell, expand=e, **kw)
            if not_vacuous(unions, wst, W, H, cell):
                return e, want, wst
    raise AssertionError("no expand leaves a partly redacted cell")


def run_device(t, frames, opts, out_of_place=False):
    buf = t.upload(frames)
    dst = t.upload(np.zeros_like(frames)) if out_of_place else None
    t.m.redact_device(buf.ptr, opts, dst.ptr if dst else None)
    st = t.m.redact_results()
    assert t.m.redact_ms() >= 0
    if out_of_place:
        assert np.array_equal(dev_read(buf), frames.reshape(-1))
    return dev_read(dst or buf).reshape(frames.shape), st


@pytest.mark.parametrize("fmt", [R.RGB, R.NV12])
def test_device_selection_and_masks(gpu, twin, fmt):
    rng = np.random.default_rng(77 + fmt)
    frames = frames_of(rng, B, FW, FH, fmt)
    dets, recs, words, ow = twin.detect(max_per_frame=2)
    assert ow == FW and words.shape[2] == FH and len(dets[0]) > 3 and len(dets[1]) == 0
    confs = np.unique(np.concatenate([d["conf"] for d in dets]))  # table values: a few levels, many ties
    assert len(confs) >= 2
    classes = np.concatenate([d["cls"] for d in dets])
    cls0 = int(np.bincount(classes).argmax())
    cases_ = [
        (dict(), 1.0, False, R.MOSAIC, 2, False),
        (dict(min_conf=float(confs[len(confs) // 2])), 1.0, False, R.MOSAIC, 8, True),  # not the lowest level
        (dict(classes=(cls0, 1)), 0.6, False, R.FILL, 16, False),
        (dict(), 1.0, True, R.MOSAIC, 4, False),
        (dict(min_conf=float(confs[1])), 1.5, True, R.FILL, 2, True),
    ]
    for sel, start, use_masks, mode, cell, oop in cases_:
        masks_of = (recs, words) if use_masks else None
        e, want, wst = pick_expand(frames, FW, FH, fmt, dets, mode, cell, start, masks_of=masks_of, **sel)
        got, st = run_device(twin, frames, gpu_opts(gpu, FW, FH, fmt, mode, cell, use_masks=use_masks, expand=e, **sel), oop)
        assert st.tobytes() == wst.tobytes(), (sel, e, st, wst)
        same("device form %s expand %g" % (sel, e), got, want)
        n_sel = wst["regions"].sum() + wst["skipped"].sum()
        if sel:
            assert 0 < n_sel < sum(len(d) for d in dets), sel
        if use_masks:  # two slots a frame: some regions are masks, the others fall back to their rectangles
            assert wst["masked"].sum() >= 2 and wst["regions"].sum() > wst["masked"].sum(), wst
        else:
            assert not wst["masked"].any()
    # the host-memory form: in place on the caller's bytes
    e, want, wst = pick_expand(frames, FW, FH, fmt, dets, R.MOSAIC, 8)
    got, st = twin.m.redact(frames, gpu_opts(gpu, FW, FH, fmt, R.MOSAIC, 8, expand=e))
    assert st.tobytes() == wst.tobytes()
    same("mars_hip_redact", got, want)


def test_device_repeat_with_another_frame_size(gpu, twin):
    """two consecutive calls with different frame sizes on one model: the results are the second call's"""
    rng = np.random.default_rng(5)
    for W, H in ((FW, FH), (66, 40), (FW, FH)):
        frames = frames_of(rng, B, W, H, R.RGB)
        dets = twin.detect(src=(W, H))[0]
        e, want, wst = pick_expand(frames, W, H, R.RGB, dets, R.MOSAIC, 4)
        got, st = run_device(twin, frames, gpu_opts(gpu, W, H, R.RGB, R.MOSAIC, 4, expand=e))
        assert st.tobytes() == wst.tobytes()
        same("%d x %d" % (W, H), got, want)


def test_device_refusals(gpu, twin):
    FILE, TENSOR = gpu.MARS_ERR_INVALID_FILE, gpu.MARS_ERR_INVALID_TENSOR
    frames = frames_of(np.random.default_rng(1), B, FW, FH, R.RGB)
    buf = twin.upload(frames)
    twin.detect(native=gpu.mask_native_opts(77, 43))  # the mask grid is not the frame
    bad = [(gpu.redact_opts(FW, FH, use_masks=True), None, TENSOR),
           (gpu.redact_opts(FW, FH, spare_identified=True), None, TENSOR),                    # no identity results on the model
           (gpu.redact_opts(FW, FH), buf.ptr + 1, FILE), (gpu.redact_opts(FW, FH), buf.ptr + frames.size - 1, FILE),  # a partial overlap
           (gpu.redact_opts(FW, FH, cell=3), None, FILE), (gpu.redact_opts(9000, FH), None, TENSOR)]
    for o, dst, code in bad:
        with pytest.raises(gpu.MarsError) as e:
            twin.m.redact_device(buf.ptr, o, dst)
        assert e.value.code == code, (o.flags, dst)
    fresh = gpu.Model(seg_graph(NM, False, S)[0], batch=B)
    with pytest.raises(gpu.MarsError) as e:
        fresh.redact_results()  # before any call
    assert e.value.code == TENSOR and fresh.redact_ms() < 0
    with pytest.raises(gpu.MarsError) as e:
        fresh.redact_device(buf.ptr, gpu.redact_opts(FW, FH))  # no detections in HBM
    assert e.value.code == TENSOR
    fresh.pipe_open(download_outputs=False, detect=True, dfl_heads=gpu.yolo_dfl_heads(**DFL_KW))
    with pytest.raises(gpu.MarsError) as e:
        fresh.redact_device(buf.ptr, gpu.redact_opts(FW, FH))  # an open pipe
    assert e.value.code == TENSOR
    fresh.pipe_close()
    fresh.close()
    assert np.array_equal(dev_read(buf), frames.reshape(-1))  # no refused call touched a pixel
    twin.detect()
    twin.m.redact_device(buf.ptr, gpu.redact_opts(FW, FH, use_masks=True))  # and the good configuration passes
    assert twin.m.redact_results()["regions"].sum() > 0


def crop_want(frames_rgb, dets, slots, nhwc):
    kept, dropped = roi_select_np(dets, FW, FH, slots)
    x = np.full((slots, 160 * 160 * 3), -17, dtype=np.int8)
    for k, (f, i, x0, y0, x1, y1) in enumerate(kept):
        x[k] = roi_crop_np(frames_rgb[f].reshape(FH, FW, 3), (x0, y0, x1, y1), 160, 160, nhwc)
    return x


def test_ordering_against_crops_and_sparing_the_identified(gpu, twin):
    """crop -> redact in place -> crop into a second destination, nothing waiting in between: the first crops are those of the original
    frames, the second those of the redacted ones.  Then the identities of the first destination's crops, matched against a synthetic
    gallery, spare some detections and not others"""
    d2, tin, tout, nhwc = second_stage(gpu, "shipped")
    first, second = gpu.Model(d2, batch=4), gpu.Model(d2, batch=4)
    frames = frames_of(np.random.default_rng(9), B, FW, FH, R.RGB)
    buf = twin.upload(frames)
    dets = twin.detect()[0]
    assert sum(len(d) for d in dets) > 4
    ro = gpu.roi_opts(FW, FH)
    e, red, wst = pick_expand(frames, FW, FH, R.RGB, dets, R.MOSAIC, 8)
    opts = gpu_opts(gpu, FW, FH, R.RGB, R.MOSAIC, 8, expand=e)
    first.crop_detections(twin.m, buf.ptr, ro, device=True)
    twin.m.redact_device(buf.ptr, opts)
    second.crop_detections(twin.m, buf.ptr, ro, device=True)
    for model, src, what in ((first, frames, "crops enqueued before the redaction"), (second, red, "crops enqueued behind it")):
        assert len(model.roi_results()[0]) == 4  # (waits)
        want = crop_want(src, dets, 4, nhwc)
        for k in range(4):
            same("%s, slot %d" % (what, k), model.read_tensor(tin, frame=k)[:want[k].size].view(np.int8), want[k])
    assert not np.array_equal(crop_want(frames, dets, 4, nhwc), crop_want(red, dets, 4, nhwc))
    same("the frames", dev_read(buf).reshape(frames.shape), red)
    assert twin.m.redact_results().tobytes() == wst.tobytes()
    # identities: the four cropped detections get one, the others none
    from test_gpu_gallery import gallery_of, vectors
    g, ids = gallery_of(gpu, vectors(0x6A190000, 50, 64, shift=9) + 40000, ids=np.arange(50) + 1000)
    buf2 = twin.upload(frames)
    first.crop_detections(twin.m, buf2.ptr, ro, device=True)
    first.run_device(sync=False)
    first.classify_device(top_k=3)
    first.match_device(g, top_k=3)
    twin.m.identify_detections(first)
    idents = twin.m.identity_results()
    known = [idents[f, :len(dets[f])] for f in range(B)]
    scores = np.sort(np.concatenate([k["score"][k["cls"] >= 0] for k in known]))
    assert len(scores) == 4 and sum((k["cls"] < 0).sum() for k in known) >= 1
    for ident_min in (0.0, float(scores[2]) if scores[2] > scores[1] else float(scores[-1])):
        e, want, wst = pick_expand(frames, FW, FH, R.RGB, dets, R.FILL, 4, idents=known, ident_min=ident_min)
        o = gpu_opts(gpu, FW, FH, R.RGB, R.FILL, 4, spare_identified=True, ident_min=ident_min, expand=e)
        b3 = twin.upload(frames)
        twin.m.redact_device(b3.ptr, o)
        st = twin.m.redact_results()
        assert st.tobytes() == wst.tobytes(), (ident_min, st, wst)
        same("sparing the identified, ident_min %g" % ident_min, dev_read(b3).reshape(frames.shape), want)
        spared = sum(len(d) for d in dets) - wst["regions"].sum() - wst["skipped"].sum()
        assert 0 < spared <= 4 and wst["regions"].sum() > 0, (ident_min, spared)
    g.close()
    first.close()
    second.close()
