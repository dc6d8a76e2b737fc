"""The overlay on the device (mars_yolo_overlay_frames, mars_hip_overlay_device, mars_hip_overlay), byte for byte and count for count against
the restatement of include/mars_hip.h "Overlay" (tests/overlayref.py, pinned by tests/test_overlay_cpu.py, which also runs the case
generators below through the restatement and asserts that no case is vacuous).  There is no tolerance anywhere."""
import ctypes as C

import numpy as np
import pytest

import overlayref as O
from test_gpu_move import Dev, hbm, same  # noqa: F401  (hbm: the fixture of guarded allocations)

pytestmark = pytest.mark.gpu

DET = np.dtype([("x", "<f4"), ("y", "<f4"), ("w", "<f4"), ("h", "<f4"), ("conf", "<f4"), ("cls", "<i4")])  # mars_det_t
KPT = np.dtype([("x", "<f4"), ("y", "<f4"), ("v", "<f4")])                                                  # mars_kpt_t
RGB_SIZES = [(31, 17), (33, 45), (65, 66), (80, 70), (257, 130)]  # rows that are no multiple of 4 or 16 bytes, a one-pixel last tile, 2 x 2 and 5 x 3 tiles
NV12_SIZES = [(32, 18), (66, 34), (66, 130), (128, 66)]
ALL = O.MASKS | O.BOXES | O.KEYPOINTS | O.LABELS
K = 5
NO_KEY = (9, 200, 77)
# (layers, the other options): each layer alone, all together at the defaults, the smallest and the largest of every size with P = 1 and P = 256
CONFIGS = [(O.MASKS, {}), (O.BOXES, {}), (O.KEYPOINTS, {}), (O.LABELS, {}), (ALL, {}),
           (ALL, dict(scale=1, thickness=1, radius=1, alpha=1, palette=1, color_by=O.FIXED)),
           (ALL, dict(scale=8, thickness=16, radius=8, alpha=256, palette=256, text=O.TEXT_CLASS, names=True))]
NAMES = ["person", "a name of 16 by.", "", "car", "Dog~{", "\x7f\x01"]  # exactly NAME_LEN bytes; empty: the number shows; bytes outside the font


# ---- the cases (functions of their arguments alone: tests/test_overlay_cpu.py runs them through the restatement without a device) -----------
def host_case(seed, W, H, fmt):
    """F frames (the last one without a box: its tiles meet no element), boxes of which two overlap around the centre (outlines, tints, labels
    and markers of one layer on the same pixels; wherever the frame allows it they span two mask words and a tile border), one in the top
    left corner (its label flips inside), one on the right edge (its label is cut there), one across the tile corner (64, 64) where there
    is one, two that the rectangle rule skips, and random ones; masks for the first two and some others; keypoints for the first two: on a
    tile border, cut at the frame's corner, dropped ones.  -> dict"""
    rng = np.random.default_rng(seed)
    F = 2 if W >= 257 else 3
    cx, cy, bw, bh = W * 0.5, H * 0.55, max(W * 0.45, 6.0), max(H * 0.4, 6.0)
    nan = float("nan")
    rows = [(cx, cy, bw, bh, 0.91, 1, 0), (cx + 3, cy + 2, bw, bh, 0.805, 2, 0), (3.0, 2.5, 8, 6, 0.7, 3, 0), (W - 3.0, H * 0.5, 8, 8, 0.005, 4, 0),
            (nan, 5, 4, 4, 0.5, 0, 0), (10, 10, 0, 4, 0.5, 0, 0), (64.0, 64.0, 11, 9, 0.995, 5, 0), (W * 0.5, H * 0.5, W * 2.0, H * 2.0, 1.0, -3, F - 2)]
    for _ in range(6):
        rows.append((rng.uniform(0, W), rng.uniform(0, H), rng.uniform(2, W * 0.4), rng.uniform(2, H * 0.4), rng.uniform(0, 1), int(rng.integers(0, 300)),
                     int(rng.integers(0, F - 1))))
    boxes = np.array([r[:6] for r in rows], dtype=DET)
    fo = np.array([r[6] for r in rows], dtype=np.int32)
    n = len(rows)
    pitch = (W + 31) // 32
    mw = rng.integers(0, 1 << 32, (4, H, pitch), dtype=np.uint64).astype(np.uint32)  # bits outside every rectangle and in the padding included
    mo = np.full(n, -1, dtype=np.int32)
    mo[[0, 1, 7, 9]] = (0, 1, 3, 1)  # a repeat; the whole-frame box has one
    kp = np.zeros((n, K), dtype=KPT)  # v = 0: none
    kp[0] = [(cx, cy, 0.9), (64.5, min(cy, H - 1.0), 0.5), (-0.5, -0.2, 1.0), (W + 20.0, 3, 1.0), (nan, 3, 1.0)]
    kp[1] = [(cx + 1, cy + 1, 0.9), (W - 0.5, H - 0.5, 0.7), (W + 8.5, H + 8.0, 0.6), (5, 5, 0.49), (-9.5, 4, 1.0)]
    kp[8] = [(rng.uniform(0, W), rng.uniform(0, H), 1.0) for _ in range(K)]
    keys = rng.integers(-2, 600, n).astype(np.int32)
    texts = ["", "ab", "LONGER than 24 bytes, it is cut", "~{|}`", "\x80\xff", "x"] + ["%d!" % i for i in range(n - 6)]
    frames = rng.integers(0, 256, (F, O.frame_bytes(W, H, fmt)), dtype=np.uint8)
    return dict(F=F, W=W, H=H, fmt=fmt, frames=frames, boxes=boxes, fo=fo, mw=mw, mo=mo, kp=kp, keys=keys, texts=texts)


def config_kw(rng_seed, kw):
    """CONFIGS' shorthand -> the keywords overlay_opts and the restatement both take (palette: a count -> random colours; names: the table)"""
    kw = dict(kw)
    if "palette" in kw:
        kw["palette"] = np.random.default_rng(rng_seed).integers(0, 256, (kw["palette"], 3), dtype=np.uint8)
    if kw.get("names"):
        kw["names"] = names_table()
    return kw


def names_table():
    t = np.zeros((len(NAMES), O.NAME_LEN), dtype=np.uint8)
    for i, s in enumerate(NAMES):
        b = s.encode("latin-1")
        t[i, :len(b)] = np.frombuffer(b, dtype=np.uint8)
    return t


def text_rows(texts):
    t = np.zeros((len(texts), O.TEXT_MAX), dtype=np.uint8)
    for i, s in enumerate(texts):
        b = s.encode("latin-1")[:O.TEXT_MAX]
        t[i, :len(b)] = np.frombuffer(b, dtype=np.uint8)
    return t


def want_host(c, layers, kw, flags=0, own=False):
    """the restatement on a host case; own: the caller's keys and texts instead of the composed ones"""
    return O.overlay_frames_np(c["frames"], c["boxes"], c["fo"], c["W"], c["H"], c["fmt"], keys=c["keys"] if own else None,
                               texts=text_rows(c["texts"]) if own else None, mask_words=c["mw"], mask_of_box=c["mo"], kpts=c["kp"], layers=layers,
                               no_key=NO_KEY, src_flags=flags, **kw)


def all_host_cases():
    """(id, case, layers, keywords, NV12 flags, own) of every host-form run below"""
    for fmt, sizes in ((O.RGB, RGB_SIZES), (O.NV12, NV12_SIZES)):
        for W, H in sizes:
            c = host_case(W * 1000 + H + fmt, W, H, fmt)
            for k, (layers, kw) in enumerate(CONFIGS):
                flags = (0, O.NV12_VU, O.NV12_FULL_RANGE, O.NV12_VU | O.NV12_FULL_RANGE)[k % 4] if fmt else 0
                yield "%dx%d fmt %d config %d" % (W, H, fmt, k), c, layers, config_kw(k, kw), flags, k == 5


# ---- the host-pointer form -------------------------------------------------------------------------------------------------------------------
def run_host(gpu, c, layers, kw, flags, own, inplace):
    o = gpu.overlay_opts(c["W"], c["H"], fmt=c["fmt"], src_flags=flags, layers=layers, no_key=NO_KEY, **kw)
    return gpu.overlay_frames(c["frames"], c["boxes"], c["fo"], o, keys=c["keys"] if own else None, texts=c["texts"] if own else None,
                              mask_words=c["mw"], mask_of_box=c["mo"], kpts=c["kp"], inplace=inplace)


@pytest.mark.parametrize("fmt, W, H", [(O.RGB,) + s for s in RGB_SIZES] + [(O.NV12,) + s for s in NV12_SIZES])
def test_host_pointer_form(gpu, fmt, W, H):
    """every configuration, out of place and in place: the same bytes, the restatement's"""
    O.bind(gpu)
    for what, c, layers, kw, flags, own in all_host_cases():
        if (c["fmt"], c["W"], c["H"]) != (fmt, W, H):
            continue
        want, wst, infos = want_host(c, layers, kw, flags, own)
        assert not O.not_vacuous(infos, layers, W, H), what
        for inplace in (False, True):
            got, st = run_host(gpu, c, layers, kw, flags, own, inplace)
            assert st.tobytes() == wst.tobytes(), (what, inplace, st, wst)
            same("%s in place %d" % (what, inplace), got, want)
        assert np.array_equal(want[-1], c["frames"][-1]) and not np.array_equal(want[0], c["frames"][0])  # the frame without a box


def test_every_box_skipped_leaves_the_frames_alone(gpu):
    O.bind(gpu)
    nan = float("nan")
    for fmt, W, H in ((O.RGB, 65, 66), (O.NV12, 66, 130)):
        frames = np.random.default_rng(W).integers(0, 256, (3, O.frame_bytes(W, H, fmt)), dtype=np.uint8)
        b = np.array([(nan, 5, 4, 4, 0.5, 0), (10, 10, 0, 4, 0.5, 0), (10, 10, 4, -1, 0.5, 0), (W + 40, 10, 8, 8, 0.5, 0), (10, -30, 8, 8, 0.5, 0),
                      (10, 10, 4, 4, nan, 0), (10, 10, float("inf"), 4, 0.5, 0)], dtype=DET)
        fo = np.array([0, 1, 2, 0, 1, 2, 0], dtype=np.int32)
        kp = np.zeros((7, K), dtype=KPT)
        kp["x"], kp["y"], kp["v"] = 5, 5, 1  # the keypoints of a skipped box paint nothing
        o = gpu.overlay_opts(W, H, fmt=fmt, layers=ALL)
        for inplace in (False, True):
            got, st = gpu.overlay_frames(frames, b, fo, o, kpts=kp, inplace=inplace)
            assert np.array_equal(got, frames) and st["skipped"].tolist() == [3, 2, 2]
            assert not any(st[k].any() for k in ("boxes", "masked", "labels", "markers", "pixels"))
        got, st = gpu.overlay_frames(frames, b[:1], np.array([7], dtype=np.int32), o)  # a frame index that names no frame: the box is left out
        assert np.array_equal(got, frames) and not st.view(np.int32).any()
        got, st = gpu.overlay_frames(frames, b[:0], fo[:0], o)  # no box at all
        assert np.array_equal(got, frames) and not st.view(np.int32).any()


# ---- the launchers on guarded memory ---------------------------------------------------------------------------------------------------------
class LaunchRec(C.Structure):  # mhip_overlay_t of csrc/mhip.h
    _fields_ = [("frames", C.c_void_p), ("dst", C.c_void_p), ("frame_stride", C.c_size_t), ("n_frames", C.c_int), ("w", C.c_int), ("h", C.c_int),
                ("fmt", C.c_int), ("dets", C.c_void_p), ("counts", C.c_void_p), ("list_off", C.c_void_p), ("det_cap", C.c_int), ("select_all", C.c_int),
                ("min_conf", C.c_float), ("cls_first", C.c_int), ("cls_count", C.c_int), ("tracks", C.c_void_p), ("tracked_only", C.c_int),
                ("min_hits", C.c_int), ("color_by", C.c_int), ("keys", C.c_void_p), ("text", C.c_uint), ("texts", C.c_void_p), ("names", C.c_void_p),
                ("n_names", C.c_int), ("mask_recs", C.c_void_p), ("mask_max", C.c_int), ("mask_of", C.c_void_p), ("mask_words", C.c_void_p),
                ("pose_recs", C.c_void_p), ("pose_max", C.c_int), ("kpt_rows", C.c_int), ("kpts", C.c_void_p), ("num_kpt", C.c_int),
                ("kpt_min_v", C.c_float), ("layers", C.c_uint), ("thick", C.c_int), ("radius", C.c_int), ("scale", C.c_int), ("alpha", C.c_int),
                ("palette", C.c_void_p), ("n_palette", C.c_int), ("no_key", C.c_uint32), ("text_col", C.c_uint32 * 2), ("table", C.c_void_p),
                ("table_n", C.c_void_p), ("marks", C.c_void_p), ("mark_stride", C.c_size_t), ("marks_n", C.c_void_p), ("stats", C.c_void_p)]


def packed(rgb, fmt, flags=0):
    c = O.rgb_to_yuv_np(rgb, flags) if fmt else tuple(int(v) for v in rgb)
    return c[0] | c[1] << 8 | c[2] << 16 | int(O.text_white(rgb)) << 24


@pytest.mark.parametrize("fmt, W, H", [(O.RGB, 80, 70), (O.RGB, 65, 66), (O.NV12, 128, 66), (O.NV12, 66, 130)])
def test_guard_bands_and_every_alignment(hbm, gpu, fmt, W, H):
    """the launchers themselves on guarded allocations ([256 guard bytes][frames][256 guard bytes], tests/test_gpu_move.py) at every source
    and destination alignment 0 .. 3: in place the guards around the frames stay untouched, out of place those of the destination, of
    which every byte is written, and the source stays as it was"""
    O.bind(gpu)
    L = hbm.L
    for fn in (L.mhip_overlay_select, L.mhip_overlay):
        fn.restype, fn.argtypes = C.c_int, [C.POINTER(LaunchRec)]
    c = host_case(W + fmt, W, H, fmt)
    order = np.argsort(c["fo"], kind="stable")
    b, fo, mo, kp = c["boxes"][order], c["fo"][order], c["mo"][order], c["kp"][order]
    F, n, frames = c["F"], len(b), c["frames"]
    counts = np.bincount(fo, minlength=F).astype(np.int32)
    list_off = (np.cumsum(counts) - counts).astype(np.int32)
    want, wst, infos = O.overlay_frames_np(frames, b, fo, W, H, fmt, mask_words=c["mw"], mask_of_box=mo, kpts=kp, layers=ALL, no_key=NO_KEY)
    assert not O.not_vacuous(infos, ALL, W, H)
    pal = np.array([packed(rgb, fmt) for rgb in O.PALETTE], dtype=np.uint32)
    for src_off, dst_off in ((0, None), (1, None), (2, None), (3, None), (0, 0), (0, 16), (1, 1), (2, 2), (3, 3), (5, 1), (0, 3), (3, 0), (2, 1)):
        src = hbm(frames, off=src_off, guard=0xA5)
        dst = src if dst_off is None else hbm(np.full(frames.size, 0x3C, dtype=np.uint8), off=dst_off, guard=0xC3)
        side = [hbm(x) for x in (b, counts, list_off, mo, kp, c["mw"], pal, np.zeros(12 * n, np.int32), np.zeros(F, np.int32),
                                 np.zeros(4 * n * K, np.int32), np.zeros(F, np.int32), np.zeros(6 * F, np.int32))]
        p = LaunchRec(frames=src.ptr, dst=dst.ptr, frame_stride=O.frame_bytes(W, H, fmt), n_frames=F, w=W, h=H, fmt=fmt, dets=side[0].ptr,
                      counts=side[1].ptr, list_off=side[2].ptr, select_all=1, min_hits=1, text=5, mask_of=side[3].ptr, mask_words=side[5].ptr,
                      kpt_rows=1, kpts=side[4].ptr, num_kpt=K, kpt_min_v=0.5, layers=ALL, thick=2, radius=2, scale=2, alpha=96, palette=side[6].ptr,
                      n_palette=16, no_key=packed(NO_KEY, fmt), text_col=(C.c_uint32 * 2)(packed((0, 0, 0), fmt), packed((255, 255, 255), fmt)),
                      table=side[7].ptr, table_n=side[8].ptr, marks=side[9].ptr, marks_n=side[10].ptr, stats=side[11].ptr)
        assert L.mhip_overlay_select(C.byref(p)) == 0 and L.mhip_overlay(C.byref(p)) == 0
        what = "%d x %d fmt %d offsets %s %s" % (W, H, fmt, src_off, dst_off)
        same(what, dst.read(what), want)
        if dst is not src:
            src.unchanged(what)
        same(what + ": statistics", side[11].read(what).view(np.int32), wst.view(np.int32))
        for d in side[:7]:
            d.unchanged(what)
        for d in side[7:]:
            d.read(what)  # their guards
        for d in [src, dst] + side:
            d.free()


# ---- the device form: a synthetic graph with DFL, seg and pose heads (tests/test_gpu_pose.py) at its smallest size ----------------------------
S, NM, B = 64, 4, 3
FW, FH = 100, 56  # the camera frames the detections are mapped into, the native mask grid and the keypoints' pixels


class Twin:
    def __init__(self, gpu):
        from test_gpu_pose import DFL_KW, GRAPH_SEED, fill, pose_graph
        self.gpu, self.kw = gpu, DFL_KW
        d, heads, self.kpts, self.coefs, self.pr = pose_graph(K, 3, False, S, nm=NM)
        self.d = d
        self.m = gpu.Model(d, batch=B)
        fill(self.m, GRAPH_SEED + 99, zero_frame=1)
        self.m.run()
        self.trk = gpu.Tracker(B)
        self.bufs = []

    def detect(self, src=(FW, FH), masks=True, pose=True, track=0, native=None):
        """the tails whose results the overlay reads, the pose tail last: -> (dets, mask records, mask words, pose records, keypoints, tracks)"""
        kw = dict(self.kw, src=src)
        g, m = self.gpu, self.m
        recs = words = precs = kp = tracks = None
        if masks:
            m.detect_seg_native_device(g.seg_opts(self.coefs, self.pr, max_per_frame=2), native, **kw)
            recs, words, _ = m.mask_native_results()
        if pose:
            # (keypoint scales that keep the keypoints within a few cells of their detection: the tensors' own throw them off the frame)
            m.detect_pose_device(g.pose_opts(self.kpts, num_kpt=K, max_per_frame=3, kpt_scales=0.004), **kw)
            precs, kp = m.pose_results()
        if not masks and not pose:
            m.detect_dfl_device(**kw)
        dets = m.detect_results()
        if track:  # the tracker takes the upper half of the confidences: some detections get an id and others none
            confs = np.unique(np.concatenate([d["conf"] for d in dets]))
            thr = float(confs[len(confs) // 2])
            for _ in range(track):
                tracks = m.track(self.trk, min_conf=thr)
        return dets, recs, words, precs, kp, tracks

    def upload(self, frames):
        self.bufs.append(self.gpu.DeviceBuffer(frames))
        return self.bufs[-1]

    def close(self):
        self.trk.close()
        self.m.close()
        for x in self.bufs:
            x.free()


@pytest.fixture(scope="module")
def twin(gpu):
    O.bind(gpu)
    t = Twin(gpu)
    yield t
    t.close()


def dev_read(buf):
    out = np.empty(buf.size, dtype=np.uint8)
    assert buf._hip.hipMemcpy(C.c_void_p(out.ctypes.data), C.c_void_p(buf.ptr), C.c_size_t(buf.size), 2) == 0  # hipMemcpyDeviceToHost
    return out


def want_device(frames, W, H, fmt, res, layers, min_conf=0.0, classes=None, tracked_only=False, min_hits=0, flags=0, **kw):
    """the restatement over fetched results: the selection here, then the host form's rule with the slots each detection has"""
    dets, recs, words, precs, kp, tracks = res
    boxes, fo, mo, kps, trs, mws = [], [], [], [], [], []
    for f in range(len(frames)):
        mslot = {} if recs is None else {int(r["det"]): j for j, r in reversed(list(enumerate(recs[f]))) if r["det"] >= 0}
        pslot = {} if precs is None else {int(r["det"]): j for j, r in reversed(list(enumerate(precs[f]))) if r["det"] >= 0}
        for i, d in enumerate(dets[f]):
            if not np.float32(d["conf"]) >= np.float32(min_conf):
                continue
            if classes is not None and classes[1] and not classes[0] <= int(d["cls"]) < classes[0] + classes[1]:
                continue
            if tracked_only and not (tracks[f, i]["id"] >= 0 and tracks[f, i]["hits"] >= (min_hits or 1)):
                continue
            boxes.append(d)
            fo.append(f)
            trs.append(tracks[f, i] if tracks is not None else np.array((-1, 0), dtype=[("id", "<i4"), ("hits", "<i4")]))
            mo.append(-1)
            if layers & O.MASKS and i in mslot:
                mo[-1] = len(mws)
                mws.append(words[f][mslot[i]])
            kps.append(kp[f][pslot[i]] if layers & O.KEYPOINTS and i in pslot else None)
    return O.overlay_frames_np(frames, np.array(boxes, dtype=DET), np.array(fo, dtype=np.int32), W, H, fmt, mask_words=mws or None,
                               mask_of_box=mo if mws else None, kpts=kps, tracks=trs, layers=layers, no_key=NO_KEY, src_flags=flags, **kw)


def run_device(t, frames, opts, out_of_place=False):
    buf = t.upload(frames)
    dst = t.upload(np.zeros_like(frames)) if out_of_place else None
    t.m.overlay_device(buf.ptr, opts, dst.ptr if dst else None)
    st = t.m.overlay_results()
    assert t.m.overlay_ms() >= 0
    if out_of_place:
        assert np.array_equal(dev_read(buf), frames.reshape(-1))
    return dev_read(dst or buf).reshape(frames.shape), st


@pytest.mark.parametrize("fmt", [O.RGB, O.NV12])
def test_device_form_with_masks_tracks_and_keypoints(gpu, twin, fmt):
    rng = np.random.default_rng(31 + fmt)
    frames = rng.integers(0, 256, (B, O.frame_bytes(FW, FH, fmt)), dtype=np.uint8)
    twin.trk.reset()
    res = twin.detect(track=2)  # two steps: hits reach 2
    dets, recs, words, precs, kp, tracks = res
    assert len(dets[0]) > 3 and len(dets[1]) == 0 and (recs["det"] >= 0).any() and (precs["det"] >= 0).any()
    ids = np.concatenate([tracks[f, :len(dets[f])]["id"] for f in range(B)])
    assert (ids >= 0).any() and (ids < 0).any(), "the tracker takes some detections and not others"
    confs = np.unique(np.concatenate([d["conf"] for d in dets]))
    pf = int(np.flatnonzero((precs["det"] >= 0).any(axis=1))[0])
    cls0 = int(dets[pf][precs[pf][precs[pf]["det"] >= 0][0]["det"]]["cls"])  # the class of a detection that has keypoints
    names = names_table()
    flags = gpu.NV12_VU if fmt else 0
    cases = [(ALL, dict(), dict(color_by=O.BY_TRACK, text=7, names=names, kpt_min_v=1e-6), False),  # (every visibility: the graph's are low)
             (ALL, dict(tracked_only=True, min_hits=2), dict(text=O.TEXT_TRACK, scale=1), True),
             (O.BOXES | O.LABELS, dict(min_conf=float(confs[len(confs) // 2])), dict(), True),
             (O.MASKS | O.KEYPOINTS, dict(classes=(cls0, 1)), dict(radius=3, alpha=200, kpt_min_v=1e-6), False),
             (0, dict(), dict(thickness=1), False)]
    for layers, sel, kw, oop in cases:
        want, wst, infos = want_device(frames, FW, FH, fmt, res, layers or (O.BOXES | O.LABELS), flags=flags, **sel, **kw)
        got, st = run_device(twin, frames, gpu.overlay_opts(FW, FH, fmt=fmt, src_flags=flags, layers=layers, no_key=NO_KEY, **sel, **kw), oop)
        assert st.tobytes() == wst.tobytes(), (layers, sel, st, wst)
        same("device form %s %s" % (layers, sel), got, want)
        assert wst["boxes"].sum() > 0 and wst["pixels"].sum() > 0 and np.array_equal(got[1], frames[1])  # frame 1 has no detection
        if sel:
            assert wst["boxes"].sum() + wst["skipped"].sum() < sum(len(d) for d in dets), sel
        if layers & O.MASKS and not sel:  # two mask slots a frame: some elements are tinted and others not
            assert wst["masked"].sum() > 0 and wst["boxes"].sum() > wst["masked"].sum()
        if layers & O.KEYPOINTS and not sel:
            assert wst["markers"].sum() > 0
    # the host-memory form: in place on the caller's bytes
    want, wst, _ = want_device(frames, FW, FH, fmt, res, O.BOXES | O.LABELS, flags=flags)
    got, st = twin.m.overlay(frames, gpu.overlay_opts(FW, FH, fmt=fmt, src_flags=flags, no_key=NO_KEY))
    assert st.tobytes() == wst.tobytes()
    same("mars_hip_overlay", got, want)


def test_device_repeat_with_another_frame_size(gpu, twin):
    """consecutive calls with different frame sizes, palettes and names on one model: the results are the last call's"""
    rng = np.random.default_rng(5)
    for k, (W, H) in enumerate(((FW, FH), (66, 40), (FW, FH))):
        frames = rng.integers(0, 256, (B, O.frame_bytes(W, H, O.RGB)), dtype=np.uint8)
        res = twin.detect(src=(W, H))
        kw = dict(palette=rng.integers(0, 256, (3 + k, 3), dtype=np.uint8), names=names_table()[:k + 1])
        want, wst, _ = want_device(frames, W, H, O.RGB, res, ALL, **kw)
        got, st = run_device(twin, frames, gpu.overlay_opts(W, H, layers=ALL, no_key=NO_KEY, **kw))
        assert st.tobytes() == wst.tobytes()
        same("%d x %d" % (W, H), got, want)


def test_device_refusals(gpu, twin):
    FILE, TENSOR = gpu.MARS_ERR_INVALID_FILE, gpu.MARS_ERR_INVALID_TENSOR
    frames = np.random.default_rng(1).integers(0, 256, (B, O.frame_bytes(FW, FH, O.RGB)), dtype=np.uint8)
    buf = twin.upload(frames)
    from test_gpu_pose import pose_graph
    fresh = gpu.Model(pose_graph(K, 3, False, S, nm=NM)[0], batch=B)
    with pytest.raises(gpu.MarsError) as e:
        fresh.overlay_results()  # before any call
    assert e.value.code == TENSOR and fresh.overlay_ms() < 0
    with pytest.raises(gpu.MarsError) as e:
        fresh.overlay_device(buf.ptr, gpu.overlay_opts(FW, FH))  # no detections in HBM
    assert e.value.code == TENSOR
    fresh.close()
    twin.detect()
    good = gpu.overlay_opts(FW, FH, layers=ALL)
    twin.m.overlay_device(buf.ptr, good)
    st0 = twin.m.overlay_results()
    painted = dev_read(buf)
    assert st0["pixels"].sum() > 0
    twin2 = Twin(gpu)  # a model with detections but no masks, keypoints or tracks of this batch
    twin2.detect(masks=False, pose=False)
    for o in (gpu.overlay_opts(FW, FH, layers=O.MASKS), gpu.overlay_opts(FW, FH, layers=O.KEYPOINTS), gpu.overlay_opts(FW, FH, tracked_only=True),
              gpu.overlay_opts(FW, FH, color_by=O.BY_TRACK), gpu.overlay_opts(FW, FH, text=O.TEXT_TRACK)):
        with pytest.raises(gpu.MarsError) as e:
            twin2.m.overlay_device(buf.ptr, o)
        assert e.value.code == TENSOR, (o.layers, o.flags, o.color_by, o.text)
    twin2.m.overlay_device(buf.ptr, gpu.overlay_opts(FW, FH, layers=O.BOXES, text=O.TEXT_TRACK))  # the text is not asked for without LABELS
    twin2.m.overlay_results()
    twin2.m.pipe_open(download_outputs=False, detect=True, dfl_heads=gpu.yolo_dfl_heads(**twin2.kw))
    with pytest.raises(gpu.MarsError) as e:
        twin2.m.overlay_device(buf.ptr, gpu.overlay_opts(FW, FH))  # an open pipe
    assert e.value.code == TENSOR
    twin2.m.pipe_close()
    twin2.close()
    buf = twin.upload(frames)
    twin.detect(native=gpu.mask_native_opts(77, 43))  # the mask grid is not the frame
    bad = [(gpu.overlay_opts(FW, FH, layers=O.MASKS), None, TENSOR), (gpu.overlay_opts(9000, FH), None, TENSOR),
           (good, buf.ptr + 1, FILE), (good, buf.ptr + frames.size - 1, FILE),  # a partial overlap
           (gpu.overlay_opts(FW, FH, layers=16), None, FILE), (gpu.overlay_opts(FW, FH, text=8), None, FILE), (gpu.overlay_opts(FW, FH, flags=2), None, FILE),
           (gpu.overlay_opts(FW, FH, color_by=3), None, FILE), (gpu.overlay_opts(FW, FH, thickness=17), None, FILE),
           (gpu.overlay_opts(FW, FH, radius=9), None, FILE), (gpu.overlay_opts(FW, FH, scale=9), None, FILE), (gpu.overlay_opts(FW, FH, alpha=257), None, FILE),
           (gpu.overlay_opts(FW, FH, scale=-1), None, FILE), (gpu.overlay_opts(FW, FH, min_conf=float("nan")), None, FILE),
           (gpu.overlay_opts(FW, FH, kpt_min_v=-1.0), None, FILE), (gpu.overlay_opts(FW, FH, min_hits=-1), None, FILE),
           (gpu.overlay_opts(FW, FH, palette=np.zeros((257, 3), np.uint8)), None, FILE), (gpu.overlay_opts(FW + 1, FH, fmt=O.NV12), None, FILE),
           (gpu.overlay_opts(FW, FH, src_flags=1), None, FILE), (gpu.overlay_opts(0, FH), None, FILE)]
    o = gpu.overlay_opts(FW, FH)
    o.n_palette = 4  # a count without a table
    bad.append((o, None, FILE))
    for o, dst, code in bad:
        with pytest.raises(gpu.MarsError) as e:
            twin.m.overlay_device(buf.ptr, o, dst)
        assert e.value.code == code, (o.layers, o.text, o.flags, dst)
    assert np.array_equal(dev_read(buf), frames.reshape(-1))  # no refused call touched a pixel
    assert twin.m.overlay_results().tobytes() == st0.tobytes()  # and the state is that of the last good call
    twin.detect()
    twin.m.overlay_device(buf.ptr, good)  # and the good configuration passes again
    assert twin.m.overlay_results().tobytes() == st0.tobytes() and np.array_equal(dev_read(buf), painted)  # (the results wait)


def test_ordering_against_crops_and_redaction(gpu, twin):
    """crop -> overlay in place -> crop into a second destination, nothing waiting in between: the first crops are those of the original
    frames, the second those of the painted ones.  Then a fill redaction in place and an overlay behind it: the labels lie over the fill"""
    from test_gpu_redact import crop_want
    from test_gpu_roi import second_stage
    import redactref as R
    d2, tin, tout, nhwc = second_stage(gpu, "shipped")
    first, second = gpu.Model(d2, batch=4), gpu.Model(d2, batch=4)
    frames = np.random.default_rng(9).integers(0, 256, (B, O.frame_bytes(FW, FH, O.RGB)), dtype=np.uint8)
    buf = twin.upload(frames)
    res = twin.detect(masks=False, pose=False)
    dets = res[0]
    ro = gpu.roi_opts(FW, FH)
    kw = dict(thickness=3, scale=1)
    want, wst, _ = want_device(frames, FW, FH, O.RGB, res, O.BOXES | O.LABELS, **kw)
    first.crop_detections(twin.m, buf.ptr, ro, device=True)
    twin.m.overlay_device(buf.ptr, gpu.overlay_opts(FW, FH, no_key=NO_KEY, **kw))
    second.crop_detections(twin.m, buf.ptr, ro, device=True)
    for model, src, what in ((first, frames, "crops enqueued before the overlay"), (second, want, "crops enqueued behind it")):
        assert len(model.roi_results()[0]) == 4  # (waits)
        cw = crop_want(src, dets, 4, nhwc)
        for k in range(4):
            same("%s, slot %d" % (what, k), model.read_tensor(tin, frame=k)[:cw[k].size].view(np.int8), cw[k])
    assert not np.array_equal(crop_want(frames, dets, 4, nhwc), crop_want(want, dets, 4, nhwc))
    same("the frames", dev_read(buf).reshape(frames.shape), want)
    assert twin.m.overlay_results().tobytes() == wst.tobytes()
    first.close()
    second.close()
    # redaction, then the overlay, both in place and only enqueued
    fill = (1, 2, 3)
    b2 = twin.upload(frames)
    twin.m.redact_device(b2.ptr, gpu.redact_opts(FW, FH, mode=gpu.REDACT_FILL, fill=fill, expand=0.6))
    twin.m.overlay_device(b2.ptr, gpu.overlay_opts(FW, FH, layers=O.LABELS, no_key=NO_KEY, scale=1))
    red = np.stack([R.redact_frame_np(frames[f], FW, FH, R.RGB, R.union_np(dets[f], FW, FH, 0.6)[0], R.FILL, 0, fill) for f in range(B)])
    want2, wst2, infos = want_device(red, FW, FH, O.RGB, res, O.LABELS, scale=1)
    assert twin.m.overlay_results().tobytes() == wst2.tobytes()  # (waits)
    same("labels over the fill", dev_read(b2).reshape(frames.shape), want2)
    filled = np.stack([R.union_np(dets[f], FW, FH, 0.6)[0] for f in range(B)])
    assert any((i["covered"] & filled[f]).any() for f, i in enumerate(infos)) and not np.array_equal(want2, red)
