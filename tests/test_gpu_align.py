"""Aligned crops on the device (include/mars_hip.h, "Aligned crops"): mars_yolo_crop_aligned, the device chain pose detector -> aligned crops ->
second model, the selection rules, the ROI and fit tables and the label join.  The expected bytes come from the numpy restatement of
tests/alignref.py (checked by hand and against the host fit in tests/test_align_cpu.py); every comparison is bit-exact."""
import numpy as np
import pytest

import alignref
from alignref import FIT_KEYS, align_crop_np, align_fit_np, align_select_np, fit_tuple, kpts
from conftest import lcg_frame
from rotref import nv12_to_rgb_np
from test_gpu_rot import SOURCE_IDS, SOURCES, second_stage, source

pytestmark = pytest.mark.gpu

F = np.float32
FULL, VU = 1, 2
W, H = 98, 62
NAN = float("nan")
MIN_VIS = 0.5  # of every host-pointer call here: a box loses a point by a low visibility


def uniforms(seed, n):
    """n numbers of [0, 1) from the suite's LCG, three bytes each"""
    b = lcg_frame(seed, 3 * n).astype(np.uint8).astype(np.float64).reshape(n, 3)
    return (b[:, 0] * 65536 + b[:, 1] * 256 + b[:, 2]) / 16777216.0


def placed(tmpl, tw, th, cx, cy, scale, ang, noise=None):
    """the template under the similarity (scale, ang) that carries the target's centre to (cx, cy), + noise [K][2] -> [K][2]"""
    d = np.asarray(tmpl, dtype=np.float64) - (tw / 2, th / 2)
    c, s = np.cos(ang) * scale, np.sin(ang) * scale
    xy = np.stack([cx + c * d[:, 0] - s * d[:, 1], cy + s * d[:, 0] + c * d[:, 1]], axis=1)
    return xy if noise is None else xy + noise


_u = uniforms(0xA1160001, 64)
SIMS = [(1.0, 0.0), (1.0, np.pi / 2)] + [(0.4 * 7.5 ** _u[2 * k], 2 * np.pi * _u[2 * k + 1]) for k in range(12)]  # (scale, angle)
CENTRES = [(49, 31),                                       # inside the frame
           (2, 31), (96, 31), (49, 1.5), (49, 60.5),       # over each edge
           (3, 3), (95, 3), (3, 59), (95, 59),             # over each corner
           (0, 0), (98, 62)]                               # exactly on a corner
N_SKIP = 5


def geometry_sets(gpu, tw, th):
    """-> (template [5][2], KPT_DTYPE [n][5]): every centre under every similarity with a little noise, then one box per skip reason a
    keypoint set can show (coincident template points need their own call)"""
    tmpl = gpu.align_template_face5(tw, th)
    n = len(CENTRES) * len(SIMS)
    noise = (uniforms(0xA1160002 + tw, n * 10).reshape(n, 5, 2) - 0.5) * 0.6
    sets = []
    for ci, (cx, cy) in enumerate(CENTRES):
        for si, (scale, ang) in enumerate(SIMS):
            first = si < 2  # the identity and the quarter turn stay noise-free
            sets.append(kpts(placed(tmpl, tw, th, cx, cy, scale, ang, None if first else noise[ci * len(SIMS) + si] * scale)))
    few = kpts(placed(tmpl, tw, th, 49, 31, 1.0, 0.3), v=[1.0, 0.4, 0.2, 0.0, 0.49])
    bad = kpts(placed(tmpl, tw, th, 49, 31, 1.0, 0.3))
    bad[2]["y"] = NAN
    small = kpts(placed(tmpl, tw, th, 49, 31, 1.5 / max(tw, th), 0.3))
    large = kpts(placed(tmpl, tw, th, 49, 31, 40000.0 / min(tw, th), 0.3))
    off = kpts(placed(tmpl, tw, th, -20, 31, 1.0, 0.3))
    return tmpl, np.stack(sets + [few, bad, small, large, off])


def expected_host(rgb, kp, fo, tmpl, tw, th, nhwc=True, **kw):
    """-> (crops [n][tw * th * 3], [(x0, y0, x1, y1)], [fit tuples], [skip reason or None])"""
    crops, rects, fits, whys = [], [], [], []
    for i in range(len(kp)):
        fit, rect, why = align_fit_np(kp[i], tmpl, tw, th, rgb.shape[2], rgb.shape[1], **kw)
        crops.append(align_crop_np(rgb[fo[i]], kp[i], tmpl, tw, th, nhwc, **kw))
        rects.append(rect)
        fits.append(fit_tuple(fit))
        whys.append(why)
    return np.stack(crops), rects, fits, whys


def check_tables(rois, fits, fo, rects, want_fits):
    assert (rois["frame"] == fo).all() and (rois["det"] == -1).all()
    assert [(int(r["x0"]), int(r["y0"]), int(r["x1"]), int(r["y1"])) for r in rois] == rects
    assert [tuple(int(f[k]) for k in FIT_KEYS) for f in fits] == want_fits


@pytest.mark.parametrize("src", SOURCES, ids=SOURCE_IDS)
def test_crop_aligned_geometries(gpu, src):
    kind, flags = src
    raw, rgb = source(kind, flags, W, H, 2)
    fmt = gpu.CAMERA_NV12 if kind == "nv12" else gpu.CAMERA_RGB
    for tw, th in [(32, 32), (40, 24)]:
        tmpl, kp = geometry_sets(gpu, tw, th)
        fo = (np.arange(len(kp)) % 2).astype(np.int32)
        for expand in (0.0, 1.25):
            want, rects, wfits, whys = expected_host(rgb, kp, fo, tmpl, tw, th, min_vis=MIN_VIS, expand=expand)
            # nothing is left out silently: the five skipped boxes are the last five, one per reason; every other box is kept, but for a
            # centre put exactly on a corner: the fitted centre lands a rounding error inside or outside the frame (float32 arithmetic is
            # the same everywhere, so the count is a constant of this test: 9 of 28 at 32 x 32, 5 of 28 at 40 x 24)
            assert whys[-N_SKIP:] == [alignref.FEW, alignref.NOT_FINITE, alignref.SMALL, alignref.LARGE, alignref.OFF_FRAME]
            n_kept = sum(w is None for w in whys)
            on_corner = len(CENTRES[:-2]) * len(SIMS)
            assert all(w is None for w in whys[:on_corner]) and all(w in (None, alignref.OFF_FRAME) for w in whys[on_corner:-N_SKIP])
            assert (n_kept, len(kp) - n_kept) == {(32, 32): (135, 24), (40, 24): (131, 28)}[(tw, th)]
            for nhwc in (1, 0):
                o = gpu.roi_opts(W, H, fmt=fmt, src_flags=flags, expand=expand)
                got, rois, fits = gpu.crop_aligned(raw, kp, fo, gpu.align_opts(tmpl, min_vis=MIN_VIS), o, tw, th, nhwc)
                check_tables(rois, fits, fo, rects, wfits)
                if (tw, th) == (32, 32):  # the device and mars_yolo_align_fit compile one text (csrc/align_fit.h): they compute the same bits too
                    for i in range(len(kp)):
                        kept, hfit, hrect = gpu.align_fit(kp[i], gpu.align_opts(tmpl, min_vis=MIN_VIS), o, tw, th)
                        assert kept == (int(fits[i]["n_used"]) > 0), i
                        assert [int(hfit[k]) for k in FIT_KEYS] == [int(fits[i][k]) for k in FIT_KEYS], i
                        assert hrect == (int(rois[i]["x0"]), int(rois[i]["y0"]), int(rois[i]["x1"]), int(rois[i]["y1"])), i
                assert int((fits["n_used"] > 0).sum()) == n_kept and int((rois["x1"] > rois["x0"]).sum()) == n_kept
                assert int((fits["n_used"] == 0).sum()) == len(kp) - n_kept
                w = want if nhwc else want.reshape(-1, th, tw, 3).transpose(0, 3, 1, 2).reshape(len(kp), -1)
                bad = [i for i in range(len(kp)) if not np.array_equal(got[i], w[i])]
                assert not bad, (tw, th, nhwc, expand, bad[:8], int((got != w).sum()))
                skipped = [i for i, why in enumerate(whys) if why is not None]
                assert (got[skipped] == -17).all() and not (got[0] == -17).all()
                assert all(fit_tuple(fits[i]) == (0,) * 8 and tuple(rois[i])[2:] == (0, 0, 0, 0) for i in skipped)


def test_crop_aligned_coincident_template_points(gpu):
    """D == 0: the mask leaves two template points that coincide; every box is skipped"""
    raw, rgb = source("rgb", 0, W, H, 2)
    tmpl = gpu.align_template_face5(32, 32)
    kp = np.stack([kpts(placed(tmpl, 32, 32, 49, 31, 1.0, a)) for a in (0.0, 0.7)])
    tmpl[1] = tmpl[0]
    fo = np.array([0, 1], dtype=np.int32)
    assert [align_fit_np(k, tmpl, 32, 32, W, H, use=3)[2] for k in kp] == [alignref.DEGENERATE] * 2
    got, rois, fits = gpu.crop_aligned(raw, kp, fo, gpu.align_opts(tmpl, use=3), gpu.roi_opts(W, H), 32, 32)
    assert (got == -17).all() and not fits.tobytes().strip(b"\0") and (rois["x1"] == 0).all() and (rois["frame"] == fo).all()
    got, rois, fits = gpu.crop_aligned(raw, kp, fo, gpu.align_opts(tmpl, use=0b10101), gpu.roi_opts(W, H), 32, 32)  # the same sets under another mask
    want, rects, wfits, whys = expected_host(rgb, kp, fo, tmpl, 32, 32, use=0b10101)
    assert whys == [None, None] and np.array_equal(got, want)
    check_tables(rois, fits, fo, rects, wfits)


@pytest.mark.parametrize("src", [SOURCES[0], SOURCES[4]], ids=[SOURCE_IDS[0], SOURCE_IDS[4]])
def test_crop_aligned_scale_limits(gpu, src):
    """a 13 x down-scale near 45 degrees (the staged chunk must shrink to a few columns), and a 4 x to 8 x up-scale into 112 x 112"""
    kind, flags = src
    BW, BH = 640, 360
    raw, rgb = source(kind, flags, BW, BH)
    fmt = gpu.CAMERA_NV12 if kind == "nv12" else gpu.CAMERA_RGB
    u = uniforms(0xA1160003, 200).reshape(10, 10, 2) - 0.5
    cases = [(32, 32, [(320, 180, 13.0, np.pi / 4), (320, 180, 13.0, np.pi / 6), (300.5, 170.25, 12.5, 0.0), (320, 180, 13.3, -0.8)]),
             (112, 112, [(320, 180, 1 / 4, 0.3), (5, 355, 1 / 8, np.pi / 4), (100.5, 99.5, 1 / 6, np.pi / 2), (636, 3, 1 / 5, 2.5)])]
    for tw, th, sims in cases:
        tmpl = gpu.align_template_face5(tw, th)
        kp = np.stack([kpts(placed(tmpl, tw, th, cx, cy, s, a, u[k, :5] * s)) for k, (cx, cy, s, a) in enumerate(sims)])
        fo = np.zeros(len(kp), dtype=np.int32)
        for nhwc in (1, 0):
            want, rects, wfits, whys = expected_host(rgb, kp, fo, tmpl, tw, th, nhwc)
            assert whys == [None] * len(kp)
            got, rois, fits = gpu.crop_aligned(raw, kp, fo, gpu.align_opts(tmpl), gpu.roi_opts(BW, BH, fmt=fmt, src_flags=flags), tw, th, nhwc)
            check_tables(rois, fits, fo, rects, wfits)
            for i in range(len(kp)):
                assert np.array_equal(got[i], want[i]), (tw, th, nhwc, i, int((got[i] != want[i]).sum()))


@pytest.mark.parametrize("K", [2, 17, 32])
def test_crop_aligned_template_sizes_and_masks(gpu, K):
    """masks that leave 2 points, 4 points and all of them"""
    raw, rgb = source("rgb", 0, W, H, 2)
    tw, th = 40, 24
    u = uniforms(0xA1160004 + K, 2 * K + 6 * 2 * K).reshape(-1, 2)
    tmpl = (u[:K] * (tw, th)).astype(F)
    sims = [(49, 31, 1.0, 0.0), (30, 40, 0.7, 1.1), (80, 12, 1.8, -2.0), (10, 55, 0.5, 3.0), (97, 1, 1.2, 0.4), (49, 31, 2.6, 4.0)]
    kp = np.stack([kpts(placed(tmpl, tw, th, cx, cy, s, a, (u[K * (1 + k):K * (2 + k)] - 0.5) * s)) for k, (cx, cy, s, a) in enumerate(sims)])
    fo = (np.arange(len(kp)) % 2).astype(np.int32)
    masks = [0b11] if K == 2 else [(1 << 1) | (1 << (K - 1)), 0b1011 | (1 << (K - 1)), 0]
    for use in masks + ([(1 << K) - 1] if K != 2 else [0]):
        want, rects, wfits, whys = expected_host(rgb, kp, fo, tmpl, tw, th, use=use)
        assert sum(w is None for w in whys) >= 4
        n = K if use == 0 else bin(use).count("1")
        assert all(f[7] == n for f, w in zip(wfits, whys) if w is None)
        got, rois, fits = gpu.crop_aligned(raw, kp, fo, gpu.align_opts(tmpl, use=use), gpu.roi_opts(W, H), tw, th)
        check_tables(rois, fits, fo, rects, wfits)
        assert np.array_equal(got, want), (K, use, int((got != want).sum()))


@pytest.mark.parametrize("flags", [0, FULL, VU, FULL | VU], ids=SOURCE_IDS[1:])
def test_aligned_nv12_crop_equals_rgb_crop_of_the_converted_frame(gpu, flags):
    nv = np.stack([lcg_frame(0xA1163000 + 7 * flags + f, W * H * 3 // 2) for f in range(2)])
    rgb = np.stack([gpu.nv12_to_rgb(nv[f], W, H, flags) for f in range(2)])
    for tw, th, nhwc in [(32, 32, 0), (40, 24, 1)]:
        tmpl, kp = geometry_sets(gpu, tw, th)
        fo = (np.arange(len(kp)) % 2).astype(np.int32)
        al = gpu.align_opts(tmpl, min_vis=MIN_VIS)
        a, ra, fa = gpu.crop_aligned(nv, kp, fo, al, gpu.roi_opts(W, H, fmt=gpu.CAMERA_NV12, src_flags=flags), tw, th, nhwc)
        b, rb, fb = gpu.crop_aligned(rgb, kp, fo, al, gpu.roi_opts(W, H), tw, th, nhwc)
        assert ra.tobytes() == rb.tobytes() and fa.tobytes() == fb.tobytes() and (ra["frame"] == fo).all()
        assert np.array_equal(a, b), int((a != b).sum())


# ---- the device chain ----------------------------------------------------------------------------------------------------------------------
# The pose twin's random weights give keypoints scattered around each detection's cell; a least-squares fit of a 17-point template to them
# has a small scale (the correlation of two unrelated point sets), so the crops are a few dozen pixels wide: what a second stage sees.
CW, CH, DET_B, DET_CONF = 320, 240, 3, 0.01
DET_HW = 64
K = 17
FRAME_SEED = 0xA116C000
TMPL = (uniforms(0xA1160005, 2 * K).reshape(K, 2) * 160).astype(F)


class Chain:
    """the pose twin, batch 3, with its NV12 frames in HBM"""

    def __init__(self, gpu, flags=0, hw=DET_HW):
        self.gpu, self.flags = gpu, flags
        d = gpu.synth_model(width_x16=1, input_hw=hw, seed=1, head="pose")
        self.kpt = gpu.pose_twin_tensors(d)
        self.det = gpu.Model(d, batch=DET_B)
        self.bufs = []

    def frames(self, seed):
        nv = np.stack([lcg_frame(seed + f, CW * CH * 3 // 2) for f in range(DET_B)])
        buf = self.gpu.DeviceBuffer(nv)
        self.bufs.append(buf)
        return nv, buf

    def detect(self, buf, num_kpt=K, **pose):
        """front-end -> graph -> DFL tail + keypoints; nothing here waits"""
        self.det.preprocess_nv12_device(buf.ptr, CW, CH, DET_B, flags=self.flags)
        self.det.run_device(sync=False)
        self.det.detect_pose_device(self.gpu.pose_opts(self.kpt, num_kpt=num_kpt, **pose), conf=DET_CONF, src=(CW, CH))

    def opts(self, **kw):
        return self.gpu.roi_opts(CW, CH, fmt=self.gpu.CAMERA_NV12, src_flags=self.flags, **{k: v for k, v in kw.items() if k not in ("use", "min_vis")})

    def align(self, **kw):
        return self.gpu.align_opts(TMPL, use=kw.get("use", 0), min_vis=kw.get("min_vis", 0.0))

    def results(self):
        return (self.det.detect_results(),) + self.det.pose_results()

    def close(self):
        self.det.close()
        for b in self.bufs:
            b.free()


_rgb = {}


def expected_input(nv, flags, res, slots, nhwc, **kw):
    """-> (ROI records, fit tuples, dropped, [slots][160 * 160 * 3] bytes) of the numpy selection, fit and sampler over the fetched lists"""
    dets, recs, kp = res
    sel = {k: kw[k] for k in ("min_conf", "classes", "max_per_frame") if k in kw}
    fit_kw = {k: kw[k] for k in ("use", "min_vis", "expand", "min_size") if k in kw}
    kept, fits, where, dropped = align_select_np(dets, recs, kp, TMPL, 160, 160, CW, CH, slots, **sel, **fit_kw)
    key = (nv.tobytes(), flags)
    if key not in _rgb:
        _rgb[key] = [nv12_to_rgb_np(nv[f], CW, CH, flags) for f in range(len(nv))]
    x = np.full((slots, 160 * 160 * 3), -17, dtype=np.int8)
    for k, (f, t) in enumerate(where):
        x[k] = align_crop_np(_rgb[key][f], kp[f][t], TMPL, 160, 160, nhwc, **fit_kw)
    return kept, fits, dropped, x


def check_slots(dst, tin, kept, fits, dropped, want):
    rois, got_dropped = dst.roi_results()
    assert [tuple(int(v) for v in r) for r in rois] == kept and got_dropped == dropped
    table = dst.align_results()
    assert len(table) == dst.batch
    assert [tuple(int(f[k]) for k in FIT_KEYS) for f in table] == fits + [(0,) * 8] * (dst.batch - len(fits))
    for k in range(dst.batch):
        got = dst.read_tensor(tin, frame=k)[:want[k].size].view(np.int8)
        assert np.array_equal(got, want[k]), (k, int((got != want[k]).sum()))


@pytest.mark.parametrize("which", ["shipped", "nhwc_twin"])
def test_chain_end_to_end(gpu, which):
    """preprocess_nv12_device -> run_device -> detect_pose_device -> crop_pose_detections_device -> run -> classify -> label_detections, nothing
    waiting in between; then the lists, both tables, the second model's input and the labels are fetched"""
    d2, tin, tout, nhwc = second_stage(gpu, which)
    c = Chain(gpu)
    dst = gpu.Model(d2, batch=4)
    nv, buf = c.frames(FRAME_SEED)
    c.detect(buf)
    before = [x.tobytes() for x in c.results()[0]] + [x.tobytes() for x in c.results()[1:]]
    c.detect(buf)
    dst.crop_pose_detections_device(c.det, buf.ptr, c.opts(), c.align())
    dst.run_device(sync=False)
    dst.classify_device(top_k=3)
    c.det.label_detections(dst)
    res = c.results()
    assert [x.tobytes() for x in res[0]] + [x.tobytes() for x in res[1:]] == before  # the crop call leaves the lists alone
    n_pose = int((res[1]["det"] >= 0).sum())
    assert n_pose >= 6 and all((r["det"][:int((r["det"] >= 0).sum())] >= 0).all() for r in res[1])
    kept, fits, dropped, want = expected_input(nv, 0, res, 4, nhwc)
    assert len(kept) == 4 and dropped > 0  # more boxes than the second stage has frames: the drop path runs
    check_slots(dst, tin, kept, fits, dropped, want)
    top, _ = dst.classify_results(3)
    labels = c.det.label_results()
    assert int((labels["cls"] >= 0).sum()) == len(kept)
    for k, (f, i, *_r) in enumerate(kept):  # the join is on det, the index in the frame's detection list
        assert labels[f, i].tobytes() == top[k, 0].tobytes()
    # a long destination: the frames behind the last crop are -17, their fit records zeros
    big = gpu.Model(d2, batch=16)
    big.crop_pose_detections_device(c.det, buf.ptr, c.opts(max_per_frame=2), c.align())
    kept, fits, dropped, want = expected_input(nv, 0, res, 16, nhwc, max_per_frame=2)
    assert 0 < len(kept) <= 6 and dropped == 0 and (want[len(kept):] == -17).all() and not (want[:len(kept)] == -17).all()
    check_slots(big, tin, kept, fits, dropped, want)
    big.close()
    dst.close()
    c.close()


def test_chain_selection_rules(gpu):
    """one detection pass, many option sets (the pose block stays in HBM between the crop calls)"""
    d2, tin, tout, nhwc = second_stage(gpu, "shipped")
    c = Chain(gpu, flags=FULL | VU)
    nv, buf = c.frames(FRAME_SEED)
    c.detect(buf)
    res = c.results()
    dets, recs, kp = res
    taken = [d[r["det"][r["det"] >= 0]] for d, r in zip(dets, recs)]
    assert sum(len(t) for t in taken) >= 6
    classes = sorted({int(v) for t in taken for v in t["cls"]})
    confs = np.sort(np.concatenate([t["conf"] for t in taken]))
    vis = np.sort(np.concatenate([k["v"][:len(t)].reshape(-1) for k, t in zip(kp, taken)]))
    sets = [dict(), dict(expand=1.5), dict(expand=0.5), dict(min_size=24), dict(min_size=100000),
            dict(classes=(classes[0], 1)), dict(classes=(classes[len(classes) // 2], max(classes) + 1)), dict(classes=(max(classes) + 1, 3)),
            dict(min_conf=float(confs[len(confs) // 2])), dict(max_per_frame=1), dict(max_per_frame=2, min_conf=float(confs[1])),
            dict(min_vis=float(vis[len(vis) // 2])), dict(min_vis=float(vis[-1]) + 0.5), dict(use=0b1010101, min_vis=float(vis[len(vis) // 4])),
            dict(use=0b11)]
    seen_short = seen_drop = seen_fewer = False
    for batch in (8, 2):
        dst = gpu.Model(d2, batch=batch)
        for kw in sets:
            dst.crop_pose_detections_device(c.det, buf.ptr, c.opts(**kw), c.align(**kw))
            kept, fits, dropped, want = expected_input(nv, FULL | VU, res, batch, nhwc, **kw)
            check_slots(dst, tin, kept, fits, dropped, want)
            seen_short |= 0 < len(kept) < batch
            seen_drop |= dropped > 0
            if kw in (dict(classes=(max(classes) + 1, 3)), dict(min_size=100000), dict(min_vis=float(vis[-1]) + 0.5)):
                assert kept == [] and dropped == 0 and (want == -17).all()
            if kw == dict(max_per_frame=1):
                assert len({k[0] for k in kept}) == len(kept)
            if "min_vis" in kw and kept:
                seen_fewer |= any(f[7] < (K if "use" not in kw else 4) for f in fits)  # min_vis removed points from a fit that was still made
        dst.close()
    assert seen_short and seen_drop and seen_fewer
    c.close()


def test_chain_repeats_on_new_frames(gpu):
    """three rounds of detect -> aligned crop -> run on different frames, nothing waiting inside a round: the tables are reused and every
    round's input is its own"""
    d2, tin, tout, nhwc = second_stage(gpu, "nhwc_twin")
    c = Chain(gpu)
    dst = gpu.Model(d2, batch=4)
    seen = []
    for r in range(3):
        nv, buf = c.frames(FRAME_SEED + 16 * (r + 1))
        c.detect(buf)
        dst.crop_pose_detections_device(c.det, buf.ptr, c.opts(max_per_frame=2), c.align())
        dst.run_device(sync=False)
        res = c.results()
        kept, fits, dropped, want = expected_input(nv, 0, res, 4, nhwc, max_per_frame=2)
        assert len(kept) >= 2
        check_slots(dst, tin, kept, fits, dropped, want)
        seen.append(want[0].tobytes())
    assert len(set(seen)) == 3
    # an upright crop call into the same model leaves no fit table to fetch; the next aligned one brings it back
    dst.crop_detections(c.det, buf.ptr, c.opts(), device=True)
    with pytest.raises(gpu.MarsError) as ei:
        dst.align_results()
    assert ei.value.code == gpu.MARS_ERR_INVALID_TENSOR
    dst.crop_pose_detections_device(c.det, buf.ptr, c.opts(max_per_frame=2), c.align())
    check_slots(dst, tin, kept, fits, dropped, want)
    dst.close()
    c.close()


def test_crop_pose_host_frames_and_refusals(gpu):
    d2, tin, tout, nhwc = second_stage(gpu, "shipped")
    c = Chain(gpu)
    dst = gpu.Model(d2, batch=8)
    nv, buf = c.frames(FRAME_SEED)
    BAD_FILE, BAD_TENSOR = gpu.MARS_ERR_INVALID_FILE, gpu.MARS_ERR_INVALID_TENSOR

    def refused(code, det, frames, into, opts, align, **kw):
        with pytest.raises(gpu.MarsError) as ei:
            into.crop_pose_detections_device(det, frames, opts, align, **kw)
        assert ei.value.code == code

    refused(BAD_TENSOR, c.det, buf.ptr, dst, c.opts(), c.align())  # no pose results in HBM yet
    with pytest.raises(gpu.MarsError) as ei:
        dst.align_results()                                        # and no aligned crop call yet
    assert ei.value.code == BAD_TENSOR
    # an upright DFL decode leaves detections, not keypoints
    c.det.preprocess_nv12_device(buf.ptr, CW, CH, DET_B)
    c.det.run_device(sync=False)
    c.det.detect_dfl_device(conf=DET_CONF, src=(CW, CH))
    refused(BAD_TENSOR, c.det, buf.ptr, dst, c.opts(), c.align())
    c.detect(buf)
    refused(BAD_TENSOR, c.det, buf.ptr, dst, c.opts(), gpu.align_opts(TMPL[:5]))  # num_kpt != K of the pose call
    refused(BAD_TENSOR, c.det, buf.ptr, c.det, c.opts(), c.align())               # det_model == dst_model
    refused(BAD_TENSOR, c.det, buf.ptr, dst, c.opts(), c.align(), input_index=1)
    refused(BAD_FILE, c.det, buf.ptr, dst, c.opts(keep_aspect=True), c.align())   # the two flags
    refused(BAD_FILE, c.det, buf.ptr, dst, c.opts(area=True), c.align())
    refused(BAD_FILE, c.det, buf.ptr, dst, c.opts(), None)
    refused(BAD_FILE, c.det, buf.ptr, dst, c.opts(), gpu.align_opts(TMPL, use=1 << K))
    dst.pipe_open()
    refused(BAD_TENSOR, c.det, buf.ptr, dst, c.opts(), c.align())                 # an open pipe
    dst.pipe_close()
    # the host-frame form equals the device form
    dst.crop_pose_detections(c.det, nv, c.opts(expand=1.5), c.align())
    res = c.results()
    kept, fits, dropped, want = expected_input(nv, 0, res, 8, nhwc, expand=1.5)
    assert len(kept) > 0
    check_slots(dst, tin, kept, fits, dropped, want)
    # a pose call followed by set_batch: the results are gone with the batch they were made for
    c.det.set_batch(2)
    refused(BAD_TENSOR, c.det, buf.ptr, dst, c.opts(), c.align())
    dst.close()
    c.close()
