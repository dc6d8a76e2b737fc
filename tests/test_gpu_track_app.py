"""Appearance in tracking on the device (include/mars_hip.h, "Appearance in tracking"): the kernel's cosine matrix through its test hook, seeded
scenes through mars_yolo_track_lists_app, ties, the two thresholds' edges, a full table, the staircase with appearance keys, split calls,
the plain calls on a tracker with a plane, and the chain crop -> classify -> track_app_device.  The expected values come from the numpy
restatement of tests/trackappref.py (pinned by tests/test_track_app_cpu.py); every comparison -- outputs, every field of every live state,
the counters, the embeddings -- is bit-exact."""
import numpy as np
import pytest

from conftest import lcg_frame
from test_track_cpu import DET, LOW, SCENE_IDS, SCENE_OPTS, SCENES, SLOTS, F, box, frames, iou_np, scene
from trackappref import (APP_LOW, APP_SCENE_C, APP_SCENE_OPTS, APP_SCENE_S, SCENE_EVENTS, TrackerAppNp, app_scene, cosine_matrix_np, cosine_np,
                         quantise_np, rand_vectors, track_app_np)

pytestmark = pytest.mark.gpu
APP_KEYS = ("app_thresh", "app_min_iou", "smooth")


def same_state(trk, ref, what):
    for b in range(ref.S):
        st, cnt = trk.read(b)
        want, want_cnt = ref.read(b)
        assert cnt.tolist() == want_cnt.tolist(), (what, b, cnt, want_cnt)
        assert st.dtype == want.dtype and st.shape == want.shape, (what, b, st.shape, want.shape)
        assert st.tobytes() == want.tobytes(), (what, b)
        q, ee = trk.read_embeddings(b)
        wq, wee = ref.read_embeddings(b)
        assert ee.tolist() == wee.tolist(), (what, b, "ee")
        assert q.shape == wq.shape and q.tobytes() == wq.tobytes(), (what, b, "embeddings")


def both(gpu, trk, ref, dets, counts, vectors, index, what, idents=None, **kw):
    """the same frames through the device and through the restatement: outputs, states, counters and embeddings agree to the bit"""
    app = {k: kw.pop(k) for k in APP_KEYS if k in kw}
    out = gpu.track_lists_app(trk, dets, counts, vectors, index, gpu.track_opts(**kw), gpu.track_app_opts(**app), idents=idents)
    want = track_app_np(ref, dets, counts, vectors, index, idents=idents, **kw, **app)
    assert out.dtype == want.dtype and out.shape == want.shape, what
    assert out.tobytes() == want.tobytes(), (what, np.argwhere(out != want)[:4])
    same_state(trk, ref, what)
    return out


def pair(gpu, streams, channels):
    return gpu.Tracker(streams, channels), TrackerAppNp(streams, channels)


# ---- the matrix routine --------------------------------------------------------------------------------------------------------------------
# the corners of nt, nc in {1, 256} and C in {1, 4096}, then a handful around the 16-row tile, the 64-channel step and the table's edge
MATRIX = [(nt, nc, c) for nt in (1, 256) for nc in (1, 256) for c in (1, 4096)] + [
    (15, 17, 64), (16, 16, 65), (17, 15, 1), (255, 256, 64), (256, 255, 65), (16, 255, 4096), (17, 1, 64), (1, 17, 65), (255, 15, 4096)]


@pytest.mark.parametrize("shape", MATRIX, ids=["t%d_c%d_ch%d" % s for s in MATRIX])
def test_cosine_matrix(gpu, shape):
    """another seeded vector in every row and every column: a misplaced tile, lane or 64-channel step shows as a wrong float.  Rows and
    columns without an embedding give zeros"""
    nt, nc, c = shape
    seed = 0x7AD0000 + 0x1000 * (nt + 3 * nc) + c
    tv = rand_vectors(seed, nt, c, shift=8)
    tv[:, 0] |= 1  # (no null rows but those made below)
    cv = rand_vectors(seed + 1, nc, c, shift=3)
    cv[:, 0] |= 1
    if nc > 2:
        cv[nc // 2] = 0        # a null vector
    if nc == 256:
        cv[255, -1] = -(1 << 31)
    quant = [quantise_np(v) for v in tv]
    tq = np.stack([q for q, _ in quant])
    tee = np.array([e for _, e in quant], dtype=np.int32)
    if nt > 2:
        tee[[1, nt - 1]] = 0   # slots without an embedding: their bytes must not matter
    cq = [quantise_np(v) for v in cv]
    want = cosine_matrix_np(tq, tee, np.stack([q for q, _ in cq]), [e for _, e in cq])
    got = gpu.track_cosine_matrix(tq, tee, cv)
    assert got.shape == want.shape == (nt, nc)
    assert got.tobytes() == want.tobytes(), np.argwhere(got.view(np.uint32) != want.view(np.uint32))[:6]
    r, k = nt // 3, nc // 3  # ... and the vectorised restatement is the scalar one
    if tee[r] and cq[k][1]:
        assert want[r, k].tobytes() == cosine_np(cq[k][0], cq[k][1], tq[r], int(tee[r])).tobytes()
    assert (want[tee == 0] == 0).all() and np.abs(want).max() > 0.0


# ---- seeded scenes -------------------------------------------------------------------------------------------------------------------------
APP_SHAPES = [(s, c) for s in APP_SCENE_S for c in APP_SCENE_C]


@pytest.mark.parametrize("shape", APP_SHAPES, ids=["s%d_c%d" % s for s in APP_SHAPES])
def test_track_lists_app(gpu, shape):
    streams, channels = shape
    seed = 0x7AA0000 + 0x10000 * APP_SHAPES.index(shape)  # (trackappref.app_scene_list's: the scenes tests/test_track_app_cpu.py pins)
    for major in (False, True):
        dets, counts, vectors, index = app_scene(seed, streams, channels, major)
        for smooth in (False, True):
            for low in (APP_LOW, 0.0):
                trk, ref = pair(gpu, streams, channels)
                both(gpu, trk, ref, dets, counts, vectors, index, (shape, major, smooth, low), low_conf=low, stream_major=major, smooth=smooth,
                     **APP_SCENE_OPTS)
                assert all(ref.events[k] >= 1 for k in SCENE_EVENTS), ref.events
                trk.close()


def test_default_options_and_identities(gpu):
    """no options at all, and MARS_TRACK_CARRY_IDENTITY beside the embeddings"""
    dets, counts, vectors, index = app_scene(0x7AA1000, 2, 64)
    trk, ref = pair(gpu, 2, 64)
    out = gpu.track_lists_app(trk, dets, counts, vectors, index)
    assert out.tobytes() == track_app_np(ref, dets, counts, vectors, index).tobytes()
    same_state(trk, ref, "defaults")
    ids = np.zeros(dets.shape, dtype=gpu.CLS_DTYPE)
    ids["cls"] = (np.arange(ids.size).reshape(ids.shape) % 5) - 1
    ids["score"] = (np.arange(ids.size).reshape(ids.shape) % 7) / F(8)
    both(gpu, trk, ref, dets, counts, vectors, index, "identities", idents=ids, carry_identity=True, smooth=True)
    trk.close()


# ---- ties, edges ---------------------------------------------------------------------------------------------------------------------------
def test_exact_ties(gpu):
    """two equal tracks, two equal detections, one embedding everywhere: four equal keys go by slot, then by index"""
    d, n = frames([box(0), box(0)], [box(1), box(1)])
    vec = np.array([[5, -3, 2]], dtype=np.int32)
    idx = np.zeros(d.shape, dtype=np.int32)
    trk, ref = pair(gpu, 1, 3)
    out = both(gpu, trk, ref, d, n, vec, idx, "ties")
    assert out[1, :2].tolist() == [(1, 2), (2, 2)]
    # the same with the pairs eligible on appearance alone
    d, n = frames([box(0, w=60, h=60), box(0, w=60, h=60)], [box(44, w=60, h=60), box(44, w=60, h=60)])
    trk.reset()
    ref.reset()
    out = both(gpu, trk, ref, d, n, vec, idx, "ties on appearance")
    assert out[1, :2].tolist() == [(1, 2), (2, 2)] and ref.events["app_low_iou"] == 2
    trk.close()


def test_threshold_edges(gpu):
    """app_thresh at the pair's own cosine bits makes it eligible, the next float above does not; the same for app_min_iou and the IoU"""
    d, n = frames([box(100, w=60, h=60)], [box(144, w=60, h=60)])
    vec = np.array([[100, 7, -20, 3], [90, 30, -10, 12]], dtype=np.int32)
    idx = np.zeros(d.shape, dtype=np.int32)
    idx[1, 0] = 1
    (q0, qq0), (q1, qq1) = quantise_np(vec[0]), quantise_np(vec[1])
    cs = cosine_np(q1, qq1, q0, qq0)
    iou = iou_np(F(100), F(0), F(60), F(60), F(144), F(0), F(60), F(60))
    assert F(0.75) < cs < F(1) and F(0.1) < iou < F(0.3)
    up = lambda v: np.nextafter(F(v), F(2), dtype=F)
    trk, ref = pair(gpu, 1, 4)
    for kw, ids in ((dict(app_thresh=cs), (1, 2)), (dict(app_thresh=up(cs)), (2, 1)), (dict(app_min_iou=iou), (1, 2)), (dict(app_min_iou=up(iou)), (2, 1)),
                    (dict(app_thresh=cs, app_min_iou=iou), (1, 2))):
        trk.reset()
        ref.reset()
        out = both(gpu, trk, ref, d, n, vec, idx, kw, **{k: float(v) for k, v in kw.items()})
        assert out[1, 0].tolist() == ids, kw
    trk.close()


# ---- a full table --------------------------------------------------------------------------------------------------------------------------
def test_full_table(gpu):
    """256 live tracks and 257 detections, C = 64.  The boxes stand in pairs 30 apart and step towards each other as in the seeded scenes'
    crossing: the IoU prefers the partner's box.  In a seeded share of the pairs the embeddings say the same as the IoU (the two objects
    did swap), in the others they contradict it -- appearance decides.  The 257th detection overflows"""
    C = 64
    base = rand_vectors(0x7AE0000, SLOTS, C, shift=16)
    swap = lcg_frame(0x7AE0001, SLOTS // 2) < 100
    first, second, emb = [], [], []
    for j in range(SLOTS // 2):
        x, y = 100.0 + 300.0 * (j % 16), 100.0 + 300.0 * (j // 16)
        first += [box(x, y=y, w=60, h=60), box(x + 30, y=y, w=60, h=60)]
        second += [box(x + 20, y=y, w=60, h=60), box(x + 10, y=y, w=60, h=60)]
        emb += [2 * j + 1, 2 * j] if swap[j] else [2 * j, 2 * j + 1]
    second.append(box(9000.0, y=9000.0, w=60, h=60))
    d, n = frames(first, second, max_det=300)
    vectors = np.concatenate([base, base + rand_vectors(0x7AE0002, SLOTS, C, shift=26)])
    idx = np.full(d.shape, -1, dtype=np.int32)
    idx[0, :SLOTS] = np.arange(SLOTS)
    idx[1, :SLOTS] = SLOTS + np.array(emb)
    trk, ref = pair(gpu, 1, C)
    out = both(gpu, trk, ref, d, n, vectors, idx, "full table")
    assert 20 < swap.sum() < 108 and ref.events["key_changed"] == 2 * int((~swap).sum())
    assert (out["hits"][1, :SLOTS] == 2).all() and out[1, SLOTS].tolist() == (-1, 0) and trk.read(0)[1].tolist() == [256, 0, 1, 0]
    assert out["id"][1, :SLOTS].tolist() == [e + 1 for e in emb]  # every box went to the track its embedding names
    trk.close()


def test_staircase_with_appearance_keys(gpu):
    """test_gpu_track's staircase -- 256 tracks and 256 detections on a line, the gaps strictly shrinking, one mutual pair per round -- with
    iou_thresh at 0.9, so that every pair is eligible on appearance alone and every key is fmaxf(iou, cos): one cosine of about 0.24 for
    all pairs, below every neighbour's IoU"""
    gap = F(40) - np.arange(2 * SLOTS, dtype=F) * F(0.05)
    x = np.concatenate([[F(0)], np.cumsum(gap[:-1], dtype=F)]).astype(F)
    d, n = frames([box(float(v), w=100.0, h=100.0) for v in x[0::2]], [box(float(v), w=100.0, h=100.0) for v in x[1::2]], max_det=SLOTS)
    vectors = np.array([[4, 0], [1, 4]], dtype=np.int32)
    idx = np.zeros(d.shape, dtype=np.int32)
    idx[1] = 1
    trk, ref = pair(gpu, 1, 2)
    out = both(gpu, trk, ref, d, n, vectors, idx, "staircase", iou_thresh=0.9, app_thresh=0.2)
    assert out["id"][1].tolist() == list(range(1, SLOTS + 1)) and (out["hits"][1] == 2).all() and ref.events["app_low_iou"] == SLOTS
    trk.close()


# ---- calls ---------------------------------------------------------------------------------------------------------------------------------
def test_split_calls(gpu):
    """one call over 4 steps == two calls over 2 steps, embeddings included, under both maps and with the blend"""
    S, T = 2, 4
    for major in (False, True):
        dets, counts, vectors, index = app_scene(0x7AA2000, S, 65, major)
        kw = dict(low_conf=APP_LOW, stream_major=major, smooth=True, **APP_SCENE_OPTS)
        one, ref = pair(gpu, S, 65)
        whole = both(gpu, one, ref, dets, counts, vectors, index, ("whole", major), **kw)
        two = gpu.Tracker(S, 65)
        got = np.zeros_like(whole)
        for c in range(2):
            sel = [b * T + 2 * c + t for b in range(S) for t in range(2)] if major else list(range(2 * c * S, (2 * c + 2) * S))
            app = gpu.track_app_opts(smooth=True)
            got[sel] = gpu.track_lists_app(two, dets[sel], counts[sel], vectors, index[sel], gpu.track_opts(**{k: v for k, v in kw.items() if k != "smooth"}), app)
        assert got.tobytes() == whole.tobytes()
        same_state(two, ref, ("halves", major))
        one.close()
        two.close()


@pytest.mark.parametrize("shape", SCENES, ids=SCENE_IDS)
def test_plain_calls_on_a_tracker_with_a_plane(gpu, shape):
    """mars_yolo_track_lists on a tracker with a plane, and the appearance call with no vectors, give the bytes of the plain call on a
    tracker without one"""
    streams, steps, boxes, max_det = shape
    dets, counts = scene(0x7AC0000 + boxes, streams, steps, boxes, max_det)
    o = gpu.track_opts(low_conf=LOW, **SCENE_OPTS)
    plain, plane, app, one = gpu.Tracker(streams), gpu.Tracker(streams, 65), gpu.Tracker(streams, 64), gpu.Tracker(streams, 1)
    want = gpu.track_lists(plain, dets, counts, o)
    assert gpu.track_lists(plane, dets, counts, o).tobytes() == want.tobytes()
    assert gpu.track_lists_app(app, dets, counts, None, None, o).tobytes() == want.tobytes()
    assert gpu.track_lists_app(one, dets, counts, None, np.zeros(dets.shape, dtype=np.int32), o).tobytes() == want.tobytes()
    for b in range(streams):
        st, cnt = plain.read(b)
        for t in (plane, app, one):
            assert t.read(b)[0].tobytes() == st.tobytes() and t.read(b)[1].tolist() == cnt.tolist()
            assert (t.read_embeddings(b)[1] == 0).all() and not t.read_embeddings(b)[0].any()
    with pytest.raises(gpu.MarsError) as ei:
        plain.read_embeddings(0)
    assert ei.value.code == gpu.MARS_ERR_INVALID_TENSOR
    with pytest.raises(gpu.MarsError) as ei:
        gpu.track_lists_app(plain, dets, counts, None, None, o)  # a tracker without a plane
    assert ei.value.code == gpu.MARS_ERR_INVALID_TENSOR
    for t in (plain, plane, app, one):
        t.close()


def test_a_stale_embedding_never_survives_death_and_birth(gpu):
    """max_miss = 1: a track with an embedding dies in the step in which a box WITHOUT one is born into its slot, through the plain call;
    the slot then holds no embedding, so a later box that looks like the dead track and jumps is not taken on appearance"""
    d, n = frames([box(100, w=60, h=60)], [], [box(5000, w=60, h=60)], [box(5044, w=60, h=60)])
    vec = np.array([[9, 1, -4]], dtype=np.int32)
    none = np.full(d.shape, -1, dtype=np.int32)
    idx = none.copy()
    idx[0, 0] = idx[3, 0] = 0
    trk, ref = pair(gpu, 1, 3)
    both(gpu, trk, ref, d[:1], n[:1], vec, idx[:1], "birth", max_miss=1)
    assert trk.read_embeddings(0)[1].tolist() == [quantise_np(vec[0])[1]]
    out = gpu.track_lists(trk, d[1:3], n[1:3], gpu.track_opts(max_miss=1))  # the plain call keeps the plane consistent
    assert out.tobytes() == track_app_np(ref, d[1:3], n[1:3], None, None, max_miss=1).tobytes()
    same_state(trk, ref, "death and birth")
    st, cnt = trk.read(0)
    assert st["id"].tolist() == [2] and cnt.tolist() == [2, 1, 0, 0] and ref.slots[0][0]["id"] == 2  # slot 0 again
    assert trk.read_embeddings(0)[1].tolist() == [0] and not trk.read_embeddings(0)[0].any()
    out = both(gpu, trk, ref, d[3:], n[3:], vec, idx[3:], "the look-alike", max_miss=1)
    assert out[0, 0].tolist() == (3, 1)  # born: IoU 0.154 and nothing to compare with
    trk.close()


def test_lifecycle_and_refusals_on_the_device(gpu):
    BAD_FILE, BAD_TENSOR = gpu.MARS_ERR_INVALID_FILE, gpu.MARS_ERR_INVALID_TENSOR

    def refused(code, fn, *a, **kw):
        with pytest.raises(gpu.MarsError) as ei:
            fn(*a, **kw)
        assert ei.value.code == code

    refused(BAD_TENSOR, gpu.Tracker, 3, 4097)
    trk = gpu.Tracker(3, 8)
    d, n = frames([box(0)], [box(1)], [box(2)], [box(3)])
    vec, idx = np.ones((2, 8), dtype=np.int32), np.zeros(d.shape, dtype=np.int32)
    refused(BAD_TENSOR, gpu.track_lists_app, trk, d, n, vec, idx)          # 4 frames, 3 streams
    refused(BAD_TENSOR, trk.read_embeddings, 3)
    refused(BAD_FILE, gpu.track_lists_app, trk, d[:3], n[:3], vec, idx[:3], gpu.track_opts(carry_identity=True))
    refused(BAD_FILE, gpu.track_lists_app, trk, d[:3], n[:3], vec, idx[:3], None, gpu.track_app_opts(app_thresh=1.5))
    refused(BAD_FILE, gpu.track_lists_app, trk, d[:3], n[:3], vec, None)   # vectors without their index
    assert all(len(trk.read(b)[0]) == 0 and len(trk.read_embeddings(b)[1]) == 0 for b in range(3))  # nothing moved
    gpu.track_lists_app(trk, d[:3], n[:3], vec, idx[:3])
    assert all(trk.read_embeddings(b)[1].tolist() == [8 * 127 * 127] for b in range(3))
    trk.reset()
    assert all(len(trk.read_embeddings(b)[1]) == 0 for b in range(3))
    gpu.track_lists(trk, d[:3], n[:3])
    assert all(trk.read_embeddings(b)[1].tolist() == [0] for b in range(3))  # the reset cleared the plane: the new tracks hold nothing
    trk.close()
    trk.close()


# ---- the chain -----------------------------------------------------------------------------------------------------------------------------
CW, CH, DET_B, DET_CONF = 320, 240, 4, 0.01
FRAME_SEED = 0x7AF0000


def lists_of(dets):
    d = np.zeros((len(dets), 1000), dtype=DET)
    for f, x in enumerate(dets):
        d[f, :len(x)] = x
    return d, np.array([len(x) for x in dets], dtype=np.int32)


def test_chain_tracks_with_appearance(gpu):
    """the DFL detector twin at batch 4 -> crops -> the second-model twin at batch 8 -> classify -> track_app_device over S = 2, two steps,
    twice: the ids and the tables, embeddings included, are those of mars_yolo_track_lists_app fed the fetched detections, sums and ROI
    table; the second call meets tracks that hold embeddings"""
    BAD_TENSOR = gpu.MARS_ERR_INVALID_TENSOR

    def refused(fn, *a, **kw):
        with pytest.raises(gpu.MarsError) as ei:
            fn(*a, **kw)
        assert ei.value.code == BAD_TENSOR

    det = gpu.Model(gpu.synth_model(width_x16=1, input_hw=64, seed=1, head="dfl"), batch=DET_B)
    dst = gpu.Model(gpu.synth_model(tiny=True, input_hw=160, seed=5), batch=8)
    nv = np.stack([lcg_frame(FRAME_SEED + f % 2, CW * CH * 3 // 2) for f in range(DET_B)])  # each stream sees its frame again in step 1
    buf = gpu.DeviceBuffer(nv)
    ropts = gpu.roi_opts(CW, CH, fmt=gpu.CAMERA_NV12, max_per_frame=2)
    probe = gpu.Tracker(2, 4095)

    def detect():
        det.preprocess_nv12_device(buf.ptr, CW, CH, DET_B)
        det.run_device(sync=False)
        det.detect_dfl_device(conf=DET_CONF, src=(CW, CH))

    def second():
        dst.crop_detections(det, buf.ptr, ropts, device=True)
        dst.run_device(sync=False)
        dst.classify_device(top_k=1)

    refused(det.track_app_device, dst, probe)   # no detections in HBM, no crop call
    detect()
    refused(det.track_app_device, dst, probe)   # no crop call into dst out of det
    dst.crop_detections(det, buf.ptr, ropts, device=True)
    dst.run_device(sync=False)
    refused(det.track_app_device, dst, probe)   # no classify results
    dst.classify_device(top_k=1)
    _, sums = dst.classify_results(1)
    C = sums.shape[1]
    assert C != 4095
    refused(det.track_app_device, dst, probe)   # the tracker's channels are not the classify results' C
    refused(det.track_app_device, det, probe)   # det_model == cls_model
    plain = gpu.Tracker(2)
    refused(det.track_app_device, dst, plain)   # a tracker without a plane
    plain.close()
    three = gpu.Tracker(3, C)
    refused(det.track_app_device, dst, three)   # 4 frames, 3 streams
    three.close()
    refused(det.track_results)                  # nothing pending: every call above was refused before any device work
    trk, fed, ref = gpu.Tracker(2, C), gpu.Tracker(2, C), TrackerAppNp(2, C)
    refused(det.track_app_device, dst, trk, carry_identity=True)  # no identity results
    kw = None
    for r in range(2):
        if r:
            detect()
            second()
        dets = det.detect_results()
        if kw is None:  # thresholds inside the detector's own confidences: the upper half is the high set, the quarter below it the low set
            conf = np.sort(np.concatenate([x["conf"] for x in dets]))
            kw = dict(min_conf=float(conf[len(conf) // 2]), low_conf=float(conf[len(conf) // 4]), iou_thresh=0.5)
            assert 0 < kw["low_conf"] < kw["min_conf"] <= 1
        app = gpu.track_app_opts(smooth=bool(r))
        if r:
            tracks = det.track_app(dst, trk, gpu.track_opts(**kw), app)
        else:
            det.track_app_device(dst, trk, gpu.track_opts(**kw), app)
            tracks = det.track_results()
        rois, _ = dst.roi_results()
        _, sums = dst.classify_results(1)
        d, n = lists_of(dets)
        index = np.full(d.shape, -1, dtype=np.int32)
        for k, roi in enumerate(rois):
            index[roi["frame"], roi["det"]] = k
        assert len(rois) >= 2 and (index >= 0).sum() == len(rois) and len(set(rois["frame"].tolist())) >= 2
        got = gpu.track_lists_app(fed, d, n, sums[:len(rois)], index, gpu.track_opts(**kw), app)
        want = track_app_np(ref, d, n, sums[:len(rois)], index, smooth=bool(r), **kw)
        assert tracks.tobytes() == got.tobytes() == want.tobytes(), r
        same_state(trk, ref, ("chain", r))
        same_state(fed, ref, ("fed", r))
    assert sum((trk.read_embeddings(b)[1] > 0).sum() for b in range(2)) >= 2 and ref.events["smooth"] >= 1
    det.pipe_open()
    refused(det.track_app_device, dst, trk)     # an open pipe
    det.pipe_close()
    for t in (trk, fed, probe):
        t.close()
    buf.free()
    dst.close()
    det.close()
