"""NV12 camera frames through the device front-end and the camera pipe (include/mars_hip.h, "NV12 camera frames").  The expected bytes come
from a numpy restatement of the conversion (int32, >>, np.clip) fed to the oracle's letterbox; every comparison is bit-exact."""
import numpy as np
import pytest

import marsfile
from conftest import lcg_frame

pytestmark = pytest.mark.gpu

FULL, VU = 1, 2
ALL_FLAGS = [0, FULL, VU, FULL | VU]
FLAG_IDS = ["limited_uv", "full_uv", "limited_vu", "full_vu"]


def nv12_to_rgb_np(buf, w, h, flags):
    """the conversion as the header states it: Y plane [h][w], chroma plane [h/2][w/2][2] behind it, nearest chroma, integer BT.601"""
    buf = np.asarray(buf, dtype=np.uint8).reshape(-1)
    assert buf.size == w * h * 3 // 2 and w % 2 == 0 and h % 2 == 0
    y = buf[:w * h].reshape(h, w).astype(np.int32)
    c = buf[w * h:].reshape(h // 2, w // 2, 2).astype(np.int32)
    u, v = (c[..., 1], c[..., 0]) if flags & VU else (c[..., 0], c[..., 1])
    d = np.repeat(np.repeat(u - 128, 2, axis=0), 2, axis=1)
    e = np.repeat(np.repeat(v - 128, 2, axis=0), 2, axis=1)
    if flags & FULL:
        r = (256 * y + 359 * e + 128) >> 8
        g = (256 * y - 88 * d - 183 * e + 128) >> 8
        b = (256 * y + 454 * d + 128) >> 8
    else:
        cc = y - 16
        r = (298 * cc + 409 * e + 128) >> 8
        g = (298 * cc - 100 * d - 208 * e + 128) >> 8
        b = (298 * cc + 516 * d + 128) >> 8
    return np.clip(np.stack([r, g, b], axis=-1), 0, 255).astype(np.uint8)


def nv12_frame(seed, w, h):
    return lcg_frame(seed, w * h * 3 // 2)


_ALL_TRIPLES = None


def all_triples_frame():
    """4096 x 4096: every (Y, U, V) once.  2 x 2 block b (row-major over 2048 x 2048) carries the chroma pair (b >> 6) = U * 256 + V and the
    four Y values 4 (b & 63) .. + 3"""
    global _ALL_TRIPLES
    if _ALL_TRIPLES is None:
        b = np.arange(2048 * 2048, dtype=np.int64).reshape(2048, 2048)
        y = np.empty((4096, 4096), dtype=np.uint8)
        base = (b & 63) * 4
        y[0::2, 0::2], y[0::2, 1::2], y[1::2, 0::2], y[1::2, 1::2] = base, base + 1, base + 2, base + 3
        c = np.stack([(b >> 14) & 255, (b >> 6) & 255], axis=-1).astype(np.uint8)
        _ALL_TRIPLES = np.concatenate([y.reshape(-1), c.reshape(-1)])
    return _ALL_TRIPLES


def test_all_triples_frame_is_complete():
    f = all_triples_frame()
    y = f[:4096 * 4096].reshape(4096, 4096).astype(np.int64)
    c = f[4096 * 4096:].reshape(2048, 2048, 2).astype(np.int64)
    uv = np.repeat(np.repeat(c[..., 0] * 256 + c[..., 1], 2, axis=0), 2, axis=1)
    seen = np.bincount((uv * 256 + y).reshape(-1), minlength=1 << 24)
    assert seen.size == 1 << 24 and (seen == 1).all()


@pytest.mark.parametrize("flags", ALL_FLAGS, ids=FLAG_IDS)
def test_nv12_to_rgb_every_triple(gpu, flags):
    """every (Y, U, V): both clamps and the floor shift on negative sums"""
    f = all_triples_frame()
    want = nv12_to_rgb_np(f, 4096, 4096, flags)
    assert want.min() == 0 and want.max() == 255
    got = gpu.nv12_to_rgb(f, 4096, 4096, flags)
    assert np.array_equal(got, want), int((got != want).sum())


@pytest.mark.parametrize("flags", ALL_FLAGS, ids=FLAG_IDS)
def test_nv12_to_rgb_sizes(gpu, flags):
    """one chroma pair, a row shorter than a thread's 16 pixels, ragged row ends with rows at every dword alignment, the camera size"""
    for i, (w, h) in enumerate([(2, 2), (6, 2), (98, 62), (1280, 720)]):
        f = nv12_frame(0x12A000 + 16 * i + flags, w, h)
        got = gpu.nv12_to_rgb(f, w, h, flags)
        want = nv12_to_rgb_np(f, w, h, flags)
        assert got.shape == (h, w, 3) and np.array_equal(got, want), (w, h, int((got != want).sum()))


# (w, h, tw, th, nhwc)
GEOMETRIES = [(1280, 720, 640, 640, 1),   # camera geometry
              (1280, 720, 640, 640, 0),   # ... planar
              (98, 62, 224, 160, 1),      # growing axes, w % 4 == 2, repeated edge rows
              (50, 42, 200, 216, 1),      # bands left and right
              (334, 500, 320, 320, 1),    # shrinking
              (1920, 1080, 1024, 576, 1), # four columns per thread
              (6, 2, 24, 8, 1),           # one chroma row
              (640, 480, 640, 640, 1),    # 4:3 source, bands above and below
              (2000, 1500, 50, 50, 1)]    # the strip form is not offered: conversion + per-pixel kernel by the launcher's own choice


@pytest.mark.parametrize("form", [0, 1, 2], ids=["strips", "tiles", "per_pixel"])
def test_letterbox_nv12_forms_write_the_same_bytes(gpu, orc, form, monkeypatch):
    """the fused strip kernel (form 0, where it is offered) and the conversion followed by the tiled / per-pixel kernels (forced, or chosen by
    the launcher) against numpy + the oracle's letterbox"""
    monkeypatch.setenv("MARS_HIP_LETTERBOX_FORM", str(form))
    for i, (w, h, tw, th, nhwc) in enumerate(GEOMETRIES):
        flags = ALL_FLAGS[i % 4]
        f = nv12_frame(0x12B000 + i, w, h)
        got = gpu.letterbox_nv12(f, w, h, tw, th, nhwc, flags)
        want = orc.letterbox(nv12_to_rgb_np(f, w, h, flags), tw, th, nhwc)
        assert np.array_equal(got, want), (w, h, tw, th, nhwc, flags, form, int((got != want).sum()))


@pytest.mark.parametrize("flags", [FULL, VU], ids=["full_uv", "limited_vu"])
def test_letterbox_nv12_fused_flags(gpu, orc, flags):
    """the fused kernel at the ragged geometry under the flag combinations the geometry list gives other sizes"""
    for (w, h, tw, th, nhwc) in [(98, 62, 224, 160, 0), (210, 158, 128, 128, 1)]:
        f = nv12_frame(0x12C000 + flags, w, h)
        got = gpu.letterbox_nv12(f, w, h, tw, th, nhwc, flags)
        want = orc.letterbox(nv12_to_rgb_np(f, w, h, flags), tw, th, nhwc)
        assert np.array_equal(got, want), (w, h, flags, int((got != want).sum()))


def test_preprocess_nv12_over_a_batch(gpu, orc):
    """B = 5 frames of 210 x 158: 49770 bytes each, 2 mod 4, so frames 1 and 3 start at dword-unaligned addresses; into an NHWC and an
    NCHW-tagged graph input, in two calls; one frame's graph outputs against the oracle's"""
    B, w, h, hw = 5, 210, 158, 128
    fb = w * h * 3 // 2
    assert fb == 49770 and fb % 4 == 2
    frames = lcg_frame(0x12D000, B * fb).reshape(B, fb)
    for nchw in (False, True):
        d = gpu.synth_model(width_x16=4, input_hw=hw, seed=5, nchw_int8=nchw)
        hdr, tensors, _ = marsfile.parse(d)
        tin = hdr["inputs"][0]
        m = gpu.Model(d, batch=B)
        m.preprocess_nv12(frames[:2], w, h, flags=0, first_frame=0)
        m.preprocess_nv12(frames[2:], w, h, flags=0, first_frame=2)
        m.run_device()
        m.download()
        xs = [orc.letterbox(nv12_to_rgb_np(frames[f], w, h, 0), hw, hw, 0 if nchw else 1) for f in range(B)]
        for f in range(B):
            assert np.array_equal(m.read_tensor(tin, frame=f)[:xs[f].size].view(np.int8), xs[f]), (nchw, f)
        g = orc.Graph(d)
        g.set_input(0, xs[3].tobytes())
        assert g.run() == 0
        for oi, ti in enumerate(hdr["outputs"]):
            assert np.array_equal(m.output_view(oi)[3], g.tensor(ti)), (nchw, oi)
        with pytest.raises(gpu.MarsError):
            m.preprocess_nv12(frames, w, h, first_frame=1)  # frames beyond the batch
        m.close()


def test_camera_pipe_nv12_equals_preprocess_run_detect(gpu):
    """mars_hip_pipe_* in camera mode fed NV12 frames returns, batch for batch, what mars_hip_preprocess_nv12 + run + detect give"""
    d = gpu.synth_model(width_x16=4, input_hw=128, seed=31)
    hdr, tensors, _ = marsfile.parse(d)
    B, cw, ch, N = 3, 200, 152, 5
    fb = cw * ch * 3 // 2
    outputs = tuple(range(len(hdr["outputs"])))
    batches = [lcg_frame(0xCA300 + 10 * k, B * fb).reshape(B, fb) for k in range(N)]
    m = gpu.Model(d, batch=B)
    want = []
    for k in range(N):
        m.preprocess_nv12(batches[k], cw, ch)
        m.run_device()
        want.append([x.tobytes() for x in m.detect(outputs=outputs, thresh=0.45)])
    m.pipe_open(download_outputs=False, detect=True, det_outputs=outputs, thresh=0.45, camera=(cw, ch), camera_format=gpu.CAMERA_NV12)
    got = []
    for k in range(N):
        v = m.pipe_input_view(0)
        assert v.shape == (3, 200 * 152 * 3 // 2)
        v[:] = batches[k]
        m.pipe_submit()
        if k >= 2:
            got.append([x.tobytes() for x in m.pipe_wait()[1]])
            assert gpu.lib().mars_hip_pipe_camera_ms(m.p) > 0
    for _ in range(2):
        got.append([x.tobytes() for x in m.pipe_wait()[1]])
        assert gpu.lib().mars_hip_pipe_camera_ms(m.p) > 0
    m.pipe_close()
    m.close()
    assert got == want
    assert sum(len(b) for w_ in want for b in w_) > 0


def test_camera_pipe_nv12_heads_equal_the_rgb_pipe(gpu):
    """raw heads, boxes in camera pixels: the RGB camera pipe fed the numpy-converted frames and the NV12 camera pipe fed the NV12 frames
    return the same detections (full range, V before U)"""
    from test_gpu_yolo_heads import camera_graph
    d = camera_graph()[0]
    B, cw, ch, N = 3, 200, 152, 5
    flags = FULL | VU
    fb = cw * ch * 3 // 2
    batches = [lcg_frame(0xCA400 + 10 * k, B * fb).reshape(B, fb) for k in range(N)]
    m = gpu.Model(d, batch=B)

    def run(fmt_kw, feed):
        m.pipe_open(download_outputs=False, detect=True, camera=(cw, ch), heads=gpu.yolo_heads(conf=0.01), **fmt_kw)
        got = []
        for k in range(N):
            if k >= 3:
                got.append(m.pipe_wait()[1])
            m.pipe_input_view(0)[:] = feed[k]
            m.pipe_submit()
        while len(got) < N:
            got.append(m.pipe_wait()[1])
        m.pipe_close()
        return got

    rgb = [np.stack([nv12_to_rgb_np(b[f], cw, ch, flags) for f in range(B)]).reshape(B, -1) for b in batches]
    want = run({}, rgb)
    got = run(dict(camera_format=gpu.CAMERA_NV12, camera_flags=flags), batches)
    m.close()
    total, xmax = 0, 0.0
    for k in range(N):
        for f in range(B):
            assert got[k][f].tobytes() == want[k][f].tobytes(), (k, f)
            total += len(want[k][f])
            xmax = max([xmax] + [float(v) for v in want[k][f]["x"]])
    assert total > 0 and xmax > 64  # boxes in camera pixels (200 wide), not in the 64 x 64 of the graph input


def test_nv12_error_paths_leave_the_model_usable(gpu, orc):
    d = gpu.synth_model(width_x16=4, input_hw=128, seed=5)
    hdr, tensors, _ = marsfile.parse(d)
    B, w, h = 2, 60, 44
    fb = w * h * 3 // 2
    frames = lcg_frame(0x12E000, B * fb).reshape(B, fb)
    m = gpu.Model(d, batch=B)
    junk = np.zeros(B * fb + 4096, dtype=np.uint8)
    for bw, bh in [(59, 44), (60, 43)]:  # odd w, odd h
        with pytest.raises(RuntimeError):
            gpu.nv12_to_rgb(junk, bw, bh)
        with pytest.raises(RuntimeError):
            gpu.letterbox_nv12(junk, bw, bh, 128, 128)
        with pytest.raises(gpu.MarsError) as ei:
            m.preprocess_nv12(junk, bw, bh)
        assert ei.value.code == gpu.MARS_ERR_INVALID_FILE
        with pytest.raises(gpu.MarsError) as ei:
            m.pipe_open(download_outputs=False, detect=True, det_outputs=(0, 1, 2), camera=(bw, bh), camera_format=gpu.CAMERA_NV12)
        assert ei.value.code == gpu.MARS_ERR_INVALID_FILE
    # flag bit 2
    with pytest.raises(RuntimeError):
        gpu.nv12_to_rgb(frames[0], w, h, flags=4)
    with pytest.raises(RuntimeError):
        gpu.letterbox_nv12(frames[0], w, h, 128, 128, flags=4)
    with pytest.raises(gpu.MarsError) as ei:
        m.preprocess_nv12(frames, w, h, flags=4)
    assert ei.value.code == gpu.MARS_ERR_INVALID_FILE
    with pytest.raises(gpu.MarsError) as ei:
        m.pipe_open(download_outputs=False, detect=True, det_outputs=(0, 1, 2), camera=(w, h), camera_format=gpu.CAMERA_NV12, camera_flags=4)
    assert ei.value.code == gpu.MARS_ERR_INVALID_FILE
    # an unknown camera format
    with pytest.raises(gpu.MarsError) as ei:
        m.pipe_open(download_outputs=False, detect=True, det_outputs=(0, 1, 2), camera=(w, h), camera_format=7)
    assert ei.value.code == gpu.MARS_ERR_INVALID_FILE
    # the model still runs, and right
    m.preprocess_nv12(frames, w, h, flags=VU)
    m.run_device()
    m.download()
    tin = hdr["inputs"][0]
    for f in range(B):
        x = orc.letterbox(nv12_to_rgb_np(frames[f], w, h, VU), 128, 128, 1)
        assert np.array_equal(m.read_tensor(tin, frame=f)[:x.size].view(np.int8), x), f
    g = orc.Graph(d)
    g.set_input(0, x.tobytes())
    assert g.run() == 0
    for oi, ti in enumerate(hdr["outputs"]):
        assert np.array_equal(m.output_view(oi)[B - 1], g.tensor(ti)), oi
    m.close()
