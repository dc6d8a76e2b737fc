"""GPU parity, graph level: mars_load_memory / mars_run through the C-ABI against the CPU
oracle (O2 memory semantics) and the golden vectors of the reference.  Covers the shipped
model files, the synthetic YOLOv5 twins (fused and unfused plans), batching and the
per-layer graphs of test_oracle.py."""
import json
import os
import struct
import zlib

import ctypes as C

import numpy as np
import pytest

import cases
import eltref
import marsfile
from conftest import lcg_frame
from test_oracle import LAYER_KINDS, _layer_graph, model_bytes, model_input

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
GOLD = json.load(open(os.path.join(HERE, "golden", "golden.json")))


@pytest.fixture
def exact_f32(gpu):
    """float32 convolutions in the reference's summation order (bit-identical) for tests that compare digests / bytes;
    the library default (1) sends every convolution with no byte-wise max-pool downstream to the f32 matrix cores"""
    gpu.set_tuning("f32_mfma", 0)
    yield
    gpu.set_tuning("f32_mfma", 1)


def close_f32(got, want, tol=1e-4):
    """north_star's float32 bar: |a-b| <= 1e-4 * max(1, |b|) (NaN == NaN)"""
    a, b = got.view(np.float32).astype(np.float64), want.view(np.float32).astype(np.float64)
    return (np.isnan(a) & np.isnan(b)) | (a == b) | (np.abs(a - b) <= tol * np.maximum(1.0, np.abs(b)))


def run_oracle(orc, d, x):
    g = orc.Graph(d)
    g.set_input(0, x.tobytes())
    rc = g.run()
    return g, rc


@pytest.mark.parametrize("name", cases.SHIPPED)
def test_shipped_models_all_tensors(gpu, orc, name, exact_f32):
    """as shipped: NCHW-tagged, packed-weight bytes walked as OIHW, f32/fp16 bias bytes read as
    int32 -- every activation tensor must equal what the reference leaves (golden + oracle)"""
    d = model_bytes(name)
    hdr, tensors, _ = marsfile.parse(d)
    x = model_input(tensors[hdr["inputs"][0]], "pattern")
    m = gpu.Model(d, fusion=0)
    m.input_view(0)[0, :len(x)] = x
    want = GOLD["models"][name]["pattern"]
    if want["rc"] == 0:
        m.run()
    else:
        with pytest.raises(gpu.MarsError) as e:
            m.run()
        assert e.value.code == want["rc"]
    for ti, dg in want["tensors"].items():
        got = m.read_tensor(int(ti))
        assert cases.digest(got) == dg, "tensor %s" % ti
    out = m.output_view(0)[0]
    assert cases.digest(out) == want["out"]
    m.close()


@pytest.mark.parametrize("name,kw", cases.SYNTH, ids=lambda v: v if isinstance(v, str) else "")
@pytest.mark.parametrize("fusion", [0, 1])
def test_synthetic_models(gpu, orc, name, kw, fusion, exact_f32):
    d = gpu.synth_model(**kw)
    hdr, tensors, _ = marsfile.parse(d)
    tin = tensors[hdr["inputs"][0]]
    B = 3
    xs = [model_input(tin, "lcg")] + [lcg_frame(0x5EED0000 + f, marsfile.tensor_nbytes(tin)) for f in range(1, B)]
    if tin["dtype"] == 0:
        xs = [xs[0]] + [cases.f32(0x5EED0000 + f, marsfile.tensor_nbytes(tin) // 4, 0, 1).view(np.uint8) for f in range(1, B)]
    m = gpu.Model(d, batch=B, fusion=fusion)
    for f in range(B):
        m.input_view(0)[f] = xs[f]
    m.run()
    for f in range(B):
        g, rc = run_oracle(orc, d, xs[f])
        assert rc == 0
        for oi, ti in enumerate(hdr["outputs"]):
            want = g.tensor(ti)
            got = m.output_view(oi)[f]
            if tin["dtype"] == 0:
                # float32 graphs: the task's bar is |a-b| <= 1e-4*max(1,|b|); this build keeps the reference's
                # summation order in the conv and restates libm's expf exactly (csrc/expf_exact.h), so the
                # outputs are in fact bit-identical -- which matters, because byte-moving layers (max-pool on
                # float BYTES) downstream of a sigmoid turn any last-bit difference into garbage
                a, b = got.view(np.float32).astype(np.float64), want.view(np.float32).astype(np.float64)
                ok = (np.isnan(a) & np.isnan(b)) | (a == b) | (np.abs(a - b) <= 1e-4 * np.maximum(1.0, np.abs(b)))
                assert ok.all(), "frame %d output %d: %d values out of tolerance" % (f, oi, int((~ok).sum()))
            assert np.array_equal(got, want), "frame %d output %d: %d bytes differ" % (f, oi, int((got != want).sum()))
        if fusion == 0 and f == 1:  # unfused plan materialises every tensor: check them all, bit for bit
            for ti, t in enumerate(tensors):
                if t["size"] == 0 and marsfile.tensor_nbytes(t):
                    try:
                        got = m.read_tensor(ti, frame=f)
                    except gpu.MarsError:  # written by no layer (no-op kinds): not materialised in HBM
                        assert not g.tensor(ti).any()
                        continue
                    assert np.array_equal(got, g.tensor(ti)), "tensor %d" % ti
    # a second run over the same inputs is idempotent
    first = [m.output_view(i).copy() for i in range(len(hdr["outputs"]))]
    m.run()
    for i in range(len(hdr["outputs"])):
        assert np.array_equal(first[i], m.output_view(i))
    m.close()


@pytest.mark.parametrize("kind", LAYER_KINDS)
def test_single_layer_graphs(gpu, orc, kind, exact_f32):
    d = _layer_graph(kind)
    hdr, tensors, _ = marsfile.parse(d)
    x = model_input(tensors[hdr["inputs"][0]], "lcg")
    g, rc = run_oracle(orc, d, x)
    m = gpu.Model(d, batch=2, fusion=0)
    m.input_view(0)[0] = x
    m.input_view(0)[1] = x[::-1]
    if rc == 0:
        m.run()
    else:
        with pytest.raises(gpu.MarsError) as e:
            m.run()
        assert e.value.code == rc
    for ti, t in enumerate(tensors):
        if t["size"] == 0 and marsfile.tensor_nbytes(t):
            try:
                got = m.read_tensor(ti, frame=0)
            except gpu.MarsError:
                assert not g.tensor(ti).any()  # tensor no layer writes: not materialised on the device
                continue
            want = g.tensor(ti)
            if t["dtype"] == 0 and kind == "f32_chain":  # nothing in that graph is approximate: bit for bit, NaN for NaN (tests/eltref.py)
                eltref.assert_same("f32_chain tensor %d" % ti, got, want, "f32")
            else:
                assert np.array_equal(got, want), "tensor %d" % ti
    m.close()


def test_mars_test_c_call_pattern(gpu):
    """the reference's executor smoke (src/mars/mars_test.c:33-148): init -> load_file -> fill
    alloc_size bytes of the input -> run -> read the output through vaddr -> free"""
    import ctypes as C
    L = gpu.lib()
    p = C.POINTER(gpu.MarsModel)()
    path = os.path.join(HERE, "golden", "models", "tiny_160_int8.mars").encode()
    assert L.mars_load_file(path, C.byref(p)) == 0
    assert L.mars_get_num_inputs(p) == 1 and L.mars_get_num_outputs(p) == 1
    tin = L.mars_get_input(p, 0).contents
    # alloc_size = the reference's shared working-buffer size (largest NDHWC32-rounded activation, :250-334),
    # which is what mars_test.c:73-84 fills -- not the input's own 3*160*160 bytes
    assert tin.vaddr and tin.paddr and tin.alloc_size == GOLD["models"]["tiny_160_int8"]["pattern"]["io_alloc"][0] == 1517824
    assert not L.mars_get_input(p, 1) and not L.mars_get_output(p, -1)
    buf = np.ctypeslib.as_array(C.cast(tin.vaddr, C.POINTER(C.c_int8)), shape=(tin.alloc_size,))
    buf[:] = (np.arange(tin.alloc_size) % 127).astype(np.int8)
    assert L.mars_run(p) == 0 and L.mars_run(p) == 0
    assert p.contents.inference_count == 2 and p.contents.total_inference_us > 0
    tout = L.mars_get_output(p, 0).contents
    out = np.ctypeslib.as_array(C.cast(tout.vaddr, C.POINTER(C.c_uint8)), shape=(tout.alloc_size,))
    nout = L.mars_hip_tensor_frame_bytes(p, p.contents.header.output_tensor_ids[0])
    assert cases.digest(out[:nout]) == GOLD["models"]["tiny_160_int8"]["pattern"]["out"]
    assert not out[nout:].any()
    L.mars_print_summary(p)
    L.mars_free(p)
    assert L.mars_load_file(b"/nonexistent.mars", C.byref(p)) == gpu.MARS_ERR_INVALID_FILE


@pytest.mark.parametrize("name", cases.SHIPPED)
def test_io_alloc_size_is_the_references(gpu, name):
    """row a3: mars_get_input()/mars_get_output()->alloc_size after a load = what the reference's loader reports
    (its shared working-buffer size, mars_runtime.c:250-334), the staging behind vaddr is that large, and a batch
    switches to n densely packed frames"""
    import ctypes as C
    L = gpu.lib()
    want = GOLD["models"][name]["pattern"]["io_alloc"]
    m = gpu.Model(model_bytes(name))
    tin, tout = m.input(0).contents, m.output(0).contents
    assert [tin.alloc_size, tout.alloc_size] == want
    for t in (tin, tout):  # every byte a mars_test.c-style caller touches is there
        buf = np.ctypeslib.as_array(C.cast(t.vaddr, C.POINTER(C.c_uint8)), shape=(t.alloc_size,))
        buf[-1] = buf[0]
    m.set_batch(3)
    fb = L.mars_hip_tensor_frame_bytes(m.p, m.header.input_tensor_ids[0])
    assert m.input(0).contents.alloc_size == 3 * fb
    m.set_batch(1)
    assert m.input(0).contents.alloc_size == want[0]
    m.close()


def test_test_init_c_call_pattern(gpu):
    """the reference's L1 acceptance test (examples/test_init.c:33-131)"""
    import ctypes as C
    L = gpu.lib()
    assert L.nna_init() == 0 and L.nna_is_ready() == 1  # idempotent
    hw = gpu.HwInfo()
    assert L.nna_get_hw_info(C.byref(hw)) == 0
    assert hw.oram_size == 160 * 1024 and hw.version == 950
    p = L.nna_malloc(1 << 20)
    assert p
    C.memset(p, 0xAA, 1 << 20)
    assert C.cast(p, C.POINTER(C.c_ubyte))[0] == 0xAA
    L.nna_free(p)
    L.nna_free(p)  # unknown pointer: logs, does not crash
    q = L.nna_calloc(100, 10)
    assert q and bytes((C.c_ubyte * 1000).from_address(q)) == b"\0" * 1000
    L.nna_free(q)
    assert L.nna_oram_malloc(4096) == 1
    tot, used, free = C.c_size_t(), C.c_size_t(), C.c_size_t()
    assert L.nna_oram_get_stats(C.byref(tot), C.byref(used), C.byref(free)) == 0
    assert tot.value == 160 * 1024 and used.value >= 4096 and free.value == tot.value - used.value
    assert L.nna_lock() == 0 and L.nna_unlock() == 0


def test_full_size_properties(gpu, orc):
    """BASELINE config sizes, through size-independent properties: (i) every frame of a batch
    equals the same frame run alone (frames are independent), (ii) fused == unfused plan,
    (iii) one frame of the full 640x640 yolov5n twin against the CPU oracle."""
    d = gpu.synth_model(width_x16=4, input_hw=640, seed=7)
    hdr, tensors, _ = marsfile.parse(d)
    nb = marsfile.tensor_nbytes(tensors[hdr["inputs"][0]])
    B = 8
    m = gpu.Model(d, batch=B, fusion=1)
    for f in range(B):
        m.input_view(0)[f] = lcg_frame(0x5EED0000 + f, nb)
    m.run()
    outs = [m.output_view(i).copy() for i in range(3)]
    m.set_batch(1)
    for f in (0, 5):
        m.input_view(0)[0] = lcg_frame(0x5EED0000 + f, nb)
        m.run()
        for i in range(3):
            assert np.array_equal(m.output_view(i)[0], outs[i][f])
    m.set_fusion(0)
    m.input_view(0)[0] = lcg_frame(0x5EED0000 + 5, nb)
    m.run()
    for i in range(3):
        assert np.array_equal(m.output_view(i)[0], outs[i][5])
    m.close()
    g, rc = run_oracle(orc, d, lcg_frame(0x5EED0000, nb))
    assert rc == 0
    for i, ti in enumerate(hdr["outputs"]):
        assert np.array_equal(g.tensor(ti), outs[i][0])


def test_config4_yolov5s_twin_640_batch256(gpu, orc):
    """BASELINE configs 3/4 at their own size: the yolov5s_int8 twin (width 8), 640x640, 256 frames on one GPU.
    Frames 0 and 255 against the CPU oracle bit for bit (all three heads), and batch independence: frames of the
    256-batch == the same frames run as a batch of 2; decode+NMS of those frames == the oracle's tail."""
    d = gpu.synth_model(width_x16=8, input_hw=640, seed=1)
    hdr, tensors, _ = marsfile.parse(d)
    nb = marsfile.tensor_nbytes(tensors[hdr["inputs"][0]])
    B = 256
    m = gpu.Model(d, batch=B)
    iv = m.input_view(0)
    for f in range(B):
        iv[f] = lcg_frame(0x5EED0000 + f, nb)
    m.run()
    dets = m.detect(outputs=(0, 1, 2), thresh=0.45)
    outs = [m.output_view(i).copy() for i in range(3)]
    for f in (0, 255):
        g, rc = run_oracle(orc, d, lcg_frame(0x5EED0000 + f, nb))
        assert rc == 0
        parts = []
        for i, ti in enumerate(hdr["outputs"]):
            want = g.tensor(ti)
            assert np.array_equal(want, outs[i][f]), "frame %d head %d: %d bytes differ" % (f, i, int((want != outs[i][f]).sum()))
            parts.append(orc.parse_output(want.view(np.int8), len(want) // 85, np.float32(tensors[ti]["scale"])))
        want_d = orc.nms(np.concatenate(parts)[:1000], 0.45)
        assert dets[f].tobytes() == want_d.tobytes(), "detections of frame %d" % f
        g.close()
    m.set_batch(2)
    for k, f in enumerate((100, 201)):
        m.input_view(0)[k] = lcg_frame(0x5EED0000 + f, nb)
    m.run()
    for k, f in enumerate((100, 201)):
        for i in range(3):
            assert np.array_equal(m.output_view(i)[k], outs[i][f]), "frame %d of the batch != the frame alone" % f
    m.close()


def test_config3_yolov5n_twin_640_batch256(gpu, orc):
    """BASELINE config 3 at its own size: a yolov5n-class int8 graph (the twin at width 4 -- the shipped yolov5n_int8.mars
    is the older compiler's NCHW-tagged file and runs at batch 1 in test_shipped_models_all_tensors), 640x640, 256 frames
    on one GPU, decode + NMS tail on.  Frames 0 and 255 against the CPU oracle bit for bit (all three heads and the kept
    boxes: order, coordinates, confidences, classes), a frame in the middle against the same frame run alone, and the
    pipelined path's detections for frame 255 against the synchronous ones."""
    d = gpu.synth_model(width_x16=4, input_hw=640, seed=1)
    hdr, tensors, _ = marsfile.parse(d)
    nb = marsfile.tensor_nbytes(tensors[hdr["inputs"][0]])
    B = 256
    m = gpu.Model(d, batch=B)
    iv = m.input_view(0)
    for f in range(B):
        iv[f] = lcg_frame(0x5EED0000 + f, nb)
    m.run()
    dets = m.detect(outputs=(0, 1, 2), thresh=0.45)
    outs = [m.output_view(i).copy() for i in range(3)]
    for f in (0, 255):
        g, rc = run_oracle(orc, d, lcg_frame(0x5EED0000 + f, nb))
        assert rc == 0
        parts = []
        for i, ti in enumerate(hdr["outputs"]):
            want = g.tensor(ti)
            assert np.array_equal(want, outs[i][f]), "frame %d head %d: %d bytes differ" % (f, i, int((want != outs[i][f]).sum()))
            parts.append(orc.parse_output(want.view(np.int8), len(want) // 85, np.float32(tensors[ti]["scale"])))
        want_d = orc.nms(np.concatenate(parts)[:1000], 0.45)
        assert dets[f].tobytes() == want_d.tobytes(), "detections of frame %d" % f
        g.close()
    # the double-buffered path at this batch: same detections
    m.pipe_open(download_outputs=False, detect=True, det_outputs=(0, 1, 2), thresh=0.45)
    m.pipe_input_view(0)[:] = iv
    m.pipe_submit()
    _, pd = m.pipe_wait()
    for f in (0, 131, 255):
        assert pd[f].tobytes() == dets[f].tobytes(), "pipelined detections of frame %d" % f
    m.pipe_close()
    m.set_batch(1)
    m.input_view(0)[0] = lcg_frame(0x5EED0000 + 131, nb)
    m.run()
    for i in range(3):
        assert np.array_equal(m.output_view(i)[0], outs[i][131]), "frame 131 of the batch != the frame alone"
    m.close()


def test_config2_tiny160_batch64(gpu, orc):
    """BASELINE config 2: the shipped tiny_160_int8.mars at batch 64.  Frame 0 carries the reference's test pattern
    (mars_test.c:82-84) and must give the golden digest; every other frame is its own LCG frame, checked against the
    oracle (which test_oracle.py pins to the same goldens); a frame in the middle repeats the pattern."""
    d = model_bytes("tiny_160_int8")
    hdr, tensors, _ = marsfile.parse(d)
    tin = tensors[hdr["inputs"][0]]
    nb = marsfile.tensor_nbytes(tin)
    B = 64
    xs = [model_input(tin, "pattern") if f in (0, 37) else lcg_frame(0x5EED0000 + f, nb) for f in range(B)]
    for fusion in (1, 0):
        m = gpu.Model(d, batch=B, fusion=fusion)
        for f in range(B):
            m.input_view(0)[f] = xs[f]
        m.run()
        out = m.output_view(0)
        assert cases.digest(out[0]) == GOLD["models"]["tiny_160_int8"]["pattern"]["out"]
        assert np.array_equal(out[37], out[0])
        want = orc.run_frames(d, np.stack(xs), out.shape[1], nthreads=8)
        for f in range(B):
            assert np.array_equal(out[f], want[f]), "frame %d (fusion %d)" % (f, fusion)
        m.close()


@pytest.mark.parametrize("mode", [3, 4, 2, 1])
def test_config5_yolov5s_f32_twin_640(gpu, orc, mode):
    """BASELINE config 5 at size: the yolov5s_float32 twin (width 8, NCHW/OIHW f32), 640x640, with the float32
    convolutions on the matrix cores -- everywhere on the bf16 cores with split operands (modes 3 / 4 = three / six piece products, conv_f32_split; 3 is what
    bench.py --dtype f32 measures since round 4), everywhere on the f32 cores (mode 2) and under the
    default policy (mode 1: exact upstream of the byte-wise SPPF max-pools, matrix cores for the head).  One frame
    against the CPU oracle within north_star's tolerance |a-b| <= 1e-4*max(1,|b|) on all three heads; frames of a batch
    are independent bit for bit (same kernels, same order)."""
    d = gpu.synth_model(width_x16=8, input_hw=640, seed=1, float32=True)
    hdr, tensors, _ = marsfile.parse(d)
    n = marsfile.tensor_nbytes(tensors[hdr["inputs"][0]]) // 4
    xs = [cases.f32(0x5EED0000 + f, n, 0.0, 1.0).view(np.uint8) for f in range(3)]
    try:
        gpu.set_tuning("f32_mfma", mode)
        m = gpu.Model(d, batch=3)
        for f in range(3):
            m.input_view(0)[f] = xs[f]
        m.run()
        outs = [m.output_view(i).copy() for i in range(3)]
        g, rc = run_oracle(orc, d, xs[1])
        assert rc == 0
        for i, ti in enumerate(hdr["outputs"]):
            ok = close_f32(outs[i][1], g.tensor(ti))
            a = outs[i][1].view(np.float32).astype(np.float64)
            b = g.tensor(ti).view(np.float32).astype(np.float64)
            assert ok.all(), "mode %d head %d: %d of %d values out of tolerance, worst %.3g" % (
                mode, i, int((~ok).sum()), a.size, float(np.nanmax(np.abs(a - b) / np.maximum(1.0, np.abs(b)))))
        g.close()
        m.set_batch(1)
        m.input_view(0)[0] = xs[2]
        m.run()
        for i in range(3):
            assert np.array_equal(m.output_view(i)[0], outs[i][2])
        m.close()
    finally:
        gpu.set_tuning("f32_mfma", 1)


def test_config5_at_batch_256(gpu, orc):
    """BASELINE config 5 AT ITS BATCH (verdict r3: the f32 tests ran at batch <= 3): the yolov5s_float32 twin, 640x640, 256
    frames in one run -- i.e. the two-stream execution of the float kernels -- in mode 3 (split-bf16 matrix-core path, the
    benchmark's).  Frames 0 and 255 against the CPU oracle within |a-b| <= 1e-4*max(1,|b|) on all three heads; frame 128 (the
    first of the second stream's half) bit-identical to a batch-1 run of the same input."""
    d = gpu.synth_model(width_x16=8, input_hw=640, seed=1, float32=True)
    hdr, tensors, _ = marsfile.parse(d)
    n = marsfile.tensor_nbytes(tensors[hdr["inputs"][0]]) // 4
    B = 256
    probe = {0: 0, 255: 1, 128: 2}
    xs = [cases.f32(0x5EED0000 + 7 * k, n, 0.0, 1.0).view(np.uint8) for k in range(3)]
    try:
        gpu.set_tuning("f32_mfma", 3)
        m = gpu.Model(d, batch=B)
        iv = m.input_view(0)
        for f in range(B):
            iv[f] = xs[probe.get(f, f % 3)]
        m.run()
        outs = {f: [m.output_view(i)[f].copy() for i in range(3)] for f in probe}
        m.close()
        for f in (0, 255):
            g, rc = run_oracle(orc, d, xs[probe[f]])
            assert rc == 0
            for i, ti in enumerate(hdr["outputs"]):
                ok = close_f32(outs[f][i], g.tensor(ti))
                a = outs[f][i].view(np.float32).astype(np.float64)
                b = g.tensor(ti).view(np.float32).astype(np.float64)
                assert ok.all(), "frame %d head %d: %d of %d values out of tolerance, worst %.3g" % (
                    f, i, int((~ok).sum()), a.size, float(np.nanmax(np.abs(a - b) / np.maximum(1.0, np.abs(b)))))
            g.close()
        m1 = gpu.Model(d, batch=1)
        m1.input_view(0)[0] = xs[probe[128]]
        m1.run()
        for i in range(3):
            assert np.array_equal(m1.output_view(i)[0], outs[128][i])
        m1.close()
    finally:
        gpu.set_tuning("f32_mfma", 1)


@pytest.mark.parametrize("name,kw", [c for c in cases.SYNTH if c[1].get("float32")], ids=lambda v: v if isinstance(v, str) else "")
def test_f32_matrix_core_path_within_tolerance(gpu, orc, name, kw):
    """float32 convolutions on v_mfma_f32_16x16x4_f32 (modes 2 / 1) and on v_mfma_f32_16x16x32_bf16 with split operands (modes
    3 and 4: three / six piece products) against the oracle, tensor by tensor (unfused plan), on the float twins and the shipped tiny_160_f32.mars.
    * matrix cores everywhere (modes 3, 4 and 2): every float tensor written BEFORE the first byte-wise MAXPOOL / fused-ReLU clamp
      is within 1e-4 of the tensor's magnitude.  (Behind the SPPF pools the reference's byte-maxed floats reach 1e38 and cancel: any
      change of rounding there moves values by percents, in the reference's own terms too -- those tensors say nothing
      about a kernel; the full-size graph outputs are held to the bar by test_config5_yolov5s_f32_twin_640.)
    * default policy (mode 1): the same tensors are BIT-IDENTICAL when a byte-discontinuous layer follows them (the
      policy keeps their convolutions in the reference's order), and the whole of tiny_160_f32 (no such layer) is
      within tolerance on the matrix cores."""
    for d, is_tiny160 in ((gpu.synth_model(**kw), False), (model_bytes("tiny_160_f32"), True)):
        hdr, tensors, layers = marsfile.parse(d)
        tin = tensors[hdr["inputs"][0]]
        x = cases.f32(0x5EED0000 + 3, marsfile.tensor_nbytes(tin) // 4, 0, 1).view(np.uint8)
        g, rc = run_oracle(orc, d, x)
        assert rc == 0
        # tensors written before the first byte-discontinuous layer: MAXPOOL, or a float conv with fused act == RELU
        upstream, hit = [], False
        for L in layers:
            fused_relu = L["type"] == marsfile.CONV2D and struct.unpack_from("<I", L["params"], 48)[0] == 1
            if L["type"] == marsfile.MAXPOOL or fused_relu:
                hit = True
                break
            upstream += list(L["outs"])
        try:
            for mode in (3, 4, 2, 1):
                gpu.set_tuning("f32_mfma", mode)
                m = gpu.Model(d, batch=2, fusion=0)
                m.input_view(0)[0] = x
                m.input_view(0)[1] = x
                m.run()
                checked = 0
                for ti in upstream:
                    t = tensors[ti]
                    if t["size"] or t["dtype"] != 0 or not marsfile.tensor_nbytes(t):
                        continue
                    try:
                        got = m.read_tensor(ti, frame=1)
                    except gpu.MarsError:
                        continue  # written by no layer
                    want = g.tensor(ti)
                    if mode == 1 and hit:
                        assert np.array_equal(got, want), "mode 1 tensor %d must be bit-identical (policy)" % ti
                    else:
                        # a fused multiply-add chain differs from mul-then-add by up to K * 2^-24 * sum|a*w|; where the sum
                        # cancels (random twin weights) that is large relative to the ELEMENT, so the 1e-4 band is taken
                        # against the tensor's magnitude here (graph outputs: element-wise, test_config5_...)
                        a, b = got.view(np.float32).astype(np.float64), want.view(np.float32).astype(np.float64)
                        if not np.isfinite(b).all() or np.abs(b).max() > 1e6:
                            break  # the random-weight twin has no normalisation: from here on tensors run away (1e37, inf)
                        assert np.isfinite(a).all()
                        err, scale = float(np.abs(a - b).max()), max(1.0, float(np.abs(b).max()))
                        assert err <= 1e-4 * scale, "mode %d tensor %d: max error %.3g against magnitude %.3g" % (mode, ti, err, scale)
                        assert close_f32(got, want, 1e-2).sum() >= 0.999 * a.size
                    checked += 1
                assert checked > 0 or not upstream
                m.close()
        finally:
            gpu.set_tuning("f32_mfma", 1)
        g.close()


def test_f32_well_conditioned_twin_element_wise(gpu, orc):
    """VERDICT r4 (weak 1 / next 6): the float kernels' accuracy on numbers that mean something.  The float twins blow up to 1e38 where
    a map width is not a multiple of 4 (the reference's byte-wise CONCAT then cuts floats between bytes: cases.SYNTH "v5n_128_f32");
    at 128 x 128 -- as at config 5's 640 x 640 -- every width is, and the oracle's tensors are 100 % finite and O(0.1).  On the bf16
    matrix cores (modes 3 / 4: conv_f32_patch / conv_f32_stem / conv_f32_split) and on the f32 matrix cores (mode 2):
    * every float tensor written BEFORE the first byte-wise MAXPOOL (unfused plan: each layer's output materialised) is held
      ELEMENT-WISE to |a - b| <= 1e-4 * max(1, |b|) -- the kernels' accuracy, on sane numbers;
    * behind the pools (the reference maxes the BYTES of the floats, mars_runtime.c:919-957: a last-bit difference can flip a byte
      comparison and come out as another float) every tensor, the three heads included, stays 100 % finite with >= 99.5 % of its
      elements inside the same bound, in the unfused and in the fused plan."""
    d = gpu.synth_model(**dict(cases.SYNTH)["v5n_128_f32"])
    hdr, tensors, layers = marsfile.parse(d)
    tin = tensors[hdr["inputs"][0]]
    x = cases.f32(0x5EED0000 + 11, marsfile.tensor_nbytes(tin) // 4, 0, 1).view(np.uint8)
    g, rc = run_oracle(orc, d, x)
    assert rc == 0
    written = [to for L in layers for to in L["outs"] if not tensors[to]["size"] and tensors[to]["dtype"] == 0 and marsfile.tensor_nbytes(tensors[to])]
    first_pool = min(i for i, L in enumerate(layers) if L["type"] == marsfile.MAXPOOL)
    upstream = {to for L in layers[:first_pool] for to in L["outs"]}
    for ti in written:  # the premise: a well-conditioned workload
        b = g.tensor(ti).view(np.float32)
        assert np.isfinite(b).all() and np.abs(b).max() < 1e3, "tensor %d of the oracle: max %g" % (ti, float(np.abs(b).max()))
    try:
        for mode in (3, 4, 2):
            gpu.set_tuning("f32_mfma", mode)
            for fusion in (0, 1):
                m = gpu.Model(d, batch=2, fusion=fusion)
                m.input_view(0)[0] = x
                m.input_view(0)[1] = x
                m.run()
                checked = 0
                for ti in (written if fusion == 0 else list(hdr["outputs"])):
                    try:
                        got = m.read_tensor(ti, frame=1)
                    except gpu.MarsError:
                        continue
                    ok = close_f32(got, g.tensor(ti))
                    a = got.view(np.float32)
                    assert np.isfinite(a).all(), "mode %d tensor %d: %.4f finite" % (mode, ti, float(np.isfinite(a).mean()))
                    if ti in upstream:
                        assert ok.all(), "mode %d fusion %d tensor %d: %d of %d outside 1e-4" % (mode, fusion, ti, int((~ok).sum()), ok.size)
                    else:
                        assert ok.mean() >= 0.995, "mode %d fusion %d tensor %d (behind the byte-wise pools): %d of %d outside 1e-4" % (
                            mode, fusion, ti, int((~ok).sum()), ok.size)
                    checked += 1
                assert checked >= (50 if fusion == 0 else 3)
                m.close()
    finally:
        gpu.set_tuning("f32_mfma", 1)
    g.close()


def test_detect_on_model_outputs(gpu, orc):
    """decode + NMS over the three head tensors of a batch == the reference tail on the
    concatenated [sum(H*W*3), 85] prediction list of each frame"""
    d = gpu.synth_model(width_x16=4, input_hw=128, seed=11)
    hdr, tensors, _ = marsfile.parse(d)
    nb = marsfile.tensor_nbytes(tensors[hdr["inputs"][0]])
    B = 4
    m = gpu.Model(d, batch=B)
    for f in range(B):
        m.input_view(0)[f] = lcg_frame(0x5EED0000 + f, nb)
    m.run()
    dets = m.detect(outputs=(0, 1, 2), thresh=0.45)
    scale = np.float32(tensors[hdr["outputs"][0]]["scale"])
    for f in range(B):
        pred = np.concatenate([m.output_view(i)[f] for i in range(3)]).view(np.int8)
        raw = orc.parse_output(pred, len(pred) // 85, scale)
        want = orc.nms(raw, 0.45)
        assert len(raw) > 10
        assert dets[f].tobytes() == want.tobytes()
    # pipelined form used by bench.py: graph on the main stream, tail on the auxiliary stream, no
    # host sync in between; the next graph's output layers wait for the previous tail by event
    import ctypes as C
    for _ in range(3):
        m.run_device(sync=False)
        m.detect_device(outputs=(0, 1, 2), thresh=0.45)
    assert gpu.lib().mars_hip_sync() == 0
    again = m.detect(outputs=(0, 1, 2), thresh=0.45)
    for f in range(B):
        assert again[f].tobytes() == dets[f].tobytes()
    m.close()


@pytest.mark.parametrize("width,hw,seed,B", [(4, 128, 698702, 3), (8, 160, 911481, 2), (4, 224, 911456, 3), (8, 96, 335533, 5)])
def test_varied_scale_twins_with_tail(gpu, orc, width, hw, seed, B):
    """twins whose every convolution has its own scales, several frames: graph outputs and the detection tail (each head
    decoded with ITS scale, candidates capped at 1000 in order) against the oracle"""
    d = gpu.synth_model(width_x16=width, input_hw=hw, seed=seed, vary_scales=True)
    hdr, tensors, _ = marsfile.parse(d)
    nb = marsfile.tensor_nbytes(tensors[hdr["inputs"][0]])
    m = gpu.Model(d, batch=B)
    xs = [lcg_frame(seed * 16 + f, nb) for f in range(B)]
    for f in range(B):
        m.input_view(0)[f] = xs[f]
    m.run()
    dets = m.detect(outputs=(0, 1, 2), thresh=0.45)
    for f in range(B):
        g, rc = run_oracle(orc, d, xs[f])
        assert rc == 0
        parts = []
        for oi, ti in enumerate(hdr["outputs"]):
            assert np.array_equal(m.output_view(oi)[f], g.tensor(ti)), (f, oi)
            pred = g.tensor(ti).view(np.int8)
            parts.append(orc.parse_output(pred, len(pred) // 85, np.float32(tensors[ti]["scale"])))
        raw = np.concatenate(parts)[:1000]
        assert len(raw) > 10
        assert dets[f].tobytes() == orc.nms(raw, 0.45).tobytes()
    m.close()


def _silu_conv(G, rng, x, in_c, out_c, hw, k, s_conv, s_sig, s_out, wscale=0.004):
    """conv -> sigmoid -> mul with its own three scales (the plan folds the chain into the conv's LUT epilogue)"""
    a = G.tensor([1, hw, hw, out_c], scale=s_conv)
    g = G.tensor([1, hw, hw, out_c], scale=s_sig)
    o = G.tensor([1, hw, hw, out_c], scale=s_out)
    wt = G.tensor([out_c, k, k, in_c], scale=wscale, data=rng.integers(-127, 128, (out_c, k, k, in_c), dtype=np.int8))
    b = G.tensor([out_c], dtype=marsfile.I32, scale=1.0, data=rng.integers(-2000, 2000, out_c, dtype=np.int32))
    G.conv(x, a, wt, b, (k, k), (1, 1))
    G.layer(marsfile.SIGMOID, [a], [g])
    G.layer(marsfile.MUL, [a, g], [o])
    return o


@pytest.mark.parametrize("c,slots", [(32, 0), (64, 3), (128, 0), (128, 5), (256, 0)])
def test_paired_convs_own_tables(gpu, orc, c, slots):
    """C3 shape: cv1 and cv2 over one input run as one grid, each with its OWN fused SiLU table (different scales on
    the two branches); a 1x1 follows cv1, a concat of both branches is read through (never materialised) by cv3 and
    another 1x1 follows that"""
    rng = np.random.default_rng(c + slots)
    hw = 24
    G = marsfile.Graph()
    x = G.tensor([1, hw, hw, c], scale=0.04)
    cv1 = _silu_conv(G, rng, x, c, c // 2 if c <= 128 else c, hw, 1, 0.05, 1.0 / 256, 0.03)
    cv2 = _silu_conv(G, rng, x, c, c // 2 if c <= 128 else c, hw, 1, 0.09, 1.0 / 200, 0.07)
    cm = c // 2 if c <= 128 else c
    m1 = _silu_conv(G, rng, cv1, cm, cm, hw, 1, 0.06, 1.0 / 256, 0.045, wscale=0.01)
    cat = G.tensor([1, hw, hw, 2 * cm], scale=0.05)
    G.concat([m1, cv2], cat)
    cv3 = _silu_conv(G, rng, cat, 2 * cm, cm, hw, 1, 0.07, 1.0 / 256, 0.05)      # reads the virtual concat
    m2 = _silu_conv(G, rng, cv3, cm, cm, hw, 1, 0.05, 1.0 / 256, 0.04, wscale=0.01)  # chained behind it
    d = G.serialise([x], [m2, cv1, cv3])
    hdr, tensors, _ = marsfile.parse(d)
    B = 3
    try:
        gpu.set_tuning("persist_slots", slots)
        m = gpu.Model(d, batch=B)
        xs = [lcg_frame(0xC4A100 + f, hw * hw * c) for f in range(B)]
        for f in range(B):
            m.input_view(0)[f] = xs[f]
        m.run()
        for f in range(B):
            g, rc = run_oracle(orc, d, xs[f])
            assert rc == 0
            for oi, ti in enumerate(hdr["outputs"]):
                want = g.tensor(ti)
                assert np.array_equal(m.output_view(oi)[f], want), (c, f, oi, int((m.output_view(oi)[f] != want).sum()))
                assert len(np.unique(want)) > 16
        m.close()
    finally:
        gpu.set_tuning("persist_slots", 0)


@pytest.mark.parametrize("out_c", [255, 170, 100])
def test_padded_output_rows(gpu, orc, out_c):
    """graph outputs with ragged pixel rows are kept at a 16-byte-aligned pitch on the device (pad_output_rows):
    mars_get_output bytes, mars_hip_read_tensor (whole and partial), mars_hip_write_tensor and the detection tail
    (anchors per pixel, and the per-byte mapping of a channel count that is no multiple of 85) all see the
    reference's dense layout"""
    import ctypes as C
    rng = np.random.default_rng(out_c)
    G = marsfile.Graph()
    x = G.tensor([1, 16, 16, 32], scale=0.03)
    o = G.tensor([1, 16, 16, out_c], scale=0.07)
    wt = G.tensor([out_c, 1, 1, 32], scale=0.004, data=rng.integers(-127, 128, (out_c, 1, 1, 32), dtype=np.int8))
    b = G.tensor([out_c], dtype=marsfile.I32, scale=1.0, data=rng.integers(-3000, 3000, out_c, dtype=np.int32))
    G.conv(x, o, wt, b, (1, 1), (1, 1))
    d = G.serialise([x], [o])
    hdr, tensors, _ = marsfile.parse(d)
    ti = hdr["outputs"][0]
    B = 3
    m = gpu.Model(d, batch=B)
    rb = C.c_int(0)
    assert gpu.lib().mars_hip_tensor_row_pitch(m.p, ti, C.byref(rb)) == (out_c + 15) // 16 * 16 and rb.value == out_c
    xs = [lcg_frame(0xFACE00 + f, 16 * 16 * 32) for f in range(B)]
    for f in range(B):
        m.input_view(0)[f] = xs[f]
    m.run()
    dets = m.detect(outputs=(0,), thresh=0.45)
    for f in range(B):
        g, rc = run_oracle(orc, d, xs[f])
        assert rc == 0
        want = g.tensor(ti)
        assert np.array_equal(m.output_view(0)[f], want)
        assert np.array_equal(m.read_tensor(ti, frame=f), want)
        assert np.array_equal(m.read_tensor(ti, frame=f, nbytes=3 * out_c + 17), want[:3 * out_c + 17])
        pred = want.view(np.int8)
        raw = orc.parse_output(pred, len(pred) // 85, np.float32(0.07))
        assert len(raw) > 5
        assert dets[f].tobytes() == orc.nms(raw, 0.45).tobytes()
    # write whole pixels back and read them again
    fresh = rng.integers(0, 256, 16 * 16 * out_c, dtype=np.uint8)
    assert gpu.lib().mars_hip_write_tensor(m.p, ti, 1, fresh.ctypes.data, fresh.size) == 0
    assert np.array_equal(m.read_tensor(ti, frame=1), fresh)
    m.close()


def test_autotune_keeps_results(gpu, orc):
    """mars_hip_autotune pins, per conv layer, the fastest of its launch variants; every variant writes the same
    bytes, so outputs before and after (and the oracle's) are identical"""
    d = gpu.synth_model(width_x16=4, input_hw=160, seed=5)
    hdr, tensors, _ = marsfile.parse(d)
    nb = marsfile.tensor_nbytes(tensors[hdr["inputs"][0]])
    B = 4
    m = gpu.Model(d, batch=B)
    xs = [lcg_frame(0xC0FFEE00 + f, nb) for f in range(B)]
    for f in range(B):
        m.input_view(0)[f] = xs[f]
    m.run()
    before = [m.output_view(i).copy() for i in range(3)]
    m.autotune(2)
    m.run()
    for i in range(3):
        assert np.array_equal(before[i], m.output_view(i))
    g, rc = run_oracle(orc, d, xs[2])
    assert rc == 0
    for i, ti in enumerate(hdr["outputs"]):
        assert np.array_equal(g.tensor(ti), m.output_view(i)[2])
    m.close()


@pytest.mark.parametrize("order", ["conv_first", "conv_second"])
@pytest.mark.parametrize("ic,hw", [(32, 48), (64, 40), (128, 24)])
def test_residual_add_folded_into_conv(gpu, orc, order, ic, hw):
    """x -> conv1x1 -> t1 -> conv3x3 -> t2; out = Add(t1, t2) in either operand order (different scales per
    operand): the fused plan folds the Add into the 3x3 convolution's epilogue (one launch fewer) and must produce
    the reference's bytes; covers the patch-staged (32/64 channels, 48/40 wide) and the one-tile MFMA epilogue"""
    rng = np.random.default_rng(ic + hw)
    G = marsfile.Graph()
    x = G.tensor([1, hw, hw, ic], scale=0.04)
    t1 = G.tensor([1, hw, hw, ic], scale=0.031)
    t2 = G.tensor([1, hw, hw, ic], scale=0.027)
    o = G.tensor([1, hw, hw, ic], scale=0.045)
    w1 = G.tensor([ic, 1, 1, ic], scale=0.02, data=rng.integers(-127, 128, (ic, 1, 1, ic), dtype=np.int8))
    b1 = G.tensor([ic], dtype=marsfile.I32, data=rng.integers(-300, 300, ic, dtype=np.int32))
    w2 = G.tensor([ic, 3, 3, ic], scale=0.01, data=rng.integers(-127, 128, (ic, 3, 3, ic), dtype=np.int8))
    b2 = G.tensor([ic], dtype=marsfile.I32, data=rng.integers(-300, 300, ic, dtype=np.int32))
    G.conv(x, t1, w1, b1, (1, 1), (1, 1))
    G.conv(t1, t2, w2, b2, (3, 3), (1, 1))
    G.layer(marsfile.ADD, [t2, t1] if order == "conv_first" else [t1, t2], [o])
    d = G.serialise([x], [o])
    B = 3
    xs = [rng.integers(-128, 128, hw * hw * ic, dtype=np.int8).view(np.uint8) for _ in range(B)]
    outs = {}
    nops = {}
    for fusion in (0, 1):
        m = gpu.Model(d, batch=B, fusion=fusion)
        for f in range(B):
            m.input_view(0)[f] = xs[f]
        m.run()
        outs[fusion] = m.output_view(0).copy()
        nops[fusion] = len(m.ops())
        m.close()
    assert nops[1] == nops[0] - 1  # the Add launch is gone
    for f in range(B):
        g, rc = run_oracle(orc, d, xs[f])
        assert rc == 0
        want = g.tensor(o)
        assert len(np.unique(want)) > 32
        assert np.array_equal(outs[0][f], want)
        assert np.array_equal(outs[1][f], want)


@pytest.mark.parametrize("order", ["conv_first", "conv_second"])
@pytest.mark.parametrize("ic,hw", [(16, 24), (48, 20)])
def test_residual_add_folded_into_conv_f32(gpu, orc, order, ic, hw):
    """the float32 form (round 4): x -> conv1x1 -> SIGMOID -> MUL -> t1 -> conv3x3 -> SIGMOID -> MUL -> t2; out = Add(t1, t2).
    The fused plan evaluates both SiLU chains and the Add in the convolutions' epilogues (5 launches fewer).  In the
    reference's summation order (f32_mfma = 0) fused and unfused plans are BIT-IDENTICAL to the oracle; on the bf16 matrix
    cores (modes 3 / 4) the fused plan stays within 1e-4 * max(1, |b|)."""
    rng = np.random.default_rng(ic * 100 + hw)
    G = marsfile.Graph()
    F, N = marsfile.F32, marsfile.NCHW

    def act():
        return G.tensor([1, ic, hw, hw], dtype=F, fmt=N)

    def conv_silu(x, k):
        a, g, o = act(), act(), act()
        amp = 1.7 / (k * k * ic) ** 0.5
        w = G.tensor([ic, ic, k, k], dtype=F, fmt=marsfile.OIHW, data=((rng.random((ic, ic, k, k), dtype=np.float32) * 2 - 1) * amp).astype(np.float32))
        b = G.tensor([ic], dtype=F, fmt=marsfile.D1, data=((rng.random(ic, dtype=np.float32) * 2 - 1) * 0.1).astype(np.float32))
        G.conv(x, a, w, b, (k, k), (1, 1))
        G.layer(marsfile.SIGMOID, [a], [g])
        G.layer(marsfile.MUL, [a, g], [o])
        return o

    x = act()
    t1 = conv_silu(x, 1)
    t2 = conv_silu(t1, 3)
    o = act()
    G.layer(marsfile.ADD, [t2, t1] if order == "conv_first" else [t1, t2], [o])
    d = G.serialise([x], [o])
    B = 3
    xs = [(rng.random(ic * hw * hw, dtype=np.float32) * 2 - 1).astype(np.float32).view(np.uint8) for _ in range(B)]
    want = []
    for f in range(B):
        g, rc = run_oracle(orc, d, xs[f])
        assert rc == 0
        want.append(g.tensor(o).copy())
        g.close()
    try:
        nops = {}
        for mode in (0, 3, 4):
            gpu.set_tuning("f32_mfma", mode)
            for fusion in (0, 1):
                m = gpu.Model(d, batch=B, fusion=fusion)
                for f in range(B):
                    m.input_view(0)[f] = xs[f]
                m.run()
                got = m.output_view(0).copy()
                nops[fusion] = len(m.ops())
                m.close()
                for f in range(B):
                    if mode == 0:
                        assert np.array_equal(got[f], want[f]), "mode 0 fusion %d frame %d" % (fusion, f)
                    else:
                        assert close_f32(got[f], want[f]).all(), "mode %d fusion %d frame %d" % (mode, fusion, f)
            assert nops[1] == nops[0] - 5  # two SIGMOID + MUL pairs and the Add are gone
    finally:
        gpu.set_tuning("f32_mfma", 1)


import f32shapes  # noqa: E402  (the shape lists and their graphs: shared with tests/golden/make_golden.py)

F32_SPLIT_SHAPES = f32shapes.SPLIT


@pytest.mark.parametrize("shape", F32_SPLIT_SHAPES, ids=lambda v: "x".join(str(q) for q in v))
def test_conv_f32_split_shapes(gpu, orc, shape):
    """one float32 convolution (+ fused SIGMOID / MUL) on the bf16 matrix cores with split operands, modes 3 (two pieces,
    three products) and 4 (three pieces, six products), over the gather forms, tile sizes, ragged channel counts, tile
    counts above and below the persistent grid, and a shape the kernel declines; every frame of the batch against the
    oracle within 1e-4 * max(1, |b|), and mode 0 bit-identical (the same plan through the reference-order kernel)"""
    h, w, ic, oc, k, st, pad, B, silu = shape
    case = f32shapes.split_case(shape)
    d, out, ow = case["d"], case["out"], case["ow"]
    xs = [q.view(np.uint8) for q in case["xs"]]
    ref = GOLD["conv_f32_family"][f32shapes.shape_id("split", shape)]  # the REFERENCE's output for each input, by digest
    want = []
    for q in xs:
        g, rc = run_oracle(orc, d, q)
        assert rc == 0
        want.append(g.tensor(out).copy())
        g.close()
    try:
        gpu.set_tuning("dual_stream_min_batch", 0)  # one launch over the whole batch: the 64-frame case must walk two tiles per workgroup
        for mode in (3, 4, 0):
            gpu.set_tuning("f32_mfma", mode)
            m = gpu.Model(d, batch=B)
            for f in range(B):
                m.input_view(0)[f] = xs[f % len(xs)]
            count = gpu.lib().mhip_conv_f32_split_launches
            count.restype = C.c_ulong
            n0 = count()
            m.run()
            declined = st == 2 and ow % 2 == 1  # (the one shape above the split kernel does not take)
            stem = mode == 3 and ic == 3 and k == 6  # round 5: in mode 3 the stem's geometry goes to conv_f32_stem (test_conv_f32_stem_shapes)
            assert count() - n0 == (0 if mode == 0 or declined or stem else 1), "mode %d: conv_f32_split launched %d time(s)" % (mode, count() - n0)
            got = m.output_view(0).copy()
            m.close()
            for f in range(B):
                if mode == 0:
                    assert np.array_equal(got[f], want[f % len(xs)]), "mode 0 frame %d" % f
                    assert cases.digest(got[f]) == ref[f % len(xs)], "mode 0 frame %d: not the reference's bytes" % f
                else:
                    ok = close_f32(got[f], want[f % len(xs)])
                    assert ok.all(), "mode %d frame %d: %d of %d out of tolerance" % (mode, f, int((~ok).sum()), ok.size)
    finally:
        gpu.set_tuning("f32_mfma", 1)
        gpu.set_tuning("dual_stream_min_batch", 64)


F32_PATCH_SHAPES = f32shapes.PATCH


@pytest.mark.parametrize("shape", F32_PATCH_SHAPES, ids=lambda v: "x".join(str(q) for q in v))
def test_conv_f32_patch_shapes(gpu, orc, shape):
    """one float32 k x k convolution (+ fused SIGMOID / MUL, + fused residual Add) through conv_f32_patch (mode 3: the input patch of a
    pixel tile staged and split once, csrc/hip/conv_f32_patch.hip): every frame of the batch against the oracle within
    1e-4 * max(1, |b|); the launch counter proves the kernel ran (and that mode 4 / mode 0 do not take it).  Run twice: one
    workgroup per CU (the default), and `persist_slots` = 3, so that three workgroups walk ALL tiles (runs of many tiles: the
    patch ring, the weight pipeline and the row tables carried through tile boundaries)."""
    h, w, ic, oc, k, st, B, silu, add = shape
    case = f32shapes.patch_case(shape)
    d, out, xs = case["d"], case["out"], case["xs"]
    nx = len(xs)
    rs = case["rs"] if add else [None] * nx
    ref = GOLD["conv_f32_family"][f32shapes.shape_id("patch", shape)]
    want = []
    for q, r in zip(xs, rs):
        g = orc.Graph(d)
        g.set_input(0, q.tobytes())
        if add:
            g.set_input(1, r.tobytes())
        assert g.run() == 0
        want.append(g.tensor(out).copy())
        g.close()
    count = gpu.lib().mhip_conv_f32_patch_launches
    count.restype = C.c_ulong
    try:
        gpu.set_tuning("dual_stream_min_batch", 0)
        for mode, slots in ((3, 0), (3, 3), (4, 0), (0, 0)):
            gpu.set_tuning("f32_mfma", mode)
            gpu.set_tuning("persist_slots", slots)
            m = gpu.Model(d, batch=B)
            for f in range(B):
                m.input_view(0)[f] = xs[f % nx].view(np.uint8)
                if add:
                    m.input_view(1)[f] = rs[f % nx].view(np.uint8)
            n0 = count()
            m.run()
            assert count() - n0 == (1 if mode == 3 else 0), "mode %d: conv_f32_patch launched %d time(s)" % (mode, count() - n0)
            got = m.output_view(0).copy()
            m.close()
            for f in range(B):
                if mode == 0:
                    assert np.array_equal(got[f], want[f % nx]), "mode 0 frame %d" % f
                    assert cases.digest(got[f]) == ref[f % nx], "mode 0 frame %d: not the reference's bytes" % f
                else:
                    ok = close_f32(got[f], want[f % nx])
                    assert ok.all(), "mode %d slots %d frame %d: %d of %d out of tolerance" % (mode, slots, f, int((~ok).sum()), ok.size)
    finally:
        gpu.set_tuning("f32_mfma", 1)
        gpu.set_tuning("persist_slots", 0)
        gpu.set_tuning("dual_stream_min_batch", 64)


@pytest.mark.parametrize("shape", [(256, 20, 20, 5, 5), (37, 13, 12, 5, 5), (9, 7, 4, 3, 3), (16, 16, 20, 2, 7), (40, 9, 36, 8, 1), (5, 3, 8, 8, 8), (64, 40, 24, 5, 5)],
                         ids=lambda v: "x".join(str(q) for q in v))
def test_maxpool_rows_form(gpu, orc, shape):
    """stride-1 MAXPOOL over [H][W][C] bytes with C a multiple of 4 but not of 16 -- what the float twins' byte-wise pools are (a 20 x 20 x 256
    float map read as H = 256, W = 20, C = 20) -- through the separable kernel (move.hip maxpool_rows_kernel): bit-identical to the
    oracle on every frame, windows clipped at the right and bottom edge, kernels up to 8 x 8, windows larger than the map."""
    H, W, Cc, kh, kw = shape
    G = marsfile.Graph()
    a = G.tensor([1, H, W, Cc], scale=0.05)
    o = G.tensor([1, H, W, Cc], scale=0.05)
    G.pool(a, o, (kh, kw), (1, 1))
    d = G.serialise([a], [o])
    rng = np.random.default_rng(H * 100 + W + Cc)
    B = 3
    xs = [rng.integers(0, 256, H * W * Cc, dtype=np.uint8) for _ in range(B)]
    m = gpu.Model(d, batch=B)
    for f in range(B):
        m.input_view(0)[f] = xs[f]
    m.run()
    got = m.output_view(0).copy()
    m.close()
    for f in range(B):
        g, rc = run_oracle(orc, d, xs[f])
        assert rc == 0
        assert np.array_equal(got[f], g.tensor(o)), "frame %d" % f
        g.close()


F32_REC_CHAINS = [
    # h, w, c0, producer (out_c, k, stride), consumer (out_c, k, stride), batch, residual   conv -> k x k conv with the tensor between them in record format
    (20, 20, 64, (32, 1, 1), (16, 3, 1), 3, None),       # a C3 bottleneck's pair on a 20-wide map (whole-row tiles), 4 chunks, 4 dummy units
    (12, 40, 64, (64, 1, 1), (64, 3, 1), 5, "x"),        # ... with the shortcut: Add(cv2(cv1(x)), x) folded into the second convolution
    (40, 40, 128, (128, 1, 1), (128, 3, 1), 4, "x"),     # the 40 x 40 bottleneck of the twins: 128-channel tiles on both sides, 16 chunks, four ring slots
    (24, 160, 48, (32, 1, 1), (64, 3, 1), 2, None),      # wide map: 2-D tiles out of 32-column strips
    (40, 40, 48, (32, 1, 1), (130, 3, 2), 3, None),      # stride-2 reader (de-interleaved patch columns), two 128-channel tiles
    (32, 160, 16, (64, 3, 2), (32, 3, 2), 2, None),      # the writer is a stride-2 3 x 3 on 16 channels (conv_f32_split's paired gather), the reader stride 2 on the 80-wide map
    (16, 24, 40, (32, 1, 1), (24, 5, 1), 4, "r"),        # 5 x 5 reader, residual from a third tensor
    (9, 20, 96, (96, 1, 1), (128, 3, 1), 37, "r"),       # short frames: frame boundaries inside a tile; 12 chunks (two ring slots: 12 % 4 == 0 -> four); 27 tiles
    (80, 80, 64, (64, 1, 1), (64, 3, 1), 9, "x"),        # 113 tiles of 512 pixels: every workgroup walks a run of tiles
    (64, 64, 3, (32, 6, 2), (64, 3, 2), 9, None),        # the twins' first two layers: conv_f32_stem writes the records, layer 3 reads them
    (128, 160, 3, (24, 6, 2), (40, 3, 2), 3, None),      # ... 24 of the stem's 32 channels (3 chunks -> the reader declines: fewer than 4) -- stays NCHW floats
]


@pytest.mark.parametrize("shape", F32_REC_CHAINS, ids=lambda v: "x".join(str(q) for q in v).replace(" ", ""))
def test_conv_f32_record_pairs(gpu, orc, shape):
    """two float32 convolutions in a row (each + SIGMOID / MUL), the second k x k: under f32_mfma = 3 the planner keeps the tensor
    between them in RECORD format (mars_plan.c rec_pairs: the first writes the two bf16 pieces channels-last, the second fills its patch
    ring by LDS-DMA -- conv_f32_prec).  Every frame of the batch against the oracle within 1e-4 * max(1, |b|); the launch counters prove
    which kernels ran; the tensor between them reads back (mars_hip_read_tensor converts) as the oracle's floats to 2^-15; at fusion
    level 0 and in the other modes nothing is in record format and the results are the same."""
    h, w, c0, (c1, k1, s1), (c2, k2, s2), B, res = shape
    rng = np.random.default_rng(h * 1000 + w * 10 + c1 + c2)
    G = marsfile.Graph()
    F, N = marsfile.F32, marsfile.NCHW

    def conv_silu(xin, ic, ih, iw, oc, k, st):
        oh, ow = (ih + st - 1) // st, (iw + st - 1) // st
        a = G.tensor([1, oc, oh, ow], dtype=F, fmt=N)
        amp = 1.7 / (k * k * ic) ** 0.5
        wt = G.tensor([oc, ic, k, k], dtype=F, fmt=marsfile.OIHW, data=((rng.random((oc, ic, k, k), dtype=np.float32) * 2 - 1) * amp).astype(np.float32))
        b = G.tensor([oc], dtype=F, fmt=marsfile.D1, data=((rng.random(oc, dtype=np.float32) * 2 - 1) * 0.1).astype(np.float32))
        G.conv(xin, a, wt, b, (k, k), (st, st), pad=marsfile.PAD_SAME)
        g_, o_ = G.tensor([1, oc, oh, ow], dtype=F, fmt=N), G.tensor([1, oc, oh, ow], dtype=F, fmt=N)
        G.layer(marsfile.SIGMOID, [a], [g_])
        G.layer(marsfile.MUL, [a, g_], [o_])
        return o_, oh, ow

    x = G.tensor([1, c0, h, w], dtype=F, fmt=N)
    t1, h1, w1 = conv_silu(x, c0, h, w, c1, k1, s1)
    t2, h2, w2 = conv_silu(t1, c1, h1, w1, c2, k2, s2)
    ins, out = [x], t2
    if res == "x":
        assert (c2, h2, w2) == (c0, h, w)
        out = G.tensor([1, c2, h2, w2], dtype=F, fmt=N)
        G.layer(marsfile.ADD, [t2, x], [out])
    elif res == "r":
        r_ = G.tensor([1, c2, h2, w2], dtype=F, fmt=N)
        out = G.tensor([1, c2, h2, w2], dtype=F, fmt=N)
        G.layer(marsfile.ADD, [t2, r_], [out])
        ins.append(r_)
    d = G.serialise(ins, [out])
    nx = min(B, 4)
    xs = [(rng.random(c0 * h * w, dtype=np.float32) * 2 - 1).astype(np.float32) for _ in range(nx)]
    rs = [(rng.random(c2 * h2 * w2, dtype=np.float32) * 2 - 1).astype(np.float32) for _ in range(nx)]
    want, mid = [], []
    for q, r in zip(xs, rs):
        g = orc.Graph(d)
        g.set_input(0, q.tobytes())
        if res == "r":
            g.set_input(1, r.tobytes())
        assert g.run() == 0
        want.append(g.tensor(out).copy())
        mid.append(g.tensor(t1).copy())
        g.close()
    L = gpu.lib()
    counts = {}
    for name in ("prec", "recin", "patch", "split", "stem"):
        counts[name] = getattr(L, "mhip_conv_f32_%s_launches" % name)
        counts[name].restype = C.c_ulong
    geom2 = L.mhip_conv_f32_patch_geom2
    geom2.restype = C.c_int
    geom2.argtypes = [C.c_int] * 11 + [C.c_void_p, C.c_int]
    gv = np.zeros(64, dtype=np.int32)
    pad2 = (k2 - 1) // 2 if s2 == 1 else max(0, ((h2 - 1) * s2 + k2 - h1)) // 2  # SAME, as the planner derives it (top = left)
    expect_patch = geom2(c2, c1, k2, k2, s2, pad2, h1, w1, h2, w2, 0, gv.ctypes.data, 64) != 0
    form_of = L.mhip_conv_f32_patch_rec_form
    form_of.restype = C.c_int
    form_of.argtypes = [C.c_int] * 10
    form = form_of(c2, c1, k2, k2, s2, pad2, h1, w1, h2, w2)  # 1: conv_f32_prec (four ring slots fit), 2: conv_f32_patch's record-input form (two slots, through registers), 0: none
    expect_rec = form != 0
    try:
        gpu.set_tuning("dual_stream_min_batch", 0)
        for mode, slots, fusion in ((3, 0, 1), (3, 3, 1), (3, 0, 0), (4, 0, 1), (0, 0, 1)):
            gpu.set_tuning("f32_mfma", mode)
            gpu.set_tuning("persist_slots", slots)
            m = gpu.Model(d, batch=B, fusion=fusion)
            for f in range(B):
                m.input_view(0)[f] = xs[f % nx].view(np.uint8)
                if res == "r":
                    m.input_view(1)[f] = rs[f % nx].view(np.uint8)
            n0 = {k_: c() for k_, c in counts.items()}
            m.run()
            dn = {k_: c() - n0[k_] for k_, c in counts.items()}
            rec = mode == 3 and fusion == 1 and expect_rec
            assert dn["prec"] == (1 if rec and form == 1 else 0) and dn["recin"] == (1 if rec and form == 2 else 0), (mode, slots, fusion, form, dn)
            if mode == 3:
                assert dn["patch"] == (0 if rec or not expect_patch else 1), (mode, fusion, dn)
                assert dn["split"] + dn["stem"] + dn["patch"] + dn["prec"] + dn["recin"] == 2, dn
            got = m.output_view(0).copy()
            if fusion == 1:  # the tensor between the two (the first MUL's output): NCHW floats whatever its device format is
                for f in (0, B - 1):
                    t = np.frombuffer(m.read_tensor(t1, f), dtype=np.float32)
                    w_ = mid[f % nx].view(np.float32)
                    tol = 2.0 ** -15 if rec else 1e-4
                    assert (np.abs(t.astype(np.float64) - w_) <= np.maximum(1e-4, tol * np.abs(w_))).all(), "mode %d: tensor between the convolutions, frame %d" % (mode, f)
                if rec and slots == 0:  # ... and written: mars_hip_write_tensor cuts the floats into the two pieces the kernels would have stored
                    probe = (np.random.default_rng(5).random(c1 * h1 * w1, dtype=np.float32) * 4 - 2).astype(np.float32)
                    pb = probe.view(np.uint8)
                    assert gpu.lib().mars_hip_write_tensor(m.p, t1, 1 % B, pb.ctypes.data, pb.size) == 0
                    back = m.read_tensor(t1, 1 % B).view(np.float32)
                    assert (np.abs(back.astype(np.float64) - probe) <= 2.0 ** -16 * np.abs(probe)).all(), "write_tensor / read_tensor round trip of a record-format tensor"
            m.close()
            for f in range(B):
                if mode == 0:
                    assert np.array_equal(got[f], want[f % nx]), "mode 0 frame %d" % f
                else:
                    ok = close_f32(got[f], want[f % nx])
                    assert ok.all(), "mode %d slots %d fusion %d frame %d: %d of %d out of tolerance" % (mode, slots, fusion, f, int((~ok).sum()), ok.size)
    finally:
        gpu.set_tuning("f32_mfma", 1)
        gpu.set_tuning("persist_slots", 0)
        gpu.set_tuning("dual_stream_min_batch", 64)


def test_record_pairs_are_chosen_per_batch(gpu, orc, monkeypatch):
    """rec_pairs addresses a pair's tensors with 32-bit offsets: a batch that takes all frames of one of them past the limit
    (MARS_HIP_REC_LIMIT here, 4 GiB in production) plans WITHOUT the record format, a smaller batch afterwards WITH it again --
    same results either way (mars_hip_set_batch re-plans: alloc_batch)."""
    h, w, c = 20, 20, 64
    rng = np.random.default_rng(77)
    G = marsfile.Graph()
    F, N = marsfile.F32, marsfile.NCHW

    def conv_silu(xin, kk):
        a = G.tensor([1, c, h, w], dtype=F, fmt=N)
        wt = G.tensor([c, c, kk, kk], dtype=F, fmt=marsfile.OIHW, data=((rng.random((c, c, kk, kk), dtype=np.float32) * 2 - 1) * (1.7 / (kk * kk * c) ** 0.5)).astype(np.float32))
        b = G.tensor([c], dtype=F, fmt=marsfile.D1, data=((rng.random(c, dtype=np.float32) * 2 - 1) * 0.1).astype(np.float32))
        G.conv(xin, a, wt, b, (kk, kk), (1, 1), pad=marsfile.PAD_SAME)
        g_, o_ = G.tensor([1, c, h, w], dtype=F, fmt=N), G.tensor([1, c, h, w], dtype=F, fmt=N)
        G.layer(marsfile.SIGMOID, [a], [g_])
        G.layer(marsfile.MUL, [a, g_], [o_])
        return o_

    x = G.tensor([1, c, h, w], dtype=F, fmt=N)
    out = conv_silu(conv_silu(x, 1), 3)
    d = G.serialise([x], [out])
    xin = (rng.random(c * h * w, dtype=np.float32) * 2 - 1).astype(np.float32)
    g = orc.Graph(d)
    g.set_input(0, xin.tobytes())
    assert g.run() == 0
    want = g.tensor(out).copy()
    g.close()
    prec = gpu.lib().mhip_conv_f32_prec_launches
    prec.restype = C.c_ulong
    frame_bytes = c * h * w * 4  # 102400: every tensor of the pair
    monkeypatch.setenv("MARS_HIP_REC_LIMIT", str(frame_bytes * 10))
    try:
        gpu.set_tuning("f32_mfma", 3)
        gpu.set_tuning("dual_stream_min_batch", 0)
        m = gpu.Model(d, batch=4)
        for B, expect in ((4, 1), (16, 0), (9, 1), (11, 0), (2, 1)):
            m.set_batch(B)
            for f in range(B):
                m.input_view(0)[f] = xin.view(np.uint8)
            n0 = prec()
            m.run()
            assert prec() - n0 == expect, "batch %d: %d record-form launch(es)" % (B, prec() - n0)
            got = m.output_view(0)
            for f in (0, B - 1):
                assert close_f32(got[f], want).all(), "batch %d frame %d" % (B, f)
        m.close()
    finally:
        gpu.set_tuning("f32_mfma", 1)
        gpu.set_tuning("dual_stream_min_batch", 64)


@pytest.mark.parametrize("shape", [(40, 40, 128, 3, 96), (160, 160, 32, 3, 16), (20, 20, 256, 3, 160)], ids=lambda v: "x".join(str(q) for q in v))
def test_conv_f32_record_form_is_the_register_form_bit_for_bit(gpu, shape, monkeypatch):
    """a C3 bottleneck (1 x 1 -> 3 x 3 + shortcut Add) at a batch that gives every workgroup a run of tiles: the record form
    (conv_f32_prec, hand-counted DMA waits) multiplies exactly the pieces the register-staged form (conv_f32_patch) cuts itself, so
    the two must write the SAME BYTES -- and the same bytes again on every repetition (a chunk read before its DMA has landed would
    show as a difference between runs)."""
    h, w, c, k, B = shape
    rng = np.random.default_rng(h + c)
    G = marsfile.Graph()
    F, N = marsfile.F32, marsfile.NCHW

    def conv_silu(xin, kk):
        a = G.tensor([1, c, h, w], dtype=F, fmt=N)
        wt = G.tensor([c, c, kk, kk], dtype=F, fmt=marsfile.OIHW, data=((rng.random((c, c, kk, kk), dtype=np.float32) * 2 - 1) * (1.7 / (kk * kk * c) ** 0.5)).astype(np.float32))
        b = G.tensor([c], dtype=F, fmt=marsfile.D1, data=((rng.random(c, dtype=np.float32) * 2 - 1) * 0.1).astype(np.float32))
        G.conv(xin, a, wt, b, (kk, kk), (1, 1), pad=marsfile.PAD_SAME)
        g_, o_ = G.tensor([1, c, h, w], dtype=F, fmt=N), G.tensor([1, c, h, w], dtype=F, fmt=N)
        G.layer(marsfile.SIGMOID, [a], [g_])
        G.layer(marsfile.MUL, [a, g_], [o_])
        return o_

    x = G.tensor([1, c, h, w], dtype=F, fmt=N)
    t2 = conv_silu(conv_silu(x, 1), k)
    out = G.tensor([1, c, h, w], dtype=F, fmt=N)
    G.layer(marsfile.ADD, [t2, x], [out])
    d = G.serialise([x], [out])
    xs = (rng.random((B, c * h * w), dtype=np.float32) * 2 - 1).astype(np.float32)
    prec = gpu.lib().mhip_conv_f32_prec_launches
    prec.restype = C.c_ulong
    try:
        gpu.set_tuning("f32_mfma", 3)
        gpu.set_tuning("dual_stream_min_batch", 0)
        digests = []
        for norec in (True, False):
            if norec:
                monkeypatch.setenv("MARS_HIP_NO_REC", "1")
            else:
                monkeypatch.delenv("MARS_HIP_NO_REC", raising=False)
            m = gpu.Model(d, batch=B)
            m.input_view(0)[:] = xs.view(np.uint8)
            n0 = prec()
            for rep in range(1 if norec else 4):
                m.run()
                digests.append(zlib.crc32(m.output_view(0).tobytes()))
            assert prec() - n0 == (0 if norec else 4)
            m.close()
        assert len(set(digests)) == 1, digests
    finally:
        gpu.set_tuning("f32_mfma", 1)
        gpu.set_tuning("dual_stream_min_batch", 64)


@pytest.mark.parametrize("shape", [(20, 20, 64, 32, 3), (40, 40, 128, 64, 4), (24, 160, 64, 32, 2), (12, 40, 96, 80, 5), (80, 80, 128, 136, 6)],
                         ids=lambda v: "x".join(str(q) for q in v))
def test_conv_f32_pairs(gpu, orc, shape):
    """C3's cv1 + cv2 in the float twins: two 1 x 1 convolutions (+ SIGMOID / MUL) over the same tensor, same shape -- under f32_mfma = 3 / 4
    ONE launch (conv_f32_split's pair form, mars_plan.c pair_convs_f32).  Both outputs against the oracle on every frame; the counter
    proves the pair ran; at fusion level 0, in mode 2 and with MARS_HIP_NO_PAIR_F32 two launches and the same results."""
    h, w, ic, oc, B = shape
    rng = np.random.default_rng(h * 100 + ic + oc)
    G = marsfile.Graph()
    F, N = marsfile.F32, marsfile.NCHW
    x = G.tensor([1, ic, h, w], dtype=F, fmt=N)
    outs = []
    for _ in range(2):
        a = G.tensor([1, oc, h, w], dtype=F, fmt=N)
        wt = G.tensor([oc, ic, 1, 1], dtype=F, fmt=marsfile.OIHW, data=((rng.random((oc, ic, 1, 1), dtype=np.float32) * 2 - 1) * (1.7 / ic ** 0.5)).astype(np.float32))
        b = G.tensor([oc], dtype=F, fmt=marsfile.D1, data=((rng.random(oc, dtype=np.float32) * 2 - 1) * 0.1).astype(np.float32))
        G.conv(x, a, wt, b, (1, 1), (1, 1))
        g_, o_ = G.tensor([1, oc, h, w], dtype=F, fmt=N), G.tensor([1, oc, h, w], dtype=F, fmt=N)
        G.layer(marsfile.SIGMOID, [a], [g_])
        G.layer(marsfile.MUL, [a, g_], [o_])
        outs.append(o_)
    d = G.serialise([x], outs)
    nx = min(B, 3)
    xs = [(rng.random(ic * h * w, dtype=np.float32) * 2 - 1).astype(np.float32) for _ in range(nx)]
    want = []
    for q in xs:
        g = orc.Graph(d)
        g.set_input(0, q.tobytes())
        assert g.run() == 0
        want.append([g.tensor(o).copy() for o in outs])
        g.close()
    count = gpu.lib().mhip_conv_f32_pair_launches
    count.restype = C.c_ulong
    try:
        gpu.set_tuning("dual_stream_min_batch", 0)
        for mode, fusion, expect in ((3, 1, 1), (4, 1, 1), (3, 0, 0), (2, 1, 0)):
            gpu.set_tuning("f32_mfma", mode)
            m = gpu.Model(d, batch=B, fusion=fusion)
            for f in range(B):
                m.input_view(0)[f] = xs[f % nx].view(np.uint8)
            n0 = count()
            m.run()
            assert count() - n0 == expect, (mode, fusion, count() - n0)
            for k in range(2):
                got = m.output_view(k).copy()
                for f in range(B):
                    ok = close_f32(got[f], want[f % nx][k])
                    assert ok.all(), "mode %d fusion %d output %d frame %d: %d of %d out of tolerance" % (mode, fusion, k, f, int((~ok).sum()), ok.size)
            m.close()
    finally:
        gpu.set_tuning("f32_mfma", 1)
        gpu.set_tuning("dual_stream_min_batch", 64)


F32_STEM_SHAPES = f32shapes.STEM


@pytest.mark.parametrize("shape", F32_STEM_SHAPES, ids=lambda v: "x".join(str(q) for q in v))
def test_conv_f32_stem_shapes(gpu, orc, shape):
    """the float twins' first layer (few channels, even kernel, stride 2) through conv_f32_stem (mode 3: pair records in LDS, weights
    in registers, one barrier per tile; csrc/hip/conv_f32_stem.hip): every frame against the oracle within 1e-4 * max(1, |b|), with
    one workgroup per CU and with `persist_slots` = 3 (three workgroups walk all tiles: the two patch slots alternate through long
    runs); the launch counter proves which kernel ran."""
    h, w, ic, oc, k, B, silu = shape
    case = f32shapes.stem_case(shape)
    d, out, xs = case["d"], case["out"], case["xs"]
    nx = len(xs)
    ref = GOLD["conv_f32_family"][f32shapes.shape_id("stem", shape)]
    want = []
    for q in xs:
        g, rc = run_oracle(orc, d, q.view(np.uint8))
        assert rc == 0
        want.append(g.tensor(out).copy())
        g.close()
    count = gpu.lib().mhip_conv_f32_stem_launches
    count.restype = C.c_ulong
    takes = k * k // 2 <= 20 and ((k - 2) // 2) % 2 == 0  # (an even pad keeps the column pairs aligned)
    try:
        gpu.set_tuning("dual_stream_min_batch", 0)
        for mode, slots in ((3, 0), (3, 3), (4, 0), (0, 0)):
            gpu.set_tuning("f32_mfma", mode)
            gpu.set_tuning("persist_slots", slots)
            m = gpu.Model(d, batch=B)
            for f in range(B):
                m.input_view(0)[f] = xs[f % nx].view(np.uint8)
            n0 = count()
            m.run()
            assert count() - n0 == (1 if mode == 3 and takes else 0), "mode %d: conv_f32_stem launched %d time(s)" % (mode, count() - n0)
            got = m.output_view(0).copy()
            m.close()
            for f in range(B):
                if mode == 0:  # the reference's summation order: its bytes, by the restatement and by the reference-made digest
                    assert np.array_equal(got[f], want[f % nx]), "mode 0 frame %d" % f
                    assert cases.digest(got[f]) == ref[f % nx], "mode 0 frame %d: not the reference's bytes" % f
                    continue
                ok = close_f32(got[f], want[f % nx])
                assert ok.all(), "mode %d slots %d frame %d: %d of %d out of tolerance" % (mode, slots, f, int((~ok).sum()), ok.size)
    finally:
        gpu.set_tuning("f32_mfma", 1)
        gpu.set_tuning("persist_slots", 0)
        gpu.set_tuning("dual_stream_min_batch", 64)


def test_deferred_load_and_arena_copy(gpu):
    """what every rank but 0 does in the multi-GPU job: load DESCRIPTORS only (weights blob zeroed,
    MARS_HIP_LOAD_DEFER_WEIGHTS), receive rank 0's packed parameter arena byte for byte (here: a device-to-device
    copy instead of the RCCL broadcast), run -- outputs must equal the fully loaded model's"""
    import ctypes as C
    import sys
    sys.path.insert(0, os.path.join(HERE, "..", "thingino-accel_amd"))
    import dist as D
    d = gpu.synth_model(width_x16=4, input_hw=128, seed=31)
    hdr, tensors, _ = marsfile.parse(d)
    nb = marsfile.tensor_nbytes(tensors[hdr["inputs"][0]])
    B = 2
    full = gpu.Model(d, batch=B)
    lazy = gpu.Model(D.strip_weights(d), batch=B, flags=1)
    pa, na = full.param_arena()
    pb, nbytes = lazy.param_arena()
    assert na == nbytes and pa and pb and pa != pb  # identical layout on both "ranks"
    hip = C.CDLL("libamdhip64.so")
    hip.hipMemcpy.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int]
    assert hip.hipMemcpy(pb, pa, na, 3) == 0  # hipMemcpyDeviceToDevice
    for f in range(B):
        x = lcg_frame(0xD15C0000 + f, nb)
        full.input_view(0)[f] = x
        lazy.input_view(0)[f] = x
    full.run()
    lazy.run()
    for i in range(len(hdr["outputs"])):
        assert np.array_equal(full.output_view(i), lazy.output_view(i))
        assert full.output_view(i).any()
    full.close()
    lazy.close()


def test_nna_model_facade(gpu, orc, tmp_path):
    """the reference's model-handle API (include/nna_model.h) over a .mars graph, used the way
    examples/test_inference.c:142-238 uses it: load -> info -> get_input -> fill -> run -> get_output -> unload"""
    import ctypes as C
    L = gpu.lib()

    class Shape(C.Structure):
        _fields_ = [("dims", C.c_int32 * 4), ("ndim", C.c_int32)]

    class Tensor(C.Structure):
        _fields_ = [("data", C.c_void_p), ("shape", Shape), ("dtype", C.c_int), ("format", C.c_int), ("bytes", C.c_size_t),
                    ("owns_data", C.c_int)]

    class Info(C.Structure):
        _fields_ = [("num_inputs", C.c_uint32), ("num_outputs", C.c_uint32), ("num_layers", C.c_uint32),
                    ("model_size", C.c_size_t), ("forward_mem_req", C.c_size_t)]

    class Opts(C.Structure):
        _fields_ = [("use_file_mapping", C.c_int), ("enable_profiling", C.c_int), ("forward_memory", C.c_void_p),
                    ("forward_mem_size", C.c_size_t)]

    L.nna_model_load.restype = C.c_void_p
    L.nna_model_load.argtypes = [C.c_char_p, C.POINTER(Opts)]
    L.nna_model_load_from_memory.restype = C.c_void_p
    L.nna_model_load_from_memory.argtypes = [C.c_void_p, C.c_size_t, C.POINTER(Opts)]
    L.nna_model_get_info.argtypes = [C.c_void_p, C.POINTER(Info)]
    for n in ("nna_model_get_input", "nna_model_get_output"):
        getattr(L, n).restype = C.POINTER(Tensor)
        getattr(L, n).argtypes = [C.c_void_p, C.c_uint32]
    for n in ("nna_model_get_input_by_name", "nna_model_get_output_by_name"):
        getattr(L, n).restype = C.POINTER(Tensor)
        getattr(L, n).argtypes = [C.c_void_p, C.c_char_p]
    L.nna_model_run.argtypes = [C.c_void_p]
    L.nna_model_unload.argtypes = [C.c_void_p]

    d = gpu.synth_model(width_x16=4, input_hw=96, seed=51)
    hdr, tensors, _ = marsfile.parse(d)
    path = tmp_path / "twin.mars"
    path.write_bytes(d)
    opts = Opts(0, 1, None, 0)
    m = L.nna_model_load(str(path).encode(), C.byref(opts))
    assert m
    info = Info()
    assert L.nna_model_get_info(m, C.byref(info)) == 0
    assert (info.num_inputs, info.num_outputs, info.num_layers, info.model_size) == (1, 3, hdr["layers"], len(d))
    assert info.forward_mem_req > 0
    tin = L.nna_model_get_input(m, 0).contents
    nb = marsfile.tensor_nbytes(tensors[hdr["inputs"][0]])
    assert tin.bytes == nb and list(tin.shape.dims) == [1, 96, 96, 3] and tin.owns_data == 0
    x = lcg_frame(0xFACADE, nb)
    C.memmove(tin.data, x.ctypes.data, nb)
    assert not L.nna_model_get_input(m, 1) and not L.nna_model_get_output(m, 3)
    o = 76 + 124 * hdr["inputs"][0] + 4
    name_in = bytes(d[o:o + 60]).split(b"\0")[0]
    assert C.addressof(L.nna_model_get_input_by_name(m, name_in).contents) == C.addressof(L.nna_model_get_input(m, 0).contents)
    assert not L.nna_model_get_input_by_name(m, b"no such tensor")
    assert L.nna_model_run(m) == 0
    g, rc = run_oracle(orc, d, x)
    assert rc == 0
    for i, ti in enumerate(hdr["outputs"]):
        t = L.nna_model_get_output(m, i).contents
        got = np.ctypeslib.as_array(C.cast(t.data, C.POINTER(C.c_uint8)), shape=(t.bytes,))
        assert np.array_equal(got, g.tensor(ti))
    L.nna_model_unload(m)  # prints the per-launch profile (enable_profiling)
    buf = np.frombuffer(d, dtype=np.uint8).copy()
    m2 = L.nna_model_load_from_memory(buf.ctypes.data, buf.size, None)
    assert m2
    L.nna_model_unload(m2)
    assert not L.nna_model_load(b"/nonexistent.mgk", None)
    junk = tmp_path / "model.mgk"
    junk.write_bytes(b"\\x7fELF" + bytes(200))
    assert not L.nna_model_load(str(junk).encode(), None)  # Venus .mgk models are not served here


@pytest.mark.parametrize("h,w,c,k", [(20, 20, 64, 5), (7, 9, 32, 3), (13, 6, 16, 4), (24, 24, 48, 9)])
def test_pool_chain_fused(gpu, orc, h, w, c, k):
    """three chained stride-1 max-pools (SPPF) run as one LDS-resident launch in the fused plan: every stage tensor
    must equal the reference's (window anchored top-left, clipped right / bottom, odd and even windows)"""
    G = marsfile.Graph()
    x = G.tensor([1, h, w, c], scale=0.05)
    p1 = G.tensor([1, h, w, c], scale=0.05)
    p2 = G.tensor([1, h, w, c], scale=0.05)
    p3 = G.tensor([1, h, w, c], scale=0.05)
    o = G.tensor([1, h, w, c], scale=0.05)
    G.pool(x, p1, (k, k), (1, 1))
    G.pool(p1, p2, (k, k), (1, 1))
    G.pool(p2, p3, (k, k), (1, 1))
    G.layer(marsfile.RELU, [p3], [o])
    d = G.serialise([x], [o])
    B = 3
    xs = [lcg_frame(0x900C0000 + f + h * w, h * w * c) for f in range(B)]
    nops = {}
    for fusion in (0, 1):
        m = gpu.Model(d, batch=B, fusion=fusion)
        for f in range(B):
            m.input_view(0)[f] = xs[f]
        m.run()
        nops[fusion] = len(m.ops())
        for f in range(B):
            g, rc = run_oracle(orc, d, xs[f])
            assert rc == 0
            for t in (p1, p2, p3, o):
                assert np.array_equal(m.read_tensor(t, frame=f), g.tensor(t)), (fusion, f, t)
        m.close()
    assert nops[1] == nops[0] - 2


def test_virtual_concat_falls_back_for_huge_batches(gpu, orc, monkeypatch):
    """segmented (virtual concat) convolutions address their output with 32-bit offsets; a batch that would push an
    output past 2 GiB makes set_batch plan again with materialised concats.  The limit is lowered through
    MARS_HIP_VCONCAT_LIMIT so that a small batch takes that path; results must not change."""
    d = gpu.synth_model(width_x16=4, input_hw=96, seed=61)
    hdr, tensors, _ = marsfile.parse(d)
    nb = marsfile.tensor_nbytes(tensors[hdr["inputs"][0]])
    xs = [lcg_frame(0xB16B0000 + f, nb) for f in range(2)]
    m = gpu.Model(d, batch=2)
    n_virtual = len(m.ops())
    for f in range(2):
        m.input_view(0)[f] = xs[f]
    m.run()
    want = [m.output_view(i).copy() for i in range(3)]
    monkeypatch.setenv("MARS_HIP_VCONCAT_LIMIT", "4096")
    m.set_batch(2)  # re-plans: concat copies are back
    assert len(m.ops()) > n_virtual
    for f in range(2):
        m.input_view(0)[f] = xs[f]
    m.run()
    for i in range(3):
        assert np.array_equal(m.output_view(i), want[i])
    g, rc = run_oracle(orc, d, xs[1])
    assert rc == 0
    for i, ti in enumerate(hdr["outputs"]):
        assert np.array_equal(g.tensor(ti), want[i][1])
    m.close()


def test_c_program_links_and_runs(gpu, orc, tmp_path):
    """tests/c/drop_in.c: a plain C caller (reference headers only) compiled with gcc, linked against the in-tree
    libnna_mars.so, run as its own process on the GPU; its output checksum equals the oracle's for the same model"""
    import subprocess
    root = os.path.join(HERE, "..")
    libdir = os.path.join(root, "thingino-accel_amd", "lib")
    exe = tmp_path / "drop_in"
    subprocess.run(["gcc", "-O1", "-Wall", "-I" + os.path.join(root, "include"), os.path.join(HERE, "c", "drop_in.c"), "-o", str(exe),
                    "-L" + libdir, "-lnna_mars", "-Wl,-rpath," + libdir], check=True)
    model = os.path.join(HERE, "golden", "models", "tiny_160_int8.mars")
    out = subprocess.run([str(exe), model], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, (out.returncode, out.stderr[-1000:])
    d = open(model, "rb").read()
    hdr, tensors, _ = marsfile.parse(d)
    n = marsfile.tensor_nbytes(tensors[hdr["inputs"][0]])
    x = (np.arange(n) % 127).astype(np.int8).view(np.uint8)
    g, rc = run_oracle(orc, d, x)
    assert rc == 0
    want = g.tensor(hdr["outputs"][0])
    h = 0xCBF29CE484222325
    for b in want.tobytes():
        h = ((h ^ b) * 0x100000001B3) & 0xFFFFFFFFFFFFFFFF
    lines = out.stdout.split()
    assert lines[0] == "mars" and int(lines[1]) == want.size and lines[2] == "%016x" % h
    assert lines[3] == "nna" and int(lines[4]) == want.size and lines[5] == "%016x" % h


def test_pipe_results_survive_the_next_submit(gpu, orc):
    """include/mars_hip.h: what mars_hip_pipe_wait() hands out stays valid until the SECOND submit after the call (four buffer
    sets, three batches in flight).  The steady-state loop -- wait k, submit k+3, only then read the results of k through
    the views (copy=False) -- must see batch k's bytes, not those of a later batch (with three buffer sets the submit right
    after the wait queued its copies into exactly these buffers)."""
    d = gpu.synth_model(width_x16=4, input_hw=96, seed=33)
    hdr, tensors, _ = marsfile.parse(d)
    nb = marsfile.tensor_nbytes(tensors[hdr["inputs"][0]])
    B, NB = 2, 9
    xs = [[lcg_frame(0xB10000 + 16 * k + f, nb) for f in range(B)] for k in range(NB)]
    m = gpu.Model(d, batch=B)
    want = []
    for k in range(NB):
        for f in range(B):
            m.input_view(0)[f] = xs[k][f]
        m.run()
        dets = m.detect(outputs=(0, 1, 2), thresh=0.45)
        want.append(([m.output_view(i).copy() for i in range(3)], dets))
    m.pipe_open(download_outputs=True, detect=True, det_outputs=(0, 1, 2), thresh=0.45)

    def submit(k):
        iv = m.pipe_input_view(0)
        for f in range(B):
            iv[f] = xs[k][f]
        m.pipe_submit()

    for k in range(3):
        submit(k)
    for k in range(NB):
        outs, (dv, cv) = m.pipe_wait(copy=False)   # views into the pipe's pinned result buffers
        if k + 3 < NB:
            submit(k + 3)                          # the next batch is queued (and may complete) before the results are read
            gpu.lib().mars_hip_sync()              # worst case: everything queued so far has finished
        for i in range(3):
            assert np.array_equal(outs[i], want[k][0][i]), (k, i)
        for f in range(B):
            assert dv[f, :cv[f]].tobytes() == want[k][1][f].tobytes(), (k, f)
    m.pipe_close()
    m.close()


def test_pipelined_io_matches_mars_run(gpu, orc):
    """mars_hip_pipe_*: five batches through the double-buffered path (upload k+1 / graph k / tail k / download k-1 on
    their own streams and buffers) == the same batches through mars_run() + mars_hip_detect(), bit for bit: raw outputs
    (the padded 255-channel heads included) and detections; then the model works synchronously again; a fourth submit
    without a wait is refused"""
    d = gpu.synth_model(width_x16=4, input_hw=96, seed=31)
    hdr, tensors, _ = marsfile.parse(d)
    nb = marsfile.tensor_nbytes(tensors[hdr["inputs"][0]])
    B, NB = 3, 5
    xs = [[lcg_frame(0xB00000 + 16 * k + f, nb) for f in range(B)] for k in range(NB)]
    m = gpu.Model(d, batch=B)
    want = []
    for k in range(NB):
        for f in range(B):
            m.input_view(0)[f] = xs[k][f]
        m.run()
        dets = m.detect(outputs=(0, 1, 2), thresh=0.45)
        want.append(([m.output_view(i).copy() for i in range(3)], dets))
    for mode in ((True, True), (False, True), (True, False)):
        m.pipe_open(download_outputs=mode[0], detect=mode[1], det_outputs=(0, 1, 2), thresh=0.45)
        got = []
        for k in range(NB):
            iv = m.pipe_input_view(0)
            for f in range(B):
                iv[f] = xs[k][f]
            m.pipe_submit()
            if k >= 1:
                got.append(m.pipe_wait())
        got.append(m.pipe_wait())
        if mode == (True, True):  # three in flight is the limit
            for _ in range(3):
                m.pipe_input_view(0)[:] = 0
                m.pipe_submit()
            with pytest.raises(gpu.MarsError):
                m.pipe_submit()
            for _ in range(3):
                m.pipe_wait()
        for k in range(NB):
            outs, dets = got[k]
            if mode[0]:
                for i in range(3):
                    assert np.array_equal(outs[i], want[k][0][i]), (mode, k, i)
            if mode[1]:
                for f in range(B):
                    assert dets[f].tobytes() == want[k][1][f].tobytes(), (mode, k, f)
        m.pipe_close()
    for f in range(B):  # back to the synchronous path on the model's own buffers
        m.input_view(0)[f] = xs[2][f]
    m.run()
    for i in range(3):
        assert np.array_equal(m.output_view(i), want[2][0][i])
    m.close()


def test_multi_gpu_recipe_from_c(gpu, orc, tmp_path):
    """tests/c/multi_gpu.c: one process per GPU from plain C -- fork before any GPU call,
    ncclUniqueId over a pipe, rank 0 loads the file, the others descriptors only, ONE ncclBroadcast of the parameter
    arena, frames sharded by rank.  Run with one rank here (an RCCL group of one: what a one-GPU box can host); every
    frame's checksum must equal the oracle's for that frame."""
    import subprocess
    root = os.path.join(HERE, "..")
    libdir = os.path.join(root, "thingino-accel_amd", "lib")
    exe = tmp_path / "multi_gpu"
    subprocess.run(["gcc", "-O1", "-Wall", "-D__HIP_PLATFORM_AMD__", "-I" + os.path.join(root, "include"), "-I/opt/rocm/include",
                    os.path.join(HERE, "c", "multi_gpu.c"), "-o", str(exe), "-L" + libdir, "-lnna_mars", "-L/opt/rocm/lib", "-lrccl",
                    "-lamdhip64", "-Wl,-rpath," + libdir, "-Wl,-rpath,/opt/rocm/lib"], check=True)
    d = gpu.synth_model(width_x16=4, input_hw=64, seed=41)
    path = tmp_path / "twin.mars"
    path.write_bytes(d)
    out = subprocess.run([str(exe), str(path), "1", "3"], capture_output=True, text=True, timeout=600)
    assert out.returncode == 0, (out.returncode, out.stdout[-500:], out.stderr[-1500:])
    hdr, tensors, _ = marsfile.parse(d)
    nb = marsfile.tensor_nbytes(tensors[hdr["inputs"][0]])
    lines = [l.split() for l in out.stdout.splitlines() if l.startswith("frame")]
    assert [int(l[1]) for l in lines] == [0, 1, 2]
    for l in lines:
        g, rc = run_oracle(orc, d, lcg_frame(0x5EED0000 + int(l[1]), nb))
        assert rc == 0
        h = 0xCBF29CE484222325
        for b in g.tensor(hdr["outputs"][0]).tobytes():
            h = ((h ^ b) * 0x100000001B3) & 0xFFFFFFFFFFFFFFFF
        assert l[4] == "%016x" % h, l
        g.close()


@pytest.mark.parametrize("B", [2, 5])
def test_two_half_batches_on_two_streams(gpu, orc, B):
    """"dual_stream_min_batch": a batch enqueued as two halves on two streams (frames [0, ceil(B/2)) and the rest; the
    default from 64 frames up, forced here at 2 and at an odd 5) writes the bytes of the one-stream run -- graph outputs,
    the detection tail that follows on the auxiliary stream without a host sync, and the pipelined I/O path -- and
    frame 0 still equals the oracle"""
    d = gpu.synth_model(width_x16=4, input_hw=96, seed=77, vary_scales=True)
    hdr, tensors, _ = marsfile.parse(d)
    nb = marsfile.tensor_nbytes(tensors[hdr["inputs"][0]])
    xs = [lcg_frame(0xD0A1 * 16 + f, nb) for f in range(B)]
    res = {}
    try:
        for dual in (0, 2):
            gpu.set_tuning("graph_max_batch", 0)
            gpu.set_tuning("dual_stream_min_batch", dual)
            m = gpu.Model(d, batch=B)
            for f in range(B):
                m.input_view(0)[f] = xs[f]
            m.run()
            outs = [m.output_view(i).copy() for i in range(3)]
            for _ in range(3):  # graph k+1 behind tail k, by events only
                m.run_device(sync=False)
                m.detect_device(outputs=(0, 1, 2), thresh=0.45)
            assert gpu.lib().mars_hip_sync() == 0
            dets = m.detect(outputs=(0, 1, 2), thresh=0.45)
            m.pipe_open(download_outputs=True, detect=True, det_outputs=(0, 1, 2), thresh=0.45)
            piped = []
            for k in range(3):
                iv = m.pipe_input_view(0)
                for f in range(B):
                    iv[f] = xs[(f + k) % B]
                m.pipe_submit()
            for k in range(3):
                po, pd = m.pipe_wait()
                piped.append(([o.copy() for o in po], [x.tobytes() for x in pd]))
            m.pipe_close()
            m.close()
            res[dual] = (outs, [x.tobytes() for x in dets], piped)
    finally:
        gpu.set_tuning("dual_stream_min_batch", 64)
        gpu.set_tuning("graph_max_batch", 8)
    a, b = res[0], res[2]
    for i in range(3):
        assert np.array_equal(a[0][i], b[0][i]), i
    assert a[1] == b[1]
    for k in range(3):
        for i in range(3):
            assert np.array_equal(a[2][k][0][i], b[2][k][0][i]), (k, i)
        assert a[2][k][1] == b[2][k][1]
    g, rc = run_oracle(orc, d, xs[0])
    assert rc == 0
    for oi, ti in enumerate(hdr["outputs"]):
        assert np.array_equal(b[0][oi][0], g.tensor(ti))


@pytest.mark.parametrize("direct", [1, 0])
def test_rgb_stem_both_forms(gpu, orc, direct):
    """the RGB stem with its fused SiLU table, three frames per run (frame boundaries; the first and the last bytes of
    the tensor, which the operand-direct form gathers byte by byte): images that are all edge tiles, ragged tile
    overhangs on every side, interior tiles, strides 1 and 2, kernels 3 / 5 / 6 -- in the operand-direct form
    (conv_i8_rgb, the default) and in the patch-staged form it replaced, against the oracle"""
    shapes = [  # h, w, out_c, k, s (or (stride_h, stride_w))
        (37, 53, 32, 6, 2), (70, 41, 16, 3, 1), (9, 5, 32, 3, 1), (33, 6, 48, 6, 2), (130, 131, 32, 6, 2), (96, 160, 64, 6, 2),
        (64, 64, 32, 5, 2), (16, 16, 32, 6, 2), (4, 128, 32, 7, (2, 4)), (61, 203, 16, 9, (2, 4)), (50, 50, 32, 4, (4, 2))]
    rng = np.random.default_rng(5)
    try:
        gpu.set_tuning("rgb_direct", direct)
        for (h, w, oc, k, s) in shapes:
            sh, sw = s if isinstance(s, tuple) else (s, s)
            oh, ow = (h + sh - 1) // sh, (w + sw - 1) // sw
            G = marsfile.Graph()
            x = G.tensor([1, h, w, 3], scale=0.02)
            a = G.tensor([1, oh, ow, oc], scale=0.05)
            sg = G.tensor([1, oh, ow, oc], scale=1.0 / 256)
            o = G.tensor([1, oh, ow, oc], scale=0.04)
            wt = G.tensor([oc, k, k, 3], scale=0.004, data=rng.integers(-127, 128, (oc, k, k, 3), dtype=np.int8))
            b = G.tensor([oc], dtype=marsfile.I32, scale=1.0, data=rng.integers(-2000, 2000, oc, dtype=np.int32))
            G.conv(x, a, wt, b, (k, k), (sh, sw))
            G.layer(marsfile.SIGMOID, [a], [sg])
            G.layer(marsfile.MUL, [a, sg], [o])
            d = G.serialise([x], [o])
            hdr, tensors, _ = marsfile.parse(d)
            B = 3
            m = gpu.Model(d, batch=B)
            xs = [lcg_frame(0x57E3 * 64 + 8 * h + f, h * w * 3) for f in range(B)]
            for f in range(B):
                m.input_view(0)[f] = xs[f]
            m.run()
            for f in range(B):
                g, rc = run_oracle(orc, d, xs[f])
                assert rc == 0
                want = g.tensor(hdr["outputs"][0])
                got = m.output_view(0)[f]
                bad = np.flatnonzero(got != want)
                assert bad.size == 0, ((h, w, oc, k, s), f, bad.size, [(int(i) // oc // ow, int(i) // oc % ow, int(i) % oc) for i in bad[:12]])
                assert len(np.unique(want)) > 16
            m.close()
    finally:
        gpu.set_tuning("rgb_direct", 1)


@pytest.mark.parametrize("width,hw,B", [(8, 256, 2), (4, 256, 1), (8, 128, 3)])
def test_fused_bottleneck_level2(gpu, orc, width, hw, B):
    """fusion level 2: the C3 bottleneck's 1x1 + SiLU evaluated on the staged patch of the following 3x3 (halo pixels
    included, zeros outside the image as the 3x3's SAME padding wants; the 1x1's output tensor is never written):
    fewer launches, the same bytes -- twins with per-convolution scales, 32- and 64-channel bottlenecks, maps that
    are not multiples of the tile, against the oracle and against level 1"""
    d = gpu.synth_model(width_x16=width, input_hw=hw, seed=41 + hw, vary_scales=True)
    hdr, tensors, _ = marsfile.parse(d)
    nb = marsfile.tensor_nbytes(tensors[hdr["inputs"][0]])
    xs = [lcg_frame(0xB0771E * 16 + f, nb) for f in range(B)]
    outs, nops = {}, {}
    for level in (1, 2):
        m = gpu.Model(d, batch=B, fusion=level)
        for f in range(B):
            m.input_view(0)[f] = xs[f]
        m.run()
        outs[level] = [m.output_view(i).copy() for i in range(3)]
        nops[level] = len(m.ops())
        m.close()
    assert nops[2] < nops[1]
    for i in range(3):
        assert np.array_equal(outs[1][i], outs[2][i]), i
    g, rc = run_oracle(orc, d, xs[B - 1])
    assert rc == 0
    for oi, ti in enumerate(hdr["outputs"]):
        assert np.array_equal(outs[2][oi][B - 1], g.tensor(ti))


def test_fused_bottleneck_refused_at_a_batch_falls_back(gpu, orc, monkeypatch):
    """a fused bottleneck is accepted at load time on geometry alone; whether the fused launch fits 32-bit offsets depends on
    the batch.  alloc_batch re-checks every fused launch at the real batch and plans again without the fusion when one
    does not fit (the 1x1 has left the plan: there would be no fallback at launch time).  MARS_HIP_BOTTLENECK_LIMIT makes
    a small batch count as too large."""
    d = gpu.synth_model(width_x16=8, input_hw=128, seed=77, vary_scales=True)
    hdr, tensors, _ = marsfile.parse(d)
    nb = marsfile.tensor_nbytes(tensors[hdr["inputs"][0]])
    xs = [lcg_frame(0xB0771F * 16 + f, nb) for f in range(3)]
    m = gpu.Model(d, batch=1, fusion=2)
    fused_ops = len(m.ops())
    monkeypatch.setenv("MARS_HIP_BOTTLENECK_LIMIT", "2")
    m.set_batch(3)  # "too large": the plan is rebuilt with the 1x1 launches back in
    assert len(m.ops()) > fused_ops
    for f in range(3):
        m.input_view(0)[f] = xs[f]
    m.run()
    for f in (0, 2):
        g, rc = run_oracle(orc, d, xs[f])
        assert rc == 0
        for oi, ti in enumerate(hdr["outputs"]):
            assert np.array_equal(m.output_view(oi)[f], g.tensor(ti)), (f, oi)
    m.close()


def test_concat_of_96_channels_is_materialised(gpu, orc):
    """a 1x1 convolution over a concat whose channel total is not a power of two (64 + 32): the never-materialised
    concat form (tile walker, K position by shifts) does not take it, so the plan must keep the copy -- found by
    tests/soak/fuzz_graphs.py, which had the fused plans fail to launch"""
    rng = np.random.default_rng(96)
    hw = 20
    G = marsfile.Graph()
    x = G.tensor([1, hw, hw, 32], scale=0.03)
    a = _silu_conv(G, rng, x, 32, 64, hw, 1, 0.05, 1.0 / 256, 0.04)
    cat = G.tensor([1, hw, hw, 96], scale=0.04)
    G.concat([a, x], cat)
    o = _silu_conv(G, rng, cat, 96, 64, hw, 1, 0.06, 1.0 / 256, 0.05)
    d = G.serialise([x], [o])
    hdr, tensors, _ = marsfile.parse(d)
    B = 2
    xs = [lcg_frame(0x960000 + f, hw * hw * 32) for f in range(B)]
    for level in (0, 1, 2):
        m = gpu.Model(d, batch=B, fusion=level)
        for f in range(B):
            m.input_view(0)[f] = xs[f]
        m.run()
        for f in range(B):
            g, rc = run_oracle(orc, d, xs[f])
            assert rc == 0
            assert np.array_equal(m.output_view(0)[f], g.tensor(hdr["outputs"][0])), (level, f)
        m.close()


def test_per_model_tuning_overrides(gpu, orc):
    """mars_hip_model_set_tuning: a knob kept on one model, in force during ITS runs only.  Observable on a float32 twin:
    f32_mfma = 0 (the reference's summation order) is bit-exact against the oracle, f32_mfma = 2 (matrix cores everywhere) is
    not (another summation order, then byte-wise max-pools over the float bits); the process default stays 1 throughout."""
    d = gpu.synth_model(width_x16=4, input_hw=64, seed=5, float32=True)
    hdr, tensors, _ = marsfile.parse(d)
    n = marsfile.tensor_nbytes(tensors[hdr["inputs"][0]]) // 4
    x = cases.f32(0x7E570001, n, 0.0, 1.0).view(np.uint8)
    a, b = gpu.Model(d, batch=1), gpu.Model(d, batch=1)
    assert gpu.get_tuning("f32_mfma") == 1
    a.set_tuning("f32_mfma", 0)
    b.set_tuning("f32_mfma", 2)
    b.set_tuning("graph_max_batch", 0)
    assert (a.get_tuning("f32_mfma"), b.get_tuning("f32_mfma"), gpu.get_tuning("f32_mfma")) == (0, 2, 1)
    assert a.get_tuning("graph_max_batch") == gpu.get_tuning("graph_max_batch") and b.get_tuning("graph_max_batch") == 0
    with pytest.raises(KeyError):
        a.set_tuning("no_such_knob", 1)
    with pytest.raises(KeyError):
        a.set_tuning("dual_stream_ways", 9)  # a value the knob refuses
    assert a.get_tuning("dual_stream_ways") == gpu.get_tuning("dual_stream_ways")
    g, rc = run_oracle(orc, d, x)
    assert rc == 0
    for rounds in range(3):  # interleaved runs (the third ones replay a's captured graph): each under its own policy
        for m in (a, b):
            m.input_view(0)[0] = x
            m.run()
            assert gpu.get_tuning("f32_mfma") == 1
    diff = 0
    for i, ti in enumerate(hdr["outputs"]):
        want = g.tensor(ti)
        assert np.array_equal(a.output_view(i)[0].view(np.uint8).ravel(), want.view(np.uint8).ravel())
        diff += int((b.output_view(i)[0].view(np.uint8).ravel() != want.view(np.uint8).ravel()).sum())
    assert diff > 0  # the matrix-core order did run for b
    g.close()
    a.close()
    b.close()


def test_mars_run_in_overlapped_chunks(gpu, orc):
    """"run_chunk": mars_run at a large batch copies chunk k+1 in while chunk k runs and chunk k-1 is copied out (three
    streams, one synchronisation at the end); forced here at 2 frames per chunk on a batch of 5 (chunks of 2, 2, 1) and
    of 9 (8 chunks at most): every frame equals the one-piece run and the oracle, the detection tail that was left
    pending before the call is respected, and the model keeps working afterwards"""
    d = gpu.synth_model(width_x16=4, input_hw=96, seed=61, vary_scales=True)
    hdr, tensors, _ = marsfile.parse(d)
    nb = marsfile.tensor_nbytes(tensors[hdr["inputs"][0]])
    try:
        for B in (5, 9):
            xs = [lcg_frame(0xC4C4 * 16 + f, nb) for f in range(B)]
            res = {}
            for chunk in (0, 2):
                gpu.set_tuning("run_chunk", chunk)
                m = gpu.Model(d, batch=B)
                for f in range(B):
                    m.input_view(0)[f] = xs[f]
                m.run()
                m.detect_device(outputs=(0, 1, 2), thresh=0.45)  # tail pending on the auxiliary stream
                for i in range(3):
                    m.output_view(i)[:] = 0
                m.run()
                res[chunk] = [m.output_view(i).copy() for i in range(3)]
                m.close()
            for i in range(3):
                assert np.array_equal(res[0][i], res[2][i]), (B, i)
            for f in (0, B - 1):
                g, rc = run_oracle(orc, d, xs[f])
                assert rc == 0
                for oi, ti in enumerate(hdr["outputs"]):
                    assert np.array_equal(res[2][oi][f], g.tensor(ti)), (B, f, oi)
        # output mode "on device": mars_run copies nothing back (vaddr keeps what it held); the detections and explicit
        # downloads still see the new results -- in one piece and in chunks
        B = 5
        xs = [lcg_frame(0xC4C5 * 16 + f, nb) for f in range(B)]
        for chunk in (0, 2):
            gpu.set_tuning("run_chunk", chunk)
            m = gpu.Model(d, batch=B)
            for f in range(B):
                m.input_view(0)[f] = xs[f]
            m.run()
            want = [m.output_view(i).copy() for i in range(3)]
            want_d = m.detect(outputs=(0, 1, 2), thresh=0.45)
            assert gpu.lib().mars_hip_set_output_mode(m.p, 1) == 0
            assert gpu.lib().mars_hip_set_output_mode(m.p, 7) != 0
            for i in range(3):
                m.output_view(i)[:] = 0x5A
            for f in range(B):
                m.input_view(0)[f] = xs[B - 1 - f]          # other frames than before
            m.run()
            for i in range(3):
                assert (m.output_view(i) == 0x5A).all(), (chunk, i)   # nothing was copied back
            got_d = m.detect(outputs=(0, 1, 2), thresh=0.45)
            for f in range(B):
                assert got_d[f].tobytes() == want_d[B - 1 - f].tobytes(), (chunk, f)
            m.download()
            for i in range(3):
                assert np.array_equal(m.output_view(i), want[i][::-1]), (chunk, i)
            assert gpu.lib().mars_hip_set_output_mode(m.p, 0) == 0
            m.run()
            for i in range(3):
                assert np.array_equal(m.output_view(i), want[i][::-1]), (chunk, i)
            m.close()
    finally:
        gpu.set_tuning("run_chunk", 128)


def _f32_conv_silu(G, rng, xin, ic, ih, iw, oc, k, st, bias=True):
    """conv (SAME) + SIGMOID + MUL on NCHW floats; -> (output tensor, out_h, out_w)"""
    F, N = marsfile.F32, marsfile.NCHW
    oh, ow = (ih + st - 1) // st, (iw + st - 1) // st
    a = G.tensor([1, oc, oh, ow], dtype=F, fmt=N)
    amp = 1.7 / (k * k * ic) ** 0.5
    wt = G.tensor([oc, ic, k, k], dtype=F, fmt=marsfile.OIHW, data=((rng.random((oc, ic, k, k), dtype=np.float32) * 2 - 1) * amp).astype(np.float32))
    if bias:
        b = G.tensor([oc], dtype=F, fmt=marsfile.D1, data=((rng.random(oc, dtype=np.float32) * 2 - 1) * 0.1).astype(np.float32))
        G.conv(xin, a, wt, b, (k, k), (st, st), pad=marsfile.PAD_SAME)
    else:
        G.conv(xin, a, wt, k=(k, k), s=(st, st), pad=marsfile.PAD_SAME)
    g_, o_ = G.tensor([1, oc, oh, ow], dtype=F, fmt=N), G.tensor([1, oc, oh, ow], dtype=F, fmt=N)
    G.layer(marsfile.SIGMOID, [a], [g_])
    G.layer(marsfile.MUL, [a, g_], [o_])
    return o_, oh, ow


@pytest.mark.parametrize("biases", [(True, False), (False, True), (False, False)], ids=["a_only", "b_only", "none"])
@pytest.mark.parametrize("oc", [32, 64, 96])
def test_conv_f32_pairs_without_bias(gpu, orc, biases, oc):
    """a convolution's bias is optional, and the one-tile pair form (2 x out_c <= 128: oc 32 / 64) selects the bias row per
    channel -- a missing second bias minus BM / 2 was a non-null pointer into page 0.  Every combination, both pair forms, against the oracle."""
    h, w, ic, B = 20, 24, 64, 3
    rng = np.random.default_rng(oc * 7 + biases[0] * 2 + biases[1])
    G = marsfile.Graph()
    x = G.tensor([1, ic, h, w], dtype=marsfile.F32, fmt=marsfile.NCHW)
    outs = [_f32_conv_silu(G, rng, x, ic, h, w, oc, 1, 1, bias=bz)[0] for bz in biases]
    d = G.serialise([x], outs)
    xs = [(rng.random(ic * h * w, dtype=np.float32) * 2 - 1).astype(np.float32) for _ in range(B)]
    count = gpu.lib().mhip_conv_f32_pair_launches
    count.restype = C.c_ulong
    try:
        gpu.set_tuning("dual_stream_min_batch", 0)
        for mode in (3, 4):
            gpu.set_tuning("f32_mfma", mode)
            m = gpu.Model(d, batch=B)
            for f in range(B):
                m.input_view(0)[f] = xs[f].view(np.uint8)
            n0 = count()
            m.run()
            assert count() - n0 == 1, mode
            for f in range(B):
                g, rc = run_oracle(orc, d, xs[f].view(np.uint8))
                assert rc == 0
                for k in range(2):
                    ok = close_f32(m.output_view(k)[f], g.tensor(outs[k]))
                    assert ok.all(), "mode %d output %d frame %d: %d of %d out of tolerance" % (mode, k, f, int((~ok).sum()), ok.size)
                g.close()
            m.close()
    finally:
        gpu.set_tuning("f32_mfma", 1)
        gpu.set_tuning("dual_stream_min_batch", 64)


@pytest.mark.parametrize("prod", [(16, 5, 2), (8, 7, 2), (24, 3, 1)], ids=lambda v: "x".join(str(q) for q in v))
def test_record_pairs_only_behind_a_producer_that_writes_records(gpu, orc, prod):
    """rec_pairs marked a producer `out_rec` whenever it had a bf16 weight image -- but conv_f32_split declines stride-2 layers
    with an odd kernel width and pad > 1 (5 x 5 pad 2, 7 x 7 pad 3), and nothing else writes records: the run failed with LAYER_FAILED.
    The planner now asks mhip_conv_f32_split_takes first.  (24, 3, 1) is the control: a producer that does write records.)"""
    ic, k, st = prod
    h, w, B = (47, 63, 3) if st == 2 else (48, 64, 3)  # odd sizes: SAME padding of a stride-2 5 x 5 / 7 x 7 is then 2 / 3 on the left
    rng = np.random.default_rng(ic * 100 + k)
    G = marsfile.Graph()
    x = G.tensor([1, ic, h, w], dtype=marsfile.F32, fmt=marsfile.NCHW)
    t1, h1, w1 = _f32_conv_silu(G, rng, x, ic, h, w, 32, k, st)
    t2, h2, w2 = _f32_conv_silu(G, rng, t1, 32, h1, w1, 32, 3, 1)
    d = G.serialise([x], [t2])
    xs = [(rng.random(ic * h * w, dtype=np.float32) * 2 - 1).astype(np.float32) for _ in range(B)]
    L = gpu.lib()
    takes = L.mhip_conv_f32_split_takes
    takes.restype = C.c_int
    takes.argtypes = [C.c_int] * 9
    pad = (k - 1) // 2 if st == 1 else max(0, ((h1 - 1) * st + k - h)) // 2
    writes_records = takes(32, ic, k, k, st, st, pad, w, w1) >= 0
    assert writes_records == (st == 1)
    prec = L.mhip_conv_f32_prec_launches
    prec.restype = C.c_ulong
    recin = L.mhip_conv_f32_recin_launches
    recin.restype = C.c_ulong
    try:
        gpu.set_tuning("f32_mfma", 3)
        gpu.set_tuning("dual_stream_min_batch", 0)
        m = gpu.Model(d, batch=B)
        for f in range(B):
            m.input_view(0)[f] = xs[f].view(np.uint8)
        n0 = prec() + recin()
        m.run()  # (MARS_ERR_LAYER_FAILED before the fix)
        assert (prec() + recin() - n0 == 1) == writes_records
        for f in range(B):
            g, rc = run_oracle(orc, d, xs[f].view(np.uint8))
            assert rc == 0
            ok = close_f32(m.output_view(0)[f], g.tensor(t2))
            assert ok.all(), "frame %d: %d of %d out of tolerance" % (f, int((~ok).sum()), ok.size)
            g.close()
        m.close()
    finally:
        gpu.set_tuning("f32_mfma", 1)
        gpu.set_tuning("dual_stream_min_batch", 64)


@pytest.mark.parametrize("how", ["process", "model"])
def test_f32_mode_change_after_load_replans(gpu, orc, how):
    """a float model's plan belongs to the f32_mfma mode it was built under (two bf16 planes under 3, three under 4, record
    tensors under 3 only).  Loaded under 3 and switched to 4, conv_f32_split read a third plane that was never packed (the next op's
    arena bytes); switched to 0, the record pairs silently stayed on the split-bf16 cores.  A change -- process-wide or per model -- now
    plans the model again (as mars_hip_set_fusion does; inputs are filled afterwards): mode 4 inside the tolerance, mode 0 BIT-EXACT
    (the reference's summation order), back to 3 with the record pairs again."""
    d = gpu.synth_model(width_x16=4, input_hw=128, seed=9, float32=True)  # (the well-conditioned small float twin: cases.SYNTH v5n_128_f32)
    hdr, tensors, _ = marsfile.parse(d)
    n = marsfile.tensor_nbytes(tensors[hdr["inputs"][0]]) // 4
    B = 2
    xs = [cases.f32(0x5EED0000 + f, n, 0.0, 1.0).view(np.uint8) for f in range(B)]
    want = []
    for f in range(B):
        g, rc = run_oracle(orc, d, xs[f])
        assert rc == 0
        want.append([g.tensor(ti).copy() for ti in hdr["outputs"]])
        g.close()
    L = gpu.lib()
    for nm in ("prec", "recin", "split"):
        getattr(L, "mhip_conv_f32_%s_launches" % nm).restype = C.c_ulong
    prec = lambda: L.mhip_conv_f32_prec_launches() + L.mhip_conv_f32_recin_launches()  # noqa: E731  (either record reader)
    split = L.mhip_conv_f32_split_launches
    try:
        gpu.set_tuning("f32_mfma", 3)
        m = gpu.Model(d, batch=B)
        for mode in (3, 4, 0, 3):
            if how == "process":
                gpu.set_tuning("f32_mfma", mode)
            else:
                m.set_tuning("f32_mfma", mode)
            for f in range(B):
                m.input_view(0)[f] = xs[f]
            p0, s0 = prec(), split()
            m.run()
            assert (prec() - p0 > 0) == (mode == 3), mode       # record pairs exist under mode 3 only
            assert (split() - s0 > 0) == (mode in (3, 4)), mode  # ... and the split-bf16 kernels under 3 / 4 only
            for f in range(B):
                for i in range(len(hdr["outputs"])):
                    got = m.output_view(i)[f]
                    if mode == 0:
                        assert np.array_equal(got, want[f][i]), "mode 0 frame %d head %d is not bit-exact" % (f, i)
                    else:
                        ok = close_f32(got, want[f][i])
                        assert ok.all(), "mode %d frame %d head %d: %d of %d out of tolerance" % (mode, f, i, int((~ok).sum()), ok.size)
        m.close()
    finally:
        gpu.set_tuning("f32_mfma", 1)


@pytest.mark.parametrize("name", ["yolov5n_int8", "yolov5nu", "tiny_160_int8"])
@pytest.mark.parametrize("fusion", [1, 0])
def test_shipped_files_at_batch_8_every_tensor(gpu, orc, name, fusion):
    """the reference's own NCHW-tagged files (BASELINE config 3's literal yolov5n_int8.mars; the 320 x 320 yolov5nu;
    config 2's tiny_160) beyond batch 1 and the pattern input: 8 LCG frames, every activation tensor the plan keeps in HBM
    against the oracle for frames 0 and 7 -- at the default fusion level, where convolution-only tensors are held pixels x channels on
    the device (mars_plan.c nhwc_internal; mars_hip_read_tensor converts), and at level 0, where every tensor is the reference's bytes --
    plus batch independence: frame 3 of the batch equals a batch-1 run of the same input, bit for bit."""
    d = model_bytes(name)
    hdr, tensors, _ = marsfile.parse(d)
    tin = tensors[hdr["inputs"][0]]
    nb = marsfile.tensor_nbytes(tin)
    B = 8
    xs = [lcg_frame(0x5EED0000 + f, nb) for f in range(B)]
    m = gpu.Model(d, batch=B, fusion=fusion)
    for f in range(B):
        m.input_view(0)[f, :nb] = xs[f]
    m.run()
    compared = 0
    for f in (0, 7):
        g, rc = run_oracle(orc, d, xs[f])
        assert rc == 0
        for ti, t in enumerate(tensors):
            if t["size"] != 0 or not marsfile.tensor_nbytes(t):
                continue
            try:
                got = m.read_tensor(ti, frame=f)
            except gpu.MarsError:  # elided by a fusion pass, or written by no layer: not in HBM
                if fusion == 0:
                    assert not g.tensor(ti).any(), "tensor %d" % ti
                continue
            want = g.tensor(ti)[:len(got)]
            assert np.array_equal(got, want), "%s fusion %d frame %d tensor %d: %d of %d bytes differ" % (name, fusion, f, ti, int((got != want).sum()), len(got))
            compared += 1
        g.close()
    assert compared >= ((10 if fusion == 0 else 8) if name.startswith("tiny") else 150 if fusion == 0 else 60), compared  # (tiny: two convolution results are elided by fuse_lut at fusion 1)
    keep = [m.read_tensor(ti, frame=3) for ti in range(len(tensors)) if tensors[ti]["size"] == 0 and marsfile.tensor_nbytes(tensors[ti]) and _readable(gpu, m, ti)]
    m.close()
    m1 = gpu.Model(d, batch=1, fusion=fusion)
    m1.input_view(0)[0, :nb] = xs[3]
    m1.run()
    k = 0
    for ti in range(len(tensors)):
        if tensors[ti]["size"] == 0 and marsfile.tensor_nbytes(tensors[ti]) and _readable(gpu, m1, ti):
            assert np.array_equal(m1.read_tensor(ti, frame=0), keep[k]), "frame 3 of the batch differs from its batch-1 run: tensor %d" % ti
            k += 1
    assert k == len(keep)
    m1.close()


def _readable(gpu, m, ti):
    try:
        m.read_tensor(ti, frame=0, nbytes=1)
        return True
    except gpu.MarsError:
        return False


@pytest.mark.parametrize("cfg", [(16, 16, 12, 20, 2), (32, 16, 9, 7, 3), (16, 48, 20, 20, 2), (64, 32, 5, 6, 4)], ids=lambda v: "x".join(str(q) for q in v))
def test_nchw_tagged_bytewise_layers_on_internal_layout(gpu, orc, cfg, monkeypatch):
    """round 6: NCHW-tagged int8 graphs keep convolution-only tensors pixels x channels on the device (mars_plan.c nhwc_internal) -- and the
    reference's byte-wise CONCAT (equal map sizes), stride-1 MAXPOOL and UPSAMPLE, which index shape[1..3] as H, W, C whatever the tag, are
    evaluated ON that layout as functions of flat byte indices (move.hip *_nchwq_kernel); a concat read by one 1 x 1 convolution only keeps
    its first N - 1 rows, the convolution takes the rest from the concat's last input (virtual_concat_q).  A graph with all of it:
    every activation tensor against the oracle at the default fusion level, with the pass switched off (MARS_HIP_NO_NHWC_INTERNAL: every
    byte-wise layer on the reference's bytes) and at fusion level 0; several frames, odd map sizes, 2 - 4 concat inputs."""
    c1, c2, h, w, nin = cfg
    rng = np.random.default_rng(c1 * 100 + h * 10 + nin)
    G = marsfile.Graph()
    N = marsfile.NCHW

    def conv(xin, ic, oc, ih, iw, k=1, st=1):
        oh, ow = (ih + st - 1) // st, (iw + st - 1) // st
        o = G.tensor([1, oc, oh, ow], fmt=N, scale=0.05)
        wt = G.tensor([oc, ic, k, k], fmt=marsfile.OIHW, scale=0.01, data=rng.integers(-127, 128, (oc, ic, k, k), dtype=np.int8))
        b = G.tensor([oc], dtype=marsfile.I32, fmt=marsfile.D1, data=rng.integers(-2000, 2000, oc, dtype=np.int32))
        G.conv(xin, o, wt, b, (k, k), (st, st), pad=marsfile.PAD_SAME)
        return o

    x = G.tensor([1, 16, h, w], fmt=N, scale=0.04)
    a = conv(x, 16, c1, h, w, 3)
    parts = [a] + [conv(x, 16, c2, h, w) for _ in range(nin - 1)]
    cat = G.tensor([1, c1 + c2 * (nin - 1), h, w], fmt=N, scale=0.05)
    G.concat(parts, cat, axis=1)
    o1 = conv(conv(cat, c1 + c2 * (nin - 1), 32, h, w), 32, 16, h, w)  # (two in a row: the first one's result is an internal tensor too)
    p1 = G.tensor([1, c1, h, w], fmt=N, scale=0.05)
    G.pool(a, p1, (5, 5), (1, 1))
    p2 = G.tensor([1, c1, h, w], fmt=N, scale=0.05)
    G.pool(p1, p2, (5, 5), (1, 1))
    cat2 = G.tensor([1, 3 * c1, h, w], fmt=N, scale=0.05)
    G.concat([a, p1, p2], cat2, axis=1)
    o2 = conv(conv(cat2, 3 * c1, 16, h, w), 16, 16, h, w, 3)
    up = G.tensor([1, c1, 2 * h, 2 * w], fmt=N, scale=0.05)
    G.upsample(a, up, 2, 2)
    o3 = conv(up, c1, 16, 2 * h, 2 * w, 3, 2)
    d = G.serialise([x], [o1, o2, o3])
    hdr, tensors, _ = marsfile.parse(d)
    B = 3
    nb = 16 * h * w
    xs = [rng.integers(0, 256, nb, dtype=np.uint8) for _ in range(B)]
    oracles = []
    for f in range(B):
        g, rc = run_oracle(orc, d, xs[f])
        assert rc == 0
        oracles.append(g)
    launches = {}
    for tag, fusion, env in (("internal", 1, None), ("tagged", 1, "1"), ("unfused", 0, None)):
        if env:
            monkeypatch.setenv("MARS_HIP_NO_NHWC_INTERNAL", env)
        else:
            monkeypatch.delenv("MARS_HIP_NO_NHWC_INTERNAL", raising=False)
        m = gpu.Model(d, batch=B, fusion=fusion)
        for f in range(B):
            m.input_view(0)[f] = xs[f]
        m.run()
        launches[tag] = len(m.ops())
        n = 0
        for f in range(B):
            for ti, t in enumerate(tensors):
                if t["size"] != 0 or not marsfile.tensor_nbytes(t):
                    continue
                if tag == "internal" and not _readable(gpu, m, ti):
                    continue  # (the two concat tensors: only their first rows exist)
                got = m.read_tensor(ti, frame=f)
                want = oracles[f].tensor(ti)[:len(got)]
                assert np.array_equal(got, want), "%s frame %d tensor %d: %d of %d bytes differ" % (tag, f, ti, int((got != want).sum()), len(got))
                n += 1
        assert n == B * (len([t for t in tensors if t["size"] == 0 and marsfile.tensor_nbytes(t)]) - (2 if tag == "internal" else 0))
        m.close()
    for g in oracles:
        g.close()
    # on the internal layout a CONCAT layer is ONE launch (on the reference's bytes: one copy per input: - (nin - 1) - 2 launches), and the
    # 1 x 1 convolution that alone reads it runs as two (virtual_concat_q: the concat's first rows + the last input directly: + 2 launches)
    assert launches["internal"] == launches["tagged"] - (nin - 1) - 2 + 2, launches


def test_shipped_file_two_half_batches(gpu, orc):
    """the NCHW-tagged path in the execution mode of the benchmark: a batch of 66 frames runs as two halves on two streams (each half
    with its own relayout scratch range and its own share of every tensor); frames at both ends of both halves, every tensor the plan
    keeps, against the oracle"""
    d = model_bytes("yolov5n_int8")
    hdr, tensors, _ = marsfile.parse(d)
    nb = marsfile.tensor_nbytes(tensors[hdr["inputs"][0]])
    B = 66
    probe = (0, 32, 33, 65)
    xs = {f: lcg_frame(0x5EED0000 + f, nb) for f in probe}
    filler = lcg_frame(0x5EED1234, nb)
    m = gpu.Model(d, batch=B)
    for f in range(B):
        m.input_view(0)[f, :nb] = xs.get(f, filler)
    m.run()
    for f in probe:
        g, rc = run_oracle(orc, d, xs[f])
        assert rc == 0
        n = 0
        for ti, t in enumerate(tensors):
            if t["size"] != 0 or not marsfile.tensor_nbytes(t) or not _readable(gpu, m, ti):
                continue
            got = m.read_tensor(ti, frame=f)
            assert np.array_equal(got, g.tensor(ti)[:len(got)]), "frame %d tensor %d" % (f, ti)
            n += 1
        assert n > 60
        g.close()
    m.close()


def test_f32_zero_tail_k_limit(gpu, orc, monkeypatch):
    """round 6: the reference's byte-wise CONCAT writes C H W BYTES of a float tensor that holds 4 C H W -- in the parity target's private
    zero-initialised buffers all but the first C / 4 + 1 channels of every concat output are exact zeros (checked here on the oracle's own
    tensors), and under the split-bf16 modes a 1 x 1 convolution reading one stops its K loop there (mars_plan.c zero_tail_f32).  The
    float twin with and without the pass (MARS_HIP_NO_ZERO_TAIL): the same floats on every head (a skipped term is +-0 * w: only the sign
    of a zero sum can differ), both inside 1e-4 of the oracle; the plan's multiply count drops; mode 0 keeps the full loop and stays
    bit-identical; mars_hip_write_tensor refuses non-zero bytes where the plan relies on zeros."""
    d = gpu.synth_model(width_x16=4, input_hw=128, seed=9, float32=True)
    hdr, tensors, layers = marsfile.parse(d)
    n = marsfile.tensor_nbytes(tensors[hdr["inputs"][0]]) // 4
    B = 2
    xs = [cases.f32(0x5EED0000 + f, n, 0.0, 1.0).view(np.uint8) for f in range(B)]
    g, rc = run_oracle(orc, d, xs[0])
    assert rc == 0
    cat_ids = [l["outs"][0] for l in layers if l["type"] == marsfile.CONCAT]
    for to in cat_ids:  # the premise, on the reference's semantics
        a = g.tensor(to).view(np.float32).reshape(tensors[to]["shape"][1], -1)
        live = [c for c in range(a.shape[0]) if (a[c] != 0).any()]
        assert max(live) <= a.shape[0] // 4, (to, max(live), a.shape[0])
    want = [g.tensor(ti).copy() for ti in hdr["outputs"]]
    g.close()
    res, macs = {}, {}
    monkeypatch.setenv("MARS_HIP_NO_VCONCAT_F32", "1")  # (the concats materialised: this test is about the zeros IN them; test_f32_virtual_concat has the other plan)
    try:
        gpu.set_tuning("f32_mfma", 3)
        for tag, env in (("limited", None), ("full", "1")):
            if env:
                monkeypatch.setenv("MARS_HIP_NO_ZERO_TAIL", env)
            else:
                monkeypatch.delenv("MARS_HIP_NO_ZERO_TAIL", raising=False)
            m = gpu.Model(d, batch=B)
            for f in range(B):
                m.input_view(0)[f] = xs[f]
            m.run()
            res[tag] = [m.output_view(i).copy() for i in range(len(hdr["outputs"]))]
            macs[tag] = sum(o["macs"] for o in m.ops())
            if tag == "limited":  # a tensor the plan relies on: zeros may be written behind its live bytes, anything else is refused
                to = cat_ids[0]
                nb = marsfile.tensor_nbytes(tensors[to])
                buf = np.zeros(nb, dtype=np.uint8)
                assert gpu.lib().mars_hip_write_tensor(m.p, to, 0, buf.ctypes.data, nb) == 0
                buf[-1] = 1
                assert gpu.lib().mars_hip_write_tensor(m.p, to, 0, buf.ctypes.data, nb) != 0
            m.close()
        assert macs["limited"] < 0.9 * macs["full"]
        for i in range(len(hdr["outputs"])):
            a, b = res["limited"][i].view(np.float32), res["full"][i].view(np.float32)
            assert ((a == b) | (np.isnan(a) & np.isnan(b))).all(), "head %d: the K limit changed a value" % i
            assert close_f32(res["limited"][i][0], want[i]).all()
        monkeypatch.delenv("MARS_HIP_NO_ZERO_TAIL", raising=False)
        gpu.set_tuning("f32_mfma", 0)
        m = gpu.Model(d, batch=1)
        m.input_view(0)[0] = xs[0]
        m.run()
        for i in range(len(hdr["outputs"])):
            assert np.array_equal(m.output_view(i)[0], want[i]), "mode 0 head %d" % i
        m.close()
    finally:
        gpu.set_tuning("f32_mfma", 1)


@pytest.mark.parametrize("mode", [3, 4])
def test_f32_virtual_concat(gpu, orc, mode, monkeypatch):
    """round 6 (mars_plan.c virtual_concat_f32, conv_f32_vcat.hip): no float CONCAT of the twin is materialised -- its readers (C3's cv3, SPPF's
    cv2, the head C3s' cv1 + cv2 pairs) run on a view of the concat's LAST input (W (N - 1) bytes in front of it, a quarter of the K loop) and a
    head launch recomputes the first (N - 1) W / 4 pixels of every output plane from the other inputs' first bytes.  Against the plan with the
    concats materialised (MARS_HIP_NO_VCONCAT_F32), three frames: the first concat's reader -- same operands in both plans -- is bit-identical
    from pixel s on and within 1e-5 before it; every head within 1e-4 of the oracle and of the other plan; the concat tensors do not exist."""
    d = gpu.synth_model(width_x16=4, input_hw=128, seed=9, float32=True)
    hdr, tensors, layers = marsfile.parse(d)
    n = marsfile.tensor_nbytes(tensors[hdr["inputs"][0]]) // 4
    B = 3
    xs = [cases.f32(0x5EED0000 + f, n, 0.0, 1.0).view(np.uint8) for f in range(B)]
    cat_ids = [l["outs"][0] for l in layers if l["type"] == marsfile.CONCAT]
    try:
        gpu.set_tuning("f32_mfma", mode)
        monkeypatch.delenv("MARS_HIP_NO_VCONCAT_F32", raising=False)
        plan = gpu.describe_plan(d)
        views = [l for l in plan if " view=-" in l]
        heads = [l for l in plan if " conv_f32_vhead " in l]
        assert len(views) == 17 and len(heads) == 17 and not any(" concat_slice " in l for l in plan)
        t_first = int(views[0].split(" out ")[1].split()[0])
        nf, run = (int(v) for v in heads[0].split(" vcat=")[1].split()[0].split("x"))
        s_pix = nf * run
        got = {}
        for tag, env in (("virtual", None), ("copied", "1")):
            if env:
                monkeypatch.setenv("MARS_HIP_NO_VCONCAT_F32", env)
            else:
                monkeypatch.delenv("MARS_HIP_NO_VCONCAT_F32", raising=False)
            m = gpu.Model(d, batch=B)
            for f in range(B):
                m.input_view(0)[f] = xs[f]
            m.run()
            got[tag] = {"heads": [m.output_view(i).copy() for i in range(len(hdr["outputs"]))],
                        "first": [m.read_tensor(t_first, frame=f).view(np.float32).copy() for f in range(B)],
                        "launches": len(m.ops()), "readable": [_readable(gpu, m, t) for t in cat_ids]}
            m.close()
        assert got["virtual"]["readable"] == [False] * len(cat_ids) and got["copied"]["readable"] == [True] * len(cat_ids)
        # 13 concats = 29 slice launches gone, 17 head launches added
        assert got["virtual"]["launches"] == got["copied"]["launches"] - sum(len(l["ins"]) for l in layers if l["type"] == marsfile.CONCAT) + 17
        C = tensors[t_first]["shape"][1]
        for f in range(B):
            a, b = got["virtual"]["first"][f].reshape(C, -1), got["copied"]["first"][f].reshape(C, -1)
            assert s_pix < a.shape[1] and np.array_equal(a[:, s_pix:], b[:, s_pix:]), "frame %d: the view changed a value behind the head pixels" % f
            assert np.isfinite(a[:, :s_pix]).all() and (np.abs(a[:, :s_pix] - b[:, :s_pix]) <= 1e-5 * np.maximum(1.0, np.abs(b[:, :s_pix]))).all(), "frame %d: head pixels" % f
        for f in range(B):
            g, rc = run_oracle(orc, d, xs[f])
            assert rc == 0
            for i, ti in enumerate(hdr["outputs"]):
                assert close_f32(got["virtual"]["heads"][i][f], g.tensor(ti)).all(), "frame %d head %d against the oracle" % (f, i)
                assert close_f32(got["virtual"]["heads"][i][f], got["copied"]["heads"][i][f]).all(), "frame %d head %d against the other plan" % (f, i)
            g.close()
    finally:
        gpu.set_tuning("f32_mfma", 1)


@pytest.mark.parametrize("cfg", [(3, 6, 2, 16, 36, 44), (3, 3, 1, 16, 20, 20), (1, 5, 2, 32, 18, 50), (4, 3, 1, 48, 11, 16), (2, 6, 2, 7, 21, 36), (3, 8, 3, 32, 40, 90),
                                 (3, 6, 2, 32, 130, 132), (3, 3, 2, 16, 9, 4)], ids=lambda v: "x".join(str(q) for q in v))
def test_nchw_stem_reads_planes(gpu, orc, cfg, monkeypatch):
    """round 6: the small-channel first layer of an NCHW-tagged graph ([C <= 4][H][W] bytes in) -- conv_i8_smallc interleaves the planes while it
    stages its patch (mhip_conv_i8_t.in_planar) instead of a relayout launch in front.  1 - 4 planes, kernels 3 - 8, strides 1 - 3, maps whose
    width is not a multiple of the 4-pixel staging unit, edges on every side (SAME padding), several frames: bit for bit against the oracle,
    with the planar form and with MARS_HIP_NO_PLANAR_STEM (the relayout in front), at fusion levels 1 and 0."""
    c, k, st, oc, h, w = cfg
    rng = np.random.default_rng(c * 1000 + k * 100 + st * 10 + oc)
    G = marsfile.Graph()
    x = G.tensor([1, c, h, w], fmt=marsfile.NCHW, scale=0.02)
    oh, ow = (h + st - 1) // st, (w + st - 1) // st
    o = G.tensor([1, oc, oh, ow], fmt=marsfile.NCHW, scale=0.05)
    wt = G.tensor([oc, c, k, k], fmt=marsfile.OIHW, scale=0.004, data=rng.integers(-127, 128, (oc, c, k, k), dtype=np.int8))
    b = G.tensor([oc], dtype=marsfile.I32, fmt=marsfile.D1, data=rng.integers(-3000, 3000, oc, dtype=np.int32))
    G.conv(x, o, wt, b, (k, k), (st, st), pad=marsfile.PAD_SAME)
    o2 = G.tensor([1, oc, oh, ow], fmt=marsfile.NCHW, scale=0.04)
    G.layer(marsfile.RELU, [o], [o2])
    d = G.serialise([x], [o2])
    hdr, tensors, _ = marsfile.parse(d)
    B = 3
    xs = [rng.integers(0, 256, c * h * w, dtype=np.uint8) for _ in range(B)]
    want = []
    for f in range(B):
        g, rc = run_oracle(orc, d, xs[f])
        assert rc == 0
        want.append(g.tensor(hdr["outputs"][0]).copy())
        g.close()
    for env in (None, "1"):
        if env:
            monkeypatch.setenv("MARS_HIP_NO_PLANAR_STEM", env)
        else:
            monkeypatch.delenv("MARS_HIP_NO_PLANAR_STEM", raising=False)
        for fusion in (1, 0):
            m = gpu.Model(d, batch=B, fusion=fusion)
            for f in range(B):
                m.input_view(0)[f] = xs[f]
            m.run()
            for f in range(B):
                assert np.array_equal(m.output_view(0)[f], want[f]), "planar=%s fusion %d frame %d" % (env is None, fusion, f)
            m.close()
