"""fuse_split_chain on the CPU (mars_hip_describe_plan's full form, no device): which fused cv1 + cv2 launches also take the bottleneck's m.cv1, the
switches, and the host packer of the chained 1x1's weight image.  The results of every such plan are checked bit for bit by
tests/test_gpu_chain_fusion.py."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

import cases
from test_oracle import model_bytes

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, "..", "thingino-accel_amd"))

FULL = 2  # MARS_HIP_DESCRIBE_FULL


def ops(lines):
    return [l for l in lines if l.startswith("op ")]


def field(line, name):
    """the integers behind ` name` in the full part of an op line"""
    return line.split(" | ", 1)[1].split(" %s " % name, 1)[1].split()


def chain_sites(lines):
    """(k x k's layer, cv1's, cv2's, the chained 1x1's layer, side) of every fused launch that carries a chain; the four ops sit in a row"""
    o = ops(lines)
    res = []
    for i, l in enumerate(o):
        if " | " not in l or " split_chain " not in l:
            continue
        side = int(field(l, "split_chain")[0])
        if not side:
            continue
        assert int(field(l, "split_next")[0]) == 1 and " split_next" in l.split(" | ")[0], l
        assert int(field(l, "split_chain")[1]) > 0, l  # the image's arena offset
        b, c, d = o[i + 1], o[i + 2], o[i + 3]
        ds = d.split(" | ")[0] + " "
        assert " k1x1 s1 c32->32 " in ds and " lut" in ds and " add=" not in ds and " pair_next" not in ds and " seg=" not in ds, d
        src = (b, c)[side - 1].split(" out ")[1].split()[0]
        assert d.split(" in ")[1].split()[0] == src, (l, b, c, d)
        assert int(field(d, "split_chain")[0]) == 0
        res.append((int(l.split()[3]), int(b.split()[3]), int(c.split()[3]), int(d.split()[3]), side))
    return res


def count(lines, what):
    return sum(what in l for l in lines)


@pytest.fixture(autouse=True)
def _switches(monkeypatch):
    for k in ("MARS_HIP_NO_CHAIN", "MARS_HIP_NO_SPLIT", "MARS_HIP_NO_POST", "MARS_HIP_FUSION"):
        monkeypatch.delenv(k, raising=False)


@pytest.mark.parametrize("hw", [640, 320])
def test_headline_twin_site(marsrt, hw):
    """the yolov5s twin: layer 12 (the first bottleneck's m.cv1) rides on the site (3, 6, 9); it reads cv1's side"""
    L = marsrt.describe_plan(marsrt.synth_model(width_x16=8, input_hw=hw, seed=1), FULL)
    assert chain_sites(L) == [(3, 6, 9, 12, 1)]
    assert sum(" conv_i8 " in l for l in ops(L)) == 60  # every op stays in the plan


def test_yolov5n_twin_site(marsrt):
    L = marsrt.describe_plan(marsrt.synth_model(width_x16=4, input_hw=640, seed=1), FULL)
    assert chain_sites(L) == [(23, 26, 29, 32, 1)]


def test_yolov5n_twin_at_320_has_no_site(marsrt):
    """no fused pair there (the patch kernel's fill rule), so nothing to chain to"""
    L = marsrt.describe_plan(marsrt.synth_model(width_x16=4, input_hw=320, seed=1), FULL)
    assert chain_sites(L) == [] and count(L, " split_next 1") == 0


@pytest.mark.parametrize("name", cases.SHIPPED)
def test_shipped_files_have_no_site(marsrt, name):
    assert chain_sites(marsrt.describe_plan(model_bytes(name), FULL)) == []


def test_switches_and_the_short_form(marsrt, monkeypatch):
    d = marsrt.synth_model(width_x16=8, input_hw=640, seed=1)
    short, full = marsrt.describe_plan(d), marsrt.describe_plan(d, FULL)
    assert " no_chain 0 " in full[-1] and full[-1].startswith("+plan")
    assert count(short, "split_chain") == 0
    # MARS_HIP_NO_CHAIN: the chain goes, the split stays, the short form does not change by a byte
    monkeypatch.setenv("MARS_HIP_NO_CHAIN", "1")
    short0, full0 = marsrt.describe_plan(d), marsrt.describe_plan(d, FULL)
    assert short0 == short
    assert chain_sites(full0) == [] and count(full0, " split_next 1 ") == 1 and " no_chain 1 " in full0[-1]
    assert count(full0, " split_chain 0") == sum(" | " in l for l in ops(full0))
    monkeypatch.delenv("MARS_HIP_NO_CHAIN")
    # MARS_HIP_NO_SPLIT removes both
    monkeypatch.setenv("MARS_HIP_NO_SPLIT", "1")
    full1 = marsrt.describe_plan(d, FULL)
    assert chain_sites(full1) == [] and count(full1, " split_next 1 ") == 0
    monkeypatch.delenv("MARS_HIP_NO_SPLIT")
    # fusion level 0 never runs either pass; level 2 has folded m.cv1 into the following 3x3 (`pre`): there is no op to take
    monkeypatch.setenv("MARS_HIP_FUSION", "0")
    assert chain_sites(marsrt.describe_plan(d, FULL)) == []
    monkeypatch.setenv("MARS_HIP_FUSION", "2")
    full2 = marsrt.describe_plan(d, FULL)
    assert chain_sites(full2) == [] and count(full2, " split_next 1 ") == 1


def test_chain_pack_is_the_1x1_in_the_lanes_order(marsrt):
    """mhip_conv_i8_chain_pack: size, every weight at its row and K position, zero pads; one tile row emulated as the lanes hold it"""
    L = marsrt.lib()
    L.mhip_conv_i8_chain_pack.restype = C.c_size_t
    L.mhip_conv_i8_chain_pack.argtypes = [C.c_void_p] * 3
    rng = np.random.default_rng(32)
    rows = np.array([L.mhip_conv_i8_oc_row(oc, 32) for oc in range(32)])
    w = rng.integers(-128, 128, (32, 32), dtype=np.int8)  # [out channel][input channel]
    w[w == 0] = 1  # so that a pad byte cannot pass for a weight
    bias = rng.integers(-5000, 5000, 32, dtype=np.int32)
    packed = np.zeros((32, 64), np.int8)  # as every conv_i8 launch reads them: rows permuted, K padded to 64
    packed[rows, :32] = w
    pbias = np.zeros(32, np.int32)
    pbias[rows] = bias
    size = L.mhip_conv_i8_chain_pack(None, None, None)
    assert size == 32 * 64 + 32 * 4
    img = np.full(size, 0x55, np.int8)
    assert L.mhip_conv_i8_chain_pack(packed.ctypes.data, pbias.ctypes.data, img.ctypes.data) == size
    # undo the LDS layout: row R, 16-byte chunk swizzled by ((R >> 1) & 2)
    wk = np.zeros((32, 64), np.int64)
    for R in range(32):
        for k in range(64):
            wk[R, k] = img[R * 64 + (((k >> 4) ^ ((R >> 1) & 2)) << 4) + (k & 15)]
    prow = np.array([L.mhip_conv_i8_split_row(0, oc) for oc in range(32)])
    assert sorted(prow) == list(range(32))
    kpos = np.array([L.mhip_conv_i8_chain_k(c) for c in range(32)])
    assert list(kpos) == [16 * (c >> 3) + (c & 7) for c in range(32)]
    for oc in range(32):
        g, rem = divmod(oc, 8)
        assert prow[oc] == (rem >> 2) * 16 + g * 4 + (rem & 3)
        assert np.array_equal(wk[prow[oc], kpos], w[oc]), oc
    pad = np.array([16 * g + 8 + j for g in range(4) for j in range(8)])
    assert not wk[:, pad].any()
    assert np.array_equal(img[32 * 64:].view(np.int32)[prow], bias)
    # one tile row: 16 pixels; lane (pixel i, group g) holds input channels 8g .. 8g + 7 as two packed words, then eight zero bytes
    x = rng.integers(-128, 128, (16, 32), dtype=np.int8)
    B = np.zeros((16, 64), np.int64)
    for i in range(16):
        for g in range(4):
            B[i, 16 * g:16 * g + 8] = x[i, 8 * g:8 * g + 8]
    acc = B @ wk.T + img[32 * 64:].view(np.int32).astype(np.int64)  # [pixel][image row]
    want = x.astype(np.int64) @ w.astype(np.int64).T + bias
    # MFMA r, lane group g, element e = image row r * 16 + 4 g + e = output channel 8 g + 4 r + e
    for g in range(4):
        for r in range(2):
            for e in range(4):
                assert np.array_equal(acc[:, r * 16 + 4 * g + e], want[:, 8 * g + 4 * r + e])
    # bias NULL = zeros
    img0 = np.full(size, 0x55, np.int8)
    L.mhip_conv_i8_chain_pack(packed.ctypes.data, None, img0.ctypes.data)
    assert np.array_equal(img0[:32 * 64], img[:32 * 64]) and not img0[32 * 64:].any()
