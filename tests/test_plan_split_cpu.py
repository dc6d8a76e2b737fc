"""fuse_split on the CPU (mars_hip_describe_plan, no device): which k x k convolutions take the C3's cv1 + cv2 pair into their launch, and the
host packer of the pair's weight image.  The results of every such plan are checked bit for bit by tests/test_gpu_split_fusion.py."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

import cases
from test_oracle import model_bytes

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, "..", "thingino-accel_amd"))


def ops(lines):
    return [l for l in lines if l.startswith("op ")]


def sites(lines):
    """(k x k's layer, cv1's layer, cv2's layer) of every fused launch; the three ops sit in a row, the first mate keeps its pair_next"""
    o = ops(lines)
    res = []
    for i, l in enumerate(o):
        if " split_next" in l:
            b, c = o[i + 1], o[i + 2]
            assert " k3x3 " in l and "->64 " in l and " pair_next" not in l and " post_next" not in l, l
            for mate in (b, c):
                assert " k1x1 s1 c64->32 " in mate and " split_next" not in mate, mate
            assert " pair_next" in b and " pair_next" not in c, (b, c)
            t = l.split(" out ")[1].split()[0]
            assert b.split(" in ")[1].split()[0] == t and c.split(" in ")[1].split()[0] == t, (l, b, c)
            res.append((int(l.split()[3]), int(b.split()[3]), int(c.split()[3])))
    return res


def count(lines, what):
    return sum(what in l for l in lines)


@pytest.fixture(autouse=True)
def _switches(monkeypatch):
    for k in ("MARS_HIP_NO_SPLIT", "MARS_HIP_NO_POST", "MARS_HIP_FUSION"):
        monkeypatch.delenv(k, raising=False)


@pytest.mark.parametrize("hw", [640, 320])
def test_headline_twin_site(marsrt, monkeypatch, hw):
    """the yolov5s twin: the stride-2 3x3 to 64 channels (layer 3) takes the first C3's cv1 + cv2 (layers 6, 9); the plan keeps every op"""
    d = marsrt.synth_model(width_x16=8, input_hw=hw, seed=1)
    L = marsrt.describe_plan(d)
    assert sites(L) == [(3, 6, 9)]
    assert " s2 c32->64 " in [l for l in ops(L) if " split_next" in l][0]
    assert sum(" conv_i8 " in l for l in ops(L)) == 60 and count(L, " seg=") == 17 and count(L, " pair_next") == 4 and count(L, " add=") == 7
    # the switch: no flag, every other line of the plan unchanged
    monkeypatch.setenv("MARS_HIP_NO_SPLIT", "1")
    L0 = marsrt.describe_plan(d)
    assert count(L0, " split_next") == 0
    assert [l.replace(" split_next", "") for l in L] == L0


def test_yolov5n_twin_site(marsrt):
    """width 4: one level down (layer 23 with 26, 29); its layer 3 makes 32 channels and has no site"""
    L = marsrt.describe_plan(marsrt.synth_model(width_x16=4, input_hw=640, seed=1))
    assert sites(L) == [(23, 26, 29)]
    l3 = [l for l in ops(L) if l.split()[3] == "3"]
    assert len(l3) == 1 and " split_next" not in l3[0] and "->32 " in l3[0]


def test_yolov5n_twin_at_320_is_below_the_fill_rule(marsrt):
    """width 4 at 320: layer 23 writes a 40 x 40 map, 40 of a tile row's 48 columns = 0.83 of full tiles at best: the patch-staged kernel does not
    take the shape (its 85 % fill rule), so mhip_conv_i8_split_ok declines and the pair stays a launch of its own"""
    L = marsrt.describe_plan(marsrt.synth_model(width_x16=4, input_hw=320, seed=1))
    assert sites(L) == []
    l23 = [l for l in ops(L) if l.split()[3] == "23"]
    assert len(l23) == 1 and " k3x3 s2 c32->64 " in l23[0]
    i = ops(L).index(l23[0])
    assert " pair_next" in ops(L)[i + 1] and " k1x1 s1 c64->32 " in ops(L)[i + 1] and " k1x1 s1 c64->32 " in ops(L)[i + 2]


def test_fusion_levels_and_the_other_switch(marsrt, monkeypatch):
    """level 2 and MARS_HIP_NO_POST keep the site; level 0 never runs the pass"""
    d = marsrt.synth_model(width_x16=8, input_hw=640, seed=1)
    monkeypatch.setenv("MARS_HIP_NO_POST", "1")
    L = marsrt.describe_plan(d)
    assert sites(L) == [(3, 6, 9)] and count(L, " post_next") == 0
    monkeypatch.delenv("MARS_HIP_NO_POST")
    monkeypatch.setenv("MARS_HIP_FUSION", "2")
    L = marsrt.describe_plan(d)
    assert sites(L) == [(3, 6, 9)] and count(L, " pre") > 0
    monkeypatch.setenv("MARS_HIP_FUSION", "0")
    assert count(marsrt.describe_plan(d), " split_next") == 0


@pytest.mark.parametrize("name", cases.SHIPPED)
def test_shipped_files_have_no_site(marsrt, name):
    assert count(marsrt.describe_plan(model_bytes(name)), " split_next") == 0


def test_split_pack_is_both_1x1s_in_another_order(marsrt):
    """mhip_conv_i8_split_pack: a plain int8 GEMM over the image's K and row order equals both 1x1s in natural order"""
    L = marsrt.lib()
    L.mhip_conv_i8_split_pack.restype = C.c_size_t
    L.mhip_conv_i8_split_pack.argtypes = [C.c_void_p] * 5
    rng = np.random.default_rng(64)
    rows = np.array([L.mhip_conv_i8_oc_row(oc, 32) for oc in range(32)])
    assert sorted(rows) == list(range(32))
    w, bias, packed, pbias = [], [], [], []
    for side in range(2):  # [out channel][input channel], as every conv_i8 launch reads them: rows permuted by mhip_conv_i8_oc_row
        w.append(rng.integers(-128, 128, (32, 64), dtype=np.int8))
        bias.append(rng.integers(-5000, 5000, 32, dtype=np.int32))
        pw = np.zeros((32, 64), np.int8)
        pw[rows] = w[side]
        pb = np.zeros(32, np.int32)
        pb[rows] = bias[side]
        packed.append(pw)
        pbias.append(pb)
    x = rng.integers(-128, 128, 64, dtype=np.int8)
    size = L.mhip_conv_i8_split_pack(None, None, None, None, None)
    assert size == 64 * 64 + 4 * 64
    img = np.zeros(size, np.int8)
    assert L.mhip_conv_i8_split_pack(packed[0].ctypes.data, pbias[0].ctypes.data, packed[1].ctypes.data, pbias[1].ctypes.data, img.ctypes.data) == size
    # undo the LDS layout: row R, 16-byte chunk swizzled by ((R >> 1) & 2); K in natural order
    wk = np.zeros((64, 64), np.int64)
    for R in range(64):
        for k in range(64):
            wk[R, k] = img[R * 64 + (((k >> 4) ^ ((R >> 1) & 2)) << 4) + (k & 15)]
    got = wk @ x.astype(np.int64) + img[64 * 64:].view(np.int32)
    prow = [np.array([L.mhip_conv_i8_split_row(side, oc) for oc in range(32)]) for side in range(2)]
    assert sorted(list(prow[0]) + list(prow[1])) == list(range(64))
    for side in range(2):
        want = w[side].astype(np.int64) @ x.astype(np.int64) + bias[side]
        assert np.array_equal(got[prow[side]], want), side
        # a round is one side's 32 rows; a lane group's 8 results are consecutive channels: row side * 32 + s * 16 + g * 4 + r <-> channel g * 8 + s * 4 + r
        for oc in range(32):
            g, rem = divmod(oc, 8)
            assert prow[side][oc] == side * 32 + (rem >> 2) * 16 + g * 4 + (rem & 3)
    # the two sides are told apart: swapping them changes the image
    img2 = np.zeros(size, np.int8)
    L.mhip_conv_i8_split_pack(packed[1].ctypes.data, pbias[1].ctypes.data, packed[0].ctypes.data, pbias[0].ctypes.data, img2.ctypes.data)
    assert np.array_equal(img2[:32 * 64], img[32 * 64:64 * 64]) and not np.array_equal(img2, img)
