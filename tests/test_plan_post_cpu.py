"""fuse_post on the CPU (mars_hip_describe_plan, no device): which 3x3 convolutions take the C3's cv3 into their launch, and the host packer
of cv3's weight image.  The results of every such plan are checked bit for bit by tests/test_gpu_post_fusion.py."""
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
    """(3x3's layer, channels, cv3's layer) of every fused launch"""
    o = ops(lines)
    res = []
    for i, l in enumerate(o):
        if " post_next" in l:
            assert " k3x3 s1 " in l and " k1x1 s1 " in o[i + 1] and " seg=2" in o[i + 1] and " post_next" not in o[i + 1], (l, o[i + 1])
            res.append((int(l.split()[3]), int(l.split("->")[1].split()[0]), int(o[i + 1].split()[3])))
    return res


def count(lines, what):
    return sum(what in l for l in lines)


def test_headline_twin_sites(marsrt, monkeypatch):
    """the yolov5s twin at 640: the backbone's 160 x 160 (32 channels, Add) and 80 x 80 (64 channels, second bottleneck, Add) blocks and the neck's
    80 x 80 one (64 channels, no Add); the plan keeps every op (a fused 1x1 stays, unlaunched, as a pair's mate does)"""
    monkeypatch.delenv("MARS_HIP_NO_POST", raising=False)
    d = marsrt.synth_model(width_x16=8, input_hw=640, seed=1)
    L = marsrt.describe_plan(d)
    assert sites(L) == [(15, 32, 20), (42, 64, 47), (149, 64, 153)]
    fused = [l for l in ops(L) if " post_next" in l]
    assert " add=" in fused[0] and " add=" in fused[1] and " add=" not in fused[2]
    monkeypatch.setenv("MARS_HIP_NO_POST", "1")
    L0 = marsrt.describe_plan(d)
    assert count(L0, " post_next") == 0
    for plan in (L, L0):
        assert sum(" conv_i8 " in l for l in ops(plan)) == 60 and count(plan, " seg=") == 17 and count(plan, " pair_next") == 4 and count(plan, " add=") == 7
    # the two plans differ in the flag and in the mirrored operand only
    strip = lambda l: l.replace(" post_next", "")
    diff = [(a, b) for a, b in zip(ops(L), ops(L0)) if strip(a) != b]
    assert len(diff) == 3 and all(" post_next" in a for a, _ in diff)


def test_yolov5n_twin_sites(marsrt, monkeypatch):
    """width 4: the 32-channel blocks at 80 x 80 fuse, the 16-channel one at 160 x 160 does not (the stage takes 32 / 64 channels)"""
    monkeypatch.delenv("MARS_HIP_NO_POST", raising=False)
    L = marsrt.describe_plan(marsrt.synth_model(width_x16=4, input_hw=640, seed=1))
    assert sites(L) == [(42, 32, 47), (149, 32, 153)]
    assert not any(" post_next" in l and " c16->16 " in l for l in L)


def test_fusion_level_2_keeps_its_plans(marsrt, monkeypatch):
    """an op that carries `pre` never takes `post`"""
    monkeypatch.delenv("MARS_HIP_NO_POST", raising=False)
    monkeypatch.setenv("MARS_HIP_FUSION", "2")
    L = marsrt.describe_plan(marsrt.synth_model(width_x16=8, input_hw=640, seed=1))
    assert count(L, " pre") > 0 and not any(" pre" in l.replace(" post_next", "") and " post_next" in l for l in ops(L))


@pytest.mark.parametrize("name", cases.SHIPPED)
def test_shipped_files_have_no_site(marsrt, monkeypatch, name):
    monkeypatch.delenv("MARS_HIP_NO_POST", raising=False)
    assert count(marsrt.describe_plan(model_bytes(name)), " post_next") == 0


@pytest.mark.parametrize("c", [32, 64])
def test_post_pack_is_the_1x1_in_another_order(marsrt, c):
    """mhip_conv_i8_post_pack: a plain int8 GEMM over the image's K order and row order equals the 1x1 in natural order"""
    L = marsrt.lib()
    L.mhip_conv_i8_post_pack.restype = C.c_size_t
    L.mhip_conv_i8_post_pack.argtypes = [C.c_int, C.c_void_p, C.c_void_p, C.c_void_p]
    n = 2 * c
    rng = np.random.default_rng(c)
    w = rng.integers(-128, 128, (n, n), dtype=np.int8)   # [out channel][input channel: u 0..c-1, y2 c..2c-1]
    bias = rng.integers(-5000, 5000, n, dtype=np.int32)
    x = rng.integers(-128, 128, n, dtype=np.int8)
    rows = np.array([L.mhip_conv_i8_oc_row(oc, n) for oc in range(n)])
    assert sorted(rows) == list(range(n))
    packed = np.zeros((n, n), np.int8)
    packed[rows] = w
    pbias = np.zeros(n, np.int32)
    pbias[rows] = bias
    size = L.mhip_conv_i8_post_pack(c, None, None, None)
    assert size == n * n + 4 * n and L.mhip_conv_i8_post_pack(48, None, None, None) == 0
    img = np.zeros(size, np.int8)
    assert L.mhip_conv_i8_post_pack(c, packed.ctypes.data, pbias.ctypes.data, img.ctypes.data) == size
    pos = np.array([L.mhip_conv_i8_post_k(c, k) for k in range(n)])
    prow = np.array([L.mhip_conv_i8_post_row(c, oc) for oc in range(n)])
    assert sorted(pos) == list(range(n)) and sorted(prow) == list(range(n))
    if c == 32:  # chunk g = [u 8g..8g+7 | y2 8g..8g+7]
        assert [int(np.where(pos == p)[0][0]) for p in range(16)] == list(range(8)) + list(range(32, 40))
    # undo the LDS layout: K step ks, row R, 16-byte chunk swizzled by ((R >> 1) & 2)
    wk = np.zeros((n, n), np.int64)
    for R in range(n):
        for p in range(n):
            ks, chunk, b = p >> 6, (p & 63) >> 4, p & 15
            wk[R, p] = img[(ks * n + R) * 64 + ((chunk ^ ((R >> 1) & 2)) << 4) + b]
    xk = np.zeros(n, np.int64)
    xk[pos] = x
    got = wk @ xk + img[n * n:].view(np.int32)
    want = w.astype(np.int64) @ x.astype(np.int64) + bias
    assert np.array_equal(got[prow], want)
    # a lane group's 2c / 4 results are consecutive channels: rows s * 16 + g * 4 + r <-> channel g * (2c / 4) + s * 4 + r
    for oc in range(n):
        g, rem = divmod(oc, n // 4)
        assert prow[oc] == (rem >> 2) * 16 + g * 4 + (rem & 3)
