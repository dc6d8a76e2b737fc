"""Instance masks without a device: the numpy restatement of include/mars_hip.h "Instance masks" (tests/segref.py) on hand-worked cases,
the records' and options' layout, and the synthetic writer's seg head."""
import ctypes as C
import hashlib
import os
import subprocess

import numpy as np
import pytest

import marsfile
import segref

F32 = np.float32
INC = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include")
FULL = (32.0, 32.0, 64.0, 64.0)  # a box over the whole 64 x 64 input


def _proto(nm, ph, pw, fill=0):
    return np.full((nm, ph, pw), fill, dtype=np.int8)


def test_dot_zero_plus_one_minus_one():
    """a = (1, 1): P = (1, -1) -> 0 (bit 0), (1, 0) -> +1 (bit 1), (0, -1) -> -1 (bit 0)"""
    p = _proto(2, 2, 16)
    p[:, 0, 0] = (1, -1)
    p[:, 0, 1] = (1, 0)
    p[:, 0, 2] = (0, -1)
    p[:, 1, 5] = (3, -2)
    (x0, y0, x1, y1, area), w = segref.mask_literal([1, 1], p, FULL, 64, 64, 1.0)
    assert (x0, y0, x1, y1) == (0, 0, 16, 2)
    assert w.tolist() == [[0b10], [1 << 5]] and area == 2


def test_extreme_dot_and_logit_min():
    """nm * (-128) * (-128) at nm = 64 is 2^20: exact in int32 and in float32; the compare is strict"""
    p = _proto(64, 1, 16, -128)
    a = np.full(64, -128, dtype=np.int8)
    for lm, bit in ((0.0, 1), (1048575.5, 1), (1048576.0, 0)):
        (_, _, _, _, area), w = segref.mask_literal(a, p, FULL, 64, 64, 1.0, lm)
        assert area == 16 * bit and w.tolist() == [[0xFFFF * bit]], lm
    # s = 0.5: dot 3 -> 1.5 > 1.0, dot 2 -> 1.0 is not > 1.0, dot -3 -> -1.5 > -2.0
    q = _proto(1, 1, 16)
    q[0, 0, :3] = (3, 2, -3)
    assert segref.mask_literal([1], q, FULL, 64, 64, 0.5, 1.0)[1].tolist() == [[0b001]]
    assert segref.mask_literal([1], q, FULL, 64, 64, 0.5, -2.0)[1].tolist() == [[0xFFFF]]
    assert segref.mask_literal([1], q, FULL, 64, 64, 0.5, -1.5)[1].tolist() == [[0xFFFF & ~0b100]]


@pytest.mark.parametrize("box, want", [
    ((32, 32, 16, 16), (6, 6, 10, 10)),      # edges at 6.0 and 10.0: floor and ceil leave them
    ((34, 30, 16, 16), (6, 5, 11, 10)),      # 6.5 -> 6, 10.5 -> 11; 5.5 -> 5, 9.5 -> 10
    ((0, 64, 16, 16), (0, 14, 2, 16)),       # partly outside: -2 -> 0, 18 -> 16
    ((-100, 32, 16, 16), (0, 6, 0, 10)),     # wholly outside on the left: empty
    ((1000, 1000, 16, 16), (16, 16, 16, 16)),  # ... on the right and below
    ((32, 32, 0, 0), (8, 8, 8, 8)),          # w = 0 on a pixel edge: empty
    ((34, 34, 0, 0), (8, 8, 9, 9)),          # w = 0 inside a pixel: that pixel
    ((32, 32, -8, 4), (9, 7, 7, 9)),         # negative width: x1 < x0, empty
    ((np.nan, 32, 16, 16), (0, 6, 0, 10)),
    ((32, 32, np.inf, 16), (0, 6, 16, 10)),
])
def test_rectangle(box, want):
    assert segref.rect(box, 64, 64, 16, 16) == want
    p = _proto(1, 16, 16, 1)
    (x0, y0, x1, y1, area), w = segref.mask_literal([1], p, box, 64, 64, 1.0)
    assert (x0, y0, x1, y1) == want
    assert area == max(x1 - x0, 0) * max(y1 - y0, 0)
    bits = segref.unpack(w, 16)
    for y in range(16):
        for x in range(16):
            assert bits[y, x] == (x0 <= x < x1 and y0 <= y < y1)


def test_rectangle_uses_both_axes_factors():
    """a 160 x 96 input with 40 x 12 prototypes: fx = 0.25, fy = 0.125"""
    assert segref.rect((80, 48, 40, 48), 160, 96, 40, 12) == (15, 3, 25, 9)


@pytest.mark.parametrize("pw, last", [(16, 0xFFFF), (32, 0xFFFFFFFF), (33, 1), (40, 0xFF)])
def test_padding_bits_and_word_boundaries(pw, last):
    p = _proto(1, 2, pw, 1)
    (_, _, x1, _, area), w = segref.mask_literal([1], p, (pw * 2, 4, pw * 4, 8), pw * 4, 8, 1.0)
    pitch = (pw + 31) // 32
    assert x1 == pw and area == 2 * pw and w.shape == (2, pitch)
    assert w[0].tolist() == [0xFFFFFFFF] * (pitch - 1) + [last]
    # one pixel on each side of the word boundary
    if pw > 32:
        q = _proto(1, 1, pw)
        q[0, 0, 31] = q[0, 0, 32] = 1
        assert segref.mask_literal([1], q, (pw * 2, 2, pw * 4, 4), pw * 4, 4, 1.0)[1].tolist() == [[1 << 31, 1]]


def test_array_form_equals_the_literal_loops():
    rng = np.random.default_rng(11)
    for nm, ph, pw in ((1, 3, 16), (4, 5, 33), (33, 4, 40), (64, 2, 32)):
        p = rng.integers(-128, 128, (nm, ph, pw), dtype=np.int8)
        p[:, 1, 3] = 0  # a dot of exactly 0 inside the box
        for k in range(4):
            a = rng.integers(-128, 128, nm, dtype=np.int8)
            box = (rng.uniform(0, 64), rng.uniform(0, 64), rng.uniform(0, 80), rng.uniform(0, 80))
            lm = (0.0, 0.0, 2.5, -1.0)[k]
            r0, w0 = segref.mask_literal(a, p, box, 64, 64, 0.01, lm)
            r1, w1 = segref.mask_array(a, p, box, 64, 64, 0.01, lm)
            assert r0 == r1 and np.array_equal(w0, w1)
            assert np.array_equal(segref.pack(segref.unpack(w0, pw)), w0)


def test_selection_and_unused_slots():
    boxes = np.zeros(6, dtype=[("x", "<f4"), ("y", "<f4"), ("w", "<f4"), ("h", "<f4"), ("conf", "<f4"), ("cls", "<i4")])
    boxes["x"], boxes["y"], boxes["w"], boxes["h"] = 32, 32, 16, 16
    boxes["conf"] = (0.9, 0.3, 0.8, 0.8, 0.2, 0.7)
    assert segref.select(boxes["conf"], 0.0, 16) == [0, 1, 2, 3, 4, 5]
    assert segref.select(boxes["conf"], 0.5, 16) == [0, 2, 3, 5]
    assert segref.select(boxes["conf"], 0.5, 3) == [0, 2, 3]
    assert segref.select(boxes["conf"], 0.8, 16) == [0, 2, 3]
    p = _proto(1, 16, 16, 1)
    recs, words = segref.mask_frame(boxes, [[1]] * 6, [1.0] * 6, p, 64, 64, min_conf=0.5, max_per_frame=5)
    assert recs["det"].tolist() == [0, 2, 3, 5, -1] and recs["area"].tolist() == [16] * 4 + [0]
    assert tuple(recs[4]) == (-1, 0, 0, 0, 0, 0) and not words[4].any() and words[0].any()


def test_record_and_options_layout(marsrt, tmp_path):
    assert C.sizeof(marsrt.MaskRec) == marsrt.MASK_DTYPE.itemsize == 24
    assert marsrt.MASK_DTYPE.names == segref.MASK_FIELDS
    S = marsrt.SegOpts
    got = [C.sizeof(marsrt.MaskRec), C.sizeof(S)] + [getattr(S, f).offset for f, _ in S._fields_]
    assert got == [24, 52, 0, 16, 20, 36, 40, 44, 48]
    src = tmp_path / "abi.c"
    src.write_text("""
#include <stddef.h>
#include <stdio.h>
#include "mars_hip.h"
int main(void) {
 printf("%zu %zu %zu %zu %zu %zu %zu %zu %zu %d %d\\n", sizeof(mars_mask_t), sizeof(mars_hip_seg_opts_t), offsetof(mars_hip_seg_opts_t, coef_tensors),
        offsetof(mars_hip_seg_opts_t, proto_tensor), offsetof(mars_hip_seg_opts_t, coef_scales), offsetof(mars_hip_seg_opts_t, proto_scale),
        offsetof(mars_hip_seg_opts_t, logit_min), offsetof(mars_hip_seg_opts_t, min_conf), offsetof(mars_hip_seg_opts_t, max_per_frame),
        MARS_SEG_MAX_PER_FRAME, MARS_SYNTH_HEAD_SEG);
 return 0;
}
""")
    exe = tmp_path / "abi"
    subprocess.check_call(["gcc", "-std=c11", "-Wall", "-Werror", "-I", INC, str(src), "-o", str(exe)])
    assert [int(v) for v in subprocess.check_output([str(exe)]).split()] == got + [64, 2]
    o = marsrt.seg_opts([5, 6, 7], 9, coef_scales=0.5, proto_scale=0.25, logit_min=1.0, min_conf=0.3, max_per_frame=8)
    assert list(o.coef_tensors) == [5, 6, 7, 0] and o.proto_tensor == 9 and list(o.coef_scales) == [0.5] * 4
    assert (o.proto_scale, o.logit_min, o.max_per_frame) == (0.25, 1.0, 8)


def test_unpack_masks(marsrt):
    rng = np.random.default_rng(3)
    for pw in (16, 32, 33, 40):
        bits = rng.integers(0, 2, (2, 3, 5, pw)).astype(bool)
        w = segref.pack(bits)
        assert w.shape == (2, 3, 5, (pw + 31) // 32)
        assert np.array_equal(marsrt.unpack_masks(w, pw), bits)


# sha256 of the files the writer gave before the seg head existed: heads "anchor" and "dfl" keep their files byte for byte
PARENT_FILES = [
    (dict(width_x16=4, input_hw=64, seed=1, head="anchor"), 1946484, "b07fb639f6667ab8435c521281fb1c701fa34010d35a0632af41f8a0affbed6c"),
    (dict(width_x16=4, input_hw=64, seed=1, head="dfl"), 2743040, "81793a34cb83152759da955dd6627eb5cab0270ca3f7e035ca66c082edf4b56a"),
    (dict(width_x16=4, input_hw=160, seed=3, nchw_int8=True, head="dfl"), 2743040, "85c0984f94043aeeb70fc5043873e797ecc7d8b303c32211af4bbf101716c748"),
    (dict(width_x16=4, input_hw=160, seed=3, nchw_int8=True, head="anchor"), 1946484, "923dd97f67a877d689df680bd665f8a2594c6a3e371868a7bc3642f2369ec22a"),
    (dict(width_x16=8, input_hw=96, seed=7, vary_scales=True, head="dfl"), 9251456, "d923d7b827cf061ed2ce4de032ccbf3d71bc517970dba49b3507e36b155ee448"),
    (dict(width_x16=4, input_hw=64, seed=2, float32=True, head="anchor"), 7532148, "aa822606179bdec9911427a757ef5b780dc88ed311263900b21774c5e752100b"),
]


@pytest.mark.parametrize("kw, size, sha", PARENT_FILES)
def test_other_heads_keep_their_files(marsrt, kw, size, sha):
    d = marsrt.synth_model(**kw)
    assert len(d) == size and hashlib.sha256(d).hexdigest() == sha


@pytest.mark.parametrize("nchw", [False, True])
@pytest.mark.parametrize("hw", [64, 160])
def test_synth_seg_head(marsrt, hw, nchw):
    """the DFL twin plus coefficient and prototype branches.  The .mars header has FOUR output slots (include/mars.h), so the seven tensors
    of the head are: graph outputs 0 - 2 the concats, output 3 the prototypes, and the three coefficient tensors internal, found by name"""
    d = marsrt.synth_model(width_x16=4, input_hw=hw, nchw_int8=nchw, seed=1, head="seg")
    hdr, tensors, layers = marsfile.parse(d)
    coefs, proto = marsrt.seg_twin_tensors(d)
    assert len(hdr["outputs"]) == 4 and hdr["outputs"][3] == proto and len(set(coefs)) == 3

    def chw(t):
        s = tensors[t]["shape"]
        return (s[1], s[2], s[3]) if nchw else (s[3], s[1], s[2])
    heads, nc, reg_max = marsrt.find_yolo_dfl_heads(d)
    assert (nc, reg_max) == (80, 16) and [s for _, _, s in heads] == [8, 16, 32]
    for k, (b, c, s) in enumerate(heads):
        g = hw // s
        assert chw(hdr["outputs"][k]) == (144, g, g) and chw(b) == (64, g, g) and chw(c) == (80, g, g)
        assert chw(coefs[k]) == (32, g, g) and tensors[coefs[k]]["dtype"] == marsfile.I8
        writers = [l for l in layers if coefs[k] in l["outs"]]
        assert len(writers) == 1 and writers[0]["type"] == marsfile.CONV2D
    assert chw(proto) == (32, hw // 4, hw // 4) and tensors[proto]["dtype"] == marsfile.I8
    assert any(l["type"] == marsfile.UPSAMPLE and tensors[l["outs"][0]]["shape"][2] == hw // 4 for l in layers)
    # the trunk and the DFL branches are the dfl twin's: the seg file only adds tensors and layers behind them
    hd, td, ld = marsfile.parse(marsrt.synth_model(width_x16=4, input_hw=hw, nchw_int8=nchw, seed=1, head="dfl"))
    assert [t["shape"] for t in tensors[:len(td)]] == [t["shape"] for t in td] and hdr["outputs"][:3] == hd["outputs"]
    assert [(l["type"], l["ins"], l["outs"]) for l in layers[:len(ld)]] == [(l["type"], l["ins"], l["outs"]) for l in ld]
    for bad in (dict(float32=True), dict(tiny=True)):
        with pytest.raises(ValueError):
            marsrt.synth_model(width_x16=4, input_hw=64, head="seg", **bad)
    assert marsrt.describe_plan(d)  # the loader and the planner take it
