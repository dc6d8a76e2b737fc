"""mars_yolo_find_dfl_heads: the anchor-free DFL heads (box + class convolution pairs) of a .mars file, found on the host, and the
synthetic twin that ends in such heads (mars_synth_model_head).  No GPU needed."""
import hashlib
import os

import numpy as np
import pytest

import marsfile
from conftest import lcg_frame

MODELS = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "models")


def _file(name):
    with open(os.path.join(MODELS, name), "rb") as fh:
        return fh.read()


def test_shipped_yolov5nu(marsrt):
    """the six convolutions in front of the three 2-input CONCATs of the shipped file (layers 210 / 225 / 240); the anchor discovery
    still finds nothing there"""
    d = _file("yolov5nu.mars")
    assert marsrt.find_yolo_dfl_heads(d) == ([(323, 336, 8), (350, 363, 16), (377, 390, 32)], 80, 16)
    assert marsrt.find_yolo_heads(d) == []
    nc, rm = (np.zeros(4, np.int32) for _ in range(2))
    P = marsrt.C.POINTER(marsrt.C.c_int)
    assert marsrt.lib().mars_yolo_find_dfl_heads(d, len(d), None, None, None, nc.ctypes.data_as(P), rm.ctypes.data_as(P), 4) == 3
    assert list(nc[:3]) == [80] * 3 and list(rm[:3]) == [16] * 3
    assert marsrt.lib().mars_yolo_find_dfl_heads(d, len(d), None, None, None, None, None, 0) == 3


@pytest.mark.parametrize("name", ["yolov5n_int8.mars", "tiny_160_int8.mars"])
def test_files_without_dfl_heads(marsrt, name):
    d = _file(name)
    assert marsrt.find_yolo_dfl_heads(d) == ([], 0, 0)
    assert marsrt.lib().mars_yolo_find_dfl_heads(d, len(d), None, None, None, None, None, 0) == 0


@pytest.mark.parametrize("nchw", [False, True])
@pytest.mark.parametrize("hw", [320, 640])
def test_anchor_twins_have_none(marsrt, hw, nchw):
    assert marsrt.find_yolo_dfl_heads(marsrt.synth_model(width_x16=4, input_hw=hw, nchw_int8=nchw, seed=1)) == ([], 0, 0)


def test_rejected_file(marsrt):
    d = _file("yolov5nu.mars")[:1000]
    assert marsrt.lib().mars_yolo_find_dfl_heads(d, len(d), None, None, None, None, None, 0) == -1
    with pytest.raises(ValueError):
        marsrt.find_yolo_dfl_heads(d)


@pytest.mark.parametrize("nchw", [False, True])
@pytest.mark.parametrize("hw", [320, 640])
def test_dfl_twins(marsrt, hw, nchw):
    """the dfl twins end in three 144-channel concats, the graph outputs, of a 64-channel box and an 80-channel class convolution; the
    anchor discovery finds nothing in them"""
    d = marsrt.synth_model(width_x16=4, input_hw=hw, nchw_int8=nchw, seed=1, head="dfl")
    hdr, tensors, layers = marsfile.parse(d)
    heads, nc, rm = marsrt.find_yolo_dfl_heads(d)
    assert (nc, rm) == (80, 16) and [s for _, _, s in heads] == [8, 16, 32]
    cats = [l for l in layers if l["type"] == marsfile.CONCAT and l["outs"][0] in hdr["outputs"]]
    assert [tuple(l["ins"]) for l in cats] == [(b, c) for b, c, _ in heads] and len(hdr["outputs"]) == 3
    for (b, c, s), o in zip(heads, hdr["outputs"]):
        n = hw // s
        want = ([1, 64, n, n], [1, 80, n, n], [1, 144, n, n]) if nchw else ([1, n, n, 64], [1, n, n, 80], [1, n, n, 144])
        assert tuple(list(tensors[t]["shape"]) for t in (b, c, o)) == want
    assert marsrt.find_yolo_heads(d) == []


def test_dfl_twin_rejects(marsrt):
    for kw in (dict(float32=True), dict(tiny=True, input_hw=160)):
        with pytest.raises(ValueError):
            marsrt.synth_model(head="dfl", **kw)


@pytest.mark.parametrize("nchw", [False, True])
@pytest.mark.parametrize("hw", [320, 640])
def test_dfl_twin_candidates_on_oracle(marsrt, orc, hw, nchw):
    """on the CPU oracle, LCG frames: at confidence 0.25 -- sigmoid(q * class scale) >= 0.25 -- a frame of the width 4 / seed 1 twin has
    some candidate cells, far fewer than the 1000 the tail keeps; and the box logits use the int8 range"""
    d = marsrt.synth_model(width_x16=4, input_hw=hw, nchw_int8=nchw, seed=1, head="dfl")
    hdr, tensors, _ = marsfile.parse(d)
    nb = marsfile.tensor_nbytes(tensors[hdr["inputs"][0]])
    for fr in range(2):
        g = orc.Graph(d)
        g.set_input(0, lcg_frame(0x5EED0000 + fr, nb).tobytes())
        assert g.run() == 0
        cands = 0
        for b, c, s in marsrt.find_yolo_dfl_heads(d)[0]:
            n = hw // s
            cl = g.tensor(c).view(np.int8)
            cl = cl.reshape(80, n * n) if nchw else cl.reshape(n * n, 80).T
            logit = cl.max(axis=0).astype(np.float32) * np.float32(tensors[c]["scale"])
            cands += int((1.0 / (1.0 + np.exp(-logit.astype(np.float64))) >= 0.25).sum())
            assert g.tensor(b).view(np.int8).std() > 10
        assert 1 <= cands <= 250, (hw, nchw, fr, cands)  # some, and at most a quarter of the cap


def _pair_graph(ca=64, cb=3, hw_a=8, hw_b=8, n_inputs=2, sigmoid_on_box=False, t1_hw=8, out_is_io=True):
    """2 t1_hw x 2 t1_hw x 16 input -> 3x3 stride-2 conv (32 ch, t1_hw x t1_hw) -> a box conv (ca channels, hw_a x hw_a) and a class conv
    (cb channels, hw_b x hw_b), 1x1 with the stride that gives that grid, concatenated"""
    in_hw = 2 * t1_hw
    rng = np.random.default_rng(ca * 131 + cb)
    G = marsfile.Graph()
    x = G.tensor([1, in_hw, in_hw, 16], scale=0.05)
    t1 = G.tensor([1, t1_hw, t1_hw, 32], scale=0.05)
    G.conv(x, t1, G.tensor([32, 3, 3, 16], scale=0.01, data=rng.integers(-127, 128, (32, 3, 3, 16), dtype=np.int8)), k=(3, 3), s=(2, 2))

    def branch(c, hw):
        o = G.tensor([1, hw, hw, c], scale=0.1)
        s = -(-t1_hw // hw)
        assert -(-t1_hw // s) == hw
        G.conv(t1, o, G.tensor([c, 1, 1, 32], scale=0.01, data=rng.integers(-127, 128, (c, 1, 1, 32), dtype=np.int8)), k=(1, 1), s=(s, s))
        return o
    a, b = branch(ca, hw_a), branch(cb, hw_b)
    ins = [a, b] + [branch(16, hw_a) for _ in range(n_inputs - 2)]
    outs = []
    if sigmoid_on_box:
        sg = G.tensor([1, hw_a, hw_a, ca], scale=0.01)
        G.layer(marsfile.SIGMOID, [a], [sg])
        outs.append(sg)
    cat = G.tensor([1, hw_a, hw_a, ca + cb + 16 * (n_inputs - 2)], scale=0.1)
    G.concat(ins, cat)
    if not out_is_io:
        G.layer(marsfile.RESHAPE, [cat], [G.tensor([0, 0, 0, 0])])
        outs.append(t1)
    else:
        outs.append(cat)
    return G.serialise([x], outs), a, b


def test_hand_built_pair(marsrt):
    """a 64 + 3 channel pair under a concat that is the graph output, and one read only by a RESHAPE; reg_max 8"""
    for io in (True, False):
        d, a, b = _pair_graph(out_is_io=io)
        assert marsrt.find_yolo_dfl_heads(d) == ([(a, b, 2)], 3, 16), io
    d, a, b = _pair_graph(ca=32, cb=1)
    assert marsrt.find_yolo_dfl_heads(d) == ([(a, b, 2)], 1, 8)


@pytest.mark.parametrize("why, kw", [
    ("a concat of three inputs", dict(n_inputs=3)),
    ("box channels no multiple of 4", dict(ca=66)),
    ("reg_max 1", dict(ca=4)),
    ("reg_max 33", dict(ca=132)),
    ("unequal grids", dict(hw_b=4)),
    ("the box convolution is also read by a SIGMOID", dict(sigmoid_on_box=True)),
    ("a grid that does not divide the input", dict(t1_hw=10, hw_a=3, hw_b=3)),
])
def test_not_a_dfl_head(marsrt, why, kw):
    d, _, _ = _pair_graph(**kw)
    assert marsrt.describe_plan(d)  # the loader takes the file
    assert marsrt.find_yolo_dfl_heads(d) == ([], 0, 0), why


# mars_synth_model's files as the tree before mars_synth_model_head wrote them (SHA-256)
OLD_SYNTH = [
    (dict(width_x16=4, input_hw=64, seed=1), "b07fb639f6667ab8435c521281fb1c701fa34010d35a0632af41f8a0affbed6c"),
    (dict(width_x16=4, input_hw=320, nchw_int8=True, seed=3), "c0319f02a85ab34466adbd3d544dc7e16828702528f924b383b491dfa3de3e76"),
    (dict(width_x16=8, input_hw=128, float32=True, seed=2), "c6c308d6b61610e0cf1268e9901cb0311fc1fdea2fb6ae8121e176ccbaa485ce"),
    (dict(tiny=True, input_hw=160, seed=5), "4ae940a95c1e83c2510f9d3522c12bc9d10f0f6800f98a9db6f811ff5c56502c"),
    (dict(width_x16=4, input_hw=96, seed=7, vary_scales=True), "bfcb59bc317cf2c74d20cd2fc7552192e39d892ad8fcd977ebf264bdcd9cee2e"),
    (dict(width_x16=4, depth_x3=2, input_hw=64, seed=1), "a5b186de684ed9a1c135d4ca6c512457cc1fa3bdbff6e111ec3d0bac5d6993b4"),
]


@pytest.mark.parametrize("kw, sha", OLD_SYNTH)
def test_old_synth_files_unchanged(marsrt, kw, sha):
    d = marsrt.synth_model(**kw)
    assert hashlib.sha256(d).hexdigest() == sha
    assert marsrt.synth_model(head="anchor", **kw) == d
