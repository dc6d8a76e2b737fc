"""mars_yolo_find_heads: the raw anchor-based YOLOv5 Detect heads of a .mars file, found on the host (no GPU needed)."""
import os

import numpy as np
import pytest

import marsfile

MODELS = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "models")


def _file(name):
    with open(os.path.join(MODELS, name), "rb") as fh:
        return fh.read()


def test_shipped_yolov5n_int8(marsrt):
    """the three 255-channel Detect convolutions behind the shipped file's no-op tail (tensors 313 / 335 / 357)"""
    assert marsrt.find_yolo_heads(_file("yolov5n_int8.mars")) == [(313, 8, 80), (335, 16, 80), (357, 32, 80)]


@pytest.mark.parametrize("nchw", [False, True])
@pytest.mark.parametrize("hw", [320, 640])
@pytest.mark.parametrize("width", [4, 8])
def test_twins(marsrt, width, hw, nchw):
    """the synthetic twins expose their heads as the graph outputs"""
    d = marsrt.synth_model(width_x16=width, input_hw=hw, nchw_int8=nchw, seed=1)
    hdr, _, _ = marsfile.parse(d)
    assert marsrt.find_yolo_heads(d) == [(t, s, 80) for t, s in zip(hdr["outputs"], (8, 16, 32))]


@pytest.mark.parametrize("name", ["yolov5nu.mars", "tiny_160_int8.mars"])
def test_files_without_anchor_heads(marsrt, name):
    """yolov5nu ends in the anchor-free DFL head (64 box + 80 class channels, concatenated): out of scope, nothing found"""
    d = _file(name)
    assert marsrt.find_yolo_heads(d) == []
    assert marsrt.lib().mars_yolo_find_heads(d, len(d), None, None, None, 0) == 0


def _head_graph(nc):
    """16 x 16 x 16 input -> 3x3 stride-2 conv (32 ch) -> 1x1 conv with 3 * (5 + nc) channels read only by a RESHAPE; beside it a
    1x1 conv of the same width read by a SIGMOID (a real layer) and a 3x3 stride-2 conv to 4 x 4 that is a graph output"""
    rng = np.random.default_rng(nc)
    C = 3 * (5 + nc)
    G = marsfile.Graph()
    x = G.tensor([1, 16, 16, 16], scale=0.05)
    t1 = G.tensor([1, 8, 8, 32], scale=0.05)
    G.conv(x, t1, G.tensor([32, 3, 3, 16], scale=0.01, data=rng.integers(-127, 128, (32, 3, 3, 16), dtype=np.int8)), k=(3, 3), s=(2, 2))
    head = G.tensor([1, 8, 8, C], scale=0.1)
    G.conv(t1, head, G.tensor([C, 1, 1, 32], scale=0.01, data=rng.integers(-127, 128, (C, 1, 1, 32), dtype=np.int8)), k=(1, 1))
    G.layer(marsfile.RESHAPE, [head], [G.tensor([0, 0, 0, 0])])
    decoy, sig = G.tensor([1, 8, 8, C], scale=0.1), G.tensor([1, 8, 8, C], scale=0.01)
    G.conv(t1, decoy, G.tensor([C, 1, 1, 32], scale=0.01, data=rng.integers(-127, 128, (C, 1, 1, 32), dtype=np.int8)), k=(1, 1))
    G.layer(marsfile.SIGMOID, [decoy], [sig])
    out = G.tensor([1, 4, 4, C], scale=0.1)
    G.conv(t1, out, G.tensor([C, 3, 3, 32], scale=0.01, data=rng.integers(-127, 128, (C, 3, 3, 32), dtype=np.int8)), k=(3, 3), s=(2, 2))
    return G.serialise([x], [out, sig]), head, out


@pytest.mark.parametrize("nc", [1, 3, 80])
def test_hand_built_graph(marsrt, nc):
    """a 3 * (5 + 3) = 24-channel head (and nc 1 / 80): found with its stride and class count, sorted by stride; a conv that a real
    layer reads is not a head, a graph output is"""
    d, head, out = _head_graph(nc)
    assert marsrt.find_yolo_heads(d) == [(head, 2, nc), (out, 4, nc)]


def test_not_a_head(marsrt):
    """channel counts that are no 3 * (5 + nc) with nc >= 1, and grids that do not divide the input evenly, are no heads"""
    for C, hw, pad in ((15, 8, marsfile.PAD_SAME), (25, 8, marsfile.PAD_SAME), (24, 7, marsfile.PAD_VALID)):
        G = marsfile.Graph()
        x = G.tensor([1, 16, 16, 16], scale=0.05)
        o = G.tensor([1, hw, hw, C], scale=0.1)
        G.conv(x, o, G.tensor([C, 3, 3, 16], scale=0.01, data=np.ones((C, 3, 3, 16), np.int8)), k=(3, 3), s=(2, 2), pad=pad)
        assert marsrt.find_yolo_heads(G.serialise([x], [o])) == [], (C, hw)


def test_rejected_file(marsrt):
    """a file the loader rejects answers -1 (find_yolo_heads: ValueError)"""
    d = _file("yolov5n_int8.mars")[:1000]
    assert marsrt.lib().mars_yolo_find_heads(d, len(d), None, None, None, 0) == -1
    with pytest.raises(ValueError):
        marsrt.find_yolo_heads(d)
