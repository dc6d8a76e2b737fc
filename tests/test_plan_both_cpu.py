"""pair_convs' one-tile form on the CPU (mars_hip_describe_plan, no device): which pairs of 1x1s over one input run as ONE tile of the tile
walker (pair_both, conv_i8_persist<BOTH>), pairs over a never-materialised concat included, which of them take the 1x1 behind one side
(fuse_both_chain), which sides are elided, and the switches.  The results of every such plan are checked bit for bit by
tests/test_gpu_both_pair.py."""
import os
import sys

import pytest

import cases
from test_oracle import model_bytes

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, "..", "thingino-accel_amd"))

FULL = 2  # MARS_HIP_DESCRIBE_FULL


def ops(lines):
    return [l for l in lines if l.startswith("op ")]


def both_sites(lines):
    """(first side's layer, second side's layer, segments of their input) of every one-tile pair; the two ops sit in a row.  A pair over a
    tensor shows ` pair_next pair_both`, one over a never-materialised concat -- which exists in this form only -- ` pair_both` alone"""
    o = ops(lines)
    res = []
    for i, l in enumerate(o):
        s = l.split(" | ")[0] + " "
        if " pair_both " not in s:
            continue
        assert (" pair_next " in s) == (" seg=" not in s) and " k1x1 s1 " in s and "->64 " in s and " lut " in s and " add=" not in s, l
        b = o[i + 1].split(" | ")[0] + " "
        assert " k1x1 s1 " in b and "->64 " in b and " lut " in b and " pair_" not in b and " add=" not in b, o[i + 1]
        assert l.split(" in ")[1].split(" out ")[0] == o[i + 1].split(" in ")[1].split(" out ")[0], (l, o[i + 1])  # one input
        assert l.split(" out ")[1].split()[0] != o[i + 1].split(" out ")[1].split()[0]
        seg = int(s.split(" seg=")[1].split()[0]) if " seg=" in s else 0
        assert (" seg=%d " % seg in b) if seg else " seg=" not in b
        res.append((int(l.split()[3]), int(o[i + 1].split()[3]), seg))
    return res


def chain_sites(lines):
    """(first side's layer, second side's, the chained 1x1's, side, elided) of every one-tile pair that carries a chain; three ops in a row.
    An elided side is no graph output and has no reader but the chained 1x1; its tensor is not in the full plan's list of kept tensors"""
    o = ops(lines)
    outputs = [int(t) for l in lines if l.startswith("outputs") for t in l.split()[1:]]
    res = []
    for i, l in enumerate(o):
        s = l.split(" | ")[0] + " "
        if " both_chain=" not in s:
            continue
        side = int(s.split(" both_chain=")[1].split()[0])
        elided = " both_elide " in s
        assert side in (1, 2) and " pair_both " in s, l
        d = o[i + 2].split(" | ")[0] + " "
        assert " k1x1 s1 c64->64 " in d and " lut " in d and " add=" not in d and " pair_" not in d and " seg=" not in d and " both_" not in d, o[i + 2]
        t_side = o[i + side - 1].split(" out ")[1].split()[0]
        assert d.split(" in ")[1].split(" out ")[0] == t_side, (l, o[i + 2])
        other_readers = [x for k, x in enumerate(o) if k != i + 2 and t_side in x.split(" in ")[1].split(" out ")[0].split()]
        other_readers += [x for x in o if " add=%s " % t_side in x.split(" | ")[0] + " "]
        if elided:
            assert not other_readers and int(t_side) not in outputs, (l, other_readers)
        else:
            assert other_readers or int(t_side) in outputs, l
        res.append((int(l.split()[3]), int(o[i + 1].split()[3]), int(o[i + 2].split()[3]), side, elided))
    return res


@pytest.fixture(autouse=True)
def _switches(monkeypatch):
    for k in ("MARS_HIP_NO_BOTH", "MARS_HIP_NO_BOTH_CHAIN", "MARS_HIP_NO_CHAIN", "MARS_HIP_NO_SPLIT", "MARS_HIP_NO_POST", "MARS_HIP_FUSION"):
        monkeypatch.delenv(k, raising=False)


@pytest.mark.parametrize("hw", [640, 320])
def test_headline_twin_sites(marsrt, hw):
    """the yolov5s twin: the second backbone C3 (128 -> 64 + 64, plain input) and the neck's 80 x 80 C3 (256 -> 64 + 64 over
    concat({upsample, backbone})); the pairs of 128 and 256 channels a side stay side by side, those over a concat two launches"""
    L = marsrt.describe_plan(marsrt.synth_model(width_x16=8, input_hw=hw, seed=1))
    assert both_sites(L) == [(26, 29, 0), (140, 143, 2)]
    # the bottleneck's m.cv1 rides on cv1's side of both; the backbone's cv1 is kept (the shortcut Add reads it), the neck's is elided
    assert chain_sites(L) == [(26, 29, 32, 1, False), (140, 143, 146, 1, True)]
    assert sum(" conv_i8 " in l for l in ops(L)) == 60  # every op stays in the plan
    for l in ops(L):
        if " pair_next" in l and " pair_both" not in l:
            assert " seg=" not in l, l  # no side-by-side pair over a concat


def test_yolov5n_twin_sites(marsrt):
    L = marsrt.describe_plan(marsrt.synth_model(width_x16=4, input_hw=640, seed=1))
    assert both_sites(L) == [(53, 56, 0), (119, 122, 2), (160, 163, 2)]
    assert chain_sites(L) == [(53, 56, 59, 1, False), (119, 122, 125, 1, True), (160, 163, 166, 1, True)]


@pytest.mark.parametrize("name", cases.SHIPPED)
def test_shipped_files(marsrt, monkeypatch, name):
    """the shipped yolov5n files have three C3s with sides of 64 channels over materialised tensors; the two whose concat virtual_concat_q cut
    in row ranges carry the form on both halves.  The other files have none.  The switch takes every one back to a side-by-side pair"""
    d = model_bytes(name)
    want = [(53, 77, 0), (119, 128, 0), (119, 128, 0), (160, 169, 0), (160, 169, 0)] if name in ("yolov5n_int8", "yolov5nu") else []
    on = marsrt.describe_plan(d)
    # a pair cut in row ranges takes no chain; yolov5nu's first such C3 has a bottleneck 1x1 with a half-step table behind cv1 (the shortcut keeps cv1)
    assert both_sites(on) == want and chain_sites(on) == ([(53, 77, 56, 1, False)] if name == "yolov5nu" else [])
    monkeypatch.setenv("MARS_HIP_NO_BOTH", "1")
    off = marsrt.describe_plan(d)
    assert both_sites(off) == [] and off == [l.replace(" both_chain=1", "").replace(" pair_both", "") for l in on]


def _pair_graph(oc, x_scale):
    """cv1, cv2: SiLU 1x1s from 128 to oc channels each over the graph input"""
    import numpy as np

    import marsfile
    from test_gpu_split_fusion import _silu_conv
    rng = np.random.default_rng(oc)
    G = marsfile.Graph()
    x = G.tensor([1, 12, 12, 128], scale=x_scale)
    cv1 = _silu_conv(G, rng, x, 128, oc, 12, 12, 1, 0.05, 1.0 / 256, 0.031, wscale=0.25 / 128)
    cv2 = _silu_conv(G, rng, x, 128, oc, 12, 12, 1, 0.09, 1.0 / 200, 0.07, wscale=0.35 / 128)
    return G.serialise([x], [cv1, cv2])


def test_no_form_where_the_device_query_says_no(marsrt):
    """sides of 32 channels; sides of 64 where one combined scale (1 / 640) cannot have a half-step table; sides of 128 (the 256-row tile is
    off by default): each stays a side-by-side pair.  The same graph with a scale the table serves takes the form"""
    for oc, x_scale in ((32, 0.037), (64, 0.04), (128, 0.037)):
        L = marsrt.describe_plan(_pair_graph(oc, x_scale))
        assert both_sites(L) == [] and sum(" pair_next" in l for l in ops(L)) == 1, (oc, ops(L))
    assert len(both_sites(marsrt.describe_plan(_pair_graph(64, 0.037)))) == 1


@pytest.mark.parametrize("width,hw", [(8, 640), (4, 640), (8, 64)])
def test_switch_restores_the_plan_without_the_form(marsrt, monkeypatch, width, hw):
    """MARS_HIP_NO_BOTH: no flag, no pair over a concat; every other line of the plan stays as it is, in its place"""
    d = marsrt.synth_model(width_x16=width, input_hw=hw, seed=1)
    on, full = marsrt.describe_plan(d), marsrt.describe_plan(d, FULL)
    assert " no_both 0 " in full[-1] and full[-1].startswith("+plan")
    assert " no_both_chain 0 " in full[-1]

    def strip(l):
        return l.replace(" both_elide", "").replace(" both_chain=1", "").replace(" both_chain=2", "")

    # MARS_HIP_NO_BOTH_CHAIN: the chains and elisions go, the one-tile pairs stay
    monkeypatch.setenv("MARS_HIP_NO_BOTH_CHAIN", "1")
    mid, full1 = marsrt.describe_plan(d), marsrt.describe_plan(d, FULL)
    assert " no_both_chain 1 " in full1[-1] and " no_both 0 " in full1[-1]
    assert chain_sites(mid) == [] and both_sites(mid) == both_sites(on) and ops(mid) == [strip(l) for l in ops(on)]
    assert sum(" needed 1 " in l for l in full1) == sum(" needed 1 " in l for l in full) + sum(e for *_, e in chain_sites(on))
    monkeypatch.delenv("MARS_HIP_NO_BOTH_CHAIN")
    monkeypatch.setenv("MARS_HIP_NO_BOTH", "1")
    off, full0 = marsrt.describe_plan(d), marsrt.describe_plan(d, FULL)
    assert " no_both 1 " in full0[-1]
    assert both_sites(off) == [] and chain_sites(off) == [] and len(off) == len(on)
    for a, b in zip(on, off):
        a = strip(a)
        if " pair_both" not in a:
            assert a == b
        elif " seg=" in a:
            assert " pair_next" not in a and b == a.replace(" pair_both", "")  # two launches, as before the form
        else:
            assert b == a.replace(" pair_both", "")  # the side-by-side pair, as before the form
    # fusion level 0 never pairs
    monkeypatch.delenv("MARS_HIP_NO_BOTH")
    monkeypatch.setenv("MARS_HIP_FUSION", "0")
    assert both_sites(marsrt.describe_plan(d)) == []
