"""The bottleneck's m.cv1 evaluated inside the launch that already runs C3's cv1 + cv2 (fuse_split_chain, conv_i8_patch<CHAIN>): the chained 1x1
reads one side of the pair from registers, its launch and its read of that side go.  Single sites and whole twins, bit for bit against the CPU
oracle and against the same file loaded with the pass switched off (MARS_HIP_NO_CHAIN) and with the fused pair switched off (MARS_HIP_NO_SPLIT),
at every tile height and ring depth of the patch-staged kernel.  Every convolution has its own three scales, weights and bias, so the tables and
combined scales of cv1, cv2 and m.cv1 all differ: swapped sides or tables cannot pass."""
import numpy as np
import pytest

import marsfile
from conftest import lcg_frame
from test_gpu_graph import run_oracle
from test_gpu_split_fusion import _silu_conv

pytestmark = pytest.mark.gpu

FULL = 2  # MARS_HIP_DESCRIBE_FULL


def chain_site(in_c, h, w, stride, odd, seed, side=1, tail="bare", d_out=32, d_add=False, second=None, d_is_output=False):
    """x (in_c channels) -> A: 3 x 3 SiLU convolution (stride 1 / 2) to 64 channels on an h x w map -> cv1, cv2: SiLU 1x1s to 32 channels each
    -> D: a SiLU 1x1 (32 -> d_out) that reads cv1 (side 1) or cv2 (side 2).  Stride 2 reads a 2h x 2w input, or (odd) a (2h - 1) x (2w - 1) one.
      tail bare   the outputs are cv1, cv2 and D
      tail c3     a C3's remainder: D is the bottleneck's first 1x1, the shortcut runs on D's input, cv3 reads concat({m, the other side})
      d_add       an Add of D's input and D's result, which the planner folds into D
      second      a second 1x1 reads D's input too: "same" D's shape (the two become a paired launch), "wide" 64 channels (D stays alone)
      d_is_output tail c3 with D's result a graph output as well"""
    rng = np.random.default_rng(seed)
    G = marsfile.Graph()
    ih, iw = (h, w) if stride == 1 else (2 * h - odd, 2 * w - odd)
    x = G.tensor([1, ih, iw, in_c], scale=0.04)
    t = _silu_conv(G, rng, x, in_c, 64, h, w, 3, 0.06, 1.0 / 250, 0.042, wscale=0.005 if in_c < 64 else 0.003, stride=stride)
    cv1 = _silu_conv(G, rng, t, 64, 32, h, w, 1, 0.05, 1.0 / 256, 0.031, wscale=0.008)
    cv2 = _silu_conv(G, rng, t, 64, 32, h, w, 1, 0.09, 1.0 / 200, 0.07, wscale=0.011)
    src, other = (cv1, cv2) if side == 1 else (cv2, cv1)
    d = _silu_conv(G, rng, src, 32, d_out, h, w, 1, 0.06, 1.0 / 230, 0.045, wscale=0.012)
    outs = [cv1, cv2, d]
    if second:
        outs.append(_silu_conv(G, rng, src, 32, 32 if second == "same" else 64, h, w, 1, 0.07, 1.0 / 220, 0.05, wscale=0.009))
    if d_add:
        m = G.tensor([1, h, w, 32], scale=0.052)
        G.layer(marsfile.ADD, [src, d], [m])
        outs = [cv1, cv2, m]
    if tail == "c3":
        c = 32
        u = _silu_conv(G, rng, d, c, c, h, w, 3, 0.055, 1.0 / 240, 0.038, wscale=0.003)
        m = G.tensor([1, h, w, c], scale=0.052)
        G.layer(marsfile.ADD, [src, u], [m])
        cat = G.tensor([1, h, w, 2 * c], scale=0.05)
        G.concat([m, other], cat)
        outs = [_silu_conv(G, rng, cat, 2 * c, 2 * c, h, w, 1, 0.07, 1.0 / 256, 0.047)] + ([d] if d_is_output else [])
    return G.serialise([x], outs)


def _run(gpu, d, xs):
    m = gpu.Model(d, batch=len(xs))
    for f, x in enumerate(xs):
        m.input_view(0)[f] = x
    m.run()
    outs = [m.output_view(i).copy() for i in range(m.header.num_outputs)]
    m.close()
    return outs


def _chains(plan):
    """the sides of every chain in a full plan"""
    return [int(l.split(" split_chain ")[1].split()[0]) for l in plan if l.startswith("op ") and " split_next 1 " in l]


def _frames(d, B, seed):
    hdr, tensors, _ = marsfile.parse(d)
    nb = marsfile.tensor_nbytes(tensors[hdr["inputs"][0]])
    return hdr, [lcg_frame(0xC4A1700 + 16 * seed + f, nb) for f in range(B)]


def _check(gpu, orc, monkeypatch, d, want_sides, B=3, seed=0):
    """want_sides: the chained side of every fused pair of the plan, 0 = a pair without a chain"""
    hdr, xs = _frames(d, B, seed)
    for k in ("MARS_HIP_NO_CHAIN", "MARS_HIP_NO_SPLIT"):
        monkeypatch.delenv(k, raising=False)
    assert _chains(gpu.describe_plan(d, FULL)) == want_sides, [l for l in gpu.describe_plan(d) if l.startswith("op ")]
    fused = _run(gpu, d, xs)
    monkeypatch.setenv("MARS_HIP_NO_CHAIN", "1")
    assert _chains(gpu.describe_plan(d, FULL)) == [0] * len(want_sides)
    nochain = _run(gpu, d, xs)
    monkeypatch.delenv("MARS_HIP_NO_CHAIN")
    monkeypatch.setenv("MARS_HIP_NO_SPLIT", "1")
    assert _chains(gpu.describe_plan(d, FULL)) == []
    plain = _run(gpu, d, xs)
    monkeypatch.delenv("MARS_HIP_NO_SPLIT")
    for f in range(B):
        g, rc = run_oracle(orc, d, xs[f])
        assert rc == 0
        for oi, ti in enumerate(hdr["outputs"]):
            want = g.tensor(ti)
            assert len(np.unique(want)) > 16
            assert np.array_equal(fused[oi][f], want), (f, oi, int((fused[oi][f] != want).sum()))
            assert np.array_equal(nochain[oi][f], want), (f, oi)
            assert np.array_equal(plain[oi][f], want), (f, oi)


# maps: one full tile; ragged last row and column (fill 0.97 and 0.92 of the 16-row tiles); all inside the kernel's 85 % fill rule.
# stride 2 from an even (2h) and an odd (2h - 1) input size
@pytest.mark.parametrize("side", [1, 2])
@pytest.mark.parametrize("h,w", [(16, 16), (31, 32), (30, 47)])
@pytest.mark.parametrize("stride,odd", [(1, 0), (2, 0), (2, 1)])
@pytest.mark.parametrize("in_c", [16, 32, 64])
def test_chain_site(gpu, orc, monkeypatch, in_c, stride, odd, h, w, side):
    """bare: cv1, cv2 and the chained 1x1 are graph outputs; batch 3, so a workgroup's tiles cross frame boundaries in the ring"""
    d = chain_site(in_c, h, w, stride, odd, seed=in_c + h + w + 7 * stride + odd + 100 * side, side=side)
    _check(gpu, orc, monkeypatch, d, [side], seed=in_c + h + stride + side)


@pytest.mark.parametrize("side", [1, 2])
@pytest.mark.parametrize("stride", [1, 2])
def test_chain_site_in_a_c3(gpu, orc, monkeypatch, stride, side):
    """the C3's remainder behind it, whose 3x3 takes cv3 (fuse_post): the three fusions in one plan"""
    d = chain_site(32, 31, 32, stride, 0, seed=100 + stride + 10 * side, side=side, tail="c3")
    monkeypatch.delenv("MARS_HIP_NO_POST", raising=False)
    assert sum(" post_next" in l for l in gpu.describe_plan(d)) == 1
    _check(gpu, orc, monkeypatch, d, [side], seed=10 + stride + side)


@pytest.mark.parametrize("ring", [1, 2, 3, 4])
@pytest.mark.parametrize("variant", [10, 9, 11])  # 16 / 8 / 4 tile rows
@pytest.mark.parametrize("in_c", [32, 16])
def test_chain_site_every_tile_height_and_ring(gpu, orc, monkeypatch, in_c, variant, ring):
    """every instantiation of the chained kernel, forced through the launch knobs, on the (31, 32) stride-2 map; the LDS budget is raised so
    that four patch buffers fit"""
    d = chain_site(in_c, 31, 32, 2, 1, seed=400 + in_c, side=1 + (ring & 1))
    try:
        gpu.set_tuning("variant", variant)
        gpu.set_tuning("patch_ring", ring)
        gpu.set_tuning("patch_lds_kb", 160)
        _check(gpu, orc, monkeypatch, d, [1 + (ring & 1)], seed=variant + ring)
    finally:
        gpu.set_tuning("variant", 0)
        gpu.set_tuning("patch_ring", 0)
        gpu.set_tuning("patch_lds_kb", 80)


def test_declined_to_64_channels(gpu, orc, monkeypatch):
    d = chain_site(32, 31, 32, 2, 0, seed=600, d_out=64)
    _check(gpu, orc, monkeypatch, d, [0], seed=6)


def test_declined_folded_add(gpu, orc, monkeypatch):
    d = chain_site(32, 31, 32, 2, 0, seed=610, d_add=True)
    assert sum(" k1x1 s1 c32->32 " in l and " add=" in l for l in gpu.describe_plan(d)) == 1
    _check(gpu, orc, monkeypatch, d, [0], seed=7)


def test_second_reader_of_the_same_shape_pairs_with_it(gpu, orc, monkeypatch):
    """two 1x1s of one shape over cv1 are a paired launch (pair_convs, which runs first): a member of a pair is not taken"""
    d = chain_site(32, 31, 32, 2, 0, seed=620, second="same")
    assert sum(" pair_next" in l for l in gpu.describe_plan(d)) == 2
    _check(gpu, orc, monkeypatch, d, [0], seed=8)


def test_second_reader_of_another_shape_still_runs(gpu, orc, monkeypatch):
    """a 1x1 to 64 channels reads cv1 too: only the adjacent qualifying op is taken, the other one is a launch of its own and reads cv1 from memory"""
    d = chain_site(32, 31, 32, 2, 0, seed=630, second="wide")
    _check(gpu, orc, monkeypatch, d, [1], seed=9)


def test_chained_output_is_a_graph_output_too(gpu, orc, monkeypatch):
    d = chain_site(32, 31, 32, 2, 0, seed=640, tail="c3", d_is_output=True)
    _check(gpu, orc, monkeypatch, d, [1], seed=10)


# layer 3 (width 8) writes a 16 x 16 map at 64; layer 23 (width 4) 16 x 16 at 128: the smallest inputs that keep the fused pair
@pytest.mark.parametrize("width,hw", [(8, 64), (4, 128)])
def test_whole_twins(gpu, orc, monkeypatch, width, hw):
    """whole twins with per-convolution scales, batch 2: every graph output against the oracle and against both switches"""
    d = gpu.synth_model(width_x16=width, input_hw=hw, seed=170 + hw + width, vary_scales=True)
    plan = [l for l in gpu.describe_plan(d, FULL) if l.startswith("op ")]
    i = [k for k, l in enumerate(plan) if " split_next 1 " in l][0]
    assert int(plan[i].split()[3]) == (3 if width == 8 else 23) and int(plan[i + 3].split()[3]) == (12 if width == 8 else 32)
    hdr, xs = _frames(d, 2, width)
    monkeypatch.delenv("MARS_HIP_NO_CHAIN", raising=False)
    monkeypatch.delenv("MARS_HIP_NO_SPLIT", raising=False)
    assert _chains(gpu.describe_plan(d, FULL)) == [1]
    fused = _run(gpu, d, xs)
    monkeypatch.setenv("MARS_HIP_NO_CHAIN", "1")
    nochain = _run(gpu, d, xs)
    monkeypatch.delenv("MARS_HIP_NO_CHAIN")
    monkeypatch.setenv("MARS_HIP_NO_SPLIT", "1")
    plain = _run(gpu, d, xs)
    monkeypatch.delenv("MARS_HIP_NO_SPLIT")
    for f in range(2):
        g, rc = run_oracle(orc, d, xs[f])
        assert rc == 0
        for oi, ti in enumerate(hdr["outputs"]):
            want = g.tensor(ti)
            assert np.array_equal(fused[oi][f], want), (f, oi, int((fused[oi][f] != want).sum()))
            assert np.array_equal(nochain[oi][f], want), (f, oi)
            assert np.array_equal(plain[oi][f], want), (f, oi)


def test_batch_change_on_one_instance(gpu, orc, monkeypatch):
    """1 -> 3 -> 1 frames on one model: alloc_batch re-checks the chained output's extent and plans again per batch"""
    monkeypatch.delenv("MARS_HIP_NO_CHAIN", raising=False)
    monkeypatch.delenv("MARS_HIP_NO_SPLIT", raising=False)
    d = chain_site(32, 31, 32, 2, 1, seed=900, tail="c3", d_is_output=True)
    assert _chains(gpu.describe_plan(d, FULL)) == [1]
    hdr, xs = _frames(d, 3, 90)
    want = []
    for x in xs:
        g, rc = run_oracle(orc, d, x)
        assert rc == 0
        want.append([g.tensor(ti) for ti in hdr["outputs"]])
    assert all(len(np.unique(w)) > 16 for w in want[0])
    m = gpu.Model(d, batch=1)
    for B in (1, 3, 1):
        m.set_batch(B)
        for f in range(B):
            m.input_view(0)[f] = xs[f]
        m.run()
        for f in range(B):
            for oi in range(len(hdr["outputs"])):
                assert np.array_equal(m.output_view(oi)[f], want[f][oi]), (B, f, oi)
    m.close()
