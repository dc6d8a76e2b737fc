"""C3's cv3 evaluated inside the k x k convolution that feeds it (fuse_post, conv_i8_patch<POST>): the last bottleneck's 3x3 result u never
goes to HBM.  Single C3 blocks and whole twins, bit for bit against the CPU oracle and against the same file loaded with the pass switched off
(MARS_HIP_NO_POST), at every tile height and ring depth of the patch-staged kernel."""
import numpy as np
import pytest

import marsfile
from conftest import lcg_frame
from test_gpu_graph import run_oracle

pytestmark = pytest.mark.gpu


def _silu_conv(G, rng, x, in_c, out_c, h, w, k, s_conv, s_sig, s_out, wscale=0.004, out=None):
    """conv -> sigmoid -> mul with its own three scales (the plan folds the chain into the conv's LUT epilogue); `out`: the MUL's result tensor"""
    a = G.tensor([1, h, w, out_c], scale=s_conv)
    g = G.tensor([1, h, w, out_c], scale=s_sig)
    o = out if out is not None else G.tensor([1, h, w, out_c], scale=s_out)
    wt = G.tensor([out_c, k, k, in_c], scale=wscale, data=rng.integers(-127, 128, (out_c, k, k, in_c), dtype=np.int8))
    b = G.tensor([out_c], dtype=marsfile.I32, scale=1.0, data=rng.integers(-2000, 2000, out_c, dtype=np.int32))
    G.conv(x, a, wt, b, (k, k), (1, 1))
    G.layer(marsfile.SIGMOID, [a], [g])
    G.layer(marsfile.MUL, [a, g], [o])
    return o


def c3_block(c, n, shortcut, h, w, seed, slice_out=False):
    """x (2c channels) -> cv1, cv2 (-> c each); n bottlenecks (1x1, 3x3, optional Add) on cv1's branch; cv3 over concat({m, cv2}) -> 2c channels;
    a different scale for every convolution.  slice_out: cv3's result is concatenated with cv1's (3c channels: a concat that stays materialised,
    so cv3 writes a channel slice of it) and a 1x1 reads that"""
    rng = np.random.default_rng(seed)
    G = marsfile.Graph()
    x = G.tensor([1, h, w, 2 * c], scale=0.04)
    cv1 = _silu_conv(G, rng, x, 2 * c, c, h, w, 1, 0.05, 1.0 / 256, 0.031)
    cv2 = _silu_conv(G, rng, x, 2 * c, c, h, w, 1, 0.09, 1.0 / 200, 0.07)
    m = cv1
    for i in range(n):
        t = _silu_conv(G, rng, m, c, c, h, w, 1, 0.06 + 0.01 * i, 1.0 / 256, 0.045 - 0.004 * i, wscale=0.01)
        u = _silu_conv(G, rng, t, c, c, h, w, 3, 0.055 + 0.007 * i, 1.0 / 240, 0.038 + 0.003 * i, wscale=0.003)
        if shortcut:
            s = G.tensor([1, h, w, c], scale=0.052 + 0.005 * i)
            G.layer(marsfile.ADD, [m, u], [s])
            u = s
        m = u
    cat = G.tensor([1, h, w, 2 * c], scale=0.05)
    G.concat([m, cv2], cat)
    cv3 = _silu_conv(G, rng, cat, 2 * c, 2 * c, h, w, 1, 0.07, 1.0 / 256, 0.047)
    outs = [cv3, cv1]
    if slice_out:
        wide = G.tensor([1, h, w, 3 * c], scale=0.047)
        G.concat([cv3, cv1], wide)
        outs = [_silu_conv(G, rng, wide, 3 * c, c, h, w, 1, 0.06, 1.0 / 256, 0.05), cv2]
    return G.serialise([x], outs)


def _run(gpu, d, xs):
    m = gpu.Model(d, batch=len(xs))
    for f, x in enumerate(xs):
        m.input_view(0)[f] = x
    m.run()
    n_out = m.header.num_outputs
    outs = [m.output_view(i).copy() for i in range(n_out)]
    m.close()
    return outs


def _check_block(gpu, orc, monkeypatch, d, want_sites, B=3, seed=0):
    hdr, tensors, _ = marsfile.parse(d)
    nb = marsfile.tensor_nbytes(tensors[hdr["inputs"][0]])
    xs = [lcg_frame(0x9057000 + 16 * seed + f, nb) for f in range(B)]
    monkeypatch.delenv("MARS_HIP_NO_POST", raising=False)
    plan = gpu.describe_plan(d)
    assert sum(" post_next" in l for l in plan) == want_sites, [l for l in plan if l.startswith("op ")]
    fused = _run(gpu, d, xs)
    monkeypatch.setenv("MARS_HIP_NO_POST", "1")
    assert sum(" post_next" in l for l in gpu.describe_plan(d)) == 0
    plain = _run(gpu, d, xs)
    monkeypatch.delenv("MARS_HIP_NO_POST")
    for f in range(B):
        g, rc = run_oracle(orc, d, xs[f])
        assert rc == 0
        for oi, ti in enumerate(hdr["outputs"]):
            want = g.tensor(ti)
            assert len(np.unique(want)) > 16
            assert np.array_equal(fused[oi][f], want), (f, oi, int((fused[oi][f] != want).sum()))
            assert np.array_equal(plain[oi][f], want), (f, oi)


# maps: one full tile; ragged last row and column (fill 0.97 and 0.92 of the 16-row tiles); 20 x 20 is below the kernel's 85 % fill rule
@pytest.mark.parametrize("h,w", [(16, 16), (31, 32), (30, 47)])
@pytest.mark.parametrize("shortcut", [False, True])
@pytest.mark.parametrize("c", [32, 64])
def test_c3_block_fused(gpu, orc, monkeypatch, c, shortcut, h, w):
    """one bottleneck: its 3x3 (with the folded Add where there is a shortcut) takes cv3; batch 3, so tiles cross frame boundaries in the ring"""
    d = c3_block(c, 1, shortcut, h, w, seed=c + h + w + shortcut)
    _check_block(gpu, orc, monkeypatch, d, 1, seed=c + h)


@pytest.mark.parametrize("shortcut", [False, True])
@pytest.mark.parametrize("c", [32, 64])
def test_c3_block_two_bottlenecks(gpu, orc, monkeypatch, c, shortcut):
    """n = 2: only the last 3x3 fuses (with a shortcut the first one's output has two readers, without one it feeds a 1x1, not the concat)"""
    d = c3_block(c, 2, shortcut, 31, 32, seed=200 + c + shortcut)
    _check_block(gpu, orc, monkeypatch, d, 1, seed=2 * c)
    plan = [l for l in gpu.describe_plan(d) if l.startswith("op ")]
    k3 = [l for l in plan if " k3x3 " in l]
    assert len(k3) == 2 and " post_next" not in k3[0] and " post_next" in k3[1]


@pytest.mark.parametrize("c", [32, 64])
def test_c3_block_below_the_fill_rule_is_not_fused(gpu, orc, monkeypatch, c):
    d = c3_block(c, 1, True, 20, 20, seed=300 + c)
    _check_block(gpu, orc, monkeypatch, d, 0, seed=3 * c)


@pytest.mark.parametrize("ring", [1, 2])
@pytest.mark.parametrize("variant", [10, 9, 11])  # 16 / 8 / 4 tile rows
@pytest.mark.parametrize("c,shortcut", [(32, True), (32, False), (64, True), (64, False)])
def test_c3_block_every_tile_height_and_ring(gpu, orc, monkeypatch, c, shortcut, variant, ring):
    """every instantiation of the fused kernel, forced through the launch knobs; the LDS budget is raised so that the 64-channel block fits 16-row
    tiles with two patch buffers too"""
    d = c3_block(c, 1, shortcut, 30, 47, seed=400 + c + shortcut)
    try:
        gpu.set_tuning("variant", variant)
        gpu.set_tuning("patch_ring", ring)
        gpu.set_tuning("patch_lds_kb", 120)
        _check_block(gpu, orc, monkeypatch, d, 1, seed=variant + ring)
    finally:
        gpu.set_tuning("variant", 0)
        gpu.set_tuning("patch_ring", 0)
        gpu.set_tuning("patch_lds_kb", 80)


@pytest.mark.parametrize("c", [32, 64])
def test_c3_block_small_batch_policy(gpu, orc, monkeypatch, c):
    """few workgroups: the small-batch policy runs the fused launch on 4-row tiles (a flagged op has no other launch form)"""
    d = c3_block(c, 1, True, 31, 32, seed=500 + c)
    try:
        gpu.set_tuning("few_wgs", 1 << 20)
        _check_block(gpu, orc, monkeypatch, d, 1, B=1, seed=5 * c)
    finally:
        gpu.set_tuning("few_wgs", 256)


def test_cv3_writes_a_channel_slice(gpu, orc, monkeypatch):
    """cv3's result goes into a concat of 96 channels that stays materialised: the fused launch stores into that tensor's channel slice"""
    d = c3_block(32, 1, True, 31, 32, seed=600, slice_out=True)
    monkeypatch.delenv("MARS_HIP_NO_POST", raising=False)
    plan = [l for l in gpu.describe_plan(d) if l.startswith("op ")]
    i = [k for k, l in enumerate(plan) if " post_next" in l]
    assert len(i) == 1 and " pix_stride=96" in plan[i[0] + 1], plan
    _check_block(gpu, orc, monkeypatch, d, 1, seed=6)


@pytest.mark.parametrize("width,hw,B", [(8, 128, 3), (4, 256, 2)])
def test_whole_twins(gpu, orc, monkeypatch, width, hw, B):
    """whole twins with per-convolution scales: fusion level 1 against the oracle and against the pass switched off, level 2 against level 1"""
    monkeypatch.delenv("MARS_HIP_NO_POST", raising=False)
    d = gpu.synth_model(width_x16=width, input_hw=hw, seed=90 + hw, vary_scales=True)
    hdr, tensors, _ = marsfile.parse(d)
    nb = marsfile.tensor_nbytes(tensors[hdr["inputs"][0]])
    xs = [lcg_frame(0x9057F00 + f, nb) for f in range(B)]
    assert sum(" post_next" in l for l in gpu.describe_plan(d)) >= 2

    def run(level):
        m = gpu.Model(d, batch=B, fusion=level)
        for f in range(B):
            m.input_view(0)[f] = xs[f]
        m.run()
        o = [m.output_view(i).copy() for i in range(3)]
        m.close()
        return o

    l1, l2 = run(1), run(2)
    monkeypatch.setenv("MARS_HIP_NO_POST", "1")
    plain = run(1)
    monkeypatch.delenv("MARS_HIP_NO_POST")
    for i in range(3):
        assert np.array_equal(l1[i], plain[i]), i
        assert np.array_equal(l2[i], l1[i]), i
    g, rc = run_oracle(orc, d, xs[B - 1])
    assert rc == 0
    for oi, ti in enumerate(hdr["outputs"]):
        assert np.array_equal(l1[oi][B - 1], g.tensor(ti)), oi
