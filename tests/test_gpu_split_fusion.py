"""C3's cv1 + cv2 evaluated inside the k x k convolution that feeds them (fuse_split, conv_i8_patch<SPLIT>): the k x k result never goes to HBM
and the pair launch goes.  Single sites and whole twins, bit for bit against the CPU oracle and against the same file loaded with the pass
switched off (MARS_HIP_NO_SPLIT), at every tile height and ring depth of the patch-staged kernel.  Every convolution has its own three scales,
weights and bias, so the two sides' tables and combined scales differ: a swap of the sides cannot pass."""
import numpy as np
import pytest

import marsfile
from conftest import lcg_frame
from test_gpu_graph import run_oracle

pytestmark = pytest.mark.gpu


def _silu_conv(G, rng, x, in_c, out_c, h, w, k, s_conv, s_sig, s_out, wscale=0.004, stride=1, out=None):
    """conv -> sigmoid -> mul with its own three scales (the plan folds the chain into the conv's LUT epilogue); h, w: the OUTPUT map"""
    a = G.tensor([1, h, w, out_c], scale=s_conv)
    g = G.tensor([1, h, w, out_c], scale=s_sig)
    o = out if out is not None else G.tensor([1, h, w, out_c], scale=s_out)
    wt = G.tensor([out_c, k, k, in_c], scale=wscale, data=rng.integers(-127, 128, (out_c, k, k, in_c), dtype=np.int8))
    b = G.tensor([out_c], dtype=marsfile.I32, scale=1.0, data=rng.integers(-2000, 2000, out_c, dtype=np.int32))
    G.conv(x, a, wt, b, (k, k), (stride, stride))
    G.layer(marsfile.SIGMOID, [a], [g])
    G.layer(marsfile.MUL, [a, g], [o])
    return o


def split_site(in_c, h, w, stride, odd, seed, k=3, tail="outputs"):
    """x (in_c channels) -> A: k x k SiLU convolution (stride 1 / 2) to 64 channels on an h x w map -> cv1, cv2: SiLU 1x1s to 32 channels each.
    Stride 2 reads a 2h x 2w input, or (odd) a (2h - 1) x (2w - 1) one.  tail:
      outputs   both sides are graph outputs
      c3        a C3's remainder: one bottleneck with a shortcut on cv1's branch, cv3 over concat({m, cv2})
      third     a third 1x1 reads A's result too
      t_out     A's result is a graph output as well"""
    rng = np.random.default_rng(seed)
    G = marsfile.Graph()
    ih, iw = (h, w) if stride == 1 else (2 * h - odd, 2 * w - odd)
    x = G.tensor([1, ih, iw, in_c], scale=0.04)
    t = _silu_conv(G, rng, x, in_c, 64, h, w, k, 0.06, 1.0 / 250, 0.042, wscale=0.005 if in_c < 64 else 0.003, stride=stride)
    cv1 = _silu_conv(G, rng, t, 64, 32, h, w, 1, 0.05, 1.0 / 256, 0.031, wscale=0.008)
    cv2 = _silu_conv(G, rng, t, 64, 32, h, w, 1, 0.09, 1.0 / 200, 0.07, wscale=0.011)
    outs = [cv1, cv2]
    if tail == "c3":
        c = 32
        b1 = _silu_conv(G, rng, cv1, c, c, h, w, 1, 0.06, 1.0 / 256, 0.045, wscale=0.01)
        u = _silu_conv(G, rng, b1, c, c, h, w, 3, 0.055, 1.0 / 240, 0.038, wscale=0.003)
        m = G.tensor([1, h, w, c], scale=0.052)
        G.layer(marsfile.ADD, [cv1, u], [m])
        cat = G.tensor([1, h, w, 2 * c], scale=0.05)
        G.concat([m, cv2], cat)
        outs = [_silu_conv(G, rng, cat, 2 * c, 2 * c, h, w, 1, 0.07, 1.0 / 256, 0.047)]
    elif tail == "third":
        outs.append(_silu_conv(G, rng, t, 64, 32, h, w, 1, 0.07, 1.0 / 220, 0.05, wscale=0.009))
    elif tail == "t_out":
        outs.append(t)
    return G.serialise([x], outs)


def slices_site(h, w, seed):
    """cv1 and cv2 feed a concat that a 3 x 3 convolution reads: it stays materialised, so the 1x1s write channel slices of it"""
    rng = np.random.default_rng(seed)
    G = marsfile.Graph()
    x = G.tensor([1, h, w, 32], scale=0.04)
    t = _silu_conv(G, rng, x, 32, 64, h, w, 3, 0.06, 1.0 / 250, 0.042, wscale=0.005)
    cv1 = _silu_conv(G, rng, t, 64, 32, h, w, 1, 0.05, 1.0 / 256, 0.05, wscale=0.008)
    cv2 = _silu_conv(G, rng, t, 64, 32, h, w, 1, 0.09, 1.0 / 200, 0.05, wscale=0.011)
    cat = G.tensor([1, h, w, 64], scale=0.05)
    G.concat([cv1, cv2], cat)
    o = _silu_conv(G, rng, cat, 64, 32, h, w, 3, 0.07, 1.0 / 256, 0.047, wscale=0.003)
    return G.serialise([x], [o])


def _run(gpu, d, xs, extra=()):
    m = gpu.Model(d, batch=len(xs))
    for f, x in enumerate(xs):
        m.input_view(0)[f] = x
    m.run()
    outs = [m.output_view(i).copy() for i in range(m.header.num_outputs)]
    more = [[m.read_tensor(ti, frame=f) for f in range(len(xs))] for ti in extra]
    m.close()
    return outs, more


def _flags(plan):
    return sum(" split_next" in l for l in plan)


def _check(gpu, orc, monkeypatch, d, want_sites, B=3, seed=0):
    hdr, tensors, _ = marsfile.parse(d)
    nb = marsfile.tensor_nbytes(tensors[hdr["inputs"][0]])
    xs = [lcg_frame(0x5711700 + 16 * seed + f, nb) for f in range(B)]
    monkeypatch.delenv("MARS_HIP_NO_SPLIT", raising=False)
    plan = gpu.describe_plan(d)
    assert _flags(plan) == want_sites, [l for l in plan if l.startswith("op ")]
    fused, _ = _run(gpu, d, xs)
    monkeypatch.setenv("MARS_HIP_NO_SPLIT", "1")
    assert _flags(gpu.describe_plan(d)) == 0
    plain, _ = _run(gpu, d, xs)
    monkeypatch.delenv("MARS_HIP_NO_SPLIT")
    for f in range(B):
        g, rc = run_oracle(orc, d, xs[f])
        assert rc == 0
        for oi, ti in enumerate(hdr["outputs"]):
            want = g.tensor(ti)
            assert len(np.unique(want)) > 16
            assert np.array_equal(fused[oi][f], want), (f, oi, int((fused[oi][f] != want).sum()))
            assert np.array_equal(plain[oi][f], want), (f, oi)


# maps: one full tile; ragged last row and column (fill 0.97 and 0.92 of the 16-row tiles); all inside the kernel's 85 % fill rule.
# stride 2 from an even (2h) and an odd (2h - 1) input size
@pytest.mark.parametrize("h,w", [(16, 16), (31, 32), (30, 47)])
@pytest.mark.parametrize("stride,odd", [(1, 0), (2, 0), (2, 1)])
@pytest.mark.parametrize("in_c", [16, 32, 64])
def test_split_site(gpu, orc, monkeypatch, in_c, stride, odd, h, w):
    """both sides are graph outputs; batch 3, so a workgroup's tiles cross frame boundaries in the ring"""
    d = split_site(in_c, h, w, stride, odd, seed=in_c + h + w + 7 * stride + odd)
    _check(gpu, orc, monkeypatch, d, 1, seed=in_c + h + stride)


@pytest.mark.parametrize("stride", [1, 2])
def test_split_site_feeds_a_c3_remainder(gpu, orc, monkeypatch, stride):
    """the pair's results feed the rest of a C3 block, whose 3x3 takes cv3 (fuse_post): both fusions in one plan"""
    d = split_site(32, 31, 32, stride, 0, seed=100 + stride, tail="c3")
    monkeypatch.delenv("MARS_HIP_NO_POST", raising=False)
    assert sum(" post_next" in l for l in gpu.describe_plan(d)) == 1
    _check(gpu, orc, monkeypatch, d, 1, seed=10 + stride)


@pytest.mark.parametrize("ring", [1, 2, 3, 4])
@pytest.mark.parametrize("variant", [10, 9, 11])  # 16 / 8 / 4 tile rows
@pytest.mark.parametrize("in_c,stride", [(32, 1), (16, 2)])
def test_split_site_every_tile_height_and_ring(gpu, orc, monkeypatch, in_c, stride, variant, ring):
    """every instantiation of the fused kernel, forced through the launch knobs; the LDS budget is raised so that four patch buffers fit (stride 1,
    32 channels: 11 KB patches of 16-row tiles; stride 2, 16 channels: 18 KB)"""
    d = split_site(in_c, 31, 32, stride, stride - 1, seed=400 + in_c + stride)
    try:
        gpu.set_tuning("variant", variant)
        gpu.set_tuning("patch_ring", ring)
        gpu.set_tuning("patch_lds_kb", 160)
        _check(gpu, orc, monkeypatch, d, 1, seed=variant + ring)
    finally:
        gpu.set_tuning("variant", 0)
        gpu.set_tuning("patch_ring", 0)
        gpu.set_tuning("patch_lds_kb", 80)


def test_split_site_small_batch_policy(gpu, orc, monkeypatch):
    """few workgroups: the small-batch policy runs the fused launch on 4-row tiles (a flagged op has no other launch form)"""
    d = split_site(32, 31, 32, 2, 0, seed=500)
    try:
        gpu.set_tuning("few_wgs", 1 << 20)
        _check(gpu, orc, monkeypatch, d, 1, B=1, seed=5)
    finally:
        gpu.set_tuning("few_wgs", 256)


@pytest.mark.parametrize("tail", ["third", "t_out"])
def test_declined_result_has_another_use(gpu, orc, monkeypatch, tail):
    """a third reader of the k x k result, or the result a graph output: it must be written, the pair stays a launch of its own"""
    d = split_site(32, 31, 32, 2, 0, seed=600 + len(tail), tail=tail)
    _check(gpu, orc, monkeypatch, d, 0, seed=6)
    assert sum(" pair_next" in l for l in gpu.describe_plan(d)) == 1


def test_declined_members_write_channel_slices(gpu, orc, monkeypatch):
    """cv1 and cv2 write the slices of a materialised concat: the fused launch stores dense tensors only, and no pair is formed over slices"""
    d = slices_site(31, 32, seed=700)
    plan = [l for l in gpu.describe_plan(d) if l.startswith("op ")]
    assert sum(" pix_stride=64" in l for l in plan) == 2, plan
    _check(gpu, orc, monkeypatch, d, 0, seed=7)


def test_declined_below_the_fill_rule(gpu, orc, monkeypatch):
    d = split_site(32, 20, 20, 2, 0, seed=800)
    _check(gpu, orc, monkeypatch, d, 0, seed=8)


# layer 3 (width 8) writes a 16 x 16 map at 64 and 32 x 32 at 128; layer 23 (width 4) 8 x 8 at 64 (below the fill rule: declined) and 16 x 16 at 128
@pytest.mark.parametrize("width,hw,site", [(8, 64, True), (8, 128, True), (4, 64, False), (4, 128, True)])
def test_whole_twins(gpu, orc, monkeypatch, width, hw, site):
    """whole twins with per-convolution scales, batch 2: every graph output and both sides' tensors against the oracle and against the pass
    switched off; the elided tensor does not read back"""
    B = 2
    monkeypatch.delenv("MARS_HIP_NO_SPLIT", raising=False)
    d = gpu.synth_model(width_x16=width, input_hw=hw, seed=70 + hw + width, vary_scales=True)
    hdr, tensors, _ = marsfile.parse(d)
    nb = marsfile.tensor_nbytes(tensors[hdr["inputs"][0]])
    xs = [lcg_frame(0x5711F00 + f, nb) for f in range(B)]
    plan = [l for l in gpu.describe_plan(d) if l.startswith("op ")]
    layer = 3 if width == 8 else 23
    i = [k for k, l in enumerate(plan) if int(l.split()[3]) == layer][0]
    assert (" split_next" in plan[i]) == site and _flags(plan) == int(site), plan[i]
    assert " pair_next" in plan[i + 1] and " k1x1 s1 c64->32 " in plan[i + 1] and " k1x1 s1 c64->32 " in plan[i + 2]
    t_mid = int(plan[i].split(" out ")[1].split()[0])
    sides = [int(plan[i + 1].split(" out ")[1].split()[0]), int(plan[i + 2].split(" out ")[1].split()[0])]

    fused, fsides = _run(gpu, d, xs, extra=sides)
    monkeypatch.setenv("MARS_HIP_NO_SPLIT", "1")
    plain, psides = _run(gpu, d, xs, extra=sides + [t_mid])
    monkeypatch.delenv("MARS_HIP_NO_SPLIT")
    for f in range(B):
        g, rc = run_oracle(orc, d, xs[f])
        assert rc == 0
        for oi, ti in enumerate(hdr["outputs"]):
            assert np.array_equal(fused[oi][f], g.tensor(ti)), (f, oi)
            assert np.array_equal(plain[oi][f], g.tensor(ti)), (f, oi)
        for k, ti in enumerate(sides):
            want = g.tensor(ti)
            assert len(np.unique(want)) > 16
            assert np.array_equal(fsides[k][f], want), (f, k, int((fsides[k][f] != want).sum()))
            assert np.array_equal(psides[k][f], want), (f, k)
        assert np.array_equal(psides[2][f], g.tensor(t_mid)), f
    if site:  # never written, never allocated: as a fused cv3's u
        m = gpu.Model(d, batch=B)
        m.run()
        with pytest.raises(gpu.MarsError):
            m.read_tensor(t_mid)
        m.close()
