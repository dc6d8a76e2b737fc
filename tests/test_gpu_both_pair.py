"""C3's cv1 + cv2 with sides of 64 channels as ONE tile of the tile walker (pair_convs' pair_both, conv_i8_persist<BOTH>): tile rows 0-63 are
cv1, rows 64-127 cv2, the input K step -- a never-materialised concat included -- is staged once for both.  Single sites and whole twins, bit
for bit against the CPU oracle and against the same file loaded with the form switched off (MARS_HIP_NO_BOTH: side-by-side pairs over plain
inputs, two launches over a concat), at both tile widths, with resident and with streamed weights.  Every convolution has its own three
scales, weights and bias, so the two sides' tables and combined scales differ: a swap of the sides or of their tables cannot pass.
The 1x1 from 64 to 64 channels behind one side (the bottleneck's m.cv1) evaluated in that side's waves (fuse_both_chain,
conv_i8_persist<CHAIN>), with the side stored or -- where the 1x1 is its only reader -- elided, against the oracle and against
MARS_HIP_NO_BOTH_CHAIN and MARS_HIP_NO_BOTH."""
import numpy as np
import pytest

import marsfile
from conftest import lcg_frame
from test_gpu_graph import run_oracle
from test_gpu_split_fusion import _silu_conv

pytestmark = pytest.mark.gpu


def both_site(in_c, h, w, seed, cat=None, tail="outputs", x_scale=0.037, side=1, oc=64):
    """cv1, cv2: SiLU 1x1s from in_c to oc (64, or 128: the 256-row tile) channels each on an h x w map, over
      cat None   the graph input x (in_c channels)
      cat "up"   concat({2x upsample of a half-size tensor, x}), in_c / 2 channels each: the neck's C3 (h, w even)
      cat "flat" concat({a 3 x 3 convolution of x, x}), in_c / 2 channels each (any h, w)
    tail:
      outputs   both sides are graph outputs
      c3        a C3's remainder behind them: the bottleneck's 1x1 and 3x3 on cv1's branch (no shortcut), cv3 over concat({that, cv2})
      c3add     ... with the shortcut: an Add of cv1 and the 3x3's result, so cv1 has a second reader
      chain     D: a SiLU 1x1 (64 -> 64) reads side `side` (1 = cv1, 2 = cv2); the outputs are the other side and D: the side is D's alone
      chain_out ... and the side is a graph output as well
      chain_2nd ... and a second 1x1 (64 -> 32) reads the side too"""
    rng = np.random.default_rng(seed)
    G = marsfile.Graph()
    if cat is None:
        x = src = G.tensor([1, h, w, in_c], scale=x_scale)
    else:
        c = in_c // 2
        x = G.tensor([1, h, w, c], scale=0.04)
        if cat == "up":
            half = _silu_conv(G, rng, x, c, c, h // 2, w // 2, 3, 0.06, 1.0 / 250, 0.042, wscale=0.004, stride=2)
            first = G.tensor([1, h, w, c], scale=0.042)
            G.upsample(half, first, 2, 2)
        else:
            first = _silu_conv(G, rng, x, c, c, h, w, 3, 0.06, 1.0 / 250, 0.042, wscale=0.004)
        src = G.tensor([1, h, w, in_c], scale=0.042)
        G.concat([first, x], src)
    ws = 0.25 / in_c
    cv1 = _silu_conv(G, rng, src, in_c, oc, h, w, 1, 0.05, 1.0 / 256, 0.031, wscale=ws)
    cv2 = _silu_conv(G, rng, src, in_c, oc, h, w, 1, 0.09, 1.0 / 200, 0.07, wscale=1.4 * ws)
    outs = [cv1, cv2]
    if tail in ("c3", "c3add"):
        b1 = _silu_conv(G, rng, cv1, 64, 64, h, w, 1, 0.06, 1.0 / 256, 0.045, wscale=0.006)
        u = _silu_conv(G, rng, b1, 64, 64, h, w, 3, 0.055, 1.0 / 240, 0.038, wscale=0.002)
        if tail == "c3add":
            mm = G.tensor([1, h, w, 64], scale=0.052)
            G.layer(marsfile.ADD, [cv1, u], [mm])
            u = mm
        cat2 = G.tensor([1, h, w, 128], scale=0.05)
        G.concat([u, cv2], cat2)
        outs = [_silu_conv(G, rng, cat2, 128, 128, h, w, 1, 0.07, 1.0 / 256, 0.047, wscale=0.004)]
    elif tail.startswith("chain"):
        src, other = (cv1, cv2) if side == 1 else (cv2, cv1)
        dd = _silu_conv(G, rng, src, 64, 64, h, w, 1, 0.06, 1.0 / 230, 0.045, wscale=0.006)
        outs = [other, dd]
        if tail == "chain_out":
            outs.append(src)
        elif tail == "chain_2nd":
            outs.append(_silu_conv(G, rng, src, 64, 32, h, w, 1, 0.07, 1.0 / 220, 0.05, wscale=0.007))
    return G.serialise([x], outs)


def _chains(plan):
    """(side, elided) of every chained 1x1 of a plan"""
    return [(int(l.split(" both_chain=")[1].split()[0]), " both_elide" in l) for l in plan if " both_chain=" in l]


def _run(gpu, d, xs):
    m = gpu.Model(d, batch=len(xs))
    for f, x in enumerate(xs):
        m.input_view(0)[f] = x
    m.run()
    outs = [m.output_view(i).copy() for i in range(m.header.num_outputs)]
    m.close()
    return outs


def _ops(gpu, d):
    return [l for l in gpu.describe_plan(d) if l.startswith("op ")]


def _both(plan):
    return sum(" pair_both" in l for l in plan)


def _frames(d, B, seed):
    hdr, tensors, _ = marsfile.parse(d)
    nb = marsfile.tensor_nbytes(tensors[hdr["inputs"][0]])
    return hdr, [lcg_frame(0xB07A100 + 16 * seed + f, nb) for f in range(B)]


def _check(gpu, orc, monkeypatch, d, want_sites, B, seed, over_concat, want_chains=()):
    """the one-tile form is in the plan `want_sites` times, with the chains `want_chains` ((side, elided) each); its bytes, the bytes of the
    plans with the chain and with the form switched off, and the oracle's agree"""
    hdr, xs = _frames(d, B, seed)
    monkeypatch.delenv("MARS_HIP_NO_BOTH", raising=False)
    monkeypatch.delenv("MARS_HIP_NO_BOTH_CHAIN", raising=False)
    plan = _ops(gpu, d)
    assert _both(plan) == want_sites, plan
    assert _chains(plan) == list(want_chains), plan
    if over_concat:
        assert all(" seg=2" in l for l in plan if " pair_both" in l), plan
    one_tile = _run(gpu, d, xs)
    monkeypatch.setenv("MARS_HIP_NO_BOTH_CHAIN", "1")
    unchained = _ops(gpu, d)
    assert _both(unchained) == want_sites and _chains(unchained) == [], unchained
    nochain = _run(gpu, d, xs) if want_chains else one_tile
    monkeypatch.delenv("MARS_HIP_NO_BOTH_CHAIN")
    monkeypatch.setenv("MARS_HIP_NO_BOTH", "1")
    off = _ops(gpu, d)
    assert _both(off) == 0 and _chains(off) == []
    if over_concat:  # no pair is formed over a concat without the form
        assert not any(" pair_next" in l and " seg=" in l for l in off), off
    plain = _run(gpu, d, xs)
    monkeypatch.delenv("MARS_HIP_NO_BOTH")
    for f in range(B):
        g, rc = run_oracle(orc, d, xs[f])
        assert rc == 0
        for oi, ti in enumerate(hdr["outputs"]):
            want = g.tensor(ti)
            assert len(np.unique(want)) > 16
            assert np.array_equal(one_tile[oi][f], want), (f, oi, int((one_tile[oi][f] != want).sum()))
            assert np.array_equal(nochain[oi][f], want), (f, oi)
            assert np.array_equal(plain[oi][f], want), (f, oi)


# maps: less than one tile; exactly one 256-pixel tile (one frame); ragged last tile, tiles across frame boundaries (batch 3).
# in_c 64 / 128 / 256 keep the weights of both sides resident in LDS, 512 does not (1 KB + 2 pixel stages + 8 K steps x 8 KB > 80 KB)
MAPS = [(5, 5, 2), (16, 16, 1), (12, 12, 3)]


@pytest.mark.parametrize("h,w,B", MAPS)
@pytest.mark.parametrize("in_c", [64, 128, 256, 512])
def test_plain_input(gpu, orc, monkeypatch, in_c, h, w, B):
    d = both_site(in_c, h, w, seed=in_c + h)
    _check(gpu, orc, monkeypatch, d, 1, B, seed=in_c + h + B, over_concat=False)


@pytest.mark.parametrize("h,w,B,cat", [(5, 5, 2, "flat"), (6, 6, 2, "up"), (16, 16, 1, "up"), (12, 12, 3, "up")])
@pytest.mark.parametrize("in_c", [64, 128, 256, 512])
def test_concat_input(gpu, orc, monkeypatch, in_c, h, w, B, cat):
    """two segments of in_c / 2 channels (in_c 64: a K step's halves come from different tensors); "up": the first one is read through the 2x
    nearest upsample of its half-size tensor (even maps only: 6 x 6 stands in for 5 x 5 there)"""
    d = both_site(in_c, h, w, seed=1000 + in_c + h, cat=cat)
    if cat == "up":
        assert not any(" upsample" in l.lower() for l in _ops(gpu, d)), "the upsample is folded into the segmented read"
    _check(gpu, orc, monkeypatch, d, 1, B, seed=in_c + h + B + 1, over_concat=True)


@pytest.mark.parametrize("wres", [3, 0])
@pytest.mark.parametrize("bpx", [128, 256])
@pytest.mark.parametrize("in_c,cat", [(128, None), (256, "up"), (64, "up")])
def test_every_tile_width_and_weight_form(gpu, orc, monkeypatch, in_c, cat, bpx, wres):
    """both instantiations (128 / 256 pixels per tile), weights resident and streamed through the ring, forced through the launch knobs:
    12 x 12 at batch 3 is 432 pixels -- a ragged last tile either way, tiles that cross frame boundaries"""
    d = both_site(in_c, 12, 12, seed=2000 + in_c + bpx, cat=cat)
    try:
        gpu.set_tuning("both_bpx", bpx)
        gpu.set_tuning("wres", wres)
        _check(gpu, orc, monkeypatch, d, 1, 3, seed=bpx + wres + in_c, over_concat=cat is not None)
    finally:
        gpu.set_tuning("both_bpx", 0)
        gpu.set_tuning("wres", 3)


@pytest.mark.parametrize("cat", [None, "up"])
def test_inside_a_c3(gpu, orc, monkeypatch, cat):
    """the C3's remainder behind the pair (the neck's block has no shortcut): cv1's side is read by the bottleneck's 1x1, cv2's by cv3"""
    d = both_site(128, 12, 12, seed=3000, cat=cat, tail="c3")
    _check(gpu, orc, monkeypatch, d, 1, 3, seed=30, over_concat=cat is not None, want_chains=[(1, True)])


@pytest.mark.parametrize("cat", [None, "up"])
def test_inside_a_c3_with_a_shortcut(gpu, orc, monkeypatch, cat):
    """the backbone's block: the Add (folded into the 3x3) reads cv1 too, so the side is chained and kept"""
    d = both_site(128, 12, 12, seed=3100, cat=cat, tail="c3add")
    assert sum(" add=" in l for l in _ops(gpu, d)) == 1
    _check(gpu, orc, monkeypatch, d, 1, 3, seed=31, over_concat=cat is not None, want_chains=[(1, False)])


@pytest.mark.parametrize("h,w,B", MAPS)
@pytest.mark.parametrize("side", [1, 2])
@pytest.mark.parametrize("in_c,cat", [(64, None), (128, None), (256, "flat"), (512, "flat")])
def test_chain_elided(gpu, orc, monkeypatch, in_c, cat, side, h, w, B):
    """the 1x1 is the side's only reader: the side is not stored, its tensor is not allocated"""
    d = both_site(in_c, h, w, seed=6000 + in_c + h + side, cat=cat, tail="chain", side=side)
    _check(gpu, orc, monkeypatch, d, 1, B, seed=60 + in_c + h + side, over_concat=cat is not None, want_chains=[(side, True)])


@pytest.mark.parametrize("tail", ["chain_out", "chain_2nd"])
@pytest.mark.parametrize("side", [1, 2])
@pytest.mark.parametrize("in_c,cat", [(128, None), (256, "up")])
def test_chain_side_kept(gpu, orc, monkeypatch, in_c, cat, side, tail):
    """the side is a graph output, or a second 1x1 (another shape, a launch of its own) reads it: chained and stored"""
    d = both_site(in_c, 12, 12, seed=6500 + in_c + side, cat=cat, tail=tail, side=side)
    _check(gpu, orc, monkeypatch, d, 1, 3, seed=65 + in_c + side, over_concat=cat is not None, want_chains=[(side, False)])


@pytest.mark.parametrize("wres", [3, 0])
@pytest.mark.parametrize("bpx", [128, 256])
@pytest.mark.parametrize("side,tail", [(1, "chain"), (2, "chain_out")])
def test_chain_every_tile_width_and_weight_form(gpu, orc, monkeypatch, side, tail, bpx, wres):
    d = both_site(256, 12, 12, seed=6700 + bpx + side, cat="up", tail=tail, side=side)
    try:
        gpu.set_tuning("both_bpx", bpx)
        gpu.set_tuning("wres", wres)
        _check(gpu, orc, monkeypatch, d, 1, 3, seed=bpx + wres + side, over_concat=True, want_chains=[(side, tail == "chain")])
    finally:
        gpu.set_tuning("both_bpx", 0)
        gpu.set_tuning("wres", 3)


@pytest.mark.parametrize("wres", [3, 0])
@pytest.mark.parametrize("h,w,B", MAPS)
@pytest.mark.parametrize("in_c,cat", [(128, None), (256, None), (256, "flat"), (512, "flat")])
def test_sides_of_128(gpu, orc, monkeypatch, in_c, cat, h, w, B, wres):
    """the 256-row tile (part 2), behind its knob: off by default (a side-by-side pair over a tensor, two launches over a concat), on it is
    one tile; in_c 128 keeps the weights resident, 256 and 512 stream them"""
    d = both_site(in_c, h, w, seed=7000 + in_c + h, cat=cat, oc=128)
    monkeypatch.delenv("MARS_HIP_NO_BOTH", raising=False)
    assert _both(_ops(gpu, d)) == 0
    try:
        gpu.set_tuning("both_wide", 2)  # (1: over a concat only -- over a tensor the instantiation holds one workgroup per CU)
        gpu.set_tuning("wres", wres)
        _check(gpu, orc, monkeypatch, d, 1, B, seed=70 + in_c + h, over_concat=cat is not None)
    finally:
        gpu.set_tuning("both_wide", 0)
        gpu.set_tuning("wres", 3)


@pytest.mark.parametrize("variant", [2, 14])
def test_forced_launch_variant(gpu, orc, monkeypatch, variant):
    """a launch variant forced from outside: a plain one-tile pair steps aside (its members run as that variant, one after the other), a
    chained one has no other form and runs as it is; same bytes either way"""
    try:
        gpu.set_tuning("variant", variant)
        d = both_site(256, 12, 12, seed=6900 + variant, cat="up")
        _check(gpu, orc, monkeypatch, d, 1, 3, seed=69 + variant, over_concat=True)
        d = both_site(256, 12, 12, seed=6950 + variant, cat="up", tail="c3")
        _check(gpu, orc, monkeypatch, d, 1, 3, seed=70 + variant, over_concat=True, want_chains=[(1, True)])
    finally:
        gpu.set_tuning("variant", 0)


def test_elided_tensor_cannot_be_read(gpu, monkeypatch):
    monkeypatch.delenv("MARS_HIP_NO_BOTH", raising=False)
    monkeypatch.delenv("MARS_HIP_NO_BOTH_CHAIN", raising=False)
    d = both_site(128, 12, 12, seed=6800, tail="chain", side=1)
    plan = _ops(gpu, d)
    assert _chains(plan) == [(1, True)]
    t_side = int([l for l in plan if " pair_both" in l][0].split(" out ")[1].split()[0])
    m = gpu.Model(d, batch=1)
    m.run()
    with pytest.raises(gpu.MarsError):
        m.read_tensor(t_side)
    m.close()


def test_declined_without_a_half_step_table(gpu, orc, monkeypatch):
    """an input scale of 0.04 makes cv1's combined scale 1 / 640, which the half-step table cannot serve (an accumulator of 320 requantises to
    0.49999997: mhip_conv_i8_lut2_ok); the form needs both tables, so the pair stays side by side"""
    d = both_site(128, 12, 12, seed=4100, x_scale=0.04)
    monkeypatch.delenv("MARS_HIP_NO_BOTH", raising=False)
    assert sum(" pair_next" in l for l in _ops(gpu, d)) == 1
    _check(gpu, orc, monkeypatch, d, 0, 3, seed=41, over_concat=False)


def test_declined_sides_of_32(gpu, orc, monkeypatch):
    """sides of 32 channels over a plain input stay a side-by-side pair"""
    rng = np.random.default_rng(4000)
    G = marsfile.Graph()
    x = G.tensor([1, 12, 12, 64], scale=0.04)
    cv1 = _silu_conv(G, rng, x, 64, 32, 12, 12, 1, 0.05, 1.0 / 256, 0.031, wscale=0.004)
    cv2 = _silu_conv(G, rng, x, 64, 32, 12, 12, 1, 0.09, 1.0 / 200, 0.07, wscale=0.006)
    d = G.serialise([x], [cv1, cv2])
    monkeypatch.delenv("MARS_HIP_NO_BOTH", raising=False)
    assert sum(" pair_next" in l for l in _ops(gpu, d)) == 1
    _check(gpu, orc, monkeypatch, d, 0, 3, seed=40, over_concat=False)


@pytest.mark.parametrize("width", [8, 4])
def test_whole_twins(gpu, orc, monkeypatch, width):
    """64 x 64 twins with per-convolution scales, batch 3: every graph output against the oracle, with the form and without"""
    d = gpu.synth_model(width_x16=width, input_hw=64, seed=250 + width, vary_scales=True)
    hdr, xs = _frames(d, 3, width)
    monkeypatch.delenv("MARS_HIP_NO_BOTH", raising=False)
    plan = _ops(gpu, d)
    assert _both(plan) >= 1 and any(" pair_both" in l and " seg=2" in l for l in plan), plan
    assert (1, False) in _chains(plan) and (1, True) in _chains(plan), plan  # the backbone's block keeps cv1, the neck's elides it
    one_tile = _run(gpu, d, xs)
    monkeypatch.setenv("MARS_HIP_NO_BOTH_CHAIN", "1")
    assert _chains(_ops(gpu, d)) == []
    nochain = _run(gpu, d, xs)
    monkeypatch.delenv("MARS_HIP_NO_BOTH_CHAIN")
    monkeypatch.setenv("MARS_HIP_NO_BOTH", "1")
    assert _both(_ops(gpu, d)) == 0
    plain = _run(gpu, d, xs)
    monkeypatch.delenv("MARS_HIP_NO_BOTH")
    for f in range(3):
        g, rc = run_oracle(orc, d, xs[f])
        assert rc == 0
        for oi, ti in enumerate(hdr["outputs"]):
            want = g.tensor(ti)
            assert np.array_equal(one_tile[oi][f], want), (f, oi, int((one_tile[oi][f] != want).sum()))
            assert np.array_equal(nochain[oi][f], want), (f, oi)
            assert np.array_equal(plain[oi][f], want), (f, oi)


def test_batch_change_on_one_instance(gpu, orc, monkeypatch):
    """1 -> 3 -> 1 frames on one model: alloc_batch asks the device code again for every batch"""
    monkeypatch.delenv("MARS_HIP_NO_BOTH", raising=False)
    monkeypatch.delenv("MARS_HIP_NO_BOTH_CHAIN", raising=False)
    d = both_site(256, 12, 12, seed=5000, cat="up", tail="c3")
    assert _both(_ops(gpu, d)) == 1 and _chains(_ops(gpu, d)) == [(1, True)]
    hdr, xs = _frames(d, 3, 50)
    want = []
    for x in xs:
        g, rc = run_oracle(orc, d, x)
        assert rc == 0
        want.append([g.tensor(ti) for ti in hdr["outputs"]])
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
