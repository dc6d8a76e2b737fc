"""The int8 fused-table epilogues at rounding ties, both clamps and the accumulator edges (tests/edgecases.py; the conditions those sites meet are
asserted on the host by tests/test_requant_edges_cpu.py).  Every site runs under the default plan, with each of its fusions switched off, under
the forced launch variants that take its shape, and unfused (fusion 0: the no-table epilogue, lut_i8_kernel and binary_i8_kernel meet the same
ties and clamps, and every tensor is materialised) -- bit for bit against the CPU oracle each time."""
import ctypes

import numpy as np
import pytest

import edgecases
import marsfile

pytestmark = pytest.mark.gpu

SITES = edgecases.all_sites()
_cache = {}


def _site(name, orc):
    """the site with the oracle's tensors of every frame (computed once per module: the forced-variant cases reuse them)"""
    if name not in _cache:
        s = SITES[name]()
        per_frame, cov = edgecases.evaluate(orc, s)
        edgecases.check_needs(s, cov)
        _cache[name] = (s, per_frame)
    return _cache[name]


def _rows_launches(gpu):
    count = gpu.lib().mhip_conv_i8_rows_launches
    count.restype = ctypes.c_ulong
    return count()


def _run_and_compare(gpu, s, per_frame, fusion, what):
    """one model, all frames; the graph outputs -- and at fusion 0 every activation tensor -- against the oracle's"""
    hdr, tensors, _ = marsfile.parse(s.d)
    B = len(s.frames)
    m = gpu.Model(s.d, batch=B, fusion=fusion)
    try:
        for f in range(B):
            m.input_view(0)[f] = s.frames[f]
        n0 = _rows_launches(gpu)
        m.run()
        assert _rows_launches(gpu) - n0 >= s.min_rows, (s.name, what, "the rows kernel did not run")
        for f in range(B):
            for oi, ti in enumerate(hdr["outputs"]):
                want, got = per_frame[f][ti], m.output_view(oi)[f]
                bad = np.flatnonzero(got != want)
                assert bad.size == 0, (s.name, what, "frame %d output %d" % (f, oi), int(bad.size),
                                       [(int(i), int(got.view(np.int8)[i]), int(want.view(np.int8)[i])) for i in bad[:8]])
            if fusion == 0:
                for ti, want in per_frame[f].items():
                    got = m.read_tensor(ti, frame=f)
                    assert np.array_equal(got, want), (s.name, what, "frame %d tensor %d" % (f, ti), int((got != want).sum()))
    finally:
        m.close()


def _with_tuning(gpu, knobs, fn):
    """knobs: ((name, value, default), ...), restored whatever happens"""
    try:
        for k, v, _ in knobs:
            gpu.set_tuning(k, v)
        fn()
    finally:
        for k, _, dflt in knobs:
            gpu.set_tuning(k, dflt)


SWITCHES = ("MARS_HIP_NO_BOTH", "MARS_HIP_NO_BOTH_CHAIN", "MARS_HIP_NO_SPLIT", "MARS_HIP_NO_CHAIN", "MARS_HIP_NO_POST", "MARS_HIP_BOTTLENECK_LIMIT")


@pytest.mark.parametrize("name", list(SITES))
def test_site_fused_and_with_each_fusion_off(gpu, orc, monkeypatch, name):
    s, per_frame = _site(name, orc)
    for k in SWITCHES:
        monkeypatch.delenv(k, raising=False)

    def body():
        _run_and_compare(gpu, s, per_frame, s.fusion, "default plan")
        for sw in s.off:
            monkeypatch.setenv(sw, "2")  # (the bottleneck limit: a batch of 3 counts as too large)
            try:
                _run_and_compare(gpu, s, per_frame, s.fusion, sw)
            finally:
                monkeypatch.delenv(sw)
    _with_tuning(gpu, s.tuning, body)


@pytest.mark.parametrize("name", list(SITES))
def test_site_unfused_every_tensor(gpu, orc, monkeypatch, name):
    s, per_frame = _site(name, orc)
    for k in SWITCHES:
        monkeypatch.delenv(k, raising=False)
    _with_tuning(gpu, s.tuning, lambda: _run_and_compare(gpu, s, per_frame, 0, "fusion 0"))


WALK = [(("variant", 2, 0), ("persist_slots", 1, 0)), (("variant", 2, 0), ("persist_slots", 3, 0)), (("variant", 14, 0),), (("variant", 15, 0),)]
PATCH = [(("variant", v, 0), ("patch_ring", r, 0), ("patch_lds_kb", 160 if r > 2 else 80, 80)) for v in (9, 10, 11) for r in (1, 4)]
WIDE = [(("variant", v, 0),) for v in (12, 13, 18, 19)]
FORCED = [(n, k) for n in ("k3_s1", "k3_s2") for k in WALK + PATCH] + [("k3_c128", k) for k in WIDE] + \
         [(n, k) for n in ("patch_c16", "split_s1", "split_chain2", "post_add", "add3_c32") for k in PATCH[1::2]] + \
         [("stem", (("rgb_direct", d, 1),)) for d in (1, 0)] + \
         [(n, k) for n in ("k1_16x16", "both", "both_chain1_elided", "add_c128_o0_lut", "slow_table") for k in WALK[1:3]]


@pytest.mark.parametrize("name,knobs", FORCED, ids=lambda v: v if isinstance(v, str) else "-".join("%s%d" % (k, x) for k, x, _ in v))
def test_site_under_a_forced_launch_form(gpu, orc, monkeypatch, name, knobs):
    """the launch knobs pick the kernel, never the bytes: the tile walker (streamed and resident weights), every tile height and ring depth of the
    patch-staged kernel, the wide one-tile forms, the stem with and without the direct RGB read; fused forms keep their kernel where they have
    no other"""
    s, per_frame = _site(name, orc)
    for k in SWITCHES:
        monkeypatch.delenv(k, raising=False)
    keep = tuple(t for t in s.tuning if t[0] not in [k[0] for k in knobs])
    _with_tuning(gpu, keep + tuple(knobs), lambda: _run_and_compare(gpu, s, per_frame, s.fusion, "forced"))
