"""The sites of tests/edgecases.py on the host: each one plans as the launch form it is meant to reach, the numpy model of every requantising
stage equals the CPU oracle, the oracle equals the reference build on the same file, and -- from the numpy accumulators and the oracle's table
alone, never from the library -- every stage meets its coverage conditions: at least 32 witnessed ties of each sign, 16 results clamped on each
side, 8 with |2p| >= 256, and every listed edge accumulator at a pixel of every frame.  tests/test_gpu_requant_edges.py runs the same sites
through the kernels."""
import numpy as np
import pytest

import edgecases
import marsfile

SITES = edgecases.all_sites()
_cache = {}


def _site(name, orc):
    if name not in _cache:
        s = SITES[name]()
        per_frame, cov = edgecases.evaluate(orc, s)  # asserts: numpy model == oracle, stage by stage, frame by frame; edge accumulators present
        _cache[name] = (s, per_frame, cov)
    return _cache[name]


def _plan(marsrt, monkeypatch, s, flags=0, fusion=None):
    monkeypatch.setenv("MARS_HIP_FUSION", str(s.fusion if fusion is None else fusion))
    for k in ("MARS_HIP_NO_BOTH", "MARS_HIP_NO_BOTH_CHAIN", "MARS_HIP_NO_SPLIT", "MARS_HIP_NO_CHAIN", "MARS_HIP_NO_POST", "MARS_HIP_BOTTLENECK_LIMIT"):
        monkeypatch.delenv(k, raising=False)
    return [l for l in marsrt.describe_plan(s.d, flags) if l.startswith("op ")]


@pytest.mark.parametrize("name", list(SITES))
def test_site_plans_as_intended(marsrt, monkeypatch, name):
    s = SITES[name]()
    plan = _plan(marsrt, monkeypatch, s)
    for flag in s.form:
        assert any(flag in l for l in plan), (flag, plan)
    full = _plan(marsrt, monkeypatch, s, flags=2)
    for flag in s.full:
        assert any(flag in l for l in full), (flag, plan)
    convs = [l for l in full if " conv_i8 " in l]
    assert convs and " safe %d " % s.safe in convs[0], convs[0]
    if s.lut2 is not None:  # the half-step table: on every convolution of a dyadic site, on none where the scale is refused
        assert all((" lut2_off -1 " not in l) == s.lut2 for l in convs if " lut" in l.split(" | ")[0]), plan
    # every fusion of the site has a switch that takes it out of the plan again
    for sw in s.off:
        monkeypatch.setenv(sw, "2")
        off = [l for l in marsrt.describe_plan(s.d, 2) if l.startswith("op ")]
        monkeypatch.delenv(sw)
        if sw != "MARS_HIP_BOTTLENECK_LIMIT":  # (that one acts per batch, at allocation)
            assert off != full, (sw, plan)
    # the unfused plan keeps every layer that requantises as a launch of its own
    plain = _plan(marsrt, monkeypatch, s, fusion=0)
    assert len(plain) >= len(plan) and not any(f in l for l in plain for f in (" split_next", " post_next", " pair_both", " pre")), plain


def test_refused_scale_has_the_quirk_accumulator(marsrt, orc):
    """1 / 640: an accumulator lands on 0x3EFFFFFF, the host refuses the half-step table, the reference rounds +-a* to +-1"""
    s, per_frame, cov = _site("slow_table", orc)
    cs = cov[0]["cs"]
    assert marsrt.lib().mhip_conv_i8_lut2_ok(__import__("ctypes").c_float(cs)) == 0
    a = s.quirk
    assert a == edgecases.quirk_acc(cs) and a in s.stages[0]["edges"].values() and -a in s.stages[0]["edges"].values()
    q, p, r = edgecases.requant(np.array([a, -a, a - 1, 1 - a]), cs)
    assert p[0].view(np.uint32) == 0x3EFFFFFF and list(q) == [1, -1, 0, 0]
    assert int(np.float32(2) * p[0]) == 0  # what the half-step index would make of it
    for e in (-4, -5, -3):
        assert marsrt.lib().mhip_conv_i8_lut2_ok(__import__("ctypes").c_float(2.0 ** e)) == 1


def test_witness_table(orc):
    """the table behind every site: neighbours differ for most inputs (measured through the oracle)"""
    s, _, _ = _site("k1_16x16", orc)
    tab, _ = edgecases.table_after(orc, marsfile.parse(s.d), s.stages[0]["layer"])
    d = tab[1:] != tab[:-1]   # d[i]: inputs i - 128 and i - 127 map to different bytes
    assert int(d[:128].sum()) >= 70 and int(d[128:].sum()) >= 120, (int(d[:128].sum()), int(d[128:].sum()))


@pytest.mark.parametrize("name", list(SITES))
def test_numpy_model_equals_the_oracle_and_covers_the_edges(orc, name):
    s, per_frame, cov = _site(name, orc)
    edgecases.check_needs(s, cov)
    hdr, tensors, _ = marsfile.parse(s.d)
    for ti in hdr["outputs"]:
        assert len(np.unique(np.concatenate([t[ti] for t in per_frame]))) > 16


@pytest.mark.parametrize("name", list(SITES))
def test_oracle_equals_the_reference(orc, ref, name):
    """the restatement is not the only witness: the reference's own layer functions on the same file, every activation tensor"""
    s, per_frame, _ = _site(name, orc)
    for f in (0, len(s.frames) - 1):
        r = ref.O2Model(s.d)
        r.set_input(0, s.frames[f].tobytes())
        assert r.run() == 0
        for ti, want in per_frame[f].items():
            assert np.array_equal(r.tensor(ti)[:len(want)], want), (name, f, ti)
        r.close()
