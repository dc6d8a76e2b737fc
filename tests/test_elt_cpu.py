"""tests/eltref.py pinned, without a GPU.  Every case of tests/test_gpu_elt.py that a .mars file can express runs as a one-layer graph on the
CPU oracle, and eltref has to give the same bytes (floats: bit for bit, NaN for NaN) for both frames.  The oracle's observation of each
graph is then held to the compiled reference by the `witness` of tests/test_oracle.py (live where oracle/_ref was built, else as
golden.json "vs_reference" recorded it), so that eltref and the oracle are not each other's only witness.  The same graphs carry the host's
scale rules: output scales of 0, negative, NaN and 2^-127, negative and NaN input scales of the int8 sigmoid, batch-norm scales not > 0.
The builders' own assertions (ties, clamps, subnormals, witnesses of fused and reciprocal forms) run here too, with no GPU in sight."""
import numpy as np
import pytest

import eltref as E
from test_oracle import graph_of, sig, witness  # noqa: F401  (witness: a fixture)


def run_graph(impl, name, frame):
    k = E.graph_case(name)
    big = name.split("/")[0] in E.BIG_GRAPHS
    g = graph_of(impl)(k["d"], **(dict(slack_mult=1, slack_add=4096) if big else {}))
    for i, frames in enumerate(k["inputs"]):
        g.set_input(i, np.ascontiguousarray(frames[frame]).tobytes())
    rc = g.run()
    out = g.tensor(k["out"])
    g.close()
    return rc, out


def observe(impl, name):
    """what the witness compares: return code and the output tensor's bytes of both frames; every float NaN as one pattern (which operand's
    payload a NaN + NaN keeps is the compiler's choice of operand order, not the layer's)"""
    obs = {}
    for f in range(2):
        rc, out = run_graph(impl, name, f)
        if E.graph_case(name)["dtype"] == "f32":
            out = out.view(np.float32).copy()
            out[np.isnan(out)] = E.from_bits([0x7FC00000])[0]
        obs["rc%d" % f], obs["out%d" % f] = rc, sig(out)
    return obs


@pytest.mark.parametrize("name", E.GRAPH_CASES)
def test_graph_cases(orc, witness, name):
    k = E.graph_case(name)
    for f in range(2):
        rc, out = run_graph(orc, name, f)
        assert rc == 0
        E.assert_same("%s frame %d" % (name, f), out, k["want"][f], k["dtype"])
    witness("elt/" + name, observe(orc, name), lambda R: observe(R, name))


def record(R):
    """golden.json "vs_reference": the reference's side of test_graph_cases (called by test_oracle.record_vs_reference)"""
    return {"elt/" + name: observe(R, name) for name in E.GRAPH_CASES}


# ---- the builders' assertions, and the launcher-only cases ------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", E.BINARY_CASES, ids=E.binary_id)
def test_binary_i8_builders(case):
    a, b, sa, sb, inv, want = E.binary_case(*case)
    assert len(want) == 65536 and want.dtype == np.int8


def test_unary_tables():
    E.check_unary_tables()
    for kind, sk in E.UNARY_CASES:
        for f in range(2):
            assert set(E.unary_bytes(f).tolist()) == set(range(-128, 128))


def test_bn_i8_builders():
    cs = E.bn_i8_cases()
    for name, k in cs.items():
        planes = k["x"].reshape(E.BN_N * k["c"], E.BN_HW)
        assert (np.sort(planes, axis=1) == np.arange(-128, 128)).all(), name  # every int8 value in every channel
    assert cs["searched_a"]["c"] >= 8 + len(E.SPECIAL_SC_BI) and cs["searched_b"]["c"] >= 8


def test_f32_builders():
    E.f32_binary_case()
    E.f32_relu_sweep()
    for shape in E.BN_F32_SHAPES:
        E.bn_f32_case(shape)
        E.bn_f32_case(shape, True)
    for w in E.SIGMOID_CASES:
        E.f32_sigmoid_case(w)
    assert len(E.sigmoid_band("neg")) == len(E.sigmoid_band("pos")) == 17 * (1 << 17) + 1


def test_trunc_and_compare_rules_by_hand(orc):
    F = E.F
    v = np.array([0.99, -0.99, 127.5, 2147483520.0, 2147483648.0, -2147483648.0, -2147483904.0, np.nan, np.inf, -np.inf], dtype=F)
    want = [0, 0, 127, 2147483520, E.INT_MIN, E.INT_MIN, E.INT_MIN, E.INT_MIN, E.INT_MIN, E.INT_MIN]
    assert E.trunc_x86(v).tolist() == want
    assert [orc.trunc_x86(q) for q in v] == want
    assert E.q8(np.array([3e9, -3e9, 126.5, 126.49, -128.6, np.nan], dtype=F)).tolist() == [-128, -128, 127, 126, -128, -128]
    # the comparison rule: NaN for NaN whatever the payload; -0.0 is not +0.0; NaN against a number differs
    a = E.from_bits([0x7FC00000, 0x80000000, 0x3F800000, 0x7FC00000])
    b = E.from_bits([0xFFC00001, 0x00000000, 0x3F800000, 0x3F800000])
    assert E.differing(a, b, "f32").tolist() == [1, 3] and E.differing(b, a, "f32").tolist() == [1, 3]
    assert E.relu_f32(E.from_bits([0xBF800000, 0x80000000, 0x00000000]), 0).view(np.uint32).tolist() == [0x80000000, 0x80000000, 0]


MUTATIONS = {  # the four one-line changes to eltwise.hip that the GPU tests must notice, applied to the restatement: each changes expected bytes
    "y * inv -> y / so": lambda: sum(int((E.binary_i8(m, *E.binary_case("ODD", m)[:4], E.ODD_SO, form="div") != E.binary_case("ODD", m)[5]).sum()) for m in (0, 1)),
    "y / out_scale -> y * (1 / out_scale)": lambda: sum(
        int((E.batchnorm_i8(k["x"], E.BN_N, k["c"], E.BN_HW, k["s"], k["b"], k["in_scale"], k["out_scale"], form="recip") != k["want"]).sum())
        for k in (E.bn_i8_cases()[n] for n in ("searched_a", "searched_b"))),
    "x * alpha -> 0.0f": lambda: int((E.bits(E.relu_f32(E.f32_relu_sweep(), 0, form="max")) != E.bits(E.relu_f32(E.f32_relu_sweep(), 0))).sum()),
    "no INT_MIN for v >= 2^31": lambda: sum(int((E.binary_i8(m, *E.binary_case("HUGE", m)[:5], saturating=True) != E.binary_case("HUGE", m)[5]).sum()) for m in (0, 1)),
}


@pytest.mark.parametrize("which", list(MUTATIONS))
def test_cases_tell_mutations_apart(which):
    assert MUTATIONS[which]() >= 1
