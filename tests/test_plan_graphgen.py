"""The planner's rewrites against the graph's own inputs and outputs, on random graphs (tests/graphgen.py), on the CPU (mars_hip_describe_plan).

The pipelined path (mars_hip_pipe_submit) hands every graph input and output over in a buffer of its own, with nothing mapped in front of it and
in the graph's own dense layout.  So a launch may not read a graph input or output through a view that starts in front of it (virtual_concat_f32:
view=-N), and no graph input or output may be held in another layout (nhwc_c, rec_c) or left partly unwritten (partial).  A padded pixel pitch
(pix_stride) is allowed: the pipe unpads it.  And a rank that loads descriptors only plans what rank 0 plans.  Every graph is planned at fusion
levels 0 / 1 / 2, the float ones under f32_mfma 3 and 4 (the split-bf16 modes, where virtual_concat_f32 runs) as well."""
import re

import numpy as np
import pytest

import graphgen
import marsfile

N = 30  # graphs per generator and seed


def _graphs(gen, seed, n=N, **opt):
    """the first n graphs a generator draws from one seed (the soak scripts' draws in between are not needed here)"""
    rng = np.random.default_rng(seed)
    out = []
    while len(out) < n:
        r = gen(rng, **opt)
        if r is not None:
            out.append(r[0])
    return out


# what every test below draws: name -> (generator, seed, options, f32_mfma modes it is planned under).  tools/plan_corpus.py dumps the plans of
# exactly these graphs
CORPUS = {}
for _nchw in (None, True):
    for _int in (False, True):
        CORPUS["int8", _nchw, _int] = (graphgen.int8_graph, 4100 + 2 * bool(_nchw) + _int, dict(nchw=_nchw, interior_outputs=_int), (None,))
for _int in (False, True):
    CORPUS["int8_chain", _int] = (graphgen.int8_graph, 4110 + _int, dict(nchw=True, interior_outputs=_int, concat_chain=True), (None,))
    CORPUS["f32", _int] = (graphgen.f32_graph, 4120 + _int, dict(interior_outputs=_int), (1, 3, 4))
    CORPUS["vcat_f32", _int] = (graphgen.vcat_f32_graph, 4130 + _int, dict(interior_outputs=_int), (1, 3, 4))


def corpus_graphs(key):
    gen, seed, opt, _ = CORPUS[key]
    return _graphs(gen, seed, **opt)


def strip_full(lines):
    """a MARS_HIP_DESCRIBE_FULL dump without what the flag adds: the lines that start with '+', and everything from ' |' on in the others"""
    return [l.split(" |")[0] for l in lines if not l.startswith("+")]


def plan_violations(marsrt, d):
    """-> the plan lines that break the I/O invariants, plus a note if the descriptor-only plan differs"""
    hdr = marsfile.parse(d)[0]
    io = set(hdr["inputs"]) | set(hdr["outputs"])
    L = marsrt.describe_plan(d)
    assert L, "empty plan"  # (a plan the planner's own check rejects fails the load: it must not pass for a plan without violations)
    bad = []
    for l in L:
        if l.startswith("op ") and " view=-" in l:
            t_in = [int(v) for v in re.search(r" in ((?:\d+ ?)*) out ", l).group(1).split()]
            if t_in[0] in io:
                bad.append(l)
        if l.startswith("tensor "):
            f = l.split()
            t, kv = int(f[1]), dict(zip(f[2::2], f[3::2]))
            if t in io and (int(kv["nhwc_c"]) or int(kv["partial"]) or int(kv["rec_c"])):
                bad.append(l)
    if marsrt.describe_plan(d, flags=1) != L:
        bad.append("descriptor-only plan differs")
    return bad


def check_plans(marsrt, monkeypatch, graphs, f32_modes=(None,)):
    saved = marsrt.get_tuning("f32_mfma")
    found = []
    try:
        for mode in f32_modes:
            if mode is not None:
                marsrt.set_tuning("f32_mfma", mode)
            for level in (0, 1, 2):
                monkeypatch.setenv("MARS_HIP_FUSION", str(level))
                for gi, d in enumerate(graphs):
                    found += ["graph %d mode %s level %d: %s" % (gi, mode, level, l) for l in plan_violations(marsrt, d)]
    finally:
        marsrt.set_tuning("f32_mfma", saved)
    assert not found, "\n".join(found[:20])


@pytest.fixture(autouse=True)
def _plain_env(monkeypatch):
    for k in ("MARS_HIP_NO_VCONCAT_F32", "MARS_HIP_NO_ZERO_TAIL", "MARS_HIP_NO_NHWC_INTERNAL", "MARS_HIP_FUSION", "MARS_HIP_REC_LIMIT"):
        monkeypatch.delenv(k, raising=False)


@pytest.mark.parametrize("nchw", [None, True])
@pytest.mark.parametrize("interior", [False, True])
def test_int8_graphs(marsrt, monkeypatch, nchw, interior):
    check_plans(marsrt, monkeypatch, corpus_graphs(("int8", nchw, interior)))


@pytest.mark.parametrize("interior", [False, True])
def test_int8_concat_chain_graphs(marsrt, monkeypatch, interior):
    gs = corpus_graphs(("int8_chain", interior))
    check_plans(marsrt, monkeypatch, gs)
    if not interior:  # the chain is there, and its three concats stay pixels x channels (concat_q) when no graph output pins them
        monkeypatch.setenv("MARS_HIP_FUSION", "1")
        assert sum(sum(" concat_q " in l for l in marsrt.describe_plan(d)) >= 3 for d in gs) >= N * 3 // 4


@pytest.mark.parametrize("interior", [False, True])
def test_f32_graphs(marsrt, monkeypatch, interior):
    check_plans(marsrt, monkeypatch, corpus_graphs(("f32", interior)), f32_modes=CORPUS["f32", interior][3])


@pytest.mark.parametrize("interior", [False, True])
def test_vcat_f32_graphs(marsrt, monkeypatch, interior):
    gs = corpus_graphs(("vcat_f32", interior))
    check_plans(marsrt, monkeypatch, gs, f32_modes=CORPUS["vcat_f32", interior][3])
    # (the pass still runs on these graphs: some concats are read through a view -- rarely where graph outputs sit inside the motif)
    saved = marsrt.get_tuning("f32_mfma")
    try:
        marsrt.set_tuning("f32_mfma", 3)
        assert sum(any(" view=-" in l for l in marsrt.describe_plan(d)) for d in gs) >= (1 if interior else N // 2)
    finally:
        marsrt.set_tuning("f32_mfma", saved)


@pytest.mark.parametrize("key", sorted(CORPUS, key=str), ids=lambda k: "-".join(str(v) for v in k))
def test_full_dump_only_adds(marsrt, monkeypatch, key):
    """MARS_HIP_DESCRIBE_FULL (flags=2) adds fields and lines and alters nothing: stripped of them, the full dump of every graph of the corpus is the
    default dump, line for line, at every fusion level and float mode -- and it does add (every op line grows, the totals line is there)"""
    gs, modes = corpus_graphs(key), CORPUS[key][3]
    saved = marsrt.get_tuning("f32_mfma")
    try:
        for mode in modes:
            if mode is not None:
                marsrt.set_tuning("f32_mfma", mode)
            for level in (0, 1, 2):
                monkeypatch.setenv("MARS_HIP_FUSION", str(level))
                for gi, d in enumerate(gs):
                    for defer in (0, 1):
                        short, full = marsrt.describe_plan(d, flags=defer), marsrt.describe_plan(d, flags=defer | 2)
                        assert strip_full(full) == short, "graph %d mode %s level %d" % (gi, mode, level)
                        assert full[-1].startswith("+plan n_ops %d " % sum(l.startswith("op ") for l in short))
                        assert all(" | err " in l for l in full if l.startswith("op "))
    finally:
        marsrt.set_tuning("f32_mfma", saved)


def vcat_last_input_is_output():
    """a float C3-like graph: two 1 x 1 convolutions of the input -> CONCAT [1, 32, 8, 8] -> one 1 x 1 convolution, where the concat's LAST input
    is also a graph output.  virtual_concat_f32 would read that input through a view 32 bytes in front of it"""
    rng = np.random.default_rng(7)
    G = marsfile.Graph()
    F, NC = marsfile.F32, marsfile.NCHW

    def conv(t, ic, oc):
        w = G.tensor([oc, ic, 1, 1], dtype=F, fmt=marsfile.OIHW, data=((rng.random((oc, ic, 1, 1)) * 2 - 1) * 0.4).astype(np.float32))
        b = G.tensor([oc], dtype=F, fmt=marsfile.D1, data=((rng.random(oc) * 2 - 1) * 0.1).astype(np.float32))
        o = G.tensor([1, oc, 8, 8], dtype=F, fmt=NC)
        G.conv(t, o, w, b, (1, 1), (1, 1))
        return o

    x = G.tensor([1, 16, 8, 8], dtype=F, fmt=NC)
    a, b = conv(x, 16, 16), conv(x, 16, 16)
    cat = G.tensor([1, 32, 8, 8], dtype=F, fmt=NC)
    G.concat([a, b], cat, axis=1)
    r = conv(cat, 32, 16)
    return G.serialise([x], [r, b]), G.serialise([x], [r]), b


@pytest.mark.parametrize("mode", [3, 4])
def test_vcat_f32_keeps_graph_outputs_out_of_views(marsrt, monkeypatch, mode):
    """the hand-built case of the invariant above: with the concat's last input a graph output the concat is copied (no view); with the same
    graph minus that output it is read through a view of exactly that tensor (so the check is the only thing that differs)"""
    with_out, without, b = vcat_last_input_is_output()
    saved = marsrt.get_tuning("f32_mfma")
    try:
        marsrt.set_tuning("f32_mfma", mode)
        views = [l for l in marsrt.describe_plan(without) if " view=-" in l]
        assert len(views) == 1 and " in %d out " % b in views[0], views
        assert plan_violations(marsrt, with_out) == []
        assert not any(" view=-" in l for l in marsrt.describe_plan(with_out))
    finally:
        marsrt.set_tuning("f32_mfma", saved)
