"""Soak test (GPU box, through gpurun): random float32 NCHW graphs around the reference's byte-wise CONCAT of equal maps -- 2 to 4 branches
(1x1 / 3x3 convolutions, chained byte-wise max-pools as in SPPF, the graph input itself) -> CONCAT in the exporter's form [1, sum C, H, W] -> one
1x1 convolution or two of the same shape (a C3's cv1 + cv2: one paired launch) -> sometimes a k x k convolution behind (record-format pairs) --
under the split-bf16 modes (f32_mfma 3 / 4), where the planner cuts the readers' K loops (zero_tail_f32) and, for map widths that are multiples
of 4, never materialises the concat (virtual_concat_f32: a view of the last input + a head launch).  Every graph output against the oracle
within 1e-4 * max(1, |b|), with the passes on and with MARS_HIP_NO_VCONCAT_F32, wherever the plain plan (fusion level 0) is inside it; several frames.
The graphs come from tests/graphgen.py (vcat_f32_graph).
  python tests/soak/fuzz_vcat_f32.py SEED N"""
import os, sys
import numpy as np
sys.path.insert(0, os.path.join(os.path.dirname(__file__), ".."))
sys.path.insert(0, os.path.join(os.path.dirname(__file__), "..", "..", "thingino-accel_amd"))
sys.path.insert(0, os.path.join(os.path.dirname(__file__), "..", "..", "oracle"))
import graphgen, marsfile, marsrt as gpu, orcbind as orc
gpu.nna_init()
rng = np.random.default_rng(int(sys.argv[1]) if len(sys.argv) > 1 else 0)
N = int(sys.argv[2]) if len(sys.argv) > 2 else 50
bad = 0
views = 0
skipped = 0  # graphs whose shapes reach past the checker's allocations (orcbind.E_BOUNDS): nothing to compare against


def run_all(d, xs, want, tag, fusion):
    """-> mismatching (frame, output) pairs, or -1 when the run failed"""
    hdr = marsfile.parse(d)[0]
    m = gpu.Model(d, batch=len(xs), fusion=fusion)
    for f in range(len(xs)):
        m.input_view(0)[f] = xs[f].view(np.uint8)
    try:
        m.run()
    except gpu.MarsError as e:
        print("RUN FAILED", tag, e, flush=True); m.close(); return -1
    n = 0
    for f in range(len(xs)):
        for oi in range(len(hdr["outputs"])):
            a = m.output_view(oi)[f].view(np.float32); b = want[f][oi].view(np.float32)
            fin = np.isfinite(b) & (np.abs(b) < 1e6)
            if fin.all() and not bool(np.all(np.abs(a - b) <= 1e-4 * np.maximum(1.0, np.abs(b)))):
                n += 1
                if fusion:
                    print("MISMATCH", tag, "frame", f, "output", oi, "worst", float(np.max(np.abs(a - b) / np.maximum(1.0, np.abs(b)))), flush=True)
    m.close()
    return n


ill = 0
for it in range(N):
    d, desc = graphgen.vcat_f32_graph(rng)
    hdr, tensors, _ = marsfile.parse(d)
    n_in = int(np.prod(tensors[hdr["inputs"][0]]["shape"]))
    B = int(rng.integers(1, 4))
    xs = [((np.random.default_rng(1000 * it + f).random(n_in) * 2 - 1) * 2).astype(np.float32) for f in range(B)]
    want = []
    for f in range(B):
        g = orc.Graph(d); g.set_input(0, xs[f].tobytes()); rc = g.run()
        if rc == orc.E_BOUNDS:
            break
        assert rc == 0, (rc, desc)
        want.append([g.tensor(ti).copy() for ti in hdr["outputs"]])
    if len(want) < B:
        skipped += 1
        print("SKIPPED graph", it, "(past the checker's allocations)", desc, flush=True)
        continue
    for mode in (3, 4):
        gpu.set_tuning("f32_mfma", mode)
        os.environ.pop("MARS_HIP_NO_VCONCAT_F32", None)
        # the plain plan first (fusion level 0: one launch per layer, every concat copied, full K loops).  Where THAT is outside the tolerance the
        # graph is ill-conditioned for the split-bf16 arithmetic (floats spliced or max-ed byte-wise reach 1e38 and cancel: runs of 6 or 10 bytes,
        # the pools of the SPPF form) and says nothing about the passes: counted, not compared
        r0 = run_all(d, xs, want, ("graph", it, "mode", mode, "unfused", desc), 0)
        if r0 != 0:
            bad += r0 < 0
            ill += r0 > 0
            continue
        views += sum(" view=-" in l for l in gpu.describe_plan(d))
        r = run_all(d, xs, want, ("graph", it, "mode", mode, "virtual", desc), 1)
        bad += abs(r)
        os.environ["MARS_HIP_NO_VCONCAT_F32"] = "1"
        r = run_all(d, xs, want, ("graph", it, "mode", mode, "copied", desc), 1)
        bad += abs(r)
        os.environ.pop("MARS_HIP_NO_VCONCAT_F32", None)
gpu.set_tuning("f32_mfma", 1)
print("f32 concat fuzz done:", N, "graphs x 2 modes,", ill, "ill-conditioned (skipped),", skipped, "skipped (past the checker's allocations),", views, "launches on a view,", bad, "mismatches")
