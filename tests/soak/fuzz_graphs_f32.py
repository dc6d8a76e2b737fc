"""Soak test (GPU box, through gpurun): random float32 NCHW graphs -- convolutions (1x1 / 3x3 / 5x5, stride 1 / 2, fused
ReLU byte clamp, conv -> sigmoid -> mul chains), byte-wise max-pools, LeakyReLU / ReLU, sigmoid, add / mul, batchnorm --
vs the oracle: bit for bit with f32_mfma = 0 (the reference's summation order), and within 1e-4 * max(1, |b|) under the
default policy (matrix cores wherever no byte-wise consumer follows), where a value that the reference itself lets run
away (|b| > 1e6 or non-finite) ends the comparison of that output.  The graphs come from tests/graphgen.py (f32_graph).
  python tests/soak/fuzz_graphs_f32.py SEED N"""
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
skipped = 0  # graphs whose shapes reach past the checker's allocations (orcbind.E_BOUNDS): nothing to compare against


for it in range(N):
    r = graphgen.f32_graph(rng)
    if r is None:
        continue
    d, desc = r
    hdr, tensors, _ = marsfile.parse(d)
    n_in = int(np.prod(tensors[hdr["inputs"][0]]["shape"]))
    B = int(rng.integers(1, 3))
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
    for mode in (0, 1):
        gpu.set_tuning("f32_mfma", mode)
        for level in (0, 1):
            m = gpu.Model(d, batch=B, fusion=level)
            for f in range(B):
                m.input_view(0)[f] = xs[f].view(np.uint8)
            try:
                m.run()
            except gpu.MarsError as e:
                bad += 1; print("RUN FAILED", it, mode, level, e, desc, flush=True); m.close(); continue
            for f in range(B):
                for oi in range(len(hdr["outputs"])):
                    a = m.output_view(oi)[f].view(np.float32); b = want[f][oi].view(np.float32)
                    if mode == 0:
                        ok = np.array_equal(a.view(np.uint32), b.view(np.uint32))
                    else:
                        fin = np.isfinite(b) & (np.abs(b) < 1e6)
                        ok = bool(np.all(np.abs(a[fin] - b[fin]) <= 1e-4 * np.maximum(1.0, np.abs(b[fin])))) if fin.all() else True
                    if not ok:
                        bad += 1
                        print("MISMATCH graph", it, "mode", mode, "level", level, "frame", f, "output", oi, desc, flush=True)
            m.close()
gpu.set_tuning("f32_mfma", 1)
print("f32 graph fuzz done:", N, "graphs,", skipped, "skipped (past the checker's allocations),", bad, "mismatches")
