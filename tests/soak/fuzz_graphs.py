"""Soak test (GPU box, through gpurun): random int8 NHWC graphs -- convolutions (1x1 / 3x3 / 5x5, stride 1 / 2, fused
ReLU, conv -> sigmoid -> mul chains), max-pools, ReLU family, sigmoid, add / mul, concats, 2x upsampling, with shared
inputs and several readers per tensor -- at fusion levels 0, 1 and 2, several frames, every graph output vs the oracle.
The graphs come from tests/graphgen.py (int8_graph): FUZZ_NCHW=1 / 0 makes every graph NCHW-tagged / NHWC, FUZZ_INTERIOR=1
draws the graph outputs from inside the graph, FUZZ_CHAIN=1 adds a chain of concats to the NCHW-tagged ones.
  python tests/soak/fuzz_graphs.py SEED N"""
import os, sys
import numpy as np
sys.path.insert(0, os.path.join(os.path.dirname(__file__), ".."))
sys.path.insert(0, os.path.join(os.path.dirname(__file__), "..", "..", "thingino-accel_amd"))
sys.path.insert(0, os.path.join(os.path.dirname(__file__), "..", "..", "oracle"))
import graphgen, marsfile, marsrt as gpu, orcbind as orc
from conftest import lcg_frame
gpu.nna_init()
rng = np.random.default_rng(int(sys.argv[1]) if len(sys.argv) > 1 else 0)
N = int(sys.argv[2]) if len(sys.argv) > 2 else 50
bad = 0
skipped = 0  # graphs whose shapes reach past the checker's allocations (orcbind.E_BOUNDS): nothing to compare against
NCHW = None if os.environ.get("FUZZ_NCHW") is None else os.environ["FUZZ_NCHW"] == "1"
OPTS = dict(interior_outputs=os.environ.get("FUZZ_INTERIOR") == "1", concat_chain=os.environ.get("FUZZ_CHAIN") == "1")


for it in range(N):
    r = graphgen.int8_graph(rng, nchw=NCHW, **OPTS)
    if r is None:
        continue
    d, desc = r
    hdr, tensors, _ = marsfile.parse(d)
    nb = marsfile.tensor_nbytes(tensors[hdr["inputs"][0]])
    B = int(rng.integers(1, 4))
    xs = [lcg_frame(0xF00D * 64 + 4 * it + f, nb) for f in range(B)]
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
    for level in (0, 1, 2):
        m = gpu.Model(d, batch=B, fusion=level)
        for f in range(B):
            m.input_view(0)[f] = xs[f]
        try:
            m.run()
        except gpu.MarsError as e:
            bad += 1
            print("RUN FAILED graph", it, "level", level, "batch", B, e, desc, flush=True)
            m.close()
            continue
        for f in range(B):
            for oi in range(len(hdr["outputs"])):
                if not np.array_equal(m.output_view(oi)[f], want[f][oi]):
                    bad += 1
                    print("MISMATCH graph", it, "level", level, "frame", f, "output", oi, desc, flush=True)
        m.close()
print("graph fuzz done:", N, "graphs,", skipped, "skipped (past the checker's allocations),", bad, "mismatches")
