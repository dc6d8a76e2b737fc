"""Soak test (GPU box): the pipelined I/O path (mars_hip_pipe_*) on random graphs whose outputs sit inside the graph --
a concat's last input, a tensor other layers read, a convolution's input (tests/graphgen.py, interior_outputs).  The pipe hands every graph
input and output over in a per-slot buffer of its own, with nothing mapped in front of it.  Graphs in turn: int8 NHWC, int8 NCHW-tagged with a
chain of concats (concat_chain), float around the byte-wise concat under f32_mfma 3 and 4 (virtual_concat_f32).  Per graph: 4 batches of
different frames through Model.run(), then the same 4 batches through the pipe with download_outputs (at most 3 in flight, drained with
pipe_wait).  Every pipe output equals Model.run()'s on the same frames, and both equal the oracle: int8 bit for bit, float within
1e-4 * max(1, |b|) as fuzz_vcat_f32.py holds it (a graph whose plain plan, fusion level 0, is outside that is ill-conditioned for the split-bf16
arithmetic: counted, and only pipe against run compared).
  python tests/soak/fuzz_pipe.py SEED N"""
import os, sys, time
import numpy as np
sys.path.insert(0, os.path.join(os.path.dirname(__file__), ".."))
sys.path.insert(0, os.path.join(os.path.dirname(__file__), "..", "..", "thingino-accel_amd"))
sys.path.insert(0, os.path.join(os.path.dirname(__file__), "..", "..", "oracle"))
import graphgen, marsfile, marsrt as gpu, orcbind as orc
from conftest import lcg_frame
gpu.nna_init()
rng = np.random.default_rng(int(sys.argv[1]) if len(sys.argv) > 1 else 0)
N = int(sys.argv[2]) if len(sys.argv) > 2 else 30
K = 4  # batches per graph
bad = skipped = ill = views = 0
t0 = time.time()


def same(a, b, is_f32):
    if not is_f32:
        return np.array_equal(a, b)
    a, b = a.view(np.float32), b.view(np.float32)
    fin = np.isfinite(b) & (np.abs(b) < 1e6)
    return bool(np.all(np.abs(a - b) <= 1e-4 * np.maximum(1.0, np.abs(b)))) if fin.all() else True


def run_batches(d, frames, B, fusion=None):
    """Model.run() over K batches -> [batch][output] uint8 [B, frame_bytes]"""
    m = gpu.Model(d, batch=B) if fusion is None else gpu.Model(d, batch=B, fusion=fusion)
    res = []
    try:
        for k in range(len(frames) // B):
            for f in range(B):
                m.input_view(0)[f] = frames[k * B + f]
            m.run()
            res.append([m.output_view(oi).copy() for oi in range(m.header.num_outputs)])
    finally:
        m.close()
    return res


def pipe_batches(d, frames, B):
    """the same batches through the pipe: submit, wait once 3 are in flight, drain"""
    m = gpu.Model(d, batch=B)
    res = []
    try:
        m.pipe_open(download_outputs=True)
        inflight = 0
        for k in range(len(frames) // B):
            iv = m.pipe_input_view(0)
            for f in range(B):
                iv[f] = frames[k * B + f]
            m.pipe_submit()
            inflight += 1
            if inflight == 3:
                res.append(m.pipe_wait()[0]); inflight -= 1
        while inflight:
            res.append(m.pipe_wait()[0]); inflight -= 1
        m.pipe_close()
    finally:
        m.close()
    return res


for it in range(N):
    kind = it % 3
    if kind == 0:
        r = graphgen.int8_graph(rng, nchw=False, interior_outputs=True)
    elif kind == 1:
        r = graphgen.int8_graph(rng, nchw=True, interior_outputs=True, concat_chain=True)
    else:
        r = graphgen.vcat_f32_graph(rng, interior_outputs=True)
    if r is None:
        continue
    d, desc = r
    is_f32 = kind == 2
    mode = 3 + (it // 3) % 2 if is_f32 else 1
    gpu.set_tuning("f32_mfma", mode)
    hdr, tensors, _ = marsfile.parse(d)
    nb = marsfile.tensor_nbytes(tensors[hdr["inputs"][0]])
    B = int(rng.integers(1, 4))
    if is_f32:
        frames = [((np.random.default_rng(7000 * it + j).random(nb // 4) * 2 - 1) * 2).astype(np.float32).view(np.uint8) for j in range(K * B)]
        views += sum(" view=-" in l for l in gpu.describe_plan(d))
    else:
        frames = [lcg_frame(0xB1BE * 64 + 16 * it + j, nb) for j in range(K * B)]
    want = []
    for x in frames:
        g = orc.Graph(d); g.set_input(0, x.tobytes()); rc = g.run()
        if rc == orc.E_BOUNDS:
            break
        assert rc == 0, (rc, desc)
        want.append([g.tensor(ti).copy() for ti in hdr["outputs"]])
    if len(want) < len(frames):
        skipped += 1
        print("SKIPPED graph", it, "(past the checker's allocations)", desc, flush=True)
        continue
    tag = ("graph", it, "mode", mode, "batch", B, "outputs", hdr["outputs"], desc)
    try:
        ran = run_batches(d, frames, B)
        piped = pipe_batches(d, frames, B)
        plain = run_batches(d, frames[:B], B, fusion=0) if is_f32 else None
    except gpu.MarsError as e:
        bad += 1
        print("RUN FAILED", tag, e, flush=True)
        continue
    vs_oracle = True
    if plain is not None and not all(same(plain[0][oi][f], want[f][oi], True) for f in range(B) for oi in range(len(want[0]))):
        ill += 1
        vs_oracle = False
    for k in range(K):
        for f in range(B):
            for oi in range(len(hdr["outputs"])):
                a, p = ran[k][oi][f], piped[k][oi][f]
                if not same(p, a, is_f32):
                    bad += 1
                    print("PIPE != RUN", tag, "batch", k, "frame", f, "output", oi, flush=True)
                if vs_oracle and not (same(a, want[k * B + f][oi], is_f32) and same(p, want[k * B + f][oi], is_f32)):
                    bad += 1
                    print("MISMATCH vs oracle", tag, "batch", k, "frame", f, "output", oi, flush=True)
gpu.set_tuning("f32_mfma", 1)
print("pipe fuzz: %.1f s" % (time.time() - t0))
print("pipe fuzz done:", N, "graphs x", K, "batches,", ill, "ill-conditioned (pipe vs run only),", skipped,
      "skipped (past the checker's allocations),", views, "launches on a view,", bad, "mismatches")
