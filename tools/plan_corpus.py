#!/usr/bin/env python3
"""The full plan dump (marsrt.describe_plan with DESCRIBE_FULL) of a fixed corpus of .mars graphs, as one text file: the proof that a change to the
planner changed no plan.  Run it on two builds and compare the files (cmp): equal files = the same launches, offsets, extents and work counts.

Host only (no GPU, no oracle).  The corpus:
  - the six shipped files under tests/golden/models/ that test_descriptor_only_ranks_plan_alike names,
  - synthetic twins: int8 and float32, input 640 and 320, width_x16 4 and 8,
  - every graph tests/test_plan_graphgen.py draws (its CORPUS table and generators, imported), and its hand-built view case,
each at fusion level 0 / 1 / 2, float graphs under f32_mfma 1 / 3 / 4, with and without the weight blob (flags 0 / 1);
  - the files and twins once more (levels 1 / 2) with every MARS_HIP_NO_* switch set alone and with MARS_HIP_REC_LIMIT lowered.

usage: tools/plan_corpus.py OUT.txt      -> prints the number of plans and the SHA-256 of OUT.txt
"""
import hashlib
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "thingino-accel_amd"))

import marsfile  # noqa: E402
import marsrt  # noqa: E402
import test_plan_graphgen as tg  # noqa: E402

SHIPPED = ["yolov5n_int8", "yolov5nu", "tiny_160_int8", "tiny_160_f32", "test_simple", "test_model"]
SWITCHES = [("MARS_HIP_NO_FUSE_LUT", "1"), ("MARS_HIP_NO_NHWC_INTERNAL", "1"), ("MARS_HIP_NO_VCONCAT_Q", "1"), ("MARS_HIP_NO_PAIR_F32", "1"),
            ("MARS_HIP_NO_REC", "1"), ("MARS_HIP_NO_ZERO_TAIL", "1"), ("MARS_HIP_NO_VCONCAT_F32", "1"), ("MARS_HIP_NO_ROWPAD", "1"),
            ("MARS_HIP_REC_LIMIT", str(1 << 20)), ("MARS_HIP_REC_LIMIT", str(1 << 16))]
ENV = sorted({k for k, _ in SWITCHES} | {"MARS_HIP_FUSION", "MARS_HIP_VCONCAT_LIMIT", "MARS_HIP_BOTTLENECK_LIMIT"})


def is_float(d):
    hdr, tensors, _ = marsfile.parse(d)
    return any(tensors[t]["dtype"] == marsfile.F32 for t in hdr["inputs"])


def corpus():
    """-> (name, file bytes, f32_mfma modes, with the switch sweep)"""
    for n in SHIPPED:
        d = open(os.path.join(ROOT, "tests", "golden", "models", n + ".mars"), "rb").read()
        yield "file:" + n, d, (1, 3, 4) if is_float(d) else (None,), True
    for f32 in (False, True):
        for hw in (640, 320):
            for w in (4, 8):
                yield "twin:f32=%d,hw=%d,w=%d" % (f32, hw, w), marsrt.synth_model(width_x16=w, input_hw=hw, seed=1, float32=f32), (1, 3, 4) if f32 else (None,), True
    for key in sorted(tg.CORPUS, key=str):
        for gi, d in enumerate(tg.corpus_graphs(key)):
            yield "graph:%s:%d" % ("-".join(str(v) for v in key), gi), d, tg.CORPUS[key][3], False
    with_out, without, _ = tg.vcat_last_input_is_output()
    yield "graph:vcat_last_input_is_output", with_out, (1, 3, 4), False
    yield "graph:vcat_last_input_not_output", without, (1, 3, 4), False


def main():
    if len(sys.argv) != 2:
        sys.exit(__doc__)
    for k in ENV:
        os.environ.pop(k, None)
    saved = marsrt.get_tuning("f32_mfma")
    plans = 0
    with open(sys.argv[1], "w") as out:
        def dump(name, d, mode, level, flags, switch=None):
            nonlocal plans
            os.environ["MARS_HIP_FUSION"] = str(level)
            if switch:
                os.environ[switch[0]] = switch[1]
            try:
                lines = marsrt.describe_plan(d, flags=flags | marsrt.DESCRIBE_FULL)
            except ValueError:
                lines = ["(rejected)"]
            finally:
                if switch:
                    del os.environ[switch[0]]
            out.write("== %s f32_mfma=%s fusion=%d flags=%d %s\n" % (name, mode, level, flags, "%s=%s" % switch if switch else "-"))
            out.write("\n".join(lines) + "\n")
            plans += 1

        try:
            for name, d, modes, sweep in corpus():
                for mode in modes:
                    if mode is not None:
                        marsrt.set_tuning("f32_mfma", mode)
                    for level in (0, 1, 2):
                        for flags in (0, 1):
                            dump(name, d, mode, level, flags)
                    if sweep:
                        for level in (1, 2):
                            for sw in SWITCHES:
                                dump(name, d, mode, level, 0, sw)
                marsrt.set_tuning("f32_mfma", saved)
        finally:
            marsrt.set_tuning("f32_mfma", saved)
    h = hashlib.sha256()
    with open(sys.argv[1], "rb") as f:
        for block in iter(lambda: f.read(1 << 20), b""):
            h.update(block)
    print("%d plans, sha256 %s" % (plans, h.hexdigest()))


if __name__ == "__main__":
    main()
