#!/usr/bin/env python3
"""The launch plans (marsrt.describe_plan, plain and MARS_HIP_DESCRIBE_FULL) of a fixed corpus aimed at the fused int8 launch forms, as one text file:
the proof that a change to the planner's grouping code changed no plan.  Run it on two builds and compare the files (cmp).

Host only (no GPU, no oracle).  The corpus:
  - the four shipped files FILES under tests/golden/models/,
  - synthetic twins: widths 4 / 8 / 16 x every head kind x input 64 / 128 / 160 / 320 / 640, and the tiny / nchw_int8 / float32 / vary_scales variants,
  - the fusion sites of tests/edgecases.py (split, chain, pair, one-tile pair with its tails, C3 at both fusion levels) and of test_plan_both_cpu.py,
  - the site builders of the GPU fusion tests with their variants (built_sites): chain_site (sides, strides, tail c3, second= same / wide, d_add,
    d_out, d_is_output), both_site (cat None / up / flat x every tail x side, sides of 128, no half-step table), split_site (every tail),
    slices_site and c3_block (one and two bottlenecks, shortcut, slice_out),
  - 300 seeds of tests/graphgen.py, the generators in turn,
each under MARS_HIP_FUSION 0 / 1 / 2 and, at levels 1 and 2, with every MARS_HIP_NO_* switch set alone; float graphs under f32_mfma 3 (the mode that
forms float pairs), the rest under the default mode.

The tool counts the lines that carry each launch-group flag and fails when one of them never shows: a comparison of two dumps proves nothing about
a form the corpus does not hold.

usage: tools/plan_dump.py OUT.txt [JOBS]      -> prints the corpus size, the per-flag line counts and the SHA-256 of OUT.txt
"""
import hashlib
import multiprocessing
import os
import re
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "thingino-accel_amd"))

import numpy as np  # noqa: E402

import edgecases  # noqa: E402
import graphgen  # noqa: E402
import marsfile  # noqa: E402
import marsrt  # noqa: E402
import test_gpu_both_pair  # noqa: E402
import test_gpu_chain_fusion  # noqa: E402
import test_gpu_post_fusion  # noqa: E402
import test_gpu_split_fusion  # noqa: E402
import test_plan_both_cpu  # noqa: E402

FILES = ["yolov5n_int8", "yolov5nu", "tiny_160_int8", "tiny_160_f32"]
NO_SWITCHES = ["FUSE_LUT", "NHWC_INTERNAL", "VCONCAT_Q", "PAIR_F32", "REC", "ZERO_TAIL", "VCONCAT_F32", "ROWPAD", "POST", "SPLIT", "CHAIN", "BOTH", "BOTH_CHAIN"]
SETTINGS = [(level, None) for level in (0, 1, 2)] + [(level, "MARS_HIP_NO_" + s) for level in (1, 2) for s in NO_SWITCHES]
ENV = ["MARS_HIP_NO_" + s for s in NO_SWITCHES] + ["MARS_HIP_FUSION", "MARS_HIP_REC_LIMIT", "MARS_HIP_VCONCAT_LIMIT", "MARS_HIP_BOTTLENECK_LIMIT"]
SITES = ["split_s1", "split_s2", "split_chain1", "split_chain2", "pair", "both", "both_chain1_elided", "both_chain2_kept", "both_cat", "post_add", "post",
         "pre_add", "pre", "slice", "add3_c32", "add3_c128"]
GENERATORS = [(graphgen.int8_graph, dict(nchw=None)), (graphgen.int8_graph, dict(nchw=True)), (graphgen.int8_graph, dict(nchw=None, interior_outputs=True)),
              (graphgen.int8_graph, dict(nchw=True, interior_outputs=True, concat_chain=True)), (graphgen.f32_graph, dict()),
              (graphgen.vcat_f32_graph, dict(interior_outputs=True))]
SEEDS = 300
# (flag, pattern over one op line of the full dump): every launch form shows in at least one of them
FLAGS = [("pair_next", r"conv_i8 .* pair_next 1 "), ("pair_next of conv_f32", r"conv_f32 .* pair_next 1 "), ("pair_both", r" pair_both 1 "),
         ("both_chain 1", r" both_chain 1 "), ("both_chain 2", r" both_chain 2 "), ("both_elide", r" both_elide 1"), ("post_next", r" post_next 1 "),
         ("split_next", r" split_next 1 "), ("split_chain 1", r" split_chain 1 "), ("split_chain 2", r" split_chain 2 "), ("pre", r" pre 1 ")]


def is_float(d):
    hdr, tensors, _ = marsfile.parse(d)
    return any(tensors[t]["dtype"] == marsfile.F32 for t in hdr["inputs"])


def built_sites():
    """the sites the GPU fusion tests build, every option of their builders at least once -> (name, file bytes)"""
    chain, both, split, post = test_gpu_chain_fusion.chain_site, test_gpu_both_pair.both_site, test_gpu_split_fusion.split_site, test_gpu_post_fusion.c3_block
    for stride in (1, 2):
        for side in (1, 2):
            for tail in ("bare", "c3"):
                yield "chain:s%d,side%d,%s" % (stride, side, tail), chain(32, 31, 32, stride, stride - 1, seed=100 + stride + 10 * side, side=side, tail=tail)
    for side in (1, 2):
        for second in ("same", "wide"):
            yield "chain:second=%s,side%d" % (second, side), chain(32, 31, 32, 2, 0, seed=620 + side, side=side, second=second)
            yield "chain:second=%s,side%d,c3" % (second, side), chain(32, 31, 32, 2, 0, seed=625 + side, side=side, second=second, tail="c3")
        yield "chain:d_is_output,side%d" % side, chain(32, 31, 32, 2, 0, seed=640 + side, side=side, tail="c3", d_is_output=True)
        yield "chain:d_add,side%d" % side, chain(32, 31, 32, 2, 0, seed=610 + side, side=side, d_add=True)
        yield "chain:d_out64,side%d" % side, chain(32, 31, 32, 2, 0, seed=600 + side, side=side, d_out=64)
    for in_c in (16, 64):
        yield "chain:in_c%d" % in_c, chain(in_c, 31, 32, 2, 1, seed=400 + in_c)
    for in_c, cat in ((128, None), (256, "up"), (256, "flat")):
        for tail in ("outputs", "c3", "c3add"):
            yield "both:%d,%s,%s" % (in_c, cat, tail), both(in_c, 12, 12, seed=3000 + in_c, cat=cat, tail=tail)
        for side in (1, 2):
            for tail in ("chain", "chain_out", "chain_2nd"):
                yield "both:%d,%s,%s,side%d" % (in_c, cat, tail, side), both(in_c, 12, 12, seed=6500 + in_c + side, cat=cat, tail=tail, side=side)
    yield "both:oc128", both(256, 12, 12, seed=7000, oc=128)
    yield "both:oc128,flat", both(256, 12, 12, seed=7001, cat="flat", oc=128)
    yield "both:no_half_step_table", both(128, 12, 12, seed=4100, x_scale=0.04)
    for stride in (1, 2):
        for tail in ("outputs", "c3", "third", "t_out"):
            yield "split:s%d,%s" % (stride, tail), split(32, 31, 32, stride, 0, seed=100 + stride + len(tail), tail=tail)
    yield "split:below_the_fill_rule", split(32, 20, 20, 2, 0, seed=800)
    yield "split:slices", test_gpu_split_fusion.slices_site(31, 32, seed=700)
    for c in (32, 64):
        for n in (1, 2):
            for shortcut in (False, True):
                yield "c3_block:c%d,n%d,shortcut%d" % (c, n, shortcut), post(c, n, shortcut, 32, 32, seed=c + n + shortcut)
    yield "c3_block:slice_out", post(32, 1, True, 32, 32, seed=9, slice_out=True)


def corpus():
    """-> (name, file bytes)"""
    for n in FILES:
        yield "file:" + n, open(os.path.join(ROOT, "tests", "golden", "models", n + ".mars"), "rb").read()
    for w in (4, 8, 16):
        for head in sorted(marsrt.SYNTH_HEADS):
            for hw in (64, 128, 160, 320, 640):
                yield "twin:w=%d,head=%s,hw=%d" % (w, head, hw), marsrt.synth_model(width_x16=w, input_hw=hw, head=head)
        for variant in ("tiny", "nchw_int8", "float32", "vary_scales"):
            for hw in (160, 320):
                yield "twin:w=%d,%s,hw=%d" % (w, variant, hw), marsrt.synth_model(width_x16=w, input_hw=hw, **{variant: True})
    sites = edgecases.all_sites()
    for n in SITES:
        yield "site:" + n, sites[n]().d
    for oc, x_scale in ((32, 0.037), (64, 0.037), (64, 0.04), (128, 0.037)):
        yield "site:pair_graph_%d_%g" % (oc, x_scale), test_plan_both_cpu._pair_graph(oc, x_scale)
    for name, d in built_sites():
        yield "site:" + name, d
    for seed in range(SEEDS):
        gen, opt = GENERATORS[seed % len(GENERATORS)]
        rng = np.random.default_rng(7000 + seed)
        r = None
        while r is None:
            r = gen(rng, **opt)
        yield "graph:%d" % seed, r[0]


def dump(job):
    name, d = job
    for k in ENV:
        os.environ.pop(k, None)
    marsrt.set_tuning("f32_mfma", 3 if is_float(d) else 1)
    out = []
    for level, switch in SETTINGS:
        os.environ["MARS_HIP_FUSION"] = str(level)
        if switch:
            os.environ[switch] = "1"
        for flags in (0, marsrt.DESCRIBE_FULL):
            try:
                lines = marsrt.describe_plan(d, flags=flags)
            except ValueError:
                lines = ["(rejected)"]
            out.append("== %s fusion=%d %s flags=%d\n%s\n" % (name, level, switch or "-", flags, "\n".join(lines)))
        if switch:
            del os.environ[switch]
    return "".join(out)


def main():
    if len(sys.argv) not in (2, 3):
        sys.exit(__doc__)
    jobs = list(corpus())
    counts = dict.fromkeys((f for f, _ in FLAGS), 0)
    h = hashlib.sha256()
    with multiprocessing.Pool(int(sys.argv[2]) if len(sys.argv) == 3 else min(16, os.cpu_count() or 1)) as pool, open(sys.argv[1], "w") as out:
        for text in pool.imap(dump, jobs, chunksize=4):
            out.write(text)
            h.update(text.encode())
            for f, pat in FLAGS:
                counts[f] += len(re.findall(pat, text, re.M))
    print("%d corpus items x %d settings x 2 dumps = %d plans" % (len(jobs), len(SETTINGS), 2 * len(jobs) * len(SETTINGS)))
    for f, _ in FLAGS:
        print("  lines with %-22s %d" % (f, counts[f]))
    print("sha256 %s" % h.hexdigest())
    missing = [f for f, _ in FLAGS if not counts[f]]
    if missing:
        sys.exit("the corpus holds no launch with: " + ", ".join(missing))


if __name__ == "__main__":
    main()
