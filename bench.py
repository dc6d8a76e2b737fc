#!/usr/bin/env python3
"""Benchmark of the mars_runtime hot path on MI355X.

A "step" = one pass of the whole hot path over one batch of synthetic frames that are
already resident in HBM: every layer of the .mars graph (int8 MFMA conv + fused requant /
SiLU-LUT epilogue, pooling, concat, upsample, add) and the decode + NMS detection tail.

Workload at N=1 = the configuration BASELINE.json's metric is quoted on: yolov5s_int8,
640x640, batch 256.  The reference repo does not ship that file (.MISSING_LARGE_BLOBS), so it
is the seeded synthetic twin written by mars_synth_model() (same format, same YOLOv5s layer
sequence, NHWC/OHWI int8).  N>1: one process per GPU (torch.distributed.run), frames sharded,
parameters broadcast once over RCCL, no collective in the forward pass.  Frames per GPU: 256 at
every N (weak scaling) -- except the default N=8 run, which is BASELINE config 4: 1024 frames in
total = 128 per GPU (`--weak` keeps 256 per GPU there too; `--total-batch T` asks for any total).

Prints ONE JSON line (rank 0).  `roofline` is for the dominant kernel (conv_i8_kernel, the
implicit-GEMM MFMA convolution): algorithmic bytes (and, as `mfma_view`, int8 ops) of all its launches / their summed
duration, measured with HIP events on the library's stream inside the timed region.
`roofline.frac_wall` puts the same algorithmic bytes over `ms_per_step` (the execution mode of `value`: two
half-batches on two streams).  `cpu_baseline` is the reference's own C code (oracle/_ref, -O3 -funroll-loops as in
its Makefile:21) on one host core over a bounded sample (as many frames of the same workload as fit in ~14 s, at most
16); the GPU's head tensors AND its detections (kept boxes, order, classes: the reference's parse_output + nms on
the reference's head tensors) for those frames are compared with it bit for bit (`map_delta`).
`sustained_images_per_s` = >= 3 s of back-to-back steps after the timed region, with the shader clock the chip held.
`roofline.copy_rate_measured` / `frac_of_copy_rate`: what a plain 1 GiB device copy reaches on the same box (read + write),
and the conv family's byte rate against it -- beside `frac`, which stays against the guide's 8 TB/s; `frac_of_achievable`
holds it against the guide's measured 6.3 TB/s.  `roofline.pipes`: per step, the time each pipe (matrix, vector, scalar, LDS,
HBM) would need alone, from the committed instruction-mix profile of the same kernel sources (which one binds the family).
`--io pipelined` (any N): every rank also feeds its frames from pinned host memory through mars_hip_pipe_* and reports
the I/O-inclusive rate (MAX over ranks), the first thing an 8-GPU run is bound by.

A plain run (`bench.py --gpus N --steps K --warmup W`) is lean: set-up, W warm-up steps, the K timed steps (with the
roofline's HIP events in the last of them, as always), `--dump-outputs` if asked, the line.  Everything else above -- the
sustained leg, the pipelined-I/O, PCIe-inclusive, graph-only and batch-1 legs, the CPU baselines and their parity checks,
the copy-rate probe with `roofline.pipes`, and the other BASELINE configs (`configs`) -- runs only with `--full`.  Legs asked
for by name (`--io pipelined|camera`, `--sustain-s S`) run either way.
`--dump-outputs DIR`: what the timed path computed in its last step, as float32 .npy files (dump_outputs() lists them).
"""
import hashlib
import argparse
import importlib.util
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(ROOT, "tests"))


def load_marsrt():
    spec = importlib.util.spec_from_file_location("marsrt", os.path.join(ROOT, "thingino-accel_amd", "marsrt.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def load_probe():
    """bench.py's measurement probes (copy rate, shader clock): thingino-accel_amd/lib/libmars_probe.so, NOT part of the product
    library (csrc/probe/mars_probe.hip)"""
    import ctypes as C
    L = C.CDLL(os.path.join(ROOT, "thingino-accel_amd", "lib", "libmars_probe.so"))
    L.mars_probe_copy_rate_gbs.restype = C.c_double
    L.mars_probe_copy_rate_gbs.argtypes = [C.c_size_t, C.c_int]
    L.mars_probe_copy_form.restype = C.c_char_p
    L.mars_probe_clock_mhz.restype = C.c_float
    L.mars_probe_clock_mhz.argtypes = [C.c_int]
    return L


def pipe_times(args, conv_bytes, copy_gbs, clock_mhz):
    """Which pipe binds the conv family, per step, from the committed instruction-mix pass of the same workload and the same
    kernel sources (profiles/inst_mix.json, tools/inst_mix.py --json; None when no matching profile exists): the time each
    pipe would need if it ran alone at full rate -- 1024 SIMDs / 256 CUs at the shader clock the sustained leg measured
    (else 2400 MHz): a v_mfma_i32_16x16x64_i8 holds its SIMD's matrix pipe 16 cycles, any other vector instruction its
    issue port 4, a scalar instruction its CU's scalar unit 1 (lower bound), LDS = the cycles the LDS arrays were
    indexing; HBM = the algorithmic bytes at 8 TB/s, at the guide's achievable 6.3 TB/s, and at this box's copy rate."""
    path = os.path.join(ROOT, "profiles", "inst_mix.json")
    hbm = {"hbm_ms_at_peak": conv_bytes / 8e12 * 1e3, "hbm_ms_at_achievable": conv_bytes / 6.3e12 * 1e3,
           "hbm_ms_at_copy_rate": conv_bytes / (copy_gbs * 1e9) * 1e3 if copy_gbs and copy_gbs > 0 else None}
    try:
        with open(path) as fh:
            d = json.load(fh)
        if d["config"] != {"width": args.width, "hw": args.hw, "batch": args.batch}:
            return dict(hbm, source="profiles/inst_mix.json is for another workload")
        if d.get("kernel_source_sha16") != kernel_source_sha16():
            return dict(hbm, source="profiles/inst_mix.json was taken with other kernel sources (%s, now %s)" % (d.get("kernel_source_sha16"), kernel_source_sha16()))
        c = d["conv_i8_per_step"]
        clk = (clock_mhz or 2400.0) * 1e6
        out = {"mfma_ms": c["mfma"] * 16 / (1024 * clk) * 1e3, "valu_ms": (c["valu"] - c["mfma"]) * 4 / (1024 * clk) * 1e3,
               "salu_ms": c["salu"] / (256 * clk) * 1e3,
               "lds_ms": c["lds_idx_active_cycles"] / (256 * clk) * 1e3 if c.get("lds_idx_active_cycles") else None,
               "valu_per_mfma": (c["valu"] - c["mfma"]) / c["mfma"], "salu_per_mfma": c["salu"] / c["mfma"],
               "clock_mhz_assumed": clk / 1e6,
               "source": "profiles/inst_mix.json (kernel sources %s)" % d["kernel_source_sha16"]}
        out.update(hbm)
        return out
    except (OSError, KeyError, ValueError, ZeroDivisionError):
        return dict(hbm, source=None)


def load_dist_helpers():
    spec = importlib.util.spec_from_file_location("mdist", os.path.join(ROOT, "thingino-accel_amd", "dist.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def frames_for_rank(D, rank, world, per_gpu, nbytes, f32=False):
    from conftest import lcg_frame
    if f32:  # uniform [0, 1) floats from the same LCG
        import cases
        return [cases.f32(0x5EED0000 + f, nbytes // 4, 0.0, 1.0).view(np.uint8) for f in D.shard_frames(per_gpu, rank, world)]
    return [lcg_frame(0x5EED0000 + f, nbytes) for f in D.shard_frames(per_gpu, rank, world)]


def cpu_baseline(model_bytes, frames, out_ids, budget_s=14.0, max_frames=16, file_model=False, on_frame=None):
    """rank 0, N=1 only: the reference's own C (or, failing that, this repo's port) on ONE host
    core over a bounded sample of the same workload: as many frames as fit in ~budget_s seconds.
    Returns (record, per-frame outputs) so the GPU results for those frames can be compared."""
    sys.path.insert(0, os.path.join(ROOT, "oracle"))
    # (a shipped file reads / writes past some tensors' nominal extent: the harness's wide default slack)
    kw = {} if file_model else dict(slack_mult=1, slack_add=4096)
    runner, kind, how = None, "port", "oracle/restate (gcc -O2)"
    try:
        import refbind
        if refbind.available():
            runner = refbind.O2Model(model_bytes, fast=True, **kw)
            kind, how = "reference", "the reference's own layer functions (oracle/_ref, gcc -O3 -funroll-loops)"
    except Exception:  # noqa: BLE001
        runner = None
    if runner is None:
        import orcbind
        runner = orcbind.Graph(model_bytes, **kw)
    outs, spent, n = [], 0.0, 0
    while n < min(max_frames, len(frames)) and (n == 0 or spent + spent / n <= budget_s):
        if n:
            runner.close()
            runner = (refbind.O2Model(model_bytes, fast=True, **kw) if kind == "reference"
                      else orcbind.Graph(model_bytes, **kw))  # fresh zeroed tensors per frame
        runner.set_input(0, frames[n].tobytes())
        t0 = time.time()
        rc = runner.run()
        spent += time.time() - t0
        if rc != 0:
            raise RuntimeError("cpu baseline run failed: %d" % rc)
        outs.append([runner.tensor(ti) for ti in out_ids])
        if on_frame is not None:  # --model: the caller compares every activation tensor of the frame while the run is held
            on_frame(runner, n)
        n += 1
    runner.close()
    return dict(value=n / spent, unit="images/s", cores=1, kind=kind,
                sample="%d frames of the same workload through %s, %.1f s of CPU time" % (n, how, spent)), outs


def cpu_baseline_parallel(model_bytes, frames, out_ids, nthreads, ref_outs, f32=False, file_model=False):
    """the same reference code, frames-parallel: one frame per thread, every host core this process may use (ctypes
    releases the GIL; every thread owns its model instance).  One frame per thread, so ~one single-frame time."""
    import threading
    sys.path.insert(0, os.path.join(ROOT, "oracle"))
    # every core this process may use, but no more threads than keep the leg near one single-frame time: beyond ~64 the
    # reference's scalar loops share memory bandwidth (256 threads: 8x one core on the int8 twin), and a float32 frame is
    # 35 s alone (256 at once: 260 s)
    cap = 16 if f32 else 64
    n = nthreads or min(len(os.sched_getaffinity(0)), cap)
    n = max(1, min(n, len(frames)))
    kind = "port"
    try:
        import refbind
        use_ref = refbind.available()
    except Exception:  # noqa: BLE001
        use_ref = False
    kw = {} if file_model else dict(slack_mult=1, slack_add=4096)
    if use_ref:
        kind = "reference"
        mk = lambda: refbind.O2Model(model_bytes, fast=True, **kw)  # noqa: E731
    else:
        import orcbind
        mk = lambda: orcbind.Graph(model_bytes, **kw)  # noqa: E731
    runners = [mk() for _ in range(n)]
    for i, r in enumerate(runners):
        r.set_input(0, frames[i].tobytes())
    rcs = [None] * n
    th = [threading.Thread(target=lambda i=i: rcs.__setitem__(i, runners[i].run())) for i in range(n)]
    t0 = time.time()
    for t in th:
        t.start()
    for t in th:
        t.join()
    dt = time.time() - t0
    if any(rc != 0 for rc in rcs):
        raise RuntimeError("parallel cpu baseline failed: %r" % (rcs,))
    same = all(np.array_equal(runners[f].tensor(ti), ref_outs[f][i]) for f in range(min(n, len(ref_outs))) for i, ti in enumerate(out_ids))
    for r in runners:
        r.close()
    return dict(value=n / dt, unit="images/s", cores=n, host_cores=len(os.sched_getaffinity(0)), kind=kind, matches_single_core_run=bool(same),
                sample="%d frames at once, one per thread, %.1f s wall" % (n, dt))


def input_hw_of(t):
    """(H, W) of a graph input by its format tag (NHWC = 7: [N, H, W, C]; anything else is read as NCHW: reference mars_runtime.c:561-562)"""
    sh = list(t["shape"]) + [1, 1, 1, 1]
    return (sh[1], sh[2]) if t["fmt"] == 7 else (sh[2], sh[3])


def synth_frames(first, n, nbytes, f32):
    """frame f = LCG(seed 0x5EED0000 + f) bytes (int8 inputs) or uniform [0, 1) floats from the same LCG (f32 inputs)"""
    from conftest import lcg_frame
    import cases
    if f32:
        return [cases.f32(0x5EED0000 + f, nbytes // 4, 0.0, 1.0).view(np.uint8) for f in range(first, first + n)]
    return [lcg_frame(0x5EED0000 + f, nbytes) for f in range(first, first + n)]


def reference_runner(model_bytes, file_model):
    """the reference's own layer functions on a private arena (oracle/_ref, -O3 -funroll-loops), else this repo's restatement;
    shipped files get the wide slack their out-of-tensor reads / writes need"""
    sys.path.insert(0, os.path.join(ROOT, "oracle"))
    kw = {} if file_model else dict(slack_mult=1, slack_add=4096)
    try:
        import refbind
        if refbind.available():
            return refbind.O2Model(model_bytes, fast=True, **kw), "reference"
    except Exception:  # noqa: BLE001
        pass
    import orcbind
    return orcbind.Graph(model_bytes, **kw), "port"


def compare_frame(model, runner, tensors, out_ids, frame, f32, every_tensor):
    """GPU frame `frame` against the CPU run held by `runner`: graph outputs, and (every_tensor) every activation tensor the plan keeps
    in HBM.  int8: bit for bit; f32: |a - b| <= 1e-4 * max(1, |b|).  -> (tensors compared, tensors equal, worst relative error)"""
    def same(a, b):
        if not f32:
            return bool(np.array_equal(a, b)), 0.0
        x, y = a.view(np.float32).astype(np.float64), b.view(np.float32).astype(np.float64)
        if (np.isnan(x) != np.isnan(y)).any() or (np.isinf(x) != np.isinf(y)).any():
            return False, float("inf")
        bad = ~((np.isnan(x) & np.isnan(y)) | (x == y))
        if not bad.any():
            return True, 0.0
        err = float((np.abs(x - y)[bad] / np.maximum(1.0, np.abs(y)[bad])).max())
        return err <= 1e-4, err
    n = ok = 0
    worst = 0.0
    for i, ti in enumerate(out_ids):
        e, w = same(model.output_view(i)[frame], runner.tensor(ti))
        n += 1
        ok += int(e)
        worst = max(worst, w)
    if every_tensor:
        import marsfile
        for ti, t in enumerate(tensors):
            if t["size"] != 0 or not marsfile.tensor_nbytes(t) or ti in out_ids:
                continue
            try:
                got = model.read_tensor(ti, frame=frame)
            except Exception:  # noqa: BLE001  (elided by a fusion pass, or written by no layer: not in HBM)
                continue
            e, w = same(got, runner.tensor(ti)[:len(got)])
            n += 1
            ok += int(e)
            worst = max(worst, w)
    return n, ok, worst


DUMP_BUDGET = 64 * 10 ** 6  # bytes, all files of one --dump-outputs together
DUMP_SEED = 0x5EED


def dump_outputs(model, tensors, out_ids, detect, outdir):
    """--dump-outputs DIR: what a caller of the timed path receives for its last step, as float32 .npy files --
    output<i>.npy: graph output i (the head tensor bytes as int8, or float32 for a float graph) of the frames in frames.npy,
    [frames, values]; every frame when the budget allows, else a sample of frames drawn with a fixed seed (if not even one
    frame fits: a seeded sample of each output's values of frame 0, their indices in output<i>_index.npy);
    detections.npy (tail on): the kept boxes of every frame, rows (frame, x, y, w, h, conf, cls) in the library's order.
    Inputs and the sample depend only on the arguments, so two builds can be compared file for file."""
    os.makedirs(outdir, exist_ok=True)
    model.download()
    batch = model.batch
    files = {}
    if detect:
        dets = model.detect(outputs=tuple(range(len(out_ids))), thresh=0.45)
        rows = [np.column_stack([np.full(len(d), f, np.float32)] + [d[k].astype(np.float32) for k in ("x", "y", "w", "h", "conf", "cls")])
                for f, d in enumerate(dets) if len(d)]
        files["detections"] = np.concatenate(rows) if rows else np.zeros((0, 7), np.float32)
    heads = [model.output_view(i).view(np.float32 if tensors[ti]["dtype"] == 0 else np.int8) for i, ti in enumerate(out_ids)]
    left = DUMP_BUDGET - sum(a.nbytes for a in files.values()) - 4096
    per_frame = sum(h.shape[1] for h in heads) * 4
    rng = np.random.default_rng(DUMP_SEED)
    keep = min(batch, left // per_frame) if per_frame else batch
    if keep >= 1:
        frames = np.arange(batch) if keep == batch else np.sort(rng.choice(batch, keep, replace=False))
        for i, h in enumerate(heads):
            files["output%d" % i] = h[frames].astype(np.float32)
    else:
        frames = np.zeros(1, np.int64)
        for i, h in enumerate(heads):
            n = min(h.shape[1], max(1, left * h.shape[1] * 4 // per_frame // 12))  # value (float32) + index (float64): 12 bytes
            idx = np.sort(rng.choice(h.shape[1], n, replace=False))
            files["output%d" % i] = h[0, idx].astype(np.float32)[None]
            files["output%d_index" % i] = idx.astype(np.float64)
    files["frames"] = frames.astype(np.float64)
    for name, a in files.items():
        np.save(os.path.join(outdir, name + ".npy"), a)


def short_leg(M, name, model_bytes, batch, steps, warmup, tail, f32_mode=None, cpu_frames=1, file_model=False, what=""):
    """One short leg of another BASELINE config under the same clock as the headline: its own model instance, frames resident in
    HBM, `warmup` + `steps` steps between synchronisations, one further step with HIP events around the convolution launches (one
    stream) for the roofline, then `cpu_frames` frames compared with the reference's CPU run.  -> a compact dict."""
    import marsfile
    hdr, tensors, _ = marsfile.parse(model_bytes)
    tin = tensors[hdr["inputs"][0]]
    f32 = tin["dtype"] == 0
    nb = marsfile.tensor_nbytes(tin)
    out_ids = list(hdr["outputs"])
    saved_mode = M.get_tuning("f32_mfma")
    if f32 and f32_mode is not None:
        M.set_tuning("f32_mfma", f32_mode)
    t_all = time.perf_counter()
    try:
        model = M.Model(model_bytes, batch=batch)
        frames = synth_frames(0, batch, nb, f32)
        iv = model.input_view(0)
        for f in range(batch):
            iv[f, :nb] = frames[f]
        model.upload()
        outputs = tuple(range(len(out_ids)))
        tail = tail and not f32

        def step():
            model.run_device(sync=False)
            if tail:
                model.detect_device(outputs=outputs, thresh=0.45)
        for _ in range(warmup):
            step()
        M.lib().mars_hip_sync()
        # three windows of `steps` steps, the MEDIAN one reported: a leg is a few tens of milliseconds long, and one stall (the previous leg's
        # buffers still being released, a clock step) moved a single window by 10 % on some boxes.  All three are in the line.
        windows = []
        for _ in range(3):
            t0 = time.perf_counter()
            for _ in range(steps):
                step()
            M.lib().mars_hip_sync()
            windows.append(time.perf_counter() - t0)
        dt = sorted(windows)[1]
        model.set_profiling(2)
        step()
        M.lib().mars_hip_sync()
        ops = model.ops()
        model.set_profiling(0)
        ckind = 1 if f32 else 0
        conv_ms = sum(o["ms"] for o in ops if o["kind"] == ckind)
        conv_bytes = sum(o["bytes"] for o in ops if o["kind"] == ckind) * batch
        conv_flop = sum(2.0 * o["macs"] for o in ops if o["kind"] == ckind) * batch
        mode = M.get_tuning("f32_mfma")
        mpeak = (2.5e15 / 3.0 if mode == 3 else 2.5e15 / 6.0 if mode == 4 else 157.3e12) if f32 else 5e15
        hbm_floor, mfma_floor = conv_bytes / 8e12, conv_flop / mpeak
        bound = "hbm" if hbm_floor >= mfma_floor else "mfma"  # the roof that is nearer: whichever floor is higher
        rec = {"workload": what, "value": batch * steps / dt, "unit": "images/s", "ms_per_step": dt / steps * 1e3, "steps": steps, "warmup": warmup,
               "batch": batch, "dtype": ("f32 (f32_mfma mode %d)" % mode) if f32 else "int8", "tail": bool(tail),
               "bound": bound, "frac": (max(hbm_floor, mfma_floor) / (conv_ms * 1e-3)) if conv_ms > 0 else None,
               "frac_hbm": (hbm_floor / (conv_ms * 1e-3)) if conv_ms > 0 else None, "frac_mfma": (mfma_floor / (conv_ms * 1e-3)) if conv_ms > 0 else None,
               "frac_wall": max(hbm_floor, mfma_floor) / (dt / steps),
               "conv_ms_per_step": conv_ms, "conv_launches": sum(1 for o in ops if o["kind"] == ckind),
               "conv_gmac_per_image": conv_flop / 2e9 / batch, "conv_algorithmic_mb_per_image": conv_bytes / 1e6 / batch,
               "windows_ms_per_step": [w / steps * 1e3 for w in windows],
               "timing": "value: wall clock around %d steps, the median of three such windows (the library's execution mode at this batch); frac: HIP events, one stream, one further step" % steps}
        if cpu_frames > 0:
            model.download()
            n = ok = 0
            worst = 0.0
            kind = None
            tc = time.perf_counter()
            picks = sorted(set([0, batch - 1][:cpu_frames])) if cpu_frames <= 2 else list(range(min(cpu_frames, batch)))
            dets_ok = None
            gdets = model.detect(outputs=outputs, thresh=0.45) if tail else None
            for f in picks:
                runner, kind = reference_runner(model_bytes, file_model)
                runner.set_input(0, frames[f].tobytes())
                rc = runner.run()
                if rc != 0:
                    raise RuntimeError("%s: cpu reference run failed: %d" % (name, rc))
                a, b, w = compare_frame(model, runner, tensors, out_ids, f, f32, every_tensor=file_model)
                n += a
                ok += b
                worst = max(worst, w)
                if tail:
                    want = reference_detections([runner.tensor(ti) for ti in out_ids], [float(tensors[ti]["scale"]) for ti in out_ids])
                    dets_ok = (dets_ok is not False) and gdets[f].tobytes() == want.tobytes()
                runner.close()
            rec["parity"] = {"ok": bool(n > 0 and ok == n and dets_ok is not False), "frames": picks, "tensors_compared": n, "tensors_equal": ok, "cpu": kind,
                             "rule": "|a-b| <= 1e-4*max(1,|b|)" if f32 else "bit-exact", "cpu_seconds": time.perf_counter() - tc}
            if f32:
                rec["parity"]["worst_relative_error"] = worst
            if dets_ok is not None:
                rec["parity"]["detections_bit_exact"] = bool(dets_ok)
        model.close()
    finally:
        M.set_tuning("f32_mfma", saved_mode)
    rec["leg_seconds"] = time.perf_counter() - t_all
    return rec


def extra_configs(M, args):
    """BASELINE.json's other configs (and north_star's 320 x 320 frames) as short legs beside the headline, so that the driver's one
    default run observes them: separate model instances, after the headline's timed region and every leg of it.  Sized from the
    headline's own arguments (default: 640 x 640, batch 256), so the small test invocation runs small legs."""
    hw, b = args.hw, args.batch
    st, wu = max(3, min(args.steps, 12)), max(1, min(args.warmup, 3))
    cpu = 0 if args.no_cpu_baseline else 1
    gold = os.path.join(ROOT, "tests", "golden", "models")
    legs = []
    legs.append(("config3_yolov5n_int8", dict(width_x16=4, input_hw=hw), dict(batch=b, tail=True, cpu_frames=2 * cpu),
                 "synthetic yolov5n_int8 twin (width_x16=4), %dx%d, batch %d, decode+NMS on" % (hw, hw, b)))
    legs.append(("config3_shipped_yolov5n_int8_mars", os.path.join(gold, "yolov5n_int8.mars"), dict(batch=b, tail=False, cpu_frames=cpu),
                 "the reference's own models/yolov5n_int8.mars (NCHW-tagged: conv2d_int8_mxu path, mxu_conv.c:630-670), 640x640, batch %d, graph only "
                 "(its head tensors have shape [0,0,0,0]: the file's tail is all no-ops, SURVEY App. C)" % b))
    legs.append(("config5_yolov5s_float32", dict(width_x16=args.width, input_hw=hw, float32=True), dict(batch=b, tail=False, cpu_frames=cpu, f32_mode=3),
                 "synthetic yolov5s_float32 twin (width_x16=%d), %dx%d, batch %d, graph only, f32_mfma mode 3" % (args.width, hw, hw, b)))
    legs.append(("yolov5s_int8_%d" % (hw // 2), dict(width_x16=args.width, input_hw=hw // 2), dict(batch=b, tail=True, cpu_frames=2 * cpu),
                 "synthetic yolov5s_int8 twin (width_x16=%d), %dx%d, batch %d, decode+NMS on" % (args.width, hw // 2, hw // 2, b)))
    legs.append(("yolov5n_int8_%d" % (hw // 2), dict(width_x16=4, input_hw=hw // 2), dict(batch=b, tail=True, cpu_frames=2 * cpu),
                 "synthetic yolov5n_int8 twin (width_x16=4), %dx%d, batch %d, decode+NMS on" % (hw // 2, hw // 2, b)))
    legs.append(("config2_tiny_160_int8_mars", os.path.join(gold, "tiny_160_int8.mars"), dict(batch=min(64, b), tail=False, cpu_frames=2 * cpu),
                 "the reference's own models/tiny_160_int8.mars, 160x160, batch %d" % min(64, b)))
    out = {}
    for name, src, kw, what in legs:
        if isinstance(src, dict) and (src["input_hw"] % 32 or src["input_hw"] < 64):
            out[name] = {"workload": what, "skipped": "the twins need a frame size that is a multiple of 32"}
            continue
        try:
            if isinstance(src, dict):
                mb = M.synth_model(seed=1, **src)
                out[name] = short_leg(M, name, mb, steps=st, warmup=wu, what=what, **kw)
            else:
                with open(src, "rb") as fh:
                    mb = fh.read()
                out[name] = short_leg(M, name, mb, steps=st, warmup=wu, what=what, file_model=True, **kw)
        except Exception as e:  # noqa: BLE001  (a failing leg must not cost the headline its line)
            out[name] = {"workload": what, "error": "%s: %s" % (type(e).__name__, e)}
    return out


def kernel_source_sha16():
    """sha256 (first 16 hex digits) over the device sources: ties a committed PMC profile to the kernels it profiled"""
    h = hashlib.sha256()
    d = os.path.join(ROOT, "thingino-accel_amd", "csrc", "hip")
    for f in sorted(os.listdir(d)):
        if f.endswith((".hip", ".hpp", ".h")):
            with open(os.path.join(d, f), "rb") as fh:
                h.update(f.encode() + b"\0" + fh.read())
    return h.hexdigest()[:16]


def pmc_traffic(args):
    """HBM bytes one step's conv launches move, from the committed rocprofv3 PMC passes (FETCH_SIZE doubled per
    MI355X_MICROARCH.md, WRITE_SIZE; tools/pmc_summary.py) -- counters cannot be collected from inside this
    process, so the number is the profiled one of the same workload (size, width, batch, dtype) AND the same kernel sources
    (the profile records their hash), or None when no matching profile exists.  profiles/pmc_traffic.json is the headline's;
    the other workloads' summaries are profiles/rNN_<name>_pmc_traffic.json (tools/profile_configs.sh): the newest match wins."""
    pdir = os.path.join(os.path.dirname(os.path.abspath(__file__)), "profiles")
    want = {"width": args.width, "hw": args.hw, "batch": args.batch}
    dtype = "f32" if args.dtype == "f32" else "int8"
    try:
        names = sorted((f for f in os.listdir(pdir) if f.endswith("pmc_traffic.json")), reverse=True)
    except OSError:
        return None, None
    why = None
    for name in ["pmc_traffic.json"] + [n for n in names if n != "pmc_traffic.json"]:
        try:
            with open(os.path.join(pdir, name)) as fh:
                d = json.load(fh)
            if d["config"] != want or d.get("dtype", "int8") != dtype:
                why = why or "profiles/%s is for another workload" % name
                continue
            if d.get("kernel_source_sha16") != kernel_source_sha16():
                why = "profiles/%s was taken with other kernel sources (%s, now %s)" % (name, d.get("kernel_source_sha16"), kernel_source_sha16())
                continue
            c = d["conv_i8"]  # (the family total: conv_i8_* or, for a float workload, conv_f32_*)
            return c["read_bytes_per_step"] + c["write_bytes_per_step"], "profiles/%s (per step, all %s launches; kernel sources %s)" % (
                name, d.get("family", "conv_i8"), d["kernel_source_sha16"])
        except (OSError, KeyError, ValueError):
            continue
    return None, why


def reference_detections(ref_outs, scales, thresh=0.45):
    """the reference's own tail (mars_yolo_test.c:80-130, oracle/_ref) on the reference's head tensors of one frame"""
    import refbind
    import orcbind
    pred = np.concatenate([o.view(np.int8).ravel() for o in ref_outs])
    tail = refbind if refbind.available() else orcbind
    return tail.nms(tail.parse_output(pred, len(pred) // 85, np.float32(scales[0])), thresh)


def self_launch(n):
    """`python bench.py --gpus N` with no launcher: N child processes of this (GPU-untouched) one, one per GPU, with the
    environment torch.distributed.run would give them (thingino-accel_amd/dist.py: spawn_ranks); rank 0's single JSON line
    is relayed, a failing rank fails the job, and a line whose n_gpus is not N is refused.  Returns the exit code."""
    D = load_dist_helpers()
    argv = [a for a in sys.argv[1:] if a != "--self-launch"]
    # one rank on one GPU still takes the multi-process path (RCCL group, arena broadcast, barriers, MAX over ranks)
    rc, out, codes = D.spawn_ranks(n, [sys.executable, os.path.abspath(__file__)] + argv, extra_env={"BENCH_FORCE_DIST": "1"})
    if rc != 0:
        print("bench: the %d-rank job failed (exit codes per rank: %r)" % (n, codes), file=sys.stderr)
        return rc
    lines = [l for l in out.splitlines() if l.startswith("{")]
    try:
        d = json.loads(lines[-1]) if len(lines) == 1 else None
    except ValueError:
        d = None
    if d is None or d.get("n_gpus") != n or (d.get("config", {}).get("rccl") or {}).get("ranks_in_group") != n:
        print("bench: rank 0 did not report one line for %d GPUs (got %r)" % (n, out[-400:]), file=sys.stderr)
        return 1
    print(lines[0], flush=True)
    return 0


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--batch", type=int, default=256, help="frames per GPU")
    ap.add_argument("--total-batch", type=int, default=0,
                    help="frames over ALL GPUs (split evenly; must divide by the GPU count).  Default: --batch per GPU, "
                         "except 1024 in total at 8 GPUs (BASELINE config 4: 128 per GPU)")
    ap.add_argument("--weak", action="store_true", help="--batch frames per GPU at every GPU count (also at 8)")
    ap.add_argument("--cpu-threads", type=int, default=0,
                    help="threads of the frames-parallel CPU baseline (0 = every core this process may run on)")
    ap.add_argument("--hw", type=int, default=640)
    ap.add_argument("--width", type=int, default=8, help="channel multiple x16: 8 = yolov5s, 4 = yolov5n")
    ap.add_argument("--dtype", choices=["int8", "f32"], default="int8",
                    help="int8 (default): the headline workload.  f32: BASELINE config 5, the yolov5s_float32 twin (NCHW / OIHW "
                         "float32) with its convolutions on the f32 matrix cores (mars_hip_set_tuning f32_mfma=2); graph only "
                         "(float heads have no int8 decode), outputs checked against the CPU reference within 1e-4*max(1,|b|)")
    ap.add_argument("--model", type=str, default="",
                    help="run this .mars file instead of a synthetic twin (any file the runtime loads, e.g. tests/golden/models/yolov5n_int8.mars: "
                         "BASELINE config 3's literal file, NCHW-tagged -> the conv2d_int8_mxu path).  Inputs per SURVEY 8d (LCG bytes / uniform floats "
                         "by the input's dtype), graph only (no decode + NMS), CPU leg through the reference's own layer functions with every "
                         "activation tensor the plan keeps compared, not just the outputs")
    ap.add_argument("--no-extra-configs", action="store_true",
                    help="skip the short legs of the other BASELINE configs (`configs` in the line: config 3 twin and literal file, config 5, the "
                         "320x320 workloads, config 2) that the default int8 run appends after the headline's legs")
    ap.add_argument("--f32-mode", type=int, default=None, help="--dtype f32 (default 3) / a float --model (default 1): 0 exact order, 1 default policy, 2 f32 matrix cores everywhere, "
                                                            "3 (default) bf16 matrix cores everywhere, operands split in two (three piece products), 4 split in three (six)")
    ap.add_argument("--timed-only", action="store_true",
                    help="skip the legs after the timed region (mars_run / pipelined I/O / batch-1 latency / CPU baselines): "
                         "what profiling passes want")
    ap.add_argument("--no-cpu-baseline", action="store_true")
    ap.add_argument("--tune", action="append", default=[], metavar="KEY=INT",
                    help="mars_hip_set_tuning(KEY, INT) before the model is loaded (experiments; results never depend on it)")
    ap.add_argument("--vary-scales", action="store_true",
                    help="check run, not the benchmark workload: the twin with per-convolution scales (every fused table "
                         "differs); the CPU-baseline leg then compares its frames bit for bit as usual")
    ap.add_argument("--no-tail", action="store_true", help="graph only, skip decode+NMS")
    ap.add_argument("--io", choices=["resident", "pipelined", "camera"], default="resident",
                    help="pipelined: after the timed (resident) region every rank also runs its batches through mars_hip_pipe_* "
                         "(pinned host frames in, detections out) and the line carries `pipelined_io` (MAX over ranks); at N=1 "
                         "the default run measures this anyway.  camera (N=1): additionally the reference demo's whole loop "
                         "(src/mars/mars_yolo_test.c:132-214) -- uint8 RGB 1280x720 frames in pinned host memory -> letterbox / px-128 on "
                         "the device -> graph -> decode + NMS -> detections back, pipelined (mars_hip_pipe_* in camera mode): `camera_io`")
    ap.add_argument("--full", action="store_true",
                    help="also run every leg beyond the timed steps (sustained, I/O, batch-1, CPU baselines and parity, copy-rate "
                         "probe, the other BASELINE configs); a plain run does only what the headline figure needs")
    ap.add_argument("--dump-outputs", type=str, default="", metavar="DIR",
                    help="after the timed steps, write what the last one computed (graph outputs of a seeded sample of frames, "
                         "every frame's detections) to DIR/<name>.npy as float32, 64 MB at most")
    ap.add_argument("--sustain-s", type=float, default=None,
                    help="seconds of back-to-back steps of the sustained leg (0 = skip; default 3 with --full, else 0)")
    ap.add_argument("--ops", type=str, default="", help="write a per-launch table (last timed step) to this file")
    ap.add_argument("--autotune", action="store_true",
                    help="time the launch variants of every convolution once before the warmup and pin the fastest "
                         "(mars_hip_autotune; a load-time cost, outside the timed region).  Off by default: the default "
                         "launch policy was re-derived from the tuner's choices and is within 1 %% of it")
    ap.add_argument("--no-autotune", action="store_true", help="(default; kept for older command lines)")
    ap.add_argument("--event-steps", type=int, default=1,
                    help="timed steps (the last ones) whose launches are bracketed by HIP events for the roofline; "
                         "each event pair costs a queue barrier, so not every step carries them")
    ap.add_argument("--self-launch", action="store_true",
                    help="start the --gpus N ranks as child processes of this one even at N=1 (what `--gpus N` with N>1 does "
                         "by itself when no launcher has set WORLD_SIZE): rehearses the N>1 entry point on one GPU")
    args = ap.parse_args()
    if args.sustain_s is None:
        args.sustain_s = 3.0 if args.full else 0.0
    # the legs behind --full; --timed-only (profiling passes) skips them even there
    extras = args.full and not args.timed_only

    # ---- N ranks: either a launcher started us (torch.distributed.run sets WORLD_SIZE; it must equal --gpus), or this
    # process -- which has not imported torch nor made a HIP call -- starts one fresh child per GPU and relays rank 0's line
    if "WORLD_SIZE" not in os.environ and (args.gpus > 1 or args.self_launch):
        sys.exit(self_launch(args.gpus))
    world = int(os.environ.get("WORLD_SIZE", "1"))
    if world != args.gpus:
        raise SystemExit("bench: --gpus %d but the launcher started %d ranks (WORLD_SIZE): refusing to report a line whose "
                         "n_gpus is not the --gpus asked for" % (args.gpus, world))
    rank = int(os.environ.get("RANK", "0"))
    local_rank = int(os.environ.get("LOCAL_RANK", "0"))
    dist = None
    # frames per GPU: explicit total > config 4 at eight GPUs > --batch per GPU
    total_batch = args.total_batch if args.total_batch > 0 else (1024 if world == 8 and not args.weak and args.batch == 256 else 0)
    if total_batch:
        if total_batch % world:
            raise SystemExit("--total-batch %d does not divide over %d GPUs" % (total_batch, world))
        args.batch = total_batch // world
    # BENCH_FORCE_DIST=1: take the multi-process path (process group, descriptor-only load is skipped on rank 0, arena
    # broadcast, barriers, max over ranks) with however many ranks there are -- a one-GPU rehearsal of the N>1 code
    multi = world > 1 or os.environ.get("BENCH_FORCE_DIST") == "1"
    # stdout carries exactly ONE line, the JSON: whatever libraries write to file descriptor 1 while the job runs (RCCL
    # prints a version banner there) goes to stderr instead; the descriptor is restored just before the line is printed
    sys.stdout.flush()
    saved_stdout = os.dup(1)
    os.dup2(2, 1)
    if multi:
        import torch
        import torch.distributed as dist
        os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
        os.environ.setdefault("MASTER_PORT", "29533")
        os.environ.setdefault("RANK", "0")
        os.environ.setdefault("WORLD_SIZE", "1")
        torch.cuda.set_device(local_rank)
        dist.init_process_group("nccl", device_id=torch.device("cuda", local_rank))
    os.environ.setdefault("MARS_HIP_DEVICE", str(local_rank))

    M = load_marsrt()
    D = load_dist_helpers()
    PROBE = load_probe()
    import marsfile
    M.nna_init()
    f32 = args.dtype == "f32"
    file_hdr = None
    if args.model:  # a .mars file instead of a twin: its input's dtype / shape decide the frame bytes; graph only
        with open(args.model, "rb") as fh:
            model_bytes = fh.read()
        file_hdr = marsfile.parse(model_bytes)
        tin0 = file_hdr[1][file_hdr[0]["inputs"][0]]
        f32 = tin0["dtype"] == 0
        args.dtype = "f32" if f32 else "int8"
        args.hw, args.in_w = input_hw_of(tin0)
        args.width = 0
        args.no_tail = True
    if args.f32_mode is None:
        args.f32_mode = 1 if args.model else 3
    dual_min = 64  # the library's default for "dual_stream_min_batch"
    for kv in args.tune:
        k, v = kv.split("=")
        M.set_tuning(k, int(v))
        if k == "dual_stream_min_batch":
            dual_min = int(v)
    dual_on = dual_min > 0
    if f32:
        args.no_tail = True
        M.set_tuning("f32_mfma", args.f32_mode)
    if not args.model:
        model_bytes = M.synth_model(width_x16=args.width, input_hw=args.hw, seed=1, vary_scales=args.vary_scales, float32=f32)
    hdr, tensors, _ = marsfile.parse(model_bytes)
    in_bytes = marsfile.tensor_nbytes(tensors[hdr["inputs"][0]])
    out_ids = list(hdr["outputs"])

    rccl_info = None
    if multi and rank != 0:
        # descriptors only; the packed parameters arrive by RCCL broadcast from rank 0
        model = M.Model(D.strip_weights(model_bytes), batch=args.batch, flags=1)
    else:
        model = M.Model(model_bytes, batch=args.batch)
    if multi:
        import torch
        ptr, nbytes = model.param_arena()
        sizes = [None] * dist.get_world_size()
        dist.all_gather_object(sizes, int(nbytes))  # every rank planned the same arena (descriptors + batch decide it)
        if len(set(sizes)) != 1:
            raise RuntimeError("parameter arena sizes differ across ranks: %r" % (sizes,))
        if rank == 0:
            print("bench: %d ranks in the RCCL group, parameter arena %d bytes broadcast from rank 0" % (dist.get_world_size(), nbytes),
                  file=sys.stderr)
        t = torch.as_tensor(D.DeviceBuffer(ptr, nbytes), device="cuda")
        torch.cuda.synchronize()
        dist.barrier()
        tb = time.perf_counter()
        dist.broadcast(t, src=0)  # the one collective of the path: weights over xGMI
        torch.cuda.synchronize()
        tb = time.perf_counter() - tb
        rccl_info = {"ranks_in_group": dist.get_world_size(), "backend": dist.get_backend(), "param_arena_bytes": int(nbytes),
                     "broadcast_ms": D.max_over_ranks(dist, tb, device="cuda") * 1e3}

    frames = frames_for_rank(D, rank, world, args.batch, in_bytes, f32)
    iv = model.input_view(0)
    for f in range(args.batch):
        iv[f, :in_bytes] = frames[f]
    model.upload()  # inputs resident in HBM before the timed region
    outputs = tuple(range(len(out_ids)))
    if args.autotune and not args.no_autotune:
        model.run_device()  # real activations in every tensor first: MFMA clocks depend on the data
        model.autotune(3)

    def step():
        # graph on the main stream; decode+NMS tail on the auxiliary stream, where it overlaps the
        # NEXT step's convolutions (the next step's output-writing layers wait for it by event)
        model.run_device(sync=False)
        if not args.no_tail:
            model.detect_device(outputs=outputs, thresh=0.45)

    def barrier():
        M.lib().mars_hip_sync()
        if dist is not None:
            import torch
            torch.cuda.synchronize()
            dist.barrier()

    for _ in range(args.warmup):
        step()
    # ---- timed region: exactly K steps; in the last `event_steps` of them every launch is bracketed by
    # HIP events on the library's stream (per-kernel durations for the roofline)
    conv_ms = conv_ops = all_ms = 0.0
    ckind = 1 if f32 else 0  # the dominant kernel family: conv_f32_* or conv_i8_*
    per_kind = {}
    ev_steps = max(1, min(args.event_steps, args.steps))
    barrier()
    t0 = time.perf_counter()
    for k in range(args.steps):
        timed = k >= args.steps - ev_steps
        model.set_profiling((1 if args.ops else 2) if timed else 0)  # 2: one event per run of same-kind launches
        step()
        if timed:
            for op in model.ops():
                per_kind[op["kind"]] = per_kind.get(op["kind"], 0.0) + op["ms"]
                all_ms += op["ms"]
                if op["kind"] == ckind:
                    conv_ms += op["ms"]
                    conv_ops += 2.0 * op["macs"] * args.batch
    barrier()
    dt = time.perf_counter() - t0
    model.set_profiling(False)
    if dist is not None:
        dt = D.max_over_ranks(dist, dt, device="cuda")
    if args.dump_outputs and rank == 0:  # before any further leg: the last timed step's results, as a caller would read them
        dump_outputs(model, tensors, out_ids, not args.no_tail, args.dump_outputs)

    # ---- sustained leg (every rank): the timed region above is a burst of K steps after an idle device; a camera pipeline
    # runs for hours.  Back-to-back steps for >= --sustain-s seconds, the shader clock sampled while they run
    # (mars_hip_clock_mhz: one probe wave on its own stream): the chip lowers its clock under a sustained int8 MFMA load.
    sustained = None
    if args.sustain_s > 0 and not args.timed_only:
        # 8 % more steps than the timed region's pace predicts: back to back the steps run a little faster than in the
        # 30-step burst, and the leg must not end short of --sustain-s
        nsteps = max(args.steps, int(1.08 * args.sustain_s / max(dt / args.steps, 1e-4)) + 1)
        clocks = []
        barrier()
        t1 = time.perf_counter()
        for k in range(nsteps):
            step()
            if k % max(1, nsteps // 8) == nsteps // 16:  # ~8 samples spread over the leg (each blocks the host ~0.3 ms)
                c = float(PROBE.mars_probe_clock_mhz(200))
                if c > 0:
                    clocks.append(c)
        barrier()
        dts = time.perf_counter() - t1
        # (the prediction can fall short -- a slow first burst on a small batch --: top up in eighths until the asked time has passed;
        # every rank takes the same decision from the same MAX over ranks)
        while (D.max_over_ranks(dist, dts, device="cuda") if dist is not None else dts) < args.sustain_s and nsteps < 1000000:
            extra = max(1, nsteps // 8)
            for k in range(extra):
                step()
            barrier()
            nsteps += extra
            dts = time.perf_counter() - t1
        if dist is not None:
            dts = D.max_over_ranks(dist, dts, device="cuda")
        sustained = {"images_per_s": world * args.batch * nsteps / dts, "steps": nsteps, "seconds": dts,
                     "ms_per_step": dts / nsteps * 1e3,
                     "shader_clock_mhz": {"median": float(np.median(clocks)) if clocks else None,
                                          "min": min(clocks) if clocks else None, "max": max(clocks) if clocks else None,
                                          "samples": len(clocks), "how": "s_memtime / s_memrealtime of a probe wave beside the running graph"}}

    # ---- I/O-inclusive leg (every rank; default at N=1, --io pipelined at any N): frames come from pinned host memory
    # every batch (mars_hip_pipe_*: upload k+1 / graph k / tail k / download k-1 on their own streams), detections (or the
    # raw head tensors too) go back.  The staging buffers are filled once (a camera would DMA into them).
    pipe_rates = {}
    want_pipe = not f32 and not args.no_tail and not args.timed_only and ((extras and world == 1) or args.io == "pipelined")
    if want_pipe:
        stacked = np.stack(frames)
        modes = (("detections", False), ("raw_outputs", True)) if world == 1 else (("detections", False),)
        for key, dl in modes:
            model.pipe_open(download_outputs=dl, detect=True, det_outputs=outputs, thresh=0.45)
            # untimed: fill all four staging slots (a camera would DMA into them) by running four batches through and
            # draining them, so that the timed loop below copies nothing on the host
            for k in range(4):
                model.pipe_input_view(0)[:] = stacked
                model.pipe_submit()
                if k >= 2:
                    model.pipe_wait(copy=False)
            for _ in range(2):
                model.pipe_wait(copy=False)
            # the window holds every batch that is counted -- the three that fill the pipeline are submitted
            # after t1 and the last three are drained before the clock stops (fill and drain are inside: the rate is
            # slightly pessimistic, never optimistic)
            nb = 16
            barrier()
            t1 = time.perf_counter()
            for k in range(3):
                model.pipe_submit()
            for _ in range(nb):
                model.pipe_wait(copy=False)
                model.pipe_submit()
            for _ in range(3):
                model.pipe_wait(copy=False)
            dtp = time.perf_counter() - t1
            if dist is not None:
                dtp = D.max_over_ranks(dist, dtp, device="cuda")
            model.pipe_close()
            pipe_rates[key] = world * (nb + 3) * args.batch / dtp

    # ---- camera leg (--io camera): the demo's loop.  Frames: 1280 x 720 uint8 RGB (a camera's native size; the front-end shrinks
    # them to the graph's 640 x 640 exactly as the reference's load_image() does) from pinned host memory, every batch.
    camera = None
    if args.io == "camera" and world == 1 and not f32 and not args.no_tail and not args.timed_only:
        from conftest import lcg_frame
        cw, chh = 1280, 720
        model.pipe_open(download_outputs=False, detect=True, det_outputs=outputs, thresh=0.45, camera=(cw, chh))
        shots = [lcg_frame(0xCA3E0000 + k, cw * chh * 3) for k in range(8)]
        for k in range(4):  # fill the four staging slots once (a camera would DMA into them), untimed
            v = model.pipe_input_view(0)
            for f in range(args.batch):
                v[f] = shots[(f + k) % 8]
            model.pipe_submit()
            if k >= 2:
                model.pipe_wait(copy=False)
        for _ in range(2):
            model.pipe_wait(copy=False)
        nb, pre_ms = 12, []
        barrier()
        t1 = time.perf_counter()
        for k in range(3):
            model.pipe_submit()
        for _ in range(nb):
            model.pipe_wait(copy=False)
            pre_ms.append(float(M.lib().mars_hip_pipe_camera_ms(model.p)))
            model.pipe_submit()
        for _ in range(3):
            model.pipe_wait(copy=False)
        dtc = time.perf_counter() - t1
        model.pipe_close()
        pre = float(np.median([x for x in pre_ms if x > 0])) if any(x > 0 for x in pre_ms) else None
        pre_bytes = args.batch * (cw * chh * 3 + in_bytes)  # every camera byte read once + every graph-input byte written once
        camera = {"images_per_s": (nb + 3) * args.batch / dtc, "frame": "%dx%d uint8 RGB, pinned host memory" % (cw, chh),
                  "host_to_device_bytes_per_batch": args.batch * cw * chh * 3, "returns": "detections",
                  "timing": "%d batches submitted AND drained inside the window, three in flight" % (nb + 3),
                  "preproc_kernel": {"ms_per_batch": pre, "algorithmic_bytes": pre_bytes,
                                     "achieved_gbs": pre_bytes / (pre * 1e-3) / 1e9 if pre else None,
                                     "frac_of_hbm_peak": pre_bytes / (pre * 1e-3) / 8e12 if pre else None,
                                     "how": "HIP events around the letterbox kernel (preproc.hip: letterbox_strip_kernel) on the main stream ahead of the graph (mars_hip_pipe_camera_ms), median"}}

    result = None
    if rank == 0 and args.ops:
        import ctypes as C
        L = M.lib()
        with open(args.ops, "w") as fh:
            fh.write("op layer kind ms gmac_per_img mb_per_img TOPs GBs\n")
            for i, op in enumerate(model.ops()):
                tops = 2 * op["macs"] * args.batch / (op["ms"] * 1e-3) / 1e12 if op["ms"] > 0 else 0
                gbs = op["bytes"] * args.batch / (op["ms"] * 1e-3) / 1e9 if op["ms"] > 0 else 0
                fh.write("%d %d %d %.4f %.4f %.3f %.1f %.0f\n" % (i, op["layer"], op["kind"], op["ms"], op["macs"] / 1e9,
                                                                 op["bytes"] / 1e6, tops, gbs))
    if rank == 0:
        n_conv = sum(1 for op in model.ops() if op["kind"] == ckind)
        macs_per_img = sum(op["macs"] for op in model.ops() if op["kind"] == ckind)
        bytes_per_img = sum(op["bytes"] for op in model.ops())
        achieved = conv_ops / (conv_ms * 1e-3) / 1e12 if conv_ms > 0 else 0.0
        conv_bytes_per_img = sum(op["bytes"] for op in model.ops() if op["kind"] == ckind)
        traffic, traffic_src = pmc_traffic(args)
        # f32: the ceiling of the path that runs -- v_mfma_f32_16x16x4_f32 at 157.3 TF, or (mode 3) six bf16 MFMAs per product on
        # the 2.5 PF bf16 cores = 417 TF of float32 work; int8: the dense int8 MFMA rate
        mpeak = (2.5e15 / 3.0 if args.f32_mode == 3 else 2.5e15 / 6.0 if args.f32_mode == 4 else 157.3e12) if f32 else 5e15
        floor_ms = sum(max(op["bytes"] * args.batch / 8e12, 2.0 * op["macs"] * args.batch / mpeak)
                       for op in model.ops() if op["kind"] == ckind) * 1e3
        peak = mpeak / 1e12  # dense int8 MFMA, TOP/s: 2x the ~2.5 PF bf16 dense peak (MI355X_MICROARCH.md, Matrix cores)
        conv_s = conv_ms / ev_steps * 1e-3
        hbm_gbs = conv_bytes_per_img * args.batch / conv_s / 1e9 if conv_ms > 0 else 0.0
        # int8: the conv family's arithmetic intensity (2*MAC / algorithmic byte ~ 260 op/B) is below the machine's ridge
        # (5000 TOP/s / 8 TB/s = 625 op/B), so its roof is HBM: achieved = algorithmic bytes of the conv launches / their
        # summed durations; the matrix-roof view of the same launches is reported next to it.  f32: 4-byte activations but
        # a 32x lower matrix peak (157.3 TF, v_mfma_f32_16x16x4_f32): ridge 20 flop/B against ~65 flop/B -> the roof is MFMA.
        # the roof that bounds the family = whichever floor is HIGHER: algorithmic bytes at 8 TB/s against 2 * MAC at the matrix peak of the
        # path that runs (the float32 twin in mode 3 is nearer the HBM roof -- 64.7 GB / 8 TB/s = 8.1 ms against 5.0 ms of bf16x3)
        hbm_floor_s, mfma_floor_s = conv_bytes_per_img * args.batch / 8e12, 2.0 * macs_per_img * args.batch / mpeak
        by_hbm = hbm_floor_s >= mfma_floor_s
        roof = {"bound": "hbm" if by_hbm else "mfma",
                "kernel": (("conv_f32_prec / conv_f32_patch / conv_f32_stem (k x k layers: input patch staged once -- by LDS-DMA from record-format tensors where a convolution wrote them) + conv_f32_split (1 x 1 layers, C3 pairs in one launch); v_mfma_f32_16x16x32_bf16, 3 per product" if args.f32_mode == 3
                            else "conv_f32_split (v_mfma_f32_16x16x32_bf16, 6 per product)" if args.f32_mode == 4 else "conv_f32_mfma / conv_f32_kernel") if f32 else "conv_i8_*") + " (%d launches per step)" % n_conv,
                "achieved": hbm_gbs if by_hbm else achieved, "peak": 8000.0 if by_hbm else peak, "unit": "GB/s" if by_hbm else ("TFLOP/s" if f32 else "TOP/s"),
                "frac": hbm_gbs / 8000.0 if by_hbm else (achieved / peak),
                "floors_ms": {"hbm": hbm_floor_s * 1e3, "mfma": mfma_floor_s * 1e3},
                "traffic": traffic, "traffic_source": traffic_src,
                "algorithmic_bytes": conv_bytes_per_img * args.batch,
                "intensity_ops_per_byte": 2.0 * macs_per_img / conv_bytes_per_img if conv_bytes_per_img else None,
                "mfma_view": {"achieved": achieved, "peak": peak, "unit": "TFLOP/s" if f32 else "TOP/s", "frac": achieved / peak},
                "hbm_view": {"achieved": hbm_gbs, "peak": 8000.0, "unit": "GB/s", "frac": hbm_gbs / 8000.0},
                # what the same launches would take with every layer on its own roof: sum over the conv launches of
                # max(algorithmic bytes / 8 TB/s, 2*MAC / matrix peak); `frac_of_per_layer_floor` = that / measured
                "per_layer_floor_ms": floor_ms,
                "frac_of_per_layer_floor": (floor_ms / (conv_ms / ev_steps)) if conv_ms > 0 else 0.0,
                "event_timed_steps": ev_steps,
                # kernel durations: HIP events on the library's stream, every launch over the FULL batch on ONE stream.
                # The timed steps themselves run the batch as two halves on two streams (config.execution), whose launches
                # overlap: ms_per_step may be smaller than the sum of kernel durations
                "timing": "hip events, one stream, full-batch launches",
                # the same algorithmic bytes over the step time of `value` (its execution mode: config.execution), so that
                # kernel time <= step time holds on this line: frac_wall <= what the per-kernel view can show
                "wall_achieved": conv_bytes_per_img * args.batch / (dt / args.steps) / 1e9 if by_hbm else 2.0 * macs_per_img * args.batch / (dt / args.steps) / 1e12,
                "frac_wall": (conv_bytes_per_img * args.batch / (dt / args.steps) / 1e9 / 8000.0) if by_hbm else (2.0 * macs_per_img * args.batch / (dt / args.steps) / mpeak),
                "conv_ms_per_step": conv_ms / ev_steps,
                "all_kernels_ms_per_step": all_ms / ev_steps,
                "ms_per_step_by_kind": {str(k): v / ev_steps for k, v in sorted(per_kind.items())}}
        result = {
            "metric": ("images/sec %s %dx%d batch%d" % (os.path.basename(args.model), args.in_w, args.hw, args.batch)) if args.model else
                      "images/sec %s_%s %dx%d batch%d" % ("yolov5s" if args.width == 8 else "yolov5n" if args.width == 4 else
                                                        "yolov5(width_x16=%d)" % args.width, "float32" if f32 else "int8",
                                                        args.hw, args.hw, args.batch),
            "value": world * args.batch * args.steps / dt,
            "unit": "images/s",
            "n_gpus": world,
            "steps": args.steps,
            "warmup": args.warmup,
            "ms_per_step": dt / args.steps * 1e3,
            "higher_is_better": True,
            # 256 (= --batch) frames on every GPU: weak.  The default 8-GPU run is BASELINE config 4 (1024 frames in all,
            # 128 per GPU): the same total as 4 GPUs x 256, i.e. strong scaling from there
            "scaling": "strong" if total_batch else "weak",
            "vs_baseline": None,
            # the arithmetic the convolutions run in: modes 3 / 4 multiply exact bf16 pieces of the float32 operands on the bf16 matrix
            # cores and accumulate in f32 (DESIGN.md section 5 "f32 path, round 4"); results inside north_star's 1e-4, checked below
            "dtype": ("f32 (bf16x3: operands split exactly into two bf16 pieces, three piece products, f32 accumulate)" if args.f32_mode == 3
                      else "f32 (bf16x6: three bf16 pieces, six piece products, f32 accumulate)" if args.f32_mode == 4 else "f32") if f32 else "int8",
            "data": "synthetic",
            "config": {"workload": ("file %s (sha256 %s, %d layers, input %s %s), frames per SURVEY 8d, batch %d per GPU, graph only%s" % (
                                        os.path.basename(args.model), hashlib.sha256(model_bytes).hexdigest()[:16], hdr["layers"],
                                        "f32" if f32 else "int8", "NHWC" if tensors[hdr["inputs"][0]]["fmt"] == 7 else "NCHW-tagged", args.batch,
                                        ", f32_mfma mode %d" % args.f32_mode if f32 else "")) if args.model else
                                   ("synthetic yolov5s_float32.mars twin (mars_synth_model width_x16=%d, seed 1, float32), %dx%d f32 "
                                    "NCHW frames, batch %d per GPU, graph only, f32_mfma mode %d%s" %
                                    (args.width, args.hw, args.hw, args.batch, args.f32_mode,
                                     "" if args.f32_mode < 3 or os.environ.get("MARS_HIP_NO_ZERO_TAIL") else
                                     "; 1 x 1 convolutions that read a byte-wise CONCAT's output stop their K loop at the last channel it can have written "
                                     "(exact zeros behind it: DESIGN.md section 5; conv_gmac_per_image counts the multiplied part; MARS_HIP_NO_ZERO_TAIL=1 runs the full loops)" +
                                     ("" if os.environ.get("MARS_HIP_NO_VCONCAT_F32") else "; those concats are not materialised: their readers run on a view of the concat's "
                                      "last input, a head launch recomputes the first pixels (virtual_concat_f32; MARS_HIP_NO_VCONCAT_F32=1 copies them)"))) if f32 else
                                   "synthetic yolov5s_int8.mars twin (mars_synth_model width_x16=%d, seed 1), %dx%d int8 "
                                   "NHWC frames, batch %d per GPU, decode+NMS tail %s%s" %
                                   (args.width, args.hw, args.hw, args.batch, "off" if args.no_tail else "on",
                                    ", per-convolution scales (check run)" if args.vary_scales else ""),
                       "frames_per_gpu": args.batch, "frames_total": args.batch * world,
                       "baseline_config": ("configs[3]: 1024 frames frame-sharded over 8 GPUs" if world == 8 and args.batch * world == 1024
                                           else "configs[1]-class: the metric's batch 256 per GPU" if args.batch == 256 else "custom"),
                       "execution": ("two half-batches on two streams (dual_stream_min_batch)" if dual_on and args.batch >= dual_min
                                     else "one stream"),
                       "ranks": world, "sharding": "frames", "collectives_in_forward": 0,
                       "autotuned_launch_variants": bool(args.autotune and not args.no_autotune), "conv_gmac_per_image": macs_per_img / 1e9, "algorithmic_mb_per_image": bytes_per_img / 1e6},
            "roofline": roof,
        }
        if sustained is not None:
            result["sustained_images_per_s"] = sustained["images_per_s"]
            result["sustained"] = sustained
        if pipe_rates:
            result["pipelined_io"] = {"images_per_s": pipe_rates.get("detections"), "returns": "detections (4 KB per frame)",
                                      "ranks": world, "timing": "barrier, then 19 batches per rank submitted AND drained inside the window (pipeline fill and drain included), MAX over ranks"}
            if world == 1:
                result["pipelined_detections_images_per_s"] = pipe_rates.get("detections")
                result["pipelined_raw_outputs_images_per_s"] = pipe_rates.get("raw_outputs")
        if camera is not None:
            result["camera_io"] = camera
        if multi:
            result["config"]["rccl"] = rccl_info
        if world == 1 and extras:
            # not the headline value: the same batch INCLUDING host->HBM input copies and HBM->host
            # output copies through the reference API's mars_run() (pinned staging, one stream)
            M.lib().mars_hip_sync()
            model.run()  # first call: creates the copy streams / events of the chunked path
            t1 = time.perf_counter()
            for _ in range(3):
                model.run()
            result["pcie_inclusive_images_per_s"] = 3 * args.batch / (time.perf_counter() - t1)
            if not args.no_tail and not f32:
                # the same call for a caller that wants detections, not head tensors: the graph outputs stay in HBM
                # (mars_hip_set_output_mode), mars_hip_detect brings back 24 KB per frame at most
                M.lib().mars_hip_set_output_mode(model.p, 1)
                model.run()
                t1 = time.perf_counter()
                for _ in range(3):
                    model.run()
                    model.detect(outputs=outputs, thresh=0.45)
                result["pcie_inclusive_detections_only_images_per_s"] = 3 * args.batch / (time.perf_counter() - t1)
                M.lib().mars_hip_set_output_mode(model.p, 0)
            if not args.no_tail:
                # context for `value`: the same steps without the decode + NMS tail.  The twin's random heads put ~19 000
                # predictions per frame above the threshold, so every frame hits the reference's cap of 1000 candidates
                # and keeps ~780 boxes: the worst case for the sort and the NMS (a trained detector yields tens).
                dets = model.detect(outputs=outputs, thresh=0.45)
                result["config"]["kept_boxes_per_frame"] = float(np.mean([len(x) for x in dets]))
                M.lib().mars_hip_sync()
                for _ in range(3):
                    model.run_device(sync=False)
                M.lib().mars_hip_sync()
                t1 = time.perf_counter()
                for _ in range(10):
                    model.run_device(sync=False)
                M.lib().mars_hip_sync()
                result["graph_only_images_per_s"] = 10 * args.batch / (time.perf_counter() - t1)
        if world == 1 and extras:
            # the reference's real call pattern (mars_test.c:33-148): ONE frame per mars_run.  Latency of the graph alone
            # (input resident) and through mars_run() (H2D + graph + D2H), median of 20
            m1 = M.Model(model_bytes, batch=1)
            m1.input_view(0)[0] = frames[0]
            m1.upload()
            lat = {}
            def run_and_detect():  # the demo's loop (mars_yolo_test.c:132-214): run, then decode + NMS of the result
                m1.run()
                m1.detect(outputs=outputs, thresh=0.45)
            legs = [("graph_resident_ms", m1.run_device), ("mars_run_ms", m1.run)]
            if not args.no_tail:
                legs.append(("mars_run_plus_detect_ms", run_and_detect))
            for name, fn in legs:
                for _ in range(3):
                    fn()
                ts = []
                for _ in range(20):
                    t1 = time.perf_counter()
                    fn()
                    ts.append(time.perf_counter() - t1)
                lat[name] = sorted(ts)[len(ts) // 2] * 1e3
            lat["launches"] = len(m1.ops())
            result["latency_batch1"] = lat
            m1.close()
        if world == 1 and not args.no_cpu_baseline and extras:
            model.download()
            every = {"tensors_compared": 0, "tensors_equal": 0}

            def all_tensors(runner, f):  # --model: every activation tensor the plan keeps in HBM, frame f, against the reference's
                a, b, _ = compare_frame(model, runner, tensors, out_ids, f, f32, every_tensor=True)
                every["tensors_compared"] += a
                every["tensors_equal"] += b
            base, ref_outs = cpu_baseline(model_bytes, frames, out_ids, max_frames=1 if f32 else (2 if args.model else 16), file_model=bool(args.model),
                                          on_frame=all_tensors if args.model else None)
            if args.model:
                base["every_materialised_tensor"] = dict(every, rule="|a-b| <= 1e-4*max(1,|b|)" if f32 else "bit-exact",
                                                         ok=every["tensors_compared"] > 0 and every["tensors_equal"] == every["tensors_compared"])
            if f32:  # north_star: within 1e-4 on the float32 models
                worst = 0.0
                heads = []  # is the comparison informative?  finite share and magnitude of every head, on both sides
                for f in range(len(ref_outs)):
                    for i in range(len(out_ids)):
                        a = model.output_view(i)[f].view(np.float32).astype(np.float64)
                        b = ref_outs[f][i].view(np.float32).astype(np.float64)
                        fin = np.isfinite(a) & np.isfinite(b)
                        sane = fin & (np.abs(b) < 1e6)
                        heads.append({"head": i, "finite_fraction_gpu": float(np.isfinite(a).mean()), "finite_fraction_reference": float(np.isfinite(b).mean()),
                                      "max_abs_reference": float(np.abs(b[fin]).max()) if fin.any() else None,
                                      "worst_relative_error_where_finite_and_below_1e6": float((np.abs(a - b)[sane] / np.maximum(1.0, np.abs(b)[sane])).max()) if sane.any() else None})
                        if (np.isnan(a) != np.isnan(b)).any() or (np.isinf(a) != np.isinf(b)).any():
                            worst = float("inf")  # a NaN / inf on one side only is a failure, not a value np.nanmax may drop
                        bad = ~((np.isnan(a) & np.isnan(b)) | (a == b))
                        if bad.any() and worst != float("inf"):
                            err = np.abs(a - b)[bad] / np.maximum(1.0, np.abs(b)[bad])
                            worst = float("inf") if np.isnan(err).any() else max(worst, float(err.max()))
                base["gpu_matches_within_1e-4"] = bool(worst <= 1e-4)
                base["worst_relative_error"] = worst
                base["heads"] = heads
                same = worst == 0.0
            else:
                same = all(np.array_equal(ref_outs[f][i], model.output_view(i)[f])
                           for f in range(len(ref_outs)) for i in range(len(out_ids)))
            base["gpu_matches_bit_exact"] = bool(same)
            base["frames_compared"] = len(ref_outs)
            if not f32 and not args.no_tail:
                # BASELINE's "mAP delta vs CPU ref": no labelled data exists for this path, so it degenerates to exact
                # agreement of the kept boxes -- count, order, coordinates, confidences, classes -- between the GPU tail
                # on the GPU's heads and the reference's parse_output + nms on the reference's heads
                gdets = model.detect(outputs=outputs, thresh=0.45)
                scales = [float(tensors[ti]["scale"]) for ti in out_ids]
                nbox, dsame = 0, True
                for f in range(len(ref_outs)):
                    want = reference_detections(ref_outs[f], scales)
                    nbox += len(want)
                    dsame = dsame and gdets[f].tobytes() == want.tobytes()
                base["detections_match_bit_exact"] = bool(dsame)
                base["detections_compared"] = int(nbox)
                result["map_delta"] = 0.0 if (dsame and same) else None
                result["map_delta_evidence"] = ("%d kept boxes of %d frames (index order, boxes, confidences, classes) and the int8 head "
                                                "tensors bit-identical to the reference's CPU run" % (nbox, len(ref_outs))) if (dsame and same) else "MISMATCH"
            result["cpu_baseline"] = base
            # the fair node-level figure -- frames are independent, one frame per thread on every core
            result["cpu_baseline_all_cores"] = cpu_baseline_parallel(model_bytes, frames, out_ids, args.cpu_threads, ref_outs, f32, bool(args.model))
    if rank == 0 and world == 1 and extras and not f32:
        # (last of all legs: after a 2 GiB allocate / copy / free the raw-heads mars_run leg ran at 9.4k instead of 15.9k img/s)
        # What a plain copy reaches on THIS box: `peak` stays the guide's 8 TB/s, but no kernel that reads and writes HBM
        # gets there -- a 1 GiB device-to-device copy (read + write bytes over its time) is the practical ceiling the
        # conv family's byte rate can be held against.  Untimed for `value`: it runs after the timed region.
        copy_gbs = float(PROBE.mars_probe_copy_rate_gbs(1 << 30, 10))
        result["roofline"]["copy_rate_measured"] = copy_gbs if copy_gbs > 0 else None
        if copy_gbs > 0:
            result["roofline"]["frac_of_copy_rate"] = result["roofline"]["achieved"] / copy_gbs
            result["roofline"]["frac_wall_of_copy_rate"] = result["roofline"]["wall_achieved"] / copy_gbs
        result["roofline"]["copy_rate_how"] = ("libmars_probe.so (csrc/probe/mars_probe.hip): device-to-device copy of 1 GiB, 10 back to back, the best of "
                                               "hipMemcpyAsync and eleven 16-byte-per-lane kernels (1 / 2 / 4 / 8 loads in flight per lane, plain and non-temporal, 64- to 1024-thread "
                                               "workgroups at 2 to 32 per CU: the runtime blit's launch geometries among them); "
                                               "(read + write bytes) / time, GB/s; best form here: %s" % PROBE.mars_probe_copy_form().decode())
        # against what the guide says a kernel can reach at all (MI355X_MICROARCH.md: 6.3 TB/s measured, float4 copy)
        result["roofline"]["achievable_peak"] = 6300.0
        result["roofline"]["frac_of_achievable"] = result["roofline"]["achieved"] / 6300.0
        result["roofline"]["frac_wall_of_achievable"] = result["roofline"]["wall_achieved"] / 6300.0
        clk = (sustained or {}).get("shader_clock_mhz", {}).get("median") if sustained else None
        result["roofline"]["pipes"] = pipe_times(args, result["roofline"]["algorithmic_bytes"], copy_gbs, clk)
    model.close()
    if rank == 0 and world == 1 and not multi and extras and not args.no_extra_configs and not args.model and not f32 and not args.vary_scales:
        # every BASELINE config under the same clock as the headline -- separate model instances, after the headline's
        # timed region and all its legs (the headline's numbers are final by now)
        t1 = time.perf_counter()
        result["configs"] = extra_configs(M, args)
        result["configs_seconds"] = time.perf_counter() - t1
    if dist is not None:
        dist.barrier()
        dist.destroy_process_group()
    sys.stdout.flush()
    os.dup2(saved_stdout, 1)
    os.close(saved_stdout)
    if rank == 0:
        print(json.dumps(result), flush=True)


if __name__ == "__main__":
    main()
