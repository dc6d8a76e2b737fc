"""bench.py's contract (one JSON line with the fields the driver and the judge read), exercised on a small twin so
that it finishes in seconds.  GPU only."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def run_bench(*extra, env=None, full=True):
    out = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "3", "--warmup", "1",
                          "--batch", "4", "--hw", "160", "--width", "4"] + (["--full"] if full else []) + list(extra),
                         capture_output=True, text=True, timeout=600,
                         env=dict(os.environ, **(env or {})))
    assert out.returncode == 0, out.stderr[-2000:]
    lines = [l for l in out.stdout.splitlines() if l.startswith("{")]
    assert len(lines) == 1  # exactly one JSON line
    assert out.stdout.strip() == lines[0]  # ... and nothing else on stdout (library banners go to stderr)
    return json.loads(lines[0])


def test_bench_line_has_the_contract_fields():
    d = run_bench("--hw", "256")  # (every map width of the float twin a multiple of 4 -- the well-conditioned case, cases.SYNTH -- and 256 / 2 = 128 still a size the twins accept)
    for k in ("metric", "value", "unit", "n_gpus", "steps", "warmup", "ms_per_step", "higher_is_better", "scaling",
              "vs_baseline", "dtype", "data", "config", "roofline", "cpu_baseline"):
        assert k in d, k
    assert d["n_gpus"] == 1 and d["steps"] == 3 and d["warmup"] == 1 and d["higher_is_better"] is True
    assert d["unit"] == "images/s" and d["scaling"] == "weak" and d["vs_baseline"] is None and d["dtype"] == "int8"
    assert d["value"] > 0 and d["ms_per_step"] > 0 and "workload" in d["config"]
    r = d["roofline"]
    for k in ("bound", "achieved", "peak", "unit", "frac", "traffic"):
        assert k in r, k
    assert r["bound"] in ("hbm", "mfma") and r["peak"] > 0 and abs(r["frac"] - r["achieved"] / r["peak"]) < 1e-9
    c = d["cpu_baseline"]
    for k in ("value", "unit", "cores", "kind", "sample"):
        assert k in c, k
    assert c["kind"] in ("reference", "port") and c["cores"] == 1 and c["value"] > 0
    assert c["gpu_matches_bit_exact"] is True and c["frames_compared"] >= 1
    a = d["cpu_baseline_all_cores"]  # frames-parallel over the host cores, core count stated
    assert a["cores"] >= 1 and a["value"] > 0 and a["kind"] == c["kind"] and a["matches_single_core_run"] is True
    assert r["per_layer_floor_ms"] > 0 and 0 < r["frac_of_per_layer_floor"] <= 1.0
    lat = d["latency_batch1"]
    assert lat["graph_resident_ms"] > 0 and lat["mars_run_ms"] >= lat["graph_resident_ms"] * 0.5 and lat["launches"] > 0
    assert d["config"]["frames_total"] == 4 and d["config"]["ranks"] == 1
    assert d["graph_only_images_per_s"] > 0 and d["config"]["kept_boxes_per_frame"] >= 0
    # round 3: wall-clock roofline of the execution mode `value` is quoted in, detections compared with the CPU leg's,
    # a sustained leg with the shader clock it ran at
    assert 0 < r["frac_wall"] <= 1.0 and abs(r["frac_wall"] - r["wall_achieved"] / r["peak"]) < 1e-9
    assert c["detections_match_bit_exact"] is True and c["detections_compared"] >= 0 and d["map_delta"] == 0.0
    assert d["sustained_images_per_s"] > 0 and d["sustained"]["steps"] >= 3 and d["sustained"]["seconds"] > 0
    assert lat["mars_run_plus_detect_ms"] >= lat["mars_run_ms"]
    # the practical ceiling of the box (a plain device copy) beside the data-sheet peak
    assert 2000 < r["copy_rate_measured"] < 8000 and abs(r["frac_of_copy_rate"] - r["achieved"] / r["copy_rate_measured"]) < 1e-9
    # round 4: the guide's achievable rate beside the data-sheet peak, the per-pipe times (HBM always; the instruction pipes
    # when the committed profile matches this workload and these kernel sources), the probes from their own library
    assert r["achievable_peak"] == 6300.0 and abs(r["frac_of_achievable"] - r["achieved"] / 6300.0) < 1e-9
    pp = r["pipes"]
    assert pp["hbm_ms_at_peak"] > 0 and pp["hbm_ms_at_achievable"] > pp["hbm_ms_at_peak"] and pp["hbm_ms_at_copy_rate"] > 0
    assert "source" in pp and "libmars_probe.so" in r["copy_rate_how"]
    assert "submitted AND drained inside the window" in d["pipelined_io"]["timing"]
    # round 6: the other BASELINE configs as short legs of the same run -- config 3 (twin AND the reference's own
    # NCHW-tagged file: the conv2d_int8_mxu path), config 5 (float32), the 320-class workloads, config 2 -- each with its rate, the
    # roof that bounds it and a comparison with the reference's CPU run
    cf = d["configs"]
    assert set(cf) == {"config3_yolov5n_int8", "config3_shipped_yolov5n_int8_mars", "config5_yolov5s_float32", "yolov5s_int8_128", "yolov5n_int8_128",
                       "config2_tiny_160_int8_mars"}
    for name, leg in cf.items():
        assert "error" not in leg, (name, leg)
        for k in ("workload", "value", "ms_per_step", "steps", "frac", "bound", "parity"):
            assert k in leg, (name, k)
        assert leg["value"] > 0 and leg["ms_per_step"] > 0 and leg["bound"] in ("hbm", "mfma") and 0 < leg["frac"] <= 1.0, (name, leg)
        assert leg["parity"]["ok"] is True and leg["parity"]["tensors_compared"] >= 1 and leg["parity"]["cpu"] in ("reference", "port"), (name, leg)
    assert cf["config5_yolov5s_float32"]["parity"]["worst_relative_error"] <= 1e-4 and cf["config5_yolov5s_float32"]["dtype"].startswith("f32")
    assert cf["config3_yolov5n_int8"]["parity"]["detections_bit_exact"] is True
    # the literal file: every activation tensor the plan keeps, not just the (never written) output
    assert cf["config3_shipped_yolov5n_int8_mars"]["parity"]["tensors_compared"] > 50
    assert d["configs_seconds"] < 120


def test_bench_model_flag_runs_a_shipped_file():
    """`--model PATH`: BASELINE config 3's literal file (NCHW-tagged -> the conv2d_int8_mxu path every shipped model takes), LCG frames,
    every activation tensor the plan keeps compared with the reference's CPU run of the same frames"""
    d = run_bench("--model", os.path.join(ROOT, "tests", "golden", "models", "yolov5n_int8.mars"), "--sustain-s", "0")
    assert "yolov5n_int8.mars" in d["metric"] and "640x640" in d["metric"] and d["dtype"] == "int8" and d["value"] > 0
    assert "NCHW-tagged" in d["config"]["workload"] and "configs" not in d
    c = d["cpu_baseline"]
    assert c["gpu_matches_bit_exact"] is True and c["frames_compared"] >= 1 and c["kind"] in ("reference", "port")
    assert c["every_materialised_tensor"]["ok"] is True and c["every_materialised_tensor"]["tensors_compared"] > 50
    r = d["roofline"]
    assert r["bound"] in ("hbm", "mfma") and 0 < r["frac"] <= 1.0


def test_bench_sustained_leg_runs_for_the_asked_time():
    d = run_bench("--no-cpu-baseline", "--no-extra-configs", "--sustain-s", "1.0")
    s = d["sustained"]
    assert 0.9 <= s["seconds"] < 5.0 and s["steps"] > 10 and s["shader_clock_mhz"]["median"] > 500
    d = run_bench("--no-cpu-baseline", "--no-extra-configs", "--sustain-s", "0")
    assert "sustained" not in d and "sustained_images_per_s" not in d


def test_bench_flags():
    d = run_bench("--no-cpu-baseline", "--no-extra-configs", "--no-tail", "--no-autotune")
    assert "cpu_baseline" not in d and "tail off" in d["config"]["workload"]
    assert d["config"]["autotuned_launch_variants"] is False


def test_bench_multi_rank_path_with_one_rank():
    """BENCH_FORCE_DIST=1: the N>1 code path (RCCL process group, equal-arena assertion, parameter-arena broadcast,
    barriers, max over ranks) with one rank on this box's one GPU"""
    d = run_bench("--no-cpu-baseline", env={"BENCH_FORCE_DIST": "1", "MASTER_ADDR": "127.0.0.1", "MASTER_PORT": "29541"})
    assert d["n_gpus"] == 1 and d["value"] > 0 and d["scaling"] == "weak"
    rc = d["config"]["rccl"]
    assert rc["ranks_in_group"] == 1 and rc["backend"] == "nccl" and rc["param_arena_bytes"] > 0 and rc["broadcast_ms"] >= 0
    # --io pipelined is honoured on the multi-rank path: every rank drives its own pinned-host pipeline
    d = run_bench("--no-cpu-baseline", "--io", "pipelined", "--sustain-s", "0",
                  env={"BENCH_FORCE_DIST": "1", "MASTER_ADDR": "127.0.0.1", "MASTER_PORT": "29542"})
    assert d["pipelined_io"]["images_per_s"] > 0 and d["config"]["rccl"]["ranks_in_group"] == 1


def test_bench_total_batch_flag():
    d = run_bench("--no-cpu-baseline", "--no-extra-configs", "--total-batch", "6")
    assert d["config"]["frames_per_gpu"] == 6 and d["config"]["frames_total"] == 6 and d["scaling"] == "strong"


def test_bench_starts_its_own_ranks():
    """`bench.py --gpus N` with no launcher starts N ranks itself (dist.spawn_ranks: fresh children of a parent that never
    touched the GPU) and relays rank 0's line; with one GPU here, `--self-launch` takes that entry point for N = 1: the
    child runs the whole multi-process path and the line's rank count is the RCCL group's."""
    env = {k: v for k, v in os.environ.items() if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK", "MASTER_ADDR", "MASTER_PORT")}
    out = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--self-launch", "--steps", "3", "--warmup", "1",
                          "--batch", "4", "--hw", "160", "--width", "4", "--full", "--no-cpu-baseline", "--sustain-s", "0"],
                         capture_output=True, text=True, timeout=600, env=env)
    assert out.returncode == 0, out.stderr[-2000:]
    assert out.stdout.count("\n") == 1 and out.stdout.startswith("{")
    d = json.loads(out.stdout)
    assert d["n_gpus"] == 1 and d["config"]["rccl"]["ranks_in_group"] == d["n_gpus"] and d["config"]["rccl"]["backend"] == "nccl"
    assert d["config"]["ranks"] == 1 and d["value"] > 0
    # a rank count the box cannot serve fails the job instead of reporting fewer GPUs than asked for
    out = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "2", "--steps", "1", "--warmup", "0",
                          "--batch", "2", "--hw", "160", "--width", "4", "--no-cpu-baseline", "--sustain-s", "0", "--timed-only"],
                         capture_output=True, text=True, timeout=600, env=env)
    assert out.returncode != 0 and out.stdout == ""


def test_bench_camera_leg():
    """--io camera: the reference demo's whole loop (RGB camera frames -> front-end -> graph -> decode + NMS -> detections), pipelined"""
    d = run_bench("--no-cpu-baseline", "--no-extra-configs", "--io", "camera", "--sustain-s", "0")
    c = d["camera_io"]
    assert c["images_per_s"] > 0 and "1280x720" in c["frame"] and c["host_to_device_bytes_per_batch"] == 4 * 1280 * 720 * 3
    k = c["preproc_kernel"]
    assert k["ms_per_batch"] > 0 and k["achieved_gbs"] > 0 and 0 < k["frac_of_hbm_peak"] < 1


def test_bench_plain_run_is_lean_and_dumps_outputs(tmp_path):
    """without --full the line carries the headline and its roofline but no further leg; --dump-outputs writes the last timed
    step's head tensors and detections, identical from run to run"""
    dumps = []
    for k in range(2):
        d = run_bench("--dump-outputs", str(tmp_path / str(k)), full=False)
        assert d["steps"] == 3 and d["warmup"] == 1 and d["ms_per_step"] > 0 and d["value"] > 0 and d["dtype"] == "int8"
        assert abs(d["value"] - 4 * 1e3 / d["ms_per_step"]) < 1e-6 * d["value"] and d["roofline"]["bound"] in ("hbm", "mfma")
        for k2 in ("cpu_baseline", "cpu_baseline_all_cores", "sustained", "pipelined_io", "latency_batch1", "configs", "graph_only_images_per_s"):
            assert k2 not in d, k2
        dumps.append({f.stem: np.load(f) for f in (tmp_path / str(k)).iterdir()})
    a, b = dumps
    assert set(a) == set(b) and {"output0", "output1", "output2", "detections", "frames"} <= set(a)
    assert sum(v.nbytes for v in a.values()) <= 64 * 10 ** 6
    assert a["frames"].tolist() == [0, 1, 2, 3] and a["output0"].shape[0] == 4 and a["detections"].shape[1] == 7
    assert all(v.dtype in (np.float32, np.float64) for v in a.values())
    for name in a:
        assert np.array_equal(a[name], b[name]), name
