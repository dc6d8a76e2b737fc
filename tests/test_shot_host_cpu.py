"""The host side of the best shots (csrc/host/mars_shots.c) on the CPU, under AddressSanitizer + UBSan: tests/c/shots_host.c is a
stand-alone program that stands in for the device layer (host malloc, memcpy, a launch that does nothing) and drives the option checks, the
frame -> stream map, the uint8 relayout of read_pixels and collect at exact-size buffers, and the object's host paths around them."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "thingino-accel_amd")
HOST = os.path.join(PKG, "csrc", "host")


def test_shots_host_side_under_sanitizers(tmp_path):
    out = tmp_path / "shots_host"
    cmd = ["gcc", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-fno-omit-frame-pointer", "-ffp-contract=off",
           "-Wall", "-Wextra", "-Wno-unused-parameter", "-I" + os.path.join(ROOT, "include"), "-I" + os.path.join(PKG, "csrc"), "-I" + HOST,
           os.path.join(ROOT, "tests", "c", "shots_host.c"), os.path.join(HOST, "mars_shots.c"), os.path.join(HOST, "mars_stage.c"), "-lm",
           "-o", str(out)]
    subprocess.check_call(cmd)
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1")
    r = subprocess.run([str(out)], env=env, capture_output=True, text=True, timeout=60)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "ERROR: AddressSanitizer" not in r.stderr and "runtime error" not in r.stderr and "LeakSanitizer" not in r.stderr, r.stderr
    assert "shots_host: ok" in r.stdout
