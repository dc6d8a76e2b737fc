"""The tail stages' shared host helpers (csrc/host/mars_stage.c: result blocks, side arrays, scale-keyed tables) on the CPU, under
AddressSanitizer + UBSan: tests/c/stage_block.c is a stand-alone program that stands in for the device layer (host malloc, counted events,
a knob that makes the N-th allocation, upload or synchronise fail) and checks the order of the device calls and the records' state."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "thingino-accel_amd")
HOST = os.path.join(PKG, "csrc", "host")


def test_stage_helpers_under_sanitizers(tmp_path):
    out = tmp_path / "stage_block"
    cmd = ["gcc", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-fno-omit-frame-pointer", "-ffp-contract=off",
           "-Wall", "-Wextra", "-Wno-unused-parameter", "-I" + os.path.join(ROOT, "include"), "-I" + os.path.join(PKG, "csrc"), "-I" + HOST,
           os.path.join(ROOT, "tests", "c", "stage_block.c"), os.path.join(HOST, "mars_stage.c"), "-lm", "-o", str(out)]
    subprocess.check_call(cmd)
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1")
    r = subprocess.run([str(out)], env=env, capture_output=True, text=True, timeout=60)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "ERROR: AddressSanitizer" not in r.stderr and "runtime error" not in r.stderr and "LeakSanitizer" not in r.stderr, r.stderr
    assert "stage_block: ok" in r.stdout
