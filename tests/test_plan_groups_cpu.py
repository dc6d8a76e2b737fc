"""The launch-group rule (op_form / op_span / op_head / op_is_mate, csrc/host/mars_internal.h) on the CPU, under AddressSanitizer + UBSan:
tests/c/plan_groups.c is a stand-alone program that includes the helpers without the device layer and checks form, span, members and head
on hand-made op arrays (every form, groups back to back, at the plan's end and cut short by it)."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "thingino-accel_amd")
HOST = os.path.join(PKG, "csrc", "host")


def test_group_rule_under_sanitizers(tmp_path):
    out = tmp_path / "plan_groups"
    cmd = ["cc", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-fno-omit-frame-pointer", "-Wall", "-Wextra",
           "-Wno-unused-parameter", "-I" + os.path.join(ROOT, "include"), "-I" + os.path.join(PKG, "csrc"), "-I" + HOST,
           os.path.join(ROOT, "tests", "c", "plan_groups.c"), "-lm", "-o", str(out)]
    subprocess.check_call(cmd)
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1")
    r = subprocess.run([str(out)], env=env, capture_output=True, text=True, timeout=60)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "ERROR: AddressSanitizer" not in r.stderr and "runtime error" not in r.stderr and "LeakSanitizer" not in r.stderr, r.stderr
    assert "plan_groups: ok" in r.stdout
