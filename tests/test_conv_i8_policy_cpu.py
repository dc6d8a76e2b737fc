"""The launch policy of the int8 convolution family (csrc/hip/conv_i8.hip, host part) on the CPU: which variant a layer runs.

Every variant writes the same bytes, so the bit-exact GPU tests cannot see the policy slip; a slip shows only as lost speed.
tests/c/conv_i8_policy.c walks a fixed grid of layer descriptors under the default knobs and eight knob settings and prints, per
descriptor and setting, the mhip_conv_i8_variants list (default first), the seg / pre / post / split / both / chain predicates and
mhip_conv_i8_code.  tests/golden/conv_i8_policy.txt is that program's output (built with -DNO_CODE) against the library of the
commit BEFORE the policy was gathered into resolve_code(): every column recorded there must stay as it is."""
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "thingino-accel_amd")
GOLDEN = os.path.join(ROOT, "tests", "golden", "conv_i8_policy.txt")
LABEL_WORDS = 10  # kind c o k s m f t a n


@pytest.fixture(scope="module")
def lines(tmp_path_factory):
    exe = tmp_path_factory.mktemp("conv_i8_policy") / "conv_i8_policy"
    libdir = os.path.join(PKG, "lib")
    subprocess.check_call(["gcc", "-O1", "-Wall", "-Wextra", "-I" + os.path.join(PKG, "csrc"), os.path.join(ROOT, "tests", "c", "conv_i8_policy.c"),
                           "-o", str(exe), "-L" + libdir, "-lnna_mars", "-Wl,-rpath," + libdir])
    env = {k: v for k, v in os.environ.items() if not k.startswith("MARS_HIP_")}  # the knobs' defaults, not this shell's
    r = subprocess.run([str(exe)], env=env, capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, (r.returncode, r.stderr[-1000:])
    return r.stdout.splitlines()


def cells(lines):
    """(knob, kind, variants list, code) of every descriptor under every knob setting ("=": what the default knobs answer)"""
    knobs = lines[0].split()[2:]
    for line in lines[1:]:
        words = line.split()
        cols = words[LABEL_WORDS:]
        assert len(cols) == len(knobs), line
        for knob, col in zip(knobs, cols):
            rec, code = col.rsplit("/", 1)
            if rec == "=":
                rec = cols[0].rsplit("/", 1)[0]
            yield knob, words[0], [int(c) for c in rec.split("|")[0].split(",") if c], int(code), line


def test_recorded_columns_are_unchanged(lines):
    want = open(GOLDEN).read().splitlines()
    assert len(want) > 200 and len(want[0].split()) == 11
    got = [re.sub(r"/-?\d+(?= |$)", "", l) for l in lines]
    assert len(got) == len(want)
    for g, w in zip(got, want):
        assert g == w


def test_code_is_the_first_listed_variant_or_the_forced_one(lines):
    """plain and never-materialised-concat layers (p->variant == 0): the list's first entry, or under the "variant" knob that code where the layer lists it"""
    seen = forced_seen = 0
    for knob, kind, codes, code, line in cells(lines):
        if kind not in ("plain", "deep", "seg", "pair"):
            continue
        assert codes, line
        forced = int(knob.split("=")[1]) if knob.startswith("variant=") else 0
        if forced in codes:
            assert code == forced, (knob, line)
            forced_seen += 1
        else:
            assert code == codes[0], (knob, line)
        seen += 1
    assert seen > 1000 and forced_seen > 20


def test_code_of_a_fused_layer_is_a_listed_variant(lines):
    """pre / post / split (/ chain) layers: the launch height is one of the listed ones; no height fits = the launch refuses the layer"""
    seen = 0
    for knob, kind, codes, code, line in cells(lines):
        if kind not in ("pre", "post", "split", "chain"):
            continue
        if codes:
            assert code in codes and code in (9, 10, 11), (knob, line)
            seen += 1
        else:
            assert code == -1, (knob, line)
    assert seen > 200
