"""Gallery match (include/mars_hip.h, "Gallery match"), the part that needs no GPU: the entry points are exported, the options struct matches its
ctypes mirror, the quantisation rule on the host equals its numpy restatement bit for bit, arguments that can never be valid are refused up
front, and the numpy restatement that tests/test_gpu_gallery.py compares the device against is itself checked on cases worked out by hand."""
import ctypes as C

import numpy as np
import pytest

F = np.float32
CLS = np.dtype([("cls", "<i4"), ("score", "<f4")])  # mars_cls_t, restated so that the helpers need no library
NEW = ["mars_yolo_embed_quantise", "mars_hip_gallery_create", "mars_hip_gallery_add", "mars_hip_gallery_count", "mars_hip_gallery_clear",
       "mars_hip_gallery_free", "mars_hip_match_chunk", "mars_yolo_match_vectors", "mars_hip_match_device", "mars_hip_match_results",
       "mars_hip_match", "mars_hip_identify_detections_device", "mars_hip_identity_results"]
I32_MAX, I32_MIN = 2 ** 31 - 1, -2 ** 31


# ---- the numpy restatement (Python / int64 integers, np.float32 scalar steps rounded one by one) ----------------------------------------
def quantise_np(vectors, c):
    """int32 embeddings [n][c] -> (int8 q [n][c], int32 qq [n]); qq == 0: a null vector.  Python integers: no width to overflow"""
    v = np.asarray(vectors, dtype=np.int64).reshape(-1, c)
    q = np.zeros(v.shape, dtype=np.int8)
    qq = np.zeros(len(v), dtype=np.int32)
    for n, row in enumerate(v):
        m = max(abs(int(x)) for x in row)
        if m == 0:
            continue
        for i, x in enumerate(row):
            mag = (abs(int(x)) * 127 + m // 2) // m
            q[n, i] = -mag if x < 0 else mag
        qq[n] = int((q[n].astype(np.int64) ** 2).sum())
    return q, qq


def inv_norm(ss):
    """1.0f / sqrtf((float)ss)"""
    return F(F(1) / np.sqrt(F(int(ss))))


def match_np(gallery, ids, queries, c, top_k, min_score=0.0):
    """gallery [G][c] and queries [n][c] int32 embeddings, ids [G] -> (CLS entries [n][top_k], int32 rows [n][top_k])"""
    g, gg = quantise_np(gallery, c)
    q, qq = quantise_np(queries, c)
    assert (gg > 0).all(), "a null vector cannot be a gallery row"
    ginv = np.array([inv_norm(x) for x in gg], dtype=F)
    dots = q.astype(np.int64) @ g.astype(np.int64).T
    assert np.abs(dots).max(initial=0) <= 127 * 127 * 4096
    G, n = len(g), len(q)
    top = np.zeros((n, top_k), dtype=CLS)
    top["cls"] = -1
    rows = np.full((n, top_k), -1, dtype=np.int32)
    ms = F(min_score)
    for i in range(n):
        if qq[i] == 0:
            continue
        key = dots[i].astype(F) * ginv  # element by element: (float)dot, rounded to nearest-even, then one float32 product
        qinv = inv_norm(qq[i])
        for k, r in enumerate(sorted(range(G), key=lambda r: (-key[r], r))[:top_k]):
            score = F(key[r] * qinv)
            if ms != 0 and score < ms:
                continue
            top[i, k] = (ids[r], score)
            rows[i, k] = r
    return top, rows


def ident_np(rois, top1, counts, max_det=1000):
    """the label join of tests/test_classify_cpu.py on match entries"""
    out = np.zeros((len(counts), max_det), dtype=CLS)
    out["cls"] = -1
    for k, r in enumerate(rois):
        assert 0 <= r["det"] < counts[r["frame"]]
        out[r["frame"], r["det"]] = top1[k]
    return out


# ---- exports, sizes ----------------------------------------------------------------------------------------------------------------------
def test_gallery_symbols_are_exported(marsrt):
    L = marsrt.lib()
    for n in NEW:
        assert n in marsrt.EXPORTS["mars_hip.h"], n
        assert hasattr(L, n), n
    for f in (marsrt.Gallery, marsrt.Gallery.add, marsrt.Gallery.count, marsrt.Gallery.clear, marsrt.Gallery.close, marsrt.embed_quantise,
              marsrt.match_opts, marsrt.match_vectors, marsrt.match_chunk, marsrt.Model.match_device, marsrt.Model.match_results,
              marsrt.Model.match, marsrt.Model.identify_detections, marsrt.Model.identity_results):
        assert callable(f)


def test_match_opts_layout(marsrt, tmp_path):
    import os
    import subprocess
    assert [f[0] for f in marsrt.MatchOpts._fields_] == ["top_k", "min_score", "flags"]
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    src = tmp_path / "match_abi.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "mars_hip.h"\n'
                   'int main(void){ printf("%zu %zu %zu %zu %d", sizeof(mars_hip_match_opts_t), offsetof(mars_hip_match_opts_t, top_k),\n'
                   ' offsetof(mars_hip_match_opts_t, min_score), offsetof(mars_hip_match_opts_t, flags), MARS_CLS_MAX_TOPK); return 0; }\n')
    exe = tmp_path / "match_abi"
    subprocess.run(["gcc", "-I", os.path.join(root, "include"), str(src), "-o", str(exe)], check=True)
    got = subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.split()
    O = marsrt.MatchOpts
    assert got == [str(C.sizeof(O)), str(O.top_k.offset), str(O.min_score.offset), str(O.flags.offset), str(marsrt.CLS_MAX_TOPK)]
    assert marsrt.CLS_MAX_TOPK == 8  # the classify tail's limit, reused


def test_match_chunk_is_a_function_of_the_row_count(marsrt):
    """what the GPU tests build their galleries around: a multiple of 64, never more than 256 chunks, refusals as 0"""
    for rows in (1, 17, 1024, 1025, 65536, 2 ** 20, 2 ** 24):
        ch = marsrt.match_chunk(rows)
        assert ch >= 64 and ch % 64 == 0 and (rows + ch - 1) // ch <= 256, rows
    assert marsrt.match_chunk(0) == 0 and marsrt.match_chunk(2 ** 24 + 1) == 0 and marsrt.match_chunk(-5) == 0
    ch = marsrt.match_chunk(1)
    assert marsrt.match_chunk(ch + 1) == ch and marsrt.match_chunk(3 * ch + 5) == ch  # the GPU tests' galleries around the cut


# ---- the restatement itself ---------------------------------------------------------------------------------------------------------------
def test_restated_quantisation_by_hand():
    q, qq = quantise_np([[3, -4]], 2)  # m = 4: (3 * 127 + 2) / 4 = 383 / 4 = 95;  (4 * 127 + 2) / 4 = 127
    assert q.tolist() == [[95, -127]] and qq.tolist() == [95 * 95 + 127 * 127] and qq[0] == 25154
    q, qq = quantise_np([[1]], 1)
    assert q.tolist() == [[127]] and qq.tolist() == [16129]
    q, qq = quantise_np([[0, 0, 0]], 3)
    assert q.tolist() == [[0, 0, 0]] and qq.tolist() == [0]  # null
    q, _ = quantise_np([[6, -12, 3]], 3)  # scale-invariant: the same row as 2, -4, 1
    assert q.tolist() == quantise_np([[2, -4, 1]], 3)[0].tolist() == [[64, -127, 32]]  # (2 * 127 + 2) / 4 = 64, (127 + 2) / 4 = 32
    q, qq = quantise_np([[I32_MIN, I32_MAX, 1]], 3)  # m = 2^31: ((2^31 - 1) * 127 + 2^30) / 2^31 = 127 + (2^30 - 127) / 2^31 -> 127
    assert q.tolist() == [[-127, 127, 0]]


def test_restated_match_by_hand():
    """C = 2.  Gallery rows (3, -4), (1, 0), (3, -4) again, (0, 5); query (3, -4): q = (95, -127), qq = 25154.
    dots: 25154, 95 * 127 = 12065, 25154, -127 * 127 = -16129.  The equal rows 0 and 2 tie: row 0 first"""
    gal = [[3, -4], [1, 0], [3, -4], [0, 5]]
    ids = [40, 41, 42, 43]
    top, rows = match_np(gal, ids, [[3, -4]], 2, 4)
    assert rows.tolist() == [[0, 2, 1, 3]] and top["cls"].tolist() == [[40, 42, 41, 43]]
    inv_a, inv_b = inv_norm(25154), inv_norm(16129)
    assert inv_b == F(1 / 127)
    want = [F(F(F(25154) * inv_a) * inv_a), F(F(F(25154) * inv_a) * inv_a), F(F(F(12065) * inv_b) * inv_a), F(F(F(-16129) * inv_b) * inv_a)]
    assert top["score"][0].tobytes() == np.array(want, dtype=F).tobytes()
    assert abs(float(want[0]) - 1.0) < 1e-6 and abs(float(want[2]) - 95 / np.sqrt(25154.0)) < 1e-6 and want[3] < 0
    # min_score cuts a suffix: exactly the third score keeps three entries, anything above the first keeps none
    top3, rows3 = match_np(gal, ids, [[3, -4]], 2, 4, min_score=want[2])
    assert rows3.tolist() == [[0, 2, 1, -1]] and top3["cls"].tolist() == [[40, 42, 41, -1]] and top3["score"][0, 3] == 0
    top0, rows0 = match_np(gal, ids, [[3, -4]], 2, 4, min_score=np.nextafter(want[0], F(2)))
    assert rows0.tolist() == [[-1] * 4] and (top0["cls"] == -1).all() and (top0["score"] == 0).all()
    # fewer rows than top_k, and a null query beside a real one
    top, rows = match_np(gal[:2], ids[:2], [[0, 0], [1, 0]], 2, 3)
    assert rows.tolist() == [[-1, -1, -1], [1, 0, -1]] and top["cls"].tolist() == [[-1, -1, -1], [41, 40, -1]]
    assert abs(float(top["score"][1, 0]) - 1.0) < 1e-6


# ---- the rule on the host, bit for bit ----------------------------------------------------------------------------------------------------
def embeddings(seed, n, c, bits):
    rng = np.random.default_rng(seed)
    lim = 2 ** bits
    return rng.integers(-lim, lim, (n, c), dtype=np.int64).clip(I32_MIN, I32_MAX).astype(np.int32)


@pytest.mark.parametrize("c", [1, 2, 5, 64, 65, 4096])
def test_embed_quantise_equals_the_restatement(marsrt, c):
    n = 3 if c == 4096 else 24
    cases = [embeddings(0x6A11E000 + c, n, c, 31), embeddings(0x6A11E100 + c, n, c, 9)]  # the 64-bit product; small values: many equal q
    edge = np.zeros((6, c), dtype=np.int32)
    edge[0, :] = I32_MAX
    edge[1, :] = I32_MIN  # accepted: magnitudes are taken in 64 bits
    edge[2, 0] = I32_MIN
    edge[2, -1] = I32_MAX
    edge[3, 0] = -1       # row 4 stays all zero: null
    edge[5, :] = np.arange(c) % 255 - 127
    cases.append(edge)
    # the rounding boundary: m = 254, |v| = 2 j + 1 -> |v| * 127 * 2 + m = 254 * (2 j + 2), an exact multiple of 2 m: the half rounds up
    half = np.zeros((2, c), dtype=np.int32)
    half[:, 0] = (254, -254)
    half[0, 1:] = (2 * (np.arange(c - 1) % 126) + 1)
    half[1, 1:] = -(2 * (np.arange(c - 1) % 126) + 1)
    cases.append(half)
    for v in cases:
        want_q, want_qq = quantise_np(v, c)
        q, qq = marsrt.embed_quantise(v, c)
        assert q.dtype == np.int8 and q.tobytes() == want_q.tobytes()
        assert qq.dtype == np.int32 and qq.tobytes() == want_qq.tobytes()
    if c > 1:
        q, _ = marsrt.embed_quantise(half, c)
        assert q[0, 1] == 1 and q[1, 1] == -1 and q[0, 0] == 127  # |v| = 1: (127 + 127) / 254 = 1 exactly at the half
    assert marsrt.embed_quantise(edge, c)[1][4] == 0


# ---- refusals -----------------------------------------------------------------------------------------------------------------------------
def test_gallery_bad_arguments_are_refused_up_front(marsrt):
    L = marsrt.lib()
    BAD_FILE, BAD_TENSOR = marsrt.MARS_ERR_INVALID_FILE, marsrt.MARS_ERR_INVALID_TENSOR
    P = C.POINTER(marsrt.MarsModel)
    a = marsrt.MarsModel()                     # never looked into: the refusals come first
    empty = (C.c_char * 256)()                 # stands where a gallery would: all zero reads as one without rows
    gal = C.cast(empty, C.c_void_p)
    vec = np.ones(2 * 3, dtype=np.int32)
    ids = np.zeros(2, dtype=np.int32)
    top = np.full(2 * 8, 77, dtype=marsrt.CLS_DTYPE)
    rows = np.full(2 * 8, 77, dtype=np.int32)
    q = np.full(6, 77, dtype=np.int8)

    # the rule on the host
    assert L.mars_yolo_embed_quantise(None, 2, 3, q.ctypes.data, None) == BAD_FILE
    assert L.mars_yolo_embed_quantise(vec.ctypes.data, 2, 3, None, None) == BAD_FILE
    assert L.mars_yolo_embed_quantise(vec.ctypes.data, 0, 3, q.ctypes.data, None) == BAD_FILE
    assert L.mars_yolo_embed_quantise(vec.ctypes.data, 2, 0, q.ctypes.data, None) == BAD_FILE
    assert L.mars_yolo_embed_quantise(vec.ctypes.data, 2, 4097, q.ctypes.data, None) == BAD_TENSOR
    assert (q == 77).all()
    assert L.mars_yolo_embed_quantise(vec.ctypes.data, 2, 3, q.ctypes.data, None) == marsrt.MARS_OK and (q == 127).all()  # qq may be NULL

    # the lifecycle
    out = C.c_void_p()
    assert L.mars_hip_gallery_create(64, 16, None) == BAD_FILE
    for ch, cap, code in ((0, 16, BAD_FILE), (-1, 16, BAD_FILE), (4097, 16, BAD_TENSOR), (64, 0, BAD_FILE), (64, -3, BAD_FILE),
                          (64, 2 ** 24 + 1, BAD_TENSOR)):
        assert L.mars_hip_gallery_create(ch, cap, C.byref(out)) == code, (ch, cap)
        assert not out.value
    assert L.mars_hip_gallery_add(None, vec.ctypes.data, ids.ctypes.data, 2) == BAD_FILE
    assert L.mars_hip_gallery_add(gal, None, ids.ctypes.data, 2) == BAD_FILE
    assert L.mars_hip_gallery_add(gal, vec.ctypes.data, None, 2) == BAD_FILE
    assert L.mars_hip_gallery_add(gal, vec.ctypes.data, ids.ctypes.data, 0) == BAD_FILE
    assert L.mars_hip_gallery_add(gal, vec.ctypes.data, ids.ctypes.data, 2) == BAD_TENSOR  # more rows than the capacity (0) holds
    assert L.mars_hip_gallery_count(None) == -1 and L.mars_hip_gallery_count(gal) == 0
    assert L.mars_hip_gallery_clear(None) == BAD_FILE
    L.mars_hip_gallery_free(None)

    # options
    def run(o, n=2, g=gal, v=vec, tp=top):
        return L.mars_yolo_match_vectors(g, None if v is None else v.ctypes.data, n, None if o is None else C.byref(o),
                                         None if tp is None else tp.ctypes.data, rows.ctypes.data)

    good = marsrt.match_opts(top_k=3)
    bad = [marsrt.match_opts(top_k=-1), marsrt.match_opts(top_k=9), marsrt.match_opts(min_score=-0.5), marsrt.match_opts(min_score=float("nan")),
           marsrt.match_opts(min_score=float("inf"))]
    for bit in (1, 2, 1 << 31):
        o = marsrt.match_opts()
        o.flags = bit  # no flag bit exists
        bad.append(o)
    for o in bad:
        assert run(o) == BAD_FILE
        assert L.mars_hip_match_device(C.pointer(a), gal, C.byref(o)) == BAD_FILE
        assert L.mars_hip_match(C.pointer(a), gal, C.byref(o), top.ctypes.data, None) == BAD_FILE
    assert run(None) == BAD_FILE
    for kw in (dict(n=0), dict(n=-1), dict(g=None), dict(v=None), dict(tp=None)):
        assert run(good, **kw) == BAD_FILE, kw
    assert run(good, n=65536) == BAD_TENSOR  # too many queries
    assert run(good) == BAD_TENSOR           # an empty gallery
    assert (top["cls"] == 77).all() and (rows == 77).all()  # nothing was written

    # the model forms
    assert L.mars_hip_match_device(P(), gal, C.byref(good)) == BAD_FILE
    assert L.mars_hip_match_device(C.pointer(a), None, C.byref(good)) == BAD_FILE
    assert L.mars_hip_match_device(C.pointer(a), gal, None) == BAD_FILE
    assert L.mars_hip_match(P(), gal, C.byref(good), top.ctypes.data, None) == BAD_FILE
    assert L.mars_hip_match(C.pointer(a), None, C.byref(good), top.ctypes.data, None) == BAD_FILE
    assert L.mars_hip_match(C.pointer(a), gal, None, top.ctypes.data, None) == BAD_FILE
    assert L.mars_hip_match(C.pointer(a), gal, C.byref(good), None, None) == BAD_FILE
    assert L.mars_hip_match_results(P(), top.ctypes.data, None) == BAD_FILE
    assert L.mars_hip_match_results(C.pointer(a), None, None) == BAD_FILE
    assert L.mars_hip_identify_detections_device(P(), C.pointer(a)) == BAD_FILE
    assert L.mars_hip_identify_detections_device(C.pointer(a), P()) == BAD_FILE
    assert L.mars_hip_identify_detections_device(C.pointer(a), C.pointer(a)) == BAD_TENSOR  # det_model == cls_model
    assert L.mars_hip_identity_results(P(), top.ctypes.data) == BAD_FILE
    assert L.mars_hip_identity_results(C.pointer(a), None) == BAD_FILE
