"""The byte-moving kernels of csrc/hip/move.hip, and the layout dispatch of csrc/hip/eltwise.hip, one launcher call at a time: every
branch a launcher can take (vector width from channel counts and the alignment of pointers, strides and offsets; special forms; limits)
against tests/moveref.py, byte for byte.  An id names the branch, the comment above a table the launcher condition that selects it.

Every operand lives in an allocation laid out [256 guard bytes][payload][256 guard bytes].  Outputs are pre-filled with 0x5A: after a call
both guards still hold it, and so does every payload byte the restatement does not write (between frames, outside a slice, behind
rows_only rows).  Input guards and the padding between frames hold +127 for the pools (an over-read would win a maximum), random bytes for
the copies.  No case starts a kernel with arguments its launcher is not meant to take; refusals are asserted only where the launcher returns
before any launch.  The tables and input builders need no GPU: tests/test_move_cpu.py checks the same cases against the CPU oracle."""
import ctypes as C
import zlib

import numpy as np
import pytest

import moveref as R

pytestmark = pytest.mark.gpu

U8, I8 = np.uint8, np.int8
SENT = 0x5A
GUARD = 256


def seed_of(cid):
    return zlib.crc32(cid.encode()) & 0xFFFF


def align16(n):
    return (n + 15) & ~15


def name_of(t):
    return "x".join("_".join(str(q) for q in v) if isinstance(v, tuple) else str(v) for v in t)


# ---- device memory --------------------------------------------------------------------------------------------------------------------------
def declare(L):
    """prototypes of the launchers and of the library's own allocation / copy calls (csrc/mhip.h): pointers as c_void_p, strides as c_size_t"""
    P, Z, I, F = C.c_void_p, C.c_size_t, C.c_int, C.c_float
    L.mhip_malloc.restype = P
    L.mhip_malloc.argtypes = [Z]
    L.mhip_free.restype = None
    L.mhip_free.argtypes = [P]
    for n, a in (("mhip_h2d_async", [P, P, Z]), ("mhip_d2h_async", [P, P, Z]), ("mhip_sync", []),
                 ("mhip_maxpool_i8", [P, Z, P, Z] + [I] * 12),
                 ("mhip_pool_chain_i8", [P, Z, C.POINTER(P), C.POINTER(Z)] + [I] * 7),
                 ("mhip_unpad_rows", [P, P, Z, I, I]),
                 ("mhip_concat_slice", [P, Z, P, Z] + [I] * 6),
                 ("mhip_upsample_i8", [P, Z, P, Z] + [I] * 10),
                 ("mhip_nchw_to_nhwc_pad", [P, Z, P, Z] + [I] * 4),
                 ("mhip_concat_nchwq", [C.POINTER(P), C.POINTER(Z), C.POINTER(I), I, P, Z] + [I] * 5),
                 ("mhip_upsample_nchwq", [P, Z, I, I, I, P, Z] + [I] * 11),
                 ("mhip_maxpool_nchwq", [P, Z, P, Z] + [I] * 6),
                 ("mhip_lut_i8", [P, Z, P, Z, I, Z, P]),
                 ("mhip_relu_bytes", [P, Z, I, Z]),
                 ("mhip_binary_i8", [I, P, Z, P, Z, P, Z, I, Z, F, F, F, I, I, I])):
        f = getattr(L, n)
        f.restype, f.argtypes = I, a
    return L


class Dev:
    """[256 guard bytes][payload][256 guard bytes] in HBM; the payload starts `off` bytes behind a 256-byte boundary.  guard: one byte value,
    or 512 bytes (those in front, then those behind)"""

    def __init__(self, L, payload, off=0, guard=SENT):
        payload = np.ascontiguousarray(payload).reshape(-1).view(U8)
        g = np.full(2 * GUARD, guard, dtype=U8) if np.isscalar(guard) else np.ascontiguousarray(guard).reshape(-1).view(U8)
        assert 0 <= off < 256 and len(g) == 2 * GUARD
        self.L, self.n = L, len(payload)
        self.image = np.concatenate([g[:GUARD], payload, g[GUARD:]])
        self.raw = L.mhip_malloc(len(self.image) + 512)
        assert self.raw, "mhip_malloc"
        self.lo = ((self.raw + 255) & ~255) + off
        self.ptr = self.lo + GUARD
        assert L.mhip_h2d_async(self.lo, self.image.ctypes.data, len(self.image)) == 0 and L.mhip_sync() == 0

    def read(self, what):
        """the payload as the device holds it now; the guards must be what went up"""
        got = np.empty_like(self.image)
        assert self.L.mhip_sync() == 0
        assert self.L.mhip_d2h_async(got.ctypes.data, self.lo, len(got)) == 0 and self.L.mhip_sync() == 0
        same(what + ": guard in front", got[:GUARD], self.image[:GUARD])
        same(what + ": guard behind", got[GUARD + self.n:], self.image[GUARD + self.n:])
        return got[GUARD:GUARD + self.n]

    def unchanged(self, what):
        same(what + ": an input changed", self.read(what), self.image[GUARD:GUARD + self.n])

    def free(self):
        if self.raw:
            self.L.mhip_free(self.raw)
            self.raw = None


@pytest.fixture
def hbm(gpu):
    L = declare(gpu.lib())
    made = []

    def make(payload, off=0, guard=SENT):
        made.append(Dev(L, payload, off, guard))
        return made[-1]

    make.L = L
    yield make
    for d in made:
        d.free()


def same(what, got, want):
    got, want = np.asarray(got).reshape(-1).view(U8), np.asarray(want).reshape(-1).view(U8)
    assert len(got) == len(want), (what, len(got), len(want))
    bad = np.flatnonzero(got != want)
    if len(bad):
        pytest.fail("%s: %d of %d bytes differ; first (index, got, want): %s"
                    % (what, len(bad), len(got), [(int(i), int(got[i]), int(want[i])) for i in bad[:6]]))


def strided(frames, stride, fill):
    """frames[f] at f * stride of one payload; every other byte is `fill` (one value) or random (fill = a seed as a 1-tuple)"""
    n = len(frames) * stride
    out = R.random_bytes(fill[0], n).view(U8) if isinstance(fill, tuple) else np.full(n, fill, dtype=U8)
    for f, x in enumerate(frames):
        assert len(x) <= stride
        out[f * stride:f * stride + len(x)] = np.asarray(x).view(U8)
    return out


def pool_in(hbm, frames, stride, off=0):
    """pool operands: +127 between the frames and in both guards"""
    return hbm(strided(frames, stride, 127), off, guard=127)


def copy_in(hbm, frames, stride, seed, off=0):
    return hbm(strided(frames, stride, (seed + 77,)), off, guard=R.random_bytes(seed + 78, 2 * GUARD))


def sentinel(n):
    return np.full(n, SENT, dtype=U8)


def copy_frames(cid, frames, n, k=0):
    """frame f of input k of a copy case: its own seed each, so that no mix-up of frames or inputs cancels"""
    return [R.random_bytes(seed_of(cid) * 64 + f * 4 + k, n) for f in range(frames)]


# ---- mhip_maxpool_i8 ------------------------------------------------------------------------------------------------------------------------
# (in_h, in_w, ch, out_h, out_w, kh, kw, sh, sw), then: in_off / out_off = bytes added to the pointer, pstride / choff = the slice output,
# odd = in_stride is the frame + 1.  The launcher: A16 / A4 = both pointers, both strides, pstride and choff multiples of 16 / 4;
#   v16 = ch % 16 == 0 and A16;  v4 = ch % 4 == 0 and A4
#   rows form  (maxpool_rows_kernel)  : not v16, v4, strides 1 x 1, dense output, 1 <= kh <= MP_KMAX = 8, kw >= 1, out <= in both ways
#   else v16   (maxpool16_kernel), else v4 (maxpool_kernel<4>), else maxpool_kernel<1>
MAXPOOL = {
    "v16_s2": ((7, 9, 16, 4, 5, 3, 3, 2, 2), {}),                          # windows clipped right and bottom
    "v16_s2_2x2": ((7, 9, 32, 4, 5, 2, 2, 2, 2), {}),
    "v16_slice": ((6, 5, 16, 6, 5, 5, 5, 1, 1), dict(pstride=48, choff=16)),
    "v16_to_rows": ((6, 5, 16, 6, 5, 3, 3, 1, 1), dict(in_off=4)),         # A16 fails, A4 holds, stride 1, dense: the rows form
    "v16_to_v4": ((7, 9, 16, 4, 5, 3, 3, 2, 2), dict(out_off=4)),          # A16 fails, stride 2: maxpool_kernel<4>
    "v16_to_v1": ((7, 9, 16, 4, 5, 3, 3, 2, 2), dict(in_off=1)),           # A4 fails: maxpool_kernel<1>
    "rows_c4": ((9, 7, 4, 9, 7, 3, 3, 1, 1), {}),
    "rows_c12_kmax": ((17, 5, 12, 17, 5, 8, 2, 1, 1), {}),                 # kh = MP_KMAX; 17 rows = 2 strips of MP_RPT = 8 and 1
    "rows_k9_falls_back": ((17, 5, 12, 17, 5, 9, 2, 1, 1), {}),            # kh = 9 > MP_KMAX: maxpool_kernel<4>
    "rows_kw_gt_w": ((5, 3, 20, 5, 3, 2, 7, 1, 1), {}),                    # a window wider than the map
    "rows_out_smaller": ((10, 8, 20, 8, 7, 3, 2, 1, 1), {}),               # out < in both ways
    "rows_h_lt_strip": ((3, 4, 8, 3, 4, 5, 5, 1, 1), {}),                  # out_h < MP_RPT
    "v4_s2": ((9, 9, 12, 5, 5, 3, 3, 2, 2), {}),
    "v4_slice_c20": ((6, 6, 20, 6, 6, 2, 2, 1, 1), dict(pstride=44, choff=24)),  # a slice keeps it off the rows form
    "v1_c3": ((7, 6, 3, 7, 6, 3, 3, 1, 1), {}),
    "v1_c5_s2": ((7, 6, 5, 4, 3, 2, 2, 2, 2), {}),
    "v1_stride_odd": ((5, 5, 4, 5, 5, 3, 3, 1, 1), dict(odd=True)),        # ch % 4 == 0 but in_stride = frame + 1
}
POOL_FRAMES = 3


def maxpool_frames(cid):
    in_h, in_w, ch = MAXPOOL[cid][0][:3]
    return R.pool_frames(seed_of(cid), POOL_FRAMES, in_h, in_w, ch)


def maxpool_want(cid, xs=None):
    """dense results, frame by frame"""
    return [R.maxpool(x, *MAXPOOL[cid][0]) for x in (maxpool_frames(cid) if xs is None else xs)]


@pytest.mark.parametrize("cid", list(MAXPOOL))
def test_maxpool_i8(hbm, cid):
    (in_h, in_w, ch, out_h, out_w, kh, kw, sh, sw), o = MAXPOOL[cid]
    xs = maxpool_frames(cid)
    n_in = in_h * in_w * ch
    in_stride = n_in + 1 if o.get("odd") else align16(n_in) + 32
    pstride, choff = o.get("pstride", 0), o.get("choff", 0)
    npix, ps = out_h * out_w, o.get("pstride", ch)
    out_stride = align16(npix * ps) + 48
    a = pool_in(hbm, xs, in_stride, o.get("in_off", 0))
    d = hbm(sentinel(POOL_FRAMES * out_stride), o.get("out_off", 0))
    assert hbm.L.mhip_maxpool_i8(a.ptr, in_stride, d.ptr, out_stride, POOL_FRAMES, in_h, in_w, ch, out_h, out_w, kh, kw, sh, sw, pstride, choff) == 0
    want = sentinel(POOL_FRAMES * out_stride).view(I8)
    for f, w in enumerate(maxpool_want(cid, xs)):
        R.place(want[f * out_stride:], w, npix, ch, ps, choff)
    same("maxpool_i8 " + cid, d.read(cid), want)
    a.unchanged(cid)


def test_maxpool_i8_refusals_and_empty(hbm):
    a, d = pool_in(hbm, [np.zeros(64, I8)], 64), hbm(sentinel(256))
    L = hbm.L
    assert L.mhip_maxpool_i8(a.ptr, 64, d.ptr, 256, 1, 2, 2, 16, 2, 2, 2, 2, 1, 1, 31, 16) == -1  # out_pix_stride < out_ch_off + ch
    assert L.mhip_maxpool_i8(a.ptr, 64, d.ptr, 256, 1, 2, 2, 16, 0, 2, 2, 2, 1, 1, 0, 0) == 0     # out_h = 0: nothing to do
    same("maxpool_i8 out_h = 0", d.read("empty"), sentinel(256))


# ---- mhip_pool_chain_i8 -----------------------------------------------------------------------------------------------------------------------
# (h, w, ch, kh, kw, n, frames).  The launcher takes ch % 16 == 0, 1 <= n <= 3, 16-byte aligned pointers and strides and h * w <= 960 (two
# planes of h * w * 8 dwords in 60 KiB of LDS); workgroup id -> frame (slot / ncg) * 8 + (id & 7), channel group slot % ncg with slot = id >> 3
# and ncg = ch / 16: frames 8, 9 and 17 are where a second round of eight begins.
POOL_CHAIN = [(3, 5, 16, 2, 2, 1, 1), (20, 20, 16, 5, 5, 3, 7), (20, 20, 16, 5, 5, 3, 8), (6, 7, 48, 3, 3, 3, 9), (6, 7, 32, 2, 7, 2, 17),
              (1, 1, 16, 5, 5, 3, 3),
              (30, 32, 16, 5, 5, 3, 2),   # h * w = 960: the LDS limit
              (4, 4, 16, 9, 9, 3, 3)]     # a window larger than the map


def chain_frames(case):
    h, w, ch, kh, kw, n, frames = case
    return R.pool_frames(seed_of(name_of(case)), frames, h, w, ch)


def chain_want(case, xs=None, kh=None, kw=None):
    """[stage][frame]"""
    h, w, ch, kh0, kw0, n, frames = case
    cur, stages = list(chain_frames(case) if xs is None else xs), []
    for _ in range(n):
        cur = [R.maxpool(x, h, w, ch, h, w, kh or kh0, kw or kw0, 1, 1) for x in cur]
        stages.append(cur)
    return stages


def call_chain(hbm, a, in_stride, outs, strides, n, frames, h, w, ch, kh, kw):
    po = (C.c_void_p * 3)(*[o.ptr if o is not None else None for o in outs])
    ps = (C.c_size_t * 3)(*strides)
    return hbm.L.mhip_pool_chain_i8(a.ptr, in_stride, po, ps, n, frames, h, w, ch, kh, kw)


@pytest.mark.parametrize("case", POOL_CHAIN, ids=name_of)
def test_pool_chain_i8(hbm, case):
    h, w, ch, kh, kw, n, frames = case
    xs = chain_frames(case)
    nb = h * w * ch
    in_stride = nb + 32
    strides = [nb + 16 * (i + 1) if i < n else 0 for i in range(3)]  # a stride of its own per stage
    a = pool_in(hbm, xs, in_stride)
    outs = [hbm(sentinel(frames * strides[i])) if i < n else None for i in range(3)]
    assert call_chain(hbm, a, in_stride, outs, strides, n, frames, h, w, ch, kh, kw) == 0
    for i, stage in enumerate(chain_want(case, xs)):
        got = outs[i].read("%s stage %d" % (name_of(case), i))
        for f in range(frames):  # frame by frame: a wrong frame mapping is named
            same("pool_chain %s stage %d frame %d" % (name_of(case), i, f), got[f * strides[i]:f * strides[i] + nb], stage[f])
        same("pool_chain %s stage %d" % (name_of(case), i), got, strided(stage, strides[i], SENT))
    a.unchanged(name_of(case))


def test_pool_chain_i8_refusals(hbm):
    a = pool_in(hbm, [np.zeros(1024, I8)], 1024)
    outs = [hbm(sentinel(1024)) for _ in range(3)]
    args = dict(h=2, w=2, ch=16, n=3)
    for bad in (dict(h=31, w=31), dict(ch=24), dict(n=4)):  # h * w = 961 > 960; ch % 16 != 0; n > 3
        k = dict(args, **bad)
        assert call_chain(hbm, a, 1024, outs, [1024] * 3, k["n"], 1, k["h"], k["w"], k["ch"], 5, 5) == -1, bad
    for o in outs:
        same("pool_chain refusals", o.read("refusals"), sentinel(1024))


# ---- mhip_unpad_rows --------------------------------------------------------------------------------------------------------------------------
# (rows, width, pitch): one thread per 16 source bytes; a chunk that lies inside the row is one unaligned 16-byte store, the row's last chunk
# goes byte by byte.  The launcher takes pitch >= width, pitch % 16 == 0 and a 16-byte aligned source.
UNPAD = [(1, 1, 16), (3, 15, 16), (3, 16, 16), (5, 17, 32), (4, 255, 256), (1000, 85, 96), (2, 33, 64)]


@pytest.mark.parametrize("case", UNPAD, ids=name_of)
def test_unpad_rows(hbm, case):
    rows, width, pitch = case
    src = R.random_bytes(seed_of(name_of(case)), rows * pitch)
    a = hbm(src, guard=R.random_bytes(seed_of(name_of(case)) + 1, 2 * GUARD))
    d = hbm(sentinel(rows * width))  # dense: ends at rows * width, the guard right behind it
    assert hbm.L.mhip_unpad_rows(a.ptr, d.ptr, rows, width, pitch) == 0
    same("unpad_rows " + name_of(case), d.read(name_of(case)), R.unpad_rows(src, rows, width, pitch))
    a.unchanged(name_of(case))


def test_unpad_rows_refusals(hbm):
    a, d = hbm(np.zeros(256, U8)), hbm(sentinel(256))
    assert hbm.L.mhip_unpad_rows(a.ptr, d.ptr, 2, 20, 16) == -1  # pitch < width
    assert hbm.L.mhip_unpad_rows(a.ptr, d.ptr, 2, 20, 24) == -1  # pitch % 16 != 0
    same("unpad_rows refusals", d.read("refusals"), sentinel(256))


# ---- mhip_concat_slice ------------------------------------------------------------------------------------------------------------------------
# (out_h, out_w, in_c, out_c, ch_off), then in_off / out_off and s4 = in_stride = 4 (mod 8).  The launcher: width V in 16, 8, 4 is taken when
# in_c, out_c and ch_off are multiples of V and so are both pointers and both strides; the widest that holds; else bytes.
V16 = (3, 5, 16, 48, 32)
CONCAT = {
    "v16": (V16, {}),
    "v8": ((3, 5, 40, 80, 40), {}),        # the float twins' 40-byte rows
    "v8_24": ((2, 3, 16, 40, 24), {}),
    "v4": ((3, 5, 20, 60, 40), {}),
    "v1": ((3, 5, 3, 8, 5), {}),
    "v16_to_v8": (V16, dict(out_off=8)),
    "v16_to_v4": (V16, dict(s4=True)),
    "v16_to_v1": (V16, dict(in_off=1)),
}
COPY_FRAMES = 3


@pytest.mark.parametrize("cid", list(CONCAT))
def test_concat_slice(hbm, cid):
    (out_h, out_w, in_c, out_c, ch_off), o = CONCAT[cid]
    npix = out_h * out_w
    xs = copy_frames(cid, COPY_FRAMES, npix * in_c)
    in_stride = align16(npix * in_c) + (20 if o.get("s4") else 16)
    out_stride = align16(npix * out_c) + 32
    a = copy_in(hbm, xs, in_stride, seed_of(cid), o.get("in_off", 0))
    d = hbm(sentinel(COPY_FRAMES * out_stride), o.get("out_off", 0))
    assert hbm.L.mhip_concat_slice(a.ptr, in_stride, d.ptr, out_stride, COPY_FRAMES, out_h, out_w, in_c, out_c, ch_off) == 0
    want = sentinel(COPY_FRAMES * out_stride).view(I8)
    for f in range(COPY_FRAMES):
        R.concat_slice(want[f * out_stride:], xs[f], out_h, out_w, in_c, out_c, ch_off)
    same("concat_slice " + cid, d.read(cid), want)
    a.unchanged(cid)


# ---- mhip_upsample_i8 -------------------------------------------------------------------------------------------------------------------------
# (in_h, in_w, ch, out_h, out_w, scale_h, scale_w), then the slice output and pointer offsets.  The launcher: as the max-pool's v16 / v4 / bytes
# (ch and the alignment of both pointers, both strides, pstride and choff), no special form.
UPSAMPLE = {
    "v16_2x2": ((3, 4, 16, 6, 8, 2, 2), {}),
    "v16_clamp": ((3, 4, 16, 7, 9, 2, 2), {}),          # the last row and column clamp to in_h - 1, in_w - 1
    "v4_3x1": ((2, 5, 20, 6, 5, 3, 1), {}),
    "v1_2x3": ((3, 3, 3, 6, 9, 2, 3), {}),
    "v16_slice": ((3, 4, 16, 6, 8, 2, 2), dict(pstride=48, choff=32)),
    "v16_to_v4": ((3, 4, 16, 6, 8, 2, 2), dict(in_off=4)),
    "v16_to_v1": ((3, 4, 16, 6, 8, 2, 2), dict(in_off=1)),
}


@pytest.mark.parametrize("cid", list(UPSAMPLE))
def test_upsample_i8(hbm, cid):
    (in_h, in_w, ch, out_h, out_w, sh, sw), o = UPSAMPLE[cid]
    n_in, npix, ps, choff = in_h * in_w * ch, out_h * out_w, o.get("pstride", ch), o.get("choff", 0)
    xs = copy_frames(cid, COPY_FRAMES, n_in)
    in_stride, out_stride = align16(n_in) + 16, align16(npix * ps) + 32
    a = copy_in(hbm, xs, in_stride, seed_of(cid), o.get("in_off", 0))
    d = hbm(sentinel(COPY_FRAMES * out_stride))
    assert hbm.L.mhip_upsample_i8(a.ptr, in_stride, d.ptr, out_stride, COPY_FRAMES, in_h, in_w, ch, out_h, out_w, sh, sw, o.get("pstride", 0), choff) == 0
    want = sentinel(COPY_FRAMES * out_stride).view(I8)
    for f in range(COPY_FRAMES):
        R.place(want[f * out_stride:], R.upsample(xs[f], in_h, in_w, ch, out_h, out_w, sh, sw), npix, ch, ps, choff)
    same("upsample_i8 " + cid, d.read(cid), want)
    a.unchanged(cid)


# ---- mhip_nchw_to_nhwc_pad --------------------------------------------------------------------------------------------------------------------
# (c, hw, c_pad), in_off, bytewise = under MARS_HIP_NCHW_BYTEWISE (read on every call).  The launcher: dwords = hw % 4 == 0 and input pointer
# and stride multiples of 4.  c_pad = 4: nchw_to_nhwc_c4_kernel, refused without dwords.  Else dwords and no MARS_HIP_NCHW_BYTEWISE:
# nchw_to_nhwc4_kernel; else the byte-wise nchw_to_nhwc_kernel.  The output pointer and stride are multiples of 16 in every form.
RELAYOUT = {
    "c4_1x4": ((1, 4, 4), {}), "c4_3x36": ((3, 36, 4), {}), "c4_4x1028": ((4, 1028, 4), {}),
    "dw_5x4": ((5, 4, 16), {}), "dw_16x36": ((16, 36, 16), {}), "dw_17x36": ((17, 36, 32), {}), "dw_40x1028": ((40, 1028, 48), {}),
    "bytes_hw_odd": ((17, 35, 32), {}),
    "bytes_in_plus1": ((16, 36, 16), dict(in_off=1)),
    "bytes_by_env": ((17, 36, 32), dict(bytewise=True)),  # both forms on the same bytes
}


@pytest.mark.parametrize("cid", list(RELAYOUT))
def test_nchw_to_nhwc_pad(hbm, cid, monkeypatch):
    (c, hw, c_pad), o = RELAYOUT[cid]
    monkeypatch.delenv("MARS_HIP_NCHW_BYTEWISE", raising=False)
    xs = copy_frames(cid, COPY_FRAMES, c * hw)
    in_stride = ((c * hw + 3) & ~3) + 8 if hw % 4 == 0 else c * hw + 3
    out_stride = hw * c_pad + 32
    a = copy_in(hbm, xs, in_stride, seed_of(cid), o.get("in_off", 0))
    want = strided([R.nchw_to_nhwc_pad(x, c, hw, c_pad) for x in xs], out_stride, SENT)  # (pad channels: 0)
    got = []
    for env in ((None, "1") if o.get("bytewise") else (None,)):
        if env:
            monkeypatch.setenv("MARS_HIP_NCHW_BYTEWISE", env)
        d = hbm(sentinel(COPY_FRAMES * out_stride))
        assert hbm.L.mhip_nchw_to_nhwc_pad(a.ptr, in_stride, d.ptr, out_stride, COPY_FRAMES, c, hw, c_pad) == 0
        got.append(d.read(cid))
        same("nchw_to_nhwc_pad %s%s" % (cid, " (byte-wise)" if env else ""), got[-1], want)
    if o.get("bytewise"):
        same("nchw_to_nhwc_pad: dword form against byte-wise form", got[0], got[1])
    a.unchanged(cid)


def test_nchw_to_nhwc_pad_refusal(hbm):
    a, d = hbm(np.zeros(256, U8)), hbm(sentinel(256))
    assert hbm.L.mhip_nchw_to_nhwc_pad(a.ptr, 108, d.ptr, 144, 1, 3, 35, 4) == -1  # c_pad = 4 and hw % 4 != 0
    same("nchw_to_nhwc_pad refusal", d.read("refusal"), sentinel(256))


# ---- mhip_concat_nchwq ------------------------------------------------------------------------------------------------------------------------
# (in_c per input, H, W, rows_only); inputs and output pixels x channels.  One kernel, two paths per thread (16 channels of one pixel): map rows
# h >= N - 1 take one 16-byte load from the last input (zeros where c0 >= in_c[last]), rows h < N - 1 go byte by byte over all inputs.
# rows_only in 1 .. H - 1 limits the launch to the first rows_only map rows; anything else is the whole map.
CONCATQ = [((16,), 3, 4, 0), ((16, 16), 5, 3, 0), ((32, 16, 16), 2, 7, 0),
           ((16, 16, 16, 16), 2, 4, 0),  # H < N - 1: every byte by the slow path
           ((16, 48), 1, 5, 0),
           ((48, 16), 6, 5, 0),          # c0 >= in_c[last]: the zero fill of the fast path
           ((16, 32), 6, 5, 1),          # rows_only = N - 1: rows >= 1 keep the sentinel
           ((16, 32), 6, 5, 6),          # rows_only = H: the whole map
           ((16, 32), 6, 5, 9)]          # rows_only > H: the whole map


def concatq_frames(case):
    """[frame][input]: the inputs' NCHW bytes"""
    in_cs, H, W, _ = case
    per_input = [copy_frames(name_of(case), COPY_FRAMES, c * H * W, k) for k, c in enumerate(in_cs)]
    return [[per_input[k][f] for k in range(len(in_cs))] for f in range(COPY_FRAMES)]


@pytest.mark.parametrize("case", CONCATQ, ids=name_of)
def test_concat_nchwq(hbm, case):
    in_cs, H, W, rows_only = case
    N, out_c, cid = len(in_cs), sum(in_cs), name_of(case)
    xs = concatq_frames(case)
    in_strides = [c * H * W + 16 * (k + 1) for k, c in enumerate(in_cs)]
    ins = [copy_in(hbm, [R.to_pxc(xs[f][k], in_cs[k], H, W) for f in range(COPY_FRAMES)], in_strides[k], seed_of(cid) + 8 * k) for k in range(N)]
    out_stride = out_c * H * W + 32
    d = hbm(sentinel(COPY_FRAMES * out_stride))
    rc = hbm.L.mhip_concat_nchwq((C.c_void_p * 4)(*[a.ptr for a in ins]), (C.c_size_t * 4)(*in_strides), (C.c_int * 4)(*in_cs), N, d.ptr, out_stride,
                                 COPY_FRAMES, out_c, H, W, rows_only)
    assert rc == 0
    rows = rows_only if 0 < rows_only < H else H
    want = sentinel(COPY_FRAMES * out_stride).view(I8)
    for f in range(COPY_FRAMES):  # the flat-byte concat of the NCHW bytes, then pixels x channels; its first `rows` map rows
        want[f * out_stride:f * out_stride + rows * W * out_c] = R.to_pxc(R.concat_q(xs[f], in_cs, H, W), out_c, H, W)[:rows * W * out_c]
    same("concat_nchwq " + cid, d.read(cid), want)
    for a in ins:
        a.unchanged(cid)


# ---- mhip_upsample_nchwq ----------------------------------------------------------------------------------------------------------------------
# ((Ci, Hi, Wi), (Co, Ho, Wo), sh, sw); the q-arguments are the reference's view of the two tensors: qih = Ci, qiw = Hi, qch = Wi, qoh = Co,
# qow = Ho.  The launcher: Co == Ci, Ho == 2 Hi, Wo == 2 Wi, factors 2 x 2, Ci % 32 == 0, aligned input and no MARS_HIP_UPSAMPLE_GENERIC (read
# on every call): upsample_nchwq_tile2_kernel; else the byte-by-byte upsample_nchwq_kernel.  Bytes behind qoh * qow * qch are written as 0.
UPSAMPLEQ = {
    "tile2_32": ((32, 3, 4), (32, 6, 8), 2, 2),
    "tile2_64_zero_half": ((64, 2, 2), (64, 4, 4), 2, 2),  # channel groups c0 >= C / 2 are zero
    "gen_c16": ((16, 3, 4), (16, 6, 8), 2, 2),             # Ci % 32 != 0
    "gen_3x3": ((16, 3, 5), (16, 9, 15), 3, 3),
    "gen_1x2": ((16, 4, 3), (16, 4, 6), 1, 2),
    "gen_clamp": ((32, 3, 4), (32, 7, 8), 2, 2),           # Ho odd: the column clamp ix > qiw - 1; generic because Ho != 2 Hi
    "gen_co_ne_ci": ((16, 3, 4), (32, 6, 4), 2, 2),        # Co != Ci
}


@pytest.mark.parametrize("cid", list(UPSAMPLEQ))
def test_upsample_nchwq(hbm, cid, monkeypatch):
    (ci, hi, wi), (co, ho, wo), sh, sw = UPSAMPLEQ[cid]
    monkeypatch.delenv("MARS_HIP_UPSAMPLE_GENERIC", raising=False)
    xs = copy_frames(cid, COPY_FRAMES, ci * hi * wi)
    in_stride, out_stride = ci * hi * wi + 16, co * ho * wo + 32
    a = copy_in(hbm, [R.to_pxc(x, ci, hi, wi) for x in xs], in_stride, seed_of(cid))
    want = strided([R.to_pxc(R.upsample_q(x, ci, hi, wi, co, ho, wo, sh, sw), co, ho, wo) for x in xs], out_stride, SENT)
    got = []
    for env in ((None, "1") if cid.startswith("tile2") else (None,)):
        if env:
            monkeypatch.setenv("MARS_HIP_UPSAMPLE_GENERIC", env)
        d = hbm(sentinel(COPY_FRAMES * out_stride))
        assert hbm.L.mhip_upsample_nchwq(a.ptr, in_stride, ci, hi, wi, d.ptr, out_stride, co, ho, wo, COPY_FRAMES, ci, hi, wi, co, ho, sh, sw) == 0
        got.append(d.read(cid))
        same("upsample_nchwq %s%s" % (cid, " (generic)" if env else ""), got[-1], want)
    if len(got) == 2:
        same("upsample_nchwq: tile2 form against generic form", got[0], got[1])
    a.unchanged(cid)


# ---- mhip_maxpool_nchwq -----------------------------------------------------------------------------------------------------------------------
# (C, H, W, kh, kw): stride 1, output = input size; kh runs over CHANNELS and kw over map rows of one column (the reference on an NCHW-tagged
# tensor).  The launcher takes C % 16 == 0 and 1 <= kh <= 17; kw == 5: maxpool_nchwq_kernel<5> (with a fixed five-term channel maximum where
# kh == 5 too), any other kw: the generic maxpool_nchwq_kernel<0>.  (MARS_HIP_MAXPOOL_Q_GENERIC is latched at the first call: not toggled here.)
MAXPOOLQ = {
    "k5x5": (16, 4, 3, 5, 5),
    "k5x5_two_loads": (32, 2, 1, 5, 5),  # H < kw: the row clamp H - 1 - h; a second 16-byte load
    "kw5_kh3": (48, 6, 5, 3, 5),
    "kw5_kh17": (48, 6, 5, 17, 5),       # the channel window at its limit inside <5>
    "gen_3x7": (48, 6, 5, 3, 7),
    "gen_17x3": (32, 5, 4, 17, 3),
    "gen_16x1": (16, 5, 4, 16, 1),       # a window running off the only channel group
    "gen_1x1": (16, 3, 3, 1, 1),         # identity
}


def maxpoolq_frames(cid):
    """NCHW bytes"""
    c, h, w = MAXPOOLQ[cid][:3]
    return R.pool_frames(seed_of(cid), POOL_FRAMES, c, h, w)


@pytest.mark.parametrize("cid", list(MAXPOOLQ))
def test_maxpool_nchwq(hbm, cid):
    c, h, w, kh, kw = MAXPOOLQ[cid]
    xs = maxpoolq_frames(cid)
    nb = c * h * w
    in_stride, out_stride = nb + 16, nb + 32
    a = pool_in(hbm, [R.to_pxc(x, c, h, w) for x in xs], in_stride)
    d = hbm(sentinel(POOL_FRAMES * out_stride))
    assert hbm.L.mhip_maxpool_nchwq(a.ptr, in_stride, d.ptr, out_stride, POOL_FRAMES, c, h, w, kh, kw) == 0
    same("maxpool_nchwq " + cid, d.read(cid), strided([R.to_pxc(R.maxpool_q(x, c, h, w, kh, kw), c, h, w) for x in xs], out_stride, SENT))
    a.unchanged(cid)


def test_maxpool_nchwq_refusals(hbm):
    a, d = pool_in(hbm, [np.zeros(512, I8)], 512), hbm(sentinel(512))
    assert hbm.L.mhip_maxpool_nchwq(a.ptr, 512, d.ptr, 512, 1, 16, 2, 2, 18, 5) == -1  # kh > 17
    assert hbm.L.mhip_maxpool_nchwq(a.ptr, 512, d.ptr, 512, 1, 24, 2, 2, 5, 5) == -1   # C % 16 != 0
    same("maxpool_nchwq refusals", d.read("refusals"), sentinel(512))


# ---- eltwise.hip: where the bytes land ----------------------------------------------------------------------------------------------------------
# mhip_lut_i8 / mhip_relu_bytes: a thread owns 16 bytes; vec = pointers and strides multiples of 16 -> 16-byte body and a byte tail of n % 16,
# else every byte on its own.
ELT_N = [1, 15, 16, 17, 4096 + 5]


@pytest.mark.parametrize("off", [0, 1], ids=["aligned", "plus1"])
@pytest.mark.parametrize("n", ELT_N)
def test_lut_i8_layout(hbm, n, off):
    rng = np.random.default_rng(n * 2 + off)
    lut = rng.permutation(256).astype(U8)  # a permutation: no wrong index maps to the right byte
    xs = copy_frames("lut%d_%d" % (n, off), COPY_FRAMES, n)
    in_stride, out_stride = align16(n) + 16, align16(n) + 32
    a = copy_in(hbm, xs, in_stride, n + off, off)
    t = hbm(lut)
    d = hbm(sentinel(COPY_FRAMES * out_stride), off)
    assert hbm.L.mhip_lut_i8(a.ptr, in_stride, d.ptr, out_stride, COPY_FRAMES, n, t.ptr) == 0
    same("lut_i8 n %d pointer + %d" % (n, off), d.read("lut"), strided([lut[(x.astype(np.int32) + 128) & 255] for x in xs], out_stride, SENT))
    a.unchanged("lut")


@pytest.mark.parametrize("off", [0, 1], ids=["aligned", "plus1"])
@pytest.mark.parametrize("n", ELT_N)
def test_relu_bytes_layout(hbm, n, off):
    """in place: the bytes between the frames and the guards hold 0xA5, which a stray ReLU would zero (0x5A is positive: it would not show)"""
    xs = copy_frames("relu%d_%d" % (n, off), COPY_FRAMES, n)
    stride = align16(n) + 16
    d = hbm(strided(xs, stride, 0xA5), off, guard=0xA5)
    assert hbm.L.mhip_relu_bytes(d.ptr, stride, COPY_FRAMES, n) == 0
    same("relu_bytes n %d pointer + %d" % (n, off), d.read("relu"), strided([np.maximum(x, 0) for x in xs], stride, 0xA5))


# mhip_binary_i8 with a slice output (run, pix_stride, ch_off): element i -> (i / run) * pix_stride + ch_off + i % run.  vec = all three pointers
# and strides multiples of 16 and run, pix_stride, ch_off multiples of 16 -> one 16-byte store per thread inside a pixel; else byte by byte.
BINARY = {"vec_16_48_16": (16, 48, 16), "vec_32_64_32": (32, 64, 32), "scalar_12_40_20": (12, 40, 20), "scalar_16_40_24": (16, 40, 24)}
BIN_SA = BIN_SB = 0.05
BIN_INV = 1.0 / 0.0675  # y / so = a b / 27 (mul), 20 (a + b) / 27 (add): + 0.5 is an odd number over 54, never nearer than 1 / 54 to an integer


def binary_case(cid, is_mul):
    """-> operands [frame] a, b in -40 .. 40 (nothing clamps) and the results of the plain formula trunc(y * inv + 0.5) in float32.  Asserts
    that no element comes within 1e-3 of a rounding tie: the subject is where bytes land, not how they round"""
    run = BINARY[cid][0]
    n = 6 * run
    rng = np.random.default_rng(seed_of(cid) + is_mul)
    a = [rng.integers(-40, 41, n, dtype=I8) for _ in range(COPY_FRAMES)]
    b = [rng.integers(-40, 41, n, dtype=I8) for _ in range(COPY_FRAMES)]
    F = np.float32
    want = []
    for x, y in zip(a, b):
        va, vb = x.astype(F) * F(BIN_SA), y.astype(F) * F(BIN_SB)
        t = (va * vb if is_mul else va + vb) * F(BIN_INV)
        exact = (x.astype(np.float64) * float(F(BIN_SA))) * (y.astype(np.float64) * float(F(BIN_SB))) if is_mul else \
            x.astype(np.float64) * float(F(BIN_SA)) + y.astype(np.float64) * float(F(BIN_SB))
        u = exact * float(F(BIN_INV)) + 0.5
        assert np.abs(u - np.rint(u)).min() >= 1e-3, (cid, is_mul, "an element on a rounding tie")
        r = np.trunc(t + F(0.5))
        assert r.min() >= -128 and r.max() <= 127
        want.append(r.astype(I8))
    return a, b, want


@pytest.mark.parametrize("is_mul", [0, 1], ids=["add", "mul"])
@pytest.mark.parametrize("cid", list(BINARY))
def test_binary_i8_slice_layout(hbm, cid, is_mul):
    run, ps, choff = BINARY[cid]
    n = 6 * run
    a, b, w = binary_case(cid, is_mul)
    sa_, sb_, so_ = n + 16, n + 32, align16(6 * ps) + 48
    da, db = copy_in(hbm, a, sa_, seed_of(cid)), copy_in(hbm, b, sb_, seed_of(cid) + 3)
    d = hbm(sentinel(COPY_FRAMES * so_))
    assert hbm.L.mhip_binary_i8(is_mul, da.ptr, sa_, db.ptr, sb_, d.ptr, so_, COPY_FRAMES, n, BIN_SA, BIN_SB, BIN_INV, run, ps, choff) == 0
    want = sentinel(COPY_FRAMES * so_).view(I8)
    for f in range(COPY_FRAMES):
        R.place(want[f * so_:], w[f], 6, run, ps, choff)
    same("binary_i8 %s %s" % (cid, "mul" if is_mul else "add"), d.read(cid), want)
    da.unchanged(cid)
    db.unchanged(cid)


def test_binary_i8_slice_refusals(hbm):
    a, d = hbm(np.zeros(256, U8)), hbm(sentinel(256))
    args = (a.ptr, 256, a.ptr, 256, d.ptr, 256, 1)
    assert hbm.L.mhip_binary_i8(0, *args, 40, BIN_SA, BIN_SB, BIN_INV, 16, 48, 16) == -1  # n % run != 0
    assert hbm.L.mhip_binary_i8(0, *args, 32, BIN_SA, BIN_SB, BIN_INV, 16, 31, 16) == -1  # pix_stride < ch_off + run
    same("binary_i8 refusals", d.read("refusals"), sentinel(256))
