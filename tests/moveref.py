"""numpy restatement of the byte-moving layers (csrc/hip/move.hip): the reference's three loops -- MAXPOOL, CONCAT, UPSAMPLE of
mars_runtime.c -- over FLAT BYTES, with shape[1..3] read as H, W, C whatever a tensor's tag; the two layouts of an NCHW-tagged tensor on the
device; the relayout, the row un-padder and the slice form of an output.  Written to be read, not to be fast: the shapes of the tests are tiny.
tests/test_move_cpu.py pins this file against the CPU oracle (and the compiled reference where it is there), tests/test_gpu_move.py compares
the launchers of csrc/mhip.h against it byte for byte.  Also here: the input frames both of those files use."""
import numpy as np

I8, U8 = np.int8, np.uint8


def _i8(x):
    return np.ascontiguousarray(x).reshape(-1).view(I8)


# ---- the reference's loops ----------------------------------------------------------------------------------------------------------------
def maxpool(x, in_h, in_w, ch, out_h, out_w, kh, kw, sh, sw):
    """window anchored top-left at (oy sh, ox sw), clipped at the bottom and right edge, no padding, identity -128, int8 compare
    -> int8 [out_h * out_w * ch]"""
    x = _i8(x)[:in_h * in_w * ch].reshape(in_h, in_w, ch)
    out = np.full((out_h, out_w, ch), -128, dtype=I8)
    for oy in range(out_h):
        for ox in range(out_w):
            for ky in range(kh):
                iy = oy * sh + ky
                if iy >= in_h:
                    break
                for kx in range(kw):
                    ix = ox * sw + kx
                    if ix >= in_w:
                        break
                    out[oy, ox] = np.maximum(out[oy, ox], x[iy, ix])
    return out.reshape(-1)


def concat_slice(out, x, out_h, out_w, in_c, out_c, ch_off):
    """one input of a CONCAT, in place: runs of in_c bytes, pixel after pixel of the OUTPUT's extent, to ch_off of out_c-byte pixels.  Bytes
    read behind the input's end are 0 (a tensor's zeroed slack); `out` is long enough for every run"""
    x = _i8(x)
    for pix in range(out_h * out_w):
        run = np.zeros(in_c, dtype=I8)
        have = x[pix * in_c:(pix + 1) * in_c]
        run[:len(have)] = have
        out[pix * out_c + ch_off:pix * out_c + ch_off + in_c] = run


def concat(ins, in_cs, out_h, out_w, out_c):
    """the whole layer: input after input at ch_off = the sum of the in_c before it, later inputs over earlier ones where runs overlap
    (sum(in_cs) > out_c: NCHW-tagged tensors) -> int8 [out_h * out_w * out_c], the output tensor's own bytes"""
    n = out_h * out_w * out_c
    out = np.zeros(n + sum(in_cs), dtype=I8)
    off = 0
    for x, in_c in zip(ins, in_cs):
        concat_slice(out, x, out_h, out_w, in_c, out_c, off)
        off += in_c
    return out[:n].copy()


def upsample(x, in_h, in_w, ch, out_h, out_w, scale_h, scale_w, out_bytes=None):
    """nearest: source row min(oy / scale_h, in_h - 1), column min(ox / scale_w, in_w - 1); runs of ch bytes.  out_bytes: the size of the
    output tensor where it is larger than out_h * out_w * ch (NCHW-tagged: the rest is never written and stays 0)"""
    x = _i8(x)[:in_h * in_w * ch].reshape(in_h, in_w, ch)
    n = out_h * out_w * ch
    out = np.zeros(n if out_bytes is None else out_bytes, dtype=I8)
    assert len(out) >= n
    for oy in range(out_h):
        iy = min(oy // scale_h, in_h - 1)
        for ox in range(out_w):
            ix = min(ox // scale_w, in_w - 1)
            out[(oy * out_w + ox) * ch:(oy * out_w + ox + 1) * ch] = x[iy, ix]
    return out


# ---- NCHW-tagged tensors held pixels x channels -------------------------------------------------------------------------------------------
def to_pxc(flat, C, H, W):
    """the bytes of a [1, C, H, W] tensor -> [H * W][C]: what the *_nchwq kernels take and produce"""
    return np.ascontiguousarray(_i8(flat)[:C * H * W].reshape(C, H * W).T).reshape(-1)


def from_pxc(pxc, C, H, W):
    return np.ascontiguousarray(_i8(pxc)[:C * H * W].reshape(H * W, C).T).reshape(-1)


def maxpool_q(x, C, H, W, kh, kw):
    """stride-1 MAXPOOL [1, C, H, W] -> [1, C, H, W] as the reference runs it: rows are channels, columns map rows, runs of W bytes"""
    return maxpool(x, C, H, W, C, H, kh, kw, 1, 1)


def concat_q(ins, in_cs, H, W):
    """CONCAT of [1, C_k, H, W] tensors: out[f + k W] = in_k[f]"""
    return concat(ins, [W] * len(ins), sum(in_cs), H, W)


def upsample_q(x, ci, hi, wi, co, ho, wo, sh, sw):
    """UPSAMPLE [1, ci, hi, wi] -> [1, co, ho, wo]: co x ho runs of wi bytes; the tensor's bytes behind them stay 0"""
    return upsample(x, ci, hi, wi, co, ho, sh, sw, out_bytes=co * ho * wo)


# ---- relayout, rows, slices ---------------------------------------------------------------------------------------------------------------
def nchw_to_nhwc_pad(x, c, hw, c_pad):
    """[c][hw] -> [hw][c_pad], channels c .. c_pad - 1 zero"""
    out = np.zeros((hw, c_pad), dtype=I8)
    out[:, :c] = _i8(x)[:c * hw].reshape(c, hw).T
    return out.reshape(-1)


def unpad_rows(src, rows, width, pitch):
    """dst[r * width + k] = src[r * pitch + k], k < width"""
    return np.ascontiguousarray(_i8(src)[:rows * pitch].reshape(rows, pitch)[:, :width]).reshape(-1)


def place(dst, dense, npix, ch, pix_stride, ch_off):
    """slice output, in place: dense [npix][ch] lands at pix * pix_stride + ch_off + c of `dst`; every other byte keeps what it held"""
    dense = _i8(dense)
    for pix in range(npix):
        dst[pix * pix_stride + ch_off:pix * pix_stride + ch_off + ch] = dense[pix * ch:(pix + 1) * ch]


# ---- input frames -------------------------------------------------------------------------------------------------------------------------
SIGNS = np.array([0x80, 0x7F, 0xFF, 0x00, 0x01], dtype=U8).view(I8)


def random_bytes(seed, n):
    return np.random.default_rng(seed).integers(-128, 128, n, dtype=I8)


def pool_frame(kind, seed, in_h, in_w, ch):
    """kind % 3 == 0: uniform random bytes.  1: "peaks" -- all -128 but a dozen isolated bytes in -100 .. 127, each lighting exactly the
    outputs whose windows hold it (a window one row or column off shows).  2: "signs" -- 0x80 0x7F 0xFF 0x00 0x01 cycling along the channel
    axis, one step further per pixel, so that one channel meets both signs inside a window (the packed-int16 even / odd-byte maxima)"""
    n = in_h * in_w * ch
    rng = np.random.default_rng(seed)
    if kind % 3 == 0:
        return rng.integers(-128, 128, n, dtype=I8)
    if kind % 3 == 1:
        x = np.full(n, -128, dtype=I8)
        at = rng.choice(n, size=min(12, n), replace=False)
        x[at] = rng.integers(-100, 128, len(at), dtype=I8)
        return x
    pix, c = np.divmod(np.arange(n), ch)
    return SIGNS[(pix + c) % 5]


def pool_frames(seed, frames, in_h, in_w, ch):
    """frame f is of kind f % 3, each from its own seed"""
    return [pool_frame(f, seed * 1000 + f, in_h, in_w, ch) for f in range(frames)]
