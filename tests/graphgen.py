"""Random .mars graphs for the soak scripts (tests/soak/) and the CPU tests of the planner and the checker.  Host only: nothing here
imports marsrt or touches a device.  Each generator is a function of (rng, options) and returns (file bytes, description) or None;
with the default options a seed gives the graphs the soak scripts have always drawn (the random draws are the same, in the same order).

Options (off by default, so existing seeds keep their graphs):
  interior_outputs  the graph outputs are drawn from any activation: a concat's last input, a tensor that other layers read, a
                    convolution's input (the pipelined path rebinds every graph output to a buffer of its own, nothing mapped in front)
  concat_chain      (int8_graph, NCHW-tagged graphs) a [1, 2C, H, W] concat feeds two further concats of equal H, W: once as the first
                    input and once as the last, all three with C a multiple of 16 (each qualifies for concat_q)"""
import collections

import numpy as np

import marsfile

F, NC = marsfile.F32, marsfile.NCHW


def _pick_outputs(rng, G, x, keep):
    """interior_outputs: the outputs in `keep` plus up to three activations drawn from the whole graph (four at most), preferring the
    tensors the planner treats specially -- a concat's last input, a convolution's input, a tensor with more than one reader.  Each
    kind is drawn three times in four, so that some graphs keep the passes such an output rules out"""
    readers = collections.Counter(t for l in G.layers for t in l["ins"])
    acts = [i for i, t in enumerate(G.tensors) if t["size"] == 0 and i != x]
    cat_last = [l["ins"][-1] for l in G.layers if l["type"] == marsfile.CONCAT and l["ins"][-1] != x]
    conv_in = [l["ins"][0] for l in G.layers if l["type"] == marsfile.CONV2D and l["ins"][0] != x]
    shared = [t for t in acts if readers[t] > 1]
    picked = list(keep)
    for pool in (cat_last, conv_in + shared, acts):
        pool = [t for t in dict.fromkeys(pool) if t not in picked]
        if pool and rng.integers(0, 4):
            picked.append(int(pool[int(rng.integers(0, len(pool)))]))
    return picked[:4]


def int8_graph(rng, nchw=None, interior_outputs=False, concat_chain=False):
    """int8 graphs (tests/soak/fuzz_graphs.py) -- convolutions (1x1 .. 7x7, strides 1 .. 3, fused ReLU, conv -> sigmoid -> mul chains), max-pools,
    the ReLU family, sigmoid, add / mul, concats, 2x / 3x upsampling, the detectors' C3 / SPPF motifs, with shared inputs and several readers per
    tensor.  nchw: None = NCHW-tagged one time in four (drawn), True / False = always / never.

    Tensors are kept as (id, d1, d2, d3) = their shape[1..3].  NHWC graphs: (H, W, C).  NCHW-tagged graphs: (C, H, W) -- convolutions take their
    dims by the tag, while pools / concats / upsampling index shape[1..3] as H, W, C whatever the tag says (the reference's behaviour), so there a
    pool halves "C" and "H" and a concat joins along "W" """
    G = marsfile.Graph()
    nchw = bool(rng.integers(0, 4) == 0) if nchw is None else bool(nchw)
    fmt = marsfile.NCHW if nchw else marsfile.NHWC
    h, w = int(rng.integers(6, 40)), int(rng.integers(6, 40))
    c = int(rng.choice([3, 5, 8, 16, 24, 32, 40, 64]))
    dims = (c, h, w) if nchw else (h, w, c)
    x = G.tensor([1, *dims], fmt=fmt, scale=float(rng.choice([0.02, 0.04])))
    avail = [(x, *dims)]
    desc = [("nchw" if nchw else "nhwc", dims)]

    def mkconv(t, tc, th, tw, k, s, oc, pad, silu, act):
        oh, ow = (th + s - 1) // s, (tw + s - 1) // s  # the output tensor's shape; VALID still fills it (unpadded window)
        wshape = (oc, tc, k, k) if nchw else (oc, k, k, tc)
        wt = G.tensor(list(wshape), fmt=marsfile.OIHW if nchw else marsfile.OHWI, scale=0.003 / (k * k * tc) ** 0.5 * 8,
                      data=rng.integers(-127, 128, wshape, dtype=np.int8))
        b = G.tensor([oc], dtype=marsfile.I32, fmt=marsfile.D1, scale=1.0, data=rng.integers(-3000, 3000, oc, dtype=np.int32)) \
            if rng.integers(0, 5) else marsfile.NONE
        od = (oc, oh, ow) if nchw else (oh, ow, oc)
        a = G.tensor([1, *od], fmt=fmt, scale=float(rng.choice([0.04, 0.06])))
        G.conv(t, a, wt, b, (k, k), (s, s), pad=pad, act=act)
        out = a
        if silu:
            sg = G.tensor([1, *od], fmt=fmt, scale=1.0 / 256)
            o = G.tensor([1, *od], fmt=fmt, scale=float(rng.choice([0.03, 0.05])))
            G.layer(marsfile.SIGMOID, [a], [sg])
            G.layer(marsfile.MUL, [a, sg], [o])
            out = o
        return out, od

    for _ in range(int(rng.integers(3, 11))):
        t, d1, d2, d3 = avail[int(rng.integers(0, len(avail)))]
        op = str(rng.choice(["conv", "conv", "conv", "pool", "act", "bin", "concat", "up", "c3", "sppf"]))
        if op == "conv":
            tc, th, tw = (d1, d2, d3) if nchw else (d3, d1, d2)
            if th * tw > 4000 or tc > 300:
                continue
            k = int(rng.choice([1, 3, 5, 7])) if tc > 4 else int(rng.choice([3, 6]))
            if tc >= 64 and k == 7: k = 3
            s = int(rng.choice([1, 1, 2, 3]))
            oc = int(rng.choice([7, 16, 24, 32, 64, 81, 128]))
            pad = int(rng.choice([marsfile.PAD_SAME, marsfile.PAD_SAME, marsfile.PAD_SAME, marsfile.PAD_VALID]))
            silu = bool(rng.integers(0, 2))
            out, od = mkconv(t, tc, th, tw, k, s, oc, pad, silu, 0 if silu else int(rng.integers(0, 2)))
            avail.append((out, *od)); desc.append(("conv", k, s, tc, oc, silu, pad))
        elif op == "pool":
            k = int(rng.choice([2, 3, 5])); s = int(rng.choice([1, 2]))
            od = ((d1 + s - 1) // s, (d2 + s - 1) // s, d3)
            o = G.tensor([1, *od], fmt=fmt, scale=G.tensors[t]["scale"])
            G.pool(t, o, (k, k), (s, s))
            avail.append((o, *od)); desc.append(("pool", k, s))
        elif op == "act":
            kind = int(rng.choice([marsfile.RELU, marsfile.RELU6, marsfile.LEAKY, marsfile.SIGMOID]))
            o = G.tensor([1, d1, d2, d3], fmt=fmt, scale=float(rng.choice([0.01, 0.03])))
            G.layer(kind, [t], [o])
            avail.append((o, d1, d2, d3)); desc.append(("act", kind))
        elif op == "bin":
            same = [q for q in avail if q[1:] == (d1, d2, d3) and q[0] != t]
            if not same:
                continue
            u = same[int(rng.integers(0, len(same)))][0]
            o = G.tensor([1, d1, d2, d3], fmt=fmt, scale=float(rng.choice([0.03, 0.06])))
            G.layer(int(rng.choice([marsfile.ADD, marsfile.MUL])), [t, u], [o])
            avail.append((o, d1, d2, d3)); desc.append(("bin",))
        elif op == "concat":
            same = [q for q in avail if q[1] == d1 and q[2] == d2 and q[0] != t]
            if not same:
                continue
            extra = same[:int(rng.integers(1, 3))]
            parts = [t] + [q[0] for q in extra]
            cs = d3 + sum(q[3] for q in extra)
            o = G.tensor([1, d1, d2, cs], fmt=fmt, scale=G.tensors[t]["scale"])
            G.concat(parts, o)
            avail.append((o, d1, d2, cs)); desc.append(("concat", [d3] + [q[3] for q in extra]))
        elif op in ("c3", "sppf"):
            # the detectors' motifs, which the planner has passes for (virtual_concat / virtual_concat_q, pairs, pool chains, the byte-wise
            # layers on the internal layout): C3 = two 1x1 convolutions of one tensor (one of them through a bottleneck with a shortcut)
            # -> concat -> 1x1;  SPPF = 1x1 -> three chained 5x5 stride-1 pools -> concat of the four -> 1x1
            tc, th, tw = (d1, d2, d3) if nchw else (d3, d1, d2)
            if th * tw > 2500 or tc > 200:
                continue
            oc = int(rng.choice([16, 32, 64]))
            pad = marsfile.PAD_SAME
            silu = bool(rng.integers(0, 2))
            if op == "c3":
                a, od = mkconv(t, tc, th, tw, 1, 1, oc, pad, silu, 0)
                b, _ = mkconv(t, tc, th, tw, 1, 1, oc, pad, silu, 0)
                if rng.integers(0, 2):
                    m1, _ = mkconv(a, oc, th, tw, 1, 1, oc, pad, silu, 0)
                    m2, _ = mkconv(m1, oc, th, tw, 3, 1, oc, pad, silu, 0)
                    a2 = G.tensor([1, *od], fmt=fmt, scale=float(rng.choice([0.05, 0.08])))
                    G.layer(marsfile.ADD, [a, m2], [a2])
                    a = a2
                parts = [a, b]
            else:
                a, od = mkconv(t, tc, th, tw, 1, 1, oc, pad, silu, 0)
                parts = [a]
                for _i in range(3):
                    o = G.tensor([1, *od], fmt=fmt, scale=G.tensors[parts[-1]]["scale"])
                    G.pool(parts[-1], o, (5, 5), (1, 1))
                    parts.append(o)
            # (NCHW-tagged: the exporter's form, [1, sum C, H, W] along axis 1 -- which the reference's byte-wise CONCAT turns into a shift
            #  of the last input by N - 1 map rows, reading past the inputs' ends into the arena)
            cd = (od[0] * len(parts), od[1], od[2]) if nchw else (od[0], od[1], od[2] * len(parts))
            cat = G.tensor([1, *cd], fmt=fmt, scale=G.tensors[parts[0]]["scale"])
            if nchw:
                G.concat(parts, cat, axis=1)
            else:
                G.concat(parts, cat)
            cc, ch, cw = cd if nchw else (cd[2], cd[0], cd[1])
            roc = int(rng.choice([16, 32, 48]))
            out, od2 = mkconv(cat, cc, ch, cw, 1, 1, roc, pad, silu, 0)
            avail.append((parts[0], *od)); avail.append((out, *od2)); desc.append((op, tc, oc, silu))
            if rng.integers(0, 3) == 0:  # a second reader of the same shape: the head C3s' cv1 + cv2 over a concat (one paired launch)
                out2, _ = mkconv(cat, cc, ch, cw, 1, 1, roc, pad, silu, 0)
                avail.append((out2, *od2))
        else:
            if d1 * d2 > 600:
                continue
            f = int(rng.choice([2, 2, 3]))
            o = G.tensor([1, d1 * f, d2 * f, d3], fmt=fmt, scale=G.tensors[t]["scale"])
            G.upsample(t, o, f if rng.integers(0, 2) else 0, f if rng.integers(0, 2) else 0)
            avail.append((o, d1 * f, d2 * f, d3)); desc.append(("up", f))
    if concat_chain and nchw:
        # [1, 2C, H, W] = concat(a, b) of two 1x1 convolutions of one tensor; then concat(cat, u) and concat(v, cat) of equal H, W, each read by a
        # 1x1 convolution (NCHW-tagged, along axis 1: every input a multiple of 16 planes, so each of the three can stay pixels x channels)
        cand = [q for q in avail if q[1] <= 200 and q[2] * q[3] <= 1600]
        if cand:
            t, tc, th, tw = cand[int(rng.integers(0, len(cand)))]
            cc = int(rng.choice([16, 32]))
            silu = bool(rng.integers(0, 2))
            pad = marsfile.PAD_SAME
            a, od = mkconv(t, tc, th, tw, 1, 1, cc, pad, silu, 0)
            b, _ = mkconv(t, tc, th, tw, int(rng.choice([1, 3])), 1, cc, pad, silu, 0)
            cat = G.tensor([1, 2 * cc, th, tw], fmt=fmt, scale=G.tensors[a]["scale"])
            G.concat([a, b], cat, axis=1)
            for first in (True, False):
                uc = int(rng.choice([16, 32]))
                u, _ = mkconv(t, tc, th, tw, 1, 1, uc, pad, silu, 0)
                cat2 = G.tensor([1, 2 * cc + uc, th, tw], fmt=fmt, scale=G.tensors[cat]["scale"])
                G.concat([cat, u] if first else [u, cat], cat2, axis=1)
                r, od2 = mkconv(cat2, 2 * cc + uc, th, tw, 1, 1, int(rng.choice([16, 32])), pad, silu, 0)
                avail.append((r, *od2))
            desc.append(("concat_chain", tc, cc, th, tw))
    outs = [q[0] for q in avail[1:]][-3:]
    if not outs:
        return None
    if interior_outputs:
        outs = _pick_outputs(rng, G, x, outs[-1:])
    return G.serialise([x], outs), desc


def f32_graph(rng, interior_outputs=False):
    """float32 NCHW graphs (tests/soak/fuzz_graphs_f32.py) -- convolutions (1x1 / 3x3 / 5x5, stride 1 / 2, fused ReLU byte clamp, conv -> sigmoid ->
    mul chains), byte-wise max-pools, LeakyReLU / ReLU, sigmoid, add / mul, batchnorm"""
    G = marsfile.Graph()
    c, h, w = int(rng.choice([3, 8, 16, 32])), int(rng.integers(6, 30)), int(rng.integers(6, 30))
    x = G.tensor([1, c, h, w], dtype=F, fmt=NC)
    avail = [(x, c, h, w)]
    desc = []
    for _ in range(int(rng.integers(3, 9))):
        t, tc, th, tw = avail[int(rng.integers(0, len(avail)))]
        op = str(rng.choice(["conv", "conv", "conv", "pool", "act", "bin", "bn"]))
        if op == "conv":
            k = int(rng.choice([1, 3, 5])); s = int(rng.choice([1, 1, 2])); oc = int(rng.choice([8, 16, 24, 64, 100]))
            oh, ow = (th + s - 1) // s, (tw + s - 1) // s
            a0 = 1.7 / (k * k * tc) ** 0.5
            wt = G.tensor([oc, tc, k, k], dtype=F, fmt=marsfile.OIHW, data=((rng.random((oc, tc, k, k)) * 2 - 1) * a0).astype(np.float32))
            b = G.tensor([oc], dtype=F, fmt=marsfile.D1, data=((rng.random(oc) * 2 - 1) * 0.1).astype(np.float32))
            a = G.tensor([1, oc, oh, ow], dtype=F, fmt=NC)
            silu = bool(rng.integers(0, 2))
            G.conv(t, a, wt, b, (k, k), (s, s), act=0 if silu else int(rng.integers(0, 2)))
            out = a
            if silu:
                sg = G.tensor([1, oc, oh, ow], dtype=F, fmt=NC); o = G.tensor([1, oc, oh, ow], dtype=F, fmt=NC)
                G.layer(marsfile.SIGMOID, [a], [sg]); G.layer(marsfile.MUL, [a, sg], [o])
                out = o
            avail.append((out, oc, oh, ow)); desc.append(("conv", k, s, tc, oc, silu))
        elif op == "pool":  # indexes shape[1..3] as H, W, C over BYTES: stride 1 keeps the shape
            k = int(rng.choice([2, 3, 5]))
            o = G.tensor([1, tc, th, tw], dtype=F, fmt=NC)
            G.pool(t, o, (k, k), (1, 1))
            avail.append((o, tc, th, tw)); desc.append(("pool", k))
        elif op == "act":
            kind = int(rng.choice([marsfile.RELU, marsfile.LEAKY, marsfile.SIGMOID]))
            o = G.tensor([1, tc, th, tw], dtype=F, fmt=NC)
            G.layer(kind, [t], [o])
            avail.append((o, tc, th, tw)); desc.append(("act", kind))
        elif op == "bin":
            same = [q for q in avail if q[1:] == (tc, th, tw) and q[0] != t]
            if not same:
                continue
            o = G.tensor([1, tc, th, tw], dtype=F, fmt=NC)
            G.layer(int(rng.choice([marsfile.ADD, marsfile.MUL])), [t, same[int(rng.integers(0, len(same)))][0]], [o])
            avail.append((o, tc, th, tw)); desc.append(("bin",))
        else:
            sc = G.tensor([tc], dtype=F, fmt=marsfile.D1, data=(rng.random(tc) + 0.5).astype(np.float32))
            bi = G.tensor([tc], dtype=F, fmt=marsfile.D1, data=(rng.random(tc) - 0.5).astype(np.float32))
            o = G.tensor([1, tc, th, tw], dtype=F, fmt=NC)
            G.layer(marsfile.BATCHNORM, [t, sc, bi], [o])
            avail.append((o, tc, th, tw)); desc.append(("bn",))
    outs = [q[0] for q in avail[1:]][-3:]
    if not outs:
        return None
    if interior_outputs:
        outs = _pick_outputs(rng, G, x, outs[-1:])
    return G.serialise([x], outs), desc


def vcat_f32_graph(rng, interior_outputs=False):
    """float32 NCHW graphs around the reference's byte-wise CONCAT of equal maps (tests/soak/fuzz_vcat_f32.py) -- 2 to 4 branches (1x1 / 3x3
    convolutions, chained byte-wise max-pools as in SPPF, the graph input itself) -> CONCAT in the exporter's form [1, sum C, H, W] -> one 1x1
    convolution or two of the same shape (a C3's cv1 + cv2: one paired launch) -> sometimes a k x k convolution behind (record-format pairs).
    Map widths that are multiples of 4 let virtual_concat_f32 read the concat's last input through a view."""
    G = marsfile.Graph()
    h = int(rng.integers(4, 26))
    w = int(rng.choice([4, 8, 12, 16, 20, 24, 40, 6, 10]))  # (6, 10: the concat's runs are not whole floats -- it stays materialised)
    c_in = int(rng.choice([8, 16, 32]))
    x = G.tensor([1, c_in, h, w], dtype=F, fmt=NC)

    def conv(t, tc, th, tw, k, s, oc, silu):
        oh, ow = (th + s - 1) // s, (tw + s - 1) // s
        a0 = 1.7 / (k * k * tc) ** 0.5
        wt = G.tensor([oc, tc, k, k], dtype=F, fmt=marsfile.OIHW, data=((rng.random((oc, tc, k, k)) * 2 - 1) * a0).astype(np.float32))
        b = G.tensor([oc], dtype=F, fmt=marsfile.D1, data=((rng.random(oc) * 2 - 1) * 0.1).astype(np.float32)) if rng.integers(0, 4) else marsfile.NONE
        a = G.tensor([1, oc, oh, ow], dtype=F, fmt=NC)
        G.conv(t, a, wt, b, (k, k), (s, s), act=0)
        if not silu:
            return a, oh, ow
        sg = G.tensor([1, oc, oh, ow], dtype=F, fmt=NC); o = G.tensor([1, oc, oh, ow], dtype=F, fmt=NC)
        G.layer(marsfile.SIGMOID, [a], [sg]); G.layer(marsfile.MUL, [a, sg], [o])
        return o, oh, ow

    nb = int(rng.integers(2, 5))
    oc = int(rng.choice([8, 16, 32, 64]))
    silu = bool(rng.integers(0, 2))
    kind = str(rng.choice(["convs", "convs", "sppf", "with_input"]))
    parts = []
    if kind == "sppf":
        a, _, _ = conv(x, c_in, h, w, 1, 1, oc, silu)
        parts = [a]
        for _ in range(nb - 1):
            o = G.tensor([1, oc, h, w], dtype=F, fmt=NC)
            G.pool(parts[-1], o, (5, 5), (1, 1))
            parts.append(o)
    else:
        for q in range(nb):
            if kind == "with_input" and q == 0 and c_in == oc:
                parts.append(x)
                continue
            a, _, _ = conv(x, c_in, h, w, int(rng.choice([1, 1, 3])), 1, oc, silu)
            parts.append(a)
        rng.shuffle(parts)
    cat = G.tensor([1, oc * nb, h, w], dtype=F, fmt=NC)
    G.concat([int(p) for p in parts], cat, axis=1)
    outs = []
    roc = int(rng.choice([8, 16, 40, 64, 128, 7, 255]))  # (7, 255: channel counts that are not multiples of the head kernel's 4-channel lanes)
    readers = 2 if rng.integers(0, 3) == 0 else 1
    for _ in range(readers):
        r, _, _ = conv(cat, oc * nb, h, w, 1, 1, roc, silu)
        outs.append(r)
    if rng.integers(0, 3) == 0 and roc % 8 == 0:  # a k x k convolution behind the reader: a record-format pair where the shapes allow
        r2, _, _ = conv(outs[0], roc, h, w, 3, int(rng.choice([1, 2])), int(rng.choice([16, 32])), silu)
        outs = [r2] + outs[1:]
    outs = outs[:4]
    if interior_outputs:
        outs = _pick_outputs(rng, G, x, outs)
    return G.serialise([x], outs), (kind, nb, oc, roc, readers, h, w, c_in, silu)
