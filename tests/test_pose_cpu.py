"""Pose keypoints without a device: the numpy restatement of include/mars_hip.h "Pose keypoints" (tests/poseref.py) on hand-worked cases,
the records' and options' layout, and the synthetic writer's pose head (its detections on the CPU oracle are the DFL twin's)."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import marsfile
import poseref
from conftest import lcg_frame
from test_gpu_yolo_dfl import decode_dfl
from test_gpu_yolo_heads import letterbox_map, nms, sig_table

F32 = np.float32
INC = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include")


def test_hand_worked_points():
    """x = ((q * s) * 2 + g) * stride"""
    # 10 * 0.25 = 2.5; * 2 = 5; + 3 = 8; * 8 = 64
    assert poseref.point(10, 3, 8, 0.25) == F32(64.0)
    # -7 * 0.5 = -3.5; * 2 = -7; + 0 = -7; * 32 = -224
    assert poseref.point(-7, 0, 32, 0.5) == F32(-224.0)
    # -128 * 0.125 = -16; * 2 = -32; + 7 = -25; * 16 = -400, and the other end: 127 * 0.125 = 15.875; 31.75 + 7 = 38.75; * 16 = 620
    assert poseref.point(-128, 7, 16, 0.125) == F32(-400.0) and poseref.point(127, 7, 16, 0.125) == F32(620.0)
    # a scale with a rounding in every step: 3 * 0.1f = 0.3f (0.30000000447 rounds up to 0.3000000119); * 2 = 0.6f; + 5 = 5.6000000238 ->
    # 5.5999999046 (= 5.6f); * 16 is exact: 89.599998474 (= 89.6f)
    assert poseref.point(3, 5, 16, 0.1) == F32(89.6)
    assert float(poseref.point(3, 5, 16, 0.1)) == 89.59999847412109
    # a byte of 0 is the cell's corner
    assert poseref.point(0, 6, 8, 0.07) == F32(48.0)


def test_hand_worked_keypoints_d3():
    """K = 2, D = 3 at cell (gx 3, gy 1), stride 8, scale 0.25: bytes (10, -4, 0) and (0, 8, 4)"""
    k = poseref.keypoints(np.array([10, -4, 0, 0, 8, 4], dtype=np.int8), 2, 3, 3, 1, 8, 0.25)
    # (2.5 * 2 + 3) * 8 = 64; (-1 * 2 + 1) * 8 = -8; sigmoid(0) = 0.5
    assert tuple(k[0]) == (F32(64.0), F32(-8.0), F32(0.5))
    # (0 + 3) * 8 = 24; (2 * 2 + 1) * 8 = 40; sigmoid(1) = 0.7310586
    assert (k[1]["x"], k[1]["y"]) == (F32(24.0), F32(40.0))
    assert k[1]["v"] == sig_table(0.25)[4 + 128] and abs(float(k[1]["v"]) - 0.7310585786) < 1e-7
    # the visibility is the class confidence's function of (byte, scale): the table the DFL restatement uses
    row = np.arange(-128, 128, dtype=np.int8)
    kk = poseref.keypoints(np.stack([row * 0, row * 0, row], axis=1).reshape(-1)[:96], 32, 3, 0, 0, 8, 0.02)
    assert np.array_equal(kk["v"], sig_table(0.02)[:32])


def test_d2_has_visibility_one():
    k = poseref.keypoints(np.array([10, -4, 0, 8], dtype=np.int8), 2, 2, 3, 1, 8, 0.25)
    assert k.tolist() == [(64.0, -8.0, 1.0), (24.0, 40.0, 1.0)]


def _frame(confs, **kw):
    """six detections from two heads (a 4 x 4 grid of stride 8 and a 2 x 2 grid of stride 16), K = 2, D = 3"""
    rng = np.random.default_rng(5)
    arrs = [rng.integers(-128, 128, (6, 4, 4), dtype=np.int8), rng.integers(-128, 128, (6, 2, 2), dtype=np.int8)]
    origins = [5, 17, 0, 19, 15, 16]  # cells 5, 0 and 15 of head 0; cells 1, 3 and 0 of head 1
    return arrs, origins, poseref.pose_frame(np.array(confs, dtype=F32), origins, arrs, [0.25, 0.5], [8, 16], 2, 3, **kw)


def test_selection_and_unused_slots():
    confs = (0.9, 0.3, 0.8, 0.8, 0.2, 0.7)
    assert poseref.select(confs, 0.0, 32) == [0, 1, 2, 3, 4, 5]
    assert poseref.select(confs, 0.5, 32) == [0, 2, 3, 5]
    assert poseref.select(confs, 0.5, 3) == [0, 2, 3]
    assert poseref.select(confs, 0.8, 32) == [0, 2, 3]
    assert poseref.select(confs, 0.0, 1) == [0]
    arrs, origins, (recs, kpts) = _frame(confs, min_conf=0.5, max_per_frame=5)
    assert recs.tolist() == [(0, 0, 5), (2, 0, 0), (3, 1, 3), (5, 1, 0), (-1, -1, -1)]
    assert kpts.shape == (5, 2) and kpts[4].tolist() == [(0.0, 0.0, 0.0)] * 2 and kpts[:4]["v"].all()
    # slot 2: cell 3 of head 1 is (gx 1, gy 1) on a grid 2 wide, stride 16, scale 0.5
    row = arrs[1].reshape(6, -1)[:, 3]
    assert kpts[2].tobytes() == poseref.keypoints(row, 2, 3, 1, 1, 16, 0.5).tobytes()
    # slot 0: cell 5 of head 0 is (gx 1, gy 1) on a grid 4 wide
    assert kpts[0]["x"][0] == poseref.point(arrs[0][0, 1, 1], 1, 8, 0.25) and kpts[0]["y"][1] == poseref.point(arrs[0][4, 1, 1], 1, 8, 0.25)
    # the cut: more records pass than slots
    _, _, (recs, kpts) = _frame(confs, max_per_frame=2)
    assert recs["det"].tolist() == [0, 1] and recs["head"].tolist() == [0, 1]
    # nothing kept: every slot is the empty pattern
    recs, kpts = poseref.pose_frame(np.zeros(0, dtype=F32), [], arrs, [0.25, 0.5], [8, 16], 2, 3, max_per_frame=3)
    assert recs.tolist() == [(-1, -1, -1)] * 3 and not kpts.view(np.uint8).any()


def test_letterbox_mapping_1280_720():
    """a 64 x 64 input fed from 1280 x 720: scale 0.05, 64 x 36 pixels of picture, 14 rows of padding above; x' = x * 20, y' = (y - 14) * 20"""
    k = poseref.keypoints(np.array([10, -4, 0, 0, 8, 4], dtype=np.int8), 2, 3, 3, 1, 8, 0.25, src=(1280, 720), in_hw=(64, 64))
    plain = poseref.keypoints(np.array([10, -4, 0, 0, 8, 4], dtype=np.int8), 2, 3, 3, 1, 8, 0.25)
    assert k["x"].tolist() == [1280.0, 480.0] and k["y"].tolist() == [(-8.0 - 14.0) * 20.0, (40.0 - 14.0) * 20.0]
    assert np.array_equal(k["v"], plain["v"])
    # the same numbers the boxes get
    d = np.zeros(2, dtype=[("x", "<f4"), ("y", "<f4"), ("w", "<f4"), ("h", "<f4")])
    d["x"], d["y"] = plain["x"], plain["y"]
    m = letterbox_map(d, 1280, 720, 64, 64)
    assert np.array_equal(m["x"], k["x"]) and np.array_equal(m["y"], k["y"])


def test_record_and_options_layout(marsrt, tmp_path):
    assert marsrt.POSE_DTYPE == poseref.POSE_DTYPE and marsrt.KPT_DTYPE == poseref.KPT_DTYPE
    S = marsrt.PoseOpts
    got = [C.sizeof(S)] + [getattr(S, f).offset for f, _ in S._fields_]
    assert got == [48, 0, 16, 20, 24, 40, 44]
    src = tmp_path / "abi.c"
    src.write_text("""
#include <stddef.h>
#include <stdio.h>
#include "mars_hip.h"
int main(void) {
 printf("%zu %zu %zu %zu %zu %zu %zu %zu %zu %d %d %d\\n", sizeof(mars_pose_t), sizeof(mars_kpt_t), sizeof(mars_hip_pose_opts_t),
        offsetof(mars_hip_pose_opts_t, kpt_tensors), offsetof(mars_hip_pose_opts_t, num_kpt), offsetof(mars_hip_pose_opts_t, kpt_dim),
        offsetof(mars_hip_pose_opts_t, kpt_scales), offsetof(mars_hip_pose_opts_t, min_conf), offsetof(mars_hip_pose_opts_t, max_per_frame),
        MARS_POSE_MAX_PER_FRAME, MARS_POSE_MAX_KPT, MARS_SYNTH_HEAD_POSE);
 return 0;
}
""")
    exe = tmp_path / "abi"
    subprocess.check_call(["gcc", "-std=c11", "-Wall", "-Werror", "-I", INC, str(src), "-o", str(exe)])
    assert [int(v) for v in subprocess.check_output([str(exe)]).split()] == [12, 12] + got + [256, 32, 3]
    assert (marsrt.POSE_MAX_PER_FRAME, marsrt.POSE_MAX_KPT, marsrt.SYNTH_HEADS["pose"]) == (256, 32, 3)
    o = marsrt.pose_opts([5, 6, 7], num_kpt=5, kpt_dim=2, kpt_scales=0.5, min_conf=0.3, max_per_frame=8)
    assert list(o.kpt_tensors) == [5, 6, 7, 0] and (o.num_kpt, o.kpt_dim, o.max_per_frame) == (5, 2, 8) and list(o.kpt_scales) == [0.5] * 4
    o = marsrt.pose_opts([1, 2, 3], kpt_scales=[0.5, 0.25, 0.125])
    assert (o.num_kpt, o.kpt_dim, o.max_per_frame, o.min_conf) == (17, 0, 0, 0.0) and list(o.kpt_scales) == [0.5, 0.25, 0.125, 0.0]


@pytest.mark.parametrize("nchw", [False, True])
@pytest.mark.parametrize("hw", [64, 160])
def test_synth_pose_head(marsrt, hw, nchw):
    """the DFL twin plus three keypoint branches behind it: three graph outputs, the keypoint tensors internal and found by name"""
    d = marsrt.synth_model(width_x16=4, input_hw=hw, nchw_int8=nchw, seed=1, head="pose")
    hdr, tensors, layers = marsfile.parse(d)
    kp = marsrt.pose_twin_tensors(d)
    assert len(hdr["outputs"]) == 3 and len(set(kp)) == 3 and not set(kp) & set(hdr["outputs"])

    def chw(t):
        s = tensors[t]["shape"]
        return (s[1], s[2], s[3]) if nchw else (s[3], s[1], s[2])
    heads, nc, reg_max = marsrt.find_yolo_dfl_heads(d)
    assert (nc, reg_max) == (80, 16) and [s for _, _, s in heads] == [8, 16, 32]
    for k, (b, c, s) in enumerate(heads):
        g = hw // s
        assert chw(hdr["outputs"][k]) == (144, g, g) and chw(b) == (64, g, g) and chw(c) == (80, g, g)
        assert chw(kp[k]) == (51, g, g) and tensors[kp[k]]["dtype"] == marsfile.I8
        writers = [l for l in layers if kp[k] in l["outs"]]
        readers = [l for l in layers if kp[k] in l["ins"]]
        assert len(writers) == 1 and writers[0]["type"] == marsfile.CONV2D and [l["type"] for l in readers] == [marsfile.RESHAPE]
    # the trunk and the DFL branches are the dfl twin's, weights included: the pose file only adds tensors and layers behind them
    dd = marsrt.synth_model(width_x16=4, input_hw=hw, nchw_int8=nchw, seed=1, head="dfl")
    hd, td, ld = marsfile.parse(dd)
    assert [t["shape"] for t in tensors[:len(td)]] == [t["shape"] for t in td] and hdr["outputs"] == hd["outputs"]
    assert [(l["type"], l["ins"], l["outs"]) for l in layers[:len(ld)]] == [(l["type"], l["ins"], l["outs"]) for l in ld]
    for bad in (dict(float32=True), dict(tiny=True)):
        with pytest.raises(ValueError):
            marsrt.synth_model(width_x16=4, input_hw=64, head="pose", **bad)
    with pytest.raises(KeyError):
        marsrt.pose_twin_tensors(dd)
    assert marsrt.describe_plan(d)  # the loader and the planner take it


def test_pose_twin_detections_equal_the_dfl_twin(marsrt, orc):
    """on the CPU oracle: the three outputs of the pose twin are the DFL twin's bytes, so are the kept detections; the keypoint tensors hold
    51 channels of varied bytes on the heads' grids"""
    hw, conf = 160, 0.1
    files = {h: marsrt.synth_model(width_x16=4, input_hw=hw, seed=1, head=h) for h in ("dfl", "pose")}
    kept = {}
    for h, d in files.items():
        hdr, tensors, _ = marsfile.parse(d)
        g = orc.Graph(d)
        g.set_input(0, lcg_frame(0x5EED0000, marsfile.tensor_nbytes(tensors[hdr["inputs"][0]])).tobytes())
        assert g.run() == 0
        hs = []
        for b, c, s in marsrt.find_yolo_dfl_heads(d)[0]:
            n = hw // s
            hs.append((np.ascontiguousarray(g.tensor(b).view(np.int8).reshape(n, n, 64).transpose(2, 0, 1)),
                       np.ascontiguousarray(g.tensor(c).view(np.int8).reshape(n, n, 80).transpose(2, 0, 1)), tensors[b]["scale"], tensors[c]["scale"], s))
        cand, _ = decode_dfl(hs, marsrt.DET_DTYPE, conf)
        kept[h] = (nms(cand, 0.45), [g.tensor(t).tobytes() for t in hdr["outputs"]])
        if h == "pose":
            for t, (_, _, s) in zip(marsrt.pose_twin_tensors(d), marsrt.find_yolo_dfl_heads(d)[0]):
                a = g.tensor(t).view(np.int8)
                assert a.size == 51 * (hw // s) ** 2 and len(np.unique(a)) > 8
    assert kept["pose"][1] == kept["dfl"][1]
    assert len(kept["dfl"][0]) > 0 and kept["pose"][0].tobytes() == kept["dfl"][0].tobytes()
