#!/usr/bin/env python3
"""The letterbox front-end alone at the camera leg's geometry (256 frames of 1280 x 720 RGB -> 640 x 640 int8), for a kernel trace:
  rocprofv3 --kernel-trace --stats --output-format csv -d gpurun_out/lb -o lb -- python3 tools/letterbox_time.py [form]
form: 0 strips (default), 1 16 x 16 tiles, 2 one thread per pixel (MARS_HIP_LETTERBOX_FORM).
A further argument "nv12": after the RGB launches, as many with the same number of NV12 frames (letterbox_strip_kernel<.., 1> beside <.., 0> in the trace; under
form 1 / 2: nv12_to_rgb_kernel + the RGB kernel)."""
import importlib.util
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
args = [a for a in sys.argv[1:] if a != "nv12"]
if args:
    os.environ["MARS_HIP_LETTERBOX_FORM"] = args[0]
spec = importlib.util.spec_from_file_location("marsrt", os.path.join(ROOT, "thingino-accel_amd", "marsrt.py"))
M = importlib.util.module_from_spec(spec)
spec.loader.exec_module(M)
M.nna_init()
B, w, h = 256, 1280, 720
d = M.synth_model(width_x16=4, input_hw=640, seed=1)
m = M.Model(d, batch=B)
rng = np.random.default_rng(1)
frames = rng.integers(0, 256, (B, h, w, 3), dtype=np.uint8)
for _ in range(6):
    m.preprocess(frames)
if "nv12" in sys.argv[1:]:
    nv12 = rng.integers(0, 256, (B, w * h * 3 // 2), dtype=np.uint8)
    for _ in range(6):
        m.preprocess_nv12(nv12, w, h)
M.lib().mars_hip_sync()
m.close()
print("done")
