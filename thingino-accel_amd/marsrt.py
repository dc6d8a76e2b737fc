"""ctypes view of libnna_mars.so -- the C-ABI the reference's callers bind.

Host-side mirror of the reference's C interface for this path (same function
names, argument meaning and error codes: include/nna.h, nna_memory.h,
nna_tensor.h, mars_runtime.h, mxu_ops.h) plus the additive mars_hip_* calls of
include/mars_hip.h.  There is no compute in this file and no fallback: if the
shared library or the GPU is missing, calls fail.

The package directory is called ``thingino-accel_amd`` (not importable by name);
load this module by path::

    import importlib.util, os
    spec = importlib.util.spec_from_file_location("marsrt", ".../thingino-accel_amd/marsrt.py")
"""
import ctypes as C
import os

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(_HERE, "lib", "libnna_mars.so")

MARS_OK = 0
MARS_ERR_INVALID_MAGIC = -1
MARS_ERR_VERSION_MISMATCH = -2
MARS_ERR_ALLOC_FAILED = -3
MARS_ERR_INVALID_FILE = -4
MARS_ERR_NNA_INIT_FAILED = -5
MARS_ERR_LAYER_FAILED = -6
MARS_ERR_INVALID_TENSOR = -7
MARS_ERR_INVALID_LAYER = -8
NNA_SUCCESS = 0

DET_DTYPE = np.dtype([("x", "<f4"), ("y", "<f4"), ("w", "<f4"), ("h", "<f4"),
                      ("conf", "<f4"), ("cls", "<i4")])
MAX_DET = 1000


# ---- struct mirrors (include/mars.h, include/mars_runtime.h) -----------------
class MarsHeader(C.Structure):
    _pack_ = 1
    _fields_ = [("magic", C.c_uint32), ("version_major", C.c_uint16), ("version_minor", C.c_uint16),
                ("flags", C.c_uint32), ("num_layers", C.c_uint32), ("num_tensors", C.c_uint32),
                ("num_inputs", C.c_uint32), ("num_outputs", C.c_uint32), ("weights_offset", C.c_uint64),
                ("weights_size", C.c_uint64), ("input_tensor_ids", C.c_uint32 * 4),
                ("output_tensor_ids", C.c_uint32 * 4)]


class MarsTensorDesc(C.Structure):
    _pack_ = 1
    _fields_ = [("id", C.c_uint32), ("name", C.c_char * 60), ("dtype", C.c_uint32), ("format", C.c_uint32),
                ("ndims", C.c_uint32), ("shape", C.c_int32 * 6), ("data_offset", C.c_uint64),
                ("data_size", C.c_uint64), ("scale", C.c_float), ("zero_point", C.c_int32)]


class MarsRuntimeTensor(C.Structure):
    _fields_ = [("desc", MarsTensorDesc), ("vaddr", C.c_void_p), ("paddr", C.c_void_p),
                ("alloc_size", C.c_size_t), ("is_external", C.c_bool)]


class MarsRuntimeLayer(C.Structure):
    _fields_ = [("desc", C.c_uint8 * 112), ("is_executed", C.c_bool)]


class MarsModel(C.Structure):
    _fields_ = [("header", MarsHeader), ("tensors", C.POINTER(MarsRuntimeTensor)),
                ("layers", C.POINTER(MarsRuntimeLayer)), ("ddr_base", C.c_void_p), ("ddr_paddr", C.c_void_p),
                ("ddr_size", C.c_size_t), ("oram_base", C.c_void_p), ("oram_paddr", C.c_void_p),
                ("oram_size", C.c_size_t), ("weights", C.c_void_p), ("weights_size", C.c_size_t),
                ("total_inference_us", C.c_uint64), ("inference_count", C.c_uint32)]


class HwInfo(C.Structure):
    _fields_ = [("oram_vbase", C.c_uint32), ("oram_pbase", C.c_uint32), ("oram_size", C.c_uint32),
                ("version", C.c_uint32)]


class SynthOpts(C.Structure):
    _fields_ = [("width_x16", C.c_int), ("depth_x3", C.c_int), ("input_hw", C.c_int), ("float32", C.c_int),
                ("nchw_int8", C.c_int), ("seed", C.c_uint), ("tiny", C.c_int), ("vary_scales", C.c_int)]


class YoloHeads(C.Structure):  # mars_yolo_heads_t: zero = default in every field
    _fields_ = [("n_heads", C.c_int), ("head_tensors", C.c_int * 4), ("strides", C.c_int * 4), ("anchors", C.c_float * 24),
                ("conf_thresh", C.c_float), ("nms_thresh", C.c_float), ("src_w", C.c_int), ("src_h", C.c_int)]


class YoloDflHeads(C.Structure):  # mars_yolo_dfl_heads_t: zero = default in every field
    _fields_ = [("n_heads", C.c_int), ("box_tensors", C.c_int * 4), ("cls_tensors", C.c_int * 4), ("strides", C.c_int * 4),
                ("reg_max", C.c_int), ("box_scales", C.c_float * 4), ("cls_scales", C.c_float * 4), ("conf_thresh", C.c_float),
                ("nms_thresh", C.c_float), ("src_w", C.c_int), ("src_h", C.c_int)]


class PipeOpts(C.Structure):
    _fields_ = [("download_outputs", C.c_int), ("detect", C.c_int), ("det_outputs", C.c_int * 4), ("n_det_outputs", C.c_int),
                ("nms_thresh", C.c_float), ("camera_w", C.c_int), ("camera_h", C.c_int), ("heads", C.POINTER(YoloHeads)),
                ("dfl_heads", C.POINTER(YoloDflHeads)), ("camera_format", C.c_int), ("camera_flags", C.c_uint)]


CAMERA_RGB, CAMERA_NV12 = 0, 1        # MARS_HIP_CAMERA_*
NV12_FULL_RANGE, NV12_VU = 1, 2       # MARS_NV12_*
ROI_KEEP_ASPECT, ROI_AREA = 1, 4      # MARS_ROI_*
ROI_DTYPE = np.dtype([("frame", "<i4"), ("det", "<i4"), ("x0", "<i4"), ("y0", "<i4"), ("x1", "<i4"), ("y1", "<i4")])  # mars_roi_t


class RoiOpts(C.Structure):  # mars_hip_roi_opts_t: zero = default in every field but the frame size
    _fields_ = [("src_w", C.c_int), ("src_h", C.c_int), ("src_format", C.c_int), ("src_flags", C.c_uint), ("expand", C.c_float),
                ("min_conf", C.c_float), ("min_size", C.c_int), ("cls_first", C.c_int), ("cls_count", C.c_int), ("max_per_frame", C.c_int),
                ("flags", C.c_uint)]


CLS_MAX_TOPK, CLS_SOFTMAX = 8, 1       # MARS_CLS_*
CLS_DTYPE = np.dtype([("cls", "<i4"), ("score", "<f4")])  # mars_cls_t


class ClsOpts(C.Structure):  # mars_hip_cls_opts_t: zero = default in every field
    _fields_ = [("output_index", C.c_int), ("tensor", C.c_int), ("top_k", C.c_int), ("scale", C.c_float), ("flags", C.c_uint)]


class MatchOpts(C.Structure):  # mars_hip_match_opts_t: zero = default in every field
    _fields_ = [("top_k", C.c_int), ("min_score", C.c_float), ("flags", C.c_uint)]


TRACK_SLOTS, TRACK_MAX_CAND = 256, 256                                   # MARS_TRACK_*
TRACK_ANY_CLASS, TRACK_CARRY_IDENTITY, TRACK_STREAM_MAJOR = 1, 2, 4
TRACK_DTYPE = np.dtype([("id", "<i4"), ("hits", "<i4")])                 # mars_track_t
TRACK_STATE_DTYPE = np.dtype([("id", "<i4"), ("cls", "<i4"), ("hits", "<i4"), ("miss", "<i4"), ("x", "<f4"), ("y", "<f4"), ("w", "<f4"),
                              ("h", "<f4"), ("vx", "<f4"), ("vy", "<f4"), ("ident", CLS_DTYPE)])  # mars_track_state_t


class TrackRec(C.Structure):  # mars_track_t
    _fields_ = [("id", C.c_int), ("hits", C.c_int)]


class ClsRec(C.Structure):  # mars_cls_t
    _fields_ = [("cls", C.c_int), ("score", C.c_float)]


class TrackState(C.Structure):  # mars_track_state_t
    _fields_ = [("id", C.c_int), ("cls", C.c_int), ("hits", C.c_int), ("miss", C.c_int), ("x", C.c_float), ("y", C.c_float), ("w", C.c_float),
                ("h", C.c_float), ("vx", C.c_float), ("vy", C.c_float), ("ident", ClsRec)]


class TrackOpts(C.Structure):  # mars_hip_track_opts_t: zero = default in every field
    _fields_ = [("min_conf", C.c_float), ("low_conf", C.c_float), ("iou_thresh", C.c_float), ("iou_thresh_low", C.c_float),
                ("max_miss", C.c_int), ("cls_first", C.c_int), ("cls_count", C.c_int), ("flags", C.c_uint)]


TRACK_APP_SMOOTH = 1                                                     # MARS_TRACK_APP_*
TRACK_APP_MAX_C = 4096


class TrackAppOpts(C.Structure):  # mars_hip_track_app_opts_t: zero = default in every field
    _fields_ = [("app_thresh", C.c_float), ("app_min_iou", C.c_float), ("flags", C.c_uint)]


SEG_MAX_PER_FRAME, SEG_MAX_NM = 64, 64                                  # MARS_SEG_*
MASK_DTYPE = np.dtype([("det", "<i4"), ("x0", "<i4"), ("y0", "<i4"), ("x1", "<i4"), ("y1", "<i4"), ("area", "<i4")])  # mars_mask_t


class MaskRec(C.Structure):  # mars_mask_t
    _fields_ = [("det", C.c_int), ("x0", C.c_int), ("y0", C.c_int), ("x1", C.c_int), ("y1", C.c_int), ("area", C.c_int)]


class SegOpts(C.Structure):  # mars_hip_seg_opts_t: zero = default in every field but the tensor indices
    _fields_ = [("coef_tensors", C.c_int * 4), ("proto_tensor", C.c_int), ("coef_scales", C.c_float * 4), ("proto_scale", C.c_float),
                ("logit_min", C.c_float), ("min_conf", C.c_float), ("max_per_frame", C.c_int)]


MASK_NATIVE_MAX = 8192                                                  # MARS_MASK_NATIVE_MAX
MASK_GEOM_FIELDS = ("in_w", "in_h", "nw", "nh", "px", "py", "base_w", "base_h", "out_w", "out_h")


class MaskNativeOpts(C.Structure):  # mars_hip_mask_native_opts_t: zero = default in every field
    _fields_ = [("out_w", C.c_int), ("out_h", C.c_int), ("flags", C.c_uint)]


class MaskGeom(C.Structure):  # mars_mask_geom_t
    _fields_ = [(n, C.c_int) for n in MASK_GEOM_FIELDS]


POSE_MAX_PER_FRAME, POSE_MAX_KPT = 256, 32                              # MARS_POSE_*
POSE_DTYPE = np.dtype([("det", "<i4"), ("head", "<i4"), ("cell", "<i4")])  # mars_pose_t
KPT_DTYPE = np.dtype([("x", "<f4"), ("y", "<f4"), ("v", "<f4")])          # mars_kpt_t


class PoseOpts(C.Structure):  # mars_hip_pose_opts_t: zero = default in every field but the tensor indices and num_kpt
    _fields_ = [("kpt_tensors", C.c_int * 4), ("num_kpt", C.c_int), ("kpt_dim", C.c_int), ("kpt_scales", C.c_float * 4),
                ("min_conf", C.c_float), ("max_per_frame", C.c_int)]


ALIGN_DTYPE = np.dtype([("X0", "<i4"), ("Y0", "<i4"), ("Ux", "<i4"), ("Uy", "<i4"), ("Vx", "<i4"), ("Vy", "<i4"), ("used", "<u4"),
                        ("n_used", "<i4")])                              # mars_align_t


class AlignOpts(C.Structure):  # mars_hip_align_opts_t: zero = default in every field but num_kpt and the template
    _fields_ = [("num_kpt", C.c_int), ("tmpl", (C.c_float * 2) * POSE_MAX_KPT), ("use", C.c_uint), ("min_vis", C.c_float)]


OBB_AGNOSTIC = 1                                                        # MARS_OBB_AGNOSTIC
OBB_DTYPE = np.dtype([("x", "<f4"), ("y", "<f4"), ("w", "<f4"), ("h", "<f4"), ("conf", "<f4"), ("cls", "<i4"), ("angle", "<f4"),
                      ("pred", "<i4")])                                  # mars_obb_t


class ObbOpts(C.Structure):  # mars_hip_obb_opts_t: zero = default in every field but the tensor indices
    _fields_ = [("angle_tensors", C.c_int * 4), ("angle_scales", C.c_float * 4), ("flags", C.c_uint)]


TILE_MAX_TILES, TILE_MAX_CAND = 64, 2048                                 # MARS_TILE_*
TILE_KEEP_ASPECT, TILE_MATCH_IOS, TILE_AGNOSTIC, TILE_AREA = 1, 2, 4, 16
TILE_DTYPE = np.dtype([("x0", "<i4"), ("y0", "<i4"), ("x1", "<i4"), ("y1", "<i4")])  # mars_tile_t
TILE_SRC_DTYPE = np.dtype([("tile", "<i4"), ("det", "<i4")])              # mars_tile_src_t
TILE_STATS_DTYPE = np.dtype([("candidates", "<i4"), ("overflow", "<i4"), ("invalid", "<i4"), ("edge", "<i4"), ("suppressed", "<i4"),
                             ("truncated", "<i4")])                        # mars_tile_stats_t


class TileOpts(C.Structure):  # mars_hip_tile_opts_t: zero = default in every field but the frame size and the table
    _fields_ = [("src_w", C.c_int), ("src_h", C.c_int), ("src_format", C.c_int), ("src_flags", C.c_uint), ("n_tiles", C.c_int),
                ("tiles", C.c_void_p), ("flags", C.c_uint), ("merge_thresh", C.c_float), ("edge_margin", C.c_float), ("max_per_tile", C.c_int)]


REDACT_MOSAIC, REDACT_FILL = 0, 1                                        # MARS_REDACT_*
REDACT_USE_MASKS, REDACT_SPARE_IDENTIFIED = 1, 2
REDACT_MAX_DIM = 8192
REDACT_STATS_DTYPE = np.dtype([("regions", "<i4"), ("masked", "<i4"), ("skipped", "<i4"), ("pixels", "<i4")])  # mars_redact_stats_t


class RedactOpts(C.Structure):  # mars_hip_redact_opts_t: zero = default in every field but the frame size
    _fields_ = [("src_w", C.c_int), ("src_h", C.c_int), ("src_format", C.c_int), ("src_flags", C.c_uint), ("mode", C.c_int), ("cell", C.c_int),
                ("fill", C.c_ubyte * 3), ("expand", C.c_float), ("min_conf", C.c_float), ("ident_min", C.c_float), ("cls_first", C.c_int),
                ("cls_count", C.c_int), ("flags", C.c_uint)]


OVERLAY_MASKS, OVERLAY_BOXES, OVERLAY_KEYPOINTS, OVERLAY_LABELS = 1, 2, 4, 8  # MARS_OVERLAY_*
OVERLAY_BY_CLASS, OVERLAY_BY_TRACK, OVERLAY_FIXED = 0, 1, 2
OVERLAY_TEXT_CLASS, OVERLAY_TEXT_TRACK, OVERLAY_TEXT_CONF = 1, 2, 4
OVERLAY_TRACKED_ONLY = 1
OVERLAY_TEXT_MAX, OVERLAY_NAME_LEN, OVERLAY_MAX_NAMES = 24, 16, 4096
OVERLAY_STATS_DTYPE = np.dtype([("boxes", "<i4"), ("masked", "<i4"), ("labels", "<i4"), ("markers", "<i4"), ("skipped", "<i4"),
                                ("pixels", "<i4")])  # mars_overlay_stats_t


class OverlayOpts(C.Structure):  # mars_hip_overlay_opts_t: zero = default in every field but the frame size
    _fields_ = [("src_w", C.c_int), ("src_h", C.c_int), ("src_format", C.c_int), ("src_flags", C.c_uint), ("layers", C.c_uint),
                ("color_by", C.c_int), ("text", C.c_uint), ("thickness", C.c_int), ("radius", C.c_int), ("scale", C.c_int), ("alpha", C.c_int),
                ("no_key", C.c_ubyte * 3), ("min_conf", C.c_float), ("kpt_min_v", C.c_float), ("cls_first", C.c_int), ("cls_count", C.c_int),
                ("min_hits", C.c_int), ("flags", C.c_uint), ("n_palette", C.c_int), ("palette", C.c_void_p), ("n_names", C.c_int),
                ("names", C.c_void_p)]


MOTION_STREAM_MAJOR, MOTION_FRAME_DIFF = 1, 2                             # MARS_MOTION_*
MOTION_MAX_ZONES = 64
MOTION_STATS_DTYPE = np.dtype([("active", "<i4"), ("x0", "<i4"), ("y0", "<i4"), ("x1", "<i4"), ("y1", "<i4"), ("first", "<i4")])  # mars_motion_stats_t
MOTION_DET_DTYPE = np.dtype([("active", "<i4"), ("cells", "<i4")])        # mars_motion_det_t


class MotionOpts(C.Structure):  # mars_hip_motion_opts_t: zero = default in every field
    _fields_ = [("threshold", C.c_int), ("learn", C.c_int), ("learn_active", C.c_int), ("min_neighbors", C.c_int), ("flags", C.c_uint),
                ("n_zones", C.c_int), ("zones", C.c_void_p)]


EVENTS_MAX_LINES, EVENTS_MAX_ZONES, EVENTS_MAX_VERTS = 32, 32, 8          # MARS_EVENTS_*
EVENTS_STREAM_MAJOR, EVENTS_ANCHOR_BOTTOM = 1, 2
EVENT_DTYPE = np.dtype([("zones", "<u4"), ("entered", "<u4"), ("exited", "<u4"), ("dwelled", "<u4"), ("lines_in", "<u4"),
                        ("lines_out", "<u4")])                           # mars_event_t
EVENT_SLOT_DTYPE = np.dtype([("id", "<i4"), ("last_step", "<i4"), ("qx", "<i4"), ("qy", "<i4"), ("inside", "<u4"), ("dwelled", "<u4"),
                             ("since", "<i4", (EVENTS_MAX_ZONES,))])      # mars_event_slot_t


class EventLine(C.Structure):  # mars_event_line_t
    _fields_ = [("ax", C.c_int), ("ay", C.c_int), ("bx", C.c_int), ("by", C.c_int)]


class EventZone(C.Structure):  # mars_event_zone_t
    _fields_ = [("n", C.c_int), ("dwell", C.c_int), ("x", C.c_int * EVENTS_MAX_VERTS), ("y", C.c_int * EVENTS_MAX_VERTS)]


class EventRules(C.Structure):  # mars_hip_event_rules_t
    _fields_ = [("n_lines", C.c_int), ("n_zones", C.c_int), ("lines", EventLine * EVENTS_MAX_LINES), ("zones", EventZone * EVENTS_MAX_ZONES)]


class EventsOpts(C.Structure):  # mars_hip_events_opts_t: zero = default in every field
    _fields_ = [("max_gap", C.c_int), ("min_hits", C.c_int), ("flags", C.c_uint)]


SHOT_STREAM_MAJOR, SHOT_KEEP_ASPECT, SHOT_INSIDE = 1, 2, 4                # MARS_SHOT_*
SHOT_FREE, SHOT_LIVE, SHOT_DONE = 0, 1, 2
SHOT_DTYPE = np.dtype([("score", "<i8"), ("sharp", "<i4"), ("mean", "<i4"), ("slot", "<i4"), ("taken", "<i4")])  # mars_shot_t
SHOT_SLOT_DTYPE = np.dtype([("id", "<i4"), ("state", "<i4"), ("first_step", "<i4"), ("last_step", "<i4"), ("best_step", "<i4"), ("seen", "<i4"),
                            ("taken", "<i4"), ("cls", "<i4"), ("conf", "<f4"), ("x0", "<i4"), ("y0", "<i4"), ("x1", "<i4"), ("y1", "<i4"),
                            ("sharp", "<i4"), ("mean", "<i4"), ("pad", "<i4"), ("score", "<i8")])  # mars_shot_slot_t


class ShotOpts(C.Structure):  # mars_hip_shot_opts_t: zero = default in every field
    _fields_ = [("max_gap", C.c_int), ("min_hits", C.c_int), ("min_mean", C.c_int), ("max_mean", C.c_int), ("min_sharp", C.c_int),
                ("src_w", C.c_int), ("src_h", C.c_int), ("flags", C.c_uint)]


assert C.sizeof(MarsHeader) == 76 and C.sizeof(MarsTensorDesc) == 124
assert SHOT_DTYPE.itemsize == 24 and SHOT_SLOT_DTYPE.itemsize == 72 and C.sizeof(ShotOpts) == 32
assert EVENT_DTYPE.itemsize == 24 and EVENT_SLOT_DTYPE.itemsize == 152 and C.sizeof(EventRules) == 2824 and C.sizeof(EventsOpts) == 12
assert MOTION_STATS_DTYPE.itemsize == 24 and MOTION_DET_DTYPE.itemsize == 8 and C.sizeof(MotionOpts) == 32
assert REDACT_STATS_DTYPE.itemsize == 16 and C.sizeof(RedactOpts) == 52
assert OVERLAY_STATS_DTYPE.itemsize == 24 and C.sizeof(OverlayOpts) == 104
assert TILE_DTYPE.itemsize == 16 and TILE_SRC_DTYPE.itemsize == 8 and TILE_STATS_DTYPE.itemsize == 24 and C.sizeof(TileOpts) == 48
assert OBB_DTYPE.itemsize == 32 and C.sizeof(ObbOpts) == 36
assert POSE_DTYPE.itemsize == KPT_DTYPE.itemsize == 12 and C.sizeof(PoseOpts) == 48
assert ALIGN_DTYPE.itemsize == 32 and C.sizeof(AlignOpts) == 268
assert C.sizeof(MaskRec) == MASK_DTYPE.itemsize == 24 and C.sizeof(SegOpts) == 52
assert C.sizeof(MaskNativeOpts) == 12 and C.sizeof(MaskGeom) == 40
assert C.sizeof(TrackRec) == TRACK_DTYPE.itemsize == 8 and C.sizeof(TrackState) == TRACK_STATE_DTYPE.itemsize == 48


class CompileOpts(C.Structure):  # mars_compile_opts_t (include/mars_compile.h)
    _fields_ = [("float32", C.c_int), ("nhwc", C.c_int), ("verbose", C.c_int)]

# every symbol the headers under include/ declare (checked by tests/test_abi.py)
EXPORTS = {
    "nna.h": ["nna_init", "nna_deinit", "nna_get_hw_info", "nna_is_ready", "nna_get_version", "nna_lock",
              "nna_unlock"],
    "nna_memory.h": ["nna_malloc", "nna_memalign", "nna_calloc", "nna_free", "nna_oram_malloc", "nna_oram_free",
                     "nna_oram_get_stats", "nna_cache_flush", "nna_cache_invalidate"],
    "nna_tensor.h": ["nna_tensor_create", "nna_tensor_from_data", "nna_tensor_destroy", "nna_tensor_data",
                     "nna_tensor_shape", "nna_tensor_dtype", "nna_tensor_numel", "nna_tensor_bytes",
                     "nna_tensor_reshape", "nna_shape_make"],
    "nna_model.h": ["nna_model_load", "nna_model_load_from_memory", "nna_model_get_info", "nna_model_get_input",
                    "nna_model_get_input_by_name", "nna_model_get_output", "nna_model_get_output_by_name",
                    "nna_model_run", "nna_model_unload"],
    "mars_runtime.h": ["mars_load_file", "mars_load_memory", "mars_free", "mars_get_input", "mars_get_output",
                       "mars_run", "mars_get_error_string", "mars_get_num_inputs", "mars_get_num_outputs",
                       "mars_print_summary"],
    "mxu_ops.h": ["mxu_init", "mxu_is_initialized", "mxu_mul_f32", "mxu_add_f32", "mxu_sub_f32", "mxu_relu_f32",
                  "conv2d_int8_mxu", "conv2d_int8_nhwc_mxu", "conv2d_float32_mxu"],
    "mars_hip.h": ["mars_hip_set_batch", "mars_hip_get_batch", "mars_hip_upload_inputs", "mars_hip_run_device",
                   "mars_hip_run_device_async", "mars_hip_download_outputs", "mars_hip_sync",
                   "mars_hip_tensor_device", "mars_hip_tensor_row_pitch", "mars_hip_read_tensor", "mars_hip_write_tensor", "mars_hip_set_fusion",
                   "mars_hip_set_profiling", "mars_hip_num_ops", "mars_hip_op_info", "mars_hip_stream",
                   "mars_hip_load_memory_ex", "mars_hip_describe_plan", "mars_hip_param_arena", "mars_yolo_parse_output", "mars_yolo_nms",
                   "mars_hip_detect", "mars_hip_detect_device", "mars_synth_model", "mars_hip_set_tuning", "mars_hip_autotune", "mars_yolo_letterbox",
                   "mars_hip_preprocess", "mars_hip_preprocess_device", "mars_hip_tensor_frame_bytes", "mars_hip_tensor_byte_size", "mars_hip_pipe_open",
                   "mars_hip_pipe_input", "mars_hip_pipe_submit", "mars_hip_pipe_wait", "mars_hip_pipe_close", "mars_hip_pipe_camera_ms", "mars_hip_set_output_mode",
                   "mars_hip_get_tuning", "mars_hip_model_set_tuning", "mars_hip_model_get_tuning", "mars_yolo_find_heads",
                   "mars_hip_detect_heads", "mars_hip_detect_heads_device", "mars_hip_detect_results", "mars_yolo_find_dfl_heads",
                   "mars_hip_detect_dfl", "mars_hip_detect_dfl_device", "mars_synth_model_head", "mars_hip_nv12_frame_bytes",
                   "mars_yolo_nv12_to_rgb", "mars_yolo_letterbox_nv12", "mars_hip_preprocess_nv12", "mars_hip_preprocess_nv12_device",
                   "mars_yolo_crop_boxes", "mars_hip_crop_detections_device", "mars_hip_crop_detections", "mars_hip_roi_results",
                   "mars_yolo_classify_maps", "mars_hip_classify_device", "mars_hip_classify_results", "mars_hip_classify",
                   "mars_hip_label_detections_device", "mars_hip_label_results",
                   "mars_yolo_embed_quantise", "mars_hip_gallery_create", "mars_hip_gallery_add", "mars_hip_gallery_count",
                   "mars_hip_gallery_clear", "mars_hip_gallery_free", "mars_hip_match_chunk", "mars_yolo_match_vectors",
                   "mars_hip_match_device", "mars_hip_match_results", "mars_hip_match", "mars_hip_identify_detections_device",
                   "mars_hip_identity_results",
                   "mars_hip_tracker_create", "mars_hip_tracker_reset", "mars_hip_tracker_free", "mars_hip_tracker_read",
                   "mars_yolo_track_lists", "mars_hip_track_device", "mars_hip_track_results", "mars_hip_track",
                   "mars_yolo_track_cosine", "mars_yolo_embed_blend", "mars_hip_tracker_create_app", "mars_hip_tracker_read_embeddings",
                   "mars_yolo_track_lists_app", "mars_hip_track_app_device", "mars_hip_track_app", "mars_yolo_track_cosine_matrix",
                   "mars_hip_detect_seg_device", "mars_hip_mask_results", "mars_hip_detect_seg", "mars_hip_mask_ms", "mars_yolo_masks",
                   "mars_hip_detect_seg_native_device", "mars_hip_mask_native_results", "mars_hip_detect_seg_native", "mars_hip_mask_native_ms",
                   "mars_yolo_mask_taps", "mars_yolo_masks_native",
                   "mars_hip_detect_pose_device", "mars_hip_pose_results", "mars_hip_detect_pose", "mars_hip_pose_ms", "mars_yolo_keypoints",
                   "mars_hip_detect_obb_device", "mars_hip_obb_results", "mars_hip_detect_obb", "mars_hip_obb_ms", "mars_yolo_obb_nms",
                   "mars_yolo_obb_corners", "mars_yolo_crop_obb", "mars_hip_crop_obb_device", "mars_hip_crop_obb",
                   "mars_yolo_align_fit", "mars_yolo_align_template_face5", "mars_yolo_crop_aligned", "mars_hip_crop_pose_device",
                   "mars_hip_crop_pose", "mars_hip_align_results",
                   "mars_tile_grid", "mars_hip_preprocess_tiles_device", "mars_hip_preprocess_tiles", "mars_hip_merge_tiles_device",
                   "mars_hip_tile_results", "mars_hip_tile_frames", "mars_hip_merge_tiles", "mars_hip_tile_ms", "mars_yolo_tile_frames", "mars_yolo_merge_tiles",
                   "mars_yolo_redact_frames", "mars_hip_redact_device", "mars_hip_redact_results", "mars_hip_redact", "mars_hip_redact_ms",
                   "mars_overlay_default_palette", "mars_overlay_rgb_to_yuv", "mars_overlay_glyph", "mars_overlay_text", "mars_yolo_overlay_frames",
                   "mars_hip_overlay_device", "mars_hip_overlay_results", "mars_hip_overlay", "mars_hip_overlay_ms",
                   "mars_hip_motion_create", "mars_hip_motion_reset", "mars_hip_motion_free", "mars_hip_motion_grid", "mars_hip_motion_read",
                   "mars_yolo_motion_frames", "mars_hip_motion_device", "mars_hip_motion_results", "mars_hip_motion_detections_device",
                   "mars_hip_motion_det_results", "mars_yolo_motion_boxes", "mars_hip_motion_ms",
                   "mars_hip_events_create", "mars_hip_events_free", "mars_hip_events_reset", "mars_hip_events_set_rules", "mars_hip_events_read",
                   "mars_hip_events_read_slots", "mars_yolo_event_lists", "mars_hip_events_device", "mars_hip_events_results", "mars_hip_events",
                   "mars_hip_events_ms",
                   "mars_hip_shots_create", "mars_hip_shots_free", "mars_hip_shots_reset", "mars_hip_shots_flush", "mars_hip_shots_read",
                   "mars_hip_shots_read_slots", "mars_hip_shots_read_pixels", "mars_hip_shots_collect", "mars_yolo_shot_lists",
                   "mars_hip_shots_device", "mars_hip_shots_results", "mars_hip_shots", "mars_hip_shots_ms"],
    "mars_compile.h": ["mars_compile_onnx", "mars_compile_file", "mars_compile_last_error"],
}

_lib = None


def lib():
    """dlopen the C-ABI library and declare prototypes.  Raises if it was not built."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise FileNotFoundError("%s not built: run `python -c 'import __graft_entry__ as g; g.build()'`" % LIB_PATH)
    L = C.CDLL(LIB_PATH, mode=os.RTLD_LOCAL)  # never interpose the oracle's same-named symbols
    P = C.POINTER
    L.nna_get_version.restype = C.c_char_p
    L.nna_get_hw_info.argtypes = [P(HwInfo)]
    L.nna_malloc.restype = C.c_void_p
    L.nna_malloc.argtypes = [C.c_size_t]
    L.nna_calloc.restype = C.c_void_p
    L.nna_calloc.argtypes = [C.c_size_t, C.c_size_t]
    L.nna_memalign.restype = C.c_void_p
    L.nna_memalign.argtypes = [C.c_size_t, C.c_size_t]
    L.nna_free.argtypes = [C.c_void_p]
    L.nna_free.restype = None
    L.nna_oram_malloc.restype = C.c_void_p
    L.nna_oram_malloc.argtypes = [C.c_size_t]
    L.nna_oram_get_stats.argtypes = [P(C.c_size_t)] * 3
    L.mars_load_file.argtypes = [C.c_char_p, P(P(MarsModel))]
    L.mars_load_memory.argtypes = [C.c_void_p, C.c_size_t, P(P(MarsModel))]
    L.mars_hip_load_memory_ex.argtypes = [C.c_void_p, C.c_size_t, C.c_uint, P(P(MarsModel))]
    L.mars_hip_describe_plan.restype = C.c_size_t
    L.mars_hip_describe_plan.argtypes = [C.c_void_p, C.c_size_t, C.c_uint, C.c_char_p, C.c_size_t]
    L.mars_free.argtypes = [P(MarsModel)]
    L.mars_free.restype = None
    L.mars_get_input.restype = P(MarsRuntimeTensor)
    L.mars_get_input.argtypes = [P(MarsModel), C.c_int]
    L.mars_get_output.restype = P(MarsRuntimeTensor)
    L.mars_get_output.argtypes = [P(MarsModel), C.c_int]
    L.mars_get_num_inputs.argtypes = [P(MarsModel)]
    L.mars_get_num_outputs.argtypes = [P(MarsModel)]
    L.mars_run.argtypes = [P(MarsModel)]
    L.mars_get_error_string.restype = C.c_char_p
    L.mars_get_error_string.argtypes = [C.c_int]
    L.mars_print_summary.argtypes = [P(MarsModel)]
    L.mars_hip_tensor_frame_bytes.restype = C.c_size_t
    L.mars_hip_tensor_frame_bytes.argtypes = [P(MarsModel), C.c_int]
    L.mars_hip_tensor_byte_size.restype = C.c_size_t
    L.mars_hip_tensor_byte_size.argtypes = [P(MarsTensorDesc)]
    L.mars_hip_pipe_open.argtypes = [P(MarsModel), P(PipeOpts)]
    L.mars_hip_pipe_input.restype = C.c_void_p
    L.mars_hip_pipe_input.argtypes = [P(MarsModel), C.c_int]
    L.mars_hip_pipe_submit.argtypes = [P(MarsModel)]
    L.mars_hip_pipe_camera_ms.restype = C.c_float
    L.mars_hip_pipe_camera_ms.argtypes = [P(MarsModel)]
    L.mars_hip_pipe_wait.argtypes = [P(MarsModel), P(C.c_void_p), P(C.c_void_p), P(C.c_void_p)]
    L.mars_hip_pipe_close.argtypes = [P(MarsModel)]
    L.mars_hip_pipe_close.restype = None
    L.mars_hip_set_output_mode.argtypes = [P(MarsModel), C.c_int]
    for n in ("mars_hip_upload_inputs", "mars_hip_run_device", "mars_hip_run_device_async",
              "mars_hip_download_outputs", "mars_hip_get_batch", "mars_hip_num_ops"):
        getattr(L, n).argtypes = [P(MarsModel)]
    L.mars_hip_set_batch.argtypes = [P(MarsModel), C.c_int]
    L.mars_hip_set_fusion.argtypes = [P(MarsModel), C.c_int]
    L.mars_hip_set_tuning.argtypes = [C.c_char_p, C.c_int]
    L.mars_hip_get_tuning.argtypes = [C.c_char_p, P(C.c_int)]
    L.mars_hip_model_set_tuning.argtypes = [C.c_void_p, C.c_char_p, C.c_int]
    L.mars_hip_model_get_tuning.argtypes = [C.c_void_p, C.c_char_p, P(C.c_int)]
    L.mars_hip_autotune.argtypes = [P(MarsModel), C.c_int]
    L.mars_yolo_letterbox.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_void_p]
    L.mars_hip_preprocess.argtypes = [P(MarsModel), C.c_int, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int]
    L.mars_hip_preprocess_device.argtypes = [P(MarsModel), C.c_int, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int]
    L.mars_hip_nv12_frame_bytes.restype = C.c_size_t
    L.mars_hip_nv12_frame_bytes.argtypes = [C.c_int, C.c_int]
    L.mars_yolo_nv12_to_rgb.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_uint, C.c_void_p]
    L.mars_yolo_letterbox_nv12.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_uint, C.c_void_p]
    L.mars_hip_preprocess_nv12.argtypes = [P(MarsModel), C.c_int, C.c_void_p, C.c_int, C.c_int, C.c_uint, C.c_int, C.c_int]
    L.mars_hip_preprocess_nv12_device.argtypes = [P(MarsModel), C.c_int, C.c_void_p, C.c_int, C.c_int, C.c_uint, C.c_int, C.c_int]
    L.mars_yolo_crop_boxes.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_int, P(RoiOpts), C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p]
    L.mars_hip_crop_detections_device.argtypes = [P(MarsModel), C.c_void_p, P(MarsModel), C.c_int, P(RoiOpts)]
    L.mars_hip_crop_detections.argtypes = [P(MarsModel), C.c_void_p, P(MarsModel), C.c_int, P(RoiOpts)]
    L.mars_hip_roi_results.argtypes = [P(MarsModel), C.c_void_p, C.c_int, P(C.c_int), P(C.c_int)]
    L.mars_yolo_crop_obb.argtypes = L.mars_yolo_crop_boxes.argtypes
    L.mars_hip_crop_obb_device.argtypes = [P(MarsModel), C.c_void_p, P(MarsModel), C.c_int, P(RoiOpts)]
    L.mars_hip_crop_obb.argtypes = [P(MarsModel), C.c_void_p, P(MarsModel), C.c_int, P(RoiOpts)]
    L.mars_yolo_align_fit.argtypes = [C.c_void_p, P(AlignOpts), P(RoiOpts), C.c_int, C.c_int, C.c_void_p, C.c_void_p]
    L.mars_yolo_align_template_face5.argtypes = [C.c_int, C.c_int, C.c_void_p]
    L.mars_yolo_crop_aligned.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_int, P(AlignOpts), P(RoiOpts), C.c_int, C.c_int, C.c_int,
                                         C.c_void_p, C.c_void_p, C.c_void_p]
    L.mars_hip_crop_pose_device.argtypes = [P(MarsModel), C.c_void_p, P(MarsModel), C.c_int, P(RoiOpts), P(AlignOpts)]
    L.mars_hip_crop_pose.argtypes = [P(MarsModel), C.c_void_p, P(MarsModel), C.c_int, P(RoiOpts), P(AlignOpts)]
    L.mars_hip_align_results.argtypes = [P(MarsModel), C.c_void_p, C.c_int]
    L.mars_yolo_classify_maps.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_float, P(ClsOpts), C.c_void_p, C.c_void_p]
    L.mars_hip_classify_device.argtypes = [P(MarsModel), P(ClsOpts)]
    L.mars_hip_classify_results.argtypes = [P(MarsModel), C.c_void_p, C.c_void_p, P(C.c_int)]
    L.mars_hip_classify.argtypes = [P(MarsModel), P(ClsOpts), C.c_void_p, C.c_void_p]
    L.mars_hip_label_detections_device.argtypes = [P(MarsModel), P(MarsModel)]
    L.mars_hip_label_results.argtypes = [P(MarsModel), C.c_void_p]
    L.mars_yolo_embed_quantise.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_void_p]
    L.mars_hip_gallery_create.argtypes = [C.c_int, C.c_int, P(C.c_void_p)]
    L.mars_hip_gallery_add.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int]
    L.mars_hip_gallery_count.argtypes = [C.c_void_p]
    L.mars_hip_gallery_clear.argtypes = [C.c_void_p]
    L.mars_hip_gallery_free.argtypes = [C.c_void_p]
    L.mars_hip_gallery_free.restype = None
    L.mars_hip_match_chunk.argtypes = [C.c_int]
    L.mars_yolo_match_vectors.argtypes = [C.c_void_p, C.c_void_p, C.c_int, P(MatchOpts), C.c_void_p, C.c_void_p]
    L.mars_hip_match_device.argtypes = [P(MarsModel), C.c_void_p, P(MatchOpts)]
    L.mars_hip_match_results.argtypes = [P(MarsModel), C.c_void_p, C.c_void_p]
    L.mars_hip_match.argtypes = [P(MarsModel), C.c_void_p, P(MatchOpts), C.c_void_p, C.c_void_p]
    L.mars_hip_identify_detections_device.argtypes = [P(MarsModel), P(MarsModel)]
    L.mars_hip_identity_results.argtypes = [P(MarsModel), C.c_void_p]
    L.mars_hip_tracker_create.argtypes = [C.c_int, P(C.c_void_p)]
    L.mars_hip_tracker_reset.argtypes = [C.c_void_p]
    L.mars_hip_tracker_free.argtypes = [C.c_void_p]
    L.mars_hip_tracker_free.restype = None
    L.mars_hip_tracker_read.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_int, P(C.c_int), C.c_void_p]
    L.mars_yolo_track_lists.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_int, P(TrackOpts), C.c_void_p]
    L.mars_hip_track_device.argtypes = [P(MarsModel), C.c_void_p, P(TrackOpts)]
    L.mars_hip_track_results.argtypes = [P(MarsModel), C.c_void_p]
    L.mars_hip_track.argtypes = [P(MarsModel), C.c_void_p, P(TrackOpts), C.c_void_p]
    L.mars_yolo_track_cosine.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_int, C.c_int, P(C.c_float)]
    L.mars_yolo_embed_blend.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_int, C.c_int, C.c_void_p, P(C.c_int)]
    L.mars_hip_tracker_create_app.argtypes = [C.c_int, C.c_int, P(C.c_void_p)]
    L.mars_hip_tracker_read_embeddings.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_int, P(C.c_int)]
    L.mars_yolo_track_lists_app.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_int, C.c_int,
                                            P(TrackOpts), P(TrackAppOpts), C.c_void_p]
    L.mars_hip_track_app_device.argtypes = [P(MarsModel), P(MarsModel), C.c_void_p, P(TrackOpts), P(TrackAppOpts)]
    L.mars_hip_track_app.argtypes = [P(MarsModel), P(MarsModel), C.c_void_p, P(TrackOpts), P(TrackAppOpts), C.c_void_p]
    L.mars_yolo_track_cosine_matrix.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_void_p]
    L.mars_hip_detect_seg_device.argtypes = [P(MarsModel), P(YoloDflHeads), P(SegOpts)]
    L.mars_hip_mask_results.argtypes = [P(MarsModel), C.c_void_p, C.c_void_p, P(C.c_int), P(C.c_int), P(C.c_int)]
    L.mars_hip_detect_seg.argtypes = [P(MarsModel), P(YoloDflHeads), P(SegOpts), C.c_void_p, P(C.c_int), C.c_void_p, C.c_void_p]
    L.mars_hip_mask_ms.restype = C.c_float
    L.mars_hip_mask_ms.argtypes = [P(MarsModel)]
    L.mars_yolo_masks.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_int, C.c_int, C.c_float, C.c_float,
                                  C.c_void_p, C.c_void_p]
    L.mars_hip_detect_seg_native_device.argtypes = [P(MarsModel), P(YoloDflHeads), P(SegOpts), P(MaskNativeOpts)]
    L.mars_hip_mask_native_results.argtypes = [P(MarsModel), C.c_void_p, C.c_void_p, P(C.c_int), P(C.c_int), P(C.c_int)]
    L.mars_hip_detect_seg_native.argtypes = [P(MarsModel), P(YoloDflHeads), P(SegOpts), P(MaskNativeOpts), C.c_void_p, P(C.c_int), C.c_void_p,
                                             C.c_void_p]
    L.mars_hip_mask_native_ms.restype = C.c_float
    L.mars_hip_mask_native_ms.argtypes = [P(MarsModel)]
    L.mars_yolo_mask_taps.argtypes = [C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p]
    L.mars_yolo_masks_native.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_int, C.c_int, C.c_void_p, P(MaskGeom), C.c_float, C.c_float,
                                         C.c_void_p, C.c_void_p]
    L.mars_hip_detect_pose_device.argtypes = [P(MarsModel), P(YoloDflHeads), P(PoseOpts)]
    L.mars_hip_pose_results.argtypes = [P(MarsModel), C.c_void_p, C.c_void_p, P(C.c_int)]
    L.mars_hip_detect_pose.argtypes = [P(MarsModel), P(YoloDflHeads), P(PoseOpts), C.c_void_p, P(C.c_int), C.c_void_p, C.c_void_p]
    L.mars_hip_pose_ms.restype = C.c_float
    L.mars_hip_pose_ms.argtypes = [P(MarsModel)]
    L.mars_yolo_keypoints.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_float, C.c_void_p]
    L.mars_hip_detect_obb_device.argtypes = [P(MarsModel), P(YoloDflHeads), P(ObbOpts)]
    L.mars_hip_obb_results.argtypes = [P(MarsModel), C.c_void_p, C.c_void_p]
    L.mars_hip_detect_obb.argtypes = [P(MarsModel), P(YoloDflHeads), P(ObbOpts), C.c_void_p, P(C.c_int), C.c_void_p]
    L.mars_hip_obb_ms.restype = C.c_float
    L.mars_hip_obb_ms.argtypes = [P(MarsModel)]
    L.mars_yolo_obb_nms.argtypes = [C.c_void_p, C.c_int, C.c_float, C.c_uint]
    L.mars_yolo_obb_corners.argtypes = [C.c_void_p, C.c_void_p]
    L.mars_yolo_obb_corners.restype = None
    L.mars_tile_grid.argtypes = [C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_int]
    L.mars_hip_preprocess_tiles_device.argtypes = [P(MarsModel), C.c_int, C.c_void_p, P(TileOpts)]
    L.mars_hip_preprocess_tiles.argtypes = [P(MarsModel), C.c_int, C.c_void_p, P(TileOpts)]
    L.mars_hip_merge_tiles_device.argtypes = [P(MarsModel), P(TileOpts)]
    L.mars_hip_tile_results.argtypes = [P(MarsModel), C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
    L.mars_hip_merge_tiles.argtypes = [P(MarsModel), P(TileOpts), C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
    L.mars_hip_tile_frames.argtypes = [P(MarsModel)]
    L.mars_hip_tile_ms.restype = C.c_float
    L.mars_hip_tile_ms.argtypes = [P(MarsModel)]
    L.mars_yolo_tile_frames.argtypes = [C.c_void_p, C.c_int, P(TileOpts), C.c_int, C.c_int, C.c_int, C.c_void_p]
    L.mars_yolo_merge_tiles.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_int, P(TileOpts), C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p,
                                        C.c_void_p]
    L.mars_yolo_redact_frames.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, P(RedactOpts), C.c_void_p,
                                          C.c_void_p]
    L.mars_hip_redact_device.argtypes = [P(MarsModel), C.c_void_p, C.c_void_p, P(RedactOpts)]
    L.mars_hip_redact_results.argtypes = [P(MarsModel), C.c_void_p]
    L.mars_hip_redact.argtypes = [P(MarsModel), C.c_void_p, P(RedactOpts), C.c_void_p]
    L.mars_hip_redact_ms.restype = C.c_float
    L.mars_hip_redact_ms.argtypes = [P(MarsModel)]
    L.mars_overlay_default_palette.argtypes = [C.c_void_p]
    L.mars_overlay_rgb_to_yuv.restype = None
    L.mars_overlay_rgb_to_yuv.argtypes = [C.c_void_p, C.c_uint, C.c_void_p]
    L.mars_overlay_glyph.restype = None
    L.mars_overlay_glyph.argtypes = [C.c_int, C.c_void_p]
    L.mars_overlay_text.argtypes = [C.c_uint, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_float, C.c_void_p]
    L.mars_yolo_overlay_frames.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p,
                                           C.c_void_p, C.c_int, P(OverlayOpts), C.c_void_p, C.c_void_p]
    L.mars_hip_overlay_device.argtypes = [P(MarsModel), C.c_void_p, C.c_void_p, P(OverlayOpts)]
    L.mars_hip_overlay_results.argtypes = [P(MarsModel), C.c_void_p]
    L.mars_hip_overlay.argtypes = [P(MarsModel), C.c_void_p, P(OverlayOpts), C.c_void_p]
    L.mars_hip_overlay_ms.restype = C.c_float
    L.mars_hip_overlay_ms.argtypes = [P(MarsModel)]
    L.mars_hip_motion_create.argtypes = [C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, P(C.c_void_p)]
    L.mars_hip_motion_reset.argtypes = [C.c_void_p, C.c_int]
    L.mars_hip_motion_free.argtypes = [C.c_void_p]
    L.mars_hip_motion_free.restype = None
    L.mars_hip_motion_grid.argtypes = [C.c_int, C.c_int, C.c_int, P(C.c_int), P(C.c_int), P(C.c_int)]
    L.mars_hip_motion_read.argtypes = [C.c_void_p, C.c_int, C.c_void_p, P(C.c_int)]
    L.mars_yolo_motion_frames.argtypes = [C.c_void_p, C.c_void_p, C.c_int, P(MotionOpts), C.c_void_p, C.c_void_p, C.c_void_p]
    L.mars_hip_motion_device.argtypes = [C.c_void_p, C.c_void_p, C.c_int, P(MotionOpts)]
    L.mars_hip_motion_results.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
    L.mars_hip_motion_detections_device.argtypes = [P(MarsModel), C.c_void_p, C.c_float]
    L.mars_hip_motion_det_results.argtypes = [P(MarsModel), C.c_void_p]
    L.mars_yolo_motion_boxes.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_float, C.c_void_p]
    L.mars_hip_motion_ms.restype = C.c_float
    L.mars_hip_motion_ms.argtypes = [C.c_void_p]
    L.mars_hip_events_create.argtypes = [C.c_int, P(C.c_void_p)]
    L.mars_hip_events_free.argtypes = [C.c_void_p]
    L.mars_hip_events_free.restype = None
    L.mars_hip_events_reset.argtypes = [C.c_void_p, C.c_int]
    L.mars_hip_events_set_rules.argtypes = [C.c_void_p, C.c_int, P(EventRules)]
    L.mars_hip_events_read.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, P(C.c_int), P(C.c_int)]
    L.mars_hip_events_read_slots.argtypes = [C.c_void_p, C.c_int, C.c_void_p]
    L.mars_yolo_event_lists.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_int, P(EventsOpts), C.c_void_p, C.c_void_p,
                                        C.c_void_p]
    L.mars_hip_events_device.argtypes = [P(MarsModel), C.c_void_p, P(EventsOpts)]
    L.mars_hip_events_results.argtypes = [P(MarsModel), C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
    L.mars_hip_events.argtypes = [P(MarsModel), C.c_void_p, P(EventsOpts), C.c_void_p, C.c_void_p, C.c_void_p]
    L.mars_hip_events_ms.restype = C.c_float
    L.mars_hip_events_ms.argtypes = [C.c_void_p]
    L.mars_hip_shots_create.argtypes = [C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, P(C.c_void_p)]
    L.mars_hip_shots_free.argtypes = [C.c_void_p]
    L.mars_hip_shots_free.restype = None
    L.mars_hip_shots_reset.argtypes = [C.c_void_p, C.c_int]
    L.mars_hip_shots_flush.argtypes = [C.c_void_p, C.c_int]
    L.mars_hip_shots_read.argtypes = [C.c_void_p, C.c_int, C.c_void_p, P(C.c_int), P(C.c_int), P(C.c_int)]
    L.mars_hip_shots_read_slots.argtypes = [C.c_void_p, C.c_int, C.c_void_p]
    L.mars_hip_shots_read_pixels.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_void_p]
    L.mars_hip_shots_collect.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_int, P(C.c_int)]
    L.mars_yolo_shot_lists.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_int, P(ShotOpts),
                                       C.c_void_p]
    L.mars_hip_shots_device.argtypes = [P(MarsModel), P(MarsModel), C.c_int, C.c_void_p, P(ShotOpts)]
    L.mars_hip_shots_results.argtypes = [P(MarsModel), C.c_void_p, C.c_void_p]
    L.mars_hip_shots.argtypes = [P(MarsModel), P(MarsModel), C.c_int, C.c_void_p, P(ShotOpts), C.c_void_p]
    L.mars_hip_shots_ms.restype = C.c_float
    L.mars_hip_shots_ms.argtypes = [C.c_void_p]
    L.mars_hip_set_profiling.argtypes = [P(MarsModel), C.c_int]
    L.mars_hip_set_profiling.restype = None
    L.mars_hip_tensor_device.restype = C.c_void_p
    L.mars_hip_tensor_device.argtypes = [P(MarsModel), C.c_int, P(C.c_size_t)]
    L.mars_hip_read_tensor.argtypes = [P(MarsModel), C.c_int, C.c_int, C.c_void_p, C.c_size_t]
    L.mars_hip_tensor_row_pitch.argtypes = [P(MarsModel), C.c_int, P(C.c_int)]
    L.mars_hip_write_tensor.argtypes = [P(MarsModel), C.c_int, C.c_int, C.c_void_p, C.c_size_t]
    L.mars_hip_op_info.argtypes = [P(MarsModel), C.c_int, P(C.c_int), P(C.c_int), P(C.c_double), P(C.c_double),
                                   P(C.c_float)]
    L.mars_hip_stream.restype = C.c_void_p
    L.mars_hip_param_arena.restype = C.c_void_p
    L.mars_hip_param_arena.argtypes = [P(MarsModel), P(C.c_size_t)]
    L.mars_yolo_parse_output.argtypes = [C.c_void_p, C.c_int, C.c_float, C.c_void_p, C.c_int]
    L.mars_yolo_nms.argtypes = [C.c_void_p, C.c_int, C.c_float]
    L.mars_hip_detect.argtypes = [P(MarsModel), P(C.c_int), C.c_int, C.c_float, C.c_void_p, P(C.c_int)]
    L.mars_hip_detect_device.argtypes = [P(MarsModel), P(C.c_int), C.c_int, C.c_float]
    L.mars_yolo_find_heads.argtypes = [C.c_void_p, C.c_size_t, P(C.c_int), P(C.c_int), P(C.c_int), C.c_int]
    L.mars_hip_detect_heads.argtypes = [P(MarsModel), P(YoloHeads), C.c_void_p, P(C.c_int)]
    L.mars_hip_detect_heads_device.argtypes = [P(MarsModel), P(YoloHeads)]
    L.mars_hip_detect_results.argtypes = [P(MarsModel), C.c_void_p, P(C.c_int)]
    L.mars_yolo_find_dfl_heads.argtypes = [C.c_void_p, C.c_size_t, P(C.c_int), P(C.c_int), P(C.c_int), P(C.c_int), P(C.c_int), C.c_int]
    L.mars_hip_detect_dfl.argtypes = [P(MarsModel), P(YoloDflHeads), C.c_void_p, P(C.c_int)]
    L.mars_hip_detect_dfl_device.argtypes = [P(MarsModel), P(YoloDflHeads)]
    L.mars_compile_onnx.restype = C.c_size_t
    L.mars_compile_onnx.argtypes = [C.c_char_p, C.c_size_t, P(CompileOpts), C.c_void_p, C.c_size_t]
    L.mars_compile_file.argtypes = [C.c_char_p, C.c_char_p, P(CompileOpts)]
    L.mars_compile_last_error.restype = C.c_char_p
    L.mars_synth_model.restype = C.c_size_t
    L.mars_synth_model.argtypes = [P(SynthOpts), C.c_void_p, C.c_size_t]
    L.mars_synth_model_head.restype = C.c_size_t
    L.mars_synth_model_head.argtypes = [P(SynthOpts), C.c_int, C.c_void_p, C.c_size_t]
    conv_args = [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_void_p,
                 C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int]
    for n in ("conv2d_int8_mxu", "conv2d_int8_nhwc_mxu"):
        getattr(L, n).argtypes = conv_args + [C.c_float, C.c_float, C.c_float]
        getattr(L, n).restype = None
    L.conv2d_float32_mxu.argtypes = conv_args + [C.c_void_p]
    L.conv2d_float32_mxu.restype = None
    for n in ("mxu_mul_f32", "mxu_add_f32", "mxu_sub_f32"):
        getattr(L, n).argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_size_t]
        getattr(L, n).restype = None
    L.mxu_relu_f32.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t]
    L.mxu_relu_f32.restype = None
    _lib = L
    return L


class MarsError(RuntimeError):
    def __init__(self, code, what=""):
        self.code = code
        msg = lib().mars_get_error_string(code).decode()
        super().__init__("%s: %s (%d)" % (what, msg, code))


def set_tuning(key, value):
    """Launch-policy knob of the conv kernels (mars_hip_set_tuning); results never depend on it."""
    if lib().mars_hip_set_tuning(key.encode(), int(value)) != 0:
        raise KeyError(key)


def get_tuning(key):
    v = C.c_int(0)
    if lib().mars_hip_get_tuning(key.encode(), C.byref(v)) != 0:
        raise KeyError(key)
    return v.value


def letterbox(rgb, tw, th, nhwc=True):
    """mars_yolo_letterbox: uint8 RGB [h][w][3] -> int8 letterboxed frame, on the GPU."""
    rgb = np.ascontiguousarray(rgb, dtype=np.uint8)
    h, w = rgb.shape[:2]
    out = np.zeros(tw * th * 3, dtype=np.int8)
    if lib().mars_yolo_letterbox(rgb.ctypes.data, w, h, tw, th, int(bool(nhwc)), out.ctypes.data) != 0:
        raise RuntimeError("mars_yolo_letterbox failed")
    return out


def _nv12_frames(nv12, w, h, batched):
    """NV12 bytes as a contiguous uint8 array of [n, w * h * 3 / 2] (batched) or [w * h * 3 / 2]; the size must fit (odd sizes: the
    library refuses them, so whatever arrives is passed on)"""
    a = np.ascontiguousarray(nv12, dtype=np.uint8)
    fb = lib().mars_hip_nv12_frame_bytes(int(w), int(h))
    if fb:
        a = a.reshape(-1, fb) if batched else a.reshape(-1)
        if not batched and a.size != fb:
            raise ValueError("an NV12 frame of %d x %d is %d bytes, got %d" % (w, h, fb, a.size))
    return a


def nv12_to_rgb(nv12, w, h, flags=0):
    """mars_yolo_nv12_to_rgb: one NV12 frame (w * h * 3 / 2 bytes: Y plane, then interleaved chroma) -> uint8 RGB [h][w][3], on the GPU."""
    a = _nv12_frames(nv12, w, h, False)
    out = np.zeros((max(int(h), 0), max(int(w), 0), 3), dtype=np.uint8)
    if lib().mars_yolo_nv12_to_rgb(a.ctypes.data, int(w), int(h), int(flags), out.ctypes.data) != 0:
        raise RuntimeError("mars_yolo_nv12_to_rgb failed")
    return out


def letterbox_nv12(nv12, w, h, tw, th, nhwc=True, flags=0):
    """mars_yolo_letterbox_nv12: one NV12 frame -> int8 letterboxed frame, on the GPU (what letterbox() gives for nv12_to_rgb() of it)."""
    a = _nv12_frames(nv12, w, h, False)
    out = np.zeros(tw * th * 3, dtype=np.int8)
    if lib().mars_yolo_letterbox_nv12(a.ctypes.data, int(w), int(h), tw, th, int(bool(nhwc)), int(flags), out.ctypes.data) != 0:
        raise RuntimeError("mars_yolo_letterbox_nv12 failed")
    return out


def roi_opts(w, h, fmt=CAMERA_RGB, src_flags=0, expand=0.0, min_conf=0.0, min_size=0, classes=None, max_per_frame=0, keep_aspect=False,
             area=False):
    """mars_hip_roi_opts_t for frames of w x h.  classes = (first, count): the class window; area: box-filter the down-scaled axes
    (MARS_ROI_AREA; the rotated calls refuse it); zero means default everywhere else"""
    o = RoiOpts(int(w), int(h), int(fmt), int(src_flags), float(expand), float(min_conf), int(min_size))
    if classes is not None:
        o.cls_first, o.cls_count = int(classes[0]), int(classes[1])
    o.max_per_frame = int(max_per_frame)
    o.flags = (ROI_KEEP_ASPECT if keep_aspect else 0) | (ROI_AREA if area else 0)
    return o


def _crop_host(fn, dtype, frames, boxes, frame_of_box, opts, tw, th, nhwc):
    a = np.ascontiguousarray(frames, dtype=np.uint8).reshape(-1)
    fb = opts.src_w * opts.src_h * 3 // (2 if opts.src_format == CAMERA_NV12 else 1)
    if fb <= 0 or a.size % fb:
        raise ValueError("frames of %d x %d are %d bytes each, got %d" % (opts.src_w, opts.src_h, fb, a.size))
    b = np.ascontiguousarray(boxes, dtype=dtype).reshape(-1)
    fo = np.ascontiguousarray(frame_of_box, dtype=np.int32).reshape(-1)
    if fo.size != b.size:
        raise ValueError("one frame index per box")
    out = np.zeros((b.size, tw * th * 3), dtype=np.int8)
    rois = np.zeros(b.size, dtype=ROI_DTYPE)
    rc = getattr(lib(), fn)(a.ctypes.data, a.size // fb, b.ctypes.data, fo.ctypes.data, b.size, C.byref(opts), tw, th, int(bool(nhwc)),
                            out.ctypes.data, rois.ctypes.data)
    if rc != MARS_OK:
        raise MarsError(rc, fn)
    return out, rois


def crop_boxes(frames, boxes, frame_of_box, opts, tw, th, nhwc=True):
    """mars_yolo_crop_boxes: frames (uint8, [n] frames of opts.src_w x opts.src_h, RGB or NV12) and boxes (DET_DTYPE records, box i in frame
    frame_of_box[i]) -> (int8 crops [n_boxes][tw * th * 3], ROI_DTYPE records [n_boxes]; x1 == x0: skipped, its crop is all -17), on the GPU"""
    return _crop_host("mars_yolo_crop_boxes", DET_DTYPE, frames, boxes, frame_of_box, opts, tw, th, nhwc)


def crop_obb(frames, boxes, frame_of_box, opts, tw, th, nhwc=True):
    """mars_yolo_crop_obb: crop_boxes for oriented boxes (OBB_DTYPE records), each cut along its own axes ("Rotated crops"); x0 .. y1 of the
    ROI records = the enclosing rectangle"""
    return _crop_host("mars_yolo_crop_obb", OBB_DTYPE, frames, boxes, frame_of_box, opts, tw, th, nhwc)


def align_opts(tmpl, use=0, min_vis=0.0):
    """mars_hip_align_opts_t ("Aligned crops"): tmpl = K template points (u, v) in target pixels; use = the mask of the keypoints that may take
    part (0: all K); min_vis = the visibility a keypoint needs.  More than POSE_MAX_KPT points give num_kpt = their number, which the
    library refuses"""
    t = np.asarray(tmpl, dtype=np.float32).reshape(-1, 2)
    o = AlignOpts()
    o.num_kpt = len(t)
    for j in range(min(len(t), POSE_MAX_KPT)):
        o.tmpl[j][0], o.tmpl[j][1] = float(t[j, 0]), float(t[j, 1])
    o.use, o.min_vis = int(use), float(min_vis)
    return o


def align_template_face5(tw, th):
    """mars_yolo_align_template_face5: the public 5-point face template scaled to a tw x th target -> float32 [5][2]"""
    t = np.zeros((5, 2), dtype=np.float32)
    if lib().mars_yolo_align_template_face5(int(tw), int(th), t.ctypes.data) != 5:
        raise ValueError("mars_yolo_align_template_face5 refuses this size")
    return t


def align_fit(kpts, align, opts, tw, th):
    """mars_yolo_align_fit, pure host code: one keypoint set (KPT_DTYPE [K]) -> (kept, one ALIGN_DTYPE record, (x0, y0, x1, y1)); ValueError
    where the library returns -1"""
    k = np.ascontiguousarray(kpts, dtype=KPT_DTYPE).reshape(-1)
    if k.size < align.num_kpt:
        raise ValueError("%d keypoints for a template of %d" % (k.size, align.num_kpt))
    fit = np.zeros((), dtype=ALIGN_DTYPE)
    roi = np.zeros((), dtype=ROI_DTYPE)
    rc = lib().mars_yolo_align_fit(k.ctypes.data, C.byref(align), C.byref(opts), int(tw), int(th), fit.ctypes.data, roi.ctypes.data)
    if rc < 0:
        raise ValueError("mars_yolo_align_fit refuses these arguments")
    return bool(rc), fit, (int(roi["x0"]), int(roi["y0"]), int(roi["x1"]), int(roi["y1"]))


def crop_aligned(frames, kpts, frame_of_box, align, opts, tw, th, nhwc=True):
    """mars_yolo_crop_aligned: crop_boxes for keypoint sets (KPT_DTYPE [n_boxes][K]), each fitted to the template of `align` and cut with the
    rotated sampler ("Aligned crops") -> (int8 crops, ROI_DTYPE records, ALIGN_DTYPE records); a skipped box: -17, zeros, zeros"""
    a = np.ascontiguousarray(frames, dtype=np.uint8).reshape(-1)
    fb = opts.src_w * opts.src_h * 3 // (2 if opts.src_format == CAMERA_NV12 else 1)
    if fb <= 0 or a.size % fb:
        raise ValueError("frames of %d x %d are %d bytes each, got %d" % (opts.src_w, opts.src_h, fb, a.size))
    K = max(int(align.num_kpt), 1)
    k = np.ascontiguousarray(kpts, dtype=KPT_DTYPE).reshape(-1, K)
    fo = np.ascontiguousarray(frame_of_box, dtype=np.int32).reshape(-1)
    if fo.size != len(k):
        raise ValueError("one frame index per keypoint set")
    out = np.zeros((len(k), tw * th * 3), dtype=np.int8)
    rois = np.zeros(len(k), dtype=ROI_DTYPE)
    fits = np.zeros(len(k), dtype=ALIGN_DTYPE)
    rc = lib().mars_yolo_crop_aligned(a.ctypes.data, a.size // fb, k.ctypes.data, fo.ctypes.data, len(k), C.byref(align), C.byref(opts), tw, th,
                                      int(bool(nhwc)), out.ctypes.data, rois.ctypes.data, fits.ctypes.data)
    if rc != MARS_OK:
        raise MarsError(rc, "mars_yolo_crop_aligned")
    return out, rois, fits


def tile_grid(W, H, tile_w, tile_h, overlap_x=0, overlap_y=0):
    """mars_tile_grid: the tile table (TILE_DTYPE records, row-major) of a W x H frame; ValueError where the library returns -1"""
    n = lib().mars_tile_grid(int(W), int(H), int(tile_w), int(tile_h), int(overlap_x), int(overlap_y), None, 0)
    if n < 0:
        raise ValueError("mars_tile_grid refuses these sizes")
    tiles = np.zeros(n, dtype=TILE_DTYPE)
    if lib().mars_tile_grid(int(W), int(H), int(tile_w), int(tile_h), int(overlap_x), int(overlap_y), tiles.ctypes.data, n) != n:
        raise RuntimeError("mars_tile_grid changed its mind")
    return tiles


def tile_opts(w, h, tiles, fmt=CAMERA_RGB, src_flags=0, keep_aspect=False, ios=False, agnostic=False, merge_thresh=0.0, edge_margin=0.0,
              max_per_tile=0, flags=0, area=False):
    """mars_hip_tile_opts_t for camera frames of w x h cut by `tiles` (TILE_DTYPE records, or rows of x0, y0, x1, y1); zero means default
    everywhere else; area: MARS_TILE_AREA, the front-end box-filters the down-scaled axes.  The table is copied and kept alive by the returned object"""
    t = np.ascontiguousarray(tiles)
    if t.dtype != TILE_DTYPE:
        t = np.ascontiguousarray(np.asarray(tiles, dtype=np.int32).reshape(-1, 4)).view(TILE_DTYPE).reshape(-1)
    t = t.reshape(-1).copy()
    f = int(flags) | (TILE_KEEP_ASPECT if keep_aspect else 0) | (TILE_MATCH_IOS if ios else 0) | (TILE_AGNOSTIC if agnostic else 0) | (TILE_AREA if area else 0)
    o = TileOpts(int(w), int(h), int(fmt), int(src_flags), int(t.size), t.ctypes.data, f, float(merge_thresh), float(edge_margin), int(max_per_tile))
    o._table = t
    return o


def _tile_frame_bytes(opts):
    return opts.src_w * opts.src_h * 3 // (2 if opts.src_format == CAMERA_NV12 else 1)


def tile_frames(frames, opts, tw, th, nhwc=True):
    """mars_yolo_tile_frames: camera frames (uint8, [n] frames of opts.src_w x opts.src_h, RGB or NV12) -> int8 tiles
    [n * n_tiles][tw * th * 3], on the GPU"""
    a = np.ascontiguousarray(frames, dtype=np.uint8).reshape(-1)
    fb = _tile_frame_bytes(opts)
    if fb <= 0 or a.size % fb:
        raise ValueError("frames of %d x %d are %d bytes each, got %d" % (opts.src_w, opts.src_h, fb, a.size))
    n = a.size // fb
    out = np.zeros((n * max(opts.n_tiles, 0), tw * th * 3), dtype=np.int8)
    rc = lib().mars_yolo_tile_frames(a.ctypes.data, n, C.byref(opts), int(tw), int(th), int(bool(nhwc)), out.ctypes.data)
    if rc != MARS_OK:
        raise MarsError(rc, "mars_yolo_tile_frames")
    return out


def merge_tiles(dets, counts, opts, tw, th):
    """mars_yolo_merge_tiles: dets (DET_DTYPE [n * n_tiles][max_det], pixels of a tw x th input) and counts [n * n_tiles] ->
    (DET_DTYPE [n][MAX_DET] in camera pixels, counts [n], TILE_SRC_DTYPE [n][MAX_DET], TILE_STATS_DTYPE [n]), on the GPU"""
    d = np.ascontiguousarray(dets, dtype=DET_DTYPE)
    c = np.ascontiguousarray(counts, dtype=np.int32).reshape(-1)
    if d.ndim != 2 or d.shape[0] != c.size or opts.n_tiles <= 0 or c.size % opts.n_tiles:
        raise ValueError("dets is [n * n_tiles][max_det], counts [n * n_tiles]")
    n = c.size // opts.n_tiles
    out = np.zeros((n, MAX_DET), dtype=DET_DTYPE)
    oc = np.zeros(n, dtype=np.int32)
    org = np.zeros((n, MAX_DET), dtype=TILE_SRC_DTYPE)
    st = np.zeros(n, dtype=TILE_STATS_DTYPE)
    rc = lib().mars_yolo_merge_tiles(d.ctypes.data, c.ctypes.data, n, d.shape[1], C.byref(opts), int(tw), int(th), out.ctypes.data, oc.ctypes.data,
                                     org.ctypes.data, st.ctypes.data)
    if rc != MARS_OK:
        raise MarsError(rc, "mars_yolo_merge_tiles")
    return out, oc, org, st


def redact_opts(w, h, fmt=CAMERA_RGB, src_flags=0, mode=REDACT_MOSAIC, cell=0, fill=(0, 0, 0), expand=0.0, min_conf=0.0, ident_min=0.0,
                classes=None, use_masks=False, spare_identified=False, flags=None):
    """mars_hip_redact_opts_t for frames of w x h.  mode: REDACT_MOSAIC / REDACT_FILL; cell: 2 .. 64, a power of two (0: 16); fill = (R, G, B)
    or (Y, U, V); classes = (first, count): the class window; use_masks / spare_identified: the device form's flags (flags overrides both);
    zero means default everywhere else"""
    o = RedactOpts(int(w), int(h), int(fmt), int(src_flags), int(mode), int(cell))
    o.fill[:] = [int(v) for v in fill]
    o.expand, o.min_conf, o.ident_min = float(expand), float(min_conf), float(ident_min)
    if classes is not None:
        o.cls_first, o.cls_count = int(classes[0]), int(classes[1])
    o.flags = int(flags) if flags is not None else (REDACT_USE_MASKS if use_masks else 0) | (REDACT_SPARE_IDENTIFIED if spare_identified else 0)
    return o


def redact_frame_bytes(opts):
    return opts.src_w * opts.src_h * 3 // (2 if opts.src_format == CAMERA_NV12 else 1)


def redact_frames(frames, boxes, frame_of_box, opts, mask_words=None, mask_of_box=None, inplace=False):
    """mars_yolo_redact_frames: frames (uint8, [n] frames of opts.src_w x opts.src_h, RGB or NV12) with the regions of boxes (DET_DTYPE records,
    box i in frame frame_of_box[i]) mosaicked or filled, on the GPU -> (the redacted frames, uint8 [n][frame bytes]; REDACT_STATS_DTYPE [n]).
    mask_words = uint32 [n_masks][h][(w + 31) / 32] and mask_of_box = [n_boxes] indices into it (-1: the rectangle alone), or both None.
    inplace: the in-place kernels run (on a copy: the caller's array is left alone)"""
    a = np.ascontiguousarray(frames, dtype=np.uint8).reshape(-1)
    fb = redact_frame_bytes(opts)
    if fb <= 0 or a.size == 0 or a.size % fb:
        raise ValueError("frames of %d x %d are %d bytes each, got %d" % (opts.src_w, opts.src_h, fb, a.size))
    b = np.ascontiguousarray(boxes, dtype=DET_DTYPE).reshape(-1)
    fo = np.ascontiguousarray(frame_of_box, dtype=np.int32).reshape(-1)
    if fo.size != b.size:
        raise ValueError("one frame index per box")
    mw = mo = None
    if mask_of_box is not None:
        mo = np.ascontiguousarray(mask_of_box, dtype=np.int32).reshape(-1)
        pitch = (opts.src_w + 31) // 32
        mw = np.ascontiguousarray(mask_words if mask_words is not None else np.zeros(0), dtype=np.uint32).reshape(-1)
        if mo.size != b.size or mw.size % (opts.src_h * pitch) or (mo.size and int(mo.max()) >= mw.size // (opts.src_h * pitch)):
            raise ValueError("mask_of_box: one index per box, inside mask_words [.][%d][%d]" % (opts.src_h, pitch))
    n = a.size // fb
    out = a.copy() if inplace else np.zeros_like(a)
    src = out if inplace else a
    stats = np.zeros(n, dtype=REDACT_STATS_DTYPE)
    rc = lib().mars_yolo_redact_frames(src.ctypes.data, n, b.ctypes.data if b.size else None, fo.ctypes.data if b.size else None, b.size,
                                       mw.ctypes.data if mw is not None and mw.size else None, mo.ctypes.data if mo is not None and mo.size else None,
                                       C.byref(opts), out.ctypes.data, stats.ctypes.data)
    if rc != MARS_OK:
        raise MarsError(rc, "mars_yolo_redact_frames")
    return out.reshape(n, fb), stats


def overlay_default_palette():
    """mars_overlay_default_palette: the built-in palette, uint8 [16][3] R, G, B; host only"""
    out = np.zeros((16, 3), dtype=np.uint8)
    assert lib().mars_overlay_default_palette(out.ctypes.data) == 16
    return out


def rgb_to_yuv(rgb, flags=0):
    """mars_overlay_rgb_to_yuv: (R, G, B) -> (Y, first stored chroma byte, second), flags = NV12_*; host only"""
    a = np.array([int(v) for v in rgb], dtype=np.uint8)
    out = np.zeros(3, dtype=np.uint8)
    lib().mars_overlay_rgb_to_yuv(a.ctypes.data, int(flags), out.ctypes.data)
    return tuple(int(v) for v in out)


def overlay_glyph(byte):
    """mars_overlay_glyph: the seven row bytes of the glyph that `byte` (any int) shows as; host only"""
    out = np.zeros(7, dtype=np.uint8)
    lib().mars_overlay_glyph(int(byte), out.ctypes.data)
    return out


def overlay_names(names):
    """a list of str / bytes -> the NUL-padded table uint8 [n][OVERLAY_NAME_LEN] (longer names are cut)"""
    t = np.zeros((len(names), OVERLAY_NAME_LEN), dtype=np.uint8)
    for i, s in enumerate(names):
        b = (s.encode("latin-1") if isinstance(s, str) else bytes(s))[:OVERLAY_NAME_LEN]
        t[i, :len(b)] = np.frombuffer(b, dtype=np.uint8)
    return t


def overlay_text(cls, conf, track_id=-1, text=0, names=None):
    """mars_overlay_text: the label bytes the device form composes for a detection; names: None, a list, or an overlay_names() table; host only"""
    t = None
    if names is not None:
        t = names if isinstance(names, np.ndarray) else overlay_names(names)
        t = np.ascontiguousarray(t, dtype=np.uint8).reshape(-1, OVERLAY_NAME_LEN)
    out = np.zeros(OVERLAY_TEXT_MAX, dtype=np.uint8)
    n = lib().mars_overlay_text(int(text), t.ctypes.data if t is not None and len(t) else None, len(t) if t is not None else 0, int(cls),
                                int(track_id), C.c_float(float(conf)), out.ctypes.data)
    return out[:n].tobytes()


def overlay_opts(w, h, fmt=CAMERA_RGB, src_flags=0, layers=0, color_by=OVERLAY_BY_CLASS, text=0, thickness=0, radius=0, scale=0, alpha=0,
                 no_key=(0, 0, 0), min_conf=0.0, kpt_min_v=0.0, classes=None, min_hits=0, tracked_only=False, flags=None, palette=None, names=None):
    """mars_hip_overlay_opts_t for frames of w x h.  layers: OVERLAY_MASKS | _BOXES | _KEYPOINTS | _LABELS (0: boxes and labels); color_by:
    OVERLAY_BY_CLASS / _BY_TRACK / _FIXED; text: OVERLAY_TEXT_* (0: class and confidence); palette: uint8 [P][3] (None: the built-in one); names:
    a list or an overlay_names() table; classes = (first, count): the class window; zero means default everywhere else.  The returned record
    keeps the palette and names arrays alive"""
    o = OverlayOpts(int(w), int(h), int(fmt), int(src_flags), int(layers), int(color_by), int(text), int(thickness), int(radius), int(scale),
                    int(alpha))
    o.no_key[:] = [int(v) for v in no_key]
    o.min_conf, o.kpt_min_v, o.min_hits = float(min_conf), float(kpt_min_v), int(min_hits)
    if classes is not None:
        o.cls_first, o.cls_count = int(classes[0]), int(classes[1])
    o.flags = int(flags) if flags is not None else (OVERLAY_TRACKED_ONLY if tracked_only else 0)
    if palette is not None:
        o._palette = np.ascontiguousarray(palette, dtype=np.uint8).reshape(-1, 3)
        o.n_palette, o.palette = len(o._palette), o._palette.ctypes.data
    if names is not None:
        o._names = np.ascontiguousarray(names if isinstance(names, np.ndarray) else overlay_names(names), dtype=np.uint8).reshape(-1, OVERLAY_NAME_LEN)
        o.n_names, o.names = len(o._names), o._names.ctypes.data
    return o


def overlay_frames(frames, boxes, frame_of_box, opts, keys=None, texts=None, mask_words=None, mask_of_box=None, kpts=None, inplace=False):
    """mars_yolo_overlay_frames: frames (uint8, [n] frames of opts.src_w x opts.src_h, RGB or NV12) with the boxes (DET_DTYPE records, box i in
    frame frame_of_box[i]) painted in on the GPU -> (the painted frames, uint8 [n][frame bytes]; OVERLAY_STATS_DTYPE [n]).  keys = int32
    [n_boxes] colour keys; texts = a list of bytes / str or uint8 [n_boxes][OVERLAY_TEXT_MAX]; mask_words / mask_of_box as in redact_frames;
    kpts = KPT_DTYPE [n_boxes][K]; each may be None.  inplace: the in-place kernels run (on a copy: the caller's array is left alone)"""
    a = np.ascontiguousarray(frames, dtype=np.uint8).reshape(-1)
    fb = redact_frame_bytes(opts)
    if fb <= 0 or a.size == 0 or a.size % fb:
        raise ValueError("frames of %d x %d are %d bytes each, got %d" % (opts.src_w, opts.src_h, fb, a.size))
    b = np.ascontiguousarray(boxes, dtype=DET_DTYPE).reshape(-1)
    fo = np.ascontiguousarray(frame_of_box, dtype=np.int32).reshape(-1)
    if fo.size != b.size:
        raise ValueError("one frame index per box")
    ky = tx = kp = mw = mo = None
    K = 0
    if keys is not None:
        ky = np.ascontiguousarray(keys, dtype=np.int32).reshape(-1)
        if ky.size != b.size:
            raise ValueError("one key per box")
    if texts is not None:
        if isinstance(texts, np.ndarray):
            tx = np.ascontiguousarray(texts, dtype=np.uint8).reshape(-1, OVERLAY_TEXT_MAX)
        else:
            tx = np.zeros((len(texts), OVERLAY_TEXT_MAX), dtype=np.uint8)
            for i, s in enumerate(texts):
                t = (s.encode("latin-1") if isinstance(s, str) else bytes(s))[:OVERLAY_TEXT_MAX]
                tx[i, :len(t)] = np.frombuffer(t, dtype=np.uint8)
        if len(tx) != b.size:
            raise ValueError("one text per box")
    if kpts is not None and b.size:
        kp = np.ascontiguousarray(kpts, dtype=KPT_DTYPE).reshape(b.size, -1)
        K = kp.shape[1]
    if mask_of_box is not None:
        mo = np.ascontiguousarray(mask_of_box, dtype=np.int32).reshape(-1)
        pitch = (opts.src_w + 31) // 32
        mw = np.ascontiguousarray(mask_words if mask_words is not None else np.zeros(0), dtype=np.uint32).reshape(-1)
        if mo.size != b.size or mw.size % (opts.src_h * pitch) or (mo.size and int(mo.max()) >= mw.size // (opts.src_h * pitch)):
            raise ValueError("mask_of_box: one index per box, inside mask_words [.][%d][%d]" % (opts.src_h, pitch))
    n = a.size // fb
    out = a.copy() if inplace else np.zeros_like(a)
    src = out if inplace else a
    stats = np.zeros(n, dtype=OVERLAY_STATS_DTYPE)
    ptr = lambda x: x.ctypes.data if x is not None and x.size else None
    rc = lib().mars_yolo_overlay_frames(src.ctypes.data, n, ptr(b), ptr(fo) if b.size else None, b.size, ptr(ky), ptr(tx), ptr(mw), ptr(mo), ptr(kp), K,
                                        C.byref(opts), out.ctypes.data, stats.ctypes.data)
    if rc != MARS_OK:
        raise MarsError(rc, "mars_yolo_overlay_frames")
    return out.reshape(n, fb), stats


def motion_grid(w, h, cell=0):
    """mars_hip_motion_grid: (gw, gh, pitch) of w x h frames at that cell size (0: 16); host only"""
    gw, gh, pitch = C.c_int(), C.c_int(), C.c_int()
    rc = lib().mars_hip_motion_grid(int(w), int(h), int(cell), C.byref(gw), C.byref(gh), C.byref(pitch))
    if rc != MARS_OK:
        raise MarsError(rc, "mars_hip_motion_grid")
    return gw.value, gh.value, pitch.value


def motion_opts(threshold=0, learn=0, learn_active=0, min_neighbors=0, stream_major=False, frame_diff=False, zones=None, flags=None):
    """mars_hip_motion_opts_t.  threshold: luma levels, 1 .. 255 (0: 8); learn / learn_active: the background's shifts, 1 .. 16 (0: 4 and 8);
    min_neighbors: 0 .. 8; zones: TILE_DTYPE records or rows of (x0, y0, x1, y1), at most MOTION_MAX_ZONES (the record keeps them alive);
    flags overrides stream_major and frame_diff"""
    o = MotionOpts(int(threshold), int(learn), int(learn_active), int(min_neighbors))
    o.flags = int(flags) if flags is not None else (MOTION_STREAM_MAJOR if stream_major else 0) | (MOTION_FRAME_DIFF if frame_diff else 0)
    if zones is not None and len(zones):
        z = np.asarray(zones)
        o._zones = np.ascontiguousarray(z if z.dtype == TILE_DTYPE else np.asarray(zones, dtype=np.int32).reshape(-1, 4)).reshape(-1).view(np.int32)
        o.n_zones, o.zones = o._zones.size // 4, o._zones.ctypes.data
    return o


class Motion:
    """mars_hip_motion_t: the background grids of `streams` camera streams of w x h frames (fmt: CAMERA_RGB / CAMERA_NV12) at one cell size,
    held on the device between calls"""

    def __init__(self, streams, w, h, fmt=CAMERA_RGB, cell=0):
        self.p = C.c_void_p()
        rc = lib().mars_hip_motion_create(int(streams), int(w), int(h), int(fmt), int(cell), C.byref(self.p))
        if rc != MARS_OK:
            self.p = None
            raise MarsError(rc, "mars_hip_motion_create")
        self.streams, self.w, self.h, self.fmt, self.cell = int(streams), int(w), int(h), int(fmt), int(cell) or 16
        self.gw, self.gh, self.pitch = motion_grid(w, h, cell)
        self.frame_bytes = self.w * self.h * 3 // (2 if self.fmt == CAMERA_NV12 else 1)
        self._frames = self._zones = 0

    def _arrays(self, n, nz):
        return (np.zeros((n, self.gh, self.pitch), dtype=np.uint32), np.zeros(n, dtype=MOTION_STATS_DTYPE), np.zeros((n, nz), dtype=np.int32))

    def frames(self, frames, opts=None, **kw):
        """mars_yolo_motion_frames: frames (uint8, [n] frames in host memory) go through the detector, on the GPU -> (maps uint32
        [n][gh][pitch], MOTION_STATS_DTYPE [n], zone counts int32 [n][n_zones]); waits.  opts = motion_opts(...), or its keywords"""
        o = opts if opts is not None else motion_opts(**kw)
        a = np.ascontiguousarray(frames, dtype=np.uint8).reshape(-1)
        if a.size == 0 or a.size % self.frame_bytes:
            raise ValueError("frames of %d x %d are %d bytes each, got %d" % (self.w, self.h, self.frame_bytes, a.size))
        n = a.size // self.frame_bytes
        maps, stats, zc = self._arrays(n, o.n_zones)
        rc = lib().mars_yolo_motion_frames(self.p, a.ctypes.data, n, C.byref(o), maps.ctypes.data, stats.ctypes.data, zc.ctypes.data if o.n_zones else None)
        if rc != MARS_OK:
            raise MarsError(rc, "mars_yolo_motion_frames")
        self._frames, self._zones = n, o.n_zones
        return maps, stats, zc

    def device(self, frames_dev, n_frames, opts=None, **kw):
        """mars_hip_motion_device: n_frames frames at device address frames_dev; enqueues only"""
        o = opts if opts is not None else motion_opts(**kw)
        rc = lib().mars_hip_motion_device(self.p, C.c_void_p(frames_dev), int(n_frames), C.byref(o))
        if rc != MARS_OK:
            raise MarsError(rc, "mars_hip_motion_device")
        self._frames, self._zones = int(n_frames), o.n_zones

    def results(self):
        """-> (maps, stats, zone counts) of the last device() (mars_hip_motion_results); waits"""
        maps, stats, zc = self._arrays(self._frames, self._zones)
        rc = lib().mars_hip_motion_results(self.p, maps.ctypes.data if self._frames else None, stats.ctypes.data if self._frames else None,
                                           zc.ctypes.data if zc.size else None)
        if rc != MARS_OK:
            raise MarsError(rc, "mars_hip_motion_results")
        return maps, stats, zc

    def boxes(self, boxes, frame_of_box, expand=0.0):
        """mars_yolo_motion_boxes: DET_DTYPE records, box i in frame frame_of_box[i] of the last call -> MOTION_DET_DTYPE [n]; waits"""
        b = np.ascontiguousarray(boxes, dtype=DET_DTYPE).reshape(-1)
        fo = np.ascontiguousarray(frame_of_box, dtype=np.int32).reshape(-1)
        if fo.size != b.size:
            raise ValueError("one frame index per box")
        out = np.zeros(b.size, dtype=MOTION_DET_DTYPE)
        rc = lib().mars_yolo_motion_boxes(self.p, b.ctypes.data if b.size else None, fo.ctypes.data if b.size else None, b.size, float(expand),
                                          out.ctypes.data if b.size else None)
        if rc != MARS_OK:
            raise MarsError(rc, "mars_yolo_motion_boxes")
        return out

    def read(self, stream):
        """-> (bg uint16 [gh][gw], initialised) of that stream (mars_hip_motion_read); waits"""
        bg = np.zeros((self.gh, self.gw), dtype=np.uint16)
        init = C.c_int()
        rc = lib().mars_hip_motion_read(self.p, int(stream), bg.ctypes.data, C.byref(init))
        if rc != MARS_OK:
            raise MarsError(rc, "mars_hip_motion_read")
        return bg, bool(init.value)

    def reset(self, stream=-1):
        rc = lib().mars_hip_motion_reset(self.p, int(stream))
        if rc != MARS_OK:
            raise MarsError(rc, "mars_hip_motion_reset")

    def ms(self):
        """device time (ms) of the last device() call's kernels (mars_hip_motion_ms); < 0: not available"""
        return float(lib().mars_hip_motion_ms(self.p))

    def close(self):
        if self.p:
            lib().mars_hip_motion_free(self.p)
            self.p = None


def event_rules(lines=(), zones=()):
    """mars_hip_event_rules_t.  lines: rows of (ax, ay, bx, by), directed A -> B; zones: polygons, each a list of 3 .. EVENTS_MAX_VERTS
    (x, y) vertices, or a pair (vertices, dwell steps).  Integer pixels in [-32768, 32768].  Counts beyond what the record holds raise
    ValueError; everything else is left to the library's checks"""
    lines, zones = list(lines), list(zones)
    if len(lines) > EVENTS_MAX_LINES or len(zones) > EVENTS_MAX_ZONES:
        raise ValueError("at most %d lines and %d zones" % (EVENTS_MAX_LINES, EVENTS_MAX_ZONES))
    r = EventRules()
    r.n_lines, r.n_zones = len(lines), len(zones)
    for k, ln in enumerate(lines):
        r.lines[k] = EventLine(*[int(v) for v in ln])
    for k, z in enumerate(zones):
        verts, dwell = (z[0], z[1]) if len(z) == 2 and not np.isscalar(z[0]) and np.isscalar(z[1]) else (z, 0)
        if len(verts) > EVENTS_MAX_VERTS:
            raise ValueError("at most %d vertices" % EVENTS_MAX_VERTS)
        r.zones[k].n, r.zones[k].dwell = len(verts), int(dwell)
        for v, (x, y) in enumerate(verts):
            r.zones[k].x[v], r.zones[k].y[v] = int(x), int(y)
    return r


def event_opts(max_gap=0, min_hits=0, stream_major=False, anchor_bottom=False, flags=None):
    """mars_hip_events_opts_t; zero means default everywhere (max_gap 30, min_hits 1, the anchor is the box centre).  flags overrides
    stream_major and anchor_bottom"""
    f = int(flags) if flags is not None else (EVENTS_STREAM_MAJOR if stream_major else 0) | (EVENTS_ANCHOR_BOTTOM if anchor_bottom else 0)
    return EventsOpts(int(max_gap), int(min_hits), f)


class Events:
    """mars_hip_events_t: per camera stream the rules (lines and zones), a table of TRACK_SLOTS slots, a step counter and running totals,
    held on the device between calls"""

    def __init__(self, streams):
        self.streams = int(streams)
        self.p = C.c_void_p()
        rc = lib().mars_hip_events_create(self.streams, C.byref(self.p))
        if rc != MARS_OK:
            self.p = C.c_void_p()
            raise MarsError(rc, "mars_hip_events_create")

    def set_rules(self, rules, stream=-1):
        """the rules of one stream (-1: of all) are replaced and that stream is reset (mars_hip_events_set_rules); waits"""
        rc = lib().mars_hip_events_set_rules(self.p, int(stream), C.byref(rules))
        if rc != MARS_OK:
            raise MarsError(rc, "mars_hip_events_set_rules")

    def reset(self, stream=-1):
        """that stream's table empty, its step and totals zero, its rules kept (-1: all streams); waits"""
        rc = lib().mars_hip_events_reset(self.p, int(stream))
        if rc != MARS_OK:
            raise MarsError(rc, "mars_hip_events_reset")

    def read(self, stream):
        """-> (line totals int64 [EVENTS_MAX_LINES][in, out], zone totals int64 [EVENTS_MAX_ZONES][entered, exited, dwelled, lost], counters
        int64 [first, expired, overflow, dropped, duplicates], used slots, step) of one stream (mars_hip_events_read); waits"""
        lt = np.zeros((EVENTS_MAX_LINES, 2), dtype=np.int64)
        zt = np.zeros((EVENTS_MAX_ZONES, 4), dtype=np.int64)
        cnt = np.zeros(5, dtype=np.int64)
        used, step = C.c_int(0), C.c_int(0)
        rc = lib().mars_hip_events_read(self.p, int(stream), lt.ctypes.data, zt.ctypes.data, cnt.ctypes.data, C.byref(used), C.byref(step))
        if rc != MARS_OK:
            raise MarsError(rc, "mars_hip_events_read")
        return lt, zt, cnt, used.value, step.value

    def read_slots(self, stream):
        """-> EVENT_SLOT_DTYPE [TRACK_SLOTS], the table of one stream in canonical form (mars_hip_events_read_slots); waits"""
        slots = np.zeros(TRACK_SLOTS, dtype=EVENT_SLOT_DTYPE)
        rc = lib().mars_hip_events_read_slots(self.p, int(stream), slots.ctypes.data)
        if rc != MARS_OK:
            raise MarsError(rc, "mars_hip_events_read_slots")
        return slots

    def ms(self):
        """device time (ms) of the last call's kernel (mars_hip_events_ms); < 0: not available"""
        return float(lib().mars_hip_events_ms(self.p))

    def close(self):
        if self.p:
            lib().mars_hip_events_free(self.p)
            self.p = C.c_void_p()


def _event_arrays(frames, max_det):
    return (np.zeros((frames, max_det), dtype=EVENT_DTYPE), np.zeros((frames, EVENTS_MAX_LINES, 2), dtype=np.int32),
            np.zeros((frames, EVENTS_MAX_ZONES, 4), dtype=np.int32))


def event_lists(events, dets, tracks, counts, opts=None):
    """mars_yolo_event_lists: dets = DET_DTYPE [frames][max_det], tracks = TRACK_DTYPE of that shape, counts = [frames] -> (EVENT_DTYPE
    [frames][max_det], line counts int32 [frames][EVENTS_MAX_LINES][in, out], zone counts int32 [frames][EVENTS_MAX_ZONES][inside, entered,
    exited, dwelled]), on the GPU; the object's tables move on by these frames"""
    d = np.ascontiguousarray(dets, dtype=DET_DTYPE)
    t = np.ascontiguousarray(tracks, dtype=TRACK_DTYPE)
    c = np.ascontiguousarray(counts, dtype=np.int32).reshape(-1)
    if d.ndim != 2 or d.shape[0] != c.size or t.shape != d.shape:
        raise ValueError("dets and tracks must be [frames][max_det] with one count per frame")
    o = opts if opts is not None else event_opts()
    rec, lc, zc = _event_arrays(d.shape[0], d.shape[1])
    rc = lib().mars_yolo_event_lists(events.p, d.ctypes.data, t.ctypes.data, c.ctypes.data, d.shape[0], d.shape[1], C.byref(o), rec.ctypes.data,
                                     lc.ctypes.data, zc.ctypes.data)
    if rc != MARS_OK:
        raise MarsError(rc, "mars_yolo_event_lists")
    return rec, lc, zc


def shot_opts(max_gap=0, min_hits=0, min_mean=0, max_mean=0, min_sharp=0, src=None, stream_major=False, keep_aspect=False, inside=False,
              flags=None):
    """mars_hip_shot_opts_t; zero means default everywhere (max_gap 30, min_hits 1, no mean window, stretch geometry).  src = (w, h) of
    the frames, needed by inside only.  flags overrides stream_major, keep_aspect and inside"""
    f = int(flags) if flags is not None else ((SHOT_STREAM_MAJOR if stream_major else 0) | (SHOT_KEEP_ASPECT if keep_aspect else 0) |
                                              (SHOT_INSIDE if inside else 0))
    w, h = src if src is not None else (0, 0)
    return ShotOpts(int(max_gap), int(min_hits), int(min_mean), int(max_mean), int(min_sharp), int(w), int(h), f)


class Shots:
    """mars_hip_shots_t: per camera stream a table of `slots` entries with the best crop of every live track, its pixels in a plane of
    tw x th x 3 int8 crops, a step counter and counters, held on the device between calls"""

    def __init__(self, streams, slots, tw, th, nhwc=True):
        self.streams, self.slots, self.tw, self.th, self.nhwc = int(streams), int(slots), int(tw), int(th), bool(nhwc)
        self.p = C.c_void_p()
        rc = lib().mars_hip_shots_create(self.streams, self.slots, self.tw, self.th, int(self.nhwc), C.byref(self.p))
        if rc != MARS_OK:
            self.p = C.c_void_p()
            raise MarsError(rc, "mars_hip_shots_create")

    def reset(self, stream=-1):
        """that stream's table empty, its step and counters zero (-1: all streams); waits"""
        rc = lib().mars_hip_shots_reset(self.p, int(stream))
        if rc != MARS_OK:
            raise MarsError(rc, "mars_hip_shots_reset")

    def flush(self, stream=-1):
        """the end of a stream: every LIVE slot becomes DONE and adds to `finished` (mars_hip_shots_flush); waits"""
        rc = lib().mars_hip_shots_flush(self.p, int(stream))
        if rc != MARS_OK:
            raise MarsError(rc, "mars_hip_shots_flush")

    def read(self, stream):
        """-> (counters int64 [finished, lost, dropped, overflow, duplicates, taken], LIVE slots, DONE slots, step) of one stream
        (mars_hip_shots_read); waits"""
        cnt = np.zeros(6, dtype=np.int64)
        live, done, step = C.c_int(0), C.c_int(0), C.c_int(0)
        rc = lib().mars_hip_shots_read(self.p, int(stream), cnt.ctypes.data, C.byref(live), C.byref(done), C.byref(step))
        if rc != MARS_OK:
            raise MarsError(rc, "mars_hip_shots_read")
        return cnt, live.value, done.value, step.value

    def read_slots(self, stream):
        """-> SHOT_SLOT_DTYPE [slots], the table of one stream in canonical form (mars_hip_shots_read_slots); waits"""
        slots = np.zeros(self.slots, dtype=SHOT_SLOT_DTYPE)
        rc = lib().mars_hip_shots_read_slots(self.p, int(stream), slots.ctypes.data)
        if rc != MARS_OK:
            raise MarsError(rc, "mars_hip_shots_read_slots")
        return slots

    def pixels(self, stream, slot):
        """-> uint8 [th][tw][3], the picture of a LIVE or DONE slot (mars_hip_shots_read_pixels); waits"""
        rgb = np.zeros((self.th, self.tw, 3), dtype=np.uint8)
        rc = lib().mars_hip_shots_read_pixels(self.p, int(stream), int(slot), rgb.ctypes.data)
        if rc != MARS_OK:
            raise MarsError(rc, "mars_hip_shots_read_pixels")
        return rgb

    def collect(self, stream, cap):
        """-> (SHOT_SLOT_DTYPE [k], uint8 [k][th][tw][3], DONE slots there were): the first k = min(cap, DONE) finished shots by ascending
        slot with their pictures; those k slots are FREE afterwards (mars_hip_shots_collect); waits"""
        cap = int(cap)
        slots = np.zeros(max(cap, 1), dtype=SHOT_SLOT_DTYPE)
        rgb = np.zeros((max(cap, 1), self.th, self.tw, 3), dtype=np.uint8)
        n = C.c_int(0)
        rc = lib().mars_hip_shots_collect(self.p, int(stream), slots.ctypes.data, rgb.ctypes.data, cap, C.byref(n))
        if rc != MARS_OK:
            raise MarsError(rc, "mars_hip_shots_collect")
        k = max(min(cap, n.value), 0)
        return slots[:k].copy(), rgb[:k].copy(), n.value

    def ms(self):
        """device time (ms) of the last call's kernels (mars_hip_shots_ms); < 0: not available"""
        return float(lib().mars_hip_shots_ms(self.p))

    def close(self):
        if self.p:
            lib().mars_hip_shots_free(self.p)
            self.p = C.c_void_p()


def shot_lists(shots, crops, rois, confs, cls, tracks, frames, opts=None):
    """mars_yolo_shot_lists: crops = int8 [n][tw * th * 3] in the object's layout, rois = ROI_DTYPE [n], confs = float32 [n], cls = int32
    [n], tracks = TRACK_DTYPE [n], one entry per crop, over `frames` frames -> SHOT_DTYPE [n], on the GPU; the object's tables move on
    by these frames"""
    x = np.ascontiguousarray(crops, dtype=np.int8)
    r = np.ascontiguousarray(rois, dtype=ROI_DTYPE).reshape(-1)
    n = r.size
    cf = np.ascontiguousarray(confs, dtype=np.float32).reshape(-1)
    cl = np.ascontiguousarray(cls, dtype=np.int32).reshape(-1)
    t = np.ascontiguousarray(tracks, dtype=TRACK_DTYPE).reshape(-1)
    if x.size != n * shots.tw * shots.th * 3 or cf.size != n or cl.size != n or t.size != n:
        raise ValueError("one crop of tw * th * 3 bytes, one ROI, confidence, class and track per crop")
    o = opts if opts is not None else shot_opts()
    rec = np.zeros(n, dtype=SHOT_DTYPE)
    rc = lib().mars_yolo_shot_lists(shots.p, x.ctypes.data, r.ctypes.data, cf.ctypes.data, cl.ctypes.data, t.ctypes.data, n, int(frames),
                                    C.byref(o), rec.ctypes.data)
    if rc != MARS_OK:
        raise MarsError(rc, "mars_yolo_shot_lists")
    return rec


def cls_opts(output_index=0, tensor=0, top_k=0, scale=0.0, softmax=False):
    """mars_hip_cls_opts_t: pool graph output `output_index`, or TENSOR index `tensor` when > 0; zero means default everywhere"""
    return ClsOpts(int(output_index), int(tensor), int(top_k), float(scale), CLS_SOFTMAX if softmax else 0)


def classify_maps(maps, c, h, w, nhwc=True, scale=1.0, opts=None, want_sums=True):
    """mars_yolo_classify_maps: int8 maps, [n] dense maps of [h][w][c] (nhwc) or [c][h][w] -> (CLS_DTYPE entries [n][top_k], int32 sums
    [n][c] or None), on the GPU"""
    a = np.ascontiguousarray(maps).view(np.int8).reshape(-1)
    per = int(c) * int(h) * int(w)
    if per <= 0 or a.size % per or a.size == 0:
        raise ValueError("maps of %d x %d x %d are %d bytes each, got %d" % (c, h, w, per, a.size))
    o = opts if opts is not None else cls_opts()
    n, k = a.size // per, o.top_k if 0 < o.top_k <= CLS_MAX_TOPK else 1
    top = np.zeros((n, k), dtype=CLS_DTYPE)
    sums = np.zeros((n, int(c)), dtype=np.int32) if want_sums else None
    rc = lib().mars_yolo_classify_maps(a.ctypes.data, n, int(c), int(h), int(w), int(bool(nhwc)), float(scale), C.byref(o), top.ctypes.data,
                                       sums.ctypes.data if want_sums else None)
    if rc != MARS_OK:
        raise MarsError(rc, "mars_yolo_classify_maps")
    return top, sums


def embed_quantise(vectors, c):
    """mars_yolo_embed_quantise: int32 embeddings [n][c] -> (int8 q [n][c], int32 qq [n]; qq == 0 marks a null vector).  Host only"""
    v = np.ascontiguousarray(vectors, dtype=np.int32).reshape(-1)
    if int(c) <= 0 or v.size == 0 or v.size % int(c):
        raise ValueError("embeddings of %d values, got %d values" % (c, v.size))
    n = v.size // int(c)
    q = np.zeros((n, int(c)), dtype=np.int8)
    qq = np.zeros(n, dtype=np.int32)
    rc = lib().mars_yolo_embed_quantise(v.ctypes.data, n, int(c), q.ctypes.data, qq.ctypes.data)
    if rc != MARS_OK:
        raise MarsError(rc, "mars_yolo_embed_quantise")
    return q, qq


def match_opts(top_k=0, min_score=0.0):
    """mars_hip_match_opts_t; zero means default everywhere (top_k 1, no threshold)"""
    return MatchOpts(int(top_k), float(min_score), 0)


def match_chunk(rows):
    """mars_hip_match_chunk: gallery rows per workgroup of the match kernel for a gallery of `rows` rows"""
    return int(lib().mars_hip_match_chunk(int(rows)))


class Gallery:
    """mars_hip_gallery_t: enrolled embeddings of `channels` int32 values with an id each, quantised on the host, held on the device"""

    def __init__(self, channels, capacity):
        self.channels = int(channels)
        self.p = C.c_void_p()
        rc = lib().mars_hip_gallery_create(self.channels, int(capacity), C.byref(self.p))
        if rc != MARS_OK:
            self.p = C.c_void_p()
            raise MarsError(rc, "mars_hip_gallery_create")

    def add(self, vectors, ids):
        """int32 vectors [n][channels] with ids [n] (>= 0): all are appended or none"""
        v = np.ascontiguousarray(vectors, dtype=np.int32).reshape(-1)
        i = np.ascontiguousarray(ids, dtype=np.int32).reshape(-1)
        if i.size == 0 or v.size != i.size * self.channels:
            raise ValueError("%d ids need %d values, got %d" % (i.size, i.size * self.channels, v.size))
        rc = lib().mars_hip_gallery_add(self.p, v.ctypes.data, i.ctypes.data, int(i.size))
        if rc != MARS_OK:
            raise MarsError(rc, "mars_hip_gallery_add")

    def count(self):
        return int(lib().mars_hip_gallery_count(self.p))

    def clear(self):
        rc = lib().mars_hip_gallery_clear(self.p)
        if rc != MARS_OK:
            raise MarsError(rc, "mars_hip_gallery_clear")

    def close(self):
        if self.p:
            lib().mars_hip_gallery_free(self.p)
            self.p = C.c_void_p()


def match_vectors(gallery, vectors, opts=None, want_rows=True):
    """mars_yolo_match_vectors: int32 embeddings [n][channels] against the gallery -> (CLS_DTYPE entries [n][top_k] with cls = id, int32 row
    indices [n][top_k] or None), on the GPU"""
    v = np.ascontiguousarray(vectors, dtype=np.int32).reshape(-1)
    c = gallery.channels
    if v.size == 0 or v.size % c:
        raise ValueError("embeddings of %d values, got %d values" % (c, v.size))
    o = opts if opts is not None else match_opts()
    n, k = v.size // c, o.top_k if 0 < o.top_k <= CLS_MAX_TOPK else 1
    top = np.zeros((n, k), dtype=CLS_DTYPE)
    rows = np.zeros((n, k), dtype=np.int32) if want_rows else None
    rc = lib().mars_yolo_match_vectors(gallery.p, v.ctypes.data, n, C.byref(o), top.ctypes.data, rows.ctypes.data if want_rows else None)
    if rc != MARS_OK:
        raise MarsError(rc, "mars_yolo_match_vectors")
    return top, rows


def track_opts(min_conf=0.0, low_conf=0.0, iou_thresh=0.0, iou_thresh_low=0.0, max_miss=0, classes=None, any_class=False,
               carry_identity=False, stream_major=False):
    """mars_hip_track_opts_t; zero means default everywhere (min_conf 0.5, no second pass, IoU 0.3 / 0.5, max_miss 30, every class).
    classes = (first, count)"""
    first, count = classes if classes else (0, 0)
    flags = (TRACK_ANY_CLASS if any_class else 0) | (TRACK_CARRY_IDENTITY if carry_identity else 0) | (TRACK_STREAM_MAJOR if stream_major else 0)
    return TrackOpts(float(min_conf), float(low_conf), float(iou_thresh), float(iou_thresh_low), int(max_miss), int(first), int(count), flags)


def track_app_opts(app_thresh=0.0, app_min_iou=0.0, smooth=False):
    """mars_hip_track_app_opts_t; zero means default (cosine threshold 0.75, spatial gate 0.1, a matched slot takes the detection's
    embedding as it is); smooth: MARS_TRACK_APP_SMOOTH, the 3 : 1 blend"""
    return TrackAppOpts(float(app_thresh), float(app_min_iou), TRACK_APP_SMOOTH if smooth else 0)


class Tracker:
    """mars_hip_tracker_t: the track tables of `streams` camera streams, TRACK_SLOTS slots each, held on the device between calls;
    channels > 0: with an int8 embedding of that many channels per slot ("Appearance in tracking", mars_hip_tracker_create_app)"""

    def __init__(self, streams, channels=0):
        self.streams = int(streams)
        self.channels = int(channels)
        self.p = C.c_void_p()
        if self.channels:
            rc, what = lib().mars_hip_tracker_create_app(self.streams, self.channels, C.byref(self.p)), "mars_hip_tracker_create_app"
        else:
            rc, what = lib().mars_hip_tracker_create(self.streams, C.byref(self.p)), "mars_hip_tracker_create"
        if rc != MARS_OK:
            self.p = C.c_void_p()
            raise MarsError(rc, what)

    def read_embeddings(self, stream):
        """-> (int8 [live][channels], int32 [live]): the embeddings of the live tracks of one stream by ascending slot, aligned with read();
        ee == 0: the track has none.  Waits"""
        q = np.zeros((TRACK_SLOTS, max(self.channels, 1)), dtype=np.int8)
        ee = np.zeros(TRACK_SLOTS, dtype=np.int32)
        n = C.c_int(0)
        rc = lib().mars_hip_tracker_read_embeddings(self.p, int(stream), q.ctypes.data, ee.ctypes.data, TRACK_SLOTS, C.byref(n))
        if rc != MARS_OK:
            raise MarsError(rc, "mars_hip_tracker_read_embeddings")
        return q[:n.value].copy(), ee[:n.value].copy()

    def reset(self):
        """every table empty, the next id 1, the counters 0"""
        rc = lib().mars_hip_tracker_reset(self.p)
        if rc != MARS_OK:
            raise MarsError(rc, "mars_hip_tracker_reset")

    def read(self, stream):
        """-> (TRACK_STATE_DTYPE records of the live tracks of one stream by ascending slot, int64 [births, deaths, overflow, dropped]).  Waits"""
        states = np.zeros(TRACK_SLOTS, dtype=TRACK_STATE_DTYPE)
        n = C.c_int(0)
        counters = np.zeros(4, dtype=np.int64)
        rc = lib().mars_hip_tracker_read(self.p, int(stream), states.ctypes.data, TRACK_SLOTS, C.byref(n), counters.ctypes.data)
        if rc != MARS_OK:
            raise MarsError(rc, "mars_hip_tracker_read")
        return states[:n.value].copy(), counters

    def close(self):
        if self.p:
            lib().mars_hip_tracker_free(self.p)
            self.p = C.c_void_p()


def track_lists(tracker, dets, counts, opts=None, idents=None):
    """mars_yolo_track_lists: dets = DET_DTYPE [frames][max_det], counts = [frames], idents = None or CLS_DTYPE [frames][max_det] ->
    TRACK_DTYPE [frames][max_det], on the GPU; the tracker's tables move on by these frames"""
    d = np.ascontiguousarray(dets, dtype=DET_DTYPE)
    c = np.ascontiguousarray(counts, dtype=np.int32).reshape(-1)
    if d.ndim != 2 or d.shape[0] != c.size:
        raise ValueError("dets must be [frames][max_det] with one count per frame")
    i = None
    if idents is not None:
        i = np.ascontiguousarray(idents, dtype=CLS_DTYPE)
        if i.shape != d.shape:
            raise ValueError("idents must have the shape of dets")
    o = opts if opts is not None else track_opts()
    out = np.zeros(d.shape, dtype=TRACK_DTYPE)
    rc = lib().mars_yolo_track_lists(tracker.p, d.ctypes.data, c.ctypes.data, i.ctypes.data if i is not None else None, d.shape[0], d.shape[1],
                                     C.byref(o), out.ctypes.data)
    if rc != MARS_OK:
        raise MarsError(rc, "mars_yolo_track_lists")
    return out


def track_lists_app(tracker, dets, counts, vectors=None, emb_index=None, opts=None, app=None, idents=None):
    """mars_yolo_track_lists_app: track_lists on a Tracker(streams, channels) with embeddings: vectors = int32 [n_vectors][channels] or None,
    emb_index = int [frames][max_det], the row of vectors detection (f, i) uses (anything outside 0 .. n_vectors - 1: none)"""
    d = np.ascontiguousarray(dets, dtype=DET_DTYPE)
    c = np.ascontiguousarray(counts, dtype=np.int32).reshape(-1)
    if d.ndim != 2 or d.shape[0] != c.size:
        raise ValueError("dets must be [frames][max_det] with one count per frame")
    i = None
    if idents is not None:
        i = np.ascontiguousarray(idents, dtype=CLS_DTYPE)
        if i.shape != d.shape:
            raise ValueError("idents must have the shape of dets")
    v, nv, e = None, 0, None
    if vectors is not None and np.size(vectors):
        v = np.ascontiguousarray(vectors, dtype=np.int32).reshape(-1)
        if not tracker.channels or v.size % tracker.channels:
            raise ValueError("embeddings of %d values, got %d values" % (tracker.channels, v.size))
        nv = v.size // tracker.channels
    if emb_index is not None:
        e = np.ascontiguousarray(emb_index, dtype=np.int32)
        if e.shape != d.shape:
            raise ValueError("emb_index must have the shape of dets")
    o = opts if opts is not None else track_opts()
    a = app if app is not None else track_app_opts()
    out = np.zeros(d.shape, dtype=TRACK_DTYPE)
    rc = lib().mars_yolo_track_lists_app(tracker.p, d.ctypes.data, c.ctypes.data, i.ctypes.data if i is not None else None,
                                         v.ctypes.data if v is not None else None, nv, e.ctypes.data if e is not None else None, d.shape[0],
                                         d.shape[1], C.byref(o), C.byref(a), out.ctypes.data)
    if rc != MARS_OK:
        raise MarsError(rc, "mars_yolo_track_lists_app")
    return out


def track_cosine(q, qq, e, ee):
    """mars_yolo_track_cosine: the cosine of a detection's (q, qq) and a slot's (e, ee), int8 vectors of one length -> np.float32; host only"""
    a, b = np.ascontiguousarray(q, dtype=np.int8).reshape(-1), np.ascontiguousarray(e, dtype=np.int8).reshape(-1)
    if a.size != b.size:
        raise ValueError("two vectors of one length")
    out = C.c_float(0)
    rc = lib().mars_yolo_track_cosine(a.ctypes.data, int(qq), b.ctypes.data, int(ee), int(a.size), C.byref(out))
    if rc != MARS_OK:
        raise MarsError(rc, "mars_yolo_track_cosine")
    return np.float32(out.value)


def embed_blend(e, ee, q, qq):
    """mars_yolo_embed_blend: the MARS_TRACK_APP_SMOOTH update of a slot holding (e, ee) matched to a detection with (q, qq) ->
    (int8 [channels], ee); host only"""
    a, b = np.ascontiguousarray(e, dtype=np.int8).reshape(-1), np.ascontiguousarray(q, dtype=np.int8).reshape(-1)
    if a.size != b.size:
        raise ValueError("two vectors of one length")
    out = np.zeros(a.size, dtype=np.int8)
    oe = C.c_int(0)
    rc = lib().mars_yolo_embed_blend(a.ctypes.data, int(ee), b.ctypes.data, int(qq), int(a.size), out.ctypes.data, C.byref(oe))
    if rc != MARS_OK:
        raise MarsError(rc, "mars_yolo_embed_blend")
    return out, int(oe.value)


def track_cosine_matrix(track_q, track_ee, vectors):
    """mars_yolo_track_cosine_matrix, a test hook: int8 [nt][channels] and int32 [nt] standing where slots would, int32 vectors
    [nc][channels] -> float32 [nt][nc], the ungated cosines of the tracking kernel's own matrix routine (0 where a side has no embedding)"""
    tq = np.ascontiguousarray(track_q, dtype=np.int8)
    te = np.ascontiguousarray(track_ee, dtype=np.int32).reshape(-1)
    v = np.ascontiguousarray(vectors, dtype=np.int32)
    if tq.ndim != 2 or v.ndim != 2 or tq.shape[1] != v.shape[1] or tq.shape[0] != te.size:
        raise ValueError("track_q [nt][channels], track_ee [nt], vectors [nc][channels]")
    out = np.zeros((tq.shape[0], v.shape[0]), dtype=np.float32)
    rc = lib().mars_yolo_track_cosine_matrix(tq.ctypes.data, te.ctypes.data, v.ctypes.data, tq.shape[0], v.shape[0], tq.shape[1], out.ctypes.data)
    if rc != MARS_OK:
        raise MarsError(rc, "mars_yolo_track_cosine_matrix")
    return out


class DeviceBuffer:
    """bytes in HBM for the *_device calls (a stand-in for a capture card that writes there): hipMalloc + a blocking copy through the HIP runtime
    the library itself is linked against.  .ptr is the device address"""

    def __init__(self, data):
        a = np.ascontiguousarray(data, dtype=np.uint8).reshape(-1)
        lib()  # the runtime is loaded with the library
        self._hip = C.CDLL("libamdhip64.so", mode=os.RTLD_GLOBAL)
        p = C.c_void_p()
        if self._hip.hipMalloc(C.byref(p), C.c_size_t(max(a.size, 1))) != 0:
            raise MemoryError("hipMalloc of %d bytes" % a.size)
        self.ptr, self.size = p.value, a.size
        if self._hip.hipMemcpy(C.c_void_p(self.ptr), C.c_void_p(a.ctypes.data), C.c_size_t(a.size), 1) != 0:  # hipMemcpyHostToDevice
            self.free()
            raise RuntimeError("hipMemcpy to the device")

    def free(self):
        if self.ptr:
            self._hip.hipFree(C.c_void_p(self.ptr))
            self.ptr = None

    def __del__(self):
        try:
            self.free()
        except Exception:
            pass


SYNTH_HEADS = {"anchor": 0, "dfl": 1, "seg": 2, "pose": 3, "obb": 4}  # MARS_SYNTH_HEAD_*


def synth_model(width_x16=8, depth_x3=1, input_hw=640, float32=False, nchw_int8=False, seed=1, tiny=False, vary_scales=False, head="anchor"):
    """Bytes of a synthetic well-formed .mars graph (mars_synth_model; head="dfl": mars_synth_model_head with the anchor-free DFL
    Detect head, int8 only; head="seg": that head plus mask coefficients and prototypes, see seg_twin_tensors; head="pose": the DFL head
    plus keypoint tensors of 17 x 3 channels, see pose_twin_tensors; head="obb": the DFL head plus 1-channel angle tensors, see
    obb_twin_tensors)."""
    o = SynthOpts(width_x16, depth_x3, input_hw, int(float32), int(nchw_int8), seed, int(tiny), int(vary_scales))
    if head == "anchor":
        make = lib().mars_synth_model
    else:
        hd = SYNTH_HEADS[head]
        make = lambda opts, buf, cap: lib().mars_synth_model_head(opts, hd, buf, cap)  # noqa: E731
    n = make(C.byref(o), None, 0)
    if n == 0:
        raise ValueError("mars_synth_model rejected the options")
    buf = (C.c_uint8 * n)()
    assert make(C.byref(o), buf, n) == n
    return bytes(buf)


DESCRIBE_FULL = 2  # MARS_HIP_DESCRIBE_FULL


def describe_plan(file_bytes, flags=0):
    """the launch plan of a .mars file as a list of text lines (mars_hip_describe_plan; host only: works without a GPU).
    flags: 1 (MARS_HIP_LOAD_DEFER_WEIGHTS) plans from the descriptors alone, as a rank without the weight blob does; DESCRIBE_FULL (2) adds, behind
    " |", every field of each launch that the run path reads and each tensor's sizes, and lines that start with "+": the needed tensors the short
    form leaves out, and the plan's totals with the environment switches it was built under.  The short form is a prefix of the full one."""
    b = bytes(file_bytes)
    n = lib().mars_hip_describe_plan(b, len(b), flags, None, 0)
    if n == 0:
        raise ValueError("the loader rejects the file")
    buf = C.create_string_buffer(n + 1)
    lib().mars_hip_describe_plan(b, len(b), flags, buf, n + 1)
    return buf.value.decode().splitlines()


def find_yolo_heads(file_bytes):
    """anchor-based YOLOv5 Detect heads of a .mars file (mars_yolo_find_heads; host only: works without a GPU), by stride:
    a list of (tensor index, stride, classes).  ValueError if the loader rejects the file."""
    b = bytes(file_bytes)
    ti, st, nc = (C.c_int * 4)(), (C.c_int * 4)(), (C.c_int * 4)()
    n = lib().mars_yolo_find_heads(b, len(b), ti, st, nc, 4)
    if n < 0:
        raise ValueError("the loader rejects the file")
    return [(ti[k], st[k], nc[k]) for k in range(min(n, 4))]


def yolo_heads(heads=None, anchors=None, conf=0.25, thresh=0.45, src=None):
    """mars_yolo_heads_t.  heads: None (found on the loaded file) or a list of tensor indices / (tensor index, stride) pairs;
    anchors: None (YOLOv5 P3-P5 defaults) or [head][3][2] pixels; src = (w, h): boxes mapped back through the letterbox of
    frames of that size"""
    h = YoloHeads()
    for k, e in enumerate(heads or ()):
        ti, st = e if isinstance(e, (tuple, list)) else (e, 0)
        h.head_tensors[k], h.strides[k] = int(ti), int(st)
    h.n_heads = len(heads or ())
    if anchors is not None:
        for i, v in enumerate(np.asarray(anchors, dtype=np.float32).reshape(-1)):
            h.anchors[i] = float(v)
    h.conf_thresh, h.nms_thresh = conf, thresh
    if src is not None:
        h.src_w, h.src_h = int(src[0]), int(src[1])
    return h


def find_yolo_dfl_heads(file_bytes):
    """anchor-free DFL heads of a .mars file (mars_yolo_find_dfl_heads; host only: works without a GPU), by stride:
    ([(box tensor index, class tensor index, stride)], classes, reg_max) -- classes and reg_max of the first head, 0 if there is none.
    ValueError if the loader rejects the file."""
    b = bytes(file_bytes)
    bt, ct, st, nc, rm = ((C.c_int * 4)() for _ in range(5))
    n = lib().mars_yolo_find_dfl_heads(b, len(b), bt, ct, st, nc, rm, 4)
    if n < 0:
        raise ValueError("the loader rejects the file")
    return [(bt[k], ct[k], st[k]) for k in range(min(n, 4))], nc[0] if n else 0, rm[0] if n else 0


def yolo_dfl_heads(heads=None, reg_max=0, box_scales=None, cls_scales=None, conf=0.25, thresh=0.45, src=None):
    """mars_yolo_dfl_heads_t.  heads: None (found on the loaded file) or a list of (box tensor, class tensor[, stride]); box_scales /
    cls_scales: None (the tensors' own), one number for every head or a list; src = (w, h): boxes mapped back through the letterbox
    of frames of that size"""
    h = YoloDflHeads()
    for k, e in enumerate(heads or ()):
        h.box_tensors[k], h.cls_tensors[k] = int(e[0]), int(e[1])
        h.strides[k] = int(e[2]) if len(e) > 2 else 0
    h.n_heads = len(heads or ())
    h.reg_max = int(reg_max)
    for dst, v in ((h.box_scales, box_scales), (h.cls_scales, cls_scales)):
        if v is not None:
            for k, x in enumerate(v if isinstance(v, (tuple, list)) else [v] * 4):
                dst[k] = float(x)
    h.conf_thresh, h.nms_thresh = conf, thresh
    if src is not None:
        h.src_w, h.src_h = int(src[0]), int(src[1])
    return h


def seg_twin_tensors(file_bytes):
    """the mask tensors of a synth_model(head="seg") file, found by the names the writer gives them (host only):
    ([coefficient tensor index per head, by stride], prototype tensor index).  KeyError if the file has no such tensors."""
    b = bytes(file_bytes)
    hdr = MarsHeader.from_buffer_copy(b[:C.sizeof(MarsHeader)])
    names = {}
    for i in range(hdr.num_tensors):
        o = 76 + 124 * i
        names[b[o + 4:o + 64].split(b"\0")[0].decode()] = i
    return [names["seg.coef%d" % k] for k in range(3)], names["seg.proto"]


def seg_opts(coefs, proto, coef_scales=None, proto_scale=0.0, logit_min=0.0, min_conf=0.0, max_per_frame=0):
    """mars_hip_seg_opts_t.  coefs: the coefficient tensor index of every DFL head, in the heads' order; proto: the prototype tensor index;
    coef_scales: None (the tensors' own), one number for every head or a list"""
    o = SegOpts()
    for k, t in enumerate(coefs):
        o.coef_tensors[k] = int(t)
    o.proto_tensor = int(proto)
    if coef_scales is not None:
        for k, x in enumerate(coef_scales if isinstance(coef_scales, (tuple, list)) else [coef_scales] * 4):
            o.coef_scales[k] = float(x)
    o.proto_scale, o.logit_min, o.min_conf, o.max_per_frame = float(proto_scale), float(logit_min), float(min_conf), int(max_per_frame)
    return o


def masks(coefs, proto, boxes, in_w, in_h, s, logit_min=0.0):
    """mars_yolo_masks: coefs int8 [n][nm] (one row per box), proto int8 [nm][ph][pw], boxes DET_DTYPE [n] in pixels of an in_w x in_h
    input -> (records MASK_DTYPE [n], words uint32 [n][ph][pitch]); host arrays in and out, runs on the GPU"""
    a = np.ascontiguousarray(coefs, dtype=np.int8)
    pr = np.ascontiguousarray(proto, dtype=np.int8)
    bx = np.ascontiguousarray(boxes, dtype=DET_DTYPE)
    nm, ph, pw = pr.shape
    n = len(bx)
    assert a.shape == (n, nm) or (n == 0 and a.size == 0)
    recs = np.zeros(n, dtype=MASK_DTYPE)
    words = np.zeros((n, ph, (pw + 31) // 32), dtype=np.uint32)
    rc = lib().mars_yolo_masks(a.ctypes.data, n, nm, pr.ctypes.data, ph, pw, bx.ctypes.data, int(in_w), int(in_h), float(s), float(logit_min),
                               recs.ctypes.data, words.ctypes.data)
    if rc != 0:
        raise ValueError("mars_yolo_masks refused its arguments or failed (%d)" % rc)
    return recs, words


def mask_native_opts(out_w=0, out_h=0, flags=0):
    """mars_hip_mask_native_opts_t: 0 / 0 = the frame the DFL options map into (src), otherwise the graph input"""
    o = MaskNativeOpts()
    o.out_w, o.out_h, o.flags = int(out_w), int(out_h), int(flags)
    return o


def mask_geom(in_w, in_h, out_w, out_h, nw=None, nh=None, px=0, py=0, base_w=None, base_h=None):
    """mars_mask_geom_t: the letterboxed content nw x nh at (px, py) inside the in_w x in_h graph input (default: all of it), the grid the
    boxes are in (default: the graph input) and the output grid"""
    g = MaskGeom()
    g.in_w, g.in_h, g.out_w, g.out_h, g.px, g.py = int(in_w), int(in_h), int(out_w), int(out_h), int(px), int(py)
    g.nw, g.nh = int(in_w if nw is None else nw), int(in_h if nh is None else nh)
    g.base_w, g.base_h = int(in_w if base_w is None else base_w), int(in_h if base_h is None else base_h)
    return g


def mask_taps(out_n, in_n, n_content, pad, P):
    """mars_yolo_mask_taps (host only): the tap table of one axis -> (ia, ib, w1) int32 [out_n]; ValueError where it refuses"""
    n = max(int(out_n), 0)
    ia, ib, w1 = (np.zeros(n, dtype=np.int32) for _ in range(3))
    if lib().mars_yolo_mask_taps(int(out_n), int(in_n), int(n_content), int(pad), int(P), ia.ctypes.data, ib.ctypes.data, w1.ctypes.data) != 0:
        raise ValueError("mars_yolo_mask_taps refused its arguments")
    return ia, ib, w1


def masks_native(coefs, proto, boxes, geom, s, logit_min=0.0):
    """mars_yolo_masks_native: as masks(), the boxes in pixels of geom's base grid, geom a mask_geom() -> (records MASK_DTYPE [n], words uint32
    [n][out_h][pitch]); host arrays in and out, runs on the GPU"""
    a = np.ascontiguousarray(coefs, dtype=np.int8)
    pr = np.ascontiguousarray(proto, dtype=np.int8)
    bx = np.ascontiguousarray(boxes, dtype=DET_DTYPE)
    nm, ph, pw = pr.shape
    n = len(bx)
    assert a.shape == (n, nm) or (n == 0 and a.size == 0)
    recs = np.zeros(n, dtype=MASK_DTYPE)
    words = np.zeros((n, max(geom.out_h, 0), (max(geom.out_w, 0) + 31) // 32), dtype=np.uint32)
    rc = lib().mars_yolo_masks_native(a.ctypes.data, n, nm, pr.ctypes.data, ph, pw, bx.ctypes.data, C.byref(geom), float(s), float(logit_min),
                                      recs.ctypes.data, words.ctypes.data)
    if rc != 0:
        raise ValueError("mars_yolo_masks_native refused its arguments or failed (%d)" % rc)
    return recs, words


def unpack_masks(words, pw):
    """uint32 [..., PH, pitch] mask words -> bool [..., PH, pw]: pixel x is bit x & 31 of word x >> 5"""
    w = np.ascontiguousarray(words, dtype="<u4")
    bits = np.unpackbits(w.view(np.uint8).reshape(w.shape[:-1] + (w.shape[-1] * 4,)), axis=-1, bitorder="little")
    return bits[..., :pw].astype(bool)


def pose_twin_tensors(file_bytes):
    """the keypoint tensors of a synth_model(head="pose") file, found by the names the writer gives them (host only): the tensor index per
    head, by stride.  KeyError if the file has no such tensors."""
    b = bytes(file_bytes)
    hdr = MarsHeader.from_buffer_copy(b[:C.sizeof(MarsHeader)])
    names = {}
    for i in range(hdr.num_tensors):
        o = 76 + 124 * i
        names[b[o + 4:o + 64].split(b"\0")[0].decode()] = i
    return [names["pose.kpt%d" % k] for k in range(3)]


def pose_opts(kpts, num_kpt=17, kpt_dim=0, kpt_scales=None, min_conf=0.0, max_per_frame=0):
    """mars_hip_pose_opts_t.  kpts: the keypoint tensor index of every DFL head, in the heads' order; num_kpt, kpt_dim: K and D (0: 3);
    kpt_scales: None (the tensors' own), one number for every head or a list"""
    o = PoseOpts()
    for k, t in enumerate(kpts):
        o.kpt_tensors[k] = int(t)
    o.num_kpt, o.kpt_dim = int(num_kpt), int(kpt_dim)
    if kpt_scales is not None:
        for k, x in enumerate(kpt_scales if isinstance(kpt_scales, (tuple, list)) else [kpt_scales] * 4):
            o.kpt_scales[k] = float(x)
    o.min_conf, o.max_per_frame = float(min_conf), int(max_per_frame)
    return o


def keypoints(rows, K, D, gx, gy, stride, s):
    """mars_yolo_keypoints: rows int8 [n][K * D] (one row per detection), gx, gy, stride int [n] (every row's cell and stride), s the
    keypoint scale -> KPT_DTYPE [n][K]; host arrays in and out, runs on the GPU"""
    a = np.ascontiguousarray(rows, dtype=np.int8)
    n = len(a)
    g = [np.ascontiguousarray(v, dtype=np.int32) for v in (gx, gy, stride)]
    assert (a.shape == (n, K * D) or (n == 0 and a.size == 0)) and all(v.shape == (n,) for v in g)
    kp = np.zeros((n, K), dtype=KPT_DTYPE)
    rc = lib().mars_yolo_keypoints(a.ctypes.data, n, int(K), int(D), g[0].ctypes.data, g[1].ctypes.data, g[2].ctypes.data, float(s), kp.ctypes.data)
    if rc != 0:
        raise ValueError("mars_yolo_keypoints refused its arguments or failed (%d)" % rc)
    return kp


def obb_twin_tensors(file_bytes):
    """the angle tensors of a synth_model(head="obb") file, found by the names the writer gives them (host only): the tensor index per
    head, by stride.  KeyError if the file has no such tensors."""
    b = bytes(file_bytes)
    hdr = MarsHeader.from_buffer_copy(b[:C.sizeof(MarsHeader)])
    names = {}
    for i in range(hdr.num_tensors):
        o = 76 + 124 * i
        names[b[o + 4:o + 64].split(b"\0")[0].decode()] = i
    return [names["obb.ang%d" % k] for k in range(3)]


def obb_opts(angles, angle_scales=None, agnostic=False, flags=0):
    """mars_hip_obb_opts_t.  angles: the angle tensor index of every DFL head, in the heads' order; angle_scales: None (the tensors' own),
    one number for every head or a list; agnostic: MARS_OBB_AGNOSTIC; flags: further bits, as given"""
    o = ObbOpts()
    for k, t in enumerate(angles):
        o.angle_tensors[k] = int(t)
    if angle_scales is not None:
        for k, x in enumerate(angle_scales if isinstance(angle_scales, (tuple, list)) else [angle_scales] * 4):
            o.angle_scales[k] = float(x)
    o.flags = int(flags) | (OBB_AGNOSTIC if agnostic else 0)
    return o


def obb_nms(boxes, thresh=0.45, agnostic=False, flags=0):
    """mars_yolo_obb_nms: OBB_DTYPE [n] -> the kept boxes in order (confidence descending, position ascending; ProbIoU suppression); host
    arrays in and out, runs on the GPU"""
    a = np.array(boxes, dtype=OBB_DTYPE, copy=True).reshape(-1)
    n = lib().mars_yolo_obb_nms(a.ctypes.data, len(a), float(thresh), int(flags) | (OBB_AGNOSTIC if agnostic else 0))
    if n < 0:
        raise ValueError("mars_yolo_obb_nms refused its arguments or failed (%d)" % n)
    return a[:n]


def obb_corners(boxes):
    """mars_yolo_obb_corners of every box: OBB_DTYPE [n] -> float32 [n][4][2] (host only)"""
    a = np.ascontiguousarray(np.atleast_1d(boxes), dtype=OBB_DTYPE)
    out = np.zeros((len(a), 4, 2), dtype=np.float32)
    for i in range(len(a)):
        lib().mars_yolo_obb_corners(a[i:i + 1].ctypes.data, out[i].ctypes.data)
    return out


def compile_onnx(onnx_bytes, float32=False, nhwc=False, verbose=False):
    """ONNX model bytes -> .mars file bytes (mars_compile_onnx; host-only, needs no GPU)."""
    o = CompileOpts(int(float32), int(nhwc), int(verbose))
    n = lib().mars_compile_onnx(onnx_bytes, len(onnx_bytes), C.byref(o), None, 0)
    if n == 0:
        raise ValueError(lib().mars_compile_last_error().decode())
    buf = C.create_string_buffer(n)
    assert lib().mars_compile_onnx(onnx_bytes, len(onnx_bytes), C.byref(o), buf, n) == n
    return buf.raw


def nna_init():
    rc = lib().nna_init()
    if rc != NNA_SUCCESS:
        raise RuntimeError("nna_init failed (%d): no usable MI355X; this library has no CPU path" % rc)


class Model:
    """mars_load_memory / mars_run / mars_free with numpy views of the pinned I/O staging."""

    def __init__(self, file_bytes, batch=1, fusion=None, flags=0):
        L = lib()
        self._bytes = np.frombuffer(bytes(file_bytes), dtype=np.uint8).copy()
        self.p = C.POINTER(MarsModel)()
        self._segn_max = 16  # slots per frame of the last detect_seg_native_device (before one, the C call refuses the fetch)
        rc = L.mars_hip_load_memory_ex(self._bytes.ctypes.data, self._bytes.size, flags, C.byref(self.p))
        if rc != MARS_OK:
            self.p = None
            raise MarsError(rc, "mars_load_memory")
        if fusion is not None:
            self.set_fusion(fusion)
        if batch != 1:
            self.set_batch(batch)

    # -- reference API
    @property
    def header(self):
        return self.p.contents.header

    def tensor_desc(self, idx):
        return self.p.contents.tensors[idx].desc

    def input(self, i=0):
        return lib().mars_get_input(self.p, i)

    def output(self, i=0):
        return lib().mars_get_output(self.p, i)

    def _view(self, rt, tid):
        # batch * frame bytes by shape; alloc_size is larger for a single frame (the reference's working-buffer size)
        t = rt.contents
        n = lib().mars_hip_tensor_frame_bytes(self.p, tid) * self.batch
        return np.ctypeslib.as_array(C.cast(t.vaddr, C.POINTER(C.c_uint8)), shape=(n,))

    def input_view(self, i=0):
        """uint8 view [batch, frame_bytes] of mars_get_input(i)->vaddr."""
        return self._view(self.input(i), self.header.input_tensor_ids[i]).reshape(self.batch, -1)

    def output_view(self, i=0):
        return self._view(self.output(i), self.header.output_tensor_ids[i]).reshape(self.batch, -1)

    def run(self):
        rc = lib().mars_run(self.p)
        if rc != MARS_OK:
            raise MarsError(rc, "mars_run")

    # -- extensions
    @property
    def batch(self):
        return lib().mars_hip_get_batch(self.p)

    def set_batch(self, n):
        rc = lib().mars_hip_set_batch(self.p, n)
        if rc != MARS_OK:
            raise MarsError(rc, "mars_hip_set_batch")

    def set_fusion(self, level):
        rc = lib().mars_hip_set_fusion(self.p, level)
        if rc != MARS_OK:
            raise MarsError(rc, "mars_hip_set_fusion")

    def upload(self):
        rc = lib().mars_hip_upload_inputs(self.p)
        if rc != MARS_OK:
            raise MarsError(rc, "upload")

    def run_device(self, sync=True):
        rc = (lib().mars_hip_run_device if sync else lib().mars_hip_run_device_async)(self.p)
        if rc != MARS_OK:
            raise MarsError(rc, "run_device")

    def download(self):
        rc = lib().mars_hip_download_outputs(self.p)
        if rc != MARS_OK:
            raise MarsError(rc, "download")

    def read_tensor(self, idx, frame=0, nbytes=None):
        if nbytes is None:
            d = self.tensor_desc(idx)
            n = 1
            for k in range(d.ndims):
                n *= max(d.shape[k], 0)
            nbytes = n * (4 if d.dtype in (0, 1) else 2 if d.dtype == 2 else 1)
        out = np.zeros(nbytes, dtype=np.uint8)
        rc = lib().mars_hip_read_tensor(self.p, idx, frame, out.ctypes.data, nbytes)
        if rc != MARS_OK:
            raise MarsError(rc, "read_tensor %d" % idx)
        return out

    def set_profiling(self, on):
        lib().mars_hip_set_profiling(self.p, int(on))

    def preprocess(self, rgb_frames, first_frame=0, input_index=0):
        """uint8 RGB frames [n][h][w][3] -> letterboxed int8 frames of the graph input, in HBM"""
        a = np.ascontiguousarray(rgb_frames, dtype=np.uint8)
        n, h, w = a.shape[:3]
        rc = lib().mars_hip_preprocess(self.p, input_index, a.ctypes.data, w, h, first_frame, n)
        if rc != MARS_OK:
            raise MarsError(rc, "mars_hip_preprocess")

    def preprocess_nv12(self, nv12_frames, w, h, flags=0, first_frame=0, input_index=0):
        """NV12 frames [n][w * h * 3 / 2] -> letterboxed int8 frames of the graph input, in HBM (mars_hip_preprocess_nv12)"""
        a = _nv12_frames(nv12_frames, w, h, True)
        n = a.shape[0] if a.ndim > 1 else 1
        rc = lib().mars_hip_preprocess_nv12(self.p, input_index, a.ctypes.data, int(w), int(h), int(flags), first_frame, n)
        if rc != MARS_OK:
            raise MarsError(rc, "mars_hip_preprocess_nv12")

    def preprocess_device(self, dev_ptr, w, h, frames, first_frame=0, input_index=0):
        """mars_hip_preprocess_device: RGB frames already in device memory (DeviceBuffer.ptr); enqueues only"""
        rc = lib().mars_hip_preprocess_device(self.p, input_index, C.c_void_p(dev_ptr), int(w), int(h), first_frame, int(frames))
        if rc != MARS_OK:
            raise MarsError(rc, "mars_hip_preprocess_device")

    def preprocess_nv12_device(self, dev_ptr, w, h, frames, flags=0, first_frame=0, input_index=0):
        """mars_hip_preprocess_nv12_device: NV12 frames already in device memory; enqueues only"""
        rc = lib().mars_hip_preprocess_nv12_device(self.p, input_index, C.c_void_p(dev_ptr), int(w), int(h), int(flags), first_frame, int(frames))
        if rc != MARS_OK:
            raise MarsError(rc, "mars_hip_preprocess_nv12_device")

    def preprocess_tiles(self, frames, opts, input_index=0, device=False):
        """tiled inference, the front-end: batch / opts.n_tiles camera frames -> their tiles in graph input `input_index`, model frame
        c * n_tiles + t = tile t of camera frame c.  device=False: frames = uint8 host array, uploaded, the call waits
        (mars_hip_preprocess_tiles); device=True: frames = a device address (DeviceBuffer.ptr), enqueues only"""
        if device:
            rc = lib().mars_hip_preprocess_tiles_device(self.p, input_index, C.c_void_p(frames), C.byref(opts))
        else:
            a = np.ascontiguousarray(frames, dtype=np.uint8).reshape(-1)
            fb = _tile_frame_bytes(opts)
            if opts.n_tiles > 0 and self.batch % opts.n_tiles == 0 and fb > 0 and a.size != fb * (self.batch // opts.n_tiles):
                raise ValueError("%d camera frames of %d bytes each, got %d bytes" % (self.batch // opts.n_tiles, fb, a.size))
            rc = lib().mars_hip_preprocess_tiles(self.p, input_index, a.ctypes.data, C.byref(opts))
        if rc != MARS_OK:
            raise MarsError(rc, "mars_hip_preprocess_tiles")

    def merge_tiles(self, opts):
        """tiled inference, the merge: the per-tile lists the last detect_*_device left in HBM (graph-input pixels) -> one list per camera
        frame in camera pixels, on the device (mars_hip_merge_tiles_device); enqueues only, tile_results() waits"""
        rc = lib().mars_hip_merge_tiles_device(self.p, C.byref(opts))
        if rc != MARS_OK:
            raise MarsError(rc, "mars_hip_merge_tiles_device")

    def tile_results(self):
        """-> (DET_DTYPE [C][MAX_DET], counts [C], TILE_SRC_DTYPE [C][MAX_DET], TILE_STATS_DTYPE [C]) of the last merge_tiles(); waits"""
        n = max(lib().mars_hip_tile_frames(self.p), 1)  # the library's own count; before any merge it is 0 and the call below refuses
        out = np.zeros((n, MAX_DET), dtype=DET_DTYPE)
        oc = np.zeros(n, dtype=np.int32)
        org = np.zeros((n, MAX_DET), dtype=TILE_SRC_DTYPE)
        st = np.zeros(n, dtype=TILE_STATS_DTYPE)
        rc = lib().mars_hip_tile_results(self.p, out.ctypes.data, oc.ctypes.data, org.ctypes.data, st.ctypes.data)
        if rc != MARS_OK:
            raise MarsError(rc, "mars_hip_tile_results")
        return out, oc, org, st

    def tile_ms(self):
        """device time (ms) of the last merge_tiles() kernel (mars_hip_tile_ms); < 0: not available"""
        return float(lib().mars_hip_tile_ms(self.p))

    def crop_detections(self, det_model, frames, opts, input_index=0, device=False):
        """the second stage: the detections det_model's last detect_*_device left in HBM -> crops of its frames in THIS model's input
        `input_index`, one per frame of this model's batch.  device=False: frames = uint8 host array, uploaded, the call waits
        (mars_hip_crop_detections); device=True: frames = a device address (DeviceBuffer.ptr), enqueues only
        (mars_hip_crop_detections_device)"""
        if device:
            rc = lib().mars_hip_crop_detections_device(det_model.p, C.c_void_p(frames), self.p, input_index, C.byref(opts))
        else:
            a = np.ascontiguousarray(frames, dtype=np.uint8)
            rc = lib().mars_hip_crop_detections(det_model.p, a.ctypes.data, self.p, input_index, C.byref(opts))
        if rc != MARS_OK:
            raise MarsError(rc, "mars_hip_crop_detections")

    def crop_obb_detections(self, det_model, frames, opts, input_index=0):
        """crop_detections over the oriented boxes det_model's last detect_obb_device left in HBM, each cut along its own axes: frames =
        uint8 host array, uploaded, the call waits (mars_hip_crop_obb)"""
        a = np.ascontiguousarray(frames, dtype=np.uint8)
        rc = lib().mars_hip_crop_obb(det_model.p, a.ctypes.data, self.p, input_index, C.byref(opts))
        if rc != MARS_OK:
            raise MarsError(rc, "mars_hip_crop_obb")

    def crop_obb_detections_device(self, det_model, frames_dev, opts, input_index=0):
        """the same with frames_dev = a device address (DeviceBuffer.ptr); enqueues only (mars_hip_crop_obb_device)"""
        rc = lib().mars_hip_crop_obb_device(det_model.p, C.c_void_p(frames_dev), self.p, input_index, C.byref(opts))
        if rc != MARS_OK:
            raise MarsError(rc, "mars_hip_crop_obb_device")

    def crop_pose_detections(self, det_model, frames, opts, align, input_index=0):
        """crop_detections over the keypoints det_model's last detect_pose_device left in HBM, each set fitted to the template of `align`
        (align_opts(...)) and cut aligned: frames = uint8 host array, uploaded, the call waits (mars_hip_crop_pose)"""
        a = np.ascontiguousarray(frames, dtype=np.uint8)
        rc = lib().mars_hip_crop_pose(det_model.p, a.ctypes.data, self.p, input_index, C.byref(opts), C.byref(align) if align is not None else None)
        if rc != MARS_OK:
            raise MarsError(rc, "mars_hip_crop_pose")

    def crop_pose_detections_device(self, det_model, frames_dev, opts, align, input_index=0):
        """the same with frames_dev = a device address (DeviceBuffer.ptr); enqueues only (mars_hip_crop_pose_device)"""
        rc = lib().mars_hip_crop_pose_device(det_model.p, C.c_void_p(frames_dev), self.p, input_index, C.byref(opts),
                                             C.byref(align) if align is not None else None)
        if rc != MARS_OK:
            raise MarsError(rc, "mars_hip_crop_pose_device")

    def align_results(self):
        """-> ALIGN_DTYPE [batch]: the fit records of the last aligned crop call, record k beside roi_results()[0][k], zeros behind the kept
        ones (mars_hip_align_results); waits"""
        fits = np.zeros(self.batch, dtype=ALIGN_DTYPE)
        rc = lib().mars_hip_align_results(self.p, fits.ctypes.data, self.batch)
        if rc != MARS_OK:
            raise MarsError(rc, "mars_hip_align_results")
        return fits

    def roi_results(self):
        """-> (ROI_DTYPE records of the crops the last crop_detections() wrote, frame k of the input <- rois[k]; boxes dropped for want of a frame)"""
        rois = np.zeros(self.batch, dtype=ROI_DTYPE)
        kept, dropped = C.c_int(0), C.c_int(0)
        rc = lib().mars_hip_roi_results(self.p, rois.ctypes.data, self.batch, C.byref(kept), C.byref(dropped))
        if rc != MARS_OK:
            raise MarsError(rc, "mars_hip_roi_results")
        return rois[:min(kept.value, self.batch)].copy(), dropped.value

    def classify_device(self, opts=None, **kw):
        """the classifier head of this model's current batch, on the device (mars_hip_classify_device): pools the feature tensor, ranks,
        scores; enqueues only.  opts = cls_opts(...), or its keywords"""
        o = opts if opts is not None else cls_opts(**kw)
        rc = lib().mars_hip_classify_device(self.p, C.byref(o))
        if rc != MARS_OK:
            raise MarsError(rc, "mars_hip_classify_device")

    def classify_results(self, top_k, want_sums=True):
        """-> (CLS_DTYPE entries [batch][top_k], int32 sums [batch][C] or None) of the last classify_device().  top_k MUST be the one
        given there: the library copies batch x that many entries, and a smaller top_k here makes the array too short for them.  Waits"""
        n = self.batch
        top = np.zeros((n, max(int(top_k), 1)), dtype=CLS_DTYPE)
        sums = np.zeros((n, 4096), dtype=np.int32) if want_sums else None
        ch = C.c_int(0)
        rc = lib().mars_hip_classify_results(self.p, top.ctypes.data, sums.ctypes.data if want_sums else None, C.byref(ch))
        if rc != MARS_OK:
            raise MarsError(rc, "mars_hip_classify_results")
        return top, (sums.reshape(-1)[:n * ch.value].reshape(n, ch.value).copy() if want_sums else None)

    def classify(self, opts=None, want_sums=True, **kw):
        """classify_device + classify_results (mars_hip_classify's work, through the two calls: the channel count is only known afterwards)"""
        o = opts if opts is not None else cls_opts(**kw)
        self.classify_device(o)
        return self.classify_results(o.top_k if o.top_k else 1, want_sums)

    def label_detections(self, cls_model):
        """THIS model is the detector: cls_model's top-1 entries go through its ROI table onto this model's detection lists, on the device
        (mars_hip_label_detections_device); enqueues only"""
        rc = lib().mars_hip_label_detections_device(self.p, cls_model.p)
        if rc != MARS_OK:
            raise MarsError(rc, "mars_hip_label_detections_device")

    def label_results(self):
        """-> CLS_DTYPE [batch][MAX_DET]: entry i of frame f belongs to detect_results()[f][i]; {-1, 0} where no crop was cut.  Waits"""
        labels = np.zeros((self.batch, MAX_DET), dtype=CLS_DTYPE)
        rc = lib().mars_hip_label_results(self.p, labels.ctypes.data)
        if rc != MARS_OK:
            raise MarsError(rc, "mars_hip_label_results")
        return labels

    def match_device(self, gallery, opts=None, **kw):
        """the pooled sums of the last classify_device() against the gallery, on the device (mars_hip_match_device); enqueues only.
        opts = match_opts(...), or its keywords"""
        o = opts if opts is not None else match_opts(**kw)
        rc = lib().mars_hip_match_device(self.p, gallery.p, C.byref(o))
        if rc != MARS_OK:
            raise MarsError(rc, "mars_hip_match_device")
        self._match_top_k = o.top_k if o.top_k else 1

    def match_results(self, top_k=None, want_rows=True):
        """-> (CLS_DTYPE entries [batch][top_k] with cls = id, int32 rows [batch][top_k] or None) of the last match_device().  The arrays
        are sized by the top_k that call enqueued (the library copies that many entries per frame); a top_k given here must equal it.
        Waits"""
        k = getattr(self, "_match_top_k", 0)
        if not k:  # no match call yet: the library refuses below
            k = max(int(top_k or 1), 1)
        elif top_k is not None and max(int(top_k), 1) != k:
            raise ValueError("match_results(top_k=%d) after match_device(top_k=%d)" % (top_k, k))
        top = np.zeros((self.batch, k), dtype=CLS_DTYPE)
        rows = np.zeros((self.batch, k), dtype=np.int32) if want_rows else None
        rc = lib().mars_hip_match_results(self.p, top.ctypes.data, rows.ctypes.data if want_rows else None)
        if rc != MARS_OK:
            raise MarsError(rc, "mars_hip_match_results")
        return top, rows

    def match(self, gallery, opts=None, want_rows=True, **kw):
        """match_device + match_results (mars_hip_match)"""
        o = opts if opts is not None else match_opts(**kw)
        k = o.top_k if o.top_k else 1
        top = np.zeros((self.batch, max(k, 1)), dtype=CLS_DTYPE)
        rows = np.zeros((self.batch, max(k, 1)), dtype=np.int32) if want_rows else None
        rc = lib().mars_hip_match(self.p, gallery.p, C.byref(o), top.ctypes.data, rows.ctypes.data if want_rows else None)
        if rc != MARS_OK:
            raise MarsError(rc, "mars_hip_match")
        self._match_top_k = k
        return top, rows

    def identify_detections(self, cls_model):
        """THIS model is the detector: cls_model's top-1 match entries go through its ROI table onto this model's detection lists, on the
        device (mars_hip_identify_detections_device), into an array beside the labels; enqueues only"""
        rc = lib().mars_hip_identify_detections_device(self.p, cls_model.p)
        if rc != MARS_OK:
            raise MarsError(rc, "mars_hip_identify_detections_device")

    def identity_results(self):
        """-> CLS_DTYPE [batch][MAX_DET] with cls = id: entry i of frame f belongs to detect_results()[f][i]; {-1, 0} where no crop was cut
        or nothing matched.  Waits"""
        idents = np.zeros((self.batch, MAX_DET), dtype=CLS_DTYPE)
        rc = lib().mars_hip_identity_results(self.p, idents.ctypes.data)
        if rc != MARS_OK:
            raise MarsError(rc, "mars_hip_identity_results")
        return idents

    def redact_device(self, frames_dev, opts, dst_dev=None):
        """THIS model is the detector: its batch of frames at the device address frames_dev with the regions of the detections its last
        detect_*_device left in HBM mosaicked or filled, in place or (dst_dev: a second device address) into another buffer; enqueues only
        (mars_hip_redact_device)"""
        rc = lib().mars_hip_redact_device(self.p, C.c_void_p(frames_dev), C.c_void_p(dst_dev) if dst_dev else None, C.byref(opts))
        if rc != MARS_OK:
            raise MarsError(rc, "mars_hip_redact_device")

    def redact_results(self):
        """-> REDACT_STATS_DTYPE [batch] of the last redact_device() (mars_hip_redact_results); waits"""
        stats = np.zeros(self.batch, dtype=REDACT_STATS_DTYPE)
        rc = lib().mars_hip_redact_results(self.p, stats.ctypes.data)
        if rc != MARS_OK:
            raise MarsError(rc, "mars_hip_redact_results")
        return stats

    def redact(self, frames, opts):
        """redact_device on frames in host memory (uint8, this model's batch of them): -> (the redacted frames, the statistics); the caller's
        array is left alone (mars_hip_redact works in place on a copy); waits"""
        a = np.ascontiguousarray(frames, dtype=np.uint8).reshape(-1).copy()
        fb = redact_frame_bytes(opts)
        if fb <= 0 or a.size != fb * self.batch:
            raise ValueError("%d frames of %d bytes each, got %d bytes" % (self.batch, fb, a.size))
        stats = np.zeros(self.batch, dtype=REDACT_STATS_DTYPE)
        rc = lib().mars_hip_redact(self.p, a.ctypes.data, C.byref(opts), stats.ctypes.data)
        if rc != MARS_OK:
            raise MarsError(rc, "mars_hip_redact")
        return a.reshape(self.batch, fb), stats

    def redact_ms(self):
        """device time (ms) of the last redact_device() (mars_hip_redact_ms); < 0: not available"""
        return float(lib().mars_hip_redact_ms(self.p))

    def overlay_device(self, frames_dev, opts, dst_dev=None):
        """paint the detections the last detect*(device=True) left in HBM -- and, where opts asks for them, this batch's track ids, native
        masks and keypoints -- into this model's batch of frames at device pointer frames_dev (overlay_opts(); dst_dev None: in place);
        enqueues only (mars_hip_overlay_device)"""
        rc = lib().mars_hip_overlay_device(self.p, C.c_void_p(frames_dev), C.c_void_p(dst_dev) if dst_dev else None, C.byref(opts))
        if rc != MARS_OK:
            raise MarsError(rc, "mars_hip_overlay_device")

    def overlay_results(self):
        """-> OVERLAY_STATS_DTYPE [batch] of the last overlay_device() (mars_hip_overlay_results); waits"""
        stats = np.zeros(self.batch, dtype=OVERLAY_STATS_DTYPE)
        rc = lib().mars_hip_overlay_results(self.p, stats.ctypes.data)
        if rc != MARS_OK:
            raise MarsError(rc, "mars_hip_overlay_results")
        return stats

    def overlay(self, frames, opts):
        """overlay_device on frames in host memory (uint8, this model's batch of them): -> (the painted frames, the statistics); the caller's
        array is left alone (mars_hip_overlay works in place on a copy); waits"""
        a = np.ascontiguousarray(frames, dtype=np.uint8).reshape(-1).copy()
        fb = redact_frame_bytes(opts)
        if a.size != fb * self.batch:
            raise ValueError("%d frames of %d bytes, got %d bytes" % (self.batch, fb, a.size))
        stats = np.zeros(self.batch, dtype=OVERLAY_STATS_DTYPE)
        rc = lib().mars_hip_overlay(self.p, a.ctypes.data, C.byref(opts), stats.ctypes.data)
        if rc != MARS_OK:
            raise MarsError(rc, "mars_hip_overlay")
        return a.reshape(self.batch, fb), stats

    def overlay_ms(self):
        """device time (ms) of the last overlay_device() (mars_hip_overlay_ms); < 0: not available"""
        return float(lib().mars_hip_overlay_ms(self.p))

    def motion_detections_device(self, motion, expand=0.0):
        """THIS model is the detector: the detections its last detect_*_device call left in HBM are counted against the maps of motion's
        last call (mars_hip_motion_detections_device); enqueues only"""
        rc = lib().mars_hip_motion_detections_device(self.p, motion.p, float(expand))
        if rc != MARS_OK:
            raise MarsError(rc, "mars_hip_motion_detections_device")

    def motion_det_results(self):
        """-> MOTION_DET_DTYPE [batch][MAX_DET]: entry i of frame f belongs to detect_results()[f][i] (mars_hip_motion_det_results); waits"""
        out = np.zeros((self.batch, MAX_DET), dtype=MOTION_DET_DTYPE)
        rc = lib().mars_hip_motion_det_results(self.p, out.ctypes.data)
        if rc != MARS_OK:
            raise MarsError(rc, "mars_hip_motion_det_results")
        return out

    def track_device(self, tracker, opts=None, **kw):
        """THIS model is the detector: the detections its last detect_*_device call left in HBM (and, with carry_identity, the identities
        of identify_detections) go through the tracker, on the device (mars_hip_track_device); enqueues only.  opts = track_opts(...), or
        its keywords"""
        o = opts if opts is not None else track_opts(**kw)
        rc = lib().mars_hip_track_device(self.p, tracker.p, C.byref(o))
        if rc != MARS_OK:
            raise MarsError(rc, "mars_hip_track_device")

    def track_results(self):
        """-> TRACK_DTYPE [batch][MAX_DET]: entry i of frame f belongs to detect_results()[f][i]; {-1, 0} where no track took the box.  Waits"""
        tracks = np.zeros((self.batch, MAX_DET), dtype=TRACK_DTYPE)
        rc = lib().mars_hip_track_results(self.p, tracks.ctypes.data)
        if rc != MARS_OK:
            raise MarsError(rc, "mars_hip_track_results")
        return tracks

    def track_app_device(self, cls_model, tracker, opts=None, app=None, **kw):
        """track_device with the embeddings of the second stage: the sums cls_model's last classify_device left and the ROI table of the crop
        call from this model into it steer the association (mars_hip_track_app_device); enqueues only.  app = track_app_opts(...)"""
        o = opts if opts is not None else track_opts(**kw)
        a = app if app is not None else track_app_opts()
        rc = lib().mars_hip_track_app_device(self.p, cls_model.p, tracker.p, C.byref(o), C.byref(a))
        if rc != MARS_OK:
            raise MarsError(rc, "mars_hip_track_app_device")

    def track_app(self, cls_model, tracker, opts=None, app=None, **kw):
        """track_app_device + track_results (mars_hip_track_app)"""
        o = opts if opts is not None else track_opts(**kw)
        a = app if app is not None else track_app_opts()
        tracks = np.zeros((self.batch, MAX_DET), dtype=TRACK_DTYPE)
        rc = lib().mars_hip_track_app(self.p, cls_model.p, tracker.p, C.byref(o), C.byref(a), tracks.ctypes.data)
        if rc != MARS_OK:
            raise MarsError(rc, "mars_hip_track_app")
        return tracks

    def track(self, tracker, opts=None, **kw):
        """track_device + track_results (mars_hip_track)"""
        o = opts if opts is not None else track_opts(**kw)
        tracks = np.zeros((self.batch, MAX_DET), dtype=TRACK_DTYPE)
        rc = lib().mars_hip_track(self.p, tracker.p, C.byref(o), tracks.ctypes.data)
        if rc != MARS_OK:
            raise MarsError(rc, "mars_hip_track")
        return tracks

    def events_device(self, events, opts=None, **kw):
        """THIS model is the detector: the detections its last detect_*_device call left in HBM and the track ids track_device or
        track_app_device hung on them go through the events object, on the device (mars_hip_events_device); enqueues only.  opts =
        event_opts(...), or its keywords"""
        o = opts if opts is not None else event_opts(**kw)
        rc = lib().mars_hip_events_device(self.p, events.p, C.byref(o))
        if rc != MARS_OK:
            raise MarsError(rc, "mars_hip_events_device")

    def events_results(self, events):
        """-> (EVENT_DTYPE [batch][MAX_DET], line counts, zone counts) as event_lists gives them: entry i of frame f belongs to
        detect_results()[f][i] (mars_hip_events_results); waits"""
        rec, lc, zc = _event_arrays(self.batch, MAX_DET)
        rc = lib().mars_hip_events_results(self.p, events.p, rec.ctypes.data, lc.ctypes.data, zc.ctypes.data)
        if rc != MARS_OK:
            raise MarsError(rc, "mars_hip_events_results")
        return rec, lc, zc

    def events(self, events, opts=None, **kw):
        """events_device + events_results (mars_hip_events)"""
        o = opts if opts is not None else event_opts(**kw)
        rec, lc, zc = _event_arrays(self.batch, MAX_DET)
        rc = lib().mars_hip_events(self.p, events.p, C.byref(o), rec.ctypes.data, lc.ctypes.data, zc.ctypes.data)
        if rc != MARS_OK:
            raise MarsError(rc, "mars_hip_events")
        return rec, lc, zc

    def shots_device(self, det_model, shots, opts=None, input_index=0, **kw):
        """THIS model is the second stage: the crops the last crop call out of det_model wrote into its input, its ROI table, and
        det_model's detection lists and track ids go through the shots object, on the device (mars_hip_shots_device); enqueues only.
        opts = shot_opts(...), or its keywords"""
        o = opts if opts is not None else shot_opts(**kw)
        rc = lib().mars_hip_shots_device(det_model.p, self.p, int(input_index), shots.p, C.byref(o))
        if rc != MARS_OK:
            raise MarsError(rc, "mars_hip_shots_device")

    def shots_results(self, shots):
        """-> SHOT_DTYPE [batch]: entry k belongs to roi_results()[0][k] (mars_hip_shots_results); waits"""
        rec = np.zeros(self.batch, dtype=SHOT_DTYPE)
        rc = lib().mars_hip_shots_results(self.p, shots.p, rec.ctypes.data)
        if rc != MARS_OK:
            raise MarsError(rc, "mars_hip_shots_results")
        return rec

    def shots(self, det_model, shots, opts=None, input_index=0, **kw):
        """shots_device + shots_results (mars_hip_shots)"""
        o = opts if opts is not None else shot_opts(**kw)
        rec = np.zeros(self.batch, dtype=SHOT_DTYPE)
        rc = lib().mars_hip_shots(det_model.p, self.p, int(input_index), shots.p, C.byref(o), rec.ctypes.data)
        if rc != MARS_OK:
            raise MarsError(rc, "mars_hip_shots")
        return rec

    def write_tensor(self, idx, data, frame=0):
        """mars_hip_write_tensor: one frame of an activation tensor from host memory"""
        a = np.ascontiguousarray(data).view(np.uint8).reshape(-1)
        rc = lib().mars_hip_write_tensor(self.p, idx, frame, a.ctypes.data, a.size)
        if rc != MARS_OK:
            raise MarsError(rc, "write_tensor %d" % idx)

    def set_tuning(self, key, value):
        """per-model override of a launch-policy knob (mars_hip_model_set_tuning)"""
        if lib().mars_hip_model_set_tuning(self.p, key.encode(), int(value)) != 0:
            raise KeyError(key)

    def get_tuning(self, key):
        v = C.c_int(0)
        if lib().mars_hip_model_get_tuning(self.p, key.encode(), C.byref(v)) != 0:
            raise KeyError(key)
        return v.value

    def autotune(self, reps=3):
        rc = lib().mars_hip_autotune(self.p, reps)
        if rc != 0:
            raise MarsError(rc, "mars_hip_autotune")

    def ops(self):
        n = lib().mars_hip_num_ops(self.p)
        res = []
        for i in range(n):
            layer, kind = C.c_int(), C.c_int()
            macs, byt, ms = C.c_double(), C.c_double(), C.c_float()
            lib().mars_hip_op_info(self.p, i, C.byref(layer), C.byref(kind), C.byref(macs), C.byref(byt), C.byref(ms))
            res.append(dict(layer=layer.value, kind=kind.value, macs=macs.value, bytes=byt.value, ms=ms.value))
        return res

    def param_arena(self):
        n = C.c_size_t()
        p = lib().mars_hip_param_arena(self.p, C.byref(n))
        return p, n.value

    def detect(self, outputs=(0,), thresh=0.45):
        idx = (C.c_int * len(outputs))(*outputs)
        dets = np.zeros((self.batch, MAX_DET), dtype=DET_DTYPE)
        counts = np.zeros(self.batch, dtype=np.int32)
        rc = lib().mars_hip_detect(self.p, idx, len(outputs), thresh, dets.ctypes.data,
                                   counts.ctypes.data_as(C.POINTER(C.c_int)))
        if rc != MARS_OK:
            raise MarsError(rc, "mars_hip_detect")
        return [dets[f, :counts[f]].copy() for f in range(self.batch)]

    def detect_device(self, outputs=(0,), thresh=0.45):
        idx = (C.c_int * len(outputs))(*outputs)
        rc = lib().mars_hip_detect_device(self.p, idx, len(outputs), thresh)
        if rc != MARS_OK:
            raise MarsError(rc, "mars_hip_detect_device")

    def detect_heads(self, heads=None, anchors=None, conf=0.25, thresh=0.45, src=None):
        """decode + NMS of raw YOLOv5 Detect heads (mars_hip_detect_heads): a record array per frame, as detect().  Arguments
        as for yolo_heads()."""
        h = yolo_heads(heads, anchors, conf, thresh, src)
        dets = np.zeros((self.batch, MAX_DET), dtype=DET_DTYPE)
        counts = np.zeros(self.batch, dtype=np.int32)
        rc = lib().mars_hip_detect_heads(self.p, C.byref(h), dets.ctypes.data, counts.ctypes.data_as(C.POINTER(C.c_int)))
        if rc != MARS_OK:
            raise MarsError(rc, "mars_hip_detect_heads")
        return [dets[f, :counts[f]].copy() for f in range(self.batch)]

    def detect_heads_device(self, heads=None, anchors=None, conf=0.25, thresh=0.45, src=None):
        rc = lib().mars_hip_detect_heads_device(self.p, C.byref(yolo_heads(heads, anchors, conf, thresh, src)))
        if rc != MARS_OK:
            raise MarsError(rc, "mars_hip_detect_heads_device")

    def detect_dfl(self, heads=None, **kw):
        """decode + NMS of raw anchor-free DFL heads (mars_hip_detect_dfl): a record array per frame, as detect().  Arguments as for
        yolo_dfl_heads()."""
        h = yolo_dfl_heads(heads, **kw)
        dets = np.zeros((self.batch, MAX_DET), dtype=DET_DTYPE)
        counts = np.zeros(self.batch, dtype=np.int32)
        rc = lib().mars_hip_detect_dfl(self.p, C.byref(h), dets.ctypes.data, counts.ctypes.data_as(C.POINTER(C.c_int)))
        if rc != MARS_OK:
            raise MarsError(rc, "mars_hip_detect_dfl")
        return [dets[f, :counts[f]].copy() for f in range(self.batch)]

    def detect_dfl_device(self, heads=None, **kw):
        rc = lib().mars_hip_detect_dfl_device(self.p, C.byref(yolo_dfl_heads(heads, **kw)))
        if rc != MARS_OK:
            raise MarsError(rc, "mars_hip_detect_dfl_device")

    def detect_seg_device(self, seg, heads=None, **kw):
        """DFL decode + NMS + instance masks, results stay in HBM (mars_hip_detect_seg_device).  seg: seg_opts(); heads and the keywords
        as for yolo_dfl_heads()"""
        rc = lib().mars_hip_detect_seg_device(self.p, C.byref(yolo_dfl_heads(heads, **kw)), C.byref(seg) if seg is not None else None)
        if rc != MARS_OK:
            raise MarsError(rc, "mars_hip_detect_seg_device")
        self._seg_max = seg.max_per_frame or 16

    def mask_results(self):
        """the masks the last detect_seg_device left in HBM (mars_hip_mask_results): (records MASK_DTYPE [batch][max_per_frame],
        words uint32 [batch][max_per_frame][PH][pitch], PW); unpack_masks(words, PW) gives the pixels"""
        ph, pw, pitch = C.c_int(), C.c_int(), C.c_int()
        rc = lib().mars_hip_mask_results(self.p, None, None, C.byref(ph), C.byref(pw), C.byref(pitch))
        if rc != MARS_OK:
            raise MarsError(rc, "mars_hip_mask_results")
        recs = np.zeros((self.batch, self._seg_max), dtype=MASK_DTYPE)
        words = np.zeros((self.batch, self._seg_max, ph.value, pitch.value), dtype=np.uint32)
        rc = lib().mars_hip_mask_results(self.p, recs.ctypes.data, words.ctypes.data, None, None, None)
        if rc != MARS_OK:
            raise MarsError(rc, "mars_hip_mask_results")
        return recs, words, pw.value

    def detect_seg(self, seg, heads=None, **kw):
        """detect_seg_device + detect_results + mask_results (mars_hip_detect_seg): (a record array per frame, records, words, PW)"""
        self.detect_seg_device(seg, heads, **kw)
        return (self.detect_results(),) + self.mask_results()

    def detect_seg_native_device(self, seg, native=None, heads=None, **kw):
        """DFL decode + NMS + instance masks in frame pixels, results stay in HBM (mars_hip_detect_seg_native_device).  seg: seg_opts();
        native: mask_native_opts() or None (every default); heads and the keywords as for yolo_dfl_heads()"""
        rc = lib().mars_hip_detect_seg_native_device(self.p, C.byref(yolo_dfl_heads(heads, **kw)), C.byref(seg) if seg is not None else None,
                                                     C.byref(native) if native is not None else None)
        if rc != MARS_OK:
            raise MarsError(rc, "mars_hip_detect_seg_native_device")
        self._segn_max = seg.max_per_frame or 16

    def mask_native_results(self):
        """the masks the last detect_seg_native_device left in HBM (mars_hip_mask_native_results): (records MASK_DTYPE [batch][max_per_frame],
        words uint32 [batch][max_per_frame][out_h][pitch], out_w); unpack_masks(words, out_w) gives the pixels"""
        oh, ow, pitch = C.c_int(), C.c_int(), C.c_int()
        rc = lib().mars_hip_mask_native_results(self.p, None, None, C.byref(oh), C.byref(ow), C.byref(pitch))
        if rc != MARS_OK:
            raise MarsError(rc, "mars_hip_mask_native_results")
        recs = np.zeros((self.batch, self._segn_max), dtype=MASK_DTYPE)
        words = np.zeros((self.batch, self._segn_max, oh.value, pitch.value), dtype=np.uint32)
        rc = lib().mars_hip_mask_native_results(self.p, recs.ctypes.data, words.ctypes.data, None, None, None)
        if rc != MARS_OK:
            raise MarsError(rc, "mars_hip_mask_native_results")
        return recs, words, ow.value

    def detect_seg_native(self, seg, native=None, heads=None, **kw):
        """detect_seg_native_device + detect_results + mask_native_results: (a record array per frame, records, words, out_w)"""
        self.detect_seg_native_device(seg, native, heads, **kw)
        return (self.detect_results(),) + self.mask_native_results()

    def detect_pose_device(self, pose, heads=None, **kw):
        """DFL decode + NMS + pose keypoints, results stay in HBM (mars_hip_detect_pose_device).  pose: pose_opts(); heads and the keywords
        as for yolo_dfl_heads()"""
        rc = lib().mars_hip_detect_pose_device(self.p, C.byref(yolo_dfl_heads(heads, **kw)), C.byref(pose) if pose is not None else None)
        if rc != MARS_OK:
            raise MarsError(rc, "mars_hip_detect_pose_device")
        self._pose_max = pose.max_per_frame or 32

    def pose_results(self):
        """the keypoints the last detect_pose_device left in HBM (mars_hip_pose_results): (records POSE_DTYPE [batch][max_per_frame],
        keypoints KPT_DTYPE [batch][max_per_frame][K])"""
        k = C.c_int()
        rc = lib().mars_hip_pose_results(self.p, None, None, C.byref(k))
        if rc != MARS_OK:
            raise MarsError(rc, "mars_hip_pose_results")
        recs = np.zeros((self.batch, self._pose_max), dtype=POSE_DTYPE)
        kpts = np.zeros((self.batch, self._pose_max, k.value), dtype=KPT_DTYPE)
        rc = lib().mars_hip_pose_results(self.p, recs.ctypes.data, kpts.ctypes.data, None)
        if rc != MARS_OK:
            raise MarsError(rc, "mars_hip_pose_results")
        return recs, kpts

    def detect_pose(self, pose, heads=None, **kw):
        """detect_pose_device + detect_results + pose_results (mars_hip_detect_pose): (a record array per frame, records, keypoints)"""
        self.detect_pose_device(pose, heads, **kw)
        return (self.detect_results(),) + self.pose_results()

    def pose_ms(self):
        """device time (ms) of the keypoint stage of the last detect_pose_device (mars_hip_pose_ms); < 0: not available"""
        return float(lib().mars_hip_pose_ms(self.p))

    def detect_obb_device(self, obb, heads=None, **kw):
        """oriented decode + sort + rotated NMS, results stay in HBM (mars_hip_detect_obb_device).  obb: obb_opts(); heads and the keywords
        as for yolo_dfl_heads()"""
        rc = lib().mars_hip_detect_obb_device(self.p, C.byref(yolo_dfl_heads(heads, **kw)), C.byref(obb) if obb is not None else None)
        if rc != MARS_OK:
            raise MarsError(rc, "mars_hip_detect_obb_device")

    def obb_results(self):
        """the oriented boxes the last detect_obb_device left in HBM (mars_hip_obb_results): an OBB_DTYPE array per frame"""
        boxes = np.zeros((self.batch, MAX_DET), dtype=OBB_DTYPE)
        counts = np.zeros(self.batch, dtype=np.int32)
        rc = lib().mars_hip_obb_results(self.p, boxes.ctypes.data, counts.ctypes.data)
        if rc != MARS_OK:
            raise MarsError(rc, "mars_hip_obb_results")
        return [boxes[f, :counts[f]].copy() for f in range(self.batch)]

    def detect_obb(self, obb, heads=None, **kw):
        """detect_obb_device + detect_results + obb_results: (the enclosing upright rectangles, a record array per frame; the oriented boxes,
        an OBB_DTYPE array per frame, index-aligned)"""
        self.detect_obb_device(obb, heads, **kw)
        return self.detect_results(), self.obb_results()

    def obb_ms(self):
        """device time (ms) of the oriented stage (decode + sort + NMS) of the last detect_obb_device (mars_hip_obb_ms); < 0: not available"""
        return float(lib().mars_hip_obb_ms(self.p))

    def detect_results(self):
        """the detections the last detect_device / detect_heads_device / detect_dfl_device left in HBM (mars_hip_detect_results)"""
        dets = np.zeros((self.batch, MAX_DET), dtype=DET_DTYPE)
        counts = np.zeros(self.batch, dtype=np.int32)
        rc = lib().mars_hip_detect_results(self.p, dets.ctypes.data, counts.ctypes.data_as(C.POINTER(C.c_int)))
        if rc != MARS_OK:
            raise MarsError(rc, "mars_hip_detect_results")
        return [dets[f, :counts[f]].copy() for f in range(self.batch)]

    # -- pipelined host I/O (mars_hip_pipe_*)
    def pipe_open(self, download_outputs=True, detect=False, det_outputs=(0,), thresh=0.45, camera=None, heads=None, dfl_heads=None,
                  camera_format=CAMERA_RGB, camera_flags=0):
        """camera = (w, h): input 0 is fed from uint8 RGB camera frames, the letterbox front-end runs on the device behind the upload.
        camera_format = CAMERA_NV12: the frames are NV12 (w * h * 3 / 2 bytes each; camera_flags: NV12_FULL_RANGE | NV12_VU).
        heads (with detect): True (found on the file), a list as for detect_heads() or a YoloHeads -- the tail decodes those raw
        heads instead of det_outputs; in camera mode their boxes come back in camera pixels.  dfl_heads: the same for anchor-free DFL
        heads (True, a list as for detect_dfl() or a YoloDflHeads); not both"""
        cw, ch = camera if camera else (0, 0)
        o = PipeOpts(int(download_outputs), int(detect), (C.c_int * 4)(*(list(det_outputs) + [0] * (4 - len(det_outputs)))),
                     len(det_outputs) if detect else 0, thresh, int(cw), int(ch))
        if heads is not None and heads is not False:
            h = heads if isinstance(heads, YoloHeads) else yolo_heads(None if heads is True else heads, thresh=thresh)
            o.heads = C.pointer(h)  # copied by mars_hip_pipe_open
        if dfl_heads is not None and dfl_heads is not False:
            dh = dfl_heads if isinstance(dfl_heads, YoloDflHeads) else yolo_dfl_heads(None if dfl_heads is True else dfl_heads, thresh=thresh)
            o.dfl_heads = C.pointer(dh)
        o.camera_format, o.camera_flags = int(camera_format), int(camera_flags)
        rc = lib().mars_hip_pipe_open(self.p, C.byref(o))
        if rc != MARS_OK:
            raise MarsError(rc, "mars_hip_pipe_open")
        self._pipe = (bool(download_outputs), bool(detect))
        self._pipe_camera = (int(cw), int(ch)) if camera else None
        self._pipe_camera_nv12 = bool(camera) and int(camera_format) == CAMERA_NV12

    def pipe_input_view(self, i=0):
        """uint8 view [batch, frame_bytes] of the staging buffer the NEXT pipe_submit() uploads (camera mode, input 0:
        [batch, h * w * 3] RGB bytes, or [batch, h * w * 3 / 2] NV12 bytes)"""
        ptr = lib().mars_hip_pipe_input(self.p, i)
        if i == 0 and getattr(self, "_pipe_camera", None):
            n = self._pipe_camera[0] * self._pipe_camera[1] * 3 * self.batch
            if self._pipe_camera_nv12:
                n = lib().mars_hip_nv12_frame_bytes(*self._pipe_camera) * self.batch
        else:
            n = lib().mars_hip_tensor_frame_bytes(self.p, self.header.input_tensor_ids[i]) * self.batch
        return np.ctypeslib.as_array(C.cast(ptr, C.POINTER(C.c_uint8)), shape=(n,)).reshape(self.batch, -1)

    def pipe_submit(self):
        rc = lib().mars_hip_pipe_submit(self.p)
        if rc != MARS_OK:
            raise MarsError(rc, "mars_hip_pipe_submit")

    def pipe_wait(self, copy=True):
        """-> (outputs: list of uint8 [batch, frame_bytes] or None, dets: list of record arrays per frame or None).
        copy=False returns views into the pipe's pinned result buffers: valid until the SECOND pipe_submit() after this
        call (include/mars_hip.h, mars_hip_pipe_wait)."""
        nout = self.header.num_outputs
        outs = (C.c_void_p * max(nout, 1))()
        dets, counts = C.c_void_p(), C.c_void_p()
        rc = lib().mars_hip_pipe_wait(self.p, outs, C.byref(dets), C.byref(counts))
        if rc != MARS_OK:
            raise MarsError(rc, "mars_hip_pipe_wait")
        want_out, want_det = self._pipe
        ro = rd = None
        if want_out:
            ro = []
            for i in range(nout):
                n = lib().mars_hip_tensor_frame_bytes(self.p, self.header.output_tensor_ids[i]) * self.batch
                a = np.ctypeslib.as_array(C.cast(outs[i], C.POINTER(C.c_uint8)), shape=(n,)).reshape(self.batch, -1)
                ro.append(a.copy() if copy else a)
        if want_det:
            d = np.ctypeslib.as_array(C.cast(dets.value, C.POINTER(C.c_uint8)),
                                      shape=(self.batch * MAX_DET * DET_DTYPE.itemsize,)).view(DET_DTYPE).reshape(self.batch, MAX_DET)
            c = np.ctypeslib.as_array(C.cast(counts.value, C.POINTER(C.c_int32)), shape=(self.batch,))
            rd = [d[f, :c[f]].copy() for f in range(self.batch)] if copy else (d, c)
        return ro, rd

    def pipe_close(self):
        lib().mars_hip_pipe_close(self.p)

    def close(self):
        if self.p:
            lib().mars_free(self.p)
            self.p = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


# ---- direct kernels with host pointers (include/mxu_ops.h) --------------------
def conv2d_int8(nhwc, x, in_h, in_w, in_c, w, out_c, kh, kw, bias, out_h, out_w, sh, sw, pt, pl,
                in_scale, w_scale, out_scale):
    L = lib()
    fn = L.conv2d_int8_nhwc_mxu if nhwc else L.conv2d_int8_mxu
    x = np.ascontiguousarray(x, dtype=np.int8)
    w = np.ascontiguousarray(w, dtype=np.int8)
    b = None if bias is None else np.ascontiguousarray(bias, dtype=np.int32)
    out = np.zeros(out_h * out_w * out_c, dtype=np.int8)
    fn(x.ctypes.data, in_h, in_w, in_c, w.ctypes.data, out_c, kh, kw, None if b is None else b.ctypes.data,
       out.ctypes.data, out_h, out_w, sh, sw, pt, pl, in_scale, w_scale, out_scale)
    return out


def conv2d_f32(x, in_h, in_w, in_c, w, out_c, kh, kw, bias, out_h, out_w, sh, sw, pt, pl):
    x = np.ascontiguousarray(x, dtype=np.float32)
    w = np.ascontiguousarray(w, dtype=np.float32)
    b = None if bias is None else np.ascontiguousarray(bias, dtype=np.float32)
    out = np.zeros(out_h * out_w * out_c, dtype=np.float32)
    lib().conv2d_float32_mxu(x.ctypes.data, in_h, in_w, in_c, w.ctypes.data, out_c, kh, kw,
                             None if b is None else b.ctypes.data, out.ctypes.data, out_h, out_w, sh, sw, pt, pl, None)
    return out


def parse_output(pred_i8, npred, scale, maxd=1000):
    p = np.ascontiguousarray(pred_i8, dtype=np.int8)
    dets = np.zeros(maxd, dtype=DET_DTYPE)
    n = lib().mars_yolo_parse_output(p.ctypes.data, npred, scale, dets.ctypes.data, maxd)
    if n < 0:
        raise RuntimeError("mars_yolo_parse_output failed")
    return dets[:n].copy()


def nms(dets, thresh=0.45):
    d = np.ascontiguousarray(dets, dtype=DET_DTYPE).copy()
    n = lib().mars_yolo_nms(d.ctypes.data, len(d), thresh)
    if n < 0:
        raise RuntimeError("mars_yolo_nms failed")
    return d[:n].copy()
