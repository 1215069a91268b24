"""ctypes binding of libhmmr_hip.so (include/hmmr_hip.h).

There is no CPU fallback: if the shared library has not been built
(`python -m human_dynamics_amd.build`) `load()` raises, and every compute
entry point of the package goes through `load()`.
"""
from __future__ import annotations

import ctypes as C
import os

from . import devflags

HERE = os.path.dirname(os.path.abspath(__file__))
# devflags LIB_PATH (HMMR_LIB_PATH) lets a development run A/B two builds of the library; the default is the in-tree build
LIB_PATH = devflags.get("LIB_PATH") or os.path.join(HERE, "libhmmr_hip.so")

HMMR_F32, HMMR_BF16, HMMR_F16X3 = 0, 1, 2
FLAG_SATURATED = 1
FLAG_NAN = 2          # with FLAG_SATURATED: the clamped value was a NaN (include/hmmr_hip.h)
ABI_VERSION = 19
RESNET_UNITS = 16
RESNET_PROF_SLOTS = 64
MAX_TEMPORAL_BLOCKS = 8
MAX_REGRESSORS = 8

_vp, _fp, _ip = C.c_void_p, C.c_void_p, C.c_void_p   # all device pointers travel as void*


class ConvDesc(C.Structure):
    _fields_ = [
        ("in_", _vp), ("w", _vp), ("scale", _fp), ("shift", _fp), ("res", _vp), ("out", _vp),
        ("out2", _vp), ("scale2", _fp), ("shift2", _fp),
        ("in_dtype", C.c_int), ("out_dtype", C.c_int),
        ("n_img", C.c_int), ("hin", C.c_int), ("win", C.c_int), ("cin", C.c_int),
        ("in_img_stride", C.c_int64), ("in_row_stride", C.c_int), ("in_px_stride", C.c_int),
        ("kh", C.c_int), ("kw", C.c_int), ("sy", C.c_int), ("sx", C.c_int), ("py", C.c_int), ("px", C.c_int),
        ("ho", C.c_int), ("wo", C.c_int), ("cout", C.c_int), ("ldo", C.c_int),
        ("ldr", C.c_int), ("res_strided", C.c_int), ("res_img_stride", C.c_int64),
        ("res_row_stride", C.c_int), ("res_px_stride", C.c_int),
        ("relu", C.c_int), ("tile", C.c_int),
        ("split_k", C.c_int), ("ws", _vp), ("ws_bytes", C.c_size_t),
        ("pro_scale", _fp), ("pro_shift", _fp),
        ("out_b", _vp), ("ldo_b", C.c_int), ("n_split", C.c_int), ("relu_b", C.c_int),
        ("in2", _vp), ("cin2", C.c_int), ("k_order", C.c_int),
        ("batch", C.c_int), ("batch_in_bytes", C.c_int64), ("batch_w_bytes", C.c_int64), ("batch_out_bytes", C.c_int64),
        ("batch_res_bytes", C.c_int64), ("batch_scale_bytes", C.c_int64), ("batch_shift_bytes", C.c_int64),
    ]


class TailDesc(C.Structure):
    _fields_ = [
        ("dtype", C.c_int), ("h2", _vp), ("m", C.c_int), ("c_mid", C.c_int), ("depth", C.c_int),
        ("w3", _vp), ("scale3", _fp), ("shift3", _fp),
        ("res", _vp), ("ldr", C.c_int), ("res_strided", C.c_int), ("res_img_stride", C.c_int64),
        ("res_row_stride", C.c_int), ("res_px_stride", C.c_int), ("ho", C.c_int), ("wo", C.c_int),
        ("out", _vp), ("pre_scale", _fp), ("pre_shift", _fp),
        ("w1", _vp), ("scale1", _fp), ("shift1", _fp), ("relu1", C.c_int), ("n2", C.c_int),
        ("out_h1", _vp),
        ("h1", _vp), ("hin", C.c_int), ("win", C.c_int), ("w2", _vp), ("scale2", _fp), ("shift2", _fp),
        ("xp", _vp), ("wsc", _vp), ("shift_sc", _fp),
        ("conv2_stride", C.c_int), ("out_pre", _vp),
        ("pair_stream", _vp), ("c_xp", C.c_int), ("unit_stream", _vp), ("trunk_keep_stride", C.c_int),
    ]


class Debug(C.Structure):
    """hmmr_debug_t: development switches, all zero = product defaults."""
    _fields_ = [("stem_route", C.c_int), ("stem_no_conv1", C.c_int), ("gemm_probe", C.c_int), ("smpl_blend_mfma", C.c_int), ("ief_no_group", C.c_int), ("reserved", C.c_int * 2), ("keep_dead_rows", C.c_int),
                ("pair_min_pixels", C.c_int), ("pair_two_tile_min", C.c_int), ("pair_form", C.c_int)]


class LaunchCounts(C.Structure):
    """hmmr_launch_counts_t: how often each fused-unit kernel was launched since the last clear."""
    _fields_ = [("unit_pair", C.c_ulonglong), ("b1_unit", C.c_ulonglong), ("tail_split", C.c_ulonglong), ("conv3x3_stream", C.c_ulonglong),
                ("conv1x1_stream", C.c_ulonglong)]


class StemCounts(C.Structure):
    """hmmr_stem_counts_t: the stem's launches since the last clear (one pass: fused OR fused_conv1, or repack + gemm + pool)."""
    _fields_ = [(k, C.c_ulonglong) for k in ("fused", "fused_conv1", "repack", "gemm", "pool")]


TILE_GENERIC, TILE_PATCH, TILE_STREAM_3X3, TILE_STREAM_1X1 = range(4)
CONV_TILE_MAX = 63       # HMMR_CONV_TILE_MAX: tile numbers are 1 .. this


class ConvTileInfo(C.Structure):
    """hmmr_conv_tile_info_t: one row of the tile list (csrc/conv_tiles.h)."""
    _fields_ = [(k, C.c_int) for k in ("tile", "family", "fm", "fn", "wgm", "wgn", "pixels", "channels", "row_blocks", "depth", "occupancy", "wmax",
                                       "split_only", "conv3_form", "cols", "tune_cols", "narrow", "rank", "candidate")] + [("text", C.c_char_p)]


class Layer(C.Structure):
    _fields_ = [("w", _vp), ("scale", _fp), ("shift", _fp), ("tile", C.c_int), ("k_order", C.c_int)]


class ResnetUnit(C.Structure):
    _fields_ = [("conv1", Layer), ("conv2", Layer), ("conv3", Layer), ("shortcut", Layer), ("c3sc", Layer), ("sc_c1", Layer),
                ("w3_frag", _vp), ("w1n_frag", _vp), ("pair_stream", _vp), ("conv1_frag", _vp), ("unit_stream", _vp), ("pre_scale", _fp), ("pre_shift", _fp),
                ("c_in", C.c_int), ("base", C.c_int), ("depth", C.c_int), ("stride", C.c_int),
                ("fuse_preact", C.c_int), ("fuse_tail", C.c_int)]


class ResnetWeights(C.Structure):
    _fields_ = [("dtype", C.c_int), ("stem", Layer),
                ("unit", ResnetUnit * RESNET_UNITS), ("post_scale", _fp), ("post_shift", _fp)]


SC_NONE, SC_LAUNCH, SC_LAUNCH_WITH_CONV1, SC_IN_CONV3, SC_IN_TAIL = range(5)
CONV1_LAUNCH, CONV1_READY = range(2)
CONV2_LAUNCH, CONV2_IN_TAIL = range(2)
END_CONV3_LAUNCH, END_TAIL_BF16, END_TAIL_BF16_STRIDE2, END_TAIL_SPLIT, END_B1_UNIT, END_UNIT_PAIR = range(6)


class UnitPlan(C.Structure):
    """hmmr_unit_plan_t: what hmmr_resnet50_fwd launches for one unit (hmmr_resnet50_plan; host only)"""
    _fields_ = [(k, C.c_int) for k in ("shortcut", "conv1", "conv2", "end", "reads_fused_preact", "writes_raw", "writes_pre",
                                       "pair_demoted", "swaps_t1_t2", "leaves_h1", "trunk_keep_stride")]


def resnet_plan(rw, n_total):
    """[UnitPlan] * 16 for a pass of n_total frames over the packed table `rw` under the current hmmr_debug_t."""
    plan = (UnitPlan * RESNET_UNITS)()
    check(load().hmmr_resnet50_plan(C.byref(rw), int(n_total), plan), "hmmr_resnet50_plan")
    return list(plan)


class TemporalBlock(C.Structure):
    _fields_ = [("gn1_gamma", _fp), ("gn1_beta", _fp), ("conv1", Layer),
                ("gn2_gamma", _fp), ("gn2_beta", _fp), ("conv2", Layer)]


class TemporalWeights(C.Structure):
    _fields_ = [("dtype", C.c_int), ("num_blocks", C.c_int), ("block", TemporalBlock * MAX_TEMPORAL_BLOCKS)]


class HallucinatorWeights(C.Structure):
    _fields_ = [("dtype", C.c_int), ("fc1", Layer), ("fc2", Layer), ("fc3", Layer)]


class IefRegressor(C.Structure):
    _fields_ = [("nd", C.c_int), ("fc1_phi", Layer), ("fc1_theta", Layer), ("fc2", Layer), ("fc3", Layer)]


class IefWeights(C.Structure):
    _fields_ = [("dtype", C.c_int), ("num_regressors", C.c_int), ("num_stages", C.c_int),
                ("reg", IefRegressor * MAX_REGRESSORS), ("mean_theta", _fp),
                ("no_optcam", C.c_int), ("delta_from_start", C.c_int)]


class IefRegGrads(C.Structure):
    """hmmr_ief_reg_grads_t: one regressor's gradients in the layouts of the HMMR_F32 bank (csrc/ief_grad.hip); each may be NULL"""
    _fields_ = [(k, _fp) for k in ("d_fc1_phi", "d_fc1_theta", "d_fc2", "d_fc3", "d_b1", "d_b2", "d_b3")]


class IefBwdDesc(C.Structure):
    """hmmr_ief_bwd_desc_t: one call of the IEF backward"""
    _fields_ = [("strips", _fp), ("omega_start", _fp), ("keep", _vp), ("keep_scale", C.c_float), ("m", C.c_int), ("d_omegas", _fp),
                ("d_strips", _fp), ("d_omega_start", _fp), ("reg", IefRegGrads * MAX_REGRESSORS)]


TEMPORAL_GRAD_NAMES = ("gn1_gamma", "gn1_beta", "conv1", "b1", "gn2_gamma", "gn2_beta", "conv2", "b2")
HALLUCINATOR_GRAD_NAMES = ("fc1", "fc2", "fc3", "b1", "b2", "b3")


class TemporalBlockGrads(C.Structure):
    """hmmr_temporal_block_grads_t: one temporal block's gradients in the layouts of the HMMR_F32 bank (csrc/movie_grad.hip); each may be NULL"""
    _fields_ = [("d_" + k, _fp) for k in TEMPORAL_GRAD_NAMES]


class TemporalBwdDesc(C.Structure):
    """hmmr_temporal_bwd_desc_t: one call of the temporal encoder's backward"""
    _fields_ = [("phi", _fp), ("b", C.c_int), ("t", C.c_int), ("d_strips", _fp), ("d_phi", _fp),
                ("block", TemporalBlockGrads * MAX_TEMPORAL_BLOCKS)]


class HallucinatorBwdDesc(C.Structure):
    """hmmr_hallucinator_bwd_desc_t: one call of the hallucinator's backward"""
    _fields_ = [("phi", _fp), ("m", C.c_int), ("d_out", _fp), ("d_phi", _fp)] + [("d_" + k, _fp) for k in HALLUCINATOR_GRAD_NAMES]


DISC_POSE_LAYERS = ("conv1", "conv2", "heads", "fc1", "fc2", "fc_out")
DISC_POSE_GRAD_NAMES = ("conv1", "bc1", "conv2", "bc2", "heads", "bj", "fc1", "b1", "fc2", "b2", "fc_out", "bo")


class Rows(C.Structure):
    """hmmr_rows_t: a segment of rows {ptr, ld (floats per row), n}"""
    _fields_ = [("ptr", _fp), ("ld", C.c_int64), ("n", C.c_int)]


class DiscPoseWeights(C.Structure):
    """hmmr_disc_pose_weights_t: the pose discriminator's HMMR_F32 bank (csrc/disc_pose.hip)"""
    _fields_ = [("dtype", C.c_int)] + [(k, Layer) for k in DISC_POSE_LAYERS]


class DiscPoseGrads(C.Structure):
    """hmmr_disc_pose_grads_t: the twelve gradients in the layouts of the bank; each may be NULL"""
    _fields_ = [("d_" + k, _fp) for k in DISC_POSE_GRAD_NAMES]


class DiscPoseBwdDesc(C.Structure):
    """hmmr_disc_pose_bwd_desc_t: one call of the pose discriminator's backward"""
    _fields_ = [("rows_a", Rows), ("rows_b", Rows), ("d_out", _fp), ("d_poses_a", _fp), ("ld_a", C.c_int64), ("d_poses_b", _fp),
                ("ld_b", C.c_int64), ("grads", DiscPoseGrads)]


class PosePriorDesc(C.Structure):
    """hmmr_pose_prior_desc_t: the closed loop of one step (losses, d_rs_fake, the gradients of w_d * d_pose)"""
    _fields_ = [("real", Rows), ("fake", Rows), ("w_e", C.c_float), ("w_d", C.c_float), ("losses", _fp), ("d_rs_fake", _fp),
                ("grads", DiscPoseGrads)]


class SmplConsts(C.Structure):
    _fields_ = [("num_verts", C.c_int), ("num_kps", C.c_int), ("lbs_nnz", C.c_int), ("vpad", C.c_int),
                ("dirs", _fp), ("j_template", _fp), ("j_shapedirs", _fp), ("parents", _ip),
                ("lbs_idx", _ip), ("lbs_w", _fp), ("kreg_ptr", _ip), ("kreg_idx", _ip), ("kreg_val", _fp),
                ("dirs_split", _vp)]


class SmplGradConsts(C.Structure):
    """hmmr_smpl_grad_consts_t: what hmmr_smpl_bwd needs beside SmplConsts (the keypoint regressor by vertex)"""
    _fields_ = [("num_verts", C.c_int), ("num_kps", C.c_int), ("vk_ptr", _ip), ("vk_idx", _ip), ("vk_val", _fp)]


LOSS_KP, LOSS_KP_OPTCAM, LOSS_JOINTS, LOSS_SMPL, LOSS_CONST, LOSS_SHAPE_PRIOR = 1, 2, 4, 8, 16, 32      # hmmr_seq_loss_desc_t.flags
LOSS_NAMES = ("e_kp", "e_joints", "e_smpl_pose", "e_smpl_shape", "e_const", "e_shape", "total")              # losses[0..6] (HMMR_L_*)
LOSS_NO_VISIBLE, LOSS_NOT_FINITE = 1, 2


class SeqLossDesc(C.Structure):
    """hmmr_seq_loss_desc_t: one call of the trainer's loss stage (csrc/losses.hip)"""
    _fields_ = [("B", C.c_int), ("T", C.c_int), ("K", C.c_int), ("delta_t", C.c_int), ("flags", C.c_uint), ("weights", C.c_float * 6),
                ("kps_pred", _fp), ("joints_pred", _fp), ("rs_pred", _fp), ("beta_pred", _fp), ("ld_beta", C.c_int),
                ("kps_gt", _fp), ("joints_gt", _fp), ("rs_gt", _fp), ("shapes_gt", _fp), ("has_gt3d_smpl", _fp), ("has_gt3d_joints", _fp),
                ("losses", _fp), ("d_kps", _fp), ("d_joints", _fp), ("d_rs", _fp), ("d_beta", _fp), ("best_cam", _fp), ("status", _vp),
                ("ws", _vp), ("ws_bytes", C.c_size_t)]


class AdamSeg(C.Structure):
    """hmmr_adam_seg_t: one tensor of a TF Adam step (csrc/adam.hip); g NULL or n 0 = skipped"""
    _fields_ = [("p", _fp), ("g", _fp), ("m", _fp), ("v", _fp), ("n", C.c_longlong)]


class AdamHyper(C.Structure):
    """hmmr_adam_hyper_t: the hyper-parameters of a step; the beta powers are the caller's float32 products"""
    _fields_ = [(k, C.c_float) for k in ("lr", "beta1", "beta2", "eps", "beta1_power", "beta2_power")]


class Var(C.Structure):
    """hmmr_var_t: one checkpoint variable for the C-side packers (csrc/pack.cpp)"""
    _fields_ = [("name", C.c_char_p), ("data", _fp), ("numel", C.c_int64)]


class SmplSource(C.Structure):
    """hmmr_smpl_source_t: the body model in the src/tf_smpl layout"""
    _fields_ = [("num_verts", C.c_int), ("num_kps", C.c_int), ("v_template", _fp), ("shapedirs", _fp), ("posedirs", _fp),
                ("J_regressor", _fp), ("lbs_weights", _fp), ("kp_regressor", _fp), ("parents", _ip)]


class VideoPlan(C.Structure):
    """hmmr_video_plan_t: the sliding-window plan of a whole-video call (csrc/video_plan.cpp; host only)"""
    _fields_ = [(k, C.c_int) for k in ("n", "T", "fov", "margin", "g", "n_windows", "max_frames", "max_windows", "resnet_passes", "tail_passes")]


class TracksPlan(C.Structure):
    """hmmr_tracks_plan_t: the plan of a call over several tracks laid end to end (csrc/video_plan.cpp; host only).  Track k holds
    frames [off[k], off[k + 1]) and ceil(n_k / g) windows; windows are numbered globally, track after track; slot t of local window lw
    holds frame lw g + t - margin of ITS track or the zero image, and its slots margin .. margin + g - 1 are the track's output rows
    off[k] + lw g .. (include/hmmr_hip.h)"""
    _fields_ = [(k, C.c_int) for k in ("n_tracks", "T", "fov", "margin", "g", "n_frames", "n_windows", "max_frames", "max_windows",
                                       "resnet_passes", "tail_passes")]


class Model(C.Structure):
    """hmmr_model_t: the packed stages of one model, as hmmr_predict_video reads them"""
    _fields_ = [("resnet", C.POINTER(ResnetWeights)), ("temporal", C.POINTER(TemporalWeights)), ("hallucinator", C.POINTER(HallucinatorWeights)),
                ("ief", C.POINTER(IefWeights)), ("smpl", C.POINTER(SmplConsts)), ("sequence_length", C.c_int), ("fov", C.c_int)]


RENDER_MAX_FRAMES, RENDER_MIN_SIZE, RENDER_MAX_SIZE, RENDER_MAX_FACES = 4096, 16, 1024, 65536
RENDER_BG_COLOR, RENDER_BG_FLOAT, RENDER_BG_FRAME = 0, 1, 2
# hmmr_track_* (csrc/track.hip): limits, the gap scan's step, the status bits of hmmr_track_crop_geom
TRACK_MAX_KPS, TRACK_MAX_KERNEL, TRACK_MAX_RADIUS, TRACK_MAX_ROWS, TRACK_TILE = 64, 31, 64, 1 << 27, 256
TRACK_EMPTY, TRACK_BEFORE_ORIGIN, TRACK_CLIPPED, TRACK_NOT_FINITE = 1, 2, 4, 8
# hmmr_video_bbox (csrc/person_view.hip): the status bits of a track's box
BBOX_EMPTY, BBOX_NOT_FINITE, BBOX_DEGENERATE, BBOX_BEYOND_START = 1, 2, 4, 8


class RenderDesc(C.Structure):
    """hmmr_render_desc_t: one call of the rasteriser (csrc/render.hip)"""
    _fields_ = [("verts", _fp), ("ld_verts", C.c_int64), ("cams", _fp), ("ld_cam", C.c_int64), ("geom", _fp),
                ("faces", _ip), ("face_colors", _fp), ("ld_face_colors", C.c_int64),
                ("n", C.c_int), ("nv", C.c_int), ("nf", C.c_int), ("size", C.c_int),
                ("rotate", C.c_int), ("rot", C.c_float * 9), ("color", C.c_float * 3), ("bg_color", C.c_float * 3),
                ("light_dir", C.c_float * 3), ("light_int_ambient", C.c_float), ("light_int_directional", C.c_float),
                ("light_color_ambient", C.c_float * 3), ("light_color_directional", C.c_float * 3),
                ("bg_mode", C.c_int), ("bg_image", _vp), ("bg_add", C.c_float), ("bg_mul", C.c_float),
                ("frame_h", C.c_int), ("frame_w", C.c_int), ("out_h", C.c_int), ("out_w", C.c_int),
                ("rgb", _vp), ("alpha", _fp), ("face_index", _ip), ("ws", _vp), ("ws_bytes", C.c_size_t)]


SCENE_MAX_TRACKS = 16


class SceneTrack(C.Structure):
    """hmmr_scene_track_t: one person track of the scene view (csrc/render.hip)"""
    _fields_ = [("verts", _fp), ("ld_verts", C.c_int64), ("cams", _fp), ("ld_cam", C.c_int64), ("geom", _fp),
                ("priority", _fp), ("start", C.c_int), ("end", C.c_int), ("color", C.c_float * 3)]


class SceneDesc(C.Structure):
    """hmmr_scene_desc_t: one call of the scene view (csrc/render.hip)"""
    _fields_ = [("tracks", C.POINTER(SceneTrack)), ("n_tracks", C.c_int), ("faces", _ip),
                ("nv", C.c_int), ("nf", C.c_int), ("n_frames", C.c_int), ("size", C.c_int),
                ("out_h", C.c_int), ("out_w", C.c_int), ("bg_color", C.c_float * 3),
                ("light_dir", C.c_float * 3), ("light_int_ambient", C.c_float), ("light_int_directional", C.c_float),
                ("light_color_ambient", C.c_float * 3), ("light_color_directional", C.c_float * 3),
                ("bg_mode", C.c_int), ("bg_image", _vp), ("frame_h", C.c_int), ("frame_w", C.c_int),
                ("rgb", _vp), ("alpha", _fp), ("face_index", _ip), ("owner", _ip), ("ws", _vp), ("ws_bytes", C.c_size_t)]


SKELETON_MAX_RADIUS, COLLAGE_MAX_PANEL_WIDTH = 1024, 4096


class SkeletonDesc(C.Structure):
    """hmmr_skeleton_desc_t: one call of the skeleton panel (csrc/collage.hip)"""
    _fields_ = [("kps", _fp), ("ld_kps", C.c_int64), ("vis", _vp), ("n", C.c_int), ("nk", C.c_int), ("h", C.c_int), ("w", C.c_int),
                ("kp_add", C.c_float), ("kp_mul", C.c_float), ("draw_edges", C.c_int), ("radius", C.c_int),
                ("bg_float", _fp), ("bg_add", C.c_float), ("bg_mul", C.c_float), ("bg_u8", _vp), ("out", _vp)]


class CollageDesc(C.Structure):
    """hmmr_collage_desc_t: one call of the 2x2 collage (csrc/collage.hip)"""
    _fields_ = [("rend_crop", _vp), ("skel_crop", _vp), ("render_og", _vp), ("rot_og", _vp),
                ("n", C.c_int), ("S", C.c_int), ("h", C.c_int), ("w", C.c_int), ("out", _vp)]


# name -> (restype, argtypes); mirrors include/hmmr_hip.h one to one
SIGNATURES = {
    "hmmr_abi_version": (C.c_int, []),
    "hmmr_pack_resnet_bytes": (C.c_size_t, [C.POINTER(Var), C.c_int, C.c_int]),
    "hmmr_pack_resnet": (C.c_int, [C.POINTER(Var), C.c_int, C.c_int, _vp, C.c_size_t, _vp, C.POINTER(ResnetWeights)]),
    "hmmr_pack_temporal_bytes": (C.c_size_t, [C.POINTER(Var), C.c_int, C.c_int, C.c_int]),
    "hmmr_pack_temporal": (C.c_int, [C.POINTER(Var), C.c_int, C.c_int, C.c_int, _vp, C.c_size_t, _vp, C.POINTER(TemporalWeights)]),
    "hmmr_pack_hallucinator_bytes": (C.c_size_t, [C.POINTER(Var), C.c_int, C.c_int]),
    "hmmr_pack_hallucinator": (C.c_int, [C.POINTER(Var), C.c_int, C.c_int, _vp, C.c_size_t, _vp, C.POINTER(HallucinatorWeights)]),
    "hmmr_pack_ief_bytes": (C.c_size_t, [C.POINTER(Var), C.c_int, C.c_int, C.POINTER(C.c_int), C.c_int]),
    "hmmr_pack_ief": (C.c_int, [C.POINTER(Var), C.c_int, C.c_int, C.POINTER(C.c_int), C.c_int, C.c_int, _vp, C.c_size_t, _vp, C.POINTER(IefWeights)]),
    "hmmr_pack_smpl_bytes": (C.c_size_t, [C.POINTER(SmplSource), C.c_int, C.c_int]),
    "hmmr_pack_smpl": (C.c_int, [C.POINTER(SmplSource), C.c_int, C.c_int, _vp, C.c_size_t, _vp, C.POINTER(SmplConsts)]),
    "hmmr_pack_smpl_grad_bytes": (C.c_size_t, [C.POINTER(SmplSource), C.c_int]),
    "hmmr_pack_smpl_grad": (C.c_int, [C.POINTER(SmplSource), C.c_int, _vp, C.c_size_t, _vp, C.POINTER(SmplGradConsts)]),
    "hmmr_last_error": (C.c_char_p, []),
    "hmmr_run_flags": (C.c_int, [C.POINTER(C.c_uint), C.c_int]),
    "hmmr_set_debug": (None, [C.POINTER(Debug)]),
    "hmmr_get_debug": (None, [C.POINTER(Debug)]),
    "hmmr_launch_counts": (None, [C.POINTER(LaunchCounts), C.c_int]),
    "hmmr_stem_launch_counts": (None, [C.POINTER(StemCounts), C.c_int]),
    "hmmr_conv_gemm": (C.c_int, [C.POINTER(ConvDesc), _vp]),
    "hmmr_conv_tile_info": (C.c_int, [C.c_int, C.POINTER(ConvTileInfo)]),
    "hmmr_conv_tile_for": (C.c_int, [C.c_int] * 6),
    "hmmr_conv_tile_fits": (C.c_int, [C.c_int] * 8),
    "hmmr_conv_tile_f_movie": (C.c_int, []),
    "hmmr_conv_splitk_workspace_bytes": (C.c_size_t, [C.c_int, C.c_int, C.c_int]),
    "hmmr_resnet50_workspace_bytes": (C.c_size_t, [C.c_int, C.c_int]),
    "hmmr_resnet50_fwd": (C.c_int, [C.POINTER(ResnetWeights), _fp, C.c_int, C.c_int, _fp, _vp, C.c_size_t, _vp,
                                    C.POINTER(C.c_float)]),
    "hmmr_resnet50_stem_workspace_bytes": (C.c_size_t, [C.POINTER(ResnetWeights), C.c_int]),
    "hmmr_resnet50_stem": (C.c_int, [C.POINTER(ResnetWeights), _fp, C.c_int, C.c_int, _vp, _vp, C.POINTER(C.c_int), _vp, C.c_size_t, _vp]),
    "hmmr_resnet50_plan": (C.c_int, [C.POINTER(ResnetWeights), C.c_int, C.POINTER(UnitPlan)]),
    "hmmr_temporal_workspace_bytes": (C.c_size_t, [C.c_int, C.c_int, C.c_int]),
    "hmmr_temporal_fwd": (C.c_int, [C.POINTER(TemporalWeights), _fp, C.c_int, C.c_int, _fp, _vp, C.c_size_t, _vp]),
    "hmmr_hallucinator_workspace_bytes": (C.c_size_t, [C.c_int, C.c_int]),
    "hmmr_hallucinator_fwd": (C.c_int, [C.POINTER(HallucinatorWeights), _fp, C.c_int, _fp, _vp, C.c_size_t, _vp]),
    "hmmr_groupnorm_relu": (C.c_int, [_fp, _fp, _fp, C.c_int, C.c_int, C.c_int, C.c_int, _vp, C.c_int, _vp]),
    "hmmr_ief_workspace_bytes": (C.c_size_t, [C.c_int, C.c_int, C.c_int]),
    "hmmr_ief_fwd": (C.c_int, [C.POINTER(IefWeights), _fp, C.c_int, _fp, _vp, C.c_size_t, _vp]),
    "hmmr_ief_fwd_from": (C.c_int, [C.POINTER(IefWeights), _fp, _fp, C.c_int, _fp, _vp, C.c_size_t, _vp]),
    "hmmr_ief_bwd_workspace_bytes": (C.c_size_t, [C.c_int, C.c_int, C.c_int]),
    "hmmr_ief_fwd_train": (C.c_int, [C.POINTER(IefWeights), _fp, _fp, _vp, C.c_float, C.c_int, _fp, _vp, C.c_size_t, _vp]),
    "hmmr_ief_bwd": (C.c_int, [C.POINTER(IefWeights), C.POINTER(IefBwdDesc), _vp, C.c_size_t, _vp]),
    "hmmr_temporal_bwd_workspace_bytes": (C.c_size_t, [C.c_int, C.c_int, C.c_int]),
    "hmmr_temporal_bwd": (C.c_int, [C.POINTER(TemporalWeights), C.POINTER(TemporalBwdDesc), _vp, C.c_size_t, _vp]),
    "hmmr_hallucinator_bwd_workspace_bytes": (C.c_size_t, [C.c_int]),
    "hmmr_hallucinator_bwd": (C.c_int, [C.POINTER(HallucinatorWeights), C.POINTER(HallucinatorBwdDesc), _vp, C.c_size_t, _vp]),
    "hmmr_pack_disc_pose_bytes": (C.c_size_t, [C.POINTER(Var), C.c_int, C.c_int]),
    "hmmr_pack_disc_pose": (C.c_int, [C.POINTER(Var), C.c_int, C.c_int, _vp, C.c_size_t, _vp, C.POINTER(DiscPoseWeights)]),
    "hmmr_disc_pose_workspace_bytes": (C.c_size_t, [C.c_int]),
    "hmmr_disc_pose_fwd": (C.c_int, [C.POINTER(DiscPoseWeights), C.POINTER(Rows), C.POINTER(Rows), _fp, _vp, C.c_size_t, _vp]),
    "hmmr_disc_pose_bwd": (C.c_int, [C.POINTER(DiscPoseWeights), C.POINTER(DiscPoseBwdDesc), _vp, C.c_size_t, _vp]),
    "hmmr_pose_prior": (C.c_int, [C.POINTER(DiscPoseWeights), C.POINTER(PosePriorDesc), _vp, C.c_size_t, _vp]),
    "hmmr_smpl_workspace_bytes": (C.c_size_t, [C.c_int]),
    "hmmr_smpl_fwd": (C.c_int, [C.POINTER(SmplConsts), _fp, C.c_int, _fp, C.c_int, _fp, C.c_int, C.c_int,
                                _fp, _fp, _fp, _fp, _vp, C.c_size_t, _vp]),
    "hmmr_smpl_bwd_workspace_bytes": (C.c_size_t, [C.POINTER(SmplConsts), C.c_int]),
    "hmmr_smpl_bwd": (C.c_int, [C.POINTER(SmplConsts), C.POINTER(SmplGradConsts), _fp, C.c_int, _fp, C.c_int, _fp, C.c_int, _fp, C.c_int,
                                _fp, _fp, _fp, _fp, _fp, _fp, _fp, _vp, C.c_size_t, _vp]),
    "hmmr_seq_losses_workspace_bytes": (C.c_size_t, [C.c_int, C.c_int]),
    "hmmr_seq_losses": (C.c_int, [C.POINTER(SeqLossDesc), _vp]),
    "hmmr_omega_loss_grad_workspace_bytes": (C.c_size_t, [C.POINTER(SmplConsts), C.c_int, C.c_int]),
    "hmmr_omega_loss_grad": (C.c_int, [C.POINTER(SmplConsts), C.POINTER(SmplGradConsts), C.POINTER(SeqLossDesc), _fp, C.c_int, _fp, _fp,
                                       _vp, C.c_size_t, _vp]),
    "hmmr_strip_mse_workspace_bytes": (C.c_size_t, [C.c_int]),
    "hmmr_strip_mse": (C.c_int, [_fp, C.c_longlong, _fp, C.c_longlong, C.c_int, C.c_int, C.c_float, _fp, _fp, C.c_longlong, _fp, C.c_longlong,
                                 _vp, C.c_size_t, _vp]),
    "hmmr_adam_step": (C.c_int, [C.POINTER(AdamSeg), C.c_int, C.POINTER(AdamHyper), _vp]),
    "hmmr_crop_frames": (C.c_int, [_vp, _ip, C.c_int, C.c_int, C.c_int, _fp, _vp]),
    "hmmr_tube_augment": (C.c_int, [_vp, C.c_int, C.c_int, C.c_int, C.c_int, _ip, _vp, _fp, C.c_int, _fp, _vp]),
    "hmmr_track_workspace_bytes": (C.c_size_t, [C.c_int, C.c_int]),
    "hmmr_track_bbox": (C.c_int, [_fp, _vp, C.POINTER(C.c_int32), C.c_int, C.c_int, C.c_double, C.c_int, C.POINTER(C.c_double), C.c_int,
                                  _fp, _fp, _ip, _vp, C.c_size_t, _vp]),
    "hmmr_track_smooth": (C.c_int, [_fp, C.POINTER(C.c_int32), C.c_int, C.c_int, C.POINTER(C.c_double), C.c_int, _fp, _vp, C.c_size_t, _vp]),
    "hmmr_track_crop_geom": (C.c_int, [_fp, C.POINTER(C.c_int32), _ip, C.c_int, C.c_int, C.c_int, _ip, _fp, _ip, _vp]),
    "hmmr_bottleneck_tail": (C.c_int, [C.POINTER(TailDesc), _vp]),
    "hmmr_pair_stream_bytes": (C.c_size_t, [C.c_int, C.c_int, C.c_int]),
    "hmmr_b1_unit_stream_bytes": (C.c_size_t, [C.c_int]),
    "hmmr_trunk_keep_launches": (C.c_ulonglong, [C.c_int]),
    "hmmr_conv3x3_stream_bytes": (C.c_size_t, [C.c_int, C.c_int]),
    "hmmr_conv1x1_stream_bytes": (C.c_size_t, [C.c_int, C.c_int]),
    "hmmr_mfma_rate_probe": (C.c_int, [C.c_int, C.c_int, _fp, _vp]),
    "hmmr_clock_probe": (C.c_int, [_vp, C.c_int, C.c_int, _vp, _vp]),
    "hmmr_render_handoff": (C.c_int, [_fp, C.c_int64, _fp, C.c_int64, _fp, C.c_int64, _fp, C.c_int, C.c_int, C.c_int,
                                      _fp, _fp, _fp, _vp]),
    "hmmr_render_workspace_bytes": (C.c_size_t, [C.c_int, C.c_int, C.c_int]),
    "hmmr_render_mesh": (C.c_int, [C.POINTER(RenderDesc), _vp]),
    "hmmr_render_scene_workspace_bytes": (C.c_size_t, [C.c_int, C.c_int, C.c_int, C.c_int]),
    "hmmr_render_scene": (C.c_int, [C.POINTER(SceneDesc), _vp]),
    "hmmr_video_bbox": (C.c_int, [_fp, C.c_longlong, _fp, C.c_longlong, C.c_int, _fp, C.c_double, C.POINTER(C.c_int32), C.c_int, C.c_int, C.c_int,
                                  C.c_double, _ip, _fp, _ip, _vp]),
    "hmmr_skeleton_radius": (C.c_int, [C.c_int, C.c_int]),
    "hmmr_draw_skeleton": (C.c_int, [C.POINTER(SkeletonDesc), _vp]),
    "hmmr_collage_width": (C.c_int, [C.c_int, C.c_int, C.c_int]),
    "hmmr_compose_collage": (C.c_int, [C.POINTER(CollageDesc), _vp]),
    "hmmr_eval_joints": (C.c_int, [_fp, _fp, C.c_int, C.c_int, C.c_int, C.c_int, _fp, _fp, _fp, _fp, _vp]),
    "hmmr_eval_verts": (C.c_int, [_fp, C.c_int64, _fp, C.c_int64, C.c_int, C.c_int, _fp, _vp]),
    "hmmr_eval_joints_ld": (C.c_int, [_fp, C.c_int64, _fp, C.c_int64, C.c_int, C.c_int, C.c_int, C.c_int, _fp, _fp, _fp, _fp, _vp]),
    "hmmr_eval_kps": (C.c_int, [_fp, C.c_int64, _fp, C.c_int64, C.c_int, C.c_int, C.c_double, C.c_int, C.c_float,
                                _fp, _fp, _fp, _fp, _vp]),
    "hmmr_rotmat_to_axis_angle": (C.c_int, [_fp, C.c_int64, C.c_int, C.c_int, _fp, C.c_int64, _vp]),
    "hmmr_axis_angle_to_rotmat": (C.c_int, [_fp, C.c_int64, C.c_int, C.c_int, _fp, C.c_int64, _vp]),
    "hmmr_global_rigid_transformation": (C.c_int, [_fp, _fp, _ip, C.c_int, _fp, _fp, C.c_int, _vp]),
    "hmmr_smpl_fwd_records": (C.c_int, [C.POINTER(SmplConsts), _fp, C.c_int, C.c_int, _fp, C.c_int64, C.POINTER(C.c_int32),
                                        _vp, C.c_size_t, _vp]),
    "hmmr_smpl_fwd_strided": (C.c_int, [C.POINTER(SmplConsts), _fp, C.c_int, _fp, C.c_int, _fp, C.c_int, C.c_int,
                                        _fp, _fp, _fp, _fp, C.c_int64, _vp, C.c_size_t, _vp]),
    "hmmr_video_plan": (C.c_int, [C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.POINTER(VideoPlan)]),
    "hmmr_record_layout": (C.c_int, [C.c_int, C.c_int, C.c_int, C.POINTER(C.c_int32), C.POINTER(C.c_int64)]),
    "hmmr_gather_windows": (C.c_int, [_fp, C.c_int, _fp, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, _fp, _vp]),
    "hmmr_keep_rows": (C.c_int, [_fp, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, _fp, C.c_int64, _vp]),
    "hmmr_predict_video_workspace_bytes": (C.c_size_t, [C.POINTER(Model), C.c_int, C.c_int, C.c_int]),
    "hmmr_predict_video": (C.c_int, [C.POINTER(Model), _fp, C.c_int, _fp, C.c_int64, C.POINTER(C.c_int32), C.c_int, C.c_int,
                                     _vp, C.c_size_t, _vp]),
    "hmmr_tracks_plan": (C.c_int, [C.POINTER(C.c_int32), C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.POINTER(TracksPlan)]),
    "hmmr_tracks_window_owner": (C.c_int, [C.POINTER(C.c_int32), C.c_int, C.c_int, C.c_int, C.POINTER(C.c_int), C.POINTER(C.c_int)]),
    "hmmr_tracks_window_rows": (C.c_int, [C.POINTER(C.c_int32), C.c_int, C.c_int, C.c_int, C.c_int, C.POINTER(C.c_int), C.POINTER(C.c_int)]),
    "hmmr_tracks_tail_pass": (C.c_int, [C.POINTER(C.c_int32), C.c_int, C.POINTER(TracksPlan), C.c_int, C.POINTER(C.c_int), C.POINTER(C.c_int),
                                        C.POINTER(C.c_int), C.POINTER(C.c_int)]),
    "hmmr_gather_windows_tracks": (C.c_int, [_fp, _fp, C.POINTER(C.c_int32), C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, _fp, _vp]),
    "hmmr_keep_rows_tracks": (C.c_int, [_fp, C.POINTER(C.c_int32), C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, _fp, C.c_int64,
                                        _vp]),
    "hmmr_predict_tracks_workspace_bytes": (C.c_size_t, [C.POINTER(Model), C.POINTER(C.c_int32), C.c_int, C.c_int, C.c_int]),
    "hmmr_predict_tracks": (C.c_int, [C.POINTER(Model), _fp, C.POINTER(C.c_int32), C.c_int, _fp, C.c_int64, C.POINTER(C.c_int32), C.c_int, C.c_int,
                                      _vp, C.c_size_t, _vp]),
}

_lib = None


class HmmrError(RuntimeError):
    pass


def load():
    """Load libhmmr_hip.so and bind every symbol of the header.  Raises if the
    library is missing -- there is deliberately no fallback path."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise HmmrError("%s not found: build it with `python -m human_dynamics_amd.build` "
                        "(the HIP library is mandatory; there is no CPU fallback)" % LIB_PATH)
    # PyTorch-ROCm ships its own HIP runtime (torch/lib/libamdhip64.so).  Import
    # torch FIRST so that libhmmr_hip.so binds to that already-loaded runtime
    # (same soname) -- two HIP runtimes in one process cannot see each other's
    # streams, allocations or code objects.
    import torch  # noqa: F401
    if torch.cuda.is_available():
        torch.cuda.init()
    lib = C.CDLL(LIB_PATH)
    for name, (res, args) in SIGNATURES.items():
        fn = getattr(lib, name)      # AttributeError if the .so does not export it
        fn.restype, fn.argtypes = res, args
    if lib.hmmr_abi_version() != ABI_VERSION:
        raise HmmrError("libhmmr_hip.so ABI version mismatch")
    _lib = lib
    return lib


def launch_counts(clear=False):
    """{kernel family: launches since the last clear} (hmmr_launch_counts)."""
    c = LaunchCounts()
    load().hmmr_launch_counts(C.byref(c), int(bool(clear)))
    return {k: int(getattr(c, k)) for k, _ in LaunchCounts._fields_}


def conv_tiles(family=None):
    """[ConvTileInfo] of every value hmmr_conv_desc_t.tile takes, or of one family's (TILE_*), by number (hmmr_conv_tile_info)."""
    lib, rows = load(), []
    for t in range(1, CONV_TILE_MAX + 1):
        r = ConvTileInfo()
        if lib.hmmr_conv_tile_info(t, C.byref(r)) == 0 and family in (None, r.family):
            rows.append(r)
    return rows


def stem_launch_counts(clear=False):
    """{fused, fused_conv1, repack, gemm, pool: the stem's launches since the last clear} (hmmr_stem_launch_counts)."""
    c = StemCounts()
    load().hmmr_stem_launch_counts(C.byref(c), int(bool(clear)))
    return {k: int(getattr(c, k)) for k, _ in StemCounts._fields_}


def check(rc, what=""):
    if rc != 0:
        msg = load().hmmr_last_error()
        raise HmmrError("%s failed (%d): %s" % (what or "hmmr call", rc, msg.decode() if msg else "?"))


def ptr(t):
    """Device pointer of a torch tensor (or None) as a ctypes-compatible int."""
    return None if t is None else t.data_ptr()
