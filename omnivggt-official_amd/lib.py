"""ctypes binding of libomnivggt_hip.so (the C ABI declared in include/omnivggt_hip.h).

This is the ONLY way the Python host reaches compute: there is no eager/PyTorch
fallback.  Importing this module never needs a GPU (the library loads on a CPU-only
host so the symbol table can be checked); calling a kernel without one fails loudly.
"""
import ctypes as C
import os

HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(HERE, "libomnivggt_hip.so")

OVG_BF16, OVG_F16, OVG_F32, OVG_F16X2 = 0, 1, 2, 3
EPI_STORE, EPI_GELU, EPI_RES, EPI_PATCH = 0, 1, 2, 3
OVG_MAX_SEG = 8
KV_TILE = 64
ABI_VERSION = 13
TILE_AUTO, TILE_128, TILE_256 = 0, 1, 2
# ovg_attn_params.variant (OVG_ATTN_* of include/omnivggt_hip.h): 0 = the launch plan chooses; the kernels by name; the plan knobs of the A/B tools
ATTN_AUTO, ATTN_BASELINE = 0, 1
ATTN_SPEC256, ATTN_LAZY256, ATTN_FORCED256, ATTN_SPEC128, ATTN_LAZY128, ATTN_SPEC512 = 50, 52, 53, 54, 55, 57
ATTN_PLAN_ROWTAIL512, ATTN_PLAN_ROWTAIL256, ATTN_PLAN_KEYTAIL256, ATTN_PLAN_KEYTAIL512 = 71, 72, 73, 74
ATTN_F32X_FAST_PV = 92                                         # ovg_attn_params.variant in the split-f16 mode (opt-in): PV without P_lo x V_hi, +16 % at 3e-5 .. 1e-4 instead of 1e-5 .. 5e-5
ATTN_RETIRED = (2, 6, 8, 18, 19, 21, 25, 31, 32, 33, 51, 56, 58, 59)     # the A/B history of rounds 1-4: always OVG_E_UNSUPPORTED
TILE_R02_EPILOGUE, TILE_128X, TILE_256X = 16, 17, 18      # retired selectors (r02 epilogue forms): always OVG_E_UNSUPPORTED

ERRORS = {0: "OVG_OK", -1: "OVG_E_ARG", -2: "OVG_E_DTYPE", -3: "OVG_E_LAUNCH", -4: "OVG_E_UNSUPPORTED"}

vp, i64, i32, f32 = C.c_void_p, C.c_int64, C.c_int, C.c_float


class LayerNormParams(C.Structure):
    _fields_ = [("x", vp), ("ldx", i64), ("y", vp), ("ldy", i64), ("weight", vp), ("bias", vp),
                ("rows", i64), ("eps", f32), ("dtype", i32), ("out_f32", i32), ("y_lo", vp)]


class LinearParams(C.Structure):
    _fields_ = [("x", vp), ("ldx", i64), ("w", vp), ("ldw", i64), ("bias", vp), ("y", vp), ("ldy", i64),
                ("M", i64), ("N", i64), ("K", i64), ("dtype", i32), ("epilogue", i32), ("out_f32", i32),
                ("res", vp), ("ldres", i64), ("gamma", vp), ("inject", vp), ("inj_period", i64),
                ("table", vp), ("p0", i64), ("p1", i64), ("row_off", i64), ("tile", i32),
                ("x_lo", vp), ("w_lo", vp), ("y_lo", vp)]


class QkvParams(C.Structure):
    _fields_ = [("x", vp), ("ldx", i64), ("w", vp), ("bias", vp), ("q", vp), ("k", vp), ("vt", vp),
                ("M", i64), ("seq", i64), ("nq_pad", i64), ("nk_pad", i64), ("dtype", i32),
                ("qk_norm", i32), ("qn_w", vp), ("qn_b", vp), ("kn_w", vp), ("kn_b", vp), ("qk_eps", f32),
                ("rope", i32), ("rope_cos", vp), ("rope_sin", vp), ("max_pos", i32),
                ("tokens_per_view", i64), ("grid_w", i32), ("n_special", i32), ("q_scale", f32), ("part", i32), ("tile", i32),
                ("x_lo", vp), ("w_lo", vp), ("q_lo", vp), ("k_lo", vp), ("vt_lo", vp)]


class KvSegment(C.Structure):
    _fields_ = [("k", vp), ("vt", vp), ("nk", i64), ("nk_pad", i64), ("k_lo", vp), ("vt_lo", vp)]


class AttnParams(C.Structure):
    _fields_ = [("q", vp), ("nq", i64), ("nq_pad", i64), ("seg", KvSegment * OVG_MAX_SEG), ("nseg", i32),
                ("out", vp), ("ldo", i64), ("BH", i64), ("dtype", i32), ("variant", i32),
                ("kv_heads", i32), ("out_bh_stride", i64), ("lse", vp), ("kv_splits", i32), ("ws_part", vp), ("ws_lse", vp),
                ("ws_part_bytes", i64), ("ws_lse_bytes", i64), ("q_lo", vp), ("out_lo", vp), ("fallback_count", vp), ("cus", i32)]


class AttnPlanOut(C.Structure):
    _fields_ = [("splits", i32), ("q_tile", i32), ("part_bytes", i64), ("lse_bytes", i64), ("main_rows", i64), ("tail_q_tile", i32)]


class AttnMergeParams(C.Structure):
    _fields_ = [("a", vp), ("lda", i64), ("lse_a", vp), ("b", vp), ("ldb", i64), ("lse_b", vp),
                ("out", vp), ("ldo", i64), ("rows", i64), ("n_pad", i64), ("dtype", i32), ("a_lo", vp), ("b_lo", vp), ("out_lo", vp)]


class BlockWeights(C.Structure):
    _fields_ = [("n1_w", vp), ("n1_b", vp), ("qkv_w", vp), ("qkv_b", vp),
                ("qn_w", vp), ("qn_b", vp), ("kn_w", vp), ("kn_b", vp),
                ("proj_w", vp), ("proj_b", vp), ("ls1", vp), ("n2_w", vp), ("n2_b", vp),
                ("fc1_w", vp), ("fc1_b", vp), ("fc2_w", vp), ("fc2_b", vp), ("ls2", vp),
                ("qkv_w_lo", vp), ("proj_w_lo", vp), ("fc1_w_lo", vp), ("fc2_w_lo", vp)]


class BlockParams(C.Structure):
    _fields_ = [("w", BlockWeights), ("x_in", vp), ("ld_in", i64), ("x_out", vp), ("ld_out", i64),
                ("M", i64), ("seq", i64), ("BH", i64), ("nq_pad", i64), ("nk_pad", i64),
                ("dtype", i32), ("ln_eps", f32), ("qk_norm", i32), ("rope", i32), ("qk_eps", f32),
                ("rope_cos", vp), ("rope_sin", vp), ("max_pos", i32),
                ("tokens_per_view", i64), ("grid_w", i32), ("n_special", i32),
                ("inject", vp), ("inj_period", i64),
                ("ws_xn", vp), ("ws_q", vp), ("ws_k", vp), ("ws_vt", vp), ("ws_attn", vp), ("ws_hid", vp),
                ("extra", KvSegment * OVG_MAX_SEG), ("nseg_extra", i32), ("local_seg_index", i32),
                ("attn_variant", i32), ("qkv_part", i32), ("ev_attn_start", vp), ("ev_attn_stop", vp),
                ("skip_attention", i32), ("gemm_tile", i32), ("ws_attn_part", vp), ("ws_attn_lse", vp), ("attn_kv_splits", i32),
                ("ws_attn_part_bytes", i64), ("ws_attn_lse_bytes", i64),
                ("ws_xn_lo", vp), ("ws_q_lo", vp), ("ws_k_lo", vp), ("ws_vt_lo", vp), ("ws_attn_lo", vp), ("ws_hid_lo", vp),
                ("attn_fallback_count", vp), ("attn_cus", i32)]


class BlockWorkspace(C.Structure):
    _fields_ = [("xn", i64), ("q", i64), ("k", i64), ("vt", i64), ("attn", i64), ("hid", i64), ("total", i64)]


class PackWeightsParams(C.Structure):
    _fields_ = [("src", vp), ("lds", i64), ("dst", vp), ("ldd", i64), ("rows", i64), ("k", i64), ("k_pad", i64), ("dtype", i32), ("dst_lo", vp)]


class Im2colParams(C.Structure):
    _fields_ = [("img", vp), ("img2", vp), ("out", vp), ("k_pad", i64), ("V", i64), ("C", i32), ("Hpx", i32),
                ("Wpx", i32), ("dtype", i32), ("mode", i32), ("mean", f32 * 3), ("std", f32 * 3),
                ("depth_stats", vp), ("views_per_batch", i64), ("out_lo", vp)]


class DepthStatsParams(C.Structure):
    _fields_ = [("depth", vp), ("mask", vp), ("B", i64), ("n_per_batch", i64), ("stats", vp), ("partial", vp),
                ("nblocks", i32)]


class DinoSpecialsParams(C.Structure):
    _fields_ = [("x", vp), ("ldx", i64), ("V", i64), ("tokens_per_view", i64), ("cls", vp), ("pos0", vp),
                ("reg", vp), ("n_reg", i32)]


class AssembleParams(C.Structure):
    _fields_ = [("xd", vp), ("ldxd", i64), ("norm_w", vp), ("norm_b", vp), ("eps", f32),
                ("camera_token", vp), ("register_token", vp), ("cam_add", vp), ("depth_tok", vp),
                ("depth_row", vp), ("placeholder", vp), ("out", vp), ("ldo", i64),
                ("V", i64), ("S", i64), ("tokens_per_view", i64), ("n_special", i32), ("view0", i64)]


class CopyRowsParams(C.Structure):
    _fields_ = [("x", vp), ("ldx", i64), ("y", vp), ("ldy", i64), ("rows", i64), ("n", i64)]


class HeadLayerNormParams(C.Structure):
    _fields_ = [("x", vp), ("ldx", i64), ("y", vp), ("ldy", i64), ("weight", vp), ("bias", vp),
                ("rows", i64), ("p0", i64), ("p1", i64), ("row_off", i64), ("eps", f32), ("dtype", i32)]


class ConvParams(C.Structure):
    _fields_ = [("x", vp), ("ldx", i64), ("w", vp), ("bias", vp), ("y", vp), ("ldy", i64),
                ("add1", vp), ("ld1", i64), ("add2", vp), ("ld2", i64), ("pos_x", vp), ("pos_y", vp),
                ("n_img", i64), ("H", i32), ("W", i32), ("Cin", i32), ("Cout", i32), ("w_rows", i32), ("ksize", i32),
                ("stride", i32), ("upshuffle", i32), ("relu", i32), ("out_f32", i32), ("dtype", i32)]


class UpsampleParams(C.Structure):
    _fields_ = [("x", vp), ("ldx", i64), ("y", vp), ("ldy", i64), ("pos_x", vp), ("pos_y", vp),
                ("n_img", i64), ("H", i32), ("W", i32), ("OH", i32), ("OW", i32), ("C", i32), ("dtype", i32)]


class DptOutParams(C.Structure):
    _fields_ = [("h", vp), ("w2", vp), ("b2", vp), ("val", vp), ("conf", vp), ("npix", i64), ("out_dim", i32), ("activation", i32)]


class DptTailParams(C.Structure):
    _fields_ = [("x", vp), ("ldx", i64), ("pos_x", vp), ("pos_y", vp), ("w1", vp), ("ldw1", i64), ("b1", vp), ("w2", vp), ("b2", vp),
                ("val", vp), ("conf", vp), ("n_img", i64), ("H", i32), ("W", i32), ("OH", i32), ("OW", i32), ("C", i32),
                ("out_dim", i32), ("activation", i32), ("dtype", i32)]


class HeadsToTokensParams(C.Structure):
    _fields_ = [("x", vp), ("n_pad", i64), ("y", vp), ("ldy", i64), ("n", i64), ("heads", i32), ("dtype", i32)]


class UnprojectParams(C.Structure):
    _fields_ = [("depth", vp), ("cam", vp), ("out", vp), ("S", i64), ("H", i32), ("W", i32)]


CAMERA_MAX_TRUNK = 4


class CameraBlockWeights(C.Structure):
    _fields_ = [("n1_w", vp), ("n1_b", vp), ("n2_w", vp), ("n2_b", vp), ("ls1", vp), ("ls2", vp),
                ("qkv_w", vp), ("qkv_b", vp), ("proj_w", vp), ("proj_b", vp), ("fc1_w", vp), ("fc1_b", vp), ("fc2_w", vp), ("fc2_b", vp)]


class CameraHeadParams(C.Structure):
    _fields_ = [("tokens", vp), ("ld_tokens", i64), ("S", i32), ("iters", i32), ("dtype", i32), ("trunk_depth", i32), ("dim", i32), ("heads", i32),
                ("token_norm_w", vp), ("token_norm_b", vp), ("trunk_norm_w", vp), ("trunk_norm_b", vp), ("empty_pose", vp),
                ("embed_w", vp), ("embed_b", vp), ("mod_w", vp), ("mod_b", vp), ("blk", CameraBlockWeights * CAMERA_MAX_TRUNK),
                ("pb1_w", vp), ("pb1_b", vp), ("pb2_w", vp), ("pb2_b", vp), ("ws", vp), ("ws_bytes", i64), ("out", vp)]


class CameraTablesParams(C.Structure):
    _fields_ = [("extrinsics", vp), ("intrinsics", vp), ("index", vp), ("B", i32), ("S", i32), ("Sc", i32), ("H", i32), ("W", i32), ("G", i32),
                ("pose_w", vp), ("pose_b", vp), ("adapt_w", vp), ("adapt_b", vp), ("enc", vp), ("emb", vp), ("tables", vp)]


PCT_MAX_COLS, PCT_MAX_Q = 4, 4
PF_BLACK_BG, PF_WHITE_BG = 1, 2
PF_COUNT, PF_SCATTER = 1, 2


class PercentileParams(C.Structure):
    _fields_ = [("x", vp), ("n", i64), ("stride", i64), ("col_stride", i64), ("ncols", i32), ("nq", i32), ("q", f32 * PCT_MAX_Q),
                ("mask", vp), ("out", vp), ("norm_out", vp), ("ws", vp), ("ws_bytes", i64)]


class PointFilterParams(C.Structure):
    _fields_ = [("conf", vp), ("mask", vp), ("threshold", vp), ("min_conf", f32), ("flags", i32), ("images", vp), ("hw", i64),
                ("points", vp), ("n", i64), ("stage", i32), ("pad", i32), ("index_base", i64), ("capacity", i64),
                ("out_points", vp), ("out_colors", vp), ("out_index", vp), ("out_count", vp), ("ws", vp), ("ws_bytes", i64)]


VG_COUNT, VG_SCATTER = 1, 2
VG_OVERFLOW, VG_BAD_VOXEL = 1, 2


class VoxelDownsampleParams(C.Structure):
    _fields_ = [("points", vp), ("conf", vp), ("colors", vp), ("voxel", vp), ("n", i64), ("stage", i32), ("pad", i32), ("capacity", i64),
                ("out_points", vp), ("out_colors", vp), ("out_index", vp), ("out_count", vp), ("ws", vp), ("ws_bytes", i64)]


RENDER_MAX_RADIUS = 8
RENDER_NO_PREREAD = 1


class RenderParams(C.Structure):
    _fields_ = [("points", vp), ("colors", vp), ("n", i64), ("cams", vp), ("V", i32), ("H", i32), ("W", i32), ("radius", i32),
                ("near", f32), ("background", C.c_uint8 * 3), ("pad0", C.c_uint8), ("flags", i32), ("pad1", i32),
                ("ws", vp), ("ws_bytes", i64), ("out_rgb", vp), ("out_depth", vp), ("out_index", vp)]


MESH_SHADE_COLOR, MESH_SHADE_HEADLIGHT, MESH_SHADE_NORMAL = 0, 1, 2
MESH_CULL_NONE, MESH_CULL_BACK, MESH_CULL_FRONT = 0, 1, 2


class RenderMeshParams(C.Structure):
    _fields_ = [("vertices", vp), ("faces", vp), ("normals", vp), ("colors", vp), ("M", i64), ("F", i64), ("cams", vp),
                ("V", i32), ("H", i32), ("W", i32), ("shading", i32), ("cull", i32), ("coop_threshold", i32), ("near", f32),
                ("background", C.c_uint8 * 3), ("pad0", C.c_uint8), ("flags", i32), ("pad1", i32),
                ("ws", vp), ("ws_bytes", i64), ("out_rgb", vp), ("out_depth", vp), ("out_index", vp)]


MVC_MAX_VIEWS = 32767
MVC_TILE_DEFAULT, MVC_TILE_256x1, MVC_TILE_16x16, MVC_TILE_8x32, MVC_TILE_32x8 = 0, 1, 2, 3, 4
MVC_ROTATE_TARGETS, MVC_KEEP_MAP = 1, 2


class ConsistencyParams(C.Structure):
    _fields_ = [("points", vp), ("cams", vp), ("valid", vp), ("S", i32), ("H", i32), ("W", i32), ("src_first", i32), ("src_count", i32),
                ("tol", f32), ("near", f32), ("tile", i32), ("flags", i32), ("pad", i32), ("ws", vp), ("ws_bytes", i64),
                ("support", vp), ("violations", vp), ("occluded", vp)]


NN_QUERY_TILE, NN_REFERENCE_TILE = 512, 512                  # queries per workgroup, references per LDS tile (tests place shapes around them)
NN_EXCLUDE_SAME_INDEX = 1


class NnParams(C.Structure):
    _fields_ = [("query", vp), ("reference", vp), ("query_valid", vp), ("reference_valid", vp), ("nq", i64), ("nr", i64),
                ("flags", i32), ("splits", i32), ("ws", vp), ("ws_bytes", i64), ("index", vp), ("sqdist", vp)]


FPS_SMALL_MAX, FPS_TILE = 8192, 1024                         # largest cloud of the one-workgroup form, points per workgroup of the per-step form
FPS_INCLUDE_LAST = 1
FPS_PATH_AUTO, FPS_PATH_ONE_WORKGROUP, FPS_PATH_PER_STEP = 0, 1, 2


class FpsParams(C.Structure):
    _fields_ = [("points", vp), ("valid", vp), ("batch", i64), ("n", i64), ("npoint", i64), ("first", i64), ("flags", i32), ("path", i32),
                ("ws", vp), ("ws_bytes", i64), ("index", vp), ("sqdist", vp), ("distance", vp)]


RS_BUILD, RS_SEARCH = 1, 2                                   # ovg_radius_params.stage
RS_EXCLUDE_SAME_INDEX = 1
RS_BAD_ORIGIN, RS_OVER_BUDGET, RS_NOT_BUILT = 1, 2, 4        # out_stats[0]
RS_MIN_SLOTS, RS_QUERY_BLOCK = 1024, 256                     # smallest hash table, queries per workgroup (tests place shapes around them)


class RadiusParams(C.Structure):
    _fields_ = [("query", vp), ("reference", vp), ("query_valid", vp), ("reference_valid", vp), ("origin", vp), ("nq", i64), ("nr", i64),
                ("radius_sq", f32), ("cell", f32), ("flags", i32), ("stage", i32), ("max_pairs", i64), ("ws", vp), ("ws_bytes", i64),
                ("out_stats", vp), ("count", vp), ("index", vp), ("sqdist", vp)]


KNN_MAX_K = 32                                               # ovg_knn_params.k
KNN_NORMALS_SWEEPS = 8                                       # Jacobi sweeps of ovg_knn_normals


class KnnParams(C.Structure):
    _fields_ = [("query", vp), ("reference", vp), ("query_valid", vp), ("reference_valid", vp), ("origin", vp), ("nq", i64), ("nr", i64),
                ("radius_sq", f32), ("cell", f32), ("flags", i32), ("k", i32), ("max_pairs", i64), ("ws", vp), ("ws_bytes", i64),
                ("out_stats", vp), ("count", vp), ("index", vp), ("sqdist", vp)]


CL_UNUSABLE, CL_NOISE, CL_BORDER, CL_CORE = 0, 1, 2, 3           # ovg_cluster's kind
CL_INTERNAL = 8                                              # out_stats[0] of ovg_cluster, next to the RS_ flags


class ClusterParams(C.Structure):
    _fields_ = [("points", vp), ("valid", vp), ("origin", vp), ("n", i64), ("radius_sq", f32), ("cell", f32), ("min_neighbours", i32),
                ("flags", i32), ("max_pairs", i64), ("ws", vp), ("ws_bytes", i64), ("out_stats", vp), ("root", vp), ("kind", vp),
                ("degree", vp)]


class KnnNormalsParams(C.Structure):
    _fields_ = [("query", vp), ("reference", vp), ("index", vp), ("viewpoint", vp), ("nq", i64), ("nr", i64), ("k", i32),
                ("viewpoint_stride", i32), ("normal", vp), ("curvature", vp), ("covariance", vp), ("used", vp)]


ALIGN_THREADS, ALIGN_TILE, ALIGN_JACOBI_SWEEPS, ALIGN_SUMS, ALIGN_PARTIAL_BYTES = 256, 1024, 12, 18, 160   # the order of ovg_align_moments' sums
ALIGN_GATE = 1                                               # ovg_align_moments_params.flags
ALIGN_SCALE, ALIGN_COMPOSE = 1, 2                            # ovg_align_solve_params.flags
ALIGN_FEW_PAIRS, ALIGN_NO_SPREAD, ALIGN_NOT_FINITE = 1, 2, 4 # out_status of ovg_align_solve
ALIGN_SPREAD_EPS = 2.0 ** -40


class AlignMomentsParams(C.Structure):
    _fields_ = [("source", vp), ("target", vp), ("index", vp), ("source_valid", vp), ("target_valid", vp), ("sqdist", vp), ("centre", vp),
                ("n", i64), ("m", i64), ("max_sqdist", f32), ("flags", i32), ("ws", vp), ("ws_bytes", i64), ("out_count", vp), ("out_sums", vp)]


class AlignSolveParams(C.Structure):
    _fields_ = [("count", vp), ("sums", vp), ("centre", vp), ("flags", i64), ("transform", vp), ("out_scale", vp), ("out_rms", vp),
                ("out_count", vp), ("out_status", vp)]


class AlignApplyParams(C.Structure):
    _fields_ = [("points", vp), ("transform", vp), ("n", i64), ("out", vp)]


WALIGN_SUMS, WALIGN_PARTIAL_BYTES = 20, 176                  # ovg_align_wmoments: the 18 sums weighted, then W and W^2
WALIGN_CAUCHY = 1                                            # ovg_align_wmoments_params.flags
WALIGN_KEEP = 4                                              # ovg_align_wsolve_params.flags, next to ALIGN_SCALE


class AlignWMomentsParams(C.Structure):
    _fields_ = [("source", vp), ("target", vp), ("weight", vp), ("source_valid", vp), ("target_valid", vp), ("transform", vp),
                ("delta", vp), ("centre", vp), ("delta_scale", C.c_double), ("n", i64), ("flags", i64), ("ws", vp), ("ws_bytes", i64),
                ("out_count", vp), ("out_sums", vp)]


class AlignWSolveParams(C.Structure):
    _fields_ = [("count", vp), ("sums", vp), ("centre", vp), ("flags", i64), ("transform", vp), ("out_scale", vp), ("out_rms", vp),
                ("out_fit_rms", vp), ("out_weight", vp), ("out_count", vp), ("out_status", vp)]


class AlignMoveMapsParams(C.Structure):
    _fields_ = [("points", vp), ("depth", vp), ("points_conf", vp), ("depth_conf", vp), ("transform", vp), ("scale", vp), ("n", i64),
                ("out_points", vp), ("out_depth", vp), ("out_points_conf", vp), ("out_depth_conf", vp)]


class AlignMoveCamerasParams(C.Structure):
    _fields_ = [("extrinsic", vp), ("transform", vp), ("scale", vp), ("views", i64), ("out", vp)]


DEPTHEVAL_THREADS, DEPTHEVAL_TILE, DEPTHEVAL_SUMS, DEPTHEVAL_COUNTS, DEPTHEVAL_PARTIAL_BYTES = 256, 1024, 5, 4, 80   # the order of ovg_deptheval_sums
DEPTHEVAL_MAX_GROUPS, DEPTHEVAL_CHUNK, DEPTHEVAL_MEDIAN_GROUP_BYTES = 4096, 16384, 4128
DEPTHEVAL_MOMENTS, DEPTHEVAL_METRICS = 0, 1                  # ovg_deptheval_sums_params.mode
DEPTHEVAL_NONE, DEPTHEVAL_MEDIAN, DEPTHEVAL_SCALE, DEPTHEVAL_SCALE_SHIFT = 0, 1, 2, 3   # ovg_deptheval_solve_params.mode
DEPTHEVAL_FEW, DEPTHEVAL_NOT_FINITE, DEPTHEVAL_NO_SPREAD, DEPTHEVAL_BAD_FIT = 1, 2, 4, 8   # status of ovg_deptheval_solve
DEPTHEVAL_SPREAD_EPS = 2.0 ** -40


class DepthEvalMedianParams(C.Structure):
    _fields_ = [("pred", vp), ("gt", vp), ("valid", vp), ("groups", i64), ("n", i64), ("stride", i64), ("min_depth", f32), ("max_depth", f32),
                ("ws", vp), ("ws_bytes", i64), ("out_count", vp), ("out_median", vp)]


class DepthEvalSumsParams(C.Structure):
    _fields_ = [("pred", vp), ("gt", vp), ("valid", vp), ("groups", i64), ("n", i64), ("stride", i64), ("min_depth", f32), ("max_depth", f32),
                ("mode", i32), ("reserved", i32), ("coeff", vp), ("clip_min", C.c_double), ("clip_max", C.c_double), ("ws", vp), ("ws_bytes", i64),
                ("out_counts", vp), ("out_sums", vp)]


class DepthEvalSolveParams(C.Structure):
    _fields_ = [("count", vp), ("count_stride", i64), ("sums", vp), ("median", vp), ("groups", i64), ("mode", i32), ("reserved", i32),
                ("coeff", vp), ("status", vp)]


PLANE_HYP_TILE, PLANE_POINT_TILE = 512, 512                 # hypotheses per workgroup, points per LDS tile of ovg_plane_score (tests place shapes around them)
PLANE_NONE, PLANE_FEW, PLANE_NO_SPREAD, PLANE_NOT_FINITE = 1, 2, 4, 8   # status bits of ovg_plane_select (NONE) and ovg_plane_fit
PLANE_COLLINEAR_EPS, PLANE_SPREAD_EPS = 2.0 ** -20, 2.0 ** -40


class PlaneHypothesesParams(C.Structure):
    _fields_ = [("points", vp), ("valid", vp), ("candidates", vp), ("axis", vp), ("n", i64), ("m", i64), ("H", i64), ("seed", C.c_uint64),
                ("min_abs_cos", f32), ("pad", i32), ("planes", vp), ("index", vp)]


class PlaneScoreParams(C.Structure):
    _fields_ = [("points", vp), ("valid", vp), ("planes", vp), ("n", i64), ("H", i64), ("threshold", f32), ("splits", i32), ("count", vp)]


class PlaneSelectParams(C.Structure):
    _fields_ = [("count", vp), ("planes", vp), ("H", i64), ("min_inliers", i32), ("pad", i32), ("best", vp), ("plane", vp),
                ("best_count", vp), ("status", vp)]


class PlaneMaskParams(C.Structure):
    _fields_ = [("points", vp), ("valid", vp), ("plane", vp), ("gate", vp), ("n", i64), ("threshold", f32), ("pad", i32), ("inlier", vp),
                ("distance", vp), ("out_count", vp)]


class PlaneFitParams(C.Structure):
    _fields_ = [("count", vp), ("sums", vp), ("centre", vp), ("axis", vp), ("plane", vp), ("out_rms", vp), ("out_eigen", vp), ("status", vp)]


TSDF_TILE_DEFAULT, TSDF_TILE_256x1x1, TSDF_TILE_8x8x4, TSDF_TILE_16x4x4, TSDF_TILE_32x8x1 = 0, 1, 2, 3, 4   # ovg_tsdf_integrate_params.tile
TSDF_COUNT, TSDF_SCATTER = 1, 2                              # ovg_tsdf_extract_params.stage
TSDF_GREY, TSDF_EXTRACT_BLOCK = 128, 256                     # colour of a vertex without one; lattice points per extraction workgroup


class TsdfIntegrateParams(C.Structure):
    _fields_ = [("tsdf", vp), ("weight", vp), ("color", vp), ("nx", i32), ("ny", i32), ("nz", i32), ("origin", f32 * 3), ("voxel", f32),
                ("trunc", f32), ("max_weight", f32), ("near", f32), ("depth", vp), ("cams", vp), ("valid", vp), ("obs_weight", vp),
                ("colors", vp), ("S", i32), ("H", i32), ("W", i32), ("view_first", i32), ("view_count", i32), ("tile", i32)]


class TsdfExtractParams(C.Structure):
    _fields_ = [("tsdf", vp), ("weight", vp), ("color", vp), ("nx", i32), ("ny", i32), ("nz", i32), ("origin", f32 * 3), ("voxel", f32),
                ("min_weight", f32), ("stage", i32), ("pad", i32), ("vertex_capacity", i64), ("quad_capacity", i64), ("vertices", vp),
                ("normals", vp), ("colors", vp), ("faces", vp), ("out_count", vp), ("ws", vp), ("ws_bytes", i64)]


MAP_UNUSABLE, MAP_DEPTH_EDGE, MAP_NORMAL_EDGE, MAP_NO_NORMAL = 1, 2, 4, 8                       # bits of ovg_map_edges' flags
MAP_TILE_DEFAULT, MAP_TILE_256x1, MAP_TILE_16x16, MAP_TILE_32x8, MAP_TILE_64x4 = 0, 1, 2, 3, 4  # ovg_map_edges_params.tile
MAP_COUNT, MAP_SCATTER = 1, 2                                # ovg_map_triangulate_params.stage
MAP_BLOCK, MAP_MAX_RADIUS = 256, 3                           # pixels per triangulation workgroup; largest window radius of ovg_map_edges


class MapDepthParams(C.Structure):
    _fields_ = [("points", vp), ("cams", vp), ("depth", vp), ("valid", vp), ("S", i32), ("H", i32), ("W", i32), ("near", f32), ("z", vp)]


class MapNormalsParams(C.Structure):
    _fields_ = [("points", vp), ("z", vp), ("S", i32), ("H", i32), ("W", i32), ("rel_tol", f32), ("normals", vp)]


class MapEdgesParams(C.Structure):
    _fields_ = [("z", vp), ("normals", vp), ("S", i32), ("H", i32), ("W", i32), ("radius", i32), ("rel_tol", f32), ("min_cos", f32),
                ("tile", i32), ("pad", i32), ("flags", vp)]


class MapTriangulateParams(C.Structure):
    _fields_ = [("z", vp), ("points", vp), ("keep", vp), ("normals", vp), ("colors", vp), ("S", i32), ("H", i32), ("W", i32),
                ("rel_tol", f32), ("stage", i32), ("pad", i32), ("vertex_capacity", i64), ("face_capacity", i64), ("out_vertices", vp),
                ("out_normals", vp), ("out_colors", vp), ("out_pixel_index", vp), ("out_faces", vp), ("out_count", vp), ("ws", vp),
                ("ws_bytes", i64)]


MS_COUNT, MS_SCATTER = 1, 2                                  # ovg_mesh_simplify_params.stage
MS_OVERFLOW, MS_BAD_VOXEL = 1, 2                             # flags in out_count[2]
MS_POS_MEAN, MS_POS_FIRST = 0, 1                             # ovg_mesh_simplify_params.position


class MeshSimplifyParams(C.Structure):
    _fields_ = [("vertices", vp), ("faces", vp), ("normals", vp), ("colors", vp), ("voxel", vp), ("num_vertices", i64), ("num_faces", i64),
                ("stage", i32), ("position", i32), ("vertex_capacity", i64), ("face_capacity", i64), ("out_vertices", vp),
                ("out_normals", vp), ("out_colors", vp), ("out_source_index", vp), ("out_vertex_count", vp), ("out_faces", vp),
                ("out_count", vp), ("ws", vp), ("ws_bytes", i64)]


MT_REFERENCED, MT_BOUNDARY, MT_NONMANIFOLD = 1, 2, 4          # ovg_mesh_topology: bits of vertex_flags
MT_INTERNAL = 1                                              # flag in out_count[7]
MSEL_COUNT, MSEL_SCATTER = 1, 2                              # ovg_mesh_select_params.stage
MSM_NONFINITE = 1                                            # ovg_mesh_smooth: flag in out_status[0]


class MeshTopologyParams(C.Structure):
    _fields_ = [("vertices", vp), ("faces", vp), ("num_vertices", i64), ("num_faces", i64), ("vertex_root", vp), ("face_root", vp),
                ("vertex_flags", vp), ("out_count", vp), ("ws", vp), ("ws_bytes", i64)]


class MeshSelectParams(C.Structure):
    _fields_ = [("vertices", vp), ("faces", vp), ("face_keep", vp), ("vertex_keep", vp), ("num_vertices", i64), ("num_faces", i64),
                ("stage", i32), ("pad", i32), ("vertex_capacity", i64), ("face_capacity", i64), ("out_vertices", vp), ("out_source_index", vp),
                ("out_faces", vp), ("out_face_index", vp), ("out_count", vp), ("ws", vp), ("ws_bytes", i64)]


class MeshSmoothParams(C.Structure):
    _fields_ = [("vertices", vp), ("faces", vp), ("fixed", vp), ("num_vertices", i64), ("num_faces", i64), ("iterations", i32),
                ("fix_boundary", i32), ("lam", f32), ("mu", f32), ("out_vertices", vp), ("out_normals", vp), ("out_status", vp), ("ws", vp),
                ("ws_bytes", i64)]


RS_F32_CHW, RS_U8_HWC = 0, 1


class ResampleFrame(C.Structure):
    _fields_ = [("src_off", i64), ("src_w", i32), ("src_h", i32), ("res_w", i32), ("res_h", i32), ("crop_y", i32), ("out_h", i32),
                ("mid_row0", i32), ("mid_rows", i32), ("mid_off", i64), ("h_bounds_off", i32), ("h_k_off", i32), ("h_ksize", i32),
                ("v_bounds_off", i32), ("v_k_off", i32), ("v_ksize", i32), ("canvas_w", i32), ("canvas_h", i32), ("pad_top", i32),
                ("pad_left", i32), ("canvas_off", i64)]


class ResampleParams(C.Structure):
    _fields_ = [("frames", vp), ("frames_host", vp), ("nframes", i32), ("out_format", i32), ("src", vp), ("src_bytes", i64),
                ("coef", vp), ("coef_host", vp), ("coef_len", i64), ("lut", vp), ("out", vp), ("out_elems", i64),
                ("ws", vp), ("ws_bytes", i64)]


class DepthFrame(C.Structure):
    _fields_ = [("src_off", i64), ("src_w", i32), ("src_h", i32), ("rows_off", i32), ("cols_off", i32), ("out_w", i32), ("out_h", i32),
                ("out_off", i64)]


class DepthParams(C.Structure):
    _fields_ = [("frames", vp), ("frames_host", vp), ("nframes", i32), ("max_depth", f32), ("src", vp), ("src_elems", i64),
                ("index", vp), ("index_host", vp), ("index_len", i64), ("depth", vp), ("mask", vp), ("out_elems", i64)]


# every entry point of include/omnivggt_hip.h: name -> (restype, argtypes)
SYMBOLS = {
    "ovg_abi_version": (i32, []),
    "ovg_build_info": (C.c_char_p, []),
    "ovg_layernorm": (i32, [C.POINTER(LayerNormParams), vp]),
    "ovg_linear": (i32, [C.POINTER(LinearParams), vp]),
    "ovg_qkv": (i32, [C.POINTER(QkvParams), vp]),
    "ovg_flash_attn": (i32, [C.POINTER(AttnParams), vp]),
    "ovg_block_forward": (i32, [C.POINTER(BlockParams), vp]),
    "ovg_block_attn_prologue": (i32, [C.POINTER(BlockParams), vp]),
    "ovg_block_attn_epilogue": (i32, [C.POINTER(BlockParams), vp]),
    "ovg_im2col": (i32, [C.POINTER(Im2colParams), vp]),
    "ovg_depth_stats": (i32, [C.POINTER(DepthStatsParams), vp]),
    "ovg_dino_specials": (i32, [C.POINTER(DinoSpecialsParams), vp]),
    "ovg_assemble_tokens": (i32, [C.POINTER(AssembleParams), vp]),
    "ovg_copy_rows": (i32, [C.POINTER(CopyRowsParams), vp]),
    "ovg_head_layernorm": (i32, [C.POINTER(HeadLayerNormParams), vp]),
    "ovg_conv": (i32, [C.POINTER(ConvParams), vp]),
    "ovg_upsample": (i32, [C.POINTER(UpsampleParams), vp]),
    "ovg_dpt_out": (i32, [C.POINTER(DptOutParams), vp]),
    "ovg_dpt_tail": (i32, [C.POINTER(DptTailParams), vp]),
    "ovg_unproject": (i32, [C.POINTER(UnprojectParams), vp]),
    "ovg_heads_to_tokens": (i32, [C.POINTER(HeadsToTokensParams), vp]),
    "ovg_probe_mfma": (i32, [vp, vp, vp, i32, vp]),
    "ovg_attn_merge": (i32, [C.POINTER(AttnMergeParams), vp]),
    "ovg_attn_plan": (i32, [C.POINTER(AttnParams), C.POINTER(AttnPlanOut)]),
    "ovg_block_workspace_bytes": (i32, [C.POINTER(BlockParams), C.POINTER(BlockWorkspace)]),
    "ovg_pack_weights": (i32, [C.POINTER(PackWeightsParams), vp]),
    "ovg_camera_head": (i32, [C.POINTER(CameraHeadParams), vp]),
    "ovg_camera_head_workspace_bytes": (i64, [i32, i32]),
    "ovg_camera_tables": (i32, [C.POINTER(CameraTablesParams), vp]),
    "ovg_percentile": (i32, [C.POINTER(PercentileParams), vp]),
    "ovg_percentile_workspace_bytes": (i64, [i64, i32]),
    "ovg_point_filter": (i32, [C.POINTER(PointFilterParams), vp]),
    "ovg_point_filter_workspace_bytes": (i64, [i64]),
    "ovg_resample_frames": (i32, [C.POINTER(ResampleParams), vp]),
    "ovg_resample_workspace_bytes": (i64, [vp, i32]),
    "ovg_depth_frames": (i32, [C.POINTER(DepthParams), vp]),
    # added under ABI 13 without a new number: load() reports a library that predates them by name
    "ovg_voxel_downsample": (i32, [C.POINTER(VoxelDownsampleParams), vp]),
    "ovg_voxel_downsample_workspace_bytes": (i64, [i64]),
    "ovg_render_points": (i32, [C.POINTER(RenderParams), vp]),
    "ovg_render_workspace_bytes": (i64, [i32, i32, i32]),
    "ovg_multiview_consistency": (i32, [C.POINTER(ConsistencyParams), vp]),
    "ovg_consistency_workspace_bytes": (i64, [i32, i32, i32]),
    "ovg_nearest_neighbours": (i32, [C.POINTER(NnParams), vp]),
    "ovg_nn_workspace_bytes": (i64, [i64, i64]),
    "ovg_farthest_point_sample": (i32, [C.POINTER(FpsParams), vp]),
    "ovg_fps_workspace_bytes": (i64, [i64, i64, i64]),
    "ovg_radius_search": (i32, [C.POINTER(RadiusParams), vp]),
    "ovg_radius_workspace_bytes": (i64, [i64, i64]),
    "ovg_knn_search": (i32, [C.POINTER(KnnParams), vp]),
    "ovg_knn_normals": (i32, [C.POINTER(KnnNormalsParams), vp]),
    "ovg_cluster": (i32, [C.POINTER(ClusterParams), vp]),
    "ovg_align_moments": (i32, [C.POINTER(AlignMomentsParams), vp]),
    "ovg_align_workspace_bytes": (i64, [i64]),
    "ovg_align_solve": (i32, [C.POINTER(AlignSolveParams), vp]),
    "ovg_align_apply": (i32, [C.POINTER(AlignApplyParams), vp]),
    "ovg_align_wmoments": (i32, [C.POINTER(AlignWMomentsParams), vp]),
    "ovg_align_wmoments_workspace_bytes": (i64, [i64]),
    "ovg_align_wsolve": (i32, [C.POINTER(AlignWSolveParams), vp]),
    "ovg_align_move_maps": (i32, [C.POINTER(AlignMoveMapsParams), vp]),
    "ovg_align_move_cameras": (i32, [C.POINTER(AlignMoveCamerasParams), vp]),
    "ovg_plane_hypotheses": (i32, [C.POINTER(PlaneHypothesesParams), vp]),
    "ovg_plane_score": (i32, [C.POINTER(PlaneScoreParams), vp]),
    "ovg_plane_select": (i32, [C.POINTER(PlaneSelectParams), vp]),
    "ovg_plane_mask": (i32, [C.POINTER(PlaneMaskParams), vp]),
    "ovg_plane_fit": (i32, [C.POINTER(PlaneFitParams), vp]),
    "ovg_tsdf_integrate": (i32, [C.POINTER(TsdfIntegrateParams), vp]),
    "ovg_tsdf_extract": (i32, [C.POINTER(TsdfExtractParams), vp]),
    "ovg_tsdf_extract_workspace_bytes": (i64, [i32, i32, i32]),
    "ovg_render_mesh": (i32, [C.POINTER(RenderMeshParams), vp]),
    "ovg_render_mesh_workspace_bytes": (i64, [i32, i32, i32]),
    "ovg_deptheval_median": (i32, [C.POINTER(DepthEvalMedianParams), vp]),
    "ovg_deptheval_median_workspace_bytes": (i64, [i64, i64]),
    "ovg_deptheval_sums": (i32, [C.POINTER(DepthEvalSumsParams), vp]),
    "ovg_deptheval_sums_workspace_bytes": (i64, [i64, i64]),
    "ovg_deptheval_solve": (i32, [C.POINTER(DepthEvalSolveParams), vp]),
    "ovg_map_depth": (i32, [C.POINTER(MapDepthParams), vp]),
    "ovg_map_normals": (i32, [C.POINTER(MapNormalsParams), vp]),
    "ovg_map_edges": (i32, [C.POINTER(MapEdgesParams), vp]),
    "ovg_map_triangulate": (i32, [C.POINTER(MapTriangulateParams), vp]),
    "ovg_map_triangulate_workspace_bytes": (i64, [i32, i32, i32]),
    "ovg_mesh_simplify": (i32, [C.POINTER(MeshSimplifyParams), vp]),
    "ovg_mesh_simplify_workspace_bytes": (i64, [i64, i64]),
    "ovg_mesh_topology": (i32, [C.POINTER(MeshTopologyParams), vp]),
    "ovg_mesh_topology_workspace_bytes": (i64, [i64, i64]),
    "ovg_mesh_select": (i32, [C.POINTER(MeshSelectParams), vp]),
    "ovg_mesh_select_workspace_bytes": (i64, [i64, i64]),
    "ovg_mesh_smooth": (i32, [C.POINTER(MeshSmoothParams), vp]),
    "ovg_mesh_smooth_workspace_bytes": (i64, [i64, i64]),
}


class OvgError(RuntimeError):
    pass


_lib = None


def load(build_if_missing=True):
    """Load the shared library. A missing or STALE library (its build stamp differs from the digest of csrc/,
    the header and the compiler flags) is rebuilt in-tree when hipcc is available, otherwise loading fails
    loudly: kernels from an older source tree must never be validated or benchmarked by accident."""
    global _lib
    if _lib is not None:
        return _lib
    from . import build as B
    if not os.path.exists(LIB_PATH) or not B.is_current():
        if not build_if_missing or not B.have_hipcc():
            raise OvgError("libomnivggt_hip.so is %s (run __graft_entry__.build()); there is no fallback path"
                           % ("missing" if not os.path.exists(LIB_PATH) else "stale: csrc/ changed since it was built"))
        B.build()      # takes an exclusive file lock and re-checks the stamp under it: N ranks starting together build once
    # torch bundles its own libamdhip64.so.7; it MUST be in the process before our library is
    # dlopen'ed, otherwise the loader maps /opt/rocm's copy for us and torch's copy for torch:
    # two HIP runtimes, and our launches on torch's streams fail (OVG_E_LAUNCH).
    import torch  # noqa: F401
    lib = C.CDLL(LIB_PATH)
    for name, (res, args) in SYMBOLS.items():
        try:
            fn = getattr(lib, name)
        except AttributeError:       # ABI mismatch, fail loudly (entries may be added without a new ABI number: a stale library lacks them)
            raise OvgError("%s lacks %s: the library predates this binding; rebuild it with __graft_entry__.build()" % (LIB_PATH, name)) from None
        fn.restype = res
        fn.argtypes = args
    if lib.ovg_abi_version() != ABI_VERSION:
        raise OvgError("ABI version mismatch: library %d, binding %d" % (lib.ovg_abi_version(), ABI_VERSION))
    _lib = lib
    return lib


def check(rc, what):
    if rc != 0:
        raise OvgError("%s failed: %s (%d)" % (what, ERRORS.get(rc, "?"), rc))


def call(name, params, stream):
    """Invoke `name(&params, stream)`; raises OvgError on a non-zero return code."""
    lib = load()
    rc = getattr(lib, name)(C.byref(params), stream)
    check(rc, name)


def ptr(t):
    """Device pointer of a torch tensor (None -> NULL)."""
    return None if t is None else t.data_ptr()


class _SplitF16:
    """compute_dtype sentinel of the split-f16 mode (C ABI: OVG_F16X2): every 16-bit tensor is a (hi, lo) pair of f16 planes, every
    contraction three f16 MFMAs with f32 accumulation -- outputs within 1e-4 of the reference like the f32 mode, at ~3x its speed."""
    _instance = None

    def __new__(cls):                         # ONE instance per process: the mode is tested with `is` (is_split, dtype_code, cache keys), so
        if cls._instance is None:             # copy.deepcopy(model), pickle / torch.save + load and multiprocessing must all hand back F32X itself
            cls._instance = super().__new__(cls)
        return cls._instance

    def __repr__(self):
        return "f32x"

    def __reduce__(self):
        return (_SplitF16, ())

    def __copy__(self):
        return self

    def __deepcopy__(self, memo):
        return self


F32X = _SplitF16()


def is_split(dtype):
    return dtype is F32X


def storage_dtype(dtype):
    """torch dtype of the planes / tensors that hold `dtype` activations and GEMM weights."""
    import torch
    return torch.float16 if dtype is F32X else dtype


def head_dtype(dtype):
    """dtype the prediction heads run in for an aggregator compute dtype (the split mode keeps the heads on the exact-f32 kernels)."""
    import torch
    return torch.float32 if dtype is F32X else dtype


def dtype_code(torch_dtype):
    import torch
    if torch_dtype is F32X:
        return OVG_F16X2
    return {torch.bfloat16: OVG_BF16, torch.float16: OVG_F16, torch.float32: OVG_F32}[torch_dtype]


def require_gpu():
    import torch
    if not torch.cuda.is_available():
        raise OvgError("no HIP device visible: the aggregator hot path has no CPU fallback")
