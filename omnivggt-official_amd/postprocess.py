"""Post-processing of the prediction dict on the device.

`pose_encoding_to_extri_intri` mirrors omnivggt/utils/pose_enc.py:65-130 (O(S) tensor math, any device);
`unproject_depth_map_to_point_map` mirrors omnivggt/utils/geometry.py:151-266 but keeps the maps on the GPU:
the per-frame numpy loop of the reference becomes one `ovg_unproject` launch (no device->host copy of the
(S, H, W) maps before export / visualisation).
"""
import torch

from . import camera_math, ops


def pose_encoding_to_extri_intri(pose_encoding, image_size_hw=None, pose_encoding_type="absT_quaR_FoV", build_intrinsics=True):
    """utils/pose_enc.py:65-130: (B,S,9) -> extrinsics (B,S,3,4) camera-from-world, intrinsics (B,S,3,3) in pixels."""
    if pose_encoding_type != "absT_quaR_FoV":
        raise NotImplementedError
    return camera_math.pose_decoding(pose_encoding, image_size_hw, build_intrinsics)


def unproject_depth_map_to_point_map(depth_map, extrinsics_cam, intrinsics_cam, check_skew=None):
    """utils/geometry.py:151-266: depth (S,H,W,1) or (S,H,W), extrinsics (S,3,4) camera-from-world, intrinsics (S,3,3)
    -> world points (S,H,W,3) f32 on the device (the reference returns a numpy array after a host loop).

    Nothing here waits for the device: the camera-from-world inverse (closed_form_inverse_se3, geometry.py:269-318) and the packing of
    the 16 per-frame camera numbers are O(S) tensor operations on the depth map's device, queued in front of the one `ovg_unproject`
    launch. The reference's zero-skew assertion (geometry.py:251) is evaluated where it is free -- on intrinsics that arrive as HOST
    tensors -- and on device-resident intrinsics only when `check_skew=True` (one scalar device -> host read, i.e. a sync)."""
    if not depth_map.is_cuda:
        raise ops.L.OvgError("unproject_depth_map_to_point_map needs HIP device tensors: there is no CPU fallback")
    d = depth_map.squeeze(-1) if depth_map.dim() == 4 else depth_map
    d = d.float().contiguous()
    S = d.shape[0]
    if check_skew is None:
        check_skew = not intrinsics_cam.is_cuda
    if check_skew:
        k = intrinsics_cam.detach().reshape(S, 3, 3)
        if bool(((k[:, 0, 1] != 0) | (k[:, 1, 0] != 0)).any()):
            raise AssertionError("Intrinsic matrix must have zero skew")      # geometry.py:251
    ext = extrinsics_cam.detach().to(device=d.device, dtype=torch.float32, non_blocking=True).reshape(S, 3, 4)
    intr = intrinsics_cam.detach().to(device=d.device, dtype=torch.float32, non_blocking=True).reshape(S, 3, 3)
    Rt = ext[:, :, :3].transpose(1, 2)                                       # world-from-camera rotation
    c = -torch.bmm(Rt, ext[:, :, 3:])                                        # camera centre in the world
    cam = torch.cat([Rt.reshape(S, 9), c.reshape(S, 3), intr[:, 0, 0:1], intr[:, 1, 1:2], intr[:, 0, 2:3], intr[:, 1, 2:3]], dim=1)
    return ops.unproject(d, cam.contiguous())


# ---------------------------------------------------------------------------------------------------------------------------------
# Point-cloud extraction and export (visual_util.py:42-73, :77-267, inference.py:368-384)
# ---------------------------------------------------------------------------------------------------------------------------------

def percentile(x, q, dim=None):
    """numpy-2 `percentile(x, q, axis=dim, method="linear")` of a float32 HIP device tensor of any size, bit for bit (ovg_percentile;
    the supported answer where torch.quantile refuses inputs above 2^24 elements). q: a scalar or a 1-D sequence of percentiles in
    [0, 100]; dim None reduces over all elements, an int over that dimension. The result is a device tensor shaped like numpy's:
    q's axis first (for 1-D q), then the remaining dimensions. A NaN anywhere in a reduced slice makes that slice's result NaN."""
    if not isinstance(x, torch.Tensor) or not x.is_cuda:
        raise ops.L.OvgError("percentile needs a HIP device tensor: there is no CPU fallback")
    if x.dtype != torch.float32:
        raise ValueError("percentile: x must be float32 (numpy's rule depends on the dtype)")
    scalar = not isinstance(q, (list, tuple, torch.Tensor)) and not hasattr(q, "__len__")
    qs = [float(q)] if scalar else [float(v) for v in (q.tolist() if isinstance(q, torch.Tensor) else q)]
    if not qs or any(not (0.0 <= v <= 100.0) for v in qs):
        raise ValueError("percentiles must be in the range [0, 100]")
    if dim is None:
        cols, rest = x.reshape(-1, 1), ()
    else:
        xm = x.movedim(dim, 0)
        rest = tuple(xm.shape[1:])
        cols = xm.reshape(xm.shape[0], -1)
    if cols.shape[0] == 0:
        raise ValueError("percentile of an empty reduction")
    n, C = cols.shape
    out = torch.empty(len(qs), C, device=x.device, dtype=torch.float32)
    ws = None
    for c0 in range(0, C, ops.L.PCT_MAX_COLS):
        nc = min(ops.L.PCT_MAX_COLS, C - c0)
        view = cols[:, c0:c0 + nc]
        if ws is None:
            ws = torch.empty(ops.percentile_workspace_bytes(n, ops.L.PCT_MAX_COLS), device=x.device, dtype=torch.uint8)
        for j0 in range(0, len(qs), ops.L.PCT_MAX_Q):
            qq = qs[j0:j0 + ops.L.PCT_MAX_Q]
            r = ops.percentile(view, n, view.stride(0), view.stride(1) if nc > 1 else 0, nc, qq, ws=ws)
            out[j0:j0 + len(qq), c0:c0 + nc] = r.t()
    out = out.reshape((len(qs),) + rest)
    return out[0] if scalar else out


def get_world_points_from_depth(predictions, gt_scale=1):
    """Device analogue of visual_util.py:42-73: adds `extrinsic` (B,S,3,4), `intrinsic` (B,S,3,3) and `world_points_from_depth`
    (B,S,H,W,3) f32 to the prediction dict as OmniVGGT.forward returns it (batch dimension kept, tensors stay on the device; the
    reference squeezes the batch and converts every entry to numpy). Returns the dict."""
    depth = predictions["depth"]
    if not depth.is_cuda:
        raise ops.L.OvgError("get_world_points_from_depth needs HIP device tensors: there is no CPU fallback")
    extrinsic, intrinsic = pose_encoding_to_extri_intri(predictions["pose_enc"], predictions["images"].shape[-2:])
    predictions["extrinsic"] = extrinsic
    predictions["intrinsic"] = intrinsic
    d = depth * gt_scale if gt_scale != 1 else depth
    predictions["world_points_from_depth"] = torch.stack(
        [unproject_depth_map_to_point_map(d[b], extrinsic[b], intrinsic[b], check_skew=False) for b in range(d.shape[0])])
    return predictions


class PointCloud:
    """Result of predictions_to_point_cloud. points (M,3) f32, colors (M,3) u8 and indices (M,) int64 (flat pixel index into the
    batch element's S x H x W maps, or None) are device tensors; conf_threshold (the f32 percentile, 0 when conf_thres == 0) and
    scene_scale (f32) are 0-d device tensors; transform is the (4,4) float64 numpy alignment; extrinsic (S',3,4) the selected
    frames' cameras on the device; conf (M,) f32 the points' confidence after the sky-mask rule (device, or None when not asked for)."""
    __slots__ = ("points", "colors", "conf_threshold", "scene_scale", "transform", "extrinsic", "indices", "conf")

    def __init__(self, points, colors, conf_threshold, scene_scale, transform, extrinsic, indices=None, conf=None):
        self.points, self.colors, self.conf_threshold, self.scene_scale = points, colors, conf_threshold, scene_scale
        self.transform, self.extrinsic, self.indices, self.conf = transform, extrinsic, indices, conf

    def __len__(self):
        return int(self.points.shape[0])


def _parse_frame(filter_by_frames):
    if filter_by_frames in ("all", "All"):
        return None
    try:
        return int(filter_by_frames.split(":")[0])
    except (ValueError, IndexError, AttributeError):
        return None


def scene_alignment(extrinsic0):
    """inv(E0) @ diag(1,-1,-1,1) @ R_y(180 deg) in float64 (visual_util.py:320-358); E0 the (3,4) camera-from-world of the first frame."""
    import numpy as np
    e = np.eye(4)
    e[:3, :4] = np.asarray(extrinsic0, dtype=np.float64)
    return np.linalg.inv(e) @ np.diag([1.0, -1.0, -1.0, 1.0]) @ np.diag([-1.0, 1.0, -1.0, 1.0])


def _prediction_geometry(predictions, prediction_mode, b, images, want_intrinsic=False):
    """The maps and cameras predictions_to_point_cloud and prediction_consistency work on, for batch element b of the dict
    OmniVGGT.forward returns (images: its `images` with the batch dimension): "Pointmap" modes take world_points / world_points_conf
    (world_points_from_depth / depth_conf when the dict has no world_points), other modes world_points_from_depth / depth_conf, decoded
    from pose_enc and un-projected here on the device when absent. -> (points, confidence tensor WITH its batch dimension or None,
    extrinsic (S,3,4), intrinsic (S,3,3) or None when not asked for)."""
    H, W = images.shape[-2], images.shape[-1]
    extrinsic = predictions["extrinsic"][b] if "extrinsic" in predictions else None
    intrinsic = predictions["intrinsic"][b] if want_intrinsic and "intrinsic" in predictions else None
    if "Pointmap" in prediction_mode and "world_points" in predictions:
        pts, conf = predictions["world_points"][b], predictions.get("world_points_conf")
    elif "world_points_from_depth" in predictions:
        pts, conf = predictions["world_points_from_depth"][b], predictions.get("depth_conf")
    else:
        sub = {"depth": predictions["depth"][b:b + 1], "pose_enc": predictions["pose_enc"][b:b + 1], "images": images[b:b + 1]}
        get_world_points_from_depth(sub)
        pts, conf = sub["world_points_from_depth"][0], predictions.get("depth_conf")
        if extrinsic is None:
            extrinsic = sub["extrinsic"][0]
        if want_intrinsic and intrinsic is None:
            intrinsic = sub["intrinsic"][0]
    if extrinsic is None or (want_intrinsic and intrinsic is None):
        if "pose_enc" not in predictions:
            raise ValueError("predictions carry neither `extrinsic`%s nor `pose_enc`: the cameras are needed"
                             % (" / `intrinsic`" if want_intrinsic else ""))
        ext, intr = pose_encoding_to_extri_intri(predictions["pose_enc"][b:b + 1], (H, W))
        extrinsic = ext[0] if extrinsic is None else extrinsic
        intrinsic = intr[0] if want_intrinsic and intrinsic is None else intrinsic
    return pts, conf, extrinsic, intrinsic


def predictions_to_point_cloud(predictions, conf_thres=50.0, filter_by_frames="all", mask_black_bg=False, mask_white_bg=False,
                               prediction_mode="Predicted Pointmap", sky_mask=None, min_conf=1e-5, batch_index=0, return_indices=False,
                               return_conf=False, keep_mask=None):
    """The point cloud of visual_util.predictions_to_glb (:77-267) on the device, for the dict OmniVGGT.forward returns (batch dimension
    included; batch_index=0 is what the reference's select_first_batch keeps).

    Same choices as the reference: "Pointmap" modes take world_points / world_points_conf (world_points_from_depth / depth_conf when
    the dict has no world_points), other modes world_points_from_depth / depth_conf, computed here on the device when absent; a missing
    confidence map is all ones. filter_by_frames "k: ..." keeps frame k, anything unparsable keeps all frames. conf_thres None means
    10, 0 skips the percentile. The threshold is numpy's linear percentile of the (sky-masked) confidences of the selected frames, bit
    for bit; a pixel is kept when conf >= threshold and conf > min_conf (f32), and, on request, when its u8 colour is not black
    (r+g+b < 16) or white (all channels > 240). Colours are trunc(x * 255) of the f32 image, clamped to [0, 255] (the clamp only
    matters for inputs outside [0, 1]). sky_mask: a user-supplied (S, H, W) tensor at the map size; the confidence is multiplied by
    (sky_mask > 0.1) before the frame filter, as in the reference (mask resizing and the ONNX sky model are not part of this).
    scene_scale is ||P95 - P5|| of the kept, untransformed vertices; transform is inv(E0) @ diag(1,-1,-1,1) @ R_y(180) with E0 the
    first selected camera, which the writers apply (the vertices themselves are copied untransformed).
    return_conf: PointCloud.conf holds the kept pixels' confidence after the sky-mask rule (what voxel_downsample ranks by).
    keep_mask: an (S, H, W) bool device tensor (e.g. consistency_mask(...)); pixels where it is False are dropped. Unlike sky_mask it
    does not enter the percentile: the threshold is computed first, on the same values as without it, then the dropped pixels take
    confidence -inf for the filter launches (conf >= threshold and conf > min_conf fails for -inf, also when conf_thres == 0).
    return_conf still reports the original confidences; scene_scale is computed on the kept points. None takes the path without it.

    One divergence: an empty selection returns M = 0 (scene_scale 1); the reference substitutes one white point at (1, 0, 0).
    Exactly one device -> host synchronisation: reading M (with the first selected camera) to size the result. CPU tensors raise
    OvgError: there is no CPU fallback."""
    L = ops.L
    if not isinstance(predictions, dict):
        raise ValueError("predictions must be a dictionary")
    images = predictions["images"]
    if images.dim() == 4:
        images = images.unsqueeze(0)
    B = images.shape[0]
    if not isinstance(batch_index, int) or not 0 <= batch_index < B:
        raise ValueError("batch_index %r out of range for a batch of %d" % (batch_index, B))
    if conf_thres is None:
        conf_thres = 10.0
    b = batch_index
    S, H, W = images.shape[1], images.shape[-2], images.shape[-1]
    if sky_mask is not None and tuple(sky_mask.shape) != (S, H, W):
        raise ValueError("sky_mask must be (S, H, W) = %r at the map size, got %r" % ((S, H, W), tuple(sky_mask.shape)))
    if keep_mask is not None:
        if not isinstance(keep_mask, torch.Tensor) or keep_mask.dtype != torch.bool or tuple(keep_mask.shape) != (S, H, W):
            raise ValueError("keep_mask must be a bool tensor (S, H, W) = %r at the map size" % ((S, H, W),))
    if not images.is_cuda:
        raise L.OvgError("predictions_to_point_cloud needs HIP device tensors: there is no CPU fallback")
    if keep_mask is not None and not keep_mask.is_cuda:
        raise L.OvgError("predictions_to_point_cloud needs HIP device tensors: there is no CPU fallback")
    pts, conf, extrinsic, _ = _prediction_geometry(predictions, prediction_mode, b, images)
    conf = torch.ones(S, H, W, device=images.device, dtype=torch.float32) if conf is None else conf[b]
    for t in (pts, conf, extrinsic):
        if not t.is_cuda:
            raise L.OvgError("predictions_to_point_cloud needs HIP device tensors: there is no CPU fallback")
    pts = pts.reshape(S, H, W, 3).float().contiguous()
    conf = conf.reshape(S, H, W).float().contiguous()
    img = images[b].reshape(S, 3, H, W).float().contiguous()
    mask = None
    if sky_mask is not None:
        mask = sky_mask.to(device=images.device, dtype=torch.float32).contiguous()
    frame = _parse_frame(filter_by_frames)
    base = 0
    if frame is not None:
        if not -S <= frame < S:
            raise ValueError("filter_by_frames selects frame %d of %d" % (frame, S))
        frame %= S
        sl = slice(frame, frame + 1)
        pts, conf, img, extrinsic = pts[sl], conf[sl], img[sl], extrinsic[sl]
        mask = None if mask is None else mask[sl]
        keep_mask = None if keep_mask is None else keep_mask[sl]
        base = frame * H * W
    n, hw = conf.numel(), H * W
    dev = conf.device
    cf = conf.reshape(-1)
    mk = None if mask is None else mask.reshape(-1)
    if conf_thres == 0.0:
        thr = None
        conf_threshold = torch.zeros((), device=dev, dtype=torch.float32)
    else:
        thr = ops.percentile(cf, n, 1, 0, 1, [float(conf_thres)], mask=mk).reshape(1)
        conf_threshold = thr.reshape(())
    flags = (L.PF_BLACK_BG if mask_black_bg else 0) | (L.PF_WHITE_BG if mask_white_bg else 0)
    ws = torch.empty(ops.point_filter_workspace_bytes(n), device=dev, dtype=torch.uint8)
    count = torch.empty(1, device=dev, dtype=torch.int64)
    # the threshold above saw the confidences as they are; only the filter launches see the dropped pixels at -inf
    cf_filter = cf if keep_mask is None else torch.where(keep_mask.reshape(-1), cf, cf.new_full((), float("-inf")))
    args = dict(conf=cf_filter, images=img, points=pts, hw=hw, ws=ws, threshold=thr, mask=mk, min_conf=min_conf, flags=flags, index_base=base)
    ops.point_filter(L.PF_COUNT, out_count=count, **args)
    # the one synchronisation: the cloud size and the first selected camera in one copy (int64 counts are exact in float64 below 2^53)
    host = torch.cat([count.double(), extrinsic[0].reshape(-1).double()]).cpu().numpy()
    M = int(host[0])
    transform = scene_alignment(host[1:13].reshape(3, 4))
    out_pts = torch.empty(M, 3, device=dev, dtype=torch.float32)
    out_col = torch.empty(M, 3, device=dev, dtype=torch.uint8)
    out_idx = torch.empty(M, device=dev, dtype=torch.int64) if return_indices or return_conf else None
    if M:
        ops.point_filter(L.PF_SCATTER, capacity=M, out_points=out_pts, out_colors=out_col, out_index=out_idx, **args)
        _, scale = ops.percentile(out_pts, M, 3, 1, 3, [5.0, 95.0], norm=True)
    else:
        scale = torch.ones((), device=dev, dtype=torch.float32)
    out_conf = None
    if return_conf:
        local = out_idx - base if base else out_idx
        out_conf = cf[local] if mk is None else cf[local] * (mk[local] > 0.1).to(torch.float32)      # the kernels' rule: inf * 0 is NaN
    return PointCloud(out_pts, out_col, conf_threshold, scale, transform, extrinsic, out_idx if return_indices else None, out_conf)


# ---------------------------------------------------------------------------------------------------------------------------------
# Multi-view depth consistency: which pixels do the other views agree with (ovg_multiview_consistency)
# ---------------------------------------------------------------------------------------------------------------------------------

class ConsistencyResult:
    """Result of multiview_consistency: support, violations (S,H,W) int16 device tensors ((1,H,W) for frame=k), occluded likewise or
    None. Per pixel, the number of other views that confirm it / look through it / cannot see it."""
    __slots__ = ("support", "violations", "occluded")

    def __init__(self, support, violations, occluded=None):
        self.support, self.violations, self.occluded = support, violations, occluded


def _pack_cams(extrinsic, intrinsic, V, dev):
    """(V,16) f32 rows as ovg_render_points reads them: rotation row-major, translation, fx, fy, cx, cy; inputs rounded to f32 first."""
    ext = extrinsic.to(device=dev, dtype=torch.float32)
    intr = intrinsic.to(device=dev, dtype=torch.float32).expand(V, 3, 3)
    return torch.cat([ext[:, :, :3].reshape(V, 9), ext[:, :, 3], intr[:, 0, 0:1], intr[:, 1, 1:2], intr[:, 0, 2:3], intr[:, 1, 2:3]],
                     dim=1).contiguous()


def multiview_consistency(points, extrinsic, intrinsic, valid=None, rel_tol=0.02, near=1e-3, frame=None, return_occluded=False):
    """Geometric consistency of S point maps with their S cameras on the device (ovg_multiview_consistency): every pixel's 3-D point
    is projected into each other view (the projection of render_point_cloud, nearest pixel) and its depth zc there is compared with
    the depth d that view holds along the ray. |zc - d| <= rel_tol * d counts as support, zc < d - rel_tol * d as a violation (the
    other view sees a surface behind the point: it looks through it -- a floater), zc > d + rel_tol * d as occluded (no evidence).
    Pairs that leave the frame, fall behind the camera or nearer than `near`, or hit an unusable pixel count nowhere. The rule is
    exact (tests/consistency_twin.py restates it in numpy float32) and two calls give identical bytes. Nearest-pixel lookup only: no
    bilinear depth, no neighbourhood search, no averaging of depths across views.

    points: (S,H,W,3) f32 device tensor, world points in the frame of `extrinsic` (world_points, or world_points_from_depth).
    extrinsic (S,3,4) world-to-camera, intrinsic (S,3,3) or one (3,3): device tensors, numpy arrays or lists, rounded to f32 and
    packed as render_point_cloud packs them. valid: optional (S,H,W) bool / u8 tensor; pixels where it is 0 are neither sources nor
    targets. frame=k computes source view k only (all views stay targets): the cheap form for filter_by_frames.
    rel_tol = 0.02 is the knee measured on ground-truth depth of a real four-view scene (tests/golden/real/infinigen_294: support
    >= 1 for 83 % of the valid pixels, a violation for 1.5 %; halving it loses a fifth of the support, doubling it gains nothing),
    not on predictions of a trained checkpoint: predicted depth is noisier, so treat it as a lower bound.

    -> ConsistencyResult(support, violations, occluded or None). No device -> host synchronisation. CPU tensors raise OvgError (there
    is no CPU fallback); bad shapes, frame, rel_tol or near raise ValueError."""
    import math
    import numpy as np
    L = ops.L
    if not isinstance(points, torch.Tensor) or points.dim() != 4 or points.shape[3] != 3 or 0 in points.shape:
        raise ValueError("multiview_consistency: points must be a (S, H, W, 3) tensor")
    S, H, W = (int(v) for v in points.shape[:3])
    if S > L.MVC_MAX_VIEWS or S * H * W >= 1 << 31:
        raise ValueError("multiview_consistency: S = %d views of %d x %d exceed S <= %d, S * H * W < 2^31" % (S, H, W, L.MVC_MAX_VIEWS))
    ext, intr = torch.as_tensor(extrinsic).detach(), torch.as_tensor(intrinsic).detach()
    if tuple(ext.shape) != (S, 3, 4):
        raise ValueError("multiview_consistency: extrinsic must be (S, 3, 4) = (%d, 3, 4), got %r" % (S, tuple(ext.shape)))
    if tuple(intr.shape) not in ((3, 3), (S, 3, 3)):
        raise ValueError("multiview_consistency: intrinsic must be (3, 3) or (S, 3, 3) = (%d, 3, 3), got %r" % (S, tuple(intr.shape)))
    if valid is not None and (not isinstance(valid, torch.Tensor) or tuple(valid.shape) != (S, H, W)
                              or valid.dtype not in (torch.bool, torch.uint8)):
        raise ValueError("multiview_consistency: valid must be a bool / uint8 tensor (S, H, W) = %r" % ((S, H, W),))
    try:
        with np.errstate(over="ignore"):
            tol32, near32 = float(np.float32(rel_tol)), float(np.float32(near))
    except (TypeError, ValueError):
        tol32 = near32 = float("nan")
    if not (tol32 >= 0.0 and math.isfinite(tol32)):
        raise ValueError("multiview_consistency: rel_tol must be non-negative and finite in float32, got %r" % (rel_tol,))
    if not (near32 > 0.0 and math.isfinite(near32)):
        raise ValueError("multiview_consistency: near must be positive and finite in float32, got %r" % (near,))
    if frame is not None and (isinstance(frame, bool) or not isinstance(frame, (int, np.integer)) or not -S <= frame < S):
        raise ValueError("multiview_consistency: frame %r out of range for %d views" % (frame, S))
    if not points.is_cuda or (valid is not None and not valid.is_cuda):
        raise L.OvgError("multiview_consistency needs HIP device tensors: there is no CPU fallback")
    dev = points.device
    cams = _pack_cams(ext, intr, S, dev)
    if valid is not None:
        valid = (valid.to(torch.uint8) if valid.dtype == torch.bool else valid).contiguous()
    first, count = (0, S) if frame is None else (int(frame) % S, 1)
    sup, vio, occ = ops.multiview_consistency(points.float().contiguous(), cams, tol32, near=near32, valid=valid, src_first=first,
                                              src_count=count, occluded=return_occluded)
    return ConsistencyResult(sup, vio, occ)


def prediction_consistency(predictions, prediction_mode="Predicted Pointmap", batch_index=0, valid=None, **kw):
    """multiview_consistency of the dict OmniVGGT.forward returns: the points by the same choices predictions_to_point_cloud makes for
    `prediction_mode` (world_points, or world_points_from_depth, decoding pose_enc and un-projecting on the device when the dict
    lacks them), the cameras from `extrinsic` / `intrinsic` of the dict, else decoded from pose_enc. **kw: rel_tol, near, frame,
    return_occluded. -> ConsistencyResult; consistency_mask(result) is the keep_mask of predictions_to_point_cloud."""
    if not isinstance(predictions, dict):
        raise ValueError("predictions must be a dictionary")
    images = predictions["images"]
    if images.dim() == 4:
        images = images.unsqueeze(0)
    B = images.shape[0]
    if not isinstance(batch_index, int) or not 0 <= batch_index < B:
        raise ValueError("batch_index %r out of range for a batch of %d" % (batch_index, B))
    if not images.is_cuda:
        raise ops.L.OvgError("prediction_consistency needs HIP device tensors: there is no CPU fallback")
    S, H, W = images.shape[1], images.shape[-2], images.shape[-1]
    pts, _, extrinsic, intrinsic = _prediction_geometry(predictions, prediction_mode, batch_index, images, want_intrinsic=True)
    return multiview_consistency(pts.reshape(S, H, W, 3), extrinsic, intrinsic, valid=valid, **kw)


def consistency_mask(result, min_support=1, max_violations=0):
    """(S,H,W) bool: pixels that at least `min_support` other views confirm and at most `max_violations` look through."""
    return (result.support >= min_support) & (result.violations <= max_violations)


# ---------------------------------------------------------------------------------------------------------------------------------
# Nearest neighbours between clouds: mutual matches and cloud-to-cloud distances (ovg_nearest_neighbours)
# ---------------------------------------------------------------------------------------------------------------------------------

class NNResult:
    """Result of nearest_neighbours: index int32 (the nearest reference point, -1 where there is none) and sqdist float32 (the squared
    distance to it, +inf where there is none), device tensors shaped like the query without its last dimension."""
    __slots__ = ("index", "sqdist")

    def __init__(self, index, sqdist):
        self.index, self.sqdist = index, sqdist


def _nn_points(x, name):
    if isinstance(x, PointCloud):
        x = x.points
    if not isinstance(x, torch.Tensor) or x.dim() < 1 or x.shape[-1] != 3 or x.dtype != torch.float32:
        raise ValueError("%s must be a float32 tensor (..., 3) or a PointCloud" % name)
    if x.numel() // 3 >= 1 << 31:
        raise ValueError("%s holds %d points: the search takes fewer than 2^31" % (name, x.numel() // 3))
    return x


def _nn_valid(v, lead, name):
    if v is None:
        return None
    if not isinstance(v, torch.Tensor) or tuple(v.shape) != tuple(lead) or v.dtype not in (torch.bool, torch.uint8):
        raise ValueError("%s must be a bool / uint8 tensor shaped %r" % (name, tuple(lead)))
    return v


def nearest_neighbours(query, reference, query_valid=None, reference_valid=None, exclude_self=False):
    """For every query point its nearest reference point, searched exhaustively on the device (ovg_nearest_neighbours): no k-d tree, no
    copy to the host. The rule is exact (tests/nn_twin.py restates it in numpy float32): d = (dx dx + dy dy) + dz dz in float32 without
    fused multiply-adds, the smallest d wins and equal distances go to the LOWEST reference index, so two calls, and any tiling of
    the launch, give identical bytes. A point is usable when its coordinates are finite and its valid entry (if given) is non-zero;
    an unusable query, or a query without a usable reference, gets index -1 and sqdist +inf. A distance that overflows float32 to
    +inf still matches.

    query, reference: float32 device tensors (..., 3), or PointClouds (their points); flattened for the search. query_valid /
    reference_valid: optional bool / uint8 tensors shaped like the points without the last dimension. exclude_self=True searches
    inside one cloud: query and reference must hold the same number of points and reference i is no candidate of query i (each
    point's nearest OTHER point: the distance that isolates floaters).

    -> NNResult(index int32, sqdist float32) shaped like the query's leading dimensions. No device -> host synchronisation. CPU
    tensors raise OvgError (there is no CPU fallback); bad shapes or dtypes raise ValueError."""
    q, r = _nn_points(query, "query"), _nn_points(reference, "reference")
    lead = tuple(q.shape[:-1])
    qv, rv = _nn_valid(query_valid, lead, "query_valid"), _nn_valid(reference_valid, tuple(r.shape[:-1]), "reference_valid")
    nq, nr = q.numel() // 3, r.numel() // 3
    if exclude_self and nq != nr:
        raise ValueError("exclude_self searches inside one cloud: query and reference must hold the same number of points (%d, %d)" % (nq, nr))
    if not all(t is None or t.is_cuda for t in (q, r, qv, rv)):
        raise ops.L.OvgError("nearest_neighbours needs HIP device tensors: there is no CPU fallback")
    if nq == 0 or nr == 0:
        return NNResult(torch.full(lead, -1, device=q.device, dtype=torch.int32),
                        torch.full(lead, float("inf"), device=q.device, dtype=torch.float32))
    u8 = lambda v: None if v is None else (v.to(torch.uint8) if v.dtype == torch.bool else v).reshape(-1).contiguous()
    idx, sq = ops.nearest_neighbours(q.reshape(nq, 3).contiguous(), r.reshape(nr, 3).contiguous(), u8(qv), u8(rv),
                                     exclude_self=bool(exclude_self))
    return NNResult(idx.reshape(lead), sq.reshape(lead))


def reciprocal_matches(P1, P2, valid1=None, valid2=None):
    """Mutual nearest neighbours of two point sets on the device: the contract of the reference's find_reciprocal_matches
    (omnivggt/utils/geometry.py, two scipy k-d trees on the host) as two searches and one gather.
    -> (reciprocal_in_P2 bool [n2], nn2_in_P1 int32 [n2], count): nn2_in_P1[j] is the point of P1 nearest to P2[j] (-1 where there is
    none), reciprocal_in_P2[j] is True when P2[j] is in turn the point of P2 nearest to P1[nn2_in_P1[j]], count is the 0-d int64
    device tensor of their number. A -1 neighbour is never reciprocal. Ties follow nearest_neighbours (lowest index), so the result
    is deterministic where a k-d tree's is not. P1, P2: float32 (..., 3) device tensors or PointClouds, flattened; valid1 / valid2 as
    in nearest_neighbours. Nothing is read back."""
    nn1_in_P2 = nearest_neighbours(P1, P2, valid1, valid2).index.reshape(-1)
    nn2_in_P1 = nearest_neighbours(P2, P1, valid2, valid1).index.reshape(-1)
    n2 = nn2_in_P1.numel()
    if nn1_in_P2.numel() == 0:
        rec = torch.zeros(n2, device=nn2_in_P1.device, dtype=torch.bool)
    else:
        back = nn1_in_P2[nn2_in_P1.clamp_min(0).long()]
        rec = (nn2_in_P1 >= 0) & (back == torch.arange(n2, device=back.device, dtype=torch.int32))
    return rec, nn2_in_P1, rec.sum()


class CloudDistance:
    """Result of cloud_distance (Python floats and ints). accuracy / accuracy_median: mean / median distance from the predicted points to
    their nearest ground-truth point; completeness / completeness_median: the same from the ground truth to the prediction; chamfer:
    (accuracy + completeness) / 2; n_pred / n_gt: how many points of each cloud found a neighbour and entered the figures. With a
    threshold: precision (share of those predicted points within it), recall (share of those ground-truth points), fscore (their
    harmonic mean, 0 when both are 0); None without."""
    __slots__ = ("accuracy", "accuracy_median", "completeness", "completeness_median", "chamfer", "n_pred", "n_gt", "precision", "recall",
                 "fscore", "threshold")

    def __init__(self, **kw):
        for k in self.__slots__:
            setattr(self, k, kw.get(k))

    def __repr__(self):
        return "CloudDistance(%s)" % ", ".join("%s=%r" % (k, getattr(self, k)) for k in self.__slots__)


def _order_statistic_median(sq):
    """Median of sqrt(sq) in float64 for a 1-D float32 device tensor (len >= 1) through percentile(): sqrt is monotonic, so the middle
    distances are the roots of the middle squared distances, and percentile(., 50) of an odd number of values IS an order statistic
    (no interpolation). An even count is made odd once with -inf in front (-> the lower middle value) and once with +inf behind (->
    the upper one); the median is the mean of the two roots, as numpy.median has it. (Beyond 2^24 values the rank follows numpy's
    float32 index rule, as percentile does.)"""
    n = sq.numel()
    if n % 2:
        return percentile(sq, 50.0).double().sqrt()
    if n == 2:                                                               # the padded forms below would interpolate towards their own +inf
        return sq.double().sqrt().mean()
    buf = torch.empty(n + 2, device=sq.device, dtype=torch.float32)
    buf[0], buf[n + 1] = float("-inf"), float("inf")
    buf[1:n + 1] = sq
    lo, hi = percentile(buf[:n + 1], 50.0), percentile(buf[1:], 50.0)
    return (lo.double().sqrt() + hi.double().sqrt()) / 2


def cloud_distance(pred, gt, threshold=None):
    """Accuracy, completeness, chamfer distance and F-score of a predicted cloud against a ground-truth cloud, the figures by which
    reconstructions are scored, from two exact nearest-neighbour searches on the device (nearest_neighbours) instead of two k-d
    trees on the host. Distances are sqrt(sqdist) in float64, means are float64 sums on the device, medians go through the exact
    percentile(). Points without a neighbour (non-finite coordinates, or an empty other side) are left out of every figure and of
    n_pred / n_gt; a side with no matched point reports nan. threshold: optional positive distance; precision = share of the matched
    predicted points with distance < threshold, recall likewise for the ground truth, fscore = 2 P R / (P + R).
    pred, gt: float32 (..., 3) device tensors or PointClouds. -> CloudDistance (one device -> host read at the end)."""
    if threshold is not None and not (isinstance(threshold, (int, float)) and not isinstance(threshold, bool) and threshold > 0):
        raise ValueError("cloud_distance: threshold must be a positive number or None, got %r" % (threshold,))
    sides = []
    for a, b in ((pred, gt), (gt, pred)):
        res = nearest_neighbours(a, b)
        sq = res.sqdist.reshape(-1)[res.index.reshape(-1) >= 0]
        n = int(sq.numel())
        if n == 0:
            sides.append((float("nan"), float("nan"), 0, float("nan")))
            continue
        d = sq.double().sqrt()
        within = (d < float(threshold)).double().mean() if threshold is not None else d.new_zeros(())
        vals = torch.stack([d.mean(), _order_statistic_median(sq), within]).tolist()
        sides.append((vals[0], vals[1], n, vals[2]))
    (acc, acc_med, n_pred, prec), (comp, comp_med, n_gt, rec) = sides
    out = dict(accuracy=acc, accuracy_median=acc_med, completeness=comp, completeness_median=comp_med, chamfer=(acc + comp) / 2,
               n_pred=n_pred, n_gt=n_gt, threshold=None if threshold is None else float(threshold))
    if threshold is not None:
        out.update(precision=prec, recall=rec, fscore=2 * prec * rec / (prec + rec) if prec + rec > 0 else 0.0)
    return CloudDistance(**out)


# ---------------------------------------------------------------------------------------------------------------------------------
# Radius neighbour search on a hash grid: floater removal and F-score of full clouds (ovg_radius_search)
# ---------------------------------------------------------------------------------------------------------------------------------

# The default work budget of a radius search, in candidate pairs (distances the search evaluates). MEASURED on an MI355X
# (profiles/radius_probe.txt, tools/probes/radius_probe.py): the grid loop evaluates 4.7e10 .. 4.1e11 pairs/s (lowest at 8 neighbours
# per query, where hash probes and short divergent loops dominate). 2^37 = 1.4e11 pairs is the largest power of two that stays under
# 5 s at the LOWEST measured rate (2.9 s); 2^40, the size of the 1 M x 1 M exhaustive search, would be 23 s there. The 64-neighbour
# search inside the full 64-view cloud (17.2 M points) needs 5.2e9.
RADIUS_MAX_PAIRS = 1 << 37


class RadiusResult:
    """Result of radius_neighbours: count int32 (reference points within the radius), index int32 (the nearest of them, -1 where there
    is none) and sqdist float32 (the squared distance to it, +inf where there is none), device tensors shaped like the query without
    its last dimension."""
    __slots__ = ("count", "index", "sqdist")

    def __init__(self, count, index, sqdist):
        self.count, self.index, self.sqdist = count, index, sqdist


def _f32(x):
    import struct
    return struct.unpack("f", struct.pack("f", x))[0]


def _radius_sq(radius, what="radius"):
    """f32(f32(radius)^2), checked: the squared radius exactly as the kernel compares with it."""
    import math
    if isinstance(radius, bool) or not isinstance(radius, (int, float)) or not (radius > 0 and math.isfinite(radius)):
        raise ValueError("%s must be a positive finite number, got %r" % (what, radius))
    try:
        r = _f32(float(radius))
        r2 = _f32(r * r)                                                     # the product of two float32 is exact in float64: one rounding
    except OverflowError:
        r2 = float("inf")
    if not (math.isfinite(r2) and r2 >= 2.0 ** -100):
        raise ValueError("%s %r squares to %r in float32: outside [2^-100, float32 max]" % (what, radius, r2))
    return r2


def _radius_grid(what, query, reference, radius, query_valid, reference_valid, exclude_self, cell_size, origin, max_pairs):
    """The front half radius_neighbours and knn_neighbours share: the argument checks, the grid of the reference cloud (ops.radius_search,
    L.RS_BUILD), the one device -> host read of its statistics and the budget's ValueError.
    -> (lead, device, args, max_pairs): lead the query's leading shape; args the keyword arguments of the search stage over the built
    grid, or None when a side is empty (nothing was launched)."""
    import math
    L = ops.L
    q, r = _nn_points(query, "query"), _nn_points(reference, "reference")
    lead = tuple(q.shape[:-1])
    qv, rv = _nn_valid(query_valid, lead, "query_valid"), _nn_valid(reference_valid, tuple(r.shape[:-1]), "reference_valid")
    nq, nr = q.numel() // 3, r.numel() // 3
    if exclude_self and nq != nr:
        raise ValueError("exclude_self searches inside one cloud: query and reference must hold the same number of points (%d, %d)" % (nq, nr))
    radius_sq = _radius_sq(radius)
    reach = ops.radius_reach(radius_sq)
    if cell_size is None:
        cell = reach
    else:
        if isinstance(cell_size, bool) or not isinstance(cell_size, (int, float)) or not math.isfinite(cell_size):
            raise ValueError("cell_size must be a finite number, got %r" % (cell_size,))
        cell = _f32(float(cell_size))
        if not (cell >= reach and math.isfinite(cell)):
            raise ValueError("cell_size %r is below the reach %r of radius %r (the radius plus its rounding margin)" % (cell_size, reach, radius))
    if max_pairs is None:
        max_pairs = RADIUS_MAX_PAIRS
    if isinstance(max_pairs, bool) or not isinstance(max_pairs, int) or not 0 <= max_pairs < 1 << 63:
        raise ValueError("max_pairs must be a non-negative integer, got %r" % (max_pairs,))
    org = None
    if isinstance(origin, torch.Tensor):
        if origin.dtype != torch.float32 or origin.numel() != 3:
            raise ValueError("origin must hold three float32 values")
        org = origin
    elif origin is not None:
        try:
            vals = [float(v) for v in origin]
        except (TypeError, ValueError):
            raise ValueError("origin must be three finite numbers or a float32 tensor [3], got %r" % (origin,)) from None
        if len(vals) != 3 or not all(math.isfinite(v) and abs(v) <= 3.4028234663852886e38 for v in vals):
            raise ValueError("origin must be three finite float32 numbers, got %r" % (origin,))
    if not all(t is None or t.is_cuda for t in (q, r, qv, rv, org)):
        raise L.OvgError("%s needs HIP device tensors: there is no CPU fallback" % what)
    dev = q.device
    if nq == 0 or nr == 0:
        return lead, dev, None, max_pairs
    if origin is not None and org is None:
        org = torch.tensor(vals, device=dev, dtype=torch.float32)
    elif org is not None:
        org = org.reshape(3).contiguous()
    u8 = lambda v: None if v is None else (v.to(torch.uint8) if v.dtype == torch.bool else v).reshape(-1).contiguous()
    args = dict(query=q.reshape(nq, 3).contiguous(), reference=r.reshape(nr, 3).contiguous(), radius_sq=radius_sq, cell=cell,
                ws=torch.empty(ops.radius_workspace_bytes(nq, nr), device=dev, dtype=torch.uint8), query_valid=u8(qv),
                reference_valid=u8(rv), origin=org, exclude_self=bool(exclude_self))
    stats = ops.radius_search(L.RS_BUILD, **args)[0]
    flags, cells, largest, pairs = (int(v) for v in stats.cpu().tolist())   # the one synchronisation
    if flags & L.RS_BAD_ORIGIN:
        raise ValueError("%s: the origin on the device is not finite" % what)
    if pairs > max_pairs:
        raise ValueError("%s: radius %r makes the search evaluate %d candidate pairs, above the budget of %d (max_pairs); "
                         "the largest of the %d occupied cells holds %d of the %d reference points -- lower the radius, or raise max_pairs "
                         "knowingly" % (what, radius, pairs, max_pairs, cells, largest, nr))
    return lead, dev, args, max_pairs


def radius_neighbours(query, reference, radius, query_valid=None, reference_valid=None, exclude_self=False, cell_size=None, origin=None,
                      max_pairs=None):
    """For every query point the number of reference points within `radius` and the nearest of them, searched through a uniform hash grid
    on the device (ovg_radius_search), so that the cost is linear in the clouds for a sensible radius where nearest_neighbours is
    quadratic. The result is defined WITHOUT the grid, as nearest_neighbours' rule restricted to d <= radius_sq (tests/radius_twin.py
    restates it by brute force): d = (dx dx + dy dy) + dz dz in float32 without fused multiply-adds, radius_sq = f32(f32(radius)^2),
    a usable reference is within the radius when d <= radius_sq (inclusive), the nearest is the smallest d, equal distances go to the
    LOWEST reference index. The grid never changes a byte, nor does cell_size or origin; two calls give identical
    bytes. An unusable query (non-finite coordinates or a zero valid entry), or one with nothing within the radius, gets count 0,
    index -1, sqdist +inf; a distance that overflows float32 is never within a radius.

    query, reference: float32 device tensors (..., 3), or PointClouds; query_valid / reference_valid: optional bool / uint8 tensors
    shaped like the points without the last dimension. exclude_self=True searches inside one cloud (equal sizes): point i does not count
    for itself. cell_size: the grid's cell edge, at least (and by default) the radius plus a rounding margin (ops.radius_reach);
    origin: three finite floats or a float32 device tensor [3] the grid is anchored at (default zeros) -- both move work, not results.
    max_pairs: the work budget (default RADIUS_MAX_PAIRS). A radius too large for the cloud would make single threads walk most of it;
    the grid is built first, the number of candidate pairs (distances the search would evaluate) is read back -- the one device -> host
    synchronisation -- and a count above the budget raises ValueError before the search is launched.

    -> RadiusResult(count int32, index int32, sqdist float32) shaped like the query's leading dimensions. An empty side returns
    zeros / -1 / +inf without a launch. CPU tensors raise OvgError (there is no CPU fallback); a bad radius, cell or shape raises
    ValueError."""
    lead, dev, args, max_pairs = _radius_grid("radius_neighbours", query, reference, radius, query_valid, reference_valid, exclude_self,
                                              cell_size, origin, max_pairs)
    if args is None:
        return RadiusResult(torch.zeros(lead, device=dev, dtype=torch.int32), torch.full(lead, -1, device=dev, dtype=torch.int32),
                            torch.full(lead, float("inf"), device=dev, dtype=torch.float32))
    _, cnt, idx, sq = ops.radius_search(ops.L.RS_SEARCH, max_pairs=max_pairs, **args)
    return RadiusResult(cnt.reshape(lead), idx.reshape(lead), sq.reshape(lead))


def _cloud_radius(what, cloud_or_points, pts, radius, rel_radius):
    """The radius of a search inside a cloud: `radius` as given, or f32(rel_radius) * scene_scale of a PointCloud in one float32
    multiply on the host (which reads scene_scale back)."""
    import math
    if rel_radius is None:
        return radius
    if isinstance(rel_radius, bool) or not isinstance(rel_radius, (int, float)) or not (rel_radius > 0 and math.isfinite(rel_radius)):
        raise ValueError("rel_radius must be a positive finite number, got %r" % (rel_radius,))
    if not isinstance(cloud_or_points, PointCloud) or cloud_or_points.scene_scale is None:
        raise ValueError("rel_radius needs a PointCloud with its scene_scale")
    _radius_sq(rel_radius, "rel_radius")
    if not pts.is_cuda:
        raise ops.L.OvgError("%s needs HIP device tensors: there is no CPU fallback" % what)
    return _f32(_f32(float(rel_radius)) * float(cloud_or_points.scene_scale.to(torch.float32)))


def radius_outlier_mask(cloud_or_points, radius=None, rel_radius=None, min_neighbours=2, valid=None):
    """Radius outlier test of a cloud on the device: True where a point has at least min_neighbours OTHER points within `radius`
    (radius_neighbours inside the cloud with exclude_self; Open3D's remove_radius_outlier counts the point itself, so its nb_points is
    min_neighbours + 1). It judges what multiview_consistency cannot: floaters that a single view sees. Exactly one of radius (in the
    cloud's units) and rel_radius (a PointCloud only: f32(rel_radius) * scene_scale, multiplied on the host) must be given. valid:
    optional bool / uint8 tensor; a point that is not valid or not finite is no neighbour of anything and is itself False.
    -> bool device tensor shaped like the points without the last dimension. Synchronises as radius_neighbours does; errors as there."""
    if (radius is None) == (rel_radius is None):
        raise ValueError("radius_outlier_mask: give exactly one of radius and rel_radius")
    if isinstance(min_neighbours, bool) or not isinstance(min_neighbours, int) or min_neighbours < 1:
        raise ValueError("min_neighbours must be a positive integer, got %r" % (min_neighbours,))
    pts = _nn_points(cloud_or_points, "cloud_or_points")
    _nn_valid(valid, tuple(pts.shape[:-1]), "valid")
    radius = _cloud_radius("radius_outlier_mask", cloud_or_points, pts, radius, rel_radius)
    res = radius_neighbours(pts, pts, radius, valid, valid, exclude_self=True)
    return res.count >= min_neighbours


def remove_radius_outliers(cloud, radius=None, rel_radius=None, min_neighbours=2):
    """A PointCloud without its radius outliers (radius_outlier_mask), in input order: points, colors and conf are gathered, `indices`
    are the input cloud's at the kept points when it has them (so they still name pixels of the prediction maps) and the positions in the
    input cloud otherwise; transform, extrinsic, conf_threshold and scene_scale are passed through unchanged, as
    farthest_point_downsample does. write_ply, write_glb and render_point_cloud accept the result as they are."""
    if not isinstance(cloud, PointCloud):
        raise ValueError("remove_radius_outliers takes a PointCloud")
    return _gather_cloud(cloud, radius_outlier_mask(cloud, radius=radius, rel_radius=rel_radius, min_neighbours=min_neighbours))


def _gather_cloud(cloud, keep):
    """The points of a PointCloud where the bool mask `keep` is True, in input order."""
    M = len(cloud)
    idx = torch.nonzero(keep.reshape(-1)).reshape(-1)
    return PointCloud(cloud.points.reshape(M, 3)[idx], None if cloud.colors is None else cloud.colors.reshape(M, 3)[idx],
                      cloud.conf_threshold, cloud.scene_scale, cloud.transform, cloud.extrinsic,
                      idx if cloud.indices is None else cloud.indices[idx], None if cloud.conf is None else cloud.conf[idx])


def cloud_fscore(pred, gt, threshold, max_pairs=None):
    """Precision, recall and F-score of a predicted cloud against a ground-truth cloud at a distance threshold, with the truncated
    accuracy / completeness / chamfer, from two radius searches on the device (radius_neighbours at radius = threshold): linear in the
    clouds, where cloud_distance's two unbounded exhaustive searches stop at about a million points.
    n_pred / n_gt: the usable points (finite coordinates) of each side. precision: the share of the usable predicted points with a
    ground-truth point within the threshold; recall: the same from the ground truth; fscore = 2 P R / (P + R), 0 when both are 0.
    accuracy / completeness: the float64 mean of min(sqrt(sqdist), threshold) over the usable points of the side (a point with nothing
    within the threshold counts as the threshold: the truncated distance); chamfer their mean. Medians are None; a side without usable
    points reports nan.
    "Within" here is d_f32 <= f32(f32(threshold)^2) on the float32 squared distance, inclusive, where cloud_distance tests
    sqrt(d) < threshold in float64: two functions, two rules, and a point exactly at the threshold may count here and not there.
    pred, gt: float32 (..., 3) device tensors or PointClouds. -> CloudDistance. max_pairs: the budget of each search, as in
    radius_neighbours (ValueError when exceeded)."""
    _radius_sq(threshold, "threshold")
    a, b = _nn_points(pred, "pred"), _nn_points(gt, "gt")
    if not (a.is_cuda and b.is_cuda):
        raise ops.L.OvgError("cloud_fscore needs HIP device tensors: there is no CPU fallback")
    sides = []
    for x, y in ((a, b), (b, a)):
        res = radius_neighbours(x, y, threshold, max_pairs=max_pairs)
        ok = torch.isfinite(x).all(dim=-1).reshape(-1)
        d = res.sqdist.reshape(-1).double().sqrt().clamp_max(float(threshold))
        hits = (res.count.reshape(-1) >= 1) & ok
        n, k, total = torch.stack([ok.sum().double(), hits.sum().double(), torch.where(ok, d, d.new_zeros(())).sum()]).tolist()
        n, k = int(n), int(k)
        sides.append((total / n if n else float("nan"), n, k / n if n else float("nan")))
    (acc, n_pred, prec), (comp, n_gt, rec) = sides
    return CloudDistance(accuracy=acc, completeness=comp, chamfer=(acc + comp) / 2, n_pred=n_pred, n_gt=n_gt, threshold=float(threshold),
                         precision=prec, recall=rec, fscore=2 * prec * rec / (prec + rec) if prec + rec > 0 else 0.0)


# ---------------------------------------------------------------------------------------------------------------------------------
# The k nearest neighbours on the same grid: surface normals and the statistical outlier filter (ovg_knn_search, ovg_knn_normals)
# ---------------------------------------------------------------------------------------------------------------------------------

KNN_MAX_K = ops.L.KNN_MAX_K


class KNNResult:
    """Result of knn_neighbours: count int32 (reference points within the radius, shaped like the query without its last dimension:
    fewer than k were found where count < k), index int32 and sqdist float32 shaped like that plus (k,): the nearest neighbours in
    ascending distance, -1 / +inf from rank min(k, count) on. Device tensors."""
    __slots__ = ("count", "index", "sqdist")

    def __init__(self, count, index, sqdist):
        self.count, self.index, self.sqdist = count, index, sqdist


def _knn_k(k):
    if isinstance(k, bool) or not isinstance(k, int) or not 1 <= k <= KNN_MAX_K:
        raise ValueError("k must be an integer in [1, %d], got %r" % (KNN_MAX_K, k))
    return k


def knn_neighbours(query, reference, k, radius, query_valid=None, reference_valid=None, exclude_self=False, cell_size=None, origin=None,
                   max_pairs=None):
    """For every query point its k nearest reference points among those within `radius` (the hybrid search: Open3D's
    KDTreeSearchParamHybrid), through the hash grid of radius_neighbours on the device (ovg_knn_search). A radius is REQUIRED: it is
    what bounds the cells a query visits, and an unbounded k-nearest search is out of scope; `count` tells whether fewer than k were
    found. The result is defined WITHOUT the grid (tests/knn_twin.py restates it by brute force): with radius_neighbours' float32 d,
    usable points and inclusive d <= radius_sq, the neighbours of a query are its candidates in ascending order of (d, reference
    index) -- nearest first, equal distances in ascending index -- so rank 0 is radius_neighbours' index / sqdist, count is its
    count, and the first k columns of a search with a larger k are the search with k. Two calls give identical bytes; cell_size and
    origin move work, never a result.

    Arguments, the work budget max_pairs with its one device -> host read and ValueError, and the errors are radius_neighbours';
    k is an integer in [1, KNN_MAX_K].

    -> KNNResult(count int32 lead, index int32 lead + (k,), sqdist float32 lead + (k,)), lead the query's leading dimensions. An
    empty side returns zeros / -1 / +inf without a launch."""
    k = _knn_k(k)
    lead, dev, args, max_pairs = _radius_grid("knn_neighbours", query, reference, radius, query_valid, reference_valid, exclude_self,
                                              cell_size, origin, max_pairs)
    if args is None:
        return KNNResult(torch.zeros(lead, device=dev, dtype=torch.int32), torch.full(lead + (k,), -1, device=dev, dtype=torch.int32),
                         torch.full(lead + (k,), float("inf"), device=dev, dtype=torch.float32))
    _, cnt, idx, sq = ops.knn_search(k=k, max_pairs=max_pairs, **args)
    return KNNResult(cnt.reshape(lead), idx.reshape(lead + (k,)), sq.reshape(lead + (k,)))


def estimate_normals(cloud_or_points, k=16, radius=None, rel_radius=None, viewpoint=None, valid=None, return_curvature=False, image_hw=None):
    """Surface normals of a cloud on the device: for every point the plane through its k nearest neighbours within the radius
    (knn_neighbours inside the cloud, the point being its own first neighbour as in Open3D's estimate_normals), by the float64
    covariance of the neighbours and the eigenvector of its smallest eigenvalue (ovg_knn_normals, include/omnivggt_hip.h). A point
    with fewer than three neighbours (itself included), and a point that is not valid or not finite, gets the normal (0, 0, 0).
    Exactly one of radius (in the cloud's units) and rel_radius (a PointCloud only: f32(rel_radius) * scene_scale) must be given, as
    in radius_outlier_mask; valid: optional bool / uint8 tensor, a point that is not valid is no neighbour of anything.
    viewpoint: None -- the normal's component of largest magnitude is made positive (deterministic, not a surface orientation);
    three numbers or a float32 tensor [3] -- every normal points to the half space of that point; a float32 tensor shaped like the
    points -- one viewpoint per point; "cameras" (a PointCloud with `indices` and `extrinsic`, and image_hw=(H, W) of the prediction
    maps) -- every point is oriented towards the centre -R^T t of the camera that saw it, view = indices // (H W) (clamped to the
    cloud's cameras; a cloud of one selected frame uses its one camera), computed on the device.
    -> float32 device tensor shaped like the points, unit normals; with return_curvature also the surface variation
    lambda0 / (lambda0 + lambda1 + lambda2) as a float32 tensor without the last dimension (0 on a plane, at most 1/3).
    Synchronises as radius_neighbours does; errors as there."""
    import math
    k = _knn_k(k)
    if (radius is None) == (rel_radius is None):
        raise ValueError("estimate_normals: give exactly one of radius and rel_radius")
    pts = _nn_points(cloud_or_points, "cloud_or_points")
    lead = tuple(pts.shape[:-1])
    _nn_valid(valid, lead, "valid")
    n = pts.numel() // 3
    view, cams = None, None
    if isinstance(viewpoint, str):
        if viewpoint != "cameras":
            raise ValueError("viewpoint %r: the only named viewpoint is \"cameras\"" % (viewpoint,))
        c = cloud_or_points
        if not isinstance(c, PointCloud) or c.indices is None or c.extrinsic is None:
            raise ValueError("viewpoint=\"cameras\" needs a PointCloud with its indices and extrinsic")
        if (not isinstance(image_hw, (tuple, list)) or len(image_hw) != 2
                or not all(isinstance(v, int) and not isinstance(v, bool) and v > 0 for v in image_hw)):
            raise ValueError("viewpoint=\"cameras\" needs image_hw=(H, W), two positive integers, got %r" % (image_hw,))
        if not isinstance(c.extrinsic, torch.Tensor) or c.extrinsic.dim() != 3 or tuple(c.extrinsic.shape[1:]) != (3, 4) or c.extrinsic.shape[0] < 1:
            raise ValueError("viewpoint=\"cameras\": the cloud's extrinsic must be a tensor (S, 3, 4)")
        if c.indices.numel() != n:
            raise ValueError("viewpoint=\"cameras\": the cloud holds %d indices for %d points" % (c.indices.numel(), n))
        view, cams = c.indices, c.extrinsic
    elif isinstance(viewpoint, torch.Tensor):
        if viewpoint.dtype != torch.float32 or (tuple(viewpoint.shape) != (3,) and tuple(viewpoint.shape) != tuple(pts.shape)):
            raise ValueError("viewpoint must be a float32 tensor [3] or one shaped like the points %r" % (tuple(pts.shape),))
    elif viewpoint is not None:
        try:
            vals = [float(v) for v in viewpoint]
        except (TypeError, ValueError):
            raise ValueError("viewpoint must be three finite numbers, a float32 tensor or \"cameras\", got %r" % (viewpoint,)) from None
        if len(vals) != 3 or not all(math.isfinite(v) and abs(v) <= 3.4028234663852886e38 for v in vals):
            raise ValueError("viewpoint must be three finite float32 numbers, got %r" % (viewpoint,))
    radius = _cloud_radius("estimate_normals", cloud_or_points, pts, radius, rel_radius)
    _radius_sq(radius)
    if not all(t is None or t.is_cuda for t in (pts, valid, viewpoint if isinstance(viewpoint, torch.Tensor) else None, view, cams)):
        raise ops.L.OvgError("estimate_normals needs HIP device tensors: there is no CPU fallback")
    res = knn_neighbours(pts, pts, k, radius, valid, valid)
    dev = pts.device
    if n == 0:
        normal = torch.zeros(lead + (3,), device=dev, dtype=torch.float32)
        return (normal, torch.zeros(lead, device=dev, dtype=torch.float32)) if return_curvature else normal
    if view is not None:
        e = cams.to(torch.float64)
        centres = (-(e[:, :, :3].transpose(1, 2) @ e[:, :, 3:4]).reshape(-1, 3)).to(torch.float32)      # -R^T t, rounded once
        v = torch.div(view.reshape(-1), image_hw[0] * image_hw[1], rounding_mode="floor") if centres.shape[0] > 1 else torch.zeros_like(view.reshape(-1))
        vp = centres[v.clamp(0, centres.shape[0] - 1)].contiguous()
    elif isinstance(viewpoint, torch.Tensor):
        vp = viewpoint.reshape(-1, 3).contiguous() if viewpoint.dim() > 1 else viewpoint.contiguous()
    elif viewpoint is not None:
        vp = torch.tensor(vals, device=dev, dtype=torch.float32)
    else:
        vp = None
    flat = pts.reshape(n, 3).contiguous()
    normal, curv, _, _ = ops.knn_normals(flat, flat, res.index.reshape(n, k), viewpoint=vp, curvature=bool(return_curvature))
    normal = normal.reshape(lead + (3,))
    return (normal, curv.reshape(lead)) if return_curvature else normal


def statistical_outlier_mask(cloud_or_points, k=16, std_ratio=2.0, radius=None, rel_radius=None, valid=None):
    """Statistical outlier test of a cloud on the device: True where a point's mean distance to its k nearest OTHER points is at most
    the cloud's mean of that figure plus std_ratio standard deviations. knn_neighbours runs inside the cloud with exclude_self and a
    radius (exactly one of radius and rel_radius, as in radius_outlier_mask: it bounds the search, choose it a few times the
    expected spacing). A point with count < k -- fewer than k others within the radius, or not valid, or not finite -- is an outlier
    and takes no part in the statistics. For the others a_i = the float64 mean of sqrt(float64(sqdist)) over the k ranks,
    thr = mean(a) + std_ratio * std(a) with the population standard deviation in float64, and the mask is a_i <= thr.
    Open3D's remove_statistical_outlier counts the point itself among its nb_neighbors (at distance 0), so its nb_neighbors is
    k + 1 and its mean distance is ours times k / (k + 1); mean and deviation scale alike, so the kept set is the same for the
    same std_ratio, but for the radius bound, which Open3D's unbounded search does not have.
    -> bool device tensor shaped like the points without the last dimension. Synchronises as radius_neighbours does; errors as there."""
    import math
    k = _knn_k(k)
    if isinstance(std_ratio, bool) or not isinstance(std_ratio, (int, float)) or not (std_ratio >= 0 and math.isfinite(std_ratio)):
        raise ValueError("std_ratio must be a non-negative finite number, got %r" % (std_ratio,))
    if (radius is None) == (rel_radius is None):
        raise ValueError("statistical_outlier_mask: give exactly one of radius and rel_radius")
    pts = _nn_points(cloud_or_points, "cloud_or_points")
    _nn_valid(valid, tuple(pts.shape[:-1]), "valid")
    radius = _cloud_radius("statistical_outlier_mask", cloud_or_points, pts, radius, rel_radius)
    res = knn_neighbours(pts, pts, k, radius, valid, valid, exclude_self=True)
    full = res.count >= k
    a = res.sqdist.to(torch.float64).sqrt().sum(-1) / k                      # ranks in ascending order; +inf where a row is not full
    sel = a[full]
    if sel.numel() == 0:
        return full
    mean = sel.mean()
    thr = mean + float(std_ratio) * ((sel - mean) ** 2).mean().sqrt()
    return full & (a <= thr)


def remove_statistical_outliers(cloud, k=16, std_ratio=2.0, radius=None, rel_radius=None):
    """A PointCloud without its statistical outliers (statistical_outlier_mask), in input order, gathered as remove_radius_outliers
    gathers: points, colors and conf at the kept points, `indices` the input cloud's there (or the positions in the input cloud when
    it has none), everything else passed through. write_ply, write_glb and render_point_cloud accept the result as they are."""
    if not isinstance(cloud, PointCloud):
        raise ValueError("remove_statistical_outliers takes a PointCloud")
    return _gather_cloud(cloud, statistical_outlier_mask(cloud, k=k, std_ratio=std_ratio, radius=radius, rel_radius=rel_radius))


# ---------------------------------------------------------------------------------------------------------------------------------
# Clustering on the same grid: Euclidean connected components and DBSCAN, "keep the main structure" (ovg_cluster)
# ---------------------------------------------------------------------------------------------------------------------------------

CL_UNUSABLE, CL_NOISE, CL_BORDER, CL_CORE = ops.L.CL_UNUSABLE, ops.L.CL_NOISE, ops.L.CL_BORDER, ops.L.CL_CORE


class ClusterResult:
    """Result of cluster_points. Shaped like the points without their last dimension, device tensors: labels int32 (the dense cluster
    number, -1 for noise and unusable points), kind uint8 (CL_UNUSABLE / CL_NOISE / CL_BORDER / CL_CORE), root int32 (the lowest
    point index of the point's cluster, -1 where labels is -1) and degree int32 (the other points within the radius). Per cluster,
    in label order: roots int32 [C] and sizes int64 [C] (core and border points). num_clusters: C, a host int."""
    __slots__ = ("labels", "kind", "root", "degree", "roots", "sizes", "num_clusters")

    def __init__(self, labels, kind, root, degree, roots, sizes, num_clusters):
        self.labels, self.kind, self.root, self.degree = labels, kind, root, degree
        self.roots, self.sizes, self.num_clusters = roots, sizes, num_clusters


def _min_neighbours(min_neighbours):
    if isinstance(min_neighbours, bool) or not isinstance(min_neighbours, int) or not 0 <= min_neighbours < 1 << 31:
        raise ValueError("min_neighbours must be a non-negative integer, got %r" % (min_neighbours,))
    return min_neighbours


def cluster_points(cloud_or_points, radius=None, rel_radius=None, min_neighbours=0, valid=None, order="size", cell_size=None, origin=None,
                   max_pairs=None):
    """Which points of a cloud belong together, on the device (ovg_cluster over the hash grid of radius_neighbours): Euclidean
    connected components (min_neighbours = 0) or DBSCAN. The result is defined WITHOUT the grid and without the union-find that
    computes it (tests/cluster_twin.py restates it by brute force), with radius_neighbours' float32 d, usable points and inclusive
    d <= radius_sq: two usable points are neighbours when they are within the radius of each other; a point with at least
    min_neighbours OTHER points within the radius is a core point (Open3D's cluster_dbscan counts the point itself: its min_points is
    min_neighbours + 1); the clusters are the connected components of the core points under the neighbour relation; a usable point
    that is not core but has a core neighbour is a border point and joins the cluster of its NEAREST core neighbour, equal distances
    going to the lowest index (classic DBSCAN leaves this to the visiting order; here two calls, and any schedule, give identical
    bytes); every other usable point is noise. A cluster is named by its lowest point index (`root`).

    Exactly one of radius (in the cloud's units) and rel_radius (a PointCloud only: f32(rel_radius) * scene_scale) must be given, as
    in radius_outlier_mask. valid: optional bool / uint8 tensor; a point that is not valid or not finite is no neighbour of anything.
    order: "size" (default) numbers the clusters by descending size, equal sizes by ascending root, so label 0 is the largest
    cluster; "index" numbers them by ascending root. cell_size, origin and max_pairs are radius_neighbours': they move work, never a
    result, and the budget's one device -> host read and ValueError are the same (the dense labels read the number of clusters back
    as well).

    -> ClusterResult. An empty cloud returns empty results without a launch. CPU tensors raise OvgError (there is no CPU fallback);
    a bad radius, cell, order or shape raises ValueError."""
    if (radius is None) == (rel_radius is None):
        raise ValueError("cluster_points: give exactly one of radius and rel_radius")
    min_neighbours = _min_neighbours(min_neighbours)
    if order not in ("size", "index"):
        raise ValueError("order must be \"size\" or \"index\", got %r" % (order,))
    pts = _nn_points(cloud_or_points, "cloud_or_points")
    _nn_valid(valid, tuple(pts.shape[:-1]), "valid")
    radius = _cloud_radius("cluster_points", cloud_or_points, pts, radius, rel_radius)
    lead, dev, args, max_pairs = _radius_grid("cluster_points", pts, pts, radius, valid, valid, True, cell_size, origin, max_pairs)
    if args is None:
        none = torch.full(lead, -1, device=dev, dtype=torch.int32)
        return ClusterResult(none, torch.zeros(lead, device=dev, dtype=torch.uint8), none.clone(), torch.zeros(lead, device=dev, dtype=torch.int32),
                             torch.zeros(0, device=dev, dtype=torch.int32), torch.zeros(0, device=dev, dtype=torch.int64), 0)
    stats = torch.zeros(4, device=dev, dtype=torch.int64)
    _, root, kind, degree = ops.cluster(args["query"], args["radius_sq"], args["cell"], args["ws"], min_neighbours, valid=args["query_valid"],
                                        origin=args["origin"], max_pairs=max_pairs, out_stats=stats)
    member = root >= 0
    roots, inverse, sizes = torch.unique(root[member], return_inverse=True, return_counts=True)       # ascending root
    if int(stats[0]) & ops.L.CL_INTERNAL:
        raise ops.L.OvgError("cluster_points: the union-find left its bounds (OVG_CL_INTERNAL): no result")
    if order == "size":
        by_size = torch.sort(sizes, descending=True, stable=True).indices                            # equal sizes: ascending root
        rank = torch.empty_like(by_size)
        rank[by_size] = torch.arange(by_size.numel(), device=dev)
        roots, sizes, inverse = roots[by_size], sizes[by_size], rank[inverse]
    labels = torch.full_like(root, -1)
    labels[member] = inverse.to(torch.int32)
    return ClusterResult(labels.reshape(lead), kind.reshape(lead), root.reshape(lead), degree.reshape(lead), roots, sizes.to(torch.int64),
                         int(roots.numel()))


def _cluster_result(result):
    if not isinstance(result, ClusterResult):
        raise ValueError("expected the ClusterResult of cluster_points")
    return result


def largest_cluster_mask(result):
    """True at the points (core and border) of the largest cluster of a ClusterResult, equal sizes going to the lowest root; all
    False when there is no cluster. -> bool tensor shaped like result.labels."""
    res = _cluster_result(result)
    if res.num_clusters == 0:
        return torch.zeros_like(res.labels, dtype=torch.bool)
    top = res.roots[res.sizes == res.sizes.max()].min()                          # whatever the order of the labels
    return res.root == top


def cluster_size_mask(result, min_size):
    """True at the points of the clusters of a ClusterResult that hold at least min_size points (core and border); noise and unusable
    points are False. -> bool tensor shaped like result.labels."""
    res = _cluster_result(result)
    if isinstance(min_size, bool) or not isinstance(min_size, int) or min_size < 1:
        raise ValueError("min_size must be a positive integer, got %r" % (min_size,))
    if res.num_clusters == 0:
        return torch.zeros_like(res.labels, dtype=torch.bool)
    return (res.labels >= 0) & (res.sizes[res.labels.clamp_min(0).long()] >= min_size)


def remove_small_clusters(cloud, radius=None, rel_radius=None, min_size=None, keep_largest=None, min_neighbours=0):
    """A PointCloud without its detached islands, in input order: the points of the clusters (cluster_points) with at least min_size
    points, or with keep_largest=True the largest cluster alone -- the floater islands that radius_outlier_mask and
    statistical_outlier_mask pass, because inside an island every point has neighbours. Exactly one of min_size / keep_largest and
    exactly one of radius / rel_radius must be given. Gathered as remove_radius_outliers gathers: points, colors and conf at the
    kept points, `indices` the input cloud's there (or the positions in the input cloud when it has none), everything else passed
    through. write_ply, write_glb and render_point_cloud accept the result as they are."""
    if not isinstance(cloud, PointCloud):
        raise ValueError("remove_small_clusters takes a PointCloud")
    if keep_largest is not None and not isinstance(keep_largest, bool):
        raise ValueError("keep_largest must be True, False or None, got %r" % (keep_largest,))
    if (min_size is None) == (not keep_largest):
        raise ValueError("remove_small_clusters: give exactly one of min_size and keep_largest")
    if min_size is not None and (isinstance(min_size, bool) or not isinstance(min_size, int) or min_size < 1):
        raise ValueError("min_size must be a positive integer, got %r" % (min_size,))
    res = cluster_points(cloud, radius=radius, rel_radius=rel_radius, min_neighbours=min_neighbours)
    return _gather_cloud(cloud, largest_cluster_mask(res) if keep_largest else cluster_size_mask(res, min_size))


def cluster_colors(labels):
    """A colour per cluster label for write_ply, write_glb and render_point_cloud: uint8 [..., 3] from an integer tensor of labels, a
    fixed integer hash of the label (the same label is the same colour in every call, channels in [56, 255]); noise (a negative
    label) is grey (128, 128, 128). A few torch integer operations on the labels' device."""
    if not isinstance(labels, torch.Tensor) or labels.dtype not in (torch.int32, torch.int64):
        raise ValueError("labels must be an int32 / int64 tensor")
    h = ((labels.to(torch.int64) + 1) * 2654435761) & 0xFFFFFFFF
    h = ((h ^ (h >> 15)) * 0x2C1B3C6D) & 0xFFFFFFFF
    h = ((h ^ (h >> 12)) * 0x297A2D39) & 0xFFFFFFFF
    h = h ^ (h >> 15)
    rgb = torch.stack([h & 255, (h >> 8) & 255, (h >> 16) & 255], -1)
    rgb = 56 + ((rgb * 200) >> 8)
    return torch.where((labels < 0).unsqueeze(-1), torch.full_like(rgb, 128), rgb).to(torch.uint8)


# ---------------------------------------------------------------------------------------------------------------------------------
# Registration: the similarity / rigid transform between paired points, ICP, aligned scores (ovg_align_moments / _solve / _apply)
# ---------------------------------------------------------------------------------------------------------------------------------

ALIGN_FEW_PAIRS, ALIGN_NO_SPREAD, ALIGN_NOT_FINITE = ops.L.ALIGN_FEW_PAIRS, ops.L.ALIGN_NO_SPREAD, ops.L.ALIGN_NOT_FINITE


class Similarity:
    """A transform q ~ s R p + t between two frames, all on the device: matrix float64 (4, 4) = [s R, t; 0 0 0 1]; scale (0-d float64: s),
    count (0-d int64: the pairs the last fit used), rms (0-d float64: their root mean square distance BEFORE that fit's step) and status
    (0-d int32: 0, or ALIGN_FEW_PAIRS | ALIGN_NO_SPREAD | ALIGN_NOT_FINITE when the fit was degenerate and its step the identity)."""
    __slots__ = ("matrix", "scale", "count", "rms", "status")

    def __init__(self, matrix, scale, count, rms, status):
        self.matrix, self.scale, self.count, self.rms, self.status = matrix, scale, count, rms, status

    @classmethod
    def identity(cls, device, status=0):
        return cls(torch.eye(4, device=device, dtype=torch.float64), torch.ones((), device=device, dtype=torch.float64),
                   torch.zeros((), device=device, dtype=torch.int64), torch.zeros((), device=device, dtype=torch.float64),
                   torch.full((), status, device=device, dtype=torch.int32))

    def apply(self, points_or_cloud):
        """float32(matrix p) for every point (ovg_align_apply: float64 arithmetic, one rounding): a float32 tensor shaped like the input, or
        for a PointCloud a new cloud with the moved points and every other field carried over."""
        pts = _nn_points(points_or_cloud, "points_or_cloud")
        if not (pts.is_cuda and self.matrix.is_cuda):
            raise ops.L.OvgError("Similarity.apply needs HIP device tensors: there is no CPU fallback")
        n = pts.numel() // 3
        out = ops.align_apply(pts.reshape(n, 3).contiguous(), self.matrix.contiguous()).reshape(pts.shape) if n else pts.clone()
        if isinstance(points_or_cloud, PointCloud):
            c = points_or_cloud
            return PointCloud(out, c.colors, c.conf_threshold, c.scene_scale, c.transform, c.extrinsic, c.indices, c.conf)
        return out


class ICPResult:
    """Result of icp: transform (a Similarity: the final source -> target transform, with the last iteration's count, rms and status and
    the scale of the whole matrix), and per iteration rms float64, count int64 and status int32 device tensors [iterations]: the used
    pairs of each iteration and their root mean square distance before that iteration's step."""
    __slots__ = ("transform", "rms", "count", "status")

    def __init__(self, transform, rms, count, status):
        self.transform, self.rms, self.count, self.status = transform, rms, count, status


def _u8_flat(v):
    return None if v is None else (v.to(torch.uint8) if v.dtype == torch.bool else v).reshape(-1).contiguous()


def _align_step(src, tgt, with_scale, transform, compose, index=None, source_valid=None, target_valid=None, sqdist=None, max_sqdist=None,
                scale=None, rms=None, count=None, status=None):
    """Two moment passes and the solve for contiguous [n, 3] / [m, 3] device tensors: the first pass without a centre gives the means of
    the used pairs, the second is centred on them (so no sum loses the cloud's extent against its offset), the solve adds them back."""
    kw = dict(index=index, source_valid=source_valid, target_valid=target_valid, sqdist=sqdist, max_sqdist=max_sqdist)
    ws = torch.empty(ops.align_workspace_bytes(src.shape[0]), device=src.device, dtype=torch.uint8)
    n0, s0 = ops.align_moments(src, tgt, ws=ws, **kw)
    centre = s0[:6] / n0.clamp_min(1).to(torch.float64)
    n1, s1 = ops.align_moments(src, tgt, centre=centre, ws=ws, **kw)
    return ops.align_solve(n1, s1, transform, centre=centre, with_scale=with_scale, compose=compose, scale=scale, rms=rms, out_count=count,
                           status=status)


def fit_similarity(source, target, source_valid=None, target_valid=None, with_scale=True):
    """The least-squares similarity (with_scale=True: Umeyama's Sim(3) fit) or rigid transform that takes `source` onto `target`, point i
    onto point i, on the device: the float64 moments of the pairs summed in a fixed order (ovg_align_moments: two calls give the same
    bytes), first about the origin, then about the means of the first pass, and Horn's quaternion solve (ovg_align_solve), which
    always returns a proper rotation -- for mirrored clouds the reflection-corrected Umeyama solution. A pair is used when its six
    coordinates are finite and its valid entries (if given) are non-zero.

    source, target: float32 device tensors (..., 3) with the same number of points, or PointClouds; source_valid / target_valid:
    optional bool / uint8 tensors shaped like the points without the last dimension. -> Similarity. Fewer than three used pairs, a
    source without spread or a non-finite sum give the identity with `status` set, never a NaN. No device -> host synchronisation.
    CPU tensors raise OvgError (there is no CPU fallback); bad shapes or dtypes raise ValueError; empty sides return the identity with
    count 0 and ALIGN_FEW_PAIRS."""
    a, b = _nn_points(source, "source"), _nn_points(target, "target")
    sv = _nn_valid(source_valid, tuple(a.shape[:-1]), "source_valid")
    tv = _nn_valid(target_valid, tuple(b.shape[:-1]), "target_valid")
    n, m = a.numel() // 3, b.numel() // 3
    if n != m:
        raise ValueError("fit_similarity pairs point i with point i: source and target must hold the same number of points (%d, %d)" % (n, m))
    if not all(t is None or t.is_cuda for t in (a, b, sv, tv)):
        raise ops.L.OvgError("fit_similarity needs HIP device tensors: there is no CPU fallback")
    out = Similarity.identity(a.device, ALIGN_FEW_PAIRS)
    if n == 0:
        return out
    scale, rms, count, status = (torch.empty(1, device=a.device, dtype=d) for d in (torch.float64, torch.float64, torch.int64, torch.int32))
    _align_step(a.reshape(n, 3).contiguous(), b.reshape(n, 3).contiguous(), bool(with_scale), out.matrix, False, source_valid=_u8_flat(sv),
                target_valid=_u8_flat(tv), scale=scale, rms=rms, count=count, status=status)
    return Similarity(out.matrix, scale[0], count[0], rms[0], status[0])


def _align_init(init):
    """The matrix of icp's `init` (None: none), checked."""
    m = init.matrix if isinstance(init, Similarity) else init
    if m is not None and (not isinstance(m, torch.Tensor) or m.dtype != torch.float64 or tuple(m.shape) != (4, 4)):
        raise ValueError("init must be None, a Similarity or a float64 tensor (4, 4)")
    return m


def icp(source, target, init=None, iterations=20, max_distance=None, with_scale=False, search="exhaustive"):
    """Point-to-point ICP on the device: `iterations` times, the source is moved by the running transform (ovg_align_apply), every moved
    point finds its nearest target point, the moments of those pairs -- gated at f32(f32(max_distance)^2) on the search's float32 squared
    distance, inclusive -- give the rigid (with_scale=True: similarity) step as in fit_similarity, and the step is multiplied onto the
    running float64 transform on the device. The iteration count is fixed: nothing is tested on the host, and an iteration that is left
    with fewer than three pairs is an identity step with its status set.
    search="exhaustive" uses nearest_neighbours (quadratic; max_distance may be None: no gate) and the whole loop runs without a device
    -> host synchronisation. search="grid" uses radius_neighbours with radius max_distance (required), linear in the clouds for a sensible
    radius; it builds the grid anew and reads the grid's statistics back ONCE PER ITERATION, as every radius_neighbours call does, and
    raises that function's ValueError when the radius is too large for its work budget. Both searches return the same pairs wherever
    the nearest point lies within max_distance.
    source, target: float32 device tensors (..., 3) or PointClouds; init: None (identity), a Similarity or a float64 device tensor
    (4, 4). -> ICPResult. CPU tensors raise OvgError; bad arguments raise ValueError; an empty side returns `init` with zero counts and
    ALIGN_FEW_PAIRS in every iteration."""
    a, b = _nn_points(source, "source"), _nn_points(target, "target")
    if isinstance(iterations, bool) or not isinstance(iterations, int) or iterations < 1:
        raise ValueError("iterations must be a positive integer, got %r" % (iterations,))
    if search not in ("exhaustive", "grid"):
        raise ValueError("search must be 'exhaustive' or 'grid', got %r" % (search,))
    if max_distance is None:
        if search == "grid":
            raise ValueError("search='grid' needs max_distance: it is the radius of the search")
        max_sq = None
    else:
        max_sq = _radius_sq(max_distance, "max_distance")
    T = _align_init(init)
    if not (a.is_cuda and b.is_cuda and (T is None or T.is_cuda)):
        raise ops.L.OvgError("icp needs HIP device tensors: there is no CPU fallback")
    dev = a.device
    T = torch.eye(4, device=dev, dtype=torch.float64) if T is None else T.clone().contiguous()
    n, m = a.numel() // 3, b.numel() // 3
    rms = torch.zeros(iterations, device=dev, dtype=torch.float64)
    count = torch.zeros(iterations, device=dev, dtype=torch.int64)
    status = torch.full((iterations,), ALIGN_FEW_PAIRS, device=dev, dtype=torch.int32)
    scale = torch.empty(1, device=dev, dtype=torch.float64)
    if n and m:
        src, tgt = a.reshape(n, 3).contiguous(), b.reshape(m, 3).contiguous()
        moved = torch.empty_like(src)
        for it in range(iterations):
            ops.align_apply(src, T, out=moved)
            if search == "exhaustive":
                index, sqdist = ops.nearest_neighbours(moved, tgt)
            else:
                res = radius_neighbours(moved, tgt, max_distance)
                index, sqdist = res.index, res.sqdist
            _align_step(moved, tgt, bool(with_scale), T, True, index=index, sqdist=None if max_sq is None else sqdist, max_sqdist=max_sq,
                        scale=scale, rms=rms[it:it + 1], count=count[it:it + 1], status=status[it:it + 1])
    total = torch.linalg.vector_norm(T[:3, 0])
    return ICPResult(Similarity(T, total, count[-1], rms[-1], status[-1]), rms, count, status)


def aligned_cloud_distance(pred_points, gt_points, valid=None, threshold=None, with_scale=True, icp_iterations=0, max_distance=None):
    """The scores of cloud_distance after the alignment they presuppose: a fit_similarity over corresponding points (pixel i of the
    predicted point map against pixel i of the ground truth; with_scale=True is the Sim(3) Umeyama fit), optionally refined by
    `icp_iterations` rigid ICP iterations (exhaustive search, gated at max_distance when given), then cloud_distance of the moved
    prediction against the ground truth. valid: optional bool / uint8 tensor shaped like the points without the last dimension: only
    those pixels are fitted and scored (selecting them synchronises once, as cloud_distance's own read does at the end).
    pred_points, gt_points: float32 device tensors (..., 3) with the same number of points. -> (CloudDistance, Similarity)."""
    a, b = _nn_points(pred_points, "pred_points"), _nn_points(gt_points, "gt_points")
    if a.numel() != b.numel():
        raise ValueError("aligned_cloud_distance pairs point i with point i: %d predicted, %d ground-truth points" % (a.numel() // 3, b.numel() // 3))
    v = _nn_valid(valid, tuple(a.shape[:-1]), "valid")
    if isinstance(icp_iterations, bool) or not isinstance(icp_iterations, int) or icp_iterations < 0:
        raise ValueError("icp_iterations must be a non-negative integer, got %r" % (icp_iterations,))
    if not all(t is None or t.is_cuda for t in (a, b, v)):
        raise ops.L.OvgError("aligned_cloud_distance needs HIP device tensors: there is no CPU fallback")
    a, b = a.reshape(-1, 3), b.reshape(-1, 3)
    if v is not None:
        keep = v.reshape(-1) != 0
        a, b = a[keep], b[keep]
    sim = fit_similarity(a, b, with_scale=with_scale)
    if icp_iterations:
        sim = icp(a, b, init=sim, iterations=icp_iterations, max_distance=max_distance, with_scale=False).transform
    return cloud_distance(sim.apply(a), b, threshold=threshold), sim


def trajectory_ate(pred_extrinsic, gt_extrinsic, with_scale=True):
    """Absolute trajectory error of predicted cameras against ground truth after the alignment evo's align(correct_scale=True) makes:
    the camera centres -R^T t of the world-to-camera matrices (float64 on the device, rounded to float32 for the fit), a fit_similarity
    of the predicted centres onto the true ones (with_scale=False: rigid), and the root mean square distance of the moved centres in
    float64. pred_extrinsic, gt_extrinsic: float32 / float64 device tensors (S, 3, 4) or (S, 4, 4) with the same S.
    -> (ate_rms 0-d float64 device tensor, Similarity). Nothing is read back."""
    cs = []
    for e, name in ((pred_extrinsic, "pred_extrinsic"), (gt_extrinsic, "gt_extrinsic")):
        if not isinstance(e, torch.Tensor) or e.dim() != 3 or tuple(e.shape[1:]) not in ((3, 4), (4, 4)) or e.dtype not in (torch.float32, torch.float64):
            raise ValueError("%s must be a float32 / float64 tensor (S, 3, 4) or (S, 4, 4)" % name)
        cs.append(e)
    if cs[0].shape[0] != cs[1].shape[0]:
        raise ValueError("trajectory_ate pairs camera i with camera i: %d predicted, %d ground-truth cameras" % (cs[0].shape[0], cs[1].shape[0]))
    if not (cs[0].is_cuda and cs[1].is_cuda):
        raise ops.L.OvgError("trajectory_ate needs HIP device tensors: there is no CPU fallback")
    cp, cg = (-(e[:, :3, :3].double().transpose(1, 2) @ e[:, :3, 3:].double()).squeeze(-1) for e in cs)
    sim = fit_similarity(cp.float(), cg.float(), with_scale=with_scale)
    if cp.shape[0] == 0:
        return torch.full((), float("nan"), device=cp.device, dtype=torch.float64), sim
    moved = cp @ sim.matrix[:3, :3].T + sim.matrix[:3, 3]
    return ((moved - cg) ** 2).sum(1).mean().sqrt(), sim


# ---------------------------------------------------------------------------------------------------------------------------------
# Long sequences: a robust weighted Sim(3) fit, and overlapping chunks stitched into the first chunk's frame (ovg_align_wmoments /
# _wsolve / _move_maps / _move_cameras)
# ---------------------------------------------------------------------------------------------------------------------------------

class RobustFit:
    """Result of fit_similarity_robust: transform (a Similarity: the last regular fit, with the last iteration's count, rms and status)
    and, per iteration k = 0 .. iterations, device tensors [iterations + 1]: fit_rms float64 (the weighted root mean square residual
    after fit k), rms float64 (the same under the transform the weights of fit k came from: the identity for k = 0), weight float64
    (the weight sum W), effective_pairs float64 (W^2 / sum of W_i^2: how many pairs carry the fit), count int64 (used pairs) and
    status int32 (ALIGN_* bits; a degenerate refit keeps the previous transform)."""
    __slots__ = ("transform", "fit_rms", "rms", "weight", "effective_pairs", "count", "status")

    def __init__(self, transform, fit_rms, rms, weight, effective_pairs, count, status):
        self.transform, self.fit_rms, self.rms, self.weight = transform, fit_rms, rms, weight
        self.effective_pairs, self.count, self.status = effective_pairs, count, status

    @classmethod
    def identity(cls, device, iterations=0):
        k = iterations + 1
        z = lambda dt: torch.zeros(k, device=device, dtype=dt)
        return cls(Similarity.identity(device), z(torch.float64), z(torch.float64), z(torch.float64), z(torch.float64), z(torch.int64), z(torch.int32))


def _robust_number(name, v, allow_none=False):
    if v is None and allow_none:
        return None
    if isinstance(v, bool) or not isinstance(v, (int, float)) or not (v > 0) or v == float("inf"):
        raise ValueError("%s must be a positive finite number, got %r" % (name, v))
    return float(v)


def fit_similarity_robust(source, target, weights=None, source_valid=None, target_valid=None, with_scale=True, iterations=6, rel_delta=0.5,
                          delta=None):
    """fit_similarity made robust by iteratively reweighted least squares, on the device: iteration 0 is the weighted least-squares
    fit (weights: an optional float32 tensor shaped like the points without the last dimension; a pair whose weight is not finite
    and positive is not used; for weights=None iteration 0 is fit_similarity's transform byte for byte). Iteration k >= 1 multiplies
    every pair's weight by the Cauchy weight 1 / (1 + r^2 / delta^2) of its residual r under the previous transform and fits again,
    always source -> target. delta is rel_delta times the previous fit's weighted rms residual -- read on the device, nothing comes
    back to the host -- or the absolute `delta` when one is given. Each iteration is two moment passes (the first about the origin
    gives the weighted means the second is centred on) and one solve; a degenerate refit keeps the last regular transform. The
    iteration count is fixed.

    The defaults (Cauchy, rel_delta 0.5, six refits) come from a synthetic experiment -- 30 % one-sided outliers of up to the cloud's
    extent, where the plain fit is off by 0.15 and the refits reach the noise floor after five rounds -- and
    are NOT tuned on real predictions.

    -> RobustFit. CPU tensors raise OvgError (there is no CPU fallback); bad shapes, dtypes or numbers raise ValueError; empty sides
    return the identity with ALIGN_FEW_PAIRS in every iteration. No device -> host synchronisation."""
    a, b = _nn_points(source, "source"), _nn_points(target, "target")
    sv = _nn_valid(source_valid, tuple(a.shape[:-1]), "source_valid")
    tv = _nn_valid(target_valid, tuple(b.shape[:-1]), "target_valid")
    n, m = a.numel() // 3, b.numel() // 3
    if n != m:
        raise ValueError("fit_similarity_robust pairs point i with point i: source and target must hold the same number of points (%d, %d)" % (n, m))
    if weights is not None and (not isinstance(weights, torch.Tensor) or weights.dtype != torch.float32 or weights.numel() != n):
        raise ValueError("weights must be None or a float32 tensor with one entry per point")
    if isinstance(iterations, bool) or not isinstance(iterations, int) or iterations < 0:
        raise ValueError("iterations must be a non-negative integer, got %r" % (iterations,))
    rel_delta, delta = _robust_number("rel_delta", rel_delta), _robust_number("delta", delta, allow_none=True)
    if not all(t is None or t.is_cuda for t in (a, b, sv, tv, weights)):
        raise ops.L.OvgError("fit_similarity_robust needs HIP device tensors: there is no CPU fallback")
    dev, K = a.device, iterations + 1
    out = RobustFit.identity(dev, iterations)
    out.status.fill_(ALIGN_FEW_PAIRS)
    out.transform.status.fill_(ALIGN_FEW_PAIRS)
    if n == 0:
        return out
    src, tgt = a.reshape(n, 3).contiguous(), b.reshape(n, 3).contiguous()
    kw = dict(weight=None if weights is None else weights.reshape(-1).contiguous(), source_valid=_u8_flat(sv), target_valid=_u8_flat(tv),
              ws=torch.empty(ops.align_wmoments_workspace_bytes(n), device=dev, dtype=torch.uint8))
    T, scale = out.transform.matrix, torch.ones(1, device=dev, dtype=torch.float64)
    sums, n0, s0 = torch.empty(K, ops.L.WALIGN_SUMS, device=dev, dtype=torch.float64), None, None
    for k in range(K):
        if k:                                                                # the weights of fit k: the residuals under fit k - 1
            kw.update(transform=T, cauchy=True, delta=out.fit_rms[k - 1:k] if delta is None else None,
                      delta_scale=rel_delta if delta is None else delta)
        n0, s0 = ops.align_wmoments(src, tgt, count=n0, sums=s0, **kw)
        centre = s0[:6] / torch.where(s0[18] > 0, s0[18], torch.ones_like(s0[18]))
        ops.align_wmoments(src, tgt, centre=centre, count=out.count[k:k + 1], sums=sums[k], **kw)
        ops.align_wsolve(out.count[k:k + 1], sums[k], T, centre=centre, with_scale=bool(with_scale), keep=k > 0, scale=scale,
                         rms=out.rms[k:k + 1], fit_rms=out.fit_rms[k:k + 1], weight=out.weight[k:k + 1], status=out.status[k:k + 1])
    w2 = sums[:, 19]
    out.effective_pairs = torch.where(w2 > 0, out.weight * out.weight / torch.where(w2 > 0, w2, torch.ones_like(w2)), torch.zeros_like(w2))
    out.transform = Similarity(T, scale[0], out.count[-1], out.rms[-1], out.status[-1])
    return out


def chunk_plan(S, chunk_size, overlap):
    """The chunks of a sequence of S views -> [(start, end)]: chunk c starts at c (chunk_size - overlap) and ends at
    min(start + chunk_size, S); the last chunk is the first whose end is S. Consecutive chunks share exactly `overlap` views, every
    chunk adds at least one new view, S <= chunk_size gives one chunk. ValueError unless 0 < overlap < chunk_size and S >= 1."""
    for name, v in (("S", S), ("chunk_size", chunk_size), ("overlap", overlap)):
        if isinstance(v, bool) or not isinstance(v, int):
            raise ValueError("%s must be an integer, got %r" % (name, v))
    if not (0 < overlap < chunk_size and S >= 1):
        raise ValueError("chunk_plan needs 0 < overlap < chunk_size and S >= 1, got S=%d, chunk_size=%d, overlap=%d" % (S, chunk_size, overlap))
    plan, start = [], 0
    while True:
        end = min(start + chunk_size, S)
        plan.append((start, end))
        if end == S:
            return plan
        start += chunk_size - overlap


def chunk_indices(index, start, end):
    """The entries of a global view index list that fall into the chunk [start, end), as the chunk's local indices, in the list's order."""
    return [int(i) - start for i in (index or []) if start <= int(i) < end]


_STITCH_MAPS = (("world_points", 5), ("world_points_conf", 4), ("depth", 5), ("depth_conf", 4))


def _stitch_check(chunks, plan, prediction_mode, conf_percentile, weights, select):
    """The arguments of stitch_predictions -> (the plan as tuples, S, (H, W), the map keys every chunk carries, pointmap mode, whether
    every tensor is on the device)."""
    if not isinstance(prediction_mode, str):
        raise ValueError("prediction_mode must be a string, got %r" % (prediction_mode,))
    if select not in ("first", "last"):
        raise ValueError("select must be 'first' or 'last', got %r" % (select,))
    if weights not in ("confidence", None):
        raise ValueError("weights must be 'confidence' or None, got %r" % (weights,))
    if isinstance(conf_percentile, bool) or not isinstance(conf_percentile, (int, float)) or not 0.0 <= conf_percentile <= 100.0:
        raise ValueError("conf_percentile must be a number in [0, 100], got %r" % (conf_percentile,))
    try:
        plan = [(int(a), int(b)) for a, b in plan]
    except (TypeError, ValueError):
        raise ValueError("plan must be a list of (start, end) pairs, as chunk_plan returns it") from None
    if not plan or plan[0][0] != 0 or any(b <= a for a, b in plan):
        raise ValueError("plan must start at view 0 and every chunk must hold a view: %r" % (plan,))
    for (a0, b0), (a1, b1) in zip(plan, plan[1:]):
        if not (a0 < a1 < b0 < b1):
            raise ValueError("consecutive chunks must overlap and each must add a view: %r then %r" % ((a0, b0), (a1, b1)))
    if not isinstance(chunks, (list, tuple)) or len(chunks) != len(plan) or not all(isinstance(c, dict) for c in chunks):
        raise ValueError("chunks must be a list of %d prediction dicts, one per chunk of the plan" % len(plan))
    pointmap = "Pointmap" in prediction_mode
    need = ("world_points", "world_points_conf") if pointmap else ("depth", "depth_conf")
    keys = [k for k, _ in _STITCH_MAPS if k in chunks[0]]
    hw, on_device = None, True
    for c, (a, b) in zip(chunks, plan):
        for k in need + ("pose_enc", "images"):
            if k not in c:
                raise ValueError("prediction_mode %r needs `%s` in every chunk" % (prediction_mode, k))
        if [k for k, _ in _STITCH_MAPS if k in c] != keys:
            raise ValueError("every chunk must carry the same maps")
        img = c["images"]
        if not isinstance(img, torch.Tensor) or img.dim() != 5 or img.shape[0] != 1 or img.shape[1] != b - a:
            raise ValueError("chunk [%d, %d): images must be (1, %d, 3, H, W)" % (a, b, b - a))
        hw = hw or tuple(img.shape[-2:])
        lead = (1, b - a) + hw
        for k, dim in _STITCH_MAPS:
            if k in c:
                t = c[k]
                if not isinstance(t, torch.Tensor) or t.dtype != torch.float32 or t.dim() != dim or tuple(t.shape[:4]) != lead:
                    raise ValueError("chunk [%d, %d): %s must be a float32 tensor %r + its channels" % (a, b, k, lead))
        pe = [c["pose_enc"]] + list(c.get("pose_enc_list", []))
        if any(not isinstance(t, torch.Tensor) or tuple(t.shape) != (1, b - a, 9) for t in pe):
            raise ValueError("chunk [%d, %d): pose_enc (and every pose_enc_list entry) must be (1, %d, 9)" % (a, b, b - a))
        if len(c.get("pose_enc_list", [])) != len(chunks[0].get("pose_enc_list", [])):
            raise ValueError("every chunk must carry the same number of pose_enc_list entries")
        on_device = on_device and all(t.is_cuda for t in [c[k] for k in keys] + pe + [img])
    return plan, plan[-1][1], hw, keys, pointmap, on_device


def stitch_predictions(chunks, plan, prediction_mode="Predicted Pointmap", conf_percentile=50.0, weights="confidence", select="first",
                       with_scale=True, iterations=6, rel_delta=0.5):
    """The prediction dicts of overlapping chunks of one sequence (OmniVGGT.forward with B = 1, in the order of `plan`, which is
    chunk_plan's [(start, end)]) brought into the FIRST chunk's frame and merged into one dict for all S views, on the device.
    For chunk c > 0 a robust similarity (fit_similarity_robust: with_scale, iterations, rel_delta) is fitted over the views it shares
    with its predecessor: its own points there -- world_points / world_points_conf in the "Pointmap" modes, else its depth
    un-projected with its own decoded cameras, with depth_conf -- onto the merged points of the same views as they stand before the
    chunk is written. A pixel pair is used when each side's confidence reaches that side's `conf_percentile` (percentile over those
    views); its weight is the smaller of the two confidences (weights="confidence") or 1 (weights=None). The chunk's maps
    (points moved, depth times the fitted scale, confidences copied: ovg_align_move_maps) and cameras (ovg_align_move_cameras: the
    cameras that see the moved points at the scaled depth) are then written straight into the merged buffers for the views it owns:
    select="first" keeps the earlier chunk's overlap views, select="last" overwrites them, maps and cameras together.

    -> dict: world_points, world_points_conf, depth, depth_conf (those the chunks carry) and images for all S views; extrinsic
    (1, S, 3, 4) and intrinsic (1, S, 3, 3); pose_enc and pose_enc_list (every refinement entry moved and re-encoded; chunk 0's
    bytes are copied); chunks (the plan); chunk_transforms (one RobustFit per chunk, the identity for chunk 0). No device -> host
    synchronisation. CPU tensors raise OvgError, bad arguments ValueError."""
    plan, S, (H, W), keys, pointmap, on_device = _stitch_check(chunks, plan, prediction_mode, conf_percentile, weights, select)
    if isinstance(iterations, bool) or not isinstance(iterations, int) or iterations < 0:
        raise ValueError("iterations must be a non-negative integer, got %r" % (iterations,))
    _robust_number("rel_delta", rel_delta)
    if not on_device:
        raise ops.L.OvgError("stitch_predictions needs HIP device tensors: there is no CPU fallback")
    dev, px = chunks[0]["images"].device, H * W
    out = {k: torch.empty((1, S) + tuple(chunks[0][k].shape[2:]), device=dev, dtype=torch.float32) for k in keys}
    out["images"] = torch.empty((1, S) + tuple(chunks[0]["images"].shape[2:]), device=dev, dtype=chunks[0]["images"].dtype)
    out["extrinsic"] = torch.empty(1, S, 3, 4, device=dev, dtype=torch.float32)
    out["intrinsic"] = torch.empty(1, S, 3, 3, device=dev, dtype=torch.float32)
    n_list = len(chunks[0].get("pose_enc_list", []))
    enc_list = [torch.empty(1, S, 9, device=dev, dtype=torch.float32) for _ in range(n_list)]
    enc_last = torch.empty(1, S, 9, device=dev, dtype=torch.float32)
    fits = []
    pk, ck = ("world_points", "world_points_conf") if pointmap else ("depth", "depth_conf")
    for c, (chunk, (a, b)) in enumerate(zip(chunks, plan)):
        ext, intr = camera_math.pose_decoding(chunk["pose_enc"].float(), (H, W))
        ext, intr = ext.float().contiguous(), intr.float().contiguous()
        if c == 0:
            for k in keys:
                out[k][:, a:b] = chunk[k]
            out["images"][:, a:b], out["extrinsic"][:, a:b], out["intrinsic"][:, a:b] = chunk["images"], ext, intr
            enc_last[:, a:b] = chunk["pose_enc"]
            for dst, e in zip(enc_list, chunk.get("pose_enc_list", [])):
                dst[:, a:b] = e
            fits.append(RobustFit.identity(dev, iterations))
            continue
        ov = plan[c - 1][1] - a
        cs, ct = chunk[ck][0, :ov].contiguous(), out[ck][0, a:a + ov].contiguous()
        if pointmap:
            src, tgt = chunk[pk][0, :ov], out[pk][0, a:a + ov]
        else:
            src = unproject_depth_map_to_point_map(chunk[pk][0, :ov], ext[0, :ov], intr[0, :ov], check_skew=False)
            tgt = unproject_depth_map_to_point_map(out[pk][0, a:a + ov], out["extrinsic"][0, a:a + ov], out["intrinsic"][0, a:a + ov],
                                                   check_skew=False)
        fit = fit_similarity_robust(src.reshape(-1, 3), tgt.reshape(-1, 3), weights=torch.minimum(cs, ct).reshape(-1) if weights else None,
                                    source_valid=(cs >= percentile(cs, conf_percentile)).reshape(-1),
                                    target_valid=(ct >= percentile(ct, conf_percentile)).reshape(-1), with_scale=with_scale,
                                    iterations=iterations, rel_delta=rel_delta)
        fits.append(fit)
        M, s = fit.transform.matrix, fit.transform.scale.reshape(1)
        lo = ov if select == "first" else 0                                  # the chunk's first owned view, local; global: a + lo
        g = a + lo
        own = {k: chunk[k][0, lo:].contiguous() for k in keys}
        dst = {k: out[k][0, g:b] for k in keys}
        ops.align_move_maps((b - g) * px, transform=M, scale=s, points=own.get("world_points"), depth=own.get("depth"),
                            points_conf=own.get("world_points_conf"), depth_conf=own.get("depth_conf"), out_points=dst.get("world_points"),
                            out_depth=dst.get("depth"), out_points_conf=dst.get("world_points_conf"), out_depth_conf=dst.get("depth_conf"))
        ops.align_move_cameras(ext[0, lo:].contiguous(), M, s, out=out["extrinsic"][0, g:b])
        out["intrinsic"][:, g:b], out["images"][:, g:b] = intr[:, lo:], chunk["images"][:, lo:]
        enc_last[:, g:b] = camera_math.pose_encoding(out["extrinsic"][:, g:b], intr[:, lo:], (H, W))
        for dst_e, e in zip(enc_list, chunk.get("pose_enc_list", [])):
            e_ext, e_intr = camera_math.pose_decoding(e.float(), (H, W))
            moved = ops.align_move_cameras(e_ext[0, lo:].float().contiguous(), M, s)
            dst_e[:, g:b] = camera_math.pose_encoding(moved.unsqueeze(0), e_intr[:, lo:], (H, W))
    out["pose_enc"] = enc_last
    if n_list:
        out["pose_enc_list"] = enc_list
    out["chunks"], out["chunk_transforms"] = plan, fits
    return out


# ---------------------------------------------------------------------------------------------------------------------------------
# Depth and pose evaluation: aligned depth metrics (ovg_deptheval_*), relative pose accuracy and AUC
# ---------------------------------------------------------------------------------------------------------------------------------

DEPTH_ALIGNMENTS = {"none": ops.L.DEPTHEVAL_NONE, "median": ops.L.DEPTHEVAL_MEDIAN, "scale": ops.L.DEPTHEVAL_SCALE,
                    "scale_shift": ops.L.DEPTHEVAL_SCALE_SHIFT}
DEPTH_FEW, DEPTH_NOT_FINITE, DEPTH_NO_SPREAD, DEPTH_BAD_FIT = (ops.L.DEPTHEVAL_FEW, ops.L.DEPTHEVAL_NOT_FINITE, ops.L.DEPTHEVAL_NO_SPREAD,
                                                               ops.L.DEPTHEVAL_BAD_FIT)
DEPTH_FIGURES = ("abs_rel", "sq_rel", "rmse", "mae", "rmse_log", "delta1", "delta2", "delta3")


class DepthMetrics:
    """Result of depth_metrics. Per group (one per view with scope="view", one in all with scope="sequence") float64 device tensors
    [G]: abs_rel (mean |q - g| / g), sq_rel (mean (q - g)^2 / g), rmse, mae, rmse_log (root mean square of log q - log g), delta1 /
    delta2 / delta3 (share of pixels with max(q / g, g / q) < 1.25, 1.25^2, 1.25^3), q the aligned and clipped prediction; n int64 [G]
    (used pixels), scale / shift float64 [G] (the alignment q = scale pred + shift), status int32 [G] (DEPTH_* bits, 0 for a regular
    fit; a degenerate group is scored unaligned). A group with n = 0 reports nan. Python floats: `mean` (dict by figure: the mean over
    the groups with n > 0, the per-image protocol), `pooled` (dict: all used pixels as one set), `n_total` (int)."""
    __slots__ = DEPTH_FIGURES + ("n", "scale", "shift", "status", "mean", "pooled", "n_total", "align", "scope")

    def __init__(self, **kw):
        for k in self.__slots__:
            setattr(self, k, kw.get(k))

    def __repr__(self):
        return "DepthMetrics(align=%r, scope=%r, n_total=%r, mean=%r, pooled=%r)" % (self.align, self.scope, self.n_total, self.mean, self.pooled)


def _depth_number(what, name, v, lo=None, lo_open=False):
    if isinstance(v, bool) or not isinstance(v, (int, float)) or v != v:
        raise ValueError("%s: %s must be a number, not NaN, got %r" % (what, name, v))
    if lo is not None and (v <= lo if lo_open else v < lo):
        raise ValueError("%s: %s must be %s %r, got %r" % (what, name, ">" if lo_open else ">=", lo, v))
    return float(v)


def _depth_args(what, pred, gt, valid, align, scope, min_depth, max_depth):
    """-> (pred [G, n], gt [G, n], valid u8 [G, n] or None, solve mode): the checked arguments as the entries take them."""
    if align not in DEPTH_ALIGNMENTS:
        raise ValueError("%s: align must be one of %s, got %r" % (what, " | ".join(DEPTH_ALIGNMENTS), align))
    if scope not in ("view", "sequence"):
        raise ValueError("%s: scope must be view | sequence, got %r" % (what, scope))
    maps = []
    for t, name in ((pred, "pred"), (gt, "gt")):
        if not isinstance(t, torch.Tensor) or t.dtype != torch.float32 or t.dim() not in (3, 4) or (t.dim() == 4 and t.shape[-1] != 1):
            raise ValueError("%s: %s must be a float32 tensor (S, H, W) or (S, H, W, 1)" % (what, name))
        maps.append(t.reshape(t.shape[:3]))
    S, H, W = maps[0].shape
    if maps[1].shape != maps[0].shape or S < 1 or H * W < 1:
        raise ValueError("%s: pred and gt must hold the same S >= 1 maps of H x W >= 1 pixels, got %r and %r" % (what, tuple(pred.shape), tuple(gt.shape)))
    if S * H * W >= 1 << 31 or (scope == "view" and S > ops.L.DEPTHEVAL_MAX_GROUPS):
        raise ValueError("%s: fewer than 2^31 pixels and at most %d views per call" % (what, ops.L.DEPTHEVAL_MAX_GROUPS))
    if valid is not None:
        if not isinstance(valid, torch.Tensor) or valid.dtype not in (torch.bool, torch.uint8) or valid.dim() not in (3, 4) or \
                tuple(valid.shape[:3]) != (S, H, W) or (valid.dim() == 4 and valid.shape[-1] != 1):
            raise ValueError("%s: valid must be a bool / uint8 tensor shaped like the maps" % what)
    _depth_number(what, "min_depth", min_depth, 0.0)
    _depth_number(what, "max_depth", max_depth)
    if not all(t is None or t.is_cuda for t in (pred, gt, valid)):
        raise ops.L.OvgError("%s needs HIP device tensors: there is no CPU fallback" % what)
    shape = (S, H * W) if scope == "view" else (1, S * H * W)
    p, g = (m.contiguous().reshape(shape) for m in maps)
    v = None if valid is None else valid.reshape(S, H, W).contiguous().view(torch.uint8).reshape(shape)
    return p, g, v, DEPTH_ALIGNMENTS[align]


def _depth_coeff(p, g, v, mode, min_depth, max_depth):
    """The alignment of every group -> (coeff f64 [G, 2], status int32 [G]); one pass over the maps, four for the median."""
    L = ops.L
    if mode == L.DEPTHEVAL_MEDIAN:
        count, med = ops.deptheval_median(p, g, v, min_depth, max_depth)
        return ops.deptheval_solve(mode, count, median=med)
    counts, sums = ops.deptheval_sums(p, g, v, min_depth, max_depth)
    return ops.deptheval_solve(mode, counts, sums=sums)


def align_depth(pred, gt, valid=None, align="median", scope="view", min_depth=0.0, max_depth=float("inf")):
    """The alignment a depth benchmark makes before it scores: gt ~ scale pred + shift over the USED pixels of a group -- valid (or
    all), pred and gt finite, pred > 0, min_depth < gt <= max_depth. align: "none" (1, 0), "median" (ratio of the medians, the
    protocol of scale-ambiguous predictions), "scale" (least squares through the origin), "scale_shift" (least squares, the protocol
    of affine-invariant depth). scope: "view" fits every map on its own, "sequence" all S maps with one pair of coefficients.
    pred, gt: float32 device tensors (S, H, W) or (S, H, W, 1); valid: bool / uint8 like them. The medians are exact order statistics
    (a radix select per group: no sort, no compaction), the sums float64 in a fixed order: two calls give identical bytes.
    -> (scale, shift, status): float64 / float64 / int32 device tensors [S] or [1]; a degenerate group (no used pixel, no spread, a
    fit that is not positive and finite) gets (1, 0) and its DEPTH_* status bits. `scale` is what get_world_points_from_depth(gt_scale=)
    and fuse_predictions take. Nothing is read back."""
    p, g, v, mode = _depth_args("align_depth", pred, gt, valid, align, scope, min_depth, max_depth)
    coeff, status = _depth_coeff(p, g, v, mode, min_depth, max_depth)
    return coeff[:, 0], coeff[:, 1], status


def depth_metrics(pred, gt, valid=None, align="median", scope="view", min_depth=0.0, max_depth=float("inf"), clip_min=1e-3, clip_max=None):
    """AbsRel, SqRel, RMSE, MAE, RMSE-log and delta < 1.25 / 1.25^2 / 1.25^3 of predicted depth against ground truth after the
    alignment of align_depth (same arguments), on the device: q = scale pred + shift, clipped to [clip_min, clip_max] (clip_min > 0
    keeps the logarithm defined where a shift drives q below zero; clip_max None: no upper clip), scored against gt over the used
    pixels. The term sums are float64 in the fixed order of include/omnivggt_hip.h, the ratios and roots float64 torch operations on
    them. -> DepthMetrics (one device -> host read at the end, for its summary floats)."""
    what = "depth_metrics"
    cmin = _depth_number(what, "clip_min", clip_min, 0.0, lo_open=True)
    cmax = float("inf") if clip_max is None else _depth_number(what, "clip_max", clip_max)
    if cmin == float("inf") or cmax < cmin:
        raise ValueError("%s: clip_min must be finite and clip_max >= clip_min, got %r, %r" % (what, clip_min, clip_max))
    p, g, v, mode = _depth_args(what, pred, gt, valid, align, scope, min_depth, max_depth)
    coeff, status = _depth_coeff(p, g, v, mode, min_depth, max_depth)
    counts, sums = ops.deptheval_sums(p, g, v, min_depth, max_depth, coeff=coeff, clip_min=cmin, clip_max=cmax)
    n = counts[:, 0]
    nd = n.double()
    mean = sums / nd[:, None]                                                 # 0 / 0 = nan for a group without a used pixel
    per = torch.stack([mean[:, 0], mean[:, 1], mean[:, 2].sqrt(), mean[:, 3], mean[:, 4].sqrt(),
                       counts[:, 1].double() / nd, counts[:, 2].double() / nd, counts[:, 3].double() / nd])            # [8, G]
    has = n > 0
    over_groups = torch.where(has, per, torch.zeros_like(per)).sum(1) / has.sum().double()
    tn = nd.sum()
    tm = sums.sum(0) / tn
    pooled = torch.stack([tm[0], tm[1], tm[2].sqrt(), tm[3], tm[4].sqrt(), counts[:, 1].sum().double() / tn, counts[:, 2].sum().double() / tn,
                          counts[:, 3].sum().double() / tn])
    host = torch.cat([over_groups, pooled, tn[None]]).tolist()               # the one device -> host read
    out = {k: per[i] for i, k in enumerate(DEPTH_FIGURES)}
    out.update(n=n, scale=coeff[:, 0], shift=coeff[:, 1], status=status, align=align, scope=scope, n_total=int(host[16]),
               mean=dict(zip(DEPTH_FIGURES, host[0:8])), pooled=dict(zip(DEPTH_FIGURES, host[8:16])))
    return DepthMetrics(**out)


def _pose_matrices(what, pred_extrinsic, gt_extrinsic, min_cameras):
    es = []
    for e, name in ((pred_extrinsic, "pred_extrinsic"), (gt_extrinsic, "gt_extrinsic")):
        if not isinstance(e, torch.Tensor) or e.dim() != 3 or tuple(e.shape[1:]) not in ((3, 4), (4, 4)) or e.dtype not in (torch.float32, torch.float64):
            raise ValueError("%s must be a float32 / float64 tensor (S, 3, 4) or (S, 4, 4)" % name)
        es.append(e)
    if es[0].shape[0] != es[1].shape[0] or es[0].shape[0] < min_cameras:
        raise ValueError("%s pairs camera i with camera i and needs at least %d: %d predicted, %d ground-truth cameras"
                         % (what, min_cameras, es[0].shape[0], es[1].shape[0]))
    if not (es[0].is_cuda and es[1].is_cuda):
        raise ops.L.OvgError("%s needs HIP device tensors: there is no CPU fallback" % what)
    return es


def _relative_poses(e):
    """World-to-camera [A | t] (S, 3+, 4) -> (A_j A_i^-1, t_j - A_j A_i^-1 t_i) for all pairs i < j (i major), float64. The 3 x 3 inverse
    is the adjugate over the determinant (cross products of the columns' partners): elementwise, no solver."""
    A, t = e[:, :3, :3].double(), e[:, :3, 3].double()
    S = A.shape[0]
    i, j = torch.triu_indices(S, S, 1, device=e.device)
    r0, r1, r2 = A[:, 0], A[:, 1], A[:, 2]
    c0, c1, c2 = torch.linalg.cross(r1, r2), torch.linalg.cross(r2, r0), torch.linalg.cross(r0, r1)
    det = (r0 * c0).sum(1)
    inv = torch.stack([c0, c1, c2], 2) / det[:, None, None]
    rel = A[j] @ inv[i]
    return rel, t[j] - (rel @ t[i][:, :, None]).squeeze(-1)


def relative_pose_errors(pred_extrinsic, gt_extrinsic):
    """Relative pose errors over all pairs i < j of S >= 2 cameras, the figures RRA / RTA / AUC are made of: rel_ij = E_j E_i^-1 of the
    world-to-camera matrices in float64 on the device -- unchanged by any similarity of the world frame, so no alignment is needed.
    Rotation error: the angle of dR = R_pred R_gt^T as atan2(|vee(dR - dR^T)| / 2, (tr dR - 1) / 2) (accurate at 0 and at 180 degrees
    alike); translation error: the angle between the two relative translations as atan2(|a x b|, a . b), folded to min(theta, 180 -
    theta) (the sign of a direction is not observable), 0 when either is shorter than 1e-12.
    pred_extrinsic, gt_extrinsic: float32 / float64 device tensors (S, 3, 4) or (S, 4, 4). -> (rot_err, trans_err) in degrees,
    float64 device tensors [S (S - 1) / 2], pair (i, j) at i-major position. Nothing is read back."""
    ep, eg = _pose_matrices("relative_pose_errors", pred_extrinsic, gt_extrinsic, 2)
    (rp, a), (rg, b) = _relative_poses(ep), _relative_poses(eg)
    dR = rp @ rg.transpose(1, 2)
    w = torch.stack([dR[:, 2, 1] - dR[:, 1, 2], dR[:, 0, 2] - dR[:, 2, 0], dR[:, 1, 0] - dR[:, 0, 1]], 1)
    rot = torch.rad2deg(torch.atan2(0.5 * torch.linalg.vector_norm(w, dim=1), (dR[:, 0, 0] + dR[:, 1, 1] + dR[:, 2, 2] - 1.0) / 2.0))
    theta = torch.rad2deg(torch.atan2(torch.linalg.vector_norm(torch.linalg.cross(a, b), dim=1), (a * b).sum(1)))
    trans = torch.minimum(theta, 180.0 - theta)
    short = (torch.linalg.vector_norm(a, dim=1) < 1e-12) | (torch.linalg.vector_norm(b, dim=1) < 1e-12)
    return rot, torch.where(short, torch.zeros_like(trans), trans)


def pose_auc(rot_err, trans_err, thresholds=(5, 15, 30)):
    """Relative pose accuracy from the errors of relative_pose_errors (degrees, device tensors of one length >= 1), for every integer
    threshold t >= 1: "RRA@t" / "RTA@t" the share of pairs with rotation / translation error below t, "Acc@t" with both below it,
    "AUC@t" the mean over the integer degrees d = 1 .. t of the share of pairs whose larger error lies below d. Counted in integers
    on the device. -> dict of Python floats (one device -> host read)."""
    for e, name in ((rot_err, "rot_err"), (trans_err, "trans_err")):
        if not isinstance(e, torch.Tensor) or e.dim() != 1 or not e.dtype.is_floating_point or e.numel() < 1:
            raise ValueError("pose_auc: %s must be a 1-D floating-point tensor with at least one pair" % name)
    if rot_err.shape != trans_err.shape:
        raise ValueError("pose_auc: %d rotation and %d translation errors" % (rot_err.numel(), trans_err.numel()))
    ts = list(thresholds) if isinstance(thresholds, (tuple, list)) else None
    if not ts or any(isinstance(t, bool) or not isinstance(t, int) or t < 1 or t > 180 for t in ts):
        raise ValueError("pose_auc: thresholds must be a sequence of integer degrees in [1, 180], got %r" % (thresholds,))
    if not (rot_err.is_cuda and trans_err.is_cuda):
        raise ops.L.OvgError("pose_auc needs HIP device tensors: there is no CPU fallback")
    r, t = rot_err.double(), trans_err.double()
    worst = torch.maximum(r, t)
    thr = torch.tensor(ts, device=r.device, dtype=torch.float64)
    degrees = torch.arange(1, max(ts) + 1, device=r.device, dtype=torch.float64)
    below = torch.cumsum((worst[:, None] < degrees[None, :]).sum(0), 0)       # [max t]: pairs-below-d summed over d = 1 .. t
    counts = torch.cat([(r[:, None] < thr).sum(0), (t[:, None] < thr).sum(0), ((r[:, None] < thr) & (t[:, None] < thr)).sum(0),
                        below[torch.tensor([x - 1 for x in ts], device=r.device)]]).tolist()
    P, k, out = r.numel(), len(ts), {}
    for i, x in enumerate(ts):
        out["RRA@%d" % x], out["RTA@%d" % x], out["Acc@%d" % x] = counts[i] / P, counts[k + i] / P, counts[2 * k + i] / P
        out["AUC@%d" % x] = counts[3 * k + i] / (P * x)
    return out


def evaluate_predictions(predictions, gt_depth=None, gt_valid=None, gt_extrinsic=None, batch_index=0, **kw):
    """Scores batch element `batch_index` of the dict OmniVGGT.forward returns against whatever ground truth is given: with gt_depth
    (S, H, W[, 1]) (and gt_valid) depth_metrics of predictions["depth"] (keywords: align, scope, min_depth, max_depth, clip_min,
    clip_max); with gt_extrinsic (S, 3 | 4, 4) relative_pose_errors and pose_auc (keyword: thresholds) of the cameras decoded from
    predictions["pose_enc"] (or predictions["extrinsic"] when present). -> a plain dict: "depth" (DepthMetrics), "rot_err",
    "trans_err" (device tensors), "pose" (the pose_auc dict) -- each only when its ground truth was given."""
    if not isinstance(predictions, dict):
        raise ValueError("evaluate_predictions: predictions must be the dict OmniVGGT.forward returns")
    if gt_depth is None and gt_extrinsic is None:
        raise ValueError("evaluate_predictions: give gt_depth, gt_extrinsic or both")
    thresholds = kw.pop("thresholds", (5, 15, 30))
    unknown = set(kw) - {"align", "scope", "min_depth", "max_depth", "clip_min", "clip_max"}
    if unknown:
        raise ValueError("evaluate_predictions: unknown keywords %s" % sorted(unknown))
    b, out = batch_index, {}
    if gt_depth is not None:
        if "depth" not in predictions:
            raise ValueError("evaluate_predictions: predictions carry no `depth`")
        out["depth"] = depth_metrics(predictions["depth"][b], gt_depth, gt_valid, **kw)
    if gt_extrinsic is not None:
        if "extrinsic" in predictions:
            ext = predictions["extrinsic"][b]
        elif "pose_enc" in predictions:
            ext = pose_encoding_to_extri_intri(predictions["pose_enc"][b:b + 1], build_intrinsics=False)[0][0]
        else:
            raise ValueError("evaluate_predictions: predictions carry neither `extrinsic` nor `pose_enc`: the cameras are needed")
        out["rot_err"], out["trans_err"] = relative_pose_errors(ext if ext.dtype in (torch.float32, torch.float64) else ext.float(), gt_extrinsic)
        out["pose"] = pose_auc(out["rot_err"], out["trans_err"], thresholds)
    return out


# ---------------------------------------------------------------------------------------------------------------------------------
# Plane segmentation: RANSAC over seeded hypotheses, least-squares refit, floor alignment (ovg_plane_*)
# ---------------------------------------------------------------------------------------------------------------------------------

PLANE_NONE, PLANE_FEW, PLANE_NO_SPREAD, PLANE_NOT_FINITE = ops.L.PLANE_NONE, ops.L.PLANE_FEW, ops.L.PLANE_NO_SPREAD, ops.L.PLANE_NOT_FINITE
PLANE_MAX_HYPOTHESES = 1 << 24


class PlaneResult:
    """Result of segment_plane, all on the device: plane float32 (4,) = (nx, ny, nz, w) with |n| = 1 and n.p + w = 0 on the plane (zeros
    when there is none); inlier bool, shaped like the points without their last dimension; count (0-d int64: the inliers), hypothesis
    (0-d int32: the winning hypothesis, -1 for none), rms (0-d float64: the root mean square distance of the last refit's inliers to
    its plane, 0 without a refit) and status (0-d int32: 0, or PLANE_NONE when no hypothesis reached min_inliers, with PLANE_FEW |
    PLANE_NO_SPREAD | PLANE_NOT_FINITE from a refit round that kept the previous plane). distance: the signed residual float32 shaped
    like `inlier` (NaN at unusable points), None unless asked for."""
    __slots__ = ("plane", "inlier", "count", "hypothesis", "rms", "status", "distance")

    def __init__(self, plane, inlier, count, hypothesis, rms, status, distance=None):
        self.plane, self.inlier, self.count, self.hypothesis, self.rms, self.status, self.distance = plane, inlier, count, hypothesis, rms, status, distance


def _plane_int(value, name, lo, hi):
    if isinstance(value, bool) or not isinstance(value, int) or not lo <= value < hi:
        raise ValueError("%s must be an integer in [%d, %d), got %r" % (name, lo, hi, value))
    return value


def _plane_args(what, cloud_or_points, threshold, rel_threshold, hypotheses, seed, refit, min_inliers, valid, axis, max_angle_deg, candidates):
    """The argument checks segment_plane and segment_planes share, ValueErrors first, then the device check.
    -> (pts, lead, valid, threshold float32 as a host float, axis float32 [3] device tensor or None, min_abs_cos, candidates)"""
    import math
    if (threshold is None) == (rel_threshold is None):
        raise ValueError("%s: give exactly one of threshold and rel_threshold" % what)
    pts = _nn_points(cloud_or_points, "cloud_or_points")
    lead = tuple(pts.shape[:-1])
    valid = _nn_valid(valid, lead, "valid")
    if threshold is not None:
        if isinstance(threshold, bool) or not isinstance(threshold, (int, float)) or not (threshold >= 0 and math.isfinite(threshold)):
            raise ValueError("threshold must be a finite number >= 0, got %r" % (threshold,))
        try:
            threshold = _f32(float(threshold))
        except OverflowError:
            threshold = float("inf")
        if not math.isfinite(threshold):
            raise ValueError("threshold %r is not finite in float32" % (threshold,))
    _plane_int(hypotheses, "hypotheses", 1, PLANE_MAX_HYPOTHESES + 1)
    _plane_int(seed, "seed", 0, 1 << 64)
    _plane_int(refit, "refit", 0, 65)
    _plane_int(min_inliers, "min_inliers", 3, 1 << 31)
    if max_angle_deg is not None:
        if axis is None:
            raise ValueError("max_angle_deg needs an axis")
        if isinstance(max_angle_deg, bool) or not isinstance(max_angle_deg, (int, float)) or not 0 < max_angle_deg <= 90:
            raise ValueError("max_angle_deg must be a number in (0, 90], got %r" % (max_angle_deg,))
    min_abs_cos = 0.0 if max_angle_deg is None else max(0.0, min(1.0, _f32(math.cos(math.radians(float(max_angle_deg))))))
    host_axis = None
    if isinstance(axis, torch.Tensor):
        if axis.numel() != 3 or axis.dtype not in (torch.float32, torch.float64):
            raise ValueError("axis must hold three float32 / float64 values")
    elif axis is not None:
        try:
            host_axis = [float(v) for v in axis]
        except (TypeError, ValueError):
            raise ValueError("axis must be three finite numbers or a tensor of three, got %r" % (axis,)) from None
        if len(host_axis) != 3 or not all(math.isfinite(v) for v in host_axis):
            raise ValueError("axis must be three finite numbers, got %r" % (axis,))
        x, y, z = host_axis
        length = math.sqrt((x * x + y * y) + z * z)
        if not (length > 0 and math.isfinite(length)):
            raise ValueError("axis must have a finite non-zero length, got %r" % (axis,))
        host_axis = [x / length, y / length, z / length]
    if candidates is not None and (not isinstance(candidates, torch.Tensor) or candidates.dim() != 1 or
                                   candidates.dtype not in (torch.int32, torch.int64) or candidates.numel() >= 1 << 31):
        raise ValueError("candidates must be a one-dimensional int32 / int64 tensor of point indices")
    if rel_threshold is not None:
        threshold = _cloud_radius(what, cloud_or_points, pts, None, rel_threshold)       # reads scene_scale back: the one synchronisation
    tensors = (pts, valid, candidates, axis if isinstance(axis, torch.Tensor) else None)
    if not all(t is None or t.is_cuda for t in tensors):
        raise ops.L.OvgError("%s needs HIP device tensors: there is no CPU fallback" % what)
    if host_axis is not None:
        axis = torch.tensor(host_axis, dtype=torch.float64).to(torch.float32).to(pts.device)
    elif axis is not None:
        a = axis.reshape(3).to(torch.float64)
        axis = (a / ((a[0] * a[0] + a[1] * a[1]) + a[2] * a[2]).sqrt()).to(torch.float32).contiguous()
    if candidates is not None:
        candidates = candidates.to(torch.int32).contiguous()
    return pts, lead, valid, threshold, axis, min_abs_cos, candidates


def _segment_plane(pts, valid, threshold, hypotheses, seed, refit, min_inliers, axis, min_abs_cos, candidates, want_distance):
    """segment_plane for contiguous [n, 3] points, u8 [n] valid, int32 candidates (None or non-empty): launches only."""
    dev = pts.device
    planes, _ = ops.plane_hypotheses(pts, hypotheses, seed, valid=valid, candidates=candidates, axis=axis, min_abs_cos=min_abs_cos)
    count = ops.plane_score(pts, planes, threshold, valid=valid)
    best, plane, _, status = ops.plane_select(count, planes, min_inliers)
    want = True if want_distance else None
    inlier, distance, total = ops.plane_mask(pts, plane, threshold, valid=valid, gate=status, distance=want)
    rms = torch.zeros(1, device=dev, dtype=torch.float64)
    if refit:
        ws = torch.empty(ops.align_workspace_bytes(pts.shape[0]), device=dev, dtype=torch.uint8)
        step = torch.empty(1, device=dev, dtype=torch.int32)
    for _ in range(refit):
        n0, s0 = ops.align_moments(pts, pts, source_valid=inlier, ws=ws)
        centre = s0[:6] / n0.clamp_min(1).to(torch.float64)
        n1, s1 = ops.align_moments(pts, pts, source_valid=inlier, centre=centre, ws=ws)
        ops.plane_fit(n1, s1, plane, centre=centre, axis=axis, rms=rms, status=step)
        status = status | step
        inlier, distance, total = ops.plane_mask(pts, plane, threshold, valid=valid, gate=status, inlier=inlier, distance=distance, out_count=total)
    return PlaneResult(plane, inlier, total[0], best[0], rms[0], status[0], distance)


def _empty_plane(lead, dev, want_distance):
    return PlaneResult(torch.zeros(4, device=dev, dtype=torch.float32), torch.zeros(lead, device=dev, dtype=torch.bool),
                       torch.zeros((), device=dev, dtype=torch.int64), torch.full((), -1, device=dev, dtype=torch.int32),
                       torch.zeros((), device=dev, dtype=torch.float64), torch.full((), PLANE_NONE, device=dev, dtype=torch.int32),
                       torch.full(lead, float("nan"), device=dev, dtype=torch.float32) if want_distance else None)


def segment_plane(cloud_or_points, threshold=None, rel_threshold=None, hypotheses=1024, seed=0, refit=2, min_inliers=3, valid=None,
                  axis=None, max_angle_deg=None, candidates=None, return_distance=False):
    """The dominant plane of a cloud -- the floor, a wall, a table top -- by RANSAC on the device (ovg_plane_hypotheses, _score,
    _select, _mask, _fit; what Open3D's segment_plane and PCL's SACSegmentation do on the host). The result is defined without a
    schedule (include/omnivggt_hip.h; tests/plane_twin.py restates it by brute force), so two calls give identical bytes:

      a plane is (nx, ny, nz, w) in float32 with |n| = 1; a point is an INLIER when it is usable (valid and finite) and
      |((nx x + ny y) + nz z) + w| <= threshold in float32 without fused multiply-adds (inclusive);
      hypothesis h < `hypotheses` is the plane through three points drawn by a splitmix64 hash of (seed, h) from `candidates` (int32 /
      int64 point indices; default: every point), void when a draw repeats, is unusable or out of range, when the three are
      near-collinear, or, with `axis` and max_angle_deg, when its normal is more than max_angle_deg away from +-axis;
      the WINNER has the most inliers over all usable points, ties to the lowest h; none reaching min_inliers (>= 3) gives no plane;
      `refit` rounds then replace the plane by the least-squares plane through its inliers (the float64 moments of ovg_align_moments,
      the Jacobi solve of estimate_normals) and recompute the inliers; a degenerate round keeps the plane and sets a status bit.

    Exactly one of threshold (in the cloud's units) and rel_threshold (a PointCloud only: f32(rel_threshold) * scene_scale, as
    radius_outlier_mask's rel_radius, read back from the device: the only synchronisation) must be given. axis: three numbers or a
    tensor of three, normalised here; the normal then points to the axis' side (n.axis >= 0) -- pass the scene's up direction to get
    a floor normal that points up -- and without it the normal's largest component is positive.

    -> PlaneResult. An empty cloud returns a result with status PLANE_NONE without a launch. CPU tensors raise OvgError (there is no
    CPU fallback); bad arguments raise ValueError."""
    if not isinstance(return_distance, bool):
        raise ValueError("return_distance must be True or False, got %r" % (return_distance,))
    pts, lead, valid, threshold, axis, min_abs_cos, candidates = _plane_args(
        "segment_plane", cloud_or_points, threshold, rel_threshold, hypotheses, seed, refit, min_inliers, valid, axis, max_angle_deg, candidates)
    n = pts.numel() // 3
    if n == 0 or (candidates is not None and candidates.numel() == 0):
        return _empty_plane(lead, pts.device, return_distance)
    res = _segment_plane(pts.reshape(n, 3).contiguous(), _u8_flat(valid), threshold, hypotheses, seed, refit, min_inliers, axis, min_abs_cos,
                         candidates, return_distance)
    res.inlier = res.inlier.reshape(lead).to(torch.bool)
    if res.distance is not None:
        res.distance = res.distance.reshape(lead)
    return res


def segment_planes(cloud_or_points, max_planes=4, min_inliers=None, threshold=None, rel_threshold=None, hypotheses=1024, seed=0, refit=2,
                   valid=None, axis=None, max_angle_deg=None, candidates=None):
    """The dominant planes of a cloud one after the other (segment_plane's arguments and rule): plane k is searched among the points no
    earlier plane took -- it draws from the candidates still unlabelled (every unlabelled point without a list) with seed + k and is
    scored over the unlabelled points only -- and the extraction stops at the first plane below min_inliers (default: a twentieth of
    the cloud, at least 3) or after max_planes. Extraction is sequential: it synchronises with the device once per plane, to read
    the plane's status and the length of the next candidate list back.

    -> (planes float32 (P, 4), labels int32 shaped like the points without their last dimension): the plane's rank in extraction
    order at its inliers, -1 elsewhere; cluster_colors(labels) colours them. Errors as segment_plane."""
    n_all = _nn_points(cloud_or_points, "cloud_or_points").numel() // 3
    if min_inliers is None:
        min_inliers = max(3, n_all // 20)
    _plane_int(max_planes, "max_planes", 1, 1 << 16)
    pts, lead, valid, threshold, axis, min_abs_cos, candidates = _plane_args(
        "segment_planes", cloud_or_points, threshold, rel_threshold, hypotheses, seed, refit, min_inliers, valid, axis, max_angle_deg, candidates)
    dev, n = pts.device, n_all
    labels = torch.full((n,), -1, device=dev, dtype=torch.int32)
    planes = []
    if n:
        flat = pts.reshape(n, 3).contiguous()
        base = torch.ones(n, device=dev, dtype=torch.uint8) if valid is None else (_u8_flat(valid) != 0).to(torch.uint8)
        cand = candidates
        for k in range(max_planes):
            free = labels < 0
            if k > 0 or cand is not None:
                if candidates is None:
                    cand = torch.nonzero(free).reshape(-1).to(torch.int32)
                else:
                    inside = (cand >= 0) & (cand < n)
                    cand = cand[inside & free[cand.clamp(0, n - 1).long()]]
                if cand.numel() == 0:
                    break
            res = _segment_plane(flat, base & free.to(torch.uint8), threshold, hypotheses, (seed + k) & ((1 << 64) - 1), refit, min_inliers, axis,
                                 min_abs_cos, cand, False)
            if int(res.status) & PLANE_NONE:
                break
            labels = torch.where(res.inlier != 0, torch.full_like(labels, k), labels)
            planes.append(res.plane)
    out = torch.stack(planes) if planes else torch.zeros(0, 4, device=dev, dtype=torch.float32)
    return out, labels.reshape(lead)


def remove_plane(cloud, result, keep="outliers"):
    """A PointCloud without the inliers of a PlaneResult (keep="outliers": the scene without its floor, for cluster_points, where the
    floor would join every object into one component) or with them alone (keep="inliers"), in input order. Points that are not
    usable are no inliers and stay with the outliers. Gathered as remove_radius_outliers gathers: points, colors and conf at the kept
    points, `indices` the input cloud's there (or the positions in the input cloud when it has none), everything else passed through."""
    if not isinstance(cloud, PointCloud):
        raise ValueError("remove_plane takes a PointCloud")
    if not isinstance(result, PlaneResult):
        raise ValueError("expected the PlaneResult of segment_plane")
    if keep not in ("outliers", "inliers"):
        raise ValueError("keep must be \"outliers\" or \"inliers\", got %r" % (keep,))
    if result.inlier.numel() != len(cloud):
        raise ValueError("the PlaneResult holds %d points, the cloud %d" % (result.inlier.numel(), len(cloud)))
    inl = result.inlier.reshape(-1).to(torch.bool)
    return _gather_cloud(cloud, inl if keep == "inliers" else ~inl)


def floor_alignment(plane, up=(0.0, 1.0, 0.0)):
    """The rigid transform that puts a plane on the ground: a Similarity (scale 1, float64) whose rotation takes the plane's normal onto
    `up` by the shortest arc -- an antiparallel normal is turned by half a turn about the axis perpendicular to it that the first
    coordinate axis not parallel to it gives -- and whose translation puts the plane at height 0, so that up . (moved point) is the
    point's signed distance to the plane. plane: a PlaneResult or a tensor of four (nx, ny, nz, w); up: three numbers.
    Similarity.apply(cloud) then moves a cloud for write_glb and render_point_cloud. A few float64 torch operations on the plane's
    device; nothing is read back. A plane of zeros (no plane) gives a matrix of NaNs."""
    import math
    if isinstance(plane, PlaneResult):
        plane = plane.plane
    if not isinstance(plane, torch.Tensor) or plane.numel() != 4 or plane.dtype not in (torch.float32, torch.float64):
        raise ValueError("plane must be a PlaneResult or a float32 / float64 tensor of four values")
    try:
        u = [float(v) for v in up]
    except (TypeError, ValueError):
        raise ValueError("up must be three finite numbers, got %r" % (up,)) from None
    length = math.sqrt(sum(v * v for v in u)) if len(u) == 3 else 0.0
    if len(u) != 3 or not (length > 0 and math.isfinite(length)):
        raise ValueError("up must be three finite numbers with a non-zero length, got %r" % (up,))
    dev = plane.device
    q = plane.reshape(4).to(torch.float64)
    norm = (q[:3] * q[:3]).sum().sqrt()
    n, w = q[:3] / norm, q[3] / norm
    u = torch.tensor([v / length for v in u], dtype=torch.float64, device=dev)
    eye = torch.eye(3, dtype=torch.float64, device=dev)

    def cross_matrix(v):
        zero = torch.zeros((), dtype=torch.float64, device=dev)
        return torch.stack([torch.stack([zero, -v[2], v[1]]), torch.stack([v[2], zero, -v[0]]), torch.stack([-v[1], v[0], zero])])

    c = (n * u).sum()
    K = cross_matrix(torch.linalg.cross(n, u))
    near = K @ K / (1.0 + c).clamp_min(1e-300)
    R = eye + K + near                                                          # Rodrigues with sin = |n x u|, (1 - cos) / sin^2 = 1 / (1 + cos)
    # antiparallel: half a turn about a = e x n / |e x n|, e the first coordinate axis not parallel to n; R = 2 a a^T - I
    first = (n[0].abs() < 0.9).to(torch.float64)
    e = torch.stack([first, 1.0 - first, torch.zeros((), dtype=torch.float64, device=dev)])
    a = torch.linalg.cross(e, n)
    a = a / (a * a).sum().sqrt()
    half = 2.0 * torch.outer(a, a) - eye
    R = torch.where(1.0 + c < 1e-12, half, R)
    M = torch.eye(4, dtype=torch.float64, device=dev)
    M[:3, :3] = R
    M[:3, 3] = w * u
    return Similarity(M, torch.ones((), device=dev, dtype=torch.float64), torch.zeros((), device=dev, dtype=torch.int64),
                      torch.zeros((), device=dev, dtype=torch.float64), torch.zeros((), device=dev, dtype=torch.int32))


# ---------------------------------------------------------------------------------------------------------------------------------
# Farthest-point sampling: a fixed number of well-spread points (ovg_farthest_point_sample)
# ---------------------------------------------------------------------------------------------------------------------------------

class FPSResult:
    """Result of farthest_point_sample: index int32 (the sampled points in selection order, -1 where a cloud has no usable point),
    sqdist float32 (each sample's squared distance to the samples before it, 1e10 for the first, +inf with index -1) and distance
    (float32, every point's squared distance to its nearest sample, +inf for unusable points; None unless asked for)."""
    __slots__ = ("index", "sqdist", "distance")

    def __init__(self, index, sqdist, distance=None):
        self.index, self.sqdist, self.distance = index, sqdist, distance


def farthest_point_sample(xyz, npoint, valid=None, include_ends=False, first=0, return_distance=False):
    """npoint well-spread points of every cloud, chosen on the device one after the other (ovg_farthest_point_sample): sample 0 is point
    `first`, every further sample is the point farthest from all samples so far. The deterministic path of the reference's
    farthest_point_sample (omnivggt/utils/po_utils/misc.py, a Python loop of torch launches), index for index: the rule is exact
    (tests/fps_twin.py restates it in numpy float32): d = (dx dx + dy dy) + dz dz in float32 without fused multiply-adds, every point
    keeps the smallest d to a sample, starting from the reference's 1e10 (distances saturate there: points farther than 1e5 from every
    sample tie), the largest wins and ties go to the LOWEST index, so two calls, and both forms of the kernel, give identical bytes.
    include_ends: sample 1 is the last point (the reference's option; needs N >= 2). A point is usable when its coordinates are
    finite and its valid entry (if given) is non-zero: unusable points are never chosen (only forced: `first`, or the last point
    with include_ends, are reported as they are and change nothing). With fewer distinct usable points than npoint the lowest-index
    usable point repeats, as in the reference.

    xyz: float32 device tensor (N, 3) or (B, N, 3), or a PointCloud (its points); valid: optional bool / uint8 tensor (N,) / (B, N).
    -> FPSResult(index, sqdist, distance) shaped (npoint,) or (B, npoint) (distance: (N,) or (B, N) with return_distance, else None).
    index is int32 like NNResult's (the reference returns int64); sqdist from the first free sample on never increases: it is the
    squared coverage radius of the samples before it. npoint > N raises ValueError (the reference turns random there), so does
    include_ends with N < 2; N == 0 or npoint == 0 give empty results. No device -> host synchronisation. CPU tensors raise OvgError
    (there is no CPU fallback); bad shapes or dtypes raise ValueError."""
    x = xyz.points if isinstance(xyz, PointCloud) else xyz
    if not isinstance(x, torch.Tensor) or x.dim() not in (2, 3) or x.shape[-1] != 3 or x.dtype != torch.float32:
        raise ValueError("xyz must be a float32 tensor (N, 3) or (B, N, 3) or a PointCloud")
    lead, N = tuple(x.shape[:-2]), int(x.shape[-2])
    if isinstance(npoint, bool) or not isinstance(npoint, int) or npoint < 0:
        raise ValueError("npoint must be a non-negative integer, got %r" % (npoint,))
    if isinstance(first, bool) or not isinstance(first, int):
        raise ValueError("first must be an integer, got %r" % (first,))
    if valid is not None and (not isinstance(valid, torch.Tensor) or tuple(valid.shape) != lead + (N,) or valid.dtype not in (torch.bool, torch.uint8)):
        raise ValueError("valid must be a bool / uint8 tensor shaped %r" % (lead + (N,),))
    if npoint > N:
        raise ValueError("farthest_point_sample: npoint %d exceeds the %d points of a cloud" % (npoint, N))
    if include_ends and N < 2:
        raise ValueError("farthest_point_sample: include_ends needs at least two points")
    if N >= 1 << 31:
        raise ValueError("a cloud holds %d points: the sampler takes fewer than 2^31" % N)
    if N and not 0 <= first < N:
        raise ValueError("farthest_point_sample: first %d is outside [0, %d)" % (first, N))
    if not all(t is None or t.is_cuda for t in (x, valid)):
        raise ops.L.OvgError("farthest_point_sample needs HIP device tensors: there is no CPU fallback")
    B = 1 if not lead else lead[0]
    if N == 0 or npoint == 0 or B == 0:
        dist = torch.full(lead + (N,), float("inf"), device=x.device, dtype=torch.float32) if return_distance else None
        return FPSResult(torch.empty(lead + (npoint,), device=x.device, dtype=torch.int32),
                         torch.empty(lead + (npoint,), device=x.device, dtype=torch.float32), dist)
    v = None if valid is None else (valid.to(torch.uint8) if valid.dtype == torch.bool else valid).reshape(B, N).contiguous()
    idx, sq, dist = ops.farthest_point_sample(x.reshape(B, N, 3).contiguous(), npoint, v, first=first, include_last=bool(include_ends),
                                              distance=bool(return_distance))
    return FPSResult(idx.reshape(lead + (npoint,)), sq.reshape(lead + (npoint,)), None if dist is None else dist.reshape(lead + (N,)))


def farthest_point_downsample(cloud, n, first=0):
    """The n farthest-point samples of a PointCloud (farthest_point_sample from point `first`) as a PointCloud, in selection order:
    a preview or evaluation subset of exactly n well-spread points, where voxel_downsample gives one point per cell. points, colors and
    conf are gathered, `indices` are the input cloud's at the samples when it has them (so they still name pixels of the prediction
    maps) and the positions in the input cloud otherwise; transform, extrinsic, conf_threshold and scene_scale are passed through
    unchanged. write_ply, write_glb and render_point_cloud accept the result as they are. Samples of -1 (a cloud without a usable
    point) are dropped; counting them is the one device -> host synchronisation. n above the cloud's size raises ValueError."""
    M = len(cloud)
    res = farthest_point_sample(cloud.points.reshape(M, 3), n, first=first)
    idx = res.index[res.index >= 0].long()                                  # the one synchronisation
    return PointCloud(cloud.points.reshape(M, 3)[idx], None if cloud.colors is None else cloud.colors.reshape(M, 3)[idx],
                      cloud.conf_threshold, cloud.scene_scale, cloud.transform, cloud.extrinsic,
                      idx if cloud.indices is None else cloud.indices[idx], None if cloud.conf is None else cloud.conf[idx])


# ---------------------------------------------------------------------------------------------------------------------------------
# Voxel-grid decimation and the PLY / GLB writers
# ---------------------------------------------------------------------------------------------------------------------------------

def voxel_downsample(cloud, voxel_size=None, rel_size=None, conf=None):
    """Voxel-grid decimation of a PointCloud on the device (ovg_voxel_downsample): one point per occupied cell of a regular grid.

    Exactly one of voxel_size (the cell edge in the cloud's units: a positive float or a 0-d f32 device tensor) and rel_size (a positive
    float; the edge is f32(rel_size) * cloud.scene_scale, one f32 multiply on the device, no host copy) must be given. The rule is
    exact (tests/voxelgrid_twin.py restates it in numpy): points with a non-finite coordinate are dropped; the grid starts at the
    component-wise minimum of the others; cell = floor((p - origin) / edge) in f32; inside a cell the point with the largest `conf`
    wins (an optional (M,) f32 device tensor, e.g. cloud.conf of predictions_to_point_cloud(return_conf=True); NaN ranks lowest), ties
    and calls without conf go to the earliest point; the winners keep their input order. Two calls give identical bytes.

    The result carries the winners' points and colors, `indices` composed with the input cloud's when it has them (so they still name
    pixels of the prediction maps; positions in the input cloud otherwise) and `conf` gathered from the argument (or from cloud.conf).
    transform, extrinsic, conf_threshold and scene_scale are passed through unchanged: scene_scale still describes the full selection.
    write_ply / write_glb accept the result as they are.

    Exactly one device -> host synchronisation (the count and the kernel's flags in one copy). A grid of more than 2^21 cells along an
    axis, or an edge that is not positive on the device, raises ValueError. An empty cloud returns an empty cloud without a launch.
    CPU tensors raise OvgError: there is no CPU fallback."""
    import math
    L = ops.L
    if (voxel_size is None) == (rel_size is None):
        raise ValueError("voxel_downsample: give exactly one of voxel_size and rel_size")
    given = voxel_size if rel_size is None else rel_size
    if isinstance(given, torch.Tensor):
        if rel_size is not None or given.numel() != 1:
            raise ValueError("voxel_downsample: rel_size must be a float, voxel_size a float or a one-element tensor")
    else:
        given = float(given)
        if not (given > 0.0 and math.isfinite(given)):
            raise ValueError("voxel_downsample: the size must be positive and finite, got %r" % given)
    pts, col = cloud.points, cloud.colors
    for t in (pts, col, conf, given if isinstance(given, torch.Tensor) else None):
        if t is not None and not (isinstance(t, torch.Tensor) and t.is_cuda):
            raise L.OvgError("voxel_downsample needs HIP device tensors: there is no CPU fallback")
    M = int(pts.shape[0])
    if conf is not None and tuple(conf.shape) != (M,):
        raise ValueError("voxel_downsample: conf must be (M,) = (%d,), got %r" % (M, tuple(conf.shape)))
    src_conf = conf if conf is not None else cloud.conf
    if M == 0:
        return PointCloud(pts, col, cloud.conf_threshold, cloud.scene_scale, cloud.transform, cloud.extrinsic, cloud.indices, src_conf)
    dev = pts.device
    pts = pts.reshape(M, 3).float().contiguous()
    col = col.reshape(M, 3).contiguous()
    rank = None if conf is None else conf.float().contiguous()
    if isinstance(given, torch.Tensor):
        voxel = given.detach().to(torch.float32).reshape(())
    else:
        voxel = torch.full((), given, device=dev, dtype=torch.float32)
        if rel_size is not None:
            voxel = voxel * cloud.scene_scale.to(torch.float32).reshape(())
    ws = torch.empty(ops.voxel_downsample_workspace_bytes(M), device=dev, dtype=torch.uint8)
    count = torch.empty(2, device=dev, dtype=torch.int64)
    args = dict(points=pts, voxel=voxel, ws=ws, conf=rank, colors=col)
    ops.voxel_downsample(L.VG_COUNT, out_count=count, **args)
    kept, flags = (int(v) for v in count.cpu().tolist())                 # the one synchronisation
    if flags:
        ok = torch.isfinite(pts).all(dim=1)
        extent = (pts[ok].max(dim=0).values - pts[ok].min(dim=0).values).tolist() if bool(ok.any()) else []
        what = "is not a positive finite number" if flags & L.VG_BAD_VOXEL else "gives more than 2^21 cells along an axis"
        raise ValueError("voxel_downsample: voxel size %r %s (extent of the cloud %r)" % (float(voxel), what, extent))
    out_pts = torch.empty(kept, 3, device=dev, dtype=torch.float32)
    out_col = torch.empty(kept, 3, device=dev, dtype=torch.uint8)
    out_idx = torch.empty(kept, device=dev, dtype=torch.int64)
    if kept:
        ops.voxel_downsample(L.VG_SCATTER, capacity=kept, out_points=out_pts, out_colors=out_col, out_index=out_idx, **args)
    indices = out_idx if cloud.indices is None else cloud.indices[out_idx]
    return PointCloud(out_pts, out_col, cloud.conf_threshold, cloud.scene_scale, cloud.transform, cloud.extrinsic, indices,
                      None if src_conf is None else src_conf[out_idx])


def _host_cloud(cloud):
    import numpy as np
    pts = cloud.points.detach().cpu().numpy().astype(np.float32).reshape(-1, 3)
    col = cloud.colors.detach().cpu().numpy().astype(np.uint8).reshape(-1, 3)
    return pts, col


def write_ply(path, cloud, apply_transform=True, normals=None):
    """Binary little-endian PLY of the cloud: `x y z` float, `red green blue` uchar per vertex. apply_transform: the vertices are
    mapped by cloud.transform in float64 on the host and stored as float32 (as the aligned scene shows them); False stores them as
    selected. An empty cloud (M = 0) writes a valid file with no vertices.
    normals: an optional (M, 3) float32 tensor (estimate_normals); the vertex then carries `nx ny nz` float after `x y z`. Under
    apply_transform they are mapped by the inverse transpose of the transform's linear part in float64 and renormalised (zero
    normals stay zero). Without normals the file is the same, byte for byte, as before they existed."""
    import numpy as np
    pts, col = _host_cloud(cloud)
    nrm = None
    if normals is not None:
        if not isinstance(normals, torch.Tensor) or normals.dtype != torch.float32 or tuple(normals.shape) != (len(pts), 3):
            raise ValueError("normals must be a float32 tensor (%d, 3)" % len(pts))
        nrm = normals.detach().cpu().numpy()
    if apply_transform and len(pts):
        T = np.asarray(cloud.transform, dtype=np.float64)
        pts = (pts.astype(np.float64) @ T[:3, :3].T + T[:3, 3]).astype(np.float32)
        if nrm is not None:
            n64 = nrm.astype(np.float64) @ np.linalg.inv(T[:3, :3])          # rows n^T A^-1 = (A^-T n)^T
            length = np.sqrt((n64 * n64).sum(1, keepdims=True))
            nrm = np.where(length > 0, n64 / np.where(length > 0, length, 1.0), 0.0).astype(np.float32)
    fields = [("x", "<f4"), ("y", "<f4"), ("z", "<f4")] + ([("nx", "<f4"), ("ny", "<f4"), ("nz", "<f4")] if nrm is not None else [])
    rec = np.empty(len(pts), dtype=fields + [("red", "u1"), ("green", "u1"), ("blue", "u1")])
    rec["x"], rec["y"], rec["z"] = pts[:, 0], pts[:, 1], pts[:, 2]
    if nrm is not None:
        rec["nx"], rec["ny"], rec["nz"] = nrm[:, 0], nrm[:, 1], nrm[:, 2]
    rec["red"], rec["green"], rec["blue"] = col[:, 0], col[:, 1], col[:, 2]
    header = ("ply\nformat binary_little_endian 1.0\nelement vertex %d\nproperty float x\nproperty float y\nproperty float z\n%s"
              "property uchar red\nproperty uchar green\nproperty uchar blue\nend_header\n"
              % (len(pts), "property float nx\nproperty float ny\nproperty float nz\n" if nrm is not None else ""))
    with open(path, "wb") as fh:
        fh.write(header.encode("ascii"))
        fh.write(rec.tobytes())


CAMERA_COLORS = ((230, 25, 75), (60, 180, 75), (255, 225, 25), (0, 130, 200), (245, 130, 48), (145, 30, 180), (70, 240, 240),
                 (240, 50, 230))
_FRUSTUM_FACES = (0, 1, 2, 0, 2, 3, 0, 3, 4, 0, 4, 1, 1, 3, 2, 1, 4, 3)    # four sides from the apex, two triangles of the base


def camera_frusta(extrinsic, height):
    """(S, 5, 3) float64 vertices of one four-sided pyramid per camera-from-world (3,4) extrinsic: vertex 0 the apex at the camera
    centre -R^T t, vertices 1..4 the square base at distance `height` along the camera's +z axis, its corners height / 2 away from
    the axis on the diagonals of the image plane (the reference's cone of radius 0.05 and height 0.1 scene scales turned by 45 degrees,
    visual_util.py:270-318, has the same proportions)."""
    import numpy as np
    e = np.asarray(extrinsic, dtype=np.float64).reshape(-1, 3, 4)
    Rt = e[:, :, :3].transpose(0, 2, 1)                                   # world-from-camera rotations
    centre = -np.einsum("sij,sj->si", Rt, e[:, :, 3])
    a = height / 2.0 / np.sqrt(2.0)
    local = np.array([[0.0, 0.0, 0.0], [a, a, height], [-a, a, height], [-a, -a, height], [a, -a, height]])
    return centre[:, None, :] + np.einsum("sij,vj->svi", Rt, local)


def _glb_add_cameras(gltf, node, binary, extrinsic, height):
    """One TRIANGLES primitive per camera (camera_frusta of the given height, CAMERA_COLORS cycled, double-sided) appended to mesh 0
    of `gltf` under `node`. -> the binary chunk with the cameras' buffers behind what it held."""
    import numpy as np
    ext = extrinsic
    ext = ext.detach().cpu().numpy() if isinstance(ext, torch.Tensor) else np.asarray(ext)
    verts = camera_frusta(ext, height).astype("<f4")
    S = len(verts)
    if S:
        binary += b"\0" * (-len(binary) % 4)
        rgba = np.array([CAMERA_COLORS[i % len(CAMERA_COLORS)] + (255,) for i in range(S)], np.uint8)
        parts = [verts.tobytes(), np.repeat(rgba[:, None, :], 5, axis=1).tobytes(), np.tile(np.array(_FRUSTUM_FACES, "<u2"), S).tobytes()]
        views, accs = gltf.setdefault("bufferViews", []), gltf.setdefault("accessors", [])
        prims = gltf.setdefault("meshes", [{"primitives": []}])[0]["primitives"]
        v0 = len(views)
        for part, target in zip(parts, (34962, 34962, 34963)):
            views.append({"buffer": 0, "byteOffset": len(binary), "byteLength": len(part), "target": target})
            binary += part
        gltf["materials"] = [{"doubleSided": True}]
        for i in range(S):
            a0 = len(accs)
            accs += [{"bufferView": v0, "byteOffset": 60 * i, "componentType": 5126, "count": 5, "type": "VEC3",
                      "min": [float(v) for v in verts[i].min(axis=0)], "max": [float(v) for v in verts[i].max(axis=0)]},
                     {"bufferView": v0 + 1, "byteOffset": 20 * i, "componentType": 5121, "normalized": True, "count": 5, "type": "VEC4"},
                     {"bufferView": v0 + 2, "byteOffset": 36 * i, "componentType": 5123, "count": 18, "type": "SCALAR"}]
            prims.append({"attributes": {"POSITION": a0, "COLOR_0": a0 + 1}, "indices": a0 + 2, "mode": 4, "material": 0})
        node["mesh"] = 0
        gltf["buffers"] = [{"byteLength": len(binary)}]
    return binary


def _glb_write(path, gltf, binary):
    """The GLB container: header, the JSON chunk padded with spaces, the binary chunk padded with zeros (when there is one)."""
    import json
    import struct
    js = json.dumps(gltf, separators=(",", ":")).encode("utf-8")
    js += b" " * (-len(js) % 4)
    binary += b"\0" * (-len(binary) % 4)
    chunks = struct.pack("<II", len(js), 0x4E4F534A) + js
    if binary:
        chunks += struct.pack("<II", len(binary), 0x004E4942) + binary
    with open(path, "wb") as fh:
        fh.write(struct.pack("<III", 0x46546C67, 2, 12 + len(chunks)))
        fh.write(chunks)


def write_glb(path, cloud, cameras=False, camera_scale=0.05):
    """glTF 2.0 binary of the cloud: one POINTS primitive with POSITION (f32 VEC3, with the min / max the spec requires) and COLOR_0
    (normalized u8 VEC4, alpha 255), under one node whose `matrix` is cloud.transform (column-major, as glTF stores it). The vertices
    stay untransformed, as in the reference's file: trimesh's Scene.apply_transform moves the scene graph, not the vertex buffer. This
    follows the reference file's structure; it was not compared byte-wise with trimesh's export (trimesh is not a dependency here).
    An empty cloud writes a node without a mesh.

    cameras=True adds one TRIANGLES primitive per camera of cloud.extrinsic to the same mesh, so under the same aligned node: a
    four-sided pyramid (camera_frusta) with its apex at the camera centre, opening along the camera's +z axis, of height
    camera_scale * cloud.scene_scale, in one flat colour per camera from CAMERA_COLORS (cycled), double-sided. This follows the
    reference's placement and size rule (visual_util.py:270-318); the reference builds its cones with trimesh, so the files are not
    compared byte-wise. With cameras=False the file is what it was without the argument."""
    import numpy as np
    pts, col = _host_cloud(cloud)
    M = len(pts)
    node = {"matrix": [float(v) for v in np.asarray(cloud.transform, dtype=np.float64).T.reshape(-1)]}
    gltf = {"asset": {"version": "2.0", "generator": "omnivggt_official_amd.postprocess"}, "scene": 0, "scenes": [{"nodes": [0]}],
            "nodes": [node]}
    binary = b""
    if M:
        rgba = np.concatenate([col, np.full((M, 1), 255, np.uint8)], axis=1)
        pos_bytes, col_bytes = pts.astype("<f4").tobytes(), rgba.tobytes()
        binary = pos_bytes + col_bytes
        node["mesh"] = 0
        gltf["meshes"] = [{"primitives": [{"attributes": {"POSITION": 0, "COLOR_0": 1}, "mode": 0}]}]
        gltf["buffers"] = [{"byteLength": len(binary)}]
        gltf["bufferViews"] = [{"buffer": 0, "byteOffset": 0, "byteLength": len(pos_bytes), "target": 34962},
                               {"buffer": 0, "byteOffset": len(pos_bytes), "byteLength": len(col_bytes), "target": 34962}]
        gltf["accessors"] = [{"bufferView": 0, "componentType": 5126, "count": M, "type": "VEC3",
                              "min": [float(v) for v in pts.min(axis=0)], "max": [float(v) for v in pts.max(axis=0)]},
                             {"bufferView": 1, "componentType": 5121, "normalized": True, "count": M, "type": "VEC4"}]
    if cameras:
        binary = _glb_add_cameras(gltf, node, binary, cloud.extrinsic, float(camera_scale) * float(cloud.scene_scale))
    _glb_write(path, gltf, binary)


# ---------------------------------------------------------------------------------------------------------------------------------
# Headless rendering of a PointCloud (what inference.py hands to viser_wrapper, as images)
# ---------------------------------------------------------------------------------------------------------------------------------

class RenderResult:
    """Result of render_point_cloud: rgb (V,H,W,3) u8, depth (V,H,W) f32 or None, index (V,H,W) int64 or None, device tensors."""
    __slots__ = ("rgb", "depth", "index")

    def __init__(self, rgb, depth=None, index=None):
        self.rgb, self.depth, self.index = rgb, depth, index


def render_point_cloud(cloud, extrinsic, intrinsic, size, point_radius=1, near=1e-3, background=(255, 255, 255), return_depth=True,
                       return_index=False):
    """Draw a PointCloud from V pinhole cameras into 8-bit images on the device (ovg_render_points): every point becomes a square of
    (2 point_radius + 1)^2 pixels around its rounded projection, the nearest point of a pixel wins, equal depths go to the earliest
    point. The rule is exact (tests/render_twin.py restates it in numpy float32) and two calls give identical bytes.

    extrinsic: (V,3,4) (or one (3,4)) world-to-camera in the frame of cloud.points -- the untransformed frame predictions["extrinsic"]
    lives in, not the aligned frame of cloud.transform. intrinsic: (V,3,3), or one (3,3) for all views; fx, fy, cx, cy are read, skew
    is ignored. Both may be device tensors, numpy arrays or lists; they are rounded to f32 and packed on the device. size: (H, W).
    Pixel centres sit at integer coordinates (the convention of unproject_depth_map_to_point_map), points with camera depth <= near
    or a non-finite camera coordinate are not drawn, pixels no point reaches take `background`, depth 0 and index -1.

    -> RenderResult(rgb (V,H,W,3) u8, depth (V,H,W) f32 camera z of the winning point or None, index (V,H,W) int64 or None).
    index names POSITIONS IN `cloud` (rows of cloud.points), also when the cloud carries `indices`: cloud.indices[index] (where
    index >= 0) maps on to the pixels of the prediction maps.

    No device -> host synchronisation: every size is known before the launches. An empty cloud returns background images. CPU
    clouds raise OvgError (there is no CPU fallback); a bad size, point_radius, near or background raises ValueError."""
    import math
    import numpy as np
    L = ops.L
    try:
        H, W = (int(v) for v in size)
        ok = (H, W) == tuple(size) and H > 0 and W > 0
    except (TypeError, ValueError):
        ok = False
    if not ok:
        raise ValueError("render_point_cloud: size must be (H, W), two positive integers, got %r" % (size,))
    if isinstance(point_radius, bool) or not isinstance(point_radius, (int, np.integer)) or not 0 <= point_radius <= L.RENDER_MAX_RADIUS:
        raise ValueError("render_point_cloud: point_radius must be an integer in [0, %d], got %r" % (L.RENDER_MAX_RADIUS, point_radius))
    try:
        near32 = float(np.float32(near))
    except (TypeError, ValueError):
        near32 = float("nan")
    if not (near32 > 0.0 and math.isfinite(near32)):
        raise ValueError("render_point_cloud: near must be positive and finite in float32, got %r" % (near,))
    try:
        bg = tuple(int(v) for v in background)
        ok = len(bg) == 3 and all(0 <= v <= 255 for v in bg) and bg == tuple(background)
    except (TypeError, ValueError):
        ok = False
    if not ok:
        raise ValueError("render_point_cloud: background must be three integers in [0, 255], got %r" % (background,))
    ext, intr = torch.as_tensor(extrinsic).detach(), torch.as_tensor(intrinsic).detach()
    if ext.dim() == 2:
        ext = ext[None]
    if ext.dim() != 3 or tuple(ext.shape[1:]) != (3, 4) or ext.shape[0] == 0:
        raise ValueError("render_point_cloud: extrinsic must be (V, 3, 4), got %r" % (tuple(ext.shape),))
    V = int(ext.shape[0])
    if tuple(intr.shape) not in ((3, 3), (V, 3, 3)):
        raise ValueError("render_point_cloud: intrinsic must be (3, 3) or (V, 3, 3) = (%d, 3, 3), got %r" % (V, tuple(intr.shape)))
    if V * H * W >= 1 << 31:
        raise ValueError("render_point_cloud: V * H * W = %d pixels is 2^31 or more; render fewer views per call" % (V * H * W))
    pts, col = cloud.points, cloud.colors
    if not (isinstance(pts, torch.Tensor) and pts.is_cuda and isinstance(col, torch.Tensor) and col.is_cuda):
        raise L.OvgError("render_point_cloud needs HIP device tensors: there is no CPU fallback")
    M = int(pts.shape[0])
    if M >= 1 << 32:
        raise ValueError("render_point_cloud: the cloud has 2^32 points or more")
    dev = pts.device
    cams = _pack_cams(ext, intr, V, dev)
    rgb, depth, index = ops.render_points(pts.reshape(M, 3).float().contiguous(), col.reshape(M, 3).contiguous(), cams, H, W,
                                          radius=int(point_radius), near=near32, background=bg, depth=return_depth, index=return_index)
    return RenderResult(rgb, depth, index)


def orbit_cameras(extrinsic0, centre, n, axis=None):
    """n world-to-camera (3,4) extrinsics on a circle: camera k is camera 0 moved rigidly by a rotation of 2 pi k / n about the line
    through `centre` along `axis` -- E_k = E_0 T(centre) R_axis(-theta_k) T(-centre) in 4x4 matrices, so E_0 comes back for k = 0,
    every camera keeps its distance to `centre` and sees `centre` at the same place in its image. axis: a world direction, by
    default camera 0's up direction (minus the second row of its rotation: image y points down). Host only: float64 numpy in,
    (n, 3, 4) float64 numpy out; device tensors are copied to the host."""
    import numpy as np

    def host(a):
        return np.asarray(a.detach().cpu().numpy() if isinstance(a, torch.Tensor) else a, dtype=np.float64)

    e0 = np.eye(4)
    e0[:3, :4] = host(extrinsic0).reshape(3, 4)
    c = host(centre).reshape(3)
    if isinstance(n, bool) or not isinstance(n, (int, np.integer)) or n < 1:
        raise ValueError("orbit_cameras: n must be a positive integer, got %r" % (n,))
    a = -e0[1, :3] if axis is None else host(axis).reshape(3)
    norm = float(np.linalg.norm(a))
    if not (norm > 0.0 and np.isfinite(norm)):
        raise ValueError("orbit_cameras: the axis must be a finite non-zero vector, got %r" % (a.tolist(),))
    a = a / norm
    K = np.array([[0.0, -a[2], a[1]], [a[2], 0.0, -a[0]], [-a[1], a[0], 0.0]])
    t_in, t_out = np.eye(4), np.eye(4)
    t_in[:3, 3], t_out[:3, 3] = -c, c
    out = np.empty((int(n), 3, 4))
    for k in range(int(n)):
        th = -2.0 * np.pi * k / int(n)
        rot = np.eye(4)
        rot[:3, :3] = np.eye(3) + np.sin(th) * K + (1.0 - np.cos(th)) * (K @ K)      # Rodrigues
        out[k] = (e0 @ t_out @ rot @ t_in)[:3]
    return out


def cloud_centre(cloud):
    """(3,) f32 device tensor: the per-axis median of cloud.points (ovg_percentile with q = 50: numpy's linear percentile, exact and
    deterministic), a robust centre for orbit_cameras. A NaN coordinate anywhere makes that axis NaN, as in numpy."""
    pts = cloud.points
    if not (isinstance(pts, torch.Tensor) and pts.is_cuda):
        raise ops.L.OvgError("cloud_centre needs HIP device tensors: there is no CPU fallback")
    M = int(pts.shape[0])
    if M == 0:
        raise ValueError("cloud_centre of an empty cloud")
    return ops.percentile(pts.reshape(M, 3).float().contiguous(), M, 3, 1, 3, [50.0]).reshape(3)


def write_png(path, image):
    """One (H, W, 3) u8 image (a device or host tensor, or an array) as an 8-bit RGB PNG, through Pillow."""
    import numpy as np
    from PIL import Image
    a = image.detach().cpu().numpy() if isinstance(image, torch.Tensor) else np.asarray(image)
    if a.dtype != np.uint8 or a.ndim != 3 or a.shape[2] != 3:
        raise ValueError("write_png: expected one (H, W, 3) uint8 image, got %s %r" % (a.dtype, a.shape))
    Image.fromarray(np.ascontiguousarray(a)).save(path, format="PNG")


# ---------------------------------------------------------------------------------------------------------------------------------
# Volumetric fusion: depth maps into a TSDF volume, one mesh from its zero level (ovg_tsdf_integrate, ovg_tsdf_extract)
# ---------------------------------------------------------------------------------------------------------------------------------

TSDF_MAX_VOXELS = 1 << 28          # lattice points tsdf_volume allocates at most: 2 GiB of tsdf + weight, 4 GiB more with colours
TSDF_TRUNC_VOXELS = 4.0            # the default truncation distance in voxels
TSDF_MAX_WEIGHT = 64.0             # the default clamp of a lattice point's weight


class TSDFVolume:
    """A dense truncated signed-distance volume on the device: tsdf, weight (nz,ny,nx) f32 and color (nz,ny,nx,4) f32 (r, g, b in
    [0, 255] and the colour weight) or None; origin (three floats, float32 values: the position of lattice point (0, 0, 0)),
    voxel_size and trunc (floats, float32 values), dims = (nx, ny, nz). Lattice point (i, j, k) lies at origin + voxel_size (i, j, k).
    transform ((4,4) float64 numpy or None), extrinsic and scene_scale travel to the meshes extracted from it, for the writers."""
    __slots__ = ("tsdf", "weight", "color", "origin", "voxel_size", "trunc", "dims", "transform", "extrinsic", "scene_scale")

    def __init__(self, tsdf, weight, color, origin, voxel_size, trunc, dims, transform=None, extrinsic=None, scene_scale=None):
        self.tsdf, self.weight, self.color, self.origin, self.voxel_size, self.trunc, self.dims = tsdf, weight, color, origin, voxel_size, trunc, dims
        self.transform, self.extrinsic, self.scene_scale = transform, extrinsic, scene_scale


class Mesh:
    """Result of tsdf_extract: vertices (M,3) f32, faces (F,3) int32 (indices into vertices, triangle normals pointing from inside to
    outside), normals (M,3) f32 and colors (M,3) u8 device tensors; transform the (4,4) float64 numpy alignment the writers apply
    (identity when the volume carries none); extrinsic (S,3,4) and scene_scale for write_mesh_glb's cameras, or None."""
    __slots__ = ("vertices", "faces", "normals", "colors", "transform", "extrinsic", "scene_scale")

    def __init__(self, vertices, faces, normals, colors, transform, extrinsic=None, scene_scale=None):
        self.vertices, self.faces, self.normals, self.colors, self.transform = vertices, faces, normals, colors, transform
        self.extrinsic, self.scene_scale = extrinsic, scene_scale


MESH_SHADINGS = {"color": 0, "headlight": 1, "normal": 2}
MESH_CULLS = {None: 0, "back": 1, "front": 2}


def render_mesh(mesh, extrinsic, intrinsic, size, shading="headlight", cull=None, smooth=True, near=1e-3, background=(255, 255, 255),
                return_depth=True, return_index=False):
    """Draw a Mesh from V pinhole cameras into 8-bit images on the device (ovg_render_mesh): z-buffered triangles with per-pixel
    perspective-correct depth, colour and normal. The nearest face of a pixel wins, equal depths go to the earliest face, nothing is
    blended. The rule is exact (tests/raster_twin.py restates it in numpy) and two calls give identical bytes.

    extrinsic, intrinsic, size, near, background: as for render_point_cloud -- (V,3,4) or one (3,4) world-to-camera in the frame of
    mesh.vertices (not the aligned frame of mesh.transform), (V,3,3) or one (3,3), (H, W); pixel centres at integer coordinates.
    shading: "headlight" (the vertex colour times 0.25 + 0.75 |n . optical axis|: a light at the camera, both sides lit), "color"
    (the vertex colour alone) or "normal" (the world normal as 255 (n / |n| + 1) / 2). A mesh without colours (mesh.colors None) is
    128 grey. smooth: interpolate mesh.normals; False (or mesh.normals None) shades every face with its own normal. cull: None draws
    both sides, "back" drops faces whose outward normal looks away from the camera, "front" the others.

    NO CLIPPING: a face is not drawn in a view in which one of its vertices has camera depth <= near, a non-finite camera
    coordinate or a projection more than 16384 pixels from the origin of the image -- neither cut at the near plane nor at a guard
    band. A triangle that reaches behind the camera disappears from that view as a whole; subdivide such faces if that matters. A
    face with a vertex index outside the mesh is skipped. Also not in it: anti-aliasing, textures, transparency, a top-left fill rule
    (a pixel centre exactly on a shared edge is covered by both faces, and depth, then the lower face index decide).

    -> RenderResult(rgb (V,H,W,3) u8, depth (V,H,W) f32 camera z of the surface at the pixel centre or None, index (V,H,W) int64 face
    index or None); pixels no face covers take `background`, depth 0 and index -1.

    No device -> host synchronisation: every size is known before the launches. A mesh without faces returns background images.
    CPU meshes raise OvgError (there is no CPU fallback); a bad size, shading, cull, near or background raises ValueError."""
    import math
    import numpy as np
    L = ops.L
    if not isinstance(mesh, Mesh):
        raise ValueError("render_mesh: expected a Mesh")
    try:
        H, W = (int(v) for v in size)
        ok = (H, W) == tuple(size) and H > 0 and W > 0
    except (TypeError, ValueError):
        ok = False
    if not ok:
        raise ValueError("render_mesh: size must be (H, W), two positive integers, got %r" % (size,))
    if not isinstance(shading, str) or shading not in MESH_SHADINGS:
        raise ValueError("render_mesh: shading must be one of %r, got %r" % (sorted(MESH_SHADINGS), shading))
    if not (cull is None or isinstance(cull, str)) or cull not in MESH_CULLS:
        raise ValueError("render_mesh: cull must be None, \"back\" or \"front\", got %r" % (cull,))
    try:
        near32 = float(np.float32(near))
    except (TypeError, ValueError):
        near32 = float("nan")
    if isinstance(near, bool) or not (near32 > 0.0 and math.isfinite(near32)):
        raise ValueError("render_mesh: near must be positive and finite in float32, got %r" % (near,))
    try:
        bg = tuple(int(v) for v in background)
        ok = len(bg) == 3 and all(0 <= v <= 255 for v in bg) and bg == tuple(background)
    except (TypeError, ValueError):
        ok = False
    if not ok:
        raise ValueError("render_mesh: background must be three integers in [0, 255], got %r" % (background,))
    ext, intr = torch.as_tensor(extrinsic).detach(), torch.as_tensor(intrinsic).detach()
    if ext.dim() == 2:
        ext = ext[None]
    if ext.dim() != 3 or tuple(ext.shape[1:]) != (3, 4) or ext.shape[0] == 0:
        raise ValueError("render_mesh: extrinsic must be (V, 3, 4), got %r" % (tuple(ext.shape),))
    V = int(ext.shape[0])
    if tuple(intr.shape) not in ((3, 3), (V, 3, 3)):
        raise ValueError("render_mesh: intrinsic must be (3, 3) or (V, 3, 3) = (%d, 3, 3), got %r" % (V, tuple(intr.shape)))
    if V * H * W >= 1 << 31:
        raise ValueError("render_mesh: V * H * W = %d pixels is 2^31 or more; render fewer views per call" % (V * H * W))
    vert, faces = mesh.vertices, mesh.faces
    for t in (vert, faces, mesh.normals, mesh.colors):
        if t is not None and not (isinstance(t, torch.Tensor) and t.is_cuda):
            raise L.OvgError("render_mesh needs HIP device tensors: there is no CPU fallback")
    if vert is None or faces is None:
        raise ValueError("render_mesh: the mesh has no vertices or no faces tensor")
    M, F = int(vert.shape[0]), int(faces.shape[0])
    if M >= 1 << 31 or F >= 1 << 31:
        raise ValueError("render_mesh: the mesh has 2^31 vertices or faces or more")
    cams = _pack_cams(ext, intr, V, vert.device)
    normals = mesh.normals.reshape(M, 3).float().contiguous() if smooth and mesh.normals is not None else None
    colors = mesh.colors.reshape(M, 3).contiguous() if mesh.colors is not None else None
    rgb, depth, index = ops.render_mesh(vert.reshape(M, 3).float().contiguous(), faces.reshape(F, 3).to(torch.int32).contiguous(), cams, H, W,
                                        normals=normals, colors=colors, shading=MESH_SHADINGS[shading], cull=MESH_CULLS[cull], near=near32,
                                        background=bg, depth=return_depth, index=return_index)
    return RenderResult(rgb, depth, index)


def _tsdf_positive(what, name, value):
    import math
    import numpy as np
    try:
        with np.errstate(over="ignore"):
            v = float(np.float32(value))
    except (TypeError, ValueError):
        v = float("nan")
    if isinstance(value, bool) or not (v > 0.0 and math.isfinite(v)):
        raise ValueError("%s: %s must be positive and finite in float32, got %r" % (what, name, value))
    return v


def tsdf_volume(origin, voxel_size, dims, trunc=None, color=True, device="cuda", max_voxels=TSDF_MAX_VOXELS):
    """A fresh TSDFVolume (tsdf 1, everything else 0) of dims = (nx, ny, nz) lattice points with its point (0, 0, 0) at `origin`.
    trunc: the truncation distance in world units, TSDF_TRUNC_VOXELS voxels by default. A volume above max_voxels lattice points
    (TSDF_MAX_VOXELS by default; 2^31 - 1 at the most) is refused with a ValueError that names its size."""
    import math
    import numpy as np
    what = "tsdf_volume"
    try:
        o = [float(np.float32(v)) for v in origin]
    except (TypeError, ValueError):
        o = []
    if len(o) != 3 or not all(math.isfinite(v) for v in o):
        raise ValueError("%s: origin must be three finite numbers, got %r" % (what, origin))
    voxel = _tsdf_positive(what, "voxel_size", voxel_size)
    trunc = _tsdf_positive(what, "trunc", TSDF_TRUNC_VOXELS * voxel if trunc is None else trunc)
    try:
        d = tuple(dims)
    except TypeError:
        d = ()
    if len(d) != 3 or any(isinstance(v, bool) or not isinstance(v, (int, np.integer)) or v < 1 for v in d):
        raise ValueError("%s: dims must be three positive integers (nx, ny, nz), got %r" % (what, dims))
    nx, ny, nz = (int(v) for v in d)
    if isinstance(max_voxels, bool) or not isinstance(max_voxels, int) or max_voxels < 1:
        raise ValueError("%s: max_voxels must be a positive integer, got %r" % (what, max_voxels))
    if nx * ny * nz > min(max_voxels, (1 << 31) - 1):
        raise ValueError("%s: %d x %d x %d = %d lattice points exceed max_voxels = %d (%.1f GiB of volume state): use a larger voxel_size "
                         "or a smaller resolution" % (what, nx, ny, nz, nx * ny * nz, min(max_voxels, (1 << 31) - 1),
                                                       nx * ny * nz * (24 if color else 8) / 2.0 ** 30))
    dev = torch.device(device)
    if dev.type != "cuda":
        raise ops.L.OvgError("tsdf_volume needs a HIP device: there is no CPU fallback")
    return TSDFVolume(torch.ones(nz, ny, nx, device=dev, dtype=torch.float32), torch.zeros(nz, ny, nx, device=dev, dtype=torch.float32),
                      torch.zeros(nz, ny, nx, 4, device=dev, dtype=torch.float32) if color else None, tuple(o), voxel, trunc, (nx, ny, nz))


def tsdf_volume_for(points_or_cloud, voxel_size=None, resolution=256, margin=TSDF_TRUNC_VOXELS, valid=None, trunc=None, color=True,
                    max_voxels=TSDF_MAX_VOXELS):
    """A fresh TSDFVolume round a PointCloud or a (..., 3) f32 device tensor of points (e.g. world_points_from_depth): the bounds of
    the finite points (those with valid != 0 when a bool / u8 tensor of the leading shape is given) by torch reductions, `margin`
    voxels (rounded up to whole voxels) added on every side so that the free space in front of a surface is part of the volume.
    voxel_size None: the longest side, margins included, spans `resolution` lattice points. One device -> host read-back: the six
    bounds. A PointCloud hands its transform, cameras and scene scale on to the volume. ValueError for bad arguments, no finite
    point, or a volume above max_voxels; OvgError for CPU tensors."""
    import math
    import numpy as np
    what = "tsdf_volume_for"
    cloud = points_or_cloud if isinstance(points_or_cloud, PointCloud) else None
    pts = cloud.points if cloud is not None else points_or_cloud
    if not isinstance(pts, torch.Tensor) or pts.dtype != torch.float32 or pts.dim() < 2 or pts.shape[-1] != 3:
        raise ValueError("%s: expected a PointCloud or a float32 tensor (..., 3)" % what)
    if valid is not None and (not isinstance(valid, torch.Tensor) or valid.dtype not in (torch.bool, torch.uint8)
                              or tuple(valid.shape) != tuple(pts.shape[:-1])):
        raise ValueError("%s: valid must be a bool / uint8 tensor %r" % (what, tuple(pts.shape[:-1])))
    if voxel_size is not None:
        voxel_size = _tsdf_positive(what, "voxel_size", voxel_size)
    if isinstance(margin, bool) or not isinstance(margin, (int, float)) or not (0 <= margin <= 1024):
        raise ValueError("%s: margin must be a number of voxels in [0, 1024], got %r" % (what, margin))
    pad = int(math.ceil(margin))
    if isinstance(resolution, bool) or not isinstance(resolution, (int, np.integer)) or not 2 * pad + 2 <= resolution < 1 << 31:
        raise ValueError("%s: resolution must be an integer >= 2 * margin + 2 = %d, got %r" % (what, 2 * pad + 2, resolution))
    if not pts.is_cuda or (valid is not None and not valid.is_cuda):
        raise ops.L.OvgError("tsdf_volume_for needs HIP device tensors: there is no CPU fallback")
    p = pts.reshape(-1, 3)
    ok = torch.isfinite(p).all(dim=1)
    if valid is not None:
        ok = ok & (valid.reshape(-1) != 0)
    inf = torch.full((), float("inf"), device=p.device, dtype=torch.float32)
    lo = torch.where(ok[:, None], p, inf).amin(dim=0) if p.shape[0] else inf.expand(3)
    hi = torch.where(ok[:, None], p, -inf).amax(dim=0) if p.shape[0] else (-inf).expand(3)
    b = torch.cat([lo, hi]).double().cpu().numpy()                          # the one read-back
    if not np.isfinite(b).all():
        raise ValueError("%s: no finite point to bound the volume with" % what)
    lo, extent = b[:3], b[3:] - b[:3]
    if voxel_size is None:
        voxel_size = float(np.float32(max(float(extent.max()), 1e-30) / (int(resolution) - 1 - 2 * pad)))
        voxel_size = _tsdf_positive(what, "the voxel size derived from the bounds", voxel_size)
    # 1e-4 of a voxel of slack: a voxel size derived from the longest side (and rounded to float32) spans exactly `resolution` points
    dims = tuple(int(math.ceil(float(e) / voxel_size - 1e-4)) + 1 + 2 * pad for e in extent)
    vol = tsdf_volume([float(v) - pad * voxel_size for v in lo], voxel_size, dims, trunc=trunc, color=color, device=p.device,
                      max_voxels=max_voxels)
    if cloud is not None:
        vol.transform, vol.extrinsic, vol.scene_scale = cloud.transform, cloud.extrinsic, cloud.scene_scale
    return vol


def _tsdf_colors(images, S, H, W):
    """(S,H,W,3) u8 from (S,3,H,W) floats in [0, 1] by ovg_point_filter's colour rule u8(trunc(clamp(x * 255f, 0, 255))), NaN as 0;
    (S,H,W,3) u8 as it is."""
    if isinstance(images, torch.Tensor) and images.dtype == torch.uint8 and tuple(images.shape) == (S, H, W, 3):
        return images.contiguous()
    if isinstance(images, torch.Tensor) and images.is_floating_point() and tuple(images.shape) == (S, 3, H, W):
        x = torch.nan_to_num(images.float() * 255.0, nan=0.0, posinf=255.0, neginf=0.0).clamp(0.0, 255.0)
        return x.to(torch.uint8).permute(0, 2, 3, 1).contiguous()
    raise ValueError("tsdf_integrate: images must be (S, 3, H, W) = (%d, 3, %d, %d) floats in [0, 1] or (S, H, W, 3) uint8" % (S, H, W))


def tsdf_integrate(volume, depth, extrinsic, intrinsic, images=None, weight=None, valid=None, near=1e-3, max_weight=TSDF_MAX_WEIGHT,
                   views=None):
    """Averages S depth maps with their cameras into the volume on the device (ovg_tsdf_integrate), in place; -> the volume.
    Every lattice point is projected into each view (the projection of render_point_cloud, nearest pixel) and compared with the
    z-depth d the view holds there: sdf = d - zc. A point more than `trunc` behind the surface is hidden and left alone; otherwise
    min(sdf / trunc, 1) enters the running weighted mean of the point, so a view that sees through a point (a floater of another
    view) pulls it towards free space. The rule is exact (tests/tsdf_twin.py restates it in numpy float32): views are taken in
    ascending order, two calls give identical bytes, and integrating views [0, k) and then [k, S) gives the bytes of one call.

    depth: (S,H,W) or (S,H,W,1) f32 device tensor (predictions["depth"][b]). extrinsic (S,3,4) world-to-camera, intrinsic (S,3,3) or
    one (3,3): device tensors, numpy arrays or lists, rounded to f32. images: (S,3,H,W) floats in [0, 1] or (S,H,W,3) u8 colours for a
    volume with colours; only observations within `trunc` of the surface colour a point. weight: optional (S,H,W) f32 per-pixel
    observation weights (pixels whose weight is not finite and > 0 are skipped); valid: optional (S,H,W) bool / u8; pixels with a
    depth that is not finite or <= near are skipped as well. max_weight clamps a point's accumulated weight. views: None for all, or
    (first, count) / a range of consecutive views. ValueError for shapes and values, OvgError for CPU tensors: no CPU fallback."""
    import numpy as np
    what = "tsdf_integrate"
    if not isinstance(volume, TSDFVolume):
        raise ValueError("%s: expected a TSDFVolume" % what)
    if isinstance(depth, torch.Tensor) and depth.dim() == 4 and depth.shape[-1] == 1:
        depth = depth[..., 0]
    if not isinstance(depth, torch.Tensor) or depth.dim() != 3 or 0 in depth.shape or not depth.is_floating_point():
        raise ValueError("%s: depth must be a (S, H, W) or (S, H, W, 1) float tensor" % what)
    S, H, W = (int(v) for v in depth.shape)
    if S * H * W >= 1 << 31:
        raise ValueError("%s: S = %d views of %d x %d exceed S * H * W < 2^31" % (what, S, H, W))
    ext, intr = torch.as_tensor(extrinsic).detach(), torch.as_tensor(intrinsic).detach()
    if tuple(ext.shape) != (S, 3, 4):
        raise ValueError("%s: extrinsic must be (S, 3, 4) = (%d, 3, 4), got %r" % (what, S, tuple(ext.shape)))
    if tuple(intr.shape) not in ((3, 3), (S, 3, 3)):
        raise ValueError("%s: intrinsic must be (3, 3) or (S, 3, 3) = (%d, 3, 3), got %r" % (what, S, tuple(intr.shape)))
    if valid is not None and (not isinstance(valid, torch.Tensor) or tuple(valid.shape) != (S, H, W)
                              or valid.dtype not in (torch.bool, torch.uint8)):
        raise ValueError("%s: valid must be a bool / uint8 tensor (S, H, W) = %r" % (what, (S, H, W)))
    if weight is not None and (not isinstance(weight, torch.Tensor) or tuple(weight.shape) != (S, H, W) or not weight.is_floating_point()):
        raise ValueError("%s: weight must be a float tensor (S, H, W) = %r" % (what, (S, H, W)))
    colors = None
    if images is not None:
        if volume.color is None:
            raise ValueError("%s: images need a volume with colours" % what)
        colors = _tsdf_colors(images, S, H, W)
    near32, max_weight32 = _tsdf_positive(what, "near", near), _tsdf_positive(what, "max_weight", max_weight)
    if views is None:
        first, count = 0, S
    else:
        if isinstance(views, range):
            views = (views.start, len(views)) if views.step == 1 else None
        if not isinstance(views, (tuple, list)) or len(views) != 2 or any(isinstance(v, bool) or not isinstance(v, (int, np.integer)) for v in views):
            raise ValueError("%s: views must be None, (first, count) or a range of consecutive views" % what)
        first, count = int(views[0]), int(views[1])
        if not (0 <= first < S and 0 < count <= S - first):
            raise ValueError("%s: views %d .. %d outside [0, %d)" % (what, first, first + count - 1, S))
    for t in (volume.tsdf, depth, valid, weight, colors):
        if t is not None and not t.is_cuda:
            raise ops.L.OvgError("tsdf_integrate needs HIP device tensors: there is no CPU fallback")
    dev = volume.tsdf.device
    cams = _pack_cams(ext, intr, S, dev)
    if valid is not None:
        valid = (valid.to(torch.uint8) if valid.dtype == torch.bool else valid).contiguous()
    ops.tsdf_integrate(volume.tsdf, volume.weight, depth.float().contiguous(), cams, volume.origin, volume.voxel_size, volume.trunc,
                       max_weight=max_weight32, near=near32, color=volume.color, valid=valid,
                       obs_weight=None if weight is None else weight.float().contiguous(), colors=colors, view_first=first, view_count=count)
    return volume


def tsdf_extract(volume, min_weight=1.0):
    """The mesh of the volume's zero level by naive surface nets on the device (ovg_tsdf_extract): one vertex per cell whose 8 corners
    carry at least `min_weight` and differ in sign, at the mean of the cell's edge crossings, one quad (two triangles) per
    sign-changing lattice edge whose four cells are all there. Normals are the normalised gradient of the cell (inside to outside),
    colours the mean of the coloured corners (128 grey without any). Deterministic: vertices in ascending cell index, faces in
    ascending (lattice index, axis); tests/tsdf_twin.py restates the rule. One device -> host read-back: the two counts.
    -> Mesh; a volume without a crossing, or with an axis of length 1, gives an empty one."""
    import numpy as np
    L = ops.L
    if not isinstance(volume, TSDFVolume):
        raise ValueError("tsdf_extract: expected a TSDFVolume")
    min_weight = _tsdf_positive("tsdf_extract", "min_weight", min_weight)
    if not volume.tsdf.is_cuda:
        raise L.OvgError("tsdf_extract needs HIP device tensors: there is no CPU fallback")
    dev = volume.tsdf.device
    nx, ny, nz = volume.dims
    ws = torch.empty(ops.tsdf_extract_workspace_bytes(nx, ny, nz), device=dev, dtype=torch.uint8)
    count = torch.empty(2, device=dev, dtype=torch.int64)
    args = dict(tsdf=volume.tsdf, weight=volume.weight, origin=volume.origin, voxel=volume.voxel_size, ws=ws, min_weight=min_weight,
                color=volume.color, out_count=count)
    ops.tsdf_extract(L.TSDF_COUNT, **args)
    M, Q = (int(v) for v in count.cpu().numpy())                            # the one synchronisation
    vertices = torch.empty(M, 3, device=dev, dtype=torch.float32)
    normals = torch.empty(M, 3, device=dev, dtype=torch.float32)
    colors = torch.empty(M, 3, device=dev, dtype=torch.uint8)
    faces = torch.empty(2 * Q, 3, device=dev, dtype=torch.int32)
    if M:
        ops.tsdf_extract(L.TSDF_SCATTER, vertex_capacity=M, quad_capacity=Q, vertices=vertices, normals=normals, colors=colors, faces=faces,
                         **args)
    transform = np.eye(4) if volume.transform is None else np.asarray(volume.transform, dtype=np.float64)
    return Mesh(vertices, faces, normals, colors, transform, volume.extrinsic, volume.scene_scale)


def mesh_to_point_cloud(mesh):
    """A PointCloud of the mesh's vertices and colours (its transform and cameras carried over), for every function that takes a
    cloud: normals, filters, clustering, registration, rendering, the point writers. scene_scale is the mesh's, else ||P95 - P5|| of
    the vertices as predictions_to_point_cloud computes it (1 for an empty mesh)."""
    if not isinstance(mesh, Mesh):
        raise ValueError("mesh_to_point_cloud: expected a Mesh")
    pts = mesh.vertices
    if not pts.is_cuda:
        raise ops.L.OvgError("mesh_to_point_cloud needs HIP device tensors: there is no CPU fallback")
    M = int(pts.shape[0])
    scale = mesh.scene_scale
    if scale is None:
        scale = ops.percentile(pts, M, 3, 1, 3, [5.0, 95.0], norm=True)[1] if M else torch.ones((), device=pts.device, dtype=torch.float32)
    return PointCloud(pts, mesh.colors, torch.zeros((), device=pts.device, dtype=torch.float32), scale, mesh.transform, mesh.extrinsic)


def fuse_predictions(predictions, batch_index=0, voxel_size=None, resolution=256, conf_thres=50.0, keep_mask=None, trunc=None,
                     near=1e-3, max_weight=TSDF_MAX_WEIGHT, min_weight=1.0, min_conf=1e-5, color=True, margin=TSDF_TRUNC_VOXELS,
                     max_voxels=TSDF_MAX_VOXELS):
    """Fuses the S depth maps of the dict OmniVGGT.forward returns into one surface: tsdf_volume_for round the un-projected depth,
    tsdf_integrate of `depth` with the cameras, tsdf_extract. -> (TSDFVolume, Mesh).
    The choices are prediction_consistency's for the depth branch: `depth`, `depth_conf`, the cameras from `extrinsic` / `intrinsic`
    of the dict, else decoded from pose_enc; world_points_from_depth (un-projected here when absent) bounds the volume. A pixel is
    used when its confidence is >= the conf_thres-th percentile of depth_conf (numpy's linear percentile, as
    predictions_to_point_cloud computes it; 0 or a dict without depth_conf skips the percentile) and > min_conf, and, with keep_mask
    (an (S,H,W) bool device tensor, e.g. consistency_mask(...)), where that is True. Colours come from `images`. The mesh carries the
    alignment inv(E0) @ diag(1,-1,-1,1) @ R_y(180) of the first camera, the cameras, and ||P95 - P5|| of its vertices as scene scale.
    ValueError for bad arguments, OvgError for CPU tensors: there is no CPU fallback."""
    what = "fuse_predictions"
    if not isinstance(predictions, dict):
        raise ValueError("predictions must be a dictionary")
    images = predictions["images"]
    if images.dim() == 4:
        images = images.unsqueeze(0)
    B = images.shape[0]
    if not isinstance(batch_index, int) or not 0 <= batch_index < B:
        raise ValueError("batch_index %r out of range for a batch of %d" % (batch_index, B))
    b = batch_index
    S, H, W = images.shape[1], images.shape[-2], images.shape[-1]
    if keep_mask is not None and (not isinstance(keep_mask, torch.Tensor) or keep_mask.dtype != torch.bool or tuple(keep_mask.shape) != (S, H, W)):
        raise ValueError("keep_mask must be a bool tensor (S, H, W) = %r at the map size" % ((S, H, W),))
    if conf_thres is None:
        conf_thres = 10.0
    if isinstance(conf_thres, bool) or not isinstance(conf_thres, (int, float)) or not 0.0 <= conf_thres <= 100.0:
        raise ValueError("%s: conf_thres must be a percentile in [0, 100], got %r" % (what, conf_thres))
    if "depth" not in predictions:
        raise ValueError("%s: predictions carry no `depth`" % what)
    if not images.is_cuda or (keep_mask is not None and not keep_mask.is_cuda):
        raise ops.L.OvgError("fuse_predictions needs HIP device tensors: there is no CPU fallback")
    pts, conf, extrinsic, intrinsic = _prediction_geometry(predictions, "Depthmap and Camera Branch", b, images, want_intrinsic=True)
    depth = predictions["depth"][b].reshape(S, H, W).float().contiguous()
    valid = torch.isfinite(depth) & (depth > float(near))
    if conf is not None:
        cf = conf[b].reshape(-1).float().contiguous()
        ok = cf > float(min_conf)
        if conf_thres != 0.0:
            ok = ok & (cf >= ops.percentile(cf, cf.numel(), 1, 0, 1, [float(conf_thres)]).reshape(()))
        valid = valid & ok.reshape(S, H, W)
    if keep_mask is not None:
        valid = valid & keep_mask
    volume = tsdf_volume_for(pts.reshape(S, H, W, 3).float(), voxel_size=voxel_size, resolution=resolution, margin=margin, valid=valid,
                             trunc=trunc, color=color, max_voxels=max_voxels)
    volume.extrinsic = extrinsic
    volume.transform = scene_alignment(extrinsic[0].detach().double().cpu().numpy())
    tsdf_integrate(volume, depth, extrinsic, intrinsic, images=images[b].reshape(S, 3, H, W) if color else None, valid=valid, near=near,
                   max_weight=max_weight)
    mesh = tsdf_extract(volume, min_weight=min_weight)
    M = int(mesh.vertices.shape[0])
    scale = ops.percentile(mesh.vertices, M, 3, 1, 3, [5.0, 95.0], norm=True)[1] if M else torch.ones((), device=depth.device, dtype=torch.float32)
    volume.scene_scale = mesh.scene_scale = scale
    return volume, mesh


def _host_mesh(mesh, apply_transform):
    """Host arrays of a mesh: vertices f32, normals f32, colours u8, faces int32; under apply_transform the vertices are mapped by
    mesh.transform in float64 and the normals by the inverse transpose of its linear part, renormalised (write_ply's rule)."""
    import numpy as np
    if not isinstance(mesh, Mesh):
        raise ValueError("expected a Mesh")
    pts = mesh.vertices.detach().cpu().numpy().astype(np.float32).reshape(-1, 3)
    nrm = mesh.normals.detach().cpu().numpy().astype(np.float32).reshape(-1, 3)
    col = mesh.colors.detach().cpu().numpy().astype(np.uint8).reshape(-1, 3)
    faces = mesh.faces.detach().cpu().numpy().astype(np.int32).reshape(-1, 3)
    if apply_transform and len(pts):
        T = np.asarray(mesh.transform, dtype=np.float64)
        pts = (pts.astype(np.float64) @ T[:3, :3].T + T[:3, 3]).astype(np.float32)
        n64 = nrm.astype(np.float64) @ np.linalg.inv(T[:3, :3])
        length = np.sqrt((n64 * n64).sum(1, keepdims=True))
        nrm = np.where(length > 0, n64 / np.where(length > 0, length, 1.0), 0.0).astype(np.float32)
    return pts, nrm, col, faces


def write_mesh_ply(path, mesh, apply_transform=True):
    """Binary little-endian PLY of the mesh: `x y z nx ny nz` float and `red green blue` uchar per vertex, then one
    `list uchar int vertex_indices` of three per face. apply_transform as in write_ply: vertices by mesh.transform in float64, normals
    by the inverse transpose of its linear part. An empty mesh writes a valid file with no vertices and no faces."""
    import numpy as np
    pts, nrm, col, faces = _host_mesh(mesh, apply_transform)
    if apply_transform and len(faces) and np.linalg.det(np.asarray(mesh.transform, dtype=np.float64)[:3, :3]) < 0:
        faces = faces[:, ::-1]                                              # a mirroring transform turns the winding round
    rec = np.empty(len(pts), dtype=[("x", "<f4"), ("y", "<f4"), ("z", "<f4"), ("nx", "<f4"), ("ny", "<f4"), ("nz", "<f4"),
                                    ("red", "u1"), ("green", "u1"), ("blue", "u1")])
    for k, name in enumerate(("x", "y", "z")):
        rec[name], rec["n" + name] = pts[:, k], nrm[:, k]
    rec["red"], rec["green"], rec["blue"] = col[:, 0], col[:, 1], col[:, 2]
    frec = np.empty(len(faces), dtype=[("n", "u1"), ("v", "<i4", (3,))])
    frec["n"], frec["v"] = 3, faces
    header = ("ply\nformat binary_little_endian 1.0\nelement vertex %d\nproperty float x\nproperty float y\nproperty float z\n"
              "property float nx\nproperty float ny\nproperty float nz\nproperty uchar red\nproperty uchar green\nproperty uchar blue\n"
              "element face %d\nproperty list uchar int vertex_indices\nend_header\n" % (len(pts), len(faces)))
    with open(path, "wb") as fh:
        fh.write(header.encode("ascii"))
        fh.write(rec.tobytes())
        fh.write(frec.tobytes())


def write_mesh_glb(path, mesh, cameras=False, camera_scale=0.05):
    """glTF 2.0 binary of the mesh: one indexed TRIANGLES primitive with POSITION (f32 VEC3 with min / max), NORMAL (f32 VEC3),
    COLOR_0 (normalized u8 VEC4, alpha 255) and u32 indices, under one node whose `matrix` is mesh.transform (column-major), as
    write_glb places its cloud: the vertices stay untransformed. An empty mesh writes a node without a mesh. cameras=True adds
    write_glb's pyramids for mesh.extrinsic, of height camera_scale * mesh.scene_scale, to the same mesh under the same node."""
    import numpy as np
    pts, nrm, col, faces = _host_mesh(mesh, False)
    M = len(pts)
    node = {"matrix": [float(v) for v in np.asarray(mesh.transform, dtype=np.float64).T.reshape(-1)]}
    gltf = {"asset": {"version": "2.0", "generator": "omnivggt_official_amd.postprocess"}, "scene": 0, "scenes": [{"nodes": [0]}],
            "nodes": [node]}
    binary = b""
    if M and len(faces):
        rgba = np.concatenate([col, np.full((M, 1), 255, np.uint8)], axis=1)
        parts = [pts.astype("<f4").tobytes(), nrm.astype("<f4").tobytes(), rgba.tobytes(), faces.astype("<u4").tobytes()]
        views, off = [], 0
        for part, target in zip(parts, (34962, 34962, 34962, 34963)):
            views.append({"buffer": 0, "byteOffset": off, "byteLength": len(part), "target": target})
            off += len(part)                                                # every part is a multiple of 4 bytes long
        binary = b"".join(parts)
        node["mesh"] = 0
        gltf["meshes"] = [{"primitives": [{"attributes": {"POSITION": 0, "NORMAL": 1, "COLOR_0": 2}, "indices": 3, "mode": 4}]}]
        gltf["buffers"] = [{"byteLength": len(binary)}]
        gltf["bufferViews"] = views
        gltf["accessors"] = [{"bufferView": 0, "componentType": 5126, "count": M, "type": "VEC3",
                              "min": [float(v) for v in pts.min(axis=0)], "max": [float(v) for v in pts.max(axis=0)]},
                             {"bufferView": 1, "componentType": 5126, "count": M, "type": "VEC3"},
                             {"bufferView": 2, "componentType": 5121, "normalized": True, "count": M, "type": "VEC4"},
                             {"bufferView": 3, "componentType": 5125, "count": 3 * len(faces), "type": "SCALAR"}]
    if cameras:
        if mesh.extrinsic is None or mesh.scene_scale is None:
            raise ValueError("write_mesh_glb: cameras=True needs a mesh with extrinsic and scene_scale")
        binary = _glb_add_cameras(gltf, node, binary, mesh.extrinsic, float(camera_scale) * float(mesh.scene_scale))
    _glb_write(path, gltf, binary)


# ---------------------------------------------------------------------------------------------------------------------------------
# Image-space map geometry: normals, edge masks and per-view meshes straight from the (S, H, W) maps (ovg_map_depth,
# ovg_map_normals, ovg_map_edges, ovg_map_triangulate)
# ---------------------------------------------------------------------------------------------------------------------------------

class MapEdges:
    """Result of map_edges: flags (S,H,W) u8 with the bits ops.L.MAP_UNUSABLE / MAP_DEPTH_EDGE / MAP_NORMAL_EDGE / MAP_NO_NORMAL, and
    the (S,H,W) bool views of it depth_edge, normal_edge and usable. Device tensors."""
    __slots__ = ("flags", "depth_edge", "normal_edge", "usable")

    def __init__(self, flags):
        L = ops.L
        self.flags = flags
        self.depth_edge, self.normal_edge = (flags & L.MAP_DEPTH_EDGE) != 0, (flags & L.MAP_NORMAL_EDGE) != 0
        self.usable = (flags & L.MAP_UNUSABLE) == 0


class MapMesh(Mesh):
    """A Mesh from triangulate_maps / predictions_to_mesh: additionally pixel_index (M,) int64, the flat index of every vertex into the
    S x H x W maps it was built from, and conf_threshold (0-d f32 device tensor: predictions_to_mesh's percentile; else None)."""
    __slots__ = ("pixel_index", "conf_threshold")

    def __init__(self, vertices, faces, normals, colors, transform, extrinsic=None, scene_scale=None, pixel_index=None, conf_threshold=None):
        Mesh.__init__(self, vertices, faces, normals, colors, transform, extrinsic, scene_scale)
        self.pixel_index, self.conf_threshold = pixel_index, conf_threshold


def _map_f32(what, name, value, positive=False, allow_inf=False):
    """A host number as the float32 value the kernels see; None with allow_inf is +inf (the test switched off)."""
    import math
    import numpy as np
    if value is None and allow_inf:
        return float("inf")
    try:
        with np.errstate(over="ignore"):
            v = float(np.float32(value))
    except (TypeError, ValueError):
        v = float("nan")
    ok = not isinstance(value, bool) and (v > 0.0 if positive else v >= 0.0) and (allow_inf or math.isfinite(v))
    if not ok:
        raise ValueError("%s: %s must be %s in float32, got %r" % (what, name, "positive and finite" if positive else
                                                                    "non-negative" + ("" if allow_inf else " and finite"), value))
    return v


def _map_points(what, points):
    if not isinstance(points, torch.Tensor) or points.dim() != 4 or points.shape[3] != 3 or 0 in points.shape or not points.is_floating_point():
        raise ValueError("%s: points must be a (S, H, W, 3) float tensor" % what)
    S, H, W = (int(v) for v in points.shape[:3])
    if S * H * W >= 1 << 31:
        raise ValueError("%s: S = %d views of %d x %d exceed S * H * W < 2^31" % (what, S, H, W))
    return S, H, W


def _map_like(what, t, name, shape, dtypes):
    if t is None:
        return
    if not isinstance(t, torch.Tensor) or tuple(t.shape) != tuple(shape) or not (t.dtype in dtypes if dtypes else t.is_floating_point()):
        raise ValueError("%s: %s must be a %s tensor %r" % (what, name, "bool / uint8" if dtypes else "float", tuple(shape)))


def _map_u8(t):
    return None if t is None else (t.to(torch.uint8) if t.dtype == torch.bool else t).contiguous()


def _map_need_device(what, *ts):
    for t in ts:
        if t is not None and not t.is_cuda:
            raise ops.L.OvgError("%s needs HIP device tensors: there is no CPU fallback" % what)


def camera_depth_maps(points=None, extrinsic=None, depth=None, valid=None, near=1e-3):
    """The usable-depth map z (S,H,W) f32 that map_normals, map_edges and triangulate_maps read (ovg_map_depth): a pixel's camera
    depth where it is usable -- valid (if given), finite and > near -- and NaN elsewhere. Exactly one of two inputs: points
    (S,H,W,3), world points in the frame of extrinsic (S,3,4) world-to-camera (device tensor, numpy array or list, rounded to f32),
    whose depth is the third row of the camera transform; or depth (S,H,W) / (S,H,W,1), taken as it is. valid: optional (S,H,W)
    bool / u8. No device -> host synchronisation; CPU tensors raise OvgError, bad shapes or near ValueError."""
    what = "camera_depth_maps"
    if (points is None) == (depth is None):
        raise ValueError("%s: exactly one of points / depth" % what)
    near32 = _map_f32(what, "near", near, positive=True)
    if points is not None:
        S, H, W = _map_points(what, points)
        if extrinsic is None:
            raise ValueError("%s: points need the extrinsic (S, 3, 4) of their views" % what)
        ext = torch.as_tensor(extrinsic).detach()
        if tuple(ext.shape) != (S, 3, 4):
            raise ValueError("%s: extrinsic must be (S, 3, 4) = (%d, 3, 4), got %r" % (what, S, tuple(ext.shape)))
        _map_like(what, valid, "valid", (S, H, W), (torch.bool, torch.uint8))
        _map_need_device(what, points, valid)
        cams = _pack_cams(ext, torch.eye(3), S, points.device)              # the intrinsics are not read
        return ops.map_depth(points=points.float().contiguous(), cams=cams, valid=_map_u8(valid), near=near32)
    if isinstance(depth, torch.Tensor) and depth.dim() == 4 and depth.shape[-1] == 1:
        depth = depth[..., 0]
    if not isinstance(depth, torch.Tensor) or depth.dim() != 3 or 0 in depth.shape or not depth.is_floating_point() or depth.numel() >= 1 << 31:
        raise ValueError("%s: depth must be a (S, H, W) or (S, H, W, 1) float tensor, S * H * W < 2^31" % what)
    _map_like(what, valid, "valid", tuple(depth.shape), (torch.bool, torch.uint8))
    _map_need_device(what, depth, valid)
    return ops.map_depth(depth=depth.float().contiguous(), valid=_map_u8(valid), near=near32)


def map_normals(points, z, rel_tol=0.03):
    """Normals (S,H,W,3) f32 of a point map from its own pixel grid (ovg_map_normals): the normalised cross product of the vertical
    and the horizontal finite difference, central where both neighbours are usable, one-sided at the frame, next to unusable pixels
    and across depth steps (a neighbour counts when |z_q - z_p| <= rel_tol * z_p; rel_tol None switches that off). They point back
    towards the camera -- the outside of the surface, as Mesh normals do -- without needing the camera; pixels without both
    differences carry (0, 0, 0). points (S,H,W,3), z = camera_depth_maps(...). The rule is exact (tests/mapgeom_twin.py restates it);
    no search, no eigen-solve, no synchronisation. write_ply(normals=...) takes normals[flat indices of the cloud]."""
    what = "map_normals"
    S, H, W = _map_points(what, points)
    _map_like(what, z, "z", (S, H, W), None)
    tol32 = _map_f32(what, "rel_tol", rel_tol, allow_inf=True)
    _map_need_device(what, points, z)
    return ops.map_normals(points.float().contiguous(), z.float().contiguous(), rel_tol=tol32)


def map_edges(z, normals=None, radius=1, rel_tol=0.03, max_angle_deg=None):
    """Edge flags of the maps over a (2 radius + 1)^2 pixel window, radius 1, 2 or 3 (ovg_map_edges): a usable pixel is a DEPTH
    EDGE when the usable depths of its window spread by more than rel_tol * its own depth -- the relative depth-edge test that removes
    the flying pixels of a depth head at discontinuities, per view, without a search -- and, with normals (map_normals') and
    max_angle_deg, a NORMAL EDGE when a window pixel's normal makes a larger angle with its own (cos < cos(max_angle_deg), the
    float64 cosine rounded once to f32); pixels without a normal are flagged NO_NORMAL instead. z = camera_depth_maps(...).
    -> MapEdges(flags, depth_edge, normal_edge, usable); edge_mask(result) is the keep mask. No synchronisation."""
    import math
    import numpy as np
    what = "map_edges"
    if not isinstance(z, torch.Tensor) or z.dim() != 3 or 0 in z.shape or not z.is_floating_point() or z.numel() >= 1 << 31:
        raise ValueError("%s: z must be a (S, H, W) float tensor, S * H * W < 2^31" % what)
    _map_like(what, normals, "normals", tuple(z.shape) + (3,), None)
    if isinstance(radius, bool) or not isinstance(radius, (int, np.integer)) or not 1 <= radius <= ops.L.MAP_MAX_RADIUS:
        raise ValueError("%s: radius must be 1, 2 or 3, got %r" % (what, radius))
    tol32 = _map_f32(what, "rel_tol", rel_tol, allow_inf=True)
    min_cos = float("-inf")
    if max_angle_deg is not None:
        if isinstance(max_angle_deg, bool) or not isinstance(max_angle_deg, (int, float)) or not 0.0 <= max_angle_deg <= 180.0:
            raise ValueError("%s: max_angle_deg must be an angle in [0, 180], got %r" % (what, max_angle_deg))
        if normals is None:
            raise ValueError("%s: max_angle_deg needs normals" % what)
        min_cos = float(np.float32(math.cos(math.radians(float(max_angle_deg)))))
    _map_need_device(what, z, normals)
    flags = ops.map_edges(z.float().contiguous(), None if normals is None else normals.float().contiguous(), radius=int(radius),
                          rel_tol=tol32, min_cos=min_cos)
    return MapEdges(flags)


def edge_mask(result, depth=True, normal=False):
    """(S,H,W) bool keep mask of a MapEdges: usable pixels that are no depth edge (depth=True) and no normal edge (normal=True);
    pixels flagged NO_NORMAL stay. It is the keep_mask of predictions_to_point_cloud / fuse_predictions / predictions_to_mesh and the
    valid of multiview_consistency / tsdf_integrate."""
    if not isinstance(result, MapEdges):
        raise ValueError("edge_mask: expected a MapEdges")
    keep = result.usable
    if depth:
        keep = keep & ~result.depth_edge
    if normal:
        keep = keep & ~result.normal_edge
    return keep


def _prediction_maps(what, predictions, prediction_mode, batch_index, near, valid):
    """-> (points (S,H,W,3) f32, z, confidence WITH its batch dimension or None, extrinsic, images with the batch dimension)."""
    if not isinstance(predictions, dict):
        raise ValueError("predictions must be a dictionary")
    images = predictions["images"]
    if images.dim() == 4:
        images = images.unsqueeze(0)
    B = images.shape[0]
    if not isinstance(batch_index, int) or not 0 <= batch_index < B:
        raise ValueError("batch_index %r out of range for a batch of %d" % (batch_index, B))
    if not images.is_cuda:
        raise ops.L.OvgError("%s needs HIP device tensors: there is no CPU fallback" % what)
    S, H, W = images.shape[1], images.shape[-2], images.shape[-1]
    pts, conf, extrinsic, _ = _prediction_geometry(predictions, prediction_mode, batch_index, images)
    pts = pts.reshape(S, H, W, 3).float().contiguous()
    z = camera_depth_maps(points=pts, extrinsic=extrinsic, valid=valid, near=near)
    return pts, z, conf, extrinsic, images


def prediction_normals(predictions, prediction_mode="Predicted Pointmap", batch_index=0, rel_tol=0.03, near=1e-3, valid=None):
    """map_normals of the dict OmniVGGT.forward returns: the points by the choices predictions_to_point_cloud makes for
    `prediction_mode`, their depth in the dict's cameras (`extrinsic`, else decoded from pose_enc). -> (normals (S,H,W,3), z (S,H,W))."""
    pts, z, _, _, _ = _prediction_maps("prediction_normals", predictions, prediction_mode, batch_index, near, valid)
    return map_normals(pts, z, rel_tol=rel_tol), z


def prediction_edges(predictions, prediction_mode="Predicted Pointmap", batch_index=0, radius=1, rel_tol=0.03, max_angle_deg=None,
                     near=1e-3, valid=None):
    """map_edges of the dict OmniVGGT.forward returns, on the same maps as prediction_normals (the normals are computed only for
    max_angle_deg). -> MapEdges; edge_mask(result) is the keep_mask of predictions_to_point_cloud."""
    pts, z, _, _, _ = _prediction_maps("prediction_edges", predictions, prediction_mode, batch_index, near, valid)
    normals = None if max_angle_deg is None else map_normals(pts, z, rel_tol=rel_tol)
    return map_edges(z, normals, radius=radius, rel_tol=rel_tol, max_angle_deg=max_angle_deg)


def _triangulate(what, pts, z, keep, colors, normals, tol32, extrinsic, conf_threshold=None):
    """COUNT, the one read-back (the two counts with the first camera), SCATTER. -> MapMesh."""
    import numpy as np
    L = ops.L
    S, H, W = (int(v) for v in z.shape)
    dev = z.device
    ws = torch.empty(ops.map_triangulate_workspace_bytes(S, H, W), device=dev, dtype=torch.uint8)
    count = torch.empty(2, device=dev, dtype=torch.int64)
    args = dict(z=z, points=pts, ws=ws, rel_tol=tol32, keep=keep, normals=normals, colors=colors, out_count=count)
    ops.map_triangulate(L.MAP_COUNT, **args)
    # the one synchronisation: both counts and the first camera in one copy (int64 counts are exact in float64 below 2^53)
    first = extrinsic[0].reshape(-1).to(device=dev, dtype=torch.float64) if extrinsic is not None else torch.zeros(0, device=dev, dtype=torch.float64)
    host = torch.cat([count.double(), first]).cpu().numpy()
    M, F = int(host[0]), int(host[1])
    transform = scene_alignment(host[2:14].reshape(3, 4)) if extrinsic is not None else np.eye(4)
    vertices = torch.empty(M, 3, device=dev, dtype=torch.float32)
    out_normals = torch.empty(M, 3, device=dev, dtype=torch.float32)
    out_colors = torch.empty(M, 3, device=dev, dtype=torch.uint8)
    index = torch.empty(M, device=dev, dtype=torch.int64)
    faces = torch.empty(F, 3, device=dev, dtype=torch.int32)
    if M:
        ops.map_triangulate(L.MAP_SCATTER, vertex_capacity=M, face_capacity=F, vertices=vertices, out_normals=out_normals, out_colors=out_colors,
                            pixel_index=index, faces=faces, **args)
        scale = ops.percentile(vertices, M, 3, 1, 3, [5.0, 95.0], norm=True)[1]
    else:
        scale = torch.ones((), device=dev, dtype=torch.float32)
    return MapMesh(vertices, faces, out_normals, out_colors, transform, extrinsic, scale, index, conf_threshold)


def triangulate_maps(points, z, keep=None, images=None, normals=None, rel_tol=0.03, extrinsic=None):
    """The grid mesh of S point maps on the device (ovg_map_triangulate), what the reference's viz.pts3d_to_trimesh builds: two
    triangles per 2 x 2 pixel quad, (a, c, b) and (b, c, d) with the diagonal b-c, wound so that they face the camera. A face is
    emitted when its three pixels are usable in z (camera_depth_maps), finite and kept, and it is not torn: the spread of its three
    depths is at most rel_tol times the smallest (None switches that off). Vertices are the pixels a face names, in pixel order, at
    native resolution; faces in ascending (view, y, x). Deterministic and exact (tests/mapgeom_twin.py restates the rule).

    points (S,H,W,3), z (S,H,W) device tensors; keep: optional (S,H,W) bool / u8 (edge_mask(...), a confidence test, ...); images:
    (S,3,H,W) floats in [0, 1] or (S,H,W,3) u8 vertex colours (128 grey without); normals: optional (S,H,W,3) (map_normals') copied to
    the vertices ((0, 0, 0) without). extrinsic (S,3,4): the views' cameras, for the alignment inv(E0) @ diag(1,-1,-1,1) @ R_y(180)
    of the first one that the writers apply and for write_mesh_glb(cameras=True); without it the transform is the identity.
    -> MapMesh (a Mesh with pixel_index), scene_scale = ||P95 - P5|| of its vertices: write_mesh_ply, write_mesh_glb, render_mesh and
    mesh_to_point_cloud take it as it is. Exactly one device -> host synchronisation: the two counts, read with the first camera.
    CPU tensors raise OvgError (there is no CPU fallback), bad shapes and values ValueError."""
    what = "triangulate_maps"
    S, H, W = _map_points(what, points)
    _map_like(what, z, "z", (S, H, W), None)
    _map_like(what, keep, "keep", (S, H, W), (torch.bool, torch.uint8))
    _map_like(what, normals, "normals", (S, H, W, 3), None)
    tol32 = _map_f32(what, "rel_tol", rel_tol, allow_inf=True)
    colors = None
    if images is not None:
        try:
            colors = _tsdf_colors(images, S, H, W)
        except ValueError:
            raise ValueError("%s: images must be (S, 3, H, W) = (%d, 3, %d, %d) floats in [0, 1] or (S, H, W, 3) uint8" % (what, S, H, W)) from None
    ext = None
    if extrinsic is not None:
        ext = torch.as_tensor(extrinsic).detach()
        if tuple(ext.shape) != (S, 3, 4):
            raise ValueError("%s: extrinsic must be (S, 3, 4) = (%d, 3, 4), got %r" % (what, S, tuple(ext.shape)))
    _map_need_device(what, points, z, keep, normals, colors)
    return _triangulate(what, points.float().contiguous(), z.float().contiguous(), _map_u8(keep), colors,
                        None if normals is None else normals.float().contiguous(), tol32, ext)


def predictions_to_mesh(predictions, conf_thres=50.0, filter_by_frames="all", prediction_mode="Predicted Pointmap", keep_mask=None,
                        rel_tol=0.03, edge_radius=1, with_normals=True, batch_index=0, min_conf=1e-5, near=1e-3):
    """The per-view grid mesh of the dict OmniVGGT.forward returns, at native resolution: the quick look at a prediction that needs no
    volume (fuse_predictions is the fused surface). The maps, the frame filter, the confidence rule and the alignment are
    predictions_to_point_cloud's: points and confidence by `prediction_mode`, filter_by_frames "k: ..." keeps frame k, the threshold
    is numpy's linear percentile of the selected frames' confidences (conf_thres None means 10, 0 skips it), a pixel is kept when
    conf >= threshold and conf > min_conf, and, with keep_mask ((S,H,W) bool device tensor), where that is True. On top of that the
    depth edges of map_edges(radius=edge_radius, rel_tol) are dropped (edge_radius 0 skips the test) -- the flying pixels between
    a foreground and its background -- and triangulate_maps(rel_tol) drops torn faces. Colours come from `images`; with_normals fills
    the vertex normals with map_normals(rel_tol), else they are (0, 0, 0) and render_mesh shades by face.
    -> MapMesh with transform = inv(E0) @ diag(1,-1,-1,1) @ R_y(180) of the first selected camera, extrinsic, scene_scale, pixel_index
    (flat indices into the selected frames' maps) and conf_threshold, so write_mesh_ply, write_mesh_glb(cameras=True), render_mesh
    and mesh_to_point_cloud work on it unchanged. Exactly one device -> host synchronisation (the counts, read with the first
    camera). CPU tensors raise OvgError: there is no CPU fallback."""
    import numpy as np
    what = "predictions_to_mesh"
    if conf_thres is None:
        conf_thres = 10.0
    if isinstance(conf_thres, bool) or not isinstance(conf_thres, (int, float)) or not 0.0 <= conf_thres <= 100.0:
        raise ValueError("%s: conf_thres must be a percentile in [0, 100], got %r" % (what, conf_thres))
    if isinstance(edge_radius, bool) or not isinstance(edge_radius, (int, np.integer)) or not 0 <= edge_radius <= ops.L.MAP_MAX_RADIUS:
        raise ValueError("%s: edge_radius must be 0 (no edge test), 1, 2 or 3, got %r" % (what, edge_radius))
    tol32 = _map_f32(what, "rel_tol", rel_tol, allow_inf=True)
    if isinstance(predictions, dict) and keep_mask is not None:
        im = predictions["images"]
        shape = (im.shape[-4], im.shape[-2], im.shape[-1])
        if not isinstance(keep_mask, torch.Tensor) or keep_mask.dtype != torch.bool or tuple(keep_mask.shape) != shape:
            raise ValueError("keep_mask must be a bool tensor (S, H, W) = %r at the map size" % (shape,))
        _map_need_device(what, keep_mask)
    pts, z, conf, extrinsic, images = _prediction_maps(what, predictions, prediction_mode, batch_index, near, None)
    b = batch_index
    S, H, W = (int(v) for v in z.shape)
    conf = torch.ones(S, H, W, device=z.device, dtype=torch.float32) if conf is None else conf[b].reshape(S, H, W).float().contiguous()
    img = images[b].reshape(S, 3, H, W)
    _map_need_device(what, conf, extrinsic)
    frame = _parse_frame(filter_by_frames)
    if frame is not None:
        if not -S <= frame < S:
            raise ValueError("filter_by_frames selects frame %d of %d" % (frame, S))
        frame %= S
        sl = slice(frame, frame + 1)
        pts, z, conf, img, extrinsic = pts[sl].contiguous(), z[sl].contiguous(), conf[sl].contiguous(), img[sl], extrinsic[sl]
        keep_mask = None if keep_mask is None else keep_mask[sl]
        S = 1
    cf = conf.reshape(-1)
    keep = cf > float(min_conf)
    if conf_thres == 0.0:
        conf_threshold = torch.zeros((), device=z.device, dtype=torch.float32)
    else:
        conf_threshold = ops.percentile(cf, cf.numel(), 1, 0, 1, [float(conf_thres)]).reshape(())
        keep = keep & (cf >= conf_threshold)
    keep = keep.reshape(S, H, W)
    if keep_mask is not None:
        keep = keep & keep_mask
    if edge_radius:
        flags = ops.map_edges(z, radius=int(edge_radius), rel_tol=tol32)
        keep = keep & ((flags & ops.L.MAP_DEPTH_EDGE) == 0)
    normals = ops.map_normals(pts, z, rel_tol=tol32) if with_normals else None
    return _triangulate(what, pts, z, keep.to(torch.uint8), _tsdf_colors(img.float(), S, H, W), normals, tol32, extrinsic, conf_threshold)


# ---------------------------------------------------------------------------------------------------------------------------------
# Mesh simplification: vertex clustering on the grid of voxel_downsample, duplicate faces merged (ovg_mesh_simplify)
# ---------------------------------------------------------------------------------------------------------------------------------

class SimplifiedMesh(Mesh):
    """A Mesh from simplify_mesh: additionally source_index (M',) int64, the input index of every output vertex's leader (the lowest
    valid vertex of its cell); vertex_count (M',) int32, the valid input vertices of that cell; pixel_index (M',) int64 =
    mesh.pixel_index[source_index] when the input was a MapMesh, else None; and the host integers cells (occupied cells),
    degenerate_faces and duplicate_faces (faces dropped by either rule)."""
    __slots__ = ("source_index", "vertex_count", "pixel_index", "cells", "degenerate_faces", "duplicate_faces")

    def __init__(self, vertices, faces, normals, colors, transform, extrinsic=None, scene_scale=None, source_index=None, vertex_count=None,
                 pixel_index=None, cells=0, degenerate_faces=0, duplicate_faces=0):
        Mesh.__init__(self, vertices, faces, normals, colors, transform, extrinsic, scene_scale)
        self.source_index, self.vertex_count, self.pixel_index = source_index, vertex_count, pixel_index
        self.cells, self.degenerate_faces, self.duplicate_faces = cells, degenerate_faces, duplicate_faces


MESH_POSITIONS = {"mean": 0, "first": 1}


def simplify_mesh(mesh, voxel_size=None, rel_size=None, position="mean"):
    """Vertex clustering of a Mesh on the device (ovg_mesh_simplify): the vertices that share a cell of a regular grid become one, the
    faces that collapse disappear. The first reducer to reach for when a mesh is too large to write or view; linear and order-free.

    Exactly one of voxel_size (the cell edge in the mesh's units: a positive float or a 0-d f32 device tensor) and rel_size (a positive
    float; the edge is f32(rel_size) * mesh.scene_scale, one f32 multiply on the device) must be given, as for voxel_downsample, whose
    grid this is: vertices with a non-finite coordinate are dropped, the grid starts at the component-wise minimum of the others, cell
    = floor((p - origin) / edge) in f32. The rule is exact (tests/meshsimp_twin.py restates it): a face with an index outside the
    mesh or an invalid vertex is dropped; a face whose three cells are not pairwise different is dropped as degenerate; of the faces
    with the same unordered set of three cells the lowest input index survives with its own winding (a back-to-back copy goes too:
    render_mesh draws both sides by default). One output vertex per cell a surviving face names, in the order of the cells' lowest
    vertex index; faces in input order. position "mean": the order-free integer mean of the cell's vertices; "first": the lowest
    vertex of the cell as it is. Colours are the channel means rounded half up, normals the normalised integer sum of the cell's
    usable normals ((0, 0, 0) when they cancel); a mesh without normals / colours gives a mesh without. Two calls give identical bytes.

    -> SimplifiedMesh: transform, extrinsic and scene_scale passed through unchanged, so write_mesh_ply, write_mesh_glb, render_mesh
    and mesh_to_point_cloud take it as it is; source_index, vertex_count, pixel_index (for a MapMesh) and the three host counts.
    Not in it: quadric placement, edge collapse, smoothing, a guarantee of manifoldness (clustering can pinch a surface).

    Exactly one device -> host synchronisation (the six counts in one copy). A grid of more than 2^21 cells along an axis, or an edge
    that is not positive on the device, raises ValueError, as does rel_size on a mesh without scene_scale. A mesh without vertices or
    without faces returns an empty mesh without a launch. CPU tensors raise OvgError: there is no CPU fallback."""
    import math
    L = ops.L
    what = "simplify_mesh"
    if not isinstance(mesh, Mesh):
        raise ValueError("%s: expected a Mesh" % what)
    if (voxel_size is None) == (rel_size is None):
        raise ValueError("%s: give exactly one of voxel_size and rel_size" % what)
    if not isinstance(position, str) or position not in MESH_POSITIONS:
        raise ValueError("%s: position must be one of %r, got %r" % (what, sorted(MESH_POSITIONS), position))
    given = voxel_size if rel_size is None else rel_size
    if isinstance(given, torch.Tensor):
        if rel_size is not None or given.numel() != 1:
            raise ValueError("%s: rel_size must be a float, voxel_size a float or a one-element tensor" % what)
    else:
        given = float(given)
        if not (given > 0.0 and math.isfinite(given)):
            raise ValueError("%s: the size must be positive and finite, got %r" % (what, given))
    if rel_size is not None and mesh.scene_scale is None:
        raise ValueError("%s: rel_size needs a mesh with scene_scale" % what)
    vert, faces, nrm, col = mesh.vertices, mesh.faces, mesh.normals, mesh.colors
    if vert is None or faces is None:
        raise ValueError("%s: the mesh has no vertices or no faces tensor" % what)
    pix = getattr(mesh, "pixel_index", None)
    for t in (vert, faces, nrm, col, pix, given if isinstance(given, torch.Tensor) else None):
        if t is not None and not (isinstance(t, torch.Tensor) and t.is_cuda):
            raise L.OvgError("%s needs HIP device tensors: there is no CPU fallback" % what)
    M, F = int(vert.shape[0]), int(faces.shape[0])
    if M >= 1 << 31 or F >= (1 << 32) - 1:
        raise ValueError("%s: the mesh has 2^31 vertices or 2^32 - 1 faces or more" % what)
    dev = vert.device

    def result(v, f, n, c, src, cnt, cells=0, degenerate=0, duplicates=0):
        return SimplifiedMesh(v, f, n, c, mesh.transform, mesh.extrinsic, mesh.scene_scale, src, cnt, None if pix is None else pix[src],
                              cells, degenerate, duplicates)

    def empty(cells=0, degenerate=0, duplicates=0):
        return result(torch.empty(0, 3, device=dev, dtype=torch.float32), torch.empty(0, 3, device=dev, dtype=torch.int32),
                      None if nrm is None else torch.empty(0, 3, device=dev, dtype=torch.float32),
                      None if col is None else torch.empty(0, 3, device=dev, dtype=torch.uint8), torch.empty(0, device=dev, dtype=torch.int64),
                      torch.empty(0, device=dev, dtype=torch.int32), cells, degenerate, duplicates)
    if M == 0 or F == 0:
        return empty()
    vert = vert.reshape(M, 3).float().contiguous()
    faces = faces.reshape(F, 3).to(torch.int32).contiguous()
    nrm = None if nrm is None else nrm.reshape(M, 3).float().contiguous()
    col = None if col is None else col.reshape(M, 3).to(torch.uint8).contiguous()
    if isinstance(given, torch.Tensor):
        voxel = given.detach().to(torch.float32).reshape(())
    else:
        voxel = torch.full((), given, device=dev, dtype=torch.float32)
        if rel_size is not None:
            voxel = voxel * mesh.scene_scale.to(device=dev, dtype=torch.float32).reshape(())
    ws = torch.empty(ops.mesh_simplify_workspace_bytes(M, F), device=dev, dtype=torch.uint8)
    count = torch.empty(6, device=dev, dtype=torch.int64)
    args = dict(vertices=vert, faces=faces, voxel=voxel, ws=ws, normals=nrm, colors=col, position=MESH_POSITIONS[position], out_count=count)
    ops.mesh_simplify(L.MS_COUNT, **args)
    Mo, Fo, flags, cells, degenerate, duplicates = (int(v) for v in count.cpu().tolist())       # the one synchronisation
    if flags:
        ok = torch.isfinite(vert).all(dim=1)
        extent = (vert[ok].max(dim=0).values - vert[ok].min(dim=0).values).tolist() if bool(ok.any()) else []
        why = "is not a positive finite number" if flags & L.MS_BAD_VOXEL else "gives more than 2^21 cells along an axis"
        raise ValueError("%s: voxel size %r %s (extent of the mesh %r)" % (what, float(voxel), why, extent))
    if Mo == 0:
        return empty(cells, degenerate, duplicates)
    out_v = torch.empty(Mo, 3, device=dev, dtype=torch.float32)
    out_n = None if nrm is None else torch.empty(Mo, 3, device=dev, dtype=torch.float32)
    out_c = None if col is None else torch.empty(Mo, 3, device=dev, dtype=torch.uint8)
    src = torch.empty(Mo, device=dev, dtype=torch.int64)
    cnt = torch.empty(Mo, device=dev, dtype=torch.int32)
    out_f = torch.empty(Fo, 3, device=dev, dtype=torch.int32)
    ops.mesh_simplify(L.MS_SCATTER, vertex_capacity=Mo, face_capacity=Fo, out_vertices=out_v, out_normals=out_n, out_colors=out_c,
                      source_index=src, vertex_count=cnt, out_faces=out_f, **args)
    return result(out_v, out_f, out_n, out_c, src, cnt, cells, degenerate, duplicates)


# ---------------------------------------------------------------------------------------------------------------------------------
# Mesh cleaning: connected components, small-piece removal and Laplacian / Taubin smoothing (ovg_mesh_topology / _select / _smooth)
# ---------------------------------------------------------------------------------------------------------------------------------
# Not in any of it: hole filling, edge-adjacency components, pinch-vertex detection, cotangent or area weights, quadric simplification,
# any guarantee that smoothing keeps a mesh free of self-intersections.

MT_REFERENCED, MT_BOUNDARY, MT_NONMANIFOLD = ops.L.MT_REFERENCED, ops.L.MT_BOUNDARY, ops.L.MT_NONMANIFOLD


class MeshTopology:
    """Result of mesh_topology. Device tensors: vertex_root int32 (M,) (the lowest vertex index of the vertex's component, -1 for a
    vertex no live face names), face_root int32 (F,) (-1 for a face that is not live), vertex_flags uint8 (M,) (MT_REFERENCED |
    MT_BOUNDARY | MT_NONMANIFOLD), vertex_labels / face_labels int32 (the dense component number, -1 where the root is -1); per
    component, in label order: roots int32 (C,), face_sizes and vertex_sizes int64 (C,). Host integers: num_components, live_faces,
    referenced_vertices, edges, boundary_edges, nonmanifold_edges, boundary_vertices, nonmanifold_vertices, euler (= referenced_vertices
    - edges + live_faces); closed: there is a live face and no boundary edge."""
    __slots__ = ("vertex_root", "face_root", "vertex_flags", "vertex_labels", "face_labels", "roots", "face_sizes", "vertex_sizes",
                 "num_components", "live_faces", "referenced_vertices", "edges", "boundary_edges", "nonmanifold_edges", "boundary_vertices",
                 "nonmanifold_vertices", "euler", "closed")

    def __init__(self, vertex_root, face_root, vertex_flags, vertex_labels, face_labels, roots, face_sizes, vertex_sizes, counts=(0,) * 7):
        self.vertex_root, self.face_root, self.vertex_flags = vertex_root, face_root, vertex_flags
        self.vertex_labels, self.face_labels, self.roots, self.face_sizes, self.vertex_sizes = vertex_labels, face_labels, roots, face_sizes, vertex_sizes
        self.num_components = int(roots.numel())
        (self.live_faces, self.referenced_vertices, self.edges, self.boundary_edges, self.nonmanifold_edges, self.boundary_vertices,
         self.nonmanifold_vertices) = (int(c) for c in counts)
        self.euler = self.referenced_vertices - self.edges + self.live_faces
        self.closed = self.live_faces > 0 and self.boundary_edges == 0


class MeshSubset(Mesh):
    """A Mesh from select_faces / remove_small_components: additionally source_index (M',) int64, the input index of every output vertex;
    face_index (F',) int64, the input index of every output face; pixel_index (M',) int64 = mesh.pixel_index[source_index] when the
    input carried one (a MapMesh, a SimplifiedMesh of one), else None."""
    __slots__ = ("source_index", "face_index", "pixel_index")

    def __init__(self, vertices, faces, normals, colors, transform, extrinsic=None, scene_scale=None, source_index=None, face_index=None,
                 pixel_index=None):
        Mesh.__init__(self, vertices, faces, normals, colors, transform, extrinsic, scene_scale)
        self.source_index, self.face_index, self.pixel_index = source_index, face_index, pixel_index


def _mesh_arrays(what, mesh, *more):
    """The checks the mesh operations share -> (vertices f32 (M,3), faces int32 (F,3), M, F, device); tensors are None for an empty mesh."""
    if not isinstance(mesh, Mesh):
        raise ValueError("%s: expected a Mesh" % what)
    vert, faces = mesh.vertices, mesh.faces
    if vert is None or faces is None:
        raise ValueError("%s: the mesh has no vertices or no faces tensor" % what)
    for t in (vert, faces, mesh.normals, mesh.colors, getattr(mesh, "pixel_index", None)) + more:
        if t is not None and not (isinstance(t, torch.Tensor) and t.is_cuda):
            raise ops.L.OvgError("%s needs HIP device tensors: there is no CPU fallback" % what)
    M, F = int(vert.shape[0]), int(faces.shape[0])
    if M >= 1 << 31 or F >= 1 << 31:
        raise ValueError("%s: the mesh has 2^31 vertices or faces or more" % what)
    if M == 0 or F == 0:
        return None, None, M, F, vert.device
    return vert.reshape(M, 3).float().contiguous(), faces.reshape(F, 3).to(torch.int32).contiguous(), M, F, vert.device


def _mesh_mask(what, name, mask, n):
    if mask is None:
        return None
    if not isinstance(mask, torch.Tensor) or mask.dtype not in (torch.bool, torch.uint8) or mask.numel() != n:
        raise ValueError("%s: %s must be a bool / uint8 tensor of %d elements" % (what, name, n))
    return mask


def mesh_topology(mesh, order="size"):
    """What hangs together in a Mesh, and how its edges are used, on the device (ovg_mesh_topology; tests/meshops_twin.py restates the
    rule). A vertex is valid when its coordinates are finite; a face is live when its indices lie in the mesh, are pairwise different
    and name valid vertices (zero area does not matter). Two vertices are connected when a live face names both, and a component is
    named by its lowest vertex index. This is VERTEX connectivity: two faces that meet in one corner only are one component, where
    Open3D's cluster_connected_triangles (faces joined across shared edges) would give two. An edge held by one live face is a boundary
    edge, by three or more a non-manifold edge (a duplicated face counts twice); their end vertices carry MT_BOUNDARY / MT_NONMANIFOLD.

    order: "size" (default) numbers the components by descending face count, equal counts by ascending root, exactly as cluster_points
    numbers clusters, so label 0 is the largest piece; "index" numbers them by ascending root.

    -> MeshTopology. One read of the eight counts (the dense labels read the number of components back as well, as cluster_points
    does). A mesh without vertices or without faces returns empty results without a launch. CPU tensors raise OvgError (there is no
    CPU fallback), OVG_MT_INTERNAL (the union-find left its bounds: a bug) raises OvgError too.
    Not in it: hole filling, edge-adjacency components, pinch-vertex detection (two fans meeting in one vertex pass as manifold),
    cotangent or area weights, quadric simplification, any guarantee that smoothing keeps a mesh free of self-intersections."""
    what = "mesh_topology"
    if order not in ("size", "index"):
        raise ValueError("%s: order must be \"size\" or \"index\", got %r" % (what, order))
    vert, faces, M, F, dev = _mesh_arrays(what, mesh)
    if vert is None:
        none32 = lambda n: torch.full((n,), -1, device=dev, dtype=torch.int32)
        return MeshTopology(none32(M), none32(F), torch.zeros(M, device=dev, dtype=torch.uint8), none32(M), none32(F), none32(0),
                            torch.zeros(0, device=dev, dtype=torch.int64), torch.zeros(0, device=dev, dtype=torch.int64))
    vroot, froot = torch.empty(M, device=dev, dtype=torch.int32), torch.empty(F, device=dev, dtype=torch.int32)
    vflags, count = torch.empty(M, device=dev, dtype=torch.uint8), torch.empty(8, device=dev, dtype=torch.int64)
    ws = torch.empty(ops.mesh_topology_workspace_bytes(M, F), device=dev, dtype=torch.uint8)
    ops.mesh_topology(vert, faces, ws, vroot, froot, vflags, count)
    counts = count.cpu().tolist()                                                                    # the one read of the counts
    if counts[7] & ops.L.MT_INTERNAL:
        raise ops.L.OvgError("%s: the union-find left its bounds (OVG_MT_INTERNAL): no result" % what)
    fmember, vmember = froot >= 0, vroot >= 0
    roots, finverse, fsizes = torch.unique(froot[fmember], return_inverse=True, return_counts=True)   # ascending root
    vinverse = torch.searchsorted(roots, vroot[vmember])                                             # every component holds a live face
    vsizes = torch.bincount(vinverse, minlength=roots.numel())
    if order == "size":
        by_size = torch.sort(fsizes, descending=True, stable=True).indices                           # equal sizes: ascending root
        rank = torch.empty_like(by_size)
        rank[by_size] = torch.arange(by_size.numel(), device=dev)
        roots, fsizes, vsizes, finverse, vinverse = roots[by_size], fsizes[by_size], vsizes[by_size], rank[finverse], rank[vinverse]
    flabels, vlabels = torch.full_like(froot, -1), torch.full_like(vroot, -1)
    flabels[fmember] = finverse.to(torch.int32)
    vlabels[vmember] = vinverse.to(torch.int32)
    return MeshTopology(vroot, froot, vflags, vlabels, flabels, roots, fsizes.to(torch.int64), vsizes.to(torch.int64), counts[:7])


def select_faces(mesh, face_mask=None, vertex_mask=None):
    """The sub-mesh of the live faces that face_mask keeps (bool / uint8 (F,), None: all) and whose three corners vertex_mask keeps
    (bool / uint8 (M,), None: all), on the device (ovg_mesh_select): one output vertex per vertex a kept face names, in ascending input
    index; the kept faces in input order with their corners renumbered. Called without a mask it drops the faces that are not live
    (an index outside the mesh, a repeated index, a vertex with a non-finite coordinate) and the vertices nothing names.

    -> MeshSubset: normals, colours and pixel_index gathered through source_index; transform, extrinsic and scene_scale passed through
    unchanged, so the writers, render_mesh, simplify_mesh and smooth_mesh take it as it is. Exactly one device -> host synchronisation
    (the two counts). A mesh without vertices or without faces returns an empty mesh without a launch. CPU tensors raise OvgError."""
    what = "select_faces"
    if not isinstance(mesh, Mesh):
        raise ValueError("%s: expected a Mesh" % what)
    M0 = 0 if mesh.vertices is None else int(mesh.vertices.shape[0])
    F0 = 0 if mesh.faces is None else int(mesh.faces.shape[0])
    face_mask, vertex_mask = _mesh_mask(what, "face_mask", face_mask, F0), _mesh_mask(what, "vertex_mask", vertex_mask, M0)
    vert, faces, M, F, dev = _mesh_arrays(what, mesh, face_mask, vertex_mask)
    nrm, col, pix = mesh.normals, mesh.colors, getattr(mesh, "pixel_index", None)

    def result(v, f, src, fidx):
        return MeshSubset(v, f, None if nrm is None else nrm.reshape(M, 3)[src], None if col is None else col.reshape(M, 3)[src], mesh.transform,
                          mesh.extrinsic, mesh.scene_scale, src, fidx, None if pix is None else pix.reshape(M)[src])
    Mo = Fo = 0
    if vert is not None:
        ws = torch.empty(ops.mesh_select_workspace_bytes(M, F), device=dev, dtype=torch.uint8)
        count = torch.empty(2, device=dev, dtype=torch.int64)
        args = dict(vertices=vert, faces=faces, ws=ws, face_keep=None if face_mask is None else face_mask.reshape(F).to(torch.uint8).contiguous(),
                    vertex_keep=None if vertex_mask is None else vertex_mask.reshape(M).to(torch.uint8).contiguous(), out_count=count)
        ops.mesh_select(ops.L.MSEL_COUNT, **args)
        Mo, Fo = (int(c) for c in count.cpu().tolist())                                              # the one synchronisation
    out_v, out_f = torch.empty(Mo, 3, device=dev, dtype=torch.float32), torch.empty(Fo, 3, device=dev, dtype=torch.int32)
    src, fidx = torch.empty(Mo, device=dev, dtype=torch.int64), torch.empty(Fo, device=dev, dtype=torch.int64)
    if Fo:
        ops.mesh_select(ops.L.MSEL_SCATTER, vertex_capacity=Mo, face_capacity=Fo, out_vertices=out_v, source_index=src, out_faces=out_f,
                        face_index=fidx, **args)
    return result(out_v, out_f, src, fidx)


def remove_small_components(mesh, min_faces=None, rel_faces=None, keep_largest=None):
    """A Mesh without its detached pieces (mesh_topology followed by select_faces): the shells a fused volume keeps where a few lattice
    points survived carving, the islands map_edges cut loose from a grid mesh. Exactly one of the three must be given: min_faces (a
    positive integer: the components with at least that many live faces stay), rel_faces (a float in (0, 1]: those with at least
    rel_faces x the mesh's live faces), keep_largest=True (the component with the most live faces alone, equal counts going to the
    lowest root). Components are mesh_topology's: vertex connectivity. -> MeshSubset, faces and vertices in input order."""
    import math
    what = "remove_small_components"
    if keep_largest is not None and not isinstance(keep_largest, bool):
        raise ValueError("%s: keep_largest must be True, False or None, got %r" % (what, keep_largest))
    if (min_faces is not None) + (rel_faces is not None) + bool(keep_largest) != 1:
        raise ValueError("%s: give exactly one of min_faces, rel_faces and keep_largest" % what)
    if min_faces is not None and (isinstance(min_faces, bool) or not isinstance(min_faces, int) or min_faces < 1):
        raise ValueError("%s: min_faces must be a positive integer, got %r" % (what, min_faces))
    if rel_faces is not None:
        if isinstance(rel_faces, bool) or not isinstance(rel_faces, (int, float)) or not (math.isfinite(rel_faces) and 0.0 < rel_faces <= 1.0):
            raise ValueError("%s: rel_faces must be a float in (0, 1], got %r" % (what, rel_faces))
    topo = mesh_topology(mesh, order="size")
    if topo.num_components == 0:
        return select_faces(mesh, face_mask=torch.zeros_like(topo.face_root, dtype=torch.bool))
    if keep_largest:
        keep = topo.face_labels == 0
    else:
        least = float(min_faces) if min_faces is not None else float(rel_faces) * topo.live_faces
        keep = (topo.face_labels >= 0) & (topo.face_sizes[topo.face_labels.clamp_min(0).long()].double() >= least)
    return select_faces(mesh, face_mask=keep)


MESH_NORMALS = ("recompute", "keep", None)


def _smooth(what, mesh, iterations, lam, mu, fix_boundary, fixed, want_normals):
    """-> (vertices, normals or None) of ovg_mesh_smooth on the mesh, or None for a mesh without vertices or faces."""
    M0 = 0 if not isinstance(mesh, Mesh) or mesh.vertices is None else int(mesh.vertices.shape[0])
    fixed = _mesh_mask(what, "fixed", fixed, M0)
    vert, faces, M, F, dev = _mesh_arrays(what, mesh, fixed)
    if vert is None:
        return None
    out_v = torch.empty(M, 3, device=dev, dtype=torch.float32)
    out_n = torch.empty(M, 3, device=dev, dtype=torch.float32) if want_normals else None
    status = torch.empty(1, device=dev, dtype=torch.int64)
    ws = torch.empty(ops.mesh_smooth_workspace_bytes(M, F), device=dev, dtype=torch.uint8)
    ops.mesh_smooth(vert, faces, ws, iterations, lam, mu, out_v, status, fixed=None if fixed is None else fixed.reshape(M).to(torch.uint8).contiguous(),
                    fix_boundary=fix_boundary, out_normals=out_n)
    if iterations and int(status.cpu()) & ops.L.MSM_NONFINITE:                                       # the one synchronisation
        raise ValueError("%s: a vertex left the finite float32 range (OVG_MSM_NONFINITE)" % what)
    return out_v, out_n


def smooth_mesh(mesh, iterations=10, lam=0.5, mu=-0.53, fix_boundary=True, fixed=None, normals="recompute"):
    """Laplacian / Taubin smoothing of a Mesh on the device (ovg_mesh_smooth; tests/meshops_twin.py restates the rule bit for bit).
    Every iteration moves each movable vertex by lam towards the mean of its neighbours and then, when mu != 0, by mu (negative: away
    from it) -- Taubin's pair, which takes the noise out without the shrinking of the plain Laplacian (mu = 0). The neighbours of a
    vertex are the other two corners of every live face that names it, so a neighbour across a manifold edge counts twice and the mean
    is the umbrella mean; duplicated faces and non-manifold edges weigh in by their multiplicity. The sums run in integers on a 2^30
    grid that is laid over the mesh anew in every step: two calls, and any schedule, give identical bytes.

    A vertex moves when its coordinates are finite, a live face names it, fixed (bool / uint8 (M,), optional) is 0 there and, with
    fix_boundary (default), it ends no boundary edge; every other vertex keeps its bytes. All of that is decided on the input mesh.
    lam in (0, 1], mu <= 0 and finite, iterations an int in [0, 1000]. normals: "recompute" (default: area-free face normals of the
    smoothed mesh summed per vertex and normalised, (0, 0, 0) where none is usable), "keep" (the input's) or None.

    -> a mesh of the input's own class with new vertices and normals, everything else shared with the input. One device -> host
    synchronisation (the status). A mesh without vertices or without faces is returned as it is, without a launch. A vertex that
    leaves the finite float32 range raises ValueError; CPU tensors raise OvgError: there is no CPU fallback.
    Not in it: hole filling, edge-adjacency components, pinch-vertex detection, cotangent or area weights, quadric simplification,
    any guarantee that smoothing keeps a mesh free of self-intersections."""
    import copy
    import math
    what = "smooth_mesh"
    if not isinstance(mesh, Mesh):
        raise ValueError("%s: expected a Mesh" % what)
    if isinstance(iterations, bool) or not isinstance(iterations, int) or not 0 <= iterations <= 1000:
        raise ValueError("%s: iterations must be an integer in [0, 1000], got %r" % (what, iterations))
    for name, v in (("lam", lam), ("mu", mu)):
        if isinstance(v, bool) or not isinstance(v, (int, float)) or not math.isfinite(v):
            raise ValueError("%s: %s must be a finite number, got %r" % (what, name, v))
    if not 0.0 < lam <= 1.0:
        raise ValueError("%s: lam must lie in (0, 1], got %r" % (what, lam))
    if mu > 0.0:
        raise ValueError("%s: mu must be <= 0, got %r" % (what, mu))
    if not isinstance(fix_boundary, bool):
        raise ValueError("%s: fix_boundary must be True or False, got %r" % (what, fix_boundary))
    if not (normals is None or isinstance(normals, str)) or normals not in MESH_NORMALS:
        raise ValueError("%s: normals must be one of %r, got %r" % (what, MESH_NORMALS, normals))
    got = _smooth(what, mesh, iterations, float(lam), float(mu), fix_boundary, fixed, normals == "recompute")
    out = copy.copy(mesh)
    if got is not None:
        out.vertices = got[0]
        out.normals = got[1] if normals == "recompute" else (mesh.normals if normals == "keep" else None)
    elif normals is None:
        out.normals = None
    return out


def mesh_vertex_normals(mesh):
    """Vertex normals of a Mesh from its faces, on the device (ovg_mesh_smooth with no iteration): per live face the unit normal
    (pb - pa) x (pc - pa) in float64, summed per vertex in integers (order-free) and normalised; (0, 0, 0) for a vertex without a
    usable face. -> f32 (M, 3) device tensor; an empty (0, 3) or all-zero tensor for a mesh without vertices or faces."""
    what = "mesh_vertex_normals"
    if not isinstance(mesh, Mesh):
        raise ValueError("%s: expected a Mesh" % what)
    got = _smooth(what, mesh, 0, 0.5, 0.0, False, None, True)
    if got is None:
        M = 0 if mesh.vertices is None else int(mesh.vertices.shape[0])
        return torch.zeros(M, 3, device=mesh.vertices.device if mesh.vertices is not None else "cpu", dtype=torch.float32)
    return got[1]
