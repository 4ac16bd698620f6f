"""ovg_deptheval_median / ovg_deptheval_sums / ovg_deptheval_solve and postprocess.align_depth, depth_metrics, relative_pose_errors,
pose_auc, evaluate_predictions on the device against tests/deptheval_twin.py: every output byte for byte in exact-size guarded buffers
(sizes around the thread block, the tile and the second fold's stride; masks; non-finite, zero, negative and subnormal values; the open
and the closed depth bound; the median's tie and byte structures; the strict delta thresholds and both clips), the one sum that holds
a logarithm within 1e-10, the pose angles within 1e-9 degrees with exact counts, and the gated cases of the three entries for the
stream contract's coverage test. Every case runs twice."""
import ctypes

import numpy as np
import pytest
import torch

import deptheval_twin as twin
import stream_contract as sc
import test_gpu_stream_contract as tsc
from kernel_guards import GUARD_BYTE, guarded
from omnivggt_official_amd import lib as L
from omnivggt_official_amd import ops, postprocess

pytestmark = pytest.mark.gpu
F = np.float32
MODES = (twin.NONE, twin.MEDIAN, twin.SCALE, twin.SCALE_SHIFT)
N_SMALL = [1, 2, 63, 64, 65, 255, 256, 257, 1023, 1024, 1025, 2049]
FRAME = 518 * 518                                                             # 263 tiles: more than the 256 threads of the second fold
WORST_LOG = [0.0]                                                             # largest relative deviation of the log sum seen in this session


@pytest.fixture(autouse=True)
def _need_gpu():
    L.require_gpu()
    yield


def _dev(a):
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _g(shape, dtype):
    v, chk = guarded((1,) + tuple(shape), dtype, "cuda", guard_bytes=4096)
    return v[0], chk


def _median(p, g, v, lo, hi):
    G, n = p.shape
    (count, c0), (med, c1), (ws, c2) = _g((G,), torch.int64), _g((G, 2, 2), torch.float32), _g((ops.deptheval_median_workspace_bytes(G, n),), torch.uint8)
    ops.deptheval_median(p, g, v, lo, hi, ws=ws, count=count, median=med)
    torch.cuda.synchronize()
    c0("count"), c1("median"), c2("median workspace")
    return count.cpu().numpy(), med.cpu().numpy()


def _sums(p, g, v, lo, hi, coeff=None, clip_min=1e-3, clip_max=np.inf):
    G, n = p.shape
    (counts, c0), (sums, c1), (ws, c2) = _g((G, 4), torch.int64), _g((G, 5), torch.float64), _g((ops.deptheval_sums_workspace_bytes(G, n),), torch.uint8)
    ops.deptheval_sums(p, g, v, lo, hi, coeff=_dev(coeff), clip_min=clip_min, clip_max=clip_max, ws=ws, counts=counts, sums=sums)
    torch.cuda.synchronize()
    c0("counts"), c1("sums"), c2("sums workspace")
    return counts.cpu().numpy(), sums.cpu().numpy()


def _solve(mode, count, sums=None, med=None):
    G = len(count)
    (coeff, c0), (status, c1) = _g((G, 2), torch.float64), _g((G,), torch.int32)
    ops.deptheval_solve(mode, _dev(count), _dev(sums), _dev(med), coeff=coeff, status=status)
    torch.cuda.synchronize()
    c0("coeff"), c1("status")
    return coeff.cpu().numpy(), status.cpu().numpy()


def _log_floor(pred, gt, valid, lo, hi, coeff, clip_min, clip_max, want):
    """Where the 1e-10 of the log sum is claimed, and what holds elsewhere. The bound of DESIGN 12m presupposes |log| <= 2.1 and
    rmse_log >= 0.01. A group outside it (a single survivor that the alignment maps ONTO its ground truth has d = log q - log g of a few
    ulp: nothing but the logarithms' rounding) is held to the absolute error the same reasoning gives: each logarithm within 4 ulp of
    its magnitude, so d within delta = 8 x 2^-52 x max|log|, a term d d within 2 |d| delta + delta^2, N of them. -> float64 [G]:
    0 where the relative bound alone applies."""
    use = twin.used(pred, gt, valid, lo, hi)
    floor = np.zeros(len(pred))
    with np.errstate(all="ignore"):
        for k in range(len(pred)):
            n = int(use[k].sum())
            if n == 0:
                continue
            lq = np.log(twin.aligned(pred[k][use[k]], coeff[k], clip_min, clip_max))
            lg = np.log(gt[k][use[k]].astype(np.float64))
            big = max(np.abs(lq).max(), np.abs(lg).max())
            if big <= 2.1 and np.sqrt(want[k] / n) >= 0.01:
                continue
            delta = 8 * 2.0 ** -52 * big
            floor[k] = n * (2 * np.abs(lq - lg).max() * delta + delta * delta)
    return floor


def _same(got, want, name, log_floor=None):
    """Bytes; with log_floor (float64 [G], from _log_floor) the last column of a sums array is held to 1e-10 relative instead, or to
    that absolute floor where it is not 0 (and the deviation is recorded)."""
    got, want = np.asarray(got), np.asarray(want)
    assert got.dtype == want.dtype and got.shape == want.shape, (name, got.dtype, want.dtype, got.shape, want.shape)
    if log_floor is not None:
        a, b = got[:, 4], want[:, 4]
        both = np.isfinite(a) & np.isfinite(b)
        assert (both == np.isfinite(b)).all() and np.array_equal(a[~both], b[~both], equal_nan=True), (name, a, b)
        floor = np.where(np.isfinite(log_floor), log_floor, 0.0)
        assert (np.abs(a[both] - b[both]) <= np.maximum(1e-10 * np.abs(b[both]), floor[both])).all(), (name, a, b, floor)
        nz = both & (b != 0) & (floor == 0)
        if nz.any():
            WORST_LOG[0] = max(WORST_LOG[0], float((np.abs(a[nz] - b[nz]) / np.abs(b[nz])).max()))
        got, want = got[:, :4], want[:, :4]
    assert np.ascontiguousarray(got).tobytes() == np.ascontiguousarray(want).tobytes(), (name, np.argwhere(got != want)[:8].tolist(), got, want)


def _check_all(pred, gt, valid, lo=0.0, hi=np.inf, clip_min=1e-3, clip_max=np.inf, name=""):
    """Every entry on one input, twice, against the twin: the medians, the moments, the four solves, the metrics under each."""
    p, g, v = _dev(pred), _dev(gt), _dev(valid)
    w_med = twin.median(pred, gt, valid, lo, hi)
    w_mom = twin.sums(pred, gt, valid, lo, hi)
    for rep in range(2):
        tag = "%s run %d" % (name, rep)
        med, mom = _median(p, g, v, lo, hi), _sums(p, g, v, lo, hi)
        _same(med[0], w_med[0], tag + " median count"), _same(med[1], w_med[1], tag + " median")
        _same(mom[0], w_mom[0], tag + " moment counts"), _same(mom[1], w_mom[1], tag + " moments")
        for mode in MODES:
            w_coeff, w_status = twin.solve(mode, w_mom[0], w_mom[1], w_med[1])
            coeff, status = _solve(mode, mom[0] if mode != twin.MEDIAN else med[0], mom[1], med[1])
            _same(coeff, w_coeff, "%s coeff mode %d" % (tag, mode)), _same(status, w_status, "%s status mode %d" % (tag, mode))
            assert not np.isnan(coeff).any()
            if rep and mode != twin.SCALE_SHIFT:                              # the metric kernel knows no mode, only coefficients: one set is rerun
                continue
            w_met = twin.sums(pred, gt, valid, lo, hi, twin.METRICS, w_coeff, clip_min, clip_max)
            met = _sums(p, g, v, lo, hi, coeff, clip_min, clip_max)
            floor = _log_floor(pred, gt, valid, lo, hi, w_coeff, clip_min, clip_max, w_met[1][:, 4])
            _same(met[0], w_met[0], "%s metric counts mode %d" % (tag, mode)), _same(met[1], w_met[1], "%s metrics mode %d" % (tag, mode), log_floor=floor)
    return w_med, w_mom


def _maps(G, n, seed, mask):
    """gt in [0.5, 8], pred = gt (1 + 0.1 noise) 1.7 + 0.3, with every special value planted among the masked-out and the unmasked
    pixels (where the row is long enough), gt on the open lower bound 0.5 (excluded) and on the closed upper bound 8 (included)."""
    rng = np.random.default_rng(seed)
    gt = rng.uniform(0.5, 8.0, (G, n)).astype(F)
    pred = (gt * (1 + 0.1 * rng.normal(size=(G, n))) * 1.7 + 0.3).astype(F)
    valid = None
    if mask == "half":
        valid = (rng.random((G, n)) < 0.5).astype(np.uint8)
    elif mask == "empty_group":
        valid = (rng.random((G, n)) < 0.5).astype(np.uint8)
    elif mask == "single":
        valid = np.zeros((G, n), np.uint8)
        valid[np.arange(G), rng.integers(0, n, G)] = 1
    if n >= 63:
        specials = [np.nan, np.inf, -np.inf, 0.0, -1.5, 1e-45, -1e-45]
        for k in range(G):
            at = rng.choice(n, 4 * len(specials) + 4, replace=False)
            for i, s in enumerate(specials):
                pred[k, at[4 * i]], gt[k, at[4 * i + 1]] = s, s
                if valid is not None and mask != "single":
                    valid[k, at[4 * i]], valid[k, at[4 * i + 1]] = 1, 1
                    pred[k, at[4 * i + 2]], gt[k, at[4 * i + 3]] = s, s
                    valid[k, at[4 * i + 2]], valid[k, at[4 * i + 3]] = 0, 0
            gt[k, at[-4]], gt[k, at[-3]] = 0.5, 8.0
            if valid is not None and mask != "single":
                valid[k, at[-4]], valid[k, at[-3]] = 1, 1
    if mask == "empty_group":
        valid[G // 2] = 0
    return pred, gt, valid


@pytest.mark.parametrize("mask", ["none", "half", "empty_group", "single"])
@pytest.mark.parametrize("G", [1, 3, 64])
def test_every_output_matches_the_twin_small_sizes(G, mask):
    assert (L.DEPTHEVAL_TILE, L.DEPTHEVAL_THREADS) == (1024, 256)
    for n in N_SMALL:
        pred, gt, valid = _maps(G, n, 1000 * G + n, mask)
        w_med, _ = _check_all(pred, gt, valid, 0.5, 8.0, name="G %d n %d %s" % (G, n, mask))
        use = twin.used(pred, gt, valid, 0.5, 8.0)
        assert (w_med[0] == use.sum(1)).all() and not use[gt == F(0.5)].any()
        if mask in ("none", "half") and n >= 63:
            assert use[gt == F(8.0)].all() and (w_med[0] < n).all()           # the bound pixel counts; the specials do not
        if mask == "empty_group" and G > 1:
            assert w_med[0][G // 2] == 0
        if mask == "single":
            assert (w_med[0] <= 1).all()


def test_every_output_matches_the_twin_one_frame_per_group():
    pred, gt, valid = _maps(3, FRAME, 7, "half")
    assert (FRAME + 1023) // 1024 == 263
    w_med, _ = _check_all(pred, gt, valid, 0.5, 8.0, clip_max=12.0, name="3 x 518^2")
    assert (w_med[0] > 100000).all()


def _from_bits(bits):
    return np.asarray(bits, np.uint32).view(F)


def test_median_stress_ties_bytes_and_bins():
    """One call, one group per structure, rows cut to their length by the mask. pred and gt of a group carry DIFFERENT structures."""
    n = 70016
    rows = []
    rows.append(np.full(n, 2.5, F))                                           # all equal
    r = np.full(70005, 3.25, F)                                               # 70 000 copies (more than a 16-bit bin holds) and a few others
    r[:5] = [1.0, 2.0, 7.0, 9.0, 3.0]
    rows.append(r)
    rows.append((1.0 + np.arange(256) * 2.0 ** -23).astype(F))                # keys that differ in the lowest byte only
    rows.append(_from_bits((np.arange(1, 127, dtype=np.uint32) << 24) | 0x00345678))   # ... in the highest byte only
    rows.append(np.concatenate([np.full(500, 1.5, F), np.full(500, 3.0, F)])) # even n: the two middles in different top-byte bins (0x3f / 0x40)
    rows.append(np.concatenate([np.full(500, 1.5, F), np.full(501, 3.0, F)])) # odd n: both ranks are the same element
    rows.append(_from_bits(np.random.default_rng(3).integers(1, 0x7f800000, 4097, dtype=np.uint32)))   # any positive finite key, subnormals too
    rows.append(_from_bits(np.arange(1, 300, dtype=np.uint32)))               # subnormals only
    G = len(rows)
    rng = np.random.default_rng(11)
    pred, gt, valid = np.ones((G, n), F), np.ones((G, n), F), np.zeros((G, n), np.uint8)
    for k, r in enumerate(rows):
        at = rng.permutation(n)[:len(r)]                                      # scattered over the chunks of the histogram pass
        pred[k, at], gt[k, at], valid[k, at] = rng.permutation(r), np.resize(rng.permutation(rows[(k + 3) % G]), len(r)), 1
    w_med, _ = _check_all(pred, gt, valid, name="median stress")
    assert w_med[0].tolist() == [len(r) for r in rows]
    assert w_med[1][0, 0].tolist() == [2.5, 2.5] and w_med[1][1, 0].tolist() == [3.25, 3.25] and w_med[1][4, 0].tolist() == [1.5, 3.0]
    full = np.stack([np.concatenate([r, np.full(n - len(r), r[0], F)]) for r in rows[:2]])      # no mask at all: the whole rows
    w2, _ = _check_all(full, full[::-1].copy(), None, name="median stress, unmasked")
    assert w2[0].tolist() == [n, n] and w2[1][1, 0].tolist() == [3.25, 3.25]
    even = np.concatenate([np.full(500, 1.5, F), np.full(500, 3.0, F)])[None]
    assert twin.median(even, even)[1][0, 0].tolist() == [1.5, 3.0]
    _check_all(even, even[:, ::-1].copy(), None, name="split middles")


def test_metric_stress_strict_deltas_clips_and_negative_fits():
    # ratios of exactly 1.25, 1.25^2, 1.25^3 (and their reciprocals where f32 holds them) are not below their thresholds
    q = np.array([[1.25, 1.5625, 1.953125, 0.5, 1.0, 1.2499999, 1.5624999, 1.9531249]], F)
    g = np.ones_like(q)
    g[0, 3] = 0.625                                                           # g / q = 1.25 exactly
    ident = np.array([[1.0, 0.0]])
    for rep in range(2):
        counts, sums = _sums(_dev(q), _dev(g), None, 0.0, np.inf, ident)
        w = twin.sums(q, g, mode=twin.METRICS, coeff=ident)
        _same(counts, w[0], "strict deltas"), _same(sums, w[1], "strict delta sums", log_floor=_log_floor(q, g, None, 0.0, np.inf, ident, 1e-3, np.inf, w[1][:, 4]))
        assert counts[0].tolist() == [8, 2, 5, 7]
    # q below clip_min and above a finite clip_max, a negative s p + t, coefficients that are not numbers
    pred, gt, valid = _maps(3, 2049, 5, "half")
    for coeff, cmin, cmax in ((np.array([[1e-5, 0.0], [40.0, 0.0], [1.0, -3.0]]), 1e-3, 30.0), (np.array([[1.0, -50.0], [np.nan, 0.0], [np.inf, 1.0]]), 0.25, np.inf),
                              (np.array([[2.0, 0.5], [1e300, 1e300], [0.5, -0.25]]), 1e-3, 2.0)):
        w = twin.sums(pred, gt, valid, 0.5, 8.0, twin.METRICS, coeff, cmin, cmax)
        for rep in range(2):
            got = _sums(_dev(pred), _dev(gt), _dev(valid), 0.5, 8.0, coeff, cmin, cmax)
            _same(got[0], w[0], "clip counts"), _same(got[1], w[1], "clip sums", log_floor=_log_floor(pred, gt, valid, 0.5, 8.0, coeff, cmin, cmax, w[1][:, 4]))
    # through the public entry: a steep line whose intercept is far below zero, so that small pred land under the clip
    rng = np.random.default_rng(9)
    p = rng.uniform(0.05, 4.0, (2, 31, 33)).astype(F)
    gtm = np.maximum(3.0 * p - 2.0, 0.05).astype(F)
    res = postprocess.depth_metrics(_dev(p), _dev(gtm), align="scale_shift", clip_min=0.01)
    coeff = np.stack([res.scale.cpu().numpy(), res.shift.cpu().numpy()], 1)
    assert (coeff[:, 1] < -1.0).all() and ((coeff[:, 0:1] * p.reshape(2, -1) + coeff[:, 1:2]) < 0).any()
    w = twin.sums(p.reshape(2, -1), gtm.reshape(2, -1), mode=twin.METRICS, coeff=coeff, clip_min=0.01)
    _same(res.n.cpu().numpy(), w[0][:, 0], "n"), _same(res.abs_rel.cpu().numpy(), twin.figures(*w)["abs_rel"], "abs_rel under the clip")


@pytest.mark.parametrize("scope", ["view", "sequence"])
@pytest.mark.parametrize("align", ["none", "median", "scale", "scale_shift"])
def test_depth_metrics_every_alignment_and_scope(align, scope):
    S, H, W = 3, 37, 29
    rng = np.random.default_rng(21)
    gt = rng.uniform(0.5, 8.0, (S, H, W)).astype(F)
    pred = (gt * (1 + 0.1 * rng.normal(size=gt.shape)) * 1.7 + 0.3).astype(F)
    valid = rng.random((S, H, W)) < 0.5
    shape = (S, H * W) if scope == "view" else (1, S * H * W)
    p2, g2, v2 = pred.reshape(shape), gt.reshape(shape), valid.reshape(shape).astype(np.uint8)
    mode = postprocess.DEPTH_ALIGNMENTS[align]
    w_med, w_mom = twin.median(p2, g2, v2, 0.6, 7.5), twin.sums(p2, g2, v2, 0.6, 7.5)
    w_coeff, w_status = twin.solve(mode, w_mom[0], w_mom[1], w_med[1])
    w_counts, w_sums = twin.sums(p2, g2, v2, 0.6, 7.5, twin.METRICS, w_coeff, 1e-3, 8.0)
    fig = twin.figures(w_counts, w_sums)
    # the condition under which the log sum's bound of 1e-10 is claimed
    q = np.clip(w_coeff[:, 0:1] * p2.astype(np.float64) + w_coeff[:, 1:2], 1e-3, 8.0)
    use = twin.used(p2, g2, v2, 0.6, 7.5)
    assert max(np.abs(np.log(q[use])).max(), np.abs(np.log(g2[use].astype(np.float64))).max()) <= 2.1 and fig["rmse_log"].min() >= 0.01
    for rep in range(2):
        for vv in (valid, valid.astype(np.uint8)[..., None]) if rep == 0 else (valid,):
            scale, shift, status = postprocess.align_depth(_dev(pred), _dev(gt[..., None]), _dev(vv), align, scope, 0.6, 7.5)
            _same(scale.cpu().numpy(), w_coeff[:, 0], "scale"), _same(shift.cpu().numpy(), w_coeff[:, 1], "shift"), _same(status.cpu().numpy(), w_status, "status")
            res = postprocess.depth_metrics(_dev(pred[..., None]), _dev(gt), _dev(vv), align, scope, 0.6, 7.5, clip_max=8.0)
            assert (res.align, res.scope, res.n_total) == (align, scope, int(w_counts[:, 0].sum())) and (w_status == 0).all()
            _same(res.n.cpu().numpy(), w_counts[:, 0], "n"), _same(res.scale.cpu().numpy(), w_coeff[:, 0], "scale"), _same(res.shift.cpu().numpy(), w_coeff[:, 1], "shift")
            for k in postprocess.DEPTH_FIGURES:
                got = getattr(res, k).cpu().numpy()
                if k == "rmse_log":
                    assert (np.abs(got - fig[k]) <= 1e-10 * fig[k]).all(), (k, got, fig[k])
                    WORST_LOG[0] = max(WORST_LOG[0], float((np.abs(got - fig[k]) / fig[k]).max()))
                else:
                    _same(got, fig[k], k)
                pooled = twin.figures(w_counts.sum(0, keepdims=True), w_sums.sum(0, keepdims=True))[k][0]
                assert abs(res.mean[k] - fig[k].mean()) <= 1e-10 * abs(fig[k].mean()) and abs(res.pooled[k] - pooled) <= 1e-10 * abs(pooled), k
    if align != "none":
        assert (np.abs(w_coeff[:, 0] - 1 / 1.7) < 0.1).all() and fig["delta1"].min() > 0.8                    # the alignment undoes the planted scale
    print("largest relative deviation of the log sum so far: %.3g" % WORST_LOG[0])


def test_groups_without_pixels_report_nan_and_the_summary_skips_them():
    gt = np.random.default_rng(2).uniform(1, 4, (3, 9, 7)).astype(F)
    pred = (gt * 2).astype(F)
    valid = np.ones((3, 9, 7), bool)
    valid[1] = False
    res = postprocess.depth_metrics(_dev(pred), _dev(gt), _dev(valid), "scale")
    assert res.n.tolist() == [63, 0, 63] and res.status.tolist() == [0, postprocess.DEPTH_FEW, 0] and res.scale.tolist() == [0.5, 1.0, 0.5]
    for k in postprocess.DEPTH_FIGURES:
        v = getattr(res, k).cpu().numpy()
        assert np.isnan(v[1]) and np.isfinite(v[[0, 2]]).all() and np.isfinite(res.mean[k]) and np.isfinite(res.pooled[k])
    assert res.mean["abs_rel"] == 0.0 and res.mean["delta1"] == 1.0 and res.n_total == 126
    none = postprocess.depth_metrics(_dev(pred), _dev(gt), _dev(np.zeros((3, 9, 7), bool)), "median", "sequence")
    assert none.n.tolist() == [0] and none.status.tolist() == [postprocess.DEPTH_FEW] and np.isnan(none.mean["rmse"]) and none.n_total == 0


def test_bad_arguments_are_refused_and_write_nothing():
    lib = L.load()
    pred, gt, valid = _maps(3, 300, 1, "half")
    p, g, v = _dev(pred), _dev(gt), _dev(valid)
    (count, _), (med, _), (mws, _) = _g((3,), torch.int64), _g((3, 2, 2), torch.float32), _g((ops.deptheval_median_workspace_bytes(3, 300),), torch.uint8)
    (counts, _), (sums, _), (sws, _) = _g((3, 4), torch.int64), _g((3, 5), torch.float64), _g((ops.deptheval_sums_workspace_bytes(3, 300),), torch.uint8)
    (coeff, _), (status, _) = _g((3, 2), torch.float64), _g((3,), torch.int32)
    outs = (count, med, mws, counts, sums, sws, coeff, status)
    cin = _dev(np.tile([1.0, 0.0], (3, 1)))
    nan = float("nan")
    st = torch.cuda.current_stream().cuda_stream

    def median(**kw):
        q = L.DepthEvalMedianParams(pred=p.data_ptr(), gt=g.data_ptr(), valid=v.data_ptr(), groups=3, n=300, stride=300, min_depth=0.0,
                                    max_depth=float("inf"), ws=mws.data_ptr(), ws_bytes=mws.numel(), out_count=count.data_ptr(), out_median=med.data_ptr())
        for k, x in kw.items():
            setattr(q, k, x)
        return lib.ovg_deptheval_median(ctypes.byref(q), st)

    def sums_(**kw):
        q = L.DepthEvalSumsParams(pred=p.data_ptr(), gt=g.data_ptr(), valid=v.data_ptr(), groups=3, n=300, stride=300, min_depth=0.0,
                                  max_depth=float("inf"), mode=L.DEPTHEVAL_METRICS, coeff=cin.data_ptr(), clip_min=1e-3, clip_max=float("inf"),
                                  ws=sws.data_ptr(), ws_bytes=sws.numel(), out_counts=counts.data_ptr(), out_sums=sums.data_ptr())
        for k, x in kw.items():
            setattr(q, k, x)
        return lib.ovg_deptheval_sums(ctypes.byref(q), st)

    def solve(**kw):
        q = L.DepthEvalSolveParams(count=counts.data_ptr(), count_stride=4, sums=sums.data_ptr(), median=med.data_ptr(), groups=3,
                                   mode=L.DEPTHEVAL_SCALE_SHIFT, coeff=coeff.data_ptr(), status=status.data_ptr())
        for k, x in kw.items():
            setattr(q, k, x)
        return lib.ovg_deptheval_solve(ctypes.byref(q), st)

    shared = (dict(pred=None), dict(gt=None), dict(ws=None), dict(groups=0), dict(groups=4097), dict(n=0), dict(n=1 << 31), dict(stride=299),
              dict(min_depth=nan), dict(min_depth=-1.0), dict(max_depth=nan), dict(pred=p.data_ptr() + 2), dict(gt=g.data_ptr() + 1),
              dict(ws_bytes=255), dict(ws_bytes=0))
    for bad in shared + (dict(out_count=None), dict(out_median=None), dict(ws=mws.data_ptr() + 8), dict(out_count=count.data_ptr() + 4)):
        assert median(**bad) == -1, bad
    for bad in shared + (dict(out_counts=None), dict(out_sums=None), dict(ws=sws.data_ptr() + 8), dict(mode=2), dict(coeff=None), dict(clip_min=0.0),
                         dict(clip_min=nan), dict(clip_max=nan), dict(clip_max=1e-4), dict(out_sums=sums.data_ptr() + 4)):
        assert sums_(**bad) == -1, bad
    for bad in (dict(count=None), dict(coeff=None), dict(status=None), dict(count_stride=0), dict(groups=0), dict(groups=4097), dict(mode=4), dict(mode=-1),
                dict(sums=None), dict(mode=L.DEPTHEVAL_MEDIAN, median=None), dict(coeff=coeff.data_ptr() + 4), dict(status=status.data_ptr() + 2)):
        assert solve(**bad) == -1, bad
    torch.cuda.synchronize()
    for o in outs:
        assert bool((o.contiguous().view(torch.uint8) == GUARD_BYTE).all())
    assert median() == 0 and sums_() == 0 and solve() == 0                    # the same structs without the fault are accepted
    torch.cuda.synchronize()


# ---------------------------------------------------------------------------------------------
# poses
# ---------------------------------------------------------------------------------------------
def _rot(axis, deg):
    a = np.asarray(axis, np.float64) / np.linalg.norm(axis)
    K = np.array([[0, -a[2], a[1]], [a[2], 0, -a[0]], [-a[1], a[0], 0]])
    t = np.deg2rad(deg)
    return np.eye(3) + np.sin(t) * K + (1 - np.cos(t)) * K @ K


def _rig(S, seed, wobble):
    """S cameras on a circle of radius 3 looking at the origin; wobble: each turned by up to that many degrees about a random axis and
    moved by up to 0.4 -- the predicted rig."""
    rng = np.random.default_rng(seed)
    E = np.zeros((S, 3, 4))
    for k in range(S):
        a = 2 * np.pi * k / S
        c = np.array([3 * np.cos(a), 0.5 * np.sin(2 * a), 3 * np.sin(a)])
        z = -c / np.linalg.norm(c)
        x = np.cross([0, 1, 0], z)
        x /= np.linalg.norm(x)
        R = np.stack([x, np.cross(z, x), z])
        if wobble:
            R = _rot(rng.normal(size=3), rng.uniform(0.5, wobble)) @ R
            c = c + rng.uniform(-0.4, 0.4, 3)
        E[k, :, :3], E[k, :, 3] = R, -R @ c
    return E


@pytest.mark.parametrize("S", [2, 5, 16])
def test_pose_errors_and_auc_match_the_twin(S):
    gt, pred = _rig(S, S, 0.0), _rig(S, S, 25.0)
    w_rot, w_trans = twin.relative_pose_errors(pred, gt)
    both = np.concatenate([w_rot, w_trans])
    assert (np.abs(both - np.round(both)) > 1e-6).all() and w_rot.max() > 1.0    # no error sits on a threshold: exact counts are a fair demand
    want = twin.pose_auc(w_rot, w_trans)
    for rep in range(2):
        for dt, form in ((torch.float64, 3), (torch.float64, 4), (torch.float32, 3)):
            P, Gt = pred.astype(F).astype(np.float64), gt.astype(F).astype(np.float64)         # what both sides see in the float32 form
            if dt == torch.float64:
                P, Gt = pred, gt
            wr, wt = twin.relative_pose_errors(P, Gt)
            ep, eg = (torch.from_numpy(np.concatenate([e, np.tile([[[0, 0, 0, 1.0]]], (S, 1, 1))], 1)[:, :form]).to(dt).cuda() for e in (P, Gt))
            rot, trans = postprocess.relative_pose_errors(ep, eg)
            assert rot.dtype == trans.dtype == torch.float64 and rot.shape == trans.shape == (S * (S - 1) // 2,)
            assert np.abs(rot.cpu().numpy() - wr).max() <= 1e-9 and np.abs(trans.cpu().numpy() - wt).max() <= 1e-9
            if dt == torch.float64:
                assert postprocess.pose_auc(rot, trans) == want
                assert postprocess.pose_auc(rot.float(), trans, thresholds=[30, 5]) == {k: v for k, v in want.items() if not k.endswith("@15")}
    zero = postprocess.relative_pose_errors(torch.from_numpy(gt).cuda(), torch.from_numpy(gt).cuda())
    assert float(zero[0].abs().max()) <= 1e-9 and float(zero[1].abs().max()) <= 1e-9
    assert postprocess.pose_auc(*zero)["AUC@30"] == 1.0


def test_evaluate_predictions_is_the_glue():
    S, H, W = 4, 14, 18
    rng = np.random.default_rng(4)
    gt = rng.uniform(0.5, 8.0, (S, H, W)).astype(F)
    depth = torch.from_numpy((gt * 0.5).astype(F))[None, ..., None].cuda()
    E = torch.from_numpy(_rig(S, 1, 0.0)).cuda()
    out = postprocess.evaluate_predictions({"depth": depth, "extrinsic": E[None].float()}, gt_depth=_dev(gt), gt_extrinsic=E, align="scale", thresholds=(5,))
    assert sorted(out) == ["depth", "pose", "rot_err", "trans_err"] and out["depth"].scale.tolist() == [2.0] * S and out["depth"].mean["abs_rel"] == 0.0
    assert out["pose"]["AUC@5"] == 1.0 and sorted(out["pose"]) == ["AUC@5", "Acc@5", "RRA@5", "RTA@5"]
    enc = torch.zeros(1, S, 9, device="cuda")
    enc[..., 6] = 1.0                                                         # identity quaternions (x, y, z, w)
    enc[0, :, 0] = torch.arange(S, device="cuda")
    only_pose = postprocess.evaluate_predictions({"pose_enc": enc}, gt_extrinsic=E)
    assert sorted(only_pose) == ["pose", "rot_err", "trans_err"] and only_pose["rot_err"].shape == (6,) and float(only_pose["rot_err"].max()) > 10.0
    assert sorted(postprocess.evaluate_predictions({"depth": depth}, gt_depth=_dev(gt[..., None]), gt_valid=_dev(gt > 1))) == ["depth"]


# ---------------------------------------------------------------------------------------------
# the stream and no-sync contract of the three entries (recorded for test_gpu_stream_contract's coverage test)
# ---------------------------------------------------------------------------------------------
def test_depth_evaluation_entries_are_gated():
    G, n = 3, 2049
    real, decoy = _maps(G, n, 800, "half"), _maps(G, n, 801, "half")
    t = lambda a: torch.from_numpy(a)

    def inputs(c):
        return c.inp(t(real[0]), t(decoy[0])), c.inp(t(real[1]), t(decoy[1])), c.inp(t(real[2]), t(decoy[2]))

    def median_case():
        c = sc.Case("deptheval_median 3 x 2049, half masked")
        p, g, v = inputs(c)
        ws, count, med = c.ws(ops.deptheval_median_workspace_bytes(G, n)), c.out((G,), torch.int64), c.out((G, 2, 2), torch.float32)
        c.call = lambda: ops.deptheval_median(p, g, v, 0.5, 8.0, ws=ws, count=count, median=med)
        return c

    def moments_case():
        c = sc.Case("deptheval_sums moments 3 x 2049")
        p, g, v = inputs(c)
        ws, counts, sums = c.ws(ops.deptheval_sums_workspace_bytes(G, n)), c.out((G, 4), torch.int64), c.out((G, 5), torch.float64)
        c.call = lambda: ops.deptheval_sums(p, g, v, 0.5, 8.0, ws=ws, counts=counts, sums=sums)
        return c

    def metrics_case():
        c = sc.Case("deptheval_sums metrics 3 x 2049")
        p, g, v = inputs(c)
        coeff = c.inp(t(np.array([[0.6, -0.1], [0.55, 0.0], [0.5, 0.2]])), t(np.array([[0.5, 0.1], [0.6, -0.2], [0.58, 0.0]])))
        ws, counts, sums = c.ws(ops.deptheval_sums_workspace_bytes(G, n)), c.out((G, 4), torch.int64), c.out((G, 5), torch.float64)
        c.call = lambda: ops.deptheval_sums(p, g, v, 0.5, 8.0, coeff=coeff, clip_min=1e-3, clip_max=20.0, ws=ws, counts=counts, sums=sums)
        return c

    def solve_case():
        c = sc.Case("deptheval_solve scale and shift, 3 groups")
        ma, mb = twin.sums(*real, 0.5, 8.0), twin.sums(*decoy, 0.5, 8.0)
        counts, sums = c.inp(t(ma[0]), t(mb[0])), c.inp(t(ma[1]), t(mb[1]))
        coeff, status = c.out((G, 2), torch.float64), c.out((G,), torch.int32)
        c.call = lambda: ops.deptheval_solve(L.DEPTHEVAL_SCALE_SHIFT, counts, sums=sums, coeff=coeff, status=status)
        return c

    cases = tsc.family([median_case, moments_case, metrics_case, solve_case], "depth evaluation")
    assert {e for c in cases for e in c.entries} == {"ovg_deptheval_median", "ovg_deptheval_sums", "ovg_deptheval_solve"}
    assert all(e in tsc.COVERED for e in ("ovg_deptheval_median", "ovg_deptheval_sums", "ovg_deptheval_solve"))
