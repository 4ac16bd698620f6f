"""Depth evaluation (ovg_deptheval_median / ovg_deptheval_sums / ovg_deptheval_solve), host side: the numpy twin
(tests/deptheval_twin.py) against plain formulations that share no code with it (np.median, np.linalg.lstsq, np.sum of the textbook
metric formulas), the C ABI without a device (struct layouts, enums, every argument check that returns before a launch), the Python
layers' argument checks, the degenerate groups, and the pose figures on cases worked out by hand."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

import abi_layout
import common
import deptheval_twin as twin
from omnivggt_official_amd import lib as L
from omnivggt_official_amd import ops, postprocess

HEADER = os.path.join(common.ROOT, "include", "omnivggt_hip.h")
F = np.float32


def _maps(G, n, seed, shifted=True):
    rng = np.random.default_rng(seed)
    gt = rng.uniform(0.5, 8.0, (G, n)).astype(F)
    pred = (gt * (1 + 0.1 * rng.normal(size=(G, n))) * 1.7 + (0.3 if shifted else 0.0)).astype(F)
    return pred, gt, rng


# ---------------------------------------------------------------------------------------------
# the twin against independent formulations
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [1, 2, 255, 1025, 5000])
def test_twin_median_is_numpys_median(n):
    pred, gt, rng = _maps(3, n, n)
    valid = (rng.random((3, n)) < 0.5).astype(np.uint8)
    valid[:, 0] = 1
    pred[1, n // 2], gt[2, n - 1] = np.nan, np.inf
    for v in (None, valid):
        count, med = twin.median(pred, gt, v, 0.6, 7.5)
        use = twin.used(pred, gt, v, 0.6, 7.5)
        for k in range(3):
            assert count[k] == use[k].sum()
            if count[k] == 0:
                assert med[k].tobytes() == np.zeros((2, 2), F).tobytes()
                continue
            for m, x in enumerate((pred, gt)):
                want = np.median(x[k][use[k]].astype(np.float64))
                got = 0.5 * (float(med[k, m, 0]) + float(med[k, m, 1]))
                assert abs(got - want) <= 1e-12 * abs(want), (n, k, m, got, want)
                assert med[k, m, 0] <= med[k, m, 1] and (count[k] % 2 == 0 or med[k, m, 0] == med[k, m, 1])


@pytest.mark.parametrize("n", [2, 257, 1024, 2049, 300000])
def test_twin_sums_and_solve_against_lstsq_and_textbook_metrics(n):
    pred, gt, rng = _maps(2, n, n + 1)
    valid = (rng.random((2, n)) < 0.5).astype(np.uint8)
    valid[:, :2] = 1
    if n > 2:
        pred[0, 2], gt[1, 2] = -1.0, np.nan
    use = twin.used(pred, gt, valid)
    counts, mom = twin.sums(pred, gt, valid)
    assert (counts[:, 1:] == 0).all()
    count_m, med = twin.median(pred, gt, valid)
    assert (count_m == counts[:, 0]).all()
    for k in range(2):
        p, g = pred[k][use[k]].astype(np.float64), gt[k][use[k]].astype(np.float64)
        want = np.array([p.sum(), g.sum(), (p * p).sum(), (p * g).sum(), (g * g).sum()])
        assert np.abs(mom[k] - want).max() <= 1e-12 * np.abs(want).max()
        ref = {twin.NONE: (1.0, 0.0), twin.MEDIAN: (np.median(g) / np.median(p), 0.0),
               twin.SCALE: (np.linalg.lstsq(p[:, None], g, rcond=None)[0][0], 0.0),
               twin.SCALE_SHIFT: tuple(np.linalg.lstsq(np.stack([p, np.ones_like(p)], 1), g, rcond=None)[0])}
        for mode, (s, t) in ref.items():
            coeff, status = twin.solve(mode, counts, mom, med)
            assert status[k] == 0 and abs(coeff[k, 0] - s) <= 1e-10 * abs(s) and abs(coeff[k, 1] - t) <= 1e-10 * max(abs(t), 1.0), (mode, coeff[k], s, t)
            # the textbook metrics under the twin's own coefficients
            c2, met = twin.sums(pred, gt, valid, mode=twin.METRICS, coeff=coeff, clip_min=1e-3, clip_max=50.0)
            q = np.clip(coeff[k, 0] * p + coeff[k, 1], 1e-3, 50.0)
            want = np.array([np.sum(np.abs(q - g) / g), np.sum((q - g) ** 2 / g), np.sum((q - g) ** 2), np.sum(np.abs(q - g)),
                             np.sum((np.log(q) - np.log(g)) ** 2)])
            assert (np.abs(met[k] - want) <= 1e-12 * np.abs(want)).all(), (mode, met[k], want)
            ratio = np.maximum(q / g, g / q)
            assert c2[k].tolist() == [len(p)] + [int((ratio < d).sum()) for d in twin.DELTAS]
            fig = twin.figures(c2, met)
            assert abs(fig["abs_rel"][k] - np.mean(np.abs(q - g) / g)) <= 1e-12 and abs(fig["rmse"][k] - np.sqrt(np.mean((q - g) ** 2))) <= 1e-12
            assert abs(fig["delta1"][k] - np.mean(ratio < 1.25)) <= 1e-15


def test_twin_predicate_edges_and_strict_deltas():
    tiny = np.array([1e-45], F)[0]                                            # the smallest subnormal: positive, so used
    pred = np.array([[1.0, 0.0, -1.0, tiny, np.nan, np.inf, -np.inf, 2.0, 2.0, 2.0]], F)
    gt = np.array([[1.0, 1.0, 1.0, 1.0, 1.0, 1.0, 1.0, 0.5, 4.0, np.nan]], F)
    assert twin.used(pred, gt, None, 0.5, 4.0)[0].tolist() == [True, False, False, True, False, False, False, False, True, False]
    assert twin.used(pred, gt, np.array([[0] + [1] * 9], np.uint8), 0.5, 4.0)[0].tolist()[:4] == [False, False, False, True]
    # ratios of exactly 1.25, 1.25^2, 1.25^3 are NOT below their thresholds; one ulp less is
    q = np.array([[1.25, 1.5625, 1.953125, np.nextafter(F(1.25), F(0)), 1.0 / 1.25]], F)
    counts, _ = twin.sums(q, np.ones_like(q), mode=twin.METRICS, coeff=np.array([[1.0, 0.0]]))
    assert counts[0].tolist() == [5, 2, 3, 4]                                 # f32(0.8) lies above 0.8: its ratio 1 / q is just below 1.25


def test_twin_degenerate_groups_are_identity_with_the_right_bit():
    one, zero = np.array([1], np.int64), np.array([0], np.int64)
    m = np.array([[2.0, 4.0, 4.0, 8.0, 16.0]])                                # one pixel p = 2, g = 4
    med = np.array([[[2.0, 2.0], [4.0, 4.0]]], F)
    ident = [[1.0, 0.0]]
    for mode in (twin.NONE, twin.MEDIAN, twin.SCALE, twin.SCALE_SHIFT):
        c, s = twin.solve(mode, zero, np.zeros((1, 5)), np.zeros((1, 2, 2), F))
        assert c.tolist() == ident and s.tolist() == [twin.FEW], mode
    assert [twin.solve(mode, one, m, med)[0].tolist() for mode in (twin.NONE, twin.MEDIAN, twin.SCALE)] == [ident, [[2.0, 0.0]], [[2.0, 0.0]]]
    assert twin.solve(twin.SCALE_SHIFT, one, m, med)[1].tolist() == [twin.FEW]                 # a line needs two points
    for k, v in ((0, np.inf), (3, np.nan), (4, -np.inf)):
        bad = m.copy()
        bad[0, k] = v
        for mode in (twin.SCALE, twin.SCALE_SHIFT):
            c, s = twin.solve(mode, np.array([5]), bad)
            assert c.tolist() == ident and s.tolist() == [twin.NOT_FINITE]
        assert twin.solve(twin.NONE, np.array([5]), bad)[1].tolist() == [0]                    # NONE reads no sum
    assert twin.solve(twin.MEDIAN, one, med=np.array([[[np.inf, 2.0], [4.0, 4.0]]], F))[1].tolist() == [twin.NOT_FINITE]
    assert twin.solve(twin.SCALE_SHIFT, zero, np.full((1, 5), np.nan))[1].tolist() == [twin.FEW | twin.NOT_FINITE]
    # all pred equal: no spread for the line, a regular fit through the origin
    p, g = np.full((1, 300), 2.0, F), np.linspace(1, 3, 300, dtype=F)[None]
    counts, mom = twin.sums(p, g)
    c, s = twin.solve(twin.SCALE_SHIFT, counts, mom)
    assert c.tolist() == ident and s.tolist() == [twin.NO_SPREAD]
    assert twin.solve(twin.SCALE, counts, mom)[1].tolist() == [0]
    # a falling line: s <= 0 is a bad fit, never a negative scale
    p = np.linspace(1, 3, 300, dtype=F)[None]
    counts, mom = twin.sums(p, (4.0 - p).astype(F))
    c, s = twin.solve(twin.SCALE_SHIFT, counts, mom)
    assert c.tolist() == ident and s.tolist() == [twin.BAD_FIT]
    assert twin.solve(twin.MEDIAN, one, med=np.zeros((1, 2, 2), F))[1].tolist() == [twin.BAD_FIT]      # 0 / 0
    assert not np.isnan(np.concatenate([twin.solve(mo, one, np.full((1, 5), 1e308), med)[0].ravel() for mo in range(4)])).any()


# ---------------------------------------------------------------------------------------------
# the C ABI without a device
# ---------------------------------------------------------------------------------------------
def _layout(struct, cname, extra):
    enums, (eps,) = abi_layout.check({cname: struct}, extra, ["OVG_DEPTHEVAL_SPREAD_EPS"])
    assert eps == L.DEPTHEVAL_SPREAD_EPS == twin.SPREAD_EPS == 2.0 ** -40
    return enums


def test_ctypes_struct_layouts_and_enums_match_c_deptheval():
    names = ["OVG_DEPTHEVAL_THREADS", "OVG_DEPTHEVAL_TILE", "OVG_DEPTHEVAL_SUMS", "OVG_DEPTHEVAL_COUNTS", "OVG_DEPTHEVAL_PARTIAL_BYTES",
             "OVG_DEPTHEVAL_MAX_GROUPS", "OVG_DEPTHEVAL_CHUNK", "OVG_DEPTHEVAL_MEDIAN_GROUP_BYTES", "OVG_ABI_VERSION"]
    want = [L.DEPTHEVAL_THREADS, L.DEPTHEVAL_TILE, L.DEPTHEVAL_SUMS, L.DEPTHEVAL_COUNTS, L.DEPTHEVAL_PARTIAL_BYTES, L.DEPTHEVAL_MAX_GROUPS,
            L.DEPTHEVAL_CHUNK, L.DEPTHEVAL_MEDIAN_GROUP_BYTES, L.ABI_VERSION]
    assert _layout(L.DepthEvalMedianParams, "ovg_deptheval_median_params", names) == want
    assert _layout(L.DepthEvalSumsParams, "ovg_deptheval_sums_params", ["OVG_DEPTHEVAL_MOMENTS", "OVG_DEPTHEVAL_METRICS"]) == \
        [L.DEPTHEVAL_MOMENTS, L.DEPTHEVAL_METRICS] == [twin.MOMENTS, twin.METRICS]
    modes = ["OVG_DEPTHEVAL_NONE", "OVG_DEPTHEVAL_MEDIAN", "OVG_DEPTHEVAL_SCALE", "OVG_DEPTHEVAL_SCALE_SHIFT", "OVG_DEPTHEVAL_FEW",
             "OVG_DEPTHEVAL_NOT_FINITE", "OVG_DEPTHEVAL_NO_SPREAD", "OVG_DEPTHEVAL_BAD_FIT"]
    assert _layout(L.DepthEvalSolveParams, "ovg_deptheval_solve_params", modes) == \
        [L.DEPTHEVAL_NONE, L.DEPTHEVAL_MEDIAN, L.DEPTHEVAL_SCALE, L.DEPTHEVAL_SCALE_SHIFT, L.DEPTHEVAL_FEW, L.DEPTHEVAL_NOT_FINITE,
         L.DEPTHEVAL_NO_SPREAD, L.DEPTHEVAL_BAD_FIT] == \
        [twin.NONE, twin.MEDIAN, twin.SCALE, twin.SCALE_SHIFT, twin.FEW, twin.NOT_FINITE, twin.NO_SPREAD, twin.BAD_FIT]
    assert (L.DEPTHEVAL_THREADS, L.DEPTHEVAL_TILE, L.DEPTHEVAL_SUMS, L.DEPTHEVAL_COUNTS) == (twin.THREADS, twin.TILE, twin.SUMS, twin.COUNTS)
    assert L.DEPTHEVAL_PARTIAL_BYTES >= 8 * (L.DEPTHEVAL_SUMS + L.DEPTHEVAL_COUNTS) and L.DEPTHEVAL_MEDIAN_GROUP_BYTES == 4 * (4 * 256 + 8)
    assert (postprocess.DEPTH_FEW, postprocess.DEPTH_NOT_FINITE, postprocess.DEPTH_NO_SPREAD, postprocess.DEPTH_BAD_FIT) == (1, 2, 4, 8)
    assert postprocess.DEPTH_ALIGNMENTS == {"none": 0, "median": 1, "scale": 2, "scale_shift": 3}
    text = open(HEADER).read()
    for entry in ("ovg_deptheval_median", "ovg_deptheval_sums", "ovg_deptheval_solve"):
        assert re.search(r"int\s+%s\s*\(\s*const\s+%s_params\s*\*\s*,\s*void\s*\*\s*stream\s*\)\s*;" % (entry, entry), text)
        assert entry in L.SYMBOLS
    for q in ("ovg_deptheval_median_workspace_bytes", "ovg_deptheval_sums_workspace_bytes"):
        assert re.search(r"int64_t\s+%s\s*\(\s*int64_t\s+groups\s*,\s*int64_t\s+n\s*\)\s*;" % q, text) and q in L.SYMBOLS
        assert text.index(q) < text.index("#define OVG_ABI_VERSION")                           # named in the ABI-13 list
    assert L.load().ovg_abi_version() == 13


def test_argument_validation_of_the_three_entries_without_gpu():
    lib = L.load()
    mws, sws = lib.ovg_deptheval_median_workspace_bytes, lib.ovg_deptheval_sums_workspace_bytes
    assert [mws(g, n) for g, n in ((1, 1), (1, (1 << 31) - 1), (3, 2049), (64, 268324), (4096, 1000))] == [4352, 4352, 12544, 264192, 4128 * 4096]
    assert [sws(g, n) for g, n in ((1, 1), (1, 1024), (1, 1025), (3, 2049), (64, 268324))] == [256, 256, 256, 768, 64 * 263 * 80]
    for q in (mws, sws):
        assert [q(g, n) for g, n in ((0, 5), (-1, 5), (4097, 5), (1, 0), (1, -1), (1, 1 << 31), (2, 1 << 30), (4096, 1 << 19), (1 << 62, 4),
                                     (1, -(1 << 63)))] == [-1] * 10
    assert ops.deptheval_median_workspace_bytes(3, 2049) == 12544 and ops.deptheval_sums_workspace_bytes(3, 2049) == 768
    for bad in ((0, 1), (1, 0), (4097, 1), (1, 1 << 31), (1, 1 << 70)):
        with pytest.raises(L.OvgError):
            ops.deptheval_median_workspace_bytes(*bad)
        with pytest.raises(L.OvgError):
            ops.deptheval_sums_workspace_bytes(*bad)
    big = 1 << 40                                                             # fake, never dereferenced: every call below fails its checks
    nan, inf = float("nan"), float("inf")
    shared = (dict(pred=None), dict(gt=None), dict(ws=None), dict(groups=0), dict(groups=-1), dict(groups=4097), dict(n=0), dict(n=-1),
              dict(n=1 << 31, stride=1 << 31, ws_bytes=1 << 50), dict(groups=4096, n=1 << 19, stride=1 << 19, ws_bytes=1 << 50),
              dict(stride=4999), dict(stride=0), dict(stride=-5000), dict(stride=1 << 39), dict(min_depth=nan), dict(min_depth=-1.0),
              dict(min_depth=-inf), dict(max_depth=nan), dict(pred=big + 2), dict(gt=big + 1), dict(ws=big + 8), dict(ws=big + 4),
              dict(ws_bytes=0), dict(ws_bytes=-256))

    def median(**kw):
        p = L.DepthEvalMedianParams(pred=big, gt=big, valid=big + 1, groups=3, n=5000, stride=5000, min_depth=0.0, max_depth=inf, ws=big,
                                    ws_bytes=mws(3, 5000), out_count=big, out_median=big)
        for k, v in kw.items():
            setattr(p, k, v)
        return lib.ovg_deptheval_median(ctypes.byref(p), None)

    assert lib.ovg_deptheval_median(None, None) == -1
    for bad in shared + (dict(out_count=None), dict(out_median=None), dict(out_count=big + 4), dict(out_median=big + 2),
                         dict(ws_bytes=mws(3, 5000) - 1)):
        assert median(**bad) == -1, bad

    def sums(**kw):
        p = L.DepthEvalSumsParams(pred=big, gt=big, valid=big + 3, groups=3, n=5000, stride=5000, min_depth=0.0, max_depth=inf,
                                  mode=L.DEPTHEVAL_METRICS, coeff=big, clip_min=1e-3, clip_max=inf, ws=big, ws_bytes=sws(3, 5000),
                                  out_counts=big, out_sums=big)
        for k, v in kw.items():
            setattr(p, k, v)
        return lib.ovg_deptheval_sums(ctypes.byref(p), None)

    assert lib.ovg_deptheval_sums(None, None) == -1
    for bad in shared + (dict(out_counts=None), dict(out_sums=None), dict(out_counts=big + 4), dict(out_sums=big + 4), dict(coeff=big + 4),
                         dict(ws_bytes=sws(3, 5000) - 1), dict(mode=2), dict(mode=-1), dict(coeff=None), dict(clip_min=0.0), dict(clip_min=-1.0),
                         dict(clip_min=nan), dict(clip_min=inf), dict(clip_max=nan), dict(clip_max=1e-4), dict(clip_max=-inf)):
        assert sums(**bad) == -1, bad
    for bad in (dict(mode=L.DEPTHEVAL_MOMENTS, out_sums=None), dict(mode=L.DEPTHEVAL_MOMENTS, n=0)):
        assert sums(**bad) == -1, bad

    def solve(**kw):
        p = L.DepthEvalSolveParams(count=big, count_stride=4, sums=big, median=big + 4, groups=3, mode=L.DEPTHEVAL_SCALE_SHIFT, coeff=big,
                                   status=big + 4)
        for k, v in kw.items():
            setattr(p, k, v)
        return lib.ovg_deptheval_solve(ctypes.byref(p), None)

    assert lib.ovg_deptheval_solve(None, None) == -1
    for bad in (dict(count=None), dict(coeff=None), dict(status=None), dict(count_stride=0), dict(count_stride=-4), dict(groups=0),
                dict(groups=4097), dict(groups=-3), dict(mode=4), dict(mode=-1), dict(sums=None), dict(mode=L.DEPTHEVAL_SCALE, sums=None),
                dict(mode=L.DEPTHEVAL_MEDIAN, median=None), dict(count=big + 4), dict(sums=big + 4), dict(median=big + 2), dict(coeff=big + 4),
                dict(status=big + 2)):
        assert solve(**bad) == -1, bad


# ---------------------------------------------------------------------------------------------
# the Python layers
# ---------------------------------------------------------------------------------------------
def test_ops_wrappers_check_their_arguments_before_any_device_call():
    p, g = torch.ones(3, 50), torch.ones(3, 50)
    v = torch.ones(3, 50, dtype=torch.uint8)
    f64 = lambda *s: torch.zeros(*s, dtype=torch.float64)
    i64 = lambda *s: torch.zeros(*s, dtype=torch.int64)
    shared = (dict(pred=p.double()), dict(pred=torch.ones(150)), dict(pred=torch.ones(0, 50)), dict(pred=torch.ones(3, 0)),
              dict(pred=torch.ones(3, 100)[:, ::2]), dict(gt=torch.ones(3, 51)), dict(gt=torch.ones(2, 50)), dict(gt=torch.ones(3, 100)[:, :50]),
              dict(gt=[[1.0]]), dict(valid=v.bool()), dict(valid=v[:2]), dict(valid=torch.ones(3, 100, dtype=torch.uint8)[:, :50]),
              dict(min_depth=float("nan")), dict(min_depth=-0.5), dict(min_depth="0"), dict(max_depth=float("nan")), dict(max_depth=None),
              dict(ws=torch.zeros(1 << 16)), dict(pred=torch.ones(4097, 2), gt=torch.ones(4097, 2), valid=None))
    for kw in shared + (dict(count=i64(2)), dict(count=f64(3)), dict(median=torch.zeros(3, 4)), dict(median=f64(3, 2, 2))):
        with pytest.raises(L.OvgError, match="must be"):
            ops.deptheval_median(**dict(dict(pred=p, gt=g, valid=v), **kw))
    for kw in shared + (dict(coeff=f64(3)), dict(coeff=torch.zeros(3, 2)), dict(counts=i64(3)), dict(counts=i64(3, 3)), dict(sums=f64(3, 4)),
                        dict(sums=torch.zeros(3, 5)), dict(coeff=f64(3, 2), clip_min=0.0), dict(coeff=f64(3, 2), clip_min=float("nan")),
                        dict(coeff=f64(3, 2), clip_min=float("inf")), dict(coeff=f64(3, 2), clip_max=1e-4), dict(coeff=f64(3, 2), clip_max=None)):
        with pytest.raises(L.OvgError, match="must be"):
            ops.deptheval_sums(**dict(dict(pred=p, gt=g, valid=v), **kw))
    for kw in (dict(), dict(valid=None), dict(min_depth=0.5, max_depth=4.0), dict(pred=torch.ones(3, 100)[:, :50], gt=torch.ones(3, 100)[:, :50], valid=None)):
        with pytest.raises(L.OvgError, match="no CPU fallback"):
            ops.deptheval_median(**dict(dict(pred=p, gt=g, valid=v), **kw))
        with pytest.raises(L.OvgError, match="no CPU fallback"):
            ops.deptheval_sums(**dict(dict(pred=p, gt=g, valid=v), **kw))
    with pytest.raises(L.OvgError, match="no CPU fallback"):
        ops.deptheval_sums(p, g, coeff=f64(3, 2), clip_max=10.0)
    ok = dict(mode=L.DEPTHEVAL_SCALE_SHIFT, count=i64(3, 4), sums=f64(3, 5))
    for kw in (dict(mode=4), dict(mode=-1), dict(mode="median"), dict(mode=True), dict(count=i64(3, 3)), dict(count=torch.zeros(3, dtype=torch.int32)),
               dict(count=i64(0)), dict(count=i64(4097)), dict(count=i64(3, 8)[:, ::2]), dict(sums=None), dict(sums=f64(2, 5)), dict(sums=torch.zeros(3, 5)),
               dict(mode=L.DEPTHEVAL_MEDIAN), dict(mode=L.DEPTHEVAL_MEDIAN, median=torch.zeros(3, 4)), dict(coeff=f64(3)), dict(status=i64(3))):
        with pytest.raises(L.OvgError, match="must be"):
            ops.deptheval_solve(**dict(ok, **kw))
    for kw in (dict(), dict(count=i64(3)), dict(mode=L.DEPTHEVAL_NONE, sums=None), dict(mode=L.DEPTHEVAL_MEDIAN, median=torch.zeros(3, 2, 2))):
        with pytest.raises(L.OvgError, match="no CPU fallback"):
            ops.deptheval_solve(**dict(ok, **kw))


def test_public_entries_check_their_arguments_and_refuse_cpu_tensors():
    p, g = torch.ones(2, 6, 5), torch.ones(2, 6, 5, 1)
    bad_depth = (dict(pred=p.double()), dict(pred=torch.ones(6, 5)), dict(pred=torch.ones(2, 6, 5, 3)), dict(gt=torch.ones(2, 6, 4)),
                 dict(gt=torch.ones(3, 6, 5)), dict(gt=p.numpy()), dict(pred=torch.ones(0, 6, 5), gt=torch.ones(0, 6, 5)),
                 dict(valid=torch.ones(2, 6, 5)), dict(valid=torch.ones(2, 6, 4, dtype=torch.bool)), dict(valid=torch.ones(2, 30, dtype=torch.bool)),
                 dict(align="affine"), dict(align=None), dict(align=1), dict(scope="pixel"), dict(scope=None), dict(min_depth=-1.0),
                 dict(min_depth=float("nan")), dict(min_depth="0"), dict(max_depth=float("nan")), dict(max_depth=None), dict(min_depth=True))
    for fn in (postprocess.align_depth, postprocess.depth_metrics):
        for kw in bad_depth:
            with pytest.raises(ValueError):
                fn(**dict(dict(pred=p, gt=g), **kw))
        for kw in (dict(), dict(valid=torch.ones(2, 6, 5, dtype=torch.bool)), dict(valid=torch.ones(2, 6, 5, 1, dtype=torch.uint8)), dict(align="none"),
                   dict(align="scale"), dict(align="scale_shift", scope="sequence"), dict(min_depth=0.1, max_depth=80.0)):
            with pytest.raises(L.OvgError, match="no CPU fallback"):
                fn(**dict(dict(pred=p, gt=g), **kw))
    for kw in (dict(clip_min=0.0), dict(clip_min=-1e-3), dict(clip_min=float("nan")), dict(clip_min=float("inf")), dict(clip_min=None),
               dict(clip_max=1e-4), dict(clip_max=float("nan")), dict(clip_max="10"), dict(clip_min=True)):
        with pytest.raises(ValueError):
            postprocess.depth_metrics(p, g, **kw)
    with pytest.raises(L.OvgError, match="no CPU fallback"):
        postprocess.depth_metrics(p, g, clip_min=1e-2, clip_max=100.0)
    e = torch.eye(4)[None].repeat(3, 1, 1)
    for kw in (dict(gt_extrinsic=e[:2]), dict(pred_extrinsic=e[0]), dict(pred_extrinsic=e[:, :2]), dict(pred_extrinsic=e.half()),
               dict(pred_extrinsic=e.numpy()), dict(pred_extrinsic=e[:1], gt_extrinsic=e[:1]), dict(pred_extrinsic=e[:0], gt_extrinsic=e[:0])):
        with pytest.raises(ValueError):
            postprocess.relative_pose_errors(**dict(dict(pred_extrinsic=e, gt_extrinsic=e[:, :3]), **kw))
    with pytest.raises(L.OvgError, match="no CPU fallback"):
        postprocess.relative_pose_errors(e, e[:, :3].double())
    r = torch.zeros(3, dtype=torch.float64)
    for kw in (dict(rot_err=r[:2]), dict(rot_err=r[:0], trans_err=r[:0]), dict(rot_err=r.long()), dict(trans_err=[0.0] * 3), dict(rot_err=r[None]),
               dict(thresholds=()), dict(thresholds=5), dict(thresholds=(5.0,)), dict(thresholds=(0,)), dict(thresholds=(5, 181)), dict(thresholds=(True,))):
        with pytest.raises(ValueError):
            postprocess.pose_auc(**dict(dict(rot_err=r, trans_err=r), **kw))
    with pytest.raises(L.OvgError, match="no CPU fallback"):
        postprocess.pose_auc(r, r.float())
    pred = {"depth": g[None], "pose_enc": torch.zeros(1, 2, 9)}
    for args, kw in (((pred,), {}), (([],), dict(gt_depth=g)), ((pred,), dict(gt_depth=g, colour=1)), (({},), dict(gt_depth=g)),
                     (({"depth": g[None]},), dict(gt_extrinsic=e[:2])), ((pred,), dict(gt_depth=g, align="affine")),
                     ((pred,), dict(gt_extrinsic=e[:2], thresholds=(0,)))):
        with pytest.raises((ValueError, L.OvgError)) as info:
            postprocess.evaluate_predictions(*args, **kw)
        assert isinstance(info.value, ValueError) or "no CPU fallback" in str(info.value)
    with pytest.raises(L.OvgError, match="no CPU fallback"):
        postprocess.evaluate_predictions(pred, gt_depth=g)
    with pytest.raises(L.OvgError, match="no CPU fallback"):
        postprocess.evaluate_predictions(pred, gt_extrinsic=e[:2])


# ---------------------------------------------------------------------------------------------
# poses, in numpy
# ---------------------------------------------------------------------------------------------
def _rot(axis, deg):
    a = np.asarray(axis, np.float64) / np.linalg.norm(axis)
    K = np.array([[0, -a[2], a[1]], [a[2], 0, -a[0]], [-a[1], a[0], 0]])
    t = np.deg2rad(deg)
    return np.eye(3) + np.sin(t) * K + (1 - np.cos(t)) * K @ K


def _rig(S, seed):
    rng = np.random.default_rng(seed)
    E = np.zeros((S, 3, 4))
    for k in range(S):
        E[k, :, :3] = _rot(rng.normal(size=3), rng.uniform(-40, 40))
        E[k, :, 3] = rng.normal(size=3) + [0, 0, 3]
    return E


def test_twin_relative_pose_errors_known_cases():
    E = _rig(6, 0)
    rot, trans = twin.relative_pose_errors(E, E)
    assert rot.shape == trans.shape == (15,) and np.abs(rot).max() <= 1e-9 and np.abs(trans).max() <= 1e-9
    # camera 1 turned by 10 degrees about an axis, in its own frame: every pair with it is off by 10 degrees, the others by 0
    P = E.copy()
    P[1, :, :3] = _rot([1, 2, 3], 10.0) @ E[1, :, :3]
    P[1, :, 3] = _rot([1, 2, 3], 10.0) @ E[1, :, 3]
    rot, _ = twin.relative_pose_errors(P, E)
    i, j = np.triu_indices(6, 1)
    assert np.abs(rot - np.where((i == 1) | (j == 1), 10.0, 0.0)).max() <= 1e-9
    # a similarity of the world, x_new = s Q x + c, applied to every predicted camera: E' = E S^-1 (no longer a rigid matrix)
    Q, s, c = _rot([0.3, -1, 2], 77.0), 3.7, np.array([4.0, -2.0, 9.0])
    Sinv = np.eye(4)
    Sinv[:3, :3], Sinv[:3, 3] = Q.T / s, -(Q.T / s) @ c
    P2 = np.stack([np.concatenate([e, [[0, 0, 0, 1]]]) @ Sinv for e in _rig(6, 1)])
    base = twin.relative_pose_errors(_rig(6, 1), E)
    moved = twin.relative_pose_errors(P2, E)
    assert max(np.abs(base[0] - moved[0]).max(), np.abs(base[1] - moved[1]).max()) <= 1e-9 and base[0].min() > 1.0
    # translation direction: opposite directions fold to 0, perpendicular ones give 90, a vanishing baseline gives 0
    A = np.tile(np.concatenate([np.eye(3), np.zeros((3, 1))], 1), (2, 1, 1))
    B = A.copy()
    A[1, :, 3], B[1, :, 3] = [1, 0, 0], [-2, 0, 0]
    assert np.abs(twin.relative_pose_errors(A, B)[1]).max() <= 1e-9
    B[1, :, 3] = [0, 3, 0]
    assert abs(twin.relative_pose_errors(A, B)[1][0] - 90.0) <= 1e-9
    B[1, :, 3] = [1, 1, 0]
    assert abs(twin.relative_pose_errors(A, B)[1][0] - 45.0) <= 1e-9
    B[1, :, 3] = [0, 1e-13, 0]
    assert twin.relative_pose_errors(A, B)[1][0] == 0.0


def test_twin_pose_auc_worked_by_hand_on_five_pairs():
    rot = np.array([0.5, 2.5, 4.0, 12.0, 40.0])
    trans = np.array([1.5, 0.2, 20.0, 3.0, 1.0])
    # larger error per pair: 1.5, 2.5, 20, 12, 40 -> pairs below d = 1, 2, 3 ..: 0, 1, 2, 2, 2 | 2 x 7 (d = 6 .. 12), 3 x 2 (13, 14), 3 (15) | ...
    out = twin.pose_auc(rot, trans, (5, 15, 30))
    assert (out["RRA@5"], out["RTA@5"], out["Acc@5"]) == (3 / 5, 4 / 5, 2 / 5)
    assert (out["RRA@15"], out["RTA@15"], out["Acc@15"]) == (4 / 5, 4 / 5, 3 / 5)
    assert (out["RRA@30"], out["RTA@30"], out["Acc@30"]) == (4 / 5, 1.0, 4 / 5)
    assert out["AUC@5"] == (0 + 1 + 2 + 2 + 2) / 25
    assert out["AUC@15"] == (7 + 2 * 7 + 3 * 3) / 75                          # d = 13, 14, 15 see three pairs (12 < 13)
    assert out["AUC@30"] == (7 + 2 * 7 + 3 * 8 + 4 * 10) / 150               # d = 13 .. 20: three pairs, d = 21 .. 30: four
