"""-m gpu: the kernels behind the DPT heads where they are most intricate, under the two gates of test_gpu_edges.py (whose helpers this file
uses) -- the fused output stage (csrc/ovg_dpt_tail.h) with many tiles per workgroup, in every form its entry accepts and at its geometry
edges, against kernel_guards.dpt_tail_budget; the 256-pixel LDS-DMA convolutions (csrc/ovg_conv256.h) at ragged sizes, with images smaller
than a tile, strided sources and every length class of their k loop; ovg_camera_tables with its encoding read back. Outputs sit inside guard
bands, everything a kernel must not depend on is poisoned and the poisoned run is compared bit for bit with the zero-padded one."""
import pytest
import torch

import kernel_guards as kg
from omnivggt_official_amd import lib as L, ops
from test_gpu_edges import DEV, GATE, MODES, Slot, _conv_ref, _global, _need_gpu, _sync_check, _val  # noqa: F401 (_need_gpu: the autouse fixture)

pytestmark = pytest.mark.gpu
WORST = {}


def _note(family, used):
    WORST[family] = max(WORST.get(family, 0.0), used)
    print("worst used budget so far: " + ", ".join("%s %.3f" % kv for kv in sorted(WORST.items())), flush=True)


# =============================================================================================
# ovg_dpt_tail
# =============================================================================================
def _persist_images():
    """n with 2 cus < 9 n < 3 cus and 9 n no multiple of cus: every workgroup owns two or three tiles and the last round is partial."""
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    n = (5 * cus) // 18 + 1
    while (9 * n) % cus == 0:
        n += 1
    assert 2 * cus < 9 * n < 3 * cus, (cus, n)
    return n


def _pixel_strided(t, poison, pad=8):
    """t [n, H, W, C] (CPU) -> the same values as a channel slice of a device [n, H, W, C + pad] buffer, poison (or zeros) in the gaps."""
    shape = tuple(t.shape[:-1]) + (t.shape[-1] + pad,)
    big = kg.poison_values(shape, t.dtype, "cpu") if poison else torch.zeros(shape, dtype=t.dtype)
    big[..., : t.shape[-1]] = t
    return big.to(DEV)[..., : t.shape[-1]]


def _wide_w1(w1, poison):
    """w1 [32, 1152] -> a [128, 1152] view of a device [128, 1160] matrix (ldw1 = 1160) whose rows 32.. and columns 1152.. hold poison (or
    zeros): the kernel must read 32 rows of 1152 values."""
    big = kg.poison_values((128, 1160), w1.dtype, "cpu") if poison else torch.zeros(128, 1160, dtype=w1.dtype)
    big[:32, :1152] = w1
    return big.to(DEV)[:, :1152]


@pytest.mark.parametrize("case", list(kg.DPT_TAIL_CASES))
@pytest.mark.parametrize("mode", ["bf16", "f16"])
def test_dpt_tail_every_form_against_the_per_element_budget(mode, case):
    dt = MODES[mode]
    n = _persist_images() if kg.DPT_TAIL_CASES[case][0] == 0 else None
    I = kg.dpt_tail_inputs(case, mode, n=n)
    n, OH, OW, od, act = I["n"], I["OH"], I["OW"], I["od"], I["act"]
    H, W = I["x"].shape[1:3]
    tag = "dpt_tail_%s_%s" % (case, mode)
    assert ops.dpt_tail_supported(I["x"], dt, OH, OW), tag
    dv = lambda t: None if t is None else t.to(DEV)
    posd = None if I["pos"] is None else (dv(I["pos"][0]), dv(I["pos"][1]))
    b1d, w2d, b2d = dv(I["b1"]), dv(I["w2"]), dv(I["b2"])
    outs = []
    for poison in (True, False):
        tv = Slot.get((n, OH, OW, od - 1), torch.float32, None, tag="tailv")
        tc = Slot.get((n * OH, OW), torch.float32, None, tag="tailc")
        ops.dpt_tail(_pixel_strided(I["x"], poison), OH, OW, dt, posd, _wide_w1(I["w1"], poison), b1d, w2d, b2d, act, out=(tv.view, tc.view.view(n, OH, OW)))
        _sync_check(tv.check, tc.check)
        outs.append((_val(tv.view), _val(tc.view).view(n, OH, OW)))
    assert torch.equal(outs[0][0], outs[1][0]) and torch.equal(outs[0][1], outs[1][1]), \
        "%s: the result depends on what lies beside x, behind row 32 of w1 or beside its 1152 columns" % tag
    val, conf = outs[0]
    B = kg.dpt_tail_budget(I["x"].double(), OH, OW, I["pos"], I["w1"].double(), I["b1"], I["w2"], I["b2"], act, mode)
    share = float(B["win"]["window"].double().mean())
    assert share <= 0.10, "%s: the rounding window holds %.1f%% of the upsampled map" % (tag, 100 * share)
    gate = kg.DPT_TAIL_GATE[mode]
    _global(tag + ".val", val, B["val"], gate)
    _global(tag + ".conf", conf, B["conf"], gate)
    _note("dpt_tail", kg.check_dpt_tail(tag, val, conf, B))
    # the three launches it replaces, on dense operands: their 16-bit map against the window, their outputs against the same budget, and
    # the two forms against each other at the global gate
    w1z = torch.zeros(128, 9 * 128, dtype=dt)
    w1z[:32] = I["w1"]
    xd = I["x"].to(DEV)
    up3 = ops.upsample(xd, OH, OW, dt, pos=posd)
    hmap = ops.conv(up3, w1z.to(DEV), b1d, dt, 32, ksize=3, relu=True, out_f32=True)
    v3, c3 = ops.dpt_out(hmap, w2d, b2d, act)
    torch.cuda.synchronize()
    kg.check_upsampled_map(tag + "_upsample", up3, B["win"])
    _note("dpt_tail three launches", kg.check_dpt_tail(tag + "_three_launches", v3, c3, B))
    _global(tag + ".val_vs_three_launches", val, v3.double().cpu(), gate)
    _global(tag + ".conf_vs_three_launches", conf, c3.double().cpu(), gate)
    print("%s: n=%d %dx%d -> %dx%d, window share %.2f%%" % (tag, n, H, W, OH, OW, 100 * share), flush=True)
    Slot.cache.clear()


# =============================================================================================
# the 256-pixel convolutions
# =============================================================================================
def _expected_conv256(mode, n, H, W, cin, cout, k, stride, up, ldx):
    """ovg_conv's dispatch condition (csrc/ovg_head.hip), restated: None = the 128-pixel kernel, else the GEMM columns per tile (256 or 128)
    of the 256-pixel form: a 16-bit output, every GEMM column real, an even number of 32-channel k-stages, at least 16384 output pixels, the
    images a tile of 256 consecutive output pixels can touch (255 // (OH OW) + 2: two from 256-pixel maps on) and the weights within 32-bit
    byte offsets."""
    s = up if up > 1 else 1
    pd = k // 2
    opix = ((H + 2 * pd - k) // stride + 1) * ((W + 2 * pd - k) // stride + 1)
    M = n * opix
    cols = s * s * cout
    ok = (mode in ("bf16", "f16") and cols % 128 == 0 and cin % 32 == 0 and (k * k * (cin // 32)) % 2 == 0 and M >= 16384
          and (255 // opix + 2) * H * W * ldx * 2 < (1 << 32) - 65536 and cols * k * k * cin * 2 < (1 << 32))
    return (256 if cols % 256 == 0 else 128) if ok else None


FORMS = {"1x1_pos": dict(k=1, pos=True), "3x3_add2_relu": dict(k=3, adds=2, relu=True), "3x3s2_add1": dict(k=3, stride=2, adds=1),
         "convT2": dict(up=2), "convT4": dict(up=4)}

#  group: [(n, H, W, cin, form, x as a channel slice too)]; every entry runs with 128 and with 256 GEMM columns
CONV256_CASES = {
    # M just above the line and ragged: 16512 = 64.5 tiles (65 m-tiles: a group tail of one in the tile order, mtiles % 4 = 1)
    "ragged_128x129": [(1, 128, 129, 64, f, True) for f in ("1x1_pos", "3x3_add2_relu", "convT2", "convT4")],
    # 129 x 127 = 16383 is ONE pixel below the line: the 128-pixel kernel takes it (printed), the other side of the switch at the same size
    "ragged_129x127": [(1, 129, 127, 64, f, False) for f in ("1x1_pos", "3x3_add2_relu", "convT2", "convT4")],
    # 129 x 129 = 16641 = 65 tiles + 1 pixel: 66 m-tiles (a group tail of two), the last tile holds one live row
    "ragged_129x129": [(1, 129, 129, 64, f, False) for f in ("1x1_pos", "3x3_add2_relu", "convT2", "convT4")],
    "stride2_257x255": [(1, 257, 255, 64, "3x3s2_add1", True)],                                     # 129 x 128 outputs
    # images smaller than a tile: 16 images of 4 x 4 per tile; 1 x 1 maps (eight of nine taps outside, the wrapped offset for every pixel)
    "tiny_images": [(1100, 4, 4, 64, "3x3_add2_relu", False), (1100, 4, 4, 128, "1x1_pos", False), (16400, 1, 1, 64, "3x3_add2_relu", True), (16400, 1, 1, 64, "convT2", False)],
    # images of 255 and 257 pixels: a tile boundary walks through the images
    "images_255_257": [(65, 15, 17, 64, "3x3_add2_relu", False), (64, 257, 1, 64, "3x3_add2_relu", False), (65, 15, 17, 64, "convT2", False)],
    # k loops of 2, 4, 6 and 18 stages on both ring depths (prologue + drain only; drain without / with one steady-state iteration)
    "k_loops": [(1, 128, 129, 64, "1x1_pos", False), (1, 128, 129, 128, "1x1_pos", False), (1, 128, 129, 192, "1x1_pos", False), (1, 128, 129, 64, "3x3_add2_relu", False)],
}


def _conv256_one(mode, n, H, W, cin, fname, cols, sliced, g):
    dt = MODES[mode]
    f = FORMS[fname]
    k, stride, up, relu, adds, pos = f.get("k", 1), f.get("stride", 1), f.get("up", 0), f.get("relu", False), f.get("adds", 0), f.get("pos", False)
    s_ = up if up > 1 else 1
    cout = cols // (s_ * s_)
    pd = k // 2
    OH, OW = (H + 2 * pd - k) // stride + 1, (W + 2 * pd - k) // stride + 1
    tag = "conv256_%s_%s_n%d_%dx%d_cin%d_cols%d" % (fname, mode, n, H, W, cin, cols)
    want = _expected_conv256(mode, n, H, W, cin, cout, k, stride, up, cin)
    if n * OH * OW < 16384:                     # a listed shape below the line is a finding about the list, printed and still checked
        print("%s: M = %d is dispatched to the 128-pixel kernel" % (tag, n * OH * OW), flush=True)
    else:
        assert want == cols, "%s: expected the 256-pixel form with %d columns, the restated dispatch says %s" % (tag, cols, want)
    x = torch.randn(n, H, W, cin, generator=g).to(dt)
    w = (torch.randn(cols, k * k * cin, generator=g) * (k * k * cin) ** -0.5).to(dt)
    bias = torch.randn(cout, generator=g) * 0.3
    adds_t = [torch.randn(n, OH, OW, cout, generator=g).to(dt) for _ in range(adds)]
    ps = (torch.randn(OW, cout // 2, generator=g) * 0.1, torch.randn(OH, cout // 2, generator=g) * 0.1) if pos else None
    d64 = lambda t: None if t is None else t.double()
    add_d = [_pixel_strided(t, True) for t in adds_t]
    posd = None if ps is None else (ps[0].to(DEV), ps[1].to(DEV))

    def run(xd):
        slot = Slot.get((n, OH * s_, OW * s_, cout), dt, cout + 8, tag="c256")
        ops.conv(xd, w.to(DEV), bias.to(DEV), dt, cout, ksize=k, stride=stride, upshuffle=up, relu=relu,
                 add1=add_d[0] if adds >= 1 else None, add2=add_d[1] if adds >= 2 else None, pos=posd, out=slot.view)
        _sync_check(slot.check)
        return _val(slot.view)

    # dense x, allocated exactly: the descriptor's range ends behind the last image's bottom-right pixel
    got = run(x.to(DEV))
    ref, mag = _conv_ref(x.double(), w.double(), bias.double(), cout, k, stride, up, relu, d64(adds_t[0]) if adds >= 1 else None,
                         d64(adds_t[1]) if adds >= 2 else None, None if ps is None else (ps[0].double(), ps[1].double()))
    _global(tag, got, ref, GATE[mode])
    used = kg.elementwise_budget(tag, got, ref, mag, kg.U_OUT[mode], kg.gemm_c(k * k * cin, mode) + 4 * kg.MARGIN, extra=kg.f16_subnormal_floor(mode), quiet=True)
    _note("conv 256x%d" % cols if n * OH * OW >= 16384 else "conv 128-pixel", used)
    if sliced:
        assert _expected_conv256(mode, n, H, W, cin, cout, k, stride, up, cin + 8) == want
        assert torch.equal(run(_pixel_strided(x, True)), got), "%s: a channel slice of a wider buffer (ldx = Cin + 8) gives other bits than the dense source" % tag
        kg.STATS["numeric"] += 1


@pytest.mark.parametrize("group", list(CONV256_CASES))
@pytest.mark.parametrize("mode", ["bf16", "f16"])
def test_conv256_ragged_tiny_strided_and_short_k_loops(mode, group):
    g = torch.Generator().manual_seed(131 + list(CONV256_CASES).index(group))
    for (n, H, W, cin, fname, sliced) in CONV256_CASES[group]:
        for cols in (128, 256):
            _conv256_one(mode, n, H, W, cin, fname, cols, sliced, g)
    Slot.cache.clear()
    torch.cuda.empty_cache()


# =============================================================================================
# ovg_camera_tables
# =============================================================================================
@pytest.mark.parametrize("case", list(kg.CAMERA_CASES))
def test_camera_tables_encoding_and_tables_per_element(case):
    """The entry with caller-owned enc / emb / tables inside guard bands (raw parameters, as the stream-contract case passes them): the
    encoding read back and compared per element with the float64 evaluation of camera_math, the tables with the budget carried through both
    Linear layers, rows of views without a camera exactly adapt_b. fx != fy on a non-square frame in every case."""
    G = 2
    weights = kg.camera_weights(G)
    ext, intr, idx = kg.camera_inputs(case)
    B, S = ext.shape[:2]
    Sc = len(idx)
    hw = kg.CAMERA_HW
    assert float((intr[..., 0, 0] - intr[..., 1, 1]).abs().min()) > 1.0 and hw[0] != hw[1]
    Bd = kg.camera_tables_budget(ext, intr, idx, hw, *weights)
    wd = [t.to(DEV) for t in weights]
    extd, intrd, idxd = ext.to(DEV).contiguous(), intr.to(DEV).contiguous(), torch.tensor(idx, dtype=torch.int32, device=DEV)
    enc = Slot.get((B * Sc, 9), torch.float32, None, tag="camenc")
    emb = Slot.get((G * B * Sc, 1024), torch.float32, None, tag="camemb")
    tab = Slot.get((G * B * S, 1024), torch.float32, None, tag="camtab")
    p = L.CameraTablesParams()
    p.B, p.S, p.Sc, p.H, p.W, p.G = B, S, Sc, hw[0], hw[1], G
    p.pose_w, p.pose_b, p.adapt_w, p.adapt_b = (L.ptr(t) for t in wd)
    p.extrinsics, p.intrinsics, p.index = L.ptr(extd), L.ptr(intrd), L.ptr(idxd)
    p.enc, p.emb, p.tables = L.ptr(enc.view), L.ptr(emb.view), L.ptr(tab.view)
    L.call("ovg_camera_tables", p, ops._stream())
    _sync_check(enc.check, emb.check, tab.check)
    a, b = kg.check_camera_tables("camera_tables_" + case, _val(enc.view), _val(tab.view).view(G, B * S, 1024), Bd)
    _note("camera encoding", a)
    _note("camera tables", b)
    # the front end on the same inputs: the same bits
    got = ops.camera_tables(extd, intrd, idxd, S, hw, *wd)
    torch.cuda.synchronize()
    assert torch.equal(got.cpu(), tab.view.view(G, B * S, 1024).cpu()), "camera_tables %s: ops.camera_tables and the raw call disagree" % case
    Slot.cache.clear()
