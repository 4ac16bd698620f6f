"""Shapes, arithmetic and CPU models behind tests/test_gpu_address_range.py (a plain helper module like kernel_guards;
tests/test_address_range_host.py proves on the CPU that the table says what it claims and that the oracles see a wrapped address).

The GPU tests run the block and head kernels on operands whose byte offsets pass 2 GiB and 4 GiB and whose element indices pass 2^31,
with compute kept tiny. Two forms:

  stride form   few rows, a row (or pixel) stride of FAR_STRIDE_BYTES = 16 MiB + 64 B: row 128 starts past 2 GiB, row 256 past 4 GiB
                (= 2^31 elements of a 16-bit type), row 512 past 8 GiB (= 2^31 f32 elements). ONE operand is far per case, the others sit
                at ld = row length + NEAR_PAD, so a failure names its operand. Oracle: bit-equal to the near twin (every operand near).
  count form    dense layouts with many rows; the inputs are periodic with period PERIOD (a prime, no multiple of any tile) rows, pixels,
                heads or frames, so output row m must equal output row m mod PERIOD; the first PERIOD rows are the near twin.

CASES is the one table both test modules read: the GPU module takes every shape from it, the host module proves by arithmetic that the
far operand of each case passes exactly the lines the case claims, that every other operand stays below 2 GiB, and that the case fits
MEM_CAP. Operands are modelled as [rows, cols] with a row stride (NHWC maps: rows = pixels; q / k [BH, n_pad, 64]: rows = BH n_pad;
V^T [BH, 64, n_pad]: rows = 64 BH)."""
import collections

import numpy as np

GIB = 1 << 30
LINES = {"2GiB": 1 << 31, "4GiB": 1 << 32, "2^31el": 1 << 31}      # the first two on the last byte's offset, the third on the last element's index
FAR_STRIDE_BYTES = (16 << 20) + 64
# ovg_conv's 256-pixel form needs >= 16384 output pixels: at 129 x 128 pixels the 16 MiB stride would take 277 GB per tensor; 512 KiB + 64 B
# per pixel passes the same three lines in 8.7 GB
CONV256_STRIDE_BYTES = (512 << 10) + 64
NEAR_PAD = 8
PERIOD = 1031
ROWS16, ROWS32 = 257, 513          # rows of a far 16-bit / f32 operand: two GEMM tiles + 1; f32 needs 513 rows for 2^31 elements
MEM_CAP = 24 * GIB                 # per test
TENSOR_CAP = 12 * GIB              # per tensor: a dense operand that needs more to cross its lines is listed in NOT_RUN instead
CHUNK_BYTES = 1 << 28              # device-side comparisons and guard checks work in steps of at most this
ALL3 = ("2GiB", "4GiB", "2^31el")


class Operand(collections.namedtuple("Operand", "rows cols ld esz planes")):
    """rows x cols elements of esz bytes, row stride ld elements; planes: 2 for the (hi, lo) pair of the split-f16 mode (same layout each)."""
    __slots__ = ()

    @property
    def last_elem(self):
        return (self.rows - 1) * self.ld + self.cols - 1

    @property
    def last_byte(self):
        return (self.last_elem + 1) * self.esz - 1

    @property
    def bytes(self):
        return (self.last_byte + 1) * self.planes

    def lines(self):
        return tuple(n for n in ALL3 if (self.last_elem if n == "2^31el" else self.last_byte) >= LINES[n])


def dense(rows, cols, esz, planes=1):
    return Operand(rows, cols, cols, esz, planes)


def near(rows, cols, esz, planes=1):
    return Operand(rows, cols, cols + NEAR_PAD, esz, planes)


def far(rows, cols, esz, planes=1, stride_bytes=FAR_STRIDE_BYTES):
    assert stride_bytes % esz == 0 and stride_bytes % 16 == 0
    return Operand(rows, cols, stride_bytes // esz, esz, planes)


def far_rows(esz):
    return ROWS16 if esz == 2 else ROWS32


# name: unique; entry: the C entry; form: "stride" | "count"; far: {operand: lines its last byte / element passes}; operands: {name: Operand};
# arg: whatever else the GPU test needs to rebuild the call (shape numbers, mode, tile, ...); scratch: bytes of device memory the test holds
# besides the operands (near twin, chunk temporaries, workspaces)
Case = collections.namedtuple("Case", "name entry form far operands arg scratch")
CASES = collections.OrderedDict()
CHUNK_SCRATCH = 4 * CHUNK_BYTES     # a chunk, its gathered twin, the comparison mask and the indices of what differs


def _add(name, entry, form, claims, operands, arg=None, scratch=0):
    """claims: {operand: the lines it is meant to pass} -- written down here, proved from the shapes by test_address_range_host.py."""
    assert name not in CASES and all(n in operands for n in claims), name
    CASES[name] = Case(name, entry, form, {n: tuple(c) for n, c in claims.items()}, operands, arg or {}, scratch + CHUNK_SCRATCH)


def twin_of(op):
    """The near twin of a strided operand: the same rows at ld = cols + NEAR_PAD (an operand the entry takes no stride for stays dense)."""
    return op if op.ld == op.cols else near(op.rows, op.cols, op.esz, op.planes)


def _stride_case(name, entry, shapes, which, arg=None, stride_bytes=FAR_STRIDE_BYTES, scratch=0, fixed=()):
    """shapes: {operand: (rows, cols, esz[, planes])}; `which` is placed far, the rest near; `fixed`: operands whose layout the entry fixes
    (no stride in its parameter struct): dense."""
    ops = {}
    for n, s in shapes.items():
        rows, cols, esz = s[:3]
        planes = s[3] if len(s) > 3 else 1
        ops[n] = far(rows, cols, esz, planes, stride_bytes) if n == which else (dense if n in fixed else near)(rows, cols, esz, planes)
    twin = sum(twin_of(o).bytes for o in ops.values())
    _add("%s.%s" % (name, which), entry, "stride", {which: ALL3}, ops, dict(arg or {}, far=which), scratch + twin)


# ---- ovg_linear, stride form: K = 64; STORE in bf16 / f32 / f32x, GELU / RES / PATCH in bf16; both forced tiles for the 16-bit dtypes -----
LINEAR_K = 64
LINEAR_COMBOS = (("bf16", "store", 128), ("bf16", "store", 256), ("f32", "store", 128), ("f32x", "store", 128), ("f32x", "store", 256),
                 ("bf16", "gelu", 128), ("bf16", "gelu", 256), ("bf16", "res", 128), ("bf16", "res", 256),
                 ("bf16", "patch", 128), ("bf16", "patch", 256))
PATCH_P0, PATCH_P1, PATCH_OFF = 256, 259, 3


def linear_shapes(mode, epi, tile, which):
    """{operand: (rows, cols, esz, planes)} of one stride-form ovg_linear case. The far operand decides the row counts: 257 rows where it
    is 16-bit, 513 where it is f32; a far w has as many rows as the next tile multiple above that."""
    ein, planes = (4 if mode == "f32" else 2), (2 if mode == "f32x" else 1)
    eout = 4 if (mode == "f32" or epi in ("res", "patch")) else 2
    e_far = {"x": ein, "w": ein, "y": eout, "res": 4}[which]
    M = far_rows(e_far) if which != "w" else ROWS16
    N = tile if which != "w" else (far_rows(ein) + tile - 1) // tile * tile
    out_rows = M if epi != "patch" else ((M - 1) // PATCH_P0) * PATCH_P1 + PATCH_OFF + (M - 1) % PATCH_P0 + 1
    s = {"x": (M, LINEAR_K, ein, planes), "w": (N, LINEAR_K, ein, planes), "y": (out_rows, N, eout, planes if eout == 2 else 1)}
    if epi == "res":
        s["res"] = (M, N, 4, 1)
    return s


for _mode, _epi, _tile in LINEAR_COMBOS:
    for _which in ("x", "w", "y") + (("res",) if _epi == "res" else ()):
        _stride_case("linear.%s.%s.t%d" % (_epi, _mode, _tile), "ovg_linear", linear_shapes(_mode, _epi, _tile, _which), _which,
                     dict(mode=_mode, epi=_epi, tile=_tile))

# ---- the other strided entries ------------------------------------------------------------------------------------------------------
for _mode, _tile in (("bf16", 128), ("bf16", 256), ("f32", 128), ("f32x", 128)):
    _e, _pl = (4 if _mode == "f32" else 2), (2 if _mode == "f32x" else 1)
    _M = far_rows(_e)                                                                  # one sequence of M tokens: BH = 16
    _pad = (_M + 63) // 64 * 64
    _stride_case("qkv.%s.t%d" % (_mode, _tile), "ovg_qkv",
                 {"x": (_M, 1024, _e, _pl), "w": (3072, 1024, _e, _pl), "q": (16 * _pad, 64, _e, _pl), "k": (16 * _pad, 64, _e, _pl),
                  "vt": (16 * 64, _pad, _e, _pl)}, "x", dict(mode=_mode, tile=_tile, M=_M), fixed=("w", "q", "k", "vt"))
for _mode in ("bf16", "f32", "f32x"):
    _e, _pl = (4 if _mode == "f32" else 2), (2 if _mode == "f32x" else 1)
    _nq = far_rows(_e)
    _pad = (_nq + 63) // 64 * 64
    _stride_case("flash_attn.%s" % _mode, "ovg_flash_attn",
                 {"q": (16 * _pad, 64, _e, _pl), "k": (16 * 128, 64, _e, _pl), "vt": (16 * 64, 128, _e, _pl), "out": (_nq, 1024, _e, _pl)},
                 "out", dict(mode=_mode, nq=_nq, nk=65), fixed=("q", "k", "vt"))
    for _which in ("a", "b", "out"):
        _stride_case("attn_merge.%s" % _mode, "ovg_attn_merge",
                     {"a": (_nq, 1024, _e, _pl), "b": (_nq, 1024, _e, _pl), "out": (_nq, 1024, _e, _pl), "lse": (32, _pad, 4)}, _which, dict(mode=_mode, rows=_nq),
                     fixed=("lse",))
for _mode, _f32 in (("bf16", False), ("bf16", True), ("f32x", False)):
    _eo, _pl = (4 if _f32 else 2), (2 if _mode == "f32x" else 1)
    for _which in ("x", "y"):
        _rows = far_rows(4 if _which == "x" else _eo)
        _stride_case("layernorm.%s%s" % (_mode, ".f32out" if _f32 else ""), "ovg_layernorm",
                     {"x": (_rows, 1024, 4), "y": (_rows, 1024, _eo, _pl)}, _which, dict(mode=_mode, f32=_f32, rows=_rows))
for _which in ("x", "y"):
    _stride_case("copy_rows", "ovg_copy_rows", {"x": (ROWS32, 64, 4), "y": (ROWS32, 64, 4)}, _which, dict(rows=ROWS32, n=64))
for _mode in ("bf16", "f32", "f32x"):
    _e, _pl = (4 if _mode == "f32" else 2), (2 if _mode == "f32x" else 1)
    for _which in ("src", "dst"):
        _rows = far_rows(4 if _which == "src" else _e)
        _stride_case("pack_weights.%s" % _mode, "ovg_pack_weights", {"src": (_rows, 588, 4), "dst": (_rows, 640, _e, _pl)}, _which,
                     dict(mode=_mode, rows=_rows))
_stride_case("dino_specials", "ovg_dino_specials", {"x": (103 * 5, 1024, 4)}, "x", dict(V=103, tpv=5))
for _which in ("xd", "out"):
    _stride_case("assemble_tokens", "ovg_assemble_tokens", {"xd": (86 * 6, 1024, 4), "out": (86 * 6, 1024, 4), "depth_tok": (43, 1024, 4)}, _which,
                 dict(V=86, tpv=6), fixed=("depth_tok",))
for _mode in ("bf16", "f32"):
    _e = 4 if _mode == "f32" else 2
    for _which in ("x", "y"):
        _stride_case("head_layernorm.%s" % _mode, "ovg_head_layernorm", {"x": (2 * 262, 2048, 4), "y": (2 * 257, 2048, _e)}, _which,
                     dict(mode=_mode, views=2, tpv=262))
_stride_case("heads_to_tokens.bf16", "ovg_heads_to_tokens", {"x": (16 * 320, 64, 2), "y": (ROWS16, 1024, 2)}, "y", dict(n=ROWS16, n_pad=320), fixed=("x",))
# ovg_conv, 128-pixel form: one 23 x 23 image (529 pixels: below the 16384 of the 256-pixel form), 3 x 3, 64 -> 128 channels, two adds
for _mode in ("bf16", "f32"):
    _e = 4 if _mode == "f32" else 2
    for _which in ("x", "y", "add1", "add2"):
        _stride_case("conv128.%s" % _mode, "ovg_conv",
                     {"x": (529, 64, _e), "w": (128, 576, _e), "y": (529, 128, _e), "add1": (529, 128, _e), "add2": (529, 128, _e)}, _which,
                     dict(mode=_mode, n=1, H=23, W=23, cin=64, cout=128), fixed=("w",))
# ... and the 256-pixel form (16-bit): 129 x 128 pixels. Its x cannot be far: the form exists only while the images of a tile fit 32-bit
# offsets (conv256.count.* below sits on that line); y / add1 / add2 at CONV256_STRIDE_BYTES per pixel
for _which in ("y", "add1", "add2"):
    _stride_case("conv256.bf16", "ovg_conv",
                 {"x": (129 * 128, 64, 2), "w": (128, 576, 2), "y": (129 * 128, 128, 2), "add1": (129 * 128, 128, 2), "add2": (129 * 128, 128, 2)}, _which,
                 dict(mode="bf16", n=1, H=129, W=128, cin=64, cout=128), stride_bytes=CONV256_STRIDE_BYTES, fixed=("w",))
for _mode in ("bf16", "f32"):
    _e = 4 if _mode == "f32" else 2
    for _which in ("x", "y"):
        _stride_case("upsample.%s" % _mode, "ovg_upsample", {"x": (23 * 23, 8, _e), "y": (24 * 23, 8, _e)}, _which,
                     dict(mode=_mode, H=23, W=23, OH=24, OW=23, C=8))
# ovg_dpt_tail refuses H W ldx >= 2^31 elements, so one image cannot pass 4 GiB: two images of 16 x 15 pixels, the second starts at 3.75 GiB
_stride_case("dpt_tail.bf16", "ovg_dpt_tail", {"x": (2 * 16 * 15, 128, 2), "w1": (32, 1152, 2), "val": (2 * 20 * 19, 1, 4), "conf": (2 * 20, 19, 4)}, "x",
             dict(mode="bf16", n=2, H=16, W=15, OH=20, OW=19), fixed=("val", "conf"))
for _mode in ("bf16", "f32"):
    _stride_case("camera_head.%s" % _mode, "ovg_camera_head", {"tokens": (ROWS32, 2048, 4), "out": (ROWS32, 9, 4)}, "tokens",
                 dict(mode=_mode, S=ROWS32), scratch=128 << 20, fixed=("out",))
for _mode in ("bf16", "f32"):
    _e = 4 if _mode == "f32" else 2
    for _which in ("x_in", "x_out"):
        _stride_case("block_forward.%s" % _mode, "ovg_block_forward", {"x_in": (ROWS32, 1024, 4), "x_out": (ROWS32, 1024, 4)}, _which,
                     dict(mode=_mode, M=ROWS32, seq=ROWS32, tpv=ROWS32, gw=31), scratch=2 * (ROWS32 * 8192 + 3 * 16 * 576 * 64) * _e + (64 << 20))

# ---- count form ----------------------------------------------------------------------------------------------------------------------
COUNT_M = (1 << 24) + 257
# (the f32 output of the 256 tile would be 16 GiB at COUNT_M rows, above TENSOR_CAP: it passes all three lines at 2^23 + 257 rows, 8 GiB)
for _N, _tile, _out, _M in ((128, 128, "16", COUNT_M), (128, 128, "f32", COUNT_M), (256, 256, "16", COUNT_M), (256, 256, "f32", (1 << 23) + 257),
                            (128, 128, "res", COUNT_M)):
    _eo = 2 if _out == "16" else 4
    _o = {"x": dense(_M, LINEAR_K, 2), "w": dense(_N, LINEAR_K, 2), "y": dense(_M, _N, _eo)}
    if _out == "res":
        _o["res"] = dense(_M, _N, 4)
    _add("linear.count.N%d.%s" % (_N, _out), "ovg_linear", "count", {n: (("2GiB",) if n == "x" else ALL3) for n in _o if n != "w" and _o[n].lines()}, _o,
         dict(N=_N, tile=_tile, out=_out, M=_M))
_R = (1 << 20) + 5
_add("layernorm.count", "ovg_layernorm", "count", {"x": ("2GiB", "4GiB"), "y": ("2GiB",)}, {"x": dense(_R, 1024, 4), "y": dense(_R, 1024, 2)}, dict(rows=_R))
_add("copy_rows.count", "ovg_copy_rows", "count", {"x": ("2GiB", "4GiB"), "y": ("2GiB", "4GiB")}, {"x": dense(_R, 1024, 4), "y": dense(_R, 1024, 4)}, dict(rows=_R))
_R = 262144 + 7                       # head_layernorm: 2^16 blocks of 4 rows per trip of its grid-stride loop
_add("head_layernorm.count", "ovg_head_layernorm", "count", {"x": ("2GiB",)}, {"x": dense(_R + 5, 2048, 4), "y": dense(_R, 2048, 2)}, dict(rows=_R))
_O = 16385                            # 16385^2 = 2^28 + 32769 output pixels: the second trip of the 2^20-block grids of upsample / unproject
_add("upsample.count", "ovg_upsample", "count", {"y": ALL3}, {"x": dense(5 * 4, 8, 2), "y": dense(_O * _O, 8, 2)}, dict(H=5, W=4, OH=_O, OW=_O, C=8))
_add("unproject.count", "ovg_unproject", "count", {"out": ("2GiB",)}, {"depth": dense(_O * _O, 1, 4), "out": dense(_O * _O, 3, 4)}, dict(H=_O, W=_O))
_BH = (1 << 19) + 16                  # many short sequences: BH x 64 rows x 128 B passes 4 GiB in q, k, V^T and the output
_add("flash_attn.count", "ovg_flash_attn", "count", {"q": ALL3, "k": ALL3, "vt": ALL3, "out": ALL3},
     {"q": dense(_BH * 64, 64, 2), "k": dense(_BH * 64, 64, 2), "vt": dense(_BH * 64, 64, 2), "out": dense((_BH // 16) * 64, 1024, 2)},
     dict(BH=_BH, nq=64, nk=50))
# ovg_conv's 256-pixel form on both sides of its line: two images of 129 x 128 pixels, tile_images H W ldx 2 < 2^32 - 65536 with
# tile_images = 2 holds for ldx <= 65024 and fails from 65032 on (ldx % 8 == 0)
CONV256_LDX = (65024, 65032)
for _ldx in CONV256_LDX:
    _add("conv256.count.ldx%d" % _ldx, "ovg_conv", "count", {"x": ("2GiB",) if _ldx == CONV256_LDX[0] else ALL3},
         {"x": Operand(2 * 129 * 128, 64, _ldx, 2, 1), "w": dense(128, 576, 2), "y": dense(2 * 129 * 128, 128, 2)},
         dict(n=2, H=129, W=128, cin=64, cout=128, ldx=_ldx), scratch=3 * near(2 * 129 * 128, 128, 2).bytes)
DPT_TAIL_LDX = ((1 << 31) // 20 - 1) // 8 * 8          # the largest ldx % 8 == 0 with 5 x 4 x ldx < 2^31
_add("dpt_tail.count", "ovg_dpt_tail", "count", {"x": ALL3},
     {"x": Operand(2 * 5 * 4, 128, DPT_TAIL_LDX, 2, 1), "w1": dense(32, 1152, 2), "val": dense(2 * 20 * 19, 1, 4), "conf": dense(2 * 20, 19, 4)},
     dict(n=2, H=5, W=4, OH=20, OW=19, ldx=DPT_TAIL_LDX))
for _mode, _M in (("bf16", 262144 + 128), ("f32", 131072 + 128)):
    _e = 4 if _mode == "f32" else 2
    _add("block_forward.count.%s" % _mode, "ovg_block_forward", "count", {"hid": ("2GiB",)},
         {"x_in": dense(_M, 1024, 4), "x_out": dense(_M, 1024, 4), "xn": dense(_M, 1024, _e), "attn": dense(_M, 1024, _e), "hid": dense(_M, 4096, _e),
          "q": dense(_M * 16, 64, _e), "k": dense(_M * 16, 64, _e), "vt": dense(_M * 16, 64, _e)}, dict(mode=_mode, M=_M, seq=64, gw=10),
         scratch=13 * (1 << 20) * _e)

# Dense operands whose smallest line-crossing shape needs more than TENSOR_CAP for one tensor, or more than a second of compute: not run.
# (operand, the shape at which it would first pass 4 GiB or take its second grid trip, bytes of the largest tensor that shape needs)
NOT_RUN = (
    ("ovg_qkv q / k / V^T", "one output passes 2^31 elements at M = 2^25 tokens: x [2^25, 1024] in bf16 is 64 GiB", (1 << 25) * 1024 * 2),
    ("ovg_dpt_out h", "second trip of its 2^20-block grid needs > 2^28 pixels of 32 f32 channels", ((1 << 28) + 1) * 32 * 4),
    ("ovg_im2col out", "ruled out by the issue by name; the size given is its f32 input: 2450 images of 518 x 518 px make the 3.36 million "
     "640-wide bf16 rows (4.3 GB) that pass 4 GiB", 2450 * 3 * 518 * 518 * 4),
)


# ---- CPU models of a 32-bit address (planted defects: test_address_range_host.py) ------------------------------------------------------
def strided_store(buf, first, rows, ldb, rowb, value, wrap32=False):
    """numpy uint8 buffer: write `value` into the rowb bytes of each of `rows` rows, row r at byte offset first + r ldb -- or, wrap32, at
    first + (r ldb mod 2^32): what a kernel does that forms the row offset in 32 bits."""
    for r in range(rows):
        off = (r * ldb) % (1 << 32) if wrap32 else r * ldb
        buf[first + off:first + off + rowb] = value[r] if np.ndim(value) else value
    return buf


def strided_gather(src, rows, ldb, rowb, wrap32=False):
    """[rows, rowb] uint8: row r read from byte offset r ldb of src (mod 2^32 with wrap32)."""
    return np.stack([src[((r * ldb) % (1 << 32) if wrap32 else r * ldb):][:rowb] for r in range(rows)])


def first_wrapped_row(ldb):
    """The first row whose 32-bit byte offset r ldb differs from the true one."""
    return -(-(1 << 32) // ldb)


def first_aperiodic_row(t, period=PERIOD, chunk_rows=None):
    """t [rows, ...] (torch, any device): the first row m with t[m] != t[m mod period] bit for bit, or None. Compared in chunks of at most
    CHUNK_BYTES; the first `period` rows are the twin every other row is held against."""
    import torch
    rows = t.shape[0]
    flat = t.reshape(rows, -1)
    if flat.dtype in (torch.bfloat16, torch.float16):
        flat = flat.view(torch.int16)                     # bit for bit: -0.0 != 0.0, NaN == NaN
    elif flat.dtype == torch.float32:
        flat = flat.view(torch.int32)
    twin = flat[:period]
    rowb = max(1, flat.shape[1] * flat.element_size())
    step = chunk_rows or max(1, CHUNK_BYTES // rowb)
    for a in range(period, rows, step):
        b = min(a + step, rows)
        idx = torch.arange(a, b, device=t.device) % period
        diff = (flat[a:b] != twin[idx]).any(dim=1)
        if bool(diff.any()):
            return a + int(torch.nonzero(diff)[0])
    return None


def tile_periodic(base, rows):
    """base [period, ...] -> [rows, ...] with row m = base[m mod period], filled in place in chunks (no index tensor of `rows` entries)."""
    import torch
    period = base.shape[0]
    out = torch.empty((rows,) + tuple(base.shape[1:]), dtype=base.dtype, device=base.device)
    full = rows // period
    if full:
        out[:full * period].view((full, period) + tuple(base.shape[1:])).copy_(base.unsqueeze(0).expand((full, period) + tuple(base.shape[1:])))
    if rows % period:
        out[full * period:].copy_(base[:rows % period])
    return out
