"""Build libomnivggt_hip.so (gfx950) in-tree with hipcc.

`python -m omnivggt_official_amd.build` or `__graft_entry__.build()`.  hipcc
cross-compiles without a GPU; the .so lands next to this file so it travels
with the tree (git-ignored, not gpurun-ignored).
"""
import hashlib
import os
import subprocess
import sys
from concurrent.futures import ThreadPoolExecutor

HERE = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(HERE, "csrc")
OUT = os.path.join(HERE, "libomnivggt_hip.so")
SOURCES = ["ovg_gemm.hip", "ovg_attn.hip", "ovg_elem.hip", "ovg_block.hip", "ovg_head.hip", "ovg_camhead.hip", "ovg_camtab.hip", "ovg_pointcloud.hip",
           "ovg_preprocess.hip", "ovg_render.hip", "ovg_consistency.hip", "ovg_nn.hip", "ovg_fps.hip", "ovg_radius.hip", "ovg_normals.hip",
           "ovg_align.hip", "ovg_plane.hip", "ovg_tsdf.hip", "ovg_raster.hip", "ovg_deptheval.hip", "ovg_mapgeom.hip", "ovg_meshops.hip", "ovg_meshsimp.hip"]
FLAGS = ["--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "-fno-gpu-rdc", "-Wall", "-Wno-unused-function"]
# every exact-arithmetic unit restates a numpy twin (tests/*_twin.py) operation for operation, one rounding each: no FMA contraction
# anywhere in it, the inlined HIP header helpers and the shared primitives of csrc/ovg_geom.h and csrc/ovg_project.h included
EXACT_UNITS = ("ovg_pointcloud.hip", "ovg_render.hip", "ovg_consistency.hip", "ovg_nn.hip", "ovg_fps.hip", "ovg_radius.hip", "ovg_normals.hip",
               "ovg_align.hip", "ovg_plane.hip", "ovg_tsdf.hip", "ovg_raster.hip", "ovg_deptheval.hip", "ovg_mapgeom.hip")
# attention: no NaN can occur on valid inputs (masked scores are -inf, never inf-inf), and without
# this hipcc inserts a canonicalising v_max before every fmaxf on an MFMA output (64 VALU / tile)
EXTRA_FLAGS = {"ovg_attn.hip": ["-fno-honor-nans"], **{unit: ["-ffp-contract=off"] for unit in EXACT_UNITS},
               "ovg_meshsimp.hip": ["-ffp-contract=off"],      # exact like the thirteen: the mean position and the normalisation restate numpy
               "ovg_meshops.hip": ["-ffp-contract=off"]}       # and so do the quantisation, the update and the normals of the smoother


# attn16_kernel<bf16, QB, WAVES, MODE 0, RING, X3 0>: the three launches of the bf16 plan (mangled-name fragment -> QB)
PINNED_ATTENTION_KERNELS = {"IDF16bLi4ELi8ELi0ELi5ELi0E": 4, "IDF16bLi4ELi4ELi0ELi3ELi0E": 4, "IDF16bLi2ELi4ELi0ELi3ELi0E": 2}


# everything a pinned hot loop may contain besides scalar (s_*) instructions
PINNED_LOOP_MNEMONICS = {"v_mfma_f32_16x16x32_bf16", "v_exp_f32", "v_cvt_pk_bf16_f32", "ds_read_b128",
                         "v_add_u32_e32", "v_or_b32_e32", "v_lshl_or_b32", "v_lshl_add_u32", "v_add_lshl_u32", "v_lshlrev_b32_e32", "v_and_b32_e32"}


def check_pinned_attention_loops(asm_text):
    """The order-pinned attention body (csrc/ovg_attn16_body_q*.inc: one `asm volatile` per MFMA / exp / convert / fragment read) is only
    correct while hipcc allocates registers AROUND those statements without materialising copies: it inserts no hazard wait states for
    inline asm, so a v_mov that builds a P fragment in front of the consuming asm MFMA, or a spilled accumulator, yields finite, plausible,
    WRONG attention output that the kernel's own post-pass check (row sums, non-finite values) need not catch (round-4 advisor finding).
    So the build itself disassembles what it just compiled and refuses to produce a library unless the hot loop of every shipped speculative
    kernel holds exactly one tile's instructions and nothing outside PINNED_LOOP_MNEMONICS (+ scalar instructions). Returns the per-kernel counts.
    build() reacts to a failure by recompiling ovg_attn.hip with the compiler-scheduled tile body (-DOVG_ATTN_PIPE_LOOP=0: slower, always correct)."""
    import re
    kernels, name, body = {}, None, []
    for line in asm_text.splitlines():
        m = re.match(r"^(_ZN\S*attn16_kernel\S*):", line)
        if m:
            name, body = m.group(1), []
            continue
        if name is not None:
            body.append(line)
            if "s_endpgm" in line:
                kernels[name], name = body, None
    report = {}
    for pat, qb in PINNED_ATTENTION_KERNELS.items():
        hits = [k for k in kernels if pat in k]
        if len(hits) != 1:
            raise RuntimeError("pinned-attention check: kernel %s not found exactly once (%r)" % (pat, hits))
        blocks, cur = [], []
        for line in kernels[hits[0]]:
            if re.match(r"^\.LBB", line):
                blocks.append(cur)
                cur = []
            elif line.startswith("\t") and not line.strip().startswith((".", ";")):
                cur.append(line.split()[0])
        blocks.append(cur)
        pinned = [b for b in blocks if sum("v_mfma" in i for i in b) == 18 * qb and b.count("v_exp_f32") == 16 * qb]
        if len(pinned) != 1:
            raise RuntimeError("pinned-attention check: %s has %d candidate hot loops (MFMA / exp counts per block: %r)"
                               % (pat, len(pinned), [(sum("v_mfma" in i for i in b), b.count("v_exp_f32")) for b in blocks if any("v_mfma" in i for i in b)]))
        hot = pinned[0]
        if hot.count("v_cvt_pk_bf16_f32") != 8 * qb or hot.count("ds_read_b128") != 16:
            raise RuntimeError("pinned-attention check: %s hot loop holds %d converts / %d fragment reads" % (pat, hot.count("v_cvt_pk_bf16_f32"), hot.count("ds_read_b128")))
        # WHITELIST (round-5 advisor: a blacklist of v_mov / v_accvgpr / ... would let any other compiler-inserted VALU write into an MFMA
        # source pass): besides scalar instructions the hot loop may hold exactly the tile's own matrix / exp / convert instructions, the
        # fragment reads, and the integer address arithmetic of the ring (which writes LDS addresses, never an MFMA operand)
        bad = [i for i in hot if not (i.startswith("s_") or i in PINNED_LOOP_MNEMONICS)]
        if bad:
            raise RuntimeError("pinned-attention check: hipcc put instructions outside the pinned tile's own set (register copies / spills / "
                               "re-materialised operands) inside the hot loop of %s: %r -- the bf16 attention results of such a build are NOT "
                               "trustworthy" % (pat, sorted(set(bad))))
        report[pat] = {"instructions": len(hot), "mfma": 18 * qb}
    return report

TRANS_OPS = ("v_exp_f32", "v_log_f32", "v_rcp_f32", "v_rsq_f32", "v_sqrt_f32", "v_sin_f32", "v_cos_f32", "v_exp_f16", "v_log_f16", "v_rcp_f16", "v_rsq_f16", "v_sqrt_f16")


def _vregs(operand):
    """VGPR numbers named by one operand: v12, -v12, |v12|, v[4:7]."""
    import re
    out = set()
    for m in re.finditer(r"\bv\[(\d+):(\d+)\]", operand):
        out.update(range(int(m.group(1)), int(m.group(2)) + 1))
    for m in re.finditer(r"\bv(\d+)\b", operand):
        out.add(int(m.group(1)))
    return out


def check_trans_use_in_asm(asm_text):
    """gfx950: the result of a transcendental VALU instruction (v_exp_f32, v_rcp_f32, ...) may not be read by a VALU instruction in the next
    issue slot. hipcc pads that for the instructions it schedules, NOT for an inline-asm statement that reads the register (it treats the
    statement as opaque: cdna_hip_programming.md 5.7 item 2) -- the reader then sees the OLD register contents, silently. Round 6 found the
    split-f16 attention body (v_exp_f32 by the compiler, v_cvt_pk_f16_f32 / v_fma_mix / v_pk_add_f32 in asm statements) depending on where the
    scheduler happened to put its exps. This check walks the assembly of a translation unit and refuses any compiler-scheduled transcendental
    whose destination is read by the inline-asm instruction that directly follows it. Returns the number of (transcendental, asm) neighbours seen."""
    seen, in_asm, prev = 0, False, None          # prev = (mnemonic, dest regs) of the previous real instruction if the compiler scheduled it
    for line in asm_text.splitlines():
        t = line.strip()
        if t.startswith(";;#ASMSTART"):
            in_asm = True
            continue
        if t.startswith(";;#ASMEND"):
            in_asm = False
            continue
        if not line.startswith("\t") or not t or t.startswith((".", ";")):
            if t.endswith(":"):
                prev = None                      # a label: the fall-through neighbour is still the previous instruction, but be conservative
            continue
        mnem, _, rest = t.partition(" ")
        ops = [o.strip() for o in rest.split(",")]
        if in_asm and prev is not None and (mnem.startswith("v_") or mnem.startswith("ds_") or mnem.startswith("global_") or mnem.startswith("buffer_")):
            seen += 1
            srcs = set()
            for o in (ops[1:] if mnem.startswith("v_") and not mnem.startswith("v_cmp") else ops):
                srcs |= _vregs(o)
            if mnem.startswith("v_fma_mix") or mnem.startswith("v_pk_add") or mnem.startswith("v_mfma"):
                srcs |= _vregs(ops[0])           # read-modify-write destinations
            if srcs & prev[1]:
                raise RuntimeError("trans-use check: compiler-scheduled %s writes v%s and the inline-asm `%s` directly behind it reads it -- "
                                   "hipcc pads no hazard for asm statements; put an opaque wait state between them (ovg_attn16.h pv_step)"
                                   % (prev[0], sorted(prev[1]), t))
        if mnem == "s_nop":
            prev = None
            continue
        if not in_asm and mnem.split("_e32")[0].split("_e64")[0] in TRANS_OPS:
            prev = (mnem, _vregs(ops[0]))
        else:
            prev = None
    return seen


def _hipcc():
    for c in (os.environ.get("HIPCC"), "/opt/rocm/bin/hipcc", "hipcc"):
        if c and (os.path.isabs(c) and os.path.exists(c) or not os.path.isabs(c)):
            return c
    raise RuntimeError("hipcc not found")


def _digest():
    h = hashlib.sha256()
    files = [os.path.join(CSRC, f) for f in sorted(os.listdir(CSRC))]
    files.append(os.path.join(HERE, "..", "include", "omnivggt_hip.h"))
    for f in files:
        with open(f, "rb") as fh:
            h.update(fh.read())
    h.update(" ".join(FLAGS).encode())
    h.update(repr(sorted(EXTRA_FLAGS.items())).encode())
    return h.hexdigest()


def is_current():
    """True when the in-tree .so was built from exactly the current sources / header / flags."""
    stamp = OUT + ".stamp"
    return os.path.exists(OUT) and os.path.exists(stamp) and open(stamp).read().strip() == _digest()


def have_hipcc():
    try:
        c = _hipcc()
    except RuntimeError:
        return False
    import shutil
    return os.path.isabs(c) or shutil.which(c) is not None


def build(force=False, verbose=True):
    """Compile every HIP translation unit for gfx950 and link the shared library.
    Safe against concurrent callers (one process per GPU all finding a stale library at start-up): an exclusive file lock
    serialises them, the objects of each caller go to a private directory, and the library appears by an atomic rename --
    a reader never maps a half-written .so, and whoever comes second finds the stamp current and returns."""
    import fcntl
    import shutil
    import tempfile
    stamp = OUT + ".stamp"
    with open(OUT + ".lock", "w") as lock:
        fcntl.flock(lock, fcntl.LOCK_EX)
        try:
            dig = _digest()
            if not force and is_current():
                return OUT
            hipcc = _hipcc()
            os.makedirs(os.path.join(HERE, "build"), exist_ok=True)
            objdir = tempfile.mkdtemp(prefix="obj.", dir=os.path.join(HERE, "build"))

            def cc(src, extra=()):
                obj = os.path.join(objdir, src.replace(".hip", ".o"))
                cmd = [hipcc, *FLAGS, *EXTRA_FLAGS.get(src, []), *extra, "-c", os.path.join(CSRC, src), "-o", obj]
                if src == "ovg_attn.hip":
                    cmd.insert(1, "-save-temps=obj")          # keeps the gfx950 assembly of THIS compile next to the object: checked below
                r = subprocess.run(cmd, capture_output=True, text=True)
                if r.returncode != 0:
                    raise RuntimeError("hipcc failed for %s:\n%s" % (src, r.stderr[-4000:]))
                if verbose and r.stderr.strip():
                    sys.stderr.write(r.stderr)
                if src == "ovg_attn.hip" and not extra:
                    asm = [f for f in os.listdir(objdir) if f.startswith("ovg_attn") and f.endswith(".s") and "gfx950" in f]
                    if len(asm) != 1:
                        raise RuntimeError("pinned-attention check: expected one gfx950 assembly file of ovg_attn.hip, found %r" % asm)
                    try:
                        text = open(os.path.join(objdir, asm[0])).read()
                        check_pinned_attention_loops(text)
                        check_trans_use_in_asm(text)
                    except RuntimeError as e:
                        # a hipcc that schedules the pinned body differently must not leave the user without a library (round-5 advisor):
                        # the compiler-scheduled body is the same arithmetic without hand-placed instructions -- nothing for the guard to
                        # check -- at a few percent of attention throughput
                        sys.stderr.write("WARNING: %s\nWARNING: rebuilding ovg_attn.hip with -DOVG_ATTN_PIPE_LOOP=0 (compiler-scheduled attention "
                                         "tile body: correct, slower); fix csrc/ovg_attn16_body_q*.inc for this compiler to get the pinned loop back\n" % e)
                        return cc(src, extra=("-DOVG_ATTN_PIPE_LOOP=0",))
                return obj

            try:
                with ThreadPoolExecutor(max_workers=len(SOURCES)) as ex:
                    objs = list(ex.map(cc, SOURCES))
                tmp_out = os.path.join(objdir, "libomnivggt_hip.so")
                r = subprocess.run([hipcc, "--offload-arch=gfx950", "-shared", "-fPIC", "-o", tmp_out, *objs], capture_output=True, text=True)
                if r.returncode != 0:
                    raise RuntimeError("link failed:\n" + r.stderr[-4000:])
                if os.path.exists(stamp):
                    os.remove(stamp)                      # never a current stamp next to a library it does not describe
                os.replace(tmp_out, OUT)
                with open(stamp + ".tmp", "w") as fh:
                    fh.write(dig)
                os.replace(stamp + ".tmp", stamp)
            finally:
                shutil.rmtree(objdir, ignore_errors=True)
            return OUT
        finally:
            fcntl.flock(lock, fcntl.LOCK_UN)


if __name__ == "__main__":
    print(build(force="--force" in sys.argv))
