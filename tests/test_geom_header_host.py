"""CPU only: the primitives of csrc/ovg_geom.h are defined there and nowhere else, read from the source.

The thirteen exact-arithmetic units each carried their own copy of the finite tests, the wave / workgroup scans, the one-workgroup
count scan, the integer reductions, the float64 fold, the 3 x 3 Jacobi solve, the murmur finaliser and the hosts' al / round256 /
size_ok. Every one of them is half of a bit-exactness contract with a numpy twin: a fix to one copy had to be repeated in the others.

 1. none of the shared names is DEFINED (a function body follows its parameter list) in any .hip file or in any other header of csrc/
 2. each of them is defined exactly once in ovg_geom.h
 3. the thirteen units include the header themselves; ovg_project.h takes finite_f32 from it
 4. the scan is proved on a synthetic unit that redefines two of the names locally (and merely calls or mentions others)
"""
import os
import re

from test_launch_streams_host import CSRC, strip

HEADER = "ovg_geom.h"
SHARED = ("finite_f32", "finite_f64", "finite3", "wave_incl_scan", "block_excl_scan", "count_scan", "wave_reduce", "block_reduce", "fold_block",
          "jacobi_rotate", "jacobi_sweeps3", "jacobi_smallest", "mix_murmur64", "al", "round256", "size_ok")
UNITS = ("ovg_pointcloud.hip", "ovg_render.hip", "ovg_consistency.hip", "ovg_nn.hip", "ovg_fps.hip", "ovg_radius.hip", "ovg_normals.hip",
         "ovg_align.hip", "ovg_plane.hip", "ovg_tsdf.hip", "ovg_raster.hip", "ovg_deptheval.hip", "ovg_mapgeom.hip")


def definitions(src, names=SHARED):
    """-> [(name, line)] of every function definition of one of `names` in the source: the name, its balanced parameter list, optional
    trailing qualifiers, then `{`. Calls (followed by `;`, `,`, `)` or an operator) and declarations are no definitions; comments and
    strings do not count."""
    clean = strip(src)
    found = []
    for m in re.finditer(r"\b(%s)\s*\(" % "|".join(map(re.escape, names)), clean):
        before = clean[:m.start()].rstrip()
        if not before or not (before[-1].isalnum() or before[-1] in "_*&>"):     # a definition follows its return type
            continue
        if re.search(r"\b(return|else|case|new|delete|throw|sizeof)$", before):
            continue
        depth, j = 1, m.end()
        while j < len(clean) and depth:
            depth += {"(": 1, ")": -1}.get(clean[j], 0)
            j += 1
        if re.match(r"\s*(const\s*)?(noexcept\s*)?\{", clean[j:]):
            found.append((m.group(1), clean.count("\n", 0, m.start()) + 1))
    return found


def _sources():
    for f in sorted(os.listdir(CSRC)):
        if f.endswith((".hip", ".h", ".inc")):
            with open(os.path.join(CSRC, f)) as fh:
                yield f, fh.read()


SYNTHETIC = '''
#include "ovg_geom.h"
namespace {
// OVG_DEV bool finite_f32(float f) { return true; } in a comment defines nothing
const char* s = "bool al(const void* q, uintptr_t a) {";
OVG_DEV bool finite3(float x, float y, float z) {
  return finite_f32(x) && finite_f32(y) && finite_f32(z);
}
template <typename T>
OVG_DEV T wave_incl_scan (T v) { return v; }
bool size_ok(int64_t n);
__global__ void k(int64_t* c, int64_t n) {
  const int64_t t = count_scan(c, c, n);
  if (finite_f64((double)t) && al(c, 8)) { c[0] = round256(t); }
  else { c[0] = (int64_t)mix_murmur64((uint64_t)t); }
}
}  // namespace
'''


def test_scan_reports_local_redefinitions_and_nothing_else():
    assert definitions(SYNTHETIC) == [("finite3", 6), ("wave_incl_scan", 10)]
    assert definitions("inline bool al(const void* q, uintptr_t a) { return true; }\nint64_t round256(int64_t b) const noexcept\n{ return b; }\n") == \
        [("al", 1), ("round256", 2)]
    assert definitions("  if (x) return size_ok(n) ? 1 : 0;\n  y = al(p, 4) && finite3(a, b, c);\n") == []


def test_shared_names_are_defined_in_the_header_only():
    per_file = {f: definitions(src) for f, src in _sources()}
    assert HEADER in per_file and len(per_file) >= 25, sorted(per_file)
    elsewhere = {f: d for f, d in per_file.items() if f != HEADER and d}
    assert not elsewhere, "shared primitives redefined outside %s: %r" % (HEADER, elsewhere)
    names = [n for n, _ in per_file[HEADER]]
    once = [n for n in SHARED if n != "finite3"]
    assert sorted(n for n in names if n != "finite3") == sorted(once), names        # each exactly once ...
    assert names.count("finite3") == 2                                                # ... and finite3 for three floats and for a pointer


def test_the_thirteen_units_include_the_header():
    sources = dict(_sources())
    for unit in UNITS:
        assert re.search(r'^\s*#\s*include\s+"%s"' % re.escape(HEADER), strip_keep_strings(sources[unit]), re.M), unit
    project = strip_keep_strings(sources["ovg_project.h"])
    assert re.search(r'^\s*#\s*include\s+"%s"' % re.escape(HEADER), project, re.M)
    geom = strip_keep_strings(sources[HEADER])
    assert re.search(r"^\s*#\s*pragma\s+clang\s+fp\s+contract\s*\(\s*off\s*\)", geom, re.M) and "__global__" not in strip(sources[HEADER])
    from omnivggt_official_amd import build as B
    assert tuple(B.EXACT_UNITS) == UNITS and all(B.EXTRA_FLAGS[u] == ["-ffp-contract=off"] for u in UNITS)


def strip_keep_strings(src):
    """Comments -> nothing; the quoted file name of an #include stays (strip() blanks string literals)."""
    return re.sub(r"//[^\n]*|/\*.*?\*/", "", src, flags=re.S)
