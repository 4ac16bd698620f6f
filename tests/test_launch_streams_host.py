"""CPU only: where csrc/ queues its work, read from the source. The header promises for every entry "never allocates or frees, never
synchronises the device" and that the work goes to the caller's stream. test_gpu_stream_contract.py gates every entry behind a blocked side
stream; what that cannot see -- a first-stage clear queued on the null stream that happens to run early enough -- the source shows:

 1. every OVG_LAUNCH(kernel, grid, block, lds, STREAM, args...) in csrc/ (.hip, .h, .inc) names as its fifth argument the hipStream_t
    parameter of an enclosing function, a local initialised from a `void*` parameter of it (hipStream_t st = static_cast<hipStream_t>(stream)),
    or that cast itself -- never a literal, nullptr or a named default stream
 2. no raw launch (hipLaunchKernelGGL outside the macro's definition, <<< >>>, hipModuleLaunchKernel, ...) anywhere in csrc/
 3. no hipMalloc* / hipFree* / hip*Synchronize and no hipMemcpy* / hipMemset* that is not *Async
    (one commented exception: the two hipMemcpyToSymbol of the timeline lab knob in ovg_gemm.hip, compiled only under OVG_GEMM_TIMELINE)
 4. the parser is proved on synthetic snippets: one good, and a literal 0, a missing stream and a raw launch, each of which it must reject
 5. "the library holds NO mutable state" but a lock-guarded memo of per-device kernel opt-ins: every function-local `static` that is
    not const is a std::mutex, or is touched only behind a std::lock_guard of its function or handed to opt_in_big_lds, which takes one
"""
import os
import re

CSRC = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "omnivggt-official_amd", "csrc")
SUFFIXES = (".hip", ".h", ".inc")

# (file, call) -> why it may stay. The lab knob ovg_lab_gemm_timeline sets two __device__ symbols; it exists only in a library built with
# -DOVG_GEMM_TIMELINE (tools/lab), is not declared in the header and is no entry of the ABI.
SYNC_EXCEPTIONS = {("ovg_gemm.hip", "hipMemcpyToSymbol"): "timeline lab knob, #ifdef OVG_GEMM_TIMELINE only"}

FORBIDDEN = [
    (re.compile(r"\bhipMalloc\w*\s*\("), "allocates"),
    (re.compile(r"\bhipHostMalloc\w*\s*\("), "allocates"),
    (re.compile(r"\bhipFree\w*\s*\("), "frees"),
    (re.compile(r"\bhipHostFree\w*\s*\("), "frees"),
    (re.compile(r"\bhip\w*Synchronize\s*\("), "synchronises"),
    (re.compile(r"\bhipMemcpy\w*\s*\("), "copies"),
    (re.compile(r"\bhipMemset\w*\s*\("), "clears"),
]
RAW_LAUNCH = re.compile(r"\bhipLaunchKernelGGL\b|<<<|\bhipModuleLaunchKernel\b|\bhipLaunchKernel\b|\bhipLaunchCooperativeKernel\b|\bhipExtLaunch\w*")
NOT_A_STREAM = re.compile(r"^(0[xX]?[0-9a-fA-F]*[uUlL]*|\d+|nullptr|NULL|hipStreamLegacy|hipStreamPerThread|hipStreamDefault|)$")


class LaunchError(AssertionError):
    pass


def strip(src):
    """Comments, string and character literals -> spaces, offsets and newlines kept."""
    out, i, n = list(src), 0, len(src)

    def blank(a, b):
        for j in range(a, b):
            if out[j] != "\n":
                out[j] = " "
    while i < n:
        c = src[i]
        if src.startswith("//", i):
            j = i
            while True:                                   # a backslash-newline continues a line comment
                k = src.find("\n", j)
                k = n if k < 0 else k
                if k < n and src[k - 1] == "\\":
                    j = k + 1
                    continue
                break
            blank(i, k)
            i = k
        elif src.startswith("/*", i):
            k = src.find("*/", i + 2)
            k = n if k < 0 else k + 2
            blank(i, k)
            i = k
        elif c in "\"'":
            if c == "'" and i > 0 and (src[i - 1].isalnum()):     # digit separator 1'000
                i += 1
                continue
            j = i + 1
            while j < n and src[j] != c:
                j += 2 if src[j] == "\\" else 1
            blank(i + 1, min(j, n))
            i = j + 1
        else:
            i += 1
    return "".join(out)


def split_args(text):
    """Top-level commas of a balanced argument list -> stripped arguments. ( [ { nest; < > do not (a template kernel name with a comma has
    to stand in parentheses for the preprocessor as well)."""
    args, depth, cur = [], 0, []
    for ch in text:
        if ch in "([{":
            depth += 1
        elif ch in ")]}":
            depth -= 1
            if depth < 0:
                raise LaunchError("unbalanced argument list: %r" % text[:80])
        if ch == "," and depth == 0:
            args.append("".join(cur).strip())
            cur = []
        else:
            cur.append(ch)
    if depth:
        raise LaunchError("unbalanced argument list: %r" % text[:80])
    args.append("".join(cur).strip())
    return args


def launches(clean):
    """-> [(offset, [arguments])] of every OVG_LAUNCH(...) use in comment-free source (the #define itself is no use)."""
    found = []
    for m in re.finditer(r"\bOVG_LAUNCH\s*\(", clean):
        line0 = clean.rfind("\n", 0, m.start()) + 1
        if re.match(r"\s*#\s*define\b", clean[line0:m.start()]):
            continue
        depth, j = 1, m.end()
        while j < len(clean) and depth:
            depth += {"(": 1, ")": -1}.get(clean[j], 0)
            j += 1
        if depth:
            raise LaunchError("OVG_LAUNCH at offset %d: parentheses do not balance" % m.start())
        found.append((m.start(), split_args(clean[m.end():j - 1])))
    return found


def kernel_name(arg):
    """`name`, `ns::name` or `(name<T, 4>)` -> the name without its template arguments; anything else raises."""
    a = arg.strip()
    while a.startswith("(") and a.endswith(")"):
        a = a[1:-1].strip()
    m = re.match(r"^([A-Za-z_]\w*(?:::[A-Za-z_]\w*)*)\s*(<.*>)?$", a, re.S)
    if not m:
        raise LaunchError("kernel name does not parse: %r" % arg)
    return m.group(1)


def enclosing_headers(clean, pos):
    """Text in front of every `{` that is still open at pos, innermost last (function signatures, lambdas, namespaces, control flow), and the
    offset of the outermost one that has a parameter list (the function body the launch sits in)."""
    stack = []
    for m in re.finditer(r"[{}]", clean[:pos]):
        if m.group() == "{":
            stack.append(m.start())
        elif stack:
            stack.pop()
    heads, body = [], None
    for b in stack:
        a = max(clean.rfind(ch, 0, b) for ch in ";{}") + 1
        h = clean[a:b]
        heads.append(h)
        if body is None and ")" in h and not re.match(r"\s*(namespace\b|extern\b\s*$)", h):
            body = b
    return heads, body


PARAM_STREAM = re.compile(r"\bhipStream_t\s+(\w+)\s*[,)]")
PARAM_VOID = re.compile(r"\bvoid\s*\*\s*(\w+)\s*[,)]")
CAST = r"(?:static_cast\s*<\s*hipStream_t\s*>\s*\(\s*(\w+)\s*\)|reinterpret_cast\s*<\s*hipStream_t\s*>\s*\(\s*(\w+)\s*\)|\(\s*hipStream_t\s*\)\s*(\w+))"
LOCAL_STREAM = re.compile(r"\bhipStream_t\s+(\w+)\s*(?:=|\(|\{)\s*" + CAST)


def check_stream_argument(clean, pos, args, where):
    if len(args) < 5:
        raise LaunchError("%s: OVG_LAUNCH with %d arguments has no stream" % (where, len(args)))
    kernel_name(args[0])
    st = args[4]
    if NOT_A_STREAM.match(st):
        raise LaunchError("%s: the stream argument is %r" % (where, st))
    heads, body = enclosing_headers(clean, pos)
    if body is None:
        raise LaunchError("%s: launch outside any function" % where)
    params, voids = set(), set()
    for h in heads:
        params.update(PARAM_STREAM.findall(h))
        voids.update(PARAM_VOID.findall(h))
    for m in LOCAL_STREAM.finditer(clean[body:pos]):
        src = next(g for g in m.groups()[1:] if g)
        if src in voids:
            params.add(m.group(1))
    m = re.match(r"^" + CAST + r"$", st)
    if m:
        src = next(g for g in m.groups() if g)
        if src in voids:
            return src
        raise LaunchError("%s: the stream argument casts %r, which is no void* parameter of the enclosing function" % (where, src))
    if not re.match(r"^[A-Za-z_]\w*$", st):
        raise LaunchError("%s: the stream argument %r is not an identifier" % (where, st))
    if st not in params:
        raise LaunchError("%s: the stream argument %r is neither a hipStream_t parameter nor a local made from the entry's void* stream "
                          "(known here: %s)" % (where, st, sorted(params)))
    return st


def check_source(name, src, exceptions=SYNC_EXCEPTIONS):
    """All four rules on one file's text -> number of launches checked; raises LaunchError naming file and line."""
    clean = strip(src)

    def at(pos):
        return "%s:%d" % (name, clean.count("\n", 0, pos) + 1)
    for m in RAW_LAUNCH.finditer(clean):
        line0 = clean.rfind("\n", 0, m.start()) + 1
        if m.group() == "hipLaunchKernelGGL" and re.match(r"\s*#\s*define\s+OVG_LAUNCH\b", clean[line0:m.start()]):
            continue
        raise LaunchError("%s: raw launch %r outside OVG_LAUNCH" % (at(m.start()), m.group()))
    for rx, verb in FORBIDDEN:
        for m in rx.finditer(clean):
            call = m.group().rstrip("( \t\n")
            if call.endswith("Async") and verb in ("copies", "clears"):
                continue
            if (os.path.basename(name), call) in exceptions:
                continue
            raise LaunchError("%s: %s %s behind an entry that promises not to" % (at(m.start()), call, verb))
    found = launches(clean)
    for pos, args in found:
        check_stream_argument(clean, pos, args, at(pos))
    return len(found)


def _files():
    for f in sorted(os.listdir(CSRC)):
        if f.endswith(SUFFIXES):
            with open(os.path.join(CSRC, f)) as fh:
                yield f, fh.read()


# =============================================================================================
# the parser, proved on synthetic snippets
# =============================================================================================
GOOD = '''
#define OVG_LAUNCH(...) do { (void)hipGetLastError(); hipLaunchKernelGGL(__VA_ARGS__); } while (0)
namespace {
template <typename T, int N> __global__ void k(T* p, int n) {}
// OVG_LAUNCH(k, 1, 1, 0, 0) in a comment is no launch, nor is "hipMalloc(" in a string
const char* s = "hipMalloc( <<< ";
int inner(const P& p, hipStream_t st, bool big) {
  if (big) { OVG_LAUNCH((k<float, 4>), dim3(f(p.a, 2), 1), dim3(256), 0, st, p.x, (int)p.n); }
  auto again = [&](int i) { OVG_LAUNCH(ns::plain, grid, block, lds_bytes(i, 2), st, p.x); };
  return 0;
}
}  // namespace
extern "C" int ovg_thing(const P* p, void* stream) {
  hipStream_t s2 = static_cast<hipStream_t>(stream);
  for (int i = 0; i < 3; ++i) { OVG_LAUNCH(plain, dim3(1), dim3(64), 0, s2, p->x); }
  OVG_LAUNCH(plain, dim3(1), dim3(64), 0, static_cast<hipStream_t>(stream), p->x);
  hipMemsetAsync(p->x, 0, 4, s2);
  return inner(*p, s2, true);
}
'''
BAD = {
    "a literal 0": ('extern "C" int e(const P* p, void* stream) {\n  OVG_LAUNCH(plain, dim3(1), dim3(64), 0, 0, p->x);\n  return 0;\n}\n', "stream argument is '0'"),
    "a missing stream": ('extern "C" int e(const P* p, void* stream) {\n  OVG_LAUNCH(plain, dim3(1), dim3(64), 0);\n  return 0;\n}\n', "has no stream"),
    "a raw launch": ('extern "C" int e(const P* p, void* stream) {\n  hipLaunchKernelGGL(plain, dim3(1), dim3(64), 0, (hipStream_t)stream, p->x);\n  return 0;\n}\n',
                     "raw launch"),
    "a triple-chevron launch": ('int e(P* p, hipStream_t st) {\n  plain<<<1, 64, 0, st>>>(p->x);\n  return 0;\n}\n', "raw launch"),
    "nullptr": ('int e(P* p, hipStream_t st) {\n  OVG_LAUNCH(plain, 1, 64, 0, nullptr, p->x);\n  return 0;\n}\n', "stream argument is 'nullptr'"),
    "a named default stream": ('int e(P* p, hipStream_t st) {\n  OVG_LAUNCH(plain, 1, 64, 0, hipStreamPerThread, p->x);\n  return 0;\n}\n', "stream argument is"),
    "someone else's stream": ('hipStream_t g_side;\nint e(P* p, hipStream_t st) {\n  OVG_LAUNCH(plain, 1, 64, 0, g_side, p->x);\n  return 0;\n}\n', "neither a hipStream_t parameter"),
    "a local made from nothing": ('int e(P* p, void* stream) {\n  hipStream_t st = static_cast<hipStream_t>(other);\n  OVG_LAUNCH(plain, 1, 64, 0, st, p->x);\n  return 0;\n}\n',
                                  "neither a hipStream_t parameter"),
    "unbalanced parentheses": ('int e(P* p, hipStream_t st) {\n  OVG_LAUNCH(plain, dim3(1, 64, 0, st, p->x;\n  return 0;\n}\n', "do not balance"),
    "a synchronise": ('int e(P* p, hipStream_t st) {\n  OVG_LAUNCH(plain, 1, 64, 0, st, p->x);\n  hipStreamSynchronize(st);\n  return 0;\n}\n', "synchronises"),
    "a device synchronise": ('int e(P* p, hipStream_t st) {\n  hipDeviceSynchronize();\n  return 0;\n}\n', "synchronises"),
    "an allocation": ('int e(P* p, hipStream_t st) {\n  void* q; hipMallocAsync(&q, 4, st);\n  return 0;\n}\n', "allocates"),
    "a free": ('int e(P* p, hipStream_t st) {\n  hipFree(p->x);\n  return 0;\n}\n', "frees"),
    "a blocking copy": ('int e(P* p, hipStream_t st) {\n  hipMemcpy(p->x, p->y, 4, hipMemcpyDeviceToHost);\n  return 0;\n}\n', "copies"),
    "a blocking clear": ('int e(P* p, hipStream_t st) {\n  hipMemset(p->x, 0, 4);\n  return 0;\n}\n', "clears"),
}


def test_parser_accepts_the_good_snippet_and_counts_its_launches():
    assert check_source("good.hip", GOOD) == 4
    clean = strip(GOOD)
    names = [kernel_name(a[0]) for _, a in launches(clean)]
    assert names == ["k", "ns::plain", "plain", "plain"], names
    assert [a[4] for _, a in launches(clean)] == ["st", "st", "s2", "static_cast<hipStream_t>(stream)"]
    assert split_args("(k<float, 4>), dim3(f(a, 2), 1), x[3, 4], {1, 2}") == ["(k<float, 4>)", "dim3(f(a, 2), 1)", "x[3, 4]", "{1, 2}"]


def test_parser_rejects_every_bad_snippet():
    for what, (src, msg) in BAD.items():
        try:
            check_source("bad.hip", src)
        except LaunchError as e:
            assert msg in str(e), (what, str(e))
            assert "bad.hip:" in str(e) or "balance" in str(e), (what, str(e))
        else:
            raise AssertionError("the parser accepted %s" % what)


def test_exception_is_by_file_and_call_only():
    src = 'int lab(void* b) {\n  hipMemcpyToSymbol(HIP_SYMBOL(g), &b, 8);\n  return 0;\n}\n'
    assert check_source("ovg_gemm.hip", src) == 0
    try:
        check_source("ovg_attn.hip", src)
    except LaunchError as e:
        assert "copies" in str(e)
    else:
        raise AssertionError("hipMemcpyToSymbol passed outside its one file")


# =============================================================================================
# csrc/
# =============================================================================================
def test_every_launch_in_csrc_goes_to_the_callers_stream():
    total, per_file = 0, {}
    for name, src in _files():
        n = check_source(name, src)
        per_file[name] = n
        total += n
    print("OVG_LAUNCH sites: %d in %d files: %s" % (total, len(per_file), {k: v for k, v in per_file.items() if v}), flush=True)
    assert total >= 100, "only %d launch sites found: the scan lost csrc/" % total
    assert sum(1 for v in per_file.values() if v) >= 15, per_file


def test_macro_is_defined_once_and_is_the_only_raw_launch():
    defs = []
    for name, src in _files():
        for m in re.finditer(r"^\s*#\s*define\s+OVG_LAUNCH\b.*$", strip(src), re.M):
            defs.append((name, m.group().strip()))
    assert len(defs) == 1 and defs[0][0] == "ovg_common.h", defs
    assert "hipLaunchKernelGGL(__VA_ARGS__)" in defs[0][1], defs


def test_timeline_knob_exception_is_what_it_says():
    """The two hipMemcpyToSymbol calls sit inside #ifdef OVG_GEMM_TIMELINE and nowhere else; the default build does not define it."""
    with open(os.path.join(CSRC, "ovg_gemm.hip")) as fh:
        clean = strip(fh.read())
    calls = [m.start() for m in re.finditer(r"\bhipMemcpyToSymbol\s*\(", clean)]
    assert len(calls) == 2, calls
    for pos in calls:
        a = clean.rfind("#ifdef OVG_GEMM_TIMELINE", 0, pos)
        assert a >= 0 and "#endif" not in clean[a:pos], "hipMemcpyToSymbol outside the timeline block"
    for name, src in _files():
        if name != "ovg_gemm.hip":
            assert "hipMemcpyToSymbol" not in strip(src), name
    with open(os.path.join(os.path.dirname(CSRC), "build.py")) as fh:
        build = fh.read()
    assert "OVG_GEMM_TIMELINE" not in build, "the default build must not compile the lab knob"


# =============================================================================================
# mutable statics
# =============================================================================================
STATIC_LOCAL = re.compile(r"^[ \t]+static[ \t]+(?!const\b|constexpr\b|OVG_DEV\b|__device__\b|inline\b)([^;=({]*?)\b(\w+)\s*(?:\[[^\]]*\])?\s*(?:=|;|\{)", re.M)


def unguarded_statics(name, src):
    """-> ["file:line name: why"] for every mutable function-local static that is reachable without the lock."""
    clean = strip(src)
    bad = []
    for m in STATIC_LOCAL.finditer(clean):
        typ, var = m.group(1).strip(), m.group(2)
        if "std::mutex" in typ:
            continue
        where = "%s:%d %s" % (name, clean.count("\n", 0, m.start()) + 1, var)
        _, body = enclosing_headers(clean, m.start())
        if body is None:
            bad.append(where + ": not inside a function")
            continue
        depth, end = 0, len(clean)
        for b in re.finditer(r"[{}]", clean[body:]):
            depth += 1 if b.group() == "{" else -1
            if depth == 0:
                end = body + b.end()
                break
        for use in re.finditer(r"\b%s\b" % re.escape(var), clean[body:end]):
            pos = body + use.start()
            if pos == m.start(2):
                continue
            locked = re.search(r"std::lock_guard\s*<\s*std::mutex\s*>", clean[body:pos]) is not None
            handed = re.search(r"opt_in_big_lds\s*\(\s*$", clean[max(body, pos - 40):pos]) is not None
            if not (locked or handed):
                bad.append("%s: used at line %d without the lock" % (where, clean.count("\n", 0, pos) + 1))
    return bad


def test_mutable_statics_are_guarded():
    good = ('int memo(int dev) {\n  static std::mutex mu;\n  static unsigned done = 0u;\n  static const int n = 3;\n  std::lock_guard<std::mutex> lock(mu);\n'
            '  if ((done >> dev) & 1u) return n;\n  done |= 1u << dev;\n  return 0;\n}\n'
            'int entry(int which, int dev) {\n  static unsigned opted[4] = {0u, 0u, 0u, 0u};\n  return opt_in_big_lds(opted[which], fn, 4, dev);\n}\n'
            'struct S {\n  static constexpr int k = 2;\n  static OVG_DEV int f(int x) { return static_cast<int>(x); }\n};\n')
    assert unguarded_statics("good.hip", good) == []
    racy = 'int entry(int dev) {\n  static unsigned opted[2] = {0u, 0u};\n  if (!((opted[0] >> dev) & 1u)) opted[0] |= 1u << dev;\n  return 0;\n}\n'
    found = unguarded_statics("racy.hip", racy)
    assert len(found) == 2 and "racy.hip:2 opted" in found[0] and "line 3" in found[0], found
    late = 'int entry(int dev) {\n  static std::mutex mu;\n  static int seen = 0;\n  if (seen) return 1;\n  std::lock_guard<std::mutex> lock(mu);\n  seen = 1;\n  return 0;\n}\n'
    assert len(unguarded_statics("late.hip", late)) == 1              # the read in front of the lock
    total = []
    for name, src in _files():
        total += unguarded_statics(name, src)
    assert total == [], total
    with open(os.path.join(CSRC, "ovg_head.hip")) as fh:
        head = strip(fh.read())
    assert len(re.findall(r"opt_in_big_lds\s*\(\s*opted\[", head)) == 2 and "std::lock_guard<std::mutex>" in head
