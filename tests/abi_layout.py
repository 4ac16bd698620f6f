"""The C side of include/omnivggt_hip.h as gcc sees it, against the ctypes mirrors of omnivggt_official_amd.lib (host tests)."""
import ctypes
import os
import subprocess
import tempfile

HEADER = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "omnivggt_hip.h")


def check(structs, ints=(), doubles=(), rename=None):
    """structs: {C struct name: ctypes class}; ints / doubles: names of integer / double-valued macros and enumerators of the header;
    rename: {ctypes field name: C member name} where the two differ. Compiles a C99 program against the header that prints sizeof
    and every member's offset, asserts them against ctypes, and -> (the ints' values, the doubles' values read back from %.17g)."""
    member = lambda n: (rename or {}).get(n, n)
    src = '#include <stdio.h>\n#include <stddef.h>\n#include "%s"\nint main(void){\n' % HEADER
    for cname, cls in structs.items():
        src += 'printf("%%zu\\n", sizeof(%s));\n' % cname
        for n, _ in cls._fields_:
            src += 'printf("%%zu\\n", offsetof(%s, %s));\n' % (cname, member(n))
    for name in ints:
        src += 'printf("%%lld\\n", (long long)%s);\n' % name
    for name in doubles:
        src += 'printf("%%.17g\\n", (double)%s);\n' % name
    src += "return 0;}\n"
    with tempfile.TemporaryDirectory() as d:
        c, exe = os.path.join(d, "t.c"), os.path.join(d, "t")
        with open(c, "w") as f:
            f.write(src)
        subprocess.check_call(["gcc", "-std=c99", c, "-o", exe])
        out = iter(subprocess.check_output([exe]).decode().split())
    for cname, cls in structs.items():
        assert int(next(out)) == ctypes.sizeof(cls), cname
        for n, _ in cls._fields_:
            assert int(next(out)) == getattr(cls, n).offset, (cname, n)
    return [int(next(out)) for _ in ints], [float(next(out)) for _ in doubles]
