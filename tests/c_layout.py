"""What the C compiler makes of include/care_hip.h: the values of sizeof / offsetof / constant expressions, for the tests
that hold the ctypes mirrors of care_amd/_lib.py against the header."""
import os
import subprocess
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def c_layout(expr_list):
    """[int(value of e) for e in expr_list]: integer expressions of C over the header, compiled with gcc and run."""
    with tempfile.TemporaryDirectory() as td:
        src = os.path.join(td, "sz.c")
        open(src, "w").write('#include <stdio.h>\n#include <stddef.h>\n#include "care_hip.h"\nint main(void) {\n'
                             + "".join('  printf("%lld\\n", (long long)({}));\n'.format(e) for e in expr_list)
                             + "  return 0;\n}\n")
        subprocess.run(["gcc", "-I", os.path.join(ROOT, "include"), src, "-o", os.path.join(td, "sz")], check=True)
        return [int(v) for v in subprocess.run([os.path.join(td, "sz")], capture_output=True, text=True, check=True).stdout.split()]
