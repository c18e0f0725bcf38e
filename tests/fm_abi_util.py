"""What the three FM ABI tests (test_fm_abi.py, test_fm_sampled_abi.py, test_fm_approx_abi.py) share: the functions a header
declares, a numpy array as a C pointer, and the C layout of a struct of include/archon_hip.h."""
import ctypes
import os
import re
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def declared(header):
    src = open(os.path.join(ROOT, "include", header)).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    return set(re.findall(r"\b(archon_[a-z0-9_]+)\s*\(", src))


def p(a):
    return ctypes.c_void_p(a.ctypes.data)


def layout(tmp_path, struct, names):
    """[sizeof(struct), offsetof(struct, name) for every name] as a C compiler sees the header"""
    src = tmp_path / "sz.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "archon_hip.h"\nint main(void){printf("%%zu", sizeof(%s));' % struct
                   + "".join('printf(" %%zu", offsetof(%s, %s));' % (struct, k) for k in names) + "return 0;}\n")
    exe = tmp_path / "sz"
    subprocess.run(["gcc", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)], check=True)
    return [int(t) for t in subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.split()]
