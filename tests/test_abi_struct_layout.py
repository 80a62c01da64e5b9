"""CPU: every ctypes mirror of a struct of include/hegpu.h (heongpu_amd/_lib.py) has the header's layout.  Per class a small
C program is written from the class's _fields_, compiled against the header with the host C compiler and run: it prints
sizeof of the struct and offsetof and the size of every named field, which must equal ctypes.sizeof, Cls.<field>.offset
and .size.  A field the header lacks fails the compile; a field the mirror lacks, or fields in another order, show as a
size or offset that differs.  Needs no library: _lib.py is loaded from its file."""
import ctypes
import importlib.util
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CC = next((c for c in (os.environ.get("CC"), "cc", "gcc", "clang") if c and shutil.which(c)), None)

MIRRORS = {
    "PolyStep": "hegpu_poly_step",
    "BootstrapConfig": "hegpu_bootstrap_config",
    "BootstrapPlan": "hegpu_bootstrap_plan",
    "SlimBootstrapConfig": "hegpu_slim_bootstrap_config",
    "SlimBootstrapPlan": "hegpu_slim_bootstrap_plan",
    "LinearFactor": "hegpu_linear_factor",
}


def _mirrors():
    spec = importlib.util.spec_from_file_location("hegpu_lib_mirrors", os.path.join(ROOT, "heongpu_amd", "_lib.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def header_layout(c_name, fields, tmp_path):
    """[sizeof(c_name), offsetof and sizeof of fields[0], of fields[1], ...] as the C compiler lays the header's struct out"""
    lines = ['#include <stddef.h>', '#include <stdio.h>', '#include "hegpu.h"', 'int main(void)', '{',
             f'    printf("%zu\\n", sizeof({c_name}));']
    for f in fields:
        lines.append(f'    printf("%zu %zu\\n", offsetof({c_name}, {f}), sizeof((({c_name}*) 0)->{f}));')
    lines += ['    return 0;', '}', '']
    src, exe = tmp_path / "layout.c", tmp_path / "layout"
    src.write_text("\n".join(lines))
    subprocess.run([CC, "-std=c99", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)],
                   check=True)
    return [int(v) for v in subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.split()]


@pytest.mark.skipif(CC is None, reason="no C compiler is installed")
@pytest.mark.parametrize("cls_name", sorted(MIRRORS))
def test_ctypes_mirror_has_the_headers_layout(cls_name, tmp_path):
    cls = getattr(_mirrors(), cls_name)
    fields = [f[0] for f in cls._fields_]
    want = header_layout(MIRRORS[cls_name], fields, tmp_path)
    got = [ctypes.sizeof(cls)]
    for f in fields:
        got += [getattr(cls, f).offset, getattr(cls, f).size]
    print(cls_name, "header", want, "ctypes", got)
    assert got == want
