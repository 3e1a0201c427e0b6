"""What every per-feature CPU test asserts of its own entry points (tests/test_*_cpu.py), in one place: the ABI number, and that the
header, _lib's table read from it, the built library and the header's changelog agree on each symbol."""
import os
import re
import shutil
import subprocess

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ABI = 15   # the one place the tests spell the number


def header_text():
    return open(os.path.join(REPO, "include", "trajopt_hip.h")).read()


def check_abi_entries(entries):
    """The header's ABI number is _lib's, the loaded library's and ABI; each of `entries` is declared in the header, with as many
    arguments as _lib.SIGNATURES holds for it, is exported by the library, and is named by the changelog in front of
    `#define TOHIP_ABI_VERSION`.  -> (header text, that changelog) for what a test asserts beyond this."""
    from trajectory_optimization_amd import _lib
    header = header_text()
    assert f"#define TOHIP_ABI_VERSION {ABI}\n" in header and _lib.ABI_VERSION == ABI == _lib.lib().tohip_abi_version()
    before = header.split("#define TOHIP_ABI_VERSION")[0]
    for sym in entries:
        decl = re.search(r"\b(?:int|size_t)\s+" + sym + r"\(([^;]*)\);", header)
        assert decl, sym
        n_args = len([a for a in decl.group(1).split(",") if a.strip()])
        assert sym in _lib.SIGNATURES and len(_lib.SIGNATURES[sym][1]) == n_args, sym
        assert hasattr(_lib.lib(), sym), sym
        assert re.search(r"\b" + sym + r"\b", before), sym   # the changelog line
    return header, before


def c_layouts(structs, tmp_path):
    """{C struct name: field names} -> {C struct name: {"sizeof": bytes, field: offset}} as the host C compiler lays the header's
    structs out: one program of sizeof / offsetof lines, compiled against include/trajopt_hip.h and run."""
    cc = shutil.which("cc") or shutil.which("gcc") or shutil.which("clang") or "/opt/rocm/llvm/bin/clang"   # (the library's toolchain)
    lines = ['#include <stdio.h>', '#include <stddef.h>', '#include "trajopt_hip.h"', "int main(void) {"]
    for name, fields in structs.items():
        lines.append(f'    printf("{name} sizeof %zu\\n", sizeof({name}));')
        lines += [f'    printf("{name} {f} %zu\\n", offsetof({name}, {f}));' for f in fields]
    lines += ["    return 0;", "}"]
    src, exe = tmp_path / "layout.c", tmp_path / "layout"
    src.write_text("\n".join(lines) + "\n")
    subprocess.check_call([cc, "-std=c99", "-I", os.path.join(REPO, "include"), str(src), "-o", str(exe)])
    got = {name: {} for name in structs}
    for line in subprocess.check_output([str(exe)], text=True).splitlines():
        name, key, value = line.split()
        got[name][key] = int(value)
    return got
