"""The C boundary without a GPU and without the built library: unmore_amd._lib reads its argument and return types from include/umr.h,
and its ctypes.Structure mirrors are compared, field by field, with what a host C compiler makes of the same header."""
import ctypes
import os
import re
import shlex
import shutil
import subprocess

import pytest

from unmore_amd import _lib as L

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INCLUDE = os.path.join(ROOT, "include")

vp, i32, i64, f32 = ctypes.c_void_p, ctypes.c_int32, ctypes.c_int64, ctypes.c_float


def _header():
    return open(os.path.join(INCLUDE, "umr.h")).read()


def test_every_struct_of_the_header_has_a_mirror():
    structs = re.findall(r"typedef\s+struct\s+(umr_\w+)", _header())
    assert len(structs) == len(set(structs)) == 10
    assert set(structs) == set(L.MIRRORS)
    assert len(set(L.MIRRORS.values())) == len(L.MIRRORS)


def test_every_mirror_has_the_fields_of_its_struct_in_order():
    """A field left out of a mirror can hide in alignment padding, where no size or offset moves: compare the names too."""
    text = re.sub(r"/\*.*?\*/", " ", _header(), flags=re.S)
    bodies = dict((name, body) for body, name in re.findall(r"typedef\s+struct\s+\w+\s*\{([^{}]*)\}\s*(umr_\w+)\s*;", text))
    assert set(bodies) == set(L.MIRRORS)
    for cname, mirror in L.MIRRORS.items():
        declared = [re.search(r"(\w+)\s*(\[\d+\])?\s*$", d).group(1) for decl in bodies[cname].split(";") if decl.strip() for d in decl.split(",")]
        assert declared == [f for f, _ in mirror._fields_], cname


def _compiler():
    """the first of $CC, cc, gcc, clang and the clang that ships beside hipcc"""
    hipcc = shutil.which("hipcc") or os.path.join(os.environ.get("ROCM_PATH", "/opt/rocm"), "bin", "hipcc")
    beside = os.path.join(os.path.dirname(os.path.dirname(os.path.realpath(hipcc))), "lib", "llvm", "bin", "clang")
    for cand in (os.environ.get("CC"), "cc", "gcc", "clang", beside):
        words = shlex.split(cand) if cand else []
        if words and shutil.which(words[0]):
            return words
    pytest.fail("no host C compiler found ($CC, cc, gcc, clang, ROCm's clang): the layout of the struct mirrors cannot be checked")


def test_mirrors_match_the_layout_a_c_compiler_gives(tmp_path):
    lines, want = [], {}
    for cname, mirror in L.MIRRORS.items():
        lines.append(f'    printf("{cname} %zu\\n", sizeof({cname}));')
        want[cname] = ctypes.sizeof(mirror)
        for field, _ in mirror._fields_:
            lines.append(f'    printf("{cname}.{field} %zu %zu\\n", offsetof({cname}, {field}), sizeof((({cname}*)0)->{field}));')
            want[f"{cname}.{field}"] = (getattr(mirror, field).offset, getattr(mirror, field).size)
    src, exe = tmp_path / "layout.c", tmp_path / "layout"
    src.write_text('#include <stddef.h>\n#include <stdio.h>\n#include "umr.h"\nint main(void) {\n' + "\n".join(lines) + "\n    return 0;\n}\n")
    cc = subprocess.run(_compiler() + ["-I", INCLUDE, str(src), "-o", str(exe)], capture_output=True, text=True)
    assert cc.returncode == 0, f"a mirror names a field its C struct lacks, or the header does not compile as C:\n{cc.stderr}"
    got = {}
    for line in subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.splitlines():
        key, *nums = line.split()
        got[key] = int(nums[0]) if len(nums) == 1 else (int(nums[0]), int(nums[1]))
    wrong = {k: {"C": got[k], "ctypes": want[k]} for k in want if got[k] != want[k]}
    assert not wrong, f"(offset, size) per field, size per struct: {wrong}"
    assert len(got) == len(want) == 10 + sum(len(m._fields_) for m in L.MIRRORS.values())


# written out by hand from include/umr.h, one for every rule of the reader: it is not tested against itself
PINNED = {
    "umr_mask_iou": [vp, vp, i32, i64, vp, vp, vp, vp, vp, vp, i32, i64, i32, i32, i64, i64, vp, vp, vp, vp, vp, i64, vp],
    "umr_box_loss": [vp, i32, i64, i64, i32, i64, vp, vp, i32, f32, f32, f32, f32, f32, i32, i32, f32, vp, vp, i32, vp, vp, vp, vp, vp, vp, vp,
                     i64, vp],
    "umr_center_peaks_certified": [vp, vp, vp, vp, vp, vp, i32, i32, i32, i32, i32, i32, f32, ctypes.c_double, vp],
    "umr_get_debug_option": [ctypes.c_char_p, ctypes.POINTER(ctypes.c_int), ctypes.POINTER(ctypes.c_int)],
    "umr_gemm_nt": [vp, vp],
    "umr_version": [],
    "umr_poly_rle_workspace": [i64, i32, i32, i64],
    "umr_last_error_string": [],
}
PINNED_RETURNS = {"umr_poly_rle_workspace": ctypes.c_int64, "umr_last_error_string": ctypes.c_char_p}


@pytest.mark.parametrize("name", sorted(PINNED))
def test_pinned_signatures(name):
    assert len(PINNED["umr_mask_iou"]) == 23 and len(PINNED["umr_box_loss"]) == 29
    assert L.ARGTYPES[name] == PINNED[name]
    assert L.RESTYPES.get(name) is PINNED_RETURNS.get(name)        # absent: ctypes' default, a C int


def test_every_prototype_of_the_header_is_bound():
    text = re.sub(r"/\*.*?\*/", " ", _header(), flags=re.S)
    text = re.sub(r"typedef\s+struct[^{}]*\{[^{}]*\}[^;]*;", " ", text)
    declared = set(re.findall(r"\b(umr_\w+)\s*\(", text))
    assert len(declared) >= 116
    assert sorted(declared) == L.exported_symbols() and len(L.ARGTYPES) == len(declared)
    int64 = set(re.findall(r"\bint64_t\s+(umr_\w+)\s*\(", text))
    assert len(int64) >= 22 and int64 == {n for n, r in L.RESTYPES.items() if r is ctypes.c_int64}


@pytest.mark.parametrize("decl,names", [("int umr_x(unsigned n);", "unsigned.*umr_x"), ("int umr_x(int64_t);", "umr_x"),
                                        ("size_t umr_x(void);", "size_t.*umr_x"), ("int (*umr_cb)(int a);", "umr_cb")])
def test_a_declaration_outside_the_table_raises_and_names_the_prototype(tmp_path, monkeypatch, decl, names):
    hdr = tmp_path / "umr.h"
    hdr.write_text("/* int umr_in_a_comment(float x); */\n#include <stdint.h>\nint umr_ok(const float* p, int64_t n);\n" + decl + "\n")
    monkeypatch.setattr(L, "HEADER", str(hdr))
    with pytest.raises(RuntimeError, match=names):
        L._read_header()
    hdr.write_text(hdr.read_text().replace(decl, ""))
    assert L._read_header() == ({"umr_ok": [vp, i64]}, {})


def test_a_missing_header_raises(tmp_path, monkeypatch):
    monkeypatch.setattr(L, "HEADER", str(tmp_path / "umr.h"))
    with pytest.raises(RuntimeError, match="umr.h is missing"):
        L._read_header()
