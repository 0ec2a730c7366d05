"""CPU tests of the header reader (orb_slam2_aruco_amd/header.py): gcc's own layout of every record and value of every constant of
include/orbfe.h, ten prototypes written out by hand, the prototypes binding.load() installs, and the declarations it must refuse."""
import ctypes as C
import os
import re
import subprocess

import pytest

from orb_slam2_aruco_amd import binding, header

CODE = re.sub(r"/\*.*?\*/", "", open(header.HEADER_PATH).read(), flags=re.S)
vp, i32, f32, f64, sz, cp = C.c_void_p, C.c_int, C.c_float, C.c_double, C.c_size_t, C.c_char_p
NAMED = {     # restype, argtypes: from the hand-written tables the reader replaced
    "orbfe_fuse_search": (i32, [vp, vp, i32, i32, i32, vp, vp, vp, vp, vp, vp, vp, i32, vp, vp, vp, vp, vp, i32, f32, f32, f64, vp, vp, i32]),
    "orbfe_sim3_solve_batch_device": (i32, [vp, vp, i32, vp, vp, vp, vp, vp, i32, vp, vp, vp, i32, i32, f64, i32, i32, vp, vp, vp, vp]),
    "orbfe_corner_subpix": (i32, [vp, i32, i32, sz, vp, i32, i32, i32, f64, i32]),
    "orbfe_lba_scratch_bytes": (sz, [i32] * 5),
    "orbfe_extractor_get_scale_factor": (f32, [vp]),
    "orbfe_last_error": (cp, []),
    "orbfe_extractor_destroy": (None, [vp]),
    "orbfe_device_alloc": (vp, [i32, sz]),
    "orbfe_aruco_create": (vp, [cp, i32]),
    "orbfe_pipeline_gather_plan": (i32, [i32, i32, i32, i32, i32, sz, vp, i32]),
}


# no record of the header needs padding today: this one does, in front of `d` and at its end
PADDED = "typedef struct orbfe_padded { char tag[3]; double d; int32_t n; uint8_t m[2][3]; uint16_t last; } orbfe_padded;"


def test_records_and_constants_equal_the_compilers(tmp_path, monkeypatch):
    """one C program against the header prints sizeof and every offsetof of every record (and of PADDED) and the value of every
    ORBFE_* constant; the names of the records and constants are found here, not taken from the reader"""
    names = re.findall(r"\}\s*(orbfe_\w+)\s*;", CODE)
    consts = [n for n in re.findall(r"#define\s+ORBFE_(\w+)", CODE) if n != "H"]
    assert sorted(names) == sorted(header.records) and sorted(consts) == sorted(header.defines)
    monkeypatch.setitem(header.records, "orbfe_padded", header._parse(PADDED)[1]["orbfe_padded"])
    names.append("orbfe_padded")
    lines = ['#include <stdio.h>', '#include "orbfe.h"', PADDED, 'int main(void) {']
    for r in names:
        lines.append('printf("%s %%zu\\n", sizeof(%s));' % (r, r))
        lines += ['printf("%s.%s %%zu %%zu\\n", offsetof(%s, %s), sizeof(((%s*)0)->%s));' % (r, f, r, f, r, f) for f, _, _ in header.records[r]]
    lines += ['printf("#%s %%lld\\n", (long long)(ORBFE_%s));' % (n, n) for n in consts] + ["return 0; }"]
    (tmp_path / "layout.c").write_text("\n".join(lines))
    subprocess.check_call(["gcc", "-I", os.path.dirname(header.HEADER_PATH), str(tmp_path / "layout.c"), "-o", str(tmp_path / "layout")])
    want = {l.split()[0]: [int(v) for v in l.split()[1:]] for l in subprocess.check_output([str(tmp_path / "layout")], text=True).splitlines()}
    got = {"#" + n: [v] for n, v in header.defines.items()}
    for r in names:
        dt, st = header.dtype(r), header.structure(r)
        assert dt.itemsize == C.sizeof(st) == want[r][0], r
        got[r] = [dt.itemsize]
        for f, _, _ in header.records[r]:
            assert (dt.fields[f][1], dt.fields[f][0].itemsize) == (getattr(st, f).offset, getattr(st, f).size), (r, f)
            got[r + "." + f] = [dt.fields[f][1], dt.fields[f][0].itemsize]
    assert got == want and want["orbfe_padded.d"] == [8, 8] and want["orbfe_padded"] == [32]


@pytest.mark.parametrize("name", sorted(NAMED))
def test_named_prototypes(name):
    assert header.functions[name] == NAMED[name]


def test_every_exported_function_carries_its_declared_prototype():
    if not os.path.exists(binding.LIB_PATH):
        __import__("__graft_entry__").build()
    L = binding.load()
    for name, (restype, argtypes) in header.functions.items():
        params = re.search(r"\b%s\s*\(([^()]*)\)" % name, CODE).group(1)
        declared = 0 if params.strip() == "void" else params.count(",") + 1
        assert hasattr(L, name), name
        assert len(getattr(L, name).argtypes) == len(argtypes) == declared and getattr(L, name).restype == restype, name


@pytest.mark.parametrize("text", [
    pytest.param("int orbfe_f(wchar_t x);", id="unknown_type"),
    pytest.param("int orbfe_f(other_t* x);", id="pointer_to_unknown_type"),
    pytest.param("int orbfe_f(int (*callback)(int), int n);", id="function_pointer"),
    pytest.param("int orbfe_f(const char* format, ...);", id="varargs"),
    pytest.param("int orbfe_f(int);", id="unnamed_parameter"),
    pytest.param("typedef struct orbfe_r { struct { int a; } in; } orbfe_r;", id="nested_struct"),
    pytest.param("typedef struct orbfe_r { int* p; } orbfe_r;", id="pointer_field"),
    pytest.param("#define ORBFE_X 1.5", id="non_integer_constant"),
    pytest.param("#define CALL orbfe_g(0)\nint orbfe_f(int x);", id="call_that_is_no_declaration"),
])
def test_reader_refuses_what_it_cannot_read(text):
    with pytest.raises(header.HeaderError):
        header._parse(text)


def test_reader_reads_a_small_header():
    assert header._parse("#define ORBFE_X (-3)\nconst char* orbfe_f(const float K[4], size_t n);") == (
        {"orbfe_f": (cp, [vp, sz])}, {}, {"X": -3})
