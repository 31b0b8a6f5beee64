"""CPU-side checks of the boundary: the C-ABI library loads, exports every symbol the headers declare, abi.py's prototype
table and struct layouts agree with the headers, and compute entry points fail loudly without a GPU."""
import ctypes as C
import os
import re

import pytest

from riichienv_amd import abi, vecenv

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_library_exports_every_declared_symbol():
    # the drop-in surface + the measurement / test hooks (declared apart: riichi_mi355x_bench.h)
    hdr = open(os.path.join(ROOT, "include", "riichi_mi355x.h")).read() + open(os.path.join(ROOT, "include", "riichi_mi355x_bench.h")).read()
    product = set(re.findall(r"\b(rmj_[a-z_]+)\s*\(", open(os.path.join(ROOT, "include", "riichi_mi355x.h")).read()))
    assert not {s for s in product if s.startswith(("rmj_bench_", "rmj_time_"))}, "measurement hooks belong in riichi_mi355x_bench.h"
    declared = set(re.findall(r"\b(rmj_[a-z_]+)\s*\(", hdr))
    declared -= {"rmj_env"}
    assert declared == set(vecenv.EXPORTS), declared ^ set(vecenv.EXPORTS)
    lib = vecenv.load_lib()
    for sym in declared:
        assert getattr(lib, sym) is not None
    assert b"gfx950" in lib.rmj_version()


def _headers():
    """both headers as one text without comments (product header first)"""
    text = "".join(open(os.path.join(ROOT, "include", h)).read() for h in ("riichi_mi355x.h", "riichi_mi355x_bench.h"))
    return re.sub(r"/\*.*?\*/", " ", text, flags=re.S)


_HANDLES = ("rmj_handle", "rmj_ppo_handle", "rmj_logset_handle", "rmj_logreplay_handle")
_SCALARS = {"int": C.c_int, "float": C.c_float, "double": C.c_double, "char": C.c_char,
            **{f"{u}int{b}_t": getattr(C, f"c_{u}int{b}") for u in ("", "u") for b in (8, 16, 32, 64)}}


def _scalar_kind(t):
    """(size, floating, signed) of a ctypes scalar"""
    return C.sizeof(t), t._type_ in "fdg", t._type_ in "fdg" or t(-1).value < 0


def _is_pointer(t):
    return t in (C.c_void_p, C.c_char_p) or issubclass(t, C._Pointer)


def test_prototype_table_matches_the_headers():
    """abi.PROTOTYPES against every rmj_* prototype the two headers declare: the same names, the same number of arguments, and per
    argument the same kind - a scalar of the same size and signedness, c_void_p for a handle, a pointer for a pointer, and for
    POINTER(S) the class that mirrors the pointed-to struct."""
    protos = re.findall(r"\b(const\s+char\s*\*|int)\s+(rmj_\w+)\s*\(([^)]*)\)\s*;", _headers())
    table = {row[0]: row for row in abi.PROTOTYPES}
    assert len(table) == len(abi.PROTOTYPES), "a name is listed twice"
    assert {name for _, name, _ in protos} == set(table), {name for _, name, _ in protos} ^ set(table)
    assert [name for _, name, _ in protos] == [row[0] for row in abi.PROTOTYPES], "the table is ordered as the headers are"
    for ret, name, params in protos:
        _, argtypes, *restype = table[name]
        if ret != "int":
            assert restype == [C.c_char_p], f"{name}: a const char* result needs restype c_char_p"
        else:
            assert not restype, f"{name}: the header returns int"
        params = [] if params.strip() == "void" else [" ".join(p.split()) for p in params.split(",")]
        assert len(argtypes) == len(params), f"{name}: {len(argtypes)} argtypes for {len(params)} parameters ({params})"
        for i, (param, at) in enumerate(zip(params, argtypes)):
            where = f"{name} argument {i} ({param!r}, {at.__name__})"
            ctype = re.sub(r"\bconst\b", "", param).rsplit(None, 1)[0] if "*" not in param else param
            if "*" in param:
                assert _is_pointer(at), where
                m = re.match(r"(?:const )?(Rmj\w+) ?\*", param)
                if issubclass(at, C._Pointer) and issubclass(at._type_, C.Structure):
                    assert m and at._type_ is abi.STRUCTS.get(m.group(1)), where
            elif ctype.strip() in _HANDLES:
                assert at is C.c_void_p, where
            else:
                assert ctype.strip() in _SCALARS, where
                assert not _is_pointer(at) and _scalar_kind(at) == _scalar_kind(_SCALARS[ctype.strip()]), where


def _struct_fields():
    """{struct name: [field names]} of every `typedef struct RmjX { ... } RmjX;` of the headers, in declaration order"""
    out = {}
    for name, body in re.findall(r"typedef\s+struct\s+(Rmj\w+)\s*\{(.*?)\}\s*\1\s*;", _headers(), flags=re.S):
        fields = []
        for decl in body.split(";"):
            if decl.strip():
                first, *more = decl.split(",")
                for d in [first.split()[-1]] + more:   # "uint8_t n_tiles, tiles[14]" / "const float *value, *log_prob"
                    fields.append(re.sub(r"\[.*", "", d).strip(" *\n"))
        out[name] = fields
    return out


def test_struct_layouts_match_the_headers(tmp_path):
    """Every struct of the two headers has a ctypes class in abi.py (abi.STRUCTS) and the other way round; sizeof and, by position,
    every field's offset and size agree with what the host C compiler makes of the header."""
    import subprocess

    structs = _struct_fields()
    assert set(structs) == set(abi.STRUCTS), f"header structs without a ctypes class / classes without a header struct: {set(structs) ^ set(abi.STRUCTS)}"
    lines = []
    for name, fields in structs.items():
        lines.append(f'printf("{name} %zu", sizeof({name}));')
        lines += [f'printf(" %zu %zu", offsetof({name}, {f}), sizeof((({name}*)0)->{f}));' for f in fields]
        lines.append('printf("\\n");')
    src = tmp_path / "layout.c"
    src.write_text('#include <stddef.h>\n#include <stdio.h>\n#include "riichi_mi355x_bench.h"\nint main(void) {\n' + "\n".join(lines) + "\nreturn 0;\n}\n")
    exe = tmp_path / "layout"
    subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)])
    for line in subprocess.check_output([str(exe)]).decode().splitlines():
        name, size, *rest = line.split()
        cls = abi.STRUCTS[name]
        want = list(zip(map(int, rest[0::2]), map(int, rest[1::2])))
        got = [(getattr(cls, f).offset, getattr(cls, f).size) for f, _ in cls._fields_]
        assert len(got) == len(want), f"{name}: {len(got)} ctypes fields for {len(want)} in the header"
        assert C.sizeof(cls) == int(size), f"{name}: sizeof {C.sizeof(cls)} against the header's {size}"
        for (f, _), g, w, hf in zip(cls._fields_, got, want, structs[name]):
            assert g == w, f"{name}.{f} (header: {hf}): (offset, size) {g} against the header's {w}"


def test_pack_unpack_roundtrip():
    a = abi.pack_action(abi.CHI, 57, [65, 62])
    assert abi.unpack_action(a) == (abi.CHI, 57, [62, 65])  # Action::new sorts (action.rs:97-98)
    assert abi.unpack_action(abi.pack_action(abi.RIICHI)) == (abi.RIICHI, None, [])


def test_no_cpu_fallback():
    """Without a HIP device the product path must fail loudly (never route through the oracle)."""
    import torch

    if torch.cuda.is_available():
        pytest.skip("GPU present")
    lib = vecenv.load_lib()
    assert lib.rmj_device_count() == 0
    with pytest.raises(vecenv.RmjError):
        vecenv.VecRiichiEnv(4)
    with pytest.raises(vecenv.RmjError):
        vecenv.eval_hands([abi.HandCase()])
    src = open(os.path.join(ROOT, "riichienv_amd", "vecenv.py")).read()
    assert "oracle" not in src.replace("oracle/oracle.py", "")


def _build_c_example(tmp_path):
    import subprocess

    exe = tmp_path / "rollout"
    lib_dir = os.path.join(ROOT, "riichienv_amd")
    cmd = ["gcc", "-O2", "-Wall", "-Werror", "-I" + os.path.join(ROOT, "include"), os.path.join(ROOT, "examples", "rollout.c"), "-o", str(exe),
           "-L" + lib_dir, "-l:libriichi_mi355x.so", "-Wl,-rpath," + lib_dir]
    subprocess.check_call(cmd)
    return str(exe)


def test_plain_c_program_links_against_the_boundary_and_fails_loudly_without_a_gpu(tmp_path):
    """examples/rollout.c sees nothing but include/riichi_mi355x.h (C, not C++): it must compile warning-free with gcc, link
    against the shared library, and - in this container, without a GPU - stop at rmj_create with the library's error text
    instead of computing anything on the CPU."""
    import subprocess

    import torch

    exe = _build_c_example(tmp_path)
    if torch.cuda.is_available():
        pytest.skip("a GPU is present: covered by the gpu test")
    p = subprocess.run([exe], capture_output=True, text=True)
    assert p.returncode == 1 and "no HIP device" in p.stderr and "0 device(s)" in p.stdout


@pytest.mark.gpu
def test_plain_c_program_runs_a_rollout(tmp_path):
    import subprocess

    p = subprocess.run([_build_c_example(tmp_path)], capture_output=True, text=True)
    assert p.returncode == 0, p.stderr
    assert "env.step calls advanced a game" in p.stdout and '"type"' in p.stdout
