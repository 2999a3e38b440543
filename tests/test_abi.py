"""The C-ABI shared library loads and exports every symbol the headers declare (no compute calls here: no GPU)."""
import ctypes as C
import os
import re

import pytest

import gi_raytracer_amd as gi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def declared(header):
    txt = open(os.path.join(ROOT, header)).read()
    txt = re.sub(r"/\*.*?\*/", "", txt, flags=re.S)
    return set(re.findall(r"\b(gih?_[a-z0-9_]+)\s*\(", txt))


HEADERS = ("include/gi_hip.h", "gi_raytracer_amd/csrc/gi_host.h")
SCALARS = {"int": C.c_int, "int32_t": C.c_int32, "uint32_t": C.c_uint32, "int64_t": C.c_int64, "uint64_t": C.c_uint64, "float": C.c_float, "double": C.c_double}


def declarations(header):
    """name -> (return type, [parameter, ...]) as the header writes them: comments removed, the parameter list split at top-level commas,
    `(void)` as no parameter."""
    txt = open(os.path.join(ROOT, header)).read()
    txt = re.sub(r"/\*.*?\*/", "", txt, flags=re.S)
    txt = re.sub(r"//[^\n]*", "", txt)
    out = {}
    for ret, name, params in re.findall(r"([A-Za-z_][A-Za-z0-9_ ]*?[\s*]+)\b(gih?_[a-z0-9_]+)\s*\(([^;{}]*)\)\s*;", txt):
        parts, depth, cur = [], 0, ""
        for ch in params:
            depth += ch in "([" and 1 or ch in ")]" and -1 or 0
            if ch == "," and depth == 0:
                parts.append(cur)
                cur = ""
            else:
                cur += ch
        parts = [" ".join(p.split()) for p in parts + [cur]]
        out[name] = (" ".join(ret.split()), [] if parts in ([""], ["void"]) else parts)
    return out


def is_pointer(t):
    return t in (C.c_void_p, C.c_char_p) or (isinstance(t, type) and issubclass(t, C._Pointer))


def check_type(c_text, ctype, what):
    """c_text is a return type, or a parameter with or without its name."""
    if "*" in c_text:
        assert is_pointer(ctype), f"{what}: `{c_text}` is a pointer, the table has {ctype}"
        return
    words = [w for w in c_text.split() if w not in ("const", "volatile")]
    if words[0] == "void":
        assert ctype is None, f"{what}: `{c_text}` returns nothing, the table has {ctype}"
        return
    assert words[0] in SCALARS and len(words) <= 2, f"{what}: `{c_text}` is no scalar this test knows"
    assert ctype is SCALARS[words[0]], f"{what}: `{c_text}` is {SCALARS[words[0]].__name__}, the table has {ctype}"


def test_signature_table_agrees_with_the_declarations():
    decl = {}
    for h in HEADERS:
        d = declarations(h)
        assert set(d) == declared(h), set(d) ^ declared(h)      # the parser missed no declaration
        decl.update(d)
    assert list(gi.ABI_SYMBOLS) == list(gi.SIGNATURES) and set(gi.SIGNATURES) == set(decl)
    for name, (ret, params) in decl.items():
        restype, argtypes = gi.SIGNATURES[name]
        assert len(argtypes) == len(params), f"{name}: the header has {len(params)} parameters, the table {len(argtypes)}"
        check_type(ret, restype, f"{name} returns")
        for k, (p, t) in enumerate(zip(params, argtypes)):
            check_type(p, t, f"{name} parameter {k}")


def test_the_loader_applies_the_table_and_nothing_else_sets_argtypes():
    L = gi.lib()
    for name, (restype, argtypes) in gi.SIGNATURES.items():
        f = getattr(L, name)
        assert f.restype is restype and list(f.argtypes) == list(argtypes), name
    pkg = os.path.join(ROOT, "gi_raytracer_amd")
    hits = [(f, n) for f in sorted(os.listdir(pkg)) if f.endswith(".py")
            for n, line in enumerate(open(os.path.join(pkg, f)), 1) if re.search(r"\.(argtypes|restype)\b", line)]
    assert [f for f, _ in hits] == ["_abi.py"], hits            # one line: the loop in lib()


def test_library_exports_every_declared_symbol():
    L = gi.lib()
    names = declared("include/gi_hip.h") | declared("gi_raytracer_amd/csrc/gi_host.h")
    assert names == set(gi.ABI_SYMBOLS)
    for n in names:
        assert hasattr(L, n), n


def test_abi_signatures_carry_no_framework_types():
    txt = open(os.path.join(ROOT, "include/gi_hip.h")).read()
    assert "torch" not in txt and "std::" not in txt and "hip/" not in txt   # plain pointers and sizes only


def test_struct_sizes_match_the_header_layout():
    assert C.sizeof(gi.RenderParams) == 9 * 8 + 2 * 8 + 5 * 4 + 2 * 4 + 4 + 8 + 8   # incl. 4 bytes of padding before noise_thresh
    assert C.sizeof(gi.SceneDesc) % 8 == 0 and C.sizeof(gi.PhotonMapDesc) % 8 == 0


def test_no_gpu_means_loud_failure_not_a_cpu_fallback():
    import torch
    if torch.cuda.is_available():
        pytest.skip("a GPU is present")
    with pytest.raises(gi.GiError):
        gi.RayTracer()


def test_product_never_touches_the_oracle():
    for dirpath, _, files in os.walk(os.path.join(ROOT, "gi_raytracer_amd")):
        for f in files:
            if f.endswith((".py", ".cpp", ".hip", ".h")):
                src = open(os.path.join(dirpath, f)).read()
                assert "gi_oracle" not in src and "oracle_lib" not in src and "libgi_emul" not in src, f
    for dirpath, _, files in os.walk(os.path.join(ROOT, "include")):
        for f in files:
            assert "oracle" not in open(os.path.join(dirpath, f)).read().lower(), f
