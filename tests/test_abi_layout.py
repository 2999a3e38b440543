"""The ctypes mirrors of the header structs have the headers' layout: a C++ program generated from the classes prints sizeof of each struct and
offsetof and sizeof of every field as g++ sees them in include/gi_hip.h and csrc/gi_host.h.  A field the header lacks, or one the mirror lacks, fails the compile."""
import ctypes as C
import os
import subprocess

import gi_raytracer_amd as gi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MODULES = [f[:-3] for f in sorted(os.listdir(os.path.dirname(gi.__file__))) if f.endswith(".py") and not f.startswith("__")]


def test_every_struct_in_the_package_is_listed():
    mirrors = {v for m in MODULES for v in vars(__import__("gi_raytracer_amd." + m, fromlist=["x"])).values()
               if isinstance(v, type) and issubclass(v, C.Structure) and v is not C.Structure}
    assert mirrors == set(gi.STRUCTS.values()) and len(mirrors) == len(gi.STRUCTS)


def test_struct_mirrors_have_the_headers_layout(tmp_path):
    lines = ["#include <cstddef>", "#include <cstdio>", f'#include "{ROOT}/include/gi_hip.h"', f'#include "{ROOT}/gi_raytracer_amd/csrc/gi_host.h"',
             "int main() {"]
    want = []
    for c_type, s in gi.STRUCTS.items():
        lines.append(f'    std::printf("{c_type} %zu\\n", sizeof({c_type}));')
        want.append(f"{c_type} {C.sizeof(s)}")
        # a structured binding takes exactly as many names as the struct has fields: a header field the mirror lacks fails the compile too
        lines.append(f"    {{ {c_type} v{{}}; auto& [{', '.join(f'f{k}' for k in range(len(s._fields_)))}] = v; (void)f0; }}")
        for name, _ in s._fields_:        # the width too: offsets alone would not see a last field of the wrong width inside the tail padding
            lines.append(f'    std::printf("{c_type}.{name} %zu %zu\\n", offsetof({c_type}, {name}), sizeof((({c_type}*)0)->{name}));')
            want.append(f"{c_type}.{name} {getattr(s, name).offset} {getattr(s, name).size}")
    src, exe = tmp_path / "layout.cpp", tmp_path / "layout"
    src.write_text("\n".join(lines + ["    return 0;", "}"]) + "\n")
    subprocess.run(["g++", "-std=c++17", "-Wall", str(src), "-o", str(exe)], check=True)
    got = subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.splitlines()
    assert got == want, [(g, w) for g, w in zip(got, want) if g != w]
