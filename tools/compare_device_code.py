#!/usr/bin/env python3
"""Is the device code of gi_kernels.hip the same in two source trees?  For a change that is meant to move host code only, or kernels between the files it includes.

usage: tools/compare_device_code.py CSRC_A CSRC_B      (two gi_raytracer_amd/csrc directories; A == B checks the comparison itself)

Each side is compiled with its own Makefile's HIPFLAGS plus --offload-device-only, the gfx950 code object is unbundled where hipcc bundled it,
and the two are compared kernel by kernel: the disassembled text (instruction addresses and encodings dropped) and the kernel's metadata record
(arguments, VGPR / SGPR / AGPR counts, LDS, scratch, spills -- what tools/kernel_resources.py reports, and the rest of the record).  The objects
themselves are not compared: two builds of one source differ in bytes that are no code.  Exit status 0 = every kernel the same."""
import os, re, subprocess, sys, tempfile
from concurrent.futures import ThreadPoolExecutor

LLVM = "/opt/rocm/lib/llvm/bin"
HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")


def hipflags(csrc):
    mk = open(os.path.join(csrc, "Makefile")).read()
    arch = re.search(r"^ARCH \?= (\S+)", mk, re.M).group(1)
    return re.search(r"^HIPFLAGS := (.*)$", mk, re.M).group(1).replace("$(ARCH)", arch).split(), arch


def code_object(csrc, out):
    flags, arch = hipflags(csrc)
    subprocess.run([HIPCC] + flags + ["--offload-device-only", "-c", "gi_kernels.hip", "-o", out], cwd=csrc, check=True, stderr=subprocess.DEVNULL)
    if open(out, "rb").read(24) == b"__CLANG_OFFLOAD_BUNDLE__":
        subprocess.run([f"{LLVM}/clang-offload-bundler", "--unbundle", "--type=o", f"--input={out}", f"--output={out}.elf", f"--targets=hipv4-amdgcn-amd-amdhsa--{arch}"], check=True)
        out += ".elf"
    return out


def kernels(co):
    """{kernel symbol: (disassembly without addresses, metadata record)}"""
    notes = subprocess.run([f"{LLVM}/llvm-readelf", "--notes", co], capture_output=True, text=True, check=True).stdout
    meta = {}
    for b in re.split(r"\n(?=\s+- \.agpr_count:)", notes)[1:]:
        b = re.split(r"\n\S", b)[0]                                  # up to the end of the kernel list
        meta[re.search(r"\.symbol:\s+'?([^'\s]+?)(?:\.kd)?'?\s", b).group(1)] = b
    dis = subprocess.run([f"{LLVM}/llvm-objdump", "-d", "--no-show-raw-insn", co], capture_output=True, text=True, check=True).stdout
    text = {}
    for part in re.split(r"\n(?=[0-9a-f]+ <[^>]+>:)", dis)[1:]:
        name = re.match(r"[0-9a-f]+ <([^>]+)>:", part).group(1)
        text[name] = "\n".join(re.sub(r"\s*//.*$", "", line) for line in part.splitlines()[1:])
    return {k: (text.get(k), meta[k]) for k in meta}


def main():
    a, b = (os.path.abspath(p) for p in sys.argv[1:3])
    with tempfile.TemporaryDirectory() as td:
        with ThreadPoolExecutor(2) as ex:
            ka, kb = ex.map(lambda x: kernels(code_object(x[0], os.path.join(td, x[1]))), ((a, "a.co"), (b, "b.co")))
    diff = sorted(set(ka) ^ set(kb))
    for k in diff:
        print("only in", "A" if k in ka else "B", k)
    n_text = n_meta = 0
    for k in sorted(set(ka) & set(kb)):
        if ka[k][0] is None or ka[k][0] != kb[k][0]:
            n_text += 1
            print("text differs:", k)
        if ka[k][1] != kb[k][1]:
            n_meta += 1
            print("metadata differs:", k)
    n_ins = sum(len(t.splitlines()) for t, _ in ka.values() if t)
    print(f"{len(ka)} kernels in A ({n_ins} lines of disassembly), {len(kb)} in B: {len(diff)} not in both, {n_text} differ in text, {n_meta} in metadata"
          + (" -- same device code" if not (diff or n_text or n_meta) else ""))
    return 1 if diff or n_text or n_meta else 0


if __name__ == "__main__":
    sys.exit(main())
