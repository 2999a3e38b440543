"""How the tests compile C++ of their own.  Test infrastructure, a plain module like emul_lib: the CPU build's compile flags, kept once in
tests/host_emul/Makefile, and the one line that links a C++ program against the product library."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def flags():
    """The flags of the CPU build of the device functions (FLAGS of tests/host_emul/Makefile), for a test that compiles a file of its own against
    gi_device.h."""
    return subprocess.run(["make", "-s", "-C", os.path.join(ROOT, "tests", "host_emul"), "flags"], check=True, capture_output=True, text=True).stdout.split()


def client(source, exe, *extra):
    """Compile the C++ program `source` (a path under the repository root) and link it against gi_raytracer_amd/libgi_raytracer_hip.so; extra: the
    caller's own flags (-O1, -Wall)."""
    lib = os.path.join(ROOT, "gi_raytracer_amd")
    subprocess.run(["g++", "-std=c++17", *extra, os.path.join(ROOT, source), "-L" + lib, "-lgi_raytracer_hip",
                    "-Wl,-rpath," + lib, "-Wl,-rpath,/opt/rocm/lib", "-L/opt/rocm/lib", "-o", str(exe)], check=True)
