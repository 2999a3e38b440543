"""The failure paths of the host ABI's helpers (gi_scratch.h: DevBuf, EventTimer, finish_to_host) under the address and undefined-behaviour
sanitizers: tests/host_abi/host_abi.cpp over a malloc-backed stub of HIP, built here as a program of its own and run directly.  It fails every
HIP call of a wrapper-shaped sequence once; a leak, a double free or a wrong error code on any of those paths fails the program."""
import os
import subprocess

DIR = os.path.join(os.path.dirname(os.path.abspath(__file__)), "host_abi")


def test_host_helpers_failure_paths_under_sanitizers(tmp_path):
    exe = str(tmp_path / "host_abi")
    subprocess.run([os.environ.get("CXX", "g++"), "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-static-libasan", "-static-libubsan",
                    "-fno-omit-frame-pointer", os.path.join(DIR, "host_abi.cpp"), "-o", exe], check=True)
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 0 and "host_abi ok" in r.stdout, r.stdout + r.stderr
    assert "Sanitizer" not in r.stderr and "runtime error" not in r.stderr, r.stderr
