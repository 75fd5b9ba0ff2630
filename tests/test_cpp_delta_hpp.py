"""Builds tests/cpp/delta_hpp_test.cpp (g++, against include/csic.hpp + libcsic_hip.so) and runs it: csic.hpp's wrappers of the temporal
layer and of .csic version 5 (deltaLayout, delta, undelta, writeContainerSeq, containerGop) and their refusals.  No GPU."""
import os
import subprocess

from conftest import ROOT

PKG = os.path.join(ROOT, "chroma-subsampling-image-compressor_amd")


def test_cpp_delta_wrappers(tmp_path):
    src = os.path.join(ROOT, "tests", "cpp", "delta_hpp_test.cpp")
    exe = str(tmp_path / "delta_hpp_test")
    assert os.path.exists(os.path.join(PKG, "libcsic_hip.so")), "build libcsic_hip.so first (python -c 'import __graft_entry__ as g; g.build()')"
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-I" + os.path.join(ROOT, "include"), src,
                           "-L" + PKG, "-lcsic_hip", "-Wl,-rpath," + PKG, "-Wl,-rpath,/opt/rocm/lib", "-o", exe])
    r = subprocess.run([exe, str(tmp_path)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and "all checks passed" in r.stdout, r.stdout + r.stderr
