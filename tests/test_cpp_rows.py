"""Builds tests/cpp/rows_fuzz.cpp together with the host codec of the row-prediction layer (csrc/csic_rows_host.cpp), the container
(csrc/csic_container.cpp) and the host codecs it reads through under ASan + UBSan and runs it: a stand-alone program, nothing is loaded
into python.  Random frames round-trip with every buffer in a heap block of exactly its size; about 4 000 mutated maps either decode to
frames that go through the layer again or are refused with CSIC_EFORMAT; about 3 000 mutated version-8 files are read or refused --
never an access out of range."""
import os
import subprocess

from conftest import ROOT

PKG = os.path.join(ROOT, "chroma-subsampling-image-compressor_amd")
SAN = ["-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-fno-omit-frame-pointer", "-g", "-O1"]
UNITS = ["csic_rows_host.cpp", "csic_container.cpp", "csic_pack_host.cpp", "csic_rice_host.cpp", "csic_rans_host.cpp", "csic_delta_host.cpp", "csic_mc_host.cpp",
         "csic_host.cpp"]


def test_host_codec_and_reader_fuzz_under_asan_ubsan(tmp_path):
    exe = str(tmp_path / "rows_fuzz")
    subprocess.check_call(["g++", "-std=c++17", "-Wall", *SAN, "-I" + os.path.join(ROOT, "include"), "-I" + os.path.join(PKG, "csrc"),
                           os.path.join(ROOT, "tests", "cpp", "rows_fuzz.cpp"), *[os.path.join(PKG, "csrc", u) for u in UNITS], "-lz", "-o", exe])
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=1", UBSAN_OPTIONS="print_stacktrace=1")
    r = subprocess.run([exe, str(tmp_path)], capture_output=True, text=True, timeout=600, env=env)
    assert r.returncode == 0 and "rows fuzz ok" in r.stdout, r.stdout[-2000:] + r.stderr[-4000:]
