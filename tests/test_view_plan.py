"""plan_view / check_view (csrc/csic_select.cpp) and the `decompress --window --scale` arguments, without a GPU.  tests/cpp/view_plan.cpp
is built with csic_select.cpp and csic_host.cpp under ASan + UBSan as a stand-alone program -- nothing is loaded into python -- and
asserts, over scale x factor x alignment x widths 1 .. 9 x origins x knobs, that grid x block covers every output pixel exactly once,
that the fast kernel is chosen only under its conditions and that exactly the views outside the frame are refused.  The CLI half
writes a raw container on the host and checks every refusal and --help: none of them reaches a device."""
import os
import subprocess

import numpy as np

from conftest import ROOT

PKG = os.path.join(ROOT, "chroma-subsampling-image-compressor_amd")
SAN = ["-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-fno-omit-frame-pointer", "-g", "-O1"]


def test_plan_view_under_asan_ubsan(tmp_path):
    exe = str(tmp_path / "view_plan")
    subprocess.check_call(["g++", "-std=c++17", "-Wall", "-Wextra", *SAN, "-I" + os.path.join(ROOT, "include"), "-I" + os.path.join(PKG, "csrc"),
                           os.path.join(ROOT, "tests", "cpp", "view_plan.cpp"), os.path.join(PKG, "csrc", "csic_select.cpp"),
                           os.path.join(PKG, "csrc", "csic_host.cpp"), "-o", exe])
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=1", UBSAN_OPTIONS="print_stacktrace=1")
    r = subprocess.run([exe], capture_output=True, text=True, timeout=600, env=env)
    assert r.returncode == 0 and "view plan ok" in r.stdout, r.stdout[-2000:] + r.stderr[-4000:]


def test_view_of_a_window():
    import csic_amd as csic
    app = csic.ImageCompressionApp
    assert app.viewOf(512, 512) is None
    assert app.viewOf(512, 512, (100, 60, 256, 128), 4) == csic.View(100, 60, 64, 32, 4)
    assert app.viewOf(512, 300, None, 8) == csic.View(0, 0, 64, 37, 8)                   # 300 // 8: the remainder is dropped
    assert app.viewOf(512, 512, (1, 3, 103, 50), 8) == csic.View(1, 3, 12, 6, 8)
    assert app.viewOf(512, 512, (0, 0, 512, 512)) == csic.View(0, 0, 512, 512, 1)
    for window, scale in (((400, 0, 113, 64), 1), ((0, 449, 64, 64), 1), ((-1, 0, 8, 8), 1), ((0, 0, 0, 8), 1), ((0, 0, 7, 64), 8), ((0, 0, 64, 15), 16),
                          ((0, 0, 8, 8), 3), (None, 0)):
        try:
            app.viewOf(512, 512, window, scale)
        except csic.IllegalArgumentException as e:
            assert e.status == csic._native.EINVAL_SIZE
        else:
            raise AssertionError((window, scale))


def test_decompress_argument_refusals_and_help(tmp_path, capsys):
    import csic_amd as csic
    from csic_amd.app import main
    cp = csic.make_c_params(64, 48, 2, 0, 6, 5, 5, 2, (3, 1, 2), out_format=csic.PixelFormat.PLANAR_BITS)
    lay = csic._native.CsicPlanarBitsLayout()
    csic._native.check(csic._native.lib().csic_planar_bits_layout_of(cp, lay))
    packed, out = str(tmp_path / "x.csic"), str(tmp_path / "x.png")
    csic.write_container(packed, cp, np.zeros((1, lay.frame_bytes), dtype=np.uint8))
    base = ["decompress", "--input", packed, "--output", out]
    capsys.readouterr()
    for extra, status, word in ((["--scale", "3"], 2, "--scale must be 1, 2, 4, 8 or 16"), (["--scale", "x"], 2, "--scale must be"),
                                (["--window", "1,2,3"], 2, "--window must be x,y,w,h"), (["--window", "a,b,c,d"], 2, "--window must be x,y,w,h"),
                                (["--window", "60,0,5,8"], 1, "does not lie inside the 64x48 frame"), (["--window", "0,41,8,8"], 1, "does not lie inside"),
                                (["--window", "-1,0,8,8"], 1, "does not lie inside"), (["--window", "0,0,0,8"], 1, "does not lie inside"),
                                (["--window", "0,0,7,16", "--scale", "8"], 1, "smaller than one 8x8 box"), (["--scale", "16", "--window", "0,0,64,15"], 1, "smaller than one"),
                                (["--window", "0,0,8,8", "--frame", "1"], 1, "--frame must be in 0..0")):
        assert main(base + extra) == status, extra
        printed = capsys.readouterr().out
        assert printed.startswith("[ERROR]") and word in printed, (extra, printed)
        assert not os.path.exists(out)
    assert main(["decompress", "--input", packed, "--output-pattern", str(tmp_path / "f_%d.png"), "--window", "60,0,5,8"]) == 1
    assert "does not lie inside" in capsys.readouterr().out and not os.path.exists(tmp_path / "f_0.png")
    assert main(["decompress", "--help"]) == 0
    text = capsys.readouterr().out
    for word in ("--window x,y,w,h", "--scale s", "source pixels", "(w // s) x (h // s)", "remainder", "dropped", "--frame", "--output-pattern"):
        assert word in text, word
