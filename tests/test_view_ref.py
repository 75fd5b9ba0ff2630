"""tests/view_ref.py against itself: scale 1 is a crop, the worked vector of include/csic.h, and -- on the exact inputs the GPU
tests use -- each of six wrong rules gives a different frame for at least one case of every scale >= 2, so a kernel that followed one
of them would fail tests/test_gpu_view.py.  The Python layer's View and the library's refusals that need no device are here too."""
import ctypes as C

import numpy as np
import pytest

import view_ref as R


def test_scale_one_is_the_crop(oracle):
    for c in R.DISCRIMINATING[:2]:
        d = R.decoded(oracle, c, R.ARGB)
        for v in R.views_of(c.W, c.H, 1):
            assert np.array_equal(R.view(oracle, c, v), d[v.y0:v.y0 + v.height, v.x0:v.x0 + v.width]), (c, v)


def test_the_worked_vector_of_the_header():
    boxes = np.array([[0xFF102030, 0xFF112131, 0xFF000000, 0xFF000001], [0xFF122232, 0xFF142434, 0xFF0000FF, 0xFF000100]], dtype=np.uint32)
    assert R.box(boxes, R.View(0, 0, 2, 1, 2)).tolist() == [[0xFF122232, 0xFF000040]]
    # the largest sum: 256 bytes of 255, + 128 = 65 408, fits 16 bits
    assert R.box(np.full((16, 16), 0xFFFFFFFF, dtype=np.uint32), R.View(0, 0, 1, 1, 16)).tolist() == [[0xFFFFFFFF]]


@pytest.mark.parametrize("rule", R.WRONG_RULES, ids=[f.__name__ for f in R.WRONG_RULES])
def test_the_inputs_tell_each_wrong_rule_from_the_right_one(oracle, rule):
    pairs = list(R.cases_and_views())
    for s in R.SCALES[1:]:
        assert any(not np.array_equal(rule(oracle, c, v), R.view(oracle, c, v)) for c, v in pairs if v.scale == s and c in R.DISCRIMINATING), \
            (rule.__name__, s)


def test_the_sweep_covers_what_it_claims():
    pairs = list(R.cases_and_views())
    cases = {c for c, _ in pairs}
    assert {(c.W, c.H) for c in cases} == set(R.SHAPES)
    assert {(c.a, c.b) for c in cases} == set(R.MODES) and {c.f for c in cases} == set(R.FACTORS)
    assert {c.bits for c in cases} == {(8, 8, 8), (6, 5, 5), (3, 3, 2), (1, 1, 1)} and {c.avg for c in cases} == {False, True}
    for s in R.SCALES:
        for f in R.FACTORS:
            vs = [v for c, v in pairs if v.scale == s and c.f == f]
            assert {v.width % 4 == 0 for v in vs} == {True, False}, (s, f)          # both kernels
            assert any(v.x0 % 2 == 1 and v.y0 % 2 == 1 for v in vs), (s, f)
    # 130 x 70 at scale 16: more than one box per row, and a width that is no multiple of 4
    assert R.View(0, 0, 8, 4, 16) in R.views_of(130, 70, 16)
    for c, v in pairs:
        assert v.x0 + v.width * v.scale <= c.W and v.y0 + v.height * v.scale <= c.H


def test_python_view_and_refusals_without_a_device():
    import csic_amd as csic
    N = csic._native
    assert csic.View(1, 2, 3, 4) == (1, 2, 3, 4, 1) and csic.View(0, 0, 8, 8, 4).scale == 4
    v = N.CsicView(1, 2, 3, 4, 8)
    assert C.sizeof(N.CsicView) == 20 and (v.x0, v.y0, v.width, v.height, v.scale) == (1, 2, 3, 4, 8)
    px = (C.c_uint32 * 8)()
    lib = N.lib()
    assert lib.csic_decode_view_device(None, px, 1, C.byref(v), px, 0, 1, None) == N.EINVAL_NULL
    assert lib.csic_decode_view_host(None, px, 32, 1, C.byref(v), px, 8, 0, 1) == N.EINVAL_NULL
    assert lib.csic_decode_view_kernel_name(None, 3, 0, C.byref(v)) == b""
