"""The range-checking build (libcsic_hip_debug.so: `make -C chroma-subsampling-image-compressor_amd/csrc debug`, -DCSIC_DEBUG).
GPU AddressSanitizer is not available on the pool, so this is the device-side sanitizer stand-in: every global
access of the pixel kernels is checked against the frame extent and traps.  Two things are shown here, in CHILD processes
(CSIC_LIB selects the library at import time, and a trap ends its process):
  * the checks are live: one checked read outside the frame kills the child (and the same read inside the frame does not);
  * a broad parity sample through every kernel family runs clean under them;
  * so do the readers of the planar formats -- reconstruct (whose output stores are checked too), decode, code statistics -- at the
    smallest shapes at which they take each of their paths.
The whole `-m gpu` suite under the debug library is run by tools/run_debug_suite.sh (log: profiles/r04_gpu_tests_debug.log)."""
import os
import subprocess
import sys

import pytest

from conftest import ROOT

pytestmark = pytest.mark.gpu

PKG = os.path.join(ROOT, "chroma-subsampling-image-compressor_amd")
DEBUG_LIB = os.path.join(PKG, "libcsic_hip_debug.so")


def _child(code, timeout=300):
    env = dict(os.environ, CSIC_LIB=DEBUG_LIB, PYTHONPATH=ROOT + os.pathsep + os.environ.get("PYTHONPATH", ""))
    return subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, timeout=timeout, env=env, cwd=ROOT)


@pytest.fixture(scope="module", autouse=True)
def _built():
    if not os.path.exists(DEBUG_LIB):
        subprocess.check_call(["make", "-C", os.path.join(PKG, "csrc"), "-s", "debug"])


PROBE = """
import ctypes as C, sys, torch, csic_amd as csic
N = csic._native; lib = N.lib()
assert lib.csic_debug_build() == 1, "not the debug build"
buf = torch.arange(64 * 8, dtype=torch.int32, device="cuda:0")
sink = torch.zeros(1, dtype=torch.int32, device="cuda:0")
off = int(sys.argv[1]) if len(sys.argv) > 1 else %d
N.check(lib.csic_debug_probe_device(C.c_void_p(buf.data_ptr()), 64, 4, off, C.c_void_p(sink.data_ptr()), None))
torch.cuda.synchronize()
print("read", int(sink.item()))
"""


def test_the_product_library_is_not_the_debug_build():
    import csic_amd
    assert csic_amd._native.lib().csic_debug_build() == 0


def test_a_checked_read_inside_the_frame_passes_and_one_outside_traps():
    ok = _child(PROBE % (64 * 4 - 1))                       # the frame's last pixel: extent = (H - 1) * pitch + W = 256
    assert ok.returncode == 0 and "read 255" in ok.stdout, ok.stdout + ok.stderr
    bad = _child(PROBE % (64 * 4))                          # one past it -- still inside the ALLOCATION (512 words): only the check can object
    assert bad.returncode != 0 and "read" not in bad.stdout, bad.stdout + bad.stderr
    neg = _child(PROBE % -1)
    assert neg.returncode != 0 and "read" not in neg.stdout, neg.stdout + neg.stderr


SAMPLE = """
import itertools, numpy as np, torch, csic_amd as csic
from oracle import oracle as orc
N = csic._native
assert N.lib().csic_debug_build() == 1
rng = np.random.default_rng(404)
modes = [(4, 4), (2, 2), (2, 0), (1, 1), (4, 0), (1, 0)]
orders = list(itertools.permutations((1, 2, 3)))
kernels = set()
for it in range(260):
    W, H = int(rng.integers(1, 120)), int(rng.integers(1, 50))
    if rng.random() < 0.4: W = (W + 7) // 8 * 8
    a, b = modes[int(rng.integers(0, 6))]
    f = int(rng.choice([1, 2, 4, 8]))
    op = orders[int(rng.integers(0, 6))]
    avg = rng.random() < 0.25
    if avg: op = (3, 1, 2)
    planar = rng.random() < 0.3
    argb = rng.integers(0, 1 << 32, W * H, dtype=np.uint32)
    p = orc.OracleParams(width=W, height=H, chroma_a=a, chroma_b=b, y_bits=7, cb_bits=6, cr_bits=5, factor=f, op=op)
    cp = csic.make_c_params(W, H, a, b, 7, 6, 5, f, op, out_format=2 if planar else 0, sampling=csic.Sampling.AVG if avg else csic.Sampling.HOLD_DECIMATE)
    with csic.Plan(cp, 0) as pl:
        for variant in (0, 5, 7, 9, 10, 11) if not avg else (0, 8):
            pl.tune(N.TUNE_VARIANT, variant)
            kernels.add(pl.kernel_name.split("<")[0])
            want = orc.process(p, argb, form="avg" if avg else "stream")
            if planar:
                d = torch.from_numpy(argb.view(np.int32)).cuda()
                got = pl.reconstruct_device(pl.process_device(d)).cpu().numpy().view(np.uint32)
            else:
                got = pl.process_host(argb)
            assert np.array_equal(got, want), (pl.kernel_name, W, H, a, b, f, op, avg, planar, variant)
torch.cuda.synchronize()
print("clean", len(kernels), sorted(kernels))
"""


def test_every_kernel_family_runs_clean_under_the_range_checks():
    r = _child(SAMPLE, timeout=900)
    assert r.returncode == 0 and "clean" in r.stdout, r.stdout[-2000:] + r.stderr[-2000:]
    for fam in ("k_avg", "k_dec", "k_decflat", "k_f1flat", "k_f1x4", "k_flatgen", "k_generic", "k_planar_flat", "k_planar_strided", "k_planar_avg_f1", "k_planar_avg_gen"):
        assert f"'{fam}'" in r.stdout, (fam, r.stdout)


# The plane readers -- the reconstruct kernels (whose output stores are range-checked against the frame's n pixels), the decode
# kernels and the code statistics -- on VALID inputs only, at the smallest shapes at which they take each of their paths:
#   reconstruct  64 x 40 at factors 1 and 2 (factor 1: 2560 positions = two whole blocks of 64 threads x 4 groups x 4 positions on the
#                straight-line body, the rest on the checked one; module width % 4 == 0: the fast path), 37 x 21 (module width % 4 != 0:
#                every group position by position, a ragged tail of 1), 200 x 26 x 3 frames (the per-frame extent on frames 1 and 2);
#                each with the default kernels, CSIC_TUNE_VARIANT 9 and non-temporal accesses off;
#   decode       64 x 40 and 36 x 22 at factors 1, 2, 4, 8 (the fast kernel, from planes at factor 1 the reconstruct kernels; 22 is ragged
#                against 4 and 8), 37 x 21 at factor 2 (the general kernel);
#   code stats   13 x 9, the smallest shape of test_gpu_code_stats.py, all three kernels.
# Every operation order, 4:4:4 / 4:2:2 / 4:2:0 / 4:1:1, bits (8, 8, 8) and (7, 6, 5); every result is held against the oracle.
PLANE_READERS = """
import itertools, numpy as np, torch, csic_amd as csic
from oracle import oracle as orc
N = csic._native
assert N.lib().csic_debug_build() == 1
ARGB, YCC, PLANAR, BITS = N.FMT_ARGB8888, N.FMT_YCBCR888X, N.FMT_PLANAR, N.FMT_PLANAR_BITS
rng = np.random.default_rng(505)
stems, checked = set(), 0

def plan(W, H, a, b, bits, f, op, fmt):
    return csic.Plan(csic.make_c_params(W, H, a, b, *bits, f, op, out_format=fmt), 0)
def oparams(W, H, a, b, bits, f, op, fmt=ARGB):
    return orc.OracleParams(width=W, height=H, chroma_a=a, chroma_b=b, y_bits=bits[0], cb_bits=bits[1], cr_bits=bits[2], factor=f, op=op, out_format=fmt)
def dev(x):
    return torch.from_numpy(np.ascontiguousarray(x).reshape(-1).view(np.int32)).cuda()
def host(t):
    return t.cpu().numpy().view(np.uint32)
def hists(planes, bits):
    out = np.zeros((2, 3, 256), dtype=np.uint64)
    for p, (v, q) in enumerate(zip(planes, bits)):
        c = np.asarray(v, dtype=np.uint8).reshape(-1).astype(np.int64) >> (8 - q)
        out[0, p] = np.bincount(c, minlength=256)
        out[1, p] = np.bincount(np.concatenate([c[:1], np.diff(c) % (1 << q)]), minlength=256)
    return out

TUNES = ((N.TUNE_VARIANT, 0), (N.TUNE_VARIANT, 9), (N.TUNE_NONTEMPORAL, 0))
for op, (a, b), bits in itertools.product(itertools.permutations((1, 2, 3)), ((4, 4), (2, 2), (2, 0), (1, 1)), ((8, 8, 8), (7, 6, 5))):
    for W, H, f, nf in ((64, 40, 1, 1), (64, 40, 2, 1), (37, 21, 1, 1), (200, 26, 1, 3)):
        frames = rng.integers(0, 1 << 32, (nf, W * H), dtype=np.uint32)
        want = {o: np.stack([orc.process(oparams(W, H, a, b, bits, f, op, o), fr).reshape(-1) for fr in frames]) for o in (ARGB, YCC)}
        for fmt in (PLANAR, BITS):
            with plan(W, H, a, b, bits, f, op, fmt) as pl:
                buf = pl.process_device(dev(frames), nframes=nf)
                recon = pl.reconstruct_device if fmt == PLANAR else pl.reconstruct_bits_device
                for knob, value in TUNES:
                    pl.tune(N.TUNE_VARIANT, 0); pl.tune(N.TUNE_NONTEMPORAL, 1); pl.tune(knob, value)
                    for o in (ARGB, YCC):
                        got = host(recon(buf, nframes=nf, out_format=o)).reshape(nf, -1)
                        assert np.array_equal(got, want[o]), ("reconstruct", W, H, f, nf, op, a, b, bits, fmt, knob, value, o)
                        checked += 1
    for W, H, f in [(W, H, f) for W, H in ((64, 40), (36, 22)) for f in (1, 2, 4, 8)] + [(37, 21, 2)]:
        frame = rng.integers(0, 1 << 32, W * H, dtype=np.uint32)
        srcs = {}
        for s in (YCC, PLANAR, BITS):
            with plan(W, H, a, b, bits, f, op, s) as ps:
                srcs[s] = ps.process_device(dev(frame))
        with plan(W, H, a, b, bits, f, op, ARGB) as pl:
            for o in (ARGB, YCC):
                small = orc.process(oparams(W, H, a, b, bits, f, op, o), frame).reshape(-(-H // f), -(-W // f))
                want = small[np.arange(H)[:, None] // f, np.arange(W)[None, :] // f]
                for s, src in srcs.items():
                    name = pl.decode_kernel_name(s, o)
                    stems.add(name.split("<")[0])
                    assert np.array_equal(host(pl.decode_device(src, s, out_format=o)), want), (name, W, H, f, op, a, b, bits)
                    checked += 1
    W, H = 13, 9
    frame = rng.integers(0, 1 << 32, W * H, dtype=np.uint32)
    want = hists(orc.planar(oparams(W, H, a, b, bits, 1, op), frame)[1:], bits)
    for fmt in (PLANAR, BITS):
        with plan(W, H, a, b, bits, 1, op, fmt) as pl:
            buf = pl.process_device(dev(frame))
            for force in (0, 1):
                pl.tune(N.TUNE_FORCE_GENERIC, force)
                name = pl.code_stats_kernel_name()
                stems.add(name.split("<")[0])
                got = pl.code_stats_device(buf).cpu().numpy().view(np.uint64)[0]
                assert np.array_equal(got, want), (name, op, a, b, bits)
                checked += 1
torch.cuda.synchronize()
print("clean", checked, sorted(stems))
"""


def test_the_plane_readers_run_clean_under_the_range_checks():
    r = _child(PLANE_READERS, timeout=300)
    # 6 orders x 4 modes x 2 bit triples, each: 4 shapes x 2 formats x 3 tunings x 2 outputs reconstructed, 9 shapes x 3 sources x 2
    # outputs decoded, 2 formats x 2 kernels counted
    assert r.returncode == 0 and f"clean {48 * (48 + 54 + 4)} " in r.stdout, r.stdout[-2000:] + r.stderr[-2000:]
    for stem in ("k_recon", "k_rbits", "k_decode", "k_decode_gen", "k_cstat_bytes", "k_cstat_bits", "k_cstat_gen"):
        assert f"'{stem}'" in r.stdout, (stem, r.stdout)
