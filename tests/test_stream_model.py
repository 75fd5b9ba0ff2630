"""The cycle-level stream model (csic_stream_*) against the reference's handshake tests and the oracle.

 * SpatialDownsamplerSpec.scala:20-46 (decimation KAT, driven exactly as the spec drives the RTL), :48-58 (back-pressure),
   :60-118 (factors 4 and 8), :120-145 (5x3), :147-151 (factor 3 rejected);
 * RGB2YCbCrTester.scala:12-30 and ColorQuantizerSpec.scala:72-100 through their register slices;
 * the pixel stream that comes out of ImageCompressorTop / ImageProcessor, under random producer gaps and random
   back-pressure, equals oracle/csic_oracle.c:orc_process_stream for all six op orders (handshakes must never change data);
 * structural timing: three non-pipe Queue(1)s cap ImageCompressorTop at 0.5 pixel / clock (ImageCompressorTop.scala:63-65),
   ImageProcessor (no queues) runs at 1 pixel / clock, and the app collector's budget of Wo*Ho*40 + 10000 cycles
   (ImageCompressorTopApp.scala:110).
CPU only: the model is host code."""
import itertools

import numpy as np
import pytest


@pytest.fixture(scope="module")
def csic():
    import csic_amd
    return csic_amd


@pytest.fixture(scope="module")
def S(csic):
    from csic_amd import stream
    return stream


def ycc(y, cb, cr):
    return y | (cb << 8) | (cr << 16)


# ---- SpatialDownsamplerSpec.scala ---------------------------------------------------------------------------------------
def _spec_decimation(S, w, h, f, expected):
    """The loop of SpatialDownsamplerSpec.scala:21-45, statement for statement."""
    dut = S.SpatialDownsampler(w, h, f)
    dut.poke(out_ready=True)                                          # :22
    in_idx, out_count, total_in = 0, 0, w * h
    guard = 0
    while out_count < len(expected):                                  # :28
        dut.poke(in_valid=False)
        dut.poke(in_valid=(in_idx < total_in and dut.peek().in_ready))    # :29
        if dut._in.in_valid:                                          # :30
            dut.poke(in_bits=ycc(in_idx & 255, (100 + in_idx) & 255, (200 + in_idx) & 255))   # :31-33
            in_idx += 1                                               # :34
        sig = dut.peek()
        if sig.out_valid:                                             # :36
            exp = expected[out_count]
            assert sig.out_bits == ycc(exp & 255, (100 + exp) & 255, (200 + exp) & 255)      # :37-40
            out_count += 1
        dut.step()                                                    # :43
        guard += 1
        assert guard < 10 * total_in + 100
    return dut.cycles


def test_spatial_downsampler_4x4_factor_2(S):
    _spec_decimation(S, 4, 4, 2, [0, 2, 8, 10])                       # SpatialDownsamplerSpec.scala:26


def test_spatial_downsampler_factor_4_and_8(S):
    _spec_decimation(S, 8, 8, 4, [r * 8 + c for r in range(0, 8, 4) for c in range(0, 8, 4)])        # :62-65
    _spec_decimation(S, 16, 16, 8, [r * 16 + c for r in range(0, 16, 8) for c in range(0, 16, 8)])   # :92-95


def test_spatial_downsampler_5x3_non_divisible(S):
    _spec_decimation(S, 5, 3, 2, [0, 2, 4, 10, 12, 14])               # :122


def test_spatial_downsampler_back_pressure(S):
    """SpatialDownsamplerSpec.scala:48-58, verbatim: at a sample point in.ready follows out.ready."""
    dut = S.SpatialDownsampler(4, 4, 2)
    dut.poke(out_ready=False)
    dut.step()
    assert dut.peek().in_ready is False
    dut.poke(out_ready=True)
    dut.step()
    assert dut.peek().in_ready is True
    # and off a sample point the pixel is swallowed whatever out.ready says (SpatialDownsampler.scala:49-53)
    dut.poke(in_valid=True, in_bits=ycc(1, 2, 3), out_ready=True)
    dut.step()                                                        # pixel 0 accepted: col = 1, not a sample column
    dut.poke(out_ready=False)
    sig = dut.peek()
    assert sig.in_ready is True and sig.out_valid is False


def test_factor_3_is_rejected(S, csic):
    with pytest.raises(csic.IllegalArgumentException):                # SpatialDownsamplerSpec.scala:147-151
        S.SpatialDownsampler(4, 4, 3)
    with pytest.raises(csic.IllegalArgumentException):                # ChromaSubsampler.scala:17
        S.ChromaSubsampler(4, 4, 8, 3, 3)
    with pytest.raises(csic.IllegalArgumentException):                # ColorQuantizer.scala:13
        S.ColorQuantizer(0, 8, 8)
    with pytest.raises(csic.IllegalArgumentException):                # ImageCompressorTop.scala:31
        S.ImageCompressorTop(8, 8, 4, 4, 8, 8, 8, 1, 1, 1, 2)


# ---- register slices: RGB2YCbCrTester.scala:12-30, ColorQuantizerSpec.scala:72-100 ----------------------------------------
def test_rgb2ycbcr_slice_matches_reference_model(S, csic):
    dut = S.RGB2YCbCr()
    dut.poke(out_ready=True)
    for (r, g, b) in [(0, 0, 0), (255, 255, 255), (255, 0, 0), (0, 255, 0), (0, 0, 255)]:    # RGB2YCbCrTester.scala:12-18
        assert dut.peek().in_ready is True
        dut.poke(in_valid=True, in_bits=(r << 16) | (g << 8) | b)
        dut.step()                                                    # :24
        dut.poke(in_valid=False)
        sig = dut.peek()
        assert sig.out_valid is True
        y, cb, cr = sig.out_bits & 255, (sig.out_bits >> 8) & 255, (sig.out_bits >> 16) & 255
        exp = {(0, 0, 0): (0, 128, 128), (255, 255, 255): (255, 128, 128), (255, 0, 0): (77, 85, 255),
               (0, 255, 0): (149, 43, 21), (0, 0, 255): (29, 255, 107)}[(r, g, b)]
        assert (y, cb, cr) == exp, (r, g, b)
        dut.step()                                                    # out fires, the slice empties
        assert dut.peek().out_valid is False


def test_register_slice_holds_its_pixel_under_back_pressure(S):
    """in.ready = !valid || out.ready (RGB2YCbCr.scala:73, ColorQuantizer.scala:33, ChromaSubsampler.scala:40)."""
    dut = S.ColorQuantizer(3, 3, 2)
    dut.poke(in_valid=True, in_bits=ycc(200, 50, 220), out_ready=False)
    assert dut.peek() == (True, False, 0)
    dut.step()
    dut.poke(in_bits=ycc(16, 16, 16))
    for _ in range(5):                                                # full and blocked: not ready, output stable
        sig = dut.peek()
        assert sig.in_ready is False and sig.out_valid is True and sig.out_bits == ycc(192, 32, 192)   # ColorQuantizerSpec Y3Cb3Cr2
        dut.step()
    dut.poke(out_ready=True)
    assert dut.peek().in_ready is True                                # full, but draining this cycle: accepts the next pixel
    dut.step()
    assert dut.peek().out_bits == ycc(0, 0, 0)                        # (16,16,16) -> (0,0,0) at 3/3/2 bits


# ---- the stream equals the oracle's, whatever the handshakes do ----------------------------------------------------------
ORDERS = list(itertools.permutations((1, 2, 3)))


def _oracle_stream(oracle, W, H, a, b, bits, f, op, out_format):
    p = oracle.OracleParams(width=W, height=H, chroma_a=a, chroma_b=b, y_bits=bits[0], cb_bits=bits[1], cr_bits=bits[2],
                            factor=f, op=op, out_format=out_format)
    return p


@pytest.mark.parametrize("op", ORDERS)
def test_top_stream_equals_oracle_under_random_handshakes(S, csic, oracle, op):
    rng = np.random.default_rng(sum(op) * 7 + op[0])
    for _ in range(12):
        f = int(rng.choice([1, 2, 4, 8]))
        a, b = [(4, 4), (2, 2), (2, 0), (1, 1), (1, 0)][int(rng.integers(0, 5))]
        W, H = int(rng.integers(1, 40)), int(rng.integers(1, 24))
        bits = tuple(int(x) for x in rng.integers(1, 9, 3))
        frame = oracle.synth_frame(W * H, int(rng.integers(0, 1 << 30)))
        for inverse in (False, True):
            want = oracle.process(_oracle_stream(oracle, W, H, a, b, bits, f, op, 0 if inverse else 1), frame, form="stream").reshape(-1)
            with S.ImageCompressorTop(W, H, a, b, *bits, f, *op, inverse=inverse) as dut:
                assert dut.depth == 7
                got, cyc = dut.run(frame)                              # the harness's own handshakes: valid and ready held high
                assert np.array_equal(got, want if inverse else want & 0xFFFFFF), (W, H, a, b, bits, f, op)
                dut.reset()
                pv = rng.integers(0, 2, int(rng.integers(1, 9))).astype(np.uint8)
                pr = rng.integers(0, 2, int(rng.integers(1, 9))).astype(np.uint8)
                pv[0] = pr[-1] = 1
                got2, cyc2 = dut.run(frame, in_valid_pattern=pv, out_ready_pattern=pr)
                assert np.array_equal(got2, got) and cyc2 >= cyc


def test_image_processor_stream_equals_oracle(S, csic, oracle):
    rng = np.random.default_rng(5)
    for _ in range(20):
        f = int(rng.choice([1, 2, 4, 8]))
        a, b = [(4, 4), (2, 2), (2, 0), (1, 1), (1, 0)][int(rng.integers(0, 5))]
        W, H = f * int(rng.integers(1, 12)), f * int(rng.integers(1, 10))
        frame = oracle.synth_frame(W * H, int(rng.integers(0, 1 << 30)))
        want = oracle.process(_oracle_stream(oracle, W, H, a, b, (8, 8, 8), f, (3, 1, 2), 1), frame, form="stream").reshape(-1)
        with S.ImageProcessor(csic.ImageProcessorParams(W, H, f, a, b)) as dut:
            assert dut.depth == 3
            got, cyc = dut.run(frame)
            assert np.array_equal(got, want & 0xFFFFFF)
            # no queues: one pixel per clock, plus the two register stages to fill
            assert W * H <= cyc <= W * H + 3
            dut.reset()
            got2, _ = dut.run(frame, out_ready_pattern=[1, 0, 0, 1, 1, 0])
            assert np.array_equal(got2, got)
    with pytest.raises(csic.IllegalArgumentException):                 # ImageProcessor.scala:25 via ImageProcessorParams
        csic.ImageProcessorParams(10, 8, 4, 4, 4)


def test_single_stage_models_match_the_oracle_stage_by_stage(S, oracle):
    """ChromaSubsampler alone on a YCbCr stream (how ChromaSubsamplerImageSpec.scala:150-170 drives it)."""
    rng = np.random.default_rng(11)
    W, H = 13, 7
    src = rng.integers(0, 1 << 24, W * H, dtype=np.uint32)
    for (a, b) in [(4, 4), (2, 2), (2, 0), (1, 1), (1, 0)]:
        h, v = 4 // a, (2 if b == 0 else 1)
        with S.ChromaSubsampler(W, H, 8, a, b) as dut:
            got, _ = dut.run(src, out_ready_pattern=[1, 1, 0])
        y = src & 255
        want = np.empty_like(src)
        for i in range(W * H):                                         # SURVEY.md App. A.3 closed form
            c, r = i % W, i // W
            s = i - (c % h) if r % v == 0 else (r - 1) * W + ((W - 1) // h) * h
            want[i] = y[i] | (src[s] & 0xFFFF00)
        assert np.array_equal(got, want), (a, b)


# ---- timing -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("op", [(3, 1, 2), (1, 2, 3), (2, 3, 1)])
def test_top_never_exceeds_half_a_pixel_per_clock(S, oracle, op):
    """Queue(gen, 1) with pipe = false cannot enqueue and dequeue in one cycle (ImageCompressorTop.scala:63-65): the input side
    accepts at most one pixel every two cycles, whatever the consumer does."""
    W, H, f = 32, 16, 2
    frame = oracle.synth_frame(W * H, 3)
    with S.ImageCompressorTop(W, H, 2, 0, 8, 8, 8, f, *op) as dut:
        dut.poke(out_ready=True)
        accepted, last_accept, cycles = 0, -10, 0
        while accepted < W * H:
            dut.poke(in_valid=True, in_bits=int(frame[accepted]))
            if dut.peek().in_ready:
                assert cycles - last_accept >= 2 or accepted < 2       # (the first two pixels fill the empty slice + queue)
                last_accept = cycles
                accepted += 1
            dut.step()
            cycles += 1
        assert cycles >= 2 * W * H - 2
        dut.reset()
        out, cyc = dut.run(frame)
        assert out.size == (W // f) * (H // f)
        assert 2 * W * H - 2 <= cyc <= 2 * W * H + 16                  # 0.5 px/clk + the pipeline's depth


def test_app_collection_budget(S, oracle):
    """ImageCompressorTopApp.scala:110: the collector stops after Wo*Ho*40 + 10000 cycles.  At 2 cycles per INPUT pixel the run
    needs ~2*W*H cycles, so the budget holds for f <= 4 (40 / f^2 >= 2.5) at any size -- and for f = 8 (40 / 64 = 0.625) only
    while 1.375 * W * H < 10000.  The model predicts that the app's own default invocation (in128x128.png, sf = 8,
    ImageCompressorTopApp.scala:164-173) collects 160 of its 256 pixels before the budget runs out; the rest of that
    output image keeps its magenta fill (:133).  No committed output of the reference covers a default run: a prediction of
    the model, not a pinned fact."""
    spatial, color, chroma = 1, 2, 3
    for f, (W, H) in itertools.product((1, 2, 4), ((16, 16), (128, 128), (256, 64))):
        frame = oracle.synth_frame(W * H, f)
        with S.ImageCompressorTop(W, H, 2, 0, 8, 8, 8, f, chroma, spatial, color) as dut:
            out, cyc = dut.run(frame, max_out=(W // f) * (H // f), max_cycles=dut.collection_budget())
            assert out.size == (W // f) * (H // f) and cyc <= dut.collection_budget(), (f, W, H)
    # f = 8, small frame: fits
    with S.ImageCompressorTop(64, 64, 4, 4, 8, 8, 8, 8, spatial, color, chroma) as dut:
        out, cyc = dut.run(oracle.synth_frame(64 * 64, 1), max_out=64, max_cycles=dut.collection_budget())
        assert out.size == 64 and cyc < dut.collection_budget()
    # the app's defaults: 128x128, 4:4:4, 8/8/8, sf = 8, spatial -> color -> chroma
    with S.ImageCompressorTop(128, 128, 4, 4, 8, 8, 8, 8, spatial, color, chroma) as dut:
        assert dut.collection_budget() == 256 * 40 + 10000
        frame = oracle.synth_frame(128 * 128, 2)
        out, cyc = dut.run(frame, max_out=256, max_cycles=dut.collection_budget())
        assert cyc == dut.collection_budget() and out.size == 160
        full, cyc_full = S.ImageCompressorTop(128, 128, 4, 4, 8, 8, 8, 8, spatial, color, chroma).run(frame)
        assert full.size == 256 and np.array_equal(full[:160], out) and cyc_full > dut.collection_budget()


def test_sof_eol_are_accepted_and_ignored(S, oracle):
    """SpatialDownsampler.scala:11-12 declares sof / eol and no logic reads them."""
    W, H = 12, 6
    frame = oracle.synth_frame(W * H, 9)
    outs = []
    for sof, eol in ((False, False), (True, True)):
        with S.ImageCompressorTop(W, H, 2, 0, 5, 5, 5, 2, 3, 1, 2) as dut:
            dut.poke(out_ready=True, sof=sof, eol=eol)
            got, i = [], 0
            for _ in range(4 * W * H):
                dut.poke(in_valid=i < W * H, in_bits=int(frame[min(i, W * H - 1)]))
                sig = dut.peek()
                if sig.out_valid:
                    got.append(sig.out_bits)
                if sig.in_ready and i < W * H:
                    i += 1
                dut.step()
            outs.append(got)
    assert outs[0] == outs[1] and len(outs[0]) == (W // 2) * (H // 2)


def test_the_model_is_not_reachable_from_the_compute_path():
    """The cycle model simulates interface timing; the image path must never route through it (no CPU fallback)."""
    import os
    from conftest import ROOT
    pkg = os.path.join(ROOT, "chroma-subsampling-image-compressor_amd")
    for name in ("compressor.py", "pipeline.py", "distributed.py", "model.py", "stages.py"):
        src = open(os.path.join(pkg, name)).read()
        assert "csic_stream" not in src and "from .stream" not in src and "import stream" not in src, name
    for name in ("csic_kernels.hip", "csic_select.cpp", "csic_select.h", "csic_hip_common.h", "csic_pipeline.hip", "csic_multi.hip", "csic_graph.hip", "csic_png.cpp"):
        assert "csic_stream" not in open(os.path.join(pkg, "csrc", name)).read(), name
