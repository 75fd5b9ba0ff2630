"""What the motion-compensated temporal layer is worth, on the host: sequences A, B and D of tests/test_delta_sequences.py and a diagonal
pan, 8 frames each built from tests/golden/inputs/in512.png, at that file's three parameter sets and both codings, written as version-6
files (gop 8: one key frame, seven delta frames) and as the same frames each coded alone (versions 3 / 4).  The stored size of every
frame of every file must equal the size the numpy statement gives: the delta of tests/mc_ref.py -- difference frames and maps are
compared byte for byte on all 8 frames as well --, then the formats' size formulas of tests/test_delta_sequences.py, plus map_bytes
for a delta frame.

    B   the whole frame pans 2 px per frame, range 2          GATE: strictly below half of the key-only total, every set, both codings
                                                               (csic_delta_* stores it at 1.00 - 1.01)
    A   a static frame with a moving patch, range 2           printed: the 4-bit map costs more than csic_delta_*'s 1-bit map gains
    D   the left half scrolls 3 rows per frame, range 4       printed
    P   the whole frame pans (3, -2) per frame, range 4       printed

The ratios are printed next to those of csic_delta_* on the same frames.  The CLI round trip is here too (it needs a device:
compress --inputs --motion runs the device codecs): the device's file is the host writer's, byte for byte."""
import os

import numpy as np
import pytest

from conftest import GOLDEN, load_png_rgb
from delta_ref import frame_buffers, ref_delta, ref_map_layout
from mc_ref import ref_mc_delta, ref_mc_layout
from test_container import CSQ, _c_params, _layout
from test_delta_sequences import NFRAMES, SETS, SIZE_OF, sequences
from test_pack_host import codes_of

import csic_amd as csic

CASES = {"B": 2, "A": 2, "D": 4, "P": 4}                                     # sequence: range


def _frames_rgb(name):
    rgb = load_png_rgb(os.path.join(GOLDEN, "inputs", "in512.png"))
    if name == "P":
        return [np.roll(np.roll(rgb, 3 * k, axis=0), -2 * k, axis=1) for k in range(NFRAMES)]
    return sequences(rgb)[name]


@pytest.mark.parametrize("name", list(CASES))
def test_sequences_from_in512(oracle, tmp_path, capsys, name):
    R = CASES[name]
    lines = []
    for a, b, bits in SETS:
        cp = _c_params(512, 512, a, b, bits, 1, CSQ)
        lay, ml = _layout(cp), csic.mc_layout(cp)
        frames = [codes_of(oracle, 512, 512, a, b, bits, 1, CSQ, 0, False, oracle.rgb_to_argb(f).reshape(-1)) for f in _frames_rgb(name)]
        ns = [c.size for c in frames[0]]
        mb = ref_mc_layout(ns)[3]
        assert mb == ml.map_bytes
        buf = frame_buffers(lay, frames, bits, 0)
        diff, maps = csic.mc_delta_host(cp, buf, NFRAMES, R)
        assert np.array_equal(csic.mc_undelta_host(cp, diff, maps, NFRAMES), buf)
        widths = [lay.geometry.y_width, lay.geometry.chroma_width, lay.geometry.chroma_width]
        ref_d, ref_m, minfo = ref_mc_delta(frames, bits, widths, NFRAMES, R)
        assert np.array_equal(diff, frame_buffers(lay, ref_d, bits, 0))
        assert all(maps[k, :mb].tobytes() == ref_m[k] for k in range(NFRAMES))
        old_d, _, _ = ref_delta(frames, bits, NFRAMES)
        old_mb = ref_map_layout(ns)[2]
        for coding in ("groups", "rice"):
            seq, alone = str(tmp_path / "seq.csic"), str(tmp_path / "alone.csic")
            csic.write_container(seq, cp, buf, coding=coding, gop=NFRAMES, motion=R)
            csic.write_container(alone, cp, buf, coding=coding)
            info = csic.container_info(seq)
            assert (info.version, info.gop, info.motion) == (6, NFRAMES, R)
            got = csic.container_coded_sizes(seq).tolist()
            want = [SIZE_OF[coding](d, bits) + (mb if k else 0) for k, d in enumerate(ref_d)]
            assert got == want, (name, a, b, bits, coding)                              # every stored size is the numpy statement's
            key_only = csic.container_coded_sizes(alone).tolist()
            assert key_only[0] == got[0]
            assert np.array_equal(csic.read_container(seq)[2], buf)
            assert csic.container_inter_groups(seq)[1:].sum() == sum(int(np.count_nonzero(nib)) for fr in minfo[1:] for _, nib in fr)
            ratio = sum(got) / sum(key_only)
            plain = sum(SIZE_OF[coding](d, bits) + (old_mb if k else 0) for k, d in enumerate(old_d)) / sum(key_only)
            per_delta = (sum(got) - got[0]) / (sum(key_only) - key_only[0])
            lines.append(f"{name} range {R}  4:{a}:{b} {bits[0]}/{bits[1]}/{bits[2]}  {coding:<7} csic_delta {plain:.3f} -> csic_mc {ratio:.3f} of key-only"
                         f"  (delta frames alone {per_delta:.3f})")
            if name == "B":
                assert ratio < 0.5, (coding, bits, ratio)                               # the gate: a pan, the key frame included
    with capsys.disabled():
        print("\n" + "\n".join(lines))


@pytest.mark.gpu
def test_cli_sequence_round_trip(tmp_path, capsys):
    """compress --inputs ... --motion R writes the host writer's file, byte for byte; decompress --frame reproduces, for every frame, the
    PNG that the single-frame path gives for that frame; inspect prints the range and the tables."""
    from PIL import Image
    assert csic._native.lib().csic_device_count() >= 1
    frames = _frames_rgb("B")[:3]
    pngs = []
    for k, f in enumerate(frames):
        pngs.append(str(tmp_path / f"in{k}.png"))
        Image.fromarray(f).save(pngs[-1])
    common = ["--a", "2", "--b", "0", "--yq", "6", "--cbq", "5", "--crq", "5", "--sf", "1", "--op1", "chroma", "--op2", "spatial", "--op3", "color"]
    for coding in ("groups", "rice"):
        seq = str(tmp_path / f"seq_{coding}.csic")
        assert csic.app.main(["compress", "--inputs", ",".join(pngs), "--gop", "2", "--motion", "2", "--coding", coding, "--output", seq] + common) == 0
        info = csic.container_info(seq)
        assert (info.version, info.nframes, info.gop, info.motion) == (6, 3, 2, 2)
        host = str(tmp_path / "host.csic")
        csic.write_container(host, info.params, csic.read_container(seq)[2], coding=coding, gop=2, motion=2)
        assert open(host, "rb").read() == open(seq, "rb").read()               # the device's file is the host writer's
        singles = 0
        for k, png in enumerate(pngs):
            one, out, single = str(tmp_path / "one.csic"), str(tmp_path / "frame.png"), str(tmp_path / "single.png")
            assert csic.app.main(["compress", "--input", png, "--output", one, "--coding", coding] + common) == 0
            assert csic.app.main(["decompress", "--input", one, "--output", single]) == 0
            singles += os.path.getsize(one)
            assert csic.app.main(["decompress", "--input", seq, "--output", out, "--frame", str(k)]) == 0
            assert open(out, "rb").read() == open(single, "rb").read()
        assert os.path.getsize(seq) < singles                                   # the panned frame in the middle is the smaller record
    capsys.readouterr()
    assert csic.app.main(["inspect", "--input", seq]) == 0
    text = capsys.readouterr().out
    assert "version 6" in text and "motion-compensated delta with gop 2, range 2" in text and "frame 1 (delta)" in text
    assert "Y table: intra" in text and "(0, -2)" in text                      # the pan: the picture moves 2 px to the right
