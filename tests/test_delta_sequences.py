"""What the temporal layer is worth, on the host: four sequences of 8 frames built from tests/golden/inputs/in512.png, at three
parameter sets and both codings, written as version-5 files (gop 8: one key frame, seven delta frames) and as the same frames each
coded alone (versions 3 / 4).  The stored size of every frame must equal the size the numpy statement gives -- the delta of
tests/delta_ref.py, then the formats' size formulas, which are checked against the byte-exact numpy encoders on one frame first.

    A   a static frame, a 96 x 96 patch of it moving 24 px per frame        must be strictly below half of the key-only total
    C   the same frame with +-1 RGB noise per frame                          printed
    D   the left half scrolls 3 rows per frame, the right half is static     printed
    B   the whole frame pans 2 px per frame                                  printed (no motion compensation: nothing to gain)

The printed table is the one tools/delta_rates.py puts into profiles/r16_delta_rates.md.  The CLI round trip is here too (it needs a
device: compress --inputs runs the device codecs)."""
import os

import numpy as np
import pytest

from conftest import GOLDEN, load_png_rgb
from delta_ref import frame_buffers, ref_delta, ref_map_layout
from test_container import CSQ, _c_params, _layout
from test_pack_host import codes_of, ref_encode, ref_groups, ref_layout
from test_rice_host import BLOCK, ref_encode_rice, ref_modes, ref_rice_layout

import csic_amd as csic

N = csic._native
SETS = [(2, 0, (6, 5, 5)), (4, 4, (8, 8, 8)), (2, 0, (3, 3, 2))]           # factor 1, order chroma, spatial, quant
NFRAMES = 8


def sequences(rgb):
    """{name: 8 frames (H, W, 3) uint8} from one image."""
    rng = np.random.default_rng(17000)
    H, W, _ = rgb.shape
    patch = rgb[208:304, 208:304].copy()
    A, B, C_, D = [], [], [], []
    for k in range(NFRAMES):
        a = rgb.copy()
        a[32 + 24 * k:128 + 24 * k, 32 + 24 * k:128 + 24 * k] = patch
        A.append(a)
        B.append(np.roll(rgb, 2 * k, axis=1))
        C_.append(np.clip(rgb.astype(np.int16) + rng.integers(-1, 2, rgb.shape), 0, 255).astype(np.uint8))
        d = rgb.copy()
        d[:, :W // 2] = np.roll(rgb[:, :W // 2], 3 * k, axis=0)
        D.append(d)
    return {"A": A, "C": C_, "D": D, "B": B}


def size_groups(planes, bits):
    """coded_bytes of the group coding: fixed_bytes + 4 * the sum of the widths."""
    return ref_layout([c.size for c in planes], bits)[3] + 4 * sum(int(ref_groups(c, q)[0].sum()) for c, q in zip(planes, bits))


def size_rice(planes, bits):
    """coded_bytes of the Rice coding: fixed_bytes + 4 * per block (ceil(R bits / 32) + ceil(U bits / 32))."""
    total = ref_rice_layout([c.size for c in planes], bits)["fixed"]
    for c, q in zip(planes, bits):
        u = ref_groups(c, q)[2]
        m = ref_modes(u, q)
        k = np.where(m == 15, 0, m)
        r = np.where(m == 15, 0, 31 * k)
        un = np.where((m != 15) & (m < q), ((u[:, 1:] >> k[:, None]) + 1).sum(axis=1), 0)
        at = np.arange(0, m.size, BLOCK)
        total += 4 * int(((np.add.reduceat(r, at) + 31) // 32 + (np.add.reduceat(un, at) + 31) // 32).sum())
    return total


SIZE_OF = {"groups": size_groups, "rice": size_rice}


def test_the_size_formulas_are_the_encoders_sizes(oracle):
    rng = np.random.default_rng(17100)
    for W, H, bits in ((97, 33, (6, 5, 5)), (300, 40, (8, 3, 1)), (31, 1, (2, 2, 7))):
        argb = (np.cumsum(rng.integers(-3, 4, W * H)).astype(np.uint32) * np.uint32(0x010203)) ^ (rng.integers(0, 1 << 32, W * H, dtype=np.uint32) & np.uint32(0x00030303))
        planes = codes_of(oracle, W, H, 2, 0, bits, 1, CSQ, 0, False, argb)
        assert size_groups(planes, bits) == len(ref_encode(planes, bits))
        assert size_rice(planes, bits) == len(ref_encode_rice(planes, bits))


def test_sequences_from_in512(oracle, tmp_path, capsys):
    rgb = load_png_rgb(os.path.join(GOLDEN, "inputs", "in512.png"))
    seqs = sequences(rgb)
    lines = ["sequence  coding  " + "  ".join(f"4:{a}:{b} {q[0]}/{q[1]}/{q[2]}" for a, b, q in SETS) + "   groups taken inter"]
    ratios = {}
    for name, frames_rgb in seqs.items():
        row = {"groups": [], "rice": []}
        share = []
        for a, b, bits in SETS:
            cp = _c_params(512, 512, a, b, bits, 1, CSQ)
            lay = _layout(cp)
            frames = [codes_of(oracle, 512, 512, a, b, bits, 1, CSQ, 0, False, oracle.rgb_to_argb(f).reshape(-1)) for f in frames_rgb]
            diffs, maps, ts = ref_delta(frames, bits, NFRAMES)
            mb = ref_map_layout([c.size for c in frames[0]])[2]
            buf = frame_buffers(lay, frames, bits, 0)
            share.append(sum(int(t.sum()) for fr in ts[1:] for t in fr) / ((NFRAMES - 1) * sum(ref_map_layout([c.size for c in frames[0]])[0])))
            for coding in ("groups", "rice"):
                seq, alone = str(tmp_path / "seq.csic"), str(tmp_path / "alone.csic")
                csic.write_container(seq, cp, buf, coding=coding, gop=NFRAMES)
                csic.write_container(alone, cp, buf, coding=coding)
                got = csic.container_coded_sizes(seq).tolist()
                want = [SIZE_OF[coding](d, bits) + (mb if k else 0) for k, d in enumerate(diffs)]
                assert got == want, (name, a, b, bits, coding)                  # the library's sizes are the numpy reference's
                key_only = csic.container_coded_sizes(alone).tolist()
                assert key_only[0] == got[0]
                assert np.array_equal(csic.read_container(seq)[2], buf)
                assert csic.container_inter_groups(seq)[1:].sum() == sum(int(t.sum()) for fr in ts[1:] for t in fr)
                ratios[(name, coding, bits)] = sum(got) / sum(key_only)
                row[coding].append(ratios[(name, coding, bits)])
        for coding in ("groups", "rice"):
            lines.append(f"{name:<9} {coding:<7} " + "  ".join(f"{r:>11.3f}" for r in row[coding]) + f"   {min(share):.2f}-{max(share):.2f}")
    with capsys.disabled():
        print("\n" + "\n".join(lines))
    for (name, coding, bits), r in ratios.items():
        if name == "A":
            assert r < 0.5, (coding, bits, r)                                   # content that stays put: below half of what it costs frame by frame


@pytest.mark.gpu
def test_cli_sequence_round_trip(tmp_path, capsys):
    """compress --inputs ... decompress --frame reproduces, for every frame, the PNG that the single-frame path gives for that frame."""
    from PIL import Image
    assert N.lib().csic_device_count() >= 1
    rgb = load_png_rgb(os.path.join(GOLDEN, "inputs", "in512.png"))
    frames = sequences(rgb)["A"][:3]
    pngs = []
    for k, f in enumerate(frames):
        pngs.append(str(tmp_path / f"in{k}.png"))
        Image.fromarray(f).save(pngs[-1])
    common = ["--a", "2", "--b", "0", "--yq", "6", "--cbq", "5", "--crq", "5", "--sf", "1", "--op1", "chroma", "--op2", "spatial", "--op3", "color"]
    for coding in ("groups", "rice"):
        seq = str(tmp_path / f"seq_{coding}.csic")
        assert csic.app.main(["compress", "--inputs", ",".join(pngs), "--gop", "2", "--coding", coding, "--output", seq] + common) == 0
        info = csic.container_info(seq)
        assert (info.version, info.nframes, info.gop) == (5, 3, 2)
        host = str(tmp_path / "host.csic")
        csic.write_container(host, info.params, csic.read_container(seq)[2], coding=coding, gop=2)
        assert open(host, "rb").read() == open(seq, "rb").read()               # the device's file is the host writer's
        assert csic.app.main(["decompress", "--input", seq, "--output-pattern", str(tmp_path / f"all_{coding}_%d.png")]) == 0
        singles = 0
        for k, png in enumerate(pngs):
            one, out, single = str(tmp_path / "one.csic"), str(tmp_path / "frame.png"), str(tmp_path / "single.png")
            assert csic.app.main(["compress", "--input", png, "--output", one, "--coding", coding] + common) == 0
            assert csic.app.main(["decompress", "--input", one, "--output", single]) == 0
            singles += os.path.getsize(one)
            assert csic.app.main(["decompress", "--input", seq, "--output", out, "--frame", str(k)]) == 0
            assert open(out, "rb").read() == open(single, "rb").read()
            assert open(tmp_path / f"all_{coding}_{k}.png", "rb").read() == open(single, "rb").read()
        assert os.path.getsize(seq) < singles                                   # the delta frame in the middle is the smaller record
    capsys.readouterr()
    assert csic.app.main(["inspect", "--input", seq]) == 0
    text = capsys.readouterr().out
    assert "version 5" in text and "temporal delta with gop 2" in text and "frame 1 (delta)" in text and "inter groups Y" in text
    assert csic.app.main(["compress", "--inputs", ",".join(pngs), "--coding", "raw", "--output", seq] + common) == 2
    with pytest.raises(csic.IllegalArgumentException):
        csic.app.main(["decompress", "--input", seq, "--output", str(tmp_path / "x.png"), "--frame", "3"])
