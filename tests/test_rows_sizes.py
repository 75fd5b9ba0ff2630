"""What the row-prediction layer is worth, on the host: tests/golden/inputs/in512.png at factor 1, four parameter sets and the three
codings, written as version-8 files and as the same frame coded alone (versions 3 / 4 / 7).  Every stored size must equal what the
numpy statement gives -- the layer of tests/rows_ref.py, then the formats' size formulas (tests/test_delta_sequences.py) or the byte-exact
rANS encoder (tests/test_rans_host.py), plus map_bytes --, and every version-8 file must be strictly smaller than the file without the
layer.  The printed table is the source of the README's "RANS + rows" column and of profiles/r23_rows_rates.md."""
import os

import numpy as np

from conftest import GOLDEN, load_png_rgb
from delta_ref import frame_buffers, ref_map_layout
from rows_ref import ref_rows
from test_container import CSQ, _c_params, _layout
from test_delta_sequences import SIZE_OF
from test_pack_host import codes_of
from test_rans_host import ref_encode_rans
from test_rows_host import plane_widths

import csic_amd as csic

SETS = [(2, 0, (6, 5, 5)), (4, 4, (8, 8, 8)), (2, 0, (3, 3, 2)), (2, 0, (4, 4, 4))]       # factor 1, order chroma, spatial, quant
SIZES = dict(SIZE_OF, rans=lambda planes, bits: len(ref_encode_rans(planes, bits)))
# the stored bytes of the frame without the layer: the README's coding table
TODAY = {(6, 5, 5): (199024, 163816, 150552), (8, 8, 8): (585284, 513204, 438628), (3, 3, 2): (92876, 65788, 55328), (4, 4, 4): (134932, 98260, 91432)}


def test_in512_with_rows_is_smaller_at_every_set_and_coding(oracle, tmp_path, capsys):
    rgb = load_png_rgb(os.path.join(GOLDEN, "inputs", "in512.png"))
    argb = oracle.rgb_to_argb(rgb).reshape(-1)
    lines = ["set           coding   today   with rows  ratio   groups from above Y / Cb / Cr"]
    for a, b, bits in SETS:
        cp = _c_params(512, 512, a, b, bits, 1, CSQ)
        lay = _layout(cp)
        frame = codes_of(oracle, 512, 512, a, b, bits, 1, CSQ, 0, False, argb)
        diff, m, ts = ref_rows(frame, plane_widths(cp), bits)
        G, _, mb, _ = ref_map_layout([c.size for c in frame])
        assert len(m) == mb == csic.rows_layout(cp).map_bytes
        buf = frame_buffers(lay, [frame], bits, 0)
        share = " / ".join(f"{int(t.sum()) / g:.2f}" for t, g in zip(ts, G))
        for coding, today in zip(("groups", "rice", "rans"), TODAY[bits]):
            rows, alone = str(tmp_path / "rows.csic"), str(tmp_path / "alone.csic")
            csic.write_container(rows, cp, buf, coding=coding, rows=True)
            csic.write_container(alone, cp, buf, coding=coding)
            got, before = int(csic.container_coded_sizes(rows)[0]), int(csic.container_coded_sizes(alone)[0])
            lines.append(f"4:{a}:{b} {bits[0]}/{bits[1]}/{bits[2]}   {coding:<7} {before:>7} {got:>9}   {got / before:.3f}   {share}")
            assert before == today == SIZES[coding](frame, bits), (bits, coding)            # the figures the README has
            assert got == SIZES[coding](diff, bits) + mb, (bits, coding)                     # the library's size is the numpy statement's
            assert got < before and os.path.getsize(rows) < os.path.getsize(alone), (bits, coding)
            assert csic.container_inter_groups(rows).tolist() == [[int(t.sum()) for t in ts]]
            assert np.array_equal(csic.read_container(rows)[2], buf)
    with capsys.disabled():
        print("\n" + "\n".join(lines))
