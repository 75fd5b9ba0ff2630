// delta_hpp_test.cpp -- csic.hpp's wrappers of the temporal layer without a GPU: deltaLayout, delta, undelta, writeContainerSeq,
// containerGop, and the refusals as exceptions.  Built and run by tests/test_cpp_delta_hpp.py against libcsic_hip.so.
#include <cstdio>
#include <string>

#include "csic.hpp"

#define REQUIRE(cond) do { if (!(cond)) { std::printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #cond); return 1; } } while (0)

int main(int argc, char **argv)
{
    const std::string dir = argc > 1 ? argv[1] : ".";
    csic_params p;
    REQUIRE(csic_params_default(&p, 100, 9) == CSIC_OK);
    p.chroma_a = 2; p.chroma_b = 0; p.factor = 1; p.y_bits = 6; p.cb_bits = 5; p.cr_bits = 5;
    p.op[0] = CSIC_OP_CHROMA; p.op[1] = CSIC_OP_SPATIAL; p.op[2] = CSIC_OP_QUANT;
    csic_params q = p;
    q.out_format = CSIC_FMT_PLANAR_BITS;
    csic_planar_bits_layout B;
    REQUIRE(csic_planar_bits_layout_of(&q, &B) == CSIC_OK);
    const csic_delta_layout L = csic::deltaLayout(p);
    REQUIRE(L.groups[0] == (100 * 9 + 31) / 32 && L.map_bytes == 4 * 3 && L.map_stride == 256 && L.map_offset[2] == 8);

    // three frames: a ramp, the same ramp again, another ramp; whole bytes of valid codes (6 bits used of every 6, 5 of every 5: any byte is)
    const int n = 3, gop = 3;
    const size_t fb = (size_t)B.frame_bytes;
    std::vector<uint8_t> frames(n * fb, 0);
    const int64_t off[3] = {B.y_offset, B.cb_offset, B.cr_offset}, bytes[3] = {B.y_bytes, B.cb_bytes, B.cr_bytes};
    for (int pl = 0; pl < 3; ++pl)
        for (int64_t i = 0; i + 1 < bytes[pl]; ++i) {                  // (the last byte stays 0: its unused high bits must be)
            frames[(size_t)(off[pl] + i)] = frames[fb + (size_t)(off[pl] + i)] = (uint8_t)(i * 7 + pl);
            frames[2 * fb + (size_t)(off[pl] + i)] = (uint8_t)(i * 5 + 1);
        }
    const csic::DeltaFrames d = csic::delta(p, frames.data(), n, gop);
    REQUIRE(d.diff.size() == frames.size() && d.maps.size() == (size_t)n * (size_t)L.map_stride);
    for (int64_t i = 0; i < L.map_bytes; ++i) REQUIRE(d.maps[(size_t)i] == 0);                         // the key frame's map
    REQUIRE(d.maps[(size_t)L.map_stride] == 0xFF);                                                     // an identical frame: every group inter
    for (size_t i = 0; i < fb; ++i) REQUIRE(d.diff[fb + i] == 0);                                      // and its difference frame is zero
    REQUIRE(csic::undelta(p, d.diff.data(), d.maps.data(), n, gop) == frames);

    const std::string file = dir + "/seq.csic";
    csic::writeContainerSeq(file, p, frames.data(), n, CSIC_CODING_RICE, gop);
    REQUIRE(csic::containerGop(file) == gop && csic::containerInfo(file).version == 5);
    const csic::Container c = csic::readContainer(file);
    REQUIRE(c.nframes == n && c.bytes == frames);
    csic::writeContainer(dir + "/alone.csic", p, frames.data(), n, CSIC_CODING_RICE);
    REQUIRE(csic::containerGop(dir + "/alone.csic") == 1);
    const std::vector<uint64_t> seq = csic::containerCodedSizes(file), alone = csic::containerCodedSizes(dir + "/alone.csic");
    REQUIRE(seq[0] == alone[0] && seq[1] < alone[1]);

    // refusals surface as exceptions with the library's status
    int caught = 0;
    try { csic::delta(p, frames.data(), n, 0); } catch (const std::exception &) { ++caught; }
    try { csic::writeContainerSeq(file, p, frames.data(), n, CSIC_CODING_RAW, gop); } catch (const std::exception &) { ++caught; }
    std::vector<uint8_t> bad = d.maps;
    bad[0] = 1;                                                                                        // a bit in the key frame's map
    try { csic::undelta(p, d.diff.data(), bad.data(), n, gop); } catch (const std::exception &) { ++caught; }
    REQUIRE(caught == 3);
    std::printf("all checks passed\n");
    return 0;
}
