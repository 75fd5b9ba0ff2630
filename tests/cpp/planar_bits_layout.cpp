// tests/cpp/planar_bits_layout.cpp -- prints ImageCompressorTop::planarBitsLayout() (include/csic.hpp; no GPU needed) for the
// parameter sets given on the command line, one line each:  W H a b yb cbb crb f op1 op2 op3  ->  the layout's fields.
// tests/test_planar_bits_layout.py compares the lines with what the Python host reports.
#include <cstdio>
#include <cstdlib>

#include "csic.hpp"

int main(int argc, char **argv)
{
    for (int i = 1; i + 11 <= argc; i += 11) {
        int v[11];
        for (int k = 0; k < 11; ++k) v[k] = std::atoi(argv[i + k]);
        csic::ImageCompressorTop top(v[0], v[1], v[2], v[3], v[4], v[5], v[6], v[7], (csic::ProcessingStep)v[8],
                                     (csic::ProcessingStep)v[9], (csic::ProcessingStep)v[10]);
        const csic_planar_bits_layout L = top.planarBitsLayout();
        std::printf("%d %d %d %d %d %d %d %d %lld %d %d %d %lld %lld %lld %lld %lld %lld %lld %lld\n", L.geometry.y_width,
                    L.geometry.y_height, L.geometry.chroma_width, L.geometry.chroma_height, L.geometry.module_width, L.geometry.hold_h,
                    L.geometry.hold_v, L.geometry.replay_last, (long long)L.geometry.chroma_samples, L.y_bits, L.cb_bits, L.cr_bits,
                    (long long)L.y_bytes, (long long)L.cb_bytes, (long long)L.cr_bytes, (long long)L.y_offset, (long long)L.cb_offset,
                    (long long)L.cr_offset, (long long)L.frame_bytes, (long long)L.payload_bytes);
    }
    return 0;
}
