// csic_internal.h -- shared between the host-only translation unit and the HIP one.
#pragma once
#include "csic.h"

#include <cstdarg>
#include <cstddef>
#include <cstdint>

namespace csic {

// Derived, validated geometry of one parameter set.
struct Geometry {
    int32_t W, H;        // input
    int32_t Wo, Ho;      // output, ceil(W/f) x ceil(H/f)
    int32_t f;           // spatial factor
    int32_t h, v;        // chroma horizontal / vertical hold factors: h = 4/a, v = (b == 0) ? 2 : 1
    int32_t s_first;     // 1 = spatial stage sits before the chroma stage (order class S-before-C)
    int32_t last_sample_col; // ((W-1)/h)*h : column of the last chroma sample of a (chroma) row
    uint32_t mask_y, mask_cb, mask_cr; // quantiser AND masks, 0xFF << (8 - bits)
};

int  set_error(int status, const char *fmt, ...) __attribute__((format(printf, 2, 3)));
void clear_error();
int  derive_geometry(const csic_params *p, Geometry *g);   // validates first
void planar_layout(const Geometry &g, const csic_params *p, csic_planar_layout *layout);   // csic.h: CSIC_FMT_PLANAR
void planar_bits_layout(const Geometry &g, const csic_params *p, csic_planar_bits_layout *layout);   // csic.h: CSIC_FMT_PLANAR_BITS

// csic_pack_host.cpp: the group coding (csic.h: csic_pack_*).  Everything both codecs, the Rice coding and the container derive from the
// parameters, the host codec on one frame, and the checks csic_unpack_host makes on their own (csic_container_write_coded).
constexpr int64_t RICE_BLOCK = 256;           // groups per block: a block of the Rice format and of both device codecs' kernels
struct PackGeometry {
    csic_planar_bits_layout bits;             // the PLANAR_BITS frame the coding reads and restores
    csic_pack_layout layout;
    int64_t n[3];                             // samples per plane
    int32_t q[3];                             // bits per code
    int64_t src_offset[3], src_bytes[3];      // the planes' payload ranges inside a frame buffer
    int64_t max_payload_dwords;               // sum of G_p q_p: no frame's payload is longer
    int64_t blocks[3], block0[3], nblocks;    // blocks of RICE_BLOCK groups: per plane, a plane's first block number, per frame (NB)
};
int pack_geometry(const csic_params *p, PackGeometry *G);     // validates first (out_format ignored)
int pack_frame(const PackGeometry &G, const unsigned char *frame, unsigned char *coded, size_t capacity, uint64_t *coded_bytes);
int unpack_frame(const PackGeometry &G, const unsigned char *coded, size_t coded_bytes, unsigned char *frame);
int pack_check_coded(const PackGeometry &G, const unsigned char *coded, size_t coded_bytes);

// csic_rice_host.cpp: the Rice coding (csic.h: csic_rice_*), the same three for it.  `pk` is the group coding's geometry of the same
// parameters: the PLANAR_BITS frame, n, q, the payload ranges, the groups, the blocks and -- in pk.layout -- the nibble and anchors
// sections are the group coding's; `layout` repeats them in the Rice coding's public struct.
inline int64_t rice_chunk_cap(int q) { return 248 * (int64_t)q + 1; }     // dwords: no chunk of a plane of q bits per code is longer
struct RiceGeometry {
    PackGeometry pk;
    csic_rice_layout layout;
    int64_t max_payload_dwords;               // sum of B_p (248 q_p + 1)
};
int rice_geometry(const csic_params *p, RiceGeometry *G);
int rice_pack_frame(const RiceGeometry &G, const unsigned char *frame, unsigned char *coded, size_t capacity, uint64_t *coded_bytes);
int rice_unpack_frame(const RiceGeometry &G, const unsigned char *coded, size_t coded_bytes, unsigned char *frame);
int rice_check_coded(const RiceGeometry &G, const unsigned char *coded, size_t coded_bytes);

// csic_rans_host.cpp: the rANS coding (csic.h: csic_rans_*), the same three for it.  `pk` gives the PLANAR_BITS frame, n, q, the payload
// ranges and the groups; the blocks are the rANS coding's own (1024 groups, csic_rans_decode.h) and so are all section offsets.
struct RansGeometry {
    PackGeometry pk;
    csic_rans_layout layout;
    int64_t block0[3], nblocks;               // a plane's first block number; blocks per frame (NB)
    int64_t max_payload_dwords;               // the raw chunks of all blocks
};
int rans_geometry(const csic_params *p, RansGeometry *G);
int rans_pack_frame(const RansGeometry &G, const unsigned char *frame, unsigned char *coded, size_t capacity, uint64_t *coded_bytes);
int rans_unpack_frame(const RansGeometry &G, const unsigned char *coded, size_t coded_bytes, unsigned char *frame);
int rans_check_coded(const RansGeometry &G, const unsigned char *coded, size_t coded_bytes);
// the scaling rule of csic.h: counts c[0, nsym) with sum N > 0 -> frequencies f[0, nsym) with sum M
void rans_scale_counts(const uint32_t *c, int nsym, uint64_t N, uint16_t *f);

// csic_delta_host.cpp: the temporal layer (csic.h: csic_delta_*).  `pk` is the group coding's geometry of the same parameters; `layout`
// is the map's.  delta_frame writes the difference frame of `cur` against `prev` (NULL: a key frame) and its map; undelta_frame is the
// inverse; both allow diff == cur.  delta_check_map is what csic_undelta_host and the container ask of a map nobody vouches for.
struct DeltaGeometry {
    PackGeometry pk;
    csic_delta_layout layout;
};
int delta_geometry(const csic_params *p, DeltaGeometry *G);
void delta_frame(const DeltaGeometry &G, const unsigned char *cur, const unsigned char *prev, unsigned char *diff, unsigned char *map);
void undelta_frame(const DeltaGeometry &G, const unsigned char *diff, const unsigned char *map, const unsigned char *prev, unsigned char *cur);
int delta_check_map(const DeltaGeometry &G, const unsigned char *map, bool key, int frame);

// csic_mc_host.cpp: the motion-compensated temporal layer (csic.h: csic_mc_*), the same for it.  mc_candidates writes the (2 range + 1)^2
// candidates in rank order and returns their number; neither frame function works in place.  mc_check_range is the refusal of a range
// outside 0..MC_MAX_RANGE.  What both layers refuse of a call is temporal_check_call of csic_temporal_host.h.
constexpr int MC_MAX_RANGE = 7, MC_MAX_CANDIDATES = (2 * MC_MAX_RANGE + 1) * (2 * MC_MAX_RANGE + 1);
constexpr int MC_TABLE_WORDS = 16, MC_TABLE_BYTES = 4 * MC_TABLE_WORDS;
constexpr int MC_COUNTERS = 256;              // vote counters per frame and plane in the device codec's workspace (>= MC_MAX_CANDIDATES)
struct McGeometry {
    PackGeometry pk;
    csic_mc_layout layout;
};
struct McCandidate { int dy, dx; };
int mc_geometry(const csic_params *p, McGeometry *G);
int mc_candidates(int range, McCandidate *out);
void mc_delta_frame(const McGeometry &G, const unsigned char *cur, const unsigned char *prev, int range, unsigned char *diff, unsigned char *map);
void mc_undelta_frame(const McGeometry &G, const unsigned char *diff, const unsigned char *map, const unsigned char *prev, unsigned char *cur);
int mc_check_map(const McGeometry &G, const unsigned char *map, bool key, int frame);
int mc_check_range(int32_t range);

// csic_rows_host.cpp: the row-prediction layer (csic.h: csic_rows_*), the same for it: a frame stands alone, so there is no previous
// frame and no gop.  rows_frame does not work in place, unrows_frame does.
constexpr int ROWS_BAND = CSIC_ROWS_BAND;
struct RowsGeometry {
    PackGeometry pk;
    csic_rows_layout layout;
};
int rows_geometry(const csic_params *p, RowsGeometry *G);
void rows_frame(const RowsGeometry &G, const unsigned char *frame, unsigned char *diff, unsigned char *map);
void unrows_frame(const RowsGeometry &G, const unsigned char *diff, const unsigned char *map, unsigned char *frame);
int rows_check_map(const RowsGeometry &G, const unsigned char *map, int frame);

// Exact unsigned division by a run-time constant without a divide (k_generic's stream-index arithmetic): for
// 1 <= d < 2^31 and every n < 2^31,  n / d == (uint64(n) * m) >> k  with  k = 31 + ceil(log2 d),  m = ceil(2^k / d) < 2^32.
// (Error term e = m*d - 2^k < d <= 2^ceil(log2 d), and n * e < 2^31 * 2^ceil(log2 d) = 2^k.)  Host side, csic_host.cpp;
// checked against the hardware divide over edge cases and random pairs in tests/cpp/host_sanitize.cpp.
void magic_div(uint32_t d, uint32_t *m, uint32_t *k);

// csic_inflate.cpp: what the PNG reader needs of zlib, faster.  zlib_decode_exact: 0 if in[0, in_len) is a well-formed zlib
// stream of exactly out_len bytes with the right check value (1 corrupt, 2 truncated, 3 longer, 4 shorter than out_len).
int      zlib_decode_exact(const unsigned char *in, size_t in_len, unsigned char *out, size_t out_len);
uint32_t crc32_update(uint32_t crc, const unsigned char *p, size_t n);      // crc32_update(0, ..) starts a CRC, as zlib's crc32
uint32_t adler32_update(uint32_t adler, const unsigned char *p, size_t n);  // adler32_update(1, ..) starts a sum, as zlib's adler32

// csic_png.cpp: csic_png_write_argb on a given number of threads (<= 0: CSIC_PNG_THREADS or up to 16); the bytes written do
// not depend on it.  The file pools of csic_files.hip, parallel over files already, ask for 1.
int png_write_argb_threads(const char *path, const uint32_t *src, int32_t width, int32_t height, int32_t level, int threads);

} // namespace csic
