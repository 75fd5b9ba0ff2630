// csic_container.cpp -- .csic files: CSIC_FMT_PLANAR_BITS frames on disk (host only, no device; byte layout in include/csic.h).
// A file is an 80-byte header -- magic, version, frame count, CRC-32 of everything behind the CRC field, the parameters -- and per
// frame the three planes' payload bytes back to back: the padding of a frame buffer never reaches the file, and reading zeroes it.
// Version 3 holds the frames group-coded instead (csic_pack_host.cpp): a coding word, a table of the frames' coded sizes, the coded frames;
// version 4 is the same layout with the frames Rice-coded (csic_rice_host.cpp).  What differs between the two is one row of codec_of;
// the little-endian dwords are csic_group_host.h's.  Version 5 holds a sequence through the temporal layer (csic_delta_host.cpp): the word
// behind the coding is the gop, a key frame's record is its coded frame, a delta frame's its map and then its coded difference frame.
// Version 6 is version 5 through the motion-compensated layer (csic_mc_host.cpp): its maps, and the range + 1 in bits 8.. of the coding word.
// What differs between those two is one row of layer_of.  Version 7 holds everything that is rANS-coded (csic_rans_host.cpp): the third row
// of codec_of, the coding word and the gop as in version 6 -- a range field of 0 for no motion layer, a gop of 0 for frames that stand alone.
// Version 8 holds frames that stand alone, each through the row-prediction layer (csic_rows_host.cpp) and any of the three codings: the
// third row of layer_of, bit 16 of the coding word, and a map in front of EVERY frame's coded difference frame.
#include <zlib.h>

#include <cstdio>
#include <cstring>
#include <new>
#include <vector>

#include "csic_group_host.h"

namespace csic {

constexpr size_t CONTAINER_HEADER = 80, CONTAINER_CRC_FROM = 16;
constexpr uint32_t CONTAINER_VERSION = 1, CONTAINER_VERSION_CODED = 3, CONTAINER_VERSION_RICE = 4, CONTAINER_VERSION_SEQ = 5, CONTAINER_VERSION_MC = 6,
                   CONTAINER_VERSION_RANS = 7, CONTAINER_VERSION_ROWS = 8;
constexpr uint32_t ROWS_FLAG = 1u << 16;          // version 8: the coding word is coding | ROWS_FLAG
constexpr size_t CODED_BODY = 8;                  // versions 3 to 8: coding, reserved (5, 6, 7: gop); then the table of sizes
static const unsigned char CONTAINER_MAGIC[4] = {0x43, 0x53, 0x49, 0x43};   // "CSIC"

static void put_u64(unsigned char *p, uint64_t v) { put_u32(p, (uint32_t)v); put_u32(p + 4, (uint32_t)(v >> 32)); }
static uint64_t get_u64(const unsigned char *p) { return (uint64_t)get_u32(p) | ((uint64_t)get_u32(p + 4) << 32); }

static uLong crc_long(uLong crc, const unsigned char *s, int64_t n)     // zlib's length is 32 bits
{
    for (int64_t done = 0; done < n;) {
        const int64_t part = n - done < (1 << 30) ? n - done : (1 << 30);
        crc = crc32(crc, s + done, (uInt)part);
        done += part;
    }
    return crc;
}

// csic_params <-> 16 little-endian int32 in the struct's field order
static_assert(sizeof(csic_params) == 64, "csic_params is 16 int32: the container stores it field by field");
static void params_fields(const csic_params &p, int32_t f[16])
{
    const int32_t v[16] = {p.width, p.height, p.chroma_a, p.chroma_b, p.y_bits, p.cb_bits, p.cr_bits, p.factor, p.op[0], p.op[1], p.op[2],
                           p.rounding, p.sampling, p.in_format, p.out_format, p.strict_divisible};
    std::memcpy(f, v, sizeof v);
}
static csic_params params_of_fields(const int32_t f[16])
{
    csic_params p;
    p.width = f[0]; p.height = f[1]; p.chroma_a = f[2]; p.chroma_b = f[3]; p.y_bits = f[4]; p.cb_bits = f[5]; p.cr_bits = f[6];
    p.factor = f[7]; p.op[0] = f[8]; p.op[1] = f[9]; p.op[2] = f[10]; p.rounding = f[11]; p.sampling = f[12]; p.in_format = f[13];
    p.out_format = f[14]; p.strict_divisible = f[15];
    return p;
}

// the geometries of the three codings of one parameter set: the Rice coding's (with the group coding's as .pk) and the rANS coding's
struct FileGeometry : RiceGeometry {
    RansGeometry rans;
};
static int file_geometry(const csic_params *p, FileGeometry *G)
{
    const int st = rice_geometry(p, G);
    return st != CSIC_OK ? st : rans_geometry(p, &G->rans);
}

// What depends on the coding of a coded file, for one parameter set (R.pk is the group coding's geometry): a coded frame's least and
// most bytes and its bound_bytes, and the host codec.  One row per coding; a file picks its row once.
struct Codec {
    int coding;
    uint32_t version;
    uint64_t lo, hi;
    size_t bound;
    int (*check)(const FileGeometry &R, const unsigned char *c, size_t n);
    int (*pack)(const FileGeometry &R, const unsigned char *frame, unsigned char *c, size_t cap, uint64_t *n);
    int (*unpack)(const FileGeometry &R, const unsigned char *c, size_t n, unsigned char *frame);
};
static Codec codec_of(const FileGeometry &R, int coding)
{
    const csic_pack_layout &P = R.pk.layout;
    const csic_rice_layout &L = R.layout;
    const csic_rans_layout &A = R.rans.layout;
    const Codec rows[3] = {
        {CSIC_CODING_GROUPS, CONTAINER_VERSION_CODED, (uint64_t)P.fixed_bytes, (uint64_t)(P.fixed_bytes + 4 * R.pk.max_payload_dwords), (size_t)P.bound_bytes,
         [](const FileGeometry &G, const unsigned char *c, size_t n) { return pack_check_coded(G.pk, c, n); },
         [](const FileGeometry &G, const unsigned char *f, unsigned char *c, size_t cap, uint64_t *n) { return pack_frame(G.pk, f, c, cap, n); },
         [](const FileGeometry &G, const unsigned char *c, size_t n, unsigned char *f) { return unpack_frame(G.pk, c, n, f); }},
        {CSIC_CODING_RICE, CONTAINER_VERSION_RICE, (uint64_t)L.fixed_bytes, (uint64_t)(L.fixed_bytes + 4 * R.max_payload_dwords), (size_t)L.bound_bytes,
         [](const FileGeometry &G, const unsigned char *c, size_t n) { return rice_check_coded(G, c, n); },
         [](const FileGeometry &G, const unsigned char *f, unsigned char *c, size_t cap, uint64_t *n) { return rice_pack_frame(G, f, c, cap, n); },
         [](const FileGeometry &G, const unsigned char *c, size_t n, unsigned char *f) { return rice_unpack_frame(G, c, n, f); }},
        {CSIC_CODING_RANS, CONTAINER_VERSION_RANS, (uint64_t)A.fixed_bytes, (uint64_t)(A.fixed_bytes + 4 * R.rans.max_payload_dwords), (size_t)A.bound_bytes,
         [](const FileGeometry &G, const unsigned char *c, size_t n) { return rans_check_coded(G.rans, c, n); },
         [](const FileGeometry &G, const unsigned char *f, unsigned char *c, size_t cap, uint64_t *n) { return rans_pack_frame(G.rans, f, c, cap, n); },
         [](const FileGeometry &G, const unsigned char *c, size_t n, unsigned char *f) { return rans_unpack_frame(G.rans, c, n, f); }}};
    return rows[coding == CSIC_CODING_RANS ? 2 : coding == CSIC_CODING_RICE];
}

// What depends on the temporal layer of a sequence file, for one parameter set: the version, the bytes of a delta frame's map, the
// frame codec both ways, the check of a map nobody vouches for, the inter groups of one plane's section of a map, and whether the
// inverse may run in place.  One row per layer; a file picks its row once.  motion < 0: version 5 through csic_delta_*; otherwise
// version 6 through csic_mc_* at that range.  version 0: no layer (every frame stands alone).  `rows`: version 8 through csic_rows_*,
// where no frame has a previous one and every frame has a map (has_map).
struct Layer {
    uint32_t version = 0;
    int32_t motion = -1;
    int64_t map_bytes = 0;
    bool in_place = true, rows = false;
    DeltaGeometry D;               // the geometry of the file's own layer only
    McGeometry M;
    RowsGeometry W;
    bool has_map(int32_t k, int32_t gop) const { return rows || (map_bytes > 0 && gop > 0 && k % gop != 0); }
    void (*forward)(const Layer &L, const unsigned char *cur, const unsigned char *prev, unsigned char *diff, unsigned char *map) = nullptr;
    void (*inverse)(const Layer &L, const unsigned char *diff, const unsigned char *map, const unsigned char *prev, unsigned char *cur) = nullptr;
    int (*check)(const Layer &L, const unsigned char *map, bool key, int frame) = nullptr;
    uint64_t (*inter)(const Layer &L, const unsigned char *map, int pl) = nullptr;
};
static int layer_of(const csic_params &q, int32_t motion, Layer *L)
{
    L->motion = motion;
    if (motion < 0) {
        const int st = delta_geometry(&q, &L->D);
        if (st != CSIC_OK) return st;
        L->version = CONTAINER_VERSION_SEQ;
        L->map_bytes = L->D.layout.map_bytes;
        L->in_place = true;
        L->forward = [](const Layer &l, const unsigned char *c, const unsigned char *p, unsigned char *d, unsigned char *m) { delta_frame(l.D, c, p, d, m); };
        L->inverse = [](const Layer &l, const unsigned char *d, const unsigned char *m, const unsigned char *p, unsigned char *c) { undelta_frame(l.D, d, m, p, c); };
        L->check = [](const Layer &l, const unsigned char *m, bool key, int frame) { return delta_check_map(l.D, m, key, frame); };
        L->inter = [](const Layer &l, const unsigned char *m, int pl) {                 // the set bits
            uint64_t got = 0;
            for (int64_t g = 0; g < l.D.layout.groups[pl]; ++g) got += (m[l.D.layout.map_offset[pl] + (g >> 3)] >> (g & 7)) & 1;
            return got;
        };
        return CSIC_OK;
    }
    const int st = mc_geometry(&q, &L->M);
    if (st != CSIC_OK) return st;
    L->version = CONTAINER_VERSION_MC;
    L->map_bytes = L->M.layout.map_bytes;
    L->in_place = false;                              // a group reads other groups of the previous frame
    L->forward = [](const Layer &l, const unsigned char *c, const unsigned char *p, unsigned char *d, unsigned char *m) { mc_delta_frame(l.M, c, p, l.motion, d, m); };
    L->inverse = [](const Layer &l, const unsigned char *d, const unsigned char *m, const unsigned char *p, unsigned char *c) { mc_undelta_frame(l.M, d, m, p, c); };
    L->check = [](const Layer &l, const unsigned char *m, bool key, int frame) { return mc_check_map(l.M, m, key, frame); };
    L->inter = [](const Layer &l, const unsigned char *m, int pl) {                     // the nibbles that are not 0
        uint64_t got = 0;
        for (int64_t g = 0; g < l.M.layout.groups[pl]; ++g) got += nibble_at(m + l.M.layout.map_offset[pl], g) != 0;
        return got;
    };
    return CSIC_OK;
}

static int rows_layer_of(const csic_params &q, Layer *L)
{
    const int st = rows_geometry(&q, &L->W);
    if (st != CSIC_OK) return st;
    L->version = CONTAINER_VERSION_ROWS;
    L->motion = -1;
    L->map_bytes = L->W.layout.map_bytes;
    L->in_place = true;
    L->rows = true;
    L->forward = [](const Layer &l, const unsigned char *c, const unsigned char *, unsigned char *d, unsigned char *m) { rows_frame(l.W, c, d, m); };
    L->inverse = [](const Layer &l, const unsigned char *d, const unsigned char *m, const unsigned char *, unsigned char *c) { unrows_frame(l.W, d, m, c); };
    L->check = [](const Layer &l, const unsigned char *m, bool, int frame) { return rows_check_map(l.W, m, frame); };
    L->inter = [](const Layer &l, const unsigned char *m, int pl) {                     // the set bits: the groups predicted from above
        uint64_t got = 0;
        for (int64_t g = 0; g < l.W.layout.groups[pl]; ++g) got += (m[l.W.layout.map_offset[pl] + (g >> 3)] >> (g & 7)) & 1;
        return got;
    };
    return CSIC_OK;
}

struct FileCloser {
    FILE *f;
    ~FileCloser() { if (f) fclose(f); }
};

// Reads and checks everything but the CRC (and, version 3, the coded frames themselves): header fields, parameters, the table of
// sizes, the file's length.  `sizes` (may be NULL) receives the stored bytes of each frame; the file pointer is left behind the
// header (version 1) or the table (version 3).  *stored_crc may be NULL.
// What a coded file's body says in front of its table: the coding, the gop (1 below version 5) and the temporal layer (none below
// version 5: no maps, motion -1).
struct CodedBody {
    int coding = CSIC_CODING_RAW;
    int32_t gop = 1;
    Layer layer;
};

static int read_header(FILE *f, const char *path, csic_container_info *info, FileGeometry *G, uint32_t *stored_crc, std::vector<uint64_t> *sizes,
                       CodedBody *body = nullptr)
{
    CodedBody cb;
    unsigned char h[CONTAINER_HEADER];
    if (fseek(f, 0, SEEK_END) != 0) return set_error(CSIC_EIO, "cannot seek in %s", path);
    const long long size = ftello(f);
    if (size < 0 || fseek(f, 0, SEEK_SET) != 0) return set_error(CSIC_EIO, "cannot seek in %s", path);
    if ((size_t)size < CONTAINER_HEADER) return set_error(CSIC_EFORMAT, "%s: %lld bytes is shorter than a .csic header", path, size);
    if (fread(h, 1, sizeof h, f) != sizeof h) return set_error(CSIC_EIO, "cannot read %s", path);
    if (std::memcmp(h, CONTAINER_MAGIC, 4) != 0) return set_error(CSIC_EFORMAT, "%s is not a .csic file (bad magic)", path);
    const uint32_t version = get_u32(h + 4), nframes = get_u32(h + 8);
    if (version != CONTAINER_VERSION && version != CONTAINER_VERSION_CODED && version != CONTAINER_VERSION_RICE && version != CONTAINER_VERSION_SEQ &&
        version != CONTAINER_VERSION_MC && version != CONTAINER_VERSION_RANS && version != CONTAINER_VERSION_ROWS)
        return set_error(CSIC_EFORMAT, "%s: container version %u is not supported (1, 3, 4, 5, 6, 7 and 8 are)", path, version);
    if (nframes < 1 || nframes > 65535) return set_error(CSIC_EFORMAT, "%s: nframes must be in 1..65535. Got %u", path, nframes);
    int32_t fields[16];
    for (int i = 0; i < 16; ++i) fields[i] = (int32_t)get_u32(h + 16 + 4 * i);
    const csic_params p = params_of_fields(fields);
    if (p.out_format != CSIC_FMT_PLANAR_BITS || file_geometry(&p, G) != CSIC_OK)
        return set_error(CSIC_EFORMAT, "%s: the stored parameters are not a valid PLANAR_BITS parameter set", path);
    const csic_planar_bits_layout &L = G->pk.bits;
    if (version == CONTAINER_VERSION) {
        const long long want = (long long)CONTAINER_HEADER + (long long)nframes * L.payload_bytes;
        if (size != want) return set_error(CSIC_EFORMAT, "%s: %lld bytes, but %u frames of these parameters make %lld", path, size, nframes, want);
        if (sizes) sizes->assign(nframes, (uint64_t)L.payload_bytes);
    } else {
        const long long front = (long long)(CONTAINER_HEADER + CODED_BODY) + 8ll * nframes;
        if (size < front) return set_error(CSIC_EFORMAT, "%s: %lld bytes is shorter than the size table of %u frames", path, size, nframes);
        std::vector<unsigned char> t(CODED_BODY + 8 * (size_t)nframes);
        if (fread(t.data(), 1, t.size(), f) != t.size()) return set_error(CSIC_EIO, "cannot read %s", path);
        int coding = version == CONTAINER_VERSION_RICE ? CSIC_CODING_RICE : CSIC_CODING_GROUPS;
        if (version == CONTAINER_VERSION_ROWS) {                   // coding | 1 << 16, every other bit zero; then a zero word
            const uint32_t c = get_u32(t.data()), id = c & ~ROWS_FLAG;
            if (!(c & ROWS_FLAG) || (id != CSIC_CODING_GROUPS && id != CSIC_CODING_RICE && id != CSIC_CODING_RANS) || get_u32(t.data() + 4) != 0)
                return set_error(CSIC_EFORMAT, "%s: coding word %#x (then %u) is not what version %u holds (1, 3 or 5 with bit 16 set, then 0)", path, c,
                                 get_u32(t.data() + 4), version);
            coding = (int)id;
            const int st = rows_layer_of(p, &cb.layer);
            if (st != CSIC_OK) return set_error(CSIC_EFORMAT, "%s: the stored parameters have no layout in the row-prediction layer", path);
        } else if (version == CONTAINER_VERSION_RANS) {                   // 5 | (range + 1) << 8 with a field of 0 for no motion layer; gop 0: no layer at all
            const uint32_t c = get_u32(t.data()), field = c >> 8, gop = get_u32(t.data() + 4);
            if ((c & 0xFFu) != CSIC_CODING_RANS) return set_error(CSIC_EFORMAT, "%s: coding %u is not the one version %u holds (5)", path, c & 0xFFu, version);
            if (field > (uint32_t)MC_MAX_RANGE + 1 || gop > 65535 || (gop == 0 && field != 0))
                return set_error(CSIC_EFORMAT, "%s: motion field %u and gop %u of a version-%u file: the field is a range + 1 of 1..%d or 0, the gop at most 65535, and a range needs a gop",
                                 path, field, gop, version, MC_MAX_RANGE + 1);
            coding = CSIC_CODING_RANS;
            if (gop > 0) {
                cb.gop = (int32_t)gop;
                const int st = layer_of(p, (int32_t)field - 1, &cb.layer);
                if (st != CSIC_OK) return set_error(CSIC_EFORMAT, "%s: the stored parameters have no layout in the file's temporal layer", path);
            }
        } else if (version == CONTAINER_VERSION_SEQ || version == CONTAINER_VERSION_MC) {
            uint32_t c = get_u32(t.data());
            const uint32_t gop = get_u32(t.data() + 4);
            int32_t motion = -1;
            if (version == CONTAINER_VERSION_MC) {                 // coding | (range + 1) << 8, every other bit zero
                const uint32_t field = c >> 8;
                if (field < 1 || field > (uint32_t)MC_MAX_RANGE + 1)
                    return set_error(CSIC_EFORMAT, "%s: motion field %u of the coding word %#x is not a range + 1 of 1..%d", path, field, c, MC_MAX_RANGE + 1);
                motion = (int32_t)field - 1;
                c &= 0xFFu;
            }
            if (c != CSIC_CODING_GROUPS && c != CSIC_CODING_RICE) return set_error(CSIC_EFORMAT, "%s: coding %u is not one version %u holds (1 or 3)", path, c, version);
            if (gop < 1 || gop > 65535) return set_error(CSIC_EFORMAT, "%s: gop must be in 1..65535. Got %u", path, gop);
            coding = (int)c;
            cb.gop = (int32_t)gop;
            const int st = layer_of(p, motion, &cb.layer);
            if (st != CSIC_OK) return motion < 0 ? st : set_error(CSIC_EFORMAT, "%s: the stored parameters have no motion-compensated layout", path);
        } else if (get_u32(t.data()) != (uint32_t)coding || get_u32(t.data() + 4) != 0)
            return set_error(CSIC_EFORMAT, "%s: coding %u (reserved word %u) is not what version %u holds (%d, 0)", path, get_u32(t.data()), get_u32(t.data() + 4),
                             version, coding);
        cb.coding = coding;
        const Codec codec = codec_of(*G, coding);
        long long want = front;
        if (sizes) sizes->resize(nframes);
        for (uint32_t k = 0; k < nframes; ++k) {
            const uint64_t sz = get_u64(t.data() + CODED_BODY + 8 * (size_t)k);
            const uint64_t map = cb.layer.has_map((int32_t)k, cb.gop) ? (uint64_t)cb.layer.map_bytes : 0, lo = codec.lo + map, hi = codec.hi + map;     // a delta record: map, then coded frame
            if (sz < lo || sz > hi || sz % 4 != 0)
                return set_error(CSIC_EFORMAT, "%s: frame %u is stored in %llu bytes; these parameters code to %llu .. %llu, in dwords", path, k,
                                 (unsigned long long)sz, (unsigned long long)lo, (unsigned long long)hi);
            want += (long long)sz;
            if (sizes) (*sizes)[k] = sz;
        }
        if (size != want) return set_error(CSIC_EFORMAT, "%s: %lld bytes, but the header and the frames' sizes make %lld", path, size, want);
    }
    info->params = p;
    info->version = (int32_t)version;
    info->nframes = (int32_t)nframes;
    info->payload_bytes = L.payload_bytes;
    info->file_bytes = size;
    if (stored_crc) *stored_crc = get_u32(h + 12);
    if (body) *body = cb;
    return CSIC_OK;
}

static void fill_header(unsigned char h[CONTAINER_HEADER], uint32_t version, const csic_params &q, int32_t nframes)
{
    std::memcpy(h, CONTAINER_MAGIC, 4);
    put_u32(h + 4, version);
    put_u32(h + 8, (uint32_t)nframes);
    put_u32(h + 12, 0);
    int32_t fields[16];
    params_fields(q, fields);
    for (int i = 0; i < 16; ++i) put_u32(h + 16 + 4 * i, (uint32_t)fields[i]);
}

// the parameters a file stores, and their geometry; nframes checked
static int writer_params(const csic_params *p, int32_t nframes, csic_params *q, FileGeometry *G)
{
    *q = *p;
    q->out_format = CSIC_FMT_PLANAR_BITS;
    const int st = file_geometry(q, G);           // csic_validate first: refuses in_format != ARGB for PLANAR_BITS
    if (st != CSIC_OK) return st;
    if (nframes < 1 || nframes > 65535) return set_error(CSIC_EINVAL_SIZE, "nframes must be in 1..65535. Got %d", nframes);
    return CSIC_OK;
}

// A version-3 or version-4 file from coded frames in memory: frame k is frames[k][0, sizes[k]).  With a gop (> 0) a version-5 file:
// maps[k][0, map_bytes) of the layer stands in front of every delta frame, and the version is the layer's.
static int write_coded_file(const char *path, const csic_params &q, const unsigned char *const *frames, const uint64_t *sizes, int32_t nframes, const Codec &codec,
                            int32_t gop = 0, const unsigned char *const *maps = nullptr, const Layer &layer = Layer())
{
    const size_t map_bytes = (size_t)layer.map_bytes;
    const auto map_of = [&](int32_t k) { return layer.has_map(k, gop) ? map_bytes : (size_t)0; };
    unsigned char h[CONTAINER_HEADER];
    fill_header(h, layer.rows || (gop > 0 && codec.coding != CSIC_CODING_RANS) ? layer.version : codec.version, q, nframes);   // (version 7: with or without a layer)
    std::vector<unsigned char> t(CODED_BODY + 8 * (size_t)nframes);
    put_u32(t.data(), (uint32_t)codec.coding | (uint32_t)(layer.motion + 1) << 8 | (layer.rows ? ROWS_FLAG : 0u));
    put_u32(t.data() + 4, (uint32_t)gop);
    for (int32_t k = 0; k < nframes; ++k) put_u64(t.data() + CODED_BODY + 8 * (size_t)k, sizes[k] + map_of(k));
    uLong crc = crc32(0L, h + CONTAINER_CRC_FROM, (uInt)(CONTAINER_HEADER - CONTAINER_CRC_FROM));
    crc = crc_long(crc, t.data(), (int64_t)t.size());
    for (int32_t k = 0; k < nframes; ++k) {
        if (map_of(k)) crc = crc_long(crc, maps[k], (int64_t)map_bytes);
        crc = crc_long(crc, frames[k], (int64_t)sizes[k]);
    }
    put_u32(h + 12, (uint32_t)crc);

    FileCloser fc{fopen(path, "wb")};
    if (!fc.f) return set_error(CSIC_EIO, "cannot open %s for writing", path);
    bool ok = fwrite(h, 1, sizeof h, fc.f) == sizeof h && fwrite(t.data(), 1, t.size(), fc.f) == t.size();
    for (int32_t k = 0; ok && k < nframes; ++k)
        ok = (!map_of(k) || fwrite(maps[k], 1, map_bytes, fc.f) == map_bytes) && fwrite(frames[k], 1, (size_t)sizes[k], fc.f) == (size_t)sizes[k];
    FILE *f = fc.f;
    fc.f = nullptr;
    if (fclose(f) != 0) ok = false;
    if (!ok) return set_error(CSIC_EIO, "cannot write %s", path);
    return CSIC_OK;
}

// What the readers of one thing of a file share: the NULLs, the file opened, its header read and checked, then
// take(file, info, table of sizes, body) with an allocation failure caught; the error state is cleared on success.
template <class Take> static int with_header(const char *path, const void *out, Take take)
{
    if (!path || !out) return set_error(CSIC_EINVAL_NULL, "argument is NULL");
    FileCloser fc{fopen(path, "rb")};
    if (!fc.f) return set_error(CSIC_EIO, "cannot open %s", path);
    try {
        FileGeometry G;
        csic_container_info ci;
        std::vector<uint64_t> table;
        CodedBody body;
        int st = read_header(fc.f, path, &ci, &G, nullptr, &table, &body);
        if (st == CSIC_OK) st = take(fc.f, ci, table, body);
        if (st != CSIC_OK) return st;
    } catch (const std::bad_alloc &) {
        return set_error(CSIC_ENOMEM, "out of host memory reading %s", path);
    }
    clear_error();
    return CSIC_OK;
}

} // namespace csic

using namespace csic;

extern "C" {

int csic_container_info_of(const char *path, csic_container_info *info)
{
    return with_header(path, info, [&](FILE *, const csic_container_info &ci, const std::vector<uint64_t> &, const CodedBody &) { *info = ci; return (int)CSIC_OK; });
}

int csic_container_coded_sizes(const char *path, uint64_t *sizes, int32_t n)
{
    return with_header(path, sizes, [&](FILE *, const csic_container_info &ci, const std::vector<uint64_t> &table, const CodedBody &) {
        if (n != ci.nframes) return set_error(CSIC_EINVAL_SIZE, "expected room for %d sizes, got %d", ci.nframes, n);
        std::memcpy(sizes, table.data(), table.size() * sizeof(uint64_t));
        return (int)CSIC_OK;
    });
}

int csic_container_write(const char *path, const csic_params *p, const void *frames, int32_t nframes)
{
    if (!path || !p || !frames) return set_error(CSIC_EINVAL_NULL, "argument is NULL");
    csic_params q;
    FileGeometry C;
    const int st = writer_params(p, nframes, &q, &C);
    if (st != CSIC_OK) return st;
    const PackGeometry &G = C.pk;
    const csic_planar_bits_layout &L = G.bits;

    unsigned char h[CONTAINER_HEADER];
    fill_header(h, CONTAINER_VERSION, q, nframes);
    const unsigned char *base = static_cast<const unsigned char *>(frames);
    uLong crc = crc32(0L, h + CONTAINER_CRC_FROM, (uInt)(CONTAINER_HEADER - CONTAINER_CRC_FROM));
    for (int32_t k = 0; k < nframes; ++k)
        for (int pl = 0; pl < 3; ++pl) crc = crc_long(crc, base + (int64_t)k * L.frame_bytes + G.src_offset[pl], G.src_bytes[pl]);
    put_u32(h + 12, (uint32_t)crc);

    FileCloser fc{fopen(path, "wb")};
    if (!fc.f) return set_error(CSIC_EIO, "cannot open %s for writing", path);
    bool ok = fwrite(h, 1, sizeof h, fc.f) == sizeof h;
    for (int32_t k = 0; ok && k < nframes; ++k)
        for (int pl = 0; ok && pl < 3; ++pl)
            ok = fwrite(base + (int64_t)k * L.frame_bytes + G.src_offset[pl], 1, (size_t)G.src_bytes[pl], fc.f) == (size_t)G.src_bytes[pl];
    FILE *f = fc.f;
    fc.f = nullptr;
    if (fclose(f) != 0) ok = false;
    if (!ok) return set_error(CSIC_EIO, "cannot write %s", path);
    clear_error();
    return CSIC_OK;
}

int csic_container_write_ex(const char *path, const csic_params *p, const void *frames, int32_t nframes, int32_t coding)
{
    if (coding == CSIC_CODING_RAW) return csic_container_write(path, p, frames, nframes);
    if (!path || !p || !frames) return set_error(CSIC_EINVAL_NULL, "argument is NULL");
    if (coding != CSIC_CODING_GROUPS && coding != CSIC_CODING_RICE && coding != CSIC_CODING_RANS)
        return set_error(CSIC_EINVAL_FORMAT, "coding must be CSIC_CODING_RAW(0), CSIC_CODING_GROUPS(1), CSIC_CODING_RICE(3) or CSIC_CODING_RANS(5). Got %d", coding);
    csic_params q;
    FileGeometry G;
    int st = writer_params(p, nframes, &q, &G);
    if (st != CSIC_OK) return st;
    const Codec codec = codec_of(G, coding);
    try {
        // the table of sizes stands in front of the frames: every frame is coded before the first byte is written
        std::vector<unsigned char> all;
        std::vector<uint64_t> sizes((size_t)nframes);
        for (int32_t k = 0; k < nframes; ++k) {
            const size_t at = all.size();
            all.resize(at + codec.bound);
            st = codec.pack(G, static_cast<const unsigned char *>(frames) + (int64_t)k * G.pk.bits.frame_bytes, all.data() + at, codec.bound, &sizes[k]);
            if (st != CSIC_OK) return st;
            all.resize(at + (size_t)sizes[k]);
        }
        std::vector<const unsigned char *> ptrs((size_t)nframes);
        size_t at = 0;
        for (int32_t k = 0; k < nframes; ++k) { ptrs[k] = all.data() + at; at += (size_t)sizes[k]; }
        st = write_coded_file(path, q, ptrs.data(), sizes.data(), nframes, codec);
    } catch (const std::bad_alloc &) {
        return set_error(CSIC_ENOMEM, "out of host memory coding %d frames for %s", nframes, path);
    }
    if (st != CSIC_OK) return st;
    clear_error();
    return CSIC_OK;
}

int csic_container_write_coded_ex(const char *path, const csic_params *p, const void *coded, size_t stride_bytes, const uint64_t *sizes,
                                  int32_t nframes, int32_t coding)
{
    if (!path || !p || !coded || !sizes) return set_error(CSIC_EINVAL_NULL, "argument is NULL");
    if (coding != CSIC_CODING_GROUPS && coding != CSIC_CODING_RICE && coding != CSIC_CODING_RANS)
        return set_error(CSIC_EINVAL_FORMAT, "coded frames are CSIC_CODING_GROUPS(1), CSIC_CODING_RICE(3) or CSIC_CODING_RANS(5). Got %d", coding);
    csic_params q;
    FileGeometry G;
    int st = writer_params(p, nframes, &q, &G);
    if (st != CSIC_OK) return st;
    const Codec codec = codec_of(G, coding);
    try {
        std::vector<const unsigned char *> ptrs((size_t)nframes);
        for (int32_t k = 0; k < nframes; ++k) {
            if (sizes[k] > stride_bytes)
                return set_error(CSIC_EINVAL_SIZE, "frame %d: %llu coded bytes do not fit the stride of %zu", k, (unsigned long long)sizes[k], stride_bytes);
            ptrs[k] = static_cast<const unsigned char *>(coded) + (size_t)k * stride_bytes;
            st = codec.check(G, ptrs[k], (size_t)sizes[k]);
            if (st != CSIC_OK) return st;
        }
        st = write_coded_file(path, q, ptrs.data(), sizes, nframes, codec);
    } catch (const std::bad_alloc &) {
        return set_error(CSIC_ENOMEM, "out of host memory writing %s", path);
    }
    if (st != CSIC_OK) return st;
    clear_error();
    return CSIC_OK;
}

int csic_container_write_coded(const char *path, const csic_params *p, const void *coded, size_t stride_bytes, const uint64_t *sizes,
                               int32_t nframes)
{
    return csic_container_write_coded_ex(path, p, coded, stride_bytes, sizes, nframes, CSIC_CODING_GROUPS);
}

// csic_container_write_seq and csic_container_write_coded_seq: what they refuse of coding and gop
static int seq_check(int32_t coding, int32_t gop)
{
    if (coding != CSIC_CODING_GROUPS && coding != CSIC_CODING_RICE && coding != CSIC_CODING_RANS)
        return set_error(CSIC_EINVAL_FORMAT, "a sequence is coded with CSIC_CODING_GROUPS(1), CSIC_CODING_RICE(3) or CSIC_CODING_RANS(5). Got %d", coding);
    if (gop < 1 || gop > 65535) return set_error(CSIC_EINVAL_SIZE, "gop must be in 1..65535. Got %d", gop);
    return CSIC_OK;
}

constexpr int32_t MOTION_ROWS = -2;                // write_seq, write_coded_seq: not a temporal layer but csic_rows_*, version 8 (gop 0)
static int writer_layer(const csic_params &q, int32_t motion, Layer *L) { return motion == MOTION_ROWS ? rows_layer_of(q, L) : layer_of(q, motion, L); }
// seq_check for the row-prediction layer: the coding alone
static int rows_check(int32_t coding)
{
    if (coding != CSIC_CODING_GROUPS && coding != CSIC_CODING_RICE && coding != CSIC_CODING_RANS)
        return set_error(CSIC_EINVAL_FORMAT, "the row-prediction layer sits in front of CSIC_CODING_GROUPS(1), CSIC_CODING_RICE(3) or CSIC_CODING_RANS(5). Got %d", coding);
    return CSIC_OK;
}

// motion < 0: version 5 through csic_delta_*; otherwise version 6 through csic_mc_* at that range
static int write_seq(const char *path, const csic_params *p, const void *frames, int32_t nframes, int32_t coding, int32_t gop, int32_t motion)
{
    if (!path || !p || !frames) return set_error(CSIC_EINVAL_NULL, "argument is NULL");
    int st = motion == MOTION_ROWS ? rows_check(coding) : seq_check(coding, gop);
    if (st != CSIC_OK) return st;
    csic_params q;
    FileGeometry G;
    Layer layer;
    if ((st = writer_params(p, nframes, &q, &G)) != CSIC_OK || (st = writer_layer(q, motion, &layer)) != CSIC_OK) return st;
    const Codec codec = codec_of(G, coding);
    try {
        const size_t fb = (size_t)G.pk.bits.frame_bytes, mb = (size_t)layer.map_bytes;
        const unsigned char *x = static_cast<const unsigned char *>(frames);
        std::vector<unsigned char> diff(fb), maps((size_t)nframes * mb), all;
        std::vector<uint64_t> sizes((size_t)nframes);
        for (int32_t k = 0; k < nframes; ++k) {
            layer.forward(layer, x + (size_t)k * fb, gop > 0 && k % gop ? x + (size_t)(k - 1) * fb : nullptr, diff.data(), maps.data() + (size_t)k * mb);
            const size_t at = all.size();
            all.resize(at + codec.bound);
            st = codec.pack(G, diff.data(), all.data() + at, codec.bound, &sizes[k]);
            if (st != CSIC_OK) return st;
            all.resize(at + (size_t)sizes[k]);
        }
        std::vector<const unsigned char *> ptrs((size_t)nframes), mptrs((size_t)nframes);
        size_t at = 0;
        for (int32_t k = 0; k < nframes; ++k) { ptrs[k] = all.data() + at; at += (size_t)sizes[k]; mptrs[k] = maps.data() + (size_t)k * mb; }
        st = write_coded_file(path, q, ptrs.data(), sizes.data(), nframes, codec, gop, mptrs.data(), layer);
    } catch (const std::bad_alloc &) {
        return set_error(CSIC_ENOMEM, "out of host memory coding %d frames for %s", nframes, path);
    }
    if (st != CSIC_OK) return st;
    clear_error();
    return CSIC_OK;
}

int csic_container_write_seq(const char *path, const csic_params *p, const void *frames, int32_t nframes, int32_t coding, int32_t gop)
{
    return write_seq(path, p, frames, nframes, coding, gop, -1);
}

int csic_container_write_seq_ex(const char *path, const csic_params *p, const void *frames, int32_t nframes, int32_t coding, int32_t gop, int32_t range)
{
    const int st = mc_check_range(range);
    return st != CSIC_OK ? st : write_seq(path, p, frames, nframes, coding, gop, range);
}

static int write_coded_seq(const char *path, const csic_params *p, const void *coded, size_t stride_bytes, const uint64_t *sizes,
                           const void *maps, size_t map_stride, int32_t nframes, int32_t coding, int32_t gop, int32_t motion)
{
    if (!path || !p || !coded || !sizes || !maps) return set_error(CSIC_EINVAL_NULL, "argument is NULL");
    int st = motion == MOTION_ROWS ? rows_check(coding) : seq_check(coding, gop);
    if (st != CSIC_OK) return st;
    csic_params q;
    FileGeometry G;
    Layer layer;
    if ((st = writer_params(p, nframes, &q, &G)) != CSIC_OK || (st = writer_layer(q, motion, &layer)) != CSIC_OK) return st;
    const size_t mb = (size_t)layer.map_bytes;
    if (map_stride < mb)
        return set_error(CSIC_EINVAL_SIZE, "a map of these parameters has %zu bytes: a map_stride of %zu cannot hold it", mb, map_stride);
    const Codec codec = codec_of(G, coding);
    try {
        std::vector<const unsigned char *> ptrs((size_t)nframes), mptrs((size_t)nframes);
        for (int32_t k = 0; k < nframes; ++k) {
            if (sizes[k] > stride_bytes)
                return set_error(CSIC_EINVAL_SIZE, "frame %d: %llu coded bytes do not fit the stride of %zu", k, (unsigned long long)sizes[k], stride_bytes);
            ptrs[k] = static_cast<const unsigned char *>(coded) + (size_t)k * stride_bytes;
            mptrs[k] = static_cast<const unsigned char *>(maps) + (size_t)k * map_stride;
            if ((st = codec.check(G, ptrs[k], (size_t)sizes[k])) != CSIC_OK) return st;
            if ((st = layer.check(layer, mptrs[k], gop > 0 && k % gop == 0, k)) != CSIC_OK) return st;
        }
        st = write_coded_file(path, q, ptrs.data(), sizes, nframes, codec, gop, mptrs.data(), layer);
    } catch (const std::bad_alloc &) {
        return set_error(CSIC_ENOMEM, "out of host memory writing %s", path);
    }
    if (st != CSIC_OK) return st;
    clear_error();
    return CSIC_OK;
}

int csic_container_write_coded_seq(const char *path, const csic_params *p, const void *coded, size_t stride_bytes, const uint64_t *sizes,
                                   const void *maps, size_t map_stride, int32_t nframes, int32_t coding, int32_t gop)
{
    return write_coded_seq(path, p, coded, stride_bytes, sizes, maps, map_stride, nframes, coding, gop, -1);
}

int csic_container_write_coded_seq_ex(const char *path, const csic_params *p, const void *coded, size_t stride_bytes, const uint64_t *sizes,
                                      const void *maps, size_t map_stride, int32_t nframes, int32_t coding, int32_t gop, int32_t range)
{
    const int st = mc_check_range(range);
    return st != CSIC_OK ? st : write_coded_seq(path, p, coded, stride_bytes, sizes, maps, map_stride, nframes, coding, gop, range);
}

int csic_container_write_rows(const char *path, const csic_params *p, const void *frames, int32_t nframes, int32_t coding)
{
    return write_seq(path, p, frames, nframes, coding, 0, MOTION_ROWS);
}

int csic_container_write_coded_rows(const char *path, const csic_params *p, const void *coded, size_t stride_bytes, const uint64_t *sizes,
                                    const void *maps, size_t map_stride, int32_t nframes, int32_t coding)
{
    return write_coded_seq(path, p, coded, stride_bytes, sizes, maps, map_stride, nframes, coding, 0, MOTION_ROWS);
}

int csic_container_rows(const char *path, int32_t *flag)
{
    return with_header(path, flag, [&](FILE *, const csic_container_info &, const std::vector<uint64_t> &, const CodedBody &body) { *flag = body.layer.rows ? 1 : 0; return (int)CSIC_OK; });
}

int csic_container_motion(const char *path, int32_t *range)
{
    return with_header(path, range, [&](FILE *, const csic_container_info &, const std::vector<uint64_t> &, const CodedBody &body) { *range = body.layer.motion; return (int)CSIC_OK; });
}

int csic_container_gop(const char *path, int32_t *gop)
{
    return with_header(path, gop, [&](FILE *, const csic_container_info &, const std::vector<uint64_t> &, const CodedBody &body) { *gop = body.gop; return (int)CSIC_OK; });
}

int csic_container_inter_groups(const char *path, uint64_t *counts, int32_t n)
{
    return with_header(path, counts, [&](FILE *f, const csic_container_info &ci, const std::vector<uint64_t> &table, const CodedBody &body) {
        if (n != 3 * ci.nframes) return set_error(CSIC_EINVAL_SIZE, "expected room for %d counts, got %d", 3 * ci.nframes, n);
        const Layer &layer = body.layer;
        std::vector<uint64_t> got((size_t)n, 0);
        std::vector<unsigned char> map((size_t)layer.map_bytes);
        long long at = ftello(f);                      // where the records begin
        for (int32_t k = 0; k < ci.nframes; at += (long long)table[k], ++k) {
            if (!layer.has_map(k, body.gop)) continue;
            if (fseeko(f, at, SEEK_SET) != 0 || fread(map.data(), 1, map.size(), f) != map.size()) return set_error(CSIC_EIO, "cannot read %s", path);
            const int st = layer.check(layer, map.data(), false, k);
            if (st != CSIC_OK) return st;
            for (int pl = 0; pl < 3; ++pl) got[3 * (size_t)k + pl] = layer.inter(layer, map.data(), pl);
        }
        std::memcpy(counts, got.data(), got.size() * sizeof(uint64_t));
        return (int)CSIC_OK;
    });
}

static int container_read(const char *path, void *frames, size_t frames_bytes)
{
    FileCloser fc{fopen(path, "rb")};
    if (!fc.f) return set_error(CSIC_EIO, "cannot open %s", path);
    FileGeometry C;
    csic_container_info ci;
    uint32_t stored = 0;
    std::vector<uint64_t> sizes;
    CodedBody body;
    int st = read_header(fc.f, path, &ci, &C, &stored, &sizes, &body);
    if (st != CSIC_OK) return st;
    const PackGeometry &G = C.pk;
    const Layer &layer = body.layer;
    const csic_planar_bits_layout &L = G.bits;
    const size_t need = (size_t)ci.nframes * (size_t)L.frame_bytes;
    if (frames_bytes != need)
        return set_error(CSIC_EINVAL_SIZE, "expected room for %zu bytes (%d frames of %lld), got %zu", need, ci.nframes, (long long)L.frame_bytes,
                         frames_bytes);
    // bytes [16, here) of the file take part in the CRC; the file pointer stands where the frames begin
    const long long front = ftello(fc.f);
    if (front < (long long)CONTAINER_HEADER) return set_error(CSIC_EIO, "cannot read %s", path);
    std::vector<unsigned char> h((size_t)front);
    if (fseek(fc.f, 0, SEEK_SET) != 0 || fread(h.data(), 1, h.size(), fc.f) != h.size()) return set_error(CSIC_EIO, "cannot read %s", path);
    uLong crc = crc_long(0L, h.data() + CONTAINER_CRC_FROM, (int64_t)(h.size() - CONTAINER_CRC_FROM));
    unsigned char *base = static_cast<unsigned char *>(frames);
    std::memset(base, 0, need);
    std::vector<unsigned char> coded, diff;
    const Codec codec = codec_of(C, body.coding);     // (unused by version 1)
    for (int32_t k = 0; k < ci.nframes && st == CSIC_OK; ++k) {
        unsigned char *fr = base + (int64_t)k * L.frame_bytes;
        if (ci.version == (int32_t)CONTAINER_VERSION) {
            for (int pl = 0; pl < 3; ++pl) {
                unsigned char *d = fr + G.src_offset[pl];
                if (fread(d, 1, (size_t)G.src_bytes[pl], fc.f) != (size_t)G.src_bytes[pl]) return set_error(CSIC_EIO, "cannot read %s", path);
                crc = crc_long(crc, d, G.src_bytes[pl]);
            }
        } else {
            coded.resize((size_t)sizes[k]);            // within the coding's sizes: read_header checked the table
            if (fread(coded.data(), 1, coded.size(), fc.f) != coded.size()) return set_error(CSIC_EIO, "cannot read %s", path);
            crc = crc_long(crc, coded.data(), (int64_t)coded.size());
            const size_t map = layer.has_map(k, body.gop) ? (size_t)layer.map_bytes : 0;     // versions 5 to 8: the map first (read_header: the record holds it)
            unsigned char *d = fr;                         // the difference frame -> the frame, in place where the layer allows it
            if (map && !layer.in_place) {
                diff.assign((size_t)L.frame_bytes, 0);
                d = diff.data();
            }
            if (map) st = layer.check(layer, coded.data(), false, k);
            if (st == CSIC_OK) st = codec.unpack(C, coded.data() + map, coded.size() - map, d);
            if (st == CSIC_OK && map) layer.inverse(layer, d, coded.data(), layer.rows ? nullptr : fr - L.frame_bytes, fr);
        }
    }
    if (st == CSIC_OK && (uint32_t)crc != stored)
        st = set_error(CSIC_EFORMAT, "%s: CRC mismatch (stored %08x, computed %08x)", path, stored, (uint32_t)crc);
    if (st != CSIC_OK) {
        std::memset(base, 0, need);
        return st;
    }
    return CSIC_OK;
}

int csic_container_read(const char *path, void *frames, size_t frames_bytes)
{
    if (!path || !frames) return set_error(CSIC_EINVAL_NULL, "argument is NULL");
    int st;
    try {
        st = container_read(path, frames, frames_bytes);
    } catch (const std::bad_alloc &) {
        return set_error(CSIC_ENOMEM, "out of host memory reading %s", path);
    }
    if (st != CSIC_OK) return st;
    clear_error();
    return CSIC_OK;
}

} // extern "C"
