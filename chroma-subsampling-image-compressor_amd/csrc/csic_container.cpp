// csic_container.cpp -- .csic files: CSIC_FMT_PLANAR_BITS frames on disk (host only, no device; byte layout in include/csic.h).
// A file is an 80-byte header -- magic, version, frame count, CRC-32 of everything behind the CRC field, the parameters -- and per
// frame the three planes' payload bytes back to back: the padding of a frame buffer never reaches the file, and reading zeroes it.
#include <zlib.h>

#include <cstdio>
#include <cstring>

#include "csic_internal.h"

namespace csic {

constexpr size_t CONTAINER_HEADER = 80, CONTAINER_CRC_FROM = 16;
constexpr uint32_t CONTAINER_VERSION = 1;
static const unsigned char CONTAINER_MAGIC[4] = {0x43, 0x53, 0x49, 0x43};   // "CSIC"

static void put_u32(unsigned char *p, uint32_t v) { p[0] = (unsigned char)v; p[1] = (unsigned char)(v >> 8); p[2] = (unsigned char)(v >> 16); p[3] = (unsigned char)(v >> 24); }
static uint32_t get_u32(const unsigned char *p) { return (uint32_t)p[0] | ((uint32_t)p[1] << 8) | ((uint32_t)p[2] << 16) | ((uint32_t)p[3] << 24); }

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

struct FileCloser {
    FILE *f;
    ~FileCloser() { if (f) fclose(f); }
};

// Reads and checks everything but the CRC: header fields, parameters, the file's length.  *stored_crc may be NULL.
static int read_header(FILE *f, const char *path, csic_container_info *info, csic_planar_bits_layout *L, uint32_t *stored_crc)
{
    unsigned char h[CONTAINER_HEADER];
    if (fseek(f, 0, SEEK_END) != 0) return set_error(CSIC_EIO, "cannot seek in %s", path);
    const long long size = ftello(f);
    if (size < 0 || fseek(f, 0, SEEK_SET) != 0) return set_error(CSIC_EIO, "cannot seek in %s", path);
    if ((size_t)size < CONTAINER_HEADER) return set_error(CSIC_EFORMAT, "%s: %lld bytes is shorter than a .csic header", path, size);
    if (fread(h, 1, sizeof h, f) != sizeof h) return set_error(CSIC_EIO, "cannot read %s", path);
    if (std::memcmp(h, CONTAINER_MAGIC, 4) != 0) return set_error(CSIC_EFORMAT, "%s is not a .csic file (bad magic)", path);
    const uint32_t version = get_u32(h + 4), nframes = get_u32(h + 8);
    if (version != CONTAINER_VERSION) return set_error(CSIC_EFORMAT, "%s: container version %u is not supported (1 is)", path, version);
    if (nframes < 1 || nframes > 65535) return set_error(CSIC_EFORMAT, "%s: nframes must be in 1..65535. Got %u", path, nframes);
    int32_t fields[16];
    for (int i = 0; i < 16; ++i) fields[i] = (int32_t)get_u32(h + 16 + 4 * i);
    const csic_params p = params_of_fields(fields);
    if (p.out_format != CSIC_FMT_PLANAR_BITS || csic_validate(&p) != CSIC_OK || csic_planar_bits_layout_of(&p, L) != CSIC_OK)
        return set_error(CSIC_EFORMAT, "%s: the stored parameters are not a valid PLANAR_BITS parameter set", path);
    const long long want = (long long)CONTAINER_HEADER + (long long)nframes * L->payload_bytes;
    if (size != want) return set_error(CSIC_EFORMAT, "%s: %lld bytes, but %u frames of these parameters make %lld", path, size, nframes, want);
    info->params = p;
    info->version = (int32_t)version;
    info->nframes = (int32_t)nframes;
    info->payload_bytes = L->payload_bytes;
    info->file_bytes = size;
    if (stored_crc) *stored_crc = get_u32(h + 12);
    return CSIC_OK;
}

} // namespace csic

using namespace csic;

extern "C" {

int csic_container_info_of(const char *path, csic_container_info *info)
{
    if (!path || !info) return set_error(CSIC_EINVAL_NULL, "argument is NULL");
    FileCloser fc{fopen(path, "rb")};
    if (!fc.f) return set_error(CSIC_EIO, "cannot open %s", path);
    csic_planar_bits_layout L;
    csic_container_info ci;
    const int st = read_header(fc.f, path, &ci, &L, nullptr);
    if (st != CSIC_OK) return st;
    *info = ci;
    clear_error();
    return CSIC_OK;
}

int csic_container_write(const char *path, const csic_params *p, const void *frames, int32_t nframes)
{
    if (!path || !p || !frames) return set_error(CSIC_EINVAL_NULL, "argument is NULL");
    csic_params q = *p;
    q.out_format = CSIC_FMT_PLANAR_BITS;
    int st = csic_validate(&q);                       // refuses in_format != ARGB for PLANAR_BITS
    if (st != CSIC_OK) return st;
    if (nframes < 1 || nframes > 65535) return set_error(CSIC_EINVAL_SIZE, "nframes must be in 1..65535. Got %d", nframes);
    csic_planar_bits_layout L;
    st = csic_planar_bits_layout_of(&q, &L);
    if (st != CSIC_OK) return st;

    unsigned char h[CONTAINER_HEADER];
    std::memcpy(h, CONTAINER_MAGIC, 4);
    put_u32(h + 4, CONTAINER_VERSION);
    put_u32(h + 8, (uint32_t)nframes);
    int32_t fields[16];
    params_fields(q, fields);
    for (int i = 0; i < 16; ++i) put_u32(h + 16 + 4 * i, (uint32_t)fields[i]);
    const int64_t plane_off[3] = {L.y_offset, L.cb_offset, L.cr_offset}, plane_bytes[3] = {L.y_bytes, L.cb_bytes, L.cr_bytes};
    const unsigned char *base = static_cast<const unsigned char *>(frames);
    uLong crc = crc32(0L, h + CONTAINER_CRC_FROM, (uInt)(CONTAINER_HEADER - CONTAINER_CRC_FROM));
    for (int32_t k = 0; k < nframes; ++k)
        for (int pl = 0; pl < 3; ++pl) {
            const unsigned char *s = base + (int64_t)k * L.frame_bytes + plane_off[pl];
            for (int64_t done = 0; done < plane_bytes[pl];) {              // zlib's length is 32 bits
                const int64_t part = plane_bytes[pl] - done < (1 << 30) ? plane_bytes[pl] - done : (1 << 30);
                crc = crc32(crc, s + done, (uInt)part);
                done += part;
            }
        }
    put_u32(h + 12, (uint32_t)crc);

    FileCloser fc{fopen(path, "wb")};
    if (!fc.f) return set_error(CSIC_EIO, "cannot open %s for writing", path);
    bool ok = fwrite(h, 1, sizeof h, fc.f) == sizeof h;
    for (int32_t k = 0; ok && k < nframes; ++k)
        for (int pl = 0; ok && pl < 3; ++pl)
            ok = fwrite(base + (int64_t)k * L.frame_bytes + plane_off[pl], 1, (size_t)plane_bytes[pl], fc.f) == (size_t)plane_bytes[pl];
    FILE *f = fc.f;
    fc.f = nullptr;
    if (fclose(f) != 0) ok = false;
    if (!ok) return set_error(CSIC_EIO, "cannot write %s", path);
    clear_error();
    return CSIC_OK;
}

int csic_container_read(const char *path, void *frames, size_t frames_bytes)
{
    if (!path || !frames) return set_error(CSIC_EINVAL_NULL, "argument is NULL");
    FileCloser fc{fopen(path, "rb")};
    if (!fc.f) return set_error(CSIC_EIO, "cannot open %s", path);
    csic_planar_bits_layout L;
    csic_container_info ci;
    uint32_t stored = 0;
    const int st = read_header(fc.f, path, &ci, &L, &stored);
    if (st != CSIC_OK) return st;
    const size_t need = (size_t)ci.nframes * (size_t)L.frame_bytes;
    if (frames_bytes != need)
        return set_error(CSIC_EINVAL_SIZE, "expected room for %zu bytes (%d frames of %lld), got %zu", need, ci.nframes, (long long)L.frame_bytes,
                         frames_bytes);
    // the file pointer stands behind the header; bytes [16, 80) of it take part in the CRC
    unsigned char h[CONTAINER_HEADER];
    if (fseek(fc.f, 0, SEEK_SET) != 0 || fread(h, 1, sizeof h, fc.f) != sizeof h) return set_error(CSIC_EIO, "cannot read %s", path);
    uLong crc = crc32(0L, h + CONTAINER_CRC_FROM, (uInt)(CONTAINER_HEADER - CONTAINER_CRC_FROM));
    const int64_t plane_off[3] = {L.y_offset, L.cb_offset, L.cr_offset}, plane_bytes[3] = {L.y_bytes, L.cb_bytes, L.cr_bytes};
    unsigned char *base = static_cast<unsigned char *>(frames);
    std::memset(base, 0, need);
    for (int32_t k = 0; k < ci.nframes; ++k)
        for (int pl = 0; pl < 3; ++pl) {
            unsigned char *d = base + (int64_t)k * L.frame_bytes + plane_off[pl];
            if (fread(d, 1, (size_t)plane_bytes[pl], fc.f) != (size_t)plane_bytes[pl]) return set_error(CSIC_EIO, "cannot read %s", path);
            for (int64_t done = 0; done < plane_bytes[pl];) {
                const int64_t part = plane_bytes[pl] - done < (1 << 30) ? plane_bytes[pl] - done : (1 << 30);
                crc = crc32(crc, d + done, (uInt)part);
                done += part;
            }
        }
    if ((uint32_t)crc != stored) {
        std::memset(base, 0, need);
        return set_error(CSIC_EFORMAT, "%s: CRC mismatch (stored %08x, computed %08x)", path, stored, (uint32_t)crc);
    }
    clear_error();
    return CSIC_OK;
}

} // extern "C"
