// rows_fuzz.cpp -- the host codec of the row-prediction layer (csic_rows_host / csic_unrows_host, csrc/csic_rows_host.cpp) and the
// version-8 reader (csrc/csic_container.cpp) under ASan + UBSan, every buffer in a heap block of exactly its size:
//   1. random frames of random parameter sets -- rows shorter than a group, rows of 32 K + delta samples, one band and several --
//      through csic_rows_host and back, apart and in place;
//   2. about 4 000 mutated maps -- bit flips, random bytes, all ones -- into csic_unrows_host: CSIC_OK with frames that go through the
//      layer and back to themselves, or CSIC_EFORMAT with the destination untouched;
//   3. version-8 files of the three codings written by csic_container_write_rows, then about 3 000 mutated copies -- bit flips with and
//      without a re-signed CRC, truncations, extensions, damaged header words -- into csic_container_info_of, csic_container_rows,
//      csic_container_inter_groups and csic_container_read: CSIC_OK, CSIC_EFORMAT or, where the header's size changed,
//      CSIC_EINVAL_SIZE, never an access out of range.
// Built and run by tests/test_cpp_rows.py with the directory for its files as the only argument; no GPU, nothing of the HIP library.
#include <zlib.h>

#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <memory>
#include <string>
#include <vector>

#include "csic.h"

static uint64_t rng_state = 0x9E3779B97F4A7C15ull;
static uint32_t rnd()
{
    rng_state ^= rng_state << 13; rng_state ^= rng_state >> 7; rng_state ^= rng_state << 17;
    return (uint32_t)(rng_state >> 16);
}

#define REQUIRE(cond) do { if (!(cond)) { std::printf("FAILED %s:%d: %s (%s)\n", __FILE__, __LINE__, #cond, csic_last_error()); return 1; } } while (0)

typedef std::unique_ptr<unsigned char[]> Block;          // exactly its size on the heap: ASan sees one byte too many
static Block block(size_t n, int fill)
{
    Block b(new unsigned char[n ? n : 1]);
    std::memset(b.get(), fill, n);
    return b;
}

static csic_params random_params()
{
    static const int ab[6][2] = {{4, 4}, {2, 2}, {2, 0}, {1, 1}, {4, 0}, {1, 0}};
    csic_params p;
    const int widths[8] = {20, 32, 33, 63, 64, 95, 130, 40};
    csic_params_default(&p, widths[rnd() % 8] * (rnd() % 4 == 0 ? 2 : 1), 1 + (int)(rnd() % 40));
    const int k = (int)(rnd() % 6);
    p.chroma_a = ab[k][0]; p.chroma_b = ab[k][1];
    p.y_bits = 1 + (int)(rnd() % 8); p.cb_bits = 1 + (int)(rnd() % 8); p.cr_bits = 1 + (int)(rnd() % 8);
    p.factor = 1;
    p.op[0] = 3; p.op[1] = 1; p.op[2] = 2;
    p.out_format = CSIC_FMT_PLANAR_BITS;
    return p;
}

// `n` valid frames: random bytes, rows repeated here and there, normalised through the inverse with maps of zeros (the codes as they
// are, the bits behind a plane's last sample 0, 0xEE outside the payload ranges)
static int make_frames(const csic_params &p, const csic_planar_bits_layout &B, const csic_rows_layout &L, int n, Block &frames)
{
    const size_t fb = (size_t)B.frame_bytes;
    Block raw = block(n * fb, 0), maps = block((size_t)(n - 1) * L.map_stride + L.map_bytes, 0);
    const int kind = (int)(rnd() % 3);
    for (size_t i = 0; i < n * fb; ++i) raw[i] = kind == 0 ? (unsigned char)rnd() : kind == 1 ? (unsigned char)(i % 97 < 60 ? 0x55 : rnd()) : (unsigned char)((i / 7) & 0xFF);
    frames = block(n * fb, 0xEE);
    REQUIRE(csic_unrows_host(&p, raw.get(), maps.get(), n, frames.get()) == CSIC_OK);
    return 0;
}

static int codec_fuzz()
{
    int refused = 0, decoded = 0;
    for (int it = 0; it < 400; ++it) {
        const csic_params p = random_params();
        csic_planar_bits_layout B;
        csic_rows_layout L;
        REQUIRE(csic_planar_bits_layout_of(&p, &B) == CSIC_OK && csic_rows_layout_of(&p, &L) == CSIC_OK);
        const int n = 1 + (int)(rnd() % 3);
        const size_t fb = (size_t)B.frame_bytes, total = n * fb, mbytes = (size_t)(n - 1) * L.map_stride + L.map_bytes;
        Block src;
        if (make_frames(p, B, L, n, src)) return 1;
        Block diff = block(total, 0xEE), maps = block(mbytes, 0xEE), back = block(total, 0xEE);
        REQUIRE(csic_rows_host(&p, src.get(), n, diff.get(), maps.get()) == CSIC_OK);
        REQUIRE(csic_unrows_host(&p, diff.get(), maps.get(), n, back.get()) == CSIC_OK && std::memcmp(back.get(), src.get(), total) == 0);
        Block work = block(total, 0);
        std::memcpy(work.get(), diff.get(), total);
        REQUIRE(csic_unrows_host(&p, work.get(), maps.get(), n, work.get()) == CSIC_OK && std::memcmp(work.get(), src.get(), total) == 0);
        REQUIRE(csic_rows_host(&p, src.get(), n, src.get(), maps.get()) == CSIC_EINVAL_SIZE);      // forward: not even in place
        for (int m = 0; m < 10; ++m) {
            Block bad = block(mbytes, 0);
            std::memcpy(bad.get(), maps.get(), mbytes);
            const int how = (int)(rnd() % 4);
            const size_t frame = rnd() % n, at = frame * L.map_stride + rnd() % L.map_bytes;
            if (how == 0) bad[at] ^= (unsigned char)(1u << (rnd() % 8));
            else if (how == 1) bad[at] = (unsigned char)rnd();
            else if (how == 2) std::memset(bad.get() + frame * L.map_stride, 0xFF, (size_t)L.map_bytes);
            else for (int k = 0; k < 8; ++k) bad[frame * L.map_stride + rnd() % L.map_bytes] ^= (unsigned char)rnd();
            Block out = block(total, 0x5A);
            const int st = csic_unrows_host(&p, diff.get(), bad.get(), n, out.get());
            REQUIRE(st == CSIC_OK || st == CSIC_EFORMAT);
            if (st == CSIC_EFORMAT) {
                for (size_t i = 0; i < total; ++i) REQUIRE(out[i] == 0x5A);
                ++refused;
                continue;
            }
            ++decoded;                                                  // other frames, but frames: they go through the layer and back
            Block d2 = block(total, 0x5A), m2 = block(mbytes, 0), b2 = block(total, 0x5A);
            REQUIRE(csic_rows_host(&p, out.get(), n, d2.get(), m2.get()) == CSIC_OK);
            REQUIRE(csic_unrows_host(&p, d2.get(), m2.get(), n, b2.get()) == CSIC_OK && std::memcmp(b2.get(), out.get(), total) == 0);
        }
    }
    REQUIRE(refused > 100 && decoded > 100);
    std::printf("codec: %d mutated maps refused, %d decoded\n", refused, decoded);
    return 0;
}

static bool write_file(const std::string &path, const std::vector<unsigned char> &v)
{
    FILE *f = std::fopen(path.c_str(), "wb");
    if (!f) return false;
    const bool ok = std::fwrite(v.data(), 1, v.size(), f) == v.size();
    return std::fclose(f) == 0 && ok;
}

static int container_fuzz(const std::string &dir)
{
    const std::string good = dir + "/rows_good.csic", bad = dir + "/rows_bad.csic";
    int ok = 0, refused = 0;
    for (int it = 0; it < 60; ++it) {
        const csic_params p = random_params();
        csic_planar_bits_layout B;
        csic_rows_layout L;
        REQUIRE(csic_planar_bits_layout_of(&p, &B) == CSIC_OK && csic_rows_layout_of(&p, &L) == CSIC_OK);
        const int n = 1 + (int)(rnd() % 3), coding = (const int[]){CSIC_CODING_GROUPS, CSIC_CODING_RICE, CSIC_CODING_RANS}[it % 3];
        const size_t total = (size_t)n * B.frame_bytes;
        Block src;
        if (make_frames(p, B, L, n, src)) return 1;
        REQUIRE(csic_container_write_rows(good.c_str(), &p, src.get(), n, coding) == CSIC_OK);
        REQUIRE(csic_container_write_rows(good.c_str(), &p, src.get(), n, CSIC_CODING_RAW) == CSIC_EINVAL_FORMAT);
        FILE *f = std::fopen(good.c_str(), "rb");
        REQUIRE(f != nullptr);
        std::vector<unsigned char> data;
        for (int c; (c = std::fgetc(f)) != EOF;) data.push_back((unsigned char)c);
        std::fclose(f);
        int32_t flag = 0;
        REQUIRE(csic_container_rows(good.c_str(), &flag) == CSIC_OK && flag == 1);
        Block back = block(total, 0x5A);
        REQUIRE(csic_container_read(good.c_str(), back.get(), total) == CSIC_OK);
        for (int pl = 0; pl < 3; ++pl) {
            const int64_t off = pl == 0 ? B.y_offset : pl == 1 ? B.cb_offset : B.cr_offset, nb = pl == 0 ? B.y_bytes : pl == 1 ? B.cb_bytes : B.cr_bytes;
            for (int k = 0; k < n; ++k) REQUIRE(std::memcmp(back.get() + k * B.frame_bytes + off, src.get() + k * B.frame_bytes + off, (size_t)nb) == 0);
        }
        for (int m = 0; m < 50; ++m) {
            std::vector<unsigned char> v = data;
            const int how = (int)(rnd() % 6);
            if (how == 0) v[rnd() % v.size()] ^= (unsigned char)(1u << (rnd() % 8));
            else if (how == 1) v[80 + rnd() % 8] ^= (unsigned char)(1u << (rnd() % 8));                 // the coding word, the zero word
            else if (how == 2) v[96 + rnd() % (v.size() - 96)] = (unsigned char)rnd();                  // a map or a coded frame (n = 1: from the first record on)
            else if (how == 3) v.resize(v.size() - 1 - rnd() % 40);
            else if (how == 4) v.insert(v.end(), 1 + rnd() % 9, (unsigned char)rnd());
            else for (int k = 0; k < 6; ++k) v[88 + 8 * n + rnd() % (size_t)L.map_bytes] ^= (unsigned char)rnd();      // the first frame's map
            if (rnd() % 4 != 0 && v.size() > 16) {                                                        // mostly with a CRC that is right again
                const uint32_t crc = (uint32_t)crc32(0L, v.data() + 16, (uInt)(v.size() - 16));
                for (int k = 0; k < 4; ++k) v[12 + k] = (unsigned char)(crc >> (8 * k));
            }
            REQUIRE(write_file(bad, v));
            csic_container_info info;
            const int si = csic_container_info_of(bad.c_str(), &info);
            REQUIRE(si == CSIC_OK || si == CSIC_EFORMAT);
            REQUIRE(csic_container_rows(bad.c_str(), &flag) == si);
            size_t room = total;
            if (si == CSIC_OK) {
                csic_planar_bits_layout B2;
                REQUIRE(csic_planar_bits_layout_of(&info.params, &B2) == CSIC_OK);
                room = (size_t)info.nframes * (size_t)B2.frame_bytes;
                if (room > (64u << 20)) continue;                        // a header that now names a huge frame: the reader would only be refused the memory
                std::vector<uint64_t> counts(3 * (size_t)info.nframes);
                const int sg = csic_container_inter_groups(bad.c_str(), counts.data(), (int32_t)counts.size());
                REQUIRE(sg == CSIC_OK || sg == CSIC_EFORMAT);
            }
            Block out = block(room, 0x5A);
            const int st = csic_container_read(bad.c_str(), out.get(), room);
            REQUIRE(st == CSIC_OK || st == CSIC_EFORMAT || st == CSIC_EINVAL_SIZE);
            REQUIRE(si == CSIC_OK || st == CSIC_EFORMAT);
            st == CSIC_OK ? ++ok : ++refused;
        }
    }
    REQUIRE(refused > 500);
    std::printf("container: %d mutated files refused, %d read\n", refused, ok);
    std::remove(good.c_str());
    std::remove(bad.c_str());
    return 0;
}

int main(int argc, char **argv)
{
    if (argc < 2) { std::printf("usage: rows_fuzz DIR\n"); return 2; }
    if (codec_fuzz() || container_fuzz(argv[1])) return 1;
    std::printf("rows fuzz ok\n");
    return 0;
}
