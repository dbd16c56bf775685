// state_file.h -- the container of the library's own state file (cogaps_session_save_state / _load_state): host code only.
//
//   [header, 40 bytes] magic "CGHSTATE", u32 version, u32 nSections, u64 fileBytes, u64 checksum, u64 reserved
//   [section table]    nSections x { u32 id, u32 reserved, u64 offset (from the file's start), u64 bytes }
//   [payload]          the sections, each padded with zero bytes to a multiple of 8
//
// All integers little-endian (the library runs on little-endian hosts only and writes its words as they lie in memory).  The checksum
// covers everything behind the header -- table, payload, pads -- as 64-bit words.  What the sections mean is the caller's business
// (session_state.h); this file knows bytes.
#pragma once
#include <errno.h>
#include <stdint.h>
#include <stdio.h>
#include <string.h>
#include <unistd.h>
#include <algorithm>
#include <string>
#include <vector>
#include <stdexcept>

namespace cgstate {

static const char MAGIC[8] = {'C', 'G', 'H', 'S', 'T', 'A', 'T', 'E'};
static const uint32_t VERSION = 1;
static const uint32_t MAX_SECTIONS = 256;

struct Header { char magic[8]; uint32_t version, nSections; uint64_t fileBytes, checksum, reserved; };
struct TableEntry { uint32_t id, reserved; uint64_t offset, bytes; };
static_assert(sizeof(Header) == 40 && sizeof(TableEntry) == 24, "the file's layout");

inline uint64_t pad8(uint64_t n) { return (n + 7u) & ~(uint64_t)7u; }

// 64-bit checksum over 64-bit words, fed in pieces whose lengths are multiples of 8
struct Checksum {
    uint64_t h = 0x243F6A8885A308D3ull;
    void feed(const void *p, size_t bytes)
    {
        const unsigned char *b = (const unsigned char *)p;
        for (size_t i = 0; i + 8 <= bytes; i += 8) { uint64_t w; memcpy(&w, b + i, 8); h = (h ^ w) * 0x9E3779B97F4A7C15ull; h ^= h >> 29; }
    }
    uint64_t value() const { uint64_t x = h; x ^= x >> 31; x *= 0xBF58476D1CE4E5B9ull; return x ^ (x >> 29); }
};
inline uint64_t hash_bytes(const void *p, size_t bytes)
{
    Checksum c; const size_t whole = bytes & ~(size_t)7u; c.feed(p, whole);
    uint64_t tail = 0; memcpy(&tail, (const unsigned char *)p + whole, bytes - whole); tail ^= (uint64_t)bytes << 56; c.feed(&tail, 8);
    return c.value();
}

// One array of the state: where it lives -- host memory or device memory, never both -- and its size.  The same list describes what a
// save writes and what a load expects to find.
struct Section { uint32_t id; void *host; void *dev; uint64_t bytes; };
// `bytes` bytes in pieces of at most pieceBytes, in order: each(offset, n).  How a device section passes through the staging buffer,
// whichever way it goes.
template <class Each> inline void in_pieces(uint64_t bytes, size_t pieceBytes, Each each)
{
    for (uint64_t o = 0; o < bytes; ) { const size_t n = (size_t)std::min<uint64_t>(pieceBytes, bytes - o); each(o, n); o += n; }
}

// Writes path + ".tmp" in the same directory, flushes it to the disk, then renames it over `path`: a save that dies half way leaves the
// previous file as it was.  `copyOut(section, offset, n, buffer)` fetches n bytes of a device section into the staging buffer.
struct Writer {
    std::string path, tmp; FILE *f = nullptr; Checksum sum; uint64_t written = 0;
    explicit Writer(const char *p) : path(p), tmp(std::string(p) + ".tmp")
    {
        f = fopen(tmp.c_str(), "wb");
        if (!f) throw std::runtime_error("state file: cannot write " + tmp + ": " + strerror(errno));
    }
    ~Writer() { if (f) { fclose(f); remove(tmp.c_str()); } }
    void put(const void *p, size_t n, bool summed = true)
    {
        if (n && fwrite(p, 1, n, f) != n) throw std::runtime_error("state file: writing " + tmp + " failed: " + strerror(errno));
        if (summed) sum.feed(p, n);
        written += n;
    }
    template <class CopyOut> void write(const std::vector<Section> &secs, void *staging, size_t stagingBytes, CopyOut copyOut)
    {
        Header h; memset(&h, 0, sizeof(h)); memcpy(h.magic, MAGIC, 8); h.version = VERSION; h.nSections = (uint32_t)secs.size();
        std::vector<TableEntry> tab(secs.size());
        uint64_t off = sizeof(Header) + sizeof(TableEntry) * secs.size();
        for (size_t i = 0; i < secs.size(); ++i) { tab[i].id = secs[i].id; tab[i].reserved = 0; tab[i].offset = off; tab[i].bytes = secs[i].bytes; off += pad8(secs[i].bytes); }
        h.fileBytes = off;
        put(&h, sizeof(h), false);
        put(tab.data(), sizeof(TableEntry) * tab.size());
        for (const Section &s : secs) {
            if (s.host) put(s.host, (size_t)(s.bytes & ~(uint64_t)7u));
            else in_pieces(s.bytes & ~(uint64_t)7u, stagingBytes, [&](uint64_t o, size_t n) { copyOut(s, o, n, staging); put(staging, n); });
            if (const size_t rest = (size_t)(s.bytes & 7u)) {      // the last, partial word with its zero pad
                uint64_t w = 0;
                if (s.host) memcpy(&w, (const char *)s.host + (s.bytes - rest), rest); else { copyOut(s, s.bytes - rest, rest, staging); memcpy(&w, staging, rest); }
                put(&w, 8);
            }
        }
        h.checksum = sum.value();
        if (fseek(f, 0, SEEK_SET) != 0 || fwrite(&h, 1, sizeof(h), f) != sizeof(h) || fflush(f) != 0 || fsync(fileno(f)) != 0)
            throw std::runtime_error("state file: writing " + tmp + " failed: " + strerror(errno));
        if (fclose(f) != 0) { f = nullptr; remove(tmp.c_str()); throw std::runtime_error("state file: writing " + tmp + " failed: " + strerror(errno)); }
        f = nullptr;
        if (rename(tmp.c_str(), path.c_str()) != 0) { const std::string why = strerror(errno); remove(tmp.c_str()); throw std::runtime_error("state file: cannot replace " + path + ": " + why); }
    }
};

// Opens a state file and validates the container: magic, version, length, table, checksum -- in that order, each with its own message.
// Nothing is handed out before all of them hold.
struct Reader {
    FILE *f = nullptr; Header h; std::vector<TableEntry> tab;
    Reader(const char *path, void *staging, size_t stagingBytes)
    {
        f = fopen(path, "rb");
        if (!f) throw std::runtime_error(std::string("state file: cannot read ") + path + ": " + strerror(errno));
        try { validate(path, staging, stagingBytes); } catch (...) { fclose(f); f = nullptr; throw; }
    }
    void validate(const char *path, void *staging, size_t stagingBytes)
    {
        if (fseek(f, 0, SEEK_END) != 0) fail_io(path);
        const long long actual = ftell(f);
        if (actual < 0 || fseek(f, 0, SEEK_SET) != 0) fail_io(path);
        if ((uint64_t)actual < sizeof(Header) || fread(&h, 1, sizeof(h), f) != sizeof(h) || memcmp(h.magic, MAGIC, 8) != 0)
            throw std::runtime_error(std::string("state file: ") + path + " is not a state file of this library (its first bytes are not the magic)");
        if (h.version > VERSION) throw std::runtime_error(std::string("state file: ") + path + " has format version " + std::to_string(h.version) + ", newer than the version " + std::to_string(VERSION) + " this library reads");
        if (h.version == 0) throw std::runtime_error(std::string("state file: ") + path + " has format version 0, which never existed");
        if ((uint64_t)actual < h.fileBytes) throw std::runtime_error(std::string("state file: ") + path + " is truncated: " + std::to_string(actual) + " of " + std::to_string(h.fileBytes) + " bytes");
        if ((uint64_t)actual != h.fileBytes || h.nSections > MAX_SECTIONS || (h.fileBytes & 7u) || h.fileBytes < sizeof(Header) + sizeof(TableEntry) * (uint64_t)h.nSections)
            throw std::runtime_error(std::string("state file: ") + path + " is corrupt: its length and section count do not fit its header");
        tab.resize(h.nSections);
        Checksum sum;
        if (fread(tab.data(), sizeof(TableEntry), tab.size(), f) != tab.size()) fail_io(path);
        sum.feed(tab.data(), sizeof(TableEntry) * tab.size());
        in_pieces(h.fileBytes - sizeof(Header) - sizeof(TableEntry) * tab.size(), stagingBytes, [&](uint64_t, size_t n) {
            if (fread(staging, 1, n, f) != n) fail_io(path);
            sum.feed(staging, n); });
        if (sum.value() != h.checksum) throw std::runtime_error(std::string("state file: ") + path + " is corrupt: its checksum does not match its contents");
        uint64_t off = sizeof(Header) + sizeof(TableEntry) * tab.size();
        for (const TableEntry &e : tab) {      // (behind the checksum this can only be a writer's mistake)
            if (e.offset != off || e.bytes > h.fileBytes - off) throw std::runtime_error(std::string("state file: ") + path + " is corrupt: its section table does not describe its payload");
            off += pad8(e.bytes);
        }
        if (off != h.fileBytes) throw std::runtime_error(std::string("state file: ") + path + " is corrupt: its section table does not describe its payload");
    }
    ~Reader() { if (f) fclose(f); }
    [[noreturn]] static void fail_io(const char *path) { throw std::runtime_error(std::string("state file: reading ") + path + " failed"); }
    const TableEntry *find(uint32_t id) const { for (const TableEntry &e : tab) if (e.id == id) return &e; return nullptr; }
    void read(const TableEntry &e, uint64_t offset, void *dst, size_t n)
    {
        if (fseek(f, (long)(e.offset + offset), SEEK_SET) != 0 || fread(dst, 1, n, f) != n) throw std::runtime_error("state file: reading a section failed");
    }
    // a device section, the way Writer::write sends one out: `copyIn(section, offset, n, buffer)` takes n bytes from the staging buffer
    template <class CopyIn> void read_pieces(const TableEntry &e, const Section &s, void *staging, size_t stagingBytes, CopyIn copyIn)
    {
        in_pieces(s.bytes, stagingBytes, [&](uint64_t o, size_t n) { read(e, o, staging, n); copyIn(s, o, n, staging); });
    }
};

} // namespace cgstate
