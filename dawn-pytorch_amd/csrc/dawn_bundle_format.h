// The model bundle file (include/dawn_hip.h: "model bundle"), host side only: the layout constants, the header / index parser with
// every refusal, the checksum in plain C++.  No HIP in here: the same text compiles into the library (dawn_bundle.hip), into
// tools/dawn_generate.cpp and into the sanitizer program tools/bundle_check.cpp.  Header only, everything in one namespace.
//
// Every number of the file is read byte by byte as little-endian; every sum of two file numbers goes through add_ok().
#pragma once
#include "../../include/dawn_hip.h"

#include <stdint.h>
#include <stdio.h>
#include <string.h>

#include <algorithm>
#include <string>
#include <vector>

namespace dawn_bundle_format {

constexpr unsigned char MAGIC[8] = {'D', 'A', 'W', 'N', 'B', 'N', 'D', 'L'};
constexpr uint32_t VERSION = 1;
constexpr uint64_t HEADER_BYTES = 64, ENTRY_FIXED_BYTES = 48, ALIGN = 256, HOST_ALIGN = 16;
constexpr uint64_t MAX_INDEX_BYTES = 256ull << 20, MAX_HOST_BYTES = 64ull << 20, MAX_NAME_BYTES = 4096;
enum { STAGE_HUBERT = 0, STAGE_POSE = 1, STAGE_BLINK = 2, STAGE_DECODER = 3, STAGE_INPUTS = 4, STAGE_UNET = 5, STAGE_HOST = 6, STAGE_MOTION = 7, N_STAGES = 8 };
// STAGE_MOTION is optional and came after the first release of version 1: a reader from before it refuses a file that has the stage, by
// the stage number of the first such entry ("index entry i '<name>': stage 7"); a file without it reads as before.
enum { KIND_DEVICE = 0, KIND_HOST = 1 };
constexpr int N_DTYPES = 8;         // informational: 0 bytes, 1 f32, 2 bf16, 3 f16, 4 i32, 5 f64, 6 i64, 7 i16

inline const char* stage_name(uint32_t s) {
    static const char* const names[N_STAGES] = {"hubert", "pose", "blink", "decoder", "inputs", "unet", "host", "motion"};
    return s < N_STAGES ? names[s] : "?";
}

struct Header {
    uint32_t version = 0, abi = 0;
    uint64_t n_entries = 0, index_bytes = 0, payload_offset = 0, device_bytes = 0, file_bytes = 0;
};
struct Entry {
    uint32_t stage = 0, kind = 0, dtype = 0;
    std::string name;
    uint64_t offset = 0, length = 0, s1 = 0, s2 = 0;      // offset: bytes from the payload start
};
struct Bundle {
    Header h;
    std::vector<Entry> entries;
    std::vector<unsigned char> host;                       // payload bytes [device_bytes, file_bytes - payload_offset)
    const unsigned char* host_blob(const Entry& e) const { return host.data() + (e.offset - h.device_bytes); }
};

inline bool add_ok(uint64_t a, uint64_t b, uint64_t* out) { return !__builtin_add_overflow(a, b, out); }
inline uint32_t rd32(const unsigned char* p) { return (uint32_t)p[0] | (uint32_t)p[1] << 8 | (uint32_t)p[2] << 16 | (uint32_t)p[3] << 24; }
inline uint64_t rd64(const unsigned char* p) { return (uint64_t)rd32(p) | (uint64_t)rd32(p + 4) << 32; }

// s1 = sum w[i], s2 = sum (i + 1) w[i] mod 2^64 over the n little-endian 32-bit words at p
inline void checksum(const unsigned char* p, uint64_t n_words, uint64_t* s1, uint64_t* s2) {
    uint64_t a = 0, b = 0;
    for (uint64_t i = 0; i < n_words; ++i) {
        const uint64_t w = rd32(p + 4 * i);
        a += w;
        b += (i + 1) * w;
    }
    *s1 = a;
    *s2 = b;
}

inline int refuse(std::string* err, const std::string& what) {
    *err = "bundle: " + what;
    return -1;
}
inline std::string u64s(uint64_t v) {
    char m[32];
    snprintf(m, sizeof m, "%llu", (unsigned long long)v);
    return m;
}
inline std::string entry_id(const Entry& e) { return std::string("entry '") + stage_name(e.stage) + "/" + e.name + "'"; }

// the 64 header bytes; actual_file_bytes = what the file system says; abi = dawn_abi_version() of the reader
inline int parse_header(const unsigned char* p, uint64_t n, uint64_t actual_file_bytes, uint32_t abi, Header* h, std::string* err) {
    if (n < HEADER_BYTES) return refuse(err, "header: " + u64s(n) + " bytes, " + u64s(HEADER_BYTES) + " needed");
    if (memcmp(p, MAGIC, 8) != 0) return refuse(err, "magic: not a DAWN bundle");
    h->version = rd32(p + 8);
    h->abi = rd32(p + 12);
    h->n_entries = rd64(p + 16);
    h->index_bytes = rd64(p + 24);
    h->payload_offset = rd64(p + 32);
    h->device_bytes = rd64(p + 40);
    h->file_bytes = rd64(p + 48);
    if (h->version != VERSION) return refuse(err, "version: " + u64s(h->version) + ", this reader takes " + u64s(VERSION));
    if (h->abi != abi) return refuse(err, "abi: written for ABI " + u64s(h->abi) + ", this library is ABI " + u64s(abi));
    if (rd64(p + 56) != 0) return refuse(err, "reserved: header word 7 must be zero");
    if (h->file_bytes != actual_file_bytes)
        return refuse(err, "file_bytes: header says " + u64s(h->file_bytes) + ", the file has " + u64s(actual_file_bytes));
    uint64_t index_end = 0;
    if (h->index_bytes > MAX_INDEX_BYTES || !add_ok(HEADER_BYTES, h->index_bytes, &index_end) || index_end > h->file_bytes)
        return refuse(err, "index_bytes: " + u64s(h->index_bytes) + " leaves the file");
    if (h->n_entries > h->index_bytes / ENTRY_FIXED_BYTES)
        return refuse(err, "n_entries: " + u64s(h->n_entries) + " entries do not fit an index of " + u64s(h->index_bytes) + " bytes");
    if (h->payload_offset % ALIGN != 0 || h->payload_offset < index_end || h->payload_offset > h->file_bytes)
        return refuse(err, "payload_offset: " + u64s(h->payload_offset) + " (a multiple of 256 between the index end and the file end)");
    const uint64_t payload = h->file_bytes - h->payload_offset;
    if (h->device_bytes % ALIGN != 0 || h->device_bytes > payload)
        return refuse(err, "device_bytes: " + u64s(h->device_bytes) + " (a multiple of 256 within the payload of " + u64s(payload) + ")");
    if (payload - h->device_bytes > MAX_HOST_BYTES) return refuse(err, "host part: " + u64s(payload - h->device_bytes) + " bytes, at most 64 MiB");
    return 0;
}

// the index_bytes bytes behind the header
inline int parse_index(const unsigned char* p, uint64_t n, const Header& h, std::vector<Entry>* out, std::string* err) {
    if (n < h.index_bytes) return refuse(err, "index: " + u64s(n) + " bytes, " + u64s(h.index_bytes) + " needed");
    out->clear();
    uint64_t at = 0;
    for (uint64_t i = 0; i < h.n_entries; ++i) {
        const std::string id = "index entry " + u64s(i);
        if (h.index_bytes - at < ENTRY_FIXED_BYTES) return refuse(err, id + ": leaves the index");
        const unsigned char* q = p + at;
        Entry e;
        e.stage = rd32(q);
        e.kind = rd32(q + 4);
        e.dtype = rd32(q + 8);
        const uint64_t name_len = rd32(q + 12);
        e.offset = rd64(q + 16);
        e.length = rd64(q + 24);
        e.s1 = rd64(q + 32);
        e.s2 = rd64(q + 40);
        at += ENTRY_FIXED_BYTES;
        const uint64_t padded = (name_len + 7) & ~(uint64_t)7;
        if (name_len < 1 || name_len > MAX_NAME_BYTES || padded > h.index_bytes - at) return refuse(err, id + ": name_len " + u64s(name_len) + " leaves the index");
        e.name.assign((const char*)q + ENTRY_FIXED_BYTES, (size_t)name_len);
        if (e.name.find('\0') != std::string::npos) return refuse(err, id + ": name holds a zero byte");
        for (uint64_t k = name_len; k < padded; ++k)
            if (q[ENTRY_FIXED_BYTES + k] != 0) return refuse(err, id + ": name padding is not zero");
        at += padded;
        if (e.stage >= N_STAGES) return refuse(err, id + " '" + e.name + "': stage " + u64s(e.stage));
        if (e.kind > KIND_HOST) return refuse(err, id + " '" + e.name + "': kind " + u64s(e.kind));
        if (e.dtype >= (uint32_t)N_DTYPES) return refuse(err, id + " '" + e.name + "': dtype " + u64s(e.dtype));
        if (e.stage == STAGE_HOST && e.kind != KIND_HOST) return refuse(err, entry_id(e) + ": a device tensor in the host stage");
        out->push_back(std::move(e));
    }
    if (at != h.index_bytes) return refuse(err, "index_bytes: " + u64s(h.index_bytes) + ", the entries take " + u64s(at));
    return 0;
}

inline uint64_t blob_struct_bytes(const Entry& e, bool* array) {
    *array = false;
    if (e.name == "cfg") {
        switch (e.stage) {
            case STAGE_HUBERT: return sizeof(dawn_hubert_cfg);
            case STAGE_POSE: case STAGE_BLINK: return sizeof(dawn_pbnet_cfg);
            case STAGE_DECODER: return sizeof(dawn_decoder_cfg);
            case STAGE_INPUTS: return sizeof(dawn_inputs_cfg);
            case STAGE_UNET: return sizeof(dawn_unet_cfg);
            case STAGE_MOTION: return sizeof(dawn_motion_cfg);
            default: return 0;
        }
    }
    if (e.stage != STAGE_HOST) return 0;
    if (e.name == "defaults") return sizeof(dawn_bundle_defaults);
    *array = true;
    if (e.name.compare(0, 11, "steps.ddim.") == 0) return sizeof(dawn_ddim_step);
    if (e.name.compare(0, 16, "steps.ancestral.") == 0) return sizeof(dawn_ancestral_step);
    return 0;
}

// ranges, alignment, overlaps, names, struct sizes
inline int validate(const Header& h, const std::vector<Entry>& entries, std::string* err) {
    const uint64_t payload = h.file_bytes - h.payload_offset;
    std::vector<const Entry*> by_off, by_name;
    for (const Entry& e : entries) {
        uint64_t end = 0;
        if (e.length == 0) return refuse(err, entry_id(e) + ": length 0");
        if (!add_ok(e.offset, e.length, &end)) return refuse(err, entry_id(e) + ": offset + length overflows");
        if (e.kind == KIND_DEVICE) {
            if (e.offset % ALIGN != 0) return refuse(err, entry_id(e) + ": offset " + u64s(e.offset) + " is not a multiple of 256");
            if (e.length % 4 != 0) return refuse(err, entry_id(e) + ": length " + u64s(e.length) + " is not a multiple of 4");
            if (end > h.device_bytes) return refuse(err, entry_id(e) + ": leaves the device part of the payload (" + u64s(h.device_bytes) + " bytes)");
        } else {
            if (e.offset % HOST_ALIGN != 0) return refuse(err, entry_id(e) + ": offset " + u64s(e.offset) + " is not a multiple of 16");
            if (e.offset < h.device_bytes || end > payload) return refuse(err, entry_id(e) + ": leaves the host part of the payload");
            bool array = false;
            const uint64_t unit = blob_struct_bytes(e, &array);
            if (unit && (array ? e.length % unit != 0 : e.length != unit))
                return refuse(err, entry_id(e) + ": " + u64s(e.length) + " bytes, the struct has " + u64s(unit));
        }
        by_off.push_back(&e);
        by_name.push_back(&e);
    }
    std::sort(by_off.begin(), by_off.end(), [](const Entry* a, const Entry* b) { return a->offset < b->offset; });
    for (size_t i = 1; i < by_off.size(); ++i)
        if (by_off[i - 1]->offset + by_off[i - 1]->length > by_off[i]->offset)
            return refuse(err, entry_id(*by_off[i]) + " overlaps " + entry_id(*by_off[i - 1]));
    std::sort(by_name.begin(), by_name.end(), [](const Entry* a, const Entry* b) {
        return a->stage != b->stage ? a->stage < b->stage : a->kind != b->kind ? a->kind < b->kind : a->name < b->name;
    });
    for (size_t i = 1; i < by_name.size(); ++i)
        if (by_name[i - 1]->stage == by_name[i]->stage && by_name[i - 1]->kind == by_name[i]->kind && by_name[i - 1]->name == by_name[i]->name)
            return refuse(err, entry_id(*by_name[i]) + ": name given twice");
    return 0;
}

// host blobs against their checksum words (padded with zeros to whole words)
inline int check_host_blobs(const Bundle& b, std::string* err) {
    for (const Entry& e : b.entries) {
        if (e.kind != KIND_HOST) continue;
        std::vector<unsigned char> padded(b.host_blob(e), b.host_blob(e) + e.length);
        padded.resize((padded.size() + 3) & ~(size_t)3, 0);
        uint64_t s1 = 0, s2 = 0;
        checksum(padded.data(), padded.size() / 4, &s1, &s2);
        if (s1 != e.s1 || s2 != e.s2) return refuse(err, entry_id(e) + ": checksum mismatch");
    }
    return 0;
}

// header + index from memory (what the sanitizer program feeds truncated and mutated); actual_file_bytes as parse_header
inline int parse_memory(const unsigned char* p, uint64_t n, uint64_t actual_file_bytes, uint32_t abi, Bundle* b, std::string* err) {
    if (parse_header(p, n, actual_file_bytes, abi, &b->h, err) != 0) return -1;
    if (n - HEADER_BYTES < b->h.index_bytes) return refuse(err, "index: " + u64s(n - HEADER_BYTES) + " bytes, " + u64s(b->h.index_bytes) + " needed");
    if (parse_index(p + HEADER_BYTES, b->h.index_bytes, b->h, &b->entries, err) != 0) return -1;
    return validate(b->h, b->entries, err);
}

inline bool file_size(FILE* f, uint64_t* out) {
    if (fseeko(f, 0, SEEK_END) != 0) return false;
    const off_t n = ftello(f);
    if (n < 0) return false;
    *out = (uint64_t)n;
    return fseeko(f, 0, SEEK_SET) == 0;
}

// header, index and the host part of the file at `path`; the device part is not read
inline int open_file(const char* path, uint32_t abi, Bundle* b, std::string* err) {
    FILE* f = path ? fopen(path, "rb") : nullptr;
    if (!f) return refuse(err, std::string("cannot open '") + (path ? path : "(null)") + "'");
    uint64_t size = 0;
    unsigned char head[HEADER_BYTES];
    int rc = 0;
    std::vector<unsigned char> index;
    if (!file_size(f, &size)) rc = refuse(err, "cannot size the file");
    const size_t got = rc == 0 ? fread(head, 1, sizeof head, f) : 0;
    if (rc == 0) rc = parse_header(head, got, size, abi, &b->h, err);
    if (rc == 0) {
        index.resize((size_t)b->h.index_bytes);
        if (fread(index.data(), 1, index.size(), f) != index.size()) rc = refuse(err, "index: short read");
    }
    if (rc == 0) rc = parse_index(index.data(), index.size(), b->h, &b->entries, err);
    if (rc == 0) rc = validate(b->h, b->entries, err);
    if (rc == 0) {
        b->host.resize((size_t)(b->h.file_bytes - b->h.payload_offset - b->h.device_bytes));
        if (fseeko(f, (off_t)(b->h.payload_offset + b->h.device_bytes), SEEK_SET) != 0 ||
            fread(b->host.data(), 1, b->host.size(), f) != b->host.size())
            rc = refuse(err, "host part: short read");
    }
    if (rc == 0) rc = check_host_blobs(*b, err);
    fclose(f);
    return rc;
}

}  // namespace dawn_bundle_format
