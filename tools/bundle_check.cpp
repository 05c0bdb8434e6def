// bundle_check: the host-only parsers of this repository under the host compiler's sanitizers.  A stand-alone program (no HIP, no
// library): it compiles csrc/dawn_bundle_format.h and tools/media_files.h with -fsanitize=address,undefined and feeds them valid and
// broken files (tests/test_bundle_cpu.py).
//
//   bundle_check [--abi N] bundle FILE     open the bundle as dawn_bundle_open does          -> exit 0 accepted, 3 refused (message on stderr)
//   bundle_check [--abi N] mutate FILE     FILE is a valid bundle; in memory: every truncation of its header and index, length by
//                                          length, then every header and index field set to 0, 2^63 and 2^64 - 1 (32-bit fields: 0, 2^31,
//                                          2^32 - 1).  One line per case class; exit 0 unless a truncation was accepted or FILE is not valid
//   bundle_check wav FILE | pnm FILE | y4m FILE       parse the file                         -> exit 0 accepted, 3 refused
//
// Build:  g++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=all -I dawn-pytorch_amd/csrc tools/bundle_check.cpp -o bundle_check
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <string>
#include <vector>

#include "dawn_bundle_format.h"
#include "media_files.h"

namespace fmt = dawn_bundle_format;

namespace {

// what dawn_bundle_open checks, on a whole file in memory
int check_memory(const std::vector<unsigned char>& file, uint32_t abi, std::string* err) {
    fmt::Bundle b;
    if (fmt::parse_memory(file.data(), file.size(), file.size(), abi, &b, err) != 0) return -1;
    const uint64_t host_at = b.h.payload_offset + b.h.device_bytes;         // (validated: within file_bytes == file.size())
    b.host.assign(file.begin() + (ptrdiff_t)host_at, file.end());
    return fmt::check_host_blobs(b, err);
}

void put(std::vector<unsigned char>& f, size_t at, uint64_t v, int bytes) {
    for (int i = 0; i < bytes; ++i) f[at + i] = (unsigned char)(v >> (8 * i));
}

int mutate(const std::vector<unsigned char>& file, uint32_t abi) {
    std::string err;
    if (check_memory(file, abi, &err) != 0) {
        fprintf(stderr, "bundle_check: the input is not a valid bundle: %s\n", err.c_str());
        return 3;
    }
    fmt::Bundle b;
    fmt::parse_memory(file.data(), file.size(), file.size(), abi, &b, &err);
    const size_t head = (size_t)(fmt::HEADER_BYTES + b.h.index_bytes);
    size_t accepted = 0;
    for (size_t n = 0; n < head; ++n) {                                        // a fresh allocation of exactly n bytes: a read past it is a report
        std::vector<unsigned char> cut(file.begin(), file.begin() + (ptrdiff_t)n);
        if (check_memory(cut, abi, &err) == 0) ++accepted;
    }
    printf("TRUNCATIONS %zu accepted %zu\n", head, accepted);
    struct Field { size_t at; int bytes; };
    std::vector<Field> fields;
    for (size_t at = 8; at < 16; at += 4) fields.push_back({at, 4});          // version, abi
    for (size_t at = 16; at < 64; at += 8) fields.push_back({at, 8});         // n_entries .. the reserved word
    size_t at = fmt::HEADER_BYTES;
    for (const fmt::Entry& e : b.entries) {
        for (int k = 0; k < 4; ++k) fields.push_back({at + 4 * (size_t)k, 4});            // stage, kind, dtype, name_len
        for (int k = 0; k < 4; ++k) fields.push_back({at + 16 + 8 * (size_t)k, 8});       // offset, length, s1, s2
        at += fmt::ENTRY_FIXED_BYTES + ((e.name.size() + 7) & ~(size_t)7);
    }
    size_t cases = 0, refused = 0, unchanged = 0;
    for (const Field& fd : fields) {
        const uint64_t values[3] = {0, fd.bytes == 8 ? 1ull << 63 : 1ull << 31, fd.bytes == 8 ? ~0ull : 0xffffffffull};
        for (uint64_t v : values) {
            std::vector<unsigned char> m(file);
            put(m, fd.at, v, fd.bytes);
            ++cases;
            if (m == file) ++unchanged;                                        // (the field held that value already)
            else if (check_memory(m, abi, &err) != 0) ++refused;
            else printf("ACCEPTED field at byte %zu = %llu\n", fd.at, (unsigned long long)v);
        }
    }
    printf("FIELDS %zu cases %zu refused %zu unchanged %zu\n", fields.size(), cases, refused, unchanged);
    return accepted == 0 ? 0 : 1;
}

}  // namespace

int main(int argc, char** argv) {
    uint32_t abi = 8;
    int i = 1;
    if (argc > 2 && strcmp(argv[1], "--abi") == 0) {
        abi = (uint32_t)strtoul(argv[2], nullptr, 10);
        i = 3;
    }
    if (argc - i != 2) {
        fprintf(stderr, "usage: bundle_check [--abi N] bundle|mutate|wav|pnm|y4m FILE\n");
        return 2;
    }
    const std::string mode = argv[i];
    const char* path = argv[i + 1];
    std::string err;
    int rc = 0;
    if (mode == "bundle") {
        fmt::Bundle b;
        rc = fmt::open_file(path, abi, &b, &err);
        if (rc == 0) printf("OK %zu entries, %llu device bytes\n", b.entries.size(), (unsigned long long)b.h.device_bytes);
    } else {
        std::vector<unsigned char> raw;
        if (media_files::read_file(path, &raw, &err) != 0) {
            fprintf(stderr, "bundle_check: %s\n", err.c_str());
            return 2;
        }
        if (mode == "mutate") return mutate(raw, abi);
        if (mode == "wav") {
            media_files::Wav w;
            rc = media_files::parse_wav(raw.data(), raw.size(), &w, &err);
            if (rc == 0) printf("OK %ld frames, %d channels, %d Hz\n", w.n_frames, w.channels, w.rate);
        } else if (mode == "pnm") {
            media_files::Image im;
            rc = media_files::parse_pnm(raw.data(), raw.size(), &im, &err);
            if (rc == 0) printf("OK %d x %d x %d\n", im.width, im.height, im.channels);
        } else if (mode == "y4m") {
            media_files::Y4m v;
            rc = media_files::parse_y4m(raw.data(), raw.size(), &v, &err);
            if (rc == 0) printf("OK %ld frames of %d x %d, %zu bytes\n", v.n_frames, v.width, v.height, v.frames.size());
        } else {
            fprintf(stderr, "usage: bundle_check [--abi N] bundle|mutate|wav|pnm|y4m FILE\n");
            return 2;
        }
    }
    if (rc != 0) {
        fprintf(stderr, "bundle_check: refused: %s\n", err.c_str());
        return 3;
    }
    return 0;
}
