// The file parsers of tools/dawn_generate.cpp, from memory: a RIFF/WAVE file of 16-bit PCM, a binary PPM / PGM and a YUV4MPEG2 stream
// of 8-bit 4:2:0 frames.  Plain C++, no
// HIP; tools/bundle_check.cpp runs them under the host sanitizers.  Every size read from a file is checked against the bytes that
// are there before it is used.
#pragma once
#include <stdint.h>
#include <stdio.h>
#include <string.h>

#include <string>
#include <vector>

namespace media_files {

struct Wav {
    int channels = 0, rate = 0;
    long n_frames = 0;
    std::vector<int16_t> pcm;                  // n_frames x channels, interleaved
};
struct Image {
    int width = 0, height = 0, channels = 0;   // 3 = P6 (RGB), 1 = P5 (grey)
    std::vector<unsigned char> pixels;         // height rows of width x channels bytes
};

inline int refuse(std::string* err, const std::string& what) {
    *err = what;
    return -1;
}
inline uint32_t le16(const unsigned char* p) { return (uint32_t)p[0] | (uint32_t)p[1] << 8; }
inline uint32_t le32(const unsigned char* p) { return le16(p) | le16(p + 2) << 16; }

// 16-bit PCM, 1 .. 8 channels: format tag 1, or 0xFFFE (extensible) with the PCM subformat -- what Python's `wave` reads.  A chunk whose
// size leaves the file is refused.
inline int parse_wav(const unsigned char* p, size_t n, Wav* out, std::string* err) {
    static const unsigned char PCM_GUID_TAIL[14] = {0x00, 0x00, 0x00, 0x00, 0x10, 0x00, 0x80, 0x00, 0x00, 0xAA, 0x00, 0x38, 0x9B, 0x71};
    if (n < 12 || memcmp(p, "RIFF", 4) != 0 || memcmp(p + 8, "WAVE", 4) != 0) return refuse(err, "wav: not a RIFF/WAVE file");
    size_t at = 12;
    bool have_fmt = false;
    int bits = 0;
    while (n - at >= 8) {
        const unsigned char* id = p + at;
        const size_t size = le32(p + at + 4);
        at += 8;
        if (size > n - at) return refuse(err, "wav: chunk '" + std::string((const char*)id, 4) + "' of " + std::to_string(size) + " bytes leaves the file");
        if (memcmp(id, "fmt ", 4) == 0) {
            if (size < 16) return refuse(err, "wav: fmt chunk shorter than 16 bytes");
            const uint32_t tag = le16(p + at);
            out->channels = (int)le16(p + at + 2);
            const uint32_t rate = le32(p + at + 4);
            bits = (int)le16(p + at + 14);
            if (tag == 0xFFFE) {
                if (size < 40 || le16(p + at + 24) != 1 || memcmp(p + at + 26, PCM_GUID_TAIL, 14) != 0)
                    return refuse(err, "wav: extensible format without the PCM subformat");
            } else if (tag != 1) {
                return refuse(err, "wav: format tag " + std::to_string(tag) + " (PCM only)");
            }
            if (bits != 16) return refuse(err, "wav: " + std::to_string(bits) + " bits per sample (16 only)");
            if (out->channels < 1 || out->channels > 8) return refuse(err, "wav: " + std::to_string(out->channels) + " channels (1 .. 8)");
            if (rate < 1 || rate > 0x7fffffffu) return refuse(err, "wav: sample rate " + std::to_string(rate));
            out->rate = (int)rate;
            have_fmt = true;
        } else if (memcmp(id, "data", 4) == 0) {
            if (!have_fmt) return refuse(err, "wav: data chunk before the fmt chunk");
            const size_t frame = 2 * (size_t)out->channels;
            out->n_frames = (long)(size / frame);
            if (out->n_frames < 1) return refuse(err, "wav: no audio frame");
            out->pcm.resize((size_t)out->n_frames * out->channels);
            for (size_t i = 0; i < out->pcm.size(); ++i) out->pcm[i] = (int16_t)le16(p + at + 2 * i);
            return 0;
        }
        at += size;
        if ((size & 1) && at < n) ++at;        // chunks are padded to even sizes
    }
    return refuse(err, "wav: no data chunk");
}

// "P6" / "P5", width, height, maxval 255 in decimal, separated by whitespace ('#' starts a comment to the end of the line), one
// whitespace byte, then the raster.  Sides 1 .. 65535 (what dawn_image_ingest takes); a raster shorter than the header says is refused.
inline int parse_pnm(const unsigned char* p, size_t n, Image* out, std::string* err) {
    if (n < 2 || p[0] != 'P' || (p[1] != '6' && p[1] != '5')) return refuse(err, "pnm: not a binary PPM (P6) or PGM (P5)");
    out->channels = p[1] == '6' ? 3 : 1;
    size_t at = 2;
    long v[3] = {0, 0, 0};
    for (int k = 0; k < 3; ++k) {
        for (;;) {                             // whitespace and comments in front of the number
            if (at >= n) return refuse(err, "pnm: header ends early");
            if (p[at] == '#') {
                while (at < n && p[at] != '\n') ++at;
            } else if (p[at] == ' ' || p[at] == '\t' || p[at] == '\n' || p[at] == '\r' || p[at] == '\v' || p[at] == '\f') {
                ++at;
            } else {
                break;
            }
        }
        int digits = 0;
        while (at < n && p[at] >= '0' && p[at] <= '9') {
            if (++digits > 6) return refuse(err, "pnm: a header number has more than 6 digits");
            v[k] = v[k] * 10 + (p[at++] - '0');
        }
        if (digits == 0) return refuse(err, "pnm: a header number is missing");
    }
    if (at >= n || !(p[at] == ' ' || p[at] == '\t' || p[at] == '\n' || p[at] == '\r')) return refuse(err, "pnm: no whitespace after maxval");
    ++at;
    if (v[0] < 1 || v[0] > 65535 || v[1] < 1 || v[1] > 65535) return refuse(err, "pnm: sides " + std::to_string(v[0]) + " x " + std::to_string(v[1]) + " (1 .. 65535)");
    if (v[2] != 255) return refuse(err, "pnm: maxval " + std::to_string(v[2]) + " (255 only)");
    const size_t need = (size_t)v[0] * (size_t)v[1] * (size_t)out->channels;
    if (n - at < need) return refuse(err, "pnm: raster of " + std::to_string(n - at) + " bytes, " + std::to_string(need) + " needed");
    out->width = (int)v[0];
    out->height = (int)v[1];
    out->pixels.assign(p + at, p + at + need);
    return 0;
}

// A YUV4MPEG2 (.y4m) stream of 8-bit 4:2:0 frames, as tools/dawn_generate.cpp writes them and dawn_yuv420_to_frames reads them.
//   stream header   "YUV4MPEG2" then space-separated tokens up to a newline: W<width> H<height> are required; F (rate), A (aspect) and
//                   X (comment) tokens are accepted and ignored; I = interlacing: "Ip" and "I?" only; C = colourspace: "C420",
//                   "C420jpeg", "C420mpeg2", "C420paldv" or none -- ALL taken as 8-bit 4:2:0 whose chroma sample is replicated over its
//                   2 x 2 block: the siting differences between them (a shift of at most half a pixel) are ignored.
//   frames          "FRAME", optional parameters, a newline, then W H + 2 (W/2) (H/2) bytes: Y, U, V planes (I420).
// A header line (stream or frame) longer than 256 bytes, another colourspace or bit depth, interlaced content, a W or H that the
// kernel does not take (W % 4, H % 2, 2 .. 65536), a truncated last frame, a stream without a frame: refused, the cause named.
struct Y4m {
    int width = 0, height = 0;
    long n_frames = 0;
    std::vector<unsigned char> frames;         // n_frames x (3 W H / 2) bytes, back to back
};
constexpr size_t Y4M_MAX_LINE = 256;

// the line that starts at p[at]: *end = the index of its '\n'; a line without one within Y4M_MAX_LINE bytes (or the file) is refused
inline int y4m_line(const unsigned char* p, size_t n, size_t at, const char* what, size_t* end, std::string* err) {
    for (size_t i = at; i < n; ++i) {
        if (i - at >= Y4M_MAX_LINE) return refuse(err, std::string("y4m: ") + what + " is longer than 256 bytes");
        if (p[i] == '\n') {
            *end = i;
            return 0;
        }
    }
    if (n - at >= Y4M_MAX_LINE) return refuse(err, std::string("y4m: ") + what + " is longer than 256 bytes");
    return refuse(err, std::string("y4m: ") + what + " ends early (no newline)");
}

inline int parse_y4m(const unsigned char* p, size_t n, Y4m* out, std::string* err) {
    if (n < 10 || memcmp(p, "YUV4MPEG2", 9) != 0 || (p[9] != ' ' && p[9] != '\n')) return refuse(err, "y4m: not a YUV4MPEG2 stream");
    size_t end = 0;
    if (y4m_line(p, n, 0, "the stream header", &end, err) != 0) return -1;
    long W = -1, H = -1;
    size_t at = 9;
    while (at < end) {
        if (p[at] == ' ') {
            ++at;
            continue;
        }
        size_t stop = at;
        while (stop < end && p[stop] != ' ') ++stop;
        const std::string tok((const char*)p + at, stop - at);
        at = stop;
        const std::string val = tok.substr(1);
        if (tok[0] == 'W' || tok[0] == 'H') {
            long v = 0;
            if (val.empty() || val.size() > 6) return refuse(err, "y4m: bad header token '" + tok + "'");
            for (char ch : val) {
                if (ch < '0' || ch > '9') return refuse(err, "y4m: bad header token '" + tok + "'");
                v = v * 10 + (ch - '0');
            }
            (tok[0] == 'W' ? W : H) = v;
        } else if (tok[0] == 'C') {
            if (val != "420" && val != "420jpeg" && val != "420mpeg2" && val != "420paldv")
                return refuse(err, "y4m: colourspace '" + tok + "' (8-bit 4:2:0 only: C420, C420jpeg, C420mpeg2, C420paldv)");
        } else if (tok[0] == 'I') {
            if (val != "p" && val != "?") return refuse(err, "y4m: interlacing '" + tok + "' (progressive only: Ip or I?)");
        } else if (tok[0] != 'F' && tok[0] != 'A' && tok[0] != 'X') {
            return refuse(err, "y4m: unknown header token '" + tok + "'");
        }
    }
    if (W < 0 || H < 0) return refuse(err, "y4m: the stream header lacks W or H");
    if (W < 4 || W > 65536 || W % 4 != 0) return refuse(err, "y4m: W" + std::to_string(W) + " (a multiple of 4, 4 .. 65536)");
    if (H < 2 || H > 65536 || H % 2 != 0) return refuse(err, "y4m: H" + std::to_string(H) + " (even, 2 .. 65536)");
    const size_t frame = (size_t)W * (size_t)H / 2 * 3;           // at most 3 * 2^31: fits size_t
    out->width = (int)W;
    out->height = (int)H;
    out->n_frames = 0;
    out->frames.clear();
    at = end + 1;
    while (at < n) {
        if (y4m_line(p, n, at, "a FRAME header", &end, err) != 0) return -1;
        if (end - at < 5 || memcmp(p + at, "FRAME", 5) != 0 || (end - at > 5 && p[at + 5] != ' '))
            return refuse(err, "y4m: no FRAME header where frame " + std::to_string(out->n_frames) + " starts");
        at = end + 1;
        if (n - at < frame)
            return refuse(err, "y4m: frame " + std::to_string(out->n_frames) + " is cut: " + std::to_string(n - at) + " bytes, " + std::to_string(frame) + " needed");
        out->frames.insert(out->frames.end(), p + at, p + at + frame);
        at += frame;
        ++out->n_frames;
    }
    if (out->n_frames < 1) return refuse(err, "y4m: no frame");
    return 0;
}

inline int read_file(const char* path, std::vector<unsigned char>* out, std::string* err) {
    FILE* f = fopen(path, "rb");
    if (!f) return refuse(err, std::string("cannot open '") + path + "'");
    unsigned char buf[1 << 16];
    size_t got;
    out->clear();
    while ((got = fread(buf, 1, sizeof buf, f)) > 0) out->insert(out->end(), buf, buf + got);
    fclose(f);
    return 0;
}

}  // namespace media_files
