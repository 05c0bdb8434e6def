// Host program: prices every LDS access site of the window-tiled fused temporal layer (csrc/temporal_layer16.hip) with the per-instruction
// bank model of gfx950's LDS, from the byte offsets the kernels themselves use (csrc/temporal_layer16.h).
//
//     g++ -std=c++17 -O1 -I dawn-pytorch_amd/csrc tools/tl16_lds_banks.cpp -o tl16_lds_banks
//     tl16_lds_banks [--layout current|parent] [--waves 13|8] [--shape Fext q0 Fq win HW]... [--offsets]
//
// The model (per wave-instruction; only lanes of one group can conflict, equal dword addresses broadcast, N distinct dwords on one bank
// of a group take N LDS cycles instead of 1 -- the extra cycles are what SQ_LDS_BANK_CONFLICT counts, all cycles SQ_LDS_IDX_ACTIVE):
//     ds_read_b32 / ds_write_b32   2 groups {0-31} {32-63}                                   bank = (a / 4) mod 32
//     ds_read_b64                  2 groups {0-31} {32-63}                                   bank = (a / 4) mod 64
//     ds_read_b128                 4 groups {0-3,12-15,20-27} {4-11,16-19,28-31} (+32 twice)  bank = (a / 4) mod 64
//     ds_read2_b64                 two accesses, each 4 groups of 16 consecutive lanes        bank = (a / 4) mod 32
//     ds_write_b64                 4 groups of 16 consecutive lanes                           bank = (a / 4) mod 32
// (the compiler pairs some 8-byte stores into ds_write2[st64]_b64: two ds_write_b64 accesses, priced as such).
//
// `--layout parent` prices the layout this one replaced (bias-table copies 132 floats apart, V^T fragment halves fetched by one
// ds_read2_b64); below the table the alternatives that were weighed are priced too.  Lines starting with SITE / OFF are for tests.
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <functional>
#include <map>
#include <set>
#include <string>
#include <vector>

#include "temporal_layer16.h"

namespace {

enum Kind { READ_B32, READ_B64, READ_B128, READ2_B64_HALF, WRITE_B32, WRITE_B64 };
const char* kind_name(Kind k) {
    switch (k) {
        case READ_B32: return "ds_read_b32";
        case READ_B64: return "ds_read_b64";
        case READ_B128: return "ds_read_b128";
        case READ2_B64_HALF: return "ds_read2_b64 (one of its two accesses)";
        case WRITE_B32: return "ds_write_b32";
        default: return "ds_write_b64";
    }
}
int kind_bytes(Kind k) { return k == READ_B32 || k == WRITE_B32 ? 4 : k == READ_B128 ? 16 : 8; }
int kind_banks(Kind k) { return k == READ_B64 || k == READ_B128 ? 64 : 32; }
int kind_groups(Kind k) { return k == READ_B32 || k == READ_B64 || k == WRITE_B32 ? 2 : 4; }
int lane_group(Kind k, int lane) {
    if (kind_groups(k) == 2) return lane >> 5;
    if (k == READ_B128) {
        const int l = lane & 31;
        const bool first = l < 4 || (l >= 12 && l < 16) || (l >= 20 && l < 28);
        return 2 * (lane >> 5) + (first ? 0 : 1);
    }
    return lane >> 4;
}

// one wave-instruction: byte address per lane, -1 = lane inactive.  Returns the LDS cycles beyond one per group.
int extra_cycles(Kind k, const int (&addr)[64]) {
    const int nb = kind_banks(k), dw = kind_bytes(k) / 4;
    int extra = 0;
    for (int grp = 0; grp < kind_groups(k); ++grp) {
        std::map<int, std::set<int>> bank;                      // bank -> distinct dword addresses
        for (int l = 0; l < 64; ++l) {
            if (addr[l] < 0 || lane_group(k, l) != grp) continue;
            for (int d = 0; d < dw; ++d) bank[(addr[l] / 4 + d) % nb].insert(addr[l] / 4 + d);
        }
        size_t ways = 1;
        for (const auto& b : bank) ways = std::max(ways, b.second.size());
        extra += (int)ways - 1;
    }
    return extra;
}

struct Site {
    std::string name;
    Kind kind;
    long instrs = 0, extra = 0;      // per workgroup
    int worst = 0;
};

struct Layout {
    int band_stride;
    bool vt_read2;                   // V^T fragment halves by one ds_read2_b64 (else two ds_read_b64)
};
struct Shape { int Fext, q0, Fq, win, HW; };

using AddrFn = std::function<int(int lane)>;
void issue(Site& s, long times, const AddrFn& f) {
    int a[64];
    for (int l = 0; l < 64; ++l) a[l] = f(l);
    const int e = extra_cycles(s.kind, a);
    s.instrs += times;
    s.extra += times * e;
    s.worst = std::max(s.worst, e);
}

// Every LDS wave-instruction of one workgroup (one pixel column), by site.  waves = 13 (temporal_layer13_kernel) or 8.
std::vector<Site> price(const Shape& sh, const Layout& lay, int waves, bool vt_image = false, bool k_split = false) {
    const int FA = TL16_ROWS, HEADS = 8;
    const int nblk = (sh.Fext + 15) >> 4, nkb = (16 + 2 * sh.win + 15) >> 4;
    const int delta = (((sh.q0 - sh.win) % 16) + 16) % 16;
    const int nqt = (sh.Fq + delta + 15) / 16;
    auto band_read = [&](int n, int g, int blk) {                       // tl16_band_read_idx at the layout's stride
        return ((15 - n) & 3) * lay.band_stride + ((15 - n) & ~3) + 4 * g + 16 * blk;
    };
    std::vector<Site> S = {{"X planes: store (phase 0)", WRITE_B64},      {"X planes: read, query rows", READ_B128},
                           {"X planes: read, K/V projection", READ_B128}, {"K planes: store", WRITE_B64},
                           {"V^T: store", WRITE_B64},                     {"bias table: store", WRITE_B32},
                           {"bias table: read", READ_B128},               {"K planes: read", k_split ? READ_B64 : READ_B128},
                           {"V^T: read", lay.vt_read2 || vt_image ? READ2_B64_HALF : READ_B64}};
    enum { XST, XRQ, XRK, KST, VST, BST, BRD, KRD, VRD };
    // phase 0: 16 lanes per row, rows (tid >> 4) + (threads / 16) . pass; three plane stores each
    const int rpp = waves * 4;
    for (int w = 0; w < waves; ++w)
        for (int pass = 0; pass * rpp < FA; ++pass)
            issue(S[XST], 3, [&](int l) {
                const int tid = 64 * w + l, sub = tid & 15, j = (tid >> 4) + rpp * pass;
                return j < FA ? TL16_X_BASE + tl16_x_off(0, sub >> 1, j, sub & 1) : -1;
            });
    // K / V projection: every (K | V, feature half) combination reads all row tiles; K and V each store two halves per row tile
    for (int rt = 0; rt < nblk; ++rt) {
        for (int s = 0; s < 2; ++s)
            issue(S[XRK], 4L * 3 * HEADS, [&](int l) { return TL16_X_BASE + tl16_x_off(0, (l >> 4) + 4 * s, 16 * rt + (l & 15), 0); });
        for (int half = 0; half < 2; ++half) {
            issue(S[KST], 3L * HEADS, [&](int l) {
                if (k_split) return TL16_K_BASE + (((half * 4) + (l >> 4)) * FA + 16 * rt + (l & 15)) * 8;
                return TL16_K_BASE + tl16_k_off(0, l >> 4, 16 * rt + (l & 15), half);
            });
            issue(S[VST], 3L * HEADS, [&](int l) { return TL16_V_BASE + tl16_v_off(0, half, l, rt); });
        }
    }
    for (int w = 0; w < 8; ++w)                                        // threads 0..511 write the head's table
        issue(S[BST], HEADS, [&](int l) {
            const int tid = 64 * w + l;
            return (tid & 127) < lay.band_stride ? TL16_BAND_BASE + 4 * ((tid >> 7) * lay.band_stride + (tid & 127)) : -1;
        });
    // the query tiles
    for (int t = 0; t < nqt; ++t) {
        const int i0 = sh.q0 - delta + 16 * t;
        const int B0 = (i0 - sh.win) >> 4;
        const int blo = std::max(0, -B0), bhi = std::min(nkb, nblk - B0), Bf = B0 + blo, NV = bhi - blo, NP = (NV + 1) / 2;
        for (int s = 0; s < 2; ++s)
            issue(S[XRQ], 3L * HEADS, [&](int l) {
                const int row = std::max(0, std::min(i0 + (l & 15), sh.Fext - 1));
                return TL16_X_BASE + tl16_x_off(0, (l >> 4) + 4 * s, row, 0);
            });
        for (int j = 0; j < NV; ++j) {
            issue(S[BRD], HEADS, [&](int l) { return TL16_BAND_BASE + 4 * band_read(l & 15, l >> 4, blo + j); });
            if (k_split) {
                for (int half = 0; half < 2; ++half)
                    issue(S[KRD], 3L * HEADS, [&](int l) { return TL16_K_BASE + (((half * 4) + (l >> 4)) * FA + 16 * (Bf + j) + (l & 15)) * 8; });
            } else
                issue(S[KRD], 3L * HEADS, [&](int l) { return TL16_K_BASE + tl16_k_off(0, l >> 4, 16 * (Bf + j) + (l & 15), 0); });
        }
        for (int kk = 0; kk < NP; ++kk)
            for (int mb = 0; mb < 2; ++mb)
                for (int part = 0; part < 2; ++part) {
                    const int blk = Bf + (part == 0 || 2 * kk + 1 >= NV ? 2 * kk : 2 * kk + 1);
                    issue(S[VRD], 3L * HEADS, [&](int l) {
                        if (vt_image) return TL16_V_BASE + ((mb * TL16_BLOCKS + blk) * 64 + l) * 8;      // [block][lane] x 8 B
                        return TL16_V_BASE + tl16_v_off(0, mb, l, blk);
                    });
                }
    }
    return S;
}

// LDS-array cycles of a conflict-free wave-instruction
int base_cycles(Kind k) { return kind_groups(k); }

void report(const Shape& sh, const Layout& lay, const char* layname, int waves) {
    const std::vector<Site> S = price(sh, lay, waves);
    std::printf("\n## layout %s, %d waves, Fext %d q0 %d Fq %d win %d, %d pixel columns\n", layname, waves, sh.Fext, sh.q0, sh.Fq, sh.win, sh.HW);
    std::printf("| site | instruction | accesses / workgroup | LDS cycles each, conflict-free | extra cycles each (worst) | extra / workgroup | extra / launch |\n|---|---|---|---|---|---|---|\n");
    long tot = 0, cyc = 0;
    for (const Site& s : S) {
        std::printf("| %s | %s | %ld | %d | %.2f (%d) | %ld | %.3e |\n", s.name.c_str(), kind_name(s.kind), s.instrs, base_cycles(s.kind),
                    s.instrs ? (double)s.extra / s.instrs : 0.0, s.worst, s.extra, (double)s.extra * sh.HW);
        tot += s.extra;
        cyc += s.instrs * base_cycles(s.kind) + s.extra;
    }
    std::printf("| total | | | | | %ld | %.3e |\n", tot, (double)tot * sh.HW);
    std::printf("predicted SQ_LDS_BANK_CONFLICT %.4e, SQ_LDS_IDX_ACTIVE %.4e per launch\n", (double)tot * sh.HW, (double)cyc * sh.HW);
    for (const Site& s : S)
        std::printf("SITE %s %d %d:%d:%d:%d \"%s\" %ld %ld %ld\n", layname, waves, sh.Fext, sh.q0, sh.Fq, sh.win, s.name.c_str(), s.instrs,
                    s.instrs * base_cycles(s.kind), s.extra);
}

void alternatives(const Shape& sh, const Layout& cur) {
    std::printf("\n## alternatives weighed (13 waves, Fext %d q0 %d Fq %d win %d): LDS cycles per workgroup = accesses x cycles + extra\n", sh.Fext, sh.q0, sh.Fq, sh.win);
    auto line = [&](const char* what, const Site& s) {
        std::printf("| %s | %s | %ld | %ld | %ld |\n", what, kind_name(s.kind), s.instrs, s.instrs * base_cycles(s.kind) + s.extra, s.extra);
    };
    std::printf("| option | instruction | accesses | LDS cycles | of them extra |\n|---|---|---|---|---|\n");
    Layout l2 = cur;
    l2.vt_read2 = true;
    line("V^T read, [lane][block] image, one ds_read2_b64 per fragment", price(sh, l2, 13)[8]);
    line("V^T read, [block][lane] image, one ds_read2_b64 per fragment", price(sh, l2, 13, true)[8]);
    l2.vt_read2 = false;
    line("V^T read, [lane][block] image, two ds_read_b64 per fragment", price(sh, l2, 13)[8]);
    for (int stride : {128, 132, 112, 144}) {
        Layout l3 = cur;
        l3.band_stride = stride;
        char buf[96];
        std::snprintf(buf, sizeof buf, "bias table read, copies %d floats apart%s", stride, stride == 144 ? " (does not fit the LDS size)" : "");
        line(buf, price(sh, l3, 13)[6]);
    }
    line("K planes store, [plane][k-group][row] x 16 B (two halves per row)", price(sh, cur, 13)[3]);
    line("K planes read, the same: one ds_read_b128 per fragment", price(sh, cur, 13)[7]);
    line("K planes store, [plane][half][k-group][row] x 8 B", price(sh, cur, 13, false, true)[3]);
    line("K planes read, the same: two ds_read_b64 per fragment", price(sh, cur, 13, false, true)[7]);
}

void offsets() {
    // the helpers' values for a sample of lanes and indices: tests compare them with the documented layouts
    for (int pl = 0; pl < 3; ++pl)
        for (int o : {0, 3, 7})
            for (int row : {0, 17, 207})
                for (int h = 0; h < 2; ++h) std::printf("OFF x %d %d %d %d %d\n", pl, o, row, h, TL16_X_BASE + tl16_x_off(pl, o, row, h));
    for (int pl = 0; pl < 3; ++pl)
        for (int g = 0; g < 4; ++g)
            for (int row : {0, 17, 207})
                for (int h = 0; h < 2; ++h) std::printf("OFF k %d %d %d %d %d\n", pl, g, row, h, TL16_K_BASE + tl16_k_off(pl, g, row, h));
    for (int pl = 0; pl < 3; ++pl)
        for (int mb = 0; mb < 2; ++mb)
            for (int lane : {0, 5, 31, 63})
                for (int blk : {0, 6, 12}) std::printf("OFF v %d %d %d %d %d\n", pl, mb, lane, blk, TL16_V_BASE + tl16_v_off(pl, mb, lane, blk));
    for (int lane = 0; lane < 64; lane += 3)
        for (int blk : {0, 5}) std::printf("OFF band %d %d %d 0 %d\n", lane & 15, lane >> 4, blk, TL16_BAND_BASE + 4 * tl16_band_read_idx(lane & 15, lane >> 4, blk));
}

}  // namespace

int main(int argc, char** argv) {
    const Layout current = {TL16_BAND_STRIDE, false}, parent = {132, true};
    std::vector<Shape> shapes;
    std::vector<int> waves;
    std::vector<std::string> layouts;
    bool offs = false;
    for (int i = 1; i < argc; ++i) {
        if (!std::strcmp(argv[i], "--offsets")) offs = true;
        else if (!std::strcmp(argv[i], "--layout") && i + 1 < argc) layouts.push_back(argv[++i]);
        else if (!std::strcmp(argv[i], "--waves") && i + 1 < argc) waves.push_back(std::atoi(argv[++i]));
        else if (!std::strcmp(argv[i], "--shape") && i + 5 < argc) {
            shapes.push_back({std::atoi(argv[i + 1]), std::atoi(argv[i + 2]), std::atoi(argv[i + 3]), std::atoi(argv[i + 4]), std::atoi(argv[i + 5])});
            i += 5;
        } else {
            std::fprintf(stderr, "usage: %s [--layout current|parent]... [--waves 13|8]... [--shape Fext q0 Fq win HW]... [--offsets]\n", argv[0]);
            return 2;
        }
    }
    if (offs) {
        offsets();
        return 0;
    }
    if (shapes.empty()) shapes = {{200, 0, 200, 40, 4096}, {200, 0, 200, 40, 1024}};       // the benchmark's 64-channel levels
    if (waves.empty()) waves = {13, 8};
    if (layouts.empty()) layouts = {"parent", "current"};
    for (const Shape& sh : shapes) {
        if (sh.Fext < 1 || sh.Fext > TL16_ROWS || sh.q0 < 0 || sh.Fq < 1 || sh.q0 + sh.Fq > sh.Fext || sh.win < 0 || 16 + 2 * sh.win > 16 * TL16_KEY_BLOCKS) {
            std::fprintf(stderr, "shape outside the kernels' instantiation\n");
            return 2;
        }
        for (int w : waves)
            for (const std::string& l : layouts) {
                if ((w != 13 && w != 8) || (l != "parent" && l != "current")) {
                    std::fprintf(stderr, "--waves 13|8, --layout current|parent\n");
                    return 2;
                }
                report(sh, l == "parent" ? parent : current, l.c_str(), w);
            }
    }
    alternatives(shapes[0], current);
    return 0;
}
