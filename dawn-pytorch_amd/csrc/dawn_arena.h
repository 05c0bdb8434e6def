// Host-side sub-allocator shared by the C-side stage hosts (dawn_ctx.hip, dawn_decoder.hip, dawn_hubert.hip, dawn_pbnet.hip).
#pragma once
#include <stddef.h>
#include <stdint.h>
#include <iterator>
#include <map>
#include <vector>

// Host-side sub-allocator over the caller's workspace.  First fit with coalescing; `dry` = measuring pass (no base
// pointer, nothing is launched): the sequence of alloc/free calls of an evaluation is a pure function of the shapes, so
// the high-water mark of the dry pass IS the workspace requirement of the real one.
struct DawnArena {
    char* base = nullptr;
    size_t cap = 0, high = 0;
    bool dry = false, defer = false;
    std::map<size_t, size_t> freeb;          // offset -> size
    std::map<size_t, size_t> used;           // offset -> size
    std::vector<size_t> deferred;
    void reset(void* b, size_t c, bool d) {
        base = (char*)b; cap = c; dry = d; high = 0; defer = false;
        freeb.clear(); used.clear(); deferred.clear();
        freeb[0] = d ? ((size_t)1 << 62) : c;
    }
    void* alloc(size_t bytes) {
        bytes = (bytes + 255) & ~(size_t)255;
        if (bytes == 0) bytes = 256;
        for (auto it = freeb.begin(); it != freeb.end(); ++it) {
            if (it->second >= bytes) {
                const size_t off = it->first, sz = it->second;
                freeb.erase(it);
                if (sz > bytes) freeb[off + bytes] = sz - bytes;
                used[off] = bytes;
                if (off + bytes > high) high = off + bytes;
                return dry ? (void*)(uintptr_t)(off + 4096) : (void*)(base + off);   // dry: fake non-null addresses
            }
        }
        return nullptr;
    }
    void release_off(size_t off) {
        auto u = used.find(off);
        if (u == used.end()) return;
        size_t sz = u->second;
        used.erase(u);
        auto nx = freeb.lower_bound(off);
        if (nx != freeb.end() && off + sz == nx->first) { sz += nx->second; nx = freeb.erase(nx); }
        if (nx != freeb.begin()) {
            auto pv = std::prev(nx);
            if (pv->first + pv->second == off) { pv->second += sz; return; }
        }
        freeb[off] = sz;
    }
    void free(const void* p) {
        if (!p) return;
        const size_t off = dry ? (size_t)((uintptr_t)p - 4096) : (size_t)((const char*)p - base);
        if (defer) deferred.push_back(off);       // buffers released inside a side-stream region: reusable after the join
        else release_off(off);
    }
    void flush_deferred() {
        for (size_t o : deferred) release_off(o);
        deferred.clear();
    }
};
