// Host-side plumbing shared by the C-side stage hosts (dawn_ctx.hip, dawn_decoder.hip, dawn_hubert.hip, dawn_pbnet.hip, dawn_motion.hip): the
// return-code macro, the workspace arithmetic and refusals, and the named-weight table a *_create reads its pointers from.
// Header only, internal linkage throughout: the library's symbol table gains nothing from it.
#pragma once
#include "dawn_common.h"
#include "dawn_arena.h"
#include "../../include/dawn_hip.h"

#include <stdio.h>
#include <string>

#define CK(expr)                              \
    do {                                      \
        const int rc__ = (expr);              \
        if (rc__ != 0) return rc__;           \
    } while (0)

// `float* ptr` of `floats` floats from the arena, or the caller's refusal (a dry pass never runs out)
#define DAWN_ALLOC(arena, ptr, floats, code, msg)                \
    float* ptr = (float*)(arena).alloc((size_t)(floats) * 4);    \
    if (!ptr) return dawn_set_error_msg(code, msg)

namespace {

inline size_t a256(size_t b) { return (b + 255) & ~(size_t)255; }

inline bool overlaps(const void* a, size_t an, const void* b, size_t bn) {
    const uintptr_t x = (uintptr_t)a, y = (uintptr_t)b;
    return x < y + bn && y < x + an;
}

// "<who>: workspace of <have> bytes, <need> needed (<query>)" under the caller's code; query = the entry point that sizes it
inline int refuse_workspace(int code, const char* who, size_t have, size_t need, const char* query) {
    char m[240];
    snprintf(m, sizeof m, "%s: workspace of %zu bytes, %zu needed (%s)", who, have, need, query);
    return dawn_set_error_msg(code, m);
}

// The caller's dawn_named_ptr table by name, for the life of one *_create (it reads the caller's array in place: a lookup is a scan,
// a few thousand names at the most).  `missing` is the creator's text in front of the quoted name ("dawn_x_create: missing packed
// weight"); the FIRST required name that is absent or NULL is the one reported, under `code`.
class DawnWeights {
    const dawn_named_ptr* table_;
    int n_;
    const char* missing_;
    int code_;
    bool ok_ = true;

public:
    DawnWeights(const dawn_named_ptr* table, int n, const char* missing, int code) : table_(table), n_(n), missing_(missing), code_(code) {}
    const void* opt(const std::string& k) const {
        for (int i = n_ - 1; i >= 0; --i)          // entries without a name are skipped; of a name given twice the last one counts
            if (table_[i].name && k == table_[i].name) return table_[i].ptr;
        return nullptr;
    }
    const void* get(const std::string& k) {
        const void* p = opt(k);
        if (!p && ok_) {
            ok_ = false;
            dawn_set_error_msg(code_, (std::string(missing_) + " '" + k + "'").c_str());
        }
        return p;
    }
    const float* getf(const std::string& k) { return (const float*)get(k); }
    bool ok() const { return ok_; }
    int code() const { return code_; }
};

}  // namespace
