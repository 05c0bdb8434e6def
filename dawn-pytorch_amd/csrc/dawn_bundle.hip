// The model bundle loader (include/dawn_hip.h: "model bundle"): open / upload / verify / tables / handles.  The file format and every
// refusal of it live in dawn_bundle_format.h (host code without HIP, shared with tools/); this unit adds the one kernel -- the checksum
// of the uploaded tensors -- the upload through the library's own bounded staging, and the glue to the six *_create calls (and to the
// optional seventh, dawn_motion_create).
#include "dawn_host.h"
#include "dawn_bundle_format.h"

#include <memory>

namespace fmt = dawn_bundle_format;

namespace {

// ---------------------------------------------------------------------------------------------------------------- the checksum kernel
// One workgroup per work item: words [first, first + n) of the tensor at `offset` bytes of the region.  `first` is a multiple of
// ITEM_WORDS and a tensor starts at a multiple of 256 bytes, so an item starts 16-byte aligned: whole 16-byte loads, then up to three
// single words.  With j the index inside the item: s1 = sum w, s2 = (first + 1) s1 + sum j w, where j w < 2^48 and the running sum
// wraps mod 2^64 like every other term; integers only, so neither the lane a word lands in nor the order of the adds matters.
constexpr int CK_THREADS = 256;
constexpr unsigned ITEM_WORDS = 65536;              // 256 KiB per item: 64 16-byte loads per lane
constexpr size_t MAX_ITEMS_PER_LAUNCH = 1u << 20;

struct WorkItem {
    unsigned long long offset;                      // bytes from the region base to the item's first word
    unsigned long long first;                       // index of that word inside its tensor
    unsigned n;                                     // words, 1 .. ITEM_WORDS
    unsigned tensor;                                // (host bookkeeping: index into the device-tensor list)
};
static_assert(sizeof(WorkItem) == 24, "work list layout");

__device__ __forceinline__ unsigned long long wave_sum_u64(unsigned long long v) {
#pragma unroll
    for (int o = 32; o >= 1; o >>= 1) v += __shfl_xor(v, o, 64);
    return v;
}

__global__ __launch_bounds__(CK_THREADS) void bundle_checksum_kernel(const unsigned char* __restrict__ base, const WorkItem* __restrict__ items,
                                                                     ulonglong2* __restrict__ partials) {
    const WorkItem it = items[blockIdx.x];
    const unsigned* w = (const unsigned*)(base + it.offset);
    const unsigned quads = it.n >> 2;
    unsigned long long a = 0, b = 0;
#pragma unroll 4
    for (unsigned q = threadIdx.x; q < quads; q += CK_THREADS) {
        const u32x4 v = *(const u32x4*)(w + 4 * (size_t)q);
        const unsigned j = 4 * q;
        a += (unsigned long long)v[0] + v[1] + v[2] + v[3];
        b += (unsigned long long)j * v[0] + (unsigned long long)(j + 1) * v[1] + (unsigned long long)(j + 2) * v[2] +
             (unsigned long long)(j + 3) * v[3];
    }
    const unsigned tail = 4 * quads + threadIdx.x;  // the last n % 4 words: lanes 0 .. 2
    if (tail < it.n) {
        const unsigned v = w[tail];
        a += v;
        b += (unsigned long long)tail * v;
    }
    a = wave_sum_u64(a);
    b = wave_sum_u64(b);
    __shared__ unsigned long long sa[CK_THREADS / DAWN_WAVE], sb[CK_THREADS / DAWN_WAVE];
    if ((threadIdx.x & (DAWN_WAVE - 1)) == 0) {
        sa[threadIdx.x / DAWN_WAVE] = a;
        sb[threadIdx.x / DAWN_WAVE] = b;
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        unsigned long long s1 = 0, sj = 0;
#pragma unroll
        for (int i = 0; i < CK_THREADS / DAWN_WAVE; ++i) { s1 += sa[i]; sj += sb[i]; }
        partials[blockIdx.x] = ulonglong2{s1, sj + (it.first + 1) * s1};
    }
}

constexpr size_t STAGING_BYTES = 8u << 20;

int refuse(int code, const char* who, const std::string& what) { return dawn_set_error_msg(code, (std::string(who) + ": " + what).c_str()); }

// a stage with a weight table and a cfg struct: everything but the host stage
bool model_stage(int stage) { return stage >= 0 && stage < fmt::N_STAGES && stage != fmt::STAGE_HOST; }

}  // namespace

struct dawn_bundle {
    std::string path;
    fmt::Bundle f;
    std::vector<const fmt::Entry*> tensors;                         // device tensors, index order
    std::vector<WorkItem> items;
    std::vector<dawn_named_ptr> tables[fmt::N_STAGES];
    size_t items_bytes() const { return a256(items.size() * sizeof(WorkItem)); }
    const fmt::Entry* find(uint32_t stage, uint32_t kind, const char* name) const {
        for (const fmt::Entry& e : f.entries)
            if (e.stage == stage && e.kind == kind && e.name == name) return &e;
        return nullptr;
    }
};

extern "C" int dawn_bundle_open(const char* path, dawn_bundle** out) {
    if (!path || !out) return dawn_set_error_msg(-350, "dawn_bundle_open: NULL argument");
    std::unique_ptr<dawn_bundle> b(new dawn_bundle);
    b->path = path;
    std::string err;
    if (fmt::open_file(path, (uint32_t)dawn_abi_version(), &b->f, &err) != 0) return refuse(-351, "dawn_bundle_open", err);
    for (const fmt::Entry& e : b->f.entries) {
        if (e.kind != fmt::KIND_DEVICE) continue;
        const unsigned t = (unsigned)b->tensors.size();
        b->tensors.push_back(&e);
        const uint64_t words = e.length / 4;
        for (uint64_t first = 0; first < words; first += ITEM_WORDS)
            b->items.push_back(WorkItem{e.offset + 4 * first, first, (unsigned)std::min<uint64_t>(ITEM_WORDS, words - first), t});
    }
    *out = b.release();
    return 0;
}

extern "C" void dawn_bundle_close(dawn_bundle* b) { delete b; }

extern "C" size_t dawn_bundle_device_bytes(const dawn_bundle* b) { return b ? (size_t)b->f.h.device_bytes : 0; }

extern "C" size_t dawn_bundle_verify_workspace_bytes(const dawn_bundle* b) {
    return b ? std::max<size_t>(256, b->items_bytes() + a256(b->items.size() * sizeof(ulonglong2))) : 0;
}

namespace {

int region_check(const dawn_bundle* b, const void* device_mem, size_t bytes, const char* who) {
    if (!b || !device_mem) return refuse(-350, who, "NULL argument");
    if (((uintptr_t)device_mem & 255) != 0) return refuse(-352, who, "device_mem is not 256-byte aligned");
    if (bytes < b->f.h.device_bytes)
        return refuse(-353, who, "device memory of " + fmt::u64s(bytes) + " bytes, " + fmt::u64s(b->f.h.device_bytes) + " needed (dawn_bundle_device_bytes)");
    return 0;
}

struct Staging {                                                    // two pinned buffers and their "copy done" events
    void* buf[2] = {nullptr, nullptr};
    hipEvent_t ev[2] = {nullptr, nullptr};
    FILE* file = nullptr;
    ~Staging() {
        for (int i = 0; i < 2; ++i) {
            if (ev[i]) (void)hipEventDestroy(ev[i]);
            if (buf[i]) (void)hipHostFree(buf[i]);
        }
        if (file) fclose(file);
    }
};

}  // namespace

extern "C" int dawn_bundle_upload(dawn_bundle* b, void* device_mem, size_t bytes, void* stream) {
    const char* who = "dawn_bundle_upload";
    CK(region_check(b, device_mem, bytes, who));
    const hipStream_t st = (hipStream_t)stream;
    const uint64_t total = b->f.h.device_bytes;
    if (total == 0) return 0;
    Staging s;
    s.file = fopen(b->path.c_str(), "rb");
    uint64_t size = 0;
    if (!s.file || !fmt::file_size(s.file, &size)) return refuse(-354, who, "cannot open '" + b->path + "'");
    if (size != b->f.h.file_bytes) return refuse(-354, who, "the file changed since dawn_bundle_open: " + fmt::u64s(size) + " bytes, " + fmt::u64s(b->f.h.file_bytes) + " then");
    if (fseeko(s.file, (off_t)b->f.h.payload_offset, SEEK_SET) != 0) return refuse(-354, who, "cannot seek to the payload");
    const size_t chunk = (size_t)std::min<uint64_t>(STAGING_BYTES, total);
    for (int i = 0; i < 2; ++i) {
        hipError_t e = hipHostMalloc(&s.buf[i], chunk, hipHostMallocDefault);
        if (e == hipSuccess) e = hipEventCreateWithFlags(&s.ev[i], hipEventDisableTiming);
        if (e != hipSuccess) return dawn_set_error(e, __FILE__, __LINE__);
    }
    uint64_t done = 0;
    for (int i = 0; done < total; ++i) {
        const int k = i & 1;
        const size_t n = (size_t)std::min<uint64_t>(chunk, total - done);
        hipError_t e = i >= 2 ? hipEventSynchronize(s.ev[k]) : hipSuccess;          // the buffer's previous copy has left it
        if (e != hipSuccess) return dawn_set_error(e, __FILE__, __LINE__);
        if (fread(s.buf[k], 1, n, s.file) != n) {
            (void)hipStreamSynchronize(st);
            return refuse(-354, who, "short read of the device part at payload byte " + fmt::u64s(done));
        }
        e = hipMemcpyAsync((unsigned char*)device_mem + done, s.buf[k], n, hipMemcpyHostToDevice, st);
        if (e == hipSuccess) e = hipEventRecord(s.ev[k], st);
        if (e != hipSuccess) {
            (void)hipStreamSynchronize(st);
            return dawn_set_error(e, __FILE__, __LINE__);
        }
        done += n;
    }
    const hipError_t e = hipStreamSynchronize(st);
    if (e != hipSuccess) return dawn_set_error(e, __FILE__, __LINE__);
    return 0;
}

extern "C" int dawn_bundle_verify(dawn_bundle* b, const void* device_mem, size_t bytes, void* workspace, size_t workspace_bytes, void* stream) {
    const char* who = "dawn_bundle_verify";
    CK(region_check(b, device_mem, bytes, who));
    const size_t need = dawn_bundle_verify_workspace_bytes(b);
    if (!workspace) return refuse(-350, who, "NULL workspace");
    if (((uintptr_t)workspace & 15) != 0) return refuse(-352, who, "workspace is not 16-byte aligned");
    if (workspace_bytes < need) return refuse_workspace(-355, who, workspace_bytes, need, "dawn_bundle_verify_workspace_bytes");
    if (overlaps(device_mem, (size_t)b->f.h.device_bytes, workspace, need)) return refuse(-356, who, "the workspace overlaps the device memory");
    const size_t n = b->items.size();
    if (n == 0) return 0;
    const hipStream_t st = (hipStream_t)stream;
    WorkItem* d_items = (WorkItem*)workspace;
    ulonglong2* d_part = (ulonglong2*)((unsigned char*)workspace + b->items_bytes());
    hipError_t e = hipMemcpyAsync(d_items, b->items.data(), n * sizeof(WorkItem), hipMemcpyHostToDevice, st);
    if (e != hipSuccess) return dawn_set_error(e, __FILE__, __LINE__);
    for (size_t i0 = 0; i0 < n; i0 += MAX_ITEMS_PER_LAUNCH) {
        const size_t cnt = std::min(MAX_ITEMS_PER_LAUNCH, n - i0);
        hipLaunchKernelGGL(bundle_checksum_kernel, dim3((unsigned)cnt), dim3(CK_THREADS), 0, st, (const unsigned char*)device_mem, d_items + i0,
                           d_part + i0);
        DAWN_LAUNCH_CHECK();
    }
    std::vector<ulonglong2> part(n);
    e = hipMemcpyAsync(part.data(), d_part, n * sizeof(ulonglong2), hipMemcpyDeviceToHost, st);
    if (e == hipSuccess) e = hipStreamSynchronize(st);
    if (e != hipSuccess) return dawn_set_error(e, __FILE__, __LINE__);
    std::vector<uint64_t> s1(b->tensors.size(), 0), s2(b->tensors.size(), 0);
    for (size_t i = 0; i < n; ++i) {
        s1[b->items[i].tensor] += part[i].x;
        s2[b->items[i].tensor] += part[i].y;
    }
    for (size_t t = 0; t < b->tensors.size(); ++t) {
        const fmt::Entry& en = *b->tensors[t];
        if (s1[t] != en.s1 || s2[t] != en.s2)
            return refuse(-357, who, std::string("checksum mismatch in stage '") + fmt::stage_name(en.stage) + "', tensor '" + en.name + "'");
    }
    return 0;
}

extern "C" int dawn_bundle_table(dawn_bundle* b, int stage, const void* device_mem, const dawn_named_ptr** table, int* n) {
    const char* who = "dawn_bundle_table";
    if (!b || !device_mem || !table || !n) return refuse(-350, who, "NULL argument");
    if (!model_stage(stage)) return refuse(-358, who, "stage " + std::to_string(stage) + ": 0 .. 5, or 7 (motion)");
    std::vector<dawn_named_ptr>& t = b->tables[stage];
    t.clear();
    for (const fmt::Entry* e : b->tensors)
        if (e->stage == (uint32_t)stage) t.push_back(dawn_named_ptr{e->name.c_str(), (const unsigned char*)device_mem + e->offset});
    *table = t.data();
    *n = (int)t.size();
    return 0;
}

extern "C" int dawn_bundle_cfg(const dawn_bundle* b, int stage, void* out, size_t out_bytes) {
    const char* who = "dawn_bundle_cfg";
    if (!b || !out) return refuse(-350, who, "NULL argument");
    if (!model_stage(stage)) return refuse(-358, who, "stage " + std::to_string(stage) + ": 0 .. 5, or 7 (motion)");
    const fmt::Entry* e = b->find((uint32_t)stage, fmt::KIND_HOST, "cfg");
    if (!e) return refuse(-359, who, std::string("stage '") + fmt::stage_name((uint32_t)stage) + "' is missing from the bundle (no cfg)");
    if (out_bytes != e->length) return refuse(-360, who, std::string("stage '") + fmt::stage_name((uint32_t)stage) + "': out_bytes = " + fmt::u64s(out_bytes) + ", the struct has " + fmt::u64s(e->length));
    memcpy(out, b->f.host_blob(*e), (size_t)e->length);
    return 0;
}

extern "C" int dawn_bundle_host(const dawn_bundle* b, const char* name, const void** ptr, size_t* bytes) {
    const char* who = "dawn_bundle_host";
    if (!b || !name || !ptr || !bytes) return refuse(-350, who, "NULL argument");
    const fmt::Entry* e = b->find(fmt::STAGE_HOST, fmt::KIND_HOST, name);
    if (!e) return refuse(-361, who, std::string("no host blob '") + name + "' in the bundle");
    *ptr = b->f.host_blob(*e);
    *bytes = (size_t)e->length;
    return 0;
}

extern "C" void dawn_bundle_destroy_handles(dawn_generate_args* a) {
    if (!a) return;
    dawn_hubert_destroy(a->hubert);
    dawn_pbnet_destroy(a->pose);
    dawn_pbnet_destroy(a->blink);
    dawn_decoder_destroy(a->decoder);
    dawn_inputs_destroy(a->inputs);
    dawn_ctx_destroy(a->unet);
    a->hubert = nullptr; a->pose = nullptr; a->blink = nullptr; a->decoder = nullptr; a->inputs = nullptr; a->unet = nullptr;
}

extern "C" int dawn_bundle_create_handles(dawn_bundle* b, const void* device_mem, dawn_generate_args* args) {
    const char* who = "dawn_bundle_create_handles";
    if (!b || !device_mem || !args) return refuse(-350, who, "NULL argument");
    dawn_generate_args h;
    memset(&h, 0, sizeof h);
    dawn_hubert_cfg c_hub; dawn_pbnet_cfg c_pose, c_blink; dawn_decoder_cfg c_dec; dawn_inputs_cfg c_in; dawn_unet_cfg c_unet;
    void* const cfgs[6] = {&c_hub, &c_pose, &c_blink, &c_dec, &c_in, &c_unet};
    const size_t sizes[6] = {sizeof c_hub, sizeof c_pose, sizeof c_blink, sizeof c_dec, sizeof c_in, sizeof c_unet};
    const dawn_named_ptr* tab[6];
    int n[6];
    for (int s = 0; s < 6; ++s) {                                   // every stage is looked up before the first handle is made
        CK(dawn_bundle_cfg(b, s, cfgs[s], sizes[s]));
        CK(dawn_bundle_table(b, s, device_mem, &tab[s], &n[s]));
    }
    int rc = dawn_hubert_create(&c_hub, tab[0], n[0], &h.hubert);
    if (rc == 0) rc = dawn_pbnet_create(&c_pose, tab[1], n[1], &h.pose);
    if (rc == 0) rc = dawn_pbnet_create(&c_blink, tab[2], n[2], &h.blink);
    if (rc == 0) rc = dawn_decoder_create(&c_dec, tab[3], n[3], &h.decoder);
    if (rc == 0) rc = dawn_inputs_create(&c_in, tab[4], n[4], &h.inputs);
    if (rc == 0) rc = dawn_ctx_create(&c_unet, tab[5], n[5], &h.unet);
    const fmt::Entry* d = b->find(fmt::STAGE_HOST, fmt::KIND_HOST, "defaults");
    if (rc == 0 && d) {
        dawn_bundle_defaults def;
        memcpy(&def, b->f.host_blob(*d), sizeof def);
        if (def.up_border != 0) rc = dawn_ctx_set_option(h.unet, DAWN_OPT_UP_BORDER, def.up_border);
    }
    if (rc != 0) {                                                  // (the destroy calls leave the message of the failed create alone)
        dawn_bundle_destroy_handles(&h);
        return rc;
    }
    args->hubert = h.hubert; args->pose = h.pose; args->blink = h.blink; args->decoder = h.decoder; args->inputs = h.inputs; args->unet = h.unet;
    return 0;
}

extern "C" int dawn_bundle_create_motion(dawn_bundle* b, const void* device_mem, dawn_motion** m) {
    const char* who = "dawn_bundle_create_motion";
    if (!b || !device_mem || !m) return refuse(-350, who, "NULL argument");
    if (!b->find(fmt::STAGE_MOTION, fmt::KIND_HOST, "cfg")) return refuse(-359, who, "stage 'motion' is missing from the bundle (no cfg)");
    dawn_motion_cfg cfg;
    const dawn_named_ptr* tab = nullptr;
    int n = 0;
    CK(dawn_bundle_cfg(b, fmt::STAGE_MOTION, &cfg, sizeof cfg));
    CK(dawn_bundle_table(b, fmt::STAGE_MOTION, device_mem, &tab, &n));
    return dawn_motion_create(&cfg, tab, n, m);
}
