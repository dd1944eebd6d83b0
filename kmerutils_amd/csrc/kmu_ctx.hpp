// kmu_ctx.hpp -- host-side context of libkmu: device, stream, error text, workspace arena, per-kernel timing, and the steps every
// host driver is written in:
//   dev_array<T>(ctx, name, count, &p)  workspace `name` as `count` elements of T (dev_buf: the same in bytes, for padded or mixed buffers)
//   grid_for(ctx, n, per_block, per_cu) ceil(n / per_block) workgroups, at least 1, at most per_cu per CU (the rest by grid stride)
//   launch(ctx, name, kernel, grid, block, lds, args...)  the ONLY kernel launch of the library: on ctx->stream, timed as `name`
//                                       (nullptr: not timed), hipGetLastError checked behind every launch
//   check_mem(ctx, mem)                 the one "bad mem" refusal
//   stage_to_device(ctx, name, p, count, mem, &d)   an input: a host array staged in workspace `name`, a device array as it is
//   place_output(ctx, name, caller, count, mem, &d) / bring_output(ctx, caller, d, count, mem)   an output the kernels write in place:
//                                       the caller's array on a device call; workspace `name`, copied down behind the kernels, on a
//                                       host call (copy_out: a result produced in the workspace on both kinds of call)
//   read_back(ctx, {{&host, device}, ...})   a few words for the host: the copies and ONE synchronisation, no return in between
//                                       (caller_word: an element of a caller's input array, already here on a host call)
//   zero_first_offset(ctx, out, mem)    the first offset of an empty result
//   finish_call / finish_checked        the end of a call: synchronise and collect the kernel times, but leave a device call of an
//                                       async_device context in flight; finish_sync: always synchronise; finish_synced: behind a
//                                       read_back; refuse(ctx, code, fmt, ...): the error exit after work was enqueued
// A launch that was never timed stays untimed (profile_get reads at most 32 names and tests read the set of names as route probes);
// a timer that spans two kernels stays ONE KernelTimer scope around two launch(ctx, nullptr, ...).
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

#include <cstdarg>
#include <cstdio>
#include <cstring>
#include <map>
#include <string>
#include <vector>

#include "../../include/kmu.h"

struct kmu_comm;
struct kmu_ctx {
    int device = 0;
    kmu_comm *comm = nullptr; // kmu_comm_init / kmu_comm_init_custom (kmu_comm.hip)
    hipStream_t stream = nullptr;
    bool own_stream = false;
    bool async_device = false;
    bool err_unread = false; // the device error word holds bits no host read has seen yet (get_err_word / check_err_word)
    uint32_t lds_attr_set = 0; // kernels whose MaxDynamicSharedMemorySize was raised on THIS context's device (bit per kernel group)
    std::string err;
    // kmu_sketch_partial / kmu_sketch_hashed_partial: where the all-sequences paths leave their per-slot minima instead of
    // turning them into a signature (device memory; null in every other call)
    uint64_t *partial_out = nullptr;
    kmu_hll_params hll = {1.001, 20.0, 65534u, 0u}; // SetSketchParams of KMU_ALGO_HLL calls (kmu_set_hll_params)
    // grow-on-demand device scratch buffers, keyed by purpose (never shrunk; freed with the context)
    struct Buf {
        void *p = nullptr;
        size_t bytes = 0;
    };
    std::map<std::string, Buf> bufs;
    // pinned host staging
    std::map<std::string, Buf> hbufs;
    // profiling
    bool profiling = false;
    struct Pending {
        std::string name;
        hipEvent_t a, b;
    };
    std::vector<Pending> pending;
    std::vector<hipEvent_t> event_pool;
    struct Stat {
        uint64_t launches = 0;
        double ms = 0;
    };
    std::map<std::string, Stat> stats;
    // k_pmh_points' a-priori q_max bound: c of KMU_PMH_TAU_C, read at the first launch (0: no bound)
    bool pmh_tau_read = false;
    double pmh_tau_c = 0.0;
    int num_cus = 256;
    size_t lds_per_block = 65536;
    // kmu_sketch_count on host buffers: uploads and downloads run on streams of their own, next to the kernels
    hipStream_t pipe_h2d = nullptr, pipe_d2h = nullptr;
};

namespace kmu {

extern thread_local std::string g_create_error;

inline int fail(kmu_ctx *ctx, int code, const char *fmt, ...) {
    char buf[512];
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(buf, sizeof buf, fmt, ap);
    va_end(ap);
    if (ctx) ctx->err = buf;
    else g_create_error = buf;
    return code;
}

#define KMU_HIP(ctx, expr)                                                                              \
    do {                                                                                                \
        hipError_t e_ = (expr);                                                                         \
        if (e_ != hipSuccess)                                                                           \
            return kmu::fail((ctx), e_ == hipErrorOutOfMemory ? KMU_E_OOM : KMU_E_HIP, "%s: %s (%s:%d)", #expr, \
                             hipGetErrorString(e_), __FILE__, __LINE__);                                \
    } while (0)

#define KMU_TRY(expr)           \
    do {                        \
        int rc_ = (expr);       \
        if (rc_ != KMU_OK) return rc_; \
    } while (0)

// device scratch buffer of at least `bytes`
inline int dev_buf(kmu_ctx *ctx, const char *name, size_t bytes, void **out) {
    auto &b = ctx->bufs[name];
    if (b.bytes < bytes) {
        if (b.p) {
            KMU_HIP(ctx, hipStreamSynchronize(ctx->stream));
            KMU_HIP(ctx, hipFree(b.p));
            b.p = nullptr;
            b.bytes = 0;
        }
        size_t want = bytes + bytes / 8 + 256;
        KMU_HIP(ctx, hipMalloc(&b.p, want));
        b.bytes = want;
    }
    *out = b.p;
    return KMU_OK;
}
// dev_buf as `count` elements of T
template <class T> inline int dev_array(kmu_ctx *ctx, const char *name, size_t count, T **out) {
    void *p;
    KMU_TRY(dev_buf(ctx, name, count * sizeof(T), &p));
    *out = static_cast<T *>(p);
    return KMU_OK;
}
inline int check_mem(kmu_ctx *ctx, int mem) {
    if (mem != KMU_MEM_HOST && mem != KMU_MEM_DEVICE) return fail(ctx, KMU_E_BAD_ARG, "bad mem %d", mem);
    return KMU_OK;
}
// `count` elements of a host array of a KMU_MEM_HOST call staged in workspace `name` (of `count + pad` elements); a device array
// (or null) as it is
template <class T> inline int stage_to_device(kmu_ctx *ctx, const char *name, const T *p, size_t count, int mem, const T **out, size_t pad = 0) {
    if (mem == KMU_MEM_DEVICE || !p) { *out = p; return KMU_OK; }
    T *d;
    KMU_TRY(dev_array(ctx, name, count + pad ? count + pad : 1, &d));
    if (count) KMU_HIP(ctx, hipMemcpyAsync(d, p, count * sizeof(T), hipMemcpyHostToDevice, ctx->stream));
    *out = d;
    return KMU_OK;
}
// (an array whose element type the call chooses at run time: in bytes)
inline int stage_to_device(kmu_ctx *ctx, const char *name, const void *p, size_t bytes, int mem, const void **out, size_t pad = 0) {
    return stage_to_device(ctx, name, static_cast<const uint8_t *>(p), bytes, mem, reinterpret_cast<const uint8_t **>(out), pad);
}
// where the kernels write a caller's output: the caller's array on a device call, workspace `name` of `count` elements on a host
// call (an output the caller does not want, null, stays null)
template <class T> inline int place_output(kmu_ctx *ctx, const char *name, T *caller, size_t count, int mem, T **out) {
    if (mem == KMU_MEM_HOST && caller) return dev_array(ctx, name, count, out);
    *out = caller;
    return KMU_OK;
}
// ... and behind the kernels: a host call copies `count` elements of the workspace down, a device call has nothing to do
template <class T> inline int bring_output(kmu_ctx *ctx, T *caller, const T *placed, size_t count, int mem) {
    if (mem == KMU_MEM_HOST && caller && count) KMU_HIP(ctx, hipMemcpyAsync(caller, placed, count * sizeof(T), hipMemcpyDeviceToHost, ctx->stream));
    return KMU_OK;
}
// a device array of the workspace to a caller's array that lives where `mem` says
inline int copy_out(kmu_ctx *ctx, void *dst, const void *src, size_t bytes, int mem) {
    if (!dst || !bytes) return KMU_OK;
    KMU_HIP(ctx, hipMemcpyAsync(dst, src, bytes, mem == KMU_MEM_HOST ? hipMemcpyDeviceToHost : hipMemcpyDeviceToDevice, ctx->stream));
    return KMU_OK;
}
// a few words of device memory for the host (a null source: none): every copy on the stream, then ONE synchronisation.  The destinations are mostly stack
// locals, so this does not return before the stream was synchronised, whatever a copy said.
struct Word {
    void *dst;
    const void *src;
    size_t bytes;
    template <class T> Word(T *d, const T *s) : dst(d), src(s), bytes(sizeof(T)) {}
    Word(void *d, const void *s, size_t n) : dst(d), src(s), bytes(n) {} // (a short array)
};
inline int read_back(kmu_ctx *ctx, std::initializer_list<Word> words) {
    hipError_t e = hipSuccess;
    for (const Word &w : words)
        if (w.src && e == hipSuccess) e = hipMemcpyAsync(w.dst, w.src, w.bytes, hipMemcpyDeviceToHost, ctx->stream);
    const hipError_t s = hipStreamSynchronize(ctx->stream);
    KMU_HIP(ctx, e);
    KMU_HIP(ctx, s);
    return KMU_OK;
}
// one element of a caller's input array: already here on a host call, read back on a device call
template <class T> inline int caller_word(kmu_ctx *ctx, const T *p, int mem, T *out) {
    if (mem == KMU_MEM_HOST) { *out = *p; return KMU_OK; }
    return read_back(ctx, {{out, p}});
}
// the first offset of an empty result, on either side of `mem`
inline int zero_first_offset(kmu_ctx *ctx, uint64_t *offsets_out, int mem) {
    if (!offsets_out) return KMU_OK;
    if (mem == KMU_MEM_HOST) offsets_out[0] = 0;
    else KMU_HIP(ctx, hipMemsetAsync(offsets_out, 0, 8, ctx->stream));
    return KMU_OK;
}
inline int host_buf(kmu_ctx *ctx, const char *name, size_t bytes, void **out) {
    auto &b = ctx->hbufs[name];
    if (b.bytes < bytes) {
        if (b.p) {
            KMU_HIP(ctx, hipStreamSynchronize(ctx->stream));
            KMU_HIP(ctx, hipHostFree(b.p));
            b.p = nullptr;
            b.bytes = 0;
        }
        size_t want = bytes + bytes / 8 + 256;
        KMU_HIP(ctx, hipHostMalloc(&b.p, want, hipHostMallocDefault));
        b.bytes = want;
    }
    *out = b.p;
    return KMU_OK;
}

// RAII-ish timing scope around one kernel launch (hipEvents on the context stream); a null name times nothing
struct KernelTimer {
    kmu_ctx *ctx;
    hipEvent_t a = nullptr, b = nullptr;
    const char *name;
    KernelTimer(kmu_ctx *c, const char *n) : ctx(c), name(n) {
        if (!name || !ctx->profiling) return;
        auto get = [&]() {
            hipEvent_t e;
            if (!ctx->event_pool.empty()) {
                e = ctx->event_pool.back();
                ctx->event_pool.pop_back();
            } else {
                (void) hipEventCreate(&e);
            }
            return e;
        };
        a = get();
        b = get();
        (void) hipEventRecord(a, ctx->stream);
    }
    ~KernelTimer() {
        if (!name || !ctx->profiling) return;
        (void) hipEventRecord(b, ctx->stream);
        ctx->pending.push_back({name, a, b});
    }
};

// ceil(n / per_block) workgroups, at least one, at most per_cu per CU
inline int grid_for(const kmu_ctx *ctx, uint64_t n, int per_block, int per_cu = 8) {
    const uint64_t blocks = (n + per_block - 1) / per_block, cap = (uint64_t) ctx->num_cus * per_cu;
    return (int) (blocks < 1 ? 1 : blocks < cap ? blocks : cap);
}

// one kernel launch on the context's stream: timed as `name` (nullptr: not timed), checked.  The arguments are converted to the
// kernel's own parameter types, so nullptr and pointers to non-const pass as they are.
template <class... P, class... A>
inline int launch(kmu_ctx *ctx, const char *name, void (*kern)(P...), dim3 grid, dim3 block, size_t lds, A &&...args) {
    {
        KernelTimer t(ctx, name);
        hipLaunchKernelGGL(kern, grid, block, lds, ctx->stream, static_cast<P>(args)...);
    }
    KMU_HIP(ctx, hipGetLastError());
    return KMU_OK;
}

inline void profile_collect(kmu_ctx *ctx) {
    if (ctx->pending.empty()) return;
    (void) hipStreamSynchronize(ctx->stream);
    for (auto &p : ctx->pending) {
        float ms = 0;
        if (hipEventElapsedTime(&ms, p.a, p.b) == hipSuccess) {
            auto &s = ctx->stats[p.name];
            s.launches++;
            s.ms += ms;
        }
        ctx->event_pool.push_back(p.a);
        ctx->event_pool.push_back(p.b);
    }
    ctx->pending.clear();
}

// sequence inputs resolved to device memory
struct DevSeqs {
    const uint8_t *bases = nullptr;
    const uint64_t *offsets = nullptr;        // n_seq + 1
    const uint64_t *packed_offsets = nullptr; // n_seq (+1) or null
    uint64_t total_bytes = 0;                 // size of `bases` in bytes
    uint32_t n_seq = 0;
    int packed = 0;
    std::vector<uint64_t> h_offsets; // host copy of offsets (always available)
    std::vector<uint64_t> h_packed_offsets;
};

int stage_sequences(kmu_ctx *ctx, const uint8_t *bases, const uint64_t *offsets, const uint64_t *packed_offsets,
                    uint32_t n_seq, int input_kind, int mem, DevSeqs *out);

// the end of a call: synchronise and collect the kernel times, but leave a device call of an async_device context in flight
int finish_call(kmu_ctx *ctx, int mem);
// the end of a call whose contract is to synchronise in every context (its counts are on the host when it returns)
inline int finish_sync(kmu_ctx *ctx) {
    KMU_HIP(ctx, hipStreamSynchronize(ctx->stream));
    if (ctx->profiling) profile_collect(ctx);
    return KMU_OK;
}
// ... where the last operation of the call was a read_back: the stream is synchronised already
inline int finish_synced(kmu_ctx *ctx) {
    if (ctx->profiling) profile_collect(ctx);
    return KMU_OK;
}
// a refusal after kernels were enqueued: their times are collected (profile_collect synchronises), then fail
template <class... A> inline int refuse(kmu_ctx *ctx, int code, const char *fmt, A... args) {
    (void) finish_synced(ctx);
    return fail(ctx, code, fmt, args...);
}

// device error word (bit flags set by kernels)
enum : uint32_t { DERR_NON_ACGT = 1u, DERR_TABLE_FULL = 2u, DERR_BAD_AA = 4u, DERR_EMPTY_SEQ = 8u, DERR_BAD_RANGE = 16u };
int get_err_word(kmu_ctx *ctx, uint32_t **out); // zeroed on the stream
int check_err_word(kmu_ctx *ctx, uint32_t *d_err);
// the end of a call whose kernels had the error word: read it (an asynchronous device call leaves that to a later one), finish_call
inline int finish_checked(kmu_ctx *ctx, int mem, uint32_t *d_err) {
    if (!(mem == KMU_MEM_DEVICE && ctx->async_device)) KMU_TRY(check_err_word(ctx, d_err));
    return finish_call(ctx, mem);
}

void comm_free(kmu_ctx *ctx); // kmu_comm.hip
// kmu_count.hip, for kmu_sketch_count
int count_add_device_begin(kmu_counter *c, DevSeqs &ds, const uint64_t *host_offsets, int mem, uint32_t *d_err);
int count_add_device_end(kmu_counter *c);
kmu_ctx *counter_ctx(kmu_counter *c);
int count_chunked_begin(kmu_counter *c, DevSeqs &all, const uint64_t *host_offsets, uint32_t *d_err, void **handle, int *on);
int count_chunked_level1(kmu_counter *c, void *handle, uint64_t bases_ready);
int count_chunked_finish(kmu_counter *c, void *handle);
void count_chunked_abort(void *handle);

int check_kmer(kmu_ctx *ctx, int kmer_type, int k);
inline bool kmer_is_aa(int t) { return t == KMU_KMERAA32BIT || t == KMU_KMERAA64BIT; }
inline int kmer_val_bytes(int t) { return (t == KMU_KMER64BIT || t == KMU_KMERAA64BIT) ? 8 : 4; }
bool fhash_valid(int fhash, int kmer_type);
// fhash_valid, and packed (2-bit) input only where the k-mer type and the fhash are defined on it
int check_fhash_input(kmu_ctx *ctx, int kmer_type, int fhash, int input_kind);
// check_kmer and check_fhash_input of a call that takes kmu_hash_params
int check_hash_params(kmu_ctx *ctx, const kmu_hash_params *p);

// exclusive scan of n u32 values into u64 offsets, out[n] = total (kmu_ingest.hip)
int device_scan_u32(kmu_ctx *ctx, const uint32_t *in, uint64_t n, uint64_t *out);

// radix partition of a device u64 array by the top bits of fmix64(key) (kmu_count.hip)
int partition_u64(kmu_ctx *ctx, const uint64_t *in, uint64_t n, int region_bits, const uint64_t **items_out,
                  const uint64_t **bounds_out, bool hashed_out = false);

} // namespace kmu
