// kmu_sketch_pipe.hip -- kmu_sketch_count: per-sequence signatures and the k-mer count of the same reads in one call; on host
// buffers a pipeline over chunks of whole reads (upload | sketch | download | count).
#include <algorithm>
#include <condition_variable>
#include <memory>
#include <mutex>
#include <string>
#include <thread>

#include "kmu_hostpack.hpp"
#include "kmu_pipe_plan.hpp"
#include "kmu_sketch_host.hpp"

using namespace kmu;

// the events of the chunks (upload enqueued, sketch done): what was created is destroyed with the owner, whichever way the call ends
struct ChunkEvents {
    std::vector<hipEvent_t> up, sk;
    ~ChunkEvents() {
        for (const std::vector<hipEvent_t> *v : {&up, &sk})
            for (hipEvent_t e : *v) (void) hipEventDestroy(e);
    }
};

extern "C" int kmu_sketch_count(kmu_ctx *ctx, const kmu_sketch_params *p_in, kmu_counter *counter, const uint8_t *bases,
                                const uint64_t *offsets, uint32_t n_seq, void *sig_out) {
    if (!ctx || !p_in || !sig_out || !offsets) return KMU_E_BAD_ARG;
    kmu_sketch_params p_res; // (checked as unpacked input: packed input is refused below, as unsupported)
    KMU_TRY(sketch_seq_params(ctx, p_in, KMU_INPUT_ASCII, &p_res));
    const kmu_sketch_params *p = &p_res;
    if (p->mode != KMU_MODE_PER_SEQ || p->block_size != 0 || p->input_kind != KMU_INPUT_ASCII || p->algo == KMU_ALGO_BOTTOMK)
        return fail(ctx, KMU_E_UNSUPPORTED, "kmu_sketch_count: whole unpacked sequences, one signature each");
    if (counter && counter_ctx(counter) != ctx) return fail(ctx, KMU_E_BAD_ARG, "the counter belongs to another context");
    if (counter && kmer_is_aa(p->kmer_type)) return fail(ctx, KMU_E_BAD_ARG, "counting is defined on DNA k-mers");
    KMU_HIP(ctx, hipSetDevice(ctx->device));
    const size_t rowb = (size_t) p->sketch_size * sig_elem_bytes(p->sig_type);
    uint32_t *d_err;
    KMU_TRY(get_err_word(ctx, &d_err));
    if (p->mem == KMU_MEM_DEVICE) {
        DevSeqs ds;
        KMU_TRY(stage_sequences(ctx, bases, offsets, nullptr, n_seq, KMU_INPUT_ASCII, KMU_MEM_DEVICE, &ds));
        if (counter) { // (a distributed counter: census, route, scatter, and the all-to-all leaves on the exchange stream)
            DevSeqs dc = ds;
            KMU_TRY(count_add_device_begin(counter, dc, nullptr, KMU_MEM_DEVICE, d_err));
        }
        if (n_seq) KMU_TRY(sketch_per_seq_device(ctx, p, ds, nullptr, nullptr, sig_out, d_err, nullptr));
        if (counter) KMU_TRY(count_add_device_end(counter));
        if (!ctx->async_device) KMU_TRY(check_err_word(ctx, d_err));
        return finish_call(ctx, KMU_MEM_DEVICE);
    }
    if (p->mem != KMU_MEM_HOST) return fail(ctx, KMU_E_BAD_ARG, "bad mem %d", p->mem);
    if (!bases && n_seq) return fail(ctx, KMU_E_BAD_ARG, "null sequence buffers");
    // ---- host buffers: upload | sketch | download | count as a pipeline over chunks of whole reads ----
    const uint64_t off0 = n_seq ? offsets[0] : 0, total = n_seq ? offsets[n_seq] - off0 : 0;
    std::vector<uint64_t> h_off((size_t) n_seq + 1);
    for (uint32_t i = 0; i <= n_seq; i++) h_off[i] = offsets[i] - off0;
    uint64_t *d_o;
    void *d_b, *d_sig;
    KMU_TRY(dev_buf(ctx, "in.bases", total + 64, &d_b));
    KMU_TRY(dev_array(ctx, "in.offsets", (size_t) n_seq + 1, &d_o));
    KMU_TRY(dev_buf(ctx, "out.sig", (size_t) n_seq * rowb + 64, &d_sig));
    if (!ctx->pipe_h2d) KMU_HIP(ctx, hipStreamCreateWithFlags(&ctx->pipe_h2d, hipStreamNonBlocking));
    if (!ctx->pipe_d2h) KMU_HIP(ctx, hipStreamCreateWithFlags(&ctx->pipe_d2h, hipStreamNonBlocking));
    KMU_HIP(ctx, hipMemcpyAsync(d_o, h_off.data(), ((size_t) n_seq + 1) * 8, hipMemcpyHostToDevice, ctx->stream));
    uint64_t chunk_bytes = 512ull << 20;
    if (const char *e = getenv("KMU_PIPE_CHUNK_MB")) chunk_bytes = (uint64_t) std::max(1, atoi(e)) << 20;
    // Chunk sizes: the first one is an eighth of the others (the kernels start after 1 ms of upload instead of 9).  The upload
    // (4.38 GB at ~55 GB/s = 80 ms) is what the first phase is bound by -- a chunk's sketch + level 1 take 8 ms, its upload 9.3 --
    // and what is left when the last byte has arrived is the last chunk's sketch + level 1, then level 2 and the region build,
    // which need all of level 1.  (Tapering the last chunks shortens that tail by a chunk's sketch but pays for it in small
    // launches: 149.1 / 149.2 ms against 146.2 / 144.0 without, same box, r03: not kept.)
    // The bases cross PCIe packed (kmu_hostpack.hip): the host's cores pack chunk after chunk ahead of the upload, a quarter of the
    // bytes travels, a kernel on the upload stream restores the ASCII stream.  KMU_PIPE_PACK=0: the plain upload; small calls keep
    // it too.  Packed data arrive ~4x as fast as the kernels consume them, so the chunks may GROW: each three times its predecessor
    // (64 MB, 192 MB, 576 MB, 1.7 GB, the rest: every one is there before the kernels of the one before are through) -- five
    // launches of the sketch kernels instead of nine, each closer to the batched run's efficiency.  Headline workload, same box
    // (scripts/r04_hostleg.sh): 114.0 ms with growth 3, 115.3 / 116.0 with 2 / 4, 118.3 with equal chunks (KMU_PIPE_GROWTH=1),
    // 127.7 with the plain upload (KMU_PIPE_PACK=0); the device-resident step takes 104.5.
    bool packed_up = n_seq > 0 && total >= (32ull << 20);
    if (const char *e = getenv("KMU_PIPE_PACK")) packed_up = n_seq > 0 && atoi(e) != 0 && total >= 16;
    if (kmer_is_aa(p->kmer_type)) packed_up = false; // (residues are no bases: the 2-bit packer would reject every byte outside ACGT)
    uint64_t growth = packed_up ? 3 : 1;
    if (const char *e = getenv("KMU_PIPE_GROWTH")) growth = (uint64_t) std::max(1, atoi(e));
    std::vector<uint32_t> cut;       // chunk c = reads [cut[c], cut[c + 1])
    std::vector<uint64_t> pk_bounds; // its packed form: the stream [pk_bounds[c], pk_bounds[c + 1])
    pipe_chunk_plan(h_off, n_seq, total, chunk_bytes, growth, packed_up, &cut, &pk_bounds);
    const size_t n_chunks = cut.size() - 1;
    packed_up = packed_up && n_chunks > 0;
    void *h_packed = nullptr, *d_packed = nullptr;
    std::unique_ptr<PackPipe> packer;
    if (packed_up) {
        KMU_TRY(host_buf(ctx, "pipe.packed", (size_t) (total / 4 + 64), &h_packed));
        KMU_TRY(dev_buf(ctx, "pipe.packed_d", (size_t) (total / 4 + 64), &d_packed));
        int threads = 16;
        threads = std::min<int>(threads, std::max(1u, std::thread::hardware_concurrency()));
        try {
            packer.reset(new PackPipe(bases + off0, (uint8_t *) h_packed, total, threads));
        } catch (const std::exception &) { // (no threads to be had: the plain upload, same chunks)
            packer.reset();
            packed_up = false;
        }
    }
    ChunkEvents events;
    std::vector<hipEvent_t> &ev_up = events.up, &ev_sk = events.sk;
    for (size_t c = 0; c < n_chunks; c++)
        for (std::vector<hipEvent_t> *v : {&ev_up, &ev_sk}) {
            hipEvent_t e;
            KMU_HIP(ctx, hipEventCreateWithFlags(&e, hipEventDisableTiming));
            v->push_back(e);
        }
    int rc = KMU_OK;
    // (the uploads of the packed form are enqueued by a thread of their own: nothing in here touches the context's error state --
    //  a failure comes back as a code and a text, and the calling thread reports it)
    auto upload = [&](size_t c, std::string *msg) -> int {
        auto hip_ok = [&](hipError_t e, const char *what) {
            if (e == hipSuccess) return true;
            *msg = std::string(what) + ": " + hipGetErrorString(e);
            return false;
        };
        if (packed_up) {
            // in pieces of 64 M bases, each as soon as it is packed: the chunk's packing runs under its own upload.  Only copies go
            // on the upload stream: the kernel that restores the ASCII stream runs on the compute stream in front of the chunk's
            // kernels (on the upload stream it would wait for a CU that the persistent sketch kernels do not release, and every
            // copy behind it with it)
            const uint64_t p0 = pk_bounds[c], p1 = pk_bounds[c + 1], piece = 64ull << 20;
            for (uint64_t q0 = p0; q0 < p1; q0 += piece) {
                const uint64_t q1 = std::min(p1, q0 + piece);
                if (!packer->wait_prefix(q1)) {
                    *msg = "pattern not a code in alphabet_2b (non-ACGT byte in a sequence)";
                    return KMU_E_NON_ACGT;
                }
                if (!hip_ok(hipMemcpyAsync((uint8_t *) d_packed + q0 / 4, (const uint8_t *) h_packed + q0 / 4, (size_t) ((q1 - q0 + 3) / 4), hipMemcpyHostToDevice,
                                           ctx->pipe_h2d), "upload of a packed chunk")) return KMU_E_HIP;
            }
            return hip_ok(hipEventRecord(ev_up[c], ctx->pipe_h2d), "hipEventRecord") ? KMU_OK : KMU_E_HIP;
        }
        const uint64_t b0 = h_off[cut[c]], b1 = h_off[cut[c + 1]];
        if (!hip_ok(hipMemcpyAsync((uint8_t *) d_b + b0, bases + off0 + b0, b1 - b0, hipMemcpyHostToDevice, ctx->pipe_h2d), "upload of a chunk")) return KMU_E_HIP;
        return hip_ok(hipEventRecord(ev_up[c], ctx->pipe_h2d), "hipEventRecord") ? KMU_OK : KMU_E_HIP;
    };
    DevSeqs all;
    all.bases = (const uint8_t *) d_b;
    all.offsets = d_o;
    all.n_seq = n_seq;
    all.total_bytes = total;
    // the count's level-1 partition runs under the upload too, for the part of the stream that has arrived
    void *cc = nullptr;
    int cc_on = 0;
    if (counter && n_seq) {
        DevSeqs dc = all;
        rc = count_chunked_begin(counter, dc, h_off.data(), d_err, &cc, &cc_on);
    }
    // Packed uploads are enqueued by a thread of their own: an upload waits for the packer, and the thread that launches the
    // kernels of chunk c must not stand behind the packing of chunk c + 1.  It waits (on the host) only until the upload of ITS
    // chunk has been enqueued -- an event that has not been recorded yet cannot be waited for on a stream.
    std::mutex up_mu;
    std::condition_variable up_cv;
    size_t up_done = 0; // uploads of chunks [0, up_done) are enqueued
    int up_rc = KMU_OK;
    std::string up_msg, my_msg;
    std::thread uploader;
    if (packed_up && rc == KMU_OK) {
        try {
            uploader = std::thread([&] {
                (void) hipSetDevice(ctx->device);
                for (size_t c = 0; c < n_chunks; c++) {
                    std::string m;
                    const int r = upload(c, &m);
                    std::lock_guard<std::mutex> g(up_mu);
                    if (r != KMU_OK) { up_rc = r; up_msg = m; }
                    up_done = r == KMU_OK ? c + 1 : n_chunks; // (a failure releases every waiter)
                    up_cv.notify_all();
                    if (r != KMU_OK) return;
                }
            });
        } catch (const std::exception &) { rc = fail(ctx, KMU_E_HIP, "kmu_sketch_count: cannot start the upload thread"); }
    } else if (n_chunks && rc == KMU_OK) {
        rc = upload(0, &my_msg);
        if (rc != KMU_OK) (void) fail(ctx, rc, "%s", my_msg.c_str());
    }
    for (size_t c = 0; c < n_chunks && rc == KMU_OK; c++) {
        if (packed_up) {
            std::unique_lock<std::mutex> g(up_mu);
            up_cv.wait(g, [&] { return up_done > c; });
            rc = up_rc;
            if (rc != KMU_OK) (void) fail(ctx, rc, "%s", up_msg.c_str());
        } else if (c + 1 < n_chunks) {
            rc = upload(c + 1, &my_msg);
            if (rc != KMU_OK) (void) fail(ctx, rc, "%s", my_msg.c_str());
        }
        if (rc != KMU_OK) break;
        DevSeqs ds = all;
        ds.offsets = all.offsets + cut[c];
        ds.n_seq = cut[c + 1] - cut[c];
        uint8_t *d_rows = (uint8_t *) d_sig + (size_t) cut[c] * rowb;
        if (hipStreamWaitEvent(ctx->stream, ev_up[c], 0) != hipSuccess) { rc = fail(ctx, KMU_E_HIP, "hipStreamWaitEvent failed"); break; }
        if (packed_up && pk_bounds[c + 1] > pk_bounds[c]) {
            KernelTimer tm(ctx, "k_unpack2b");
            rc = launch_unpack2b(ctx, (const uint8_t *) d_packed + pk_bounds[c] / 4, pk_bounds[c + 1] - pk_bounds[c], (uint8_t *) d_b + pk_bounds[c]);
            if (rc != KMU_OK) break;
        }
        rc = sketch_per_seq_device(ctx, p, ds, nullptr, nullptr, d_rows, d_err, h_off.data() + cut[c]);
        if (rc != KMU_OK) break;
        if (hipEventRecord(ev_sk[c], ctx->stream) != hipSuccess || hipStreamWaitEvent(ctx->pipe_d2h, ev_sk[c], 0) != hipSuccess ||
            hipMemcpyAsync((uint8_t *) sig_out + (size_t) cut[c] * rowb, d_rows, (size_t) ds.n_seq * rowb, hipMemcpyDeviceToHost,
                           ctx->pipe_d2h) != hipSuccess)
            rc = fail(ctx, KMU_E_HIP, "signature download failed: %s", hipGetErrorString(hipGetLastError()));
        if (rc == KMU_OK && cc_on) rc = count_chunked_level1(counter, cc, h_off[cut[c + 1]]);
    }
    if (rc == KMU_OK && counter) { // the whole read set is resident by now: ev_up of the last chunk has been waited for
        if (cc_on) {
            rc = count_chunked_finish(counter, cc);
            cc = nullptr;
        } else {
            DevSeqs dc = all;
            rc = count_add_device_begin(counter, dc, h_off.data(), KMU_MEM_HOST, d_err);
            if (rc == KMU_OK) rc = count_add_device_end(counter);
        }
    }
    if (cc) count_chunked_abort(cc);
    if (uploader.joinable()) uploader.join(); // (a call that failed elsewhere: the uploads still queued are harmless, the buffers stay)
    packer.reset(); // (joins the workers: a call that ends early stops them at their next slab)
    (void) hipStreamSynchronize(ctx->pipe_h2d);
    (void) hipStreamSynchronize(ctx->pipe_d2h);
    if (rc != KMU_OK) {
        (void) hipStreamSynchronize(ctx->stream);
        return rc;
    }
    KMU_TRY(check_err_word(ctx, d_err));
    return finish_call(ctx, KMU_MEM_HOST);
}
