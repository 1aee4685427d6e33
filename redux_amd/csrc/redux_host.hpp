// redux_host.hpp -- the host-pointer side of the C ABI (redux_encode_blocks, redux_decode_blocks,
// redux_compress, redux_decompress): what a Rust / C / ctypes caller holding plain host memory binds.
//
// A call is a pipeline over CHUNKS of whole blocks:
//
//   caller memory --(N CPU threads)--> pinned ring --(H2D DMA)--> chunk slot in HBM
//        --> coder kernels of that chunk (its own HIP stream) --> dense chunk output
//        --(D2H DMA)--> caller memory
//
// Why it looks like this (numbers: tools/ubench/pcie.hip on the MI355X box, profiles/r02_host_abi/):
//   * hipMalloc / hipFree / hipHostMalloc cost milliseconds to hundreds of milliseconds: everything is
//     allocated once, kept in a per-device context and only ever grown (redux_host_release() frees it).
//     The context is guarded by one mutex: concurrent calls are safe and serialise.
//   * H2D from pageable memory through the runtime's own staging runs at 29 GB/s, from pinned memory at
//     57 GB/s, and 4 CPU threads fill a pinned buffer at 76 GB/s: the input is staged by a small pool of
//     copy threads (alive for the duration of the call) through a ring of pinned pieces.
//   * a block is a serial chain: the coder kernel of ANY number of 64 KiB blocks takes ~12 ms (decode
//     ~28 ms).  Eight chunks are therefore in flight on eight streams -- a chunk of 128 MiB is 32
//     workgroups, the chip holds 1024 -- so that the PCIe transfers of later chunks hide under the
//     kernels of earlier ones and only ONE kernel latency is exposed at the end of the call.
//   * the way back is one DMA per chunk straight into the caller's (pageable) memory, issued by a drain
//     thread when the chunk's event fires, so that draining chunk k never delays staging and launching
//     chunk k+8.  Nothing that depends on a running kernel is ever put into a copy queue: the SDMA
//     queues are in order, and a 16 KiB result copy waiting for its kernel blocks every copy behind it.
//
// Included by redux_hip.hip (one translation unit), whose ABI entry points choose the coder a call runs (EncodeCoder,
// DecodeCoder).
#pragma once

#include "../../include/redux_hip.h"

#include <hip/hip_runtime.h>

#include <array>
#include <atomic>
#include <chrono>
#include <condition_variable>
#include <functional>
#include <initializer_list>
#include <mutex>
#include <optional>
#include <stdint.h>
#include <string.h>
#include <thread>
#include <utility>
#include <vector>

namespace redux {
namespace host {

// The HIP runtime multiplexes the streams of a process onto FOUR hardware queues per priority level
// (GPU_MAX_HW_QUEUES), the null stream holds one of the normal-priority ones, and streams that share a
// queue run one after the other (tools/ubench/queues.hip: 3 default-priority streams run at once, the
// 4th waits; 4 high- + 4 low-priority streams all run at once).  Measured with 16 default-priority
// compute streams + a copy stream + a drain stream: 2.6 chunk kernels in flight, 13 GB/s.
// So: eight streams, four created at the highest and four at the lowest priority (none at the
// application's own level), chunk k does EVERYTHING (its H2D, its kernels, its D2H) on stream k % 8,
// and chunks are large enough that eight kernels in flight outrun the PCIe link:
//   chunk bytes / PCIe rate >= kernel latency / 8   ->  >= 78 MB (encode, 12.5 ms), >= 175 MB (decode, 28 ms).
constexpr int      kSlots      = 8;             // chunk slots in HBM = streams (a slot is reused once its chunk has been drained)
constexpr int      kStreams    = kSlots;
constexpr int      kPieces     = 8;             // pinned staging ring
constexpr uint64_t kPieceBytes = 16ull << 20;
constexpr uint64_t kEncChunkMax = 128ull << 20; // input bytes per chunk
constexpr uint64_t kDecChunkMax = 256ull << 20; // output bytes per chunk
constexpr uint64_t kChunkMin    = 16ull << 20;
constexpr int      kCopyThreads = 4;            // incl. the calling thread

// ---- N threads that copy one buffer together -------------------------------------------------
class CopyPool {
    int                      n_;
    std::vector<std::thread> th_;
    std::mutex               m_;
    std::condition_variable  go_, done_;
    uint64_t                 gen_ = 0;
    int                      pending_ = 0;
    bool                     stop_ = false;
    char                    *d_ = nullptr;
    const char              *s_ = nullptr;
    size_t                   len_ = 0;

    void worker(int id)
    {
        uint64_t seen = 0;
        for (;;) {
            std::unique_lock<std::mutex> l(m_);
            go_.wait(l, [&] { return stop_ || gen_ != seen; });
            if (stop_)
                return;
            seen = gen_;
            char *d = d_; const char *s = s_; const size_t len = len_;
            l.unlock();
            const size_t a = len * (size_t)(id + 1) / (size_t)(n_ + 1), b = len * (size_t)(id + 2) / (size_t)(n_ + 1);
            memcpy(d + a, s + a, b - a);
            l.lock();
            if (--pending_ == 0)
                done_.notify_one();
        }
    }

public:
    explicit CopyPool(int helpers) : n_(helpers)
    {
        for (int i = 0; i < n_; i++)
            th_.emplace_back([this, i] { worker(i); });
    }
    ~CopyPool()
    {
        {
            std::lock_guard<std::mutex> l(m_);
            stop_ = true;
        }
        go_.notify_all();
        for (auto &t : th_)
            t.join();
    }
    void copy(void *dst, const void *src, size_t len)
    {
        if (len < (1u << 20) || n_ == 0) {
            memcpy(dst, src, len);
            return;
        }
        {
            std::lock_guard<std::mutex> l(m_);
            d_ = (char *)dst; s_ = (const char *)src; len_ = len; pending_ = n_; gen_++;
        }
        go_.notify_all();
        memcpy(dst, src, len / (size_t)(n_ + 1)); // slice 0 on the calling thread
        std::unique_lock<std::mutex> l(m_);
        done_.wait(l, [&] { return pending_ == 0; });
    }
};

// ---- persistent per-device context -----------------------------------------------------------
struct Buf {
    bool   pinned = false; // hipHostMalloc'd (a pinned mirror of a device array), else hipMalloc'd
    void  *p      = nullptr;
    size_t cap    = 0;
};

struct Slot {          // one chunk in flight
    Buf d_in, d_ws, d_out, d_off, d_sz, d_st, d_sum, d_used, d_tab, d_crc, d_stf, d_base;                      // device
    Buf h_off{true}, h_sz{true}, h_st{true}, h_sum{true}, h_used{true}, h_tab{true}, h_crc{true}, h_stf{true}; // pinned mirrors of the small arrays
    hipEvent_t done = nullptr; // recorded after the chunk's kernels
    // (d_stf / h_stf: the stored-block flags, u8 per block)
    // (d_base: the chunk's share of the base of the XOR-against-base filter, base_len bytes of it: BaseIo)
    uint64_t base_len = 0;

    std::array<Buf *, 20> bufs()
    {
        return {&d_in, &d_ws, &d_out, &d_off, &d_sz, &d_st, &d_sum, &d_used, &d_tab, &d_crc, &d_stf, &d_base,
                &h_off, &h_sz, &h_st, &h_sum, &h_used, &h_tab, &h_crc, &h_stf};
    }
};

struct Ctx {
    std::mutex  mu;
    // Both only ever written with mu held: `want` by the call that has just locked the context (the device it is to run on),
    // `device` by ctx_init_locked / ctx_teardown_locked (the device the streams, events and buffers below were created on).
    int         want = -1;
    int         device = -1;
    bool        ready = false;
    hipStream_t stream[kStreams] = {};
    hipStream_t drain = nullptr; // bulk D2H, issued by the drain thread once a chunk's event has fired
    Slot        slot[kSlots];
    void       *piece[kPieces] = {};      // input staging ring
    hipEvent_t  piece_free[kPieces] = {};
    Buf         d_counts;   // u64[256]: byte_histogram
    uint64_t    allocs = 0; // hipMalloc / hipHostMalloc calls so far (redux_host_allocations)
    // timeline of the last call, seconds since its start: per chunk {staging begins, device work enqueued,
    // kernels done (drain thread saw the event), results in caller memory}; trace[0..3] of chunk 0 etc.
    std::vector<double> trace;
    double              t0 = 0;
};

static double now_s()
{
    return std::chrono::duration<double>(std::chrono::steady_clock::now().time_since_epoch()).count();
}

static Ctx g_ctx[16];

#define HOST_TRY(expr)                                                                                 \
    do {                                                                                               \
        hipError_t e_ = (expr);                                                                        \
        if (e_ != hipSuccess) {                                                                        \
            fprintf(stderr, "redux_hip: %s failed: %s (%s:%d)\n", #expr, hipGetErrorString(e_),       \
                    __FILE__, __LINE__);                                                               \
            return REDUX_IO_ERROR;                                                                     \
        }                                                                                              \
    } while (0)

static void free_buf(Buf &b)
{
    if (b.p)
        (void)(b.pinned ? hipHostFree(b.p) : hipFree(b.p));
    b.p = nullptr; b.cap = 0;
}

static int grow_buf(Ctx &c, Buf &b, size_t need)
{
    if (b.cap >= need)
        return REDUX_OK;
    if (b.p)
        HOST_TRY(b.pinned ? hipHostFree(b.p) : hipFree(b.p));
    b.p = nullptr; b.cap = 0;
    const size_t cap = (need + need / 8 + 4095) & ~(size_t)4095;
    HOST_TRY(b.pinned ? hipHostMalloc(&b.p, cap, hipHostMallocDefault) : hipMalloc(&b.p, cap));
    c.allocs++;
    b.cap = cap;
    return REDUX_OK;
}

// every (buffer, bytes) pair in turn; the first failure ends it
static int grow_bufs(Ctx &c, std::initializer_list<std::pair<Buf *, uint64_t>> need)
{
    for (const auto &n : need) {
        const int rc = grow_buf(c, *n.first, n.second);
        if (rc != REDUX_OK)
            return rc;
    }
    return REDUX_OK;
}

// the context of HIP's current device; its streams, events and staging ring are created by the first call that
// holds its mutex (ctx_init_locked) and torn down by redux_host_release under the same mutex
static int ctx_of_current_device(Ctx **out, int *dev_out)
{
    int dev = 0;
    HOST_TRY(hipGetDevice(&dev));
    if (dev < 0 || dev >= 16)
        return REDUX_UNSUPPORTED;
    *out     = &g_ctx[dev];
    *dev_out = dev;
    return REDUX_OK;
}

static void ctx_teardown_locked(Ctx &c);

// c.mu is held and c.want says which device the call runs on.  A context that was built for another device -- the fleet
// was reconfigured, or fleet entry i and default-mode device d share g_ctx[] -- is torn down first: its streams, events,
// HBM and pinned buffers belong to the device they were created on.
static int ctx_init_locked(Ctx &c)
{
    if (c.ready && c.device != c.want)
        ctx_teardown_locked(c); // (leaves HIP's current device at c.device: set again below)
    HOST_TRY(hipSetDevice(c.want));
    if (c.ready)
        return REDUX_OK;
    int pri_lo = 0, pri_hi = 0; // numerically: lo = least urgent, hi = most urgent
    HOST_TRY(hipDeviceGetStreamPriorityRange(&pri_lo, &pri_hi));
    for (int i = 0; i < kStreams; i++)
        HOST_TRY(hipStreamCreateWithPriority(&c.stream[i], hipStreamNonBlocking, (i & 1) ? pri_hi : pri_lo));
    HOST_TRY(hipStreamCreateWithFlags(&c.drain, hipStreamNonBlocking));
    for (int i = 0; i < kSlots; i++)
        HOST_TRY(hipEventCreateWithFlags(&c.slot[i].done, hipEventDisableTiming));
    for (int i = 0; i < kPieces; i++) {
        HOST_TRY(hipHostMalloc(&c.piece[i], kPieceBytes, hipHostMallocDefault));
        HOST_TRY(hipEventCreateWithFlags(&c.piece_free[i], hipEventDisableTiming));
        c.allocs++;
    }
    c.device = c.want;
    c.ready  = true;
    return REDUX_OK;
}

// frees everything the context holds on the device it was built for (c.mu is held)
static void ctx_teardown_locked(Ctx &c)
{
    if (!c.ready)
        return;
    (void)hipSetDevice(c.device);
    for (int i = 0; i < kStreams; i++) // (a call in flight holds c.mu, so these are idle: belt and braces)
        if (c.stream[i]) (void)hipStreamSynchronize(c.stream[i]);
    for (Slot &s : c.slot) {
        for (Buf *b : s.bufs())
            free_buf(*b);
        if (s.done) (void)hipEventDestroy(s.done);
        s.done = nullptr;
    }
    free_buf(c.d_counts);
    for (int i = 0; i < kPieces; i++) {
        if (c.piece[i]) (void)hipHostFree(c.piece[i]);
        if (c.piece_free[i]) (void)hipEventDestroy(c.piece_free[i]);
        c.piece[i] = nullptr; c.piece_free[i] = nullptr;
    }
    for (int i = 0; i < kStreams; i++) {
        if (c.stream[i]) (void)hipStreamDestroy(c.stream[i]);
        c.stream[i] = nullptr;
    }
    if (c.drain) (void)hipStreamDestroy(c.drain);
    c.drain = nullptr;
    c.ready = false;
}

// A call on an unusually large shape (one block of hundreds of MiB, a generous decode capacity) leaves slot buffers behind
// that no ordinary call needs: the context keeps what the chunk pipeline itself can ask for (256 MiB of payload + workspace)
// and gives back anything above kTrimBytes when such a call ends.
constexpr size_t kTrimBytes = 1ull << 30;
static void ctx_trim_locked(Ctx &c)
{
    if (!c.ready)
        return;
    for (Slot &s : c.slot)
        for (Buf *b : {&s.d_in, &s.d_ws, &s.d_out, &s.d_base})
            if (b->cap > kTrimBytes)
                free_buf(*b);
}

struct CallerDevice { // HIP's current device when the scope began, made current again when it ends
    int d = -1;
    CallerDevice() { (void)hipGetDevice(&d); }
    ~CallerDevice()
    {
        if (d >= 0)
            (void)hipSetDevice(d);
    }
};

static int ctx_release_all()
{
    CallerDevice caller; // freeing another device's context must not move the caller
    for (Ctx &c : g_ctx) {
        std::lock_guard<std::mutex> lc(c.mu); // waits for a call in flight on that device
        ctx_teardown_locked(c);
    }
    return REDUX_OK;
}

// stage `len` host bytes into the slot's device input at byte offset 0, through the pinned ring, on `s`
static int stage_h2d(Ctx &c, CopyPool &pool, uint64_t &piece_no, void *d_dst, const uint8_t *src, uint64_t len, hipStream_t s)
{
    for (uint64_t o = 0; o < len; o += kPieceBytes) {
        const uint64_t n = len - o < kPieceBytes ? len - o : kPieceBytes;
        const int      k = (int)(piece_no % kPieces);
        if (piece_no >= (uint64_t)kPieces)
            HOST_TRY(hipEventSynchronize(c.piece_free[k])); // the H2D that last read this piece has finished
        pool.copy(c.piece[k], src + o, n);
        HOST_TRY(hipMemcpyAsync((uint8_t *)d_dst + o, c.piece[k], n, hipMemcpyHostToDevice, s));
        HOST_TRY(hipEventRecord(c.piece_free[k], s));
        piece_no++;
    }
    return REDUX_OK;
}

// `len` device bytes -> caller memory on the drain stream.  The destination is pageable: the runtime
// pins it on the fly and DMAs straight into it at ~55 GB/s -- no second CPU pass over host DRAM, whose
// bandwidth the staging threads and both DMA directions already share.  (An own pinned ring + copy
// threads on this side measured 15 % slower on 4 GiB for that reason.)
static int drain_d2h(Ctx &c, uint8_t *dst, const void *d_src, uint64_t len)
{
    HOST_TRY(hipMemcpyAsync(dst, d_src, len, hipMemcpyDeviceToHost, c.drain));
    HOST_TRY(hipStreamSynchronize(c.drain));
    return REDUX_OK;
}

// ---- which contexts a host-pointer call runs on ------------------------------------------------
// Default: the context of HIP's current device (g_ctx[device id]).  redux_host_set_devices() installs a FLEET instead:
// context i serves device fleet[i] -- ids may repeat, each entry is its own context with its own streams and buffers --
// and every redux_encode_blocks / redux_decode_blocks call deals its chunks round-robin over all of them.  The data starts
// and ends in host memory, so nothing is exchanged between devices: each context is fed over its own PCIe link.
static std::mutex       g_fleet_mu;
static std::vector<int> g_fleet;                                    // empty: current device only
static std::atomic<uint64_t> g_chunk_min{0}, g_chunk_max{0};        // test hook (redux_host_set_chunk_bytes): 0 = the defaults

// Which contexts a call runs on, and the device each is to run on.  Nothing of a context is touched here: the caller locks
// every context's mutex (always in this order) and only then records the device in it (take_contexts).
static int contexts_for_call(std::vector<Ctx *> &out, std::vector<int> &want)
{
    std::lock_guard<std::mutex> l(g_fleet_mu);
    if (g_fleet.empty()) {
        Ctx *cp  = nullptr;
        int  dev = 0;
        int  rc  = ctx_of_current_device(&cp, &dev);
        if (rc != REDUX_OK)
            return rc;
        out.push_back(cp);
        want.push_back(dev);
        return REDUX_OK;
    }
    for (size_t i = 0; i < g_fleet.size(); i++) {
        out.push_back(&g_ctx[i]);
        want.push_back(g_fleet[i]);
    }
    return REDUX_OK;
}

// contexts_for_call + their mutexes, taken in context order (two calls cannot deadlock); each context then knows its device
static int take_contexts(std::vector<Ctx *> &ctx, std::vector<std::unique_lock<std::mutex>> &locks)
{
    std::vector<int> want;
    int rc = contexts_for_call(ctx, want);
    if (rc != REDUX_OK)
        return rc;
    for (size_t i = 0; i < ctx.size(); i++) {
        locks.emplace_back(ctx[i]->mu);
        ctx[i]->want = want[i];
    }
    return REDUX_OK;
}

// The fleet changes under g_fleet_mu, held across the assignment AND the release of the old contexts: a call that asks for
// its contexts meanwhile waits, then sees the new fleet.  (A call that already holds contexts of the old fleet finishes
// first -- the release waits for its mutexes -- and whatever it leaves built for an old device is rebuilt by the next
// call that finds the device changed: ctx_init_locked.)
static int set_devices(const int32_t *ids, uint32_t n)
{
    if (n > 16 || (n && !ids))
        return REDUX_INVALID_INPUT;
    int count = 0;
    if (hipGetDeviceCount(&count) != hipSuccess)
        return REDUX_IO_ERROR;
    for (uint32_t i = 0; i < n; i++)
        if (ids[i] < 0 || ids[i] >= count)
            return REDUX_INVALID_INPUT;
    std::lock_guard<std::mutex> l(g_fleet_mu);
    g_fleet.assign(ids, ids + n);
    ctx_release_all(); // contexts are bound to a device when they are built: start from none
    return REDUX_OK;
}

// `bytes` within [kChunkMin, chunk_max], or within the test hook's bounds where it sets them
static uint64_t clamp_chunk_bytes(uint64_t bytes, uint64_t chunk_max)
{
    const uint64_t lo = g_chunk_min.load() ? g_chunk_min.load() : kChunkMin;
    const uint64_t hi = g_chunk_max.load() ? g_chunk_max.load() : chunk_max;
    return bytes < lo ? lo : bytes > hi ? hi : bytes;
}

// blocks per chunk: whole 64-block waves; an eighth of a context's share of the call (eight chunks in flight per
// context), within [kChunkMin, chunk_max] bytes of payload
static uint64_t chunk_blocks_for(uint64_t nblocks, uint32_t block_size, uint64_t chunk_max, size_t nctx)
{
    const uint64_t bytes = clamp_chunk_bytes((nblocks * (uint64_t)block_size + kSlots * nctx - 1) / (kSlots * nctx), chunk_max);
    uint64_t cb = (bytes + block_size - 1) / block_size;
    cb = (cb + 63) / 64 * 64;
    return cb < nblocks ? cb : nblocks;
}

// cb rounded up to whole frames of frame_blocks blocks, for the layouts whose frames do not divide a 64-block wave (the
// record layout): a chunk's layout is then its part of the whole input's.  The chunk's last wave may be partly filled,
// which the coders take.  A frame count that divides cb leaves it as it is.
static uint64_t chunk_blocks_framed(uint64_t cb, uint64_t nblocks, uint32_t frame_blocks)
{
    if (frame_blocks <= 1 || cb >= nblocks)
        return cb;
    cb = (cb + frame_blocks - 1) / frame_blocks * frame_blocks;
    return cb < nblocks ? cb : nblocks;
}

// ---- what the contexts of one call share ---------------------------------------------------------
// A call's units are its chunks (redux_encode_blocks ...) or its groups of inputs (the `_v` calls), in block order.  The
// ledger keeps the call's first error, the first unit with a non-OK block, and -- encode -- where each unit's streams go in
// the dense output: known once every earlier unit's size is, whichever context coded it.
struct Ledger {
    std::mutex              m;
    std::condition_variable cv;
    bool                    abort = false;
    int                     error = REDUX_OK;
    uint64_t                bad_unit = ~0ull; // first unit (in block order) with a non-OK block, and that status
    int                     bad_status = REDUX_OK;
    std::vector<uint64_t>   size, prefix; // prefix[k] = sum of size[0..k): valid for k <= prefix_n
    std::vector<char>       known;
    uint64_t                prefix_n = 0;

    explicit Ledger(uint64_t nunits) : size(nunits, 0), prefix(nunits + 1, 0), known(nunits, 0) {}
    void fail(int rc)
    {
        std::lock_guard<std::mutex> l(m);
        if (error == REDUX_OK)
            error = rc;
        abort = true;
        cv.notify_all();
    }
    bool aborted()
    {
        std::lock_guard<std::mutex> l(m);
        return abort;
    }
    void publish(uint64_t k, uint64_t bytes)
    {
        std::lock_guard<std::mutex> l(m);
        size[k]  = bytes;
        known[k] = 1;
        while (prefix_n < size.size() && known[prefix_n]) {
            prefix[prefix_n + 1] = prefix[prefix_n] + size[prefix_n];
            prefix_n++;
        }
        cv.notify_all();
    }
    // bytes of all units before k, once they are all published; nothing if the call fails meanwhile
    std::optional<uint64_t> base_of(uint64_t k)
    {
        std::unique_lock<std::mutex> l(m);
        cv.wait(l, [&] { return abort || prefix_n >= k; });
        if (abort)
            return std::nullopt;
        return prefix[k];
    }
    void note_bad(uint64_t k, int st)
    {
        std::lock_guard<std::mutex> l(m);
        if (k < bad_unit) {
            bad_unit   = k;
            bad_status = st;
        }
    }
    int result() const { return error != REDUX_OK ? error : bad_status; }
};

// ---- one call over its contexts ------------------------------------------------------------------
// Takes the call's contexts (take_contexts), sizes the call for their number -- plan(nctx, &nunits) -- and runs
// work(ctx, ledger, first, stride) for the units first, first + stride, ... of each context: context 0 on the calling thread,
// every other on a thread of its own.  Returns the call's error, or failing that the first non-OK unit status in block order.
template <typename Plan, typename Work>
static int run_fleet(Plan &&plan, Work &&work)
{
    std::vector<Ctx *> ctx;
    std::vector<std::unique_lock<std::mutex>> locks;
    int rc = take_contexts(ctx, locks);
    if (rc != REDUX_OK)
        return rc;
    CallerDevice caller; // (every context makes its own device current on the thread that drives it)
    uint64_t     nunits = 0;
    if ((rc = plan(ctx.size(), nunits)) != REDUX_OK)
        return rc;
    Ledger L(nunits);
    const uint64_t nctx = ctx.size() < nunits ? ctx.size() : nunits; // (a call of one unit uses one context)
    std::vector<std::thread> th;
    for (uint64_t d = 1; d < nctx; d++)
        th.emplace_back([&, d] { work(*ctx[d], L, d, nctx); });
    work(*ctx[0], L, 0, nctx);
    for (auto &t : th)
        t.join();
    for (Ctx *c : ctx) {
        if (c->ready)
            (void)hipSetDevice(c->device);
        ctx_trim_locked(*c);
    }
    return L.result();
}

// ---- the chunk pipeline of one context -----------------------------------------------------------
// What became of a chunk's results: rc (REDUX_OK: in caller memory), or `aborted`: not placed because the call failed
// elsewhere (its error is that failure's).
struct Placed {
    int  rc      = REDUX_OK;
    bool aborted = false;
};

// hand-over between the issuing thread and the drain thread of one context
struct Handover {
    std::mutex              m;
    std::condition_variable cv;
    uint64_t                issued = 0;  // chunks whose device work has been enqueued
    uint64_t                drained = 0; // chunks whose results are in the caller's memory
    bool                    abort = false;
};

static void *slot_ws(const Slot &s) { return (void *)(((uintptr_t)s.d_ws.p + 255) & ~(uintptr_t)255); }

// a small result array -> its pinned mirror, on the chunk's stream
static bool fetch_small(Buf &h, const Buf &d, uint64_t bytes, hipStream_t s)
{
    return hipMemcpyAsync(h.p, d.p, bytes, hipMemcpyDeviceToHost, s) == hipSuccess;
}

// The chunks first, first + stride, ... of the call on context c (the calling thread of the call holds c.mu).  What differs by
// direction is the Op's (EncodeChunks, DecodeChunks): grow (what a slot holds), stage and launch (chunk k's H2D and kernels),
// fetch (its small result arrays) and place (its results -> caller memory).
template <typename Op>
static void run_chunks_on_ctx(Ctx &c, const Op &op, Ledger &L, uint64_t first, uint64_t stride)
{
    int rc = ctx_init_locked(c); // (makes c.want HIP's current device on this thread)
    if (rc != REDUX_OK)
        return L.fail(rc);
    const uint64_t mine   = first < op.nchunks ? (op.nchunks - first + stride - 1) / stride : 0; // chunks of this context
    const int      nslots = (int)(mine < (uint64_t)kSlots ? mine : (uint64_t)kSlots);
    for (int i = 0; i < nslots; i++)
        if ((rc = op.grow(c, c.slot[i])) != REDUX_OK)
            return L.fail(rc);
    c.trace.assign(mine * 4, 0.0);
    c.t0 = now_s();
    Handover H; // j = ordinal of a chunk within this context: slot and stream j % 8
    // ---- drain thread: results of chunk k -> caller memory -------------------------------------
    std::thread drain([&] {
        (void)hipSetDevice(c.device);
        for (uint64_t j = 0; j < mine; j++) {
            {
                std::unique_lock<std::mutex> l(H.m);
                H.cv.wait(l, [&] { return H.issued > j || H.abort; });
                if (H.abort)
                    return;
            }
            const uint64_t k = first + j * stride, b0 = k * op.cb, nb = (b0 + op.cb <= op.nblocks ? op.cb : op.nblocks - b0);
            Slot          &s  = c.slot[j % kSlots];
            hipStream_t    st = c.stream[j % kStreams]; // idle once the chunk's event has fired
            Placed         r;
            if (hipEventSynchronize(s.done) != hipSuccess || !op.fetch(s, st, nb) || hipStreamSynchronize(st) != hipSuccess)
                r.rc = REDUX_IO_ERROR;
            c.trace[j * 4 + 2] = now_s() - c.t0;
            if (r.rc == REDUX_OK) {
                if (((const int32_t *)s.h_sum.p)[0] != REDUX_OK)
                    L.note_bad(k, ((const int32_t *)s.h_sum.p)[0]);
                r = op.place(c, s, k, b0, nb, L);
            }
            c.trace[j * 4 + 3] = now_s() - c.t0;
            if (r.rc != REDUX_OK)
                L.fail(r.rc);
            const bool stop = r.rc != REDUX_OK || r.aborted;
            std::lock_guard<std::mutex> l(H.m);
            H.drained = j + 1;
            if (stop)
                H.abort = true;
            H.cv.notify_all();
            if (stop)
                return;
        }
    });

    // ---- issuing side (this thread): stage, H2D, kernels ----------------------------------------
    {
        CopyPool pool(kCopyThreads - 1);
        uint64_t piece_no = 0;
        for (uint64_t j = 0; j < mine; j++) {
            {
                std::unique_lock<std::mutex> l(H.m); // the slot's previous chunk must be in the caller's memory
                H.cv.wait(l, [&] { return H.abort || j < (uint64_t)kSlots || H.drained + kSlots > j; });
                if (H.abort)
                    break;
            }
            if (L.aborted())
                break;
            c.trace[j * 4 + 0] = now_s() - c.t0;
            const uint64_t k = first + j * stride, b0 = k * op.cb, nb = (b0 + op.cb <= op.nblocks ? op.cb : op.nblocks - b0);
            Slot          &s  = c.slot[j % kSlots];
            hipStream_t    st = c.stream[j % kStreams];
            auto issue = [&]() -> int {
                int r = op.stage(c, s, st, b0, nb, pool, piece_no);
                if (r != REDUX_OK)
                    return r;
                HOST_TRY(hipMemsetAsync(s.d_sum.p, 0, 8, st));
                if ((r = op.launch(s, st, b0, nb)) != REDUX_OK)
                    return r;
                // (the small result arrays are fetched by the drain thread once the event has fired: a D2H
                // enqueued here would sit in the in-order SDMA queue until this chunk's kernels end, with
                // every other chunk's drain copies stuck behind it -- measured: 15-20 ms stalls)
                HOST_TRY(hipEventRecord(s.done, st));
                return REDUX_OK;
            };
            rc = issue();
            c.trace[j * 4 + 1] = now_s() - c.t0;
            if (rc != REDUX_OK)
                L.fail(rc);
            std::lock_guard<std::mutex> l(H.m);
            if (rc != REDUX_OK)
                H.abort = true;
            else
                H.issued = j + 1;
            H.cv.notify_all();
            if (rc != REDUX_OK)
                break;
        }
        {
            std::lock_guard<std::mutex> l(H.m); // (left early because another context failed: release the drain thread)
            if (H.issued < mine)
                H.abort = true;
            H.cv.notify_all();
        }
    }
    drain.join();
    for (int i = 0; i < kStreams; i++) // nothing of this call stays in flight
        (void)hipStreamSynchronize(c.stream[i]);
}

template <typename Op>
static int run_chunks(Op &op)
{
    return run_fleet([&](size_t nctx, uint64_t &nunits) { return op.plan(nctx, nunits); },
                     [&](Ctx &c, Ledger &L, uint64_t first, uint64_t stride) { run_chunks_on_ctx(c, op, L, first, stride); });
}

// ---- the coder of a chunked call ---------------------------------------------------------------
// Chosen by the call's ABI entry point (redux_hip.hip): the workspace and stream room a chunk needs, and the launch of one
// chunk's kernels on its stream, between the slot's buffers.
struct EncodeCoder {
    // workspace and stream-area bytes for chunks of at most max_in input bytes (`several`: the call has more than one chunk)
    std::function<void(uint64_t max_in, bool several, uint64_t &ws_bytes, uint64_t &bound)> size;
    // len bytes in s.d_in -> streams in s.d_out (room: bound), s.d_off, s.d_st, s.d_sum
    std::function<int(Slot &s, uint64_t len, uint64_t bound, void *ws, uint64_t ws_bytes, hipStream_t st)> launch;
};

struct DecodeCoder {
    std::function<uint64_t(uint64_t cb)> workspace; // bytes for chunks of at most cb blocks
    // nb streams in s.d_in (offsets s.d_off) -> out_bytes bytes in s.d_out, s.d_sz, s.d_st, s.d_sum; d_in_used may be null
    std::function<int(Slot &s, uint64_t nb, uint64_t out_bytes, void *d_in_used, void *ws, uint64_t ws_bytes, hipStream_t st)> launch;
    // where block b of s.d_out is: false = at b * block_size, s.d_sz[b] bytes; true = out_bytes of original-order bytes, cut
    // into blocks of block_size (the byte-plane layout, after its inverse transform)
    bool original_order = false;
};

// Segment-static coding (include/redux_hip.h): the call's tables, u32[nseg][E][258] in caller memory, travel per chunk through
// the slot's d_tab / h_tab as the CRCs travel through d_crc / h_crc.  Chunks are whole segments of G blocks, so chunk
// [b0, b0 + nb) owns the tables (b0 / G) E .. of the call: encode's coder leaves them in d_tab and they are fetched with the
// chunk's small arrays; decode stages them to d_tab before its coder runs.  cum == null: the call has no tables.
struct SegmentTablesIo {
    uint32_t *cum = nullptr;
    uint32_t  E = 1, G = 0;
    uint64_t chunk_blocks(uint64_t cb, uint64_t nblocks) const // cb rounded up to whole segments
    {
        if (!cum || cb >= nblocks)
            return cb;
        cb = (cb + G - 1) / G * G;
        return cb < nblocks ? cb : nblocks;
    }
    uint64_t bytes(uint64_t nb) const { return cum ? (nb + G - 1) / G * E * 258ull * 4 : 0; } // of a chunk's tables (nb >= 1)
    uint32_t *at(uint64_t b0) const { return cum + b0 / G * E * 258ull; }
};

// The XOR-against-base filter (include/redux_hip.h): the call's base, base_len bytes of caller memory next to its len bytes
// of original data.  A chunk that holds original bytes [o0, o0 + n) owns base[o0 .. min(o0 + n, base_len)): it is staged
// through the pinned ring into the slot's d_base, which only these calls allocate, and the chunk's coder finds it there with
// its length in s.base_len.  on false: the call has no base.
struct BaseIo {
    const uint8_t *p   = nullptr;
    uint64_t       len = 0;
    bool           on  = false;
    uint64_t share(uint64_t o0, uint64_t n) const { return !on || len <= o0 ? 0 : len - o0 < n ? len - o0 : n; }
    int stage(Ctx &c, Slot &s, hipStream_t st, uint64_t o0, uint64_t n, CopyPool &pool, uint64_t &piece_no) const
    {
        s.base_len = share(o0, n);
        return s.base_len ? stage_h2d(c, pool, piece_no, s.d_base.p, p + o0, s.base_len, st) : REDUX_OK;
    }
};

// Mixed layouts (include/redux_hip.h): the call's unit table, u8 per unit of 8 blocks in caller memory, travels per chunk
// through the slot's d_stf / h_stf as the stored flags do (the two never meet in one call).  Chunks are whole 64-block waves,
// so chunk [b0, b0 + nb) owns table bytes b0 / 8 .. : encode fetches them with the chunk's small arrays when its coder chose
// them (given false) and stages them in front of its coder when the caller dictates them (given true); decode stages them.
struct UnitTableIo {
    uint8_t *table = nullptr; // null: the call has no unit table
    bool     given = false;
    static uint64_t bytes(uint64_t nb) { return (nb + 7) / 8; }
    uint8_t *at(uint64_t b0) const { return table + b0 / 8; }
    int stage(Slot &s, hipStream_t st, uint64_t b0, uint64_t nb) const
    {
        memcpy(s.h_stf.p, at(b0), bytes(nb));
        HOST_TRY(hipMemcpyAsync(s.d_stf.p, s.h_stf.p, bytes(nb), hipMemcpyHostToDevice, st));
        return REDUX_OK;
    }
};

// ================================================================================================
// encode: chunk k = blocks [k * cb, k * cb + nb) of the input -> its streams at their place in the dense output
// ================================================================================================
struct EncodeChunks {
    const uint8_t     *in;
    uint64_t           in_len;
    uint32_t           block_size;
    uint8_t           *out;
    uint64_t           out_cap;
    uint64_t          *out_offsets;
    int32_t           *block_status;
    const EncodeCoder &coder;
    uint32_t          *block_crc; // may be null: CRC-32 of each input block (redux_crc.hpp), on the staged chunk
    uint8_t           *stored;    // may be null: the stored-block flags the coder leaves in s.d_stf (redux_store.hpp)
    SegmentTablesIo    tables;    // cum may be null: the segment tables the coder leaves in s.d_tab
    BaseIo             base;      // on: the chunk's share of the base, staged to s.d_base next to its input
    UnitTableIo        units;     // table may be null: the unit table of the mixed layouts, in s.d_stf
    uint32_t           frame_blocks = 1; // chunks are whole frames of so many blocks (chunk_blocks_framed)
    uint64_t           nblocks = 0, cb = 0, nchunks = 0, max_in = 0, ws_bytes = 0, bound = 0;

    int plan(size_t nctx, uint64_t &n)
    {
        nblocks = redux_block_count(in_len, block_size);
        cb      = tables.chunk_blocks(chunk_blocks_for(nblocks, block_size, kEncChunkMax, nctx), nblocks);
        cb      = chunk_blocks_framed(cb, nblocks, frame_blocks);
        nchunks = n = (nblocks + cb - 1) / cb;
        max_in  = cb * (uint64_t)block_size < in_len ? cb * (uint64_t)block_size : in_len; // bytes of the largest chunk
        coder.size(max_in, nchunks > 1, ws_bytes, bound);
        return REDUX_OK;
    }
    uint64_t len_of(uint64_t b0, uint64_t nb) const // input bytes of a chunk
    {
        const uint64_t o0 = b0 * (uint64_t)block_size;
        return o0 + nb * (uint64_t)block_size <= in_len ? nb * (uint64_t)block_size : in_len - o0;
    }
    int grow(Ctx &c, Slot &s) const
    {
        const int rc = grow_bufs(c, {{&s.d_in, max_in + 16}, {&s.d_ws, ws_bytes + 256}, {&s.d_out, bound + 16}, {&s.d_off, (cb + 1) * 8},
                                     {&s.d_st, cb * 4}, {&s.d_sum, 8}, {&s.h_off, (cb + 1) * 8}, {&s.h_st, cb * 4}, {&s.h_sum, 8}});
        if (rc == REDUX_OK && (stored || units.table)) {
            const int r2 = grow_bufs(c, {{&s.d_stf, cb}, {&s.h_stf, cb}});
            if (r2 != REDUX_OK)
                return r2;
        }
        if (rc == REDUX_OK && tables.cum) {
            const int r2 = grow_bufs(c, {{&s.d_tab, tables.bytes(cb)}, {&s.h_tab, tables.bytes(cb)}});
            if (r2 != REDUX_OK)
                return r2;
        }
        if (rc == REDUX_OK && base.on) {
            const int r2 = grow_buf(c, s.d_base, max_in + 16);
            if (r2 != REDUX_OK)
                return r2;
        }
        return rc != REDUX_OK || !block_crc ? rc : grow_bufs(c, {{&s.d_crc, cb * 4}, {&s.h_crc, cb * 4}});
    }
    int stage(Ctx &c, Slot &s, hipStream_t st, uint64_t b0, uint64_t nb, CopyPool &pool, uint64_t &piece_no) const
    {
        if (units.table && units.given) {
            const int r2 = units.stage(s, st, b0, nb);
            if (r2 != REDUX_OK)
                return r2;
        }
        const int rc = stage_h2d(c, pool, piece_no, s.d_in.p, in + b0 * (uint64_t)block_size, len_of(b0, nb), st);
        return rc != REDUX_OK || !base.on ? rc : base.stage(c, s, st, b0 * (uint64_t)block_size, len_of(b0, nb), pool, piece_no);
    }
    int launch(Slot &s, hipStream_t st, uint64_t b0, uint64_t nb) const
    {
        if (block_crc) { // the staged input, before any transform
            const int rc = redux_crc32_blocks_dev(s.d_in.p, len_of(b0, nb), block_size, s.d_crc.p, st);
            if (rc != REDUX_OK)
                return rc;
        }
        return coder.launch(s, len_of(b0, nb), bound, slot_ws(s), ws_bytes, st);
    }
    bool fetch(Slot &s, hipStream_t st, uint64_t nb) const
    {
        return fetch_small(s.h_off, s.d_off, (nb + 1) * 8, st) && fetch_small(s.h_st, s.d_st, nb * 4, st) &&
               fetch_small(s.h_sum, s.d_sum, 8, st) && (!block_crc || fetch_small(s.h_crc, s.d_crc, nb * 4, st)) &&
               (!stored || fetch_small(s.h_stf, s.d_stf, nb, st)) &&
               (!units.table || units.given || fetch_small(s.h_stf, s.d_stf, units.bytes(nb), st)) &&
               (!tables.cum || fetch_small(s.h_tab, s.d_tab, tables.bytes(nb), st));
    }
    Placed place(Ctx &c, Slot &s, uint64_t k, uint64_t b0, uint64_t nb, Ledger &L) const
    {
        const uint64_t *ho    = (const uint64_t *)s.h_off.p;
        const uint64_t  total = ho[nb];
        L.publish(k, total); // then wait for the sizes of all earlier chunks (other contexts' included)
        const std::optional<uint64_t> base = L.base_of(k);
        if (!base)
            return {REDUX_OK, true};
        if (*base + total > out_cap)
            return {REDUX_OUTPUT_TOO_SMALL};
        const int rc = total ? drain_d2h(c, out + *base, s.d_out.p, total) : REDUX_OK;
        if (rc != REDUX_OK)
            return {rc};
        for (uint64_t i = 0; i <= nb; i++)
            out_offsets[b0 + i] = *base + ho[i]; // (entry b0 + nb is written again, with the same value, by the next chunk)
        if (block_status)
            memcpy(block_status + b0, s.h_st.p, nb * 4);
        if (block_crc)
            memcpy(block_crc + b0, s.h_crc.p, nb * 4);
        if (stored)
            memcpy(stored + b0, s.h_stf.p, nb);
        if (units.table && !units.given)
            memcpy(units.at(b0), s.h_stf.p, units.bytes(nb));
        if (tables.cum)
            memcpy(tables.at(b0), s.h_tab.p, tables.bytes(nb));
        return {};
    }
};

static int encode_blocks(const uint8_t *in, uint64_t in_len, uint32_t block_size, uint8_t *out, uint64_t out_cap,
                         uint64_t *out_offsets, int32_t *block_status, const EncodeCoder &coder, uint32_t *block_crc = nullptr,
                         uint8_t *stored = nullptr, SegmentTablesIo tables = {}, BaseIo base = {}, UnitTableIo units = {},
                         uint32_t frame_blocks = 1)
{
    EncodeChunks op{in, in_len, block_size, out, out_cap, out_offsets, block_status, coder, block_crc, stored, tables, base, units,
                    frame_blocks};
    return run_chunks(op);
}

// ================================================================================================
// decode: chunk k = blocks [k * cb, k * cb + nb) -> out[k * cb * block_size ..), chunk_out bytes of it
// ================================================================================================
struct DecodeChunks {
    const uint8_t     *in;
    const uint64_t    *in_offsets;
    uint64_t           nblocks;
    uint32_t           block_size;
    uint8_t           *out;
    uint64_t           out_len; // bytes the call writes: nblocks * block_size, or out[0 .. out_len) exactly in the planes layout
    uint32_t          *out_sizes;
    int32_t           *block_status;
    uint64_t          *in_used;
    const DecodeCoder &coder;
    uint32_t          *block_crc; // may be null: CRC-32 of what each block decoded to (redux_crc.hpp), on the chunk's output
    const uint8_t     *stored;    // may be null: stored-block flags, staged to s.d_stf with the chunk's offsets (redux_store.hpp)
    SegmentTablesIo    tables;    // cum may be null: the segment tables, staged to s.d_tab with the chunk's offsets
    BaseIo             base;      // on: the share of the base that lies next to the chunk's output, staged to s.d_base
    UnitTableIo        units;     // table may be null: the unit table of the mixed layouts, staged to s.d_stf
    uint32_t           frame_blocks = 1; // chunks are whole frames of so many blocks (chunk_blocks_framed)
    uint64_t           cb = 0, nchunks = 0, ws_bytes = 0, max_in = 0;

    int plan(size_t nctx, uint64_t &n)
    {
        cb       = tables.chunk_blocks(chunk_blocks_for(nblocks, block_size, kDecChunkMax, nctx), nblocks);
        cb       = chunk_blocks_framed(cb, nblocks, frame_blocks);
        nchunks  = n = (nblocks + cb - 1) / cb;
        ws_bytes = coder.workspace(cb);
        for (uint64_t k = 0; k < nchunks; k++) {
            const uint64_t b0 = k * cb, b1 = (b0 + cb <= nblocks ? b0 + cb : nblocks);
            if (in_offsets[b1] < in_offsets[b0])
                return REDUX_INVALID_INPUT;
            const uint64_t len = in_offsets[b1] - in_offsets[b0];
            max_in = len > max_in ? len : max_in;
        }
        return REDUX_OK;
    }
    uint64_t chunk_out(uint64_t b0, uint64_t nb) const // bytes a chunk's blocks write into out
    {
        const uint64_t full = nb * (uint64_t)block_size, o = b0 * (uint64_t)block_size;
        return out_len - o < full ? out_len - o : full;
    }
    int grow(Ctx &c, Slot &s) const
    {
        const uint64_t used = in_used ? cb * 8 : 8;
        const int      rc   = grow_bufs(c, {{&s.d_in, max_in + 32}, {&s.d_ws, ws_bytes + 256}, {&s.d_out, cb * (uint64_t)block_size + 16},
                                            {&s.d_off, (cb + 1) * 8}, {&s.d_sz, cb * 4}, {&s.d_st, cb * 4}, {&s.d_sum, 8}, {&s.d_used, used},
                                            {&s.h_off, (cb + 1) * 8}, {&s.h_sz, cb * 4}, {&s.h_st, cb * 4}, {&s.h_sum, 8}, {&s.h_used, used}});
        if (rc == REDUX_OK && (stored || units.table)) {
            const int r2 = grow_bufs(c, {{&s.d_stf, cb}, {&s.h_stf, cb}});
            if (r2 != REDUX_OK)
                return r2;
        }
        if (rc == REDUX_OK && tables.cum) {
            const int r2 = grow_bufs(c, {{&s.d_tab, tables.bytes(cb)}, {&s.h_tab, tables.bytes(cb)}});
            if (r2 != REDUX_OK)
                return r2;
        }
        if (rc == REDUX_OK && base.on) {
            const int r2 = grow_buf(c, s.d_base, cb * (uint64_t)block_size + 16);
            if (r2 != REDUX_OK)
                return r2;
        }
        return rc != REDUX_OK || !block_crc ? rc : grow_bufs(c, {{&s.d_crc, cb * 4}, {&s.h_crc, cb * 4}});
    }
    int stage(Ctx &c, Slot &s, hipStream_t st, uint64_t b0, uint64_t nb, CopyPool &pool, uint64_t &piece_no) const
    {
        // the chunk's offsets, rebased to the chunk's first byte (the pinned mirror of the previous
        // chunk in this slot has been consumed: that chunk is drained)
        const uint64_t i0 = in_offsets[b0];
        uint64_t      *ho = (uint64_t *)s.h_off.p;
        for (uint64_t i = 0; i <= nb; i++) {
            if (in_offsets[b0 + i] < i0 || (i && in_offsets[b0 + i] < in_offsets[b0 + i - 1]))
                return REDUX_INVALID_INPUT;
            ho[i] = in_offsets[b0 + i] - i0;
        }
        HOST_TRY(hipMemcpyAsync(s.d_off.p, ho, (nb + 1) * 8, hipMemcpyHostToDevice, st));
        if (stored) {
            memcpy(s.h_stf.p, stored + b0, nb);
            HOST_TRY(hipMemcpyAsync(s.d_stf.p, s.h_stf.p, nb, hipMemcpyHostToDevice, st));
        }
        if (tables.cum) {
            memcpy(s.h_tab.p, tables.at(b0), tables.bytes(nb));
            HOST_TRY(hipMemcpyAsync(s.d_tab.p, s.h_tab.p, tables.bytes(nb), hipMemcpyHostToDevice, st));
        }
        if (units.table) {
            const int r2 = units.stage(s, st, b0, nb);
            if (r2 != REDUX_OK)
                return r2;
        }
        const int rc = stage_h2d(c, pool, piece_no, s.d_in.p, in + i0, in_offsets[b0 + nb] - i0, st);
        return rc != REDUX_OK || !base.on ? rc : base.stage(c, s, st, b0 * (uint64_t)block_size, chunk_out(b0, nb), pool, piece_no);
    }
    int launch(Slot &s, hipStream_t st, uint64_t b0, uint64_t nb) const
    {
        const int rc = coder.launch(s, nb, chunk_out(b0, nb), in_used ? s.d_used.p : nullptr, slot_ws(s), ws_bytes, st);
        if (rc != REDUX_OK || !block_crc)
            return rc;
        return coder.original_order ? redux_crc32_blocks_dev(s.d_out.p, chunk_out(b0, nb), block_size, s.d_crc.p, st)
                                    : redux_crc32_sizes_dev(s.d_out.p, nb, block_size, s.d_sz.p, s.d_crc.p, st);
    }
    bool fetch(Slot &s, hipStream_t st, uint64_t nb) const
    {
        return fetch_small(s.h_sz, s.d_sz, nb * 4, st) && fetch_small(s.h_st, s.d_st, nb * 4, st) &&
               fetch_small(s.h_sum, s.d_sum, 8, st) && (!in_used || fetch_small(s.h_used, s.d_used, nb * 8, st)) &&
               (!block_crc || fetch_small(s.h_crc, s.d_crc, nb * 4, st));
    }
    Placed place(Ctx &c, Slot &s, uint64_t, uint64_t b0, uint64_t nb, Ledger &) const
    {
        const uint64_t n  = chunk_out(b0, nb);
        const int      rc = n ? drain_d2h(c, out + b0 * (uint64_t)block_size, s.d_out.p, n) : REDUX_OK;
        if (rc != REDUX_OK)
            return {rc};
        memcpy(out_sizes + b0, s.h_sz.p, nb * 4);
        if (block_status)
            memcpy(block_status + b0, s.h_st.p, nb * 4);
        if (in_used)
            memcpy(in_used + b0, s.h_used.p, nb * 8);
        if (block_crc)
            memcpy(block_crc + b0, s.h_crc.p, nb * 4);
        return {};
    }
};

static int decode_blocks(const uint8_t *in, const uint64_t *in_offsets, uint64_t nblocks, uint32_t block_size, uint8_t *out,
                         uint64_t out_len, uint32_t *out_sizes, int32_t *block_status, uint64_t *in_used, const DecodeCoder &coder,
                         uint32_t *block_crc = nullptr, const uint8_t *stored = nullptr, SegmentTablesIo tables = {}, BaseIo base = {},
                         UnitTableIo units = {}, uint32_t frame_blocks = 1)
{
    DecodeChunks op{in, in_offsets, nblocks, block_size, out, out_len, out_sizes, block_status, in_used, coder, block_crc, stored, tables,
                    base, units, frame_blocks};
    return run_chunks(op);
}

// ================================================================================================
// byte histogram of host memory (the frequency table of the static model)
//
// The input is staged chunk by chunk through the pinned ring into the slots of the CURRENT device's context (the fleet of
// redux_host_set_devices is not used: the result is 2 KiB, there is nothing to spread), and k_byte_hist of each chunk adds
// into one u64[256] on the device.  Chunk j runs on stream j % kStreams and slot j % kSlots, so the staging of a chunk
// into a slot is ordered after the kernel that read the slot's previous chunk.  One read-back at the end.
// E > 1 (redux_plane_static_tables): counts is u64[E][256], the counts of the byte-plane layout's blocks b by b mod E.  The
// chunks are then whole frames of E * block_size bytes, so that a chunk's layout is its part of the whole input's and its
// first block is a multiple of E; the layout of each chunk goes into the slot's workspace and k_plane_hist counts that.
// pairs (redux_context_static_tables, E = 1): counts is u64[256][256], the (previous byte, byte) counts inside blocks of
// block_size; the chunks are whole blocks and k_context_hist counts each.
// ================================================================================================
static int byte_histogram(const uint8_t *in, uint64_t in_len, uint64_t *counts, uint32_t block_size = 0, uint32_t E = 1,
                          bool pairs = false)
{
    Ctx *cp  = nullptr;
    int  dev = 0;
    int  rc  = ctx_of_current_device(&cp, &dev);
    if (rc != REDUX_OK)
        return rc;
    Ctx                        &c = *cp;
    std::lock_guard<std::mutex> l(c.mu);
    c.want = dev;
    if ((rc = ctx_init_locked(c)) != REDUX_OK)
        return rc;
    uint64_t chunk = clamp_chunk_bytes((in_len + kSlots - 1) / kSlots, kEncChunkMax);
    chunk = (chunk + 65535) / 65536 * 65536; // (whole 64 KiB: the test hook's 1-byte chunks become 64 KiB)
    if (E > 1) {
        const uint64_t frame = (uint64_t)E * block_size;
        chunk = (chunk + frame - 1) / frame * frame;
    }
    if (pairs) {
        chunk = (chunk + block_size - 1) / block_size * block_size;
        if (chunk > in_len && in_len) // (one chunk: no more room than the input, whatever the block size)
            chunk = in_len;
    }
    const uint64_t nchunks = (in_len + chunk - 1) / chunk;
    const int      nslots  = (int)(nchunks < (uint64_t)kSlots ? nchunks : (uint64_t)kSlots);
    const size_t   cbytes  = pairs ? (size_t)65536 * 8 : (size_t)E * 256 * 8;
    if ((rc = grow_buf(c, c.d_counts, cbytes)) != REDUX_OK)
        return rc;
    for (int i = 0; i < nslots; i++) {
        if ((rc = grow_buf(c, c.slot[i].d_in, chunk + 16)) != REDUX_OK)
            return rc;
        if (E > 1 && (rc = grow_buf(c, c.slot[i].d_ws, chunk + 16)) != REDUX_OK)
            return rc;
    }
    HOST_TRY(hipMemsetAsync(c.d_counts.p, 0, cbytes, c.stream[0]));
    HOST_TRY(hipStreamSynchronize(c.stream[0])); // (the other streams do not wait for stream 0)
    {
        CopyPool pool(kCopyThreads - 1);
        uint64_t piece_no = 0;
        for (uint64_t j = 0; j < nchunks && rc == REDUX_OK; j++) {
            const uint64_t o = j * chunk, n = in_len - o < chunk ? in_len - o : chunk;
            hipStream_t    st = c.stream[j % kStreams];
            void          *d  = c.slot[j % kSlots].d_in.p;
            rc = stage_h2d(c, pool, piece_no, d, in + o, n, st);
            if (rc == REDUX_OK && E > 1) {
                void *x = c.slot[j % kSlots].d_ws.p;
                if ((rc = redux_planes_dev(d, x, n, block_size, E, 0, st)) == REDUX_OK)
                    rc = redux_plane_histogram_dev(x, n, block_size, E, c.d_counts.p, nullptr, 0, st);
            } else if (rc == REDUX_OK && pairs)
                rc = redux_context_histogram_dev(d, n, block_size, c.d_counts.p, st);
            else if (rc == REDUX_OK)
                rc = redux_histogram_dev(d, n, c.d_counts.p, nullptr, 0, st);
        }
    }
    for (int i = 0; i < kStreams; i++) // nothing of this call stays in flight
        if (hipStreamSynchronize(c.stream[i]) != hipSuccess && rc == REDUX_OK)
            rc = REDUX_IO_ERROR;
    if (rc == REDUX_OK && hipMemcpy(counts, c.d_counts.p, cbytes, hipMemcpyDeviceToHost) != hipSuccess)
        rc = REDUX_IO_ERROR;
    ctx_trim_locked(c);
    return rc;
}

// ================================================================================================
// per-block CRC-32 of host memory (redux_crc32_blocks)
//
// As byte_histogram: the CURRENT device's context, chunks of whole blocks staged through the pinned ring, chunk j on stream
// and slot j % kSlots (stream order keeps a slot's staging behind the kernel that read its previous chunk), each chunk's
// k_crc32 into the slot's d_crc and its CRCs copied straight into the caller's array on the same stream.
// ================================================================================================
static int crc32_blocks(const uint8_t *in, uint64_t in_len, uint32_t block_size, uint32_t *crc)
{
    Ctx *cp  = nullptr;
    int  dev = 0;
    int  rc  = ctx_of_current_device(&cp, &dev);
    if (rc != REDUX_OK)
        return rc;
    Ctx                        &c = *cp;
    std::lock_guard<std::mutex> l(c.mu);
    c.want = dev;
    if ((rc = ctx_init_locked(c)) != REDUX_OK)
        return rc;
    const uint64_t nblocks = redux_block_count(in_len, block_size);
    uint64_t       cb      = clamp_chunk_bytes((in_len + kSlots - 1) / kSlots, kEncChunkMax) / block_size;
    cb                     = cb < 1 ? 1 : cb;
    const uint64_t nchunks = (nblocks + cb - 1) / cb, chunk = cb * block_size;
    const int      nslots  = (int)(nchunks < (uint64_t)kSlots ? nchunks : (uint64_t)kSlots);
    for (int i = 0; i < nslots; i++)
        if ((rc = grow_bufs(c, {{&c.slot[i].d_in, (chunk < in_len ? chunk : in_len) + 16}, {&c.slot[i].d_crc, cb * 4}})) != REDUX_OK)
            return rc;
    {
        CopyPool pool(kCopyThreads - 1);
        uint64_t piece_no = 0;
        for (uint64_t j = 0; j < nchunks && rc == REDUX_OK; j++) {
            const uint64_t o = j * chunk, n = in_len - o < chunk ? in_len - o : chunk, b0 = j * cb;
            const uint64_t nb = nblocks - b0 < cb ? nblocks - b0 : cb;
            hipStream_t    st = c.stream[j % kStreams];
            Slot          &s  = c.slot[j % kSlots];
            rc = stage_h2d(c, pool, piece_no, s.d_in.p, in + o, n, st);
            if (rc == REDUX_OK)
                rc = redux_crc32_blocks_dev(s.d_in.p, n, block_size, s.d_crc.p, st);
            if (rc == REDUX_OK && hipMemcpyAsync(crc + b0, s.d_crc.p, nb * 4, hipMemcpyDeviceToHost, st) != hipSuccess)
                rc = REDUX_IO_ERROR;
        }
    }
    for (int i = 0; i < kStreams; i++) // nothing of this call stays in flight
        if (hipStreamSynchronize(c.stream[i]) != hipSuccess && rc == REDUX_OK)
            rc = REDUX_IO_ERROR;
    ctx_trim_locked(c);
    return rc;
}

// ================================================================================================
// many independent inputs in one call (redux_encode_blocks_v / redux_decode_blocks_v)
//
// Consecutive inputs are packed into GROUPS of at most kVGroupBytes; a group is staged into HBM with every input at a
// 16-byte boundary (so that the fast kernels apply), coded by ONE launch over its block table and copied back.  The point
// of these calls is many small inputs -- the reference's corpus harness, 36 files of 4 KB - 4 MB, is one group -- where
// what counts is that all blocks share a launch.  A batch of several groups is dealt over the fleet (redux_host_set_devices):
// group k runs on context k mod n, each context on its first slot and its own thread; the encoder's dense output keeps
// block order through a ledger of group sizes.
// ================================================================================================
constexpr uint64_t kVGroupBytes = 512ull << 20;

// One group of consecutive inputs = one launch.  first_block = number of its first block; nb its blocks.
struct VGroup {
    uint64_t i0, i1, first_block, nb;
};

// inputs [0, ninputs) -> groups of at most kVGroupBytes of (16-byte padded) payload each
static std::vector<VGroup> v_groups(const uint64_t *len, uint64_t ninputs, uint32_t block_size)
{
    std::vector<VGroup> g;
    uint64_t            blk = 0;
    const uint64_t      cap = g_chunk_max.load() ? g_chunk_max.load() : kVGroupBytes; // (redux_host_set_chunk_bytes: a harness drives many groups through a small batch)
    for (uint64_t i0 = 0; i0 < ninputs;) {
        uint64_t i1 = i0, pos = 0;
        do {
            pos += (len[i1] + 15) & ~15ull;
            i1++;
        } while (i1 < ninputs && pos + len[i1] <= cap);
        const uint64_t nb = redux_block_count_v(len + i0, i1 - i0, block_size);
        g.push_back({i0, i1, blk, nb});
        blk += nb;
        i0 = i1;
    }
    return g;
}

struct EncVCall {
    const redux_params *p;
    const uint8_t      *in;
    const uint64_t     *in_off, *in_len;
    uint32_t            block_size;
    uint8_t            *out;
    uint64_t            out_cap;
    uint64_t           *out_offsets;
    int32_t            *block_status;
};

static int encode_v_group(Ctx &c, const EncVCall &E, const VGroup &G, uint64_t gi, Ledger &L, CopyPool &pool, uint64_t &piece_no)
{
    int         rc;
    Slot       &s  = c.slot[0];
    hipStream_t st = c.stream[0];
    std::vector<uint64_t> doff;
    uint64_t              pos = 0;
    for (uint64_t i = G.i0; i < G.i1; i++) {
        doff.push_back(pos);
        pos += (E.in_len[i] + 15) & ~15ull;
    }
    if (pos > 0xFFFFFFFFull) // (one input of 4 GiB or more: lane offsets are 32-bit; redux_encode_blocks takes it)
        return REDUX_UNSUPPORTED;
    const uint64_t nb = G.nb;
    const uint64_t ne = redux_block_table_v(doff.data(), E.in_len + G.i0, G.i1 - G.i0, E.block_size, nullptr); // entries: blocks + idle lanes
    std::vector<redux_block> tbl(ne);
    redux_block_table_v(doff.data(), E.in_len + G.i0, G.i1 - G.i0, E.block_size, tbl.data());
    const uint64_t ws_bytes = redux_encode_workspace_bytes(E.p, ne * (uint64_t)E.block_size, E.block_size);
    const uint64_t bound    = nb * redux_encode_slot_bytes(E.p, E.block_size);
    if ((rc = grow_bufs(c, {{&s.d_in, pos + 16}, {&s.d_ws, ws_bytes + 256}, {&s.d_out, bound + 16}, {&s.d_off, (nb + 1) * 8},
                            {&s.d_st, nb * 4}, {&s.d_sum, 8}, {&s.d_tab, ne * sizeof(redux_block)}, {&s.h_off, (nb + 1) * 8},
                            {&s.h_st, nb * 4}, {&s.h_sum, 8}, {&s.h_tab, ne * sizeof(redux_block)}})))
        return rc;
    memcpy(s.h_tab.p, tbl.data(), ne * sizeof(redux_block));
    HOST_TRY(hipMemcpyAsync(s.d_tab.p, s.h_tab.p, ne * sizeof(redux_block), hipMemcpyHostToDevice, st));
    for (uint64_t k = 0; k < G.i1 - G.i0; k++)
        if (E.in_len[G.i0 + k] &&
            (rc = stage_h2d(c, pool, piece_no, (uint8_t *)s.d_in.p + doff[k], E.in + E.in_off[G.i0 + k], E.in_len[G.i0 + k], st)))
            return rc;
    HOST_TRY(hipMemsetAsync(s.d_sum.p, 0, 8, st));
    if ((rc = redux_encode_blocks_v_dev(E.p, s.d_in.p, pos, s.d_tab.p, ne, nb, E.block_size, REDUX_V_ALIGNED16, s.d_out.p, bound, s.d_off.p,
                                        s.d_st.p, s.d_sum.p, slot_ws(s), ws_bytes, st)))
        return rc;
    HOST_TRY(hipMemcpyAsync(s.h_off.p, s.d_off.p, (nb + 1) * 8, hipMemcpyDeviceToHost, st));
    HOST_TRY(hipMemcpyAsync(s.h_st.p, s.d_st.p, nb * 4, hipMemcpyDeviceToHost, st));
    HOST_TRY(hipMemcpyAsync(s.h_sum.p, s.d_sum.p, 8, hipMemcpyDeviceToHost, st));
    HOST_TRY(hipStreamSynchronize(st));
    const uint64_t *ho    = (const uint64_t *)s.h_off.p;
    const uint64_t  total = ho[nb];
    L.publish(gi, total);
    const std::optional<uint64_t> out_base = L.base_of(gi);
    if (!out_base) // (another group failed)
        return REDUX_OK;
    if (*out_base + total > E.out_cap)
        return REDUX_OUTPUT_TOO_SMALL;
    if (total && (rc = drain_d2h(c, E.out + *out_base, s.d_out.p, total)))
        return rc;
    for (uint64_t i = 0; i <= nb; i++) // (entry nb is also the next group's entry 0: the same value from either side)
        E.out_offsets[G.first_block + i] = *out_base + ho[i];
    if (E.block_status)
        memcpy(E.block_status + G.first_block, s.h_st.p, nb * 4);
    if (((const int32_t *)s.h_sum.p)[0] != REDUX_OK)
        L.note_bad(gi, ((const int32_t *)s.h_sum.p)[0]);
    return REDUX_OK;
}

struct DecVCall {
    const redux_params *p;
    const uint8_t      *in;
    const uint64_t     *in_offsets;
    uint8_t            *out;
    const uint64_t     *out_off, *out_len;
    uint32_t            block_size;
    uint32_t           *out_sizes;
    int32_t            *block_status;
};

static int decode_v_group(Ctx &c, const DecVCall &D, const VGroup &G, uint64_t gi, Ledger &L, CopyPool &pool, uint64_t &piece_no)
{
    int         rc;
    Slot       &s  = c.slot[0];
    hipStream_t st = c.stream[0];
    std::vector<uint64_t> doff;
    uint64_t              pos = 0;
    for (uint64_t i = G.i0; i < G.i1; i++) {
        doff.push_back(pos);
        pos += (D.out_len[i] + 15) & ~15ull;
    }
    const uint64_t nb = G.nb, blk_base = G.first_block;
    const uint64_t ne = redux_block_table_v(doff.data(), D.out_len + G.i0, G.i1 - G.i0, D.block_size, nullptr);
    std::vector<redux_block> tbl(ne);
    redux_block_table_v(doff.data(), D.out_len + G.i0, G.i1 - G.i0, D.block_size, tbl.data()); // offset = where the block goes, length = its room
    const uint64_t sb0 = D.in_offsets[blk_base];
    for (uint64_t i = 0; i < nb; i++)
        if (D.in_offsets[blk_base + i + 1] < D.in_offsets[blk_base + i])
            return REDUX_INVALID_INPUT;
    const uint64_t len_in = D.in_offsets[blk_base + nb] - sb0;
    if (len_in && !D.in)
        return REDUX_INVALID_INPUT;
    const uint64_t wsb = redux_decode_workspace_bytes(D.p, ne, D.block_size);
    if ((rc = grow_bufs(c, {{&s.d_in, len_in + 32}, {&s.d_ws, wsb + 256}, {&s.d_out, pos + 16}, {&s.d_off, (nb + 1) * 8},
                            {&s.d_sz, nb * 4}, {&s.d_st, nb * 4}, {&s.d_sum, 8}, {&s.d_tab, ne * sizeof(redux_block)},
                            {&s.h_off, (nb + 1) * 8}, {&s.h_sz, nb * 4}, {&s.h_st, nb * 4}, {&s.h_sum, 8},
                            {&s.h_tab, ne * sizeof(redux_block)}})))
        return rc;
    uint64_t *ho = (uint64_t *)s.h_off.p;
    for (uint64_t i = 0; i <= nb; i++)
        ho[i] = D.in_offsets[blk_base + i] - sb0;
    memcpy(s.h_tab.p, tbl.data(), ne * sizeof(redux_block));
    HOST_TRY(hipMemcpyAsync(s.d_off.p, ho, (nb + 1) * 8, hipMemcpyHostToDevice, st));
    HOST_TRY(hipMemcpyAsync(s.d_tab.p, s.h_tab.p, ne * sizeof(redux_block), hipMemcpyHostToDevice, st));
    if (len_in && (rc = stage_h2d(c, pool, piece_no, s.d_in.p, D.in + sb0, len_in, st)))
        return rc;
    HOST_TRY(hipMemsetAsync(s.d_sum.p, 0, 8, st));
    if ((rc = redux_decode_blocks_v_dev(D.p, s.d_in.p, s.d_off.p, s.d_tab.p, ne, nb, D.block_size, REDUX_V_ALIGNED16, s.d_out.p, pos,
                                        s.d_sz.p, s.d_st.p, s.d_sum.p, slot_ws(s), wsb, st)))
        return rc;
    HOST_TRY(hipMemcpyAsync(s.h_sz.p, s.d_sz.p, nb * 4, hipMemcpyDeviceToHost, st));
    HOST_TRY(hipMemcpyAsync(s.h_st.p, s.d_st.p, nb * 4, hipMemcpyDeviceToHost, st));
    HOST_TRY(hipMemcpyAsync(s.h_sum.p, s.d_sum.p, 8, hipMemcpyDeviceToHost, st));
    HOST_TRY(hipStreamSynchronize(st));
    const uint32_t *hs = (const uint32_t *)s.h_sz.p;
    // an input's blocks are back to back in both buffers: whole runs of full blocks leave as one copy
    uint64_t b = 0;
    for (uint64_t k = 0; k < G.i1 - G.i0; k++) {
        const uint64_t cnt = redux_block_count(D.out_len[G.i0 + k], D.block_size);
        for (uint64_t j = 0; j < cnt;) {
            uint64_t run = 0, j1 = j;
            while (j1 < cnt) { // extend over blocks that decoded to a whole block_size; the first shorter one ends the run
                const uint32_t sz = hs[b + j1];
                run += sz;
                j1++;
                if (sz != D.block_size)
                    break;
            }
            if (run && (rc = drain_d2h(c, D.out + D.out_off[G.i0 + k] + j * (uint64_t)D.block_size,
                                       (const uint8_t *)s.d_out.p + doff[k] + j * (uint64_t)D.block_size, run)))
                return rc;
            j = j1;
        }
        b += cnt;
    }
    memcpy(D.out_sizes + blk_base, hs, nb * 4);
    if (D.block_status)
        memcpy(D.block_status + blk_base, s.h_st.p, nb * 4);
    if (((const int32_t *)s.h_sum.p)[0] != REDUX_OK)
        L.note_bad(gi, ((const int32_t *)s.h_sum.p)[0]);
    return REDUX_OK;
}

// group_fn(c, g, ledger, pool, piece_no) for every group, the groups dealt round-robin over the call's contexts; each context
// runs its groups one after the other, on its first slot and stream
template <typename F>
static int run_groups(uint64_t ngroups, F &&group_fn)
{
    return run_fleet([&](size_t, uint64_t &nunits) { nunits = ngroups; return REDUX_OK; },
                     [&](Ctx &c, Ledger &L, uint64_t first, uint64_t stride) {
                         int rc = ctx_init_locked(c); // (makes c.want HIP's current device on this thread)
                         if (rc != REDUX_OK)
                             return L.fail(rc);
                         CopyPool pool(kCopyThreads - 1);
                         uint64_t piece_no = 0;
                         for (uint64_t g = first; g < ngroups && !L.aborted(); g += stride)
                             if ((rc = group_fn(c, g, L, pool, piece_no)) != REDUX_OK)
                                 return L.fail(rc);
                         (void)hipStreamSynchronize(c.stream[0]);
                     });
}

static int encode_blocks_v(const redux_params *p, const uint8_t *in, const uint64_t *in_off, const uint64_t *in_len, uint64_t ninputs,
                           uint32_t block_size, uint8_t *out, uint64_t out_cap, uint64_t *out_offsets, int32_t *block_status)
{
    const std::vector<VGroup> groups = v_groups(in_len, ninputs, block_size);
    const EncVCall            E{p, in, in_off, in_len, block_size, out, out_cap, out_offsets, block_status};
    return run_groups(groups.size(), [&](Ctx &c, uint64_t g, Ledger &L, CopyPool &pool, uint64_t &piece_no) {
        return encode_v_group(c, E, groups[g], g, L, pool, piece_no);
    });
}

static int decode_blocks_v(const redux_params *p, const uint8_t *in, const uint64_t *in_offsets, uint8_t *out, const uint64_t *out_off,
                           const uint64_t *out_len, uint64_t ninputs, uint32_t block_size, uint32_t *out_sizes, int32_t *block_status)
{
    const std::vector<VGroup> groups = v_groups(out_len, ninputs, block_size);
    const DecVCall            D{p, in, in_offsets, out, out_off, out_len, block_size, out_sizes, block_status};
    return run_groups(groups.size(), [&](Ctx &c, uint64_t g, Ledger &L, CopyPool &pool, uint64_t &piece_no) {
        return decode_v_group(c, D, groups[g], g, L, pool, piece_no);
    });
}

} // namespace host
} // namespace redux
