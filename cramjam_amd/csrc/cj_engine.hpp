// cj_engine.hpp — private host-side state shared by engine.hip (C-ABI, batch submission) and frame.hip
// (framed formats on top of the batch engine).  Not part of the C-ABI.
#pragma once
#include "cj_common.hpp"

#include <algorithm>
#include <atomic>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <mutex>
#include <string>
#include <thread>
#include <vector>

namespace cj {

std::string& hip_err_slot();     // thread-local text behind cj_last_hip_error()

inline bool hip_ok(hipError_t e, const char* what) {
    if (e == hipSuccess) return true;
    hip_err_slot() = std::string(what) + ": " + hipGetErrorString(e);
    (void)hipGetLastError();
    return false;
}
#define HIP_TRY(expr, ret) do { if (!cj::hip_ok((expr), #expr)) return (ret); } while (0)

// Owners: each releases what it holds in its destructor (on the device that is current then: cj_engine_destroy sets it) and is not copyable.
struct DevBuf {
    void* p = nullptr;
    size_t cap = 0;
    DevBuf() = default;
    DevBuf(const DevBuf&) = delete;
    DevBuf& operator=(const DevBuf&) = delete;
    ~DevBuf() { release(); }
    bool reserve(size_t n) { return n <= cap || reserve_exact(n + n / 4 + 4096); }
    // for buffers of gigabytes (the record areas of big chunks): no growth slack
    bool reserve_exact(size_t n) {
        if (n <= cap) return true;
        release();
        if (!hip_ok(hipMalloc(&p, n), "hipMalloc")) { p = nullptr; return false; }
        cap = n;
        return true;
    }
    void release() { if (p) (void)hipFree(p); p = nullptr; cap = 0; }
};

struct PinnedBuf {          // page-locked host staging (full PCIe rate, truly asynchronous copies)
    uint8_t* p = nullptr;
    size_t cap = 0;
    PinnedBuf() = default;
    PinnedBuf(const PinnedBuf&) = delete;
    PinnedBuf& operator=(const PinnedBuf&) = delete;
    ~PinnedBuf() { release(); }
    bool reserve(size_t n) {
        if (n <= cap) return true;
        release();
        size_t want = n + n / 4 + 4096;
        if (!hip_ok(hipHostMalloc((void**)&p, want, hipHostMallocDefault), "hipHostMalloc")) { p = nullptr; return false; }
        cap = want;
        return true;
    }
    void release() { if (p) (void)hipHostFree(p); p = nullptr; cap = 0; }
};

// an event / a stream, created where it is first needed (h == nullptr until then); reads as the handle
template <class H, hipError_t (*Destroy)(H)>
struct Owned {
    H h = nullptr;
    Owned() = default;
    Owned(Owned&& o) noexcept : h(o.h) { o.h = nullptr; }
    Owned(const Owned&) = delete;
    Owned& operator=(const Owned&) = delete;
    ~Owned() { if (h) (void)Destroy(h); }
    operator H() const { return h; }
};
struct Event : Owned<hipEvent_t, hipEventDestroy> {
    bool create() { return h || hip_ok(hipEventCreateWithFlags(&h, hipEventDisableTiming), "hipEventCreateWithFlags"); }
};
struct Stream : Owned<hipStream_t, hipStreamDestroy> {
    bool create() { return h || hip_ok(hipStreamCreateWithFlags(&h, hipStreamNonBlocking), "hipStreamCreateWithFlags"); }
};

// A scratch area that the calls on one engine share (its buffers are listed where cj_engine declares it): `mu` serialises the host
// side of the calls, `free` is recorded behind the last kernel that used the area.
struct Scratch {
    std::mutex mu;
    Event free;
};
// One turn at a scratch.  The lock is held for the whole call.  The constructor makes `s` wait for the previous user (rc: 0 or
// CJ_E_*); a buffer of the scratch that has to grow is reallocated only once that user has finished (reserve: 0 or CJ_E_*); done(s)
// hands the scratch to the next turn — a call that returns an error before it records nothing.
struct ScratchTurn {
    Scratch& sc;
    std::lock_guard<std::mutex> lock;
    int rc;
    ScratchTurn(Scratch& sc_, hipStream_t s) : sc(sc_), lock(sc_.mu), rc(open(s)) {}
    int wait_host() {
        if (sc.free) HIP_TRY(hipEventSynchronize(sc.free), CJ_E_NO_DEVICE);
        return 0;
    }
    template <class Buf>
    int reserve(Buf& buf, size_t bytes) {
        if (bytes > buf.cap && wait_host() != 0) return CJ_E_NO_DEVICE;
        return buf.reserve(bytes) ? 0 : CJ_E_OOM;
    }
    int done(hipStream_t s) {
        HIP_TRY(hipGetLastError(), CJ_E_NO_DEVICE);
        HIP_TRY(hipEventRecord(sc.free, s), CJ_E_NO_DEVICE);
        return 0;
    }
private:
    int open(hipStream_t s) {
        if (!sc.free) return sc.free.create() ? 0 : CJ_E_NO_DEVICE;
        HIP_TRY(hipStreamWaitEvent(s, sc.free, 0), CJ_E_NO_DEVICE);
        return 0;
    }
};

// The bytes of a scratch that one slice of a batch may take: a default that the tests lower through a cj_debug_*_budget export
// (0 = back to the default; returns the previous value)
struct SlotBudget {
    const uint64_t def;
    std::atomic<uint64_t> cur;
    explicit SlotBudget(uint64_t d) : def(d), cur(d) {}
    uint64_t load() const { return cur.load(); }
    uint64_t exchange(uint64_t bytes) { return cur.exchange(bytes ? bytes : def); }
};

// host-side pack/scatter of many small buffers is memcpy-bound on one core (~20 GB/s); split it over a few threads
template <class F>
void parallel_chunks(size_t n, size_t total_bytes, F&& fn) {
    unsigned t = total_bytes > (32u << 20) ? std::min(16u, std::max(1u, std::thread::hardware_concurrency())) : 1u;
    if (t <= 1 || n < 2 * t) { fn(0, n); return; }
    std::vector<std::thread> th;
    const size_t per = (n + t - 1) / t;
    for (unsigned k = 0; k < t; k++) {
        const size_t a = k * per, b = std::min(n, a + per);
        if (a >= b) break;
        th.emplace_back([=, &fn] { fn(a, b); });
    }
    for (auto& x : th) x.join();
}

}  // namespace cj

// LOCK ORDER of the engine's mutexes: mu -> fb -> {scratch, zstd_slots, deflate_slots, zstd_enc_slots}.  A host batch stages under `mu` and takes the
// scratches inside it.  A frame batch holds its `fb` turn while cj::launch takes `scratch` for its LZ4 / Snappy blocks (decompress).  A
// container batch (Blosc, BGZF, ORC, Parquet) holds its `fb` turn while cj::inner_decode or cj::inner_encode (cj_codecs.hpp) takes
// `scratch`, `zstd_slots`, `deflate_slots` or `zstd_enc_slots` for its entries, once per call — the encoders once per turn of slots
// (cj_container.hpp: for_turns).  The inner ones are taken one after another,
// never one inside another, and no path takes two of the graph's mutexes the other way round; `dict_stage` is taken alone or under `mu` only.  The three
// slotted scratches (`zstd_slots`, `deflate_slots`, `zstd_enc_slots`) are taken in one place, cj::slot_slices below.  The table
// of every entry's turns: DESIGN.md §2; two streams and two threads per scratch: tests/test_scratch_streams_gpu.py.
struct cj_engine {                 // (members are destroyed last to first: the streams outlive every buffer and event)
    int device = 0;
    cj::Stream stream;
    cj::Stream stream_back;        // batch_host_sliced: the copies back to the host (the engine's stream keeps uploading and decoding the next slice)
    std::mutex mu;                 // serialises host-batch staging on this engine
    cj::DevBuf d_in, d_out, d_meta;
    cj::Scratch scratch;           // the workgroup decoders: LZ4 parse->decode scratch (sync points, per-chunk meta), record tables, big-chunk areas
    cj::DevBuf d_sync, d_pmeta, d_lanelist;   // d_lanelist: word [2] = the workgroup decoder's chunk counter
    cj::PinnedBuf h_in, h_out, h_res;   // h_res: the results of a sliced host batch (engine.hip: batch_host_sliced)
    std::vector<cj::Event> slice_ev;
    std::vector<uint64_t> h_meta;
    cj::DevBuf d_frame;            // frame.hip: assembled / staged framed stream
    cj::DevBuf d_tab;              // LDS decoder variant 2: per-workgroup record tables
    cj::DevBuf d_biglist, d_bigrecs, d_bigmisc, d_bigslabtab;   // chunks of 64 KiB .. 256 KiB in a device batch (big_chunks.hpp, CJ_FLAG_BIG_CHUNKS): record areas; list + summaries + slab items; the slab decoder's tables
    cj::PinnedBuf h_count;         // pinned words: the number of big chunks of the last flagged batches, copied back without waiting (engine.hip plan_big)
    cj::Event big_ev[8];           // ... one event per slot (the copy has landed)
    uint32_t big_obs[8] = {};      // ... the counts that have
    int big_state[8] = {};         // 0 = empty, 1 = copy in flight, 2 = count known
    int big_next = 0;
    cj::DevBuf d_big, d_bigtab;    // large.hip: parse scratch / record tables of one large stream (under `mu`)
    int n_cu = 0;
    cj::Scratch fb;                // frame_batch.hip, blosc_batch.hip, bgzf_batch.hip, orc_batch.hip, parquet_batch.hip: batches of framed streams / Blosc chunks / BGZF streams / ORC streams / Parquet chunks — frame table, block rows and decode slots, its staging
    cj::DevBuf d_fb;
    cj::PinnedBuf h_fb;
    cj::Scratch dict_stage;        // lz4_dict.hip: dictionary compress — the staged `dictionary tail | chunk` slots and their rows
    cj::DevBuf d_dict_stage;
    cj::DevBuf d_dict;             // ... the dictionary of a host batch (under `mu`)
    cj::Scratch deflate_slots;     // deflate_encode.hip: the workgroups' sequence-record slots of a compress batch
    cj::DevBuf d_deflate_slots;
    cj::Scratch zstd_slots;        // zstd.hip: the wavefronts' literal slots of a decode batch
    cj::DevBuf d_zstd_slots;
    cj::Scratch zstd_enc_slots;    // zstd_encode.hip: the workgroups' record and literal slots of a compress batch
    cj::DevBuf d_zstd_enc_slots;
};

namespace cj {
// Every DevBuf and PinnedBuf of cj_engine, once (tests/test_scratch_contents_model.py holds this list to the struct above and to the table
// of DESIGN.md §5.10b): its name, the member, the mutex its users hold (kOwnMu: `mu` alone; else the Scratch, whose `free` event its last
// user recorded), and whether it CARRIES STATE between calls by design — such a buffer is not scratch and is never filled.  The
// cj_debug_scratch_* exports (engine.hip) walk this one table, so what they name, fill and read back cannot disagree.
enum BufOwner { kOwnMu, kOwnScratch, kOwnFb, kOwnDictStage, kOwnDeflateSlots, kOwnZstdSlots, kOwnZstdEncSlots };
struct EngineBuf {
    const char* name;
    DevBuf cj_engine::* dev;       // one of the two is set
    PinnedBuf cj_engine::* pin;
    BufOwner owner;
    bool carries_state;
};
#define CJ_DEV(m, own) {#m, &cj_engine::m, nullptr, own, false}
#define CJ_PIN(m, own, state) {#m, nullptr, &cj_engine::m, own, state}
inline constexpr EngineBuf kEngineBufs[] = {
    CJ_DEV(d_in, kOwnMu), CJ_DEV(d_out, kOwnMu), CJ_DEV(d_meta, kOwnMu),
    CJ_DEV(d_sync, kOwnScratch), CJ_DEV(d_pmeta, kOwnScratch), CJ_DEV(d_lanelist, kOwnScratch),
    CJ_PIN(h_in, kOwnMu, false), CJ_PIN(h_out, kOwnMu, false), CJ_PIN(h_res, kOwnMu, false),
    CJ_DEV(d_frame, kOwnMu), CJ_DEV(d_tab, kOwnScratch),
    CJ_DEV(d_biglist, kOwnScratch), CJ_DEV(d_bigrecs, kOwnScratch), CJ_DEV(d_bigmisc, kOwnScratch), CJ_DEV(d_bigslabtab, kOwnScratch),
    CJ_PIN(h_count, kOwnScratch, true),       // plan_big (engine.hip) reads the counts that EARLIER calls posted here
    CJ_DEV(d_big, kOwnMu), CJ_DEV(d_bigtab, kOwnMu),
    CJ_DEV(d_fb, kOwnFb), CJ_PIN(h_fb, kOwnFb, false),
    CJ_DEV(d_dict_stage, kOwnDictStage), CJ_DEV(d_dict, kOwnMu),
    CJ_DEV(d_deflate_slots, kOwnDeflateSlots), CJ_DEV(d_zstd_slots, kOwnZstdSlots), CJ_DEV(d_zstd_enc_slots, kOwnZstdEncSlots),
};
#undef CJ_DEV
#undef CJ_PIN
constexpr int kEngineBufCount = (int)(sizeof(kEngineBufs) / sizeof(kEngineBufs[0]));
inline Scratch* buf_scratch(cj_engine* e, BufOwner o) {
    switch (o) {
    case kOwnScratch: return &e->scratch;
    case kOwnFb: return &e->fb;
    case kOwnDictStage: return &e->dict_stage;
    case kOwnDeflateSlots: return &e->deflate_slots;
    case kOwnZstdSlots: return &e->zstd_slots;
    case kOwnZstdEncSlots: return &e->zstd_enc_slots;
    default: return nullptr;
    }
}

constexpr size_t kGridChunks = (size_t)1 << 22;     // chunks per launch of a wavefront-per-chunk kernel: a grid stays below 2^32 threads
cj_engine* default_engine();     // lazily created on device 0 (tuning builds: $CJ_DEVICE); nullptr when no device is usable
// submit one batch on stream s (slices very large decode batches); 0 or CJ_E_*
int launch(cj_engine* e, cj_codec codec, cj_op op, const BatchArgs& a, hipStream_t s);
void fill_args(BatchArgs& a, uint32_t flags, size_t n, const uint8_t* in_base, const uint64_t* in_off,
               const uint64_t* in_len, uint8_t* out_base, const uint64_t* out_off, const uint64_t* out_cap,
               int64_t* result);

// The u64 rows of a batch of n chunks, one after another from a base pointer (a host copy such as e->h_meta, or the device one in e->d_meta)
struct BatchRows {
    uint64_t* in_off; uint64_t* in_len; uint64_t* out_off; uint64_t* out_cap; int64_t* result;
    uint64_t* end;               // the first row after them
    size_t n;
    // chunks [a0, a0 + k) of the same rows (end stays the whole batch's)
    BatchRows sub(size_t a0, size_t k) const { return {in_off + a0, in_len + a0, out_off + a0, out_cap + a0, result + a0, end, k}; }
};
inline BatchRows batch_rows(uint64_t* base, size_t n) {
    return {base, base + n, base + 2 * n, base + 3 * n, reinterpret_cast<int64_t*>(base + 4 * n), base + 5 * n, n};
}
inline void fill_args(BatchArgs& a, uint32_t flags, const uint8_t* in_base, uint8_t* out_base, const BatchRows& r) {
    fill_args(a, flags, r.n, in_base, r.in_off, r.in_len, out_base, r.out_off, r.out_cap, r.result);
}

// ---- launches of the kernels that give every wavefront (or lane) one chunk ---------------------------------------------------------
size_t grid_chunks();            // kGridChunks, unless cj_debug_grid_chunks has lowered it (engine.hip)
inline dim3 wave_grid(size_t n_chunks) { return dim3((unsigned)((n_chunks + kWavesPerBlock - 1) / kWavesPerBlock)); }
inline dim3 lane_grid(size_t n) { return dim3((unsigned)((n + kBlockThreads - 1) / kBlockThreads)); }
// the 16-byte step of every table and slot inside a scratch buffer
__host__ __device__ constexpr uint64_t up16(uint64_t x) { return (x + 15u) & ~(uint64_t)15u; }
// A batch of n chunks in slices of at most `per`: launch(a) with the BatchArgs of each slice in turn — its rows begin at the slice's
// first chunk (out_off / out_cap may be null: a size query), the base pointers are the batch's
template <class F>
void for_slices(size_t n, size_t per, uint32_t flags, const uint8_t* in_base, const uint64_t* in_off, const uint64_t* in_len, uint8_t* out_base,
                const uint64_t* out_off, const uint64_t* out_cap, int64_t* result, F&& launch) {
    for (size_t first = 0; first < n; first += per) {
        BatchArgs a;
        fill_args(a, flags, std::min(per, n - first), in_base, in_off + first, in_len + first, out_base, out_off ? out_off + first : nullptr,
                  out_cap ? out_cap + first : nullptr, result + first);
        launch(a);
    }
}
template <class F>
void for_slices(const BatchArgs& b, size_t per, F&& launch) {
    for_slices(b.n_chunks, per, b.flags, b.in_base, b.in_off, b.in_len, b.out_base, b.out_off, b.out_cap, b.result, launch);
}

// One turn at a slotted scratch (`sc`, its slots in `buf`): batch `b` in slices of as many chunks as there are slots — what `budget`
// bytes hold (one at least) and `limit` allows — launch(a, slots) for each; enqueue only (a turn that grows the slots waits for their
// previous user while it reallocates).  It is the one turn its caller takes at `sc`, under whatever outer turns the caller holds
// (LOCK ORDER above).  0 or CJ_E_*.
template <class F>
int slot_slices(Scratch& sc, DevBuf& buf, size_t slot_bytes, uint64_t budget, uint64_t limit, const BatchArgs& b, hipStream_t s, F&& launch) {
    const size_t per = (size_t)std::min<uint64_t>({b.n_chunks, std::max<uint64_t>(1, budget / slot_bytes), limit});
    ScratchTurn turn(sc, s);
    if (turn.rc != 0 || (turn.rc = turn.reserve(buf, per * slot_bytes)) != 0) return turn.rc;
    uint8_t* slots = (uint8_t*)buf.p;
    for_slices(b, per, [&](const BatchArgs& a) { launch(a, slots); });
    return turn.done(s);
}

#if defined(__HIPCC__)
// the workgroups of Kernel that one CU holds at once (asked once per kernel; 0: not known)
template <auto Kernel>
int resident_per_cu(int threads) {
    static std::atomic<int> known{-1};
    int v = known.load();
    if (v < 0) {
        v = 0;
        if (hipOccupancyMaxActiveBlocksPerMultiprocessor(&v, Kernel, threads, 0) != hipSuccess) { (void)hipGetLastError(); v = 0; }
        known.store(v);
    }
    return v;
}
// ... that the device holds at once, as the `limit` of slot_slices: a launch of more workgroups than that ends in a tail of a few of
// them.  Not known: no limit.  0 or CJ_E_*.
template <auto Kernel>
int resident_limit(cj_engine* e, int threads, uint64_t& limit) {
    if (e->n_cu == 0) HIP_TRY(hipDeviceGetAttribute(&e->n_cu, hipDeviceAttributeMultiprocessorCount, e->device), CJ_E_NO_DEVICE);
    const uint64_t resident = (uint64_t)resident_per_cu<Kernel>(threads) * (uint64_t)e->n_cu;
    limit = resident != 0 ? resident : ~0ull;
    return 0;
}
#endif
}  // namespace cj
