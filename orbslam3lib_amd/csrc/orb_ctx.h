// orb_ctx.h -- internal to liborbgpu.so: the context (orbgpu_ctx), its device buffers, the error
// and stream helpers and the two dispatch helpers shared by orb_runtime.cpp (create, ingest, the
// batch itself), orb_post.cpp (what runs after a batch) and orb_matchers.cpp (the ORBmatcher searches).
#pragma once
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstring>
#include <mutex>
#include <string>
#include <vector>

#include "../../include/orbgpu.h"
#include "orb_geometry.h"
#include "orb_kernels.h"
#include "orb_layout.h"

namespace orbgpu {

// Sets the calling thread's orbgpu_last_error message and returns code (orb_runtime.cpp).
int fail(int code, const std::string& msg);

#define HIP_TRY(expr)                                                                  \
    do {                                                                               \
        hipError_t e_ = (expr);                                                        \
        if (e_ != hipSuccess)                                                          \
            return fail(ORBGPU_ERR_HIP, std::string(#expr) + ": " + hipGetErrorString(e_)); \
    } while (0)

enum Stage { ST_RESIZE, ST_BLUR, ST_FAST48, ST_FAST, ST_FAST_TOP, ST_OCTREE, ST_ORIENT, ST_FINAL, ST_KNN,
             ST_STEREO, ST_GRID, ST_SBS, ST_SOA, ST_SBP, ST_FISHEYE, ST_TAIL, ST_COUNT };
// names as rocprofv3 shows the kernels (templates with their argument)
inline const char* const kStageNames[ST_COUNT] = {"k_blur_resize",    "k_blur",   "k_fast_cells<48>", "k_fast_cells<64>",
                                                  "k_fast_cells<80>", "k_octree", "k_orient_desc",    "k_finalize",
                                                  "k_knn2",           "k_stereo",  "k_undistort_grid",
                                                  "k_sbs_split",      "k_pack_soa",       "k_sbp",
                                                  "k_fisheye_stereo", "k_pyr_tail"};

// hipMalloc / hipFree on one thread while another thread captures a stream into a graph fails
// the allocation and invalidates the capture on this HIP (measured: two contexts run from two
// threads, test_two_threads_two_contexts_concurrently), whatever the capture mode.  Device
// allocations and graph captures of every context therefore take this one process-wide lock.
inline std::recursive_mutex& alloc_capture_mutex() {
    static std::recursive_mutex mu;  // recursive: context creation holds it around its allocations
    return mu;
}

// A device buffer of a context.  Every DevBuf registers itself in its context's list when it is
// constructed (there is no other constructor), so orbgpu_destroy releases all of them.
struct DevBuf {
    void* p = nullptr;
    size_t bytes = 0;
    explicit DevBuf(std::vector<DevBuf*>& owner) { owner.push_back(this); }
    DevBuf(const DevBuf&) = delete;
    DevBuf& operator=(const DevBuf&) = delete;
    int ensure(size_t n) {
        if (n <= bytes) return 0;
        std::lock_guard<std::recursive_mutex> lk(alloc_capture_mutex());
        release();
        if (hipMalloc(&p, n) != hipSuccess) return -1;
        bytes = n;
        return 0;
    }
    void release() {
        std::lock_guard<std::recursive_mutex> lk(alloc_capture_mutex());
        if (p) hipFree(p);
        p = nullptr;
        bytes = 0;
    }
    template <class T>
    T* as() const { return reinterpret_cast<T*>(p); }
};

struct Pending {
    int stage;
    hipEvent_t a, b;
};

// one sub-batch (whole stereo pairs when the batch is split) and the stream it runs on
struct Chunk { int img0, n; hipStream_t st; };

// Measurement knobs (launch shapes, stream counts, kernel variants, phase clocks) are read only
// when ORBGPU_DIAGNOSTICS=1 is set as well: a stray ORBGPU_* variable in a deployment never
// changes the product's kernel path.  Parsed once per context, in orbgpu_create, from the one
// table in orb_runtime.cpp (kKnobTable) that orbgpu_diagnostic_knobs reports from as well.
struct DiagKnobs {
    GeomKnobs geom;
    int streams = 0;            // ORBGPU_STREAMS: every sub stream is a chunk (0: the chunk policy)
    bool streams_forced = false;
    // stages launched once over the whole batch on the main stream (join before, fork after), so
    // their per-launch duration is their own; off by default: each join / fork costs ~30 us of
    // idle GPU per step (ORBGPU_ISOLATE=<stage bit mask> turns it on)
    unsigned isolate_mask = 0;
    bool stagger = true;        // ORBGPU_STAGGER=0: the chunks start every layout in lockstep
    bool oct_stamps = false;    // ORBGPU_OCT_STAMPS: octree phase clocks
    bool use_graph = true;      // ORBGPU_GRAPH=0 launches every kernel directly (A/B)
    bool knn_nosplit = false;   // ORBGPU_KNN_NOSPLIT: no split kNN2 launches
    bool no_fuse_out = false;   // ORBGPU_NO_FUSE_OUT: k_finalize assembles even without lapping areas
    int fast_small = -1;        // ORBGPU_FAST_SMALL: the small-list FAST kernel never (0) / always (1)
    bool fast_ovf_all = false;  // ORBGPU_FAST_OVF_ALL: every small-list cell through the overflow pass
};

// What a matcher's last call left on the device: result row r is over batch image image[r] (two_cam: and image[r] + 1).
struct MatchCover { std::vector<int32_t> image; bool two_cam = false; };

enum Search { S_SBP, S_TRACK, S_INIT, S_BOW, S_RELOC, S_TRI, S_FUSE, S_SIM3, S_BOWKF, S_COUNT };

// Where the results of a search's last call lie in its result buffer: exactly what its download reads
// (nullptr: the search has no such slot).
struct ResultSlots {
    int32_t *match = nullptr, *nmatches = nullptr;      // [row][row_cap], [row] (fuse: first, nfused)
    size_t row_cap = 0;                                 // entries of a match row
    int32_t* hist = nullptr;                            // [row][kRotBins]; sim3: the replay's stats [row][kSim3Stats]
    float* prev_out = nullptr;                          // init: [row][row_cap][2]
    int32_t *best_idx = nullptr, *best_dist = nullptr;  // fuse, sim3: [point row]
    uint8_t* code = nullptr;                            // fuse, sim3: [point row]; bowkf: [row][row_cap]
    short2* best = nullptr;                             // bowkf: [row][row_cap] {bestDist1, bestDist2}
};
struct SearchResult {
    DevBuf buf;  // never shared: one search's results outlive the other searches' calls
    ResultSlots at;
    MatchCover cover;
    std::vector<int32_t> point_off;  // fuse, sim3: pair p's point rows are [point_off[p], point_off[p + 1])
    SearchResult(std::vector<DevBuf*>& owner) : buf(owner) {}
};

// Device-to-host copy on the context's own stream, waited for before the call returns (the
// callers ran ctx_sync first, so the stream is idle and the copy sees every result).  Never a
// null-stream hipMemcpy: that would also order against other contexts' and torch's work.
#define D2H(dst, src, bytes)                                                               \
    do {                                                                                   \
        HIP_TRY(hipMemcpyAsync((dst), (src), (bytes), hipMemcpyDeviceToHost, c->stream));  \
        HIP_TRY(hipStreamSynchronize(c->stream));                                          \
    } while (0)

}  // namespace orbgpu

struct orbgpu_ctx {
    using DevBuf = orbgpu::DevBuf;
    orbgpu_params prm{};
    int device = 0;
    hipStream_t stream = nullptr;
    std::vector<hipStream_t> sub;  // sub-batch streams (sub[0] == stream)
    int max_w = 0, max_h = 0, max_images = 0;
    orbgpu::ScaleTables tab;
    orbgpu::DiagKnobs knobs;
    // geometry of the current image size (orb_geometry.h; plan.A with the device pointers bound)
    int gw = -1, gh = -1;
    orbgpu::GeomPlan plan;
    // device buffers: one line each, released by orbgpu_destroy through `bufs`
    std::vector<DevBuf*> bufs;
    DevBuf input{bufs}, pyr{bufs}, blur{bufs}, rtab{bufs}, cellkeys{bufs}, cellcnt{bufs}, octws{bufs}, lvlkey{bufs},
        lvlangle{bufs}, lvldesc{bufs}, lvlcnt{bufs}, status{bufs}, outkps{bufs}, outdesc{bufs}, outn{bufs},
        outmono{bufs}, laps{bufs}, midx1{bufs}, mdist1{bufs}, midx2{bufs}, mdist2{bufs}, mnq{bufs}, mpart{bufs},
        scratch{bufs}, octdbg{bufs}, fastovf{bufs}, strow{bufs}, stidx{bufs}, stur{bufs}, stdepth{bufs},
        stsad{bufs}, gxy{bufs}, gcell{bufs}, gstart{bufs}, gidx{bufs}, sbs{bufs}, soa{bufs}, m16{bufs},
        fel2r{bufs}, fer2l{bufs}, fedepth{bufs}, fep3d{bufs}, fecnt{bufs};
    float grid_bounds[4] = {0, 0, 0, 0}, grid_inv[2] = {0, 0};  // of the last undistort_grid
    // The ORBmatcher searches (orb_matchers.cpp).  `work` holds what dies with a call, for all nine: the
    // uploaded inputs and the kernels' scratch, laid out anew by every call (orb_layout.h).  Sharing it rests
    // on two facts: run_search waits for the search's stream before it returns, and a context is driven by
    // one thread, so no kernel of an earlier search reads `work` when the next one lays it out.  An error
    // path of run_search (a failed HIP call) returns before that wait; the next call's ensure may then free
    // `work` under what was enqueued, and the hipFree in DevBuf::ensure waits for the device, as it always has.
    DevBuf work{bufs};
    // What a download reads, one record per search: results stay until that search runs again.
    orbgpu::SearchResult res[orbgpu::S_COUNT] = {{bufs}, {bufs}, {bufs}, {bufs}, {bufs}, {bufs}, {bufs}, {bufs}, {bufs}};
    int soa_images = 0, soa_pairs = 0;  // coverage of the last orbgpu_pack_soa
    int grid_images = 0;   // images of the last orbgpu_undistort_grid_batch
    int stereo_pairs = 0;  // pairs of the last orbgpu_stereo_matches_batch
    int fisheye_pairs = 0;  // pairs of the last orbgpu_fisheye_stereo_batch
    hipEvent_t fork = nullptr;
    hipEvent_t ext_done = nullptr;  // work on a caller's stream (rejoin)
    // double-buffered input (orbgpu_upload_images_async): batch k reads slot in_slot while the copy
    // stream fills the other slot for batch k + 1; slot_free[j] = sub stream j's work enqueued before
    // the current batch began (everything that read the other slot), slot_ready = the async copy
    DevBuf input2{bufs};
    int in_slot = 0, pending_slot = -1;
    hipStream_t copy = nullptr;
    hipEvent_t slot_ready = nullptr;
    std::vector<hipEvent_t> slot_free;
    std::vector<hipEvent_t> join;  // one per sub stream
    bool serialize = false;  // profiling: every stage isolated
    // the captured launch sequences of one-stream batches (run_batch / run_batch_match), keyed by
    // {images, width, height, input slot, match pairs, stereo rows only}: one exec per key, so
    // alternating input slots (async uploads) or match variants replay instead of recapturing
    struct GraphRec { int key[7]; hipGraphExec_t exec; unsigned long long used; };
    std::vector<GraphRec> graphs;
    unsigned long long graph_tick = 0;
    bool last_fused = false;   // the last batch's outputs were assembled by k_orient_desc
    std::vector<int32_t> laps_host;  // lapping areas currently in `laps` (device), per image
    bool need_fork = true;           // the main stream holds work the sub streams must wait for
    bool restagger = false;          // the next batch re-staggers the chunks (after serialized runs)
    std::vector<hipEvent_t> stagger_ev;
    std::vector<orbgpu::Chunk> last_chunks;
    int last_images = 0, last_w = 0, last_h = 0, last_pairs = 0;
    // profiling: bit s of prof_mask brackets stage s launches with HIP events
    unsigned prof_mask = 0;
    std::vector<orbgpu::Pending> pending;
    std::vector<hipEvent_t> event_pool;
    double stage_ms[orbgpu::ST_COUNT] = {};
    long long stage_n[orbgpu::ST_COUNT] = {};
};

namespace orbgpu {

inline hipEvent_t take_event(orbgpu_ctx* c) {
    if (!c->event_pool.empty()) {
        hipEvent_t e = c->event_pool.back();
        c->event_pool.pop_back();
        return e;
    }
    hipEvent_t e;
    hipEventCreate(&e);
    return e;
}

template <class F>
int timed(orbgpu_ctx* c, int stage, hipStream_t s, F&& launch) {
    hipEvent_t a = nullptr, b = nullptr;
    const bool prof = (c->prof_mask >> stage) & 1u;
    if (prof) {
        a = take_event(c);
        b = take_event(c);
        hipEventRecord(a, s);
    }
    hipError_t e = launch();
    if (e != hipSuccess)
        return fail(ORBGPU_ERR_HIP, std::string(kStageNames[stage]) + ": " + hipGetErrorString(e));
    if (prof) {
        hipEventRecord(b, s);
        c->pending.push_back({stage, a, b});
    }
    return 0;
}

// Makes stream s wait for everything already enqueued on the context's other streams.
inline int join_all(orbgpu_ctx* c, hipStream_t s) {
    for (size_t k = 0; k < c->sub.size() && k < c->join.size(); ++k) {
        if (c->sub[k] == s) continue;
        HIP_TRY(hipEventRecord(c->join[k], c->sub[k]));
        HIP_TRY(hipStreamWaitEvent(s, c->join[k], 0));
    }
    return 0;
}

// After work was enqueued on a caller's stream s (not one of the context's own): the context's
// streams wait for it before they touch the buffers again (the next batch overwrites what it reads).
inline int rejoin(orbgpu_ctx* c, hipStream_t s) {
    for (hipStream_t t : c->sub)
        if (t == s) return 0;
    HIP_TRY(hipEventRecord(c->ext_done, s));
    HIP_TRY(hipStreamWaitEvent(c->stream, c->ext_done, 0));
    c->need_fork = true;
    return 0;
}

// Waits for the work of this context's own streams (the chunk streams, and the copy stream when
// with_copy) -- never the whole device: two contexts driven from two threads (one extractor per
// eye, Frame.cc:142-145) or torch work beside them do not wait for each other.  Work enqueued on
// a caller's stream is covered through rejoin(), which every such entry point calls.
inline int ctx_sync(orbgpu_ctx* c, bool with_copy = false) {
    HIP_TRY(hipSetDevice(c->device));
    for (hipStream_t s : c->sub) HIP_TRY(hipStreamSynchronize(s));
    if (with_copy && c->copy) HIP_TRY(hipStreamSynchronize(c->copy));
    return 0;
}

// True when p points into device memory (hipMalloc / torch CUDA tensors): the device entry
// points refuse host pointers instead of faulting on them.  A failed query leaves a sticky
// error for hipGetLastError, which the launchers read: clear it.
inline bool device_ptr(const void* p) {
    hipPointerAttribute_t at{};
    if (hipPointerGetAttributes(&at, p) != hipSuccess) {
        (void)hipGetLastError();
        return false;
    }
    return at.type == hipMemoryTypeDevice || at.type == hipMemoryTypeManaged;
}

// A per-image count the device wrote: k_finalize stores -5 (octree workspace overflow) or -2
// (output capacity) instead of a count; map them to the status the caller gets.
inline int count_status(int32_t nk) {
    if (nk == -5) return fail(ORBGPU_ERR_OVERFLOW, "device workspace overflow (octree)");
    if (nk < 0) return fail(ORBGPU_ERR_CAPACITY, "context output capacity exceeded");
    return 0;
}

inline DevBuf& in_buf(orbgpu_ctx* c, int slot) { return slot ? c->input2 : c->input; }
inline uint8_t* cur_input(orbgpu_ctx* c) { return in_buf(c, c->in_slot).as<uint8_t>(); }

// MatchArgs over the context's last batch: pair p = images 2p (query) and 2p + 1 (train)
// (orb_post.cpp; the captured batch + match graph of orb_runtime.cpp uses it too)
MatchArgs stereo_match_args(orbgpu_ctx* c, int stereo_only);

// True when `stage` of a batch split over `chunks` runs as one whole-batch launch (serialized
// profiling, or the stage's bit of ORBGPU_ISOLATE).
inline bool isolates(const orbgpu_ctx* c, const std::vector<Chunk>& chunks, int stage) {
    return chunks.size() > 1 && (c->serialize || ((c->knobs.isolate_mask >> stage) & 1u));
}

// The isolate bracket: every chunk stream joins chunk 0's, fn(chunk 0's stream) enqueues its
// work over the whole batch there, and the other chunk streams wait for it (fork back).
template <class F>
int isolated(orbgpu_ctx* c, const std::vector<Chunk>& chunks, F&& fn) {
    const hipStream_t s0 = chunks[0].st;
    for (size_t k = 1; k < chunks.size(); ++k) {
        HIP_TRY(hipEventRecord(c->join[k], chunks[k].st));
        HIP_TRY(hipStreamWaitEvent(s0, c->join[k], 0));
    }
    if (int r = fn(s0)) return r;
    HIP_TRY(hipEventRecord(c->fork, s0));
    for (size_t k = 1; k < chunks.size(); ++k) HIP_TRY(hipStreamWaitEvent(chunks[k].st, c->fork, 0));
    return 0;
}

// Work over the first `count` units of the last batch (unit = 1: images, 2: whole stereo pairs).
// Without a caller's stream it follows the batch's chunks, so each chunk's share runs right after
// its extraction on that chunk's stream (unit 2: only if every chunk holds whole pairs) -- or, when
// iso_stage >= 0 is isolated (isolates()), as one launch inside the isolate bracket.  Otherwise:
// join every chunk stream into the caller's (or the main) stream, one launch, rejoin.
// launch(first, n, stream, single) enqueues units [first, first + n) and returns a status;
// single: this call makes no other launch.
template <class F>
int after_batch(orbgpu_ctx* c, void* stream, int count, int unit, int iso_stage, F&& launch) {
    const std::vector<Chunk>& chunks = c->last_chunks;
    bool chunked = !stream && !chunks.empty();
    if (unit == 2)
        for (const Chunk& ch : chunks) chunked &= (ch.img0 % 2) == 0 && (ch.n % 2) == 0;
    if (chunked && iso_stage >= 0 && isolates(c, chunks, iso_stage))
        return isolated(c, chunks, [&](hipStream_t s0) { return launch(0, count, s0, true); });
    if (chunked) {
        for (const Chunk& ch : chunks) {
            const int first = ch.img0 / unit, n = std::min(ch.n / unit, count - first);
            if (n <= 0) continue;
            if (int r = launch(first, n, ch.st, chunks.size() == 1)) return r;
        }
        return 0;
    }
    hipStream_t s = stream ? (hipStream_t)stream : c->stream;
    if (int r = join_all(c, s)) return r;  // the extraction may have run on the chunk streams
    if (int r = launch(0, count, s, true)) return r;
    return rejoin(c, s);
}

}  // namespace orbgpu
