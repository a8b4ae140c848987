// orb_runtime.cpp -- host runtime of liborbgpu.so: contexts, ingest and the batch itself.
//
// Owns one HIP stream and every device buffer of a context (allocated once per geometry,
// never inside a launch sequence), sized and laid out by the pure planner of orb_geometry.h, and
// enqueues the kernels of orb_pyramid.hip, orb_fast.hip, orb_octree.hip and orb_orient.hip.  There
// is no CPU compute path: every result comes from the device.  What runs after a batch (matching, downloads, getters) is in orb_post.cpp; the
// context itself and the helpers both files share are in orb_ctx.h.
#include <link.h>

#include <cstdio>
#include <cstdlib>

#include "orb_ctx.h"

using namespace orbgpu;

namespace {

thread_local std::string g_err;

constexpr size_t kGraphCacheSize = 4;  // captured batch sequences kept per context

// chunk streams a batch of n images is split over (whole stereo pairs per chunk)
inline int kChunksFor(int n) { return n >= 256 ? 2 : 3; }

bool diagnostics_on() {
    const char* g = getenv("ORBGPU_DIAGNOSTICS");
    return g && std::strcmp(g, "1") == 0;
}

// Every diagnostic knob: its variable and how its value lands in DiagKnobs (orb_ctx.h).  The one
// list parse_knobs (once per context, in orbgpu_create) and orbgpu_diagnostic_knobs walk.
struct KnobDef {
    const char* name;
    void (*parse)(DiagKnobs& k, const char* v);
};
const KnobDef kKnobTable[] = {
    {"ORBGPU_OD_ITERS", [](DiagKnobs& k, const char* v) { k.geom.od_iters = std::max(1, atoi(v)); }},
    {"ORBGPU_OCT_SMALL_LDS", [](DiagKnobs& k, const char* v) { k.geom.oct_small_lds = atoi(v); }},
    {"ORBGPU_OCT_SMALL_THREADS",
     [](DiagKnobs& k, const char* v) { k.geom.oct_small_threads = atoi(v) == 128 ? 128 : kOctSmallThreads; }},
    {"ORBGPU_OCT_SPLIT", [](DiagKnobs& k, const char* v) { k.geom.oct_split = std::max(0, atoi(v)); }},
    {"ORBGPU_OCT_GENERIC", [](DiagKnobs& k, const char*) { k.geom.oct_generic = true; }},
    {"ORBGPU_OCT_PYR",
     [](DiagKnobs& k, const char* v) { k.geom.oct_pyr_max = std::max(0, std::min(kOctPyrMaxD, atoi(v))); }},
    {"ORBGPU_OCT_ROUNDS", [](DiagKnobs& k, const char* v) { k.geom.oct_rounds = atoi(v) != 0; }},
    {"ORBGPU_FAST_PITCH", [](DiagKnobs& k, const char* v) {  // force the larger tiles
         const int P = atoi(v);
         k.geom.fast_min_tier = P == kCellMax ? 2 : P == kCellPitchSmall ? 1 : 0;
     }},
    {"ORBGPU_STREAMS", [](DiagKnobs& k, const char* v) { k.streams = atoi(v), k.streams_forced = true; }},
    {"ORBGPU_ISOLATE", [](DiagKnobs& k, const char* v) { k.isolate_mask = (unsigned)strtoul(v, nullptr, 0); }},
    {"ORBGPU_STAGGER", [](DiagKnobs& k, const char* v) { k.stagger = atoi(v) != 0; }},
    {"ORBGPU_OCT_STAMPS", [](DiagKnobs& k, const char*) { k.oct_stamps = true; }},
    {"ORBGPU_GRAPH", [](DiagKnobs& k, const char* v) { k.use_graph = atoi(v) != 0; }},
    {"ORBGPU_KNN_NOSPLIT", [](DiagKnobs& k, const char*) { k.knn_nosplit = true; }},
    {"ORBGPU_NO_TAIL", [](DiagKnobs& k, const char*) { k.geom.no_tail = true; }},
    {"ORBGPU_TAIL_MIN", [](DiagKnobs& k, const char* v) { k.geom.tail_min = std::max(0, atoi(v)); }},
    {"ORBGPU_NO_FUSE_OUT", [](DiagKnobs& k, const char*) { k.no_fuse_out = true; }},
    {"ORBGPU_FAST_SMALL", [](DiagKnobs& k, const char* v) { k.fast_small = atoi(v) != 0 ? 1 : 0; }},
    {"ORBGPU_FAST_OVF_ALL", [](DiagKnobs& k, const char*) { k.fast_ovf_all = true; }},
};

DiagKnobs parse_knobs() {
    DiagKnobs k;
    if (diagnostics_on())
        for (const KnobDef& d : kKnobTable)
            if (const char* v = getenv(d.name)) d.parse(k, v);
    return k;
}

// torch bundles its own libamdhip64 (loaded by path, so a copy of the same soname from /opt/rocm
// that liborbgpu mapped first does not satisfy it): two HIP runtimes in one process then each own
// the device, and torch's sees none.  Entry points that start device work refuse that state with
// ORBGPU_ERR_RUNTIME instead of letting the other runtime fail silently later.  The object list
// is only rescanned when the process has loaded something since the last check (dlpi_adds).
int check_single_hip_runtime() {
    struct Scan { unsigned long long adds; std::vector<std::string> paths; };
    // shared by every context and thread (one per eye in the headset): the cached verdict and
    // its message are read and rescanned under one lock
    static std::mutex mu;
    static unsigned long long checked_adds = ~0ull;
    static int verdict = 0;
    static std::string msg;
    Scan sc{0, {}};
    dl_iterate_phdr([](dl_phdr_info* i, size_t, void* d) -> int {
        static_cast<Scan*>(d)->adds = i->dlpi_adds;
        return 1;  // the counter is the same in every entry: stop at the first
    }, &sc);
    std::lock_guard<std::mutex> lk(mu);
    if (sc.adds != checked_adds) {
        dl_iterate_phdr([](dl_phdr_info* i, size_t, void* d) -> int {
            const char* nm = i->dlpi_name;
            if (!nm || !*nm) return 0;
            const char* base = std::strrchr(nm, '/');
            base = base ? base + 1 : nm;
            if (std::strncmp(base, "libamdhip64.so", 14) == 0) static_cast<Scan*>(d)->paths.push_back(nm);
            return 0;
        }, &sc);
        checked_adds = sc.adds;
        verdict = sc.paths.size() > 1 ? ORBGPU_ERR_RUNTIME : 0;
        std::string paths;
        for (const auto& q : sc.paths) paths += (paths.empty() ? "" : ", ") + q;
        msg = "two HIP runtimes are mapped into this process (" + paths +
              "): import torch before loading liborbgpu.so, so that both bind to one runtime";
    }
    if (verdict) g_err = msg;  // every refusal, cached or fresh, on every thread
    return verdict;
}

}  // namespace

int orbgpu::fail(int code, const std::string& msg) {
    g_err = msg;
    return code;
}

namespace {

int alloc_all(orbgpu_ctx* c, int n_images) {
    const GeomPlan& P = c->plan;
    const size_t ni = (size_t)std::max(n_images, 1);
    int r = 0;
    r |= c->pyr.ensure(ni * P.pyr_img + 256);
    r |= c->blur.ensure(ni * P.blur_img + 256);
    r |= c->rtab.ensure(sizeof(int4) * (P.rtab.size() + 1));
    r |= c->cellkeys.ensure(ni * P.cellkeys_img * 4 + 256);
    r |= c->cellcnt.ensure(ni * P.cellcnt_img * 4 + 256);
    r |= c->octws.ensure(ni * P.octws_img + 256);
    r |= c->lvlkey.ensure(ni * P.lvlkp_img * 4 + 256);
    r |= c->lvlangle.ensure(ni * P.lvlkp_img * 4 + 256);
    r |= c->lvldesc.ensure(ni * P.lvlkp_img * 32 + 256);
    r |= c->lvlcnt.ensure(ni * kMaxLevels * 4);
    r |= c->status.ensure(ni * kMaxLevels * 4);
    r |= c->outkps.ensure(ni * P.out_cap * sizeof(orbgpu_keypoint) + 256);
    r |= c->outdesc.ensure(ni * P.out_cap * 32 + 256);
    r |= c->outn.ensure(ni * 4);
    r |= c->outmono.ensure(ni * 4);
    r |= c->laps.ensure(ni * 8);
    const size_t np = (ni + 1) / 2;
    r |= c->midx1.ensure(np * P.out_cap * 4 + 256);
    r |= c->mdist1.ensure(np * P.out_cap * 4 + 256);
    r |= c->midx2.ensure(np * P.out_cap * 4 + 256);
    r |= c->mdist2.ensure(np * P.out_cap * 4 + 256);
    r |= c->mnq.ensure(np * 4 + 64);
    {  // FAST overflow queue [img][fast_qcap] (image, cell) and two counters per image slot (zeroed
       // once: k_fast_cells_ovf's last workgroup resets its launch's pair)
        void* before = c->fastovf.p;
        const size_t ent = ni * (size_t)std::max(P.A.fast_qcap, 1) * 8;
        r |= c->fastovf.ensure(ent + ni * 8 + 256);
        if (!r && c->fastovf.p != before && hipMemset(c->fastovf.p, 0, c->fastovf.bytes) != hipSuccess) r = -1;
    }
    {  // split kNN2 partials, then the arrival counters of the fused merge (zeroed once: the last
       // workgroup of each query block resets its counter)
        void* before = c->mpart.p;
        const size_t cnt_bytes = knn2_counter_slots(P.out_cap) * 4;
        r |= c->mpart.ensure((size_t)kKnnSplitSlots * P.out_cap * 8 + 256 + cnt_bytes);
        if (!r && c->mpart.p != before && hipMemset(c->mpart.p, 0, c->mpart.bytes) != hipSuccess) r = -1;
    }
    return r ? fail(ORBGPU_ERR_HIP, "hipMalloc failed (device memory)") : 0;
}

// Graph execs are launched on c->stream: the last launch of one may still run when it is
// destroyed, so the stream drains first.
void drop_graph(orbgpu_ctx* c) {
    if (c->graphs.empty()) return;
    hipStreamSynchronize(c->stream);
    for (auto& g : c->graphs) hipGraphExecDestroy(g.exec);
    c->graphs.clear();
}

// Switches the context to w x h images: plans the geometry (orb_geometry.h), sizes the buffers,
// uploads the tables and binds the device pointers into the launch arguments.
int set_geometry(orbgpu_ctx* c, int w, int h) {
    if (c->gw == w && c->gh == h) return 0;
    if (c->gw >= 0)  // the tables and buffers below are still read by the last batch's kernels
        if (int e = ctx_sync(c, true)) return e;
    drop_graph(c);  // its launches carry the old geometry and buffers
    c->gw = c->gh = -1;  // until the new plan is bound
    std::string err;
    if (int e = plan_geometry(c->tab, c->prm, w, h, c->max_images, c->knobs.geom, &c->plan, &err)) return fail(e, err);
    if (int r = alloc_all(c, c->max_images)) return r;
    const GeomPlan& P = c->plan;
    HIP_TRY(hipMemcpyAsync(c->rtab.p, P.rtab.data(), sizeof(int4) * P.rtab.size(), hipMemcpyHostToDevice, c->stream));
    HIP_TRY(hipStreamSynchronize(c->stream));  // pageable source
    c->need_fork = true;
    BatchArgs& A = c->plan.A;
    for (int l = 0; l < A.nlevels; ++l) {
        A.lvl_base[l] = l == 0 ? nullptr : c->pyr.as<uint8_t>() + P.pyr_off[l];
        A.blur_base[l] = c->blur.as<uint8_t>() + P.blur_off[l];
    }
    A.rtab = c->rtab.as<int4>();
    A.cellkeys = c->cellkeys.as<uint32_t>();
    A.cellcnt = c->cellcnt.as<int32_t>();
    A.octws = c->octws.as<uint8_t>();
    A.lvlkey = c->lvlkey.as<uint32_t>();
    A.lvlangle = c->lvlangle.as<float>();
    A.lvldesc = c->lvldesc.as<uint8_t>();
    A.lvlcnt = c->lvlcnt.as<int32_t>();
    A.status = c->status.as<int32_t>();
    A.out_kps = c->outkps.p;
    A.out_desc = c->outdesc.as<uint8_t>();
    A.out_n = c->outn.as<int32_t>();
    A.out_mono = c->outmono.as<int32_t>();
    A.laps = c->laps.as<int32_t>();
    A.fast_ovf = c->fastovf.as<int2>();
    A.fast_ovf_cnt = reinterpret_cast<int*>(c->fastovf.as<uint8_t>() + (size_t)std::max(c->max_images, 1) *
                                                                           std::max(A.fast_qcap, 1) * 8);
    A.fast_small = c->knobs.fast_small;
    A.fast_ovf_all = c->knobs.fast_ovf_all ? 1 : 0;
    c->gw = w;
    c->gh = h;
    return 0;
}

void resolve_pending(orbgpu_ctx* c) {
    for (auto& p : c->pending) {
        float ms = 0;
        if (hipEventSynchronize(p.b) == hipSuccess && hipEventElapsedTime(&ms, p.a, p.b) == hipSuccess) {
            c->stage_ms[p.stage] += ms;
            c->stage_n[p.stage] += 1;
        }
        c->event_pool.push_back(p.a);
        c->event_pool.push_back(p.b);
    }
    c->pending.clear();
}

int ensure_input(orbgpu_ctx* c, int n_images, int w, int h, int slot = -1) {
    if (n_images < 1 || n_images > c->max_images)
        return fail(ORBGPU_ERR_CAPACITY, "n_images exceeds the context's max_images");
    if (w > c->max_w || h > c->max_h) return fail(ORBGPU_ERR_CAPACITY, "image larger than context max");
    if (in_buf(c, slot < 0 ? c->in_slot : slot).ensure((size_t)c->max_images * c->max_w * c->max_h + 256))
        return fail(ORBGPU_ERR_HIP, "hipMalloc failed (input)");
    return 0;
}

// Up to k chunk streams (never more than max_images / 2), each with its join event and, once the
// async upload exists, its slot_free event; created under the allocation / capture lock.  A new
// stream changes the chunk layout, so the batch that asked for it forks from the main stream.
int ensure_sub_streams(orbgpu_ctx* c, int k) {
    k = std::min(k, std::max(1, c->max_images / 2));
    if ((int)c->sub.size() >= k) return 0;
    std::lock_guard<std::recursive_mutex> lk(alloc_capture_mutex());
    HIP_TRY(hipSetDevice(c->device));
    while ((int)c->sub.size() < k) {
        hipStream_t st;
        hipEvent_t jn, fr = nullptr;
        HIP_TRY(hipStreamCreateWithFlags(&st, hipStreamNonBlocking));
        if (hipEventCreateWithFlags(&jn, hipEventDisableTiming) != hipSuccess ||
            (c->copy && hipEventCreateWithFlags(&fr, hipEventDisableTiming) != hipSuccess)) {
            hipStreamDestroy(st);
            return fail(ORBGPU_ERR_HIP, "hipEventCreate failed");
        }
        c->sub.push_back(st);
        c->join.push_back(jn);
        if (fr) c->slot_free.push_back(fr);
    }
    return 0;
}

// A synchronous upload / ingest replaces whatever an async upload staged for the next batch.
int drop_pending_upload(orbgpu_ctx* c) {
    if (c->pending_slot < 0) return 0;
    HIP_TRY(hipStreamSynchronize(c->copy));
    c->pending_slot = -1;
    return 0;
}

}  // namespace

// =============================================================================================
extern "C" {

const char* orbgpu_last_error(void) { return g_err.c_str(); }

int orbgpu_diagnostic_knobs(char* buf, size_t cap) {
    std::string out;
    int n = 0;
    for (const KnobDef& d : kKnobTable)
        if (const char* v = diagnostics_on() ? getenv(d.name) : nullptr) {
            out += (out.empty() ? "" : ";") + std::string(d.name) + "=" + v;
            ++n;
        }
    if (buf && cap) {
        const size_t m = std::min(cap - 1, out.size());
        std::memcpy(buf, out.data(), m);
        buf[m] = 0;
    }
    return n;
}
int orbgpu_abi_version(void) { return ORBGPU_ABI_VERSION; }
int orbgpu_num_stages(void) { return ST_COUNT; }
const char* orbgpu_stage_name(int s) { return (s >= 0 && s < ST_COUNT) ? kStageNames[s] : ""; }

int orbgpu_create(const orbgpu_params* p, int device, int max_width, int max_height,
                  int max_images, orbgpu_ctx** out) {
    if (!p || !out) return fail(ORBGPU_ERR_INVALID, "null argument");
    *out = nullptr;
    if (p->nlevels < 1 || p->nlevels > kMaxLevels || p->nfeatures < 0 || !(p->scale_factor > 1.0f) ||
        max_width <= 0 || max_height <= 0 || max_images <= 0 || max_width >= 4096 + 16 ||
        max_height >= 4096 + 16)
        return fail(ORBGPU_ERR_INVALID, "invalid ORB parameters or sizes");
    if (int e = check_single_hip_runtime()) return e;
    // streams, events and buffers are created under the allocation / capture lock (another
    // thread's context may be capturing a graph)
    std::lock_guard<std::recursive_mutex> create_lk(alloc_capture_mutex());
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0)
        return fail(ORBGPU_ERR_NO_DEVICE, "no HIP device");
    if (device == ORBGPU_DEVICE_CURRENT && hipGetDevice(&device) != hipSuccess)
        return fail(ORBGPU_ERR_NO_DEVICE, "hipGetDevice failed");
    if (device < 0 || device >= ndev) return fail(ORBGPU_ERR_NO_DEVICE, "bad device ordinal");
    hipDeviceProp_t prop;
    HIP_TRY(hipGetDeviceProperties(&prop, device));
    if (std::string(prop.gcnArchName).find("gfx950") == std::string::npos)
        return fail(ORBGPU_ERR_NO_DEVICE, std::string("device is not gfx950: ") + prop.gcnArchName);
    HIP_TRY(hipSetDevice(device));
    orbgpu_ctx* c = new orbgpu_ctx();
    c->prm = *p;
    c->device = device;
    c->max_w = max_width;
    c->max_h = max_height;
    c->max_images = max_images;
    c->tab = build_tables(c->prm);
    c->knobs = parse_knobs();
    if (hipStreamCreateWithFlags(&c->stream, hipStreamNonBlocking) != hipSuccess) {
        delete c;
        return fail(ORBGPU_ERR_HIP, "hipStreamCreate failed");
    }
    c->sub.push_back(c->stream);
    {
        // 2 or 3 chunk streams (with the copy stream of orbgpu_upload_images_async, 3 or 4 of the 4
        // hardware queues a process gets, GPU_MAX_HW_QUEUES = 4; a 5th stream shares a queue and
        // the ingest copy then serialises with the kernels: 3.16 vs 1.75 ms per 128-pair step).
        // Round 4, C2 at 256 pairs: 2 streams 503-508 Mfeatures/s, 3 streams 485-492, 4 streams
        // 467-500, 1 stream 469 (tools/stagger_ab.sh); a token ring that lets one chunk at a time
        // run its pyramid + FAST while the others run octree / orientation / matching: 498 at 2
        // streams, 477-486 at 3 (the stages do not overlap better than side by side)
        // A context that can never hold more than one stereo pair (the single-pair / one-eye
        // extractor) gets one stream: chunks are whole pairs, and every stream takes one of the
        // process's hardware queues, which a second context (the other eye's thread) needs for its
        // own work not to queue behind this one's.
        // the chunk streams the largest batch takes (kChunksFor); run_batch_impl adds the third
        // stream of a smaller batch when one first asks for it (ensure_sub_streams), so a context
        // sized for >= 256 images that never runs a small batch holds 2 streams, not an idle third
        const int want = c->knobs.streams_forced ? c->knobs.streams : kChunksFor(max_images);
        const int ns = std::max(1, std::min({8, want, max_images / 2}));
        for (int k = 1; k < ns; ++k) {
            hipStream_t st;
            if (hipStreamCreateWithFlags(&st, hipStreamNonBlocking) != hipSuccess) break;
            c->sub.push_back(st);
        }
        bool ok = hipEventCreateWithFlags(&c->fork, hipEventDisableTiming) == hipSuccess &&
                  hipEventCreateWithFlags(&c->ext_done, hipEventDisableTiming) == hipSuccess;
        for (size_t k = 0; ok && k < c->sub.size(); ++k) {
            hipEvent_t ev;
            ok = hipEventCreateWithFlags(&ev, hipEventDisableTiming) == hipSuccess;
            if (ok) c->join.push_back(ev);
        }
        if (!ok) {
            orbgpu_destroy(c);
            return fail(ORBGPU_ERR_HIP, "hipEventCreate failed");
        }
    }
    int r = ensure_input(c, 1, max_width, max_height);
    if (!r) r = set_geometry(c, max_width, max_height);
    if (r) {
        orbgpu_destroy(c);
        return r;
    }
    *out = c;
    return ORBGPU_OK;
}

int orbgpu_destroy(orbgpu_ctx* c) {
    if (!c) return ORBGPU_OK;
    hipSetDevice(c->device);
    if (c->stream) hipStreamSynchronize(c->stream);
    resolve_pending(c);
    if (c->copy) hipStreamSynchronize(c->copy);
    std::lock_guard<std::recursive_mutex> destroy_lk(alloc_capture_mutex());  // frees and destroys
    for (auto e : c->event_pool) hipEventDestroy(e);
    for (DevBuf* b : c->bufs) b->release();
    drop_graph(c);
    for (size_t k = 1; k < c->sub.size(); ++k) hipStreamDestroy(c->sub[k]);
    if (c->fork) hipEventDestroy(c->fork);
    if (c->ext_done) hipEventDestroy(c->ext_done);
    if (c->slot_ready) hipEventDestroy(c->slot_ready);
    for (auto e : c->slot_free) hipEventDestroy(e);
    if (c->copy) hipStreamDestroy(c->copy);
    for (hipEvent_t e : c->stagger_ev) hipEventDestroy(e);
    for (auto e : c->join) hipEventDestroy(e);
    if (c->stream) hipStreamDestroy(c->stream);
    delete c;
    return ORBGPU_OK;
}

uint8_t* orbgpu_device_input(orbgpu_ctx* c) { return c ? cur_input(c) : nullptr; }

int orbgpu_upload_images(orbgpu_ctx* c, const uint8_t* images, int n, int w, int h, int stride) {
    if (!c || !images) return fail(ORBGPU_ERR_INVALID, "null argument");
    if (w <= 0 || h <= 0) return fail(ORBGPU_ERR_EMPTY_IMAGE, "empty image");
    if (stride < w) return fail(ORBGPU_ERR_INVALID, "stride < width");
    int r = ensure_input(c, n, w, h);
    if (r) return r;
    HIP_TRY(hipSetDevice(c->device));
    if ((r = drop_pending_upload(c))) return r;
    r = join_all(c, c->stream);  // sub streams may still read the previous images
    if (r) return r;
    HIP_TRY(hipMemcpy2DAsync(cur_input(c), w, images, stride, w, (size_t)h * n, hipMemcpyHostToDevice,
                             c->stream));
    c->need_fork = true;
    return ORBGPU_OK;
}

int orbgpu_upload_images_async(orbgpu_ctx* c, const uint8_t* images, int n, int w, int h, int stride) {
    if (!c || !images) return fail(ORBGPU_ERR_INVALID, "null argument");
    if (w <= 0 || h <= 0) return fail(ORBGPU_ERR_EMPTY_IMAGE, "empty image");
    if (stride < w) return fail(ORBGPU_ERR_INVALID, "stride < width");
    if (c->pending_slot >= 0) return fail(ORBGPU_ERR_INVALID, "an async upload is already staged (run a batch first)");
    const int slot = 1 - c->in_slot;
    int r = ensure_input(c, n, w, h, slot);
    if (r) return r;
    HIP_TRY(hipSetDevice(c->device));
    if (!c->copy) {  // under the allocation / capture lock: another thread may be capturing a graph
        std::lock_guard<std::recursive_mutex> lk(alloc_capture_mutex());
        HIP_TRY(hipStreamCreateWithFlags(&c->copy, hipStreamNonBlocking));
        HIP_TRY(hipEventCreateWithFlags(&c->slot_ready, hipEventDisableTiming));
        while (c->slot_free.size() < c->sub.size()) {
            hipEvent_t e;
            HIP_TRY(hipEventCreateWithFlags(&e, hipEventDisableTiming));
            c->slot_free.push_back(e);
        }
    }
    // the slot was last read by work enqueued before the current batch began (slot_free)
    for (size_t k = 0; k < c->slot_free.size(); ++k) HIP_TRY(hipStreamWaitEvent(c->copy, c->slot_free[k], 0));
    HIP_TRY(hipMemcpy2DAsync(in_buf(c, slot).p, w, images, stride, w, (size_t)h * n, hipMemcpyHostToDevice,
                             c->copy));
    HIP_TRY(hipEventRecord(c->slot_ready, c->copy));
    c->pending_slot = slot;
    return ORBGPU_OK;
}

int orbgpu_host_alloc(size_t bytes, void** ptr) {
    if (!ptr) return fail(ORBGPU_ERR_INVALID, "null argument");
    *ptr = nullptr;
    std::lock_guard<std::recursive_mutex> lk(alloc_capture_mutex());
    HIP_TRY(hipHostMalloc(ptr, bytes ? bytes : 1, hipHostMallocDefault));
    return ORBGPU_OK;
}

int orbgpu_host_free(void* ptr) {
    std::lock_guard<std::recursive_mutex> lk(alloc_capture_mutex());
    if (ptr) HIP_TRY(hipHostFree(ptr));
    return ORBGPU_OK;
}

// The batch's kernels; match_pairs > 0 appends the stereo kNN2 of pairs [0, match_pairs) when the
// batch runs as one captured graph (*matched = true: one submission for extraction and match).
static int run_batch_impl(orbgpu_ctx* c, int n, int w, int h, const int32_t* laps, void* stream,
                          int match_pairs, int stereo_only, bool* matched) {
    if (matched) *matched = false;
    if (!c) return fail(ORBGPU_ERR_INVALID, "null ctx");
    if (int e = check_single_hip_runtime()) return e;
    if (w <= 0 || h <= 0) return fail(ORBGPU_ERR_EMPTY_IMAGE, "empty image");
    int r = ensure_input(c, n, w, h);
    if (r) return r;
    HIP_TRY(hipSetDevice(c->device));
    r = set_geometry(c, w, h);
    if (r) return r;
    hipStream_t s = stream ? (hipStream_t)stream : c->stream;
    // the lapping areas change rarely (per camera): upload them only when they differ from the
    // copy already on the device, after every stream has finished reading the old one
    {
        std::vector<int32_t> want((size_t)n * 2, 0);
        if (laps) std::memcpy(want.data(), laps, (size_t)n * 8);
        if (want != c->laps_host) {
            r = join_all(c, s);
            if (r) return r;
            HIP_TRY(hipMemcpyAsync(c->laps.p, want.data(), (size_t)n * 8, hipMemcpyHostToDevice, s));
            HIP_TRY(hipStreamSynchronize(s));  // `want` is pageable host memory
            c->laps_host.swap(want);
            c->need_fork = true;
        }
    }
    BatchArgs A = c->plan.A;
    A.nimages = n;
    A.img0 = 0;
    A.octdbg = nullptr;
    // no image with a lapping area a keypoint can fall in (every x is >= minBorderX = 16): every
    // keypoint is mono and k_orient_desc writes the assembled outputs itself (no k_finalize)
    A.fuse_out = 1;
    for (int i = 0; i < n; ++i) {
        const int l0 = c->laps_host[2 * i], l1 = c->laps_host[2 * i + 1];
        if (l1 >= kMinBorder && l0 <= l1) A.fuse_out = 0;
    }
    if (c->knobs.no_fuse_out) A.fuse_out = 0;
    c->last_fused = A.fuse_out != 0;  // orbgpu_get_level_keypoints reads the outputs then
    if (c->knobs.oct_stamps) {  // diagnostic build of the octree phase clocks
        const size_t bytes = (size_t)n * kMaxLevels * 8 * 8;
        if (!c->octdbg.ensure(bytes)) {
            hipMemsetAsync(c->octdbg.p, 0, bytes, s);
            A.octdbg = c->octdbg.as<unsigned long long>();
        }
    }
    // an async upload staged the next batch in the other input slot: read it once the copy lands
    // (each chunk stream waits on the copy alone, so the chunks keep their steady-state offsets);
    // first note what every stream has enqueued so far -- the readers of the slot we leave
    bool slot_switch = false;
    if (c->pending_slot >= 0) {
        c->in_slot = c->pending_slot;
        c->pending_slot = -1;
        slot_switch = true;
    }
    for (size_t k = 0; k < c->sub.size() && k < c->slot_free.size(); ++k)
        HIP_TRY(hipEventRecord(c->slot_free[k], c->sub[k]));
    A.lvl_base[0] = cur_input(c);
    A.lv[0].img_stride = (long long)w * h;
    // Sub-batches (whole stereo pairs) on parallel streams: the stages have complementary
    // bottlenecks (octree latency, FAST VALU, blur/resize HBM), so their phases overlap.
    std::vector<Chunk> chunks;
    // chunks per batch: batches of >= 128 pairs take 2 (each chunk fills the GPU); smaller ones
    // 3 (C5's 16 1080p pairs: 161 vs 154 Mfeatures/s); ORBGPU_STREAMS forces the stream count
    const int kmax = c->knobs.streams_forced ? (int)c->sub.size() : kChunksFor(n);
    if (!stream && (n % 2) == 0 && !c->knobs.streams_forced)
        if (int e_ = ensure_sub_streams(c, std::min(kmax, n / 2))) return e_;
    const int K = (!stream && (n % 2) == 0) ? std::min({(int)c->sub.size(), kmax, n / 2}) : 1;
    // a different sub-batch layout than last time may put an image on another stream: drain first
    if (!c->last_chunks.empty() && ((int)c->last_chunks.size() != K || c->last_images != n))
        if (int e_ = ctx_sync(c)) return e_;
    const bool relayout = c->last_chunks.empty() || (int)c->last_chunks.size() != K || c->last_images != n;
    if (K > 1) {
        // sub stream k > 0 waits for the main stream only when the main stream holds work it
        // depends on (a new layout, uploaded images, new lapping areas): in the steady state
        // every chunk's chain of steps stays on its own stream, so the streams keep the offset
        // they were given at the first step (stagger below) instead of restarting in lockstep
        const bool fork = relayout || c->need_fork;
        if (fork) HIP_TRY(hipEventRecord(c->fork, s));
        for (int k = 0; k < K; ++k) {
            const int p0 = (int)((long long)k * (n / 2) / K), p1 = (int)((long long)(k + 1) * (n / 2) / K);
            if (p1 > p0) {
                if (k > 0 && fork) HIP_TRY(hipStreamWaitEvent(c->sub[k], c->fork, 0));
                chunks.push_back({2 * p0, 2 * (p1 - p0), c->sub[k]});
            }
        }
        c->need_fork = false;
    } else {
        chunks.push_back({0, n, s});
    }
    if (slot_switch)
        for (const Chunk& ch : chunks) HIP_TRY(hipStreamWaitEvent(ch.st, c->slot_ready, 0));
    // first step of a layout: chunk k starts after chunk k-1 finished its pyramid + blur, so the
    // chunks run different stages (memory-, VALU- and latency-bound ones) at the same time
    // (also after serialized profiling runs, which leave every chunk stream joined: without a new
    // stagger the chunks would run each stage side by side from then on)
    const bool stagger = (relayout || c->restagger) && c->knobs.stagger && chunks.size() > 1 && !c->serialize;
    if (stagger) c->restagger = false;
    while (stagger && c->stagger_ev.size() < chunks.size()) {
        hipEvent_t ev;
        HIP_TRY(hipEventCreateWithFlags(&ev, hipEventDisableTiming));
        c->stagger_ev.push_back(ev);
    }
    auto chunk_args = [&](const Chunk& ch) {
        BatchArgs B = A;
        B.img0 = ch.img0;
        B.nimages = ch.n;
        return B;
    };
    // one stage over the batch: each chunk's share on its stream, or (isolated) the whole batch once
    auto each = [&](int stage, auto launch) -> int {
        if (isolates(c, chunks, stage))
            return isolated(c, chunks, [&](hipStream_t s0) {
                return timed(c, stage, s0, [&] { return launch(A, s0); });
            });
        for (const Chunk& ch : chunks) {
            const BatchArgs B = chunk_args(ch);
            if (int rr = timed(c, stage, ch.st, [&] { return launch(B, ch.st); })) return rr;
        }
        return 0;
    };
    // the kernel sequence of this batch (every launch goes to the chunk streams)
    auto launch_all = [&]() -> int {
        int r = 0;
        // k_blur_resize makes levels 1 .. last_br - 1; k_pyr_tail the rest (or k_blur the last blur)
        int chunk_images = 0;
        for (const Chunk& ch : chunks) chunk_images = std::max(chunk_images, ch.n);
        if (c->serialize || chunks.size() == 1) chunk_images = n;
        const bool tail = A.tail0 <= A.nlevels && chunk_images >= A.tail_min;
        const int last_br = tail ? A.tail0 : A.nlevels;
        // the pyramid of one (args, stream), handed stage by stage to run(stage, launch): level
        // l - 1's blur and level l in one pass over level l - 1, then the tail or the last level's blur
        auto pyramid = [&](auto&& run) -> int {
            for (int l = 1; l < last_br; ++l)
                if (int rr = run(ST_RESIZE, [&](const BatchArgs& B, hipStream_t st) { return launch_blur_resize(B, l, st); }))
                    return rr;
            if (tail) return run(ST_TAIL, [](const BatchArgs& B, hipStream_t st) { return launch_pyr_tail(B, st); });
            const int lt = A.nlevels - 1;
            return run(ST_BLUR, [&](const BatchArgs& B, hipStream_t st) { return launch_blur_level(B, lt, st); });
        };
        if (c->plan.generic_pyr) {  // scale steps above 2: every level from HBM, then every blur
            for (int l = 1; l < A.nlevels; ++l) {
                r = each(ST_RESIZE, [&](const BatchArgs& B, hipStream_t st) { return launch_level_linear(B, l, st); });
                if (r) return r;
            }
            for (int l = 0; l < A.nlevels; ++l) {
                r = each(ST_BLUR, [&](const BatchArgs& B, hipStream_t st) { return launch_blur_level(B, l, st); });
                if (r) return r;
            }
        } else if (stagger) {
            // chunk-major: chunk k's first kernel waits for chunk k-1's pyramid + blur
            for (size_t k = 0; k < chunks.size(); ++k) {
                const Chunk& ch = chunks[k];
                const BatchArgs B = chunk_args(ch);
                if (k > 0) HIP_TRY(hipStreamWaitEvent(ch.st, c->stagger_ev[k - 1], 0));
                r = pyramid([&](int stage, auto launch) {
                    return timed(c, stage, ch.st, [&] { return launch(B, ch.st); });
                });
                if (r) return r;
                HIP_TRY(hipEventRecord(c->stagger_ev[k], ch.st));
            }
        } else if ((r = pyramid(each))) {  // stage-major over the chunks
            return r;
        }
        {   // the FAST tiles as one group: one join / fork around all of them when isolated
            const int tiles[3] = {kCellPitchTiny, kCellPitchSmall, kCellMax};
            const int stages[3] = {ST_FAST48, ST_FAST, ST_FAST_TOP};
            bool any[3], iso = false;
            for (int t = 0; t < 3; ++t) {
                int c0, c1;
                fast_cell_range(A, tiles[t], &c0, &c1);
                any[t] = c1 > c0;
                iso = iso || (any[t] && isolates(c, chunks, stages[t]));
            }
            auto fast = [&](bool whole) -> int {  // whole: the whole batch on chunk 0's stream
                for (int t = 0; t < 3; ++t) {
                    if (!any[t]) continue;
                    for (const Chunk& ch : chunks) {
                        const BatchArgs B = whole ? A : chunk_args(ch);
                        const hipStream_t st = ch.st;
                        const int tile = tiles[t];
                        if (int rr = timed(c, stages[t], st, [&] { return launch_fast_cells(B, tile, st); })) return rr;
                        if (whole) break;
                    }
                }
                return 0;
            };
            r = iso ? isolated(c, chunks, [&](hipStream_t) { return fast(true); }) : fast(false);
            if (r) return r;
        }
        if ((r = each(ST_OCTREE, [](const BatchArgs& B, hipStream_t st) { return launch_octree(B, st); }))) return r;
        if ((r = each(ST_ORIENT, [](const BatchArgs& B, hipStream_t st) { return launch_orient_desc(B, st); }))) return r;
        if (!A.fuse_out)
            if ((r = each(ST_FINAL, [](const BatchArgs& B, hipStream_t st) { return launch_finalize(B, st); }))) return r;
        return 0;
    };
    // One stream, no caller stream, no instrumentation (the single-pair / latency shape, e.g.
    // orbgpu_extract_stereo): the ~15 launches are captured once into a hipGraph and replayed
    // while the batch shape and input slot stay the same -- one submission instead of ~15.
    const bool graphable = chunks.size() == 1 && !stream && c->prof_mask == 0 && c->knobs.use_graph &&
                           !c->knobs.oct_stamps;
    const bool with_match = graphable && match_pairs > 0 && 2 * match_pairs <= n && c->plan.out_cap <= 65535;
    auto launch_match = [&]() -> int {
        MatchArgs m = stereo_match_args(c, stereo_only);
        m.part = match_pairs * 2 <= kKnnSplitSlots && !c->knobs.knn_nosplit ? c->mpart.as<uint2>() : nullptr;
        HIP_TRY(launch_knn2_pairs(m, match_pairs, s));
        return 0;
    };
    if (graphable) {
        const int key[7] = {n, w, h, c->in_slot, with_match ? match_pairs : 0, with_match ? stereo_only : 0, A.fuse_out};
        orbgpu_ctx::GraphRec* rec = nullptr;
        for (auto& g : c->graphs)
            if (std::memcmp(key, g.key, sizeof key) == 0) rec = &g;
        if (!rec) {
            if (c->graphs.size() >= kGraphCacheSize) {  // evict the least recently launched exec
                size_t lru = 0;
                for (size_t k = 1; k < c->graphs.size(); ++k)
                    if (c->graphs[k].used < c->graphs[lru].used) lru = k;
                HIP_TRY(hipStreamSynchronize(c->stream));  // its last launch may still run
                hipGraphExecDestroy(c->graphs[lru].exec);
                c->graphs.erase(c->graphs.begin() + lru);
            }
            hipGraphExec_t ex = nullptr;
            hipError_t ei = hipSuccess;
            {
                std::lock_guard<std::recursive_mutex> lk(alloc_capture_mutex());  // no allocation mid-capture
                HIP_TRY(hipStreamBeginCapture(s, hipStreamCaptureModeThreadLocal));
                int rr = launch_all();
                if (!rr && with_match) rr = launch_match();
                hipGraph_t g = nullptr;
                const hipError_t ec = hipStreamEndCapture(s, &g);
                if (rr || ec != hipSuccess) {
                    if (g) hipGraphDestroy(g);
                    return rr ? rr : fail(ORBGPU_ERR_HIP, std::string("hipStreamEndCapture: ") + hipGetErrorString(ec));
                }
                ei = hipGraphInstantiate(&ex, g, nullptr, nullptr, 0);
                hipGraphDestroy(g);
            }
            if (ei != hipSuccess)
                return fail(ORBGPU_ERR_HIP, std::string("hipGraphInstantiate: ") + hipGetErrorString(ei));
            orbgpu_ctx::GraphRec nr{};
            std::memcpy(nr.key, key, sizeof key);
            nr.exec = ex;
            c->graphs.push_back(nr);
            rec = &c->graphs.back();
        }
        rec->used = ++c->graph_tick;
        HIP_TRY(hipGraphLaunch(rec->exec, s));
    } else if ((r = launch_all())) {
        return r;
    }
    c->last_chunks = chunks;
    c->last_images = n;
    c->last_w = w;
    c->last_h = h;
    if (with_match) {
        c->last_pairs = match_pairs;
        if (matched) *matched = true;
    }
    // a caller's stream: the context's streams wait for it before they touch this batch's
    // buffers again (the next async upload overwrites the input slot this batch read)
    if (stream && (r = rejoin(c, s))) return r;
    return ORBGPU_OK;
}

int orbgpu_run_batch(orbgpu_ctx* c, int n, int w, int h, const int32_t* laps, void* stream) {
    return run_batch_impl(c, n, w, h, laps, stream, 0, 0, nullptr);
}

int orbgpu_run_batch_match(orbgpu_ctx* c, int n, int w, int h, const int32_t* laps, int stereo_rows_only,
                           void* stream) {
    if (!c) return fail(ORBGPU_ERR_INVALID, "null ctx");
    if (n < 2 || (n % 2) != 0) return fail(ORBGPU_ERR_INVALID, "run_batch_match needs whole stereo pairs");
    bool matched = false;
    int r = run_batch_impl(c, n, w, h, laps, stream, n / 2, stereo_rows_only ? 1 : 0, &matched);
    if (r || matched) return r;
    return orbgpu_match_stereo_batch(c, n / 2, stereo_rows_only, stream);
}

int orbgpu_synchronize(orbgpu_ctx* c) {
    if (!c) return fail(ORBGPU_ERR_INVALID, "null ctx");
    if (int e_ = ctx_sync(c, true)) return e_;
    resolve_pending(c);
    if (c->knobs.oct_stamps && c->octdbg.p && c->last_images > 0) {
        const int n = c->last_images, L = c->prm.nlevels;
        std::vector<unsigned long long> d((size_t)n * kMaxLevels * 8);
        D2H(d.data(), c->octdbg.p, d.size() * 8);
        for (int l = 0; l < L; ++l) {
            double acc[8] = {}, phase1 = 0;
            for (int i = 0; i < n; ++i) {
                const unsigned long long* s = &d[((size_t)i * kMaxLevels + l) * 8];
                for (int k = 0; k < 7; ++k) acc[k] += (double)s[k];
                acc[7] += (double)(s[7] & 0xFFFFFFFFull);  // slot 7: rounds, the phase-1 ones in the upper half
                phase1 += (double)(s[7] >> 32);
            }
            fprintf(stderr, "octree L%d us: init %.1f choose %.1f barrier %.1f sort %.1f rebuild(direct phase 1: list build) %.1f relabel(pyramid: gather+histogram) %.1f best(pyramid: sums) %.1f rounds %.1f phase-1 rounds %.1f\n",
                    l, acc[0] / n / 100, acc[1] / n / 100, acc[2] / n / 100, acc[3] / n / 100,
                    acc[4] / n / 100, acc[5] / n / 100, acc[6] / n / 100, acc[7] / n, phase1 / n);
        }
    }
    return ORBGPU_OK;
}

int orbgpu_extract(orbgpu_ctx* c, const uint8_t* image, int w, int h, int stride, int lap0,
                   int lap1, orbgpu_keypoint* kps, uint8_t* desc, int cap, int* n, int* n_mono) {
    if (!c) return fail(ORBGPU_ERR_INVALID, "null ctx");
    if (!image || w <= 0 || h <= 0) return fail(ORBGPU_ERR_EMPTY_IMAGE, "empty image");  // :1092
    int r = orbgpu_upload_images(c, image, 1, w, h, stride);
    if (r) return r;
    int32_t laps[2] = {lap0, lap1};
    r = orbgpu_run_batch(c, 1, w, h, laps, nullptr);
    if (r) return r;
    return orbgpu_download_result(c, 0, kps, desc, cap, n, n_mono);
}

int orbgpu_extract_stereo(orbgpu_ctx* c, const uint8_t* left, const uint8_t* right, int w, int h,
                          int stride, const int lap_left[2], const int lap_right[2],
                          orbgpu_keypoint* kl, uint8_t* dl, int* nl, int* ml, orbgpu_keypoint* kr,
                          uint8_t* dr, int* nr, int* mr, int cap) {
    if (!c) return fail(ORBGPU_ERR_INVALID, "null ctx");
    if (!left || !right || w <= 0 || h <= 0) return fail(ORBGPU_ERR_EMPTY_IMAGE, "empty image");
    int r = ensure_input(c, 2, w, h);
    if (r) return r;
    if (stride < w) return fail(ORBGPU_ERR_INVALID, "stride < width");
    HIP_TRY(hipSetDevice(c->device));
    if ((r = drop_pending_upload(c))) return r;
    r = join_all(c, c->stream);  // sub streams of an earlier batch may still read the input
    if (r) return r;
    c->need_fork = true;
    HIP_TRY(hipMemcpy2DAsync(cur_input(c), w, left, stride, w, h, hipMemcpyHostToDevice, c->stream));
    HIP_TRY(hipMemcpy2DAsync(cur_input(c) + (size_t)w * h, w, right, stride, w, h,
                             hipMemcpyHostToDevice, c->stream));
    int32_t laps[4] = {lap_left ? lap_left[0] : 0, lap_left ? lap_left[1] : 0,
                       lap_right ? lap_right[0] : 0, lap_right ? lap_right[1] : 0};
    r = orbgpu_run_batch(c, 2, w, h, laps, nullptr);
    if (r) return r;
    r = orbgpu_download_result(c, 0, kl, dl, cap, nl, ml);
    if (r) return r;
    return orbgpu_download_result(c, 1, kr, dr, cap, nr, mr);
}

int orbgpu_ingest_images(orbgpu_ctx* c, const uint8_t* device_images, int n, int w, int h, int stride,
                         void* stream) {
    if (!c || !device_images) return fail(ORBGPU_ERR_INVALID, "null argument");
    if (w <= 0 || h <= 0) return fail(ORBGPU_ERR_EMPTY_IMAGE, "empty image");
    if (stride < w) return fail(ORBGPU_ERR_INVALID, "stride < width");
    int r = ensure_input(c, n, w, h);
    if (r) return r;
    HIP_TRY(hipSetDevice(c->device));
    if (!device_ptr(device_images)) return fail(ORBGPU_ERR_INVALID, "device_images is not device memory");
    if ((r = drop_pending_upload(c))) return r;
    hipStream_t s = stream ? (hipStream_t)stream : c->stream;
    if ((r = join_all(c, s))) return r;  // the chunk streams may still read the previous images
    HIP_TRY(hipMemcpy2DAsync(cur_input(c), w, device_images, stride, w, (size_t)h * n, hipMemcpyDeviceToDevice, s));
    c->need_fork = true;
    return rejoin(c, s);
}

// ---- wire formats (orb_io.hip) ---------------------------------------------------------------
uint8_t* orbgpu_device_sbs_input(orbgpu_ctx* c) {
    if (!c) return nullptr;
    if (hipSetDevice(c->device) != hipSuccess) return nullptr;
    const size_t frames = (size_t)(c->max_images / 2 > 0 ? c->max_images / 2 : 1);
    if (c->sbs.ensure(frames * c->max_h * 2 * (size_t)c->max_w + 256)) {
        fail(ORBGPU_ERR_HIP, "hipMalloc failed (sbs staging)");
        return nullptr;
    }
    return c->sbs.as<uint8_t>();
}

static int check_sbs(orbgpu_ctx* c, int n, int w, int h, int stride) {
    if (w <= 0 || h <= 0) return fail(ORBGPU_ERR_EMPTY_IMAGE, "empty image");
    if (stride < 2 * w) return fail(ORBGPU_ERR_INVALID, "stride < 2 * width (side-by-side frame)");
    if (n < 1) return fail(ORBGPU_ERR_INVALID, "bad frame count");
    return ensure_input(c, 2 * n, w, h);
}

int orbgpu_ingest_sbs(orbgpu_ctx* c, const uint8_t* frames, int n, int w, int h, int stride, void* stream) {
    if (!c || !frames) return fail(ORBGPU_ERR_INVALID, "null argument");
    int r = check_sbs(c, n, w, h, stride);
    if (r) return r;
    HIP_TRY(hipSetDevice(c->device));
    hipStream_t s = stream ? (hipStream_t)stream : c->stream;
    if ((r = drop_pending_upload(c))) return r;
    r = join_all(c, s);  // sub streams may still read the previous images
    if (r) return r;
    SbsArgs a{frames, (long long)h * stride, stride, w, h, n, cur_input(c)};
    r = timed(c, ST_SBS, s, [&] { return launch_sbs_split(a, s); });
    if (r) return r;
    c->need_fork = true;
    // a caller's stream: the next batch (forked from the context's stream) waits for the split
    return rejoin(c, s);
}

int orbgpu_upload_sbs(orbgpu_ctx* c, const uint8_t* frames, int n, int w, int h, int stride) {
    if (!c || !frames) return fail(ORBGPU_ERR_INVALID, "null argument");
    int r = check_sbs(c, n, w, h, stride);
    if (r) return r;
    HIP_TRY(hipSetDevice(c->device));
    const size_t bytes = (size_t)n * h * stride;
    if (c->sbs.ensure(bytes + 256)) return fail(ORBGPU_ERR_HIP, "hipMalloc failed (sbs staging)");
    r = join_all(c, c->stream);
    if (r) return r;
    // 2W bytes of each of the n*h rows: never reads the padding after the last row's pixels
    HIP_TRY(hipMemcpy2DAsync(c->sbs.p, stride, frames, stride, 2 * (size_t)w, (size_t)n * h,
                             hipMemcpyHostToDevice, c->stream));
    return orbgpu_ingest_sbs(c, c->sbs.as<uint8_t>(), n, w, h, stride, nullptr);
}

int orbgpu_extract_features(orbgpu_ctx* c, const uint8_t* image, int image_len, int width, int height,
                            int stride, int threshold, int lap_l0, int lap_l1, int lap_r0, int lap_r1,
                            int* count_l, int32_t* x_l, int32_t* y_l, int32_t* angle_l, int32_t* level_l,
                            uint8_t* orb_l, int* count_r, int32_t* x_r, int32_t* y_r, int32_t* angle_r,
                            int32_t* level_r, uint8_t* orb_r, int kp_cap, int* mono_l, int* mono_r,
                            int16_t* indices, int16_t* dist1, int16_t* dist2, int match_cap) {
    (void)threshold;  // the DSP ignores it too (orbslam_dsp.cpp:1003-1087): the ctx's FAST thresholds apply
    if (!c || !image) return fail(ORBGPU_ERR_INVALID, "null argument");
    if ((long long)image_len < (long long)stride * (height - 1) + 2LL * width)
        return fail(ORBGPU_ERR_INVALID, "image_len smaller than the side-by-side frame");
    int r = orbgpu_upload_sbs(c, image, 1, width, height, stride);
    if (r) return r;
    const int32_t laps[4] = {lap_l0, lap_l1, lap_r0, lap_r1};
    r = orbgpu_run_batch(c, 2, width, height, laps, nullptr);
    if (!r) r = orbgpu_match_stereo_batch(c, 1, 1, nullptr);
    if (!r) r = orbgpu_pack_soa(c, 2, 1, nullptr);
    if (!r) r = orbgpu_download_soa(c, 0, x_l, y_l, angle_l, level_l, orb_l, kp_cap, count_l, mono_l);
    if (!r) r = orbgpu_download_soa(c, 1, x_r, y_r, angle_r, level_r, orb_r, kp_cap, count_r, mono_r);
    int nq = 0;
    if (!r) r = orbgpu_download_matches16(c, 0, indices, dist1, dist2, match_cap, &nq);
    return r;
}

int orbgpu_set_profiling(orbgpu_ctx* c, int enable) {
    if (!c) return fail(ORBGPU_ERR_INVALID, "null ctx");
    // enable: 0 = off, 1 = every stage, otherwise (1u << 31) | [1u << 30] | stage mask: the
    // selected stages; bit 30 also runs every stage as one whole-batch launch (serial timing)
    const unsigned e = (unsigned)enable;
    c->prof_mask = e == 0 ? 0u : e == 1 ? 0xFFFFFFFFu : (e & 0x3FFFFFFFu);
    const bool was_serial = c->serialize;
    c->serialize = e != 0 && e != 1 && (e & (1u << 30));
    if (was_serial && !c->serialize) c->restagger = true;
    return ORBGPU_OK;
}

int orbgpu_stage_times(orbgpu_ctx* c, double* ms, int64_t* launches, int max_stages) {
    if (!c) return fail(ORBGPU_ERR_INVALID, "null ctx");
    resolve_pending(c);
    for (int s = 0; s < ST_COUNT && s < max_stages; ++s) {
        if (ms) ms[s] = c->stage_ms[s];
        if (launches) launches[s] = c->stage_n[s];
    }
    return ST_COUNT;
}

int orbgpu_reset_stage_times(orbgpu_ctx* c) {
    if (!c) return fail(ORBGPU_ERR_INVALID, "null ctx");
    resolve_pending(c);
    for (int s = 0; s < ST_COUNT; ++s) c->stage_ms[s] = 0, c->stage_n[s] = 0;
    return ORBGPU_OK;
}

}  // extern "C"
