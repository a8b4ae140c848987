// orb_matchers.cpp -- the part of the C ABI (include/orbgpu.h) that runs the ORBmatcher searches over
// the device-resident results of a batch: the local-map search (orb_sbp.hip), the motion-model search
// (orb_track.hip), the initialisation search (orb_init.hip), the bag-of-words search (orb_bow.hip), the
// triangulation search (orb_tri.hip), the relocalisation search (orb_reloc.hip), the map-point fusion
// (orb_fuse.hip), the loop closer's Sim3 projection searches (orb_sim3.hip) and its keyframe-to-keyframe
// bag-of-words search (orb_bowkf.hip).  Every entry point validates its own arguments, in its own order.
// What dies with a call (uploaded inputs, the kernels' scratch) it lays out in the context's one workspace,
// what its download reads in its own result buffer, each region named once (orb_layout.h); the download
// reads the slots the call recorded.  What the searches share -- the offsets check, the padded row uploads,
// the common argument fields, the node searches' grouping regions, the launch path and the download -- is
// written once, below.
#include <cmath>
#include <type_traits>

#include "orb_ctx.h"

using namespace orbgpu;

namespace {

// offsets[0 .. n]: must ascend.  rebase == false: offsets[0] must be 0; rebase == true: offsets[0] >= 0
// and the caller passes the points from offsets[0] on.  Each entry is checked before the next one is
// read.  *max_span = the largest offsets[k + 1] - offsets[k], *total = offsets[n] - offsets[0].
int check_offsets(const int32_t* offsets, int n, bool rebase, const char* name, int* max_span, int* total) {
    *max_span = *total = 0;
    if (n < 1) return 0;
    if (rebase ? offsets[0] < 0 : offsets[0] != 0)
        return fail(ORBGPU_ERR_INVALID, rebase ? "negative keyframe offset" : name);
    for (int k = 0; k < n; ++k) {
        if (offsets[k + 1] < offsets[k])
            return fail(ORBGPU_ERR_INVALID, rebase ? std::string(name) + " must ascend" : std::string(name));
        *max_span = std::max(*max_span, offsets[k + 1] - offsets[k]);
    }
    *total = offsets[n] - offsets[0];
    return 0;
}

// A caller's padded array holds one row of `stride` entries per result row: each row must cover the
// keypoints of its image, image[r * image_stride] among the first n_images of the batch.
int rows_cover_counts(orbgpu_ctx* c, int n_images, const int32_t* image, int image_stride, int rows, int stride,
                      const char* msg) {
    if (int e_ = ctx_sync(c)) return e_;  // (sets the device)
    std::vector<int32_t> counts((size_t)n_images);
    D2H(counts.data(), c->outn.p, counts.size() * 4);
    for (int r = 0; r < rows; ++r)
        if (stride < std::min(counts[image[(size_t)r * image_stride]], (int32_t)c->plan.out_cap))
            return fail(ORBGPU_ERR_INVALID, msg);
    return 0;
}

// `rows` host rows of src_pitch bytes into device rows of dst_pitch bytes, `width` bytes of each;
// fill_byte >= 0 fills the device rows first (what the copy leaves of a row reads as that byte).
// src == nullptr: an optional input the caller did not pass, nothing to do.
int upload_rows(const void* dst_, size_t dst_pitch, const void* src, size_t src_pitch, size_t width, size_t rows,
                int fill_byte, hipStream_t s) {
    if (!src) return 0;
    void* const dst = const_cast<void*>(dst_);  // an input region: the argument structs name those const
    if (fill_byte >= 0) HIP_TRY(hipMemsetAsync(dst, fill_byte, dst_pitch * rows, s));
    if (width) HIP_TRY(hipMemcpy2DAsync(dst, dst_pitch, src, src_pitch, width, rows, hipMemcpyHostToDevice, s));
    return 0;
}

// {frames [np], offsets [np + 1] rebased to 0}: pair p's points from 0 on the device
std::vector<int32_t> frames_and_offsets(const int32_t* frames, const int32_t* offsets, size_t np) {
    std::vector<int32_t> head(2 * np + 1);
    std::copy(frames, frames + np, head.begin());
    for (size_t p = 0; p <= np; ++p) head[np + p] = offsets[p] - offsets[0];
    return head;
}

// The fields every search's argument struct shares, filled by name (the structs share no base: their
// layouts are the kernels' argument layouts).
template <class Args>
void bind_frame(Args& a, const orbgpu_ctx* c) {
    a.kps = c->outkps.p;
    a.out_n = c->outn.as<int32_t>();
    a.out_cap = c->plan.out_cap;
    a.desc = c->outdesc.as<uint8_t>();
}

template <class Args>
void bind_grid(Args& a, const orbgpu_ctx* c) {  // of the last orbgpu_undistort_grid_batch
    a.xy_un = c->gxy.as<float>();
    a.cell_start = c->gstart.as<int32_t>();
    a.cell_idx = c->gidx.as<int32_t>();
    std::memcpy(a.bounds, c->grid_bounds, sizeof a.bounds);
    std::memcpy(a.grid_inv, c->grid_inv, sizeof a.grid_inv);
}

template <class Args>
void bind_scale(Args& a, const orbgpu_ctx* c) {
    for (int l = 0; l < kMaxLevels; ++l) a.scale[l] = l < c->prm.nlevels ? c->tab.scale[l] : 1.0f;
    a.nlevels = c->prm.nlevels;
}

// Row r of a search's results = batch image images[r * step], or image r * step where there is no list.
MatchCover cover_of(size_t rows, const int32_t* images, int step, bool two_cam) {
    MatchCover cover;
    cover.image.resize(rows);
    for (size_t r = 0; r < rows; ++r) cover.image[r] = images ? images[r * step] : (int32_t)r * step;
    cover.two_cam = two_cam;
    return cover;
}

// A call over no pairs: the search has no row left.
int no_results(SearchResult& res) {
    res.cover.image.clear();
    res.point_off.clear();
    return ORBGPU_OK;
}

// The result slots every search has: its match rows, its counts and, where it has them (hist != nullptr),
// hist_words words per row: the rotation histogram, or sim3's replay stats.
ResultSlots add_match_rows(Layout& out, size_t rows, size_t row_cap, int32_t*& match, int32_t*& nmatches, int32_t** hist,
                           size_t hist_words) {
    ResultSlots rs;
    rs.row_cap = row_cap;
    rs.match = match = out.add<int32_t>(rows * row_cap);
    rs.nmatches = nmatches = out.add<int32_t>(rows);
    if (hist) rs.hist = *hist = out.add<int32_t>(rows * hist_words);
    return rs;
}

// Host to device into an input region: the argument structs name those const (the kernels only read them).
int h2d(const void* dst, const void* src, size_t bytes, hipStream_t s) {
    if (bytes) HIP_TRY(hipMemcpyAsync(const_cast<void*>(dst), src, bytes, hipMemcpyHostToDevice, s));
    return 0;
}

// One search.  fill(ws, out, rs) names every region of the workspace and of the search's result buffer once,
// as `field = ws.add<T>(n)`, and notes in rs the result slots the download reads.  It runs twice with the same
// counts: over two empty layouts, for the sizes the buffers must hold, and, once they hold them, over the
// buffers, for the addresses.  Then, on the caller's (or the main) stream: what the batch left on the chunk
// streams (keypoints, descriptors, grid, mvuRight) first, then upload(s), then launch(s).  The host inputs
// are pageable: the call waits, so the caller may reuse them on return -- and the workspace is free for the
// next search.  Last, the search's record says where its results lie and what they cover.
template <class Fill, class Upload, class Launch>
int run_search(orbgpu_ctx* c, void* stream, SearchResult& res, const char* search, MatchCover cover, Fill&& fill,
               Upload&& upload, Launch&& launch) {
    ResultSlots rs;
    Layout ws, out;
    fill(ws, out, rs);
    if (out.bytes > res.buf.bytes) no_results(res);  // the rows of the last call go with the buffer they lie in
    if (c->work.ensure(ws.bytes) || res.buf.ensure(out.bytes))
        return fail(ORBGPU_ERR_HIP, std::string("hipMalloc failed (") + search + ")");
    ws = Layout{(uintptr_t)c->work.p};
    out = Layout{(uintptr_t)res.buf.p};
    fill(ws, out, rs);
    hipStream_t s = stream ? (hipStream_t)stream : c->stream;
    if (int r = join_all(c, s)) return r;
    if (int r = upload(s)) return r;
    if (int r = timed(c, ST_SBP, s, [&] { return launch(s); })) return r;
    HIP_TRY(hipStreamSynchronize(s));
    c->need_fork = true;  // the next batch's chunk streams must not overwrite what this reads
    res.at = rs;
    res.cover = std::move(cover);
    return ORBGPU_OK;
}

// Result row `row` of the search's last call: its match row, its count and (when rot_hist is set) its
// rotation histogram, from the slots the call recorded.
int download_matches(orbgpu_ctx* c, const SearchResult& res, int row, const char* bad_row, int32_t* match, int cap,
                     int* n_kp, int* nmatches, int32_t* rot_hist) {
    const MatchCover& cover = res.cover;
    if (row < 0 || (size_t)row >= cover.image.size()) return fail(ORBGPU_ERR_INVALID, bad_row);
    if (int e_ = ctx_sync(c)) return e_;  // (sets the device)
    int32_t nk[2] = {0, 0}, nm = 0;
    D2H(nk, c->outn.as<int32_t>() + cover.image[(size_t)row], cover.two_cam ? 8 : 4);
    D2H(&nm, res.at.nmatches + row, 4);
    if (int e = count_status(nk[0])) return e;
    if (cover.two_cam)
        if (int e = count_status(nk[1])) return e;
    if (!cover.two_cam) nk[1] = 0;
    const int n = nk[0] + nk[1];  // two-camera frames: Nleft + Nright, the right ones from Nleft on
    if (n_kp) *n_kp = n;
    if (nmatches) *nmatches = nm;
    if (rot_hist) D2H(rot_hist, res.at.hist + (size_t)row * kRotBins, 4 * kRotBins);
    if (n > cap) return fail(ORBGPU_ERR_CAPACITY, "caller capacity too small");
    if (match && n) D2H(match, res.at.match + (size_t)row * res.at.row_cap, 4 * (size_t)n);
    return ORBGPU_OK;
}

size_t row_cap(const orbgpu_ctx* c, bool two_cam) { return (two_cam ? 2 : 1) * (size_t)c->plan.out_cap; }

// Shared by the pinhole and two-camera entry points (orb_sbp.hip).
int sbp_run(orbgpu_ctx* c, int n_frames, int image_step, int two_cam, int use_uright,
            const orbgpu_map_point* mps, const int32_t* mp_offsets, const int32_t* l2r, const int32_t* r2l,
            int lr_stride, const uint8_t* kp_block, int kp_stride, float th, float nnratio, int far_points,
            float th_far, void* stream) {
    static_assert(sizeof(orbgpu_map_point) == sizeof(MapPointIn), "map point layout");
    if (!c || !mp_offsets || n_frames < 1) return fail(ORBGPU_ERR_INVALID, "null argument");
    const int images_needed = (n_frames - 1) * image_step + (two_cam ? 2 : 1);
    if (image_step < 1 || images_needed > c->grid_images)
        return fail(ORBGPU_ERR_INVALID, "frames must lie in the last orbgpu_undistort_grid_batch");
    if (use_uright && (image_step != 2 || n_frames > c->stereo_pairs))
        return fail(ORBGPU_ERR_INVALID, "mvuRight needs image_step 2 and a stereo_matches_batch over the pairs");
    if (sbp_resolve_lds_bytes(c->plan.out_cap, two_cam) > 160 * 1024)
        return fail(ORBGPU_ERR_CAPACITY, "keypoint capacity above the matcher's LDS budget");
    if ((kp_block && kp_stride < 1) || ((l2r || r2l) && lr_stride < 1))
        return fail(ORBGPU_ERR_INVALID, "stride");
    int max_mps, total;
    if (int e = check_offsets(mp_offsets, n_frames, false, "mp_offsets", &max_mps, &total)) return e;
    if (total > 0 && !mps) return fail(ORBGPU_ERR_INVALID, "null map points");
    HIP_TRY(hipSetDevice(c->device));
    const size_t cap = (size_t)c->plan.out_cap, ncap = row_cap(c, two_cam), nf = (size_t)n_frames;
    SearchResult& res = c->res[S_SBP];
    SbpArgs a{};
    bind_frame(a, c);
    bind_grid(a, c);
    bind_scale(a, c);
    a.uright = use_uright ? c->stur.as<float>() : nullptr;
    a.two_cam = two_cam;
    a.image_step = image_step;
    a.img0 = 0;
    a.th = th;
    a.nnratio = nnratio;
    a.th_far = th_far;
    a.far_points = far_points != 0;
    a.factor = th != 1.0;  // bFactor (:48)
    return run_search(
        c, stream, res, "projection search", cover_of(nf, nullptr, image_step, two_cam != 0),
        [&](Layout& ws, Layout& out, ResultSlots& rs) {
            a.mps = ws.add<MapPointIn>((size_t)total);
            a.mp_off = ws.add<int32_t>(nf + 1);
            a.cand = ws.add<SbpCand>((size_t)total);
            a.kp_block = kp_block ? ws.add<uint8_t>(nf * ncap) : nullptr;
            a.l2r = l2r ? ws.add<int32_t>(nf * cap) : nullptr;
            a.r2l = r2l ? ws.add<int32_t>(nf * cap) : nullptr;
            rs = add_match_rows(out, nf, ncap, a.match, a.nmatches, nullptr, 0);
        },
        [&](hipStream_t s) -> int {
            if (int e = h2d(a.mps, mps, (size_t)total * sizeof(MapPointIn), s)) return e;
            if (int e = h2d(a.mp_off, mp_offsets, (nf + 1) * 4, s)) return e;
            if (int e = upload_rows(a.kp_block, ncap, kp_block, kp_stride, std::min((size_t)kp_stride, ncap), nf, 0, s)) return e;
            const size_t lrw = std::min((size_t)lr_stride, cap) * 4;
            if (int e = upload_rows(a.l2r, cap * 4, l2r, (size_t)lr_stride * 4, lrw, nf, 0xFF, s)) return e;
            return upload_rows(a.r2l, cap * 4, r2l, (size_t)lr_stride * 4, lrw, nf, 0xFF, s);
        },
        [&](hipStream_t s) { return launch_sbp(a, n_frames, max_mps, s); });
}

// Shared by the pinhole entry point (K, rig == nullptr) and the two-camera one (rig, K == nullptr:
// frame f = images 2f and 2f + 1; kp_block and the match array cover Nleft + Nright keypoints).
int track_run(orbgpu_ctx* c, int n_frames, int image_step, int use_uright, const orbgpu_last_point* pts,
              const int32_t* pt_offsets, const orbgpu_track_pose* poses, const float* K,
              const orbgpu_track_rig* rig, float mbf, float mb, const uint8_t* kp_block, int kp_stride, float th,
              int mono, int check_orientation, void* stream) {
    static_assert(sizeof(orbgpu_last_point) == sizeof(LastPointIn) && sizeof(orbgpu_last_point) == 56,
                  "last point layout");
    static_assert(sizeof(orbgpu_track_pose) == 96, "track pose layout");
    static_assert(sizeof(orbgpu_track_rig) == sizeof(TrackRig) && sizeof(orbgpu_track_rig) == 80, "track rig layout");
    const bool two_cam = rig != nullptr;
    if (!c || !pt_offsets || !poses || (!K && !rig) || n_frames < 1) return fail(ORBGPU_ERR_INVALID, "null argument");
    if (image_step != 1 && image_step != 2) return fail(ORBGPU_ERR_INVALID, "image_step must be 1 or 2");
    if ((n_frames - 1) * image_step + (two_cam ? 2 : 1) > c->grid_images)
        return fail(ORBGPU_ERR_INVALID, "frames must lie in the last orbgpu_undistort_grid_batch");
    if (use_uright && (image_step != 2 || n_frames > c->stereo_pairs))
        return fail(ORBGPU_ERR_INVALID, "mvuRight needs image_step 2 and a stereo_matches_batch over the pairs");
    if (track_resolve_lds_bytes(c->plan.out_cap) > 160 * 1024)
        return fail(ORBGPU_ERR_CAPACITY, "keypoint capacity above the matcher's LDS budget");
    if (kp_block && kp_stride < 1) return fail(ORBGPU_ERR_INVALID, "stride");
    int max_pts, total;
    if (int e = check_offsets(pt_offsets, n_frames, false, "pt_offsets", &max_pts, &total)) return e;
    if (total > 0 && !pts) return fail(ORBGPU_ERR_INVALID, "null points");
    // the motion direction decides the window's level range (:1727-1734)
    std::vector<TrackFrame> frames(n_frames);
    for (int f = 0; f < n_frames; ++f) {
        const orbgpu_track_pose& P = poses[f];
        TrackFrame& T = frames[f];
        std::memcpy(T.Rcw, P.Rcw, sizeof T.Rcw);
        std::memcpy(T.tcw, P.tcw, sizeof T.tcw);
        float twc[3];
        for (int k = 0; k < 3; ++k) twc[k] = -((P.Rcw[k] * P.tcw[0] + P.Rcw[3 + k] * P.tcw[1]) + P.Rcw[6 + k] * P.tcw[2]);
        const float tlc_z = ((P.Rlw[6] * twc[0] + P.Rlw[7] * twc[1]) + P.Rlw[8] * twc[2]) + P.tlw[2];
        T.dir = mono ? 0 : tlc_z > mb ? kTrackForward : -tlc_z > mb ? kTrackBackward : 0;
        T.pad[0] = T.pad[1] = T.pad[2] = 0;
    }
    HIP_TRY(hipSetDevice(c->device));
    const size_t cap = row_cap(c, two_cam), nf = (size_t)n_frames;
    const size_t sides = two_cam ? 2 : 1;  // candidate records per point
    SearchResult& res = c->res[S_TRACK];
    TrackStereoArgs a{};
    bind_frame(a, c);
    bind_grid(a, c);
    bind_scale(a, c);
    a.uright = use_uright ? c->stur.as<float>() : nullptr;
    a.image_step = image_step;
    for (int k = 0; k < 4; ++k) a.K[k] = K ? K[k] : 0.f;
    a.mbf = mbf;
    a.th = th;
    a.check_orientation = check_orientation != 0;
    if (two_cam) std::memcpy(&a.rig, rig, sizeof a.rig);
    return run_search(
        c, stream, res, "motion-model search", cover_of(nf, nullptr, image_step, two_cam),
        [&](Layout& ws, Layout& out, ResultSlots& rs) {
            a.pts = ws.add<LastPointIn>((size_t)total);
            a.pt_off = ws.add<int32_t>(nf + 1);
            a.frames = ws.add<TrackFrame>(nf);
            a.cand = ws.add<TrackCand>(sides * total);
            a.kp_block = kp_block ? ws.add<uint8_t>(nf * cap) : nullptr;
            a.side_mask = two_cam ? ws.add<uint32_t>(nf * cap) : nullptr;
            a.side_hist = two_cam ? ws.add<int32_t>(nf * 2 * (kRotBins + 1)) : nullptr;
            rs = add_match_rows(out, nf, cap, a.match, a.nmatches, &a.rot_hist, kRotBins);
        },
        [&](hipStream_t s) -> int {
            if (int e = h2d(a.pts, pts, (size_t)total * sizeof(LastPointIn), s)) return e;
            if (int e = h2d(a.pt_off, pt_offsets, (nf + 1) * 4, s)) return e;
            if (int e = h2d(a.frames, frames.data(), nf * sizeof(TrackFrame), s)) return e;
            return upload_rows(a.kp_block, cap, kp_block, kp_stride, std::min((size_t)kp_stride, cap), nf, 0, s);
        },
        [&](hipStream_t s) {
            return two_cam ? launch_track_stereo(a, n_frames, max_pts, s)
                           : launch_track(static_cast<const TrackArgs&>(a), n_frames, max_pts, s);
        });
}

// MapPoint::PredictScale before its clamps (MapPoint.cc:541): log(float) is the host libm's logf
int predicted_scale(float ratio, float log_scale) { return (int)std::ceil(std::log(ratio) / log_scale); }

// thresholds[n] = the largest float r with ceilf(logf(r) / logf(scale_factor)) <= n, by bisection over the
// bit patterns of the positive floats (the step function is monotone in r)
void predict_scale_table(float scale_factor, int nlevels, float* thresholds) {
    const float log_scale = std::log(scale_factor);
    auto as_float = [](uint32_t b) {
        float f;
        std::memcpy(&f, &b, 4);
        return f;
    };
    for (int n = 0; n + 1 < nlevels; ++n) {
        uint32_t lo = 0x00000001u, hi = 0x7F7FFFFFu;  // the predicate holds at lo
        if (predicted_scale(as_float(hi), log_scale) <= n) lo = hi;
        while (hi - lo > 1) {
            const uint32_t mid = lo + (hi - lo) / 2;
            if (predicted_scale(as_float(mid), log_scale) <= n) lo = mid; else hi = mid;
        }
        thresholds[n] = as_float(lo);
    }
}

// What orbgpu_fuse_batch and orbgpu_sim3_search_by_projection_batch share: pairs of a batch image and a list
// of points.  head = frames [np], lists [np], the pairs' output rows [np + 1], the list offsets rebased to 0
// [nl + 1]; rows = the output rows of all pairs; max_pts = the longest list a pair names; skip_pitch = the
// device pitch of the skip rows.
struct ListPairs {
    std::vector<int32_t> head;
    int max_pts = 0, total_pts = 0;
    size_t rows = 0, skip_pitch = 1;
};

// The checks on those arguments, in orbgpu_fuse_batch's order (pair_check(p): the caller's own test of pair
// p), then the head.  n_pairs == 0 passes with an empty head.
template <class PairCheck>
int check_list_pairs(orbgpu_ctx* c, int n_pairs, const int32_t* frames, const int32_t* lists, int n_lists,
                     const void* pts, const int32_t* list_offsets, const void* poses, const float* K,
                     const uint8_t* skip, int skip_stride, ListPairs* lp, PairCheck&& pair_check) {
    if (n_pairs > 0 && (!frames || !lists || !list_offsets || !poses || !K)) return fail(ORBGPU_ERR_INVALID, "null array");
    if (n_pairs > 0 && n_lists < 1) return fail(ORBGPU_ERR_INVALID, "no lists");
    for (int p = 0; p < n_pairs; ++p) {
        if (frames[p] < 0 || frames[p] >= c->grid_images)
            return fail(ORBGPU_ERR_INVALID, "frames must lie in the last orbgpu_undistort_grid_batch");
        if (lists[p] < 0 || lists[p] >= n_lists) return fail(ORBGPU_ERR_INVALID, "list outside [0, n_lists)");
        if (int e = pair_check(p)) return e;
    }
    int max_list = 0;
    if (n_pairs > 0)
        if (int e = check_offsets(list_offsets, n_lists, true, "list_offsets", &max_list, &lp->total_pts)) return e;
    if (lp->total_pts > 0 && !pts) return fail(ORBGPU_ERR_INVALID, "null points");
    for (int p = 0; p < n_pairs; ++p)  // over the lists the pairs name
        lp->max_pts = std::max(lp->max_pts, list_offsets[lists[p] + 1] - list_offsets[lists[p]]);
    if (n_pairs > 0 && skip && skip_stride < lp->max_pts) return fail(ORBGPU_ERR_INVALID, "skip_stride below a list's length");
    if (max_list > kFuseMaxPoints) return fail(ORBGPU_ERR_CAPACITY, "a list holds more than ORBGPU_FUSE_MAX_POINTS points");
    if ((long long)n_pairs * lp->max_pts > INT32_MAX) return fail(ORBGPU_ERR_CAPACITY, "more point rows than an int32 counts");
    if (n_pairs == 0) return 0;
    const size_t np = (size_t)n_pairs, nl = (size_t)n_lists;
    std::vector<int32_t>& head = lp->head;
    head.resize(3 * np + 1 + nl + 1);
    std::copy(frames, frames + np, head.begin());
    std::copy(lists, lists + np, head.begin() + np);
    head[2 * np] = 0;
    for (size_t p = 0; p < np; ++p)
        head[2 * np + p + 1] = head[2 * np + p] + (list_offsets[lists[p] + 1] - list_offsets[lists[p]]);
    for (size_t l = 0; l <= nl; ++l) head[3 * np + 1 + l] = list_offsets[l] - list_offsets[0];
    lp->rows = (size_t)head[3 * np];  // at most max_images * ORBGPU_FUSE_MAX_POINTS
    lp->skip_pitch = (size_t)std::max(lp->max_pts, 1);
    return 0;
}

// What fuse and sim3 lay out alike in the workspace, into the fields FuseArgs and Sim3Args name alike: the
// head (frames, lists [np each], out_off [np + 1], list_off), the points, the poses and the skip rows.
template <class Args>
void add_list_regions(Layout& ws, Args& a, const ListPairs& lp, size_t np, bool skip) {
    a.frames = ws.add<int32_t>(lp.head.size());
    a.lists = a.frames + np;
    a.out_off = a.lists + np;
    a.list_off = a.out_off + np + 1;
    a.pts = ws.add<FusePoint>((size_t)lp.total_pts);
    a.poses = ws.add<RelocPose>(np);
    a.skip = skip ? ws.add<uint8_t>(np * lp.skip_pitch) : nullptr;
    a.skip_stride = (int)lp.skip_pitch;
}

// Their uploads (pts: the caller's, from list_offsets[0] on).
template <class Args>
int upload_list_inputs(const Args& a, const ListPairs& lp, size_t np, const void* pts, const void* poses,
                       const uint8_t* skip, int skip_stride, hipStream_t s) {
    if (int e = h2d(a.frames, lp.head.data(), lp.head.size() * 4, s)) return e;
    if (int e = h2d(a.pts, pts, (size_t)lp.total_pts * sizeof(FusePoint), s)) return e;
    if (int e = h2d(a.poses, poses, np * sizeof(RelocPose), s)) return e;
    return upload_rows(a.skip, lp.skip_pitch, skip, (size_t)skip_stride, (size_t)lp.max_pts, np, 0, s);
}

// Their result slots of the point side, one entry per output row of all pairs.
template <class Args>
void add_point_rows(Layout& out, ResultSlots& rs, Args& a, size_t rows) {
    rs.best_idx = a.best_idx = out.add<int32_t>(rows);
    rs.best_dist = a.best_dist = out.add<int32_t>(rows);
    rs.code = a.code = out.add<uint8_t>(rows);
}

// The point side of a download (fuse, sim3): pair `pair`'s rows of best_idx, best_dist and code, after the
// keypoint side `r` has written its count: both counts are out before either capacity is judged.
int download_point_rows(orbgpu_ctx* c, const SearchResult& res, int pair, int r, int32_t* best_idx, int32_t* best_dist,
                        uint8_t* code, int cap_points, int* n_points) {
    const size_t row0 = (size_t)res.point_off[(size_t)pair];
    const int n = res.point_off[(size_t)pair + 1] - res.point_off[(size_t)pair];
    if (n_points) *n_points = n;
    if (r && r != ORBGPU_ERR_CAPACITY) return r;
    if (n > cap_points) return fail(ORBGPU_ERR_CAPACITY, "caller capacity too small (points)");
    if (r) return r;
    if (best_idx && n) D2H(best_idx, res.at.best_idx + row0, 4 * (size_t)n);
    if (best_dist && n) D2H(best_dist, res.at.best_dist + row0, 4 * (size_t)n);
    if (code && n) D2H(code, res.at.code + row0, (size_t)n);
    return ORBGPU_OK;
}

// The three searches over vocabulary nodes (bow, tri, bowkf): np pairs of a batch image (up to cap keypoints)
// and a keyframe of the host's points (nkf in all), and a head of head_bytes: frames [np], kf_off [np + 1],
// then what a search appends of its own.
struct NodeDims { size_t np, nkf, cap, head_bytes; };

// What the three lay out alike in the workspace, into the fields BowArgs, TriArgs and BowKfArgs name alike:
// the head, the keyframe points, the node rows, what the grouping kernel leaves for the match kernel
// (orb_bow_group.h), and match_bin, which the match kernel writes and the finish kernel of the same call
// reads: no download does, so it lies in the workspace.
template <class Args>
void add_node_regions(Layout& ws, Args& a, const NodeDims& d) {
    a.frames = reinterpret_cast<const int32_t*>(ws.add<uint8_t>(d.head_bytes));
    a.kf_off = a.frames + d.np;
    a.kf_pts = ws.add<std::remove_pointer_t<decltype(a.kf_pts)>>(d.nkf);
    a.f_nodes = ws.add<int32_t>(d.np * d.cap);
    a.kf_order = ws.add<int32_t>(d.nkf);
    a.kf_seg_node = ws.add<int32_t>(d.nkf);
    a.kf_seg_start = ws.add<int32_t>(d.nkf + d.np);  // pair p at kf_off[p] + p
    a.f_order = ws.add<int32_t>(d.np * d.cap);
    a.f_seg_node = ws.add<int32_t>(d.np * d.cap);
    a.f_seg_start = ws.add<int32_t>(d.np * (d.cap + 1));
    a.nseg = ws.add<int32_t>(2 * d.np);
    a.f_desc = ws.add<uint8_t>(d.np * d.cap * 32);
    a.match_bin = ws.add<uint8_t>(d.np * d.cap);
}

// The uploads the three share: the head, the keyframe points (the caller's, from kf_offsets[0] on), the flag
// rows filled with 0 (into d_flags; f_flags == nullptr: none) and the node rows filled with -1.
template <class Args>
int upload_node_inputs(const Args& a, const uint8_t* d_flags, const NodeDims& d, const void* head, const void* kf_pts,
                       const int32_t* f_nodes, int node_stride, const uint8_t* f_flags, int flag_stride, hipStream_t s) {
    if (int e = h2d(a.frames, head, d.head_bytes, s)) return e;
    if (int e = h2d(a.kf_pts, kf_pts, d.nkf * sizeof *a.kf_pts, s)) return e;
    if (int e = upload_rows(d_flags, d.cap, f_flags, (size_t)flag_stride, std::min((size_t)flag_stride, d.cap), d.np, 0, s)) return e;
    return upload_rows(a.f_nodes, d.cap * 4, f_nodes, (size_t)node_stride * 4, std::min((size_t)node_stride, d.cap) * 4, d.np, -1, s);
}

// The checks the three make alike, in the order all three keep: every pair's image lies among the first
// n_images of the batch (`where`: the message otherwise), the offsets ascend, no stride is negative.
int check_node_pairs(int n_pairs, const int32_t* frames, int n_images, const char* where, const int32_t* kf_offsets,
                     bool negative_stride, const char* stride_msg, int* max_kf, int* total) {
    for (int p = 0; p < n_pairs; ++p)
        if (frames[p] < 0 || frames[p] >= n_images) return fail(ORBGPU_ERR_INVALID, where);
    if (int e = check_offsets(kf_offsets, n_pairs, true, "kf_offsets", max_kf, total)) return e;
    if (n_pairs > 0 && negative_stride) return fail(ORBGPU_ERR_INVALID, stride_msg);
    return 0;
}

// *max_side = the longest side the grouping kernel orders in LDS: the context's keypoint capacity, or a keyframe
int check_max_side(const orbgpu_ctx* c, int max_kf, int* max_side) {
    *max_side = std::max(c->plan.out_cap, max_kf);
    if (*max_side > kBowMaxPoints)
        return fail(ORBGPU_ERR_CAPACITY, "more keypoints on a side than the grouping kernel orders (ORBGPU_BOW_MAX_POINTS)");
    return 0;
}

}  // namespace

extern "C" {

// ---- ORBmatcher::SearchByProjection(F, vpMapPoints, th, bFarPoints, thFarPoints) (orb_sbp.hip) ----
int orbgpu_search_by_projection_batch(orbgpu_ctx* c, int n_frames, int image_step, int use_uright,
                                      const orbgpu_map_point* mps, const int32_t* mp_offsets,
                                      const uint8_t* kp_block, int kp_stride, float th, float nnratio,
                                      int far_points, float th_far, void* stream) {
    return sbp_run(c, n_frames, image_step, 0, use_uright, mps, mp_offsets, nullptr, nullptr, 0, kp_block,
                   kp_stride, th, nnratio, far_points, th_far, stream);
}

int orbgpu_search_by_projection_stereo(orbgpu_ctx* c, int n_pairs, const orbgpu_map_point* mps,
                                       const int32_t* mp_offsets, const int32_t* left_to_right,
                                       const int32_t* right_to_left, int lr_stride, const uint8_t* kp_block,
                                       int kp_stride, float th, float nnratio, int far_points, float th_far,
                                       void* stream) {
    return sbp_run(c, n_pairs, 2, 1, 0, mps, mp_offsets, left_to_right, right_to_left, lr_stride, kp_block,
                   kp_stride, th, nnratio, far_points, th_far, stream);
}

int orbgpu_download_projection_matches(orbgpu_ctx* c, int frame, int32_t* match, int cap, int* n_kp,
                                       int* nmatches) {
    if (!c) return fail(ORBGPU_ERR_INVALID, "bad frame");
    return download_matches(c, c->res[S_SBP], frame, "bad frame", match, cap, n_kp, nmatches, nullptr);
}

// ---- ORBmatcher::SearchByProjection(CurrentFrame, LastFrame, th, bMono) (orb_track.hip) --------
int orbgpu_track_by_projection_batch(orbgpu_ctx* c, int n_frames, int image_step, int use_uright,
                                     const orbgpu_last_point* pts, const int32_t* pt_offsets,
                                     const orbgpu_track_pose* poses, const float K[4], float mbf, float mb,
                                     const uint8_t* kp_block, int kp_stride, float th, int mono,
                                     int check_orientation, void* stream) {
    if (!K) return fail(ORBGPU_ERR_INVALID, "null argument");
    return track_run(c, n_frames, image_step, use_uright, pts, pt_offsets, poses, K, nullptr, mbf, mb, kp_block,
                     kp_stride, th, mono, check_orientation, stream);
}

int orbgpu_track_by_projection_stereo(orbgpu_ctx* c, int n_pairs, const orbgpu_last_point* pts,
                                      const int32_t* pt_offsets, const orbgpu_track_pose* poses,
                                      const orbgpu_track_rig* rig, float mb, const uint8_t* kp_block, int kp_stride,
                                      float th, int mono, int check_orientation, void* stream) {
    if (!rig) return fail(ORBGPU_ERR_INVALID, "null argument");
    return track_run(c, n_pairs, 2, 0, pts, pt_offsets, poses, nullptr, rig, 0.f, mb, kp_block, kp_stride, th, mono,
                     check_orientation, stream);
}

int orbgpu_download_track_matches(orbgpu_ctx* c, int frame, int32_t* match, int cap, int* n_kp, int* nmatches,
                                  int32_t rot_hist[30]) {
    if (!c) return fail(ORBGPU_ERR_INVALID, "bad frame");
    return download_matches(c, c->res[S_TRACK], frame, "bad frame", match, cap, n_kp, nmatches, rot_hist);
}

// ---- ORBmatcher::SearchForInitialization (orb_init.hip) -----------------------------------------
int orbgpu_search_for_initialization_batch(orbgpu_ctx* c, int n_pairs, const int32_t* image_pairs,
                                           const float* prev_matched, int pm_stride, int window_size, float nnratio,
                                           int check_orientation, void* stream) {
    if (!c) return fail(ORBGPU_ERR_INVALID, "null ctx");
    if (n_pairs < 0 || n_pairs > c->max_images) return fail(ORBGPU_ERR_INVALID, "bad pair count");
    if (n_pairs > 0 && !image_pairs) return fail(ORBGPU_ERR_INVALID, "null image pairs");
    if (window_size < 0) return fail(ORBGPU_ERR_INVALID, "negative window");
    for (int k = 0; k < 2 * n_pairs; ++k)
        if (image_pairs[k] < 0 || image_pairs[k] >= c->grid_images)
            return fail(ORBGPU_ERR_INVALID, "images must lie in the last orbgpu_undistort_grid_batch");
    if (n_pairs > 0 && init_replay_lds_bytes(c->plan.out_cap) > 160 * 1024)
        return fail(ORBGPU_ERR_CAPACITY, "keypoint capacity above the matcher's LDS budget");
    SearchResult& res = c->res[S_INIT];
    if (n_pairs == 0) return no_results(res);
    const size_t cap = (size_t)c->plan.out_cap, np = (size_t)n_pairs;
    if (prev_matched)  // one row of pm_stride points per pair: it must cover F1's keypoints
        if (int e = rows_cover_counts(c, c->grid_images, image_pairs, 2, n_pairs, pm_stride,
                                      "pm_stride below F1's keypoint count"))
            return e;
    HIP_TRY(hipSetDevice(c->device));
    InitArgs a{};
    bind_frame(a, c);
    bind_grid(a, c);
    a.window = (float)window_size;
    a.nnratio = nnratio;
    a.check_orientation = check_orientation != 0;
    return run_search(
        c, stream, res, "initialization search", cover_of(np, image_pairs, 2, false),  // the rows are over F1's keypoints
        [&](Layout& ws, Layout& out, ResultSlots& rs) {
            a.pairs = ws.add<int32_t>(2 * np);
            a.nsearch = ws.add<int32_t>(np);
            a.prev = prev_matched ? ws.add<float>(np * cap * 2) : nullptr;
            a.cand = ws.add<InitCand>(np * cap);
            a.l0_desc = ws.add<uint8_t>(np * cap * 32);
            a.l0_xy = ws.add<float>(np * cap * 2);
            a.l0_idx = ws.add<int32_t>(np * cap);
            a.l0_pre = ws.add<int32_t>(np * (cap + 1));
            rs = add_match_rows(out, np, cap, a.match12, a.nmatches, &a.rot_hist, kRotBins);
            rs.prev_out = a.prev_out = out.add<float>(np * cap * 2);
        },
        [&](hipStream_t s) -> int {
            if (int e = h2d(a.pairs, image_pairs, np * 8, s)) return e;
            HIP_TRY(hipMemsetAsync(a.nsearch, 0, np * 4, s));  // the searched-keypoint counts
            return upload_rows(a.prev, cap * 8, prev_matched, (size_t)pm_stride * 8, std::min((size_t)pm_stride, cap) * 8, np, -1, s);
        },
        [&](hipStream_t s) { return launch_init_search(a, n_pairs, s); });
}

int orbgpu_download_initialization_matches(orbgpu_ctx* c, int pair, int32_t* match12, float* prev_matched, int cap,
                                           int* n1, int* nmatches, int32_t rot_hist[30]) {
    if (!c) return fail(ORBGPU_ERR_INVALID, "bad pair");
    const SearchResult& res = c->res[S_INIT];
    int nk = 0;
    int* pn = n1 ? n1 : &nk;
    if (int r = download_matches(c, res, pair, "bad pair", match12, cap, pn, nmatches, rot_hist)) return r;
    if (prev_matched && *pn) D2H(prev_matched, res.at.prev_out + 2 * (size_t)pair * res.at.row_cap, 8 * (size_t)*pn);
    return ORBGPU_OK;
}

// ---- ORBmatcher::SearchByBoW(KeyFrame*, Frame&, ...) (orb_bow.hip) -------------------------------
static_assert(sizeof(orbgpu_bow_point) == 44 && sizeof(BowPoint) == 44, "orbgpu_bow_point is 44 bytes");
static_assert(ORBGPU_BOW_MAX_POINTS == kBowMaxPoints, "the header states the grouping kernel's limit");

int orbgpu_search_by_bow_batch(orbgpu_ctx* c, int n_pairs, const int32_t* frames, const orbgpu_bow_point* kf_pts,
                               const int32_t* kf_offsets, const int32_t* f_nodes, int node_stride, float nnratio,
                               int check_orientation, void* stream) {
    if (!c) return fail(ORBGPU_ERR_INVALID, "null ctx");
    if (n_pairs < 0 || n_pairs > c->max_images) return fail(ORBGPU_ERR_INVALID, "bad pair count");
    if (n_pairs > 0 && (!frames || !kf_pts || !kf_offsets || !f_nodes)) return fail(ORBGPU_ERR_INVALID, "null array");
    int max_kf, total, max_side;
    if (int e = check_node_pairs(n_pairs, frames, c->last_images, "frames must lie in the last orbgpu_run_batch", kf_offsets,
                                 node_stride < 0, "negative node_stride", &max_kf, &total))
        return e;
    SearchResult& res = c->res[S_BOW];
    if (n_pairs == 0) return no_results(res);
    // one row of node_stride nodes per pair: it must cover the frame's keypoints
    if (int e = rows_cover_counts(c, c->last_images, frames, 1, n_pairs, node_stride,
                                  "node_stride below the frame's keypoint count"))
        return e;
    if (int e = check_max_side(c, max_kf, &max_side)) return e;
    const size_t cap = (size_t)c->plan.out_cap, np = (size_t)n_pairs;
    const std::vector<int32_t> head = frames_and_offsets(frames, kf_offsets, np);
    const NodeDims d{np, (size_t)total, cap, head.size() * 4};
    HIP_TRY(hipSetDevice(c->device));
    BowArgs a{};
    bind_frame(a, c);
    a.nnratio = nnratio;
    a.check_orientation = check_orientation != 0;
    return run_search(
        c, stream, res, "bag-of-words search", cover_of(np, frames, 1, false),
        [&](Layout& ws, Layout& out, ResultSlots& rs) {
            add_node_regions(ws, a, d);
            rs = add_match_rows(out, np, cap, a.match, a.nmatches, &a.rot_hist, kRotBins);
        },
        [&](hipStream_t s) {
            return upload_node_inputs(a, nullptr, d, head.data(), kf_pts + kf_offsets[0], f_nodes, node_stride, nullptr, 0, s);
        },
        [&](hipStream_t s) { return launch_bow_search(a, n_pairs, max_side, s); });
}

int orbgpu_download_bow_matches(orbgpu_ctx* c, int pair, int32_t* match, int cap, int* n_kp, int* nmatches,
                                int32_t rot_hist[30]) {
    if (!c) return fail(ORBGPU_ERR_INVALID, "bad pair");
    return download_matches(c, c->res[S_BOW], pair, "bad pair", match, cap, n_kp, nmatches, rot_hist);
}

// ---- ORBmatcher::SearchForTriangulation(pKF1, pKF2, ...) on pinhole keyframes (orb_tri.hip) --------
static_assert(sizeof(orbgpu_triang_point) == 56 && sizeof(TriPoint) == 56, "orbgpu_triang_point is 56 bytes");
static_assert(sizeof(orbgpu_triang_pair) == 44 && sizeof(TriPair) == 44, "orbgpu_triang_pair is 44 bytes");
static_assert(ORBGPU_TRI_HAS_POINT == kTriHasPoint && ORBGPU_TRI_STEREO == kTriStereo, "the header states the flag bits");

int orbgpu_search_for_triangulation_batch(orbgpu_ctx* c, int n_pairs, const int32_t* frames,
                                          const orbgpu_triang_point* kf_pts, const int32_t* kf_offsets,
                                          const orbgpu_triang_pair* pairs, const int32_t* f_nodes, int node_stride,
                                          const uint8_t* f_flags, int flag_stride, int only_stereo, int coarse,
                                          int check_orientation, void* stream) {
    if (!c) return fail(ORBGPU_ERR_INVALID, "null ctx");
    if (n_pairs < 0 || n_pairs > c->max_images) return fail(ORBGPU_ERR_INVALID, "bad pair count");
    if (n_pairs > 0 && (!frames || !kf_pts || !kf_offsets || !pairs || !f_nodes))
        return fail(ORBGPU_ERR_INVALID, "null array");
    int max_kf, total, max_side;
    if (int e = check_node_pairs(n_pairs, frames, c->grid_images, "frames must lie in the last orbgpu_undistort_grid_batch",
                                 kf_offsets, node_stride < 0 || (f_flags && flag_stride < 0), "negative stride", &max_kf, &total))
        return e;
    SearchResult& res = c->res[S_TRI];
    if (n_pairs == 0) return no_results(res);
    const size_t cap = (size_t)c->plan.out_cap, np = (size_t)n_pairs, nkf = (size_t)total;
    if (int e = check_max_side(c, max_kf, &max_side)) return e;
    for (size_t i = 0; i < nkf; ++i)  // the level tables are indexed with it
        if (kf_pts[kf_offsets[0] + i].octave < 0 || kf_pts[kf_offsets[0] + i].octave >= c->prm.nlevels)
            return fail(ORBGPU_ERR_INVALID, "octave of a keyframe point outside [0, nlevels)");
    // one row of nodes (and of flags) per pair: it must cover keyframe 1's keypoints
    if (int e = rows_cover_counts(c, c->grid_images, frames, 1, n_pairs, f_flags ? std::min(node_stride, flag_stride) : node_stride,
                                  "node_stride or flag_stride below the frame's keypoint count"))
        return e;
    // the head: frames [np], offsets [np + 1], the pairs, then (8-byte aligned) the two level tables
    const std::vector<int32_t> head = frames_and_offsets(frames, kf_offsets, np);
    const size_t pairs_at = head.size() * 4, tab_at = (pairs_at + np * sizeof(TriPair) + 7) & ~(size_t)7;
    std::vector<uint8_t> in(tab_at + kMaxLevels * 12, 0);
    std::memcpy(in.data(), head.data(), pairs_at);
    std::memcpy(in.data() + pairs_at, pairs, np * sizeof(TriPair));
    for (int l = 0; l < c->prm.nlevels; ++l) {
        const double epi = 3.84 * (double)c->tab.sigma2[l];  // Pinhole.cpp:123: a double product
        const float disc = (float)100 * c->tab.scale[l];     // :1037: int * float
        std::memcpy(in.data() + tab_at + 8 * (size_t)l, &epi, 8);
        std::memcpy(in.data() + tab_at + 8 * (size_t)kMaxLevels + 4 * (size_t)l, &disc, 4);
    }
    const NodeDims d{np, nkf, cap, in.size()};
    HIP_TRY(hipSetDevice(c->device));
    TriArgs a{};
    bind_frame(a, c);
    a.xy_un = c->gxy.as<float>();
    a.nlevels = c->prm.nlevels;
    a.only_stereo = only_stereo != 0;
    a.coarse = coarse != 0;
    a.check_orientation = check_orientation != 0;
    return run_search(
        c, stream, res, "triangulation search", cover_of(np, frames, 1, false),
        [&](Layout& ws, Layout& out, ResultSlots& rs) {
            add_node_regions(ws, a, d);
            const uint8_t* const dhead = reinterpret_cast<const uint8_t*>(a.frames);  // what the head appends
            a.pairs = reinterpret_cast<const TriPair*>(dhead + pairs_at);
            a.epi_th = reinterpret_cast<const double*>(dhead + tab_at);
            a.disc_th = reinterpret_cast<const float*>(a.epi_th + kMaxLevels);
            a.f_flags = f_flags ? ws.add<uint8_t>(np * cap) : nullptr;
            a.kf_desc = ws.add<uint4>(2 * nkf);  // keyframe 2's packed rows: 32 B of descriptor
            a.kf_meta = ws.add<float4>(nkf);     // and 16 B of {x, y, angle, octave and flags} per point
            rs = add_match_rows(out, np, cap, a.match, a.nmatches, &a.rot_hist, kRotBins);
        },
        [&](hipStream_t s) {
            return upload_node_inputs(a, a.f_flags, d, in.data(), kf_pts + kf_offsets[0], f_nodes, node_stride, f_flags, flag_stride, s);
        },
        [&](hipStream_t s) { return launch_tri_search(a, n_pairs, max_side, s); });
}

int orbgpu_download_triangulation_matches(orbgpu_ctx* c, int pair, int32_t* match12, int cap, int* n1, int* nmatches,
                                          int32_t rot_hist[30]) {
    if (!c) return fail(ORBGPU_ERR_INVALID, "bad pair");
    return download_matches(c, c->res[S_TRI], pair, "bad pair", match12, cap, n1, nmatches, rot_hist);
}

// ---- ORBmatcher::SearchByBoW(KeyFrame*, KeyFrame*, ...) on pinhole keyframes (orb_bowkf.hip) --------
static_assert(sizeof(orbgpu_bowkf_point) == sizeof(BowPoint), "orbgpu_bowkf_point is orbgpu_bow_point");
static_assert(ORBGPU_BOWKF_HAS_POINT == ORBGPU_BOW_HAS_POINT, "the two searches share the flag bit");
static_assert(ORBGPU_BOWKF_NO_NODE == kBowKfNoNode && ORBGPU_BOWKF_NODE_NOT_COMMON == kBowKfNodeNotCommon &&
                  ORBGPU_BOWKF_NO_MAP_POINT == kBowKfNoMapPoint && ORBGPU_BOWKF_NO_CANDIDATE == kBowKfNoCandidate &&
                  ORBGPU_BOWKF_NOT_BELOW_TH_LOW == kBowKfNotBelowThLow && ORBGPU_BOWKF_RATIO_FAILED == kBowKfRatioFailed &&
                  ORBGPU_BOWKF_MATCHED == kBowKfMatched && ORBGPU_BOWKF_ROTATION_REJECTED == kBowKfRotationRejected,
              "the header states the decision codes");

int orbgpu_search_by_bow_kf_batch(orbgpu_ctx* c, int n_pairs, const int32_t* frames, const orbgpu_bowkf_point* kf_pts,
                                  const int32_t* kf_offsets, const int32_t* f_nodes, int node_stride,
                                  const uint8_t* f_flags, int flag_stride, float nnratio, int check_orientation,
                                  void* stream) {
    if (!c) return fail(ORBGPU_ERR_INVALID, "null ctx");
    if (n_pairs < 0 || n_pairs > c->max_images) return fail(ORBGPU_ERR_INVALID, "bad pair count");
    if (!std::isfinite(nnratio)) return fail(ORBGPU_ERR_INVALID, "nnratio not finite");
    if (n_pairs > 0 && (!frames || !kf_pts || !kf_offsets || !f_nodes)) return fail(ORBGPU_ERR_INVALID, "null array");
    int max_kf, total, max_side;
    if (int e = check_node_pairs(n_pairs, frames, c->last_images, "frames must lie in the last orbgpu_run_batch", kf_offsets,
                                 node_stride < 0 || (f_flags && flag_stride < 0), "negative stride", &max_kf, &total))
        return e;
    SearchResult& res = c->res[S_BOWKF];
    if (n_pairs == 0) return no_results(res);
    if (int e = check_max_side(c, max_kf, &max_side)) return e;
    // one row of nodes (and of flags) per pair: it must cover keyframe 1's keypoints
    if (int e = rows_cover_counts(c, c->last_images, frames, 1, n_pairs, f_flags ? std::min(node_stride, flag_stride) : node_stride,
                                  "node_stride or flag_stride below the frame's keypoint count"))
        return e;
    const size_t cap = (size_t)c->plan.out_cap, np = (size_t)n_pairs;
    const std::vector<int32_t> head = frames_and_offsets(frames, kf_offsets, np);
    const NodeDims d{np, (size_t)total, cap, head.size() * 4};
    HIP_TRY(hipSetDevice(c->device));
    BowKfArgs a{};
    bind_frame(a, c);
    a.nnratio = nnratio;
    a.check_orientation = check_orientation != 0;
    return run_search(
        c, stream, res, "keyframe bag-of-words search", cover_of(np, frames, 1, false),
        [&](Layout& ws, Layout& out, ResultSlots& rs) {
            add_node_regions(ws, a, d);
            a.f_flags = f_flags ? ws.add<uint8_t>(np * cap) : nullptr;
            a.kf_desc = ws.add<uint4>(2 * d.nkf);  // keyframe 2's packed rows: 32 B of descriptor
            a.kf_meta = ws.add<float2>(d.nkf);     // and 8 B of {angle, flags} per point
            rs = add_match_rows(out, np, cap, a.match, a.nmatches, &a.rot_hist, kRotBins);
            rs.best = a.best = out.add<short2>(np * cap);
            rs.code = a.code = out.add<uint8_t>(np * cap);
        },
        [&](hipStream_t s) {
            return upload_node_inputs(a, a.f_flags, d, head.data(), kf_pts + kf_offsets[0], f_nodes, node_stride, f_flags, flag_stride, s);
        },
        [&](hipStream_t s) { return launch_bowkf_search(a, n_pairs, max_side, s); });
}

int orbgpu_download_bow_kf_matches(orbgpu_ctx* c, int pair, int32_t* match12, uint8_t* code, int16_t* best, int cap,
                                   int* n1, int* nmatches, int32_t rot_hist[30]) {
    if (!c) return fail(ORBGPU_ERR_INVALID, "bad pair");
    const SearchResult& res = c->res[S_BOWKF];
    int nk = 0;
    int* pn = n1 ? n1 : &nk;
    if (int r = download_matches(c, res, pair, "bad pair", match12, cap, pn, nmatches, rot_hist)) return r;
    const size_t row0 = (size_t)pair * res.at.row_cap;
    if (best && *pn) D2H(best, res.at.best + row0, 4 * (size_t)*pn);
    if (code && *pn) D2H(code, res.at.code + row0, (size_t)*pn);
    return ORBGPU_OK;
}

// ---- ORBmatcher::SearchByProjection(Frame&, KeyFrame*, sAlreadyFound, th, ORBdist) (orb_reloc.hip) ----
static_assert(sizeof(orbgpu_reloc_point) == 60 && sizeof(RelocPoint) == 60, "orbgpu_reloc_point is 60 bytes");
static_assert(sizeof(orbgpu_reloc_pose) == 60 && sizeof(RelocPose) == 60, "orbgpu_reloc_pose is 60 bytes");

int orbgpu_predict_scale_table(float scale_factor, int nlevels, float* thresholds) {
    if (!(scale_factor > 1.0f) || !std::isfinite(scale_factor) || nlevels < 1 || nlevels > kMaxLevels ||
        (nlevels > 1 && !thresholds))
        return fail(ORBGPU_ERR_INVALID, "scale_factor above 1, nlevels in [1, 16] and a table of nlevels - 1 entries");
    predict_scale_table(scale_factor, nlevels, thresholds);
    return ORBGPU_OK;
}

int orbgpu_reloc_by_projection_batch(orbgpu_ctx* c, int n_pairs, const int32_t* frames, const orbgpu_reloc_point* pts,
                                     const int32_t* kf_offsets, const orbgpu_reloc_pose* poses, const float K[4],
                                     const uint8_t* kp_block, int kp_stride, float th, int orb_dist,
                                     int check_orientation, void* stream) {
    if (!c) return fail(ORBGPU_ERR_INVALID, "null ctx");
    if (n_pairs < 0 || n_pairs > c->max_images) return fail(ORBGPU_ERR_INVALID, "bad pair count");
    if (orb_dist < 0 || orb_dist > 255) return fail(ORBGPU_ERR_INVALID, "orb_dist outside [0, 255]");
    if (!(th >= 0.0f) || !std::isfinite(th)) return fail(ORBGPU_ERR_INVALID, "th negative or not finite");
    if (n_pairs > 0 && (!frames || !kf_offsets || !poses || !K)) return fail(ORBGPU_ERR_INVALID, "null array");
    for (int p = 0; p < n_pairs; ++p)
        if (frames[p] < 0 || frames[p] >= c->grid_images)
            return fail(ORBGPU_ERR_INVALID, "frames must lie in the last orbgpu_undistort_grid_batch");
    int max_pts, total_pts;
    if (int e = check_offsets(kf_offsets, n_pairs, true, "kf_offsets", &max_pts, &total_pts)) return e;
    if (total_pts > 0 && !pts) return fail(ORBGPU_ERR_INVALID, "null points");
    if (n_pairs > 0 && kp_block && kp_stride < 0) return fail(ORBGPU_ERR_INVALID, "negative kp_stride");
    if (n_pairs > 0 && reloc_resolve_lds_bytes(c->plan.out_cap) > 160 * 1024)
        return fail(ORBGPU_ERR_CAPACITY, "keypoint capacity above the matcher's LDS budget");
    SearchResult& res = c->res[S_RELOC];
    if (n_pairs == 0) return no_results(res);
    const size_t cap = (size_t)c->plan.out_cap, np = (size_t)n_pairs, total = (size_t)total_pts;
    if (kp_block)  // one row of kp_stride flags per pair: it must cover the frame's keypoints
        if (int e = rows_cover_counts(c, c->grid_images, frames, 1, n_pairs, kp_stride,
                                      "kp_stride below the frame's keypoint count"))
            return e;
    const std::vector<int32_t> head = frames_and_offsets(frames, kf_offsets, np);
    HIP_TRY(hipSetDevice(c->device));
    RelocArgs a{};
    bind_frame(a, c);
    bind_grid(a, c);
    bind_scale(a, c);
    predict_scale_table(c->prm.scale_factor, c->prm.nlevels, a.level_step);  // Frame.cc:132 + MapPoint.cc:541
    for (int k = 0; k < 4; ++k) a.K[k] = K[k];
    a.th = th;
    a.orb_dist = orb_dist;
    a.check_orientation = check_orientation != 0;
    return run_search(
        c, stream, res, "relocalisation search", cover_of(np, frames, 1, false),
        [&](Layout& ws, Layout& out, ResultSlots& rs) {
            a.frames = ws.add<int32_t>(head.size());
            a.kf_off = a.frames + np;
            a.pts = ws.add<RelocPoint>(total);
            a.poses = ws.add<RelocPose>(np);
            a.cand = ws.add<RelocCand>(total);
            a.kp_block = kp_block ? ws.add<uint8_t>(np * cap) : nullptr;
            rs = add_match_rows(out, np, cap, a.match, a.nmatches, &a.rot_hist, kRotBins);
        },
        [&](hipStream_t s) -> int {
            if (int e = h2d(a.frames, head.data(), head.size() * 4, s)) return e;
            if (int e = h2d(a.pts, pts ? pts + kf_offsets[0] : nullptr, total * sizeof(RelocPoint), s)) return e;
            if (int e = h2d(a.poses, poses, np * sizeof(RelocPose), s)) return e;
            return upload_rows(a.kp_block, cap, kp_block, kp_stride, std::min((size_t)kp_stride, cap), np, 0, s);
        },
        [&](hipStream_t s) { return launch_reloc(a, n_pairs, max_pts, s); });
}

int orbgpu_download_reloc_matches(orbgpu_ctx* c, int pair, int32_t* match, int cap, int* n_kp, int* nmatches,
                                  int32_t rot_hist[30]) {
    if (!c) return fail(ORBGPU_ERR_INVALID, "bad pair");
    return download_matches(c, c->res[S_RELOC], pair, "bad pair", match, cap, n_kp, nmatches, rot_hist);
}

// ---- ORBmatcher::Fuse(pKF, vpMapPoints, th) and its Sim3 overload on pinhole keyframes (orb_fuse.hip) ----
static_assert(sizeof(orbgpu_fuse_point) == 68 && sizeof(FusePoint) == 68, "orbgpu_fuse_point is 68 bytes");
static_assert(ORBGPU_FP_VALID == kFpValid && ORBGPU_FUSE_MAX_POINTS == kFuseMaxPoints, "the header states the kernel's constants");
static_assert(ORBGPU_FUSE_SKIPPED == kFuseSkipped && ORBGPU_FUSE_NEG_DEPTH == kFuseNegDepth &&
                  ORBGPU_FUSE_NOT_IN_IMAGE == kFuseNotInImage && ORBGPU_FUSE_DISTANCE == kFuseDistance &&
                  ORBGPU_FUSE_NORMAL == kFuseNormal && ORBGPU_FUSE_EMPTY_WINDOW == kFuseEmptyWindow &&
                  ORBGPU_FUSE_ABOVE_TH_LOW == kFuseAboveThLow && ORBGPU_FUSE_FUSED == kFuseFused,
              "the header states the decision codes");

int orbgpu_fuse_batch(orbgpu_ctx* c, int n_pairs, const int32_t* frames, const int32_t* lists, int n_lists,
                      const orbgpu_fuse_point* pts, const int32_t* list_offsets, const orbgpu_reloc_pose* poses,
                      const float K[4], const uint8_t* skip, int skip_stride, float th, float bf, int use_uright,
                      int sim3, void* stream) {
    if (!c) return fail(ORBGPU_ERR_INVALID, "null ctx");
    if (n_pairs < 0 || n_pairs > c->max_images) return fail(ORBGPU_ERR_INVALID, "bad pair count");
    if (!(th >= 0.0f) || !std::isfinite(th)) return fail(ORBGPU_ERR_INVALID, "th negative or not finite");
    const bool gate = sim3 == 0, stereo = gate && use_uright != 0;
    if (gate && (!(bf >= 0.0f) || !std::isfinite(bf))) return fail(ORBGPU_ERR_INVALID, "bf negative or not finite");
    ListPairs lp;
    if (int e = check_list_pairs(c, n_pairs, frames, lists, n_lists, pts, list_offsets, poses, K, skip, skip_stride, &lp,
                                 [&](int p) {
                                     if (stereo && ((frames[p] & 1) || frames[p] / 2 >= c->stereo_pairs))
                                         return fail(ORBGPU_ERR_INVALID, "mvuRight needs the left image of a pair of the last stereo_matches_batch");
                                     return 0;
                                 }))
        return e;
    SearchResult& res = c->res[S_FUSE];
    if (n_pairs == 0) return no_results(res);
    const size_t cap = (size_t)c->plan.out_cap, np = (size_t)n_pairs;
    HIP_TRY(hipSetDevice(c->device));
    FuseArgs a{};
    bind_frame(a, c);
    bind_grid(a, c);
    bind_scale(a, c);
    for (int l = 0; l < kMaxLevels; ++l) a.inv_sigma2[l] = l < c->prm.nlevels ? c->tab.inv_sigma2[l] : 1.0f;
    a.uright = stereo ? c->stur.as<float>() : nullptr;
    predict_scale_table(c->prm.scale_factor, c->prm.nlevels, a.level_step);  // MapPoint.cc:516-531
    for (int k = 0; k < 4; ++k) a.K[k] = K[k];
    a.th = th;
    a.bf = gate ? bf : 0.0f;
    a.sim3 = !gate;
    const int r = run_search(
        c, stream, res, "fuse", cover_of(np, frames, 1, false),
        [&](Layout& ws, Layout& out, ResultSlots& rs) {
            add_list_regions(ws, a, lp, np, skip != nullptr);
            int32_t* first;  // the keypoint side is a match row: the lowest point that fused onto each keypoint
            rs = add_match_rows(out, np, cap, first, a.nfused, nullptr, 0);
            a.first = reinterpret_cast<uint32_t*>(first);
            add_point_rows(out, rs, a, lp.rows);
        },
        [&](hipStream_t s) -> int {
            HIP_TRY(hipMemsetAsync(a.first, 0xFF, np * cap * 4, s));  // -1: no point fused onto the keypoint
            HIP_TRY(hipMemsetAsync(a.nfused, 0, np * 4, s));
            return upload_list_inputs(a, lp, np, pts ? pts + list_offsets[0] : nullptr, poses, skip, skip_stride, s);
        },
        [&](hipStream_t s) { return launch_fuse(a, n_pairs, lp.max_pts, s); });
    if (r == ORBGPU_OK) res.point_off.assign(lp.head.begin() + 2 * np, lp.head.begin() + 3 * np + 1);
    return r;
}

int orbgpu_download_fuse_matches(orbgpu_ctx* c, int pair, int32_t* best_idx, int32_t* best_dist, uint8_t* code,
                                 int cap_points, int32_t* first, int cap_kp, int* n_points, int* n_kp, int* nfused) {
    if (!c || pair < 0 || (size_t)pair >= c->res[S_FUSE].cover.image.size()) return fail(ORBGPU_ERR_INVALID, "bad pair");
    // the keypoint side first: both counts are out before either capacity is judged
    const int r = download_matches(c, c->res[S_FUSE], pair, "bad pair", first, cap_kp, n_kp, nfused, nullptr);
    return download_point_rows(c, c->res[S_FUSE], pair, r, best_idx, best_dist, code, cap_points, n_points);
}

// ---- ORBmatcher::SearchByProjection(pKF, Scw, vpPoints[, vpPointsKFs], vpMatched[, vpMatchedKF], th, ratioHamming)
// on pinhole keyframes (orb_sim3.hip) ----
static_assert(ORBGPU_SIM3_SKIPPED == kFuseSkipped && ORBGPU_SIM3_NEG_DEPTH == kFuseNegDepth &&
                  ORBGPU_SIM3_NOT_IN_IMAGE == kFuseNotInImage && ORBGPU_SIM3_DISTANCE == kFuseDistance &&
                  ORBGPU_SIM3_NORMAL == kFuseNormal && ORBGPU_SIM3_EMPTY_WINDOW == kFuseEmptyWindow &&
                  ORBGPU_SIM3_NOT_MATCHED == kSim3NotMatched && ORBGPU_SIM3_MATCHED == kSim3Matched &&
                  ORBGPU_SIM3_PROJECT_DIV == kSim3ProjectDiv && ORBGPU_SIM3_PROJECT_INVZ == kSim3ProjectInvz,
              "the header states the decision codes and the projection forms");

int orbgpu_sim3_search_by_projection_batch(orbgpu_ctx* c, int n_pairs, const int32_t* frames, const int32_t* lists,
                                           int n_lists, const orbgpu_fuse_point* pts, const int32_t* list_offsets,
                                           const orbgpu_reloc_pose* poses, const float K[4], const uint8_t* skip,
                                           int skip_stride, const uint8_t* kp_block, int kp_stride, float th,
                                           float ratio_hamming, int projection, void* stream) {
    if (!c) return fail(ORBGPU_ERR_INVALID, "null ctx");
    if (n_pairs < 0 || n_pairs > c->max_images) return fail(ORBGPU_ERR_INVALID, "bad pair count");
    if (!(th >= 0.0f) || !std::isfinite(th)) return fail(ORBGPU_ERR_INVALID, "th negative or not finite");
    const float limit = 50.0f * ratio_hamming;  // TH_LOW * ratioHamming (:524): int * float, a float
    if (!std::isfinite(ratio_hamming) || !(limit >= 0.0f && limit < 256.0f))
        return fail(ORBGPU_ERR_INVALID, "ratio_hamming not finite or 50 * ratio_hamming outside [0, 256) (256 would match keypoint -1)");
    if (projection != ORBGPU_SIM3_PROJECT_DIV && projection != ORBGPU_SIM3_PROJECT_INVZ)
        return fail(ORBGPU_ERR_INVALID, "projection is ORBGPU_SIM3_PROJECT_DIV or ORBGPU_SIM3_PROJECT_INVZ");
    // the context's own limit, whatever the batch holds: a pair count above 0 is enough to meet it
    if (n_pairs > 0 && sim3_resolve_lds_bytes(c->plan.out_cap) > 160 * 1024)
        return fail(ORBGPU_ERR_CAPACITY, "keypoint capacity above the matcher's LDS budget");
    ListPairs lp;
    if (int e = check_list_pairs(c, n_pairs, frames, lists, n_lists, pts, list_offsets, poses, K, skip, skip_stride, &lp,
                                 [](int) { return 0; }))
        return e;
    if (n_pairs > 0 && kp_block && kp_stride < 0) return fail(ORBGPU_ERR_INVALID, "negative kp_stride");
    SearchResult& res = c->res[S_SIM3];
    if (n_pairs == 0) return no_results(res);
    const size_t cap = (size_t)c->plan.out_cap, np = (size_t)n_pairs, rows = lp.rows;
    if (kp_block)  // one row of kp_stride flags per pair: it must cover the frame's keypoints
        if (int e = rows_cover_counts(c, c->grid_images, frames, 1, n_pairs, kp_stride,
                                      "kp_stride below the frame's keypoint count"))
            return e;
    HIP_TRY(hipSetDevice(c->device));
    Sim3Args a{};
    bind_frame(a, c);
    bind_grid(a, c);
    bind_scale(a, c);
    predict_scale_table(c->prm.scale_factor, c->prm.nlevels, a.level_step);  // MapPoint.cc:516-531
    for (int k = 0; k < 4; ++k) a.K[k] = K[k];
    a.th = th;
    a.limit = limit;
    a.projection = projection;
    const int r = run_search(
        c, stream, res, "Sim3 projection search", cover_of(np, frames, 1, false),
        [&](Layout& ws, Layout& out, ResultSlots& rs) {
            add_list_regions(ws, a, lp, np, skip != nullptr);
            a.kp_block = kp_block ? ws.add<uint8_t>(np * cap) : nullptr;
            a.cand = ws.add<RelocCand>(rows);
            a.order = ws.add<int32_t>(rows);  // the replay's own: no download reads it
            rs = add_match_rows(out, np, cap, a.match, a.nmatches, &a.stats, kSim3Stats);
            add_point_rows(out, rs, a, rows);
        },
        [&](hipStream_t s) -> int {
            if (int e = upload_list_inputs(a, lp, np, pts ? pts + list_offsets[0] : nullptr, poses, skip, skip_stride, s)) return e;
            return upload_rows(a.kp_block, cap, kp_block, kp_stride, std::min((size_t)kp_stride, cap), np, 0, s);
        },
        [&](hipStream_t s) { return launch_sim3(a, n_pairs, lp.max_pts, s); });
    if (r == ORBGPU_OK) res.point_off.assign(lp.head.begin() + 2 * np, lp.head.begin() + 3 * np + 1);
    return r;
}

int orbgpu_download_sim3_matches(orbgpu_ctx* c, int pair, int32_t* match, int cap_kp, int32_t* best_idx,
                                 int32_t* best_dist, uint8_t* code, int cap_points, int* n_kp, int* n_points,
                                 int* nmatches) {
    if (!c || pair < 0 || (size_t)pair >= c->res[S_SIM3].cover.image.size()) return fail(ORBGPU_ERR_INVALID, "bad pair");
    const int r = download_matches(c, c->res[S_SIM3], pair, "bad pair", match, cap_kp, n_kp, nmatches, nullptr);
    return download_point_rows(c, c->res[S_SIM3], pair, r, best_idx, best_dist, code, cap_points, n_points);
}

int orbgpu_sim3_replay_stats(orbgpu_ctx* c, int pair, int32_t stats[4]) {
    static_assert(kSim3Stats == 4, "the header states the count");
    if (!c || !stats || pair < 0 || (size_t)pair >= c->res[S_SIM3].cover.image.size()) return fail(ORBGPU_ERR_INVALID, "bad pair");
    if (int e_ = ctx_sync(c)) return e_;
    D2H(stats, c->res[S_SIM3].at.hist + (size_t)pair * kSim3Stats, 4 * kSim3Stats);
    return ORBGPU_OK;
}

}  // extern "C"
