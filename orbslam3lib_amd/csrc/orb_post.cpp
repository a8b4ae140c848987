// orb_post.cpp -- the part of the C ABI (include/orbgpu.h) that runs after a batch: matching,
// stereo, fisheye and grid over the device-resident results, SoA packing and export, and their
// downloads / getters.  The ORBmatcher searches are in orb_matchers.cpp; the context and the
// dispatch helpers are in orb_ctx.h.
#include <cstdio>
#include <cstdlib>

#include "orb_ctx.h"

using namespace orbgpu;

// MatchArgs over the context's last batch: pair p = images 2p (query) and 2p + 1 (train)
MatchArgs orbgpu::stereo_match_args(orbgpu_ctx* c, int stereo_only) {
    MatchArgs m;
    m.desc = c->outdesc.as<uint8_t>();
    m.out_n = c->outn.as<int32_t>();
    m.out_mono = c->outmono.as<int32_t>();
    m.out_cap = c->plan.out_cap;
    m.stereo_only = stereo_only;
    m.idx1 = c->midx1.as<int32_t>();
    m.dist1 = c->mdist1.as<int32_t>();
    m.idx2 = c->midx2.as<int32_t>();
    m.dist2 = c->mdist2.as<int32_t>();
    m.nq = c->mnq.as<int32_t>();
    m.part = nullptr;
    m.cnt = reinterpret_cast<uint32_t*>(c->mpart.as<uint8_t>() + (size_t)kKnnSplitSlots * c->plan.out_cap * 8 + 256);
    m.cnt_slots = (int)knn2_counter_slots(c->plan.out_cap);
    m.pair0 = 0;
    return m;
}

extern "C" {

int orbgpu_get_device(const orbgpu_ctx* c) { return c ? c->device : fail(ORBGPU_ERR_INVALID, "null ctx"); }

int orbgpu_get_scale_tables(const orbgpu_ctx* c, float* scale, float* inv_scale, float* sigma2,
                            float* inv_sigma2, int32_t* fpl) {
    if (!c) return fail(ORBGPU_ERR_INVALID, "null ctx");
    for (int l = 0; l < c->prm.nlevels; ++l) {
        if (scale) scale[l] = c->tab.scale[l];
        if (inv_scale) inv_scale[l] = c->tab.inv_scale[l];
        if (sigma2) sigma2[l] = c->tab.sigma2[l];
        if (inv_sigma2) inv_sigma2[l] = c->tab.inv_sigma2[l];
        if (fpl) fpl[l] = c->tab.nper[l];
    }
    return ORBGPU_OK;
}

int orbgpu_download_counts(orbgpu_ctx* c, int n, int32_t* nk, int32_t* nm) {
    if (!c) return fail(ORBGPU_ERR_INVALID, "null ctx");
    if (n > c->last_images) return fail(ORBGPU_ERR_INVALID, "more images than the last batch");
    HIP_TRY(hipStreamSynchronize(c->stream));
    if (int e_ = ctx_sync(c)) return e_;
    if (nk) D2H(nk, c->outn.p, (size_t)n * 4);
    if (nm) D2H(nm, c->outmono.p, (size_t)n * 4);
    return ORBGPU_OK;
}

int orbgpu_candidate_counts(orbgpu_ctx* c, int n, int32_t* counts) {
    if (!c || !counts) return fail(ORBGPU_ERR_INVALID, "null argument");
    if (n > c->last_images) return fail(ORBGPU_ERR_INVALID, "more images than the last batch");
    if (int e_ = ctx_sync(c)) return e_;  // (sets the device)
    std::vector<int32_t> cc((size_t)n * c->plan.cellcnt_img);
    if (!cc.empty())
        D2H(cc.data(), c->cellcnt.p, cc.size() * 4);
    const BatchArgs& A = c->plan.A;
    for (int i = 0; i < n; ++i) {
        long long s = 0;
        for (int l = 0; l < A.nlevels; ++l)
            for (int k = 0; k < A.lv[l].ncells; ++k) s += cc[(size_t)i * c->plan.cellcnt_img + A.lv[l].cellcnt_off + k];
        counts[i] = (int32_t)s;
    }
    return ORBGPU_OK;
}

int orbgpu_download_result(orbgpu_ctx* c, int img, orbgpu_keypoint* kps, uint8_t* desc, int cap,
                           int* n, int* n_mono) {
    if (!c || img < 0 || img >= c->last_images) return fail(ORBGPU_ERR_INVALID, "bad image index");
    if (int e_ = ctx_sync(c)) return e_;
    int32_t nk = 0, nm = 0;
    D2H(&nk, c->outn.as<int32_t>() + img, 4);
    D2H(&nm, c->outmono.as<int32_t>() + img, 4);
    if (int e = count_status(nk)) return e;
    if (n) *n = nk;
    if (n_mono) *n_mono = nm;
    if (nk > cap) return fail(ORBGPU_ERR_CAPACITY, "caller capacity too small");
    if (kps && nk)
        D2H(kps, c->outkps.as<orbgpu_keypoint>() + (size_t)img * c->plan.out_cap,
                          sizeof(orbgpu_keypoint) * nk);
    if (desc && nk)
        D2H(desc, c->outdesc.as<uint8_t>() + (size_t)img * c->plan.out_cap * 32, 32 * (size_t)nk);
    return ORBGPU_OK;
}

int orbgpu_get_pyramid_level(orbgpu_ctx* c, int img, int level, int blurred, uint8_t* dst,
                             int dst_stride, int* width, int* height) {
    if (!c || img < 0 || img >= c->last_images || level < 0 || level >= c->prm.nlevels)
        return fail(ORBGPU_ERR_INVALID, "bad image/level");
    if (int e_ = ctx_sync(c)) return e_;
    const LevelGeom& G = c->plan.A.lv[level];
    if (width) *width = G.w;
    if (height) *height = G.h;
    if (!dst) return ORBGPU_OK;
    if (dst_stride < G.w) return fail(ORBGPU_ERR_INVALID, "dst_stride < level width");
    const uint8_t* src;
    int pitch;
    if (blurred) {
        src = c->plan.A.blur_base[level] + (size_t)img * c->plan.blur_img;
        pitch = G.bpitch;
    } else if (level == 0) {
        src = cur_input(c) + (size_t)img * c->last_w * c->last_h;
        pitch = c->last_w;
    } else {
        src = c->plan.A.lvl_base[level] + (size_t)img * c->plan.pyr_img;
        pitch = G.pitch;
    }
    HIP_TRY(hipMemcpy2DAsync(dst, dst_stride, src, pitch, G.w, G.h, hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(hipStreamSynchronize(c->stream));
    return ORBGPU_OK;
}

int orbgpu_get_level_keypoints(orbgpu_ctx* c, int img, orbgpu_keypoint* kps, uint8_t* desc, int cap,
                               int32_t* counts) {
    if (!c || img < 0 || img >= c->last_images) return fail(ORBGPU_ERR_INVALID, "bad image index");
    if (int e_ = ctx_sync(c)) return e_;
    const int L = c->prm.nlevels;
    std::vector<int32_t> cnt(kMaxLevels), st(kMaxLevels);
    D2H(cnt.data(), c->lvlcnt.as<int32_t>() + img * kMaxLevels, 4 * kMaxLevels);
    D2H(st.data(), c->status.as<int32_t>() + img * kMaxLevels, 4 * kMaxLevels);
    int off = 0;
    for (int l = 0; l < L; ++l) {
        if (st[l]) return fail(ORBGPU_ERR_OVERFLOW, "octree status " + std::to_string(st[l]));
        const LevelGeom& G = c->plan.A.lv[l];
        const int m = cnt[l];
        counts[l] = m;
        if (off + m > cap) return fail(ORBGPU_ERR_CAPACITY, "caller capacity too small");
        std::vector<uint32_t> keys(m);
        std::vector<float> ang(m);
        const size_t base = (size_t)img * c->plan.lvlkp_img + G.kp_off;
        if (m) {
            D2H(keys.data(), c->lvlkey.as<uint32_t>() + base, 4 * m);
            if (c->last_fused) {  // k_orient_desc wrote the assembled rows (all mono, level order) only
                const size_t row = (size_t)img * c->plan.out_cap + off;
                std::vector<orbgpu_keypoint> ok(m);
                D2H(ok.data(), c->outkps.as<orbgpu_keypoint>() + row, sizeof(orbgpu_keypoint) * m);
                for (int i = 0; i < m; ++i) ang[i] = ok[i].angle;
                if (desc) D2H(desc + 32 * (size_t)off, c->outdesc.as<uint8_t>() + row * 32, 32 * (size_t)m);
            } else {
                D2H(ang.data(), c->lvlangle.as<float>() + base, 4 * m);
                if (desc)
                    D2H(desc + 32 * (size_t)off, c->lvldesc.as<uint8_t>() + base * 32, 32 * (size_t)m);
            }
        }
        for (int i = 0; i < m; ++i) {
            orbgpu_keypoint& k = kps[off + i];
            k.x = (float)((keys[i] & 0xFFF) + kMinBorder);
            k.y = (float)(((keys[i] >> 12) & 0xFFF) + kMinBorder);
            k.size = (float)G.patch;
            k.angle = ang[i];
            k.response = (float)(keys[i] >> 24);
            k.octave = l;
            k.class_id = -1;
        }
        off += m;
    }
    return ORBGPU_OK;
}

int orbgpu_match_knn2(orbgpu_ctx* c, const uint8_t* q, int nq, const uint8_t* t, int nt,
                      int32_t* i1, int32_t* d1, int32_t* i2, int32_t* d2) {
    if (!c || nq < 0 || nt < 0 || (nq && !q) || (nt && !t)) return fail(ORBGPU_ERR_INVALID, "bad args");
    if (nt > 65535) return fail(ORBGPU_ERR_INVALID, "train set larger than 65535 rows");
    if (nq == 0) return ORBGPU_OK;
    HIP_TRY(hipSetDevice(c->device));
    const size_t need = 32 * (size_t)(nq + nt) + 16 * (size_t)nq + 1024;
    if (c->scratch.ensure(need)) return fail(ORBGPU_ERR_HIP, "hipMalloc failed (match scratch)");
    uint8_t* dq = c->scratch.as<uint8_t>();
    uint8_t* dt = dq + 32 * (size_t)nq;
    int32_t* o = reinterpret_cast<int32_t*>(dt + 32 * (size_t)nt + 256 - ((32 * (size_t)(nq + nt)) & 255));
    HIP_TRY(hipMemcpyAsync(dq, q, 32 * (size_t)nq, hipMemcpyHostToDevice, c->stream));
    if (nt) HIP_TRY(hipMemcpyAsync(dt, t, 32 * (size_t)nt, hipMemcpyHostToDevice, c->stream));
    int r = timed(c, ST_KNN, c->stream, [&] {
        return launch_knn2_plain(dq, nq, dt, nt, o, o + nq, o + 2 * nq, o + 3 * nq, c->stream);
    });
    if (r) return r;
    std::vector<int32_t> h(4 * (size_t)nq);
    HIP_TRY(hipMemcpyAsync(h.data(), o, 16 * (size_t)nq, hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(hipStreamSynchronize(c->stream));
    for (int i = 0; i < nq; ++i) {
        if (i1) i1[i] = h[i];
        if (d1) d1[i] = h[nq + i];
        if (i2) i2[i] = h[2 * nq + i];
        if (d2) d2[i] = h[3 * nq + i];
    }
    return ORBGPU_OK;
}

int orbgpu_export_descriptors(orbgpu_ctx* c, int img, int row0, uint8_t* dst, int cap, int* n_rows, void* stream) {
    if (!c || img < 0 || img >= c->last_images || row0 < 0 || (cap > 0 && !dst))
        return fail(ORBGPU_ERR_INVALID, "bad arguments");
    HIP_TRY(hipSetDevice(c->device));
    if (cap > 0 && !device_ptr(dst)) return fail(ORBGPU_ERR_INVALID, "device_dst is not device memory");
    hipStream_t s = stream ? (hipStream_t)stream : c->stream;
    int r = join_all(c, s);  // the descriptors come from the chunk streams
    if (r) return r;
    int32_t nk = 0;  // the count decides the copy size: read it once the batch is done
    HIP_TRY(hipMemcpyAsync(&nk, c->outn.as<int32_t>() + img, 4, hipMemcpyDeviceToHost, s));
    HIP_TRY(hipStreamSynchronize(s));
    if (int e = count_status(nk)) return e;
    const int n = nk > row0 ? nk - row0 : 0;
    if (n_rows) *n_rows = n;
    if (n > cap) return fail(ORBGPU_ERR_CAPACITY, "caller capacity too small");
    if (n)
        HIP_TRY(hipMemcpyAsync(dst, c->outdesc.as<uint8_t>() + ((size_t)img * c->plan.out_cap + row0) * 32, 32 * (size_t)n,
                               hipMemcpyDeviceToDevice, s));
    return rejoin(c, s);
}

// the packed layout's largest size (every image at the context's row capacity): no device access
size_t orbgpu_export_batch_bytes(const orbgpu_ctx* c, int n_images, int n_pairs) {
    if (!c || n_images < 0 || n_pairs < 0) return 0;
    const size_t cap = (size_t)c->plan.out_cap;
    return 8 * (size_t)n_images + 4 * (size_t)n_pairs + cap * (sizeof(orbgpu_keypoint) + 32) * (size_t)n_images +
           16 * cap * (size_t)n_pairs;
}

int orbgpu_export_batch(orbgpu_ctx* c, int n_images, int n_pairs, void* device_dst, size_t dst_bytes,
                        size_t* used, void* stream) {
    if (!c || n_images < 0 || n_images > c->last_images || n_pairs < 0 || n_pairs > c->last_pairs ||
        2 * n_pairs > n_images)
        return fail(ORBGPU_ERR_INVALID, "bad image / pair count");
    if (used) *used = 0;
    if (n_images == 0) return ORBGPU_OK;
    HIP_TRY(hipSetDevice(c->device));
    if (device_dst && !device_ptr(device_dst)) return fail(ORBGPU_ERR_INVALID, "device_dst is not device memory");
    hipStream_t s = stream ? (hipStream_t)stream : c->stream;
    int r = join_all(c, s);  // the outputs come from the chunk streams
    if (r) return r;
    // the produced rows size the layout: read the counts once the batch (and its match) is done
    std::vector<int32_t> cnt((size_t)n_images + n_pairs);
    HIP_TRY(hipMemcpyAsync(cnt.data(), c->outn.p, 4 * (size_t)n_images, hipMemcpyDeviceToHost, s));
    if (n_pairs) HIP_TRY(hipMemcpyAsync(cnt.data() + n_images, c->mnq.p, 4 * (size_t)n_pairs, hipMemcpyDeviceToHost, s));
    HIP_TRY(hipStreamSynchronize(s));
    size_t need = 4 * (2 * (size_t)n_images + n_pairs);
    for (int i = 0; i < n_images; ++i) {
        if (int e = count_status(cnt[i])) return e;  // -5 / -2 status words are not row counts
        need += (sizeof(orbgpu_keypoint) + 32) * (size_t)cnt[i];
    }
    for (int p = 0; p < n_pairs; ++p) need += 16 * (size_t)std::max(cnt[n_images + p], 0);
    if (used) *used = need;
    if (!device_dst) return rejoin(c, s);  // size query
    if (dst_bytes < need) return fail(ORBGPU_ERR_CAPACITY, "export buffer too small");
    if (reinterpret_cast<uintptr_t>(device_dst) % 4) return fail(ORBGPU_ERR_INVALID, "device_dst not 4-byte aligned");
    ExportArgs x;
    x.kps = c->outkps.p;
    x.desc = c->outdesc.as<uint8_t>();
    x.out_n = c->outn.as<int32_t>();
    x.out_mono = c->outmono.as<int32_t>();
    x.nq = c->mnq.as<int32_t>();
    x.idx1 = c->midx1.as<int32_t>();
    x.dist1 = c->mdist1.as<int32_t>();
    x.idx2 = c->midx2.as<int32_t>();
    x.dist2 = c->mdist2.as<int32_t>();
    x.out_cap = c->plan.out_cap;
    x.nimages = n_images;
    x.npairs = n_pairs;
    x.dst = device_dst;
    HIP_TRY(launch_pack_export(x, s));
    return rejoin(c, s);
}

int orbgpu_match_knn2_device(orbgpu_ctx* c, const uint8_t* q, int nq, const uint8_t* t, int nt, int32_t* i1,
                             int32_t* d1, int32_t* i2, int32_t* d2, void* stream) {
    if (!c || nq < 0 || nt < 0 || (nq && (!q || !i1 || !d1 || !i2 || !d2)) || (nt && !t))
        return fail(ORBGPU_ERR_INVALID, "bad args");
    if (nt > 65535) return fail(ORBGPU_ERR_INVALID, "train set larger than 65535 rows");
    if (nq == 0) return ORBGPU_OK;
    HIP_TRY(hipSetDevice(c->device));
    for (const void* p : {(const void*)q, (const void*)i1, (const void*)d1, (const void*)i2, (const void*)d2})
        if (!device_ptr(p)) return fail(ORBGPU_ERR_INVALID, "query / outputs must be device memory");
    if (nt && !device_ptr(t)) return fail(ORBGPU_ERR_INVALID, "train must be device memory");
    hipStream_t s = stream ? (hipStream_t)stream : c->stream;
    int r = timed(c, ST_KNN, s, [&] { return launch_knn2_plain(q, nq, t, nt, i1, d1, i2, d2, s); });
    if (r) return r;
    return rejoin(c, s);
}

int orbgpu_match_stereo_batch(orbgpu_ctx* c, int n_pairs, int stereo_only, void* stream) {
    if (!c || n_pairs < 1 || 2 * n_pairs > c->last_images) return fail(ORBGPU_ERR_INVALID, "bad pair count");
    HIP_TRY(hipSetDevice(c->device));
    if (c->plan.out_cap > 65535) return fail(ORBGPU_ERR_INVALID, "matcher supports < 65536 rows per image");
    const MatchArgs m = stereo_match_args(c, stereo_only);
    // the split path (<= 4 pairs) writes its partial lists to one buffer: only a call that is a
    // single launch may use it (the slots are then its own)
    uint2* split_part = n_pairs * 2 <= kKnnSplitSlots && !c->knobs.knn_nosplit ? c->mpart.as<uint2>() : nullptr;
    // follow the extraction's sub-batches so each chunk matches right after it is extracted
    int r = after_batch(c, stream, n_pairs, 2, ST_KNN, [&](int p0, int np, hipStream_t st, bool single) {
        MatchArgs mm = m;
        mm.pair0 = p0;
        mm.part = single ? split_part : nullptr;
        return timed(c, ST_KNN, st, [&] { return launch_knn2_pairs(mm, np, st); });
    });
    if (r) return r;
    c->last_pairs = n_pairs;
    return ORBGPU_OK;
}

int orbgpu_download_matches(orbgpu_ctx* c, int pair, int32_t* i1, int32_t* d1, int32_t* i2,
                            int32_t* d2, int cap, int* nq) {
    if (!c || pair < 0 || pair >= c->last_pairs) return fail(ORBGPU_ERR_INVALID, "bad pair");
    if (int e_ = ctx_sync(c)) return e_;
    int32_t n = 0;
    D2H(&n, c->mnq.as<int32_t>() + pair, 4);
    if (nq) *nq = n;
    if (n > cap) return fail(ORBGPU_ERR_CAPACITY, "caller capacity too small");
    const size_t o = (size_t)pair * c->plan.out_cap;
    if (n) {
        if (i1) D2H(i1, c->midx1.as<int32_t>() + o, 4 * (size_t)n);
        if (d1) D2H(d1, c->mdist1.as<int32_t>() + o, 4 * (size_t)n);
        if (i2) D2H(i2, c->midx2.as<int32_t>() + o, 4 * (size_t)n);
        if (d2) D2H(d2, c->mdist2.as<int32_t>() + o, 4 * (size_t)n);
    }
    return ORBGPU_OK;
}

int orbgpu_stereo_matches_batch(orbgpu_ctx* c, int n_pairs, float mbf, float mb, void* stream) {
    if (!c || n_pairs < 1 || 2 * n_pairs > c->last_images) return fail(ORBGPU_ERR_INVALID, "bad pair count");
    if (!(mb > 0.f) || !(mbf > 0.f)) return fail(ORBGPU_ERR_INVALID, "mbf and mb must be positive");
    HIP_TRY(hipSetDevice(c->device));
    const BatchArgs& A = c->plan.A;
    const int H0 = A.lv[0].h;
    const size_t np = (size_t)n_pairs;
    if (c->strow.ensure(np * (H0 + 1) * 4 + 256) || c->stidx.ensure(np * c->plan.out_cap * 4 + 256) ||
        c->stur.ensure(np * c->plan.out_cap * 4 + 256) || c->stdepth.ensure(np * c->plan.out_cap * 4 + 256) ||
        c->stsad.ensure(np * c->plan.out_cap * 4 + 256))
        return fail(ORBGPU_ERR_HIP, "hipMalloc failed (stereo buffers)");
    StereoArgs S{};
    S.kps = c->outkps.p;
    S.desc = c->outdesc.as<uint8_t>();
    S.out_n = c->outn.as<int32_t>();
    S.out_cap = c->plan.out_cap;
    S.nlevels = A.nlevels;
    S.H0 = H0;
    for (int l = 0; l < A.nlevels; ++l) {
        S.lvl_base[l] = l == 0 ? cur_input(c) : A.lvl_base[l];
        S.limg_stride[l] = l == 0 ? (long long)A.lv[0].w * A.lv[0].h : A.lv[l].img_stride;
        S.lw[l] = A.lv[l].w;
        S.lh[l] = A.lv[l].h;
        S.lpitch[l] = l == 0 ? A.lv[0].w : A.lv[l].pitch;
        S.scale[l] = c->tab.scale[l];
        S.inv_scale[l] = c->tab.inv_scale[l];
    }
    S.mbf = mbf;
    S.mb = mb;
    S.row_start = c->strow.as<int32_t>();
    S.row_idx = c->stidx.as<int32_t>();
    S.u_right = c->stur.as<float>();
    S.depth = c->stdepth.as<float>();
    S.sad = c->stsad.as<int32_t>();
    // follow the extraction's sub-batches (each chunk's pairs right after their extraction)
    int r = after_batch(c, stream, n_pairs, 2, -1, [&](int p0, int npp, hipStream_t st, bool) {
        StereoArgs SS = S;
        SS.pair0 = p0;
        return timed(c, ST_STEREO, st, [&] { return launch_stereo(SS, npp, st); });
    });
    if (r) return r;
    c->stereo_pairs = n_pairs;
    return ORBGPU_OK;
}

int orbgpu_download_stereo(orbgpu_ctx* c, int pair, float* u_right, float* depth, int32_t* sad, int cap,
                           int* n) {
    if (!c || pair < 0 || pair >= c->stereo_pairs) return fail(ORBGPU_ERR_INVALID, "bad pair");
    if (int e_ = ctx_sync(c)) return e_;  // (sets the device)
    int32_t nl = 0;
    D2H(&nl, c->outn.as<int32_t>() + 2 * pair, 4);
    if (int e = count_status(nl)) return e;
    if (n) *n = nl;
    if (nl > cap) return fail(ORBGPU_ERR_CAPACITY, "caller capacity too small");
    const size_t o = (size_t)pair * c->plan.out_cap;
    if (nl) {
        if (u_right) D2H(u_right, c->stur.as<float>() + o, 4 * (size_t)nl);
        if (depth) D2H(depth, c->stdepth.as<float>() + o, 4 * (size_t)nl);
        if (sad) D2H(sad, c->stsad.as<int32_t>() + o, 4 * (size_t)nl);
    }
    return ORBGPU_OK;
}

// ---- Frame::ComputeStereoFishEyeMatches (orb_fisheye.hip) -------------------------------------
int orbgpu_fisheye_stereo_batch(orbgpu_ctx* c, int n_pairs, const orbgpu_kb8_rig* rig, void* stream) {
    if (!c || !rig || n_pairs < 1 || 2 * n_pairs > c->last_images) return fail(ORBGPU_ERR_INVALID, "bad pair count");
    for (int k = 0; k < 2; ++k)
        if (!(rig->cam_left[k] != 0.f) || !(rig->cam_right[k] != 0.f))
            return fail(ORBGPU_ERR_INVALID, "zero focal length");
    // BFMatchORB of the stereo rows (Frame.cc:1164), then the triangulation on the same streams
    if (int r = orbgpu_match_stereo_batch(c, n_pairs, 1, stream)) return r;
    HIP_TRY(hipSetDevice(c->device));
    const size_t np = (size_t)n_pairs, oc = (size_t)c->plan.out_cap;
    if (c->fel2r.ensure(np * oc * 4 + 256) || c->fer2l.ensure(np * oc * 4 + 256) ||
        c->fedepth.ensure(np * oc * 4 + 256) || c->fep3d.ensure(np * oc * 12 + 256) || c->fecnt.ensure(np * 8 + 256))
        return fail(ORBGPU_ERR_HIP, "hipMalloc failed (fisheye buffers)");
    FisheyeArgs F{};
    F.kps = c->outkps.p;
    F.out_n = c->outn.as<int32_t>();
    F.out_mono = c->outmono.as<int32_t>();
    F.out_cap = c->plan.out_cap;
    F.idx1 = c->midx1.as<int32_t>();
    F.dist1 = c->mdist1.as<int32_t>();
    for (int k = 0; k < 8; ++k) {
        F.cam_l[k] = rig->cam_left[k];
        F.cam_r[k] = rig->cam_right[k];
    }
    F.prec_l = rig->precision_left;
    F.prec_r = rig->precision_right;
    for (int k = 0; k < 9; ++k) F.R12[k] = rig->R12[k];
    for (int k = 0; k < 3; ++k) F.t12[k] = rig->t12[k];
    for (int l = 0; l < kMaxLevels; ++l) F.sigma2[l] = l < c->plan.A.nlevels ? c->tab.sigma2[l] : 0.f;
    F.l2r = c->fel2r.as<int32_t>();
    F.r2l = c->fer2l.as<int32_t>();
    F.depth = c->fedepth.as<float>();
    F.p3d = c->fep3d.as<float>();
    F.counts = c->fecnt.as<int32_t>();
    int r = after_batch(c, stream, n_pairs, 2, -1, [&](int p0, int npp, hipStream_t st, bool) -> int {
        HIP_TRY(hipMemsetAsync(F.r2l + (size_t)p0 * oc, 0xFF, (size_t)npp * oc * 4, st));  // -1
        HIP_TRY(hipMemsetAsync(F.counts + 2 * (size_t)p0, 0, (size_t)npp * 8, st));
        FisheyeArgs FF = F;
        FF.pair0 = p0;
        return timed(c, ST_FISHEYE, st, [&] { return launch_fisheye(FF, npp, st); });
    });
    if (r) return r;
    c->fisheye_pairs = n_pairs;
    return ORBGPU_OK;
}

int orbgpu_download_fisheye(orbgpu_ctx* c, int pair, int32_t* l2r, int32_t* r2l, float* depth, float* p3d, int cap,
                            int* n_left, int* n_right, int* n_matches) {
    if (!c || pair < 0 || pair >= c->fisheye_pairs) return fail(ORBGPU_ERR_INVALID, "bad pair");
    if (int e_ = ctx_sync(c)) return e_;  // (sets the device)
    int32_t n[2] = {0, 0}, cnt[2] = {0, 0};
    D2H(n, c->outn.as<int32_t>() + 2 * pair, 8);
    D2H(cnt, c->fecnt.as<int32_t>() + 2 * pair, 8);
    if (int e = count_status(n[0])) return e;
    if (int e = count_status(n[1])) return e;
    if (n_left) *n_left = n[0];
    if (n_right) *n_right = n[1];
    if (n_matches) *n_matches = cnt[0];
    if (n[0] > cap || n[1] > cap) return fail(ORBGPU_ERR_CAPACITY, "caller capacity too small");
    const size_t o = (size_t)pair * c->plan.out_cap;
    if (n[0]) {
        if (l2r) D2H(l2r, c->fel2r.as<int32_t>() + o, 4 * (size_t)n[0]);
        if (depth) D2H(depth, c->fedepth.as<float>() + o, 4 * (size_t)n[0]);
        if (p3d) D2H(p3d, c->fep3d.as<float>() + 3 * o, 12 * (size_t)n[0]);
    }
    if (n[1] && r2l) D2H(r2l, c->fer2l.as<int32_t>() + o, 4 * (size_t)n[1]);
    return ORBGPU_OK;
}

int orbgpu_pack_soa(orbgpu_ctx* c, int n_images, int n_pairs, void* stream) {
    if (!c || n_images < 0 || n_images > c->last_images || n_pairs < 0 || n_pairs > c->last_pairs)
        return fail(ORBGPU_ERR_INVALID, "bad image/pair count");
    HIP_TRY(hipSetDevice(c->device));
    const size_t cap = (size_t)c->plan.out_cap;
    if (c->soa.ensure((size_t)c->max_images * cap * 16 + 256) ||
        c->m16.ensure((size_t)(c->max_images / 2 + 1) * cap * 6 + 256))
        return fail(ORBGPU_ERR_HIP, "hipMalloc failed (soa buffers)");
    const size_t plane = (size_t)c->max_images * cap;
    const size_t mplane = (size_t)(c->max_images / 2 + 1) * cap;
    SoaArgs a{};
    a.kps = c->outkps.p;
    a.out_n = c->outn.as<int32_t>();
    a.out_cap = c->plan.out_cap;
    a.nimages = n_images;
    a.img0 = 0;
    a.x = c->soa.as<int32_t>();
    a.y = a.x + plane;
    a.angle = a.y + plane;
    a.level = a.angle + plane;
    a.nq = c->mnq.as<int32_t>();
    a.idx1 = c->midx1.as<int32_t>();
    a.dist1 = c->mdist1.as<int32_t>();
    a.dist2 = c->mdist2.as<int32_t>();
    a.idx16 = c->m16.as<int16_t>();
    a.d1_16 = a.idx16 + mplane;
    a.d2_16 = a.d1_16 + mplane;
    hipStream_t s = stream ? (hipStream_t)stream : c->stream;
    int r = join_all(c, s);  // the chunk streams produced the keypoints and matches
    if (r) return r;
    r = timed(c, ST_SOA, s, [&] { return launch_pack_soa(a, n_pairs, s); });
    if (r) return r;
    c->soa_images = n_images;
    c->soa_pairs = n_pairs;
    c->need_fork = true;  // the next batch's chunk streams must not overwrite what this reads
    return ORBGPU_OK;
}

int orbgpu_download_soa(orbgpu_ctx* c, int image, int32_t* x, int32_t* y, int32_t* angle, int32_t* level,
                        uint8_t* orb, int cap, int* count, int* mono) {
    if (!c || image < 0 || image >= c->soa_images) return fail(ORBGPU_ERR_INVALID, "bad image");
    if (int e_ = ctx_sync(c)) return e_;  // (sets the device)
    int32_t nm[2] = {0, 0};
    D2H(&nm[0], c->outn.as<int32_t>() + image, 4);
    D2H(&nm[1], c->outmono.as<int32_t>() + image, 4);
    if (int e = count_status(nm[0])) return e;
    if (count) *count = nm[0];
    if (mono) *mono = nm[1];
    if (nm[0] > cap) return fail(ORBGPU_ERR_CAPACITY, "caller capacity too small");
    const size_t n = (size_t)nm[0];
    if (!n) return ORBGPU_OK;
    const size_t plane = (size_t)c->max_images * c->plan.out_cap, o = (size_t)image * c->plan.out_cap;
    int32_t* dst[4] = {x, y, angle, level};
    for (int k = 0; k < 4; ++k)
        if (dst[k]) D2H(dst[k], c->soa.as<int32_t>() + k * plane + o, 4 * n);
    if (orb) D2H(orb, c->outdesc.as<uint8_t>() + o * 32, 32 * n);
    return ORBGPU_OK;
}

int orbgpu_download_matches16(orbgpu_ctx* c, int pair, int16_t* indices, int16_t* dist1, int16_t* dist2,
                              int cap, int* nq) {
    if (!c || pair < 0 || pair >= c->soa_pairs) return fail(ORBGPU_ERR_INVALID, "bad pair");
    if (int e_ = ctx_sync(c)) return e_;  // (sets the device)
    int32_t n = 0;
    D2H(&n, c->mnq.as<int32_t>() + pair, 4);
    if (nq) *nq = n;
    if (n > cap) return fail(ORBGPU_ERR_CAPACITY, "caller capacity too small");
    if (!n) return ORBGPU_OK;
    const size_t mplane = (size_t)(c->max_images / 2 + 1) * c->plan.out_cap, o = (size_t)pair * c->plan.out_cap;
    int16_t* dst[3] = {indices, dist1, dist2};
    for (int k = 0; k < 3; ++k)
        if (dst[k]) D2H(dst[k], c->m16.as<int16_t>() + k * mplane + o, 2 * (size_t)n);
    return ORBGPU_OK;
}

int orbgpu_image_bounds(int cols, int rows, const float K[4], const float* dist, int ndist, float bounds[4]) {
    if (!K || !bounds || (ndist > 0 && !dist) || ndist < 0) return fail(ORBGPU_ERR_INVALID, "null argument");
    image_bounds_host(cols, rows, K, dist, ndist, bounds);
    return ORBGPU_OK;
}

int orbgpu_undistort_grid_batch(orbgpu_ctx* c, int n, const float K[4], const float* dist, int ndist,
                                void* stream) {
    if (!c || !K || (ndist > 0 && !dist) || ndist < 0) return fail(ORBGPU_ERR_INVALID, "null argument");
    if (n < 1 || n > c->last_images) return fail(ORBGPU_ERR_INVALID, "bad image count");
    if (!(K[0] != 0.f) || !(K[1] != 0.f)) return fail(ORBGPU_ERR_INVALID, "fx and fy must be nonzero");
    HIP_TRY(hipSetDevice(c->device));
    const size_t ni = (size_t)n, cap = (size_t)c->plan.out_cap;
    if (c->gxy.ensure(ni * cap * 8 + 256) || c->gcell.ensure(ni * cap * 4 + 256) ||
        c->gstart.ensure(ni * (kGridCols * kGridRows + 1) * 4 + 256) || c->gidx.ensure(ni * cap * 4 + 256))
        return fail(ORBGPU_ERR_HIP, "hipMalloc failed (grid buffers)");
    GridArgs g{};
    g.kps = c->outkps.p;
    g.out_n = c->outn.as<int32_t>();
    g.out_cap = c->plan.out_cap;
    g.undistort = ndist > 0 && dist[0] != 0.0f;
    for (int i = 0; i < 4; ++i) g.K[i] = K[i];
    grid_dist_table(dist, ndist, g.k);
    image_bounds_host(c->plan.A.lv[0].w, c->plan.A.lv[0].h, K, dist, ndist, g.bounds);
    g.grid_inv[0] = static_cast<float>(kGridCols) / (g.bounds[1] - g.bounds[0]);  // Frame.cc:107-108
    g.grid_inv[1] = static_cast<float>(kGridRows) / (g.bounds[3] - g.bounds[2]);
    g.xy_un = c->gxy.as<float>();
    g.cell = c->gcell.as<int32_t>();
    g.cell_start = c->gstart.as<int32_t>();
    g.cell_idx = c->gidx.as<int32_t>();
    int r = after_batch(c, stream, n, 1, -1, [&](int img0, int nn, hipStream_t st, bool) {
        GridArgs gg = g;
        gg.img0 = img0;
        return timed(c, ST_GRID, st, [&] { return launch_undistort_grid(gg, nn, st); });
    });
    if (r) return r;
    c->grid_images = n;
    std::memcpy(c->grid_bounds, g.bounds, sizeof g.bounds);
    std::memcpy(c->grid_inv, g.grid_inv, sizeof g.grid_inv);
    return ORBGPU_OK;
}

int orbgpu_download_grid(orbgpu_ctx* c, int image, float* xy_un, int32_t* cell, int32_t* cell_start,
                         int32_t* cell_idx, int cap, int* n) {
    if (!c || image < 0 || image >= c->grid_images) return fail(ORBGPU_ERR_INVALID, "bad image");
    if (int e_ = ctx_sync(c)) return e_;  // (sets the device)
    int32_t nk = 0;
    D2H(&nk, c->outn.as<int32_t>() + image, 4);
    nk = std::max(nk, 0);
    if (n) *n = nk;
    if (nk > cap) return fail(ORBGPU_ERR_CAPACITY, "caller capacity too small");
    const size_t o = (size_t)image * c->plan.out_cap;
    const size_t G = kGridCols * kGridRows + 1;
    if (xy_un && nk) D2H(xy_un, c->gxy.as<float>() + 2 * o, 8 * (size_t)nk);
    if (cell && nk) D2H(cell, c->gcell.as<int32_t>() + o, 4 * (size_t)nk);
    if (cell_start) D2H(cell_start, c->gstart.as<int32_t>() + (size_t)image * G, 4 * G);
    if (cell_idx && nk) D2H(cell_idx, c->gidx.as<int32_t>() + o, 4 * (size_t)nk);
    return ORBGPU_OK;
}

int orbgpu_descriptor_distance(const uint8_t* a, const uint8_t* b) {
    int dist = 0;
    for (int i = 0; i < 8; ++i) {
        uint32_t pa, pb;
        std::memcpy(&pa, a + 4 * i, 4);
        std::memcpy(&pb, b + 4 * i, 4);
        dist += __builtin_popcount(pa ^ pb);
    }
    return dist;
}

}  // extern "C"
