// Host harness of the resize loops' work split (orb_kernels.h resize_run / resize_row_carried) and of
// the finished resize tables the planner writes for them (orb_geometry.h resize_level), for
// tests/test_resize_runs.py: pure host code, built as a shared library and read with ctypes.
#include <cstdint>
#include <cstring>
#include <string>

#include "../../orbslam3lib_amd/csrc/orb_geometry.h"

using namespace orbgpu;

namespace {
struct IntDiv {
    int operator()(int n, int d) const { return n / d; }
};
}  // namespace

extern "C" {

// out = {q, row0, row1} of thread t
void rr_resize_run(int t, int nq, int nrows, int nthreads, int32_t* out) {
    const ResizeRun r = resize_run(t, nq, nrows, nthreads, IntDiv{});
    out[0] = r.q;
    out[1] = r.row0;
    out[2] = r.row1;
}

int rr_row_carried(int prev_sy1, int sy0) { return resize_row_carried(prev_sy1, sy0) ? 1 : 0; }

constexpr int kLevelFields = 14;
const char* rr_level_fields() {
    return "w,h,area2,simd_end,tiles_x,tiles_y,xtab_off,ytab_off,band_row_off,tile_quad_off,qrec_off,qbase_off,"
           "yrec_off,tpitch";
}

// The plan of a w x h image: lv gets kLevelFields ints per level (rr_level_fields' order), sc =
// {tail0, generic_pyr, kBrMaxQuads, kBrMaxRows}, rtab up to rtab_cap int4 (*rtab_n: the plan's count).
int rr_plan(int w, int h, int nlevels, float scale_factor, int nfeatures, int32_t* lv, int32_t* sc, int32_t* rtab,
            int rtab_cap, int32_t* rtab_n) {
    const orbgpu_params prm{nfeatures, scale_factor, nlevels, 20, 7};
    GeomPlan P;
    std::string msg;
    const int r = plan_geometry(build_tables(prm), prm, w, h, 2, GeomKnobs{}, &P, &msg);
    if (r) return r;
    for (int l = 0; l < nlevels; ++l) {
        const LevelGeom& G = P.A.lv[l];
        const int v[kLevelFields] = {G.w, G.h, G.area2, G.simd_end, G.tiles_x, G.tiles_y, G.xtab_off, G.ytab_off,
                                     G.band_row_off, G.tile_quad_off, G.qrec_off, G.qbase_off, G.yrec_off, G.tpitch};
        std::memcpy(lv + l * kLevelFields, v, sizeof(v));
    }
    sc[0] = P.A.tail0;
    sc[1] = P.generic_pyr ? 1 : 0;
    sc[2] = kBrMaxQuads;
    sc[3] = kBrMaxRows;
    *rtab_n = (int32_t)P.rtab.size();
    if ((int)P.rtab.size() <= rtab_cap) std::memcpy(rtab, P.rtab.data(), sizeof(int4) * P.rtab.size());
    return 0;
}

}  // extern "C"
