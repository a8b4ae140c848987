// selftest.cpp -- TEST INFRASTRUCTURE ONLY.
//
// One 160x120 extraction and three DistributeOctTree cases through the reference's code, folded
// into one FNV-1a digest.  Built twice from the same sources: into libref_extractor.so (the
// function alone, REF_SELFTEST_NO_MAIN) and, with -fsanitize=address, into the stand-alone
// ref_selftest program, which prints the digest.  Equal digests and a clean sanitizer exit show
// that the stand-in Mat hides no out-of-bounds access of the reference's patch sampling.
#include <cstdint>
#include <cstdio>
#include <vector>

#include "orb_oracle.h"

extern "C" {
int ref_extract(int nfeatures, float scale_factor, int nlevels, int ini_th, int min_th, const uint8_t* img, int w,
                int h, int stride, int lap0, int lap1, oracle_kp* kps, uint8_t* desc, int cap, int* n_out);
int ref_distribute_octree(const oracle_kp* keys, int n, int minX, int maxX, int minY, int maxY, int N, oracle_kp* out,
                          int cap);
uint64_t ref_selftest_digest(int* n_keypoints);
}

namespace {

struct Rng {  // xorshift64*
    uint64_t s;
    uint32_t next() {
        s ^= s >> 12, s ^= s << 25, s ^= s >> 27;
        return (uint32_t)((s * 0x2545F4914F6CDD1DULL) >> 32);
    }
};

void fold(uint64_t& d, const void* p, size_t n) {
    const uint8_t* b = (const uint8_t*)p;
    for (size_t i = 0; i < n; ++i) d = (d ^ b[i]) * 0x100000001B3ULL;
}

void fold_kps(uint64_t& d, const oracle_kp* k, int n) {
    fold(d, &n, sizeof n);
    for (int i = 0; i < n; ++i) {  // field by field: no padding, no uninitialised bytes
        fold(d, &k[i].x, 4), fold(d, &k[i].y, 4), fold(d, &k[i].size, 4), fold(d, &k[i].angle, 4);
        fold(d, &k[i].response, 4), fold(d, &k[i].octave, 4), fold(d, &k[i].class_id, 4);
    }
}

}  // namespace

uint64_t ref_selftest_digest(int* n_keypoints) {
    uint64_t d = 0xCBF29CE484222325ULL;
    Rng rng{0x9E3779B97F4A7C15ULL};
    // 8x8 blocks of random grey plus +-8 of pixel noise: corners on every level
    const int W = 160, H = 120;
    std::vector<uint8_t> img((size_t)W * H);
    std::vector<int> block((W / 8) * (H / 8));
    for (int& b : block) b = 16 + (int)(rng.next() % 224);
    for (int y = 0; y < H; ++y)
        for (int x = 0; x < W; ++x) {
            int v = block[(y / 8) * (W / 8) + x / 8] + (int)(rng.next() % 17) - 8;
            img[(size_t)y * W + x] = (uint8_t)(v < 0 ? 0 : v > 255 ? 255 : v);
        }
    const int cap = 4096;
    std::vector<oracle_kp> kps(cap);
    std::vector<uint8_t> desc((size_t)cap * 32);
    int n = 0;
    int mono = ref_extract(300, 1.2f, 4, 20, 7, img.data(), W, H, W, 40, 100, kps.data(), desc.data(), cap, &n);
    fold(d, &mono, sizeof mono);
    fold_kps(d, kps.data(), n);
    fold(d, desc.data(), (size_t)n * 32);
    if (n_keypoints) *n_keypoints = n;
    // octree: scattered keys, a cluster with heavy response ties, one row
    for (int c = 0; c < 3; ++c) {
        const int w = c == 0 ? 608 : c == 1 ? 300 : 127, h = c == 0 ? 448 : c == 1 ? 200 : 64;
        const int nk = c == 0 ? 3000 : c == 1 ? 400 : 50, N = c == 0 ? 500 : c == 1 ? 60 : 7;
        std::vector<oracle_kp> keys(nk), out(nk + 4 * N + 16);
        for (int i = 0; i < nk; ++i) {
            oracle_kp k = {};
            k.x = (float)(c == 1 ? 100 + rng.next() % 24 : rng.next() % w);
            k.y = (float)(c == 1 ? 80 + rng.next() % 24 : c == 2 ? 9 : rng.next() % h);
            k.size = 7, k.angle = -1, k.class_id = -1;
            k.response = (float)(c == 1 ? 20 + rng.next() % 3 : rng.next() % 256);
            keys[i] = k;
        }
        int m = ref_distribute_octree(keys.data(), nk, 16, 16 + w, 16, 16 + h, N, out.data(), (int)out.size());
        fold_kps(d, out.data(), m);
    }
    return d;
}

#ifndef REF_SELFTEST_NO_MAIN
int main() {
    int n = 0;
    uint64_t d = ref_selftest_digest(&n);
    printf("ref_selftest digest %016llx keypoints %d\n", (unsigned long long)d, n);
    return n > 0 ? 0 : 1;
}
#endif
