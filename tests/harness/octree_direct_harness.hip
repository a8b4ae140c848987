// octree_direct_harness.hip -- TEST INFRASTRUCTURE for tests/test_octree_direct.py: the count-pyramid
// formulation of orb_octree.h on the host (SerialPolicy) with the direct phase 1 switched on or
// off, an explicit node capacity, and the round counter of the diagnostic clocks.  Not part of
// liborbgpu.so.
#include <algorithm>
#include <vector>

#include "../../orbslam3lib_amd/csrc/orb_octree.h"
#include "../../orbslam3lib_amd/csrc/orb_policy.h"

using namespace orbgpu;

extern "C" {

// octree_distribute with a pyramid of depth D (D = 0: the label passes).  rounds = 1 walks phase 1
// round by round, 0 builds its list directly.  cap <= 0: the node capacity the product plans.
// A run that returns kOctDeep is redone with the label passes, as the kernel does (*deep = 1).
// counts[0] = rounds the pyramid run executed, counts[1] = the phase-1 rounds among them.
int octd_octree(const uint32_t* keys, int n, int W, int H, int N, int cap, int D, int rounds, uint32_t* out,
                int out_cap, int* deep, long long* counts) {
    const int nIni = oct_nini(W, H);
    if (cap <= 0) cap = std::max(N + 3, 4 * nIni) + 8;
    std::vector<uint16_t> nq(n + 1);
    std::vector<uint8_t> mem(oct_nodemem_bytes(cap) + 64);
    std::vector<uint32_t> pyr(oct_pyr_bytes(D, nIni) / 4 + 1);
    std::vector<uint16_t> tbl(W + H + 2);
    unsigned long long dbg[8] = {};
    OctWST<kGeneric, kGeneric> w;
    w.keys = const_cast<uint32_t*>(keys);  // read-only without a cell gather
    w.n = n;
    w.nq = nq.data();
    w.cell_off = nullptr;
    w.cellkeys = nullptr;
    w.ncells = 0;
    w.cell_cap = 0;
    w.m = oct_nodemem_carve<kGeneric>((uint8_t*)(((uintptr_t)mem.data() + 15) & ~(uintptr_t)15), cap);
    w.cap = cap;
    w.out_keys = out;
    w.out_cap = out_cap;
    w.dbg = dbg;
    w.pyr = pyr.data();
    w.pyrD = D;
    w.xcode = tbl.data();
    w.ycode = tbl.data() + W + 1;
    w.rounds = rounds;
    OctShared sh;
    SerialPolicy p;
    int r = octree_distribute(p, w, &sh, W, H, N);
    counts[0] = (long long)(dbg[7] & 0xFFFFFFFFull);
    counts[1] = (long long)(dbg[7] >> 32);
    *deep = r == kOctDeep;
    if (r == kOctDeep) {
        w.pyrD = 0;
        r = octree_distribute(p, w, &sh, W, H, N);
    }
    return r;
}

// The same node of the key order two ways: oct_key_path (the closed form) against the recurrence
// k_{d+1} = 4 (nIni 4^d - 1 - k_d) + (3 - q_{d+1}) run forwards from a path index.
uint32_t octd_key_of_path(int d, uint32_t idx, int nIni) {
    uint32_t k = idx >> (2 * d);
    for (int s = 0; s < d; ++s) {
        const uint32_t q = (idx >> (2 * (d - 1 - s))) & 3u;
        k = 4u * ((uint32_t)(nIni << (2 * s)) - 1u - k) + (3u - q);
    }
    return k;
}
uint32_t octd_path_of_key(int d, uint32_t k, int nIni) { return oct_key_path(d, k, nIni); }

}  // extern "C"
