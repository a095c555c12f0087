// arp_api.hip — C ABI (include/arpeggio_hip.h) over the HIP kernels.  gfx950 only.
//
// Build: hipcc --offload-arch=gfx950 -O3 -std=c++17 -ffp-contract=off -shared -fPIC
//        arp_api.hip -o libarpeggio_hip.so
#include <hip/hip_runtime.h>

#include <algorithm>
#include <atomic>
#include <chrono>
#include <cmath>
#include <mutex>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <functional>
#include <string>
#include <vector>

#include "../../include/arpeggio_hip.h"
#include "arp_grid.h"
#include "arp_numerics.h"
#include "arp_pairs.h"
#include "arp_bag_table.h"
#include "arp_planes.h"
#include "arp_prepare.h"
#include "arp_models.h"
#include "arp_json.h"
#include "arp_shard.h"
#include "arp_cif.h"
#include "arp_comm.h"
#include "arp_sort.h"
#include "arp_persist.h"
#include "arp_respair.h"
#include "arp_respersist.h"
#include "arp_filter.h"
#include "arp_bridge.h"
#include "arp_bridgepersist.h"
#include "arp_similarity.h"
#include "arp_coupling.h"
#include "arp_lifetimes.h"
#include "arp_networks.h"
#include "arp_poses.h"
#include "arp_poses_planes.h"
#include "arp_poses_fingerprints.h"
#include "arp_poses_shortlist.h"
#include "arp_library_shortlist.h"
#include "arp_poses_clusters.h"
#include "arp_library_clusters.h"
#include "arp_library.h"
#include "arp_library_fingerprints.h"
#include "arp_library_planes.h"
#include "arp_library_bridges.h"
#include "arp_blob.h"

namespace {

std::string g_create_error;   // arp_create failures only (no context to hold the message); written under g_create_mutex
std::mutex g_create_mutex;
void set_create_error(const std::string& m) {
    std::lock_guard<std::mutex> lk(g_create_mutex);
    g_create_error = m;
}

template <class T>
struct DevBuf {
    T* p = nullptr;
    size_t cap = 0;
    bool borrowed = false;   // p points into memory owned by someone else (the device copy of an uploaded blob)
    // *fresh (optional) is set when new memory was allocated (contents undefined)
    hipError_t reserve(size_t n, bool* fresh = nullptr) {
        if (fresh) *fresh = false;
        if (n <= cap && p) return hipSuccess;
        release();
        size_t c = n + n / 4 + 64;
        hipError_t e = hipMalloc((void**)&p, c * sizeof(T));
        if (e == hipSuccess) { cap = c; if (fresh) *fresh = true; }
        else p = nullptr;
        return e;
    }
    void borrow(void* ptr, size_t n) {
        release();
        p = (T*)ptr;
        cap = n;
        borrowed = true;
    }
    void release() {
        if (p && !borrowed) (void)hipFree(p);
        p = nullptr;
        cap = 0;
        borrowed = false;
    }
};

struct Grid {
    GridDesc d{};
    DevBuf<int> cell_of, cnt, start, perm, sums;
    // atom grids: {cell, rank in cell} per atom and a second histogram buffer (double-buffered: a build counts in
    // hist[cur] and clears hist[1 - cur], the one the previous build used)
    DevBuf<int2> cell_rank;
    DevBuf<int> cnt2;
    DevBuf<unsigned long long> chain;   // k_scan_tiles_chained: {launch number, tile total} per tile
    unsigned int chain_epoch = 0;
    int cur = 0;
    size_t used[2] = {0, 0};   // counters of hist[k] that may be non-zero
    int n_points = 0;   // points offered
    int n_binned = 0;   // points that passed the filter
    bool valid = false;
    double radius = 0;
    void release() { cell_of.release(); cnt.release(); start.release(); perm.release(); sums.release(); cell_rank.release();
                     cnt2.release(); chain.release(); valid = false; }
};

struct Bag {  // outputs of one ring/amide kernel, resident in HBM until fetched: the columns PLANE_TABLES (arp_bag_table.h) names
    // the arrays are sub-ranges of ONE allocation (slab), so that a small bag reaches the host with one copy
    DevBuf<uint8_t> slab;
    uint8_t* col[BAG_COLS] = {};   // column j of the table; null: the bag has no such column
    int* id(int q) const { return (int*)col[q]; }
    template <class T> T* val(int q) const { return (T*)col[BAG_VAL0 + q]; }
    uint8_t* byte(int q) const { return col[BAG_BYTE0 + q]; }
    size_t cap = 0;
    int64_t count = 0;
    bool valid = false;
    uint64_t version = 0;        // bumped whenever a launch refills the bag
    uint64_t staged_version = 0; // version whose records are in the context's page-locked staging area, at stage_off[]
    size_t stage_off[BAG_COLS] = {0};
    void release() { slab.release(); for (uint8_t*& p : col) p = nullptr; cap = 0; valid = false; staged_version = 0; }
};

// scratch of the radix sort (arp_sort.h: radix_sort): keys and payload double-buffered, digit table, digit totals
struct SortScratch {
    DevBuf<unsigned long long> key[2], val[2];
    DevBuf<int> table;
    DevBuf<long long> total;
    void release() { key[0].release(); key[1].release(); val[0].release(); val[1].release(); table.release(); total.release(); }
};

// the used prefixes of every array of every bag, gathered into one device buffer for one copy to the host
// (perm: the segment's elements — es bytes each — leave in the order perm[0], perm[1], ...: the canonical order of a small bag)
struct PackSeg { const uint8_t* src; uint32_t dst, bytes; const uint32_t* perm; uint32_t es; };
struct PackTable { PackSeg s[48]; int n; };
// n 16-byte quads from the device to a page-locked host buffer (small results: see arp_fetch_packed)
__global__ __launch_bounds__(256) void k_copy_quads(const int4* __restrict__ src, int4* __restrict__ dst, unsigned n) {
    for (unsigned i = blockIdx.x * blockDim.x + threadIdx.x; i < n; i += gridDim.x * blockDim.x) dst[i] = src[i];
}
__global__ __launch_bounds__(256) void k_pack_segments(PackTable t, uint8_t* __restrict__ out) {
    const PackSeg g = t.s[blockIdx.y];        // segment blockIdx.y, spread over the gridDim.x blocks of its row
    if (g.perm) {
        const uint32_t n = g.bytes / g.es;
        for (uint32_t i = blockIdx.x * blockDim.x + threadIdx.x; i < n; i += gridDim.x * blockDim.x) {
            const uint32_t q = g.perm[i];
            if (g.es == 4) reinterpret_cast<uint32_t*>(out + g.dst)[i] = reinterpret_cast<const uint32_t*>(g.src)[q];
            else if (g.es == 8) reinterpret_cast<unsigned long long*>(out + g.dst)[i] = reinterpret_cast<const unsigned long long*>(g.src)[q];
            else out[g.dst + i] = g.src[q];
        }
        return;
    }
    const uint32_t words = g.bytes >> 2;
    const uint32_t* __restrict__ src = reinterpret_cast<const uint32_t*>(g.src);      // (arrays of a slab start on 256-byte boundaries,
    uint32_t* __restrict__ dst = reinterpret_cast<uint32_t*>(out + g.dst);            //  destinations on 16-byte ones)
    for (uint32_t i = blockIdx.x * blockDim.x + threadIdx.x; i < words; i += gridDim.x * blockDim.x) dst[i] = src[i];
    if (blockIdx.x == 0 && threadIdx.x < (g.bytes & 3u)) out[g.dst + (words << 2) + threadIdx.x] = g.src[(words << 2) + threadIdx.x];
}
// Canonical order of the four ring / amide bags (the order the reference creates their records in: by the ids of the two
// partners, I:947-1382): the kernels emit them through one atomic counter per bag, i.e. in any order.  A bag of up to
// BAG_SORT_MAX records is sorted by ONE block (bitonic network in LDS on {first id, second id, record index}); larger bags keep
// the device's order (the caller sorts them: config 5 has 10^5 records per bag, a protein a few hundred).
#define BAG_SORT_MAX 8192      // (96 KB of LDS: key + index)
static_assert(BAG_SORT_MAX == ARP_BAG_SORT_MAX, "include/arpeggio_hip.h");
struct BagOrderArgs { const int* first[4]; const int* second[4]; int n[4]; uint32_t* perm[4]; };
__global__ __launch_bounds__(1024) void k_bag_order(BagOrderArgs A) {
    __shared__ unsigned long long s_key[BAG_SORT_MAX];
    __shared__ uint32_t s_idx[BAG_SORT_MAX];
    const int b = blockIdx.x, n = A.n[b];
    if (n <= 0 || n > BAG_SORT_MAX) return;
    int m = 2;
    while (m < n) m <<= 1;
    const int tid = (int)threadIdx.x, lane = tid & 63, w = tid >> 6;
    for (int i = tid; i < m; i += 1024) {
        s_key[i] = i < n ? (((unsigned long long)(uint32_t)A.first[b][i] << 32) | (unsigned long long)(uint32_t)A.second[b][i]) : ~0ull;
        s_idx[i] = (uint32_t)i;
    }
    __syncthreads();
    // Bitonic network over m slots.  Every wave owns a contiguous chunk of C slots: the steps whose partners lie inside a chunk
    // (distance j < C: 81 of the 91 steps of 8192 slots) need no block barrier — a wave's LDS operations are performed in
    // order — and a step walks the m / 2 PAIRS, not the m slots.  (One barrier per step over all slots: 176 us for 8192.)
    const int C = max(m / 16, min(m, 128));
    const int nwave_active = m / C;
    auto step = [&](int pr, int j, int k) {      // compare-exchange of pair pr at distance j inside the merge of size k
        const int i = ((pr & ~(j - 1)) << 1) | (pr & (j - 1)), l = i + j;
        const unsigned long long ka = s_key[i], kb = s_key[l];
        const uint32_t ia = s_idx[i], ib = s_idx[l];
        const bool up = (i & k) == 0;
        const bool gt = ka > kb || (ka == kb && ia > ib);      // (ties by record index: the order is a function of the records)
        if (gt == up) { s_key[i] = kb; s_key[l] = ka; s_idx[i] = ib; s_idx[l] = ia; }
    };
    for (int k = 2; k <= m; k <<= 1)
        for (int j = k >> 1; j > 0; j >>= 1) {
            if (j >= C) {
                __syncthreads();
                for (int pr = tid; pr < (m >> 1); pr += 1024) step(pr, j, k);
                __syncthreads();
            } else {
                if (w < nwave_active)
                    for (int q = lane; q < (C >> 1); q += 64) step(w * (C >> 1) + q, j, k);
                __builtin_amdgcn_wave_barrier();
                asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
            }
        }
    __syncthreads();
    for (int i = tid; i < n; i += 1024) A.perm[b][i] = s_idx[i];
}
// blocks per segment: one per 16 KiB of the largest segment, at most 64
inline dim3 pack_grid(const PackTable& t) {
    uint32_t mx = 0;
    for (int k = 0; k < t.n; ++k) mx = std::max(mx, t.s[k].bytes);
    return dim3(std::min<uint32_t>(std::max<uint32_t>((mx + 16383u) >> 14, 1u), 64u), (unsigned)t.n);
}

// arp_set_batch: item i belongs to the structure s with off[s] <= i < off[s + 1] (empty structures have none)
__global__ __launch_bounds__(256) void k_fill_sid(const long long* __restrict__ off, int nstruct, int* __restrict__ sid, long long total) {
    for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (long long)gridDim.x * blockDim.x) {
        int lo = 0, hi = nstruct;
        while (hi - lo > 1) {
            const int mid = (lo + hi) >> 1;
            if (off[mid] <= i) lo = mid; else hi = mid;
        }
        sid[i] = lo;
    }
}

enum Slot { SLOT_BIN = 0, SLOT_SCAN = 1, SLOT_SCATTER = 2, SLOT_UNUSED = 3, SLOT_SEARCH = 4, SLOT_SIFT = 5, SLOT_MARK = 6, SLOT_PLANES = 7, NSLOT = 8 };

struct EventPair { int slot; hipEvent_t a, b; };

// What the contact grid of a whole-structure pass was built from: a pass with an equal key reuses it (arp_ctx::grid_reuse)
struct GridKey {
    double radius = 0.0;
    uint64_t static_epoch = 0, sel_epoch = 0;
    bool fuse_sets = false, init_plus = false, all_res = false;
    bool operator==(const GridKey& o) const {
        return radius == o.radius && static_epoch == o.static_epoch && sel_epoch == o.sel_epoch && fuse_sets == o.fuse_sets &&
               init_plus == o.init_plus && all_res == o.all_res;
    }
};
// What a balance hint of k_search (sb_tile) was made for: grid, launch shape, and what its entries are (by_atoms: atom
// positions, k_balance_atoms; else tiles, k_balance_blocks)
struct HintKey {
    bool by_atoms = false;
    uint64_t static_epoch = 0, sel_epoch = 0;
    double radius = 0.0;
    int blocks = 0, tx = 0;
    bool operator==(const HintKey& o) const {
        return by_atoms == o.by_atoms && static_epoch == o.static_epoch && sel_epoch == o.sel_epoch && radius == o.radius &&
               blocks == o.blocks && tx == o.tx;
    }
};

}  // namespace

// a table reduced on the device: its columns in one piece (table_layout), its rows, whether it is that of the last results, and
// the arguments of the launch that made it (0 for a launch without; a launch with more than two packs them into the two
// words); launches counts the launches that made it anew
struct ResultTable {
    DevBuf<uint8_t> slab;
    int64_t count = 0, launches = 0;
    uint64_t arg[2] = {0, 0};
    bool valid = false;
    bool made_with(uint64_t arg0, uint64_t arg1) const { return valid && arg[0] == arg0 && arg[1] == arg1; }
};

// the atom-atom records a caller asked for (arp_contacts_filter_launch): the kept records as the filter left them, and their
// canonical order in a slab of their own, laid out as sorted_slab is — with room for the ring / amide bags behind the columns
struct FilteredBag {
    DevBuf<uint8_t> cols, slab;
    int64_t count = 0;
    uint32_t sift_any = 0, ctype_mask = 0;
    bool csr = false;                   // the slab's first column is N + 1 row offsets
    bool valid = false;
};

// the model-by-model matrix of shared features (arp_models_similarity_launch): the bit matrix it is multiplied from, the
// matrix, and what it was made for; rows / words / slices / launches answer arp_models_similarity_info
struct SimilarityResult {
    DevBuf<unsigned long long> bits;
    DevBuf<uint32_t> inter;
    int64_t F = 0, rows = 0, words = 0, slices = 0, launches = 0;
    uint32_t planes = 0, ctype_mask = 0, flags = 0;
    bool valid = false;
};

// what the coupling tables (arp_models_coupling_launch) keep beside their slab: the model bits of all U rows and of the K
// features with their counts, and what arp_models_coupling_info answers
struct CouplingScratch {
    DevBuf<unsigned long long> rowbits, bits;
    DevBuf<uint32_t> n_row, n;
    int64_t rows = 0, features = 0, tile_pairs = 0;
    uint32_t flags = 0;
};

// What a launch over poses keeps of its records (arp_poses_contacts_launch and arp_library_contacts_launch, pose_records_launch):
// the uploaded poses, the counters, the per-pose summary rows and record offsets, the appended records and their sort, the
// result's five columns in one slab
struct PoseRecords {
    DevBuf<float> xyz;
    DevBuf<double> hx;
    DevBuf<unsigned long long> ctr;                     // [0] records appended, [1] device error
    DevBuf<uint32_t> summary;
    DevBuf<unsigned long long> pose_off;
    SortScratch sort;
    DevBuf<uint8_t> slab;
    size_t off[5] = {0, 0, 0, 0, 0};
    int64_t count = 0;
    void release() { xyz.release(); hx.release(); ctr.release(); summary.release(); pose_off.release(); sort.release(); slab.release(); }
};
// the contacts of ligand poses on the resident receptor (arp_poses_contacts_launch): the movable set's tables (made once per
// structure and selection) and the records
struct PosesResult {
    DevBuf<int> sel_h, pos_of;
    uint64_t movable_static = 0, movable_sel = 0;       // static_epoch / sel_epoch the tables were made for (0: none)
    PoseRecords rec;
    int64_t P = 0, S = 0, SH = 0;
    bool valid = false;
    void release() { sel_h.release(); pos_of.release(); rec.release(); movable_static = movable_sel = 0; valid = false; }
};

// the ligand library (arp_set_ligand_library, arp_library.h): the ligands' per-atom table beside the receptor.  It reads nothing of
// the resident structure and stays through new structures; the host keeps the offsets a launch lays its poses out by
struct LigandLibrary {
    DevBuf<int> atom_off, h_off, sb_nbr;
    DevBuf<uint16_t> tmask, flags;
    DevBuf<double2> rad;
    std::vector<int> host_atom_off, host_hrows;         // [L + 1]; [L] hydrogen rows of ligand l
    int64_t L = 0, atoms = 0, hrows = 0;
    int max_atoms = 0;
    bool resident = false;
    void release() { atom_off.release(); h_off.release(); sb_nbr.release(); tmask.release(); flags.release(); rad.release(); resident = false; }
};
// the contacts of a launch over the library (arp_library_contacts_launch): the per-pose / per-ligand tables of the uploaded poses
// and the records; and the best pose per ligand made from their summary (arp_library_best_launch), which goes with them
// (void_pose_results)
struct LibraryResult {
    DevBuf<int> lig_of;
    DevBuf<long long> tab;                              // pose_off [L + 1] | xyz_at [L] | hx_at [L]
    PoseRecords rec;
    DevBuf<long long> best_n, best_score;
    DevBuf<int> best_pose;
    std::vector<int64_t> host_pose_off;                 // [L + 1] as the launch took it (the library shortlist: candidates, same poses)
    int64_t L = 0, T = 0, blocks = 0, nx = 0;           // nx: the floats of the uploaded poses
    double cutoff = 0.0, vdw_comp = 0.0;                // of the launch (the library water bridges: the receptor's pass must match)
    bool valid = false, best_valid = false;
    void release() {
        lig_of.release(); tab.release(); rec.release(); best_n.release(); best_score.release(); best_pose.release(); valid = best_valid = false;
    }
};

// the fingerprints of the resident poses result (arp_poses_fingerprints_launch, arp_poses_fingerprints.h): the presence bitmap of
// the nodes with its word bases, the columns, the bit matrix, the scores, and what they were made for.  Valid only while the
// poses result it was made from is (void_pose_results); one made with class planes
// (arp_poses_fingerprints_planes_launch: `classes`) read the poses-planes result too and goes with either
struct PoseFpResult {
    DevBuf<unsigned long long> presence, bits;
    DevBuf<uint32_t> base, count, cross, occ, inter;
    DevBuf<long long> total;
    DevBuf<int> ids;
    int64_t P = 0, Q = 0, U = 0, NP = 0, W = 0, slices = 0, launches = 0;
    uint32_t planes = 0, ctype_mask = 0, flags = 0;
    bool valid = false, classes = false;
    void release() {
        presence.release(); bits.release(); base.release(); count.release(); cross.release(); occ.release(); inter.release();
        total.release(); ids.release(); valid = false;
    }
};

// what the fingerprints of the resident library result (arp_library_fingerprints_launch, arp_library_fingerprints.h) keep beside
// their PoseFpResult (arp_ctx::libfp): the uploaded references, and the best pose per (ligand, reference) made from count and
// cross (arp_library_fingerprints_best_launch), which goes with them (void_pose_results)
struct LibraryFpTables {
    DevBuf<long long> ref_off, best_n, best_q32;
    DevBuf<int> ref_node, best_pose;
    DevBuf<uint32_t> ref_planes, best_shared, best_count;
    int64_t L = 0, features = 0;
    bool best_valid = false;
    void release() {
        ref_off.release(); best_n.release(); best_q32.release(); ref_node.release(); best_pose.release(); ref_planes.release();
        best_shared.release(); best_count.release(); best_valid = false;
    }
};

// the shortlist of the resident poses result (arp_poses_shortlist_launch, arp_poses_shortlist.h): a sort scratch of its own (the
// source's sorted buffers are not disturbed), the chosen poses with their scores and summary rows, lengths and offsets per table,
// the word block of the one wait, and the chosen poses' records in one slab.  Valid only while the poses result is; one that
// read the poses-planes result (`planes`) goes with that as well.  The library shortlist (arp_library_shortlist_launch,
// arp_library_shortlist.h) is a second object of the same shape over the library's results: `ligand` and `unit` are its own
struct ShortlistResult {
    SortScratch sort;
    DevBuf<int> ids, pose, ligand;
    DevBuf<long long> score;
    DevBuf<uint32_t> summary, pl_summary;
    DevBuf<unsigned long long> len, off, words;
    DevBuf<uint8_t> slab;
    size_t aa_off[5] = {0, 0, 0, 0, 0};
    PplColumns col{};
    int64_t K = 0, ncand = 0, total[PSL_TABLES] = {0, 0, 0, 0, 0}, launches = 0;
    int kind = 0, unit = 0;
    uint32_t tables = 0;
    bool valid = false, planes = false;
    void release() {
        sort.release(); ids.release(); pose.release(); ligand.release(); score.release(); summary.release(); pl_summary.release(); len.release(); off.release();
        words.release(); slab.release(); valid = false;
    }
};

// the leader clustering of the resident fingerprint result (arp_poses_clusters_launch, arp_poses_clusters.h): the leaders' positions
// round by round (`next`), the per-position and per-cluster arrays, the uploaded order (or none) and the word block of the last
// wait.  The fingerprint result is read only while the launch runs: valid while the poses result is; one made from a fingerprint
// with class planes (`classes`) goes with the poses-planes result as well
struct ClustersResult {
    DevBuf<uint32_t> next, size;
    DevBuf<int> order, pose, cluster, leader, leader_position;
    DevBuf<long long> similarity;
    DevBuf<unsigned long long> words;
    int64_t M = 0, C = 0, unassigned = 0, max_clusters = 0, W = 0, lanes = 0, launches = 0;
    uint64_t threshold = 0;
    bool valid = false, classes = false;
    void release() {
        next.release(); size.release(); order.release(); pose.release(); cluster.release(); leader.release(); leader_position.release();
        similarity.release(); words.release(); valid = false;
    }
};

// the leader clustering of the resident library fingerprint (arp_library_clusters_launch, arp_library_clusters.h): the window
// form's round state (`start`, the leaders of each round `wl` with their number `nl`, `made`), the per-position and per-cluster
// arrays with `ligand` beside `pose`, the uploaded list (or none) and the word block of the last wait.  The fingerprint and the
// shortlist are read only while the launch runs: valid while the library result is (void_pose_results)
struct LibClustersResult {
    DevBuf<uint32_t> start, nl, made, size;
    DevBuf<int> order, wl, pose, ligand, cluster, leader, leader_position;
    DevBuf<long long> similarity;
    DevBuf<unsigned long long> words;
    int64_t M = 0, C = 0, unassigned = 0, max_clusters = 0, W = 0, rounds = 0, launches = 0;
    uint64_t threshold = 0;
    bool valid = false;
    void release() {
        start.release(); nl.release(); made.release(); size.release(); order.release(); wl.release(); pose.release(); ligand.release();
        cluster.release(); leader.release(); leader_position.release(); similarity.release(); words.release(); valid = false;
    }
};

// the ligand-water-receptor contacts of the resident library result (arp_library_water_bridges_launch, arp_library_bridges.h): a sort
// scratch of its own for the receptor's legs (the shared one and the water-bridge table are left alone), the table of every
// water's legs by atom id, the per-tile counts with their totals, the prefixes at every pose's first record, the per-pose arrays
// and the eight columns in one slab.  Valid while the library result AND the atom-atom bag are (void_pose_results, void_results)
struct LibBridgesResult {
    SortScratch sort;
    DevBuf<uint2> water_legs;
    DevBuf<long long> tile, totals, at;
    DevBuf<unsigned long long> bridge_off;
    DevBuf<uint32_t> waters, legs;
    DevBuf<uint8_t> slab;
    size_t off[8] = {0, 0, 0, 0, 0, 0, 0, 0};
    int64_t T = 0, rows = 0, lig_legs = 0, rec_legs = 0, rec_waters = 0, launches = 0;
    uint32_t sift_any = 0;
    bool valid = false;
    void release() {
        sort.release(); water_legs.release(); tile.release(); totals.release(); at.release(); bridge_off.release(); waters.release(); legs.release();
        slab.release(); valid = false;
    }
};

// the ring / amide contacts of ligand poses (arp_poses_planes_launch, arp_poses_planes.h): the atoms of the resident rings and
// amides (arp_set_plane_atoms), the movable set's tables (made once per structure, selection and plane atoms), an all-atom 6 A
// grid of its own by local id (the static order of the passes is left alone), the per-block lists, the records and their sort
struct PosesPlanesResult {
    DevBuf<int> ring_off, ring_idx, amide_atoms;
    bool have_atoms = false;
    DevBuf<int> pos_of, hist, res_off, res_atoms, mring, hring, mamide, am_pos, cnt, sums;
    DevBuf<uint8_t> res_selm, ring_static;
    Grid grid;
    bool setup = false;
    int n_mring = 0, n_hring = 0, n_mamide = 0;
    DevBuf<float> xyz;
    DevBuf<PplRing> ws_ring;
    DevBuf<PplAmide> ws_amide;
    DevBuf<PlaneRec> rec;
    DevBuf<unsigned long long> ctr, pose_off;
    DevBuf<uint32_t> summary;
    SortScratch sort;
    DevBuf<uint8_t> slab;
    PplColumns col{};
    int64_t counts[4] = {0, 0, 0, 0};
    int64_t P = 0, S = 0, launches = 0;
    bool valid = false;
    void release() {
        ring_off.release(); ring_idx.release(); amide_atoms.release(); pos_of.release(); hist.release(); res_off.release(); res_atoms.release();
        mring.release(); hring.release(); mamide.release(); am_pos.release(); cnt.release(); sums.release(); res_selm.release(); ring_static.release();
        grid.release(); xyz.release(); ws_ring.release(); ws_amide.release(); rec.release(); ctr.release(); pose_off.release(); summary.release();
        sort.release(); slab.release(); have_atoms = setup = valid = false;
    }
};

// the plane table of the ligand library (arp_set_ligand_library_planes, arp_library_planes.h): ring paths and amide atoms by index
// within the ligand, CSR over the ligands.  Like the library it reads nothing of the resident structure
struct LibraryPlaneAtoms {
    DevBuf<int> ring_off, ring_atom_off, ring_atom_idx, amide_off, amide_atoms;
    int64_t L = 0, TR = 0, TM = 0;
    bool resident = false;
    void release() { ring_off.release(); ring_atom_off.release(); ring_atom_idx.release(); amide_off.release(); amide_atoms.release(); resident = false; }
};
// the ring / amide contacts of a launch over the library (arp_library_planes_launch): the per-structure set-up (an all-atom 6 A
// grid of its own by local id and the residue -> atoms CSR of the receptor), the per-pose / per-ligand tables of the uploaded
// poses, the per-block lists, the records and their sort, the four tables in one slab
struct LibraryPlanesResult {
    DevBuf<int> hist, res_off, res_atoms, sums;
    Grid grid;
    bool setup = false;
    DevBuf<int> lig_of;
    DevBuf<long long> tab;                              // pose_off [L + 1] | xyz_at [L]
    DevBuf<float> xyz;
    DevBuf<PplRing> ws_ring;
    DevBuf<PplAmide> ws_amide;
    DevBuf<PlaneRec> rec;
    DevBuf<unsigned long long> ctr, pose_off;
    DevBuf<uint32_t> summary;
    SortScratch sort;
    DevBuf<uint8_t> slab;
    PplColumns col{};
    int64_t counts[4] = {0, 0, 0, 0};
    std::vector<int64_t> host_pose_off;                 // [L + 1] as the launch took it
    int64_t L = 0, T = 0, blocks = 0, launches = 0, nx = 0;
    bool valid = false;
    void release() {
        hist.release(); res_off.release(); res_atoms.release(); sums.release(); grid.release(); lig_of.release(); tab.release(); xyz.release();
        ws_ring.release(); ws_amide.release(); rec.release(); ctr.release(); pose_off.release(); summary.release(); sort.release(); slab.release();
        setup = valid = false;
    }
};

struct arp_ctx {
    int device = 0;
    hipStream_t stream = nullptr;       // the stream every pass is enqueued on (own_stream unless arp_use_stream)
    hipStream_t own_stream = nullptr;
    bool external_stream = false;
    std::string err;
    int num_cu = 256;
    int search_resident = 768;          // blocks of k_search<MODE_CONTACTS> the chip holds at once (occupancy x CUs)
    int sift_per_cu = 4;                // blocks of the per-pair kernel a CU holds at once
    bool xcd_round_robin = true;   // consecutive blocks of a launch land on XCDs (x0 + b) % 8 (arp_create's probe)
    uint64_t seg_last[PAIR_SEGS] = {0, 0, 0, 0, 0, 0, 0, 0};   // pairs per segment of the last contact pass (the next one's sift blocks are shared out by it)

    // ---- sizes
    int64_t n = 0, nres = 0, nring = 0, namide = 0;
    // ---- host mirrors needed for later set_* calls / grid boxes
    std::vector<float> h_xyz;
    double lo[3] = {0, 0, 0}, hi[3] = {0, 0, 0};
    double ring_lo[3] = {0, 0, 0}, ring_hi[3] = {0, 0, 0};
    double am_lo[3] = {0, 0, 0}, am_hi[3] = {0, 0, 0};
    // ---- raw inputs
    DevBuf<float4> xyz;          // w unused
    DevBuf<double2> rad;         // {vdw, cov}
    DevBuf<uint16_t> tmask, flags;
    DevBuf<int> res_id, res_prev, res_next;
    DevBuf<uint8_t> res_flags;
    DevBuf<int> bond_off, bond_idx, h_off;
    DevBuf<double> h_xyz_d;
    DevBuf<float4> sb;           // single-bond neighbour xyz, w = 1 if present
    DevBuf<int> sb_idx;          // ... and which atom it is, as arp_set_single_bond_neighbours uploaded it
    int sb_index_src = 0;        // where the resident neighbour INDEX is: 0 nowhere (coordinates only), 1 sb_idx, 2 blob_sb_nbr
    DevBuf<int> gid;
    DevBuf<uint8_t> home, sel, plus, res_sel, res_plus;
    bool has_res = false, has_gid = false, has_home = false;
    int64_t max_res_id = -1, max_ring_res = -1, max_amide_res = -1;   // host-side range checks of the uploaded indices
    bool sel_made = false;
    bool sel_uploaded = false;   // arp_set_selection / arp_set_selection_state since the last arp_set_atoms
    bool sel_prefilled = false;  // sel already holds the default selection (all ones) for the resident structure: written while arp_set_blob waited for the validation
    size_t sp_cnt_zeroed = 0;    // leading ints of sp_cnt cleared the same way (ensure_static's fill of a fresh structure)
    bool sel_all = false;        // the uploaded selection covers every atom: selection_plus = selection, no expansion search
    int64_t nsel = -1;            // selected atoms of the uploaded mask; their indices are in sel_list when nsel <= SMALL_SEL_MAX
    DevBuf<int> sel_list;
    bool whole_structure = false; // caller's assertion (arp_set_whole_structure): the selection is the whole GLOBAL structure
    DevBuf<double> ring_c, ring_n;
    DevBuf<int> ring_res;
    DevBuf<uint8_t> ring_sel, ring_plus;
    DevBuf<float> am_c, am_n;
    DevBuf<int> am_res;
    DevBuf<uint8_t> am_sel, am_plus;
    DevBuf<uint8_t> ring_home, am_home;
    DevBuf<int> ring_gid, am_gid;
    bool has_group_owner = false;
    // ---- derived
    DevBuf<float4> s_xyzm;
    DevBuf<int4> s_aux;
    DevBuf<int4> s_qa;            // second quad of the sift records, cell-sorted (the first one is s_xyzm)
    DevBuf<int> st_h, sp_h, s_h;  // index of every atom's first hydrogen: static, in the spatial order, cell-sorted
    DevBuf<int> tmp_i32;          // scratch for index uploads
    DevBuf<int4> st_qa;           // selection-independent record columns, composed once per structure (k_prepare_static)
    DevBuf<float> longest_bond;   // k_longest_bond, once per uploaded structure (ensure_static)
    DevBuf<uint16_t> rad_idx;     // per atom: index of its {vdw, cov} pair in rad_tab (RAD_NONE: not in the table)
    DevBuf<double2> rad_tab;      // RAD_TABLE distinct radius pairs of the structure
    DevBuf<int4> st_aux;
    DevBuf<float4> st_xyzm;
    DevBuf<float4> sp_xyzm;       // the same columns in the spatial order of the structure (what the per-pass grid builds read)
    DevBuf<int4> sp_aux, sp_qa;
    DevBuf<int> sp_cnt;
    DevBuf<int> sp_sums;         // tile totals of the static order's scan (grids beyond 32768 cells)
    DevBuf<int2> sp_cr;
    DevBuf<int> sp_cell;          // cell of every row of the spatial order
    GridDesc sp_grid{};           // the grid the spatial order was made for
    double sp_radius = 0;         // ... and its cell edge (0: no order yet)
    DevBuf<unsigned long long> compact_chain;   // k_compact_atoms: one word per block
    // sp_keep_base: kept rows (no hydrogens) before every block of a whole-structure k_compact_atoms over the spatial order, made
    // from the order by the second such build over it (make_keep_bases).  Layout: [ticket, 3 words of padding | count per block | base per block, the total last]
    DevBuf<int> sp_keep;
    int sp_keep_rows = 0, sp_keep_blocks = 0;   // rows per block the table was made for, and its blocks
    uint64_t sp_keep_epoch = 0;                 // static_epoch of the order it describes (0: none)
    uint64_t sp_keep_seen = 0;                  // static_epoch of the last order a whole-structure grid was built over without it
#ifdef ARP_COMPACT_LOOKBACK                     // (developer builds: the look-back everywhere, for A/B runs of one source)
    bool compact_lookback = true;
#else
    bool compact_lookback = false;              // arp_set_compact_lookback: tests compare the two ways of finding a block's base
#endif
    bool compact_used_table = false;            // the last grid build read the table
    DevBuf<int> s_cell;                         // cell of every row of the contact grid (k_search: blocks split by atoms)
    bool s_cell_valid = false;                  // ... written by the build of the grid that is in place
    DevBuf<int> sb_tile;                        // k_search's runs of tiles with equal numbers of atoms (k_balance_blocks): a hint from the pass before
    bool sb_valid = false;
    HintKey sb_key;                                          // ... what it was made for
    DevBuf<int> sb_cw, sb_cwp, sb_sums;                      // weight per cell, its running sum, tile totals of that scan
    // (the key of the last pass that ran WITHOUT a hint: the hint is worked out by the second such pass over one grid — a
    // structure that is evaluated once, the usual case, never pays for it)
    bool sb_seen = false;
    HintKey sb_seen_key;
    unsigned int compact_epoch = 0;
    bool static_dirty = true;
    // The contact grid of a WHOLE-STRUCTURE pass (every atom selected: selection_plus = all atoms, I:1395 / 1407) depends on the
    // structure and the cell edge only — it is the structure's own neighbour grid, the counterpart of the KD-tree the reference
    // builds over `entity` (I:1394).  Such a pass keeps it: the next one with the same structure, cell edge and (whole)
    // selection launches no k_compact_atoms.  Any other selection compacts per pass, as the reference rebuilds
    // NeighborSearch(selection_plus) (I:1442).  arp_set_grid_reuse(ctx, 0) switches the reuse off (bench.py reports both).
    bool grid_reuse = true;
    bool sort_after_pass = false;     // arp_set_sort_after_pass
    bool cg_valid = false, cg_pending = false, cg_reused = false;
    GridKey cg_key;                   // what the grid in place was built from
    uint64_t static_epoch = 0, sel_epoch = 0;
    int64_t cg_binned = 0;
    double host_enqueue_us = 0, host_wait_us = 0;   // arp_run_launch: time spent enqueueing / waiting (arp_get_host_times)
    int64_t host_passes = 0;
    Grid atom_grid, all_grid, ring_grid, amide_grid;   // contact grid (selection_plus, no H) / every atom at 6 A
    DevBuf<float4> a_xyzm;        // cell-sorted records of all_grid
    DevBuf<int4> a_aux;
    bool all_grid_current = false;  // all_grid matches the current inputs and selection
    hipStream_t stream2 = nullptr;  // ring / amide kernels run here, concurrently with the contact pipeline
    hipEvent_t ev_sel = nullptr, ev_planes = nullptr, ev_lists = nullptr;
    // arp_set_blob: the centre grids and candidate lists of the new structure are made on the second stream, behind ev_upload (the
    // validation kernel on the main one) and in front of ev_uplists; the main stream joins them before anything reads or replaces
    // what they read or write (join_upload_lists)
    hipEvent_t ev_upload = nullptr, ev_uplists = nullptr;
    bool uplists_pending = false;
    DevBuf<int> upload_bad;           // number of the last upload whose device-side check failed (validate_resident_blob)
    bool upload_bad_cleared = false;
    int ahead_seq = 0;                // != 0: ensure_static is enqueued ahead of the verdict of upload number ahead_seq
    double last_cutoff = 0.0;         // cell edge of the context's last pass
    bool uplists_defer = false;       // inside enqueue_contacts: see join_upload_lists
    DevBuf<uint8_t> tmp_u8;
    // ---- pair list and outputs of the atom-contact pass
    DevBuf<int2> pairs;
    DevBuf<int> out_i, out_j;
    DevBuf<float> out_d;
    DevBuf<uint16_t> out_s;
    DevBuf<uint8_t> out_ct;
    int64_t n_contacts = 0;
    // ---- canonical (i, j) order of the atom-atom bag, made on the device (arp_sort.h; arp_atom_contacts_sort)
    SortScratch sort_aa;
    DevBuf<uint8_t> sorted_slab;        // the five sorted columns (+ the packed ring / amide bags of a packed fetch) in one piece
    size_t srt_off[5] = {0, 0, 0, 0, 0};  // byte offsets of i, j, distance, SIFt, contact type in sorted_slab
    size_t srt_bytes = 0;               // bytes of the five columns
    bool contacts_sorted = false;       // sorted_slab holds the records of the last launch in (i, j) order
    bool packed_csr = false;            // arp_set_packed_layout: the sorted bag's first column is N + 1 row offsets instead of k bgn ids
    bool sorted_is_csr = false;         // ... and that is what sorted_slab holds now
    int64_t gid_max = -1;               // largest global atom id of a shard (-1: not known, 31-bit keys)
    bool pass_pending = false;      // arp_run_enqueue without its arp_run_wait yet
    double pending_cutoff = 5.0, pending_comp = 0.1, pending_expand = 6.0;
    int pending_seq_adj = 0;
    int64_t contacts_expected = 0;   // contacts the previous pass over this structure found (0: none yet): sizes the sift launch
    bool contacts_valid = false;
    double bag_cutoff = 0.0, bag_comp = 0.0;   // of the pass that made the atom-atom bag, and whether everything was selected in it
    bool bag_sel_all = false;
    u64* d_ctr = nullptr;        // C_COUNT device counters
    u64 h_ctr[C_COUNT] = {0};
    int64_t stats[8] = {0, 0, 0, 0, 0, 0, 0, 0};
    int64_t contact_cells = 0;
    bool ctr_clean = false;
    u64 publish_seq = 0;         // number of k_publish_counters launches; the kernel stores it in h_ctr_pinned[C_COUNT]
    bool ctr_zero_ok = false;    // the last arp_run_launch left the whole block zeroed (k_publish_counters) and nothing touched it since
    u64* h_ctr_pinned = nullptr;   // pinned mirror of the counter block + completion word
    PublishArgs pub{nullptr, nullptr, 0, 0};   // in-kernel end-of-pass publication (arp_run_launch sets it for one pass)
    // residue sets of arp_run_launch, tagged with the pass number (never cleared between passes; wrap -> one memset)
    // static candidate lists of the ring / amide loops (k_plane_lists), rebuilt when the structure changes
    DevBuf<int2> plist[4];
    DevBuf<u64> plist_count;       // [4]
    bool plist_count_cleared = false;   // k_point_grids has just zeroed them (same stream, same pass)
    bool lists_dirty = true;
    long long plist_known[4] = {-1, -1, -1, -1};   // entries the lists held at the end of the last pass (-1: not known yet)
    DevBuf<uint8_t> blob_dev;      // device copy of the last arp_set_blob upload (the input arrays are views into it)
    int64_t blob_nbond = 0, blob_nh = 0, blob_nrad = 0;
    bool validate_on_device = false;   // blob uploads: k_prepare_static checks what the classic setters check on the host
    DevBuf<int> blob_sb_nbr;
    uint64_t blob_bytes = 0;       // size of the resident blob (0: the structure came through the classic setters)
    // ---- sharded structures assembled on the device (arp_shard_*)
    DevBuf<uint8_t> rec_home, rec_face[2];
    arp_rec_header rec_home_hdr;
    bool has_rec_home = false;
    DevBuf<int> sh_scan;           // flags / counts and their exclusive scans
    DevBuf<int2> sh_src;
    DevBuf<int8_t> origin, ring_origin, am_origin;
    DevBuf<uint8_t> sh_sel;
    bool shard_resident = false;
    DevBuf<uint8_t> res_tag;       // [0, nres) = selection residues, [nres, 2 nres) = selection_plus residues
    int res_tag_value = 0;
    bool fuse_sets = false;        // the contact-grid build of the current pass also makes the residue / ring / amide sets
    bool init_plus_in_bin = false; // ... and writes selection_plus = selection (whole-structure selection)
    // ---- device-resident result bags of the ring / amide kernels
    Bag bag[BAG_KINDS];
    void void_bags();               // (defined behind the results that go with the bags)
    bool bags_valid() const { bool v = true; for (const Bag& b : bag) v = v && b.valid; return v; }
    DevBuf<uint32_t> bag_perm_big[4];   // ... of a bag beyond BAG_SORT_MAX records (bag_order_large)
    SortScratch sort_bags;                // ... the radix sort's scratch for them
    DevBuf<int> bagsort_i, bagsort_j;
    DevBuf<uint16_t> bagsort_s;
    DevBuf<uint8_t> bagsort_ct;
    DevBuf<uint32_t> bag_perm;     // canonical order of the small ring / amide bags (k_bag_order), BAG_SORT_MAX indices per bag
    DevBuf<uint8_t> bag_pack;      // staging of small bags: device side ...
    uint8_t* bag_stage = nullptr;  // ... and its page-locked host copy
    size_t bag_stage_cap = 0;
    // ---- exchange between shards (arp_comm_*: RCCL on the context's stream)
    ncclComm_t comm = nullptr;
    int comm_rank = 0, comm_world = 1;
    DevBuf<uint8_t> comm_recv[2];          // what the left / right neighbour sent last
    DevBuf<unsigned long long> comm_words; // sizes on their way: [0, 1] out (left, right), [2, 3] in
    DevBuf<int> xl_send[2], xl_recv[2];    // per-pass selection exchange: local atom indices sent to / received from each neighbour
    DevBuf<uint8_t> xl_send_buf[2], xl_recv_buf[2];
    int64_t xl_nsend[2] = {0, 0}, xl_nrecv[2] = {0, 0};
    // ---- several structures in one pass (arp_set_batch): structure s = atoms [atom_off[s], atom_off[s + 1]), rings, amides likewise
    int64_t batch_n = 0;
    std::vector<int64_t> batch_atom_off, batch_ring_off, batch_amide_off;
    std::vector<double> batch_box;       // 6 per structure: lo xyz, hi xyz
    DevBuf<int> sid_atom, sid_ring, sid_amide;
    DevBuf<long long> batch_off_dev;   // the three offset tables of arp_set_batch, one after the other
    // live: a table was uploaded into `place` since the partition was declared — kernels in flight and grids of the running
    // pass may read it, so a refill takes a fresh buffer and the old one is retired (batch_grid_desc)
    struct BatchGrid { double radius = 0; bool valid = false, live = false; DevBuf<BatchPlace> place; GridDesc d{}; } batch_grid[4];
    std::vector<DevBuf<BatchPlace>> batch_retired;   // tables replaced since the last start-over: intact until the next one
    int64_t batch_restarts = 0;        // how often the tables were started over since arp_set_batch (arp_get_stats, stats[7])
    // ---- one topology, several models (arp_set_topology / arp_set_models): the kept topology blob and its ring / amide atoms,
    // and the number of models the resident structure holds (0: no model mode; see inputs_changed)
    DevBuf<uint8_t> topo_dev;
    arp_blob_header topo_hdr{};
    bool has_topo = false;
    DevBuf<int> topo_ring_off, topo_ring_idx, topo_amide_atoms;
    DevBuf<float> models_xyz;
    DevBuf<double> models_box;
    int64_t models_n = 0;
    // ---- the results made on the device from the bags of a pass (DESIGN.md 5e ... 5k).  They share the scratch — none needs it
    // once it is made — and are voided with what they read (void_results)
    SortScratch table_sort;               // the re-keyed records, double-buffered, and the digit tables of their sort
    DevBuf<int> table_tiles, table_rows;  // run detection (arp_runs.h)
    DevBuf<long long> table_total;
    uint8_t* table_stage = nullptr;       // page-locked host side of a fetch's one copy (its first word also receives U)
    size_t table_stage_cap = 0;
    ResultTable persist, respair, respersist;
    FilteredBag filtered;                 // arp_contacts_filter_launch: tile counts and total in table_tiles / table_total
    ResultTable bridges, bridgepersist;   // arp_water_bridges_launch, and arp_models_water_bridge_persistence_launch from its rows
    DevBuf<long long> bridge_off;         // [L + 1] kept pairs per water run, then their exclusive prefix; [L] = rows
    DevBuf<int> bridge_res;               // [L] residue of every sorted leg's partner
    SimilarityResult similarity;          // arp_models_similarity_launch
    ResultTable lifetimes;                // arp_models_lifetimes_launch
    ResultTable networks;                 // arp_networks_launch: the component table ...
    DevBuf<int> net_label, net_scratch;   // ... the label of each of its net_nodes nodes, and the per-node scratch (arp_networks.h)
    int64_t net_nodes = 0;
    ResultTable coupling;                 // arp_models_coupling_launch: features and pairs in one slab; count = kept pairs
    CouplingScratch couple;
    // the ligand-pose family: no bag is read; void_pose_results says what each reads
    PosesPlanesResult pplanes;            // arp_poses_planes_launch; its plane atoms go with the structure, rings or amides
    PosesResult poses;                    // arp_poses_contacts_launch
    PoseFpResult posefp;                  // arp_poses_fingerprints_launch
    ShortlistResult shortlist;            // arp_poses_shortlist_launch
    ClustersResult clusters;              // arp_poses_clusters_launch
    LigandLibrary library;                // arp_set_ligand_library
    LibraryResult libres;                 // arp_library_contacts_launch, arp_library_best_launch
    PoseFpResult libfp;                   // arp_library_fingerprints_launch: P = Q + T rows, the references first
    LibraryFpTables libfpx;               // ... its references, arp_library_fingerprints_best_launch
    LibraryPlaneAtoms libplanes;          // arp_set_ligand_library_planes
    LibraryPlanesResult libpl;            // arp_library_planes_launch
    ShortlistResult libshortlist;         // arp_library_shortlist_launch
    LibClustersResult libclusters;        // arp_library_clusters_launch
    LibBridgesResult libbridges;          // arp_library_water_bridges_launch: reads the library result and the atom-atom bag
    // ---- profiling
    bool profiling = false;
    std::vector<EventPair> ev_pool;
    size_t ev_used = 0;
    double k_ms[NSLOT] = {0};
    int64_t k_launches[NSLOT] = {0};
};
// (the library water bridges read the atom-atom bag as well: they go wherever the bags go, and by void_results)
void arp_ctx::void_bags() {
    for (Bag& b : bag) b.valid = false;
    libbridges.valid = false;
}

namespace {

#define FAIL(ctx, code, msg) do { (ctx)->err = (msg); return (code); } while (0)
#define HIPCHK(ctx, expr)                                                                       \
    do {                                                                                        \
        hipError_t e_ = (expr);                                                                 \
        if (e_ != hipSuccess) {                                                                 \
            (ctx)->err = std::string(#expr) + ": " + hipGetErrorString(e_);                     \
            return ARP_E_HIP;                                                                   \
        }                                                                                       \
    } while (0)
#define CHK(expr) do { int rc_ = (expr); if (rc_ != ARP_OK) return rc_; } while (0)

template <class T>
int upload(arp_ctx* c, DevBuf<T>& buf, const T* src, size_t n) {
    HIPCHK(c, buf.reserve(n ? n : 1));
    if (n) HIPCHK(c, hipMemcpyAsync(buf.p, src, n * sizeof(T), hipMemcpyHostToDevice, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    return ARP_OK;
}
// several uploads of one setter: enqueue them all, synchronise once (upload_done) before the sources go away
template <class T>
int upload_async(arp_ctx* c, DevBuf<T>& buf, const T* src, size_t n) {
    HIPCHK(c, buf.reserve(n ? n : 1));
    if (n) HIPCHK(c, hipMemcpyAsync(buf.p, src, n * sizeof(T), hipMemcpyHostToDevice, c->stream));
    return ARP_OK;
}
int upload_done(arp_ctx* c) {
    HIPCHK(c, hipStreamSynchronize(c->stream));
    return ARP_OK;
}
template <class T>
int download_async(arp_ctx* c, T* dst, const T* src, size_t n) {
    if (n && dst) HIPCHK(c, hipMemcpyAsync(dst, src, n * sizeof(T), hipMemcpyDeviceToHost, c->stream));
    return ARP_OK;
}
template <class T>
int download(arp_ctx* c, T* dst, const T* src, size_t n) {
    if (n && dst) HIPCHK(c, hipMemcpyAsync(dst, src, n * sizeof(T), hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    return ARP_OK;
}

int env_int(const char* name, int dflt) {
    const char* v = getenv(name);
    return (v && *v) ? atoi(v) : dflt;
}

// Every ARP_* switch of this file: read once per process, the first time one is asked for (sw()).  Default, clamp, meaning.
// (arp_json.h reads ARP_EXPORT_THREADS / ARP_EXPORT_MMAP on every call.)
struct Switches {
    // ---- grids
    int deterministic = env_int("ARP_DETERMINISTIC", 0);                        // 1: fixed order inside a cell (k_cellsort), centre grids by the general path
    int chained_scan = env_int("ARP_CHAINED_SCAN", 1);                          // 0: large contact grids scan in two launches, never by k_scan_tiles_chained
    int compact_512_max_rows = env_int("ARP_COMPACT_512_MAX_ROWS", 150000);     // k_compact_atoms: 512 rows per block up to this many atoms, 1024 beyond
    // ---- contact search (k_search)
    int search_blocks = env_int("ARP_SEARCH_BLOCKS", 0);                        // > 0: this many blocks (rounded up to a multiple of 8)
    int search_cpw = std::max(1, env_int("ARP_SEARCH_CPW", 12));                // cells per wave, at most
    int search_tile = env_int("ARP_SEARCH_TILE", -1);                           // -1: tiles of two cells on large grids, 1 / 2: always that tile
    int search_tile_min_cells = env_int("ARP_SEARCH_TILE_MIN_CELLS", 60000);    // ... large: this many cells
    int search_balance = env_int("ARP_SEARCH_BALANCE", -1);                     // blocks split atoms: -1 on sparse / clumped grids, 0 never, 1 always
    int search_apb = std::max(8, env_int("ARP_SEARCH_APB", 128));               // ... atoms per block then
    int balance_hint = env_int("ARP_SEARCH_BALANCE_HINT", 1);                   // 0: no balance hint from the passes before
    int cell_weight_x16 = std::max(0, env_int("ARP_SEARCH_CELL_WEIGHT_X16", 64));   // k_balance_blocks: weight of a cell in sixteenths of an atom
    int balance_hint_atoms = env_int("ARP_SEARCH_BALANCE_HINT_ATOMS", 1);       // 0: no hint for blocks that split atoms (k_balance_atoms)
    int balance_hint_eager = env_int("ARP_SEARCH_BALANCE_HINT_EAGER", 0);       // 1: the hint is made by the first pass over a grid, not the second
    int w_unit = std::max(0, env_int("ARP_SEARCH_W_UNIT", 100));                // k_cell_weights: wave instructions per unit of work,
    int w_chunk = std::max(0, env_int("ARP_SEARCH_W_CHUNK", 85));               // ... per chunk,
    int w_test_x8 = std::max(0, env_int("ARP_SEARCH_W_TEST_X8", 2));            // ... per eight distance tests
    // ---- per-pair kernel (k_sift, k_sift_planes)
    int sift_bpc = env_int("ARP_SIFT_BPC", 0);                                  // > 0: blocks per CU instead of the occupancy arp_create measured
    int sift_ppb = std::max(64, env_int("ARP_SIFT_PPB", 256));                  // pairs per block the launch is sized for
    int64_t stream_out_bytes = (int64_t)env_int("ARP_STREAM_OUT_MB", 96) << 20;  // streaming stores above this many bytes of records
    int sift_shares = env_int("ARP_SIFT_SHARES", 1);                            // 0: equal blocks per pair-list segment, not by the last pass's sizes
    int sift_seg_by_block = env_int("ARP_SIFT_SEG_BY_BLOCK", 0);                // 1: segment by block index even where blocks go round-robin over XCDs
    // ---- ring / amide loops
    int plane_ipw = std::max(1, env_int("ARP_PLANE_IPW", 4));                   // grid walks: rings / amides per wavefront
    int plane_cpw = std::max(1, env_int("ARP_PLANE_CPW", 16));                  // list blocks of a pass: chunks of 64 entries per wave, at most
    double plane_chunk_factor = env_int("ARP_PLANE_CHUNK_FACTOR_X10", 10) / 10.0;   // ... chunks per wave against the sift batches per wave
    int planes_mode = env_int("ARP_PLANES_MODE", 0);                            // 0: the lists in the sift launch, 1: a kernel of their own on the second stream
    int bag_lists = env_int("ARP_BAG_LISTS", 2);                                // arp_*_launch: bit k = loop k from its list, else by its grid walk
    // ---- sorts and fetches
    int sort_small = env_int("ARP_SORT_SMALL", 1);                              // 0: no one-launch sort of a small atom-atom bag (k_sort_small)
    int sort_small_blocks = std::max(1, std::min(64, env_int("ARP_SORT_SMALL_BLOCKS", SORT_SMALL_BLOCKS)));   // ... its blocks
    size_t fetch_direct_max = (size_t)std::max(0, env_int("ARP_FETCH_DIRECT_MAX_KB", 1024)) << 10;   // packed fetches up to this size by a kernel, not the copy engine
    // ---- passes, uploads, waits
    int inkernel_publish = env_int("ARP_INKERNEL_PUBLISH", 1);                  // 0: the counters of a pass by k_publish_counters, not by its last kernel
    int spin_wait = env_int("ARP_SPIN_WAIT", 1);                                // 0: the end of a pass by hipStreamSynchronize, not by polling
    int join_spin_us = env_int("ARP_JOIN_SPIN_US", 25);                         // polling for the upload's lists before a stream wait, microseconds
    int grids_with_upload = env_int("ARP_GRIDS_WITH_UPLOAD", 1);                // 0: centre grids and lists of a blob in its first pass, not with the upload
    int upload_aside = env_int("ARP_UPLOAD_ASIDE", 1);                          // 0: ... with the upload, but on the main stream
    int lists_with_upload = env_int("ARP_LISTS_WITH_UPLOAD", 1);                // 0: only the grids with the upload, the lists in the first pass
    int static_with_upload = env_int("ARP_STATIC_WITH_UPLOAD", 1);              // 0: a blob's static columns in its first pass, not ahead of the verdict
};
const Switches& sw() {
    static const Switches s{};
    return s;
}

inline int nblocks(int64_t work, int threads, int max_blocks = 2048) {
    int64_t b = (work + threads - 1) / threads;
    if (b < 1) b = 1;
    if (b > max_blocks) b = max_blocks;
    return (int)b;
}

struct Prof {  // brackets one launch with events when profiling is on
    arp_ctx* c;
    int slot;
    hipStream_t st;
    EventPair* ep = nullptr;
    Prof(arp_ctx* c_, int slot_, hipStream_t st_ = nullptr) : c(c_), slot(slot_), st(st_ ? st_ : c_->stream) {
        if (!c->profiling) return;
        if (c->ev_pool.capacity() < 256) c->ev_pool.reserve(256);
        if (c->ev_used >= 250) return;
        if (c->ev_used == c->ev_pool.size()) {
            EventPair e{slot, nullptr, nullptr};
            if (hipEventCreate(&e.a) != hipSuccess || hipEventCreate(&e.b) != hipSuccess) return;
            c->ev_pool.push_back(e);
        }
        ep = &c->ev_pool[c->ev_used++];
        ep->slot = slot;
        (void)hipEventRecord(ep->a, st);
    }
    ~Prof() {
        if (ep) (void)hipEventRecord(ep->b, st);
    }
};

void collect_events(arp_ctx* c) {  // call after the pass has ended
    for (size_t k = 0; k < c->ev_used; ++k) {
        float ms = 0;
        (void)hipEventSynchronize(c->ev_pool[k].b);   // the host may have seen the completion word before the last event landed
        if (hipEventElapsedTime(&ms, c->ev_pool[k].a, c->ev_pool[k].b) == hipSuccess) {
            c->k_ms[c->ev_pool[k].slot] += ms;
            c->k_launches[c->ev_pool[k].slot] += 1;
        }
    }
    c->ev_used = 0;
}

int check_launch(arp_ctx* c, const char* what) {
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) {
        c->err = std::string(what) + ": " + hipGetErrorString(e);
        return ARP_E_HIP;
    }
    return ARP_OK;
}

// Choose grid dimensions: cell edge >= radius (slightly larger so that rounding in the
// binning can never separate a pair within the radius by two cells), at most 2^26 cells.
void make_grid_desc(GridDesc& d, const double lo[3], const double hi[3], double radius) {
    double edge = radius * (1.0 + 1e-6);
    if (!(edge > 0)) edge = 1.0;
    for (;;) {
        double nx = std::floor((hi[0] - lo[0]) / edge) + 1, ny = std::floor((hi[1] - lo[1]) / edge) + 1,
               nz = std::floor((hi[2] - lo[2]) / edge) + 1;
        if (nx * ny * nz <= (double)(1 << 26) && nx < 2e9 && ny < 2e9 && nz < 2e9) {
            d.nx = (int)nx; d.ny = (int)ny; d.nz = (int)nz;
            break;
        }
        edge *= 1.26;
    }
    d.ncell = d.nx * d.ny * d.nz;
    d.ox = lo[0]; d.oy = lo[1]; d.oz = lo[2];
    d.inv = 1.0 / edge;
    d.place = nullptr; d.sid_atom = nullptr; d.sid_ring = nullptr; d.sid_amide = nullptr;
}

// The one rule that voids the results made on the device from the bags of a pass (DESIGN.md 5e ... 5k).  `lost` names what was
// refilled, lost or remade: the atom-atom bag, the ring / amide bags, the bridge table, the packed layout.  A result goes when it
// reads any of that, and what is made from it goes with it (it stands behind its source in the list below, which is the one
// statement of what each result reads).  A launch sets its own result valid again.
enum : unsigned { RES_AA = 1u << 0, RES_PLANES = 1u << 1, RES_BRIDGES = 1u << 2, RES_LAYOUT = 1u << 3 };
void void_results(arp_ctx* c, unsigned lost) {
    const unsigned bags = RES_AA | RES_PLANES;
    const struct { bool* valid; unsigned reads, makes; } results[] = {
        {&c->persist.valid, RES_AA, 0},
        {&c->lifetimes.valid, RES_AA, 0},
        {&c->networks.valid, RES_AA, 0},
        {&c->bridges.valid, RES_AA, RES_BRIDGES},
        {&c->bridgepersist.valid, RES_BRIDGES, 0},
        {&c->libbridges.valid, RES_AA, 0},      // (the library water bridges, DESIGN.md 5aa: also a row of void_pose_results)
        {&c->respair.valid, bags, 0},
        {&c->respersist.valid, bags, 0},
        {&c->filtered.valid, bags | RES_LAYOUT, 0},      // (its slab is sized for the four bags packed behind the kept records)
        {&c->similarity.valid, (c->similarity.flags & SIM_BY_RESIDUE) ? bags : RES_AA, 0},      // (the bags of its level)
        {&c->coupling.valid, (c->couple.flags & COUPLE_BY_RESIDUE) ? bags : RES_AA, 0}};       // (the same rule)
    for (const auto& r : results)
        if (r.reads & lost) { *r.valid = false; lost |= r.makes; }
}

// The same rule for the results of the ligand-pose family (DESIGN.md 5o ... 5s), which read no bag: `lost` names what was
// replaced or is about to be — the structure, the selection, or one of the rows below itself.  A row goes when it
// is lost or reads something lost, and what reads it goes with it (it stands behind its source).  The ligand-library result
//  is a row of the same table: it reads the structure and the library (POSE_LIBRARY, lost by
// arp_set_ligand_library) and NO selection; the library fingerprint reads that result's records (made with class
// planes, DESIGN.md 5z: `classes`, the library-planes result's as well, and goes with either), and its best-pose
// table reads the fingerprint; the library-planes result reads the structure, the library and the library's
// plane table (POSE_LIBRARY_PLANE_ATOMS, lost with the library and by arp_set_ligand_library_planes), its per-structure set-up the
// structure alone.  The fingerprint and the
// shortlist read the poses-planes result only when they were made with class planes / with a ring or amide table or weight; the
// clusters read the fingerprint result only while their launch runs, so they stand behind what THAT was made from, not behind it.
// A launch names its own result here before it writes it, and sets it valid again at its end.
enum : unsigned {
    POSE_STRUCTURE = 1u << 0, POSE_SELECTION = 1u << 1, POSE_PLANE_ATOMS = 1u << 2, POSE_MOVABLE = 1u << 3, POSE_CONTACTS = 1u << 4,
    POSE_PLANES = 1u << 5, POSE_FINGERPRINT = 1u << 6, POSE_SHORTLIST = 1u << 7,
    POSE_CLUSTERS = 1u << 8,
    POSE_LIBRARY = 1u << 9,           // the ligand library itself (arp_set_ligand_library)
    POSE_LIBRARY_CONTACTS = 1u << 10, POSE_LIBRARY_BEST = 1u << 11,
    POSE_LIBRARY_FINGERPRINT = 1u << 12, POSE_LIBRARY_FP_BEST = 1u << 13,
    POSE_LIBRARY_PLANE_ATOMS = 1u << 14,      // the library's plane table (arp_set_ligand_library_planes)
    POSE_LIBRARY_PLANES_SETUP = 1u << 15, POSE_LIBRARY_PLANES = 1u << 16,
    POSE_LIBRARY_SHORTLIST = 1u << 17,
    POSE_LIBRARY_CLUSTERS = 1u << 18,
    POSE_LIBRARY_BRIDGES = 1u << 19
};
void void_pose_results(arp_ctx* c, unsigned lost) {
    const unsigned inputs = POSE_STRUCTURE | POSE_SELECTION;
    const struct { bool* valid; unsigned is, reads; } results[] = {
        {&c->pplanes.have_atoms, POSE_PLANE_ATOMS, POSE_STRUCTURE},
        {&c->pplanes.setup, POSE_MOVABLE, inputs | POSE_PLANE_ATOMS},      // (the movable set's tables of the poses-planes result)
        {&c->pplanes.valid, POSE_PLANES, POSE_MOVABLE},
        {&c->poses.valid, POSE_CONTACTS, inputs},       // (its movable tables go by static_epoch / sel_epoch)
        {&c->posefp.valid, POSE_FINGERPRINT, POSE_CONTACTS | (c->posefp.classes ? POSE_PLANES : 0u)},
        {&c->shortlist.valid, POSE_SHORTLIST, POSE_CONTACTS | (c->shortlist.planes ? POSE_PLANES : 0u)},
        {&c->clusters.valid, POSE_CLUSTERS, POSE_CONTACTS | (c->clusters.classes ? POSE_PLANES : 0u)},
        // the library result reads the structure and the library, no selection; the best-pose table reads its summary
        {&c->libres.valid, POSE_LIBRARY_CONTACTS, POSE_STRUCTURE | POSE_LIBRARY},
        {&c->libres.best_valid, POSE_LIBRARY_BEST, POSE_LIBRARY_CONTACTS},
        // the library's plane table names atoms of the library's ligands; the set-up of the library-planes result (grid, residue
        // CSR) reads the structure alone; the result reads the structure, the library and the plane table, and no selection
        {&c->libplanes.resident, POSE_LIBRARY_PLANE_ATOMS, POSE_LIBRARY},
        {&c->libpl.setup, POSE_LIBRARY_PLANES_SETUP, POSE_STRUCTURE},
        {&c->libpl.valid, POSE_LIBRARY_PLANES, POSE_STRUCTURE | POSE_LIBRARY | POSE_LIBRARY_PLANE_ATOMS},
        // the library fingerprint reads the library result's records and, made with class planes, the
        // library-planes result's (so its row stands behind that one's); its best-pose table reads its count and cross
        {&c->libfp.valid, POSE_LIBRARY_FINGERPRINT, POSE_LIBRARY_CONTACTS | (c->libfp.classes ? POSE_LIBRARY_PLANES : 0u)},
        {&c->libfpx.best_valid, POSE_LIBRARY_FP_BEST, POSE_LIBRARY_FINGERPRINT},
        // the library shortlist reads the library result and, made with a ring or amide table or weight, the
        // library-planes result; the library fingerprint only while its launch runs (scores are taken then)
        {&c->libshortlist.valid, POSE_LIBRARY_SHORTLIST, POSE_LIBRARY_CONTACTS | (c->libshortlist.planes ? POSE_LIBRARY_PLANES : 0u)},
        // the library clusters read the library result (lig_of, T); the library fingerprint and the library
        // shortlist only while their launch runs, so they stand behind the library result alone
        {&c->libclusters.valid, POSE_LIBRARY_CLUSTERS, POSE_LIBRARY_CONTACTS},
        // the library water bridges read the library result's records; and the atom-atom bag of the receptor's
        // pass, by which they are a row of void_results as well
        {&c->libbridges.valid, POSE_LIBRARY_BRIDGES, POSE_LIBRARY_CONTACTS}};
    for (const auto& r : results)
        if ((r.is | r.reads) & lost) { *r.valid = false; lost |= r.is; }
}

// What a caller can replace, for inputs_changed.  IN_BATCH_GRIDS is no input: batch_grid_desc started the grid tables of the
// batch over (every slot held another radius; arp_get_stats counts it in stats[7]).
enum : unsigned {
    IN_ATOMS = 1u << 0, IN_RESIDUES = 1u << 1, IN_BONDS = 1u << 2, IN_HYDROGENS = 1u << 3,
    IN_NEIGHBOURS = 1u << 4,        // single-bond neighbours: indices or coordinates
    IN_RINGS = 1u << 5, IN_AMIDES = 1u << 6, IN_OWNERSHIP = 1u << 7, IN_GROUP_OWNERSHIP = 1u << 8,
    IN_SELECTION = 1u << 9, IN_SELECTION_STATE = 1u << 10, IN_BATCH = 1u << 11, IN_WHOLE_STRUCTURE = 1u << 12,
    IN_EVERYTHING = (1u << 13) - 1,   // a new structure: blob upload, shard assembly, an upload abandoned
    IN_BATCH_GRIDS = 1u << 13,
};

// The one place that marks derived state stale because an input changed; whoever builds an artefact sets it valid again.
//
//   input                  static  lists  contact  all-atom  centre  batch  selection  default    results  model  pose     plane
//                          columns        grid     grid      grids                     selection           mode   results  atoms
//   atoms                  x       x      x        x         (b)     x      x          x          x        x      x        x
//   residues               x       x      x        x                        x                     x        x      x        x
//   bonds, hydrogens       x       x                                                              x        x      x        x
//   single-bond nbrs       x       x                                                              x        x      x        x
//   rings / amides         x       x                         own(b)  x      x                     x        x      x        x
//   ownership              x       x      x        x         (b)     x                            x        x      x        x
//   group ownership        x       x                         (b)     x                            x        x      x        x
//   selection                                      x                        x                     x               x
//   selection state        x (s)   x      x        x                        x                     x               x
//   batch                  x       x      x        x         x       x                            x        x      x        x
//   whole structure                                                                               x               x
//   batch grid tables      x (k)   x      x        x         x                                    (no input)
//   models                 as a blob upload (everything), then as a batch; model mode begins after both      (m)
//
// static columns: k_prepare_static's records and their spatial order; the contact count of the last pass that sizes the sift
//   launch goes with them, and so does sp_keep_base, the kept rows before every block of a whole-structure grid build
//   (k_keep_bases: hydrogen flags and the order, no selection; a new order for resident columns voids it as well: its epoch).  The lists are made beside them (from the centre grids and the atoms as uploaded), so whatever
//   stales the columns stales the lists at the same moment.
// (s) the static columns read no selection; a staged shard pass recomposes them all the same (a change of that is a change of
//   the kernels the staged path launches).  (k) the same structure in new grid tables keeps its contact count.
// batch grid tables: a start-over can come in the MIDDLE of a pass — at any of its up to three radii: the order of the static
//   columns (cutoff), the all-atom grid of the expansion, the centre grids (6 A), the last also on the second stream — behind
//   kernels of that pass which read a table and in front of launches that use a grid built from one.  That is safe because no
//   table is overwritten: the old ones are retired intact (batch_grid_desc), so what was built earlier in the pass stays
//   usable to its end, and the marks set here only make the NEXT user rebuild (the columns again inside the same pass, when
//   the expansion's grid build asks ensure_static: the same layout from a new table, the same records).  A placement is a
//   pure function of the boxes and the radius (arp_batchgrid.h), so a rebuilt table equals the retired one.
// contact grid: what atom_grid was built from; the whole-structure reuse also checks its GridKey.  all-atom grid: M_SEL is in
//   its records.
// centre grids: a ring / amide upload voids its own grid; (b) both, when a batch partition was in force: they were built in
//   its layout.  A reset with no partition in force voids none (the shard path sets ownership over grids made with the upload).
// batch: the partition was declared for the arrays that were resident then (arp_set_batch again after the change); its grid
//   tables go with it.  arp_set_batch records the new partition after this call.
// selection: selection_plus and the sets are made again (sel_made, sel_epoch).  default selection: a new structure starts
//   with everything selected (I:1395) and no whole-structure assertion.
// results: the atom-atom bag and the four ring / amide bags of the last pass; the fetches refuse until the next launch.  What
//   is made from them on the device goes with them by the one rule of void_results.
// pose results: the poses result, the poses-planes result with its movable set-up, the fingerprint, the shortlist and the
//   clusters read the structure and the selection, no bag; plane atoms (arp_set_plane_atoms) name atoms of the structure and
//   stay through a new selection.  void_pose_results is the one statement of what each of them reads.
// model mode: the resident structure is the F models of the kept topology (arp_models_planes answers); any other structure
//   input ends it — a blob, a setter, a batch — while a selection keeps it.  (m) arp_set_models uploads and validates the
//   expanded blob (IN_EVERYTHING), declares the partition (IN_BATCH) and then writes the ring residues of every model, which
//   nothing made so far reads: the all-atom grid it builds for them holds atoms and residue ids only.  The kept topology is
//   no derived state: only arp_set_topology replaces it.
void inputs_changed(arp_ctx* c, unsigned what) {
    const unsigned columns = IN_EVERYTHING & ~(IN_SELECTION | IN_WHOLE_STRUCTURE);
    const unsigned partition = IN_ATOMS | IN_RINGS | IN_AMIDES | IN_OWNERSHIP | IN_GROUP_OWNERSHIP | IN_BATCH;
    const unsigned layout = IN_BATCH | IN_BATCH_GRIDS;
    const unsigned structure = IN_EVERYTHING & ~(IN_SELECTION | IN_SELECTION_STATE | IN_WHOLE_STRUCTURE);
    if (what & (columns | IN_BATCH_GRIDS)) { c->static_dirty = c->lists_dirty = true; c->sp_keep_epoch = 0; }
    if (what & columns) c->contacts_expected = 0;
    if (what & (IN_ATOMS | IN_RESIDUES | IN_OWNERSHIP | IN_SELECTION_STATE | layout)) c->atom_grid.valid = false;
    if (what & (IN_ATOMS | IN_RESIDUES | IN_OWNERSHIP | IN_SELECTION | IN_SELECTION_STATE | layout)) c->all_grid_current = false;
    const bool relaid = (what & layout) || ((what & partition) && c->batch_n > 0);
    if (relaid || (what & IN_RINGS)) c->ring_grid.valid = false;
    if (relaid || (what & IN_AMIDES)) c->amide_grid.valid = false;
    if (what & partition) {
        c->batch_n = 0;
        for (auto& g : c->batch_grid) g.valid = false;
    }
    if (what & (IN_ATOMS | IN_RESIDUES | IN_RINGS | IN_AMIDES | IN_SELECTION | IN_SELECTION_STATE)) {
        c->sel_made = false;
        ++c->sel_epoch;
    }
    if (what & IN_ATOMS) {
        c->sel_uploaded = c->sel_prefilled = c->sel_all = c->whole_structure = false;
        c->nsel = -1;
    }
    if (what & structure) c->models_n = 0;
    if (what & IN_EVERYTHING) {
        c->contacts_valid = false;
        void_results(c, RES_AA | RES_PLANES);
        c->void_bags();
    }
    void_pose_results(c, ((what & structure) ? POSE_STRUCTURE : 0u) | ((what & IN_EVERYTHING & ~structure) ? POSE_SELECTION : 0u));
}

// Several structures in one grid (arp_set_batch): the placement of arp_batchgrid.h (batch_layout), cached per radius in four
// slots; this function keeps the cache and uploads the table.
//
// Nothing is ever copied into a table that something may still read.  A pass asks for up to three radii (cutoff, expansion,
// 6 A for the centre grids) and enqueues kernels that read a table through GridDesc::place before it asks for the next one,
// and the context's streams do not wait for a blocking copy; so a slot whose buffer has held a table since the partition was
// declared (live) is refilled into a FRESH buffer and the old one is retired, intact.  When every slot holds another radius
// the tables start over: all slots become free and whatever was built in the old tables is marked stale
// (inputs_changed(IN_BATCH_GRIDS)) — for the NEXT user: a grid or an order built earlier in the running pass keeps reading
// its retired table to the end of that pass.  The buffers a start-over retired are freed by the next start-over, after both
// streams have drained, or by arp_set_batch, which has waited for the stream.
void release_batch_tables(arp_ctx* c) {      // (the caller knows that nothing in flight reads them)
    for (auto& b : c->batch_retired) b.release();
    c->batch_retired.clear();
    for (auto& g : c->batch_grid) g.live = false;      // (their buffers are reused in place)
}
int batch_grid_desc(arp_ctx* c, GridDesc& d, double radius) {
    arp_ctx::BatchGrid* slot = nullptr;
    for (auto& g : c->batch_grid)
        if (g.valid && g.radius == radius) { d = g.d; return ARP_OK; }
    for (auto& g : c->batch_grid)
        if (!g.valid) { slot = &g; break; }
    if (!slot) {   // every slot holds another radius: start over (grids built with the old tables are rebuilt by their next user)
        if (!c->batch_retired.empty()) {
            HIPCHK(c, hipStreamSynchronize(c->stream));
            if (c->stream2) HIPCHK(c, hipStreamSynchronize(c->stream2));
            for (auto& b : c->batch_retired) b.release();
            c->batch_retired.clear();
        }
        for (auto& g : c->batch_grid) g.valid = false;
        slot = &c->batch_grid[0];
        ++c->batch_restarts;
        inputs_changed(c, IN_BATCH_GRIDS);
    }
    const int64_t B = c->batch_n;
    std::vector<BatchPlace> pl((size_t)B);
    int dims[3] = {1, 1, 1};
    const double edge = batch_layout(B, c->batch_box.data(), radius, pl.data(), dims);
    if (slot->live) {
        c->batch_retired.push_back(slot->place);
        slot->place = DevBuf<BatchPlace>{};
        slot->live = false;
    }
    HIPCHK(c, slot->place.reserve((size_t)B));
    HIPCHK(c, hipMemcpy(slot->place.p, pl.data(), (size_t)B * sizeof(BatchPlace), hipMemcpyHostToDevice));   // (a buffer nothing reads)
    slot->live = true;
    GridDesc g{};
    g.nx = dims[0]; g.ny = dims[1]; g.nz = dims[2]; g.ncell = dims[0] * dims[1] * dims[2];
    g.ox = c->lo[0]; g.oy = c->lo[1]; g.oz = c->lo[2];   // (not used for binning: every structure has its own origin)
    g.inv = 1.0 / edge;
    g.place = slot->place.p; g.sid_atom = c->sid_atom.p; g.sid_ring = c->sid_ring.p; g.sid_amide = c->sid_amide.p;
    slot->d = g; slot->radius = radius; slot->valid = true;
    d = g;
    return ARP_OK;
}
// the grid of a pass over the resident structure(s)
int grid_desc_for(arp_ctx* c, GridDesc& d, const double lo[3], const double hi[3], double radius) {
    if (c->batch_n > 0) return batch_grid_desc(c, d, radius);
    make_grid_desc(d, lo, hi, radius);
    return ARP_OK;
}

// Exclusive scan of a cell histogram (in place when in == out): out[ncell] = the total, also written to *total_out if given.
// The one choice of kernels for every grid: ONE 1024-thread block up to 32768 cells; above that tiles of 16384 counters and a
// fix-up, two launches (a 1 M-atom contact grid has 10 tiles; their totals go to sums).  The caller brackets it with Prof.
int enqueue_scan(arp_ctx* c, hipStream_t st, const int* in, int ncell, int* out, DevBuf<int>& sums, u64* total_out = nullptr) {
    if (ncell > 32768) {
        const int ntiles = (ncell + TILE_CELLS - 1) / TILE_CELLS;
        HIPCHK(c, sums.reserve((size_t)ntiles + 2));
        hipLaunchKernelGGL(k_scan_tiles, dim3(ntiles), dim3(1024), 0, st, in, ncell, out, sums.p);
        hipLaunchKernelGGL(k_scan_fix, dim3((ncell + 4095) / 4096), dim3(1024), 0, st, out, ncell, sums.p, ntiles, total_out);
    } else if (in != out) {
        if (ncell <= 4096) hipLaunchKernelGGL((k_scan_small<4>), dim3(1), dim3(1024), 0, st, in, ncell, out, total_out);
        else if (ncell <= 16384) hipLaunchKernelGGL((k_scan_small<16>), dim3(1), dim3(1024), 0, st, in, ncell, out, total_out);
        else hipLaunchKernelGGL((k_scan_small<32>), dim3(1), dim3(1024), 0, st, in, ncell, out, total_out);
    } else {      // (no total_out in place)
        if (ncell <= 4096) hipLaunchKernelGGL((k_scan_inplace<4>), dim3(1), dim3(1024), 0, st, out, ncell);
        else if (ncell <= 16384) hipLaunchKernelGGL((k_scan_inplace<16>), dim3(1), dim3(1024), 0, st, out, ncell);
        else hipLaunchKernelGGL((k_scan_inplace<32>), dim3(1), dim3(1024), 0, st, out, ncell);
    }
    return check_launch(c, "k_scan");
}

// the scans read / write whole int4s and whole tiles: histogram and start table are padded to a tile multiple
size_t scan_padded(int ncell) {
    return std::max<size_t>(((size_t)ncell / TILE_CELLS + 1) * TILE_CELLS + 8, 65536 + 8);
}

// grid buffers sized for the current descriptor; the histogram is zero on entry (see below)
int reserve_grid(arp_ctx* c, Grid& G, int n, hipStream_t st = nullptr) {
    if (!st) st = c->stream;
    const int ncell = G.d.ncell;
    HIPCHK(c, G.cell_of.reserve((size_t)std::max(n, 1)));
    HIPCHK(c, G.perm.reserve((size_t)std::max(n, 1)));
    {   // k_scatter's atomicSub takes every counter back to 0, so only a fresh allocation needs clearing
        bool fresh = false;
        HIPCHK(c, G.cnt.reserve(scan_padded(ncell), &fresh));
        if (fresh) HIPCHK(c, hipMemsetAsync(G.cnt.p, 0, G.cnt.cap * sizeof(int), st));
    }
    HIPCHK(c, G.start.reserve(scan_padded(ncell)));
    HIPCHK(c, G.sums.reserve((size_t)(ncell + TILE_CELLS - 1) / TILE_CELLS + 2));
    return ARP_OK;
}

// bin + scan + scatter (+ optional cell sort) for rings / amides.  P = point accessor.
template <class P>
int build_grid(arp_ctx* c, Grid& G, P pts, int n, const double lo[3], const double hi[3], double radius, const int* sid) {
    CHK(grid_desc_for(c, G.d, lo, hi, radius));
    G.radius = radius;
    G.n_points = n;
    const int ncell = G.d.ncell;
    CHK(reserve_grid(c, G, n));
    {
        Prof p(c, SLOT_BIN);
        if (n > 0) {
            hipLaunchKernelGGL((k_bin<P>), dim3(nblocks(n, 256)), dim3(256), 0, c->stream, pts, n, G.d, sid, G.cell_of.p, G.cnt.p);
            CHK(check_launch(c, "k_bin"));
        }
    }
    {
        Prof p(c, SLOT_SCAN);
        CHK(enqueue_scan(c, c->stream, G.cnt.p, ncell, G.start.p, G.sums));
    }
    {
        Prof p(c, SLOT_SCATTER);
        if (n > 0) {
            hipLaunchKernelGGL(k_scatter, dim3(nblocks(n, 256)), dim3(256), 0, c->stream, n, G.cell_of.p, G.start.p, G.cnt.p, G.perm.p);
            // The order inside a cell does not change any result set (pairs are oriented by packed
            // id and callers sort); ARP_DETERMINISTIC=1 additionally fixes the device-side order.
            if (sw().deterministic)
                hipLaunchKernelGGL(k_cellsort, dim3(nblocks(ncell, 256)), dim3(256), 0, c->stream, ncell, G.start.p, G.perm.p);
            CHK(check_launch(c, "k_scatter/k_cellsort"));
        }
    }
    G.valid = true;
    return ARP_OK;
}

// The main stream waits for the grids / lists the last arp_set_blob left to the second stream (no-op when nothing is pending)
// (Inside a pass — uplists_defer — the callers that only prepare arguments ask without waiting: the one reader of the lists is the
// last launch of the pass, enqueue_contacts joins in front of it, and by then the event has usually fired: no wait on the stream,
// which would cost the main stream ~6 us between two of its kernels.)
int join_upload_lists(arp_ctx* c, bool must = false) {
    if (!c->uplists_pending) return ARP_OK;
    if (hipEventQuery(c->ev_uplists) == hipSuccess) { c->uplists_pending = false; return ARP_OK; }
    (void)hipGetLastError();      // (hipErrorNotReady is not an error)
    if (c->uplists_defer && !must) return ARP_OK;
    if (c->uplists_defer) {
        // In front of the last launch of a pass: the host is tens of microseconds ahead of the device there (grid build and search
        // are queued), the lists a few short of done — asking again for a little while costs the device nothing, a wait on the
        // stream costs it ~6 us between search and per-pair kernel.
        const auto t0 = std::chrono::steady_clock::now();
        while (std::chrono::duration<double, std::micro>(std::chrono::steady_clock::now() - t0).count() < sw().join_spin_us) {
            if (hipEventQuery(c->ev_uplists) == hipSuccess) { c->uplists_pending = false; return ARP_OK; }
            (void)hipGetLastError();
        }
    }
    c->uplists_pending = false;
    HIPCHK(c, hipStreamWaitEvent(c->stream, c->ev_uplists, 0));
    return ARP_OK;
}

// Selection-independent part of every atom record (rebuilt only when an input changed) and its SPATIAL ORDER: the rows sorted
// by cell of the grid with cell edge `radius` (counting sort, x fastest), which a pass with that cell edge compacts into its
// contact grid in one launch (k_compact_atoms).  radius = 0: any order will do (the one that exists, 6 A when there is none).
inline int compact_rows(int n) { return n <= sw().compact_512_max_rows ? 512 : 1024; }      // rows per block of k_compact_atoms
int ensure_static(arp_ctx* c, double radius = 0.0) {
    if (radius <= 0) radius = c->sp_radius > 0 ? c->sp_radius : 6.0;
    const bool columns = c->static_dirty;
    if (!columns && c->sp_radius == radius) return ARP_OK;
    const int n = (int)c->n;
    if (columns) {
        HIPCHK(c, c->st_qa.reserve((size_t)std::max(n, 1)));
        HIPCHK(c, c->st_h.reserve((size_t)std::max(n, 1)));
        HIPCHK(c, c->st_aux.reserve((size_t)std::max(n, 1)));
        HIPCHK(c, c->st_xyzm.reserve((size_t)std::max(n, 1)));
    }
    RawAtoms r;
    r.xyz = c->xyz.p; r.tmask = c->tmask.p; r.flags = c->flags.p; r.res_id = c->res_id.p;
    r.res_flags = c->has_res ? c->res_flags.p : nullptr;
    r.res_prev = c->has_res ? c->res_prev.p : nullptr;
    r.res_next = c->has_res ? c->res_next.p : nullptr;
    r.home = c->has_home ? c->home.p : nullptr;
    r.rad = c->rad.p; r.rad_idx = c->rad_idx.p; r.h_off = c->h_off.p; r.bond_off = c->bond_off.p; r.bond_idx = c->bond_idx.p; r.sb = c->sb.p;
    if (n > 0) {
        // counting sort by cell.  The longest-bond words sit behind the histogram, so ONE fill clears both.
        GridDesc d;
        CHK(grid_desc_for(c, d, c->lo, c->hi, radius));
        HIPCHK(c, c->sp_xyzm.reserve((size_t)n)); HIPCHK(c, c->sp_aux.reserve((size_t)n)); HIPCHK(c, c->sp_qa.reserve((size_t)n)); HIPCHK(c, c->sp_h.reserve((size_t)n));
        HIPCHK(c, c->sp_cr.reserve((size_t)n)); HIPCHK(c, c->sp_cell.reserve((size_t)n));
        // layout of sp_cnt: [longest bond, longest atom - hydrogen distance, 2 words of padding | histogram of ncell + 1 cells]:
        // a fresh structure clears all of it with ONE fill, a new order for resident columns only the histogram
        float keep_longest[2] = {0.0f, 0.0f};
        // (the one-block scan reads and writes whole int4s up to its 32768 slots; the tiled one of larger grids whole tiles)
        const size_t want = std::max<size_t>(d.ncell > 32768 ? scan_padded(d.ncell) + 8 : (size_t)d.ncell + 8, 32768 + 8);
        const bool regrow = !columns && c->sp_cnt.cap < want;
        if (regrow) {      // (a larger grid for resident columns: the two words survive the reallocation through the host)
            HIPCHK(c, hipMemcpyAsync(keep_longest, c->sp_cnt.p, sizeof(keep_longest), hipMemcpyDeviceToHost, c->stream));
            HIPCHK(c, hipStreamSynchronize(c->stream));
        }
        const bool cleared = c->sp_cnt.cap >= want && c->sp_cnt_zeroed >= want;      // (arp_set_blob did, while it waited for the validation)
        c->sp_cnt_zeroed = 0;
        HIPCHK(c, c->sp_cnt.reserve(want));
        int* const hist = c->sp_cnt.p + 4;
        c->longest_bond.borrow(c->sp_cnt.p, 2);
        if (columns) {
            if (!cleared) HIPCHK(c, hipMemsetAsync(c->sp_cnt.p, 0, want * sizeof(int), c->stream));
            hipLaunchKernelGGL(k_prepare_static, dim3(nblocks(n, 256)), dim3(256), 0, c->stream, r, n, c->st_xyzm.p, c->st_aux.p, c->st_qa.p, c->st_h.p,
                               d, hist, c->sp_cr.p, c->h_xyz_d.p, (unsigned int*)c->longest_bond.p,
                               c->ahead_seq ? (const int*)c->upload_bad.p : (const int*)nullptr, c->ahead_seq);
        } else {
            if (regrow) HIPCHK(c, hipMemcpyAsync(c->sp_cnt.p, keep_longest, sizeof(keep_longest), hipMemcpyHostToDevice, c->stream));
            HIPCHK(c, hipMemsetAsync(hist, 0, ((size_t)d.ncell + 4) * sizeof(int), c->stream));
            hipLaunchKernelGGL(k_static_bin, dim3(nblocks(n, 256)), dim3(256), 0, c->stream, n, c->st_xyzm.p, d, hist, c->sp_cr.p);
        }
        CHK(check_launch(c, "k_prepare_static"));
        // (larger grids — a batch of structures side by side: 10^6 cells — by tiles: one block walking them with a running carry
        // was 177 us of a 64-structure batch's first pass)
        CHK(enqueue_scan(c, c->stream, hist, d.ncell, hist, c->sp_sums));
        hipLaunchKernelGGL(k_static_permute, dim3(nblocks(n, 256)), dim3(256), 0, c->stream, n, c->sp_cr.p, hist, c->st_xyzm.p,
                           c->st_aux.p, c->st_qa.p, c->st_h.p, c->sp_xyzm.p, c->sp_aux.p, c->sp_qa.p, c->sp_h.p, c->sp_cell.p,
                           c->ahead_seq ? (const int*)c->upload_bad.p : (const int*)nullptr, c->ahead_seq);
        CHK(check_launch(c, "k_static_permute"));
        c->sp_grid = d;
    }
    else {      // no atoms: nothing to order; the two longest-distance words still exist (zero)
        c->sp_cnt_zeroed = 0;
        HIPCHK(c, c->sp_cnt.reserve(8));
        HIPCHK(c, hipMemsetAsync(c->sp_cnt.p, 0, 8 * sizeof(int), c->stream));
        c->longest_bond.borrow(c->sp_cnt.p, 2);
    }
    c->sp_radius = radius;
    c->static_dirty = false;
    ++c->static_epoch;      // (whatever was derived from the old columns or their order is stale)
    return ARP_OK;
}
// sp_keep_base of the spatial order in place (k_keep_bases: one launch on the main stream, once per order).  Not made with the
// order itself: there it was 2.8 us of every structure's first pass (0.1034 -> 0.1062 ms at 100 k atoms), and a structure that is
// evaluated once, or whose passes keep their grid, never reads it.  The second whole-structure grid build over an order makes it
// (enqueue_contacts), as the search's hint is worked out by the second pass over a grid.
int make_keep_bases(arp_ctx* c) {
    const int n = (int)c->n;
    const int rows = compact_rows(n), nb = (n + rows - 1) / rows;
    bool fresh = false;
    HIPCHK(c, c->sp_keep.reserve(4 + 2 * (size_t)nb + 1, &fresh));
    if (fresh) HIPCHK(c, hipMemsetAsync(c->sp_keep.p, 0, 4 * sizeof(int), c->stream));      // (the ticket: every launch leaves it zero)
    int* const cnt = c->sp_keep.p + 4;
    if (rows == 512) hipLaunchKernelGGL(k_keep_bases<512>, dim3(nb), dim3(256), 0, c->stream, n, c->sp_xyzm.p, cnt, cnt + nb, (unsigned int*)c->sp_keep.p);
    else hipLaunchKernelGGL(k_keep_bases<1024>, dim3(nb), dim3(256), 0, c->stream, n, c->sp_xyzm.p, cnt, cnt + nb, (unsigned int*)c->sp_keep.p);
    CHK(check_launch(c, "k_keep_bases"));
    c->sp_keep_rows = rows; c->sp_keep_blocks = nb;
    c->sp_keep_epoch = c->static_epoch;
    return ARP_OK;
}

StaticAtoms static_atoms(arp_ctx* c) {
    StaticAtoms r;
    r.xyzm = c->sp_xyzm.p;
    r.qa = c->sp_qa.p;
    r.hoff = c->sp_h.p;
    r.aux = c->sp_aux.p;
    r.sel = c->sel_made ? c->sel.p : nullptr;
    r.plus = c->sel_made ? c->plus.p : nullptr;
    r.all = (c->sel_made && c->sel_all) ? 1 : 0;
    return r;
}

// k_scan_scatter_atoms<S> for steps = S chunks of 16 x 256 cells of the start table in LDS (1 ... 9).  (The deduced return type
// instantiates the chain where it is called, in the order S = 1 ... 9: the kernels keep their places in the code object.)
template <int S = 1, class... Args>
auto launch_scan_scatter(int steps, dim3 grid, hipStream_t st, Args... args) {
    if (S == 9 || steps <= S) {
        hipLaunchKernelGGL((k_scan_scatter_atoms<S>), grid, dim3(1024), S * 16384, st, args...);
        return;
    }
    if constexpr (S < 9) launch_scan_scatter<S + 1>(steps, grid, st, args...);
}

// Grid over the atoms selected by the (req, forb) meta masks (or an explicit mask): three launches —
// k_bin_atoms (records composed on the fly), scan, k_scatter_atoms (writes the cell-sorted search and
// sift records directly).
int build_atom_grid(arp_ctx* c, Grid& G, DevBuf<float4>& sx, DevBuf<int4>& sa, DevBuf<int4>* srec, double radius,
                    uint32_t req, uint32_t forb, const uint8_t* active, u64* total_out = nullptr, uint8_t* plus_init = nullptr,
                    hipStream_t st = nullptr, ResMarks rm = ResMarks{nullptr, nullptr, 0}, GroupMasks gm = GroupMasks{}, bool world = false) {
    if (!st) st = c->stream;
    const int n = (int)c->n;
    // world: one grid over the box of ALL resident atoms in their own coordinates, whatever the partition (build_world_grid)
    if (world) make_grid_desc(G.d, c->lo, c->hi, radius);
    else CHK(grid_desc_for(c, G.d, c->lo, c->hi, radius));
    G.radius = radius;
    G.n_points = n;
    const int ncell = G.d.ncell;
    HIPCHK(c, G.cell_rank.reserve((size_t)std::max(n, 1)));
    {   // both histograms: zero when freshly allocated; afterwards each build clears the other one
        bool f0 = false, f1 = false;
        HIPCHK(c, G.cnt.reserve(scan_padded(ncell), &f0));
        HIPCHK(c, G.cnt2.reserve(scan_padded(ncell), &f1));
        if (f0) { HIPCHK(c, hipMemsetAsync(G.cnt.p, 0, G.cnt.cap * sizeof(int), st)); G.used[0] = 0; }
        if (f1) { HIPCHK(c, hipMemsetAsync(G.cnt2.p, 0, G.cnt2.cap * sizeof(int), st)); G.used[1] = 0; }
    }
    HIPCHK(c, G.start.reserve(scan_padded(ncell)));
    HIPCHK(c, G.sums.reserve((size_t)(ncell + TILE_CELLS - 1) / TILE_CELLS + 2));
    HIPCHK(c, sx.reserve((size_t)std::max(n, 1)));
    HIPCHK(c, sa.reserve((size_t)std::max(n, 1)));
    if (srec) { HIPCHK(c, srec->reserve((size_t)std::max(n, 1))); HIPCHK(c, c->s_h.reserve((size_t)std::max(n, 1))); }
    CHK(ensure_static(c));
    const StaticAtoms r = static_atoms(c);
    int* const hist = G.cur ? G.cnt2.p : G.cnt.p;
    int* const other = G.cur ? G.cnt.p : G.cnt2.p;
    if (n > 0) {
        {
            Prof p(c, SLOT_BIN, st);
            const int nzero = (int)G.used[1 - G.cur];
            if (active) hipLaunchKernelGGL((k_bin_atoms<1>), dim3(nblocks(n, 256)), dim3(256), 0, st, r, n, G.d, active, 0u, 0u, G.cell_rank.p, hist, plus_init, other, nzero, rm);
            else hipLaunchKernelGGL((k_bin_atoms<2>), dim3(nblocks(n, 256)), dim3(256), 0, st, r, n, G.d, (const uint8_t*)nullptr, req, forb, G.cell_rank.p, hist, plus_init, other, nzero, rm);
            CHK(check_launch(c, "k_bin_atoms"));
            G.used[1 - G.cur] = 0;
            G.used[G.cur] = ((size_t)ncell + 3) & ~(size_t)3;
        }
        int4* const rec = srec ? srec->p : (int4*)nullptr;
        const int nb = (n + SCAT_ATOMS - 1) / SCAT_ATOMS;
        if (ncell <= SCAN_LDS_CELLS) {   // start table in LDS: scan + scatter in one launch
            Prof p(c, SLOT_SCATTER, st);
            const int steps = (ncell + 16 * 256 - 1) / (16 * 256);
            launch_scan_scatter(steps, dim3(nb), st, r, n, ncell, G.cell_rank.p, hist, G.start.p, total_out, sx.p, sa.p, rec, c->s_h.p, gm);
            CHK(check_launch(c, "k_scan_scatter_atoms"));
        } else {
            {
                Prof p(c, SLOT_SCAN, st);
                const int ntiles = (ncell + TILE_CELLS - 1) / TILE_CELLS;
                if (sw().chained_scan && ntiles <= CHAIN_TILES && ntiles <= 2 * c->num_cu) {   // one launch: the tiles hand their totals on themselves (all resident at once)
                    bool fresh = false;
                    HIPCHK(c, G.chain.reserve(CHAIN_TILES, &fresh));
                    if (fresh || G.chain_epoch == 0xFFFFFFFFu) {   // new buffer, or the launch number wraps: no stale word may match a future one
                        HIPCHK(c, hipMemsetAsync(G.chain.p, 0, G.chain.cap * sizeof(unsigned long long), st));
                        G.chain_epoch = 0;
                    }
                    ++G.chain_epoch;
                    hipLaunchKernelGGL(k_scan_tiles_chained, dim3(ntiles), dim3(1024), 0, st, hist, ncell, G.start.p, G.chain.p, G.chain_epoch, total_out,
                                       (int*)(c->d_ctr + ctr_dev(C_ERR)));
                    CHK(check_launch(c, "k_scan"));
                } else {
                    CHK(enqueue_scan(c, st, hist, ncell, G.start.p, G.sums, total_out));
                }
            }
            Prof p(c, SLOT_SCATTER, st);
            hipLaunchKernelGGL(k_scatter_atoms, dim3(nblocks(n, 256)), dim3(256), 0, st, r, n, G.cell_rank.p, G.start.p, sx.p, sa.p, rec, c->s_h.p, gm);
            CHK(check_launch(c, "k_scatter_atoms"));
        }
        G.cur = 1 - G.cur;
    } else {
        HIPCHK(c, hipMemsetAsync(G.start.p, 0, ((size_t)ncell + 1) * sizeof(int), st));
        if (total_out) HIPCHK(c, hipMemsetAsync(total_out, 0, sizeof(u64), st));
    }
    G.valid = true;
    G.n_binned = -1;  // known on the device only (start[ncell])
    return ARP_OK;
}
int build_contact_grid(arp_ctx* c, double radius, uint32_t req, uint32_t forb, const uint8_t* active, u64* total_out = nullptr,
                       ResMarks rm = ResMarks{nullptr, nullptr, 0}, GroupMasks gm = GroupMasks{}) {
    c->cg_valid = false;      // (the buffers of the pass's grid are rewritten)
    c->s_cell_valid = false;
    return build_atom_grid(c, c->atom_grid, c->s_xyzm, c->s_aux, &c->s_qa, radius, req, forb, active, total_out, nullptr, nullptr, rm, gm);
}
// The contact grid of a pass as an ordered compaction of the static columns (k_compact_atoms): ONE launch.
// use_table: the caller has seen that sp_keep_base describes this pass (enqueue_contacts): no chain, no look-back.
int build_contact_grid_compact(arp_ctx* c, double radius, uint32_t req, uint32_t forb, u64* total_out, uint8_t* plus_init, ResMarks rm,
                               bool use_table = false) {
    Grid& G = c->atom_grid;
    const int n = (int)c->n;
    CHK(grid_desc_for(c, G.d, c->lo, c->hi, radius));
    G.radius = radius;
    G.n_points = n;
    const int ncell = G.d.ncell;
    HIPCHK(c, G.start.reserve(scan_padded(ncell)));
    HIPCHK(c, c->s_xyzm.reserve((size_t)std::max(n, 1)));
    HIPCHK(c, c->s_aux.reserve((size_t)std::max(n, 1)));
    HIPCHK(c, c->s_qa.reserve((size_t)std::max(n, 1)));
    HIPCHK(c, c->s_h.reserve((size_t)std::max(n, 1)));
    CHK(ensure_static(c, radius));
    if (n > 0) {
        Prof p(c, SLOT_BIN);
        const int rows_per_block = compact_rows(n);
        const int nb = (n + rows_per_block - 1) / rows_per_block;
        // (the caller's look at the table was before this function's ensure_static: a new order since then, and the look-back it is)
        use_table = use_table && c->sp_keep_epoch == c->static_epoch && c->sp_keep_rows == rows_per_block && c->sp_keep_blocks == nb;
        if (!use_table) {
            bool fresh = false;
            HIPCHK(c, c->compact_chain.reserve((size_t)nb, &fresh));
            if (fresh || c->compact_epoch >= (1u << 30) - 1u) {   // new buffer, or the 30-bit launch number wraps: no stale word may match
                HIPCHK(c, hipMemsetAsync(c->compact_chain.p, 0, c->compact_chain.cap * sizeof(unsigned long long), c->stream));
                c->compact_epoch = 0;
            }
            ++c->compact_epoch;
        }
        c->compact_used_table = use_table;
        CompactArgs A;
        A.r = static_atoms(c);
        A.sp_cell = c->sp_cell.p; A.n = n; A.ncell = ncell; A.req = req; A.forb = forb;
        A.s_xyzm = c->s_xyzm.p; A.s_aux = c->s_aux.p; A.s_qa = c->s_qa.p; A.s_h = c->s_h.p;
        HIPCHK(c, c->s_cell.reserve((size_t)std::max(n, 1)));
        A.s_cell = c->s_cell.p;
        A.start = G.start.p; A.chain = c->compact_chain.p; A.epoch = c->compact_epoch; A.total_out = total_out;
        A.plus_init = plus_init; A.rm = rm; A.err = (int*)(c->d_ctr + ctr_dev(C_ERR));
        A.keep_base = use_table ? c->sp_keep.p + 4 + nb : nullptr;
        if (use_table) {
            if (rows_per_block == 512) hipLaunchKernelGGL((k_compact_atoms<512, true>), dim3(nb), dim3(512), 0, c->stream, A);
            else hipLaunchKernelGGL((k_compact_atoms<1024, true>), dim3(nb), dim3(1024), 0, c->stream, A);
        }
        else if (rows_per_block == 512) hipLaunchKernelGGL(k_compact_atoms<512>, dim3(nb), dim3(512), 0, c->stream, A);
        else hipLaunchKernelGGL(k_compact_atoms<1024>, dim3(nb), dim3(1024), 0, c->stream, A);
        CHK(check_launch(c, "k_compact_atoms"));
        c->s_cell_valid = true;
    } else {
        c->compact_used_table = false;
        HIPCHK(c, hipMemsetAsync(G.start.p, 0, ((size_t)ncell + 1) * sizeof(int), c->stream));
        if (total_out) HIPCHK(c, hipMemsetAsync(total_out, 0, sizeof(u64), c->stream));
    }
    G.valid = true;
    G.n_binned = -1;
    return ARP_OK;
}
// every atom (hydrogens included), used by the expansion and atom-plane; plus_init: also start selection_plus
int build_all_grid(arp_ctx* c, double radius, uint8_t* plus_init = nullptr, hipStream_t st = nullptr) {
    CHK(build_atom_grid(c, c->all_grid, c->a_xyzm, c->a_aux, nullptr, radius, 0, 0, nullptr, nullptr, plus_init, st));
    c->all_grid_current = true;
    return ARP_OK;
}

// The all-atom grid of the queries with caller-given centres (arp_search, arp_ring_residues): a centre belongs to no structure
// of a batch and to no model, so these answer over all resident atoms in world coordinates — with a partition in force the
// grid is built over the box of everything resident instead of the batch layout (whose cells a centre cannot be located in),
// and the pass, which needs the layout, builds its own again.
int build_world_grid(arp_ctx* c, double radius) {
    CHK(build_atom_grid(c, c->all_grid, c->a_xyzm, c->a_aux, nullptr, radius, 0, 0, nullptr, nullptr, nullptr, nullptr,
                        ResMarks{nullptr, nullptr, 0}, GroupMasks{}, /*world=*/true));
    c->all_grid_current = false;
    return ARP_OK;
}

// Entries per segment of the contact pair list: an even number (the per-pair kernel fetches the pairs of a batch as 16-byte
// quads), and 64 entries short of the allocation (it reads up to a batch beyond the end of a segment and ignores what it gets).
inline size_t pair_segcap(size_t cap) { return cap > 64 ? ((cap - 64) / PAIR_SEGS) & ~(size_t)1 : 0; }
// Blocks of the neighbour search: ~ARP_SEARCH_CPW cells per wave, a multiple of 8 (one per XCD).
int search_blocks(const GridDesc& d, int cpw = 1) {
    int nb = (d.ncell + SEARCH_WAVES * cpw - 1) / (SEARCH_WAVES * cpw);
    nb = std::max(8, std::min(nb, 8192));
    return (nb + 7) & ~7;
}
// ... rounded to whole rounds of resident blocks once the launch comes near one: with 656 blocks on a chip that holds 768,
// the CUs given three blocks have half as much work again as those given two, and the kernel lasts as long as the former
// (100 k atoms: 38.3 -> 35.3 us with 768)
int search_blocks_balanced(const arp_ctx* c, const GridDesc& d, int cpw) {
    if (sw().search_blocks > 0) return (sw().search_blocks + 7) & ~7;
    const int nb = search_blocks(d, cpw), R = c->search_resident;
    if (R < 8 || 2 * nb < R) return nb;
    return std::min(std::max(1, (nb + R / 2) / R) * R, 8192) & ~7;
}

// zero a range of LOGICAL counters (callers outside a whole pass: a pass zeroes the block as it publishes it)
int zero_counter(arp_ctx* c, int first, int count) {
    if (c->ctr_clean) return ARP_OK;  // arp_run_launch cleared the whole block with one memset
    c->ctr_zero_ok = false;
    if ((first == C_STAT_CAND || first == C_STAT_MCAND) && count == 2 * STAT_SLOTS) {   // two neighbouring words of every slot line: one 2-D fill
        HIPCHK(c, hipMemset2DAsync(c->d_ctr + ctr_dev(first), sizeof(u64) * CTR_LINE, 0, 2 * sizeof(u64), STAT_SLOTS, c->stream));
        return ARP_OK;
    }
    if (first == C_SEG_PAIRS && count == PAIR_SEGS) {                                   // eight whole lines
        HIPCHK(c, hipMemsetAsync(c->d_ctr + ctr_dev(first), 0, sizeof(u64) * PAIR_SEGS * CTR_LINE, c->stream));
        return ARP_OK;
    }
    for (int k = first; k < first + count; ++k) HIPCHK(c, hipMemsetAsync(c->d_ctr + ctr_dev(k), 0, sizeof(u64), c->stream));
    return ARP_OK;
}
int enqueue_counter_copy(arp_ctx* c, int zero = 0) {  // counter block -> pinned host memory (capturable)
    ++c->publish_seq;
    hipLaunchKernelGGL(k_publish_counters, dim3(1), dim3(256), 0, c->stream, c->d_ctr, c->h_ctr_pinned, (int)C_COUNT, zero, c->publish_seq);
    CHK(check_launch(c, "k_publish_counters"));
    return ARP_OK;
}
int collect_counters(arp_ctx* c) {  // the only stream sync of a pass
    // The pass ends by storing its number in pinned memory (pass_end in the last kernel, or k_publish_counters):
    // polling that word wakes the host ~10 us sooner than hipStreamSynchronize.  Bounded: after 2 ms (or with a
    // caller-owned stream or ARP_SPIN_WAIT=0) the runtime's own wait takes over.
    if (sw().spin_wait && !c->external_stream) {
        volatile u64* flag = c->h_ctr_pinned + C_COUNT;
        const auto t0 = std::chrono::steady_clock::now();
        for (int it = 0; *flag != c->publish_seq; ++it) {
            if ((it & 255) == 255 && std::chrono::steady_clock::now() - t0 > std::chrono::milliseconds(2)) break;
            __builtin_ia32_pause();
        }
        std::atomic_thread_fence(std::memory_order_acquire);
        if (*flag != c->publish_seq) {
            HIPCHK(c, hipStreamSynchronize(c->stream));
            if (*flag != c->publish_seq) FAIL(c, ARP_E_HIP, "the pass ended without publishing its counters");
        }
        else if ((c->publish_seq & 15) == 0) (void)hipStreamQuery(c->stream);   // lets the runtime retire finished commands
    } else {
        HIPCHK(c, hipStreamSynchronize(c->stream));
    }
    memcpy(c->h_ctr, c->h_ctr_pinned, sizeof(u64) * C_COUNT);
    auto fold = [&](int first, int into) {
        u64 t = 0;
        for (int k = 0; k < STAT_SLOTS; ++k) t += c->h_ctr[first + k];
        c->h_ctr[into] = t;
    };
    fold(C_STAT_CAND, C_CAND); fold(C_STAT_ACC, C_ACC); fold(C_STAT_MCAND, C_MARK_CAND); fold(C_STAT_MACC, C_MARK_ACC);
    return ARP_OK;
}
int read_counters(arp_ctx* c) {
    CHK(enqueue_counter_copy(c));
    return collect_counters(c);
}

// CSR offsets: start at 0, never decrease (the kernels index with them unchecked)
bool csr_ok(const int32_t* off, int64_t n) {
    if (off[0] != 0) return false;
    for (int64_t i = 0; i < n; ++i)
        if (off[i + 1] < off[i]) return false;
    return true;
}

template <class T>
bool all_finite(const T* v, int64_t n) {
    for (int64_t i = 0; i < n; ++i)
        if (!std::isfinite((double)v[i])) return false;
    return true;
}

// The atom lists k_ring_geometry / k_amide_geometry read unchecked, against a structure of n_atoms atoms (`who` = the entry
// point that was called).  Rings: CSR offsets, at least three atoms each, indices in range.
int check_ring_atoms(arp_ctx* c, const char* who, int64_t nring, const int32_t* off, const int32_t* idx, int64_t n_atoms) {
    const std::string w(who);
    if (nring == 0) return ARP_OK;
    if (!csr_ok(off, nring)) FAIL(c, ARP_E_ARG, w + ": ring offsets must start at 0 and never decrease");
    if (off[nring] > 0 && !idx) FAIL(c, ARP_E_ARG, w + ": ring atom indices missing");
    for (int64_t r = 0; r < nring; ++r)
        if (off[r + 1] - off[r] < 3) FAIL(c, ARP_E_ARG, w + ": a ring needs at least three atoms");
    for (int64_t k = 0; k < off[nring]; ++k)
        if (idx[k] < 0 || idx[k] >= n_atoms) FAIL(c, ARP_E_ARG, w + ": ring atom index out of range");
    return ARP_OK;
}
// Amides: N, C, O of each group of four are read; the fourth atom is not.
int check_amide_atoms(arp_ctx* c, const char* who, int64_t namide, const int32_t* atoms, int64_t n_atoms) {
    for (int64_t k = 0; k < 4 * namide; ++k)
        if ((k & 3) != 3 && (atoms[k] < 0 || atoms[k] >= n_atoms)) FAIL(c, ARP_E_ARG, std::string(who) + ": amide atom index out of range");
    return ARP_OK;
}

int ensure_ring_grid(arp_ctx* c) {
    CHK(join_upload_lists(c));
    if (c->ring_grid.valid) return ARP_OK;
    PtsD3 pts{c->ring_c.p};
    return build_grid<PtsD3>(c, c->ring_grid, pts, (int)c->nring, c->ring_lo, c->ring_hi, 6.0, c->sid_ring.p);
}
int ensure_amide_grid(arp_ctx* c) {
    CHK(join_upload_lists(c));
    if (c->amide_grid.valid) return ARP_OK;
    PtsF3 pts{c->am_c.p};
    return build_grid<PtsF3>(c, c->amide_grid, pts, (int)c->namide, c->am_lo, c->am_hi, 6.0, c->sid_amide.p);
}

// both centre grids in one launch when they are small (k_point_grids); otherwise each by the general path
int ensure_center_grids(arp_ctx* c) {
    CHK(join_upload_lists(c));      // (whoever asks for the grids on the main stream reads them there)
    const bool want_r = c->nring > 0 && !c->ring_grid.valid, want_a = c->namide > 0 && !c->amide_grid.valid;
    const int small_points = 16384;
    if ((want_r || want_a) && !sw().deterministic && c->nring <= small_points && c->namide <= small_points) {
        PointGridJob<PtsD3> jr{};
        PointGridJob<PtsF3> ja{};
        bool fits = true;
        if (want_r) {
            Grid& G = c->ring_grid;
            CHK(grid_desc_for(c, G.d, c->ring_lo, c->ring_hi, 6.0));
            fits = fits && G.d.ncell <= POINT_GRID_ITEMS * 1024;
        }
        if (want_a) {
            Grid& G = c->amide_grid;
            CHK(grid_desc_for(c, G.d, c->am_lo, c->am_hi, 6.0));
            fits = fits && G.d.ncell <= POINT_GRID_ITEMS * 1024;
        }
        if (fits) {
            if (want_r) {
                Grid& G = c->ring_grid;
                G.radius = 6.0; G.n_points = (int)c->nring;
                CHK(reserve_grid(c, G, (int)c->nring));
                jr = PointGridJob<PtsD3>{PtsD3{c->ring_c.p}, (int)c->nring, G.d, c->sid_ring.p, G.cell_of.p, G.cnt.p, G.start.p, G.perm.p};
            }
            if (want_a) {
                Grid& G = c->amide_grid;
                G.radius = 6.0; G.n_points = (int)c->namide;
                CHK(reserve_grid(c, G, (int)c->namide));
                ja = PointGridJob<PtsF3>{PtsF3{c->am_c.p}, (int)c->namide, G.d, c->sid_amide.p, G.cell_of.p, G.cnt.p, G.start.p, G.perm.p};
            }
            // (the entry counts of the candidate lists, which are rebuilt whenever the grids are, cleared on the way)
            const bool with_counts = c->lists_dirty || !c->plist_count.p;
            if (with_counts) { HIPCHK(c, c->plist_count.reserve(4)); c->lists_dirty = true; }
            Prof p(c, SLOT_BIN);
            hipLaunchKernelGGL(k_point_grids, dim3(2), dim3(1024), 0, c->stream, jr, ja, with_counts ? c->plist_count.p : (u64*)nullptr);
            CHK(check_launch(c, "k_point_grids"));
            c->plist_count_cleared = with_counts;
            if (want_r) c->ring_grid.valid = true;
            if (want_a) c->amide_grid.valid = true;
            return ARP_OK;
        }
    }
    if (c->nring > 0) CHK(ensure_ring_grid(c));
    if (c->namide > 0) CHK(ensure_amide_grid(c));
    return ARP_OK;
}

// ---- enqueue-only building blocks (no host synchronisation) -----------------------------------

// _make_selection, part 1 (I:1384-1424): selection_plus from the selection mask already in c->sel
int enqueue_expansion(arp_ctx* c, double radius, hipStream_t st = nullptr) {
    ++c->sel_epoch;
    if (!st) st = c->stream;
    const int n = (int)c->n;
    HIPCHK(c, c->plus.reserve((size_t)std::max(n, 1)));
    c->sel_made = true;   // (I:1407 selection_plus = selection is written by the binning kernel below)
    // I:1420-1424: search_all(6.0) over ALL atoms (hydrogens included)
    CHK(build_all_grid(c, radius, c->plus.p, st));
    CHK(zero_counter(c, C_STAT_MCAND, 2 * STAT_SLOTS));
    // With every atom selected, selection_plus = selection whatever the pairs are: the search is skipped (the
    // grid is still built, the atom-plane kernel walks it).
    if (n > 0 && !c->sel_all) {
        Prof p(c, SLOT_MARK, st);
        hipLaunchKernelGGL((k_search<MODE_MARK>), dim3(search_blocks(c->all_grid.d)), dim3(64 * SEARCH_WAVES), 0, st,
                           c->all_grid.d, c->all_grid.start.p, c->a_xyzm.p, c->a_aux.p, radius * radius, 1, 0, (int2*)nullptr,
                           0ull, c->d_ctr + ctr_dev(C_SCRATCH0), c->d_ctr + ctr_dev(C_STAT_MCAND), c->d_ctr + ctr_dev(C_STAT_MACC), c->plus.p, GroupMasks{}, (const int*)nullptr, (const int*)nullptr);
        CHK(check_launch(c, "k_search<MARK>"));
    }
    // all_grid stays usable for the atom-plane kernel: it reads plus[] directly, M_SEL is current
    c->contacts_valid = false;
    c->void_bags();
    return ARP_OK;
}

int check_residue_ranges(arp_ctx* c) {   // the set kernels index the residue table with the uploaded ids, unchecked
    if (std::max({c->max_res_id, c->max_ring_res, c->max_amide_res}) >= std::max<int64_t>(c->nres, 1))
        FAIL(c, ARP_E_ARG, "selection sets: an atom, ring or amide refers to a residue beyond the residue table (arp_set_residues)");
    return ARP_OK;
}

// I:1413-1437: residue, ring and amide sets of the selection and of selection_plus.  Only the ring / amide
// kernels consume them, so arp_run_launch puts this stage on their stream.
int enqueue_selection_sets(arp_ctx* c, hipStream_t st) {
    const int n = (int)c->n;
    const size_t nres = (size_t)std::max<int64_t>(c->nres, 1);
    CHK(check_residue_ranges(c));
    HIPCHK(c, c->res_sel.reserve(2 * nres));   // [0, nres) = selection residues, [nres, 2 nres) = selection_plus residues
    uint8_t* res_sel = c->res_sel.p;
    uint8_t* res_plus = c->res_sel.p + nres;
    // arp_set_whole_structure: every residue of the (global) table is selected — also those whose atoms live on
    // another rank of a sharded run, which the local atoms could not tell
    const bool all_res = c->whole_structure && c->sel_all;
    HIPCHK(c, hipMemsetAsync(res_sel, all_res ? 1 : 0, 2 * nres, st));
    if (n > 0 && !all_res)
        hipLaunchKernelGGL(k_res_mark, dim3(nblocks(n, 256)), dim3(256), 0, st, n, c->res_id.p, c->sel.p, c->plus.p,
                           res_sel, res_plus);
    if (c->nring + c->namide > 0)
        hipLaunchKernelGGL(k_group_mask, dim3(nblocks(c->nring + c->namide, 256)), dim3(256), 0, st, (int)c->nring, (int)c->namide,
                           c->ring_res.p, c->am_res.p, res_sel, res_plus, c->ring_sel.p, c->ring_plus.p, c->am_sel.p, c->am_plus.p);
    return check_launch(c, "selection sets");
}

int enqueue_selection(arp_ctx* c, double radius) {   // the whole _make_selection on the main stream
    ++c->sel_epoch;
    CHK(enqueue_expansion(c, radius));
    return enqueue_selection_sets(c, c->stream);
}

// the default selection of a structure nobody uploaded one for: everything (I:1395 with no selectors)
int default_selection(arp_ctx* c) {
    if (c->sel_uploaded) return ARP_OK;
    const size_t n = (size_t)std::max<int64_t>(c->n, 1);
    HIPCHK(c, c->sel.reserve(n));
    if (!c->sel_prefilled) HIPCHK(c, hipMemsetAsync(c->sel.p, 1, n, c->stream));
    c->sel_prefilled = false;
    c->sel_all = true;
    c->sel_uploaded = true;
    return ARP_OK;
}

int ensure_default_selection(arp_ctx* c) {  // whole structure selected (I:1395 with no selectors)
    if (c->sel_made) return ARP_OK;
    CHK(default_selection(c));
    return enqueue_selection(c, 6.0);   // an uploaded selection that was not expanded yet is expanded here
}

int bag_reserve(arp_ctx* c, int kind, size_t cap) {
    Bag& b = c->bag[kind];
    cap = cap + cap / 4 + 64;
    size_t off[BAG_COLS];
    const size_t total = bag_slab_layout(kind, cap, 0, off);
    b.release();
    HIPCHK(c, b.slab.reserve(total));
    for (int j = 0; j < BAG_COLS; ++j)
        if (bag_has(kind, j)) b.col[j] = b.slab.p + off[j];
    b.cap = cap;
    return ARP_OK;
}

// One wavefront per ring / amide up to PLANE_BLOCKS blocks, several items per wave beyond: the waves queue their
// records in LDS and a block pays ONE counter atomic when it ends.
#define PLANE_BLOCKS 1024
// items (rings / amides) per wavefront of the ring / amide kernels: their candidate pairs gather in the wave's LDS queue
// until 64 are there for a full-lane evaluation, so a wave should see a few items; every item costs a few dependent
// loads, so not too many (sweep in profiles/README.md)
int plane_blocks(int64_t items) {
    const int ipw = sw().plane_ipw;
    return nblocks((items + ipw - 1) / ipw * 64, 256, PLANE_BLOCKS);
}
// The four ring / amide kernels: prepare_* sizes the bag, clears its counter and fills the kernel arguments
// (nb = number of blocks, 0 when there is nothing to do); enqueue_* launches one of them, enqueue_planes all
// four as ONE launch (k_planes).
int prepare_atom_plane(arp_ctx* c, AtomPlaneArgs& a, int& nb, bool contact_grid = false) {  // I:947-1062
    Bag& b = c->bag[BAG_AP];
    nb = 0;
    if (!b.cap) CHK(bag_reserve(c, BAG_AP, (size_t)c->nring * 8 + 256));
    CHK(zero_counter(c, C_AP, 1));
    if (c->nring == 0 || c->n == 0) return ARP_OK;
    // contact_grid: the grid of the pass (selection_plus without hydrogens, atom_plane_cg_body); else the all-atom 6 A grid
    // (I:960 radius): the one the selection expansion has just built, if it is still current
    if (!contact_grid && !(c->all_grid_current && c->all_grid.valid && c->all_grid.radius == 6.0)) CHK(build_all_grid(c, 6.0));
    const Grid& G = contact_grid ? c->atom_grid : c->all_grid;
    a = AtomPlaneArgs{G.d, G.start.p, contact_grid ? c->s_xyzm.p : c->a_xyzm.p, contact_grid ? c->s_aux.p : c->a_aux.p, (int)c->nring,
                      c->ring_c.p, c->ring_n.p, c->ring_res.p, c->ring_sel.p, c->ring_plus.p, c->plus.p,
                      c->has_group_owner ? c->ring_home.p : nullptr, c->has_group_owner ? c->ring_gid.p : nullptr, c->has_gid ? c->gid.p : nullptr,
                      (long long)b.cap, b.id(0), b.id(1), b.val<double>(0), b.val<double>(1), b.byte(0), b.byte(1), c->d_ctr + ctr_dev(C_AP),
                      c->st_xyzm.p, c->sel_made ? c->sel.p : nullptr, (c->sel_made && c->sel_all) ? 1 : 0};
    nb = plane_blocks(c->nring);
    return ARP_OK;
}
int prepare_plane_plane(arp_ctx* c, PlanePlaneArgs& a, int& nb) {  // I:1064-1194
    Bag& b = c->bag[BAG_PP];
    nb = 0;
    if (!b.cap) CHK(bag_reserve(c, BAG_PP, (size_t)c->nring * 16 + 256));
    CHK(zero_counter(c, C_PP, 1));
    if (c->nring == 0) return ARP_OK;
    CHK(ensure_ring_grid(c));
    a = PlanePlaneArgs{c->ring_grid.d, c->ring_grid.start.p, c->ring_grid.perm.p, (int)c->nring, c->ring_c.p, c->ring_n.p,
                       c->ring_res.p, c->ring_sel.p, c->ring_plus.p, c->has_group_owner ? c->ring_home.p : nullptr,
                       c->has_group_owner ? c->ring_gid.p : nullptr, (long long)b.cap, b.id(0), b.id(1), b.val<double>(0), b.val<double>(1),
                       b.val<double>(2), b.val<double>(3), b.byte(0), b.byte(1), b.byte(2), c->d_ctr + ctr_dev(C_PP)};
    nb = plane_blocks(c->nring);
    return ARP_OK;
}
int prepare_group_group(arp_ctx* c, GroupGroupArgs& a, int& nb) {  // I:1217-1300
    Bag& b = c->bag[BAG_GG];
    nb = 0;
    if (!b.cap) CHK(bag_reserve(c, BAG_GG, (size_t)c->namide * 8 + 256));
    CHK(zero_counter(c, C_GG, 1));
    if (c->namide == 0) return ARP_OK;
    CHK(ensure_amide_grid(c));
    a = GroupGroupArgs{c->amide_grid.d, c->amide_grid.start.p, c->amide_grid.perm.p, (int)c->namide, c->am_c.p, c->am_n.p,
                       c->am_sel.p, c->am_plus.p, c->has_group_owner ? c->am_home.p : nullptr,
                       c->has_group_owner ? c->am_gid.p : nullptr, (long long)b.cap, b.id(0), b.id(1), b.val<float>(0), b.val<float>(1),
                       b.val<float>(2), b.byte(0), c->d_ctr + ctr_dev(C_GG)};
    nb = plane_blocks(c->namide);
    return ARP_OK;
}
int prepare_group_plane(arp_ctx* c, GroupPlaneArgs& a, int& nb) {  // I:1302-1382
    Bag& b = c->bag[BAG_GP];
    nb = 0;
    if (!b.cap) CHK(bag_reserve(c, BAG_GP, (size_t)c->namide * 8 + 256));
    CHK(zero_counter(c, C_GP, 1));
    if (c->namide == 0 || c->nring == 0) return ARP_OK;
    CHK(ensure_ring_grid(c));
    a = GroupPlaneArgs{c->ring_grid.d, c->ring_grid.start.p, c->ring_grid.perm.p, (int)c->namide, c->am_c.p, c->am_n.p,
                       c->am_sel.p, c->am_plus.p, c->ring_c.p, c->ring_n.p, c->ring_sel.p, c->ring_plus.p,
                       c->has_group_owner ? c->am_home.p : nullptr, c->has_group_owner ? c->am_gid.p : nullptr,
                       c->has_group_owner ? c->ring_gid.p : nullptr, (long long)b.cap, b.id(0), b.id(1), b.val<double>(0), b.val<double>(1),
                       b.val<double>(2), b.byte(0), c->d_ctr + ctr_dev(C_GP)};
    nb = plane_blocks(c->namide);
    return ARP_OK;
}

// One ring / amide loop alone by its grid walk (arp_planes.h); kind: 0 atom-plane, 1 plane-plane, 2 group-group, 3 group-plane
template <class Args, class Prepare>
int enqueue_walk(arp_ctx* c, Prepare prepare, void (*kernel)(Args), const char* what) {
    Args a{};
    int nb = 0;
    CHK(prepare(c, a, nb));
    if (!nb) return ARP_OK;
    Prof p(c, SLOT_PLANES, c->stream);
    hipLaunchKernelGGL(kernel, dim3(nb), dim3(256), 0, c->stream, a);
    return check_launch(c, what);
}
int enqueue_bag_walk(arp_ctx* c, int kind) {
    if (kind == 0) return enqueue_walk(c, [](arp_ctx* c, AtomPlaneArgs& a, int& nb) { return prepare_atom_plane(c, a, nb); }, k_atom_plane, "k_atom_plane");
    if (kind == 1) return enqueue_walk(c, prepare_plane_plane, k_plane_plane, "k_plane_plane");
    if (kind == 2) return enqueue_walk(c, prepare_group_group, k_group_group, "k_group_group");
    return enqueue_walk(c, prepare_group_plane, k_group_plane, "k_group_plane");
}
// Static candidate lists of the ring / amide loops (arp_planes.h): built on the stream when the structure changed.
PlaneLists plane_lists(arp_ctx* c) {
    PlaneLists L;
    for (int k = 0; k < 4; ++k) { L.pairs[k] = c->plist[k].p; L.cap[k] = (long long)c->plist[k].cap; }
    L.count = c->plist_count.p;
    return L;
}
int ensure_plane_lists(arp_ctx* c) {
    CHK(join_upload_lists(c));
    if (!c->lists_dirty && c->plist_count.p) return ARP_OK;
    const size_t want[4] = {(size_t)c->nring * 96 + 256, (size_t)c->nring * 16 + 256, (size_t)c->namide * 16 + 256, (size_t)c->namide * 8 + 256};
    for (int k = 0; k < 4; ++k) HIPCHK(c, c->plist[k].reserve(want[k]));
    HIPCHK(c, c->plist_count.reserve(4));
    if (!c->plist_count_cleared) HIPCHK(c, hipMemsetAsync(c->plist_count.p, 0, 4 * sizeof(u64), c->stream));   // (else: k_point_grids did, on this stream)
    c->plist_count_cleared = false;
    AtomRingListArgs ar{};
    PlanePlaneArgs pp{};
    GroupGroupArgs gg{};
    GroupPlaneArgs gp{};
    int n0 = 0, n1 = 0, n2 = 0, n3 = 0;
    {   // (argument blocks and bag buffers only: the counters of the output bags are the evaluation's affair — a pass clears them
        // itself, and at upload time each would be a fill launch in front of the lists)
        const bool was_clean = c->ctr_clean;
        c->ctr_clean = true;
        int rc = prepare_plane_plane(c, pp, n1);      // (ring / amide grids: built here if need be)
        if (rc == ARP_OK) rc = prepare_group_group(c, gg, n2);
        if (rc == ARP_OK) rc = prepare_group_plane(c, gp, n3);
        c->ctr_clean = was_clean;
        CHK(rc);
    }
    // atom-plane candidates atom by atom against the ring grid (ar_enumerate): the atoms as uploaded, no atom grid
    if (c->nring > 0 && c->n > 0) {
        ar = AtomRingListArgs{c->ring_grid.d, c->ring_grid.start.p, c->ring_grid.perm.p, (int)c->n, c->xyz.p, c->tmask.p, c->flags.p, c->ring_c.p};
        n0 = nblocks(c->n, 256, 4096);
    }
    // one wavefront per ring / amide: a stencil walk is a chain of dependent loads, and this kernel runs alone
    if (n1) n1 = nblocks(c->nring * 64, 256, 4096);
    if (n2) n2 = nblocks(c->namide * 64, 256, 4096);
    if (n3) n3 = nblocks(c->namide * 64, 256, 4096);
    if (n0 + n1 + n2 + n3 > 0) {
        hipLaunchKernelGGL(k_plane_lists, dim3(n0 + n1 + n2 + n3), dim3(256), 0, c->stream, ar, pp, gg, gp, plane_lists(c), n0, n0 + n1,
                           n0 + n1 + n2, n0 + n1 + n2 + n3);
        CHK(check_launch(c, "k_plane_lists"));
    }
    c->lists_dirty = false;
    return ARP_OK;
}

// f(S, G) with S, G = std::integral_constant<int, 0 or 1>: two run-time bits as the template parameters of a kernel.  (The
// deduced return types instantiate f where this is called, in the order below: the kernels keep their places in the code object.)
template <class F>
auto with_bits(bool s, bool g, F f) {
    using I0 = std::integral_constant<int, 0>;
    using I1 = std::integral_constant<int, 1>;
    if (s) { if (g) f(I1{}, I1{}); else f(I1{}, I0{}); }
    else { if (g) f(I0{}, I1{}); else f(I0{}, I0{}); }
}

// The pass proper: _calculate_atom_contacts (I:693-936) = contact grid (bin + scan/scatter), neighbour search, fused
// per-pair kernel; with_planes: the four ring / amide loops (I:938-1382) ride in the last launch (k_sift_planes).
// fuse_sets (arp_run_launch): the grid build also produces the residue / ring / amide sets of I:1413-1437.
int enqueue_contacts(arp_ctx* c, double cutoff, double vdw_comp, int include_seq_adj, bool with_planes) {
    struct Defer { arp_ctx* c; ~Defer() { c->uplists_defer = false; } } defer{c};
    c->uplists_defer = !c->external_stream;
    c->bag_cutoff = cutoff; c->bag_comp = vdw_comp; c->bag_sel_all = c->sel_made && c->sel_all;      // (what the bag is made under)
    // the tree is built on selection_plus (I:1442); hydrogens are dropped at I:712
    if (!c->ctr_clean) CHK(zero_counter(c, C_BINNED, 1));
    CHK(zero_counter(c, C_ERR, 1));      // (before the grid build: its chained scan may raise the flag)
    ResMarks rm{nullptr, nullptr, 0};
    GroupMasks gm{};
    bool masks_after_bin = false;
    // the grid of the previous whole-structure pass, if nothing it depends on has changed (see grid_reuse)
    const bool all_res_now = c->whole_structure && c->sel_all;
    const bool whole = c->sel_made && c->sel_all && c->n > 0;
    auto grid_key = [&]() { return GridKey{cutoff, c->static_epoch, c->sel_epoch, c->fuse_sets, c->init_plus_in_bin, all_res_now}; };
    const bool reuse_grid = c->grid_reuse && whole && c->cg_valid && !c->cg_pending && c->atom_grid.valid && c->cg_key == grid_key() &&
                            !c->static_dirty && c->sp_radius == cutoff;
    c->cg_reused = reuse_grid;
    if (c->fuse_sets) {
        const size_t nres = (size_t)std::max<int64_t>(c->nres, 1);
        CHK(check_residue_ranges(c));
        bool fresh = false;
        HIPCHK(c, c->res_tag.reserve(2 * nres, &fresh));
        if (!reuse_grid && (fresh || c->res_tag_value >= 255)) {
            HIPCHK(c, hipMemsetAsync(c->res_tag.p, 0, c->res_tag.cap, c->stream));
            c->res_tag_value = 0;
        }
        // (a reused grid keeps the residue tags its build left: the masks below are made from the same tag value)
        const uint8_t tag = reuse_grid ? (uint8_t)c->res_tag_value : (uint8_t)++c->res_tag_value;
        const bool all_res = c->whole_structure && c->sel_all;   // every residue of the (global) table is selected
        if (!all_res) rm = ResMarks{c->res_tag.p, c->res_tag.p + nres, tag};
        gm = GroupMasks{(int)c->nring, (int)c->namide, c->ring_res.p, c->am_res.p, c->res_tag.p, c->res_tag.p + nres, tag,
                        all_res ? 1 : 0, c->ring_sel.p, c->ring_plus.p, c->am_sel.p, c->am_plus.p};
        if (c->n == 0) masks_after_bin = true;   // no scatter launch to carry them
    }
    // The static candidate lists of a structure's ring / amide loops — two centre grids, k_plane_lists — are made with its upload
    // when it comes as a blob (arp_set_blob: on the second stream, behind the validation kernel, joined below).  Structures set up
    // by the classic setters or assembled from shards build them in their first pass: nothing before the last launch of the pass
    // reads them, so they go on the second stream, beside the grid build and the search of this pass, and are enqueued AFTER the
    // search (the host needs ~5 us per launch: enqueued first they held the main stream's kernels back by as much).
    // (The other way round — search on the second stream, lists on the main one, so that the last launch follows the longer
    // chain in stream order — was no faster: the search then shares the chip with the 1024-thread scan blocks of the lists.)
    const bool fork_lists = with_planes && c->nring + c->namide > 0 && c->n > 0 &&
                            (c->lists_dirty || !c->plist_count.p || (c->nring > 0 && !c->ring_grid.valid) || (c->namide > 0 && !c->amide_grid.valid)) &&
                            !c->external_stream && c->stream2;
    if (fork_lists) {
        CHK(ensure_static(c, cutoff));                                  // (what the lists read is in place on the main stream here)
        HIPCHK(c, hipEventRecord(c->ev_sel, c->stream));
    }
    if (!reuse_grid) {
        c->cg_valid = false;
        // A whole-structure pass keeps every row of the spatial order that is no hydrogen, whatever else the pass is: where its
        // blocks' records begin follows from the order alone (sp_keep_base), and k_compact_atoms reads it instead of looking back.
        // Any other selection or predicate, a table of another order or of other blocks, an order's first build: the look-back.
        const uint32_t req = M_PLUS, forb = M_HYDROGEN;
        CHK(ensure_static(c, cutoff));      // (the order of this pass: what the table has to describe)
        const bool whole_pass = c->sel_made && c->sel_all && req == M_PLUS && forb == M_HYDROGEN && c->n > 0 && !c->compact_lookback;
        if (whole_pass && (c->sp_keep_epoch != c->static_epoch || c->sp_keep_rows != compact_rows((int)c->n))) {
            if (c->sp_keep_seen == c->static_epoch) CHK(make_keep_bases(c));      // the second such build over this order
            else c->sp_keep_seen = c->static_epoch;                               // the first one looks back
        }
        const bool use_table = whole_pass && c->sp_keep_epoch == c->static_epoch && c->sp_keep_rows == compact_rows((int)c->n);
        CHK(build_contact_grid_compact(c, cutoff, req, forb, c->d_ctr + ctr_dev(C_BINNED), c->init_plus_in_bin ? c->plus.p : nullptr, rm, use_table));
        if (whole) {      // what this grid was built from; its atom count arrives with the counters of the pass (finish_contacts)
            c->cg_valid = true; c->cg_pending = true;
            c->cg_key = grid_key();      // (after the build: ensure_static may have made a new spatial order)
        }
    }
    if (masks_after_bin && c->nring + c->namide > 0) {
        hipLaunchKernelGGL(k_group_masks, dim3(nblocks(c->nring + c->namide, 256)), dim3(256), 0, c->stream, gm);
        CHK(check_launch(c, "k_group_masks"));
    }
    c->contact_cells = c->atom_grid.d.ncell;
    if (!c->pairs.p) HIPCHK(c, c->pairs.reserve((size_t)c->n * 16 + 8192));
    const size_t segcap = pair_segcap(c->pairs.cap);   // the pair list is PAIR_SEGS segments of segcap entries
    const size_t cap = segcap * PAIR_SEGS;
    if (cap >= ((size_t)1 << 32)) FAIL(c, ARP_E_CAPACITY, "contact list beyond 2^32 entries (k_sift's task queue holds 32-bit output indices)");
    HIPCHK(c, c->out_i.reserve(cap)); HIPCHK(c, c->out_j.reserve(cap)); HIPCHK(c, c->out_d.reserve(cap));
    HIPCHK(c, c->out_s.reserve(cap)); HIPCHK(c, c->out_ct.reserve(cap));
    CHK(zero_counter(c, C_SEG_PAIRS, PAIR_SEGS));
    CHK(zero_counter(c, C_STAT_CAND, 2 * STAT_SLOTS));
    bool search_launched = false;
    auto launch_search = [&]() -> int {
        if (search_launched || c->n == 0) return ARP_OK;
        search_launched = true;
        Prof p(c, SLOT_SEARCH);
        // the contact search ends with a block-level flush of its pair queues, which amortises better over
        // ~3 cells per wave; the flush-free expansion search prefers 1 (sweeps in profiles/README.md)
        // Small grids (a protein of a few thousand atoms has ~1000 cells) get fewer cells per wave: the chip is far from full
        // and a wave's cells are a serial chain (1tqn_h stand-in: 22 -> 16 us).
        // (twelve since the waves of a block CLAIM their work: a longer list per block evens out better — 1 M atoms 196 -> 176 us —;
        // three was the optimum of the static three-cells-per-wave assignment)
        const int cpw = std::max(1, std::min(sw().search_cpw, c->atom_grid.d.ncell / (SEARCH_WAVES * 2 * c->num_cu)));
        // tiles of two x-adjacent cells (k_search): fewer, fuller units — worth it where a wave still has several to claim
        const int tile_x = sw().search_tile > 0 ? std::min(sw().search_tile, 2) : (c->atom_grid.d.ncell >= sw().search_tile_min_cells ? 2 : 1);
        // Sparse grids (fewer atoms than cells: a protein in its box, a ligand's selection_plus, a batch): the blocks split the
        // ATOMS of the grid evenly instead of its cells (k_search, cell_of_pos) and their number goes with the atoms — what the
        // grid's build reported last time, all atoms of the structure before that is known.
        const int64_t atoms_est = c->cg_reused ? c->cg_binned : (c->stats[4] == c->atom_grid.d.ncell && c->stats[3] > 0 ? c->stats[3] : c->n);
        // ... and so do the blocks of a CLUMPED structure (cells with hundreds of atoms: a chain folded onto itself), which the
        // previous pass over this structure gives away by its distance tests per atom (uniform protein density: ~80)
        const bool clumped = c->stats[3] > 0 && c->stats[4] == c->atom_grid.d.ncell && c->stats[0] > 150 * c->stats[3];
        const bool by_atoms = c->s_cell_valid && (sw().search_balance == 1 || (sw().search_balance < 0 && ((int64_t)c->atom_grid.d.ncell > atoms_est || clumped)));
        int nblocks_search = search_blocks_balanced(c, c->atom_grid.d, cpw);
        if (by_atoms) {
            const int R = c->search_resident;
            int nbk = (int)std::min<int64_t>(std::max<int64_t>((atoms_est + sw().search_apb - 1) / sw().search_apb, 8), 8192);
            nbk = (nbk + 7) & ~7;
            nblocks_search = (R >= 8 && 2 * nbk >= R) ? std::min(std::max(1, (nbk + R / 2) / R) * R, 8192) & ~7 : nbk;
        }
        const bool hint_wanted = sw().balance_hint && whole && (!by_atoms || sw().balance_hint_atoms);
        const HintKey hint_key{by_atoms, c->static_epoch, c->sel_epoch, cutoff, nblocks_search, tile_x};
        const bool hint_ok = hint_wanted && c->sb_valid && c->sb_key == hint_key && c->sb_tile.p;
        const int* const balance_hint = hint_ok ? (const int*)c->sb_tile.p : (const int*)nullptr;
        auto search = [&](auto tx) {
            hipLaunchKernelGGL((k_search<MODE_CONTACTS, decltype(tx)::value>), dim3(nblocks_search), dim3(64 * SEARCH_WAVES), 0,
                               c->stream, c->atom_grid.d, c->atom_grid.start.p, c->s_xyzm.p, c->s_aux.p, cutoff * cutoff,
                               include_seq_adj, c->has_home ? 1 : 0, c->pairs.p, (u64)segcap, c->d_ctr + ctr_dev(C_SEG_PAIRS), c->d_ctr + ctr_dev(C_STAT_CAND),
                               c->d_ctr + ctr_dev(C_STAT_ACC), (uint8_t*)nullptr, masks_after_bin ? GroupMasks{} : gm,
                               by_atoms ? (const int*)c->s_cell.p : (const int*)nullptr, balance_hint);
        };
        if (tile_x == 2) search(std::integral_constant<int, 2>{});
        else search(std::integral_constant<int, 1>{});
        // the hint for the LATER passes over this grid (same structure, selection, cutoff, launch shape), made behind the search of
        // the SECOND pass over it: the launch sits between the search and the per-pair kernel of that pass (6 us + a gap: a tenth
        // of a structure's first pass when it was made there), and a structure that is evaluated once never needs it.  First and
        // second pass run on equal runs of cells.
        if (hint_wanted && !hint_ok && nblocks_search >= 16) {
            const bool seen = c->sb_seen && c->sb_seen_key == hint_key;
            if (seen || sw().balance_hint_eager) {
                HIPCHK(c, c->sb_tile.reserve((size_t)nblocks_search + 1));
                if (!by_atoms) {
                    hipLaunchKernelGGL(k_balance_blocks, dim3(nblocks(nblocks_search + 1, 256)), dim3(256), 0, c->stream, c->atom_grid.d, c->atom_grid.start.p,
                                       nblocks_search, tile_x, sw().cell_weight_x16, c->sb_tile.p);
                } else {
                    // runs of ATOMS of equal weight: weight per cell, its running sum (the scans of the grid builds), one binary search per block
                    const int ncell = c->atom_grid.d.ncell;
                    HIPCHK(c, c->sb_cw.reserve(scan_padded(ncell))); HIPCHK(c, c->sb_cwp.reserve(scan_padded(ncell)));
                    hipLaunchKernelGGL(k_cell_weights, dim3(nblocks(ncell, 256, 2048)), dim3(256), 0, c->stream, c->atom_grid.d, c->atom_grid.start.p, sw().w_unit, sw().w_chunk, sw().w_test_x8, c->sb_cw.p);
                    CHK(enqueue_scan(c, c->stream, c->sb_cw.p, ncell, c->sb_cwp.p, c->sb_sums));
                    hipLaunchKernelGGL(k_balance_atoms, dim3(nblocks(nblocks_search + 1, 256)), dim3(256), 0, c->stream, c->atom_grid.d, c->atom_grid.start.p,
                                       (const int*)c->sb_cwp.p, nblocks_search, c->sb_tile.p);
                }
                c->sb_valid = true;
                c->sb_key = hint_key;
            } else {
                c->sb_seen = true;
                c->sb_seen_key = hint_key;
            }
        }
        return check_launch(c, "k_search<CONTACTS>");
    };
    // the per-pair kernel of the pass; merged_: with the list blocks of the ring / amide loops in front (np of them)
    AtomPlaneArgs ap{};
    PlanePlaneArgs pp{};
    GroupGroupArgs gg{};
    GroupPlaneArgs gp{};
    int np = 0;
    bool sift_launched = false;
    auto launch_sift = [&](bool merged_) -> int {
        sift_launched = true;
        CHK(join_upload_lists(c, /*must=*/true));      // (the list blocks of this launch read what the upload's second stream made)
        Prof p(c, SLOT_SIFT);
        // (the blocks split their work statically: all of them must be resident from the start)
        const int sift_blocks_per_cu = sw().sift_bpc > 0 ? sw().sift_bpc : c->sift_per_cu;
        SiftArgs sa{c->pairs.p, c->d_ctr + ctr_dev(C_SEG_PAIRS), (u64)segcap, c->s_xyzm.p, c->s_qa.p, c->s_h.p, {0, 0, 0, 0, 0, 0, 0, 0},
                          SiftSide{c->rad_tab.p, c->rad.p, c->xyz.p, c->h_off.p, c->bond_off.p, c->sb.p, c->longest_bond.p}, c->bond_idx.p, c->h_xyz_d.p,
                          c->has_gid ? c->gid.p : nullptr, vdw_comp, c->out_i.p, c->out_j.p, c->out_d.p, c->out_s.p, c->out_ct.p,
                          (int*)(c->d_ctr + ctr_dev(C_ERR)), c->xcd_round_robin ? 0 : 1};
        // No more sift blocks than the pairs can feed (one batch of 64 per wave and block at least): what the previous pass over
        // this structure found, or ~13 per heavy atom for the first one.  A protein-sized structure then runs 70-odd blocks
        // instead of 1024, whose start-up and end-of-pass tickets were most of the kernel (stand-in: 25 -> 16 us).
        const int pairs_per_block = sw().sift_ppb;
        const int64_t expect = (c->contacts_expected > 0) ? c->contacts_expected : (int64_t)c->n * 13;
        const bool stream_out = expect * 15 > sw().stream_out_bytes;     // (15 B per record)
        const int by_work = (int)std::min<int64_t>((expect + pairs_per_block - 1) / pairs_per_block + PAIR_SEGS, 1 << 20);
        const int slots = merged_ ? std::max(c->num_cu * sift_blocks_per_cu - np, 8 * PAIR_SEGS) : c->num_cu * sift_blocks_per_cu;
        const int nsift = std::max(std::min(slots, by_work), 8 * PAIR_SEGS) & ~(PAIR_SEGS - 1);
        // (four variants each: streaming stores or not, global ids or not — template parameters of the kernels, see sift_body)
        {   // a segment's share of the sift blocks goes with its size in the pass before (k_sift: nblk)
            const int B = nsift / PAIR_SEGS;
            uint64_t tot = 0;
            for (int k = 0; k < PAIR_SEGS; ++k) tot += c->seg_last[k];
            int given = 0, big = 0;
            for (int k = 0; k < PAIR_SEGS; ++k) {
                sa.nblk[k] = (sw().sift_shares && tot > 0 && B > 1) ? std::max(1, (int)((double)nsift * (double)c->seg_last[k] / (double)tot + 0.5)) : B;
                given += sa.nblk[k];
                if (sa.nblk[k] > sa.nblk[big]) big = k;
            }
            // the shares add up to the launch (the largest one takes the rounding; never below one block)
            while (given != nsift) {
                const int step = given > nsift ? -1 : 1;
                if (sa.nblk[big] + step < 1) { for (int k = 0; k < PAIR_SEGS; ++k) sa.nblk[k] = B; break; }
                sa.nblk[big] += step; given += step;
                big = 0;
                for (int k = 1; k < PAIR_SEGS; ++k) if (sa.nblk[k] > sa.nblk[big]) big = k;
            }
        }
        const bool with_gid = sa.gid != nullptr;
        if (merged_)
            with_bits(stream_out, with_gid, [&](auto S, auto G) {
                hipLaunchKernelGGL((k_sift_planes<decltype(S)::value, decltype(G)::value>), dim3(np + nsift), dim3(256), 0, c->stream, sa, nsift,
                                   ap, pp, gg, gp, plane_lists(c), c->d_ctr + ctr_dev(C_PLIST), np, c->pub);
            });
        else
            with_bits(stream_out, with_gid, [&](auto S, auto G) {
                hipLaunchKernelGGL((k_sift<decltype(S)::value, decltype(G)::value>), dim3(nsift), dim3(256), 0, c->stream, sa, c->pub);
            });
        return check_launch(c, "k_sift");
    };
    // A structure's FIRST pass (fork_lists): the list chain (~55 us at 100 k atoms) is longer than grid build + search (~43 us), and
    // the host needs ~5 us per launch.  So the main stream gets ALL its kernels first — grid, search, per-pair kernel — and the
    // second stream the lists and, behind them and behind the search (ring / amide masks), their evaluation as a kernel of its own
    // (k_planes); the two last kernels end the pass together (pass_end: expected = 2).  Later passes evaluate the resident lists
    // in the leading blocks of the per-pair launch.
    bool lists_forked = false;
    if (fork_lists) {
        if (c->pub.expected) c->pub.expected = 2;
        CHK(launch_search());
        HIPCHK(c, hipEventRecord(c->ev_lists, c->stream));              // (the masks are in place)
        CHK(launch_sift(false));
        // (enqueued behind the two big launches: a list kernel that starts beside the search takes CU slots the search counts on —
        // its blocks are all meant to be resident at once — and doubles it: 27 -> 54 us at 100 k atoms)
        CHK(join_upload_lists(c, true));           // (on the MAIN stream, before the two change places)
        HIPCHK(c, hipStreamWaitEvent(c->stream2, c->ev_sel, 0));
        std::swap(c->stream, c->stream2);
        int rc = ensure_center_grids(c);
        if (rc == ARP_OK) rc = ensure_plane_lists(c);
        std::swap(c->stream, c->stream2);
        CHK(rc);
        lists_forked = true;
    }
    // ---- ring / amide loops (I:938-1382): evaluated from the static candidate lists by the leading blocks of the
    // last launch (ARP_PLANES_MODE=1: as a kernel of their own on the second stream, beside the search)
    int n0 = 0, n1 = 0, n2 = 0, n3 = 0;
    if (with_planes && c->nring + c->namide > 0) {
        CHK(ensure_center_grids(c));
        CHK(ensure_plane_lists(c));
        CHK(prepare_atom_plane(c, ap, n0, /*contact_grid=*/true));   // (argument blocks and bag buffers; no grid is walked)
        CHK(prepare_plane_plane(c, pp, n1));
        CHK(prepare_group_group(c, gg, n2));
        CHK(prepare_group_plane(c, gp, n3));
    }
    const bool have_planes = n0 + n1 + n2 + n3 > 0;
    // blocks for the list evaluation: one wave per 64 entries, from what the lists held last time (their capacity at first)
    if (have_planes) {
        long long entries = 0;
        for (int k = 0; k < 4; ++k) entries += std::min<long long>((long long)c->plist[k].cap, c->plist_known[k] >= 0 ? c->plist_known[k] + 64 : (long long)c->plist[k].cap / 4);
        // Few, fat blocks: they and the sift blocks of the same launch must ALL be resident from the start (the sift
        // blocks split their work statically: one that had to wait for a slot would finish that much later than the rest),
        // so the sift part gets num_cu * blocks-per-CU minus these.  Sixteen list chunks (of 64 entries) per wave are still
        // inside the time the sift blocks need (sweep in profiles/README.md); ring-heavy structures get more blocks, up to half the slots.
        // ... and fewer when the sift part itself is short: a list chunk takes about as long as a batch of 64 pairs (2.3 vs 2.5-3 us
        // in the block traces of round 2, profiles/README.md), and a sift wave of a small structure has only a batch or two.
        const int64_t expect_pairs = (c->contacts_expected > 0) ? c->contacts_expected : (int64_t)c->n * 13;
        const double batches_per_wave = (double)expect_pairs / (64.0 * 4.0 * std::min<double>(c->num_cu * 4.0, std::max(1.0, expect_pairs / 256.0)));
        const int chunks_per_wave = std::max(2, std::min(sw().plane_cpw, (int)(sw().plane_chunk_factor * batches_per_wave + 0.5)));
        np = (int)std::min<long long>(std::max<long long>((entries + 256 * chunks_per_wave - 1) / (256 * chunks_per_wave), 8), 2 * c->num_cu);
        np = (np + 7) & ~7;
    }
    const bool merged = have_planes && c->n > 0 && !lists_forked && (sw().planes_mode == 0 || c->external_stream);
    const bool planes_alone = (have_planes && !merged) || lists_forked;   // (forked: launched whatever it holds — it ends the pass with the per-pair kernel)
    hipStream_t st2 = c->external_stream ? c->stream : c->stream2;   // a caller-owned stream: everything in order on it
    if (planes_alone && !lists_forked && c->pub.expected) c->pub.expected = (c->n > 0) ? 2 : 1;
    CHK(launch_search());
    if (planes_alone) {
        if (st2 != c->stream) {      // the ring / amide masks are made by the search launch (or by k_group_masks before it)
            if (!lists_forked) HIPCHK(c, hipEventRecord(c->ev_lists, c->stream));
            HIPCHK(c, hipStreamWaitEvent(st2, c->ev_lists, 0));
        }
        Prof p(c, SLOT_PLANES, st2);
        hipLaunchKernelGGL(k_planes, dim3(std::max(np, 8)), dim3(256), 0, st2, ap, pp, gg, gp, plane_lists(c), c->d_ctr + ctr_dev(C_PLIST), c->pub, 15);
        CHK(check_launch(c, "k_planes"));
    }
    if (c->n > 0) {
        if (!sift_launched) CHK(launch_sift(merged));
    } else if (!planes_alone) {
        c->pub.expected = 0;   // nothing was launched that could publish: the caller falls back to k_publish_counters
    }
    if (planes_alone && st2 != c->stream) {   // join: whatever follows on the main stream sees the bags
        HIPCHK(c, hipEventRecord(c->ev_planes, c->stream2));
        HIPCHK(c, hipStreamWaitEvent(c->stream, c->ev_planes, 0));
    }
    return ARP_OK;
}

// After read_counters(): publish contact results; returns true when the pair buffer overflowed.
bool finish_contacts(arp_ctx* c) {
    const u64 segcap = pair_segcap(c->pairs.cap);
    u64 np = 0, worst = 0;
    for (int k = 0; k < PAIR_SEGS; ++k) { np += c->h_ctr[C_SEG_PAIRS + k]; worst = std::max(worst, c->h_ctr[C_SEG_PAIRS + k]); }
    c->h_ctr[C_PAIRS] = np;
    c->h_ctr[C_SCRATCH0] = worst;
    for (int k = 0; k < PAIR_SEGS; ++k) c->seg_last[k] = c->h_ctr[C_SEG_PAIRS + k];
    if (worst > segcap) return true;
    c->n_contacts = (int64_t)np;
    c->contacts_expected = (int64_t)np;
    c->contacts_valid = true;
    c->contacts_sorted = false;
    void_results(c, RES_AA);
    c->stats[0] = (int64_t)c->h_ctr[C_CAND];
    c->stats[1] = (int64_t)c->h_ctr[C_ACC];
    c->stats[2] = (int64_t)np;
    if (c->cg_reused) c->h_ctr[C_BINNED] = (u64)c->cg_binned;         // (no grid build in this pass: the count its build reported)
    else if (c->cg_pending) { c->cg_binned = (int64_t)(uint32_t)c->h_ctr[C_BINNED]; c->cg_pending = false; }
    c->stats[3] = (int64_t)(uint32_t)c->h_ctr[C_BINNED];
    c->stats[4] = c->contact_cells;
    return false;
}

// ---- canonical order of the atom-atom bag (arp_sort.h) --------------------------------------------------------
// Layout of the sorted slab: the five columns one after the other, each on a 256-byte boundary; what follows them
// (sorted_extra bytes) is the caller's (the packed ring / amide bags of arp_fetch_packed).
void sorted_layout(size_t k, size_t off[5], size_t* bytes, size_t first_col_entries) {      // (first column: k bgn ids, or N + 1 row offsets)
    off[0] = 0;
    off[1] = off[0] + al256(first_col_entries * sizeof(int32_t));
    off[2] = off[1] + al256(k * sizeof(int32_t));
    off[3] = off[2] + al256(k * sizeof(float));
    off[4] = off[3] + al256(k * sizeof(uint16_t));
    *bytes = off[4] + al256(k * sizeof(uint8_t));
}
// A slab bound to the offsets of its columns — sorted_layout's or a table's (table_layout) —: col[q] is column q as whatever
// pointer it is assigned to.
struct Column {
    uint8_t* p;
    template <class T> operator T*() const { return (T*)p; }
};
struct Columns {
    uint8_t* slab;
    const size_t* off;
    Column operator[](int q) const { return Column{slab + off[q]}; }
};
// Canonical order of a bag by the radix sort of arp_sort.h: keys {first id << idbits | second id}, the other columns riding in
// the payload.  Radix passes over the bits of the first id — or, small_nbin > 0, ONE launch that groups the records by first id
// (k_sort_small, small_nbin ids) —, then the runs of equal first id ordered by the second in one launch (k_sort_runs).  A holds
// the columns in and out; the scratch is sized for cap >= k records.
int id_bits(int64_t idmax) {      // significant bits of the ids 0 ... idmax (at least one)
    int bits = 1;
    while (((int64_t)1 << bits) <= idmax) ++bits;
    return bits;
}
int radix_sort(arp_ctx* c, SortScratch& s, SortArgs& A, size_t k, size_t cap, int idbits, int small_nbin, const char* what) {
    const int passes = (idbits + SORT_MAX_BITS - 1) / SORT_MAX_BITS;
    HIPCHK(c, s.key[0].reserve(cap)); HIPCHK(c, s.val[0].reserve(cap));
    if (passes > 1) { HIPCHK(c, s.key[1].reserve(cap)); HIPCHK(c, s.val[1].reserve(cap)); }
    const long long tiles = ((long long)k + SORT_TILE - 1) / SORT_TILE;
    if (tiles > ((long long)1 << 30) / SORT_BINS) FAIL(c, ARP_E_CAPACITY, std::string(what) + ": too many records for the digit table");
    const int tstride = (int)((tiles + 3) & ~3ll);
    HIPCHK(c, s.table.reserve((size_t)SORT_BINS * (size_t)tstride));
    HIPCHK(c, s.total.reserve(SORT_BINS));
    A.n = (long long)k; A.T = (int)tiles; A.tstride = tstride; A.jbits = idbits;
    A.table = s.table.p; A.total = s.total.p;
    int last = 0;      // the key / payload buffer the last launch wrote
    if (small_nbin > 0) {
        A.key_out = s.key[0].p;
        A.val_out = s.val[0].p;
        hipLaunchKernelGGL(k_sort_small, dim3(std::min(sw().sort_small_blocks, small_nbin)), dim3(SORT_SMALL_THREADS), 0, c->stream, A, small_nbin);
    } else {
        int shift = idbits;
        for (int ps = 0; ps < passes; ++ps) {
            A.first = ps == 0; A.last = 0;
            A.shift = shift;
            A.bits = idbits / passes + (ps < idbits % passes ? 1 : 0);
            shift += A.bits;
            A.key_in = ps > 0 ? s.key[(ps - 1) & 1].p : nullptr;
            A.val_in = ps > 0 ? s.val[(ps - 1) & 1].p : nullptr;
            A.key_out = s.key[ps & 1].p;
            A.val_out = s.val[ps & 1].p;
            hipLaunchKernelGGL(k_sort_hist, dim3(A.T), dim3(SORT_THREADS), 0, c->stream, A);
            hipLaunchKernelGGL(k_sort_scan, dim3(1 << A.bits), dim3(SORT_THREADS), 0, c->stream, A);
            hipLaunchKernelGGL(k_sort_scatter, dim3(A.T), dim3(SORT_THREADS), 0, c->stream, A);
        }
        last = (passes - 1) & 1;
    }
    A.key_in = s.key[last].p;
    A.val_in = s.val[last].p;
    hipLaunchKernelGGL(k_sort_runs, dim3((unsigned)((k + 255) / 256)), dim3(256), 0, c->stream, A);
    return check_launch(c, what);
}
int sort_contacts(arp_ctx* c, size_t extra_bytes = 0) {
    if (!c->contacts_valid) FAIL(c, ARP_E_ARG, "arp_atom_contacts_sort: no atom-contact results (call a launch first)");
    const size_t k = (size_t)c->n_contacts;
    const bool csr = c->packed_csr && !c->has_gid;      // (a shard's records carry global ids: no table of rows)
    const size_t rows = (size_t)std::max<int64_t>(c->n, 0);
    size_t off[5], bytes;
    sorted_layout(k, off, &bytes, csr ? rows + 1 : k);
    if (c->contacts_sorted && c->sorted_is_csr == csr && c->sorted_slab.cap >= bytes + extra_bytes) return ARP_OK;
    {   // sized from the capacity of the unsorted columns, so that the slab is allocated once per structure size
        size_t off_cap[5], bytes_cap;
        sorted_layout(std::max(k, c->out_i.cap), off_cap, &bytes_cap, std::max(std::max(k, c->out_i.cap), rows + 1));
        HIPCHK(c, c->sorted_slab.reserve(std::max(bytes_cap, bytes + extra_bytes)));
    }
    for (int q = 0; q < 5; ++q) c->srt_off[q] = off[q];
    c->srt_bytes = bytes;
    c->sorted_is_csr = csr;
    if (k == 0) {
        if (csr) HIPCHK(c, hipMemsetAsync(c->sorted_slab.p + off[0], 0, (rows + 1) * sizeof(int32_t), c->stream));
        c->contacts_sorted = true;
        return ARP_OK;
    }
    if (k >= ((size_t)1 << 31)) FAIL(c, ARP_E_CAPACITY, "arp_atom_contacts_sort: 2^31 records or more (the digit table's prefixes are 32-bit)");
    // significant bits of an atom index: packed ids of the resident structure, global ids on a shard
    const int64_t idmax = c->has_gid ? (c->gid_max >= 0 ? c->gid_max : ((int64_t)1 << 31) - 1) : std::max<int64_t>(c->n - 1, 1);
    SortArgs A{};
    A.ci = c->out_i.p; A.cj = c->out_j.p;
    A.d_in = c->out_d.p; A.s_in = c->out_s.p; A.ct_in = c->out_ct.p;
    uint8_t* slab = c->sorted_slab.p;
    A.i_out = (int*)(slab + off[0]); A.j_out = (int*)(slab + off[1]); A.d_out = (float*)(slab + off[2]);
    A.s_out = (uint16_t*)(slab + off[3]); A.ct_out = slab + off[4];
    A.row_out = csr ? A.i_out : nullptr;
    A.nrows = (int)rows;
    // a small bag: one block groups the records by bgn atom in one launch (k_sort_small)
    const bool small = sw().sort_small && k <= (size_t)SORT_SMALL_MAX_RECORDS && idmax + 1 <= (int64_t)SORT_SMALL_MAX_BINS;
    CHK(radix_sort(c, c->sort_aa, A, k, std::max(k, c->out_i.cap), id_bits(idmax), small ? (int)idmax + 1 : 0, "arp_atom_contacts_sort"));
    c->contacts_sorted = true;
    return ARP_OK;
}
// static candidate lists: entry counts travel with the counters of the pass; a list that was too small is re-sized and
// rebuilt before the pass is repeated
int finish_plane_lists(arp_ctx* c, bool grow) {
    if (!c->plist_count.p || c->nring + c->namide == 0) return 0;
    int again = 0;
    for (int k = 0; k < 4; ++k) {
        const u64 cnt = c->h_ctr[C_PLIST + k];
        c->plist_known[k] = (long long)cnt;
        if (cnt > (u64)c->plist[k].cap) {
            again = 1;
            if (grow) {
                c->plist[k].release();
                HIPCHK(c, c->plist[k].reserve((size_t)cnt + (size_t)cnt / 8 + 64));
                c->lists_dirty = true;
            }
        }
    }
    return again;
}
bool finish_bag(arp_ctx* c, int kind) {
    Bag& b = c->bag[kind];
    const u64 k = c->h_ctr[PLANE_TABLES[kind].counter];
    if (k > b.cap) return true;
    b.count = (int64_t)k;
    b.valid = true;
    ++b.version;
    void_results(c, RES_PLANES);
    return false;
}
int grow_pairs(arp_ctx* c) {
    const size_t need = ((size_t)c->h_ctr[C_SCRATCH0] + (size_t)c->h_ctr[C_SCRATCH0] / 8 + 64) * PAIR_SEGS;
    c->pairs.release(); c->out_i.release(); c->out_j.release(); c->out_d.release(); c->out_s.release(); c->out_ct.release();
    HIPCHK(c, c->pairs.reserve(need));
    return ARP_OK;
}
int grow_bag(arp_ctx* c, int kind) { return bag_reserve(c, kind, (size_t)c->h_ctr[PLANE_TABLES[kind].counter]); }
int device_error(arp_ctx* c) {
    if ((int)(uint32_t)c->h_ctr[C_ERR] == ARP_E_XBOND_NBR)
        FAIL(c, ARP_E_XBOND_NBR, "xbond donor without a single-bond heavy neighbour (reference: AttributeError at utils.py:173)");
    if ((int)(uint32_t)c->h_ctr[C_ERR] == ARP_E_HIP)
        FAIL(c, ARP_E_HIP, "the grid's prefix scan timed out waiting for another tile (device shared or partly masked?): results of this pass are invalid; "
                           "ARP_CHAINED_SCAN=0 selects the two-launch scan");
    return ARP_OK;
}

// One ring / amide loop alone (arp_plane_plane_launch ...) from the static candidate lists of the structure, like the loops of a
// whole pass: the entries of the list in chunks of 64 over the waves of ONE launch (k_planes with the other three kinds masked
// out) — a launch of >= 1024 waves that each take a chunk or two, instead of one wave per ring / amide walking its 27-cell
// stencil as a chain of dependent loads (the grid walks of arp_planes.h, which the lists are built by: 10 k rings took 22 - 37 us).
// kind: 0 atom-plane, 1 plane-plane, 2 group-group, 3 group-plane.
int enqueue_bag_from_lists(arp_ctx* c, int kind) {
    AtomPlaneArgs ap{};
    PlanePlaneArgs pp{};
    GroupGroupArgs gg{};
    GroupPlaneArgs gp{};
    int nb = 0;
    if (c->n > 0 && kind == 0) CHK(ensure_static(c, c->last_cutoff));      // (the atoms' records by local id: st_xyzm)
    CHK(ensure_center_grids(c));
    CHK(ensure_plane_lists(c));
    if (kind == 0) CHK(prepare_atom_plane(c, ap, nb, /*contact_grid=*/true));
    else if (kind == 1) CHK(prepare_plane_plane(c, pp, nb));
    else if (kind == 2) CHK(prepare_group_group(c, gg, nb));
    else CHK(prepare_group_plane(c, gp, nb));
    if (!nb) return ARP_OK;
    const long long entries = std::min<long long>((long long)c->plist[kind].cap, c->plist_known[kind] >= 0 ? c->plist_known[kind] + 64 : (long long)c->plist[kind].cap);
    // one chunk of 64 entries per wave while the chip has room (8 waves per SIMD), more beyond
    const int blocks = (int)std::min<long long>(std::max<long long>((entries + 255) / 256, 8), (long long)c->num_cu * 8);
    Prof p(c, SLOT_PLANES, c->stream);
    hipLaunchKernelGGL(k_planes, dim3(blocks), dim3(256), 0, c->stream, ap, pp, gg, gp, plane_lists(c), c->d_ctr + ctr_dev(C_PLIST), PublishArgs{nullptr, nullptr, 0, 0}, 1 << kind);
    return check_launch(c, "k_planes (one list)");
}
// One ring / amide loop alone (arp_*_launch), from its candidate list or by its grid walk (ARP_BAG_LISTS), once more while a
// bag or a list was too small (re-sized: a list is rebuilt by the next attempt)
int bag_launch(arp_ctx* c, int kind, int64_t* count) {
    const bool from_lists = ((sw().bag_lists >> kind) & 1) != 0;
    HIPCHK(c, hipSetDevice(c->device));
    CHK(ensure_default_selection(c));
    for (int attempt = 0;; ++attempt) {
        CHK(from_lists ? enqueue_bag_from_lists(c, kind) : enqueue_bag_walk(c, kind));
        CHK(read_counters(c));
        collect_events(c);
        const bool list_small = from_lists && finish_plane_lists(c, /*grow=*/true) != 0;
        const bool bag_small = finish_bag(c, kind);
        if (!list_small && !bag_small) break;
        if (attempt == (from_lists ? 3 : 2)) FAIL(c, ARP_E_CAPACITY, "result bag could not be sized");
        if (bag_small) CHK(grow_bag(c, kind));
    }
    if (count) *count = c->bag[kind].count;
    return ARP_OK;
}

// The end of a whole pass (arp_run_wait, arp_run_stage), after its counters have arrived: publish every result and re-size what
// was too small.  Returns 1 when the pass must run again, 0 when it is done, < 0 on an error.
int finish_pass(arp_ctx* c) {
    int again = 0;
    if (finish_contacts(c)) { CHK(grow_pairs(c)); again = 1; }
    for (int kind = 0; kind < BAG_KINDS; ++kind)
        if (finish_bag(c, kind)) { CHK(grow_bag(c, kind)); again = 1; }
    const int lists = finish_plane_lists(c, true);
    if (lists < 0) return lists;
    return again | lists;
}
void pass_counts(arp_ctx* c, int64_t counts[5]) {      // expansion statistics and record counts of a finished pass
    c->stats[5] = (int64_t)c->h_ctr[C_MARK_CAND];
    c->stats[6] = (int64_t)c->h_ctr[C_MARK_ACC];
    if (counts) {
        counts[0] = c->n_contacts;
        for (int b = 0; b < BAG_KINDS; ++b) counts[1 + b] = c->bag[PACKED_ORDER[b]].count;
    }
}

}  // namespace

// =====================================================================================
extern "C" {

const char* arp_version(void) { return "arpeggio_hip 0.2.0 (gfx950)"; }

int arp_device_count(void) {
    int n = 0;
    return hipGetDeviceCount(&n) == hipSuccess ? n : 0;
}

int arp_device_synchronize(arp_ctx* c) {
    if (!c) return ARP_E_ARG;
    HIPCHK(c, hipSetDevice(c->device));
    HIPCHK(c, hipDeviceSynchronize());
    return ARP_OK;
}

int arp_create(int device, arp_ctx** out) {
    if (!out) return ARP_E_ARG;
    *out = nullptr;
    int ndev = 0;
    hipError_t e = hipGetDeviceCount(&ndev);
    if (e != hipSuccess || ndev <= 0) {
        set_create_error(std::string("no HIP device available: ") + (e != hipSuccess ? hipGetErrorString(e) : "device count is 0"));
        return ARP_E_HIP;
    }
    if (device < 0 || device >= ndev) {
        set_create_error("device ordinal out of range");
        return ARP_E_ARG;
    }
    e = hipSetDevice(device);
    if (e != hipSuccess) { set_create_error(hipGetErrorString(e)); return ARP_E_HIP; }
    arp_ctx* c = new (std::nothrow) arp_ctx();
    if (!c) return ARP_E_NOMEM;
    c->device = device;
    // the fused scan + scatter keeps the whole start table in LDS: up to 144 KB of the CU's 160 KB
    (void)hipFuncSetAttribute((const void*)k_scan_scatter_atoms<4>, hipFuncAttributeMaxDynamicSharedMemorySize, 4 * 16384);
    (void)hipFuncSetAttribute((const void*)k_scan_scatter_atoms<5>, hipFuncAttributeMaxDynamicSharedMemorySize, 5 * 16384);
    (void)hipFuncSetAttribute((const void*)k_scan_scatter_atoms<6>, hipFuncAttributeMaxDynamicSharedMemorySize, 6 * 16384);
    (void)hipFuncSetAttribute((const void*)k_scan_scatter_atoms<7>, hipFuncAttributeMaxDynamicSharedMemorySize, 7 * 16384);
    (void)hipFuncSetAttribute((const void*)k_scan_scatter_atoms<8>, hipFuncAttributeMaxDynamicSharedMemorySize, 8 * 16384);
    (void)hipFuncSetAttribute((const void*)k_scan_scatter_atoms<9>, hipFuncAttributeMaxDynamicSharedMemorySize, 9 * 16384);
    hipDeviceProp_t prop;
    if (hipGetDeviceProperties(&prop, device) == hipSuccess) c->num_cu = prop.multiProcessorCount;
    {
        int per_cu = 0;
        if (hipOccupancyMaxActiveBlocksPerMultiprocessor(&per_cu, (const void*)k_search<MODE_CONTACTS>, 64 * SEARCH_WAVES, 0) == hipSuccess && per_cu > 0)
            c->search_resident = per_cu * c->num_cu;
        per_cu = 0;
        if (hipOccupancyMaxActiveBlocksPerMultiprocessor(&per_cu, (const void*)k_sift_planes<0, 0>, 256, 0) == hipSuccess && per_cu > 0)
            c->sift_per_cu = per_cu;
    }
    e = hipStreamCreateWithFlags(&c->own_stream, hipStreamNonBlocking);
    c->stream = c->own_stream;
    if (e == hipSuccess) {   // the second stream (ring / amide kernel) yields to the main one
        int lo_prio = 0, hi_prio = 0;
        (void)hipDeviceGetStreamPriorityRange(&lo_prio, &hi_prio);
        e = hipStreamCreateWithPriority(&c->stream2, hipStreamNonBlocking, lo_prio);
    }
    if (e == hipSuccess) e = hipEventCreateWithFlags(&c->ev_sel, hipEventDisableTiming);
    if (e == hipSuccess) e = hipEventCreateWithFlags(&c->ev_planes, hipEventDisableTiming);
    if (e == hipSuccess) e = hipEventCreateWithFlags(&c->ev_lists, hipEventDisableTiming);
    if (e == hipSuccess) e = hipEventCreateWithFlags(&c->ev_upload, hipEventDisableTiming);
    if (e == hipSuccess) e = hipEventCreateWithFlags(&c->ev_uplists, hipEventDisableTiming);
    if (e == hipSuccess) e = hipMalloc((void**)&c->d_ctr, sizeof(u64) * C_DEV_WORDS);
    if (e == hipSuccess) e = hipMemset(c->d_ctr, 0, sizeof(u64) * C_DEV_WORDS);
    if (e == hipSuccess) e = hipHostMalloc((void**)&c->h_ctr_pinned, sizeof(u64) * (C_COUNT + 1), hipHostMallocDefault);
    if (e == hipSuccess) memset(c->h_ctr_pinned, 0, sizeof(u64) * (C_COUNT + 1));
    if (e != hipSuccess) {
        set_create_error(hipGetErrorString(e));
        delete c;
        return ARP_E_HIP;
    }
    {   // k_sift deals its blocks to the pair-list segments by (XCD, blockIdx / 8): exact only if consecutive blocks of a launch go
        // round-robin over eight XCDs (up to a rotation).  Looked at once; otherwise the blocks are dealt out by index (seg_by_block).
        int* probe = nullptr;
        int h_probe[64];
        bool rr = false;
        if (hipMalloc((void**)&probe, sizeof(h_probe)) == hipSuccess) {
            hipLaunchKernelGGL(k_xcc_probe, dim3(64), dim3(64), 0, c->stream, probe);
            if (hipMemcpyAsync(h_probe, probe, sizeof(h_probe), hipMemcpyDeviceToHost, c->stream) == hipSuccess && hipStreamSynchronize(c->stream) == hipSuccess) {
                rr = true;
                for (int b = 0; b < 64; ++b) rr = rr && ((h_probe[b] - h_probe[0] - b) & 7) == 0;
            }
            (void)hipFree(probe);
        }
        (void)hipGetLastError();
        c->xcd_round_robin = rr && !sw().sift_seg_by_block;
    }
    *out = c;
    return ARP_OK;
}

void arp_destroy(arp_ctx* c) {
    if (c && c->comm) { (void)rccl().CommDestroy(c->comm); c->comm = nullptr; }
    if (!c) return;
    (void)hipSetDevice(c->device);
    if (c->stream) (void)hipStreamSynchronize(c->stream);
    if (c->stream2) (void)hipStreamSynchronize(c->stream2);
    for (auto& e : c->ev_pool) { (void)hipEventDestroy(e.a); (void)hipEventDestroy(e.b); }
    c->xyz.release(); c->rad.release(); c->tmask.release(); c->flags.release(); c->res_id.release();
    c->res_prev.release(); c->res_next.release(); c->res_flags.release(); c->bond_off.release();
    c->bond_idx.release(); c->h_off.release(); c->h_xyz_d.release(); c->sb.release(); c->gid.release();
    c->home.release(); c->sel.release(); c->plus.release(); c->res_sel.release(); c->res_plus.release();
    c->ring_c.release(); c->ring_n.release(); c->ring_res.release(); c->ring_sel.release(); c->ring_plus.release();
    c->am_c.release(); c->am_n.release(); c->am_res.release(); c->am_sel.release(); c->am_plus.release();
    c->s_xyzm.release(); c->s_aux.release(); c->s_qa.release(); c->tmp_i32.release(); c->sel_list.release(); c->st_qa.release(); c->rad_idx.release(); c->rad_tab.release(); c->st_aux.release(); c->st_xyzm.release();
    c->upload_bad.release(); c->sb_tile.release(); c->sb_cw.release(); c->sb_cwp.release(); c->sb_sums.release();
    c->sp_xyzm.release(); c->sp_aux.release(); c->sp_qa.release(); c->st_h.release(); c->sp_h.release(); c->s_h.release(); c->sp_cnt.release(); c->sp_cr.release();
    c->atom_grid.release(); c->all_grid.release(); c->a_xyzm.release(); c->a_aux.release(); c->ring_grid.release(); c->amide_grid.release(); c->tmp_u8.release();
    c->pairs.release(); c->out_i.release(); c->out_j.release(); c->out_d.release(); c->out_s.release(); c->out_ct.release();
    for (Bag& b : c->bag) b.release();
    c->bag_pack.release(); c->bag_perm.release();
    c->sort_aa.release(); c->sort_bags.release(); c->sorted_slab.release();
    c->table_sort.release(); c->table_tiles.release(); c->table_rows.release(); c->table_total.release();
    c->persist.slab.release(); c->respair.slab.release(); c->respersist.slab.release();
    c->filtered.cols.release(); c->filtered.slab.release();
    c->bridges.slab.release(); c->bridge_off.release(); c->bridge_res.release();
    c->bridgepersist.slab.release();
    c->lifetimes.slab.release();
    c->networks.slab.release(); c->net_label.release(); c->net_scratch.release();
    c->similarity.bits.release(); c->similarity.inter.release();
    c->poses.release();
    c->pplanes.release();
    c->posefp.release();
    c->shortlist.release();
    c->libshortlist.release();
    c->clusters.release();
    c->libclusters.release();
    c->libbridges.release();
    c->library.release();
    c->libres.release();
    c->libfp.release();
    c->libfpx.release();
    c->libplanes.release();
    c->libpl.release();
    c->sb_idx.release();
    c->coupling.slab.release(); c->couple.rowbits.release(); c->couple.bits.release(); c->couple.n_row.release(); c->couple.n.release();
    if (c->table_stage) (void)hipHostFree(c->table_stage);
    if (c->bag_stage) (void)hipHostFree(c->bag_stage);
    c->res_tag.release(); c->blob_sb_nbr.release(); c->blob_dev.release(); c->longest_bond.release();
    c->rec_home.release(); c->rec_face[0].release(); c->rec_face[1].release(); c->sh_scan.release(); c->sh_src.release();
    c->origin.release(); c->ring_origin.release(); c->am_origin.release(); c->sh_sel.release();
    release_batch_tables(c);
    for (auto& g : c->batch_grid) g.place.release();
    c->sid_atom.release(); c->sid_ring.release(); c->sid_amide.release(); c->batch_off_dev.release();
    for (auto& l : c->plist) l.release();
    c->plist_count.release();   // (views into the blob were released above: no-ops)
    c->ring_home.release(); c->am_home.release(); c->ring_gid.release(); c->am_gid.release();
    if (c->h_ctr_pinned) (void)hipHostFree(c->h_ctr_pinned);
    if (c->d_ctr) (void)hipFree(c->d_ctr);
    if (c->ev_sel) (void)hipEventDestroy(c->ev_sel);
    if (c->ev_planes) (void)hipEventDestroy(c->ev_planes);
    if (c->ev_lists) (void)hipEventDestroy(c->ev_lists);
    if (c->ev_upload) (void)hipEventDestroy(c->ev_upload);
    if (c->ev_uplists) (void)hipEventDestroy(c->ev_uplists);
    if (c->stream2) (void)hipStreamDestroy(c->stream2);
    if (c->own_stream) (void)hipStreamDestroy(c->own_stream);
    delete c;
}

const char* arp_last_error(arp_ctx* c) { return c ? c->err.c_str() : g_create_error.c_str(); }

// ---- inputs --------------------------------------------------------------------------
int arp_set_atoms(arp_ctx* c, int64_t n, const float* xyz, const double* vdw, const double* cov, const uint16_t* type_mask,
                  const uint16_t* flags, const int32_t* res_id) {
    if (!c) return ARP_E_ARG;
    CHK(join_upload_lists(c));
    if (n < 0 || n > 0x7FFFFFF0LL) FAIL(c, ARP_E_ARG, "arp_set_atoms: n out of range");
    if (n > 0 && (!xyz || !vdw || !cov || !type_mask || !flags || !res_id)) FAIL(c, ARP_E_ARG, "arp_set_atoms: null input");
    // the grids are sized from the bounding box: a NaN / inf coordinate has no cell
    if (!all_finite(xyz, 3 * n)) FAIL(c, ARP_E_ARG, "arp_set_atoms: non-finite coordinate");
    c->blob_bytes = 0;           // the resident structure no longer is the blob that was uploaded / assembled
    c->shard_resident = false;
    if (!all_finite(vdw, n) || !all_finite(cov, n)) FAIL(c, ARP_E_ARG, "arp_set_atoms: non-finite radius");
    int64_t max_res = -1;
    for (int64_t i = 0; i < n; ++i) {
        if (res_id[i] < 0) FAIL(c, ARP_E_ARG, "arp_set_atoms: negative residue index");
        max_res = std::max<int64_t>(max_res, res_id[i]);
    }
    c->max_res_id = max_res;
    HIPCHK(c, hipSetDevice(c->device));
    // uploads below are enqueued together; whatever the exit path, they are complete before the staging vectors die
    struct SyncOnExit { arp_ctx* c; ~SyncOnExit() { (void)hipStreamSynchronize(c->stream); } } sync_on_exit{c};
    inputs_changed(c, IN_ATOMS);
    c->sb_index_src = 0;         // (of the atoms before: arp_set_single_bond_neighbours follows)
    c->n = n;
    c->h_xyz.assign(xyz, xyz + 3 * n);
    points_box(xyz, n, c->lo, c->hi);
    std::vector<float4> x4((size_t)n);
    std::vector<double2> r2((size_t)n);
    for (int64_t i = 0; i < n; ++i) {
        x4[i] = make_float4(xyz[3 * i], xyz[3 * i + 1], xyz[3 * i + 2], 0.f);
        r2[i] = make_double2(vdw[i], cov[i]);
    }
    CHK(upload_async(c, c->xyz, x4.data(), (size_t)n));
    CHK(upload_async(c, c->rad, r2.data(), (size_t)n));
    {   // dictionary of the distinct {vdw, cov} pairs (element values: a handful per structure), compared bit for bit
        std::vector<double2> tab((size_t)RAD_TABLE, make_double2(0.0, 0.0));
        std::vector<uint16_t> idx((size_t)std::max<int64_t>(n, 1), (uint16_t)RAD_NONE);
        std::vector<std::pair<uint64_t, uint64_t>> keys;   // bit patterns, in table order
        int last = 0;
        for (int64_t i = 0; i < n; ++i) {
            uint64_t kv, kc;
            memcpy(&kv, &vdw[i], 8);
            memcpy(&kc, &cov[i], 8);
            int hit = -1;
            if (!keys.empty() && keys[(size_t)last].first == kv && keys[(size_t)last].second == kc) hit = last;
            for (size_t k = 0; hit < 0 && k < keys.size(); ++k)
                if (keys[k].first == kv && keys[k].second == kc) hit = (int)k;
            if (hit < 0) {
                if ((int)keys.size() >= RAD_TABLE) continue;   // stays RAD_NONE: k_sift fetches the uploaded radii
                hit = (int)keys.size();
                keys.emplace_back(kv, kc);
                tab[(size_t)hit] = make_double2(vdw[i], cov[i]);
            }
            last = hit;
            idx[(size_t)i] = (uint16_t)hit;
        }
        CHK(upload_async(c, c->rad_idx, idx.data(), (size_t)std::max<int64_t>(n, 1)));
        CHK(upload_async(c, c->rad_tab, tab.data(), (size_t)RAD_TABLE));
        CHK(upload_done(c));   // tab / idx go out of scope here
    }
    CHK(upload_async(c, c->tmask, type_mask, (size_t)n));
    CHK(upload_async(c, c->flags, flags, (size_t)n));
    CHK(upload_async(c, c->res_id, res_id, (size_t)n));
    // defaults for the optional per-atom inputs: no bonds, no hydrogens, no neighbours
    std::vector<int> zeros((size_t)n + 1, 0);
    CHK(upload_async(c, c->bond_off, zeros.data(), (size_t)n + 1));
    CHK(upload_async(c, c->h_off, zeros.data(), (size_t)n + 1));
    HIPCHK(c, c->bond_idx.reserve(1));
    HIPCHK(c, c->h_xyz_d.reserve(3));
    std::vector<float4> sb0((size_t)n, make_float4(0, 0, 0, 0));
    CHK(upload_async(c, c->sb, sb0.data(), (size_t)n));
    CHK(upload_done(c));   // (the staging vectors above live until here)
    c->has_gid = c->has_home = false;
    c->gid_max = -1;
    return ARP_OK;
}

int arp_set_residues(arp_ctx* c, int64_t nres, const uint8_t* res_flags, const int32_t* prev, const int32_t* next) {
    if (!c) return ARP_E_ARG;
    if (nres < 0 || (nres > 0 && (!res_flags || !prev || !next))) FAIL(c, ARP_E_ARG, "arp_set_residues: bad input");
    if (nres <= c->max_res_id) FAIL(c, ARP_E_ARG, "arp_set_residues: an atom refers to a residue beyond the table");
    HIPCHK(c, hipSetDevice(c->device));
    inputs_changed(c, IN_RESIDUES);
    c->nres = nres;
    CHK(upload(c, c->res_flags, res_flags, (size_t)nres));
    CHK(upload(c, c->res_prev, prev, (size_t)nres));
    CHK(upload(c, c->res_next, next, (size_t)nres));
    c->has_res = true;
    return ARP_OK;
}

int arp_set_bonds(arp_ctx* c, const int32_t* bond_off, const int32_t* bond_idx) {
    if (!c || !bond_off) return ARP_E_ARG;
    HIPCHK(c, hipSetDevice(c->device));
    inputs_changed(c, IN_BONDS);
    if (!csr_ok(bond_off, c->n)) FAIL(c, ARP_E_ARG, "arp_set_bonds: offsets must start at 0 and never decrease");
    const int64_t m = bond_off[c->n];
    if (m < 0 || (m > 0 && !bond_idx)) FAIL(c, ARP_E_ARG, "arp_set_bonds: bad CSR");
    CHK(upload(c, c->bond_off, bond_off, (size_t)c->n + 1));
    CHK(upload(c, c->bond_idx, bond_idx, (size_t)m));
    return ARP_OK;
}

int arp_set_hydrogens(arp_ctx* c, const int32_t* h_off, const double* h_xyz) {
    if (!c || !h_off) return ARP_E_ARG;
    HIPCHK(c, hipSetDevice(c->device));
    inputs_changed(c, IN_HYDROGENS);
    if (!csr_ok(h_off, c->n)) FAIL(c, ARP_E_ARG, "arp_set_hydrogens: offsets must start at 0 and never decrease");
    const int64_t m = h_off[c->n];
    if (m < 0 || (m > 0 && !h_xyz)) FAIL(c, ARP_E_ARG, "arp_set_hydrogens: bad CSR");
    CHK(upload(c, c->h_off, h_off, (size_t)c->n + 1));
    CHK(upload(c, c->h_xyz_d, h_xyz, (size_t)m * 3));
    return ARP_OK;
}

int arp_set_single_bond_neighbours(arp_ctx* c, const int32_t* sb_nbr) {
    if (!c || (c->n > 0 && !sb_nbr)) return ARP_E_ARG;
    HIPCHK(c, hipSetDevice(c->device));
    inputs_changed(c, IN_NEIGHBOURS);
    for (int64_t i = 0; i < c->n; ++i)
        if (sb_nbr[i] < -1 || sb_nbr[i] >= c->n) FAIL(c, ARP_E_ARG, "arp_set_single_bond_neighbours: index out of range");
    // the neighbour's coordinates are gathered on the device from the uploaded atoms (x, y, z, 1) / (0, 0, 0, 0)
    // (the index stays resident: a pose that moves the neighbour moves these coordinates with it, arp_poses.h)
    CHK(upload(c, c->sb_idx, sb_nbr, (size_t)c->n));
    c->sb_index_src = 1;
    HIPCHK(c, c->sb.reserve((size_t)std::max<int64_t>(c->n, 1)));
    if (c->n > 0) {
        hipLaunchKernelGGL(k_gather_neighbours, dim3(nblocks(c->n, 256)), dim3(256), 0, c->stream, (int)c->n, c->sb_idx.p, c->xyz.p, c->sb.p);
        CHK(check_launch(c, "k_gather_neighbours"));
        HIPCHK(c, hipStreamSynchronize(c->stream));
    }
    return ARP_OK;
}

int arp_set_rings(arp_ctx* c, int64_t nring, const double* center, const double* normal, const int32_t* ring_res) {
    if (!c) return ARP_E_ARG;
    CHK(join_upload_lists(c));
    if (nring < 0 || (nring > 0 && (!center || !normal || !ring_res))) FAIL(c, ARP_E_ARG, "arp_set_rings: bad input");
    if (!all_finite(center, 3 * nring)) FAIL(c, ARP_E_ARG, "arp_set_rings: non-finite ring centre");   // (normals may be NaN: class '')
    c->max_ring_res = -1;
    for (int64_t i = 0; i < nring; ++i) {
        if (ring_res[i] < -1) FAIL(c, ARP_E_ARG, "arp_set_rings: residue index below -1");
        c->max_ring_res = std::max<int64_t>(c->max_ring_res, ring_res[i]);
    }
    HIPCHK(c, hipSetDevice(c->device));
    inputs_changed(c, IN_RINGS);
    c->nring = nring;
    points_box(center, nring, c->ring_lo, c->ring_hi);
    CHK(upload(c, c->ring_c, center, (size_t)nring * 3));
    CHK(upload(c, c->ring_n, normal, (size_t)nring * 3));
    CHK(upload(c, c->ring_res, ring_res, (size_t)nring));
    HIPCHK(c, c->ring_sel.reserve((size_t)std::max<int64_t>(nring, 1)));
    HIPCHK(c, c->ring_plus.reserve((size_t)std::max<int64_t>(nring, 1)));
    c->has_group_owner = false;
    return ARP_OK;
}

int arp_set_amides(arp_ctx* c, int64_t namide, const float* center, const float* normal, const int32_t* amide_res) {
    if (!c) return ARP_E_ARG;
    CHK(join_upload_lists(c));
    if (namide < 0 || (namide > 0 && (!center || !normal || !amide_res))) FAIL(c, ARP_E_ARG, "arp_set_amides: bad input");
    if (!all_finite(center, 3 * namide)) FAIL(c, ARP_E_ARG, "arp_set_amides: non-finite amide centre");
    c->max_amide_res = -1;
    for (int64_t i = 0; i < namide; ++i) {
        if (amide_res[i] < -1) FAIL(c, ARP_E_ARG, "arp_set_amides: residue index below -1");
        c->max_amide_res = std::max<int64_t>(c->max_amide_res, amide_res[i]);
    }
    HIPCHK(c, hipSetDevice(c->device));
    inputs_changed(c, IN_AMIDES);
    c->namide = namide;
    points_box(center, namide, c->am_lo, c->am_hi);
    CHK(upload(c, c->am_c, center, (size_t)namide * 3));
    CHK(upload(c, c->am_n, normal, (size_t)namide * 3));
    CHK(upload(c, c->am_res, amide_res, (size_t)namide));
    HIPCHK(c, c->am_sel.reserve((size_t)std::max<int64_t>(namide, 1)));
    HIPCHK(c, c->am_plus.reserve((size_t)std::max<int64_t>(namide, 1)));
    c->has_group_owner = false;
    return ARP_OK;
}

// ---- one-blob upload (layout, names of the arrays and the host packer: arp_blob.h) -------------------------------------------
namespace {
// header of a blob: counts, size and offsets as arp_blob_layout writes them, finite boxes
int check_blob_header(arp_ctx* c, const arp_blob_header& h, uint64_t bytes) {
    if (h.magic != ARP_BLOB_MAGIC) FAIL(c, ARP_E_ARG, "arp_set_blob: bad magic");
    arp_blob_header want;
    if (!blob_header(h.n, h.nres, h.nbond, h.nh, h.nring, h.namide, want)) FAIL(c, ARP_E_ARG, "arp_set_blob: counts out of range");
    if (h.bytes != want.bytes || h.bytes > bytes) FAIL(c, ARP_E_ARG, "arp_set_blob: size does not match the counts");
    if (memcmp(h.off, want.off, sizeof(h.off)) != 0) FAIL(c, ARP_E_ARG, "arp_set_blob: unexpected array offset");
    if (h.n_rad < 0 || h.n_rad > RAD_TABLE) FAIL(c, ARP_E_ARG, "arp_set_blob: n_rad out of range");
    if (h.n > 0 && h.nres <= 0) FAIL(c, ARP_E_ARG, "arp_set_blob: atoms without a residue table");
    for (int k = 0; k < 3; ++k) {
        const bool ok = std::isfinite(h.lo[k]) && std::isfinite(h.hi[k]) && h.lo[k] <= h.hi[k] && std::isfinite(h.ring_lo[k]) &&
                        std::isfinite(h.ring_hi[k]) && h.ring_lo[k] <= h.ring_hi[k] && std::isfinite(h.amide_lo[k]) &&
                        std::isfinite(h.amide_hi[k]) && h.amide_lo[k] <= h.amide_hi[k];
        if (!ok) FAIL(c, ARP_E_ARG, "arp_set_blob: bad bounding box");
    }
    return ARP_OK;
}

// the input arrays of the context become views into c->blob_dev (which holds, or is about to hold, a blob with header h)
void borrow_blob_views(arp_ctx* c, const arp_blob_header& h) {
    uint8_t* const d = c->blob_dev.p;
    const size_t n1 = (size_t)std::max<int64_t>(h.n, 1);
    auto at = [&](BlobArray a) { return d + h.off[a]; };
    auto atleast1 = [](int64_t v) { return (size_t)std::max<int64_t>(v, 1); };
    c->xyz.borrow(at(BLOB_XYZ), n1); c->rad.borrow(at(BLOB_RAD), n1); c->tmask.borrow(at(BLOB_TMASK), n1);
    c->flags.borrow(at(BLOB_FLAGS), n1); c->res_id.borrow(at(BLOB_RES_ID), n1);
    c->res_flags.borrow(at(BLOB_RES_FLAGS), atleast1(h.nres)); c->res_prev.borrow(at(BLOB_RES_PREV), atleast1(h.nres));
    c->res_next.borrow(at(BLOB_RES_NEXT), atleast1(h.nres));
    c->bond_off.borrow(at(BLOB_BOND_OFF), (size_t)h.n + 1); c->bond_idx.borrow(at(BLOB_BOND_IDX), atleast1(h.nbond));
    c->h_off.borrow(at(BLOB_H_OFF), (size_t)h.n + 1); c->h_xyz_d.borrow(at(BLOB_H_XYZ), (size_t)std::max<int64_t>(3 * h.nh, 3));
    c->blob_sb_nbr.borrow(at(BLOB_SB_NBR), n1);
    c->sb_index_src = 2;
    c->ring_c.borrow(at(BLOB_RING_C), atleast1(3 * h.nring)); c->ring_n.borrow(at(BLOB_RING_N), atleast1(3 * h.nring));
    c->ring_res.borrow(at(BLOB_RING_RES), atleast1(h.nring));
    c->am_c.borrow(at(BLOB_AMIDE_C), atleast1(3 * h.namide)); c->am_n.borrow(at(BLOB_AMIDE_N), atleast1(3 * h.namide));
    c->am_res.borrow(at(BLOB_AMIDE_RES), atleast1(h.namide));
    c->rad_idx.borrow(at(BLOB_RAD_IDX), n1); c->rad_tab.borrow(at(BLOB_RAD_TAB), (size_t)RAD_TABLE);
    c->n = h.n; c->nres = h.nres; c->nring = h.nring; c->namide = h.namide;
    c->has_res = true;
    c->blob_nbond = h.nbond; c->blob_nh = h.nh; c->blob_nrad = h.n_rad;
    c->blob_bytes = h.bytes;
    c->max_res_id = h.nres - 1; c->max_ring_res = h.nres - 1; c->max_amide_res = h.nres - 1;   // (ranges verified on the device)
    for (int k = 0; k < 3; ++k) {
        c->lo[k] = h.lo[k]; c->hi[k] = h.hi[k];
        c->ring_lo[k] = h.ring_lo[k]; c->ring_hi[k] = h.ring_hi[k];
        c->am_lo[k] = h.amide_lo[k]; c->am_hi[k] = h.amide_hi[k];
    }
    c->h_xyz.clear();
}

// No structure is resident any more (a failed upload: the arrays it overwrote are void).
void drop_resident(arp_ctx* c) {
    c->uplists_pending = false;
    inputs_changed(c, IN_EVERYTHING);
    c->n = c->nres = c->nring = c->namide = 0;
    c->blob_bytes = 0;
    c->sp_radius = 0;
    c->sel_prefilled = false; c->sp_cnt_zeroed = 0;
    c->ctr_zero_ok = false;
}

// Device-side validation of the resident blob (what arp_set_atoms ... check on the host) + the bookkeeping of a new
// structure.  Waits for the stream.  `also` = further device error words OR-ed in (shard assembly), may be null.
// batch_next: the caller declares a batch partition next (arp_set_models), so nothing is made ahead for ONE structure.
int validate_resident_blob(arp_ctx* c, const arp_blob_header& h, const char* who, const int* also = nullptr, bool gather_sb = false, bool rad_from_table = false,
                           bool batch_next = false) {
    int* const d_err = (int*)(c->d_ctr + ctr_dev(C_ERR));
    const bool after_batch = c->batch_n > 0 || batch_next;      // (before the bookkeeping below resets it)
    // The verdict reaches the host the way the counters of a pass do: the last block of the kernel stores the counter block in
    // the pinned mirror and the host polls the completion word (pass_end) — no copy launch behind the kernel, no
    // hipStreamSynchronize (~15 us per structure).  That needs the whole block zero at the start (its tickets live there) and
    // leaves it zero.  With further device words to read (`also`) or a caller-owned stream: a copy and a stream wait.
    const bool polled = !also && !c->external_stream;
    const bool counters_were_zero = c->ctr_zero_ok;      // (the error word is the only counter touched here, and it ends as zero when all is well)
    if (polled) {
        if (!c->ctr_zero_ok) HIPCHK(c, hipMemsetAsync(c->d_ctr, 0, sizeof(u64) * C_DEV_WORDS, c->stream));
    } else {
        HIPCHK(c, hipMemsetAsync(d_err, 0, sizeof(u64), c->stream));
    }
    c->ctr_zero_ok = false;
    if (gather_sb) HIPCHK(c, c->sb.reserve((size_t)std::max<int64_t>(h.n, 1)));
    BlobCheck bc;
    bc.n = (int)h.n; bc.nres = (int)h.nres; bc.nbond = (int)h.nbond; bc.nh = (int)h.nh; bc.nring = (int)h.nring; bc.namide = (int)h.namide;
    bc.nrad = (int)h.n_rad;
    for (int k = 0; k < 3; ++k) {   // float32 coordinates against the double box: widen by one float ulp either way
        bc.lo[k] = std::nextafter((float)h.lo[k], -INFINITY);
        bc.hi[k] = std::nextafter((float)h.hi[k], INFINITY);
    }
    bc.xyz = c->xyz.p; bc.rad = c->rad.p; bc.rad_idx = c->rad_idx.p; bc.res_id = c->res_id.p; bc.res_prev = c->res_prev.p;
    bc.res_next = c->res_next.p; bc.bond_off = c->bond_off.p; bc.bond_idx = c->bond_idx.p; bc.h_off = c->h_off.p;
    bc.h_xyz = c->h_xyz_d.p; bc.sb_nbr = c->blob_sb_nbr.p; bc.ring_c = c->ring_c.p; bc.ring_res = c->ring_res.p;
    bc.am_c = c->am_c.p; bc.am_res = c->am_res.p; bc.err = d_err;
    bc.sb_out = gather_sb ? c->sb.p : nullptr;
    bc.rad_out = rad_from_table ? (double2*)c->rad.p : nullptr;
    bc.rad_tab = (const double2*)c->rad_tab.p;
    // The two fills the first pass over a new structure would otherwise begin with ride in this launch (each is ~4 us of
    // launch on the host and a gap on the device): the default selection and the cleared histogram of the static order.
    const size_t sel_words = ((size_t)std::max<int64_t>(h.n, 1) + 3) / 4;
    HIPCHK(c, c->sel.reserve(sel_words * 4));
    bc.fill_ones = (uint32_t*)c->sel.p; bc.fill_ones_n = (int)sel_words;
    const size_t zero_ints = std::min<size_t>(c->sp_cnt.cap & ~(size_t)3, (size_t)1 << 30);
    bc.fill_zero = (int4*)c->sp_cnt.p; bc.fill_zero_n = (int)(zero_ints / 4);
    const int64_t work = std::max({h.n, h.nbond, 3 * h.nh, h.nring, h.namide, h.nres, (int64_t)1});
    PublishArgs pub{c->d_ctr, c->h_ctr_pinned, 0, 0};
    if (polled) { pub.expected = 1; pub.seq = ++c->publish_seq; }
    // (what the second stream waits for below is the structure's copy, not its validation: the event goes in front of the kernel)
    // (not when the context's last structure was a batch: the next call is arp_set_batch again, which throws away whatever was made
    // for the concatenation as ONE structure — whose overlaid coordinates make for enormous candidate lists on top: a batch of 64
    // stand-ins took 3.2 instead of 1.4 ms end to end)
    const bool with_upload = sw().grids_with_upload && polled && h.n > 0 && h.nring + h.namide > 0 && !after_batch;
    const bool on_second = with_upload && sw().upload_aside && c->stream2 && c->ev_upload && c->ev_uplists;
    // single-bond neighbour coordinates, ring / amide masks, bookkeeping: as the classic setters leave them (before the launches
    // below, which read some of it: ownership flags, the batch, the static state)
    const size_t n1 = (size_t)std::max<int64_t>(h.n, 1);
    HIPCHK(c, c->sb.reserve(n1));
    HIPCHK(c, c->ring_sel.reserve((size_t)std::max<int64_t>(h.nring, 1))); HIPCHK(c, c->ring_plus.reserve((size_t)std::max<int64_t>(h.nring, 1)));
    HIPCHK(c, c->am_sel.reserve((size_t)std::max<int64_t>(h.namide, 1))); HIPCHK(c, c->am_plus.reserve((size_t)std::max<int64_t>(h.namide, 1)));
    inputs_changed(c, IN_EVERYTHING);
    c->has_gid = c->has_home = c->has_group_owner = false;
    c->gid_max = -1;
    c->shard_resident = false;
    c->sel_prefilled = true; c->sp_cnt_zeroed = zero_ints;      // (k_validate_blob's fills)
    // a failed check also leaves the number of this upload in a word of its own (the error word goes back to zero when the verdict
    // is published): kernels enqueued ahead of the verdict look at it and leave (speculative static order, below)
    HIPCHK(c, c->upload_bad.reserve(1));
    if (!c->upload_bad_cleared) { HIPCHK(c, hipMemsetAsync(c->upload_bad.p, 0, sizeof(int), c->stream)); c->upload_bad_cleared = true; }
    bc.bad_seq = polled ? c->upload_bad.p : nullptr;
    bc.seq = (int)(pub.seq & 0x7FFFFFFF);
    if (on_second) HIPCHK(c, hipEventRecord(c->ev_upload, c->stream));
    hipLaunchKernelGGL(k_validate_blob, dim3(nblocks(work, 256, 2048)), dim3(256), 0, c->stream, bc, pub);
    CHK(check_launch(c, "k_validate_blob"));
    // The 6 A grids of the ring and amide centres and the candidate lists of the ring / amide loops depend on what was uploaded
    // only (centres, their boxes, the atoms as they came): they are built beside the validation kernel, on the SECOND stream, as
    // soon as the copy has landed, while the host waits for the verdict and turns round, and the first pass joins them in front of
    // its grid build (ARP_UPLOAD_ASIDE=0: behind the validation kernel on the main stream, where the static order of the first pass
    // then waits for them: 25 us of latency chains at 100 k atoms).  A structure that fails the validation has them thrown away
    // below: centres outside their box are clamped into it, nothing is written out of bounds.
    // A failure behind the validation kernel (an allocation, a launch) or a failed verdict: the verdict may still be on its way
    // and kernels of the second stream may be reading the blob — wait for both streams, consume what was published, leave no
    // structure resident.
    auto abandon = [&](int rc) -> int {
        const std::string why = c->err;
        if (c->stream2) (void)hipStreamSynchronize(c->stream2);
        if (polled) (void)collect_counters(c); else (void)hipStreamSynchronize(c->stream);
        c->err = why;
        drop_resident(c);
        return rc;
    };
    if (with_upload) {
        if (on_second) {
            if (hipStreamWaitEvent(c->stream2, c->ev_upload, 0) != hipSuccess) { c->err = "hipStreamWaitEvent failed (upload lists)"; return abandon(ARP_E_HIP); }
            std::swap(c->stream, c->stream2);
        }
        int rc = ensure_center_grids(c);
        if (rc == ARP_OK && sw().lists_with_upload) rc = ensure_plane_lists(c);      // (the four candidate lists need nothing else: see ar_enumerate)
        if (on_second) {
            std::swap(c->stream, c->stream2);
            if (rc == ARP_OK) {
                if (hipEventRecord(c->ev_uplists, c->stream2) != hipSuccess) { c->err = "hipEventRecord failed (upload lists)"; rc = ARP_E_HIP; }
                else c->uplists_pending = true;
            }
        }
        if (rc != ARP_OK) return abandon(rc);
    }
    // The static columns of the structure and their spatial order — the first three launches of its first pass — go out NOW, for the
    // cell edge of the context's last pass: they run while the host waits for the verdict and turns round (13 us between the end of
    // the validation kernel and the first launch of the pass, at 100 k atoms), and leave at once when the check has failed
    // (upload_bad: the arrays they would index are what the check is about).  A pass with another cell edge re-orders the columns
    // as it does for any resident structure.
    if (sw().static_with_upload && polled && h.n > 0 && c->last_cutoff > 0 && !after_batch) {
        c->ahead_seq = bc.seq;
        const int rc = ensure_static(c, c->last_cutoff);
        c->ahead_seq = 0;
        if (rc != ARP_OK) return abandon(rc);
    }
    int h_err[2] = {0, 0};
    if (polled) {
        const int rc = collect_counters(c);
        if (rc != ARP_OK) return abandon(rc);
        h_err[0] = (int)(uint32_t)c->h_ctr[C_ERR];
    } else {
        HIPCHK(c, hipMemcpyAsync(&h_err[0], d_err, sizeof(int), hipMemcpyDeviceToHost, c->stream));
        if (also) HIPCHK(c, hipMemcpyAsync(&h_err[1], also, sizeof(int), hipMemcpyDeviceToHost, c->stream));
        HIPCHK(c, hipStreamSynchronize(c->stream));
    }
    if (h_err[0] != 0 || h_err[1] != 0) {      // (whatever was made ahead of the verdict is void)
        c->err = std::string(who) + ": the structure failed validation (non-finite value, point outside its box, index out of range, "
                                    "offsets that are not a CSR, or an item that occurs twice)";
        return abandon(ARP_E_ARG);
    }
    c->ctr_zero_ok = polled ? true : counters_were_zero;      // (polled: the publishing block returned every counter to zero)
    return ARP_OK;
}
}  // namespace

int arp_set_blob(arp_ctx* c, const void* blob, uint64_t bytes) {
    if (!c || !blob || bytes < sizeof(arp_blob_header)) return ARP_E_ARG;
    CHK(join_upload_lists(c));
    arp_blob_header h;
    memcpy(&h, blob, sizeof(h));
    CHK(check_blob_header(c, h, bytes));
    HIPCHK(c, hipSetDevice(c->device));
    HIPCHK(c, c->blob_dev.reserve((size_t)h.bytes));
    // The per-atom radii (16 of a structure's ~87 bytes per atom) are redundant when every atom's {vdw, cov} pair is in the
    // blob's table — always, for real structures: a handful of elements —: they stay on the host and the validation kernel
    // writes them on the device from the table.  (From 32 768 atoms on: below that the second copy costs more than the bytes.)
    bool rad_from_table = h.n >= 32768 && h.n_rad > 0 && h.n_rad <= RAD_TABLE;
    if (rad_from_table) {
        const uint16_t* ridx = blob_at<uint16_t>((const uint8_t*)blob, h, BLOB_RAD_IDX);
        unsigned any_none = 0;
        for (int64_t i = 0; i < h.n; ++i) any_none |= (unsigned)(ridx[i] == RAD_NONE);
        rad_from_table = any_none == 0;
    }
    if (rad_from_table) {
        const uint64_t rad = h.off[BLOB_RAD], after = h.off[BLOB_RAD + 1];       // everything before the radii, everything behind them
        HIPCHK(c, hipMemcpyAsync(c->blob_dev.p, blob, (size_t)rad, hipMemcpyHostToDevice, c->stream));
        HIPCHK(c, hipMemcpyAsync(c->blob_dev.p + after, (const uint8_t*)blob + after, (size_t)(h.bytes - after), hipMemcpyHostToDevice, c->stream));
    } else {
        HIPCHK(c, hipMemcpyAsync(c->blob_dev.p, blob, (size_t)h.bytes, hipMemcpyHostToDevice, c->stream));
    }
    borrow_blob_views(c, h);
    return validate_resident_blob(c, h, "arp_set_blob", nullptr, /*gather_sb=*/true, rad_from_table);   // (one launch: checks + single-bond neighbour coordinates)
}

int arp_get_blob(arp_ctx* c, void* host, uint64_t cap, uint64_t* bytes) {
    if (!c || !bytes) return ARP_E_ARG;
    if (c->blob_bytes == 0 || !c->blob_dev.p) FAIL(c, ARP_E_ARG, "arp_get_blob: the resident structure did not come from a blob");
    *bytes = c->blob_bytes;
    if (!host) return ARP_OK;
    if (cap < c->blob_bytes) FAIL(c, ARP_E_CAPACITY, "arp_get_blob: buffer too small");
    HIPCHK(c, hipSetDevice(c->device));
    HIPCHK(c, hipMemcpyAsync(host, c->blob_dev.p, (size_t)c->blob_bytes, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    return ARP_OK;
}

// ---- sharded structures assembled on the device ---------------------------------------------------------
namespace {
int check_rec_header(arp_ctx* c, const arp_rec_header& h, uint64_t bytes, const char* who) {
    const std::string w(who);
    if (h.magic != ARP_REC_MAGIC) FAIL(c, ARP_E_ARG, w + ": bad magic");
    arp_rec_header want;
    if (!rec_header(h.na, h.nh, h.nb, h.nring, h.namide, want)) FAIL(c, ARP_E_ARG, w + ": counts out of range");
    if (h.bytes != want.bytes || h.bytes > bytes) FAIL(c, ARP_E_ARG, w + ": size does not match the counts");
    if (memcmp(h.off, want.off, sizeof(h.off)) != 0) FAIL(c, ARP_E_ARG, w + ": unexpected section offset");
    if (h.n_rad < 0 || h.n_rad > RAD_TABLE) FAIL(c, ARP_E_ARG, w + ": n_rad out of range");
    return ARP_OK;
}
RecList rec_list(const uint8_t* base, const arp_rec_header& h) {
    RecList l;
    l.a = (const arp_rec_atom*)(base + h.off[REC_ATOMS]); l.h = (const double*)(base + h.off[REC_H_XYZ]); l.b = (const int*)(base + h.off[REC_BONDS]);
    l.r = (const arp_rec_ring*)(base + h.off[REC_RINGS]); l.m = (const arp_rec_amide*)(base + h.off[REC_AMIDES]);
    l.na = (int)h.na; l.nh = (int)h.nh; l.nb = (int)h.nb; l.nr = (int)h.nring; l.nm = (int)h.namide;
    return l;
}
RecList empty_rec_list() {
    RecList l;
    l.a = nullptr; l.h = nullptr; l.b = nullptr; l.r = nullptr; l.m = nullptr;
    l.na = l.nh = l.nb = l.nr = l.nm = 0;
    return l;
}
}  // namespace

int arp_shard_set_home(arp_ctx* c, const void* records, uint64_t bytes) {
    if (!c || !records || bytes < sizeof(arp_rec_header)) return ARP_E_ARG;
    arp_rec_header h;
    memcpy(&h, records, sizeof(h));
    CHK(check_rec_header(c, h, bytes, "arp_shard_set_home"));
    {   // the CSR runs of the home records are read by the face kernels: check them here (the merge checks received buffers)
        const arp_rec_atom* a = (const arp_rec_atom*)((const uint8_t*)records + h.off[REC_ATOMS]);
        for (int64_t i = 0; i < h.na; ++i) {
            const bool ok = a[i].h_cnt >= 0 && a[i].bond_cnt >= 0 && a[i].h_start >= 0 && a[i].bond_start >= 0 &&
                            (int64_t)a[i].h_start + a[i].h_cnt <= h.nh && (int64_t)a[i].bond_start + a[i].bond_cnt <= h.nb &&
                            (i == 0 || a[i - 1].gid < a[i].gid);
            if (!ok) FAIL(c, ARP_E_ARG, "arp_shard_set_home: atom records must ascend by gid and their runs must lie inside the sections");
        }
    }
    HIPCHK(c, hipSetDevice(c->device));
    HIPCHK(c, c->rec_home.reserve((size_t)h.bytes));
    HIPCHK(c, hipMemcpyAsync(c->rec_home.p, records, (size_t)h.bytes, hipMemcpyHostToDevice, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    c->rec_home_hdr = h;
    c->has_rec_home = true;
    return ARP_OK;
}

int arp_shard_pack_face(arp_ctx* c, int slot, double x_lo, double x_hi, uint64_t* device_ptr, uint64_t* out_bytes) {
    if (!c || slot < 0 || slot > 1 || !device_ptr || !out_bytes || std::isnan(x_lo) || std::isnan(x_hi)) return ARP_E_ARG;
    if (!c->has_rec_home) FAIL(c, ARP_E_ARG, "arp_shard_pack_face: call arp_shard_set_home first");
    HIPCHK(c, hipSetDevice(c->device));
    const arp_rec_header& H = c->rec_home_hdr;
    const RecList home = rec_list(c->rec_home.p, H);
    // five flag / count arrays, each one longer than its set (the scans leave the totals there)
    const size_t na = (size_t)H.na, nr = (size_t)H.nring, nm = (size_t)H.namide;
    HIPCHK(c, c->sh_scan.reserve(3 * (na + 1) + (nr + 1) + (nm + 1)));
    int* fa = c->sh_scan.p; int* fh = fa + na + 1; int* fb = fh + na + 1; int* fr = fb + na + 1; int* fm = fr + nr + 1;
    hipLaunchKernelGGL(k_face_flags, dim3(nblocks((int64_t)std::max({na, nr, nm, (size_t)1}), 256)), dim3(256), 0, c->stream, home, x_lo, x_hi,
                       fa, fh, fb, fr, fm);
    ScanSegs S;
    S.p[0] = fa; S.p[1] = fh; S.p[2] = fb; S.p[3] = fr; S.p[4] = fm;
    S.n[0] = S.n[1] = S.n[2] = (int)na; S.n[3] = (int)nr; S.n[4] = (int)nm;
    hipLaunchKernelGGL(k_scan_segments, dim3(5), dim3(1024), 0, c->stream, S);
    CHK(check_launch(c, "k_face_flags / k_scan_segments"));
    int tot[5];
    const int* last[5] = {fa + na, fh + na, fb + na, fr + nr, fm + nm};
    for (int k = 0; k < 5; ++k) HIPCHK(c, hipMemcpyAsync(&tot[k], last[k], sizeof(int), hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    arp_rec_header F;
    if (!rec_header(tot[0], tot[1], tot[2], tot[3], tot[4], F)) FAIL(c, ARP_E_ARG, "arp_shard_pack_face: counts out of range");
    const uint64_t bytes = F.bytes;
    // any box that contains the points will do: the home boxes, clipped to the x range that was asked for
    for (int k = 0; k < 3; ++k) {
        F.lo[k] = H.lo[k]; F.hi[k] = H.hi[k]; F.ring_lo[k] = H.ring_lo[k]; F.ring_hi[k] = H.ring_hi[k];
        F.amide_lo[k] = H.amide_lo[k]; F.amide_hi[k] = H.amide_hi[k];
    }
    auto clip = [&](double& lo, double& hi) {
        const double l = std::max(lo, x_lo), u = std::min(hi, x_hi);
        if (l <= u) { lo = l; hi = u; }    // (an empty face keeps the home box; its points are none)
    };
    clip(F.lo[0], F.hi[0]); clip(F.ring_lo[0], F.ring_hi[0]); clip(F.amide_lo[0], F.amide_hi[0]);
    F.n_rad = H.n_rad;
    memcpy(F.rad_tab, H.rad_tab, sizeof(F.rad_tab));
    DevBuf<uint8_t>& out = c->rec_face[slot];
    HIPCHK(c, out.reserve((size_t)bytes));
    HIPCHK(c, hipMemsetAsync(out.p, 0, (size_t)bytes, c->stream));         // alignment gaps travel too: keep them defined
    HIPCHK(c, hipMemcpyAsync(out.p, &F, sizeof(F), hipMemcpyHostToDevice, c->stream));
    hipLaunchKernelGGL(k_face_write, dim3(nblocks((int64_t)std::max({na, nr, nm, (size_t)1}), 256)), dim3(256), 0, c->stream, home, fa, fh, fb, fr,
                       fm, (arp_rec_atom*)(out.p + F.off[REC_ATOMS]), (double*)(out.p + F.off[REC_H_XYZ]), (int*)(out.p + F.off[REC_BONDS]),
                       (arp_rec_ring*)(out.p + F.off[REC_RINGS]), (arp_rec_amide*)(out.p + F.off[REC_AMIDES]));
    CHK(check_launch(c, "k_face_write"));
    HIPCHK(c, hipStreamSynchronize(c->stream));     // the caller hands the buffer to another stream (RCCL)
    *device_ptr = (uint64_t)(uintptr_t)out.p;
    *out_bytes = bytes;
    return ARP_OK;
}

int arp_shard_assemble(arp_ctx* c, uint64_t dev_left, uint64_t bytes_left, uint64_t dev_right, uint64_t bytes_right, int64_t nres_global,
                       int64_t counts[3]) {
    if (!c || nres_global < 0) return ARP_E_ARG;
    CHK(join_upload_lists(c));
    if (!c->has_rec_home) FAIL(c, ARP_E_ARG, "arp_shard_assemble: call arp_shard_set_home first");
    HIPCHK(c, hipSetDevice(c->device));
    inputs_changed(c, IN_EVERYTHING);      // (the blob of the resident structure is overwritten below)
    arp_rec_header hd[3];
    hd[0] = c->rec_home_hdr;
    const uint8_t* base[3] = {c->rec_home.p, (const uint8_t*)(uintptr_t)dev_left, (const uint8_t*)(uintptr_t)dev_right};
    const uint64_t given[3] = {hd[0].bytes, bytes_left, bytes_right};
    RecLists L;
    L.l[0] = rec_list(base[0], hd[0]);
    for (int s = 1; s < 3; ++s) {
        if (!base[s]) { L.l[s] = empty_rec_list(); memset(&hd[s], 0, sizeof(hd[s])); continue; }
        if (given[s] < sizeof(arp_rec_header)) FAIL(c, ARP_E_ARG, "arp_shard_assemble: halo buffer shorter than its header");
        HIPCHK(c, hipMemcpyAsync(&hd[s], base[s], sizeof(arp_rec_header), hipMemcpyDeviceToHost, c->stream));
    }
    HIPCHK(c, hipStreamSynchronize(c->stream));
    for (int s = 1; s < 3; ++s)
        if (base[s]) {
            CHK(check_rec_header(c, hd[s], given[s], "arp_shard_assemble"));
            L.l[s] = rec_list(base[s], hd[s]);
        }
    const int64_t n = hd[0].na + hd[1].na + hd[2].na, nh = hd[0].nh + hd[1].nh + hd[2].nh;
    const int64_t nring = hd[0].nring + hd[1].nring + hd[2].nring, namide = hd[0].namide + hd[1].namide + hd[2].namide;
    if (!rec_counts_ok(n, nh, 0, nring, namide)) FAIL(c, ARP_E_ARG, "arp_shard_assemble: merged counts out of range");
    if (n > 0 && nres_global <= 0) FAIL(c, ARP_E_ARG, "arp_shard_assemble: atoms without a residue table");
    // positions, hydrogen and local-bond counts, their scans
    HIPCHK(c, c->sh_scan.reserve(2 * ((size_t)n + 1) + 4));
    HIPCHK(c, c->sh_src.reserve((size_t)std::max<int64_t>(n, 1)));
    int* hoff = c->sh_scan.p; int* boff = hoff + n + 1; int* d_err = boff + n + 1;
    HIPCHK(c, hipMemsetAsync(d_err, 0, sizeof(int), c->stream));
    if (n > 0) {
        hipLaunchKernelGGL(k_merge_positions, dim3(nblocks(n, 256)), dim3(256), 0, c->stream, L, c->sh_src.p, hoff, boff, d_err);
        CHK(check_launch(c, "k_merge_positions"));
    }
    ScanSegs S;
    memset(&S, 0, sizeof(S));
    S.p[0] = hoff; S.p[1] = boff; S.n[0] = S.n[1] = (int)n;
    hipLaunchKernelGGL(k_scan_segments, dim3(2), dim3(1024), 0, c->stream, S);
    CHK(check_launch(c, "k_scan_segments"));
    int tot[3] = {0, 0, 0};
    HIPCHK(c, hipMemcpyAsync(&tot[0], hoff + n, sizeof(int), hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipMemcpyAsync(&tot[1], boff + n, sizeof(int), hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipMemcpyAsync(&tot[2], d_err, sizeof(int), hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    if (tot[2] != 0 || tot[0] != nh)
        FAIL(c, ARP_E_ARG, "arp_shard_assemble: an atom occurs twice in home + halos, a list is not ascending, or a record's runs leave its sections");
    const int64_t nbond = tot[1];
    // the blob the merged structure lives in
    arp_blob_header B;
    if (!blob_header(n, nres_global, nbond, nh, nring, namide, B)) FAIL(c, ARP_E_ARG, "arp_shard_assemble: merged counts out of range");
    const uint64_t bytes = B.bytes;
    {   // boxes: the union over the parts that hold points of the kind (none: 0, as the header is)
        bool any[3] = {false, false, false};
        for (int s = 0; s < 3; ++s) {
            if (hd[s].na > 0) box_union(B.lo, B.hi, any[0], hd[s].lo, hd[s].hi);
            if (hd[s].nring > 0) box_union(B.ring_lo, B.ring_hi, any[1], hd[s].ring_lo, hd[s].ring_hi);
            if (hd[s].namide > 0) box_union(B.amide_lo, B.amide_hi, any[2], hd[s].amide_lo, hd[s].amide_hi);
        }
    }
    B.n_rad = hd[0].n_rad;
    CHK(check_blob_header(c, B, bytes));
    HIPCHK(c, c->blob_dev.reserve((size_t)bytes));
    HIPCHK(c, hipMemsetAsync(c->blob_dev.p, 0, (size_t)bytes, c->stream));
    HIPCHK(c, hipMemcpyAsync(c->blob_dev.p, &B, sizeof(B), hipMemcpyHostToDevice, c->stream));
    HIPCHK(c, hipMemcpyAsync(c->blob_dev.p + B.off[BLOB_RAD_TAB], hd[0].rad_tab, sizeof(double) * 2 * RAD_TABLE, hipMemcpyHostToDevice, c->stream));
    borrow_blob_views(c, B);
    const size_t n1 = (size_t)std::max<int64_t>(n, 1), r1 = (size_t)std::max<int64_t>(nring, 1), m1 = (size_t)std::max<int64_t>(namide, 1);
    HIPCHK(c, c->sb.reserve(n1)); HIPCHK(c, c->gid.reserve(n1)); HIPCHK(c, c->home.reserve(n1)); HIPCHK(c, c->origin.reserve(n1));
    HIPCHK(c, c->sh_sel.reserve(n1));
    HIPCHK(c, c->ring_gid.reserve(r1)); HIPCHK(c, c->ring_home.reserve(r1)); HIPCHK(c, c->ring_origin.reserve(r1));
    HIPCHK(c, c->am_gid.reserve(m1)); HIPCHK(c, c->am_home.reserve(m1)); HIPCHK(c, c->am_origin.reserve(m1));
    if (nres_global > 0) {
        hipLaunchKernelGGL(k_init_residues, dim3(nblocks(nres_global, 256)), dim3(256), 0, c->stream, (int)nres_global, c->res_flags.p,
                           c->res_prev.p, c->res_next.p);
        CHK(check_launch(c, "k_init_residues"));
    }
    MergeOut O;
    O.n = (int)n; O.nres = (int)nres_global; O.n_rad = (int)B.n_rad;
    O.xyz = c->xyz.p; O.rad = c->rad.p; O.tmask = c->tmask.p; O.flags = c->flags.p; O.res_id = c->res_id.p;
    O.res_flags = c->res_flags.p; O.res_prev = c->res_prev.p; O.res_next = c->res_next.p;
    O.bond_off = c->bond_off.p; O.bond_idx = c->bond_idx.p; O.h_off = c->h_off.p; O.h_xyz = c->h_xyz_d.p; O.sb_nbr = c->blob_sb_nbr.p;
    O.rad_idx = c->rad_idx.p; O.rad_tab = c->rad_tab.p;
    O.sb = c->sb.p; O.gid = c->gid.p; O.home = c->home.p; O.origin = c->origin.p; O.sel = c->sh_sel.p;
    hipLaunchKernelGGL(k_merge_fill, dim3(nblocks(std::max<int64_t>(n, 1), 256)), dim3(256), 0, c->stream, L, O, c->sh_src.p, hoff, boff, d_err);
    CHK(check_launch(c, "k_merge_fill"));
    GroupOut G;
    G.ring_c = c->ring_c.p; G.ring_n = c->ring_n.p; G.ring_res = c->ring_res.p; G.ring_gid = c->ring_gid.p; G.ring_home = c->ring_home.p;
    G.ring_origin = c->ring_origin.p;
    G.am_c = c->am_c.p; G.am_n = c->am_n.p; G.am_res = c->am_res.p; G.am_gid = c->am_gid.p; G.am_home = c->am_home.p; G.am_origin = c->am_origin.p;
    if (nring + namide > 0) {
        hipLaunchKernelGGL(k_merge_groups, dim3(nblocks(std::max(nring, namide), 256)), dim3(256), 0, c->stream, L, G, d_err);
        CHK(check_launch(c, "k_merge_groups"));
    }
    CHK(validate_resident_blob(c, B, "arp_shard_assemble", d_err));     // waits; resets selection and ownership state
    c->has_gid = c->has_home = true;
    c->gid_max = -1;      // (the merged ids live on the device only: the sort takes the 31-bit key width)
    c->has_group_owner = true;
    c->shard_resident = true;
    if (counts) { counts[0] = n; counts[1] = nring; counts[2] = namide; }
    return ARP_OK;
}

int arp_shard_layout(arp_ctx* c, int32_t* global_id, int8_t* origin, uint8_t* sel, int32_t* ring_gid, int8_t* ring_origin,
                     int32_t* amide_gid, int8_t* amide_origin) {
    if (!c) return ARP_E_ARG;
    if (!c->shard_resident) FAIL(c, ARP_E_ARG, "arp_shard_layout: no structure assembled by arp_shard_assemble is resident");
    HIPCHK(c, hipSetDevice(c->device));
    CHK(download_async(c, global_id, c->gid.p, (size_t)c->n));
    CHK(download_async(c, origin, c->origin.p, (size_t)c->n));
    CHK(download_async(c, sel, c->sh_sel.p, (size_t)c->n));
    CHK(download_async(c, ring_gid, c->ring_gid.p, (size_t)c->nring));
    CHK(download_async(c, ring_origin, c->ring_origin.p, (size_t)c->nring));
    CHK(download_async(c, amide_gid, c->am_gid.p, (size_t)c->namide));
    CHK(download_async(c, amide_origin, c->am_origin.p, (size_t)c->namide));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    return ARP_OK;
}

int arp_set_ownership(arp_ctx* c, const uint8_t* is_home, const int32_t* global_id) {
    if (!c) return ARP_E_ARG;
    HIPCHK(c, hipSetDevice(c->device));
    inputs_changed(c, IN_OWNERSHIP);      // (M_HOME is part of the sorted records)
    if (is_home) { CHK(upload(c, c->home, is_home, (size_t)c->n)); c->has_home = true; }
    else c->has_home = false;
    if (global_id) {
        if (c->n > 0 && global_id[0] < 0) FAIL(c, ARP_E_ARG, "arp_set_ownership: global_id must not be negative");
        for (int64_t i = 1; i < c->n; ++i)
            if (global_id[i] <= global_id[i - 1]) FAIL(c, ARP_E_ARG, "arp_set_ownership: global_id must be strictly increasing");
        CHK(upload(c, c->gid, global_id, (size_t)c->n));
        c->has_gid = true;
        c->gid_max = c->n > 0 ? (int64_t)global_id[c->n - 1] : -1;
    } else { c->has_gid = false; c->gid_max = -1; }
    return ARP_OK;
}

int arp_set_group_ownership(arp_ctx* c, const uint8_t* ring_home, const int32_t* ring_gid, const uint8_t* amide_home,
                            const int32_t* amide_gid) {
    if (!c) return ARP_E_ARG;
    HIPCHK(c, hipSetDevice(c->device));
    inputs_changed(c, IN_GROUP_OWNERSHIP);
    if (!ring_home && !ring_gid && !amide_home && !amide_gid) { c->has_group_owner = false; return ARP_OK; }
    if ((c->nring > 0 && (!ring_home || !ring_gid)) || (c->namide > 0 && (!amide_home || !amide_gid)))
        FAIL(c, ARP_E_ARG, "arp_set_group_ownership: all four arrays are required");
    for (int64_t i = 1; i < c->nring; ++i)
        if (ring_gid[i] <= ring_gid[i - 1]) FAIL(c, ARP_E_ARG, "arp_set_group_ownership: ring_gid must be strictly increasing");
    for (int64_t i = 1; i < c->namide; ++i)
        if (amide_gid[i] <= amide_gid[i - 1]) FAIL(c, ARP_E_ARG, "arp_set_group_ownership: amide_gid must be strictly increasing");
    CHK(upload(c, c->ring_home, ring_home, (size_t)c->nring)); CHK(upload(c, c->ring_gid, ring_gid, (size_t)c->nring));
    CHK(upload(c, c->am_home, amide_home, (size_t)c->namide)); CHK(upload(c, c->am_gid, amide_gid, (size_t)c->namide));
    c->has_group_owner = true;
    return ARP_OK;
}

int arp_set_single_bond_neighbour_coords(arp_ctx* c, const float* sb_xyz, const uint8_t* sb_present) {
    if (!c || (c->n > 0 && (!sb_xyz || !sb_present))) return ARP_E_ARG;
    HIPCHK(c, hipSetDevice(c->device));
    inputs_changed(c, IN_NEIGHBOURS);
    c->sb_index_src = 0;
    std::vector<float4> sb((size_t)c->n);
    for (int64_t i = 0; i < c->n; ++i)
        sb[i] = sb_present[i] ? make_float4(sb_xyz[3 * i], sb_xyz[3 * i + 1], sb_xyz[3 * i + 2], 1.0f) : make_float4(0, 0, 0, 0);
    CHK(upload(c, c->sb, sb.data(), (size_t)c->n));
    return ARP_OK;
}

int arp_set_selection_state(arp_ctx* c, const uint8_t* in_selection, const uint8_t* in_plus, const uint8_t* ring_sel,
                            const uint8_t* ring_plus, const uint8_t* amide_sel, const uint8_t* amide_plus) {
    if (!c) return ARP_E_ARG;
    if ((c->n > 0 && (!in_selection || !in_plus)) || (c->nring > 0 && (!ring_sel || !ring_plus)) ||
        (c->namide > 0 && (!amide_sel || !amide_plus)))
        FAIL(c, ARP_E_ARG, "arp_set_selection_state: null input");
    HIPCHK(c, hipSetDevice(c->device));
    inputs_changed(c, IN_SELECTION_STATE);
    CHK(upload(c, c->sel, in_selection, (size_t)c->n));
    CHK(upload(c, c->plus, in_plus, (size_t)c->n));
    c->sel_uploaded = true;
    c->nsel = -1;
    c->sel_all = false;   // the caller's masks are taken as they are
    CHK(upload(c, c->ring_sel, ring_sel, (size_t)c->nring)); CHK(upload(c, c->ring_plus, ring_plus, (size_t)c->nring));
    CHK(upload(c, c->am_sel, amide_sel, (size_t)c->namide)); CHK(upload(c, c->am_plus, amide_plus, (size_t)c->namide));
    c->sel_made = true;
    return ARP_OK;
}

int arp_set_selection(arp_ctx* c, const uint8_t* in_selection) {
    if (!c || (c->n > 0 && !in_selection)) return ARP_E_ARG;
    HIPCHK(c, hipSetDevice(c->device));
    inputs_changed(c, IN_SELECTION);      // (expansion pending)
    CHK(upload(c, c->sel, in_selection, (size_t)c->n));
    c->sel_uploaded = true;
    // how many atoms are selected decides how selection_plus is computed (arp_run_launch): everything -> nothing to do,
    // a handful -> direct test of every atom against the list (k_expand_small), otherwise the 6 A grid search
    int64_t nsel = 0;
    std::vector<int> list;
    for (int64_t i = 0; i < c->n; ++i)
        if (in_selection[i]) {
            if (nsel < SMALL_SEL_MAX) list.push_back((int)i);
            ++nsel;
        }
    c->nsel = nsel;
    c->sel_all = (nsel == c->n);
    if (nsel > 0 && nsel <= SMALL_SEL_MAX) CHK(upload(c, c->sel_list, list.data(), (size_t)nsel));
    return ARP_OK;
}

// ---- NeighborSearch.search_all -----------------------------------------------------------
int arp_search_all(arp_ctx* c, double radius, const uint8_t* active, int64_t cap, int32_t* out_i, int32_t* out_j, int64_t* count) {
    if (!c || !count || cap < 0 || !(radius > 0)) return ARP_E_ARG;
    HIPCHK(c, hipSetDevice(c->device));
    const uint8_t* d_active = nullptr;
    if (active) {
        CHK(upload(c, c->tmp_u8, active, (size_t)c->n));
        d_active = c->tmp_u8.p;
    }
    CHK(build_contact_grid(c, radius, 0, 0, d_active));
    c->atom_grid.valid = false;  // not the contact grid
    c->contacts_valid = false;
    HIPCHK(c, c->pairs.reserve((size_t)std::max<int64_t>(cap, 1)));
    CHK(zero_counter(c, C_SEARCH_PAIRS, 1));
    CHK(zero_counter(c, C_STAT_MCAND, 2 * STAT_SLOTS));
    if (c->n > 0) {
        hipLaunchKernelGGL((k_search<MODE_PAIRS>), dim3(search_blocks(c->atom_grid.d)), dim3(64 * SEARCH_WAVES), 0, c->stream,
                           c->atom_grid.d, c->atom_grid.start.p, c->s_xyzm.p, c->s_aux.p, radius * radius, 1, 0, c->pairs.p,
                           (u64)cap, c->d_ctr + ctr_dev(C_SEARCH_PAIRS), c->d_ctr + ctr_dev(C_STAT_MCAND), c->d_ctr + ctr_dev(C_STAT_MACC), (uint8_t*)nullptr, GroupMasks{}, (const int*)nullptr, (const int*)nullptr);
        CHK(check_launch(c, "k_search<PAIRS>"));
    }
    CHK(read_counters(c));
    collect_events(c);
    *count = (int64_t)c->h_ctr[C_SEARCH_PAIRS];
    if (*count > cap) FAIL(c, ARP_E_CAPACITY, "arp_search_all: output buffer too small");
    if (*count > 0) {
        std::vector<int2> tmp((size_t)*count);
        CHK(download(c, tmp.data(), c->pairs.p, (size_t)*count));
        for (int64_t k = 0; k < *count; ++k) { out_i[k] = tmp[k].x; out_j[k] = tmp[k].y; }
    }
    return ARP_OK;
}

// ---- _make_selection --------------------------------------------------------------------
int arp_make_selection(arp_ctx* c, const uint8_t* in_selection, double expand_radius, uint8_t* out_plus, uint8_t* out_ring_sel,
                       uint8_t* out_ring_plus, uint8_t* out_amide_sel, uint8_t* out_amide_plus) {
    if (!c || !(expand_radius > 0)) return ARP_E_ARG;
    if (in_selection) CHK(arp_set_selection(c, in_selection));
    else {
        HIPCHK(c, hipSetDevice(c->device));
        CHK(default_selection(c));  // nothing uploaded for this structure: whole structure (I:1395)
    }
    CHK(enqueue_selection(c, expand_radius));
    CHK(read_counters(c));
    collect_events(c);
    c->stats[5] = (int64_t)c->h_ctr[C_MARK_CAND];
    c->stats[6] = (int64_t)c->h_ctr[C_MARK_ACC];
    CHK(download(c, out_plus, c->plus.p, out_plus ? (size_t)c->n : 0));
    CHK(download(c, out_ring_sel, c->ring_sel.p, out_ring_sel ? (size_t)c->nring : 0));
    CHK(download(c, out_ring_plus, c->ring_plus.p, out_ring_plus ? (size_t)c->nring : 0));
    CHK(download(c, out_amide_sel, c->am_sel.p, out_amide_sel ? (size_t)c->namide : 0));
    CHK(download(c, out_amide_plus, c->am_plus.p, out_amide_plus ? (size_t)c->namide : 0));
    return ARP_OK;
}

int arp_get_selection(arp_ctx* c, uint8_t* out_plus, uint8_t* out_ring_sel, uint8_t* out_ring_plus, uint8_t* out_amide_sel,
                      uint8_t* out_amide_plus) {
    if (!c) return ARP_E_ARG;
    if (!c->sel_made) FAIL(c, ARP_E_ARG, "arp_get_selection: no selection has been expanded yet");
    HIPCHK(c, hipSetDevice(c->device));
    CHK(download(c, out_plus, c->plus.p, out_plus ? (size_t)c->n : 0));
    CHK(download(c, out_ring_sel, c->ring_sel.p, out_ring_sel ? (size_t)c->nring : 0));
    CHK(download(c, out_ring_plus, c->ring_plus.p, out_ring_plus ? (size_t)c->nring : 0));
    CHK(download(c, out_amide_sel, c->am_sel.p, out_amide_sel ? (size_t)c->namide : 0));
    CHK(download(c, out_amide_plus, c->am_plus.p, out_amide_plus ? (size_t)c->namide : 0));
    return ARP_OK;
}

// ---- _calculate_atom_contacts -------------------------------------------------------------
int arp_atom_contacts_launch(arp_ctx* c, double cutoff, double vdw_comp, int include_sequence_adjacent, int64_t* count) {
    if (!c || !(cutoff > 0)) return ARP_E_ARG;
    HIPCHK(c, hipSetDevice(c->device));
    CHK(ensure_default_selection(c));
    for (int attempt = 0;; ++attempt) {
        CHK(enqueue_contacts(c, cutoff, vdw_comp, include_sequence_adjacent, false));
        CHK(read_counters(c));
        collect_events(c);
        if (!finish_contacts(c)) break;
        if (attempt == 2) FAIL(c, ARP_E_CAPACITY, "arp_atom_contacts_launch: pair buffer could not be sized");
        CHK(grow_pairs(c));
    }
    if (count) *count = c->n_contacts;
    return device_error(c);
}

int arp_atom_contacts_fetch(arp_ctx* c, int64_t cap, int32_t* out_i, int32_t* out_j, float* out_dist, uint16_t* out_sift,
                            uint8_t* out_ctype, int64_t* count) {
    if (!c || !count) return ARP_E_ARG;
    if (!c->contacts_valid) FAIL(c, ARP_E_ARG, "arp_atom_contacts_fetch: no launch results");
    HIPCHK(c, hipSetDevice(c->device));
    *count = c->n_contacts;
    if (c->n_contacts > cap) FAIL(c, ARP_E_CAPACITY, "arp_atom_contacts_fetch: output buffer too small");
    const size_t k = (size_t)c->n_contacts;
    // five copies in flight, one synchronisation (into buffers from arp_host_alloc they run at PCIe speed); the records come
    // in the canonical (i, j) order once arp_atom_contacts_sort has run on them, in the order of the pair list before
    if (c->contacts_sorted && c->sorted_is_csr && out_i) {      // (this call hands out bgn ids: the sorted columns once more, as records)
        const bool was = c->packed_csr;
        c->packed_csr = false;
        const int rc = sort_contacts(c);
        c->packed_csr = was;
        CHK(rc);
    }
    const uint8_t* sl = c->sorted_slab.p;
    const bool srt = c->contacts_sorted;
    if (k) {
        if (out_i) HIPCHK(c, hipMemcpyAsync(out_i, srt ? (const void*)(sl + c->srt_off[0]) : (const void*)c->out_i.p, k * sizeof(int32_t), hipMemcpyDeviceToHost, c->stream));
        if (out_j) HIPCHK(c, hipMemcpyAsync(out_j, srt ? (const void*)(sl + c->srt_off[1]) : (const void*)c->out_j.p, k * sizeof(int32_t), hipMemcpyDeviceToHost, c->stream));
        if (out_dist) HIPCHK(c, hipMemcpyAsync(out_dist, srt ? (const void*)(sl + c->srt_off[2]) : (const void*)c->out_d.p, k * sizeof(float), hipMemcpyDeviceToHost, c->stream));
        if (out_sift) HIPCHK(c, hipMemcpyAsync(out_sift, srt ? (const void*)(sl + c->srt_off[3]) : (const void*)c->out_s.p, k * sizeof(uint16_t), hipMemcpyDeviceToHost, c->stream));
        if (out_ctype) HIPCHK(c, hipMemcpyAsync(out_ctype, srt ? (const void*)(sl + c->srt_off[4]) : (const void*)c->out_ct.p, k * sizeof(uint8_t), hipMemcpyDeviceToHost, c->stream));
    }
    HIPCHK(c, hipStreamSynchronize(c->stream));
    return ARP_OK;
}

int arp_atom_contacts_sort(arp_ctx* c) {
    if (!c) return ARP_E_ARG;
    HIPCHK(c, hipSetDevice(c->device));
    return sort_contacts(c);
}

// Canonical order of a ring / amide bag of MORE than BAG_SORT_MAX records (config 5: 42 k plane-plane records): the radix
// passes of the atom-atom bag (arp_sort.h) on {first id, second id} with the record's index riding as the payload — its bits in
// the float32 column — so that the sorted "distance" column IS the permutation k_pack_segments follows.
__global__ __launch_bounds__(256) void k_iota_bits(long long n, float* __restrict__ out, uint16_t* __restrict__ zs, uint8_t* __restrict__ zc) {
    for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (long long)gridDim.x * blockDim.x) {
        out[i] = __uint_as_float((uint32_t)i);
        zs[i] = 0;
        zc[i] = 0;
    }
}
int bag_order_large(arp_ctx* c, const int* first, const int* second, size_t k, int64_t idmax, DevBuf<uint32_t>& perm) {
    HIPCHK(c, perm.reserve(2 * k));                       // [0, k): the permutation; [k, 2 k): the indices as the sort's input column
    HIPCHK(c, c->bagsort_i.reserve(k)); HIPCHK(c, c->bagsort_j.reserve(k));
    HIPCHK(c, c->bagsort_s.reserve(2 * k)); HIPCHK(c, c->bagsort_ct.reserve(2 * k));
    float* const idx_in = reinterpret_cast<float*>(perm.p + k);
    hipLaunchKernelGGL(k_iota_bits, dim3(nblocks((int64_t)k, 256, 1024)), dim3(256), 0, c->stream, (long long)k, idx_in, c->bagsort_s.p + k, c->bagsort_ct.p + k);
    SortArgs A{};
    A.ci = first; A.cj = second;
    A.d_in = idx_in; A.s_in = c->bagsort_s.p + k; A.ct_in = c->bagsort_ct.p + k;
    A.i_out = c->bagsort_i.p; A.j_out = c->bagsort_j.p; A.d_out = reinterpret_cast<float*>(perm.p);
    A.s_out = c->bagsort_s.p; A.ct_out = c->bagsort_ct.p;
    return radix_sort(c, c->sort_bags, A, k, k, id_bits(idmax), 0, "bag_order_large");
}

// Every result of the last pass with ONE copy: the atom-atom bag in canonical order (sorted on the device if it is not yet)
// and the used prefixes of the four ring / amide bags behind it, gathered in HBM (k_pack_segments) and copied in one piece.
// arp_fetch_packed and arp_fetch_packed_filtered differ in which atom-atom columns lead the piece, in which slab (PackedAtomBag);
// everything behind that is fetch_packed_from.
namespace {
struct PackedAtomBag {
    const char* who;             // the entry point, for messages
    int64_t k;                   // records of the atom-atom bag it delivers
    bool csr;                    // first column: N + 1 row offsets
    FilteredBag* filtered;       // the kept records, sorted in their own slab already; NULL: the whole bag in sorted_slab (sorted on the way)
};
// Where every array of every bag goes in the one piece: the five atom-atom columns (sorted_layout), then the arrays of the
// ring / amide bags (the order of get_contacts, I:183-210), each on a 16-byte boundary
struct PackedPlan {
    size_t off[5], cbytes, total;
    PackTable t;
    int seg_of[BAG_KINDS][BAG_COLS];      // [b][j]: bag b in the order of get_contacts (PACKED_ORDER), column j of its table
};
int packed_plan(arp_ctx* c, const PackedAtomBag& S, PackedPlan& P, int64_t counts[5], uint64_t offsets[ARP_PACKED_OFFSETS]) {
    const std::string who = S.who;
    sorted_layout((size_t)S.k, P.off, &P.cbytes, S.csr ? (size_t)std::max<int64_t>(c->n, 0) + 1 : (size_t)S.k);
    size_t total = P.cbytes;
    PackTable& t = P.t;
    t.n = 0;
    for (int q = 0; q < ARP_PACKED_OFFSETS; ++q) offsets[q] = 0;
    for (int q = 0; q < 5; ++q) offsets[q] = P.off[q];
    counts[0] = S.k;
    for (int b = 0; b < BAG_KINDS; ++b) {
        const int kind = PACKED_ORDER[b];
        const Bag& g = c->bag[kind];
        counts[1 + b] = g.valid ? g.count : 0;
        for (int j = 0; j < BAG_COLS; ++j) P.seg_of[b][j] = -1;
        if (!g.valid || g.count == 0) continue;
        if ((uint64_t)g.count >= ((uint64_t)1 << 31)) FAIL(c, ARP_E_CAPACITY, who + ": a ring / amide bag of 2^31 records or more (fetch the bags one by one)");
        size_t at[BAG_COLS];
        const size_t end = bag_piece_layout(kind, (size_t)g.count, total, at);
        for (int j = 0; j < BAG_COLS; ++j) {
            if (!bag_has(kind, j)) continue;
            const size_t bytes = (size_t)g.count * bag_es(kind, j);
            if (bytes >= ((size_t)1 << 32) || at[j] >= ((size_t)1 << 32)) FAIL(c, ARP_E_CAPACITY, who + ": ring / amide bags too large for one piece (fetch them one by one)");
            offsets[5 + 12 * b + bag_slot(kind, j)] = at[j];
            P.seg_of[b][j] = t.n;
            t.s[t.n++] = PackSeg{g.col[j], (uint32_t)at[j], (uint32_t)bytes, nullptr, (uint32_t)bag_es(kind, j)};
        }
        total = end;
    }
    static_assert(BAG_KINDS * BAG_COLS <= sizeof(PackTable::s) / sizeof(PackSeg), "PackTable");
    P.total = total;
    return ARP_OK;
}
int fetch_packed_from(arp_ctx* c, const PackedAtomBag& S, void* host, uint64_t host_bytes, int64_t counts[5], uint64_t offsets[ARP_PACKED_OFFSETS], uint64_t* bytes_used) {
    const std::string who = S.who;
    // Sizes first: where every array of every bag goes in the one piece, and whether it fits — before anything is launched (a
    // caller with too small a buffer, or a result beyond what one piece can address, leaves with bytes_used and no work done)
    *bytes_used = 0;
    PackedPlan P;
    CHK(packed_plan(c, S, P, counts, offsets));
    PackTable& t = P.t;
    const size_t total = P.total, cbytes = P.cbytes;
    *bytes_used = total;
    if (!host || host_bytes < total) FAIL(c, ARP_E_CAPACITY, who + ": host buffer too small (bytes_used holds the size needed)");
    if (S.filtered && S.filtered->slab.cap < total) FAIL(c, ARP_E_HIP, who + ": the filtered slab has no room for the ring / amide bags");      // (sized by the launch; finish_bag voids it)
    // canonical order of the small bags, made on the device by the two sort keys the table names (plane-plane, group-group,
    // group-plane by (first id, second id), atom-plane by (ring, atom)) — the order the reference's loops create them in
    BagOrderArgs bo{};
    bool any_order = false;
    HIPCHK(c, c->bag_perm.reserve(4 * (size_t)BAG_SORT_MAX));
    for (int b = 0; b < 4; ++b) {
        const Bag& g = c->bag[PACKED_ORDER[b]];
        const bool small = g.valid && g.count > 0 && g.count <= BAG_SORT_MAX;
        bo.first[b] = g.id(PLANE_TABLES[PACKED_ORDER[b]].key[0]);
        bo.second[b] = g.id(PLANE_TABLES[PACKED_ORDER[b]].key[1]);
        bo.n[b] = small ? (int)g.count : 0;
        bo.perm[b] = c->bag_perm.p + (size_t)b * BAG_SORT_MAX;
        any_order = any_order || small;
    }
    const uint32_t* big_perm[4] = {nullptr, nullptr, nullptr, nullptr};
    for (int b = 0; b < 4; ++b) {
        const Bag& g = c->bag[PACKED_ORDER[b]];
        if (!(g.valid && g.count > BAG_SORT_MAX)) continue;
        const int64_t idmax = (c->has_gid || c->has_group_owner) ? (((int64_t)1 << 31) - 1) : std::max<int64_t>({c->n, c->nring, c->namide, 2}) - 1;      // (a shard's records carry global ids)
        CHK(bag_order_large(c, bo.first[b], bo.second[b], (size_t)g.count, idmax, c->bag_perm_big[b]));
        big_perm[b] = c->bag_perm_big[b].p;
    }
    // (on the second stream, beside the radix passes of the atom-atom bag: one block per bag, 80 us for a bag of 4096)
    const bool order_aside = any_order && c->stream2 && !c->external_stream;      // (beside the sort, which may be under way already: arp_set_sort_after_pass)
    for (int b = 0; b < 4; ++b)
        for (int q = 0; q < BAG_COLS; ++q)
            if (P.seg_of[b][q] >= 0) t.s[P.seg_of[b][q]].perm = bo.n[b] > 0 ? bo.perm[b] : big_perm[b];
    if (!S.filtered) c->contacts_sorted = c->contacts_sorted && c->sorted_slab.cap >= total && c->sorted_is_csr == S.csr;
    // (aside: the sort's launches go out first — they are the critical path, the host needs ~5 us per launch —, the one block per
    // small bag on the second stream behind them)
    if (any_order && !order_aside) {
        hipLaunchKernelGGL(k_bag_order, dim3(4), dim3(1024), 0, c->stream, bo);
        CHK(check_launch(c, "k_bag_order"));
    }
    if (!S.filtered) CHK(sort_contacts(c, total - cbytes));
    DevBuf<uint8_t>& slab = S.filtered ? S.filtered->slab : c->sorted_slab;
    if (any_order && order_aside) {
        hipLaunchKernelGGL(k_bag_order, dim3(4), dim3(1024), 0, c->stream2, bo);
        CHK(check_launch(c, "k_bag_order"));
        HIPCHK(c, hipEventRecord(c->ev_planes, c->stream2));
    }
    if (order_aside) HIPCHK(c, hipStreamWaitEvent(c->stream, c->ev_planes, 0));
    if (t.n > 0) {
        hipLaunchKernelGGL(k_pack_segments, pack_grid(t), dim3(256), 0, c->stream, t, slab.p);
        CHK(check_launch(c, "k_pack_segments"));
    }
    if (total) {
        // A small piece (a protein's bags: a few hundred kilobytes) into a page-locked, device-visible buffer is written by a kernel:
        // the copy engine needs ~10 us to get going, which is as long as such a copy takes (stand-in end to end 0.155 -> see
        // profiles/README.md).  Anything larger, or a pageable buffer: the copy engine.
        void* host_dev = nullptr;
        if (total <= sw().fetch_direct_max && host_bytes >= ((total + 15) & ~(uint64_t)15) && slab.cap >= ((total + 15) & ~(size_t)15)) {      // (whole quads on both sides)
            hipPointerAttribute_t at{};
            if (hipPointerGetAttributes(&at, host) == hipSuccess && at.type == hipMemoryTypeHost && at.devicePointer) host_dev = at.devicePointer;
            else (void)hipGetLastError();
        }
        if (host_dev && ((uintptr_t)host_dev & 15) == 0) {
            const unsigned nq = (unsigned)((total + 15) / 16);
            hipLaunchKernelGGL(k_copy_quads, dim3(nblocks(nq, 256, 1024)), dim3(256), 0, c->stream, (const int4*)slab.p, (int4*)host_dev, nq);
            CHK(check_launch(c, "k_copy_quads"));
        } else {
            HIPCHK(c, hipMemcpyAsync(host, slab.p, total, hipMemcpyDeviceToHost, c->stream));
        }
    }
    HIPCHK(c, hipStreamSynchronize(c->stream));
    return ARP_OK;
}
}  // namespace

int arp_fetch_packed(arp_ctx* c, void* host, uint64_t host_bytes, int64_t counts[5], uint64_t offsets[ARP_PACKED_OFFSETS], uint64_t* bytes_used) {
    if (!c || !counts || !offsets || !bytes_used) return ARP_E_ARG;
    if (!c->contacts_valid) FAIL(c, ARP_E_ARG, "arp_fetch_packed: no launch results");
    HIPCHK(c, hipSetDevice(c->device));
    if (c->packed_csr && c->has_gid) FAIL(c, ARP_E_ARG, "arp_fetch_packed: the row-offset layout needs packed atom ids (this context holds a shard with global ids)");
    return fetch_packed_from(c, PackedAtomBag{"arp_fetch_packed", c->n_contacts, c->packed_csr && !c->has_gid, nullptr}, host, host_bytes, counts, offsets, bytes_used);
}

int arp_atom_contacts(arp_ctx* c, double cutoff, double vdw_comp, int include_sequence_adjacent, int64_t cap, int32_t* out_i,
                      int32_t* out_j, float* out_dist, uint16_t* out_sift, uint8_t* out_ctype, int64_t* count) {
    if (!c || !count) return ARP_E_ARG;
    CHK(arp_atom_contacts_launch(c, cutoff, vdw_comp, include_sequence_adjacent, count));
    return arp_atom_contacts_fetch(c, cap, out_i, out_j, out_dist, out_sift, out_ctype, count);
}

// ---- per-atom accumulators of the contact loop (I:821-852, 923-934; U:182-221) ------------------------------
int arp_atom_accumulators(arp_ctx* c, uint16_t* out_sift4, int32_t* out_counts8) {
    if (!c || !out_sift4 || !out_counts8) return ARP_E_ARG;
    if (!c->contacts_valid) FAIL(c, ARP_E_ARG, "arp_atom_accumulators: no atom-contact results (call a launch first)");
    if (c->has_gid) FAIL(c, ARP_E_ARG, "arp_atom_accumulators: not available on a shard (contacts carry global ids)");
    HIPCHK(c, hipSetDevice(c->device));
    const size_t n = (size_t)std::max<int64_t>(c->n, 1);
    DevBuf<unsigned int> acc_s;
    DevBuf<int> acc_c;
    HIPCHK(c, acc_s.reserve(2 * n));
    HIPCHK(c, acc_c.reserve(8 * n));
    HIPCHK(c, hipMemsetAsync(acc_s.p, 0, 2 * n * sizeof(unsigned int), c->stream));
    HIPCHK(c, hipMemsetAsync(acc_c.p, 0, 8 * n * sizeof(int), c->stream));
    if (c->n_contacts > 0) {
        hipLaunchKernelGGL(k_accumulate, dim3(nblocks(c->n_contacts, 256, 4096)), dim3(256), 0, c->stream, (long long)c->n_contacts,
                           c->out_i.p, c->out_j.p, c->out_s.p, c->out_ct.p, acc_s.p, acc_c.p);
        CHK(check_launch(c, "k_accumulate"));
    }
    std::vector<unsigned int> hs(2 * n);
    int rc = download(c, hs.data(), acc_s.p, 2 * (size_t)c->n);
    if (rc == ARP_OK) rc = download(c, out_counts8, acc_c.p, 8 * (size_t)c->n);
    acc_s.release();
    acc_c.release();
    CHK(rc);
    for (int64_t a = 0; a < c->n; ++a) {   // {all, inter_only, intra_only, water_only}
        out_sift4[4 * a] = (uint16_t)(hs[2 * a] & 0x7FFF);
        out_sift4[4 * a + 1] = (uint16_t)((hs[2 * a] >> 16) & 0x7FFF);
        out_sift4[4 * a + 2] = (uint16_t)(hs[2 * a + 1] & 0x7FFF);
        out_sift4[4 * a + 3] = (uint16_t)((hs[2 * a + 1] >> 16) & 0x7FFF);
    }
    return ARP_OK;
}

int arp_atom_integer_sifts(arp_ctx* c, uint8_t* out_isift) {
    if (!c || !out_isift) return ARP_E_ARG;
    if (!c->contacts_valid) FAIL(c, ARP_E_ARG, "arp_atom_integer_sifts: no atom-contact results (call a launch first)");
    if (c->has_gid) FAIL(c, ARP_E_ARG, "arp_atom_integer_sifts: not available on a shard (contacts carry global ids)");
    HIPCHK(c, hipSetDevice(c->device));
    const size_t n4 = 4 * (size_t)std::max<int64_t>(c->n, 1);
    DevBuf<u64> last_rank;
    DevBuf<unsigned int> before, last_sift;
    DevBuf<uint8_t> out;
    HIPCHK(c, last_rank.reserve(n4));
    HIPCHK(c, before.reserve(n4));
    HIPCHK(c, last_sift.reserve(n4));
    HIPCHK(c, out.reserve(15 * n4));
    HIPCHK(c, hipMemsetAsync(last_rank.p, 0, n4 * sizeof(u64), c->stream));
    HIPCHK(c, hipMemsetAsync(before.p, 0, n4 * sizeof(unsigned int), c->stream));
    HIPCHK(c, hipMemsetAsync(last_sift.p, 0, n4 * sizeof(unsigned int), c->stream));
    if (c->n_contacts > 0) {
        const dim3 grid(nblocks(c->n_contacts, 256, 4096));
        hipLaunchKernelGGL(k_isift_last, grid, dim3(256), 0, c->stream, (long long)c->n_contacts, c->out_i.p, c->out_j.p,
                           c->out_ct.p, last_rank.p);
        hipLaunchKernelGGL(k_isift_fill, grid, dim3(256), 0, c->stream, (long long)c->n_contacts, c->out_i.p, c->out_j.p,
                           c->out_s.p, c->out_ct.p, last_rank.p, before.p, last_sift.p);
        CHK(check_launch(c, "k_isift_fill"));
    }
    hipLaunchKernelGGL(k_isift_compose, dim3((unsigned)((n4 + 255) / 256)), dim3(256), 0, c->stream, (long long)n4, before.p,
                       last_sift.p, out.p);
    CHK(check_launch(c, "k_isift_compose"));
    int rc = download(c, out_isift, out.p, 60 * (size_t)c->n);
    last_rank.release();
    before.release();
    last_sift.release();
    out.release();
    return rc;
}

// ---- ring / amide contacts: launch (results stay in HBM) + fetch ----------------------------------
// Which loops take the list path when called alone (measured on BASELINE configs[4], 10 k rings + 10 k amides, HIP events):
// plane-plane 22.5 -> 18.6 us from the list; atom-plane 37 -> 63 us (its list has 60 candidates per ring: the walk, which tests the
// atoms of a ring's cells as it meets them, does less); the two amide loops 19 - 20 us either way (a chain of five dependent round
// trips whatever evaluates 1.5 k records).  ARP_BAG_LISTS: bit k = loop k from its list (default 2: plane-plane), 0 = every loop by
// its grid walk as through round 5, 15 = all four from the lists (the way a whole pass evaluates them).
int arp_atom_plane_launch(arp_ctx* c, int64_t* count) { return c ? bag_launch(c, BAG_AP, count) : ARP_E_ARG; }
int arp_plane_plane_launch(arp_ctx* c, int64_t* count) { return c ? bag_launch(c, BAG_PP, count) : ARP_E_ARG; }
int arp_group_group_launch(arp_ctx* c, int64_t* count) { return c ? bag_launch(c, BAG_GG, count) : ARP_E_ARG; }
int arp_group_plane_launch(arp_ctx* c, int64_t* count) { return c ? bag_launch(c, BAG_GP, count) : ARP_E_ARG; }

namespace {
// Small bags travel to the host in one piece: the first *_fetch after a pass gathers the used prefix of every array of
// EVERY valid bag into one device buffer (k_pack_segments), copies it to page-locked memory and synchronises once; the
// fetch calls hand the arrays out from there — instead of six to nine small copies and a synchronisation per bag.
#define BAG_STAGE_MAX ((size_t)4 << 20)
int stage_bags(arp_ctx* c) {
    bool stale = false;
    for (const Bag& b : c->bag) stale = stale || (b.valid && b.staged_version != b.version);
    if (!stale) return ARP_OK;
    PackTable t;
    t.n = 0;
    size_t total = 0;
    for (int kind = 0; kind < BAG_KINDS; ++kind) {
        Bag& b = c->bag[kind];
        if (!b.valid) continue;
        total = bag_piece_layout(kind, (size_t)b.count, total, b.stage_off);
        for (int j = 0; j < BAG_COLS; ++j)      // (offsets beyond 32 bits: only when the total is past BAG_STAGE_MAX, and then unused)
            if (bag_has(kind, j) && b.count > 0) t.s[t.n++] = PackSeg{b.col[j], (uint32_t)b.stage_off[j], (uint32_t)((size_t)b.count * bag_es(kind, j)), nullptr, 0u};
    }
    if (total > BAG_STAGE_MAX) {   // big bags (configs[4]): array by array, as before
        for (Bag& b : c->bag) b.staged_version = 0;
        return ARP_OK;
    }
    if (total > 0) {
        if (c->bag_stage_cap < total) {
            if (c->bag_stage) (void)hipHostFree(c->bag_stage);
            c->bag_stage = nullptr;
            c->bag_stage_cap = 0;
            const size_t want = total + total / 2 + 4096;
            if (hipHostMalloc((void**)&c->bag_stage, want, hipHostMallocDefault) != hipSuccess) { c->bag_stage = nullptr; return ARP_OK; }
            c->bag_stage_cap = want;
        }
        HIPCHK(c, c->bag_pack.reserve(total));
        hipLaunchKernelGGL(k_pack_segments, pack_grid(t), dim3(256), 0, c->stream, t, c->bag_pack.p);
        CHK(check_launch(c, "k_pack_segments"));
        HIPCHK(c, hipMemcpyAsync(c->bag_stage, c->bag_pack.p, total, hipMemcpyDeviceToHost, c->stream));
        HIPCHK(c, hipStreamSynchronize(c->stream));
    } else if (!c->bag_stage) {    // nothing to copy, but "staged" needs a buffer to point into
        if (hipHostMalloc((void**)&c->bag_stage, 4096, hipHostMallocDefault) != hipSuccess) { c->bag_stage = nullptr; return ARP_OK; }
        c->bag_stage_cap = 4096;
    }
    for (Bag& b : c->bag)
        if (b.valid) b.staged_version = b.version;
    return ARP_OK;
}
// One bag to the caller's arrays: out[j] receives column j of the table (null: not wanted).  A too-small capacity returns
// ARP_E_CAPACITY with the required count.
int bag_fetch(arp_ctx* c, int kind, int64_t cap, void* const (&out)[BAG_COLS], int64_t* count) {
    if (!c || !count) return ARP_E_ARG;
    const Bag& b = c->bag[kind];
    auto what = [kind] { return std::string("arp_") + PLANE_TABLES[kind].name + "_fetch"; };
    if (!b.valid) FAIL(c, ARP_E_ARG, what() + ": no launch results");
    HIPCHK(c, hipSetDevice(c->device));
    *count = b.count;
    if (b.count > cap) FAIL(c, ARP_E_CAPACITY, what() + ": output buffer too small");
    CHK(stage_bags(c));
    const bool staged = c->bag_stage && b.staged_version == b.version && b.version != 0;
    for (int j = 0; j < BAG_COLS; ++j) {      // column by column: out of the stage, or a copy of its own
        const size_t bytes = (size_t)b.count * bag_es(kind, j);
        if (!bag_has(kind, j) || !out[j] || !bytes) continue;
        if (staged) memcpy(out[j], c->bag_stage + b.stage_off[j], bytes);
        else HIPCHK(c, hipMemcpyAsync(out[j], b.col[j], bytes, hipMemcpyDeviceToHost, c->stream));
    }
    if (!staged) HIPCHK(c, hipStreamSynchronize(c->stream));
    return ARP_OK;
}
// launch + fetch
int bag_launch_fetch(arp_ctx* c, int kind, int64_t cap, void* const (&out)[BAG_COLS], int64_t* count) {
    if (!c || !count || cap < 0) return ARP_E_ARG;
    CHK(bag_launch(c, kind, count));
    return bag_fetch(c, kind, cap, out, count);
}
}  // namespace

// The C entries name their columns; column j of the table is argument j behind cap (a table without value column 2, 3 or byte
// column 1, 2 has no such argument).
#define AP_COLS {out_atom, out_ring, out_dist, out_theta, nullptr, nullptr, out_mask, out_ctype, nullptr}
#define PP_COLS {out_bgn, out_end, out_dist, out_dihedral, out_theta_bgn, out_theta_end, out_type1, out_type2, out_ctype}
#define GG_COLS {out_bgn, out_end, out_dist, out_dihedral, out_theta, nullptr, out_ctype, nullptr, nullptr}
#define GP_COLS {out_amide, out_ring, out_dist, out_dihedral, out_theta, nullptr, out_ctype, nullptr, nullptr}
int arp_atom_plane_fetch(arp_ctx* c, int64_t cap, int32_t* out_atom, int32_t* out_ring, double* out_dist, double* out_theta,
                         uint8_t* out_mask, uint8_t* out_ctype, int64_t* count) {
    return bag_fetch(c, BAG_AP, cap, AP_COLS, count);
}
int arp_plane_plane_fetch(arp_ctx* c, int64_t cap, int32_t* out_bgn, int32_t* out_end, double* out_dist, double* out_dihedral,
                          double* out_theta_bgn, double* out_theta_end, uint8_t* out_type1, uint8_t* out_type2,
                          uint8_t* out_ctype, int64_t* count) {
    return bag_fetch(c, BAG_PP, cap, PP_COLS, count);
}
int arp_group_group_fetch(arp_ctx* c, int64_t cap, int32_t* out_bgn, int32_t* out_end, float* out_dist, float* out_dihedral,
                          float* out_theta, uint8_t* out_ctype, int64_t* count) {
    return bag_fetch(c, BAG_GG, cap, GG_COLS, count);
}
int arp_group_plane_fetch(arp_ctx* c, int64_t cap, int32_t* out_amide, int32_t* out_ring, double* out_dist, double* out_dihedral,
                          double* out_theta, uint8_t* out_ctype, int64_t* count) {
    return bag_fetch(c, BAG_GP, cap, GP_COLS, count);
}

// launch + fetch.  A too-small caller buffer returns ARP_E_CAPACITY with the required count.
int arp_atom_plane(arp_ctx* c, int64_t cap, int32_t* out_atom, int32_t* out_ring, double* out_dist, double* out_theta,
                   uint8_t* out_mask, uint8_t* out_ctype, int64_t* count) {
    return bag_launch_fetch(c, BAG_AP, cap, AP_COLS, count);
}
int arp_plane_plane(arp_ctx* c, int64_t cap, int32_t* out_bgn, int32_t* out_end, double* out_dist, double* out_dihedral,
                    double* out_theta_bgn, double* out_theta_end, uint8_t* out_type1, uint8_t* out_type2, uint8_t* out_ctype,
                    int64_t* count) {
    return bag_launch_fetch(c, BAG_PP, cap, PP_COLS, count);
}
int arp_group_group(arp_ctx* c, int64_t cap, int32_t* out_bgn, int32_t* out_end, float* out_dist, float* out_dihedral,
                    float* out_theta, uint8_t* out_ctype, int64_t* count) {
    return bag_launch_fetch(c, BAG_GG, cap, GG_COLS, count);
}
int arp_group_plane(arp_ctx* c, int64_t cap, int32_t* out_amide, int32_t* out_ring, double* out_dist, double* out_dihedral,
                    double* out_theta, uint8_t* out_ctype, int64_t* count) {
    return bag_launch_fetch(c, BAG_GP, cap, GP_COLS, count);
}
#undef AP_COLS
#undef PP_COLS
#undef GG_COLS
#undef GP_COLS

// ---- run_arpeggio (I:329-347): every stage enqueued back to back, ONE host synchronisation ---------
namespace {
// One pass = enqueue (everything back to back on the context's stream, no host synchronisation) + wait (the one host wait,
// capacity checks, a re-run if a buffer was too small).  arp_run_launch is the two in a row; arp_run_enqueue / arp_run_wait
// give them to the caller separately, so that ONE host thread keeps several contexts busy.
int run_pass_enqueue(arp_ctx* c, double cutoff, double vdw_comp, int include_sequence_adjacent, double expand_radius) {
    HIPCHK(c, hipSetDevice(c->device));
    CHK(default_selection(c));  // no selection uploaded for this structure: whole structure (I:1395)
    if (c->whole_structure && !c->sel_all)
        FAIL(c, ARP_E_ARG, "arp_run_launch: arp_set_whole_structure is on but the uploaded selection is partial");
    // every stage enqueued back to back (no host synchronisation, no allocation once the buffers are sized)
    // the counter block must be zero when a pass starts; a pass leaves it zeroed (k_publish_counters)
    auto ensure_zero = [&]() -> int {
        if (!c->ctr_zero_ok) HIPCHK(c, hipMemsetAsync(c->d_ctr, 0, sizeof(u64) * C_DEV_WORDS, c->stream));
        c->ctr_zero_ok = false;
        return ARP_OK;
    };
    auto enqueue_all = [&]() -> int {
        c->ctr_clean = true;
        struct Unclean { arp_ctx* c; ~Unclean() { c->ctr_clean = false; c->pub.expected = 0; c->fuse_sets = false; c->init_plus_in_bin = false; } } unclean{c};
        CHK(ensure_static(c, cutoff));       // (the spatial order of the columns is the one of this pass's cells)
        c->last_cutoff = cutoff;
        // The pass ends inside its last kernel (k_sift_planes): the last block to finish publishes the counters.
        c->pub = PublishArgs{c->d_ctr, c->h_ctr_pinned, 0, 0};
        if (sw().inkernel_publish && !c->external_stream) {
            c->pub.expected = 1;
            c->pub.seq = ++c->publish_seq;
        }
        // _make_selection (I:1384-1424).  Whole-structure selection (the reference's default, I:1395 with no
        // selectors): selection_plus is the selection, nothing to search.  A small selection (ligand, binding site:
        // nsel <= SMALL_SEL_MAX, worth it while the N x S direct tests stay below ~1.7e7) gets selection_plus from a
        // direct test of every atom against the selected ones — one short kernel.  Anything else: the all-atom 6 A
        // grid and the expansion search.
        // (not for several structures in one pass: their coordinates overlap, only the grid keeps them apart)
        const bool small_sel = !c->sel_all && c->nsel > 0 && c->nsel <= SMALL_SEL_MAX && c->n > 0 && !c->has_home &&
                               c->n * c->nsel <= (int64_t)1 << 24 && c->batch_n == 0;
        if (c->sel_all || small_sel) {
            c->sel_made = true;
            HIPCHK(c, c->plus.reserve((size_t)std::max<int64_t>(c->n, 1)));
            c->contacts_valid = false;
            c->void_bags();
            c->init_plus_in_bin = c->sel_all;      // selection_plus = selection: written by the contact grid's binning kernel
        } else {
            CHK(enqueue_expansion(c, expand_radius));                                // I:342 (I:1384-1424)
        }
        if (small_sel) {
            Prof p(c, SLOT_MARK);
            hipLaunchKernelGGL(k_expand_small, dim3(nblocks(c->n, 256, 1 << 22)), dim3(256), 0, c->stream, (int)c->n, c->xyz.p, c->sel_list.p,
                               (int)c->nsel, c->sel.p, expand_radius * expand_radius, c->plus.p, c->d_ctr + ctr_dev(C_STAT_MCAND));
            CHK(check_launch(c, "k_expand_small"));
        }
        // (ring / amide grids, built once per structure: with the candidate lists, in enqueue_contacts)
        // I:1413-1437 (residue / ring / amide sets) ride on the contact grid build, I:345-347 in three launches
        c->fuse_sets = true;
        CHK(enqueue_contacts(c, cutoff, vdw_comp, include_sequence_adjacent, true));
        if (c->pub.expected) return ARP_OK;                                         // the last kernel publishes (pass_end)
        return enqueue_counter_copy(c, 1);
    };
    const auto t0 = std::chrono::steady_clock::now();
    CHK(ensure_zero());
    CHK(enqueue_all());
    c->host_enqueue_us += std::chrono::duration<double, std::micro>(std::chrono::steady_clock::now() - t0).count();
    return ARP_OK;
}

int run_pass_wait(arp_ctx* c, int64_t counts[5]) {
    HIPCHK(c, hipSetDevice(c->device));
    for (int attempt = 0;; ++attempt) {
        const auto t1 = std::chrono::steady_clock::now();
        CHK(collect_counters(c));
        c->ctr_zero_ok = true;
        c->host_wait_us += std::chrono::duration<double, std::micro>(std::chrono::steady_clock::now() - t1).count();
        ++c->host_passes;
        collect_events(c);
        const int again = finish_pass(c);
        if (again < 0) return again;
        if (!again) break;
        if (attempt == 2) FAIL(c, ARP_E_CAPACITY, "arp_run_launch: result buffers could not be sized");
        CHK(run_pass_enqueue(c, c->pending_cutoff, c->pending_comp, c->pending_seq_adj, c->pending_expand));   // a buffer was too small: once more
    }
    pass_counts(c, counts);
    const int rc_dev = device_error(c);
    if (rc_dev == ARP_OK && c->sort_after_pass && c->contacts_valid && c->n_contacts > 0 && c->n_contacts < ((int64_t)1 << 31)) {
        // (room for the ring / amide bags behind the sorted columns, as arp_fetch_packed lays them out.  An upper bound — every
        // record counted as the table's largest, every column as rounded up by a whole 16 bytes —, so that the fetch finds the room
        // and does not sort again)
        size_t records = 0;
        for (const Bag& b : c->bag) records += (size_t)b.count;
        CHK(sort_contacts(c, bag_piece_bound(records)));
    }
    return rc_dev;
}
}  // namespace

int arp_run_enqueue(arp_ctx* c, double cutoff, double vdw_comp, int include_sequence_adjacent, double expand_radius) {
    if (!c || !(cutoff > 0) || !(expand_radius > 0)) return ARP_E_ARG;
    if (c->pass_pending) FAIL(c, ARP_E_ARG, "arp_run_enqueue: the previous pass has not been waited for (arp_run_wait)");
    c->pending_cutoff = cutoff; c->pending_comp = vdw_comp; c->pending_seq_adj = include_sequence_adjacent; c->pending_expand = expand_radius;
    CHK(run_pass_enqueue(c, cutoff, vdw_comp, include_sequence_adjacent, expand_radius));
    c->pass_pending = true;
    return ARP_OK;
}

int arp_run_wait(arp_ctx* c, int64_t counts[5]) {
    if (!c) return ARP_E_ARG;
    if (!c->pass_pending) FAIL(c, ARP_E_ARG, "arp_run_wait: no pass was enqueued (arp_run_enqueue)");
    c->pass_pending = false;
    return run_pass_wait(c, counts);
}

int arp_run_launch(arp_ctx* c, double cutoff, double vdw_comp, int include_sequence_adjacent, double expand_radius,
                   int64_t counts[5]) {
    CHK(arp_run_enqueue(c, cutoff, vdw_comp, include_sequence_adjacent, expand_radius));
    return arp_run_wait(c, counts);
}

// ---- staged run_arpeggio for sharded runs ------------------------------------------------------------
int arp_device_buffer(arp_ctx* c, int which, uint64_t* device_ptr, int64_t* bytes) {
    if (!c || !device_ptr || !bytes) return ARP_E_ARG;
    if (which == ARP_BUF_PLUS) {
        if (!c->plus.p) FAIL(c, ARP_E_ARG, "arp_device_buffer: selection_plus does not exist yet (run stage 0 first)");
        *device_ptr = (uint64_t)(uintptr_t)c->plus.p;
        *bytes = c->n;
    } else if (which == ARP_BUF_RES_SETS) {
        if (!c->res_sel.p) FAIL(c, ARP_E_ARG, "arp_device_buffer: residue sets do not exist yet (run stage 1 first)");
        *device_ptr = (uint64_t)(uintptr_t)c->res_sel.p;
        *bytes = 2 * std::max<int64_t>(c->nres, 1);
    } else if (which == ARP_BUF_GRID_START) {
        if (!c->atom_grid.valid || !c->atom_grid.start.p) FAIL(c, ARP_E_ARG, "arp_device_buffer: no contact grid is in place");
        *device_ptr = (uint64_t)(uintptr_t)c->atom_grid.start.p;
        *bytes = ((int64_t)c->atom_grid.d.ncell + 1) * (int64_t)sizeof(int);
    } else if (which == ARP_BUF_KEEP_BASE) {
        if (!c->compact_used_table) FAIL(c, ARP_E_ARG, "arp_device_buffer: the last grid build did not read the table of block bases");
        *device_ptr = (uint64_t)(uintptr_t)(c->sp_keep.p + 4 + c->sp_keep_blocks);
        *bytes = ((int64_t)c->sp_keep_blocks + 1) * (int64_t)sizeof(int);
    } else FAIL(c, ARP_E_ARG, "arp_device_buffer: unknown buffer");
    return ARP_OK;
}

int arp_run_stage(arp_ctx* c, int stage, double cutoff, double vdw_comp, int include_sequence_adjacent, double expand_radius,
                  int64_t counts[5]) {
    if (!c || stage < 0 || stage > 2) return ARP_E_ARG;
    c->ctr_zero_ok = false;
    HIPCHK(c, hipSetDevice(c->device));
    if (stage == 0) {          // I:1384-1424 on the local atoms; exact for the atoms this rank owns
        if (!(expand_radius > 0)) return ARP_E_ARG;
        CHK(default_selection(c));
        HIPCHK(c, hipMemsetAsync(c->d_ctr, 0, sizeof(u64) * C_DEV_WORDS, c->stream));
        c->ctr_clean = true;
        int rc = enqueue_expansion(c, expand_radius);
        c->ctr_clean = false;
        CHK(rc);
        if (!c->external_stream && !c->comm) HIPCHK(c, hipStreamSynchronize(c->stream));   // (with a communicator the exchange follows on the same stream)
        return ARP_OK;
    }
    if (!c->sel_made) FAIL(c, ARP_E_ARG, "arp_run_stage: stage 0 has not run");
    if (stage == 1) {          // I:1413, 1431 residue sets from the (now globally correct) selection_plus bits
        const int n = (int)c->n;
        const size_t nres = (size_t)std::max<int64_t>(c->nres, 1);
        CHK(check_residue_ranges(c));
        HIPCHK(c, c->res_sel.reserve(2 * nres));
        HIPCHK(c, hipMemsetAsync(c->res_sel.p, 0, 2 * nres, c->stream));
        if (n > 0)
            hipLaunchKernelGGL(k_res_mark, dim3(nblocks(n, 256)), dim3(256), 0, c->stream, n, c->res_id.p, c->sel.p, c->plus.p,
                               c->res_sel.p, c->res_sel.p + nres);
        CHK(check_launch(c, "k_res_mark"));
        if (!c->external_stream && !c->comm) HIPCHK(c, hipStreamSynchronize(c->stream));   // (with a communicator the exchange follows on the same stream)
        return ARP_OK;
    }
    // stage 2: ring / amide sets from the (now globally reduced) residue sets, then every contact bag
    if (!(cutoff > 0)) return ARP_E_ARG;
    if (!c->res_sel.p) FAIL(c, ARP_E_ARG, "arp_run_stage: stage 1 has not run");
    for (int attempt = 0;; ++attempt) {
        const size_t nres = (size_t)std::max<int64_t>(c->nres, 1);
        // the expansion statistics of stage 0 live in the counter block: keep them, clear the rest
        HIPCHK(c, hipMemsetAsync(c->d_ctr, 0, sizeof(u64) * 5 * CTR_LINE, c->stream));                      // scalars, the four bags
        HIPCHK(c, hipMemset2DAsync(c->d_ctr + ctr_dev(C_STAT_CAND), sizeof(u64) * CTR_LINE, 0, 2 * sizeof(u64), STAT_SLOTS, c->stream));
        HIPCHK(c, hipMemsetAsync(c->d_ctr + ctr_dev(C_SEG_PAIRS), 0, sizeof(u64) * PAIR_SEGS * CTR_LINE, c->stream));
        c->ctr_clean = true;
        struct Unclean { arp_ctx* c; ~Unclean() { c->ctr_clean = false; } } unclean{c};
        if (c->nring + c->namide > 0)
            hipLaunchKernelGGL(k_group_mask, dim3(nblocks(c->nring + c->namide, 256)), dim3(256), 0, c->stream, (int)c->nring,
                               (int)c->namide, c->ring_res.p, c->am_res.p, c->res_sel.p, c->res_sel.p + nres, c->ring_sel.p,
                               c->ring_plus.p, c->am_sel.p, c->am_plus.p);
        CHK(check_launch(c, "k_group_mask"));
        CHK(ensure_center_grids(c));
        CHK(enqueue_contacts(c, cutoff, vdw_comp, include_sequence_adjacent, true));
        CHK(enqueue_counter_copy(c));
        CHK(collect_counters(c));
        collect_events(c);
        const int again = finish_pass(c);
        if (again < 0) return again;
        if (!again) break;
        if (attempt == 2) FAIL(c, ARP_E_CAPACITY, "arp_run_stage: result buffers could not be sized");
    }
    pass_counts(c, counts);
    return device_error(c);
}

// ---- measurement -------------------------------------------------------------------------------
int arp_get_stats(arp_ctx* c, int64_t stats[8]) {
    if (!c || !stats) return ARP_E_ARG;
    for (int k = 0; k < 8; ++k) stats[k] = c->stats[k];
    stats[7] = c->batch_restarts;
    return ARP_OK;
}

int arp_set_profiling(arp_ctx* c, int enabled) {
    if (!c) return ARP_E_ARG;
    c->profiling = enabled != 0;   // launches bracketed by HIP events on their own streams
    return ARP_OK;
}

int arp_get_kernel_times(arp_ctx* c, double ms[8], int64_t launches[8], int reset) {
    if (!c || !ms || !launches) return ARP_E_ARG;
    for (int k = 0; k < NSLOT; ++k) { ms[k] = c->k_ms[k]; launches[k] = c->k_launches[k]; }
    if (reset) for (int k = 0; k < NSLOT; ++k) { c->k_ms[k] = 0; c->k_launches[k] = 0; }
    return ARP_OK;
}

// ---- geometric part of initialize() --------------------------------------------------
int arp_ring_geometry(arp_ctx* c, int64_t nring, const int32_t* ring_off, const int32_t* ring_idx, double* out_center,
                      double* out_normal) {
    if (!c || nring < 0 || (nring > 0 && (!ring_off || !out_center || !out_normal))) return ARP_E_ARG;
    if (nring == 0) return ARP_OK;
    CHK(check_ring_atoms(c, "arp_ring_geometry", nring, ring_off, ring_idx, c->n));
    const int64_t m = ring_off[nring];
    HIPCHK(c, hipSetDevice(c->device));
    DevBuf<int> d_off, d_idx;
    DevBuf<double> d_c, d_n;
    int rc = upload(c, d_off, ring_off, (size_t)nring + 1);
    if (rc == ARP_OK) rc = upload(c, d_idx, ring_idx, (size_t)m);
    hipError_t e = d_c.reserve((size_t)nring * 3);
    if (e == hipSuccess) e = d_n.reserve((size_t)nring * 3);
    if (rc == ARP_OK && e == hipSuccess) {
        hipLaunchKernelGGL(k_ring_geometry, dim3(nblocks(nring, 256)), dim3(256), 0, c->stream, 1, (int)c->n, (int)nring, d_off.p,
                           d_idx.p, c->xyz.p, d_c.p, d_n.p);
        rc = check_launch(c, "k_ring_geometry");
        if (rc == ARP_OK) rc = download(c, out_center, d_c.p, (size_t)nring * 3);
        if (rc == ARP_OK) rc = download(c, out_normal, d_n.p, (size_t)nring * 3);
    }
    d_off.release(); d_idx.release(); d_c.release(); d_n.release();
    if (e != hipSuccess) FAIL(c, ARP_E_NOMEM, "arp_ring_geometry: out of device memory");
    return rc;
}

int arp_amide_geometry(arp_ctx* c, int64_t namide, const int32_t* amide_atoms, float* out_center, float* out_normal) {
    if (!c || namide < 0 || (namide > 0 && (!amide_atoms || !out_center || !out_normal))) return ARP_E_ARG;
    if (namide == 0) return ARP_OK;
    CHK(check_amide_atoms(c, "arp_amide_geometry", namide, amide_atoms, c->n));
    HIPCHK(c, hipSetDevice(c->device));
    DevBuf<int> d_at;
    DevBuf<float> d_c, d_n;
    int rc = upload(c, d_at, amide_atoms, (size_t)namide * 4);
    hipError_t e = d_c.reserve((size_t)namide * 3);
    if (e == hipSuccess) e = d_n.reserve((size_t)namide * 3);
    if (rc == ARP_OK && e == hipSuccess) {
        hipLaunchKernelGGL(k_amide_geometry, dim3(nblocks(namide, 256)), dim3(256), 0, c->stream, 1, (int)c->n, (int)namide, d_at.p,
                           c->xyz.p, d_c.p, d_n.p);
        rc = check_launch(c, "k_amide_geometry");
        if (rc == ARP_OK) rc = download(c, out_center, d_c.p, (size_t)namide * 3);
        if (rc == ARP_OK) rc = download(c, out_normal, d_n.p, (size_t)namide * 3);
    }
    d_at.release(); d_c.release(); d_n.release();
    if (e != hipSuccess) FAIL(c, ARP_E_NOMEM, "arp_amide_geometry: out of device memory");
    return rc;
}

int arp_ring_residues(arp_ctx* c, int64_t nring, const double* center, int32_t* out_ring_res, double* out_shortest) {
    if (!c || nring < 0 || (nring > 0 && (!center || !out_ring_res))) return ARP_E_ARG;
    if (nring == 0) return ARP_OK;
    if (!all_finite(center, 3 * nring)) FAIL(c, ARP_E_ARG, "arp_ring_residues: non-finite ring centre");
    HIPCHK(c, hipSetDevice(c->device));
    if (c->n == 0) {
        for (int64_t r = 0; r < nring; ++r) { out_ring_res[r] = -1; if (out_shortest) out_shortest[r] = -1.0; }
        return ARP_OK;
    }
    // the all-atom grid (hydrogens included, I:1455); its cells (>= 6 A) cover the 3 A query with the 27-cell stencil
    // (with a batch or models resident: over all of them, in world coordinates — build_world_grid)
    if (c->batch_n > 0) CHK(build_world_grid(c, 6.0));
    else if (!(c->all_grid_current && c->all_grid.valid && c->all_grid.radius == 6.0)) CHK(build_all_grid(c, 6.0));
    DevBuf<double> d_c, d_d;
    DevBuf<int> d_r;
    int rc = upload(c, d_c, center, (size_t)nring * 3);
    hipError_t e = d_r.reserve((size_t)nring);
    if (e == hipSuccess) e = d_d.reserve((size_t)nring);
    if (rc == ARP_OK && e == hipSuccess) {
        hipLaunchKernelGGL(k_ring_residue, dim3(nblocks(nring * 64, 256, 4096)), dim3(256), 0, c->stream, c->all_grid.d,
                           c->all_grid.start.p, c->a_xyzm.p, c->a_aux.p, (int)nring, d_c.p, (const int*)nullptr, d_r.p, d_d.p);
        rc = check_launch(c, "k_ring_residue");
        if (rc == ARP_OK) rc = download(c, out_ring_res, d_r.p, (size_t)nring);
        if (rc == ARP_OK && out_shortest) rc = download(c, out_shortest, d_d.p, (size_t)nring);
    }
    d_c.release(); d_r.release(); d_d.release();
    if (e != hipSuccess) FAIL(c, ARP_E_NOMEM, "arp_ring_residues: out of device memory");
    return rc;
}

int arp_search(arp_ctx* c, double radius, int64_t ncenters, const double* centers, int64_t cap, int32_t* out_center, int32_t* out_atom,
               int64_t* count) {
    if (!c || !count || ncenters < 0 || cap < 0 || !(radius > 0) || (ncenters > 0 && !centers)) return ARP_E_ARG;
    *count = 0;
    if (ncenters == 0 || c->n == 0) return ARP_OK;
    if (ncenters > 0x7FFFFFF0LL) FAIL(c, ARP_E_ARG, "arp_search: too many centres");
    if (!all_finite(centers, 3 * ncenters)) FAIL(c, ARP_E_ARG, "arp_search: non-finite centre");
    HIPCHK(c, hipSetDevice(c->device));
    if (c->batch_n > 0) CHK(build_world_grid(c, std::max(radius, 6.0)));      // (all resident atoms, world coordinates)
    else if (!(c->all_grid_current && c->all_grid.valid && c->all_grid.radius >= radius)) CHK(build_all_grid(c, std::max(radius, 6.0)));
    DevBuf<double> d_c;
    DevBuf<int2> d_out;
    DevBuf<u64> d_n;
    int rc = upload(c, d_c, centers, (size_t)ncenters * 3);
    hipError_t e = d_out.reserve((size_t)std::max<int64_t>(cap, 1));
    if (e == hipSuccess) e = d_n.reserve(1);
    u64 found = 0;
    std::vector<int2> tmp;
    if (rc == ARP_OK && e == hipSuccess) {
        e = hipMemsetAsync(d_n.p, 0, sizeof(u64), c->stream);
        hipLaunchKernelGGL(k_center_search, dim3(nblocks(ncenters * 64, 256, 4096)), dim3(256), 0, c->stream, c->all_grid.d, c->all_grid.start.p,
                           c->a_xyzm.p, c->a_aux.p, (int)ncenters, d_c.p, radius * radius, d_out.p, (u64)cap, d_n.p);
        rc = check_launch(c, "k_center_search");
        if (rc == ARP_OK) rc = download(c, &found, d_n.p, 1);
        if (rc == ARP_OK && found <= (u64)cap && found > 0) {
            tmp.resize((size_t)found);
            rc = download(c, tmp.data(), d_out.p, (size_t)found);
        }
    }
    d_c.release(); d_out.release(); d_n.release();
    if (e != hipSuccess) FAIL(c, ARP_E_NOMEM, "arp_search: out of device memory");
    if (rc != ARP_OK) return rc;
    *count = (int64_t)found;
    if (found > (u64)cap) FAIL(c, ARP_E_CAPACITY, "arp_search: output buffer too small");
    std::sort(tmp.begin(), tmp.end(), [](const int2& a, const int2& b) { return a.x != b.x ? a.x < b.x : a.y < b.y; });
    for (size_t k = 0; k < tmp.size(); ++k) {
        if (out_center) out_center[k] = tmp[k].x;
        if (out_atom) out_atom[k] = tmp[k].y;
    }
    return ARP_OK;
}

// Page-locked host memory for result buffers (and inputs): copies to / from it are DMA transfers at PCIe speed,
// pageable memory goes through the runtime's staging buffer at a fraction of that.
int arp_host_alloc(uint64_t bytes, void** out) {
    if (!out) return ARP_E_ARG;
    *out = nullptr;
    if (bytes == 0) return ARP_OK;
    return hipHostMalloc(out, (size_t)bytes, hipHostMallocDefault) == hipSuccess ? ARP_OK : ARP_E_NOMEM;
}
int arp_host_free(void* p) {
    if (!p) return ARP_OK;
    return hipHostFree(p) == hipSuccess ? ARP_OK : ARP_E_HIP;
}

int arp_batch_layout(int64_t nstruct, const double* boxes, double radius, int32_t* places_out, int32_t dims_out[3], double* edge_out) {
    return batch_layout_c(nstruct, boxes, radius, places_out, dims_out, edge_out) == 0 ? ARP_OK : ARP_E_ARG;
}

int arp_set_batch(arp_ctx* c, int64_t nstruct, const int64_t* atom_off, const int64_t* ring_off, const int64_t* amide_off,
                  const double* boxes) {
    if (!c) return ARP_E_ARG;
    CHK(join_upload_lists(c));
    if (nstruct == 0) {   // back to one structure
        inputs_changed(c, IN_BATCH);
        return ARP_OK;
    }
    if (nstruct < 0 || !atom_off || !ring_off || !amide_off || !boxes) FAIL(c, ARP_E_ARG, "arp_set_batch: bad input");
    if (c->has_home || c->has_gid || c->shard_resident) FAIL(c, ARP_E_ARG, "arp_set_batch: not for a shard of a distributed structure");
    auto check = [&](const int64_t* off, int64_t total) {
        if (off[0] != 0 || off[nstruct] != total) return false;
        for (int64_t s_ = 0; s_ < nstruct; ++s_)
            if (off[s_ + 1] < off[s_]) return false;
        return true;
    };
    if (!check(atom_off, c->n) || !check(ring_off, c->nring) || !check(amide_off, c->namide))
        FAIL(c, ARP_E_ARG, "arp_set_batch: offsets must start at 0, never decrease and end at the resident atom / ring / amide counts");
    for (int64_t k = 0; k < nstruct; ++k)
        for (int a = 0; a < 3; ++a) {
            const double lo = boxes[6 * k + a], hi = boxes[6 * k + 3 + a];
            if (!std::isfinite(lo) || !std::isfinite(hi) || hi < lo || !std::isfinite(hi - lo))
                FAIL(c, ARP_E_ARG, "arp_set_batch: a box is not finite or has hi < lo");
        }
    HIPCHK(c, hipSetDevice(c->device));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    inputs_changed(c, IN_BATCH);
    release_batch_tables(c);      // (the stream has drained, and with it whatever the second stream did for a pass)
    c->batch_restarts = 0;
    c->batch_atom_off.assign(atom_off, atom_off + nstruct + 1);
    c->batch_ring_off.assign(ring_off, ring_off + nstruct + 1);
    c->batch_amide_off.assign(amide_off, amide_off + nstruct + 1);
    c->batch_box.assign(boxes, boxes + 6 * nstruct);
    // structure of every atom / ring / amide: made on the device from the three offset tables (building and uploading three
    // arrays of that length on the host was 160 us of a 64-structure batch)
    {
        const size_t m = (size_t)nstruct + 1;
        std::vector<long long> h(3 * m);
        for (size_t k = 0; k < m; ++k) { h[k] = atom_off[k]; h[m + k] = ring_off[k]; h[2 * m + k] = amide_off[k]; }
        CHK(upload(c, c->batch_off_dev, h.data(), h.size()));        // (waits: the staging vector ends here)
        const int64_t tot[3] = {c->n, c->nring, c->namide};
        DevBuf<int>* dst[3] = {&c->sid_atom, &c->sid_ring, &c->sid_amide};
        for (int k = 0; k < 3; ++k) {
            HIPCHK(c, dst[k]->reserve((size_t)std::max<int64_t>(tot[k], 1)));
            if (tot[k] > 0)
                hipLaunchKernelGGL(k_fill_sid, dim3(nblocks(tot[k], 256)), dim3(256), 0, c->stream, c->batch_off_dev.p + k * m, (int)nstruct, dst[k]->p, (long long)tot[k]);
        }
        CHK(check_launch(c, "k_fill_sid"));
    }
    c->batch_n = nstruct;
    return ARP_OK;
}

// ---- one topology, several models (arp_models.h) ----------------------------------------------------------------------
int arp_set_topology(arp_ctx* c, const void* blob, uint64_t bytes, const int32_t* ring_off, const int32_t* ring_idx,
                     const int32_t* amide_atoms) {
    if (!c || !blob || bytes < sizeof(arp_blob_header)) return ARP_E_ARG;
    if (c->has_home || c->has_gid || c->shard_resident) FAIL(c, ARP_E_ARG, "arp_set_topology: not for a shard of a distributed structure");
    arp_blob_header h;
    memcpy(&h, blob, sizeof(h));
    CHK(check_blob_header(c, h, bytes));
    const int64_t R = h.nring, A = h.namide;
    if ((R > 0 && (!ring_off || !ring_idx)) || (A > 0 && !amide_atoms)) FAIL(c, ARP_E_ARG, "arp_set_topology: ring or amide atoms missing");
    CHK(check_ring_atoms(c, "arp_set_topology", R, ring_off, ring_idx, h.n));
    CHK(check_amide_atoms(c, "arp_set_topology", A, amide_atoms, h.n));
    HIPCHK(c, hipSetDevice(c->device));
    CHK(join_upload_lists(c));
    c->has_topo = false;
    const int32_t zero = 0;
    CHK(upload(c, c->topo_dev, (const uint8_t*)blob, (size_t)h.bytes));
    CHK(upload(c, c->topo_ring_off, R > 0 ? ring_off : &zero, (size_t)R + 1));
    CHK(upload(c, c->topo_ring_idx, ring_idx, R > 0 ? (size_t)ring_off[R] : 0));
    CHK(upload(c, c->topo_amide_atoms, amide_atoms, (size_t)(4 * A)));
    c->topo_hdr = h;
    c->has_topo = true;
    return ARP_OK;
}

int arp_set_models(arp_ctx* c, int64_t nmodel, const float* xyz, const double* h_xyz) {
    if (!c) return ARP_E_ARG;
    if (c->has_home || c->has_gid || c->shard_resident) FAIL(c, ARP_E_ARG, "arp_set_models: not for a shard of a distributed structure");
    if (!c->has_topo) FAIL(c, ARP_E_ARG, "arp_set_models: no topology (arp_set_topology first)");
    const arp_blob_header& t = c->topo_hdr;
    if (nmodel < 1) FAIL(c, ARP_E_ARG, "arp_set_models: at least one model");
    const int64_t lim = (int64_t)1 << 31;
    auto reaches = [&](int64_t per) { return per > 0 && nmodel >= (lim + per - 1) / per; };     // nmodel * per >= 2^31
    if (nmodel >= lim || reaches(t.n) || reaches(t.nbond) || reaches(3 * t.nh))
        FAIL(c, ARP_E_ARG, "arp_set_models: F n, F nbond and 3 F nh must stay below 2^31");
    if ((t.n > 0 && !xyz) || (t.nh > 0 && !h_xyz)) FAIL(c, ARP_E_ARG, "arp_set_models: coordinates missing");
    const int64_t F = nmodel;
    arp_blob_header h;
    if (!blob_header(F * t.n, F * t.nres, F * t.nbond, F * t.nh, F * t.nring, F * t.namide, h))
        FAIL(c, ARP_E_ARG, "arp_set_models: counts out of range");
    h.n_rad = t.n_rad;
    HIPCHK(c, hipSetDevice(c->device));
    CHK(join_upload_lists(c));
    // From here on the resident arrays are overwritten: a failure leaves no structure resident (the topology stays kept).
    drop_resident(c);
    auto fail = [&](int rc) -> int {
        const std::string why = c->err;
        (void)hipStreamSynchronize(c->stream);
        c->err = why;
        drop_resident(c);
        return rc;
    };
    if (c->blob_dev.reserve((size_t)h.bytes) != hipSuccess || c->models_box.reserve((size_t)(18 * F)) != hipSuccess ||
        c->models_xyz.reserve((size_t)std::max<int64_t>(3 * h.n, 1)) != hipSuccess) {
        c->err = "arp_set_models: out of device memory";
        return fail(ARP_E_NOMEM);
    }
    uint8_t* const d = c->blob_dev.p;
    const uint8_t* const tp = c->topo_dev.p;
    hipError_t e = hipSuccess;
    if (h.n > 0) e = hipMemcpyAsync(c->models_xyz.p, xyz, (size_t)(3 * h.n) * sizeof(float), hipMemcpyHostToDevice, c->stream);
    if (e == hipSuccess && h.nh > 0)
        e = hipMemcpyAsync(blob_at<double>(d, h, BLOB_H_XYZ), h_xyz, (size_t)(3 * h.nh) * sizeof(double), hipMemcpyHostToDevice, c->stream);
    if (e != hipSuccess) { c->err = std::string("arp_set_models: copy of the coordinates: ") + hipGetErrorString(e); return fail(ARP_E_HIP); }
    ModelsExpand E;
    E.F = (int)F; E.n = (int)t.n; E.nres = (int)t.nres; E.nbond = (int)t.nbond; E.nh = (int)t.nh; E.nring = (int)t.nring; E.namide = (int)t.namide;
    E.xyz_in = c->models_xyz.p;                             E.xyz4 = blob_at<float4>(d, h, BLOB_XYZ);
    E.t_rad = blob_at<double2>(tp, t, BLOB_RAD);            E.rad = blob_at<double2>(d, h, BLOB_RAD);
    E.t_tmask = blob_at<uint16_t>(tp, t, BLOB_TMASK);       E.tmask = blob_at<uint16_t>(d, h, BLOB_TMASK);
    E.t_flags = blob_at<uint16_t>(tp, t, BLOB_FLAGS);       E.flags = blob_at<uint16_t>(d, h, BLOB_FLAGS);
    E.t_rad_idx = blob_at<uint16_t>(tp, t, BLOB_RAD_IDX);   E.rad_idx = blob_at<uint16_t>(d, h, BLOB_RAD_IDX);
    E.t_res_id = blob_at<int>(tp, t, BLOB_RES_ID);          E.res_id = blob_at<int>(d, h, BLOB_RES_ID);
    E.t_res_flags = blob_at<uint8_t>(tp, t, BLOB_RES_FLAGS); E.res_flags = blob_at<uint8_t>(d, h, BLOB_RES_FLAGS);
    E.t_res_prev = blob_at<int>(tp, t, BLOB_RES_PREV);      E.res_prev = blob_at<int>(d, h, BLOB_RES_PREV);
    E.t_res_next = blob_at<int>(tp, t, BLOB_RES_NEXT);      E.res_next = blob_at<int>(d, h, BLOB_RES_NEXT);
    E.t_bond_off = blob_at<int>(tp, t, BLOB_BOND_OFF);      E.bond_off = blob_at<int>(d, h, BLOB_BOND_OFF);
    E.t_bond_idx = blob_at<int>(tp, t, BLOB_BOND_IDX);      E.bond_idx = blob_at<int>(d, h, BLOB_BOND_IDX);
    E.t_h_off = blob_at<int>(tp, t, BLOB_H_OFF);            E.h_off = blob_at<int>(d, h, BLOB_H_OFF);
    E.t_sb_nbr = blob_at<int>(tp, t, BLOB_SB_NBR);          E.sb_nbr = blob_at<int>(d, h, BLOB_SB_NBR);
    E.t_am_res = blob_at<int>(tp, t, BLOB_AMIDE_RES);       E.am_res = blob_at<int>(d, h, BLOB_AMIDE_RES);
    E.t_rad_tab = blob_at<double2>(tp, t, BLOB_RAD_TAB);    E.rad_tab = blob_at<double2>(d, h, BLOB_RAD_TAB);
    E.ring_res = blob_at<int>(d, h, BLOB_RING_RES);         // (-1 until k_ring_residue below)
    const int64_t work = std::max({h.n + 1, h.nres, h.nbond, h.nring, h.namide, (int64_t)RAD_TABLE});
    hipLaunchKernelGGL(k_models_expand, dim3(nblocks(work, 256), MODELS_EXPAND_SEGMENTS), dim3(256), 0, c->stream, E);
    const float4* const xyz4 = E.xyz4;
    double* const ring_c = blob_at<double>(d, h, BLOB_RING_C);
    float* const am_c = blob_at<float>(d, h, BLOB_AMIDE_C);
    if (h.nring > 0)
        hipLaunchKernelGGL(k_ring_geometry, dim3(nblocks(h.nring, 256)), dim3(256), 0, c->stream, (int)F, (int)t.n, (int)t.nring,
                           c->topo_ring_off.p, c->topo_ring_idx.p, xyz4, ring_c, blob_at<double>(d, h, BLOB_RING_N));
    if (h.namide > 0)
        hipLaunchKernelGGL(k_amide_geometry, dim3(nblocks(h.namide, 256)), dim3(256), 0, c->stream, (int)F, (int)t.n, (int)t.namide,
                           c->topo_amide_atoms.p, xyz4, am_c, blob_at<float>(d, h, BLOB_AMIDE_N));
    hipLaunchKernelGGL(k_models_boxes, dim3((unsigned)F), dim3(256), 0, c->stream, (int)t.n, (int)t.nring, (int)t.namide, xyz4, ring_c, am_c,
                       c->models_box.p);
    int rc = check_launch(c, "k_models_expand / geometry / boxes");
    if (rc != ARP_OK) return fail(rc);
    std::vector<double> box((size_t)(18 * F));
    e = hipMemcpyAsync(box.data(), c->models_box.p, box.size() * sizeof(double), hipMemcpyDeviceToHost, c->stream);
    if (e == hipSuccess) e = hipStreamSynchronize(c->stream);
    if (e != hipSuccess) { c->err = std::string("arp_set_models: boxes: ") + hipGetErrorString(e); return fail(ARP_E_HIP); }
    // header boxes: the union over the models of atoms / ring centres / amide centres (0 for an empty set, as arp_blob_fill);
    // partition boxes: everything a model holds (as batch.concat_complexes)
    const int64_t cnt[3] = {t.n, t.nring, t.namide};
    double* const hlo[3] = {h.lo, h.ring_lo, h.amide_lo};
    double* const hhi[3] = {h.hi, h.ring_hi, h.amide_hi};
    std::vector<double> pbox((size_t)(6 * F), 0.0);
    bool finite = true, seen[3] = {false, false, false};
    for (int64_t f = 0; f < F; ++f) {
        bool any = false;
        for (int q = 0; q < 3; ++q) {
            if (cnt[q] == 0) continue;
            const double* b = &box[(size_t)(18 * f + 6 * q)];       // lo xyz, hi xyz
            for (int k = 0; k < 6; ++k) finite = finite && std::isfinite(b[k]);
            box_union(hlo[q], hhi[q], seen[q], b, b + 3);
            box_union(&pbox[(size_t)(6 * f)], &pbox[(size_t)(6 * f + 3)], any, b, b + 3);
        }
    }
    if (!finite)   // a model with a non-finite coordinate: the validation below reports it (no atom lies in an empty box)
        for (int q = 0; q < 3; ++q)
            for (int k = 0; k < 3; ++k) hlo[q][k] = hhi[q][k] = 0.0;
    borrow_blob_views(c, h);
    rc = validate_resident_blob(c, h, "arp_set_models", nullptr, /*gather_sb=*/true, /*rad_from_table=*/false, /*batch_next=*/true);
    if (rc != ARP_OK) return rc;      // (abandoned: nothing resident)
    std::vector<int64_t> ao((size_t)F + 1), ro((size_t)F + 1), mo((size_t)F + 1);
    for (int64_t f = 0; f <= F; ++f) { ao[(size_t)f] = f * t.n; ro[(size_t)f] = f * t.nring; mo[(size_t)f] = f * t.namide; }
    rc = arp_set_batch(c, F, ao.data(), ro.data(), mo.data(), pbox.data());
    if (rc != ARP_OK) return fail(rc);
    if (h.nring > 0 && h.n > 0) {     // I:1453-1492 per model, on the all-atom grid of the partition (no atoms: every ring keeps -1)
        rc = build_all_grid(c, 6.0);
        if (rc == ARP_OK) {
            hipLaunchKernelGGL(k_ring_residue, dim3(nblocks(h.nring * 64, 256, 4096)), dim3(256), 0, c->stream, c->all_grid.d,
                               c->all_grid.start.p, c->a_xyzm.p, c->a_aux.p, (int)h.nring, c->ring_c.p, c->all_grid.d.sid_ring, c->ring_res.p,
                               (double*)nullptr);
            rc = check_launch(c, "k_ring_residue");
        }
        if (rc != ARP_OK) return fail(rc);
    }
    c->models_n = F;
    return ARP_OK;
}

int arp_models_planes(arp_ctx* c, double* ring_center, double* ring_normal, int32_t* ring_res, float* amide_center, float* amide_normal) {
    if (!c) return ARP_E_ARG;
    if (c->models_n <= 0) FAIL(c, ARP_E_ARG, "arp_models_planes: no models resident (arp_set_models)");
    const int64_t F = c->models_n, R = c->nring, A = c->namide;
    if ((R > 0 && (!ring_center || !ring_normal || !ring_res)) || (A > 0 && (!amide_center || !amide_normal)))
        FAIL(c, ARP_E_ARG, "arp_models_planes: output missing");
    HIPCHK(c, hipSetDevice(c->device));
    CHK(download_async(c, ring_center, c->ring_c.p, (size_t)(3 * R)));
    CHK(download_async(c, ring_normal, c->ring_n.p, (size_t)(3 * R)));
    CHK(download_async(c, ring_res, c->ring_res.p, (size_t)R));
    CHK(download_async(c, amide_center, c->am_c.p, (size_t)(3 * A)));
    CHK(download_async(c, amide_normal, c->am_n.p, (size_t)(3 * A)));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    const int64_t per = R / F, nres = c->nres / F;     // residues of the resident partition -> of the model
    for (int64_t k = 0; k < R; ++k)
        if (ring_res[k] >= 0) ring_res[k] -= (int32_t)((k / per) * nres);
    return ARP_OK;
}

// ---- the results made on the device from the bags of a pass (DESIGN.md 5e ... 5k) -------------------------------------
// Every launch refuses (check_masks, launch_refusals), returns a result that is already made for its arguments, enqueues, waits
// for a count (wait_count) and enqueues the rest.  A result of sorted records is two parts around that wait: sort_to_runs
// (reserve, re-key, sort by every bit, count the runs, learn U) and reduce_to_rows (layout, slab, run starts, one wave per
// row); table_fetch is one copy of the slab through the page-locked stage.  A table brings a TableSpec and its two own steps.
namespace {
enum { TABLE_MAX_COLS = 14 };
// what a launch needs of the context; refused in this order before a launch looks for its result (launch_refusals)
enum : unsigned { NEED_WHOLE = 1u << 0, NEED_MODELS = 1u << 1, NEED_MODELS_U16 = 1u << 2, NEED_AA_BAG = 1u << 3, NEED_FIVE_BAGS = 1u << 4 };
struct TableSpec {
    const char* name;                // "<name>_launch" / "<name>_fetch" in messages
    ResultTable arp_ctx::* table;
    int cols;
    size_t es[TABLE_MAX_COLS];       // bytes per row of every column, in the order of the fetch's arguments (= of the slab)
    unsigned needs;                  // NEED_*: FIVE_BAGS = made from all five bags of a complete pass; else from the atom-atom bag alone
    const char* no_pass;             // the refusal when those results are missing
    long long min_rows;              // fewest rows that records can give: 0 where a table leaves records out (all of them, then)
    std::string launch() const { return std::string(name) + "_launch: "; }
};
const char* const NO_AA_PASS = "no atom-contact results (call a launch first)";
// the columns of every table in the order of its fetch's arguments
enum { PT_A = 0, PT_B, PT_NMODELS, PT_FIRST, PT_LAST, PT_DMIN, PT_DMAX, PT_DSUM, PT_BITS, PT_CTYPE, PT_COLS };
enum { RT_A = 0, RT_B, RT_N, RT_DMIN, RT_BITS, RT_CTYPE, RT_PLANES, RT_COLS };
enum { ST_A = 0, ST_B, ST_NMODELS, ST_FIRST, ST_LAST, ST_N, ST_CLS, ST_BITS, ST_DMIN, ST_DMAX, ST_DSUM, ST_CTYPE, ST_COLS };
enum { WB_WATER = 0, WB_A, WB_B, WB_DIST_A, WB_DIST_B, WB_SIFT_A, WB_SIFT_B, WB_CTYPE_A, WB_CTYPE_B, WB_COLS };
enum { WP_A = 0, WP_B, WP_NMODELS, WP_FIRST, WP_LAST, WP_NWATERS, WP_NBRIDGES, WP_DMIN, WP_DMAX, WP_DSUM, WP_BITS_A, WP_BITS_B,
       WP_CTYPE_A, WP_CTYPE_B, WP_COLS };
enum { LT_A = 0, LT_B, LT_NMODELS, LT_FIRST, LT_LAST, LT_NINTERVALS, LT_LONGEST, LT_LONGEST_START, LT_HEAD, LT_TAIL, LT_SPAN_SUM, LT_COLS };
enum { NW_ROOT = 0, NW_NNODES, NW_NEDGES, NW_SIFT, NW_CTYPE, NW_COLS };
const unsigned OVER_MODELS = NEED_WHOLE | NEED_MODELS | NEED_MODELS_U16;
const TableSpec PERSIST_TABLE = {"arp_models_persistence", &arp_ctx::persist, PT_COLS, {4, 4, 2, 4, 4, 4, 4, 8, 2 * TABLE_SIFT_BITS, 1},
                                 OVER_MODELS | NEED_AA_BAG, "no results of a pass over the resident models (launch one first)", 1};
const TableSpec RESPAIR_TABLE = {"arp_residue_pairs", &arp_ctx::respair, RT_COLS, {4, 4, 4, 4, 4 * TABLE_SIFT_BITS, 1, 4 * RESPAIR_PLANE_BAGS},
                                 NEED_WHOLE | NEED_FIVE_BAGS, "no results of a complete pass (arp_run_launch first)", 0};
const TableSpec RESPERSIST_TABLE = {"arp_models_residue_persistence", &arp_ctx::respersist, ST_COLS,
                                    {4, 4, 2, 4, 4, 4, 2 * RESPERSIST_CLASSES, 2 * TABLE_SIFT_BITS, 4, 4, 8, 1},
                                    OVER_MODELS | NEED_FIVE_BAGS, "no results of a complete pass over the resident models (arp_run_launch first)", 0};
const TableSpec BRIDGE_TABLE = {"arp_water_bridges", &arp_ctx::bridges, WB_COLS, {4, 4, 4, 4, 4, 2, 2, 1, 1}, NEED_WHOLE | NEED_AA_BAG, NO_AA_PASS, 0};
const TableSpec BRIDGEPERSIST_TABLE = {"arp_models_water_bridge_persistence", &arp_ctx::bridgepersist, WP_COLS,
                                       {4, 4, 2, 4, 4, 4, 4, 4, 4, 8, 2 * TABLE_SIFT_BITS, 2 * TABLE_SIFT_BITS, 1, 1}, OVER_MODELS | NEED_AA_BAG,
                                       "no atom-contact results of a pass over the resident models (call a launch first)", 1};
// (fewest rows 0: the masks of a launch may leave every record out)
const TableSpec LIFETIMES_TABLE = {"arp_models_lifetimes", &arp_ctx::lifetimes, LT_COLS, {4, 4, 2, 4, 4, 2, 2, 4, 2, 2, 4},
                                   OVER_MODELS | NEED_AA_BAG, PERSIST_TABLE.no_pass, 0};
const TableSpec NETWORKS_TABLE = {"arp_networks", &arp_ctx::networks, NW_COLS, {4, 4, 4, 2, 1}, NEED_WHOLE | NEED_AA_BAG, NO_AA_PASS, 0};
// (two tables in one slab: the three columns of the K features, then the three of the P kept pairs — couple_layout; it needs
// the bags of its level, which its launch refuses as similarity does)
enum { CP_A = 0, CP_B, CP_COUNT, CP_U, CP_V, CP_N11, CP_COLS, CP_FEATURE_COLS = CP_U };
const TableSpec COUPLING_TABLE = {"arp_models_coupling", &arp_ctx::coupling, CP_COLS, {4, 4, 4, 4, 4, 4}, NEED_WHOLE | NEED_MODELS, nullptr, 0};
static_assert(COUPLE_BY_RESIDUE == ARP_COUPLE_BY_RESIDUE && COUPLE_MAX_FEATURES == ARP_COUPLE_MAX_FEATURES &&
              COUPLE_MAX_WORDS * 64 == ARP_SIM_MAX_MODELS, "arp_coupling.h names the header's limits");
static_assert(PT_COLS <= TABLE_MAX_COLS && RT_COLS <= TABLE_MAX_COLS && ST_COLS <= TABLE_MAX_COLS && WB_COLS <= TABLE_MAX_COLS &&
              WP_COLS <= TABLE_MAX_COLS && LT_COLS <= TABLE_MAX_COLS, "TableSpec::es");
static_assert(ARP_LIFETIMES_MAX_GAP + 1u <= 0xFFFFu, "gap + 1 is compared with differences of models counted in uint16");
static_assert(NET_BY_RESIDUE == ARP_NET_BY_RESIDUE, "arp_networks.h names the header's bit");
static_assert(BRIDGE_F_WATER == ARP_F_WATER && BRIDGE_SAME_RESIDUE == ARP_WB_SAME_RESIDUE, "arp_bridge.h names the header's bits");
static_assert(BRIDGEPERSIST_BY_RESIDUE == ARP_WBP_BY_RESIDUE && TABLE_SIFT_BITS == ARP_WBP_BITS, "arp_bridgepersist.h names the header's bits");
static_assert(SIM_PLANES == ARP_SIM_PLANES && SIM_BY_RESIDUE == ARP_SIM_BY_RESIDUE && SIM_PLANES == TABLE_SIFT_BITS + RESPERSIST_CLASSES,
              "arp_similarity.h names the header's planes");

// ---- what a launch refuses
bool five_bags_complete(const arp_ctx* c) {
    return !c->pass_pending && c->contacts_valid && c->bags_valid();
}
int launch_refusals(arp_ctx* c, const std::string& fn, unsigned needs, const char* no_pass) {
    if ((needs & NEED_WHOLE) && (c->has_home || c->has_gid || c->shard_resident)) FAIL(c, ARP_E_ARG, fn + "not for a shard of a distributed structure");
    if ((needs & NEED_MODELS) && c->models_n <= 0) FAIL(c, ARP_E_ARG, fn + "no models resident (arp_set_models)");
    if ((needs & NEED_MODELS_U16) && c->models_n > 65535) FAIL(c, ARP_E_ARG, fn + "more than 65 535 models (the table counts models in uint16)");
    if ((needs & NEED_FIVE_BAGS) ? !five_bags_complete(c) : (needs & NEED_AA_BAG) && (c->pass_pending || !c->contacts_valid)) FAIL(c, ARP_E_ARG, fn + no_pass);
    return ARP_OK;
}
// (a left-out record keeps its slot up to the reduction, so every record of the bags counts here, kept or not)
int records_fit(arp_ctx* c, const std::string& fn, size_t k, const char* why = "") {
    if (k >= ((size_t)1 << 31)) FAIL(c, ARP_E_CAPACITY, fn + "2^31 records or more" + why);
    return ARP_OK;
}
// masks {value, every bit there is}: none reaches beyond its bits, then none is 0
int check_masks(arp_ctx* c, const std::string& fn, std::initializer_list<std::pair<uint32_t, uint32_t>> masks, const char* beyond, const char* zero) {
    for (const auto& m : masks) if (m.first & ~m.second) FAIL(c, ARP_E_ARG, fn + beyond);
    for (const auto& m : masks) if (!m.first) FAIL(c, ARP_E_ARG, fn + zero);
    return ARP_OK;
}
int check_leg_mask(arp_ctx* c, const std::string& fn, uint32_t sift_any) {
    return check_masks(c, fn, {{sift_any, ARP_FILTER_SIFT_ALL}}, "sift_any has bits beyond the 15 SIFt bits", "a sift_any of 0 makes no record a leg");
}
// A table is made: its rows, and the arguments of the launch for made_with.
int table_done(ResultTable& T, uint64_t arg0, uint64_t arg1, long long rows, int64_t* count) {
    T.count = rows; T.arg[0] = arg0; T.arg[1] = arg1; T.valid = true;
    ++T.launches;
    *count = rows;
    return ARP_OK;
}

// ---- keys
int index_bits(int64_t count) { return id_bits(std::max<int64_t>(count - 1, 1)); }      // of the ids 0 ... count - 1
// The key of (pair, model): id_a << (bits + fbits) | id_b << fbits | model, the ids atoms of the topology (n of them) or
// residues of a model (nres_t; no residue at all: 1, and every record is left out).
struct PairModelKey {
    int64_t F, n, nres_t;
    int bits, fbits;
    int total() const { return 2 * bits + fbits; }
};
int pair_model_key(arp_ctx* c, const std::string& fn, bool by_residue, const char* what, PairModelKey* G) {
    G->F = c->models_n; G->n = c->topo_hdr.n; G->nres_t = std::max<int64_t>(c->nres / G->F, 1);
    G->bits = index_bits(by_residue ? G->nres_t : G->n); G->fbits = index_bits(G->F);
    if (G->total() > 63) FAIL(c, ARP_E_CAPACITY, fn + what + " does not fit a 63-bit key");
    return ARP_OK;
}

// ---- slabs
// Layout of a table's slab: its columns one after the other, each on a 256-byte boundary (so their order is free).
struct TableLayout {
    size_t off[TABLE_MAX_COLS], bytes;
};
TableLayout table_layout(const TableSpec& spec, size_t U) {
    TableLayout L{};
    for (int q = 0; q < spec.cols; ++q) { L.off[q] = L.bytes; L.bytes += al256(U * spec.es[q]); }
    return L;
}
int table_stage_reserve(arp_ctx* c, size_t bytes) {
    if (c->table_stage && c->table_stage_cap >= bytes) return ARP_OK;
    if (c->table_stage) (void)hipHostFree(c->table_stage);
    c->table_stage = nullptr;
    c->table_stage_cap = 0;
    const size_t want = std::max(bytes + bytes / 4, (size_t)4096);
    HIPCHK(c, hipHostMalloc((void**)&c->table_stage, want, hipHostMallocDefault));
    c->table_stage_cap = want;
    return ARP_OK;
}
// One copy of `bytes` from the device into the page-locked stage, waited for: a fetch's, and the word of wait_count.
int stage_copy(arp_ctx* c, const void* dev, size_t bytes) {
    CHK(table_stage_reserve(c, bytes));
    HIPCHK(c, hipMemcpyAsync(c->table_stage, dev, bytes, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    return ARP_OK;
}

// ---- the wait for one count
// Counts per tile go to table_tiles (reserve_tile_counts, then the caller's kernel), k_runs_scan makes their exclusive prefix
// and their sum in table_total (enqueue_tile_scan), and the host reads one 64-bit word through the stage (wait_count).
int reserve_tile_counts(arp_ctx* c, int T) {
    HIPCHK(c, c->table_tiles.reserve((size_t)T));
    HIPCHK(c, c->table_total.reserve(1));
    return table_stage_reserve(c, 4096);
}
void enqueue_tile_scan(arp_ctx* c, int T) {
    RunArgs R{};
    R.T = T; R.tile_rows = c->table_tiles.p; R.total = c->table_total.p;
    hipLaunchKernelGGL(k_runs_scan, dim3(1), dim3(SORT_THREADS), 0, c->stream, R);
}
int wait_count(arp_ctx* c, const long long* dev, long long* v, const std::string& what) {
    CHK(check_launch(c, what.c_str()));
    CHK(stage_copy(c, dev, sizeof(long long)));
    memcpy(v, c->table_stage, sizeof(*v));
    return ARP_OK;
}
int wait_tile_total(arp_ctx* c, int T, long long* v, const std::string& what) {
    enqueue_tile_scan(c, T);
    return wait_count(c, c->table_total.p, v, what);
}

// ---- sorted records and their runs
// k re-keyed records in s.key[0] / s.val[0], sorted by the low keybits bits of the key — every bit of it: least significant
// digit first, up to SORT_MAX_BITS a pass, stable.  *sorted = the buffer (0 / 1) the last pass wrote.  reserve_key_sort sizes the
// scratch (cap >= k records) before the caller fills buffer 0.
int reserve_key_sort(arp_ctx* c, SortScratch& s, size_t k, size_t cap) {
    for (int q = 0; q < 2; ++q) { HIPCHK(c, s.key[q].reserve(cap)); HIPCHK(c, s.val[q].reserve(cap)); }
    const long long tiles = ((long long)k + SORT_TILE - 1) / SORT_TILE;
    HIPCHK(c, s.table.reserve((size_t)SORT_BINS * (size_t)((tiles + 3) & ~3ll)));
    HIPCHK(c, s.total.reserve(SORT_BINS));
    return ARP_OK;
}
void enqueue_key_sort(arp_ctx* c, SortScratch& s, size_t k, int keybits, int* sorted) {
    const long long tiles = ((long long)k + SORT_TILE - 1) / SORT_TILE;
    const int passes = (keybits + SORT_MAX_BITS - 1) / SORT_MAX_BITS;
    SortArgs S{};
    S.n = (long long)k; S.T = (int)tiles; S.tstride = (int)((tiles + 3) & ~3ll); S.table = s.table.p; S.total = s.total.p;
    S.first = 0; S.last = 0; S.jbits = 0;
    int shift = 0;
    for (int ps = 0; ps < passes; ++ps) {
        S.shift = shift;
        S.bits = keybits / passes + (ps < keybits % passes ? 1 : 0);
        shift += S.bits;
        S.key_in = s.key[ps & 1].p; S.val_in = s.val[ps & 1].p;
        S.key_out = s.key[(ps + 1) & 1].p; S.val_out = s.val[(ps + 1) & 1].p;
        hipLaunchKernelGGL(k_sort_hist, dim3(S.T), dim3(SORT_THREADS), 0, c->stream, S);
        hipLaunchKernelGGL(k_sort_scan, dim3(1 << S.bits), dim3(SORT_THREADS), 0, c->stream, S);
        hipLaunchKernelGGL(k_sort_scatter, dim3(S.T), dim3(SORT_THREADS), 0, c->stream, S);
    }
    *sorted = passes & 1;
}
// The runs of equal key >> R.shift among the sorted keys, counted per tile and scanned on the stream: their number stays in
// table_total.  R.key, R.k and R.shift are the caller's, and so is the room for R.T tile counts (reserve_tile_counts).
void enqueue_run_count(arp_ctx* c, RunArgs& R) {
    R.T = (int)((R.k + RUNS_TILE - 1) / RUNS_TILE);
    R.tile_rows = c->table_tiles.p;
    R.total = c->table_total.p;
    hipLaunchKernelGGL(k_runs_count, dim3(R.T), dim3(RUNS_THREADS), 0, c->stream, R);
    enqueue_tile_scan(c, R.T);
}
// ... and where each of the U runs begins (row_start[U] = k), for the reduction that follows on the stream
int enqueue_run_starts(arp_ctx* c, RunArgs& R, long long U) {
    HIPCHK(c, c->table_rows.reserve((size_t)U + 1));
    R.U = U;
    R.row_start = c->table_rows.p;
    hipLaunchKernelGGL(k_runs_starts, dim3(R.T), dim3(RUNS_THREADS), 0, c->stream, R);
    return ARP_OK;
}
// What a re-key step tells the sequence: the bits of the key the sort covers, and a run = equal key >> shift.
struct TableKey {
    int bits, shift;
};
// Records sorted by their key and the U runs among them: what sort_to_runs leaves for the step that reduces them.
struct SortedRuns {
    const unsigned long long *key, *val;
    RunArgs R;
    long long U;
};
// rekey(key, val, &K) enqueues the keys and payloads of the k records into key / val and fills K; reduce(S, col) enqueues the
// reduction of the sorted records S into the S.U rows of the columns col[0 ... spec.cols).
using RekeyStep = std::function<int(unsigned long long* key, unsigned long long* val, TableKey* K)>;
using ReduceStep = std::function<void(const SortedRuns& S, const Columns& col)>;
// The first part: k > 0 records (the scratch sized for cap >= k) re-keyed, sorted by every bit of the key, their runs counted;
// the host learns U (the one wait), which lies in [min_rows, k].
int sort_to_runs(arp_ctx* c, const std::string& fn, size_t k, size_t cap, long long min_rows, const RekeyStep& rekey, SortedRuns* S) {
    SortScratch& s = c->table_sort;
    CHK(reserve_key_sort(c, s, k, cap));
    TableKey K{};
    CHK(rekey(s.key[0].p, s.val[0].p, &K));
    int sorted = 0;
    enqueue_key_sort(c, s, k, K.bits, &sorted);
    *S = SortedRuns{s.key[sorted].p, s.val[sorted].p, RunArgs{}, 0};
    RunArgs& R = S->R;
    R.key = S->key; R.k = (long long)k; R.shift = K.shift;
    CHK(reserve_tile_counts(c, (int)((R.k + RUNS_TILE - 1) / RUNS_TILE)));
    enqueue_run_count(c, R);
    CHK(wait_count(c, c->table_total.p, &S->U, fn + "sort / count"));
    if (S->U < min_rows || S->U > (long long)k) FAIL(c, ARP_E_HIP, fn + "row count out of range");
    return ARP_OK;
}
// The second part: the slab of S.U > 0 rows, where each run begins, and the table's reduction, one wave per row.
int reduce_to_rows(arp_ctx* c, const TableSpec& spec, SortedRuns& S, const ReduceStep& reduce) {
    ResultTable& T = c->*spec.table;
    const TableLayout L = table_layout(spec, (size_t)S.U);
    HIPCHK(c, T.slab.reserve(L.bytes));
    CHK(enqueue_run_starts(c, S.R, S.U));
    reduce(S, Columns{T.slab.p, L.off});
    return check_launch(c, (spec.launch() + "reduce").c_str());
}
// Both parts: the table of k > 0 records, made with (arg0, arg1).
int table_from_records(arp_ctx* c, const TableSpec& spec, uint32_t arg0, uint32_t arg1, size_t k, size_t cap, int64_t* count,
                       const RekeyStep& rekey, const ReduceStep& reduce) {
    SortedRuns S{};
    CHK(sort_to_runs(c, spec.launch(), k, cap, spec.min_rows, rekey, &S));
    if (S.U > 0) CHK(reduce_to_rows(c, spec, S, reduce));
    return table_done(c->*spec.table, arg0, arg1, S.U, count);
}

// ---- the bags as records
// What a table reads of a pass: the atom-atom bag and — planes: a residue table — the four ring / amide bags as the re-key
// kernels walk them, placed behind the atom-atom records; the records of all those bags (k), of the four (planes) and of the
// largest of the four; and the capacity the sort scratch is sized from — the capacities of the bags' columns, so that it is
// allocated once per structure size.
struct FiveBags {
    RespairBag bag[RESPAIR_PLANE_BAGS];      // classes 1 ... 4
    size_t k, planes, cap;
    int64_t largest;
};
FiveBags five_bags(const arp_ctx* c, bool planes) {
    static_assert(RESPAIR_PLANE_BAGS == BAG_KINDS, "arp_respair.h");
    const int* const res_of[3] = {c->res_id.p, c->ring_res.p, c->am_res.p};      // by ENT_ATOM, ENT_RING, ENT_AMIDE
    FiveBags B{};
    B.k = (size_t)c->n_contacts;
    B.cap = std::max((size_t)c->n_contacts, c->out_i.cap);
    for (int m = 0; planes && m < RESPAIR_PLANE_BAGS; ++m) {
        const Bag& b = c->bag[m];
        B.bag[m] = RespairBag{b.id(0), b.id(1), res_of[PLANE_TABLES[m].entity[0]], res_of[PLANE_TABLES[m].entity[1]], (long long)b.count, (long long)B.k};
        B.k += (size_t)b.count;
        B.planes += (size_t)b.count;
        B.cap += std::max((size_t)b.count, b.cap);
        B.largest = std::max(B.largest, b.count);
    }
    return B;
}
// A table made from the bags: refuse, return the table that is made for the same launch arguments (arg0, arg1: 0 for a launch
// without), then table_from_records with rekey(B, ...) over the bags B the spec names.
using BagsRekeyStep = std::function<int(const FiveBags& B, unsigned long long* key, unsigned long long* val, TableKey* K)>;
int make_table(arp_ctx* c, const TableSpec& spec, int64_t* count, const BagsRekeyStep& rekey, const ReduceStep& reduce,
               uint32_t arg0 = 0, uint32_t arg1 = 0) {
    if (!c || !count) return ARP_E_ARG;
    const std::string fn = spec.launch();
    CHK(launch_refusals(c, fn, spec.needs, spec.no_pass));
    ResultTable& T = c->*spec.table;
    if (T.made_with(arg0, arg1)) { *count = T.count; return ARP_OK; }
    HIPCHK(c, hipSetDevice(c->device));
    const FiveBags B = five_bags(c, (spec.needs & NEED_FIVE_BAGS) != 0);
    T.valid = false;
    T.count = 0;
    if (B.k == 0) return table_done(T, arg0, arg1, 0, count);
    CHK(records_fit(c, fn, B.k));
    return table_from_records(c, spec, arg0, arg1, B.k, B.cap, count,
                              [&](unsigned long long* key, unsigned long long* val, TableKey* K) { return rekey(B, key, val, K); }, reduce);
}
// One copy of the slab into the page-locked stage; column q goes to dst[q] unless that is NULL.
int table_fetch(arp_ctx* c, const TableSpec& spec, int64_t cap, void* const dst[], int64_t* count) {
    if (!c || !count) return ARP_E_ARG;
    const std::string name = spec.name;
    const ResultTable& T = c->*spec.table;
    if (!c->contacts_valid || !T.valid) FAIL(c, ARP_E_ARG, name + "_fetch: no table (" + name + "_launch after a pass)");
    *count = T.count;
    if (T.count > cap) FAIL(c, ARP_E_CAPACITY, name + "_fetch: output buffers too small");
    const size_t U = (size_t)T.count;
    if (U == 0) return ARP_OK;
    HIPCHK(c, hipSetDevice(c->device));
    const TableLayout L = table_layout(spec, U);
    CHK(stage_copy(c, T.slab.p, L.bytes));
    for (int q = 0; q < spec.cols; ++q)
        if (dst[q]) memcpy(dst[q], c->table_stage + L.off[q], U * spec.es[q]);
    return ARP_OK;
}

// ---- the re-key steps
// The atom-atom bag keyed by topology atom pair and model (the persistence table's rows); returns what it launched with, for
// the reduction of that table.
PersistArgs enqueue_persist_rekey(arp_ctx* c, const PairModelKey& G, size_t k, unsigned long long* key, unsigned long long* val, TableKey* K) {
    PersistArgs A{};
    A.ci = c->out_i.p; A.cj = c->out_j.p; A.d_in = c->out_d.p; A.s_in = c->out_s.p; A.ct_in = c->out_ct.p;
    A.k = (long long)k;
    A.n = (uint32_t)G.n;      // (> 0: the bag has records)
    A.bbits = G.bits; A.fbits = G.fbits;
    A.key = key; A.val = val;
    *K = TableKey{G.total(), G.fbits};
    hipLaunchKernelGGL(k_persist_rekey, dim3(nblocks((int64_t)k, 256, 2048)), dim3(256), 0, c->stream, A);
    return A;
}
// The five bags keyed by topology residue pair and model (the rows of both residue tables; the residue-pair table has no model
// in its key: G.fbits = 0, G.F = 1).  The sort covers res_a << (bits + fbits) | res_b << fbits | f, and one bit more where the
// all-ones key of a left-out record would otherwise tie with a real record in the sorted bits — the pair (nres_t - 1,
// nres_t - 1) of a ring / amide bag in model F - 1, when nres_t - 1 and F - 1 are all ones themselves (bit 2 bits + fbits is
// set in ~0 and in no record: the left-out records then sort last by it).
void enqueue_residue_rekey(arp_ctx* c, const FiveBags& B, const PairModelKey& G, unsigned long long* key, unsigned long long* val, TableKey* K) {
    const bool tie = B.planes > 0 && G.nres_t - 1 == ((int64_t)1 << G.bits) - 1 && G.F - 1 == ((int64_t)1 << G.fbits) - 1;
    *K = TableKey{G.total() + (tie ? 1 : 0), G.fbits};
    RekeyArgs A{};
    A.ci = c->out_i.p; A.cj = c->out_j.p; A.d_in = c->out_d.p; A.s_in = c->out_s.p; A.ct_in = c->out_ct.p;
    A.res_id = c->res_id.p;
    A.k_aa = (long long)c->n_contacts;
    for (int m = 0; m < RESPAIR_PLANE_BAGS; ++m) A.bag[m] = B.bag[m];
    A.nres_t = (uint32_t)G.nres_t; A.rbits = G.bits; A.fbits = G.fbits;
    A.key = key; A.val = val;
    if (A.k_aa > 0) hipLaunchKernelGGL(k_residue_rekey, dim3(nblocks((int64_t)A.k_aa, 256, 2048)), dim3(256), 0, c->stream, A);
    if (B.planes > 0) hipLaunchKernelGGL(k_residue_rekey_planes, dim3(nblocks(B.largest, 256, 512), RESPAIR_PLANE_BAGS), dim3(256), 0, c->stream, A);
}
}  // namespace

// ---- contact persistence over the resident models (arp_persist.h)
int arp_models_persistence_launch(arp_ctx* c, int64_t* count) {
    PersistArgs A{};
    return make_table(c, PERSIST_TABLE, count,
        [&](const FiveBags& B, unsigned long long* key, unsigned long long* val, TableKey* K) -> int {
            PairModelKey G{};
            CHK(pair_model_key(c, PERSIST_TABLE.launch(), false, "(atom, atom, model)", &G));
            A = enqueue_persist_rekey(c, G, B.k, key, val, K);
            return ARP_OK;
        },
        [&](const SortedRuns& S, const Columns& col) {
            A.key = (unsigned long long*)S.key; A.val = (unsigned long long*)S.val; A.row_start = S.R.row_start; A.U = S.U;
            A.t_a = col[PT_A]; A.t_b = col[PT_B]; A.t_nmodels = col[PT_NMODELS]; A.t_first = col[PT_FIRST]; A.t_last = col[PT_LAST];
            A.t_dmin = col[PT_DMIN]; A.t_dmax = col[PT_DMAX]; A.t_dsum = col[PT_DSUM]; A.t_bits = col[PT_BITS]; A.t_ctype = col[PT_CTYPE];
            hipLaunchKernelGGL(k_persist_reduce, dim3(nblocks(S.U, 4, 16384)), dim3(256), 0, c->stream, A);
        });
}

int arp_models_persistence_fetch(arp_ctx* c, int64_t cap, int32_t* a, int32_t* b, uint16_t* n_models, int32_t* first, int32_t* last,
                                 float* dist_min, float* dist_max, double* dist_sum, uint16_t* bit_count, uint8_t* ctype_mask, int64_t* count) {
    void* const dst[PT_COLS] = {a, b, n_models, first, last, dist_min, dist_max, dist_sum, bit_count, ctype_mask};
    return table_fetch(c, PERSIST_TABLE, cap, dst, count);
}

// ---- residue-residue contact table of the last pass (arp_respair.h): no model in the key, every resident residue one "model"
int arp_residue_pairs_launch(arp_ctx* c, int64_t* count) {
    PairModelKey G{};
    return make_table(c, RESPAIR_TABLE, count,
        [&](const FiveBags& B, unsigned long long* key, unsigned long long* val, TableKey* K) -> int {
            G = PairModelKey{1, c->n, std::max<int64_t>(c->nres, 1), index_bits(c->nres), 0};
            enqueue_residue_rekey(c, B, G, key, val, K);
            return ARP_OK;
        },
        [&](const SortedRuns& S, const Columns& col) {
            const RespairArgs A{G.bits, S.key, S.val, S.R.row_start, S.U, col[RT_A], col[RT_B], col[RT_N], col[RT_DMIN],
                                col[RT_BITS], col[RT_CTYPE], col[RT_PLANES]};
            hipLaunchKernelGGL(k_respair_reduce, dim3(nblocks(S.U, 4, 16384)), dim3(256), 0, c->stream, A);
        });
}

int arp_residue_pairs_fetch(arp_ctx* c, int64_t cap, int32_t* res_a, int32_t* res_b, uint32_t* n_contacts, float* dist_min,
                            uint32_t* bit_count, uint8_t* ctype_mask, uint32_t* plane_count, int64_t* count) {
    void* const dst[RT_COLS] = {res_a, res_b, n_contacts, dist_min, bit_count, ctype_mask, plane_count};
    return table_fetch(c, RESPAIR_TABLE, cap, dst, count);
}

// ---- residue contact persistence over the resident models (arp_respersist.h)
int arp_models_residue_persistence_launch(arp_ctx* c, int64_t* count) {
    PairModelKey G{};
    return make_table(c, RESPERSIST_TABLE, count,
        [&](const FiveBags& B, unsigned long long* key, unsigned long long* val, TableKey* K) -> int {
            CHK(pair_model_key(c, RESPERSIST_TABLE.launch(), true, "(residue, residue, model)", &G));
            enqueue_residue_rekey(c, B, G, key, val, K);
            return ARP_OK;
        },
        [&](const SortedRuns& S, const Columns& col) {
            RespersistArgs A{};
            A.rbits = G.bits; A.fbits = G.fbits; A.key = S.key; A.val = S.val; A.row_start = S.R.row_start; A.U = S.U;
            A.t_a = col[ST_A]; A.t_b = col[ST_B]; A.t_nmodels = col[ST_NMODELS]; A.t_first = col[ST_FIRST]; A.t_last = col[ST_LAST];
            A.t_n = col[ST_N]; A.t_cls = col[ST_CLS]; A.t_bits = col[ST_BITS]; A.t_dmin = col[ST_DMIN]; A.t_dmax = col[ST_DMAX];
            A.t_dsum = col[ST_DSUM]; A.t_ctype = col[ST_CTYPE];
            hipLaunchKernelGGL(k_respersist_reduce, dim3(nblocks(S.U, 4, 16384)), dim3(256), 0, c->stream, A);
        });
}

int arp_models_residue_persistence_fetch(arp_ctx* c, int64_t cap, int32_t* res_a, int32_t* res_b, uint16_t* n_models, int32_t* first,
                                         int32_t* last, uint32_t* n_contacts, uint16_t* class_models, uint16_t* bit_models,
                                         float* dist_min, float* dist_max, double* dist_sum, uint8_t* ctype_mask, int64_t* count) {
    void* const dst[ST_COLS] = {res_a, res_b, n_models, first, last, n_contacts, class_models, bit_models, dist_min, dist_max, dist_sum, ctype_mask};
    return table_fetch(c, RESPERSIST_TABLE, cap, dst, count);
}

// ---- the atom-atom records a caller asks for (arp_filter.h): filter the bag of the pass, sort the kept records alone
// Kept records per tile, ONE wait for k', then the kept records into columns of their own and their canonical order
// (radix_sort, as sort_contacts runs it) into the filtered slab.  sorted_slab, contacts_sorted and sorted_is_csr are not
// touched: an unfiltered fetch returns what it returned.
int arp_contacts_filter_launch(arp_ctx* c, uint32_t sift_any, uint32_t ctype_mask, int64_t* kept) {
    if (!c || !kept) return ARP_E_ARG;
    const std::string fn = "arp_contacts_filter_launch: ";
    CHK(check_masks(c, fn, {{sift_any, ARP_FILTER_SIFT_ALL}, {ctype_mask, ARP_FILTER_CTYPE_ALL}},
                    "a mask has bits beyond the 15 SIFt bits / the 7 contact types", "a mask of 0 keeps nothing"));
    CHK(launch_refusals(c, fn, NEED_WHOLE | NEED_AA_BAG, NO_AA_PASS));
    FilteredBag& F = c->filtered;
    const bool csr = c->packed_csr;
    if (F.valid && F.sift_any == sift_any && F.ctype_mask == ctype_mask && F.csr == csr) { *kept = F.count; return ARP_OK; }
    HIPCHK(c, hipSetDevice(c->device));
    F.valid = false;
    const size_t k = (size_t)c->n_contacts;
    CHK(records_fit(c, fn, k, " (the digit table's prefixes are 32-bit)"));
    const size_t rows = (size_t)std::max<int64_t>(c->n, 0);
    // ---- kept records per tile, scanned; the host learns k' (the one wait)
    FilterArgs A{};
    A.ci = c->out_i.p; A.cj = c->out_j.p; A.d_in = c->out_d.p; A.s_in = c->out_s.p; A.ct_in = c->out_ct.p;
    A.k = (long long)k; A.sift_any = sift_any; A.ctype_mask = ctype_mask;
    const int T = (int)((k + FILTER_TILE - 1) / FILTER_TILE);
    long long kp = 0;
    if (k > 0) {
        CHK(reserve_tile_counts(c, T));
        A.tile_keep = c->table_tiles.p;
        hipLaunchKernelGGL(k_filter_count, dim3(T), dim3(FILTER_THREADS), 0, c->stream, A);
        CHK(wait_tile_total(c, T, &kp, fn + "count / scan"));
        if (kp < 0 || kp > (long long)k) FAIL(c, ARP_E_HIP, fn + "kept count out of range");
    }
    // ---- the slab of the sorted result, with room for the ring / amide bags arp_fetch_packed_filtered packs behind it
    const PackedAtomBag S{"arp_contacts_filter_launch", (int64_t)kp, csr, &F};
    PackedPlan P;
    int64_t counts[5];
    uint64_t offsets[ARP_PACKED_OFFSETS];
    CHK(packed_plan(c, S, P, counts, offsets));
    HIPCHK(c, F.slab.reserve(std::max(P.total, (size_t)16)));
    F.count = kp; F.sift_any = sift_any; F.ctype_mask = ctype_mask; F.csr = csr;
    if (kp == 0) {      // (0 records, no launch: the row column is all zeros, as sort_contacts leaves it for k = 0)
        if (csr) HIPCHK(c, hipMemsetAsync(F.slab.p + P.off[0], 0, (rows + 1) * sizeof(int32_t), c->stream));
        F.valid = true;
        *kept = 0;
        return ARP_OK;
    }
    // ---- the kept records, in the order the bag holds them: five columns sized for exactly k'
    size_t coff[5], cbytes;
    sorted_layout((size_t)kp, coff, &cbytes, (size_t)kp);
    HIPCHK(c, F.cols.reserve(cbytes));
    const Columns in{F.cols.p, coff}, out{F.slab.p, P.off};
    A.i_out = in[0]; A.j_out = in[1]; A.d_out = in[2]; A.s_out = in[3]; A.ct_out = in[4];
    A.kept = kp;
    hipLaunchKernelGGL(k_filter_write, dim3(T), dim3(FILTER_THREADS), 0, c->stream, A);
    CHK(check_launch(c, "k_filter_write"));
    // ---- their canonical order (the sort of sort_contacts, over k' records)
    const int64_t idmax = std::max<int64_t>(c->n - 1, 1);
    SortArgs Q{};
    Q.ci = A.i_out; Q.cj = A.j_out; Q.d_in = A.d_out; Q.s_in = A.s_out; Q.ct_in = A.ct_out;
    Q.i_out = out[0]; Q.j_out = out[1]; Q.d_out = out[2]; Q.s_out = out[3]; Q.ct_out = out[4];
    Q.row_out = csr ? Q.i_out : nullptr;
    Q.nrows = (int)rows;
    const bool small = sw().sort_small && (size_t)kp <= (size_t)SORT_SMALL_MAX_RECORDS && idmax + 1 <= (int64_t)SORT_SMALL_MAX_BINS;
    CHK(radix_sort(c, c->sort_aa, Q, (size_t)kp, std::max(k, c->out_i.cap), id_bits(idmax), small ? (int)idmax + 1 : 0, "arp_contacts_filter_launch"));
    F.valid = true;
    *kept = kp;
    return ARP_OK;
}

int arp_fetch_packed_filtered(arp_ctx* c, void* host, uint64_t host_bytes, int64_t counts[5], uint64_t offsets[ARP_PACKED_OFFSETS], uint64_t* bytes_used) {
    if (!c || !counts || !offsets || !bytes_used) return ARP_E_ARG;
    FilteredBag& F = c->filtered;
    if (!c->contacts_valid || !F.valid || F.csr != c->packed_csr) FAIL(c, ARP_E_ARG, "arp_fetch_packed_filtered: no filtered result (arp_contacts_filter_launch after a pass)");
    HIPCHK(c, hipSetDevice(c->device));
    return fetch_packed_from(c, PackedAtomBag{"arp_fetch_packed_filtered", F.count, F.csr, &F}, host, host_bytes, counts, offsets, bytes_used);
}

// What both joins on waters share (arp_water_bridges_launch, arp_library_water_bridges_launch): the legs of the resident atom-atom
// bag (k > 0 records) counted per tile and scanned — the host learns L, one wait —, keyed by (water, partner) into the scratch `s`,
// sorted by every bit so that a water's legs become one run with ascending partners, the runs counted and their starts made for L
// runs (the most there can be): U stays on the device, in table_total.  L = 0: nothing more was enqueued.
struct SortedLegs {
    BridgeLegArgs A;
    RunArgs R;
    const unsigned long long *key, *val;      // the sorted legs
    long long L;
};
int sorted_water_legs(arp_ctx* c, const std::string& fn, uint32_t sift_any, SortScratch& s, SortedLegs* S) {
    const size_t k = (size_t)c->n_contacts;
    BridgeLegArgs& A = S->A;
    A = BridgeLegArgs{};
    A.ci = c->out_i.p; A.cj = c->out_j.p; A.d_in = c->out_d.p; A.s_in = c->out_s.p; A.ct_in = c->out_ct.p;
    A.k = (long long)k; A.flags = c->flags.p; A.sift_any = sift_any;
    A.pbits = index_bits(c->n);      // (key = w << pbits | partner: at most 62 bits)
    const int tiles = (int)((k + FILTER_TILE - 1) / FILTER_TILE);
    CHK(reserve_tile_counts(c, tiles));
    A.tile_keep = c->table_tiles.p;
    hipLaunchKernelGGL(k_bridge_legs_count, dim3(tiles), dim3(FILTER_THREADS), 0, c->stream, A);
    long long L = 0;
    CHK(wait_tile_total(c, tiles, &L, fn + "legs count / scan"));
    if (L < 0 || L > (long long)k) FAIL(c, ARP_E_HIP, fn + "leg count out of range");
    S->L = L;
    if (L == 0) return ARP_OK;
    CHK(reserve_key_sort(c, s, (size_t)L, (size_t)L));
    A.key = s.key[0].p; A.val = s.val[0].p; A.legs = L;
    hipLaunchKernelGGL(k_bridge_legs_write, dim3(tiles), dim3(FILTER_THREADS), 0, c->stream, A);
    int sorted = 0;
    enqueue_key_sort(c, s, (size_t)L, 2 * A.pbits, &sorted);
    S->key = s.key[sorted].p; S->val = s.val[sorted].p;
    RunArgs& R = S->R;
    R = RunArgs{};
    R.key = S->key; R.k = L; R.shift = A.pbits;
    enqueue_run_count(c, R);      // (R.T <= tiles: table_tiles is large enough, and the legs' prefixes are consumed in stream order)
    return enqueue_run_starts(c, R, L);
}

// ---- water-mediated contacts (arp_bridge.h): the atom-atom bag joined with itself on its water atoms
// Two waits — L legs, then B rows —: a shape of its own, from the shared steps.  U, the waters with a leg, is never read by the
// host: row_start is made for L runs (the most there can be) and the kernels take U from table_total.  Of the results only the
// atom-atom bag is read, and this table alone is written; remaking it voids what is made from it (void_results).
int arp_water_bridges_launch(arp_ctx* c, uint32_t sift_any, uint32_t flags, int64_t* count) {
    if (!c || !count) return ARP_E_ARG;
    const TableSpec& spec = BRIDGE_TABLE;
    const std::string fn = spec.launch();
    CHK(check_leg_mask(c, fn, sift_any));
    if (flags & ~ARP_WB_SAME_RESIDUE) FAIL(c, ARP_E_ARG, fn + "unknown flag");
    CHK(launch_refusals(c, fn, spec.needs, spec.no_pass));
    ResultTable& T = c->bridges;
    if (T.made_with(sift_any, flags)) { *count = T.count; return ARP_OK; }
    HIPCHK(c, hipSetDevice(c->device));
    T.valid = false;
    T.count = 0;
    void_results(c, RES_BRIDGES);
    const size_t k = (size_t)c->n_contacts;
    CHK(records_fit(c, fn, k));
    const auto done = [&](long long rows) { return table_done(T, sift_any, flags, rows, count); };
    if (k == 0) return done(0);
    // ---- the legs, sorted by (water, partner), and their runs; the host learns L (wait 1)
    SortedLegs S{};
    CHK(sorted_water_legs(c, fn, sift_any, c->table_sort, &S));
    const long long L = S.L;
    if (L == 0) return done(0);
    const BridgeLegArgs& A = S.A;
    const RunArgs& R = S.R;
    // ---- kept pairs per run, scanned in 64 bits; the host learns B (wait 2)
    HIPCHK(c, c->bridge_off.reserve((size_t)L + 1));
    HIPCHK(c, c->bridge_res.reserve((size_t)L));
    BridgePairArgs P{};
    P.key = S.key; P.val = S.val; P.legs = L; P.pbits = A.pbits;
    P.row_start = R.row_start; P.runs = c->table_total.p; P.res_id = c->res_id.p; P.leg_res = c->bridge_res.p;
    P.flags = flags; P.row_off = c->bridge_off.p;
    const int pair_blocks = nblocks(L, 4, 16384);       // (one wave per run; U <= L)
    if (!(flags & ARP_WB_SAME_RESIDUE)) hipLaunchKernelGGL(k_bridge_leg_res, dim3(nblocks(L, 256, 2048)), dim3(256), 0, c->stream, P);
    hipLaunchKernelGGL(k_bridge_pairs<false>, dim3(pair_blocks), dim3(256), 0, c->stream, P);
    hipLaunchKernelGGL(k_bridge_scan, dim3(1), dim3(SORT_THREADS), 0, c->stream, P);
    long long B = 0;
    CHK(wait_count(c, c->bridge_off.p + L, &B, fn + "sort / pairs count"));
    if (B < 0) FAIL(c, ARP_E_HIP, fn + "row count out of range");
    if (B >= (1ll << 31)) { *count = B; FAIL(c, ARP_E_CAPACITY, fn + "2^31 rows or more"); }
    if (B == 0) return done(0);
    // ---- the rows, each at its rank
    const TableLayout lay = table_layout(spec, (size_t)B);
    HIPCHK(c, T.slab.reserve(lay.bytes));
    const Columns col{T.slab.p, lay.off};
    P.rows = B;
    P.t_w = col[WB_WATER]; P.t_a = col[WB_A]; P.t_b = col[WB_B]; P.t_da = col[WB_DIST_A]; P.t_db = col[WB_DIST_B];
    P.t_sa = col[WB_SIFT_A]; P.t_sb = col[WB_SIFT_B]; P.t_ca = col[WB_CTYPE_A]; P.t_cb = col[WB_CTYPE_B];
    hipLaunchKernelGGL(k_bridge_pairs<true>, dim3(pair_blocks), dim3(256), 0, c->stream, P);
    CHK(check_launch(c, (fn + "pairs write").c_str()));
    return done(B);
}

int arp_water_bridges_fetch(arp_ctx* c, int64_t cap, int32_t* water, int32_t* a, int32_t* b, float* dist_a, float* dist_b,
                            uint16_t* sift_a, uint16_t* sift_b, uint8_t* ctype_a, uint8_t* ctype_b, int64_t* count) {
    void* const dst[WB_COLS] = {water, a, b, dist_a, dist_b, sift_a, sift_b, ctype_a, ctype_b};
    return table_fetch(c, BRIDGE_TABLE, cap, dst, count);
}

// ---- water-bridge persistence over the resident models (arp_bridgepersist.h): the bridge table folded per pair
// A table whose records are the rows of the bridge table: the bridge launch's waits (none when that table is resident) and
// U.  Only the bridge table is read; nothing but this table and the shared scratch is written.
int arp_models_water_bridge_persistence_launch(arp_ctx* c, uint32_t sift_any, uint32_t flags, int64_t* count) {
    if (!c || !count) return ARP_E_ARG;
    const TableSpec& spec = BRIDGEPERSIST_TABLE;
    const std::string fn = spec.launch();
    CHK(check_leg_mask(c, fn, sift_any));
    if (flags & ~(ARP_WB_SAME_RESIDUE | ARP_WBP_BY_RESIDUE)) FAIL(c, ARP_E_ARG, fn + "unknown flag");
    CHK(launch_refusals(c, fn, spec.needs, spec.no_pass));
    const uint32_t wb_flags = flags & ARP_WB_SAME_RESIDUE;
    ResultTable& T = c->bridgepersist;
    if (T.made_with(sift_any, flags) && c->bridges.made_with(sift_any, wb_flags)) { *count = T.count; return ARP_OK; }
    PairModelKey G{};
    CHK(pair_model_key(c, fn, (flags & ARP_WBP_BY_RESIDUE) != 0, "(pair, model)", &G));
    // ---- the bridge table: made here unless the same one is resident; its own refusals and errors pass through
    T.valid = false;
    T.count = 0;
    int64_t B = 0;
    const int rc = arp_water_bridges_launch(c, sift_any, wb_flags, &B);
    if (rc != ARP_OK) { *count = B; return rc; }
    if (B == 0 || G.n <= 0) return table_done(T, sift_any, flags, 0, count);
    HIPCHK(c, hipSetDevice(c->device));
    BridgepersistArgs A{};
    return table_from_records(c, spec, sift_any, flags, (size_t)B, (size_t)B, count,
        [&](unsigned long long* key, unsigned long long* val, TableKey* K) -> int {      // its rows keyed by (pair, model)
            const TableLayout lay = table_layout(BRIDGE_TABLE, (size_t)B);
            const Columns b{c->bridges.slab.p, lay.off};
            A.bits = G.bits; A.fbits = G.fbits; A.n = (uint32_t)G.n; A.nres_t = (uint32_t)G.nres_t; A.flags = flags;
            A.b_w = b[WB_WATER]; A.b_a = b[WB_A]; A.b_b = b[WB_B]; A.b_da = b[WB_DIST_A]; A.b_db = b[WB_DIST_B];
            A.b_sa = b[WB_SIFT_A]; A.b_sb = b[WB_SIFT_B]; A.b_ca = b[WB_CTYPE_A]; A.b_cb = b[WB_CTYPE_B];
            A.rows = B; A.res_id = c->res_id.p;
            A.key = key; A.val = val;
            *K = TableKey{G.total(), G.fbits};
            hipLaunchKernelGGL(k_bridgepersist_rekey, dim3(nblocks(B, 256, 2048)), dim3(256), 0, c->stream, A);
            return ARP_OK;
        },
        [&](const SortedRuns& S, const Columns& col) {
            A.key = (unsigned long long*)S.key; A.val = (unsigned long long*)S.val; A.row_start = S.R.row_start; A.U = S.U;
            A.t_a = col[WP_A]; A.t_b = col[WP_B]; A.t_nmodels = col[WP_NMODELS]; A.t_first = col[WP_FIRST]; A.t_last = col[WP_LAST];
            A.t_nwaters = col[WP_NWATERS]; A.t_nbridges = col[WP_NBRIDGES]; A.t_dmin = col[WP_DMIN]; A.t_dmax = col[WP_DMAX];
            A.t_dsum = col[WP_DSUM]; A.t_bits_a = col[WP_BITS_A]; A.t_bits_b = col[WP_BITS_B]; A.t_ctype_a = col[WP_CTYPE_A];
            A.t_ctype_b = col[WP_CTYPE_B];
            hipLaunchKernelGGL(k_bridgepersist_reduce, dim3(nblocks(S.U, 4, 16384)), dim3(256), 0, c->stream, A);
        });
}

int arp_models_water_bridge_persistence_fetch(arp_ctx* c, int64_t cap, int32_t* a, int32_t* b, uint16_t* n_models, int32_t* first, int32_t* last,
                                              uint32_t* n_waters, uint32_t* n_bridges, float* dist_min, float* dist_max, double* dist_sum,
                                              uint16_t* bit_models_a, uint16_t* bit_models_b, uint8_t* ctype_mask_a, uint8_t* ctype_mask_b,
                                              int64_t* count) {
    void* const dst[WP_COLS] = {a, b, n_models, first, last, n_waters, n_bridges, dist_min, dist_max, dist_sum,
                                bit_models_a, bit_models_b, ctype_mask_a, ctype_mask_b};
    return table_fetch(c, BRIDGEPERSIST_TABLE, cap, dst, count);
}

// ---- fingerprint similarity between the resident models (arp_similarity.h): inter = B B^T of a bit matrix
// The result is F x F, not U rows of columns: sort_to_runs finds the rows — those of the persistence table (atom level) or of
// the residue persistence table (residue level), by their re-key steps —, and the bit matrix, the slicing and the product are
// this launch's own.  One wait (U).  Only the bags are read; nothing but the matrix, its bit matrix and the shared scratch is
// written.
int arp_models_similarity_launch(arp_ctx* c, uint32_t planes, uint32_t ctype_mask, uint32_t flags, int64_t* n_models, int64_t* n_rows) {
    if (!c || !n_models || !n_rows) return ARP_E_ARG;
    const std::string fn = "arp_models_similarity_launch: ";
    const bool by_res = (flags & ARP_SIM_BY_RESIDUE) != 0;
    if (flags & ~ARP_SIM_BY_RESIDUE) FAIL(c, ARP_E_ARG, fn + "unknown flag");
    if (planes & ~((1u << ARP_SIM_PLANES) - 1u)) FAIL(c, ARP_E_ARG, fn + "planes has bits beyond the 20 planes");
    if (!planes) FAIL(c, ARP_E_ARG, fn + "a planes mask of 0 makes no feature");
    if (!by_res && (planes >> (TABLE_SIFT_BITS + 1))) FAIL(c, ARP_E_ARG, fn + "planes 16 ... 19 (the ring / amide classes) exist at residue level only");
    if (ctype_mask & ~ARP_FILTER_CTYPE_ALL) FAIL(c, ARP_E_ARG, fn + "ctype_mask has bits beyond the 7 contact types");
    if (!ctype_mask) FAIL(c, ARP_E_ARG, fn + "a ctype_mask of 0 admits no atom-atom record");
    CHK(launch_refusals(c, fn, NEED_WHOLE | NEED_MODELS, nullptr));
    const int64_t F = c->models_n;
    *n_models = F;
    if (F > ARP_SIM_MAX_MODELS) FAIL(c, ARP_E_CAPACITY, fn + "more than 4096 models (the matrix and its page-locked stage would pass 64 MiB)");
    CHK(launch_refusals(c, fn, by_res ? NEED_FIVE_BAGS : NEED_AA_BAG, (by_res ? RESPERSIST_TABLE : PERSIST_TABLE).no_pass));
    SimilarityResult& S = c->similarity;
    if (S.valid && S.F == F && S.planes == planes && S.ctype_mask == ctype_mask && S.flags == flags) { *n_rows = S.rows; return ARP_OK; }
    S.valid = false;
    const FiveBags B = five_bags(c, by_res);
    const size_t k = B.k;
    CHK(records_fit(c, fn, k));
    PairModelKey G{};
    CHK(pair_model_key(c, fn, by_res, "(pair, model)", &G));
    HIPCHK(c, hipSetDevice(c->device));
    HIPCHK(c, S.inter.reserve((size_t)(F * F)));
    const auto done = [&](long long rows, long long words, long long slices) {
        S.F = F; S.rows = rows; S.words = words; S.slices = slices;
        S.planes = planes; S.ctype_mask = ctype_mask; S.flags = flags;
        S.valid = true;
        ++S.launches;
        *n_rows = rows;
        return ARP_OK;
    };
    // ---- the records keyed by (pair, model), sorted by every bit; the host learns U (the one wait)
    SortedRuns Q{};
    if (k > 0)
        CHK(sort_to_runs(c, fn, k, B.cap, by_res ? 0 : 1, [&](unsigned long long* key, unsigned long long* val, TableKey* K) -> int {
            if (by_res) enqueue_residue_rekey(c, B, G, key, val, K);
            else (void)enqueue_persist_rekey(c, G, k, key, val, K);
            return ARP_OK;
        }, &Q));
    const long long U = Q.U;
    if (U == 0) {      // no record with a row: no feature in any model
        HIPCHK(c, hipMemsetAsync(S.inter.p, 0, (size_t)(F * F) * sizeof(uint32_t), c->stream));
        return done(0, 0, 0);
    }
    // ---- the bit matrix: popcount(planes) planes of ceil(U / 64) words a model
    const long long NP = __builtin_popcount(planes), wpp = (U + 63) / 64, W = NP * wpp;
    if (NP * U >= (1ll << 32)) FAIL(c, ARP_E_CAPACITY, fn + "2^32 features or more (a count would not fit uint32)");
    if (F * W >= (1ll << 29)) FAIL(c, ARP_E_CAPACITY, fn + "a bit matrix of 4 GiB or more");
    HIPCHK(c, S.bits.reserve((size_t)(F * W)));
    HIPCHK(c, hipMemsetAsync(S.bits.p, 0, (size_t)(F * W) * sizeof(unsigned long long), c->stream));
    CHK(enqueue_run_starts(c, Q.R, U));
    SimArgs A{};
    A.key = Q.key; A.val = Q.val; A.row_start = Q.R.row_start; A.U = U;
    A.fbits = G.fbits; A.planes = planes; A.ctype_mask = ctype_mask; A.F = (uint32_t)F;
    A.bits = S.bits.p; A.wpp = wpp; A.W = W;
    hipLaunchKernelGGL(k_sim_bits, dim3(nblocks(U, 4, 16384)), dim3(256), 0, c->stream, A);
    // ---- inter = B B^T: the tile pairs of the upper triangle times as many word slices as fill the device (F = 8 is one
    // tile: the words supply the parallelism), a slice no shorter than one staged panel
    const long long tiles = (F + SIM_TILE - 1) / SIM_TILE, pairs = tiles * (tiles + 1) / 2, chunks = (W + SIM_KC - 1) / SIM_KC;
    const long long want = std::max<long long>(1, std::min<long long>(chunks, (2ll * c->num_cu + pairs - 1) / pairs));
    const long long per = (chunks + want - 1) / want * SIM_KC, slices = (W + per - 1) / per;
    A.per = per; A.slices = (int)slices; A.tiles = (int)tiles; A.inter = S.inter.p;
    if (slices > 1) HIPCHK(c, hipMemsetAsync(S.inter.p, 0, (size_t)(F * F) * sizeof(uint32_t), c->stream));
    hipLaunchKernelGGL(k_sim_gram, dim3((unsigned)pairs, (unsigned)slices), dim3(256), 0, c->stream, A);
    CHK(check_launch(c, (fn + "bits / gram").c_str()));
    return done(U, W, slices);
}

int arp_models_similarity_fetch(arp_ctx* c, int64_t cap_models, uint32_t* inter, int64_t* n_models) {
    if (!c || !n_models) return ARP_E_ARG;
    const SimilarityResult& S = c->similarity;
    if (!c->contacts_valid || !S.valid) FAIL(c, ARP_E_ARG, "arp_models_similarity_fetch: no matrix (arp_models_similarity_launch after a pass)");
    *n_models = S.F;
    if (S.F > cap_models) FAIL(c, ARP_E_CAPACITY, "arp_models_similarity_fetch: output buffer too small");
    if (!inter) FAIL(c, ARP_E_ARG, "arp_models_similarity_fetch: output missing");
    HIPCHK(c, hipSetDevice(c->device));
    const size_t bytes = (size_t)(S.F * S.F) * sizeof(uint32_t);
    CHK(stage_copy(c, S.inter.p, bytes));
    memcpy(inter, c->table_stage, bytes);
    return ARP_OK;
}

int arp_models_similarity_info(arp_ctx* c, int64_t info[4]) {
    if (!c || !info) return ARP_E_ARG;
    const SimilarityResult& S = c->similarity;
    info[0] = S.valid ? S.rows : 0;
    info[1] = S.valid ? S.words : 0;
    info[2] = S.valid ? S.slices : 0;
    info[3] = S.launches;
    return ARP_OK;
}

// ---- contact lifetimes over the resident models (arp_lifetimes.h): the persistence table's rows, intervals for counts
// made_with keeps two words: gap << 16 | sift_any (16 + 15 bits) and ctype_mask.
int arp_models_lifetimes_launch(arp_ctx* c, uint32_t gap, uint32_t sift_any, uint32_t ctype_mask, int64_t* count) {
    if (!c || !count) return ARP_E_ARG;
    const std::string fn = LIFETIMES_TABLE.launch();
    CHK(check_masks(c, fn, {{sift_any, ARP_FILTER_SIFT_ALL}, {ctype_mask, ARP_FILTER_CTYPE_ALL}},
                    "a mask has bits beyond the 15 SIFt bits / the 7 contact types", "a mask of 0 lets no record take part"));
    if (gap > ARP_LIFETIMES_MAX_GAP) FAIL(c, ARP_E_ARG, fn + "gap beyond 65 534 models");
    LifetimesArgs A{};
    return make_table(c, LIFETIMES_TABLE, count,
        [&](const FiveBags& B, unsigned long long* key, unsigned long long* val, TableKey* K) -> int {
            PairModelKey G{};
            CHK(pair_model_key(c, fn, false, "(atom, atom, model)", &G));
            // a < b <= n - 1 < 2^bits: the a field of a record's key is never all ones, so the all-ones key of a record that is
            // left out is no record's in the sorted bits (no tie bit, unlike enqueue_residue_rekey)
            if (G.n > ((int64_t)1 << G.bits)) FAIL(c, ARP_E_HIP, fn + "atom ids beyond their key bits");
            A.ci = c->out_i.p; A.cj = c->out_j.p; A.d_in = c->out_d.p; A.s_in = c->out_s.p; A.ct_in = c->out_ct.p;
            A.k = (long long)B.k;
            A.n = (uint32_t)G.n;      // (> 0: the bag has records)
            A.bbits = G.bits; A.fbits = G.fbits;
            A.sift_any = sift_any; A.ctype_mask = ctype_mask; A.gap = gap;
            A.key = key; A.val = val;
            *K = TableKey{G.total(), G.fbits};
            hipLaunchKernelGGL(k_lifetimes_rekey, dim3(nblocks((int64_t)B.k, 256, 2048)), dim3(256), 0, c->stream, A);
            return ARP_OK;
        },
        [&](const SortedRuns& S, const Columns& col) {
            A.key = (unsigned long long*)S.key; A.val = (unsigned long long*)S.val; A.row_start = S.R.row_start; A.U = S.U;
            A.t_a = col[LT_A]; A.t_b = col[LT_B]; A.t_nmodels = col[LT_NMODELS]; A.t_first = col[LT_FIRST]; A.t_last = col[LT_LAST];
            A.t_nintervals = col[LT_NINTERVALS]; A.t_longest = col[LT_LONGEST]; A.t_longest_start = col[LT_LONGEST_START];
            A.t_head = col[LT_HEAD]; A.t_tail = col[LT_TAIL]; A.t_span_sum = col[LT_SPAN_SUM];
            hipLaunchKernelGGL(k_lifetimes_reduce, dim3(nblocks(S.U, 4, 16384)), dim3(256), 0, c->stream, A);
        },
        gap << 16 | sift_any, ctype_mask);
}

int arp_models_lifetimes_fetch(arp_ctx* c, int64_t cap, int32_t* a, int32_t* b, uint16_t* n_models, int32_t* first, int32_t* last,
                               uint16_t* n_intervals, uint16_t* longest, int32_t* longest_start, uint16_t* head, uint16_t* tail,
                               uint32_t* span_sum, int64_t* count) {
    void* const dst[LT_COLS] = {a, b, n_models, first, last, n_intervals, longest, longest_start, head, tail, span_sum};
    return table_fetch(c, LIFETIMES_TABLE, cap, dst, count);
}

int arp_models_lifetimes_info(arp_ctx* c, int64_t info[2]) {
    if (!c || !info) return ARP_E_ARG;
    const ResultTable& T = c->lifetimes;
    info[0] = T.valid ? T.count : 0;
    info[1] = T.launches;
    return ARP_OK;
}

// ---- interaction networks (arp_networks.h): the components of the contact graph, by lock-free union-find
// Nothing is sorted: a sequence of its own from the shared steps, with ONE wait — U, the components.  Of the results only the
// atom-atom bag (and res_id) is read; this table, its labels and its scratch alone are written.
// made_with keeps two words: flags << 15 | sift_any and ctype_mask.
int arp_networks_launch(arp_ctx* c, uint32_t sift_any, uint32_t ctype_mask, uint32_t flags, int64_t* count) {
    if (!c || !count) return ARP_E_ARG;
    const TableSpec& spec = NETWORKS_TABLE;
    const std::string fn = spec.launch();
    CHK(check_masks(c, fn, {{sift_any, ARP_FILTER_SIFT_ALL}, {ctype_mask, ARP_FILTER_CTYPE_ALL}},
                    "a mask has bits beyond the 15 SIFt bits / the 7 contact types", "a mask of 0 lets no record take part"));
    if (flags & ~ARP_NET_BY_RESIDUE) FAIL(c, ARP_E_ARG, fn + "unknown flag");
    CHK(launch_refusals(c, fn, spec.needs, spec.no_pass));
    ResultTable& T = c->networks;
    const uint32_t arg0 = flags << 15 | sift_any;
    if (T.made_with(arg0, ctype_mask)) { *count = T.count; return ARP_OK; }
    HIPCHK(c, hipSetDevice(c->device));
    T.valid = false;
    T.count = 0;
    const size_t k = (size_t)c->n_contacts;
    CHK(records_fit(c, fn, k));
    const bool by_res = (flags & ARP_NET_BY_RESIDUE) != 0;
    const int64_t N = by_res ? c->nres : c->n;
    if (N >= ((int64_t)1 << 31)) FAIL(c, ARP_E_CAPACITY, fn + "2^31 nodes or more");
    c->net_nodes = N;
    const auto done = [&](long long rows) { return table_done(T, arg0, ctype_mask, rows, count); };
    if (N == 0) return done(0);
    HIPCHK(c, c->net_label.reserve((size_t)N));
    if (k == 0) {      // (no record: every node alone and untouched)
        HIPCHK(c, hipMemsetAsync(c->net_label.p, 0xFF, (size_t)N * sizeof(int), c->stream));
        return done(0);
    }
    // ---- union-find over the records, labels, counts per root
    HIPCHK(c, c->net_scratch.reserve(5 * (size_t)N + 1));
    const int tiles = (int)((N + NET_TILE - 1) / NET_TILE);
    CHK(reserve_tile_counts(c, tiles));
    NetArgs A{};
    A.ci = c->out_i.p; A.cj = c->out_j.p; A.s_in = c->out_s.p; A.ct_in = c->out_ct.p;
    A.k = (long long)k; A.res_id = c->res_id.p;
    A.sift_any = sift_any; A.ctype_mask = ctype_mask; A.flags = flags;
    A.N = (int)N;
    int* const s = c->net_scratch.p;
    A.parent = s; A.n_nodes = s + N; A.n_edges = s + 2 * N; A.bits = (uint32_t*)(s + 3 * N); A.touched = s + 4 * N; A.err = s + 5 * N;
    A.label = c->net_label.p;
    A.tile_rows = c->table_tiles.p;
    const dim3 per_node(nblocks(N, NET_THREADS, 2048)), per_record(nblocks((int64_t)k, NET_THREADS, 2048));
    hipLaunchKernelGGL(k_net_init, per_node, dim3(NET_THREADS), 0, c->stream, A);
    hipLaunchKernelGGL(k_net_hook, per_record, dim3(NET_THREADS), 0, c->stream, A);
    hipLaunchKernelGGL(k_net_label, per_node, dim3(NET_THREADS), 0, c->stream, A);
    hipLaunchKernelGGL(k_net_edges, per_record, dim3(NET_THREADS), 0, c->stream, A);
    // ---- roots per tile, scanned; the host learns U (the one wait; negative when a kernel met one of its bounds)
    hipLaunchKernelGGL(k_net_roots, dim3(tiles), dim3(NET_THREADS), 0, c->stream, A);
    long long U = 0;
    CHK(wait_tile_total(c, tiles, &U, fn + "union / label / count"));
    if (U < 0 || U > (long long)N || U > (long long)k) FAIL(c, ARP_E_HIP, fn + "row count out of range");
    if (U == 0) return done(0);
    // ---- the rows, each at its rank
    const TableLayout lay = table_layout(spec, (size_t)U);
    HIPCHK(c, T.slab.reserve(lay.bytes));
    const Columns col{T.slab.p, lay.off};
    A.U = U;
    A.t_root = col[NW_ROOT]; A.t_nnodes = col[NW_NNODES]; A.t_nedges = col[NW_NEDGES]; A.t_sift = col[NW_SIFT]; A.t_ctype = col[NW_CTYPE];
    hipLaunchKernelGGL(k_net_rows, dim3(tiles), dim3(NET_THREADS), 0, c->stream, A);
    CHK(check_launch(c, (fn + "rows").c_str()));
    return done(U);
}

int arp_networks_fetch(arp_ctx* c, int64_t cap, int32_t* root, int32_t* n_nodes, int32_t* n_edges, uint16_t* sift_or, uint8_t* ctype_or,
                       int64_t* count) {
    void* const dst[NW_COLS] = {root, n_nodes, n_edges, sift_or, ctype_or};
    return table_fetch(c, NETWORKS_TABLE, cap, dst, count);
}

int arp_networks_labels_fetch(arp_ctx* c, int64_t cap, int32_t* label, int64_t* nodes) {
    if (!c || !nodes) return ARP_E_ARG;
    const ResultTable& T = c->networks;
    if (!c->contacts_valid || !T.valid) FAIL(c, ARP_E_ARG, "arp_networks_labels_fetch: no labels (arp_networks_launch after a pass)");
    *nodes = c->net_nodes;
    if (c->net_nodes > cap) FAIL(c, ARP_E_CAPACITY, "arp_networks_labels_fetch: output buffer too small");
    if (c->net_nodes == 0) return ARP_OK;
    if (!label) FAIL(c, ARP_E_ARG, "arp_networks_labels_fetch: output missing");
    HIPCHK(c, hipSetDevice(c->device));
    const size_t bytes = (size_t)c->net_nodes * sizeof(int32_t);
    CHK(stage_copy(c, c->net_label.p, bytes));
    memcpy(label, c->table_stage, bytes);
    return ARP_OK;
}

int arp_networks_info(arp_ctx* c, int64_t info[3]) {
    if (!c || !info) return ARP_E_ARG;
    const ResultTable& T = c->networks;
    info[0] = T.valid ? T.count : 0;
    info[1] = T.valid ? c->net_nodes : 0;
    info[2] = T.launches;
    return ARP_OK;
}

// ---- contact coupling over the resident models (arp_coupling.h): n11 = B^T B of a feature-major bit matrix
// The rows are similarity's (sort_to_runs with the re-key step of the level); the bits, the band, the product and the
// emission are this launch's own.  Three waits: U rows, K features, P kept pairs.  Only the bags are read; nothing but the
// two tables, their bit matrices and the shared scratch is written.
// made_with keeps two words: planes | ctype_mask << 20 | flags << 27 | phi2_q << 28 | min_count << 39 | max_count << 51
// (20 + 7 + 1 + 11 + 12 + 12 bits) and max_pairs.
namespace {
// the slab of both tables: the feature columns for K rows, then the pair columns for P rows (the former do not move with P)
TableLayout couple_layout(size_t K, size_t P) {
    TableLayout L{};
    for (int q = 0; q < CP_COLS; ++q) { L.off[q] = L.bytes; L.bytes += al256((q < CP_FEATURE_COLS ? K : P) * COUPLING_TABLE.es[q]); }
    return L;
}
}  // namespace

int arp_models_coupling_launch(arp_ctx* c, uint32_t planes, uint32_t ctype_mask, uint32_t flags, uint32_t min_count, uint32_t max_count,
                               uint32_t phi2_q, int64_t max_pairs, int64_t* n_features, int64_t* n_pairs) {
    if (!c || !n_features || !n_pairs) return ARP_E_ARG;
    const TableSpec& spec = COUPLING_TABLE;
    const std::string fn = spec.launch();
    *n_features = 0;
    *n_pairs = 0;
    const bool by_res = (flags & ARP_COUPLE_BY_RESIDUE) != 0;
    CHK(check_masks(c, fn, {{planes, (1u << ARP_SIM_PLANES) - 1u}, {ctype_mask, ARP_FILTER_CTYPE_ALL}},
                    "a mask has bits beyond the 20 planes / the 7 contact types", "a mask of 0 lets no record take part"));
    if (flags & ~ARP_COUPLE_BY_RESIDUE) FAIL(c, ARP_E_ARG, fn + "unknown flag");
    if (!by_res && (planes >> (TABLE_SIFT_BITS + 1))) FAIL(c, ARP_E_ARG, fn + "planes 16 ... 19 (the ring / amide classes) exist at residue level only");
    if (phi2_q < 1u || phi2_q > 1024u) FAIL(c, ARP_E_ARG, fn + "phi2_q must lie in 1 ... 1024");
    if (max_pairs < 0) FAIL(c, ARP_E_ARG, fn + "max_pairs must not be negative");
    CHK(launch_refusals(c, fn, spec.needs, spec.no_pass));
    const int64_t F = c->models_n;
    if (F > ARP_SIM_MAX_MODELS) FAIL(c, ARP_E_CAPACITY, fn + "more than 4096 models (the criterion's integers would pass 64 bits)");
    if (!(1u <= min_count && min_count <= max_count && (int64_t)max_count <= F - 1))
        FAIL(c, ARP_E_ARG, fn + "1 <= min_count <= max_count <= F - 1 is required (a row present in no model or in every model is no feature; F >= 2)");
    CHK(launch_refusals(c, fn, by_res ? NEED_FIVE_BAGS : NEED_AA_BAG, (by_res ? RESPERSIST_TABLE : PERSIST_TABLE).no_pass));
    ResultTable& T = c->coupling;
    CouplingScratch& X = c->couple;
    const uint64_t arg0 = (uint64_t)planes | (uint64_t)ctype_mask << 20 | (uint64_t)flags << 27 | (uint64_t)phi2_q << 28 |
                          (uint64_t)min_count << 39 | (uint64_t)max_count << 51;
    const uint64_t arg1 = (uint64_t)max_pairs;
    if (T.made_with(arg0, arg1)) { *n_features = X.features; *n_pairs = T.count; return ARP_OK; }
    T.valid = false;
    T.count = 0;
    const FiveBags B = five_bags(c, by_res);
    const size_t k = B.k;
    CHK(records_fit(c, fn, k));
    PairModelKey G{};
    CHK(pair_model_key(c, fn, by_res, "(pair, model)", &G));
    HIPCHK(c, hipSetDevice(c->device));
    const auto done = [&](long long U, long long K, long long tile_pairs, long long P) {
        X.rows = U; X.features = K; X.tile_pairs = tile_pairs; X.flags = flags;
        *n_features = K;
        return table_done(T, arg0, arg1, P, n_pairs);
    };
    if (k == 0) return done(0, 0, 0, 0);
    // ---- the records keyed by (pair, model), sorted by every bit; the host learns U (wait 1).  The tile counts are sized for
    // the rows there can be at most, so that nothing the enqueued kernels read moves afterwards
    CHK(reserve_tile_counts(c, (int)std::max((k + RUNS_TILE - 1) / RUNS_TILE, (k + COUPLE_TILE_ROWS - 1) / COUPLE_TILE_ROWS)));
    SortedRuns Q{};
    CHK(sort_to_runs(c, fn, k, B.cap, by_res ? 0 : 1, [&](unsigned long long* key, unsigned long long* val, TableKey* K) -> int {
        if (by_res) enqueue_residue_rekey(c, B, G, key, val, K);
        else (void)enqueue_persist_rekey(c, G, k, key, val, K);
        return ARP_OK;
    }, &Q));
    const long long U = Q.U;
    if (U == 0) return done(0, 0, 0, 0);      // no record with a row
    // ---- the model bits of every row and their count
    const long long fw = (F + 63) / 64;
    if (U * fw >= (1ll << 29)) FAIL(c, ARP_E_CAPACITY, fn + "a bit matrix of 4 GiB or more");
    HIPCHK(c, X.rowbits.reserve((size_t)(U * fw)));
    HIPCHK(c, X.n_row.reserve((size_t)U));
    CHK(enqueue_run_starts(c, Q.R, U));
    CoupleArgs A{};
    A.key = Q.key; A.val = Q.val; A.row_start = Q.R.row_start; A.U = U;
    A.fbits = G.fbits; A.bbits = G.bits; A.planes = planes; A.ctype_mask = ctype_mask; A.F = (uint32_t)F; A.fw = (int)fw;
    A.rowbits = X.rowbits.p; A.n_row = X.n_row.p;
    hipLaunchKernelGGL(k_couple_bits, dim3(nblocks(U, 4, 16384)), dim3(256), 0, c->stream, A);
    // ---- the rows in the band per tile, scanned; the host learns K (wait 2)
    A.min_count = min_count; A.max_count = max_count;
    const int row_tiles = (int)((U + COUPLE_TILE_ROWS - 1) / COUPLE_TILE_ROWS);
    A.tile_keep = c->table_tiles.p;
    hipLaunchKernelGGL(k_couple_keep, dim3(row_tiles), dim3(COUPLE_TILE_ROWS), 0, c->stream, A);
    long long K = 0;
    CHK(wait_tile_total(c, row_tiles, &K, fn + "bits / band count"));
    if (K < 0 || K > U) FAIL(c, ARP_E_HIP, fn + "feature count out of range");
    *n_features = K;
    if (K > ARP_COUPLE_MAX_FEATURES) FAIL(c, ARP_E_CAPACITY, fn + "more than 65 536 features (narrow the occupancy band)");
    if (K == 0) return done(U, 0, 0, 0);
    // ---- the features at their rank: bits, counts and the feature table.  The slab has room for as many pairs as may be kept
    const long long all_pairs = K * (K - 1) / 2;
    const long long cap = std::min<long long>({(long long)max_pairs, all_pairs, (1ll << 31) - 1});
    HIPCHK(c, X.bits.reserve((size_t)(K * fw)));
    HIPCHK(c, X.n.reserve((size_t)K));
    const TableLayout room = couple_layout((size_t)K, (size_t)cap);
    HIPCHK(c, T.slab.reserve(room.bytes));
    const Columns fcol{T.slab.p, room.off};
    A.K = K; A.bits = X.bits.p; A.n = X.n.p;
    A.t_a = fcol[CP_A]; A.t_b = fcol[CP_B]; A.t_count = fcol[CP_COUNT];
    hipLaunchKernelGGL(k_couple_compact, dim3(row_tiles), dim3(COUPLE_TILE_ROWS), 0, c->stream, A);
    if (K == 1) {
        CHK(check_launch(c, (fn + "compact").c_str()));
        return done(U, 1, 0, 0);
    }
    // ---- n11 = B^T B over the tile pairs of the upper triangle, the criterion, the append; the host learns P (wait 3).  The
    // sorted records are read for the last time by k_couple_compact: their buffers now take the pairs (a buffer that has to
    // grow is freed once the device is idle: hipFree waits)
    const long long tiles = (K + SIM_TILE - 1) / SIM_TILE, tile_pairs = tiles * (tiles + 1) / 2;
    SortScratch& s = c->table_sort;
    if (cap > 0) CHK(reserve_key_sort(c, s, (size_t)cap, (size_t)cap));
    HIPCHK(c, hipMemsetAsync(c->table_total.p, 0, sizeof(long long), c->stream));
    A.tiles = (int)tiles; A.q = phi2_q; A.vbits = index_bits(K);
    A.total = (unsigned long long*)c->table_total.p; A.pair_key = s.key[0].p; A.pair_val = s.val[0].p; A.cap = cap;
    hipLaunchKernelGGL(k_couple_gram, dim3((unsigned)tile_pairs), dim3(256), 0, c->stream, A);
    long long P = 0;
    CHK(wait_count(c, c->table_total.p, &P, fn + "compact / gram"));
    if (P < 0 || P > all_pairs) FAIL(c, ARP_E_HIP, fn + "pair count out of range");
    *n_pairs = P;
    if (P > cap) FAIL(c, ARP_E_CAPACITY, fn + (P > (long long)max_pairs ? "more kept pairs than max_pairs (raise phi2_q, narrow the band, or come back with *n_pairs)"
                                                                        : "2^31 kept pairs or more"));
    if (P == 0) return done(U, K, tile_pairs, 0);
    // ---- their canonical order: ascending u << vbits | v, then the columns
    int sorted = 0;
    enqueue_key_sort(c, s, (size_t)P, 2 * A.vbits, &sorted);
    const TableLayout lay = couple_layout((size_t)K, (size_t)P);
    const Columns pcol{T.slab.p, lay.off};
    A.pair_key = s.key[sorted].p; A.pair_val = s.val[sorted].p; A.P = P;
    A.t_u = pcol[CP_U]; A.t_v = pcol[CP_V]; A.t_n11 = pcol[CP_N11];
    hipLaunchKernelGGL(k_couple_rows, dim3(nblocks(P, 256, 2048)), dim3(256), 0, c->stream, A);
    CHK(check_launch(c, (fn + "sort / rows").c_str()));
    return done(U, K, tile_pairs, P);
}

int arp_models_coupling_fetch(arp_ctx* c, int64_t cap_features, int64_t cap_pairs, int32_t* a, int32_t* b, uint32_t* count, uint32_t* u,
                              uint32_t* v, uint32_t* n11, int64_t* n_features, int64_t* n_pairs) {
    if (!c || !n_features || !n_pairs) return ARP_E_ARG;
    const ResultTable& T = c->coupling;
    if (!c->contacts_valid || !T.valid) FAIL(c, ARP_E_ARG, "arp_models_coupling_fetch: no table (arp_models_coupling_launch after a pass)");
    const size_t K = (size_t)c->couple.features, P = (size_t)T.count;
    *n_features = (int64_t)K;
    *n_pairs = (int64_t)P;
    if ((int64_t)K > cap_features || (int64_t)P > cap_pairs) FAIL(c, ARP_E_CAPACITY, "arp_models_coupling_fetch: output buffers too small");
    if (K == 0) return ARP_OK;
    HIPCHK(c, hipSetDevice(c->device));
    const TableLayout L = couple_layout(K, P);
    CHK(stage_copy(c, T.slab.p, L.bytes));
    void* const dst[CP_COLS] = {a, b, count, u, v, n11};
    for (int q = 0; q < CP_COLS; ++q)
        if (dst[q]) memcpy(dst[q], c->table_stage + L.off[q], (q < CP_FEATURE_COLS ? K : P) * COUPLING_TABLE.es[q]);
    return ARP_OK;
}

int arp_models_coupling_info(arp_ctx* c, int64_t info[4]) {
    if (!c || !info) return ARP_E_ARG;
    const ResultTable& T = c->coupling;
    info[0] = T.valid ? c->couple.rows : 0;
    info[1] = T.valid ? c->couple.features : 0;
    info[2] = T.valid ? c->couple.tile_pairs : 0;
    info[3] = T.launches;
    return ARP_OK;
}

// ---- the ligand-pose family (DESIGN.md 5o ... 5s): what its entries share
namespace {
// what every launch on a resident receptor refuses first, in this order (the pose launches, the ligand-library launch)
int receptor_refusals(arp_ctx* c, const std::string& fn) {
    if (c->pass_pending) FAIL(c, ARP_E_ARG, fn + "a pass has not been waited for (arp_run_wait)");
    if (c->n <= 0) FAIL(c, ARP_E_ARG, fn + "no structure resident");
    if (c->models_n > 0) FAIL(c, ARP_E_ARG, fn + "models are resident (the receptor is one structure)");
    if (c->batch_n > 0) FAIL(c, ARP_E_ARG, fn + "a batch is resident (the receptor is one structure)");
    if (c->has_home || c->has_gid || c->shard_resident) FAIL(c, ARP_E_ARG, fn + "not for a shard of a distributed structure");
    return ARP_OK;
}
// what both pose launches refuse first, in this order
int pose_launch_refusals(arp_ctx* c, const std::string& fn, int64_t n_poses) {
    CHK(receptor_refusals(c, fn));
    if (!c->sel_uploaded || c->nsel < 0) FAIL(c, ARP_E_ARG, fn + "no uploaded selection (arp_set_selection names the movable set)");
    if (c->sel_all || c->whole_structure || c->nsel >= c->n) FAIL(c, ARP_E_ARG, fn + "the selection is the whole structure (nothing is left as the receptor)");
    if (c->nsel < 1 || c->nsel > POSES_MAX_ATOMS) FAIL(c, ARP_E_ARG, fn + "the movable set must hold 1 ... ARP_POSES_MAX_ATOMS selected atoms");
    if (n_poses < 1 || n_poses > POSES_MAX_POSES) FAIL(c, ARP_E_ARG, fn + "1 ... ARP_POSES_MAX_POSES poses a launch (chunk them)");
    return ARP_OK;
}
// what the entries that read resident pose results refuse (other poses: P and S here, the coordinates on the device, enqueue_same_poses)
int need_poses_result(arp_ctx* c, const std::string& fn) {
    if (!c->poses.valid) FAIL(c, ARP_E_ARG, fn + "no poses result (arp_poses_contacts_launch; an input or the selection changed since)");
    return ARP_OK;
}
int need_planes_result_of_same_poses(arp_ctx* c, const std::string& fn) {
    const PosesPlanesResult& L = c->pplanes;
    if (!L.valid) FAIL(c, ARP_E_ARG, fn + "no poses-planes result (arp_poses_planes_launch; an input, the selection or the plane atoms changed since)");
    if (L.P != c->poses.P || L.S != c->poses.S) FAIL(c, ARP_E_ARG, fn + "the poses result and the poses-planes result differ in P or S (launch both on the same poses)");
    return ARP_OK;
}
// both results keep their uploaded poses: a word that differs ORs 1 into *flag_word (zeroed by the caller, read in its one wait)
void enqueue_same_poses(arp_ctx* c, void* flag_word) {
    const long long words = (long long)(c->poses.P * c->poses.S * 3);
    hipLaunchKernelGGL(k_pfp_same_poses, dim3(nblocks(words, 256, c->num_cu)), dim3(256), 0, c->stream, (const uint32_t*)c->poses.rec.xyz.p,
                       (const uint32_t*)c->pplanes.xyz.p, words, (uint32_t*)flag_word);
}

// The four ring / amide tables of the poses-planes result and of a shortlist (PplColumns, arp_poses_planes.h): the columns
// PLANE_TABLES names.  In a slab: table after table, column after column in that order, each on a 256-byte boundary.
struct PlaneLayout { size_t col[BAG_KINDS][BAG_COLS]; };
PlaneLayout plane_tables_layout(const size_t counts[4], size_t start, size_t* bytes) {
    PlaneLayout L{};
    size_t at = start;
    for (int t = 0; t < BAG_KINDS; ++t) at = bag_slab_layout(t, counts[t], at, L.col[t]);
    *bytes = at;
    return L;
}
PplColumns bind_plane_columns(uint8_t* slab, const PlaneLayout& L) {      // (base, the tables' sorted positions, is the caller's)
    PplColumns col{};
    for (int t = 0; t < BAG_KINDS; ++t) {
        col.i0[t] = (int*)(slab + L.col[t][0]); col.i1[t] = (int*)(slab + L.col[t][1]);
        for (int q = 0; q < PLANE_TABLES[t].n_val; ++q) col.d[t][q] = (double*)(slab + L.col[t][BAG_VAL0 + q]);
        for (int q = 0; q < PLANE_TABLES[t].n_byte; ++q) col.u[t][q] = slab + L.col[t][BAG_BYTE0 + q];
    }
    return col;
}

// What a fetch copies: every piece through the page-locked stage in one wait (pageable destinations cost a copy of a few tens of
// kB milliseconds now and then), then to the caller's arrays.
struct StagePiece { void* dst; const void* src; size_t bytes; };
void want_piece(std::vector<StagePiece>& pieces, void* dst, const void* src, size_t bytes) {
    if (dst && bytes) pieces.push_back(StagePiece{dst, src, bytes});
}
int stage_fetch(arp_ctx* c, const std::vector<StagePiece>& pieces) {
    std::vector<size_t> at(pieces.size() + 1, 0);      // (every piece on a 16-byte boundary of the stage)
    for (size_t q = 0; q < pieces.size(); ++q) at[q + 1] = at[q] + ((pieces[q].bytes + 15) & ~(size_t)15);
    if (at.back() > 0) CHK(table_stage_reserve(c, at.back()));
    for (size_t q = 0; q < pieces.size(); ++q)
        HIPCHK(c, hipMemcpyAsync((uint8_t*)c->table_stage + at[q], pieces[q].src, pieces[q].bytes, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    for (size_t q = 0; q < pieces.size(); ++q) memcpy(pieces[q].dst, (const uint8_t*)c->table_stage + at[q], pieces[q].bytes);
    return ARP_OK;
}
// A fetch of plane table t: the caller's column pointers are columns the table has (*records: a record column is asked for) ...
int plane_fetch_columns(arp_ctx* c, const std::string& fn, int t, const void* first, const void* second, void* const v[4], uint8_t* const u[3], bool* records) {
    *records = first || second;
    for (int q = 0; q < 4; ++q) {
        if (v[q] && q >= PLANE_TABLES[t].n_val) FAIL(c, ARP_E_ARG, fn + "the table has no such value column");
        *records = *records || v[q];
    }
    for (int q = 0; q < 3; ++q) {
        if (u[q] && q >= PLANE_TABLES[t].n_byte) FAIL(c, ARP_E_ARG, fn + "the table has no such byte column");
        *records = *records || u[q];
    }
    return ARP_OK;
}
// ... and, once the fetch has checked its capacities, the k records of those columns as pieces
void plane_fetch_pieces(std::vector<StagePiece>& pieces, const PplColumns& col, int t, size_t k, void* first, void* second, void* const v[4], uint8_t* const u[3]) {
    want_piece(pieces, first, col.i0[t], k * sizeof(int32_t));
    want_piece(pieces, second, col.i1[t], k * sizeof(int32_t));
    for (int q = 0; q < PLANE_TABLES[t].n_val; ++q) want_piece(pieces, v[q], col.d[t][q], k * PLANE_TABLES[t].val_size);
    for (int q = 0; q < PLANE_TABLES[t].n_byte; ++q) want_piece(pieces, u[q], col.u[t][q], k);
}

// Append until it fits: `launch(cap)` reserves room for cap records, zeroes the counters and launches; the first `words` counters
// come back through the stage into h — h[0] the records there are, h[1] the device's error word, which `device_error` turns into
// the launch's own refusal.  A buffer that was too small is grown to the exact count and the launch repeated, `attempts` launches
// at the most: nothing is truncated.  *needed (when given) names the count before a capacity failure.
const size_t POSE_RECORD_LIMIT = ((size_t)1 << 31) - 1;
int append_until_it_fits(arp_ctx* c, const std::string& fn, size_t cap, const unsigned long long* ctr, int words, unsigned long long* h, int attempts,
                         const std::function<int(size_t)>& launch, const std::function<int(int)>& device_error, int64_t* needed) {
    for (int attempt = 1;; ++attempt) {
        CHK(launch(cap));
        CHK(stage_copy(c, ctr, (size_t)words * sizeof(unsigned long long)));
        memcpy(h, c->table_stage, (size_t)words * sizeof(unsigned long long));
        if ((uint32_t)h[1] != 0) return device_error((int)(uint32_t)h[1]);
        if (h[0] <= cap) return ARP_OK;
        if (needed) *needed = (int64_t)h[0];
        if (h[0] > POSE_RECORD_LIMIT) FAIL(c, ARP_E_CAPACITY, fn + "2^31 records or more (fewer poses a launch)");
        if (attempt == attempts) FAIL(c, ARP_E_CAPACITY, fn + "record buffer could not be sized");
        cap = (size_t)h[0];
    }
}

// The frame of both launches over poses (arp_poses_contacts_launch, arp_library_contacts_launch), after the entry's own refusals
// and voiding: the poses go up (nx floats, nh doubles), `enqueue(sink)` launches the entry's contact kernel over all `poses` of
// them into `sink` — again with room for the exact count when the first buffer (32 records per posed atom) was too small —, and
// the tail makes pose_off, sorts by the keybits bits of the key and unpacks the five columns (hi_bits above lo_bits: the two id
// columns in the key).  One wait a launch of the kernel: the record count with the device's error word.  *count: the records,
// also before a capacity failure.
int pose_records_launch(arp_ctx* c, const std::string& fn, PoseRecords& R, int64_t poses, const float* xyz, size_t nx, const double* h_xyz, size_t nh,
                        int keybits, int hi_bits, int lo_bits, const std::function<int(const PoseSink&)>& enqueue, int64_t* count) {
    R.count = 0;
    HIPCHK(c, R.xyz.reserve(std::max<size_t>(nx, 1)));
    HIPCHK(c, R.hx.reserve(std::max<size_t>(nh, 1)));
    HIPCHK(c, hipMemcpyAsync(R.xyz.p, xyz, nx * sizeof(float), hipMemcpyHostToDevice, c->stream));
    if (nh > 0) HIPCHK(c, hipMemcpyAsync(R.hx.p, h_xyz, nh * sizeof(double), hipMemcpyHostToDevice, c->stream));
    HIPCHK(c, R.ctr.reserve(2));
    HIPCHK(c, R.summary.reserve((size_t)poses * POSES_SUMMARY));
    HIPCHK(c, R.pose_off.reserve((size_t)poses + 1));
    PoseSink sink{nullptr, nullptr, 0, R.ctr.p, R.summary.p, (int*)(R.ctr.p + 1)};
    unsigned long long h[2] = {0, 0};
    const auto launch = [&](size_t cap) -> int {
        CHK(reserve_key_sort(c, R.sort, cap, cap));
        sink.key = R.sort.key[0].p; sink.val = R.sort.val[0].p; sink.cap = cap;
        HIPCHK(c, hipMemsetAsync(R.ctr.p, 0, 2 * sizeof(unsigned long long), c->stream));
        return enqueue(sink);
    };
    const auto device_error = [&](int dev) -> int {
        if (dev == ARP_E_ARG) FAIL(c, ARP_E_ARG, fn + "non-finite pose coordinate");
        if (dev == ARP_E_XBOND_NBR) FAIL(c, ARP_E_XBOND_NBR, "xbond donor without a single-bond heavy neighbour (reference: AttributeError at utils.py:173)");
        FAIL(c, ARP_E_HIP, fn + "device error");
    };
    CHK(append_until_it_fits(c, fn, std::min(POSE_RECORD_LIMIT, std::max<size_t>((size_t)1 << 16, (nx / 3) * 32)), R.ctr.p, 2, h, 3, launch, device_error,
                             count));
    const size_t k = (size_t)h[0];
    hipLaunchKernelGGL(k_poses_offsets, dim3(1), dim3(1024), 0, c->stream, (int)poses, POSES_SUMMARY - 1, R.summary.p, R.pose_off.p);
    if (k > 0) {
        int sorted = 0;
        enqueue_key_sort(c, R.sort, k, keybits, &sorted);
        size_t bytes = 0;
        sorted_layout(k, R.off, &bytes, k);
        HIPCHK(c, R.slab.reserve(bytes));
        const Columns col{R.slab.p, R.off};
        hipLaunchKernelGGL(k_pose_columns, dim3(nblocks((int64_t)k, 256, 1 << 16)), dim3(256), 0, c->stream, (long long)k, hi_bits, lo_bits,
                           R.sort.key[sorted].p, R.sort.val[sorted].p, (int*)col[0], (int*)col[1], (float*)col[2], (uint16_t*)col[3], (uint8_t*)col[4]);
    }
    CHK(check_launch(c, "k_poses_offsets / sort / k_pose_columns"));
    R.count = (int64_t)k;
    *count = R.count;
    return ARP_OK;
}
// What a fetch of either copies, after the entry's own validity and capacity checks: pose_off and the summary rows of `poses`
// poses and, `records`, the five columns — whichever the caller gave
void pose_records_pieces(std::vector<StagePiece>& pieces, const PoseRecords& R, int64_t poses, bool records, uint64_t* pose_off, int32_t* first, int32_t* second,
                         float* dist, uint16_t* sift, uint8_t* ctype, uint32_t* summary) {
    const size_t k = (size_t)R.count;
    want_piece(pieces, pose_off, R.pose_off.p, ((size_t)poses + 1) * sizeof(uint64_t));
    want_piece(pieces, summary, R.summary.p, (size_t)poses * POSES_SUMMARY * sizeof(uint32_t));
    if (records && k > 0) {
        const uint8_t* const slab = R.slab.p;
        want_piece(pieces, first, slab + R.off[0], k * sizeof(int32_t));
        want_piece(pieces, second, slab + R.off[1], k * sizeof(int32_t));
        want_piece(pieces, dist, slab + R.off[2], k * sizeof(float));
        want_piece(pieces, sift, slab + R.off[3], k * sizeof(uint16_t));
        want_piece(pieces, ctype, slab + R.off[4], k * sizeof(uint8_t));
    }
}
// The frame of both launches over poses that give ring / amide records (arp_poses_planes_launch, arp_library_planes_launch), after
// the entry's own refusals, voiding and uploads: the counters, the summary rows and the offsets of `poses` poses are reserved,
// `enqueue(sink)` launches the entry's kernel into `sink` (it reads R.ctr and R.summary, reserved by then) — again with room for
// the exact count when the first buffer (64 records a pose, 65 536 at the least) was too small —, and the tail makes the four
// pose_off tables, sorts by the keybits bits of the key and gathers the four tables into one slab.  One wait a launch of the
// kernel: the counters (records, the device's error word, records per table).  `near_cause` names the entry's PPL_E_NEAR.
struct PlaneRecords {
    DevBuf<PlaneRec>& rec;
    DevBuf<unsigned long long>& ctr;
    DevBuf<unsigned long long>& pose_off;
    DevBuf<uint32_t>& summary;
    SortScratch& sort;
    DevBuf<uint8_t>& slab;
    PplColumns& col;
    int64_t* counts;      // [4]
    int64_t& launches;
};
struct PlaneSink { PlaneRec* rec; u64* key; u64* val; u64 cap; };
int plane_records_launch(arp_ctx* c, const std::string& fn, PlaneRecords R, int64_t poses, int keybits, const char* kernel, const std::string& near_cause,
                         const std::function<void(const PlaneSink&)>& enqueue, int64_t counts[4]) {
    for (int t = 0; t < 4; ++t) R.counts[t] = counts[t] = 0;
    HIPCHK(c, R.ctr.reserve(8));
    HIPCHK(c, R.summary.reserve((size_t)poses * PPL_SUMMARY));
    HIPCHK(c, R.pose_off.reserve(4 * ((size_t)poses + 1)));
    unsigned long long h[6] = {0, 0, 0, 0, 0, 0};
    const auto launch = [&](size_t cap) -> int {
        CHK(reserve_key_sort(c, R.sort, cap, cap));
        HIPCHK(c, R.rec.reserve(cap));
        HIPCHK(c, hipMemsetAsync(R.ctr.p, 0, 6 * sizeof(unsigned long long), c->stream));
        enqueue(PlaneSink{R.rec.p, R.sort.key[0].p, R.sort.val[0].p, (u64)cap});
        CHK(check_launch(c, kernel));
        ++R.launches;
        return ARP_OK;
    };
    const auto device_error = [&](int dev) -> int {
        if (dev == ARP_E_ARG) FAIL(c, ARP_E_ARG, fn + "non-finite pose coordinate");
        if (dev == PPL_E_NEAR) FAIL(c, ARP_E_ARG, fn + near_cause);
        FAIL(c, ARP_E_HIP, fn + "device error");
    };
    CHK(append_until_it_fits(c, fn, std::min(POSE_RECORD_LIMIT, std::max<size_t>((size_t)1 << 16, (size_t)poses * 64)), R.ctr.p, 6, h, 2, launch, device_error,
                             nullptr));
    const size_t k = (size_t)h[0];
    if (h[2] + h[3] + h[4] + h[5] != h[0]) FAIL(c, ARP_E_HIP, fn + "the tables' record counts do not add up");
    hipLaunchKernelGGL(k_poses_offsets, dim3(4), dim3(1024), 0, c->stream, (int)poses, 0, R.summary.p, R.pose_off.p);
    // the four tables in one slab
    const size_t m[4] = {(size_t)h[2], (size_t)h[3], (size_t)h[4], (size_t)h[5]};
    size_t bytes = 0;
    const PlaneLayout lay = plane_tables_layout(m, 0, &bytes);
    HIPCHK(c, R.slab.reserve(std::max<size_t>(bytes, 256)));
    PplColumns col = bind_plane_columns(R.slab.p, lay);
    for (int t = 0; t < 4; ++t) col.base[t + 1] = col.base[t] + (long long)m[t];
    if (k > 0) {
        int sorted = 0;
        enqueue_key_sort(c, R.sort, k, keybits, &sorted);
        hipLaunchKernelGGL(k_ppl_columns, dim3(nblocks((int64_t)k, 256, 1 << 16)), dim3(256), 0, c->stream, (long long)k, R.sort.val[sorted].p, R.rec.p, col);
    }
    CHK(check_launch(c, "k_poses_offsets / sort / k_ppl_columns"));
    R.col = col;
    for (int t = 0; t < 4; ++t) R.counts[t] = counts[t] = (int64_t)h[2 + t];
    return ARP_OK;
}
}  // namespace

// ---- ligand poses on the resident receptor (arp_poses.h): every pose's ligand - receptor records in one launch
// No bag is read and none is written: the receptor is the static columns in the cell order of ensure_static(cutoff), the poses
// are uploaded, the records are appended as (key, payload), sorted by every bit of the key (enqueue_key_sort over the result's
// own scratch) and unpacked into a slab laid out as the sorted atom-atom bag is.  Two waits: SH when the movable set is new, and
// the record count (with the device's error word).  A record buffer that was too small is grown to the exact count and the
// launch repeated: nothing is truncated.
static_assert(POSES_MAX_ATOMS == ARP_POSES_MAX_ATOMS && POSES_MAX_ATOMS == SMALL_SEL_MAX && POSES_MAX_POSES == ARP_POSES_MAX_POSES &&
              POSES_SUMMARY == ARP_POSES_SUMMARY, "arp_poses.h names the header's limits; sel_list holds up to SMALL_SEL_MAX atoms");
int arp_poses_contacts_launch(arp_ctx* c, int64_t n_poses, const float* xyz, const double* h_xyz, double cutoff, double vdw_comp,
                              int include_sequence_adjacent, int64_t* count) {
    if (!c || !count) return ARP_E_ARG;
    const std::string fn = "arp_poses_contacts_launch: ";
    CHK(pose_launch_refusals(c, fn, n_poses));
    if (c->n >= POSES_MAX_N) FAIL(c, ARP_E_ARG, fn + "2^21 atoms or more (the sort key holds 21 bits per atom id)");
    if (!(cutoff > 0) || !(cutoff <= ARP_POSES_MAX_CUTOFF)) FAIL(c, ARP_E_ARG, fn + "cutoff must be in (0, 6.0] (beyond 6.0 selection_plus would depend on the pose)");
    if (!std::isfinite(vdw_comp)) FAIL(c, ARP_E_ARG, fn + "vdw_comp is not finite");
    if (c->sb_index_src == 0) FAIL(c, ARP_E_ARG, fn + "single-bond neighbours were given as coordinates only (arp_set_single_bond_neighbour_coords): which atom moves with a pose is not known");
    if (!xyz) FAIL(c, ARP_E_ARG, fn + "xyz missing");
    HIPCHK(c, hipSetDevice(c->device));
    CHK(join_upload_lists(c));
    CHK(ensure_static(c, cutoff));
    PosesResult& R = c->poses;
    const int n = (int)c->n, S = (int)c->nsel;
    const int64_t P = n_poses;
    // ---- the movable set's tables, once per structure and selection (the first wait: SH)
    if (R.movable_static != c->static_epoch || R.movable_sel != c->sel_epoch) {
        R.movable_static = R.movable_sel = 0;
        HIPCHK(c, R.sel_h.reserve((size_t)S + 1));
        HIPCHK(c, R.pos_of.reserve((size_t)n));
        HIPCHK(c, hipMemsetAsync(R.pos_of.p, 0xFF, (size_t)n * sizeof(int), c->stream));
        hipLaunchKernelGGL(k_poses_movable, dim3(1), dim3(1024), 0, c->stream, S, c->sel_list.p, c->h_off.p, R.sel_h.p, R.pos_of.p);
        CHK(check_launch(c, "k_poses_movable"));
        CHK(stage_copy(c, R.sel_h.p + S, sizeof(int)));
        int sh = 0;
        memcpy(&sh, c->table_stage, sizeof(sh));
        if (sh < 0) FAIL(c, ARP_E_HIP, fn + "hydrogen count of the movable set out of range");
        R.SH = sh;
        R.S = S;
        R.movable_static = c->static_epoch; R.movable_sel = c->sel_epoch;
    }
    const int64_t SH = R.SH;
    if (SH > 0 && !h_xyz) FAIL(c, ARP_E_ARG, fn + "h_xyz missing (the movable set has hydrogens)");
    // ---- from here on the previous result is gone, and what was made from it
    void_pose_results(c, POSE_CONTACTS);
    PoseArgs A{};
    A.n = n; A.S = S; A.P = (int)P; A.SH = SH;
    A.sel_list = c->sel_list.p; A.sel_h = R.sel_h.p; A.pos_of = R.pos_of.p; A.sel = c->sel.p;
    A.st_xyzm = c->st_xyzm.p; A.st_aux = c->st_aux.p; A.st_qa = c->st_qa.p; A.h_off = c->h_off.p; A.rad = c->rad.p; A.sb = c->sb.p;
    A.sb_nbr = c->sb_index_src == 1 ? c->sb_idx.p : c->blob_sb_nbr.p;
    A.bond_off = c->bond_off.p; A.bond_idx = c->bond_idx.p; A.h_xyz = c->h_xyz_d.p;
    A.sp_xyzm = c->sp_xyzm.p; A.sp_aux = c->sp_aux.p; A.sp_qa = c->sp_qa.p; A.sp_h = c->sp_h.p;
    A.start = c->sp_cnt.p + 4; A.g = c->sp_grid;
    A.r2 = cutoff * cutoff; A.comp = vdw_comp; A.include_seq_adj = include_sequence_adjacent ? 1 : 0;
    A.idbits = index_bits(c->n);
    const auto enqueue = [&](const PoseSink& sink) -> int {
        A.pxyz = R.rec.xyz.p; A.phx = R.rec.hx.p; A.out = sink;
        hipLaunchKernelGGL(k_poses_contacts, dim3((unsigned)P), dim3(POSES_THREADS), 0, c->stream, A);
        return check_launch(c, "k_poses_contacts");
    };
    CHK(pose_records_launch(c, fn, R.rec, P, xyz, (size_t)P * S * 3, h_xyz, (size_t)P * (size_t)SH * 3, 2 * A.idbits + index_bits(P), A.idbits, A.idbits,
                            enqueue, count));
    R.P = P; R.valid = true;
    return ARP_OK;
}

int arp_poses_contacts_fetch(arp_ctx* c, int64_t cap, uint64_t* pose_off, int32_t* i, int32_t* j, float* dist, uint16_t* sift,
                             uint8_t* ctype, uint32_t* summary, int64_t* count) {
    if (!c || !count) return ARP_E_ARG;
    const PosesResult& R = c->poses;
    if (!R.valid) FAIL(c, ARP_E_ARG, "arp_poses_contacts_fetch: no result (arp_poses_contacts_launch; an input or the selection changed since)");
    *count = R.rec.count;
    const bool records = i || j || dist || sift || ctype;
    if (records && R.rec.count > cap) FAIL(c, ARP_E_CAPACITY, "arp_poses_contacts_fetch: output buffers too small");
    HIPCHK(c, hipSetDevice(c->device));
    // Straight into the caller's arrays, one wait: 6 M records of 16 384 poses are 93 MB, and a second copy of them on the host (the
    // stage of the other fetches) costs this fetch more than pageable destinations do (the timing check)
    std::vector<StagePiece> pieces;
    pose_records_pieces(pieces, R.rec, R.P, records, pose_off, i, j, dist, sift, ctype, summary);
    for (const StagePiece& q : pieces)
        HIPCHK(c, hipMemcpyAsync(q.dst, q.src, q.bytes, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    return ARP_OK;
}

int arp_poses_contacts_info(arp_ctx* c, int64_t info[4]) {
    if (!c || !info) return ARP_E_ARG;
    const PosesResult& R = c->poses;
    info[0] = R.valid ? R.P : 0;
    info[1] = R.valid ? R.S : 0;
    info[2] = R.valid ? R.SH : 0;
    info[3] = R.valid ? R.rec.count : 0;
    return ARP_OK;
}

// ---- a ligand library on the resident receptor (arp_library.h): different ligands, each with its poses, one launch
// The library is a table beside the receptor: nothing of the resident structure is read to make it and a new structure leaves it
// resident.  A launch reads the receptor's static columns in the cell order of ensure_static(cutoff), the library and the
// uploaded poses; records are appended as (key, payload), sorted by every bit of the key on the result's own scratch and unpacked
// into a slab laid out as the sorted atom-atom bag is.  One wait a launch: the record count with the device's error word (the
// hydrogen rows are known to the host: no wait for SH).
static_assert(LIB_MAX_LIGANDS == ARP_LIBRARY_MAX_LIGANDS && LIB_MAX_ATOMS == ARP_LIBRARY_MAX_ATOMS, "arp_library.h names the header's limits");
const int LIB_BLOCKS_PER_CU = 4;      // the grid of k_library_contacts: min(T, this many blocks per CU), poses taken with a grid stride

int arp_set_ligand_library(arp_ctx* c, int64_t n_ligands, const int32_t* atom_off, const uint16_t* type_mask, const uint16_t* flags,
                           const double* vdw, const double* cov, const int32_t* h_off, const int32_t* sb_nbr) {
    if (!c) return ARP_E_ARG;
    const std::string fn = "arp_set_ligand_library: ";
    // ---- the refusals, in this order: none of them touches the resident library or its result
    if (c->pass_pending) FAIL(c, ARP_E_ARG, fn + "a pass has not been waited for (arp_run_wait)");
    if (n_ligands < 1 || n_ligands > LIB_MAX_LIGANDS) FAIL(c, ARP_E_ARG, fn + "1 ... ARP_LIBRARY_MAX_LIGANDS ligands");
    if (!atom_off || !type_mask || !flags || !vdw || !cov || !h_off || !sb_nbr) FAIL(c, ARP_E_ARG, fn + "an array is missing");
    const int64_t L = n_ligands;
    if (atom_off[0] != 0) FAIL(c, ARP_E_ARG, fn + "atom_off must start at 0");
    int max_atoms = 0;
    for (int64_t l = 0; l < L; ++l) {
        const int64_t S = (int64_t)atom_off[l + 1] - atom_off[l];
        if (S < 1 || S > LIB_MAX_ATOMS) FAIL(c, ARP_E_ARG, fn + "atom_off: a ligand must hold 1 ... ARP_LIBRARY_MAX_ATOMS atoms");
        max_atoms = std::max(max_atoms, (int)S);
    }
    const int64_t TA = atom_off[L];
    if (h_off[0] != 0) FAIL(c, ARP_E_ARG, fn + "h_off must start at 0");
    for (int64_t a = 0; a < TA; ++a)
        if (h_off[a + 1] < h_off[a]) FAIL(c, ARP_E_ARG, fn + "h_off must not decrease");
    for (int64_t a = 0; a < TA; ++a)
        if (!std::isfinite(vdw[a]) || !std::isfinite(cov[a]) || vdw[a] < 0 || cov[a] < 0) FAIL(c, ARP_E_ARG, fn + "radii must be finite and not negative");
    for (int64_t l = 0; l < L; ++l)
        for (int a = atom_off[l]; a < atom_off[l + 1]; ++a) {
            const int k = sb_nbr[a], S = atom_off[l + 1] - atom_off[l];
            if (k < -1 || k >= S || k == a - atom_off[l]) FAIL(c, ARP_E_ARG, fn + "sb_nbr must be -1 or the index of another atom of the same ligand");
        }
    // ---- from here on the library before is gone, and its result
    HIPCHK(c, hipSetDevice(c->device));
    void_pose_results(c, POSE_LIBRARY);
    LigandLibrary& B = c->library;
    B.resident = false;
    std::vector<double2> rad((size_t)TA);
    for (int64_t a = 0; a < TA; ++a) rad[(size_t)a] = make_double2(vdw[a], cov[a]);
    CHK(upload_async(c, B.atom_off, atom_off, (size_t)L + 1));
    CHK(upload_async(c, B.tmask, type_mask, (size_t)TA));
    CHK(upload_async(c, B.flags, flags, (size_t)TA));
    CHK(upload_async(c, B.h_off, h_off, (size_t)TA + 1));
    CHK(upload_async(c, B.sb_nbr, sb_nbr, (size_t)TA));
    CHK(upload(c, B.rad, rad.data(), (size_t)TA));      // (waits: the caller's arrays and `rad` are free after this)
    B.host_atom_off.assign(atom_off, atom_off + L + 1);
    B.host_hrows.resize((size_t)L);
    for (int64_t l = 0; l < L; ++l) B.host_hrows[(size_t)l] = h_off[atom_off[l + 1]] - h_off[atom_off[l]];
    B.L = L; B.atoms = TA; B.hrows = h_off[TA]; B.max_atoms = max_atoms; B.resident = true;
    return ARP_OK;
}

int arp_library_contacts_launch(arp_ctx* c, const int64_t* pose_off, const float* xyz, const double* h_xyz, double cutoff, double vdw_comp,
                                int include_sequence_adjacent, int64_t* count) {
    if (!c || !count) return ARP_E_ARG;
    (void)include_sequence_adjacent;      // (accepted and without effect: the gate needs M_RES_HASSEQ on both atoms, a ligand has none)
    const std::string fn = "arp_library_contacts_launch: ";
    // ---- the refusals, in this order: none of them touches a resident result
    CHK(receptor_refusals(c, fn));
    if (c->n >= POSES_MAX_N) FAIL(c, ARP_E_ARG, fn + "2^21 atoms or more (the sort key holds 21 bits of the receptor's atom id)");
    const LigandLibrary& B = c->library;
    if (!B.resident) FAIL(c, ARP_E_ARG, fn + "no ligand library (arp_set_ligand_library)");
    if (!pose_off) FAIL(c, ARP_E_ARG, fn + "pose_off missing");
    const int64_t L = B.L;
    if (pose_off[0] != 0) FAIL(c, ARP_E_ARG, fn + "pose_off must start at 0");
    for (int64_t l = 0; l < L; ++l)
        if (pose_off[l + 1] < pose_off[l]) FAIL(c, ARP_E_ARG, fn + "pose_off must not decrease");
    const int64_t T = pose_off[L];
    if (T < 1 || T > POSES_MAX_POSES) FAIL(c, ARP_E_ARG, fn + "1 ... ARP_POSES_MAX_POSES poses a launch (chunk them)");
    if (!(cutoff > 0) || !(cutoff <= ARP_POSES_MAX_CUTOFF)) FAIL(c, ARP_E_ARG, fn + "cutoff must be in (0, 6.0]");
    if (!std::isfinite(vdw_comp)) FAIL(c, ARP_E_ARG, fn + "vdw_comp is not finite");
    if (!xyz) FAIL(c, ARP_E_ARG, fn + "xyz missing");
    // where every ligand's poses begin in the two coordinate arrays (ligand-major, then pose-major), and the ligand of every pose
    std::vector<long long> tab(3 * (size_t)L + 1);
    std::vector<int> lig_of((size_t)T);
    long long nx = 0, nh = 0;
    for (int64_t l = 0; l < L; ++l) {
        const long long P = pose_off[l + 1] - pose_off[l], S = B.host_atom_off[(size_t)l + 1] - B.host_atom_off[(size_t)l];
        tab[(size_t)l] = pose_off[l];
        tab[(size_t)(L + 1 + l)] = nx;
        tab[(size_t)(2 * L + 1 + l)] = nh;
        nx += P * S * 3;
        nh += P * (long long)B.host_hrows[(size_t)l] * 3;
        std::fill(lig_of.begin() + pose_off[l], lig_of.begin() + pose_off[l + 1], (int)l);
    }
    tab[(size_t)L] = T;
    if (nh > 0 && !h_xyz) FAIL(c, ARP_E_ARG, fn + "h_xyz missing (a posed ligand has hydrogen rows)");
    HIPCHK(c, hipSetDevice(c->device));
    CHK(join_upload_lists(c));
    CHK(ensure_static(c, cutoff));
    // ---- from here on the previous result is gone, and the best-pose table made from it
    LibraryResult& R = c->libres;
    void_pose_results(c, POSE_LIBRARY_CONTACTS);
    CHK(upload_async(c, R.tab, tab.data(), tab.size()));
    CHK(upload_async(c, R.lig_of, lig_of.data(), lig_of.size()));
    LibraryArgs A{};
    A.n = (int)c->n; A.T = (int)T;
    A.atom_off = B.atom_off.p; A.tmask = B.tmask.p; A.flags = B.flags.p; A.lrad = B.rad.p; A.lh_off = B.h_off.p; A.lsb_nbr = B.sb_nbr.p;
    A.lig_of = R.lig_of.p; A.first_pose = R.tab.p; A.xyz_at = R.tab.p + L + 1; A.hx_at = R.tab.p + 2 * L + 1;
    A.rad = c->rad.p; A.sb = c->sb.p; A.h_off = c->h_off.p; A.h_xyz = c->h_xyz_d.p;
    A.sp_xyzm = c->sp_xyzm.p; A.sp_aux = c->sp_aux.p; A.sp_qa = c->sp_qa.p; A.sp_h = c->sp_h.p;
    A.start = c->sp_cnt.p + 4; A.g = c->sp_grid;
    A.r2 = cutoff * cutoff; A.comp = vdw_comp;
    A.ibits = index_bits(c->n); A.abits = index_bits(B.max_atoms);
    const unsigned blocks = (unsigned)std::min<int64_t>(T, (int64_t)LIB_BLOCKS_PER_CU * std::max(c->num_cu, 1));
    const auto enqueue = [&](const PoseSink& sink) -> int {
        A.pxyz = R.rec.xyz.p; A.phx = R.rec.hx.p; A.out = sink;
        hipLaunchKernelGGL(k_library_contacts, dim3(blocks), dim3(LIB_THREADS), 0, c->stream, A);
        return check_launch(c, "k_library_contacts");
    };
    CHK(pose_records_launch(c, fn, R.rec, T, xyz, (size_t)nx, h_xyz, (size_t)nh, A.ibits + A.abits + index_bits(T), A.ibits, A.abits, enqueue, count));
    R.L = L; R.T = T; R.blocks = (int64_t)blocks; R.nx = nx; R.host_pose_off.assign(pose_off, pose_off + L + 1); R.valid = true;
    R.cutoff = cutoff; R.vdw_comp = vdw_comp;
    return ARP_OK;
}

int arp_library_contacts_fetch(arp_ctx* c, int64_t cap, uint64_t* pose_off, int32_t* i, int32_t* a, float* dist, uint16_t* sift, uint8_t* ctype,
                               uint32_t* summary, int64_t* count) {
    if (!c || !count) return ARP_E_ARG;
    const LibraryResult& R = c->libres;
    if (!R.valid) FAIL(c, ARP_E_ARG, "arp_library_contacts_fetch: no result (arp_library_contacts_launch; the structure or the library changed since)");
    *count = R.rec.count;
    const bool records = i || a || dist || sift || ctype;
    if (records && R.rec.count > cap) FAIL(c, ARP_E_CAPACITY, "arp_library_contacts_fetch: output buffers too small");
    HIPCHK(c, hipSetDevice(c->device));
    std::vector<StagePiece> pieces;
    pose_records_pieces(pieces, R.rec, R.T, records, pose_off, i, a, dist, sift, ctype, summary);
    return stage_fetch(c, pieces);
}

int arp_library_info(arp_ctx* c, int64_t info[8]) {
    if (!c || !info) return ARP_E_ARG;
    const LigandLibrary& B = c->library;
    const LibraryResult& R = c->libres;
    info[0] = B.resident ? B.L : 0;
    info[1] = R.valid ? R.T : 0;
    info[2] = R.valid ? R.rec.count : 0;
    info[3] = B.resident ? B.atoms : 0;
    info[4] = B.resident ? B.hrows : 0;
    info[5] = R.valid ? R.blocks : 0;
    info[6] = B.resident ? B.max_atoms : 0;
    info[7] = R.best_valid ? 1 : 0;
    return ARP_OK;
}

int arp_library_best_launch(arp_ctx* c, const int32_t* weights) {
    if (!c) return ARP_E_ARG;
    const std::string fn = "arp_library_best_launch: ";
    LibraryResult& R = c->libres;
    if (c->pass_pending) FAIL(c, ARP_E_ARG, fn + "a pass has not been waited for (arp_run_wait)");
    if (!R.valid) FAIL(c, ARP_E_ARG, fn + "no library result (arp_library_contacts_launch; the structure or the library changed since)");
    if (!weights) FAIL(c, ARP_E_ARG, fn + "weights missing");
    LibraryWeights W{};
    for (int q = 0; q < POSES_SUMMARY; ++q) {
        if (weights[q] > ARP_SHORTLIST_MAX_WEIGHT || weights[q] < -ARP_SHORTLIST_MAX_WEIGHT) FAIL(c, ARP_E_ARG, fn + "weights has an entry beyond +-ARP_SHORTLIST_MAX_WEIGHT = 2^24");
        W.w[q] = weights[q];
    }
    HIPCHK(c, hipSetDevice(c->device));
    void_pose_results(c, POSE_LIBRARY_BEST);
    HIPCHK(c, R.best_n.reserve((size_t)R.L));
    HIPCHK(c, R.best_score.reserve((size_t)R.L));
    HIPCHK(c, R.best_pose.reserve((size_t)R.L));
    hipLaunchKernelGGL(k_library_best, dim3(nblocks(R.L * 64, 256, 2048)), dim3(256), 0, c->stream, (int)R.L, (const long long*)R.tab.p,
                       (const uint32_t*)R.rec.summary.p, W, R.best_n.p, R.best_pose.p, R.best_score.p);
    CHK(check_launch(c, "k_library_best"));
    R.best_valid = true;
    return ARP_OK;
}

int arp_library_best_fetch(arp_ctx* c, int64_t cap_ligands, int64_t* n_poses, int32_t* best_pose, int64_t* score, int64_t* n_ligands) {
    if (!c || !n_ligands) return ARP_E_ARG;
    const LibraryResult& R = c->libres;
    if (!R.valid || !R.best_valid) FAIL(c, ARP_E_ARG, "arp_library_best_fetch: no result (arp_library_best_launch; the library result was replaced or the structure or the library changed since)");
    *n_ligands = R.L;
    if ((n_poses || best_pose || score) && cap_ligands < R.L) FAIL(c, ARP_E_CAPACITY, "arp_library_best_fetch: output buffers too small (cap_ligands < *n_ligands)");
    HIPCHK(c, hipSetDevice(c->device));
    std::vector<StagePiece> pieces;
    want_piece(pieces, n_poses, R.best_n.p, (size_t)R.L * sizeof(int64_t));
    want_piece(pieces, best_pose, R.best_pose.p, (size_t)R.L * sizeof(int32_t));
    want_piece(pieces, score, R.best_score.p, (size_t)R.L * sizeof(int64_t));
    return stage_fetch(c, pieces);
}

// ---- ligand poses on the resident receptor, ring and amide contacts (arp_poses_planes.h)
// No bag is read and none is written.  The resident centres, normals and residues, the two centre grids and an all-atom grid of
// this result's own (by local id: ensure_static's order, which arp_poses_contacts_launch re-sorts per cutoff, is not touched) are
// read; records are appended unsorted with a key, sorted by every bit of it and gathered into four tables.  Waits: the three list
// sizes when the set-up is new, and the counters (records, error word, records per table).
static_assert(PPL_SUMMARY == ARP_POSES_PLANES_SUMMARY && PPL_MAX_RINGS == ARP_POSES_PLANES_MAX_RINGS && PPL_MAX_AMIDES == ARP_POSES_PLANES_MAX_AMIDES &&
              PPL_MAX_HOME == ARP_POSES_PLANES_MAX_HOME && PPL_MAX_NEAR == ARP_POSES_PLANES_MAX_NEAR, "arp_poses_planes.h names the header's limits");
int arp_set_plane_atoms(arp_ctx* c, const int32_t* ring_off, const int32_t* ring_idx, const int32_t* amide_atoms) {
    if (!c) return ARP_E_ARG;
    const std::string fn = "arp_set_plane_atoms: ";
    if (c->n <= 0) FAIL(c, ARP_E_ARG, fn + "no structure resident");
    if (c->models_n > 0 || c->batch_n > 0) FAIL(c, ARP_E_ARG, fn + "models or a batch are resident (one structure)");
    if ((c->nring > 0 && !ring_off) || (c->namide > 0 && !amide_atoms)) FAIL(c, ARP_E_ARG, fn + "counts differ: the resident structure has rings or amides whose atoms are missing");
    CHK(check_ring_atoms(c, "arp_set_plane_atoms", c->nring, ring_off, ring_idx, c->n));
    CHK(check_amide_atoms(c, "arp_set_plane_atoms", c->namide, amide_atoms, c->n));
    HIPCHK(c, hipSetDevice(c->device));
    PosesPlanesResult& R = c->pplanes;
    void_pose_results(c, POSE_PLANE_ATOMS);
    const int32_t zero = 0;
    const size_t nidx = c->nring > 0 ? (size_t)ring_off[c->nring] : 0;
    CHK(upload(c, R.ring_off, c->nring > 0 ? ring_off : &zero, (size_t)c->nring + 1));
    CHK(upload(c, R.ring_idx, nidx > 0 ? ring_idx : &zero, std::max<size_t>(nidx, 1)));
    CHK(upload(c, R.amide_atoms, c->namide > 0 ? amide_atoms : &zero, std::max<size_t>(4 * (size_t)c->namide, 1)));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    R.have_atoms = true;
    return ARP_OK;
}

struct PtsF4 {  // the atoms as uploaded, by local id
    const float4* p;
    __device__ __forceinline__ num::d3 get(int i) const { const float4 v = p[i]; return {(double)v.x, (double)v.y, (double)v.z}; }
};

static int poses_planes_setup(arp_ctx* c, const std::string& fn) {
    PosesPlanesResult& R = c->pplanes;
    const int n = (int)c->n, S = (int)c->nsel, nring = (int)c->nring, namide = (int)c->namide;
    const int nres = (int)std::max<int64_t>(c->nres, 1);
    HIPCHK(c, R.pos_of.reserve((size_t)n));
    HIPCHK(c, R.res_selm.reserve((size_t)nres));
    HIPCHK(c, R.hist.reserve(scan_padded(nres)));
    HIPCHK(c, R.res_off.reserve(scan_padded(nres)));
    HIPCHK(c, R.res_atoms.reserve((size_t)n));
    HIPCHK(c, R.mring.reserve(PPL_MAX_RINGS)); HIPCHK(c, R.hring.reserve(PPL_MAX_HOME)); HIPCHK(c, R.mamide.reserve(PPL_MAX_AMIDES));
    HIPCHK(c, R.ring_static.reserve((size_t)std::max(nring, 1))); HIPCHK(c, R.am_pos.reserve((size_t)std::max(namide, 1)));
    HIPCHK(c, R.cnt.reserve(4));
    HIPCHK(c, hipMemsetAsync(R.pos_of.p, 0xFF, (size_t)n * sizeof(int), c->stream));
    HIPCHK(c, hipMemsetAsync(R.res_selm.p, 0, (size_t)nres, c->stream));
    HIPCHK(c, hipMemsetAsync(R.hist.p, 0, R.hist.cap * sizeof(int), c->stream));
    HIPCHK(c, hipMemsetAsync(R.cnt.p, 0, 4 * sizeof(int), c->stream));
    hipLaunchKernelGGL(k_ppl_mark, dim3(nblocks(n, 256)), dim3(256), 0, c->stream, n, S, c->sel_list.p, c->sel.p, c->res_id.p, R.pos_of.p, R.res_selm.p, R.hist.p);
    CHK(check_launch(c, "k_ppl_mark"));
    // residue -> atoms: the scan and the scatter of the point grids (the histogram is counted down to zero again)
    CHK(enqueue_scan(c, c->stream, R.hist.p, nres, R.res_off.p, R.sums));
    hipLaunchKernelGGL(k_scatter, dim3(nblocks(n, 256)), dim3(256), 0, c->stream, n, c->res_id.p, R.res_off.p, R.hist.p, R.res_atoms.p);
    CHK(check_launch(c, "k_scatter (residue atoms)"));
    if (nring + namide > 0) {
        PplArgs A{};
        A.n = n; A.S = S; A.nring = nring; A.namide = namide;
        A.sel_list = c->sel_list.p; A.pos_of = R.pos_of.p; A.xyz = c->xyz.p; A.ring_c = c->ring_c.p;
        A.ring_off = R.ring_off.p; A.ring_idx = R.ring_idx.p; A.amide_atoms = R.amide_atoms.p;
        hipLaunchKernelGGL(k_ppl_lists, dim3(nblocks(nring + namide, 256)), dim3(256), 0, c->stream, A, R.mring.p, R.hring.p, R.mamide.p, R.ring_static.p,
                           R.am_pos.p, R.cnt.p);
        CHK(check_launch(c, "k_ppl_lists"));
    }
    // the all-atom grid of this result, cell edge 6 A, entries = local ids
    CHK(build_grid<PtsF4>(c, R.grid, PtsF4{c->xyz.p}, n, c->lo, c->hi, 6.0, nullptr));
    CHK(stage_copy(c, R.cnt.p, 4 * sizeof(int)));
    int h[4];
    memcpy(h, c->table_stage, sizeof(h));
    if (h[0] > PPL_MAX_RINGS) FAIL(c, ARP_E_ARG, fn + "more than ARP_POSES_PLANES_MAX_RINGS rings hold a movable atom");
    if (h[1] > PPL_MAX_HOME) FAIL(c, ARP_E_ARG, fn + "more than ARP_POSES_PLANES_MAX_HOME further rings have a movable atom within 3 A of their centre");
    if (h[2] > PPL_MAX_AMIDES) FAIL(c, ARP_E_ARG, fn + "more than ARP_POSES_PLANES_MAX_AMIDES amides hold a movable atom");
    R.n_mring = h[0]; R.n_hring = h[1]; R.n_mamide = h[2];
    R.setup = true;
    return ARP_OK;
}

int arp_poses_planes_launch(arp_ctx* c, int64_t n_poses, const float* xyz, int64_t counts[4]) {
    if (!c || !counts) return ARP_E_ARG;
    const std::string fn = "arp_poses_planes_launch: ";
    CHK(pose_launch_refusals(c, fn, n_poses));
    if (c->n >= POSES_MAX_N || c->nring >= POSES_MAX_N || c->namide >= POSES_MAX_N) FAIL(c, ARP_E_ARG, fn + "2^21 atoms, rings or amides, or more (the sort key holds 21 bits per id)");
    PosesPlanesResult& R = c->pplanes;
    if (!R.have_atoms) FAIL(c, ARP_E_ARG, fn + "no plane atoms (arp_set_plane_atoms after the structure, its rings and its amides)");
    if (!xyz) FAIL(c, ARP_E_ARG, fn + "xyz missing");
    CHK(check_residue_ranges(c));
    HIPCHK(c, hipSetDevice(c->device));
    CHK(join_upload_lists(c));
    CHK(ensure_static(c));               // (radius 0: the order in place stays, only missing columns are made)
    CHK(ensure_center_grids(c));
    if (!R.setup) CHK(poses_planes_setup(c, fn));
    const int n = (int)c->n, S = (int)c->nsel;
    const int64_t P = n_poses;
    // ---- from here on the previous result is gone, and what was made with it
    void_pose_results(c, POSE_PLANES);
    const int blocks = (int)std::min<int64_t>(P, PPL_MAX_BLOCKS);
    const int ws_rings = R.n_mring + R.n_hring + PPL_MAX_NEAR;
    HIPCHK(c, R.xyz.reserve((size_t)P * S * 3));
    HIPCHK(c, hipMemcpyAsync(R.xyz.p, xyz, (size_t)P * S * 3 * sizeof(float), hipMemcpyHostToDevice, c->stream));
    HIPCHK(c, R.ws_ring.reserve((size_t)blocks * ws_rings));
    HIPCHK(c, R.ws_amide.reserve((size_t)blocks * std::max(R.n_mamide, 1)));
    PplArgs A{};
    A.n = n; A.S = S; A.P = (int)P; A.nring = (int)c->nring; A.namide = (int)c->namide;
    A.sel_list = c->sel_list.p; A.pos_of = R.pos_of.p; A.sel = c->sel.p; A.pxyz = R.xyz.p;
    A.ring_off = R.ring_off.p; A.ring_idx = R.ring_idx.p; A.amide_atoms = R.amide_atoms.p;
    A.mring = R.mring.p; A.hring = R.hring.p; A.mamide = R.mamide.p;
    A.n_mring = R.n_mring; A.n_hring = R.n_hring; A.n_mamide = R.n_mamide;
    A.ring_static = R.ring_static.p; A.am_pos = R.am_pos.p; A.res_selm = R.res_selm.p; A.res_off = R.res_off.p; A.res_atoms = R.res_atoms.p;
    A.xyz = c->xyz.p; A.st_xyzm = c->st_xyzm.p; A.res_id = c->res_id.p;
    A.ring_c = c->ring_c.p; A.ring_n = c->ring_n.p; A.ring_res = c->ring_res.p;
    A.am_c = c->am_c.p; A.am_n = c->am_n.p; A.am_res = c->am_res.p;
    A.ga = R.grid.d; A.a_start = R.grid.start.p; A.a_perm = R.grid.perm.p;
    if (c->nring > 0) { A.gr = c->ring_grid.d; A.r_start = c->ring_grid.start.p; A.r_perm = c->ring_grid.perm.p; }
    if (c->namide > 0) { A.gm = c->amide_grid.d; A.m_start = c->amide_grid.start.p; A.m_perm = c->amide_grid.perm.p; }
    A.ws_ring = R.ws_ring.p; A.ws_amide = R.ws_amide.p; A.ws_rings = ws_rings;
    A.idbits = index_bits(std::max({c->n, c->nring, c->namide})); A.pbits = index_bits(P);
    const auto enqueue = [&](const PlaneSink& sink) {
        A.rec = sink.rec; A.key = sink.key; A.val = sink.val; A.cap = sink.cap; A.ctr = R.ctr.p; A.summary = R.summary.p;
        hipLaunchKernelGGL(k_poses_planes, dim3((unsigned)blocks), dim3(PPL_THREADS), 0, c->stream, A);
    };
    CHK(plane_records_launch(c, fn, PlaneRecords{R.rec, R.ctr, R.pose_off, R.summary, R.sort, R.slab, R.col, R.counts, R.launches}, P,
                             2 + A.pbits + 2 * A.idbits, "k_poses_planes", "a pose brings more than ARP_POSES_PLANES_MAX_NEAR further rings within 3 A of a movable atom",
                             enqueue, counts));
    R.P = P; R.S = S; R.valid = true;
    return ARP_OK;
}

int arp_poses_planes_fetch(arp_ctx* c, int table, int64_t cap, uint64_t* pose_off, int32_t* first, int32_t* second, void* v0, void* v1, void* v2,
                           void* v3, uint8_t* u0, uint8_t* u1, uint8_t* u2, uint32_t* summary, int64_t* count) {
    if (!c || !count) return ARP_E_ARG;
    const PosesPlanesResult& R = c->pplanes;
    if (!R.valid) FAIL(c, ARP_E_ARG, "arp_poses_planes_fetch: no result (arp_poses_planes_launch; an input, the selection or the plane atoms changed since)");
    if (table < 0 || table > 3) FAIL(c, ARP_E_ARG, "arp_poses_planes_fetch: table must be ARP_POSES_PLANES_ATOM_PLANE ... ARP_POSES_PLANES_GROUP_PLANE");
    const int t = table;
    *count = R.counts[t];
    void* const v[4] = {v0, v1, v2, v3};
    uint8_t* const u[3] = {u0, u1, u2};
    bool records = false;
    CHK(plane_fetch_columns(c, "arp_poses_planes_fetch: ", t, first, second, v, u, &records));
    if (records && R.counts[t] > cap) FAIL(c, ARP_E_CAPACITY, "arp_poses_planes_fetch: output buffers too small");
    HIPCHK(c, hipSetDevice(c->device));
    std::vector<StagePiece> pieces;
    want_piece(pieces, pose_off, R.pose_off.p + (size_t)t * ((size_t)R.P + 1), ((size_t)R.P + 1) * sizeof(unsigned long long));
    want_piece(pieces, summary, R.summary.p, (size_t)R.P * PPL_SUMMARY * sizeof(uint32_t));
    if (records) plane_fetch_pieces(pieces, R.col, t, (size_t)R.counts[t], first, second, v, u);
    return stage_fetch(c, pieces);
}

int arp_poses_planes_info(arp_ctx* c, int64_t info[12]) {
    if (!c || !info) return ARP_E_ARG;
    const PosesPlanesResult& R = c->pplanes;
    info[0] = R.valid ? R.P : 0;
    info[1] = R.valid ? R.S : 0;
    for (int t = 0; t < 4; ++t) info[2 + t] = R.valid ? R.counts[t] : 0;
    info[6] = R.setup ? R.n_mring : 0;
    info[7] = R.setup ? R.n_hring : 0;
    info[8] = R.setup ? R.n_mamide : 0;
    info[9] = R.have_atoms ? 1 : 0;
    info[10] = R.launches;
    info[11] = 0;
    return ARP_OK;
}

// ---- a ligand library on the resident receptor, ring and amide contacts (arp_library_planes.h)
// No bag is read and none is written, and no selection.  The receptor's resident centres, normals and residues, the two centre
// grids and an all-atom grid of this result's own (by local id, for the reason of arp_poses_planes_launch) are read beside the
// library and its plane table; records are appended unsorted with a key, sorted by every bit of it and gathered into four
// tables.  One wait a launch: the counters (records, error word, records per table).
static_assert(LPL_MAX_RINGS == ARP_LIBRARY_PLANES_MAX_RINGS && LPL_MAX_AMIDES == ARP_LIBRARY_PLANES_MAX_AMIDES, "arp_library_planes.h names the header's limits");

int arp_set_ligand_library_planes(arp_ctx* c, const int32_t* ring_off, const int32_t* ring_atom_off, const int32_t* ring_atom_idx,
                                  const int32_t* amide_off, const int32_t* amide_atoms) {
    if (!c) return ARP_E_ARG;
    const std::string fn = "arp_set_ligand_library_planes: ";
    // ---- the refusals, in this order: none of them touches the resident table or a result
    if (c->pass_pending) FAIL(c, ARP_E_ARG, fn + "a pass has not been waited for (arp_run_wait)");
    const LigandLibrary& B = c->library;
    if (!B.resident) FAIL(c, ARP_E_ARG, fn + "no ligand library (arp_set_ligand_library)");
    const int64_t L = B.L;
    if (!ring_off || !ring_atom_off || !amide_off || (ring_off[L] > 0 && !ring_atom_idx) || (amide_off[L] > 0 && !amide_atoms))
        FAIL(c, ARP_E_ARG, fn + "an array is missing");
    if (!csr_ok(ring_off, L)) FAIL(c, ARP_E_ARG, fn + "ring_off must start at 0 and never decrease");
    const int64_t TR = ring_off[L];
    if (!csr_ok(ring_atom_off, TR)) FAIL(c, ARP_E_ARG, fn + "ring_atom_off must start at 0 and never decrease");
    if (!csr_ok(amide_off, L)) FAIL(c, ARP_E_ARG, fn + "amide_off must start at 0 and never decrease");
    const int64_t TM = amide_off[L];
    for (int64_t l = 0; l < L; ++l) {
        if (ring_off[l + 1] - ring_off[l] > LPL_MAX_RINGS) FAIL(c, ARP_E_ARG, fn + "a ligand has more than ARP_LIBRARY_PLANES_MAX_RINGS rings");
        if (amide_off[l + 1] - amide_off[l] > LPL_MAX_AMIDES) FAIL(c, ARP_E_ARG, fn + "a ligand has more than ARP_LIBRARY_PLANES_MAX_AMIDES amides");
    }
    for (int64_t r = 0; r < TR; ++r)
        if (ring_atom_off[r + 1] - ring_atom_off[r] < 3) FAIL(c, ARP_E_ARG, fn + "a ring needs at least three atoms");
    for (int64_t l = 0; l < L; ++l) {
        const int S = B.host_atom_off[(size_t)l + 1] - B.host_atom_off[(size_t)l];
        for (int64_t k = ring_atom_off[ring_off[l]]; k < ring_atom_off[ring_off[l + 1]]; ++k)
            if (ring_atom_idx[k] < 0 || ring_atom_idx[k] >= S) FAIL(c, ARP_E_ARG, fn + "ring atom index outside its own ligand");
        for (int64_t k = 4 * (int64_t)amide_off[l]; k < 4 * (int64_t)amide_off[l + 1]; ++k)
            if ((k & 3) != 3 && (amide_atoms[k] < 0 || amide_atoms[k] >= S)) FAIL(c, ARP_E_ARG, fn + "amide atom index outside its own ligand");
    }
    // ---- from here on the table before is gone, and its result
    HIPCHK(c, hipSetDevice(c->device));
    void_pose_results(c, POSE_LIBRARY_PLANE_ATOMS);
    LibraryPlaneAtoms& P = c->libplanes;
    const int32_t zero[4] = {0, 0, 0, 0};
    const size_t nidx = (size_t)ring_atom_off[TR];
    CHK(upload_async(c, P.ring_off, ring_off, (size_t)L + 1));
    CHK(upload_async(c, P.ring_atom_off, ring_atom_off, (size_t)TR + 1));
    CHK(upload_async(c, P.ring_atom_idx, nidx > 0 ? ring_atom_idx : zero, std::max<size_t>(nidx, 1)));
    CHK(upload_async(c, P.amide_off, amide_off, (size_t)L + 1));
    CHK(upload(c, P.amide_atoms, TM > 0 ? amide_atoms : zero, std::max<size_t>(4 * (size_t)TM, 4)));      // (waits: the caller's arrays are free after this)
    P.L = L; P.TR = TR; P.TM = TM; P.resident = true;
    return ARP_OK;
}

static int library_planes_setup(arp_ctx* c) {
    LibraryPlanesResult& R = c->libpl;
    const int n = (int)c->n;
    const int nres = (int)std::max<int64_t>(c->nres, 1);
    HIPCHK(c, R.hist.reserve(scan_padded(nres)));
    HIPCHK(c, R.res_off.reserve(scan_padded(nres)));
    HIPCHK(c, R.res_atoms.reserve((size_t)n));
    HIPCHK(c, hipMemsetAsync(R.hist.p, 0, R.hist.cap * sizeof(int), c->stream));
    hipLaunchKernelGGL(k_lpl_hist, dim3(nblocks(n, 256)), dim3(256), 0, c->stream, n, c->res_id.p, R.hist.p);
    CHK(check_launch(c, "k_lpl_hist"));
    // residue -> atoms: the scan and the scatter of the point grids (the histogram is counted down to zero again)
    CHK(enqueue_scan(c, c->stream, R.hist.p, nres, R.res_off.p, R.sums));
    hipLaunchKernelGGL(k_scatter, dim3(nblocks(n, 256)), dim3(256), 0, c->stream, n, c->res_id.p, R.res_off.p, R.hist.p, R.res_atoms.p);
    CHK(check_launch(c, "k_scatter (residue atoms)"));
    // the all-atom grid of this result, cell edge 6 A, entries = local ids
    CHK(build_grid<PtsF4>(c, R.grid, PtsF4{c->xyz.p}, n, c->lo, c->hi, 6.0, nullptr));
    R.setup = true;
    return ARP_OK;
}

int arp_library_planes_launch(arp_ctx* c, const int64_t* pose_off, const float* xyz, int64_t counts[4]) {
    if (!c || !counts) return ARP_E_ARG;
    const std::string fn = "arp_library_planes_launch: ";
    // ---- the refusals, in this order: none of them touches a resident result
    CHK(receptor_refusals(c, fn));
    if (c->n + LIB_MAX_ATOMS >= POSES_MAX_N || c->nring + LPL_MAX_RINGS >= POSES_MAX_N || c->namide + LPL_MAX_AMIDES >= POSES_MAX_N)
        FAIL(c, ARP_E_ARG, fn + "2^21 atoms, rings or amides of the complex, or more (the sort key holds 21 bits per id)");
    const LigandLibrary& B = c->library;
    if (!B.resident) FAIL(c, ARP_E_ARG, fn + "no ligand library (arp_set_ligand_library)");
    const LibraryPlaneAtoms& PA = c->libplanes;
    if (!PA.resident) FAIL(c, ARP_E_ARG, fn + "no library plane table (arp_set_ligand_library_planes after the library)");
    if (!pose_off) FAIL(c, ARP_E_ARG, fn + "pose_off missing");
    const int64_t L = B.L;
    if (pose_off[0] != 0) FAIL(c, ARP_E_ARG, fn + "pose_off must start at 0");
    for (int64_t l = 0; l < L; ++l)
        if (pose_off[l + 1] < pose_off[l]) FAIL(c, ARP_E_ARG, fn + "pose_off must not decrease");
    const int64_t T = pose_off[L];
    if (T < 1 || T > POSES_MAX_POSES) FAIL(c, ARP_E_ARG, fn + "1 ... ARP_POSES_MAX_POSES poses a launch (chunk them)");
    if (!xyz) FAIL(c, ARP_E_ARG, fn + "xyz missing");
    // (the ligand's residue is the receptor's residue count: without a residue table it would coincide with residue 0 of the atoms)
    if (c->nres < 1) FAIL(c, ARP_E_ARG, fn + "no residue table resident (arp_set_residues): the ligand is one more residue behind the receptor's");
    CHK(check_residue_ranges(c));
    // where every ligand's poses begin in the coordinate array (ligand-major, then pose-major), and the ligand of every pose
    std::vector<long long> tab(2 * (size_t)L + 1);
    std::vector<int> lig_of((size_t)T);
    long long nx = 0;
    for (int64_t l = 0; l < L; ++l) {
        const long long P = pose_off[l + 1] - pose_off[l], S = B.host_atom_off[(size_t)l + 1] - B.host_atom_off[(size_t)l];
        tab[(size_t)l] = pose_off[l];
        tab[(size_t)(L + 1 + l)] = nx;
        nx += P * S * 3;
        std::fill(lig_of.begin() + pose_off[l], lig_of.begin() + pose_off[l + 1], (int)l);
    }
    tab[(size_t)L] = T;
    HIPCHK(c, hipSetDevice(c->device));
    CHK(join_upload_lists(c));
    CHK(ensure_static(c));               // (radius 0: the order in place stays, only missing columns are made)
    CHK(ensure_center_grids(c));
    LibraryPlanesResult& R = c->libpl;
    if (!R.setup) CHK(library_planes_setup(c));
    // ---- from here on the previous result is gone
    void_pose_results(c, POSE_LIBRARY_PLANES);
    const int blocks = (int)std::min<int64_t>(T, (int64_t)LIB_BLOCKS_PER_CU * std::max(c->num_cu, 1));
    CHK(upload_async(c, R.tab, tab.data(), tab.size()));
    CHK(upload_async(c, R.lig_of, lig_of.data(), lig_of.size()));
    HIPCHK(c, R.xyz.reserve(std::max<size_t>((size_t)nx, 1)));
    HIPCHK(c, hipMemcpyAsync(R.xyz.p, xyz, (size_t)nx * sizeof(float), hipMemcpyHostToDevice, c->stream));
    HIPCHK(c, R.ws_ring.reserve((size_t)blocks * LPL_WS_RINGS));
    HIPCHK(c, R.ws_amide.reserve((size_t)blocks * LPL_MAX_AMIDES));
    LplArgs A{};
    A.n = (int)c->n; A.T = (int)T; A.nring = (int)c->nring; A.namide = (int)c->namide; A.nres = (int)c->nres;
    A.atom_off = B.atom_off.p; A.tmask = B.tmask.p; A.flags = B.flags.p; A.lh_off = B.h_off.p; A.lsb_nbr = B.sb_nbr.p;
    A.lring_off = PA.ring_off.p; A.lring_atom_off = PA.ring_atom_off.p; A.lring_atom_idx = PA.ring_atom_idx.p;
    A.lamide_off = PA.amide_off.p; A.lamide_atoms = PA.amide_atoms.p;
    A.lig_of = R.lig_of.p; A.first_pose = R.tab.p; A.xyz_at = R.tab.p + L + 1; A.pxyz = R.xyz.p;
    A.res_off = R.res_off.p; A.res_atoms = R.res_atoms.p;
    A.xyz = c->xyz.p; A.st_xyzm = c->st_xyzm.p; A.res_id = c->res_id.p;
    A.ring_c = c->ring_c.p; A.ring_n = c->ring_n.p; A.ring_res = c->ring_res.p;
    A.am_c = c->am_c.p; A.am_n = c->am_n.p; A.am_res = c->am_res.p;
    A.ga = R.grid.d; A.a_start = R.grid.start.p; A.a_perm = R.grid.perm.p;
    if (c->nring > 0) { A.gr = c->ring_grid.d; A.r_start = c->ring_grid.start.p; A.r_perm = c->ring_grid.perm.p; }
    if (c->namide > 0) { A.gm = c->amide_grid.d; A.m_start = c->amide_grid.start.p; A.m_perm = c->amide_grid.perm.p; }
    A.ws_ring = R.ws_ring.p; A.ws_amide = R.ws_amide.p;
    A.idbits = index_bits(std::max({c->n + LIB_MAX_ATOMS, c->nring + LPL_MAX_RINGS, c->namide + LPL_MAX_AMIDES})); A.pbits = index_bits(T);
    const auto enqueue = [&](const PlaneSink& sink) {
        A.rec = sink.rec; A.key = sink.key; A.val = sink.val; A.cap = sink.cap; A.ctr = R.ctr.p; A.summary = R.summary.p;
        hipLaunchKernelGGL(k_library_planes, dim3((unsigned)blocks), dim3(LPL_THREADS), 0, c->stream, A);
    };
    CHK(plane_records_launch(c, fn, PlaneRecords{R.rec, R.ctr, R.pose_off, R.summary, R.sort, R.slab, R.col, R.counts, R.launches}, T,
                             2 + A.pbits + 2 * A.idbits, "k_library_planes", "a pose brings more than ARP_POSES_PLANES_MAX_NEAR receptor rings within 3 A of a ligand atom",
                             enqueue, counts));
    R.L = L; R.T = T; R.blocks = blocks; R.nx = nx; R.host_pose_off.assign(pose_off, pose_off + L + 1); R.valid = true;
    return ARP_OK;
}

int arp_library_planes_fetch(arp_ctx* c, int table, int64_t cap, uint64_t* pose_off, int32_t* first, int32_t* second, void* v0, void* v1, void* v2,
                             void* v3, uint8_t* u0, uint8_t* u1, uint8_t* u2, uint32_t* summary, int64_t* count) {
    if (!c || !count) return ARP_E_ARG;
    const LibraryPlanesResult& R = c->libpl;
    if (!R.valid) FAIL(c, ARP_E_ARG, "arp_library_planes_fetch: no result (arp_library_planes_launch; the structure, the library or its plane table changed since)");
    if (table < 0 || table > 3) FAIL(c, ARP_E_ARG, "arp_library_planes_fetch: table must be ARP_POSES_PLANES_ATOM_PLANE ... ARP_POSES_PLANES_GROUP_PLANE");
    const int t = table;
    *count = R.counts[t];
    void* const v[4] = {v0, v1, v2, v3};
    uint8_t* const u[3] = {u0, u1, u2};
    bool records = false;
    CHK(plane_fetch_columns(c, "arp_library_planes_fetch: ", t, first, second, v, u, &records));
    if (records && R.counts[t] > cap) FAIL(c, ARP_E_CAPACITY, "arp_library_planes_fetch: output buffers too small");
    HIPCHK(c, hipSetDevice(c->device));
    std::vector<StagePiece> pieces;
    want_piece(pieces, pose_off, R.pose_off.p + (size_t)t * ((size_t)R.T + 1), ((size_t)R.T + 1) * sizeof(unsigned long long));
    want_piece(pieces, summary, R.summary.p, (size_t)R.T * PPL_SUMMARY * sizeof(uint32_t));
    if (records) plane_fetch_pieces(pieces, R.col, t, (size_t)R.counts[t], first, second, v, u);
    return stage_fetch(c, pieces);
}

int arp_library_planes_info(arp_ctx* c, int64_t info[12]) {
    if (!c || !info) return ARP_E_ARG;
    const LibraryPlaneAtoms& P = c->libplanes;
    const LibraryPlanesResult& R = c->libpl;
    info[0] = P.resident ? P.L : 0;
    info[1] = P.resident ? P.TR : 0;
    info[2] = P.resident ? P.TM : 0;
    info[3] = R.valid ? R.T : 0;
    for (int t = 0; t < 4; ++t) info[4 + t] = R.valid ? R.counts[t] : 0;
    info[8] = R.valid ? R.blocks : 0;
    info[9] = R.launches;
    info[10] = P.resident ? 1 : 0;
    info[11] = R.setup ? 1 : 0;
    return ARP_OK;
}

// ---- pose fingerprints (arp_poses_fingerprints.h): the resident poses result -> bit matrix -> scores
// Only the poses result is read (its sorted slab, pose_off, pos_of) and res_id — with class planes (5r) also the poses-planes
// result's four tables, offsets and set-up tables —; only this result's own buffers are written.
// Nothing is sorted: the columns come from a presence bitmap of the nodes.  One wait: U, which sizes the matrix.
static_assert(POSEFP_PLANES == ARP_POSEFP_PLANES && POSEFP_PLANES == TABLE_SIFT_BITS && POSEFP_MAX_REFS == ARP_POSEFP_MAX_REFS &&
              POSEFP_BY_RESIDUE == ARP_POSEFP_BY_RESIDUE && POSEFP_ALL_PAIRS == ARP_POSEFP_ALL_PAIRS && POSEFP_MAX_REFS == POSEFP_TILE &&
              POSEFP_TILE == SIM_TILE && POSEFP_KC == SIM_KC, "arp_poses_fingerprints.h names the header's limits and k_sim_gram's panel");
// the class planes: the four tables of the poses-planes result are read as well, and nothing of it is written
static_assert(POSEFP_ALL_PLANES == ARP_POSEFP_ALL_PLANES && POSEFP_PLANE_AP_ATOM == ARP_POSEFP_PLANES &&
              POSEFP_PLANE_GP_RING == ARP_POSEFP_ALL_PLANES - 1 && (ARP_AP_METSULPHURPI >> (POSEFP_AP_BITS - 1)) == 1u,
              "arp_poses_fingerprints.h names the header's planes");

// word slices of a popcount product over W words whose tiles number `tiles`: as many as fill the device, a slice no shorter
// than one staged panel (the rule of arp_models_similarity_launch)
static void popcount_slices(const arp_ctx* c, long long W, long long tiles, long long* per, long long* slices) {
    const long long chunks = (W + SIM_KC - 1) / SIM_KC;
    const long long want = std::max<long long>(1, std::min<long long>(chunks, (2ll * c->num_cu + tiles - 1) / tiles));
    *per = (chunks + want - 1) / want * SIM_KC;
    *slices = (W + *per - 1) / *per;
}

static void posefp_info(const PoseFpResult& F, int64_t info[8]) {
    const int64_t v[8] = {F.P, F.Q, F.U, F.NP, F.W, F.slices, F.launches, (int64_t)F.flags};
    for (int q = 0; q < 8; ++q) info[q] = (F.valid || q == 6) ? v[q] : 0;
}

// What both fingerprint launches (poses, library) enqueue over a finished bit matrix of A.P rows whose first A.Q are the
// references (A.bits, A.W; F.count and F.cross reserved): k_pfp_cross and k_pfp_occupancy.  *slices: the word slices of the first.
static int enqueue_cross_and_occupancy(arp_ctx* c, PoseFpResult& F, PoseFpArgs& A, long long* slices) {
    const long long P = A.P, Q = A.Q, W = A.W;
    // ---- cross = B R^T and count: the pose tiles times as many word slices as fill the device
    const long long tiles = (P + POSEFP_TILE - 1) / POSEFP_TILE;
    long long per = 0;
    popcount_slices(c, W, tiles, &per, slices);
    A.per = per; A.slices = (int)*slices;
    if (*slices > 1) {
        HIPCHK(c, hipMemsetAsync(F.count.p, 0, (size_t)P * sizeof(uint32_t), c->stream));
        if (Q > 0) HIPCHK(c, hipMemsetAsync(F.cross.p, 0, (size_t)(P * Q) * sizeof(uint32_t), c->stream));
    }
    hipLaunchKernelGGL(k_pfp_cross, dim3((unsigned)tiles, (unsigned)*slices), dim3(256), 0, c->stream, A);
    // ---- occupancy: column sums over the poses behind the references, the pose tiles cut into as many slices as fill the device
    const long long chunks = (W + POSEFP_KC - 1) / POSEFP_KC;
    // (a block keeps at least eight pose tiles where there are that many: its sums stay in registers, and fewer blocks meet on
    // a counter at the end)
    const long long pose_slices = std::max<long long>(1, std::min<long long>((tiles + 7) / 8, (2ll * c->num_cu + chunks - 1) / chunks));
    A.occ_tiles = (int)((tiles + pose_slices - 1) / pose_slices);
    hipLaunchKernelGGL(k_pfp_occupancy, dim3((unsigned)chunks, (unsigned)((tiles + A.occ_tiles - 1) / A.occ_tiles)), dim3(256), 0, c->stream, A);
    return ARP_OK;
}

// Both entries: arp_poses_fingerprints_launch admits the 15 SIFt bits and reads the poses result alone; with a bit from
// ARP_POSEFP_PLANES on (arp_poses_fingerprints_planes_launch) the four tables of the poses-planes result are
// marked and walked as well, after a check on the device that both results were made from the same pose coordinates — its flag
// comes back with U, in the one wait.
static int posefp_launch(arp_ctx* c, const std::string& fn, int n_planes, uint32_t planes, uint32_t ctype_mask, uint32_t flags, int64_t n_refs,
                         int64_t info[8]) {
    PoseFpResult& F = c->posefp;
    const PosesResult& R = c->poses;
    const PosesPlanesResult& L = c->pplanes;
    const bool classes = (planes >> ARP_POSEFP_PLANES) != 0;
    if (c->pass_pending) FAIL(c, ARP_E_ARG, fn + "a pass has not been waited for (arp_run_wait)");
    CHK(need_poses_result(c, fn));
    if (n_planes == ARP_POSEFP_PLANES && (planes & ~((1u << ARP_POSEFP_PLANES) - 1u))) FAIL(c, ARP_E_ARG, fn + "planes has bits beyond the 15 SIFt bits");
    if (planes & ~((1u << ARP_POSEFP_ALL_PLANES) - 1u)) FAIL(c, ARP_E_ARG, fn + "planes has bits beyond the 29 planes (15 SIFt bits, 14 ring / amide classes)");
    if (!planes) FAIL(c, ARP_E_ARG, fn + "a planes mask of 0 makes no feature");
    if (ctype_mask & ~ARP_FILTER_CTYPE_ALL) FAIL(c, ARP_E_ARG, fn + "ctype_mask has bits beyond the 7 contact types");
    if (!ctype_mask) FAIL(c, ARP_E_ARG, fn + "a ctype_mask of 0 admits no record");
    if (flags & ~(ARP_POSEFP_BY_RESIDUE | ARP_POSEFP_ALL_PAIRS)) FAIL(c, ARP_E_ARG, fn + "unknown flag");
    const int64_t P = R.P, Q = n_refs;
    if (Q < 0 || Q > ARP_POSEFP_MAX_REFS || Q > P) FAIL(c, ARP_E_ARG, fn + "n_refs must be 0 ... min(ARP_POSEFP_MAX_REFS, poses of the launch)");
    const bool by_res = (flags & ARP_POSEFP_BY_RESIDUE) != 0, all_pairs = (flags & ARP_POSEFP_ALL_PAIRS) != 0;
    if (by_res && (!c->has_res || c->nres <= 0)) FAIL(c, ARP_E_ARG, fn + "no residues resident (ARP_POSEFP_BY_RESIDUE)");
    if (all_pairs && P > ARP_SIM_MAX_MODELS) FAIL(c, ARP_E_CAPACITY, fn + "ARP_POSEFP_ALL_PAIRS with more than ARP_SIM_MAX_MODELS = 4096 poses (the matrix would pass 64 MiB)");
    if (classes) {
        if (!by_res) FAIL(c, ARP_E_ARG, fn + "ring / amide class planes need ARP_POSEFP_BY_RESIDUE (their nodes are residues)");
        CHK(need_planes_result_of_same_poses(c, fn));
    }
    if (F.valid && F.planes == planes && F.ctype_mask == ctype_mask && F.flags == flags && F.Q == Q) { posefp_info(F, info); return ARP_OK; }
    void_pose_results(c, POSE_FINGERPRINT);
    F.classes = classes;
    HIPCHK(c, hipSetDevice(c->device));
    const int64_t N = by_res ? c->nres : c->n, NW = (N + 63) / 64;
    const int NP = __builtin_popcount(planes);
    const size_t k = (size_t)R.rec.count;
    HIPCHK(c, F.presence.reserve((size_t)NW));
    HIPCHK(c, F.base.reserve((size_t)NW));
    HIPCHK(c, F.total.reserve(2));      // U; the same-poses flag
    HIPCHK(c, F.count.reserve((size_t)P));
    HIPCHK(c, F.cross.reserve(std::max<size_t>((size_t)(P * Q), 1)));
    if (all_pairs) HIPCHK(c, F.inter.reserve((size_t)(P * P)));
    PoseFpArgs A{};
    const uint8_t* const slab = R.rec.slab.p;
    A.ci = (const int*)(slab + R.rec.off[0]); A.cj = (const int*)(slab + R.rec.off[1]);
    A.sift = (const uint16_t*)(slab + R.rec.off[3]); A.ctype = slab + R.rec.off[4];
    A.pose_off = R.rec.pose_off.p; A.pos_of = R.pos_of.p; A.res_id = c->res_id.p;
    A.k = (long long)k; A.P = (int)P; A.Q = (int)Q; A.N = N; A.by_res = by_res ? 1 : 0;
    A.planes = planes; A.ctype_mask = ctype_mask;
    A.presence = F.presence.p; A.base = F.base.p; A.NW = NW; A.total = F.total.p;
    A.NP = NP; A.count = F.count.p; A.cross = F.cross.p;
    const auto done = [&](long long U, long long W, long long slices) {
        F.P = P; F.Q = Q; F.U = U; F.NP = NP; F.W = W; F.slices = slices;
        F.planes = planes; F.ctype_mask = ctype_mask; F.flags = flags;
        F.valid = true;
        ++F.launches;
        posefp_info(F, info);
        return ARP_OK;
    };
    // ---- the ring / amide tables (class planes): the poses-planes result's columns, offsets and set-up tables
    PoseFpTables T{};
    int64_t k_classes = 0;
    if (classes) {
        for (int t = 0; t < 4; ++t) {
            T.first[t] = L.col.i0[t]; T.second[t] = L.col.i1[t]; T.ctype[t] = L.col.u[t][PLANE_TABLES[t].ctype_col];
            T.count[t] = L.counts[t];
            k_classes = std::max(k_classes, L.counts[t]);
        }
        T.ap_mask = L.col.u[0][0];
        T.pose_off = L.pose_off.p;
        T.pos_of = L.pos_of.p; T.ring_static = L.ring_static.p; T.am_pos = L.am_pos.p;
        T.ring_off = L.ring_off.p; T.ring_idx = L.ring_idx.p; T.am_res = c->am_res.p;
        T.n = (int)c->n; T.nring = (int)c->nring; T.namide = (int)c->namide;
    }
    // ---- the columns: presence bitmap of the nodes, popcounts, scan; the host learns U (the one wait)
    long long U = 0;
    if (k > 0 || classes) {
        HIPCHK(c, hipMemsetAsync(F.presence.p, 0, (size_t)NW * sizeof(unsigned long long), c->stream));
        if (classes) HIPCHK(c, hipMemsetAsync(F.total.p + 1, 0, sizeof(long long), c->stream));
        // (a block a CU: the threads that run first all see their bit unset and OR; the fewer they are, the fewer ORs queue up
        // on the few words around the ligand — those behind them read the bit and skip)
        if (k > 0) hipLaunchKernelGGL(k_pfp_mark, dim3(nblocks((int64_t)k, 256, c->num_cu)), dim3(256), 0, c->stream, A);
        if (classes) {
            enqueue_same_poses(c, F.total.p + 1);
            if (k_classes > 0) hipLaunchKernelGGL(k_pfp_mark_planes, dim3(nblocks(k_classes, 256, c->num_cu), 4), dim3(256), 0, c->stream, A, T);
        }
        hipLaunchKernelGGL(k_pfp_scan, dim3(1), dim3(POSEFP_SCAN_THREADS), 0, c->stream, A);
        CHK(check_launch(c, (fn + "mark / scan").c_str()));
        CHK(stage_copy(c, F.total.p, 2 * sizeof(long long)));
        long long h[2];
        memcpy(h, c->table_stage, sizeof(h));
        if (classes && h[1] != 0) FAIL(c, ARP_E_ARG, fn + "the poses result and the poses-planes result were made from different poses");
        U = h[0];
        if (U < 0 || U > N) FAIL(c, ARP_E_HIP, fn + "column count out of range");
    }
    if (U == 0) {      // no participating record: no column, no feature in any pose
        HIPCHK(c, hipMemsetAsync(F.count.p, 0, (size_t)P * sizeof(uint32_t), c->stream));
        if (Q > 0) HIPCHK(c, hipMemsetAsync(F.cross.p, 0, (size_t)(P * Q) * sizeof(uint32_t), c->stream));
        if (all_pairs) HIPCHK(c, hipMemsetAsync(F.inter.p, 0, (size_t)(P * P) * sizeof(uint32_t), c->stream));
        return done(0, 0, 0);
    }
    // ---- the bit matrix: NP planes of ceil(U / 64) words a pose, OR-ed into zeroed memory by a wave per pose
    const long long wpp = (U + 63) / 64, W = (long long)NP * wpp;
    if ((long long)NP * U >= (1ll << 32)) FAIL(c, ARP_E_CAPACITY, fn + "2^32 features or more (a count would not fit uint32)");
    if (P * W >= (1ll << 29)) FAIL(c, ARP_E_CAPACITY, fn + "a bit matrix of 4 GiB or more (launch fewer poses)");
    HIPCHK(c, F.ids.reserve((size_t)U));
    HIPCHK(c, F.occ.reserve((size_t)(U * NP)));
    HIPCHK(c, F.bits.reserve((size_t)(P * W)));
    HIPCHK(c, hipMemsetAsync(F.bits.p, 0, (size_t)(P * W) * sizeof(unsigned long long), c->stream));
    HIPCHK(c, hipMemsetAsync(F.occ.p, 0, (size_t)(U * NP) * sizeof(uint32_t), c->stream));
    A.ids = F.ids.p; A.U = U; A.bits = F.bits.p; A.wpp = wpp; A.W = W; A.occ = F.occ.p;
    hipLaunchKernelGGL(k_pfp_ids, dim3(nblocks(NW, 256, 1024)), dim3(256), 0, c->stream, A);
    if (k > 0) hipLaunchKernelGGL(k_pfp_bits, dim3(nblocks(P, 4, 16384)), dim3(256), 0, c->stream, A);
    if (k_classes > 0) hipLaunchKernelGGL(k_pfp_bits_planes, dim3(nblocks(P, 4, 16384)), dim3(256), 0, c->stream, A, T);
    const long long tiles = (P + POSEFP_TILE - 1) / POSEFP_TILE;
    long long slices = 0;
    CHK(enqueue_cross_and_occupancy(c, F, A, &slices));
    // ---- all pairs: k_sim_gram on this matrix, the poses as its models
    if (all_pairs) {
        SimArgs G{};
        const long long pairs = tiles * (tiles + 1) / 2;
        long long gper = 0, gslices = 0;
        popcount_slices(c, W, pairs, &gper, &gslices);
        G.F = (uint32_t)P; G.bits = F.bits.p; G.wpp = wpp; G.W = W; G.per = gper; G.slices = (int)gslices; G.tiles = (int)tiles;
        G.inter = F.inter.p;
        if (gslices > 1) HIPCHK(c, hipMemsetAsync(F.inter.p, 0, (size_t)(P * P) * sizeof(uint32_t), c->stream));
        hipLaunchKernelGGL(k_sim_gram, dim3((unsigned)pairs, (unsigned)gslices), dim3(256), 0, c->stream, G);
    }
    CHK(check_launch(c, (fn + "ids / bits / cross / occupancy").c_str()));
    return done(U, W, slices);
}

int arp_poses_fingerprints_launch(arp_ctx* c, uint32_t planes, uint32_t ctype_mask, uint32_t flags, int64_t n_refs, int64_t info[8]) {
    if (!c || !info) return ARP_E_ARG;
    return posefp_launch(c, "arp_poses_fingerprints_launch: ", ARP_POSEFP_PLANES, planes, ctype_mask, flags, n_refs, info);
}

int arp_poses_fingerprints_planes_launch(arp_ctx* c, uint32_t planes29, uint32_t ctype_mask, uint32_t flags, int64_t n_refs, int64_t info[8]) {
    if (!c || !info) return ARP_E_ARG;
    return posefp_launch(c, "arp_poses_fingerprints_planes_launch: ", ARP_POSEFP_ALL_PLANES, planes29, ctype_mask, flags, n_refs, info);
}

int arp_poses_fingerprints_fetch(arp_ctx* c, int64_t cap_nodes, int32_t* ids, uint32_t* count, uint32_t* cross, uint32_t* occupancy,
                                 uint64_t* bits, uint32_t* inter, int64_t* n_nodes) {
    if (!c || !n_nodes) return ARP_E_ARG;
    const PoseFpResult& F = c->posefp;
    if (!F.valid)      // (voided wherever the poses result is)
        FAIL(c, ARP_E_ARG, "arp_poses_fingerprints_fetch: no result (arp_poses_fingerprints_launch; the poses result was replaced or an input or the selection changed since)");
    *n_nodes = F.U;
    if ((ids || occupancy || bits) && F.U > cap_nodes) FAIL(c, ARP_E_CAPACITY, "arp_poses_fingerprints_fetch: output buffers too small (cap_nodes < *n_nodes)");
    if (inter && !(F.flags & ARP_POSEFP_ALL_PAIRS)) FAIL(c, ARP_E_ARG, "arp_poses_fingerprints_fetch: no all-pairs matrix (launch with ARP_POSEFP_ALL_PAIRS)");
    HIPCHK(c, hipSetDevice(c->device));
    CHK(download_async(c, ids, (const int32_t*)F.ids.p, (size_t)F.U));
    CHK(download_async(c, count, (const uint32_t*)F.count.p, (size_t)F.P));
    CHK(download_async(c, cross, (const uint32_t*)F.cross.p, (size_t)(F.P * F.Q)));
    CHK(download_async(c, occupancy, (const uint32_t*)F.occ.p, (size_t)(F.U * F.NP)));
    CHK(download_async(c, (unsigned long long*)bits, (const unsigned long long*)F.bits.p, (size_t)(F.P * F.W)));
    CHK(download_async(c, inter, (const uint32_t*)F.inter.p, (size_t)(F.P * F.P)));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    return ARP_OK;
}

int arp_poses_fingerprints_info(arp_ctx* c, int64_t info[8]) {
    if (!c || !info) return ARP_E_ARG;
    posefp_info(c->posefp, info);
    return ARP_OK;
}

// ---- library fingerprints (arp_library_fingerprints.h): the resident library result -> bit matrix -> scores
// Only the library result is read (its sorted slab, pose_off, the ligands' pose ranges) and res_id — with class planes (5z) also
// the library-planes result's four tables and offsets and the receptor's ring_res and am_res —; only this result's own
// buffers are written.  The references are the caller's feature lists: rows 0 ... Q - 1 of a matrix of Q + T rows, so that
// k_pfp_scan, k_pfp_ids, k_pfp_cross and k_pfp_occupancy are launched as they are.  One wait: U, which sizes the matrix.
static_assert(LIBFP_MAX_FEATURES == ARP_LIBFP_MAX_FEATURES, "arp_library_fingerprints.h names the header's limit");
// Both entries: arp_library_fingerprints_launch admits the 15 SIFt bits (n_planes) and reads the library result alone; with a bit
// from ARP_POSEFP_PLANES on (arp_library_fingerprints_planes_launch) the four tables of the library-planes result
// are marked and walked as well, after a check on the device that both results were made from the same pose coordinates — its
// flag comes back with U, in the one wait.
static int libfp_launch(arp_ctx* c, const std::string& fn, int n_planes, uint32_t planes, uint32_t ctype_mask, uint32_t flags, int64_t n_refs,
                        const int64_t* ref_off, const int32_t* ref_node, const uint32_t* ref_planes, int64_t info[8]) {
    PoseFpResult& F = c->libfp;
    LibraryFpTables& X = c->libfpx;
    const LibraryResult& R = c->libres;
    const LibraryPlanesResult& L = c->libpl;
    const bool wide = n_planes > ARP_POSEFP_PLANES;
    const bool classes = wide && (planes >> ARP_POSEFP_PLANES) != 0;
    // ---- the refusals, in this order: none of them touches a resident result
    if (c->pass_pending) FAIL(c, ARP_E_ARG, fn + "a pass has not been waited for (arp_run_wait)");
    if (!R.valid) FAIL(c, ARP_E_ARG, fn + "no library result (arp_library_contacts_launch; the structure or the library changed since)");
    if (classes) {
        if (!L.valid) FAIL(c, ARP_E_ARG, fn + "no library-planes result (arp_library_planes_launch; the structure, the library or its plane table changed since)");
        // (equal T with other pose ranges is refused here as well: the check on the device compares R.nx words of both)
        if (L.T != R.T || L.L != R.L || L.host_pose_off != R.host_pose_off || L.nx != R.nx)
            FAIL(c, ARP_E_ARG, fn + "the library result and the library-planes result differ in T or in their pose ranges (launch both on the same poses)");
        if (!(flags & ARP_POSEFP_BY_RESIDUE)) FAIL(c, ARP_E_ARG, fn + "ring / amide class planes need ARP_POSEFP_BY_RESIDUE (their nodes are residues)");
    }
    if (!planes) FAIL(c, ARP_E_ARG, fn + "a planes mask of 0 makes no feature");
    if (!wide && (planes & ~((1u << ARP_POSEFP_PLANES) - 1u))) FAIL(c, ARP_E_ARG, fn + "planes has bits beyond the 15 SIFt bits");
    if (planes & ~((1u << ARP_POSEFP_ALL_PLANES) - 1u)) FAIL(c, ARP_E_ARG, fn + "planes has bits beyond the 29 planes (15 SIFt bits, 14 ring / amide classes)");
    if (!ctype_mask) FAIL(c, ARP_E_ARG, fn + "a ctype_mask of 0 admits no record");
    if (ctype_mask & ~ARP_FILTER_CTYPE_ALL) FAIL(c, ARP_E_ARG, fn + "ctype_mask has bits beyond the 7 contact types");
    if (flags & ~ARP_POSEFP_BY_RESIDUE) FAIL(c, ARP_E_ARG, fn + "unknown flag (ARP_POSEFP_BY_RESIDUE is the only one)");
    const bool by_res = (flags & ARP_POSEFP_BY_RESIDUE) != 0;
    if (by_res && (!c->has_res || c->nres <= 0)) FAIL(c, ARP_E_ARG, fn + "no residues resident (ARP_POSEFP_BY_RESIDUE)");
    const int64_t Q = n_refs, T = R.T, P = Q + T;
    if (Q < 0 || Q > ARP_POSEFP_MAX_REFS) FAIL(c, ARP_E_ARG, fn + "n_refs must be 0 ... ARP_POSEFP_MAX_REFS");
    if (Q > 0 && (!ref_off || !ref_node || !ref_planes)) FAIL(c, ARP_E_ARG, fn + "a reference array is missing");
    const int64_t N = by_res ? c->nres : c->n, NW = (N + 63) / 64;
    int64_t nf = 0;
    if (Q > 0) {
        if (ref_off[0] != 0) FAIL(c, ARP_E_ARG, fn + "ref_off must start at 0");
        for (int64_t q = 0; q < Q; ++q)
            if (ref_off[q + 1] < ref_off[q]) FAIL(c, ARP_E_ARG, fn + "ref_off must not decrease");
        nf = ref_off[Q];
        if (nf > ARP_LIBFP_MAX_FEATURES) FAIL(c, ARP_E_ARG, fn + "more than ARP_LIBFP_MAX_FEATURES reference features");
        for (int64_t f = 0; f < nf; ++f)
            if (ref_node[f] < 0 || (int64_t)ref_node[f] >= N) FAIL(c, ARP_E_ARG, fn + "a reference node outside [0, nodes of the level)");
        for (int64_t q = 0; q < Q; ++q)
            for (int64_t f = ref_off[q] + 1; f < ref_off[q + 1]; ++f)
                if (ref_node[f] <= ref_node[f - 1]) FAIL(c, ARP_E_ARG, fn + "the nodes of a reference must be strictly ascending");
        for (int64_t f = 0; f < nf; ++f) {
            if (!wide && (ref_planes[f] & ~((1u << ARP_POSEFP_PLANES) - 1u))) FAIL(c, ARP_E_ARG, fn + "a reference mask has bits beyond the 15 SIFt bits");
            if (ref_planes[f] & ~((1u << ARP_POSEFP_ALL_PLANES) - 1u)) FAIL(c, ARP_E_ARG, fn + "a reference mask has bits beyond the 29 planes");
        }
    }
    const int NP = __builtin_popcount(planes);
    // ---- from here on the fingerprint before is gone, and its best-pose table
    void_pose_results(c, POSE_LIBRARY_FINGERPRINT);
    F.classes = classes;
    HIPCHK(c, hipSetDevice(c->device));
    const size_t k = (size_t)R.rec.count;
    HIPCHK(c, F.presence.reserve((size_t)NW));
    HIPCHK(c, F.base.reserve((size_t)NW));
    HIPCHK(c, F.total.reserve(2));
    HIPCHK(c, F.count.reserve((size_t)P));
    HIPCHK(c, F.cross.reserve(std::max<size_t>((size_t)(P * Q), 1)));
    LibFpRefs V{};
    if (Q > 0) {
        CHK(upload_async(c, X.ref_off, (const long long*)ref_off, (size_t)Q + 1));
        CHK(upload_async(c, X.ref_node, (const int*)ref_node, (size_t)nf));
        CHK(upload_async(c, X.ref_planes, ref_planes, (size_t)nf));
        V.ref_off = X.ref_off.p; V.ref_node = X.ref_node.p; V.ref_planes = X.ref_planes.p; V.F = nf;
    }
    PoseFpArgs A{};
    const uint8_t* const slab = R.rec.slab.p;
    if (k > 0) {
        A.ci = (const int*)(slab + R.rec.off[0]);      // (the ligand side, column 1, names no node: not read)
        A.sift = (const uint16_t*)(slab + R.rec.off[3]); A.ctype = slab + R.rec.off[4];
    }
    A.pose_off = R.rec.pose_off.p; A.res_id = c->res_id.p;
    A.k = (long long)k; A.P = (int)P; A.Q = (int)Q; A.N = N; A.by_res = by_res ? 1 : 0;
    A.planes = planes; A.ctype_mask = ctype_mask;
    A.presence = F.presence.p; A.base = F.base.p; A.NW = NW; A.total = F.total.p;
    A.NP = NP; A.count = F.count.p; A.cross = F.cross.p;
    const auto done = [&](long long U, long long W, long long slices) {
        F.P = P; F.Q = Q; F.U = U; F.NP = NP; F.W = W; F.slices = slices;
        F.planes = planes; F.ctype_mask = ctype_mask; F.flags = flags;
        F.valid = true;
        X.L = R.L; X.features = nf;
        ++F.launches;
        posefp_info(F, info);
        return ARP_OK;
    };
    // ---- the ring / amide tables (class planes): the library-planes result's columns and offsets, the receptor's resident
    // ring and amide residues
    LibFpTables Tb{};
    int64_t k_classes = 0;
    if (classes) {
        for (int t = 0; t < 4; ++t) {
            Tb.first[t] = L.col.i0[t]; Tb.second[t] = L.col.i1[t]; Tb.ctype[t] = L.col.u[t][PLANE_TABLES[t].ctype_col];
            Tb.count[t] = L.counts[t];
            k_classes = std::max(k_classes, L.counts[t]);
        }
        Tb.ap_mask = L.col.u[0][0];
        Tb.pose_off = L.pose_off.p;
        Tb.ring_res = c->ring_res.p; Tb.am_res = c->am_res.p;
        Tb.n = (int)c->n; Tb.nring = (int)c->nring; Tb.namide = (int)c->namide;
        Tb.T = T;
    }
    // ---- the columns: presence bitmap of the nodes of records and references, popcounts, scan; the host learns U (the one wait,
    // after which the caller's reference arrays are free)
    long long U = 0;
    if (k > 0 || Q > 0 || classes) {
        HIPCHK(c, hipMemsetAsync(F.presence.p, 0, (size_t)NW * sizeof(unsigned long long), c->stream));
        if (classes) HIPCHK(c, hipMemsetAsync(F.total.p + 1, 0, sizeof(long long), c->stream));
        if (k + (size_t)nf > 0) hipLaunchKernelGGL(k_lfp_mark, dim3(nblocks((int64_t)k + nf, 256, c->num_cu)), dim3(256), 0, c->stream, A, V);
        if (classes) {
            // both results keep their uploaded poses: compared as 32-bit words, the flag word beside U
            if (R.nx > 0)
                hipLaunchKernelGGL(k_pfp_same_poses, dim3(nblocks(R.nx, 256, c->num_cu)), dim3(256), 0, c->stream, (const uint32_t*)R.rec.xyz.p,
                                   (const uint32_t*)L.xyz.p, (long long)R.nx, (uint32_t*)(F.total.p + 1));
            if (k_classes > 0) hipLaunchKernelGGL(k_lfp_mark_planes, dim3(nblocks(k_classes, 256, c->num_cu), 4), dim3(256), 0, c->stream, A, Tb);
        }
        hipLaunchKernelGGL(k_pfp_scan, dim3(1), dim3(POSEFP_SCAN_THREADS), 0, c->stream, A);
        CHK(check_launch(c, (fn + "mark / scan").c_str()));
        CHK(stage_copy(c, F.total.p, (classes ? 2 : 1) * sizeof(long long)));
        long long h[2] = {0, 0};
        memcpy(h, c->table_stage, (classes ? 2 : 1) * sizeof(long long));
        if (classes && h[1] != 0) FAIL(c, ARP_E_ARG, fn + "the library result and the library-planes result were made from different poses");
        U = h[0];
        if (U < 0 || U > N) FAIL(c, ARP_E_HIP, fn + "column count out of range");
    }
    if (U == 0) {      // no participating record and no reference feature: no column, no feature in any row
        HIPCHK(c, hipMemsetAsync(F.count.p, 0, (size_t)P * sizeof(uint32_t), c->stream));
        if (Q > 0) HIPCHK(c, hipMemsetAsync(F.cross.p, 0, (size_t)(P * Q) * sizeof(uint32_t), c->stream));
        return done(0, 0, 0);
    }
    // ---- the bit matrix: NP planes of ceil(U / 64) words a row, OR-ed into zeroed memory by a wave per row
    // (the two capacity limits of the pose fingerprints, over Q + T rows: they need U, so they come after the wait and leave no
    // fingerprint resident)
    const long long wpp = (U + 63) / 64, W = (long long)NP * wpp;
    if ((long long)NP * U >= (1ll << 32)) FAIL(c, ARP_E_CAPACITY, fn + "2^32 features or more (a count would not fit uint32)");
    if (P * W >= (1ll << 29)) FAIL(c, ARP_E_CAPACITY, fn + "a bit matrix of 4 GiB or more (launch fewer poses)");
    HIPCHK(c, F.ids.reserve((size_t)U));
    HIPCHK(c, F.occ.reserve((size_t)(U * NP)));
    HIPCHK(c, F.bits.reserve((size_t)(P * W)));
    HIPCHK(c, hipMemsetAsync(F.bits.p, 0, (size_t)(P * W) * sizeof(unsigned long long), c->stream));
    HIPCHK(c, hipMemsetAsync(F.occ.p, 0, (size_t)(U * NP) * sizeof(uint32_t), c->stream));
    A.ids = F.ids.p; A.U = U; A.bits = F.bits.p; A.wpp = wpp; A.W = W; A.occ = F.occ.p;
    hipLaunchKernelGGL(k_pfp_ids, dim3(nblocks(NW, 256, 1024)), dim3(256), 0, c->stream, A);
    hipLaunchKernelGGL(k_lfp_bits, dim3(nblocks(P, 4, 16384)), dim3(256), 0, c->stream, A, V);
    if (k_classes > 0) hipLaunchKernelGGL(k_lfp_bits_planes, dim3(nblocks(T, 4, 16384)), dim3(256), 0, c->stream, A, Tb);
    long long slices = 0;
    CHK(enqueue_cross_and_occupancy(c, F, A, &slices));
    CHK(check_launch(c, (fn + "ids / bits / cross / occupancy").c_str()));
    return done(U, W, slices);
}

int arp_library_fingerprints_launch(arp_ctx* c, uint32_t planes, uint32_t ctype_mask, uint32_t flags, int64_t n_refs, const int64_t* ref_off,
                                    const int32_t* ref_node, const uint32_t* ref_planes, int64_t info[8]) {
    if (!c || !info) return ARP_E_ARG;
    return libfp_launch(c, "arp_library_fingerprints_launch: ", ARP_POSEFP_PLANES, planes, ctype_mask, flags, n_refs, ref_off, ref_node, ref_planes, info);
}

int arp_library_fingerprints_planes_launch(arp_ctx* c, uint32_t planes29, uint32_t ctype_mask, uint32_t flags, int64_t n_refs, const int64_t* ref_off,
                                           const int32_t* ref_node, const uint32_t* ref_planes, int64_t info[8]) {
    if (!c || !info) return ARP_E_ARG;
    return libfp_launch(c, "arp_library_fingerprints_planes_launch: ", ARP_POSEFP_ALL_PLANES, planes29, ctype_mask, flags, n_refs, ref_off, ref_node,
                        ref_planes, info);
}

int arp_library_fingerprints_fetch(arp_ctx* c, int64_t cap_nodes, int32_t* ids, uint32_t* count, uint32_t* cross, uint32_t* occupancy, uint64_t* bits,
                                   int64_t* n_nodes) {
    if (!c || !n_nodes) return ARP_E_ARG;
    const PoseFpResult& F = c->libfp;
    if (!F.valid)
        FAIL(c, ARP_E_ARG, "arp_library_fingerprints_fetch: no result (arp_library_fingerprints_launch; the library result was replaced or the structure or the library changed since)");
    *n_nodes = F.U;
    if ((ids || occupancy || bits) && F.U > cap_nodes) FAIL(c, ARP_E_CAPACITY, "arp_library_fingerprints_fetch: output buffers too small (cap_nodes < *n_nodes)");
    HIPCHK(c, hipSetDevice(c->device));
    std::vector<StagePiece> pieces;
    want_piece(pieces, ids, F.ids.p, (size_t)F.U * sizeof(int32_t));
    want_piece(pieces, count, F.count.p, (size_t)F.P * sizeof(uint32_t));
    want_piece(pieces, cross, F.cross.p, (size_t)(F.P * F.Q) * sizeof(uint32_t));
    want_piece(pieces, occupancy, F.occ.p, (size_t)(F.U * F.NP) * sizeof(uint32_t));
    // (the bit matrix, the one large piece, goes straight to the caller's array, as arp_poses_fingerprints_fetch copies it)
    CHK(download_async(c, (unsigned long long*)bits, (const unsigned long long*)F.bits.p, (size_t)(F.P * F.W)));
    return stage_fetch(c, pieces);
}

int arp_library_fingerprints_info(arp_ctx* c, int64_t info[8]) {
    if (!c || !info) return ARP_E_ARG;
    posefp_info(c->libfp, info);
    return ARP_OK;
}

int arp_library_fingerprints_best_launch(arp_ctx* c) {
    if (!c) return ARP_E_ARG;
    const std::string fn = "arp_library_fingerprints_best_launch: ";
    const PoseFpResult& F = c->libfp;
    LibraryFpTables& X = c->libfpx;
    const LibraryResult& R = c->libres;
    if (c->pass_pending) FAIL(c, ARP_E_ARG, fn + "a pass has not been waited for (arp_run_wait)");
    if (!F.valid || !R.valid) FAIL(c, ARP_E_ARG, fn + "no library fingerprint (arp_library_fingerprints_launch; the library result was replaced or the structure or the library changed since)");
    if (F.Q < 1) FAIL(c, ARP_E_ARG, fn + "the library fingerprint has no reference (n_refs = 0)");
    HIPCHK(c, hipSetDevice(c->device));
    void_pose_results(c, POSE_LIBRARY_FP_BEST);
    const size_t L = (size_t)R.L, LQ = L * (size_t)F.Q;
    HIPCHK(c, X.best_n.reserve(L));
    HIPCHK(c, X.best_pose.reserve(LQ));
    HIPCHK(c, X.best_q32.reserve(LQ));
    HIPCHK(c, X.best_shared.reserve(LQ));
    HIPCHK(c, X.best_count.reserve(LQ));
    LibFpBest B{};
    B.L = (int)R.L; B.Q = (int)F.Q; B.Qp = 1;
    while (B.Qp < B.Q) B.Qp <<= 1;
    B.pose_off = R.tab.p; B.count = F.count.p; B.cross = F.cross.p;
    B.n_poses = X.best_n.p; B.best_pose = X.best_pose.p; B.q32 = X.best_q32.p; B.shared = X.best_shared.p; B.best_count = X.best_count.p;
    hipLaunchKernelGGL(k_lfp_best, dim3(nblocks(R.L * 64, 256, 2048)), dim3(256), 0, c->stream, B);
    CHK(check_launch(c, "k_lfp_best"));
    X.L = R.L;
    X.best_valid = true;
    return ARP_OK;
}

int arp_library_fingerprints_best_fetch(arp_ctx* c, int64_t cap_ligands, int64_t* n_poses, int32_t* best_pose, int64_t* tanimoto_q32, uint32_t* shared,
                                        uint32_t* count, int64_t* n_ligands, int64_t* n_refs) {
    if (!c || !n_ligands || !n_refs) return ARP_E_ARG;
    const PoseFpResult& F = c->libfp;
    const LibraryFpTables& X = c->libfpx;
    if (!F.valid || !X.best_valid)
        FAIL(c, ARP_E_ARG, "arp_library_fingerprints_best_fetch: no result (arp_library_fingerprints_best_launch; the library fingerprint was replaced or the library result, the structure or the library changed since)");
    *n_ligands = X.L;
    *n_refs = F.Q;
    if ((n_poses || best_pose || tanimoto_q32 || shared || count) && cap_ligands < X.L)
        FAIL(c, ARP_E_CAPACITY, "arp_library_fingerprints_best_fetch: output buffers too small (cap_ligands < *n_ligands)");
    HIPCHK(c, hipSetDevice(c->device));
    const size_t L = (size_t)X.L, LQ = L * (size_t)F.Q;
    std::vector<StagePiece> pieces;
    want_piece(pieces, n_poses, X.best_n.p, L * sizeof(int64_t));
    want_piece(pieces, best_pose, X.best_pose.p, LQ * sizeof(int32_t));
    want_piece(pieces, tanimoto_q32, X.best_q32.p, LQ * sizeof(int64_t));
    want_piece(pieces, shared, X.best_shared.p, LQ * sizeof(uint32_t));
    want_piece(pieces, count, X.best_count.p, LQ * sizeof(uint32_t));
    return stage_fetch(c, pieces);
}

// ---- pose shortlist (arp_poses_shortlist.h): the resident poses result -> ranked poses -> the chosen ones' records
// The poses result, and depending on the arguments the poses-planes result and the fingerprint result, are read; only this
// result's own buffers are written (its sort scratch included: PosesResult::sort keeps the source's sorted buffers).  One wait:
// K, the five totals, the same-poses flag and the device's error word, which size the columns the gather then fills.
static_assert(PSL_LIST == ARP_SHORTLIST_LIST && PSL_SUMMARY == ARP_SHORTLIST_SUMMARY && PSL_TANIMOTO == ARP_SHORTLIST_TANIMOTO &&
              PSL_TABLES == ARP_SHORTLIST_TABLES && PSL_SLOTS == POSES_SUMMARY && PSL_SLOTS == PPL_SUMMARY &&
              PSL_MAX_WEIGHT == ARP_SHORTLIST_MAX_WEIGHT && PSL_CTYPES_ALL == ARP_FILTER_CTYPE_ALL, "arp_poses_shortlist.h names the header's constants");

static void shortlist_info(const ShortlistResult& S, int64_t info[8]) {
    const int64_t v[8] = {S.K, S.total[0], S.total[1], S.total[2], S.total[3], S.total[4], S.launches, (int64_t)S.kind};
    for (int q = 0; q < 8; ++q) info[q] = (S.valid || q == 6) ? v[q] : 0;
}

// the checks of tables and the record filter that both shortlist launches make, in this order
static int shortlist_filter_refusals(arp_ctx* c, const std::string& fn, uint32_t tables, uint32_t sift_mask, uint32_t ctype_mask) {
    if (!tables || (tables & ~((1u << ARP_SHORTLIST_TABLES) - 1u))) FAIL(c, ARP_E_ARG, fn + "tables must be a non-zero mask of the five tables");
    if (sift_mask & ~ARP_FILTER_SIFT_ALL) FAIL(c, ARP_E_ARG, fn + "sift_mask has bits beyond the 15 SIFt bits");
    if (ctype_mask & ~ARP_FILTER_CTYPE_ALL) FAIL(c, ARP_E_ARG, fn + "ctype_mask has bits beyond the 7 contact types");
    if (!ctype_mask) FAIL(c, ARP_E_ARG, fn + "a ctype_mask of 0 keeps no record");
    return ARP_OK;
}

// What the pose shortlist and the library shortlist share once their refusals are through and the previous shortlist is void:
// A names the sources, the score's arguments, the threshold and the filter; this fills in the result.  `ids`: the caller's list
// (kind LIST), else `score` enqueues the keys and payloads of the M ranked candidates into A.key / A.val.  `same_poses` (when the
// planes source is read) enqueues the comparison into the flag word; `riders` is enqueued once the candidates stand (A.skey /
// A.sval or A.ids).  One wait.
struct ShortlistSteps {
    std::function<void(void*)> same_poses;
    std::function<void(const PslArgs&)> score, riders;
    const char* differ;
};
static int shortlist_make(arp_ctx* c, const std::string& fn, ShortlistResult& S, PslArgs& A, const int32_t* ids, int64_t M, int64_t ncand,
                          const ShortlistSteps& steps) {
    HIPCHK(c, hipSetDevice(c->device));
    const bool list = A.kind == PSL_LIST;
    HIPCHK(c, S.words.reserve(8));
    HIPCHK(c, S.pose.reserve((size_t)ncand));
    HIPCHK(c, S.score.reserve((size_t)ncand));
    HIPCHK(c, S.summary.reserve((size_t)ncand * PSL_SLOTS));
    HIPCHK(c, S.pl_summary.reserve((size_t)ncand * PSL_SLOTS));
    HIPCHK(c, S.len.reserve((size_t)ncand * PSL_TABLES));
    HIPCHK(c, S.off.reserve(((size_t)ncand + 1) * PSL_TABLES));
    A.ncand = (int)ncand;
    A.pose = S.pose.p; A.score = S.score.p; A.out_summary = S.summary.p; A.out_pl_summary = S.pl_summary.p;
    A.len = S.len.p; A.off = S.off.p; A.words = S.words.p;
    HIPCHK(c, hipMemsetAsync(S.words.p, 0, 8 * sizeof(unsigned long long), c->stream));
    if (S.planes) steps.same_poses(S.words.p + PSL_W_DIFFER);
    if (list) {
        CHK(upload_async(c, S.ids, (const int*)ids, (size_t)ncand));      // (the wait below is before the caller's array goes away)
        A.ids = S.ids.p;
    } else {
        // ---- score and rank: keys of all 64 bits, stable, so that ties stay in ascending pose
        CHK(reserve_key_sort(c, S.sort, (size_t)M, (size_t)M));
        A.key = S.sort.key[0].p; A.val = S.sort.val[0].p;
        steps.score(A);
        int sorted = 0;
        enqueue_key_sort(c, S.sort, (size_t)M, 64, &sorted);
        A.skey = S.sort.key[sorted].p; A.sval = S.sort.val[sorted].p;
    }
    // ---- lengths, offsets, and the one wait
    hipLaunchKernelGGL(k_psl_lengths, dim3(nblocks(ncand, 4, 4096), PSL_TABLES), dim3(256), 0, c->stream, A);
    hipLaunchKernelGGL(k_psl_offsets, dim3(PSL_TABLES), dim3(1024), 0, c->stream, A);
    if (steps.riders) steps.riders(A);
    CHK(check_launch(c, (fn + "score / sort / lengths / offsets").c_str()));
    CHK(stage_copy(c, S.words.p, 8 * sizeof(unsigned long long)));
    unsigned long long h[8];
    memcpy(h, c->table_stage, sizeof(h));
    ++S.launches;
    if (S.planes && h[PSL_W_DIFFER] != 0) FAIL(c, ARP_E_ARG, fn + steps.differ);
    if (h[PSL_W_ERR] != 0) FAIL(c, ARP_E_HIP, fn + "device error (a pose id out of range)");
    if (h[PSL_W_K] > (unsigned long long)ncand) FAIL(c, ARP_E_HIP, fn + "chosen count out of range");
    for (int t = 0; t < PSL_TABLES; ++t)
        if (h[PSL_W_TOTAL + t] >= (1ull << 31)) FAIL(c, ARP_E_CAPACITY, fn + "a table of 2^31 records or more (a smaller k)");
    // ---- the columns of the requested tables in one slab: atom-atom as the sorted slab is laid out, the others as the
    // poses-planes result lays out its own
    size_t bytes = 0;
    sorted_layout((size_t)h[PSL_W_TOTAL], S.aa_off, &bytes, (size_t)h[PSL_W_TOTAL]);
    const size_t m[4] = {(size_t)h[PSL_W_TOTAL + 1], (size_t)h[PSL_W_TOTAL + 2], (size_t)h[PSL_W_TOTAL + 3], (size_t)h[PSL_W_TOTAL + 4]};
    const PlaneLayout lay = plane_tables_layout(m, bytes, &bytes);
    HIPCHK(c, S.slab.reserve(std::max<size_t>(bytes, 256)));
    const PplColumns col = bind_plane_columns(S.slab.p, lay);
    const Columns aa{S.slab.p, S.aa_off};
    A.oi = aa[0]; A.oj = aa[1]; A.od = aa[2]; A.os = aa[3]; A.oct = aa[4];
    A.opl = col;
    int64_t all = 0;
    for (int t = 0; t < PSL_TABLES; ++t) { A.total[t] = (long long)h[PSL_W_TOTAL + t]; all += A.total[t]; }
    if (all > 0) {
        hipLaunchKernelGGL(k_psl_gather, dim3(nblocks(ncand, 4, 4096), PSL_TABLES), dim3(256), 0, c->stream, A);
        CHK(check_launch(c, (fn + "gather").c_str()));
    }
    S.col = col;
    S.K = (int64_t)h[PSL_W_K]; S.ncand = ncand; S.kind = A.kind; S.tables = A.tables;
    for (int t = 0; t < PSL_TABLES; ++t) S.total[t] = A.total[t];
    S.valid = true;
    return ARP_OK;
}

int arp_poses_shortlist_launch(arp_ctx* c, int kind, const int32_t* weights32, int64_t ref, const int32_t* pose_ids, int64_t n_ids, int64_t skip,
                               int64_t k, int64_t min_score, uint32_t tables, uint32_t sift_mask, uint32_t ctype_mask, int64_t info[8]) {
    if (!c || !info) return ARP_E_ARG;
    const std::string fn = "arp_poses_shortlist_launch: ";
    ShortlistResult& S = c->shortlist;
    const PosesResult& R = c->poses;
    const PosesPlanesResult& L = c->pplanes;
    const PoseFpResult& F = c->posefp;
    // ---- the refusals: none of them touches a resident result
    if (c->pass_pending) FAIL(c, ARP_E_ARG, fn + "a pass has not been waited for (arp_run_wait)");
    CHK(need_poses_result(c, fn));
    if (kind != ARP_SHORTLIST_LIST && kind != ARP_SHORTLIST_SUMMARY && kind != ARP_SHORTLIST_TANIMOTO)
        FAIL(c, ARP_E_ARG, fn + "unknown kind (ARP_SHORTLIST_LIST, ARP_SHORTLIST_SUMMARY or ARP_SHORTLIST_TANIMOTO)");
    const int64_t P = R.P;
    CHK(shortlist_filter_refusals(c, fn, tables, sift_mask, ctype_mask));
    bool planes = (tables >> 1) != 0;
    if (kind == ARP_SHORTLIST_LIST) {
        if (!pose_ids) FAIL(c, ARP_E_ARG, fn + "pose_ids missing (ARP_SHORTLIST_LIST)");
        if (n_ids < 1 || n_ids > ARP_POSES_MAX_POSES) FAIL(c, ARP_E_ARG, fn + "n_ids must be 1 ... ARP_POSES_MAX_POSES");
        if (skip != 0 || k != 0 || min_score != INT64_MIN) FAIL(c, ARP_E_ARG, fn + "ARP_SHORTLIST_LIST takes skip = 0, k = 0 and min_score = INT64_MIN (the list is the choice)");
        for (int64_t q = 0; q < n_ids; ++q)
            if (pose_ids[q] < 0 || pose_ids[q] >= P) FAIL(c, ARP_E_ARG, fn + "pose_ids has an id outside [0, P)");
    } else {
        if (skip < 0 || skip >= P) FAIL(c, ARP_E_ARG, fn + "skip must be in [0, P)");
        if (k < 1) FAIL(c, ARP_E_ARG, fn + "k must be at least 1");
    }
    if (kind == ARP_SHORTLIST_SUMMARY) {
        if (!weights32) FAIL(c, ARP_E_ARG, fn + "weights missing (ARP_SHORTLIST_SUMMARY)");
        for (int q = 0; q < 2 * PSL_SLOTS; ++q) {
            if (weights32[q] > ARP_SHORTLIST_MAX_WEIGHT || weights32[q] < -ARP_SHORTLIST_MAX_WEIGHT) FAIL(c, ARP_E_ARG, fn + "weights has an entry beyond +-ARP_SHORTLIST_MAX_WEIGHT = 2^24");
            if (q >= PSL_SLOTS && weights32[q] != 0) planes = true;
        }
    }
    if (kind == ARP_SHORTLIST_TANIMOTO) {
        if (!F.valid) FAIL(c, ARP_E_ARG, fn + "no fingerprint result (arp_poses_fingerprints_launch; ARP_SHORTLIST_TANIMOTO)");
        if (F.Q < 1) FAIL(c, ARP_E_ARG, fn + "the fingerprint result has no references (n_refs = 0)");
        if (F.P != P) FAIL(c, ARP_E_ARG, fn + "the fingerprint result and the poses result differ in P");
        if (ref < -1 || ref >= F.Q) FAIL(c, ARP_E_ARG, fn + "ref must be -1 or in [0, n_refs)");
    }
    if (planes) CHK(need_planes_result_of_same_poses(c, fn));
    // ---- from here on the previous shortlist is gone
    void_pose_results(c, POSE_SHORTLIST);
    S.planes = planes;
    const bool list = kind == ARP_SHORTLIST_LIST;
    const int64_t M = P - skip, ncand = list ? n_ids : std::min(k, M);
    PslArgs A{};
    const uint8_t* const slab = R.rec.slab.p;      // (no record: the columns are never read, every segment is empty)
    if (R.rec.count > 0) {
        A.ci = (const int*)(slab + R.rec.off[0]); A.cj = (const int*)(slab + R.rec.off[1]); A.cd = (const float*)(slab + R.rec.off[2]);
        A.cs = (const uint16_t*)(slab + R.rec.off[3]); A.cct = slab + R.rec.off[4];
    }
    A.aa_off = R.rec.pose_off.p; A.aa_count = R.rec.count;
    A.summary = R.rec.summary.p; A.P = (int)P;
    if (planes) {
        A.pl = L.col; A.pl_off = L.pose_off.p; A.pl_summary = L.summary.p;
        for (int t = 0; t < 4; ++t) A.pl_count[t] = L.counts[t];
    }
    A.kind = kind; A.skip = (int)skip; A.M = (int)M;
    if (kind == ARP_SHORTLIST_SUMMARY)
        for (int q = 0; q < 2 * PSL_SLOTS; ++q) A.w[q] = weights32[q];
    if (kind == ARP_SHORTLIST_TANIMOTO) { A.fp_count = F.count.p; A.fp_cross = F.cross.p; A.Q = (int)F.Q; A.ref = (int)ref; }
    A.min_score = list ? INT64_MIN : min_score;
    A.tables = tables; A.sift_mask = sift_mask; A.ctype_mask = ctype_mask;
    ShortlistSteps steps{};
    steps.same_poses = [&](void* flag) { enqueue_same_poses(c, flag); };
    steps.score = [&](const PslArgs& B) { hipLaunchKernelGGL(k_psl_score, dim3(nblocks(M, 256)), dim3(256), 0, c->stream, B); };
    steps.differ = "the poses result and the poses-planes result were made from different poses";
    CHK(shortlist_make(c, fn, S, A, pose_ids, M, ncand, steps));
    shortlist_info(S, info);
    return ARP_OK;
}

// a shortlist fetch: the device's error word rides along with the pieces (the gather runs after the launch's wait)
static int shortlist_stage(arp_ctx* c, const ShortlistResult& S, std::vector<StagePiece>& pieces, const std::string& fn) {
    unsigned long long err = 0;
    pieces.push_back(StagePiece{&err, S.words.p + PSL_W_ERR, sizeof(err)});
    CHK(stage_fetch(c, pieces));
    if (err != 0) FAIL(c, ARP_E_HIP, fn + ": device error (a record beyond its table's total)");
    return ARP_OK;
}

// The two fetches of a shortlist, for the pose shortlist and the library shortlist alike.  `fn` names the entry, `launch` the
// launch and what voids the result, `cap_name` the capacity of the per-entry arrays, `planes_result` the planes source.
struct ShortlistNames { const char *fn, *launch, *cap_name, *planes_result; };
static int shortlist_fetch(arp_ctx* c, const ShortlistResult& S, const ShortlistNames& N, int64_t cap_entries, int64_t cap, int32_t* ligand, int32_t* pose,
                           int64_t* score, uint32_t* summary, uint32_t* planes_summary, uint64_t* off, int32_t* i, int32_t* j, float* dist, uint16_t* sift,
                           uint8_t* ctype, int64_t* n_chosen, int64_t* count) {
    const std::string fn = N.fn;
    if (!S.valid) FAIL(c, ARP_E_ARG, fn + ": no result (" + N.launch + ")");
    *n_chosen = S.K;
    *count = S.total[0];
    const bool records = i || j || dist || sift || ctype;
    if ((off || records) && !(S.tables & 1u)) FAIL(c, ARP_E_ARG, fn + ": the atom-atom table was not requested (tables bit 0)");
    if (planes_summary && !S.planes) FAIL(c, ARP_E_ARG, fn + ": the launch did not read the " + N.planes_result + " result (no planes_summary)");
    if ((ligand || pose || score || summary || planes_summary || off) && cap_entries < S.K)
        FAIL(c, ARP_E_CAPACITY, fn + ": output buffers too small (" + N.cap_name + " < *n_chosen)");
    if (records && cap < S.total[0]) FAIL(c, ARP_E_CAPACITY, fn + ": output buffers too small (cap < *count)");
    HIPCHK(c, hipSetDevice(c->device));
    const size_t K = (size_t)S.K, n = (size_t)S.total[0];
    std::vector<StagePiece> pieces;
    want_piece(pieces, ligand, S.ligand.p, K * sizeof(int32_t));
    want_piece(pieces, pose, S.pose.p, K * sizeof(int32_t));
    want_piece(pieces, score, S.score.p, K * sizeof(int64_t));
    want_piece(pieces, summary, S.summary.p, K * PSL_SLOTS * sizeof(uint32_t));
    want_piece(pieces, planes_summary, S.pl_summary.p, K * PSL_SLOTS * sizeof(uint32_t));
    want_piece(pieces, off, S.off.p, (K + 1) * sizeof(unsigned long long));
    if (records && n > 0) {
        const uint8_t* const slab = S.slab.p;
        want_piece(pieces, i, slab + S.aa_off[0], n * sizeof(int32_t));
        want_piece(pieces, j, slab + S.aa_off[1], n * sizeof(int32_t));
        want_piece(pieces, dist, slab + S.aa_off[2], n * sizeof(float));
        want_piece(pieces, sift, slab + S.aa_off[3], n * sizeof(uint16_t));
        want_piece(pieces, ctype, slab + S.aa_off[4], n * sizeof(uint8_t));
    }
    return shortlist_stage(c, S, pieces, fn);
}
static int shortlist_planes_fetch(arp_ctx* c, const ShortlistResult& S, const ShortlistNames& N, int table, int64_t cap_entries, int64_t cap, uint64_t* off,
                                  int32_t* first, int32_t* second, void* const v[4], uint8_t* const u[3], int64_t* count) {
    const std::string fn = N.fn;
    if (!S.valid) FAIL(c, ARP_E_ARG, fn + ": no result (" + N.launch + ")");
    if (table < 0 || table > 3) FAIL(c, ARP_E_ARG, fn + ": table must be ARP_POSES_PLANES_ATOM_PLANE ... ARP_POSES_PLANES_GROUP_PLANE");
    const int t = table;
    if (!((S.tables >> (t + 1)) & 1u)) FAIL(c, ARP_E_ARG, fn + ": the table was not requested (tables bit table + 1)");
    *count = S.total[t + 1];
    bool records = false;
    CHK(plane_fetch_columns(c, fn + ": ", t, first, second, v, u, &records));
    if (off && cap_entries < S.K) FAIL(c, ARP_E_CAPACITY, fn + ": output buffers too small (" + N.cap_name + " < chosen poses)");
    if (records && cap < S.total[t + 1]) FAIL(c, ARP_E_CAPACITY, fn + ": output buffers too small (cap < *count)");
    HIPCHK(c, hipSetDevice(c->device));
    std::vector<StagePiece> pieces;
    want_piece(pieces, off, S.off.p + (size_t)(t + 1) * ((size_t)S.ncand + 1), ((size_t)S.K + 1) * sizeof(unsigned long long));
    if (records) plane_fetch_pieces(pieces, S.col, t, (size_t)S.total[t + 1], first, second, v, u);
    return shortlist_stage(c, S, pieces, fn);
}

// (the pose shortlist is voided wherever the poses result is; with the poses-planes result when it read that)
static const char* const POSE_SHORTLIST_LAUNCH = "arp_poses_shortlist_launch; a result it was made from was replaced or an input or the selection changed since";
int arp_poses_shortlist_fetch(arp_ctx* c, int64_t cap_poses, int64_t cap, int32_t* pose, int64_t* score, uint32_t* summary, uint32_t* planes_summary,
                              uint64_t* off, int32_t* i, int32_t* j, float* dist, uint16_t* sift, uint8_t* ctype, int64_t* n_chosen, int64_t* count) {
    if (!c || !n_chosen || !count) return ARP_E_ARG;
    return shortlist_fetch(c, c->shortlist, ShortlistNames{"arp_poses_shortlist_fetch", POSE_SHORTLIST_LAUNCH, "cap_poses", "poses-planes"}, cap_poses, cap,
                           nullptr, pose, score, summary, planes_summary, off, i, j, dist, sift, ctype, n_chosen, count);
}

int arp_poses_shortlist_planes_fetch(arp_ctx* c, int table, int64_t cap_poses, int64_t cap, uint64_t* off, int32_t* first, int32_t* second, void* v0,
                                     void* v1, void* v2, void* v3, uint8_t* u0, uint8_t* u1, uint8_t* u2, int64_t* count) {
    if (!c || !count) return ARP_E_ARG;
    void* const v[4] = {v0, v1, v2, v3};
    uint8_t* const u[3] = {u0, u1, u2};
    return shortlist_planes_fetch(c, c->shortlist, ShortlistNames{"arp_poses_shortlist_planes_fetch", POSE_SHORTLIST_LAUNCH, "cap_poses", "poses-planes"},
                                  table, cap_poses, cap, off, first, second, v, u, count);
}

int arp_poses_shortlist_info(arp_ctx* c, int64_t info[8]) {
    if (!c || !info) return ARP_E_ARG;
    shortlist_info(c->shortlist, info);
    return ARP_OK;
}

// ---- library shortlist (arp_library_shortlist.h): the resident library results -> ranked poses or ligands -> the
// chosen poses' records.  The library result, and depending on the arguments the library-planes result and the library
// fingerprint, are read; only this result's own buffers are written.  The launch is the pose shortlist's (shortlist_make) with the
// library's arrays behind PslArgs and k_lsl_score as the score step.
static_assert(LSL_POSES == ARP_LIBRARY_SHORTLIST_POSES && LSL_LIGANDS == ARP_LIBRARY_SHORTLIST_LIGANDS, "arp_library_shortlist.h names the header's constants");

static void library_shortlist_info(const ShortlistResult& S, int64_t info[8]) {
    shortlist_info(S, info);
    if (S.valid) info[7] = (int64_t)S.kind | ((int64_t)S.unit << 8);
}

int arp_library_shortlist_launch(arp_ctx* c, int kind, int unit, const int32_t* weights32, int64_t ref, const int32_t* pose_ids, int64_t n_ids, int64_t k,
                                 int64_t min_score, uint32_t tables, uint32_t sift_mask, uint32_t ctype_mask, int64_t info[8]) {
    if (!c || !info) return ARP_E_ARG;
    const std::string fn = "arp_library_shortlist_launch: ";
    ShortlistResult& S = c->libshortlist;
    const LibraryResult& R = c->libres;
    const LibraryPlanesResult& L = c->libpl;
    const PoseFpResult& F = c->libfp;
    // ---- the refusals, in this order: none of them touches a resident result
    if (c->pass_pending) FAIL(c, ARP_E_ARG, fn + "a pass has not been waited for (arp_run_wait)");
    if (!R.valid) FAIL(c, ARP_E_ARG, fn + "no library result (arp_library_contacts_launch; the structure or the library changed since)");
    if (kind != ARP_SHORTLIST_LIST && kind != ARP_SHORTLIST_SUMMARY && kind != ARP_SHORTLIST_TANIMOTO)
        FAIL(c, ARP_E_ARG, fn + "unknown kind (ARP_SHORTLIST_LIST, ARP_SHORTLIST_SUMMARY or ARP_SHORTLIST_TANIMOTO)");
    if (unit != ARP_LIBRARY_SHORTLIST_POSES && unit != ARP_LIBRARY_SHORTLIST_LIGANDS)
        FAIL(c, ARP_E_ARG, fn + "unknown unit (ARP_LIBRARY_SHORTLIST_POSES or ARP_LIBRARY_SHORTLIST_LIGANDS)");
    const int64_t T = R.T;
    CHK(shortlist_filter_refusals(c, fn, tables, sift_mask, ctype_mask));
    bool planes = (tables >> 1) != 0;
    if (kind == ARP_SHORTLIST_LIST) {
        if (!pose_ids) FAIL(c, ARP_E_ARG, fn + "pose_ids missing (ARP_SHORTLIST_LIST)");
        if (n_ids < 1 || n_ids > ARP_POSES_MAX_POSES) FAIL(c, ARP_E_ARG, fn + "n_ids must be 1 ... ARP_POSES_MAX_POSES");
        for (int64_t q = 0; q < n_ids; ++q)
            if (pose_ids[q] < 0 || pose_ids[q] >= T) FAIL(c, ARP_E_ARG, fn + "pose_ids has an id outside [0, T)");
        if (unit != ARP_LIBRARY_SHORTLIST_POSES || k != 0 || min_score != INT64_MIN)
            FAIL(c, ARP_E_ARG, fn + "ARP_SHORTLIST_LIST takes unit = ARP_LIBRARY_SHORTLIST_POSES, k = 0 and min_score = INT64_MIN (the list is the choice)");
    } else if (k < 1) FAIL(c, ARP_E_ARG, fn + "k must be at least 1");
    if (kind == ARP_SHORTLIST_SUMMARY) {
        if (!weights32) FAIL(c, ARP_E_ARG, fn + "weights missing (ARP_SHORTLIST_SUMMARY)");
        for (int q = 0; q < 2 * PSL_SLOTS; ++q) {
            if (weights32[q] > ARP_SHORTLIST_MAX_WEIGHT || weights32[q] < -ARP_SHORTLIST_MAX_WEIGHT) FAIL(c, ARP_E_ARG, fn + "weights has an entry beyond +-ARP_SHORTLIST_MAX_WEIGHT = 2^24");
            if (q >= PSL_SLOTS && weights32[q] != 0) planes = true;
        }
    }
    if (kind == ARP_SHORTLIST_TANIMOTO) {
        if (!F.valid) FAIL(c, ARP_E_ARG, fn + "no library fingerprint (arp_library_fingerprints_launch; ARP_SHORTLIST_TANIMOTO)");
        if (F.Q < 1) FAIL(c, ARP_E_ARG, fn + "the library fingerprint has no references (n_refs = 0)");
        if (ref < -1 || ref >= F.Q) FAIL(c, ARP_E_ARG, fn + "ref must be -1 or in [0, n_refs)");
        if (F.P != F.Q + T) FAIL(c, ARP_E_HIP, fn + "the library fingerprint and the library result differ in T");      // (never: it goes with the result)
    }
    if (planes) {
        if (!L.valid) FAIL(c, ARP_E_ARG, fn + "no library-planes result (arp_library_planes_launch; the structure, the library or its plane table changed since)");
        if (L.L != R.L || L.T != T || L.host_pose_off != R.host_pose_off || L.nx != R.nx)
            FAIL(c, ARP_E_ARG, fn + "the library result and the library-planes result differ in ligands, poses or pose ranges (launch both on the same poses)");
    }
    // ---- from here on the previous library shortlist is gone
    void_pose_results(c, POSE_LIBRARY_SHORTLIST);
    S.planes = planes;
    S.unit = unit;
    const bool list = kind == ARP_SHORTLIST_LIST, ligands = unit == ARP_LIBRARY_SHORTLIST_LIGANDS;
    int64_t posed = 0;      // the ligands with at least one pose: the candidates of unit ligands
    for (int64_t l = 0; l < R.L; ++l) posed += R.host_pose_off[(size_t)l + 1] > R.host_pose_off[(size_t)l] ? 1 : 0;
    const int64_t M = ligands ? R.L : T, ncand = list ? n_ids : std::min(k, ligands ? posed : T);
    HIPCHK(c, hipSetDevice(c->device));
    HIPCHK(c, S.ligand.reserve((size_t)ncand));
    PslArgs A{};
    const uint8_t* const slab = R.rec.slab.p;      // (no record: the columns are never read, every segment is empty)
    if (R.rec.count > 0) {
        A.ci = (const int*)(slab + R.rec.off[0]); A.cj = (const int*)(slab + R.rec.off[1]); A.cd = (const float*)(slab + R.rec.off[2]);
        A.cs = (const uint16_t*)(slab + R.rec.off[3]); A.cct = slab + R.rec.off[4];
    }
    A.aa_off = R.rec.pose_off.p; A.aa_count = R.rec.count;
    A.summary = R.rec.summary.p; A.P = (int)T;
    if (planes) {
        A.pl = L.col; A.pl_off = L.pose_off.p; A.pl_summary = L.summary.p;
        for (int t = 0; t < 4; ++t) A.pl_count[t] = L.counts[t];
    }
    A.kind = kind; A.M = (int)M;
    A.min_score = list ? INT64_MIN : min_score;
    A.tables = tables; A.sift_mask = sift_mask; A.ctype_mask = ctype_mask;
    LslScore W{};
    W.L = (int)R.L; W.T = (int)T; W.lig_pose_off = R.tab.p;
    W.summary = A.summary; W.pl_summary = A.pl_summary;
    if (kind == ARP_SHORTLIST_SUMMARY)
        for (int q = 0; q < 2 * PSL_SLOTS; ++q) W.w[q] = weights32[q];
    if (kind == ARP_SHORTLIST_TANIMOTO) { W.fp_count = F.count.p; W.fp_cross = F.cross.p; W.Q = (int)F.Q; W.ref = (int)ref; }
    ShortlistSteps steps{};
    steps.same_poses = [&](void* flag) {
        hipLaunchKernelGGL(k_pfp_same_poses, dim3(nblocks(R.nx, 256, c->num_cu)), dim3(256), 0, c->stream, (const uint32_t*)R.rec.xyz.p,
                           (const uint32_t*)L.xyz.p, (long long)R.nx, (uint32_t*)flag);
    };
    steps.score = [&](const PslArgs& B) {
        W.key = B.key; W.val = B.val;
        const bool summary = kind == ARP_SHORTLIST_SUMMARY;
        const auto kernel = ligands ? (summary ? k_lsl_score<LSL_LIGANDS, PSL_SUMMARY> : k_lsl_score<LSL_LIGANDS, PSL_TANIMOTO>)
                                    : (summary ? k_lsl_score<LSL_POSES, PSL_SUMMARY> : k_lsl_score<LSL_POSES, PSL_TANIMOTO>);
        hipLaunchKernelGGL(kernel, dim3(ligands ? nblocks(M * 64, 256, 2048) : nblocks(M, 256)), dim3(256), 0, c->stream, W);
    };
    steps.riders = [&](const PslArgs& B) {
        hipLaunchKernelGGL(k_lsl_ligands, dim3(nblocks(ncand, 256)), dim3(256), 0, c->stream, B, (const int*)R.lig_of.p, S.ligand.p);
    };
    steps.differ = "the library result and the library-planes result were made from different poses";
    CHK(shortlist_make(c, fn, S, A, pose_ids, M, ncand, steps));
    library_shortlist_info(S, info);
    return ARP_OK;
}

// (the library shortlist is voided wherever the library result is; with the library-planes result when it read that)
static const ShortlistNames library_shortlist_names(const char* fn) {
    return ShortlistNames{fn, "arp_library_shortlist_launch; a result it was made from was replaced or the structure, the library or its plane table changed since",
                          "cap_entries", "library-planes"};
}
int arp_library_shortlist_fetch(arp_ctx* c, int64_t cap_entries, int64_t cap, int32_t* ligand, int32_t* pose, int64_t* score, uint32_t* summary,
                                uint32_t* planes_summary, uint64_t* off, int32_t* i, int32_t* a, float* dist, uint16_t* sift, uint8_t* ctype,
                                int64_t* n_chosen, int64_t* count) {
    if (!c || !n_chosen || !count) return ARP_E_ARG;
    return shortlist_fetch(c, c->libshortlist, library_shortlist_names("arp_library_shortlist_fetch"), cap_entries, cap, ligand, pose, score, summary,
                           planes_summary, off, i, a, dist, sift, ctype, n_chosen, count);
}

int arp_library_shortlist_planes_fetch(arp_ctx* c, int table, int64_t cap_entries, int64_t cap, uint64_t* off, int32_t* first, int32_t* second, void* v0,
                                       void* v1, void* v2, void* v3, uint8_t* u0, uint8_t* u1, uint8_t* u2, int64_t* count) {
    if (!c || !count) return ARP_E_ARG;
    void* const v[4] = {v0, v1, v2, v3};
    uint8_t* const u[3] = {u0, u1, u2};
    return shortlist_planes_fetch(c, c->libshortlist, library_shortlist_names("arp_library_shortlist_planes_fetch"), table, cap_entries, cap, off, first,
                                  second, v, u, count);
}

int arp_library_shortlist_info(arp_ctx* c, int64_t info[8]) {
    if (!c || !info) return ARP_E_ARG;
    library_shortlist_info(c->libshortlist, info);
    return ARP_OK;
}

// ---- pose clusters (arp_poses_clusters.h): the resident fingerprint result -> leaders and members
// The fingerprint result is read while the launch runs (bits, count); only this result's own buffers are written.  The rounds are
// enqueued back to back, POSECL_ROUNDS_PER_WAIT at a time: after such a group one word — the next leader's position — comes back
// through the stage, and a sentinel there ends the rounds (no position is left).  Up to that many rounds there is one wait: the
// word block of k_pcl_finish (C, the unassigned count).
static_assert(PCL_MAX_CLUSTERS == ARP_POSECL_MAX_CLUSTERS, "arp_poses_clusters.h names the header's constant");
const int64_t POSECL_ROUNDS_PER_WAIT = 64;

static void clusters_info(const ClustersResult& S, int64_t info[8]) {
    const int64_t v[8] = {S.M, S.C, S.unassigned, S.max_clusters, S.W, S.lanes, S.launches, (int64_t)S.threshold};
    for (int q = 0; q < 8; ++q) info[q] = (S.valid || q == 6) ? v[q] : 0;
}

int arp_poses_clusters_launch(arp_ctx* c, const int32_t* order, int64_t n_order, int64_t skip, uint64_t threshold_q32, int64_t max_clusters,
                              int64_t info[8]) {
    if (!c || !info) return ARP_E_ARG;
    const std::string fn = "arp_poses_clusters_launch: ";
    ClustersResult& S = c->clusters;
    const PoseFpResult& F = c->posefp;
    // ---- the refusals: none of them touches a resident result
    if (c->pass_pending) FAIL(c, ARP_E_ARG, fn + "a pass has not been waited for (arp_run_wait)");
    CHK(need_poses_result(c, fn));
    if (!F.valid) FAIL(c, ARP_E_ARG, fn + "no fingerprint result (arp_poses_fingerprints_launch)");
    if (F.P != c->poses.P) FAIL(c, ARP_E_ARG, fn + "the fingerprint result and the poses result differ in P");
    const int64_t P = F.P;
    if (threshold_q32 > PCL_ONE_Q32) FAIL(c, ARP_E_ARG, fn + "threshold_q32 must be 0 ... 2^32 (1.0)");
    if (max_clusters < 1 || max_clusters > ARP_POSECL_MAX_CLUSTERS) FAIL(c, ARP_E_ARG, fn + "max_clusters must be 1 ... ARP_POSECL_MAX_CLUSTERS");
    if (order) {
        if (skip != 0) FAIL(c, ARP_E_ARG, fn + "an order takes skip = 0 (the list names the positions)");
        if (n_order < 1 || n_order > ARP_POSES_MAX_POSES) FAIL(c, ARP_E_ARG, fn + "n_order must be 1 ... ARP_POSES_MAX_POSES");
        for (int64_t q = 0; q < n_order; ++q)
            if (order[q] < 0 || order[q] >= P) FAIL(c, ARP_E_ARG, fn + "order has an id outside [0, P)");
    } else {
        if (n_order != 0) FAIL(c, ARP_E_ARG, fn + "n_order must be 0 without an order");
        if (skip < 0 || skip >= P) FAIL(c, ARP_E_ARG, fn + "skip must be in [0, P)");
    }
    // ---- from here on the previous clusters are gone
    void_pose_results(c, POSE_CLUSTERS);
    S.classes = F.classes;
    HIPCHK(c, hipSetDevice(c->device));
    const int64_t M = order ? n_order : P - skip, W = F.U > 0 ? F.W : 0;
    const size_t mc = (size_t)max_clusters;
    HIPCHK(c, S.words.reserve(4));
    HIPCHK(c, S.next.reserve(mc + 1));
    HIPCHK(c, S.size.reserve(mc));
    HIPCHK(c, S.leader.reserve(mc));
    HIPCHK(c, S.leader_position.reserve(mc));
    HIPCHK(c, S.pose.reserve((size_t)M));
    HIPCHK(c, S.cluster.reserve((size_t)M));
    HIPCHK(c, S.similarity.reserve((size_t)M));
    PclArgs A{};
    A.bits = W > 0 ? F.bits.p : nullptr;      // (U = 0: the matrix was never allocated)
    A.count = F.count.p; A.W = W;
    A.skip = (int)skip; A.M = (int)M;
    A.threshold = threshold_q32; A.max_clusters = (int)max_clusters;
    A.g = pcl_group_width(W); A.g_log2 = __builtin_ctz((unsigned)A.g);
    A.next = S.next.p; A.pose = S.pose.p; A.cluster = S.cluster.p; A.similarity = S.similarity.p;
    A.leader = S.leader.p; A.leader_position = S.leader_position.p; A.size = S.size.p; A.words = S.words.p;
    if (order) {
        CHK(upload_async(c, S.order, (const int*)order, (size_t)n_order));      // (the wait below is before the caller's array goes away)
        A.order = S.order.p;
    }
    // ---- nothing assigned: cluster = -1, similarity = -1, every next but the first the sentinel
    HIPCHK(c, hipMemsetAsync(S.words.p, 0, 4 * sizeof(unsigned long long), c->stream));
    HIPCHK(c, hipMemsetAsync(S.size.p, 0, mc * sizeof(uint32_t), c->stream));
    HIPCHK(c, hipMemsetAsync(S.cluster.p, 0xFF, (size_t)M * sizeof(int), c->stream));
    HIPCHK(c, hipMemsetAsync(S.similarity.p, 0xFF, (size_t)M * sizeof(long long), c->stream));
    HIPCHK(c, hipMemsetAsync(S.next.p, 0xFF, (mc + 1) * sizeof(uint32_t), c->stream));
    HIPCHK(c, hipMemsetAsync(S.next.p, 0, sizeof(uint32_t), c->stream));
    // ---- the rounds
    const int64_t rounds = std::min(max_clusters, M);
    const int per_block = PCL_THREADS / A.g;
    const dim3 grid(nblocks(M, per_block, 16 * std::max(c->num_cu, 1)));
    int64_t enqueued = 0;
    while (enqueued < rounds) {
        const int64_t end = std::min(rounds, enqueued + POSECL_ROUNDS_PER_WAIT);
        for (; enqueued < end; ++enqueued) hipLaunchKernelGGL(k_pcl_round, grid, dim3(PCL_THREADS), 0, c->stream, A, (int)enqueued);
        CHK(check_launch(c, (fn + "rounds").c_str()));
        if (enqueued < rounds) {
            CHK(stage_copy(c, S.next.p + enqueued, sizeof(uint32_t)));
            uint32_t next_leader;
            memcpy(&next_leader, c->table_stage, sizeof(next_leader));
            if (next_leader == PCL_SENTINEL) break;
        }
    }
    hipLaunchKernelGGL(k_pcl_finish, dim3(nblocks(M, PCL_THREADS, 256)), dim3(PCL_THREADS), 0, c->stream, A);
    CHK(check_launch(c, (fn + "finish").c_str()));
    CHK(stage_copy(c, S.words.p, 4 * sizeof(unsigned long long)));
    unsigned long long h[4];
    memcpy(h, c->table_stage, sizeof(h));
    ++S.launches;
    if (h[PCL_W_CLUSTERS] < 1 || h[PCL_W_CLUSTERS] > (unsigned long long)rounds || h[PCL_W_UNASSIGNED] > (unsigned long long)M)
        FAIL(c, ARP_E_HIP, fn + "cluster count out of range");
    S.M = M; S.C = (int64_t)h[PCL_W_CLUSTERS]; S.unassigned = (int64_t)h[PCL_W_UNASSIGNED]; S.max_clusters = max_clusters;
    S.W = W; S.lanes = A.g; S.threshold = threshold_q32;
    S.valid = true;
    clusters_info(S, info);
    return ARP_OK;
}

int arp_poses_clusters_fetch(arp_ctx* c, int64_t cap_positions, int64_t cap_clusters, int32_t* pose, int32_t* cluster, int64_t* similarity,
                             int32_t* leader, int32_t* leader_position, uint32_t* size, int64_t* n_positions, int64_t* n_clusters) {
    if (!c || !n_positions || !n_clusters) return ARP_E_ARG;
    const ClustersResult& S = c->clusters;
    if (!S.valid)      // (voided wherever the poses result is; with the poses-planes result when the fingerprint had class planes)
        FAIL(c, ARP_E_ARG, "arp_poses_clusters_fetch: no result (arp_poses_clusters_launch; a result it was made from was replaced or an input or the selection changed since)");
    *n_positions = S.M;
    *n_clusters = S.C;
    if ((pose || cluster || similarity) && cap_positions < S.M) FAIL(c, ARP_E_CAPACITY, "arp_poses_clusters_fetch: output buffers too small (cap_positions < *n_positions)");
    if ((leader || leader_position || size) && cap_clusters < S.C) FAIL(c, ARP_E_CAPACITY, "arp_poses_clusters_fetch: output buffers too small (cap_clusters < *n_clusters)");
    HIPCHK(c, hipSetDevice(c->device));
    const size_t M = (size_t)S.M, C = (size_t)S.C;
    std::vector<StagePiece> pieces;
    want_piece(pieces, pose, S.pose.p, M * sizeof(int32_t));
    want_piece(pieces, cluster, S.cluster.p, M * sizeof(int32_t));
    want_piece(pieces, similarity, S.similarity.p, M * sizeof(int64_t));
    want_piece(pieces, leader, S.leader.p, C * sizeof(int32_t));
    want_piece(pieces, leader_position, S.leader_position.p, C * sizeof(int32_t));
    want_piece(pieces, size, S.size.p, C * sizeof(uint32_t));
    return stage_fetch(c, pieces);
}

int arp_poses_clusters_info(arp_ctx* c, int64_t info[8]) {
    if (!c || !info) return ARP_E_ARG;
    clusters_info(c->clusters, info);
    return ARP_OK;
}

// ---- library clusters (arp_library_clusters.h): the resident library fingerprint -> leaders and members
// The library fingerprint (bits, count from row Q on), the library result (lig_of) and, for ARP_LIBCL_SHORTLIST, the library
// shortlist (its pose column) are read while the launch runs; only this result's own buffers are written.  A round is two
// launches (k_lcl_window, k_lcl_sweep) and elects up to 32 leaders; the rounds are enqueued LIBCL_ROUNDS_PER_WAIT at a time, and
// after a group that is not the last one word — the next round's start — comes back through the stage; the sentinel ends the
// rounds.  32 rounds are 64 launches: enqueued in vain (2.3 - 2.9 us a no-op launch) they cost 0.15 - 0.19 ms,
// under half of the 0.4 - 0.5 ms of the wait they stand in for, and they cover 1024 positions that all lead.
static_assert(LCL_WINDOW == ARP_LIBCL_WINDOW && LCL_LDS_WORDS == ARP_LIBCL_LDS_WORDS, "arp_library_clusters.h names the header's constants");
static_assert(LCL_ALL == ARP_LIBCL_ALL && LCL_LIST == ARP_LIBCL_LIST && LCL_SHORTLIST == ARP_LIBCL_SHORTLIST, "... and its sources");
const int64_t LIBCL_ROUNDS_PER_WAIT = 32;

static void library_clusters_info(const LibClustersResult& S, int64_t info[8]) {
    const int64_t v[8] = {S.M, S.C, S.unassigned, S.max_clusters, S.W, S.rounds, S.launches, (int64_t)S.threshold};
    for (int q = 0; q < 8; ++q) info[q] = (S.valid || q == 6) ? v[q] : 0;
}

int arp_library_clusters_launch(arp_ctx* c, int source, const int32_t* order, int64_t n_order, uint64_t threshold_q32, int64_t max_clusters,
                                int64_t info[8]) {
    if (!c || !info) return ARP_E_ARG;
    const std::string fn = "arp_library_clusters_launch: ";
    LibClustersResult& S = c->libclusters;
    const LibraryResult& R = c->libres;
    const PoseFpResult& F = c->libfp;
    const ShortlistResult& K = c->libshortlist;
    // ---- the refusals, in this order: none of them touches a resident result
    if (c->pass_pending) FAIL(c, ARP_E_ARG, fn + "a pass has not been waited for (arp_run_wait)");
    if (!R.valid) FAIL(c, ARP_E_ARG, fn + "no library result (arp_library_contacts_launch; the structure or the library changed since)");
    if (!F.valid) FAIL(c, ARP_E_ARG, fn + "no library fingerprint (arp_library_fingerprints_launch)");
    const int64_t T = R.T, Q = F.Q;
    if (F.P != Q + T) FAIL(c, ARP_E_ARG, fn + "the library fingerprint and the library result differ in T (P is not Q + T)");
    if (threshold_q32 > PCL_ONE_Q32) FAIL(c, ARP_E_ARG, fn + "threshold_q32 must be 0 ... 2^32 (1.0)");
    if (max_clusters < 1 || max_clusters > ARP_POSECL_MAX_CLUSTERS) FAIL(c, ARP_E_ARG, fn + "max_clusters must be 1 ... ARP_POSECL_MAX_CLUSTERS");
    if (source != ARP_LIBCL_ALL && source != ARP_LIBCL_LIST && source != ARP_LIBCL_SHORTLIST)
        FAIL(c, ARP_E_ARG, fn + "unknown source (ARP_LIBCL_ALL, ARP_LIBCL_LIST or ARP_LIBCL_SHORTLIST)");
    if (source == ARP_LIBCL_LIST) {
        if (!order) FAIL(c, ARP_E_ARG, fn + "order missing (ARP_LIBCL_LIST)");
        if (n_order < 1 || n_order > ARP_POSES_MAX_POSES) FAIL(c, ARP_E_ARG, fn + "n_order must be 1 ... ARP_POSES_MAX_POSES");
        for (int64_t q = 0; q < n_order; ++q)
            if (order[q] < 0 || order[q] >= T) FAIL(c, ARP_E_ARG, fn + "order has an id outside [0, T)");
    } else if (order || n_order != 0)
        FAIL(c, ARP_E_ARG, fn + "an order goes with ARP_LIBCL_LIST alone (order = NULL and n_order = 0 otherwise)");
    if (source == ARP_LIBCL_SHORTLIST) {
        if (!K.valid) FAIL(c, ARP_E_ARG, fn + "no library shortlist (arp_library_shortlist_launch; ARP_LIBCL_SHORTLIST)");
        if (K.K < 1) FAIL(c, ARP_E_ARG, fn + "the library shortlist is empty (K = 0)");
    }
    // ---- from here on the previous library clusters are gone
    void_pose_results(c, POSE_LIBRARY_CLUSTERS);
    HIPCHK(c, hipSetDevice(c->device));
    const int64_t M = source == ARP_LIBCL_ALL ? T : source == ARP_LIBCL_LIST ? n_order : K.K, W = F.U > 0 ? F.W : 0;
    const int64_t rounds = std::min(max_clusters, (M + LCL_WINDOW - 1) / LCL_WINDOW);
    const size_t mc = (size_t)max_clusters, nr = (size_t)rounds;
    HIPCHK(c, S.words.reserve(4));
    HIPCHK(c, S.made.reserve(1));
    HIPCHK(c, S.start.reserve(nr + 1));
    HIPCHK(c, S.nl.reserve(nr));
    HIPCHK(c, S.wl.reserve(nr * LCL_WINDOW));
    HIPCHK(c, S.size.reserve(mc));
    HIPCHK(c, S.leader.reserve(mc));
    HIPCHK(c, S.leader_position.reserve(mc));
    HIPCHK(c, S.pose.reserve((size_t)M));
    HIPCHK(c, S.ligand.reserve((size_t)M));
    HIPCHK(c, S.cluster.reserve((size_t)M));
    HIPCHK(c, S.similarity.reserve((size_t)M));
    LclArgs A{};
    A.bits = W > 0 ? F.bits.p + Q * W : nullptr;      // (pose t is row Q + t; U = 0: the matrix was never allocated)
    A.count = F.count.p + Q; A.W = W;
    A.lig_of = R.lig_of.p; A.M = (int)M;
    A.threshold = threshold_q32; A.max_clusters = (int)max_clusters;
    A.g = pcl_group_width(W); A.g_log2 = __builtin_ctz((unsigned)A.g);
    A.rounds = (int)rounds;
    A.start = S.start.p; A.nl = S.nl.p; A.wl = S.wl.p; A.made = S.made.p;
    A.pose = S.pose.p; A.ligand = S.ligand.p; A.cluster = S.cluster.p; A.similarity = S.similarity.p;
    A.leader = S.leader.p; A.leader_position = S.leader_position.p; A.size = S.size.p; A.words = S.words.p;
    if (source == ARP_LIBCL_LIST) {
        CHK(upload_async(c, S.order, (const int*)order, (size_t)n_order));      // (the wait below is before the caller's array goes away)
        A.ids = S.order.p;
    } else if (source == ARP_LIBCL_SHORTLIST) A.ids = K.pose.p;      // (read by k_lcl_positions alone: no id crosses to the host)
    // ---- nothing assigned: cluster = -1, similarity = -1, no leader made, every start but the first the sentinel
    HIPCHK(c, hipMemsetAsync(S.words.p, 0, 4 * sizeof(unsigned long long), c->stream));
    HIPCHK(c, hipMemsetAsync(S.made.p, 0, sizeof(uint32_t), c->stream));
    HIPCHK(c, hipMemsetAsync(S.nl.p, 0, nr * sizeof(uint32_t), c->stream));
    HIPCHK(c, hipMemsetAsync(S.size.p, 0, mc * sizeof(uint32_t), c->stream));
    HIPCHK(c, hipMemsetAsync(S.cluster.p, 0xFF, (size_t)M * sizeof(int), c->stream));
    HIPCHK(c, hipMemsetAsync(S.similarity.p, 0xFF, (size_t)M * sizeof(long long), c->stream));
    HIPCHK(c, hipMemsetAsync(S.start.p, 0xFF, (nr + 1) * sizeof(uint32_t), c->stream));
    HIPCHK(c, hipMemsetAsync(S.start.p, 0, sizeof(uint32_t), c->stream));
    hipLaunchKernelGGL(k_lcl_positions, dim3(nblocks(M, LCL_THREADS, 1 << 20)), dim3(LCL_THREADS), 0, c->stream, A);
    CHK(check_launch(c, (fn + "positions").c_str()));
    // ---- the rounds
    const int per_block = LCL_THREADS / A.g;
    const dim3 grid(nblocks(M, per_block, 16 * std::max(c->num_cu, 1)));
    int64_t enqueued = 0;
    while (enqueued < rounds) {
        const int64_t end = std::min(rounds, enqueued + LIBCL_ROUNDS_PER_WAIT);
        for (; enqueued < end; ++enqueued) {
            hipLaunchKernelGGL(k_lcl_window, dim3(1), dim3(LCL_THREADS), 0, c->stream, A, (int)enqueued);
            hipLaunchKernelGGL(k_lcl_sweep, grid, dim3(LCL_THREADS), 0, c->stream, A, (int)enqueued);
        }
        CHK(check_launch(c, (fn + "rounds").c_str()));
        if (enqueued < rounds) {
            CHK(stage_copy(c, S.start.p + enqueued, sizeof(uint32_t)));
            uint32_t next_start;
            memcpy(&next_start, c->table_stage, sizeof(next_start));
            if (next_start == PCL_SENTINEL) break;
        }
    }
    hipLaunchKernelGGL(k_lcl_finish, dim3(nblocks(M, LCL_THREADS, 256)), dim3(LCL_THREADS), 0, c->stream, A);
    CHK(check_launch(c, (fn + "finish").c_str()));
    CHK(stage_copy(c, S.words.p, 4 * sizeof(unsigned long long)));
    unsigned long long h[4];
    memcpy(h, c->table_stage, sizeof(h));
    ++S.launches;
    if (h[LCL_W_CLUSTERS] < 1 || h[LCL_W_CLUSTERS] > (unsigned long long)std::min(max_clusters, M) || h[LCL_W_UNASSIGNED] > (unsigned long long)M ||
        h[LCL_W_ROUNDS] < 1 || h[LCL_W_ROUNDS] > (unsigned long long)rounds)
        FAIL(c, ARP_E_HIP, fn + "cluster count out of range");
    S.M = M; S.C = (int64_t)h[LCL_W_CLUSTERS]; S.unassigned = (int64_t)h[LCL_W_UNASSIGNED]; S.max_clusters = max_clusters;
    S.W = W; S.rounds = (int64_t)h[LCL_W_ROUNDS]; S.threshold = threshold_q32;
    S.valid = true;
    library_clusters_info(S, info);
    return ARP_OK;
}

int arp_library_clusters_fetch(arp_ctx* c, int64_t cap_positions, int64_t cap_clusters, int32_t* pose, int32_t* ligand, int32_t* cluster,
                               int64_t* similarity, int32_t* leader, int32_t* leader_position, uint32_t* size, int64_t* n_positions,
                               int64_t* n_clusters) {
    if (!c || !n_positions || !n_clusters) return ARP_E_ARG;
    const LibClustersResult& S = c->libclusters;
    if (!S.valid)      // (voided wherever the library result is)
        FAIL(c, ARP_E_ARG, "arp_library_clusters_fetch: no result (arp_library_clusters_launch; the library result was replaced or the structure or the library changed since)");
    *n_positions = S.M;
    *n_clusters = S.C;
    if ((pose || ligand || cluster || similarity) && cap_positions < S.M)
        FAIL(c, ARP_E_CAPACITY, "arp_library_clusters_fetch: output buffers too small (cap_positions < *n_positions)");
    if ((leader || leader_position || size) && cap_clusters < S.C)
        FAIL(c, ARP_E_CAPACITY, "arp_library_clusters_fetch: output buffers too small (cap_clusters < *n_clusters)");
    HIPCHK(c, hipSetDevice(c->device));
    const size_t M = (size_t)S.M, C = (size_t)S.C;
    std::vector<StagePiece> pieces;
    want_piece(pieces, pose, S.pose.p, M * sizeof(int32_t));
    want_piece(pieces, ligand, S.ligand.p, M * sizeof(int32_t));
    want_piece(pieces, cluster, S.cluster.p, M * sizeof(int32_t));
    want_piece(pieces, similarity, S.similarity.p, M * sizeof(int64_t));
    want_piece(pieces, leader, S.leader.p, C * sizeof(int32_t));
    want_piece(pieces, leader_position, S.leader_position.p, C * sizeof(int32_t));
    want_piece(pieces, size, S.size.p, C * sizeof(uint32_t));
    return stage_fetch(c, pieces);
}

int arp_library_clusters_info(arp_ctx* c, int64_t info[8]) {
    if (!c || !info) return ARP_E_ARG;
    library_clusters_info(c->libclusters, info);
    return ARP_OK;
}

// ---- ligand-water-receptor contacts of the library result (arp_library_bridges.h): two resident results joined
// The library result's records and the atom-atom bag of a pass over the receptor alone, everything selected, are read; nothing
// resident but this result is written (its own sort scratch; the shared tile counts, run starts and stage are scratch of every
// table).  Two waits: L_r, the receptor's legs (sorted_water_legs), then the ligand legs with B, the rows.
// What the launch refuses of its two sources, behind its mask and in this order: the one statement, which
// arp_library_water_bridges_info asks as well (word [7])
static int library_bridge_sources(arp_ctx* c, const std::string& fn) {
    const LibraryResult& R = c->libres;
    if (!R.valid) FAIL(c, ARP_E_ARG, fn + "no library result (arp_library_contacts_launch; the structure or the library changed since)");
    // (models or a batch as the structure need no refusal of their own: making either voids the library result — POSE_STRUCTURE —,
    // and arp_library_contacts_launch refuses both, so "no library result" above has answered)
    CHK(launch_refusals(c, fn, NEED_WHOLE | NEED_AA_BAG, NO_AA_PASS));
    if (!c->bag_sel_all) FAIL(c, ARP_E_ARG, fn + "the atom-atom bag was made under a partial selection (a pass over the receptor with everything selected first)");
    if (c->bag_cutoff != R.cutoff || c->bag_comp != R.vdw_comp)
        FAIL(c, ARP_E_ARG, fn + "cutoff or vdw_comp of the receptor's pass differ from those of the library launch");
    return ARP_OK;
}

int arp_library_water_bridges_launch(arp_ctx* c, uint32_t sift_any, int64_t* count) {
    if (!c || !count) return ARP_E_ARG;
    const std::string fn = "arp_library_water_bridges_launch: ";
    // ---- the refusals, in this order: none of them touches a resident result
    CHK(check_leg_mask(c, fn, sift_any));
    CHK(library_bridge_sources(c, fn));
    const LibraryResult& R = c->libres;
    LibBridgesResult& X = c->libbridges;
    if (X.valid && X.sift_any == sift_any) { *count = X.rows; return ARP_OK; }
    HIPCHK(c, hipSetDevice(c->device));
    void_pose_results(c, POSE_LIBRARY_BRIDGES);
    const int64_t T = R.T;
    X.T = T; X.rows = X.lig_legs = X.rec_legs = X.rec_waters = 0; X.sift_any = sift_any;
    *count = 0;
    const size_t k = (size_t)c->n_contacts, kl = (size_t)R.rec.count;
    CHK(records_fit(c, fn, k));
    CHK(records_fit(c, fn, kl));
    HIPCHK(c, X.bridge_off.reserve((size_t)T + 1));
    HIPCHK(c, X.waters.reserve((size_t)T));
    HIPCHK(c, X.legs.reserve((size_t)T));
    const auto done = [&](long long rows) -> int {
        CHK(check_launch(c, (fn + "enqueue").c_str()));
        X.rows = rows; X.valid = true;
        *count = rows;
        return ARP_OK;
    };
    const auto zeros = [&]() -> int {      // no row and no leg counted: the per-pose arrays are valid, all zero
        HIPCHK(c, hipMemsetAsync(X.bridge_off.p, 0, ((size_t)T + 1) * sizeof(unsigned long long), c->stream));
        HIPCHK(c, hipMemsetAsync(X.waters.p, 0, (size_t)T * sizeof(uint32_t), c->stream));
        HIPCHK(c, hipMemsetAsync(X.legs.p, 0, (size_t)T * sizeof(uint32_t), c->stream));
        return done(0);
    };
    if (k == 0 || kl == 0) return zeros();
    // ---- the receptor's legs, sorted by (water, partner), and their runs; the host learns L_r (wait 1)
    SortedLegs S{};
    CHK(sorted_water_legs(c, fn, sift_any, X.sort, &S));
    if (S.L == 0) return zeros();
    ++X.launches;
    // ---- every water's (first leg, legs) by atom id; ligand legs, rows and heads per tile, scanned (wait 2, the last)
    const int tiles = (int)((kl + FILTER_TILE - 1) / FILTER_TILE);
    HIPCHK(c, X.water_legs.reserve((size_t)c->n));
    HIPCHK(c, X.tile.reserve(3 * (size_t)tiles));
    HIPCHK(c, X.totals.reserve(4));
    HIPCHK(c, X.at.reserve(3 * (size_t)T));
    HIPCHK(c, hipMemsetAsync(X.water_legs.p, 0, (size_t)c->n * sizeof(uint2), c->stream));
    const Columns rec{R.rec.slab.p, R.rec.off};
    LibBridgeArgs A{};
    A.ri = rec[0]; A.ra = rec[1]; A.rd = rec[2]; A.rs = rec[3]; A.k = (long long)kl;
    A.pose_off = R.rec.pose_off.p; A.T = (int)T; A.lig_of = R.lig_of.p; A.atom_off = c->library.atom_off.p;
    A.rec_flags = c->flags.p; A.lib_flags = c->library.flags.p; A.n = (int)c->n; A.sift_any = sift_any;
    A.lkey = S.key; A.lval = S.val; A.rlegs = S.L; A.pbits = S.A.pbits; A.row_start = S.R.row_start; A.runs = c->table_total.p;
    A.water_legs = X.water_legs.p; A.tile = X.tile.p; A.tiles = tiles; A.totals = X.totals.p; A.at = X.at.p;
    A.bridge_off = X.bridge_off.p; A.waters = X.waters.p; A.legs = X.legs.p;
    hipLaunchKernelGGL(k_libbridge_table, dim3(nblocks(S.L, 256, 2048)), dim3(256), 0, c->stream, A);
    hipLaunchKernelGGL(k_libbridge_count, dim3(tiles), dim3(FILTER_THREADS), 0, c->stream, A);
    hipLaunchKernelGGL(k_libbridge_scan, dim3(1), dim3(SORT_THREADS), 0, c->stream, A);
    CHK(check_launch(c, (fn + "table / count / scan").c_str()));
    long long tot[4] = {0, 0, 0, 0};
    CHK(stage_copy(c, X.totals.p, sizeof(tot)));
    memcpy(tot, c->table_stage, sizeof(tot));
    const long long LL = tot[0], B = tot[1];
    if (LL < 0 || LL > (long long)kl || B < 0 || tot[3] < 0 || tot[3] > S.L) FAIL(c, ARP_E_HIP, fn + "counts out of range");
    X.rec_legs = S.L; X.rec_waters = tot[3];
    if (B >= (1ll << 31)) { *count = B; FAIL(c, ARP_E_CAPACITY, fn + "2^31 rows or more"); }
    if (LL == 0) return zeros();
    X.lig_legs = LL;
    // ---- the rows, each at its rank, and the per-pose arrays from the same prefixes
    static const size_t es[8] = {4, 4, 4, 4, 4, 4, 2, 2};
    size_t at = 0;
    for (int q = 0; q < 8; ++q) { X.off[q] = at; at += ((size_t)B * es[q] + 255) & ~(size_t)255; }
    HIPCHK(c, X.slab.reserve(std::max<size_t>(at, 256)));
    const Columns col{X.slab.p, X.off};
    A.rows = B;
    A.t_pose = col[0]; A.t_water = col[1]; A.t_lig = col[2]; A.t_rec = col[3]; A.t_dl = col[4]; A.t_dr = col[5]; A.t_sl = col[6]; A.t_sr = col[7];
    hipLaunchKernelGGL(k_libbridge_write, dim3(tiles), dim3(FILTER_THREADS), 0, c->stream, A);
    hipLaunchKernelGGL(k_libbridge_poses, dim3(nblocks(T + 1, 256, 1 << 16)), dim3(256), 0, c->stream, A);
    return done(B);
}

int arp_library_water_bridges_fetch(arp_ctx* c, int64_t cap_rows, int64_t cap_poses, int32_t* pose, int32_t* water, int32_t* lig_atom, int32_t* rec_atom,
                                    float* dist_lig, float* dist_rec, uint16_t* sift_lig, uint16_t* sift_rec, uint64_t* bridge_off, uint32_t* waters,
                                    uint32_t* legs, int64_t* count) {
    if (!c || !count) return ARP_E_ARG;
    const LibBridgesResult& X = c->libbridges;
    const std::string fn = "arp_library_water_bridges_fetch: ";
    if (!X.valid) FAIL(c, ARP_E_ARG, fn + "no result (arp_library_water_bridges_launch; the library result or the atom-atom bag changed since)");
    *count = X.rows;
    const bool columns = pose || water || lig_atom || rec_atom || dist_lig || dist_rec || sift_lig || sift_rec;
    if (columns && X.rows > cap_rows) FAIL(c, ARP_E_CAPACITY, fn + "output buffers too small (cap_rows < *count)");
    if ((bridge_off || waters || legs) && X.T > cap_poses) FAIL(c, ARP_E_CAPACITY, fn + "output buffers too small (cap_poses < T)");
    HIPCHK(c, hipSetDevice(c->device));
    std::vector<StagePiece> pieces;
    const size_t B = (size_t)X.rows, T = (size_t)X.T;
    void* const dst[8] = {pose, water, lig_atom, rec_atom, dist_lig, dist_rec, sift_lig, sift_rec};
    static const size_t es[8] = {4, 4, 4, 4, 4, 4, 2, 2};
    for (int q = 0; q < 8; ++q) want_piece(pieces, dst[q], X.slab.p + X.off[q], B * es[q]);
    want_piece(pieces, bridge_off, X.bridge_off.p, (T + 1) * sizeof(uint64_t));
    want_piece(pieces, waters, X.waters.p, T * sizeof(uint32_t));
    want_piece(pieces, legs, X.legs.p, T * sizeof(uint32_t));
    return stage_fetch(c, pieces);
}

int arp_library_water_bridges_info(arp_ctx* c, int64_t info[8]) {
    if (!c || !info) return ARP_E_ARG;
    const LibBridgesResult& X = c->libbridges;
    // [7]: the two sources are resident and fit — a launch would pass every refusal behind its mask (what a caller asks before it
    // decides to run the receptor's pass)
    const std::string kept = c->err;       // (asking is no failure: the last error's text stays)
    const bool fit = library_bridge_sources(c, "") == ARP_OK;
    c->err = kept;
    const int64_t v[8] = {X.T, X.rows, X.lig_legs, X.rec_legs, X.rec_waters, (int64_t)X.sift_any, X.launches, fit ? 1 : 0};
    for (int q = 0; q < 8; ++q) info[q] = (X.valid || q >= 6) ? v[q] : 0;
    return ARP_OK;
}

// ---- exchange between the shards of a distributed structure (RCCL behind the C ABI) -----------------------------------
#define NCCLCHK(ctx, expr)                                                                              \
    do {                                                                                                \
        ncclResult_t r_ = (expr);                                                                       \
        if (r_ != ncclSuccess) {                                                                        \
            (ctx)->err = std::string(#expr) + ": " + rccl().GetErrorString(r_);                         \
            return ARP_E_HIP;                                                                           \
        }                                                                                               \
    } while (0)

int arp_comm_unique_id(uint8_t* out, uint64_t cap) {
    if (!out || cap < NCCL_UNIQUE_ID_BYTES) return ARP_E_ARG;
    if (!rccl().load()) { set_create_error(rccl().error); return ARP_E_HIP; }
    ncclUniqueId id;
    if (rccl().GetUniqueId(&id) != ncclSuccess) { set_create_error("ncclGetUniqueId failed"); return ARP_E_HIP; }
    memcpy(out, id.internal, NCCL_UNIQUE_ID_BYTES);
    return ARP_OK;
}

int arp_comm_init(arp_ctx* c, int rank, int world, const uint8_t* unique_id) {
    if (!c || !unique_id || world < 1 || rank < 0 || rank >= world) return ARP_E_ARG;
    if (c->comm) FAIL(c, ARP_E_ARG, "arp_comm_init: the context has a communicator already (arp_comm_destroy first)");
    if (!rccl().load()) FAIL(c, ARP_E_HIP, rccl().error);
    HIPCHK(c, hipSetDevice(c->device));
    ncclUniqueId id;
    memcpy(id.internal, unique_id, NCCL_UNIQUE_ID_BYTES);
    NCCLCHK(c, rccl().CommInitRank(&c->comm, world, id, rank));
    c->comm_rank = rank;
    c->comm_world = world;
    HIPCHK(c, c->comm_words.reserve(4));
    return ARP_OK;
}

int arp_comm_destroy(arp_ctx* c) {
    if (!c) return ARP_E_ARG;
    if (c->comm) {
        (void)hipStreamSynchronize(c->stream);
        (void)rccl().CommDestroy(c->comm);
        c->comm = nullptr;
    }
    c->comm_rank = 0;
    c->comm_world = 1;
    return ARP_OK;
}

int arp_comm_info(arp_ctx* c, int* rank, int* world) {
    if (!c) return ARP_E_ARG;
    if (rank) *rank = c->comm_rank;
    if (world) *world = c->comm_world;
    if (!c->comm) return ARP_E_ARG;
    // what RCCL itself says about the communicator (the ranks it connected), where the library exports the queries
    if (world && rccl().CommCount) NCCLCHK(c, rccl().CommCount(c->comm, world));
    if (rank && rccl().CommUserRank) NCCLCHK(c, rccl().CommUserRank(c->comm, rank));
    return ARP_OK;
}

int arp_shard_exchange_faces(arp_ctx* c, uint64_t left_ptr, uint64_t left_bytes, uint64_t right_ptr, uint64_t right_bytes, uint64_t received[4]) {
    if (!c || !received) return ARP_E_ARG;
    if (!c->comm) FAIL(c, ARP_E_ARG, "arp_shard_exchange_faces: no communicator (arp_comm_init)");
    HIPCHK(c, hipSetDevice(c->device));
    const int peer[2] = {c->comm_rank - 1, c->comm_rank + 1};
    const bool has[2] = {peer[0] >= 0, peer[1] < c->comm_world};
    const void* out_ptr[2] = {(const void*)(uintptr_t)left_ptr, (const void*)(uintptr_t)right_ptr};
    const unsigned long long out_bytes[2] = {has[0] ? left_bytes : 0ull, has[1] ? right_bytes : 0ull};
    // sizes first: one 64-bit word each way (device words, filled / read through the stream)
    unsigned long long words[4] = {out_bytes[0], out_bytes[1], 0ull, 0ull};
    HIPCHK(c, hipMemcpyAsync(c->comm_words.p, words, sizeof(words), hipMemcpyHostToDevice, c->stream));
    NCCLCHK(c, rccl().GroupStart());
    for (int s_ = 0; s_ < 2; ++s_)
        if (has[s_]) {
            NCCLCHK(c, rccl().Send(c->comm_words.p + s_, 8, ncclUint8, peer[s_], c->comm, c->stream));
            NCCLCHK(c, rccl().Recv(c->comm_words.p + 2 + s_, 8, ncclUint8, peer[s_], c->comm, c->stream));
        }
    NCCLCHK(c, rccl().GroupEnd());
    HIPCHK(c, hipMemcpyAsync(words, c->comm_words.p, sizeof(words), hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    for (int s_ = 0; s_ < 2; ++s_) HIPCHK(c, c->comm_recv[s_].reserve((size_t)std::max<unsigned long long>(words[2 + s_], 1)));
    NCCLCHK(c, rccl().GroupStart());
    for (int s_ = 0; s_ < 2; ++s_)
        if (has[s_]) {
            if (out_bytes[s_]) NCCLCHK(c, rccl().Send(out_ptr[s_], (size_t)out_bytes[s_], ncclUint8, peer[s_], c->comm, c->stream));
            if (words[2 + s_]) NCCLCHK(c, rccl().Recv(c->comm_recv[s_].p, (size_t)words[2 + s_], ncclUint8, peer[s_], c->comm, c->stream));
        }
    NCCLCHK(c, rccl().GroupEnd());
    HIPCHK(c, hipStreamSynchronize(c->stream));
    for (int s_ = 0; s_ < 2; ++s_) {
        received[2 * s_] = (has[s_] && words[2 + s_]) ? (uint64_t)(uintptr_t)c->comm_recv[s_].p : 0;
        received[2 * s_ + 1] = has[s_] ? words[2 + s_] : 0;
    }
    return ARP_OK;
}

int arp_shard_set_exchange_lists(arp_ctx* c, const int32_t* send_left, int64_t n_send_left, const int32_t* send_right, int64_t n_send_right,
                                 const int32_t* recv_left, int64_t n_recv_left, const int32_t* recv_right, int64_t n_recv_right) {
    if (!c || n_send_left < 0 || n_send_right < 0 || n_recv_left < 0 || n_recv_right < 0) return ARP_E_ARG;
    HIPCHK(c, hipSetDevice(c->device));
    const int32_t* src[4] = {send_left, send_right, recv_left, recv_right};
    const int64_t cnt[4] = {n_send_left, n_send_right, n_recv_left, n_recv_right};
    for (int k = 0; k < 4; ++k) {
        if (cnt[k] > 0 && !src[k]) return ARP_E_ARG;
        for (int64_t i = 0; i < cnt[k]; ++i)
            if (src[k][i] < 0 || src[k][i] >= c->n) FAIL(c, ARP_E_ARG, "arp_shard_set_exchange_lists: atom index out of range");
    }
    for (int s_ = 0; s_ < 2; ++s_) {
        CHK(upload_async(c, c->xl_send[s_], src[s_], (size_t)cnt[s_]));
        CHK(upload_async(c, c->xl_recv[s_], src[2 + s_], (size_t)cnt[2 + s_]));
        HIPCHK(c, c->xl_send_buf[s_].reserve((size_t)std::max<int64_t>(cnt[s_], 1)));
        HIPCHK(c, c->xl_recv_buf[s_].reserve((size_t)std::max<int64_t>(cnt[2 + s_], 1)));
        c->xl_nsend[s_] = cnt[s_];
        c->xl_nrecv[s_] = cnt[2 + s_];
    }
    return upload_done(c);
}

int arp_shard_exchange_plus(arp_ctx* c) {
    if (!c) return ARP_E_ARG;
    if (!c->comm) FAIL(c, ARP_E_ARG, "arp_shard_exchange_plus: no communicator (arp_comm_init)");
    if (!c->plus.p) FAIL(c, ARP_E_ARG, "arp_shard_exchange_plus: selection_plus does not exist yet (run stage 0 first)");
    HIPCHK(c, hipSetDevice(c->device));
    const int peer[2] = {c->comm_rank - 1, c->comm_rank + 1};
    const bool has[2] = {peer[0] >= 0, peer[1] < c->comm_world};
    for (int s_ = 0; s_ < 2; ++s_)
        if (has[s_] && c->xl_nsend[s_] > 0)
            hipLaunchKernelGGL(k_gather_u8, dim3(nblocks(c->xl_nsend[s_], 256)), dim3(256), 0, c->stream, (int)c->xl_nsend[s_], c->xl_send[s_].p, c->plus.p, c->xl_send_buf[s_].p);
    CHK(check_launch(c, "k_gather_u8"));
    NCCLCHK(c, rccl().GroupStart());
    for (int s_ = 0; s_ < 2; ++s_)
        if (has[s_]) {
            if (c->xl_nsend[s_] > 0) NCCLCHK(c, rccl().Send(c->xl_send_buf[s_].p, (size_t)c->xl_nsend[s_], ncclUint8, peer[s_], c->comm, c->stream));
            if (c->xl_nrecv[s_] > 0) NCCLCHK(c, rccl().Recv(c->xl_recv_buf[s_].p, (size_t)c->xl_nrecv[s_], ncclUint8, peer[s_], c->comm, c->stream));
        }
    NCCLCHK(c, rccl().GroupEnd());
    for (int s_ = 0; s_ < 2; ++s_)
        if (has[s_] && c->xl_nrecv[s_] > 0)
            hipLaunchKernelGGL(k_scatter_u8, dim3(nblocks(c->xl_nrecv[s_], 256)), dim3(256), 0, c->stream, (int)c->xl_nrecv[s_], c->xl_recv[s_].p, c->xl_recv_buf[s_].p, c->plus.p);
    return check_launch(c, "k_scatter_u8");
}

int arp_shard_reduce_residue_sets(arp_ctx* c) {
    if (!c) return ARP_E_ARG;
    if (!c->comm) FAIL(c, ARP_E_ARG, "arp_shard_reduce_residue_sets: no communicator (arp_comm_init)");
    if (!c->res_sel.p) FAIL(c, ARP_E_ARG, "arp_shard_reduce_residue_sets: residue sets do not exist yet (run stage 1 first)");
    HIPCHK(c, hipSetDevice(c->device));
    const size_t nb = 2 * (size_t)std::max<int64_t>(c->nres, 1);
    NCCLCHK(c, rccl().AllReduce(c->res_sel.p, c->res_sel.p, nb, ncclUint8, ncclMax, c->comm, c->stream));
    return ARP_OK;
}

#ifdef ARP_SEARCH_TRACE
// developer builds only: where k_search<MODE_CONTACTS> leaves its per-wave trace (device pointer to 4 u64 per wave, 0 = off)
int arp_debug_search_trace(arp_ctx* c, uint64_t device_ptr) {
    if (!c) return ARP_E_ARG;
    HIPCHK(c, hipSetDevice(c->device));
    unsigned long long* p = (unsigned long long*)(uintptr_t)device_ptr;
    HIPCHK(c, hipMemcpyToSymbol(HIP_SYMBOL(g_search_trace), &p, sizeof(p)));
    return ARP_OK;
}
int arp_debug_alloc(uint64_t bytes, uint64_t* device_ptr) {
    void* p = nullptr;
    if (hipMalloc(&p, bytes) != hipSuccess) return ARP_E_HIP;
    (void)hipMemset(p, 0, bytes);
    *device_ptr = (uint64_t)(uintptr_t)p;
    return ARP_OK;
}
int arp_debug_read(uint64_t device_ptr, void* host, uint64_t bytes) {
    return hipMemcpy(host, (const void*)(uintptr_t)device_ptr, bytes, hipMemcpyDeviceToHost) == hipSuccess ? ARP_OK : ARP_E_HIP;
}
#endif

int arp_set_sort_after_pass(arp_ctx* c, int enabled) {
    if (!c) return ARP_E_ARG;
    c->sort_after_pass = enabled != 0;
    return ARP_OK;
}

int arp_set_packed_layout(arp_ctx* c, int layout) {
    if (!c || (layout != ARP_LAYOUT_RECORDS && layout != ARP_LAYOUT_ROWS)) return ARP_E_ARG;
    if (c->packed_csr != (layout == ARP_LAYOUT_ROWS)) void_results(c, RES_LAYOUT);
    c->packed_csr = layout == ARP_LAYOUT_ROWS;
    return ARP_OK;
}

int arp_set_grid_reuse(arp_ctx* c, int enabled) {
    if (!c) return ARP_E_ARG;
    c->grid_reuse = enabled != 0;
    c->cg_valid = false;
    return ARP_OK;
}

int arp_set_compact_lookback(arp_ctx* c, int enabled) {
    if (!c) return ARP_E_ARG;
    c->compact_lookback = enabled != 0;
    c->cg_valid = false;      // (the next pass builds its grid)
    return ARP_OK;
}

int arp_set_whole_structure(arp_ctx* c, int enabled) {
    if (!c) return ARP_E_ARG;
    inputs_changed(c, IN_WHOLE_STRUCTURE);
    c->whole_structure = enabled != 0;
    return ARP_OK;
}

int arp_get_host_times(arp_ctx* c, double us[2], int64_t* passes, int reset) {
    if (!c || !us || !passes) return ARP_E_ARG;
    us[0] = c->host_enqueue_us; us[1] = c->host_wait_us; *passes = c->host_passes;
    if (reset) { c->host_enqueue_us = c->host_wait_us = 0; c->host_passes = 0; }
    return ARP_OK;
}

uint64_t arp_stream_handle(arp_ctx* c) { return c ? (uint64_t)(uintptr_t)c->stream : 0; }

int arp_use_stream(arp_ctx* c, uint64_t stream) {
    if (!c) return ARP_E_ARG;
    HIPCHK(c, hipSetDevice(c->device));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    if (stream == 0) {
        c->stream = c->own_stream;
        c->external_stream = false;
    } else {
        c->stream = (hipStream_t)(uintptr_t)stream;
        c->external_stream = true;
    }
    return ARP_OK;
}

}  // extern "C"


// ---- mmCIF category reader (host only): arp_cif_api.h, shared with the g++-built libarpeggio_host.so ----------------------------
#include "arp_cif_api.h"
