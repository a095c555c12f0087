// arp_networks.h — interaction networks: the connected components of the contact graph, labelled on the device.
//
// Every other derived result is a table of pairs.  This one answers the graph question: which atoms (or residues) hang together
// through the records of the atom-atom bag that take part — one hydrogen-bond network with its waters, the hydrophobic cluster
// a ligand sits in, an ionic cluster.  Nodes are the N resident atoms or, NET_BY_RESIDUE, the N resident residues (a record's
// nodes are then res_id[i], res_id[j]).  A record takes part when (sift & sift_any) != 0 and bit ctype of ctype_mask is set (the
// predicate of arp_filter.h); it is an edge between its two nodes.  A record with a node outside [0, N) — a residue of -1 — is
// left out.  A record whose two nodes are equal counts as an edge of that node and joins nothing.  The ring and amide bags take
// no part.  No record joins two structures of a batch or two models, so no component spans them.
//
// Results: label[v] = the smallest node id of v's component, or -1 for a node no participating record touches; and one row per
// component in ascending root: root, n_nodes, n_edges (participating records, multi-edges counted), sift_or (OR of the whole
// SIFt of those records), ctype_or (OR of 1 << ctype).  Integers, minima, counts and ORs: neither the order of the records nor
// that of the blocks can show.
//
// Nothing is sorted.  The scratch is five int32 per node — parent, n_nodes, n_edges, bits, touched — and one error word:
//   k_net_init    parent[v] = v, the rest 0
//   k_net_hook    one lane per record: mark both nodes touched, then union them lock-free.  The LARGER root always goes under
//                 the smaller one (one atomicCAS on a root's own parent word), so parent[x] <= x holds at every moment, a walk
//                 goes strictly downwards in id, and the final root of a component is its minimum whatever the order of the
//                 unions.  No lane waits for another lane's progress: a lost CAS means another union succeeded on that root.
//                 Paths are halved while they are walked (parent[x] = parent[parent[x]]: an ancestor stays an ancestor, and a
//                 root's word is never stored to, only CASed).
//                 COHERENCE.  The L2s of the XCDs are not coherent with each other and a CU's L1 is never refreshed by another
//                 CU's stores, while the CAS executes at the memory side.  A plain load of parent[] could return a stale "I am a
//                 root" for ever while the CAS on it keeps failing.  So every access to parent[] in this kernel is the CAS or a
//                 relaxed agent-scope atomic load / store (net_load / net_store: the sc1 forms, which bypass L1 and write
//                 through).  The marks are no hand-off: they are stores of the same value, read after the kernel boundary.
//                 BOUNDS.  A walk visits strictly descending ids, so it ends within N steps; a lane loses a CAS once per union
//                 that succeeded on its root, of which a structure has fewer than N and a lane meets a handful.  Both loops
//                 carry a bound they cannot reach (N steps, NET_MAX_RETRIES), and a parent outside [0, x] ends a walk too: the
//                 lane leaves and sets the error word, which turns the count the host waits for negative (k_net_roots).
//   (kernel boundary: parent is final; from here on it is only read, with plain loads)
//   k_net_label   one lane per node: label[v] = its root if touched, else -1; n_nodes[root] += 1
//   k_net_edges   one lane per record: root = label[node of i]; n_edges[root] += 1; bits[root] |= sift | (1 << ctype) << 16
//                 With the all-records masks a structure is normally ONE component: every atomic of both kernels would go to
//                 one address.  So the lanes of a wave with equal root combine first (net_wave_add): per distinct root of the
//                 wave one ballot of equality, one lane's atomicAdd of the popcount and atomicOr of the OR over those lanes.
//                 1 to 3 trips as a rule, at most 64, wave-uniform; no atomic's return value is used.
//   k_net_roots   block t: the roots (label[v] == v) among the nodes of tile t -> tile counts (k_runs_scan sums them: U)
//   (the host reads U — the one wait — and sizes the table)
//   k_net_rows    block t: row prefix[t] + rank in the tile of every root: ascending root by construction
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#define NET_BY_RESIDUE 1u        // ARP_NET_BY_RESIDUE
#define NET_THREADS 256
#define NET_TILE NET_THREADS     // nodes per block of k_net_roots / k_net_rows
#define NET_MAX_RETRIES (1 << 20)
#define NET_POISON (-2147483647 - 1)      // a tile count that makes the sum of all tile counts (< 2^31) negative

struct NetArgs {
    // the bag of the last pass, in the order the pass left it
    const int* ci;
    const int* cj;
    const uint16_t* s_in;
    const uint8_t* ct_in;
    long long k;             // records
    const int* res_id;       // [atoms] (NET_BY_RESIDUE)
    uint32_t sift_any, ctype_mask, flags;
    int N;                   // nodes
    // scratch, [N] each, and the error word
    int* parent;
    int* n_nodes;
    int* n_edges;
    uint32_t* bits;          // SIFt OR | ctype OR << 16
    int* touched;
    int* err;
    int* label;              // [N]: the first result
    // rows
    int* tile_rows;          // [tiles]: roots of tile t, then their exclusive prefix (k_runs_scan)
    long long U;
    int* t_root;
    int* t_nnodes;
    int* t_nedges;
    uint16_t* t_sift;
    uint8_t* t_ctype;
};

__device__ __forceinline__ int net_load(const int* p) { return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }
__device__ __forceinline__ void net_store(int* p, int v) { __hip_atomic_store(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }

// the two nodes of record p when it takes part and both lie in [0, N)
__device__ __forceinline__ bool net_edge(const NetArgs& A, long long p, int* a, int* b) {
    const uint32_t sf = A.s_in[p], ct = A.ct_in[p];
    if ((sf & A.sift_any) == 0u || ((A.ctype_mask >> (ct & 7u)) & 1u) == 0u) return false;
    int i = A.ci[p], j = A.cj[p];
    if (A.flags & NET_BY_RESIDUE) { i = A.res_id[i]; j = A.res_id[j]; }
    *a = i; *b = j;
    return (uint32_t)i < (uint32_t)A.N && (uint32_t)j < (uint32_t)A.N;
}

__global__ __launch_bounds__(NET_THREADS) void k_net_init(NetArgs A) {
    for (long long v = (long long)blockIdx.x * blockDim.x + threadIdx.x; v < A.N; v += (long long)gridDim.x * blockDim.x) {
        A.parent[v] = (int)v;
        A.n_nodes[v] = 0; A.n_edges[v] = 0; A.bits[v] = 0u; A.touched[v] = 0;
    }
    if (blockIdx.x == 0 && threadIdx.x == 0) A.err[0] = 0;
}

// The root of x while unions go on (k_net_hook only), its path halved; -1 when a bound is met.
__device__ __forceinline__ int net_find(int* parent, int x, int N) {
    for (int step = 0; step <= N; ++step) {
        const int p = net_load(parent + x);
        if (p == x) return x;
        if ((uint32_t)p > (uint32_t)x) return -1;
        const int g = net_load(parent + p);
        if (g == p) return p;
        if ((uint32_t)g > (uint32_t)p) return -1;
        net_store(parent + x, g);      // (x is no root and never becomes one again; g is an ancestor of x)
        x = g;
    }
    return -1;
}

__global__ __launch_bounds__(NET_THREADS) void k_net_hook(NetArgs A) {
    for (long long p = (long long)blockIdx.x * blockDim.x + threadIdx.x; p < A.k; p += (long long)gridDim.x * blockDim.x) {
        int a, b;
        if (!net_edge(A, p, &a, &b)) continue;
        A.touched[a] = 1; A.touched[b] = 1;
        bool joined = a == b;
        for (int t = 0; !joined && t < NET_MAX_RETRIES; ++t) {
            const int ra = net_find(A.parent, a, A.N), rb = net_find(A.parent, b, A.N);
            if (ra < 0 || rb < 0) break;
            if (ra == rb) { joined = true; break; }
            const int lo = min(ra, rb), hi = max(ra, rb);
            if (atomicCAS(A.parent + hi, hi, lo) == hi) { joined = true; break; }
            a = hi; b = lo;            // hi got another parent meanwhile: go on from the two roots
        }
        if (!joined) atomicOr(A.err, 1);
    }
}

// Per distinct key of the wave's lanes with on: ONE lane adds the number of those lanes to count[key] and — bits != nullptr — ORs
// the OR of their values into bits[key].  Called by all lanes of the wave.
__device__ __forceinline__ void net_wave_add(bool on, int key, uint32_t val, int* count, uint32_t* bits) {
    const int lane = threadIdx.x & 63;
    unsigned long long todo = __ballot(on);
    while (todo) {                     // (wave-uniform)
        const int lead = __ffsll((long long)todo) - 1;
        const int k0 = __shfl(key, lead);
        const bool mine = on && key == k0;
        const unsigned long long m = __ballot(mine);
        uint32_t v = mine ? val : 0u;
        if (bits) {
#pragma unroll
            for (int o = 32; o > 0; o >>= 1) v |= __shfl_xor(v, o);
        }
        if (lane == lead) {
            atomicAdd(count + k0, __popcll(m));
            if (bits) atomicOr(bits + k0, v);
        }
        on = on && !mine;
        todo &= ~m;
    }
}

__global__ __launch_bounds__(NET_THREADS) void k_net_label(NetArgs A) {
    const long long stride = (long long)gridDim.x * blockDim.x;
    for (long long base = (long long)blockIdx.x * blockDim.x; base < A.N; base += stride) {      // (block-uniform trip count)
        const long long v = base + threadIdx.x;
        const bool on = v < A.N && A.touched[v] != 0;
        int x = on ? (int)v : 0;
        bool bad = false;
        if (on) {
            int step = 0;
            for (; step <= A.N; ++step) {
                const int p = A.parent[x];
                if (p == x) break;
                if ((uint32_t)p > (uint32_t)x) { bad = true; break; }
                x = p;
            }
            bad = bad || step > A.N;
        }
        if (v < A.N) A.label[v] = on && !bad ? x : -1;
        if (bad) atomicOr(A.err, 1);
        net_wave_add(on && !bad, x, 0u, A.n_nodes, nullptr);
    }
}

__global__ __launch_bounds__(NET_THREADS) void k_net_edges(NetArgs A) {
    const long long stride = (long long)gridDim.x * blockDim.x;
    for (long long base = (long long)blockIdx.x * blockDim.x; base < A.k; base += stride) {      // (block-uniform trip count)
        const long long p = base + threadIdx.x;
        int a = 0, b = 0;
        bool on = p < A.k && net_edge(A, p, &a, &b);
        int root = on ? A.label[a] : 0;
        if (on && (uint32_t)root >= (uint32_t)A.N) { on = false; atomicOr(A.err, 1); }      // (a touched node has a label)
        const uint32_t val = on ? (uint32_t)A.s_in[p] | (1u << (A.ct_in[p] & 7u)) << 16 : 0u;
        net_wave_add(on, root, val, A.n_edges, A.bits);
    }
}

__global__ __launch_bounds__(NET_THREADS) void k_net_roots(NetArgs A) {
    __shared__ int s_w[NET_THREADS / 64];
    const long long v = (long long)blockIdx.x * NET_TILE + threadIdx.x;
    const unsigned long long m = __ballot(v < A.N && A.label[v] == (int)v);
    if ((threadIdx.x & 63) == 0) s_w[threadIdx.x >> 6] = __popcll(m);
    __syncthreads();
    if (threadIdx.x == 0) {
        int t = 0;
        for (int w = 0; w < NET_THREADS / 64; ++w) t += s_w[w];
        A.tile_rows[blockIdx.x] = blockIdx.x == 0 && A.err[0] != 0 ? NET_POISON : t;
    }
}

__global__ __launch_bounds__(NET_THREADS) void k_net_rows(NetArgs A) {
    __shared__ int s_w[NET_THREADS / 64];
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    const long long v = (long long)blockIdx.x * NET_TILE + threadIdx.x;
    const bool root = v < A.N && A.label[v] == (int)v;
    const unsigned long long m = __ballot(root);
    if (lane == 0) s_w[w] = __popcll(m);
    __syncthreads();
    long long row = A.tile_rows[blockIdx.x];
    for (int q = 0; q < w; ++q) row += s_w[q];
    row += __popcll(m & ((1ull << lane) - 1ull));
    if (root && row < A.U) {           // (row < U always: U is the sum of the same counts)
        const uint32_t bits = A.bits[v];
        A.t_root[row] = (int)v;
        A.t_nnodes[row] = A.n_nodes[v];
        A.t_nedges[row] = A.n_edges[v];
        A.t_sift[row] = (uint16_t)(bits & 0xFFFFu);
        A.t_ctype[row] = (uint8_t)(bits >> 16);
    }
}
