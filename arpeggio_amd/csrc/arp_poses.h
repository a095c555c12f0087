// arp_poses.h — ligand poses on a resident receptor: every pose's ligand - receptor contacts in one launch.
//
// A single structure is resident with an uploaded selection of S <= POSES_MAX_ATOMS atoms, the MOVABLE SET.  A pose gives new
// coordinates for those atoms (float32) and for their hydrogens (float64); everything else — the receptor, its static record
// columns, their cell order (ensure_static) — stays where it is.  For pose p the kernel emits exactly the atom-atom records
// with one selected and one unselected atom that a pass over the structure with the pose scattered in would emit: same
// filters (k_search, MODE_CONTACTS), same decision (stage A and B of sift_body, I:715-936), same float32 distance bits.
//
//   k_poses_movable   once per (structure, selection): where the hydrogens of selected atom s begin among the pose's hydrogen
//                     rows (h_off order, parents selected), their number SH, and the position s of every selected local id
//   k_poses_contacts  one block per pose, one wave per selected atom at a time: the 27 cells around the pose atom in the
//                     resident cell order, filters, decision, records appended as (key, payload) for the radix sort of
//                     arp_sort.h, and the per-pose summary (records per SIFt bit, total) reduced in LDS: one store per pose.
//                     Its record queue, cell walk, resident partner and summary are the inline pieces (pose_queue_*,
//                     pose_cell_rows, pose_resident_atom, PoseCounts) that k_library_contacts of arp_library.h uses too
//   k_pose_columns    the sorted (key, payload) pairs as the five columns (of a library result as well)
//   k_poses_offsets   pose_off[p] = exclusive prefix of the summaries' totals (block t: of slot first_slot + t; the poses-planes
//                     result launches it too, a block per table)
//
// The key is pose << 2 b | i << b | j with b = the bits of the largest packed id (b <= 21), i < j packed ids: its order is
// ascending (pose, i, j), the order of the result.  Limits that follow: n < 2^21 atoms (POSES_MAX_N), at most 2^20 poses a
// launch (POSES_MAX_POSES: 20 + 42 bits); the host refuses beyond them and callers chunk their poses.
//
// What moves with a pose: a selected atom's coordinate, its hydrogens, and — for either atom of a pair — the coordinate of
// its single-bond neighbour when that neighbour (the resident sb_nbr index says which atom it is) is itself selected
// (halogen_weak and xbond).  The two shortcuts of k_sift that rest on the RESIDENT coordinates are not taken here: the covalent
// test is membership in the bond list at any distance (I:748-757, no longest_bond gate: a pose may stretch a bond), and no
// hydrogen loop is skipped for reach (no h_slack: a pose may stretch an X-H distance).  Both only saved work.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "arp_pairs.h"
#include "arp_runs.h"

#define POSES_MAX_ATOMS 1024
#define POSES_MAX_POSES (1 << 20)
#define POSES_MAX_N (1 << 21)
#define POSES_THREADS 256
#define POSES_WAVES (POSES_THREADS / 64)
#define POSES_QCAP 256
#define POSES_SUMMARY 16

// Where a launch's records go: the unsorted (key, payload) buffers with their capacity, the exact count (also beyond cap), the
// per-pose summary rows and the device's error word
struct PoseSink {
    u64* key;
    u64* val;
    u64 cap;
    u64* count;
    uint32_t* summary;          // [poses][16]
    int* err;
};

struct PoseArgs {
    int n, S, P;
    long long SH;
    // the movable set
    const int* sel_list;        // [S] local ids, ascending
    const int* sel_h;           // [S + 1] first hydrogen row of selected atom s among a pose's SH rows
    const int* pos_of;          // [n] position in sel_list, -1: not selected
    const uint8_t* sel;         // [n] the uploaded selection
    // the poses
    const float* pxyz;          // [P][S][3]
    const double* phx;          // [P][SH][3]
    // resident, by local id
    const float4* st_xyzm;
    const int4* st_aux;
    const int4* st_qa;
    const int* h_off;
    const double2* rad;
    const float4* sb;           // single-bond neighbour: x, y, z, present
    const int* sb_nbr;          // ... and which atom it is (-1: none)
    const int* bond_off;
    const int* bond_idx;
    const double* h_xyz;
    // the receptor in cell order
    const float4* sp_xyzm;
    const int4* sp_aux;
    const int4* sp_qa;
    const int* sp_h;
    const int* start;           // [ncell + 1]
    GridDesc g;
    double r2, comp;
    int include_seq_adj;
    int idbits;
    PoseSink out;
};

__global__ __launch_bounds__(1024) void k_poses_movable(int S, const int* __restrict__ sel_list, const int* __restrict__ h_off,
                                                        int* __restrict__ sel_h, int* __restrict__ pos_of) {
    __shared__ int s_w[16];
    const int s = threadIdx.x, lane = s & 63, wv = s >> 6;
    int lid = -1, cnt = 0;
    if (s < S) {
        lid = sel_list[s];
        cnt = h_off[lid + 1] - h_off[lid];
        pos_of[lid] = s;
    }
    int incl = cnt;
#pragma unroll
    for (int off = 1; off < 64; off <<= 1) {
        const int u = __shfl_up(incl, off);
        if (lane >= off) incl += u;
    }
    if (lane == 63) s_w[wv] = incl;
    __syncthreads();
    int before = 0;
    for (int k = 0; k < wv; ++k) before += s_w[k];
    if (s < S) sel_h[s] = before + incl - cnt;
    if (s == S - 1) sel_h[S] = before + incl;
}

// One atom of a pair as the decision reads it: a moved atom's coordinate and hydrogens are the pose's, everything else is resident
struct PoseAtom {
    num::f3 x;
    uint32_t m;                 // meta word, M_SEL set for a selected atom
    int lid;
    int4 qa;                    // local id, bonded neighbours in other residues (st_qa / sp_qa)
    const double* hx;           // the hydrogen rows h0 .. h1 are in
    int h0, h1;
};

// a if c, else b, field by field (no address is taken: the atoms stay in registers)
__device__ __forceinline__ PoseAtom pose_pick(bool c, const PoseAtom& a, const PoseAtom& b) {
    PoseAtom r;
    r.x = {c ? a.x.x : b.x.x, c ? a.x.y : b.x.y, c ? a.x.z : b.x.z};
    r.m = c ? a.m : b.m;
    r.lid = c ? a.lid : b.lid;
    r.qa = make_int4(c ? a.qa.x : b.qa.x, c ? a.qa.y : b.qa.y, c ? a.qa.z : b.qa.z, c ? a.qa.w : b.qa.w);
    r.hx = c ? a.hx : b.hx;
    r.h0 = c ? a.h0 : b.h0;
    r.h1 = c ? a.h1 : b.h1;
    return r;
}

// the single-bond neighbour of atom a in pose `pose`: the pose's coordinate when that neighbour is itself a moved atom
__device__ __forceinline__ float4 pose_sb(const PoseArgs& A, int pose, int a) {
    float4 v = A.sb[a];
    if (v.w != 0.0f) {
        const int k = A.sb_nbr[a];
        const int s = (k >= 0 && k < A.n) ? A.pos_of[k] : -1;
        if (s >= 0) {
            const float* p = A.pxyz + ((size_t)pose * A.S + s) * 3;
            v.x = p[0]; v.y = p[1]; v.z = p[2];
        }
    }
    return v;
}

// How k_poses_contacts reads what the decision needs beside the two atoms: everything by local id from the resident arrays, a
// single-bond neighbour's coordinate from the pose when that neighbour moved.  (The ligand library, arp_library.h, gives
// pose_pair_sift another reader: its ligand side is staged in LDS and is never bonded to the receptor.)
struct PoseResidentReader {
    const PoseArgs& A;
    __device__ __forceinline__ double comp() const { return A.comp; }
    __device__ __forceinline__ int* err() const { return A.out.err; }
    // {vdw, cov} of bgn (of_b) or end
    __device__ __forceinline__ double2 rad(const PoseAtom& a, bool) const { return A.rad[a.lid]; }
    // the single-bond neighbour of bgn (of_b) or end: x, y, z, present
    __device__ __forceinline__ float4 sb(int pose, const PoseAtom& B, const PoseAtom& E, bool of_b) const { return pose_sb(A, pose, of_b ? B.lid : E.lid); }
    // interactions.py:748-757: end among the bonded neighbours of bgn, at ANY distance (neighbours of bgn's own residue are not in
    // qa, and a pair of one residue never gets here: I:729)
    __device__ __forceinline__ bool bonded(const PoseAtom& B, int e) const {
        const unsigned nx_ = min(min((unsigned)(B.qa.y ^ e), (unsigned)(B.qa.z ^ e)), (unsigned)(B.qa.w ^ e));
        bool cov = nx_ == 0u;
        if (!cov && B.qa.w == -2) {
            for (int k = A.bond_off[B.lid], k1 = A.bond_off[B.lid + 1]; k < k1; ++k)
                if (A.bond_idx[k] == e) { cov = true; break; }
        }
        return cov;
    }
};

// The decision for one accepted pair (B = bgn, the lower packed id; d = its float32 distance): the SIFt mask and, in *ct_out, the
// contact type.  It follows interactions.py:715-936 line by line as sift_body does — stage A's straight-line mask code, then the
// hydrogen geometry of sift_geometry — with the pose's coordinates wherever an atom, a hydrogen or a single-bond neighbour moved.
// R says how an atom's radii, its single-bond neighbour and the bonded-neighbour test are read (PoseResidentReader above,
// LibraryReader in arp_library.h): the one statement of the decision serves both kernels.
template <class Reader>
__device__ __forceinline__ uint32_t pose_pair_sift(const Reader& R, int pose, const PoseAtom& B, const PoseAtom& E, float d, int* ct_out) {
    const num::f3 xb = B.x, xe = E.x;
    const uint32_t mb = B.m, me = E.m;
    const uint32_t tb = mb & M_TMASK, te = me & M_TMASK;
    const uint32_t bw = (mb / M_WATER) & 1u, ew = (me / M_WATER) & 1u;
    // interactions.py:643-691 (__get_contact_type)
    const uint32_t ct_idx = ((mb / M_SEL) & 1u) | (((me / M_SEL) & 1u) << 1) | (bw << 2) | (ew << 3);
    *ct_out = (int)((contact_type_table() >> (4u * ct_idx)) & 15ull);
    // interactions.py:717-718 and the casts of 756-773
    const double2 rb = R.rad(B, true), re = R.rad(E, false);      // {vdw, cov}
    const double sum_vdw = rb.x + re.x;
    const float f_sum_cov = (float)(rb.y + re.y), f_sum_vdw = (float)sum_vdw, f_vdw_comp = (float)(sum_vdw + R.comp());
    // interactions.py:756-773: an exclusive ladder
    uint32_t s = ARP_S_PROXIMAL;
    s = (d <= f_vdw_comp) ? ARP_S_VDW : s;
    s = (d < f_sum_vdw) ? ARP_S_VDW_CLASH : s;
    s = (d < f_sum_cov) ? ARP_S_CLASH : s;
    // interactions.py:777-783: an hbond acceptor beside a metal
    const uint32_t metal = ((tb & (me >> 12)) | (te & (mb >> 12))) & 1u;
    const uint32_t s_metal = (d <= (float)2.8) ? metal * ARP_S_METAL_COMPLEX : 0u;
    // the type tests of I:791-921 (X bit k = bgn has k + 1 and end has k, Y the same with the atoms exchanged)
    const uint32_t X = (tb >> 1) & te, Y = (te >> 1) & tb, XY = X | Y;
    const bool in_vc = d <= f_vdw_comp, d35 = d <= (float)3.5;
    // interactions.py:791-819: water rule, else donor / acceptor (if / elif)
    const uint32_t wb = bw & (in_vc ? 1u : 0u), we = ew & (in_vc ? 1u : 0u) & ~wb;
    const uint32_t nowat = (wb | we) ^ 1u;
    const uint32_t hb_w = (wb & (((te & 3u) != 0u) ? 1u : 0u)) | (we & (((tb & 3u) != 0u) ? 1u : 0u));
    const uint32_t c1 = nowat & X & 1u, c2 = nowat & ~X & Y & 1u;
    // interactions.py:857-886: the four weak branches
    const uint32_t n4 = tb & (te >> 5) & 1u, n8 = (tb >> 5) & te & 1u;
    const uint32_t n16 = (tb >> 4) & (mb >> 13) & (((te & 0x22u) != 0u) ? 1u : 0u) & 1u;
    const uint32_t n32 = (te >> 4) & (me >> 13) & (((tb & 0x22u) != 0u) ? 1u : 0u) & 1u;
    unsigned need_ = c1 | (c2 << 1) | (n4 << 2) | (n8 << 3) | (n16 << 4) | (n32 << 5);
    uint32_t f = hb_w * (ARP_S_HBOND | ARP_S_POLAR);
    f |= (d35 & ((c1 | c2) != 0u)) ? ARP_S_POLAR : 0u;                       // I:806, 814
    f |= (d35 & ((need_ & 60u) != 0u)) ? ARP_S_WEAK_POLAR : 0u;               // I:861, 869, 877, 885
    // interactions.py:898-921: ionic, carbonyl, aromatic, hydrophobic, each behind its distance
    const uint32_t near4 = ((XY & 0x40u) << 2) | ((tb & te & ARP_T_AROMATIC) >> 1);
    f |= (d <= (float)4.0) ? near4 : 0u;
    f |= (d <= (float)3.6) ? ((XY & 0x200u) << 3) : 0u;
    f |= (tb & te & ARP_T_HYDROPHOBE) << 3;
    {
        // branches that cannot succeed whatever the pose: the donor has no hydrogen, the halogen no single-bond neighbour
        // (U:139-141).  No reach test: the longest atom - hydrogen distance of the structure bounds the resident hydrogens only.
        const bool no_hb = !(mb & M_HAS_H), no_he = !(me & M_HAS_H);
        unsigned dead = 0;
        dead |= no_hb ? (1u | 8u | 32u) : 0u;               // hydrogens of bgn, target = end
        dead |= no_he ? (2u | 4u | 16u) : 0u;               // hydrogens of end, target = bgn
        dead |= (mb & M_HAS_SB) ? 0u : 16u;
        dead |= (me & M_HAS_SB) ? 0u : 32u;
        need_ = ((need_ & ~dead) == 0u) ? 0u : need_;
    }
    // interactions.py:748-757: end among the bonded neighbours of bgn, at ANY distance
    const bool cov = R.bonded(B, E.lid);
    s = cov ? ARP_S_COVALENT : s;
    s |= s_metal;
    // interactions.py:786: feature flags only for pairs that do not clash (covalent ones do get them) within 4.5 A
    const bool feat = !(s & ARP_S_CLASH) & (d <= (float)4.5);
    s |= feat ? f : 0u;
    const unsigned need = feat ? need_ : 0u;
    // interactions.py:889-895 (halogen bond: float32 angle at the donor)
    if (feat & in_vc & ((XY & 4u) != 0u)) {
        if (X & 4u) { if (xbond(R.sb(pose, B, E, true), xb, xe, R.err())) s |= ARP_S_XBOND; }
        else if (xbond(R.sb(pose, B, E, false), xe, xb, R.err())) s |= ARP_S_XBOND;
    }
    if (need) {
        // the hydrogen geometry (sift_geometry): branch k of
        //   0 is_hbond(bgn, end)   1 is_hbond(end, bgn)          (if / elif, I:804-819)
        //   2 is_weak_hbond(end, bgn)   3 is_weak_hbond(bgn, end)   4 / 5 is_halogen_weak_hbond  (I:857-886)
        unsigned todo = need, res = 0;
        while (todo) {
            const int kind = __ffs(todo) - 1;
            todo &= todo - 1;
            bool r;
            if (kind < 4) {
                const bool donor_b = (kind == 0) || (kind == 3);
                const double clast = (kind < 2) ? ARP_COS_LAST_GE_1_57 : ARP_COS_LAST_GE_2_27;
                const double cmin = (kind < 2) ? ARP_COS_1_57 : ARP_COS_2_27;
                r = hbond_like(donor_b ? xb : xe, donor_b ? B.hx : E.hx, donor_b ? B.h0 : E.h0, donor_b ? B.h1 : E.h1, donor_b ? xe : xb,
                               donor_b ? re.x : rb.x, R.comp(), cmin, clast);
            } else {
                const bool hal_b = kind == 4;
                r = halogen_weak(hal_b ? xb : xe, R.sb(pose, B, E, hal_b), hal_b ? rb.x : re.x, hal_b ? E.hx : B.hx,
                                 hal_b ? E.h0 : B.h0, hal_b ? E.h1 : B.h1, R.comp());
            }
            res |= (r ? 1u : 0u) << kind;
        }
        if (res & 3u) s |= ARP_S_HBOND;
        // the LAST applicable weak branch decides SIFt[6] (every branch overwrites it)
        if (need & 60u) {
            const int last = 31 - __clz((int)(need & 60u));
            if ((res >> last) & 1u) s |= ARP_S_WEAK_HBOND;
        }
    }
    return s;
}

// ---- what k_poses_contacts and k_library_contacts (arp_library.h) share.  Every piece is inlined and only scalars cross its
// boundary: a helper that takes or returns the nine-row arrays of the walk gives both kernels scratch, so the
// nine-entry fill and the position select stay in the kernels.

// The per-pose summary: records per SIFt bit and, in the last slot, all of them.  A wave counts by ballot (add, mp != 0 the
// ballot of pass); at the end of the pose lane 0 of every wave adds into s_sum (zeroed by the block before) and the block
// stores the row (store: every thread calls it)
struct PoseCounts {
    uint32_t c[POSES_SUMMARY];
    __device__ __forceinline__ void clear() {
#pragma unroll
        for (int b = 0; b < POSES_SUMMARY; ++b) c[b] = 0u;
    }
    __device__ __forceinline__ void add(unsigned long long mp, bool pass, uint32_t sft) {
#pragma unroll
        for (int b = 0; b < POSES_SUMMARY - 1; ++b) c[b] += (uint32_t)__popcll(__ballot(pass && ((sft >> b) & 1u)));
        c[POSES_SUMMARY - 1] += (uint32_t)__popcll(mp);
    }
    __device__ __forceinline__ void store(uint32_t* s_sum, int lane, uint32_t* row) const {
        if (lane == 0) {
#pragma unroll
            for (int b = 0; b < POSES_SUMMARY; ++b)
                if (c[b]) atomicAdd(&s_sum[b], c[b]);
        }
        __syncthreads();
        if (threadIdx.x < POSES_SUMMARY) row[threadIdx.x] = s_sum[threadIdx.x];
        __syncthreads();      // (the next pose clears s_sum)
    }
};

// The per-wave record queue: qk / qv are the wave's rows (POSES_QCAP entries each) of the kernel's LDS arrays, qn what they hold.
// flush: the queued records leave with one atomic of lane 0
__device__ __forceinline__ void pose_queue_flush(const PoseSink& o, const u64* qk, const u64* qv, int& qn, int lane) {
    __builtin_amdgcn_wave_barrier();
    u64 base = 0;
    if (lane == 0) base = atomicAdd(o.count, (u64)qn);
    base = __shfl(base, 0);
    for (int k = lane; k < qn; k += 64)
        if (base + k < o.cap) { o.key[base + k] = qk[k]; o.val[base + k] = qv[k]; }
    __builtin_amdgcn_wave_barrier();
    qn = 0;
}
// push: the survivors of one ballot (mp != 0) take consecutive slots and are counted; a queue that could not take 64 more is flushed
__device__ __forceinline__ void pose_queue_push(const PoseSink& o, u64* qk, u64* qv, int& qn, PoseCounts& cnt, int lane, unsigned long long mp, bool pass,
                                                u64 key, u64 val, uint32_t sft) {
    if (pass) {
        const int slot = qn + __popcll(mp & ((1ull << lane) - 1ull));
        qk[slot] = key;
        qv[slot] = val;
    }
    cnt.add(mp, pass, sft);
    qn += __popcll(mp);
    if (qn > POSES_QCAP - 64) pose_queue_flush(o, qk, qv, qn, lane);
}
// end of block (every thread calls it): what is left in the per-wave queues leaves with ONE atomic
__device__ __forceinline__ void pose_queue_drain(const PoseSink& o, const u64* qk, const u64* qv, int qn, int lane, int w, int* s_qn, u64* s_base) {
    if (lane == 0) s_qn[w] = qn;
    __syncthreads();
    if (threadIdx.x == 0) {
        int tot = 0;
        for (int k = 0; k < POSES_WAVES; ++k) tot += s_qn[k];
        *s_base = tot > 0 ? atomicAdd(o.count, (u64)tot) : 0ull;
    }
    __syncthreads();
    if (qn > 0) {
        u64 base = *s_base;
        for (int k = 0; k < w; ++k) base += (u64)s_qn[k];
        for (int k = lane; k < qn; k += 64)
            if (base + k < o.cap) { o.key[base + k] = qk[k]; o.val[base + k] = qv[k]; }
    }
}

// The cell walk around a pose atom, per lane: the 27 cells around it, clamped to the grid.  A pose may lie outside the receptor's
// box: an atom a whole cell (>= the cutoff) beyond a face has no partner (inside = false).  Else nine rows of up to three
// x-neighbours, each a contiguous range of the cell order: lane r < 9 holds row r — its first position, its length, and the
// candidates up to and including it (lane 8: all of them)
struct PoseRow { int beg, len, incl; bool inside; };
__device__ __forceinline__ PoseRow pose_cell_rows(const GridDesc& g, const int* __restrict__ start, int n, float px, float py, float pz, int lane) {
    PoseRow R{0, 0, 0, false};
    const int cx = cell_coord_raw((double)px, g.ox, g.inv, g.nx), cy = cell_coord_raw((double)py, g.oy, g.inv, g.ny),
              cz = cell_coord_raw((double)pz, g.oz, g.inv, g.nz);
    if (cx < -1 || cx > g.nx || cy < -1 || cy > g.ny || cz < -1 || cz > g.nz) return R;
    R.inside = true;
    const int x0 = max(cx - 1, 0), x1 = min(cx + 1, g.nx - 1);
    if (lane < 9) {
        const int z = cz - 1 + lane / 3, y = cy - 1 + lane % 3;
        if (z >= 0 && z < g.nz && y >= 0 && y < g.ny && x0 <= x1) {
            const int row = (z * g.ny + y) * g.nx;
            const int b0 = start[row + x0], b1 = start[row + x1 + 1];
            R.beg = min(max(b0, 0), n);
            R.len = max(min(b1, n) - R.beg, 0);
        }
    }
    R.incl = R.len;
#pragma unroll
    for (int off = 1; off < 16; off <<= 1) {
        const int u = __shfl_up(R.incl, off);
        if (lane >= off) R.incl += u;
    }
    return R;
}

// The resident atom at position pos of the cell order as the decision reads it (v / aj: its sp_xyzm / sp_aux rows): its hydrogens
// are the resident rows from sp_h on, as many as the meta word counts — or, at M_HCNT_ESC, up to the next atom's first row
__device__ __forceinline__ PoseAtom pose_resident_atom(int pos, const float4& v, const int4& aj, const int4* __restrict__ sp_qa,
                                                       const int* __restrict__ sp_h, const int* __restrict__ h_off, const double* h_xyz) {
    const uint32_t mj = __float_as_uint(v.w);
    PoseAtom J;
    J.x = xyz_of(v); J.m = mj; J.lid = aj.x; J.qa = sp_qa[pos]; J.hx = h_xyz;
    J.h0 = sp_h[pos];
    const unsigned hc = (mj >> M_HCNT_SHIFT) & 3u;
    J.h1 = (mj & M_HAS_H) ? J.h0 + 1 + (int)hc : J.h0;
    if ((mj & M_HAS_H) && hc == M_HCNT_ESC) J.h1 = h_off[aj.x + 1];
    return J;
}

__global__ __launch_bounds__(POSES_THREADS) void k_poses_contacts(PoseArgs A) {
    __shared__ u64 q_key[POSES_WAVES][POSES_QCAP], q_val[POSES_WAVES][POSES_QCAP];
    __shared__ uint32_t s_sum[POSES_SUMMARY];
    __shared__ int s_qn[POSES_WAVES];
    __shared__ u64 s_base;
    const int lane = threadIdx.x & 63, w = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    const GridDesc g = A.g;
    int qn = 0;
    for (int pose = blockIdx.x; pose < A.P; pose += gridDim.x) {
        if (threadIdx.x < POSES_SUMMARY) s_sum[threadIdx.x] = 0u;
        __syncthreads();
        PoseCounts cnt;
        cnt.clear();
        const double* const phx = A.phx + (size_t)pose * (size_t)A.SH * 3;
        for (int s = w; s < A.S; s += POSES_WAVES) {
            const int lid = A.sel_list[s];
            const float* const pp = A.pxyz + ((size_t)pose * A.S + s) * 3;
            const float px = pp[0], py = pp[1], pz = pp[2];
            const int ph0 = A.sel_h[s], ph1 = A.sel_h[s + 1];
            // non-finite pose coordinates: the atom's own and its hydrogens' (every row of a pose belongs to one selected atom)
            bool bad = !(isfinite(px) && isfinite(py) && isfinite(pz));
            for (int k = 3 * ph0 + lane; k < 3 * ph1; k += 64) bad |= !isfinite(phx[k]);
            if (__any(bad)) {
                if (lane == 0) atomicExch(A.out.err, ARP_E_ARG);
                continue;
            }
            const uint32_t mh = __float_as_uint(A.st_xyzm[lid].w) | M_SEL;
            if (mh & M_HYDROGEN) continue;                               // I:712
            const int4 ah = A.st_aux[lid];
            const PoseRow row = pose_cell_rows(g, A.start, A.n, px, py, pz, lane);
            if (!row.inside) continue;
            const int total = __shfl(row.incl, 8);
            int rb_[9], re_[9];      // start of row r minus the candidates before it; candidates up to and including row r
#pragma unroll
            for (int r = 0; r < 9; ++r) {
                const int i_ = __shfl(row.incl, r), l_ = __shfl(row.len, r), b_ = __shfl(row.beg, r);
                re_[r] = i_;
                rb_[r] = b_ - (i_ - l_);
            }
            const num::d3 pd = {(double)px, (double)py, (double)pz};
            for (int base = 0; base < total; base += 64) {
                const int k = base + lane;
                int dlt = rb_[0];
#pragma unroll
                for (int r = 1; r < 9; ++r) dlt = (k >= re_[r - 1]) ? rb_[r] : dlt;
                const int pos = dlt + k;
                bool pass = k < total && pos >= 0 && pos < A.n;
                float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
                int4 aj = make_int4(0, 0, 0, 0);
                if (pass) {
                    v = A.sp_xyzm[pos];
                    aj = A.sp_aux[pos];
                }
                const uint32_t mj = __float_as_uint(v.w);
                if (pass) {
                    pass = !(mj & M_HYDROGEN) && (unsigned)aj.x < (unsigned)A.n && !A.sel[aj.x];
                    pass = pass && num::dist2_kd(pd, num::d3{(double)v.x, (double)v.y, (double)v.z}) <= A.r2;
                }
                bool h_first = false;
                if (pass) {
                    // the filters of k_search, MODE_CONTACTS: bgn = the lower packed index; I:729 same residue; I:733-741
                    // sequence-adjacent residues, res_end's polypeptide flag read after orientation (I:734)
                    h_first = ah.x < aj.x;
                    const uint32_t m_end = h_first ? mj : mh;
                    const unsigned adj = min(min((unsigned)(ah.w ^ aj.y), (unsigned)(ah.z ^ aj.y)), min((unsigned)(aj.w ^ ah.y), (unsigned)(aj.z ^ ah.y)));
                    const unsigned gate = (A.include_seq_adj ? 0u : 1u) & ((m_end & M_RES_POLY) ? 1u : 0u) & ((mh & mj & M_RES_HASSEQ) ? 1u : 0u);
                    const unsigned drop = (ah.y == aj.y ? 1u : 0u) | (gate & (adj == 0u ? 1u : 0u));
                    pass = drop == 0u;
                }
                uint32_t sft = 0;
                u64 key = 0, val = 0;
                if (pass) {
                    PoseAtom H;
                    H.x = {px, py, pz}; H.m = mh; H.lid = lid; H.qa = A.st_qa[lid]; H.hx = phx; H.h0 = ph0; H.h1 = ph1;
                    const PoseAtom J = pose_resident_atom(pos, v, aj, A.sp_qa, A.sp_h, A.h_off, A.h_xyz);
                    const PoseAtom Bg = pose_pick(h_first, H, J), En = pose_pick(h_first, J, H);
                    const float d = num::norm(num::sub(Bg.x, En.x));                    // interactions.py:745
                    int ct = 0;
                    sft = pose_pair_sift(PoseResidentReader{A}, pose, Bg, En, d, &ct);
                    key = ((u64)(unsigned)pose << (2 * A.idbits)) | ((u64)(unsigned)Bg.lid << A.idbits) | (u64)(unsigned)En.lid;
                    val = (u64)__float_as_uint(d) | ((u64)sft << 32) | ((u64)(unsigned)ct << 48);
                }
                const unsigned long long mp = __ballot(pass);
                if (mp) pose_queue_push(A.out, q_key[w], q_val[w], qn, cnt, lane, mp, pass, key, val, sft);
            }
        }
        cnt.store(s_sum, lane, A.out.summary + (size_t)pose * POSES_SUMMARY);
    }
    pose_queue_drain(A.out, q_key[w], q_val[w], qn, lane, w, s_qn, &s_base);
}

// Block t: pose_off[t][p] = what slot first_slot + t of the summary rows (POSES_SUMMARY words each) counts in the poses before p,
// pose_off[t][P] = in all of them (scan_round, arp_runs.h).  The poses result: one block on its last slot, the records of a
// pose; the poses-planes result (arp_poses_planes.h, rows of as many words): four blocks on slots 0 ... 3, its tables' counts.
__global__ __launch_bounds__(1024) void k_poses_offsets(int P, int first_slot, const uint32_t* __restrict__ summary, u64* __restrict__ pose_off) {
    __shared__ u64 s_w[16];
    const int t = (int)blockIdx.x;
    u64* const out = pose_off + (size_t)t * ((size_t)P + 1);
    u64 carry = 0;
    for (int p0 = 0; p0 < P; p0 += 1024) {
        const int p = p0 + (int)threadIdx.x;
        const u64 before = scan_round(p < P ? (u64)summary[(size_t)p * POSES_SUMMARY + first_slot + t] : 0ull, s_w, carry);
        if (p < P) out[p] = before;
    }
    if (threadIdx.x == 0) out[P] = carry;
}

// The sorted (key, payload) pairs as the result's five columns: the first id column is the key's hi_bits above its lowest
// lo_bits, the second those lowest bits (a poses result: idbits twice; a library result, arp_library.h: ibits and abits)
__global__ __launch_bounds__(256) void k_pose_columns(long long k, int hi_bits, int lo_bits, const u64* __restrict__ key, const u64* __restrict__ val,
                                                      int* __restrict__ c0, int* __restrict__ c1, float* __restrict__ cd,
                                                      uint16_t* __restrict__ cs, uint8_t* __restrict__ cct) {
    const u64 hi_mask = (1ull << hi_bits) - 1ull, lo_mask = (1ull << lo_bits) - 1ull;
    for (long long p = (long long)blockIdx.x * blockDim.x + threadIdx.x; p < k; p += (long long)gridDim.x * blockDim.x) {
        const u64 kk = key[p], v = val[p];
        c0[p] = (int)((kk >> lo_bits) & hi_mask);
        c1[p] = (int)(kk & lo_mask);
        cd[p] = __uint_as_float((uint32_t)v);
        cs[p] = (uint16_t)(v >> 32);
        cct[p] = (uint8_t)(v >> 48);
    }
}
