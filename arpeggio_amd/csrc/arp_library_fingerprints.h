// arp_library_fingerprints.h — interaction fingerprints of a ligand-library result, scored on the device.
//
// The library result (arp_library.h) is resident: every (ligand, pose)'s receptor - ligand records in ascending (global pose, i,
// a), pose_off per global pose, the ligands' pose ranges.  A screen asks of them which molecules reproduce the interactions of a
// known binder.  A feature is (node, plane) as in arp_poses_fingerprints.h: the receptor atom i of a participating record (or
// its residue) and one of the 15 SIFt bits.  The references are NOT poses of the launch: the caller gives up to 64 of them as
// feature lists (ref_off, ref_node, ref_planes), and they are the first Q rows of the matrix — which is what k_pfp_cross reads
// as its references and what k_pfp_occupancy leaves out, so both run unchanged, as do k_pfp_scan and k_pfp_ids.
//
// Shape:
//   k_lfp_mark   a thread per library record and a thread per reference feature: the node sets its bit of the presence bitmap
//                (pfp_set_bit).  A record's node is ci[r] itself: the ligand side `a` is a small integer that is also a valid
//                receptor id, so nothing here asks pos_of which side of a record is the receptor's (pfp_node does).  A
//                reference's node is a column whether a pose touches it or not: its count is complete.
//   k_lfp_bits   a wave per row: a row below Q walks its reference's features, row Q + t the records of global pose t; the
//                column is base[word] + popcount(presence & bits below), one OR per selected plane (pfp_column and pfp_or_planes of
//                arp_poses_fingerprints.h).
//   k_lfp_best   the sibling of k_library_best: a wave per ligand over its pose range, per reference the global pose of the
//                highest Tanimoto in 32 fractional bits, ties to the lower pose.  No atomics.
// No float exists here; every result is a presence, a count or an integer quotient.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "arp_poses_fingerprints.h"

#define LIBFP_MAX_FEATURES (1 << 22)      // ARP_LIBFP_MAX_FEATURES: reference features a launch

// the references as the caller gave them, uploaded: reference q holds the features ref_off[q] ... ref_off[q + 1] - 1
struct LibFpRefs {
    const long long* ref_off;       // [Q + 1]
    const int* ref_node;            // [F] nodes of the launch's level, strictly ascending within a reference
    const uint32_t* ref_planes;     // [F] plane masks before selection
    long long F;
};

// the node of library record r: the receptor atom, or its residue; -1 when it is no node (never for a record of the launch)
__device__ __forceinline__ long long lfp_record_node(const PoseFpArgs& A, long long r) {
    const int i = A.ci[r];
    const long long node = A.by_res ? (long long)A.res_id[i] : (long long)i;
    return (node >= 0 && node < A.N) ? node : -1;
}
// the node and the selected planes of reference feature f; 0 when the selection empties its mask or it names no node (never:
// the host refused such a node)
__device__ __forceinline__ uint32_t lfp_feature_planes(const PoseFpArgs& A, const LibFpRefs& R, long long f, long long* node) {
    const long long v = (long long)R.ref_node[f];
    *node = v;
    return (v >= 0 && v < A.N) ? (R.ref_planes[f] & A.planes) : 0u;
}

// threads [0, k): the records; threads [k, k + F): the reference features
__global__ __launch_bounds__(256) void k_lfp_mark(PoseFpArgs A, LibFpRefs R) {
    const long long work = A.k + R.F;
    for (long long x = (long long)blockIdx.x * blockDim.x + threadIdx.x; x < work; x += (long long)gridDim.x * blockDim.x) {
        long long node = -1;
        if (x < A.k) {
            if (!pfp_record_planes(A, x)) continue;
            node = lfp_record_node(A, x);
        } else if (!lfp_feature_planes(A, R, x - A.k, &node)) {
            continue;
        }
        if (node < 0) continue;
        pfp_set_bit(A.presence + (node >> 6), 1ull << (node & 63));
    }
}

// A.P = Q + T rows; A.pose_off is the library result's, [T + 1]
__global__ __launch_bounds__(256) void k_lfp_bits(PoseFpArgs A, LibFpRefs R) {
    const int lane = threadIdx.x & 63;
    const long long waves = (long long)gridDim.x * (blockDim.x >> 6);
    for (long long p = (long long)blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6); p < A.P; p += waves) {
        unsigned long long* const row = A.bits + p * A.W;
        if (p < (long long)A.Q) {
            const long long s = max(R.ref_off[p], 0ll), e = min(R.ref_off[p + 1], R.F);
            for (long long f = s + lane; f < e; f += 64) {
                long long node = -1;
                const uint32_t m = lfp_feature_planes(A, R, f, &node);
                if (!m) continue;
                const long long col = pfp_column(A, node);
                if (col >= A.U) continue;      // (never: k_lfp_mark set this node's bit)
                pfp_or_planes(A, row, col, m);
            }
        } else {
            const long long t = p - A.Q;
            const long long s = (long long)A.pose_off[t], e = min((long long)A.pose_off[t + 1], A.k);
            for (long long r = s + lane; r < e; r += 64) {
                const uint32_t m = pfp_record_planes(A, r);
                if (!m) continue;
                const long long node = lfp_record_node(A, r);
                if (node < 0) continue;
                const long long col = pfp_column(A, node);
                if (col >= A.U) continue;      // (never: k_lfp_mark set this node's bit)
                pfp_or_planes(A, row, col, m);
            }
        }
    }
}

// ---- the ring / amide classes as planes: the four tables of the library-planes result (arp_library_planes.h), which
// is resident beside the library result and sorted by global pose as well.  Planes 15 ... 28 are those of
// arp_poses_fingerprints.h (POSEFP_PLANE_*).  Ids are the complex's: an entity is on the LIGAND side when it is an atom with id
// >= n, a ring with id >= nring or an amide with id >= namide; everything else is the receptor's, an affected receptor ring
// included.  A record takes part when bit ctype of ctype_mask is set, exactly one of its two entities is the ligand's and its
// plane is selected.  Its node is the residue of the receptor entity: res_id[atom], am_res[amide], and for a ring the RESIDENT
// ring_res[ring] of the receptor alone — no receptor ring path is resident here, and the reason the pose route avoids ring_res
// does not apply: the ligand is no part of the resident structure, so no ligand atom can have taken a ring's residue over.  The
// posed residue that k_library_planes makes per pose is not read.  The ligand side never names a node.
//   k_lfp_mark_planes  grid (x, 4), a row per table: the sibling of k_lfp_mark, into the same presence bitmap, before k_pfp_scan
//   k_lfp_bits_planes  a wave per row >= Q walks the pose's slice of each table (its pose_off): the sibling of k_lfp_bits, into
//                      the same rows, after it.  The reference rows are k_lfp_bits's: lfp_feature_planes ANDs with the unified mask
struct LibFpTables {
    const int* first[4];                     // atom, bgn, bgn, amide
    const int* second[4];                    // ring, end, end, ring
    const uint8_t* ctype[4];
    const uint8_t* ap_mask;                  // atom_plane: ARP_AP_* bits
    const unsigned long long* pose_off;      // [4][T + 1]
    long long count[4];
    const int* ring_res;                     // [nring] the receptor's, resident
    const int* am_res;                       // [namide]
    int n, nring, namide;                    // the receptor's atoms, rings, amides
    long long T;                             // global poses
};

// the selected planes of record r of table t and its node (-1: none); 0 when the record takes no part.  The table is a template
// parameter for the reason pfp_class_planes gives: a run-time index would send the pointer arrays to scratch memory
template <int t>
__device__ __forceinline__ uint32_t lfp_class_planes(const PoseFpArgs& A, const LibFpTables& T, long long r, long long* node) {
    const uint32_t ct = T.ctype[t][r];
    if (ct >= POSEFP_CTYPES || !((A.ctype_mask >> ct) & 1u)) return 0u;
    const int a = T.first[t][r], b = T.second[t][r];
    if (a < 0 || b < 0) return 0u;      // (never: the ids are those k_library_planes wrote)
    const int na = t == 0 ? T.n : t == 1 ? T.nring : T.namide, nb = (t == 0 || t == 1 || t == 3) ? T.nring : T.namide;
    const bool la = a >= na, lb = b >= nb;
    uint32_t m;
    if (t == 0) m = ((uint32_t)T.ap_mask[r] & ((1u << POSEFP_AP_BITS) - 1u)) << (la ? POSEFP_PLANE_AP_ATOM : POSEFP_PLANE_AP_RING);
    else if (t == 1) m = 1u << POSEFP_PLANE_PP;
    else if (t == 2) m = 1u << POSEFP_PLANE_GG;
    else m = 1u << (la ? POSEFP_PLANE_GP_AMIDE : POSEFP_PLANE_GP_RING);
    m &= A.planes;
    if (la == lb || !m) return 0u;
    // (the receptor entity's id is below its count: the one index that is read)
    int res;
    if (t == 0) res = la ? T.ring_res[b] : A.res_id[a];
    else if (t == 1) res = T.ring_res[la ? b : a];
    else if (t == 2) res = T.am_res[la ? b : a];
    else res = la ? T.ring_res[b] : T.am_res[a];
    *node = (res >= 0 && (long long)res < A.N) ? (long long)res : -1;
    return m;
}

template <int t>
__device__ __forceinline__ void lfp_mark_table(const PoseFpArgs& A, const LibFpTables& T) {
    for (long long r = (long long)blockIdx.x * blockDim.x + threadIdx.x; r < T.count[t]; r += (long long)gridDim.x * blockDim.x) {
        long long node = -1;
        if (!lfp_class_planes<t>(A, T, r, &node) || node < 0) continue;
        pfp_set_bit(A.presence + (node >> 6), 1ull << (node & 63));
    }
}
// grid (x, 4): row y marks table y
__global__ __launch_bounds__(256) void k_lfp_mark_planes(PoseFpArgs A, LibFpTables T) {
    switch (blockIdx.y) {
        case 0: lfp_mark_table<0>(A, T); break;
        case 1: lfp_mark_table<1>(A, T); break;
        case 2: lfp_mark_table<2>(A, T); break;
        default: lfp_mark_table<3>(A, T); break;
    }
}

// the slice of table t that belongs to global pose p, 64 records a step, into the pose's row
template <int t>
__device__ __forceinline__ void lfp_bits_table(const PoseFpArgs& A, const LibFpTables& T, long long p, int lane, unsigned long long* row) {
    if (T.count[t] == 0) return;
    const unsigned long long* const off = T.pose_off + (long long)t * (T.T + 1) + p;
    const long long s = (long long)off[0], e = min((long long)off[1], T.count[t]);
    for (long long r = s + lane; r < e; r += 64) {
        long long node = -1;
        const uint32_t m = lfp_class_planes<t>(A, T, r, &node);
        if (!m || node < 0) continue;
        const long long col = pfp_column(A, node);
        if (col >= A.U) continue;      // (never: k_lfp_mark_planes set this node's bit)
        pfp_or_planes(A, row, col, m);
    }
}
// A.P = Q + T rows; the rows below Q are the references': k_lfp_bits wrote them
__global__ __launch_bounds__(256) void k_lfp_bits_planes(PoseFpArgs A, LibFpTables T) {
    const int lane = threadIdx.x & 63;
    const long long waves = (long long)gridDim.x * (blockDim.x >> 6);
    for (long long p = (long long)blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6); p < T.T; p += waves) {
        unsigned long long* const row = A.bits + ((long long)A.Q + p) * A.W;
        lfp_bits_table<0>(A, T, p, lane, row);
        lfp_bits_table<1>(A, T, p, lane, row);
        lfp_bits_table<2>(A, T, p, lane, row);
        lfp_bits_table<3>(A, T, p, lane, row);
    }
}

struct LibFpBest {
    int L, Q, Qp;                            // ligands; references; the power of two >= Q (<= 64)
    const long long* pose_off;               // [L + 1] the global poses of ligand l (LibraryResult::tab)
    const uint32_t* count;                   // [Q + T]
    const uint32_t* cross;                   // [Q + T][Q]
    long long* n_poses;                      // [L]
    int* best_pose;                          // [L][Q]
    long long* q32;                          // [L][Q]
    uint32_t* shared;                        // [L][Q]
    uint32_t* best_count;                    // [L][Q]
};

// A wave per ligand.  Ligands have few poses and a row of cross is Q wide: lane x takes reference x mod Qp and the poses
// x / Qp + k (64 / Qp) of the ligand, so that the lanes of a step read consecutive words of cross; a butterfly over the xor
// distances >= Qp then joins the lanes of one reference.  floor(cross 2^32 / union) is one 64-bit integer division per (pose,
// reference); 2^32 where the union is empty (pose_shortlist.tanimoto_q32).  A lane walks its poses in ascending order and a
// join prefers the lower pose at equal scores: ties go to the lower global pose.
__global__ __launch_bounds__(256) void k_lfp_best(LibFpBest B) {
    const int lane = threadIdx.x & 63;
    const int wave = (int)((blockIdx.x * blockDim.x + threadIdx.x) >> 6), nwave = (int)((gridDim.x * blockDim.x) >> 6);
    const int q = lane & (B.Qp - 1), first = lane / B.Qp, step = 64 / B.Qp;
    const unsigned long long nq = q < B.Q ? (unsigned long long)B.count[q] : 0ull;
    for (int l = wave; l < B.L; l += nwave) {
        const long long p0 = B.pose_off[l], p1 = B.pose_off[l + 1];
        unsigned long long bs = 0;
        uint32_t bc = 0, bn = 0;
        int bi = -1;
        if (q < B.Q) {
            for (long long t = p0 + first; t < p1; t += step) {
                const long long row = (long long)B.Q + t;
                const uint32_t n = B.count[row], x = B.cross[row * B.Q + q];
                const unsigned long long u = (unsigned long long)n + nq - (unsigned long long)x;
                const unsigned long long s = u == 0 ? (1ull << 32) : ((unsigned long long)x << 32) / u;
                if (bi < 0 || s > bs) { bs = s; bi = (int)t; bc = x; bn = n; }
            }
        }
        for (int o = 32; o >= B.Qp; o >>= 1) {
            const unsigned long long os = __shfl_xor(bs, o);
            const int oi = __shfl_xor(bi, o);
            const uint32_t oc = (uint32_t)__shfl_xor((int)bc, o), on = (uint32_t)__shfl_xor((int)bn, o);
            if (oi >= 0 && (bi < 0 || os > bs || (os == bs && oi < bi))) { bs = os; bi = oi; bc = oc; bn = on; }
        }
        if (lane == 0) B.n_poses[l] = p1 - p0;
        if (first == 0 && q < B.Q) {
            const long long at = (long long)l * B.Q + q;
            B.best_pose[at] = bi;
            B.q32[at] = bi < 0 ? -1ll : (long long)bs;
            B.shared[at] = bc;
            B.best_count[at] = bn;
        }
    }
}
