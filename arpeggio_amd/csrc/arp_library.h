// arp_library.h — a ligand library on a resident receptor: different ligands, each with its poses, in one launch.
//
// arp_poses.h moves ONE ligand that is part of the resident structure.  A screen is the other case: thousands of different
// molecules against one receptor.  Here the receptor is resident alone (its static columns in the cell order of ensure_static,
// which no ligand changes) and the ligands' per-atom facts are a small table BESIDE it: type mask and flags (the meta word),
// {vdw, cov}, the hydrogen rows, and the index within the ligand of the single-bond heavy neighbour.  One launch walks
// (ligand, pose) items: for global pose t of ligand l exactly the records with one receptor and one ligand atom that a pass
// over the complex (the receptor with ligand l appended as one more residue, the pose scattered in, the ligand selected) emits.
//
//   k_library_contacts  a block per pose (grid stride over T), a wave per ligand heavy atom at a time; the cell walk, the
//                       resident partner, the per-wave LDS queue and the summary are the inline pieces of arp_poses.h that
//                       k_poses_contacts is made of.  Its own: at the start of a pose the block stages the ligand's table rows
//                       and the pose's coordinates in LDS, so the radii, the single-bond neighbour's coordinate and the
//                       hydrogen range of the ligand side are LDS reads
//   k_library_best      per ligand the best pose by a weighted sum of its summary row: a wave per ligand, no atomics
//   (k_poses_offsets of arp_poses.h makes pose_off and k_pose_columns the five columns, as they are)
//
// Why the filters of k_search vanish (arp_poses.h, the filter block of k_poses_contacts): a ligand is one residue of a chain of
// its own, no polypeptide residue, without sequence neighbours and without a bond to the receptor.  So I:729 (same residue)
// never holds; the sequence-adjacent gate needs M_RES_HASSEQ on both atoms and the ligand's has none; the covalent test
// (I:748-757) never finds a ligand atom in a receptor atom's bond list; a receptor atom's single-bond neighbour is never a
// ligand atom, and a ligand atom's always is one, so its coordinate is always the pose's.  In the complex the ligand's atoms
// follow the receptor's (j = n + a > i): bgn is always the receptor atom.
//
// The decision itself is pose_pair_sift of arp_poses.h, read through LibraryReader: no second statement of I:715-936.
//
// The key is t << (b + c) | i << c | a with b = the bits of the largest receptor id (<= 21) and c = the bits of the largest
// ligand (<= 8): ascending (t, i, a), at most 20 + 21 + 8 bits.
//
// The ligand of pose t comes from a per-pose int32 id made on the host (4 bytes beside the pose's >= 12 bytes per atom): one
// load per pose, where a binary search of pose_off would be up to 17 dependent loads in front of every pose's staging.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "arp_poses.h"

#define LIB_MAX_LIGANDS (1 << 16)
#define LIB_MAX_ATOMS 256
#define LIB_THREADS POSES_THREADS
#define LIB_WAVES POSES_WAVES
#define LIB_QCAP POSES_QCAP

struct LibraryArgs {
    int n, T;
    // the library, resident (CSR over the ligands; library atom = atom_off[l] + a)
    const int* atom_off;        // [L + 1]
    const uint16_t* tmask;      // [TA]
    const uint16_t* flags;      // [TA]
    const double2* lrad;        // [TA] {vdw, cov}
    const int* lh_off;          // [TA + 1] hydrogen rows, CSR over all library atoms
    const int* lsb_nbr;         // [TA] within the ligand, -1: none
    // the launch
    const int* lig_of;          // [T] ligand of global pose t
    const long long* first_pose;    // [L] the ligand's first global pose
    const long long* xyz_at;        // [L] where its first pose begins in pxyz (floats)
    const long long* hx_at;         // [L] ... and in phx (doubles)
    const float* pxyz;
    const double* phx;
    // the receptor, resident by local id
    const double2* rad;
    const float4* sb;
    const int* h_off;
    const double* h_xyz;
    // ... and in cell order
    const float4* sp_xyzm;
    const int4* sp_aux;
    const int4* sp_qa;
    const int* sp_h;
    const int* start;
    GridDesc g;
    double r2, comp;
    int ibits, abits;
    PoseSink out;
};

// How k_library_contacts reads what pose_pair_sift needs beside the two atoms.  bgn is the receptor atom (resident arrays by local
// id), end the ligand atom (lid = its index within the ligand: the staged rows in LDS).  Never covalent.
struct LibraryReader {
    const LibraryArgs& A;
    const double2* s_rad;
    const float* s_x;
    const int* s_nbr;
    __device__ __forceinline__ double comp() const { return A.comp; }
    __device__ __forceinline__ int* err() const { return A.out.err; }
    __device__ __forceinline__ double2 rad(const PoseAtom& a, bool of_b) const { return of_b ? A.rad[a.lid] : s_rad[a.lid]; }
    __device__ __forceinline__ float4 sb(int, const PoseAtom& B, const PoseAtom& E, bool of_b) const {
        if (of_b) return A.sb[B.lid];
        const int k = s_nbr[E.lid];
        return k >= 0 ? make_float4(s_x[3 * k], s_x[3 * k + 1], s_x[3 * k + 2], 1.0f) : make_float4(0.f, 0.f, 0.f, 0.f);
    }
    __device__ __forceinline__ bool bonded(const PoseAtom&, int) const { return false; }
};

__global__ __launch_bounds__(LIB_THREADS) void k_library_contacts(LibraryArgs A) {
    __shared__ u64 q_key[LIB_WAVES][LIB_QCAP], q_val[LIB_WAVES][LIB_QCAP];
    __shared__ double2 s_rad[LIB_MAX_ATOMS];
    __shared__ float s_x[3 * LIB_MAX_ATOMS];
    __shared__ uint32_t s_m[LIB_MAX_ATOMS];
    __shared__ int s_nbr[LIB_MAX_ATOMS];
    __shared__ int s_h[LIB_MAX_ATOMS + 1];
    __shared__ uint32_t s_sum[POSES_SUMMARY];
    __shared__ int s_qn[LIB_WAVES];
    __shared__ u64 s_base;
    const int lane = threadIdx.x & 63, w = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    const GridDesc g = A.g;
    int qn = 0;
    for (int pose = blockIdx.x; pose < A.T; pose += gridDim.x) {
        // ---- stage the ligand's table rows and the pose's coordinates (the host has checked every offset and index; S is clamped
        // all the same: the staging arrays hold LIB_MAX_ATOMS rows)
        const int l = A.lig_of[pose];
        const int a0 = A.atom_off[l], S = min(A.atom_off[l + 1] - a0, LIB_MAX_ATOMS);
        const int hb = A.lh_off[a0], SH = A.lh_off[a0 + S] - hb;
        const long long local = (long long)pose - A.first_pose[l];
        const float* const px = A.pxyz + A.xyz_at[l] + local * (long long)S * 3;
        const double* const phx = A.phx + A.hx_at[l] + local * (long long)SH * 3;
        if (threadIdx.x < POSES_SUMMARY) s_sum[threadIdx.x] = 0u;
        for (int k = threadIdx.x; k < S; k += LIB_THREADS) {
            const int nbr = A.lsb_nbr[a0 + k];
            const int h0 = A.lh_off[a0 + k] - hb, h1 = A.lh_off[a0 + k + 1] - hb;
            // the meta word as k_prepare_static composes it, for a residue that is no polypeptide residue and has no sequence
            // neighbours; M_SEL: the ligand is the selection of the complex
            uint32_t m = (uint32_t)(A.tmask[a0 + k] & M_TMASK) | ((uint32_t)(A.flags[a0 + k] & 0x7F) << M_FLAG_SHIFT) | M_HOME | M_SEL;
            const bool has_nbr = nbr >= 0 && nbr < S;
            if (has_nbr) m |= M_HAS_SB;
            if (h1 > h0) m |= M_HAS_H | (min((uint32_t)(h1 - h0 - 1), M_HCNT_ESC) << M_HCNT_SHIFT);
            s_m[k] = m;
            s_rad[k] = A.lrad[a0 + k];
            s_nbr[k] = has_nbr ? nbr : -1;
            s_h[k] = h0;
            if (k == S - 1) s_h[S] = h1;
        }
        bool bad = false;      // non-finite pose coordinates: the atoms' and the hydrogen rows'
        for (int k = threadIdx.x; k < 3 * S; k += LIB_THREADS) {
            const float v = px[k];
            s_x[k] = v;
            bad |= !isfinite(v);
        }
        for (int k = threadIdx.x; k < 3 * SH; k += LIB_THREADS) bad |= !isfinite(phx[k]);
        if (__syncthreads_or(bad ? 1 : 0)) {
            if (threadIdx.x == 0) atomicExch(A.out.err, ARP_E_ARG);
            if (threadIdx.x < POSES_SUMMARY) A.out.summary[(size_t)pose * POSES_SUMMARY + threadIdx.x] = 0u;
            __syncthreads();      // (the next pose stages over these rows)
            continue;
        }
        PoseCounts cnt;
        cnt.clear();
        const LibraryReader reader{A, s_rad, s_x, s_nbr};
        for (int s = w; s < S; s += LIB_WAVES) {
            const uint32_t mh = s_m[s];
            if (mh & M_HYDROGEN) continue;                               // I:712
            const float pxs = s_x[3 * s], pys = s_x[3 * s + 1], pzs = s_x[3 * s + 2];
            const int ph0 = s_h[s], ph1 = s_h[s + 1];
            const PoseRow row = pose_cell_rows(g, A.start, A.n, pxs, pys, pzs, lane);
            if (!row.inside) continue;
            const int total = __shfl(row.incl, 8);
            int rb_[9], re_[9];      // start of row r minus the candidates before it; candidates up to and including row r
#pragma unroll
            for (int r = 0; r < 9; ++r) {
                const int i_ = __shfl(row.incl, r), l_ = __shfl(row.len, r), b_ = __shfl(row.beg, r);
                re_[r] = i_;
                rb_[r] = b_ - (i_ - l_);
            }
            const num::d3 pd = {(double)pxs, (double)pys, (double)pzs};
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
                    // every resident atom is the receptor's: no `sel` test, and none of k_search's residue filters can hold (above)
                    pass = !(mj & M_HYDROGEN) && (unsigned)aj.x < (unsigned)A.n;
                    pass = pass && num::dist2_kd(pd, num::d3{(double)v.x, (double)v.y, (double)v.z}) <= A.r2;
                }
                uint32_t sft = 0;
                u64 key = 0, val = 0;
                if (pass) {
                    PoseAtom H;
                    H.x = {pxs, pys, pzs}; H.m = mh; H.lid = s; H.qa = make_int4(s, -1, -1, -1); H.hx = phx; H.h0 = ph0; H.h1 = ph1;
                    const PoseAtom J = pose_resident_atom(pos, v, aj, A.sp_qa, A.sp_h, A.h_off, A.h_xyz);
                    const float d = num::norm(num::sub(J.x, H.x));                      // interactions.py:745, bgn = the receptor atom
                    int ct = 0;
                    sft = pose_pair_sift(reader, pose, J, H, d, &ct);
                    key = ((u64)(unsigned)pose << (A.ibits + A.abits)) | ((u64)(unsigned)J.lid << A.abits) | (u64)(unsigned)s;
                    val = (u64)__float_as_uint(d) | ((u64)sft << 32) | ((u64)(unsigned)ct << 48);
                }
                const unsigned long long mp = __ballot(pass);
                if (mp) pose_queue_push(A.out, q_key[w], q_val[w], qn, cnt, lane, mp, pass, key, val, sft);
            }
        }
        cnt.store(s_sum, lane, A.out.summary + (size_t)pose * POSES_SUMMARY);      // (the next pose stages over the rows, too)
    }
    pose_queue_drain(A.out, q_key[w], q_val[w], qn, lane, w, s_qn, &s_base);
}

// Best pose per ligand: score[t] = sum over the slots of w[s] summary[t][s] in int64 (|w| <= 2^24, a slot < 2^32: the sum fits
// 60 bits); the highest score wins, ties go to the lower global pose id.  A segmented arg-max: a wave per ligand over its
// pose_off range, each lane its poses in ascending order, then a butterfly over the wave.  No atomics.  A ligand without poses:
// -1 and INT64_MIN.
struct LibraryWeights { int w[POSES_SUMMARY]; };
__global__ __launch_bounds__(256) void k_library_best(int L, const long long* __restrict__ pose_off, const uint32_t* __restrict__ summary,
                                                      LibraryWeights W, long long* __restrict__ n_poses, int* __restrict__ best,
                                                      long long* __restrict__ score) {
    const int lane = threadIdx.x & 63;
    const int wave = (int)((blockIdx.x * blockDim.x + threadIdx.x) >> 6), nwave = (int)((gridDim.x * blockDim.x) >> 6);
    const long long none = (long long)0x8000000000000000ull;
    for (int l = wave; l < L; l += nwave) {
        const long long p0 = pose_off[l], p1 = pose_off[l + 1];
        long long bs = none;
        int bi = -1;
        for (long long t = p0 + lane; t < p1; t += 64) {
            const uint4* const row = (const uint4*)(summary + (size_t)t * POSES_SUMMARY);
            long long sc = 0;
#pragma unroll
            for (int q = 0; q < POSES_SUMMARY / 4; ++q) {
                const uint4 u = row[q];
                sc += (long long)W.w[4 * q] * (long long)u.x + (long long)W.w[4 * q + 1] * (long long)u.y +
                      (long long)W.w[4 * q + 2] * (long long)u.z + (long long)W.w[4 * q + 3] * (long long)u.w;
            }
            if (bi < 0 || sc > bs) { bs = sc; bi = (int)t; }
        }
        for (int o = 32; o > 0; o >>= 1) {
            const long long os = __shfl_xor(bs, o);
            const int oi = __shfl_xor(bi, o);
            if (oi >= 0 && (bi < 0 || os > bs || (os == bs && oi < bi))) { bs = os; bi = oi; }
        }
        if (lane == 0) {
            n_poses[l] = p1 - p0;
            best[l] = bi;
            score[l] = bs;
        }
    }
}
