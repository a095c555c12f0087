// arp_library_planes.h — a ligand library on a resident receptor: the ring and amide contacts of every pose of every ligand in
// one launch.  The companion of arp_library.h, which gives the atom-atom records of the same poses, and the
// library's counterpart of arp_poses_planes.h.
//
// The receptor is resident alone: its ring centres, normals and ring residues, its amide centres, normals and residues, the two
// centre grids.  No receptor ring or amide ever moves and no receptor atom is selected, so none of their atoms is needed.  The
// ligands' rings and amides are a table BESIDE the library (arp_set_ligand_library_planes): ring paths and amide atoms by index
// WITHIN the ligand.  For global pose t of ligand l the kernel emits exactly those records of the four ring / amide bags of the
// COMPLEX — the receptor with ligand l appended as one more residue, the pose scattered in, the ligand's rings and amides
// appended after the receptor's, geometry and ring residues made again as initialize() makes them, the ligand selected,
// _make_selection with the 6.0 A expansion — that involve an AFFECTED entity:
//   every ligand atom, every ligand ring, every ligand amide;
//   every receptor ring with a ligand atom within 3.0 A (dist2_kd <= 9.0) of its centre at the pose coordinate.
// Ids are the complex's: atom n + a, ring nring + q, amide namide + g, the ligand's residue is the receptor's residue count.
//
//   k_lpl_hist         once per structure: atoms per residue (the scan and the scatter of arp_grid.h make the residue -> atoms
//                      CSR from it; k_ppl_mark of arp_poses_planes.h would read a selection, and none is read here)
//   k_library_planes   a block per pose (grid stride over T): the ligand's meta words, amide atoms and the pose's coordinates in LDS (the
//                      staging pass is the non-finite check); geometry of the ligand's rings and amides into the block's lists;
//                      the receptor rings the pose comes near (an LDS hash set); residue and selection flags of every affected
//                      ring (a wave per ring, over ALL receptor atoms and the pose's); then a wave per home item — affected ring,
//                      ligand atom, ligand amide — with the phase-1 supersets, the per-wave LDS queue and the phase-2 evaluation
//                      of k_poses_planes: ppl_eval, read through LplReader.  No second statement of the four decisions
//   (k_poses_offsets of arp_poses.h and k_ppl_columns of arp_poses_planes.h make pose_off and the columns, as they are)
//
// What is simpler than in k_poses_planes: no receptor atom is selected (a receptor residue is in selection_plus only through an
// atom within 6.0 A of the pose), no receptor amide is moved, and there is no static list — a library ligand has no resident
// coordinate, so what a pose affects is known from the pose alone.
//
// The ligand's amide atoms are staged in LDS with the meta words (at most 32 rows of 16 B).  The ring PATHS are not: a path has no
// bound shorter than S atoms, 32 of them none below 32 S, and each is read by the one lane that makes that ring's geometry, once
// per pose; they are read from the table in global memory.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "arp_library.h"
#include "arp_poses_planes.h"

#define LPL_THREADS PPL_THREADS
#define LPL_WAVES PPL_WAVES
#define LPL_MAX_RINGS 32         // rings of one ligand
#define LPL_MAX_AMIDES 32        // amides of one ligand
#define LPL_WS_RINGS (LPL_MAX_RINGS + PPL_MAX_NEAR)      // a block's ring list: the ligand's, then the receptor's near the pose

struct LplArgs {
    int n, T, nring, namide, nres;      // the receptor's atoms, rings, amides and residues; T poses
    // the library (arp_library.h) and its plane table (CSR over the ligands, indices within the ligand)
    const int* atom_off;
    const uint16_t* tmask;
    const uint16_t* flags;
    const int* lh_off;
    const int* lsb_nbr;
    const int* lring_off;        // [L + 1]
    const int* lring_atom_off;   // [TR + 1]
    const int* lring_atom_idx;
    const int* lamide_off;       // [L + 1]
    const int* lamide_atoms;     // [TM][4]
    // the launch
    const int* lig_of;           // [T]
    const long long* first_pose; // [L]
    const long long* xyz_at;     // [L]
    const float* pxyz;
    // the receptor, by local id
    const int* res_off;          // residue -> atoms
    const int* res_atoms;
    const float4* xyz;
    const float4* st_xyzm;
    const int* res_id;
    const double* ring_c;
    const double* ring_n;
    const int* ring_res;
    const float* am_c;
    const float* am_n;
    const int* am_res;
    GridDesc ga; const int* a_start; const int* a_perm;      // every atom, 6 A
    GridDesc gr; const int* r_start; const int* r_perm;      // ring centres
    GridDesc gm; const int* m_start; const int* m_perm;      // amide centres
    PplRing* ws_ring;            // [blocks][LPL_WS_RINGS]
    PplAmide* ws_amide;          // [blocks][LPL_MAX_AMIDES]
    // the record sink (the names ppl_eval reads)
    PlaneRec* rec;
    u64* key;
    u64* val;
    u64 cap;
    u64* ctr;                    // [0] records appended (exact, also beyond cap), [1] error word, [2 .. 5] records per table
    uint32_t* summary;           // [T][16]
    int idbits, pbits;
};

__global__ __launch_bounds__(256) void k_lpl_hist(int n, const int* __restrict__ res_id, int* __restrict__ hist) {
    for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < n; i += gridDim.x * blockDim.x) atomicAdd(&hist[res_id[i]], 1);
}

struct LplShared {
    float px[LIB_MAX_ATOMS * 3];
    uint32_t m[LIB_MAX_ATOMS];
    int4 am[LPL_MAX_AMIDES];     // the ligand's amide atoms: N, C, O, fourth
    int4 q[LPL_WAVES][PPL_QCAP];
    int hash[PPL_NEAR_HASH];
    uint32_t sum[PPL_SUMMARY];
    int n_near, over;
};

// a receptor atom at x: within 6.0 A (inclusive, float64) of a ligand atom's pose coordinate
__device__ __forceinline__ bool lpl_atom_plus(const float* px, int S, num::d3 x) {
    for (int s = 0; s < S; ++s)
        if (num::dist2_kd(x, num::d3{(double)px[3 * s], (double)px[3 * s + 1], (double)px[3 * s + 2]}) <= 36.0) return true;
    return false;
}
// receptor residue res in the pose's selection_plus residues: one of its atoms is (one lane)
__device__ __forceinline__ bool lpl_res_plus(const LplArgs& A, const float* px, int S, int res) {
    if (res < 0) return false;
    for (int k = A.res_off[res], k1 = A.res_off[res + 1]; k < k1; ++k) {
        const float4 v = A.xyz[A.res_atoms[k]];
        if (lpl_atom_plus(px, S, num::d3{(double)v.x, (double)v.y, (double)v.z})) return true;
    }
    return false;
}
// ... by a whole wave (res is wave-uniform)
__device__ __forceinline__ bool lpl_res_plus_wave(const LplArgs& A, const float* px, int S, int res, int lane) {
    if (res < 0) return false;
    bool p = false;
    for (int k = A.res_off[res] + lane, k1 = A.res_off[res + 1]; k < k1; k += 64) {
        const float4 v = A.xyz[A.res_atoms[k]];
        p = p || lpl_atom_plus(px, S, num::d3{(double)v.x, (double)v.y, (double)v.z});
    }
    return __any(p) != 0;
}
__device__ __forceinline__ void lpl_near_insert(LplShared* sh, int r) {
    unsigned h = ppl_hash(r);
    for (int probe = 0; probe < PPL_NEAR_HASH; ++probe) {
        const int old = atomicCAS(&sh->hash[h], -1, r);
        if (old == -1 || old == r) return;
        h = (h + 1) & (PPL_NEAR_HASH - 1);
    }
    sh->over = 1;
}
__device__ __forceinline__ bool lpl_affected(const LplShared* sh, int r) {      // (a receptor ring)
    if (sh->n_near == 0) return false;
    unsigned h = ppl_hash(r);
    for (int probe = 0; probe < PPL_NEAR_HASH; ++probe) {
        const int v = sh->hash[h];
        if (v == r) return true;
        if (v == -1) return false;
        h = (h + 1) & (PPL_NEAR_HASH - 1);
    }
    return false;
}

// How k_library_planes reads the operands of ppl_eval.  A reference < 0 names entry -ref - 1 of the block's lists (a ligand atom:
// its index within the ligand, in LDS), one >= 0 a resident id of the receptor: never selected, in selection_plus through its
// atoms only.
struct LplReader {
    const LplArgs& A;
    const PplRing* wsr;
    const PplAmide* wsa;
    const float* px;
    const uint32_t* sm;
    int S;
    __device__ __forceinline__ PplRingV ring(int ref) const {
        PplRingV R;
        if (ref < 0) {
            const PplRing* w = wsr + (-ref - 1);
            R.id = w->id; R.res = w->res; R.sel = (w->flags & 1u) != 0; R.plus = (w->flags & 2u) != 0;
            R.c = {w->c[0], w->c[1], w->c[2]};
            R.n = {w->n[0], w->n[1], w->n[2]};
        } else {
            R.id = ref; R.res = A.ring_res[ref];
            R.sel = false;
            R.plus = lpl_res_plus(A, px, S, R.res);
            R.c = ld3(A.ring_c, ref);
            R.n = ld3(A.ring_n, ref);
        }
        return R;
    }
    __device__ __forceinline__ PplAmideV amide(int ref) const {
        PplAmideV G;
        if (ref < 0) {
            const PplAmide* w = wsa + (-ref - 1);
            G.id = w->id; G.sel = (w->flags & 1u) != 0; G.plus = (w->flags & 2u) != 0;
            G.c = {w->c[0], w->c[1], w->c[2]};
            G.n = {w->n[0], w->n[1], w->n[2]};
        } else {
            G.id = ref;
            G.sel = false;
            G.plus = lpl_res_plus(A, px, S, A.am_res[ref]);
            G.c = lf3(A.am_c, ref);
            G.n = lf3(A.am_n, ref);
        }
        return G;
    }
    __device__ __forceinline__ void atom(int ref, int* lid, num::d3* x, uint32_t* m, bool* plus) const {
        if (ref < 0) {
            const int s = -ref - 1;
            *lid = A.n + s;
            *x = {(double)px[3 * s], (double)px[3 * s + 1], (double)px[3 * s + 2]};
            *m = sm[s];
        } else {
            *lid = ref;
            const float4 v = A.st_xyzm[ref];
            *x = {(double)v.x, (double)v.y, (double)v.z};
            *m = __float_as_uint(v.w) & ~(uint32_t)M_SEL;
            *plus = lpl_atom_plus(px, S, *x);
        }
    }
};

__global__ __launch_bounds__(LPL_THREADS) void k_library_planes(LplArgs A) {
    __shared__ LplShared s_sh;
    LplShared* const sh = &s_sh;
    const int tid = (int)threadIdx.x, lane = tid & 63, w = __builtin_amdgcn_readfirstlane(tid >> 6);
    PplRing* const wsr = A.ws_ring + (size_t)blockIdx.x * LPL_WS_RINGS;
    PplAmide* const wsa = A.ws_amide + (size_t)blockIdx.x * LPL_MAX_AMIDES;
    const float* const px = sh->px;
    for (int pose = blockIdx.x; pose < A.T; pose += gridDim.x) {
        // ---- the ligand of the pose (one load), its meta words and the pose's coordinates.  The host has checked every offset,
        // count and index; the counts are clamped all the same: the block's arrays hold that many rows
        const int l = A.lig_of[pose];
        const int a0 = A.atom_off[l], S = min(A.atom_off[l + 1] - a0, LIB_MAX_ATOMS);
        const int q0 = A.lring_off[l], nLR = min(A.lring_off[l + 1] - q0, LPL_MAX_RINGS);
        const int g0 = A.lamide_off[l], nLM = min(A.lamide_off[l + 1] - g0, LPL_MAX_AMIDES);
        const float* const src = A.pxyz + A.xyz_at[l] + ((long long)pose - A.first_pose[l]) * (long long)S * 3;
        if (tid < PPL_SUMMARY) sh->sum[tid] = 0u;
        for (int k = tid; k < PPL_NEAR_HASH; k += LPL_THREADS) sh->hash[k] = -1;
        if (tid == 0) { sh->n_near = 0; sh->over = 0; }
        for (int k = tid; k < S; k += LPL_THREADS) {
            // the meta word as k_library_contacts composes it: a residue that is no polypeptide residue and has no sequence
            // neighbours (no residue flags); M_SEL: the ligand is the selection of the complex
            const int nbr = A.lsb_nbr[a0 + k];
            const int nh = A.lh_off[a0 + k + 1] - A.lh_off[a0 + k];
            uint32_t m = (uint32_t)(A.tmask[a0 + k] & M_TMASK) | ((uint32_t)(A.flags[a0 + k] & 0x7F) << M_FLAG_SHIFT) | M_HOME | M_SEL;
            if (nbr >= 0 && nbr < S) m |= M_HAS_SB;
            if (nh > 0) m |= M_HAS_H | (min((uint32_t)(nh - 1), M_HCNT_ESC) << M_HCNT_SHIFT);
            sh->m[k] = m;
        }
        for (int k = tid; k < nLM; k += LPL_THREADS) sh->am[k] = ((const int4*)A.lamide_atoms)[g0 + k];
        bool bad = false;
        for (int k = tid; k < 3 * S; k += LPL_THREADS) {
            const float v = src[k];
            sh->px[k] = v;
            bad |= !isfinite(v);
        }
        if (__syncthreads_or(bad ? 1 : 0)) {      // (block-uniform)
            if (tid == 0) atomicExch((int*)(A.ctr + 1), ARP_E_ARG);
            if (tid < PPL_SUMMARY) A.summary[(size_t)pose * PPL_SUMMARY + tid] = 0u;
            __syncthreads();
            continue;
        }
        // ---- geometry of the ligand's rings and amides (ids behind the receptor's).  A ligand amide lies in the selected residue:
        // sel and plus
        const auto at = [&](int a) { return num::f3{px[3 * a], px[3 * a + 1], px[3 * a + 2]}; };
        for (int i = tid; i < nLR; i += LPL_THREADS) {
            PplRing* o = wsr + i;
            const int p0 = A.lring_atom_off[q0 + i];
            ppl_ring_geometry_of(at, A.lring_atom_idx + p0, A.lring_atom_off[q0 + i + 1] - p0, o->c, o->n);
            o->id = A.nring + i; o->res = -1; o->flags = 0u; o->pad = 0;
        }
        for (int k = tid; k < nLM; k += LPL_THREADS) {
            PplAmide* o = wsa + k;
            ppl_amide_geometry_of(at, (const int*)&sh->am[k], o->c, o->n);
            o->id = A.namide + k; o->flags = 3u;
        }
        // ---- the receptor rings this pose comes near: a wave per ligand atom, the ring-centre grid around its pose coordinate
        if (A.nring > 0) {
            for (int s = w; s < S; s += LPL_WAVES) {
                const num::d3 x = {(double)px[3 * s], (double)px[3 * s + 1], (double)px[3 * s + 2]};
                const Stencil st = stencil_load(A.gr, A.r_start, cell_box(A.gr, x), lane);
                for (int kb = 0; kb < st.pre[9]; kb += 64) {
                    const int k = kb + lane;
                    if (k < st.pre[9]) {
                        const int r = A.r_perm[stencil_pos(st, k)];
                        if (num::dist2_kd(ld3(A.ring_c, r), x) <= 9.0) lpl_near_insert(sh, r);
                    }
                }
            }
        }
        __syncthreads();
        for (int h = tid; h < PPL_NEAR_HASH; h += LPL_THREADS) {
            const int r = sh->hash[h];
            if (r >= 0) {
                const int slot = atomicAdd(&sh->n_near, 1);
                if (slot < PPL_MAX_NEAR) {
                    PplRing* o = wsr + nLR + slot;
                    for (int q = 0; q < 3; ++q) { o->c[q] = A.ring_c[3 * (size_t)r + q]; o->n[q] = A.ring_n[3 * (size_t)r + q]; }
                    o->id = r; o->res = -1; o->flags = 0u; o->pad = 0;
                }
            }
        }
        __syncthreads();
        if (sh->over || sh->n_near > PPL_MAX_NEAR) {      // never drop a ring: the launch fails by name
            if (tid == 0) atomicExch((int*)(A.ctr + 1), PPL_E_NEAR);
            if (tid < PPL_SUMMARY) A.summary[(size_t)pose * PPL_SUMMARY + tid] = 0u;
            __syncthreads();
            continue;
        }
        const int nAff = nLR + sh->n_near;
        // ---- residue and selection flags of every affected ring: k_ring_residue's search over ALL receptor atoms (hydrogens
        // included) and over the pose's atoms (id n + a); a ring is sel when its residue is the ligand's
        uint32_t n_diff = 0, n_none = 0;
        for (int i = w; i < nAff; i += LPL_WAVES) {
            PplRing* o = wsr + i;
            const num::d3 ctr_ = {o->c[0], o->c[1], o->c[2]};
            double best = 1e300;
            int best_lid = 0x7FFFFFFF;
            {
                const Stencil st = stencil_load(A.ga, A.a_start, cell_box(A.ga, ctr_), lane);
                for (int kb = 0; kb < st.pre[9]; kb += 64) {
                    const int k = kb + lane;
                    if (k < st.pre[9]) {
                        const int lid = A.a_perm[stencil_pos(st, k)];
                        const float4 v = A.xyz[lid];
                        const num::d3 x = {(double)v.x, (double)v.y, (double)v.z};
                        if (num::dist2_kd(ctr_, x) <= 9.0) {
                            const double d = num::norm(num::sub(x, ctr_));
                            if (d < best || (d == best && lid < best_lid)) { best = d; best_lid = lid; }
                        }
                    }
                }
            }
            for (int s = lane; s < S; s += 64) {
                const num::d3 x = {(double)px[3 * s], (double)px[3 * s + 1], (double)px[3 * s + 2]};
                if (num::dist2_kd(ctr_, x) <= 9.0) {
                    const double d = num::norm(num::sub(x, ctr_));
                    const int lid = A.n + s;
                    if (d < best || (d == best && lid < best_lid)) { best = d; best_lid = lid; }
                }
            }
            for (int o_ = 32; o_ > 0; o_ >>= 1) {
                const double od = __shfl_xor(best, o_);
                const int ol = __shfl_xor(best_lid, o_);
                if (od < best || (od == best && ol < best_lid)) { best = od; best_lid = ol; }
            }
            const int res = best_lid == 0x7FFFFFFF ? -1 : best_lid >= A.n ? A.nres : A.res_id[best_lid];
            const bool sel = res == A.nres;
            const bool plus = sel || lpl_res_plus_wave(A, px, S, res, lane);
            if (lane == 0) {
                o->res = res;
                o->flags = (sel ? 1u : 0u) | (plus ? 2u : 0u);
                if (i >= nLR) n_diff += res != A.ring_res[o->id] ? 1u : 0u;
                n_none += res < 0 ? 1u : 0u;
            }
        }
        if (lane == 0) {
            if (n_diff) atomicAdd(&sh->sum[13], n_diff);
            if (n_none) atomicAdd(&sh->sum[14], n_none);
        }
        if (tid == 0) sh->sum[12] = (uint32_t)nAff;
        __syncthreads();
        // ---- the four loops: a wave per home item, candidates to the wave's queue, 64 at a time through phase 2
        int4* const q = sh->q[w];
        int qn = 0;
        const LplReader reader{A, wsr, wsa, px, sh->m, S};
        auto push = [&](bool ok, int kind, int x, int y) {
            const unsigned long long m = __ballot(ok);
            if (!m) return;
            if (ok) q[qn + __popcll(m & ((1ull << lane) - 1ull))] = make_int4(kind, x, y, 0);
            qn += __popcll(m);
            __builtin_amdgcn_wave_barrier();
            if (qn >= 64) {
                qn -= 64;
                const int4 e = q[qn + lane];
                __builtin_amdgcn_wave_barrier();
                ppl_eval(reader, sh->sum, pose, true, e, lane);
            }
        };
        const int items = nAff + S + nLM;
        for (int it = w; it < items; it += LPL_WAVES) {
            if (it < nAff) {
                // affected ring i: every atom (atom-plane), every ring (plane-plane), every receptor amide (group-plane)
                const int i = it;
                const PplRing* o = wsr + i;
                if (!(o->flags & 2u)) continue;                      // I:957, 1081, 1318: the ring is not in selection_plus
                const num::d3 ctr_ = {o->c[0], o->c[1], o->c[2]};
                {
                    const Stencil st = stencil_load(A.ga, A.a_start, cell_box(A.ga, ctr_), lane);
                    for (int kb = 0; kb < st.pre[9]; kb += 64) {
                        const int k = kb + lane;
                        bool ok = false;
                        int lid = 0;
                        if (k < st.pre[9]) {
                            lid = A.a_perm[stencil_pos(st, k)];
                            const float4 v = A.st_xyzm[lid];
                            const uint32_t m = __float_as_uint(v.w);
                            ok = num::dist2_kd(ctr_, num::d3{(double)v.x, (double)v.y, (double)v.z}) <= 36.0 && !(m & (M_HYDROGEN | ARP_T_AROMATIC));
                        }
                        push(ok, 0, -(i + 1), lid);
                    }
                }
                for (int sb_ = 0; sb_ < S; sb_ += 64) {
                    const int s = sb_ + lane;
                    bool ok = false;
                    if (s < S)
                        ok = num::dist2_kd(ctr_, num::d3{(double)px[3 * s], (double)px[3 * s + 1], (double)px[3 * s + 2]}) <= 36.0 &&
                             !(sh->m[s] & (M_HYDROGEN | ARP_T_AROMATIC));
                    push(ok, 0, -(i + 1), -(s + 1));
                }
                if (A.nring > 0) {
                    const Stencil st = stencil_load(A.gr, A.r_start, cell_box(A.gr, ctr_), lane);
                    for (int kb = 0; kb < st.pre[9]; kb += 64) {
                        const int k = kb + lane;
                        bool ok = false;
                        int b = 0;
                        if (k < st.pre[9]) {
                            b = A.r_perm[stencil_pos(st, k)];
                            ok = !lpl_affected(sh, b) && num::dist2_kd(ctr_, ld3(A.ring_c, b)) <= 36.0 * (1.0 + 1e-9);
                        }
                        push(ok, 1, -(i + 1), b);
                    }
                }
                for (int tb = i + 1; tb < nAff; tb += 64) {
                    const int t = tb + lane;
                    bool ok = false;
                    if (t < nAff) ok = num::dist2_kd(ctr_, num::d3{wsr[t].c[0], wsr[t].c[1], wsr[t].c[2]}) <= 36.0 * (1.0 + 1e-9);
                    push(ok, 1, -(i + 1), -(t + 1));
                }
                if (A.namide > 0) {
                    const Stencil st = stencil_load(A.gm, A.m_start, cell_box(A.gm, ctr_), lane);
                    for (int kb = 0; kb < st.pre[9]; kb += 64) {
                        const int k = kb + lane;
                        bool ok = false;
                        int a = 0;
                        if (k < st.pre[9]) {
                            a = A.m_perm[stencil_pos(st, k)];
                            ok = num::dist2_kd(num::to_d3(lf3(A.am_c, a)), ctr_) <= 36.0 * (1.0 + 1e-9);
                        }
                        push(ok, 3, a, -(i + 1));
                    }
                }
            } else if (it < nAff + S) {
                // ligand atom s: the unaffected receptor rings around its pose coordinate (atom-plane)
                const int s = it - nAff;
                if ((sh->m[s] & (M_HYDROGEN | ARP_T_AROMATIC)) || A.nring == 0) continue;
                const num::d3 x = {(double)px[3 * s], (double)px[3 * s + 1], (double)px[3 * s + 2]};
                const Stencil st = stencil_load(A.gr, A.r_start, cell_box(A.gr, x), lane);
                for (int kb = 0; kb < st.pre[9]; kb += 64) {
                    const int k = kb + lane;
                    bool ok = false;
                    int r = 0;
                    if (k < st.pre[9]) {
                        r = A.r_perm[stencil_pos(st, k)];
                        ok = !lpl_affected(sh, r) && num::dist2_kd(ld3(A.ring_c, r), x) <= 36.0;
                    }
                    push(ok, 0, r, -(s + 1));
                }
            } else {
                // ligand amide k: every receptor amide, both orders, and the ligand's other amides (group-group); every ring
                // (group-plane)
                const int kk = it - nAff - S;
                const PplAmide* o = wsa + kk;
                const num::d3 cad = {(double)o->c[0], (double)o->c[1], (double)o->c[2]};
                if (A.namide > 0) {
                    const Stencil st = stencil_load(A.gm, A.m_start, cell_box(A.gm, cad), lane);
                    for (int kb = 0; kb < st.pre[9]; kb += 64) {
                        const int k = kb + lane;
                        bool ok = false;
                        int b = 0;
                        if (k < st.pre[9]) {
                            b = A.m_perm[stencil_pos(st, k)];
                            ok = num::dist2_kd(cad, num::to_d3(lf3(A.am_c, b))) <= 36.0 * (1.0 + 1e-5);
                        }
                        push(ok, 2, -(kk + 1), b);
                        push(ok, 2, b, -(kk + 1));
                    }
                }
                for (int tb = 0; tb < nLM; tb += 64) {
                    const int t = tb + lane;
                    bool ok = false;
                    if (t < nLM && t != kk)
                        ok = num::dist2_kd(cad, num::d3{(double)wsa[t].c[0], (double)wsa[t].c[1], (double)wsa[t].c[2]}) <= 36.0 * (1.0 + 1e-5);
                    push(ok, 2, -(kk + 1), -(t + 1));
                }
                if (A.nring > 0) {
                    const Stencil st = stencil_load(A.gr, A.r_start, cell_box(A.gr, cad), lane);
                    for (int kb = 0; kb < st.pre[9]; kb += 64) {
                        const int k = kb + lane;
                        bool ok = false;
                        int r = 0;
                        if (k < st.pre[9]) {
                            r = A.r_perm[stencil_pos(st, k)];
                            ok = !lpl_affected(sh, r) && num::dist2_kd(cad, ld3(A.ring_c, r)) <= 36.0 * (1.0 + 1e-9);
                        }
                        push(ok, 3, -(kk + 1), r);
                    }
                }
                for (int tb = 0; tb < nAff; tb += 64) {
                    const int t = tb + lane;
                    bool ok = false;
                    if (t < nAff) ok = num::dist2_kd(cad, num::d3{wsr[t].c[0], wsr[t].c[1], wsr[t].c[2]}) <= 36.0 * (1.0 + 1e-9);
                    push(ok, 3, -(kk + 1), -(t + 1));
                }
            }
        }
        __builtin_amdgcn_wave_barrier();
        if (qn > 0) {       // (wave-uniform)
            const bool live = lane < qn;
            const int4 e = live ? q[lane] : make_int4(-1, 0, 0, 0);
            ppl_eval(reader, sh->sum, pose, live, e, lane);
            qn = 0;
        }
        __syncthreads();
        if (tid < PPL_SUMMARY) A.summary[(size_t)pose * PPL_SUMMARY + tid] = sh->sum[tid];
        if (tid < 4 && sh->sum[tid]) atomicAdd(A.ctr + 2 + tid, (unsigned long long)sh->sum[tid]);
        __syncthreads();
    }
}
