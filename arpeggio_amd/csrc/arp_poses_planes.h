// arp_poses_planes.h — ligand poses on a resident receptor: the ring and amide contacts of every pose in one launch
// (DESIGN.md 5p).  The companion of arp_poses.h, which gives the atom-atom records of the same poses.
//
// A single structure is resident with an uploaded selection, the MOVABLE SET of arp_poses.h, and with the atoms of its rings
// and amides (arp_set_plane_atoms).  A pose gives new coordinates for the movable atoms.  For pose p the kernel emits exactly
// those records of the four ring / amide bags of the POSED structure — the pose scattered in, ring and amide geometry and ring
// residues made again as initialize() makes them, _make_selection with the same selection and the 6.0 A expansion — that
// involve an AFFECTED entity:
//   every movable atom;
//   every MOVED AMIDE: N, C or O is movable;
//   every AFFECTED RING: a movable atom in its path, or a movable atom within 3.0 A (dist2_kd <= 9.0) of its centre at the
//   atom's pose coordinate or at its resident coordinate.  Any other ring keeps centre, normal and residue.
//
//   k_ppl_mark / k_ppl_lists   once per (structure, selection, plane atoms): position of every movable atom, selected residues,
//                     a residue -> atoms CSR (histogram here, the scan and the scatter of arp_grid.h), the rings with a
//                     movable atom, the further rings affected at home, the moved amides, and the tables ring -> kind,
//                     amide -> position
//   k_poses_planes    one block per pose: pose coordinates in LDS; geometry of the listed rings and amides; the rings the pose
//                     comes near (an LDS hash set); residue and selection flags of every affected ring (a wave per ring);
//                     then a wave per home item — affected ring, movable atom, moved amide — enumerates candidates with cheap
//                     squared distances into a per-wave LDS queue, and whenever 64 have gathered they are evaluated one per
//                     lane with the operation sequences of ap_eval / pp_eval / gg_eval / gp_eval on VALUES (a moved entity's
//                     operands are the pose's, an unmoved one's the resident arrays').  Records leave with one atomic per
//                     evaluated wave, unsorted, with a sort key table | pose | first id | second id
//   (k_poses_offsets  of arp_poses.h, a block per table: pose_off[t][p] = exclusive prefix of the summaries' counts)
//   k_ppl_columns     the sorted slots gathered into each table's columns
//
// selection_plus of a pose: an unselected atom is in it when it lies within 6.0 A (inclusive, float64) of a movable atom's
// pose coordinate; a residue when it is selected or holds such an atom.  Both are evaluated ON DEMAND, in phase 2, for the few
// entities that get there (the residue through the CSR): a per-pose mark sweep over all atoms would cost n x S tests a pose
// where this costs a few hundred.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "arp_planes.h"
#include "arp_poses.h"

#define PPL_THREADS 256
#define PPL_WAVES (PPL_THREADS / 64)
#define PPL_MAX_RINGS 512        // rings with a movable atom
#define PPL_MAX_HOME 512         // further rings affected at the movable atoms' resident coordinates
#define PPL_MAX_AMIDES 512       // moved amides
#define PPL_MAX_NEAR 256         // further rings one pose affects by proximity
#define PPL_NEAR_HASH 1024
#define PPL_QCAP 192
#define PPL_SUMMARY 16
#define PPL_MAX_BLOCKS 512
#define PPL_E_NEAR 77            // device error word: a pose's proximity-affected rings outgrew PPL_MAX_NEAR

struct __attribute__((aligned(16))) PplRing {      // an affected ring of the pose a block works on
    double c[3], n[3];
    int id, res;
    unsigned flags;              // 1 sel, 2 plus
    int pad;
};
struct __attribute__((aligned(16))) PplAmide {     // a moved amide
    float c[3], n[3];
    int id;
    unsigned flags;
};

struct PplArgs {
    int n, S, P, nring, namide;
    const int* sel_list;
    const int* pos_of;
    const uint8_t* sel;
    const float* pxyz;           // [P][S][3]
    const int* ring_off;
    const int* ring_idx;
    const int* amide_atoms;
    const int* mring;            // rings with a movable atom
    const int* hring;            // further rings affected at home
    const int* mamide;           // moved amides
    int n_mring, n_hring, n_mamide;
    const uint8_t* ring_static;  // 0 not on a static list, 1 movable atom in the path, 2 affected at home
    const int* am_pos;           // position among the moved amides, -1: not moved
    const uint8_t* res_selm;     // residue holds a selected atom
    const int* res_off;          // residue -> atoms
    const int* res_atoms;
    const float4* xyz;           // by local id
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
    PplRing* ws_ring;            // [blocks][ws_rings]
    PplAmide* ws_amide;          // [blocks][max(n_mamide, 1)]
    int ws_rings;
    PlaneRec* rec;
    u64* key;
    u64* val;
    u64 cap;
    u64* ctr;                    // [0] records appended (exact, also beyond cap), [1] error word, [2 .. 5] records per table
    uint32_t* summary;           // [P][16]
    int idbits, pbits;
};

// ---- set-up ----------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void k_ppl_mark(int n, int S, const int* __restrict__ sel_list, const uint8_t* __restrict__ sel,
                                                  const int* __restrict__ res_id, int* __restrict__ pos_of, uint8_t* __restrict__ res_selm,
                                                  int* __restrict__ hist) {
    for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < n; i += gridDim.x * blockDim.x) {
        const int r = res_id[i];
        if (sel[i]) res_selm[r] = 1;
        atomicAdd(&hist[r], 1);
        if (i < S) pos_of[sel_list[i]] = i;
    }
}

__global__ __launch_bounds__(256) void k_ppl_lists(PplArgs A, int* __restrict__ mring, int* __restrict__ hring, int* __restrict__ mamide,
                                                   uint8_t* __restrict__ ring_static, int* __restrict__ am_pos, int* __restrict__ cnt) {
    for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < A.nring + A.namide; i += gridDim.x * blockDim.x) {
        if (i < A.nring) {
            const int r = i;
            bool has = false;
            for (int k = A.ring_off[r]; k < A.ring_off[r + 1]; ++k) has |= A.pos_of[A.ring_idx[k]] >= 0;
            uint8_t kind = 0;
            if (has) {
                const int slot = atomicAdd(&cnt[0], 1);
                if (slot < PPL_MAX_RINGS) mring[slot] = r;
                kind = 1;
            } else {
                const num::d3 ctr_ = ld3(A.ring_c, r);
                bool near = false;
                for (int s = 0; s < A.S && !near; ++s) {
                    const float4 v = A.xyz[A.sel_list[s]];
                    near = num::dist2_kd(ctr_, num::d3{(double)v.x, (double)v.y, (double)v.z}) <= 9.0;
                }
                if (near) {
                    const int slot = atomicAdd(&cnt[1], 1);
                    if (slot < PPL_MAX_HOME) hring[slot] = r;
                    kind = 2;
                }
            }
            ring_static[r] = kind;
        } else {
            const int a = i - A.nring;
            const bool moved = A.pos_of[A.amide_atoms[4 * a]] >= 0 || A.pos_of[A.amide_atoms[4 * a + 1]] >= 0 || A.pos_of[A.amide_atoms[4 * a + 2]] >= 0;
            int pos = -1;
            if (moved) {
                const int slot = atomicAdd(&cnt[2], 1);
                if (slot < PPL_MAX_AMIDES) { mamide[slot] = a; pos = slot; }
            }
            am_pos[a] = pos;
        }
    }
}

// ---- per pose --------------------------------------------------------------------------------------------------------
struct PplShared {
    float px[POSES_MAX_ATOMS * 3];
    int4 q[PPL_WAVES][PPL_QCAP];
    int hash[PPL_NEAR_HASH];
    uint32_t sum[PPL_SUMMARY];
    int n_near, bad, over;
};

// the coordinate of atom lid in the pose
__device__ __forceinline__ num::f3 ppl_coord(const PplArgs& A, const float* px, int lid) {
    const int s = A.pos_of[lid];
    if (s >= 0) return {px[3 * s], px[3 * s + 1], px[3 * s + 2]};
    const float4 v = A.xyz[lid];
    return {v.x, v.y, v.z};
}

// k_ring_geometry's operation sequence over a pose's coordinates: `at(k)` is the pose's coordinate of the atom that the path names k
// (k_poses_planes: a local id; k_library_planes: an index within the ligand)
template <class Coord>
__device__ __forceinline__ void ppl_ring_geometry_of(const Coord& at, const int* idx, int na, double* c, double* nrm) {
    double cx = 0, cy = 0, cz = 0;
    for (int j = 0; j < na; ++j) {
        const num::f3 v = at(idx[j]);
        cx += (double)v.x; cy += (double)v.y; cz += (double)v.z;
    }
    const double inv_n = 1.0 / (double)na;
    cx *= inv_n; cy *= inv_n; cz *= inv_n;
    double nx = 0, ny = 0, nz = 0;
    for (int j = 0; j < na; ++j) {
        const num::f3 p = at(idx[j]), q = at(idx[(j + 1 == na) ? 0 : j + 1]);
        const double ax = (double)p.x - cx, ay = (double)p.y - cy, az = (double)p.z - cz;
        const double bx = (double)q.x - cx, by = (double)q.y - cy, bz = (double)q.z - cz;
        nx += ay * bz - az * by;
        ny += az * bx - ax * bz;
        nz += ax * by - ay * bx;
    }
    nx *= inv_n; ny *= inv_n; nz *= inv_n;
    const double l = sqrt(nx * nx + ny * ny + nz * nz);
    if (!(fabs(l) < 2e-6)) {
        const double inv_l = 1.0 / l;
        nx *= inv_l; ny *= inv_l; nz *= inv_l;
    }
    c[0] = cx; c[1] = cy; c[2] = cz;
    nrm[0] = nx; nrm[1] = ny; nrm[2] = nz;
}
__device__ __forceinline__ void ppl_ring_geometry(const PplArgs& A, const float* px, int r, double* c, double* nrm) {
    const int a0 = A.ring_off[r];
    ppl_ring_geometry_of([&](int lid) { return ppl_coord(A, px, lid); }, A.ring_idx + a0, A.ring_off[r + 1] - a0, c, nrm);
}

// k_amide_geometry's, over the amide's N, C, O (atoms[0 .. 2])
template <class Coord>
__device__ __forceinline__ void ppl_amide_geometry_of(const Coord& at, const int* atoms, float* c, float* nrm) {
    const num::f3 N = at(atoms[0]), Cc = at(atoms[1]), O = at(atoms[2]);
    c[0] = (Cc.x + N.x) / 2.0f;
    c[1] = (Cc.y + N.y) / 2.0f;
    c[2] = (Cc.z + N.z) / 2.0f;
    const double mx = ((double)Cc.x + O.x + N.x) / 3.0, my = ((double)Cc.y + O.y + N.y) / 3.0, mz = ((double)Cc.z + O.z + N.z) / 3.0;
    const double ux = Cc.x - mx, uy = Cc.y - my, uz = Cc.z - mz;
    const double vx = O.x - mx, vy = O.y - my, vz = O.z - mz;
    double nx = uy * vz - uz * vy, ny = uz * vx - ux * vz, nz = ux * vy - uy * vx;
    const double l = sqrt(nx * nx + ny * ny + nz * nz);
    if (l > 0) { nx /= l; ny /= l; nz /= l; }
    nrm[0] = (float)nx; nrm[1] = (float)ny; nrm[2] = (float)nz;
}
__device__ __forceinline__ void ppl_amide_geometry(const PplArgs& A, const float* px, int a, float* c, float* nrm) {
    ppl_amide_geometry_of([&](int lid) { return ppl_coord(A, px, lid); }, A.amide_atoms + 4 * a, c, nrm);
}

// an unselected atom at x: within 6.0 A (inclusive, float64) of a movable atom's pose coordinate
__device__ __forceinline__ bool ppl_atom_plus(const PplArgs& A, const float* px, num::d3 x) {
    for (int s = 0; s < A.S; ++s)
        if (num::dist2_kd(x, num::d3{(double)px[3 * s], (double)px[3 * s + 1], (double)px[3 * s + 2]}) <= 36.0) return true;
    return false;
}
// residue res in the pose's selection_plus residues: selected, or one of its atoms is (one lane)
__device__ __forceinline__ bool ppl_res_plus(const PplArgs& A, const float* px, int res) {
    if (res < 0) return false;
    if (A.res_selm[res]) return true;
    for (int k = A.res_off[res], k1 = A.res_off[res + 1]; k < k1; ++k) {
        const float4 v = A.xyz[A.res_atoms[k]];
        if (ppl_atom_plus(A, px, num::d3{(double)v.x, (double)v.y, (double)v.z})) return true;
    }
    return false;
}
// ... by a whole wave (res is wave-uniform)
__device__ __forceinline__ bool ppl_res_plus_wave(const PplArgs& A, const float* px, int res, int lane) {
    if (res < 0) return false;
    if (A.res_selm[res]) return true;
    bool p = false;
    for (int k = A.res_off[res] + lane, k1 = A.res_off[res + 1]; k < k1; k += 64) {
        const float4 v = A.xyz[A.res_atoms[k]];
        p = p || ppl_atom_plus(A, px, num::d3{(double)v.x, (double)v.y, (double)v.z});
    }
    return __any(p) != 0;
}

__device__ __forceinline__ unsigned ppl_hash(int r) { return ((unsigned)r * 2654435761u) >> 22; }      // 10 bits
__device__ __forceinline__ void ppl_near_insert(PplShared* sh, int r) {
    unsigned h = ppl_hash(r);
    for (int probe = 0; probe < PPL_NEAR_HASH; ++probe) {
        const int old = atomicCAS(&sh->hash[h], -1, r);
        if (old == -1 || old == r) return;
        h = (h + 1) & (PPL_NEAR_HASH - 1);
    }
    sh->over = 1;
}
__device__ __forceinline__ bool ppl_affected(const PplArgs& A, const PplShared* sh, int r) {
    if (A.ring_static[r]) return true;
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

// operands of phase 2, as values.  A reference < 0 names entry -ref - 1 of the pose's lists, one >= 0 a resident id.
struct PplRingV { int id, res; bool sel, plus; num::d3 c, n; };
struct PplAmideV { int id; bool sel, plus; num::f3 c, n; };
__device__ __forceinline__ PplRingV ppl_ring(const PplArgs& A, const PplRing* ws, const float* px, int ref) {
    PplRingV R;
    if (ref < 0) {
        const PplRing* w = ws + (-ref - 1);
        R.id = w->id; R.res = w->res; R.sel = (w->flags & 1u) != 0; R.plus = (w->flags & 2u) != 0;
        R.c = {w->c[0], w->c[1], w->c[2]};
        R.n = {w->n[0], w->n[1], w->n[2]};
    } else {
        R.id = ref; R.res = A.ring_res[ref];
        R.sel = R.res >= 0 && A.res_selm[R.res];
        R.plus = ppl_res_plus(A, px, R.res);
        R.c = ld3(A.ring_c, ref);
        R.n = ld3(A.ring_n, ref);
    }
    return R;
}
__device__ __forceinline__ PplAmideV ppl_amide(const PplArgs& A, const PplAmide* ws, const float* px, int ref) {
    PplAmideV G;
    if (ref < 0) {
        const PplAmide* w = ws + (-ref - 1);
        G.id = w->id; G.sel = (w->flags & 1u) != 0; G.plus = (w->flags & 2u) != 0;
        G.c = {w->c[0], w->c[1], w->c[2]};
        G.n = {w->n[0], w->n[1], w->n[2]};
    } else {
        const int res = A.am_res[ref];
        G.id = ref;
        G.sel = res >= 0 && A.res_selm[res];
        G.plus = ppl_res_plus(A, px, res);
        G.c = lf3(A.am_c, ref);
        G.n = lf3(A.am_n, ref);
    }
    return G;
}

// How k_poses_planes reads the operands of phase 2: a reference < 0 names entry -ref - 1 of the pose's lists (a movable atom: of
// sel_list), one >= 0 a resident id.  k_library_planes (arp_library_planes.h) reads the same decisions through a reader of its own.
// A reader gives ring(ref), amide(ref), atom(ref, ...) and, as `A`, the record sink: rec, key, val, cap, ctr, idbits, pbits.
struct PplReader {
    const PplArgs& A;
    const PplRing* wsr;
    const PplAmide* wsa;
    const float* px;
    __device__ __forceinline__ PplRingV ring(int ref) const { return ppl_ring(A, wsr, px, ref); }
    __device__ __forceinline__ PplAmideV amide(int ref) const { return ppl_amide(A, wsa, px, ref); }
    // atom `ref`: its id, coordinate and meta word in the pose, and whether it is in the pose's selection_plus
    __device__ __forceinline__ void atom(int ref, int* lid, num::d3* x, uint32_t* m, bool* plus) const {
        if (ref < 0) {
            const int s = -ref - 1;
            *lid = A.sel_list[s];
            *x = {(double)px[3 * s], (double)px[3 * s + 1], (double)px[3 * s + 2]};
            *m = __float_as_uint(A.st_xyzm[*lid].w) | M_SEL;
        } else {
            *lid = ref;
            const float4 v = A.st_xyzm[ref];
            *x = {(double)v.x, (double)v.y, (double)v.z};
            *m = __float_as_uint(v.w) & ~(uint32_t)M_SEL;
            *plus = ppl_atom_plus(A, px, *x);
        }
    }
};

// Phase 2: one candidate per lane, e = {table, first reference, second reference}.  The decisions and the arithmetic are those of
// ap_eval, pp_eval, gg_eval and gp_eval (arp_planes.h), expression by expression: the ONE text for the poses of one ligand and
// for a ligand library.  `sum`: the block's summary row in LDS.
template <class Reader>
__device__ __forceinline__ void ppl_eval(const Reader& rd, uint32_t* sum, int pose, bool live, int4 e, int lane) {
    const auto& A = rd.A;
    const int kind = e.x;
    bool emit = false;
    PlaneRec rec;
    rec.i0 = rec.i1 = 0; rec.u = 0; rec.pad = (unsigned)kind;
    rec.d0 = rec.d1 = rec.d2 = rec.d3 = 0.0;
    int k0 = 0, k1 = 0;         // the two ids of the sort key
    int ct = 0;
    if (live && kind == 0) {                 // ring e.y, atom e.z
        const PplRingV R = rd.ring(e.y);
        int lid;
        num::d3 x;
        uint32_t m;
        bool plus = true;
        rd.atom(e.z, &lid, &x, &m, &plus);
        if (R.plus && plus) {
            const double dist = num::norm(num::sub(x, R.c));
            ct = plane_ctype(R.sel, (m & M_SEL) != 0, true, true);
            const double cost = num::group_cos(R.n, num::sub(R.c, x));
            const double theta = num::fold_deg(acos(cost));
            uint32_t mask = 0;
            if (dist <= 4.5 && num::fold_le(cost, ARP_FOLD_COS_30_POS, ARP_FOLD_COS_30_NEG)) {
                if ((m & M_ELEM_C) && (m & ARP_T_WEAK_HBOND_DONOR)) mask |= ARP_AP_CARBONPI;
                if (m & ARP_T_POS_IONISABLE) mask |= ARP_AP_CATIONPI;
                if (m & ARP_T_HBOND_DONOR) mask |= ARP_AP_DONORPI;
                if (m & ARP_T_XBOND_DONOR) mask |= ARP_AP_HALOGENPI;
            }
            if (dist <= 6.0) {
                if ((m & M_RES_MET) && (m & M_ELEM_S)) mask |= ARP_AP_METSULPHURPI;
            }
            emit = mask != 0;
            rec.i0 = lid; rec.i1 = R.id;
            rec.d0 = dist; rec.d1 = theta;
            rec.u = mask | ((unsigned)ct << 8);
            k0 = R.id; k1 = lid;
        }
    } else if (live && kind == 1) {          // two rings
        PplRingV Ra = rd.ring(e.y), Rb = rd.ring(e.z);
        if (Ra.id > Rb.id) { const PplRingV t = Ra; Ra = Rb; Rb = t; }
        if (Ra.plus && Rb.plus) {
            const num::d3 pab = num::sub(Ra.c, Rb.c);
            const double dist = num::norm(pab);
            if (!(dist > 6.0)) {
                const bool intra = Ra.res == Rb.res;
                ct = plane_ctype(Ra.sel, Rb.sel, true, true);
                const double cosd = num::dot(Ra.n, Rb.n) / (num::norm(Ra.n) * num::norm(Rb.n));
                const double dih = num::fold_deg(acos(cosd));
                const double c_ab = num::group_cos(Ra.n, pab);
                const double c_ba = num::group_cos(Rb.n, num::sub(Rb.c, Ra.c));
                const double t_ab = num::fold_deg(acos(c_ab)), t_ba = num::fold_deg(acos(c_ba));
                const int y_ab = num::pp_class(cosd, c_ab), y_ba = num::pp_class(cosd, c_ba);
                const bool skip_ab = intra && y_ab == ARP_PP_EE;
                const bool skip_ba = intra && y_ba == ARP_PP_EE;
                emit = !(skip_ab && skip_ba);
                const bool first = !skip_ab;
                double t1, t2;
                int y1, y2;
                if (first) {
                    t1 = t_ab; t2 = skip_ba ? NAN : t_ba;
                    y1 = y_ab; y2 = skip_ba ? ARP_PP_SKIPPED : (y_ba == y_ab ? ARP_PP_SAME : y_ba);
                } else {
                    t1 = t_ba; t2 = NAN;
                    y1 = y_ba; y2 = ARP_PP_SKIPPED;
                }
                rec.i0 = first ? Ra.id : Rb.id;
                rec.i1 = first ? Rb.id : Ra.id;
                rec.d0 = dist; rec.d1 = dih; rec.d2 = t1; rec.d3 = t2;
                rec.u = (unsigned)y1 | ((unsigned)y2 << 8) | ((unsigned)ct << 16);
                k0 = rec.i0; k1 = rec.i1;
            }
        }
    } else if (live && kind == 2) {          // ordered pair of amides
        const PplAmideV Ga = rd.amide(e.y), Gb = rd.amide(e.z);
        if (Ga.plus && Gb.plus) {
            const num::f3 pab = num::sub(Ga.c, Gb.c);
            const float dist = num::norm(pab);
            if (!(dist > (float)6.0)) {
                const float cosd = num::dot(Ga.n, Gb.n) / (num::norm(Ga.n) * num::norm(Gb.n));
                const float dih = num::fold_deg(acosf(cosd));
                const float cost = num::group_cos(Ga.n, pab);
                const float theta = num::fold_deg(acosf(cost));
                emit = !(num::fold_gt_30(cosd) || num::fold_gt_30(cost));
                ct = plane_ctype(Ga.sel, Gb.sel, true, true);
                rec.i0 = Ga.id; rec.i1 = Gb.id;
                rec.d0 = (double)dist; rec.d1 = (double)dih; rec.d2 = (double)theta;
                rec.u = (unsigned)ct;
                k0 = Ga.id; k1 = Gb.id;
            }
        }
    } else if (live && kind == 3) {          // amide e.y, ring e.z
        const PplAmideV G = rd.amide(e.y);
        const PplRingV R = rd.ring(e.z);
        if (G.plus && R.plus) {
            const num::d3 cad = num::to_d3(G.c);
            const num::d3 par = num::sub(cad, R.c);
            const double dist = num::norm(par);
            if (!(dist > 6.0)) {
                const double cosd = num::dot(num::to_d3(G.n), R.n) / ((double)num::norm(G.n) * num::norm(R.n));
                const double dih = num::fold_deg(acos(cosd));
                const double cost = num::group_cos(G.n, par);
                const double theta = num::fold_deg(acos(cost));
                emit = !(num::fold_gt_30(cosd) || num::fold_gt_30(cost));
                ct = plane_ctype(G.sel, R.sel, true, true);
                rec.i0 = G.id; rec.i1 = R.id;
                rec.d0 = dist; rec.d1 = dih; rec.d2 = theta;
                rec.u = (unsigned)ct;
                k0 = G.id; k1 = R.id;
            }
        }
    }
    const unsigned long long me = __ballot(emit);
    if (!me) return;
    unsigned long long base = 0;
    if (lane == 0) base = atomicAdd(A.ctr, (unsigned long long)__popcll(me));
    base = __shfl(base, 0);
    if (emit) {
        const u64 slot = base + (u64)__popcll(me & ((1ull << lane) - 1ull));
        if (slot < A.cap) {
            A.rec[slot] = rec;
            A.key[slot] = ((u64)(unsigned)kind << (A.pbits + 2 * A.idbits)) | ((u64)(unsigned)pose << (2 * A.idbits)) | ((u64)(unsigned)k0 << A.idbits) |
                          (u64)(unsigned)k1;
            A.val[slot] = slot;
        }
    }
    // the summary: records per table, INTER atom-plane records per ARP_AP_* bit, INTER records of the other tables, all
    const bool inter = emit && ct == ARP_CT_INTER;
    uint32_t add[PPL_SUMMARY];
#pragma unroll
    for (int b = 0; b < PPL_SUMMARY; ++b) add[b] = 0u;
#pragma unroll
    for (int t = 0; t < 4; ++t) add[t] = (uint32_t)__popcll(__ballot(emit && kind == t));
#pragma unroll
    for (int b = 0; b < 5; ++b) add[4 + b] = (uint32_t)__popcll(__ballot(inter && kind == 0 && ((rec.u >> b) & 1u)));
#pragma unroll
    for (int t = 1; t < 4; ++t) add[8 + t] = (uint32_t)__popcll(__ballot(inter && kind == t));
    add[15] = (uint32_t)__popcll(me);
    if (lane == 0) {
#pragma unroll
        for (int b = 0; b < PPL_SUMMARY; ++b)
            if (add[b]) atomicAdd(&sum[b], add[b]);
    }
}

__global__ __launch_bounds__(PPL_THREADS) void k_poses_planes(PplArgs A) {
    __shared__ PplShared s_sh;
    PplShared* const sh = &s_sh;
    const int tid = (int)threadIdx.x, lane = tid & 63, w = __builtin_amdgcn_readfirstlane(tid >> 6);
    PplRing* const wsr = A.ws_ring + (size_t)blockIdx.x * A.ws_rings;
    PplAmide* const wsa = A.ws_amide + (size_t)blockIdx.x * (A.n_mamide > 0 ? A.n_mamide : 1);
    const float* const px = sh->px;
    const int nSA = A.n_mring + A.n_hring;
    for (int pose = blockIdx.x; pose < A.P; pose += gridDim.x) {
        // ---- the pose's coordinates
        if (tid < PPL_SUMMARY) sh->sum[tid] = 0u;
        for (int k = tid; k < PPL_NEAR_HASH; k += PPL_THREADS) sh->hash[k] = -1;
        if (tid == 0) { sh->n_near = 0; sh->bad = 0; sh->over = 0; }
        __syncthreads();
        {
            const float* const src = A.pxyz + (size_t)pose * A.S * 3;
            bool bad = false;
            for (int k = tid; k < 3 * A.S; k += PPL_THREADS) {
                const float v = src[k];
                sh->px[k] = v;
                bad |= !isfinite(v);
            }
            if (bad) sh->bad = 1;
        }
        __syncthreads();
        if (sh->bad) {      // (block-uniform)
            if (tid == 0) atomicExch((int*)(A.ctr + 1), ARP_E_ARG);
            if (tid < PPL_SUMMARY) A.summary[(size_t)pose * PPL_SUMMARY + tid] = 0u;
            __syncthreads();
            continue;
        }
        // ---- geometry of the listed rings and amides; the rings affected at home keep theirs
        for (int i = tid; i < nSA; i += PPL_THREADS) {
            PplRing* o = wsr + i;
            const int r = i < A.n_mring ? A.mring[i] : A.hring[i - A.n_mring];
            if (i < A.n_mring) ppl_ring_geometry(A, px, r, o->c, o->n);
            else {
                for (int q = 0; q < 3; ++q) { o->c[q] = A.ring_c[3 * (size_t)r + q]; o->n[q] = A.ring_n[3 * (size_t)r + q]; }
            }
            o->id = r; o->res = -1; o->flags = 0u; o->pad = 0;
        }
        for (int k = tid; k < A.n_mamide; k += PPL_THREADS) {
            PplAmide* o = wsa + k;
            const int a = A.mamide[k];
            ppl_amide_geometry(A, px, a, o->c, o->n);
            o->id = a; o->flags = 0u;
        }
        // ---- the further rings this pose comes near: a wave per movable atom, the ring-centre grid around its pose coordinate
        if (A.nring > 0) {
            for (int s = w; s < A.S; s += PPL_WAVES) {
                const num::d3 x = {(double)px[3 * s], (double)px[3 * s + 1], (double)px[3 * s + 2]};
                const Stencil st = stencil_load(A.gr, A.r_start, cell_box(A.gr, x), lane);
                for (int kb = 0; kb < st.pre[9]; kb += 64) {
                    const int k = kb + lane;
                    if (k < st.pre[9]) {
                        const int r = A.r_perm[stencil_pos(st, k)];
                        if (!A.ring_static[r] && num::dist2_kd(ld3(A.ring_c, r), x) <= 9.0) ppl_near_insert(sh, r);
                    }
                }
            }
        }
        __syncthreads();
        for (int h = tid; h < PPL_NEAR_HASH; h += PPL_THREADS) {
            const int r = sh->hash[h];
            if (r >= 0) {
                const int slot = atomicAdd(&sh->n_near, 1);
                if (slot < PPL_MAX_NEAR) {
                    PplRing* o = wsr + nSA + slot;
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
        const int nAff = nSA + sh->n_near;
        // ---- residue and selection flags of every affected ring (k_ring_residue over unselected atoms at home and movable atoms
        // in the pose), the pose's selection_plus flag of every moved amide
        uint32_t n_diff = 0, n_none = 0;
        for (int i = w; i < nAff + A.n_mamide; i += PPL_WAVES) {
            if (i >= nAff) {
                PplAmide* o = wsa + (i - nAff);
                const int res = A.am_res[o->id];
                const bool plus = ppl_res_plus_wave(A, px, res, lane);
                if (lane == 0) o->flags = ((res >= 0 && A.res_selm[res]) ? 1u : 0u) | (plus ? 2u : 0u);
                continue;
            }
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
                        if (!A.sel[lid] && num::dist2_kd(ctr_, x) <= 9.0) {
                            const double d = num::norm(num::sub(x, ctr_));
                            if (d < best || (d == best && lid < best_lid)) { best = d; best_lid = lid; }
                        }
                    }
                }
            }
            for (int s = lane; s < A.S; s += 64) {
                const num::d3 x = {(double)px[3 * s], (double)px[3 * s + 1], (double)px[3 * s + 2]};
                if (num::dist2_kd(ctr_, x) <= 9.0) {
                    const double d = num::norm(num::sub(x, ctr_));
                    const int lid = A.sel_list[s];
                    if (d < best || (d == best && lid < best_lid)) { best = d; best_lid = lid; }
                }
            }
            for (int o_ = 32; o_ > 0; o_ >>= 1) {
                const double od = __shfl_xor(best, o_);
                const int ol = __shfl_xor(best_lid, o_);
                if (od < best || (od == best && ol < best_lid)) { best = od; best_lid = ol; }
            }
            const int res = best_lid != 0x7FFFFFFF ? A.res_id[best_lid] : -1;
            const bool plus = ppl_res_plus_wave(A, px, res, lane);
            if (lane == 0) {
                o->res = res;
                o->flags = ((res >= 0 && A.res_selm[res]) ? 1u : 0u) | (plus ? 2u : 0u);
                n_diff += res != A.ring_res[o->id] ? 1u : 0u;
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
        const PplReader reader{A, wsr, wsa, px};
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
        const int items = nAff + A.S + A.n_mamide;
        for (int it = w; it < items; it += PPL_WAVES) {
            if (it < nAff) {
                // affected ring i: every atom (atom-plane), every ring (plane-plane), every unmoved amide (group-plane)
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
                            ok = !A.sel[lid] && num::dist2_kd(ctr_, num::d3{(double)v.x, (double)v.y, (double)v.z}) <= 36.0 &&
                                 !(m & (M_HYDROGEN | ARP_T_AROMATIC));
                        }
                        push(ok, 0, -(i + 1), lid);
                    }
                }
                for (int sb_ = 0; sb_ < A.S; sb_ += 64) {
                    const int s = sb_ + lane;
                    bool ok = false;
                    if (s < A.S) {
                        const uint32_t m = __float_as_uint(A.st_xyzm[A.sel_list[s]].w);
                        ok = num::dist2_kd(ctr_, num::d3{(double)px[3 * s], (double)px[3 * s + 1], (double)px[3 * s + 2]}) <= 36.0 &&
                             !(m & (M_HYDROGEN | ARP_T_AROMATIC));
                    }
                    push(ok, 0, -(i + 1), -(s + 1));
                }
                {
                    const Stencil st = stencil_load(A.gr, A.r_start, cell_box(A.gr, ctr_), lane);
                    for (int kb = 0; kb < st.pre[9]; kb += 64) {
                        const int k = kb + lane;
                        bool ok = false;
                        int b = 0;
                        if (k < st.pre[9]) {
                            b = A.r_perm[stencil_pos(st, k)];
                            ok = !ppl_affected(A, sh, b) && num::dist2_kd(ctr_, ld3(A.ring_c, b)) <= 36.0 * (1.0 + 1e-9);
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
                            ok = A.am_pos[a] < 0 && num::dist2_kd(num::to_d3(lf3(A.am_c, a)), ctr_) <= 36.0 * (1.0 + 1e-9);
                        }
                        push(ok, 3, a, -(i + 1));
                    }
                }
            } else if (it < nAff + A.S) {
                // movable atom s: the unaffected rings around its pose coordinate (atom-plane)
                const int s = it - nAff;
                const uint32_t m = __float_as_uint(A.st_xyzm[A.sel_list[s]].w);
                if ((m & (M_HYDROGEN | ARP_T_AROMATIC)) || A.nring == 0) continue;
                const num::d3 x = {(double)px[3 * s], (double)px[3 * s + 1], (double)px[3 * s + 2]};
                const Stencil st = stencil_load(A.gr, A.r_start, cell_box(A.gr, x), lane);
                for (int kb = 0; kb < st.pre[9]; kb += 64) {
                    const int k = kb + lane;
                    bool ok = false;
                    int r = 0;
                    if (k < st.pre[9]) {
                        r = A.r_perm[stencil_pos(st, k)];
                        ok = !ppl_affected(A, sh, r) && num::dist2_kd(ld3(A.ring_c, r), x) <= 36.0;
                    }
                    push(ok, 0, r, -(s + 1));
                }
            } else {
                // moved amide k: every amide, both orders (group-group), every ring (group-plane)
                const int kk = it - nAff - A.S;
                const PplAmide* o = wsa + kk;
                if (!(o->flags & 2u)) continue;
                const num::d3 cad = {(double)o->c[0], (double)o->c[1], (double)o->c[2]};
                {
                    const Stencil st = stencil_load(A.gm, A.m_start, cell_box(A.gm, cad), lane);
                    for (int kb = 0; kb < st.pre[9]; kb += 64) {
                        const int k = kb + lane;
                        bool ok = false;
                        int b = 0;
                        if (k < st.pre[9]) {
                            b = A.m_perm[stencil_pos(st, k)];
                            ok = A.am_pos[b] < 0 && num::dist2_kd(cad, num::to_d3(lf3(A.am_c, b))) <= 36.0 * (1.0 + 1e-5);
                        }
                        push(ok, 2, -(kk + 1), b);
                        push(ok, 2, b, -(kk + 1));
                    }
                }
                for (int tb = 0; tb < A.n_mamide; tb += 64) {
                    const int t = tb + lane;
                    bool ok = false;
                    if (t < A.n_mamide && t != kk)
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
                            ok = !ppl_affected(A, sh, r) && num::dist2_kd(cad, ld3(A.ring_c, r)) <= 36.0 * (1.0 + 1e-9);
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

// the sorted slots as the columns of the four tables (table t holds the sorted positions [base[t], base[t + 1]))
struct PplColumns {
    long long base[5];
    int* i0[4];
    int* i1[4];
    double* d[4][4];            // table 2 (group-group): float columns behind the same pointers
    uint8_t* u[4][3];
};
__global__ __launch_bounds__(256) void k_ppl_columns(long long k, const u64* __restrict__ val, const PlaneRec* __restrict__ rec, PplColumns C) {
    for (long long p = (long long)blockIdx.x * blockDim.x + threadIdx.x; p < k; p += (long long)gridDim.x * blockDim.x) {
        const PlaneRec r = rec[val[p]];
        const int t = p < C.base[1] ? 0 : p < C.base[2] ? 1 : p < C.base[3] ? 2 : 3;
        const long long q = p - C.base[t];
        C.i0[t][q] = r.i0; C.i1[t][q] = r.i1;
        if (t == 0) {
            C.d[0][0][q] = r.d0; C.d[0][1][q] = r.d1;
            C.u[0][0][q] = (uint8_t)(r.u & 255u); C.u[0][1][q] = (uint8_t)((r.u >> 8) & 255u);
        } else if (t == 1) {
            C.d[1][0][q] = r.d0; C.d[1][1][q] = r.d1; C.d[1][2][q] = r.d2; C.d[1][3][q] = r.d3;
            C.u[1][0][q] = (uint8_t)(r.u & 255u); C.u[1][1][q] = (uint8_t)((r.u >> 8) & 255u); C.u[1][2][q] = (uint8_t)((r.u >> 16) & 255u);
        } else if (t == 2) {
            ((float*)C.d[2][0])[q] = (float)r.d0; ((float*)C.d[2][1])[q] = (float)r.d1; ((float*)C.d[2][2])[q] = (float)r.d2;
            C.u[2][0][q] = (uint8_t)(r.u & 255u);
        } else {
            C.d[3][0][q] = r.d0; C.d[3][1][q] = r.d1; C.d[3][2][q] = r.d2;
            C.u[3][0][q] = (uint8_t)(r.u & 255u);
        }
    }
}
