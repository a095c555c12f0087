/*
 * arpeggio_hip.h — C ABI of the MI355X-native contact-detection hot path.
 *
 * This is the drop-in boundary for arpeggio's `InteractionComplex.run_arpeggio`
 * (reference: arpeggio/core/interactions.py:329-347).  The reference is pure
 * Python with no FFI of its own, so every entry point below names the reference
 * function it replaces (file:line, relative to the reference tree; `I:` =
 * arpeggio/core/interactions.py, `U:` = arpeggio/core/utils.py, `C:` =
 * arpeggio/core/config.py).  INTEGRATION.md shows the ctypes binding a
 * maintainer would add on the reference side.
 *
 * Conventions
 *   - extern "C", plain pointers and sizes, no C++/torch types.
 *   - All host buffers are caller-allocated; the library never keeps a host
 *     pointer after a call returns.  Device memory is owned by the context.
 *   - One HIP stream per context; calls are blocking unless named *_launch.
 *   - Return value: ARP_OK or a negative ARP_E_* code; arp_last_error() gives
 *     the message.  ARP_E_CAPACITY stores the required element count in *count
 *     so the caller can re-call with a larger buffer.
 *   - Atom indices in every output are indices into the arrays given to
 *     arp_set_atoms (the "packed atom order").  bgn = lower packed index
 *     (canonical orientation; the reference's own orientation is a hash/KD-tree
 *     artefact).
 */
#ifndef ARPEGGIO_HIP_H
#define ARPEGGIO_HIP_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* ---- error codes -------------------------------------------------------- */
#define ARP_OK            0
#define ARP_E_ARG        -1   /* bad argument / call order */
#define ARP_E_HIP        -2   /* HIP runtime error */
#define ARP_E_CAPACITY   -3   /* output buffer too small; *count = required */
#define ARP_E_XBOND_NBR  -4   /* U:173 dereferenced None: xbond donor without a
                                 single-bond heavy neighbour (reference raises
                                 AttributeError) */
#define ARP_E_NOMEM      -5

/* ---- atom type mask: bit = position in this list (keys of C:53-145) ------ */
#define ARP_T_HBOND_ACCEPTOR       (1u << 0)
#define ARP_T_HBOND_DONOR          (1u << 1)
#define ARP_T_XBOND_ACCEPTOR       (1u << 2)
#define ARP_T_XBOND_DONOR          (1u << 3)
#define ARP_T_WEAK_HBOND_ACCEPTOR  (1u << 4)
#define ARP_T_WEAK_HBOND_DONOR     (1u << 5)
#define ARP_T_POS_IONISABLE        (1u << 6)
#define ARP_T_NEG_IONISABLE        (1u << 7)
#define ARP_T_HYDROPHOBE           (1u << 8)
#define ARP_T_CARBONYL_OXYGEN      (1u << 9)
#define ARP_T_CARBONYL_CARBON      (1u << 10)
#define ARP_T_AROMATIC             (1u << 11)

/* ---- per-atom flags (u16) ------------------------------------------------ */
#define ARP_F_METAL     (1u << 0)   /* I:1990  element in C:27-31            */
#define ARP_F_HALOGEN   (1u << 1)   /* I:1991  element in C:33               */
#define ARP_F_WATER     (1u << 2)   /* get_full_id()[3][0] == 'W' (I:678)    */
#define ARP_F_HYDROGEN  (1u << 3)   /* element.strip() == 'H' (I:712, I:964) */
#define ARP_F_ELEM_C    (1u << 4)   /* element == 'C' (I:1009)               */
#define ARP_F_ELEM_S    (1u << 5)   /* element == 'S' (I:1023)               */
#define ARP_F_RES_MET   (1u << 6)   /* parent resname == 'MET' (I:1023)      */

/* ---- per-residue flags (u8) ---------------------------------------------- */
#define ARP_R_POLYPEPTIDE (1u << 0) /* residue.is_polypeptide (I:1671,1860)  */
#define ARP_R_HAS_SEQ     (1u << 1) /* hasattr(prev_residue/next_residue) (I:736) */

/* ---- atom-atom SIFt bits (order of the name list at I:178-180) ----------- */
#define ARP_S_CLASH         (1u << 0)
#define ARP_S_COVALENT      (1u << 1)
#define ARP_S_VDW_CLASH     (1u << 2)
#define ARP_S_VDW           (1u << 3)
#define ARP_S_PROXIMAL      (1u << 4)
#define ARP_S_HBOND         (1u << 5)
#define ARP_S_WEAK_HBOND    (1u << 6)
#define ARP_S_XBOND         (1u << 7)
#define ARP_S_IONIC         (1u << 8)
#define ARP_S_METAL_COMPLEX (1u << 9)
#define ARP_S_AROMATIC      (1u << 10)
#define ARP_S_HYDROPHOBIC   (1u << 11)
#define ARP_S_CARBONYL      (1u << 12)
#define ARP_S_POLAR         (1u << 13)
#define ARP_S_WEAK_POLAR    (1u << 14)

/* ---- interacting-entities codes (I:643-691, I:985-997, I:1095-1108) ------ */
#define ARP_CT_INTRA_NON_SELECTION  0
#define ARP_CT_INTRA_SELECTION      1
#define ARP_CT_INTER                2
#define ARP_CT_SELECTION_WATER      3
#define ARP_CT_NON_SELECTION_WATER  4
#define ARP_CT_WATER_WATER          5
#define ARP_CT_INTRA_BINDING_SITE   6

/* ---- atom-plane interaction bits (I:1007-1024; alphabetical = bit order) -- */
#define ARP_AP_CARBONPI      (1u << 0)
#define ARP_AP_CATIONPI      (1u << 1)
#define ARP_AP_DONORPI       (1u << 2)
#define ARP_AP_HALOGENPI     (1u << 3)
#define ARP_AP_METSULPHURPI  (1u << 4)

/* ---- plane-plane classes (I:1127-1148); 9 = '' (NaN angles) */
#define ARP_PP_FF 0
#define ARP_PP_OF 1
#define ARP_PP_EE 2
#define ARP_PP_FT 3
#define ARP_PP_OT 4
#define ARP_PP_ET 5
#define ARP_PP_FE 6
#define ARP_PP_OE 7
#define ARP_PP_EF 8
#define ARP_PP_NONE 9
#define ARP_PP_SAME 254      /* reverse visit happened and produced the same class (nothing appended) */
#define ARP_PP_SKIPPED 255   /* reverse visit dropped by the intra-residue EE rule (I:1154) or never made */

typedef struct arp_ctx arp_ctx;

/* ---- lifetime ------------------------------------------------------------ */
const char* arp_version(void);
/* device = HIP device ordinal.  Fails with ARP_E_HIP when no gfx950 device is
 * usable: there is no CPU fallback in this library. */
/* GPUs this process can see (0: none, or no HIP runtime) */
int  arp_device_count(void);
/* Waits until everything enqueued on the context's device has completed (every stream of every context on it): the
 * bracket of a timed region in a host program that has no HIP runtime of its own to ask (bench.py). */
int  arp_device_synchronize(arp_ctx* ctx);
int  arp_create(int device, arp_ctx** out);
void arp_destroy(arp_ctx* ctx);
const char* arp_last_error(arp_ctx* ctx);   /* ctx may be NULL: last create error */

/* ---- inputs: what InteractionComplex.initialize() (I:288-327) leaves behind */
/* Atoms = self.s_atoms (I:54-60).  xyz: atom.coord float32 (P:327).
 * vdw/cov: atom.vdw_radius / atom.cov_radius, Python floats (I:1501,1509).
 * type_mask: atom.atom_types (I:1959-1983).  flags: ARP_F_*.
 * res_id: index of atom.get_parent() in the residue table. */
int arp_set_atoms(arp_ctx* ctx, int64_t n, const float* xyz, const double* vdw,
                  const double* cov, const uint16_t* type_mask,
                  const uint16_t* flags, const int32_t* res_id);
/* Residue table: is_polypeptide / prev_residue / next_residue (I:1671-1693);
 * prev/next are residue indices, -1 = None. */
int arp_set_residues(arp_ctx* ctx, int64_t nres, const uint8_t* res_flags,
                     const int32_t* prev, const int32_t* next);
/* OpenBabel bond graph as CSR over packed atom indices: the set iterated by
 * ob.OBAtomAtomIter(ob_atom_bgn) (I:750). */
int arp_set_bonds(arp_ctx* ctx, const int32_t* bond_off, const int32_t* bond_idx);
/* atom.h_coords (I:1513-1529): CSR, float64 xyz per hydrogen. */
int arp_set_hydrogens(arp_ctx* ctx, const int32_t* h_off, const double* h_xyz);
/* utils.get_single_bond_neighbour (U:612-635) resolved to a packed atom index,
 * -1 = None. */
int arp_set_single_bond_neighbours(arp_ctx* ctx, const int32_t* sb_nbr);
/* biopython_str.rings (I:1697-1733, residue from I:1453-1492; -1 = None). */
int arp_set_rings(arp_ctx* ctx, int64_t nring, const double* center,
                  const double* normal, const int32_t* ring_res);
/* biopython_str.amides (I:1531-1589): float32 centre and normal. */
int arp_set_amides(arp_ctx* ctx, int64_t namide, const float* center,
                   const float* normal, const int32_t* amide_res);

/* ---- the same inputs as ONE blob --------------------------------------------------------
 * Everything arp_set_atoms ... arp_set_amides take, laid out device-ready in one contiguous host
 * buffer (ideally page-locked: arp_host_alloc) and uploaded with a single asynchronous copy.
 * The packer of a structure (what the reference's initialize(), I:288-327, leaves behind) writes
 * straight into the views arp_blob_layout describes; nothing is converted or copied again on the
 * way to the GPU.  Arrays, in the order of off[]:
 *   0 xyz4      float[4n]   x, y, z, 0 per atom (P:327)            11 h_xyz     double[3 nh]   (I:1529)
 *   1 rad       double[2n]  vdw, cov per atom (I:1501,1509)        12 sb_nbr    int32[n]       (U:612-635, -1 = None)
 *   2 type_mask uint16[n]   ARP_T_*                                13 ring_c    double[3 nring]
 *   3 flags     uint16[n]   ARP_F_*                                14 ring_n    double[3 nring]
 *   4 res_id    int32[n]                                           15 ring_res  int32[nring]   (-1 = None)
 *   5 res_flags uint8[nres] ARP_R_*                                16 amide_c   float[3 namide]
 *   6 res_prev  int32[nres]                                        17 amide_n   float[3 namide]
 *   7 res_next  int32[nres]                                        18 amide_res int32[namide]
 *   8 bond_off  int32[n+1]  CSR (I:750)                            19 rad_idx   uint16[n]  index into rad_tab, 0xFFFF = not in it
 *   9 bond_idx  int32[nbond]                                       20 rad_tab   double[2 * 256]  distinct {vdw, cov} pairs
 *  10 h_off     int32[n+1]  CSR (I:1513-1529)
 * (inside the library the arrays go by name: enum BlobArray, csrc/arp_blob.h, in this order, with their sizes in one table)
 * lo/hi, ring_lo/hi, amide_lo/hi = bounding boxes of the atom coordinates / ring centres / amide centres (the grids are
 * sized from them; arp_set_blob verifies that every point lies inside).  n_rad = entries of rad_tab in use.
 * rad[i] MUST equal rad_tab[rad_idx[i]] bit for bit wherever rad_idx[i] != 0xFFFF (arp_blob_fill writes them so): from
 * 32 768 atoms on, when every atom is in the table, arp_set_blob leaves array 1 on the host and the device writes the
 * per-atom radii from the table — a blob that disagrees with itself would be evaluated with the table's values. */
#define ARP_BLOB_MAGIC 0x31424F4C42505241ull   /* "ARPBLOB1" */
#define ARP_BLOB_ARRAYS 21
typedef struct arp_blob_header {
    uint64_t magic, bytes;
    int64_t n, nres, nbond, nh, nring, namide, n_rad;
    uint64_t off[ARP_BLOB_ARRAYS];      /* byte offsets from the start of the blob, 16-byte aligned */
    double lo[3], hi[3], ring_lo[3], ring_hi[3], amide_lo[3], amide_hi[3];
} arp_blob_header;
/* bytes needed for a blob with these counts (header included); 0 on bad counts */
uint64_t arp_blob_size(int64_t n, int64_t nres, int64_t nbond, int64_t nh, int64_t nring, int64_t namide);
/* writes the header (magic, counts, offsets) at the start of `blob`; the caller then fills the arrays, the boxes and n_rad */
int arp_blob_layout(void* blob, uint64_t bytes, int64_t n, int64_t nres, int64_t nbond, int64_t nh, int64_t nring, int64_t namide);
/* Replaces every input of the context with the blob's.  One asynchronous host-to-device copy on the context's stream,
 * then a device-side check of what the classic setters check on the host (finite coordinates inside the box, index
 * ranges, CSR offsets) that the call waits for: ARP_E_ARG if the blob fails it.  The blob may be reused or freed when
 * the call returns.  Selection and ownership are reset (whole structure, I:1395).
 * With its own streams (no caller-owned one) the context also builds what depends on the uploaded arrays only — the 6 A grids of
 * the ring / amide centres and the candidate lists of the ring / amide loops (I:938-1382) — on its second stream beside the
 * check; they may still be running when the call returns, and every later call that reads or replaces what they read or
 * write waits for them on the device (nothing for the caller to do). */
int arp_set_blob(arp_ctx* ctx, const void* blob, uint64_t bytes);
/* Host-only packer: fills every array of a blob whose header arp_blob_layout has written from the arrays the classic
 * setters take (same types and meanings; xyz is float[3 * n], hydrogen coordinates double[3 * nh], ...), builds the
 * dictionary of distinct {vdw, cov} pairs (compared bit for bit; the 256 most frequent if there are more) and the
 * three bounding boxes.  Any pointer whose count is zero may be NULL. */
int arp_blob_fill(void* blob, uint64_t bytes, const float* xyz, const double* vdw, const double* cov, const uint16_t* type_mask,
                  const uint16_t* flags, const int32_t* res_id, const uint8_t* res_flags, const int32_t* res_prev,
                  const int32_t* res_next, const int32_t* bond_off, const int32_t* bond_idx, const int32_t* h_off,
                  const double* h_xyz, const int32_t* sb_nbr, const double* ring_center, const double* ring_normal,
                  const int32_t* ring_res, const float* amide_center, const float* amide_normal, const int32_t* amide_res);

/* ---- Bio.PDB.NeighborSearch equivalents (I:707,960,1394,1420,1442) -------- */
/* NeighborSearch(atoms).search_all(radius): every unordered pair with
 * float64 d^2 <= radius^2, once, as (i<j).  active = optional u8[n] mask of the
 * atoms the tree is built on (NULL = all atoms). */
int arp_search_all(arp_ctx* ctx, double radius, const uint8_t* active,
                   int64_t cap, int32_t* out_i, int32_t* out_j, int64_t* count);

/* NeighborSearch(atoms).search(center, radius) (I:960, 1463) for ncenters centres at once: every (centre, atom) with
 * float64 d^2 <= radius^2 over ALL atoms of the structure (hydrogens included, as the tree of I:1394 / 1455 holds them).
 * centers = double[3 * ncenters].  Output sorted by (centre, atom index).  ARP_E_CAPACITY with the required count in
 * *count when cap is too small.
 * With a batch (arp_set_batch) or models (arp_set_models) resident a centre belongs to no structure: the answer is over
 * ALL resident atoms in their own (world) coordinates, atom index = index in the concatenation — also where the
 * coordinates of two structures overlap. */
int arp_search(arp_ctx* ctx, double radius, int64_t ncenters, const double* centers, int64_t cap, int32_t* out_center,
               int32_t* out_atom, int64_t* count);

/* ---- _make_selection (I:1384-1451) --------------------------------------- */
/* in_selection: u8[n] = utils.selection_parser result (NULL = keep the mask already uploaded,
 * or the whole structure if none was).
 * Computes selection_plus (6.0 A expansion over ALL atoms incl. hydrogens,
 * I:1420-1424), residue sets and ring/amide id sets (I:1416-1417,1434-1437)
 * and keeps them in the context.  Outputs may be NULL. */
int arp_make_selection(arp_ctx* ctx, const uint8_t* in_selection, double expand_radius,
                       uint8_t* out_plus /*n*/, uint8_t* out_ring_sel /*nring*/,
                       uint8_t* out_ring_plus /*nring*/, uint8_t* out_amide_sel /*namide*/,
                       uint8_t* out_amide_plus /*namide*/);

/* Download the sets computed by the last expansion (selection_plus, I:1444-1451). */
int arp_get_selection(arp_ctx* ctx, uint8_t* out_plus, uint8_t* out_ring_sel, uint8_t* out_ring_plus,
                      uint8_t* out_amide_sel, uint8_t* out_amide_plus);

/* Upload a selection mask without expanding it yet (arp_run_launch expands it). */
int arp_set_selection(arp_ctx* ctx, const uint8_t* in_selection);

/* ---- run_arpeggio (I:329-347) --------------------------------------------- */
/* The whole hot path on the resident structure: _make_selection (6.0 A expansion of the
 * selection uploaded by arp_set_selection / arp_make_selection; whole structure if none),
 * _calculate_atom_contacts, _calculate_ring_contacts, _calculate_group_contacts.  Every
 * kernel is enqueued back to back on the context stream with ONE host synchronisation at
 * the end; results stay in HBM until fetched.  counts = records per bag in the order of
 * get_contacts (I:183-210): atom-atom, plane-plane, atom-plane, group-group, group-plane. */
int arp_run_launch(arp_ctx* ctx, double cutoff, double vdw_comp, int include_sequence_adjacent,
                   double expand_radius, int64_t counts[5]);
/* The same pass in two calls, so that ONE host thread can keep several contexts (structures) busy: arp_run_enqueue returns
 * as soon as the launches are enqueued (~15 us of host time), arp_run_wait blocks for the pass, checks the capacities
 * (re-running the pass itself if a buffer was too small) and reports the counts.  Between the two calls only other contexts
 * may be used; every enqueue needs its wait before the next one on the same context. */
int arp_run_enqueue(arp_ctx* ctx, double cutoff, double vdw_comp, int include_sequence_adjacent, double expand_radius);
int arp_run_wait(arp_ctx* ctx, int64_t counts[5]);

/* ---- _calculate_atom_contacts (I:693-936) -------------------------------- */
/* Enqueue bin + sort + neighbour search + fused per-pair SIFt kernels on the
 * context stream; results stay in HBM.  Synchronises the stream before
 * returning and reports the number of emitted contacts.  If the device output
 * buffer was too small it is regrown and the pass re-run internally. */
int arp_atom_contacts_launch(arp_ctx* ctx, double cutoff, double vdw_comp,
                             int include_sequence_adjacent, int64_t* count);
/* Copy the results of the last launch to the host: in the canonical order — ascending
 * (i, j), the order the boundary defines for the reference's KD-tree delivery order
 * (I:707, exported in that order at I:183-190) — once arp_atom_contacts_sort has run on
 * them, otherwise in the order of the device's pair list (any order). */
int arp_atom_contacts_fetch(arp_ctx* ctx, int64_t cap, int32_t* out_i, int32_t* out_j,
                            float* out_dist, uint16_t* out_sift, uint8_t* out_ctype,
                            int64_t* count);
/* Put the atom-atom records of the last launch into the canonical (i, j) order in HBM
 * (csrc/arp_sort.h: least-significant-digit radix passes over the bits of i, three launches per
 * 9-bit digit; then one launch ranks every record by j inside the run of its i and writes the
 * five columns).  Enqueued on the context stream, no host
 * synchronisation; a second call on the same results is a no-op.  Per-atom accumulators
 * and integer sifts do not depend on it. */
int arp_atom_contacts_sort(arp_ctx* ctx);
/* Every result bag of the last pass with ONE device-to-host copy: the atom-atom bag in
 * canonical order (sorted on the device first if it is not yet) and the used prefixes of the
 * four ring / amide bags behind it.  host = caller's buffer (arp_host_alloc for PCIe speed)
 * of host_bytes; counts = records per bag in get_contacts order (I:183-210: atom-atom,
 * plane-plane, atom-plane, group-group, group-plane); offsets[0..4] = byte offsets of i
 * (int32), j (int32), distance (float32), SIFt (uint16), contact type (uint8) of the
 * atom-atom bag; offsets[5 + 12 * b + q] = array q of ring / amide bag b (b = 0..3 in the
 * order of counts[1..4]; q = 0, 1: the two int32 id columns, 2..5: float64 columns, 6..8:
 * float32 columns, 9..11: uint8 columns — the columns of the bag's *_fetch call in its
 * argument order within each type; 0 = the bag has no such array, or no records).  Every ring / amide bag
 * arrives in ITS canonical order as well — plane-plane, group-group and group-plane by (first
 * id, second id), atom-plane by (ring, atom): the order the reference's loops create the
 * records in (I:947-1382) — made on the device (up to ARP_BAG_SORT_MAX records by one block,
 * beyond that by the radix passes of the atom-atom bag).
 * bytes_used = bytes written; ARP_E_CAPACITY with bytes_used set when host_bytes is too small. */
#define ARP_BAG_SORT_MAX 8192
#define ARP_PACKED_OFFSETS 53
int arp_fetch_packed(arp_ctx* ctx, void* host, uint64_t host_bytes, int64_t counts[5],
                     uint64_t offsets[ARP_PACKED_OFFSETS], uint64_t* bytes_used);
/* launch + fetch. */
int arp_atom_contacts(arp_ctx* ctx, double cutoff, double vdw_comp,
                      int include_sequence_adjacent, int64_t cap, int32_t* out_i,
                      int32_t* out_j, float* out_dist, uint16_t* out_sift,
                      uint8_t* out_ctype, int64_t* count);

/* Per-atom side effects of the contact loop, computed from the contact list of the last
 * launch (I:821-852, 923-934; utils.update_atom_sift / update_atom_fsift U:182-221):
 *   out_sift4[4*a + {0,1,2,3}] = atom.sift / sift_inter_only / sift_intra_only / sift_water_only as
 *       15-bit masks (actual_fsift* = the same masks >> 5);
 *   out_counts8[8*a + k] = actual_hbonds, _intra_only, _inter_only, _water_only, actual_polars, ... (same order).
 * utils.update_atom_integer_sift (U:224-242): see arp_atom_integer_sifts. */
int arp_atom_accumulators(arp_ctx* ctx, uint16_t* out_sift4, int32_t* out_counts8);

/* utils.update_atom_integer_sift (U:224-242, called first at I:924-925) from the contact list of the last launch.
 * The reference overwrites atom.integer_sift* at every pair with "binary sift before this pair + this pair", so what
 * is left is decided by the LAST pair of each class that touched the atom, i.e. by the order in which its KD-tree
 * delivered the pairs.  Here the order is the canonical one of this library (contacts sorted by (bgn, end), bgn = lower
 * packed index — the same convention that fixes the bgn/end orientation):
 *   out_isift[60*a + 15*slot + k], slot = {integer_sift, _inter_only, _intra_only, _water_only}, k = SIFt bit,
 *   value = (bit set by an earlier pair of the class) + (bit set by the last pair of the class) in {0, 1, 2}. */
int arp_atom_integer_sifts(arp_ctx* ctx, uint8_t* out_isift);

/* ---- _calculate_ring_contacts (I:938-1206) ------------------------------- */
/* __calculate_atom_plane_contacts (I:947-1062). mask = ARP_AP_* bits. */
int arp_atom_plane(arp_ctx* ctx, int64_t cap, int32_t* out_atom, int32_t* out_ring,
                   double* out_dist, double* out_theta, uint8_t* out_mask,
                   uint8_t* out_ctype, int64_t* count);
/* __calculate_plane_plane_contacts (I:1064-1194), one record per unordered ring
 * pair after the reference's dedupe: type1 = class from the creating visit,
 * type2 = class appended by the reverse visit, ARP_PP_SAME or ARP_PP_SKIPPED. */
int arp_plane_plane(arp_ctx* ctx, int64_t cap, int32_t* out_bgn, int32_t* out_end,
                    double* out_dist, double* out_dihedral, double* out_theta_bgn,
                    double* out_theta_end, uint8_t* out_type1, uint8_t* out_type2,
                    uint8_t* out_ctype, int64_t* count);

/* launch-only / fetch-only halves of the four calls in this section and the next.  A call that replaces an input (structure,
 * selection, ownership, batch, whole-structure assertion; arp_set_blob and arp_shard_assemble included) voids the results of
 * the last launch: these four fetches, arp_atom_contacts_fetch and arp_fetch_packed return ARP_E_ARG until the next launch. */
int arp_atom_plane_launch(arp_ctx* ctx, int64_t* count);
int arp_plane_plane_launch(arp_ctx* ctx, int64_t* count);
int arp_group_group_launch(arp_ctx* ctx, int64_t* count);
int arp_group_plane_launch(arp_ctx* ctx, int64_t* count);
int arp_atom_plane_fetch(arp_ctx* ctx, int64_t cap, int32_t* out_atom, int32_t* out_ring,
                         double* out_dist, double* out_theta, uint8_t* out_mask,
                         uint8_t* out_ctype, int64_t* count);
int arp_plane_plane_fetch(arp_ctx* ctx, int64_t cap, int32_t* out_bgn, int32_t* out_end,
                          double* out_dist, double* out_dihedral, double* out_theta_bgn,
                          double* out_theta_end, uint8_t* out_type1, uint8_t* out_type2,
                          uint8_t* out_ctype, int64_t* count);
int arp_group_group_fetch(arp_ctx* ctx, int64_t cap, int32_t* out_bgn, int32_t* out_end,
                          float* out_dist, float* out_dihedral, float* out_theta,
                          uint8_t* out_ctype, int64_t* count);
int arp_group_plane_fetch(arp_ctx* ctx, int64_t cap, int32_t* out_amide, int32_t* out_ring,
                          double* out_dist, double* out_dihedral, double* out_theta,
                          uint8_t* out_ctype, int64_t* count);

/* ---- _calculate_group_contacts (I:1208-1382) ----------------------------- */
/* __calculate_group_group_contacts (I:1217-1300): ordered amide pairs, float32. */
int arp_group_group(arp_ctx* ctx, int64_t cap, int32_t* out_bgn, int32_t* out_end,
                    float* out_dist, float* out_dihedral, float* out_theta,
                    uint8_t* out_ctype, int64_t* count);
/* __calculate_group_plane_contacts (I:1302-1382): amide x ring, float64. */
int arp_group_plane(arp_ctx* ctx, int64_t cap, int32_t* out_amide, int32_t* out_ring,
                    double* out_dist, double* out_dihedral, double* out_theta,
                    uint8_t* out_ctype, int64_t* count);

/* ---- multi-GPU slab halo -------------------------------------- */
/* Marks which atoms this rank owns (u8[n]; NULL = all).  A pair is emitted by
 * the rank that owns the atom with the lower global id. global_id: i32[n] id
 * used for the ownership/orientation rule and reported in outputs instead of
 * the local index (NULL = local index). */
int arp_set_ownership(arp_ctx* ctx, const uint8_t* is_home, const int32_t* global_id);

/* Same for rings and amides: which ones this rank owns and their global ids (strictly
 * increasing).  plane-plane pairs are emitted by the owner of the lower ring id, atom-plane
 * records by the owner of the ring, group-group / group-plane by the owner of the (bgn) amide. */
int arp_set_group_ownership(arp_ctx* ctx, const uint8_t* ring_home, const int32_t* ring_gid,
                            const uint8_t* amide_home, const int32_t* amide_gid);
/* Coordinates of utils.get_single_bond_neighbour (U:612-635) given inline (float32[n,3] +
 * presence flag), for shards whose neighbour atom lives on another rank. */
int arp_set_single_bond_neighbour_coords(arp_ctx* ctx, const float* sb_xyz, const uint8_t* sb_present);
/* Install an externally combined _make_selection result (I:1444-1451): used by the slab
 * sharding after the halo exchange of selection_plus bits and the all-reduce of the
 * residue sets. */
int arp_set_selection_state(arp_ctx* ctx, const uint8_t* in_selection, const uint8_t* in_plus,
                            const uint8_t* ring_sel, const uint8_t* ring_plus,
                            const uint8_t* amide_sel, const uint8_t* amide_plus);

/* Staged form of arp_run_launch for slab-sharded runs: between the stages the caller combines the
 * selection state of the ranks ON THE DEVICE (RCCL on tensors that alias the context's buffers).
 *   stage 0  selection_plus of the local atoms (I:1384-1424); exact for the atoms this rank owns.
 *            -> caller overwrites the bits of its halo atoms with their owners' (ARP_BUF_PLUS).
 *   stage 1  residue sets of the selection and of selection_plus (I:1413, 1431).
 *            -> caller all-reduces (MAX) the set over the ranks (ARP_BUF_RES_SETS; the shard uses
 *               global residue ids, so the buffer has the same layout on every rank).
 *   stage 2  ring / amide id sets (I:1416-1437), atom contacts, ring and group contacts; fills counts
 *            like arp_run_launch.
 * Each stage returns after the context's streams have drained. */
#define ARP_BUF_PLUS      0   /* u8[n]        selection_plus                                            */
#define ARP_BUF_RES_SETS  1   /* u8[2 * nres] [0,nres) selection residues, [nres,2nres) selection_plus  */
/* For tests of the grid build (read-only, valid until the next call that changes the context): */
#define ARP_BUF_GRID_START 2  /* i32[cells + 1] first record of every cell of the contact grid in place     */
#define ARP_BUF_KEEP_BASE  3  /* i32[blocks + 1] kept rows before every block of the last grid build, which  */
                              /*                read them from this table (ARP_E_ARG if it looked back)      */
int arp_device_buffer(arp_ctx* ctx, int which, uint64_t* device_ptr, int64_t* bytes);
int arp_run_stage(arp_ctx* ctx, int stage, double cutoff, double vdw_comp, int include_sequence_adjacent,
                  double expand_radius, int64_t counts[5]);

/* ---- measurement ---------------------------------------------------------- */
/* stats[0]=candidate pairs tested by the last atom-contact search,
 * stats[1]=pairs with d<=cutoff, stats[2]=pairs passing the residue filters
 * (= emitted contacts), stats[3]=atoms binned, stats[4]=grid cells,
 * stats[5]/[6]=candidates / hits of the last selection-expansion search,
 * stats[7]=how often the grid tables of the resident batch were started over since arp_set_batch: the placement of a
 * batch is cached for four radii (cutoff, expansion radius, 6 A of the ring / amide grids, arp_search_all's); a fifth
 * one starts the cache over and the next pass rebuilds what it had built in the old tables (results do not change). */
int arp_get_stats(arp_ctx* ctx, int64_t stats[8]);
/* When enabled, every kernel of arp_atom_contacts_launch is bracketed by
 * hipEvents on the context stream.  ms[k], launches[k] accumulate per kernel
 * slot: 0 bin, 1 scan, 2 scatter (+ record build), 3 unused, 4 contact search, 5 sift,
 * 6 selection-expansion search, 7 ring/amide kernels.
 * reset != 0 clears the accumulators after reading. */
int arp_set_profiling(arp_ctx* ctx, int enabled);
int arp_get_kernel_times(arp_ctx* ctx, double ms[8], int64_t launches[8], int reset);
/* ---- geometric part of initialize() (I:288-327): from perceived rings / amide groups to what arp_set_rings /
 * arp_set_amides take.  Perception itself (SSSR, aromaticity, the amide SMARTS) is OpenBabel's and not provided. ----
 *
 * _perceive_rings (I:1697-1733) -> OBRing::findCenterAndNormal: centre = mean of the ring atoms, normal = normalised
 * mean of the cross products of consecutive centre->atom vectors, float64.  ring_off[nring+1] / ring_idx: CSR of the
 * ring atoms in ring order (indices into the atoms of arp_set_atoms).  out_*: double[3 * nring]. */
int arp_ring_geometry(arp_ctx* ctx, int64_t nring, const int32_t* ring_off, const int32_t* ring_idx, double* out_center,
                      double* out_normal);
/* _perceive_amide_groups (I:1531-1589): amide_atoms[4 * namide] = N, C, O, C-alpha of every match; centre = (C + N) / 2
 * (float32, I:1569), normal = unit normal of the C, O, N plane (the reference takes the last right-singular vector
 * of the centred coordinates: same direction, sign not reproduced).  out_*: float[3 * namide]. */
int arp_amide_geometry(arp_ctx* ctx, int64_t namide, const int32_t* amide_atoms, float* out_center, float* out_normal);
/* _assign_aromatic_rings_to_residues (I:1453-1492): residue of the atom nearest to each ring centre among ALL atoms
 * within 3.0 A (float64, inclusive), -1 when there is none; out_shortest (may be NULL) = that distance
 * ('residue_shortest_distance', I:1485), -1 when there is none.  Needs arp_set_atoms (and the residue ids given there).
 * With a batch or models resident: over all resident atoms in world coordinates, like arp_search (residue ids of the
 * concatenation; among atoms at the same distance the lowest resident index). */
int arp_ring_residues(arp_ctx* ctx, int64_t nring, const double* center, int32_t* out_ring_res, double* out_shortest);
/* Page-locked (pinned) host memory.  Result buffers allocated here make the *_fetch calls DMA transfers at PCIe speed
 * (a 1.25 M-contact list: 0.5 ms instead of 2.5 ms into pageable memory); any host pointer is accepted by every call. */
int arp_host_alloc(uint64_t bytes, void** out);
int arp_host_free(void* p);
/* The contact grid of a whole-structure pass (no selection, or every atom selected: interactions.py:1395, 1407) is the
 * structure's own neighbour grid — the counterpart of the KD-tree over `entity` (interactions.py:1394) — and is kept: the
 * next pass with the same structure, cutoff and whole selection builds none.  Passes with any other selection compact
 * selection_plus into a new grid every time, as the reference rebuilds NeighborSearch(selection_plus) (interactions.py:1442).
 * enabled = 0 makes every pass build its grid (measurements); default 1. */
int  arp_set_grid_reuse(arp_ctx* ctx, int enabled);
/* The grid build of a whole-structure pass reads where each of its blocks' records begin from a table made from the structure's
 * spatial order; every other pass finds them by a look-back over the blocks before.  enabled = 1 makes every pass look back
 * (tests hold the two against each other; results are the same either way); default 0. */
int  arp_set_compact_lookback(arp_ctx* ctx, int enabled);
/* enabled = 1: arp_run_launch / arp_run_wait enqueue the canonical sort of the atom-atom bag (arp_atom_contacts_sort) as soon as
 * the pass has reported its record count, before they return — for callers that fetch the sorted bag next (arp_fetch_packed,
 * arp_atom_contacts_fetch after a sort; I:183-190 exports every record): the sort then starts a host round trip earlier and runs
 * while the caller gets back to the library.  Default 0 (a caller that only wants counts pays for no sort). */
int  arp_set_sort_after_pass(arp_ctx* ctx, int enabled);
/* Layout of the atom-atom bag inside arp_fetch_packed's one piece.  The canonical order is by (bgn, end), so the bgn column of k
 * records is N + 1 row offsets of information — and the reference's consumers walk the bag atom by atom (get_contacts,
 * interactions.py:183-190; the per-atom accumulators, utils.py:182-242).
 *   ARP_LAYOUT_RECORDS (default)  offsets[0] -> int32 bgn[k]
 *   ARP_LAYOUT_ROWS               offsets[0] -> int32 row[N + 1], N = atoms of the resident structure: the records of atom a are
 *                                 [row[a], row[a + 1]) of the other four columns (end, distance, SIFt, type), row[N] = k.
 *                                 4 k bytes less to copy (100 k atoms, 1.25 M records: 18.8 -> 14.2 MB over PCIe).
 * Not available on a context that holds a shard with global ids (arp_fetch_packed then returns ARP_E_ARG).
 * arp_atom_contacts_fetch always hands out records. */
#define ARP_LAYOUT_RECORDS 0
#define ARP_LAYOUT_ROWS    1
int  arp_set_packed_layout(arp_ctx* ctx, int layout);

/* Sharded runs with NO selection (the reference's default, I:1395: every atom of the structure): the caller
 * asserts that the selection is the whole global structure.  Then selection_plus = selection on every rank and every
 * residue of the table is in both residue sets (I:1413-1437) — including residues whose atoms live on another rank,
 * which the local atoms cannot tell — so arp_run_launch on each shard is exact without any exchange between the
 * ranks.  arp_run_launch refuses (ARP_E_ARG) when the flag is on and the uploaded selection is partial.
 * Precondition: every residue of the table has at least one atom somewhere. */
int arp_set_whole_structure(arp_ctx* ctx, int enabled);
/* ---- exchange between the shards of a distributed structure: RCCL behind the C ABI (the reference has no
 * multi-process mode, so nothing is replaced — these carry the one-cell halo the grid sharding needs).  One process per
 * GPU, one arp_ctx each.  Rank 0 asks for a 128-byte id (arp_comm_unique_id) and hands it to the other processes by
 * whatever means the application has (a file, MPI, a TCP store); every rank then calls arp_comm_init with it.  All
 * transfers run on the context's stream (ncclSend / ncclRecv grouped per neighbour, one ncclAllReduce): no host
 * synchronisation between the kernels of a stage and the exchange that follows.  `librccl.so` is loaded on first use. */
int arp_comm_unique_id(uint8_t* out_id, uint64_t capacity /* >= 128 */);
int arp_comm_init(arp_ctx* ctx, int rank, int world, const uint8_t* unique_id /* 128 bytes */);
int arp_comm_destroy(arp_ctx* ctx);
int arp_comm_info(arp_ctx* ctx, int* rank, int* world);          /* rank / size as RCCL reports them (ncclCommUserRank / ncclCommCount);
                                                                   * ARP_E_ARG while there is no communicator */
/* Halo records of a structure: the two face buffers cut out by arp_shard_pack_face (device pointers; bytes = 0 or a missing
 * neighbour: nothing sent) go to ranks rank - 1 / rank + 1, theirs arrive in buffers the context owns:
 * received = {left pointer, left bytes, right pointer, right bytes}, valid until the next call — the arguments of
 * arp_shard_assemble.  Sizes travel first (one 64-bit word each way), then the records. */
int arp_shard_exchange_faces(arp_ctx* ctx, uint64_t left_ptr, uint64_t left_bytes, uint64_t right_ptr, uint64_t right_bytes,
                             uint64_t received[4]);
/* Per-pass selection exchange of a sharded run WITH a selection (arp_run_stage): the local indices of the atoms whose
 * selection_plus bit each neighbour needs (my home atoms inside its halo, ascending global id) and of the halo atoms it
 * owns (same order on its side).  Uploaded once per structure. */
int arp_shard_set_exchange_lists(arp_ctx* ctx, const int32_t* send_left, int64_t n_send_left, const int32_t* send_right, int64_t n_send_right,
                                 const int32_t* recv_left, int64_t n_recv_left, const int32_t* recv_right, int64_t n_recv_right);
/* between stage 0 and stage 1: halo atoms take their selection_plus bit from their owner (gather, grouped send / recv, scatter) */
int arp_shard_exchange_plus(arp_ctx* ctx);
/* between stage 1 and stage 2: the residue sets (I:1413, 1431) OR-ed over all ranks, in place (ncclAllReduce, MAX over uint8) */
int arp_shard_reduce_residue_sets(arp_ctx* ctx);
/* Several structures in ONE pass — the reference's production use is the weekly PDBe release, ~10^5 entries of a few
 * thousand atoms each (README.md:4), and one such structure is four launches of fixed cost on this chip.  The caller
 * uploads the CONCATENATION of nstruct structures through the usual setters (atom / residue / ring / amide indices
 * shifted by each structure's offsets, coordinates unchanged) and then declares the partition: structure s = atoms
 * [atom_off[s], atom_off[s + 1]), rings [ring_off[s], ..), amides [amide_off[s], ..) (nstruct + 1 entries each, first 0,
 * last = the resident counts); boxes[6 * s ..] = lo x, y, z, hi x, y, z of everything structure s holds (atoms, ring and
 * amide centres).  Every grid of a pass then gives each structure its own cells — its box at an integer cell offset, an
 * empty cell between any two structures — so no neighbour search, selection expansion (I:1420) or ring / amide loop
 * ever pairs items of different structures, while every distance is computed from the same coordinates as in a
 * single-structure run: each structure's five bags are bit-identical to its own run.  Selections: one mask over the
 * concatenated atoms (arp_set_selection).  Results carry the concatenated ids; a record belongs to the structure of its
 * first id.  nstruct = 0 returns to one structure.  Not available on a shard (arp_set_ownership).
 * Items outside their structure's declared box count as its border cells (results do not change; a box much smaller
 * than its contents only makes those cells crowded).  A box needs finite corners, hi >= lo and a finite extent. */
int arp_set_batch(arp_ctx* ctx, int64_t nstruct, const int64_t* atom_off, const int64_t* ring_off, const int64_t* amide_off,
                  const double* boxes);
/* The placement arp_set_batch's grids use at cell edge `radius`, as a pure host function (no context, no GPU; also in
 * libarpeggio_host.so): structure s occupies cells [cx, cx + nx) x [cy, cy + ny) x [cz, cz + nz) of a common grid of
 * dims_out = NX, NY, NZ cells, n = floor((hi - lo) / edge) + 1 per axis; places_out = int32[6 * nstruct] = cx, cy, cz,
 * nx, ny, nz per structure.  *edge_out = the cell edge: radius (1 + 1e-6), grown by 1.26 until every n < 4096 and
 * NX NY NZ <= 2^26.  Any two structures are at least one empty cell apart in some direction.  ARP_E_ARG for boxes
 * arp_set_batch would refuse or a NaN radius. */
int arp_batch_layout(int64_t nstruct, const double* boxes, double radius, int32_t* places_out, int32_t dims_out[3],
                     double* edge_out);
/* Every model of a multi-model structure (an NMR ensemble, the frames of a simulation) in ONE pass.  The reference keeps
 * the first model only (P:67-69: del st[1:]); here the topology is kept on the device once and any number of coordinate
 * sets for it become resident as a batch (arp_set_batch) with one structure per model.
 *
 * arp_set_topology: the topology as a blob (arp_blob_layout / arp_blob_fill; its coordinates are model 1's, its ring
 * and amide centres, normals and ring residues are not read) plus what initialize() perceives on it: ring_off[nring + 1]
 * / ring_idx = the atoms of every ring in ring-path order (at least 3 each), amide_atoms[4 * namide] = N, C, O,
 * C-alpha of every amide group.  The resident structure is not touched.
 *
 * arp_set_models: F = nmodel >= 1 models of the kept topology: xyz = float[F][n][3], h_xyz = double[F][nh][3] (the
 * hydrogens in the topology's h_off order).  Only these cross PCIe (12 bytes per atom and 24 per hydrogen of each
 * model).  On the device the F copies of the topology are expanded (atom f n + i is atom i of model f; residues, bonds,
 * hydrogens, rings and amides likewise), and each model gets the geometric part of initialize() with the arithmetic of
 * arp_ring_geometry / arp_amide_geometry / arp_ring_residues: ring centres and normals (I:1697-1733), amide centres and
 * normals (I:1531-1589) and the ring residues on the all-atom grid of its own model (I:1453-1492).  The expanded
 * structure is validated as an arp_set_blob upload is; a failure (ARP_E_ARG: a non-finite coordinate, ...) leaves NO
 * structure resident and keeps the topology, so a corrected call can follow.  A pass then evaluates every model; each
 * model's bags are bit-identical to its own single-structure run, and in their canonical order the records of model f
 * are contiguous and follow those of model f - 1 (ids of model f: atoms [f n, (f + 1) n), rings [f nring, ..), amides
 * [f namide, ..)).  Selections: one mask over the F n atoms.  Call again with any F to stream further coordinate sets
 * (trajectory chunks); a blob, a setter or arp_set_batch ends model mode.
 * Both return ARP_E_ARG on a shard (arp_set_ownership, arp_shard_assemble); arp_set_models also without a topology, and
 * when F n, F nbond or 3 F nh reach 2^31.
 *
 * arp_models_planes: what arp_set_models computed for the resident models, model after model: ring_center /
 * ring_normal double[3 * F * nring], ring_res int32[F * nring] (residue of the MODEL, -1 = none), amide_center /
 * amide_normal float[3 * F * namide].  ARP_E_ARG when no models are resident. */
int arp_set_topology(arp_ctx* ctx, const void* blob, uint64_t bytes, const int32_t* ring_off, const int32_t* ring_idx,
                     const int32_t* amide_atoms);
int arp_set_models(arp_ctx* ctx, int64_t nmodel, const float* xyz, const double* h_xyz);
int arp_models_planes(arp_ctx* ctx, double* ring_center, double* ring_normal, int32_t* ring_res, float* amide_center,
                      float* amide_normal);
/* Contact persistence over the resident models: ONE table over the topology instead of F bags.  After a pass over F
 * models (arp_set_models, then any launch that fills the atom-atom bag) the records of all models are regrouped on the
 * device into one row per distinct topology pair (a, b), a < b, rows in ascending (a, b):
 *   a, b                int32     topology atom ids
 *   n_models            uint16    models in which the pair has a record
 *   first, last         int32     lowest / highest 0-based model index with a record
 *   dist_min, dist_max  float32   over those models, the records' own float32 distances
 *   dist_sum            float64   those distances widened to float64 and added one by one in ascending model order,
 *                                 starting from 0.0 (defined to the bit; the mean is dist_sum / n_models)
 *   bit_count           uint16[ARP_PERSIST_BITS]  for SIFt bit k (ARP_S_CLASH ... ARP_S_WEAK_POLAR): models whose record has it
 *   ctype_mask          uint8     OR of 1 << ARP_CT_* over the models
 * Only the table crosses PCIe; the per-model bags stay what they were (arp_fetch_packed / arp_atom_contacts_fetch return
 * the same before, after and without these calls, in either layout, with arp_set_sort_after_pass on or off).
 *
 * arp_models_persistence_launch: enqueues the reduction on the context's stream and waits once, for *count = rows.  The
 * table is a result of the last launch and is voided with it (a new structure, models, selection or launch).  A second
 * call on the same results does nothing and returns the same count.  ARP_E_ARG: no models resident, no results of a
 * pass, more than 65 535 models (the uint16 columns), a shard.
 *
 * arp_models_persistence_fetch: the table with one device-to-host copy; any column pointer may be NULL; bit_count =
 * uint16[cap][ARP_PERSIST_BITS].  ARP_E_CAPACITY with *count = rows when cap is too small; ARP_E_ARG without a launch.
 *
 * ARP_PERSIST_STAGE_MAX: records of one bgn atom (over all models) that the reduction can stage on chip before it takes
 * a general path; 0 = the implementation has no such stage and no such limit (every atom takes the one path). */
#define ARP_PERSIST_BITS 15
#define ARP_PERSIST_STAGE_MAX 0
int arp_models_persistence_launch(arp_ctx* ctx, int64_t* count);
int arp_models_persistence_fetch(arp_ctx* ctx, int64_t cap, int32_t* a, int32_t* b, uint16_t* n_models, int32_t* first,
                                 int32_t* last, float* dist_min, float* dist_max, double* dist_sum,
                                 uint16_t* bit_count /* [cap][15] */, uint8_t* ctype_mask, int64_t* count);
/* Residue-residue contact table of the last pass: the records of all five bags folded by residue ON THE DEVICE, so that only
 * the table crosses PCIe.  It is made after a COMPLETE pass (arp_run_launch, arp_run_wait or the last arp_run_stage: all
 * five bags valid; the five launched one by one since the last input change count as one) from the bags as the pass left them.  Each record contributes the residues of its two partners:
 *   atom-atom (i, j)            res_id[i],        res_id[j]
 *   atom-plane (atom, ring)     res_id[atom],     ring_res[ring]
 *   plane-plane (bgn, end)      ring_res[bgn],    ring_res[end]
 *   group-group (bgn, end)      amide_res[bgn],   amide_res[end]
 *   group-plane (amide, ring)   amide_res[amide], ring_res[ring]
 * as the unordered pair res_a = min, res_b = max (bgn < end of a record says nothing about the order of the residues).  A
 * record with a residue of -1 (a ring or amide without one) is left out.  Atom-atom records never have res_a == res_b (the
 * reference skips intra-residue pairs, I:729); records of the other four bags can.  One row per distinct (res_a, res_b) with
 * at least one record, rows in ascending (res_a, res_b):
 *   res_a, res_b   int32      resident residue indices, res_a <= res_b (several structures or models resident: the indices of
 *                             the concatenation, so the table of each is a contiguous range of rows by res_a)
 *   n_contacts     uint32     atom-atom records of the pair
 *   dist_min       float32    smallest atom-atom distance of the pair, the bag's own float32; +inf when n_contacts == 0
 *   bit_count      uint32[ARP_RESPAIR_BITS]  atom-atom records with SIFt bit k (ARP_S_CLASH ... ARP_S_WEAK_POLAR)
 *   ctype_mask     uint8      OR of 1 << ARP_CT_* over the atom-atom records
 *   plane_count    uint32[4]  records of the atom-plane, plane-plane, group-group and group-plane bags, in that order
 * Every column is a count, a minimum or an OR: the table is a function of the bags as sets of records, whatever order the pass
 * wrote them in.  The bags stay what they were: arp_fetch_packed and the *_fetch calls return the same before, after and
 * without these calls, in either layout (arp_set_packed_layout), sorted or not (arp_set_sort_after_pass,
 * arp_atom_contacts_sort).
 *
 * arp_residue_pairs_launch: enqueues the reduction on the context's stream and waits once, for *count = rows.  The table is
 * a result of the last pass and is voided with it: by every input change and by the next launch that fills any bag.  A second
 * call on the same results launches nothing and returns the same count.  No record at all: 0 rows, ARP_OK.  ARP_E_ARG without
 * the results of a complete pass (arp_atom_contacts_launch alone is none) and on a shard of a distributed structure;
 * ARP_E_CAPACITY when the five bags together hold 2^31 records or more.
 *
 * arp_residue_pairs_fetch: the table with one device-to-host copy of one piece (its columns on 256-byte boundaries, through a
 * page-locked stage); any column pointer may be NULL; bit_count = uint32[cap][ARP_RESPAIR_BITS], plane_count =
 * uint32[cap][4].  ARP_E_CAPACITY with *count = rows when cap is too small; ARP_E_ARG without a launch. */
#define ARP_RESPAIR_BITS 15
int arp_residue_pairs_launch(arp_ctx* ctx, int64_t* count);
int arp_residue_pairs_fetch(arp_ctx* ctx, int64_t cap, int32_t* res_a, int32_t* res_b, uint32_t* n_contacts,
                            float* dist_min, uint32_t* bit_count /* [cap][15] */, uint8_t* ctype_mask,
                            uint32_t* plane_count /* [cap][4] */, int64_t* count);
/* Residue contact persistence over the resident models: the product of the two tables above — per pair of TOPOLOGY residues, in
 * how many models they touch, through which record classes, and how closely.  It is made after a COMPLETE pass over F
 * resident models (arp_set_models; all five bags valid, the condition of arp_residue_pairs_launch) from the bags as the pass
 * left them, never from the sorted slab.  A record contributes the residues of its two partners exactly as above (res_id of
 * an atom, ring_res of a ring, amide_res of an amide): resident indices.  With nres_t = nres / F the record's model is
 * f = res / nres_t (both partners lie in the same model), and the topology pair is res_a = min - f nres_t,
 * res_b = max - f nres_t.  A record with a residue of -1 is left out.  One row per distinct (res_a, res_b) with at least one
 * kept record in at least one model, rows in ascending (res_a, res_b):
 *   res_a, res_b   int32      topology residue indices, res_a <= res_b (equal only through ring / amide records)
 *   n_models       uint16     models with at least one kept record of the pair, in any bag
 *   first, last    int32      lowest / highest 0-based model index among those
 *   n_contacts     uint32     atom-atom records of the pair over all models
 *   class_models   uint16[5]  models with at least one record of class m: 0 atom-atom, 1 atom-plane, 2 plane-plane,
 *                             3 group-group, 4 group-plane
 *   bit_models     uint16[ARP_RESPERSIST_BITS]  for SIFt bit k (ARP_S_CLASH ... ARP_S_WEAK_POLAR): models in which at least
 *                             one atom-atom record of the pair has it
 *   dist_min       float32    smallest atom-atom distance over all models, the bag's own float32; +inf when
 *                             class_models[0] == 0
 *   dist_max       float32    largest of the PER-MODEL smallest atom-atom distances; -inf when class_models[0] == 0
 *   dist_sum       float64    the per-model smallest distances (models with an atom-atom record only) widened to float64 and
 *                             added one by one in ascending model order, starting from 0.0 (defined to the bit; the mean
 *                             closest approach is dist_sum / class_models[0])
 *   ctype_mask     uint8      OR of 1 << ARP_CT_* over the atom-atom records
 * Every per-model quantity is an OR, a minimum or a presence, so the order in which the pass wrote a model's records cannot
 * show; the one ordered operation is the sum over the models, and its order is fixed.  The bags, the persistence table and the
 * residue-pair table stay what they were: each returns the same before, after and without these calls, in either layout
 * (arp_set_packed_layout), with arp_set_sort_after_pass on or off.  The three tables share their scratch and none needs it
 * once made: making one voids no other.
 *
 * arp_models_residue_persistence_launch: enqueues the reduction on the context's stream and waits once, for *count = rows.
 * The table is a result of the last pass and is voided with it, wherever the residue-pair table is: by every input change
 * and by the next launch that fills any bag.  A second call on the same results launches nothing and returns the same
 * count.  No record at all: 0 rows, ARP_OK.  ARP_E_ARG: no models resident, no results of a complete pass, more than 65 535
 * models (the uint16 columns), a shard.  ARP_E_CAPACITY: the five bags together hold 2^31 records or more, or
 * (residue, residue, model) does not fit a 63-bit key.
 *
 * arp_models_residue_persistence_fetch: the table with one device-to-host copy of one piece (its columns on 256-byte
 * boundaries, in the order of the arguments, through a page-locked stage); any column pointer may be NULL; class_models =
 * uint16[cap][5], bit_models = uint16[cap][ARP_RESPERSIST_BITS].  ARP_E_CAPACITY with *count = rows when cap is too small;
 * ARP_E_ARG without a launch. */
#define ARP_RESPERSIST_BITS 15
int arp_models_residue_persistence_launch(arp_ctx* ctx, int64_t* count);
int arp_models_residue_persistence_fetch(arp_ctx* ctx, int64_t cap, int32_t* res_a, int32_t* res_b, uint16_t* n_models,
                                         int32_t* first, int32_t* last, uint32_t* n_contacts,
                                         uint16_t* class_models /* [cap][5] */, uint16_t* bit_models /* [cap][15] */,
                                         float* dist_min, float* dist_max, double* dist_sum, uint8_t* ctype_mask,
                                         int64_t* count);
/* ---- only the atom-atom records a caller asks for: the bag filtered on the device, then sorted and fetched ------------------
 * A record is kept when (sift & sift_any) != 0 && ((1u << ctype) & ctype_mask) != 0: at least one of the named SIFt bits
 * (ARP_S_*) and a contact type among the named ones (bit ARP_CT_* of ctype_mask).  Only the low 15 bits of sift_any and the
 * low 7 bits of ctype_mask may be set, and neither mask may be 0 (it would keep nothing): ARP_E_ARG otherwise.  There is no
 * distance term (a smaller cutoff is another pass) and no "none of these bits" term; the five ladder bits (clash, covalent,
 * vdw_clash, vdw, proximal) exclude each other, so "not bare proximity" is sift_any = ARP_FILTER_SIFT_ALL & ~ARP_S_PROXIMAL.
 *
 * arp_contacts_filter_launch: filters the bag of the last launch as the pass left it (never the sorted slab), waits once for
 * *kept = k', the kept records, and enqueues their canonical sort — over k' records only — into a slab of the filtered
 * result's own, in the layout arp_set_packed_layout names at this moment.  The result is byte for byte what masking the
 * columns of arp_fetch_packed with the predicate gives (the (i, j) key of a record is unique: the sort alone fixes the
 * order); in the ROWS layout row[] are the N + 1 offsets into the kept records (all zeros when none is kept).  It needs
 * atom-atom results (ARP_E_ARG without), is refused on a shard (ARP_E_ARG, like the device-reduced tables), and returns
 * ARP_E_CAPACITY for a bag of 2^31 records or more.  No record in the bag, or none kept: *kept = 0, nothing is launched.
 * A second call with the same masks and layout on the same results returns the stored count without work; other masks
 * re-make the result.  It is voided by every input change, by the next launch that fills the atom-atom bag or any ring /
 * amide bag (the bags packed behind it are sized here), and by a change of arp_set_packed_layout.  The unfiltered results
 * are neither read nor written: arp_fetch_packed, arp_atom_contacts_fetch, arp_atom_contacts_sort and the tables return the
 * same before, after and without these calls, with arp_set_sort_after_pass on or off.  With a batch or models resident the
 * ids are those of the concatenation and a structure's kept records stay one contiguous range in canonical order.
 *
 * arp_fetch_packed_filtered: arp_fetch_packed's contract in every respect — one copy, the meaning of counts and offsets, the
 * four ring / amide bags complete and in canonical order behind the atom-atom columns, ARP_E_CAPACITY with bytes_used set
 * before anything is launched — except that the atom-atom bag is the kept records: counts[0] = k'.  ARP_E_ARG without a
 * valid filtered result. */
#define ARP_FILTER_SIFT_ALL  0x7FFFu
#define ARP_FILTER_CTYPE_ALL 0x7Fu
int arp_contacts_filter_launch(arp_ctx* ctx, uint32_t sift_any, uint32_t ctype_mask, int64_t* kept);
int arp_fetch_packed_filtered(arp_ctx* ctx, void* host, uint64_t host_bytes, int64_t counts[5],
                              uint64_t offsets[ARP_PACKED_OFFSETS], uint64_t* bytes_used);
/* ---- water-mediated contacts: the atom-atom bag joined with itself on its water atoms, on the device ---------------------
 * The reference marks water contacts — the water branches of __get_contact_type (I:643-691: SELECTION_WATER,
 * NON_SELECTION_WATER, WATER_WATER) and the *_water_only hbond / polar counters per atom (I:821-852) — but never says what a
 * water sits BETWEEN.  This table does: which two atoms share a water.  It is an extension beside the mirror.
 *
 * Inputs: the atom-atom bag of the last pass as the pass left it, the per-atom flags (ARP_F_WATER) and res_id.
 *   leg      a record (i, j) with exactly one of i, j flagged ARP_F_WATER and (sift & sift_any) != 0.  The water atom is w, the
 *            other atom the partner.  Water-water records and records without a water are no legs: first-order bridges only.
 *   bridge   for every water w and every unordered pair a < b (resident atom ids) of its partners one row (w, a, b) — dropped
 *            when res_id[a] == res_id[b], unless flags has ARP_WB_SAME_RESIDUE.
 * Columns, in the order of the fetch's arguments:
 *   water, a, b        int32    resident atom ids
 *   dist_a, dist_b     float32  the bits of the distances of the records (w, a) and (w, b)
 *   sift_a, sift_b     uint16   the whole SIFt of each leg, not masked with sift_any
 *   ctype_a, ctype_b   uint8    each leg's ARP_CT_* code
 * A ligand-water-protein bridge is a row with one ARP_CT_SELECTION_WATER leg and one ARP_CT_NON_SELECTION_WATER leg.
 * Rows ascend by (water, a, b).  The (i, j) key of a record is unique, so a water's partners are distinct: the rows are
 * unique and the order is total.  Only the low 15 bits of sift_any may be set and it may not be 0; flags may hold
 * ARP_WB_SAME_RESIDUE only (ARP_E_ARG otherwise).  With a batch or models resident nothing changes: ids are resident ids, a
 * water only meets atoms of its own structure or model, and the rows of one structure or model are one contiguous range.
 *
 * arp_water_bridges_launch: makes the table on the context's stream from the bag as the pass left it (never the sorted slab)
 * and waits twice: for the number of legs, and for *count = rows.  It needs atom-atom results of a finished pass (ARP_E_ARG
 * without) and is refused on a shard of a distributed structure (ARP_E_ARG).  ARP_E_CAPACITY for a bag of 2^31 records or
 * more and for 2^31 rows or more (*count = rows).  No record or no leg: *count = 0 and nothing more is launched.  A second
 * call with the same sift_any and flags on the same results returns the stored count without work; other arguments remake
 * the table.  It is voided by every input change and by the next launch that fills the atom-atom bag.  The bags, their sorted
 * slab, the filtered bag and the three tables above are neither read nor written: every fetch returns the same before,
 * after and without these calls.
 *
 * arp_water_bridges_fetch: the table with one device-to-host copy of one piece (its columns on 256-byte boundaries, through
 * a page-locked stage); any column pointer may be NULL and is skipped.  ARP_E_CAPACITY with *count = rows when cap is too
 * small; ARP_E_ARG without a launch.  A table of 0 rows copies nothing. */
#define ARP_WB_SAME_RESIDUE (1u << 0)   /* keep the pairs of partners that share a residue */
int arp_water_bridges_launch(arp_ctx* ctx, uint32_t sift_any, uint32_t flags, int64_t* count);
int arp_water_bridges_fetch(arp_ctx* ctx, int64_t cap, int32_t* water, int32_t* a, int32_t* b, float* dist_a, float* dist_b,
                            uint16_t* sift_a, uint16_t* sift_b, uint8_t* ctype_a, uint8_t* ctype_b, int64_t* count);
/* Water-bridge persistence over the resident models: the bridge table above folded over the F resident models
 * (arp_set_models) — per pair of TOPOLOGY atoms, or of topology residues with ARP_WBP_BY_RESIDUE, that share a water in at
 * least one model: in how many models, through how many waters, with which SIFt bits on either leg, and how tight the bridge
 * is.  It is an extension beside the mirror, and its size does not depend on F.
 *
 * Input: the bridge table of arp_water_bridges_launch(ctx, sift_any, flags & ARP_WB_SAME_RESIDUE).  The launch makes that
 * table itself through that entry point (no work when the same table is resident), and afterwards it is resident and
 * fetchable exactly as if the caller had launched it.  flags may hold ARP_WB_SAME_RESIDUE and ARP_WBP_BY_RESIDUE only.
 *
 * What a bridge row (w, a, b) with resident ids contributes, with n topology atoms and nres_t = nres / F: its model is
 * f = w / n (a and b lie in the same model).  At atom level the pair is (a - f n, b - f n), already ascending, and leg "a" is
 * the row's leg a.  At residue level the pair is res_a = min, res_b = max of the two partners' topology residues
 * res_id[.] - f nres_t (as arp_models_residue_persistence defines them); leg "a" is the leg whose partner lies in res_a, and
 * the row's own leg a when the residues are equal (possible under ARP_WB_SAME_RESIDUE only).  The row's path is
 * dist_a + dist_b as ONE float32 addition (it commutes: the leg order cannot show).
 *
 * One row per distinct pair, rows ascending by the pair.  Columns, in the order of the fetch's arguments:
 *   a, b           int32      topology atom ids, a < b — or, at residue level, topology residue ids res_a <= res_b
 *   n_models       uint16     models with at least one bridge row of the pair
 *   first, last    int32      lowest / highest 0-based model index among those
 *   n_waters       uint32     sum over the models of the DISTINCT waters that bridge the pair in that model
 *   n_bridges      uint32     bridge rows of the pair over all models (atom level: equals n_waters)
 *   dist_min       float32    smallest path over all rows
 *   dist_max       float32    largest of the PER-MODEL smallest paths
 *   dist_sum       float64    the per-model smallest paths widened to float64 and added one by one in ascending model order,
 *                             starting from 0.0 (defined to the bit; the mean is dist_sum / n_models)
 *   bit_models_a, bit_models_b  uint16[ARP_WBP_BITS] each  for SIFt bit k (ARP_S_CLASH ... ARP_S_WEAK_POLAR): models in which
 *                             at least one row's leg a (b) has it — the whole SIFt of the leg, not masked with sift_any
 *   ctype_mask_a, ctype_mask_b  uint8 each  OR of 1 << ARP_CT_* of leg a (b) over all rows
 * Every per-model quantity is a presence, a count of distinct waters, a minimum or an OR; the one ordered operation is the sum
 * over the models, and its order is fixed: the table is a function of the bridge table as a set of rows.
 *
 * arp_models_water_bridge_persistence_launch: enqueues the fold on the context's stream and waits for *count = rows, after
 * the two waits of the bridge launch where that runs.  ARP_E_ARG: no models resident, more than 65 535 models (the uint16
 * columns), a shard, no atom-atom results of a finished pass, a sift_any of 0 or with bits beyond the low 15, an unknown
 * flag.  ARP_E_CAPACITY: (pair, model) does not fit a 63-bit key.  Whatever arp_water_bridges_launch returns passes through
 * unchanged.  No bridge row: *count = 0, ARP_OK, and nothing more is launched.  A second call with the same arguments on the
 * same results returns the stored count without work; other arguments remake the table.  It is voided wherever the bridge
 * table is — by every input change and by the next launch that fills the atom-atom bag — and when the bridge table is
 * remade with other arguments.  It reads the bridge table alone and writes no bag, no sorted slab, no filtered bag and no
 * other table: every other fetch returns the same before, after and without these calls.
 *
 * arp_models_water_bridge_persistence_fetch: the table with one device-to-host copy of one piece (its columns on 256-byte
 * boundaries, in the order of the arguments, through a page-locked stage); any column pointer may be NULL and is skipped;
 * bit_models_a / bit_models_b = uint16[cap][ARP_WBP_BITS].  ARP_E_CAPACITY with *count = rows when cap is too small;
 * ARP_E_ARG without a launch.  A table of 0 rows copies nothing. */
#define ARP_WBP_BY_RESIDUE (1u << 1)   /* key the rows by topology residue pair instead of topology atom pair */
#define ARP_WBP_BITS 15
int arp_models_water_bridge_persistence_launch(arp_ctx* ctx, uint32_t sift_any, uint32_t flags, int64_t* count);
int arp_models_water_bridge_persistence_fetch(arp_ctx* ctx, int64_t cap, int32_t* a, int32_t* b, uint16_t* n_models,
                                              int32_t* first, int32_t* last, uint32_t* n_waters, uint32_t* n_bridges,
                                              float* dist_min, float* dist_max, double* dist_sum,
                                              uint16_t* bit_models_a /* [cap][15] */, uint16_t* bit_models_b /* [cap][15] */,
                                              uint8_t* ctype_mask_a, uint8_t* ctype_mask_b, int64_t* count);
/* Interaction-fingerprint similarity between the resident models: which of the F models (arp_set_models) share their
 * contacts.  The persistence tables above count, per row, the models that have it; this counts, per PAIR of models, the
 * features both have — the intersection matrix from which the Tanimoto similarity, a clustering or a medoid follow on the
 * host.  It is an extension beside the mirror; the result is F x F integers whatever the structure size.
 *
 * Rows.  At atom level a row is a distinct topology atom pair (a, b) of the atom-atom bag: exactly the rows of
 *   arp_models_persistence.  With ARP_SIM_BY_RESIDUE a row is a distinct topology residue pair over the five bags: exactly
 *   the rows of arp_models_residue_persistence — a record with a residue of -1 is left out, and a complete pass is needed.
 * Planes.  ARP_SIM_PLANES = 20.  Plane q < 15: "an atom-atom record with SIFt bit q" (ARP_S_CLASH ... ARP_S_WEAK_POLAR).
 *   Plane 15 + m: "a record of class m" — 0 atom-atom, 1 atom-plane, 2 plane-plane, 3 group-group, 4 group-plane.  At atom
 *   level only the planes 0 ... 15 exist.
 * Participation.  An atom-atom record takes part only when bit `ctype` of ctype_mask is set (the contact-type half of
 *   arp_contacts_filter_launch's predicate); ring and amide records always take part.
 * Features.  Feature (row r, plane q) is present in model f when q is in `planes` and at least one participating record of
 *   row r in model f has plane q.
 * Result.  inter[f][g], uint32: the features present in both f and g.  The matrix is symmetric, inter[f][f] is the feature
 *   count of model f, and a model without records has a zero row and column.  Everything is a presence and a count: no float
 *   exists on the device, and the order of the records cannot show.
 *
 * arp_models_similarity_launch: enqueues the work on the context's stream and waits once, for *n_rows = rows (U);
 * *n_models = F.  ARP_E_ARG: a shard, no models resident, no results of a finished pass (atom level) or of a complete pass
 * (residue level), planes == 0 or with bits beyond the 20, bits 16 ... 19 at atom level, a ctype_mask of 0 or beyond
 * ARP_FILTER_CTYPE_ALL, an unknown flag.  ARP_E_CAPACITY: F > ARP_SIM_MAX_MODELS, (pair, model) does not fit a 63-bit key,
 * 2^31 records or more, popcount(planes) x U >= 2^32 (a count would not fit uint32), a bit matrix of 4 GiB or more
 * (F x popcount(planes) x ceil(U / 64) x 8 B).  No record at all: an all-zero matrix and ARP_OK.  A second call with the
 * same arguments on the same results returns without work; other arguments remake the matrix.  It is voided wherever the
 * persistence table (atom level) or the residue persistence table (residue level) is: by every input change and by the next
 * launch that refills a bag it reads.  It reads the bags as the pass left them and writes no bag, no sorted slab, no filtered
 * bag and no table: every other fetch returns the same before, after and without these calls, and no other call voids it.
 *
 * arp_models_similarity_fetch: the matrix with one device-to-host copy through the page-locked stage.  ARP_E_CAPACITY with
 * *n_models = F when cap_models < F; ARP_E_ARG without a launch.
 *
 * arp_models_similarity_info: what the last launch did — info[0] = rows U, info[1] = 64-bit words of the bit matrix per
 * model, info[2] = word slices of the product's grid (more than one: partial sums met by integer atomic adds), info[3] =
 * launches of this context that did work (one that returned a resident matrix does not count).  [0 ... 2] are 0 while no
 * matrix is resident. */
#define ARP_SIM_PLANES 20
#define ARP_SIM_MAX_MODELS 4096          /* F*F*4 B = 64 MiB result and page-locked stage */
#define ARP_SIM_BY_RESIDUE 1u
int arp_models_similarity_launch(arp_ctx* ctx, uint32_t planes, uint32_t ctype_mask, uint32_t flags,
                                 int64_t* n_models, int64_t* n_rows);
int arp_models_similarity_fetch(arp_ctx* ctx, int64_t cap_models, uint32_t* inter /* [F][F] */, int64_t* n_models);
int arp_models_similarity_info(arp_ctx* ctx, int64_t info[4]);
/* Contact coupling over the resident models: which contacts form and break TOGETHER — the salt bridge that opens whenever a
 * hydrogen bond across the pocket closes, the group of contacts that switches as one when a loop moves.  Similarity above is
 * B B^T over the models; this is B^T B over the contacts, and only the pairs of contacts that pass a threshold on their phi
 * coefficient leave the device.  It is an extension beside the mirror; every number is an integer.
 *
 * Rows.  Those of similarity: at atom level the distinct topology atom pairs (a, b) of the atom-atom bag (the rows of
 *   arp_models_persistence); with ARP_COUPLE_BY_RESIDUE the distinct topology residue pairs over the five bags (the rows of
 *   arp_models_residue_persistence) — a record with a residue of -1 is left out, and a complete pass is needed.
 * Presence.  Row r is present in model f when a participating record of r in f has a plane in `planes`, the 20-bit mask of
 *   similarity (at atom level only the planes 0 ... 15 exist); an atom-atom record takes part when bit `ctype` of ctype_mask
 *   is set, ring and amide records always.  The planes are not kept apart: a row is one contact, present or absent.
 *   n_r = the models with r present.
 * Features.  The rows with min_count <= n_r <= max_count, numbered 0 ... K - 1 in ascending row order, which is ascending
 *   (a, b).  The call requires 1 <= min_count <= max_count <= F - 1: a row of constant presence is never a feature, and the
 *   variance of a feature is never 0.
 * Pairs.  For features u < v let n11 = the models with both present and d = F n11 - n_u n_v (signed, 64 bits).  The pair
 *   is kept when
 *       1024 d^2 >= q n_u (F - n_u) n_v (F - n_v),    q = phi2_q in 1 ... 1024,
 *   that is when phi^2 >= q / 1024.  It is a comparison of integers — with F <= ARP_SIM_MAX_MODELS = 4096 both sides stay
 *   below 2^58 —, equality is kept, and an anti-correlated pair (d < 0) is kept like a correlated one.
 * Result.  Two tables:
 *   features   a, b int32 (topology atom ids, or residue ids), count uint32 (n_r)          K rows, ascending (a, b)
 *   pairs      u, v uint32 (feature numbers, u < v), n11 uint32                            P rows, ascending (u, v)
 *   The host derives phi, its sign and the Jaccard index from these integers.  Everything is exact and does not depend on
 *   the order of the records.
 * Capacity.  max_pairs is the most pairs the caller takes.  With more kept pairs the launch returns ARP_E_CAPACITY, writes
 *   the exact number into *n_pairs and leaves no result: raise phi2_q, narrow the band, or come back with that capacity.
 *   Zero kept pairs and K = 0 are valid, empty results.
 * Out of scope: the chunks of a trajectory streamed through arp_set_models cannot be merged — the threshold is not additive
 *   over chunks (a pair below it in every chunk may pass it over the whole) —, so one launch covers the resident models only.
 *
 * arp_models_coupling_launch: enqueues the work on the context's stream and waits three times, for the rows, for
 * *n_features = K and for *n_pairs = P.  ARP_E_ARG: a mask of 0 or with bits beyond its bits, an unknown flag, planes
 * 16 ... 19 at atom level, phi2_q outside 1 ... 1024, max_pairs < 0, a shard, no models resident, a band outside
 * 1 <= min_count <= max_count <= F - 1 (so F = 1 always), no results of a finished pass (atom level) or of a complete pass
 * (residue level).  ARP_E_CAPACITY: F > ARP_SIM_MAX_MODELS, (pair, model) does not fit a 63-bit key, 2^31 records or more, a
 * bit matrix of 4 GiB or more (U x ceil(F / 64) x 8 B), K > ARP_COUPLE_MAX_FEATURES (*n_features = K), more kept pairs than
 * max_pairs or 2^31 of them (*n_pairs = their number).  A second call with the same eight arguments on the same results
 * returns without work; other arguments remake the result.  It is voided wherever similarity of its level is: by every input
 * change and by the next launch that refills a bag it reads — the atom-atom bag, at residue level also the ring and amide
 * bags.  It reads the bags as the pass left them and writes no bag, no sorted slab, no filtered bag and no other result:
 * every other fetch returns the same before, after and without these calls, and no other derived result voids it.
 *
 * arp_models_coupling_fetch: both tables with one device-to-host copy through the page-locked stage; any column pointer may
 * be NULL.  ARP_E_CAPACITY with *n_features = K and *n_pairs = P when a cap is too small; ARP_E_ARG without a launch (or
 * after one that returned ARP_E_CAPACITY).  Empty tables copy nothing.
 *
 * arp_models_coupling_info: info[0] = rows U, info[1] = features K, info[2] = tile pairs of the product's grid (64 x 64
 * features a tile, upper triangle), info[3] = launches of this context that did work (one that returned a resident result
 * does not count).  [0 ... 2] are 0 while no result is resident. */
#define ARP_COUPLE_BY_RESIDUE 1u
#define ARP_COUPLE_MAX_FEATURES 65536    /* 1024 tiles a side: 524 800 tile pairs; feature numbers fit 16 + 16 key bits */
int arp_models_coupling_launch(arp_ctx* ctx, uint32_t planes, uint32_t ctype_mask, uint32_t flags, uint32_t min_count,
                               uint32_t max_count, uint32_t phi2_q, int64_t max_pairs, int64_t* n_features, int64_t* n_pairs);
int arp_models_coupling_fetch(arp_ctx* ctx, int64_t cap_features, int64_t cap_pairs, int32_t* a, int32_t* b, uint32_t* count,
                              uint32_t* u, uint32_t* v, uint32_t* n11, int64_t* n_features, int64_t* n_pairs);
int arp_models_coupling_info(arp_ctx* ctx, int64_t info[4]);
/* Contact lifetimes over the resident models: how LONG a contact lasts and how often it forms and breaks, where the
 * persistence table gives the fraction of models that have it.  The models are an ordered axis (for a trajectory streamed
 * through arp_set_models, model f is time).  It is an extension beside the mirror; every column is an integer.
 *
 * Participation.  A record of the atom-atom bag takes part when (sift & sift_any) != 0 and bit `ctype` of ctype_mask is set
 *   (arp_contacts_filter_launch's predicate).  With ARP_FILTER_SIFT_ALL and ARP_FILTER_CTYPE_ALL every record takes part.
 * Rows.  One row per topology pair (a, b), a < b, with at least one participating record, rows in ascending (a, b).
 * Intervals.  Let a pair's participating models be f1 < f2 < ... < fm.  An interval is a maximal stretch in which
 *   consecutive present models differ by at most gap + 1 (gap = models of absence tolerated inside an interval); its span is
 *   f_end - f_start + 1, so bridged holes count.
 *   a, b            int32    topology atom ids
 *   n_models        uint16   m
 *   first, last     int32    f1, fm
 *   n_intervals     uint16   number of intervals
 *   longest         uint16   the largest span
 *   longest_start   int32    first model of the interval with the largest span; on a tie, the earliest
 *   head, tail      uint16   span of the first and of the last interval (equal when n_intervals == 1): with them two chunk
 *                            tables of one trajectory merge exactly
 *   span_sum        uint32   sum of all spans (mean lifetime = span_sum / n_intervals)
 * With the all-records masks a, b, n_models, first and last are byte-equal to those columns of arp_models_persistence.
 *
 * arp_models_lifetimes_launch: enqueues the reduction on the context's stream and waits once, for *count = rows.
 * ARP_E_ARG: a shard, no models resident, more than 65 535 models, no results of a pass, a mask of 0 or with bits beyond
 * ARP_FILTER_SIFT_ALL / ARP_FILTER_CTYPE_ALL, gap > ARP_LIFETIMES_MAX_GAP.  ARP_E_CAPACITY: 2^31 records or more, (atom,
 * atom, model) does not fit a 63-bit key.  No participating record: 0 rows and ARP_OK.  A second call with the same three
 * arguments on the same results returns without work; other arguments remake the table.  It is voided wherever the
 * persistence table is (it reads the atom-atom bag alone); it writes no bag, no sorted slab, no filtered bag and no other
 * table, and no other derived result voids it.
 *
 * arp_models_lifetimes_fetch: the table with one device-to-host copy; any column pointer may be NULL.  ARP_E_CAPACITY with
 * *count = rows when cap is too small; ARP_E_ARG without a launch.
 *
 * arp_models_lifetimes_info: info[0] = rows of the resident table (0 while none is), info[1] = launches of this context that
 * did work (one that returned a resident table does not count). */
#define ARP_LIFETIMES_MAX_GAP 65534u
int arp_models_lifetimes_launch(arp_ctx* ctx, uint32_t gap, uint32_t sift_any, uint32_t ctype_mask, int64_t* count);
int arp_models_lifetimes_fetch(arp_ctx* ctx, int64_t cap, int32_t* a, int32_t* b, uint16_t* n_models, int32_t* first,
                               int32_t* last, uint16_t* n_intervals, uint16_t* longest, int32_t* longest_start,
                               uint16_t* head, uint16_t* tail, uint32_t* span_sum, int64_t* count);
int arp_models_lifetimes_info(arp_ctx* ctx, int64_t info[2]);
/* Interaction networks: the connected components of the contact graph, labelled on the device by a lock-free union-find
 * (csrc/arp_networks.h).  Which atoms form one hydrogen-bond network, waters included; how large the hydrophobic cluster is
 * that a ligand sits in; whether a salt bridge is isolated or part of an ionic cluster.  It is an extension beside the mirror.
 *
 * Inputs.  The atom-atom bag of the last pass with whatever is resident: one structure, a batch, or models.  sift_any: of the
 *   15 SIFt bits, not 0.  ctype_mask: of the 7 contact types, not 0.  flags: ARP_NET_BY_RESIDUE or 0.
 * Nodes.  The N = n resident atoms; with ARP_NET_BY_RESIDUE the N = nres resident residues, a record's nodes then being
 *   res_id[i], res_id[j].  The ring and amide bags take no part at either level.
 * Edges.  A record takes part when (sift & sift_any) != 0 and bit `ctype` of ctype_mask is set (arp_contacts_filter_launch's
 *   predicate).  A participating record is an edge between its two nodes.  A record with a negative node (a residue of -1) is
 *   left out.  A record whose two nodes are equal counts as an edge of that node and joins nothing (a pass produces none:
 *   no record joins two atoms of one residue).  No record joins two structures of a batch or two models, so no component spans them.
 * Results.
 *   label  int32 [N]   the smallest node id of the node's component, or -1 for a node without a participating record
 *   the component table, one row per component in ascending root:
 *   root      int32    the component's smallest node id
 *   n_nodes   int32    its nodes
 *   n_edges   int32    its participating records, multi-edges counted
 *   sift_or   uint16   OR of the whole SIFt of those records
 *   ctype_or  uint8    OR of 1 << ctype of those records
 * Everything is an integer, a minimum, a count or an OR: the result does not depend on the order of the records.
 *
 * arp_networks_launch: enqueues the union, the labels and the counts on the context's stream and waits once, for *count =
 * components.  ARP_E_ARG: a mask of 0 or with bits beyond ARP_FILTER_SIFT_ALL / ARP_FILTER_CTYPE_ALL, an unknown flag, a
 * shard, no atom-contact results of a pass.  ARP_E_CAPACITY: 2^31 records or more.  ARP_E_HIP "row count out of range": a
 * kernel met one of the bounds its loops cannot reach (arp_networks.h).  An empty bag or masks that no record meets: 0 rows,
 * every label -1, ARP_OK.  A second call with the same three arguments on the same results returns without work; other
 * arguments remake the result.  It is voided wherever the atom-atom bag is refilled or lost; it writes no bag, no sorted
 * slab, no filtered bag and no other table, and no other derived result voids it.
 *
 * arp_networks_fetch: the table with one device-to-host copy; any column pointer may be NULL.  ARP_E_CAPACITY with *count =
 * rows when cap is too small; ARP_E_ARG without a launch.
 *
 * arp_networks_labels_fetch: label[0 ... N) with one device-to-host copy, *nodes = N.  ARP_E_CAPACITY with *nodes = N when
 * cap < N; ARP_E_ARG without a launch.
 *
 * arp_networks_info: info[0] = rows of the resident table and info[1] = its nodes N (0 while none is resident), info[2] =
 * launches of this context that did work (one that returned a resident result does not count). */
#define ARP_NET_BY_RESIDUE 1u
int arp_networks_launch(arp_ctx* ctx, uint32_t sift_any, uint32_t ctype_mask, uint32_t flags, int64_t* count);
int arp_networks_fetch(arp_ctx* ctx, int64_t cap, int32_t* root, int32_t* n_nodes, int32_t* n_edges, uint16_t* sift_or,
                       uint8_t* ctype_or, int64_t* count);
int arp_networks_labels_fetch(arp_ctx* ctx, int64_t cap, int32_t* label, int64_t* nodes);
int arp_networks_info(arp_ctx* ctx, int64_t info[3]);
/* Ligand poses on the resident receptor: every pose's ligand - receptor contacts in one launch (csrc/arp_poses.h).  Docking and
 * virtual screening keep the receptor fixed and move the ligand thousands of times; what is wanted of each placement is its
 * interaction fingerprint.  The receptor is uploaded once; a pose is 12 bytes per ligand atom and 24 per ligand hydrogen.  It
 * is an extension beside the mirror.
 *
 * Contract.  ONE structure is resident (no batch, no models, no shard) with a selection uploaded by arp_set_selection: the
 *   MOVABLE SET, its S selected atoms in ascending packed order, 1 <= S <= ARP_POSES_MAX_ATOMS, S < n.  A pose is
 *   xyz    float32 [S][3]   coordinates of those atoms, in that order
 *   h_xyz  float64 [SH][3]  coordinates of the hydrogen rows (h_off order) whose parent atom is selected; SH is answered by
 *                           arp_poses_contacts_info after a launch and is a function of structure and selection
 *   and a launch takes n_poses of them, pose-major.  h_xyz may be NULL when SH = 0.
 * Result.  For pose p exactly the atom-atom records with one selected and one unselected atom that a pass would emit if it ran on
 *   the structure with those coordinates scattered in, with the same selection and the same (cutoff, vdw_comp,
 *   include_sequence_adjacent): the same i < j by packed id, the same float32 distance bits, the same 15-bit SIFt, the same
 *   contact type.  Records of two selected or two unselected atoms are not produced.  The records are in ascending (pose, i, j).
 *   Of a selected atom everything the decision reads is the pose's — its coordinate, its hydrogens, and the coordinate of its
 *   single-bond neighbour when that neighbour is selected too —; of an unselected atom everything is the resident structure's,
 *   except that ITS single-bond neighbour moves with the pose when that neighbour is selected (the uploaded neighbour index
 *   says which atom it is).  The covalent test is membership in the bond list at any distance; a pose may stretch bonds and
 *   X-H distances beyond any of the resident structure.
 *   summary  uint32 [n_poses][ARP_POSES_SUMMARY]  per pose: records with SIFt bit k (ARP_S_CLASH ... ARP_S_WEAK_POLAR) in slot
 *                           k < 15, all its records in slot 15 — enough to rank poses without copying a record
 *   pose_off uint64 [n_poses + 1]  the records of pose p are [pose_off[p], pose_off[p + 1])
 * Limits.  cutoff <= ARP_POSES_MAX_CUTOFF = 6.0: every accepted partner of a selected atom is then inside selection_plus
 *   whatever the pose (I:1420-1424), so no expansion is needed; beyond it membership would depend on the other ligand atoms.
 *   n < 2^21 and n_poses <= ARP_POSES_MAX_POSES a launch (the records are sorted by a 64-bit key of pose and two atom ids);
 *   callers chunk their poses.  Fewer than 2^31 records a launch.
 *   Not produced: atom-plane and plane-plane records of a pose (the ligand's own rings and amides), the per-atom accumulators.
 *
 * arp_poses_contacts_launch: uploads the poses, enqueues the work on the context's stream (arp_use_stream's, if set) and waits
 * for *count = records (and once per structure and selection for SH).  ARP_E_ARG with a message naming the cause: no
 * structure resident; a batch, models or shard ownership resident; no selection uploaded by arp_set_selection; a selection
 * of the whole structure; S or n_poses beyond the limits; cutoff > 6.0 or <= 0; single-bond neighbours given as coordinates
 * only (arp_set_single_bond_neighbour_coords); a pass enqueued and not waited for.  None of these touches a resident result.
 * A non-finite pose coordinate, found on the device: ARP_E_ARG and NO result — the result of the launch before is gone as
 * well, since a launch that has passed its argument checks voids it before it uploads.  A halogen-bond donor without a
 * single-bond neighbour: ARP_E_XBOND_NBR, as in a pass.  ARP_E_CAPACITY: 2^31 records or more, *count = their number.
 * The result is valid until an input of the structure or the selection changes (any setter, a new structure, models): the
 * fetch then refuses.  It reads no result bag and writing it voids nothing: the bags of the last pass and every table made
 * from them stay fetchable and byte-equal.  (It asks for the static columns in the cell order of `cutoff`, as a pass does.)
 *
 * arp_poses_contacts_fetch: copies what is asked for; ANY output pointer may be NULL (the summary alone: every record pointer
 * NULL, cap is then not looked at).  *count = records.  ARP_E_CAPACITY when a record column is asked for and cap < *count;
 * ARP_E_ARG without a valid result.
 *
 * arp_poses_contacts_info: info[0] = poses P, info[1] = S, info[2] = SH, info[3] = records of the resident result (all 0
 * while there is none). */
#define ARP_POSES_MAX_ATOMS 1024
#define ARP_POSES_MAX_POSES (1 << 20)
#define ARP_POSES_MAX_CUTOFF 6.0
#define ARP_POSES_SUMMARY 16
int arp_poses_contacts_launch(arp_ctx* ctx, int64_t n_poses, const float* xyz, const double* h_xyz, double cutoff,
                              double vdw_comp, int include_sequence_adjacent, int64_t* count);
int arp_poses_contacts_fetch(arp_ctx* ctx, int64_t cap, uint64_t* pose_off, int32_t* i, int32_t* j, float* dist, uint16_t* sift,
                             uint8_t* ctype, uint32_t* summary, int64_t* count);
int arp_poses_contacts_info(arp_ctx* ctx, int64_t info[4]);
/* Ligand poses on the resident receptor: the ring and amide contacts of every pose in one launch (csrc/arp_poses_planes.h).
 * The movable set and its preconditions are those of arp_poses_contacts_launch, without cutoff, hydrogen rows and single-bond
 * neighbours: none of the four ring / amide loops reads them.
 *
 * arp_set_plane_atoms: the atom paths of the resident rings (CSR ring_off [nring + 1] / ring_idx, ring-path order) and the
 *   atoms of the resident amides (amide_atoms [namide][4]: N, C, O, C-alpha), for the nring rings and namide amides that are
 *   resident.  Checked as arp_ring_geometry / arp_amide_geometry check theirs.  They are dropped with the structure, its rings
 *   or its amides, and uploading them voids the result below.
 *
 * The POSED structure of a pose is the resident one with the pose's coordinates scattered in, the geometry of its rings and
 * amides and its ring residues made again as initialize() makes them, and _make_selection with the same selection and the
 * 6.0 A expansion.  AFFECTED by a pose are: every movable atom; every amide whose N, C or O is movable; every ring with a
 * movable atom in its path or with a movable atom within 3.0 A (inclusive, float64 sum of squares) of its centre, at the atom's
 * pose coordinate or at its resident one.  The result holds exactly those records of the posed structure's four bags that
 * involve an affected entity, every column as the pass gives it; records between two unaffected entities are not reported.
 *
 * arp_poses_planes_launch: xyz float32 [n_poses][S][3].  counts[4] = records of the tables ARP_POSES_PLANES_ATOM_PLANE ...
 *   ARP_POSES_PLANES_GROUP_PLANE.  Nothing is truncated (a record buffer that was too small is grown to the counted size and the
 *   launch repeated once); the result is deterministic.  Refusals are ARP_E_ARG with the cause named: those of
 *   arp_poses_contacts_launch, "no plane atoms", "counts differ" (arp_set_plane_atoms), a non-finite pose coordinate (found on
 *   the device; no result is left), and the limits below by their names.  The result stays resident until an input, the
 *   selection or the plane atoms change; making it voids nothing else.
 *
 * arp_poses_planes_fetch: one table a call.  The id columns first / second are (atom, ring) for atom_plane, (bgn, end) for
 *   plane_plane and group_group, (amide, ring) for group_plane; records are in ascending pose, then in the canonical order of
 *   the bag: (ring, atom) for atom_plane, (first, second) for the others.  pose_off uint64 [n_poses + 1] are the table's offsets.  Value columns v0 ..: atom_plane
 *   dist, theta; plane_plane dist, dihedral, theta_bgn, theta_end; group_group dist, dihedral, theta (float32); group_plane
 *   dist, dihedral, theta (float64 unless said).  Byte columns u0 ..: atom_plane mask, ctype; plane_plane type1, type2, ctype;
 *   the others ctype.  ANY pointer may be NULL; a column the table does not have must be.  summary uint32
 *   [n_poses][ARP_POSES_PLANES_SUMMARY] per pose: slots 0-3 records per table, 4-8 INTER atom_plane records with
 *   ARP_AP_CARBONPI ... ARP_AP_METSULPHURPI, 9-11 INTER records of the other three tables, 12 affected rings, 13 those whose
 *   residue differs from the resident one, 14 those without a residue, 15 all records.
 *
 * arp_poses_planes_info: info[0] poses, [1] S, [2..5] records per table (0 without a result), [6] rings with a movable atom,
 *   [7] further rings affected at home, [8] moved amides, [9] plane atoms resident, [10] kernel launches so far, [11] 0. */
#define ARP_POSES_PLANES_SUMMARY 16
#define ARP_POSES_PLANES_MAX_RINGS 512     /* rings with a movable atom */
#define ARP_POSES_PLANES_MAX_HOME 512      /* further rings with a movable atom within 3 A at home */
#define ARP_POSES_PLANES_MAX_AMIDES 512    /* amides with a movable N, C or O */
#define ARP_POSES_PLANES_MAX_NEAR 256      /* further rings one pose brings within 3 A of a movable atom */
#define ARP_POSES_PLANES_ATOM_PLANE 0
#define ARP_POSES_PLANES_PLANE_PLANE 1
#define ARP_POSES_PLANES_GROUP_GROUP 2
#define ARP_POSES_PLANES_GROUP_PLANE 3
int arp_set_plane_atoms(arp_ctx* ctx, const int32_t* ring_off, const int32_t* ring_idx, const int32_t* amide_atoms);
int arp_poses_planes_launch(arp_ctx* ctx, int64_t n_poses, const float* xyz, int64_t counts[4]);
int arp_poses_planes_fetch(arp_ctx* ctx, int table, int64_t cap, uint64_t* pose_off, int32_t* first, int32_t* second, void* v0,
                           void* v1, void* v2, void* v3, uint8_t* u0, uint8_t* u1, uint8_t* u2, uint32_t* summary, int64_t* count);
int arp_poses_planes_info(arp_ctx* ctx, int64_t info[12]);
/* Pose fingerprints: the resident result of arp_poses_contacts_launch reduced on the device to interaction fingerprints and
 * their scores against reference poses (csrc/arp_poses_fingerprints.h).  Only small integers cross PCIe: no
 * record is copied.
 *
 * The first n_refs poses of the poses launch are the REFERENCES, 0 <= n_refs <= ARP_POSEFP_MAX_REFS and n_refs <= P.
 *   node      the receptor partner of a record: whichever of i / j is not in the movable set — that atom's packed id or, with
 *             ARP_POSEFP_BY_RESIDUE, its res_id.
 *   plane     q < ARP_POSEFP_PLANES = 15, "SIFt bit q" (ARP_S_CLASH ... ARP_S_WEAK_POLAR); `planes` is a non-zero mask of them,
 *             NP = popcount(planes).  The k-th selected plane is the k-th set bit of `planes`, ascending.
 *   A record PARTICIPATES when bit ctype of ctype_mask is set (the 7 contact types, as in arp_contacts_filter_launch) and
 *   sift & planes != 0.
 *   columns   the distinct nodes of the participating records of the whole launch, references included, ascending: ids[U].
 *   Feature (u, q) is PRESENT in pose p when a participating record of pose p has node ids[u] and SIFt bit q.
 *
 * Results (arp_poses_fingerprints_fetch; ANY pointer may be NULL):
 *   ids        int32  [U]                      the columns
 *   count      uint32 [P]                      features present in pose p
 *   cross      uint32 [P][n_refs]              features present in pose p and in reference q; the rows of the references
 *                                              themselves are included
 *   occupancy  uint32 [U][NP]                  poses p >= n_refs in which the feature is present: the references are not
 *                                              counted, so chunks that each carry the same references add up exactly
 *   bits       uint64 [P][NP][ceil(U / 64)]    the bit matrix: feature (u, k-th selected plane) is bit u & 63 of word u >> 6 of
 *                                              plane k (the layout of arp_models_similarity's matrix); padding bits are zero
 *   inter      uint32 [P][P]                   only with ARP_POSEFP_ALL_PAIRS (P <= ARP_SIM_MAX_MODELS): features present in pose
 *                                              f and in pose g; the diagonal is count
 * Everything is a presence or a count: no float exists on the device and the order of the records cannot show in a result.
 * The ring and amide records of the poses (arp_poses_planes_launch) take no part in this entry: they are the class planes of
 * arp_poses_fingerprints_planes_launch, below.
 *
 * arp_poses_fingerprints_launch: info[8] as arp_poses_fingerprints_info gives it.  One host wait (U, which sizes the matrix);
 *   every launch and copy goes on the context's stream.  A second launch with the same arguments on the same poses result
 *   returns without work (info[6], the launches that did work, stays); other arguments remake the result.  Refusals are
 *   ARP_E_ARG with the cause named, and none of them touches a resident result: no poses result; planes 0 or with bits beyond
 *   bit 14; ctype_mask 0 or with bits beyond the 7 types; an unknown flag; n_refs < 0, > ARP_POSEFP_MAX_REFS or > P; a pass
 *   enqueued and not waited for.  ARP_E_CAPACITY: ARP_POSEFP_ALL_PAIRS with P > ARP_SIM_MAX_MODELS = 4096 (nothing touched);
 *   NP * U >= 2^32; a bit matrix of 4 GiB or more (launch fewer poses) — the last two leave no fingerprint result.
 *   The result is void exactly when the poses result it was made from is void or replaced: a new arp_poses_contacts_launch,
 *   arp_set_selection, a new structure, models or a batch.  It reads no bag and voids nothing: the bags of the last pass, every
 *   table made from them and both poses results stay fetchable and byte-equal.
 *
 * arp_poses_fingerprints_fetch: *n_nodes = U.  ARP_E_CAPACITY when ids, occupancy or bits is asked for and cap_nodes < U;
 *   ARP_E_ARG without a valid result, and when inter is asked for of a launch without ARP_POSEFP_ALL_PAIRS.
 *
 * arp_poses_fingerprints_info: info[0] = P, [1] = n_refs, [2] = U, [3] = NP, [4] = words per pose W = NP * ceil(U / 64),
 *   [5] = word slices of the cross product (> 1: integer atomic adds into zeroed arrays), [6] = launches that did work,
 *   [7] = flags.  [0] ... [5] and [7] are 0 while there is no result.
 *
 * THE RING AND AMIDE CLASSES AS PLANES (arp_poses_fingerprints_planes_launch).  planes29 is a mask over
 * ARP_POSEFP_ALL_PLANES = 29 planes: the 15 SIFt bits and, behind them, 14 class planes fed by the four tables of the resident
 * poses-planes result (arp_poses_planes_launch).  An entity is on the LIGAND side when it is an atom of the movable set, a ring
 * with a movable atom in its path, or an amide whose N, C or O is movable; everything else — a receptor ring that a pose merely
 * comes near included — is on the receptor side.  A ring / amide record participates when bit ctype of ctype_mask is set,
 * EXACTLY ONE of its two entities is on the ligand side, and its plane is in the mask:
 *   plane 15 + b  atom_plane, bit b of mask (ARP_AP_*), the atom is the ligand's    node: the ring's residue
 *   plane 20 + b  atom_plane, bit b of mask, the ring is the ligand's               node: res_id[atom]
 *   plane 25      plane_plane (any class), one ring is the ligand's                 node: the other ring's residue
 *   plane 26      group_group, one amide is the ligand's                            node: am_res of the other amide
 *   plane 27      group_plane, the amide is the ligand's                            node: the ring's residue
 *   plane 28      group_plane, the ring is the ligand's                             node: am_res[amide]
 * THE RESIDUE OF A RECEPTOR RING is res_id of the first atom of its path (arp_set_plane_atoms): static, nothing per pose.  It
 * is deliberately not the posed ring_res — "the nearest atom within 3 A of the centre", which a ligand atom sitting on the
 * ring takes over, so that the feature would name the ligand's own residue (arp_residue_contacts keeps using ring_res).  A
 * node outside [0, nres) is skipped.  Class planes exist at residue level only.  ids[U] are the distinct nodes of all
 * participating records, atom-atom and ring / amide together; the plane axis is the set bits of planes29, ascending; count,
 * cross, occupancy, bits and inter mean what they mean above, over the widened feature set.
 *   Without a bit from 15 on, the entry is arp_poses_fingerprints_launch.  With one: both a poses result and a poses-planes
 *   result must be resident, with equal P and S and made from the same pose coordinates — both keep their uploaded poses, which
 *   are compared on the device as 32-bit words, the outcome read in the one wait for U.  ARP_E_ARG, cause named, resident
 *   results untouched: "no poses-planes result"; "differ in P or S"; "made from different poses" (no fingerprint result is
 *   left); class planes without ARP_POSEFP_BY_RESIDUE; planes29 0 or with bits beyond bit 28; the refusals above.
 *   ARP_E_CAPACITY as above.  The result is the one arp_poses_fingerprints_fetch / _info serve (info[3] = NP counts the class
 *   planes); a launch of either entry with other arguments remakes it.  One made with class planes is void when either source
 *   is: arp_poses_planes_launch and arp_set_plane_atoms void it too; one made without is not touched by those.  Making it
 *   voids nothing; everything goes on the context's stream. */
#define ARP_POSEFP_PLANES 15
#define ARP_POSEFP_ALL_PLANES 29
#define ARP_POSEFP_MAX_REFS 64
#define ARP_POSEFP_BY_RESIDUE 1u
#define ARP_POSEFP_ALL_PAIRS 2u
int arp_poses_fingerprints_launch(arp_ctx* ctx, uint32_t planes, uint32_t ctype_mask, uint32_t flags, int64_t n_refs, int64_t info[8]);
int arp_poses_fingerprints_planes_launch(arp_ctx* ctx, uint32_t planes29, uint32_t ctype_mask, uint32_t flags, int64_t n_refs,
                                         int64_t info[8]);
int arp_poses_fingerprints_fetch(arp_ctx* ctx, int64_t cap_nodes, int32_t* ids, uint32_t* count, uint32_t* cross, uint32_t* occupancy,
                                 uint64_t* bits, uint32_t* inter, int64_t* n_nodes);
int arp_poses_fingerprints_info(arp_ctx* ctx, int64_t info[8]);
/* Pose shortlist: the poses of the resident result of arp_poses_contacts_launch ranked on the device, and only the chosen
 * poses' records — optionally filtered — compacted for the fetch (csrc/arp_poses_shortlist.h).
 *
 * SOURCE: the resident poses result, P poses; depending on the arguments also the resident poses-planes result and the
 *   resident fingerprint result.  Nothing of them is written.
 * RANKED POSES: skip <= p < P, 0 <= skip < P.  The leading `skip` poses are the references of a fingerprint launch and take no
 *   part.
 * SCORE: an int64 of one of three kinds.
 *   ARP_SHORTLIST_LIST      no score (0).  The chosen poses are the caller's pose_ids[n_ids] in the caller's order: each id in
 *                           [0, P), repeats allowed, 1 <= n_ids <= ARP_POSES_MAX_POSES.  skip, k and min_score must be 0, 0 and
 *                           INT64_MIN.
 *   ARP_SHORTLIST_SUMMARY   score[p] = sum_{s<16} w[s] summary[p][s] + sum_{s<16} w[16 + s] planes_summary[p][s], weights32 =
 *                           int32[32] with |w| <= ARP_SHORTLIST_MAX_WEIGHT = 2^24 (the sum fits 60 bits).  A non-zero weight in
 *                           the second half needs the poses-planes result of the SAME POSES (below).
 *   ARP_SHORTLIST_TANIMOTO  from the resident fingerprint result (either entry; n_refs >= 1; its P the source's).  For reference
 *                           q: t = cross[p][q], u = count[p] + count[q] - t, score_q = (u == 0) ? 2^32 : floor(t 2^32 / u) in
 *                           unsigned 64-bit arithmetic (t < 2^32: the product fits); 0 / 0 is 1.0.  ref in [0, n_refs) names
 *                           the reference, ref = -1 takes the largest score_q over all references.  The scores are taken at
 *                           launch: the shortlist does not read the fingerprint result afterwards.
 * ORDER: descending score, ties by ascending pose id.  The chosen poses are the first K = min(k, P - skip) of that order whose
 *   score is >= min_score, k >= 1; INT64_MIN: no threshold.  K = 0 is a valid, empty shortlist.
 * TABLES: a non-zero mask.  Bit 0: the atom-atom table; bits 1 ... 4: atom_plane, plane_plane, group_group, group_plane of the
 *   poses-planes result (SAME POSES).
 * RECORD FILTER: an atom-atom record is kept when bit ctype of ctype_mask is set (7 types, non-zero) and sift_mask == 0 or
 *   sift & sift_mask != 0 (15 bits); a ring / amide record when bit ctype of ctype_mask is set.  sift_mask = 0 with ctype_mask =
 *   ARP_FILTER_CTYPE_ALL keeps everything.
 * RESULT: pose int32 [K]; score int64 [K]; summary uint32 [K][16] and planes_summary uint32 [K][16], the source rows of the
 *   chosen poses, unfiltered (what the pose has, not what was kept); per requested table off uint64 [K + 1] and the table's
 *   columns: the records of chosen pose r are [off[r], off[r + 1]), the kept records of that pose in the order the source holds
 *   them, every column with the source's type and bits.  Nothing is truncated; the result is deterministic.
 * SAME POSES: wherever the poses-planes result is read (tables bits 1 ... 4, a non-zero weight 16 ... 31) it must have the
 *   source's P and S and must have been made from the same uploaded coordinates (compared on the device as 32-bit words, the
 *   outcome read in the launch's one wait).
 *
 * arp_poses_shortlist_launch: info[8] as arp_poses_shortlist_info gives it.  One host wait (K, the five totals, the same-poses
 *   flag, the device's error word); every launch and copy goes on the context's stream.  Refusals are ARP_E_ARG with the cause
 *   named, and none of them touches a resident result: no poses result; a pass not waited for; unknown kind; weights, pose_ids
 *   (or an id, or n_ids) or ref missing or out of range; skip or k out of range; tables 0 or beyond bit 4, sift_mask beyond 15
 *   bits, ctype_mask 0 or beyond 7 bits; ARP_SHORTLIST_LIST with skip / k / min_score set; ARP_SHORTLIST_TANIMOTO without a
 *   fingerprint result, with n_refs = 0 or with another P; "no poses-planes result"; "differ in P or S".  "Made from different
 *   poses" is ARP_E_ARG too, found on the device: no shortlist is left after it.  ARP_E_CAPACITY: a table of 2^31 records or
 *   more (no shortlist left).  Every successful launch remakes the result.
 *   The shortlist is void exactly when the poses result is void or replaced (a new arp_poses_contacts_launch,
 *   arp_set_selection, a new structure, models or a batch); one that read the poses-planes result also when that is
 *   (arp_poses_planes_launch, arp_set_plane_atoms).  Making it voids nothing: the bags of the last pass, every table made from
 *   them, both poses results and the fingerprint result stay fetchable and byte-equal.
 *
 * arp_poses_shortlist_fetch: the per-pose arrays and the atom-atom table; ANY pointer but n_chosen and count may be NULL.
 *   *n_chosen = K, *count = kept atom-atom records.  ARP_E_CAPACITY when a per-pose array (pose, score, summary, planes_summary,
 *   off) is asked for and cap_poses < K, or a record column is asked for and cap < *count.  ARP_E_ARG: no valid result; off or a
 *   record column of a launch without tables bit 0; planes_summary of a launch that did not read the poses-planes result.
 * arp_poses_shortlist_planes_fetch: one ring / amide table a call (ARP_POSES_PLANES_ATOM_PLANE ...), columns and their types as
 *   arp_poses_planes_fetch; *count = kept records of the table.  ARP_E_ARG for a table that was not requested and for a column
 *   the table does not have; ARP_E_CAPACITY as above.  Both fetches pass every piece through the page-locked stage in one wait.
 * arp_poses_shortlist_info: info[0] = K, [1] ... [5] = kept records of the five tables (0 for a table not requested), [6] =
 *   launches that did work so far, [7] = kind.  [0] ... [5] and [7] are 0 while there is no result. */
#define ARP_SHORTLIST_LIST 0
#define ARP_SHORTLIST_SUMMARY 1
#define ARP_SHORTLIST_TANIMOTO 2
#define ARP_SHORTLIST_TABLES 5
#define ARP_SHORTLIST_MAX_WEIGHT (1 << 24)
int arp_poses_shortlist_launch(arp_ctx* ctx, int kind, const int32_t* weights32, int64_t ref, const int32_t* pose_ids, int64_t n_ids,
                               int64_t skip, int64_t k, int64_t min_score, uint32_t tables, uint32_t sift_mask, uint32_t ctype_mask,
                               int64_t info[8]);
int arp_poses_shortlist_fetch(arp_ctx* ctx, int64_t cap_poses, int64_t cap, int32_t* pose, int64_t* score, uint32_t* summary,
                              uint32_t* planes_summary, uint64_t* off, int32_t* i, int32_t* j, float* dist, uint16_t* sift,
                              uint8_t* ctype, int64_t* n_chosen, int64_t* count);
int arp_poses_shortlist_planes_fetch(arp_ctx* ctx, int table, int64_t cap_poses, int64_t cap, uint64_t* off, int32_t* first,
                                     int32_t* second, void* v0, void* v1, void* v2, void* v3, uint8_t* u0, uint8_t* u1, uint8_t* u2,
                                     int64_t* count);
int arp_poses_shortlist_info(arp_ctx* ctx, int64_t info[8]);
/* Pose clusters: leader clustering (sphere exclusion in rank order) of the poses of the resident fingerprint result by the
 * Tanimoto similarity of their fingerprints, on the device (csrc/arp_poses_clusters.h).  No P x P matrix is made:
 * at most positions x clusters row products, so it works at ARP_POSES_MAX_POSES poses.
 *
 * SOURCE: the resident fingerprint result, from either entry, at any level and with any planes: P, U, NP, W = NP ceil(U / 64),
 *   bits [P][W] and count [P].  Nothing of it, or of any other resident result, is written.
 * POSITIONS: order == NULL: position m names pose skip + m, M = P - skip, 0 <= skip < P (the leading `skip` poses are references
 *   and take no part); n_order must be 0.  order != NULL: M = n_order, 1 <= M <= ARP_POSES_MAX_POSES, position m names pose
 *   order[m]; every id in [0, P), checked on the host before anything is touched; repeats allowed; skip must be 0.
 * SIMILARITY of poses a and b (the arithmetic of ARP_SHORTLIST_TANIMOTO): t = sum over the W words of popcount(bits[a][w] &
 *   bits[b][w]), u = count[a] + count[b] - t, q(a, b) = (u == 0) ? 2^32 : floor(t 2^32 / u) in unsigned 64-bit arithmetic
 *   (t < 2^32: the product fits); 0 / 0 is 1.0.  a and b are SIMILAR when q >= threshold_q32, 0 <= threshold_q32 <= 2^32.
 * CLUSTERING, defined sequentially: walk the positions m = 0 ... M - 1 and keep the list of leaders made so far.  A position
 *   whose pose is similar to some leader's pose joins the FIRST such leader in leader order (not the most similar one);
 *   otherwise, while fewer than max_clusters leaders exist (1 <= max_clusters <= ARP_POSECL_MAX_CLUSTERS), it becomes the next
 *   leader; otherwise it stays unassigned.  Position 0 is always leader 0.
 * RESULT: pose int32 [M], the pose of each position; cluster int32 [M], the index in leader order, -1 when unassigned;
 *   similarity int64 [M], q to its own leader's pose, 2^32 for a leader, -1 when unassigned; leader int32 [C], the leaders' pose
 *   ids; leader_position int32 [C], their positions, strictly ascending; size uint32 [C], the members per cluster, the leader
 *   included.  Sum of size + unassigned = M.  Everything is an integer: the result is a pure function of the arguments and the
 *   fingerprint result.  U = 0 (no feature in any pose) gives q = 2^32 everywhere: one cluster of M members.
 *
 * arp_poses_clusters_launch: info[8] as arp_poses_clusters_info gives it.  One launch per round, enqueued back to back on the
 *   context's stream, 64 at a time: after such a group one word (the next leader's position) is read back and the rounds end
 *   when no position is left; up to 64 rounds there is the one wait for C and the unassigned count.  Refusals are ARP_E_ARG with
 *   the cause named, and none of them touches a resident result: a pass not waited for; no poses result; no fingerprint result;
 *   the fingerprint's P is not the poses result's; threshold_q32 > 2^32; max_clusters outside [1, 4096]; skip out of range; an
 *   order with skip != 0; n_order out of range; an id outside [0, P); order == NULL with n_order != 0.  Every successful launch
 *   remakes the result.
 *   The launch reads the fingerprint result only while it runs: a later fingerprint launch with other arguments does not void
 *   the clusters.  They are void exactly when the poses result is void or replaced (a new arp_poses_contacts_launch,
 *   arp_set_selection, a new structure, models or a batch); when the fingerprint they were made from had class planes also when
 *   the poses-planes result is (arp_poses_planes_launch, arp_set_plane_atoms).  Making them voids nothing.
 * arp_poses_clusters_fetch: ANY pointer but n_positions and n_clusters may be NULL.  *n_positions = M, *n_clusters = C.
 *   ARP_E_CAPACITY when a per-position array (pose, cluster, similarity) is asked for and cap_positions < M, or a per-cluster
 *   array (leader, leader_position, size) and cap_clusters < C.  ARP_E_ARG: no valid result.  Every piece goes through the
 *   page-locked stage in one wait.
 * arp_poses_clusters_info: info[0] = M, [1] = C, [2] = unassigned, [3] = max_clusters, [4] = W, [5] = lanes per pose of the round
 *   kernel, [6] = launches that did work so far, [7] = threshold_q32.  All but [6] are 0 while there is no result. */
#define ARP_POSECL_MAX_CLUSTERS 4096
int arp_poses_clusters_launch(arp_ctx* ctx, const int32_t* order, int64_t n_order, int64_t skip, uint64_t threshold_q32,
                              int64_t max_clusters, int64_t info[8]);
int arp_poses_clusters_fetch(arp_ctx* ctx, int64_t cap_positions, int64_t cap_clusters, int32_t* pose, int32_t* cluster,
                             int64_t* similarity, int32_t* leader, int32_t* leader_position, uint32_t* size, int64_t* n_positions,
                             int64_t* n_clusters);
int arp_poses_clusters_info(arp_ctx* ctx, int64_t info[8]);
/* Ligand library: DIFFERENT ligands, each with its poses, on one resident receptor in one launch (csrc/arp_library.h, DESIGN.md
 * 5u).  The pose entries above move one ligand that is part of the resident structure; a screen runs thousands of different
 * molecules against one receptor.  Here the receptor is resident ALONE and the ligands' per-atom facts are a table beside it.
 * It is an extension beside the mirror.
 *
 * RECEPTOR.  ONE structure is resident (no batch, no models, no shard ownership: refused as the pose launches refuse them, in
 *   the same order), n < 2^21.  No selection is needed and none is read.
 * LIBRARY (arp_set_ligand_library).  L ligands, 1 <= L <= ARP_LIBRARY_MAX_LIGANDS; ligand l has S_l atoms, 1 <= S_l <=
 *   ARP_LIBRARY_MAX_ATOMS, library atoms atom_off[l] ... atom_off[l + 1] - 1 (atom_off int32 [L + 1], atom_off[0] = 0), TA =
 *   atom_off[L] atoms in all.  Per library atom: type_mask uint16 and flags uint16 (as arp_set_atoms takes them), vdw and cov
 *   float64, h_off int32 [TA + 1] (its hydrogen rows, CSR over all library atoms, h_off[0] = 0, not decreasing; SH_l = the
 *   rows of ligand l), sb_nbr int32 (the index WITHIN ITS LIGAND of the single-bond heavy neighbour, -1: none).
 *   ARP_E_ARG with the cause named, checked in this order and before anything is touched: a pass not waited for; L out of
 *   range; an array missing; atom_off not starting at 0; a ligand with fewer than 1 or more than ARP_LIBRARY_MAX_ATOMS atoms;
 *   h_off not starting at 0; h_off decreasing; a radius that is not finite or negative; an sb_nbr outside its own ligand or
 *   equal to its own atom.
 *   The library reads nothing of the receptor and STAYS RESIDENT through new structures, models and batches: the same library
 *   runs against several receptors.  arp_set_ligand_library replaces it and voids the library result.
 * WHAT A LIGAND IS.  One residue of a chain of its own: no polypeptide residue, no sequence neighbours, no bond to the receptor.
 *   Peptide ligands and covalent ligands are out of scope.
 * POSES (arp_library_contacts_launch).  pose_off int64 [L + 1], pose_off[0] = 0, not decreasing: ligand l has P_l =
 *   pose_off[l + 1] - pose_off[l] >= 0 poses, T = pose_off[L], 1 <= T <= ARP_POSES_MAX_POSES; pose_off[l] + p is the GLOBAL id
 *   of pose p of ligand l.  Both coordinate arrays are ligand-major, then pose-major: xyz float32, sum of P_l S_l 3 values;
 *   h_xyz float64, sum of P_l SH_l 3 values (may be NULL when that sum is 0).  The library cannot see their lengths: the
 *   caller answers for them.  cutoff in (0, ARP_POSES_MAX_CUTOFF], vdw_comp finite; include_sequence_adjacent is accepted and
 *   without effect (the gate needs a sequence on both residues; a ligand has none).
 * RESULT.  For global pose t of ligand l exactly the atom-atom records with one receptor and one ligand atom that a pass would
 *   emit on the COMPLEX — the receptor with ligand l appended after its last atom as one more residue, uploaded as ONE
 *   structure, the pose's coordinates scattered in, the ligand's atoms as the selection, the same parameters.  A record is
 *   (t, i, a): i the receptor's packed id, a the ligand atom's index within its ligand (in the complex that pair is i < j = n +
 *   a: bgn is always the receptor atom); the same float32 distance bits, 15-bit SIFt and contact type.  Ascending (t, i, a).
 *   pose_off uint64 [T + 1], i int32, a int32, dist float32, sift uint16, ctype uint8, summary uint32 [T][ARP_POSES_SUMMARY]
 *   with the slots of arp_poses_contacts_fetch's summary.  Nothing is truncated: a record buffer that was too small is grown to
 *   the counted size and the launch repeated.
 *   ARP_E_ARG with the cause named, in this order, none touching a resident result: the receptor's refusals; n >= 2^21; no
 *   library; pose_off missing, not starting at 0, decreasing; T out of range; cutoff; vdw_comp; xyz missing; h_xyz missing while
 *   a posed ligand has hydrogen rows.  A non-finite pose coordinate, found on the device: ARP_E_ARG and NO result (a launch
 *   that has passed its argument checks voids the result before it).  A halogen-bond donor without a single-bond neighbour:
 *   ARP_E_XBOND_NBR, as in a pass.  ARP_E_CAPACITY: 2^31 records or more.
 *   All work goes on the context's stream (arp_use_stream's, if set); ONE host wait a launch, for *count with the device's
 *   error word.
 * BEST POSE PER LIGAND (arp_library_best_launch / _fetch).  Reads the resident summary and nothing else.  weights int32
 *   [ARP_POSES_SUMMARY], |w| <= ARP_SHORTLIST_MAX_WEIGHT; score[t] = sum over the slots s of w[s] summary[t][s] in int64.  Per
 *   ligand: n_poses int64, best_pose int32 (the global pose id of the highest score, ties to the lower id), score int64.  A
 *   ligand without poses: -1 and INT64_MIN.  20 bytes per ligand instead of 64 per pose.  arp_library_best_fetch: any array may
 *   be NULL; ARP_E_CAPACITY when one is asked for and cap_ligands < *n_ligands = L.
 * STATE.  The library result is void after a new structure, models, a batch, arp_set_ligand_library and a new library launch,
 *   and the best-pose table goes with it (or is replaced by a new arp_library_best_launch).  arp_set_selection does NOT void it:
 *   it reads no selection.  Making it voids nothing: the bags of the last pass, every table made from them and all five pose
 *   results stay fetchable and byte-equal.
 * arp_library_contacts_fetch: as arp_poses_contacts_fetch (ANY pointer may be NULL; cap is looked at only when a record column
 *   is asked for).  arp_library_info: info[0] = L, [3] = TA, [4] = hydrogen rows, [6] = the largest S_l of the resident
 *   library; [1] = T, [2] = records, [5] = blocks of k_library_contacts (poses are taken with a grid stride) of the resident
 *   result; [7] = 1 while a best-pose table is resident.
 * OUT OF SCOPE: clusters over a library result (fingerprints: arp_library_fingerprints_launch below; the ligands' own rings and
 *   amides: arp_library_planes_launch below; the shortlist: arp_library_shortlist_launch below); peptide and covalent ligands;
 *   cutoffs beyond 6.0; a batch, models or a shard as the receptor; the per-atom accumulators. */
#define ARP_LIBRARY_MAX_LIGANDS (1 << 16)
#define ARP_LIBRARY_MAX_ATOMS 256
int arp_set_ligand_library(arp_ctx* ctx, int64_t n_ligands, const int32_t* atom_off, const uint16_t* type_mask, const uint16_t* flags,
                           const double* vdw, const double* cov, const int32_t* h_off, const int32_t* sb_nbr);
int arp_library_contacts_launch(arp_ctx* ctx, const int64_t* pose_off, const float* xyz, const double* h_xyz, double cutoff,
                                double vdw_comp, int include_sequence_adjacent, int64_t* count);
int arp_library_contacts_fetch(arp_ctx* ctx, int64_t cap, uint64_t* pose_off, int32_t* i, int32_t* a, float* dist, uint16_t* sift,
                               uint8_t* ctype, uint32_t* summary, int64_t* count);
int arp_library_info(arp_ctx* ctx, int64_t info[8]);
int arp_library_best_launch(arp_ctx* ctx, const int32_t* weights);
int arp_library_best_fetch(arp_ctx* ctx, int64_t cap_ligands, int64_t* n_poses, int32_t* best_pose, int64_t* score,
                           int64_t* n_ligands);
/* Library fingerprints: the resident library result reduced on the device to interaction fingerprints and scored against
 * reference interactions (csrc/arp_library_fingerprints.h).  An extension beside the mirror.
 *
 * FEATURE.  (node, plane).  The node is the receptor atom i of a participating library record, with ARP_POSEFP_BY_RESIDUE
 *   res_id[i]; the plane is one of the 15 SIFt bits selected by `planes`.  A record participates when bit ctype of ctype_mask
 *   is set and sift & planes != 0.  The ligand side a never names a node.  This entry has no class planes (the library's ring and
 *   amide tables enter through arp_library_fingerprints_planes_launch, below) and there is no all-pairs matrix (T reaches 2^20).
 * REFERENCES need not be poses of the launch: the known binder is usually another molecule.  Q = n_refs <=
 *   ARP_POSEFP_MAX_REFS references are given as feature lists: ref_off int64 [Q + 1] (ref_off[0] = 0, not decreasing, F =
 *   ref_off[Q] <= ARP_LIBFP_MAX_FEATURES), ref_node int32 [F] (nodes of the launch's level, strictly ascending within a
 *   reference), ref_planes uint32 [F] (plane masks BEFORE selection).  The device ANDs every mask with `planes`; a feature whose
 *   mask becomes 0 is dropped; a node that keeps a plane is a column EVEN IF NO POSE TOUCHES IT, so a reference's count is
 *   complete and the chunks of one screen carry identical reference rows.  All three may be NULL when Q = 0.
 * RESULT.  Q + T rows: row q < Q is reference q, row Q + t is global pose t of the resident library result.  The arrays are
 *   those of arp_poses_fingerprints_fetch with P = Q + T: ids int32 [U] ascending; count uint32 [Q + T]; cross uint32 [Q + T][Q];
 *   occupancy uint32 [U][NP], over the rows >= Q only; bits uint64 [Q + T][NP][ceil(U / 64)].  info[8] as
 *   arp_poses_fingerprints_info: rows (Q + T), Q, U, NP, words a row, word slices of the cross product, launches, flags
 *   (info[6] counts EVERY launch that passed its refusals: there is no "same arguments" shortcut — the references are the
 *   caller's arrays and comparing them costs what uploading them does).
 *   ARP_E_ARG with the cause named, in this order, none touching a resident result: a pass not waited for; no library result
 *   resident; planes 0 or beyond the 15 bits; ctype_mask 0 or beyond the 7 types; a flag other than ARP_POSEFP_BY_RESIDUE; by
 *   residue without residues resident; Q outside 0 ... ARP_POSEFP_MAX_REFS; a reference array NULL with Q > 0; ref_off not
 *   starting at 0, or decreasing; F > ARP_LIBFP_MAX_FEATURES; a node outside [0, N) (N = atoms, or residues); nodes not
 *   strictly ascending within a reference; a mask beyond the 15 bits.  Then, once U is known (the fingerprint before is void by
 *   then and none is resident afterwards), ARP_E_CAPACITY as arp_poses_fingerprints_launch with P = Q + T: NP U >= 2^32; a bit
 *   matrix of 4 GiB or more.
 *   All work goes on the context's stream; ONE host wait a launch, for U — the caller's reference arrays are free after it.
 * BEST POSE PER LIGAND (arp_library_fingerprints_best_launch / _fetch).  Reads count and cross of the resident fingerprint and
 *   the ligands' pose ranges.  For ligand l and reference q the global pose t of the highest Tanimoto in 32 fractional bits:
 *   with x = cross[Q + t][q] and u = count[Q + t] + count[q] - x it is floor(x 2^32 / u), and 2^32 where u = 0.  Ties go to the
 *   lower global pose.  n_poses int64 [L]; best_pose int32 [L][Q]; tanimoto_q32 int64 [L][Q]; shared uint32 [L][Q] (that x);
 *   count uint32 [L][Q] (the best pose's own feature count, so that recovery follows).  A ligand without poses: -1, -1, 0, 0.
 *   Refused (ARP_E_ARG) without a resident fingerprint and when that was made with Q = 0.  _fetch: any array may be NULL;
 *   ARP_E_CAPACITY when one is asked for and cap_ligands < *n_ligands = L; *n_refs = Q.
 * STATE.  The fingerprint is void wherever the library result is (a new structure, models, a batch, arp_set_ligand_library, a
 *   new library launch) and after a new fingerprint launch; its best-pose table goes with it.  arp_set_selection voids neither.
 *   Making either voids nothing else: the library result, its best-pose table and every pose result stay fetchable and
 *   byte-equal.
 * THE RING AND AMIDE CLASSES AS PLANES (arp_library_fingerprints_planes_launch).  planes29 is a mask over
 *   ARP_POSEFP_ALL_PLANES = 29 planes: the 15 SIFt bits and the 14 class planes of arp_poses_fingerprints_planes_launch, with
 *   its bit numbers and its table -> plane map, fed by the four tables of the resident library-planes result
 *   (arp_library_planes_launch) of the SAME poses.  Without a bit from ARP_POSEFP_PLANES on, the entry does exactly what
 *   arp_library_fingerprints_launch does (reference masks may still carry bits up to 28; the selection drops them).
 *   Ids in the library-planes result are the complex's.  An entity is on the LIGAND side when it is an atom with id >= n, a
 *   ring with id >= nring or an amide with id >= namide (n, nring, namide the receptor's); everything else is the receptor's,
 *   an affected receptor ring included.  A ring / amide record takes part when bit ctype of ctype_mask is set, EXACTLY ONE of
 *   its two entities is the ligand's (ligand - ligand records of a biaryl and receptor atom - affected receptor ring records do
 *   not take part) and its plane is selected.  The node is the residue of the receptor entity: res_id[atom] of a receptor atom,
 *   the resident amide_res[amide] of a receptor amide, and the RESIDENT ring_res[ring] OF THE RECEPTOR ALONE of a receptor
 *   ring.  That is a deliberate difference from the pose route, which takes the first atom of the ring path: no receptor ring
 *   path is resident here (arp_set_plane_atoms is not needed), and the ligand is no part of the resident structure, so no ligand
 *   atom can have taken a ring's residue over.  The posed residue k_library_planes makes per pose is NOT used.  A node outside
 *   [0, nres) (a ring with residue -1) is skipped.  Class planes exist at residue level only; the ligand side never names a
 *   node.  ref_planes may carry bits up to 28.  Rows, ids, count, cross, occupancy, bits, info (info[3] = NP counts the class
 *   planes) and the best-pose table keep their meaning over the widened feature set; _fetch, _info, _best_launch and
 *   _best_fetch serve both entries.
 *   With a class plane set the launch reads the library result and the library-planes result, and checks ON THE DEVICE that
 *   both were made from the same pose coordinates (the flag comes back with U: still ONE host wait).
 *   ARP_E_ARG with the cause named, in this order, none touching a resident result: a pass not waited for; no library result;
 *   with a bit from ARP_POSEFP_PLANES on: no library-planes result; the two results differ in T (or in their pose ranges);
 *   class planes without ARP_POSEFP_BY_RESIDUE; then a mask of 0 or beyond bit 28; the refusals of
 *   arp_library_fingerprints_launch from ctype_mask on; a reference mask beyond bit 28.  Found after the wait (the fingerprint
 *   before is void by then and none is resident afterwards): "made from different poses".
 *   STATE.  A fingerprint made with class planes is void wherever the library result OR the library-planes result is
 *   (arp_library_planes_launch, arp_set_ligand_library_planes included); its best-pose table goes with it.  One made without
 *   survives both calls.  Making it voids nothing.
 * OUT OF SCOPE: atom-level nodes for rings and amides; the finer ARP_PP_* classes as planes; the all-pairs matrix; one shared
 *   pose upload for the two library launches. */
#define ARP_LIBFP_MAX_FEATURES (1 << 22)
int arp_library_fingerprints_launch(arp_ctx* ctx, uint32_t planes, uint32_t ctype_mask, uint32_t flags, int64_t n_refs,
                                    const int64_t* ref_off, const int32_t* ref_node, const uint32_t* ref_planes, int64_t info[8]);
int arp_library_fingerprints_planes_launch(arp_ctx* ctx, uint32_t planes29, uint32_t ctype_mask, uint32_t flags, int64_t n_refs,
                                           const int64_t* ref_off, const int32_t* ref_node, const uint32_t* ref_planes,
                                           int64_t info[8]);
int arp_library_fingerprints_fetch(arp_ctx* ctx, int64_t cap_nodes, int32_t* ids, uint32_t* count, uint32_t* cross,
                                   uint32_t* occupancy, uint64_t* bits, int64_t* n_nodes);
int arp_library_fingerprints_info(arp_ctx* ctx, int64_t info[8]);
int arp_library_fingerprints_best_launch(arp_ctx* ctx);
int arp_library_fingerprints_best_fetch(arp_ctx* ctx, int64_t cap_ligands, int64_t* n_poses, int32_t* best_pose,
                                        int64_t* tanimoto_q32, uint32_t* shared, uint32_t* count, int64_t* n_ligands,
                                        int64_t* n_refs);
/* Library planes: the ring and amide contacts of every pose of every ligand of the library, in one launch
 * (csrc/arp_library_planes.h).  What arp_poses_planes_launch is to arp_poses_contacts_launch, this is to
 * arp_library_contacts_launch: pi-stacking, cation-pi, donor-pi, halogen-pi and amide stacking of a screen.  An extension
 * beside the mirror; independent of the contacts launch (sharing one upload of the poses between the two is out of scope).
 *
 * RECEPTOR.  As for arp_library_contacts_launch (one structure, refused in the same order).  Its ring centres, normals and ring
 *   residues and its amide centres, normals and residues are resident as initialize() makes them; nring = 0 or namide = 0 is
 *   allowed.  No arp_set_plane_atoms of the receptor is needed: no receptor ring or amide ever moves.  No selection is read.
 * LIBRARY PLANE TABLE (arp_set_ligand_library_planes).  Beside the resident library of L ligands (the call takes no count: L is
 *   the library's): ring_off int32 [L + 1], a CSR over the ligands, TR = ring_off[L] rings in all; ring_atom_off int32 [TR + 1];
 *   ring_atom_idx int32 [ring_atom_off[TR]], every ring in ring-path order, indices WITHIN THE LIGAND; amide_off int32 [L + 1],
 *   TM = amide_off[L] amides in all; amide_atoms int32 [TM][4]: N, C, O, C-alpha, indices within the ligand (the fourth is not
 *   read and may be -1).  At most ARP_LIBRARY_PLANES_MAX_RINGS rings and ARP_LIBRARY_PLANES_MAX_AMIDES amides a ligand; a ring
 *   has at least three atoms.  ring_atom_idx may be NULL when there is no ring, amide_atoms when there is no amide.
 *   ARP_E_ARG with the cause named, checked in this order and before anything is touched: a pass not waited for; no library;
 *   an array missing; an offset array not starting at 0 or decreasing (ring_off, ring_atom_off, amide_off); a ligand over a
 *   limit; a ring of fewer than three atoms; an index outside its own ligand.
 *   Like the library the table reads nothing of the receptor and stays resident through new structures.  It is dropped by
 *   arp_set_ligand_library and replaced by a new arp_set_ligand_library_planes; either voids the result.
 * POSES (arp_library_planes_launch).  pose_off, xyz and T exactly as in arp_library_contacts_launch.  There is no h_xyz, no
 *   cutoff and no vdw_comp: none of the four loops reads them.
 * RESULT.  The COMPLEX of pose t of ligand l is the receptor with ligand l appended as one more residue, uploaded as ONE
 *   structure: the pose's coordinates scattered in, the ligand's rings and amides appended after the receptor's, ring and amide
 *   geometry and ALL ring residues made again as initialize() makes them, the ligand's atoms the selection, _make_selection
 *   with the 6.0 A expansion.  Ids are the complex's: atoms i (receptor) and n + a (ligand), rings r and nring + q, amides m
 *   and namide + g; the ligand's residue is the receptor's residue count.  AFFECTED by a pose are every ligand atom, every
 *   ligand ring, every ligand amide, and every receptor ring with a ligand atom within 3.0 A of its centre at the pose
 *   coordinate (dist2_kd <= 9.0, float64, inclusive).  (arp_poses_planes_launch's "or at its resident coordinate" does not
 *   exist here: a library ligand has no resident coordinate.)  The result of pose t is exactly the records of the complex's
 *   four bags (atom_plane, plane_plane, group_group, group_plane) that involve an affected entity: every column as the pass
 *   gives it — ids, distances and angles to the bit, masks, classes, contact type —; per table ascending (global pose, then
 *   the bag's canonical pair), as arp_poses_planes_fetch.  summary uint32 [T][ARP_POSES_PLANES_SUMMARY] with the slots of
 *   arp_poses_planes_fetch; slot 12 counts the affected rings, the ligand's included; slot 13 the receptor rings whose residue
 *   differs from the resident one (a ligand atom took the ring over); slot 14 the affected rings with residue -1.  Nothing is
 *   truncated: a record buffer that was too small is grown to the counted size and the launch repeated.  Deterministic.
 *   ARP_E_ARG with the cause named, in this order, none touching a resident result: the receptor's refusals; n +
 *   ARP_LIBRARY_MAX_ATOMS, nring + ARP_LIBRARY_PLANES_MAX_RINGS or namide + ARP_LIBRARY_PLANES_MAX_AMIDES not below 2^21 (the
 *   64-bit sort key of arp_poses_planes_launch); no library; no library plane table; pose_off missing, not starting at 0,
 *   decreasing; T out of range; xyz missing; no residue table resident (arp_set_residues: the ligand is one more residue behind
 *   the receptor's, and without a table it would coincide with residue 0).  Found on the device (the result before is void by then and none is resident
 *   afterwards): a non-finite pose coordinate, ARP_E_ARG; more than ARP_POSES_PLANES_MAX_NEAR receptor rings near one pose,
 *   ARP_E_ARG by that name — a ring is never dropped.  ARP_E_CAPACITY: 2^31 records or more.
 *   All work goes on the context's stream (arp_use_stream's, if set); ONE host wait a launch, for the counters with the
 *   device's error word.
 * arp_library_planes_fetch: the shape and column rules of arp_poses_planes_fetch with T for P (ANY pointer may be NULL; cap is
 *   looked at only when a record column is asked for; a column the table does not have: ARP_E_ARG).
 * arp_library_planes_info: info[0] = L, [1] = TR, [2] = TM of the resident plane table (zeros while there is none), [10] = 1
 *   while one is resident; [3] = T, [4 .. 7] = records per table, [8] = blocks of k_library_planes (poses are taken with a grid
 *   stride) of the resident result; [9] = launches of the kernel so far (a repeated launch counts twice); [11] = 1 while the
 *   per-structure set-up (all-atom grid, residue -> atoms) is resident.
 * STATE.  The result is void after a new structure, models, a batch, arp_set_ligand_library, arp_set_ligand_library_planes and a
 *   new launch.  arp_set_selection does NOT void it.  Making it voids nothing: the bags of the last pass, every table made from
 *   them, every pose result, the library contacts, their best-pose table and the library fingerprints stay fetchable and
 *   byte-equal.
 * OUT OF SCOPE: clusters over a library (the class planes of the library fingerprints:
 *   arp_library_fingerprints_planes_launch above; the shortlist, with the best pose per
 *   ligand over this summary: arp_library_shortlist_launch below); peptide and covalent ligands; a batch, models or a shard as the
 *   receptor; receptor - receptor records between unaffected entities. */
#define ARP_LIBRARY_PLANES_MAX_RINGS 32
#define ARP_LIBRARY_PLANES_MAX_AMIDES 32
int arp_set_ligand_library_planes(arp_ctx* ctx, const int32_t* ring_off, const int32_t* ring_atom_off, const int32_t* ring_atom_idx,
                                  const int32_t* amide_off, const int32_t* amide_atoms);
int arp_library_planes_launch(arp_ctx* ctx, const int64_t* pose_off, const float* xyz, int64_t counts[4]);
int arp_library_planes_fetch(arp_ctx* ctx, int table, int64_t cap, uint64_t* pose_off, int32_t* first, int32_t* second, void* v0,
                             void* v1, void* v2, void* v3, uint8_t* u0, uint8_t* u1, uint8_t* u2, uint32_t* summary, int64_t* count);
int arp_library_planes_info(arp_ctx* ctx, int64_t info[12]);
/* Library shortlist: the global poses of the resident library results — or its ligands, each by its best pose — ranked on the
 * device, and only the chosen poses' records — optionally filtered — compacted for the fetch (csrc/arp_library_shortlist.h,
 * DESIGN.md 5x).  What arp_poses_shortlist_launch is to the pose results, this is to the library's.
 *
 * SOURCES: the resident library result (arp_library_contacts_launch), T global poses of L ligands; wherever bits 1 ... 4 of
 *   `tables` or a non-zero weight 16 ... 31 ask for it the resident library-planes result (arp_library_planes_launch); for
 *   ARP_SHORTLIST_TANIMOTO the resident library fingerprint (arp_library_fingerprints_launch).  Nothing of them is written.
 * POSE SCORE: an int64 of one of the three kinds of arp_poses_shortlist_launch.
 *   ARP_SHORTLIST_LIST      no score (0).  The chosen poses are the caller's global poses pose_ids[n_ids] in the caller's order:
 *                           each id in [0, T), repeats allowed, 1 <= n_ids <= ARP_POSES_MAX_POSES.  unit, k and min_score must
 *                           be ARP_LIBRARY_SHORTLIST_POSES, 0 and INT64_MIN.
 *   ARP_SHORTLIST_SUMMARY   score[t] = sum_{s<16} w[s] summary[t][s] + sum_{s<16} w[16 + s] planes_summary[t][s], weights32 =
 *                           int32[32] with |w| <= ARP_SHORTLIST_MAX_WEIGHT (the sum fits 60 bits).  The second half is the
 *                           library-planes result's summary of the SAME POSES (below).
 *   ARP_SHORTLIST_TANIMOTO  pose t is row Q + t of the library fingerprint (Q = n_refs >= 1).  For reference q: x =
 *                           cross[Q + t][q], u = count[Q + t] + count[q] - x, score_q = (u == 0) ? 2^32 : floor(x 2^32 / u) in
 *                           unsigned 64-bit arithmetic.  ref in [0, Q) names the reference, ref = -1 takes the largest score_q.
 *                           The reference rows are never candidates (there is no `skip`).  The scores are taken at launch: the
 *                           shortlist does not read the fingerprint afterwards.
 * UNIT: ARP_LIBRARY_SHORTLIST_POSES — the candidates are all T global poses.  ARP_LIBRARY_SHORTLIST_LIGANDS — the candidates
 *   are the ligands that have at least one pose, each represented by its best pose: the highest pose score, ties to the lower
 *   global pose.  A ligand without poses is never a candidate and never counts towards K.
 * ORDER: descending score, ties by ascending global pose (poses are ligand-major: for ligands that is ascending ligand).  The
 *   chosen entries are the first K = min(k, candidates) of that order whose score is >= min_score, k >= 1; INT64_MIN: no
 *   threshold.  K = 0 is a valid, empty shortlist.
 * TABLES, RECORD FILTER: as arp_poses_shortlist_launch; bits 1 ... 4 name the four tables of the library-planes result.
 * RESULT: ligand int32 [K]; pose int32 [K] (the global pose); score int64 [K]; summary uint32 [K][16] and planes_summary uint32
 *   [K][16], the source rows of the chosen poses, unfiltered; per requested table off uint64 [K + 1] and the table's columns:
 *   the records of entry r are [off[r], off[r + 1]), the kept records of its pose in the order the source holds them, every
 *   column with the source's type and bits — atom-atom (i, a, dist, sift, ctype) as arp_library_contacts_fetch, ring / amide
 *   columns as arp_library_planes_fetch with the complex's ids.  Nothing is truncated; the result is deterministic.
 * SAME POSES: wherever the library-planes result is read it must have the library result's L, T and per-ligand pose ranges,
 *   and must have been made from the same uploaded coordinates (the two launches upload their poses independently; compared on
 *   the device as 32-bit words, the outcome read in the launch's one wait).
 *
 * arp_library_shortlist_launch: info[8] as arp_library_shortlist_info gives it.  One host wait (K, the five totals, the
 *   same-poses flag, the device's error word); every launch and copy goes on the context's stream (arp_use_stream's, if set).
 *   Refusals are ARP_E_ARG with the cause named, in this order, and none of them touches a resident result: a pass not waited
 *   for; no library result; unknown kind; unknown unit; tables 0 or beyond bit 4, sift_mask beyond 15 bits, ctype_mask beyond 7
 *   bits or 0; ARP_SHORTLIST_LIST with pose_ids missing, n_ids out of range, an id outside [0, T), or unit / k / min_score
 *   set; k < 1; ARP_SHORTLIST_SUMMARY with weights missing or beyond +-2^24; ARP_SHORTLIST_TANIMOTO without a library
 *   fingerprint, with n_refs = 0, with ref out of range; "no library-planes result"; "differ in ligands, poses or pose
 *   ranges".  "Made from different poses" is ARP_E_ARG too, found on the device: no shortlist is left after it.
 *   ARP_E_CAPACITY: a table of 2^31 records or more (no shortlist left).  Every successful launch remakes the result.
 *   The shortlist is void exactly when the library result is void or replaced (a new structure, models, a batch,
 *   arp_set_ligand_library, a new arp_library_contacts_launch); one that read the library-planes result also when that is
 *   (arp_library_planes_launch, arp_set_ligand_library_planes).  arp_set_selection does NOT void it, and neither does a later
 *   arp_library_fingerprints_launch.  Making it voids nothing: the bags of the last pass, every table made from them, every
 *   pose result — the pose shortlist included, which is an object of its own —, the library result with its best-pose table,
 *   the library-planes result and the library fingerprint with its best-pose table stay fetchable and byte-equal.
 *
 * arp_library_shortlist_fetch: the per-entry arrays and the atom-atom table; ANY pointer but n_chosen and count may be NULL.
 *   *n_chosen = K, *count = kept atom-atom records.  ARP_E_CAPACITY when a per-entry array (ligand, pose, score, summary,
 *   planes_summary, off) is asked for and cap_entries < K, or a record column is asked for and cap < *count.  ARP_E_ARG: no
 *   valid result; off or a record column of a launch without tables bit 0; planes_summary of a launch that did not read the
 *   library-planes result.
 * arp_library_shortlist_planes_fetch: one ring / amide table a call (ARP_POSES_PLANES_ATOM_PLANE ...), columns and their types
 *   as arp_library_planes_fetch; *count = kept records of the table.  ARP_E_ARG for a table that was not requested and for a
 *   column the table does not have; ARP_E_CAPACITY as above.  Both fetches pass every piece through the page-locked stage in
 *   one wait.
 * arp_library_shortlist_info: info[0] = K, [1] ... [5] = kept records of the five tables (0 for a table not requested), [6] =
 *   launches that did work so far, [7] = kind | unit << 8.  [0] ... [5] and [7] are 0 while there is no result.
 * OUT OF SCOPE: clusters over a library; class planes of the library fingerprints; the top m > 1 poses per ligand; a shortlist
 *   that spans several launches on the device (chunks are merged on the host); multi-GPU. */
#define ARP_LIBRARY_SHORTLIST_POSES 0
#define ARP_LIBRARY_SHORTLIST_LIGANDS 1
int arp_library_shortlist_launch(arp_ctx* ctx, int kind, int unit, const int32_t* weights32, int64_t ref, const int32_t* pose_ids,
                                 int64_t n_ids, int64_t k, int64_t min_score, uint32_t tables, uint32_t sift_mask,
                                 uint32_t ctype_mask, int64_t info[8]);
int arp_library_shortlist_fetch(arp_ctx* ctx, int64_t cap_entries, int64_t cap, int32_t* ligand, int32_t* pose, int64_t* score,
                                uint32_t* summary, uint32_t* planes_summary, uint64_t* off, int32_t* i, int32_t* a, float* dist,
                                uint16_t* sift, uint8_t* ctype, int64_t* n_chosen, int64_t* count);
int arp_library_shortlist_planes_fetch(arp_ctx* ctx, int table, int64_t cap_entries, int64_t cap, uint64_t* off, int32_t* first,
                                       int32_t* second, void* v0, void* v1, void* v2, void* v3, uint8_t* u0, uint8_t* u1,
                                       uint8_t* u2, int64_t* count);
int arp_library_shortlist_info(arp_ctx* ctx, int64_t info[8]);
/* Library clusters: leader clustering (sphere exclusion in rank order) of poses of the resident library result by the Tanimoto
 * similarity of their library fingerprints, on the device, in a WINDOW form that elects up to ARP_LIBCL_WINDOW = 32 leaders a
 * round (csrc/arp_library_clusters.h).  One representative per interaction pattern of a screen, how many poses
 * stand behind it, and their ligands; no bit and no record is copied.
 *
 * SOURCES: three resident results are read while the launch runs and none is written: the library fingerprint
 *   (arp_library_fingerprints_launch; any level, any planes, Q = 0 ... 64 references): W, bits [Q + T][W], count [Q + T]; the
 *   library result (arp_library_contacts_launch): lig_of and T; for ARP_LIBCL_SHORTLIST the library shortlist
 *   (arp_library_shortlist_launch): K and its pose column.
 * POSITIONS: position m names a GLOBAL pose in [0, T).  source = ARP_LIBCL_ALL: pose m, M = T; order must be NULL and n_order 0.
 *   ARP_LIBCL_LIST: pose order[m], M = n_order, 1 <= n_order <= ARP_POSES_MAX_POSES, every id in [0, T), checked on the host
 *   before anything is touched; repeats allowed.  ARP_LIBCL_SHORTLIST: the K >= 1 entries of the resident library shortlist in
 *   rank order (either unit, any kind), M = K; the pose column is copied on the device, no id crosses to the host; order must
 *   be NULL and n_order 0.  The positions are materialised by the launch: a later shortlist does not change the clusters.
 *   Pose t is ROW Q + t of the fingerprint; the reference rows are never positions.
 * SIMILARITY of poses a and b, exactly arp_poses_clusters_launch's: t = sum over the W words of popcount(bits[a][w] & bits[b][w]),
 *   u = count[a] + count[b] - t, q(a, b) = (u == 0) ? 2^32 : floor(t 2^32 / u) in unsigned 64-bit arithmetic; a and b are SIMILAR
 *   when q >= threshold_q32, 0 <= threshold_q32 <= 2^32.
 * CLUSTERING, defined sequentially and exactly arp_poses_clusters_launch's: walk the positions m = 0 ... M - 1; a position whose
 *   pose is similar to some leader's pose joins the FIRST such leader in leader order; otherwise, while fewer than max_clusters
 *   leaders exist (1 <= max_clusters <= ARP_POSECL_MAX_CLUSTERS), it becomes the next leader; otherwise it stays unassigned.
 *   U = 0 (no feature in any row) gives q = 2^32 everywhere: one cluster of M members.
 * RESULT: per position: pose int32 [M], the global pose; ligand int32 [M] = lig_of[pose]; cluster int32 [M], the index in leader
 *   order, -1 when unassigned; similarity int64 [M], q to its own leader's pose, 2^32 for a leader, -1 when unassigned.  Per
 *   cluster: leader int32 [C], the leaders' poses; leader_position int32 [C], strictly ascending; size uint32 [C], the leader
 *   included.  Sum of size + unassigned = M.  Everything is an integer: a pure function of the arguments and the three sources.
 *
 * arp_library_clusters_launch: info[8] as arp_library_clusters_info gives it.  One launch materialises the positions; a round is
 *   two launches: the window kernel (one block) resolves the 32 positions from the lowest unassigned one among themselves and
 *   elects up to 32 leaders, the sweep compares every unassigned position behind the window with those leaders in leader order
 *   and finds the next round's start.  rounds <= min(max_clusters, ceil(M / 32)).  The rounds are enqueued on the context's
 *   stream 32 at a time; after a group that is not the last one word (the next start) is read back and the rounds end when no
 *   position is left; then one launch and the one wait for C, the unassigned count and the rounds that ran.  Refusals are
 *   ARP_E_ARG with the cause named, in this order, and none of them touches a resident result: a pass not waited for; no library
 *   result; no library fingerprint; the fingerprint's P is not Q + T; threshold_q32 > 2^32; max_clusters outside [1, 4096]; an
 *   unknown source; ARP_LIBCL_LIST with order == NULL, with n_order out of range, with an id outside [0, T); another source with
 *   order != NULL or n_order != 0; ARP_LIBCL_SHORTLIST without a valid library shortlist, or with an empty one.  Every successful
 *   launch remakes the result.
 *   The fingerprint and the shortlist are read only while the launch runs: a later arp_library_fingerprints_launch or
 *   arp_library_shortlist_launch leaves the clusters valid.  They are void exactly when the library result is void or replaced
 *   (arp_set_ligand_library, a new arp_library_contacts_launch, a new structure, models or a batch); arp_set_selection does not
 *   void them.  Making them voids nothing; the pose clusters (arp_poses_clusters_launch) are another object and stay resident.
 * arp_library_clusters_fetch: ANY pointer but n_positions and n_clusters may be NULL.  *n_positions = M, *n_clusters = C.
 *   ARP_E_CAPACITY when a per-position array (pose, ligand, cluster, similarity) is asked for and cap_positions < M, or a
 *   per-cluster array (leader, leader_position, size) and cap_clusters < C.  ARP_E_ARG: no valid result.  Every piece goes
 *   through the page-locked stage in one wait.
 * arp_library_clusters_info: info[0] = M, [1] = C, [2] = unassigned, [3] = max_clusters, [4] = W, [5] = rounds that elected a
 *   leader, [6] = launches that did work so far, [7] = threshold_q32.  All but [6] are 0 while there is no result.
 * ARP_LIBCL_LDS_WORDS: the 32 rows a round compares against are staged in LDS when 32 W <= this many words (16 KiB a block: W <= 64), and
 *   read through L2 otherwise; the result does not depend on it.
 * OUT OF SCOPE: the window form for arp_poses_clusters_launch; similarity between ligands as the best over all pose pairs; class
 *   planes of the library fingerprints; clustering across launches; joining the most similar leader; multi-GPU. */
#define ARP_LIBCL_ALL 0
#define ARP_LIBCL_LIST 1
#define ARP_LIBCL_SHORTLIST 2
#define ARP_LIBCL_WINDOW 32
#define ARP_LIBCL_LDS_WORDS 2048
int arp_library_clusters_launch(arp_ctx* ctx, int source, const int32_t* order, int64_t n_order, uint64_t threshold_q32,
                                int64_t max_clusters, int64_t info[8]);
int arp_library_clusters_fetch(arp_ctx* ctx, int64_t cap_positions, int64_t cap_clusters, int32_t* pose, int32_t* ligand,
                               int32_t* cluster, int64_t* similarity, int32_t* leader, int32_t* leader_position, uint32_t* size,
                               int64_t* n_positions, int64_t* n_clusters);
int arp_library_clusters_info(arp_ctx* ctx, int64_t info[8]);

/* ---- ligand-water-receptor contacts of every pose of the library result, joined on the device ----------
 * Which ligand atom of which pose is tied to which receptor atom through which structural water.  TWO resident results are
 * joined and nothing else is read: the library result (arp_library_contacts_launch: T global poses, records (t, i, a) sorted by
 * (t, i, a)) and the atom-atom bag of a finished pass over the RECEPTOR ALONE WITH EVERYTHING SELECTED (arp_run_launch /
 * arp_atom_contacts_launch on the resident structure, same cutoff and vdw_comp as the library launch).  A pass over the receptor
 * voids no library result and a library launch voids no bag, so both can be resident together.
 * RECEPTOR LEG: a bag record (i, j) in which exactly one atom has ARP_F_WATER and (sift & sift_any) != 0; the water is w, the
 *   other atom j (arp_water_bridges_launch's leg, unchanged).
 * LIGAND LEG of pose t: a library record (t, i, a) with ARP_F_WATER on receptor atom i, NO ARP_F_WATER on library atom a and
 *   (sift & sift_any) != 0; the water is w = i.
 * ROWS: one row (t, w, a, j) for every ligand leg (t, w, a) and every receptor leg (w, j), ascending by (t, w, a, j).  There is
 *   no same-residue rule (a ligand is a residue of its own).  A water ligand bridges nothing in this table (its own atom is the
 *   water), and a water-water record is no leg.
 * COLUMNS, in the order of the fetch: pose int32 (global pose t), water int32 (receptor id w), lig_atom int32 (a, index within the
 *   ligand), rec_atom int32 (j, receptor id), dist_lig / dist_rec float32 (the float32 bits of the two source records),
 *   sift_lig / sift_rec uint16 (whole, not masked).  Contact types are NOT columns: a record's type depends on the selection it was
 *   made under — the ligand selected for the library record, everything selected for the receptor's pass — and neither is what a
 *   pass over the complex would print for a bridge.
 * PER POSE: bridge_off uint64 [T + 1], the row offsets; waters uint32 [T], the distinct waters with at least one row; legs
 *   uint32 [T], the ligand legs, whether or not their water has a receptor leg.
 * YARDSTICK: for pose t of ligand l, a whole-structure pass over the complex (receptor + ligand l in that pose, everything
 *   selected, same cutoff and vdw_comp) and arp_water_bridges_launch's join over its bag: the rows of pose t are exactly that
 *   table's rows (w, x, y) in which exactly one of x, y is a ligand atom n + a.  (A pair's SIFt and distance depend on the two
 *   atoms, their hydrogens and single-bond neighbours only; the ligand has no bond to the receptor; everything selected emits
 *   every pair within the cutoff.)
 * arp_library_water_bridges_launch: *count = rows.  sift_any: low 15 bits, not 0.  Refusals are ARP_E_ARG with the cause named,
 *   in this order, and none touches anything resident: sift_any beyond the 15 bits, sift_any 0; no valid library result; a shard
 *   of a distributed structure, no atom-contact results (or a pass not waited for); a bag made under a partial selection; cutoff
 *   or vdw_comp of the pass differ from the library launch's (include_sequence_adjacent need not match: a water has no sequence
 *   neighbours).  ARP_E_CAPACITY at 2^31 rows (*count = rows).  No ligand leg or no receptor leg: *count = 0 and ARP_OK, the
 *   per-pose arrays valid and all zero, nothing more launched.  The same sift_any on the same two sources returns the stored
 *   count without work.  Two waits: the receptor's legs, then ligand legs and rows.
 *   The result is void when the library result is void or replaced (arp_set_ligand_library, a new arp_library_contacts_launch, a
 *   new structure) and when the atom-atom bag is (a new pass, and whatever voids the bag: arp_set_selection among it).  Making
 *   it voids nothing: the five bags, the water-bridge table and every library result stay as they are.
 * arp_library_water_bridges_fetch: ANY pointer but count may be NULL.  *count = rows.  ARP_E_CAPACITY when a column is asked for
 *   and cap_rows < rows, or a per-pose array and cap_poses < T.  ARP_E_ARG: no valid result.  One copy through the page-locked
 *   stage.
 * arp_library_water_bridges_info: info[0] = T, [1] = rows, [2] = ligand legs, [3] = receptor legs, [4] = waters with a receptor
 *   leg, [5] = sift_any, [6] = launches that did work so far, [7] = 1 when both sources are resident and fit (a launch would
 *   pass every refusal behind its mask: what a caller asks before it decides to run the receptor's pass), else 0.  [0] ... [5]
 *   are 0 while there is no result.
 * OUT OF SCOPE: bridges through a LIGAND's water atom; second-order (water-water) bridges; bridge planes in the library
 *   fingerprint; a bridge slot in the shortlist's weights (ARP_SHORTLIST_LIST with a host order of the per-pose counts serves);
 *   restricting the join to a pose subset; the pose route (arp_poses_contacts_launch). */
int arp_library_water_bridges_launch(arp_ctx* ctx, uint32_t sift_any, int64_t* count);
int arp_library_water_bridges_fetch(arp_ctx* ctx, int64_t cap_rows, int64_t cap_poses, int32_t* pose, int32_t* water, int32_t* lig_atom,
                                    int32_t* rec_atom, float* dist_lig, float* dist_rec, uint16_t* sift_lig, uint16_t* sift_rec,
                                    uint64_t* bridge_off, uint32_t* waters, uint32_t* legs, int64_t* count);
int arp_library_water_bridges_info(arp_ctx* ctx, int64_t info[8]);
/* Host side of arp_run_launch, accumulated over *passes calls: us[0] = time spent enqueueing the pass
 * (kernel launches, memsets, events), us[1] = time spent blocked in the one synchronisation. */
int arp_get_host_times(arp_ctx* ctx, double us[2], int64_t* passes, int reset);
/* The context's hipStream_t (as an integer), for callers that want to order their own work
 * against it. */
uint64_t arp_stream_handle(arp_ctx* ctx);
/* Enqueue every pass on the caller's stream instead (0 = back to the context's own stream).
 * With a caller stream, stages 0 and 1 of arp_run_stage return WITHOUT synchronising: the caller
 * orders its exchange (e.g. RCCL through torch.distributed) on the same stream, and only stage 2
 * blocks.  The stream must outlive the context or be reset with 0 first. */
int arp_use_stream(arp_ctx* ctx, uint64_t stream);

/* ---- sharded structures assembled on the device (no counterpart in the reference) ---------------
 * One rank = one context.  The rank uploads the records of its HOME atoms / rings / amides once, the device cuts out
 * the records its two neighbours need (the atoms within one halo width of the slab faces), the caller moves those
 * buffers between the GPUs (RCCL isend / irecv on the device pointers), and the device merges home + received halos
 * into the resident structure: sorted by global id, CSR sections rebuilt, bonded global ids turned into local indices
 * (partners that are not local are dropped), residue table filled, ownership (arp_set_ownership /
 * arp_set_group_ownership) and single-bond-neighbour coordinates set.  Nothing of this goes through host memory; the
 * host sees five counters per buffer.
 *
 * A record buffer = arp_rec_header, then the sections at header.off[] (16-byte aligned): atoms (arp_rec_atom, ascending
 * gid), hydrogen coordinates (double[3] each; an atom's run starts at h_start), bonded GLOBAL ids (int32; bond_start),
 * rings (arp_rec_ring, ascending gid), amides (arp_rec_amide, ascending gid).  Residue ids are global. */
#define ARP_REC_MAGIC 0x3143455250524141ull   /* "AARPREC1" */
typedef struct arp_rec_header {
    uint64_t magic, bytes;
    int64_t na, nh, nb, nring, namide, n_rad;
    uint64_t off[5];
    double lo[3], hi[3], ring_lo[3], ring_hi[3], amide_lo[3], amide_hi[3];   /* boxes that contain the points (any such box) */
    double rad_tab[512];            /* n_rad distinct {vdw, cov} pairs of the sender's home atoms */
} arp_rec_header;
typedef struct arp_rec_atom {       /* 96 bytes */
    float x, y, z; int32_t gid;
    double vdw, cov;
    float sb_x, sb_y, sb_z; int32_t sb_has;      /* coordinates of the single-bond heavy neighbour (U:340-359) */
    int32_t res_gid, res_prev, res_next; uint16_t tmask, flags;
    int32_t h_start, h_cnt, bond_start, bond_cnt;
    uint8_t res_flags, sel, pad[14];
} arp_rec_atom;
typedef struct arp_rec_ring { double c[3], n[3]; int32_t gid, res, pad[2]; } arp_rec_ring;      /* 64 bytes */
typedef struct arp_rec_amide { float c[3], n[3]; int32_t gid, res; } arp_rec_amide;            /* 32 bytes */
/* host-only helpers: size of a record buffer, and header (magic, counts, offsets) written at its start */
uint64_t arp_records_size(int64_t na, int64_t nh, int64_t nb, int64_t nring, int64_t namide);
int arp_records_layout(void* buf, uint64_t bytes, int64_t na, int64_t nh, int64_t nb, int64_t nring, int64_t namide);
/* Host-only packer: the records of the given atoms / rings / amides (ascending ids = global ids) of a structure held as
 * the arrays of the classic setters, written into a buffer whose header arp_records_layout has prepared (na, nring,
 * namide = the list lengths; nh, nb = the hydrogens / bonds of the listed atoms).  sel = selection mask over ALL atoms
 * (NULL: everything selected).  Fills the sections, the radius dictionary of the listed atoms and the boxes. */
int arp_records_fill(void* buf, uint64_t bytes, int64_t n_atoms_total, int64_t n_res_total, int64_t n_rings_total, int64_t n_amides_total,
                     const float* xyz, const double* vdw, const double* cov,
                     const uint16_t* type_mask, const uint16_t* flags, const int32_t* res_id, const uint8_t* res_flags,
                     const int32_t* res_prev, const int32_t* res_next, const int32_t* bond_off, const int32_t* bond_idx,
                     const int32_t* h_off, const double* h_xyz, const int32_t* sb_nbr, const double* ring_center,
                     const double* ring_normal, const int32_t* ring_res, const float* amide_center, const float* amide_normal,
                     const int32_t* amide_res, const uint8_t* sel, const int64_t* atom_ids, const int64_t* ring_ids,
                     const int64_t* amide_ids);
/* Upload the home records (one asynchronous copy; the buffer may be reused when the call returns). */
int arp_shard_set_home(arp_ctx* ctx, const void* records, uint64_t bytes);
/* Records of the home atoms with x_lo <= x <= x_hi (float64 comparison; rings and amides by their centre), packed on
 * the device into a buffer the context owns until the next call with the same `slot` (0 or 1).  The order of the home
 * records is kept.  *device_ptr / *out_bytes: what to send. */
int arp_shard_pack_face(arp_ctx* ctx, int slot, double x_lo, double x_hi, uint64_t* device_ptr, uint64_t* out_bytes);
/* Merge the home records with the record buffers received from the left / right neighbour (DEVICE pointers, 0 = no
 * neighbour on that side) and make the result the resident structure of the context (as arp_set_blob would: selection
 * reset to the whole structure).  nres_global = rows of the global residue table.  counts: atoms, rings, amides.
 * ARP_E_ARG when an atom, ring or amide occurs twice. */
int arp_shard_assemble(arp_ctx* ctx, uint64_t dev_left, uint64_t bytes_left, uint64_t dev_right, uint64_t bytes_right,
                       int64_t nres_global, int64_t counts[3]);
/* What the caller needs to map results back and to exchange selection bits: global id, origin (0 home, -1 / +1 received
 * from the left / right) and selection bit of every local atom; global id and origin of every ring and amide.  Any
 * pointer may be NULL. */
int arp_shard_layout(arp_ctx* ctx, int32_t* global_id, int8_t* origin, uint8_t* sel, int32_t* ring_gid, int8_t* ring_origin,
                     int32_t* amide_gid, int8_t* amide_origin);
/* Read back the resident structure in blob form (arp_blob_header + arrays) when it came from arp_set_blob or
 * arp_shard_assemble: *bytes = size; copies when cap suffices (host may be NULL to ask for the size). */
int arp_get_blob(arp_ctx* ctx, void* host, uint64_t cap, uint64_t* bytes);

/* ---- mmCIF category reader (host only; no context, no GPU) — SURVEY.md 8 row f3 ---------------------------------
 * What the reference asks gemmi for (protein_reader.py:258-289, 415-441): one category of the file as columns
 * (cif_block.get_mmcif_category('_atom_site.') / ('_chem_comp.')).  arp_cif_open parses `text` (CIF 1.1 syntax: loops,
 * pair items, quoted strings, text fields, comments) and keeps the items of the FIRST data block whose tags start with
 * `category` (e.g. "_atom_site.", case-insensitive).  A cell is a slice of the text plus a kind: 0 value, 1 bare '?'
 * (gemmi: None), 2 bare '.' (gemmi: False).  Errors: negative return, message in err (if given). */
typedef struct arp_cif arp_cif;
int arp_cif_open(const char* text, uint64_t len, const char* category, arp_cif** out, char* err, uint64_t err_cap);
void arp_cif_close(arp_cif* t);
int64_t arp_cif_rows(const arp_cif* t);
int arp_cif_cols(const arp_cif* t);
int arp_cif_blocks(const arp_cif* t);                 /* data_ blocks in the file (gemmi's sole_block() wants exactly one) */
const char* arp_cif_tag(const arp_cif* t, int col);   /* item name after the category prefix */
const char* arp_cif_text(const arp_cif* t);           /* the text the cells point into */
/* cells of one column: begin / len / kind arrays of arp_cif_rows() entries, filled by the call */
int arp_cif_column(const arp_cif* t, int col, uint64_t* begin, uint32_t* len, uint8_t* kind);
/* float(value) / int(value) of every cell (C strtod / strtoll over the whole cell); '?' and '.' give `missing`;
 * a cell that is not a number: returns -1 and its row in *bad_row */
int arp_cif_column_f64(const arp_cif* t, int col, double missing, double* out, int64_t* bad_row);
int arp_cif_column_i64(const arp_cif* t, int col, int64_t missing, int64_t* out, int64_t* bad_row);

/* ---- JSON output (host only; no context, no GPU) ------------------------------------------
 * The reference's CLI ends with json.dump(get_contacts(), fh, indent=4, sort_keys=True) (scripts/process_protein_cli.py:
 * 184-188; records of I:172-212).  This writes the same bytes for the atom-atom records straight from the result arrays
 * (sorted keys, indentation, float repr and string escaping of Python's json module) — a Python dict per record costs
 * seconds on a whole-structure run — followed by `tail_records`: the n_tail records of the four ring / amide bags, already
 * rendered at the same indentation and joined with ",\n" (they are few; the Python layer renders them).
 * dist = float64(distance) of every contact; flags bit 0: round it here as I:190 does (round(x, 2) = rint(x * 100) / 100),
 * flags = 0: the caller has rounded already.  sift_names: 15 strings, ctype_names: 7 strings.
 * The records are rendered and written by several host threads (ARP_EXPORT_THREADS; default: the CPUs / CPU quota of the
 * process, at most 32): 814 MB for a 100 k-atom structure in 0.12 s of library time on a 16-CPU quota, 0.41 s with one.
 * Returns 0, or a negative number (-1 bad argument, -2 cannot open, -3 index out of range, -4 write error). */
int arp_write_contacts_json(const char* path, int indent, int flags, int64_t n, const int32_t* ci, const int32_t* cj,
                            const double* dist, const uint16_t* sift, const uint8_t* ctype, int64_t n_atoms,
                            const int32_t* atom_res, const char* const* atom_name, int64_t n_res,
                            const char* const* res_name, const int32_t* res_seq, const char* const* res_chain,
                            const char* const* res_icode, const char* const* res_comp_type,
                            const char* const* sift_names, const char* const* ctype_names, const char* tail_records,
                            int64_t n_tail);

#ifdef __cplusplus
}
#endif
#endif /* ARPEGGIO_HIP_H */
