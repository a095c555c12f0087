// arp_blob.h — the two host buffers a structure travels in, each described once: the blob (arp_blob_header + 21 arrays:
// arp_set_blob, arp_set_topology / arp_set_models, arp_shard_assemble) and the record buffer of the shard path (arp_rec_header
// + 5 sections).  Host code only, no context: the array names, one table row per array, the builder of a complete header that
// every size / layout / check goes through, the two host packers, and the bounding-box helpers.  Included by arp_api.hip after
// the public header (whose prototypes give the entry points their C linkage) and arp_pairs.h (RAD_TABLE, RAD_NONE).
#pragma once
#include <algorithm>
#include <cstdint>
#include <cstring>
#include <vector>

namespace {
uint64_t align16(uint64_t v) { return (v + 15ull) & ~15ull; }

// ---- bounding boxes ----------------------------------------------------------------------------------------------------
// lo / hi of cnt points whose coordinate q is coord(k, q), widened to double; 0 for an empty set
template <class Coord>
void points_box(int64_t cnt, double lo[3], double hi[3], Coord coord) {
    for (int q = 0; q < 3; ++q) lo[q] = hi[q] = cnt > 0 ? (double)coord((int64_t)0, q) : 0.0;
    for (int64_t k = 1; k < cnt; ++k)
        for (int q = 0; q < 3; ++q) {
            const double v = (double)coord(k, q);
            lo[q] = std::min(lo[q], v);
            hi[q] = std::max(hi[q], v);
        }
}
template <class T>
void points_box(const T* xyz, int64_t cnt, double lo[3], double hi[3]) {     // (packed x, y, z)
    points_box(cnt, lo, hi, [xyz](int64_t k, int q) { return xyz[3 * k + q]; });
}
// lo / hi grow to hold the box [l, u]; the first box (any still false) replaces what they held
void box_union(double lo[3], double hi[3], bool& any, const double l[3], const double u[3]) {
    for (int k = 0; k < 3; ++k) {
        lo[k] = any ? std::min(lo[k], l[k]) : l[k];
        hi[k] = any ? std::max(hi[k], u[k]) : u[k];
    }
    any = true;
}

// ---- the blob ----------------------------------------------------------------------------------------------------------
// The arrays in the order of arp_blob_header::off[] (the table in include/arpeggio_hip.h is the public statement of it).
enum BlobArray {
    BLOB_XYZ, BLOB_RAD, BLOB_TMASK, BLOB_FLAGS, BLOB_RES_ID, BLOB_RES_FLAGS, BLOB_RES_PREV, BLOB_RES_NEXT, BLOB_BOND_OFF, BLOB_BOND_IDX,
    BLOB_H_OFF, BLOB_H_XYZ, BLOB_SB_NBR, BLOB_RING_C, BLOB_RING_N, BLOB_RING_RES, BLOB_AMIDE_C, BLOB_AMIDE_N, BLOB_AMIDE_RES, BLOB_RAD_IDX,
    BLOB_RAD_TAB, BLOB_ARRAY_COUNT
};
static_assert(BLOB_ARRAY_COUNT == ARP_BLOB_ARRAYS, "one name per array of arp_blob_header::off[]");

// One row per array: it holds times * (the count it goes by) + plus elements of esize bytes.
enum BlobCount { PER_ATOM, PER_RES, PER_BOND, PER_H, PER_RING, PER_AMIDE };
struct BlobRow { uint64_t esize, times; BlobCount of; uint64_t plus; };
const BlobRow BLOB_ROWS[ARP_BLOB_ARRAYS] = {
    {4, 4, PER_ATOM, 0},                // BLOB_XYZ        float   x, y, z, 0
    {8, 2, PER_ATOM, 0},                // BLOB_RAD        double  vdw, cov
    {2, 1, PER_ATOM, 0},                // BLOB_TMASK      uint16
    {2, 1, PER_ATOM, 0},                // BLOB_FLAGS      uint16
    {4, 1, PER_ATOM, 0},                // BLOB_RES_ID     int32
    {1, 1, PER_RES, 0},                 // BLOB_RES_FLAGS  uint8
    {4, 1, PER_RES, 0},                 // BLOB_RES_PREV   int32
    {4, 1, PER_RES, 0},                 // BLOB_RES_NEXT   int32
    {4, 1, PER_ATOM, 1},                // BLOB_BOND_OFF   int32   CSR
    {4, 1, PER_BOND, 0},                // BLOB_BOND_IDX   int32
    {4, 1, PER_ATOM, 1},                // BLOB_H_OFF      int32   CSR
    {8, 3, PER_H, 0},                   // BLOB_H_XYZ      double
    {4, 1, PER_ATOM, 0},                // BLOB_SB_NBR     int32
    {8, 3, PER_RING, 0},                // BLOB_RING_C     double
    {8, 3, PER_RING, 0},                // BLOB_RING_N     double
    {4, 1, PER_RING, 0},                // BLOB_RING_RES   int32
    {4, 3, PER_AMIDE, 0},               // BLOB_AMIDE_C    float
    {4, 3, PER_AMIDE, 0},               // BLOB_AMIDE_N    float
    {4, 1, PER_AMIDE, 0},               // BLOB_AMIDE_RES  int32
    {2, 1, PER_ATOM, 0},                // BLOB_RAD_IDX    uint16
    {8, 0, PER_ATOM, 2 * RAD_TABLE},    // BLOB_RAD_TAB    double  {vdw, cov} pairs
};

// The complete header of a blob with these counts: magic, counts, bytes and offsets (n_rad and the boxes 0).  false: bad counts.
bool blob_header(int64_t n, int64_t nres, int64_t nbond, int64_t nh, int64_t nring, int64_t namide, arp_blob_header& h) {
    if (n < 0 || nres < 0 || nbond < 0 || nh < 0 || nring < 0 || namide < 0) return false;
    if (n > 0x7FFFFFF0LL || nres > 0x7FFFFFF0LL || nbond > 0x7FFFFFF0LL || nh > 0x7FFFFFF0LL / 3 || nring > 0x7FFFFFF0LL / 3 ||
        namide > 0x7FFFFFF0LL / 3)
        return false;
    memset(&h, 0, sizeof(h));
    h.magic = ARP_BLOB_MAGIC;
    h.n = n; h.nres = nres; h.nbond = nbond; h.nh = nh; h.nring = nring; h.namide = namide;
    const uint64_t cnt[6] = {(uint64_t)n, (uint64_t)nres, (uint64_t)nbond, (uint64_t)nh, (uint64_t)nring, (uint64_t)namide};
    uint64_t off = align16(sizeof(arp_blob_header));
    for (int k = 0; k < ARP_BLOB_ARRAYS; ++k) {
        const BlobRow& r = BLOB_ROWS[k];
        h.off[k] = off;
        off = align16(off + r.esize * (r.times * cnt[r.of] + r.plus));
    }
    h.bytes = off;
    return true;
}

// array a of the blob at base whose header is h
template <class T>
T* blob_at(uint8_t* base, const arp_blob_header& h, BlobArray a) { return reinterpret_cast<T*>(base + h.off[a]); }
template <class T>
const T* blob_at(const uint8_t* base, const arp_blob_header& h, BlobArray a) { return reinterpret_cast<const T*>(base + h.off[a]); }
}  // namespace

uint64_t arp_blob_size(int64_t n, int64_t nres, int64_t nbond, int64_t nh, int64_t nring, int64_t namide) {
    arp_blob_header h;
    return blob_header(n, nres, nbond, nh, nring, namide, h) ? h.bytes : 0;
}

int arp_blob_layout(void* blob, uint64_t bytes, int64_t n, int64_t nres, int64_t nbond, int64_t nh, int64_t nring, int64_t namide) {
    arp_blob_header h;
    if (!blob || !blob_header(n, nres, nbond, nh, nring, namide, h) || bytes < h.bytes) return ARP_E_ARG;
    memcpy(blob, &h, sizeof(h));
    return ARP_OK;
}

int arp_blob_fill(void* blob, uint64_t bytes, const float* xyz, const double* vdw, const double* cov, const uint16_t* type_mask,
                  const uint16_t* flags, const int32_t* res_id, const uint8_t* res_flags, const int32_t* res_prev,
                  const int32_t* res_next, const int32_t* bond_off, const int32_t* bond_idx, const int32_t* h_off,
                  const double* h_xyz, const int32_t* sb_nbr, const double* ring_center, const double* ring_normal,
                  const int32_t* ring_res, const float* amide_center, const float* amide_normal, const int32_t* amide_res) {
    if (!blob || bytes < sizeof(arp_blob_header)) return ARP_E_ARG;
    arp_blob_header h;
    memcpy(&h, blob, sizeof(h));
    if (h.magic != ARP_BLOB_MAGIC || h.bytes > bytes || h.bytes != arp_blob_size(h.n, h.nres, h.nbond, h.nh, h.nring, h.namide)) return ARP_E_ARG;
    const int64_t n = h.n;
    if ((n > 0 && (!xyz || !vdw || !cov || !type_mask || !flags || !res_id || !bond_off || !h_off || !sb_nbr)) ||
        (h.nres > 0 && (!res_flags || !res_prev || !res_next)) || (h.nbond > 0 && !bond_idx) || (h.nh > 0 && !h_xyz) ||
        (h.nring > 0 && (!ring_center || !ring_normal || !ring_res)) || (h.namide > 0 && (!amide_center || !amide_normal || !amide_res)))
        return ARP_E_ARG;
    uint8_t* const b = (uint8_t*)blob;
    float* x4 = blob_at<float>(b, h, BLOB_XYZ);
    double* r2 = blob_at<double>(b, h, BLOB_RAD);
    for (int64_t i = 0; i < n; ++i) {
        x4[4 * i] = xyz[3 * i]; x4[4 * i + 1] = xyz[3 * i + 1]; x4[4 * i + 2] = xyz[3 * i + 2]; x4[4 * i + 3] = 0.0f;
        r2[2 * i] = vdw[i]; r2[2 * i + 1] = cov[i];
    }
    auto copy = [&](BlobArray a, const void* src, size_t nbytes) { if (nbytes) memcpy(b + h.off[a], src, nbytes); };
    copy(BLOB_TMASK, type_mask, (size_t)n * 2); copy(BLOB_FLAGS, flags, (size_t)n * 2); copy(BLOB_RES_ID, res_id, (size_t)n * 4);
    copy(BLOB_RES_FLAGS, res_flags, (size_t)h.nres); copy(BLOB_RES_PREV, res_prev, (size_t)h.nres * 4); copy(BLOB_RES_NEXT, res_next, (size_t)h.nres * 4);
    if (n > 0) { copy(BLOB_BOND_OFF, bond_off, ((size_t)n + 1) * 4); copy(BLOB_H_OFF, h_off, ((size_t)n + 1) * 4); }
    else { const int32_t z = 0; copy(BLOB_BOND_OFF, &z, 4); copy(BLOB_H_OFF, &z, 4); }
    copy(BLOB_BOND_IDX, bond_idx, (size_t)h.nbond * 4); copy(BLOB_H_XYZ, h_xyz, (size_t)h.nh * 24); copy(BLOB_SB_NBR, sb_nbr, (size_t)n * 4);
    copy(BLOB_RING_C, ring_center, (size_t)h.nring * 24); copy(BLOB_RING_N, ring_normal, (size_t)h.nring * 24); copy(BLOB_RING_RES, ring_res, (size_t)h.nring * 4);
    copy(BLOB_AMIDE_C, amide_center, (size_t)h.namide * 12); copy(BLOB_AMIDE_N, amide_normal, (size_t)h.namide * 12); copy(BLOB_AMIDE_RES, amide_res, (size_t)h.namide * 4);
    // dictionary of the distinct {vdw, cov} pairs, compared bit for bit: a handful of element values in practice, so a
    // small open-addressing table keyed by the 128 bits; entries are numbered in ascending (vdw bits, cov bits) order
    uint16_t* ridx = blob_at<uint16_t>(b, h, BLOB_RAD_IDX);
    double* tab = blob_at<double>(b, h, BLOB_RAD_TAB);
    memset(tab, 0, sizeof(double) * 2 * RAD_TABLE);
    struct Key { uint64_t a, b; int64_t count; int slot; };
    std::vector<Key> keys;
    std::vector<int> hash(4096, -1);
    std::vector<int> key_of((size_t)n);
    auto bits = [](double d) { uint64_t u; memcpy(&u, &d, 8); return u; };
    for (int64_t i = 0; i < n; ++i) {
        const uint64_t ka = bits(vdw[i]), kb = bits(cov[i]);
        size_t hpos = (size_t)((ka * 0x9E3779B97F4A7C15ull) ^ (kb * 0xC2B2AE3D27D4EB4Full)) >> 20;
        int found = -1;
        for (;;) {
            hpos &= hash.size() - 1;
            const int k = hash[hpos];
            if (k < 0) break;
            if (keys[(size_t)k].a == ka && keys[(size_t)k].b == kb) { found = k; break; }
            ++hpos;
        }
        if (found < 0) {
            if (keys.size() * 2 >= hash.size()) {   // grow and re-insert
                std::vector<int> bigger(hash.size() * 4, -1);
                for (size_t k = 0; k < keys.size(); ++k) {
                    size_t p = (size_t)((keys[k].a * 0x9E3779B97F4A7C15ull) ^ (keys[k].b * 0xC2B2AE3D27D4EB4Full)) >> 20;
                    for (;; ++p) { p &= bigger.size() - 1; if (bigger[p] < 0) { bigger[p] = (int)k; break; } }
                }
                hash.swap(bigger);
                hpos = (size_t)((ka * 0x9E3779B97F4A7C15ull) ^ (kb * 0xC2B2AE3D27D4EB4Full)) >> 20;
                for (;; ++hpos) { hpos &= hash.size() - 1; if (hash[hpos] < 0) break; }
            }
            found = (int)keys.size();
            keys.push_back(Key{ka, kb, 0, -1});
            hash[hpos] = found;
        }
        ++keys[(size_t)found].count;
        key_of[(size_t)i] = found;
    }
    std::vector<int> order(keys.size());
    for (size_t k = 0; k < keys.size(); ++k) order[k] = (int)k;
    std::sort(order.begin(), order.end(), [&](int p, int q) { return keys[(size_t)p].a != keys[(size_t)q].a ? keys[(size_t)p].a < keys[(size_t)q].a : keys[(size_t)p].b < keys[(size_t)q].b; });
    if (keys.size() <= (size_t)RAD_TABLE) {
        for (size_t r = 0; r < order.size(); ++r) keys[(size_t)order[r]].slot = (int)r;
        h.n_rad = (int64_t)keys.size();
    } else {   // the 256 most frequent pairs (ties: the smaller pair first), numbered by descending frequency
        std::stable_sort(order.begin(), order.end(), [&](int p, int q) { return keys[(size_t)p].count > keys[(size_t)q].count; });
        for (size_t r = 0; r < (size_t)RAD_TABLE; ++r) keys[(size_t)order[r]].slot = (int)r;
        h.n_rad = RAD_TABLE;
    }
    for (const Key& k : keys)
        if (k.slot >= 0) { memcpy(&tab[2 * k.slot], &k.a, 8); memcpy(&tab[2 * k.slot + 1], &k.b, 8); }
    for (int64_t i = 0; i < n; ++i) {
        const int slot = keys[(size_t)key_of[(size_t)i]].slot;
        ridx[i] = slot >= 0 ? (uint16_t)slot : (uint16_t)RAD_NONE;
    }
    // bounding boxes (0 for an empty set)
    points_box(xyz, n, h.lo, h.hi);
    points_box(ring_center, h.nring, h.ring_lo, h.ring_hi);
    points_box(amide_center, h.namide, h.amide_lo, h.amide_hi);
    memcpy(blob, &h, sizeof(h));
    return ARP_OK;
}

// ---- the record buffer of the shard path ----------------------------------------------------------------------------------
namespace {
// The sections in the order of arp_rec_header::off[]; section k holds the k-th count of the header, REC_ESIZE[k] bytes each.
enum RecSection { REC_ATOMS, REC_H_XYZ, REC_BONDS, REC_RINGS, REC_AMIDES, REC_SECTION_COUNT };
const uint64_t REC_ESIZE[REC_SECTION_COUNT] = {sizeof(arp_rec_atom), 3 * sizeof(double), sizeof(int32_t), sizeof(arp_rec_ring), sizeof(arp_rec_amide)};
static_assert(sizeof(((arp_rec_header*)nullptr)->off) == REC_SECTION_COUNT * sizeof(uint64_t), "one name per section of arp_rec_header::off[]");

bool rec_counts_ok(int64_t na, int64_t nh, int64_t nb, int64_t nring, int64_t namide) {
    const int64_t lim = 0x7FFFFFF0LL / 3;
    return na >= 0 && nh >= 0 && nb >= 0 && nring >= 0 && namide >= 0 && na <= lim && nh <= lim && nb <= 0x7FFFFFF0LL && nring <= lim &&
           namide <= lim;
}

// The complete header of a record buffer with these counts: magic, counts, bytes and offsets (the rest 0).  false: bad counts.
bool rec_header(int64_t na, int64_t nh, int64_t nb, int64_t nring, int64_t namide, arp_rec_header& h) {
    if (!rec_counts_ok(na, nh, nb, nring, namide)) return false;
    memset(&h, 0, sizeof(h));
    h.magic = ARP_REC_MAGIC;
    h.na = na; h.nh = nh; h.nb = nb; h.nring = nring; h.namide = namide;
    const int64_t cnt[REC_SECTION_COUNT] = {na, nh, nb, nring, namide};
    uint64_t off = align16(sizeof(arp_rec_header));
    for (int k = 0; k < REC_SECTION_COUNT; ++k) {
        h.off[k] = off;
        off = align16(off + REC_ESIZE[k] * (uint64_t)cnt[k]);
    }
    h.bytes = off;
    return true;
}
}  // namespace

uint64_t arp_records_size(int64_t na, int64_t nh, int64_t nb, int64_t nring, int64_t namide) {
    arp_rec_header h;
    return rec_header(na, nh, nb, nring, namide, h) ? h.bytes : 0;
}

int arp_records_layout(void* buf, uint64_t bytes, int64_t na, int64_t nh, int64_t nb, int64_t nring, int64_t namide) {
    arp_rec_header h;
    if (!buf || !rec_header(na, nh, nb, nring, namide, h) || bytes < h.bytes) return ARP_E_ARG;
    memcpy(buf, &h, sizeof(h));
    return ARP_OK;
}

int arp_records_fill(void* buf, uint64_t bytes, int64_t n_total, int64_t nres_total, int64_t nring_total, int64_t namide_total, const float* xyz, const double* vdw, const double* cov,
                     const uint16_t* type_mask, const uint16_t* flags, const int32_t* res_id, const uint8_t* res_flags,
                     const int32_t* res_prev, const int32_t* res_next, const int32_t* bond_off, const int32_t* bond_idx,
                     const int32_t* h_off, const double* h_xyz, const int32_t* sb_nbr, const double* ring_center,
                     const double* ring_normal, const int32_t* ring_res, const float* amide_center, const float* amide_normal,
                     const int32_t* amide_res, const uint8_t* sel, const int64_t* atom_ids, const int64_t* ring_ids,
                     const int64_t* amide_ids) {
    if (!buf || bytes < sizeof(arp_rec_header)) return ARP_E_ARG;
    arp_rec_header h;
    memcpy(&h, buf, sizeof(h));
    if (h.magic != ARP_REC_MAGIC || h.bytes > bytes || h.bytes != arp_records_size(h.na, h.nh, h.nb, h.nring, h.namide)) return ARP_E_ARG;
    if ((h.na > 0 && (!atom_ids || !xyz || !vdw || !cov || !type_mask || !flags || !res_id || !res_flags || !res_prev || !res_next || !bond_off ||
                      !h_off || !sb_nbr)) ||
        (h.nring > 0 && (!ring_ids || !ring_center || !ring_normal || !ring_res)) ||
        (h.namide > 0 && (!amide_ids || !amide_center || !amide_normal || !amide_res)))
        return ARP_E_ARG;
    uint8_t* const b = (uint8_t*)buf;
    memset(b + sizeof(h), 0, (size_t)h.bytes - sizeof(h));
    arp_rec_atom* A = (arp_rec_atom*)(b + h.off[REC_ATOMS]);
    double* H = (double*)(b + h.off[REC_H_XYZ]);
    int32_t* B = (int32_t*)(b + h.off[REC_BONDS]);
    arp_rec_ring* R = (arp_rec_ring*)(b + h.off[REC_RINGS]);
    arp_rec_amide* M = (arp_rec_amide*)(b + h.off[REC_AMIDES]);
    int64_t hs = 0, bs = 0;
    struct Pair { uint64_t a, b; };
    std::vector<Pair> uniq;
    auto bits = [](double d) { uint64_t u; memcpy(&u, &d, 8); return u; };
    for (int64_t k = 0; k < h.na; ++k) {
        const int64_t i = atom_ids[k];
        if (i < 0 || i >= n_total || (k > 0 && atom_ids[k - 1] >= i)) return ARP_E_ARG;
        arp_rec_atom& r = A[k];
        r.x = xyz[3 * i]; r.y = xyz[3 * i + 1]; r.z = xyz[3 * i + 2]; r.gid = (int32_t)i;
        r.vdw = vdw[i]; r.cov = cov[i];
        const int32_t nb = sb_nbr[i];
        if (nb < -1 || nb >= n_total) return ARP_E_ARG;
        if (nb >= 0) { r.sb_x = xyz[3 * (int64_t)nb]; r.sb_y = xyz[3 * (int64_t)nb + 1]; r.sb_z = xyz[3 * (int64_t)nb + 2]; r.sb_has = 1; }
        const int32_t res = res_id[i];
        if (res < 0 || res >= nres_total) return ARP_E_ARG;
        r.res_gid = res; r.res_prev = res_prev[res]; r.res_next = res_next[res]; r.res_flags = res_flags[res];
        r.tmask = type_mask[i]; r.flags = flags[i];
        r.sel = sel ? sel[i] : (uint8_t)1;
        r.h_start = (int32_t)hs; r.h_cnt = h_off[i + 1] - h_off[i];
        r.bond_start = (int32_t)bs; r.bond_cnt = bond_off[i + 1] - bond_off[i];
        if (r.h_cnt < 0 || r.bond_cnt < 0 || hs + r.h_cnt > h.nh || bs + r.bond_cnt > h.nb) return ARP_E_ARG;
        if (r.h_cnt) memcpy(H + 3 * hs, h_xyz + 3 * (int64_t)h_off[i], (size_t)r.h_cnt * 24);
        if (r.bond_cnt) memcpy(B + bs, bond_idx + bond_off[i], (size_t)r.bond_cnt * 4);
        hs += r.h_cnt; bs += r.bond_cnt;
        const Pair key{bits(r.vdw), bits(r.cov)};
        bool seen = false;
        for (const Pair& u : uniq) if (u.a == key.a && u.b == key.b) { seen = true; break; }
        if (!seen && uniq.size() < 4096) uniq.push_back(key);     // (a handful of element values in practice)
    }
    if (hs != h.nh || bs != h.nb) return ARP_E_ARG;
    for (int64_t k = 0; k < h.nring; ++k) {
        const int64_t i = ring_ids[k];
        if (i < 0 || i >= nring_total || (k > 0 && ring_ids[k - 1] >= i) || ring_res[i] < -1 || ring_res[i] >= nres_total) return ARP_E_ARG;
        for (int q = 0; q < 3; ++q) { R[k].c[q] = ring_center[3 * i + q]; R[k].n[q] = ring_normal[3 * i + q]; }
        R[k].gid = (int32_t)i; R[k].res = ring_res[i];
    }
    for (int64_t k = 0; k < h.namide; ++k) {
        const int64_t i = amide_ids[k];
        if (i < 0 || i >= namide_total || (k > 0 && amide_ids[k - 1] >= i) || amide_res[i] < -1 || amide_res[i] >= nres_total) return ARP_E_ARG;
        for (int q = 0; q < 3; ++q) { M[k].c[q] = amide_center[3 * i + q]; M[k].n[q] = amide_normal[3 * i + q]; }
        M[k].gid = (int32_t)i; M[k].res = amide_res[i];
    }
    std::sort(uniq.begin(), uniq.end(), [](const Pair& p, const Pair& q) { return p.a != q.a ? p.a < q.a : p.b < q.b; });
    h.n_rad = (int64_t)std::min<size_t>(uniq.size(), RAD_TABLE);
    memset(h.rad_tab, 0, sizeof(h.rad_tab));
    for (int64_t k = 0; k < h.n_rad; ++k) { memcpy(&h.rad_tab[2 * k], &uniq[(size_t)k].a, 8); memcpy(&h.rad_tab[2 * k + 1], &uniq[(size_t)k].b, 8); }
    points_box(h.na, h.lo, h.hi, [&](int64_t k, int q) { return (&A[k].x)[q]; });
    points_box(h.nring, h.ring_lo, h.ring_hi, [&](int64_t k, int q) { return R[k].c[q]; });
    points_box(h.namide, h.amide_lo, h.amide_hi, [&](int64_t k, int q) { return M[k].c[q]; });
    memcpy(buf, &h, sizeof(h));
    return ARP_OK;
}
