// The four ring / amide result tables — of a pass (struct Bag), of the poses-planes result and of a pose shortlist alike — and
// every layout made from them.  Host arithmetic only: no HIP call in here.  (C_AP ... C_GP: arp_pairs.h, included before.)
#pragma once
#include <cstddef>
#include <cstdint>

// kind: the order of bag_launch, k_planes, plist[] and the pose tables
enum { BAG_AP, BAG_PP, BAG_GG, BAG_GP, BAG_KINDS };
enum { ENT_ATOM, ENT_RING, ENT_AMIDE };      // what an id column indexes
// A table's columns in the order of its fetch's arguments: two int32 ids, up to four values, up to three bytes.
#define BAG_COLS 9
#define BAG_VAL0 2
#define BAG_BYTE0 6
struct BagKind {
    int counter;         // its record counter
    int n_val;           // value columns ...
    size_t val_size;     // ... of this element size (double or float)
    int n_byte;          // byte columns ...
    int ctype_col;       // ... of which this one holds ctype
    int entity[2];       // what the two id columns index
    int key[2];          // canonical order: the id columns of the major and the minor sort key
    const char* name;    // in messages
};
const BagKind PLANE_TABLES[BAG_KINDS] = {
    {C_AP, 2, sizeof(double), 2, 1, {ENT_ATOM, ENT_RING}, {1, 0}, "atom_plane"},      // (a ring's atoms: by (ring, atom))
    {C_PP, 4, sizeof(double), 3, 2, {ENT_RING, ENT_RING}, {0, 1}, "plane_plane"},
    {C_GG, 3, sizeof(float), 1, 0, {ENT_AMIDE, ENT_AMIDE}, {0, 1}, "group_group"},
    {C_GP, 3, sizeof(double), 1, 0, {ENT_AMIDE, ENT_RING}, {0, 1}, "group_plane"},
};
// The order of get_contacts (I:183-210): counts[1..4] of a pass and bag b of a packed fetch.  Nothing else knows it.
const int PACKED_ORDER[BAG_KINDS] = {BAG_PP, BAG_AP, BAG_GG, BAG_GP};

inline bool bag_has(int kind, int j) {
    return j < BAG_VAL0 || (j < BAG_BYTE0 ? j - BAG_VAL0 < PLANE_TABLES[kind].n_val : j - BAG_BYTE0 < PLANE_TABLES[kind].n_byte);
}
inline size_t bag_es(int kind, int j) { return j < BAG_VAL0 ? sizeof(int32_t) : j < BAG_BYTE0 ? PLANE_TABLES[kind].val_size : 1; }
// slot of column j among the twelve offsets a bag has in a packed fetch (ABI): ids 0 and 1, 8-byte values 2..5, 4-byte values
// 6..8, bytes 9..11
inline int bag_slot(int kind, int j) {
    return j < BAG_VAL0 ? j : j < BAG_BYTE0 ? (PLANE_TABLES[kind].val_size == 8 ? 2 : 6) + (j - BAG_VAL0) : 9 + (j - BAG_BYTE0);
}
inline size_t al256(size_t v) { return (v + 255) & ~(size_t)255; }
inline size_t al16(size_t v) { return (v + 15) & ~(size_t)15; }
// In a slab: the columns the table names for m records, from `at` on, each on a 256-byte boundary.  Returns the end.
inline size_t bag_slab_layout(int kind, size_t m, size_t at, size_t off[BAG_COLS]) {
    for (int j = 0; j < BAG_COLS; ++j) {
        off[j] = at;
        if (bag_has(kind, j)) at += al256(m * bag_es(kind, j));
    }
    return at;
}
// In a piece that travels to the host (staged or packed): the used prefixes of those columns from `at` on, each on a 16-byte
// boundary.  Returns the end.
inline size_t bag_piece_layout(int kind, size_t count, size_t at, size_t off[BAG_COLS]) {
    for (int j = 0; j < BAG_COLS; ++j) {
        off[j] = at;
        if (bag_has(kind, j)) at = al16(at + count * bag_es(kind, j));
    }
    return at;
}
// An upper bound on what bag_piece_layout adds for `records` records in the four bags together: a record costs no more than the
// largest record of the table, and the rounding of a column is less than 16 bytes.
inline size_t bag_piece_bound(size_t records) {
    size_t largest = 0, columns = 0;
    for (int kind = 0; kind < BAG_KINDS; ++kind) {
        size_t record = 0;
        for (int j = 0; j < BAG_COLS; ++j)
            if (bag_has(kind, j)) { record += bag_es(kind, j); ++columns; }
        if (record > largest) largest = record;
    }
    return largest * records + 16 * columns;
}
