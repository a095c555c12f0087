// arp_batchgrid.h — where every structure of a batch (arp_set_batch) sits in the common grid.  Plain C++: no HIP, no device
// code, so the arithmetic is testable on a machine without a GPU (arp_batch_layout in both libraries).
//
// Every structure gets the cells its own box needs at the cell edge and an integer offset in a common grid — shelves along
// x, rows along y, layers along z, ONE empty cell between neighbours in every direction, the whole as near to a cube as the
// largest structure allows.  The edge starts at radius (1 + 1e-6) and grows by 1.26 until no structure has 4096 cells or
// more on an axis and the common grid has at most 2^26 cells.
#pragma once
#include <stdint.h>

#include <algorithm>
#include <cmath>

// place[s] = origin of structure s's box, its cell offset in the common grid and its cell counts
struct BatchPlace {
    double ox, oy, oz;
    int cx, cy, cz, nx, ny, nz;
};

#define ARP_BATCH_AXIS_CELLS 4096               // a structure stays BELOW this many cells on every axis
#define ARP_BATCH_GRID_CELLS ((double)(1 << 26))   // the common grid holds at most this many cells

// boxes: 6 per structure (lo xyz, hi xyz; finite, hi >= lo: arp_set_batch checks).  places: B entries.  dims: NX, NY, NZ of
// the common grid.  Returns the cell edge.
inline double batch_layout(int64_t B, const double* boxes, double radius, BatchPlace* places, int dims[3]) {
    double edge = radius * (1.0 + 1e-6);
    if (!(edge > 0)) edge = 1.0;
    int NX = 1, NY = 1, NZ = 1;
    for (;;) {
        double vol = 0;
        int mx = 1, my = 1, mz = 1;
        bool too_big = false;
        for (int64_t s_ = 0; s_ < B; ++s_) {
            const double* lo = boxes + (size_t)s_ * 6;
            const double* hi = lo + 3;
            const double nx = std::floor((hi[0] - lo[0]) / edge) + 1, ny = std::floor((hi[1] - lo[1]) / edge) + 1, nz = std::floor((hi[2] - lo[2]) / edge) + 1;
            if (!(nx < ARP_BATCH_AXIS_CELLS && ny < ARP_BATCH_AXIS_CELLS && nz < ARP_BATCH_AXIS_CELLS)) { too_big = true; break; }
            places[(size_t)s_] = BatchPlace{lo[0], lo[1], lo[2], 0, 0, 0, (int)nx, (int)ny, (int)nz};
            vol += (nx + 1) * (ny + 1) * (nz + 1);
            mx = std::max(mx, (int)nx); my = std::max(my, (int)ny); mz = std::max(mz, (int)nz);
        }
        if (!too_big) {
            const int side = (int)std::ceil(std::cbrt(vol));
            const int LX = std::max(side, mx), LY = std::max(side, my);
            int x = 0, y = 0, z = 0, row_h = 0, layer_h = 0;
            NX = NY = NZ = 1;
            for (int64_t s_ = 0; s_ < B; ++s_) {
                BatchPlace& b = places[(size_t)s_];
                if (x > 0 && x + b.nx > LX) { x = 0; y += row_h + 1; row_h = 0; }
                if (y > 0 && y + b.ny > LY) { x = 0; y = 0; z += layer_h + 1; layer_h = 0; row_h = 0; }
                b.cx = x; b.cy = y; b.cz = z;
                NX = std::max(NX, x + b.nx); NY = std::max(NY, y + b.ny); NZ = std::max(NZ, z + b.nz);
                x += b.nx + 1;
                row_h = std::max(row_h, b.ny);
                layer_h = std::max(layer_h, b.nz);
            }
            if ((double)NX * NY * NZ <= ARP_BATCH_GRID_CELLS) break;
        }
        edge *= 1.26;
    }
    dims[0] = NX; dims[1] = NY; dims[2] = NZ;
    return edge;
}

// what arp_set_batch and arp_batch_layout ask of the boxes: finite corners, hi >= lo, a finite extent (the growth of the
// edge ends only then)
inline bool batch_boxes_ok(int64_t nstruct, const double* boxes) {
    for (int64_t s_ = 0; s_ < nstruct; ++s_)
        for (int a = 0; a < 3; ++a) {
            const double lo = boxes[6 * s_ + a], hi = boxes[6 * s_ + 3 + a];
            if (!std::isfinite(lo) || !std::isfinite(hi) || hi < lo || !std::isfinite(hi - lo)) return false;
        }
    return true;
}

// The body of arp_batch_layout (include/arpeggio_hip.h), the same in both libraries.  places_out: int32[6 * nstruct] = cx,
// cy, cz, nx, ny, nz of every structure (its origin is its box's lo corner).  0, or -1 for bad arguments.
inline int batch_layout_c(int64_t nstruct, const double* boxes, double radius, int32_t* places_out, int32_t dims_out[3], double* edge_out) {
    if (nstruct < 0 || (nstruct > 0 && (!boxes || !places_out)) || !dims_out || !edge_out) return -1;
    if (!batch_boxes_ok(nstruct, boxes) || std::isnan(radius)) return -1;
    BatchPlace* pl = nstruct > 0 ? new BatchPlace[(size_t)nstruct] : nullptr;
    int dims[3];
    *edge_out = batch_layout(nstruct, boxes, radius, pl, dims);
    for (int64_t s_ = 0; s_ < nstruct; ++s_) {
        const BatchPlace& b = pl[(size_t)s_];
        int32_t* o = places_out + 6 * s_;
        o[0] = b.cx; o[1] = b.cy; o[2] = b.cz; o[3] = b.nx; o[4] = b.ny; o[5] = b.nz;
    }
    delete[] pl;
    dims_out[0] = dims[0]; dims_out[1] = dims[1]; dims_out[2] = dims[2];
    return 0;
}
