// arp_models.h — F models (coordinate sets) of ONE topology, resident as a batch partition with one structure per model
// (arp_set_topology / arp_set_models).  The reference keeps the first model only (P:67-69: del st[1:]); here every model
// is evaluated in one pass, each with exactly the arithmetic of its own single-structure run:
//   k_models_expand   the F copies of the kept topology blob, indices shifted by the model's offsets
//   k_models_boxes    bounding boxes per model (blob header, batch partition)
// Ring and amide geometry per (model, ring / amide) and the ring residues per model are the kernels of arp_prepare.h, which take
// the model count and the models' places; their arithmetic is written there only.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "arp_prepare.h"

// What k_models_expand reads (the kept topology: one structure of n atoms ...) and writes (the resident blob of F models).
struct ModelsExpand {
    int F, n, nres, nbond, nh, nring, namide;
    const float* xyz_in;                      // [F][n][3] float32, the models' coordinates
    // topology
    const double2* t_rad;
    const uint16_t* t_tmask;
    const uint16_t* t_flags;
    const uint16_t* t_rad_idx;
    const int* t_res_id;
    const uint8_t* t_res_flags;
    const int* t_res_prev;
    const int* t_res_next;
    const int* t_bond_off;
    const int* t_bond_idx;
    const int* t_h_off;
    const int* t_sb_nbr;
    const int* t_am_res;
    const double2* t_rad_tab;
    // expanded blob
    float4* xyz4;
    double2* rad;
    uint16_t* tmask;
    uint16_t* flags;
    uint16_t* rad_idx;
    int* res_id;
    uint8_t* res_flags;
    int* res_prev;
    int* res_next;
    int* bond_off;
    int* bond_idx;
    int* h_off;
    int* sb_nbr;
    int* ring_res;
    int* am_res;
    double2* rad_tab;
};
#define MODELS_EXPAND_SEGMENTS 6

__device__ __forceinline__ int shift_index(int v, int by) { return v >= 0 ? v + by : v; }   // (-1 = none stays -1)

// One grid-stride launch; blockIdx.y picks the segment: 0 per-atom arrays (F n items), 1 per-residue (F nres), 2 bonds
// (F nbond), 3 rings (F nring: residue -1 until k_ring_residue), 4 amides (F namide), 5 the radius table.  The
// coordinates go out as one 16-byte float4 per atom (w = 0, as arp_blob_fill writes them) and the radius pairs as one
// 16-byte double2; the narrower per-atom columns start at model offsets f n that are not multiples of four, so they move
// element by element.  The models' hydrogen coordinates are no part of this: they are copied into the blob as they came.
__global__ __launch_bounds__(256) void k_models_expand(ModelsExpand E) {
    const int seg = blockIdx.y;
    const int stride = gridDim.x * blockDim.x;
    const int t0 = blockIdx.x * blockDim.x + threadIdx.x;
    if (seg == 0) {
        const int total = E.F * E.n;
        for (int k = t0; k < total; k += stride) {
            const int f = k / E.n, i = k - f * E.n;
            const float* p = E.xyz_in + 3 * (size_t)k;
            E.xyz4[k] = make_float4(p[0], p[1], p[2], 0.0f);
            E.rad[k] = E.t_rad[i];
            E.tmask[k] = E.t_tmask[i];
            E.flags[k] = E.t_flags[i];
            E.rad_idx[k] = E.t_rad_idx[i];
            E.res_id[k] = E.t_res_id[i] + f * E.nres;
            E.sb_nbr[k] = shift_index(E.t_sb_nbr[i], f * E.n);
            E.bond_off[k] = E.t_bond_off[i] + f * E.nbond;
            E.h_off[k] = E.t_h_off[i] + f * E.nh;
        }
        if (t0 == 0) { E.bond_off[total] = E.F * E.nbond; E.h_off[total] = E.F * E.nh; }
    } else if (seg == 1) {
        const int total = E.F * E.nres;
        for (int k = t0; k < total; k += stride) {
            const int f = k / E.nres, i = k - f * E.nres;
            E.res_flags[k] = E.t_res_flags[i];
            E.res_prev[k] = shift_index(E.t_res_prev[i], f * E.nres);
            E.res_next[k] = shift_index(E.t_res_next[i], f * E.nres);
        }
    } else if (seg == 2) {
        const int total = E.F * E.nbond;
        for (int k = t0; k < total; k += stride) {
            const int f = k / E.nbond, i = k - f * E.nbond;
            E.bond_idx[k] = E.t_bond_idx[i] + f * E.n;
        }
    } else if (seg == 3) {
        const int total = E.F * E.nring;
        for (int k = t0; k < total; k += stride) E.ring_res[k] = -1;
    } else if (seg == 4) {
        const int total = E.F * E.namide;
        for (int k = t0; k < total; k += stride) {
            const int f = k / E.namide, i = k - f * E.namide;
            E.am_res[k] = shift_index(E.t_am_res[i], f * E.nres);
        }
    } else {
        for (int k = t0; k < RAD_TABLE; k += stride) E.rad_tab[k] = E.t_rad_tab[k];
    }
}

// min / max that keep a NaN once they have met one (a model with a non-finite coordinate gets a non-finite box, which the
// host turns into a failed validation)
__device__ __forceinline__ double lo_keep_nan(double a, double b) { return (a != a) ? a : ((b != b || b < a) ? b : a); }
__device__ __forceinline__ double hi_keep_nan(double a, double b) { return (a != a) ? a : ((b != b || b > a) ? b : a); }

// One block per model: out[18 f ...] = atoms lo xyz, hi xyz (float32 widened to double, as arp_blob_fill), ring centres lo,
// hi, amide centres lo, hi.  An empty set gives +inf / -inf, which the host replaces by 0 as arp_blob_fill does.
__global__ __launch_bounds__(256) void k_models_boxes(int n, int nring, int namide, const float4* __restrict__ xyz,
                                                      const double* __restrict__ ring_c, const float* __restrict__ am_c,
                                                      double* __restrict__ out) {
    const int f = blockIdx.x;
    double v[18];
#pragma unroll
    for (int q = 0; q < 3; ++q)
        for (int k = 0; k < 3; ++k) { v[6 * q + k] = INFINITY; v[6 * q + 3 + k] = -INFINITY; }
    auto take = [&](int q, double x, double y, double z) {
        v[6 * q] = lo_keep_nan(v[6 * q], x); v[6 * q + 1] = lo_keep_nan(v[6 * q + 1], y); v[6 * q + 2] = lo_keep_nan(v[6 * q + 2], z);
        v[6 * q + 3] = hi_keep_nan(v[6 * q + 3], x); v[6 * q + 4] = hi_keep_nan(v[6 * q + 4], y); v[6 * q + 5] = hi_keep_nan(v[6 * q + 5], z);
    };
    for (int i = threadIdx.x; i < n; i += blockDim.x) {
        const float4 p = xyz[(size_t)f * n + i];
        take(0, (double)p.x, (double)p.y, (double)p.z);
    }
    for (int r = threadIdx.x; r < nring; r += blockDim.x) {
        const size_t k = 3 * ((size_t)f * nring + r);
        take(1, ring_c[k], ring_c[k + 1], ring_c[k + 2]);
    }
    for (int a = threadIdx.x; a < namide; a += blockDim.x) {
        const size_t k = 3 * ((size_t)f * namide + a);
        take(2, (double)am_c[k], (double)am_c[k + 1], (double)am_c[k + 2]);
    }
    for (int o = 32; o > 0; o >>= 1)
#pragma unroll
        for (int q = 0; q < 18; ++q) {
            const double w = __shfl_xor(v[q], o);
            v[q] = (q % 6) < 3 ? lo_keep_nan(v[q], w) : hi_keep_nan(v[q], w);
        }
    __shared__ double s_v[4][18];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    if (lane == 0) {
#pragma unroll
        for (int q = 0; q < 18; ++q) s_v[wave][q] = v[q];
    }
    __syncthreads();
    if (threadIdx.x < 18) {
        const int q = threadIdx.x;
        double r = s_v[0][q];
        for (int w = 1; w < (int)(blockDim.x >> 6); ++w) r = (q % 6) < 3 ? lo_keep_nan(r, s_v[w][q]) : hi_keep_nan(r, s_v[w][q]);
        out[18 * (size_t)f + q] = r;
    }
}
