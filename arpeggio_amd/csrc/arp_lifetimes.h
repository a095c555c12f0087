// arp_lifetimes.h — contact lifetimes over the models of an ensemble, reduced on the device.
//
// The persistence table (arp_persist.h) says in what FRACTION of the F resident models a topology pair (a, b) has a record.  It
// ignores that the models are an ordered axis — for a trajectory streamed through arp_set_models, model f is time.  A pair present
// in models 0 ... 49 of 100 and a pair that flickers on every second model both have n_models = 50.  This table says how LONG a
// contact lasts and how often it forms and breaks: per pair the INTERVALS of its presence — maximal stretches of participating
// models in which consecutive models differ by at most gap + 1 — counted, with the longest one, its start, the sum of their
// spans (span = f_end - f_start + 1: bridged holes count), and the spans of the first and of the last interval, which make two
// chunk tables of one trajectory merge exactly (arpeggio_amd/lifetimes.py).  Every column is an integer.
//
// Which records take part is a launch argument: (sift & sift_any) != 0 and bit ctype of ctype_mask set (the predicate of
// arp_filter.h).  Rows are the pairs with at least one participating record.
//
// Shape (that of the persistence table):
//   k_lifetimes_rekey   record p -> key a << (bbits + fbits) | b << fbits | f, payload table_payload (arp_runs.h), class 0 — or,
//                       when it does not take part, the all-ones key and class TABLE_LEFT_OUT in its slot, as in arp_respair.h
//                       and for its reason: such records trail the last run, no run begins on them (k_runs_count), and the host
//                       needs no second wait.  An atom-atom record has a < b <= n - 1 < 2^bbits, so the a field of a real key is
//                       never all ones: no real key is all ones in the sorted bits, the left-out records sort strictly last, and
//                       — unlike enqueue_residue_rekey, whose pairs may be (r, r) — no tie bit is needed.
//   (radix passes of arp_sort.h over the 2 bbits + fbits bits of the key)
//   k_runs_count / k_runs_scan / k_runs_starts (arp_runs.h, shift fbits): a run = one pair, its records ascending in f, ONE
//   record per model (the bag holds a pair of a model once)
//   k_lifetimes_reduce  one wave per row, 64 consecutive sorted records per step.  Only the keys are read: f is their low fbits
//                       bits and a left-out record is the all-ones key.  A lane is an interval HEAD when it is the run's first
//                       record or when its f exceeds the f before it by more than gap + 1 (lane 0 of a later step: the carried
//                       last f of the step before).  One ballot of heads per step; an interval that ends inside the step ends
//                       on the lane below the next head above its own (__ffsll on the masked ballot), and its span comes from
//                       a __shfl of that lane's f.  The interval still open at a step's end travels to the next step as
//                       wave-uniform state — its start and the last f seen — and is closed at the next head or at the run's
//                       end.  A step in which no interval ends (the common one: contacts mostly persist) costs three ballots
//                       and four shuffles; one in which some do adds two butterflies over the lanes, a sum of spans and a
//                       maximum of (span, earliest start).  No float, no LDS, no atomics; every trip count is wave-uniform.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "arp_runs.h"

struct LifetimesArgs {
    // the bag of the last pass, in the order the pass left it
    const int* ci;
    const int* cj;
    const float* d_in;
    const uint16_t* s_in;
    const uint8_t* ct_in;
    long long k;             // records
    uint32_t n;              // atoms of the topology (ids of model f: [f n, (f + 1) n))
    int bbits, fbits;        // key = a << (bbits + fbits) | b << fbits | f
    uint32_t sift_any, ctype_mask;      // a record takes part when (sift & sift_any) != 0 and bit ctype of ctype_mask is set
    uint32_t gap;            // models of absence tolerated inside an interval (<= 65534)
    // re-keyed records: written by k_lifetimes_rekey, read (sorted) by everything after the radix passes
    unsigned long long* key;
    unsigned long long* val;
    const int* row_start;    // [U + 1]: first record of row r; row_start[U] = k (RunArgs)
    long long U;
    // the table, one column after the other (LIFETIMES_TABLE)
    int* t_a;
    int* t_b;
    uint16_t* t_nmodels;
    int* t_first;
    int* t_last;
    uint16_t* t_nintervals;
    uint16_t* t_longest;
    int* t_longest_start;
    uint16_t* t_head;
    uint16_t* t_tail;
    uint32_t* t_span_sum;
};

__global__ __launch_bounds__(256) void k_lifetimes_rekey(LifetimesArgs A) {
    for (long long p = (long long)blockIdx.x * blockDim.x + threadIdx.x; p < A.k; p += (long long)gridDim.x * blockDim.x) {
        const uint32_t sf = A.s_in[p], ct = A.ct_in[p];
        const bool part = (sf & A.sift_any) != 0u && ((A.ctype_mask >> (ct & 7u)) & 1u) != 0u;
        const uint32_t i = (uint32_t)A.ci[p], j = (uint32_t)A.cj[p];
        const uint32_t f = i / A.n;                  // (a pair never crosses models: j lies in the same model)
        const uint32_t base = f * A.n;
        A.key[p] = part ? ((unsigned long long)(i - base) << (A.bbits + A.fbits)) | ((unsigned long long)(j - base) << A.fbits) | (unsigned long long)f
                        : ~0ull;
        A.val[p] = part ? table_payload(A.d_in[p], sf, ct, 0ull) : TABLE_LEFT_OUT << TABLE_CLASS_SHIFT;
    }
}

// The intervals of a row that are closed so far, on every lane alike.  Intervals close in time order, and `longest` is replaced
// only by a strictly larger span: on a tie the earliest start stays.
struct LifetimesRow {
    uint32_t n_int, longest, lstart, head, sum;
};
__device__ __forceinline__ void lifetimes_close(LifetimesRow& r, uint32_t start, uint32_t span) {
    if (r.n_int == 0u) r.head = span;
    ++r.n_int;
    r.sum += span;
    if (span > r.longest) { r.longest = span; r.lstart = start; }
}

__global__ __launch_bounds__(256) void k_lifetimes_reduce(LifetimesArgs A) {
    const int lane = threadIdx.x & 63;
    const long long waves = (long long)gridDim.x * (blockDim.x >> 6);
    const unsigned long long fmask = (1ull << A.fbits) - 1ull, bmask = (1ull << A.bbits) - 1ull;
    const uint32_t reach = A.gap + 1u;               // consecutive present models of one interval differ by at most this
    for (long long row = (long long)blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6); row < A.U; row += waves) {
        // (the last row's range also holds the left-out records that trail it: invalid lanes below)
        const long long s = A.row_start[row], e = A.row_start[row + 1];
        const unsigned long long k0 = A.key[s];
        LifetimesRow r{0u, 0u, 0u, 0u, 0u};
        uint32_t models = 0;
        // the open interval: wave-uniform.  Its first model and the last model seen
        bool open = false;
        uint32_t c_start = 0, c_last = 0;
        for (long long q = s; q < e; q += 64) {      // (wave-uniform trip count)
            const unsigned long long key = q + lane < e ? A.key[q + lane] : ~0ull;
            const bool valid = key != ~0ull;         // (valid lanes are a prefix: the left-out records sort last)
            const int nv = __popcll(__ballot(valid));
            if (nv == 0) break;
            models += (uint32_t)nv;
            const uint32_t f = valid ? (uint32_t)(key & fmask) : 0u;
            // ---- heads: a lane whose f lies beyond the reach of the f before it (lane 0: of the carried last f)
            const uint32_t up = __shfl_up(f, 1);
            const uint32_t fp = lane == 0 ? c_last : up;
            const bool head = valid && ((lane == 0 && !open) || f - fp > reach);
            const unsigned long long hb = __ballot(head);
            const bool cont = open && !(hb & 1ull);  // the open interval goes on in this step's first lanes
            if (open && !cont) lifetimes_close(r, c_start, c_last - c_start + 1u);      // ... or it ended with the step before
            // ---- the intervals that end inside this step: each begins on a lane of `starts` and ends below the next head
            const unsigned long long starts = hb | 1ull;
            const unsigned long long above = hb & ~((2ull << lane) - 1ull);      // (lane 63: 2 << 63 wraps to 0, the mask to none)
            const bool closes = ((starts >> lane) & 1ull) && above != 0ull;
            const int end = closes ? __ffsll((long long)above) - 2 : lane;
            const uint32_t f_end = __shfl(f, end);
            const uint32_t f_start = (lane == 0 && cont) ? c_start : f;
            const uint32_t span = closes ? f_end - f_start + 1u : 0u;
            const unsigned long long cm = __ballot(closes);
            if (cm) {                                // (wave-uniform)
                // all of them at once: their number, the sum of their spans, and the largest span with the earliest start —
                // the maximum of span << 32 | ~start
                uint32_t sum = span;
                uint32_t b_span = span, b_inv = closes ? ~f_start : 0u;
#pragma unroll
                for (int o = 32; o > 0; o >>= 1) {
                    sum += __shfl_xor(sum, o);
                    const uint32_t o_span = __shfl_xor(b_span, o), o_inv = __shfl_xor(b_inv, o);
                    if (o_span > b_span || (o_span == b_span && o_inv > b_inv)) { b_span = o_span; b_inv = o_inv; }
                }
                if (r.n_int == 0u) r.head = __shfl(span, __ffsll((long long)cm) - 1);
                r.n_int += (uint32_t)__popcll(cm);
                r.sum += sum;
                if (b_span > r.longest) { r.longest = b_span; r.lstart = ~b_inv; }
            }
            // ---- the step's last interval stays open
            const int ls = 63 - __clzll((long long)starts);
            const uint32_t f_ls = __shfl(f, ls);
            c_start = (ls == 0 && cont) ? c_start : f_ls;
            c_last = __shfl(f, nv - 1);
            open = true;
        }
        // the run ends: its last interval closes (a run begins on a kept record, so there is one)
        const uint32_t tail = c_last - c_start + 1u;
        lifetimes_close(r, c_start, tail);
        if (lane == 0) {
            A.t_a[row] = (int)(k0 >> (A.bbits + A.fbits));
            A.t_b[row] = (int)((k0 >> A.fbits) & bmask);
            A.t_nmodels[row] = (uint16_t)models;
            A.t_first[row] = (int)(k0 & fmask);
            A.t_last[row] = (int)c_last;
            A.t_nintervals[row] = (uint16_t)r.n_int;
            A.t_longest[row] = (uint16_t)r.longest;
            A.t_longest_start[row] = (int)r.lstart;
            A.t_head[row] = (uint16_t)r.head;
            A.t_tail[row] = (uint16_t)tail;
            A.t_span_sum[row] = r.sum;
        }
    }
}
