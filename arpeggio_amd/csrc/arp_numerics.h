// arp_numerics.h — device arithmetic of the hot path, written so that every
// rounding step matches the reference's NumPy expressions (DESIGN.md "Arithmetic
// model").  This translation unit is compiled with -ffp-contract=off: the only
// fused operations are the explicit fma() calls.
//
//   np.dot / np.linalg.norm on float32[3]: float32 products, float64 accumulation,
//       one rounding to float32 (OpenBLAS sdot tail loop), float32 sqrt.
//   np.dot / np.linalg.norm on float64[3]: fma(z,z',fma(y,y',x*x')), float64 sqrt.
//   NumPy scalar expressions (utils.py:712-745): one rounding per operation.
//   float32 (op) Python float: the Python float is cast to float32 first (NEP 50).
#pragma once
#include <hip/hip_runtime.h>

#define ARP_PI 3.141592653589793  // np.pi

namespace num {

struct d3 { double x, y, z; };
struct f3 { float x, y, z; };

__device__ __forceinline__ d3 to_d3(f3 v) { return {(double)v.x, (double)v.y, (double)v.z}; }
__device__ __forceinline__ d3 sub(d3 a, d3 b) { return {a.x - b.x, a.y - b.y, a.z - b.z}; }
__device__ __forceinline__ f3 sub(f3 a, f3 b) { return {a.x - b.x, a.y - b.y, a.z - b.z}; }

// np.dot(a, b), float32[3]
__device__ __forceinline__ float dot(f3 a, f3 b) {
    float p0 = a.x * b.x, p1 = a.y * b.y, p2 = a.z * b.z;
    double acc = 0.0;
    acc += (double)p0;
    acc += (double)p1;
    acc += (double)p2;
    return (float)acc;
}
// np.dot(a, b), float64[3]
__device__ __forceinline__ double dot(d3 a, d3 b) {
    double acc = a.x * b.x;
    acc = fma(a.y, b.y, acc);
    acc = fma(a.z, b.z, acc);
    return acc;
}
__device__ __forceinline__ float norm(f3 v) { return sqrtf(dot(v, v)); }
__device__ __forceinline__ double norm(d3 v) { return sqrt(dot(v, v)); }

// Bio.PDB.kdtrees membership test: float64 sum of squares, no fusion.
__device__ __forceinline__ double dist2_kd(d3 a, d3 b) {
    double dx = a.x - b.x, dy = a.y - b.y, dz = a.z - b.z;
    double r = dx * dx;
    r += dy * dy;
    r += dz * dz;
    return r;
}

// utils.get_angle (utils.py:696-745), all-float64 operands
__device__ __forceinline__ double get_angle(d3 a, d3 b, d3 c) {
    d3 v1 = sub(a, b), v2 = sub(c, b);
    double m1 = sqrt(v1.x * v1.x + v1.y * v1.y + v1.z * v1.z);
    d3 n1 = {v1.x / m1, v1.y / m1, v1.z / m1};
    double m2 = sqrt(v2.x * v2.x + v2.y * v2.y + v2.z * v2.z);
    d3 n2 = {v2.x / m2, v2.y / m2, v2.z / m2};
    double res = n1.x * n2.x + n1.y * n2.y + n1.z * n2.z;
    double ang = acos(res);
    if (isnan(ang)) ang = ARP_PI;  // utils.py:741-743
    return ang;
}

// utils.get_angle with three float32 points (is_xbond, utils.py:174).
// nan_pi is set when the NaN -> np.pi substitution fired (np.pi is a Python float).
__device__ __forceinline__ float get_angle(f3 a, f3 b, f3 c, bool& nan_pi) {
    f3 v1 = sub(a, b), v2 = sub(c, b);
    float m1 = sqrtf(v1.x * v1.x + v1.y * v1.y + v1.z * v1.z);
    f3 n1 = {v1.x / m1, v1.y / m1, v1.z / m1};
    float m2 = sqrtf(v2.x * v2.x + v2.y * v2.y + v2.z * v2.z);
    f3 n2 = {v2.x / m2, v2.y / m2, v2.z / m2};
    float res = n1.x * n2.x + n1.y * n2.y + n1.z * n2.z;
    float ang = acosf(res);
    nan_pi = isnan(ang);
    return ang;
}

// utils.get_angle(nbr f32, halogen f32, hydrogen f64) (utils.py:151):
// v1 stays float32, v2 and the dot product are float64.
__device__ __forceinline__ double get_angle_mixed(f3 a, f3 b, d3 c) {
    f3 v1 = sub(a, b);
    d3 v2 = sub(c, to_d3(b));
    float m1 = sqrtf(v1.x * v1.x + v1.y * v1.y + v1.z * v1.z);
    f3 n1 = {v1.x / m1, v1.y / m1, v1.z / m1};
    double m2 = sqrt(v2.x * v2.x + v2.y * v2.y + v2.z * v2.z);
    d3 n2 = {v2.x / m2, v2.y / m2, v2.z / m2};
    double res = (double)n1.x * n2.x + (double)n1.y * n2.y + (double)n1.z * n2.z;
    double ang = acos(res);
    if (isnan(ang)) ang = ARP_PI;
    return ang;
}

// The cosines get_angle / get_angle_mixed hand to acos: the same operation sequences, without the acos.
// A DECISION at a threshold angle must not hang on the last bit of an acos implementation (the device library's differs from
// glibc's and NumPy's there: one weak hydrogen bond in 2 688 seam cases of tests/test_sift_edges.py), so inside the bands the
// reference's cosine is compared with the last double whose arccosine still passes — constants found by bisection on glibc's
// acos and NumPy's arccos, which agree on all four (tests/test_sift_edges.py pins them against both).
__device__ __forceinline__ double cos_angle(d3 a, d3 b, d3 c) {
    d3 v1 = sub(a, b), v2 = sub(c, b);
    double m1 = sqrt(v1.x * v1.x + v1.y * v1.y + v1.z * v1.z);
    d3 n1 = {v1.x / m1, v1.y / m1, v1.z / m1};
    double m2 = sqrt(v2.x * v2.x + v2.y * v2.y + v2.z * v2.z);
    d3 n2 = {v2.x / m2, v2.y / m2, v2.z / m2};
    return n1.x * n2.x + n1.y * n2.y + n1.z * n2.z;
}
__device__ __forceinline__ double cos_angle_mixed(f3 a, f3 b, d3 c) {
    f3 v1 = sub(a, b);
    d3 v2 = sub(c, to_d3(b));
    float m1 = sqrtf(v1.x * v1.x + v1.y * v1.y + v1.z * v1.z);
    f3 n1 = {v1.x / m1, v1.y / m1, v1.z / m1};
    double m2 = sqrt(v2.x * v2.x + v2.y * v2.y + v2.z * v2.z);
    d3 n2 = {v2.x / m2, v2.y / m2, v2.z / m2};
    return (double)n1.x * n2.x + (double)n1.y * n2.y + (double)n1.z * n2.z;
}
#define ARP_COS_LAST_GE_1_57 0x1.a181296fadffap-11      // the largest double c with acos(c) >= 1.57
#define ARP_COS_LAST_GE_2_27 (-0x1.49870aeb9c1fep-1)    //                                    >= 2.27
#define ARP_COS_LAST_GE_0_52 0x1.bc52cba71d363p-1       //                                    >= 0.52
#define ARP_COS_FIRST_LE_2_62 (-0x1.bbeaed2abc536p-1)   // the smallest double c with acos(c) <= 2.62
// acos(res) >= a_min as the reference decides it, NaN -> pi included (|res| > 1 or NaN passes); cos_last = the constant of a_min
__device__ __forceinline__ bool angle_ge_exact(double res, double cos_last) { return !(res > cos_last && res <= 1.0); }
// 0.52 <= acos(res) <= 2.62 (NaN -> pi fails the upper bound)
__device__ __forceinline__ bool angle_in_exact(double res) { return res <= ARP_COS_LAST_GE_0_52 && res >= ARP_COS_FIRST_LE_2_62; }

// ---- decision shortcuts ---------------------------------------------------------------------------
// The reference decides "angle >= a_min" via normalise / dot / acos (2 sqrt, 6 divisions and an acos
// per hydrogen).  cosA = (v1.v2) / sqrt(|v1|^2 |v2|^2) is the same quantity up to ~1e-15 (1e-7 when one
// vector went through float32, utils.py:151), so away from the threshold by a margin delta the decision
// can be taken on squared quantities alone; the exact sequence above runs only inside the margin, when a
// vector has zero length (NaN -> pi, utils.py:741-743) or when |cosA| is within 1e-12 of 1 (rounding can
// push the reference's cosine past 1, which also ends in the NaN -> pi substitution).
__device__ __forceinline__ bool cos_le(double dot, double q, double t) {  // cosA <= t ?
    return (t >= 0) ? (dot <= 0 || dot * dot <= t * t * q) : (dot <= 0 && dot * dot >= t * t * q);
}
__device__ __forceinline__ bool cos_ge(double dot, double q, double t) {  // cosA >= t ?
    return (t >= 0) ? (dot >= 0 && dot * dot >= t * t * q) : (dot >= 0 || dot * dot <= t * t * q);
}
// 1: angle(a,b,c) >= a_min surely; 0: surely not; -1: run the exact test.  c_min = cos(a_min).
__device__ __forceinline__ int angle_ge_fast(d3 a, d3 b, d3 c, double c_min, double delta) {
    const d3 v1 = sub(a, b), v2 = sub(c, b);
    const double dot_ = v1.x * v2.x + v1.y * v2.y + v1.z * v2.z;
    const double q = (v1.x * v1.x + v1.y * v1.y + v1.z * v1.z) * (v2.x * v2.x + v2.y * v2.y + v2.z * v2.z);
    if (!(q > 0.0) || !(dot_ * dot_ < (1.0 - 2e-12) * q)) return -1;
    if (cos_le(dot_, q, c_min - delta)) return 1;
    if (cos_ge(dot_, q, c_min + delta)) return 0;
    return -1;
}
// 1: a_lo <= angle(a,b,c) <= a_hi surely; 0: surely not; -1: exact.  c_lo = cos(a_lo) > c_hi = cos(a_hi).
__device__ __forceinline__ int angle_in_fast(d3 a, d3 b, d3 c, double c_lo, double c_hi, double delta) {
    const d3 v1 = sub(a, b), v2 = sub(c, b);
    const double dot_ = v1.x * v2.x + v1.y * v2.y + v1.z * v2.z;
    const double q = (v1.x * v1.x + v1.y * v1.y + v1.z * v1.z) * (v2.x * v2.x + v2.y * v2.y + v2.z * v2.z);
    if (!(q > 0.0) || !(dot_ * dot_ < (1.0 - 2e-12) * q)) return -1;
    if (cos_le(dot_, q, c_lo - delta) && cos_ge(dot_, q, c_hi + delta)) return 1;
    if (cos_ge(dot_, q, c_lo + delta) || cos_le(dot_, q, c_hi - delta)) return 0;
    return -1;
}
// 1: sqrt(s) <= thr surely (s = exact sum of squares, thr2 = thr * thr); 0: surely not; -1: take the sqrt
__device__ __forceinline__ int dist_le_fast(double s, double thr2) {
    if (s <= thr2 * (1.0 - 1e-14)) return 1;
    if (s >= thr2 * (1.0 + 1e-14)) return 0;
    return -1;
}
#define ARP_COS_1_57 0.0007963267107332633
#define ARP_COS_2_27 (-0.6436084187135406)
#define ARP_COS_0_52 0.8678191796776499
#define ARP_COS_2_62 (-0.8670267214458024)

// degrees + "signed" folding, utils.py:656-660 / 689-693, then abs() at the call site
__device__ __forceinline__ double fold_deg(double rad) {
    if (rad > ARP_PI / 2) rad = rad - ARP_PI;
    return fabs(rad * 180 / ARP_PI);
}
__device__ __forceinline__ float fold_deg(float rad) {
    if (rad > (float)(ARP_PI / 2)) rad = rad - (float)ARP_PI;
    float t = rad * 180.0f;
    return fabsf(t / (float)ARP_PI);
}

// The cosine utils.group_angle / group_group_angle hand to arccos (utils.py:646, 677): dot / (norm * norm), the operand types as in
// the reference.  The REPORTED angle of a ring / amide record is fold_deg(acos(c)) by the device library; every DECISION on a folded
// angle is taken on c itself (fold_le below), for the reason given at cos_angle above: at the cosine 0x1p-1 glibc folds acos to
// 60.00000000000001 and the device library to 59.99999999999999, and the float32 acosf differs about 30 degrees
// (tests/test_plane_edges.py, profiles/plane_edges.md).
__device__ __forceinline__ double group_cos(d3 normal, d3 point) { return dot(normal, point) / (norm(normal) * norm(point)); }
__device__ __forceinline__ float group_cos(f3 normal, f3 point) { return dot(normal, point) / (norm(normal) * norm(point)); }
// float32 normal against a float64 vector: the dot promotes, norm(normal) stays float32
__device__ __forceinline__ double group_cos(f3 normal, d3 other) { return dot(to_d3(normal), other) / ((double)norm(normal) * norm(other)); }

// Per cut the two cosines that bound `abs(folded degrees of arccos(c)) <= cut` as glibc's acos / acosf decide it: the smallest c that
// still passes without the fold (rad <= pi / 2) and the largest that still passes through it (rad - pi).  Found by bisection and pinned
// by tests/test_plane_edges.py::test_fold_cosines_are_the_last_that_pass, monotonic for 10 000 values either side.
#define ARP_FOLD_COS_30_POS 0x1.bb67ae8584cabp-1
#define ARP_FOLD_COS_30_NEG (-0x1.bb67ae8584caap-1)
#define ARP_FOLD_COS_60_POS 0x1.0000000000001p-1
#define ARP_FOLD_COS_60_NEG (-0x1.0000000000000p-1)
#define ARP_FOLD_COSF_30_POS 0x1.bb67aep-1f
#define ARP_FOLD_COSF_30_NEG (-0x1.bb67b2p-1f)
// folded angle of c <= cut; NaN and |c| > 1 (arccos NaN) fail, as every comparison with NaN does in the reference
__device__ __forceinline__ bool fold_le(double c, double c_pos, double c_neg) { return (c >= c_pos && c <= 1.0) || (c <= c_neg && c >= -1.0); }
__device__ __forceinline__ bool fold_le(float c, float c_pos, float c_neg) { return (c >= c_pos && c <= 1.0f) || (c <= c_neg && c >= -1.0f); }
// the angle is a number (a folded angle never exceeds 90, so this is also `<= 90`)
__device__ __forceinline__ bool fold_num(double c) { return c >= -1.0 && c <= 1.0; }
__device__ __forceinline__ bool fold_num(float c) { return c >= -1.0f && c <= 1.0f; }
// folded angle of c > 30 (false for NaN): the test of the amide loops, I:1282 / I:1363
__device__ __forceinline__ bool fold_gt_30(double c) { return fold_num(c) && !fold_le(c, ARP_FOLD_COS_30_POS, ARP_FOLD_COS_30_NEG); }
__device__ __forceinline__ bool fold_gt_30(float c) { return fold_num(c) && !fold_le(c, ARP_FOLD_COSF_30_POS, ARP_FOLD_COSF_30_NEG); }

// interactions.py:1127-1148 on the cosines of the dihedral and of theta (9 = '' when an angle is NaN)
__device__ __forceinline__ int pp_class(double cos_dihedral, double cos_theta) {
    const bool dn = fold_num(cos_dihedral), tn = fold_num(cos_theta);
    const bool d_lo = fold_le(cos_dihedral, ARP_FOLD_COS_30_POS, ARP_FOLD_COS_30_NEG);
    const bool d_mid = fold_le(cos_dihedral, ARP_FOLD_COS_60_POS, ARP_FOLD_COS_60_NEG);
    const bool t_lo = fold_le(cos_theta, ARP_FOLD_COS_30_POS, ARP_FOLD_COS_30_NEG);
    const bool t_mid = fold_le(cos_theta, ARP_FOLD_COS_60_POS, ARP_FOLD_COS_60_NEG);
    if (!dn || !tn) return 9;
    const int row = d_lo ? 0 : d_mid ? 3 : 6;
    return row + (t_lo ? 0 : t_mid ? 1 : 2);
}

}  // namespace num
