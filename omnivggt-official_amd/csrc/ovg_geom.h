// The small primitives shared by the exact-arithmetic geometry units (point clouds, rendering, consistency, neighbour searches,
// normals, registration, planes, fusion, rasterisation, depth scoring, map geometry): finite tests, wave and workgroup scans and
// reductions, the fixed-order float64 fold, the symmetric 3 x 3 Jacobi solve, a hash finaliser, and the hosts' argument helpers.
// Every one of them is part of a bit-exactness contract with a numpy twin in tests/*_twin.py: a change here changes all its users at
// once, which is the point. Units that include this are compiled with -ffp-contract=off (build.py); the pragma below covers the
// functions of this header whatever the order of the including unit's own pragma and its #include.
#pragma once
#include <math.h>
#include "ovg_common.h"

#pragma clang fp contract(off)

// ---------------------------------------------------------------------------------------------------------------------------------
// finite tests on the exponent bits: false for NaN and both infinities, true for everything else, whatever the denormal mode
// ---------------------------------------------------------------------------------------------------------------------------------
OVG_DEV bool finite_f32(float f) { return (__float_as_uint(f) & 0x7F800000u) != 0x7F800000u; }
OVG_DEV bool finite_f64(double d) { return (__double_as_longlong(d) & 0x7FF0000000000000ll) != 0x7FF0000000000000ll; }
OVG_DEV bool finite3(float x, float y, float z) { return finite_f32(x) && finite_f32(y) && finite_f32(z); }
OVG_DEV bool finite3(const float* __restrict__ p) { return finite3(p[0], p[1], p[2]); }

// murmur3's 64-bit finaliser
OVG_DEV uint64_t mix_murmur64(uint64_t h) {
  h ^= h >> 33; h *= 0xFF51AFD7ED558CCDull; h ^= h >> 33; h *= 0xC4CEB9FE1A85EC53ull; h ^= h >> 33;
  return h;
}

// ---------------------------------------------------------------------------------------------------------------------------------
// integer scans and reductions. Integer sums, minima and maxima do not depend on the order: identical bytes run to run
// ---------------------------------------------------------------------------------------------------------------------------------
template <typename T> OVG_DEV T wave_incl_scan(T v) {
  const int lane = threadIdx.x & 63;
#pragma unroll
  for (int d = 1; d < 64; d <<= 1) {
    const T o = __shfl_up(v, d, 64);
    if (lane >= d) v += o;
  }
  return v;
}

// exclusive rank of this thread's `c` items among the workgroup's, in thread order; total: the workgroup's sum. wsum: THREADS / 64
// words of LDS. Every thread calls it.
template <int THREADS> OVG_DEV uint32_t block_excl_scan(uint32_t c, uint32_t* wsum, uint32_t& total) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const uint32_t incl = wave_incl_scan(c);
  __syncthreads();                                                        // wsum may still be read from an earlier call
  if (lane == 63) wsum[wave] = incl;
  __syncthreads();
  uint32_t before = 0;
  total = 0;
  for (int w = 0; w < THREADS / 64; ++w) {
    if (w < wave) before += wsum[w];
    total += wsum[w];
  }
  return before + incl - c;
}

// dst[i] = src[0] + ... + src[i - 1] for i < n by ONE workgroup of 1024 threads, 1024 entries per round with the running total
// carried from round to round; src == dst is fine. -> the grand total (thread 0 reads it; a caller that scans again puts a
// __syncthreads() in front of the next call). Every thread calls it.
template <typename T> OVG_DEV T count_scan(const T* src, T* dst, int64_t n) {
  __shared__ T wsum[16];
  __shared__ T carry;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  if (threadIdx.x == 0) carry = 0;
  __syncthreads();
  for (int64_t b0 = 0; b0 < n; b0 += 1024) {
    const int64_t b = b0 + threadIdx.x;
    const T v = b < n ? src[b] : 0;
    const T incl = wave_incl_scan(v);
    if (lane == 63) wsum[wave] = incl;
    __syncthreads();
    T excl = carry + incl - v;
    for (int w = 0; w < wave; ++w) excl += wsum[w];
    if (b < n) dst[b] = excl;
    __syncthreads();
    if (threadIdx.x == 1023) carry = excl + v;
    __syncthreads();
  }
  return carry;
}

struct IntSum { template <typename T> OVG_DEV T operator()(T a, T b) const { return a + b; } };
struct IntMin { template <typename T> OVG_DEV T operator()(T a, T b) const { return b < a ? b : a; } };
struct IntMax { template <typename T> OVG_DEV T operator()(T a, T b) const { return a < b ? b : a; } };

// op over the 64 lanes of a wave: lane 0 leaves with the result
template <typename T, class Op> OVG_DEV T wave_reduce(T v, Op op) {
#pragma unroll
  for (int d = 32; d > 0; d >>= 1) v = op(v, (T)__shfl_down(v, d, 64));
  return v;
}

// op over a workgroup of THREADS: every thread leaves with the result. red: THREADS / 64 entries of LDS. Every thread calls it.
template <int THREADS, typename T, class Op> OVG_DEV T block_reduce(T v, T* red, Op op) {
  v = wave_reduce(v, op);
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
  __syncthreads();
  T t = red[0];
#pragma unroll
  for (int w = 1; w < THREADS / 64; ++w) t = op(t, red[w]);
  return t;
}

// ---------------------------------------------------------------------------------------------------------------------------------
// the float64 fold of a workgroup of THREADS = 256 in a FIXED order (include/omnivggt_hip.h, ovg_align_moments): v[l] = v[l] + v[l + s]
// for s = 32 .. 1 inside every wave, then (w0 + w1) + (w2 + w3). Thread k < NSUMS leaves with sum k, thread NSUMS + k with count k.
// Every thread calls it.
// ---------------------------------------------------------------------------------------------------------------------------------
template <int THREADS, int NSUMS, int NCOUNTS>
OVG_DEV void fold_block(double (&v)[NSUMS], long long (&cnt)[NCOUNTS], int64_t* out_counts, double* out_sums) {
  constexpr int kWaves = THREADS / 64;
  static_assert(kWaves == 4, "the combine below is (w0 + w1) + (w2 + w3)");
  __shared__ double part[kWaves][NSUMS];
  __shared__ long long part_n[kWaves][NCOUNTS];
#pragma unroll
  for (int s = 32; s > 0; s >>= 1) {
#pragma unroll
    for (int k = 0; k < NSUMS; ++k) v[k] = v[k] + __shfl_down(v[k], s, 64);        // lanes >= 64 - s add their own value: never read below
#pragma unroll
    for (int k = 0; k < NCOUNTS; ++k) cnt[k] += __shfl_down(cnt[k], s, 64);
  }
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  if (lane == 0) {
#pragma unroll
    for (int k = 0; k < NSUMS; ++k) part[wave][k] = v[k];
#pragma unroll
    for (int k = 0; k < NCOUNTS; ++k) part_n[wave][k] = cnt[k];
  }
  __syncthreads();
  if (threadIdx.x < NSUMS) {
    const int k = threadIdx.x;
    out_sums[k] = (part[0][k] + part[1][k]) + (part[2][k] + part[3][k]);
  } else if (threadIdx.x < NSUMS + NCOUNTS) {
    const int k = threadIdx.x - NSUMS;
    out_counts[k] = (int64_t)((part_n[0][k] + part_n[1][k]) + (part_n[2][k] + part_n[3][k]));
  }
}

// ---------------------------------------------------------------------------------------------------------------------------------
// eigenvectors of a symmetric 3 x 3 matrix by cyclic Jacobi rotations in float64 (include/omnivggt_hip.h states the rule of
// ovg_knn_normals and ovg_plane_fit, tests/knn_twin.py and tests/plane_twin.py restate it)
// ---------------------------------------------------------------------------------------------------------------------------------
// one rotation in the (p, q) plane: app, aqq, apq the matrix's entries there, arp / arq the third row's; vp, vq the matching columns
// of the accumulated rotations. theta^2 may overflow to +inf: t becomes 0, the rotation the identity
OVG_DEV void jacobi_rotate(double& app, double& aqq, double& apq, double& arp, double& arq, double (&vp)[3], double (&vq)[3]) {
  if (apq == 0.0) return;
  const double theta = (aqq - app) / (2.0 * apq);
  const double t = (theta >= 0.0 ? 1.0 : -1.0) / (fabs(theta) + sqrt(theta * theta + 1.0));
  const double c = 1.0 / sqrt(t * t + 1.0), s = t * c;
  app = app - t * apq, aqq = aqq + t * apq, apq = 0.0;
  const double rp = c * arp - s * arq, rq = s * arp + c * arq;
  arp = rp, arq = rq;
#pragma unroll
  for (int k = 0; k < 3; ++k) {
    const double a = c * vp[k] - s * vq[k], b = s * vp[k] + c * vq[k];
    vp[k] = a, vq[k] = b;
  }
}

// `sweeps` sweeps over (0, 1), (0, 2), (1, 2): the matrix in place (its diagonal ends as the eigenvalues), v0 .. v2 the columns of
// the accumulated rotations, starting from the identity
OVG_DEV void jacobi_sweeps3(double& xx, double& xy, double& xz, double& yy, double& yz, double& zz, double (&v0)[3], double (&v1)[3],
                            double (&v2)[3], int sweeps) {
  v0[0] = 1.0, v0[1] = 0.0, v0[2] = 0.0, v1[0] = 0.0, v1[1] = 1.0, v1[2] = 0.0, v2[0] = 0.0, v2[1] = 0.0, v2[2] = 1.0;
  for (int s = 0; s < sweeps; ++s) {
    jacobi_rotate(xx, yy, xy, xz, yz, v0, v1);         // (0, 1): the third index is 2
    jacobi_rotate(xx, zz, xz, xy, yz, v0, v2);         // (0, 2): the third index is 1
    jacobi_rotate(yy, zz, yz, xy, xz, v1, v2);         // (1, 2): the third index is 0
  }
}

// -> the smallest diagonal entry, the lowest column on ties; kmin its column and e that column of the rotations, normalised
OVG_DEV double jacobi_smallest(double xx, double yy, double zz, const double (&v0)[3], const double (&v1)[3], const double (&v2)[3],
                               int& kmin, double (&e)[3]) {
  double lam = xx;
  kmin = 0;
  if (yy < lam) lam = yy, kmin = 1;
  if (zz < lam) lam = zz, kmin = 2;
#pragma unroll
  for (int q = 0; q < 3; ++q) e[q] = kmin == 0 ? v0[q] : (kmin == 1 ? v1[q] : v2[q]);
  const double len = sqrt((e[0] * e[0] + e[1] * e[1]) + e[2] * e[2]);
  e[0] = e[0] / len, e[1] = e[1] / len, e[2] = e[2] / len;
  return lam;
}

// ---------------------------------------------------------------------------------------------------------------------------------
// host: what every entry checks of its arguments
// ---------------------------------------------------------------------------------------------------------------------------------
inline bool al(const void* q, uintptr_t a) { return (reinterpret_cast<uintptr_t>(q) & (a - 1)) == 0; }   // a null pointer is aligned
inline int64_t round256(int64_t b) { return (b + 255) / 256 * 256; }
inline bool size_ok(int64_t n) { return n >= 1 && n < (1ll << 31); }                                      // a count that fits int32
