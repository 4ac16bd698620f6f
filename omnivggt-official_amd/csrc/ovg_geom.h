// The small primitives shared by the exact-arithmetic geometry units (point clouds, rendering, consistency, neighbour searches,
// normals, registration, planes, fusion, rasterisation, depth scoring, map geometry, mesh operations): finite tests, float order
// keys, wave and workgroup scans and reductions, the ordered tile compaction, the fixed-order float64 fold, the symmetric 3 x 3 Jacobi solve, a hash finaliser, the
// lock-free union-find, and the hosts' argument helpers.
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

// order-preserving u32 of a finite f32 and back: an unsigned integer min / max over the keys is the float min / max, exact and order-free
OVG_DEV uint32_t order_key32(float f) {
  const uint32_t u = __float_as_uint(f);
  return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}
OVG_DEV float key_value32(uint32_t k) { return __uint_as_float((k & 0x80000000u) ? (k & 0x7FFFFFFFu) : ~k); }

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

// order-preserving compaction of one tile of keep bytes by a workgroup of THREADS (ovg_mesh_simplify, ovg_mesh_select): entry i of tile
// blockIdx.x lands at offsets[blockIdx.x] + (kept entries before it in the tile); the order inside a tile is j-major (j * THREADS +
// thread), which is the index order. emit(i, pos) for every kept entry. Every thread calls it, once per kernel.
template <int THREADS, int TILE, class Emit>
OVG_DEV void compact_tile(const uint8_t* keep, int64_t n, const int64_t* offsets, Emit emit) {
  constexpr int J = TILE / THREADS, W = THREADS / 64;
  static_assert(J * W == 64 && J <= 32, "the group counts are scanned by one wave, the kept bits live in one word");
  __shared__ uint32_t cnt[J * W];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int64_t base = (int64_t)blockIdx.x * TILE;
  uint32_t bits = 0;
#pragma unroll
  for (int j = 0; j < J; ++j) {
    const int64_t i = base + (int64_t)j * THREADS + threadIdx.x;
    const bool k = i < n && keep[i];
    bits |= (uint32_t)k << j;
    const uint64_t bal = __ballot(k);
    if (lane == 0) cnt[j * W + wave] = __popcll(bal);
  }
  __syncthreads();
  if (wave == 0) {                                     // 64 groups: one exclusive scan in wave 0
    const uint64_t v = cnt[lane];
    cnt[lane] = (uint32_t)(wave_incl_scan(v) - v);
  }
  __syncthreads();
  const int64_t off = offsets[blockIdx.x];
  const uint64_t below = (1ull << lane) - 1ull;
#pragma unroll
  for (int j = 0; j < J; ++j) {
    const bool k = (bits >> j) & 1u;
    const uint64_t bal = __ballot(k);
    if (!k) continue;
    emit(base + (int64_t)j * THREADS + threadIdx.x, off + cnt[j * W + wave] + __popcll(bal & below));
  }
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
// the lock-free union-find of ovg_cluster (csrc/ovg_radius.hip: cl_degree, cl_link, cl_flatten) and of ovg_mesh_topology
// (csrc/ovg_meshops.hip: mo_faces hooks, mt_finish flattens). What follows was written for ovg_cluster and names its launches; the
// other user keeps the same discipline: parent[x] = x before the first hook, hooks in one launch, the final finds in a later one.
// ---------------------------------------------------------------------------------------------------------------------------------
// The union-find. parent[x] of a core point x, read and written in cl_link / cl_flatten ONLY through relaxed agent-scope atomics (a
// plain load may be served from a CU's L1 or another XCD's L2 and go stale). Writes are of two kinds: a HOOK, the 32-bit
// compare-and-swap parent[hi]: hi -> lo with lo < hi, and a HALVING, the atomic min of parent[x] with a value read from parent[parent[x]].
// Invariants, by induction over the writes in the order the memory system performs them on each slot (cl_degree left parent[x] = x):
//   (a) parent[x] <= x. A hook stores lo < hi; a min never raises a slot.
//   (b) a slot only ever decreases: a hook replaces hi by lo < hi, a min is a min.
//   (c) every value ever stored in parent[x] is a member of x's component (of the graph of rule 5). A hook stores lo, a point reached
//       by following parents from b, where a, b are neighbours and hi was reached from a: by (c) for the slots followed, lo ~ b ~ a ~ hi.
//       A halving stores a value once held by parent[p], p once held by parent[x]: a member of p's component, which is x's.
//   (d) the parents form a forest: a non-root slot holds a strictly smaller index, so following parents descends and ends, after at most
//       x steps, at an r with parent[r] == r; a hook succeeds only on a slot that still holds its own index, a root at that instant,
//       and so hangs hi's whole tree under lo: under the root of another tree, or (when lo has been hooked itself since it was
//       read) under an inner node of one -- one tree fewer either way; a halving moves x under a former ancestor g, which by (b)
//       and (d) is still in x's tree. Trees only ever merge.
// After cl_link has ended every neighbour pair of core points is in one tree: cl_unite returns only after a successful hook between
// the two trees or after both walks ended at the same root. With (c) the trees are exactly the components, and by (a) along the path
// a tree's root is <= every member and is a member: the component's LOWEST index, whatever the schedule.
// Termination: nothing waits. cl_find descends by at least one index per step. A failed compare-and-swap returns the slot's new
// value, < hi by (a) and (b): another thread's hook or halving made progress, and this thread's cursor moves down to that value. So
// the two cursors of a cl_unite only move down from a0, b0 < n: find steps plus failed swaps < 2 n, and the step budget 4 n + 4
// (every outer round spends at least two steps) is never met by correct code. A value outside [0, x], or a spent budget, sets
// OVG_CL_INTERNAL and leaves: a bug ends as an error, never as a hang, and no index outside [0, n) is ever followed.
OVG_DEV int32_t cl_ld(int32_t* a) { return __hip_atomic_load(a, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }

// the root of x's tree at some instant during the call, halving the path on the way; -1 on a broken invariant or a spent budget
OVG_DEV int32_t cl_find(int32_t* parent, int32_t x, uint64_t& budget) {
  while (budget) {
    --budget;
    const int32_t p = cl_ld(parent + x);
    if (p == x) return x;
    if ((uint32_t)p > (uint32_t)x) return -1;
    const int32_t g = cl_ld(parent + p);
    if ((uint32_t)g > (uint32_t)p) return -1;
    if (g != p) __hip_atomic_fetch_min(parent + x, g, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    x = p;
  }
  return -1;
}

OVG_DEV bool cl_unite(int32_t* parent, int32_t a, int32_t b, uint64_t budget) {
  for (;;) {
    a = cl_find(parent, a, budget);
    b = cl_find(parent, b, budget);
    if ((a | b) < 0) return false;
    if (a == b) return true;
    const int32_t hi = a > b ? a : b, lo = a > b ? b : a;
    int32_t seen = hi;
    if (__hip_atomic_compare_exchange_strong(parent + hi, &seen, lo, __ATOMIC_RELAXED, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)) return true;
    if ((uint32_t)seen >= (uint32_t)hi) return false;
    a = seen, b = lo;                                  // hi is no root any more: go on from what it points to now
  }
}

// ---------------------------------------------------------------------------------------------------------------------------------
// host: what every entry checks of its arguments
// ---------------------------------------------------------------------------------------------------------------------------------
inline bool al(const void* q, uintptr_t a) { return (reinterpret_cast<uintptr_t>(q) & (a - 1)) == 0; }   // a null pointer is aligned
inline int64_t round256(int64_t b) { return (b + 255) / 256 * 256; }
inline bool size_ok(int64_t n) { return n >= 1 && n < (1ll << 31); }                                      // a count that fits int32
