// Plane segmentation by RANSAC (ovg_plane_hypotheses, ovg_plane_score, ovg_plane_select, ovg_plane_mask, ovg_plane_fit): seeded
// three-point hypotheses in float64, their inlier counts over the whole cloud, the winner, its mask and a least-squares refit from
// ovg_align_moments' sums. The hot path is the score: H hypotheses x n points on the vector ALU in ovg_nn.hip's shape -- a grid of
// (hypothesis tiles) x (point splits); a thread keeps kPlanesPerThread planes and their counters in registers, the workgroup stages
// one point tile after the other in LDS (groups of four points as x[4] y[4] z[4]: three 16-byte reads of an address all lanes share,
// a broadcast without bank conflicts) and walks it with no cross-lane traffic; a split adds its counters with one integer atomic
// per hypothesis. Integer sums do not depend on the order of arrival: identical bytes run to run and for every split count.
#include "ovg_geom.h"

// tests/plane_twin.py restates the residual in numpy float32 and the hypotheses in float64, one rounding per operation: no fused
// multiply-adds in this unit (build.py compiles it with -ffp-contract=off as well)
#pragma clang fp contract(off)

namespace {

constexpr int kThreads = 128;
constexpr int kPlanesPerThread = OVG_PLANE_HYP_TILE / kThreads;
constexpr int kPointTile = OVG_PLANE_POINT_TILE;
constexpr int kTargetWorkgroups = 2048;              // auto splits: 256 CUs x 4 SIMDs x 2 waves each, at 2 waves per workgroup
constexpr int kMaxSplits = 65535;                    // gridDim.y
constexpr int kFlat = 256;                           // threads of the one-item-per-thread launches
constexpr int kMaskPerThread = 4;                    // points per thread of plane_mask: one atomic per 1024 points
constexpr uint32_t kNanBits = 0x7FC00000u;

static_assert(kPlanesPerThread * kThreads == OVG_PLANE_HYP_TILE && kPointTile % kThreads == 0 && kPointTile % 4 == 0, "tile shapes");

OVG_DEV uint64_t mix64(uint64_t z) {
  z += 0x9E3779B97F4A7C15ull;
  z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
  z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
  return z ^ (z >> 31);
}

// the orientation of a unit normal: with an axis and d != 0 so that d > 0, else the component of largest magnitude positive
OVG_DEV bool flip_normal(const double (&e)[3], bool has_axis, double d) {
  if (has_axis && d != 0.0) return d < 0.0;
  double big = e[0];
  if (fabs(e[1]) > fabs(big)) big = e[1];
  if (fabs(e[2]) > fabs(big)) big = e[2];
  return big < 0.0;
}

__global__ __launch_bounds__(kFlat) void plane_hypotheses(ovg_plane_hypotheses_params p) {
  const int64_t h = (int64_t)blockIdx.x * kFlat + threadIdx.x;
  if (h >= p.H) return;
  int32_t idx[3];
  double pt[3][3];
  bool ok = true;
#pragma unroll
  for (int j = 0; j < 3; ++j) {
    const uint64_t pos = ((mix64(p.seed + 3ull * (uint64_t)h + (uint64_t)j) >> 32) * (uint64_t)p.m) >> 32;   // < m < 2^31
    const int32_t i = p.candidates ? p.candidates[pos] : (int32_t)pos;
    idx[j] = i;
    pt[j][0] = pt[j][1] = pt[j][2] = 0.0;
    if (i < 0 || (int64_t)i >= p.n) {
      ok = false;
      continue;
    }
    const float* s = p.points + 3 * (int64_t)i;
    const float x = s[0], y = s[1], z = s[2];
    if (!finite3(x, y, z) || (p.valid && p.valid[i] == 0)) ok = false;
    pt[j][0] = (double)x, pt[j][1] = (double)y, pt[j][2] = (double)z;
  }
  int32_t* oi = p.index + 3 * h;
  oi[0] = idx[0], oi[1] = idx[1], oi[2] = idx[2];
  if (idx[0] == idx[1] || idx[0] == idx[2] || idx[1] == idx[2]) ok = false;
  float out[4];
  out[0] = out[1] = out[2] = out[3] = __uint_as_float(kNanBits);
  if (ok) {
    const double u[3] = {pt[1][0] - pt[0][0], pt[1][1] - pt[0][1], pt[1][2] - pt[0][2]};
    const double v[3] = {pt[2][0] - pt[0][0], pt[2][1] - pt[0][1], pt[2][2] - pt[0][2]};
    const double n[3] = {u[1] * v[2] - u[2] * v[1], u[2] * v[0] - u[0] * v[2], u[0] * v[1] - u[1] * v[0]};
    const double l2 = (n[0] * n[0] + n[1] * n[1]) + n[2] * n[2];
    const double uu = (u[0] * u[0] + u[1] * u[1]) + u[2] * u[2], vv = (v[0] * v[0] + v[1] * v[1]) + v[2] * v[2];
    if (l2 > (OVG_PLANE_COLLINEAR_EPS * uu) * vv) {
      const double len = sqrt(l2);
      double e[3] = {n[0] / len, n[1] / len, n[2] / len};
      double d = 0.0;
      bool keep = true;
      if (p.axis) {
        d = (e[0] * (double)p.axis[0] + e[1] * (double)p.axis[1]) + e[2] * (double)p.axis[2];
        keep = fabs(d) >= (double)p.min_abs_cos;                                 // false for a NaN
      }
      if (keep) {
        if (flip_normal(e, p.axis != nullptr, d)) e[0] = -e[0], e[1] = -e[1], e[2] = -e[2];
        const double w = -((e[0] * pt[0][0] + e[1] * pt[0][1]) + e[2] * pt[0][2]);
        out[0] = (float)e[0], out[1] = (float)e[1], out[2] = (float)e[2], out[3] = (float)w;
      }
    }
  }
  float* o = p.planes + 4 * h;
  o[0] = out[0], o[1] = out[1], o[2] = out[2], o[3] = out[3];
}

__global__ __launch_bounds__(kFlat) void plane_zero32(int32_t* __restrict__ x, int32_t n) {
  const uint32_t i = blockIdx.x * kFlat + threadIdx.x;                       // n < 2^31: no wrap in unsigned arithmetic
  if (i < (uint32_t)n) x[i] = 0;
}

// one group of four points against the thread's planes
OVG_DEV void score_group(const f32x4 px, const f32x4 py, const f32x4 pz, float t, const float (&nx)[kPlanesPerThread],
                         const float (&ny)[kPlanesPerThread], const float (&nz)[kPlanesPerThread], const float (&w)[kPlanesPerThread],
                         int32_t (&cnt)[kPlanesPerThread]) {
#pragma unroll
  for (int r = 0; r < 4; ++r) {
#pragma unroll
    for (int k = 0; k < kPlanesPerThread; ++k) {
      const float e = ((nx[k] * px[r] + ny[k] * py[r]) + nz[k] * pz[r]) + w[k];
      cnt[k] += fabsf(e) <= t ? 1 : 0;                                       // false for a NaN: unusable points and void planes
    }
  }
}

// blockIdx.x: hypothesis tile, blockIdx.y: split (point tiles [y * tiles_per_split, (y + 1) * tiles_per_split) below ntiles)
__global__ __launch_bounds__(kThreads) void plane_score(const float* __restrict__ points, const uint8_t* __restrict__ valid,
                                                        const float* __restrict__ planes, int32_t n, int32_t H, float t, int32_t ntiles,
                                                        int32_t tiles_per_split, int32_t* __restrict__ count) {
  __shared__ __attribute__((aligned(16))) float lds[3 * kPointTile];
  const int32_t h0 = (int32_t)blockIdx.x * OVG_PLANE_HYP_TILE;               // < H < 2^31
  float nx[kPlanesPerThread], ny[kPlanesPerThread], nz[kPlanesPerThread], w[kPlanesPerThread];
  int32_t hi[kPlanesPerThread], cnt[kPlanesPerThread];
#pragma unroll
  for (int k = 0; k < kPlanesPerThread; ++k) {
    // h0 + OVG_PLANE_HYP_TILE may pass 2^31: compare the offset inside the tile, which is small
    const int32_t off = k * kThreads + (int32_t)threadIdx.x;
    const bool in = off < H - h0;
    hi[k] = in ? h0 + off : -1;
    nx[k] = ny[k] = nz[k] = w[k] = __uint_as_float(kNanBits);                // a slot past H: the void plane
    if (in) {
      const float* q = planes + 4 * (int64_t)hi[k];
      nx[k] = q[0], ny[k] = q[1], nz[k] = q[2], w[k] = q[3];
    }
    cnt[k] = 0;
  }
  const int32_t t_first = (int32_t)blockIdx.y * tiles_per_split;
  const int32_t t_end = min(t_first + tiles_per_split, ntiles);
  for (int32_t tile = t_first; tile < t_end; ++tile) {
    const int32_t j0 = tile * kPointTile;                                    // < n < 2^31
    __syncthreads();                                                         // the previous tile has been read by every wave
#pragma unroll
    for (int s = 0; s < kPointTile / kThreads; ++s) {
      const int32_t jl = s * kThreads + (int32_t)threadIdx.x;                // position in the tile
      float x = __uint_as_float(kNanBits), y = 0.0f, z = 0.0f;               // padding and unusable points: NaN
      if (jl < n - j0) {
        const int64_t j = (int64_t)j0 + jl;
        const float* q = points + 3 * j;
        const float qx = q[0], qy = q[1], qz = q[2];
        if (finite3(qx, qy, qz) && (!valid || valid[j] != 0)) x = qx, y = qy, z = qz;
      }
      float* g = lds + 12 * (jl >> 2) + (jl & 3);
      g[0] = x, g[4] = y, g[8] = z;
    }
    __syncthreads();
    const f32x4* g = reinterpret_cast<const f32x4*>(lds);
#pragma unroll 2
    for (int q = 0; q < kPointTile / 4; ++q) score_group(g[3 * q], g[3 * q + 1], g[3 * q + 2], t, nx, ny, nz, w, cnt);
  }
#pragma unroll
  for (int k = 0; k < kPlanesPerThread; ++k) {
    // count starts as zeros (plane_zero32 of the same call); an integer sum is the same in every order of arrival
    if (hi[k] >= 0 && cnt[k] != 0) atomicAdd(count + hi[k], cnt[k]);
  }
}

// one workgroup: thread t looks at the hypotheses t, t + kFlat, ... in ascending order with a strict "larger than", then the
// largest key (count << 32) | ~h over the workgroup: the largest count, the lowest h among equals
__global__ __launch_bounds__(kFlat) void plane_select(ovg_plane_select_params p) {
  __shared__ unsigned long long keys[kFlat];
  unsigned long long best = 0ull;                                            // count 0 at h = 2^32 - 1: below every real key
  for (int64_t h = threadIdx.x; h < p.H; h += kFlat) {
    const int32_t c = p.count[h];
    const unsigned long long key = ((unsigned long long)(uint32_t)(c > 0 ? c : 0) << 32) | (uint32_t)~(uint32_t)h;
    best = key > best ? key : best;
  }
  keys[threadIdx.x] = best;
  __syncthreads();
#pragma unroll
  for (int s = kFlat / 2; s > 0; s >>= 1) {
    if ((int)threadIdx.x < s) keys[threadIdx.x] = keys[threadIdx.x] > keys[threadIdx.x + s] ? keys[threadIdx.x] : keys[threadIdx.x + s];
    __syncthreads();
  }
  if (threadIdx.x != 0) return;
  const unsigned long long key = keys[0];
  const int32_t c = (int32_t)(key >> 32), h = (int32_t)~(uint32_t)key;       // H >= 1: thread 0 saw h = 0, so h is a hypothesis
  float q[4] = {0.0f, 0.0f, 0.0f, 0.0f};
  bool found = c >= p.min_inliers;
  if (found) {
    const float* s = p.planes + 4 * (int64_t)h;
    found = finite_f32(s[0]) && finite_f32(s[1]) && finite_f32(s[2]) && finite_f32(s[3]);
    if (found) q[0] = s[0], q[1] = s[1], q[2] = s[2], q[3] = s[3];
  }
  *p.best = found ? h : -1;
  p.plane[0] = q[0], p.plane[1] = q[1], p.plane[2] = q[2], p.plane[3] = q[3];
  *p.best_count = c;
  *p.status = found ? 0 : OVG_PLANE_NONE;
}

__global__ void plane_zero64(int64_t* x) { *x = 0; }

__global__ __launch_bounds__(kFlat) void plane_mask(ovg_plane_mask_params p) {
  __shared__ int32_t part[kFlat / 64];
  const bool none = p.gate && (*p.gate & OVG_PLANE_NONE) != 0;
  const float nx = p.plane[0], ny = p.plane[1], nz = p.plane[2], w = p.plane[3], t = p.threshold;
  const int64_t base = (int64_t)blockIdx.x * (kFlat * kMaskPerThread) + threadIdx.x;
  int32_t cnt = 0;
#pragma unroll
  for (int r = 0; r < kMaskPerThread; ++r) {
    const int64_t i = base + (int64_t)r * kFlat;
    if (i >= p.n) continue;
    const float* s = p.points + 3 * i;
    const float x = s[0], y = s[1], z = s[2];
    const bool usable = !none && finite3(x, y, z) && (!p.valid || p.valid[i] != 0);
    const float e = usable ? ((nx * x + ny * y) + nz * z) + w : __uint_as_float(kNanBits);
    const bool in = fabsf(e) <= t;                                           // false for a NaN
    p.inlier[i] = in ? 1 : 0;
    if (p.distance) p.distance[i] = e;
    cnt += in ? 1 : 0;
  }
  const int32_t total = block_reduce<kFlat>(cnt, part, IntSum());
  if (threadIdx.x == 0 && total != 0) atomicAdd(reinterpret_cast<unsigned long long*>(p.out_count), (unsigned long long)total);
}

__global__ __launch_bounds__(64) void plane_fit(ovg_plane_fit_params p) {
  if (threadIdx.x != 0) return;
  const int64_t n = *p.count;
  double m[OVG_ALIGN_SUMS], cen[3] = {0.0, 0.0, 0.0};
  bool finite = true;
  for (int k = 0; k < OVG_ALIGN_SUMS; ++k) m[k] = p.sums[k], finite = finite && finite_f64(m[k]);
  if (p.centre) {
    for (int k = 0; k < 6; ++k) finite = finite && finite_f64(p.centre[k]);
    for (int k = 0; k < 3; ++k) cen[k] = p.centre[k];
  }
  int32_t status = 0;
  if (n < 3) status |= OVG_PLANE_FEW;
  if (!finite) status |= OVG_PLANE_NOT_FINITE;
  double rms = 0.0, eig[3] = {0.0, 0.0, 0.0};
  if (status == 0) {
    const double dn = (double)n;
    double xx = m[6] - (m[0] * m[0]) / dn, xy = m[7] - (m[0] * m[1]) / dn, xz = m[8] - (m[0] * m[2]) / dn;
    double yy = m[10] - (m[1] * m[1]) / dn, yz = m[11] - (m[1] * m[2]) / dn, zz = m[14] - (m[2] * m[2]) / dn;
    const double g[3] = {m[0] / dn + cen[0], m[1] / dn + cen[1], m[2] / dn + cen[2]};
    double v0[3], v1[3], v2[3], e[3];
    jacobi_sweeps3(xx, xy, xz, yy, yz, zz, v0, v1, v2, OVG_KNN_NORMALS_SWEEPS);
    // the smallest eigenvalue and its unit eigenvector (ovg_knn_normals' rule); of the two others the larger and the smaller
    const double lam[3] = {xx, yy, zz};
    int kmin;
    const double low = jacobi_smallest(xx, yy, zz, v0, v1, v2, kmin, e);
    const int ka = kmin == 0 ? 1 : 0, kb = kmin == 2 ? 1 : 2;
    const double mid = lam[ka] < lam[kb] ? lam[ka] : lam[kb], top = lam[ka] < lam[kb] ? lam[kb] : lam[ka];
    if (!(mid > OVG_PLANE_SPREAD_EPS * top)) {
      status |= OVG_PLANE_NO_SPREAD;
    } else {
      double d = 0.0;
      if (p.axis) d = (e[0] * (double)p.axis[0] + e[1] * (double)p.axis[1]) + e[2] * (double)p.axis[2];
      if (flip_normal(e, p.axis != nullptr, d)) e[0] = -e[0], e[1] = -e[1], e[2] = -e[2];
      const double w = -((e[0] * g[0] + e[1] * g[1]) + e[2] * g[2]);
      const float q[4] = {(float)e[0], (float)e[1], (float)e[2], (float)w};
      if (finite_f32(q[0]) && finite_f32(q[1]) && finite_f32(q[2]) && finite_f32(q[3]) && finite_f64(low) && finite_f64(top)) {
        p.plane[0] = q[0], p.plane[1] = q[1], p.plane[2] = q[2], p.plane[3] = q[3];
        // a scatter matrix is positive semi-definite: a negative smallest eigenvalue is rounding, reported as 0
        rms = sqrt((low > 0.0 ? low : 0.0) / dn);
        eig[0] = low, eig[1] = mid, eig[2] = top;
      } else {
        status |= OVG_PLANE_NOT_FINITE;
      }
    }
  }
  if (p.out_rms) *p.out_rms = rms;
  if (p.out_eigen) p.out_eigen[0] = eig[0], p.out_eigen[1] = eig[1], p.out_eigen[2] = eig[2];
  if (p.status) *p.status = status;
}

bool threshold_ok(float t) { return t >= 0.0f && t <= 3.4028234663852886e38f; }     // false for NaN and +inf

}  // namespace

extern "C" int ovg_plane_hypotheses(const ovg_plane_hypotheses_params* p, void* stream) {
  if (!p || !p->points || !p->planes || !p->index) return OVG_E_ARG;
  if (!size_ok(p->n) || !size_ok(p->H)) return OVG_E_ARG;
  if (p->candidates ? !size_ok(p->m) : (p->m != 0 && p->m != p->n)) return OVG_E_ARG;
  if (!(p->min_abs_cos >= 0.0f && p->min_abs_cos <= 1.0f) || (!p->axis && p->min_abs_cos != 0.0f)) return OVG_E_ARG;
  if (!al(p->points, 4) || !al(p->candidates, 4) || !al(p->axis, 4) || !al(p->planes, 4) || !al(p->index, 4)) return OVG_E_ARG;
  hipStream_t st = static_cast<hipStream_t>(stream);
  ovg_plane_hypotheses_params q = *p;
  if (!q.candidates) q.m = q.n;
  OVG_LAUNCH(plane_hypotheses, dim3((unsigned)((q.H + kFlat - 1) / kFlat)), dim3(kFlat), 0, st, q);
  OVG_CHECK_LAUNCH();
  return OVG_OK;
}

extern "C" int ovg_plane_score(const ovg_plane_score_params* p, void* stream) {
  if (!p || !p->points || !p->planes || !p->count) return OVG_E_ARG;
  if (!size_ok(p->n) || !size_ok(p->H) || !threshold_ok(p->threshold) || p->splits < 0) return OVG_E_ARG;
  if (!al(p->points, 4) || !al(p->planes, 4) || !al(p->count, 4)) return OVG_E_ARG;
  hipStream_t st = static_cast<hipStream_t>(stream);
  const int32_t n = (int32_t)p->n, H = (int32_t)p->H;
  const int32_t htiles = (int32_t)((p->H + OVG_PLANE_HYP_TILE - 1) / OVG_PLANE_HYP_TILE);   // <= 2^22: fits gridDim.x
  const int32_t ntiles = (int32_t)((p->n + kPointTile - 1) / kPointTile);
  int32_t splits = p->splits > 0 ? p->splits : (kTargetWorkgroups + htiles - 1) / htiles;
  splits = splits < ntiles ? splits : ntiles;
  splits = splits < kMaxSplits ? splits : kMaxSplits;
  const int32_t per = (ntiles + splits - 1) / splits;
  splits = (ntiles + per - 1) / per;                                        // no empty split
  OVG_LAUNCH(plane_zero32, dim3((unsigned)((p->H + kFlat - 1) / kFlat)), dim3(kFlat), 0, st, p->count, H);
  OVG_CHECK_LAUNCH();
  OVG_LAUNCH(plane_score, dim3((unsigned)htiles, (unsigned)splits), dim3(kThreads), 0, st, p->points, p->valid, p->planes, n, H, p->threshold,
             ntiles, per, p->count);
  OVG_CHECK_LAUNCH();
  return OVG_OK;
}

extern "C" int ovg_plane_select(const ovg_plane_select_params* p, void* stream) {
  if (!p || !p->count || !p->planes || !p->best || !p->plane || !p->best_count || !p->status) return OVG_E_ARG;
  if (!size_ok(p->H) || p->min_inliers < 3) return OVG_E_ARG;
  if (!al(p->count, 4) || !al(p->planes, 4) || !al(p->best, 4) || !al(p->plane, 4) || !al(p->best_count, 4) || !al(p->status, 4)) return OVG_E_ARG;
  hipStream_t st = static_cast<hipStream_t>(stream);
  OVG_LAUNCH(plane_select, dim3(1), dim3(kFlat), 0, st, *p);
  OVG_CHECK_LAUNCH();
  return OVG_OK;
}

extern "C" int ovg_plane_mask(const ovg_plane_mask_params* p, void* stream) {
  if (!p || !p->points || !p->plane || !p->inlier || !p->out_count) return OVG_E_ARG;
  if (!size_ok(p->n) || !threshold_ok(p->threshold)) return OVG_E_ARG;
  if (!al(p->points, 4) || !al(p->plane, 4) || !al(p->gate, 4) || !al(p->distance, 4) || !al(p->out_count, 8)) return OVG_E_ARG;
  hipStream_t st = static_cast<hipStream_t>(stream);
  OVG_LAUNCH(plane_zero64, dim3(1), dim3(1), 0, st, p->out_count);
  OVG_CHECK_LAUNCH();
  const int64_t per_block = (int64_t)kFlat * kMaskPerThread;
  OVG_LAUNCH(plane_mask, dim3((unsigned)((p->n + per_block - 1) / per_block)), dim3(kFlat), 0, st, *p);
  OVG_CHECK_LAUNCH();
  return OVG_OK;
}

extern "C" int ovg_plane_fit(const ovg_plane_fit_params* p, void* stream) {
  if (!p || !p->count || !p->sums || !p->plane) return OVG_E_ARG;
  if (!al(p->count, 8) || !al(p->sums, 8) || !al(p->centre, 8) || !al(p->axis, 4) || !al(p->plane, 4) || !al(p->out_rms, 8) ||
      !al(p->out_eigen, 8) || !al(p->status, 4))
    return OVG_E_ARG;
  hipStream_t st = static_cast<hipStream_t>(stream);
  OVG_LAUNCH(plane_fit, dim3(1), dim3(64), 0, st, *p);
  OVG_CHECK_LAUNCH();
  return OVG_OK;
}
