// Registration of point clouds (ovg_align_moments, ovg_align_solve, ovg_align_apply): the float64 pair moments of a correspondence set
// summed in a FIXED order (include/omnivggt_hip.h states it, tests/align_twin.py restates it operation for operation), the rigid /
// similarity transform from them by Horn's quaternion method (a 4 x 4 cyclic Jacobi solve in one thread), and the transform applied.
// The moments are a streaming reduction -- 24 bytes of points, up to 10 of index, masks and gate per pair, and a gather -- bound by
// memory; the order is fixed by giving every thread its pairs, every wave its tree and every tile its slot: no atomics, no spinning.
// The weighted entries (ovg_align_wmoments, ovg_align_wsolve) are the same sums with a weight per pair -- the caller's times a Cauchy
// weight of the residual under a previous transform -- and the same solve with the weight sum in the place of the pair count: the
// robust refits that stitch overlapping chunks of a long sequence. ovg_align_move_maps / _move_cameras carry a chunk's prediction over.
#include "ovg_geom.h"

// the twin is one numpy float64 operation per rounding: no fused multiply-adds in this unit (build.py: -ffp-contract=off)
#pragma clang fp contract(off)

namespace {

constexpr int kThreads = OVG_ALIGN_THREADS;
constexpr int kTile = OVG_ALIGN_TILE;
constexpr int kRounds = kTile / kThreads;
constexpr int kSums = OVG_ALIGN_SUMS;
constexpr int kSlots = OVG_ALIGN_PARTIAL_BYTES / 8;       // a tile's partial: the int64 count, the 18 sums, one slot of padding
static_assert(kRounds >= 1 && kSlots >= kSums + 1, "a tile has pairs and its partial has room");
constexpr int kWSums = OVG_WALIGN_SUMS;
constexpr int kWSlots = OVG_WALIGN_PARTIAL_BYTES / 8;     // the weighted partial: the int64 count, the 20 sums, one slot of padding
static_assert(kWSums == kSums + 2 && kWSlots >= kWSums + 1, "the weighted sums are the 18 sums, W and W^2");

__global__ __launch_bounds__(kThreads) void align_tiles(ovg_align_moments_params p) {
  const int64_t base = (int64_t)blockIdx.x * kTile + threadIdx.x;
  const bool gate = (p.flags & OVG_ALIGN_GATE) != 0;
  double c[6] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
  if (p.centre) {
#pragma unroll
    for (int k = 0; k < 6; ++k) c[k] = p.centre[k];
  }
  double v[kSums];
#pragma unroll
  for (int k = 0; k < kSums; ++k) v[k] = 0.0;
  long long cnt[1] = {0};
#pragma unroll
  for (int r = 0; r < kRounds; ++r) {
    const int64_t i = base + (int64_t)r * kThreads;
    if (i >= p.n) continue;
    const int64_t j = p.index ? (int64_t)p.index[i] : i;
    bool use = j >= 0 && j < p.m;
    if (use && p.source_valid) use = p.source_valid[i] != 0;
    if (use && p.target_valid) use = p.target_valid[j] != 0;
    if (use && gate) use = p.sqdist[i] <= p.max_sqdist;                            // inclusive; false for a NaN
    if (!use) continue;
    const float* ps = p.source + 3 * i;
    const float* qs = p.target + 3 * j;
    const float p0 = ps[0], p1 = ps[1], p2 = ps[2], q0 = qs[0], q1 = qs[1], q2 = qs[2];
    if (!(finite_f32(p0) && finite_f32(p1) && finite_f32(p2) && finite_f32(q0) && finite_f32(q1) && finite_f32(q2))) continue;
    const double a[3] = {(double)p0 - c[0], (double)p1 - c[1], (double)p2 - c[2]};
    const double b[3] = {(double)q0 - c[3], (double)q1 - c[4], (double)q2 - c[5]};
    const double d0 = (double)q0 - (double)p0, d1 = (double)q1 - (double)p1, d2 = (double)q2 - (double)p2;
#pragma unroll
    for (int k = 0; k < 3; ++k) v[k] = v[k] + a[k], v[3 + k] = v[3 + k] + b[k];
#pragma unroll
    for (int rr = 0; rr < 3; ++rr) {
#pragma unroll
      for (int cc = 0; cc < 3; ++cc) v[6 + 3 * rr + cc] = v[6 + 3 * rr + cc] + a[rr] * b[cc];
    }
    v[15] = v[15] + ((a[0] * a[0] + a[1] * a[1]) + a[2] * a[2]);
    v[16] = v[16] + ((b[0] * b[0] + b[1] * b[1]) + b[2] * b[2]);
    v[17] = v[17] + ((d0 * d0 + d1 * d1) + d2 * d2);
    ++cnt[0];
  }
  double* slot = static_cast<double*>(p.ws) + (int64_t)blockIdx.x * kSlots;
  fold_block<kThreads>(v, cnt, reinterpret_cast<int64_t*>(slot), slot + 1);
}

// step 4: one workgroup over the tile partials, thread t the tiles t, t + 256, ... in that order
__global__ __launch_bounds__(kThreads) void align_fold(const double* ws, int64_t tiles, int64_t* out_count, double* out_sums) {
  double v[kSums];
#pragma unroll
  for (int k = 0; k < kSums; ++k) v[k] = 0.0;
  long long cnt[1] = {0};
  for (int64_t g = threadIdx.x; g < tiles; g += kThreads) {
    const double* slot = ws + g * kSlots;
    cnt[0] += *reinterpret_cast<const long long*>(slot);
#pragma unroll
    for (int k = 0; k < kSums; ++k) v[k] = v[k] + slot[1 + k];
  }
  fold_block<kThreads>(v, cnt, out_count, out_sums);
}

// ovg_align_wmoments: the tiles of align_tiles with a weight per pair -- the caller's, times the Cauchy weight of the pair's residual
// under a transform. The centred terms come from the UNMOVED source: the sums always describe the fit source -> target
__global__ __launch_bounds__(kThreads) void walign_tiles(ovg_align_wmoments_params p) {
  const int64_t base = (int64_t)blockIdx.x * kTile + threadIdx.x;
  double c[6] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
  if (p.centre) {
#pragma unroll
    for (int k = 0; k < 6; ++k) c[k] = p.centre[k];
  }
  double T[3][4] = {{1.0, 0.0, 0.0, 0.0}, {0.0, 1.0, 0.0, 0.0}, {0.0, 0.0, 1.0, 0.0}};
  if (p.transform) {
#pragma unroll
    for (int k = 0; k < 12; ++k) T[k >> 2][k & 3] = p.transform[k];
  }
  double dd = 0.0;                                                                   // delta^2, or 0: no reweighting
  if (p.flags & OVG_WALIGN_CAUCHY) {
    const double delta = p.delta_scale * (p.delta ? *p.delta : 1.0);
    if (finite_f64(delta) && delta > 0.0) dd = delta * delta;                        // a square that underflows to 0 reweights nothing either
  }
  double v[kWSums];
#pragma unroll
  for (int k = 0; k < kWSums; ++k) v[k] = 0.0;
  long long cnt[1] = {0};
#pragma unroll
  for (int r = 0; r < kRounds; ++r) {
    const int64_t i = base + (int64_t)r * kThreads;
    if (i >= p.n) continue;
    bool use = true;
    if (p.source_valid) use = p.source_valid[i] != 0;
    if (use && p.target_valid) use = p.target_valid[i] != 0;
    if (!use) continue;
    const float* ps = p.source + 3 * i;
    const float* qs = p.target + 3 * i;
    const float p0 = ps[0], p1 = ps[1], p2 = ps[2], q0 = qs[0], q1 = qs[1], q2 = qs[2];
    if (!(finite_f32(p0) && finite_f32(p1) && finite_f32(p2) && finite_f32(q0) && finite_f32(q1) && finite_f32(q2))) continue;
    double w = 1.0;
    if (p.weight) {
      const float wf = p.weight[i];
      if (!(finite_f32(wf) && wf > 0.0f)) continue;
      w = (double)wf;
    }
    const double x = (double)p0, y = (double)p1, z = (double)p2;
    double mv[3] = {x, y, z};
    if (p.transform) {
#pragma unroll
      for (int k = 0; k < 3; ++k) mv[k] = ((T[k][0] * x + T[k][1] * y) + T[k][2] * z) + T[k][3];
      if (!(finite_f64(mv[0]) && finite_f64(mv[1]) && finite_f64(mv[2]))) continue;
    }
    const double e0 = (double)q0 - mv[0], e1 = (double)q1 - mv[1], e2 = (double)q2 - mv[2];
    const double r2 = (e0 * e0 + e1 * e1) + e2 * e2;
    const double h = dd > 0.0 ? 1.0 / (1.0 + r2 / dd) : 1.0;
    const double W = w * h;
    const double a[3] = {x - c[0], y - c[1], z - c[2]};
    const double b[3] = {(double)q0 - c[3], (double)q1 - c[4], (double)q2 - c[5]};
#pragma unroll
    for (int k = 0; k < 3; ++k) v[k] = v[k] + W * a[k], v[3 + k] = v[3 + k] + W * b[k];
#pragma unroll
    for (int rr = 0; rr < 3; ++rr) {
#pragma unroll
      for (int cc = 0; cc < 3; ++cc) v[6 + 3 * rr + cc] = v[6 + 3 * rr + cc] + (W * a[rr]) * b[cc];
    }
    v[15] = v[15] + W * ((a[0] * a[0] + a[1] * a[1]) + a[2] * a[2]);
    v[16] = v[16] + W * ((b[0] * b[0] + b[1] * b[1]) + b[2] * b[2]);
    v[17] = v[17] + W * r2;
    v[18] = v[18] + W;
    v[19] = v[19] + W * W;
    ++cnt[0];
  }
  double* slot = static_cast<double*>(p.ws) + (int64_t)blockIdx.x * kWSlots;
  fold_block<kThreads>(v, cnt, reinterpret_cast<int64_t*>(slot), slot + 1);
}

__global__ __launch_bounds__(kThreads) void walign_fold(const double* ws, int64_t tiles, int64_t* out_count, double* out_sums) {
  double v[kWSums];
#pragma unroll
  for (int k = 0; k < kWSums; ++k) v[k] = 0.0;
  long long cnt[1] = {0};
  for (int64_t g = threadIdx.x; g < tiles; g += kThreads) {
    const double* slot = ws + g * kWSlots;
    cnt[0] += *reinterpret_cast<const long long*>(slot);
#pragma unroll
    for (int k = 0; k < kWSums; ++k) v[k] = v[k] + slot[1 + k];
  }
  fold_block<kThreads>(v, cnt, out_count, out_sums);
}

// one Jacobi rotation in the (P, Q) plane of the symmetric 4 x 4 matrix A, accumulated into the columns P, Q of V (ovg_knn_normals'
// rotation: theta^2 may overflow to +inf, t becomes 0 and the rotation the identity)
template <int P, int Q> OVG_DEV void jacobi4(double (&A)[4][4], double (&V)[4][4]) {
  const double apq = A[P][Q];
  if (apq == 0.0) return;
  const double theta = (A[Q][Q] - A[P][P]) / (2.0 * apq);
  const double t = (theta >= 0.0 ? 1.0 : -1.0) / (fabs(theta) + sqrt(theta * theta + 1.0));
  const double c = 1.0 / sqrt(t * t + 1.0), s = t * c;
  A[P][P] = A[P][P] - t * apq, A[Q][Q] = A[Q][Q] + t * apq, A[P][Q] = 0.0, A[Q][P] = 0.0;
#pragma unroll
  for (int r = 0; r < 4; ++r) {
    if (r != P && r != Q) {
      const double rp = c * A[r][P] - s * A[r][Q], rq = s * A[r][P] + c * A[r][Q];
      A[r][P] = rp, A[P][r] = rp, A[r][Q] = rq, A[Q][r] = rq;
    }
    const double vp = c * V[r][P] - s * V[r][Q], vq = s * V[r][P] + c * V[r][Q];
    V[r][P] = vp, V[r][Q] = vq;
  }
}

// the solve both entries share (include/omnivggt_hip.h, ovg_align_solve steps 1 .. 5): m the 18 moments, cen the centre they were
// computed with, dn the divisor -- (double)N of ovg_align_solve, the weight sum W of ovg_align_wsolve -- and status what the caller
// found before (few pairs, a non-finite input). -> the status; step, scale (identity, 1 when it is not 0) and resid = the sum of
// the weighted squared residuals AFTER the step, E of ovg_align_wsolve (0 for a degenerate step)
OVG_DEV int32_t solve_step(const double (&m)[kSums], const double (&cen)[6], double dn, int32_t status, bool with_scale, double (&step)[3][4],
                           double& scale, double& resid) {
  scale = 1.0, resid = 0.0;
  if (status == 0) {
    const double var = m[15] - ((m[0] * m[0] + m[1] * m[1]) + m[2] * m[2]) / dn;
    if (!(var > OVG_ALIGN_SPREAD_EPS * m[15])) status |= OVG_ALIGN_NO_SPREAD;
    if (status == 0) {
      double S[3][3];
      for (int r = 0; r < 3; ++r)
        for (int c = 0; c < 3; ++c) S[r][c] = m[6 + 3 * r + c] - m[r] * m[3 + c] / dn;
      double A[4][4], V[4][4];
      A[0][0] = (S[0][0] + S[1][1]) + S[2][2], A[0][1] = S[1][2] - S[2][1], A[0][2] = S[2][0] - S[0][2], A[0][3] = S[0][1] - S[1][0];
      A[1][1] = (S[0][0] - S[1][1]) - S[2][2], A[1][2] = S[0][1] + S[1][0], A[1][3] = S[2][0] + S[0][2];
      A[2][2] = (S[1][1] - S[0][0]) - S[2][2], A[2][3] = S[1][2] + S[2][1];
      A[3][3] = (S[2][2] - S[0][0]) - S[1][1];
      for (int r = 0; r < 4; ++r)
        for (int c = 0; c < 4; ++c) {
          if (c < r) A[r][c] = A[c][r];
          V[r][c] = r == c ? 1.0 : 0.0;
        }
      for (int sweep = 0; sweep < OVG_ALIGN_JACOBI_SWEEPS; ++sweep) {
        jacobi4<0, 1>(A, V), jacobi4<0, 2>(A, V), jacobi4<0, 3>(A, V);
        jacobi4<1, 2>(A, V), jacobi4<1, 3>(A, V), jacobi4<2, 3>(A, V);
      }
      int best = 0;                                                                  // the largest diagonal entry, the lowest column on ties
      for (int k = 1; k < 4; ++k)
        if (A[k][k] > A[best][best]) best = k;
      double w = V[0][best], x = V[1][best], y = V[2][best], z = V[3][best];
      const double len = sqrt(((w * w + x * x) + y * y) + z * z);
      w = w / len, x = x / len, y = y / len, z = z / len;
      const double R[3][3] = {{1.0 - 2.0 * (y * y + z * z), 2.0 * (x * y - w * z), 2.0 * (x * z + w * y)},
                              {2.0 * (x * y + w * z), 1.0 - 2.0 * (x * x + z * z), 2.0 * (y * z - w * x)},
                              {2.0 * (x * z - w * y), 2.0 * (y * z + w * x), 1.0 - 2.0 * (x * x + y * y)}};
      double tr = 0.0;
      for (int r = 0; r < 3; ++r)
        for (int c = 0; c < 3; ++c) tr = tr + R[r][c] * S[c][r];
      if (with_scale) scale = tr / var;
      const double vb = m[16] - ((m[3] * m[3] + m[4] * m[4]) + m[5] * m[5]) / dn;
      resid = with_scale ? vb - (tr * tr) / var : (var + vb) - 2.0 * tr;
      const double ma[3] = {m[0] / dn + cen[0], m[1] / dn + cen[1], m[2] / dn + cen[2]};
      const double mb[3] = {m[3] / dn + cen[3], m[4] / dn + cen[4], m[5] / dn + cen[5]};
      bool ok = finite_f64(scale);
      for (int r = 0; r < 3; ++r) {
        for (int c = 0; c < 3; ++c) step[r][c] = scale * R[r][c], ok = ok && finite_f64(step[r][c]);
        step[r][3] = mb[r] - ((step[r][0] * ma[0] + step[r][1] * ma[1]) + step[r][2] * ma[2]);
        ok = ok && finite_f64(step[r][3]);
      }
      if (!ok) status |= OVG_ALIGN_NOT_FINITE;
    }
  }
  if (status != 0) {
    scale = 1.0, resid = 0.0;
    for (int r = 0; r < 3; ++r)
      for (int c = 0; c < 4; ++c) step[r][c] = r == c ? 1.0 : 0.0;
  }
  return status;
}

__global__ __launch_bounds__(64) void align_solve(ovg_align_solve_params p) {
  if (threadIdx.x != 0) return;
  const int64_t n = *p.count;
  double m[kSums], cen[6] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
  bool finite = true;
  for (int k = 0; k < kSums; ++k) m[k] = p.sums[k], finite = finite && finite_f64(m[k]);
  if (p.centre) {
    for (int k = 0; k < 6; ++k) cen[k] = p.centre[k], finite = finite && finite_f64(cen[k]);
  }
  int32_t status = 0;
  if (n < 3) status |= OVG_ALIGN_FEW_PAIRS;
  if (!finite) status |= OVG_ALIGN_NOT_FINITE;
  const double dn = (double)(n > 0 ? n : 1);
  double step[3][4], scale, resid;
  status = solve_step(m, cen, dn, status, (p.flags & OVG_ALIGN_SCALE) != 0, step, scale, resid);
  double* T = p.transform;
  if (p.flags & OVG_ALIGN_COMPOSE) {
    if (status == 0) {                                                               // an identity step leaves the running transform as it is
      double old[4][4], out[3][4];
      for (int k = 0; k < 16; ++k) old[k >> 2][k & 3] = T[k];
      for (int r = 0; r < 3; ++r)
        for (int c = 0; c < 4; ++c)
          out[r][c] = ((step[r][0] * old[0][c] + step[r][1] * old[1][c]) + step[r][2] * old[2][c]) + step[r][3] * old[3][c];
      for (int r = 0; r < 3; ++r)
        for (int c = 0; c < 4; ++c) T[4 * r + c] = out[r][c];
    }
  } else {
    for (int r = 0; r < 3; ++r)
      for (int c = 0; c < 4; ++c) T[4 * r + c] = step[r][c];
    T[12] = 0.0, T[13] = 0.0, T[14] = 0.0, T[15] = 1.0;
  }
  if (p.out_scale) *p.out_scale = scale;
  if (p.out_rms) *p.out_rms = (n >= 1 && finite_f64(m[17])) ? sqrt(m[17] / dn) : 0.0;
  if (p.out_count) *p.out_count = n;
  if (p.out_status) *p.out_status = status;
}

__global__ __launch_bounds__(64) void walign_solve(ovg_align_wsolve_params p) {
  if (threadIdx.x != 0) return;
  const int64_t n = *p.count;
  double m[kSums], cen[6] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
  bool finite = true;
  for (int k = 0; k < kSums; ++k) m[k] = p.sums[k], finite = finite && finite_f64(m[k]);
  const double W = p.sums[18], W2 = p.sums[19];
  finite = finite && finite_f64(W) && finite_f64(W2);
  if (p.centre) {
    for (int k = 0; k < 6; ++k) cen[k] = p.centre[k], finite = finite && finite_f64(cen[k]);
  }
  const bool weighs = W > 0.0;                                                       // false for a NaN
  int32_t status = 0;
  if (n < 3 || !weighs) status |= OVG_ALIGN_FEW_PAIRS;
  if (!finite) status |= OVG_ALIGN_NOT_FINITE;
  const double dn = weighs ? W : 1.0;
  double step[3][4], scale, resid;
  status = solve_step(m, cen, dn, status, (p.flags & OVG_ALIGN_SCALE) != 0, step, scale, resid);
  const bool keep = status != 0 && (p.flags & OVG_WALIGN_KEEP) != 0;                 // the last good transform and its scale stay
  if (!keep) {
    double* T = p.transform;
    for (int r = 0; r < 3; ++r)
      for (int c = 0; c < 4; ++c) T[4 * r + c] = step[r][c];
    T[12] = 0.0, T[13] = 0.0, T[14] = 0.0, T[15] = 1.0;
    if (p.out_scale) *p.out_scale = scale;
  }
  if (p.out_rms) *p.out_rms = (weighs && finite_f64(W) && finite_f64(m[17])) ? sqrt(m[17] / W) : 0.0;
  if (p.out_fit_rms) *p.out_fit_rms = (status == 0 && finite_f64(resid)) ? sqrt((resid > 0.0 ? resid : 0.0) / W) : 0.0;
  if (p.out_weight) *p.out_weight = W;
  if (p.out_count) *p.out_count = n;
  if (p.out_status) *p.out_status = status;
}

__global__ __launch_bounds__(kThreads) void align_move_maps(ovg_align_move_maps_params p) {
  const int64_t i = (int64_t)blockIdx.x * kThreads + threadIdx.x;
  if (i >= p.n) return;
  if (p.points) {
    const float* s = p.points + 3 * i;
    const double x = (double)s[0], y = (double)s[1], z = (double)s[2];
    float o[3];
#pragma unroll
    for (int r = 0; r < 3; ++r) {
      const double* T = p.transform + 4 * r;
      o[r] = (float)(((T[0] * x + T[1] * y) + T[2] * z) + T[3]);
    }
    float* d = p.out_points + 3 * i;
    d[0] = o[0], d[1] = o[1], d[2] = o[2];
  }
  if (p.depth) p.out_depth[i] = (float)((double)p.depth[i] * *p.scale);
  if (p.points_conf) p.out_points_conf[i] = p.points_conf[i];
  if (p.depth_conf) p.out_depth_conf[i] = p.depth_conf[i];
}

// the camera that sees the moved points at s times the old depth: s (Rv x + tv) = A x' + t' for x' = M x, M = [s Rg, tM]
__global__ __launch_bounds__(64) void align_move_cameras(ovg_align_move_cameras_params p) {
  const int64_t v = (int64_t)blockIdx.x * 64 + threadIdx.x;
  if (v >= p.views) return;
  const double s = *p.scale;
  double Rg[3][3], tM[3];
  for (int r = 0; r < 3; ++r) {
    for (int c = 0; c < 3; ++c) Rg[r][c] = p.transform[4 * r + c] / s;
    tM[r] = p.transform[4 * r + 3];
  }
  const float* E = p.extrinsic + 12 * v;
  float o[12];
  for (int i = 0; i < 3; ++i) {
    const double r0 = (double)E[4 * i], r1 = (double)E[4 * i + 1], r2 = (double)E[4 * i + 2], tv = (double)E[4 * i + 3];
    double A[3];
    for (int j = 0; j < 3; ++j) A[j] = (r0 * Rg[j][0] + r1 * Rg[j][1]) + r2 * Rg[j][2];
    for (int j = 0; j < 3; ++j) o[4 * i + j] = (float)A[j];
    o[4 * i + 3] = (float)(s * tv - ((A[0] * tM[0] + A[1] * tM[1]) + A[2] * tM[2]));
  }
  float* d = p.out + 12 * v;
  for (int k = 0; k < 12; ++k) d[k] = o[k];
}

__global__ __launch_bounds__(kThreads) void align_apply(ovg_align_apply_params p) {
  const int64_t i = (int64_t)blockIdx.x * kThreads + threadIdx.x;
  if (i >= p.n) return;
  const float* s = p.points + 3 * i;
  const double x = (double)s[0], y = (double)s[1], z = (double)s[2];
  float o[3];
#pragma unroll
  for (int r = 0; r < 3; ++r) {
    const double* T = p.transform + 4 * r;
    o[r] = (float)(((T[0] * x + T[1] * y) + T[2] * z) + T[3]);
  }
  float* d = p.out + 3 * i;
  d[0] = o[0], d[1] = o[1], d[2] = o[2];
}

int64_t tiles_of(int64_t n) { return (n + kTile - 1) / kTile; }

}  // namespace

extern "C" int64_t ovg_align_workspace_bytes(int64_t n) {
  if (!size_ok(n)) return -1;
  return round256(tiles_of(n) * OVG_ALIGN_PARTIAL_BYTES);
}

extern "C" int ovg_align_moments(const ovg_align_moments_params* p, void* stream) {
  if (!p || !p->source || !p->target || !p->ws || !p->out_count || !p->out_sums) return OVG_E_ARG;
  if (!size_ok(p->n) || !size_ok(p->m) || (!p->index && p->n != p->m)) return OVG_E_ARG;
  if (p->flags & ~OVG_ALIGN_GATE) return OVG_E_ARG;
  if ((p->flags & OVG_ALIGN_GATE) && (!p->sqdist || p->max_sqdist != p->max_sqdist)) return OVG_E_ARG;
  if (!al(p->source, 4) || !al(p->target, 4) || !al(p->index, 4) || !al(p->sqdist, 4) || !al(p->centre, 8) || !al(p->out_count, 8) ||
      !al(p->out_sums, 8) || !al(p->ws, 16))
    return OVG_E_ARG;
  if (p->ws_bytes < ovg_align_workspace_bytes(p->n)) return OVG_E_ARG;
  hipStream_t st = static_cast<hipStream_t>(stream);
  const int64_t tiles = tiles_of(p->n);
  OVG_LAUNCH(align_tiles, dim3((unsigned)tiles), dim3(kThreads), 0, st, *p);
  OVG_CHECK_LAUNCH();
  OVG_LAUNCH(align_fold, dim3(1), dim3(kThreads), 0, st, static_cast<const double*>(p->ws), tiles, p->out_count, p->out_sums);
  OVG_CHECK_LAUNCH();
  return OVG_OK;
}

extern "C" int ovg_align_solve(const ovg_align_solve_params* p, void* stream) {
  if (!p || !p->count || !p->sums || !p->transform) return OVG_E_ARG;
  if (p->flags & ~(int64_t)(OVG_ALIGN_SCALE | OVG_ALIGN_COMPOSE)) return OVG_E_ARG;
  if (!al(p->count, 8) || !al(p->sums, 8) || !al(p->centre, 8) || !al(p->transform, 8) || !al(p->out_scale, 8) || !al(p->out_rms, 8) ||
      !al(p->out_count, 8) || !al(p->out_status, 4))
    return OVG_E_ARG;
  hipStream_t st = static_cast<hipStream_t>(stream);
  OVG_LAUNCH(align_solve, dim3(1), dim3(64), 0, st, *p);
  OVG_CHECK_LAUNCH();
  return OVG_OK;
}

extern "C" int64_t ovg_align_wmoments_workspace_bytes(int64_t n) {
  if (!size_ok(n)) return -1;
  return round256(tiles_of(n) * OVG_WALIGN_PARTIAL_BYTES);
}

extern "C" int ovg_align_wmoments(const ovg_align_wmoments_params* p, void* stream) {
  if (!p || !p->source || !p->target || !p->ws || !p->out_count || !p->out_sums) return OVG_E_ARG;
  if (!size_ok(p->n)) return OVG_E_ARG;
  if (p->flags & ~(int64_t)OVG_WALIGN_CAUCHY) return OVG_E_ARG;
  if (p->delta_scale != p->delta_scale) return OVG_E_ARG;
  if (!al(p->source, 4) || !al(p->target, 4) || !al(p->weight, 4) || !al(p->transform, 8) || !al(p->delta, 8) || !al(p->centre, 8) ||
      !al(p->out_count, 8) || !al(p->out_sums, 8) || !al(p->ws, 16))
    return OVG_E_ARG;
  if (p->ws_bytes < ovg_align_wmoments_workspace_bytes(p->n)) return OVG_E_ARG;
  hipStream_t st = static_cast<hipStream_t>(stream);
  const int64_t tiles = tiles_of(p->n);
  OVG_LAUNCH(walign_tiles, dim3((unsigned)tiles), dim3(kThreads), 0, st, *p);
  OVG_CHECK_LAUNCH();
  OVG_LAUNCH(walign_fold, dim3(1), dim3(kThreads), 0, st, static_cast<const double*>(p->ws), tiles, p->out_count, p->out_sums);
  OVG_CHECK_LAUNCH();
  return OVG_OK;
}

extern "C" int ovg_align_wsolve(const ovg_align_wsolve_params* p, void* stream) {
  if (!p || !p->count || !p->sums || !p->transform) return OVG_E_ARG;
  if (p->flags & ~(int64_t)(OVG_ALIGN_SCALE | OVG_WALIGN_KEEP)) return OVG_E_ARG;
  if (!al(p->count, 8) || !al(p->sums, 8) || !al(p->centre, 8) || !al(p->transform, 8) || !al(p->out_scale, 8) || !al(p->out_rms, 8) ||
      !al(p->out_fit_rms, 8) || !al(p->out_weight, 8) || !al(p->out_count, 8) || !al(p->out_status, 4))
    return OVG_E_ARG;
  hipStream_t st = static_cast<hipStream_t>(stream);
  OVG_LAUNCH(walign_solve, dim3(1), dim3(64), 0, st, *p);
  OVG_CHECK_LAUNCH();
  return OVG_OK;
}

extern "C" int ovg_align_move_maps(const ovg_align_move_maps_params* p, void* stream) {
  if (!p || !size_ok(p->n)) return OVG_E_ARG;
  if (!p->points && !p->depth && !p->points_conf && !p->depth_conf) return OVG_E_ARG;
  if (!p->points != !p->out_points || !p->depth != !p->out_depth || !p->points_conf != !p->out_points_conf ||
      !p->depth_conf != !p->out_depth_conf)
    return OVG_E_ARG;
  if ((p->points && !p->transform) || (p->depth && !p->scale)) return OVG_E_ARG;
  if (!al(p->points, 4) || !al(p->depth, 4) || !al(p->points_conf, 4) || !al(p->depth_conf, 4) || !al(p->transform, 8) || !al(p->scale, 8) ||
      !al(p->out_points, 4) || !al(p->out_depth, 4) || !al(p->out_points_conf, 4) || !al(p->out_depth_conf, 4))
    return OVG_E_ARG;
  hipStream_t st = static_cast<hipStream_t>(stream);
  OVG_LAUNCH(align_move_maps, dim3((unsigned)((p->n + kThreads - 1) / kThreads)), dim3(kThreads), 0, st, *p);
  OVG_CHECK_LAUNCH();
  return OVG_OK;
}

extern "C" int ovg_align_move_cameras(const ovg_align_move_cameras_params* p, void* stream) {
  if (!p || !p->extrinsic || !p->transform || !p->scale || !p->out) return OVG_E_ARG;
  if (!size_ok(p->views)) return OVG_E_ARG;
  if (!al(p->extrinsic, 4) || !al(p->transform, 8) || !al(p->scale, 8) || !al(p->out, 4)) return OVG_E_ARG;
  hipStream_t st = static_cast<hipStream_t>(stream);
  OVG_LAUNCH(align_move_cameras, dim3((unsigned)((p->views + 63) / 64)), dim3(64), 0, st, *p);
  OVG_CHECK_LAUNCH();
  return OVG_OK;
}

extern "C" int ovg_align_apply(const ovg_align_apply_params* p, void* stream) {
  if (!p || !p->points || !p->transform || !p->out) return OVG_E_ARG;
  if (!size_ok(p->n)) return OVG_E_ARG;
  if (!al(p->points, 4) || !al(p->transform, 8) || !al(p->out, 4)) return OVG_E_ARG;
  hipStream_t st = static_cast<hipStream_t>(stream);
  OVG_LAUNCH(align_apply, dim3((unsigned)((p->n + kThreads - 1) / kThreads)), dim3(kThreads), 0, st, *p);
  OVG_CHECK_LAUNCH();
  return OVG_OK;
}
