// Registration of point clouds (ovg_align_moments, ovg_align_solve, ovg_align_apply): the float64 pair moments of a correspondence set
// summed in a FIXED order (include/omnivggt_hip.h states it, tests/align_twin.py restates it operation for operation), the rigid /
// similarity transform from them by Horn's quaternion method (a 4 x 4 cyclic Jacobi solve in one thread), and the transform applied.
// The moments are a streaming reduction -- 24 bytes of points, up to 10 of index, masks and gate per pair, and a gather -- bound by
// memory; the order is fixed by giving every thread its pairs, every wave its tree and every tile its slot: no atomics, no spinning.
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
  double step[3][4] = {{1.0, 0.0, 0.0, 0.0}, {0.0, 1.0, 0.0, 0.0}, {0.0, 0.0, 1.0, 0.0}}, scale = 1.0;
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
      if (p.flags & OVG_ALIGN_SCALE) {
        double tr = 0.0;
        for (int r = 0; r < 3; ++r)
          for (int c = 0; c < 3; ++c) tr = tr + R[r][c] * S[c][r];
        scale = tr / var;
      }
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
    scale = 1.0;
    for (int r = 0; r < 3; ++r)
      for (int c = 0; c < 4; ++c) step[r][c] = r == c ? 1.0 : 0.0;
  }
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

extern "C" int ovg_align_apply(const ovg_align_apply_params* p, void* stream) {
  if (!p || !p->points || !p->transform || !p->out) return OVG_E_ARG;
  if (!size_ok(p->n)) return OVG_E_ARG;
  if (!al(p->points, 4) || !al(p->transform, 8) || !al(p->out, 4)) return OVG_E_ARG;
  hipStream_t st = static_cast<hipStream_t>(stream);
  OVG_LAUNCH(align_apply, dim3((unsigned)((p->n + kThreads - 1) / kThreads)), dim3(kThreads), 0, st, *p);
  OVG_CHECK_LAUNCH();
  return OVG_OK;
}
