// PCA normals from a neighbour table (ovg_knn_normals): for every query the mean and the covariance of the reference points its row
// of `index` names, in float64 over the ranks in ascending order, and the unit eigenvector of the smallest eigenvalue by cyclic
// Jacobi rotations (include/omnivggt_hip.h states the rule, tests/knn_twin.py restates the covariance operation for operation).
// One query per thread: 2 k gathered points, six running sums and a 3 x 3 solve, bound by the gather of the index rows and points.
#include "ovg_geom.h"

// the twin's covariance is one numpy float64 operation per rounding: no fused multiply-adds in this unit (build.py: -ffp-contract=off)
#pragma clang fp contract(off)

namespace {

constexpr int kThreads = 256;
constexpr int kSweeps = OVG_KNN_NORMALS_SWEEPS;

__global__ __launch_bounds__(kThreads) void knn_normals(ovg_knn_normals_params p) {
  const int64_t i = (int64_t)blockIdx.x * kThreads + threadIdx.x;
  if (i >= p.nq) return;
  const int32_t* row = p.index + i * p.k;
  int32_t m = 0;
  double sx = 0.0, sy = 0.0, sz = 0.0;
  for (int32_t t = 0; t < p.k; ++t) {
    const int32_t j = row[t];
    if (j < 0 || (int64_t)j >= p.nr) continue;
    const float* r = p.reference + 3 * (int64_t)j;
    sx = sx + (double)r[0], sy = sy + (double)r[1], sz = sz + (double)r[2];
    ++m;
  }
  const double dm = (double)(m > 0 ? m : 1);                                     // no neighbour: the sums are zero and stay zero
  const double mx = sx / dm, my = sy / dm, mz = sz / dm;
  double xx = 0.0, xy = 0.0, xz = 0.0, yy = 0.0, yz = 0.0, zz = 0.0;
  for (int32_t t = 0; t < p.k; ++t) {
    const int32_t j = row[t];
    if (j < 0 || (int64_t)j >= p.nr) continue;
    const float* r = p.reference + 3 * (int64_t)j;
    const double dx = (double)r[0] - mx, dy = (double)r[1] - my, dz = (double)r[2] - mz;
    xx = xx + dx * dx, xy = xy + dx * dy, xz = xz + dx * dz, yy = yy + dy * dy, yz = yz + dy * dz, zz = zz + dz * dz;
  }
  xx = xx / dm, xy = xy / dm, xz = xz / dm, yy = yy / dm, yz = yz / dm, zz = zz / dm;
  if (p.used) p.used[i] = m;
  if (p.covariance) {
    double* c = p.covariance + 6 * i;
    c[0] = xx, c[1] = xy, c[2] = xz, c[3] = yy, c[4] = yz, c[5] = zz;
  }
  float n[3] = {0.0f, 0.0f, 0.0f}, curv = 0.0f;
  if (m >= 3 && finite_f64(xx) && finite_f64(xy) && finite_f64(xz) && finite_f64(yy) && finite_f64(yz) && finite_f64(zz)) {
    double v0[3], v1[3], v2[3], e[3];
    const double trace = (xx + yy) + zz;
    jacobi_sweeps3(xx, xy, xz, yy, yz, zz, v0, v1, v2, kSweeps);
    int kmin;
    const double lam = jacobi_smallest(xx, yy, zz, v0, v1, v2, kmin, e);
    bool flip;
    if (p.viewpoint) {
      const float* v = p.viewpoint + (int64_t)p.viewpoint_stride * i;
      const float* q = p.query + 3 * i;
      const double d0 = (double)v[0] - (double)q[0], d1 = (double)v[1] - (double)q[1], d2 = (double)v[2] - (double)q[2];
      flip = (e[0] * d0 + e[1] * d1) + e[2] * d2 < 0.0;
    } else {
      double big = e[0];
      if (fabs(e[1]) > fabs(big)) big = e[1];
      if (fabs(e[2]) > fabs(big)) big = e[2];
      flip = big < 0.0;
    }
    n[0] = (float)(flip ? -e[0] : e[0]), n[1] = (float)(flip ? -e[1] : e[1]), n[2] = (float)(flip ? -e[2] : e[2]);
    // a covariance is positive semi-definite: a negative smallest eigenvalue is rounding, reported as 0
    curv = trace > 0.0 && lam > 0.0 ? (float)(lam / trace) : 0.0f;
  }
  float* o = p.normal + 3 * i;
  o[0] = n[0], o[1] = n[1], o[2] = n[2];
  if (p.curvature) p.curvature[i] = curv;
}

}  // namespace

extern "C" int ovg_knn_normals(const ovg_knn_normals_params* p, void* stream) {
  if (!p || !p->query || !p->reference || !p->index || !p->normal) return OVG_E_ARG;
  if (!size_ok(p->nq) || !size_ok(p->nr) || p->k < 1) return OVG_E_ARG;
  if (p->viewpoint ? (p->viewpoint_stride != 0 && p->viewpoint_stride != 3) : p->viewpoint_stride != 0) return OVG_E_ARG;
  if (!al(p->query, 4) || !al(p->reference, 4) || !al(p->index, 4) || !al(p->viewpoint, 4) || !al(p->normal, 4) || !al(p->curvature, 4) ||
      !al(p->covariance, 8) || !al(p->used, 4))
    return OVG_E_ARG;
  hipStream_t st = static_cast<hipStream_t>(stream);
  OVG_LAUNCH(knn_normals, dim3((unsigned)((p->nq + kThreads - 1) / kThreads)), dim3(kThreads), 0, st, *p);
  OVG_CHECK_LAUNCH();
  return OVG_OK;
}
