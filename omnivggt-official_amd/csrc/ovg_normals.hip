// PCA normals from a neighbour table (ovg_knn_normals): for every query the mean and the covariance of the reference points its row
// of `index` names, in float64 over the ranks in ascending order, and the unit eigenvector of the smallest eigenvalue by cyclic
// Jacobi rotations (include/omnivggt_hip.h states the rule, tests/knn_twin.py restates the covariance operation for operation).
// One query per thread: 2 k gathered points, six running sums and a 3 x 3 solve, bound by the gather of the index rows and points.
#include <math.h>
#include "ovg_common.h"

// the twin's covariance is one numpy float64 operation per rounding: no fused multiply-adds in this unit (build.py: -ffp-contract=off)
#pragma clang fp contract(off)

namespace {

constexpr int kThreads = 256;
constexpr int kSweeps = OVG_KNN_NORMALS_SWEEPS;

// one Jacobi rotation in the (p, q) plane of a symmetric 3 x 3 matrix: app, aqq, apq its entries there, arp / arq the third row's;
// vp, vq the matching columns of the accumulated rotations. theta^2 may overflow to +inf: t becomes 0, the rotation the identity
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

OVG_DEV bool finite_d(double v) { return fabs(v) <= 1.7976931348623157e308; }      // false for NaN

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
  if (m >= 3 && finite_d(xx) && finite_d(xy) && finite_d(xz) && finite_d(yy) && finite_d(yz) && finite_d(zz)) {
    double v0[3] = {1.0, 0.0, 0.0}, v1[3] = {0.0, 1.0, 0.0}, v2[3] = {0.0, 0.0, 1.0};
    const double trace = (xx + yy) + zz;
    for (int s = 0; s < kSweeps; ++s) {
      jacobi_rotate(xx, yy, xy, xz, yz, v0, v1);       // (0, 1): the third index is 2
      jacobi_rotate(xx, zz, xz, xy, yz, v0, v2);       // (0, 2): the third index is 1
      jacobi_rotate(yy, zz, yz, xy, xz, v1, v2);       // (1, 2): the third index is 0
    }
    // the smallest diagonal entry, the lowest column on ties
    double lam = xx, e[3] = {v0[0], v0[1], v0[2]};
    if (yy < lam) lam = yy, e[0] = v1[0], e[1] = v1[1], e[2] = v1[2];
    if (zz < lam) lam = zz, e[0] = v2[0], e[1] = v2[1], e[2] = v2[2];
    const double len = sqrt((e[0] * e[0] + e[1] * e[1]) + e[2] * e[2]);
    e[0] = e[0] / len, e[1] = e[1] / len, e[2] = e[2] / len;
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

bool al(const void* q, uintptr_t a) { return (reinterpret_cast<uintptr_t>(q) & (a - 1)) == 0; }

}  // namespace

extern "C" int ovg_knn_normals(const ovg_knn_normals_params* p, void* stream) {
  if (!p || !p->query || !p->reference || !p->index || !p->normal) return OVG_E_ARG;
  if (p->nq <= 0 || p->nr <= 0 || p->nq >= (1ll << 31) || p->nr >= (1ll << 31) || p->k < 1) return OVG_E_ARG;
  if (p->viewpoint ? (p->viewpoint_stride != 0 && p->viewpoint_stride != 3) : p->viewpoint_stride != 0) return OVG_E_ARG;
  if (!al(p->query, 4) || !al(p->reference, 4) || !al(p->index, 4) || !al(p->viewpoint, 4) || !al(p->normal, 4) || !al(p->curvature, 4) ||
      !al(p->covariance, 8) || !al(p->used, 4))
    return OVG_E_ARG;
  hipStream_t st = static_cast<hipStream_t>(stream);
  OVG_LAUNCH(knn_normals, dim3((unsigned)((p->nq + kThreads - 1) / kThreads)), dim3(kThreads), 0, st, *p);
  OVG_CHECK_LAUNCH();
  return OVG_OK;
}
