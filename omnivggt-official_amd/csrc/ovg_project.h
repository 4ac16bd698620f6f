// The pinhole projection shared by the rendering unit (ovg_render.hip) and the multi-view consistency unit (ovg_consistency.hip):
// rules 1-3 of tests/render_twin.py, operation for operation in float32 with one rounding each. Units that include this are compiled
// with -ffp-contract=off (build.py); the pragma below covers the functions of this header as well.
#pragma once
#include "ovg_geom.h"

#pragma clang fp contract(off)

// third row of the world-to-camera transform alone: zc = ((R20 x + R21 y) + R22 z) + tz
OVG_DEV float camera_depth(const float* __restrict__ c, float x, float y, float z) { return ((c[6] * x + c[7] * y) + c[8] * z) + c[11]; }

// c: one camera row [16] (rotation row-major, translation, fx, fy, cx, cy). false when the point is culled for this view (a camera
// coordinate is not finite, or zc <= near); otherwise zc and the rounded pixel (u, w) as floats -- not yet compared with the frame,
// possibly NaN or far outside the int32 range: compare in f32 before converting.
OVG_DEV bool project_point(const float* __restrict__ c, float x, float y, float z, float near, float& zc, float& u, float& w) {
  const float xc = ((c[0] * x + c[1] * y) + c[2] * z) + c[9];
  const float yc = ((c[3] * x + c[4] * y) + c[5] * z) + c[10];
  zc = camera_depth(c, x, y, z);
  if (!(finite_f32(xc) && finite_f32(yc) && finite_f32(zc) && zc > near)) return false;
  u = floorf((c[12] * __fdiv_rn(xc, zc) + c[14]) + 0.5f);
  w = floorf((c[13] * __fdiv_rn(yc, zc) + c[15]) + 0.5f);
  return true;
}
