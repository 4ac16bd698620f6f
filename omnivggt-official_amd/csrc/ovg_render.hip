// Point-cloud rendering (ovg_render_points): z-buffered square splats of a coloured cloud into V pinhole views, the headless stand-in
// for the reference's interactive viewer (inference.py: viser_wrapper). Three launches: fill the u64 z-buffer with ~0, splat (one
// 64-bit unsigned atomic min per covered pixel), resolve to rgb / depth / index. The splat is bound by its atomics, not by arithmetic.
#include "ovg_geom.h"
#include "ovg_project.h"

// the projection (ovg_project.h, shared with ovg_consistency.hip) restates tests/render_twin.py's numpy float32 expression operation
// for operation: no fused multiply-adds in this unit. The pragma covers the code below; build.py also compiles the unit with
// -ffp-contract=off (as for ovg_pointcloud.hip)
#pragma clang fp contract(off)

namespace {

constexpr int kThreads = 256;
constexpr uint64_t kEmpty = ~0ull;                  // bits(zc) of a finite positive float never reach 0xFFFFFFFF

int64_t rd_pixels(int64_t V, int64_t H, int64_t W) { return V * H * W; }
int64_t rd_ws_bytes(int64_t V, int64_t H, int64_t W) { return (rd_pixels(V, H, W) * 8 + 15) / 16 * 16; }
bool rd_shape_ok(int32_t V, int32_t H, int32_t W) {
  // V, H, W < 2^31 each, so the first product is below 2^62 and the second test cannot overflow
  return V > 0 && H > 0 && W > 0 && (int64_t)H * W < (1ll << 31) && (int64_t)V * ((int64_t)H * W) < (1ll << 31);
}

__global__ __launch_bounds__(kThreads) void rd_fill(u32x4* z, int64_t n16) {
  const u32x4 empty = {0xFFFFFFFFu, 0xFFFFFFFFu, 0xFFFFFFFFu, 0xFFFFFFFFu};
  for (int64_t i = (int64_t)blockIdx.x * kThreads + threadIdx.x; i < n16; i += (int64_t)gridDim.x * kThreads) z[i] = empty;
}

// one thread per point, all views in a loop: the camera rows are wave-uniform reads (the pointers are restrict kernel arguments, so
// they become scalar loads), a wave's points are neighbours in the cloud and, for a cloud in pixel order, neighbours in the image
template <bool kPreread>
__global__ __launch_bounds__(kThreads) void rd_splat(const float* __restrict__ points, const float* __restrict__ cams,
                                                     uint64_t* __restrict__ zbuf, int64_t n, int32_t V, int32_t H, int32_t W,
                                                     int32_t r, float near) {
  const int64_t i = (int64_t)blockIdx.x * kThreads + threadIdx.x;
  if (i >= n) return;
  const float x = points[3 * i], y = points[3 * i + 1], z = points[3 * i + 2];
  const float lo = (float)-r, hi_u = (float)(W - 1 + r), hi_w = (float)(H - 1 + r);    // small integers: exact in f32
  const int64_t hw = (int64_t)H * W;
  for (int32_t v = 0; v < V; ++v) {
    float zc, u, w;
    if (!project_point(cams + 16 * (int64_t)v, x, y, z, near, zc, u, w)) continue;
    if (!(u >= lo && u <= hi_u && w >= lo && w <= hi_w)) continue;         // NaN fails; past this line the conversions are in range
    const int32_t px = (int32_t)u, py = (int32_t)w;
    const uint64_t key = ((uint64_t)__float_as_uint(zc) << 32) | (uint32_t)i;
    const int32_t x0 = max(px - r, 0), x1 = min(px + r, W - 1), y0 = max(py - r, 0), y1 = min(py + r, H - 1);
    uint64_t* img = zbuf + v * hw;
    for (int32_t qy = y0; qy <= y1; ++qy) {
      uint64_t* row = img + (int64_t)qy * W;
      for (int32_t qx = x0; qx <= x1; ++qx) {
        // stored keys only decrease: a point that already loses to what a (possibly stale) plain read shows needs no atomic
        if (kPreread && row[qx] < key) continue;
        __hip_atomic_fetch_min(row + qx, key, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      }
    }
  }
}

__global__ __launch_bounds__(kThreads) void rd_resolve(const uint64_t* __restrict__ zbuf, const uint8_t* __restrict__ colors,
                                                       int64_t npix, uint32_t bg, uint8_t* __restrict__ rgb,
                                                       float* __restrict__ depth, int64_t* __restrict__ index) {
  const int64_t q = (int64_t)blockIdx.x * kThreads + threadIdx.x;
  if (q >= npix) return;
  const uint64_t key = zbuf[q];
  const bool hit = key != kEmpty;
  const uint32_t i = (uint32_t)key;
  uint8_t c0 = (uint8_t)bg, c1 = (uint8_t)(bg >> 8), c2 = (uint8_t)(bg >> 16);
  if (hit) {
    const uint8_t* c = colors + 3 * (int64_t)i;
    c0 = c[0], c1 = c[1], c2 = c[2];
  }
  rgb[3 * q] = c0, rgb[3 * q + 1] = c1, rgb[3 * q + 2] = c2;
  if (depth) depth[q] = hit ? __uint_as_float((uint32_t)(key >> 32)) : 0.0f;
  if (index) index[q] = hit ? (int64_t)i : -1;
}

}  // namespace

extern "C" int64_t ovg_render_workspace_bytes(int32_t V, int32_t H, int32_t W) { return rd_shape_ok(V, H, W) ? rd_ws_bytes(V, H, W) : -1; }

extern "C" int ovg_render_points(const ovg_render_params* p, void* stream) {
  if (!p || !p->cams || !p->ws || !p->out_rgb || p->n < 0 || p->n >= (1ll << 32)) return OVG_E_ARG;
  if (p->n > 0 && (!p->points || !p->colors)) return OVG_E_ARG;
  if (!rd_shape_ok(p->V, p->H, p->W) || p->radius < 0 || p->radius > OVG_RENDER_MAX_RADIUS) return OVG_E_ARG;
  if (!(p->near > 0.0f) || !(p->near <= 3.402823466e38f) || (p->flags & ~OVG_RENDER_NO_PREREAD)) return OVG_E_ARG;
  if (!al(p->ws, 16) || p->ws_bytes < rd_ws_bytes(p->V, p->H, p->W)) return OVG_E_ARG;
  hipStream_t st = static_cast<hipStream_t>(stream);
  const int64_t npix = rd_pixels(p->V, p->H, p->W), n16 = rd_ws_bytes(p->V, p->H, p->W) / 16;
  uint64_t* zbuf = static_cast<uint64_t*>(p->ws);
  const unsigned fill_blocks = (unsigned)((n16 + kThreads * 4 - 1) / (kThreads * 4));
  OVG_LAUNCH(rd_fill, dim3(fill_blocks < 4096 ? fill_blocks : 4096), dim3(kThreads), 0, st, static_cast<u32x4*>(p->ws), n16);
  OVG_CHECK_LAUNCH();
  if (p->n > 0) {
    const dim3 grid((unsigned)((p->n + kThreads - 1) / kThreads));        // n < 2^32: at most 2^24 workgroups
    if (p->flags & OVG_RENDER_NO_PREREAD)
      OVG_LAUNCH(rd_splat<false>, grid, dim3(kThreads), 0, st, p->points, p->cams, zbuf, p->n, p->V, p->H, p->W, p->radius, p->near);
    else
      OVG_LAUNCH(rd_splat<true>, grid, dim3(kThreads), 0, st, p->points, p->cams, zbuf, p->n, p->V, p->H, p->W, p->radius, p->near);
    OVG_CHECK_LAUNCH();
  }
  const uint32_t bg = (uint32_t)p->background[0] | ((uint32_t)p->background[1] << 8) | ((uint32_t)p->background[2] << 16);
  OVG_LAUNCH(rd_resolve, dim3((unsigned)((npix + kThreads - 1) / kThreads)), dim3(kThreads), 0, st, zbuf, p->colors, npix, bg,
             p->out_rgb, p->out_depth, p->out_index);
  OVG_CHECK_LAUNCH();
  return OVG_OK;
}
