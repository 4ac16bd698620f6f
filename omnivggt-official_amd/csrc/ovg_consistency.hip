// Multi-view depth consistency (ovg_multiview_consistency): for every pixel of S point maps, how many of the other S - 1 views
// confirm it (support), look through it (violations) or cannot see it (occluded). Two launches: the own-depth maps z[S][H][W] into the
// caller's workspace (unusable pixels as NaN, so that the pair kernel needs one read per pair), then one thread per source pixel with
// the target views in a loop. No atomics and no communication between workgroups; the cost is the S (S - 1) H W gathered reads.
#include "ovg_geom.h"
#include "ovg_project.h"

// tests/consistency_twin.py restates the rule in numpy float32, one rounding per operation: no fused multiply-adds in this unit
// (build.py compiles it with -ffp-contract=off as well)
#pragma clang fp contract(off)

namespace {

constexpr int kThreads = 256;

int64_t mvc_ws_bytes(int64_t S, int64_t H, int64_t W) { return (S * H * W * 4 + 15) / 16 * 16; }
bool mvc_shape_ok(int32_t S, int32_t H, int32_t W) {
  // S, H, W < 2^31 each, so the first product is below 2^62 and the second test cannot overflow
  return S > 0 && S <= OVG_MVC_MAX_VIEWS && H > 0 && W > 0 && (int64_t)H * W < (1ll << 31) && (int64_t)S * ((int64_t)H * W) < (1ll << 31);
}

// blockIdx.y = view: the camera row is wave-uniform (scalar loads)
__global__ __launch_bounds__(kThreads) void mvc_zmap(const float* __restrict__ points, const float* __restrict__ cams,
                                                     const uint8_t* __restrict__ valid, float* __restrict__ zmap, int32_t hw, float near) {
  const int64_t q = (int64_t)blockIdx.x * kThreads + threadIdx.x;
  if (q >= hw) return;
  const int32_t s = (int32_t)blockIdx.y;
  const int64_t g = (int64_t)s * hw + q;                                  // < 2^31 (checked by the entry)
  const float* p = points + 3 * g;
  const float z = camera_depth(cams + 16 * (int64_t)s, p[0], p[1], p[2]);
  const bool usable = (!valid || valid[g] != 0) && finite_f32(z) && z > near;
  zmap[g] = usable ? z : __uint_as_float(0x7FC00000u);
}

// TW x TH = 256 source pixels of one view per workgroup; thread t is pixel (t % TW, t / TW) of the tile, so a wave covers
// TW x (64 / TW) pixels (TW <= 64) and its 64 projections into a target view stay close together. blockIdx.y = source view.
// Every workgroup walks the targets in the same order unless kRotate (then it starts behind its own view).
template <int TW, int TH, bool kRotate>
__global__ __launch_bounds__(kThreads) void mvc_pairs(const float* __restrict__ points, const float* __restrict__ cams,
                                                      const float* __restrict__ zmap, int32_t S, int32_t H, int32_t W, int32_t src_first,
                                                      int32_t tiles_x, float tol, float near, int16_t* __restrict__ support,
                                                      int16_t* __restrict__ violations, int16_t* __restrict__ occluded) {
  static_assert(TW * TH == kThreads, "one thread per pixel of the tile");
  const int32_t tile_y = (int32_t)blockIdx.x / tiles_x, tile_x = (int32_t)blockIdx.x - tile_y * tiles_x;
  const int32_t px = tile_x * TW + (int32_t)threadIdx.x % TW, py = tile_y * TH + (int32_t)threadIdx.x / TW;
  if (px >= W || py >= H) return;
  const int32_t hw = H * W, q = py * W + px;
  const int32_t i = src_first + (int32_t)blockIdx.y;
  const int64_t g = (int64_t)i * hw + q;
  int32_t sup = 0, vio = 0, occ = 0;
  if (zmap[g] == zmap[g]) {                                               // NaN marks an unusable pixel: all three counts stay 0
    const float x = points[3 * g], y = points[3 * g + 1], z = points[3 * g + 2];
    const float hi_u = (float)(W - 1), hi_w = (float)(H - 1);            // small integers: exact in f32
    for (int32_t t = 0; t < S - 1; ++t) {
      int32_t j;
      if (kRotate) {
        j = i + 1 + t;
        j = j >= S ? j - S : j;
      } else {
        j = t < i ? t : t + 1;
      }
      float zc, u, w;
      if (!project_point(cams + 16 * (int64_t)j, x, y, z, near, zc, u, w)) continue;
      if (!(u >= 0.0f && u <= hi_u && w >= 0.0f && w <= hi_w)) continue;  // NaN fails; past this line the conversions are in range
      const float d = zmap[(int64_t)j * hw + ((int32_t)w * W + (int32_t)u)];
      if (!(d == d)) continue;                                            // the target pixel is not usable
      const float band = tol * d, diff = zc - d;                          // d > near > 0 and tol >= 0: band >= 0, exactly one class
      sup += fabsf(diff) <= band;
      vio += diff < -band;
      occ += diff > band;
    }
  }
  const int64_t o = (int64_t)blockIdx.y * hw + q;
  support[o] = (int16_t)sup;
  violations[o] = (int16_t)vio;
  if (occluded) occluded[o] = (int16_t)occ;
}

template <int TW, int TH>
int mvc_launch(const ovg_consistency_params* p, hipStream_t st) {
  const int32_t tiles_x = (p->W + TW - 1) / TW, tiles_y = (p->H + TH - 1) / TH;     // tiles_x * tiles_y <= H W < 2^31
  const dim3 grid((unsigned)(tiles_x * tiles_y), (unsigned)p->src_count);
  const float* zmap = static_cast<const float*>(p->ws);
  if (p->flags & OVG_MVC_ROTATE_TARGETS)
    OVG_LAUNCH((mvc_pairs<TW, TH, true>), grid, dim3(kThreads), 0, st, p->points, p->cams, zmap, p->S, p->H, p->W, p->src_first, tiles_x,
               p->tol, p->near, p->support, p->violations, p->occluded);
  else
    OVG_LAUNCH((mvc_pairs<TW, TH, false>), grid, dim3(kThreads), 0, st, p->points, p->cams, zmap, p->S, p->H, p->W, p->src_first, tiles_x,
               p->tol, p->near, p->support, p->violations, p->occluded);
  OVG_CHECK_LAUNCH();
  return OVG_OK;
}

}  // namespace

extern "C" int64_t ovg_consistency_workspace_bytes(int32_t S, int32_t H, int32_t W) { return mvc_shape_ok(S, H, W) ? mvc_ws_bytes(S, H, W) : -1; }

extern "C" int ovg_multiview_consistency(const ovg_consistency_params* p, void* stream) {
  if (!p || !p->points || !p->cams || !p->ws || !p->support || !p->violations) return OVG_E_ARG;
  if (!mvc_shape_ok(p->S, p->H, p->W)) return OVG_E_ARG;
  if (p->src_first < 0 || p->src_count <= 0 || p->src_first >= p->S || p->src_count > p->S - p->src_first) return OVG_E_ARG;
  if (!(p->tol >= 0.0f) || !(p->tol <= 3.402823466e38f)) return OVG_E_ARG;
  if (!(p->near > 0.0f) || !(p->near <= 3.402823466e38f)) return OVG_E_ARG;
  if (p->tile < OVG_MVC_TILE_DEFAULT || p->tile > OVG_MVC_TILE_32x8 || (p->flags & ~(OVG_MVC_ROTATE_TARGETS | OVG_MVC_KEEP_MAP))) return OVG_E_ARG;
  if (!al(p->ws, 16) || p->ws_bytes < mvc_ws_bytes(p->S, p->H, p->W)) return OVG_E_ARG;
  if (!al(p->support, 2) || !al(p->violations, 2) || !al(p->occluded, 2)) return OVG_E_ARG;
  hipStream_t st = static_cast<hipStream_t>(stream);
  const int32_t hw = p->H * p->W;
  if (!(p->flags & OVG_MVC_KEEP_MAP)) {
    OVG_LAUNCH(mvc_zmap, dim3((unsigned)(((int64_t)hw + kThreads - 1) / kThreads), (unsigned)p->S), dim3(kThreads), 0, st, p->points, p->cams,
               p->valid, static_cast<float*>(p->ws), hw, p->near);
    OVG_CHECK_LAUNCH();
  }
  switch (p->tile) {
    case OVG_MVC_TILE_256x1: return mvc_launch<256, 1>(p, st);
    case OVG_MVC_TILE_16x16: return mvc_launch<16, 16>(p, st);
    case OVG_MVC_TILE_32x8: return mvc_launch<32, 8>(p, st);
    default: return mvc_launch<8, 32>(p, st);                              // OVG_MVC_TILE_DEFAULT, OVG_MVC_TILE_8x32
  }
}
