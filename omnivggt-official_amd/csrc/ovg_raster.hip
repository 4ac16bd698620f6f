// Mesh rasterisation (ovg_render_mesh): z-buffered triangles of a Mesh into V pinhole views, shaded per pixel. Three launches: fill the
// u64 z-buffer with ~0, draw (edge functions in 8-bit sub-pixel fixed point, perspective-correct float64 depth, one 64-bit unsigned
// atomic min per covered pixel), resolve (the winning face again through the same functions, then colour / normal / shade).
// tests/raster_twin.py restates every step in numpy; no fused multiply-adds in this unit (the pragma below and -ffp-contract=off in
// build.py). The point renderer (ovg_render.hip) is not touched: the fill kernel is repeated here.
#include "ovg_geom.h"
#include "ovg_project.h"

#pragma clang fp contract(off)

namespace {

constexpr int kThreads = 256;
constexpr int kCoopDefault = 64;                    // boxes of up to this many pixels are walked by the face's own lane
constexpr uint64_t kEmpty = ~0ull;                  // bits(z) of a finite positive float never reach 0xFFFFFFFF
constexpr float kBand = 16384.0f;

int64_t rs_pixels(int64_t V, int64_t H, int64_t W) { return V * H * W; }
int64_t rs_ws_bytes(int64_t V, int64_t H, int64_t W) { return (rs_pixels(V, H, W) * 8 + 15) / 16 * 16; }
bool rs_shape_ok(int32_t V, int32_t H, int32_t W) {         // ovg_render_points' limits
  return V > 0 && H > 0 && W > 0 && (int64_t)H * W < (1ll << 31) && (int64_t)V * ((int64_t)H * W) < (1ll << 31);
}

__global__ __launch_bounds__(kThreads) void rs_fill(u32x4* z, int64_t n16) {
  const u32x4 empty = {0xFFFFFFFFu, 0xFFFFFFFFu, 0xFFFFFFFFu, 0xFFFFFFFFu};
  for (int64_t i = (int64_t)blockIdx.x * kThreads + threadIdx.x; i < n16; i += (int64_t)gridDim.x * kThreads) z[i] = empty;
}

// rule 2: camera coordinates as project_point's first half, then the screen position in 1/256 pixel. false: the vertex is not usable
OVG_DEV bool rs_vertex(const float* __restrict__ c, float x, float y, float z, float near, int32_t& X, int32_t& Y, float& zc) {
  const float xc = ((c[0] * x + c[1] * y) + c[2] * z) + c[9];
  const float yc = ((c[3] * x + c[4] * y) + c[5] * z) + c[10];
  zc = camera_depth(c, x, y, z);
  if (!(finite_f32(xc) && finite_f32(yc) && finite_f32(zc) && zc > near)) return false;
  const float sx = c[12] * __fdiv_rn(xc, zc) + c[14];
  const float sy = c[13] * __fdiv_rn(yc, zc) + c[15];
  if (!(sx >= -kBand && sx <= kBand && sy >= -kBand && sy <= kBand)) return false;      // NaN fails; |X|, |Y| <= 2^22 + 1 below
  X = (int32_t)floorf(sx * 256.0f + 0.5f);
  Y = (int32_t)floorf(sy * 256.0f + 0.5f);
  return true;
}

// what a lane needs to walk a face's box in one view: 13 registers, broadcast with __shfl on the cooperative path
struct Tri {
  int32_t X0, Y0, X1, Y1, X2, Y2;
  float z0, z1, z2;
  int32_t x0, x1, y0, y1;      // the clipped box in pixels, inclusive
};

OVG_DEV int64_t rs_area(const Tri& t) {
  return (int64_t)(t.X1 - t.X0) * (t.Y2 - t.Y0) - (int64_t)(t.Y1 - t.Y0) * (t.X2 - t.X0);
}

// rule 3: false when the face is not drawn (zero area, culled, or a box that misses the frame)
OVG_DEV bool rs_setup(Tri& t, int32_t cull, int32_t H, int32_t W) {
  const int64_t area = rs_area(t);
  if (area == 0 || (cull == OVG_MESH_CULL_BACK && area > 0) || (cull == OVG_MESH_CULL_FRONT && area < 0)) return false;
  const int32_t xmin = min(t.X0, min(t.X1, t.X2)), xmax = max(t.X0, max(t.X1, t.X2));
  const int32_t ymin = min(t.Y0, min(t.Y1, t.Y2)), ymax = max(t.Y0, max(t.Y1, t.Y2));
  t.x0 = max((xmin + 255) >> 8, 0), t.x1 = min(xmax >> 8, W - 1);          // arithmetic shifts: ceil and floor of the 1/256 values
  t.y0 = max((ymin + 255) >> 8, 0), t.y1 = min(ymax >> 8, H - 1);
  return t.x0 <= t.x1 && t.y0 <= t.y1;
}

// rules 4-5 at pixel (px, py) inside the box: differences fit int32 (below 2^23 + 2), products int64. false: not covered
OVG_DEV bool rs_pixel(const Tri& t, int64_t area, int32_t px, int32_t py, double& a0, double& a1, double& a2, double& zf) {
  const int32_t qx = px << 8, qy = py << 8;
  int64_t w0 = (int64_t)(t.X2 - t.X1) * (qy - t.Y1) - (int64_t)(t.Y2 - t.Y1) * (qx - t.X1);
  int64_t w1 = (int64_t)(t.X0 - t.X2) * (qy - t.Y2) - (int64_t)(t.Y0 - t.Y2) * (qx - t.X2);
  int64_t w2 = (int64_t)(t.X1 - t.X0) * (qy - t.Y0) - (int64_t)(t.Y1 - t.Y0) * (qx - t.X0);
  if (area < 0) w0 = -w0, w1 = -w1, w2 = -w2, area = -area;
  if ((w0 | w1 | w2) < 0) return false;
  const double ab = (double)area;
  a0 = __ddiv_rn((double)w0, ab) * __ddiv_rn(1.0, (double)t.z0);
  a1 = __ddiv_rn((double)w1, ab) * __ddiv_rn(1.0, (double)t.z1);
  a2 = __ddiv_rn((double)w2, ab) * __ddiv_rn(1.0, (double)t.z2);
  zf = __ddiv_rn(1.0, (a0 + a1) + a2);
  return true;
}

// pixels first, first + step, ... of the box in row-major order: the face's own lane (0, 1) or the whole wave (lane, 64)
OVG_DEV void rs_walk(const Tri& t, uint64_t* __restrict__ img, int32_t W, uint32_t face, uint32_t first, uint32_t step) {
  const int64_t area = rs_area(t);
  const uint32_t bw = (uint32_t)(t.x1 - t.x0 + 1), n = bw * (uint32_t)(t.y1 - t.y0 + 1);      // n <= H W < 2^31
  for (uint32_t k = first; k < n; k += step) {
    const uint32_t ry = k / bw;
    const int32_t px = t.x0 + (int32_t)(k - ry * bw), py = t.y0 + (int32_t)ry;
    double a0, a1, a2, zf;
    if (!rs_pixel(t, area, px, py, a0, a1, a2, zf)) continue;
    const uint64_t key = ((uint64_t)__float_as_uint((float)zf) << 32) | face;
    uint64_t* q = img + (int64_t)py * W + px;
    // stored keys only decrease: a face that already loses to what a (possibly stale) plain read shows needs no atomic
    if (*q < key) continue;
    __hip_atomic_fetch_min(q, key, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  }
}

// rules 1-3 of one face for one view. false: not drawn
OVG_DEV bool rs_face(const float* __restrict__ c, const float (&p)[9], float near, int32_t cull, int32_t H, int32_t W, Tri& t) {
  if (!rs_vertex(c, p[0], p[1], p[2], near, t.X0, t.Y0, t.z0)) return false;
  if (!rs_vertex(c, p[3], p[4], p[5], near, t.X1, t.Y1, t.z1)) return false;
  if (!rs_vertex(c, p[6], p[7], p[8], near, t.X2, t.Y2, t.z2)) return false;
  return rs_setup(t, cull, H, W);
}

OVG_DEV bool rs_load_face(const float* __restrict__ vertices, const int32_t* __restrict__ faces, int64_t M, int64_t f, int32_t (&i)[3],
                          float (&p)[9]) {
  i[0] = faces[3 * f], i[1] = faces[3 * f + 1], i[2] = faces[3 * f + 2];
  if (!(i[0] >= 0 && i[0] < M && i[1] >= 0 && i[1] < M && i[2] >= 0 && i[2] < M)) return false;      // rule 1: never read
#pragma unroll
  for (int k = 0; k < 3; ++k)
#pragma unroll
    for (int a = 0; a < 3; ++a) p[3 * k + a] = vertices[3 * (int64_t)i[k] + a];
  return true;
}

// one thread per face, all views in a loop (the camera row: scalar loads). A face whose box holds at most `coop` pixels is walked by its
// own lane; the others are walked by the whole wave, one after the other: no lane leaves before the wave is through the last view, so
// every lane of the wave takes part in every ballot and every shuffle. A large face costs its wave ceil(box / 64) iterations.
__global__ __launch_bounds__(kThreads) void rs_draw(const float* __restrict__ vertices, const int32_t* __restrict__ faces,
                                                    const float* __restrict__ cams, uint64_t* __restrict__ zbuf, int64_t M, int64_t F,
                                                    int32_t V, int32_t H, int32_t W, int32_t cull, float near, uint32_t coop) {
  const int64_t f = (int64_t)blockIdx.x * kThreads + threadIdx.x;
  const uint32_t lane = threadIdx.x & 63u;
  int32_t idx[3];
  float p[9] = {};
  const bool valid = f < F && rs_load_face(vertices, faces, M, f, idx, p);
  const int64_t hw = (int64_t)H * W;
  for (int32_t v = 0; v < V; ++v) {
    Tri t = {};
    uint64_t* img = zbuf + v * hw;
    bool large = false;
    if (valid && rs_face(cams + 16 * (int64_t)v, p, near, cull, H, W, t)) {
      const uint32_t n = (uint32_t)(t.x1 - t.x0 + 1) * (uint32_t)(t.y1 - t.y0 + 1);
      if (n <= coop) rs_walk(t, img, W, (uint32_t)f, 0u, 1u);
      else large = true;
    }
    uint64_t pending = __ballot(large);                                    // wave-uniform: at most 64 rounds
    while (pending) {
      const int src = __ffsll((unsigned long long)pending) - 1;
      pending &= pending - 1;
      Tri s;
      s.X0 = __shfl(t.X0, src), s.Y0 = __shfl(t.Y0, src), s.X1 = __shfl(t.X1, src), s.Y1 = __shfl(t.Y1, src);
      s.X2 = __shfl(t.X2, src), s.Y2 = __shfl(t.Y2, src), s.z0 = __shfl(t.z0, src), s.z1 = __shfl(t.z1, src), s.z2 = __shfl(t.z2, src);
      s.x0 = __shfl(t.x0, src), s.x1 = __shfl(t.x1, src), s.y0 = __shfl(t.y0, src), s.y1 = __shfl(t.y1, src);
      // faces of one wave are consecutive: the source lane's face is this lane's plus the lane difference
      rs_walk(s, img, W, (uint32_t)(f - lane + src), lane, 64u);
    }
  }
}

OVG_DEV uint8_t rs_u8(double x) { return !(x >= 0.0) ? 0 : x > 255.0 ? 255 : (uint8_t)x; }

// rule 6: one thread per pixel
__global__ __launch_bounds__(kThreads) void rs_resolve(const uint64_t* __restrict__ zbuf, const float* __restrict__ vertices,
                                                       const int32_t* __restrict__ faces, const float* __restrict__ normals,
                                                       const uint8_t* __restrict__ colors, const float* __restrict__ cams, int64_t M,
                                                       int64_t F, int64_t npix, int32_t H, int32_t W, int32_t shading, float near,
                                                       uint32_t bg, uint8_t* __restrict__ rgb, float* __restrict__ depth,
                                                       int64_t* __restrict__ index) {
  const int64_t q = (int64_t)blockIdx.x * kThreads + threadIdx.x;
  if (q >= npix) return;
  const uint64_t key = zbuf[q];
  const uint32_t f = (uint32_t)key;
  const int64_t hw = (int64_t)H * W, v = q / hw;
  const int32_t r = (int32_t)(q - v * hw), py = r / W, px = r - py * W;
  const float* c = cams + 16 * v;
  uint8_t out[3] = {(uint8_t)bg, (uint8_t)(bg >> 8), (uint8_t)(bg >> 16)};
  int32_t idx[3];
  float p[9];
  Tri t;
  double a0, a1, a2, zf;
  // the draw kernel only stores keys of faces it drew at pixels they cover: the tests repeat its own and always pass
  const bool hit = key != kEmpty && f < F && rs_load_face(vertices, faces, M, f, idx, p) && rs_face(c, p, near, OVG_MESH_CULL_NONE, H, W, t) &&
                   rs_pixel(t, rs_area(t), px, py, a0, a1, a2, zf);
  if (hit) {
    const double b[3] = {a0 * zf, a1 * zf, a2 * zf};
    double col[3] = {128.0, 128.0, 128.0}, n[3];
    if (colors) {
#pragma unroll
      for (int a = 0; a < 3; ++a)
        col[a] = (b[0] * (double)colors[3 * (int64_t)idx[0] + a] + b[1] * (double)colors[3 * (int64_t)idx[1] + a]) +
                 b[2] * (double)colors[3 * (int64_t)idx[2] + a];
    }
    if (normals) {
#pragma unroll
      for (int a = 0; a < 3; ++a)
        n[a] = (b[0] * (double)normals[3 * (int64_t)idx[0] + a] + b[1] * (double)normals[3 * (int64_t)idx[1] + a]) +
               b[2] * (double)normals[3 * (int64_t)idx[2] + a];
    } else {
      const double e1x = (double)p[3] - (double)p[0], e1y = (double)p[4] - (double)p[1], e1z = (double)p[5] - (double)p[2];
      const double e2x = (double)p[6] - (double)p[0], e2y = (double)p[7] - (double)p[1], e2z = (double)p[8] - (double)p[2];
      n[0] = e1y * e2z - e1z * e2y, n[1] = e1z * e2x - e1x * e2z, n[2] = e1x * e2y - e1y * e2x;
    }
    const double len = __dsqrt_rn((n[0] * n[0] + n[1] * n[1]) + n[2] * n[2]);
    const bool good = finite_f64(len) && len > 0.0;
    if (shading == OVG_MESH_SHADE_NORMAL) {
#pragma unroll
      for (int a = 0; a < 3; ++a) out[a] = good ? rs_u8(floor((0.5 * __ddiv_rn(n[a], len) + 0.5) * 255.0 + 0.5)) : 128;
    } else {
      double k = 1.0;
      if (shading == OVG_MESH_SHADE_HEADLIGHT) {
        const double s = good ? __ddiv_rn(fabs((n[0] * (double)c[6] + n[1] * (double)c[7]) + n[2] * (double)c[8]), len) : 1.0;
        k = 0.25 + 0.75 * s;
      }
#pragma unroll
      for (int a = 0; a < 3; ++a) out[a] = rs_u8(floor((shading == OVG_MESH_SHADE_HEADLIGHT ? k * col[a] : col[a]) + 0.5));
    }
  }
  rgb[3 * q] = out[0], rgb[3 * q + 1] = out[1], rgb[3 * q + 2] = out[2];
  if (depth) depth[q] = hit ? __uint_as_float((uint32_t)(key >> 32)) : 0.0f;
  if (index) index[q] = hit ? (int64_t)f : -1;
}

}  // namespace

extern "C" int64_t ovg_render_mesh_workspace_bytes(int32_t V, int32_t H, int32_t W) { return rs_shape_ok(V, H, W) ? rs_ws_bytes(V, H, W) : -1; }

extern "C" int ovg_render_mesh(const ovg_render_mesh_params* p, void* stream) {
  if (!p || !p->cams || !p->ws || !p->out_rgb) return OVG_E_ARG;
  if (p->M < 0 || p->M >= (1ll << 31) || p->F < 0 || p->F >= (1ll << 31)) return OVG_E_ARG;
  if ((p->M > 0 && !p->vertices) || (p->F > 0 && !p->faces)) return OVG_E_ARG;
  if (!rs_shape_ok(p->V, p->H, p->W) || !(p->near > 0.0f) || !(p->near <= 3.402823466e38f)) return OVG_E_ARG;
  if (p->shading < OVG_MESH_SHADE_COLOR || p->shading > OVG_MESH_SHADE_NORMAL || p->cull < OVG_MESH_CULL_NONE || p->cull > OVG_MESH_CULL_FRONT ||
      p->flags != 0 || p->coop_threshold < 0)
    return OVG_E_ARG;
  if (!al(p->ws, 16) || p->ws_bytes < rs_ws_bytes(p->V, p->H, p->W)) return OVG_E_ARG;
  hipStream_t st = static_cast<hipStream_t>(stream);
  const int64_t npix = rs_pixels(p->V, p->H, p->W), n16 = rs_ws_bytes(p->V, p->H, p->W) / 16;
  uint64_t* zbuf = static_cast<uint64_t*>(p->ws);
  const unsigned fill_blocks = (unsigned)((n16 + kThreads * 4 - 1) / (kThreads * 4));
  OVG_LAUNCH(rs_fill, dim3(fill_blocks < 4096 ? fill_blocks : 4096), dim3(kThreads), 0, st, static_cast<u32x4*>(p->ws), n16);
  OVG_CHECK_LAUNCH();
  if (p->F > 0 && p->M > 0) {
    const uint32_t coop = p->coop_threshold ? (uint32_t)p->coop_threshold : (uint32_t)kCoopDefault;
    OVG_LAUNCH(rs_draw, dim3((unsigned)((p->F + kThreads - 1) / kThreads)), dim3(kThreads), 0, st, p->vertices, p->faces, p->cams, zbuf, p->M,
               p->F, p->V, p->H, p->W, p->cull, p->near, coop);
    OVG_CHECK_LAUNCH();
  }
  const uint32_t bg = (uint32_t)p->background[0] | ((uint32_t)p->background[1] << 8) | ((uint32_t)p->background[2] << 16);
  OVG_LAUNCH(rs_resolve, dim3((unsigned)((npix + kThreads - 1) / kThreads)), dim3(kThreads), 0, st, zbuf, p->vertices, p->faces, p->normals,
             p->colors, p->cams, p->M, p->F, npix, p->H, p->W, p->shading, p->near, bg, p->out_rgb, p->out_depth, p->out_index);
  OVG_CHECK_LAUNCH();
  return OVG_OK;
}
