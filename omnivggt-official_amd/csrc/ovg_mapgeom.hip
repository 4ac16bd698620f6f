// Image-space map geometry (ovg_map_depth, ovg_map_normals, ovg_map_edges, ovg_map_triangulate): what follows from the prediction
// being [S][H][W] maps in which a pixel's neighbours are known for free -- the usable-depth map, normals as a cross product of two
// finite differences, depth / normal edge flags over a small window, and the grid mesh of the views by one ordered compaction.
// All stencils stay inside their view; no atomics, no communication between workgroups except through the two scans of the mesh.
#include "ovg_geom.h"
#include "ovg_project.h"

// tests/mapgeom_twin.py restates the rules in numpy, one rounding per operation: no fused multiply-adds in this unit
// (build.py compiles it with -ffp-contract=off as well)
#pragma clang fp contract(off)

namespace {

constexpr int kThreads = OVG_MAP_BLOCK;
constexpr int kR = OVG_MAP_MAX_RADIUS;

bool map_shape_ok(int32_t S, int32_t H, int32_t W) {
  // S, H, W < 2^31 each, so the first product is below 2^62 and the second test cannot overflow
  return S > 0 && H > 0 && W > 0 && (int64_t)H * W < (1ll << 31) && (int64_t)S * ((int64_t)H * W) < (1ll << 31);
}
int32_t per_view_blocks(int32_t hw) { return (int32_t)(((int64_t)hw + kThreads - 1) / kThreads); }   // S * this <= S H W < 2^31
bool pos_finite(float v) { return v > 0.0f && v <= 3.402823466e38f; }
bool tol_ok(float v) { return v >= 0.0f; }                                // +inf switches a test off; negative and NaN are refused

OVG_DEV float quiet_nan() { return __uint_as_float(0x7FC00000u); }

// ---------------------------------------------------------------------------------------------------------------------------------
// ovg_map_depth. One-dimensional grids throughout this unit (gridDim.y would cap S at 65535): workgroup b of view s is
// blockIdx.x = s * per_view + b, at most S H W < 2^31 of them. A workgroup stays in one view: the camera row is wave-uniform (scalar loads)
// ---------------------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(kThreads) void map_depth_kernel(const float* __restrict__ points, const float* __restrict__ cams,
                                                             const float* __restrict__ depth, const uint8_t* __restrict__ valid,
                                                             float* __restrict__ zmap, int32_t hw, int32_t per_view, float near) {
  const int32_t s = (int32_t)blockIdx.x / per_view;
  const int64_t q = (int64_t)((int32_t)blockIdx.x - s * per_view) * kThreads + threadIdx.x;
  if (q >= hw) return;
  const int64_t g = (int64_t)s * hw + q;                                  // < 2^31 (checked by the entry)
  float z;
  if (points) {
    const float* p = points + 3 * g;
    z = camera_depth(cams + 16 * (int64_t)s, p[0], p[1], p[2]);
  } else {
    z = depth[g];
  }
  const bool usable = (!valid || valid[g] != 0) && finite_f32(z) && z > near;
  zmap[g] = usable ? z : quiet_nan();
}

// ---------------------------------------------------------------------------------------------------------------------------------
// ovg_map_normals: one thread per pixel, its four neighbours from global memory (five point reads: nothing to stage)
// ---------------------------------------------------------------------------------------------------------------------------------
struct Diff { float v[3]; bool have; };

// the difference along one axis: `lo` / `hi` the flat indices of the neighbours before / behind g, use_lo / use_hi whether they are usable for g
OVG_DEV Diff axis_diff(const float* __restrict__ points, int64_t g, int64_t lo, int64_t hi, bool use_lo, bool use_hi) {
  Diff d;
  d.have = use_lo || use_hi;
  const float* a = points + 3 * (use_lo ? lo : g);
  const float* b = points + 3 * (use_hi ? hi : g);
#pragma unroll
  for (int k = 0; k < 3; ++k) d.v[k] = d.have ? b[k] - a[k] : 0.0f;
  return d;
}

__global__ __launch_bounds__(kThreads) void map_normals_kernel(const float* __restrict__ points, const float* __restrict__ zmap, int32_t H,
                                                               int32_t W, int32_t hw, int32_t per_view, float rel_tol,
                                                               float* __restrict__ normals) {
  const int32_t s = (int32_t)blockIdx.x / per_view;
  const int64_t q = (int64_t)((int32_t)blockIdx.x - s * per_view) * kThreads + threadIdx.x;
  if (q >= hw) return;
  const int32_t py = (int32_t)(q / W), px = (int32_t)(q - (int64_t)py * W);
  const int64_t g = (int64_t)s * hw + q;
  const float zp = zmap[g];
  float out[3] = {0.0f, 0.0f, 0.0f};
  if (zp == zp && finite3(points + 3 * g)) {
    const float band = rel_tol * zp;                                      // zp > near > 0: +inf for rel_tol = +inf
    auto usable = [&](int64_t gq) {
      const float zq = zmap[gq];
      return zq == zq && finite3(points + 3 * gq) && fabsf(zq - zp) <= band;
    };
    const bool left = px > 0 && usable(g - 1), right = px < W - 1 && usable(g + 1);
    const bool up = py > 0 && usable(g - W), down = py < H - 1 && usable(g + W);
    const Diff dh = axis_diff(points, g, g - 1, g + 1, left, right), dv = axis_diff(points, g, g - W, g + W, up, down);
    if (dh.have && dv.have) {
      const double hx = dh.v[0], hy = dh.v[1], hz = dh.v[2], vx = dv.v[0], vy = dv.v[1], vz = dv.v[2];
      const double nx = vy * hz - vz * hy, ny = vz * hx - vx * hz, nz = vx * hy - vy * hx;
      const double len = sqrt((nx * nx + ny * ny) + nz * nz);
      if (len > 0.0 && len <= 1.7976931348623157e308) {
        out[0] = (float)(nx / len);
        out[1] = (float)(ny / len);
        out[2] = (float)(nz / len);
      }
    }
  }
  float* n = normals + 3 * g;
  n[0] = out[0]; n[1] = out[1]; n[2] = out[2];
}

// ---------------------------------------------------------------------------------------------------------------------------------
// ovg_map_edges
// ---------------------------------------------------------------------------------------------------------------------------------
// what a pixel gathers over its window; see() takes one window pixel that lies inside the view
struct EdgeAcc {
  float zmin, zmax, nx, ny, nz, min_cos;
  bool with_normals, has_normal, normal_edge;
  OVG_DEV void see(float zq, float qx, float qy, float qz) {
    if (!(zq == zq)) return;
    zmin = zq < zmin ? zq : zmin;
    zmax = zq > zmax ? zq : zmax;
    if (with_normals && has_normal && !(qx == 0.0f && qy == 0.0f && qz == 0.0f)) normal_edge = normal_edge || ((nx * qx + ny * qy) + nz * qz < min_cos);
  }
  OVG_DEV uint8_t flags(float zp, float rel_tol) const {
    uint32_t f = 0;
    if (zmax - zmin > rel_tol * zp) f |= OVG_MAP_DEPTH_EDGE;
    if (with_normals) f |= has_normal ? (normal_edge ? OVG_MAP_NORMAL_EDGE : 0) : OVG_MAP_NO_NORMAL;
    return (uint8_t)f;
  }
};

OVG_DEV EdgeAcc edge_acc(float zp, float nx, float ny, float nz, bool with_normals, float min_cos) {
  EdgeAcc a;
  a.zmin = a.zmax = zp;
  a.nx = nx; a.ny = ny; a.nz = nz; a.min_cos = min_cos;
  a.with_normals = with_normals;
  a.has_normal = with_normals && !(nx == 0.0f && ny == 0.0f && nz == 0.0f);
  a.normal_edge = false;
  return a;
}

// the plain form: 256 consecutive pixels of one view per workgroup, every window pixel from global memory
__global__ __launch_bounds__(kThreads) void map_edges_plain(const float* __restrict__ zmap, const float* __restrict__ normals, int32_t H,
                                                            int32_t W, int32_t hw, int32_t per_view, int32_t r, float rel_tol,
                                                            float min_cos, uint8_t* __restrict__ flags) {
  const int32_t s = (int32_t)blockIdx.x / per_view;
  const int64_t q = (int64_t)((int32_t)blockIdx.x - s * per_view) * kThreads + threadIdx.x;
  if (q >= hw) return;
  const int32_t py = (int32_t)(q / W), px = (int32_t)(q - (int64_t)py * W);
  const int64_t base = (int64_t)s * hw, g = base + q;
  const float zp = zmap[g];
  if (!(zp == zp)) {
    flags[g] = (uint8_t)OVG_MAP_UNUSABLE;
    return;
  }
  const bool wn = normals != nullptr;
  EdgeAcc a = edge_acc(zp, wn ? normals[3 * g] : 0.0f, wn ? normals[3 * g + 1] : 0.0f, wn ? normals[3 * g + 2] : 0.0f, wn, min_cos);
  const int32_t y0 = py - r < 0 ? 0 : py - r, y1 = py + r > H - 1 ? H - 1 : py + r;
  const int32_t x0 = px - r < 0 ? 0 : px - r, x1 = px + r > W - 1 ? W - 1 : px + r;
  for (int32_t yy = y0; yy <= y1; ++yy)
    for (int32_t xx = x0; xx <= x1; ++xx) {
      const int64_t gq = base + (int64_t)yy * W + xx;
      const float zq = zmap[gq];
      if (wn && a.has_normal && zq == zq) a.see(zq, normals[3 * gq], normals[3 * gq + 1], normals[3 * gq + 2]);
      else a.see(zq, 0.0f, 0.0f, 0.0f);
    }
  flags[g] = a.flags(zp, rel_tol);
}

// the staged form: the TW x TH tile of a workgroup plus a halo of r pixels in LDS (pixels outside the view as NaN: not usable, which
// is the clipping of the window), then up to 49 LDS reads per pixel.
template <int TW, int TH>
__global__ __launch_bounds__(kThreads) void map_edges_lds(const float* __restrict__ zmap, const float* __restrict__ normals, int32_t H,
                                                          int32_t W, int32_t r, float rel_tol, float min_cos, int32_t tiles_x,
                                                          int32_t per_view, uint8_t* __restrict__ flags) {
  static_assert(TW * TH == kThreads, "one thread per pixel of the tile");
  constexpr int LW = TW + 2 * kR, LH = TH + 2 * kR;
  __shared__ float sz[LH * LW];
  __shared__ float sn[3][LH * LW];
  const int32_t s = (int32_t)blockIdx.x / per_view, tile = (int32_t)blockIdx.x - s * per_view;
  const int32_t tile_y = tile / tiles_x, tile_x = tile - tile_y * tiles_x;
  const int32_t ox = tile_x * TW - r, oy = tile_y * TH - r;               // the view coordinates of the staged block's corner
  const int32_t lw = TW + 2 * r, lh = TH + 2 * r;                         // <= LW, LH: r <= kR (checked by the entry)
  const int64_t base = (int64_t)s * ((int64_t)H * W);
  const bool wn = normals != nullptr;
  for (int32_t i = (int32_t)threadIdx.x; i < lw * lh; i += kThreads) {
    const int32_t ly = i / lw, lx = i - ly * lw, gx = ox + lx, gy = oy + ly;
    const bool in = gx >= 0 && gx < W && gy >= 0 && gy < H;
    const int64_t gq = base + (int64_t)gy * W + gx;                       // only dereferenced when `in`
    const int32_t at = ly * LW + lx;
    sz[at] = in ? zmap[gq] : quiet_nan();
    if (wn) {
      sn[0][at] = in ? normals[3 * gq] : 0.0f;
      sn[1][at] = in ? normals[3 * gq + 1] : 0.0f;
      sn[2][at] = in ? normals[3 * gq + 2] : 0.0f;
    }
  }
  __syncthreads();
  const int32_t tx = (int32_t)threadIdx.x % TW, ty = (int32_t)threadIdx.x / TW;
  const int32_t px = tile_x * TW + tx, py = tile_y * TH + ty;
  if (px >= W || py >= H) return;
  const int64_t g = base + (int64_t)py * W + px;
  const int32_t c = (ty + r) * LW + (tx + r);
  const float zp = sz[c];
  if (!(zp == zp)) {
    flags[g] = (uint8_t)OVG_MAP_UNUSABLE;
    return;
  }
  EdgeAcc a = edge_acc(zp, wn ? sn[0][c] : 0.0f, wn ? sn[1][c] : 0.0f, wn ? sn[2][c] : 0.0f, wn, min_cos);
  for (int32_t dy = -r; dy <= r; ++dy)
    for (int32_t dx = -r; dx <= r; ++dx) {
      const int32_t at = c + dy * LW + dx;                                // inside the staged block: |dy|, |dx| <= r
      if (wn && a.has_normal) a.see(sz[at], sn[0][at], sn[1][at], sn[2][at]);
      else a.see(sz[at], 0.0f, 0.0f, 0.0f);
    }
  flags[g] = a.flags(zp, rel_tol);
}

template <int TW, int TH>
int edges_launch(const ovg_map_edges_params* p, hipStream_t st) {
  const int32_t tiles_x = (p->W + TW - 1) / TW, tiles_y = (p->H + TH - 1) / TH;     // S tiles_x tiles_y <= S H W < 2^31
  OVG_LAUNCH((map_edges_lds<TW, TH>), dim3((unsigned)(p->S * tiles_x * tiles_y)), dim3(kThreads), 0, st, p->z, p->normals, p->H, p->W,
             p->radius, p->rel_tol, p->min_cos, tiles_x, tiles_x * tiles_y, p->flags);
  OVG_CHECK_LAUNCH();
  return OVG_OK;
}

// ---------------------------------------------------------------------------------------------------------------------------------
// ovg_map_triangulate: face bits per quad, referenced pixels, two scans of per-workgroup counts, two scatters (the shape of
// ovg_tsdf_extract)
// ---------------------------------------------------------------------------------------------------------------------------------
int64_t tri_blocks(int64_t n) { return (n + kThreads - 1) / kThreads; }
int64_t tri_ws_bytes(int64_t n) { return round256(4 * n) + round256(n) + 2 * round256(8 * tri_blocks(n)); }

struct TriWs { int32_t* vidx; uint8_t* fmask; int64_t* voff; int64_t* foff; };
TriWs tri_ws(void* ws, int64_t n) {
  char* b = static_cast<char*>(ws);
  TriWs w;
  w.vidx = reinterpret_cast<int32_t*>(b);
  w.fmask = reinterpret_cast<uint8_t*>(b + round256(4 * n));
  w.voff = reinterpret_cast<int64_t*>(b + round256(4 * n) + round256(n));
  w.foff = reinterpret_cast<int64_t*>(b + round256(4 * n) + round256(n) + round256(8 * tri_blocks(n)));
  return w;
}

struct Pixel { int64_t g; int32_t x, y; bool in; };
OVG_DEV Pixel pixel_of(const ovg_map_triangulate_params& p, int64_t n) {
  Pixel l;
  l.g = (int64_t)blockIdx.x * kThreads + threadIdx.x;
  l.in = l.g < n;
  const int64_t g = l.in ? l.g : 0;
  const int64_t row = g / p.W;
  l.x = (int32_t)(g - row * p.W);
  l.y = (int32_t)(row % p.H);
  return l;
}

OVG_DEV bool torn(float z0, float z1, float z2, float rel_tol) {
  float mx = z0 > z1 ? z0 : z1, mn = z0 < z1 ? z0 : z1;
  mx = mx > z2 ? mx : z2;
  mn = mn < z2 ? mn : z2;
  return mx - mn > rel_tol * mn;
}

// the two face bits of every quad, faces per workgroup
__global__ __launch_bounds__(kThreads) void tri_mark_faces(ovg_map_triangulate_params p, TriWs ws, int64_t n) {
  __shared__ uint32_t wsum[kThreads / 64];
  const Pixel l = pixel_of(p, n);
  uint32_t mask = 0;
  if (l.in && l.x < p.W - 1 && l.y < p.H - 1) {
    const int64_t at[4] = {l.g, l.g + 1, l.g + p.W, l.g + p.W + 1};       // a, b, c, d: the same view (y < H - 1)
    float z[4];
    bool corner[4];
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      z[k] = p.z[at[k]];
      corner[k] = z[k] == z[k] && finite3(p.points + 3 * at[k]) && (!p.keep || p.keep[at[k]] != 0);
    }
    if (corner[0] && corner[2] && corner[1] && !torn(z[0], z[2], z[1], p.rel_tol)) mask |= 1u;
    if (corner[1] && corner[2] && corner[3] && !torn(z[1], z[2], z[3], p.rel_tol)) mask |= 2u;
  }
  if (l.in) ws.fmask[l.g] = (uint8_t)mask;
  uint32_t total;
  block_excl_scan<kThreads>(__popc(mask), wsum, total);
  if (threadIdx.x == 0) ws.foff[blockIdx.x] = total;
}

// the pixels an emitted face names: vidx = 0 / -1, vertices per workgroup
__global__ __launch_bounds__(kThreads) void tri_mark_vertices(ovg_map_triangulate_params p, TriWs ws, int64_t n) {
  __shared__ uint32_t wsum[kThreads / 64];
  const Pixel l = pixel_of(p, n);
  bool ref = false;
  if (l.in) {
    ref = (ws.fmask[l.g] & 1u) != 0;                                                      // a of its own quad's face 0
    if (l.x > 0) ref = ref || (ws.fmask[l.g - 1] & 3u) != 0;                              // b of the quad to the left: both faces
    if (l.y > 0) ref = ref || (ws.fmask[l.g - p.W] & 3u) != 0;                            // c of the quad above: both faces
    if (l.x > 0 && l.y > 0) ref = ref || (ws.fmask[l.g - p.W - 1] & 2u) != 0;             // d of the quad above left: face 1
    ws.vidx[l.g] = ref ? 0 : -1;
  }
  uint32_t total;
  block_excl_scan<kThreads>(ref, wsum, total);
  if (threadIdx.x == 0) ws.voff[blockIdx.x] = total;
}

// exclusive scans of the two per-workgroup count arrays in place, one workgroup of 1024 threads; the totals are the mesh sizes
__global__ __launch_bounds__(1024) void tri_scan(TriWs ws, int64_t nblk, int64_t* out_count) {
  for (int which = 0; which < 2; ++which) {
    int64_t* counts = which ? ws.foff : ws.voff;
    __syncthreads();                                                      // the two scans share their LDS
    const int64_t total = count_scan(counts, counts, nblk);
    if (threadIdx.x == 0) out_count[which] = total;
  }
}

// the vertex of every referenced pixel, in ascending flat index; vidx receives the vertex index
__global__ __launch_bounds__(kThreads) void tri_vertices(ovg_map_triangulate_params p, TriWs ws, int64_t n) {
  __shared__ uint32_t wsum[kThreads / 64];
  const Pixel l = pixel_of(p, n);
  const bool active = l.in && ws.vidx[l.g] >= 0;
  uint32_t total;
  const uint32_t rank = block_excl_scan<kThreads>(active, wsum, total);
  if (!active) return;
  const int64_t pos = ws.voff[blockIdx.x] + rank;                         // <= the number of pixels < 2^31
  ws.vidx[l.g] = (int32_t)pos;
  if (pos < 0 || pos >= p.vertex_capacity) return;                        // also a workspace that COUNT did not fill: never out of bounds
  const float* src = p.points + 3 * l.g;
  float* v = p.out_vertices + 3 * pos;
  float* nrm = p.out_normals + 3 * pos;
  uint8_t* col = p.out_colors + 3 * pos;
#pragma unroll
  for (int k = 0; k < 3; ++k) {
    v[k] = src[k];
    nrm[k] = p.normals ? p.normals[3 * l.g + k] : 0.0f;
    col[k] = p.colors ? p.colors[3 * l.g + k] : (uint8_t)OVG_TSDF_GREY;
  }
  p.out_pixel_index[pos] = l.g;
}

// the faces of every quad, in ascending (pixel, which of the two)
__global__ __launch_bounds__(kThreads) void tri_faces(ovg_map_triangulate_params p, TriWs ws, int64_t n) {
  __shared__ uint32_t wsum[kThreads / 64];
  const Pixel l = pixel_of(p, n);
  // tri_mark_faces' position test again: a workspace that COUNT did not fill must not send a read out of bounds
  const uint32_t mask = l.in && l.x < p.W - 1 && l.y < p.H - 1 ? ws.fmask[l.g] & 3u : 0u;
  uint32_t total;
  const uint32_t rank = block_excl_scan<kThreads>(__popc(mask), wsum, total);
  if (!mask) return;
  int64_t pos = ws.foff[blockIdx.x] + rank;
  if (pos < 0) return;
  const int32_t a = ws.vidx[l.g], b = ws.vidx[l.g + 1], c = ws.vidx[l.g + p.W], d = ws.vidx[l.g + p.W + 1];
  if (mask & 1u) {
    if (pos < p.face_capacity) {
      int32_t* f = p.out_faces + 3 * pos;
      f[0] = a; f[1] = c; f[2] = b;
    }
    ++pos;
  }
  if ((mask & 2u) && pos < p.face_capacity) {
    int32_t* f = p.out_faces + 3 * pos;
    f[0] = b; f[1] = c; f[2] = d;
  }
}

}  // namespace

extern "C" int ovg_map_depth(const ovg_map_depth_params* p, void* stream) {
  if (!p || !p->z || (p->points != nullptr) == (p->depth != nullptr) || (p->points && !p->cams)) return OVG_E_ARG;
  if (!map_shape_ok(p->S, p->H, p->W) || !pos_finite(p->near)) return OVG_E_ARG;
  if (!al(p->points, 4) || !al(p->cams, 4) || !al(p->depth, 4) || !al(p->z, 4)) return OVG_E_ARG;
  const int32_t hw = p->H * p->W, per_view = per_view_blocks(hw);
  OVG_LAUNCH(map_depth_kernel, dim3((unsigned)(p->S * per_view)), dim3(kThreads), 0, static_cast<hipStream_t>(stream), p->points, p->cams,
             p->depth, p->valid, p->z, hw, per_view, p->near);
  OVG_CHECK_LAUNCH();
  return OVG_OK;
}

extern "C" int ovg_map_normals(const ovg_map_normals_params* p, void* stream) {
  if (!p || !p->points || !p->z || !p->normals) return OVG_E_ARG;
  if (!map_shape_ok(p->S, p->H, p->W) || !tol_ok(p->rel_tol)) return OVG_E_ARG;
  if (!al(p->points, 4) || !al(p->z, 4) || !al(p->normals, 4)) return OVG_E_ARG;
  const int32_t hw = p->H * p->W, per_view = per_view_blocks(hw);
  OVG_LAUNCH(map_normals_kernel, dim3((unsigned)(p->S * per_view)), dim3(kThreads), 0, static_cast<hipStream_t>(stream), p->points, p->z, p->H,
             p->W, hw, per_view, p->rel_tol, p->normals);
  OVG_CHECK_LAUNCH();
  return OVG_OK;
}

extern "C" int ovg_map_edges(const ovg_map_edges_params* p, void* stream) {
  if (!p || !p->z || !p->flags) return OVG_E_ARG;
  if (!map_shape_ok(p->S, p->H, p->W) || p->radius < 1 || p->radius > kR || !tol_ok(p->rel_tol)) return OVG_E_ARG;
  if (p->normals && p->min_cos != p->min_cos) return OVG_E_ARG;
  if (p->tile < OVG_MAP_TILE_DEFAULT || p->tile > OVG_MAP_TILE_64x4) return OVG_E_ARG;
  if (!al(p->z, 4) || !al(p->normals, 4)) return OVG_E_ARG;
  hipStream_t st = static_cast<hipStream_t>(stream);
  switch (p->tile) {
    case OVG_MAP_TILE_256x1: break;                                       // the plain form, below
    case OVG_MAP_TILE_32x8: return edges_launch<32, 8>(p, st);
    case OVG_MAP_TILE_64x4: return edges_launch<64, 4>(p, st);
    default: return edges_launch<16, 16>(p, st);                          // OVG_MAP_TILE_DEFAULT, OVG_MAP_TILE_16x16: profiles/mapgeom_probe.txt
  }
  const int32_t hw = p->H * p->W, per_view = per_view_blocks(hw);
  OVG_LAUNCH(map_edges_plain, dim3((unsigned)(p->S * per_view)), dim3(kThreads), 0, st, p->z, p->normals, p->H, p->W, hw, per_view, p->radius,
             p->rel_tol, p->min_cos, p->flags);
  OVG_CHECK_LAUNCH();
  return OVG_OK;
}

extern "C" int64_t ovg_map_triangulate_workspace_bytes(int32_t S, int32_t H, int32_t W) {
  return map_shape_ok(S, H, W) ? tri_ws_bytes((int64_t)S * H * W) : -1;
}

extern "C" int ovg_map_triangulate(const ovg_map_triangulate_params* p, void* stream) {
  if (!p || !p->z || !p->points || !p->ws || !p->out_count) return OVG_E_ARG;
  if (!map_shape_ok(p->S, p->H, p->W) || !tol_ok(p->rel_tol)) return OVG_E_ARG;
  if (p->stage < OVG_MAP_COUNT || p->stage > (OVG_MAP_COUNT | OVG_MAP_SCATTER)) return OVG_E_ARG;
  const int64_t n = (int64_t)p->S * p->H * p->W;
  if (!al(p->z, 4) || !al(p->points, 4) || !al(p->normals, 4) || !al(p->out_count, 8)) return OVG_E_ARG;
  if (!al(p->ws, 16) || p->ws_bytes < tri_ws_bytes(n)) return OVG_E_ARG;
  if (p->stage & OVG_MAP_SCATTER) {
    if (p->vertex_capacity < 0 || p->face_capacity < 0) return OVG_E_ARG;
    if (p->vertex_capacity > 0 && (!p->out_vertices || !p->out_normals || !p->out_colors || !p->out_pixel_index)) return OVG_E_ARG;
    if (p->face_capacity > 0 && !p->out_faces) return OVG_E_ARG;
    if (!al(p->out_vertices, 4) || !al(p->out_normals, 4) || !al(p->out_pixel_index, 8) || !al(p->out_faces, 4)) return OVG_E_ARG;
  }
  hipStream_t st = static_cast<hipStream_t>(stream);
  const TriWs ws = tri_ws(p->ws, n);
  const int64_t nblk = tri_blocks(n);                                     // <= 2^23
  if (p->stage & OVG_MAP_COUNT) {
    OVG_LAUNCH(tri_mark_faces, dim3((unsigned)nblk), dim3(kThreads), 0, st, *p, ws, n);
    OVG_CHECK_LAUNCH();
    OVG_LAUNCH(tri_mark_vertices, dim3((unsigned)nblk), dim3(kThreads), 0, st, *p, ws, n);
    OVG_CHECK_LAUNCH();
    OVG_LAUNCH(tri_scan, dim3(1), dim3(1024), 0, st, ws, nblk, p->out_count);
    OVG_CHECK_LAUNCH();
  }
  if (p->stage & OVG_MAP_SCATTER) {
    OVG_LAUNCH(tri_vertices, dim3((unsigned)nblk), dim3(kThreads), 0, st, *p, ws, n);
    OVG_CHECK_LAUNCH();
    OVG_LAUNCH(tri_faces, dim3((unsigned)nblk), dim3(kThreads), 0, st, *p, ws, n);
    OVG_CHECK_LAUNCH();
  }
  return OVG_OK;
}
