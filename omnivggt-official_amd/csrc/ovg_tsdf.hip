// Volumetric fusion (ovg_tsdf_integrate, ovg_tsdf_extract): S depth maps averaged into a dense truncated signed-distance volume, and
// the mesh of its zero level by naive surface nets. The integration is the consistency kernel's loop turned round: one thread per
// lattice point, the views in a loop, the shared projection of ovg_project.h and one gathered 4-byte depth read per (point, view);
// the state of a point lives in registers across the loop. No atomics anywhere: fixed view order per point, counts and scans for the
// mesh, so two runs give identical bytes.
#include "ovg_geom.h"
#include "ovg_project.h"

// tests/tsdf_twin.py restates both rules in numpy float32, one rounding per operation: no fused multiply-adds in this unit
// (build.py compiles it with -ffp-contract=off as well)
#pragma clang fp contract(off)

namespace {

constexpr int kThreads = 256;
static_assert(kThreads == OVG_TSDF_EXTRACT_BLOCK, "one lattice point per thread of an extraction workgroup");

OVG_DEV float min_lt(float a, float b) { return a < b ? a : b; }          // the twin's fmin: NaN in a gives b, NaN in b gives b
bool pos_finite(float v) { return v > 0.0f && v <= 3.402823466e38f; }
bool finite_host(float v) { return v >= -3.402823466e38f && v <= 3.402823466e38f; }
bool dims_ok(int32_t nx, int32_t ny, int32_t nz) {
  // each factor < 2^31: the first product is below 2^62, and it is below 2^31 before the second one is formed
  return nx > 0 && ny > 0 && nz > 0 && (int64_t)nx * ny < (1ll << 31) && (int64_t)nx * ny * nz < (1ll << 31);
}

// ---------------------------------------------------------------------------------------------------------------------------------
// integration
// ---------------------------------------------------------------------------------------------------------------------------------
// TX x TY x TZ = 256 lattice points per workgroup; thread t is point (t % TX, t / TX % TY, t / (TX TY)) of the brick, so a wave covers a
// compact piece of the lattice and its 64 projections into a view stay close together. The view index is loop-uniform: the camera row
// is read with scalar loads.
template <int TX, int TY, int TZ, bool kColor>
__global__ __launch_bounds__(kThreads) void tsdf_integrate(ovg_tsdf_integrate_params p, int32_t bricks_x, int32_t bricks_y) {
  static_assert(TX * TY * TZ == kThreads, "one thread per lattice point of the brick");
  const int32_t b = (int32_t)blockIdx.x;
  const int32_t bz = b / (bricks_x * bricks_y), rem = b - bz * (bricks_x * bricks_y), by = rem / bricks_x, bx = rem - by * bricks_x;
  const int32_t t = (int32_t)threadIdx.x;
  const int32_t i = bx * TX + t % TX, j = by * TY + t / TX % TY, k = bz * TZ + t / (TX * TY);
  if (i >= p.nx || j >= p.ny || k >= p.nz) return;
  const int64_t g = ((int64_t)k * p.ny + j) * p.nx + i;                   // < 2^31 (checked by the entry)
  const float x = p.origin[0] + p.voxel * (float)i, y = p.origin[1] + p.voxel * (float)j, z = p.origin[2] + p.voxel * (float)k;
  float T = p.tsdf[g], Wt = p.weight[g];
  f32x4 C = {0.0f, 0.0f, 0.0f, 0.0f};
  if (kColor) C = *reinterpret_cast<const f32x4*>(p.color + 4 * g);
  const float hi_u = (float)(p.W - 1), hi_w = (float)(p.H - 1);           // small integers: exact in f32
  const int32_t hw = p.H * p.W;
  const float neg_trunc = -p.trunc;
  for (int32_t s = p.view_first; s < p.view_first + p.view_count; ++s) {
    float zc, u, w;
    if (!project_point(p.cams + 16 * (int64_t)s, x, y, z, p.near, zc, u, w)) continue;
    if (!(u >= 0.0f && u <= hi_u && w >= 0.0f && w <= hi_w)) continue;    // NaN fails; past this line the conversions are in range
    const int64_t q = (int64_t)s * hw + ((int32_t)w * p.W + (int32_t)u);  // < S H W < 2^31
    const float d = p.depth[q];
    if (!(finite_f32(d) && d > p.near)) continue;
    if (p.valid && p.valid[q] == 0) continue;
    float wobs = 1.0f;
    if (p.obs_weight) {
      wobs = p.obs_weight[q];
      if (!(finite_f32(wobs) && wobs > 0.0f)) continue;
    }
    const float sdf = d - zc;
    if (sdf < neg_trunc) continue;
    const float tt = min_lt(__fdiv_rn(sdf, p.trunc), 1.0f);
    const float Wn = Wt + wobs;
    T = __fdiv_rn(T * Wt + tt * wobs, Wn);
    Wt = min_lt(Wn, p.max_weight);
    if (kColor) {
      if (sdf <= p.trunc) {
        const uint8_t* c = p.colors + 3 * q;
        const float Cw = C[3], Cn = Cw + wobs;
        C[0] = __fdiv_rn(C[0] * Cw + (float)c[0] * wobs, Cn);
        C[1] = __fdiv_rn(C[1] * Cw + (float)c[1] * wobs, Cn);
        C[2] = __fdiv_rn(C[2] * Cw + (float)c[2] * wobs, Cn);
        C[3] = min_lt(Cn, p.max_weight);
      }
    }
  }
  p.tsdf[g] = T;
  p.weight[g] = Wt;
  if (kColor) *reinterpret_cast<f32x4*>(p.color + 4 * g) = C;
}

template <int TX, int TY, int TZ>
int integrate_launch(const ovg_tsdf_integrate_params* p, hipStream_t st) {
  const int32_t bx = (p->nx + TX - 1) / TX, by = (p->ny + TY - 1) / TY, bz = (p->nz + TZ - 1) / TZ;
  const int64_t bricks = (int64_t)bx * by * bz;                           // every brick holds a lattice point: <= nx ny nz < 2^31
  if (p->colors)
    OVG_LAUNCH((tsdf_integrate<TX, TY, TZ, true>), dim3((unsigned)bricks), dim3(kThreads), 0, st, *p, bx, by);
  else
    OVG_LAUNCH((tsdf_integrate<TX, TY, TZ, false>), dim3((unsigned)bricks), dim3(kThreads), 0, st, *p, bx, by);
  OVG_CHECK_LAUNCH();
  return OVG_OK;
}

// ---------------------------------------------------------------------------------------------------------------------------------
// extraction
// ---------------------------------------------------------------------------------------------------------------------------------
struct ExWs {
  int32_t* vidx;        // [n]: -1, or >= 0 for the lattice point of an active cell (COUNT: 0; SCATTER: its vertex index)
  uint8_t* qmask;       // [n]: bit a set when the lattice edge along axis a emits a quad
  int64_t* voff;        // [blocks]: vertices per workgroup, then their exclusive scan
  int64_t* qoff;        // [blocks]: quads per workgroup, then their exclusive scan
};

int64_t ex_blocks(int64_t n) { return (n + kThreads - 1) / kThreads; }
int64_t ex_ws_bytes(int64_t n) { return round256(4 * n) + round256(n) + 2 * round256(8 * ex_blocks(n)); }
ExWs ex_ws(void* ws, int64_t n) {
  uint8_t* b = static_cast<uint8_t*>(ws);
  const int64_t o1 = round256(4 * n), o2 = o1 + round256(n), o3 = o2 + round256(8 * ex_blocks(n));
  return {reinterpret_cast<int32_t*>(b), b + o1, reinterpret_cast<int64_t*>(b + o2), reinterpret_cast<int64_t*>(b + o3)};
}

struct Lattice {
  int32_t i, j, k;
  int64_t g;
  bool in;
};

OVG_DEV Lattice lattice_of(const ovg_tsdf_extract_params& p, int64_t n) {
  Lattice l;
  l.g = (int64_t)blockIdx.x * kThreads + threadIdx.x;
  l.in = l.g < n;
  const int64_t g = l.in ? l.g : 0;
  const int64_t row = g / p.nx;
  l.i = (int32_t)(g - row * p.nx);
  l.k = (int32_t)(row / p.ny);
  l.j = (int32_t)(row - (int64_t)l.k * p.ny);
  return l;
}

// the active cells: vidx = 0 / -1 per lattice point, vertices per workgroup
__global__ __launch_bounds__(kThreads) void ex_cells(ovg_tsdf_extract_params p, ExWs ws, int64_t n) {
  __shared__ uint32_t wsum[kThreads / 64];
  const Lattice l = lattice_of(p, n);
  bool active = false;
  if (l.in && l.i < p.nx - 1 && l.j < p.ny - 1 && l.k < p.nz - 1) {
    const int64_t sy = p.nx, sz = (int64_t)p.nx * p.ny;
    bool all_obs = true;
    int inside = 0;
#pragma unroll
    for (int c = 0; c < 8; ++c) {
      const int64_t q = l.g + (c & 1) + ((c >> 1) & 1) * sy + ((c >> 2) & 1) * sz;
      all_obs = all_obs && p.weight[q] >= p.min_weight;
      inside += p.tsdf[q] < 0.0f;
    }
    active = all_obs && inside > 0 && inside < 8;
  }
  if (l.in) ws.vidx[l.g] = active ? 0 : -1;
  uint32_t total;
  block_excl_scan<kThreads>(active, wsum, total);
  if (threadIdx.x == 0) ws.voff[blockIdx.x] = total;
}

// the quads of every lattice point from the active cells: qmask, quads per workgroup
__global__ __launch_bounds__(kThreads) void ex_quads(ovg_tsdf_extract_params p, ExWs ws, int64_t n) {
  __shared__ uint32_t wsum[kThreads / 64];
  const Lattice l = lattice_of(p, n);
  uint32_t mask = 0;
  if (l.in) {
    const int32_t dims[3] = {p.nx, p.ny, p.nz}, at[3] = {l.i, l.j, l.k};
    const int64_t stride[3] = {1, p.nx, (int64_t)p.nx * p.ny};
    const bool obs0 = p.weight[l.g] >= p.min_weight, in0 = p.tsdf[l.g] < 0.0f;
#pragma unroll
    for (int a = 0; a < 3; ++a) {
      const int b = (a + 1) % 3, c = (a + 2) % 3;
      if (!(obs0 && at[a] <= dims[a] - 2 && at[b] >= 1 && at[b] <= dims[b] - 2 && at[c] >= 1 && at[c] <= dims[c] - 2)) continue;
      const int64_t up = l.g + stride[a];
      if (!(p.weight[up] >= p.min_weight) || (p.tsdf[up] < 0.0f) == in0) continue;
      const bool ring = ws.vidx[l.g - stride[b] - stride[c]] >= 0 && ws.vidx[l.g - stride[c]] >= 0 && ws.vidx[l.g] >= 0 &&
                        ws.vidx[l.g - stride[b]] >= 0;
      if (ring) mask |= 1u << a;
    }
    ws.qmask[l.g] = (uint8_t)mask;
  }
  uint32_t total;
  block_excl_scan<kThreads>(__popc(mask), wsum, total);
  if (threadIdx.x == 0) ws.qoff[blockIdx.x] = total;
}

// exclusive scans of the two per-workgroup count arrays in place, one workgroup of 1024 threads; the totals are the mesh sizes
__global__ __launch_bounds__(1024) void ex_scan(ExWs ws, int64_t nblk, int64_t* out_count) {
  for (int which = 0; which < 2; ++which) {
    int64_t* counts = which ? ws.qoff : ws.voff;
    __syncthreads();                                                      // the two scans share their LDS
    const int64_t total = count_scan(counts, counts, nblk);
    if (threadIdx.x == 0) out_count[which] = total;
  }
}

// the vertex of every active cell, in ascending cell index; vidx receives the vertex index
__global__ __launch_bounds__(kThreads) void ex_vertices(ovg_tsdf_extract_params p, ExWs ws, int64_t n) {
  __shared__ uint32_t wsum[kThreads / 64];
  const Lattice l = lattice_of(p, n);
  // the position tests repeat ex_cells': a workspace that COUNT did not fill must not send a read or a write out of bounds
  const bool active = l.in && l.i < p.nx - 1 && l.j < p.ny - 1 && l.k < p.nz - 1 && ws.vidx[l.g] >= 0;
  uint32_t total;
  const uint32_t rank = block_excl_scan<kThreads>(active, wsum, total);
  if (!active) return;
  const int64_t pos = ws.voff[blockIdx.x] + rank;                         // <= the number of cells < 2^31
  ws.vidx[l.g] = (int32_t)pos;
  if (pos < 0 || pos >= p.vertex_capacity) return;
  const int64_t sy = p.nx, sz = (int64_t)p.nx * p.ny;
  float T[8];
#pragma unroll
  for (int c = 0; c < 8; ++c) T[c] = p.tsdf[l.g + (c & 1) + ((c >> 1) & 1) * sy + ((c >> 2) & 1) * sz];
  float off[3] = {0.0f, 0.0f, 0.0f}, cnt = 0.0f, g[3];
#pragma unroll
  for (int e = 0; e < 12; ++e) {
    // the fixed edge order of the header: the x edges, the y edges, the z edges, each over the two other offsets (lower axis first)
    const int axis = e >> 2, m = e & 3;
    const int a = axis == 0 ? 2 * m : axis == 1 ? (m & 1) + 4 * (m >> 1) : m, b = a + (1 << axis);
    if ((T[a] < 0.0f) == (T[b] < 0.0f)) continue;
    const float r = __fdiv_rn(T[a], T[a] - T[b]);
    off[0] = off[0] + (axis == 0 ? r : (float)(a & 1));
    off[1] = off[1] + (axis == 1 ? r : (float)((a >> 1) & 1));
    off[2] = off[2] + (axis == 2 ? r : (float)((a >> 2) & 1));
    cnt = cnt + 1.0f;
  }
  const int32_t at[3] = {l.i, l.j, l.k};
  float* v = p.vertices + 3 * pos;
#pragma unroll
  for (int q = 0; q < 3; ++q) v[q] = p.origin[q] + p.voxel * ((float)at[q] + __fdiv_rn(off[q], cnt));
  g[0] = (((T[1] - T[0]) + (T[3] - T[2])) + (T[5] - T[4])) + (T[7] - T[6]);
  g[1] = (((T[2] - T[0]) + (T[3] - T[1])) + (T[6] - T[4])) + (T[7] - T[5]);
  g[2] = (((T[4] - T[0]) + (T[5] - T[1])) + (T[6] - T[2])) + (T[7] - T[3]);
  // the float64 root rounded once more is the correctly rounded float32 root (53 >= 2 * 24 + 2 bits: the second rounding is innocuous);
  // hipcc's float32 square root is the hardware approximation, an ulp off in places
  const float len = (float)sqrt((double)((g[0] * g[0] + g[1] * g[1]) + g[2] * g[2]));
  const bool good = len > 0.0f;
  float* nrm = p.normals + 3 * pos;
#pragma unroll
  for (int q = 0; q < 3; ++q) nrm[q] = good ? __fdiv_rn(g[q], len) : 0.0f;
  uint8_t* col = p.colors + 3 * pos;
  float acc[3] = {0.0f, 0.0f, 0.0f}, have = 0.0f;
  if (p.color) {
#pragma unroll
    for (int c = 0; c < 8; ++c) {
      const f32x4 cc = *reinterpret_cast<const f32x4*>(p.color + 4 * (l.g + (c & 1) + ((c >> 1) & 1) * sy + ((c >> 2) & 1) * sz));
      if (!(cc[3] > 0.0f)) continue;
      acc[0] = acc[0] + cc[0];
      acc[1] = acc[1] + cc[1];
      acc[2] = acc[2] + cc[2];
      have = have + 1.0f;
    }
  }
#pragma unroll
  for (int q = 0; q < 3; ++q) {
    float xq = floorf(__fdiv_rn(acc[q], have) + 0.5f);
    xq = !(xq >= 0.0f) ? 0.0f : (xq > 255.0f ? 255.0f : xq);
    col[q] = have > 0.0f ? (uint8_t)(int)xq : (uint8_t)OVG_TSDF_GREY;
  }
}

// the two triangles of every quad, in ascending (lattice index, axis)
__global__ __launch_bounds__(kThreads) void ex_faces(ovg_tsdf_extract_params p, ExWs ws, int64_t n) {
  __shared__ uint32_t wsum[kThreads / 64];
  const Lattice l = lattice_of(p, n);
  uint32_t mask = l.in ? ws.qmask[l.g] & 7u : 0u;
  const int32_t dims[3] = {p.nx, p.ny, p.nz}, at[3] = {l.i, l.j, l.k};
#pragma unroll
  for (int a = 0; a < 3; ++a) {                                           // ex_quads' position tests again, as in ex_vertices
    const int b = (a + 1) % 3, c = (a + 2) % 3;
    if (!(at[a] <= dims[a] - 2 && at[b] >= 1 && at[b] <= dims[b] - 2 && at[c] >= 1 && at[c] <= dims[c] - 2)) mask &= ~(1u << a);
  }
  uint32_t total;
  const uint32_t rank = block_excl_scan<kThreads>(__popc(mask), wsum, total);
  if (!mask) return;
  int64_t pos = ws.qoff[blockIdx.x] + rank;
  if (pos < 0) return;
  const int64_t stride[3] = {1, p.nx, (int64_t)p.nx * p.ny};
  const bool lower_inside = p.tsdf[l.g] < 0.0f;
#pragma unroll
  for (int a = 0; a < 3; ++a) {
    if (!(mask & (1u << a))) continue;
    const int b = (a + 1) % 3, c = (a + 2) % 3;
    if (pos < p.quad_capacity) {
      const int32_t v0 = ws.vidx[l.g - stride[b] - stride[c]], v1 = ws.vidx[l.g - stride[c]], v2 = ws.vidx[l.g], v3 = ws.vidx[l.g - stride[b]];
      const int32_t q1 = lower_inside ? v1 : v3, q3 = lower_inside ? v3 : v1;
      int32_t* f = p.faces + 6 * pos;
      f[0] = v0; f[1] = q1; f[2] = v2;
      f[3] = v0; f[4] = v2; f[5] = q3;
    }
    ++pos;
  }
}

}  // namespace

extern "C" int ovg_tsdf_integrate(const ovg_tsdf_integrate_params* p, void* stream) {
  if (!p || !p->tsdf || !p->weight || !p->depth || !p->cams || (p->colors && !p->color)) return OVG_E_ARG;
  if (!dims_ok(p->nx, p->ny, p->nz)) return OVG_E_ARG;
  if (!dims_ok(p->W, p->H, p->S)) return OVG_E_ARG;                       // the same test: W H < 2^31 and S H W < 2^31
  if (p->view_first < 0 || p->view_count <= 0 || p->view_first >= p->S || p->view_count > p->S - p->view_first) return OVG_E_ARG;
  if (!pos_finite(p->voxel) || !pos_finite(p->trunc) || !pos_finite(p->max_weight) || !pos_finite(p->near)) return OVG_E_ARG;
  if (!finite_host(p->origin[0]) || !finite_host(p->origin[1]) || !finite_host(p->origin[2])) return OVG_E_ARG;
  if (p->tile < OVG_TSDF_TILE_DEFAULT || p->tile > OVG_TSDF_TILE_32x8x1) return OVG_E_ARG;
  if (!al(p->tsdf, 4) || !al(p->weight, 4) || !al(p->color, 16) || !al(p->depth, 4) || !al(p->cams, 4) || !al(p->obs_weight, 4)) return OVG_E_ARG;
  hipStream_t st = static_cast<hipStream_t>(stream);
  switch (p->tile) {
    case OVG_TSDF_TILE_256x1x1: return integrate_launch<256, 1, 1>(p, st);
    case OVG_TSDF_TILE_8x8x4: return integrate_launch<8, 8, 4>(p, st);
    case OVG_TSDF_TILE_32x8x1: return integrate_launch<32, 8, 1>(p, st);
    default: return integrate_launch<16, 4, 4>(p, st);                    // OVG_TSDF_TILE_DEFAULT, OVG_TSDF_TILE_16x4x4: profiles/tsdf_probe.txt
  }
}

extern "C" int64_t ovg_tsdf_extract_workspace_bytes(int32_t nx, int32_t ny, int32_t nz) {
  return dims_ok(nx, ny, nz) ? ex_ws_bytes((int64_t)nx * ny * nz) : -1;
}

extern "C" int ovg_tsdf_extract(const ovg_tsdf_extract_params* p, void* stream) {
  if (!p || !p->tsdf || !p->weight || !p->ws || !p->out_count) return OVG_E_ARG;
  if (!dims_ok(p->nx, p->ny, p->nz)) return OVG_E_ARG;
  if (!pos_finite(p->voxel) || !pos_finite(p->min_weight)) return OVG_E_ARG;
  if (!finite_host(p->origin[0]) || !finite_host(p->origin[1]) || !finite_host(p->origin[2])) return OVG_E_ARG;
  if (p->stage < OVG_TSDF_COUNT || p->stage > (OVG_TSDF_COUNT | OVG_TSDF_SCATTER)) return OVG_E_ARG;
  const int64_t n = (int64_t)p->nx * p->ny * p->nz;
  if (!al(p->tsdf, 4) || !al(p->weight, 4) || !al(p->color, 16) || !al(p->out_count, 8)) return OVG_E_ARG;
  if (!al(p->ws, 16) || p->ws_bytes < ex_ws_bytes(n)) return OVG_E_ARG;
  if (p->stage & OVG_TSDF_SCATTER) {
    if (p->vertex_capacity < 0 || p->quad_capacity < 0) return OVG_E_ARG;
    if (p->vertex_capacity > 0 && (!p->vertices || !p->normals || !p->colors)) return OVG_E_ARG;
    if (p->quad_capacity > 0 && !p->faces) return OVG_E_ARG;
    if (!al(p->vertices, 4) || !al(p->normals, 4) || !al(p->faces, 4)) return OVG_E_ARG;
  }
  hipStream_t st = static_cast<hipStream_t>(stream);
  const ExWs ws = ex_ws(p->ws, n);
  const int64_t nblk = ex_blocks(n);                                      // <= 2^23
  if (p->stage & OVG_TSDF_COUNT) {
    OVG_LAUNCH(ex_cells, dim3((unsigned)nblk), dim3(kThreads), 0, st, *p, ws, n);
    OVG_CHECK_LAUNCH();
    OVG_LAUNCH(ex_quads, dim3((unsigned)nblk), dim3(kThreads), 0, st, *p, ws, n);
    OVG_CHECK_LAUNCH();
    OVG_LAUNCH(ex_scan, dim3(1), dim3(1024), 0, st, ws, nblk, p->out_count);
    OVG_CHECK_LAUNCH();
  }
  if (p->stage & OVG_TSDF_SCATTER) {
    OVG_LAUNCH(ex_vertices, dim3((unsigned)nblk), dim3(kThreads), 0, st, *p, ws, n);
    OVG_CHECK_LAUNCH();
    OVG_LAUNCH(ex_faces, dim3((unsigned)nblk), dim3(kThreads), 0, st, *p, ws, n);
    OVG_CHECK_LAUNCH();
  }
  return OVG_OK;
}
