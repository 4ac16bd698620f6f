// Mesh cleaning (ovg_mesh_topology, ovg_mesh_select, ovg_mesh_smooth; include/omnivggt_hip.h states the rules, tests/meshops_twin.py
// restates them in numpy): connected components and edge statistics, an ordered sub-mesh, Laplacian / Taubin smoothing with vertex normals.
// One pass over the faces (mo_faces) serves topology and smoothing: a live face marks its corners REFERENCED, hooks (a, b) and (b, c)
// in the union-find of ovg_geom.h, counts two neighbours per corner and adds its three edges to an open-addressing table whose key
// (lo << 32 | hi) is claimed by a 64-bit compare-and-swap; a pass over the slots (mo_edge_pass) turns the per-slot counts into the edge
// statistics and the BOUNDARY / NONMANIFOLD bits. Smoothing builds a CSR adjacency once (count, scan, fill) and then runs two launches per
// step: sm_quantise turns the positions into int32 grid coordinates in the step's frame, sm_update gathers the int64 neighbour sums --
// one thread per vertex, a row of more than 64 neighbours by the whole wave -- moves the vertex and reduces the frame of the next step.
// Integer atomics only, relaxed, agent scope: two runs give identical bytes. The face pass and the fill are bound by random atomics, the
// steps by the gather of 16-byte records; no workgroup waits for another.
#include "ovg_geom.h"

// the quantisation, the update and the normals restate numpy operation for operation: no fused multiply-add in this unit (build.py
// compiles it with -ffp-contract=off as well, which reaches the inlined HIP header helpers)
#pragma clang fp contract(off)

namespace {

constexpr int kThreads = 256;
constexpr int kTile = kThreads * 16;                // entries per workgroup of the scans and the ordered compactions
constexpr uint64_t kNoKey = ~0ull;                  // no edge key: lo < hi < 2^31
constexpr uint32_t kNone = 0xFFFFFFFFu;
constexpr int64_t kMinSlots = 1024;
constexpr int kLongRow = 64;                        // a longer row of the adjacency is summed by the whole wave
constexpr uint32_t kValid = 8u, kMovable = 16u;     // bits of the flag word beside OVG_MT_REFERENCED / BOUNDARY / NONMANIFOLD

struct MoHead {
  unsigned long long live, edges, boundary, nonmanifold, vreferenced, vboundary, vnonmanifold;
  uint32_t flags;                                   // OVG_MT_INTERNAL (topology) or OVG_MSM_NONFINITE (smoothing)
  uint32_t lo[2][3], hi[2][3];                      // smoothing: the order keys of the frame of the even and of the odd steps
};

struct MoEdges { uint64_t* key; uint32_t* cnt; int64_t slots; };

struct MtWs { MoHead* head; uint32_t* vflag; MoEdges edges; };
struct SelWs { uint8_t* vkeep; uint8_t* fkeep; uint32_t* rank; int64_t* vcounts; int64_t* voffsets; int64_t* fcounts; int64_t* foffsets; };
struct SmWs {
  MoHead* head; uint32_t* vflag; MoEdges edges;
  uint32_t* deg; int64_t* row; int64_t* tcounts; int64_t* toffsets; uint32_t* adj;      // row [M + 1], adj [6 F]
  int4* q; uint64_t* nsum;                                                              // q [M], nsum [M][3]
};

int64_t mo_slots(int64_t f) { return 6 * f < kMinSlots ? kMinSlots : 6 * f; }           // <= 3 F edges: load factor <= 1/2
int64_t mo_tiles(int64_t n) { return (n + kTile - 1) / kTile; }
bool mo_sizes_ok(int64_t m, int64_t f) { return size_ok(m) && size_ok(f); }

// -> the bytes of `parts` parts, each rounded up to 256; off[k]: where part k starts
template <int N> int64_t mo_offsets(const int64_t (&part)[N], int64_t (&off)[N]) {
  int64_t total = 0;
  for (int k = 0; k < N; ++k) {
    off[k] = total;
    total += round256(part[k]);
  }
  return total;
}

// the three layouts -> the bytes; with base != nullptr also the pointers
int64_t mt_layout(int64_t m, int64_t f, uint8_t* base, MtWs* ws) {
  const int64_t e = mo_slots(f), part[4] = {256, 4 * m, 8 * e, 4 * e};
  int64_t off[4];
  const int64_t total = mo_offsets(part, off);
  if (base)
    *ws = {reinterpret_cast<MoHead*>(base), reinterpret_cast<uint32_t*>(base + off[1]),
           {reinterpret_cast<uint64_t*>(base + off[2]), reinterpret_cast<uint32_t*>(base + off[3]), e}};
  return total;
}

int64_t sel_layout(int64_t m, int64_t f, uint8_t* base, SelWs* ws) {
  const int64_t vt = mo_tiles(m), ft = mo_tiles(f), part[7] = {m, f, 4 * m, 8 * vt, 8 * vt, 8 * ft, 8 * ft};
  int64_t off[7];
  const int64_t total = mo_offsets(part, off);
  if (base)
    *ws = {base, base + off[1], reinterpret_cast<uint32_t*>(base + off[2]), reinterpret_cast<int64_t*>(base + off[3]),
           reinterpret_cast<int64_t*>(base + off[4]), reinterpret_cast<int64_t*>(base + off[5]), reinterpret_cast<int64_t*>(base + off[6])};
  return total;
}

int64_t sm_layout(int64_t m, int64_t f, uint8_t* base, SmWs* ws) {
  const int64_t e = mo_slots(f), vt = mo_tiles(m);
  const int64_t part[11] = {256, 4 * m, 8 * e, 4 * e, 4 * m, 8 * (m + 1), 8 * vt, 8 * vt, 24 * f, 16 * m, 24 * m};
  int64_t off[11];
  const int64_t total = mo_offsets(part, off);
  if (base)
    *ws = {reinterpret_cast<MoHead*>(base), reinterpret_cast<uint32_t*>(base + off[1]),
           {reinterpret_cast<uint64_t*>(base + off[2]), reinterpret_cast<uint32_t*>(base + off[3]), e},
           reinterpret_cast<uint32_t*>(base + off[4]), reinterpret_cast<int64_t*>(base + off[5]), reinterpret_cast<int64_t*>(base + off[6]),
           reinterpret_cast<int64_t*>(base + off[7]), reinterpret_cast<uint32_t*>(base + off[8]), reinterpret_cast<int4*>(base + off[9]),
           reinterpret_cast<uint64_t*>(base + off[10])};
  return total;
}

template <typename T> OVG_DEV T ld(const T* p) { return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }
template <typename T> OVG_DEV void add(T* p, T v) { __hip_atomic_fetch_add(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }
// bits only ever appear: a word that already shows them needs no atomic
OVG_DEV void raise(uint32_t* p, uint32_t bits) {
  if ((ld(p) & bits) != bits) __hip_atomic_fetch_or(p, bits, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

// the corners of face f -> true when the face is LIVE (rule 2)
OVG_DEV bool live_face(const float* __restrict__ v, const int32_t* __restrict__ faces, int64_t m, int64_t f, int32_t (&c)[3]) {
  c[0] = faces[3 * f], c[1] = faces[3 * f + 1], c[2] = faces[3 * f + 2];
  if ((uint32_t)c[0] >= (uint32_t)m || (uint32_t)c[1] >= (uint32_t)m || (uint32_t)c[2] >= (uint32_t)m) return false;      // m < 2^31
  if (c[0] == c[1] || c[1] == c[2] || c[0] == c[2]) return false;
  return finite3(v + 3 * (int64_t)c[0]) && finite3(v + 3 * (int64_t)c[1]) && finite3(v + 3 * (int64_t)c[2]);
}

// what a call accumulates into, cleared: any of parent, deg, nsum and the edge table may be absent
__global__ __launch_bounds__(kThreads) void mo_clear(MoHead* head, uint32_t* vflag, int64_t m, MoEdges edges, int32_t* parent, uint32_t* deg,
                                                     uint64_t* nsum) {
  const int64_t t0 = (int64_t)blockIdx.x * kThreads + threadIdx.x, step = (int64_t)gridDim.x * kThreads;
  for (int64_t i = t0; i < m; i += step) {
    vflag[i] = 0u;
    if (parent) parent[i] = (int32_t)i;
    if (deg) deg[i] = 0u;
    if (nsum) nsum[3 * i] = 0ull, nsum[3 * i + 1] = 0ull, nsum[3 * i + 2] = 0ull;
  }
  if (edges.key)
    for (int64_t s = t0; s < edges.slots; s += step) {
      edges.key[s] = kNoKey;
      edges.cnt[s] = 0u;
    }
  if (t0 == 0) *head = {0ull, 0ull, 0ull, 0ull, 0ull, 0ull, 0ull, 0u, {{kNone, kNone, kNone}, {kNone, kNone, kNone}}, {{0u, 0u, 0u}, {0u, 0u, 0u}}};
}

// one more face on the edge {a, b}
OVG_DEV void edge_add(const MoEdges& edges, int32_t a, int32_t b) {
  const uint64_t key = a < b ? ((uint64_t)(uint32_t)a << 32) | (uint32_t)b : ((uint64_t)(uint32_t)b << 32) | (uint32_t)a;
  int64_t s = (int64_t)__umul64hi(mix_murmur64(key), (uint64_t)edges.slots);
  for (int64_t t = 0; t < edges.slots; ++t) {        // at most 3 F of the >= 6 F slots are ever claimed: the walk ends at a free one
    uint64_t k = ld(&edges.key[s]);
    if (k == kNoKey) {
      uint64_t expect = kNoKey;
      const bool won = __hip_atomic_compare_exchange_strong(&edges.key[s], &expect, key, __ATOMIC_RELAXED, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      k = won ? key : expect;
    }
    if (k == key) {
      add(&edges.cnt[s], 1u);
      return;
    }
    s = s + 1 == edges.slots ? 0 : s + 1;
  }
}

// one thread per face. A live face marks its corners, hooks (a, b) and (b, c) (parent), counts two neighbours per corner (deg) and adds
// its three edges (edges); whichever of the three the caller does not need is absent
__global__ __launch_bounds__(kThreads) void mo_faces(const float* __restrict__ v, const int32_t* __restrict__ faces, int64_t m, int64_t nf,
                                                     MoHead* head, uint32_t* vflag, MoEdges edges, int32_t* parent, uint32_t* deg) {
  __shared__ uint32_t red[kThreads / 64];
  const int64_t f = (int64_t)blockIdx.x * kThreads + threadIdx.x;
  int32_t c[3];
  const bool live = f < nf && live_face(v, faces, m, f, c);
  if (live) {
#pragma unroll
    for (int k = 0; k < 3; ++k) raise(&vflag[c[k]], (uint32_t)OVG_MT_REFERENCED);
    if (parent) {
      const uint64_t budget = 4ull * (uint64_t)m + 4;
      if (!cl_unite(parent, c[0], c[1], budget) || !cl_unite(parent, c[1], c[2], budget)) raise(&head->flags, (uint32_t)OVG_MT_INTERNAL);
    }
    if (deg) {
#pragma unroll
      for (int k = 0; k < 3; ++k) add(&deg[c[k]], 2u);
    }
    if (edges.key) {
      edge_add(edges, c[0], c[1]);
      edge_add(edges, c[1], c[2]);
      edge_add(edges, c[2], c[0]);
    }
  }
  const uint32_t total = block_reduce<kThreads>((uint32_t)live, red, IntSum());
  if (threadIdx.x == 0 && total) add(&head->live, (unsigned long long)total);
}

// every claimed slot is one distinct edge: the three edge counts, and the BOUNDARY / NONMANIFOLD bits of its two ends. The ends come from
// a table this call filled from live faces: both lie in [0, M)
__global__ __launch_bounds__(kThreads) void mo_edge_pass(MoEdges edges, uint32_t* vflag, MoHead* head) {
  __shared__ uint32_t red[kThreads / 64];
  uint32_t n[3] = {0u, 0u, 0u};
  for (int64_t s = (int64_t)blockIdx.x * kThreads + threadIdx.x; s < edges.slots; s += (int64_t)gridDim.x * kThreads) {
    const uint64_t key = edges.key[s];
    if (key == kNoKey) continue;
    const uint32_t c = edges.cnt[s], bit = c == 1u ? (uint32_t)OVG_MT_BOUNDARY : (c >= 3u ? (uint32_t)OVG_MT_NONMANIFOLD : 0u);
    ++n[0];
    n[1] += c == 1u;
    n[2] += c >= 3u;
    if (bit) {
      raise(&vflag[key >> 32], bit);
      raise(&vflag[(uint32_t)key], bit);
    }
  }
  unsigned long long* out[3] = {&head->edges, &head->boundary, &head->nonmanifold};
#pragma unroll
  for (int k = 0; k < 3; ++k) {
    __syncthreads();                                   // red is read by every thread of the previous round
    const uint32_t t = block_reduce<kThreads>(n[k], red, IntSum());
    if (threadIdx.x == 0 && t) add(out[k], (unsigned long long)t);
  }
}

// thread i: vertex i (its root by a last find, its flags) and face i (the root of its first corner). No hook runs in this launch, so
// every find ends at the tree's final root. An unreferenced vertex is its own tree and on nobody's path: its -1 is a plain store
__global__ __launch_bounds__(kThreads) void mt_finish(ovg_mesh_topology_params p, MtWs ws) {
  __shared__ uint32_t red[kThreads / 64];
  const int64_t i = (int64_t)blockIdx.x * kThreads + threadIdx.x, m = p.num_vertices;
  int32_t* parent = p.vertex_root;
  uint32_t n[3] = {0u, 0u, 0u};
  bool fine = true;
  if (i < m) {
    const uint32_t fl = ws.vflag[i];
    if (fl & OVG_MT_REFERENCED) {
      uint64_t budget = 4ull * (uint64_t)m + 4;
      const int32_t r = cl_find(parent, (int32_t)i, budget);
      fine = r >= 0;
      if (fine) __hip_atomic_fetch_min(parent + i, r, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    } else {
      parent[i] = -1;
    }
    p.vertex_flags[i] = (uint8_t)(fl & 7u);
    n[0] = (fl & OVG_MT_REFERENCED) != 0u, n[1] = (fl & OVG_MT_BOUNDARY) != 0u, n[2] = (fl & OVG_MT_NONMANIFOLD) != 0u;
  }
  if (i < p.num_faces) {
    int32_t c[3], r = -1;
    if (live_face(p.vertices, p.faces, m, i, c)) {
      uint64_t budget = 4ull * (uint64_t)m + 4;
      r = cl_find(parent, c[0], budget);
      fine = fine && r >= 0;
    }
    p.face_root[i] = r;
  }
  if (!fine) raise(&ws.head->flags, (uint32_t)OVG_MT_INTERNAL);
  unsigned long long* out[3] = {&ws.head->vreferenced, &ws.head->vboundary, &ws.head->vnonmanifold};
#pragma unroll
  for (int k = 0; k < 3; ++k) {
    __syncthreads();
    const uint32_t t = block_reduce<kThreads>(n[k], red, IntSum());
    if (threadIdx.x == 0 && t) add(out[k], (unsigned long long)t);
  }
}

__global__ void mt_done(const MoHead* head, int64_t* out_count) {
  const MoHead h = *head;
  const unsigned long long v[8] = {h.live, h.vreferenced, h.edges, h.boundary, h.nonmanifold, h.vboundary, h.vnonmanifold, h.flags};
  for (int k = 0; k < 8; ++k) out_count[k] = (int64_t)v[k];
}

// ---------------------------------------------------------------------------------------------------------------------------------
// ovg_mesh_select
// ---------------------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(kThreads) void sel_clear(SelWs ws, int64_t m, int64_t f) {
  const int64_t t0 = (int64_t)blockIdx.x * kThreads + threadIdx.x, step = (int64_t)gridDim.x * kThreads;
  u32x4* vk = reinterpret_cast<u32x4*>(ws.vkeep);                   // the keep bytes are rounded up to 256: whole 16-byte stores
  u32x4* fk = reinterpret_cast<u32x4*>(ws.fkeep);
  const u32x4 zero = {0u, 0u, 0u, 0u};
  for (int64_t i = t0; i < (m + 15) / 16; i += step) vk[i] = zero;
  for (int64_t i = t0; i < (f + 15) / 16; i += step) fk[i] = zero;
}

// one thread per face: a survivor marks itself and its three corners (several survivors may store the same byte: harmless)
__global__ __launch_bounds__(kThreads) void sel_faces(ovg_mesh_select_params p, SelWs ws) {
  const int64_t f = (int64_t)blockIdx.x * kThreads + threadIdx.x;
  int32_t c[3];
  if (f >= p.num_faces || !live_face(p.vertices, p.faces, p.num_vertices, f, c)) return;
  if (p.face_keep && !p.face_keep[f]) return;
  if (p.vertex_keep && !(p.vertex_keep[c[0]] && p.vertex_keep[c[1]] && p.vertex_keep[c[2]])) return;
  ws.fkeep[f] = 1;
#pragma unroll
  for (int k = 0; k < 3; ++k) ws.vkeep[c[k]] = 1;
}

// blockIdx.x < vtiles: a tile of vertex keep bytes, else a tile of face keep bytes
__global__ __launch_bounds__(kThreads) void sel_tile_counts(SelWs ws, int64_t m, int64_t f, int64_t vtiles) {
  __shared__ int64_t red[kThreads / 64];
  const bool vert = (int64_t)blockIdx.x < vtiles;
  const int64_t tile = vert ? blockIdx.x : blockIdx.x - vtiles, n = vert ? m : f;
  const uint8_t* keep = vert ? ws.vkeep : ws.fkeep;
  int64_t cnt = 0;
#pragma unroll 4
  for (int j = 0; j < kTile / kThreads; ++j) {
    const int64_t i = tile * kTile + (int64_t)j * kThreads + threadIdx.x;
    if (i < n) cnt += keep[i];
  }
  const int64_t t = block_reduce<kThreads>(cnt, red, IntSum());
  if (threadIdx.x == 0) (vert ? ws.vcounts : ws.fcounts)[tile] = t;
}

// the two exclusive scans of the tile counts in one workgroup of 1024 threads, and the two counts
__global__ __launch_bounds__(1024) void sel_scan(SelWs ws, int64_t vtiles, int64_t ftiles, int64_t* out_count) {
  const int64_t mv = count_scan(ws.vcounts, ws.voffsets, vtiles);
  __syncthreads();
  const int64_t mf = count_scan(ws.fcounts, ws.foffsets, ftiles);
  if (threadIdx.x == 0) out_count[0] = mv, out_count[1] = mf;
}

// the output number of every kept vertex
__global__ __launch_bounds__(kThreads) void sel_ranks(SelWs ws, int64_t m) {
  compact_tile<kThreads, kTile>(ws.vkeep, m, ws.voffsets, [&](int64_t i, int64_t pos) { ws.rank[i] = (uint32_t)pos; });
}

__global__ __launch_bounds__(kThreads) void sel_scatter_vertices(ovg_mesh_select_params p, SelWs ws) {
  compact_tile<kThreads, kTile>(ws.vkeep, p.num_vertices, ws.voffsets, [&](int64_t i, int64_t pos) {
    if (pos < 0 || pos >= p.vertex_capacity) return;
#pragma unroll
    for (int k = 0; k < 3; ++k) p.out_vertices[3 * pos + k] = p.vertices[3 * i + k];
    if (p.out_source_index) p.out_source_index[pos] = i;
  });
}

// the survivors in input order, their corners as output vertex numbers
__global__ __launch_bounds__(kThreads) void sel_scatter_faces(ovg_mesh_select_params p, SelWs ws) {
  compact_tile<kThreads, kTile>(ws.fkeep, p.num_faces, ws.foffsets, [&](int64_t f, int64_t pos) {
    if (pos < 0 || pos >= p.face_capacity) return;
#pragma unroll
    for (int k = 0; k < 3; ++k) {
      const int64_t i = p.faces[3 * f + k];
      p.out_faces[3 * pos + k] = i >= 0 && i < p.num_vertices ? (int32_t)ws.rank[i] : -1;      // a survivor's corners are kept vertices
    }
    if (p.out_face_index) p.out_face_index[pos] = f;
  });
}

// ---------------------------------------------------------------------------------------------------------------------------------
// ovg_mesh_smooth
// ---------------------------------------------------------------------------------------------------------------------------------
// min / max of the order keys of a workgroup's positions into one frame of the head; a thread without a position passes (kNone, 0).
// One barrier; an extreme that the head already shows needs no atomic, which is all but a few workgroups of a launch. Every thread calls
// it, once per kernel
OVG_DEV void frame_reduce(MoHead* head, int slot, const uint32_t (&lo)[3], const uint32_t (&hi)[3]) {
  __shared__ uint32_t red[kThreads / 64][6];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
#pragma unroll
  for (int k = 0; k < 3; ++k) {
    const uint32_t a = wave_reduce(lo[k], IntMin()), b = wave_reduce(hi[k], IntMax());
    if (lane == 0) red[wave][k] = a, red[wave][3 + k] = b;
  }
  __syncthreads();
  if (threadIdx.x >= 3) return;
  const int k = threadIdx.x;
  uint32_t a = red[0][k], b = red[0][3 + k];
#pragma unroll
  for (int w = 1; w < kThreads / 64; ++w) a = min(a, red[w][k]), b = max(b, red[w][3 + k]);
  if (a == kNone) return;                              // no position in this workgroup
  if (ld(&head->lo[slot][k]) > a) __hip_atomic_fetch_min(&head->lo[slot][k], a, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  if (ld(&head->hi[slot][k]) < b) __hip_atomic_fetch_max(&head->hi[slot][k], b, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

// rule a: the origin and the unit of a step from the keys an earlier launch left
struct Frame { double o[3]; double u; };
OVG_DEV Frame frame_of(const MoHead* head, int slot) {
  Frame fr;
  double ext = 0.0;
#pragma unroll
  for (int k = 0; k < 3; ++k) {
    fr.o[k] = (double)key_value32(head->lo[slot][k]);
    const double d = (double)key_value32(head->hi[slot][k]) - fr.o[k];
    if (d > ext) ext = d;
  }
  int e = 0;
  if (ext > 0.0) (void)frexp(ext, &e);                 // a mesh without a valid vertex leaves NaN keys: ext stays 0, nothing is quantised
  fr.u = ldexp(1.0, e - 30);
  return fr;
}

// thread i: the input's twelve bytes to the output, the final flag word (VALID, MOVABLE beside what the passes left), the first frame
__global__ __launch_bounds__(kThreads) void sm_start(ovg_mesh_smooth_params p, SmWs ws) {
  const int64_t i = (int64_t)blockIdx.x * kThreads + threadIdx.x;
  uint32_t lo[3] = {kNone, kNone, kNone}, hi[3] = {0u, 0u, 0u};
  if (i < p.num_vertices) {
    const float x[3] = {p.vertices[3 * i], p.vertices[3 * i + 1], p.vertices[3 * i + 2]};
    uint32_t w = ws.vflag[i] & 7u;
    if (finite3(x[0], x[1], x[2])) {
      w |= kValid;
      const bool held = (p.fixed && p.fixed[i]) || (p.fix_boundary && (w & OVG_MT_BOUNDARY));
      if ((w & OVG_MT_REFERENCED) && !held) w |= kMovable;
#pragma unroll
      for (int k = 0; k < 3; ++k) lo[k] = hi[k] = order_key32(x[k]);
    }
    ws.vflag[i] = w;
#pragma unroll
    for (int k = 0; k < 3; ++k) p.out_vertices[3 * i + k] = x[k];
  }
  frame_reduce(ws.head, 0, lo, hi);
}

// the row offsets of the adjacency: the sum of a tile of degrees ...
__global__ __launch_bounds__(kThreads) void sm_row_counts(SmWs ws, int64_t m) {
  __shared__ int64_t red[kThreads / 64];
  int64_t cnt = 0;
#pragma unroll 4
  for (int j = 0; j < kTile / kThreads; ++j) {
    const int64_t i = (int64_t)blockIdx.x * kTile + (int64_t)j * kThreads + threadIdx.x;
    if (i < m) cnt += ws.deg[i];
  }
  const int64_t t = block_reduce<kThreads>(cnt, red, IntSum());
  if (threadIdx.x == 0) ws.tcounts[blockIdx.x] = t;
}

// ... the exclusive scan of the tile sums in one workgroup of 1024 threads; row[M] = the number of entries ...
__global__ __launch_bounds__(1024) void sm_row_scan(SmWs ws, int64_t tiles, int64_t m) {
  const int64_t total = count_scan(ws.tcounts, ws.toffsets, tiles);
  if (threadIdx.x == 0) ws.row[m] = total;
}

// ... and the exclusive scan inside a tile: a thread owns 16 consecutive degrees
__global__ __launch_bounds__(kThreads) void sm_row_offsets(SmWs ws, int64_t m) {
  constexpr int J = kTile / kThreads;
  __shared__ int64_t wsum[kThreads / 64];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int64_t i0 = (int64_t)blockIdx.x * kTile + (int64_t)threadIdx.x * J;
  uint32_t d[J];
  int64_t mine = 0;
#pragma unroll
  for (int j = 0; j < J; ++j) {
    d[j] = i0 + j < m ? ws.deg[i0 + j] : 0u;
    mine += d[j];
  }
  const int64_t incl = wave_incl_scan(mine);
  if (lane == 63) wsum[wave] = incl;
  __syncthreads();
  int64_t at = ws.toffsets[blockIdx.x] + incl - mine;
  for (int w = 0; w < wave; ++w) at += wsum[w];
#pragma unroll
  for (int j = 0; j < J; ++j) {
    if (i0 + j < m) ws.row[i0 + j] = at;
    at += d[j];
  }
}

// one thread per face: a live face puts the two other corners into the row of each of its corners. A row is filled from its end through
// the degree that counted it, which falls back to 0; the order inside a row is the arrival order, and nothing reads it as an order
__global__ __launch_bounds__(kThreads) void sm_fill(ovg_mesh_smooth_params p, SmWs ws) {
  const int64_t f = (int64_t)blockIdx.x * kThreads + threadIdx.x;
  int32_t c[3];
  if (f >= p.num_faces || !live_face(p.vertices, p.faces, p.num_vertices, f, c)) return;
#pragma unroll
  for (int k = 0; k < 3; ++k) {
    const uint32_t left = __hip_atomic_fetch_sub(&ws.deg[c[k]], 2u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    if (left < 2u) continue;                           // never: mo_faces counted this face
    const int64_t at = ws.row[c[k]] + left - 2;
    ws.adj[at] = (uint32_t)c[(k + 1) % 3];
    ws.adj[at + 1] = (uint32_t)c[(k + 2) % 3];
  }
}

// rule b: thread i writes vertex i's record (qx, qy, qz, flag word) in the frame of this step, and thread 0 clears the other frame,
// which the update of this step fills for the next one
__global__ __launch_bounds__(kThreads) void sm_quantise(const float* __restrict__ pos, SmWs ws, int64_t m, int slot) {
  const int64_t i = (int64_t)blockIdx.x * kThreads + threadIdx.x;
  if (i == 0) {
#pragma unroll
    for (int k = 0; k < 3; ++k) ws.head->lo[slot ^ 1][k] = kNone, ws.head->hi[slot ^ 1][k] = 0u;
  }
  if (i >= m) return;
  const Frame fr = frame_of(ws.head, slot);
  int4 rec = {0, 0, 0, (int)ws.vflag[i]};
  if (rec.w & kValid) {
    rec.x = (int)llrint(((double)pos[3 * i] - fr.o[0]) / fr.u);
    rec.y = (int)llrint(((double)pos[3 * i + 1] - fr.o[1]) / fr.u);
    rec.z = (int)llrint(((double)pos[3 * i + 2] - fr.o[2]) / fr.u);
  }
  ws.q[i] = rec;
}

// the records of the neighbour pairs [j0, j1) of a row, `stride` apart, added to s: four gathers in flight
OVG_DEV void gather_pairs(const u32x2* __restrict__ pairs, const int4* __restrict__ q, int64_t j0, int64_t j1, int64_t stride, long long (&s)[3]) {
  int64_t j = j0;
  for (; j + stride < j1; j += 2 * stride) {
    const u32x2 a = pairs[j], b = pairs[j + stride];
    const int4 r0 = q[a[0]], r1 = q[a[1]], r2 = q[b[0]], r3 = q[b[1]];
    s[0] += ((long long)r0.x + r1.x) + ((long long)r2.x + r3.x);
    s[1] += ((long long)r0.y + r1.y) + ((long long)r2.y + r3.y);
    s[2] += ((long long)r0.z + r1.z) + ((long long)r2.z + r3.z);
  }
  if (j < j1) {
    const u32x2 a = pairs[j];
    const int4 r0 = q[a[0]], r1 = q[a[1]];
    s[0] += (long long)r0.x + r1.x, s[1] += (long long)r0.y + r1.y, s[2] += (long long)r0.z + r1.z;
  }
}

// rules c and d: thread i gathers the records of vertex i's row and moves the vertex; a row of more than kLongRow entries is summed by
// the whole wave, one such row after the other. A row holds whole pairs (the two other corners of a face) and starts at an even entry:
// it is read as 8-byte pairs. Every valid vertex then takes part in the frame of the next step
__global__ __launch_bounds__(kThreads) void sm_update(float* __restrict__ pos, SmWs ws, int64_t m, int slot, float factor) {
  const int64_t i = (int64_t)blockIdx.x * kThreads + threadIdx.x;
  const int lane = threadIdx.x & 63;
  const uint32_t w = i < m ? (uint32_t)ws.q[i].w : 0u;
  const bool movable = (w & kMovable) != 0u;
  const int64_t begin = movable ? ws.row[i] : 0, n = movable ? ws.row[i + 1] - begin : 0;
  const u32x2* pairs = reinterpret_cast<const u32x2*>(ws.adj);
  long long s[3] = {0, 0, 0};
  if (n <= kLongRow) gather_pairs(pairs, ws.q, begin >> 1, (begin + n) >> 1, 1, s);
  uint64_t todo = __ballot(n > kLongRow);              // the same in every lane: at most 64 rounds
  while (todo) {
    const int owner = __ffsll((long long)todo) - 1;
    todo &= todo - 1;
    const int64_t b = __shfl(begin, owner, 64) >> 1, len = __shfl(n, owner, 64) >> 1;
    long long t[3] = {0, 0, 0};
    gather_pairs(pairs, ws.q, b + lane, b + len, 64, t);
#pragma unroll
    for (int k = 0; k < 3; ++k) {
      const long long sum = __shfl(wave_reduce(t[k], IntSum()), 0, 64);
      if (lane == owner) s[k] = sum;
    }
  }
  uint32_t lo[3] = {kNone, kNone, kNone}, hi[3] = {0u, 0u, 0u};
  if (w & kValid) {
    float x[3] = {pos[3 * i], pos[3 * i + 1], pos[3 * i + 2]};
    if (movable && n > 0) {
      const Frame fr = frame_of(ws.head, slot);
#pragma unroll
      for (int k = 0; k < 3; ++k) {
        const double mean = (double)s[k] / (double)n;
        const double target = fr.o[k] + fr.u * mean;
        const double moved = (double)factor * (target - (double)x[k]);
        x[k] = (float)((double)x[k] + moved);
        pos[3 * i + k] = x[k];
      }
    }
    if (finite3(x[0], x[1], x[2])) {
#pragma unroll
      for (int k = 0; k < 3; ++k) lo[k] = hi[k] = order_key32(x[k]);
    } else {
      raise(&ws.head->flags, (uint32_t)OVG_MSM_NONFINITE);
    }
  }
  frame_reduce(ws.head, slot ^ 1, lo, hi);
}

// one thread per face: a live face (of the INPUT) with a usable normal at the final positions adds it to its three corners
__global__ __launch_bounds__(kThreads) void sm_face_normals(ovg_mesh_smooth_params p, SmWs ws) {
  const int64_t f = (int64_t)blockIdx.x * kThreads + threadIdx.x;
  int32_t c[3];
  if (f >= p.num_faces || !live_face(p.vertices, p.faces, p.num_vertices, f, c)) return;
  const float* a = p.out_vertices + 3 * (int64_t)c[0];
  const float* b = p.out_vertices + 3 * (int64_t)c[1];
  const float* d = p.out_vertices + 3 * (int64_t)c[2];
  const double d1[3] = {(double)b[0] - (double)a[0], (double)b[1] - (double)a[1], (double)b[2] - (double)a[2]};
  const double d2[3] = {(double)d[0] - (double)a[0], (double)d[1] - (double)a[1], (double)d[2] - (double)a[2]};
  const double cr[3] = {d1[1] * d2[2] - d1[2] * d2[1], d1[2] * d2[0] - d1[0] * d2[2], d1[0] * d2[1] - d1[1] * d2[0]};
  const double len = sqrt((cr[0] * cr[0] + cr[1] * cr[1]) + cr[2] * cr[2]);
  if (!(len > 0.0) || !finite_f64(len)) return;
#pragma unroll
  for (int k = 0; k < 3; ++k) {
    const long long q = llrint(cr[k] / len * 1048576.0);
    if (!q) continue;
#pragma unroll
    for (int j = 0; j < 3; ++j) add(&ws.nsum[3 * (int64_t)c[j] + k], (uint64_t)q);
  }
}

// thread i: vertex i's normal from its integer sums (rule 11 of ovg_mesh_simplify); thread 0: the status
__global__ __launch_bounds__(kThreads) void sm_finish(ovg_mesh_smooth_params p, SmWs ws) {
  const int64_t i = (int64_t)blockIdx.x * kThreads + threadIdx.x;
  if (i == 0) p.out_status[0] = (int64_t)ws.head->flags;
  if (i >= p.num_vertices || !p.out_normals) return;
  const double nx = (double)(long long)ws.nsum[3 * i], ny = (double)(long long)ws.nsum[3 * i + 1], nz = (double)(long long)ws.nsum[3 * i + 2];
  const double len = sqrt((nx * nx + ny * ny) + nz * nz);
  const bool ok = len > 0.0 && len <= 1.7976931348623157e308;
  p.out_normals[3 * i] = ok ? (float)(nx / len) : 0.0f;
  p.out_normals[3 * i + 1] = ok ? (float)(ny / len) : 0.0f;
  p.out_normals[3 * i + 2] = ok ? (float)(nz / len) : 0.0f;
}

unsigned mo_grid(int64_t work, int64_t per_block, int64_t cap) {
  const int64_t b = (work + per_block - 1) / per_block;
  return (unsigned)(b < 1 ? 1 : (b > cap ? cap : b));
}
unsigned mo_blocks(int64_t n) { return (unsigned)((n + kThreads - 1) / kThreads); }     // one thread per entry, n < 2^31

}  // namespace

extern "C" int64_t ovg_mesh_topology_workspace_bytes(int64_t vertices, int64_t faces) {
  return mo_sizes_ok(vertices, faces) ? mt_layout(vertices, faces, nullptr, nullptr) : -1;
}

extern "C" int ovg_mesh_topology(const ovg_mesh_topology_params* p, void* stream) {
  if (!p || !p->vertices || !p->faces || !p->vertex_root || !p->face_root || !p->vertex_flags || !p->out_count || !p->ws) return OVG_E_ARG;
  if (!mo_sizes_ok(p->num_vertices, p->num_faces)) return OVG_E_ARG;
  if (!al(p->vertices, 4) || !al(p->faces, 4) || !al(p->vertex_root, 4) || !al(p->face_root, 4) || !al(p->out_count, 8)) return OVG_E_ARG;
  if (!al(p->ws, 16) || p->ws_bytes < mt_layout(p->num_vertices, p->num_faces, nullptr, nullptr)) return OVG_E_ARG;
  hipStream_t st = static_cast<hipStream_t>(stream);
  MtWs ws;
  mt_layout(p->num_vertices, p->num_faces, static_cast<uint8_t*>(p->ws), &ws);
  const int64_t m = p->num_vertices, f = p->num_faces;
  OVG_LAUNCH(mo_clear, dim3(mo_grid(m > ws.edges.slots ? m : ws.edges.slots, kThreads * 4, 4096)), dim3(kThreads), 0, st, ws.head, ws.vflag, m,
             ws.edges, p->vertex_root, (uint32_t*)nullptr, (uint64_t*)nullptr);
  OVG_CHECK_LAUNCH();
  OVG_LAUNCH(mo_faces, dim3(mo_blocks(f)), dim3(kThreads), 0, st, p->vertices, p->faces, m, f, ws.head, ws.vflag, ws.edges, p->vertex_root,
             (uint32_t*)nullptr);
  OVG_CHECK_LAUNCH();
  OVG_LAUNCH(mo_edge_pass, dim3(mo_grid(ws.edges.slots, kThreads * 4, 4096)), dim3(kThreads), 0, st, ws.edges, ws.vflag, ws.head);
  OVG_CHECK_LAUNCH();
  OVG_LAUNCH(mt_finish, dim3(mo_blocks(m > f ? m : f)), dim3(kThreads), 0, st, *p, ws);
  OVG_CHECK_LAUNCH();
  OVG_LAUNCH(mt_done, dim3(1), dim3(1), 0, st, ws.head, p->out_count);
  OVG_CHECK_LAUNCH();
  return OVG_OK;
}

extern "C" int64_t ovg_mesh_select_workspace_bytes(int64_t vertices, int64_t faces) {
  return mo_sizes_ok(vertices, faces) ? sel_layout(vertices, faces, nullptr, nullptr) : -1;
}

extern "C" int ovg_mesh_select(const ovg_mesh_select_params* p, void* stream) {
  if (!p || !p->vertices || !p->faces || !p->ws) return OVG_E_ARG;
  if (!mo_sizes_ok(p->num_vertices, p->num_faces)) return OVG_E_ARG;
  if (p->stage < OVG_MSEL_COUNT || p->stage > (OVG_MSEL_COUNT | OVG_MSEL_SCATTER)) return OVG_E_ARG;
  if ((p->stage & OVG_MSEL_COUNT) && !p->out_count) return OVG_E_ARG;
  if (!al(p->vertices, 4) || !al(p->faces, 4) || !al(p->out_count, 8)) return OVG_E_ARG;
  if (p->stage & OVG_MSEL_SCATTER) {
    if (p->vertex_capacity < 0 || p->face_capacity < 0) return OVG_E_ARG;
    if ((p->vertex_capacity > 0 && !p->out_vertices) || (p->face_capacity > 0 && !p->out_faces)) return OVG_E_ARG;
    if (!al(p->out_vertices, 4) || !al(p->out_source_index, 8) || !al(p->out_faces, 4) || !al(p->out_face_index, 8)) return OVG_E_ARG;
  }
  if (!al(p->ws, 16) || p->ws_bytes < sel_layout(p->num_vertices, p->num_faces, nullptr, nullptr)) return OVG_E_ARG;
  hipStream_t st = static_cast<hipStream_t>(stream);
  SelWs ws;
  sel_layout(p->num_vertices, p->num_faces, static_cast<uint8_t*>(p->ws), &ws);
  const int64_t m = p->num_vertices, f = p->num_faces, vt = mo_tiles(m), ft = mo_tiles(f);
  if (p->stage & OVG_MSEL_COUNT) {
    OVG_LAUNCH(sel_clear, dim3(mo_grid(m > f ? m : f, kThreads * 64, 4096)), dim3(kThreads), 0, st, ws, m, f);
    OVG_CHECK_LAUNCH();
    OVG_LAUNCH(sel_faces, dim3(mo_blocks(f)), dim3(kThreads), 0, st, *p, ws);
    OVG_CHECK_LAUNCH();
    OVG_LAUNCH(sel_tile_counts, dim3((unsigned)(vt + ft)), dim3(kThreads), 0, st, ws, m, f, vt);
    OVG_CHECK_LAUNCH();
    OVG_LAUNCH(sel_scan, dim3(1), dim3(1024), 0, st, ws, vt, ft, p->out_count);
    OVG_CHECK_LAUNCH();
    OVG_LAUNCH(sel_ranks, dim3((unsigned)vt), dim3(kThreads), 0, st, ws, m);
    OVG_CHECK_LAUNCH();
  }
  if ((p->stage & OVG_MSEL_SCATTER) && p->vertex_capacity > 0) {
    OVG_LAUNCH(sel_scatter_vertices, dim3((unsigned)vt), dim3(kThreads), 0, st, *p, ws);
    OVG_CHECK_LAUNCH();
  }
  if ((p->stage & OVG_MSEL_SCATTER) && p->face_capacity > 0) {
    OVG_LAUNCH(sel_scatter_faces, dim3((unsigned)ft), dim3(kThreads), 0, st, *p, ws);
    OVG_CHECK_LAUNCH();
  }
  return OVG_OK;
}

extern "C" int64_t ovg_mesh_smooth_workspace_bytes(int64_t vertices, int64_t faces) {
  return mo_sizes_ok(vertices, faces) ? sm_layout(vertices, faces, nullptr, nullptr) : -1;
}

extern "C" int ovg_mesh_smooth(const ovg_mesh_smooth_params* p, void* stream) {
  if (!p || !p->vertices || !p->faces || !p->out_vertices || !p->out_status || !p->ws) return OVG_E_ARG;
  if (!mo_sizes_ok(p->num_vertices, p->num_faces) || p->out_vertices == p->vertices) return OVG_E_ARG;      // the live set is read from the input to the end
  if (p->iterations < 0 || p->iterations > 65536 || (p->fix_boundary != 0 && p->fix_boundary != 1)) return OVG_E_ARG;
  if (!(fabsf(p->lambda) <= 3.4028234663852886e38f) || !(fabsf(p->mu) <= 3.4028234663852886e38f)) return OVG_E_ARG;       // NaN fails as well
  if (!al(p->vertices, 4) || !al(p->faces, 4) || !al(p->out_vertices, 4) || !al(p->out_normals, 4) || !al(p->out_status, 8)) return OVG_E_ARG;
  if (!al(p->ws, 16) || p->ws_bytes < sm_layout(p->num_vertices, p->num_faces, nullptr, nullptr)) return OVG_E_ARG;
  hipStream_t st = static_cast<hipStream_t>(stream);
  SmWs ws;
  sm_layout(p->num_vertices, p->num_faces, static_cast<uint8_t*>(p->ws), &ws);
  const int64_t m = p->num_vertices, f = p->num_faces, vt = mo_tiles(m);
  const bool steps = p->iterations > 0;
  const MoEdges edges = steps && p->fix_boundary ? ws.edges : MoEdges{nullptr, nullptr, 0};
  OVG_LAUNCH(mo_clear, dim3(mo_grid(m > edges.slots ? m : edges.slots, kThreads * 4, 4096)), dim3(kThreads), 0, st, ws.head, ws.vflag, m, edges,
             (int32_t*)nullptr, steps ? ws.deg : (uint32_t*)nullptr, p->out_normals ? ws.nsum : (uint64_t*)nullptr);
  OVG_CHECK_LAUNCH();
  if (steps) {
    OVG_LAUNCH(mo_faces, dim3(mo_blocks(f)), dim3(kThreads), 0, st, p->vertices, p->faces, m, f, ws.head, ws.vflag, edges, (int32_t*)nullptr, ws.deg);
    OVG_CHECK_LAUNCH();
    if (edges.key) {
      OVG_LAUNCH(mo_edge_pass, dim3(mo_grid(edges.slots, kThreads * 4, 4096)), dim3(kThreads), 0, st, edges, ws.vflag, ws.head);
      OVG_CHECK_LAUNCH();
    }
    OVG_LAUNCH(sm_row_counts, dim3((unsigned)vt), dim3(kThreads), 0, st, ws, m);
    OVG_CHECK_LAUNCH();
    OVG_LAUNCH(sm_row_scan, dim3(1), dim3(1024), 0, st, ws, vt, m);
    OVG_CHECK_LAUNCH();
    OVG_LAUNCH(sm_row_offsets, dim3((unsigned)vt), dim3(kThreads), 0, st, ws, m);
    OVG_CHECK_LAUNCH();
    OVG_LAUNCH(sm_fill, dim3(mo_blocks(f)), dim3(kThreads), 0, st, *p, ws);
    OVG_CHECK_LAUNCH();
  }
  OVG_LAUNCH(sm_start, dim3(mo_blocks(m)), dim3(kThreads), 0, st, *p, ws);
  OVG_CHECK_LAUNCH();
  int slot = 0;
  for (int it = 0; it < p->iterations; ++it) {
    for (int half = 0; half < (p->mu != 0.0f ? 2 : 1); ++half, slot ^= 1) {
      OVG_LAUNCH(sm_quantise, dim3(mo_blocks(m)), dim3(kThreads), 0, st, p->out_vertices, ws, m, slot);
      OVG_CHECK_LAUNCH();
      OVG_LAUNCH(sm_update, dim3(mo_blocks(m)), dim3(kThreads), 0, st, p->out_vertices, ws, m, slot, half ? p->mu : p->lambda);
      OVG_CHECK_LAUNCH();
    }
  }
  if (p->out_normals) {
    OVG_LAUNCH(sm_face_normals, dim3(mo_blocks(f)), dim3(kThreads), 0, st, *p, ws);
    OVG_CHECK_LAUNCH();
  }
  OVG_LAUNCH(sm_finish, dim3(mo_blocks(m)), dim3(kThreads), 0, st, *p, ws);
  OVG_CHECK_LAUNCH();
  return OVG_OK;
}
