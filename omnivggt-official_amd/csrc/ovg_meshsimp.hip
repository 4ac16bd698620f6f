// Mesh simplification by vertex clustering on a uniform grid (ovg_mesh_simplify; include/omnivggt_hip.h states the rule,
// tests/meshsimp_twin.py restates it in numpy): every valid vertex falls into a cell of the grid of ovg_voxel_downsample, a cell becomes
// one output vertex when a surviving face names it, faces whose three cells are not pairwise different are dropped, of the faces with
// the same unordered set of three cells the lowest input index survives.
// Two open-addressing tables. The CELL table is the one of ovg_voxel_downsample: a 63-bit key claimed by a 64-bit compare-and-swap; the
// leader (integer min), the vertex count and the integer sums of position, colour and normal live in arrays indexed by the slot, and every
// vertex stores its slot once. The FACE table holds face indices only: a prober compares its sorted triple of cell slots with the triple of
// the face a slot names and issues one integer min of its own index when they agree. A slot's triple never changes while its index only
// shrinks, so the outcome is the lowest face index per triple in any arrival order. Integer atomics only, relaxed, agent scope: two runs
// give identical bytes. The insert stages are bound by random atomics, the scatters by bandwidth; no workgroup waits for another.
#include "ovg_geom.h"

// the cell arithmetic, the mean position and the normalisation restate numpy operation for operation: no fused multiply-add in this
// unit (build.py compiles it with -ffp-contract=off as well, which reaches the inlined HIP header helpers)
#pragma clang fp contract(off)

namespace {

constexpr int kThreads = 256;
constexpr int kTile = kThreads * 16;                // entries per workgroup of the ordered compactions
constexpr uint64_t kNoKey = ~0ull;                  // no cell key has bit 63
constexpr uint32_t kNone = 0xFFFFFFFFu;             // no slot / no face / no rank
constexpr float kMaxCell = 2097151.0f;              // 2^21 - 1
constexpr int64_t kMinSlots = 1024;
constexpr int kSums = 9;                            // per cell: Qx Qy Qz, red green blue, nx ny nz

struct MsHead {
  uint32_t origin[3];                               // order keys (integer min is exact and order-free)
  uint32_t flags;
  unsigned long long cells, candidates, degenerate;
};

struct MsWs {
  MsHead* head;
  uint64_t* key; uint32_t* leader; uint32_t* cnt; uint32_t* rank; uint64_t* sums;     // per cell slot; sums [slot][kSums]
  uint32_t* vslot; uint8_t* vkeep;                                                      // per vertex
  uint32_t* ftab;                                                                       // the face table
  uint8_t* fkeep;                                                                       // per face
  int64_t* vcounts; int64_t* voffsets; int64_t* fcounts; int64_t* foffsets;             // per tile
  int64_t ncs, nfs;
};

int64_t ms_slots(int64_t n) { return 2 * n < kMinSlots ? kMinSlots : 2 * n; }          // load factor <= 1/2
int64_t ms_tiles(int64_t n) { return (n + kTile - 1) / kTile; }
bool ms_sizes_ok(int64_t m, int64_t f) { return size_ok(m) && f >= 1 && f < 0xFFFFFFFFll; }

// -> the bytes; with base != nullptr also the pointers
int64_t ms_layout(int64_t m, int64_t f, uint8_t* base, MsWs* ws) {
  const int64_t ncs = ms_slots(m), nfs = ms_slots(f), vt = ms_tiles(m), ft = ms_tiles(f);
  const int64_t part[] = {256, 8 * ncs, 4 * ncs, 4 * ncs, 4 * ncs, 8 * kSums * ncs, 4 * m, m, 4 * nfs, f, 8 * vt, 8 * vt, 8 * ft, 8 * ft};
  int64_t off[15];
  off[0] = 0;
  for (int k = 0; k < 14; ++k) off[k + 1] = off[k] + round256(part[k]);
  if (base) {
    auto at = [&](int k) { return base + off[k]; };
    *ws = {reinterpret_cast<MsHead*>(at(0)), reinterpret_cast<uint64_t*>(at(1)), reinterpret_cast<uint32_t*>(at(2)),
           reinterpret_cast<uint32_t*>(at(3)), reinterpret_cast<uint32_t*>(at(4)), reinterpret_cast<uint64_t*>(at(5)),
           reinterpret_cast<uint32_t*>(at(6)), at(7), reinterpret_cast<uint32_t*>(at(8)), at(9), reinterpret_cast<int64_t*>(at(10)),
           reinterpret_cast<int64_t*>(at(11)), reinterpret_cast<int64_t*>(at(12)), reinterpret_cast<int64_t*>(at(13)), ncs, nfs};
  }
  return off[14];
}

template <typename T> OVG_DEV T ld(const T* p) { return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }
OVG_DEV void add64(uint64_t* p, uint64_t v) { __hip_atomic_fetch_add(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }
OVG_DEV void raise_flag(MsHead* head, uint32_t flag) {
  if (!(ld(&head->flags) & flag)) __hip_atomic_fetch_or(&head->flags, flag, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

__global__ __launch_bounds__(kThreads) void ms_init(MsWs ws, int64_t m, int64_t f) {
  const int64_t t0 = (int64_t)blockIdx.x * kThreads + threadIdx.x, step = (int64_t)gridDim.x * kThreads;
  for (int64_t s = t0; s < ws.ncs; s += step) {
    ws.key[s] = kNoKey;
    ws.leader[s] = kNone;
    ws.cnt[s] = 0u;
    ws.rank[s] = kNone;
#pragma unroll
    for (int k = 0; k < kSums; ++k) ws.sums[s * kSums + k] = 0ull;
  }
  for (int64_t s = t0; s < ws.nfs; s += step) ws.ftab[s] = kNone;
  u32x4* vk = reinterpret_cast<u32x4*>(ws.vkeep);                   // the keep bytes are rounded up to 256: whole 16-byte stores
  u32x4* fk = reinterpret_cast<u32x4*>(ws.fkeep);
  const u32x4 zero = {0u, 0u, 0u, 0u};
  for (int64_t i = t0; i < (m + 15) / 16; i += step) vk[i] = zero;
  for (int64_t i = t0; i < (f + 15) / 16; i += step) fk[i] = zero;
  if (t0 == 0) *ws.head = {{kNone, kNone, kNone}, 0u, 0ull, 0ull, 0ull};
}

__global__ __launch_bounds__(kThreads) void ms_origin(const float* __restrict__ v, int64_t m, MsWs ws) {
  __shared__ uint32_t red[kThreads / 64];
  uint32_t lo[3] = {kNone, kNone, kNone};
  for (int64_t i = (int64_t)blockIdx.x * kThreads + threadIdx.x; i < m; i += (int64_t)gridDim.x * kThreads) {
    const float x = v[3 * i], y = v[3 * i + 1], z = v[3 * i + 2];
    if (finite3(x, y, z)) {
      lo[0] = min(lo[0], order_key32(x));
      lo[1] = min(lo[1], order_key32(y));
      lo[2] = min(lo[2], order_key32(z));
    }
  }
#pragma unroll
  for (int k = 0; k < 3; ++k) {
    __syncthreads();                                                // red is read by every thread of the previous round
    const uint32_t t = block_reduce<kThreads>(lo[k], red, IntMin());
    if (threadIdx.x == 0 && t != kNone) __hip_atomic_fetch_min(&ws.head->origin[k], t, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  }
}

// one thread per vertex: the cell, its slot (claimed here when the cell is new), the leader, the count and the integer sums
__global__ __launch_bounds__(kThreads) void ms_insert(ovg_mesh_simplify_params p, MsWs ws) {
  __shared__ uint32_t red[kThreads / 64];
  const int64_t i = (int64_t)blockIdx.x * kThreads + threadIdx.x;
  const float v = *p.voxel;
  const bool bad = !(v > 0.0f) || !finite_f32(v);
  if (bad && i == 0) raise_flag(ws.head, (uint32_t)OVG_MS_BAD_VOXEL);
  uint32_t slot = kNone, claimed = 0u;
  float g[3] = {0.0f, 0.0f, 0.0f}, c[3] = {0.0f, 0.0f, 0.0f};
  bool valid = false;
  if (i < p.num_vertices && !bad) {
    const float x[3] = {p.vertices[3 * i], p.vertices[3 * i + 1], p.vertices[3 * i + 2]};
    if (finite3(x[0], x[1], x[2])) {
      // np.floor((p - origin) / v) in float32: one subtraction, one correctly rounded division, a floor (p >= origin, so c >= 0)
#pragma unroll
      for (int k = 0; k < 3; ++k) {
        g[k] = __fdiv_rn(__fsub_rn(x[k], key_value32(ws.head->origin[k])), v);
        c[k] = floorf(g[k]);
      }
      valid = c[0] <= kMaxCell && c[1] <= kMaxCell && c[2] <= kMaxCell;              // fails also for an extent that overflowed to inf
      if (!valid) raise_flag(ws.head, (uint32_t)OVG_MS_OVERFLOW);
    }
  }
  if (valid) {
    const uint64_t key = ((uint64_t)(uint32_t)c[0] << 42) | ((uint64_t)(uint32_t)c[1] << 21) | (uint64_t)(uint32_t)c[2];
    int64_t s = (int64_t)__umul64hi(mix_murmur64(key), (uint64_t)ws.ncs);
    for (int64_t t = 0; t < ws.ncs; ++t) {           // at most m of the >= 2m slots are ever claimed: the walk ends at a free one
      uint64_t k = ld(&ws.key[s]);
      if (k == kNoKey) {
        uint64_t expect = kNoKey;
        const bool won = __hip_atomic_compare_exchange_strong(&ws.key[s], &expect, key, __ATOMIC_RELAXED, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        k = won ? key : expect;
        claimed = won;
      }
      if (k == key) {
        slot = (uint32_t)s;
        break;
      }
      s = s + 1 == ws.ncs ? 0 : s + 1;
    }
  }
  if (slot != kNone) {
    // the leader only shrinks: a vertex that already loses to what is visible needs no atomic
    if (ld(&ws.leader[slot]) > (uint32_t)i) __hip_atomic_fetch_min(&ws.leader[slot], (uint32_t)i, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    __hip_atomic_fetch_add(&ws.cnt[slot], 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    uint64_t* sum = ws.sums + (int64_t)slot * kSums;
#pragma unroll
    for (int k = 0; k < 3; ++k) {
      const float r = __fsub_rn(g[k], c[k]);                                          // exact, in [0, 1)
      const long long q = llrint((double)r * 16777216.0);
      if (q) add64(sum + k, (uint64_t)q);
    }
    if (p.colors) {
#pragma unroll
      for (int k = 0; k < 3; ++k) {
        const uint64_t col = p.colors[3 * i + k];
        if (col) add64(sum + 3 + k, col);
      }
    }
    if (p.normals) {
      const float n[3] = {p.normals[3 * i], p.normals[3 * i + 1], p.normals[3 * i + 2]};
      if (finite3(n[0], n[1], n[2]) && fabsf(n[0]) <= 4.0f && fabsf(n[1]) <= 4.0f && fabsf(n[2]) <= 4.0f) {
#pragma unroll
        for (int k = 0; k < 3; ++k) {
          const long long q = llrint((double)n[k] * 1048576.0);
          if (q) add64(sum + 6 + k, (uint64_t)q);
        }
      }
    }
  }
  if (i < p.num_vertices) ws.vslot[i] = slot;
  const uint32_t total = block_reduce<kThreads>(claimed, red, IntSum());
  if (threadIdx.x == 0 && total) __hip_atomic_fetch_add(&ws.head->cells, (unsigned long long)total, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

OVG_DEV void sort3(uint32_t& a, uint32_t& b, uint32_t& c) {
  uint32_t t;
  if (a > b) t = a, a = b, b = t;
  if (b > c) t = b, b = c, c = t;
  if (a > b) t = a, a = b, b = t;
}

// the cell slots of face f's corners -> true when the face is live (indices inside the mesh, vertices valid)
OVG_DEV bool face_slots(const int32_t* __restrict__ faces, const uint32_t* __restrict__ vslot, int64_t m, int64_t f, uint32_t& a, uint32_t& b,
                        uint32_t& c) {
  const int64_t i0 = faces[3 * f], i1 = faces[3 * f + 1], i2 = faces[3 * f + 2];
  if (i0 < 0 || i1 < 0 || i2 < 0 || i0 >= m || i1 >= m || i2 >= m) return false;
  a = vslot[i0], b = vslot[i1], c = vslot[i2];
  return a != kNone && b != kNone && c != kNone;
}

// one thread per face: a live face with three different cells enters the face table, where the lowest index of its triple stays
__global__ __launch_bounds__(kThreads) void ms_faces(ovg_mesh_simplify_params p, MsWs ws) {
  __shared__ uint32_t red[kThreads / 64];
  const int64_t f = (int64_t)blockIdx.x * kThreads + threadIdx.x;
  uint32_t a = 0, b = 0, c = 0, degenerate = 0u, candidate = 0u;
  if (f < p.num_faces && !ws.head->flags && face_slots(p.faces, ws.vslot, p.num_vertices, f, a, b, c)) {
    degenerate = a == b || b == c || a == c;
    candidate = !degenerate;
  }
  if (candidate) {
    sort3(a, b, c);
    const uint32_t me = (uint32_t)f;
    int64_t s = (int64_t)__umul64hi(mix_murmur64(mix_murmur64(((uint64_t)a << 32) | b) + c), (uint64_t)ws.nfs);
    for (int64_t t = 0; t < ws.nfs; ++t) {           // at most F of the >= 2F slots are ever claimed
      uint32_t cur = ld(&ws.ftab[s]);
      if (cur == kNone) {
        uint32_t expect = kNone;
        if (__hip_atomic_compare_exchange_strong(&ws.ftab[s], &expect, me, __ATOMIC_RELAXED, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)) break;
        cur = expect;
      }
      // whatever index the slot shows names a face of the slot's triple: read that face's cells through it
      uint32_t x = 0, y = 0, z = 0;
      face_slots(p.faces, ws.vslot, p.num_vertices, (int64_t)cur, x, y, z);
      sort3(x, y, z);
      if (x == a && y == b && z == c) {
        if (cur > me) __hip_atomic_fetch_min(&ws.ftab[s], me, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        break;
      }
      s = s + 1 == ws.nfs ? 0 : s + 1;
    }
  }
  const uint32_t nd = block_reduce<kThreads>(degenerate, red, IntSum());
  __syncthreads();
  const uint32_t nc = block_reduce<kThreads>(candidate, red, IntSum());
  if (threadIdx.x == 0) {
    if (nd) __hip_atomic_fetch_add(&ws.head->degenerate, (unsigned long long)nd, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    if (nc) __hip_atomic_fetch_add(&ws.head->candidates, (unsigned long long)nc, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  }
}

// every claimed slot of the face table names a survivor; a survivor marks itself and the leaders of its three cells (several survivors
// may store the same byte: harmless)
__global__ __launch_bounds__(kThreads) void ms_survivors(ovg_mesh_simplify_params p, MsWs ws) {
  for (int64_t s = (int64_t)blockIdx.x * kThreads + threadIdx.x; s < ws.nfs; s += (int64_t)gridDim.x * kThreads) {
    const uint32_t f = ws.ftab[s];
    if (f == kNone) continue;
    ws.fkeep[f] = 1;                                   // only candidates of ms_faces enter the table: indices and slots are valid
#pragma unroll
    for (int k = 0; k < 3; ++k) ws.vkeep[ws.leader[ws.vslot[p.faces[3 * (int64_t)f + k]]]] = 1;
  }
}

// blockIdx.x < vtiles: a tile of vertex keep bytes, else a tile of face keep bytes
__global__ __launch_bounds__(kThreads) void ms_tile_counts(MsWs ws, int64_t m, int64_t f, int64_t vtiles) {
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

// the two exclusive scans of the tile counts in one workgroup of 1024 threads, and the six counts
__global__ __launch_bounds__(1024) void ms_scan(MsWs ws, int64_t vtiles, int64_t ftiles, int64_t* out_count) {
  const int64_t mv = count_scan(ws.vcounts, ws.voffsets, vtiles);
  __syncthreads();
  const int64_t mf = count_scan(ws.fcounts, ws.foffsets, ftiles);
  if (threadIdx.x == 0) {
    const MsHead h = *ws.head;
    const bool flagged = h.flags != 0u;
    out_count[0] = mv;
    out_count[1] = mf;
    out_count[2] = (int64_t)h.flags;
    out_count[3] = flagged ? 0 : (int64_t)h.cells;
    out_count[4] = flagged ? 0 : (int64_t)h.degenerate;
    out_count[5] = flagged ? 0 : (int64_t)h.candidates - mf;
  }
}

// the output number of every kept cell: its leader's rank among the kept leaders
__global__ __launch_bounds__(kThreads) void ms_ranks(MsWs ws, int64_t m) {
  compact_tile<kThreads, kTile>(ws.vkeep, m, ws.voffsets, [&](int64_t i, int64_t pos) {
    const int64_t s = ws.vslot[i];
    if (s < ws.ncs) ws.rank[s] = (uint32_t)pos;        // always, after this call's COUNT stage
  });
}

// one thread per cell slot: a kept cell writes its output vertex
__global__ __launch_bounds__(kThreads) void ms_scatter_vertices(ovg_mesh_simplify_params p, MsWs ws) {
  const int64_t s = (int64_t)blockIdx.x * kThreads + threadIdx.x;
  if (s >= ws.ncs) return;
  const int64_t pos = ws.rank[s];
  if (pos >= p.vertex_capacity) return;                // kNone as well
  const int64_t lead = ws.leader[s];
  const uint32_t n = ws.cnt[s];
  if (lead >= p.num_vertices || n == 0u) return;       // never, after this call's COUNT stage
  const uint64_t* sum = ws.sums + s * kSums;
  float* out = p.out_vertices + 3 * pos;
  if (p.position == OVG_MS_POS_FIRST) {
#pragma unroll
    for (int k = 0; k < 3; ++k) out[k] = p.vertices[3 * lead + k];
  } else {
    const uint64_t key = ws.key[s];
    const double v = (double)*p.voxel, den = (double)n * 16777216.0;
    const uint32_t cell[3] = {(uint32_t)(key >> 42), (uint32_t)(key >> 21) & 0x1FFFFFu, (uint32_t)key & 0x1FFFFFu};
#pragma unroll
    for (int k = 0; k < 3; ++k) {
      const double frac = (double)(long long)sum[k] / den;
      const double in_cells = (double)cell[k] + frac;
      const double offset = v * in_cells;
      out[k] = (float)((double)key_value32(ws.head->origin[k]) + offset);
    }
  }
  if (p.out_colors) {
#pragma unroll
    for (int k = 0; k < 3; ++k) p.out_colors[3 * pos + k] = (uint8_t)((2ull * sum[3 + k] + n) / (2ull * n));       // the mean, half up
  }
  if (p.out_normals) {
    const double nx = (double)(long long)sum[6], ny = (double)(long long)sum[7], nz = (double)(long long)sum[8];
    const double len = sqrt((nx * nx + ny * ny) + nz * nz);
    const bool ok = len > 0.0 && len <= 1.7976931348623157e308;
    p.out_normals[3 * pos] = ok ? (float)(nx / len) : 0.0f;
    p.out_normals[3 * pos + 1] = ok ? (float)(ny / len) : 0.0f;
    p.out_normals[3 * pos + 2] = ok ? (float)(nz / len) : 0.0f;
  }
  if (p.out_source_index) p.out_source_index[pos] = lead;
  if (p.out_vertex_count) p.out_vertex_count[pos] = (int32_t)n;
}

// the survivors in input order, their corners as output vertex numbers: vertex -> slot -> rank
__global__ __launch_bounds__(kThreads) void ms_scatter_faces(ovg_mesh_simplify_params p, MsWs ws) {
  compact_tile<kThreads, kTile>(ws.fkeep, p.num_faces, ws.foffsets, [&](int64_t f, int64_t pos) {
    if (pos < 0 || pos >= p.face_capacity) return;
#pragma unroll
    for (int k = 0; k < 3; ++k) {
      const int64_t i = p.faces[3 * f + k];
      const int64_t s = i >= 0 && i < p.num_vertices ? (int64_t)ws.vslot[i] : ws.ncs;
      p.out_faces[3 * pos + k] = s < ws.ncs ? (int32_t)ws.rank[s] : -1;        // a survivor's corners are valid vertices of kept cells
    }
  });
}

unsigned ms_grid(int64_t work, int64_t per_block, int64_t cap) {
  const int64_t b = (work + per_block - 1) / per_block;
  return (unsigned)(b < 1 ? 1 : (b > cap ? cap : b));
}

}  // namespace

extern "C" int64_t ovg_mesh_simplify_workspace_bytes(int64_t vertices, int64_t faces) {
  return ms_sizes_ok(vertices, faces) ? ms_layout(vertices, faces, nullptr, nullptr) : -1;
}

extern "C" int ovg_mesh_simplify(const ovg_mesh_simplify_params* p, void* stream) {
  if (!p || !p->vertices || !p->faces || !p->voxel || !p->ws) return OVG_E_ARG;
  if (!ms_sizes_ok(p->num_vertices, p->num_faces)) return OVG_E_ARG;
  if (p->stage < OVG_MS_COUNT || p->stage > (OVG_MS_COUNT | OVG_MS_SCATTER)) return OVG_E_ARG;
  if ((p->stage & OVG_MS_COUNT) && !p->out_count) return OVG_E_ARG;
  if (p->position != OVG_MS_POS_MEAN && p->position != OVG_MS_POS_FIRST) return OVG_E_ARG;
  if (!al(p->vertices, 4) || !al(p->faces, 4) || !al(p->normals, 4) || !al(p->voxel, 4) || !al(p->out_count, 8)) return OVG_E_ARG;
  if (p->stage & OVG_MS_SCATTER) {
    if (p->vertex_capacity < 0 || p->face_capacity < 0) return OVG_E_ARG;
    if (p->vertex_capacity > 0 && (!p->out_vertices || (p->normals != nullptr) != (p->out_normals != nullptr) ||
                                   (p->colors != nullptr) != (p->out_colors != nullptr))) return OVG_E_ARG;
    if (p->face_capacity > 0 && !p->out_faces) return OVG_E_ARG;
    if (!al(p->out_vertices, 4) || !al(p->out_normals, 4) || !al(p->out_source_index, 8) || !al(p->out_vertex_count, 4) || !al(p->out_faces, 4))
      return OVG_E_ARG;
  }
  if (!al(p->ws, 16) || p->ws_bytes < ms_layout(p->num_vertices, p->num_faces, nullptr, nullptr)) return OVG_E_ARG;
  hipStream_t st = static_cast<hipStream_t>(stream);
  MsWs ws;
  ms_layout(p->num_vertices, p->num_faces, static_cast<uint8_t*>(p->ws), &ws);
  const int64_t m = p->num_vertices, f = p->num_faces, vt = ms_tiles(m), ft = ms_tiles(f);
  if (p->stage & OVG_MS_COUNT) {
    OVG_LAUNCH(ms_init, dim3(ms_grid(ws.ncs > ws.nfs ? ws.ncs : ws.nfs, kThreads * 4, 4096)), dim3(kThreads), 0, st, ws, m, f);
    OVG_CHECK_LAUNCH();
    OVG_LAUNCH(ms_origin, dim3(ms_grid(m, kThreads * 4, 2048)), dim3(kThreads), 0, st, p->vertices, m, ws);
    OVG_CHECK_LAUNCH();
    OVG_LAUNCH(ms_insert, dim3((unsigned)((m + kThreads - 1) / kThreads)), dim3(kThreads), 0, st, *p, ws);
    OVG_CHECK_LAUNCH();
    OVG_LAUNCH(ms_faces, dim3((unsigned)((f + kThreads - 1) / kThreads)), dim3(kThreads), 0, st, *p, ws);
    OVG_CHECK_LAUNCH();
    OVG_LAUNCH(ms_survivors, dim3(ms_grid(ws.nfs, kThreads * 4, 4096)), dim3(kThreads), 0, st, *p, ws);
    OVG_CHECK_LAUNCH();
    OVG_LAUNCH(ms_tile_counts, dim3((unsigned)(vt + ft)), dim3(kThreads), 0, st, ws, m, f, vt);
    OVG_CHECK_LAUNCH();
    OVG_LAUNCH(ms_scan, dim3(1), dim3(1024), 0, st, ws, vt, ft, p->out_count);
    OVG_CHECK_LAUNCH();
    OVG_LAUNCH(ms_ranks, dim3((unsigned)vt), dim3(kThreads), 0, st, ws, m);
    OVG_CHECK_LAUNCH();
  }
  if ((p->stage & OVG_MS_SCATTER) && p->vertex_capacity > 0) {
    OVG_LAUNCH(ms_scatter_vertices, dim3((unsigned)((ws.ncs + kThreads - 1) / kThreads)), dim3(kThreads), 0, st, *p, ws);
    OVG_CHECK_LAUNCH();
  }
  if ((p->stage & OVG_MS_SCATTER) && p->face_capacity > 0) {
    OVG_LAUNCH(ms_scatter_faces, dim3((unsigned)ft), dim3(kThreads), 0, st, *p, ws);
    OVG_CHECK_LAUNCH();
  }
  return OVG_OK;
}
