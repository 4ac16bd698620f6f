// Radius neighbour search through a uniform hash grid (ovg_radius_search): for every query the number of reference points within
// radius_sq and the nearest of them, by the rule of ovg_nearest_neighbours restricted to d <= radius_sq (include/omnivggt_hip.h).
// BUILD bins the usable references: an open-addressing table of 16-byte slots {cell key, count, cursor} (the claim is ovg_pointcloud.hip's
// 64-bit compare-and-swap on the packed cell key), an exclusive scan of the counts, a scatter of 16-byte records {x, y, z, bits(j)}
// into cell order, and a cost pass that sums the cell counts of every query's box. SEARCH: one query per thread walks its box of
// cells and runs the exact rule over each cell's records. The box covers every candidate for any cell edge and origin (header), so
// the grid changes the cost and never a byte. The table is bound by random 64-bit atomics, the search by its gather of records.
// ovg_knn_search and ovg_cluster (connected components / DBSCAN: a lock-free union-find over the neighbour pairs) walk the same grid.
#include <math.h>
#include "ovg_geom.h"

// tests/radius_twin.py restates the rule and the cell function in numpy float32, one rounding per operation: no fused multiply-adds
// in this unit (build.py compiles it with -ffp-contract=off as well)
#pragma clang fp contract(off)

namespace {

constexpr int kThreads = OVG_RS_QUERY_BLOCK;
constexpr int kScanPer = 16;                           // slots per thread of the scan passes
constexpr int kScanTile = kThreads * kScanPer;         // slots per workgroup of the scan passes
constexpr uint64_t kEmpty = ~0ull;                     // no cell key has bit 63
constexpr uint32_t kInfBits = 0x7F800000u;
constexpr uint64_t kNoneKey = ~0ull;                   // above every (bits(d) << 32) | j of a candidate: bits(d) <= bits(radius_sq) < bits(+inf)
constexpr float kCellLo = -1048576.0f, kCellHi = 1048575.0f;   // -2^20, 2^20 - 1
constexpr float kMinRadiusSq = 0x1p-100f;

// nr: 0 after the clear, the cloud's once BUILD is through; cl_flags: ovg_cluster's own (OVG_CL_INTERNAL), the one word a search writes
struct RsHead { uint32_t flags, max_cell; uint64_t occupied, pairs; int64_t nr; uint32_t cl_flags; };
struct RsSlot { uint64_t key; uint32_t count, end; };  // end: the cell's first record after the scan, one past its last after the scatter
struct RsWs { RsHead* head; RsSlot* table; int64_t nslots; u32x4* rec; uint32_t* tile; int64_t ntiles; };

static_assert(sizeof(RsSlot) == 16 && sizeof(RsHead) <= 256, "workspace layout");

bool rs_shape_ok(int64_t nq, int64_t nr) { return size_ok(nq) && size_ok(nr); }
int64_t rs_slots(int64_t nr) { return 2 * nr < OVG_RS_MIN_SLOTS ? OVG_RS_MIN_SLOTS : 2 * nr; }   // load factor <= 1/2
int64_t rs_tiles(int64_t nr) { return (rs_slots(nr) + kScanTile - 1) / kScanTile; }
int64_t rs_ws_bytes(int64_t nr) { return 256 + round256(rs_slots(nr) * 16) + round256(nr * 16) + round256(rs_tiles(nr) * 4); }
RsWs rs_ws(const ovg_radius_params* p) {
  uint8_t* b = static_cast<uint8_t*>(p->ws);
  const int64_t ns = rs_slots(p->nr);
  uint8_t* rec = b + 256 + round256(ns * 16);
  return {reinterpret_cast<RsHead*>(b), reinterpret_cast<RsSlot*>(b + 256), ns, reinterpret_cast<u32x4*>(rec),
          reinterpret_cast<uint32_t*>(rec + round256(p->nr * 16)), rs_tiles(p->nr)};
}

// the f32 just above sqrt((double)radius_sq) (1 + 2^-20): the header fixes this formula, tests/radius_twin.py restates it
float rs_reach(float radius_sq) {
  const double v = sqrt((double)radius_sq) * (1.0 + 0x1p-20);
  const float r = (float)v;
  return (double)r > v ? r : nextafterf(r, INFINITY);
}

OVG_DEV float rs_origin(const float* origin, int k) {
  const float o = origin ? origin[k] : 0.0f;
  return finite_f32(o) ? o : 0.0f;
}

// C(x) of the header, shifted to [0, 2^21): monotone in x. With a finite origin and cell no NaN arises (x is finite or +-inf)
OVG_DEV uint32_t rs_cell(float x, float o, float cell) {
  const float c = floorf(__fdiv_rn(__fsub_rn(x, o), cell));
  const float k = c >= kCellLo ? (c <= kCellHi ? c : kCellHi) : kCellLo;
  return (uint32_t)((int32_t)k + (1 << 20));
}

OVG_DEV uint64_t rs_key(uint32_t cx, uint32_t cy, uint32_t cz) { return ((uint64_t)cx << 42) | ((uint64_t)cy << 21) | (uint64_t)cz; }

OVG_DEV int64_t rs_home(const RsWs& ws, uint64_t key) { return (int64_t)__umul64hi(mix_murmur64(key), (uint64_t)ws.nslots); }

// the slot of a cell in a table that no launch is writing keys to: -1 when the cell holds no reference
OVG_DEV int64_t rs_find(const RsWs& ws, uint64_t key, uint32_t& count, uint32_t& end) {
  int64_t s = rs_home(ws, key);
  for (int64_t t = 0; t < ws.nslots; ++t) {            // at most nr of the >= 2 nr slots are claimed: the walk ends at a free one
    const u32x4 e = reinterpret_cast<const u32x4*>(ws.table)[s];
    const uint64_t k = ((uint64_t)e[1] << 32) | e[0];
    if (k == key) { count = e[2]; end = e[3]; return s; }
    if (k == kEmpty) return -1;
    s = s + 1 == ws.nslots ? 0 : s + 1;
  }
  return -1;
}

struct RsBox { uint32_t lo[3], hi[3]; };

// the cells [C(fl(q - reach)), C(fl(q + reach))] per axis: every candidate of q lies in one of them (header)
OVG_DEV RsBox rs_box(const float (&q)[3], const float* origin, float cell, float reach) {
  RsBox b;
#pragma unroll
  for (int k = 0; k < 3; ++k) {
    const float o = rs_origin(origin, k);
    b.lo[k] = rs_cell(__fsub_rn(q[k], reach), o, cell);
    b.hi[k] = rs_cell(__fadd_rn(q[k], reach), o, cell);
  }
  return b;
}

// point i of a cloud; false when it is unusable
OVG_DEV bool rs_point(const float* pts, const uint8_t* valid, uint32_t i, float (&v)[3]) {
  const float* p = pts + 3 * (int64_t)i;
  v[0] = p[0], v[1] = p[1], v[2] = p[2];
  return finite3(v[0], v[1], v[2]) && (!valid || valid[i] != 0);
}

__global__ __launch_bounds__(kThreads) void rs_clear(RsWs ws) {
  const int64_t t0 = (int64_t)blockIdx.x * kThreads + threadIdx.x, step = (int64_t)gridDim.x * kThreads;
  u32x4* tab = reinterpret_cast<u32x4*>(ws.table);
  const u32x4 empty = {0xFFFFFFFFu, 0xFFFFFFFFu, 0u, 0u};
  for (int64_t i = t0; i < ws.nslots; i += step) tab[i] = empty;
  if (t0 == 0) *ws.head = {0u, 0u, 0ull, 0ull, 0ll, 0u};
}

// every usable reference claims the slot of its cell and counts itself
__global__ __launch_bounds__(kThreads) void rs_count(ovg_radius_params p, RsWs ws) {
  const uint32_t j = blockIdx.x * kThreads + threadIdx.x;                  // nr < 2^31: no wrap in unsigned arithmetic
  float r[3];
  if (j >= (uint32_t)p.nr || !rs_point(p.reference, p.reference_valid, j, r)) return;
  const uint64_t key = rs_key(rs_cell(r[0], rs_origin(p.origin, 0), p.cell), rs_cell(r[1], rs_origin(p.origin, 1), p.cell),
                              rs_cell(r[2], rs_origin(p.origin, 2), p.cell));
  int64_t s = rs_home(ws, key);
  for (int64_t t = 0; t < ws.nslots; ++t) {
    RsSlot* slot = ws.table + s;
    uint64_t k = __hip_atomic_load(&slot->key, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    if (k == kEmpty) {
      uint64_t expect = kEmpty;
      k = __hip_atomic_compare_exchange_strong(&slot->key, &expect, key, __ATOMIC_RELAXED, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) ? key : expect;
    }
    if (k == key) {
      __hip_atomic_fetch_add(&slot->count, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      return;
    }
    s = s + 1 == ws.nslots ? 0 : s + 1;
  }
}

// the exclusive scan of the slot counts in three launches: sums per tile of kScanTile slots (and the table's statistics), one
// workgroup over the tile sums, the slots of every tile. Inside a tile the order is (thread, k) with slot = base + k * kThreads +
// thread: any fixed order serves, the cells only have to tile [0, usable references) without gaps
__global__ __launch_bounds__(kThreads) void rs_tile_sums(RsWs ws) {
  __shared__ uint32_t red[3][kThreads / 64];
  const int64_t base = (int64_t)blockIdx.x * kScanTile;
  uint32_t sum = 0, occ = 0, mx = 0;
#pragma unroll 4
  for (int k = 0; k < kScanPer; ++k) {
    const int64_t s = base + (int64_t)k * kThreads + threadIdx.x;
    const uint32_t c = s < ws.nslots ? ws.table[s].count : 0u;
    sum += c, occ += c != 0, mx = max(mx, c);
  }
  sum = wave_reduce(sum, IntSum()), occ = wave_reduce(occ, IntSum()), mx = wave_reduce(mx, IntMax());
  if ((threadIdx.x & 63) == 0) red[0][threadIdx.x >> 6] = sum, red[1][threadIdx.x >> 6] = occ, red[2][threadIdx.x >> 6] = mx;
  __syncthreads();
  if (threadIdx.x == 0) {
    for (int w = 1; w < kThreads / 64; ++w) sum += red[0][w], occ += red[1][w], mx = max(mx, red[2][w]);
    ws.tile[blockIdx.x] = sum;
    if (occ) {                                         // integer sums and maxima: the same whatever the arrival order
      __hip_atomic_fetch_add(&ws.head->occupied, (uint64_t)occ, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      __hip_atomic_fetch_max(&ws.head->max_cell, mx, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
  }
}

// exclusive scan of the tile sums in place, one workgroup of 1024 threads (the total is below 2^31)
__global__ __launch_bounds__(1024) void rs_scan_tiles(RsWs ws) {
  count_scan(ws.tile, ws.tile, ws.ntiles);
}

__global__ __launch_bounds__(kThreads) void rs_starts(RsWs ws) {
  __shared__ uint32_t wsum[kThreads / 64];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int64_t base = (int64_t)blockIdx.x * kScanTile;
  uint32_t c[kScanPer], sum = 0;
#pragma unroll
  for (int k = 0; k < kScanPer; ++k) {
    const int64_t s = base + (int64_t)k * kThreads + threadIdx.x;
    c[k] = s < ws.nslots ? ws.table[s].count : 0u;
    sum += c[k];
  }
  const uint32_t incl = wave_incl_scan(sum);
  if (lane == 63) wsum[wave] = incl;
  __syncthreads();
  uint32_t run = ws.tile[blockIdx.x] + incl - sum;
  for (int w = 0; w < wave; ++w) run += wsum[w];
#pragma unroll
  for (int k = 0; k < kScanPer; ++k) {
    const int64_t s = base + (int64_t)k * kThreads + threadIdx.x;
    if (s < ws.nslots) ws.table[s].end = run;
    run += c[k];
  }
}

// every usable reference takes the next record of its cell (rs_count claimed the slot in an earlier launch: plain reads find it)
__global__ __launch_bounds__(kThreads) void rs_scatter(ovg_radius_params p, RsWs ws) {
  const uint32_t j = blockIdx.x * kThreads + threadIdx.x;
  float r[3];
  if (j >= (uint32_t)p.nr || !rs_point(p.reference, p.reference_valid, j, r)) return;
  const uint64_t key = rs_key(rs_cell(r[0], rs_origin(p.origin, 0), p.cell), rs_cell(r[1], rs_origin(p.origin, 1), p.cell),
                              rs_cell(r[2], rs_origin(p.origin, 2), p.cell));
  uint32_t count, end;
  const int64_t s = rs_find(ws, key, count, end);
  if (s < 0) return;
  const uint32_t pos = __hip_atomic_fetch_add(&ws.table[s].end, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  if (pos >= (uint32_t)p.nr) return;                   // the counts sum to the usable references: never taken after a matching rs_count
  const u32x4 e = {__float_as_uint(r[0]), __float_as_uint(r[1]), __float_as_uint(r[2]), j};
  ws.rec[pos] = e;
}

// the cost of the search: for every usable query the references in the cells of its box (hash probes only)
__global__ __launch_bounds__(kThreads) void rs_cost(ovg_radius_params p, RsWs ws, float reach) {
  const uint32_t i = blockIdx.x * kThreads + threadIdx.x;
  float q[3];
  uint64_t sum = 0;
  if (i < (uint32_t)p.nq && rs_point(p.query, p.query_valid, i, q)) {
    const RsBox b = rs_box(q, p.origin, p.cell, reach);
    for (uint32_t cx = b.lo[0]; cx <= b.hi[0]; ++cx)
      for (uint32_t cy = b.lo[1]; cy <= b.hi[1]; ++cy)
        for (uint32_t cz = b.lo[2]; cz <= b.hi[2]; ++cz) {
          uint32_t count, end;
          if (rs_find(ws, rs_key(cx, cy, cz), count, end) >= 0) sum += count;
        }
  }
  sum = wave_reduce(sum, IntSum());
  if ((threadIdx.x & 63) == 0 && sum) __hip_atomic_fetch_add(&ws.head->pairs, sum, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

OVG_DEV uint32_t rs_origin_flag(const float* origin) {
  return origin && !finite3(origin[0], origin[1], origin[2]) ? (uint32_t)OVG_RS_BAD_ORIGIN : 0u;
}

// after BUILD: the table now describes this cloud; its statistics leave for the host
__global__ void rs_built(ovg_radius_params p, RsWs ws) {
  RsHead& h = *ws.head;
  h.flags = rs_origin_flag(p.origin);
  h.nr = p.nr;
  p.out_stats[0] = (int64_t)h.flags, p.out_stats[1] = (int64_t)h.occupied, p.out_stats[2] = (int64_t)h.max_cell, p.out_stats[3] = (int64_t)h.pairs;
}

OVG_DEV uint32_t rs_refusal(const ovg_radius_params& p, const RsHead& h) {
  if (h.nr != p.nr) return OVG_RS_NOT_BUILT;
  return h.pairs > (uint64_t)p.max_pairs ? (uint32_t)OVG_RS_OVER_BUDGET : 0u;
}

__global__ void rs_searched(ovg_radius_params p, RsWs ws) {
  const RsHead& h = *ws.head;
  const uint32_t no = rs_refusal(p, h);
  p.out_stats[0] = (int64_t)(no == OVG_RS_NOT_BUILT ? no : (h.flags | no));
  p.out_stats[1] = no == OVG_RS_NOT_BUILT ? 0 : (int64_t)h.occupied;
  p.out_stats[2] = no == OVG_RS_NOT_BUILT ? 0 : (int64_t)h.max_cell;
  p.out_stats[3] = no == OVG_RS_NOT_BUILT ? 0 : (int64_t)h.pairs;
}

// one query per thread: the box of cells, a probe per cell, the rule over the cell's records. The trip counts depend on the data
// (cells per box, records per cell): lanes of a wave idle while the longest of them runs; queries arrive in pixel order, so
// neighbouring lanes mostly share their cells
__global__ __launch_bounds__(kThreads) void rs_search(ovg_radius_params p, RsWs ws, float reach) {
  if (rs_refusal(p, *ws.head)) return;                 // the work guard, the same in every thread: nothing is written
  const uint32_t i = blockIdx.x * kThreads + threadIdx.x;
  if (i >= (uint32_t)p.nq) return;
  float q[3];
  int32_t cnt = 0;
  uint64_t best = kNoneKey;
  if (rs_point(p.query, p.query_valid, i, q)) {
    const uint32_t rbits = __float_as_uint(p.radius_sq), nr = (uint32_t)p.nr;
    const bool exclude = (p.flags & OVG_RS_EXCLUDE_SAME_INDEX) != 0;
    const RsBox b = rs_box(q, p.origin, p.cell, reach);
    for (uint32_t cx = b.lo[0]; cx <= b.hi[0]; ++cx)
      for (uint32_t cy = b.lo[1]; cy <= b.hi[1]; ++cy)
        for (uint32_t cz = b.lo[2]; cz <= b.hi[2]; ++cz) {
          uint32_t count, end;
          if (rs_find(ws, rs_key(cx, cy, cz), count, end) < 0) continue;
          end = min(end, nr);                          // a workspace another call has scribbled over still cannot send a read outside rec
          const uint32_t first = end - min(count, end);
#pragma unroll 4
          for (uint32_t r = first; r < end; ++r) {
            const u32x4 e = ws.rec[r];
            const float dx = q[0] - __uint_as_float(e[0]), dy = q[1] - __uint_as_float(e[1]), dz = q[2] - __uint_as_float(e[2]);
            const float d = (dx * dx + dy * dy) + dz * dz;                 // +0, positive or +inf: the bits order like the value
            const uint32_t bits = __float_as_uint(d);
            const bool ok = bits <= rbits && !(exclude && e[3] == i);
            const uint64_t key = ((uint64_t)bits << 32) | e[3];            // (bits(d), j): the order inside a cell does not matter
            cnt += ok;
            best = ok && key < best ? key : best;
          }
        }
  }
  const bool found = best != kNoneKey;
  p.count[i] = cnt;
  p.index[i] = found ? (int32_t)(uint32_t)best : -1;
  p.sqdist[i] = __uint_as_float(found ? (uint32_t)(best >> 32) : kInfBits);
}

// ovg_knn_search: rs_search's walk, keeping the K smallest keys instead of the smallest. The selection is a sorted list of K keys in
// registers (key[0] the nearest). A candidate first meets the worst key: one 64-bit compare, and most candidates end there once the
// list is full of near points. An accepted one runs a chain of K compare-and-swaps from the front, which carries the larger key of
// every pair on and drops the last: every index is a compile-time constant after unrolling, so the list never goes to scratch (a
// runtime-indexed per-thread array would). Keys of different references differ in their low word, so no compare ever ties. The K
// smallest keys hold the k <= K smallest: the result does not depend on the instance that ran.
template <int K>
__global__ __launch_bounds__(kThreads) void knn_search(ovg_radius_params p, RsWs ws, float reach, int32_t k, int32_t* index, float* sqdist) {
  if (rs_refusal(p, *ws.head)) return;                 // the work guard, the same in every thread: nothing is written
  const uint32_t i = blockIdx.x * kThreads + threadIdx.x;
  if (i >= (uint32_t)p.nq) return;
  float q[3];
  int32_t cnt = 0;
  uint64_t key[K];
#pragma unroll
  for (int t = 0; t < K; ++t) key[t] = kNoneKey;
  if (rs_point(p.query, p.query_valid, i, q)) {
    const uint32_t rbits = __float_as_uint(p.radius_sq), nr = (uint32_t)p.nr;
    const bool exclude = (p.flags & OVG_RS_EXCLUDE_SAME_INDEX) != 0;
    const RsBox b = rs_box(q, p.origin, p.cell, reach);
    for (uint32_t cx = b.lo[0]; cx <= b.hi[0]; ++cx)
      for (uint32_t cy = b.lo[1]; cy <= b.hi[1]; ++cy)
        for (uint32_t cz = b.lo[2]; cz <= b.hi[2]; ++cz) {
          uint32_t count, end;
          if (rs_find(ws, rs_key(cx, cy, cz), count, end) < 0) continue;
          end = min(end, nr);
          const uint32_t first = end - min(count, end);
          for (uint32_t r = first; r < end; ++r) {
            const u32x4 e = ws.rec[r];
            const float dx = q[0] - __uint_as_float(e[0]), dy = q[1] - __uint_as_float(e[1]), dz = q[2] - __uint_as_float(e[2]);
            const float d = (dx * dx + dy * dy) + dz * dz;
            const uint32_t bits = __float_as_uint(d);
            const bool ok = bits <= rbits && !(exclude && e[3] == i);
            uint64_t c = ((uint64_t)bits << 32) | e[3];
            cnt += ok;
            if (ok && c < key[K - 1]) {
#pragma unroll
              for (int t = 0; t < K; ++t) {
                const bool below = c < key[t];
                const uint64_t lo = below ? c : key[t], hi = below ? key[t] : c;
                key[t] = lo, c = hi;
              }
            }
          }
        }
  }
  p.count[i] = cnt;
  int32_t* oi = index + (int64_t)i * k;
  float* od = sqdist + (int64_t)i * k;
#pragma unroll
  for (int t = 0; t < K; ++t) {
    if (t < k) {
      const bool found = key[t] != kNoneKey;
      oi[t] = found ? (int32_t)(uint32_t)key[t] : -1;
      od[t] = __uint_as_float(found ? (uint32_t)(key[t] >> 32) : kInfBits);
    }
  }
}

// ---------------------------------------------------------------------------------------------------------------------------------
// ovg_cluster: connected components / DBSCAN over the grid (the rule: include/omnivggt_hip.h). Four launches, the kernel boundary the
// only ordering between them: degree (rs_search's walk, counting; kind and the parent array), link (a lock-free union-find over the
// neighbour pairs of core points), flatten (root = find), border (non-core points join their nearest core neighbour's cluster).
// `root` IS the union-find's parent array while the launches run.
//
// The union-find (cl_ld, cl_find, cl_unite) and the invariant / termination proof that stands above it live in ovg_geom.h: ovg_mesh_topology
// runs the same code over the corners of the live faces.

// rs_search's walk over the box of point i of the one cloud: visit(bits(d), j) for every neighbour record (rule 2: j != i)
template <class Visit>
OVG_DEV void cl_walk(const ovg_radius_params& p, const RsWs& ws, float reach, uint32_t i, const float (&q)[3], Visit&& visit) {
  const uint32_t rbits = __float_as_uint(p.radius_sq), nr = (uint32_t)p.nr;
  const RsBox b = rs_box(q, p.origin, p.cell, reach);
  for (uint32_t cx = b.lo[0]; cx <= b.hi[0]; ++cx)
    for (uint32_t cy = b.lo[1]; cy <= b.hi[1]; ++cy)
      for (uint32_t cz = b.lo[2]; cz <= b.hi[2]; ++cz) {
        uint32_t count, end;
        if (rs_find(ws, rs_key(cx, cy, cz), count, end) < 0) continue;
        end = min(end, nr);
        const uint32_t first = end - min(count, end);
        for (uint32_t r = first; r < end; ++r) {
          const u32x4 e = ws.rec[r];
          const float dx = q[0] - __uint_as_float(e[0]), dy = q[1] - __uint_as_float(e[1]), dz = q[2] - __uint_as_float(e[2]);
          const float d = (dx * dx + dy * dy) + dz * dz;
          const uint32_t bits = __float_as_uint(d);
          if (bits <= rbits && e[3] != i) visit(bits, e[3]);
        }
      }
}

OVG_DEV void cl_fail(const RsWs& ws) {
  __hip_atomic_fetch_or(&ws.head->cl_flags, (uint32_t)OVG_CL_INTERNAL, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

// degree, kind (CORE, or NOISE for a usable point not yet decided: cl_border raises it to BORDER) and parent (i for a core point)
__global__ __launch_bounds__(kThreads) void cl_degree(ovg_radius_params p, RsWs ws, float reach, int32_t min_neighbours, int32_t* root,
                                                      uint8_t* kind, int32_t* degree) {
  if (rs_refusal(p, *ws.head)) return;                 // the work guard, the same in every thread: nothing is written
  const uint32_t i = blockIdx.x * kThreads + threadIdx.x;
  if (i == 0) ws.head->cl_flags = 0u;                  // no thread of this launch raises it
  if (i >= (uint32_t)p.nr) return;
  float q[3];
  int32_t cnt = 0;
  const bool usable = rs_point(p.query, p.query_valid, i, q);
  if (usable) cl_walk(p, ws, reach, i, q, [&](uint32_t, uint32_t) { ++cnt; });
  const bool core = usable && cnt >= min_neighbours;
  root[i] = core ? (int32_t)i : -1;
  kind[i] = (uint8_t)(!usable ? OVG_CL_UNUSABLE : (core ? OVG_CL_CORE : OVG_CL_NOISE));
  if (degree) degree[i] = cnt;
}

// every core i unites itself with every core neighbour j < i (the relation is symmetric bit for bit: the pair is met from its
// higher end). kind is read plainly: cl_degree wrote it in an earlier launch and nothing writes it here
__global__ __launch_bounds__(kThreads) void cl_link(ovg_radius_params p, RsWs ws, float reach, int32_t* parent, const uint8_t* kind) {
  if (rs_refusal(p, *ws.head)) return;
  const uint32_t i = blockIdx.x * kThreads + threadIdx.x, n = (uint32_t)p.nr;
  float q[3];
  if (i >= n || kind[i] != OVG_CL_CORE || !rs_point(p.query, p.query_valid, i, q)) return;
  const uint64_t budget = 4ull * n + 4;
  bool fine = true;
  cl_walk(p, ws, reach, i, q, [&](uint32_t, uint32_t j) {
    // a record's index is followed here: one from a workspace another call has scribbled over must not leave the arrays
    if (j < i && kind[j] == OVG_CL_CORE && fine) fine = cl_unite(parent, (int32_t)i, (int32_t)j, budget);
  });
  if (!fine) cl_fail(ws);
}

// root[i] = find(i) for the core points. No hook runs in this launch, so the roots are final: the min stores the tree's root
__global__ __launch_bounds__(kThreads) void cl_flatten(ovg_radius_params p, RsWs ws, int32_t* parent, const uint8_t* kind) {
  if (rs_refusal(p, *ws.head)) return;
  const uint32_t i = blockIdx.x * kThreads + threadIdx.x, n = (uint32_t)p.nr;
  if (i >= n || kind[i] != OVG_CL_CORE) return;
  uint64_t budget = 4ull * n + 4;
  const int32_t r = cl_find(parent, (int32_t)i, budget);
  if (r < 0) { cl_fail(ws); return; }
  __hip_atomic_fetch_min(parent + i, r, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

// every usable non-core i joins the core neighbour that minimises (bits(d), j), or stays NOISE. root and kind of CORE points are
// final and read plainly; a thread writes only its own non-core entries, and a reader that meets NOISE or BORDER there sees "not
// CORE" either way
__global__ __launch_bounds__(kThreads) void cl_border(ovg_radius_params p, RsWs ws, float reach, int32_t* root, uint8_t* kind) {
  if (rs_refusal(p, *ws.head)) return;
  const uint32_t i = blockIdx.x * kThreads + threadIdx.x, n = (uint32_t)p.nr;
  float q[3];
  if (i >= n || kind[i] != OVG_CL_NOISE || !rs_point(p.query, p.query_valid, i, q)) return;
  uint64_t best = kNoneKey;
  cl_walk(p, ws, reach, i, q, [&](uint32_t bits, uint32_t j) {
    const uint64_t key = ((uint64_t)bits << 32) | j;
    if (j < n && key < best && kind[j] == OVG_CL_CORE) best = key;
  });
  if (best == kNoneKey) return;
  root[i] = root[(uint32_t)best];
  kind[i] = (uint8_t)OVG_CL_BORDER;
}

__global__ void cl_done(ovg_radius_params p, RsWs ws) {
  const RsHead& h = *ws.head;
  const uint32_t no = rs_refusal(p, h);
  p.out_stats[0] = (int64_t)(no == OVG_RS_NOT_BUILT ? no : (h.flags | no | (no ? 0u : h.cl_flags)));
  p.out_stats[1] = no == OVG_RS_NOT_BUILT ? 0 : (int64_t)h.occupied;
  p.out_stats[2] = no == OVG_RS_NOT_BUILT ? 0 : (int64_t)h.max_cell;
  p.out_stats[3] = no == OVG_RS_NOT_BUILT ? 0 : (int64_t)h.pairs;
}

unsigned grid_for(int64_t work, int64_t per_block, int64_t cap) {
  const int64_t b = (work + per_block - 1) / per_block;
  return (unsigned)(b < 1 ? 1 : (b > cap ? cap : b));
}

}  // namespace

extern "C" int64_t ovg_radius_workspace_bytes(int64_t nq, int64_t nr) { return rs_shape_ok(nq, nr) ? rs_ws_bytes(nr) : -1; }

extern "C" int ovg_radius_search(const ovg_radius_params* p, void* stream) {
  if (!p || !p->query || !p->reference || !p->ws) return OVG_E_ARG;
  if (!rs_shape_ok(p->nq, p->nr) || (p->flags & ~OVG_RS_EXCLUDE_SAME_INDEX)) return OVG_E_ARG;
  if (p->stage < 1 || p->stage > (OVG_RS_BUILD | OVG_RS_SEARCH)) return OVG_E_ARG;
  if ((p->flags & OVG_RS_EXCLUDE_SAME_INDEX) && p->nq != p->nr) return OVG_E_ARG;
  if (!(p->radius_sq >= kMinRadiusSq) || !isfinite(p->radius_sq)) return OVG_E_ARG;
  const float reach = rs_reach(p->radius_sq);
  if (!(p->cell >= reach) || !isfinite(p->cell)) return OVG_E_ARG;
  if ((p->stage & OVG_RS_BUILD) && !p->out_stats) return OVG_E_ARG;
  if ((p->stage & OVG_RS_SEARCH) && (!p->count || !p->index || !p->sqdist || p->max_pairs < 0)) return OVG_E_ARG;
  if (!al(p->query, 4) || !al(p->reference, 4) || !al(p->origin, 4) || !al(p->count, 4) || !al(p->index, 4) || !al(p->sqdist, 4) ||
      !al(p->out_stats, 8))
    return OVG_E_ARG;
  if (!al(p->ws, 16) || p->ws_bytes < rs_ws_bytes(p->nr)) return OVG_E_ARG;
  hipStream_t st = static_cast<hipStream_t>(stream);
  const RsWs ws = rs_ws(p);
  const dim3 block(kThreads), per_ref((unsigned)((p->nr + kThreads - 1) / kThreads)), per_query((unsigned)((p->nq + kThreads - 1) / kThreads));
  if (p->stage & OVG_RS_BUILD) {
    OVG_LAUNCH(rs_clear, dim3(grid_for(ws.nslots, kThreads * 4, 4096)), block, 0, st, ws);
    OVG_CHECK_LAUNCH();
    OVG_LAUNCH(rs_count, per_ref, block, 0, st, *p, ws);
    OVG_CHECK_LAUNCH();
    OVG_LAUNCH(rs_tile_sums, dim3((unsigned)ws.ntiles), block, 0, st, ws);
    OVG_CHECK_LAUNCH();
    OVG_LAUNCH(rs_scan_tiles, dim3(1), dim3(1024), 0, st, ws);
    OVG_CHECK_LAUNCH();
    OVG_LAUNCH(rs_starts, dim3((unsigned)ws.ntiles), block, 0, st, ws);
    OVG_CHECK_LAUNCH();
    OVG_LAUNCH(rs_scatter, per_ref, block, 0, st, *p, ws);
    OVG_CHECK_LAUNCH();
    OVG_LAUNCH(rs_cost, per_query, block, 0, st, *p, ws, reach);
    OVG_CHECK_LAUNCH();
    OVG_LAUNCH(rs_built, dim3(1), dim3(1), 0, st, *p, ws);
    OVG_CHECK_LAUNCH();
  }
  if (p->stage & OVG_RS_SEARCH) {
    OVG_LAUNCH(rs_search, per_query, block, 0, st, *p, ws, reach);
    OVG_CHECK_LAUNCH();
    if (p->out_stats) {
      OVG_LAUNCH(rs_searched, dim3(1), dim3(1), 0, st, *p, ws);
      OVG_CHECK_LAUNCH();
    }
  }
  return OVG_OK;
}

extern "C" int ovg_knn_search(const ovg_knn_params* p, void* stream) {
  if (!p || !p->query || !p->reference || !p->ws) return OVG_E_ARG;
  if (!rs_shape_ok(p->nq, p->nr) || (p->flags & ~OVG_RS_EXCLUDE_SAME_INDEX)) return OVG_E_ARG;
  if (p->k < 1 || p->k > OVG_KNN_MAX_K) return OVG_E_ARG;
  if ((p->flags & OVG_RS_EXCLUDE_SAME_INDEX) && p->nq != p->nr) return OVG_E_ARG;
  if (!(p->radius_sq >= kMinRadiusSq) || !isfinite(p->radius_sq)) return OVG_E_ARG;
  const float reach = rs_reach(p->radius_sq);
  if (!(p->cell >= reach) || !isfinite(p->cell)) return OVG_E_ARG;
  if (!p->count || !p->index || !p->sqdist || p->max_pairs < 0) return OVG_E_ARG;
  if (!al(p->query, 4) || !al(p->reference, 4) || !al(p->origin, 4) || !al(p->count, 4) || !al(p->index, 4) || !al(p->sqdist, 4) ||
      !al(p->out_stats, 8))
    return OVG_E_ARG;
  if (!al(p->ws, 16) || p->ws_bytes < rs_ws_bytes(p->nr)) return OVG_E_ARG;
  // the search stage of ovg_radius_search over the same workspace: its params carry the grid's description, the guard and count
  const ovg_radius_params rp = {p->query, p->reference, p->query_valid, p->reference_valid, p->origin, p->nq, p->nr, p->radius_sq, p->cell,
                                p->flags, OVG_RS_SEARCH, p->max_pairs, p->ws, p->ws_bytes, p->out_stats, p->count, nullptr, nullptr};
  hipStream_t st = static_cast<hipStream_t>(stream);
  const RsWs ws = rs_ws(&rp);
  const dim3 block(kThreads), per_query((unsigned)((p->nq + kThreads - 1) / kThreads));
  if (p->k <= 4) {
    OVG_LAUNCH(knn_search<4>, per_query, block, 0, st, rp, ws, reach, p->k, p->index, p->sqdist);
  } else if (p->k <= 8) {
    OVG_LAUNCH(knn_search<8>, per_query, block, 0, st, rp, ws, reach, p->k, p->index, p->sqdist);
  } else if (p->k <= 16) {
    OVG_LAUNCH(knn_search<16>, per_query, block, 0, st, rp, ws, reach, p->k, p->index, p->sqdist);
  } else {
    OVG_LAUNCH(knn_search<32>, per_query, block, 0, st, rp, ws, reach, p->k, p->index, p->sqdist);
  }
  OVG_CHECK_LAUNCH();
  if (p->out_stats) {
    OVG_LAUNCH(rs_searched, dim3(1), dim3(1), 0, st, rp, ws);
    OVG_CHECK_LAUNCH();
  }
  return OVG_OK;
}

extern "C" int ovg_cluster(const ovg_cluster_params* p, void* stream) {
  if (!p || !p->points || !p->ws) return OVG_E_ARG;
  if (!rs_shape_ok(p->n, p->n) || p->flags != 0 || p->min_neighbours < 0) return OVG_E_ARG;
  if (!(p->radius_sq >= kMinRadiusSq) || !isfinite(p->radius_sq)) return OVG_E_ARG;
  const float reach = rs_reach(p->radius_sq);
  if (!(p->cell >= reach) || !isfinite(p->cell)) return OVG_E_ARG;
  if (!p->root || !p->kind || p->max_pairs < 0) return OVG_E_ARG;
  if (!al(p->points, 4) || !al(p->origin, 4) || !al(p->root, 4) || !al(p->degree, 4) || !al(p->out_stats, 8)) return OVG_E_ARG;
  if (!al(p->ws, 16) || p->ws_bytes < rs_ws_bytes(p->n)) return OVG_E_ARG;
  // the search stage of ovg_radius_search inside one cloud over the same workspace: its params carry the grid's description and the guard
  const ovg_radius_params rp = {p->points, p->points, p->valid, p->valid, p->origin, p->n, p->n, p->radius_sq, p->cell,
                                OVG_RS_EXCLUDE_SAME_INDEX, OVG_RS_SEARCH, p->max_pairs, p->ws, p->ws_bytes, p->out_stats, nullptr, nullptr, nullptr};
  hipStream_t st = static_cast<hipStream_t>(stream);
  const RsWs ws = rs_ws(&rp);
  const dim3 block(kThreads), per_point((unsigned)((p->n + kThreads - 1) / kThreads));
  OVG_LAUNCH(cl_degree, per_point, block, 0, st, rp, ws, reach, p->min_neighbours, p->root, p->kind, p->degree);
  OVG_CHECK_LAUNCH();
  OVG_LAUNCH(cl_link, per_point, block, 0, st, rp, ws, reach, p->root, p->kind);
  OVG_CHECK_LAUNCH();
  OVG_LAUNCH(cl_flatten, per_point, block, 0, st, rp, ws, p->root, p->kind);
  OVG_CHECK_LAUNCH();
  OVG_LAUNCH(cl_border, per_point, block, 0, st, rp, ws, reach, p->root, p->kind);
  OVG_CHECK_LAUNCH();
  if (p->out_stats) {
    OVG_LAUNCH(cl_done, dim3(1), dim3(1), 0, st, rp, ws);
    OVG_CHECK_LAUNCH();
  }
  return OVG_OK;
}
