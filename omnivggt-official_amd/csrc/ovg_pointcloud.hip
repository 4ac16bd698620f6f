// Point-cloud extraction (visual_util.py:113-236, the selection core of predictions_to_glb): exact numpy-2 linear percentiles by radix
// select (ovg_percentile) and the confidence / background filter with an order-preserving compaction (ovg_point_filter).
// Every kernel is HBM bound: the selection reads each key three times and the filter reads conf / image twice; no launch waits on the host.
// Voxel-grid decimation of a selected cloud (ovg_voxel_downsample) shares the filter's count / scan / scatter; its hash stage is bound
// by random 64-bit atomics, not by bandwidth.
#include "ovg_geom.h"

// the percentile's lerp and the scene-scale norm restate numpy's f32 / f64 operation sequence: no fused multiply-adds anywhere in this
// unit. The pragma covers the code below; build.py also compiles the unit with -ffp-contract=off, which reaches the inlined HIP header
// helpers too (their plain `x * y` would otherwise fuse with a neighbouring add: one ulp off numpy, seen on the device)
#pragma clang fp contract(off)

namespace {

constexpr int kThreads = 256;
constexpr int kMaxTargets = 2 * OVG_PCT_MAX_Q;     // ranks lo and hi of every percentile
constexpr int kSlots = kMaxTargets;                 // distinct key prefixes a pass may follow per column
constexpr int kBins1 = 2048, kBins2 = 2048, kBins3 = 1024;   // 11 / 11 / 10 bits of the u32 key
constexpr int kHistWords = kBins1 + kSlots * kBins2 + kSlots * kBins3;   // u64 counters per column
constexpr int kPerThread = 16;                      // keys per thread per grid-stride step
constexpr int kTile = kThreads * 16;                // pixels per workgroup of the filter

struct PctPlan {                                    // from the host: the same ranks / weights for every column (same n)
  int64_t rank[kMaxTargets];
  float gamma[OVG_PCT_MAX_Q];
  int32_t nq;
};

struct PctState {                                   // per column, in the workspace after the histograms
  uint64_t rank[kMaxTargets];                       // rank inside the keys that share `prefix`
  uint32_t prefix[kMaxTargets];
  int32_t slot[kMaxTargets];                        // histogram slot the target reads in the next pass
  uint32_t slot_prefix[kSlots];
  int32_t nslot;
  int32_t pad;
  uint64_t nan;
};

OVG_DEV uint32_t order_key(float f) {
  // order-preserving u32 of an f32; every NaN becomes the largest key (numpy sorts NaN last)
  const uint32_t u = __float_as_uint(f);
  if (f != f) return 0xFFFFFFFFu;
  return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}

OVG_DEV float key_value(uint32_t k) { return __uint_as_float((k & 0x80000000u) ? (k & 0x7FFFFFFFu) : ~k); }

OVG_DEV float masked(float v, const float* mask, int64_t i) {
  // visual_util.py:187-188: conf * (sky_mask > 0.1) as float, evaluated literally (inf * 0 is NaN there too)
  return mask ? v * (mask[i] > 0.1f ? 1.0f : 0.0f) : v;
}

// workspace: ncols x kHistWords u64 counters, then ncols PctState
int64_t state_offset_bytes(int32_t ncols) { return (int64_t)ncols * kHistWords * 8; }
int64_t pct_ws_bytes(int32_t ncols) { return state_offset_bytes(ncols) + (int64_t)ncols * (int64_t)sizeof(PctState); }

__global__ __launch_bounds__(kThreads) void pct_init(uint64_t* hist, PctState* st, int32_t ncols, PctPlan plan) {
  const int64_t words = (int64_t)ncols * kHistWords;
  for (int64_t i = (int64_t)blockIdx.x * kThreads + threadIdx.x; i < words; i += (int64_t)gridDim.x * kThreads) hist[i] = 0;
  if (blockIdx.x == 0 && threadIdx.x < (unsigned)ncols) {
    PctState& s = st[threadIdx.x];
    for (int t = 0; t < kMaxTargets; ++t) {
      s.rank[t] = t < 2 * plan.nq ? (uint64_t)plan.rank[t] : 0;
      s.prefix[t] = 0;
      s.slot[t] = 0;
      s.slot_prefix[t] = 0;
    }
    s.nslot = 1;
    s.pad = 0;
    s.nan = 0;
  }
}

// PASS 1: bits 31..21 of every key; PASS 2: bits 20..10 of the keys whose bits 31..21 equal a slot prefix; PASS 3: bits 9..0 under a
// 22-bit prefix. One LDS histogram per slot, flushed with integer agent-scope atomics (exact, so the counts are deterministic).
template <int PASS>
__global__ __launch_bounds__(kThreads) void pct_hist(ovg_percentile_params p, uint64_t* hist, const PctState* st) {
  constexpr int BINS = PASS == 3 ? kBins3 : 2048;
  constexpr int NS = PASS == 1 ? 1 : kSlots;
  constexpr int SHIFT = PASS == 1 ? 21 : (PASS == 2 ? 10 : 0);
  constexpr int PSHIFT = PASS == 2 ? 21 : 10;        // bits of the prefix the key must match
  __shared__ uint32_t h[NS * BINS];
  const int c = blockIdx.y;
  const PctState& s = st[c];
  const int nslot = PASS == 1 ? 1 : s.nslot;
  uint32_t sp[NS];
#pragma unroll
  for (int k = 0; k < NS; ++k) sp[k] = PASS == 1 ? 0u : s.slot_prefix[k];
  for (int i = threadIdx.x; i < nslot * BINS; i += kThreads) h[i] = 0;
  __syncthreads();
  const float* x = p.x + (int64_t)c * p.col_stride;
  const int64_t step = (int64_t)gridDim.x * kThreads * kPerThread;
  for (int64_t base = (int64_t)blockIdx.x * kThreads * kPerThread; base < p.n; base += step) {
#pragma unroll 4
    for (int j = 0; j < kPerThread; ++j) {
      const int64_t i = base + (int64_t)j * kThreads + threadIdx.x;
      if (i >= p.n) break;
      const uint32_t key = order_key(masked(x[i * p.stride], p.mask, i));
      const uint32_t bin = (key >> SHIFT) & (BINS - 1);
      if (PASS == 1) {
        atomicAdd(&h[bin], 1u);
      } else {
        const uint32_t pre = key >> PSHIFT;
#pragma unroll
        for (int k = 0; k < NS; ++k)                    // slot prefixes are distinct: at most one matches
          if (k < nslot && pre == sp[k]) atomicAdd(&h[k * BINS + bin], 1u);
      }
    }
  }
  __syncthreads();
  uint64_t* g = hist + (int64_t)c * kHistWords + (PASS == 1 ? 0 : (PASS == 2 ? kBins1 : kBins1 + kSlots * kBins2));
  for (int i = threadIdx.x; i < nslot * BINS; i += kThreads)
    if (h[i]) __hip_atomic_fetch_add(&g[i], (uint64_t)h[i], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

OVG_DEV float lerp_numpy(float a, float b, float t) {
  // numpy _lerp: a + (b-a)*t, and b - (b-a)*(1-t) where t >= 0.5; literally, so inf order statistics give numpy's NaN
  const float d = b - a;
  return t >= 0.5f ? b - d * (1.0f - t) : a + d * t;
}

// One workgroup: for every column and target, the bin of this pass that holds the target's rank; then the slots of the next pass
// (distinct prefixes) or, after PASS 3, the order statistics, the lerp and the optional norm.
template <int PASS>
__global__ __launch_bounds__(kThreads) void pct_pick(ovg_percentile_params p, const uint64_t* hist, PctState* st, PctPlan plan) {
  constexpr int BINS = PASS == 3 ? kBins3 : 2048;
  constexpr int PER = BINS / kThreads;
  constexpr int BITS = PASS == 3 ? 10 : 11;
  __shared__ uint64_t wsum[kThreads / 64];
  __shared__ uint32_t found_bin;
  __shared__ uint64_t found_rank;
  __shared__ float vals[OVG_PCT_MAX_COLS][kMaxTargets];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int ntarget = 2 * plan.nq;
  for (int c = 0; c < p.ncols; ++c) {
    PctState& s = st[c];
    const uint64_t* g = hist + (int64_t)c * kHistWords + (PASS == 1 ? 0 : (PASS == 2 ? kBins1 : kBins1 + kSlots * kBins2));
    for (int t = 0; t < ntarget; ++t) {
      const uint64_t* hs = g + (PASS == 1 ? 0 : s.slot[t] * BINS);
      uint64_t local[PER], sum = 0;
#pragma unroll
      for (int k = 0; k < PER; ++k) { local[k] = hs[threadIdx.x * PER + k]; sum += local[k]; }
      const uint64_t incl = wave_incl_scan(sum);
      if (lane == 63) wsum[wave] = incl;
      __syncthreads();
      uint64_t excl = incl - sum;
      for (int w = 0; w < wave; ++w) excl += wsum[w];
      const uint64_t r = s.rank[t];
      if (r >= excl && r < excl + sum) {
        uint64_t run = excl;
#pragma unroll
        for (int k = 0; k < PER; ++k) {
          if (r >= run && r < run + local[k]) { found_bin = threadIdx.x * PER + k; found_rank = r - run; }
          run += local[k];
        }
      }
      __syncthreads();
      if (threadIdx.x == 0) {
        s.prefix[t] = (s.prefix[t] << BITS) | found_bin;
        s.rank[t] = found_rank;
        if (PASS == 1 && t == 0) s.nan = g[kBins1 - 1];     // only NaN keys (0xFFFFFFFF) reach the top bin
        if (PASS == 3) vals[c][t] = key_value(s.prefix[t]);
      }
      __syncthreads();
    }
    if (threadIdx.x == 0 && PASS < 3) {                    // slots of the next pass: one per distinct prefix
      int n = 0;
      for (int t = 0; t < ntarget; ++t) {
        int k = 0;
        while (k < n && s.slot_prefix[k] != s.prefix[t]) ++k;
        if (k == n) s.slot_prefix[n++] = s.prefix[t];
        s.slot[t] = k;
      }
      s.nslot = n;
    }
  }
  if (PASS == 3 && threadIdx.x == 0) {
    // norm_out: np.linalg.norm of the f32 spread (percentile 1 - percentile 0 per column) as numpy evaluates it -- the BLAS dot sums the
    // f32-rounded products in f64 left to right, the sum is rounded to f32, the square root is correctly rounded
    double acc = 0.0;
    for (int c = 0; c < p.ncols; ++c) {
      float first = 0.0f, last = 0.0f;
      for (int j = 0; j < plan.nq; ++j) {
        const float v = st[c].nan ? __uint_as_float(0x7FC00000u) : lerp_numpy(vals[c][2 * j], vals[c][2 * j + 1], plan.gamma[j]);
        p.out[c * plan.nq + j] = v;
        if (j == 0) first = v;
        last = v;
      }
      const float d = last - first;
      const float sq = d * d;
      acc = acc + (double)sq;
    }
    if (p.norm_out) *p.norm_out = __fsqrt_rn((float)acc);      // correctly rounded, like np.sqrt
  }
}

// ---------------------------------------------------------------------------------------------------------------------------------
// filter: keep = conf' >= thr && conf' > min_conf (&& background tests on the u8 colours), conf' = conf * (mask > 0.1)
// ---------------------------------------------------------------------------------------------------------------------------------
OVG_DEV uint32_t color_u8(float v) {
  // numpy (x * 255).astype(uint8) for x in [0, 1]: one f32 multiply, truncation; clamped to [0, 255] outside (NaN -> 0)
  const float f = fminf(fmaxf(v * 255.0f, 0.0f), 255.0f);
  return (uint32_t)(int)f;
}

OVG_DEV void pixel_rgb(const ovg_point_filter_params& p, int64_t i, uint32_t& r, uint32_t& g, uint32_t& b) {
  const int64_t s = i / p.hw, px = i - s * p.hw;
  const float* im = p.images + s * 3 * p.hw + px;
  r = color_u8(im[0]);
  g = color_u8(im[p.hw]);
  b = color_u8(im[2 * p.hw]);
}

OVG_DEV bool keep_pixel(const ovg_point_filter_params& p, float thr, int64_t i) {
  const float c = masked(p.conf[i], p.mask, i);
  bool k = (c >= thr) & (c > p.min_conf);
  if (k && (p.flags & (OVG_PF_BLACK_BG | OVG_PF_WHITE_BG))) {
    uint32_t r, g, b;
    pixel_rgb(p, i, r, g, b);
    if ((p.flags & OVG_PF_BLACK_BG) && r + g + b < 16) k = false;
    if ((p.flags & OVG_PF_WHITE_BG) && r > 240 && g > 240 && b > 240) k = false;
  }
  return k;
}

struct PfWs {
  uint8_t* keep; int64_t* counts; int64_t* offsets;
};

int64_t pf_blocks(int64_t n) { return (n + kTile - 1) / kTile; }
int64_t pf_ws_bytes(int64_t n) { return round256(n) + 2 * round256(pf_blocks(n) * 8); }
PfWs pf_ws(const ovg_point_filter_params* p) {
  uint8_t* b = static_cast<uint8_t*>(p->ws);
  const int64_t nb = pf_blocks(p->n);
  return {b, reinterpret_cast<int64_t*>(b + round256(p->n)), reinterpret_cast<int64_t*>(b + round256(p->n) + round256(nb * 8))};
}

__global__ __launch_bounds__(kThreads) void pf_mask(ovg_point_filter_params p, PfWs ws) {
  __shared__ int64_t red[kThreads / 64];
  const float thr = p.threshold ? *p.threshold : 0.0f;
  const int64_t base = (int64_t)blockIdx.x * kTile;
  int64_t cnt = 0;
#pragma unroll 4
  for (int j = 0; j < kTile / kThreads; ++j) {
    const int64_t i = base + (int64_t)j * kThreads + threadIdx.x;
    if (i < p.n) {
      const bool k = keep_pixel(p, thr, i);
      ws.keep[i] = k;
      cnt += k;
    }
  }
  const int64_t t = block_reduce<kThreads>(cnt, red, IntSum());
  if (threadIdx.x == 0) ws.counts[blockIdx.x] = t;
}

// exclusive scan of the per-workgroup counts in one workgroup of 1024 threads; the total is the cloud size
__global__ __launch_bounds__(1024) void pf_scan(PfWs ws, int64_t nblk, int64_t* out_count) {
  const int64_t total = count_scan(ws.counts, ws.offsets, nblk);
  if (threadIdx.x == 0) *out_count = total;
}

// order-preserving scatter: entry i of the tile lands at offset[block] + (kept entries before it in the tile); the order inside a
// tile is j-major (j * 256 + thread), so the rank is the count of the earlier (j, wave) groups plus the lanes below in the ballot.
// emit(i, pos) copies entry i to output position pos (< capacity); every thread of the workgroup calls this once
template <class Emit>
OVG_DEV void scatter_tile(const uint8_t* keep, int64_t n, const int64_t* offsets, int64_t capacity, Emit emit) {
  constexpr int J = kTile / kThreads;
  __shared__ uint32_t cnt[J * (kThreads / 64)];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int64_t base = (int64_t)blockIdx.x * kTile;
  uint32_t bits = 0;
#pragma unroll
  for (int j = 0; j < J; ++j) {
    const int64_t i = base + (int64_t)j * kThreads + threadIdx.x;
    const bool k = i < n && keep[i];
    bits |= (uint32_t)k << j;
    const uint64_t bal = __ballot(k);
    if (lane == 0) cnt[j * (kThreads / 64) + wave] = __popcll(bal);
  }
  __syncthreads();
  if (wave == 0) {                                     // 64 groups: one exclusive scan in wave 0
    const uint64_t v = cnt[lane];
    cnt[lane] = (uint32_t)(wave_incl_scan(v) - v);
  }
  __syncthreads();
  const int64_t off = offsets[blockIdx.x];
  const uint64_t below = (1ull << lane) - 1ull;
#pragma unroll
  for (int j = 0; j < J; ++j) {
    const bool k = (bits >> j) & 1u;
    const uint64_t bal = __ballot(k);
    if (!k) continue;
    const int64_t i = base + (int64_t)j * kThreads + threadIdx.x;
    const int64_t pos = off + cnt[j * (kThreads / 64) + wave] + __popcll(bal & below);
    if (pos >= capacity) continue;
    emit(i, pos);
  }
}

__global__ __launch_bounds__(kThreads) void pf_scatter(ovg_point_filter_params p, PfWs ws) {
  scatter_tile(ws.keep, p.n, ws.offsets, p.capacity, [&](int64_t i, int64_t pos) {
    const float* src = p.points + i * 3;
    float* dst = p.out_points + pos * 3;
    dst[0] = src[0];
    dst[1] = src[1];
    dst[2] = src[2];
    uint32_t r, g, b;
    pixel_rgb(p, i, r, g, b);
    uint8_t* col = p.out_colors + pos * 3;
    col[0] = (uint8_t)r;
    col[1] = (uint8_t)g;
    col[2] = (uint8_t)b;
    if (p.out_index) p.out_index[pos] = p.index_base + i;
  });
}

// ---------------------------------------------------------------------------------------------------------------------------------
// voxel-grid decimation: one point per occupied cell of a grid of edge *voxel anchored at the minimum of the finite points; the
// winner of a cell is the largest conf (NaN lowest), ties to the smallest index; the winners leave in input order.
// Open-addressing table of (key, best) pairs: the 63-bit cell key claims a slot by a 64-bit compare-and-swap, then one 64-bit max of
// (conf order key << 32) | ~index picks the winner. Max and min do not depend on arrival order: two runs give the same bytes.
// ---------------------------------------------------------------------------------------------------------------------------------
constexpr uint64_t kVgEmpty = ~0ull;                // no cell key has bit 63
constexpr float kVgMaxCell = 2097151.0f;            // 2^21 - 1
constexpr int64_t kVgMinSlots = 1024;

struct VgHead { uint32_t origin[3]; uint32_t flags; };     // origin as order keys (integer min is exact and order-free)
struct VgSlot { uint64_t key, best; };                      // one 16-byte slot: the claim and the max touch the same line
struct VgWs { VgHead* head; VgSlot* table; int64_t nslots; PfWs pf; };

int64_t vg_slots(int64_t n) { return 2 * n < kVgMinSlots ? kVgMinSlots : 2 * n; }      // load factor <= 1/2
int64_t vg_ws_bytes(int64_t n) { return 256 + round256(vg_slots(n) * (int64_t)sizeof(VgSlot)) + pf_ws_bytes(n); }
VgWs vg_ws(const ovg_voxel_downsample_params* p) {
  uint8_t* b = static_cast<uint8_t*>(p->ws);
  const int64_t ns = vg_slots(p->n), nb = pf_blocks(p->n);
  uint8_t* k = b + 256 + round256(ns * (int64_t)sizeof(VgSlot));
  return {reinterpret_cast<VgHead*>(b), reinterpret_cast<VgSlot*>(b + 256), ns,
          {k, reinterpret_cast<int64_t*>(k + round256(p->n)), reinterpret_cast<int64_t*>(k + round256(p->n) + round256(nb * 8))}};
}

__global__ __launch_bounds__(kThreads) void vg_init(VgWs ws, int64_t n) {
  const int64_t t0 = (int64_t)blockIdx.x * kThreads + threadIdx.x, step = (int64_t)gridDim.x * kThreads;
  u32x4* tab = reinterpret_cast<u32x4*>(ws.table);
  const u32x4 empty = {0xFFFFFFFFu, 0xFFFFFFFFu, 0u, 0u};
  for (int64_t i = t0; i < ws.nslots; i += step) tab[i] = empty;
  u32x4* keep = reinterpret_cast<u32x4*>(ws.pf.keep);            // the keep bytes are rounded up to 256: whole 16-byte stores
  const u32x4 zero = {0u, 0u, 0u, 0u};
  for (int64_t i = t0; i < (n + 15) / 16; i += step) keep[i] = zero;
  if (t0 == 0) *ws.head = {{0xFFFFFFFFu, 0xFFFFFFFFu, 0xFFFFFFFFu}, 0u};
}

__global__ __launch_bounds__(kThreads) void vg_origin(ovg_voxel_downsample_params p, VgWs ws) {
  __shared__ uint32_t red[3][kThreads / 64];
  uint32_t m[3] = {0xFFFFFFFFu, 0xFFFFFFFFu, 0xFFFFFFFFu};
  for (int64_t i = (int64_t)blockIdx.x * kThreads + threadIdx.x; i < p.n; i += (int64_t)gridDim.x * kThreads) {
    const float x = p.points[3 * i], y = p.points[3 * i + 1], z = p.points[3 * i + 2];
    if (finite3(x, y, z)) {
      m[0] = min(m[0], order_key(x));
      m[1] = min(m[1], order_key(y));
      m[2] = min(m[2], order_key(z));
    }
  }
#pragma unroll
  for (int k = 0; k < 3; ++k) {
    m[k] = wave_reduce(m[k], IntMin());
    if ((threadIdx.x & 63) == 0) red[k][threadIdx.x >> 6] = m[k];
  }
  __syncthreads();
  if (threadIdx.x < 3) {
    uint32_t v = red[threadIdx.x][0];
    for (int w = 1; w < kThreads / 64; ++w) v = min(v, red[threadIdx.x][w]);
    if (v != 0xFFFFFFFFu) __hip_atomic_fetch_min(&ws.head->origin[threadIdx.x], v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  }
}

__global__ __launch_bounds__(kThreads) void vg_insert(ovg_voxel_downsample_params p, VgWs ws) {
  const int64_t i = (int64_t)blockIdx.x * kThreads + threadIdx.x;
  if (i >= p.n) return;
  const float v = *p.voxel;
  if (!(v > 0.0f) || !finite_f32(v)) {
    if (i == 0) __hip_atomic_fetch_or(&ws.head->flags, (uint32_t)OVG_VG_BAD_VOXEL, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    return;
  }
  const float x = p.points[3 * i], y = p.points[3 * i + 1], z = p.points[3 * i + 2];
  if (!finite3(x, y, z)) return;
  // np.floor((p - origin) / v) in float32: one subtraction, one correctly rounded division, a floor (p >= origin, so c >= 0)
  const float cx = floorf(__fdiv_rn(__fsub_rn(x, key_value(ws.head->origin[0])), v));
  const float cy = floorf(__fdiv_rn(__fsub_rn(y, key_value(ws.head->origin[1])), v));
  const float cz = floorf(__fdiv_rn(__fsub_rn(z, key_value(ws.head->origin[2])), v));
  const bool over = !(cx <= kVgMaxCell && cy <= kVgMaxCell && cz <= kVgMaxCell);       // also an extent that overflowed to inf
  if (over) {
    if (!(__hip_atomic_load(&ws.head->flags, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) & OVG_VG_OVERFLOW))
      __hip_atomic_fetch_or(&ws.head->flags, (uint32_t)OVG_VG_OVERFLOW, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    return;
  }
  const uint64_t key = ((uint64_t)(uint32_t)cx << 42) | ((uint64_t)(uint32_t)cy << 21) | (uint64_t)(uint32_t)cz;
  uint32_t ck = 0;                                    // NaN conf is the lowest value; -0 counts as +0, as numpy compares them
  if (p.conf) {
    const float c = p.conf[i];
    if (c == c) ck = order_key(c + 0.0f);
  }
  const uint64_t word = ((uint64_t)ck << 32) | (uint32_t)~(uint32_t)i;                  // larger conf first, then the smaller index
  int64_t s = (int64_t)__umul64hi(mix_murmur64(key), (uint64_t)ws.nslots);
  for (int64_t t = 0; t < ws.nslots; ++t) {          // at most n of the >= 2n slots are ever claimed: the walk ends at a free one
    VgSlot* slot = ws.table + s;
    uint64_t k = __hip_atomic_load(&slot->key, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    if (k == kVgEmpty) {
      uint64_t expect = kVgEmpty;
      k = __hip_atomic_compare_exchange_strong(&slot->key, &expect, key, __ATOMIC_RELAXED, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) ? key : expect;
    }
    if (k == key) {
      // best only grows: a point that already loses to what is visible needs no atomic (most points, once a cell holds many)
      if (__hip_atomic_load(&slot->best, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) < word)
        __hip_atomic_fetch_max(&slot->best, word, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      return;
    }
    s = s + 1 == ws.nslots ? 0 : s + 1;
  }
}

// every claimed slot names its cell's winner; nothing is kept from a call that raised a flag
__global__ __launch_bounds__(kThreads) void vg_mark(VgWs ws, int64_t n) {
  if (ws.head->flags) return;
  for (int64_t s = (int64_t)blockIdx.x * kThreads + threadIdx.x; s < ws.nslots; s += (int64_t)gridDim.x * kThreads) {
    const u32x4 e = reinterpret_cast<const u32x4*>(ws.table)[s];
    if ((e[0] & e[1]) == 0xFFFFFFFFu) continue;
    const int64_t i = (int64_t)(uint32_t)~e[2];
    if (i < n) ws.pf.keep[i] = 1;
  }
}

__global__ __launch_bounds__(kThreads) void vg_count(VgWs ws, int64_t n, int64_t* out_count) {
  __shared__ int64_t red[kThreads / 64];
  const int64_t base = (int64_t)blockIdx.x * kTile;
  int64_t cnt = 0;
#pragma unroll 4
  for (int j = 0; j < kTile / kThreads; ++j) {
    const int64_t i = base + (int64_t)j * kThreads + threadIdx.x;
    if (i < n) cnt += ws.pf.keep[i];
  }
  const int64_t t = block_reduce<kThreads>(cnt, red, IntSum());
  if (threadIdx.x == 0) {
    ws.pf.counts[blockIdx.x] = t;
    if (blockIdx.x == 0) out_count[1] = (int64_t)ws.head->flags;
  }
}

__global__ __launch_bounds__(kThreads) void vg_scatter(ovg_voxel_downsample_params p, VgWs ws) {
  scatter_tile(ws.pf.keep, p.n, ws.pf.offsets, p.capacity, [&](int64_t i, int64_t pos) {
    const float* src = p.points + i * 3;
    float* dst = p.out_points + pos * 3;
    dst[0] = src[0];
    dst[1] = src[1];
    dst[2] = src[2];
    if (p.colors) {
      const uint8_t* cs = p.colors + i * 3;
      uint8_t* col = p.out_colors + pos * 3;
      col[0] = cs[0];
      col[1] = cs[1];
      col[2] = cs[2];
    }
    if (p.out_index) p.out_index[pos] = i;
  });
}

unsigned grid_for(int64_t work, int64_t per_block, int64_t cap) {
  const int64_t b = (work + per_block - 1) / per_block;
  return (unsigned)(b < 1 ? 1 : (b > cap ? cap : b));
}

// numpy 2 linear-method index rule in f32 (tests/pointcloud_twin.py restates it): q = p / 100, vi = f32(n - 1) * q; vi >= f32(n - 1)
// takes the maximum with gamma = f32(vi + 1) (numpy's index -1); otherwise lo = floor(vi), hi = f32(lo + 1) clamped to n - 1,
// gamma = f32(vi - lo).
void index_rule(int64_t n, float pct, int64_t& lo, int64_t& hi, float& gamma) {
  const float q = pct / 100.0f;
  const float nm1 = (float)(n - 1);
  const float vi = nm1 * q;
  if (vi >= nm1) {
    lo = hi = n - 1;
    gamma = (float)((double)vi + 1.0);
    return;
  }
  const float flo = floorf(vi);
  lo = (int64_t)flo;
  hi = (int64_t)(flo + 1.0f);
  if (hi > n - 1) hi = n - 1;
  gamma = (float)((double)vi - (double)lo);
}

}  // namespace

extern "C" int64_t ovg_percentile_workspace_bytes(int64_t n, int32_t ncols) {
  if (n <= 0 || ncols < 1 || ncols > OVG_PCT_MAX_COLS) return -1;
  return pct_ws_bytes(ncols);
}

extern "C" int ovg_percentile(const ovg_percentile_params* p, void* stream) {
  if (!p || !p->x || !p->out || !p->ws || p->n <= 0 || p->stride < 1 || p->col_stride < 0) return OVG_E_ARG;
  if (p->ncols < 1 || p->ncols > OVG_PCT_MAX_COLS || p->nq < 1 || p->nq > OVG_PCT_MAX_Q) return OVG_E_ARG;
  if (p->norm_out && p->nq != 2) return OVG_E_ARG;
  if (!al(p->ws, 16) || p->ws_bytes < pct_ws_bytes(p->ncols)) return OVG_E_ARG;
  PctPlan plan{};
  plan.nq = p->nq;
  for (int j = 0; j < p->nq; ++j) {
    if (!(p->q[j] >= 0.0f && p->q[j] <= 100.0f)) return OVG_E_ARG;
    int64_t lo, hi;
    index_rule(p->n, p->q[j], lo, hi, plan.gamma[j]);
    plan.rank[2 * j] = lo;
    plan.rank[2 * j + 1] = hi;
  }
  hipStream_t st = static_cast<hipStream_t>(stream);
  uint64_t* hist = static_cast<uint64_t*>(p->ws);
  PctState* state = reinterpret_cast<PctState*>(static_cast<uint8_t*>(p->ws) + state_offset_bytes(p->ncols));
  const dim3 grid(grid_for(p->n, (int64_t)kThreads * kPerThread, 1024), p->ncols);
  OVG_LAUNCH(pct_init, dim3(grid_for((int64_t)p->ncols * kHistWords, kThreads, 256)), dim3(kThreads), 0, st, hist, state, p->ncols, plan);
  OVG_CHECK_LAUNCH();
  OVG_LAUNCH(pct_hist<1>, grid, dim3(kThreads), 0, st, *p, hist, state);
  OVG_CHECK_LAUNCH();
  OVG_LAUNCH(pct_pick<1>, dim3(1), dim3(kThreads), 0, st, *p, hist, state, plan);
  OVG_CHECK_LAUNCH();
  OVG_LAUNCH(pct_hist<2>, grid, dim3(kThreads), 0, st, *p, hist, state);
  OVG_CHECK_LAUNCH();
  OVG_LAUNCH(pct_pick<2>, dim3(1), dim3(kThreads), 0, st, *p, hist, state, plan);
  OVG_CHECK_LAUNCH();
  OVG_LAUNCH(pct_hist<3>, grid, dim3(kThreads), 0, st, *p, hist, state);
  OVG_CHECK_LAUNCH();
  OVG_LAUNCH(pct_pick<3>, dim3(1), dim3(kThreads), 0, st, *p, hist, state, plan);
  OVG_CHECK_LAUNCH();
  return OVG_OK;
}

extern "C" int64_t ovg_point_filter_workspace_bytes(int64_t n) { return n <= 0 ? -1 : pf_ws_bytes(n); }

extern "C" int ovg_point_filter(const ovg_point_filter_params* p, void* stream) {
  if (!p || !p->conf || !p->images || !p->points || !p->ws || p->n <= 0 || p->hw <= 0 || p->n % p->hw) return OVG_E_ARG;
  if (p->stage < 1 || p->stage > (OVG_PF_COUNT | OVG_PF_SCATTER) || (p->flags & ~(OVG_PF_BLACK_BG | OVG_PF_WHITE_BG))) return OVG_E_ARG;
  if ((p->stage & OVG_PF_COUNT) && !p->out_count) return OVG_E_ARG;
  if ((p->stage & OVG_PF_SCATTER) && (!p->out_points || !p->out_colors || p->capacity < 0)) return OVG_E_ARG;
  if (!al(p->ws, 16) || p->ws_bytes < pf_ws_bytes(p->n)) return OVG_E_ARG;
  hipStream_t st = static_cast<hipStream_t>(stream);
  const PfWs ws = pf_ws(p);
  const int64_t nblk = pf_blocks(p->n);
  if (nblk > 0x7FFFFFFF) return OVG_E_ARG;
  if (p->stage & OVG_PF_COUNT) {
    OVG_LAUNCH(pf_mask, dim3((unsigned)nblk), dim3(kThreads), 0, st, *p, ws);
    OVG_CHECK_LAUNCH();
    OVG_LAUNCH(pf_scan, dim3(1), dim3(1024), 0, st, ws, nblk, p->out_count);
    OVG_CHECK_LAUNCH();
  }
  if ((p->stage & OVG_PF_SCATTER) && p->capacity > 0) {
    OVG_LAUNCH(pf_scatter, dim3((unsigned)nblk), dim3(kThreads), 0, st, *p, ws);
    OVG_CHECK_LAUNCH();
  }
  return OVG_OK;
}

extern "C" int64_t ovg_voxel_downsample_workspace_bytes(int64_t n) { return n <= 0 || n >= (1ll << 32) ? -1 : vg_ws_bytes(n); }

extern "C" int ovg_voxel_downsample(const ovg_voxel_downsample_params* p, void* stream) {
  if (!p || !p->points || !p->voxel || !p->ws || p->n <= 0 || p->n >= (1ll << 32)) return OVG_E_ARG;
  if (p->stage < 1 || p->stage > (OVG_VG_COUNT | OVG_VG_SCATTER)) return OVG_E_ARG;
  if ((p->stage & OVG_VG_COUNT) && !p->out_count) return OVG_E_ARG;
  if ((p->stage & OVG_VG_SCATTER) && (!p->out_points || p->capacity < 0 || (p->colors != nullptr) != (p->out_colors != nullptr))) return OVG_E_ARG;
  if (!al(p->ws, 16) || p->ws_bytes < vg_ws_bytes(p->n)) return OVG_E_ARG;
  hipStream_t st = static_cast<hipStream_t>(stream);
  const VgWs ws = vg_ws(p);
  const int64_t nblk = pf_blocks(p->n);
  if (p->stage & OVG_VG_COUNT) {
    OVG_LAUNCH(vg_init, dim3(grid_for(ws.nslots, kThreads * 4, 4096)), dim3(kThreads), 0, st, ws, p->n);
    OVG_CHECK_LAUNCH();
    OVG_LAUNCH(vg_origin, dim3(grid_for(p->n, kThreads * 4, 2048)), dim3(kThreads), 0, st, *p, ws);
    OVG_CHECK_LAUNCH();
    OVG_LAUNCH(vg_insert, dim3((unsigned)((p->n + kThreads - 1) / kThreads)), dim3(kThreads), 0, st, *p, ws);
    OVG_CHECK_LAUNCH();
    OVG_LAUNCH(vg_mark, dim3(grid_for(ws.nslots, kThreads * 4, 4096)), dim3(kThreads), 0, st, ws, p->n);
    OVG_CHECK_LAUNCH();
    OVG_LAUNCH(vg_count, dim3((unsigned)nblk), dim3(kThreads), 0, st, ws, p->n, p->out_count);
    OVG_CHECK_LAUNCH();
    OVG_LAUNCH(pf_scan, dim3(1), dim3(1024), 0, st, ws.pf, nblk, p->out_count);
    OVG_CHECK_LAUNCH();
  }
  if ((p->stage & OVG_VG_SCATTER) && p->capacity > 0) {
    OVG_LAUNCH(vg_scatter, dim3((unsigned)nblk), dim3(kThreads), 0, st, *p, ws);
    OVG_CHECK_LAUNCH();
  }
  return OVG_OK;
}
