// Depth evaluation (ovg_deptheval_median, ovg_deptheval_sums, ovg_deptheval_solve): the masked medians of every group of pixels by a
// radix select over the four bytes of the float's bit pattern (integer histograms: no sort, no compaction, nothing read back), the
// float64 moment / metric sums of a group in the FIXED order of ovg_align_moments, and the alignment coefficients from either.
// include/omnivggt_hip.h states the rule, tests/deptheval_twin.py restates it in numpy. Both hot kernels stream 8 (+ 1 mask) bytes per
// pixel and are bound by memory; a select costs four such passes.
#include "ovg_geom.h"

// the twin is one numpy float64 operation per rounding: no fused multiply-adds in this unit (build.py: -ffp-contract=off)
#pragma clang fp contract(off)

namespace {

constexpr int kThreads = OVG_DEPTHEVAL_THREADS;
constexpr int kTile = OVG_DEPTHEVAL_TILE;
constexpr int kRounds = kTile / kThreads;
constexpr int kSums = OVG_DEPTHEVAL_SUMS;
constexpr int kCounts = OVG_DEPTHEVAL_COUNTS;
constexpr int kSlots = OVG_DEPTHEVAL_PARTIAL_BYTES / 8;   // a tile's partial: the 4 int64 counts, the 5 sums, one slot of padding
constexpr int kChunk = OVG_DEPTHEVAL_CHUNK;
constexpr int kChunkRounds = kChunk / kThreads;
constexpr int kSel = 4;                                   // selections of a group: 2 m + r, map m (0 pred, 1 gt), rank r (0 lower, 1 upper middle)
constexpr int kBins = 256;
constexpr int kGroupWords = OVG_DEPTHEVAL_MEDIAN_GROUP_BYTES / 4;
static_assert(kRounds >= 1 && kSlots >= kSums + kCounts, "a tile has pixels and its partial has room");
static_assert(kGroupWords == kSel * kBins + 2 * kSel && kChunk % kThreads == 0 && kThreads == kBins, "one thread per bin in the scan");

// THE predicate of all three entries: is pixel i (an element offset into pred / gt / valid) used? Positive and finite is tested on
// the bit pattern, so a subnormal pred counts whatever the denormal mode of the comparison would make of it.
OVG_DEV bool used_pixel(const float* pred, const float* gt, const uint8_t* valid, int64_t i, float min_depth, float max_depth, float& p, float& g) {
  if (valid && valid[i] == 0) return false;
  p = pred[i], g = gt[i];
  const uint32_t pb = __builtin_bit_cast(uint32_t, p);
  return pb - 1u < 0x7f7fffffu && finite_f32(g) && g > min_depth && g <= max_depth;
}

// ---------------------------------------------------------------------------------------------------------------------------------
// median: radix select
// ---------------------------------------------------------------------------------------------------------------------------------
// ws of group g, kGroupWords u32: hist[kSel][kBins], prefix[kSel] (the key bytes found so far, in place), rank[kSel] (the rank that
// is left inside the keys that carry the prefix)
__global__ __launch_bounds__(kThreads) void median_zero(uint32_t* ws, int64_t words) {
  const int64_t i = (int64_t)blockIdx.x * kThreads + threadIdx.x;
  if (i < words) ws[i] = 0u;
}

// one more key of `bin` in the LDS histogram h, for every lane with `pending`. Depth maps put most keys of a wave into two or three
// bins of the leading bytes: a few rounds of "the lowest pending lane's bin takes all its lanes at once" spare the same-address
// serialisation, whoever is left after them adds alone. All 64 lanes of the wave call it together; the loop is bounded.
OVG_DEV void hist_add(uint32_t* h, uint32_t bin, bool pending) {
  const int lane = threadIdx.x & 63;
#pragma unroll
  for (int it = 0; it < 3; ++it) {
    const unsigned long long act = __ballot(pending);
    if (act == 0ull) return;
    const int leader = __ffsll((long long)act) - 1;
    const uint32_t lb = (uint32_t)__shfl((int)bin, leader, 64);
    const bool mine = pending && bin == lb;
    const unsigned long long m = __ballot(mine);
    if (lane == leader) atomicAdd(&h[lb], (uint32_t)__popcll(m));
    pending = pending && !mine;
  }
  if (pending) atomicAdd(&h[bin], 1u);
}

// pass `level` (0 .. 3): byte 3 - level of the keys that agree with the prefix above it. While the two ranks of a map still share
// their prefix they share ONE histogram, the lower rank's (the scan below reads it for both).
__global__ __launch_bounds__(kThreads) void median_hist(ovg_deptheval_median_params p, int level) {
  __shared__ uint32_t h[kSel * kBins];
  const int64_t grp = blockIdx.y;
  uint32_t* gws = static_cast<uint32_t*>(p.ws) + grp * kGroupWords;
  for (int i = threadIdx.x; i < kSel * kBins; i += kThreads) h[i] = 0u;
  uint32_t prefix[kSel];
#pragma unroll
  for (int s = 0; s < kSel; ++s) prefix[s] = gws[kSel * kBins + s];
  __syncthreads();
  const int shift = 24 - 8 * level;
  const uint32_t himask = level == 0 ? 0u : 0xffffffffu << (shift + 8);            // the bytes above this pass's
  const bool split_p = prefix[0] != prefix[1], split_g = prefix[2] != prefix[3];
  const int64_t row = grp * p.stride;
  const int64_t first = (int64_t)blockIdx.x * kChunk + threadIdx.x;
  for (int r = 0; r < kChunkRounds; ++r) {
    const int64_t i = first + (int64_t)r * kThreads;
    if ((int64_t)blockIdx.x * kChunk + (int64_t)r * kThreads >= p.n) break;        // the same for the whole workgroup
    float pv = 0.0f, gv = 0.0f;
    const bool use = i < p.n && used_pixel(p.pred, p.gt, p.valid, row + i, p.min_depth, p.max_depth, pv, gv);
    const uint32_t kp = __builtin_bit_cast(uint32_t, pv), kg = __builtin_bit_cast(uint32_t, gv);
    const uint32_t bp = (kp >> shift) & 255u, bg = (kg >> shift) & 255u;
    hist_add(h, bp, use && (kp & himask) == prefix[0]);
    if (split_p) hist_add(h + kBins, bp, use && (kp & himask) == prefix[1]);
    hist_add(h + 2 * kBins, bg, use && (kg & himask) == prefix[2]);
    if (split_g) hist_add(h + 3 * kBins, bg, use && (kg & himask) == prefix[3]);
  }
  __syncthreads();
  for (int i = threadIdx.x; i < kSel * kBins; i += kThreads) {
    const uint32_t c = h[i];
    if (c) atomicAdd(&gws[i], c);
  }
}

// one workgroup per group: thread s < 4 walks the 256 bins of its selection to the bin that holds its rank, then all threads zero the
// bins for the next pass. Level 0 also derives N and the two ranks; level 3 writes the results.
__global__ __launch_bounds__(kThreads) void median_scan(ovg_deptheval_median_params p, int level) {
  __shared__ uint32_t h[kSel * kBins];
  __shared__ uint32_t state[2 * kSel];
  const int64_t grp = blockIdx.x;
  uint32_t* gws = static_cast<uint32_t*>(p.ws) + grp * kGroupWords;
  for (int i = threadIdx.x; i < kSel * kBins; i += kThreads) h[i] = gws[i];
  if (threadIdx.x < 2 * kSel) state[threadIdx.x] = gws[kSel * kBins + threadIdx.x];
  __syncthreads();
  if (threadIdx.x < kSel) {
    const int s = threadIdx.x, m = s >> 1;
    const int src = state[2 * m] != state[2 * m + 1] ? s : 2 * m;                  // shared prefix: the lower rank's histogram
    const uint32_t* hs = h + src * kBins;
    uint32_t rank = state[kSel + s];
    if (level == 0) {
      uint32_t total = 0u;
      for (int b = 0; b < kBins; ++b) total += hs[b];
      rank = (s & 1) ? total / 2u : (total > 0u ? (total - 1u) / 2u : 0u);
      if (s == 0) p.out_count[grp] = (int64_t)total;
    }
    uint32_t cum = 0u, bin = 0u, left = 0u;
    bool found = false;
    for (int b = 0; b < kBins; ++b) {
      const uint32_t c = hs[b];
      if (!found && rank - cum < c) bin = (uint32_t)b, left = rank - cum, found = true;   // cum <= rank until found
      if (!found) cum += c;
    }
    const uint32_t prefix = state[s] | (bin << (24 - 8 * level));                  // no used pixel: every bin empty, the key stays 0 = +0.0
    gws[kSel * kBins + s] = prefix;
    gws[kSel * kBins + kSel + s] = left;
    if (level == 3) p.out_median[grp * kSel + s] = __builtin_bit_cast(float, prefix);
  }
  for (int i = threadIdx.x; i < kSel * kBins; i += kThreads) gws[i] = 0u;
}

// ---------------------------------------------------------------------------------------------------------------------------------
// sums
// ---------------------------------------------------------------------------------------------------------------------------------
template <int MODE> __global__ __launch_bounds__(kThreads) void sums_tiles(ovg_deptheval_sums_params p, int64_t tiles) {
  const int64_t grp = blockIdx.y;
  const int64_t row = grp * p.stride;
  const int64_t base = (int64_t)blockIdx.x * kTile + threadIdx.x;
  double s = 1.0, t = 0.0;
  if (MODE == OVG_DEPTHEVAL_METRICS) s = p.coeff[2 * grp], t = p.coeff[2 * grp + 1];
  double v[kSums];
#pragma unroll
  for (int k = 0; k < kSums; ++k) v[k] = 0.0;
  long long cnt[kCounts] = {0, 0, 0, 0};
#pragma unroll
  for (int r = 0; r < kRounds; ++r) {
    const int64_t i = base + (int64_t)r * kThreads;
    if (i >= p.n) continue;
    float pf, gf;
    if (!used_pixel(p.pred, p.gt, p.valid, row + i, p.min_depth, p.max_depth, pf, gf)) continue;
    const double pd = (double)pf, g = (double)gf;
    if (MODE == OVG_DEPTHEVAL_MOMENTS) {
      v[0] = v[0] + pd, v[1] = v[1] + g, v[2] = v[2] + pd * pd, v[3] = v[3] + pd * g, v[4] = v[4] + g * g;
    } else {
      double q = s * pd + t;
      q = q > p.clip_min ? q : p.clip_min;
      q = q < p.clip_max ? q : p.clip_max;
      const double e = q - g, ae = fabs(e), ee = e * e;
      const double d = log(q) - log(g);
      v[0] = v[0] + ae / g, v[1] = v[1] + ee / g, v[2] = v[2] + ee, v[3] = v[3] + ae, v[4] = v[4] + d * d;
      const double r1 = q / g, r2 = g / q;
      const double ratio = r1 > r2 ? r1 : r2;
      cnt[1] += ratio < 1.25, cnt[2] += ratio < 1.5625, cnt[3] += ratio < 1.953125;
    }
    ++cnt[0];
  }
  double* slot = static_cast<double*>(p.ws) + (grp * tiles + blockIdx.x) * kSlots;
  fold_block<kThreads>(v, cnt, reinterpret_cast<int64_t*>(slot), slot + kCounts);
}

// step 4: one workgroup per group over its tile partials, thread t the tiles t, t + 256, ... in that order
__global__ __launch_bounds__(kThreads) void sums_fold(const double* ws, int64_t tiles, int64_t* out_counts, double* out_sums) {
  const int64_t grp = blockIdx.x;
  double v[kSums];
#pragma unroll
  for (int k = 0; k < kSums; ++k) v[k] = 0.0;
  long long cnt[kCounts] = {0, 0, 0, 0};
  for (int64_t k = threadIdx.x; k < tiles; k += kThreads) {
    const double* slot = ws + (grp * tiles + k) * kSlots;
#pragma unroll
    for (int c = 0; c < kCounts; ++c) cnt[c] += reinterpret_cast<const long long*>(slot)[c];
#pragma unroll
    for (int c = 0; c < kSums; ++c) v[c] = v[c] + slot[kCounts + c];
  }
  fold_block<kThreads>(v, cnt, out_counts + grp * kCounts, out_sums + grp * kSums);
}

// ---------------------------------------------------------------------------------------------------------------------------------
// solve
// ---------------------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(64) void deptheval_solve(ovg_deptheval_solve_params p) {
  const int64_t grp = (int64_t)blockIdx.x * 64 + threadIdx.x;
  if (grp >= p.groups) return;
  const int64_t n = p.count[grp * p.count_stride];
  const int mode = p.mode;
  int32_t status = 0;
  if (n < (mode == OVG_DEPTHEVAL_SCALE_SHIFT ? 2 : 1)) status |= OVG_DEPTHEVAL_FEW;
  double m[kSums] = {0.0, 0.0, 0.0, 0.0, 0.0}, med[4] = {0.0, 0.0, 0.0, 0.0};
  bool finite = true;
  if (mode == OVG_DEPTHEVAL_SCALE || mode == OVG_DEPTHEVAL_SCALE_SHIFT) {
    for (int k = 0; k < kSums; ++k) m[k] = p.sums[grp * kSums + k], finite = finite && finite_f64(m[k]);
  } else if (mode == OVG_DEPTHEVAL_MEDIAN) {
    for (int k = 0; k < 4; ++k) med[k] = (double)p.median[grp * 4 + k], finite = finite && finite_f64(med[k]);
  }
  if (!finite) status |= OVG_DEPTHEVAL_NOT_FINITE;
  double s = 1.0, t = 0.0;
  if (status == 0 && mode != OVG_DEPTHEVAL_NONE) {
    const double dn = (double)n;
    if (mode == OVG_DEPTHEVAL_MEDIAN) {
      const double mp = 0.5 * (med[0] + med[1]), mg = 0.5 * (med[2] + med[3]);
      s = mg / mp;
    } else if (mode == OVG_DEPTHEVAL_SCALE) {
      s = m[3] / m[2];
    } else {
      const double nspp = dn * m[2];
      const double det = nspp - m[0] * m[0];
      if (!(det > OVG_DEPTHEVAL_SPREAD_EPS * nspp)) {
        status |= OVG_DEPTHEVAL_NO_SPREAD;
      } else {
        s = (dn * m[3] - m[0] * m[1]) / det;
        t = (m[1] - s * m[0]) / dn;
      }
    }
    if (status == 0 && !(finite_f64(s) && finite_f64(t) && s > 0.0)) status |= OVG_DEPTHEVAL_BAD_FIT;
  }
  if (status != 0) s = 1.0, t = 0.0;
  p.coeff[2 * grp] = s, p.coeff[2 * grp + 1] = t;
  p.status[grp] = status;
}

bool sizes_ok(int64_t groups, int64_t n) {
  return groups >= 1 && groups <= OVG_DEPTHEVAL_MAX_GROUPS && n >= 1 && n < (1ll << 31) && groups * n < (1ll << 31);
}
bool layout_ok(int64_t groups, int64_t n, int64_t stride, float min_depth, float max_depth) {
  if (!sizes_ok(groups, n) || stride < n || stride >= (1ll << 40) / groups) return false;
  return min_depth >= 0.0f && max_depth == max_depth;                               // a NaN min_depth fails the comparison
}
int64_t tiles_of(int64_t n) { return (n + kTile - 1) / kTile; }

}  // namespace

extern "C" int64_t ovg_deptheval_median_workspace_bytes(int64_t groups, int64_t n) {
  if (!sizes_ok(groups, n)) return -1;
  return round256(groups * OVG_DEPTHEVAL_MEDIAN_GROUP_BYTES);
}

extern "C" int64_t ovg_deptheval_sums_workspace_bytes(int64_t groups, int64_t n) {
  if (!sizes_ok(groups, n)) return -1;
  return round256(groups * tiles_of(n) * OVG_DEPTHEVAL_PARTIAL_BYTES);
}

extern "C" int ovg_deptheval_median(const ovg_deptheval_median_params* p, void* stream) {
  if (!p || !p->pred || !p->gt || !p->ws || !p->out_count || !p->out_median) return OVG_E_ARG;
  if (!layout_ok(p->groups, p->n, p->stride, p->min_depth, p->max_depth)) return OVG_E_ARG;
  if (!al(p->pred, 4) || !al(p->gt, 4) || !al(p->out_count, 8) || !al(p->out_median, 4) || !al(p->ws, 16)) return OVG_E_ARG;
  if (p->ws_bytes < ovg_deptheval_median_workspace_bytes(p->groups, p->n)) return OVG_E_ARG;
  hipStream_t st = static_cast<hipStream_t>(stream);
  const int64_t words = p->groups * kGroupWords;
  const dim3 grid((unsigned)((p->n + kChunk - 1) / kChunk), (unsigned)p->groups);
  OVG_LAUNCH(median_zero, dim3((unsigned)((words + kThreads - 1) / kThreads)), dim3(kThreads), 0, st, static_cast<uint32_t*>(p->ws), words);
  OVG_CHECK_LAUNCH();
  for (int level = 0; level < 4; ++level) {
    OVG_LAUNCH(median_hist, grid, dim3(kThreads), 0, st, *p, level);
    OVG_CHECK_LAUNCH();
    OVG_LAUNCH(median_scan, dim3((unsigned)p->groups), dim3(kThreads), 0, st, *p, level);
    OVG_CHECK_LAUNCH();
  }
  return OVG_OK;
}

extern "C" int ovg_deptheval_sums(const ovg_deptheval_sums_params* p, void* stream) {
  if (!p || !p->pred || !p->gt || !p->ws || !p->out_counts || !p->out_sums) return OVG_E_ARG;
  if (!layout_ok(p->groups, p->n, p->stride, p->min_depth, p->max_depth)) return OVG_E_ARG;
  if (p->mode != OVG_DEPTHEVAL_MOMENTS && p->mode != OVG_DEPTHEVAL_METRICS) return OVG_E_ARG;
  if (p->mode == OVG_DEPTHEVAL_METRICS) {
    if (!p->coeff || !(p->clip_min > 0.0) || !(p->clip_min <= 1.7976931348623157e308) || !(p->clip_max >= p->clip_min)) return OVG_E_ARG;
  }
  if (!al(p->pred, 4) || !al(p->gt, 4) || !al(p->coeff, 8) || !al(p->out_counts, 8) || !al(p->out_sums, 8) || !al(p->ws, 16)) return OVG_E_ARG;
  if (p->ws_bytes < ovg_deptheval_sums_workspace_bytes(p->groups, p->n)) return OVG_E_ARG;
  hipStream_t st = static_cast<hipStream_t>(stream);
  const int64_t tiles = tiles_of(p->n);
  const dim3 grid((unsigned)tiles, (unsigned)p->groups);
  if (p->mode == OVG_DEPTHEVAL_MOMENTS) OVG_LAUNCH(sums_tiles<OVG_DEPTHEVAL_MOMENTS>, grid, dim3(kThreads), 0, st, *p, tiles);
  else OVG_LAUNCH(sums_tiles<OVG_DEPTHEVAL_METRICS>, grid, dim3(kThreads), 0, st, *p, tiles);
  OVG_CHECK_LAUNCH();
  OVG_LAUNCH(sums_fold, dim3((unsigned)p->groups), dim3(kThreads), 0, st, static_cast<const double*>(p->ws), tiles, p->out_counts, p->out_sums);
  OVG_CHECK_LAUNCH();
  return OVG_OK;
}

extern "C" int ovg_deptheval_solve(const ovg_deptheval_solve_params* p, void* stream) {
  if (!p || !p->count || !p->coeff || !p->status) return OVG_E_ARG;
  if (p->groups < 1 || p->groups > OVG_DEPTHEVAL_MAX_GROUPS || p->count_stride < 1 || p->count_stride > (1 << 20)) return OVG_E_ARG;
  if (p->mode < OVG_DEPTHEVAL_NONE || p->mode > OVG_DEPTHEVAL_SCALE_SHIFT) return OVG_E_ARG;
  if ((p->mode == OVG_DEPTHEVAL_SCALE || p->mode == OVG_DEPTHEVAL_SCALE_SHIFT) && !p->sums) return OVG_E_ARG;
  if (p->mode == OVG_DEPTHEVAL_MEDIAN && !p->median) return OVG_E_ARG;
  if (!al(p->count, 8) || !al(p->sums, 8) || !al(p->median, 4) || !al(p->coeff, 8) || !al(p->status, 4)) return OVG_E_ARG;
  hipStream_t st = static_cast<hipStream_t>(stream);
  OVG_LAUNCH(deptheval_solve, dim3((unsigned)((p->groups + 63) / 64)), dim3(64), 0, st, *p);
  OVG_CHECK_LAUNCH();
  return OVG_OK;
}
