// Exact nearest-neighbour search between two point clouds (ovg_nearest_neighbours): for every query the reference point with the
// smallest squared distance, ties to the lowest reference index. Brute force on the vector ALU: a grid of (query tiles) x (reference
// splits); a workgroup keeps kQueriesPerThread queries per thread in registers, stages one reference tile after the other in LDS
// (groups of four points as x[4] y[4] z[4], so that a group is three 16-byte reads of an address all lanes share: a broadcast, no
// bank conflicts) and walks it in ascending index with a strict "smaller than". One split stores its result; several merge the packed
// (bits(d) << 32) | j with a 64-bit unsigned atomic min (as ovg_render.hip's z-buffer does) and a last launch decodes the keys.
#include "ovg_geom.h"

// tests/nn_twin.py restates the rule in numpy float32, one rounding per operation: no fused multiply-adds in this unit (build.py
// compiles it with -ffp-contract=off as well)
#pragma clang fp contract(off)

namespace {

constexpr int kThreads = 128;
constexpr int kQueriesPerThread = OVG_NN_QUERY_TILE / kThreads;
constexpr int kRefTile = OVG_NN_REFERENCE_TILE;
constexpr int kTargetWorkgroups = 2048;              // auto splits: 256 CUs x 4 SIMDs x 2 waves each, at 2 waves per workgroup
constexpr int kMaxSplits = 65535;                    // gridDim.y
constexpr uint32_t kInfBits = 0x7F800000u;
// "nothing found yet": above bits(+inf), so that a d of +inf still wins the unsigned compare, and at or below the bits of every NaN
// (positive NaNs are 0x7F800001 .. 0x7FFFFFFF, negative ones larger still as unsigned), so that a NaN never does
constexpr uint32_t kNoneBits = 0x7F800001u;
constexpr uint32_t kNanBits = 0x7FC00000u;
constexpr uint64_t kEmptyKey = ((uint64_t)kInfBits << 32) | 0xFFFFFFFFull;

static_assert(kQueriesPerThread * kThreads == OVG_NN_QUERY_TILE && kRefTile % kThreads == 0 && kRefTile % 4 == 0, "tile shapes");

bool nn_shape_ok(int64_t nq, int64_t nr) { return size_ok(nq) && size_ok(nr); }
int64_t nn_ws_bytes(int64_t nq) { return (nq * 8 + 15) / 16 * 16; }

__global__ __launch_bounds__(256) void nn_fill(uint64_t* __restrict__ keys, int32_t nq) {
  const uint32_t i = blockIdx.x * 256 + threadIdx.x;                       // nq < 2^31: no wrap in unsigned arithmetic
  if (i < (uint32_t)nq) keys[i] = kEmptyKey;
}

__global__ __launch_bounds__(256) void nn_decode(const uint64_t* __restrict__ keys, int32_t nq, int32_t* __restrict__ index,
                                                 float* __restrict__ sqdist) {
  const uint32_t i = blockIdx.x * 256 + threadIdx.x;
  if (i >= (uint32_t)nq) return;
  const uint64_t key = keys[i];
  index[i] = (int32_t)(uint32_t)key;                                      // 0xFFFFFFFF of the empty key is -1
  sqdist[i] = __uint_as_float((uint32_t)(key >> 32));
}

// one group of four references against the thread's queries. j0: index of the group's first reference (wave-uniform).
// kExclude: skip reference j == query index (only instantiated for tiles that overlap the workgroup's own queries)
template <bool kExclude>
OVG_DEV void nn_group(const f32x4 rx, const f32x4 ry, const f32x4 rz, int32_t j0, const float (&qx)[kQueriesPerThread],
                      const float (&qy)[kQueriesPerThread], const float (&qz)[kQueriesPerThread], const int32_t (&qi)[kQueriesPerThread],
                      uint32_t (&best)[kQueriesPerThread], int32_t (&arg)[kQueriesPerThread]) {
#pragma unroll
  for (int r = 0; r < 4; ++r) {
#pragma unroll
    for (int k = 0; k < kQueriesPerThread; ++k) {
      const float dx = qx[k] - rx[r], dy = qy[k] - ry[r], dz = qz[k] - rz[r];
      const float d = (dx * dx + dy * dy) + dz * dz;                       // +0, positive, +inf or NaN: the bits order like the value
      const uint32_t b = __float_as_uint(d);
      const bool take = b < best[k] && (!kExclude || qi[k] != j0 + r);
      best[k] = take ? b : best[k];
      arg[k] = take ? j0 + r : arg[k];
    }
  }
}

template <bool kExclude>
OVG_DEV void nn_tile(const float* lds, int32_t j0, const float (&qx)[kQueriesPerThread], const float (&qy)[kQueriesPerThread],
                     const float (&qz)[kQueriesPerThread], const int32_t (&qi)[kQueriesPerThread], uint32_t (&best)[kQueriesPerThread],
                     int32_t (&arg)[kQueriesPerThread]) {
  const f32x4* g = reinterpret_cast<const f32x4*>(lds);
#pragma unroll 2
  for (int t = 0; t < kRefTile / 4; ++t)
    nn_group<kExclude>(g[3 * t], g[3 * t + 1], g[3 * t + 2], j0 + 4 * t, qx, qy, qz, qi, best, arg);
}

// blockIdx.x: query tile, blockIdx.y: split (reference tiles [y * tiles_per_split, (y + 1) * tiles_per_split) below ntiles).
// kMerge: atomic min into keys (several splits); otherwise index / sqdist are stored directly.
template <bool kMerge>
__global__ __launch_bounds__(kThreads) void nn_search(const float* __restrict__ query, const float* __restrict__ reference,
                                                      const uint8_t* __restrict__ qvalid, const uint8_t* __restrict__ rvalid, int32_t nq,
                                                      int32_t nr, int32_t ntiles, int32_t tiles_per_split, int32_t exclude,
                                                      uint64_t* __restrict__ keys, int32_t* __restrict__ index,
                                                      float* __restrict__ sqdist) {
  __shared__ __attribute__((aligned(16))) float lds[3 * kRefTile];
  const int32_t q0 = (int32_t)blockIdx.x * OVG_NN_QUERY_TILE;              // < nq < 2^31
  float qx[kQueriesPerThread], qy[kQueriesPerThread], qz[kQueriesPerThread];
  int32_t qi[kQueriesPerThread], arg[kQueriesPerThread];
  uint32_t best[kQueriesPerThread];
#pragma unroll
  for (int k = 0; k < kQueriesPerThread; ++k) {
    // q0 + 2 * OVG_NN_QUERY_TILE may pass 2^31: compare the offset inside the tile, which is small
    const int32_t off = k * kThreads + (int32_t)threadIdx.x;
    const bool in = off < nq - q0;
    qi[k] = in ? q0 + off : -1;
    float x = 0.0f, y = 0.0f, z = 0.0f;
    bool usable = false;
    if (in) {
      const float* p = query + 3 * (int64_t)qi[k];
      x = p[0], y = p[1], z = p[2];
      usable = finite3(x, y, z) && (!qvalid || qvalid[qi[k]] != 0);
    }
    // an unusable query becomes NaN: every d is NaN and nothing is ever taken
    qx[k] = usable ? x : __uint_as_float(kNanBits);
    qy[k] = y, qz[k] = z;
    best[k] = kNoneBits, arg[k] = -1;
  }
  const int32_t t_first = (int32_t)blockIdx.y * tiles_per_split;
  const int32_t t_end = min(t_first + tiles_per_split, ntiles);
  for (int32_t t = t_first; t < t_end; ++t) {
    const int32_t j0 = t * kRefTile;                                       // < nr < 2^31
    __syncthreads();                                                       // the previous tile has been read by every wave
#pragma unroll
    for (int s = 0; s < kRefTile / kThreads; ++s) {
      const int32_t jl = s * kThreads + (int32_t)threadIdx.x;              // position in the tile
      float x = __uint_as_float(kNanBits), y = 0.0f, z = 0.0f;             // padding and unusable references: NaN
      if (jl < nr - j0) {
        const int64_t j = (int64_t)j0 + jl;
        const float* p = reference + 3 * j;
        const float px = p[0], py = p[1], pz = p[2];
        if (finite3(px, py, pz) && (!rvalid || rvalid[j] != 0)) x = px, y = py, z = pz;
      }
      float* g = lds + 12 * (jl >> 2) + (jl & 3);
      g[0] = x, g[4] = y, g[8] = z;
    }
    __syncthreads();
    // wave-uniform: does [j0, j0 + kRefTile) meet the workgroup's queries [q0, q0 + OVG_NN_QUERY_TILE)? (int64: no overflow)
    if (exclude && (int64_t)j0 < (int64_t)q0 + OVG_NN_QUERY_TILE && (int64_t)q0 < (int64_t)j0 + kRefTile)
      nn_tile<true>(lds, j0, qx, qy, qz, qi, best, arg);
    else
      nn_tile<false>(lds, j0, qx, qy, qz, qi, best, arg);
  }
#pragma unroll
  for (int k = 0; k < kQueriesPerThread; ++k) {
    if (qi[k] < 0) continue;
    const bool found = best[k] != kNoneBits;
    if (kMerge) {
      // the keys start as kEmptyKey (nn_fill); (bits(d), j) orders first by distance, then by index: ties go to the lowest index
      // whatever the order in which the splits arrive
      if (found) __hip_atomic_fetch_min(keys + qi[k], ((uint64_t)best[k] << 32) | (uint32_t)arg[k], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    } else {
      index[qi[k]] = found ? arg[k] : -1;
      sqdist[qi[k]] = __uint_as_float(found ? best[k] : kInfBits);
    }
  }
}

}  // namespace

extern "C" int64_t ovg_nn_workspace_bytes(int64_t nq, int64_t nr) { return nn_shape_ok(nq, nr) ? nn_ws_bytes(nq) : -1; }

extern "C" int ovg_nearest_neighbours(const ovg_nn_params* p, void* stream) {
  if (!p || !p->query || !p->reference || !p->ws || !p->index || !p->sqdist) return OVG_E_ARG;
  if (!nn_shape_ok(p->nq, p->nr) || (p->flags & ~OVG_NN_EXCLUDE_SAME_INDEX) || p->splits < 0) return OVG_E_ARG;
  if ((p->flags & OVG_NN_EXCLUDE_SAME_INDEX) && p->nq != p->nr) return OVG_E_ARG;
  if (!al(p->query, 4) || !al(p->reference, 4) || !al(p->index, 4) || !al(p->sqdist, 4)) return OVG_E_ARG;
  if (!al(p->ws, 16) || p->ws_bytes < nn_ws_bytes(p->nq)) return OVG_E_ARG;
  hipStream_t st = static_cast<hipStream_t>(stream);
  const int32_t nq = (int32_t)p->nq, nr = (int32_t)p->nr;
  const int32_t qtiles = (int32_t)((p->nq + OVG_NN_QUERY_TILE - 1) / OVG_NN_QUERY_TILE);   // <= 2^22: fits gridDim.x
  const int32_t ntiles = (int32_t)((p->nr + kRefTile - 1) / kRefTile);
  int32_t splits = p->splits > 0 ? p->splits : (kTargetWorkgroups + qtiles - 1) / qtiles;
  splits = splits < ntiles ? splits : ntiles;
  splits = splits < kMaxSplits ? splits : kMaxSplits;
  const int32_t per = (ntiles + splits - 1) / splits;
  splits = (ntiles + per - 1) / per;                                        // no empty split
  const int32_t exclude = (p->flags & OVG_NN_EXCLUDE_SAME_INDEX) ? 1 : 0;
  uint64_t* keys = static_cast<uint64_t*>(p->ws);
  const dim3 grid((unsigned)qtiles, (unsigned)splits), flat((unsigned)((p->nq + 255) / 256));
  if (splits == 1) {
    OVG_LAUNCH(nn_search<false>, grid, dim3(kThreads), 0, st, p->query, p->reference, p->query_valid, p->reference_valid, nq, nr, ntiles, per,
               exclude, keys, p->index, p->sqdist);
    OVG_CHECK_LAUNCH();
    return OVG_OK;
  }
  OVG_LAUNCH(nn_fill, flat, dim3(256), 0, st, keys, nq);
  OVG_CHECK_LAUNCH();
  OVG_LAUNCH(nn_search<true>, grid, dim3(kThreads), 0, st, p->query, p->reference, p->query_valid, p->reference_valid, nq, nr, ntiles, per,
             exclude, keys, p->index, p->sqdist);
  OVG_CHECK_LAUNCH();
  OVG_LAUNCH(nn_decode, flat, dim3(256), 0, st, keys, nq, p->index, p->sqdist);
  OVG_CHECK_LAUNCH();
  return OVG_OK;
}
