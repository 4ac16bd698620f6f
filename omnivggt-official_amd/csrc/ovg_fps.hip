// Farthest-point sampling of point clouds (ovg_farthest_point_sample): npoint dependent steps, each takes the usable point with the
// largest squared distance to the samples so far (ties to the lowest index) and lowers every point's distance by the new sample.
// The rule (include/omnivggt_hip.h, tests/fps_twin.py):
//   usable   all three coordinates finite and the valid byte (if given) non-zero
//   state    mind[j] = 1e10f for every j (squared distances saturate there; such points tie and go in index order)
//   centre   step 0: first; step 1 with OVG_FPS_INCLUDE_LAST: n - 1 (forced, usable or not); otherwise the usable j that maximises
//            bits(mind[j]), lowest j on ties; -1 when no point is usable
//   outputs  index[i] = c, sqdist[i] = mind[c] before the step's update (1e10f for the first sample and for an unusable forced
//            centre, +inf for c = -1)
//   update   c >= 0 and usable: for every usable j, d = (dx dx + dy dy) + dz dz, mind[j] = d if d < mind[j]
//   distance mind after the last step, +inf for unusable points
// Two forms with identical bytes. One workgroup per cloud (n <= OVG_FPS_SMALL_MAX): the whole loop in one launch, points and mind in
// registers, the cloud in LDS for the broadcast read of the next centre, one barrier per step. One launch per sample (any n): mind in
// the workspace, the winner merged into the next step's key slot with a 64-bit unsigned atomic max (the mirror of ovg_nn.hip's atomic
// min); the next launch reads it. Stream order is the only synchronisation between workgroups: nothing here ever waits for another
// workgroup, every loop bound is an argument.
#include "ovg_geom.h"

// tests/fps_twin.py restates the rule in numpy float32, one rounding per operation: no fused multiply-adds in this unit (build.py
// compiles it with -ffp-contract=off as well)
#pragma clang fp contract(off)

namespace {

constexpr int kWgThreads = 1024;                                 // one workgroup per cloud
constexpr int kWgWaves = kWgThreads / 64;
constexpr int kWgPoints = OVG_FPS_SMALL_MAX / kWgThreads;        // points per thread, in registers
constexpr int kWgKeyBytes = 2 * kWgWaves * 8;                    // the waves' keys, double-buffered: one barrier per step
constexpr int kStepThreads = 256;                                // one launch per sample
constexpr int kStepWaves = kStepThreads / 64;
constexpr int kStepPoints = OVG_FPS_TILE / kStepThreads;
constexpr int64_t kMaxBatch = 65535;                             // gridDim.y
constexpr uint32_t kInfBits = 0x7F800000u;
constexpr uint32_t kNanBits = 0x7FC00000u;
constexpr float kFar = 1e10f;                                    // the reference's initial distance

static_assert(kWgPoints * kWgThreads == OVG_FPS_SMALL_MAX && kStepPoints * kStepThreads == OVG_FPS_TILE, "tile shapes");
static_assert(kWgKeyBytes + OVG_FPS_SMALL_MAX * 12 <= 160 * 1024, "the cloud and the keys fit the LDS of a CU");

bool fps_shape_ok(int64_t batch, int64_t n, int64_t npoint) {
  return batch >= 1 && batch <= kMaxBatch && n >= 1 && n < (1ll << 31) && npoint >= 1 && npoint < (1ll << 31);
}
// per cloud: npoint + 1 key slots (u64), then n mind (f32)
int64_t fps_ws_per_cloud(int64_t n, int64_t npoint) { return (4 * n + 8 * (npoint + 1) + 15) / 16 * 16; }

// mind of a usable point is +0 .. 1e10: its bits order like its value. +inf marks an unusable point (never a candidate): key 0 = none,
// below every real key, whose low word 0xFFFFFFFF - j is non-zero since j < 2^31. The larger key is the larger mind, then the LOWER j.
OVG_DEV uint64_t fps_key(float mind, uint32_t j) {
  const uint32_t b = __float_as_uint(mind);
  return b == kInfBits ? 0ull : ((uint64_t)b << 32) | (0xFFFFFFFFu - j);
}
OVG_DEV int32_t key_index(uint64_t key) { return key ? (int32_t)(0xFFFFFFFFu - (uint32_t)key) : -1; }
OVG_DEV float key_sqdist(uint64_t key) { return __uint_as_float(key ? (uint32_t)(key >> 32) : kInfBits); }

OVG_DEV uint64_t wave_max_key(uint64_t k) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    const uint64_t other = __shfl_xor(k, o, 64);
    k = other > k ? other : k;
  }
  return k;
}

OVG_DEV float sq3(float px, float py, float pz, float cx, float cy, float cz) {
  const float dx = px - cx, dy = py - cy, dz = pz - cz;
  return (dx * dx + dy * dy) + dz * dz;                                    // +0, positive, +inf, or NaN when either x is NaN
}

// mind[n - 1] after step 0, for the forced second sample: min(1e10, d(last, first)) when both are usable (an unusable point
// arrives with x = NaN: d is NaN and the comparison fails), 1e10 otherwise
OVG_DEV float forced_last_sqdist(float lx, float ly, float lz, float fx, float fy, float fz) {
  const float d = sq3(lx, ly, lz, fx, fy, fz);
  return d < kFar ? d : kFar;
}

// ---- one workgroup per cloud -------------------------------------------------------------------------------------------------
// blockIdx.x: cloud. Thread t holds points k * kWgThreads + t. LDS: the waves' keys [2][kWgWaves], then the cloud as x y z per point
// with x = NaN for an unusable point (3 n floats, sized by the launch).
__global__ __launch_bounds__(kWgThreads) void fps_one_workgroup(const float* __restrict__ points, const uint8_t* __restrict__ valid, int32_t n,
                                                                int32_t npoint, int32_t first, int32_t include_last,
                                                                int32_t* __restrict__ index, float* __restrict__ sqdist,
                                                                float* __restrict__ distance) {
  extern __shared__ __attribute__((aligned(16))) unsigned char lds_fps[];
  uint64_t* wkeys = reinterpret_cast<uint64_t*>(lds_fps);
  float* cloud = reinterpret_cast<float*>(lds_fps + kWgKeyBytes);
  const int64_t cloud0 = (int64_t)blockIdx.x * n;                          // first point of this cloud
  const int32_t tid = (int32_t)threadIdx.x;
  points += 3 * cloud0;
  index += (int64_t)blockIdx.x * npoint;
  sqdist += (int64_t)blockIdx.x * npoint;
  float x[kWgPoints], y[kWgPoints], z[kWgPoints], mind[kWgPoints];
#pragma unroll
  for (int k = 0; k < kWgPoints; ++k) {
    const int32_t j = k * kWgThreads + tid;                                // < OVG_FPS_SMALL_MAX
    x[k] = __uint_as_float(kNanBits), y[k] = 0.0f, z[k] = 0.0f;            // padding and unusable points: every d is NaN, nothing is taken
    mind[k] = __uint_as_float(kInfBits);
    if (j < n) {
      const float px = points[3 * j], py = points[3 * j + 1], pz = points[3 * j + 2];
      if (finite3(px, py, pz) && (!valid || valid[cloud0 + j] != 0)) x[k] = px, y[k] = py, z[k] = pz, mind[k] = kFar;
      cloud[3 * j] = x[k], cloud[3 * j + 1] = y[k], cloud[3 * j + 2] = z[k];
    }
  }
  __syncthreads();
  uint64_t key = 0;                                                        // the previous step's winner, the same in every thread
  for (int32_t i = 0; i < npoint; ++i) {
    int32_t c;
    float sq;
    if (i == 0) {
      c = first, sq = kFar;
    } else if (i == 1 && include_last) {
      c = n - 1;
      sq = forced_last_sqdist(cloud[3 * c], cloud[3 * c + 1], cloud[3 * c + 2], cloud[3 * first], cloud[3 * first + 1], cloud[3 * first + 2]);
    } else {
      c = key_index(key), sq = key_sqdist(key);
    }
    if (tid == 0) index[i] = c, sqdist[i] = sq;
    if (c >= 0) {                                                          // 0 <= c < n: first and n - 1 are checked by the host, a key holds a j < n
      const float cx = cloud[3 * c], cy = cloud[3 * c + 1], cz = cloud[3 * c + 2];      // an unusable forced centre has x = NaN: no update
#pragma unroll
      for (int k = 0; k < kWgPoints; ++k) {
        const float d = sq3(x[k], y[k], z[k], cx, cy, cz);
        mind[k] = d < mind[k] ? d : mind[k];
      }
    }
    if (i + 1 < npoint) {                                                  // uniform: every thread takes the barrier or none does
      uint64_t best = 0;
#pragma unroll
      for (int k = 0; k < kWgPoints; ++k) {
        const uint64_t cand = fps_key(mind[k], (uint32_t)(k * kWgThreads + tid));
        best = cand > best ? cand : best;
      }
      best = wave_max_key(best);
      // step i writes buffer i & 1 and reads it behind the barrier; buffer i & 1 is written again in step i + 2, behind the barrier of
      // step i + 1, which every thread reaches only after its reads of step i
      uint64_t* slot = wkeys + (i & 1) * kWgWaves;
      if ((tid & 63) == 0) slot[tid >> 6] = best;
      __syncthreads();
      key = 0;
#pragma unroll
      for (int w = 0; w < kWgWaves; ++w) key = slot[w] > key ? slot[w] : key;
    }
  }
  if (distance) {
#pragma unroll
    for (int k = 0; k < kWgPoints; ++k) {
      const int32_t j = k * kWgThreads + tid;
      if (j < n) distance[cloud0 + j] = mind[k];
    }
  }
}

// ---- one launch per sample ---------------------------------------------------------------------------------------------------
struct StepWs {
  uint64_t* keys;                                                          // [npoint + 1]: slot i holds the winner that step i samples
  float* mind;                                                             // [n]
};
OVG_DEV StepWs step_ws(void* ws, int64_t per_cloud, int32_t npoint) {
  unsigned char* base = static_cast<unsigned char*>(ws) + (int64_t)blockIdx.y * per_cloud;
  return {reinterpret_cast<uint64_t*>(base), reinterpret_cast<float*>(base + 8 * ((int64_t)npoint + 1))};
}

// grid (ceil(max(n, npoint + 1) / 256), batch): mind = 1e10 (usable) or +inf (unusable), every key slot = 0 (none)
__global__ __launch_bounds__(256) void fps_init(const float* __restrict__ points, const uint8_t* __restrict__ valid, int32_t n, int32_t npoint,
                                                void* __restrict__ ws, int64_t per_cloud) {
  const StepWs w = step_ws(ws, per_cloud, npoint);
  const uint32_t i = blockIdx.x * 256 + threadIdx.x;                       // n, npoint + 1 <= 2^31: no wrap in unsigned arithmetic
  if (i < (uint32_t)n) {
    const int64_t j = (int64_t)blockIdx.y * n + i;
    const float* p = points + 3 * j;
    w.mind[i] = finite3(p[0], p[1], p[2]) && (!valid || valid[j] != 0) ? kFar : __uint_as_float(kInfBits);
  }
  if (i <= (uint32_t)npoint) w.keys[i] = 0;
}

// point j of cloud blockIdx.y with x = NaN when it is unusable
OVG_DEV void load_centre(const float* __restrict__ points, const uint8_t* __restrict__ valid, int32_t n, int32_t j, float& x, float& y, float& z) {
  const int64_t g = (int64_t)blockIdx.y * n + j;
  const float px = points[3 * g], py = points[3 * g + 1], pz = points[3 * g + 2];
  x = __uint_as_float(kNanBits), y = 0.0f, z = 0.0f;
  if (finite3(px, py, pz) && (!valid || valid[g] != 0)) x = px, y = py, z = pz;
}

// grid (ceil(n / OVG_FPS_TILE), batch), launched once per step in stream order. Reads keys[step] (complete: the previous launch has
// ended), updates the workgroup's slice of mind and merges the slice's best into keys[step + 1].
__global__ __launch_bounds__(kStepThreads) void fps_step(const float* __restrict__ points, const uint8_t* __restrict__ valid, int32_t n,
                                                         int32_t npoint, int32_t first, int32_t include_last, int32_t step,
                                                         void* __restrict__ ws, int64_t per_cloud, int32_t* __restrict__ index,
                                                         float* __restrict__ sqdist) {
  __shared__ uint64_t wkeys[kStepWaves];
  const StepWs w = step_ws(ws, per_cloud, npoint);
  const int32_t tid = (int32_t)threadIdx.x;
  int32_t c;
  float sq, cx = __uint_as_float(kNanBits), cy = 0.0f, cz = 0.0f;
  if (step == 0) {
    c = first, sq = kFar;
  } else if (step == 1 && include_last) {
    c = n - 1;
    float fx, fy, fz;
    load_centre(points, valid, n, first, fx, fy, fz);
    load_centre(points, valid, n, c, cx, cy, cz);
    sq = forced_last_sqdist(cx, cy, cz, fx, fy, fz);
  } else {
    const uint64_t key = w.keys[step];
    c = key_index(key), sq = key_sqdist(key);
  }
  if (blockIdx.x == 0 && tid == 0) {
    index[(int64_t)blockIdx.y * npoint + step] = c;
    sqdist[(int64_t)blockIdx.y * npoint + step] = sq;
  }
  if (c >= 0) load_centre(points, valid, n, c, cx, cy, cz);                // 0 <= c < n; x = NaN for an unusable forced centre: no update
  const int32_t j0 = (int32_t)blockIdx.x * OVG_FPS_TILE;                   // < n < 2^31
  uint64_t best = 0;
#pragma unroll
  for (int k = 0; k < kStepPoints; ++k) {
    // j0 + OVG_FPS_TILE may pass 2^31: compare the offset inside the tile, which is small
    const int32_t jl = k * kStepThreads + tid;
    if (jl < n - j0) {
      const int32_t j = j0 + jl;
      float m = w.mind[j];
      if (__float_as_uint(m) != kInfBits) {                                // usable
        const float* p = points + 3 * ((int64_t)blockIdx.y * n + j);
        const float d = sq3(p[0], p[1], p[2], cx, cy, cz);
        if (d < m) m = d, w.mind[j] = d;
        const uint64_t cand = fps_key(m, (uint32_t)j);
        best = cand > best ? cand : best;
      }
    }
  }
  best = wave_max_key(best);
  if ((tid & 63) == 0) wkeys[tid >> 6] = best;
  __syncthreads();
  if (tid == 0) {
#pragma unroll
    for (int v = 1; v < kStepWaves; ++v) best = wkeys[v] > best ? wkeys[v] : best;
    // the slot starts as 0 (fps_init); the order in which the workgroups arrive does not matter to a maximum
    if (best) __hip_atomic_fetch_max(w.keys + step + 1, best, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  }
}

// grid (ceil(n / 256), batch)
__global__ __launch_bounds__(256) void fps_distance(const void* __restrict__ ws, int64_t per_cloud, int32_t n, int32_t npoint,
                                                    float* __restrict__ distance) {
  const StepWs w = step_ws(const_cast<void*>(ws), per_cloud, npoint);
  const uint32_t i = blockIdx.x * 256 + threadIdx.x;
  if (i < (uint32_t)n) distance[(int64_t)blockIdx.y * n + i] = w.mind[i];
}

}  // namespace

extern "C" int64_t ovg_fps_workspace_bytes(int64_t batch, int64_t n, int64_t npoint) {
  return fps_shape_ok(batch, n, npoint) ? batch * fps_ws_per_cloud(n, npoint) : -1;
}

extern "C" int ovg_farthest_point_sample(const ovg_fps_params* p, void* stream) {
  if (!p || !p->points || !p->ws || !p->index || !p->sqdist) return OVG_E_ARG;
  if (!fps_shape_ok(p->batch, p->n, p->npoint) || p->first < 0 || p->first >= p->n || (p->flags & ~OVG_FPS_INCLUDE_LAST)) return OVG_E_ARG;
  if (p->path != OVG_FPS_PATH_AUTO && p->path != OVG_FPS_PATH_ONE_WORKGROUP && p->path != OVG_FPS_PATH_PER_STEP) return OVG_E_ARG;
  if (p->path == OVG_FPS_PATH_ONE_WORKGROUP && p->n > OVG_FPS_SMALL_MAX) return OVG_E_ARG;
  if (!al(p->points, 4) || !al(p->index, 4) || !al(p->sqdist, 4) || !al(p->distance, 4)) return OVG_E_ARG;
  const int64_t per_cloud = fps_ws_per_cloud(p->n, p->npoint);
  if (!al(p->ws, 16) || p->ws_bytes < p->batch * per_cloud) return OVG_E_ARG;
  hipStream_t st = static_cast<hipStream_t>(stream);
  const int32_t n = (int32_t)p->n, npoint = (int32_t)p->npoint, first = (int32_t)p->first;
  const int32_t include_last = (p->flags & OVG_FPS_INCLUDE_LAST) ? 1 : 0;
  const unsigned batch = (unsigned)p->batch;
  if (p->path == OVG_FPS_PATH_ONE_WORKGROUP || (p->path == OVG_FPS_PATH_AUTO && p->n <= OVG_FPS_SMALL_MAX)) {
    const int lds_bytes = kWgKeyBytes + 12 * n;
    if (hipFuncSetAttribute(reinterpret_cast<const void*>(fps_one_workgroup), hipFuncAttributeMaxDynamicSharedMemorySize,
                            kWgKeyBytes + 12 * OVG_FPS_SMALL_MAX) != hipSuccess)
      return OVG_E_LAUNCH;
    OVG_LAUNCH(fps_one_workgroup, dim3(batch), dim3(kWgThreads), lds_bytes, st, p->points, p->valid, n, npoint, first, include_last, p->index,
               p->sqdist, p->distance);
    OVG_CHECK_LAUNCH();
    return OVG_OK;
  }
  const int64_t init_items = p->n > p->npoint + 1 ? p->n : p->npoint + 1;     // <= 2^31: at most 2^23 workgroups
  OVG_LAUNCH(fps_init, dim3((unsigned)((init_items + 255) / 256), batch), dim3(256), 0, st, p->points, p->valid, n, npoint, p->ws, per_cloud);
  OVG_CHECK_LAUNCH();
  const dim3 grid((unsigned)((p->n + OVG_FPS_TILE - 1) / OVG_FPS_TILE), batch);
  for (int32_t step = 0; step < npoint; ++step) {
    OVG_LAUNCH(fps_step, grid, dim3(kStepThreads), 0, st, p->points, p->valid, n, npoint, first, include_last, step, p->ws, per_cloud, p->index,
               p->sqdist);
    OVG_CHECK_LAUNCH();
  }
  if (p->distance) {
    OVG_LAUNCH(fps_distance, dim3((unsigned)((p->n + 255) / 256), batch), dim3(256), 0, st, p->ws, per_cloud, n, npoint, p->distance);
    OVG_CHECK_LAUNCH();
  }
  return OVG_OK;
}
