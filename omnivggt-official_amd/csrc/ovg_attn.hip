// Flash attention forward for the aggregator (gfx950), head_dim 64, no mask.
// Replaces F.scaled_dot_product_attention at omnivggt/layers/attention.py:61-66 for the
// frame-local blocks (batch = views*16 heads, N = 1374) and the global cross-view blocks
// (batch = 16 heads, N = S*1374; omnivggt/models/aggregator.py:317-336).
//
// Formulation (all on 16x16 MFMA tiles, "swapped" so softmax rows are lane-local):
//   S^T[key,q] = K[key,:] . Q[q,:]          A = K rows (LDS),  B = Q rows (registers)
//   O^T[d,q]  += V^T[d,key] * P^T[key,q]    A = V^T rows (LDS), B = P (registers, from S^T)
// A lane (q = lane&15, g = lane>>4) holds S^T for keys 16*kt + 4g + r: one q row lives in
// the 4 lanes {q, q+16, q+32, q+48}, so the row max/sum need two xor-shuffles only, the
// running max/sum/alpha are lane-local, and P feeds the PV MFMA with NO cross-lane
// movement: the k-slot -> key assignment of the P fragment is simply mirrored by the
// V^T fragment gather (two 8-byte LDS reads per fragment for 16-bit types).
// V arrives pre-transposed (V^T [BH,64,nk_pad], written by the QKV epilogue; 16-bit rows in the vt_pos16 key order). This file holds
// the baseline kernel (f32 parity mode + A/B reference: K/V^T tiles register-staged into LDS, issue-early / write-late, K tile
// XOR-swizzled, V^T tile row-padded) and the launch plan; the tuned 16-bit kernels (LDS-DMA staged) are in ovg_attn16.h.
// q is pre-scaled by softmax_scale*log2(e): probabilities are exp2(s - m).
// K/V^T may come as several segments (one per rank of the view-sharded all-gather).
#include "ovg_common.h"
#include <type_traits>
#include <cmath>

namespace {

constexpr int BC = OVG_KV_TILE;   // keys per tile

template <typename T> struct VFrag;
// 16-bit types: 32 keys per PV step u; slot j -> key 32u + 16*(j>>2) + 4g + (j&3)
template <typename T> struct VFrag {
  static constexpr int kSteps = 2;
  static constexpr int kRow = 136;   // V^T LDS row stride (128 B + 8 B pad): b64 reads conflict free
  static OVG_DEV u32x4 load(const unsigned char* vl, int d, int step, int g) {
    // global V^T rows are in the vt_pos16 order (ovg_common.h): chunk g of block `step` IS the fragment (keys 4g.., 16+4g..)
    const unsigned char* p = vl + d * kRow + (32 * step + 8 * g) * 2;
    const u32x2 lo = *reinterpret_cast<const u32x2*>(p);
    const u32x2 hi = *reinterpret_cast<const u32x2*>(p + 8);
    return u32x4{lo[0], lo[1], hi[0], hi[1]};
  }
  static OVG_DEV u32x4 pfrag(const f32x4 (&s)[4], int step) {
    T v[8];
    const f32x4 a = s[2 * step], b = s[2 * step + 1];
    v[0] = TT<T>::from_f32(a[0]); v[1] = TT<T>::from_f32(a[1]); v[2] = TT<T>::from_f32(a[2]); v[3] = TT<T>::from_f32(a[3]);
    v[4] = TT<T>::from_f32(b[0]); v[5] = TT<T>::from_f32(b[1]); v[6] = TT<T>::from_f32(b[2]); v[7] = TT<T>::from_f32(b[3]);
    u32x4 r;
    __builtin_memcpy(&r, v, 16);
    return r;
  }
};
// f32: 16 keys per PV step kt; MFMA i uses key 16kt + 4g + i
template <> struct VFrag<float> {
  static constexpr int kSteps = 4;
  static constexpr int kRow = 272;
  static OVG_DEV u32x4 load(const unsigned char* vl, int d, int step, int g) {
    return *reinterpret_cast<const u32x4*>(vl + d * kRow + (16 * step + 4 * g) * 4);
  }
  static OVG_DEV u32x4 pfrag(const f32x4 (&s)[4], int step) { return __builtin_bit_cast(u32x4, s[step]); }
};

// QB = 16-row q blocks per wave; 4 waves -> BQ = 64*QB q rows per workgroup
template <typename T, int QB>
__global__ __launch_bounds__(256) void attn_kernel(ovg_attn_params p, int nqt, int total_tiles) {
  constexpr int RB = OVG_D * (int)sizeof(T);   // K row bytes
  constexpr int NCH = RB / 16;                 // 16 B chunks per K row
  constexpr int NKK = NCH / 4;                 // MFMA steps over d
  constexpr int VROW = VFrag<T>::kRow;
  constexpr int NSTEP = VFrag<T>::kSteps;
  constexpr int KT_B = BC * RB, VT_B = OVG_D * VROW;
  constexpr int NBUF = sizeof(T) == 2 ? 2 : 1;
  constexpr int CPT = BC * NCH / 256;          // chunks per thread per tile (2 or 4)
  constexpr int BQ = 64 * QB;
  __shared__ __attribute__((aligned(16))) unsigned char lds[NBUF * (KT_B + VT_B)];

  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int g = lane >> 4, lr = lane & 15;
  const int lid = xcd_remap(blockIdx.x, gridDim.x);
  const int bh = lid / nqt, qt = lid % nqt;
  const int nq = (int)p.nq;
  const int q0 = qt * BQ + wave * 16 * QB;

  // ---- Q fragments (B operand), straight from global -------------------
  u32x4 qf[QB][NKK];
  {
    const unsigned char* qbase = static_cast<const unsigned char*>(p.q) + (int64_t)bh * p.nq_pad * RB;
#pragma unroll
    for (int qb = 0; qb < QB; ++qb) {
      int q = q0 + qb * 16 + lr; q = q < nq ? q : nq - 1;
#pragma unroll
      for (int kk = 0; kk < NKK; ++kk)
        qf[qb][kk] = *reinterpret_cast<const u32x4*>(qbase + (int64_t)q * RB + (4 * kk + g) * 16);
    }
  }

  f32x4 o[QB][4];
  float mrow[QB], lrow[QB];
#pragma unroll
  for (int qb = 0; qb < QB; ++qb) {
    mrow[qb] = -1.0e30f; lrow[qb] = 0.f;
#pragma unroll
    for (int dt = 0; dt < 4; ++dt) o[qb][dt] = f32x4{0.f, 0.f, 0.f, 0.f};
  }

  // ---- staging state: (segment, tile) of the NEXT tile to fetch ---------
  int fseg = 0, ftile = 0;
  int f_ntiles = (int)((p.seg[0].nk + BC - 1) / BC);
  u32x4 rk[CPT], rv[CPT];
  int k_goff[CPT], v_row[CPT], v_ch[CPT], k_loff[CPT], v_loff[CPT];
#pragma unroll
  for (int i = 0; i < CPT; ++i) {
    const int c = tid + 256 * i;
    const int row = c / NCH, ch = c % NCH;
    k_goff[i] = c * 16;
    k_loff[i] = swz_off<RB>(row, ch);
    v_row[i] = row; v_ch[i] = ch;
    v_loff[i] = row * VROW + ch * 16;
  }
  auto fetch = [&]() {
    const ovg_kv_segment sg = p.seg[fseg];
    const int kvh = p.kv_heads > 0 ? bh % p.kv_heads : bh;
    const unsigned char* kb = static_cast<const unsigned char*>(sg.k) + ((int64_t)kvh * sg.nk_pad + (int64_t)ftile * BC) * RB;
    const unsigned char* vb = static_cast<const unsigned char*>(sg.vt) + ((int64_t)kvh * OVG_D * sg.nk_pad + (int64_t)ftile * BC) * (int64_t)sizeof(T);
#pragma unroll
    for (int i = 0; i < CPT; ++i) {
      rk[i] = *reinterpret_cast<const u32x4*>(kb + k_goff[i]);
      rv[i] = *reinterpret_cast<const u32x4*>(vb + (int64_t)v_row[i] * sg.nk_pad * (int64_t)sizeof(T) + v_ch[i] * 16);
    }
    if (++ftile == f_ntiles) {
      ftile = 0; ++fseg;
      if (fseg < p.nseg) f_ntiles = (int)((p.seg[fseg].nk + BC - 1) / BC);
    }
  };
  auto stash = [&](int buf) {
    unsigned char* kl = lds + buf * (KT_B + VT_B);
    unsigned char* vl = kl + KT_B;
#pragma unroll
    for (int i = 0; i < CPT; ++i) {
      *reinterpret_cast<u32x4*>(kl + k_loff[i]) = rk[i];
      *reinterpret_cast<u32x2*>(vl + v_loff[i]) = u32x2{rv[i][0], rv[i][1]};
      *reinterpret_cast<u32x2*>(vl + v_loff[i] + 8) = u32x2{rv[i][2], rv[i][3]};
    }
  };

  // compute-side bookkeeping: valid keys left in the current segment
  int cseg = 0, ctile = 0;
  int c_ntiles = f_ntiles;
  int c_nk = (int)p.seg[0].nk;

  fetch();
  stash(0);
  __syncthreads();

  int buf = 0;
  for (int j = 0; j < total_tiles; ++j) {
    const bool more = (j + 1) < total_tiles;
    if (more) fetch();

    const unsigned char* kl = lds + buf * (KT_B + VT_B);
    const unsigned char* vl = kl + KT_B;

    // ---- S^T = K Q^T ----------------------------------------------------
    f32x4 s[QB][4];
#pragma unroll
    for (int qb = 0; qb < QB; ++qb)
#pragma unroll
      for (int kt = 0; kt < 4; ++kt) s[qb][kt] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int kt = 0; kt < 4; ++kt) {
#pragma unroll
      for (int kk = 0; kk < NKK; ++kk) {
        const u32x4 kf = *reinterpret_cast<const u32x4*>(kl + swz_off<RB>(16 * kt + lr, 4 * kk + g));
#pragma unroll
        for (int qb = 0; qb < QB; ++qb) TT<T>::mma(s[qb][kt], kf, qf[qb][kk]);
      }
    }
    // ---- mask the ragged tail of a segment ------------------------------
    const int kv0 = ctile * BC;
    if (kv0 + BC > c_nk) {
#pragma unroll
      for (int kt = 0; kt < 4; ++kt)
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          const bool dead = (kv0 + 16 * kt + 4 * g + r) >= c_nk;
#pragma unroll
          for (int qb = 0; qb < QB; ++qb) s[qb][kt][r] = dead ? -INFINITY : s[qb][kt][r];
        }
    }
    // ---- online softmax (per q block) -----------------------------------
#pragma unroll
    for (int qb = 0; qb < QB; ++qb) {
      float mx = s[qb][0][0];
#pragma unroll
      for (int kt = 0; kt < 4; ++kt)
#pragma unroll
        for (int r = 0; r < 4; ++r) mx = fmaxf(mx, s[qb][kt][r]);
      mx = fmaxf(mx, __shfl_xor(mx, 16, 64));
      mx = fmaxf(mx, __shfl_xor(mx, 32, 64));
      const float mnew = fmaxf(mrow[qb], mx);
      const float alpha = __builtin_amdgcn_exp2f(mrow[qb] - mnew);
      mrow[qb] = mnew;
      float rs = 0.f;
#pragma unroll
      for (int kt = 0; kt < 4; ++kt)
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          const float pv = __builtin_amdgcn_exp2f(s[qb][kt][r] - mnew);
          s[qb][kt][r] = pv;
          rs += pv;
        }
      lrow[qb] = lrow[qb] * alpha + rs;
#pragma unroll
      for (int dt = 0; dt < 4; ++dt) o[qb][dt] *= alpha;
    }
    // ---- O^T += V^T P^T --------------------------------------------------
#pragma unroll
    for (int st = 0; st < NSTEP; ++st) {
      u32x4 pf[QB];
#pragma unroll
      for (int qb = 0; qb < QB; ++qb) pf[qb] = VFrag<T>::pfrag(s[qb], st);
#pragma unroll
      for (int dt = 0; dt < 4; ++dt) {
        const u32x4 vf = VFrag<T>::load(vl, 16 * dt + lr, st, g);
#pragma unroll
        for (int qb = 0; qb < QB; ++qb) TT<T>::mma(o[qb][dt], vf, pf[qb]);
      }
    }

    // advance compute-side tile bookkeeping
    if (++ctile == c_ntiles) {
      ctile = 0; ++cseg;
      if (cseg < p.nseg) { c_nk = (int)p.seg[cseg].nk; c_ntiles = (c_nk + BC - 1) / BC; }
    }
    if (NBUF == 1) __syncthreads();
    if (more) stash(NBUF == 2 ? (buf ^ 1) : 0);
    __syncthreads();
    if (NBUF == 2) buf ^= 1;
  }

  // ---- epilogue: normalise and store token-major ---------------------------
  const int bq = bh / OVG_H, hh = bh % OVG_H;
#pragma unroll
  for (int qb = 0; qb < QB; ++qb) {
    float lt = lrow[qb];
    lt += __shfl_xor(lt, 16, 64);
    lt += __shfl_xor(lt, 32, 64);
    const float inv = 1.0f / lt;
    const int q = q0 + qb * 16 + lr;
    if (q < nq) {
      T* dst = p.out_bh_stride > 0 ? static_cast<T*>(p.out) + (int64_t)bh * p.out_bh_stride + (int64_t)q * p.ldo + 4 * g
                                   : static_cast<T*>(p.out) + ((int64_t)bq * nq + q) * p.ldo + hh * OVG_D + 4 * g;
#pragma unroll
      for (int dt = 0; dt < 4; ++dt)
        store4<T>(dst + 16 * dt, o[qb][dt][0] * inv, o[qb][dt][1] * inv, o[qb][dt][2] * inv, o[qb][dt][3] * inv);
      if (p.lse != nullptr && g == 0) p.lse[(int64_t)bh * p.nq_pad + q] = __builtin_amdgcn_logf(lt) + mrow[qb];
    }
  }
}

#include "ovg_attn16.h"

int total_key_tiles(const ovg_attn_params& p) {
  int total = 0;
  for (int i = 0; i < p.nseg; ++i) total += (int)((p.seg[i].nk + BC - 1) / BC);
  return total;
}

// baseline kernel (all dtypes; the f32 parity path and the in-process reference of the A/B tool)
template <typename T, int QB>
int launch_attn(const ovg_attn_params& p, hipStream_t st) {
  constexpr int BQ = 64 * QB;
  const int nqt = (int)((p.nq + BQ - 1) / BQ);
  const dim3 grid((unsigned)(p.BH * nqt)), block(256);
  OVG_LAUNCH((attn_kernel<T, QB>), grid, block, 0, st, p, nqt, total_key_tiles(p));
  OVG_CHECK_LAUNCH();
  return OVG_OK;
}

// ---- one launch of a 16-bit kernel -------------------------------------------------------------------------------------
// The key ranges a launch cuts every (batch entry, q tile) unit into: `splits` ranges of `per_split` key tiles (1 = unsplit; more = partials
// into the caller's workspace, part_rows rows per entry, + the merge launch).
struct Pass16 { int total_tiles; int splits; int per_split; int part_rows; };

Pass16 key_ranges(int total_tiles, int splits, int64_t part_rows) {
  if (splits > OVG_MAX_SEG) splits = OVG_MAX_SEG;
  if (splits > total_tiles) splits = total_tiles;
  const int per = (total_tiles + splits - 1) / splits;
  return Pass16{total_tiles, (total_tiles + per - 1) / per, per, (int)part_rows};       // every range non-empty
}

template <typename T, int QB, int WAVES, int MODE, int RING, int X3 = 0>
int launch_attn16(const ovg_attn_params& p, const Pass16& ps, hipStream_t st, int64_t row0, int64_t row1) {   // q rows [row0, row1)
  constexpr int BQ = 16 * QB * WAVES;
  const int nqt = (int)((row1 - row0 + BQ - 1) / BQ);
  const dim3 grid((unsigned)(p.BH * nqt * ps.splits)), block(64 * WAVES);
  OVG_LAUNCH((attn16_kernel<T, QB, WAVES, MODE, RING, X3>), grid, block, 0, st, p, nqt, ps.total_tiles, ps.splits, ps.per_split, (int)row0, ps.part_rows);
  OVG_CHECK_LAUNCH();
  if (ps.splits > 1) {
    const int64_t blocks = (p.BH * (row1 - row0) * 8 + 255) / 256;
    OVG_LAUNCH((attn_split_merge_kernel<T>), dim3((unsigned)(blocks < 65536 ? blocks : 65536)), dim3(256), 0, st, p, ps.splits, (int)row0, (int)(row1 - row0), ps.part_rows);
    OVG_CHECK_LAUNCH();
  }
  return OVG_OK;
}

using Launch16 = int (*)(const ovg_attn_params&, const Pass16&, hipStream_t, int64_t, int64_t);

template <typename T>
int launch_baseline16(const ovg_attn_params& p, const Pass16&, hipStream_t st, int64_t, int64_t) { return launch_attn<T, 1>(p, st); }   // whole call, never split

// ---- the kernels of the 16-bit dtypes by name (values = ovg_attn_params.variant, include/omnivggt_hip.h; numbers kept from the A/B logs under profiles/) ----
//   Baseline           baseline kernel (attn_kernel above; never split)
//   Spec256 / Spec128  speculative kernel (3-slot ring, barrier per tile) with 256- / 128-row q tiles; Spec256 = the bf16 default for short launches
//   Lazy256 / Lazy128  lazy-rescale kernel, 256- / 128-row q tiles -- the f16 default (Lazy256 for nq >= 4096, else Lazy128; a 512-row 8-wave form of the
//                      lazy-rescale body measured 4 % slower at 64 views: profiles/r02_attention_dma_ab.txt)
//   Forced256          the 256-row speculative kernel with the fallback forced (tests)
//   Spec512            speculative kernel with 512-row q tiles, 8 waves, 5-slot ring (a workgroup barrier every 2 tiles): the bf16 default for
//                      launches of >= 2.5 rounds of 512-row tiles
enum class Kernel16 : int { Baseline = OVG_ATTN_BASELINE, Spec256 = OVG_ATTN_SPEC256, Lazy256 = OVG_ATTN_LAZY256, Forced256 = OVG_ATTN_FORCED256,
                            Spec128 = OVG_ATTN_SPEC128, Lazy128 = OVG_ATTN_LAZY128, Spec512 = OVG_ATTN_SPEC512 };

// one row per kernel: q-tile rows and the launch of either dtype, launch_attn16<T, q blocks per wave, waves, MODE, ring slots>
struct Kernel16Row { Kernel16 kernel; int bq; Launch16 bf16; Launch16 f16; };
#define OVG_ROW16(name, bq, ...) {Kernel16::name, bq, launch_attn16<bf16_t, __VA_ARGS__>, launch_attn16<f16_t, __VA_ARGS__>}
constexpr Kernel16Row kKernels16[] = {
  {Kernel16::Baseline, 64, launch_baseline16<bf16_t>, launch_baseline16<f16_t>},
  OVG_ROW16(Spec256, 256, 4, 4, 0, 3),
  OVG_ROW16(Lazy256, 256, 4, 4, 1, 3),
  OVG_ROW16(Forced256, 256, 4, 4, 2, 3),
  OVG_ROW16(Spec128, 128, 2, 4, 0, 3),       // also the tail of a 128-row tail
  OVG_ROW16(Lazy128, 128, 2, 4, 1, 3),
  OVG_ROW16(Spec512, 512, 4, 8, 0, 5),
};
#undef OVG_ROW16

const Kernel16Row* kernel_row(int variant) {
  for (const Kernel16Row& r : kKernels16)
    if ((int)r.kernel == variant) return &r;
  return nullptr;
}
int q_rows(Kernel16 k) { return kernel_row((int)k)->bq; }
template <typename T> Launch16 launcher(Kernel16 k) {
  const Kernel16Row* r = kernel_row((int)k);
  return std::is_same<T, bf16_t>::value ? r->bf16 : r->f16;
}

// Retired (the A/B history of rounds 1-4; OVG_E_UNSUPPORTED; removed by the commit "Retire the A/B-history kernel variants", measurements
// under profiles/): 2, 6, 8, 18, 19, 21, 25, 31, 32, 33, 51, 56, 58, 59.
bool retired_variant(int v) {
  for (const int r : {2, 6, 8, 18, 19, 21, 25, 31, 32, 33, 51, 56, 58, 59})
    if (v == r) return true;
  return false;
}

// ---- what the caller asked for: (variant, kv_splits) decoded once; nothing below reads p.variant or p.kv_splits ----------
struct Request16 {
  bool auto_kernel;      // OVG_ATTN_AUTO: the rules choose the kernel, and both tails may be planned
  Kernel16 kernel;       // else this kernel, without a tail unless a plan knob allows one:
  enum { NoKnob, RowTail, KeyTail } knob;   // 71 / 72: the 128-row tail; 73 / 74: the key-split tail
  int tail_ranges;       // 73 / 74 with kv_splits s > 1: the key-split tail with exactly s key ranges (0 = the rule's own choice)
  int kv_splits;         // whole-launch key split: 0 = the model decides, 1 = never, 2.. = forced
  bool row_tail_allowed() const { return auto_kernel || knob == RowTail; }
  bool key_tail_allowed() const { return auto_kernel || knob == KeyTail; }
};

bool decode_request(int variant, int kv_splits, Request16* rq) {   // false: not a variant of the 16-bit dtypes
  *rq = Request16{variant == OVG_ATTN_AUTO, Kernel16::Spec256, Request16::NoKnob, 0, kv_splits};
  switch (variant) {
    case OVG_ATTN_AUTO: return true;
    case OVG_ATTN_PLAN_ROWTAIL512: rq->kernel = Kernel16::Spec512; rq->knob = Request16::RowTail; return true;   // A/B tool: the 512-row kernel with its tail split
    case OVG_ATTN_PLAN_ROWTAIL256: rq->kernel = Kernel16::Spec256; rq->knob = Request16::RowTail; return true;   // A/B tool: the 256-row kernel with a tail split
    case OVG_ATTN_PLAN_KEYTAIL256:                                                                               // A/B tool: the 256-row kernel with a key-split tail
    case OVG_ATTN_PLAN_KEYTAIL512:                                                                               // A/B tool: the 512-row kernel with a key-split tail
      rq->kernel = variant == OVG_ATTN_PLAN_KEYTAIL256 ? Kernel16::Spec256 : Kernel16::Spec512;
      rq->knob = Request16::KeyTail;
      if (kv_splits > 1) { rq->tail_ranges = kv_splits; rq->kv_splits = 0; }                                     // + kv_splits s = exactly s key ranges
      return true;
    default: {
      const Kernel16Row* r = kernel_row(variant);
      if (r == nullptr) return false;
      rq->kernel = r->kernel;
      return true;
    }
  }
}

int cu_count_attn() {
  static const int n = [] {
    int dev = 0, v = 0;
    if (hipGetDevice(&dev) != hipSuccess || hipDeviceGetAttribute(&v, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess || v <= 0) v = 256;
    return v;
  }();
  return n;
}

// ---- launch plan of the 16-bit kernels: q tile (128, 256 or 512 rows), split-KV factor and tail ----------------------------
// `slots` = workgroups resident at once (256 CUs x 2 workgroups of 4 waves, or x 1 of 8 waves). A launch of U equal units
// takes ceil(U / slots) rounds; cutting every unit into s key ranges makes the rounds 1/s as long at ~1.5 key tiles of
// fixed cost per unit (anchor prologue, Q load, epilogue). The default q tile is 256 rows; launches of >= 2.5 rounds of
// 512-row tiles take those (1 workgroup of 8 waves per CU: every staged K / V^T tile feeds twice the rows; 16 views +5.9 %,
// 64 views +3 %, 8 views -17 % -- profiles/r02_attention_dma_ab.txt), with the rows beyond the last full round in a second
// launch of 128-row tiles (dispatch16).
enum class Tail16 { None, Rows128, KeyRanges };
struct Tail16Plan { Tail16 kind; int64_t main_rows; int ranges; };   // rows [0, main_rows) of every entry in the first launch; the rest as 128-row tiles, or as the main kernel's tiles cut into `ranges` key ranges + merge
constexpr Tail16Plan kNoTail{Tail16::None, 0, 0};

struct Plan16 { Kernel16 kernel; int total_tiles;
                int splits;                          // whole-launch key split (normalised: every range non-empty); > 1 excludes a tail
                Tail16Plan tail; };

// what every rule may look at
struct PlanIn { const ovg_attn_params& p; Request16 rq; bool bf16; bool have_ws; int cus; int total_tiles; };

int64_t units_of(const PlanIn& in, Kernel16 k) { return in.p.BH * ((in.p.nq + q_rows(k) - 1) / q_rows(k)); }

// ---- rule 1: the kernel -------------------------------------------------------------------------------------------------------
Kernel16 choose_kernel(const PlanIn& in) {
  if (!in.rq.auto_kernel) return in.rq.kernel;
  const ovg_attn_params& p = in.p;
  const int cus = in.cus;
  const int64_t units512 = p.BH * ((p.nq + 511) / 512);
  // 512-row tiles (8 waves, one workgroup per CU, barrier every 2 tiles) from ~2.5 rounds of them on: 16 views +5.9 %, 64 views +3 %
  // over the 256-row kernel; below that the coarser tiles quantise worse than they gain (8 views: -17 %)
  // short sequences (frame-local attention, 1374 rows): the tile that pads the sequence least wins -- 11 x 128 = 1408 rows against
  // 6 x 256 = 3 x 512 = 1536 (64 views: 0.521 ms with 128-row tiles, 0.537 with 256-row, 0.556 with 512-row)
  const int64_t pad128 = (p.nq + 127) / 128 * 128, pad256 = (p.nq + 255) / 256 * 256;
  if (!in.bf16) return p.nq >= 4096 ? Kernel16::Lazy256 : Kernel16::Lazy128;
  if (p.nq >= 4096) {
    // Launches below 2.5 rounds of 512-row tiles: 256-row tiles (two workgroups per CU, 2 x CUs slots) or 128-row tiles (three per CU).
    // r04 A/B, one process, 16 heads x S views (profiles/r04_attention_small_launches_ab.txt; 256-row / 128-row time in ms):
    //   S = 3  0.101 / 0.090   4  0.133 / 0.121   5  0.179 / 0.210   6  0.309 / 0.283   7  0.380 / 0.364   8  0.414 / 0.456   10  0.660 / 0.670   12  0.994 / 1.008
    // i.e. pure quantisation: 128-row tiles win when they need no more (ceil) rounds of their 3 x CUs slots than the 256-row tiles of their
    // 2 x CUs slots AND either everything fits one round (more CUs busy) or their last round is at most ~65 % full (a fuller last round of
    // three 4-wave workgroups per CU runs slower than the 256-row kernel's: S = 8, 1.79 rounds, -9 %).
    const int64_t u256 = p.BH * ((p.nq + 255) / 256), u128 = p.BH * ((p.nq + 127) / 128);
    const int64_t s256 = 2 * (int64_t)cus, s128 = 3 * (int64_t)cus;
    const int64_t c256 = (u256 + s256 - 1) / s256, c128 = (u128 + s128 - 1) / s128;
    const bool small128 = c128 <= c256 && (c128 == 1 || 100 * (c128 * s128 - u128) >= 35 * s128);
    return 2 * units512 >= 5 * (int64_t)cus ? Kernel16::Spec512 : (small128 ? Kernel16::Spec128 : Kernel16::Spec256);
  }
  return (pad128 * 26 < pad256 * 25 && 2 * p.BH * (pad128 / 128) >= 15 * (int64_t)cus) ? Kernel16::Spec128 : Kernel16::Spec256;   // ... from 2.5 rounds of 3 x CUs slots on (8 views: 0.069 ms with 256-row, 0.072 with 128-row tiles)
}

// ---- rule 2: the whole-launch key split ------------------------------------------------------------------------------------------
int whole_launch_splits(const PlanIn& in, Kernel16 k) {
  const ovg_attn_params& p = in.p;
  if (in.rq.kv_splits > 1) return in.rq.kv_splits;
  int splits = 1;
  if (in.rq.kv_splits == 0 && in.have_ws && (k == Kernel16::Spec256 || k == Kernel16::Lazy256 || k == Kernel16::Spec128 || k == Kernel16::Lazy128)) {   // two-workgroups-per-CU kernels (the 512-row ones have the tail split)
    // Measured model (LDS-DMA kernels, profiles/r02_attention_splitkv_ab.txt second block): a launch of R = units / slots rounds runs at
    // eff(R) = 1 - 0.2035 / R^0.72 of the many-round rate of 1.33 PFLOP/s (0.835 at R = 1.34, 0.88-0.90 at 2.7, 0.94-0.95 at 5.4, 0.963 at
    // 10.75: measured at 8 / 16 / 32 / 64 views and on the per-rank launch of the 8-GPU run); a split costs ~1.5 key tiles per unit plus the
    // partial results' round trip through HBM (in situ ~2.5 TB/s for the write + read-back). Single-GPU launches never qualify (8 views: the
    // partials cost 17 % of the launch); the per-rank launches of the view-sharded run (8 views of queries x 64 views of keys: 3.57 ms unsplit,
    // 3.43 ms at 2 splits, 3.15 ms at 4) take 4 splits.
    const int slots = 2 * in.cus;   // NOT a fix to make: the 128-row kernels run THREE workgroups per CU (choose_kernel counts 3 x CUs for them), yet this model was fitted and shipped with 2 x CUs for all four kernels
    double nk_total = 0;
    for (int i = 0; i < p.nseg; ++i) nk_total += (double)p.seg[i].nk;
    const double t0 = 4.0 * p.BH * (double)p.nq * nk_total * OVG_D / 1.33e15;           // seconds at the many-round rate
    auto eff = [](double R) { return R < 1.0 ? 0.8 * R : 1.0 - 0.2035 / pow(R, 0.72); };   // below one round: idle CUs, linear
    const double R = (double)units_of(in, k) / slots;
    const double unsplit = t0 / eff(R);
    double best = unsplit * 0.985;                   // a split must be worth >= 1.5 %; among the splits the estimated minimum wins
    for (int s = 2; s <= OVG_MAX_SEG; ++s) {
      const int per = (in.total_tiles + s - 1) / s;
      if (per < 16) break;
      const double part_bytes = 2.0 * s * p.BH * (double)p.nq * OVG_D * 2;
      double t = t0 / eff(R * s) * (1.0 + 1.5 / per) + part_bytes / 2.5e12 + 8e-6;   // + the merge launch
      if (p.nseg > 1 && p.nseg % s == 0) t *= 0.98;    // passes that end on segment boundaries (8 segments: 3.13 ms at 4 splits, 3.18 at 5, 3.49 at 3)
      if (t < best) { best = t; splits = s; }
    }
  }
  return splits;
}

// ---- rule 3: the 128-row tail (unsplit launches of the two default bf16 kernels; the RowTail knobs force it for the A/B tool) ----
// 512-row kernel (one workgroup per CU): a launch of R = units / CUs rounds pays a whole round -- or more: nothing to overlap with -- for its
// fractional last one (tools/probes/attn_tail_probe.py, 64 views: 22.18 ms for 10.0 rounds, 24.91 ms for 10.75: +4.6 % per row). The full
// rounds keep the 512-row tiles; the remaining rows of every head go to a second launch of 128-row tiles (three workgroups per CU) that
// spreads them over the whole chip. Measured (profiles/r02_attention_dma_ab.txt): 16 / 24 / 32 / 48 / 64 views +1.5 / +11.5 / +7.6 / +4.1 / +1.5 %
// over the unsplit 512-row launch and best-or-within-1.3 % of the best of {256-row, 512-row} x {split, unsplit} at every size.
// 256-row kernel (two workgroups per CU) in the 1 .. 2.5-round regime, 8 to 14 views on one GPU (profiles/r03_attention_tail256_ab.txt,
// r03_attention_tail256_sweep.txt): 9 / 10 views (1.53 / 1.69 rounds) +6.3 / +4.5 %; 8 views (1.34 rounds) -4 % -- a third-full second round of
// lone workgroups (one per CU, the whole CU's LDS bandwidth and issue slots to itself) already runs fast; 13 / 14 views (2.19 / 2.38 rounds)
// +1.8 / -3 %. So: exactly one full round and at least half a round of tail.
Tail16Plan row_tail_128(const PlanIn& in, Kernel16 k) {
  const ovg_attn_params& p = in.p;
  const bool k512 = k == Kernel16::Spec512;
  if (!(k512 || k == Kernel16::Spec256) || !in.rq.row_tail_allowed() || !(k512 || p.nq >= 4096)) return kNoTail;
  const int tslots = k512 ? in.cus : 2 * in.cus;
  const int64_t units = units_of(in, k);
  const int64_t full = units / tslots;
  const double frac = (double)units / tslots - (double)full;
  const int64_t rows_a = full * tslots / p.BH * q_rows(k);
  const bool want = k512 ? (full >= 2 && frac > 0.05)
                         : (in.rq.knob == Request16::RowTail ? (full >= 1 && frac > 0.05) : (full == 1 && frac > 0.5));
  if (want && frac < 0.85 && rows_a > 0 && rows_a < p.nq) return Tail16Plan{Tail16::Rows128, rows_a, 0};
  return kNoTail;
}

// ---- rule 4: the key-split tail of the 256-row kernels (round 5; unsplit launches of the two-workgroups-per-CU 256-row kernels, workspace given) ----
// A launch of R = units / slots rounds with a small fractional last round leaves most CUs idle for that round's whole length (13 views: 1120
// units on 512 slots, 2.19 rounds). The full rounds run unsplit; the rows beyond them run as the same 256-row tiles cut into s key ranges
// (the tail launch is then at most one round of short units) + the exact log-sum-exp merge on those rows only. Unlike a whole-launch
// split the partials cover the tail rows only (13 views: 96 of 1120 units).
Tail16Plan key_tail_256(const PlanIn& in, Kernel16 k) {
  const ovg_attn_params& p = in.p;
  if (!in.have_ws || in.rq.kv_splits != 0 || !(k == Kernel16::Spec256 || k == Kernel16::Lazy256) || !in.rq.key_tail_allowed() || p.nq < 4096) return kNoTail;
  const bool forced = in.rq.knob == Request16::KeyTail;
  const int bq = q_rows(k);
  const int tslots = 2 * in.cus;
  const int64_t units = units_of(in, k);
  const int64_t full = units / tslots, rest = units - full * tslots;     // units of the fractional last round
  const double frac = (double)rest / tslots;
  const int64_t rows_a = full * tslots / p.BH * bq;
  // s key ranges per tail unit so that the tail launch stays within ONE round of slots (8 views: 176 units -> 2 ranges = 352 pieces; 3 ranges =
  // 528 pieces on 512 slots measured 5 % SLOWER than the unsplit launch, profiles/r05_attention_keytail_ab.txt)
  const int64_t tail_units_256 = rows_a < p.nq ? p.BH * ((p.nq - rows_a + bq - 1) / bq) : 0;   // >= rest: rows_a rounds down per entry when BH does not divide a round (round-5 advisor)
  int s = in.rq.tail_ranges ? in.rq.tail_ranges : (tail_units_256 > 0 ? (int)(tslots / tail_units_256) : 1);
  s = s > OVG_MAX_SEG ? OVG_MAX_SEG : s;
  while (s > 2 && (in.total_tiles + s - 1) / s < 16) --s;
  // measured (profiles/r05_attention_keytail_ab.txt, r05_attention_keytail_factors_ab.txt; unsplit -> key-split tail, ms): 13 views (2.19 rounds)
  // 1.168 -> 1.089 (+7 %), 14 views (2.38) 1.274 -> 1.264 at best, 8 views (1.34) 0.443 -> 0.440 at best and 0.457 with the one-round factor:
  // a last round that is a third full or more already runs fast on its lone workgroups. So: a tail of at most a quarter of a round.
  const bool want = forced ? (full >= 1 && rest > 0) : (full >= 1 && full <= 3 && frac >= 0.05 && frac <= 0.25);
  if (want && s >= 2 && rows_a > 0 && rows_a < p.nq && (in.total_tiles + s - 1) / s >= 16) return Tail16Plan{Tail16::KeyRanges, rows_a, s};
  return kNoTail;
}

// ---- rule 5: the key-split tail of the 512-row kernel (round 6; workspace given) ----
// The 128-row tail launch above walks ALL keys of a head with 32 rows per wave: whatever its size it costs 0.6-0.9 of a full 512-row round
// (64 views: 2.0 ms for 0.73 of a round's rows, 0.757 GB of fabric reads for 6.8 % of the work; 48 views: 0.65 of a round for 0.06 of one), and
// it re-reads K / V^T once per 128 rows. Instead the rows beyond the last full round stay 512-row tiles (64 rows per wave, a quarter of the K / V^T
// re-reads) and are cut along the KEYS into s ranges, s chosen so that tail units x s fills whole rounds of the chip (64 views: 192 units x 4 =
// 768 = 3 rounds of quarter-length units = 0.75 of a round for 0.73 of a round's rows), + the exact log-sum-exp merge on those rows only.
// Cost model in units of one full 512-row round (fitted to profiles/r06_attention_tail512_ab.txt, 16 / 64 views x s = 2..8): the 128-row tail
// max(0.6, 0.9 x its share of a round of 3 x CUs slots) (r02 / r05 / r06 measurements at 32 / 48 / 64 views: 0.58 / 0.65 / 0.90); a key split
// (full rounds + sqrt(fraction of the last one)) / s -- a partly filled round of lone workgroups runs faster than a full one -- x (1 + 6 key
// tiles of fixed cost per unit: Q load, ring fill, f32 partial store) + 0.03 for the merge launch, with a small preference for MORE ranges
// while a range still holds >= 128 key tiles (64 views: s = 8 measured 23.50 ms against 23.59 at s = 4 with identical round counts: finer units
// fill the ragged end of the launch); no tail launch at all: 1. Measured, old 128-row tail -> this rule: 16 / 24 / 32 / 48 / 64 views
// 1.597 -> 1.557 / 3.632 -> 3.433 / 6.152 -> 5.985 / 13.825 -> 13.447 / 23.98 -> 23.50 ms (+2.6 / +5.8 / +2.8 / +2.8 / +2.0 %).
// have_row_tail: rule 3 planned a 128-row tail for these rows -- the cost this rule has to beat (else: no tail launch at all).
Tail16Plan key_tail_512(const PlanIn& in, Kernel16 k, bool have_row_tail) {
  const ovg_attn_params& p = in.p;
  if (k != Kernel16::Spec512 || !in.have_ws || in.rq.kv_splits != 0 || !in.rq.key_tail_allowed()) return kNoTail;
  const int cus = in.cus, bq = q_rows(k), forced_ranges = in.rq.tail_ranges;
  const int64_t full = units_of(in, k) / cus;
  const int64_t rows_a = full * cus / p.BH * bq;
  const int64_t rest_rows = p.nq - rows_a;
  if (!(full >= 2 && rows_a > 0 && rest_rows > 0)) return kNoTail;
  const int64_t tail_units = p.BH * ((rest_rows + bq - 1) / bq);          // from the ACTUAL tail rows (rows_a rounds down when BH does not divide a round)
  const int64_t t128 = p.BH * ((rest_rows + 127) / 128);
  double base = 1.0;                                     // what the launch pays for these rows today
  if (have_row_tail) { const double c = 0.9 * (double)t128 / (3.0 * cus); base = c < 0.6 ? 0.6 : c; }
  double best = 1e30;
  int best_s = 0;
  for (int s = 2; s <= OVG_MAX_SEG; ++s) {
    const int per = (in.total_tiles + s - 1) / s;
    if (per < 32) break;
    if (forced_ranges && s != forced_ranges) continue;
    const double rounds = (double)(tail_units * s) / cus, whole = floor(rounds);
    double c = (whole + sqrt(rounds - whole)) / s * (1.0 + 6.0 / per) + 0.03;
    if (per >= 128) c *= 1.0 - 0.006 * s;
    if (c < best) { best = c; best_s = s; }
  }
  if (!forced_ranges && best >= base * 0.97) best_s = 0;   // a split must be worth >= 3 % of a round
  return best_s ? Tail16Plan{Tail16::KeyRanges, rows_a, best_s} : kNoTail;
}

// The plan of a call the caller's variant passed decode_request for. have_ws: the caller gave a split workspace (ovg_attn_plan: assumed).
Plan16 plan16(const ovg_attn_params& p, const Request16& rq, bool bf16, bool have_ws) {
  const int cus = (p.cus > 0 && p.cus < cu_count_attn()) ? p.cus : cu_count_attn();   // ovg_attn_params.cus: what RCCL leaves us in the sharded run
  const PlanIn in{p, rq, bf16, have_ws, cus, total_key_tiles(p)};
  const Kernel16 k = choose_kernel(in);
  Plan16 pl{k, in.total_tiles, key_ranges(in.total_tiles, whole_launch_splits(in, k), 0).splits, kNoTail};
  if (pl.splits > 1) return pl;
  pl.tail = row_tail_128(in, k);
  if (pl.tail.kind == Tail16::None) pl.tail = key_tail_256(in, k);
  const Tail16Plan keys512 = key_tail_512(in, k, pl.tail.kind == Tail16::Rows128);
  if (keys512.kind != Tail16::None) pl.tail = keys512;          // where both 512-row rules fire the key ranges win: their model compared the two
  return pl;
}

// The split workspace of a plan, for a q buffer of nq_pad rows per entry: `rows` per (key range, entry) -- the whole padded sequence for a
// whole-launch split (the layout callers of rounds 2-4 sized their buffers for), the tail's own rows padded to its q tile for a key-split
// tail -- as f32 partials [range][entry][rows][64] (ABI 9; bf16 / f16 before) + their log-sum-exps. No split: no bytes.
struct SplitWs16 { int64_t rows, part_bytes, lse_bytes; };
SplitWs16 split_workspace(const ovg_attn_params& p, const Plan16& pl, int64_t nq_pad) {
  const bool key_tail = pl.tail.kind == Tail16::KeyRanges;
  const int bq = q_rows(pl.kernel);
  const int64_t rows = key_tail ? (p.nq - pl.tail.main_rows + bq - 1) / bq * bq : nq_pad;
  const int64_t ranges = key_tail ? pl.tail.ranges : (pl.splits > 1 ? pl.splits : 0);
  return SplitWs16{rows, ranges * p.BH * rows * OVG_D * 4, ranges * p.BH * rows * 4};
}

template <typename T>
int dispatch16(const ovg_attn_params& p, hipStream_t st) {
  if (retired_variant(p.variant)) return OVG_E_UNSUPPORTED;
  Request16 rq;
  if (!decode_request(p.variant, p.kv_splits, &rq)) return OVG_E_ARG;
  const Plan16 pl = plan16(p, rq, std::is_same<T, bf16_t>::value, p.ws_part != nullptr && p.ws_lse != nullptr);
  const SplitWs16 ws = split_workspace(p, pl, p.nq_pad);
  if (ws.part_bytes > 0) {   // the partials go to caller memory: refuse a missing or undersized workspace instead of writing past it
    if (p.ws_part == nullptr || p.ws_lse == nullptr) return OVG_E_ARG;
    if (p.ws_part_bytes < ws.part_bytes || p.ws_lse_bytes < ws.lse_bytes) return OVG_E_ARG;
  }
  const Launch16 main_kernel = launcher<T>(pl.kernel);
  const Pass16 whole = key_ranges(pl.total_tiles, pl.splits, ws.rows);
  if (pl.tail.kind == Tail16::None) return main_kernel(p, whole, st, 0, p.nq);
  const int rc = main_kernel(p, whole, st, 0, pl.tail.main_rows);      // full rounds of the main kernel's tiles, unsplit, then the remaining rows
  if (rc != OVG_OK) return rc;
  if (pl.tail.kind == Tail16::Rows128) return launcher<T>(Kernel16::Spec128)(p, whole, st, pl.tail.main_rows, p.nq);   // as 128-row tiles
  return main_kernel(p, key_ranges(pl.total_tiles, pl.tail.ranges, ws.rows), st, pl.tail.main_rows, p.nq);            // cut along the keys + merge
}

// split-f16 mode (OVG_F16X2): one launch of 256-row tiles -- 8 waves x 2 q blocks, lazy-rescale softmax, a 3-slot LDS-DMA ring of
// [K hi | V^T hi | K lo | V^T lo] tiles (96 KB, one workgroup per CU), three f16 MFMAs per product
constexpr int X3_RING = 3;
constexpr Launch16 x3_exact = launch_attn16<f16_t, 2, 8, 1, X3_RING, 3>;
// OVG_ATTN_F32X_FAST_PV (opt-in, round 6): the PV contraction without its P_lo x V_hi product -- +16 % (64 views: 28.1 -> 32.6 frames/s) at 3e-5 of the f32
// mode at full depth, but 1.0e-4 on the camera token of the 64-view depth-1 parity case: NOT inside the mode's <= 1e-4 contract, so not the default
constexpr Launch16 x3_fast_pv = launch_attn16<f16_t, 2, 8, 1, X3_RING, 2>;
int dispatch_x3(const ovg_attn_params& p, hipStream_t st) {
  const Pass16 unsplit = key_ranges(total_key_tiles(p), 1, p.nq_pad);
  return (p.variant == OVG_ATTN_F32X_FAST_PV ? x3_fast_pv : x3_exact)(p, unsplit, st, 0, p.nq);
}

}  // namespace

extern "C" int ovg_flash_attn(const ovg_attn_params* p, void* stream) {
  if (!p || !p->q || !p->out) return OVG_E_ARG;
  if (p->nq <= 0 || p->nq_pad < p->nq || p->BH <= 0 || p->nseg < 1 || p->nseg > OVG_MAX_SEG) return OVG_E_ARG;
  // the kernels hold q rows, keys and key tiles as ints and decode (entry, q tile, key range) from an int block id; byte offsets are 64-bit.
  // nq and every nk below 2^27 (2^21 key tiles per segment, 2^24 over eight segments); at most 2^27 (entry, 64-row tile) units, so that a
  // launch cut into OVG_MAX_SEG key ranges still has fewer than 2^31 workgroups (BH is then below 2^27 as well)
  if (p->nq >= ((int64_t)1 << 27) || p->BH > ((int64_t)1 << 27) || p->BH * ((p->nq + 63) / 64) > (int64_t)1 << 27) return OVG_E_ARG;
  for (int i = 0; i < p->nseg; ++i) {
    const ovg_kv_segment& s = p->seg[i];
    if (!s.k || !s.vt || s.nk <= 0 || s.nk >= ((int64_t)1 << 27) || s.nk_pad % BC != 0 || s.nk_pad < ((s.nk + BC - 1) / BC) * BC) return OVG_E_ARG;
    if ((reinterpret_cast<uintptr_t>(s.k) | reinterpret_cast<uintptr_t>(s.vt)) & 15) return OVG_E_ARG;
  }
  if ((reinterpret_cast<uintptr_t>(p->q) | reinterpret_cast<uintptr_t>(p->out)) & 15) return OVG_E_ARG;
  if (p->lse && (reinterpret_cast<uintptr_t>(p->lse) & 3)) return OVG_E_ARG;
  if (p->fallback_count && (reinterpret_cast<uintptr_t>(p->fallback_count) & 3)) return OVG_E_ARG;
  if (p->kv_splits < 0 || p->kv_splits > OVG_MAX_SEG || p->cus < 0) return OVG_E_ARG;
  if ((p->ws_part && (reinterpret_cast<uintptr_t>(p->ws_part) & 15)) || (p->ws_lse && (reinterpret_cast<uintptr_t>(p->ws_lse) & 3))) return OVG_E_ARG;
  if (p->kv_splits > 1 && (p->dtype == OVG_F32 || p->variant == 1)) return OVG_E_UNSUPPORTED;   // the baseline kernel never splits
  if (p->ldo % 4 || p->kv_heads < 0 || p->out_bh_stride < 0 || (p->out_bh_stride > 0 && (p->ldo < OVG_D || p->out_bh_stride % 4))) return OVG_E_ARG;
  hipStream_t st = static_cast<hipStream_t>(stream);
  switch (p->dtype) {
    case OVG_BF16: return dispatch16<bf16_t>(*p, st);
    case OVG_F16: return dispatch16<f16_t>(*p, st);
    case OVG_F32: return launch_attn<float, 1>(*p, st);
    case OVG_F16X2: {
      if (p->kv_splits > 1 || p->kv_heads > 0 || p->out_bh_stride > 0) return OVG_E_UNSUPPORTED;
      if (!p->q_lo || !p->out_lo || ((reinterpret_cast<uintptr_t>(p->q_lo) | reinterpret_cast<uintptr_t>(p->out_lo)) & 15)) return OVG_E_ARG;
      for (int i = 0; i < p->nseg; ++i)
        if (!p->seg[i].k_lo || !p->seg[i].vt_lo || ((reinterpret_cast<uintptr_t>(p->seg[i].k_lo) | reinterpret_cast<uintptr_t>(p->seg[i].vt_lo)) & 15)) return OVG_E_ARG;
      return dispatch_x3(*p, st);
    }
    default: return OVG_E_DTYPE;
  }
}

extern "C" int ovg_attn_plan(const ovg_attn_params* p, ovg_attn_plan_out* out) {
  if (!p || !out || p->nq <= 0 || p->BH <= 0 || p->nseg < 1 || p->nseg > OVG_MAX_SEG || p->kv_splits < 0 || p->kv_splits > OVG_MAX_SEG) return OVG_E_ARG;
  for (int i = 0; i < p->nseg; ++i)
    if (p->seg[i].nk <= 0) return OVG_E_ARG;
  out->splits = 1; out->q_tile = 64; out->part_bytes = 0; out->lse_bytes = 0; out->main_rows = p->nq; out->tail_q_tile = 0;
  if (p->dtype == OVG_F16X2) { out->q_tile = 256; return OVG_OK; }
  if (p->dtype != OVG_BF16 && p->dtype != OVG_F16) return p->dtype == OVG_F32 ? OVG_OK : OVG_E_DTYPE;
  if (retired_variant(p->variant)) return OVG_E_UNSUPPORTED;   // no plan for a kernel that cannot launch
  Request16 rq;
  if (!decode_request(p->variant, p->kv_splits, &rq)) return OVG_E_ARG;   // not a variant: ovg_flash_attn refuses it too
  const Plan16 pl = plan16(*p, rq, p->dtype == OVG_BF16, true);
  if (pl.kernel == Kernel16::Baseline) return OVG_OK;            // never split: `out` holds its answer
  const SplitWs16 ws = split_workspace(*p, pl, p->nq_pad >= p->nq ? p->nq_pad : ((p->nq + BC - 1) / BC) * BC);
  const bool key_tail = pl.tail.kind == Tail16::KeyRanges;       // `splits` key ranges for the rows [main_rows, nq) only, tail_q_tile == q_tile
  out->splits = key_tail ? pl.tail.ranges : pl.splits; out->q_tile = q_rows(pl.kernel);
  if (pl.tail.kind != Tail16::None) { out->main_rows = pl.tail.main_rows; out->tail_q_tile = key_tail ? q_rows(pl.kernel) : 128; }
  out->part_bytes = ws.part_bytes; out->lse_bytes = ws.lse_bytes;
  return OVG_OK;
}
