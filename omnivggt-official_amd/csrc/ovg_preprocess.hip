// Input preprocessing (visual_util.py:679-845, omnivggt/utils/load_fn.py:53-146 after PIL's convert("RGB")): Pillow's 8-bit bicubic
// resize as two separable integer passes, the crop / white pad and ToTensor into the (S, 3, H, W) f32 model input (ovg_resample_frames),
// and the depth maps' filter + nearest gather + mask (ovg_depth_frames). One launch per pass covers every frame of a call; a block
// owns one row of one frame. The resample path is integer arithmetic only (Pillow's ImagingResampleHorizontal_8bpc /
// ImagingResampleVertical_8bpc), so it is bit-identical to Image.resize whatever the compiler does with floating point.
#include "ovg_common.h"

namespace {

constexpr int kThreads = 256;
constexpr int kPrecisionBits = 22;                  // Pillow: 32 - 8 - 2
constexpr int64_t kMaxSide = 1 << 20;                // any side above this is rejected (keeps every product below 2^63)

OVG_DEV uint32_t clip8(int32_t acc) {
  // Pillow's clip8 on the accumulator that started at 1 << (PRECISION_BITS - 1): arithmetic shift, then clamp
  const int32_t v = acc >> kPrecisionBits;
  return (uint32_t)(v < 0 ? 0 : (v > 255 ? 255 : v));
}

// horizontal pass: source rows [mid_row0, mid_row0 + mid_rows) of frame blockIdx.y -> u8 rows of res_w pixels in ws
__global__ __launch_bounds__(kThreads) void rs_horizontal(const ovg_resample_frame* __restrict__ frames, const uint8_t* __restrict__ src,
                                                          const int32_t* __restrict__ coef, uint8_t* __restrict__ ws) {
  const ovg_resample_frame f = frames[blockIdx.y];
  const int r = blockIdx.x;
  if (f.h_k_off < 0 || r >= f.mid_rows) return;
  const uint8_t* row = src + f.src_off + (int64_t)(f.mid_row0 + r) * f.src_w * 3;
  uint8_t* dst = ws + f.mid_off + (int64_t)r * f.res_w * 3;
  for (int x = threadIdx.x; x < f.res_w; x += kThreads) {
    const int first = coef[f.h_bounds_off + 2 * x];
    const int n = coef[f.h_bounds_off + 2 * x + 1];
    const int32_t* k = coef + f.h_k_off + (int64_t)x * f.h_ksize;
    const uint8_t* s = row + first * 3;
    int32_t a0 = 1 << (kPrecisionBits - 1), a1 = a0, a2 = a0;
    for (int j = 0; j < n; ++j) {
      const int32_t w = k[j];
      a0 += (int32_t)s[3 * j] * w;
      a1 += (int32_t)s[3 * j + 1] * w;
      a2 += (int32_t)s[3 * j + 2] * w;
    }
    dst[3 * x] = (uint8_t)clip8(a0);
    dst[3 * x + 1] = (uint8_t)clip8(a1);
    dst[3 * x + 2] = (uint8_t)clip8(a2);
  }
}

// vertical pass + crop + canvas: canvas row blockIdx.x of frame blockIdx.y. Rows / columns outside the content are the white pad.
template <int FMT>
__global__ __launch_bounds__(kThreads) void rs_vertical(const ovg_resample_frame* __restrict__ frames, const uint8_t* __restrict__ src,
                                                        const int32_t* __restrict__ coef, const uint8_t* __restrict__ ws,
                                                        const float* __restrict__ lut, void* __restrict__ out) {
  __shared__ float tab[256];
  if (FMT == OVG_RS_F32_CHW) {
    tab[threadIdx.x] = lut[threadIdx.x];             // kThreads == 256
    __syncthreads();
  }
  const ovg_resample_frame f = frames[blockIdx.y];
  const int y = blockIdx.x;
  if (y >= f.canvas_h) return;
  const int64_t plane = (int64_t)f.canvas_h * f.canvas_w;
  const int yy = y - f.pad_top;
  const bool row_in = yy >= 0 && yy < f.out_h;
  const int i = f.crop_y + yy;                       // resized row
  int first = 0, n = 0;
  const int32_t* k = coef;
  const uint8_t* base = src;
  if (row_in) {
    first = coef[f.v_bounds_off + 2 * i];
    n = coef[f.v_bounds_off + 2 * i + 1];
    k = coef + f.v_k_off + (int64_t)i * f.v_ksize;
    base = f.h_k_off >= 0 ? ws + f.mid_off + (int64_t)(first - f.mid_row0) * f.res_w * 3 : src + f.src_off + (int64_t)first * f.res_w * 3;
  }
  const int64_t stride = (int64_t)f.res_w * 3;
  for (int x = threadIdx.x; x < f.canvas_w; x += kThreads) {
    const int xx = x - f.pad_left;
    uint32_t v0 = 255, v1 = 255, v2 = 255;
    const bool in = row_in && xx >= 0 && xx < f.res_w;
    if (in) {
      const uint8_t* s = base + xx * 3;
      int32_t a0 = 1 << (kPrecisionBits - 1), a1 = a0, a2 = a0;
      for (int j = 0; j < n; ++j, s += stride) {
        const int32_t w = k[j];
        a0 += (int32_t)s[0] * w;
        a1 += (int32_t)s[1] * w;
        a2 += (int32_t)s[2] * w;
      }
      v0 = clip8(a0);
      v1 = clip8(a1);
      v2 = clip8(a2);
    }
    if (FMT == OVG_RS_F32_CHW) {
      float* o = static_cast<float*>(out) + f.canvas_off + (int64_t)y * f.canvas_w + x;
      o[0] = in ? tab[v0] : 1.0f;                    // the reference pads the float tensor with exactly 1.0
      o[plane] = in ? tab[v1] : 1.0f;
      o[2 * plane] = in ? tab[v2] : 1.0f;
    } else {
      uint8_t* o = static_cast<uint8_t*>(out) + f.canvas_off + ((int64_t)y * f.canvas_w + x) * 3;
      o[0] = (uint8_t)v0;
      o[1] = (uint8_t)v1;
      o[2] = (uint8_t)v2;
    }
  }
}

// depth: row blockIdx.x of frame blockIdx.y; the reference's three filter steps in its order, then the gather and the mask
__global__ __launch_bounds__(kThreads) void depth_gather(const ovg_depth_frame* __restrict__ frames, const float* __restrict__ src,
                                                         const int32_t* __restrict__ index, float max_depth, float* __restrict__ depth,
                                                         float* __restrict__ mask) {
  const ovg_depth_frame f = frames[blockIdx.y];
  const int y = blockIdx.x;
  if (y >= f.out_h) return;
  const float* row = src + f.src_off + (int64_t)index[f.rows_off + y] * f.src_w;
  const int64_t o = f.out_off + (int64_t)y * f.out_w;
  for (int x = threadIdx.x; x < f.out_w; x += kThreads) {
    float d = row[index[f.cols_off + x]];
    if (!__builtin_isfinite(d)) d = 0.0f;
    if (d > max_depth) d = 0.0f;
    if (d < 1e-5f) d = 0.0f;
    depth[o + x] = d;
    mask[o + x] = d > 1e-5f ? 1.0f : 0.0f;
  }
}

bool side_ok(int64_t v) { return v >= 1 && v <= kMaxSide; }

// every (first, count) pair of rows [i0, i1) of a table lies in [lo, hi) with 1 <= count <= ksize
bool taps_ok(const int32_t* coef, int64_t len, int32_t bounds_off, int32_t k_off, int32_t ksize, int64_t i0, int64_t i1, int64_t lo, int64_t hi) {
  if (bounds_off < 0 || k_off < 0 || ksize < 1 || ksize > kMaxSide) return false;
  if (bounds_off + 2 * i1 > len || k_off + i1 * ksize > len) return false;
  for (int64_t i = i0; i < i1; ++i) {
    const int64_t first = coef[bounds_off + 2 * i], n = coef[bounds_off + 2 * i + 1];
    if (n < 1 || n > ksize || first < lo || first + n > hi) return false;
  }
  return true;
}

bool frame_ok(const ovg_resample_frame& f, const ovg_resample_params& p) {
  if (!side_ok(f.src_w) || !side_ok(f.src_h) || !side_ok(f.res_w) || !side_ok(f.res_h) || !side_ok(f.canvas_w) || !side_ok(f.canvas_h))
    return false;
  if (f.src_off < 0 || f.src_off + 3 * (int64_t)f.src_w * f.src_h > p.src_bytes) return false;
  if (f.crop_y < 0 || f.out_h < 1 || (int64_t)f.crop_y + f.out_h > f.res_h) return false;
  if (f.pad_top < 0 || f.pad_left < 0 || (int64_t)f.pad_top + f.out_h > f.canvas_h || (int64_t)f.pad_left + f.res_w > f.canvas_w) return false;
  if (f.canvas_off < 0 || f.canvas_off + 3 * (int64_t)f.canvas_h * f.canvas_w > p.out_elems) return false;
  int64_t row_lo = 0, row_hi = f.src_h;
  if (f.h_k_off >= 0) {
    if (!p.ws || f.mid_row0 < 0 || f.mid_rows < 1 || (int64_t)f.mid_row0 + f.mid_rows > f.src_h) return false;
    if (f.mid_off < 0 || f.mid_off + 3 * (int64_t)f.mid_rows * f.res_w > p.ws_bytes) return false;
    if (!taps_ok(p.coef_host, p.coef_len, f.h_bounds_off, f.h_k_off, f.h_ksize, 0, f.res_w, 0, f.src_w)) return false;
    row_lo = f.mid_row0;
    row_hi = (int64_t)f.mid_row0 + f.mid_rows;
  } else if (f.src_w != f.res_w) {
    return false;
  }
  return taps_ok(p.coef_host, p.coef_len, f.v_bounds_off, f.v_k_off, f.v_ksize, f.crop_y, (int64_t)f.crop_y + f.out_h, row_lo, row_hi);
}

}  // namespace

extern "C" int64_t ovg_resample_workspace_bytes(const ovg_resample_frame* frames_host, int32_t nframes) {
  if (!frames_host || nframes < 1) return -1;
  int64_t need = 0;
  for (int32_t i = 0; i < nframes; ++i) {
    const ovg_resample_frame& f = frames_host[i];
    if (f.h_k_off < 0) continue;
    if (f.mid_off < 0 || f.mid_rows < 0 || !side_ok(f.res_w) || f.mid_rows > kMaxSide) return -1;
    const int64_t end = f.mid_off + 3 * (int64_t)f.mid_rows * f.res_w;
    need = end > need ? end : need;
  }
  return need;
}

extern "C" int ovg_resample_frames(const ovg_resample_params* p, void* stream) {
  if (!p || !p->frames || !p->frames_host || !p->src || !p->coef || !p->coef_host || !p->out) return OVG_E_ARG;
  if (p->nframes < 1 || p->nframes > 65535 || p->src_bytes < 3 || p->coef_len < 1 || p->out_elems < 1 || p->ws_bytes < 0) return OVG_E_ARG;
  if (p->out_format != OVG_RS_F32_CHW && p->out_format != OVG_RS_U8_HWC) return OVG_E_ARG;
  if (p->out_format == OVG_RS_F32_CHW && !p->lut) return OVG_E_ARG;
  int32_t max_mid = 0, max_canvas = 0;
  for (int32_t i = 0; i < p->nframes; ++i) {
    const ovg_resample_frame& f = p->frames_host[i];
    if (!frame_ok(f, *p)) return OVG_E_ARG;
    if (f.h_k_off >= 0 && f.mid_rows > max_mid) max_mid = f.mid_rows;
    if (f.canvas_h > max_canvas) max_canvas = f.canvas_h;
  }
  hipStream_t st = static_cast<hipStream_t>(stream);
  if (max_mid > 0) {
    OVG_LAUNCH(rs_horizontal, dim3(max_mid, p->nframes), dim3(kThreads), 0, st, p->frames, p->src, p->coef, p->ws);
    OVG_CHECK_LAUNCH();
  }
  if (p->out_format == OVG_RS_F32_CHW)
    OVG_LAUNCH(rs_vertical<OVG_RS_F32_CHW>, dim3(max_canvas, p->nframes), dim3(kThreads), 0, st, p->frames, p->src, p->coef, p->ws, p->lut, p->out);
  else
    OVG_LAUNCH(rs_vertical<OVG_RS_U8_HWC>, dim3(max_canvas, p->nframes), dim3(kThreads), 0, st, p->frames, p->src, p->coef, p->ws, p->lut, p->out);
  OVG_CHECK_LAUNCH();
  return OVG_OK;
}

extern "C" int ovg_depth_frames(const ovg_depth_params* p, void* stream) {
  if (!p || !p->frames || !p->frames_host || !p->src || !p->index || !p->index_host || !p->depth || !p->mask) return OVG_E_ARG;
  if (p->nframes < 1 || p->nframes > 65535 || p->src_elems < 1 || p->index_len < 1 || p->out_elems < 1) return OVG_E_ARG;
  int32_t max_h = 0;
  for (int32_t i = 0; i < p->nframes; ++i) {
    const ovg_depth_frame& f = p->frames_host[i];
    if (!side_ok(f.src_w) || !side_ok(f.src_h) || !side_ok(f.out_w) || !side_ok(f.out_h)) return OVG_E_ARG;
    if (f.src_off < 0 || f.src_off + (int64_t)f.src_w * f.src_h > p->src_elems) return OVG_E_ARG;
    if (f.out_off < 0 || f.out_off + (int64_t)f.out_w * f.out_h > p->out_elems) return OVG_E_ARG;
    if (f.rows_off < 0 || f.cols_off < 0 || (int64_t)f.rows_off + f.out_h > p->index_len || (int64_t)f.cols_off + f.out_w > p->index_len)
      return OVG_E_ARG;
    for (int32_t y = 0; y < f.out_h; ++y)
      if (p->index_host[f.rows_off + y] < 0 || p->index_host[f.rows_off + y] >= f.src_h) return OVG_E_ARG;
    for (int32_t x = 0; x < f.out_w; ++x)
      if (p->index_host[f.cols_off + x] < 0 || p->index_host[f.cols_off + x] >= f.src_w) return OVG_E_ARG;
    if (f.out_h > max_h) max_h = f.out_h;
  }
  hipStream_t st = static_cast<hipStream_t>(stream);
  OVG_LAUNCH(depth_gather, dim3(max_h, p->nframes), dim3(kThreads), 0, st, p->frames, p->src, p->index, p->max_depth, p->depth, p->mask);
  OVG_CHECK_LAUNCH();
  return OVG_OK;
}
