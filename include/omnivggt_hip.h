/*
 * omnivggt_hip.h -- C ABI of libomnivggt_hip.so (gfx950 / MI355X).
 *
 * Drop-in boundary for the OmniVGGT multi-view aggregator hot path
 * (reference: omnivggt/models/omnivggt_aggregator.py:130-305,
 * omnivggt/models/aggregator.py:312-341, omnivggt/layers/{block,attention,
 * mlp,rope,patch_embed,vision_transformer}.py).  The reference has no FFI of
 * its own (pure PyTorch); each entry below names the reference call site it
 * replaces.  See INTEGRATION.md for the ctypes binding a maintainer would add.
 *
 * Conventions (all entries):
 *   - `int fn(const <params>*, void* hip_stream)`; returns OVG_OK (0) or a
 *     negative OVG_E_* code.  Never throws, never allocates or frees, never
 *     synchronises the device.
 *   - every pointer is a DEVICE pointer owned by the caller and must stay valid
 *     until the stream reaches the call; 16-byte aligned unless noted.
 *   - `dtype` selects the storage/MFMA input type of activations and weights:
 *     OVG_BF16 / OVG_F16 (throughput modes, f32 accumulate), OVG_F32
 *     (parity mode, exact-f32 MFMA) or OVG_F16X2 (split-f16 parity mode, see the enum).  The residual stream, LayerNorm
 *     statistics, softmax statistics, biases, LayerScale gammas, q/k-norm
 *     affine parameters and the RoPE table are always f32.
 *   - thread-safe for distinct streams; the library holds NO mutable state: every tuning choice is either
 *     derived from the call's shapes or passed in the parameter struct (`tile`, `variant`). The one thing it remembers is which
 *     kernels it has already opted in to > 64 KB of dynamic LDS on which device: an idempotent memo, read and written under a lock.
 *   - workspace is caller-provided; ovg_block_workspace_bytes() answers how much a block call needs.
 */
#ifndef OMNIVGGT_HIP_H
#define OMNIVGGT_HIP_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* ABI history
 * 2: + DPT-head entries (ovg_head_layernorm, ovg_conv, ovg_upsample, ovg_dpt_out) and ovg_unproject
 * 3: + head-parallel sharding (ovg_attn_params.kv_heads / out_bh_stride, ovg_block_params.skip_attention, ovg_heads_to_tokens)
 * 4: per-call GEMM tile selector (`tile`) replacing the process-global debug setter of ABI 3, optional
 *    log-sum-exp output of ovg_flash_attn + ovg_attn_merge (two-launch local-first sharded attention),
 *    ovg_block_workspace_bytes, ovg_pack_weights, split-KV attention (kv_splits / ws_part / ws_lse, ovg_attn_plan)
 * 5-6: camera head entry; 16-bit V^T rows in the PV fragment order (LDS-DMA staged attention)
 * 7: split-KV workspace SIZES travel with the pointers (ws_part_bytes / ws_lse_bytes: an undersized workspace is OVG_E_ARG
 *    instead of an out-of-bounds write), ovg_camera_tables (camera-modality injection tables built on the device), OVG_F32 in the DPT-head
 *    entries, ovg_attn_plan_out.main_rows / tail_q_tile (the tail split of long attention launches is part of the queryable plan)
 * 8: OVG_F16X2 -- the split-f16 compute mode ("f32x": every 16-bit operand tensor is a PAIR of f16 planes hi + lo, products run as
 *    three f16 MFMAs hi*hi + hi*lo + lo*hi with f32 accumulation: ~2^-22 per product instead of 2^-8 (bf16) / 2^-11 (f16) at
 *    a third of the 16-bit MFMA rate; the `*_lo` pointers below, NULL / ignored for the other dtypes; single GPU and the K / V^T
 *    all-gather sharded form incl. ovg_attn_merge);
 *    ovg_attn_params.fallback_count / ovg_block_params.attn_fallback_count (telemetry of the speculative bf16 softmax)
 * 9: split-KV partials are f32 (ovg_attn_plan_out.part_bytes doubles) and a launch may split only the rows beyond its last full round
 *    along the keys (key-split tail, reported through main_rows / tail_q_tile); OVG_TILE_256P / OVG_TILE_DMA_M name the round-5 lab GEMM
 *    forms (OVG_E_UNSUPPORTED unless the library was built with -DOVG_LAB_GEMM)
 * 10: ovg_dpt_tail -- the output stage of the DPT head (upsample + position embedding + conv3x3 + ReLU + conv1x1 + activation) as one launch
 * 11: the lab GEMM selectors of ABI 9 (OVG_TILE_256P / OVG_TILE_DMA_M) are removed (OVG_E_ARG); the key-split tail of ABI 9 now also follows
 *     the 512-row attention launches (ovg_attn_plan_out: q_tile == tail_q_tile == 512, splits = key ranges of the tail rows, partials sized
 *     for the tail rows) when the caller passes a split workspace
 * 12: + point-cloud extraction (ovg_percentile, ovg_point_filter and their *_workspace_bytes queries)
 * 13: + input preprocessing (ovg_resample_frames, ovg_depth_frames, ovg_resample_workspace_bytes)
 *     + voxel-grid decimation (ovg_voxel_downsample, ovg_voxel_downsample_workspace_bytes): entries added, nothing existing changed,
 *       so the number stays; a binding looks the two symbols up by name and reports a library that predates them
 *     + point-cloud rendering (ovg_render_points, ovg_render_workspace_bytes): added the same way, looked up by name
 *     + multi-view depth consistency (ovg_multiview_consistency, ovg_consistency_workspace_bytes): added the same way
 *     + nearest-neighbour search between point clouds (ovg_nearest_neighbours, ovg_nn_workspace_bytes): added the same way
 *     + farthest-point sampling of point clouds (ovg_farthest_point_sample, ovg_fps_workspace_bytes): added the same way
 *     + radius neighbour search on a hash grid (ovg_radius_search, ovg_radius_workspace_bytes): added the same way
 *     + k nearest neighbours within a radius on that grid, and PCA normals from the table (ovg_knn_search, ovg_knn_normals): added
 *       the same way
 *     + clustering on that grid: Euclidean connected components and DBSCAN (ovg_cluster): added the same way
 *     + plane segmentation by RANSAC (ovg_plane_hypotheses, ovg_plane_score, ovg_plane_select, ovg_plane_mask, ovg_plane_fit): added
 *       the same way
 *     + volumetric fusion: depth maps into a TSDF volume and a surface-nets mesh of its zero level (ovg_tsdf_integrate,
 *       ovg_tsdf_extract, ovg_tsdf_extract_workspace_bytes): added the same way
 *     + mesh rasterisation: z-buffered, shaded triangles (ovg_render_mesh, ovg_render_mesh_workspace_bytes): added the same way
 *     + depth evaluation: masked per-group medians, aligned metric sums and the alignment solve (ovg_deptheval_median,
 *       ovg_deptheval_sums, ovg_deptheval_solve, ovg_deptheval_median_workspace_bytes, ovg_deptheval_sums_workspace_bytes): added the
 *       same way
 *     + image-space map geometry: usable depth, normals, edge flags and the grid mesh of the prediction maps (ovg_map_depth,
 *       ovg_map_normals, ovg_map_edges, ovg_map_triangulate, ovg_map_triangulate_workspace_bytes): added the same way
 *     + mesh simplification by vertex clustering on the grid of ovg_voxel_downsample, duplicate faces merged (ovg_mesh_simplify,
 *       ovg_mesh_simplify_workspace_bytes): added the same way
 *     + mesh cleaning: connected components and edge statistics, ordered sub-meshes, Laplacian / Taubin smoothing (ovg_mesh_topology,
 *       ovg_mesh_select, ovg_mesh_smooth and their *_workspace_bytes queries): added the same way
 *     + weighted, robust registration and moving a prediction into another frame, for stitching chunks of a long sequence
 *       (ovg_align_wmoments, ovg_align_wmoments_workspace_bytes, ovg_align_wsolve, ovg_align_move_maps, ovg_align_move_cameras):
 *       added the same way */
#define OVG_ABI_VERSION 13

enum { OVG_BF16 = 0, OVG_F16 = 1, OVG_F32 = 2,
       /* split-f16 ("f32x", the <= 1e-4 mode with throughput): a value x is stored as hi = f16(x) (saturated at +-65504) in the tensor the
        * ordinary pointer names and lo = f16(x - hi) in a second f16 tensor of the same shape / strides named by the matching `*_lo` pointer.
        * x ~ hi + lo to 2^-22 relative (|x| >= 2^-3; absolute 2^-25 below, where lo is an f16 subnormal). A GEMM / attention contraction over
        * such operands is hi*hi + hi*lo + lo*hi on the f16 MFMA (f16 x f16 products are exact in f32) with f32 accumulation, the dropped
        * lo*lo term is 2^-22 relative. Everything that is f32 in the other modes stays f32. */
       OVG_F16X2 = 3 };

enum {
  OVG_OK = 0,
  OVG_E_ARG = -1,      /* null pointer / bad shape / misalignment            */
  OVG_E_DTYPE = -2,    /* unsupported dtype                                   */
  OVG_E_LAUNCH = -3,   /* hipGetLastError() != hipSuccess after a launch      */
  OVG_E_UNSUPPORTED = -4
};

/* Model constants of the path (omnivggt_aggregator.py:19-37). */
#define OVG_C 1024      /* embed dim            */
#define OVG_H 16        /* heads                */
#define OVG_D 64        /* head dim             */
#define OVG_HID 4096    /* MLP hidden           */
#define OVG_KV_TILE 64  /* key tile: K/V^T buffers are padded to this */
#define OVG_MAX_SEG 8   /* K/V segments per attention call (= ranks)  */

int ovg_abi_version(void);
/* human readable build string (static storage) */
const char* ovg_build_info(void);

/* ------------------------------------------------------------------ *
 * LayerNorm over rows of 1024 (nn.LayerNorm: block.py:50,67 norm1/norm2,
 * vision_transformer.py:264 final DINO norm).  x is the f32 residual
 * stream with row stride ldx (elements); y is [rows,1024] in `dtype`
 * (out_f32 != 0: y is f32 regardless of dtype).
 *
 * Size limits of the model-path entries (this one to ovg_unproject, and ovg_camera_head): every byte offset a kernel forms from a row,
 * pixel, head or image index and a stride is 64-bit unless the entry's "Size limits" paragraph says otherwise, and what it says otherwise
 * is checked on the host: a call beyond it is refused (or, where stated, served by another kernel), never wrapped. Counts are int64_t in
 * the structs; a kernel that holds one as an int says so below. The limits that remain are memory, not arithmetic
 * (tests/test_gpu_address_range.py runs every strided operand 16 MiB per row apart and the dense ones past 4 GiB / 2^31 elements).
 * Size limits: none beyond rows > 0 (ldx, ldy multiples of 4 elements, 16-byte aligned pointers); the grid is capped at 8192 blocks of
 * four rows and strides over the rest.
 * ------------------------------------------------------------------ */
typedef struct {
  const float* x; int64_t ldx;
  void* y; int64_t ldy;
  const float* weight; const float* bias;
  int64_t rows; float eps; int dtype; int out_f32;
  void* y_lo;                    /* OVG_F16X2: lo plane of y (same ldy) */
} ovg_layernorm_params;
int ovg_layernorm(const ovg_layernorm_params*, void* stream);

/* ------------------------------------------------------------------ *
 * Generic linear  Y = epilogue(X @ W^T + bias)   (nn.Linear / addmm).
 * X [M,K] ld=ldx, W [N,K] ld=ldw, both `dtype`, K a multiple of 64.
 * epilogue:
 *   OVG_EPI_STORE : y[m,n] = acc + bias               (y dtype, or f32 if out_f32)
 *   OVG_EPI_GELU  : y[m,n] = gelu_erf(acc + bias)     (mlp.py:35-36)
 *   OVG_EPI_RES   : y_f32[m,n] = res_f32[m,n] + gamma[n]*(acc+bias)
 *                   (+ inject[(m/inj_period),n] when m % inj_period == 0)
 *                   (attention.py:75 + layer_scale.py:27 + block.py:105-106,
 *                    omnivggt_aggregator.py:284-301 camera injection)
 *   OVG_EPI_PATCH : y_f32[(m/p0)*p1 + off + m%p0, n] = acc + bias + table[(m%p0)+1, n]
 *                   (patch_embed.py:75-77 + vision_transformer.py:220-224)
 * Size limits (each a host check; OVG_E_ARG unless noted): 0 < M <= 2^30 rows; N a multiple of 128, K of 64; ldx, ldw multiples of 16
 * bytes, ldy / ldres of 4 elements. The epilogues divide the row index by p0 (PATCH) and inj_period (RES with inject) with a corrected
 * float estimate that is exact while the quotient stays below 2^22: (M - 1) / p0 and (M - 1) / inj_period must, and both periods must
 * be below 2^31. The 256 x 256 tile addresses the rows of a tile as 32-bit byte offsets from the tile's first row: it needs
 * 0 <= ldx, ldw <= 8 421 504 elements (255 ld 2 + 64 <= 2^32; 16.06 MiB per row). Beyond that OVG_TILE_AUTO runs the 128 x 128 tile
 * (64-bit row pointers, any stride) and a forced OVG_TILE_256 is OVG_E_UNSUPPORTED. y, res and the 128 x 128 tile's x / w take any stride.
 * ------------------------------------------------------------------ */
enum { OVG_EPI_STORE = 0, OVG_EPI_GELU = 1, OVG_EPI_RES = 2, OVG_EPI_PATCH = 3 };
/* workgroup tile of the GEMM kernels: 128 x 128 (4 waves, register-staged, up to 3 workgroups per CU) or 256 x 256 (8 waves, 4-slot LDS-DMA
 * ring, software-pipelined "free-running" main loop with one barrier per k-stage, 1 workgroup per CU, 16-bit dtypes, N % 256 == 0);
 * AUTO picks by shape (ovg_gemm.hip: choose_256). ABI 11: the round-5 lab selectors (4 = persistent 256 x 256, 8 = DMA-in-M flag) are gone --
 * any other value is OVG_E_ARG. */
enum { OVG_TILE_AUTO = 0, OVG_TILE_128 = 1, OVG_TILE_256 = 2,
       /* retired selectors (the r02 epilogue forms of the A/B history; their kernels left the tree, measurements under profiles/): ovg_linear
        * and ovg_qkv answer OVG_E_UNSUPPORTED to any tile with the OVG_TILE_R02_EPILOGUE bit set */
       OVG_TILE_R02_EPILOGUE = 16, OVG_TILE_128X = 17, OVG_TILE_256X = 18 };
typedef struct {
  const void* x; int64_t ldx;
  const void* w; int64_t ldw;
  const float* bias;             /* [N] or NULL */
  void* y; int64_t ldy;
  int64_t M; int64_t N; int64_t K;
  int dtype; int epilogue; int out_f32;
  /* RES */
  const float* res; int64_t ldres; const float* gamma;
  const float* inject; int64_t inj_period;   /* inject may be NULL */
  /* PATCH */
  const float* table; int64_t p0; int64_t p1; int64_t row_off;
  int tile;   /* OVG_TILE_AUTO (shape heuristic), OVG_TILE_128 or OVG_TILE_256 (16-bit dtypes, N % 256 == 0); an impossible request is OVG_E_ARG */
  /* OVG_F16X2: lo planes of x / w (same ldx / ldw) and, for 16-bit outputs (STORE / GELU without out_f32), of y (same ldy) */
  const void* x_lo; const void* w_lo; void* y_lo;
} ovg_linear_params;
int ovg_linear(const ovg_linear_params*, void* stream);

/* ------------------------------------------------------------------ *
 * Fused QKV projection (attention.py:52-58): qkv = X @ Wqkv^T + b, then per
 * head LayerNorm(64) on q,k (if qk_norm), 2-D RoPE on q,k (if rope),
 * q *= q_scale, and head-major stores:
 *   q  [B*H, nq_pad, 64]     k [B*H, nk_pad, 64]     vt [B*H, 64, nk_pad]
 * Row m of X is token n = m % seq of batch b = m / seq; RoPE positions are
 * derived from t = m % tokens_per_view: t < 5 -> (0,0) else
 * (1 + (t-5)/grid_w, 1 + (t-5)%grid_w)   (omnivggt_aggregator.py:215-224).
 * rope_cos/rope_sin: f32 [max_pos,16] (rope.py:86-117, 16 unique freqs), max_pos <= 128 (staged in LDS).
 * Padding rows/cols of q,k,vt are never written (caller zero-fills once).
 * Column order of a vt row (ABI 6). OVG_F32: natural (column n = key n). OVG_BF16 / OVG_F16: inside every block of 32 keys
 * column 8 g + 4 h + i holds key 16 h + 4 g + i (g < 4, h < 2, i < 4) -- each 16-byte chunk is then exactly the B^T fragment
 * of one lane group of the PV MFMA, so the attention kernels move K / V^T tiles global -> LDS by LDS-DMA (no register pass)
 * and read a fragment with one ds_read_b128. ovg_qkv writes this order and ovg_flash_attn expects it; the permutation is
 * local to 32-key blocks, so slicing / exchanging vt buffers at 64-key granularity (segments, ranks, heads) is unaffected.
 * Size limits (host checks, OVG_E_ARG unless noted): 0 < M <= 2^30 rows, M % seq == 0; (M - 1) / seq and, with rope,
 * (M - 1) / tokens_per_view below 2^22 and tokens_per_view below 2^31 (the epilogue's row-index divisions, as in ovg_linear);
 * nq_pad, nk_pad >= seq, nk_pad % 64 == 0; max_pos <= 128. x takes a row stride: the 128 x 128 tile any, the 256 x 256 tile
 * 0 <= ldx <= 8 421 504 elements (AUTO falls back to 128 beyond, a forced OVG_TILE_256 is OVG_E_UNSUPPORTED); w, q, k, vt are dense,
 * their offsets 64-bit (BH n_pad 64 elements may pass 2^31).
 * ------------------------------------------------------------------ */
typedef struct {
  const void* x; int64_t ldx;       /* [M,1024] dtype */
  const void* w;                    /* [3072,1024] dtype */
  const float* bias;                /* [3072] */
  void* q; void* k; void* vt;
  int64_t M; int64_t seq; int64_t nq_pad; int64_t nk_pad;
  int dtype;
  int qk_norm; const float* qn_w; const float* qn_b; const float* kn_w; const float* kn_b; float qk_eps;
  int rope; const float* rope_cos; const float* rope_sin; int max_pos;
  int64_t tokens_per_view; int grid_w; int n_special;
  float q_scale;
  int part;   /* 0 = q,k,v; 1 = k and v only; 2 = q only (sharded path: K/V first, all-gather || Q) */
  int tile;   /* OVG_TILE_* as in ovg_linear_params */
  /* OVG_F16X2: lo planes (same shapes / strides as their hi tensors) */
  const void* x_lo; const void* w_lo; void* q_lo; void* k_lo; void* vt_lo;
} ovg_qkv_params;
int ovg_qkv(const ovg_qkv_params*, void* stream);

/* ------------------------------------------------------------------ *
 * Flash attention forward, D=64, no mask, non-causal
 * (F.scaled_dot_product_attention, attention.py:61-66).  q must already be
 * multiplied by softmax_scale*log2(e) (ovg_qkv does it): the kernel uses
 * exp2.  K/V^T arrive as `nseg` segments (1 on a single GPU; one per rank
 * after the view-sharded all-gather) -- softmax runs across all of them.
 *   q   [BH, nq_pad, 64]
 *   seg[i].k [BH, nk_pad_i, 64], seg[i].vt [BH, 64, nk_pad_i] (16-bit: columns in the ovg_qkv order above), nk_i valid keys
 *   out [B*nq, H*64] token-major (row = (bh/H)*nq + n, col = (bh%H)*64 + d), ld = ldo
 * Size limits (host checks, OVG_E_ARG): the kernels hold query rows, keys and key tiles as ints and decode (entry, q tile, key range)
 * from an int block index: 0 < nq < 2^27, every 0 < nk < 2^27, BH <= 2^27 and BH * ceil(nq / 64) <= 2^27 (a launch cut into
 * OVG_MAX_SEG key ranges then has at most 2^30 workgroups); nk_pad % 64 == 0, ldo % 4 == 0. Every byte offset into q, k, vt, out, lse
 * and the split workspace is 64-bit: BH nq_pad 128 B and ldo may pass 4 GiB.
 * ------------------------------------------------------------------ */
typedef struct { const void* k; const void* vt; int64_t nk; int64_t nk_pad;
                 const void* k_lo; const void* vt_lo;   /* OVG_F16X2: lo planes of k / vt (same shapes) */
} ovg_kv_segment;
/* ovg_attn_params.variant (the numbers are the ones of the A/B logs under profiles/). 0 is what the model runs; the others are for
 * benchmarks, the A/B tools and the tests. */
#define OVG_ATTN_AUTO 0               /* the launch plan chooses: bf16 -> speculative kernel, q tile (128 / 256 / 512 rows), split and tail by shape;
                                       * f16 -> lazy-rescale kernel (256-row tiles from 4096 rows on, else 128); f32 / split-f16: one kernel each */
#define OVG_ATTN_BASELINE 1           /* baseline kernel, every dtype (the f32 parity path, the in-process reference of the tests); never splits */
#define OVG_ATTN_SPEC256 50           /* speculative-softmax kernel, 256-row q tiles (4 waves, 3-slot ring): the bf16 default for short launches */
#define OVG_ATTN_LAZY256 52           /* lazy-rescale kernel, 256-row q tiles: the f16 default from 4096 rows on */
#define OVG_ATTN_FORCED256 53         /* the 256-row speculative kernel with its fallback forced (tests) */
#define OVG_ATTN_SPEC128 54           /* speculative kernel, 128-row q tiles: bf16 launches the smaller tile pads or quantises better */
#define OVG_ATTN_LAZY128 55           /* lazy-rescale kernel, 128-row q tiles: the f16 default below 4096 rows */
#define OVG_ATTN_SPEC512 57           /* speculative kernel, 512-row q tiles (8 waves, 5-slot ring): the bf16 default from 2.5 rounds of them on */
/* plan knobs of the A/B tools and the tests: a kernel + one plan rule allowed outside the default plan */
#define OVG_ATTN_PLAN_ROWTAIL512 71   /* SPEC512 with the rule of its 128-row tail */
#define OVG_ATTN_PLAN_ROWTAIL256 72   /* SPEC256 with a 128-row tail from one full round on (the default wants exactly one) */
#define OVG_ATTN_PLAN_KEYTAIL256 73   /* SPEC256 with a key-split tail whenever a last round is left; kv_splits s > 1 = exactly s key ranges */
#define OVG_ATTN_PLAN_KEYTAIL512 74   /* SPEC512 with its key-split tail rule alone; kv_splits s > 1 = exactly s key ranges */
#define OVG_ATTN_F32X_FAST_PV 92      /* OVG_F16X2 only (opt-in): the PV contraction without its P_lo x V_hi product (+16 %, up to 1.0e-4 on single rows) */
/* Retired (the A/B history of rounds 1-4; OVG_E_UNSUPPORTED from ovg_flash_attn and ovg_attn_plan): 2, 6, 8, 18, 19, 21, 25, 31, 32, 33, 51, 56,
 * 58, 59. Any other number is OVG_E_ARG from both. All of this for the 16-bit dtypes: OVG_F32 runs the baseline kernel and OVG_F16X2 its one
 * kernel (92 aside) whatever the number. */
typedef struct {
  const void* q; int64_t nq; int64_t nq_pad;
  ovg_kv_segment seg[OVG_MAX_SEG]; int nseg;
  void* out; int64_t ldo;
  int64_t BH; int dtype;
  int variant;   /* OVG_ATTN_* above; 0 = OVG_ATTN_AUTO */
  /* head-parallel (all-to-all) sharding, both 0 otherwise:
   *   kv_heads > 0: K / V^T segments hold kv_heads heads; batch entry bh reads head bh % kv_heads (the BH entries
   *                 are (source rank, head) pairs of queries that share this rank's heads);
   *   out_bh_stride > 0: head-major output, out + bh * out_bh_stride + q * ldo + d (ldo >= 64) instead of the
   *                 token-major row (bh / 16) * nq + q, column (bh % 16) * 64 + d. */
  int kv_heads; int64_t out_bh_stride;
  /* optional f32 [BH, nq_pad]: lse[bh, q] = log2(sum_k exp2(s[q, k])) over the keys of THIS call (s = the
   * pre-scaled logits). With it, two calls over disjoint key sets are combined exactly by ovg_attn_merge --
   * the view-sharded all-gather path runs the local keys while the remote ones are still in flight. */
  float* lse;
  /* Split-KV (16-bit dtypes): a launch whose (batch entry, q tile) units do not fill the chip evenly -- 688 workgroups
   * on 512 resident slots at 8 views, the same per rank of an 8-GPU run -- is cut along the KEY axis into kv_splits
   * passes per unit; every pass writes a normalised partial result + its log-sum-exp into the caller's workspace and
   * a second (tiny) launch combines them exactly. kv_splits: 0 = the library decides (ovg_attn_plan; never splits
   * when ws_part / ws_lse are NULL), 1 = never, 2..8 = force. ws_part: `part_bytes`, ws_lse: `lse_bytes` of ovg_attn_plan.
   * Units of one (batch entry, split) run next to each other, so the K / V^T range an XCD streams shrinks by kv_splits.
   * ws_part_bytes / ws_lse_bytes: sizes of the two buffers; a call whose plan needs more than it was given is OVG_E_ARG.
   * ABI 9: the partials are f32 (normalised O per key range + its log-sum-exp: a split launch now agrees with the unsplit one to ~1e-6
   * before the final rounding; the 16-bit partials of ABI <= 8 were 6.9e-3 apart), so part_bytes doubled; and with kv_splits == 0 a launch
   * with a fractional last round may run its full rounds unsplit and only the remaining rows cut along the keys ("key-split tail":
   * ovg_attn_plan_out.main_rows < nq with tail_q_tile == q_tile), whose workspace covers those rows only. */
  int kv_splits; void* ws_part; float* ws_lse; int64_t ws_part_bytes; int64_t ws_lse_bytes;
  /* OVG_F16X2: lo planes of q and out (same shapes / strides). That mode runs one launch of 256-row tiles: no split-KV, no kv_heads /
   * head-major output (OVG_E_UNSUPPORTED), lse is available. */
  const void* q_lo; void* out_lo;
  /* Telemetry of the speculative softmax (OVG_BF16 default kernels): optional DEVICE counter; every workgroup whose speculative pass
   * failed its verification and re-ran with the lazy-rescale body adds 1 (one atomic per such workgroup; nothing is written otherwise,
   * the caller zeroes it). The counter says how often the fast path did not pay: a workgroup that re-ran returns the lazy-rescale result, one
   * that did not returns the speculative pass's, accepted by its row-sum / finiteness check (and, for the order-pinned bf16 body, by the
   * build-time disassembly guard of build.py). NULL = not counted. */
  uint32_t* fallback_count;
  /* ABI 9: CUs the launch plan may count on (0 = all the device has). One process per GPU shares its chip with RCCL's kernels in the
   * sharded run -- every channel of an exchange in flight holds a workgroup slot while the attention launch it overlaps runs -- so the q tile,
   * the tail split and the split-KV factor are planned for `cus` CUs instead of quantising against slots that are not there. ovg_attn_plan
   * answers for the same value. */
  int cus;
} ovg_attn_params;
int ovg_flash_attn(const ovg_attn_params*, void* stream);

/* Host-only query: how ovg_flash_attn would run this call with kv_splits == 0 (needs nq, BH, dtype, variant, the
 * segments' nk; pointers are ignored) and how much split workspace the caller should provide for it. */
typedef struct {
  int splits; int q_tile; int64_t part_bytes; int64_t lse_bytes;
  /* tail split of long launches (ABI 7): rows [0, main_rows) of every batch entry run as q_tile-row tiles in a first launch, the rest as
   * tail_q_tile-row tiles in a second one; main_rows == nq and tail_q_tile == 0 when the call is one launch */
  int64_t main_rows; int tail_q_tile;
} ovg_attn_plan_out;
int ovg_attn_plan(const ovg_attn_params*, ovg_attn_plan_out* out);

/* Combine two attention results over disjoint key sets (same queries):
 *   w_a = 2^(lse_a - m), w_b = 2^(lse_b - m), m = max(lse_a, lse_b);  out = (w_a * a + w_b * b) / (w_a + w_b)
 * a, b, out: [rows, 1024] `dtype` token-major (row strides lda / ldb / ldo; out may alias a or b);
 * lse_a, lse_b: f32 [16, n_pad] head-major as written by ovg_flash_attn (row = token n, B = 1).
 * Size limits: 0 < rows <= n_pad; lda, ldb, ldo >= 1024 and multiples of 4 elements, otherwise any (64-bit offsets; the grid is capped
 * at 2^16 blocks and strides over the rest). */
typedef struct {
  const void* a; int64_t lda; const float* lse_a;
  const void* b; int64_t ldb; const float* lse_b;
  void* out; int64_t ldo;
  int64_t rows; int64_t n_pad; int dtype;
  const void* a_lo; const void* b_lo; void* out_lo;   /* OVG_F16X2: lo planes of a / b / out (same strides) */
} ovg_attn_merge_params;
int ovg_attn_merge(const ovg_attn_merge_params*, void* stream);

/* ------------------------------------------------------------------ *
 * One pre-LN transformer block (block.py:81-107):
 *   x = x + ls1 * proj(attn(qkv(norm1(x))));  x = x + ls2 * fc2(gelu(fc1(norm2(x))))
 * run as LN -> QKV -> flash-attn -> proj(RES) -> LN -> fc1(GELU) -> fc2(RES [+inject]).
 * x_in/x_out are f32 with row strides (x_out may alias x_in; they may also be
 * the two halves of a (.., 2C) concat buffer, omnivggt_aggregator.py:250).
 * Size limits: those of the entries it sequences, all checked before the first launch (OVG_E_ARG): 0 < M <= 2^30, M % seq == 0,
 * BH == (M / seq) 16, (M - 1) / seq < 2^22 (with rope also (M - 1) / tokens_per_view, and 0 < tokens_per_view < 2^31), seq < 2^27,
 * every extra segment's nk < 2^27, BH * ceil(seq / 64) <= 2^27, nq_pad / nk_pad as ovg_qkv. ld_in and ld_out take
 * any multiple of 4 elements; the workspace tensors are dense and may pass 2 GiB / 2^31 elements (ws_hid does from 262 145 tokens in
 * the 16-bit modes, 131 073 in f32).
 * ------------------------------------------------------------------ */
typedef struct {
  const void* n1_w; const void* n1_b;     /* f32 [1024] */
  const void* qkv_w; const float* qkv_b;  /* dtype [3072,1024]; f32 [3072] */
  const float* qn_w; const float* qn_b; const float* kn_w; const float* kn_b; /* f32 [64] or NULL */
  const void* proj_w; const float* proj_b;
  const float* ls1;                        /* f32 [1024] (ones if no LayerScale) */
  const void* n2_w; const void* n2_b;
  const void* fc1_w; const float* fc1_b;   /* dtype [4096,1024] */
  const void* fc2_w; const float* fc2_b;   /* dtype [1024,4096] */
  const float* ls2;
  const void* qkv_w_lo; const void* proj_w_lo; const void* fc1_w_lo; const void* fc2_w_lo;   /* OVG_F16X2: lo planes of the four GEMM weights */
} ovg_block_weights;

typedef struct {
  ovg_block_weights w;
  const float* x_in; int64_t ld_in;
  float* x_out; int64_t ld_out;
  int64_t M;                 /* tokens processed by this rank            */
  int64_t seq;               /* attention sequence length (per batch)     */
  int64_t BH;                /* (M/seq) * 16                               */
  int64_t nq_pad; int64_t nk_pad;
  int dtype; float ln_eps; int qk_norm; int rope; float qk_eps;
  const float* rope_cos; const float* rope_sin; int max_pos;
  int64_t tokens_per_view; int grid_w; int n_special;
  const float* inject; int64_t inj_period;     /* fc2 epilogue; NULL = none  */
  /* caller-provided workspace */
  void* ws_xn;    /* [M,1024] dtype */
  void* ws_q; void* ws_k; void* ws_vt;
  void* ws_attn;  /* [M,1024] dtype */
  void* ws_hid;   /* [M,4096] dtype */
  /* remote K/V segments (view-sharded global attention): when nseg_extra > 0 the
   * attention step uses {local K/V^T} + extra[]; the caller fills `extra`
   * between ovg_block_attn_prologue and ovg_block_attn_epilogue. */
  ovg_kv_segment extra[OVG_MAX_SEG]; int nseg_extra; int local_seg_index;
  int attn_variant;
  int qkv_part;  /* ovg_block_attn_prologue only: 0 = LN1 + q,k,v; 1 = LN1 + k,v; 2 = q only (no LN) */
  /* optional hipEvent_t handles recorded on `stream` immediately before / after the
   * flash-attention launch (bench.py: live per-kernel timing); NULL = not recorded */
  void* ev_attn_start; void* ev_attn_stop;
  int skip_attention;  /* ovg_block_attn_epilogue only: ws_attn already holds the attention output (head-parallel sharding) */
  int gemm_tile;       /* OVG_TILE_* forwarded to the four GEMMs of the block (tests force a tile; 0 in production) */
  /* optional split-KV workspace of the block's attention launch (ovg_attn_params.ws_part / ws_lse + their sizes; NULL = never split) */
  void* ws_attn_part; float* ws_attn_lse; int attn_kv_splits; int64_t ws_attn_part_bytes; int64_t ws_attn_lse_bytes;
  /* OVG_F16X2: lo planes of the six scratch tensors (same sizes as their hi tensors; ovg_block_workspace_bytes reports the size of ONE plane) */
  void* ws_xn_lo; void* ws_q_lo; void* ws_k_lo; void* ws_vt_lo; void* ws_attn_lo; void* ws_hid_lo;
  uint32_t* attn_fallback_count;   /* forwarded to ovg_attn_params.fallback_count of the block's attention launch (NULL = not counted) */
  int attn_cus;                    /* forwarded to ovg_attn_params.cus (0 = the whole device) */
} ovg_block_params;
/* whole block */
int ovg_block_forward(const ovg_block_params*, void* stream);
/* split form for the sharded path: prologue = LN1 + QKV (writes ws_q/k/vt);
 * epilogue = attention (over local+extra segments) + proj + MLP. */
int ovg_block_attn_prologue(const ovg_block_params*, void* stream);
int ovg_block_attn_epilogue(const ovg_block_params*, void* stream);

/* Workspace query (host only, no device work): bytes of each caller-provided scratch buffer of a block call
 * with the given M, seq, BH, nq_pad, nk_pad and dtype (all other fields ignored). */
typedef struct { int64_t xn, q, k, vt, attn, hid, total; } ovg_block_workspace;
int ovg_block_workspace_bytes(const ovg_block_params*, ovg_block_workspace* out);

/* Weight pre-pack (inference.py:321-325 loads f32 checkpoints): dst[r, :k] = convert(src[r, :k]) to `dtype`,
 * dst[r, k:k_pad] = 0.  src f32 [rows, k] (ld lds), dst `dtype` [rows, k_pad] (ld ldd, k_pad % 8 == 0).
 * nn.Linear weights pack with k_pad = k; the Conv2d(k=14,s=14) patch weights with k = C_in*196, k_pad = 640 / 448.
 * Size limits: rows, k > 0, k <= k_pad < 2^34 (k_pad / 8 is held as an int), lds >= k, ldd >= k_pad; offsets 64-bit, any stride. */
typedef struct {
  const float* src; int64_t lds; void* dst; int64_t ldd;
  int64_t rows; int64_t k; int64_t k_pad; int dtype;
  void* dst_lo;                  /* OVG_F16X2: lo plane (same ldd) */
} ovg_pack_weights_params;
int ovg_pack_weights(const ovg_pack_weights_params*, void* stream);

/* ------------------------------------------------------------------ *
 * Patch im2col (Conv2d k=14,s=14 as a GEMM: patch_embed.py:65,75-77).
 * img f32 [V,C,Hpx,Wpx]; out [V*gh*gw, k_pad] dtype, element k = c*196+ky*14+kx,
 * zero for k >= C*196.  mode 0: (img[c]-mean[c])/std[c]  (omnivggt_aggregator.py:143)
 * mode 1: depth/mask: c=0 -> depth/(mean_b+1e-8)*mask, c=1 -> mask
 *         (omnivggt_aggregator.py:107-128,197); depth_stats = {sum,count} per batch
 * Size limits: V > 0, Hpx, Wpx multiples of 14 (ints: one image below 2^31 pixels), C * 196 <= k_pad < 2^34, k_pad % 64 == 0; img and
 * out are dense, their offsets 64-bit (out passes 4 GiB from 3.4 million patches on); the grid is capped at 2^16 blocks.
 * ------------------------------------------------------------------ */
typedef struct {
  const float* img; const float* img2;   /* mode1: img=depth [V,H,W], img2=mask [V,H,W] */
  void* out; int64_t k_pad;
  int64_t V; int C; int Hpx; int Wpx; int dtype; int mode;
  float mean[3]; float std[3];
  const double* depth_stats;  /* mode1: [B][2] = {sum, count}; V = B*views_per_batch */
  int64_t views_per_batch;
  void* out_lo;               /* OVG_F16X2: lo plane of out */
} ovg_im2col_params;
int ovg_im2col(const ovg_im2col_params*, void* stream);

/* masked depth statistics (omnivggt_aggregator.py:118-123): stats[b] = {sum of
 * depth where mask>0, count}.  partial: workspace of 2*nblocks doubles.
 * Size limits: B, n_per_batch, nblocks > 0 (B and nblocks are grid extents); offsets 64-bit. */
typedef struct {
  const float* depth; const float* mask; int64_t B; int64_t n_per_batch;
  double* stats; double* partial; int nblocks;
} ovg_depth_stats_params;
int ovg_depth_stats(const ovg_depth_stats_params*, void* stream);

/* DINOv2 special rows (vision_transformer.py:220-224): x[v,0]=cls+pos[0], x[v,1..4]=reg
 * Size limits: V > 0, n_reg >= 0, ldx a multiple of 4 elements, otherwise any (64-bit offsets); one block per special row with an int
 * block index: V * (1 + n_reg) <= 2^31 - 1, else OVG_E_UNSUPPORTED (answered before the pointers are checked). */
typedef struct {
  float* x; int64_t ldx; int64_t V; int64_t tokens_per_view;
  const float* cls; const float* pos0; const float* reg; int n_reg;
} ovg_dino_specials_params;
int ovg_dino_specials(const ovg_dino_specials_params*, void* stream);

/* Token assembly before the AA trunk (omnivggt_aggregator.py:147-156,202-213 and
 * vision_transformer.py:264-268): for each view v and token t
 *   t == 0     : camera_token[slot] + cam_add[v]
 *   1 <= t < 5 : register_token[slot][t-1]
 *   t >= 5     : LayerNorm_eps(xd[v,t]) + (depth_row[v] >= 0 ? depth_tok[depth_row[v]*P0+t-5] : placeholder)
 * slot = ((view0 + v) % S == 0) ? 0 : 1   (aggregator.py:343-366).
 * Size limits: V, S > 0, tokens_per_view > n_special, ldxd / ldo multiples of 4 elements, otherwise any (64-bit offsets; the grid is
 * capped at 8192 blocks of four rows); the kernel holds a token index as an int: tokens_per_view >= 2^31 is OVG_E_UNSUPPORTED
 * (answered before the pointers are checked). */
typedef struct {
  const float* xd; int64_t ldxd;        /* DINO residual stream [V*P,1024] */
  const float* norm_w; const float* norm_b; float eps;
  const float* camera_token;            /* [2,1024] */
  const float* register_token;          /* [2,4,1024] */
  const float* cam_add;                 /* [V,1024] */
  const float* depth_tok;               /* [Sd*P0,1024] or NULL */
  const int32_t* depth_row;             /* [V] index into depth_tok views or -1 */
  const float* placeholder;             /* [1024] */
  float* out; int64_t ldo;
  int64_t V; int64_t S; int64_t tokens_per_view; int n_special;
  int64_t view0;                        /* global index of local view 0 (view-sharded ranks) */
} ovg_assemble_params;
int ovg_assemble_tokens(const ovg_assemble_params*, void* stream);

/* strided f32 row copy/add helper: y[r, :n] = x[r, :n] (+ add[r / period, :n] on rows r%period==0)
 * Size limits: rows, n > 0, n, ldx, ldy multiples of 4 elements, otherwise any (64-bit offsets; 8192 blocks stride over the rows). */
typedef struct {
  const float* x; int64_t ldx; float* y; int64_t ldy; int64_t rows; int64_t n;
} ovg_copy_rows_params;
int ovg_copy_rows(const ovg_copy_rows_params*, void* stream);

/* ================================================================== *
 * DPT dense-prediction head (reference heads/dpt_head.py:185-304,
 * heads/head_act.py:61-125).  OVG_BF16 / OVG_F16 (f32 accumulate) and, since ABI 7, OVG_F32 (the parity mode: exact-f32 MFMA,
 * activations / weights / outputs all f32, Cin % 32 == 0 instead of % 64).  Activations are NHWC: [n_img, H, W, C] with a pixel
 * stride (ld, in elements) >= C.
 * ================================================================== */

/* LayerNorm over rows of 2048 of the aggregator output list (dpt_head.py:219 `self.norm`):
 * input row of output row r is x + ((r / p0) * p1 + row_off + r % p0) * ldx  (p0 patch tokens kept
 * per view out of p1 tokens per view, skipping the row_off special tokens); y is [rows, 2048] dtype.
 * Size limits: rows > 0, 0 < p0 <= p1, row_off >= 0, ldx / ldy multiples of 4 elements, otherwise any (64-bit offsets and row arithmetic;
 * 2^16 blocks of four rows stride over the rest: a second trip from 262 145 rows on). */
typedef struct {
  const float* x; int64_t ldx;
  void* y; int64_t ldy;
  const float* weight; const float* bias;
  int64_t rows; int64_t p0; int64_t p1; int64_t row_off;
  float eps; int dtype;
} ovg_head_layernorm_params;
int ovg_head_layernorm(const ovg_head_layernorm_params*, void* stream);

/* NHWC convolution as an implicit GEMM on the MFMA (nn.Conv2d k=1 / k=3 stride 1|2 pad k/2, and
 * nn.ConvTranspose2d with kernel == stride via `upshuffle`; dpt_head.py:221-240 projects /
 * resize_layers, :274-304 scratch convs, :357-399 ResidualConvUnit, :445-470 FeatureFusionBlock):
 *   y[i, oy, ox, co] = act( sum_{ky,kx,ci} x[i, oy*stride+ky-pad, ox*stride+kx-pad, ci] * w[co][(ky*k+kx)*Cin + ci]
 *                           + bias[co] + pos(ox, oy, co) + add1[i,oy,ox,co] + add2[i,oy,ox,co] )
 *   x  [n_img, H, W, Cin]  (ldx);   w [Cout_gemm, k*k*Cin] dtype, taps-major then channels;   bias f32 or NULL
 *   pos_x [OW, Cout/2], pos_y [OH, Cout/2] f32 or both NULL: the UV position embedding of dpt_head.py:262-272
 *         (channels [0, Cout/2) depend on ox only, [Cout/2, Cout) on oy only)
 *   add1 / add2: optional tensors in output geometry and dtype (ld1 / ld2) -- residual / skip sums
 *   relu != 0: clamp at 0 after all additions (the in-place ReLU that opens every ResidualConvUnit is folded
 *         into the producer of its input)
 *   upshuffle = s > 1 (requires ksize == 1, stride == 1): ConvTranspose2d(k = s, stride = s); w is
 *         [s*s*Cout, Cin] ordered (dy, dx, co), bias is [Cout]; GEMM row (i, oy, ox), column (dy, dx, co)
 *         is stored at y[i, oy*s+dy, ox*s+dx, co].  pos / add are not supported together with upshuffle.
 *   out_f32 != 0: y is f32.
 * Constraints: Cin % 64 == 0 (OVG_F32: % 32); w holds w_rows rows (a multiple of 128, zero rows beyond the Cout_gemm real ones,
 * Cout_gemm = Cout, or s*s*Cout with upshuffle: then it must itself be the multiple of 128); Cout % 4 == 0.
 * Size limits: at most 2^30 output pixels (n_img OH OW; OVG_E_ARG beyond); ldx >= Cin, ldy >= Cout, ld1 / ld2 / ldy multiples of 4 elements
 * (ldx of 8; OVG_F32: 4), otherwise any: the 128-pixel kernel forms every offset in 64 bits. The 256-pixel LDS-DMA kernels (16-bit dtypes,
 * 16-bit output, >= 16384 output pixels) address the images of a tile through one buffer descriptor with 32-bit offsets; they are chosen
 * only while (255 / (OH OW) + 2) H W ldx 2 bytes -- the images 256 consecutive output pixels can touch: two from 256-pixel maps on --
 * stay below 2^32 - 65536 and the weight matrix below 2^32 bytes; any other call runs the 128-pixel kernel. y, add1, add2 are 64-bit in both. */
typedef struct {
  const void* x; int64_t ldx;
  const void* w; const float* bias;
  void* y; int64_t ldy;
  const void* add1; int64_t ld1; const void* add2; int64_t ld2;
  const float* pos_x; const float* pos_y;
  int64_t n_img; int H; int W; int Cin; int Cout; int w_rows; int ksize; int stride; int upshuffle;
  int relu; int out_f32; int dtype;
} ovg_conv_params;
int ovg_conv(const ovg_conv_params*, void* stream);

/* Bilinear resize, align_corners = True (F.interpolate at dpt_head.py:242-247, :466), NHWC, C % 8 == 0:
 * y[i, oy, ox, :] = lerp of x[i, :, :, :] at (oy*(H-1)/(OH-1), ox*(W-1)/(OW-1)), plus the optional UV
 * position embedding (pos_x [OW, C/2], pos_y [OH, C/2], dpt_head.py:249-250) -- both in `dtype`.
 * OH == 1 / OW == 1 (one-row / one-column patch grids) take source row / column 0, like ATen.
 * Size limits: H, W, OH, OW are ints; ldx, ldy >= C and multiples of 8 elements, otherwise any. Every offset is 64-bit; 2^20 blocks of
 * 256 (pixel, 8-channel) items stride over the rest (a second trip from 2^28 items on). */
typedef struct {
  const void* x; int64_t ldx; void* y; int64_t ldy;
  const float* pos_x; const float* pos_y;
  int64_t n_img; int H; int W; int OH; int OW; int C; int dtype;
} ovg_upsample_params;
int ovg_upsample(const ovg_upsample_params*, void* stream);

/* Output stage of the DPT head (second half of scratch.output_conv2, dpt_head.py:252-258, and
 * head_act.py:61-125): conv1x1(32 -> out_dim) + activation on the ReLU'd 32-channel map that
 * ovg_conv (k = 3, Cout = 32, relu, out_f32) produced; f32 in, f32 out:
 *   activation 0 = "exp" (depth head, out_dim 2: val = exp(v0)), 1 = "inv_log" (point head, out_dim 4:
 *   val_j = sign(v_j) * expm1(|v_j|), j < 3); confidence = 1 + exp(v_last) ("expp1") in both.
 *   h [npix, 32] f32;  w2 [out_dim, 32] f32, b2 [out_dim] f32;  val [npix, out_dim-1] f32;  conf [npix] f32
 * Size limits: npix > 0 (int64, 64-bit offsets; 2^20 blocks of 256 pixels stride over the rest). */
typedef struct {
  const float* h; const float* w2; const float* b2;
  float* val; float* conf;
  int64_t npix; int out_dim; int activation;
} ovg_dpt_out_params;
int ovg_dpt_out(const ovg_dpt_out_params*, void* stream);

/* The whole output stage of the DPT head in one launch (ABI 10; 16-bit dtypes): what ovg_upsample (with the UV position tables) ->
 * ovg_conv (k = 3, Cin = 128, Cout = 32, relu, out_f32) -> ovg_dpt_out compute, without the upsampled map (n x OH x OW x 128) or the 32-channel
 * map ever reaching HBM (dpt_head.py:242-258, head_act.py:61-125):
 *   x [n, H, W, 128] dtype (pixel stride ldx elements)  --bilinear, align_corners-->  [n, OH, OW, 128] (+ pos_x [OW, 64] / pos_y [OH, 64] f32,
 *   both or neither), rounded to dtype as ovg_upsample does;  w1 [>= 32 rows, 9 * 128] dtype taps-major (row stride ldw1 elements: the
 *   zero-padded matrix ovg_conv takes is fine), b1 f32 [32] or NULL;  w2 f32 [out_dim, 32], b2 f32 [out_dim];
 *   val f32 [n, OH, OW, out_dim - 1], conf f32 [n, OH, OW]; activation as ovg_dpt_out_params.
 * Any other channel count / dtype is OVG_E_UNSUPPORTED (callers run the three-launch form).
 * Size limits: the kernel indexes ONE source image with 32-bit element offsets: H W ldx < 2^31 elements, else OVG_E_UNSUPPORTED (the
 * three-launch form takes it); the image index times H W ldx is 64-bit, so n images may pass 4 GiB. OH, OW >= 2; at most 2^30 output
 * tiles of 16 x 14 pixels (OVG_E_ARG); ldx a multiple of 8 elements, ldw1 >= 1152. val / conf are dense, their offsets 64-bit. */
typedef struct {
  const void* x; int64_t ldx;
  const float* pos_x; const float* pos_y;
  const void* w1; int64_t ldw1; const float* b1;
  const float* w2; const float* b2;
  float* val; float* conf;
  int64_t n_img; int H; int W; int OH; int OW; int C; int out_dim; int activation; int dtype;
} ovg_dpt_tail_params;
int ovg_dpt_tail(const ovg_dpt_tail_params*, void* stream);

/* ------------------------------------------------------------------ *
 * Post-processing on the device: depth maps -> world-frame point maps,
 * utils/geometry.py:151-266 (unproject_depth_map_to_point_map -> depth_to_world_coords_points ->
 * depth_to_cam_coords_points), which the reference runs as a per-frame numpy loop on the host.
 *   depth [S, H, W] f32;  cam [S, 16] f32 per frame: cam-to-world rotation row-major (9), cam-to-world
 *   translation (3), fu, fv, cu, cv (closed_form_inverse_se3 of the extrinsic and the intrinsic entries,
 *   prepared by the caller);  out [S, H, W, 3] f32.
 *   x_cam = (u - cu) * d / fu, y_cam = (v - cv) * d / fv evaluated in double and rounded to f32 exactly like
 *   the numpy expression (int64 pixel grid promotes it to float64), then world = R * cam + t in double (the
 *   reference's inverse pose is float64) rounded to f32 on store (the reference returns float64).
 * Size limits: S, H, W > 0 (H, W ints); the pixel index S H W and every offset are 64-bit; 2^20 blocks of 256 pixels stride over the rest.
 * ------------------------------------------------------------------ */
typedef struct {
  const float* depth; const float* cam; float* out;
  int64_t S; int H; int W;
} ovg_unproject_params;
int ovg_unproject(const ovg_unproject_params*, void* stream);

/* ------------------------------------------------------------------ *
 * Point-cloud extraction (ABI 12): the selection core of visual_util.py:113-236 (predictions_to_glb) on the device.
 *
 * ovg_percentile: numpy-2 percentile(..., method="linear") of f32 keys, bit for bit, for up to OVG_PCT_MAX_COLS strided columns and
 * OVG_PCT_MAX_Q percentiles per column. Key i of column c is x[c * col_stride + i * stride], i < n; with `mask` (optional, [n] f32,
 * contiguous) it is x * (mask[i] > 0.1f ? 1 : 0) evaluated literally (the reference's sky-mask rule, visual_util.py:187-188).
 *   numpy's index rule runs in f32 (q = p / 100f, vi = f32(n - 1) * q; vi >= f32(n - 1) takes the maximum; lo = floor(vi),
 *   hi = f32(lo + 1) clamped to n - 1 -- numpy itself raises there), NaN sorts last and makes the result NaN, and the lerp is numpy's
 *   two-branch _lerp in f32 without contraction, so +-inf order statistics give numpy's values (NaN included).
 *   Radix select on order-preserving u32 keys: three histogram passes (11 / 11 / 10 bits, per-workgroup LDS histograms flushed with
 *   integer atomics -- exact, so deterministic), each followed by a one-workgroup pick of the bins holding the ranks; seven launches.
 *   out [ncols][nq] f32 (device). norm_out (optional, requires nq == 2): || out[:, 1] - out[:, 0] || as numpy's np.linalg.norm
 *   evaluates it for an f32 vector (f32 products summed in f64 left to right, rounded to f32, correctly rounded sqrt): the scene scale
 *   of visual_util.py:231-236 when q = {5, 95} over the (M, 3) kept vertices (stride 3, col_stride 1, ncols 3).
 *   ws: >= ovg_percentile_workspace_bytes(n, ncols) bytes, 16-byte aligned (returns -1 on bad arguments).
 *   q must lie in [0, 100]; no host synchronisation, the result stays on the device.
 *
 * ovg_point_filter: keep = conf' >= *threshold && conf' > min_conf (threshold NULL: 0), conf' = conf with the mask rule above, and with
 * flags OVG_PF_BLACK_BG: r + g + b >= 16, OVG_PF_WHITE_BG: !(r > 240 && g > 240 && b > 240) on the u8 colours
 * u8(trunc(clamp(x * 255f, 0, 255))) (one f32 multiply; the clamp only matters outside [0, 1], NaN gives 0).
 *   conf [n], mask [n] (optional) f32; images [n / hw][3][hw] f32 (NCHW, hw pixels per frame); points [n][3] f32.
 *   stage OVG_PF_COUNT: keep mask + per-workgroup counts + their scan into ws, *out_count = M (int64, device);
 *   stage OVG_PF_SCATTER: reads what COUNT left in ws and writes the kept pixels in pixel order: out_points [M][3] f32 (copies),
 *   out_colors [M][3] u8, out_index [M] int64 (optional: index_base + pixel index), entries at positions >= capacity are dropped.
 *   Both stages in one call need capacity >= M known in advance; the usual form is COUNT, read M, allocate, SCATTER with the same ws.
 *   ws: >= ovg_point_filter_workspace_bytes(n) bytes (n keep bytes + two int64 per 4096 pixels), 16-byte aligned.
 * ------------------------------------------------------------------ */
#define OVG_PCT_MAX_COLS 4
#define OVG_PCT_MAX_Q 4
typedef struct {
  const float* x; int64_t n; int64_t stride; int64_t col_stride; int32_t ncols;
  int32_t nq; float q[OVG_PCT_MAX_Q];
  const float* mask;
  float* out; float* norm_out;
  void* ws; int64_t ws_bytes;
} ovg_percentile_params;
int64_t ovg_percentile_workspace_bytes(int64_t n, int32_t ncols);
int ovg_percentile(const ovg_percentile_params*, void* stream);

enum { OVG_PF_BLACK_BG = 1, OVG_PF_WHITE_BG = 2 };
enum { OVG_PF_COUNT = 1, OVG_PF_SCATTER = 2 };
typedef struct {
  const float* conf; const float* mask; const float* threshold; float min_conf; int32_t flags;
  const float* images; int64_t hw;
  const float* points; int64_t n;
  int32_t stage; int32_t pad;
  int64_t index_base; int64_t capacity;
  float* out_points; uint8_t* out_colors; int64_t* out_index; int64_t* out_count;
  void* ws; int64_t ws_bytes;
} ovg_point_filter_params;
int64_t ovg_point_filter_workspace_bytes(int64_t n);
int ovg_point_filter(const ovg_point_filter_params*, void* stream);

/* ------------------------------------------------------------------ *
 * Voxel-grid decimation of a point cloud (added under ABI 13): one point per occupied cell of a regular grid, chosen by an exact rule
 * that tests/voxelgrid_twin.py restates in numpy float32 bit for bit.
 *   points [n][3] f32; conf [n] f32 (optional); colors [n][3] u8 (optional, with out_colors); voxel: DEVICE f32 scalar, the cell edge.
 *   1. a point is valid when its three coordinates are finite; invalid points are never kept;
 *   2. origin = component-wise minimum of the valid points (integer min of order-preserving keys: exact, independent of order);
 *   3. cell c = floor((p - origin) / voxel) per axis: one f32 subtraction, one correctly rounded f32 division, a floor. A valid point
 *      with any c > 2^21 - 1 raises OVG_VG_OVERFLOW; a voxel that is not a positive finite number raises OVG_VG_BAD_VOXEL; a call that
 *      raised either keeps nothing. The cell key is the three 21-bit indices packed into 63 bits;
 *   4. inside a cell the largest conf wins (compared through the order-preserving u32 map, -0 as +0, NaN lowest), ties and calls
 *      without conf go to the smallest input index;
 *   5. the winners leave in input order: out_points [M'][3] / out_colors [M'][3] are copies, out_index [M'] int64 (optional) the input
 *      positions; entries at positions >= capacity are dropped.
 *   stage OVG_VG_COUNT: table + winners + keep bytes + per-workgroup counts and their scan into ws; out_count[0] = M',
 *   out_count[1] = the OVG_VG_* flags raised (two int64, device). stage OVG_VG_SCATTER: reads what COUNT left in ws.
 *   Table: open addressing, linear probing, 2n (>= 1024) slots of 16 bytes {u64 key, u64 best}; a slot is claimed by a 64-bit
 *   compare-and-swap of its key, the winner is one 64-bit max of (conf key << 32) | ~index. Max and min do not depend on arrival
 *   order, so two runs give identical bytes. No float atomics.
 *   ws: >= ovg_voxel_downsample_workspace_bytes(n) bytes (256 + 32 n for the table + the point filter's n keep bytes and counts),
 *   16-byte aligned; the query returns -1 for n <= 0 or n >= 2^32, the entry OVG_E_ARG.
 * ------------------------------------------------------------------ */
enum { OVG_VG_COUNT = 1, OVG_VG_SCATTER = 2 };
enum { OVG_VG_OVERFLOW = 1, OVG_VG_BAD_VOXEL = 2 };
typedef struct {
  const float* points; const float* conf; const uint8_t* colors; const float* voxel;
  int64_t n;
  int32_t stage; int32_t pad;
  int64_t capacity;
  float* out_points; uint8_t* out_colors; int64_t* out_index; int64_t* out_count;
  void* ws; int64_t ws_bytes;
} ovg_voxel_downsample_params;
int64_t ovg_voxel_downsample_workspace_bytes(int64_t n);
int ovg_voxel_downsample(const ovg_voxel_downsample_params*, void* stream);

/* ------------------------------------------------------------------ *
 * Point-cloud rendering (added under ABI 13): z-buffered square splats of a coloured cloud into V pinhole views, by an exact rule that
 * tests/render_twin.py restates in numpy float32 bit for bit.
 *   points [n][3] f32, colors [n][3] u8 (both may be NULL when n == 0), n < 2^32; cams [V][16] f32 on the device, per view the
 *   world-to-camera rotation row-major (9), the translation (3), fx, fy, cx, cy: ovg_unproject's `cam` row in the other direction.
 *   Every step is one f32 operation rounded on its own (no fused multiply-add):
 *   1. xc = ((R00 x + R01 y) + R02 z) + tx, likewise yc, zc;
 *   2. the point is skipped for this view unless xc, yc, zc are finite and zc > near;
 *   3. u = floor((fx (xc / zc) + cx) + 0.5), w = floor((fy (yc / zc) + cy) + 0.5): correctly rounded divisions, pixel centres at
 *      integer coordinates (ovg_unproject's convention);
 *   4. skipped unless -radius <= u <= W - 1 + radius and -radius <= w <= H - 1 + radius (compared in f32: NaN fails);
 *   5. key = (bits(zc) << 32) | i: zc is positive and finite, so its bit pattern orders like its value; ~0 means "empty";
 *   6. every pixel (u + dx, w + dy), |dx|, |dy| <= radius, inside the image takes min(stored key, key): one 64-bit unsigned atomic
 *      min. The nearest point wins, equal depths go to the smallest index, and the result does not depend on arrival order;
 *   7. a non-empty pixel resolves to rgb = colors[key & 0xffffffff], depth = the float whose bits are key >> 32, index = key &
 *      0xffffffff; an empty one to the background colour, depth 0 and index -1.
 *   Three launches (fill, splat, resolve); nothing is allocated and nothing is read back: every size is known before the call.
 *   flags: OVG_RENDER_NO_PREREAD drops the plain read of the pixel in front of the atomic (which skips the atomic when the stored key
 *   is already smaller; stored keys only decrease, so a stale read is merely conservative). The images are the same either way.
 *   ws: >= ovg_render_workspace_bytes(V, H, W) bytes (the u64 z-buffer, 8 V H W rounded up to 16), 16-byte aligned; the query returns
 *   -1 for V, H, W <= 0 or V H W >= 2^31. out_rgb [V][H][W][3] u8; out_depth [V][H][W] f32 and out_index [V][H][W] int64 are optional.
 *   OVG_E_ARG: NULL params / cams / ws / out_rgb (points / colors with n > 0), n < 0 or >= 2^32, bad V, H, W, radius outside
 *   [0, OVG_RENDER_MAX_RADIUS], a near plane that is not positive and finite, unknown flags, a misaligned or undersized workspace.
 * ------------------------------------------------------------------ */
enum { OVG_RENDER_MAX_RADIUS = 8 };
enum { OVG_RENDER_NO_PREREAD = 1 };
typedef struct {
  const float* points; const uint8_t* colors; int64_t n;
  const float* cams;
  int32_t V; int32_t H; int32_t W; int32_t radius;
  float near;
  uint8_t background[3]; uint8_t pad0;
  int32_t flags; int32_t pad1;
  void* ws; int64_t ws_bytes;
  uint8_t* out_rgb; float* out_depth; int64_t* out_index;
} ovg_render_params;
int64_t ovg_render_workspace_bytes(int32_t V, int32_t H, int32_t W);
int ovg_render_points(const ovg_render_params*, void* stream);

/* ------------------------------------------------------------------ *
 * Mesh rasterisation (added under ABI 13): z-buffered triangles of a mesh into V pinhole views with per-pixel shading, by an exact
 * rule that tests/raster_twin.py restates in numpy bit for bit. Every float operation below is one IEEE operation rounded on its own
 * (no fused multiply-add); the divisions and the square root are correctly rounded.
 *   vertices [M][3] f32, faces [F][3] int32, normals [M][3] f32 or NULL, colors [M][3] u8 or NULL, M and F < 2^31 (vertices may be
 *   NULL when M == 0, faces when F == 0); cams [V][16] f32 packed as for ovg_render_points. Per view v and face f:
 *   1. a face with a vertex index outside [0, M) is skipped (checked on the device: never an out-of-bounds read);
 *   2. per vertex xc, yc, zc by rules 1-2 of ovg_render_points (f32; the vertex is usable when they are finite and zc > near), then
 *      sx = fx (xc / zc) + cx, sy = fy (yc / zc) + cy in f32; usable only when -16384 <= sx, sy <= 16384 (compared in f32: NaN
 *      fails). X = (int) floor(sx 256 + 0.5), Y likewise: 8 bits of sub-pixel fixed point (the scaling is exact, the addition is the
 *      one rounding). A face with an unusable vertex is not drawn in that view: there is no near-plane and no guard-band clipping;
 *   3. in int64: area = (X1 - X0)(Y2 - Y0) - (Y1 - Y0)(X2 - X0); area == 0 is skipped. With x to the right and y down a face whose
 *      outward normal looks at the camera has area < 0. cull: OVG_MESH_CULL_NONE draws both sides, OVG_MESH_CULL_BACK drops area > 0,
 *      OVG_MESH_CULL_FRONT drops area < 0. The box is ceil(min / 256) .. floor(max / 256) per axis, intersected with the frame;
 *   4. the centre of pixel (px, py) is (256 px, 256 py). w0 is the edge function over edge 1 -> 2, w1 over 2 -> 0, w2 over 0 -> 1
 *      (w2 = (X1 - X0)(py' - Y0) - (Y1 - Y0)(px' - X0), the others by rotating the indices), negated when area < 0, so that
 *      w0 + w1 + w2 = |area|. A pixel of the box is covered when all three are >= 0, inclusive: pixels on a shared edge are covered
 *      by both faces, and depth, then the face index decide. Inside the box every difference is below 2^23 + 2 and every product
 *      below 2^47: exact in int64 and in f64;
 *   5. in f64: li = (double) wi / (double) |area|, ri = 1.0 / (double) zci, ai = li ri, iz = (a0 + a1) + a2, zf = 1.0 / iz,
 *      z = (float) zf: positive and finite, so its bits never reach 0xFFFFFFFF. key = bits(z) << 32 | f; every covered pixel takes
 *      the minimum of its keys by one 64-bit unsigned atomic min; ~0 means "empty";
 *   6. per non-empty pixel steps 2-5 are computed again for the winning face. bi = ai zf are the perspective-correct weights and an
 *      attribute q interpolates as (b0 q0 + b1 q1) + b2 q2 in f64. c: the interpolated vertex colour, 128 per channel when colors is
 *      NULL. n: the interpolated vertex normal; when normals is NULL the face normal e1 x e2 of e1 = p1 - p0, e2 = p2 - p0 (f64
 *      differences of the f32 world vertices, each component two products and one subtraction). len = sqrt((nx nx + ny ny) + nz nz);
 *      s = |(nx c6 + ny c7) + nz c8| / len with (c6, c7, c8) the camera's optical axis (the third rotation row), s = 1 unless len is
 *      finite and > 0. OVG_MESH_SHADE_COLOR: floor(c + 0.5); OVG_MESH_SHADE_HEADLIGHT: floor((0.25 + 0.75 s) c + 0.5);
 *      OVG_MESH_SHADE_NORMAL: floor((0.5 (nk / len) + 0.5) 255 + 0.5) per component k, or 128 when len is not finite and > 0; all
 *      clamped to [0, 255]. depth = z, index = f; an empty pixel takes the background colour, depth 0 and index -1.
 *   Three launches (fill, draw, resolve); nothing is allocated and nothing is read back. The draw kernel runs one thread per face: a
 *   face whose clipped box holds at most coop_threshold pixels (0: the library's default) is walked by its own lane, a larger one by
 *   the 64 lanes of its wave together. The images do not depend on coop_threshold.
 *   ws: >= ovg_render_mesh_workspace_bytes(V, H, W) bytes (the u64 z-buffer, 8 V H W rounded up to 16), 16-byte aligned; the query
 *   returns -1 outside ovg_render_points' shape limits (V, H, W <= 0 or V H W >= 2^31). out_rgb [V][H][W][3] u8; out_depth [V][H][W]
 *   f32 and out_index [V][H][W] int64 are optional.
 *   OVG_E_ARG: NULL params / cams / ws / out_rgb, NULL vertices with M > 0 or faces with F > 0, M or F negative or >= 2^31, bad V, H, W,
 *   a near plane that is not positive and finite, unknown shading or cull, flags other than 0, a negative coop_threshold, a misaligned
 *   or undersized workspace.
 * ------------------------------------------------------------------ */
enum { OVG_MESH_SHADE_COLOR = 0, OVG_MESH_SHADE_HEADLIGHT = 1, OVG_MESH_SHADE_NORMAL = 2 };
enum { OVG_MESH_CULL_NONE = 0, OVG_MESH_CULL_BACK = 1, OVG_MESH_CULL_FRONT = 2 };
typedef struct {
  const float* vertices; const int32_t* faces; const float* normals; const uint8_t* colors;
  int64_t M; int64_t F;
  const float* cams;
  int32_t V; int32_t H; int32_t W; int32_t shading;
  int32_t cull; int32_t coop_threshold;
  float near;
  uint8_t background[3]; uint8_t pad0;
  int32_t flags; int32_t pad1;
  void* ws; int64_t ws_bytes;
  uint8_t* out_rgb; float* out_depth; int64_t* out_index;
} ovg_render_mesh_params;
int64_t ovg_render_mesh_workspace_bytes(int32_t V, int32_t H, int32_t W);
int ovg_render_mesh(const ovg_render_mesh_params*, void* stream);

/* ------------------------------------------------------------------ *
 * Multi-view depth consistency (added under ABI 13): for every pixel of S point maps, the number of OTHER views that confirm it, look
 * through it, or cannot see it, by an exact rule that tests/consistency_twin.py restates in numpy float32 bit for bit.
 *   points [S][H][W][3] f32 world points (a point map, or un-projected depth); cams [S][16] f32 on the device, packed exactly as for
 *   ovg_render_points (world-to-camera rotation row-major, translation, fx, fy, cx, cy); valid [S][H][W] u8, optional (NULL: all valid).
 *   Every step is one f32 operation rounded on its own (no fused multiply-add):
 *   1. own depth z[j][q] = ((c6 x + c7 y) + c8 z) + c11 with c = cams[j], (x, y, z) = points[j][q]. Pixel (j, q) is USABLE when
 *      valid[j][q] != 0 (if given), z[j][q] is finite and z[j][q] > near (a non-finite coordinate makes z non-finite);
 *   2. for a usable source pixel (i, p) and every other view j != i: the camera coordinates xc, yc, zc of points[i][p] in view j, the
 *      finiteness / zc > near test and the pixel u = floor((fx (xc / zc) + cx) + 0.5), w likewise: rules 1-3 of ovg_render_points.
 *      The pair is skipped unless 0 <= u <= W - 1 and 0 <= w <= H - 1 (compared in f32: NaN fails) and (j, (w, u)) is usable;
 *   3. d = z[j][(w, u)], band = tol * d, diff = zc - d. Exactly one of: |diff| <= band -> SUPPORT; diff < -band -> VIOLATION (view j
 *      sees a surface behind the point along that ray: it looks through the point); diff > band -> OCCLUDED (the point is hidden
 *      from view j: no evidence either way);
 *   4. support / violations / occluded [src_count][H][W] int16: the number of views j in each class for the source views src_first ..
 *      src_first + src_count - 1 (row 0 of the outputs is view src_first). A source pixel that is not usable has all three 0; pairs
 *      skipped in step 2 count nowhere. occluded may be NULL.
 *   Nearest-pixel lookup only: no bilinear depth, no neighbourhood search, no averaging of depths across views.
 *   Two launches: the maps z (unusable pixels as NaN) into ws, then one thread per source pixel with the targets in a loop, counters
 *   in registers, plain stores. No atomics, nothing allocated, nothing read back; two calls give identical bytes. All S views are
 *   targets whatever the source range; OVG_MVC_KEEP_MAP skips the first launch (ws still holds the maps of an earlier call with the
 *   same points, cams, valid, near and shape: a large job cut into source ranges computes them once).
 *   tile: the 256 source pixels of a workgroup as width x height (OVG_MVC_TILE_DEFAULT is the measured best);
 *   OVG_MVC_ROTATE_TARGETS lets each source view start with the target behind it instead of all walking 0 .. S - 1. Both change
 *   speed only, never a result.
 *   ws: >= ovg_consistency_workspace_bytes(S, H, W) bytes (4 S H W rounded up to 16), 16-byte aligned; the query returns -1 for
 *   S, H, W <= 0, S > OVG_MVC_MAX_VIEWS (int16 counts) or S H W >= 2^31.
 *   OVG_E_ARG: NULL params / points / cams / ws / support / violations, bad S, H, W, a source range outside [0, S) or empty, tol
 *   negative or not finite, a near plane that is not positive and finite, unknown tile / flags, a misaligned or undersized workspace.
 * ------------------------------------------------------------------ */
enum { OVG_MVC_MAX_VIEWS = 32767 };
enum { OVG_MVC_TILE_DEFAULT = 0, OVG_MVC_TILE_256x1 = 1, OVG_MVC_TILE_16x16 = 2, OVG_MVC_TILE_8x32 = 3, OVG_MVC_TILE_32x8 = 4 };
enum { OVG_MVC_ROTATE_TARGETS = 1, OVG_MVC_KEEP_MAP = 2 };
typedef struct {
  const float* points; const float* cams; const uint8_t* valid;
  int32_t S; int32_t H; int32_t W;
  int32_t src_first; int32_t src_count;
  float tol; float near;
  int32_t tile; int32_t flags; int32_t pad;
  void* ws; int64_t ws_bytes;
  int16_t* support; int16_t* violations; int16_t* occluded;
} ovg_consistency_params;
int64_t ovg_consistency_workspace_bytes(int32_t S, int32_t H, int32_t W);
int ovg_multiview_consistency(const ovg_consistency_params*, void* stream);

/* ------------------------------------------------------------------ *
 * Nearest-neighbour search between two point clouds (added under ABI 13): for every query point the nearest reference point, by an
 * exact rule that tests/nn_twin.py restates in numpy float32 bit for bit.
 *   query [nq][3] f32, reference [nr][3] f32; query_valid [nq] u8 and reference_valid [nr] u8 are optional (NULL: all valid).
 *   Every step is one f32 operation rounded on its own (no fused multiply-add):
 *   1. a point is USABLE when its three coordinates are finite and its valid byte (if given) is non-zero;
 *   2. for a usable query q and a usable reference r: dx = q.x - r.x, dy = q.y - r.y, dz = q.z - r.z, d = (dx dx + dy dy) + dz dz.
 *      d is +0, positive or +inf (an overflow is still a candidate), so its bit pattern orders like its value;
 *   3. with OVG_NN_EXCLUDE_SAME_INDEX (nq == nr: a search inside one cloud) reference j == i is no candidate of query i;
 *   4. index[i] = the j that minimises (bits(d), j) over the candidates: the nearest reference, equal distances go to the LOWEST
 *      index; sqdist[i] = that d. An unusable query, or one without a candidate, has index -1 and sqdist +inf.
 *   Brute force, nq nr pairs at about 11 vector operations each: a grid of (query tiles of OVG_NN_QUERY_TILE) x (splits of the
 *   reference tiles of OVG_NN_REFERENCE_TILE), the queries in registers, the reference tile in LDS. One split stores index / sqdist
 *   directly (one launch); several merge the packed (bits(d) << 32) | j with a 64-bit unsigned atomic min in ws and a last launch
 *   decodes it (three launches). splits = 0 chooses enough workgroups to fill the chip when there are few query tiles; a value
 *   above the number of reference tiles is clamped. The result never depends on splits. Nothing is allocated or read back.
 *   ws: >= ovg_nn_workspace_bytes(nq, nr) bytes (the u64 keys, 8 nq rounded up to 16), 16-byte aligned; the query returns -1 for
 *   nq, nr <= 0 or >= 2^31. index [nq] int32, sqdist [nq] f32.
 *   OVG_E_ARG: NULL params / query / reference / ws / index / sqdist, bad nq / nr, unknown flags, OVG_NN_EXCLUDE_SAME_INDEX with
 *   nq != nr, splits < 0, a pointer that is not 4-byte aligned, a misaligned or undersized workspace.
 * ------------------------------------------------------------------ */
enum { OVG_NN_QUERY_TILE = 512, OVG_NN_REFERENCE_TILE = 512 };
enum { OVG_NN_EXCLUDE_SAME_INDEX = 1 };
typedef struct {
  const float* query; const float* reference;
  const uint8_t* query_valid; const uint8_t* reference_valid;
  int64_t nq; int64_t nr;
  int32_t flags; int32_t splits;
  void* ws; int64_t ws_bytes;
  int32_t* index; float* sqdist;
} ovg_nn_params;
int64_t ovg_nn_workspace_bytes(int64_t nq, int64_t nr);
int ovg_nearest_neighbours(const ovg_nn_params*, void* stream);

/* ------------------------------------------------------------------ *
 * Farthest-point sampling of point clouds (added under ABI 13): npoint well-spread points of each of `batch` clouds, chosen one
 * after the other, each the point farthest from everything chosen so far. The rule is exact (tests/fps_twin.py restates it in numpy
 * float32 bit for bit) and reproduces the deterministic path of the reference's farthest_point_sample index for index.
 *   points [batch][n][3] f32, contiguous; valid [batch][n] u8 is optional (NULL: all valid).
 *   usable: as in ovg_nearest_neighbours -- all three coordinates finite and the valid byte (if given) non-zero.
 *   state: mind[j] = float32(1e10) for every j (the reference's initial value, kept on purpose: a squared distance never counts
 *   for more than 1e10, and points that far from every sample tie and are taken in index order).
 *   step i = 0 .. npoint - 1 has a centre c:
 *     step 0: c = first;  step 1 with OVG_FPS_INCLUDE_LAST: c = n - 1 (both FORCED: taken whether usable or not);
 *     otherwise c = the usable j that maximises bits(mind[j]), the LOWEST j on ties; c = -1 when no point is usable.
 *   outputs of the step: index[i] = c; sqdist[i] = mind[c] as it stood BEFORE this step's update (1e10 for the first sample and
 *   for a forced centre that is unusable, whose mind never changes), +inf when c = -1. From the first non-forced sample on, sqdist
 *   never increases: it is the squared coverage radius of the samples before it.
 *   update: if c >= 0 and point c is usable, then for every usable j: dx = p[j].x - p[c].x, dy, dz likewise,
 *   d = (dx dx + dy dy) + dz dz, every operation rounded to f32 on its own (no fused multiply-add; an overflow to +inf is fine),
 *   mind[j] = d if d < mind[j]. A forced centre that is unusable is written to index as is and updates nothing.
 *   distance [batch][n] f32 (optional, may be NULL): mind after the last step, +inf for unusable points. For usable points it equals
 *   min(1e10, the sqdist ovg_nearest_neighbours reports against the usable sampled points) byte for byte.
 *   When fewer distinct usable points than npoint exist the rule repeats the lowest-index usable point (all mind are 0 by then).
 * Two forms, identical bytes:
 *   OVG_FPS_PATH_ONE_WORKGROUP (n <= OVG_FPS_SMALL_MAX): one workgroup per cloud runs all npoint steps in one launch, coordinates
 *   and mind in registers, the cloud staged once in LDS so that the next centre is an LDS broadcast read; per step a per-thread
 *   best, a wave reduction of the packed key and one LDS round across the waves. ws is not used.
 *   OVG_FPS_PATH_PER_STEP (any n): one launch per sample over a grid of (ceil(n / OVG_FPS_TILE), batch); mind lives in ws; every
 *   workgroup reads the centre the previous launch chose from that step's key slot, updates its slice and merges
 *   key = (bits(mind) << 32) | (0xFFFFFFFF - j) with a 64-bit unsigned atomic max into the next step's slot (0 = none: a real key
 *   has a non-zero low word since j < 2^31). Stream order between the launches is the only synchronisation between workgroups:
 *   no workgroup ever waits for another. npoint + 1 launches, + 1 for distance.
 *   OVG_FPS_PATH_AUTO: one workgroup when n <= OVG_FPS_SMALL_MAX, else per step.
 *   ws: >= ovg_fps_workspace_bytes(batch, n, npoint) bytes, 16-byte aligned, whatever the path: per cloud the npoint + 1 u64 key slots,
 *   then the n f32 mind, 4 n + 8 (npoint + 1) bytes rounded up to 16. The query returns -1 unless 1 <= batch <= 65535,
 *   1 <= n < 2^31 and 1 <= npoint < 2^31. index [batch][npoint] int32, sqdist [batch][npoint] f32. Nothing is allocated or read back.
 *   OVG_E_ARG: NULL params / points / ws / index / sqdist, a bad batch / n / npoint, first outside [0, n), unknown flags, an unknown
 *   path, OVG_FPS_PATH_ONE_WORKGROUP with n > OVG_FPS_SMALL_MAX, a pointer that is not 4-byte aligned, a misaligned or undersized
 *   workspace.
 * ------------------------------------------------------------------ */
enum { OVG_FPS_SMALL_MAX = 8192, OVG_FPS_TILE = 1024 };
enum { OVG_FPS_INCLUDE_LAST = 1 };
enum { OVG_FPS_PATH_AUTO = 0, OVG_FPS_PATH_ONE_WORKGROUP = 1, OVG_FPS_PATH_PER_STEP = 2 };
typedef struct {
  const float* points; const uint8_t* valid;
  int64_t batch; int64_t n; int64_t npoint; int64_t first;
  int32_t flags; int32_t path;
  void* ws; int64_t ws_bytes;
  int32_t* index; float* sqdist; float* distance;
} ovg_fps_params;
int64_t ovg_fps_workspace_bytes(int64_t batch, int64_t n, int64_t npoint);
int ovg_farthest_point_sample(const ovg_fps_params*, void* stream);

/* ------------------------------------------------------------------ *
 * Radius neighbour search through a uniform hash grid (added under ABI 13): for every query point how many reference points lie
 * within a radius and which one is nearest, at a cost linear in the clouds for a sensible radius. The result is DEFINED without the
 * grid, as the rule of ovg_nearest_neighbours restricted to d <= radius_sq; tests/radius_twin.py restates it by brute force in
 * numpy float32 bit for bit.
 *   query [nq][3] f32, reference [nr][3] f32; query_valid [nq] u8 and reference_valid [nr] u8 are optional (NULL: all valid).
 *   1. USABLE and d = (dx dx + dy dy) + dz dz are those of ovg_nearest_neighbours: every operation rounded to f32 on its own;
 *   2. a usable reference j is a CANDIDATE of a usable query i when bits(d) <= bits(radius_sq): inclusive, d == radius_sq counts;
 *      with OVG_RS_EXCLUDE_SAME_INDEX (nq == nr: a search inside one cloud) j != i as well;
 *   3. count[i] (int32) = the number of candidates;
 *   4. index[i] = the j that minimises (bits(d), j) over the candidates (equal distances go to the LOWEST index), sqdist[i] = that d;
 *   5. an unusable query, or one without a candidate: count 0, index -1, sqdist +inf;
 *   6. radius_sq must be finite and >= 2^-100 (no step of the covering argument below meets a subnormal). A d that overflows to
 *      +inf is never a candidate here (it is one in the unbounded search).
 * The grid never changes a byte of this. With REACH = the f32 just above sqrt((double)radius_sq) (1 + 2^-20): d <= radius_sq gives
 * fl(dx^2) <= radius_sq, so |q.x - r.x| < REACH in exact arithmetic and, r.x being a float and rounding monotone,
 * fl(q.x - REACH) <= r.x <= fl(q.x + REACH); likewise y, z. The cell of a coordinate,
 *   C(x) = clamp(floor(fl(fl(x - origin) / cell)), -2^20, 2^20 - 1)   (clamped as a float, then converted),
 * is a chain of monotone maps, so every candidate of q lies in the box of cells [C(fl(q - REACH)), C(fl(q + REACH))] per axis, and
 * scanning exactly that box with the rule above IS the exhaustive result: for every cell edge, every origin (origin: device f32[3],
 * NULL = zeros; a non-finite component counts as 0 and raises OVG_RS_BAD_ORIGIN), far coordinates included (they share the clamped
 * boundary cells). cell >= REACH is required only to keep the box to a few cells per axis. The origin is NOT taken from the cloud:
 * one outlier at -9e20 would put everything else into one cell.
 * Two stages (flags OR-ed in `stage`), like ovg_voxel_downsample:
 *   OVG_RS_BUILD  clear the table of max(OVG_RS_MIN_SLOTS, 2 nr) slots; every usable reference claims its cell's slot (open
 *     addressing, linear probing, a 64-bit compare-and-swap on the packed 63-bit cell key) and counts itself; an exclusive scan of
 *     the slot counts; a scatter of 16-byte records {x, y, z, bits(j)} into cell order through a per-cell cursor (the order INSIDE a
 *     cell is left open: count, minimum and integer sums do not depend on it); a cost pass in which every usable query sums the
 *     counts of the cells of its box. out_stats int64[4] (device) = { flags (OVG_RS_BAD_ORIGIN), occupied cells, the most points
 *     in one cell, candidate pairs = the cost pass's total: the number of distances SEARCH will evaluate }.
 *   OVG_RS_SEARCH  reads what BUILD left in ws (same reference, radius_sq, cell, origin): one query per thread (workgroups of
 *     OVG_RS_QUERY_BLOCK) walks its box, probes each cell and runs the rule over the cell's records; count / index / sqdist are
 *     stored directly. Integer atomics only, no float atomics, no workgroup ever waits for another.
 *     WORK GUARD: a radius too large for the cloud makes one thread's loop quadratic. SEARCH writes NOTHING to count / index / sqdist
 *     when the candidate pairs BUILD counted exceed max_pairs (>= 0), or when ws holds no BUILD of this nr; out_stats (optional in
 *     this stage) then reports OVG_RS_OVER_BUDGET / OVG_RS_NOT_BUILT in its flags. Callers read out_stats between the stages.
 *   ws: >= ovg_radius_workspace_bytes(nq, nr) bytes, 16-byte aligned: 256 + 16 max(1024, 2 nr) + 16 nr + 4 ceil(slots / 4096),
 *   each part rounded up to 256; the query returns -1 unless 1 <= nq, nr < 2^31. Nothing is allocated or read back.
 *   OVG_E_ARG: NULL params / query / reference / ws (out_stats in BUILD; count / index / sqdist in SEARCH), bad nq / nr, radius_sq
 *   not finite or < 2^-100, cell not finite or < REACH, unknown flags or stage, OVG_RS_EXCLUDE_SAME_INDEX with nq != nr,
 *   max_pairs < 0 in SEARCH, a pointer that is not 4-byte (out_stats: 8-byte) aligned, a misaligned or undersized workspace.
 * ------------------------------------------------------------------ */
enum { OVG_RS_BUILD = 1, OVG_RS_SEARCH = 2 };
enum { OVG_RS_EXCLUDE_SAME_INDEX = 1 };
enum { OVG_RS_BAD_ORIGIN = 1, OVG_RS_OVER_BUDGET = 2, OVG_RS_NOT_BUILT = 4 };      /* out_stats[0] */
enum { OVG_RS_MIN_SLOTS = 1024, OVG_RS_QUERY_BLOCK = 256 };
typedef struct {
  const float* query; const float* reference;
  const uint8_t* query_valid; const uint8_t* reference_valid;
  const float* origin;
  int64_t nq; int64_t nr;
  float radius_sq; float cell;
  int32_t flags; int32_t stage;
  int64_t max_pairs;
  void* ws; int64_t ws_bytes;
  int64_t* out_stats;
  int32_t* count; int32_t* index; float* sqdist;
} ovg_radius_params;
int64_t ovg_radius_workspace_bytes(int64_t nq, int64_t nr);
int ovg_radius_search(const ovg_radius_params*, void* stream);

/* ------------------------------------------------------------------ *
 * The k nearest neighbours within a radius (added under ABI 13), on the grid ovg_radius_search builds: the neighbourhood itself where
 * ovg_radius_search returns its size and its nearest point (the hybrid search: k nearest, but only those within the radius).
 * Defined WITHOUT the grid by rules 1, 2, 3 and 6 of ovg_radius_search; tests/knn_twin.py restates it by brute force:
 *   d = (dx dx + dy dy) + dz dz in f32, one rounding per operation; a CANDIDATE of a usable query i is a usable reference j with
 *   bits(d) <= bits(radius_sq) (inclusive), and j != i with OVG_RS_EXCLUDE_SAME_INDEX;
 *   count[i] = the number of candidates: the value ovg_radius_search writes;
 *   index[i][t], sqdist[i][t], t < k: the candidates in ascending order of (bits(d), j) -- nearest first, equal distances in
 *   ascending reference index; ranks t >= min(k, count[i]) hold index -1 and sqdist +inf; an unusable query has count 0 and every
 *   rank -1 / +inf. Rank 0 is ovg_radius_search's index / sqdist. 1 <= k <= OVG_KNN_MAX_K.
 * A search only: it reads the grid ovg_radius_search(stage = OVG_RS_BUILD) left in ws for the same reference, radius_sq, cell and
 * origin (ws_bytes >= ovg_radius_workspace_bytes(nq, nr)), with the same walk over the same box, so the grid never changes a byte
 * of this either. One query per thread in workgroups of OVG_RS_QUERY_BLOCK; the running selection is a sorted list of K packed keys
 * (bits(d) << 32) | j in registers, K the smallest of 4, 8, 16, 32 that is >= k (the result does not depend on K): a candidate is
 * compared with the worst key first, and only an accepted one runs the K compare-and-swaps of the insertion.
 * WORK GUARD and OVG_RS_NOT_BUILT as in OVG_RS_SEARCH: nothing is written to count / index / sqdist when the candidate pairs BUILD
 * counted exceed max_pairs or ws holds no BUILD of this nr; out_stats int64[4] (optional) reports as it does there.
 *   count [nq] int32, index [nq][k] int32, sqdist [nq][k] f32. Nothing is allocated or read back.
 *   OVG_E_ARG: as OVG_RS_SEARCH (NULL params / query / reference / ws / count / index / sqdist, bad nq / nr, radius_sq, cell, flags,
 *   OVG_RS_EXCLUDE_SAME_INDEX with nq != nr, max_pairs < 0, alignment, a misaligned or undersized workspace), and k outside
 *   [1, OVG_KNN_MAX_K].
 * ------------------------------------------------------------------ */
enum { OVG_KNN_MAX_K = 32 };
typedef struct {
  const float* query; const float* reference;
  const uint8_t* query_valid; const uint8_t* reference_valid;
  const float* origin;
  int64_t nq; int64_t nr;
  float radius_sq; float cell;
  int32_t flags; int32_t k;
  int64_t max_pairs;
  void* ws; int64_t ws_bytes;
  int64_t* out_stats;
  int32_t* count; int32_t* index; float* sqdist;
} ovg_knn_params;
int ovg_knn_search(const ovg_knn_params*, void* stream);

/* ------------------------------------------------------------------ *
 * Clustering of a point cloud (added under ABI 13), on the grid ovg_radius_search builds: which points belong together -- Euclidean
 * connected components, and DBSCAN with a deterministic border rule. Defined WITHOUT the grid and without the union-find;
 * tests/cluster_twin.py restates it by brute force. One cloud points [n][3] f32, valid [n] u8 optional (NULL: all valid), radius_sq,
 * min_neighbours >= 0:
 *   1. USABLE and d = (dx dx + dy dy) + dz dz are those of ovg_radius_search: f32, one rounding per operation. d is symmetric bit for
 *      bit (fl(a - b)^2 == fl(b - a)^2);
 *   2. i and j are NEIGHBOURS when both are usable, i != j and bits(d) <= bits(radius_sq) (inclusive);
 *   3. degree[i] (int32) = the number of neighbours of i: the count ovg_radius_search writes with OVG_RS_EXCLUDE_SAME_INDEX; 0 for an
 *      unusable point;
 *   4. CORE: usable and degree[i] >= min_neighbours. With min_neighbours = 0 every usable point is core and the result is the
 *      plain Euclidean connected components (Open3D's cluster_dbscan counts the point itself: its min_points is min_neighbours + 1);
 *   5. the clusters are the connected components of the graph whose vertices are the core points and whose edges are the neighbour
 *      pairs of core points; root[i] (int32) of a core point is the LOWEST index in its component;
 *   6. BORDER: usable, not core, with at least one core neighbour: it joins the cluster of the core neighbour j that minimises
 *      (bits(d), j) -- the nearest core point, equal distances to the lowest index -- root[i] = root[j]. (Classic DBSCAN leaves a
 *      border point between two clusters to the visiting order; this rule does not);
 *   7. NOISE: every other usable point; UNUSABLE: the rest. Both: root -1;
 *   8. kind[i] (u8) = OVG_CL_UNUSABLE / OVG_CL_NOISE / OVG_CL_BORDER / OVG_CL_CORE.
 * A search only: it reads the grid ovg_radius_search(stage = OVG_RS_BUILD) left in ws for query == reference == points, the same
 * valid on both sides, and the same radius_sq, cell and origin (ws_bytes >= ovg_radius_workspace_bytes(n, n)); with the walk of
 * OVG_RS_SEARCH over the same box the grid never changes a byte of this either. No further workspace: `root` is the union-find's
 * parent array while the launches run (one word of ws's header carries OVG_CL_INTERNAL between them). One launch per pass, one
 * point per thread in workgroups of OVG_RS_QUERY_BLOCK, the kernel boundary the only ordering between passes:
 *   degree   the walk, counting: degree, kind (CORE, or NOISE for what border decides later), parent = i for a core point, else -1;
 *   link     every core i unites itself with each core neighbour j < i. Lock-free union-find: parent[x] <= x, a slot only ever
 *            decreases, every value stored in parent[x] is a member of x's component; a hook is a 32-bit compare-and-swap that makes a
 *            root point to a smaller root (on failure: retry from the value returned), paths are halved through an atomic min
 *            with an ancestor. Hence the final root is the component's lowest index whatever the schedule. Every access to the
 *            parent array is a relaxed agent-scope atomic; no thread waits for a value another workgroup must produce;
 *   flatten  root[i] = find(i) for the core points;
 *   border   every usable non-core i takes the minimum of (bits(d), j) over its core neighbours: root[i] = root[j] and BORDER, or NOISE.
 *   A record's index j is followed only when j < n. Every device loop has a hard trip bound (2 n steps suffice, 4 n + 4 are
 *   allowed); an overrun or a parent outside [0, x] raises OVG_CL_INTERNAL in out_stats[0] and ends the thread: root / kind are
 *   then not a result. Integer atomics only; nothing is allocated or read back.
 * WORK GUARD and OVG_RS_NOT_BUILT as in ovg_knn_search: nothing is written to root / kind / degree when the candidate pairs BUILD
 * counted exceed max_pairs or ws holds no BUILD of this n; out_stats int64[4] (optional) reports as it does there.
 *   root [n] int32, kind [n] u8, degree [n] int32 (optional, NULL: not written).
 *   OVG_E_ARG: NULL params / points / ws / root / kind, n outside [1, 2^31), radius_sq not finite or < 2^-100, cell not finite or
 *   < REACH, flags != 0 (none is defined), min_neighbours < 0, max_pairs < 0, a pointer that is not 4-byte (out_stats: 8-byte)
 *   aligned (points, origin, root, degree), a misaligned or undersized workspace.
 * ------------------------------------------------------------------ */
enum { OVG_CL_UNUSABLE = 0, OVG_CL_NOISE = 1, OVG_CL_BORDER = 2, OVG_CL_CORE = 3 };       /* kind */
enum { OVG_CL_INTERNAL = 8 };                                                          /* out_stats[0], next to the OVG_RS_ flags */
typedef struct {
  const float* points; const uint8_t* valid;
  const float* origin;
  int64_t n;
  float radius_sq; float cell;
  int32_t min_neighbours; int32_t flags;
  int64_t max_pairs;
  void* ws; int64_t ws_bytes;
  int64_t* out_stats;
  int32_t* root; uint8_t* kind; int32_t* degree;
} ovg_cluster_params;
int ovg_cluster(const ovg_cluster_params*, void* stream);

/* ------------------------------------------------------------------ *
 * PCA normals from a neighbour table (added under ABI 13): for every query the normal of the plane through the reference points
 * that its row of `index` names (as ovg_knn_search writes it: any k >= 1).
 *   query [nq][3] f32, reference [nr][3] f32, index [nq][k] int32; viewpoint f32: NULL, [3] shared by all queries
 *   (viewpoint_stride 0) or [nq][3] (viewpoint_stride 3).
 *   Everything in float64, every operation rounded on its own (no fused multiply-add), over the ranks t in ascending order:
 *   1. the NEIGHBOURS are the entries with 0 <= index < nr, any other entry is skipped; m = their number;
 *   2. mean = (the sum of the neighbours, from +0) / m per coordinate;
 *   3. covariance entry ab = (the sum of (p - mean)_a (p - mean)_b, from +0) / m, for xx xy xz yy yz zz (m = 0: all zero);
 *   4. m < 3 or a non-finite covariance entry: normal (0, 0, 0), curvature 0;
 *   5. else OVG_KNN_NORMALS_SWEEPS sweeps of cyclic Jacobi rotations (0,1), (0,2), (1,2) (a zero off-diagonal entry is skipped;
 *      theta = (aqq - app) / (2 apq), t = sgn(theta) / (|theta| + sqrt(theta^2 + 1)), c = 1 / sqrt(t^2 + 1), s = t c); the normal is
 *      the column of the accumulated rotations under the SMALLEST diagonal entry lambda0 (the lowest column on ties), divided by its
 *      length;
 *   6. curvature = lambda0 / ((xx + yy) + zz) of step 3 (the surface variation; 0 when the trace or lambda0 is not positive);
 *   7. orientation: with a viewpoint v the normal is negated when (n.x (v - q).x + n.y (v - q).y) + n.z (v - q).z < 0; without, when
 *      its component of largest magnitude (the lowest axis on ties) is negative; then it is rounded to f32.
 *   normal [nq][3] f32; optional (NULL: not written) curvature [nq] f32, covariance [nq][6] f64 (step 3, written for every query),
 *   used [nq] int32 (m). One query per thread; nothing is allocated or read back.
 *   OVG_E_ARG: NULL params / query / reference / index / normal, nq or nr outside [1, 2^31), k < 1, viewpoint_stride not 0 or 3
 *   (not 0 without a viewpoint), a pointer that is not 4-byte (covariance: 8-byte) aligned.
 * ------------------------------------------------------------------ */
enum { OVG_KNN_NORMALS_SWEEPS = 8 };
typedef struct {
  const float* query; const float* reference;
  const int32_t* index; const float* viewpoint;
  int64_t nq; int64_t nr;
  int32_t k; int32_t viewpoint_stride;
  float* normal; float* curvature;
  double* covariance; int32_t* used;
} ovg_knn_normals_params;
int ovg_knn_normals(const ovg_knn_normals_params*, void* stream);

/* ------------------------------------------------------------------ *
 * Registration of point clouds (added under ABI 13): the least-squares rigid or similarity transform between paired points, as three
 * entries that never read anything back -- the pair moments, the solve, the transform applied. tests/align_twin.py restates the
 * moments and the apply operation for operation (byte-identical) and the solve by numpy's eigh and, independently, Umeyama's SVD.
 *
 * ovg_align_moments: source p [n][3] f32, target q [m][3] f32; pair i is (p[i], q[j]) with j = index[i] (int32 [n]), or j = i when
 *   index is NULL (then n == m). Pair i is USED when 0 <= j < m, all six coordinates are finite, source_valid[i] and target_valid[j]
 *   (u8, optional) are non-zero and, with OVG_ALIGN_GATE, sqdist[i] <= max_sqdist (f32 [n]; inclusive; a NaN on either side is not
 *   used). centre: NULL or f64 [6] on the device, (cp, cq). Everything in float64, every operation rounded on its own (no fused
 *   multiply-add): a = p - cp, b = q - cq, d = q - p (from the uncentred values) per coordinate, and the 18 TERMS of a pair
 *     [0..2] a   [3..5] b   [6 + 3 r + c] a_r b_c   [15] (a0 a0 + a1 a1) + a2 a2   [16] the same of b   [17] the same of d.
 *   out_count int64 [1]: the number of used pairs; out_sums f64 [18]: the sums of the terms over the used pairs, in THIS order:
 *   1. tile g holds the pairs [OVG_ALIGN_TILE g, OVG_ALIGN_TILE (g + 1)); thread t of its OVG_ALIGN_THREADS threads adds the terms of
 *      the pairs t, t + THREADS, t + 2 THREADS, ... of the tile in that order onto +0.0, skipping pairs that are not used or >= n;
 *   2. inside a wave of 64 lanes v[l] = v[l] + v[l + s] for s = 32, 16, 8, 4, 2, 1 (lane 0 holds the wave's sum);
 *   3. the four wave sums combine as (w0 + w1) + (w2 + w3): the tile's partial, written to ws;
 *   4. a second launch of one workgroup folds the partials the same way: thread t adds the partials of the tiles t, t + THREADS, ...
 *      in that order onto +0.0, then steps 2 and 3.
 *   The order is part of the rule: no float atomics, no workgroup waits for another (stream order between the two launches is the
 *   only synchronisation), so two calls give identical bytes. No used pair: count 0 and every sum +0.0.
 *   ws: >= ovg_align_workspace_bytes(n) bytes, 16-byte aligned: 160 bytes (the count and 18 sums, padded) per tile, rounded up to 256;
 *   the query returns -1 unless 1 <= n < 2^31.
 *   OVG_E_ARG: NULL params / source / target / ws / out_count / out_sums, n or m outside [1, 2^31), n != m without an index, unknown
 *   flags, OVG_ALIGN_GATE without sqdist or with a NaN max_sqdist, a pointer that is not 4-byte (centre, out_count, out_sums: 8-byte)
 *   aligned, a misaligned or undersized workspace. Nothing is written then.
 *
 * ovg_align_solve: one workgroup, one thread: the moments (count int64 [1], sums f64 [18], centre as they were computed with) ->
 *   the transform q ~ s R p + t that minimises the sum of |q - (s R p + t)|^2 over the used pairs (s = 1 without OVG_ALIGN_SCALE).
 *   All in float64, N = count:
 *   1. DEGENERATE when N < 3 (OVG_ALIGN_FEW_PAIRS), a sum or a centre entry is not finite (OVG_ALIGN_NOT_FINITE), or the source has
 *      no spread: var = sums[15] - |sums[0..2]|^2 / N is not above OVG_ALIGN_SPREAD_EPS (2^-40) sums[15] (OVG_ALIGN_NO_SPREAD: all
 *      source points coincide, or lie so far from the centre that the subtraction keeps fewer than 12 bits);
 *   2. S[r][c] = sums[6 + 3 r + c] - sums[r] sums[3 + c] / N, the mean-corrected cross-covariance (times N);
 *   3. rotation by Horn's quaternion method: the symmetric 4 x 4 matrix
 *        [ Sxx+Syy+Szz   Syz-Szy        Szx-Sxz        Sxy-Syx      ]
 *        [               Sxx-Syy-Szz    Sxy+Syx        Szx+Sxz      ]
 *        [                              -Sxx+Syy-Szz   Syz+Szy      ]
 *        [                                             -Sxx-Syy+Szz ]
 *      is diagonalised by OVG_ALIGN_JACOBI_SWEEPS sweeps of cyclic Jacobi rotations (0,1) (0,2) (0,3) (1,2) (1,3) (2,3) (the rotation
 *      of ovg_knn_normals; a zero entry is skipped); the column of the accumulated rotations under the LARGEST diagonal entry (the
 *      lowest column on ties), divided by its length, is the unit quaternion (w, x, y, z) of R -- always a proper rotation
 *      (det +1), also where the best orthogonal fit is a reflection (it then equals Umeyama's reflection-corrected solution);
 *   4. s = (sum of R[r][c] S[c][r]) / var with OVG_ALIGN_SCALE, else 1; t = (sums[3..5] / N + cq) - s R (sums[0..2] / N + cp);
 *   5. step = [s R, t; 0 0 0 1]; a step with a non-finite entry is DEGENERATE too (OVG_ALIGN_NOT_FINITE). A degenerate step is the
 *      identity with scale 1: a NaN is never written to the transform;
 *   6. transform f64 [4][4] row-major: with OVG_ALIGN_COMPOSE transform <- step transform (read, multiplied, written back: the running
 *      transform of an iteration), else transform <- step.
 *   Optional outputs (NULL: not written): out_scale f64 [1] (s of this step), out_rms f64 [1] (sqrt(sums[17] / N): the root mean square
 *   distance of the used pairs BEFORE the step; 0 when N < 1 or sums[17] is not finite), out_count int64 [1] (N), out_status int32 [1]
 *   (the OVG_ALIGN_* status bits, 0 for a regular step).
 *   OVG_E_ARG: NULL params / count / sums / transform, unknown flags, a pointer that is not 8-byte (out_status: 4-byte) aligned.
 *
 * ovg_align_apply: out[i][r] = f32(((T[r][0] x + T[r][1] y) + T[r][2] z) + T[r][3]) for r < 3, (x, y, z) = points[i] widened to
 *   float64, T the f64 [4][4] transform read from device memory; every operation rounded on its own, one rounding to f32. Non-finite
 *   points pass through as the arithmetic gives them. points [n][3] f32, out [n][3] f32 (out == points is allowed).
 *   OVG_E_ARG: NULL params / points / transform / out, n outside [1, 2^31), a pointer that is not 4-byte (transform: 8-byte) aligned.
 * ------------------------------------------------------------------ */
enum { OVG_ALIGN_THREADS = 256, OVG_ALIGN_TILE = 1024, OVG_ALIGN_JACOBI_SWEEPS = 12, OVG_ALIGN_SUMS = 18, OVG_ALIGN_PARTIAL_BYTES = 160 };
enum { OVG_ALIGN_GATE = 1 };                                                         /* ovg_align_moments_params.flags */
enum { OVG_ALIGN_SCALE = 1, OVG_ALIGN_COMPOSE = 2 };                                 /* ovg_align_solve_params.flags */
enum { OVG_ALIGN_FEW_PAIRS = 1, OVG_ALIGN_NO_SPREAD = 2, OVG_ALIGN_NOT_FINITE = 4 }; /* out_status */
#define OVG_ALIGN_SPREAD_EPS 9.094947017729282e-13                                   /* 2^-40 */
typedef struct {
  const float* source; const float* target;
  const int32_t* index;
  const uint8_t* source_valid; const uint8_t* target_valid;
  const float* sqdist;
  const double* centre;
  int64_t n; int64_t m;
  float max_sqdist; int32_t flags;
  void* ws; int64_t ws_bytes;
  int64_t* out_count; double* out_sums;
} ovg_align_moments_params;
int64_t ovg_align_workspace_bytes(int64_t n);
int ovg_align_moments(const ovg_align_moments_params*, void* stream);

typedef struct {
  const int64_t* count; const double* sums; const double* centre;
  int64_t flags;
  double* transform;
  double* out_scale; double* out_rms; int64_t* out_count; int32_t* out_status;
} ovg_align_solve_params;
int ovg_align_solve(const ovg_align_solve_params*, void* stream);

typedef struct {
  const float* points; const double* transform;
  int64_t n;
  float* out;
} ovg_align_apply_params;
int ovg_align_apply(const ovg_align_apply_params*, void* stream);

/* ------------------------------------------------------------------ *
 * Weighted, robust registration and moving a prediction into another frame (added under ABI 13): what stitching overlapping chunks
 * of a long sequence needs -- the moments of ovg_align_moments with a weight per pair, optionally reweighted by the pair's residual
 * under a previous transform (iteratively reweighted least squares with the Cauchy weight), the solve with the weight sum in the
 * place of the pair count, and the maps and cameras of a chunk carried over by the fitted transform. Four entries that never read
 * anything back. tests/stitch_twin.py restates the moments and the two moves operation for operation (byte-identical) and the solve
 * by numpy's eigh and, independently, a weighted Umeyama fit from the points. All arithmetic in float64, every operation rounded on
 * its own (no fused multiply-add).
 *
 * ovg_align_wmoments: source p [n][3] f32, target q [n][3] f32, pair i is (p[i], q[i]). weight f32 [n] or NULL (1), source_valid /
 *   target_valid u8 [n] or NULL, transform f64 [4][4] row-major or NULL (the identity; only rows 0..2 are read), delta f64 [1] on the
 *   device or NULL (1), delta_scale a host double, centre f64 [6] (cp, cq) or NULL (zeros), flags: OVG_WALIGN_CAUCHY.
 *   Pair i is USED when its six coordinates are finite, its valid bytes are non-zero, its weight (if given) is finite and > 0 and,
 *   with a transform, the three moved coordinates are finite. For a used pair
 *     w = (double)weight[i], or 1;
 *     m[r] = ((T[r][0] x + T[r][1] y) + T[r][2] z) + T[r][3], (x, y, z) = p widened -- ovg_align_apply's expression, kept in float64
 *            (m = p without a transform);
 *     e = q - m, r2 = (e0 e0 + e1 e1) + e2 e2;
 *     with OVG_WALIGN_CAUCHY: delta = delta_scale * (delta ? *delta : 1); if delta is finite and > 0 and delta delta > 0 (a square
 *            that underflows reweights nothing), h = 1 / (1 + r2 / (delta delta)), else h = 1 -- a perfect previous fit (rms 0)
 *            must not zero every weight; without the flag h = 1;
 *     W = w h;
 *     a = p - cp, b = q - cq from the UNMOVED source: the sums describe the fit source -> target, never a step onto a moved source.
 *   The 20 TERMS of a pair (OVG_WALIGN_SUMS):
 *     [0..2] W a   [3..5] W b   [6 + 3 r + c] (W a_r) b_c   [15] W ((a0 a0 + a1 a1) + a2 a2)   [16] the same of b   [17] W r2
 *     [18] W   [19] W W.
 *   out_count int64 [1]: the used pairs; out_sums f64 [20]: the sums of the terms over them in the order of ovg_align_moments, steps
 *   1 .. 4 word for word (thread, wave tree, tile slot, one-workgroup fold; OVG_ALIGN_TILE pairs per tile, OVG_ALIGN_THREADS
 *   threads), so two calls give identical bytes, and with weight == NULL and no flag sums [0..17] and the count are
 *   ovg_align_moments' bytes (W = 1 multiplies exactly). No used pair: count 0 and every sum +0.0.
 *   ws: >= ovg_align_wmoments_workspace_bytes(n) bytes, 16-byte aligned: OVG_WALIGN_PARTIAL_BYTES = 176 bytes (the count and 20 sums,
 *   padded) per tile, rounded up to 256; the query returns -1 unless 1 <= n < 2^31.
 *   OVG_E_ARG: NULL params / source / target / ws / out_count / out_sums, n outside [1, 2^31), unknown flags, a NaN delta_scale, a
 *   pointer that is not 4-byte (transform, delta, centre, out_count, out_sums: 8-byte) aligned, a misaligned or undersized
 *   workspace. Nothing is written then.
 *
 * ovg_align_wsolve: ovg_align_solve's rule (its steps 1 .. 5) on sums [0..17] with N replaced by W = sums[18]: the transform that
 *   minimises the sum of W_i |q_i - (s R p_i + t)|^2. One workgroup, one thread; count int64 [1], sums f64 [20], centre as for the
 *   moments. DEGENERATE when count < 3 or not W > 0 (OVG_ALIGN_FEW_PAIRS), when one of the 20 sums or a centre entry is not finite
 *   (OVG_ALIGN_NOT_FINITE), when var = sums[15] - |sums[0..2]|^2 / W is not above OVG_ALIGN_SPREAD_EPS sums[15]
 *   (OVG_ALIGN_NO_SPREAD), or when the step has a non-finite entry (OVG_ALIGN_NOT_FINITE).
 *   flags: OVG_ALIGN_SCALE as for ovg_align_solve; OVG_WALIGN_KEEP: a degenerate solve leaves transform AND out_scale untouched
 *   instead of writing the identity and 1 -- a refit loop keeps its last good transform. There is no compose: the moments always
 *   describe source -> target. transform f64 [4][4] <- [s R, t; 0 0 0 1].
 *   Optional outputs (NULL: not written): out_scale f64 [1] (s); out_rms f64 [1] = sqrt(sums[17] / W), the weighted root mean square
 *   residual under the transform the weights came from (0 unless W > 0 and W, sums[17] are finite); out_fit_rms f64 [1] =
 *   sqrt(max(E, 0) / W), the weighted root mean square residual AFTER this fit, from the moments alone: with tr = the sum of
 *   R[r][c] S[c][r] and vb = sums[16] - |sums[3..5]|^2 / W, E = vb - (tr tr) / var with OVG_ALIGN_SCALE and E = (var + vb) - 2 tr
 *   without (0 for a degenerate solve or an E that is not finite; E is a difference of sums of the size of vb, so its absolute
 *   error is a few ulps of vb); out_weight f64 [1] (W); out_count int64 [1]; out_status int32 [1].
 *   OVG_E_ARG: NULL params / count / sums / transform, unknown flags, a pointer that is not 8-byte (out_status: 4-byte) aligned.
 *
 * ovg_align_move_maps: one pass over the n pixels of a chunk's maps, one thread per pixel, each of four map pairs optional (NULL in,
 *   NULL out): out_points[i] = ovg_align_apply's rule for points [n][3] f32 under transform f64 [4][4]; out_depth[i] =
 *   f32((double)depth[i] * s) with s = *scale (f64 [1] on the device); out_points_conf / out_depth_conf [n] f32 are copies. An
 *   output may be its own input.
 *   OVG_E_ARG: NULL params, n outside [1, 2^31), no map at all, an input without its output or the reverse, points without
 *   transform, depth without scale, a pointer that is not 4-byte (transform, scale: 8-byte) aligned.
 *
 * ovg_align_move_cameras: one thread per camera. extrinsic f32 [views][3][4] = [Rv | tv], world-to-camera in the chunk's frame; M =
 *   transform f64 [4][4] = [s Rg, tM] the similarity that moved the chunk's points (x' = M x); s = *scale (f64 [1] on the device).
 *     Rg[r][c] = M[r][c] / s;  A[i][j] = (Rv[i][0] Rg[j][0] + Rv[i][1] Rg[j][1]) + Rv[i][2] Rg[j][2];
 *     t'[i] = s tv[i] - ((A[i][0] M[0][3] + A[i][1] M[1][3]) + A[i][2] M[2][3]);  out [views][3][4] = [A | t'] rounded to f32 once.
 *   [A | t'] is the camera that sees the moved points at s times the old depth: x = Rg^T (x' - tM) / s, so s (Rv x + tv) =
 *   Rv Rg^T (x' - tM) + s tv = A x' + t'. out == extrinsic is allowed.
 *   OVG_E_ARG: NULL params / extrinsic / transform / scale / out, views outside [1, 2^31), a pointer that is not 4-byte (transform,
 *   scale: 8-byte) aligned.
 * ------------------------------------------------------------------ */
enum { OVG_WALIGN_SUMS = 20, OVG_WALIGN_PARTIAL_BYTES = 176 };
enum { OVG_WALIGN_CAUCHY = 1 };                                                      /* ovg_align_wmoments_params.flags */
enum { OVG_WALIGN_KEEP = 4 };                                                        /* ovg_align_wsolve_params.flags, with OVG_ALIGN_SCALE */
typedef struct {
  const float* source; const float* target; const float* weight;
  const uint8_t* source_valid; const uint8_t* target_valid;
  const double* transform; const double* delta; const double* centre;
  double delta_scale;
  int64_t n; int64_t flags;
  void* ws; int64_t ws_bytes;
  int64_t* out_count; double* out_sums;
} ovg_align_wmoments_params;
int64_t ovg_align_wmoments_workspace_bytes(int64_t n);
int ovg_align_wmoments(const ovg_align_wmoments_params*, void* stream);

typedef struct {
  const int64_t* count; const double* sums; const double* centre;
  int64_t flags;
  double* transform;
  double* out_scale; double* out_rms; double* out_fit_rms; double* out_weight; int64_t* out_count; int32_t* out_status;
} ovg_align_wsolve_params;
int ovg_align_wsolve(const ovg_align_wsolve_params*, void* stream);

typedef struct {
  const float* points; const float* depth; const float* points_conf; const float* depth_conf;
  const double* transform; const double* scale;
  int64_t n;
  float* out_points; float* out_depth; float* out_points_conf; float* out_depth_conf;
} ovg_align_move_maps_params;
int ovg_align_move_maps(const ovg_align_move_maps_params*, void* stream);

typedef struct {
  const float* extrinsic; const double* transform; const double* scale;
  int64_t views;
  float* out;
} ovg_align_move_cameras_params;
int ovg_align_move_cameras(const ovg_align_move_cameras_params*, void* stream);

/* ------------------------------------------------------------------ *
 * Depth evaluation (added under ABI 13): how good a predicted depth map is against ground truth -- AbsRel, delta < 1.25 and their
 * kin after a median, scale or scale-and-shift alignment -- as three entries that never read anything back: the masked medians of
 * every group, the float64 sums of a group (the moments a fit needs, or the metric terms under given coefficients), and the solve
 * from either to the coefficients. tests/deptheval_twin.py restates all three in numpy; every output is compared byte for byte but
 * the one sum that holds a logarithm.
 *
 * Shared by the three entries. pred, gt: f32 [groups][n], G = groups rows of n contiguous pixels, row g at pred + g stride (stride
 * in ELEMENTS, the same for pred, gt and valid; stride >= n). valid: u8 [groups][n] or NULL. Pixel i of group g is USED when
 *   valid is NULL or valid[g][i] != 0,   pred and gt are finite there,   pred > 0,   min_depth < gt <= max_depth
 * (f32 comparisons; min_depth >= 0 and not NaN, max_depth not NaN, +inf allowed). A used pred or gt is therefore positive and
 * finite, subnormals included. Limits: 1 <= n, 1 <= groups <= OVG_DEPTHEVAL_MAX_GROUPS, groups n < 2^31, groups stride < 2^40.
 *
 * ovg_deptheval_median: out_count int64 [G]: the number N of used pixels of the group; out_median f32 [G][2][2]: for map m (0 pred,
 *   1 gt) the order statistics of rank (N - 1) / 2 ([m][0], the lower middle) and N / 2 ([m][1], the upper middle; integer division,
 *   ranks from 0, ascending) of that map's values over the used pixels; the median is the mean of the two. N = 0: count 0 and four
 *   +0.0. The bit pattern of a positive finite float orders like an unsigned integer, so the statistic is found by a radix select
 *   over the four bytes of the key, the most significant first: a pass counts, per group and selection, the used keys that agree
 *   with the bytes found so far into 256 bins (privatised in LDS per workgroup, merged into ws with 32-bit integer atomic adds); a
 *   one-workgroup-per-group launch then walks the bins to the one that holds the rank, appends its byte and zeroes the bins for the
 *   next pass. Integer counts only: the result is a function of the multiset of used values and nothing else -- no schedule, grid
 *   size or arrival order of an atomic can change a byte of it. No sort, no compaction.
 *   ws: >= ovg_deptheval_median_workspace_bytes(groups, n) bytes, 16-byte aligned: per group four histograms of 256 u32 and eight u32
 *   of selection state, rounded up to 256; the entry zeroes it itself (a launch of its own). The query returns -1 outside the limits.
 *   OVG_E_ARG: NULL params / pred / gt / ws / out_count / out_median, sizes outside the limits, stride < n, a NaN or negative
 *   min_depth, a NaN max_depth, a pointer that is not 4-byte (out_count: 8-byte) aligned, a misaligned or undersized workspace.
 *
 * ovg_deptheval_sums: all arithmetic in float64, every operation rounded on its own (no fused multiply-add), p = (double)pred,
 *   g = (double)gt of a used pixel. The five TERMS of a pixel by mode:
 *   OVG_DEPTHEVAL_MOMENTS   [0] p   [1] g   [2] p p   [3] p g   [4] g g          (coeff, clip_min, clip_max are not read)
 *   OVG_DEPTHEVAL_METRICS   coeff f64 [G][2] = (s, t) on the device; q = s p + t; q = q > clip_min ? q : clip_min (a NaN becomes
 *                           clip_min); q = q < clip_max ? q : clip_max; e = q - g;
 *                           [0] |e| / g   [1] (e e) / g   [2] e e   [3] |e|   [4] d d with d = log q - log g
 *                           (clip_min > 0 and finite; clip_max >= clip_min, +inf allowed)
 *   out_counts int64 [G][4]: [0] the used pixels N; METRICS: [1..3] those with max(q / g, g / q) STRICTLY below 1.25, 1.5625 and
 *   1.953125 (1.25, 1.25^2, 1.25^3: exact in binary); MOMENTS: 0. out_sums f64 [G][5]: the sums of the terms over the used pixels
 *   of the group, in the order of ovg_align_moments:
 *   1. tile k of a group holds its pixels [OVG_DEPTHEVAL_TILE k, OVG_DEPTHEVAL_TILE (k + 1)) -- a tile never straddles two groups;
 *      thread t of its OVG_DEPTHEVAL_THREADS threads adds the terms of the pixels t, t + THREADS, ... of the tile in that order onto
 *      +0.0, skipping pixels that are not used or >= n;
 *   2. inside a wave of 64 lanes v[l] = v[l] + v[l + s] for s = 32, 16, 8, 4, 2, 1;
 *   3. the four wave sums combine as (w0 + w1) + (w2 + w3): the tile's partial, written to ws;
 *   4. a second launch, one workgroup per group, folds the group's partials the same way: thread t adds the partials of the tiles
 *      t, t + THREADS, ... in that order onto +0.0, then steps 2 and 3.
 *   No float atomics, no workgroup waits for another (stream order between the two launches is the only synchronisation): two calls
 *   give identical bytes. log is the device library's float64 logarithm: term [4] is the one output held to a bound, not to bytes.
 *   ws: >= ovg_deptheval_sums_workspace_bytes(groups, n) bytes, 16-byte aligned: OVG_DEPTHEVAL_PARTIAL_BYTES per tile, rounded up
 *   to 256; the query returns -1 outside the limits.
 *   OVG_E_ARG: as for the median (out_counts, out_sums, coeff: 8-byte aligned), an unknown mode, and in METRICS a NULL coeff, a NaN
 *   clip, clip_min that is not positive and finite, clip_max < clip_min.
 *
 * ovg_deptheval_solve: one thread per group, float64: (s, t) with gt ~ s pred + t, written to coeff f64 [G][2], status int32 [G].
 *   N = count[g count_stride] (count_stride in elements: 1 for out_count of the median, 4 for out_counts of the sums), the sums
 *   (Sp, Sg, Spp, Spg, Sgg) = sums[g][0..4] of OVG_DEPTHEVAL_MOMENTS, the medians out_median[g] of ovg_deptheval_median.
 *   OVG_DEPTHEVAL_NONE         (1, 0)
 *   OVG_DEPTHEVAL_MEDIAN       s = mg / mp with m = 0.5 ((double)lower + (double)upper) of each map; t = 0
 *   OVG_DEPTHEVAL_SCALE        s = Spg / Spp; t = 0                              (least squares through the origin)
 *   OVG_DEPTHEVAL_SCALE_SHIFT  det = N Spp - Sp Sp; s = (N Spg - Sp Sg) / det; t = (Sg - s Sp) / N      (least squares)
 *   DEGENERATE, in this order: N < 1, or N < 2 for SCALE_SHIFT (OVG_DEPTHEVAL_FEW); an input the mode reads -- the five sums for
 *   SCALE and SCALE_SHIFT, the four medians for MEDIAN -- is not finite (OVG_DEPTHEVAL_NOT_FINITE; both bits may be set together);
 *   then, only while no bit is set, SCALE_SHIFT with det not above OVG_DEPTHEVAL_SPREAD_EPS (2^-40) (N Spp)
 *   (OVG_DEPTHEVAL_NO_SPREAD: all used pred equal, or so close that the subtraction keeps fewer than 12 bits); then s or t not
 *   finite, or s <= 0 (OVG_DEPTHEVAL_BAD_FIT). A degenerate group gets (1, 0) and its bits; a NaN is never written.
 *   OVG_E_ARG: NULL params / count / coeff / status, count_stride < 1, groups outside the limits, an unknown mode, NULL sums for SCALE
 *   and SCALE_SHIFT, NULL median for MEDIAN, a pointer that is not 8-byte (median, status: 4-byte) aligned.
 * ------------------------------------------------------------------ */
enum { OVG_DEPTHEVAL_THREADS = 256, OVG_DEPTHEVAL_TILE = 1024, OVG_DEPTHEVAL_SUMS = 5, OVG_DEPTHEVAL_COUNTS = 4,
       OVG_DEPTHEVAL_PARTIAL_BYTES = 80, OVG_DEPTHEVAL_MAX_GROUPS = 4096,
       OVG_DEPTHEVAL_CHUNK = 16384,                /* pixels per workgroup of a histogram pass (speed only) */
       OVG_DEPTHEVAL_MEDIAN_GROUP_BYTES = 4128 };  /* 4 x 256 u32 bins + 8 u32 of state */
enum { OVG_DEPTHEVAL_MOMENTS = 0, OVG_DEPTHEVAL_METRICS = 1 };                                                    /* ovg_deptheval_sums_params.mode */
enum { OVG_DEPTHEVAL_NONE = 0, OVG_DEPTHEVAL_MEDIAN = 1, OVG_DEPTHEVAL_SCALE = 2, OVG_DEPTHEVAL_SCALE_SHIFT = 3 }; /* ovg_deptheval_solve_params.mode */
enum { OVG_DEPTHEVAL_FEW = 1, OVG_DEPTHEVAL_NOT_FINITE = 2, OVG_DEPTHEVAL_NO_SPREAD = 4, OVG_DEPTHEVAL_BAD_FIT = 8 }; /* status */
#define OVG_DEPTHEVAL_SPREAD_EPS 9.094947017729282e-13                               /* 2^-40 */
typedef struct {
  const float* pred; const float* gt; const uint8_t* valid;
  int64_t groups; int64_t n; int64_t stride;
  float min_depth; float max_depth;
  void* ws; int64_t ws_bytes;
  int64_t* out_count; float* out_median;
} ovg_deptheval_median_params;
int64_t ovg_deptheval_median_workspace_bytes(int64_t groups, int64_t n);
int ovg_deptheval_median(const ovg_deptheval_median_params*, void* stream);

typedef struct {
  const float* pred; const float* gt; const uint8_t* valid;
  int64_t groups; int64_t n; int64_t stride;
  float min_depth; float max_depth;
  int32_t mode; int32_t reserved;
  const double* coeff; double clip_min; double clip_max;
  void* ws; int64_t ws_bytes;
  int64_t* out_counts; double* out_sums;
} ovg_deptheval_sums_params;
int64_t ovg_deptheval_sums_workspace_bytes(int64_t groups, int64_t n);
int ovg_deptheval_sums(const ovg_deptheval_sums_params*, void* stream);

typedef struct {
  const int64_t* count; int64_t count_stride;
  const double* sums; const float* median;
  int64_t groups; int32_t mode; int32_t reserved;
  double* coeff; int32_t* status;
} ovg_deptheval_solve_params;
int ovg_deptheval_solve(const ovg_deptheval_solve_params*, void* stream);

/* ------------------------------------------------------------------ *
 * Plane segmentation by RANSAC (added under ABI 13): five entries that never read anything back -- seeded hypotheses, their inlier
 * counts over the whole cloud (the hot path: H hypotheses x n points), the winner, its inlier mask, and a least-squares refit from
 * the moments of ovg_align_moments. The rule names no schedule; tests/plane_twin.py restates it in numpy by brute force and the
 * device returns its bytes (the refit: within a bound, against numpy's eigh).
 *
 * A PLANE is four float32 values (nx, ny, nz, w) with |n| = 1; its points satisfy n.p + w = 0. The VOID plane is four NaNs.
 * RESIDUAL of a point (x, y, z), in float32 with every operation rounded on its own (no fused multiply-add):
 *     e = ((nx x + ny y) + nz z) + w
 * A point is USABLE when its valid byte (u8 [n], optional) is non-zero and its three coordinates are finite. It is an INLIER of a
 * plane at the threshold t (float32, finite, >= 0) iff it is usable and |e| <= t (inclusive). A NaN e is never an inlier, so the
 * void plane has none; neither has a plane with an infinite value.
 *
 * ovg_plane_hypotheses: one thread per hypothesis h < H.
 *   DRAWS: pos_j = ((mix(seed + 3 h + j) >> 32) * m) >> 32 for j = 0, 1, 2 in unsigned 64-bit arithmetic that wraps, mix = splitmix64:
 *     z += 0x9E3779B97F4A7C15; z = (z ^ z >> 30) * 0xBF58476D1CE4E5B9; z = (z ^ z >> 27) * 0x94D049BB133111EB; z ^= z >> 31
 *   (mix(0) = 0xE220A8397B1DCDAF). m is the number of candidates: the point index is i_j = candidates[pos_j] (int32 [m]), or pos_j
 *   itself without a candidate list (then m = n). index int32 [H][3] receives (i_0, i_1, i_2) as drawn, also for void hypotheses.
 *   PLANE: float64, one rounding per operation, a, b, c the points i_0, i_1, i_2 widened: u = b - a, v = c - a,
 *   n = (u1 v2 - u2 v1, u2 v0 - u0 v2, u0 v1 - u1 v0), l2 = (n0 n0 + n1 n1) + n2 n2, uu and vv the same of u and v. The hypothesis
 *   is VOID when an index is outside [0, n), two indices are equal, a point is not usable, l2 is not above (2^-20 uu) vv (a
 *   near-collinear triple: the sine of the angle at a is at most 2^-10) or, with an axis (f32 [3] on the device, used as given: the
 *   caller normalises it), |d| >= min_abs_cos does not hold for d = (nh0 a0 + nh1 a1) + nh2 a2, nh = n / sqrt(l2) per component
 *   (a NaN axis voids every hypothesis). Otherwise nh is ORIENTED: with an axis and d != 0 so that d > 0; without one, or at
 *   d == 0, so that its component of largest magnitude is positive, the lowest component on ties (ovg_knn_normals' rule);
 *   w = -((nh0 a0 + nh1 a1) + nh2 a2) with the oriented nh and the point a; the four values are rounded to float32 once.
 *   planes f32 [H][4]: the plane, or four NaNs (bits 0x7FC00000) for a void hypothesis.
 *   OVG_E_ARG: NULL params / points / planes / index, n or H outside [1, 2^31), with candidates m outside [1, 2^31), without m != n
 *   and m != 0, min_abs_cos outside [0, 1] or NaN (it must be 0 without an axis), a pointer that is not 4-byte aligned.
 *
 * ovg_plane_score: count int32 [H] = the number of inliers of planes[h] among the n points. A grid of (hypothesis tiles of
 *   OVG_PLANE_HYP_TILE) x (point splits); a workgroup keeps its planes and counters in registers, stages tiles of
 *   OVG_PLANE_POINT_TILE points in LDS (an unusable point as NaN) and every split adds its counters with one 32-bit integer atomic
 *   add per hypothesis onto the zeros a fill launch of the same call wrote. Integer sums do not depend on the order of arrival: two
 *   calls, and every `splits` (0: chosen by the entry; otherwise the number of point splits, clamped to the number of point
 *   tiles), give identical bytes.
 *   OVG_E_ARG: NULL params / points / planes / count, n or H outside [1, 2^31), threshold negative, infinite or NaN, splits < 0,
 *   a pointer that is not 4-byte aligned.
 *
 * ovg_plane_select: one workgroup. The WINNER is the hypothesis with the largest count, ties to the lowest h. There is NO PLANE when
 *   that count is below min_inliers (>= 3) or the winner's plane holds a non-finite value: best = -1, plane = four zeros and
 *   status = OVG_PLANE_NONE; otherwise best = h, plane = planes[h], status = 0. best_count receives the largest count either way
 *   (a negative count is read as 0). A NaN is never written to `plane`.
 *   OVG_E_ARG: NULL params / count / planes / best / plane / best_count / status, H outside [1, 2^31), min_inliers < 3, a pointer
 *   that is not 4-byte aligned.
 *
 * ovg_plane_mask: inlier u8 [n] (1 / 0) for the plane read from device memory (f32 [4]); distance (f32 [n], optional): the signed
 *   residual e, NaN (0x7FC00000) for an unusable point; out_count int64 [1]: the number of inliers, summed with integer atomics
 *   onto a zero the call writes itself. gate (int32 [1], optional): when it holds OVG_PLANE_NONE there is no plane -- no inlier,
 *   every distance NaN, count 0 -- whatever `plane` holds (ovg_plane_select's zeros would make every usable point an inlier).
 *   OVG_E_ARG: NULL params / points / plane / inlier / out_count, n outside [1, 2^31), a bad threshold, a pointer that is not
 *   4-byte (out_count: 8-byte) aligned.
 *
 * ovg_plane_fit: one thread: the least-squares plane through the inliers from their moments (count int64 [1], sums f64 [18],
 *   centre f64 [6] or NULL for zeros: ovg_align_moments with source == target == the points, source_valid = the inlier mask and
 *   centre = (g0, g0), so that a == b bit for bit). All float64, N = count:
 *   1. DEGENERATE when N < 3 (OVG_PLANE_FEW) or a sum or centre entry is not finite (OVG_PLANE_NOT_FINITE);
 *   2. C[r][c] = sums[6 + 3 r + c] - (sums[r] sums[c]) / N for r <= c: the scatter matrix of the inliers (their covariance times N);
 *      the centroid g[r] = sums[r] / N + centre[r];
 *   3. ovg_knn_normals' cyclic Jacobi: OVG_KNN_NORMALS_SWEEPS sweeps of the rotations (0,1) (0,2) (1,2); the column of the
 *      accumulated rotations under the smallest diagonal entry, the lowest on ties, divided by its length;
 *   4. DEGENERATE when the middle diagonal entry is not above 2^-40 times the largest (OVG_PLANE_NO_SPREAD: the inliers are
 *      collinear or coincide), or when the new plane holds a non-finite value (OVG_PLANE_NOT_FINITE);
 *   5. oriented as a hypothesis is (d from the axis f32 [3] when given; no min_abs_cos here), w = -((nh0 g0 + nh1 g1) + nh2 g2),
 *      rounded to float32 once and written over `plane`. A degenerate step leaves `plane` as it was.
 *   Optional outputs: out_rms f64 [1] = sqrt(max(smallest entry, 0) / N), the root mean square distance of the inliers to the new
 *   plane; out_eigen f64 [3], the diagonal entries ascending (both zeros for a degenerate step); status int32 [1], the OVG_PLANE_FEW
 *   / NO_SPREAD / NOT_FINITE bits of this step, 0 for a regular one.
 *   OVG_E_ARG: NULL params / count / sums / plane, a pointer that is not 8-byte (plane, axis, status: 4-byte) aligned.
 * Nothing is written when an entry returns OVG_E_ARG.
 * ------------------------------------------------------------------ */
enum { OVG_PLANE_HYP_TILE = 512, OVG_PLANE_POINT_TILE = 512 };
enum { OVG_PLANE_NONE = 1, OVG_PLANE_FEW = 2, OVG_PLANE_NO_SPREAD = 4, OVG_PLANE_NOT_FINITE = 8 };   /* status bits */
#define OVG_PLANE_COLLINEAR_EPS 9.5367431640625e-07                                  /* 2^-20 */
#define OVG_PLANE_SPREAD_EPS 9.094947017729282e-13                                   /* 2^-40 */
typedef struct {
  const float* points; const uint8_t* valid;
  const int32_t* candidates; const float* axis;
  int64_t n; int64_t m; int64_t H;
  uint64_t seed;
  float min_abs_cos; int32_t pad;
  float* planes; int32_t* index;
} ovg_plane_hypotheses_params;
int ovg_plane_hypotheses(const ovg_plane_hypotheses_params*, void* stream);

typedef struct {
  const float* points; const uint8_t* valid; const float* planes;
  int64_t n; int64_t H;
  float threshold; int32_t splits;
  int32_t* count;
} ovg_plane_score_params;
int ovg_plane_score(const ovg_plane_score_params*, void* stream);

typedef struct {
  const int32_t* count; const float* planes;
  int64_t H;
  int32_t min_inliers; int32_t pad;
  int32_t* best; float* plane; int32_t* best_count; int32_t* status;
} ovg_plane_select_params;
int ovg_plane_select(const ovg_plane_select_params*, void* stream);

typedef struct {
  const float* points; const uint8_t* valid; const float* plane; const int32_t* gate;
  int64_t n;
  float threshold; int32_t pad;
  uint8_t* inlier; float* distance; int64_t* out_count;
} ovg_plane_mask_params;
int ovg_plane_mask(const ovg_plane_mask_params*, void* stream);

typedef struct {
  const int64_t* count; const double* sums; const double* centre; const float* axis;
  float* plane;
  double* out_rms; double* out_eigen; int32_t* status;
} ovg_plane_fit_params;
int ovg_plane_fit(const ovg_plane_fit_params*, void* stream);

/* ------------------------------------------------------------------ *
 * Volumetric fusion (added under ABI 13): S depth maps with their cameras are averaged into a dense truncated signed-distance (TSDF)
 * volume, and one mesh is extracted from its zero level by naive surface nets. Both rules are exact: tests/tsdf_twin.py restates
 * them in numpy float32 and the device returns its bytes. Every step is one f32 operation rounded on its own (no fused
 * multiply-add); min(a, b) is `a < b ? a : b`; divisions and the square root are correctly rounded.
 *
 * The VOLUME is dense and caller-owned: tsdf [nz][ny][nx] f32 and weight [nz][ny][nx] f32, optionally color [nz][ny][nx][4] f32
 * (r, g, b in [0, 255] and the colour weight). Lattice point (i, j, k) lies at origin + voxel * (i, j, k). A FRESH volume is
 * tsdf = 1 and everything else 0.
 *
 * ovg_tsdf_integrate: one thread per lattice point, the views view_first .. view_first + view_count - 1 in ascending order.
 *   depth [S][H][W] f32 z-depth; cams [S][16] f32 packed as for ovg_render_points; valid [S][H][W] u8, obs_weight [S][H][W] f32 and
 *   colors [S][H][W][3] u8 are optional (NULL). Per lattice point and view:
 *   1. p = origin + voxel * (f32) index per axis: one multiply, one add;
 *   2. rules 1-3 of ovg_render_points give zc and the pixel (u, w); the view is skipped when the point is culled (a camera
 *      coordinate is not finite, zc <= near) or unless 0 <= u <= W - 1 and 0 <= w <= H - 1 (compared in f32: NaN fails);
 *   3. d = depth[s][w][u]; skipped unless valid[s][w][u] != 0 (when given), d is finite and d > near. wobs = obs_weight[s][w][u]
 *      when given (skipped unless it is finite and > 0), else 1;
 *   4. sdf = d - zc; skipped when sdf < -trunc (the point is hidden behind the surface). t = min(sdf / trunc, 1);
 *   5. Wn = W + wobs; T = (T * W + t * wobs) / Wn; W = min(Wn, max_weight);
 *   6. with colors and a colour volume, and sdf <= trunc (free-space observations do not colour a voxel): Cn = Cw + wobs;
 *      ch = (ch * Cw + (f32) colour * wobs) / Cn for r, g, b; Cw = min(Cn, max_weight).
 *   The state of a lattice point is read once, kept in registers across the view loop and written once; there are no atomics, no
 *   workspace, no LDS and no scratch. Two calls give identical bytes, and a call over the views [0, S) gives the bytes of two
 *   calls over [0, k) and [k, S): that is the incremental form. Camera rows are wave-uniform scalar loads.
 *   tile: the 256 lattice points of a workgroup as an x x y x z brick (OVG_TSDF_TILE_DEFAULT is the brick DESIGN.md names). It
 *   changes speed only, never a byte.
 *   Nearest-pixel depth lookup only: no bilinear depth, no de-integration, no hashed or sparse volume.
 *   OVG_E_ARG (before the first HIP call; nothing is written): NULL params / tsdf / weight / depth / cams, colors without a colour
 *   volume, nx, ny, nz, S, H, W <= 0, nx ny nz >= 2^31, S H W >= 2^31, a view range outside [0, S) or empty, voxel / trunc /
 *   max_weight / near not positive and finite, an origin that is not finite, an unknown tile, a pointer that is not 4-byte (the
 *   colour volume: 16-byte) aligned.
 *
 * ovg_tsdf_extract: the mesh of the zero level by naive surface nets; no case table.
 *   A lattice point is OBSERVED when W >= min_weight (min_weight > 0, finite) and INSIDE when T < 0 (so -0 and NaN are outside).
 *   Corner c = dx + 2 dy + 4 dz of the cell (i, j, k), i < nx - 1, j < ny - 1, k < nz - 1, is the lattice point (i + dx, j + dy,
 *   k + dz). The 12 EDGES of a cell in their fixed order, as (lower corner a, upper corner b): the x edges (0,1) (2,3) (4,5) (6,7),
 *   the y edges (0,2) (1,3) (4,6) (5,7), the z edges (0,4) (1,5) (2,6) (3,7).
 *   A cell is ACTIVE when its 8 corners are observed and their insides are mixed. It owns one vertex:
 *   - every edge whose endpoints differ in `inside` contributes its crossing r = Ta / (Ta - Tb) as the local offset of a with r
 *     in place of the edge's axis; the offsets are summed per component in f32 in edge order (from 0) and divided by their number;
 *     position = origin + voxel * ((f32) index + offset) per axis;
 *   - normal: g = per axis the four differences Tb - Ta of that axis' edges, ((d0 + d1) + d2) + d3; l = sqrt((gx gx + gy gy) +
 *     gz gz); g / l when l > 0, else (0, 0, 0). It points from inside to outside;
 *   - colour: the corners c = 0 .. 7 with colour weight > 0, their r, g, b summed in f32 in that order and divided by their
 *     number, then floor(x + 0.5) clamped to [0, 255] (NaN gives 0); OVG_TSDF_GREY in all three channels when there are none or
 *     the volume has no colours.
 *   Vertices leave in ascending cell index (k ny + j) nx + i. Every lattice EDGE from the point (i, j, k) along the axis a, in
 *   ascending (lattice index, axis), with two observed endpoints that differ in `inside`, whose four surrounding cells exist and
 *   are active, emits one quad: with b = (a + 1) % 3, c = (a + 2) % 3 the vertices v0 .. v3 of the cells at the offsets (-1, -1),
 *   (0, -1), (0, 0), (-1, 0) along (b, c) -- counter-clockwise seen from +a -- in that order when the lower endpoint is the
 *   inside one, else as (v0, v3, v2, v1); the quad (q0, q1, q2, q3) leaves as the triangles (q0, q1, q2), (q0, q2, q3). The triangle
 *   normals point from inside to outside: the signed volume of an enclosed solid is positive.
 *   stage OVG_TSDF_COUNT: the active cells, the quads of every lattice point, per-workgroup counts and their scans into ws;
 *   out_count[0] = M vertices, out_count[1] = Q quads (two int64, device). stage OVG_TSDF_SCATTER reads what COUNT left in ws and
 *   writes vertices [M][3] f32, normals [M][3] f32, colors [M][3] u8 and faces [2 Q][3] int32; vertices at positions >=
 *   vertex_capacity and quads at positions >= quad_capacity are dropped (a face may then name a dropped vertex). Both stages in
 *   one call need the capacities known in advance; the usual form is COUNT, read the counts, allocate, SCATTER with the same ws.
 *   A volume without a crossing, or with an axis of length 1, gives M = Q = 0 and OVG_OK. No atomics: two calls give identical bytes.
 *   ws: >= ovg_tsdf_extract_workspace_bytes(nx, ny, nz) bytes (an int32 vertex-index volume, one byte per lattice point and two
 *   int64 per 256 lattice points, each part rounded up to 256), 16-byte aligned; the query returns -1 for nx, ny, nz <= 0 or
 *   nx ny nz >= 2^31.
 *   OVG_E_ARG (nothing is written): NULL params / tsdf / weight / ws / out_count, bad nx, ny, nz, voxel not positive and finite,
 *   an origin that is not finite, min_weight not positive and finite, an unknown stage, in SCATTER a negative capacity or a NULL
 *   vertices / normals / colors (vertex_capacity > 0) or faces (quad_capacity > 0), a misaligned pointer or an undersized workspace.
 *   Not in it: marching cubes, ray-casting the volume, mesh smoothing or decimation.
 * ------------------------------------------------------------------ */
enum { OVG_TSDF_TILE_DEFAULT = 0, OVG_TSDF_TILE_256x1x1 = 1, OVG_TSDF_TILE_8x8x4 = 2, OVG_TSDF_TILE_16x4x4 = 3, OVG_TSDF_TILE_32x8x1 = 4 };
enum { OVG_TSDF_COUNT = 1, OVG_TSDF_SCATTER = 2 };
enum { OVG_TSDF_GREY = 128, OVG_TSDF_EXTRACT_BLOCK = 256 };
typedef struct {
  float* tsdf; float* weight; float* color;
  int32_t nx; int32_t ny; int32_t nz;
  float origin[3]; float voxel; float trunc; float max_weight; float near;
  const float* depth; const float* cams; const uint8_t* valid; const float* obs_weight; const uint8_t* colors;
  int32_t S; int32_t H; int32_t W;
  int32_t view_first; int32_t view_count;
  int32_t tile;
} ovg_tsdf_integrate_params;
int ovg_tsdf_integrate(const ovg_tsdf_integrate_params*, void* stream);

typedef struct {
  const float* tsdf; const float* weight; const float* color;
  int32_t nx; int32_t ny; int32_t nz;
  float origin[3]; float voxel; float min_weight;
  int32_t stage; int32_t pad;
  int64_t vertex_capacity; int64_t quad_capacity;
  float* vertices; float* normals; uint8_t* colors; int32_t* faces; int64_t* out_count;
  void* ws; int64_t ws_bytes;
} ovg_tsdf_extract_params;
int64_t ovg_tsdf_extract_workspace_bytes(int32_t nx, int32_t ny, int32_t nz);
int ovg_tsdf_extract(const ovg_tsdf_extract_params*, void* stream);

/* ------------------------------------------------------------------ *
 * Image-space map geometry (added under ABI 13): what follows from the prediction being IMAGES -- depth / world_points are [S][H][W]
 * maps in which a pixel's neighbours are known for free. Four entries, all stencils over the maps plus one ordered compaction, by
 * exact rules that tests/mapgeom_twin.py restates in numpy; the device returns the twin's bytes. Every f32 step is one operation
 * rounded on its own (no fused multiply-add), divisions and square roots are correctly rounded, comparisons with NaN fail.
 * Pixel (s, y, x) has the flat index g = (s H + y) W + x. A stencil never leaves its view: neither the previous row's last pixel nor
 * the neighbouring view's rows are ever neighbours. Nothing is allocated, nothing is read back, all work goes to the caller's stream,
 * there are no atomics, two calls give identical bytes. Every entry answers OVG_E_ARG before its first HIP call (nothing is written)
 * to NULL params, S, H, W <= 0 or S H W >= 2^31, a pointer that is not aligned to its element, and to what its paragraph lists.
 *
 * ovg_map_depth: the usable-depth map z [S][H][W] f32, which the three other entries read and nothing else to decide usability.
 *   Exactly one of two inputs: points [S][H][W][3] with cams [S][16] (packed as for ovg_render_points), then z = camera_depth() of
 *   csrc/ovg_project.h = ((c6 x + c7 y) + c8 z) + c11, rule 1 of ovg_multiview_consistency; or depth [S][H][W], then z = depth.
 *   valid [S][H][W] u8 is optional. A pixel is USABLE when valid != 0 (if given), z is finite and z > near; z[g] is that value for a
 *   usable pixel and the quiet NaN 0x7FC00000 otherwise. One thread per pixel, blockIdx.y = view (the camera row is wave-uniform).
 *   OVG_E_ARG also: both or neither of points / depth, points without cams, NULL z, near not positive and finite.
 *
 * ovg_map_normals: normals [S][H][W][3] f32 from the point map P = points and z.
 *   A neighbour q of p (same view, one step along a row or a column) is USABLE FOR p when z[q] is not NaN, the three coordinates
 *   of P[q] are finite and |z[q] - z[p]| <= rel_tol * z[p]: one subtraction, one multiplication, inclusive; rel_tol = +inf switches
 *   the test off (the product is +inf).
 *   Horizontal difference dh (three f32 subtractions): P[x+1] - P[x-1] when both sides are usable for p, else P[x+1] - P[x] when the
 *   right one is, else P[x] - P[x-1] when the left one is, else none. Vertical difference dv likewise along y (y+1 is "right").
 *   p has NO NORMAL -- (0, 0, 0) is written -- when z[p] is NaN, a coordinate of P[p] is not finite, or either difference is missing.
 *   Otherwise dh, dv are widened to float64 and n = dv x dh: nx = dv.y dh.z - dv.z dh.y, ny = dv.z dh.x - dv.x dh.z, nz = dv.x dh.y -
 *   dv.y dh.x, every product and difference one float64 operation. With x to the right, y down and the camera looking along +z this
 *   points back towards the camera: the "inside to outside" convention of the meshes. No camera is needed (a world point map differs
 *   from camera coordinates by a proper rotation). l = sqrt((nx nx + ny ny) + nz nz) in float64; the output is n / l (float64
 *   division) rounded to f32 when l is finite and > 0, else (0, 0, 0). One thread per pixel, no LDS: five point reads per pixel.
 *   OVG_E_ARG also: NULL points / z / normals, rel_tol negative or NaN.
 *
 * ovg_map_edges: flags [S][H][W] u8, bits OVG_MAP_UNUSABLE, OVG_MAP_DEPTH_EDGE, OVG_MAP_NORMAL_EDGE, OVG_MAP_NO_NORMAL.
 *   The WINDOW of p is the (2 radius + 1)^2 block around it clipped to the view, radius in {1, 2, 3}; only its usable pixels (z not
 *   NaN) count, p included. A pixel whose z is NaN carries OVG_MAP_UNUSABLE alone. Otherwise:
 *   - DEPTH_EDGE when zmax - zmin > rel_tol * z[p], zmax / zmin over the window: one subtraction, one multiplication, strict, no
 *     division; rel_tol = +inf never flags;
 *   - with normals [S][H][W][3] (optional): NO_NORMAL when all three components of n[p] equal 0; otherwise NORMAL_EDGE when any usable
 *     q of the window whose normal is not (0, 0, 0) has (n[p].x n[q].x + n[p].y n[q].y) + n[p].z n[q].z < min_cos (f32). The caller
 *     converts an angle to min_cos (in float64, rounded once to f32); min_cos = -inf never flags.
 *   tile: OVG_MAP_TILE_256x1 is the plain form, 256 consecutive pixels of a view per workgroup and every window read from global
 *   memory; the others stage the workgroup's width x height tile plus its halo of z (and the normals) in LDS once and read the up
 *   to 49 window pixels from there. OVG_MAP_TILE_DEFAULT is the one DESIGN.md 12n names. The tile changes speed only, never a byte.
 *   OVG_E_ARG also: NULL z / flags, radius outside {1, 2, 3}, rel_tol negative or NaN, with normals a NaN min_cos, an unknown tile.
 *
 * ovg_map_triangulate: the grid mesh of the S views -- two triangles per pixel quad, the faces that are not wanted dropped, the
 * vertices compacted -- in two stages in the shape of ovg_tsdf_extract.
 *   A pixel is a CORNER when z is not NaN, the three coordinates of points are finite and keep != 0 (keep [S][H][W] u8, optional).
 *   The quad of (y, x), x < W - 1, y < H - 1, has a = (y, x), b = (y, x+1), c = (y+1, x), d = (y+1, x+1) and offers the faces
 *   0: (a, c, b) and 1: (b, c, d): the diagonal is fixed at b-c, as in the reference's pts3d_to_trimesh, and the winding is such
 *   that the triangle normal faces the camera (the direction of ovg_map_normals). A face is EMITTED when its three pixels are corners
 *   and it is not TORN: (max z - min z of the three) > rel_tol * (min z of the three), one subtraction, one multiplication, strict;
 *   rel_tol = +inf never tears. Faces leave in ascending (view, y, x, which of the two); a quad never spans two rows' ends or two
 *   views. VERTICES are the pixels that an emitted face names, in ascending flat index; a pixel decides that from the at most six
 *   faces around it (0 of its own quad, 0 and 1 of the quad to its left, 0 and 1 of the quad above, 1 of the quad above left).
 *   stage OVG_MAP_COUNT: the face bits of every quad, the referenced pixels, per-workgroup counts (OVG_MAP_BLOCK pixels each) and
 *   their scans into ws; out_count[0] = M vertices, out_count[1] = F faces (two int64, device). stage OVG_MAP_SCATTER reads what
 *   COUNT left in ws and writes per vertex out_vertices [M][3] f32 (the point as it is), out_normals [M][3] f32 (the pixel of normals
 *   [S][H][W][3] f32 as it is; (0, 0, 0) without), out_colors [M][3] u8 (the pixel of colors [S][H][W][3] u8; OVG_TSDF_GREY
 *   without) and out_pixel_index [M] int64 (g), and out_faces [F][3] int32 indices into the vertices. Vertices at positions >=
 *   vertex_capacity and faces at positions >= face_capacity are dropped (a face may then name a dropped vertex). Both stages in one
 *   call need the capacities known in advance; the usual form is COUNT, read the counts, allocate, SCATTER with the same ws. Maps
 *   without a face (H or W of 1, nothing usable) give M = F = 0 and OVG_OK.
 *   ws: >= ovg_map_triangulate_workspace_bytes(S, H, W) bytes (an int32 vertex index and one byte per pixel and two int64 per
 *   OVG_MAP_BLOCK pixels, each part rounded up to 256), 16-byte aligned; the query returns -1 for S, H, W <= 0 or S H W >= 2^31.
 *   OVG_E_ARG also: NULL z / points / ws / out_count, rel_tol negative or NaN, an unknown stage, in SCATTER a negative capacity or a
 *   NULL out_vertices / out_normals / out_colors / out_pixel_index (vertex_capacity > 0) or out_faces (face_capacity > 0), a
 *   misaligned or undersized workspace.
 *   Not in it: the reference's second, backward copy of every face (ovg_render_mesh draws both sides), per-face colours, smoothing.
 * ------------------------------------------------------------------ */
enum { OVG_MAP_UNUSABLE = 1, OVG_MAP_DEPTH_EDGE = 2, OVG_MAP_NORMAL_EDGE = 4, OVG_MAP_NO_NORMAL = 8 };
enum { OVG_MAP_TILE_DEFAULT = 0, OVG_MAP_TILE_256x1 = 1, OVG_MAP_TILE_16x16 = 2, OVG_MAP_TILE_32x8 = 3, OVG_MAP_TILE_64x4 = 4 };
enum { OVG_MAP_COUNT = 1, OVG_MAP_SCATTER = 2 };
enum { OVG_MAP_BLOCK = 256, OVG_MAP_MAX_RADIUS = 3 };
typedef struct {
  const float* points; const float* cams; const float* depth; const uint8_t* valid;
  int32_t S; int32_t H; int32_t W; float near;
  float* z;
} ovg_map_depth_params;
int ovg_map_depth(const ovg_map_depth_params*, void* stream);

typedef struct {
  const float* points; const float* z;
  int32_t S; int32_t H; int32_t W; float rel_tol;
  float* normals;
} ovg_map_normals_params;
int ovg_map_normals(const ovg_map_normals_params*, void* stream);

typedef struct {
  const float* z; const float* normals;
  int32_t S; int32_t H; int32_t W; int32_t radius;
  float rel_tol; float min_cos; int32_t tile; int32_t pad;
  uint8_t* flags;
} ovg_map_edges_params;
int ovg_map_edges(const ovg_map_edges_params*, void* stream);

typedef struct {
  const float* z; const float* points; const uint8_t* keep; const float* normals; const uint8_t* colors;
  int32_t S; int32_t H; int32_t W; float rel_tol;
  int32_t stage; int32_t pad;
  int64_t vertex_capacity; int64_t face_capacity;
  float* out_vertices; float* out_normals; uint8_t* out_colors; int64_t* out_pixel_index; int32_t* out_faces; int64_t* out_count;
  void* ws; int64_t ws_bytes;
} ovg_map_triangulate_params;
int64_t ovg_map_triangulate_workspace_bytes(int32_t S, int32_t H, int32_t W);
int ovg_map_triangulate(const ovg_map_triangulate_params*, void* stream);

/* ------------------------------------------------------------------ *
 * Mesh simplification (added under ABI 13): vertex clustering on a uniform grid (Rossignac-Borrel) with degenerate and duplicate faces
 * removed, by an exact rule that names no schedule and that tests/meshsimp_twin.py restates in numpy bit for bit.
 *   vertices [M][3] f32, faces [F][3] int32, normals [M][3] f32 (optional), colors [M][3] u8 (optional); voxel: DEVICE f32 scalar,
 *   the cell edge v. 1 <= M < 2^31, 1 <= F < 2^32 - 1.
 *   1. a vertex is VALID when its three coordinates are finite;
 *   2. the grid is the one of ovg_voxel_downsample: origin = component-wise minimum of the valid vertices; per axis g = (p - origin) / v
 *      in f32 (one subtraction, one correctly rounded division) and the cell c = floor(g). A valid vertex with any c > 2^21 - 1 raises
 *      OVG_MS_OVERFLOW, a v that is not a positive finite number OVG_MS_BAD_VOXEL; a call that raised either keeps nothing;
 *   3. the LEADER of a cell is its lowest valid vertex index;
 *   4. a face is LIVE when its three indices lie in [0, M) and its three vertices are valid; a live face whose three cells are not
 *      pairwise different is dropped as DEGENERATE;
 *   5. two live, non-degenerate faces with the same unordered set of three cells are DUPLICATES: the lowest input face index survives
 *      and keeps its own corner order (an opposite-facing copy disappears too);
 *   6. one output vertex per cell that a surviving face names, in ascending leader index; cells of unreferenced or all-degenerate
 *      geometry produce nothing;
 *   7. the output faces are the survivors in input order, int32, corners mapped to output vertex numbers;
 *   8. position OVG_MS_POS_FIRST: the leader's own twelve bytes;
 *   9. position OVG_MS_POS_MEAN: per valid vertex and axis r = g - c in f32 (exact, in [0, 1)), q = llrint((double)r * 2^24) (to
 *      nearest, ties to even), Q = sum of q over the cell (int64), n = the cell's valid vertices; the output coordinate is
 *      (float)((double)origin + (double)v * ((double)c + (double)Q / ((double)n * 16777216.0))), every operation rounded on its own, in
 *      that order, in float64: a mean that does not depend on the order of the vertices;
 *  10. colours: per channel (2 S + n) / (2 n) in integers, S the channel's sum over the cell: the mean rounded half up;
 *  11. normals: a vertex's normal takes part when its three components are finite and each has magnitude <= 4; per component the sum
 *      of llrint((double)x * 2^20) in int64; the output is that integer vector (nx, ny, nz) as float64 divided by
 *      l = sqrt((nx nx + ny ny) + nz nz) (the order of ovg_map_normals) and rounded to f32 when l is finite and > 0, else (0, 0, 0);
 *  12. out_source_index [M'] int64 is the leader's input index, out_vertex_count [M'] int32 the cell's n (both optional).
 *   stage OVG_MS_COUNT: both tables, the sums, the keep bytes, the ranks and the scans into ws; out_count[0..5] = M', F', the OVG_MS_*
 *   flags raised, the occupied cells, the degenerate faces, the duplicate faces that were dropped (six int64, device; the last three
 *   are 0 in a flagged call). stage OVG_MS_SCATTER reads what COUNT left in ws and writes the first vertex_capacity vertices
 *   (out_vertices, with normals out_normals, with colors out_colors -- each output required exactly when its input is given --,
 *   out_source_index, out_vertex_count) and the first face_capacity faces (out_faces; a face may then name a dropped vertex).
 *   Cell table: open addressing, linear probing, max(1024, 2 M) slots; the 63-bit cell key is claimed by a 64-bit compare-and-swap;
 *   leader (32-bit min), n and the nine integer sums live in arrays indexed by the slot, every vertex stores its slot once. Face
 *   table: max(1024, 2 F) slots of one 32-bit face index; a prober compares its sorted triple of cell slots with the triple of the
 *   face the slot names and issues one 32-bit min of its own index when they agree. Integer atomics only (relaxed, agent scope): no
 *   result depends on arrival order, two runs give identical bytes. Nothing is allocated, nothing is read back, every launch goes to
 *   the caller's stream.
 *   ws: >= ovg_mesh_simplify_workspace_bytes(M, F) bytes, 16-byte aligned: with C = max(1024, 2 M), T = max(1024, 2 F), tv =
 *   ceil(M / 4096), tf = ceil(F / 4096) the parts 256, 8 C, 4 C, 4 C, 4 C, 72 C, 4 M, M, 4 T, F, 8 tv, 8 tv, 8 tf, 8 tf, each rounded
 *   up to 256. The query returns -1 for M <= 0, F <= 0, M >= 2^31 or F >= 2^32 - 1.
 *   OVG_E_ARG before the first HIP call: NULL params / vertices / faces / voxel / ws, sizes outside the limits, an unknown stage or
 *   position, COUNT without out_count, in SCATTER a negative capacity, a NULL out_vertices (vertex_capacity > 0) or out_faces
 *   (face_capacity > 0), out_normals / out_colors not matching normals / colors, a pointer that is not aligned to its element, a
 *   misaligned or undersized workspace.
 *   Not in it: quadric placement, edge collapse, smoothing, a guarantee of manifoldness (clustering can pinch a surface).
 * ------------------------------------------------------------------ */
enum { OVG_MS_COUNT = 1, OVG_MS_SCATTER = 2 };
enum { OVG_MS_OVERFLOW = 1, OVG_MS_BAD_VOXEL = 2 };
enum { OVG_MS_POS_MEAN = 0, OVG_MS_POS_FIRST = 1 };
typedef struct {
  const float* vertices; const int32_t* faces; const float* normals; const uint8_t* colors; const float* voxel;
  int64_t num_vertices; int64_t num_faces;
  int32_t stage; int32_t position;
  int64_t vertex_capacity; int64_t face_capacity;
  float* out_vertices; float* out_normals; uint8_t* out_colors; int64_t* out_source_index; int32_t* out_vertex_count;
  int32_t* out_faces; int64_t* out_count;
  void* ws; int64_t ws_bytes;
} ovg_mesh_simplify_params;
int64_t ovg_mesh_simplify_workspace_bytes(int64_t vertices, int64_t faces);
int ovg_mesh_simplify(const ovg_mesh_simplify_params*, void* stream);

/* ------------------------------------------------------------------ *
 * Mesh cleaning (added under ABI 13): connected components and edge statistics (ovg_mesh_topology), an ordered sub-mesh
 * (ovg_mesh_select) and Laplacian / Taubin smoothing with vertex normals (ovg_mesh_smooth), by exact rules that name no schedule and
 * that tests/meshops_twin.py restates in numpy bit for bit.
 *   vertices [M][3] f32, faces [F][3] int32. 1 <= M < 2^31, 1 <= F < 2^31.
 *   1. a vertex is VALID when its three coordinates are finite;
 *   2. a face is LIVE when its three indices lie in [0, M), are pairwise different and name valid vertices; a face of zero area with
 *      three different indices is live;
 *   3. a vertex is REFERENCED when a live face names it;
 *   4. a live face has three EDGES, its unordered index pairs; an edge's multiplicity is the number of live faces that hold it (a
 *      duplicated face counts twice). A BOUNDARY edge has multiplicity 1, a NON-MANIFOLD edge multiplicity >= 3; a vertex carries
 *      OVG_MT_BOUNDARY when it ends a boundary edge and OVG_MT_NONMANIFOLD when it ends a non-manifold edge;
 *   5. two referenced vertices are CONNECTED when a live face names both; the components are the transitive closure, each named by
 *      its LOWEST vertex index. This is vertex connectivity: two faces that meet in one corner only are one component (Open3D's
 *      cluster_connected_triangles joins faces across shared edges only and would split them).
 *
 * ovg_mesh_topology: vertex_root [M] int32 (the component's lowest vertex index, -1 for an unreferenced vertex), face_root [F] int32
 *   (-1 for a face that is not live), vertex_flags [M] u8 (OVG_MT_REFERENCED | OVG_MT_BOUNDARY | OVG_MT_NONMANIFOLD) and out_count
 *   [8] int64 on the device: live faces, referenced vertices, distinct edges, boundary edges, non-manifold edges, boundary vertices,
 *   non-manifold vertices, status flags. The one status flag is OVG_MT_INTERNAL, raised like OVG_CL_INTERNAL when the union-find
 *   leaves its bounds: a bug ends as an error, never as a hang. Components: the lock-free union-find of ovg_cluster (csrc/ovg_geom.h
 *   carries it with its proof) over (a, b) and (b, c) of every live face; vertex_root is its parent array while the launches run.
 *   Edges: open addressing, linear probing, E = max(1024, 6 F) slots; the key (lo << 32 | hi) is claimed by a 64-bit compare-and-swap,
 *   a 32-bit count per slot; one pass over the slots derives the edge counts and ORs the vertex flags.
 *   ws: >= ovg_mesh_topology_workspace_bytes(M, F) bytes, 16-byte aligned: the parts 256, 4 M, 8 E, 4 E, each rounded up to 256.
 *
 * ovg_mesh_select: a face SURVIVES when it is live, face_keep[f] != 0 (where face_keep is given) and vertex_keep != 0 at its three
 *   corners (where vertex_keep is given). One output vertex per vertex a surviving face names, in ascending input index; the
 *   surviving faces in input order, corners mapped to output numbers.
 *   stage OVG_MSEL_COUNT: the keep bytes, the ranks and the scans into ws; out_count[0..1] = M', F' (two int64, device). stage
 *   OVG_MSEL_SCATTER reads what COUNT left in ws and writes the first vertex_capacity entries of out_vertices [.][3] f32 (the input's
 *   twelve bytes) and out_source_index [.] int64 (optional), and the first face_capacity entries of out_faces [.][3] int32 and
 *   out_face_index [.] int64 (optional). Other attributes are gathered by the caller through out_source_index.
 *   ws: >= ovg_mesh_select_workspace_bytes(M, F) bytes, 16-byte aligned: with tv = ceil(M / 4096), tf = ceil(F / 4096) the parts M,
 *   F, 4 M, 8 tv, 8 tv, 8 tf, 8 tf, each rounded up to 256.
 *
 * ovg_mesh_smooth: `iterations` times one step with factor lambda and, when mu != 0, a second step with factor mu (Taubin; mu == 0 is
 *   plain Laplacian smoothing). The live set, the flags and the neighbour multisets are fixed from the INPUT. A vertex is MOVABLE
 *   when it is valid, referenced, fixed[i] == 0 (where fixed is given) and, with fix_boundary != 0, no OVG_MT_BOUNDARY vertex; every
 *   other vertex keeps its twelve input bytes through every step. One step with factor f on the current positions P, every operation
 *   rounded on its own, in float64 unless it says otherwise:
 *   a. frame: o = component-wise minimum and max = component-wise maximum of the current positions of the valid vertices (integer
 *      min / max of order-preserving keys: exact and order-free); ext = the largest over the axes of (double)max - (double)o; e = the
 *      binary exponent of ext as frexp gives it (ext = mantissa * 2^e, mantissa in [0.5, 1)), e = 0 for ext = 0; u = 2^(e - 30). A
 *      current coordinate of a valid vertex that is not finite raises OVG_MSM_NONFINITE in out_status; the outputs are then unspecified;
 *   b. per valid vertex and axis q = llrint(((double)p - (double)o) / u), to nearest, ties to even; 0 <= q <= 2^30;
 *   c. the neighbour multiset of vertex a holds b and c once for EVERY live face that names a, b and c, whatever the corner order: on
 *      a manifold interior every neighbour appears twice and the mean is the umbrella mean; duplicated faces and non-manifold edges
 *      weigh in by multiplicity. S = the int64 sum of the neighbours' q per axis, n = the multiset's size (n <= 2 F < 2^32, |S| < 2^62);
 *   d. a movable vertex moves to p' = (float)((double)p + (double)f * (m - (double)p)) with m = (double)o + u * ((double)S / (double)n).
 *   out_vertices [M][3] f32. out_normals [M][3] f32 (optional), from the final positions: per live face d1 = (double)pb - (double)pa,
 *   d2 = (double)pc - (double)pa, c = (d1y d2z - d1z d2y, d1z d2x - d1x d2z, d1x d2y - d1y d2x), l = sqrt((cx cx + cy cy) + cz cz); a
 *   face with l finite and > 0 adds llrint(c_k / l * 2^20) per component to the int64 sums of its three vertices; the output is
 *   normalised exactly as rule 11 of ovg_mesh_simplify, a vertex without such a face gets (0, 0, 0). iterations == 0 copies the
 *   vertices and only computes normals. out_status [1] int64: the OVG_MSM_* flags raised.
 *   The neighbour multisets are a CSR adjacency built once per call (integer atomics count and fill; the order inside a row may differ
 *   from run to run, which integer sums do not see); a step is then a gather without atomics: q in one 16-byte record per vertex, one
 *   thread per vertex, a row of more than 64 neighbours summed by the thread's whole wave. The frame of the next step is reduced by
 *   the update of the one before.
 *   ws: >= ovg_mesh_smooth_workspace_bytes(M, F) bytes, 16-byte aligned: with E and tv as above the parts 256, 4 M, 8 E, 4 E, 4 M,
 *   8 (M + 1), 8 tv, 8 tv, 24 F, 16 M, 24 M, each rounded up to 256.
 *
 * All three: integer atomics only (relaxed, agent scope): no result depends on arrival order, two runs give identical bytes. Every
 * loop is bounded and no workgroup waits for another. Nothing is allocated, nothing is read back, every launch goes to the caller's
 * stream. The three queries return -1 for M <= 0, F <= 0, M >= 2^31 or F >= 2^31.
 * OVG_E_ARG before the first HIP call, and then nothing is written: NULL params / vertices / faces / ws or a NULL required output
 * (topology: all four; select: out_count in COUNT, out_vertices when vertex_capacity > 0 and out_faces when face_capacity > 0 in
 * SCATTER; smooth: out_vertices and out_status), sizes outside the limits, an unknown stage, a negative capacity, iterations outside
 * [0, 65536], a lambda or mu that is not finite, fix_boundary other than 0 / 1, out_vertices == vertices (smoothing reads the input to
 * the end), a pointer that is not aligned to its element, a misaligned or undersized workspace.
 * Not in it: hole filling, edge-adjacency components, pinch-vertex detection (two fans meeting in one vertex pass as manifold),
 * cotangent or area weights, quadric simplification, any guarantee that smoothing keeps a mesh free of self-intersections.
 * ------------------------------------------------------------------ */
enum { OVG_MT_REFERENCED = 1, OVG_MT_BOUNDARY = 2, OVG_MT_NONMANIFOLD = 4 };   /* vertex_flags */
enum { OVG_MT_INTERNAL = 1 };                                                  /* out_count[7] */
enum { OVG_MSEL_COUNT = 1, OVG_MSEL_SCATTER = 2 };
enum { OVG_MSM_NONFINITE = 1 };                                                /* out_status[0] */
typedef struct {
  const float* vertices; const int32_t* faces;
  int64_t num_vertices; int64_t num_faces;
  int32_t* vertex_root; int32_t* face_root; uint8_t* vertex_flags; int64_t* out_count;
  void* ws; int64_t ws_bytes;
} ovg_mesh_topology_params;
int64_t ovg_mesh_topology_workspace_bytes(int64_t vertices, int64_t faces);
int ovg_mesh_topology(const ovg_mesh_topology_params*, void* stream);

typedef struct {
  const float* vertices; const int32_t* faces; const uint8_t* face_keep; const uint8_t* vertex_keep;
  int64_t num_vertices; int64_t num_faces;
  int32_t stage; int32_t pad;
  int64_t vertex_capacity; int64_t face_capacity;
  float* out_vertices; int64_t* out_source_index; int32_t* out_faces; int64_t* out_face_index; int64_t* out_count;
  void* ws; int64_t ws_bytes;
} ovg_mesh_select_params;
int64_t ovg_mesh_select_workspace_bytes(int64_t vertices, int64_t faces);
int ovg_mesh_select(const ovg_mesh_select_params*, void* stream);

typedef struct {
  const float* vertices; const int32_t* faces; const uint8_t* fixed;
  int64_t num_vertices; int64_t num_faces;
  int32_t iterations; int32_t fix_boundary; float lambda; float mu;
  float* out_vertices; float* out_normals; int64_t* out_status;
  void* ws; int64_t ws_bytes;
} ovg_mesh_smooth_params;
int64_t ovg_mesh_smooth_workspace_bytes(int64_t vertices, int64_t faces);
int ovg_mesh_smooth(const ovg_mesh_smooth_params*, void* stream);

/* ------------------------------------------------------------------ *
 * Input preprocessing (ABI 13): everything the reference's loaders (visual_util.py:679-845, omnivggt/utils/load_fn.py:53-146) do
 * after PIL's convert("RGB"), for all frames of a call in one launch per pass.
 *
 * ovg_resample_frames: Pillow's 8-bit BICUBIC resize (Image.resize, a = -0.5, 22 fractional bits), then a vertical crop, placement
 * in a canvas and, for OVG_RS_F32_CHW, ToTensor (lut[u8]) into f32 CHW planes with the canvas outside the content set to 1.0f.
 *   src: packed RGB u8 HWC frames (3 bytes per pixel, rows of 3 * src_w bytes); frame f starts at src + frames[f].src_off.
 *   coef: int32 tables built on the host per (in, out) axis pair. At bounds_off: out pairs (first input index, tap count);
 *   at k_off: out rows of ksize fixed-point weights (Pillow's normalize_coeffs_8bpc). Output pixel i of a pass is
 *   clamp((2^21 + sum_j in[first + j] * k[i][j]) >> 22, 0, 255) in int32 over its tap count.
 *   Horizontal pass (only when h_k_off >= 0): source rows [mid_row0, mid_row0 + mid_rows) -> u8 rows of res_w pixels in ws at
 *   mid_off; the vertical pass then reads those rows (first index - mid_row0), else the source rows directly (src_w == res_w).
 *   Vertical pass: resized rows crop_y .. crop_y + out_h - 1 (a pass that keeps the height uses identity weights: the copy Pillow
 *   makes) -> canvas rows pad_top .., columns pad_left .. pad_left + res_w - 1.
 *   out (OVG_RS_F32_CHW): f32 [3][canvas_h][canvas_w] at out + canvas_off elements; (OVG_RS_U8_HWC): u8 [canvas_h][canvas_w][3].
 *   frames / coef: device copies; frames_host / coef_host: the same bytes on the host, validated before any HIP call (every read
 *   and write of the kernels stays inside src_bytes / coef_len / ws_bytes / out_elems, or the call returns OVG_E_ARG).
 * ovg_resample_workspace_bytes: bytes of ws the frames need (max of mid_off + 3 * mid_rows * res_w), -1 on bad arguments.
 *
 * ovg_depth_frames: the depth half of visual_util.py:763-801: d = src (non-finite -> 0, then > max_depth -> 0, then < 1e-5f -> 0),
 * gathered at rows index[rows_off + y] and columns index[cols_off + x] (cv2 INTER_NEAREST + the crop, computed on the host), written
 * to depth[out_off + y * out_w + x] and mask = d > 1e-5f ? 1 : 0 at the same offset. Frames not listed are left untouched.
 * ------------------------------------------------------------------ */
enum { OVG_RS_F32_CHW = 0, OVG_RS_U8_HWC = 1 };
typedef struct {
  int64_t src_off; int32_t src_w; int32_t src_h;
  int32_t res_w; int32_t res_h; int32_t crop_y; int32_t out_h;
  int32_t mid_row0; int32_t mid_rows; int64_t mid_off;
  int32_t h_bounds_off; int32_t h_k_off; int32_t h_ksize;
  int32_t v_bounds_off; int32_t v_k_off; int32_t v_ksize;
  int32_t canvas_w; int32_t canvas_h; int32_t pad_top; int32_t pad_left;
  int64_t canvas_off;
} ovg_resample_frame;
typedef struct {
  const ovg_resample_frame* frames; const ovg_resample_frame* frames_host; int32_t nframes; int32_t out_format;
  const uint8_t* src; int64_t src_bytes;
  const int32_t* coef; const int32_t* coef_host; int64_t coef_len;
  const float* lut;
  void* out; int64_t out_elems;
  uint8_t* ws; int64_t ws_bytes;
} ovg_resample_params;
int64_t ovg_resample_workspace_bytes(const ovg_resample_frame* frames_host, int32_t nframes);
int ovg_resample_frames(const ovg_resample_params*, void* stream);

typedef struct {
  int64_t src_off; int32_t src_w; int32_t src_h;
  int32_t rows_off; int32_t cols_off; int32_t out_w; int32_t out_h;
  int64_t out_off;
} ovg_depth_frame;
typedef struct {
  const ovg_depth_frame* frames; const ovg_depth_frame* frames_host; int32_t nframes; float max_depth;
  const float* src; int64_t src_elems;
  const int32_t* index; const int32_t* index_host; int64_t index_len;
  float* depth; float* mask; int64_t out_elems;
} ovg_depth_params;
int ovg_depth_frames(const ovg_depth_params*, void* stream);

/* head-major -> token-major: x [heads, n_pad, 64] dtype -> y [n, heads*64] dtype (row stride ldy), the layout the
 * proj GEMM reads; used after the return all-to-all of the head-parallel sharded attention. */
typedef struct {
  const void* x; int64_t n_pad; void* y; int64_t ldy; int64_t n; int heads; int dtype;
} ovg_heads_to_tokens_params;
int ovg_heads_to_tokens(const ovg_heads_to_tokens_params*, void* stream);

/* ------------------------------------------------------------------
 * Camera head: replaces CameraHead.forward / trunk_fn, omnivggt/heads/camera_head.py:84-154, for
 * one batch element: S camera tokens (row m of `tokens`, 2048 f32, row stride ld_tokens elements: the slot-0 token of
 * every view in the LAST aggregator layer, camera_head.py:96-100) -> out [iters][S][9] f32, the activated pose
 * encodings of every refinement round (absT_quaR_FoV: translation and quaternion linear, field of view ReLU,
 * heads/head_act.py:12-35). One call issues every launch of every round; nothing is read back in between.
 *   GEMM weights (mod_w [6144,2048], blk[i].qkv_w [6144,2048], proj_w [2048,2048], fc1_w [8192,2048],
 *   fc2_w [2048,8192], pb1_w [1024,2048]) in `dtype` (OVG_BF16 / OVG_F16 / OVG_F32; nn.Linear layout, K contiguous,
 *   16-byte aligned); every vector, the 9-wide embed_pose [2048,9] and pose_branch.fc2 [9,1024] matrices and all
 *   activations that carry state (residual stream, statistics, softmax, pose) f32. With OVG_F32 (the parity mode) the
 *   GEMM operands and the activation buffers between kernels are f32 too and the products run on the exact-f32 MFMA:
 *   no rounding point below f32 anywhere. dim must be 2048, heads 16 (head dim 128), trunk_depth <= OVG_CAMERA_MAX_TRUNK,
 *   S <= 4096. ws: caller-owned scratch of >= ovg_camera_head_workspace_bytes(S, dtype) bytes (returns -1 on bad args).
 * Workspace layout (carve() in csrc/ovg_camhead.hip; tests/kernel_guards.py camera_ws_views restates it): nine buffers in this
 * order, each starting on a multiple of 256 bytes from ws (sizes rounded up to 256), E = bytes per element of `dtype`:
 *   tok  [S][2048]  f32    token_norm(tokens), written once
 *   x    [S][2048]  f32    the residual stream, updated in place by every modulation and block
 *   pose [S][9]     f32    the carried pose encoding, NOT activated (out holds the activated copy of every round)
 *   part [S][32768] f32    split-K partials of the GEMM in flight, [ksplit][S][N] with ksplit * N <= 32768
 *   xn   [S][2048]  dtype  the LayerNorm feeding the next GEMM (n1, n2, ... trunk_norm: overwritten by each)
 *   e    [S][2048]  dtype  SiLU(embed_pose(pose)) of the round
 *   qkv  [S][6144]  dtype  q | k | v of the block, 16 heads x 128 each
 *   attn [S][2048]  dtype  attention output, token-major
 *   hid  [S][8192]  dtype  GELU(fc1) of the block
 * After the call the buffers hold the values of the last round's last block; nothing outside these ranges is written.
 * Size limits: 0 < S <= 4096 (OVG_E_UNSUPPORTED beyond), iters > 0; ld_tokens >= 2048 and a multiple of 4 elements, otherwise any: the
 * tokens are read once, by the token LayerNorm, through a 64-bit row offset. Every workspace offset is 64-bit (and below 2^31 at S = 4096).
 * ------------------------------------------------------------------ */
#define OVG_CAMERA_MAX_TRUNK 4
typedef struct {
  const float *n1_w, *n1_b, *n2_w, *n2_b, *ls1, *ls2;
  const void* qkv_w; const float* qkv_b;
  const void* proj_w; const float* proj_b;
  const void* fc1_w; const float* fc1_b;
  const void* fc2_w; const float* fc2_b;
} ovg_camera_block_weights;
typedef struct {
  const float* tokens; int64_t ld_tokens;
  int32_t S; int32_t iters; int32_t dtype; int32_t trunk_depth; int32_t dim; int32_t heads;
  const float *token_norm_w, *token_norm_b, *trunk_norm_w, *trunk_norm_b;
  const float* empty_pose;
  const float *embed_w, *embed_b;
  const void* mod_w; const float* mod_b;
  ovg_camera_block_weights blk[OVG_CAMERA_MAX_TRUNK];
  const void* pb1_w; const float* pb1_b;
  const float *pb2_w, *pb2_b;
  void* ws; int64_t ws_bytes;
  float* out;
} ovg_camera_head_params;
int64_t ovg_camera_head_workspace_bytes(int32_t S, int32_t dtype);
int ovg_camera_head(const ovg_camera_head_params*, void* stream);

/* ------------------------------------------------------------------
 * Camera-modality injection tables, built on the device without a host round trip (replaces, per forward:
 * ZeroAggregator.normalize_extrinsics omnivggt_aggregator.py:85-105 with closed_form_inverse_se3 utils/geometry.py:269-318,
 * extri_intri_to_pose_encoding utils/pose_enc.py:11-62 with mat_to_quat utils/rotation.py:47-109, the 25 pose_embeddings /
 * camera_adapters Linear pairs omnivggt_aggregator.py:62-75,172,211,277,286 and the zero-padded scatter :174-178,278-282):
 *   enc[b, r]       = pose encoding (t, quat xyzw, fov_h, fov_w) of camera index[r] of batch b after normalisation
 *                     (first selected camera -> identity, translations / mean distance of the others to it)
 *   emb[g, b*Sc+r]  = pose_w[g] enc[b, r] + pose_b[g]                                   g < G (= depth + 1 tables)
 *   tables[g, b*S+s] = adapt_w[g] emb[g, b*Sc+r] + adapt_b[g]   if s == index[r]        (exact-f32 MFMA)
 *                      adapt_b[g]                               otherwise (Linear of a zero row)
 * extrinsics [B,S,3,4] (world-to-camera), intrinsics [B,S,3,3] f32; index: DEVICE int32 [Sc], strictly the caller's
 * camera_gt_index (values in [0, S): the array is on the device, so the entry cannot reject it -- reads through an
 * out-of-range entry are clamped into [0, S) and its scatter is skipped, never an out-of-bounds access; a view may appear more than once,
 * as in the reference: the statistics run over the list as given and the duplicate entries scatter identical rows); pose_w [G*1024, 9] f32 row-major, pose_b [G*1024]; adapt_w [G,1024,1024] f32
 * (nn.Linear layout, 16-byte aligned), adapt_b [G,1024]; enc [B*Sc, 9] and emb [G, B*Sc, 1024] are caller-owned scratch
 * (NULL allowed when Sc == 0); tables [G, B*S, 1024] f32. Three launches (one when Sc == 0); nothing is read back.
 * ------------------------------------------------------------------ */
typedef struct {
  const float* extrinsics; const float* intrinsics; const int32_t* index;
  int32_t B; int32_t S; int32_t Sc; int32_t H; int32_t W; int32_t G;
  const float* pose_w; const float* pose_b;
  const float* adapt_w; const float* adapt_b;
  float* enc; float* emb; float* tables;
} ovg_camera_tables_params;
int ovg_camera_tables(const ovg_camera_tables_params*, void* stream);

/* MFMA lane-map probe (diagnostics; tools/selftest.py): fills out[64*4] with
 * acc of one 16x16 MFMA for dtype given raw 16-byte A/B fragments per lane. */
int ovg_probe_mfma(const void* a_frag, const void* b_frag, float* out, int dtype, void* stream);


#ifdef __cplusplus
}
#endif
#endif
