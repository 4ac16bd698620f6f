"""-m gpu: every HIP kernel, called through the C ABI, against a PyTorch CPU fp32 evaluation
of the same op on the same dtype-rounded inputs (tolerances in gpu_selftest.TOL: bf16 2e-2,
f16 4e-3, f32 2e-5 max-rel; f32 GEMM/attention additionally <= 5e-5 through a whole block)."""
import pytest
import torch

import gpu_selftest as st
from omnivggt_official_amd import lib as L

pytestmark = pytest.mark.gpu


@pytest.fixture(autouse=True)
def _need_gpu():
    L.require_gpu()
    st.results.clear()


def _assert_clean():
    bad = [r for r in st.results if not r["ok"]]
    assert st.results and not bad, bad


def test_mfma_lane_maps():
    st.test_probe()
    _assert_clean()


def test_layernorm():
    st.test_layernorm()
    _assert_clean()


def test_linear_epilogues():
    st.test_linear(False)
    _assert_clean()


def test_qkv_qknorm_rope():
    st.test_qkv(False)
    _assert_clean()


def test_flash_attention_incl_ragged_segments_and_rescale():
    st.test_attn(False)
    _assert_clean()


def test_embed_kernels():
    st.test_embed()
    _assert_clean()


def test_block_forward():
    st.test_block(False)
    _assert_clean()


def test_dpt_head_kernels_and_whole_head():
    st.test_heads(False)
    _assert_clean()


def test_camera_head_entry_vs_twin_and_f32_module():
    """SURVEY 8(f) N1 remainder: the whole iterative camera head on ovg_camera_head (split-K weight-stream GEMMs)."""
    st.test_camera_head()
    _assert_clean()


def test_gemm256_kernels_every_epilogue_ragged_m():
    """The 256 x 256 GEMMs the 64-view bench runs (qkv256_kernel, linear256_kernel<GELU|RES|STORE|PATCH>; free-running main loop since round 6)."""
    st.test_gemm256(False)
    _assert_clean()


def test_history_variants_are_not_in_the_product_library():
    """Round-4 review, hygiene: the A/B history (r02 epilogue forms, attention variants of rounds 1-4) is not in the library, which refuses
    its selectors by name -- from ovg_linear and ovg_qkv, ovg_flash_attn and ovg_attn_plan alike, and without launching anything. The
    round-5 lab GEMM selectors (4 = persistent 256 x 256, 10 = DMA-in-M) left the ABI in round 6: they are plain argument errors."""
    import torch
    from omnivggt_official_amd import ops
    x = torch.zeros(512, 1024, device="cuda", dtype=torch.bfloat16)
    w = torch.zeros(1024, 1024, device="cuda", dtype=torch.bfloat16)
    for tile in (L.TILE_256X, L.TILE_128X):
        with pytest.raises(L.OvgError, match="UNSUPPORTED"):
            ops.linear(x, w, None, torch.bfloat16, tile=tile)
    for tile in (4, 10, 42):
        with pytest.raises(L.OvgError, match="ARG"):
            ops.linear(x, w, None, torch.bfloat16, tile=tile)
    # ovg_qkv: M = 512 rows as two sequences of 256; a refused call writes nothing
    wqkv = torch.zeros(3 * 1024, 1024, device="cuda", dtype=torch.bfloat16)
    bqkv = torch.zeros(3 * 1024, device="cuda", dtype=torch.float32)
    q, k, vt = ops.alloc_qkv(32, 256, 256, torch.bfloat16, "cuda")
    for t in (q, k, vt):
        t.fill_(-7.0)
    for tile in (L.TILE_128X, L.TILE_256X):
        with pytest.raises(L.OvgError, match="UNSUPPORTED"):
            ops.qkv(x, wqkv, bqkv, 256, torch.bfloat16, q, k, vt, tile=tile)
    for tile in (4, 10, 42):
        with pytest.raises(L.OvgError, match="ARG"):
            ops.qkv(x, wqkv, bqkv, 256, torch.bfloat16, q, k, vt, tile=tile)
    torch.cuda.synchronize()
    for t in (q, k, vt):
        assert bool((t == -7.0).all())
    retired = (2, 6, 8, 18, 19, 21, 25, 31, 32, 33, 51, 56, 58, 59)
    for dt in (torch.bfloat16, torch.float16):
        q, k, vt = ops.alloc_qkv(16, 256, 256, dt, "cuda")
        for variant in retired:
            with pytest.raises(L.OvgError, match="UNSUPPORTED"):
                ops.flash_attn(q, [(k, vt, 256)], 256, dt, variant=variant)
            with pytest.raises(L.OvgError, match="UNSUPPORTED"):
                ops.attn_plan(16, 256, [256], dt, variant=variant)


def test_global_attention_at_bench_key_counts():
    """N = 10 992 / 21 984 in full, N = 87 936 on sampled rows: the launches the bench times."""
    st.test_attn_big(False)
    _assert_clean()


def test_attention_lse_output_and_merge_and_weight_pack():
    st.test_attn_lse_merge()
    _assert_clean()


def test_speculative_softmax_fallback_counter_with_attention_sinks():
    """fallback_count telemetry: exact results with attention-sink logits, 0 re-runs inside the anchored pass's exponent window,
    every workgroup reported beyond it."""
    st.test_attn_fallback_counter()
    _assert_clean()


def test_split_f16_mode_kernels_vs_float64():
    """OVG_F16X2 ("f32x", the <= 1e-4 mode with throughput): pack / LayerNorm / im2col splits, every GEMM epilogue on both tile sizes,
    the fused QKV epilogue and the three-MFMA flash attention (segments, ragged tails, forced rescale, log-sum-exp), each within 1e-5
    max-rel of a float64 evaluation of the same f32 inputs."""
    st.test_f32x(False)
    _assert_clean()


def test_loaded_library_is_the_in_tree_one():
    import os
    assert os.path.samefile(L.LIB_PATH, os.path.join(os.path.dirname(L.__file__), "libomnivggt_hip.so"))
    maps = open("/proc/self/maps").read()
    assert "libomnivggt_hip.so" in maps
