"""Kernel-by-kernel GPU self test + micro-benchmark (run on the MI355X box):

    python tests/gpu_selftest.py [--quick] [--bench]

Each HIP kernel is called through the C ABI and compared with a plain PyTorch CPU fp32
evaluation of the same op on the same (dtype-rounded) inputs.  Prints one line per check
with the max abs / max rel error so a failure can be diagnosed from the log alone.
This is a diagnostic tool; the pytest suite (tests/test_gpu_*.py) holds the gated checks.
"""
import argparse
import json
import math
import os
import sys
import time

import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "oracle"))

from omnivggt_official_amd import lib as L, ops  # noqa: E402
import aggregator_oracle as orc  # noqa: E402

DEV = "cuda"
DT = {"bf16": torch.bfloat16, "f16": torch.float16, "f32": torch.float32}
TOL = {"bf16": 2e-2, "f16": 4e-3, "f32": 2e-5}
results = []


def report(name, got, ref, tol):
    got = got.detach().float().cpu()
    ref = ref.detach().float().cpu()
    bad = ~torch.isfinite(got)
    diff = (got - ref).abs()
    diff[bad] = float("inf")
    mx = float(diff.max())
    scale = float(ref.abs().max())
    rel = mx / max(scale, 1e-30)
    ok = rel <= tol
    where = ""
    if not ok:
        idx = int(diff.flatten().argmax())
        unr = []
        for s in reversed(got.shape):
            unr.append(idx % s)
            idx //= s
        nbad = int((diff > tol * scale).sum())
        where = " worst@%s got=%g ref=%g nbad=%d/%d nonfinite=%d" % (list(reversed(unr)), float(got.flatten()[int(diff.flatten().argmax())]),
                                                                   float(ref.flatten()[int(diff.flatten().argmax())]), nbad, diff.numel(), int(bad.sum()))
    print("[%s] %-46s max_abs=%.3e ref_max=%.3e rel=%.3e tol=%.1e%s" % ("PASS" if ok else "FAIL", name, mx, scale, rel, tol, where), flush=True)
    results.append({"name": name, "ok": bool(ok), "rel": rel})
    return ok


def rnd(*shape, g, scale=1.0):
    return torch.randn(*shape, generator=g) * scale


# ---------------------------------------------------------------------------
def test_probe():
    """MFMA lane maps assumed by the kernels: A row = lane&15, B col = lane&15,
    C[row = 4*(lane>>4)+r][col = lane&15]; A and B share the k assignment."""
    g = torch.Generator().manual_seed(1)
    for name, code, per, tdt in (("bf16", L.OVG_BF16, 8, torch.bfloat16), ("f16", L.OVG_F16, 8, torch.float16), ("f32", L.OVG_F32, 4, torch.float32)):
        Kd = per * 4
        A = torch.randint(-4, 5, (16, Kd), generator=g).float()
        B = torch.randint(-4, 5, (16, Kd), generator=g).float()   # B^T rows: B[n][k]
        # lane l: row l&15, chunk l>>4 (k = per*(l>>4) .. +per)
        af = torch.stack([A[l & 15, per * (l >> 4): per * (l >> 4) + per] for l in range(64)]).to(tdt).contiguous()
        bf = torch.stack([B[l & 15, per * (l >> 4): per * (l >> 4) + per] for l in range(64)]).to(tdt).contiguous()
        out = ops.probe_mfma(af.to(DEV).view(torch.int32).view(64, 4), bf.to(DEV).view(torch.int32).view(64, 4), code).cpu()
        Cm = A @ B.t()      # C[i][j] = sum_k A[i][k] B[j][k]
        exp = torch.stack([torch.stack([Cm[4 * (l >> 4) + r, l & 15] for r in range(4)]) for l in range(64)])
        ok = report("probe_mfma_%s (C[4g+r][lane&15])" % name, out, exp, 0.0)
        if not ok:
            expT = torch.stack([torch.stack([Cm[l & 15, 4 * (l >> 4) + r] for r in range(4)]) for l in range(64)])
            print("   transposed hypothesis matches:", bool(torch.equal(out, expT)))
            print("   out[:8]=", out[:8].tolist())
            print("   exp[:8]=", exp[:8].tolist())


def test_layernorm():
    g = torch.Generator().manual_seed(2)
    rows = 1374 * 2 + 3
    big = rnd(rows, 2048, g=g, scale=2.0) + 0.3
    x = big[:, 1024:]                                  # strided view (ld = 2048)
    w, b = rnd(1024, g=g) * 0.1 + 1, rnd(1024, g=g) * 0.1
    ref = F.layer_norm(x, (1024,), w, b, 1e-5)
    xd = big.to(DEV)[:, 1024:]
    for name, dt in DT.items():
        y = ops.layernorm(xd, w.to(DEV), b.to(DEV), 1e-5, dt)
        report("layernorm_%s" % name, y, ref, TOL[name] if name != "f32" else 2e-6)
    y = ops.layernorm(xd, w.to(DEV), b.to(DEV), 1e-6, torch.bfloat16, out_f32=True)
    report("layernorm_out_f32_eps1e-6", y, F.layer_norm(x, (1024,), w, b, 1e-6), 2e-6)


def test_linear(quick):
    g = torch.Generator().manual_seed(3)
    for name, dt in DT.items():
        for (M, N, K) in ((300, 256, 128), (1374 * 2, 1024, 1024)) if not quick else ((300, 256, 128),):
            x = rnd(M, K, g=g).to(dt)
            w = (rnd(N, K, g=g) * 0.05).to(dt)
            bias = rnd(N, g=g)
            xf, wf = x.float(), w.float()
            base = xf @ wf.t() + bias
            xd, wd, bd = x.to(DEV), w.to(DEV), bias.to(DEV)
            tol = TOL[name]
            y = ops.linear(xd, wd, bd, dt)
            report("linear_store_%s_%dx%dx%d" % (name, M, N, K), y, base, tol)
            y = ops.linear(xd, wd, bd, dt, out_f32=True)
            report("linear_store_f32out_%s_%dx%dx%d" % (name, M, N, K), y, base, 2e-5 if name != "f32" else 2e-6)
            y = ops.linear(xd, wd, bd, dt, epilogue=L.EPI_GELU)
            report("linear_gelu_%s_%dx%dx%d" % (name, M, N, K), y, F.gelu(base), tol)
            res = rnd(M, 2 * N, g=g)
            gamma = rnd(N, g=g)
            per = 137
            inj = rnd((M + per - 1) // per, N, g=g)
            ref = res[:, N:] + gamma * base
            ref2 = ref.clone()
            ref2[::per] += inj[: ref2[::per].shape[0]]
            resd = res.to(DEV)
            out = torch.zeros(M, 2 * N, device=DEV)
            ops.linear(xd, wd, bd, dt, epilogue=L.EPI_RES, out=out[:, :N], res=resd[:, N:], gamma=gamma.to(DEV))
            report("linear_res_%s_%dx%dx%d" % (name, M, N, K), out[:, :N], ref, 2e-5 if name != "f32" else 2e-6)
            if N == 1024:
                ops.linear(xd, wd, bd, dt, epilogue=L.EPI_RES, out=out[:, :N], res=resd[:, N:], gamma=gamma.to(DEV), inject=inj.to(DEV), inj_period=per)
                report("linear_res_inject_%s_%dx%dx%d" % (name, M, N, K), out[:, :N], ref2, 2e-5 if name != "f32" else 2e-6)
            tail_clean = float(out[:, N:].abs().max()) == 0.0         # the launches above own out[:, :N] of a 2N-wide buffer only
            results.append({"name": "linear_res_%s_%dx%dx%d.row_gap_untouched" % (name, M, N, K), "ok": bool(tail_clean), "rel": 0.0})
            if not tail_clean:
                print("[FAIL] linear RES wrote past column N of its output rows")
        # PATCH epilogue: M = 2 views * 100 patches -> rows (v*105 + 5 + t)
        p0, p1 = 100, 105
        M, N, K = 2 * p0, 1024, 640
        x = rnd(M, K, g=g).to(dt)
        w = (rnd(N, K, g=g) * 0.05).to(dt)
        bias = rnd(N, g=g)
        table = rnd(p0 + 1, N, g=g)
        base = x.float() @ w.float().t() + bias
        ref = torch.zeros(2 * p1, N)
        for v in range(2):
            ref[v * p1 + 5: v * p1 + 5 + p0] = base[v * p0:(v + 1) * p0] + table[1:]
        out = torch.zeros(2 * p1, 2 * N, device=DEV)
        ops.linear(x.to(DEV), w.to(DEV), bias.to(DEV), dt, epilogue=L.EPI_PATCH, out=out[:, :N], table=table.to(DEV), p0=p0, p1=p1, row_off=5)
        report("linear_patch_%s" % name, out[:, :N], ref, 2e-5 if name != "f32" else 2e-6)
        tail_clean = float(out[:, N:].abs().max()) == 0.0
        results.append({"name": "linear_patch_%s.row_gap_untouched" % name, "ok": bool(tail_clean), "rel": 0.0})
        if not tail_clean:
            print("[FAIL] linear PATCH wrote past column N of its output rows")


def qkv_reference(x, w, bias, seq, qk_norm, rope, tokens_per_view, grid_w):
    """attention.py:52-58 on CPU: returns q (scaled), k, v as [B,H,N,64]."""
    M = x.shape[0]
    B = M // seq
    qkv = (x @ w.t() + bias).reshape(B, seq, 3, 16, 64).permute(2, 0, 3, 1, 4)
    q, k, v = qkv[0], qkv[1], qkv[2]
    if qk_norm is not None:
        q = F.layer_norm(q, (64,), qk_norm[0], qk_norm[1], 1e-5)
        k = F.layer_norm(k, (64,), qk_norm[2], qk_norm[3], 1e-5)
    if rope is not None:
        t = torch.arange(M) % tokens_per_view
        pp = (t - 5).clamp(min=0)
        py = torch.where(t >= 5, pp // grid_w + 1, torch.zeros_like(t))
        px = torch.where(t >= 5, pp % grid_w + 1, torch.zeros_like(t))
        pos = torch.stack([py, px], -1).reshape(B, seq, 2)
        q = orc.rope_2d(q, pos, *rope)
        k = orc.rope_2d(k, pos, *rope)
    return q * (0.125 * 1.4426950408889634), k, v


def test_qkv(quick):
    g = torch.Generator().manual_seed(4)
    tpv, gw = 1374, 37
    cos, sin = orc.rope_tables(38)
    cos16, sin16 = cos[:, :16].contiguous(), sin[:, :16].contiguous()
    for name, dt in DT.items():
        for mode, nviews in (("frame", 2), ("global", 2)):
            M = nviews * tpv
            seq = tpv if mode == "frame" else M
            x = rnd(M, 1024, g=g).to(dt)
            w = (rnd(3072, 1024, g=g) * 0.03).to(dt)
            bias = rnd(3072, g=g) * 0.1
            qn = [rnd(64, g=g) * 0.1 + 1.5, rnd(64, g=g) * 0.1, rnd(64, g=g) * 0.1 + 1.5, rnd(64, g=g) * 0.1]
            for variant in (("norm_rope", qn, (cos, sin)), ("plain", None, None)):
                vn, qk_norm, rope = variant
                qr, kr, vr = qkv_reference(x.float(), w.float(), bias, seq, qk_norm, rope, tpv, gw)
                BH = (M // seq) * 16
                q, k, vt = ops.alloc_qkv(BH, seq, seq, dt, DEV)
                ops.qkv(x.to(DEV), w.to(DEV), bias.to(DEV), seq, dt, q, k, vt,
                        qk_norm=None if qk_norm is None else [t.to(DEV) for t in qk_norm],
                        rope=None if rope is None else (cos16.to(DEV), sin16.to(DEV)))
                tol = TOL[name] * (2 if name != "f32" else 5)
                report("qkv_%s_%s_%s.q" % (name, mode, vn), q[:, :seq], qr.reshape(BH, seq, 64), tol)
                report("qkv_%s_%s_%s.k" % (name, mode, vn), k[:, :seq], kr.reshape(BH, seq, 64), tol)
                report("qkv_%s_%s_%s.vt" % (name, mode, vn), ops.get_vt(vt)[:, :, :seq], vr.reshape(BH, seq, 64).transpose(1, 2), tol)
                pad_clean = (q.shape[1] == seq or float(q[:, seq:].abs().max()) == 0.0) and \
                    (k.shape[1] == seq or (float(k[:, seq:].abs().max()) == 0.0 and float(ops.get_vt(vt)[:, :, seq:].abs().max()) == 0.0))
                results.append({"name": "qkv_%s_%s_%s.padding_untouched" % (name, mode, vn), "ok": bool(pad_clean), "rel": 0.0})
                if not pad_clean:
                    print("[FAIL] qkv padding was written")
            if quick:
                break


def attn_reference(q, k, v):
    """q pre-scaled by scale*log2e: softmax base 2."""
    s = (q @ k.transpose(-1, -2)) * math.log(2.0)
    return torch.softmax(s, dim=-1) @ v


# the kernels of the library (the A/B history -- variants 2, 6, 8, 18, 19, 21, 25, 31-33, 51, 56, 58, 59 -- left the tree and answers
# OVG_E_UNSUPPORTED): default plan, baseline, LDS-DMA staged speculative 256-row / lazy 256-row / forced
# fallback / speculative + lazy 128-row / speculative 512-row with a barrier every 2 tiles, and the plan's A/B knobs (71-73: tail splits)
ATTN16_VARIANTS = (0, 1, 50, 52, 53, 54, 55, 57)


def test_attn(quick):
    g = torch.Generator().manual_seed(5)
    for name, dt in DT.items():
        shapes = [("n1374_bh32", 32, 1374, [1374]), ("n2748_2seg", 16, 2748 // 2, [1374, 1374]),
                  ("n700_ragged_seg", 16, 700, [100, 333, 64]), ("n300_seg", 16, 300, [130, 70]),
                  ("n500_short_segs", 16, 500, [40, 64, 7, 192, 129])]      # segments shorter than one key tile, exact tiles, a 1-key tail
        variants = (1,) if name == "f32" else ATTN16_VARIANTS
        if quick:
            shapes = shapes[:2]
        for cname, BH, nq, nks in shapes:
            q = (rnd(BH, nq, 64, g=g) * 1.2).to(dt)
            ks = [(rnd(BH, nk, 64, g=g)).to(dt) for nk in nks]
            vs = [(rnd(BH, nk, 64, g=g)).to(dt) for nk in nks]
            ref = attn_reference(q.float(), torch.cat(ks, 1).float(), torch.cat(vs, 1).float())   # [BH,nq,64]
            ref_tok = ref.reshape(BH // 16, 16, nq, 64).permute(0, 2, 1, 3).reshape(-1, 1024)
            qd, _, _ = ops.alloc_qkv(BH, nq, 64, dt, DEV)
            qd[:, :nq] = q.to(DEV)
            segs = []
            for kk, vv in zip(ks, vs):
                nk = kk.shape[1]
                _, kd, vtd = ops.alloc_qkv(BH, 64, nk, dt, DEV)
                kd[:, :nk] = kk.to(DEV)
                ops.set_vt(vtd, vv.transpose(1, 2))
                segs.append((kd, vtd, nk))
            for variant in variants:
                out = ops.flash_attn(qd, segs, nq, dt, variant=variant)
                report("attn_%s_%s_v%d" % (name, cname, variant), out, ref_tok, TOL[name])
        # head-parallel sharding form: 16 batch entries = (source rank, head) pairs sharing this rank's kv_heads heads,
        # `world` K / V^T segments, head-major output; then the head-major -> token-major copy
        if name != "f32":
            world, hpr, nq, nk = 2, 8, 333, 200
            q = (rnd(world * hpr, nq, 64, g=g) * 1.2).to(dt)
            ks = [rnd(hpr, nk, 64, g=g).to(dt) for _ in range(world)]
            vs = [rnd(hpr, nk, 64, g=g).to(dt) for _ in range(world)]
            kf, vf = torch.cat(ks, 1).float(), torch.cat(vs, 1).float()                      # [hpr, world*nk, 64]
            ref = torch.stack([attn_reference(q[bh].float(), kf[bh % hpr], vf[bh % hpr]) for bh in range(world * hpr)])
            qd, _, _ = ops.alloc_qkv(world * hpr, nq, 64, dt, DEV)
            qd[:, :nq] = q.to(DEV)
            segs = []
            for kk, vv in zip(ks, vs):
                _, kd, vtd = ops.alloc_qkv(hpr, 64, nk, dt, DEV)
                kd[:, :nk] = kk.to(DEV)
                ops.set_vt(vtd, vv.transpose(1, 2))
                segs.append((kd, vtd, nk))
            for variant in ATTN16_VARIANTS:
                out = ops.flash_attn(qd, segs, nq, dt, variant=variant, kv_heads=hpr, head_major=True)
                report("attn_%s_headpar_v%d" % (name, variant), out[:, :nq], ref, TOL[name])
            tok = ops.heads_to_tokens(out, nq, dt)
            report("heads_to_tokens_%s" % name, tok, out[:, :nq].permute(1, 0, 2).reshape(nq, -1).float().cpu(), 1e-7)
        # forced-rescale cases: one key spikes against one query late in the sequence (the lazy
        # rescale branch of the tuned kernel fires mid-stream), and a slowly rising score ramp
        # (speculative kernel: spike 6 / ramp leave the f32 exponent window -> verified fallback path;
        #  spike 1 = 64 log2 units above the rest stays inside it)
        for cname, spike in (("spike", 6.0), ("spike_small", 1.0), ("ramp", 0.0)):
            BH, nq, nk = 16, 128, 640
            q = rnd(BH, nq, 64, g=g).to(dt)
            k = rnd(BH, nk, 64, g=g).to(dt)
            v = rnd(BH, nk, 64, g=g).to(dt)
            if spike:
                k[:, 500] = (q[:, 7].float() * spike).to(dt)
            else:
                k = (k.float() + q[:, 3:4].float() * torch.linspace(0, 3, nk).view(1, nk, 1)).to(dt)
            ref = attn_reference(q.float(), k.float(), v.float()).reshape(1, 16, nq, 64).permute(0, 2, 1, 3).reshape(-1, 1024)
            qd, kd, vtd = ops.alloc_qkv(BH, nq, nk, dt, DEV)
            qd[:, :nq] = q.to(DEV)
            kd[:, :nk] = k.to(DEV)
            ops.set_vt(vtd, v.transpose(1, 2))
            for variant in ((1,) if name == "f32" else ATTN16_VARIANTS):
                out = ops.flash_attn(qd, [(kd, vtd, nk)], nq, dt, variant=variant)
                report("attn_%s_%s_rescale_v%d" % (name, cname, variant), out, ref, TOL[name])



def test_attn_fallback_counter():
    """Speculative-softmax telemetry (ovg_attn_params.fallback_count, round-3 review): global attention at the 8-view key count with
    ATTENTION-SINK logits -- every query carries a common component, a few keys answer it with +40 ... +130 log2 units -- inside and
    outside the first key tile (the tile the speculative pass anchors on). The result must be the exact softmax in every case (float64
    reference on sampled rows); the counter must stay 0 while the sinks fit the f32 exponent window of the anchored pass (|log2| <= 100
    around the first-tile maximum) and must report every workgroup once the window is left."""
    g = torch.Generator().manual_seed(77)
    dt, BH, n = torch.bfloat16, 16, 8 * 1374
    rows = torch.tensor([0, 1, 17, 255, 256, 4000, 8191, n - 300, n - 1])
    # logits without sinks: ~N(0, 9.5) log2 units, first-tile maxima 10 ... 30; a sink adds 4 * gain to every query's logit
    cases = (("none", [], 0.0, 0), ("first_tile_+88", [5], 22.0, 0), ("late_+40", [3000, 9000], 10.0, 0), ("late_+56", [7777], 14.0, 0),
             ("late_+130", [7777], 32.5, None))                        # None: every workgroup must have re-run
    q32 = torch.randn(BH, n, 64, generator=g) * 1.2
    q32[:, :, 0] = 4.0                                                 # the common component every sink key answers
    k32 = torch.randn(BH, n, 64, generator=g)
    k32[:, :, 0] = 0.0
    v32 = torch.randn(BH, n, 64, generator=g)
    cnt = torch.zeros(1, dtype=torch.int32, device=DEV)
    for name, sinks, gain, want in cases:
        kk = k32.clone()
        for idx in sinks:
            kk[:, idx, 0] = gain                                       # logit boost 4 * gain log2 units for every query
        q, k, v = q32.to(dt), kk.to(dt), v32.to(dt)
        qd, kd, vtd = ops.alloc_qkv(BH, n, n, dt, DEV)
        qd[:, :n], kd[:, :n] = q.to(DEV), k.to(DEV)
        ops.set_vt(vtd, v.transpose(1, 2))
        cnt.zero_()
        out = ops.flash_attn(qd, [(kd, vtd, n)], n, dt, fallback_count=cnt)
        torch.cuda.synchronize()
        ref = attn_reference(q[:, rows].double(), k.double(), v.double()).permute(1, 0, 2).reshape(len(rows), 1024)
        report("attn_fallback_%s" % name, out[rows.to(DEV)], ref, TOL["bf16"])
        got = int(cnt.item())
        plan = ops.attn_plan(BH, n, [n], dt)
        wgs = BH * ((n + plan["q_tile"] - 1) // plan["q_tile"])
        ok = (got == want) if want is not None else (got == wgs)
        print("[%s] attn_fallback_%s: %d of %d workgroups re-ran (expected %s)" % ("PASS" if ok else "FAIL", name, got, wgs, "all" if want is None else want), flush=True)
        results.append({"name": "attn_fallback_%s.count" % name, "ok": bool(ok), "rel": float(got)})


def test_f32x(quick):
    """The split-f16 mode (OVG_F16X2, L.F32X): every 16-bit tensor is a (hi, lo) pair of f16 planes and every contraction three f16
    MFMAs. Inputs are PLAIN f32 values (split by the library's own rounding rule, ops.to_hilo / ovg_pack_weights); the references are
    float64 evaluations of the same f32 values, so the tolerances bound the whole mode -- operand split (2^-22), dropped lo*lo term,
    f32 accumulation -- not a twin with matching rounding points. Gates: 1e-5 max-rel (the bf16 / f16 / f32 gates are 2e-2 / 4e-3 / 2e-5)."""
    dt, TOLX = L.F32X, 1e-5
    g = torch.Generator().manual_seed(41)
    d64 = lambda t: t.double()
    dev = lambda t: t.to(DEV)
    # --- split rule: library pack == ops.to_hilo, reconstruction error
    w32 = rnd(384, 1024, g=g) * 0.03
    pk = ops.pack_weights(dev(w32), dt)
    th = ops.to_hilo(w32)
    report("f32x_pack_weights.hi_bits", pk.hi.float(), th.hi.float(), 0.0)
    report("f32x_pack_weights.lo_bits", pk.lo.float(), th.lo.float(), 0.0)
    report("f32x_pack_weights.value", d64(pk.hi.cpu()) + d64(pk.lo.cpu()), d64(w32), 4e-7)
    pkp = ops.pack_weights(dev(rnd(16, 588, g=g)), dt, k_pad=640)
    report("f32x_pack_weights.pad_zero", pkp.hi[:, 588:].float().abs() + pkp.lo[:, 588:].float().abs(), torch.zeros(16, 52), 0.0)
    # --- LayerNorm -> HiLo
    big = rnd(1374 + 3, 2048, g=g, scale=2.0) + 0.3
    w, b = rnd(1024, g=g) * 0.1 + 1, rnd(1024, g=g) * 0.1
    y = ops.layernorm(dev(big)[:, 1024:], dev(w), dev(b), 1e-5, dt)
    report("f32x_layernorm", d64(y.hi.cpu()) + d64(y.lo.cpu()), F.layer_norm(d64(big[:, 1024:]), (1024,), d64(w), d64(b), 1e-5), 2e-6)
    # --- subnormal lo planes must CONTRIBUTE: for |x| < 2^-3 the lo plane of the split is a subnormal f16 (typical ViT weights
    # |w| ~ 0.03, most LayerNorm outputs), so the mode's accuracy rests on the f16 MFMA and the conversions not flushing denormals. x = 2^-5 +
    # 2^-20 everywhere: hi = 2^-5 exactly, lo = 2^-20 = 16 f16-subnormal units; with w = 1 the exact sum over K = 1024 is 32 + 2^-10. A flushed lo
    # would give 32 (9.8e-4 short); likewise with the roles of x and w swapped, and through the 256 x 256 kernel.
    xs = torch.full((512, 1024), 2.0 ** -5 + 2.0 ** -20)
    hs = ops.to_hilo(dev(xs))
    lo_sub = bool((hs.lo.float().abs() > 0).all() and (hs.lo.float().abs() < 2.0 ** -14).all())
    results.append({"name": "f32x_subnormal_lo.plane_is_subnormal", "ok": lo_sub, "rel": 0.0})
    ones = ops.pack_weights(dev(torch.ones(256, 1024)), dt)
    for tile in (L.TILE_128, L.TILE_256):
        y = ops.linear(hs, ones, None, dt, out_f32=True, tile=tile)
        report("f32x_subnormal_lo.x_tile%d" % tile, y, torch.full((512, 256), 32.0 + 2.0 ** -10), 2e-6)      # 32 alone would be 3.1e-5 off
        y = ops.linear(ops.to_hilo(dev(torch.ones(512, 1024))), ops.pack_weights(dev(xs[:256]), dt), None, dt, out_f32=True, tile=tile)
        report("f32x_subnormal_lo.w_tile%d" % tile, y, torch.full((512, 256), 32.0 + 2.0 ** -10), 2e-6)
    # --- linear, every epilogue, both tile sizes
    cases = [(300, 256, 128, L.TILE_AUTO), (1374 * 2, 1024, 1024, L.TILE_AUTO), (1374 * 2 + 77, 1024, 1024, L.TILE_256)]
    if not quick:
        cases += [(1374 * 2 + 77, 4096, 1024, L.TILE_256), (700, 1024, 4096, L.TILE_256), (21000, 1024, 1024, L.TILE_AUTO)]
    for (M, N, K, tile) in cases:
        tag = "%dx%dx%d_t%d" % (M, N, K, tile)
        x32, w32, bias = rnd(M, K, g=g), rnd(N, K, g=g) * 0.05, rnd(N, g=g)
        base = d64(x32) @ d64(w32).t() + d64(bias)
        xh, wh, bd = ops.to_hilo(dev(x32)), ops.pack_weights(dev(w32), dt), dev(bias)
        y = ops.linear(xh, wh, bd, dt, tile=tile)
        report("f32x_linear_store_" + tag, d64(y.hi.cpu()) + d64(y.lo.cpu()), base, TOLX)
        y = ops.linear(xh, wh, bd, dt, out_f32=True, tile=tile)
        report("f32x_linear_store_f32out_" + tag, y, base, TOLX)
        y = ops.linear(xh, wh, bd, dt, epilogue=L.EPI_GELU, tile=tile)
        report("f32x_linear_gelu_" + tag, d64(y.hi.cpu()) + d64(y.lo.cpu()), F.gelu(base), TOLX)
        res, gamma, per = rnd(M, 2 * N, g=g), rnd(N, g=g), 137
        inj = rnd((M + per - 1) // per, N, g=g)
        ref = d64(res[:, N:]) + d64(gamma) * base
        out = torch.zeros(M, 2 * N, device=DEV)
        ops.linear(xh, wh, bd, dt, epilogue=L.EPI_RES, out=out[:, :N], res=dev(res)[:, N:], gamma=dev(gamma), tile=tile)
        report("f32x_linear_res_" + tag, out[:, :N], ref, TOLX)
        if N == 1024:
            ref2 = ref.clone()
            ref2[::per] += d64(inj[: ref2[::per].shape[0]])
            ops.linear(xh, wh, bd, dt, epilogue=L.EPI_RES, out=out[:, :N], res=dev(res)[:, N:], gamma=dev(gamma), inject=dev(inj), inj_period=per, tile=tile)
            report("f32x_linear_res_inject_" + tag, out[:, :N], ref2, TOLX)
    p0, p1, N, K = 100, 105, 1024, 640
    x32, w32, bias, table = rnd(2 * p0, K, g=g), rnd(N, K, g=g) * 0.05, rnd(N, g=g), rnd(p0 + 1, N, g=g)
    base = d64(x32) @ d64(w32).t() + d64(bias)
    ref = torch.zeros(2 * p1, N, dtype=torch.float64)
    for v in range(2):
        ref[v * p1 + 5: v * p1 + 5 + p0] = base[v * p0:(v + 1) * p0] + d64(table[1:])
    out = torch.zeros(2 * p1, N, device=DEV)
    ops.linear(ops.to_hilo(dev(x32)), ops.pack_weights(dev(w32), dt), dev(bias), dt, epilogue=L.EPI_PATCH, out=out, table=dev(table), p0=p0, p1=p1, row_off=5)
    report("f32x_linear_patch", out, ref, TOLX)
    # --- im2col -> HiLo (against the f32 kernel's output)
    imgs = torch.rand(2, 3, 56, 70, generator=g)
    c32 = ops.im2col_rgb(dev(imgs), torch.float32)
    cx = ops.im2col_rgb(dev(imgs), dt)
    report("f32x_im2col_rgb", d64(cx.hi.cpu()) + d64(cx.lo.cpu()), d64(c32.cpu()), 4e-7)
    # --- fused QKV (q/k-norm + RoPE), frame and global sequences, both tile sizes
    tpv, gw = 1374, 37
    cos, sin = orc.rope_tables(38)
    cos16, sin16 = dev(cos[:, :16].contiguous()), dev(sin[:, :16].contiguous())
    for mode, nviews, tile in (("frame", 2, L.TILE_AUTO), ("global", 2, L.TILE_AUTO), ("global", 2, L.TILE_256)):
        M = nviews * tpv
        seq = tpv if mode == "frame" else M
        x32, w32, bias = rnd(M, 1024, g=g), rnd(3072, 1024, g=g) * 0.03, rnd(3072, g=g) * 0.1
        qn = [rnd(64, g=g) * 0.1 + 1.5, rnd(64, g=g) * 0.1, rnd(64, g=g) * 0.1 + 1.5, rnd(64, g=g) * 0.1]
        for vn, qk_norm, rope in (("norm_rope", qn, (cos, sin)), ("plain", None, None)):
            qr, kr, vr = qkv_reference(d64(x32), d64(w32), d64(bias), seq, None if qk_norm is None else [d64(t) for t in qk_norm],
                                       None if rope is None else (d64(rope[0]), d64(rope[1])), tpv, gw)
            BH = (M // seq) * 16
            q, k, vt = ops.alloc_qkv(BH, seq, seq, dt, DEV)
            ops.qkv(ops.to_hilo(dev(x32)), ops.pack_weights(dev(w32), dt), dev(bias), seq, dt, q, k, vt,
                    qk_norm=None if qk_norm is None else [dev(t) for t in qk_norm], rope=None if rope is None else (cos16, sin16), tile=tile)
            val = lambda h: d64(h.hi.cpu()) + d64(h.lo.cpu())
            vtn = d64(ops.get_vt(vt.hi).cpu()) + d64(ops.get_vt(vt.lo).cpu())
            report("f32x_qkv_%s_%s_t%d.q" % (mode, vn, tile), val(q)[:, :seq], qr.reshape(BH, seq, 64), TOLX)
            report("f32x_qkv_%s_%s_t%d.k" % (mode, vn, tile), val(k)[:, :seq], kr.reshape(BH, seq, 64), TOLX)
            report("f32x_qkv_%s_%s_t%d.vt" % (mode, vn, tile), vtn[:, :, :seq], vr.reshape(BH, seq, 64).transpose(1, 2), TOLX)
            if not (float(val(q)[:, seq:].abs().max()) == 0.0 and float(vtn[:, :, seq:].abs().max()) == 0.0):
                print("[FAIL] f32x qkv padding was written")
                results.append({"name": "f32x_qkv_padding", "ok": False, "rel": float("nan")})
    # --- flash attention on (hi, lo) planes: single / multi / ragged segments, forced rescale, log-sum-exp
    def run_attn(tag, BH, nq, q32, ks32, vs32, tol=TOLX, want_lse=False):
        ref = attn_reference(d64(q32), torch.cat([d64(t) for t in ks32], 1), torch.cat([d64(t) for t in vs32], 1))
        ref_tok = ref.reshape(BH // 16, 16, nq, 64).permute(0, 2, 1, 3).reshape(-1, 1024)
        qd, _, _ = ops.alloc_qkv(BH, nq, 64, dt, DEV)
        qh = ops.to_hilo(dev(q32))
        qd.hi[:, :nq], qd.lo[:, :nq] = qh.hi, qh.lo
        segs = []
        for kk, vv in zip(ks32, vs32):
            nk = kk.shape[1]
            _, kd, vtd = ops.alloc_qkv(BH, 64, nk, dt, DEV)
            kh, vh = ops.to_hilo(dev(kk)), ops.to_hilo(dev(vv.transpose(1, 2).contiguous()))
            kd.hi[:, :nk], kd.lo[:, :nk] = kh.hi, kh.lo
            ops.set_vt(vtd.hi, vh.hi)
            ops.set_vt(vtd.lo, vh.lo)
            segs.append((kd, vtd, nk))
        # both forms of the PV contraction: all three products (the mode: 1e-5) and the opt-in form without P_lo x V_hi (variant
        # ATTN_F32X_FAST_PV) -- P is then one f16 value per key (2^-11 relative), so on these adversarially peaky random logits (sigma ~ 10:
        # a handful of keys carry a row) a row can be off by a few 1e-4 of the tensor maximum; the log-sum-exp is exact in both
        for form, variant, ftol in (("", 0, tol), ("_pv2", L.ATTN_F32X_FAST_PV, 4e-4)):
            lse = torch.zeros(BH, qd.shape[1], device=DEV) if want_lse else None
            out = ops.flash_attn(qd, segs, nq, dt, lse=lse, variant=variant)
            report("f32x_attn_" + tag + form, d64(out.hi.cpu()) + d64(out.lo.cpu()), ref_tok, ftol)
            if want_lse:
                s2 = d64(q32) @ torch.cat([d64(t) for t in ks32], 1).transpose(-1, -2)
                report("f32x_attn_" + tag + form + ".lse", lse[:, :nq], torch.logsumexp(s2 * math.log(2.0), -1) / math.log(2.0), 5e-6)
    shapes = [("n1374_bh32", 32, 1374, [1374]), ("n2748_2seg", 16, 1374, [1374, 1374]), ("n700_ragged_seg", 16, 700, [100, 333, 64]), ("n300_seg", 16, 300, [130, 70]),
              ("n500_short_segs", 16, 500, [40, 64, 7, 192, 129])]
    for cname, BH, nq, nks in (shapes[:2] if quick else shapes):
        run_attn(cname, BH, nq, rnd(BH, nq, 64, g=g) * 1.2, [rnd(BH, nk, 64, g=g) for nk in nks], [rnd(BH, nk, 64, g=g) for nk in nks], want_lse=(cname in ("n300_seg", "n500_short_segs") or quick))
    for cname, spike in (("spike", 6.0), ("spike_small", 1.0), ("ramp", 0.0)):
        BH, nq, nk = 16, 128, 640
        q32, k32, v32 = rnd(BH, nq, 64, g=g), rnd(BH, nk, 64, g=g), rnd(BH, nk, 64, g=g)
        if spike:
            k32[:, 500] = q32[:, 7] * spike
        else:
            k32 = k32 + q32[:, 3:4] * torch.linspace(0, 3, nk).view(1, nk, 1)
        run_attn(cname + "_rescale", BH, nq, q32, [k32], [v32])
    if not quick:      # one global-attention launch at the 8-view key count (10 992 keys: 172 tiles), sampled rows checked in float64
        BH, n = 16, 8 * 1374
        q32, k32, v32 = rnd(BH, n, 64, g=g) * 1.2, rnd(BH, n, 64, g=g), rnd(BH, n, 64, g=g)
        qd, kd, vtd = ops.alloc_qkv(BH, n, n, dt, DEV)
        for dst, src in ((qd, q32), (kd, k32)):
            h = ops.to_hilo(dev(src))
            dst.hi[:, :n], dst.lo[:, :n] = h.hi, h.lo
        vh = ops.to_hilo(dev(v32.transpose(1, 2).contiguous()))
        ops.set_vt(vtd.hi, vh.hi)
        ops.set_vt(vtd.lo, vh.lo)
        rows = torch.tensor([0, 1, 255, 256, 257, 4095, 5000, n - 257, n - 2, n - 1])
        ref = attn_reference(d64(q32[:, rows]), d64(k32), d64(v32)).permute(1, 0, 2).reshape(len(rows), 1024)
        for form, variant, ftol in (("", 0, TOLX), ("_pv2", L.ATTN_F32X_FAST_PV, 4e-4)):
            out = ops.flash_attn(qd, [(kd, vtd, n)], n, dt, variant=variant)
            report("f32x_attn_global_n10992_rows" + form, (d64(out.hi[rows.to(DEV)].cpu()) + d64(out.lo[rows.to(DEV)].cpu())), ref, ftol)


def test_heads(quick):
    """DPT-head entries (ovg_head_layernorm / ovg_conv / ovg_upsample / ovg_dpt_out) against their torch
    emulation (tests/head_ops_emul.py) on the same inputs in all three dtypes (f32 = the parity mode's exact-f32 MFMA
    convolutions, r03), then the whole HipDPTHead against the f32 PyTorch head on CPU (f32 gate 1e-4: the same
    arithmetic up to summation order and the out_conv-before-upsample reordering)."""
    import head_ops_emul as emul
    import importlib
    heads = importlib.import_module("omnivggt_official_amd.heads")
    heads_hip = importlib.import_module("omnivggt_official_amd.heads_hip")
    g = torch.Generator().manual_seed(9)
    for name, dt in (("bf16", torch.bfloat16), ("f16", torch.float16), ("f32", torch.float32)):
        tol = TOL[name]
        # LayerNorm(2048) with the special-token skip
        x = rnd(2 * 1374, 2048, g=g) * 2.0 + 0.3
        w, b = rnd(2048, g=g) * 0.2 + 1.0, rnd(2048, g=g) * 0.1
        got = ops.head_layernorm(x.to(DEV), w.to(DEV), b.to(DEV), 1e-5, dt, 2)
        report("head_layernorm_%s" % name, got, emul.head_layernorm(x, w, b, 1e-5, torch.float32, 2), tol)

        def conv_case(tag, n, H, W, cin, cout, k=1, stride=1, up=0, relu=False, adds=0, pos=False, bias=True, out_f32=False, pad_rows=False):
            x = (rnd(n, H, W, cin, g=g)).to(dt)
            rows = (up * up * cout) if up > 1 else cout
            wt = (rnd(rows, k * k * cin, g=g) * (1.0 / (k * k * cin) ** 0.5)).to(dt)
            if pad_rows:
                wp = torch.zeros(128, wt.shape[1], dtype=dt)
                wp[:rows] = wt
                wt = wp
            bs = rnd(cout, g=g) * 0.3 if bias else None
            pd = k // 2
            OH, OW = (H + 2 * pd - k) // stride + 1, (W + 2 * pd - k) // stride + 1
            a1 = rnd(n, OH, OW, cout, g=g).to(dt) if adds >= 1 else None
            a2 = rnd(n, OH, OW, cout, g=g).to(dt) if adds >= 2 else None
            ps = (rnd(OW, cout // 2, g=g) * 0.1, rnd(OH, cout // 2, g=g) * 0.1) if pos else None
            dv = lambda t: None if t is None else t.to(DEV)
            got = ops.conv(dv(x), dv(wt), dv(bs), dt, cout, ksize=k, stride=stride, upshuffle=up, relu=relu, add1=dv(a1), add2=dv(a2),
                           pos=None if ps is None else (dv(ps[0]), dv(ps[1])), out_f32=out_f32)
            ref = emul.conv(x, wt, bs, torch.float32, cout, ksize=k, stride=stride, upshuffle=up, relu=relu, add1=a1, add2=a2, pos=ps, out_f32=True)
            report("conv_%s_%s" % (tag, name), got, ref, 2e-5 if out_f32 else tol)

        conv_case("1x1_pos_2048to256", 2, 37, 37, 2048, 256, pos=True)
        conv_case("convT4_256", 1, 37, 37, 256, 256, up=4)
        conv_case("convT2_512", 1, 37, 37, 512, 512, up=2)
        conv_case("3x3s2_1024", 1, 37, 37, 1024, 1024, k=3, stride=2)
        conv_case("3x3_nobias_relu_512to256", 1, 74, 74, 512, 256, k=3, relu=True, bias=False)
        conv_case("3x3_add2_relu_256", 2, 37, 37, 256, 256, k=3, relu=True, adds=2)
        conv_case("3x3_add1_256_ragged", 1, 75, 53, 256, 256, k=3, adds=1)
        conv_case("3x3_256to128", 1, 60, 60, 256, 128, k=3)
        conv_case("3x3_128to32_f32out", 1, 70, 66, 128, 32, k=3, relu=True, out_f32=True, pad_rows=True)
        if not quick:
            conv_case("1x1_256", 1, 148, 148, 256, 256)
        # the 256 x 256 LDS-DMA conv kernel (ovg_conv256.h; 16-bit modes, GEMM columns % 256 == 0, >= 16384 output pixels): every tap / border /
        # epilogue form it serves, tiles that straddle two images (ragged widths), stride 2, the ConvTranspose scatter and the UV tables
        conv_case("c256_3x3_add2_relu_256_two_images", 3, 77, 75, 256, 256, k=3, relu=True, adds=2)
        conv_case("c256_3x3_nobias_relu_512to256", 1, 148, 148, 512, 256, k=3, relu=True, bias=False)
        conv_case("c256_1x1_pos_2048to512", 12, 37, 37, 2048, 512, pos=True)
        conv_case("c256_convT2_512", 12, 37, 37, 512, 512, up=2)
        conv_case("c256_3x3s2_1024", 14, 74, 74, 1024, 1024, k=3, stride=2)
        # round 6: the free-running loop's shortest k loops (2 k-stages: prologue + drain only) and the 128-column geometry (two workgroups per CU,
        # 3-slot ring: 18 and 72 k-stages, border taps through the out-of-range DMA offsets)
        conv_case("c256_1x1_64to256_two_stages", 1, 148, 148, 64, 256)
        conv_case("c256n_3x3_64to128", 1, 148, 148, 64, 128, k=3, relu=True)
        conv_case("c256n_3x3_256to128_two_images", 2, 131, 127, 256, 128, k=3, adds=1)
        # bilinear align_corners resize (+ UV tables)
        for tag, n, H, W, OH, OW, c, pos in (("19to37", 2, 19, 19, 37, 37, 256, False), ("37to74", 1, 37, 37, 74, 74, 256, False),
                                             ("148to296", 1, 148, 148, 296, 296, 256, False), ("296to518_pos", 1, 296, 296, 518, 518, 128, True)):
            x = rnd(n, H, W, c, g=g).to(dt)
            ps = (rnd(OW, c // 2, g=g) * 0.1, rnd(OH, c // 2, g=g) * 0.1) if pos else None
            got = ops.upsample(x.to(DEV), OH, OW, dt, pos=None if ps is None else (ps[0].to(DEV), ps[1].to(DEV)))
            report("upsample_%s_%s" % (tag, name), got, emul.upsample(x, OH, OW, torch.float32, pos=ps), tol)
    for act, od in (("exp", 2), ("inv_log", 4)):
        h = F.relu(rnd(3, 50, 41, 32, g=g))
        w2, b2 = rnd(od, 32, g=g) * 0.2, rnd(od, g=g) * 0.1
        val, conf = ops.dpt_out(h.to(DEV), w2.to(DEV), b2.to(DEV), act)
        rv, rc = emul.dpt_out(h, w2, b2, act)
        report("dpt_out_%s_val" % act, val, rv, 2e-5)
        report("dpt_out_%s_conf" % act, conf, rc, 2e-5)
    # the one-launch output stage (ovg_dpt_tail, 16-bit dtypes): vs the emulated chain on the same 16-bit inputs, and vs the three-launch HIP form
    # it replaces (ovg_upsample -> ovg_conv -> ovg_dpt_out); tiles cut by the image border in both directions, with / without the UV tables
    for name, dt in (("bf16", torch.bfloat16), ("f16", torch.float16)):
        for tag, n, H, W, OH, OW, od, act, pos in (("40to70_pos", 2, 40, 40, 70, 70, 2, "exp", True), ("ragged_53x47to75x61", 1, 53, 47, 75, 61, 4, "inv_log", False),
                                                   ("296to518_pos", 1, 296, 296, 518, 518, 4, "inv_log", True)):
            if quick and OH > 100:
                continue
            x = rnd(n, H, W, 128, g=g).to(dt)
            w1 = torch.zeros(128, 9 * 128, dtype=dt)
            w1[:32] = (rnd(32, 9 * 128, g=g) * (1.0 / (9 * 128) ** 0.5)).to(dt)
            b1, w2, b2 = rnd(32, g=g) * 0.3, rnd(od, 32, g=g) * 0.2, rnd(od, g=g) * 0.1
            ps = (rnd(OW, 64, g=g) * 0.1, rnd(OH, 64, g=g) * 0.1) if pos else None
            psd = None if ps is None else (ps[0].to(DEV), ps[1].to(DEV))
            xd, w1d, b1d, w2d, b2d = x.to(DEV), w1.to(DEV), b1.to(DEV), w2.to(DEV), b2.to(DEV)
            val, conf = ops.dpt_tail(xd, OH, OW, dt, psd, w1d, b1d, w2d, b2d, act)
            up = emul.upsample(x, OH, OW, dt, pos=ps)
            rv, rc = emul.dpt_out(emul.conv(up, w1, b1, torch.float32, 32, ksize=3, relu=True, out_f32=True), w2, b2, act)
            gate = 4e-3 if name == "bf16" else 5e-4
            report("dpt_tail_%s_%s_val" % (tag, name), val, rv, gate)
            report("dpt_tail_%s_%s_conf" % (tag, name), conf, rc, gate)
            hmap = ops.conv(ops.upsample(xd, OH, OW, dt, pos=psd), w1d, b1d, dt, 32, ksize=3, relu=True, out_f32=True)
            v3, c3 = ops.dpt_out(hmap, w2d, b2d, act)
            report("dpt_tail_%s_%s_val_vs_three_launches" % (tag, name), val, v3, gate)
            report("dpt_tail_%s_%s_conf_vs_three_launches" % (tag, name), conf, c3, gate)
    # whole head: HIP (16-bit) vs PyTorch f32 on CPU, S = 2
    for od, act in ((2, "exp"), (4, "inv_log")):
        torch.manual_seed(11 + od)
        head = heads.DPTHead(dim_in=2048, output_dim=od, activation=act, conf_activation="expp1", intermediate_layer_idx=(0, 1, 2, 3)).eval()
        with torch.no_grad():
            for pname, prm in head.named_parameters():
                if prm.dim() > 1:
                    prm.mul_(1.6)
                elif "bias" in pname:
                    prm.uniform_(-0.2, 0.2)
            last = head.scratch.output_conv2[2]
            last.weight.mul_(0.2 / float(last.weight.abs().max()))
            toks = [rnd(1, 2, 1374, 2048, g=g) * 0.7 for _ in range(4)]
            images = torch.zeros(1, 2, 3, 518, 518)
            rv, rc = head(toks, images=images, patch_start_idx=5)
            hip = heads_hip.HipDPTHead(head)
            toks_d = [t.to(DEV) for t in toks]
            for name, dt in (("bf16", torch.bfloat16), ("f16", torch.float16), ("f32", torch.float32)):
                val, conf = hip(toks_d, images.to(DEV), 5, dtype=dt)
                gate = {"bf16": 4e-2, "f16": 6e-3, "f32": 1e-4}[name]
                report("dpt_head_%s_%s_val" % (act, name), val, rv, gate)
                report("dpt_head_%s_%s_conf" % (act, name), conf, rc, gate)
            # per-frame results do not depend on how many frames a pass takes (model.dpt_frames_chunk: 64 on this part, 8 in the reference)
            v1, c1 = hip(toks_d, images.to(DEV), 5, frames_chunk_size=1, dtype=torch.bfloat16)
            v2, c2 = hip(toks_d, images.to(DEV), 5, frames_chunk_size=2, dtype=torch.bfloat16)
            report("dpt_head_%s_bf16_frame_chunking_is_bit_invariant" % act, torch.cat([v1.flatten(), c1.flatten()]), torch.cat([v2.flatten(), c2.flatten()]), 0.0)
            if quick:
                break


def test_embed():
    g = torch.Generator().manual_seed(6)
    V, Hp = 2, 518
    img = torch.rand(V, 3, Hp, Hp, generator=g)
    mean = torch.tensor(orc.RESNET_MEAN).view(1, 3, 1, 1)
    std = torch.tensor(orc.RESNET_STD).view(1, 3, 1, 1)
    xn = (img - mean) / std
    cols = F.unfold(xn, kernel_size=14, stride=14).transpose(1, 2).reshape(V * 1369, 588)
    for name, dt in DT.items():
        out = ops.im2col_rgb(img.to(DEV), dt)
        report("im2col_rgb_%s" % name, out[:, :588], cols, 1e-2 if name == "bf16" else (1e-3 if name == "f16" else 1e-6))
        pad_zero = float(out[:, 588:].abs().max()) == 0
        results.append({"name": "im2col_rgb_%s.pad_zero" % name, "ok": bool(pad_zero), "rel": 0.0})
        if not pad_zero:
            print("[FAIL] im2col pad not zero")
    depth = 0.5 + 5 * torch.rand(V, Hp, Hp, generator=g)
    mask = (torch.rand(V, Hp, Hp, generator=g) > 0.2).float()
    stats = ops.depth_stats(depth.reshape(1, -1).to(DEV), mask.reshape(1, -1).to(DEV)).cpu()
    valid = depth[mask > 0]
    report("depth_stats.sum", stats[:, 0], valid.double().sum().reshape(1), 1e-9)
    report("depth_stats.count", stats[:, 1], torch.tensor([float(valid.numel())]), 0.0)
    dn = orc.normalize_depth(depth.reshape(1, V, Hp, Hp, 1), mask.reshape(1, V, Hp, Hp)).reshape(V, 1, Hp, Hp)
    maps = torch.cat([dn, mask.reshape(V, 1, Hp, Hp)], dim=1)
    cols = F.unfold(maps, kernel_size=14, stride=14).transpose(1, 2).reshape(V * 1369, 392)
    out = ops.im2col_depth(depth.to(DEV), mask.to(DEV), stats.to(DEV), V, torch.float32)
    report("im2col_depth_f32", out[:, :392], cols, 2e-6)
    # dino specials + assemble
    P, S = 1374, 2
    x = torch.zeros(V * P, 1024, device=DEV)
    cls, pos0, reg = rnd(1024, g=g), rnd(1024, g=g), rnd(4, 1024, g=g)
    ops.dino_specials(x, V, P, cls.to(DEV), pos0.to(DEV), reg.to(DEV))
    ref = torch.zeros(V, P, 1024)
    ref[:, 0] = cls + pos0
    ref[:, 1:5] = reg
    report("dino_specials", x.view(V, P, 1024), ref, 0.0)
    xd = rnd(V * P, 1024, g=g)
    nw, nb = rnd(1024, g=g) * 0.1 + 1, rnd(1024, g=g) * 0.1
    cam, regt = rnd(2, 1024, g=g), rnd(2, 4, 1024, g=g)
    cam_add = rnd(V, 1024, g=g)
    dtok = rnd(1 * 1369, 1024, g=g)
    drow = torch.tensor([-1, 0], dtype=torch.int32)
    ph = rnd(1024, g=g)
    out = torch.zeros(V * P, 1024, device=DEV)
    ops.assemble_tokens(xd.to(DEV), nw.to(DEV), nb.to(DEV), 1e-6, cam.to(DEV), regt.to(DEV), cam_add.to(DEV), dtok.to(DEV),
                        drow.to(DEV), ph.to(DEV), out, V, S)
    ln = F.layer_norm(xd.view(V, P, 1024), (1024,), nw, nb, 1e-6)
    ref = torch.zeros(V, P, 1024)
    ref[0, 0] = cam[0] + cam_add[0]
    ref[1, 0] = cam[1] + cam_add[1]
    ref[0, 1:5], ref[1, 1:5] = regt[0], regt[1]
    ref[0, 5:] = ln[0, 5:] + ph
    ref[1, 5:] = ln[1, 5:] + dtok
    report("assemble_tokens", out.view(V, P, 1024), ref, 2e-6)


def test_block(quick):
    """One frame block and one global block through ovg_block_forward vs oracle.block."""
    from omnivggt_official_amd import aggregator as agg
    g = torch.Generator().manual_seed(7)
    S, P = 2, 1374
    keys = {}
    for nm, shape in (("norm1.weight", (1024,)), ("norm1.bias", (1024,)), ("attn.qkv.weight", (3072, 1024)), ("attn.qkv.bias", (3072,)),
                      ("attn.q_norm.weight", (64,)), ("attn.q_norm.bias", (64,)), ("attn.k_norm.weight", (64,)), ("attn.k_norm.bias", (64,)),
                      ("attn.proj.weight", (1024, 1024)), ("attn.proj.bias", (1024,)), ("ls1.gamma", (1024,)),
                      ("norm2.weight", (1024,)), ("norm2.bias", (1024,)), ("mlp.fc1.weight", (4096, 1024)), ("mlp.fc1.bias", (4096,)),
                      ("mlp.fc2.weight", (1024, 4096)), ("mlp.fc2.bias", (1024,)), ("ls2.gamma", (1024,))):
        from omnivggt_official_amd import weights
        keys["blk." + nm] = weights.draw("aggregator.frame_blocks.0." + nm, shape, seed=5)
    x = rnd(S * P, 1024, g=g)
    pos_yx = torch.cartesian_prod(torch.arange(37), torch.arange(37)) + 1
    pos = torch.cat([torch.zeros(5, 2, dtype=pos_yx.dtype), pos_yx]).unsqueeze(0).expand(S, -1, -1)
    rope = orc.rope_tables(38)
    inj = rnd(S, 1024, g=g)
    for name, dt in DT.items():
        if quick and name == "f16":
            continue
        for mode in ("frame", "global"):
            if mode == "frame":
                ref = orc.block(x.view(S, P, 1024), keys, "blk", pos, rope, True).reshape(S * P, 1024).clone()
                ref[::P] += inj
            else:
                ref = orc.block(x.view(1, S * P, 1024), keys, "blk", pos.reshape(1, S * P, 2), rope, True).reshape(S * P, 1024)
            runner = agg.BlockRunner(keys, "blk", dt, DEV, qk_norm=True, rope=True, ln_eps=1e-5)
            ws = agg.Workspace(S * P, P if mode == "frame" else S * P, dt, DEV)
            buf = torch.zeros(S * P, 2048, device=DEV)
            xin = x.to(DEV)
            runner.forward(ws, xin, buf[:, 1024:], inject=inj.to(DEV) if mode == "frame" else None, inj_period=P)
            tol = {"bf16": 3e-2, "f16": 6e-3, "f32": 5e-5}[name]
            report("block_%s_%s" % (name, mode), buf[:, 1024:], ref, tol)


# ---------------------------------------------------------------------------
# The kernels the 64-view bench actually runs (VERDICT r1 "close the parity hole under the headline number"):
# the 256 x 256 ping-pong GEMMs forced through `tile`, every epilogue, ragged M, and global attention at the
# real key counts.
# ---------------------------------------------------------------------------
def test_gemm256(quick, tile=None, auto_is=True):
    """linear256_kernel<STORE|GELU|RES(+inject)|PATCH> and qkv256_kernel (all three `part`s), forced with
    tile = OVG_TILE_256, against the same CPU f32 references as the 128 x 128 path; M % 256 != 0 everywhere."""
    g = torch.Generator().manual_seed(13)
    T256 = L.TILE_256 if tile is None else tile
    for name, dt in (("bf16", torch.bfloat16), ("f16", torch.float16)):
        tol = TOL[name]
        # (the short-K shapes walk the prologue / drain logic of the free-running loop: 2, 4 and 6 k-stages against a 4-slot ring)
        shapes = [(777, 1024, 1024), (33000, 4096, 1024), (33000, 1024, 4096), (777, 256, 64), (1000, 512, 128), (520, 256, 192)]
        if not quick and name == "bf16":
            shapes.append((64 * 1374, 4096, 1024))        # the bench's own M: 344 x 16 = 5504 workgroups, XCD remap at full size
        for (M, N, K) in shapes:
            x = rnd(M, K, g=g).to(dt)
            w = (rnd(N, K, g=g) * (0.05 if K == 1024 else 0.025)).to(dt)
            bias = rnd(N, g=g)
            base = x.float() @ w.float().t() + bias
            xd, wd, bd = x.to(DEV), w.to(DEV), bias.to(DEV)
            tag = "%s_%dx%dx%d" % (name, M, N, K)
            if M <= 33000:
                y = ops.linear(xd, wd, bd, dt, tile=T256)
                report("gemm256_store_" + tag, y, base, tol)
                y = ops.linear(xd, wd, bd, dt, out_f32=True, tile=T256)
                report("gemm256_store_f32out_" + tag, y, base, 2e-5)
            y = ops.linear(xd, wd, bd, dt, epilogue=L.EPI_GELU, tile=T256)
            report("gemm256_gelu_" + tag, y, F.gelu(base), tol)
            if N == 1024:
                res = rnd(M, 2 * N, g=g)
                gamma = rnd(N, g=g)
                per = 1374
                inj = rnd((M + per - 1) // per, N, g=g)
                ref = res[:, N:] + gamma * base
                resd = res.to(DEV)
                out = torch.zeros(M, 2 * N, device=DEV)
                ops.linear(xd, wd, bd, dt, epilogue=L.EPI_RES, out=out[:, :N], res=resd[:, N:], gamma=gamma.to(DEV), tile=T256)
                report("gemm256_res_" + tag, out[:, :N], ref, 2e-5)
                ref2 = ref.clone()
                ref2[::per] += inj[: ref2[::per].shape[0]]
                ops.linear(xd, wd, bd, dt, epilogue=L.EPI_RES, out=out[:, :N], res=resd[:, N:], gamma=gamma.to(DEV), inject=inj.to(DEV),
                           inj_period=per, tile=T256)
                report("gemm256_res_inject_" + tag, out[:, :N], ref2, 2e-5)
                # in place on the residual stream (x_out aliases res), as ovg_block_forward's fc2 runs it
                buf = resd[:, N:].clone()
                ops.linear(xd, wd, bd, dt, epilogue=L.EPI_RES, out=buf, res=buf, gamma=gamma.to(DEV), tile=T256)
                report("gemm256_res_inplace_" + tag, buf, ref, 2e-5)
        # automatic choice == forced choice where the heuristic picks 256 (M >= 32768, light epilogue): bit-identical
        x = rnd(33000, 1024, g=g).to(dt).to(DEV)
        w = (rnd(4096, 1024, g=g) * 0.05).to(dt).to(DEV)
        b = rnd(4096, g=g).to(DEV)
        ya, yf, y1 = ops.linear(x, w, b, dt), ops.linear(x, w, b, dt, tile=T256), ops.linear(x, w, b, dt, tile=L.TILE_128)
        if auto_is:
            report("gemm256_auto_is_256_%s" % name, ya, yf.float(), 0.0)
        report("gemm256_vs_128_%s" % name, yf, y1.float(), tol)
        # PATCH epilogue (DINO patch embed: K = 640, rows remapped past the 5 special tokens)
        p0, p1 = 1369, 1374
        M, N, K = 3 * p0, 1024, 640
        x = rnd(M, K, g=g).to(dt)
        w = (rnd(N, K, g=g) * 0.05).to(dt)
        bias = rnd(N, g=g)
        table = rnd(p0 + 1, N, g=g)
        base = x.float() @ w.float().t() + bias
        ref = torch.zeros(3 * p1, N)
        for v in range(3):
            ref[v * p1 + 5: v * p1 + 5 + p0] = base[v * p0:(v + 1) * p0] + table[1:]
        out = torch.zeros(3 * p1, N, device=DEV)
        ops.linear(x.to(DEV), w.to(DEV), bias.to(DEV), dt, epilogue=L.EPI_PATCH, out=out, table=table.to(DEV), p0=p0, p1=p1, row_off=5, tile=T256)
        report("gemm256_patch_%s" % name, out, ref, 2e-5)
        # an illegal forced tile is refused, not silently replaced
        try:
            ops.linear(x.to(DEV)[:, :640], w.to(DEV)[:128], None, dt, tile=T256)
            results.append({"name": "gemm256_illegal_n_refused_" + name, "ok": False, "rel": float("nan")})
            print("[FAIL] tile=256 with N=128 was accepted")
        except L.OvgError:
            results.append({"name": "gemm256_illegal_n_refused_" + name, "ok": True, "rel": 0.0})

    # fused QKV: 24 views (M = 32 976 = 128 x 256 + 208), global and frame sequences, part 0 / 1 + 2
    tpv, gw = 1374, 37
    cos, sin = orc.rope_tables(38)
    cos16, sin16 = cos[:, :16].contiguous().to(DEV), sin[:, :16].contiguous().to(DEV)
    for name, dt in (("bf16", torch.bfloat16), ("f16", torch.float16)):
        nviews = 24
        M = nviews * tpv
        x = rnd(M, 1024, g=g).to(dt)
        w = (rnd(3072, 1024, g=g) * 0.03).to(dt)
        bias = rnd(3072, g=g) * 0.1
        qn = [rnd(64, g=g) * 0.1 + 1.5, rnd(64, g=g) * 0.1, rnd(64, g=g) * 0.1 + 1.5, rnd(64, g=g) * 0.1]
        qnd = [t.to(DEV) for t in qn]
        xd, wd, bd = x.to(DEV), w.to(DEV), bias.to(DEV)
        for mode in ("global", "frame"):
            seq = tpv if mode == "frame" else M
            qr, kr, vr = qkv_reference(x.float(), w.float(), bias, seq, qn, (cos, sin), tpv, gw)
            BH = (M // seq) * 16
            tol = TOL[name] * 2
            q, k, vt = ops.alloc_qkv(BH, seq, seq, dt, DEV)
            ops.qkv(xd, wd, bd, seq, dt, q, k, vt, qk_norm=qnd, rope=(cos16, sin16), tile=T256)
            report("qkv256_%s_%s.q" % (name, mode), q[:, :seq], qr.reshape(BH, seq, 64), tol)
            report("qkv256_%s_%s.k" % (name, mode), k[:, :seq], kr.reshape(BH, seq, 64), tol)
            report("qkv256_%s_%s.vt" % (name, mode), ops.get_vt(vt)[:, :, :seq], vr.reshape(BH, seq, 64).transpose(1, 2), tol)
            ok_pad = float(q[:, seq:].abs().max()) == 0.0 and float(k[:, seq:].abs().max()) == 0.0 and float(ops.get_vt(vt)[:, :, seq:].abs().max()) == 0.0
            results.append({"name": "qkv256_%s_%s.padding_untouched" % (name, mode), "ok": ok_pad, "rel": 0.0})
            if not ok_pad:
                print("[FAIL] qkv256 wrote padding rows")
            q2, k2, vt2 = ops.alloc_qkv(BH, seq, seq, dt, DEV)
            ops.qkv(xd, wd, bd, seq, dt, q2, k2, vt2, qk_norm=qnd, rope=(cos16, sin16), part=1, tile=T256)
            kv_only = float(q2.abs().max()) == 0.0
            ops.qkv(xd, wd, bd, seq, dt, q2, k2, vt2, qk_norm=qnd, rope=(cos16, sin16), part=2, tile=T256)
            same = kv_only and torch.equal(q2, q) and torch.equal(k2, k) and torch.equal(vt2, vt)
            results.append({"name": "qkv256_%s_%s.part1+part2==part0" % (name, mode), "ok": bool(same), "rel": 0.0})
            print("[%s] qkv256_%s_%s part 1 + part 2 == part 0 (bitwise), part 1 leaves q alone" % ("PASS" if same else "FAIL", name, mode), flush=True)
            if mode == "global" and auto_is:       # the automatic choice at this M is the 256 kernel as well
                q3, k3, vt3 = ops.alloc_qkv(BH, seq, seq, dt, DEV)
                ops.qkv(xd, wd, bd, seq, dt, q3, k3, vt3, qk_norm=qnd, rope=(cos16, sin16))
                results.append({"name": "qkv256_%s_auto_is_256" % name, "ok": bool(torch.equal(q3, q) and torch.equal(k3, k) and torch.equal(vt3, vt)), "rel": 0.0})


def _attn_ref_rows_gpu(q, k, v, rows):
    """f32 softmax(q k^T) v on the DEVICE with plain torch ops for the selected query rows of every head (base-2 logits)."""
    qs = q[:, rows].float()
    s = torch.matmul(qs, k.float().transpose(1, 2)) * math.log(2.0)
    return torch.matmul(torch.softmax(s, dim=-1), v.float())


def test_attn_big(quick):
    """Global attention at the bench's key counts: N = 10 992 (8 views) and 21 984 (16 views) in FULL against a plain
    torch f32 evaluation (device, head by head), N = 87 936 (64 views) on sampled query rows -- first / last workgroup,
    a 256-row tile boundary, rows spread over every XCD's share of the grid -- plus a float64 CPU evaluation of a few
    rows for independence from the device BLAS. Variants: default (speculative), lazy-rescale, forced fallback."""
    g = torch.Generator().manual_seed(17)
    cases = [("bf16", torch.bfloat16, 8, (0, 50, 52, 53, 54, 57, 72)), ("f16", torch.float16, 8, (0, 50, 52, 72)), ("bf16", torch.bfloat16, 16, (0,)),
             ("bf16", torch.bfloat16, 11, (0, 72))]   # 72 / 0 at 8 and 11 views: the 256-row launch with its 128-row tail launch (1.34 / 1.85 rounds)
    if not quick:
        cases.append(("bf16", torch.bfloat16, 64, (0, 50, 52, 53, 57)))
        cases.append(("f16", torch.float16, 64, (0,)))
    for name, dt, S, variants in cases:
        n = S * 1374
        BH = 16
        q, k, vt = ops.alloc_qkv(BH, n, n, dt, DEV)
        q[:, :n] = (torch.randn(BH, n, 64, generator=g) * 1.2).to(dt).to(DEV)
        k[:, :n] = torch.randn(BH, n, 64, generator=g).to(dt).to(DEV)
        v = torch.randn(BH, n, 64, generator=g).to(dt).to(DEV)
        ops.set_vt(vt, v.transpose(1, 2))
        if S <= 16:
            rows = torch.arange(n, device=DEV)
        else:
            pick = set(range(0, 260)) | set(range(n - 300, n))
            for t in range(1, 8):
                base = (n * t // 8) // 256 * 256
                pick |= set(range(base - 3, base + 4))
            pick |= set(range(17, n, 1009))
            rows = torch.tensor(sorted(pick), device=DEV)
        ref = torch.cat([_attn_ref_rows_gpu(q[h:h + 1, :n], k[h:h + 1, :n], v[h:h + 1], rows) for h in range(BH)])   # [16, R, 64]
        ref_tok = ref.permute(1, 0, 2).reshape(rows.numel(), 1024)
        # independent float64 check of the reference itself on a few rows (CPU)
        r64 = rows[:: max(1, rows.numel() // 24)][:24].cpu()
        s64 = (q[:, r64].double().cpu() @ k[:, :n].double().cpu().transpose(1, 2)) * math.log(2.0)
        o64 = (torch.softmax(s64, -1) @ v.double().cpu()).permute(1, 0, 2).reshape(r64.numel(), 1024)
        sel = torch.searchsorted(rows.cpu(), r64)
        report("attn_big_%s_S%d_device_ref_vs_f64" % (name, S), ref_tok[sel.to(DEV)], o64.float(), 2e-5)
        for variant in variants:
            out = ops.flash_attn(q, [(k, vt, n)], n, dt, variant=variant)
            report("attn_big_%s_S%d_N%d_v%d_%s" % (name, S, n, variant, "full" if S <= 16 else "%drows" % rows.numel()), out[rows], ref_tok, TOL[name])
        del q, k, vt, v, ref, ref_tok
        torch.cuda.empty_cache()


def test_attn_lse_merge():
    """Two launches over disjoint key sets + ovg_attn_merge == one launch over all keys (the local-first all-gather
    path of sharding.py); the per-row log-sum-exp itself against torch.logsumexp; every kernel family."""
    g = torch.Generator().manual_seed(19)
    for name, dt in DT.items():
        BH, nq, nka, nkb = 16, 1374, 1374, 2 * 1374 - 77
        q = (rnd(BH, nq, 64, g=g) * 1.2).to(dt)
        ka, kb = rnd(BH, nka, 64, g=g).to(dt), rnd(BH, nkb, 64, g=g).to(dt)
        va, vb = rnd(BH, nka, 64, g=g).to(dt), rnd(BH, nkb, 64, g=g).to(dt)
        kall, vall = torch.cat([ka, kb], 1).float(), torch.cat([va, vb], 1).float()
        ref = attn_reference(q.float(), kall, vall).permute(1, 0, 2).reshape(nq, 1024)
        lse_ref_a = torch.logsumexp((q.float() @ ka.float().transpose(1, 2)) * math.log(2.0), -1) / math.log(2.0)
        qd, kad, vtad = ops.alloc_qkv(BH, nq, nka, dt, DEV)
        _, kbd, vtbd = ops.alloc_qkv(BH, 64, nkb, dt, DEV)
        qd[:, :nq] = q.to(DEV)
        kad[:, :nka] = ka.to(DEV); ops.set_vt(vtad, va.transpose(1, 2))
        kbd[:, :nkb] = kb.to(DEV); ops.set_vt(vtbd, vb.transpose(1, 2))
        for variant in ((1,) if name == "f32" else ATTN16_VARIANTS):
            la = torch.full((BH, qd.shape[1]), float("nan"), device=DEV)
            lb = torch.full((BH, qd.shape[1]), float("nan"), device=DEV)
            oa = ops.flash_attn(qd, [(kad, vtad, nka)], nq, dt, variant=variant, lse=la)
            ob = ops.flash_attn(qd, [(kbd, vtbd, nkb)], nq, dt, variant=variant, lse=lb)
            report("attn_lse_%s_v%d" % (name, variant), la[:, :nq], lse_ref_a, 2e-5 if name == "f32" else 2e-3)
            merged = ops.attn_merge(oa, la, ob, lb, dt, out=oa)          # in place on launch A's output, like sharding.py
            report("attn_merge_%s_v%d" % (name, variant), merged, ref, TOL[name] * (1.5 if name != "f32" else 1))
    # tail split of the automatic plan (16 views = 2.69 rounds of 512-row tiles -> 512-row launch + 128-row tail launch): outputs and
    # log-sum-exps of BOTH launches against the baseline kernel on the same device buffers, token-major and head-major
    g2 = torch.Generator().manual_seed(23)
    BH, n = 16, 16 * 1374
    qd, kd, vtd = ops.alloc_qkv(BH, n, n, torch.bfloat16, DEV)
    qd[:, :n] = (rnd(BH, n, 64, g=g2) * 1.3).to(torch.bfloat16).to(DEV)
    kd[:, :n] = rnd(BH, n, 64, g=g2).to(torch.bfloat16).to(DEV)
    ops.set_vt(vtd, rnd(BH, 64, n, g=g2).to(torch.bfloat16))
    l1 = torch.full((BH, qd.shape[1]), float("nan"), device=DEV)
    l0 = torch.full((BH, qd.shape[1]), float("nan"), device=DEV)
    o1 = ops.flash_attn(qd, [(kd, vtd, n)], n, torch.bfloat16, variant=1, lse=l1)
    o0 = ops.flash_attn(qd, [(kd, vtd, n)], n, torch.bfloat16, variant=0, lse=l0)
    report("attn_tailsplit_bf16_S16_out", o0, o1, TOL["bf16"])
    report("attn_tailsplit_bf16_S16_lse", l0[:, :n], l1[:, :n], 2e-3)
    h0 = ops.flash_attn(qd, [(kd, vtd, n)], n, torch.bfloat16, variant=0, head_major=True)
    report("attn_tailsplit_bf16_S16_headmajor", h0[:, :n].permute(1, 0, 2).reshape(n, 1024), o1, TOL["bf16"])
    del qd, kd, vtd, o0, o1, h0
    # key-split tail of the automatic plan (13 views = 2.19 rounds of 256-row tiles -> 16384 rows unsplit + 1478 rows cut into 5 key ranges + merge;
    # 8 views = 1.34 rounds: not taken automatically, forced here through the A/B variant 73): outputs and log-sum-exps against the baseline kernel and against the SAME kernel unsplit
    # (f32 partials: the split rows must agree with the unsplit launch to 1e-3, round-4 review item 4), token-major and head-major, bf16 and f16
    for name, dt, S, kt_variant, kt_splits in (("bf16", torch.bfloat16, 13, 0, 0), ("f16", torch.float16, 13, 0, 0), ("bf16", torch.bfloat16, 8, 73, 2)):   # last: forced (A/B knob)
        BH, n = 16, S * 1374
        qd, kd, vtd = ops.alloc_qkv(BH, n, n, dt, DEV)
        qd[:, :n] = (rnd(BH, n, 64, g=g2) * 1.3).to(dt).to(DEV)
        kd[:, :n] = rnd(BH, n, 64, g=g2).to(dt).to(DEV)
        ops.set_vt(vtd, rnd(BH, 64, n, g=g2).to(dt))
        plan = ops.attn_plan(BH, n, [n], dt, kt_variant, kt_splits, nq_pad=qd.shape[1])
        ok_plan = plan["splits"] > 1 and plan["main_rows"] < n and plan["tail_q_tile"] == plan["q_tile"] == 256
        results.append({"name": "attn_keytail_%s_S%d_plan" % (name, S), "ok": bool(ok_plan), "rel": 0.0})
        print("[%s] attn_keytail_%s_S%d plan %s" % ("PASS" if ok_plan else "FAIL", name, S, plan), flush=True)
        ws = ops.alloc_split_ws(plan, DEV)
        l1 = torch.full((BH, qd.shape[1]), float("nan"), device=DEV)
        l0 = torch.full((BH, qd.shape[1]), float("nan"), device=DEV)
        o1 = ops.flash_attn(qd, [(kd, vtd, n)], n, dt, variant=1, lse=l1)
        o0 = ops.flash_attn(qd, [(kd, vtd, n)], n, dt, variant=kt_variant, kv_splits=kt_splits, lse=l0, split_ws=ws)
        ou = ops.flash_attn(qd, [(kd, vtd, n)], n, dt, variant=0, kv_splits=1)
        report("attn_keytail_%s_S%d_out" % (name, S), o0, o1, TOL[name])
        report("attn_keytail_%s_S%d_lse" % (name, S), l0[:, :n], l1[:, :n], 2e-3)
        # split rows vs the unsplit launch: f32 partials + exact merge; what remains is the 16-bit rounding of P against a different softmax
        # anchor per key range and the final rounding: at most one ulp of the output -- 2^-8 (bf16) / 2^-11 (f16) of the value (bf16 partials: 6.9e-3)
        report("attn_keytail_%s_S%d_vs_unsplit" % (name, S), o0, ou.float(), 4e-3 if name == "bf16" else 1e-3)
        frac_diff = float((o0 != ou).float().mean())
        print("       attn_keytail_%s_S%d: %.2f %% of the outputs differ from the unsplit launch (speculative-softmax anchors differ per key range: P rounds differently)" % (name, S, 100 * frac_diff), flush=True)
        h0 = ops.flash_attn(qd, [(kd, vtd, n)], n, dt, variant=kt_variant, kv_splits=kt_splits, head_major=True, split_ws=ws)
        report("attn_keytail_%s_S%d_headmajor" % (name, S), h0[:, :n].permute(1, 0, 2).reshape(n, 1024), o1, TOL[name])
        try:                                                   # the tail workspace is checked like the whole-launch one
            ops.flash_attn(qd, [(kd, vtd, n)], n, dt, variant=kt_variant, kv_splits=kt_splits, split_ws=(ws[0][: ws[0].numel() // 2], ws[1]))
            results.append({"name": "attn_keytail_%s_S%d_small_ws_refused" % (name, S), "ok": False, "rel": float("nan")})
            print("[FAIL] undersized key-split tail workspace accepted")
        except L.OvgError:
            results.append({"name": "attn_keytail_%s_S%d_small_ws_refused" % (name, S), "ok": True, "rel": 0.0})
        del qd, kd, vtd, o0, o1, ou, h0, ws
    # split-KV: forced 2..8 key splits (+ the library's own plan) == the single-pass result, token-major and head-major,
    # ragged multi-segment key lists, with the total log-sum-exp output
    for name, dt in (("bf16", torch.bfloat16), ("f16", torch.float16)):
        BH, nq, nks = 16, 700, [1374, 999, 64, 2000]
        q = (rnd(BH, nq, 64, g=g) * 1.2).to(dt)
        ks = [rnd(BH, nk, 64, g=g).to(dt) for nk in nks]
        vs = [rnd(BH, nk, 64, g=g).to(dt) for nk in nks]
        kall, vall = torch.cat(ks, 1).float(), torch.cat(vs, 1).float()
        ref = attn_reference(q.float(), kall, vall)
        ref_tok = ref.permute(1, 0, 2).reshape(nq, 1024)
        lse_ref = torch.logsumexp((q.float() @ kall.transpose(1, 2)) * math.log(2.0), -1) / math.log(2.0)
        qd, _, _ = ops.alloc_qkv(BH, nq, 64, dt, DEV)
        qd[:, :nq] = q.to(DEV)
        segs = []
        for kk, vv in zip(ks, vs):
            nk = kk.shape[1]
            _, kd, vtd = ops.alloc_qkv(BH, 64, nk, dt, DEV)
            kd[:, :nk] = kk.to(DEV)
            ops.set_vt(vtd, vv.transpose(1, 2))
            segs.append((kd, vtd, nk))
        for variant in (0, 50, 52, 53, 54, 55, 57):
            for splits in (0, 2, 3, 5, 8):
                plan = ops.attn_plan(BH, nq, nks, dt, variant, splits, nq_pad=qd.shape[1])
                ws = ops.alloc_split_ws(plan, DEV)
                lse = torch.full((BH, qd.shape[1]), float("nan"), device=DEV)
                out = ops.flash_attn(qd, segs, nq, dt, variant=variant, kv_splits=splits, split_ws=ws, lse=lse)
                tag = "attn_splitkv_%s_v%d_s%d(plan %d)" % (name, variant, splits, plan["splits"])
                report(tag, out, ref_tok, TOL[name] * 1.5)
                report(tag + ".lse", lse[:, :nq], lse_ref, 2e-3)
            hm = ops.flash_attn(qd, segs, nq, dt, variant=variant, kv_splits=4, head_major=True,
                                split_ws=ops.alloc_split_ws(ops.attn_plan(BH, nq, nks, dt, variant, 4, nq_pad=qd.shape[1]), DEV))
            report("attn_splitkv_%s_v%d_headmajor" % (name, variant), hm[:, :nq], ref, TOL[name] * 1.5)
    # weight pre-pack == torch's own rounding, zero padding
    w = rnd(1024, 3, 14, 14, g=g)
    for name, dt in DT.items():
        got = ops.pack_weights(w.to(DEV), dt, k_pad=640)
        exp = torch.zeros(1024, 640)
        exp[:, :588] = w.reshape(1024, -1).to(dt).float()
        report("pack_weights_%s" % name, got, exp, 0.0)


def test_camera_head(timing=False):
    """ovg_camera_head (csrc/ovg_camhead.hip) through heads_hip.HipCameraHead against (i) the torch restatement of the
    entry on the same packed weights (tests/head_ops_emul.camera_head: same rounding points, f32 accumulate) and
    (ii) the f32 PyTorch CameraHead module on CPU (the reference's arithmetic, heads/camera_head.py:84-154).
    S = 3 (one partial 16-row block), 8, 70 (two 64-token z slices, ragged), 128; also B = 2 and a strided token view."""
    import head_ops_emul as emul
    import importlib
    heads = importlib.import_module("omnivggt_official_amd.heads")
    heads_hip = importlib.import_module("omnivggt_official_amd.heads_hip")
    torch.manual_seed(21)
    head = heads.CameraHead(dim_in=2048).eval()
    with torch.no_grad():
        for name, p in head.named_parameters():        # sensitised: LayerScale ~ 0.7, non-zero empty pose, wider matrices
            if name.endswith("gamma"):
                p.fill_(0.7)
            elif name == "empty_pose_tokens":
                p.normal_(0, 0.5)
            elif p.dim() > 1:
                p.mul_(1.5)
            elif "bias" in name:
                p.uniform_(-0.1, 0.1)
    g = torch.Generator().manual_seed(4)
    head_dev = heads.CameraHead(dim_in=2048).eval()
    head_dev.load_state_dict(head.state_dict())
    head_dev = head_dev.to(DEV)
    hip = heads_hip.HipCameraHead(head_dev)
    tol_twin = {"bf16": 1.5e-2, "f16": 2e-3, "f32": 1e-5}        # f32: nothing is rounded below f32, the twin IS the module's arithmetic
    tol_mod = {"bf16": 4e-2, "f16": 5e-3, "f32": 1e-5}
    for name, dt in (("bf16", torch.bfloat16), ("f16", torch.float16), ("f32", torch.float32)):
        for B, S in ((1, 3), (1, 8), (2, 8), (1, 70), (1, 128)):
            toks = rnd(B, S, 3, 2048, g=g) * 1.3                       # tokens_per_view = 3: row stride 3 * 2048
            with torch.no_grad():
                ref32 = torch.stack(head([toks]), 0)                   # [4, B, S, 9] f32 module on CPU
                W = hip._weights(dt, torch.device(DEV))
                Wc = {k: (v.cpu() if torch.is_tensor(v) else v) for k, v in W.items() if k != "blocks"}
                Wc["blocks"] = [{k: v.cpu() for k, v in blk.items()} for blk in W["blocks"]]
                twin = torch.stack([emul.camera_head(toks[b, :, 0], Wc, dt) for b in range(B)], 1)
                got = torch.stack(hip([toks.to(DEV)], dtype=dt), 0)
            tag = "camera_head_%s_B%d_S%d" % (name, B, S)
            report(tag + "_vs_twin", got, twin, tol_twin[name])
            report(tag + "_vs_f32_module", got, ref32, tol_mod[name])
            for grp, sl in (("T", slice(0, 3)), ("quat", slice(3, 7)), ("fov", slice(7, 9))):      # each component group against its own maximum
                report("%s_vs_twin.%s" % (tag, grp), got[..., sl], twin[..., sl], tol_twin[name])
                report("%s_vs_f32_module.%s" % (tag, grp), got[..., sl], ref32[..., sl], tol_mod[name])
    if timing:
        toks = (rnd(1, 8, 1374, 2048, g=g) * 1.3).to(DEV)
        for label, fn in (("hip bf16", lambda: hip([toks], dtype=torch.bfloat16)), ("hip f32", lambda: hip([toks], dtype=torch.float32)),
                          ("pytorch f32", lambda: head_dev([toks]))):
            with torch.no_grad():
                ms = bench(fn, iters=20, warm=5)
            print("camera head S=8 %-12s %.3f ms per forward (4 refinement rounds)" % (label, ms), flush=True)


def bench(fn, iters=10, warm=3):
    for _ in range(warm):
        fn()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(iters):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / iters


def microbench():
    print("---- micro-benchmarks (bf16, random data) ----", flush=True)
    g = torch.Generator().manual_seed(9)
    dt = torch.bfloat16
    out = {}
    for S in (8, 16):
        M = S * 1374
        x = rnd(M, 1024, g=g).to(dt).to(DEV)
        for nm, N, K in (("qkv-shape", 3072, 1024), ("proj", 1024, 1024), ("fc1", 4096, 1024), ("fc2", 1024, 4096)):
            xx = x if K == 1024 else rnd(M, K, g=g).to(dt).to(DEV)
            w = (rnd(N, K, g=g) * 0.03).to(dt).to(DEV)
            b = torch.zeros(N, device=DEV)
            y = torch.empty(M, N, device=DEV, dtype=dt)
            ms = bench(lambda: ops.linear(xx, w, b, dt, out=y))
            tf = 2.0 * M * N * K / ms / 1e9
            print("gemm %-10s S=%d M=%d N=%d K=%d: %.3f ms  %.1f TFLOP/s" % (nm, S, M, N, K, ms, tf), flush=True)
            out["gemm_%s_S%d" % (nm, S)] = {"ms": ms, "tflops": tf}
        # global attention
        for variant in (1, 0):
            BH, n = 16, M
            q, k, vt = ops.alloc_qkv(BH, n, n, dt, DEV)
            q[:, :n] = rnd(BH, n, 64, g=g).to(dt).to(DEV)
            k[:, :n] = rnd(BH, n, 64, g=g).to(dt).to(DEV)
            ops.set_vt(vt, rnd(BH, 64, n, g=g).to(dt))
            o = torch.empty(n, 1024, device=DEV, dtype=dt)
            ms = bench(lambda: ops.flash_attn(q, [(k, vt, n)], n, dt, out=o, variant=variant), iters=5)
            tf = 4.0 * n * n * 1024 / ms / 1e9
            print("global attn S=%d N=%d variant(QB)=%d: %.3f ms  %.1f TFLOP/s (%.1f%% of 2.5 PF)" % (S, n, variant, ms, tf, tf / 25.0), flush=True)
            out["gattn_S%d_qb%d" % (S, variant)] = {"ms": ms, "tflops": tf}
        # frame attention
        for variant in (1, 0):
            BH, n = S * 16, 1374
            q, k, vt = ops.alloc_qkv(BH, n, n, dt, DEV)
            q[:, :n] = rnd(BH, n, 64, g=g).to(dt).to(DEV)
            k[:, :n] = rnd(BH, n, 64, g=g).to(dt).to(DEV)
            ops.set_vt(vt, rnd(BH, 64, n, g=g).to(dt))
            o = torch.empty(S * n, 1024, device=DEV, dtype=dt)
            ms = bench(lambda: ops.flash_attn(q, [(k, vt, n)], n, dt, out=o, variant=variant), iters=5)
            tf = 4.0 * BH * n * n * 64 / ms / 1e9
            print("frame attn S=%d variant(QB)=%d: %.3f ms  %.1f TFLOP/s" % (S, variant, ms, tf), flush=True)
            out["fattn_S%d_qb%d" % (S, variant)] = {"ms": ms, "tflops": tf}
        xf = rnd(M, 1024, g=g).to(DEV)
        w1 = torch.ones(1024, device=DEV)
        y = torch.empty(M, 1024, device=DEV, dtype=dt)
        ms = bench(lambda: ops.layernorm(xf, w1, w1, 1e-5, dt, out=y))
        print("layernorm S=%d: %.3f ms  %.1f GB/s" % (S, ms, M * 1024 * 6 / ms / 1e6), flush=True)
        out["ln_S%d" % S] = {"ms": ms}
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--quick", action="store_true")
    ap.add_argument("--bench", action="store_true")
    ap.add_argument("--only", default="")
    ap.add_argument("--alt-lib", default="", help="name of an alternate build under tools/probes/_build/ (build_alt.py) to run the checks on instead of the product library")
    args = ap.parse_args()
    L.require_gpu()
    if args.alt_lib:
        import ctypes
        alt = ctypes.CDLL(os.path.join(ROOT, "tools", "probes", "_build", args.alt_lib, "libomnivggt_hip.so"))
        for name, (res, a) in L.SYMBOLS.items():
            f = getattr(alt, name)
            f.restype, f.argtypes = res, a
        L.load()
        L._lib = alt
        print("checks run on the alternate build", args.alt_lib, flush=True)
    print(L.load().ovg_build_info().decode(), torch.cuda.get_device_name(0), flush=True)
    tests = {"probe": test_probe, "layernorm": test_layernorm, "linear": lambda: test_linear(args.quick), "qkv": lambda: test_qkv(args.quick),
             "attn": lambda: test_attn(args.quick), "embed": test_embed, "block": lambda: test_block(args.quick),
             "heads": lambda: test_heads(args.quick), "gemm256": lambda: test_gemm256(args.quick),
             "attn_big": lambda: test_attn_big(args.quick),
             "lse_merge": test_attn_lse_merge, "camera": lambda: test_camera_head(timing=True), "f32x": lambda: test_f32x(args.quick), "fallback": test_attn_fallback_counter}
    for name, fn in tests.items():
        if args.only and name not in args.only.split(","):
            continue
        t0 = time.time()
        try:
            fn()
        except Exception as e:  # keep going: one log should show every problem
            import traceback
            traceback.print_exc()
            print("[FAIL] %s raised %r" % (name, e), flush=True)
            results.append({"name": name + "_exception", "ok": False, "rel": float("nan")})
        torch.cuda.synchronize()
        print("  (%s: %.1fs)" % (name, time.time() - t0), flush=True)
    nfail = sum(1 for r in results if not r["ok"])
    print("SELFTEST: %d checks, %d failed" % (len(results), nfail), flush=True)
    mb = microbench() if args.bench else {}
    os.makedirs(os.path.join(ROOT, "gpurun_out"), exist_ok=True)
    json.dump({"results": results, "microbench": mb}, open(os.path.join(ROOT, "gpurun_out", "selftest.json"), "w"), indent=1)
    return 1 if nfail else 0


if __name__ == "__main__":
    sys.exit(main())
