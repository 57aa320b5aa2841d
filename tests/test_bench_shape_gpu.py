"""Model-level parity AT THE SHAPES THE BENCHMARK TIMES (VERDICT r2 "next" item 1).

B = 16 segments x 1024 target tokens: 16 384 decoder rows and 4 096 encoder rows, so every product of the step goes
to the kernels `bench.py` times — the tall-shape ping-pong GEMM (`gemm_nt8`, M >= 4096), the fused wi + gated-GELU
launch and the grouped weight-gradient launch (M >= 1024) — which the B = 2 oracle tests of test_model_gpu.py never
reach.  The test asserts that they dispatched (mrmt3_dispatch_counts) and compares, dropout off:

  * the CPU oracle (oracle/t5_ref.py autograd, fp32) on the same inputs against what the REFERENCE ITSELF produced
    at this shape (tests/golden/bench_shape.npz, written by tests/golden/make_golden.py --bench-shape): loss, 8192
    sampled logits, every gradient tensor's norm and 256 sampled elements — the oracle is pinned at this shape too;
  * the HIP bf16 training path (Engine.forward -> fused lm_head + CE -> Engine.backward, exactly what
    Trainer._step_body enqueues) against the oracle: loss within 1e-3 (north_star), sampled logits no worse than the
    reference's own torch.autocast(bfloat16) run at this shape (recorded in the same fixture), EVERY gradient tensor
    within 1.5 x what autocast loses on that tensor (+2e-3) and with cosine > 0.9995.

Round 5: the fused projection + row launches (gemm_rows.hip) carry every N = 512 data gradient with K <= 1152 and every
d_wo of the step; the test asserts that they dispatched, and runs twice — with the tile height the launch picks at
these 16 384 decoder rows (64) and with the 128-row tiles the 64-segment benchmark batch takes (knob MRMT3_ROWS_BM),
same fixture, same thresholds.
"""
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
FIX = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "bench_shape.npz")
FIX_LONG = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "long_shape.npz")


def _build(variant, dtype, dev):
    from mrmt3.synthetic import T5_SMALL
    if variant == "t5":
        from models.t5 import T5ForConditionalGeneration as M
        m = M(T5_SMALL, compute_dtype=dtype)
    else:
        from models.t5_segmem_v2_with_prev import T5SegMemV2WithPrev as M
        m = M(T5_SMALL, segmem_num_layers=1, segmem_length=64, compute_dtype=dtype)
    return m.load_golden().to(dev).eval()


_ORACLE = {}          # (shape, variant) -> (sd with .grad, loss): the CPU oracle pass is shared by the tile-height cases


def _oracle(variant, fix, mel, lab, prev, shape="bench"):
    from mrmt3.synthetic import T5_SMALL, golden_weights
    from oracle import t5_ref
    if (shape, variant) in _ORACLE:
        return _ORACLE[(shape, variant)]

    # ---- the oracle at this shape, pinned to the reference's recorded outputs ---------------------------------
    torch.set_num_threads(min(16, os.cpu_count() or 8))
    sd = {k: torch.from_numpy(v).requires_grad_(True)
          for k, v in golden_weights(T5_SMALL, 0 if variant == "t5" else 1).items()}
    logits = t5_ref.forward_logits(sd, T5_SMALL, mel, lab, variant=variant, targets_prev=prev.clone())
    ref_loss = t5_ref.ce_loss(logits, lab)
    ref_loss.backward()
    idx = torch.from_numpy(fix[f"{variant}.logit_idx"])
    ref_logit = fix[f"{variant}.logit_val"]
    np.testing.assert_allclose(logits.detach().reshape(-1)[idx].numpy(), ref_logit, atol=5e-5, rtol=0)
    assert abs(ref_loss.item() - float(fix[f"{variant}.fp32.loss"])) < 2e-5
    names = fix[f"{variant}.grad_names"].tolist()
    for n, norm, si, sv in zip(names, fix[f"{variant}.grad_norm"], fix[f"{variant}.grad_sample_idx"],
                               fix[f"{variant}.grad_sample_val"]):
        g = sd[n].grad
        assert g is not None, n
        assert abs(g.double().norm().item() - norm) <= 1e-4 * norm + 1e-9, n
        np.testing.assert_allclose(g.reshape(-1)[torch.from_numpy(si)].numpy(), sv, rtol=0,
                                   atol=2e-4 * float(np.abs(sv).max()) + 1e-9, err_msg=n)
    _ORACLE[(shape, variant)] = (sd, ref_loss.detach())
    return _ORACLE[(shape, variant)]


@pytest.mark.parametrize("tile", ["auto", 128], ids=["tile_auto", "tile128"])
@pytest.mark.parametrize("variant", ["t5", "segmem_v2_with_prev"])
def test_bench_shape_loss_logits_and_every_gradient_vs_oracle(variant, tile, knobs):
    from mrmt3 import lib
    from mrmt3.synthetic import bench_shape_inputs
    assert torch.cuda.is_available()
    dev = torch.device("cuda:0")
    fix = np.load(FIX)
    mel, lab, prev = (torch.from_numpy(a) for a in bench_shape_inputs())
    B, Ld = lab.shape
    assert B * Ld >= 16384 and B * mel.shape[1] >= 4096
    sd, ref_loss = _oracle(variant, fix, mel, lab, prev)
    idx = torch.from_numpy(fix[f"{variant}.logit_idx"])
    ref_logit = fix[f"{variant}.logit_val"]
    names = fix[f"{variant}.grad_names"].tolist()
    if tile == "auto":
        knobs.unset("MRMT3_ROWS_BM")
        assert lib.load().mrmt3_gemm_nt_normbwd_partial_rows(B * Ld) == B * Ld // 64      # 64-row tiles at 16 384 rows
    else:
        knobs.set("MRMT3_ROWS_BM", tile)                  # the tiles the 64-segment benchmark batch takes by itself
        assert lib.load().mrmt3_gemm_nt_normbwd_partial_rows(B * Ld) == B * Ld // 128

    counts, eng = _hip_path_vs_oracle(variant, fix, mel, lab, prev, sd, ref_loss, "bench shape")
    # the kernels of the benchmark step really ran: ping-pong NT, fused wi + GEGLU, grouped weight gradients
    # (at 16 segments the dispatch rule gives the ping-pong kernel 57 of the step's NT products — both its 256-row and
    # its 128-row form — and the others to the tile kernel; at 64 segments it is 113 of 161, same kernels)
    assert counts["gemm_nt8"] >= 40 and counts["gemm_nt_geglu"] >= 16, counts
    assert counts["tn_group"] >= 1 and eng.tn_group.last_info.n_items > 0, counts
    assert counts["attn_fwd"] >= 24 and counts["attn_bwd"] + counts["attn_bwd_onepass"] >= 24, counts
    # the one-pass attention backward took the encoder's 8 self-attention sites (256 keys) AND the decoder's 8 cross-attention
    # sites — 256 keys for MT3Net, 320 (256 frames + 64 memory slots) for MR-MT3's own model since round 6
    assert counts["attn_bwd_onepass"] >= 16, counts
    # ... and the fused backward row kernels (MRMT3_FUSE_ROWS default 6): d_qkv / d_cq -> norm backward (8 encoder + 16
    # decoder sites), d_wo -> gated-GELU backward (16 sites).  A silent fall-back to the two-kernel form fails here.
    assert eng.fuse_rows & 6 == 6, eng.fuse_rows
    assert counts["gemm_nt_normbwd"] >= 16 and counts["gemm_nt_geglubwd"] >= 16, counts


def _hip_path_vs_oracle(variant, fix, mel, lab, prev, sd, ref_loss, what):
    """The HIP bf16 training path (forward -> fused lm_head + CE -> backward) against the oracle's loss, the reference's
    recorded logits and every gradient tensor of the oracle; returns (dispatch counts of that pass, engine)."""
    from mrmt3 import lib
    dev = torch.device("cuda:0")
    idx = torch.from_numpy(fix[f"{variant}.logit_idx"])
    ref_logit = fix[f"{variant}.logit_val"]
    names = fix[f"{variant}.grad_names"].tolist()
    m = _build(variant, torch.bfloat16, dev)
    eng, flat = m.engine, m.flat
    flat.ensure_grads()
    d_mel, d_lab = mel.to(dev), lab.to(dev)
    d_prev = prev.clone().to(dev) if variant != "t5" else None
    with torch.no_grad():
        out = m(inputs=d_mel, labels=d_lab, targets_prev=None if d_prev is None else d_prev.clone())
    got = out.reshape(-1)[idx.to(dev)].float().cpu().numpy()
    lib.dispatch_counts(reset=True)
    dec, tape = eng.forward(d_mel, d_lab, None if d_prev is None else d_prev.clone(), training=False, need_grad=True,
                            want_logits=False)
    loss, dl = lib.lmhead_cross_entropy(dec, eng.W("lm_head"), d_lab.reshape(-1), want_grad=True, grad_dtype=torch.bfloat16)
    flat.G.zero_()
    eng.backward(tape, dl)
    torch.cuda.synchronize()
    counts = lib.dispatch_counts()
    print(variant, what, "dispatch:", counts, "grouped weight-gradient items:", eng.tn_group.last_info.n_items)

    d_loss = abs(loss.item() - ref_loss.item())
    rel = np.linalg.norm(got - ref_logit) / np.linalg.norm(ref_logit)
    max_d = float(np.abs(got - ref_logit).max())
    print(variant, what + ": loss %.6f oracle %.6f (|d| %.2e); logits rel-L2 %.3e max|d| %.3e (autocast: %.3e / %.3e)"
          % (loss.item(), ref_loss.item(), d_loss, rel, max_d, float(fix[f"{variant}.autocast_rel_l2"]),
             float(fix[f"{variant}.autocast_max_abs"])))
    assert d_loss < 1e-3                                            # north_star tolerance on the loss
    assert rel <= float(fix[f"{variant}.autocast_rel_l2"])
    assert max_d <= float(fix[f"{variant}.autocast_max_abs"]) and max_d < 5e-2
    assert np.abs(got - ref_logit).mean() <= np.abs(fix[f"{variant}.autocast_logit_val"] - ref_logit).mean()

    auto_rel = dict(zip(names, fix[f"{variant}.grad_rel_l2"].tolist()))
    worst_rel, worst_cos = (0.0, ""), (1.0, "")
    ratios = []
    for k, ref in sd.items():
        g = flat.grad(k).float().cpu()
        r = ref.grad
        if r is None or r.norm() == 0:
            assert g.norm() < 1e-6, k
            continue
        cos = torch.nn.functional.cosine_similarity(g.flatten(), r.flatten(), dim=0).item()
        rl = ((g - r).norm() / r.norm()).item()
        worst_rel = max(worst_rel, (rl, k))
        worst_cos = min(worst_cos, (cos, k))
        ratios.append(rl / max(auto_rel[k], 1e-9))
        assert cos > 0.9995 and rl < 4e-2, (k, cos, rl)
        assert rl <= 1.5 * auto_rel[k] + 2e-3, (k, rl, auto_rel[k])
    print(variant, what + " gradients: worst rel-L2 %.3e (%s), worst cosine %.6f (%s), median ratio to the "
          "reference's autocast deviation %.2f, max %.2f" % (worst_rel + worst_cos + (float(np.median(ratios)), max(ratios))))
    return counts, eng


def test_long_context_shape_loss_logits_and_every_gradient_vs_oracle(knobs):
    """BASELINE configs[4] (config_slakh_segmem_finetune.yaml, models/t5_segmem_v2_with_prev.py:60-153) at the shape a
    segment of the 12-segment step has: 2048 mel frames + 64 memory slots, 1024-token targets, B = 2 (VERDICT r4 item 8 —
    until now this config was held to the oracle at B = 1 x 128 tokens only).  Same three legs as the bench shape: the
    oracle pinned to what the reference recorded at this shape (tests/golden/long_shape.npz, make_golden.py
    --long-shape), fp32 logits of the HIP engine within 2e-4 of the reference's, the bf16 training path against the oracle
    under the bench-shape rule — loss within 1e-3, every gradient tensor within 1.5 x the reference's own autocast
    deviation — and the dispatch this shape takes: two-pass attention backward at 2048 / 2112 keys, the fused row kernels on
    the encoder's 4096 rows, the grouped weight gradients."""
    from mrmt3 import lib
    from mrmt3.synthetic import long_shape_inputs
    variant = "segmem_v2_with_prev"
    fix = np.load(FIX_LONG)
    mel, lab, prev = (torch.from_numpy(a) for a in long_shape_inputs())
    assert tuple(mel.shape) == (2, 2048, 512) and tuple(lab.shape) == (2, 1024)
    knobs.unset("MRMT3_ROWS_BM")
    sd, ref_loss = _oracle(variant, fix, mel, lab, prev, shape="long")
    # fp32 engine: logits against the reference's own
    dev = torch.device("cuda:0")
    m32 = _build(variant, torch.float32, dev)
    with torch.no_grad():
        got32 = m32(inputs=mel.to(dev), labels=lab.to(dev), targets_prev=prev.clone().to(dev))
    idx = torch.from_numpy(fix[f"{variant}.logit_idx"])
    np.testing.assert_allclose(got32.reshape(-1)[idx.to(dev)].cpu().numpy(), fix[f"{variant}.logit_val"], atol=2e-4, rtol=0)
    del m32, got32
    counts, eng = _hip_path_vs_oracle(variant, fix, mel, lab, prev, sd, ref_loss, "long context")
    # 8 encoder self-attention sites over 2048 keys, 8 decoder cross-attention sites over 2048 + 64 keys, 8 causal sites,
    # the memory encoder's one: all on the two-pass backward (the one-pass kernel owns exactly 256 keys)
    assert counts["attn_bwd_onepass"] == 0 and counts["attn_bwd"] == 25 and counts["attn_fwd"] == 25, counts
    # fused row launches: the norm backward behind 8 + 8 + 8 attention-input projections; the gated-GELU backward of the 8 + 8
    # feed-forward sublayers and of the memory encoder's one (its shortcut goes through the stacks' own feed-forward piece)
    assert counts["gemm_nt_normbwd"] == 24 and counts["gemm_nt_geglubwd"] == 17, counts
    assert counts["tn_group"] >= 1 and eng.tn_group.last_info.n_items > 0, counts
    assert counts["gemm_nt8"] >= 8 and counts["gemm_nt_geglu"] >= 8, counts
