"""Forward / backward of the MR-MT3 encoder–decoder as an explicit tape over the C-ABI kernels.

This is the host-side wiring that the reference gets from HF `T5Block` + autograd
(`models/t5.py:99-180,478-702`, `models/t5_segmem*.py`): every sublayer is a short, fixed sequence
of kernel launches, and the backward is written out by hand in reverse order so that
  * activations are kept in the dtype the next kernel consumes (bf16 GEMM operands, fp32 residual
    stream and statistics),
  * weight gradients accumulate straight into the flat gradient buffer (`FlatParams.G`),
  * a per-layer callback can start the RCCL all-reduce of finished gradient slices while the rest of
    the backward still runs (`on_layer_done`).

Residual-stream convention: a sublayer returns its un-dropped output `y`; the NEXT fused kernel
(`add_rmsnorm`) applies dropout to `y`, adds it to the residual `x` and normalises — one pass over
the row for three reference ops (`hidden + dropout(sublayer)`, then `T5LayerNorm`).
"""
from __future__ import annotations

import os

import torch

from . import lib
from .params import FlatParams
from .synthetic import sinusoid_table


class Tape:
    """Saved tensors of one forward pass (dropped as soon as backward has consumed them)."""

    def __init__(self):
        self.ops = []

    def push(self, **kw):
        self.ops.append(kw)

    def pop(self):
        return self.ops.pop()


class Engine:
    def __init__(self, cfg: dict, flat: FlatParams, variant: str = "t5", segmem_length: int = 64,
                 segmem_num_layers: int = 0, compute_dtype=torch.bfloat16, max_pos: int = 5000):
        self.cfg, self.flat, self.variant = cfg, flat, variant
        self.segmem_length, self.segmem_num_layers = segmem_length, segmem_num_layers
        self.dt = compute_dtype
        self.d, self.H, self.dff, self.V = cfg["d_model"], cfg["num_heads"], cfg["d_ff"], cfg["vocab_size"]
        self.inner = cfg["d_kv"] * self.H
        assert cfg["d_kv"] == 64, "kernels are specialised for d_kv = 64"
        self.eps = cfg["layer_norm_epsilon"]
        self.max_pos = max_pos
        self._pos = None
        self._stream_ctr = 0
        self.seed = 365
        # optional DEVICE step counter (int32[1]) salting every dropout mask in-kernel.  The trainer sets it (and
        # restarts the site counter every step) so that a hipGraph replay, whose by-value arguments are frozen,
        # still draws fresh masks each step — and draws the SAME masks as the eager path would.
        self.step_dev = None
        # dtype of sublayer outputs / dgrad outputs entering the fp32 residual add: the compute dtype
        # (bf16 halves that stream's HBM traffic; the residual itself and all statistics stay fp32)
        self.y_dtype = compute_dtype
        self.overlap_wgrad = False      # nothing in the package reads it: bench.py's roofline repeat still sets and restores it
        # residual-stream GRADIENT of the bf16 path: bf16 between the norm-backward sites of a stack (f32 at both
        # ends) halves the largest streams of the backward row kernels; the forward residual stays f32
        self.res_grad_dtype = (torch.bfloat16 if compute_dtype == torch.bfloat16 and
                               os.environ.get("MRMT3_RES_GRAD", "bf16") == "bf16" else torch.float32)
        # lm_head (and the final decoder norm feeding it) in "bf16" (MFMA bf16 operands) or "f32" (exact-f32 MFMA on
        # the master weights; inference / parity only)
        self.head_dtype = "bf16"
        self._wt32 = {}
        # bf16(O - bf16(O)) of an attention site is kept for the backward's delta where the value rows share a large common
        # component — cross-attention over near-identical encoder frames.  "all": every site; "cross": the
        # self-attention sites skip the extra 50 MB write + read per site
        self.lo_sites = os.environ.get("MRMT3_ATTN_LO", "all")
        self.norm_dw = lib.NormDwBatch() if os.environ.get("MRMT3_NORM_DW_BATCH", "1") != "0" else None
        # weight-gradient GEMMs are off the critical dgrad chain (their outputs are only needed by the optimizer / the
        # gradient exchange): every shape the grouped kernel takes is deferred to the next join_wgrad() — one launch for
        # the weight gradients of a whole gradient bucket (lib.TnGroup); the others run at once, one by one.
        # MRMT3_TN_GROUP=0 (A/B switch): every gradient through mrmt3_gemm_tn
        self.tn_group = lib.TnGroup() if os.environ.get("MRMT3_TN_GROUP", "1") != "0" else None
        # projection + row kernel in one launch (csrc/gemm_rows.hip; bf16 engine only).  MRMT3_FUSE_ROWS bits: 1 the o / co /
        # wo projection with the residual add + norm behind it, 2 the 512-column data gradients with the norm backward,
        # 4 the wo data gradient with the gated-GELU backward.  Same results as the two-kernel form (tests/test_gemm_rows_gpu.py).
        # Default 6: same-box step A/B at 64 segments (profiles/r04_fuse_rows_step_ab.txt) 24.68 ms unfused, 24.25-24.29 with
        # bit 4, 24.18 with bits 2 + 4 (K <= 1152), 24.45-24.47 when bit 1 is added — the forward fusion costs what it saves
        # (its K loop is bound by the CU's L2 -> LDS rate and does not overlap its row phase)
        self.fuse_rows = int(os.environ.get("MRMT3_FUSE_ROWS", "6")) if compute_dtype == torch.bfloat16 else 0
        # the norm-backward fusion up to this K (d_cq 384, d_qkv 1152; d_wi, K = 2048, stays on the ping-pong product +
        # the stand-alone row kernel: 224 against 205 us cold, profiles/r04_gemm_rows_ab.txt)
        self.fuse_normbwd_max_k = int(os.environ.get("MRMT3_FUSE_NORMBWD_MAXK", "1152"))

    # ---- helpers ---------------------------------------------------------------------------------------
    def pos(self, device):
        if self._pos is None or self._pos.device != device:
            self._pos = sinusoid_table(self.max_pos, self.d).to(device).contiguous()
        return self._pos

    def _sid(self):
        self._stream_ctr += 1
        return self._stream_ctr

    def W(self, name):
        return self.flat.W(name, self.dt)

    def ln(self, key):
        return self.flat.master(key)

    def WT(self, name):
        """Transposed weight [in, out] for the data-gradient products: the pre-transposed bf16 copy, or — fp32 path — an
        f32 transpose of the master made on demand (kept for one forward/backward pass: prepare() drops them, the AdamW
        kernel rewrites the master without touching torch's version counters)."""
        if self.dt == torch.bfloat16:
            return self.flat.WT(name)
        t = self._wt32.get(name)
        if t is None:
            w = self.flat.W(name, torch.float32)
            t = torch.empty(w.shape[1], w.shape[0], device=w.device, dtype=torch.float32)
            lib.transpose(w, t)
            self._wt32[name] = t
        return t

    def wgrad(self, a, b, out):
        """out += a^T @ b, complete after the next join_wgrad() (inputs were produced on the current stream).
        Shapes the grouped kernel takes are only recorded here (operands kept alive) and launched with every other
        gradient that is due; everything else runs now, on the current stream."""
        if self.flat.is_frozen(out):                      # a frozen weight has no gradient: nothing is queued or launched
            return None
        if a.dtype == torch.float32:                      # fp32 training / parity path: exact-f32 product, in place, now
            return lib.gemm_tn_f32(a, b, out, accumulate=True)
        if self.tn_group is not None and self.tn_group.ok(a, b, out):
            return self.tn_group.add(a, b, out, accumulate=True)
        return lib.gemm_tn(a, b, out, accumulate=True)

    def ndw(self, key):
        """The gradient slot of a norm weight, or None when it is frozen (no partial rows, no deferred reduction)."""
        return None if key in self.flat.frozen else self.flat.grad(key)

    def _embed_bwd(self, *a, **kw):
        """lib.embed_bwd into the decoder's embedding table, unless the table is frozen."""
        if "decoder_embed_tokens.weight" not in self.flat.frozen:
            lib.embed_bwd(*a, **kw)

    def encoder_frozen(self) -> bool:
        """Every parameter of the encoder stack and its input projection is frozen: backward stops above it."""
        return self.flat.all_frozen("encoder.") and "proj.weight" in self.flat.frozen

    def segmem_frozen(self) -> bool:
        """The memory encoder, its projection and the table its input gradient would land in are all frozen."""
        f = self.flat
        return (f.all_frozen("segmem_encoder.") and "segmem_proj.weight" in f.frozen and
                "decoder_embed_tokens.weight" in f.frozen)

    def _norm_bwd(self, *a, **kw):
        """lib.add_rmsnorm_bwd with the norm-weight gradient deferred to one batched reduction (flush_norm_dw).
        fp32 path: the kernel's second output (the masked gradient of the sublayer output below) is bf16-only, so it is
        formed from dx1 here — dx1 itself without dropout, one mask-and-copy launch with it."""
        want_dy, bf16 = kw.pop("want_dy", True), self.dt == torch.bfloat16
        dx1, dy = lib.add_rmsnorm_bwd(*a, defer=self.norm_dw, want_dy=want_dy and bf16, **kw)
        if bf16 or not want_dy:
            return dx1, dy
        p = kw.get("p", 0.0)
        if p <= 0.0:
            return dx1, dx1
        return dx1, lib.dropmask_cast(dx1, p=p, seed=kw.get("seed", 0), stream_id=kw.get("stream_y", 0),
                                      step=kw.get("step"), out_dtype=torch.float32)

    def _proj_addnorm(self, x, pend, w_norm, xn_dtype=None, **kw):
        """add_rmsnorm_fwd(x, y, ...) where y is the pending projection `pend` = (a, W) of the sublayer above (None: the
        stack's first norm, nothing to add): one fused launch when the shape allows, else the product then the row kernel."""
        xn_dtype = xn_dtype or self.dt
        y = None
        if pend is not None:
            a, w = pend
            if ((self.fuse_rows & 1) and self.y_dtype == torch.bfloat16 and xn_dtype == torch.bfloat16 and x.shape[1] == 512 and
                    lib.gemm_rows_ok(a, w)):
                return lib.gemm_nt_addnorm(a, w, x, w_norm, self.eps, **kw)
            y = lib.gemm_nt(a, w, out_dtype=self.y_dtype)
        return lib.add_rmsnorm_fwd(x, y, w_norm, self.eps, xn_dtype, **kw)

    def _proj_norm_bwd(self, a, wt, dres, x1, rstd, w_norm, dw, **kw):
        """_norm_bwd(gemm_nt(a, wt), dres, ...): the data gradient of a sublayer's input projection and the backward of the
        norm in front of it, one fused launch when the shape allows."""
        # (only with the batched norm-weight reduce: without it the fused call would have to build its one-site reduce table
        # by a host-to-device copy, which the capture of the step does not allow — ADVICE r4)
        if ((self.fuse_rows & 2) and self.norm_dw is not None and self.y_dtype == torch.bfloat16 and dres is not None and
                x1.shape[1] == 512 and a.shape[1] <= self.fuse_normbwd_max_k and lib.gemm_rows_ok(a, wt)):
            return lib.gemm_nt_normbwd(a, wt, dres, x1, rstd, w_norm, dw, defer=self.norm_dw, **kw)
        dxn = lib.gemm_nt(a, wt, out_dtype=self.y_dtype)
        return self._norm_bwd(dxn, dres, x1, rstd, w_norm, dw, **kw)

    def _proj_geglu_bwd(self, dy, wt, h, **kw):
        """geglu_bwd(h, gemm_nt(dy, wt)): the wo data gradient and the gated-GELU backward."""
        if (self.fuse_rows & 4) and h.dtype == torch.bfloat16 and lib.gemm_rows_ok(dy, wt, N=wt.shape[0]):
            return lib.gemm_nt_geglubwd(dy, wt, h, **kw)
        dg = lib.gemm_nt(dy, wt)
        return lib.geglu_bwd(h, dg, **kw)

    # ---- sublayer pieces: each stated once; the stacks and the one-layer memory-encoder shortcut are made of them ----------
    # Dropout site ids always come from the caller: the stack loop draws them (`_sid()`) in a fixed order, the shortcut (which
    # never drops) passes 0 and draws none — the masks of every later site depend on how many were drawn.
    def _rng(self, p):
        """The dropout arguments every site of a step shares (its own stream id is added by the piece)."""
        return dict(p=p, seed=self.seed, step=self.step_dev)

    def _addnorm(self, x, pend, key, p, s_in, keep, **kw):
        """The add + norm in front of a sublayer: `pend` (the projection the sublayer above left pending, dropped at site
        s_in) is added to the residual stream x — in place when nothing is kept for a backward.  Returns (x1, xn, rstd)."""
        return self._proj_addnorm(x, pend, self.ln(key), stream_y=s_in, x1=None if keep else x, **self._rng(p), **kw)

    def _addnorm_bwd(self, t, a, wname, dx, p, **kw):
        """Backward of the `_addnorm` of record t through the projection `wname` that read its output (a: the gradient of that
        projection's output); dx: the residual gradient, updated in place unless `dx1=` says otherwise.  Returns (dx, dy)."""
        kw.setdefault("dx1", dx)
        return self._proj_norm_bwd(a, self.WT(wname), dx, t["x1"], t["rstd"], self.ln(t["ln"]), self.ndw(t["ln"]),
                                   stream_y=t["s_in"], **self._rng(p), **kw)

    def _attn_fwd(self, q, k, v, B, Lq, Lk, causal, pack, sid, p, keep, want_lo):
        """One attention site: (o, lse, o_lo).  Lk = 0: self-attention, the keys are the query rows.  pack (a lib.PackPlan): the
        query rows are packed end to end (the keys too when Lk = 0, else dense [B*Lk]) — the varlen kernels."""
        kw = dict(stream_id=sid, want_lse=keep, want_lo=keep and want_lo, **self._rng(p))
        if pack is not None:
            return lib.attn_fwd_varlen(q, k, v, pack, self.H, Lk, causal, **kw)
        return lib.attn_fwd(q, k, v, B, self.H, Lq, Lk or Lq, causal, **kw)

    def _attn_bwd(self, t, q, k, v, do, dq, dk, dv, B, Lq, Lk, causal, pack, p):
        """Backward of the `_attn_fwd` whose outputs record t holds, into the caller's dq / dk / dv."""
        kw = dict(stream_id=t["s_att"], o_lo=t["o_lo"], **self._rng(p))
        if pack is not None:
            return lib.attn_bwd_varlen(q, k, v, t["o"], do, t["lse"], dq, dk, dv, pack, self.H, Lk, causal, **kw)
        return lib.attn_bwd(q, k, v, t["o"], do, t["lse"], dq, dk, dv, B, self.H, Lq, Lk or Lq, causal, **kw)

    def _oproj_bwd(self, dy, o, wname):
        """Backward of an attention output projection that was left pending into the next add + norm (dy: that norm's masked
        gradient): the weight gradient, and the gradient of the attention output."""
        self.wgrad(dy, o, self.flat.GW(wname))
        return lib.gemm_nt(dy, self.WT(wname))

    def _ff_fwd(self, x, pend, pre, i, key, p, s_in, s_g, keep):
        """Gated-GELU feed-forward sublayer of layer i of stack `pre`: add + norm, wi and the gate (one launch in bf16: K2 + K7,
        same bits as the two kernels); wo is left pending.  Returns (x1, the tape record, the pending (g, wo))."""
        x, xn, rstd = self._addnorm(x, pend, key, p, s_in, keep)
        wi = self.W(f"{pre}.{i}.wi")
        if xn.dtype == torch.bfloat16:
            h, g = lib.gemm_nt_geglu(xn, wi, stream_id=s_g, **self._rng(p))
        else:
            h = lib.gemm_nt(xn, wi)
            g = lib.geglu_fwd(h, stream_id=s_g, **self._rng(p))
        return x, dict(kind="ff", i=i, ln=key, x1=x, xn=xn, rstd=rstd, h=h, g=g, s_in=s_in, s_g=s_g), (g, self.W(f"{pre}.{i}.wo"))

    def _ff_bwd(self, t, pre, dx, dy, p):
        """Backward of `_ff_fwd` (dy: the masked gradient of the pending wo projection): (dx, dy) below the sublayer."""
        wi, wo = f"{pre}.{t['i']}.wi", f"{pre}.{t['i']}.wo"
        self.wgrad(dy, t["g"], self.flat.GW(wo))
        dh = self._proj_geglu_bwd(dy, self.WT(wo), t["h"], stream_id=t["s_g"], **self._rng(p))
        self.wgrad(dh, t["xn"], self.flat.GW(wi))
        return self._addnorm_bwd(t, dh, wi, dx, p)

    def _final_fwd(self, x, pend, pre, p, s_in, s_out, keep, xn_dtype=None):
        """The closing norm of stack `pre` (its output dropped at site s_out): (out, the tape record)."""
        key = f"{pre}.final_layer_norm.weight"
        x, out, rstd = self._addnorm(x, pend, key, p, s_in, keep, xn_dtype=xn_dtype, stream_out=s_out, out_drop=True)
        return out, dict(kind="final", ln=key, x1=x, rstd=rstd, s_in=s_in, s_out=s_out)

    def _final_bwd(self, t, d_out, p, want_dy, dx_dtype):
        """Backward of `_final_fwd`: (dx in `dx_dtype`, dy or None)."""
        return self._norm_bwd(d_out, None, t["x1"], t["rstd"], self.ln(t["ln"]), self.ndw(t["ln"]), want_dy=want_dy,
                              stream_y=t["s_in"], stream_out=t["s_out"], out_drop=True, dx1_dtype=dx_dtype, **self._rng(p))

    def _input_fwd(self, a, wname, L, p, s_emb):
        """Input prologue of the encoder and the memory encoder: projection `wname` of a, + sinusoid, dropout at site s_emb."""
        src = lib.gemm_nt(a, self.W(wname), out_dtype=self.y_dtype)
        return lib.addpos_fwd(src, self.pos(a.device), L, stream_id=s_emb, **self._rng(p))

    def _input_bwd(self, dx, a, wname, p, s_emb):
        """Backward of `_input_fwd`: the projection's weight gradient; returns the masked gradient of its output."""
        dsrc = lib.dropmask_cast(dx, stream_id=s_emb, out_dtype=self.dt, **self._rng(p))
        self.wgrad(dsrc, a, self.flat.GW(wname))
        return dsrc

    def flush_norm_dw(self):
        if self.norm_dw is not None:
            self.norm_dw.flush()

    def join_wgrad(self):
        """Launch every weight gradient recorded so far (and sum the queued norm-weight gradients: both are what a
        gradient bucket needs before it is sent)."""
        self.flush_norm_dw()
        if self.tn_group is not None:
            self.tn_group.flush()        # the deferred weight gradients: their operands were produced on this stream

    def reset_deferred(self):
        """Forget every deferred launch: the weight gradients recorded for the grouped launch and the queued norm-weight
        reductions.  After an aborted hipGraph capture (or an exception in the middle of a backward pass) these still
        name tensors of work that never ran — a later flush would accumulate uninitialised memory into the gradients
        (ADVICE r2)."""
        if self.tn_group is not None:
            self.tn_group.clear()
        if self.norm_dw is not None:
            self.norm_dw.clear()

    def begin_step(self):
        """Start of a training step: nothing deferred by an aborted capture / a failed step leaks into this one, and the
        dropout site ids restart (they are per-step: step_dev salts them)."""
        self.reset_deferred()
        self._stream_ctr = 0

    def prepare(self, training: bool):
        if self.dt == torch.bfloat16:
            self.flat.refresh_shadows(need_transposed=training)
        else:
            self._wt32 = {}

    # ---- one T5Stack (models/t5.py:507-702) ----------------------------------------------------------
    def stack_fwd(self, prefix, x, B, L, n_layers, is_decoder, enc=None, Le=0, p=0.0, tape=None, out_dtype=None, pack=None):
        """x: [B*L, d] fp32 (embeddings + sinusoid, dropout already applied).
        enc: [B*Le, d] compute-dtype encoder states for cross-attention.  Returns the final-normed
        (and dropped) states [B*L, d] in the compute dtype.  pack (a lib.PackPlan): x is [Tcap, d], rows packed end to end —
        every row-wise kernel runs on the Tcap rows, the attention sites on the varlen kernels (encoder states stay dense)."""
        inner = self.inner
        keep = tape is not None
        push = tape.push if keep else (lambda **kw: None)
        cross = is_decoder and enc is not None
        pend = None          # the projection of the sublayer above, not yet added to the residual stream: (operand, weight)
        sy = 0               # ... and the dropout site of its output
        # cross-attention K | V of every layer in one projection of the encoder output: [B*Le, n_layers * 768]
        kv_all = lib.gemm_nt(enc, self.W(f"{prefix}.ckv_all")) if is_decoder and n_layers > 0 else None
        for i in range(n_layers):
            b = f"{prefix}.block.{i}.layer"
            # -- self attention
            ln = f"{b}.0.layer_norm.weight"
            x, xn, rstd = self._addnorm(x, pend, ln, p, sy, keep)
            qkv = lib.gemm_nt(xn, self.W(f"{prefix}.{i}.qkv"))
            s_att = self._sid()
            o, lse, o_lo = self._attn_fwd(qkv[:, :inner], qkv[:, inner:2 * inner], qkv[:, 2 * inner:], B, L, 0, is_decoder,
                                          pack, s_att, p, keep, self.lo_sites == "all")
            push(kind="self", i=i, ln=ln, x1=x, xn=xn, rstd=rstd, qkv=qkv, o=o, o_lo=o_lo, lse=lse, s_in=sy, s_att=s_att)
            pend, sy = (o, self.W(f"{prefix}.{i}.o")), self._sid()
            if cross:
                ln = f"{b}.1.layer_norm.weight"
                x, xn, rstd = self._addnorm(x, pend, ln, p, sy, keep)
                q = lib.gemm_nt(xn, self.W(f"{prefix}.{i}.cq"))
                kv = kv_all[:, i * 2 * inner:(i + 1) * 2 * inner]        # this layer's K | V columns (row stride n_layers * 768)
                s_att = self._sid()
                o, lse, o_lo = self._attn_fwd(q, kv[:, :inner], kv[:, inner:], B, L, Le, False, pack, s_att, p, keep, True)
                push(kind="cross", i=i, ln=ln, x1=x, xn=xn, rstd=rstd, q=q, kv=kv, o=o, o_lo=o_lo, lse=lse, s_in=sy, s_att=s_att)
                pend, sy = (o, self.W(f"{prefix}.{i}.co")), self._sid()
            # -- gated-GELU feed forward
            ln = f"{b}.{2 if cross else 1}.layer_norm.weight"
            x, rec, pend = self._ff_fwd(x, pend, prefix, i, ln, p, sy, self._sid(), keep)
            push(**rec)
            sy = self._sid()
        out, rec = self._final_fwd(x, pend, prefix, p, sy, self._sid(), keep, xn_dtype=out_dtype)
        push(prefix=prefix, n_layers=n_layers, is_decoder=is_decoder, cross=cross, B=B, L=L, Le=Le, enc=enc, p=p, pack=pack,
             **rec)
        return out

    def stack_bwd(self, tape, d_out, d_enc=None, on_layer_done=None):
        """d_out: fp32 [B*L, d] gradient w.r.t. the stack output.  Accumulates weight grads into
        flat.G, adds cross-attention gradients into d_enc (fp32 [B*Le, d]) and returns the gradient
        w.r.t. the stack input x."""
        f = self.flat
        fin = tape.pop()
        assert fin["kind"] == "final"
        prefix, n_layers, is_dec = fin["prefix"], fin["n_layers"], fin["is_decoder"]
        B, L, Le, enc, p, pack = fin["B"], fin["L"], fin["Le"], fin["enc"], fin["p"], fin["pack"]
        inner = self.inner
        has_y = n_layers > 0
        dx, dy = self._final_bwd(fin, d_out, p, has_y, self.res_grad_dtype if has_y else torch.float32)
        # gradient of the cross-attention K | V of every layer, side by side like the forward's kv_all: the gradient of
        # the encoder output is then ONE product with K = n_layers * 768 after the loop instead of n_layers f32 accumulations
        dkv_all = (torch.empty(B * Le, n_layers * 2 * inner, device=d_out.device, dtype=self.dt)
                   if is_dec and n_layers > 0 else None)
        for i in reversed(range(n_layers)):
            t = tape.pop()
            assert t["kind"] == "ff" and t["i"] == i
            dx, dy = self._ff_bwd(t, prefix, dx, dy, p)
            if fin["cross"]:
                t = tape.pop()
                assert t["kind"] == "cross"
                do = self._oproj_bwd(dy, t["o"], f"{prefix}.{i}.co")
                dq = torch.empty_like(t["q"])
                dkv = dkv_all[:, i * 2 * inner:(i + 1) * 2 * inner]
                kv = t["kv"]
                self._attn_bwd(t, t["q"], kv[:, :inner], kv[:, inner:], do, dq, dkv[:, :inner], dkv[:, inner:], B, L, Le, False,
                               pack, p)
                self.wgrad(dq, t["xn"], f.GW(f"{prefix}.{i}.cq"))
                self.wgrad(dkv, enc, f.GW(f"{prefix}.{i}.ckv"))
                dx, dy = self._addnorm_bwd(t, dq, f"{prefix}.{i}.cq", dx, p)
            t = tape.pop()
            assert t["kind"] == "self" and t["i"] == i
            do = self._oproj_bwd(dy, t["o"], f"{prefix}.{i}.o")
            qkv = t["qkv"]
            dqkv = torch.empty_like(qkv)
            self._attn_bwd(t, qkv[:, :inner], qkv[:, inner:2 * inner], qkv[:, 2 * inner:], do, dqkv[:, :inner],
                           dqkv[:, inner:2 * inner], dqkv[:, 2 * inner:], B, L, 0, is_dec, pack, p)
            self.wgrad(dqkv, t["xn"], f.GW(f"{prefix}.{i}.qkv"))
            last = i == 0                                     # the stack's input gradient leaves in f32
            dx, dy = self._addnorm_bwd(t, dqkv, f"{prefix}.{i}.qkv", dx, p, want_dy=not last,
                                       dx1=None if (last and dx.dtype != torch.float32) else dx)
            if on_layer_done is not None:
                on_layer_done(prefix, i)
        if dkv_all is not None and d_enc is not None:      # (None: everything below the cross k|v projections is frozen)
            lib.gemm_nt(dkv_all, self.WT(f"{prefix}.ckv_all"), out=d_enc)          # d_enc is written here and nowhere else
        return dx

    # ---- model pieces ------------------------------------------------------------------------------------
    def _act(self, t):
        """torch tensor -> contiguous compute-dtype 2-D operand."""
        t = t.contiguous()
        if t.dtype != self.dt:
            out = torch.empty(t.shape, device=t.device, dtype=self.dt)
            lib.cast(t.view(-1), out.view(-1))
            t = out
        return t

    def encode(self, mel, p=0.0, tape=None):
        """proj -> + sinusoid -> dropout -> encoder stack (models/t5.py:122-136).  mel [B,Le,d]."""
        B, Le, d = mel.shape
        mel2 = self._act(mel.reshape(B * Le, d))
        s_emb = self._sid()
        x = self._input_fwd(mel2, "proj", Le, p, s_emb)
        if tape is not None:
            tape.push(kind="enc_in", mel=mel2, s_emb=s_emb, p=p)
        return self.stack_fwd("encoder", x, B, Le, self.cfg["num_layers"], False, p=p, tape=tape)

    def encode_bwd(self, tape, d_enc_out, on_layer_done=None):
        dx = self.stack_bwd(tape, d_enc_out, on_layer_done=on_layer_done)
        t = tape.pop()
        assert t["kind"] == "enc_in"
        self._input_bwd(dx, t["mel"], "proj", t["p"], t["s_emb"])

    def segmem(self, ids, B, L, tape=None):
        """embed -> segmem_proj -> 1-layer bidirectional encoder, dropout 0
        (models/t5_segmem.py:56-66, models/t5_segmem_v2_with_prev.py:121-123; the positional call
        `self.segmem_encoder(segmem_embeds)` routes the embeddings through `embed_tokens` =
        segmem_proj).  Returns the first `segmem_length` positions [B, Ls, d] in the compute dtype.

        Only those Ls outputs are ever used (`[:, :self.segmem_length]`), so the reference's one-layer memory encoder is
        restricted EXACTLY (6.4 -> ~1 GFLOP per segment, SURVEY §7 "segmem-encoder shortcut"): its self-attention — the one
        part written out here — takes keys / values from all L rows and queries from the first Ls; the sublayers behind it
        are the stacks' own pieces on Ls rows.  No dropout, so no site id is drawn (the generic path draws the stack's)."""
        f, d, inner = self.flat, self.d, self.inner
        keep = tape is not None
        Ls = min(self.segmem_length, L)
        emb = lib.embed_fwd(ids.reshape(-1), f.master("decoder_embed_tokens.weight"), None, L, shift=False,
                            pad_id=self.cfg["pad_token_id"])
        emb_a = self._act(emb)
        x = self._input_fwd(emb_a, "segmem_proj", L, 0.0, 0)
        rec = dict(kind="seg_in", ids=ids.reshape(-1), emb=emb_a, L=L, Ls=Ls, B=B)
        if self.segmem_num_layers != 1:
            if keep:
                tape.push(short=False, **rec)
            full = self.stack_fwd("segmem_encoder", x, B, L, self.segmem_num_layers, False, p=0.0, tape=tape)
            return full.view(B, L, d)[:, :Ls]
        pre, b = "segmem_encoder", "segmem_encoder.block.0.layer"
        Wqkv = self.W(f"{pre}.0.qkv")
        _, xn_full, rstd_full = self._proj_addnorm(x, None, self.ln(f"{b}.0.layer_norm.weight"), write_x1=False)
        kv = lib.gemm_nt(xn_full, Wqkv[inner:])                                     # [B*L, 2*inner]
        xs = x.view(B, L, d)[:, :Ls].contiguous().view(B * Ls, d)
        xns = xn_full.view(B, L, d)[:, :Ls].contiguous().view(B * Ls, d)
        q = lib.gemm_nt(xns, Wqkv[:inner])
        o, lse, o_lo = self._attn_fwd(q, kv[:, :inner], kv[:, inner:], B, Ls, L, False, None, 0, 0.0, keep, True)
        # (keep = True also without a tape: B*Ls rows, and xs is x itself when L = Ls — nothing is updated in place)
        x1, ff, pend = self._ff_fwd(xs, (o, self.W(f"{pre}.0.o")), pre, 0, f"{b}.1.layer_norm.weight", 0.0, 0, 0, True)
        out, fin = self._final_fwd(x1, pend, pre, 0.0, 0, 0, True)
        if keep:
            tape.push(short=True, x=x, xn_full=xn_full, rstd_full=rstd_full, kv=kv, xns=xns, q=q, o=o, o_lo=o_lo, lse=lse,
                      s_att=0, ff=ff, fin=fin, **rec)
        return out.view(B, Ls, d)

    def segmem_bwd(self, tape, d_mem):
        """d_mem: fp32 [B, Ls, d] gradient w.r.t. the memory vectors."""
        f, d, inner = self.flat, self.d, self.inner
        if tape.ops[-1]["kind"] != "seg_in":                    # generic multi-layer path
            fin = next(o for o in reversed(tape.ops) if o["kind"] == "seg_in")
            B, L, Ls = fin["B"], fin["L"], fin["Ls"]
            d_full = torch.zeros(B, L, d, device=d_mem.device, dtype=torch.float32)
            d_full[:, :Ls] = d_mem
            dx = self.stack_bwd(tape, d_full.view(B * L, d))
            t = tape.pop()
        else:
            t = tape.pop()
            B, L, Ls = t["B"], t["L"], t["Ls"]
            pre, b = "segmem_encoder", "segmem_encoder.block.0.layer"
            GW, WT = f.GW(f"{pre}.0.qkv"), self.WT(f"{pre}.0.qkv")
            # (the residual gradient stays f32 on these B*Ls rows: it is scattered into the zero-padded f32 one below)
            dx1, dy = self._final_bwd(t["fin"], d_mem.contiguous().view(B * Ls, d), 0.0, True, torch.float32)
            dx1, dy = self._ff_bwd(t["ff"], pre, dx1, dy, 0.0)
            do = self._oproj_bwd(dy, t["o"], f"{pre}.0.o")
            kv = t["kv"]
            dq, dkv = torch.empty_like(t["q"]), torch.empty_like(kv)
            self._attn_bwd(t, t["q"], kv[:, :inner], kv[:, inner:], do, dq, dkv[:, :inner], dkv[:, inner:], B, Ls, L, False,
                           None, 0.0)
            self.wgrad(dq, t["xns"], GW[:inner])
            self.wgrad(dkv, t["xn_full"], GW[inner:])
            # the input gradient of the row-restricted attention: two products (keys / values on all L rows, queries on the
            # first Ls) summed, under the residual gradient zero-padded from Ls to L rows
            dxn_full = lib.gemm_nt(dkv, WT[:, inner:], out_dtype=torch.float32)          # [B*L, d]
            dxns = lib.gemm_nt(dq, WT[:, :inner], out_dtype=torch.float32)               # [B*Ls, d]
            dxn_full.view(B, L, d)[:, :Ls] += dxns.view(B, Ls, d)
            dres = torch.zeros(B, L, d, device=dx1.device, dtype=torch.float32)
            dres[:, :Ls] = dx1.view(B, Ls, d)
            dx, _ = self._norm_bwd(dxn_full, dres.view(B * L, d), t["x"], t["rstd_full"],
                                   self.ln(f"{b}.0.layer_norm.weight"), self.ndw(f"{b}.0.layer_norm.weight"), want_dy=False)
        assert t["kind"] == "seg_in"
        dsrc = self._input_bwd(dx, t["emb"], "segmem_proj", 0.0, 0)
        if "decoder_embed_tokens.weight" in f.frozen:
            return
        demb = lib.gemm_nt(dsrc, self.WT("segmem_proj"), out_dtype=torch.float32)
        self._embed_bwd(t["ids"], demb, f.grad("decoder_embed_tokens.weight"), t["L"], shift=False,
                        pad_id=self.cfg["pad_token_id"])

    @staticmethod
    def prev_row_ids(labels, start_id, pad_id):
        """V1/V2 memory ids (models/t5_segmem_v2.py:126-133) from the shifted decoder inputs."""
        B, L = labels.shape
        dec = torch.cat([labels.new_full((B, 1), start_id), labels[:, :-1]], 1)
        dec = dec.masked_fill(dec == -100, pad_id)
        seg = torch.cat([dec[:, 1:], dec.new_zeros(B, 1)], 1)
        # row 0's memory ids: [1, 0, 0, ...] — built on the device (an indexed host write would be a host-to-device copy,
        # which a hipGraph capture of the step does not allow)
        dummy = (torch.arange(L, device=dec.device) == 0).to(dec.dtype).unsqueeze(0)
        return torch.cat([dummy, seg[:-1]], 0).contiguous()

    # ---- full forward / backward --------------------------------------------------------------------------
    def forward(self, mel, labels, targets_prev=None, training=False, need_grad=False, want_logits=True, pack=None):
        """Returns (logits [B, Ld, V] fp32, tape or None) — or, with want_logits=False, the final-normed decoder states
        [B*Ld, d] in the compute dtype instead of the logits (the trainer feeds them to the fused lm_head + CE call, so
        the 403 MB of f32 logits of a 64-segment batch never exist).  Mirrors get_model_outputs of the four
        reference model classes (models/t5.py:99-180, t5_segmem.py:68-170, t5_segmem_v2.py:64-167,
        t5_segmem_v2_with_prev.py:60-153).

        pack (a lib.PackPlan of these labels, lib.pack_plan): the decoder runs on each row's scored prefix only, its rows packed
        end to end — logits / decoder states come back as [Tcap, ...] rows in packed order, scored against plan.targets.  The
        encoder, the memory encoder and its ids (built from the full labels) stay dense.  Same loss and gradients as the dense
        step (causality: nothing after a row's last scored label reaches a scored position); with dropout on, the row-wise
        masks are keyed by the packed row, so they differ from the dense step's but are drawn the same way."""
        cfg, f = self.cfg, self.flat
        if not mel.is_cuda:
            raise RuntimeError("MR-MT3 MI355X path needs device tensors (no CPU fallback)")
        self.prepare(need_grad)
        p = float(cfg["dropout_rate"]) if training else 0.0
        tape = Tape() if need_grad else None
        B, Le, d = mel.shape
        Ld = labels.shape[1]
        labels = labels.contiguous()
        Ls = self.segmem_length
        enc = self.encode(mel, p=p, tape=tape)                                  # [B*Le, d]
        table = f.master("decoder_embed_tokens.weight")
        start, pad = cfg["decoder_start_token_id"], cfg["pad_token_id"]
        pos = self.pos(mel.device)
        variant = self.variant
        mem = None
        if variant == "segmem_v2_with_prev":
            assert targets_prev is not None
            targets_prev.masked_fill_(targets_prev == -100, pad)                 # in place, like the reference (:119)
        if Ls == 0:
            # model_segmem_length=0 (the reference's no-memory ablation): `[:, :0]` leaves nothing to attend
            # to or prepend, so the step is the plain MT3 one and the memory block receives no gradient
            variant = "t5"
        if variant != "t5":
            if variant == "segmem_v2_with_prev":
                ids = targets_prev.contiguous()
            else:
                ids = self.prev_row_ids(labels, start, pad)
            Lm = ids.shape[1]
            mem = self.segmem(ids, B, Lm, tape=tape)                             # [B, Ls, d]
            Ls = mem.shape[1]
        s_emb = self._sid()
        if variant == "segmem_v1" and pack is not None:
            raise ValueError("packed decoder rows are not supported for segmem_v1 (its memory slots are prepended to the "
                             "decoder input)")
        if variant == "segmem_v1":
            # memory is PREPENDED to the decoder input embeddings (t5_segmem.py:138-160)
            emb = lib.embed_fwd(labels.view(-1), table, None, Ld, shift=True, start_id=start, pad_id=pad)
            xin = torch.cat([mem.float(), emb.view(B, Ld, d)], 1).contiguous()
            Lx = Ld + Ls
            x = lib.addpos_fwd(xin.view(B * Lx, d), pos, Lx, p=p, seed=self.seed, step=self.step_dev, stream_id=s_emb)
            enc_cat, Lc = enc, Le
        else:
            Lx = Ld
            if pack is not None:
                x = lib.embed_fwd_packed(pack, table, pos, p=p, seed=self.seed, step=self.step_dev, stream_id=s_emb)
            else:
                x = lib.embed_fwd(labels.view(-1), table, pos, Ld, shift=True, start_id=start, pad_id=pad, p=p,
                                  seed=self.seed, step=self.step_dev, stream_id=s_emb)
            if mem is not None:
                enc_cat = torch.cat([enc.view(B, Le, d), mem], 1).contiguous().view(-1, d)
                Lc = Le + Ls
            else:
                enc_cat, Lc = enc, Le
        if tape is not None:
            tape.push(kind="dec_in", s_emb=s_emb, p=p, labels=labels, B=B, Le=Le, Ld=Ld, Lx=Lx, Lc=Lc, Ls=Ls,
                      Lm=(ids.shape[1] if variant != "t5" else 0), variant=variant, pack=pack)
        head_f32 = self.head_dtype == "f32" and tape is None and self.dt == torch.bfloat16
        dec = self.stack_fwd("decoder", x, B, Lx, cfg["num_decoder_layers"], True, enc=enc_cat, Le=Lc, p=p, tape=tape,
                             out_dtype=torch.float32 if head_f32 else None, pack=pack)
        if variant == "segmem_v1":
            dec = dec.view(B, Lx, d)[:, Ls:].contiguous().view(B * Ld, d)
        if tape is not None:
            tape.push(kind="head", dec=dec)
        if not want_logits:
            return dec, tape
        w_head = f.W("lm_head", torch.float32) if head_f32 else self.W("lm_head")
        logits = lib.gemm_nt(dec, w_head, out_dtype=torch.float32)               # [B*Ld, V]
        if pack is not None:
            return logits, tape                                                   # [Tcap, V], packed rows
        return logits.view(B, Ld, self.V), tape

    def backward(self, tape, dlogits, on_layer_done=None):
        """dlogits: [B*Ld, V] in the compute dtype (anything else is cast).  Accumulates into flat.G.  With an fp32 engine
        every product, the attention backward and the row-wise kernels run in exact f32 (the reference's own training
        precision, config/config_slakh_segmem.yaml:47): slow, and the tight pin of this hand-written tape against autograd."""
        f, cfg, d = self.flat, self.cfg, self.d
        variant, Ls = self.variant, self.segmem_length
        t = tape.pop()
        assert t["kind"] == "head"
        dl = dlogits.reshape(-1, self.V)
        if dl.dtype != self.dt:
            dl = self._act(dl)
        self.wgrad(dl, t["dec"], f.GW("lm_head"))
        d_dec = lib.gemm_nt(dl, self.WT("lm_head"), out_dtype=torch.float32)
        if on_layer_done is not None:
            on_layer_done("lm_head", 0)
        # peek the decoder-input record (it sits below the decoder stack's records)
        din = next(o for o in reversed(tape.ops) if o["kind"] == "dec_in")
        B, Le, Ld, Lx, Lc, Ls = din["B"], din["Le"], din["Ld"], din["Lx"], din["Lc"], din["Ls"]
        variant = din["variant"]                                # "t5" when segmem_length is 0
        if variant == "segmem_v1":
            full = torch.zeros(B, Lx, d, device=d_dec.device, dtype=torch.float32)
            full[:, Ls:] = d_dec.view(B, Ld, d)
            d_dec = full.view(B * Lx, d)
        # Backward cut-off: with the whole encoder (and the memory encoder, if there is one) frozen nothing below the
        # cross-attention k|v projections needs a gradient — d_enc is not formed and those backward passes do not run
        skip_enc = self.encoder_frozen()
        skip_mem = variant == "t5" or self.segmem_frozen()
        # (segmem_v1's memory gradient comes out of the decoder INPUT; the other variants' memory rows are part of d_enc)
        need_d_enc = not skip_enc if variant in ("t5", "segmem_v1") else not (skip_enc and skip_mem)
        d_enc_cat = (torch.empty(B * Lc, d, device=d_dec.device, dtype=torch.float32)      # written by stack_bwd's one d_enc product
                     if need_d_enc else None)
        dx = self.stack_bwd(tape, d_dec, d_enc=d_enc_cat, on_layer_done=on_layer_done)
        t = tape.pop()
        assert t["kind"] == "dec_in"
        table_g = f.grad("decoder_embed_tokens.weight")
        start, pad = cfg["decoder_start_token_id"], cfg["pad_token_id"]
        d_mem = None
        if variant == "segmem_v1":
            dxm = lib.dropmask_cast(dx, p=t["p"], seed=self.seed, step=self.step_dev, stream_id=t["s_emb"],
                                    out_dtype=self.dt).float().view(B, Lx, d)
            d_mem = dxm[:, :Ls]
            self._embed_bwd(t["labels"].view(-1), dxm[:, Ls:].contiguous().view(-1, d), table_g, Ld, shift=True,
                            start_id=start, pad_id=pad)
            d_enc = d_enc_cat
        else:
            if t["pack"] is not None:          # the packed inputs are already shifted: a plain scatter-add over the Tcap rows
                self._embed_bwd(t["pack"].dec_ids, dx, table_g, t["pack"].Tcap, shift=False, pad_id=pad, p=t["p"],
                                seed=self.seed, step=self.step_dev, stream_id=t["s_emb"])
            else:
                self._embed_bwd(t["labels"].view(-1), dx, table_g, Ld, shift=True, start_id=start, pad_id=pad, p=t["p"],
                                seed=self.seed, step=self.step_dev, stream_id=t["s_emb"])
            if variant != "t5" and d_enc_cat is not None:
                dcat = d_enc_cat.view(B, Lc, d)
                d_enc = None if skip_enc else dcat[:, :Le].contiguous().view(-1, d)
                d_mem = None if skip_mem else dcat[:, Le:]
            else:
                d_enc = d_enc_cat
        if variant != "t5":
            if skip_mem:                                       # frozen memory encoder: its records leave the tape unread
                while tape.ops.pop()["kind"] != "seg_in":
                    pass
            else:
                self.segmem_bwd(tape, d_mem)
            if on_layer_done is not None:
                on_layer_done("segmem", 0)                     # the memory encoder's gradients are final (their bucket may leave)
        if skip_enc:
            del tape.ops[:]                                    # frozen encoder: no d_enc was formed, nothing is launched
        else:
            self.encode_bwd(tape, d_enc, on_layer_done=on_layer_done)
        self.join_wgrad()
        assert not tape.ops, [o["kind"] for o in tape.ops]
