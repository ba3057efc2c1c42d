"""Operand modes of the DiT engine: where a block's GEMM operands live and how a launch on them is described, once per operand format.

DiTEngine writes its blocks once, against the LOGICAL operands `xn` (the AdaLN-normalised stream), `attn` (the attention output), `mlp`
(the GELU'd hidden) and `attn_mlp` ([attn | mlp] as the ONE K = 5D operand of the single blocks' proj_out), and the logical outputs `qkv`
(k | v | q), `mlp` (stored with GELU) and `x` (the gated residual into X). A mode maps those names to buffers, columns, K, lo offsets and
scales and owns the launches whose form depends on the format: AdaLN LayerNorm, adapter down-projection, grouped
GEMM, fused projection, attention step, embedders. It holds its engine (weakly: the last owner still releases an engine) and no state."""
from __future__ import annotations

import weakref
from typing import Optional

import torch

from .. import ops
from ..ops import LX_EPI_GELU, LX_EPI_RESID_F32, LX_EPI_STORE_BF16, LX_EPI_STORE_F32


class Mode:
    def __init__(self, eng):
        self._eng = weakref.ref(eng)

    eng = property(lambda self: self._eng())

    def fused(self, p: str, ready, image_out_only: bool, qkv) -> None:
        """The single blocks' [k | v | q | mlp] projection of xn. Where q/k/v and the hidden differ in format (e4m3, split): two launches over
        the weight's row ranges, the second with the first's adapter slabs from column 3r on; image_out_only: the image rows' hidden only."""
        D, only = self.eng.cfg.inner_dim, ("img",) if image_out_only else None
        r_qkv, r_mlp = ({s: slice(*r) for s in ("txt", "img", "cond")} for r in ((0, 3 * D), (3 * D, 7 * D)))
        lora = self.gemm("xn", "qkv", p + ".fused", None, w_rows=r_qkv, lora_mod_cols=D, lora_toff_max=2)
        self.gemm("xn", "mlp", p + ".fused", None, w_rows=r_mlp, t_col0=3 * self.eng.cfg.lora_r, only=only, lora=lora)


class Mode16(Mode):
    """bf16 or fp16 operand images (engine.f16 says which; the same buffers, viewed by engine._op): XN and the columns of Y."""
    COLS = {"qkv": (0, 3), "attn": (2, 3), "mlp": (3, 7), "attn_mlp": (2, 7)}      # of Y = [k | v | q -> attn | mlp], in units of D

    def operand(self, a: str) -> torch.Tensor:
        e, D = self.eng, self.eng.cfg.inner_dim
        return e.XN if a == "xn" else e.Y[:, self.COLS[a][0] * D: self.COLS[a][1] * D]

    def ln(self, base_by_stream, shift_off: int, scale_off: int, lora_for: Optional[str] = None, include_txt: bool = False):
        """AdaLN LayerNorm + modulation of every stream of this forward into `xn`.
        lora_for: the Linear that reads xn next (its adapter's down-projection of the adapter rows is computed by the same launch, on the
        matrix pipe, while the normalised rows are at hand: 76 of the 132 lx_lora_down launches of a denoise step sit behind a LayerNorm).
        Returns what gemm() takes as `lora` ((adapter, 1 slab, first adapter row)), or None when there is nothing to hand over."""
        e = self.eng
        segs = e._ln_segs(base_by_stream, shift_off, scale_off)
        lora, ready = None, None
        lo = e.w.lora.get(lora_for) if lora_for is not None else None
        if (lo is not None and e.ln_lora and e.lora_scale == 1.0 and e.lora_w is None and lo.down.shape[0] <= 16
                and e.cfg.inner_dim in (3072, 256) and e._lora_rows(include_txt) is not None):      # (the widths the kernel is built for)
            r0, n = e._lora_rows(include_txt)
            lora = (e._down(lora_for, lo), e.TL[r0:r0 + n, : lo.down.shape[0]], r0, n)       # slab 0 of TLs: the consumer sums one slab
            ready = (lo, 1, r0)
        if e.f16:
            ops.ln_modulate_segs(e.X, segs, e.XN16, e.mods.stride(0), f16_ovf=e.f16_ovf, lora=lora)
        else:
            ops.ln_modulate_segs(e.X, segs, e.XN, e.mods.stride(0), lora=lora)
        return ready

    def lora_t(self, A: torch.Tensor, name: str, include_txt: bool = False):
        """The adapter's down-projection of the adapter rows of the 16-bit image A, as the `lora` of the launch that consumes it."""
        e = self.eng
        lo = e.w.lora.get(name)
        if lo is None or e.lora_scale == 0.0 or e._lora_rows(include_txt) is None:
            return e.NO_LORA
        r0, n = e._lora_rows(include_txt)
        t = e.TL[r0:r0 + n, : lo.down.shape[0]]
        ops.lora_down(e._op(A[r0:r0 + n]), e._down(name, lo), t, n_split=e.TL_SPLIT, split_stride=e.TLs.stride(0))
        e._scale_lora(t, e._lora_segs(r0, n), n_slab=e.TL_SPLIT)
        return lo, e.TL_SPLIT, r0

    def launch(self, A: torch.Tensor, Cbuf: torch.Tensor, main: str, txt: Optional[str], *, epilogue, gelu_col_start=0, qkv=None, only=None, lora=None, **kw):
        """The grouped launch (engine._launch_streams) of the 16-bit image A into Cbuf. lora = None: the adapter's down-projection is computed
        here, from A. qkv = (wq, wk, wq_txt, wk_txt[, layer]): RMSNorm + RoPE + V^T in the launch's epilogue. Returns the `lora` it ran with."""
        e = self.eng
        if lora is None:
            lora = self.lora_t(A, main, include_txt=txt is None) if e._lora_wanted(only) else e.NO_LORA

        def desc(s, name: str, rows: Optional[slice], **k):
            a, c = e._op(e.rows(A, s.name)), e.rows(Cbuf, s.name)
            if e.f16 and (epilogue & 0xff) == LX_EPI_STORE_BF16 and qkv is None:
                c = c.view(torch.float16)               # a 16-bit store of this mode is the next GEMM's fp16 operand
            if qkv is not None:
                k["qkv"] = e._qkv_kw(s, qkv)
            return ops.gemm_desc(a, e._w_rows(e._W(name), rows), c, gelu_col_start=gelu_col_start, **k, **e._f16_kw())

        e._launch_streams(desc, e.gemm_ws(), main, txt, epilogue=epilogue, only=only, lora=lora, **kw)
        return lora

    def gemm(self, a: str, out: str, main: str, txt: Optional[str], **kw):
        """Linear main / txt over the token streams, from logical operand a into logical output out (every mode's form of
        engine._launch_streams, whose keywords it takes). Returns the `lora` it ran with, for a sibling launch over the same operand."""
        Cbuf, epilogue = (self.eng.X, LX_EPI_RESID_F32) if out == "x" else (self.operand(out), LX_EPI_STORE_BF16 | (LX_EPI_GELU if out == "mlp" else 0))
        return self.launch(self.operand(a), Cbuf, main, txt, epilogue=epilogue, **kw)

    def single(self, a: str, stream: str, name: str, C: torch.Tensor, **k) -> None:
        """One ungrouped launch of Linear `name` on one stream's rows of logical operand a (in this mode: without the workspace plans)."""
        e = self.eng
        ops.gemm([ops.gemm_desc(e._op(e.rows(self.operand(a), stream)), e._W(name), C, **k, **e._f16_kw())])

    def fused(self, p: str, ready, image_out_only: bool, qkv) -> None:
        """Here ONE launch over all of Y, GELU from the mlp columns on; image_out_only: the text and condition rows get k | v only."""
        e, D = self.eng, self.eng.cfg.inner_dim
        kv_only = {"txt": slice(0, 2 * D), "cond": slice(0, 2 * D)} if image_out_only else None
        self.launch(e.XN, e.Y, p + ".fused", None, epilogue=LX_EPI_STORE_BF16 | LX_EPI_GELU, gelu_col_start=3 * D, lora_mod_cols=D, lora_toff_max=3,
                    w_rows=kv_only, qkv=qkv, lora=ready)

    def attention(self, wq, wk, wq_txt, wk_txt, prepped: bool = False, layer: Optional[int] = None, img_only: bool = False) -> None:
        """RMSNorm + RoPE of q / k and V^T (unless the projection's epilogue did them: prepped), then the joint attention, O over q in Y.
        img_only: only the image segment has queries (the last single block of a forward: the text / condition rows serve keys and values,
        their q columns were not computed and hold whatever the previous layer left there)."""
        e = self.eng
        D, H, B, Y = e.cfg.inner_dim, e.cfg.num_attention_heads, e.B, e.Y
        cached = e.cond_cache and layer is not None
        streams = e._all_streams() if cached else e._streams()      # key / value segments (queries: the streams of this forward)
        seg_row0, seg_len, seg_vt0, bias, _ = e._attn_segments(streams)
        # the separate q / k / v pass: the streams with rows in this forward (a cond_skip forward leaves the condition stream's part of the
        # per-layer images as the first forward of the conditioning wrote it)
        qsegs = [] if prepped else e._qsegs(e._streams(), wq, wk, wq_txt, wk_txt)
        # cached, in a cond_skip forward: only the text / image segments have queries (img_only: qseg_mask, which wins)
        nq = len(e._streams()) if cached and e.cond_skip and not img_only else 0
        flags = (ops.ATTN_Q_LOG2 | ops.ATTN_BOUNDED) if e._layer_nomax(wq) else 0
        if not e.pair_plan:             # the batch-size-invariant plans: the attention kernel must not depend on the batch size either
            flags |= ops.ATTN_INVARIANT
        okw = dict(f16_ovf=e.f16_ovf) if e.f16 else {}      # O is the output projection's A operand: fp16 in the fp16 operand mode
        if img_only:
            okw["qseg_mask"] = 1 << [s.name for s in streams].index("img")
        if e.f16:
            flags |= ops.ATTN_O_F16
        # the caller's mask: a block-level call's (prepared inside the call) or the conditioning's (prepared by set_conditioning)
        mask, mask_ws = (e.attn_mask, None) if e.attn_mask is not None else (e.cond_mask, e._mask_ws)
        if mask is not None:
            # lx_attn_fwd_masked: always a running maximum -- BOUNDED / INVARIANT do not apply to it
            if e.model_config.get("attn_fp8", False):
                raise NotImplementedError("attention_mask is not supported in attn_fp8 mode")
            if cached:        # (unreachable through the public surface: condition caching exists only under rules that replace the mask)
                raise NotImplementedError("attention_mask is not supported on condition-cached forwards")
            if not prepped:
                ops.qkv_prep_segs(Y, 2 * D, 0, D, qsegs, B, H, e.VT, in_f16=e.f16)
            mflags = (ops.ATTN_Q_LOG2 if e._layer_nomax(wq) else 0) | (ops.ATTN_O_F16 if e.f16 else 0)
            ops.attn_fwd_masked(Y, Y, e.VT, Y, mask, q_col=2 * D, k_col=0, o_col=2 * D, B=B, H=H, seg_row0=seg_row0, seg_len=seg_len,
                                seg_vt0=seg_vt0, bias=bias, flags=mflags, workspace=mask_ws, prepped=mask_ws is not None, **okw)
            return
        if e.model_config.get("attn_fp8", False):
            # opt-in fp8 (e4m3) attention (BASELINE configs[4]): q / k / v^T go to byte images, both attention products run on
            # the 64-deep f8f6f4 MFMA; softmax statistics and the output accumulators stay fp32 (include/lx.h, lx_attn_fwd_fp8)
            e._fp8_images()
            # cached: keys / V^T of this forward's streams into the layer's e4m3 images, where the attention reads all streams' from
            K8, VT8 = (e.KC8[layer], e.VTC8[layer]) if cached else (e.K8, e.VT8)
            if not prepped:                # otherwise the projection epilogue already wrote the three byte images
                ops.qkv_prep_fp8_segs(Y, 2 * D, 0, D, qsegs, B, H, e.Q8, K8, VT8, in_f16=e.f16)
            f8 = (ops.ATTN_O_F16 if e.f16 else 0) | (ops.ATTN_P_EXP2 if e.model_config.get("attn_fp8_exp2", False) else 0)
            if cached:
                okw["n_qseg"] = nq
            ops.attn_fwd_fp8(e.Q8, K8, VT8, Y, o_col=2 * D, B=B, H=H, seg_row0=seg_row0, seg_len=seg_len, seg_vt0=seg_vt0, bias=bias, flags=f8, **okw)
            return
        if cached:
            # keys from the layer's key image, V^T from the layer's V^T image (the condition stream's part written by the first
            # forward of this conditioning); in a cond_skip forward only the text / image segments have queries
            if not prepped:                # no fused epilogue (stream lengths it does not take, or switched off): the separate pass writes them
                ops.qkv_prep_kv_segs(Y, 2 * D, 0, D, qsegs, B, H, e.KC[layer], 0, e.VTC[layer], in_f16=e.f16)
            ops.attn_fwd(Y, e.KC[layer], e.VTC[layer], Y, q_col=2 * D, k_col=0, o_col=2 * D, B=B, H=H, seg_row0=seg_row0,
                         seg_len=seg_len, seg_vt0=seg_vt0, bias=bias, n_qseg=nq, flags=flags, **okw)
            return
        if not prepped:                    # otherwise the projection launch already normalised / rotated k and q and wrote V^T
            # (fp16 operand mode: an unfused projection stored k | v | q as fp16 -- the pass reads them as such and leaves bf16 k / q, bf16 V^T)
            ops.qkv_prep_segs(Y, 2 * D, 0, D, qsegs, B, H, e.VT, in_f16=e.f16)
        ops.attn_fwd(Y, Y, e.VT, Y, q_col=2 * D, k_col=0, o_col=2 * D, B=B, H=H, seg_row0=seg_row0, seg_len=seg_len,
                     seg_vt0=seg_vt0, bias=bias, flags=flags, **okw)

    def embed(self, x: torch.Tensor, name: str, out: torch.Tensor, lora: bool, step: bool = False) -> None:
        """out(fp32) = Linear_name(x) on the 16-bit image of x (context_embedder / x_embedder). step: x is the step's latents, converted
        into the engine's own image (nothing is allocated: this runs inside the step graph's capture)."""
        e = self.eng
        if step:
            x, lat = e._op(e.lat16), x
            ops.convert(x, lat.contiguous())
        x = x.to(device=e.device, dtype=torch.float16 if e.f16 else torch.bfloat16).contiguous()
        lo = e.w.lora.get(name) if (lora and e.lora_scale != 0.0) else None
        tl = None
        if lo is not None:               # (no row guard, unlike SplitMode.embed: DESIGN.md section 7)
            tl = e.TL[: x.shape[0], : e.cfg.lora_r]
            ops.lora_down(x, e._down(name, lo), tl)
            e._scale_lora(tl, e._embed_segs(x.shape[0]))
        ops.gemm([ops.gemm_desc(x, e._W(name), out, bias=e.w.t[name + ".b"], epilogue=LX_EPI_STORE_F32, lora_t=tl,
                                lora_up=lo.up if lo is not None else None, **e._f16_kw())])


class E4M3Mode(Mode16):
    """model_config["gemm_fp8"]: the block GEMMs read e4m3 images with fixed activation scales, XN8 = e4m3(xn * S_X8) and Y8 = [attn | mlp]
    = e4m3(. * S_Y8), against tiled e4m3 weights with per-output-row scales (engine.w8, engine._cs); no workspace: lx_gemm_fp8_kernel
    has no pair plan. xn, q/k/v and the attention output also exist as bf16 (XN, Y): the adapters and the attention prep read those. The
    embedders and the final projection are Mode16's, on bf16 operands."""

    def ln(self, base_by_stream, shift_off, scale_off, lora_for=None, include_txt=False):
        e = self.eng                          # XN (bf16, for the adapters' down-projection) + XN8
        ops.ln_modulate_fp8_segs(e.X, e._ln_segs(base_by_stream, shift_off, scale_off), e.XN, e.XN8, e.mods.stride(0), e.S_X8)

    def gemm(self, a: str, out: str, main: str, txt: Optional[str], *, lora=None, **kw):
        e, D = self.eng, self.eng.cfg.inner_dim
        A8, act_scale = (e.XN8, e.S_X8) if a == "xn" else (e.Y8[:, D if a == "mlp" else 0: D if a == "attn" else 5 * D], e.S_Y8)
        Cbuf, epilogue, out_scale = ((e.Y8[:, D:], ops.LX_EPI_STORE_FP8 | LX_EPI_GELU, e.S_Y8) if out == "mlp" else      # the hidden: straight to e4m3
                                     (e.X, LX_EPI_RESID_F32, 0.0) if out == "x" else (self.operand(out), LX_EPI_STORE_BF16, 0.0))
        # The adapter's down-projection: from the operand's bf16 image where it has one, else from the e4m3 one. Unlike the other two modes
        # this does not ask whether the launch has adapter rows at all (engine._lora_wanted): DESIGN.md section 7.
        if lora is None and a in ("xn", "attn"):
            lora = self.lora_t(self.operand(a), main, txt is None)
        elif lora is None:
            lo, rows = e.w.lora.get(main), e._lora_rows(txt is None)
            lora = e.NO_LORA
            if lo is not None and e.lora_scale != 0.0 and rows is not None:
                t = e.TL[rows[0]:rows[0] + rows[1], : lo.down.shape[0]]
                ops.lora_down_fp8(A8[rows[0]:rows[0] + rows[1]], e.lora_scale / act_scale, lo.down, t, n_split=e.TL_SPLIT, split_stride=e.TLs.stride(0))
                if e.lora_w_ns is not None:             # (lora_scale went in with the descale above: the table without it)
                    e._scale_lora(t, e._lora_segs(*rows), n_slab=e.TL_SPLIT, table=e.lora_w_ns)
                lora = (lo, e.TL_SPLIT, rows[0])

        def desc(s, name: str, rows: Optional[slice], **k):
            return ops.gemm_desc(e.rows(A8, s.name), e._w_rows(e.w8[name], rows), e.rows(Cbuf, s.name), fp8=True,
                                 col_scale=e._cs(name, act_scale, rows), out_scale=out_scale, **k)

        e._launch_streams(desc, None, main, txt, epilogue=epilogue, lora=lora, **kw)
        return lora

    fused = Mode.fused                             # q/k/v as bf16 for the attention prep, the MLP hidden straight to e4m3

    def attention(self, wq, wk, wq_txt, wk_txt, prepped=False, layer=None, img_only=False) -> None:
        """The unfused bf16 attention + its output's e4m3 image. No per-layer images (no condition cache here); no img_only (DESIGN.md s. 7)."""
        e, D = self.eng, self.eng.cfg.inner_dim
        Mode16.attention(self, wq, wk, wq_txt, wk_txt)
        ops.convert_fp8(e.Y[:, 2 * D: 3 * D], e.Y8[:, :D], e.S_Y8)


class SplitMode(Mode):
    """model_config["precise"]: every operand a bf16 (hi | lo) pair, hi in columns [0, K) and lo `a_lo_off` columns further; weights
    [W_hi | W_lo] where they have a rounding residual. xn in XN2, q/k/v as fp32 in Y32, [attn | mlp] in YA."""

    def operand(self, a: str):                      # -> (pair buffer, K, lo offset)
        e, D = self.eng, self.eng.cfg.inner_dim
        if a == "xn":
            return e.XN2, D, D
        return (e.YA[:, D:] if a == "mlp" else e.YA), {"attn": D, "mlp": 4 * D, "attn_mlp": 5 * D}[a], 5 * D

    def ln(self, base_by_stream, shift_off, scale_off, lora_for=None, include_txt=False):
        e = self.eng
        ops.ln_modulate_split_segs(e.X, e._ln_segs(base_by_stream, shift_off, scale_off), e.XN2, e.mods.stride(0), e.cfg.inner_dim)

    def desc(self, A2: torch.Tensor, name: str, Cbuf: torch.Tensor, *, K: int, a_lo_off: int, w_rows: Optional[slice] = None, **kw):
        """GEMM descriptor of a split-bf16 launch: A2 holds the hi image in columns [0, K) and the lo image a_lo_off columns
        further; the weight is [W_hi | W_lo] (3 K-segments) when it has a rounding residual, else W (2 segments)."""
        e = self.eng
        w2 = e.w.t.get(name + ".w2")
        W = e._w_rows(w2 if w2 is not None else e.w.t[name + ".w"], w_rows)
        return ops.gemm_desc(A2, W, Cbuf, K=K, N=W.shape[0], k_segs=3 if w2 is not None else 2, a_lo_off=a_lo_off, **kw)

    def lora_terms(self, A2: torch.Tensor, name: str, K: int, a_lo_off: int, r0: int, n: int, segs=None):
        """t = x A_down^T for rows [r0, r0+n) with x = hi + lo: one slab per cross term (the consumer GEMM adds them).
        Returns the `lora` of the launch that consumes them (NO_LORA: no adapter on this Linear). segs: how the rows map to images where
        they are not the token streams' (_lora_segs)."""
        e = self.eng
        lo = e.w.lora.get(name)
        if lo is None or e.lora_scale == 0.0:
            return e.NO_LORA
        R = lo.down.shape[0]
        terms = [(A2[r0:r0 + n, :K], lo.down), (A2[r0:r0 + n, a_lo_off:a_lo_off + K], lo.down)]
        if lo.down_lo is not None:
            terms.append((A2[r0:r0 + n, :K], lo.down_lo))
        # one launch for the cross terms (slab s = term s; the consumer GEMM adds the slabs)
        ops.lora_down_terms(terms, e.TLs[0, r0:r0 + n, :R], e.TLs.stride(0))
        e._scale_lora(e.TLs[0, r0:r0 + n, :R], e._lora_segs(r0, n) if segs is None else segs, n_slab=len(terms))
        return lo, len(terms), r0

    def gemm(self, a: str, out: str, main: str, txt: Optional[str], *, only=None, lora=None, **kw):
        e, D = self.eng, self.eng.cfg.inner_dim
        A2, K, a_lo_off = self.operand(a)
        # the hidden becomes a GELU'd bf16 pair, hi at [D, 5D) of YA and lo 5D further; q/k/v stay fp32
        Cbuf, epilogue, c_lo_off = ((e.YA[:, D:], LX_EPI_STORE_BF16 | LX_EPI_GELU, 5 * D) if out == "mlp" else
                                    (e.X, LX_EPI_RESID_F32, 0) if out == "x" else (e.Y32, LX_EPI_STORE_F32, 0))
        if lora is None:
            lora = e.NO_LORA
            if e._lora_wanted(only) and e._lora_rows(txt is None) is not None:
                lora = self.lora_terms(A2, main, K, a_lo_off, *e._lora_rows(txt is None))

        def desc(s, name: str, rows: Optional[slice], **k):
            return self.desc(e.rows(A2, s.name), name, e.rows(Cbuf, s.name), K=K, a_lo_off=a_lo_off, w_rows=rows, c_lo_off=c_lo_off, **k)

        # (the workspace admits lx_gemm4_kernel<true> and its split form; None under LX_PAIR_PLAN=0)
        e._launch_streams(desc, e.gemm_ws(), main, txt, epilogue=epilogue, only=only, lora=lora, **kw)
        return lora

    def single(self, a: str, stream: str, name: str, C: torch.Tensor, **k) -> None:
        A2, K, a_lo_off = self.operand(a)
        ops.gemm([self.desc(self.eng.rows(A2, stream), name, C, K=K, a_lo_off=a_lo_off, **k)], self.eng.gemm_ws())

    def attention(self, wq, wk, wq_txt, wk_txt, prepped: bool = False, layer: Optional[int] = None, img_only: bool = False) -> None:
        """fp32 q / k / v in Y32 = [k | v | q]: per-head RMSNorm + RoPE in fp32, fp32 attention, output pair into YA's attn columns.
        layer: the block's index among all blocks, for the per-layer images of the condition cache. img_only: only the image segment has
        queries (the last single block of a forward; split-bf16 attention only -- the exact-fp32 kernel has no query-segment subset)."""
        e = self.eng
        D, H, B = e.cfg.inner_dim, e.cfg.num_attention_heads, e.B
        if e.precise_attn_split:
            # split-bf16 attention: hi.hi + hi.lo + lo.hi on the bf16 MFMA (3/16 of the fp32-MFMA cost), fp32 softmax
            cached = e.cond_cache and layer is not None
            qsegs = e._qsegs(e._streams(), wq, wk, wq_txt, wk_txt)          # the prep pass: the streams with rows in this forward
            streams = e._all_streams() if cached else e._streams()      # key / value segments
            seg_row0, seg_len, seg_vt0, bias, _ = e._attn_segments(streams)
            kw, vt = {}, e.VT2
            if cached:
                # k and V^T pairs of this forward's streams into the layer's images (q into the shared QK2): the condition stream's part is
                # written by the first forward of a conditioning and left alone by the cond_skip forwards, which read it from there
                vt = e.VTC2[layer]
                ops.qkv_prep_split_kv_segs(e.Y32, 2 * D, 0, D, qsegs, B, H, e.QK2, 2 * D, e.KC2[layer], 0, D, vt)
                kw["K"] = e.KC2[layer]
            else:
                ops.qkv_prep_split_segs(e.Y32, 2 * D, 0, D, qsegs, B, H, e.QK2, q2_col=2 * D, k2_col=0, lo_off=D, VT2=vt)
            if img_only:
                kw["qseg_mask"] = 1 << [s.name for s in streams].index("img")
            elif cached and e.cond_skip:
                kw["n_qseg"] = len(e._streams())
            ops.attn_fwd_split(e.QK2, vt, e.YA, q_col=2 * D, k_col=0, qk_lo_off=D, o_col=0, o_lo_off=5 * D, B=B, H=H, seg_row0=seg_row0, seg_len=seg_len,
                               seg_vt0=seg_vt0, bias=bias, flags=(ops.ATTN_Q_LOG2 | ops.ATTN_BOUNDED) if e._layer_nomax(wq) else 0, **kw)
            return
        seg_row0, seg_len, seg_vt0, bias, qsegs = e._attn_segments(e._streams(), (wq, wk, wq_txt, wk_txt))
        ops.qkv_prep_f32_segs(e.Y32, 2 * D, 0, qsegs, B, H)
        ops.attn_fwd_f32(e.Y32, e.YA, q_col=2 * D, k_col=0, v_col=D, o_col=0, o_lo_off=5 * D, B=B, H=H, seg_row0=seg_row0, seg_len=seg_len, bias=bias)

    def embed(self, x32: torch.Tensor, name: str, out: torch.Tensor, lora: bool, step: bool = False) -> None:
        """out(fp32) = Linear_name(x32) with x as a hi/lo pair (context_embedder / x_embedder). step: the pair goes into the engine's lat2."""
        e = self.eng
        x32 = x32.to(device=e.device, dtype=torch.float32).contiguous()
        rows, K = x32.shape
        pair = e.lat2 if step else torch.empty(rows, 2 * K, dtype=torch.bfloat16, device=e.device)
        ops.split_bf16(x32, pair, K)
        kw = {}
        if lora:
            # the row guard: more input rows than the adapter scratch holds -> no adapter term (Mode16.embed has none: DESIGN.md section 7)
            lo, ns, _ = self.lora_terms(pair, name, K, K, 0, rows, segs=e._embed_segs(rows)) if rows <= e.TLs.shape[1] else e.NO_LORA
            if lo is not None:
                kw = dict(lora_t=e.TL[:rows], lora_up=lo.up, lora_nsplit=ns, lora_split_stride=e.TLs.stride(0))
        ops.gemm([self.desc(pair, name, out, K=K, a_lo_off=K, bias=e.w.t[name + ".b"], epilogue=LX_EPI_STORE_F32, **kw)], e.gemm_ws())
