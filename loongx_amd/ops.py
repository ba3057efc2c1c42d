"""Thin torch-tensor -> C-ABI wrappers (one function per include/lx.h entry point).

torch is used for device memory and streams only; every function here launches a hand-written HIP kernel
from liblx_amd.so on the current torch stream and raises LxError on failure.  There is no fallback.
"""
from __future__ import annotations

import ctypes as C
import math
from typing import Optional, Sequence

import torch

from . import _lib as L
from ._lib import (LX_EPI_QKV, LX_EPI_GELU, LX_EPI_RESID_F32, LX_EPI_SPLIT_BF16, LX_EPI_STORE_BF16, LX_EPI_STORE_F32, LX_EPI_STORE_FP8, LX_OPERANDS_F16, LX_OPERANDS_FP8, LX_W_TILED,
                   AttnDesc, GemmDesc, check, lib)


def _stream() -> int:
    return torch.cuda.current_stream().cuda_stream


def _p(t: Optional[torch.Tensor]) -> Optional[int]:
    return None if t is None else t.data_ptr()


def _req(t: torch.Tensor, dtype, name: str):
    if t.dtype != dtype:
        raise TypeError(f"{name}: expected {dtype}, got {t.dtype}")
    if not t.is_cuda:
        raise ValueError(f"{name}: must live on the GPU (the hot path has no CPU fallback)")


def tile_weight(W: torch.Tensor) -> torch.Tensor:
    """nn.Linear weight [N,K] bf16 (N % 256 == 0, K % 64 == 0) -> the pre-tiled layout LX_W_TILED expects, same shape/bytes:
    [N/256][K/64] blocks of 256 rows x 64 cols; inside a block row r, the 16-B chunk c sits at position c ^ ((r>>1)&7)
    (the LDS swizzle of gemm.hip), so the kernel's global->LDS DMA copies a block verbatim. Pure layout plumbing.
    e4m3 weights (uint8 [N,K], K % 128 == 0) tile the same way with 128 elements per 128-B block row (16 per chunk)."""
    N, K = W.shape
    e = 16 // W.element_size()                       # elements per 16-B chunk
    assert W.dtype in (torch.bfloat16, torch.float16, torch.uint8) and N % 256 == 0 and K % (8 * e) == 0
    t = W.reshape(N // 256, 256, K // (8 * e), 8, e).permute(0, 2, 1, 3, 4)       # [nb, kb, row, chunk, e]
    r = torch.arange(256, device=W.device)
    src = torch.arange(8, device=W.device)[None, :] ^ ((r >> 1) & 7)[:, None]    # position p holds chunk p ^ f(r)
    t = t[:, :, r[:, None], src]                                                  # gather chunks per row
    out = t.contiguous().reshape(N, K)
    out.lx_tiled = True
    return out


def untile_weight(Wt: torch.Tensor) -> torch.Tensor:
    """Inverse of tile_weight (the chunk XOR is an involution): the tiled image -> nn.Linear row-major [N,K]."""
    N, K = Wt.shape
    e = 16 // Wt.element_size()
    t = Wt.reshape(N // 256, K // (8 * e), 256, 8, e)
    r = torch.arange(256, device=Wt.device)
    src = torch.arange(8, device=Wt.device)[None, :] ^ ((r >> 1) & 7)[:, None]
    return t[:, :, r[:, None], src].permute(0, 2, 1, 3, 4).contiguous().reshape(N, K)


def quantize_weight_fp8(W: torch.Tensor):
    """bf16 / fp32 [N,K] (row-major) -> (e4m3 bytes [N,K] uint8, row_descale [N] fp32): row n is stored as e4m3(W[n] * s_n) with
    s_n = 448 / max|W[n]| (per-output-channel scale, folded into the GEMM's col_scale), row_descale = 1 / s_n."""
    Wf = W.float()
    amax = Wf.abs().amax(dim=1).clamp_min(1e-12)
    s = 448.0 / amax
    W8 = (Wf * s[:, None]).clamp(-448.0, 448.0).to(torch.float8_e4m3fn).view(torch.uint8).contiguous()
    return W8, (1.0 / s).contiguous()


def gemm_desc(A: torch.Tensor, W: torch.Tensor, C_: torch.Tensor, *, bias=None, epilogue=LX_EPI_STORE_BF16,
              gate=None, rows_per_batch=None, lora_t=None, lora_up=None, lora_mod_cols=0, lora_toff_max=0,
              gelu_col_start=0, M=None, N=None, K=None, lora_nsplit=1, lora_split_stride=0, k_segs=0, a_lo_off=0,
              c_lo_off=0, fp8=False, col_scale=None, out_scale=0.0, qkv=None, f16=False, f16_ovf=None) -> GemmDesc:
    """A [M,K] bf16 (row stride A.stride(0)), W [N,K] bf16, C_ [M,N] bf16|fp32 (strided views welcome).
    Precise mode: k_segs = 2 | 3 with A's lo image a_lo_off columns after the hi image (pass K explicitly: A then has more than K
    columns) and, for 3, W = [N, 2K] = [W_hi | W_lo] (pass N, K); c_lo_off != 0 adds LX_EPI_SPLIT_BF16 (hi/lo output pair)."""
    if fp8:      # e4m3 byte operands (LX_OPERANDS_FP8): acc * col_scale[n] first, then the usual epilogue
        _req(A, torch.uint8, "A"); _req(W, torch.uint8, "W")
        epilogue |= LX_OPERANDS_FP8
    elif f16:    # IEEE fp16 operands (LX_OPERANDS_F16): a 16-bit store writes fp16 too (saturated; f16_ovf = int32 device counter of clipping waves)
        _req(A, torch.float16, "A"); _req(W, torch.float16, "W")
        assert col_scale is None and not k_segs and not c_lo_off
        epilogue |= LX_OPERANDS_F16
        if f16_ovf is not None:
            _req(f16_ovf, torch.int32, "f16_ovf")
            col_scale = f16_ovf                       # (one pointer slot for the two operand modes: a union in lx.h)
    else:
        _req(A, torch.bfloat16, "A"); _req(W, torch.bfloat16, "W")
    d = GemmDesc()
    d.A, d.W, d.C = A.data_ptr(), W.data_ptr(), C_.data_ptr()
    d.bias = _p(bias)
    d.M = A.shape[0] if M is None else M
    d.K = A.shape[1] if K is None else K
    d.N = W.shape[0] if N is None else N
    d.lda, d.ldw, d.ldc = A.stride(0), W.stride(0), C_.stride(0)
    d.rows_per_batch = d.M if rows_per_batch is None else rows_per_batch
    d.gate = _p(gate)
    d.gate_ld = gate.stride(0) if gate is not None else 0
    d.lora_t, d.lora_up = _p(lora_t), _p(lora_up)
    if lora_t is not None:
        d.lora_r, d.lora_ldt = lora_up.shape[1], lora_t.stride(0)
    d.lora_mod_cols, d.lora_toff_max = lora_mod_cols, lora_toff_max
    d.lora_nsplit, d.lora_split_stride = lora_nsplit, lora_split_stride
    d.k_segs, d.a_lo_off, d.c_lo_off = k_segs, a_lo_off, c_lo_off
    if c_lo_off:
        epilogue |= LX_EPI_SPLIT_BF16
    if getattr(W, "lx_tiled", False):
        epilogue |= LX_W_TILED
    d.epilogue, d.gelu_col_start = epilogue, gelu_col_start
    d.col_scale, d.out_scale = _p(col_scale), float(out_scale)
    if qkv is not None:
        # LX_EPI_QKV: the first 3 * d columns are [k | v | q]; RMSNorm + RoPE on k / q and the V^T image come out of the epilogue
        # qkv = dict(norm_q=[128] f32, norm_k=[128] f32, rope=[rows_per_batch, 128] f32 (cos, sin) pairs, vt=V^T image,
        #            vt_pos0=first slot of this stream in a V^T row, d=inner dim)
        _req(qkv["norm_q"], torch.float32, "qkv.norm_q"); _req(qkv["norm_k"], torch.float32, "qkv.norm_k")
        f8 = qkv.get("q8") is not None      # e4m3 images for lx_attn_fwd_fp8 instead of the bf16 outputs
        _req(qkv["vt"], torch.uint8 if f8 else torch.bfloat16, "qkv.vt")
        rope = qkv["rope"]
        _req(rope, torch.float32, "qkv.rope")
        assert rope.is_contiguous() and rope.shape == (d.rows_per_batch, 128), (rope.shape, d.rows_per_batch)
        assert qkv["vt"].is_contiguous()
        d.qkv_norm_q, d.qkv_norm_k, d.qkv_rope = _p(qkv["norm_q"]), _p(qkv["norm_k"]), _p(rope)
        d.qkv_d, d.qkv_vt_ld, d.qkv_vt_pos0 = int(qkv["d"]), qkv["vt"].shape[-1], int(qkv["vt_pos0"])
        if f8:      # qkv = dict(..., q8=[M, ld8] u8, k8=[M, ld8] u8, vt=byte V^T image): the scales are the fp8 attention path's constants
            q8, k8 = qkv["q8"], qkv["k8"]
            _req(q8, torch.uint8, "qkv.q8"); _req(k8, torch.uint8, "qkv.k8")
            assert q8.shape[0] == d.M and k8.shape[0] == d.M and q8.stride(0) == k8.stride(0) and q8.stride(1) == 1 and k8.stride(1) == 1
            d.qkv_q8, d.qkv_k8, d.qkv_vt8, d.qkv_ld8 = q8.data_ptr(), k8.data_ptr(), qkv["vt"].data_ptr(), q8.stride(0)
            d.qkv_q_scale, d.qkv_k_scale, d.qkv_v_scale = FP8_Q_SCALE, FP8_K_SCALE, FP8_V_SCALE
        else:
            d.qkv_vt = _p(qkv["vt"])
        d.epilogue = epilogue = epilogue | LX_EPI_QKV
        kimg = qkv.get("k")                 # optional separate key image [M, ld]
        if kimg is not None:
            _req(kimg, torch.bfloat16, "qkv.k")
            assert kimg.shape[0] == d.M and kimg.stride(1) == 1
            d.qkv_k, d.qkv_k_ld = kimg.data_ptr(), kimg.stride(0)
        d._keep = (qkv["norm_q"], qkv["norm_k"], rope, qkv["vt"], kimg, qkv.get("q8"), qkv.get("k8"))     # the descriptor holds raw pointers: keep temporaries alive until launch
    kind = epilogue & 0xff
    want = torch.bfloat16 if kind == LX_EPI_STORE_BF16 else (torch.uint8 if kind == LX_EPI_STORE_FP8 else torch.float32)
    if f16 and kind == LX_EPI_STORE_BF16 and qkv is None:
        want = torch.float16                          # (with LX_EPI_QKV the buffer holds bf16 k / q beside fp16 columns: either view passes)
    if not (f16 and qkv is not None and kind == LX_EPI_STORE_BF16 and C_.dtype in (torch.float16, torch.bfloat16)):
        _req(C_, want, "C")
    return d


class LaunchTimer:
    """Brackets selected kernel launches with HIP events on the launch stream (bench.py roofline measurement).
    Events cannot be recorded inside a replayed graph, so a bracketed denoise step runs the eager launch path (~2 % slower
    than the replay). `only_calls` limits that to the given DiTEngine.forward calls (0-based, counted while this timer is
    installed as ops.TIMER); every other call replays the captured graph and `active` is False."""

    def __init__(self, only_calls=None):
        self.records = {}   # kind -> list of (start_event, end_event, algorithmic_flops)
        self.bytes = {}     # kind -> algorithmic operand + output bytes summed over the bracketed launches
        self.only_calls = None if only_calls is None else set(only_calls)
        self.calls = 0
        self.active = only_calls is None

    def next_call(self) -> bool:
        """DiTEngine.forward asks once per call: bracket (and therefore run eagerly) this one?"""
        self.active = self.only_calls is None or self.calls in self.only_calls
        self.calls += 1
        return self.active

    def bracket(self, kind: str, flops: float, nbytes: float = 0.0):
        s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        self.records.setdefault(kind, []).append((s, e, flops))
        self.bytes[kind] = self.bytes.get(kind, 0.0) + nbytes
        return s, e

    def summary(self):
        """kind -> dict(launches, flops, ms) ; call after torch.cuda.synchronize()."""
        out = {}
        for kind, recs in self.records.items():
            ms = sum(s.elapsed_time(e) for s, e, _ in recs)
            out[kind] = dict(launches=len(recs), flops=sum(f for _, _, f in recs), ms=ms, bytes=self.bytes.get(kind, 0.0))
        return out


TIMER: Optional[LaunchTimer] = None


def _timed(kind: str, cost, call) -> None:
    """Run `call` (one launch), between two events when a timer is installed and active for this forward call.
    cost() -> (algorithmic flops, operand + output bytes): worked out only for a bracketed launch."""
    if TIMER is None or not TIMER.active:
        return call()
    s, e = TIMER.bracket(kind, *cost())
    s.record()
    call()
    e.record()


def _attn_cost(B, H, q_rows, S):
    return lambda: (4.0 * B * H * q_rows * S * 128, 0.0)


def gemm_workspace(device) -> torch.Tensor:
    """Zero-filled scratch for lx_gemm_bf16_ws (split-K pair plan): one per stream / engine, owned by the caller."""
    return torch.zeros(lib.lx_gemm_workspace_bytes(), dtype=torch.uint8, device=device)


def gemm_workspace_status(ws: torch.Tensor) -> None:
    """Synchronises the current stream; raises LxError if a pair-plan workgroup timed out since the last check."""
    check(lib.lx_gemm_workspace_status(ws.data_ptr(), _stream()), "lx_gemm_workspace_status")


def gemm(problems: Sequence[GemmDesc], workspace: Optional[torch.Tensor] = None) -> None:
    n = len(problems)
    arr = (GemmDesc * n)(*problems)
    if workspace is not None:
        call = lambda: check(lib.lx_gemm_bf16_ws(arr, n, workspace.data_ptr(), workspace.numel(), _stream()), "lx_gemm_bf16_ws")
    else:
        call = lambda: check(lib.lx_gemm_bf16(arr, n, _stream()), "lx_gemm_bf16")

    def _bytes(p):   # each operand read once, the output written once (the fp32 residual epilogue also reads it)
        epi = p.epilogue & 0xff
        out_b = 2 if epi == LX_EPI_STORE_BF16 else (8 if epi == LX_EPI_RESID_F32 else 4)
        return 2.0 * p.M * p.K + 2.0 * p.N * p.K + float(out_b) * p.M * p.N
    _timed("gemm", lambda: (sum(2.0 * p.M * p.N * p.K for p in problems), sum(_bytes(p) for p in problems)), call)


def gemm_last_plan() -> int:
    """The launch plan of this thread's last successful gemm() (an LX_GEMM_PLAN_* value, include/lx.h)."""
    return lib.lx_gemm_last_plan()


def lora_down(X: torch.Tensor, Adown: torch.Tensor, T: torch.Tensor, n_split: int = 1, split_stride: int = 0) -> None:
    """T (slab 0) [M,R] fp32; with n_split > 1 slab s lives split_stride floats further (same row stride).
    X and Adown both bf16, or both fp16 (the operand images of the fp16-operand mode: lx_lora_down_f16)."""
    _req(T, torch.float32, "T")
    dt, nm = (torch.float16, "lx_lora_down_f16") if X.dtype == torch.float16 else (torch.bfloat16, "lx_lora_down")
    _req(X, dt, "X"); _req(Adown, dt, "Adown")
    check(getattr(lib, nm)(X.data_ptr(), X.stride(0), Adown.data_ptr(), T.data_ptr(), T.stride(0), X.shape[0], X.shape[1],
                           Adown.shape[0], n_split, split_stride, _stream()), nm)


def lora_down_terms(terms, T: torch.Tensor, slab_stride: int) -> None:
    """terms: [(X [M,K] bf16, Adown [R,K] bf16), ...] (<= 4); slab s of T (fp32, slab_stride floats apart) = X_s . Adown_s^T: one launch."""
    n = len(terms)
    M, K = terms[0][0].shape
    R = terms[0][1].shape[0]
    xs, ls, as_ = (C.c_void_p * n)(), (C.c_int * n)(), (C.c_void_p * n)()
    for i, (x, a) in enumerate(terms):
        _req(x, torch.bfloat16, "X"); _req(a, torch.bfloat16, "Adown")
        assert x.shape == (M, K) and a.shape == (R, K) and a.is_contiguous() and x.stride(1) == 1
        xs[i], ls[i], as_[i] = x.data_ptr(), x.stride(0), a.data_ptr()
    _req(T, torch.float32, "T")
    check(lib.lx_lora_down_terms(xs, ls, as_, n, T.data_ptr(), T.stride(0), M, K, R, slab_stride, _stream()), "lx_lora_down_terms")


def lora_scale_rows(T: torch.Tensor, segs, W: torch.Tensor, period: int, n_slab: int = 1, slab_stride: int = 0) -> None:
    """T[row, c] *= W[b, c % period] on every slab of the adapter scratch (slab 0 = T [rows, R] fp32, row stride T.stride(0); slab s lives
    slab_stride floats further), for the rows of segs = [(row0, n_rows, rows_per_batch), ...] (<= 3), b = ((row - row0) // rows_per_batch)
    % W.shape[0]. W fp32 [n_batches, >= min(period, R)]: the engine's per-image adapter-weight table. One launch."""
    _req(T, torch.float32, "T"); _req(W, torch.float32, "W")
    assert T.dim() == 2 and W.dim() == 2 and T.stride(1) == 1 and W.stride(1) == 1
    arr = (L.RowScaleSeg * max(len(segs), 1))()
    for i, (row0, n_rows, rpb) in enumerate(segs):
        arr[i].row0, arr[i].n_rows, arr[i].rows_per_batch = row0, n_rows, rpb
    R, rows = T.shape[1], sum(s[1] for s in segs)
    _timed("lora_scale", lambda: (float(rows * R * n_slab), 8.0 * rows * R * n_slab),
           lambda: check(lib.lx_lora_scale_rows(T.data_ptr(), T.stride(0), R, n_slab, slab_stride, arr, len(segs), W.data_ptr(), W.stride(0),
                                                W.shape[0], period, _stream()), "lx_lora_scale_rows"))


def linear_skinny(X, W, bias, Y, act_in=0, act_out=0, accumulate=False) -> None:
    _req(X, torch.float32, "X"); _req(W, torch.bfloat16, "W"); _req(Y, torch.float32, "Y")
    check(lib.lx_linear_skinny(X.data_ptr(), X.stride(0), W.data_ptr(), W.stride(0), _p(bias), Y.data_ptr(), Y.stride(0),
                               X.shape[0], W.shape[0], W.shape[1], act_in, act_out, int(accumulate), _stream()), "lx_linear_skinny")


def timestep_embed(t: torch.Tensor, out: torch.Tensor) -> None:
    _req(t, torch.float32, "t"); _req(out, torch.float32, "out")
    check(lib.lx_timestep_embed(t.data_ptr(), out.data_ptr(), out.shape[0], out.shape[1], _stream()), "lx_timestep_embed")


def rope_table(ids: torch.Tensor, axes=(16, 56, 56), theta: float = 10000.0, out=None):
    """ids fp32 [L,3] on the GPU -> (cos, sin) fp32 [L, sum(axes)] (written into `out=(cos, sin)` when given)."""
    _req(ids, torch.float32, "ids")
    ids = ids.contiguous()
    Lq, tot = ids.shape[0], sum(axes)
    if out is None:
        cos = torch.empty(Lq, tot, dtype=torch.float32, device=ids.device)
        sin = torch.empty_like(cos)
    else:
        cos, sin = out
        assert cos.shape == (Lq, tot) and sin.shape == (Lq, tot) and cos.is_contiguous() and sin.is_contiguous()
    check(lib.lx_rope_table(ids.data_ptr(), Lq, axes[0], axes[1], axes[2], float(theta), cos.data_ptr(), sin.data_ptr(), _stream()), "lx_rope_table")
    return cos, sin


def _ln_segs(segs):
    """[(row0, n_rows, rows_per_batch, shift_tensor, scale_tensor), ...] -> lx_ln_seg[len(segs)]"""
    arr = (L.LnSeg * len(segs))()
    for i, (row0, n_rows, rpb, sh, sc) in enumerate(segs):
        arr[i].row0, arr[i].n_rows, arr[i].rows_per_batch = row0, n_rows, rpb
        arr[i].shift, arr[i].scale = sh.data_ptr(), sc.data_ptr()
    return arr


def _qkv_segs(segs, vt=True):
    """[(row0, rows_per_batch, vt_pos0, wq, wk, cos, sin), ...] -> lx_qkv_seg[len(segs)]; vt=False: no V^T image, vt_pos0 = 0"""
    arr = (L.QkvSeg * len(segs))()
    for i, (row0, rpb, vt0, wq, wk, cos, sin) in enumerate(segs):
        arr[i].row0, arr[i].rows_per_batch, arr[i].vt_pos0 = row0, rpb, vt0 if vt else 0
        arr[i].wq, arr[i].wk, arr[i].cos_tab, arr[i].sin_tab = _p(wq), _p(wk), _p(cos), _p(sin)
    return arr


def _fill_bias(d, bias) -> None:
    """the 3 x 3 (query segment, key segment) additive bias table of an attention descriptor; None: zeros"""
    for i in range(3):
        for j in range(3):
            d.bias[i][j] = 0.0 if bias is None else float(bias[i][j])


def ln_modulate(X, shift, scale, Y, rows_per_batch, eps=1e-6, mod_ld=None, f16_ovf=None) -> None:
    _req(X, torch.float32, "X"); _req(shift, torch.float32, "shift"); _req(scale, torch.float32, "scale")
    if Y.dtype == torch.float16:          # the fp16 operand image: the one-segment form of lx_ln_modulate_f16_segs
        return ln_modulate_segs(X, [(0, X.shape[0], rows_per_batch, shift, scale)], Y, shift.stride(0) if mod_ld is None else mod_ld, eps, f16_ovf=f16_ovf)
    _req(Y, torch.bfloat16, "Y")
    check(lib.lx_ln_modulate(X.data_ptr(), X.stride(0), shift.data_ptr(), scale.data_ptr(),
                             shift.stride(0) if mod_ld is None else mod_ld, Y.data_ptr(), Y.stride(0), X.shape[0], X.shape[1],
                             rows_per_batch, eps, _stream()), "lx_ln_modulate")


def ln_modulate_delta(X, shift, scale, P, rows_per_batch, row_sums, sums, eps=1e-6, mod_ld=None) -> None:
    """The step-cache probe (lx_ln_modulate_delta): m = LN(X) * (1 + scale) + shift in fp32, row_sums[row] = (sum |m - P|, sum |P|) against
    P as found, then P = m; sums (float64 [2]) = the row pairs added in row order. X, P fp32 [M, D] (row strides free), row_sums fp32
    [M, 2] contiguous."""
    _req(X, torch.float32, "X"); _req(shift, torch.float32, "shift"); _req(scale, torch.float32, "scale"); _req(P, torch.float32, "P")
    _req(row_sums, torch.float32, "row_sums"); _req(sums, torch.float64, "sums")
    assert P.shape == X.shape and row_sums.is_contiguous() and row_sums.numel() >= 2 * X.shape[0] and sums.is_contiguous() and sums.numel() >= 2
    check(lib.lx_ln_modulate_delta(X.data_ptr(), X.stride(0), shift.data_ptr(), scale.data_ptr(),
                                   shift.stride(0) if mod_ld is None else mod_ld, P.data_ptr(), P.stride(0), X.shape[0], X.shape[1],
                                   rows_per_batch, eps, row_sums.data_ptr(), sums.data_ptr(), _stream()), "lx_ln_modulate_delta")


def qkv_prep(QKV, q_col, k_col, v_col, row0, n_rows, rows_per_batch, H, wq, wk, cos, sin, VT, vt_pos0, eps=1e-6) -> None:
    _req(QKV, torch.bfloat16, "QKV")
    check(lib.lx_qkv_prep(QKV.data_ptr(), QKV.stride(0), q_col, k_col, v_col, row0, n_rows, rows_per_batch, H, _p(wq), _p(wk), eps,
                          _p(cos), _p(sin), _p(VT), VT.shape[-1] if VT is not None else 0, vt_pos0, _stream()), "lx_qkv_prep")


def ln_modulate_segs(X, segs, Y, mod_ld, eps=1e-6, lora=None, f16_ovf=None) -> None:
    """segs: list of (row0, n_rows, rows_per_batch, shift_tensor, scale_tensor); one launch. Y bf16, or fp16 (the A operand of an
    fp16-operand GEMM: saturated, f16_ovf = int32 device counter of the rows that clipped).
    lora = (Adown [R, D] in Y's 16-bit format, T [rows, >= R] fp32 (row stride T.stride(0)), first row, row count): also the LoRA
    down-projection of those rows of Y, T[row - first] = Y_row . Adown^T, on the matrix pipe inside the same launch (what
    lora_down(Y[first:first+count], Adown, T) computes; D = 3072 | 256)."""
    f16 = Y.dtype == torch.float16
    nm, extra = "lx_ln_modulate" + ("_lora" if lora is not None else "") + ("_f16" if f16 else "") + "_segs", ()
    if lora is not None:
        A, T, r0, cnt = lora
        _req(A, torch.float16 if f16 else torch.bfloat16, "Adown"); _req(T, torch.float32, "T")
        assert A.is_contiguous() and A.shape[1] == X.shape[1] and T.shape[0] >= cnt and T.stride(1) == 1
        extra = (A.data_ptr(), A.shape[0], T.data_ptr(), T.stride(0), r0, cnt)
    if f16:
        extra += (_p(f16_ovf),)
    check(getattr(lib, nm)(X.data_ptr(), X.stride(0), _ln_segs(segs), len(segs), mod_ld, Y.data_ptr(), Y.stride(0), X.shape[1], eps, *extra, _stream()), nm)


def qkv_prep_segs(QKV, q_col, k_col, v_col, segs, n_batches, H, VT, eps=1e-6, in_f16=False) -> None:
    """segs: list of (row0, rows_per_batch, vt_pos0, wq, wk, cos, sin); one launch. in_f16: the q / k / v columns hold IEEE fp16 (the 16-bit
    store of an fp16-operand projection without the fused epilogue); q / k are written back as bf16, V^T as bf16 either way."""
    fn, nm = (lib.lx_qkv_prep_f16in_segs, "lx_qkv_prep_f16in_segs") if in_f16 else (lib.lx_qkv_prep_segs, "lx_qkv_prep_segs")
    check(fn(QKV.data_ptr(), QKV.stride(0), q_col, k_col, v_col, _qkv_segs(segs), len(segs), n_batches, H, eps, _p(VT), VT.shape[-1] if VT is not None else 0, _stream()), nm)


def qkv_prep_kv_segs(QKV, q_col, k_col, v_col, segs, n_batches, H, K2, k2_col, VT, eps=1e-6, in_f16=False) -> None:
    """qkv_prep_segs with the keys in an image of their own: q in place, k (bf16) into the same rows of K2 bf16 [M, ldk2] at k2_col + h*128
    (the k columns of QKV stay as they are), V^T into VT. Rows and V^T tiles of segments that are not in `segs` stay as they are."""
    _req(K2, torch.bfloat16, "K2"); _req(VT, torch.bfloat16, "VT")
    assert K2.stride(1) == 1 and VT.is_contiguous()
    fn, nm = (lib.lx_qkv_prep_kv_f16in_segs, "lx_qkv_prep_kv_f16in_segs") if in_f16 else (lib.lx_qkv_prep_kv_segs, "lx_qkv_prep_kv_segs")
    check(fn(QKV.data_ptr(), QKV.stride(0), q_col, k_col, v_col, _qkv_segs(segs), len(segs), n_batches, H, eps, K2.data_ptr(), K2.stride(0), k2_col,
             VT.data_ptr(), VT.shape[-1], _stream()), nm)


def _attn_desc(Q, K, VT, O, q_col, k_col, o_col, B, H, seg_row0, seg_len, seg_vt0, bias, scale):
    d = AttnDesc()
    d.Q, d.K, d.VT, d.O = Q.data_ptr(), K.data_ptr(), VT.data_ptr(), O.data_ptr()
    d.ldq, d.ldk, d.ldo, d.vt_ld = Q.stride(0), K.stride(0), O.stride(0), VT.shape[-1]
    d.q_col, d.k_col, d.o_col, d.B, d.H, d.n_seg = q_col, k_col, o_col, B, H, len(seg_len)
    for i in range(len(seg_len)):
        d.seg_row0[i], d.seg_len[i], d.seg_vt0[i] = seg_row0[i], seg_len[i], seg_vt0[i]
    _fill_bias(d, bias)
    d.scale = (1.0 / math.sqrt(128.0)) if scale is None else scale
    return d


ATTN_Q_LOG2, ATTN_BOUNDED, ATTN_INVARIANT, ATTN_O_F16, ATTN_PREFER_4WAVE, ATTN_P_EXP2 = (L.LX_ATTN_Q_LOG2, L.LX_ATTN_BOUNDED, L.LX_ATTN_INVARIANT, L.LX_ATTN_O_F16,
                                                                                         L.LX_ATTN_PREFER_4WAVE, L.LX_ATTN_P_EXP2)
Q_LOG2_FACTOR = (1.0 / math.sqrt(128.0)) * 1.4426950408889634       # what LX_ATTN_Q_LOG2 expects q to carry already


def _q_rows(seg_len, n_qseg, qseg_mask):
    if qseg_mask:
        return sum(L_ for i, L_ in enumerate(seg_len) if (qseg_mask >> i) & 1)
    return sum(seg_len[:n_qseg]) if n_qseg else sum(seg_len)


def attn_fwd(Q, K, VT, O, *, q_col, k_col, o_col, B, H, seg_row0, seg_len, seg_vt0, bias=None, scale=None, n_qseg=0, flags=0, f16_ovf=None,
             qseg_mask=0) -> None:
    """n_qseg = k > 0: only the first k segments have queries (all segments still serve keys / values); qseg_mask != 0: exactly the
    segments whose bit is set (any subset).
    flags: ATTN_Q_LOG2 [| ATTN_BOUNDED] (include/lx.h): q carries scale * log2 e; the caller bounds the scores -> no running max."""
    d = _attn_desc(Q, K, VT, O, q_col, k_col, o_col, B, H, seg_row0, seg_len, seg_vt0, bias, scale)
    d.n_qseg = n_qseg
    d.flags = flags
    d.qseg_mask = qseg_mask
    d.f16_ovf = _p(f16_ovf)               # (ATTN_O_F16: O is written as fp16, saturated; int32 device counter of clipping waves)
    _timed("attn", _attn_cost(B, H, _q_rows(seg_len, n_qseg, qseg_mask), sum(seg_len)), lambda: check(lib.lx_attn_fwd(C.byref(d), _stream()), "lx_attn_fwd"))


# ---- attention under a caller's mask (include/lx.h lx_attn_fwd_masked) ------------------------------------------------------------
_MASK_DTYPES = {torch.bool: L.LX_ATTN_MASK_BOOL, torch.float32: L.LX_ATTN_MASK_F32, torch.bfloat16: L.LX_ATTN_MASK_BF16,
                torch.float16: L.LX_ATTN_MASK_F16}


def _mask_desc(mask: torch.Tensor, workspace: Optional[torch.Tensor]) -> "L.AttnMaskDesc":
    """mask: [Bm, Hm, Sq, Sk] (rank 2 / 3: leading dims of size 1 added), any strides, bool or fp32 / bf16 / fp16 additive"""
    if mask.dtype not in _MASK_DTYPES:
        raise TypeError(f"attention mask: dtype {mask.dtype} is not one of bool, float32, bfloat16, float16")
    if not mask.is_cuda:
        raise ValueError("attention mask: must live on the GPU (the hot path has no CPU fallback)")
    if not 2 <= mask.dim() <= 4:
        raise ValueError(f"attention mask: rank {mask.dim()} (expected 2..4)")
    while mask.dim() < 4:
        mask = mask.unsqueeze(0)
    m = L.AttnMaskDesc()
    m.mask, m.dtype = mask.data_ptr(), _MASK_DTYPES[mask.dtype]
    for i in range(4):
        m.dims[i], m.strides[i] = mask.shape[i], mask.stride(i)
    if workspace is not None:
        m.workspace, m.workspace_bytes = workspace.data_ptr(), workspace.numel() * workspace.element_size()
    return m


def _seg_desc(B, H, seg_len, seg_vt0, bias) -> AttnDesc:
    d = AttnDesc()
    d.B, d.H, d.n_seg = B, H, len(seg_len)
    for i in range(len(seg_len)):
        d.seg_len[i], d.seg_vt0[i] = seg_len[i], seg_vt0[i]
    _fill_bias(d, bias)
    return d


def attn_mask_workspace_bytes(mask, *, B, H, seg_len, seg_vt0, bias=None) -> int:
    """The bytes lx_attn_mask_workspace asks for this mask shape / dtype and these segments."""
    d, m = _seg_desc(B, H, seg_len, seg_vt0, bias), _mask_desc(mask, None)
    n = C.c_size_t(0)
    check(lib.lx_attn_mask_workspace(C.byref(d), C.byref(m), C.byref(n)), "lx_attn_mask_workspace")
    return int(n.value)


def attn_mask_workspace(mask, *, B, H, seg_len, seg_vt0, bias=None, device=None) -> torch.Tensor:
    """A workspace (uint8 tensor) of that size."""
    n = attn_mask_workspace_bytes(mask, B=B, H=H, seg_len=seg_len, seg_vt0=seg_vt0, bias=bias)
    return torch.empty(max(n, 1), dtype=torch.uint8, device=device if device is not None else mask.device)


def attn_mask_prep(mask, workspace, *, B, H, seg_len, seg_vt0, bias=None) -> None:
    """Read `mask` once into `workspace` (tile classes, per-query-tile lists of non-EMPTY key tiles, row bits / biases) for
    attn_fwd_masked(..., prepped=True) with the same segments and mask shape."""
    d, m = _seg_desc(B, H, seg_len, seg_vt0, bias), _mask_desc(mask, workspace)
    check(lib.lx_attn_mask_prep(C.byref(d), C.byref(m), _stream()), "lx_attn_mask_prep")


def attn_fwd_masked(Q, K, VT, O, mask, *, q_col, k_col, o_col, B, H, seg_row0, seg_len, seg_vt0, bias=None, scale=None, flags=0,
                    f16_ovf=None, workspace=None, prepped=False, n_qseg=0, qseg_mask=0) -> torch.Tensor:
    """attn_fwd under a per-(query, key) mask over the concatenated segments (SDPA's attn_mask: bool = attend, float = additive,
    -inf masks); flags: 0 | ATTN_Q_LOG2 | ATTN_O_F16; n_qseg / qseg_mask as in attn_fwd (the mask still spans every segment). Runs
    lx_attn_mask_prep first unless `prepped` (the workspace then holds what an attn_mask_prep of the same mask wrote). Returns the
    workspace."""
    if workspace is None:
        workspace = attn_mask_workspace(mask, B=B, H=H, seg_len=seg_len, seg_vt0=seg_vt0, bias=bias, device=Q.device)
    d = _attn_desc(Q, K, VT, O, q_col, k_col, o_col, B, H, seg_row0, seg_len, seg_vt0, bias, scale)
    d.flags, d.f16_ovf, d.n_qseg, d.qseg_mask = flags, _p(f16_ovf), n_qseg, qseg_mask
    m = _mask_desc(mask, workspace)
    if not prepped:
        check(lib.lx_attn_mask_prep(C.byref(d), C.byref(m), _stream()), "lx_attn_mask_prep")
    _timed("attn", _attn_cost(B, H, _q_rows(seg_len, n_qseg, qseg_mask), sum(seg_len)),
           lambda: check(lib.lx_attn_fwd_masked(C.byref(d), C.byref(m), _stream()), "lx_attn_fwd_masked"))
    return workspace


# fp8 (e4m3) attention path: fixed operand scales. q and k are RMS-normalised (|x| <= sqrt(128) * |w|), so 16 keeps them inside
# e4m3's normal range [2^-6, 448] with headroom; v is a raw projection output and is stored unscaled (clamped to +-448).
# q scale: chosen so that (1/sqrt(128)) x log2(e) / (q scale x k scale) = 2^-11 exactly -- the attention kernel then applies the whole
# factor as an MX block scale of its score MFMAs (attn.hip, lx_attn_fp8_pipe_kernel POW2); 16.32 instead of 16
FP8_K_SCALE, FP8_V_SCALE = 16.0, 1.0
FP8_Q_SCALE = 2048.0 * (1.0 / math.sqrt(128.0)) * 1.4426950408889634 / FP8_K_SCALE


def qkv_prep_fp8_segs(QKV, q_col, k_col, v_col, segs, n_batches, H, Q8, K8, VT8, eps=1e-6, in_f16=False) -> None:
    """segs as in qkv_prep_segs; Q8 / K8: uint8 [rows, H*128]; VT8: uint8 [B, H, 128, Spad]. The 16-bit QKV buffer (bf16, or fp16 with
    in_f16) is not modified."""
    fn, nm = (lib.lx_qkv_prep_fp8_f16in_segs, "lx_qkv_prep_fp8_f16in_segs") if in_f16 else (lib.lx_qkv_prep_fp8_segs, "lx_qkv_prep_fp8_segs")
    check(fn(QKV.data_ptr(), QKV.stride(0), q_col, k_col, v_col, _qkv_segs(segs), len(segs), n_batches, H, eps, Q8.data_ptr(), K8.data_ptr(), Q8.stride(0),
             VT8.data_ptr(), VT8.shape[-1], FP8_Q_SCALE, FP8_K_SCALE, FP8_V_SCALE, _stream()), nm)


def attn_fwd_fp8(Q8, K8, VT8, O, *, o_col, B, H, seg_row0, seg_len, seg_vt0, bias=None, scale=None, flags=0, f16_ovf=None, qseg_mask=0,
                 n_qseg=0) -> None:
    """flags: 0 | ATTN_O_F16 (O written as fp16 for an fp16-operand output projection) | ATTN_P_EXP2 (probabilities by v_exp_f32 + e4m3
    rounding instead of the log-linear byte code of the score); n_qseg / qseg_mask as in attn_fwd. K8 / VT8 may be images other than the
    one Q8 sits in (the per-layer images of the condition cache)."""
    d = _attn_desc(Q8, K8, VT8, O, 0, 0, o_col, B, H, seg_row0, seg_len, seg_vt0, bias, scale)
    d.flags, d.f16_ovf, d.qseg_mask, d.n_qseg = flags, _p(f16_ovf), qseg_mask, n_qseg
    args = (C.byref(d), 1.0 / (FP8_Q_SCALE * FP8_K_SCALE), 1.0 / FP8_V_SCALE, _stream())
    _timed("attn", _attn_cost(B, H, _q_rows(seg_len, n_qseg, qseg_mask), sum(seg_len)), lambda: check(lib.lx_attn_fwd_fp8(*args), "lx_attn_fwd_fp8"))


# ---- fp8 GEMM path (include/lx.h "fp8 GEMM path") ----------------------------------------------------------------------
def ln_modulate_fp8_segs(X, segs, Y, Y8, mod_ld, y8_scale, eps=1e-6) -> None:
    """segs as in ln_modulate_segs; Y bf16 (or None) and Y8 uint8 (e4m3 of y * y8_scale), same row indexing."""
    check(lib.lx_ln_modulate_fp8_segs(X.data_ptr(), X.stride(0), _ln_segs(segs), len(segs), mod_ld, _p(Y), Y.stride(0) if Y is not None else 0, Y8.data_ptr(),
                                      Y8.stride(0), float(y8_scale), X.shape[1], eps, _stream()), "lx_ln_modulate_fp8_segs")


def convert_fp8(src: torch.Tensor, dst: torch.Tensor, scale: float) -> None:
    """src bf16 | fp32 [M,K] (row stride honoured) -> dst uint8 [M,K] = e4m3(src * scale)."""
    _req(dst, torch.uint8, "dst")
    check(lib.lx_convert_fp8(src.data_ptr(), int(src.dtype == torch.bfloat16), src.stride(0), dst.data_ptr(), dst.stride(0), float(scale),
                             src.shape[0], src.shape[1], _stream()), "lx_convert_fp8")


def lora_down_fp8(X8: torch.Tensor, x_descale: float, Adown: torch.Tensor, T: torch.Tensor, n_split: int = 1, split_stride: int = 0) -> None:
    _req(X8, torch.uint8, "X8"); _req(Adown, torch.bfloat16, "Adown"); _req(T, torch.float32, "T")
    check(lib.lx_lora_down_fp8(X8.data_ptr(), X8.stride(0), float(x_descale), Adown.data_ptr(), T.data_ptr(), T.stride(0), X8.shape[0], X8.shape[1],
                               Adown.shape[0], n_split, split_stride, _stream()), "lx_lora_down_fp8")


# ---- precise mode (include/lx.h "Precise mode") -----------------------------------------------------------------------
def split_bf16(src: torch.Tensor, dst: torch.Tensor, lo_off: int) -> None:
    """src fp32 [M,K] -> dst bf16 [M, >= lo_off + K]: hi at column k, lo at lo_off + k."""
    _req(src, torch.float32, "src"); _req(dst, torch.bfloat16, "dst")
    check(lib.lx_split_bf16(src.data_ptr(), src.stride(0), dst.data_ptr(), dst.stride(0), lo_off, src.shape[0], src.shape[1], _stream()),
          "lx_split_bf16")


def ln_modulate_split_segs(X, segs, Y, mod_ld, y_lo_off, eps=1e-6) -> None:
    check(lib.lx_ln_modulate_split_segs(X.data_ptr(), X.stride(0), _ln_segs(segs), len(segs), mod_ld, Y.data_ptr(), Y.stride(0), y_lo_off, X.shape[1], eps,
                                        _stream()), "lx_ln_modulate_split_segs")


def qkv_prep_f32_segs(QKV, q_col, k_col, segs, n_batches, H, eps=1e-6) -> None:
    """segs as in qkv_prep_segs (the vt_pos0 entry is ignored); QKV fp32 [M, ld], q / k normalised + rotated in place."""
    _req(QKV, torch.float32, "QKV")
    check(lib.lx_qkv_prep_f32_segs(QKV.data_ptr(), QKV.stride(0), q_col, k_col, _qkv_segs(segs, vt=False), len(segs), n_batches, H, eps, _stream()), "lx_qkv_prep_f32_segs")


def attn_fwd_f32(QKV, O, *, q_col, k_col, v_col, o_col, o_lo_off, B, H, seg_row0, seg_len, bias=None, scale=None) -> None:
    _req(QKV, torch.float32, "QKV"); _req(O, torch.bfloat16, "O")
    d = L.AttnF32Desc()
    d.QKV, d.ld, d.q_col, d.k_col, d.v_col = QKV.data_ptr(), QKV.stride(0), q_col, k_col, v_col
    d.O, d.ldo, d.o_col, d.o_lo_off = O.data_ptr(), O.stride(0), o_col, o_lo_off
    d.B, d.H, d.n_seg = B, H, len(seg_len)
    for i in range(len(seg_len)):
        d.seg_row0[i], d.seg_len[i] = seg_row0[i], seg_len[i]
    _fill_bias(d, bias)
    d.scale = (1.0 / math.sqrt(128.0)) if scale is None else scale
    _timed("attn", _attn_cost(B, H, sum(seg_len), sum(seg_len)), lambda: check(lib.lx_attn_fwd_f32(C.byref(d), _stream()), "lx_attn_fwd_f32"))


def qkv_prep_split_segs(QKV, q_col, k_col, v_col, segs, n_batches, H, QK2, q2_col, k2_col, lo_off, VT2, eps=1e-6) -> None:
    """segs as in qkv_prep_segs. QKV fp32 [M, ld] (raw projections) -> QK2 bf16 [M, ld2] (q / k after RMSNorm + RoPE as hi / lo pairs:
    hi at q2_col / k2_col + h*128, lo lo_off columns further) and VT2 bf16 [2, B, H, 128, Spad] (the hi and the lo V^T image)."""
    _req(QKV, torch.float32, "QKV"); _req(QK2, torch.bfloat16, "QK2"); _req(VT2, torch.bfloat16, "VT2")
    assert VT2.dim() == 5 and VT2.shape[0] == 2 and VT2.is_contiguous() and QK2.stride(1) == 1
    check(lib.lx_qkv_prep_split_segs(QKV.data_ptr(), QKV.stride(0), q_col, k_col, v_col, _qkv_segs(segs), len(segs), n_batches, H, eps, QK2.data_ptr(), QK2.stride(0),
                                     q2_col, k2_col, lo_off, VT2.data_ptr(), VT2.shape[-1], VT2.stride(0), _stream()), "lx_qkv_prep_split_segs")


def qkv_prep_split_kv_segs(QKV, q_col, k_col, v_col, segs, n_batches, H, Q2, q2_col, K2, k2_col, lo_off, VT2, eps=1e-6) -> None:
    """qkv_prep_split_segs with the key pair in an image of its own: q pairs into Q2 (hi at q2_col), k pairs into the same rows of K2
    bf16 [M, ldk] (hi at k2_col), both lo halves lo_off columns further; VT2 as there. Rows and V^T tiles of other segments stay as they are."""
    _req(QKV, torch.float32, "QKV"); _req(Q2, torch.bfloat16, "Q2"); _req(K2, torch.bfloat16, "K2"); _req(VT2, torch.bfloat16, "VT2")
    assert VT2.dim() == 5 and VT2.shape[0] == 2 and VT2.is_contiguous() and Q2.stride(1) == 1 and K2.stride(1) == 1
    check(lib.lx_qkv_prep_split_kv_segs(QKV.data_ptr(), QKV.stride(0), q_col, k_col, v_col, _qkv_segs(segs), len(segs), n_batches, H, eps, Q2.data_ptr(),
                                        Q2.stride(0), q2_col, K2.data_ptr(), K2.stride(0), k2_col, lo_off, VT2.data_ptr(), VT2.shape[-1], VT2.stride(0),
                                        _stream()), "lx_qkv_prep_split_kv_segs")


def attn_fwd_split(QK2, VT2, O, *, q_col, k_col, qk_lo_off, o_col, o_lo_off, B, H, seg_row0, seg_len, seg_vt0, bias=None, scale=None,
                   flags=0, K=None, VT=None, n_qseg=0, qseg_mask=0) -> None:
    """Precise-mode attention on the bf16 matrix pipe: q / k pairs in QK2 (hi at q_col / k_col, lo qk_lo_off columns further), the two V^T
    images in VT2 [2, B, H, 128, Spad]; O bf16 gets the output pair (hi at o_col, lo o_lo_off columns further).
    K / VT: the key pairs (bf16 [M, ldk], hi at k_col) / the V^T images ([2, B, H, 128, Spad]) when they live elsewhere (default: QK2 / VT2);
    n_qseg / qseg_mask as in attn_fwd."""
    K, VT = QK2 if K is None else K, VT2 if VT is None else VT
    _req(QK2, torch.bfloat16, "QK2"); _req(K, torch.bfloat16, "K"); _req(VT, torch.bfloat16, "VT"); _req(O, torch.bfloat16, "O")
    assert VT.dim() == 5 and VT.shape[0] == 2 and VT.is_contiguous()
    d = _attn_desc(QK2, K, VT, O, q_col, k_col, o_col, B, H, seg_row0, seg_len, seg_vt0, bias, scale)
    d.flags, d.n_qseg, d.qseg_mask = flags, n_qseg, qseg_mask
    args = (C.byref(d), qk_lo_off, VT.stride(0), o_lo_off, _stream())
    _timed("attn", _attn_cost(B, H, _q_rows(seg_len, n_qseg, qseg_mask), sum(seg_len)), lambda: check(lib.lx_attn_fwd_split(*args), "lx_attn_fwd_split"))


def euler_step(x: torch.Tensor, v: torch.Tensor, dsigma: float) -> None:
    _req(x, torch.float32, "x")
    check(lib.lx_euler_step(x.data_ptr(), v.data_ptr(), int(v.dtype == torch.bfloat16), float(dsigma), x.numel(), _stream()), "lx_euler_step")


def scale_noise(x0: torch.Tensor, z: torch.Tensor, sigma: float, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """out = sigma*z + (1 - sigma)*x0 (lx_scale_noise): fp32, contiguous, one shape; `out` is allocated when not given."""
    _req(x0, torch.float32, "x0"); _req(z, torch.float32, "z")
    out = torch.empty_like(x0, memory_format=torch.contiguous_format) if out is None else out
    _req(out, torch.float32, "out")
    assert x0.shape == z.shape == out.shape and x0.is_contiguous() and z.is_contiguous() and out.is_contiguous()
    check(lib.lx_scale_noise(out.data_ptr(), x0.data_ptr(), z.data_ptr(), float(sigma), out.numel(), _stream()), "lx_scale_noise")
    return out


def _step_operands(name: str, x, v, parts: int, inpaint, held: str, piece: str, also=()):
    """What the guided and blended steps check and marshal alike: x fp32 and v fp32 or bf16 hold `parts` parts of n elements (`held`: the
    refusal's wording), inpaint = (x0, z, m) or None is fp32 with n elements each (`piece`: the same), and everything, the entry's
    further tensors `also` included, is contiguous. -> (n, whether v is bf16, the addresses of x0, z and m: None, C's NULL, without inpaint)"""
    _req(x, torch.float32, "x")
    if v.dtype not in (torch.float32, torch.bfloat16):
        raise TypeError(f"v: expected float32 or bfloat16, got {v.dtype}")
    n = x.numel() // parts
    assert x.numel() == parts * n and v.numel() == parts * n, f"{name}: {held}"
    x0, z, m = (None, None, None) if inpaint is None else inpaint
    if inpaint is not None:
        _req(x0, torch.float32, "x0"); _req(z, torch.float32, "z"); _req(m, torch.float32, "m")
        assert x0.numel() == n and z.numel() == n and m.numel() == n, f"{name}: {piece}"
    assert all(t.is_contiguous() for t in (x, v, x0, z, m) + tuple(also) if t is not None), f"{name}: contiguous operands"
    return n, int(v.dtype == torch.bfloat16), (_p(x0), _p(z), _p(m))


def euler_step_blend(x: torch.Tensor, v: torch.Tensor, dsigma: float, x0: torch.Tensor, z: torch.Tensor, m: torch.Tensor, sigma_next: float) -> None:
    """x <- m*(x + dsigma*v) + (1 - m)*(sigma_next*z + (1 - sigma_next)*x0) in place (lx_euler_step_blend): x, x0, z, m fp32, v fp32 or
    bf16, all contiguous with x's element count."""
    n, bf16, blend = _step_operands("euler_step_blend", x, v, 1, (x0, z, m), *("one element count for all operands",) * 2)
    check(lib.lx_euler_step_blend(x.data_ptr(), v.data_ptr(), bf16, float(dsigma), *blend, float(sigma_next), n, _stream()), "lx_euler_step_blend")


def euler_step_cfg(x: torch.Tensor, v: torch.Tensor, dsigma: float, scale: float, inpaint=None, sigma_next: float = 0.0) -> None:
    """The step under true classifier-free guidance, in place (lx_euler_step_cfg): x fp32 and v fp32 or bf16 hold [positive; negative]
    halves of n elements each; both halves of x become x[:n] + dsigma * (vn + scale * (vp - vn)). inpaint = (x0, z, m), fp32 with n
    elements each: blended with the source at sigma_next as euler_step_blend does, once, for both halves. All contiguous."""
    n, bf16, blend = _step_operands("euler_step_cfg", x, v, 2, inpaint, "x and v hold two halves of one element count",
                                    "x0, z and m have the element count of one half")
    check(lib.lx_euler_step_cfg(x.data_ptr(), v.data_ptr(), bf16, float(dsigma), float(scale), *blend, float(sigma_next), n, _stream()),
          "lx_euler_step_cfg")


def euler_step_cfg3(x: torch.Tensor, v: torch.Tensor, dsigma: float, scale_brain: float, scale_text: float, inpaint=None,
                    sigma_next: float = 0.0) -> None:
    """The step under brain guidance nested in true classifier-free guidance, in place (lx_euler_step_cfg3): x fp32 and v fp32 or bf16 hold
    [full; text; negative] parts of n elements each; all three parts of x become x[:n] + dsigma * (vN + scale_text * (gb - vN)) with
    gb = vT + scale_brain * (vF - vT). inpaint = (x0, z, m), fp32 with n elements each: blended with the source at sigma_next as
    euler_step_blend does, once, for all parts. All contiguous."""
    n, bf16, blend = _step_operands("euler_step_cfg3", x, v, 3, inpaint, "x and v hold three parts of one element count",
                                    "x0, z and m have the element count of one part")
    check(lib.lx_euler_step_cfg3(x.data_ptr(), v.data_ptr(), bf16, float(dsigma), float(scale_brain), float(scale_text), *blend,
                                 float(sigma_next), n, _stream()), "lx_euler_step_cfg3")


def apg_workspace_bytes(n_images: int, elems: int) -> int:
    """bytes of euler_step_apg's workspace for parts of n_images images of elems elements (lx_apg_workspace_bytes)"""
    return int(lib.lx_apg_workspace_bytes(int(n_images), int(elems)))


def euler_step_apg(x: torch.Tensor, v: torch.Tensor, sigma: float, dsigma: float, scales, eta: float, norm_threshold: float, momentum: float,
                   M: torch.Tensor, sums: torch.Tensor, workspace: torch.Tensor, inpaint=None, sigma_next: float = 0.0) -> None:
    """The guided step under adaptive projected guidance, in place (lx_euler_step_apg). scales = (s,): x fp32 and v fp32 or bf16 hold two
    parts laid out as euler_step_cfg's; scales = (scale_brain, scale_text): three parts as euler_step_cfg3's. M is fp32 with one part's
    element count (the momentum state: read unless momentum == 0, always written), sums float64 [n_images, 3] (written: sum Db^2, sum Db w,
    sum w^2 per image; its first dimension says how many images a part holds), workspace a contiguous buffer of at least
    apg_workspace_bytes(n_images, elems) bytes. inpaint = (x0, z, m), fp32 with one part's element count. All contiguous; nothing is
    synchronised."""
    scales = tuple(float(s) for s in scales)
    assert len(scales) in (1, 2), "euler_step_apg: scales is (scale,) for two parts or (scale_brain, scale_text) for three"
    parts = len(scales) + 1
    n, bf16, blend = _step_operands("euler_step_apg", x, v, parts, inpaint, f"x and v hold {parts} parts of one element count",
                                    "x0, z and m have the element count of one part", also=(M, sums, workspace))
    _req(M, torch.float32, "M")
    _req(sums, torch.float64, "sums")
    assert M.numel() == n, "euler_step_apg: M has the element count of one part"
    assert sums.dim() == 2 and sums.shape[1] == 3 and sums.shape[0] >= 1, "euler_step_apg: sums is [n_images, 3]"
    n_images = sums.shape[0]
    assert n % n_images == 0, "euler_step_apg: a part holds n_images images of one element count"
    check(lib.lx_euler_step_apg(x.data_ptr(), v.data_ptr(), bf16, parts, scales[0], scales[-1], float(sigma), float(dsigma), float(eta),
                                float(norm_threshold), float(momentum), M.data_ptr(), sums.data_ptr(), workspace.data_ptr(),
                                workspace.numel() * workspace.element_size(), *blend, float(sigma_next), n_images, n // n_images, _stream()),
          "lx_euler_step_apg")


def _multi_scales(name: str, scales):
    scales = tuple(float(s) for s in scales)
    assert len(scales) <= 2, f"{name}: scales is (), (scale,) for two parts or (scale_brain, scale_text) for three"
    return scales, len(scales) + 1


def dpmpp2m_step(x: torch.Tensor, v: torch.Tensor, sigma: float, dsigma: float, c: float, D: torch.Tensor, scales=(), inpaint=None,
                 sigma_next: float = 0.0) -> None:
    """One step of DPM-Solver++(2M) on the flow's sigmas, in place (lx_dpmpp2m_step): the Euler step of euler_step (scales = ()),
    euler_step_cfg (scales = (s,)) or euler_step_cfg3 (scales = (scale_brain, scale_text)) along its guided velocity g, plus
    c * (d - D) with d = x - sigma * g the denoised prediction; D (fp32, one part's element count: the previous step's d) becomes d. c == 0
    does not read D and is that Euler step bit for bit. inpaint = (x0, z, m) blends the result as euler_step_blend does. All contiguous;
    nothing is synchronised."""
    scales, parts = _multi_scales("dpmpp2m_step", scales)
    n, bf16, blend = _step_operands("dpmpp2m_step", x, v, parts, inpaint, f"x and v hold {parts} part(s) of one element count",
                                    "x0, z and m have the element count of one part", also=(D,))
    _req(D, torch.float32, "D")
    assert D.numel() == n, "dpmpp2m_step: D has the element count of one part"
    check(lib.lx_dpmpp2m_step(x.data_ptr(), v.data_ptr(), bf16, parts, scales[0] if scales else 0.0, scales[-1] if scales else 0.0,
                              float(sigma), float(dsigma), float(c), D.data_ptr(), *blend, float(sigma_next), n, _stream()), "lx_dpmpp2m_step")


def dpmpp2m_step_apg(x: torch.Tensor, v: torch.Tensor, sigma: float, dsigma: float, c: float, D: torch.Tensor, scales, eta: float,
                     norm_threshold: float, momentum: float, M: torch.Tensor, sums: torch.Tensor, workspace: torch.Tensor, inpaint=None,
                     sigma_next: float = 0.0) -> None:
    """dpmpp2m_step under adaptive projected guidance, in place (lx_dpmpp2m_step_apg): euler_step_apg's operands and passes, with
    c * (d - D) added around the projected velocity. D is fp32 with one part's element count; c == 0 does not read it and is
    euler_step_apg bit for bit."""
    scales, parts = _multi_scales("dpmpp2m_step_apg", scales)
    assert parts > 1, "dpmpp2m_step_apg: scales is (scale,) for two parts or (scale_brain, scale_text) for three"
    n, bf16, blend = _step_operands("dpmpp2m_step_apg", x, v, parts, inpaint, f"x and v hold {parts} parts of one element count",
                                    "x0, z and m have the element count of one part", also=(D, M, sums, workspace))
    _req(D, torch.float32, "D")
    _req(M, torch.float32, "M")
    _req(sums, torch.float64, "sums")
    assert D.numel() == n and M.numel() == n, "dpmpp2m_step_apg: D and M have the element count of one part"
    assert sums.dim() == 2 and sums.shape[1] == 3 and sums.shape[0] >= 1, "dpmpp2m_step_apg: sums is [n_images, 3]"
    n_images = sums.shape[0]
    assert n % n_images == 0, "dpmpp2m_step_apg: a part holds n_images images of one element count"
    check(lib.lx_dpmpp2m_step_apg(x.data_ptr(), v.data_ptr(), bf16, parts, scales[0], scales[-1], float(sigma), float(dsigma), float(c),
                                  D.data_ptr(), float(eta), float(norm_threshold), float(momentum), M.data_ptr(), sums.data_ptr(),
                                  workspace.data_ptr(), workspace.numel() * workspace.element_size(), *blend, float(sigma_next), n_images,
                                  n // n_images, _stream()), "lx_dpmpp2m_step_apg")


def flowedit_inputs(x_src: torch.Tensor, z_fe: torch.Tensor, noise: torch.Tensor, sigma: float, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """The inputs of one FlowEdit forward (lx_flowedit_inputs): out[1] = the source x_src noised to sigma (scale_noise's bits), out[0] =
    z_fe + (out[1] - x_src). x_src, z_fe and noise are fp32, contiguous, of one shape; out is fp32 contiguous with twice their element
    count, [target; source], allocated as [2, *shape] when not given."""
    for t, name in ((x_src, "x_src"), (z_fe, "z_fe"), (noise, "noise")):
        _req(t, torch.float32, name)
    out = torch.empty((2,) + tuple(x_src.shape), dtype=torch.float32, device=x_src.device) if out is None else out
    _req(out, torch.float32, "out")
    n = x_src.numel()
    assert z_fe.numel() == n and noise.numel() == n and out.numel() == 2 * n, "flowedit_inputs: x_src, z_fe and noise hold n elements, out 2n"
    assert all(t.is_contiguous() for t in (x_src, z_fe, noise, out)), "flowedit_inputs: contiguous operands"
    check(lib.lx_flowedit_inputs(out.data_ptr(), x_src.data_ptr(), z_fe.data_ptr(), noise.data_ptr(), float(sigma), n, _stream()),
          "lx_flowedit_inputs")
    return out


def flowedit_step(z_fe: torch.Tensor, v: torch.Tensor, coef: float, m: Optional[torch.Tensor] = None) -> None:
    """FlowEdit's update after one forward, in place (lx_flowedit_step): z_fe += coef * m * (v[:n] - v[n:]) with v = [target; source], fp32
    or bf16, of twice z_fe's element count; m (fp32, z_fe's element count; None: no mask) is 1 where the edit acts and 0 where the element
    keeps its bits. All contiguous; nothing is synchronised."""
    _req(z_fe, torch.float32, "z_fe")
    if v.dtype not in (torch.float32, torch.bfloat16):
        raise TypeError(f"v: expected float32 or bfloat16, got {v.dtype}")
    n = z_fe.numel()
    assert v.numel() == 2 * n, "flowedit_step: v holds two parts of z_fe's element count"
    if m is not None:
        _req(m, torch.float32, "m")
        assert m.numel() == n, "flowedit_step: m has z_fe's element count"
    assert all(t.is_contiguous() for t in (z_fe, v, m) if t is not None), "flowedit_step: contiguous operands"
    check(lib.lx_flowedit_step(z_fe.data_ptr(), v.data_ptr(), int(v.dtype == torch.bfloat16), float(coef), _p(m), n, _stream()),
          "lx_flowedit_step")


def convert(dst: torch.Tensor, src: torch.Tensor) -> None:
    assert dst.numel() == src.numel() and dst.is_contiguous() and src.is_contiguous()
    fmt = {torch.float32: 0, torch.bfloat16: 1, torch.float16: 2}
    assert src.dtype != torch.float16, "lx_convert reads fp32 or bf16"
    check(lib.lx_convert(dst.data_ptr(), fmt[dst.dtype], src.data_ptr(), fmt[src.dtype], dst.numel(), _stream()), "lx_convert")


# ---- VAE row kernels (include/lx.h "FLUX VAE") ------------------------------------------------------------------------
def groupnorm_silu(x: torch.Tensor, gamma, beta, y: torch.Tensor, groups: int = 32, eps: float = 1e-6, silu: bool = True) -> None:
    """x [B, P, C] fp32|bf16 (contiguous) -> y bf16 [B, P, C]."""
    B, P, Cc = x.shape
    _req(y, torch.bfloat16, "y")
    nb = lib.lx_groupnorm_workspace_bytes(B, P, groups)
    ws = torch.empty(nb, dtype=torch.uint8, device=x.device)
    check(lib.lx_groupnorm_silu(x.data_ptr(), int(x.dtype == torch.bfloat16), B, P, Cc, groups, gamma.data_ptr(), beta.data_ptr(), eps,
                                int(silu), y.data_ptr(), ws.data_ptr(), nb, _stream()), "lx_groupnorm_silu")


def im2col3x3(x: torch.Tensor, out: torch.Tensor, mode: int = 0) -> None:
    """x bf16 [B,H,W,C] (contiguous) -> out bf16 [B*Ho*Wo, Kpad]."""
    _req(x, torch.bfloat16, "x"); _req(out, torch.bfloat16, "out")
    B, H, W, Cc = x.shape
    check(lib.lx_im2col3x3(x.data_ptr(), B, H, W, Cc, mode, out.data_ptr(), out.shape[1], _stream()), "lx_im2col3x3")


def softmax_rows(S: torch.Tensor, P: torch.Tensor, scale: float, n_valid: Optional[int] = None) -> None:
    """P bf16 = softmax(scale * S) row by row. n_valid: only the first n_valid columns of S are keys (the others may hold anything);
    their probabilities fill P[:, :n_valid] and the remaining columns of P, up to P.shape[1], are set to +0."""
    _req(S, torch.float32, "S"); _req(P, torch.bfloat16, "P")
    if n_valid is None:
        check(lib.lx_softmax_rows(S.data_ptr(), S.stride(0), scale, P.data_ptr(), P.stride(0), S.shape[0], S.shape[1], _stream()), "lx_softmax_rows")
        return
    assert P.shape[0] == S.shape[0] and S.shape[1] >= n_valid, "softmax_rows: S and P need the same rows, S at least n_valid columns"
    check(lib.lx_softmax_rows_valid(S.data_ptr(), S.stride(0), scale, P.data_ptr(), P.stride(0), S.shape[0], int(n_valid), P.shape[1], _stream()),
          "lx_softmax_rows_valid")


# The same three on split-bf16 pair images (precise mode): hi at column c, lo at column lo_off + c of the same row.
def _req_pair(t, n_cols: int, lo_off: int, name: str) -> None:
    _req(t, torch.bfloat16, name)
    if lo_off % 8:
        raise ValueError(f"{name}: lo_off={lo_off} must be a multiple of 8")
    if lo_off < n_cols or t.stride(-2) < lo_off + n_cols or t.stride(-1) != 1:
        raise ValueError(f"{name}: rows of {t.stride(-2)} elements cannot hold a hi and a lo half of {n_cols} columns with lo_off={lo_off}")


def groupnorm_silu_split(x: torch.Tensor, gamma, beta, y: torch.Tensor, y_lo_off: int, groups: int = 32, eps: float = 1e-6, silu: bool = True) -> None:
    """x fp32 [B, P, C] (contiguous) -> the pair image y bf16 [B*P, >= y_lo_off + C] (row stride y.stride(0))."""
    B, P, Cc = x.shape
    _req(x, torch.float32, "x"); _req(gamma, torch.float32, "gamma"); _req(beta, torch.float32, "beta"); _req_pair(y, Cc, y_lo_off, "y")
    assert x.is_contiguous() and y.dim() == 2 and y.shape[0] == B * P, "groupnorm_silu_split: x contiguous, one row of y per pixel"
    nb = lib.lx_groupnorm_workspace_bytes(B, P, groups)
    ws = torch.empty(nb, dtype=torch.uint8, device=x.device)
    check(lib.lx_groupnorm_silu_split(x.data_ptr(), B, P, Cc, groups, gamma.data_ptr(), beta.data_ptr(), eps, int(silu), y.data_ptr(), y.stride(0),
                                      y_lo_off, ws.data_ptr(), nb, _stream()), "lx_groupnorm_silu_split")


def im2col3x3_split(x: torch.Tensor, C_: int, x_lo_off: int, out: torch.Tensor, mode: int = 0) -> None:
    """x bf16 [B, H, W, ld]: pair pixels of C_ channels (hi at 0, lo at x_lo_off; W, H contiguous, row stride x.stride(2)) -> out bf16
    [B*Ho*Wo, 2*Kpad] (contiguous): hi taps | lo taps."""
    _req_pair(x, C_, x_lo_off, "x"); _req(out, torch.bfloat16, "out")
    B, H, W, _ = x.shape
    ld = x.stride(2)
    assert x.stride(1) == W * ld and x.stride(0) == H * W * ld, "im2col3x3_split: pixels must lie back to back"
    assert out.dim() == 2 and out.is_contiguous() and out.shape[1] % 2 == 0, "im2col3x3_split: out is [rows, 2*Kpad], contiguous"
    check(lib.lx_im2col3x3_split(x.data_ptr(), ld, x_lo_off, B, H, W, C_, mode, out.data_ptr(), out.shape[1] // 2, _stream()), "lx_im2col3x3_split")


def softmax_rows_split(S: torch.Tensor, P: torch.Tensor, scale: float, n_valid: int, n_store: int, p_lo_off: int) -> None:
    """The pair P (hi at column c, lo at p_lo_off + c) = softmax(scale * S[:, :n_valid]) row by row; columns [n_valid, n_store) of both
    halves are set to +0, nothing else of P is written and columns >= n_valid of S are not read."""
    _req(S, torch.float32, "S"); _req_pair(P, n_store, p_lo_off, "P")
    assert P.shape[0] == S.shape[0] and S.shape[1] >= n_valid, "softmax_rows_split: S and P need the same rows, S at least n_valid columns"
    check(lib.lx_softmax_rows_split(S.data_ptr(), S.stride(0), scale, P.data_ptr(), P.stride(0), p_lo_off, S.shape[0], int(n_valid), int(n_store), _stream()),
          "lx_softmax_rows_split")


# The fp16-operand VAE's producers (operands="fp16"): fp16 images for LX_OPERANDS_F16 launches. f16_ovf: int32 device counter of the waves
# that clipped a value to +-65504, or None (not reported). im2col3x3 takes the fp16 images viewed as 16-bit words.
def _req_ovf(f16_ovf) -> None:
    if f16_ovf is not None:
        _req(f16_ovf, torch.int32, "f16_ovf")


def groupnorm_silu_f16(x: torch.Tensor, gamma, beta, y: torch.Tensor, groups: int = 32, eps: float = 1e-6, silu: bool = True, f16_ovf=None) -> None:
    """x fp32 [B, P, C] (contiguous) -> y fp16 [B, P, C] (contiguous), saturated to +-65504."""
    B, P, Cc = x.shape
    _req(x, torch.float32, "x"); _req(gamma, torch.float32, "gamma"); _req(beta, torch.float32, "beta"); _req(y, torch.float16, "y")
    _req_ovf(f16_ovf)
    if not (x.is_contiguous() and y.is_contiguous() and y.numel() == B * P * Cc):
        raise ValueError("groupnorm_silu_f16: x and y contiguous, y as many elements as x")
    nb = lib.lx_groupnorm_workspace_bytes(B, P, groups)
    ws = torch.empty(nb, dtype=torch.uint8, device=x.device)
    check(lib.lx_groupnorm_silu_f16(x.data_ptr(), B, P, Cc, groups, gamma.data_ptr(), beta.data_ptr(), eps, int(silu), y.data_ptr(), ws.data_ptr(), nb,
                                    _p(f16_ovf), _stream()), "lx_groupnorm_silu_f16")


def softmax_rows_f16(S: torch.Tensor, P: torch.Tensor, scale: float, n_valid: Optional[int] = None) -> None:
    """softmax_rows with fp16 probabilities; one entry point for both forms (n_valid None: every column of S is a key and P has as many)."""
    _req(S, torch.float32, "S"); _req(P, torch.float16, "P")
    nv = S.shape[1] if n_valid is None else int(n_valid)
    if P.shape[0] != S.shape[0] or S.shape[1] < nv or P.shape[1] < nv or S.stride(1) != 1 or P.stride(1) != 1:
        raise ValueError("softmax_rows_f16: S and P need the same rows, unit column strides and at least n_valid columns each")
    check(lib.lx_softmax_rows_f16(S.data_ptr(), S.stride(0), scale, P.data_ptr(), P.stride(0), S.shape[0], nv, P.shape[1], _stream()), "lx_softmax_rows_f16")


def convert_f16(dst: torch.Tensor, src: torch.Tensor, f16_ovf=None) -> None:
    """dst fp16 = src (fp32 | bf16), saturated to +-65504 and counted in f16_ovf."""
    _req(dst, torch.float16, "dst")
    if src.dtype not in (torch.float32, torch.bfloat16):
        raise TypeError(f"src: expected torch.float32 or torch.bfloat16, got {src.dtype}")
    _req(src, src.dtype, "src"); _req_ovf(f16_ovf)
    if dst.numel() != src.numel() or not (dst.is_contiguous() and src.is_contiguous()):
        raise ValueError("convert_f16: dst and src contiguous with the same number of elements")
    check(lib.lx_convert_f16(dst.data_ptr(), src.data_ptr(), int(src.dtype == torch.bfloat16), dst.numel(), _p(f16_ovf), _stream()), "lx_convert_f16")


# ---- CS3 / DGF -------------------------------------------------------------------------------------------
def s4_scan(u, lam, w, D, y) -> None:
    B, H, Lq = u.shape
    check(lib.lx_s4_scan(u.data_ptr(), lam.data_ptr(), w.data_ptr(), D.data_ptr(), y.data_ptr(), B, H, Lq, lam.shape[1], _stream()), "lx_s4_scan")


def s4_conv(u, K, D, y) -> None:
    B, H, Lq = u.shape
    check(lib.lx_s4_conv(u.data_ptr(), K.data_ptr(), D.data_ptr(), y.data_ptr(), B, H, Lq, _stream()), "lx_s4_conv")


def chanmix(x, W, bias, resid, ln_g, ln_b, y, act=0) -> None:
    B, Hin, Lq = x.shape
    check(lib.lx_chanmix(x.data_ptr(), W.data_ptr(), _p(bias), _p(resid), _p(ln_g), _p(ln_b), y.data_ptr(), B, Hin, W.shape[0], Lq,
                         act, _stream()), "lx_chanmix")


def pyramid_pool(x, y, sizes, y_col0=0) -> None:
    B, Cc, Lq = x.shape
    arr = (C.c_int * len(sizes))(*sizes)
    check(lib.lx_pyramid_pool(x.data_ptr(), y.data_ptr(), B, Cc, Lq, arr, len(sizes), y.stride(-2), y_col0, _stream()), "lx_pyramid_pool")


def layernorm_relu(x, g, b, eps=1e-5) -> None:
    check(lib.lx_layernorm_relu(x.data_ptr(), g.data_ptr(), b.data_ptr(), x.shape[0], x.shape[1], eps, _stream()), "lx_layernorm_relu")


def linear_f32(X, W, bias, Y, *, M, N, K, ldx, ldy, x_trans=False, y_trans=False, accumulate=False, ldw=None) -> None:
    check(lib.lx_linear_f32(X.data_ptr(), ldx, int(x_trans), W.data_ptr(), W.stride(0) if ldw is None else ldw, _p(bias), Y.data_ptr(),
                            ldy, int(y_trans), M, N, K, int(accumulate), _stream()), "lx_linear_f32")


def chan_gemm_f32(X, W, bias, Y, *, N, K, epilogue=0, ldw=None) -> None:
    """Y[b, n, l] (=|+=) sum_k W[n, k] X[b, k, l] + bias[n] on channel-major fp32 [B, K, L] / [B, N, L] (fp32 MFMA)."""
    B, _, Lq = X.shape
    check(lib.lx_chan_gemm_f32(X.data_ptr(), X.stride(0), X.stride(1), W.data_ptr(), W.stride(0) if ldw is None else ldw, _p(bias),
                               Y.data_ptr(), Y.stride(0), Y.stride(1), B, N, K, Lq, epilogue, None, _stream()), "lx_chan_gemm_f32")


def duan_fwd(x, c, p, y, keep_k, eps=1e-3) -> None:
    """p: dict with gate.0.weight/bias, gate.2.weight/bias, mlp.0.weight/bias, mlp.2.weight/bias (conv1x1 as [out,in])."""
    B, Cc, Lq = x.shape
    Hd = p["gate.0.weight"].shape[0]
    nbytes = lib.lx_duan_workspace_bytes(B, Cc, Lq, Hd)
    ws = torch.empty(nbytes, dtype=torch.uint8, device=x.device)
    check(lib.lx_duan_fwd(x.data_ptr(), c.data_ptr(), p["gate.0.weight"].data_ptr(), p["gate.0.bias"].data_ptr(),
                          p["gate.2.weight"].data_ptr(), p["gate.2.bias"].data_ptr(), p["mlp.0.weight"].data_ptr(),
                          p["mlp.0.bias"].data_ptr(), p["mlp.2.weight"].data_ptr(), p["mlp.2.bias"].data_ptr(), y.data_ptr(),
                          B, Cc, Lq, Hd, eps, keep_k, ws.data_ptr(), nbytes, _stream()), "lx_duan_fwd")
