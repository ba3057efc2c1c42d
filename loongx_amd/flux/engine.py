"""DiT engine: one LoongX/Flux denoise step on MI355X, composed from the liblx_amd.so kernels.

Implements the arithmetic of the reference's `tranformer_forward` (src/flux/transformer.py:47-252) and
`block_forward` / `single_block_forward` / `attn_forward` (src/flux/block.py) on a stream-major token layout:

    X  fp32 [B*T text rows | B*N image rows | B*C condition rows, D]   residual stream (fp32 accumulate)
    XN bf16 same rows                                                  AdaLN-normalised GEMM operand
    Y  bf16 [rows, 7D] = [k | v | q/attn-out | mlp]                    projections; attention writes O over q

Per step the engine hoists everything that does not depend on the timestep (reference recomputes it 28x):
context_embedder(prompt_embeds), x_embedder(condition_latents), both RoPE tables, the guidance/text parts of
temb, cond_temb (c_t is fixed, transformer.py:108-114) and therefore EVERY modulation vector of the condition stream.
LoRA semantics follow lora_controller.enable_lora: the condition stream runs W + s*B*A, the image stream the base
weights unless model_config["latent_lora"]; evaluated as a rank-r epilogue term, never by merging weights.
"""
from __future__ import annotations

import math
import os
from typing import Dict, List, NamedTuple, Optional, Sequence

import torch

from .. import ops
from ..ops import LX_EPI_RESID_F32, LX_EPI_STORE_F32
from .modes import E4M3Mode, Mode16, SplitMode
from .step_cache import StepCacheState, normalise_model_config, step_cache_config
from .weights import FluxConfig, PackedWeights

NEG_INF = float("-inf")


def _pad64(n: int) -> int:
    return (n + 63) // 64 * 64


class Stream(NamedTuple):
    """One token stream of the stream-major layout (DiTEngine.streams, built by setup())."""
    name: str                # "txt" | "img" | "cond"
    len: int                 # tokens per sample
    row0: int                # first row of X / XN / Y
    vt0: int                 # first slot of a V^T row
    mods: torch.Tensor       # its modulation vectors: the step's (mods) or the conditioning's (cmods)


class HostWord:
    """One int32 device word watched from the host without a synchronisation: a pinned host word and an event. take() gives the value
    a previous request() copied, once that copy has landed; request() enqueues the next copy unless one is in flight. So a value
    surfaces at most one call late."""

    def __init__(self):
        self.host: Optional[torch.Tensor] = None
        self.event = None

    def take(self) -> Optional[int]:
        if self.event is None or not self.event.query():
            return None
        self.event = None
        return int(self.host[0])

    def request(self, word: torch.Tensor) -> None:
        if self.event is not None:
            return
        if self.host is None:
            self.host = torch.zeros(1, dtype=torch.int32).pin_memory()
        self.host.copy_(word, non_blocking=True)
        self.event = torch.cuda.Event()
        self.event.record()

    def drop(self) -> None:
        """Forget a copy in flight (what it would report has been reported, or reset, otherwise)."""
        self.event = None


def mask_argument(attention_mask) -> None:
    """What an attention_mask argument must be before anything else is looked at (attn_forward, tranformer_forward, set_conditioning)."""
    if not isinstance(attention_mask, torch.Tensor) or attention_mask.dim() < 2:
        raise NotImplementedError("attention_mask must be a tensor of rank 2..4 over the concatenated [text | image | condition] sequence")


def refuse_masked_modes(model_config: Optional[Dict], precise_default: bool) -> None:
    """The arithmetic modes that have no masked attention kernel."""
    mc = model_config or {}
    if bool(mc.get("precise", precise_default)):
        raise NotImplementedError("attention_mask is not supported in precise mode")
    if mc.get("attn_fp8", False):
        raise NotImplementedError("attention_mask is not supported in attn_fp8 mode")


def refuse_wide_lora_modes(w: PackedWeights, model_config: Optional[Dict], precise_default: bool) -> None:
    """The arithmetic modes whose kernels evaluate adapters from one 16-column down-projection slab only."""
    wide = max([lo.down.shape[0] for lo in w.lora.values()] + [0])
    if wide <= 16:
        return
    mc = model_config or {}
    for mode, on in (("precise", bool(mc.get("precise", precise_default))), ("gemm_fp8", bool(mc.get("gemm_fp8", False)))):
        if on:
            raise ValueError(f"LoRA rank {w.cfg.lora_r} is not supported in {mode} mode ({wide} adapter columns behind one GEMM; that "
                             "mode takes at most 16): use the bf16 or fp16 operand mode")


class DiTEngine:
    def __init__(self, weights: PackedWeights, device="cuda"):
        self.w = weights
        self.cfg: FluxConfig = weights.cfg
        self.device = torch.device(device)
        if self.cfg.attention_head_dim != 128:
            raise ValueError("the gfx950 attention kernel is specialised for head_dim 128 (FLUX.1)")
        self.shape = None
        self.cond_ready = False          # set_conditioning() completed and nothing has replaced what it set up since (configure() unsets it)
        self.sched = None
        self.graphs: Dict = {}
        self._warmed = set()             # kernel sets (modes) that have run eagerly once: first launches must not happen inside a capture
        self.use_graph = os.environ.get("LX_GRAPH", "1") != "0"
        # The projection launches normalise / rotate k and q and write V^T in their epilogue (LX_EPI_QKV) wherever the shapes allow it
        # (_rope_pairs decides); False forces the separate lx_qkv_prep pass everywhere (tests compare the two).
        self.qkv_epilogue = True
        # The LayerNorm launches also compute the LoRA down-projection of the Linear that reads their output (lx_ln_modulate_lora_segs: on
        # the matrix pipe, inside the same launch); False = the separate lx_lora_down launches everywhere (tests compare the two).
        self.ln_lora = True
        self.model_config: Dict = {}
        self.c_factor: Optional[float] = None
        self.latent_lora = False
        self.attn_bias: Dict[str, Dict[str, float]] = {}
        self.cos_main = self.sin_main = self.cos_cond = self.sin_cond = None      # RoPE tables of the conditioning (set_conditioning / configure)
        # A caller's attention_mask, [Bm, Hm, Sq, S] over the concatenated [txt | img | cond] sequence.
        #   attn_mask: block.attn_forward's, set for the duration of one call (the mask is prepared inside every such call);
        #   cond_mask: the conditioning's (set_conditioning(attention_mask=...)): prepared ONCE there into `_mask_ws`, which all 57 attention
        #     launches of every forward of that conditioning read (attn_fwd_masked(prepped=True)), eagerly or from the captured step graph.
        # Both None: the unmasked kernels, untouched.
        self.attn_mask: Optional[torch.Tensor] = None
        self.cond_mask: Optional[torch.Tensor] = None
        self._mask_ws: Optional[torch.Tensor] = None
        # Split-K pair plan of the GEMM (lx_gemm_bf16_ws): needs a caller-owned workspace, one per stream -- this engine owns one
        # and runs on one stream at a time. LX_PAIR_PLAN=0 (or engine.pair_plan = False before the first step) gives launch plans
        # that do not depend on the batch size, i.e. data-parallel shards equal the single-GPU batch bit for bit.
        self.pair_plan = os.environ.get("LX_PAIR_PLAN", "1") != "0"
        self.lora_scale = 1.0            # lora_controller.enable_lora / set_lora_scale drive this (0 = adapters off everywhere)
        # Per-adapter weights (set_adapter_weights): name -> float, or one float per image of the conditioning. set_conditioning turns them
        # and lora_scale into `lora_w`, fp32 [B, cfg.lora_r]: the factor of every column of the stacked adapter's down-projection, which
        # lx_lora_scale_rows applies to the adapter scratch (TLs / tmod) right after it is written. None = every factor is 1: no such
        # launch anywhere. `lora_w_ns`: the same without lora_scale (the e4m3 down-projection takes lora_scale as its scalar argument).
        self.adapter_weights: Dict[str, object] = {}
        # generate() under true CFG sets this to 2 for the steps of one call: the conditioning then holds [positive; negative] halves of
        # the same images, and a per-image weight table of half its batch applies to each half.
        self.adapter_weight_tiles = 1
        self.lora_w: Optional[torch.Tensor] = None
        self.lora_w_ns: Optional[torch.Tensor] = None
        self._lora_w_bufs: Dict = {}     # (B, R, which) -> the table's buffer: one address per shape, so step graphs can hold it
        # Precise mode (model_config["precise"], default `precise_default`): fp32-class arithmetic for the reference's shipped
        # fp32 configuration -- split-bf16 MFMA GEMMs (2 or 3 K-segments), fp32 q/k/v, fp32 attention (csrc/precise.hip).
        self.precise_default = False
        self.attn_nomax = False
        self._nomax_room = 100.0         # what the largest finite attention bias leaves of the bounded kernel's score range (_setup_nomax)
        self.precise = False
        self.precise_attn_split = False  # decided when the precise buffers are allocated (_setup_precise)
        # fp8 GEMM path (model_config["gemm_fp8"]; BASELINE configs[4]): e4m3 operand images on the 64-deep f8f6f4 MFMA
        self.gemm_fp8 = False
        self.w8: Dict[str, torch.Tensor] = {}          # name -> tiled e4m3 weight / name + ".rs" -> row de-scale, built on first use
        self._w8_key = None                            # (weights, weights_version) the images were quantised from
        # fp16 operand mode (model_config["operands"] = "fp16", default `operands_default`; OminiModel(dtype=torch.float16)): every GEMM of
        # the forward multiplies IEEE fp16 images (11 significand bits) instead of bf16 ones (8) on v_mfma_f32_*_f16, same rate, same
        # layouts; fp32 accumulation, residual stream and everything between the GEMMs as in the bf16 mode; attention operands (q, k, V^T)
        # stay bf16. The bf16 mode's per-forward error IS the 8-bit rounding of the GEMM A operands (tools/bf16_ablation.py: 4.58e-3, with
        # fp16 images 7.0e-4), and bf16 weights convert to fp16 exactly down to 2^-24 granularity. fp16 has 5 exponent bits: the producers
        # saturate at +-65504 and count the waves that did in `f16_ovf` (f16_overflow_count()).
        self.operands_default = "bf16"
        self.f16 = False
        self.w16: Dict[str, torch.Tensor] = {}         # name -> fp16 image of the (tiled) weight / name + ".down" -> fp16 LoRA down-projection
        self.w16_inexact_share, self.w16_clipped = 0.0, 0
        self._w16_key, self._w16_gen = None, 0
        self._w16_wstat = (0, 0, 0)      # (values that lost bits, values clipped, values) of the weight images, without the adapters'
        self.f16_ovf: Optional[torch.Tensor] = None
        self._ovf_word, self._ovf_seen = HostWord(), 0         # f16_overflow_poll(sync=False)
        self._gemm_ws: Optional[torch.Tensor] = None
        self._err_word = HostWord()                            # check_status(sync=False)
        # the operand modes of the block GEMMs (modes.py; stateless). _select_mode picks `mode`; attention_module always runs mode16
        self.mode16, self.mode8, self.mode_split = Mode16(self), E4M3Mode(self), SplitMode(self)
        self.mode = self.mode16
        # Step-invariant condition stream (model_config independent_condition / union_cond_attn = False: the condition queries see
        # only condition keys, its timestep c_t is fixed, so its hidden states, keys and values are the same at every denoise step):
        # the first forward after set_conditioning() computes all three streams and leaves the condition keys / V^T of every layer in
        # per-layer images; the following forwards run the text and image rows only. LX_COND_CACHE=0 recomputes every step.
        self.cond_cache_enabled = os.environ.get("LX_COND_CACHE", "1") != "0"
        self.cond_cache = False          # decided per conditioning (set_conditioning)
        self.cond_cached = False         # the per-layer images hold this conditioning's condition keys / values
        self.cond_skip = False           # the forward being enqueued runs without the condition rows
        self.KC = self.VTC = None        # [layers, M, D] keys / [layers, B, H, 128, vt_ld] V^T, allocated on first use
        self.KC2 = self.VTC2 = None      # precise mode's: [layers, M, 2D] key pairs (hi | lo) / [layers, 2, B, H, 128, vt_ld] V^T pairs
        self.KC8 = self.VTC8 = None      # attn_fp8's: [layers, M, D] e4m3 keys / [layers, B, H, 128, vt_ld] e4m3 V^T (half the bf16 images)
        # Step cache (model_config step_cache_thresh; step_cache.py has the rule): decided per conditioning (set_conditioning). With it on a
        # step is three parts -- probe, body, reuse (_forward_step_cache) -- and the host reads one pair of doubles between the first and the
        # next. The buffers exist only once a conditioning has asked for them, and then until the shape changes (step graphs hold them):
        #   sc_m fp32 [B*N, D]: the image stream's norm1 input of double block 0 at the previous step;  sc_R fp32 [B*N, D]: X0 during a
        #   computed step's blocks, then the residual X_img - X0 that skipped steps add;  sc_rows / sc_sums / sc_host: the probe's sums.
        self.step_cache: Optional[StepCacheState] = None
        self.sc_m = self.sc_R = self.sc_rows = self.sc_sums = self.sc_host = None
        # (Round 5 removed three measured-negative options that lived here as environment switches: the q/k/v adapters' down-projection
        # inside ln_modulate (LX_LN_LORA: -1.1 %; it could absorb the 57 launches per step that read the AdaLN-normalised stream, not the 75
        # that read an attention output or a GELU hidden), adapter rows on merged weights W' = W + s B A (LX_LORA_MERGE: +11.5 GB, the GEMMs
        # give the saved launches back as lost weight sharing) and the MLP-up half of the single blocks on a second stream (LX_OVERLAP: the
        # step runs at the package power cap, +0.3 % / -1 %). DESIGN.md sections 3.2, 9 and 10 keep the measurements.)

    # ------------------------------------------------------------------------------------------ workspace
    def setup(self, B: int, T: int, N: int, C: int) -> None:
        cfg, dev = self.cfg, self.device
        # slab width of the LoRA scratch: the widest down-projection of the adapter set (the fused single-block GEMM's four modules x
        # rank), 16 for the ranks that fit lx_lora_down's narrow form. (A wider adapter set re-allocates even where its installer left
        # `shape` alone: the slabs are written by kernels.)
        tl_w = (max([16, cfg.lora_r] + [lo.down.shape[0] for lo in self.w.lora.values()]) + 3) // 4 * 4
        if self.shape == (B, T, N, C) and self.TLs.shape[2] >= tl_w and self.tmod.shape[1] >= (cfg.num_layers + cfg.num_single_layers) * cfg.lora_r:
            return
        D, H = cfg.inner_dim, cfg.num_attention_heads
        self.B, self.T, self.N, self.C = B, T, N, C
        self.r_txt, self.r_img, self.r_cond = 0, B * T, B * (T + N)
        self.M = B * (T + N + C)
        M = self.M
        f32, bf16 = torch.float32, torch.bfloat16
        self.X = torch.zeros(M, D, dtype=f32, device=dev)
        self.XN = torch.zeros(M, D, dtype=bf16, device=dev)
        self.Y = torch.zeros(M, 7 * D, dtype=bf16, device=dev)
        self.XN16, self.Y16 = self.XN.view(torch.float16), self.Y.view(torch.float16)    # the same bytes as fp16 operand images (operands = "fp16")
        self.vt0 = {"txt": 0, "img": _pad64(T), "cond": _pad64(T) + _pad64(N)}
        self.VT = torch.zeros(B, H, 128, _pad64(T) + _pad64(N) + _pad64(C), dtype=bf16, device=dev)
        self.Q8 = self.K8 = self.VT8 = None                       # fp8 attention images, allocated on first use
        self.TL_SPLIT = 4                 # K-split slabs of the LoRA down-projection: 35.50 ms per step against 35.72 with 2 and 36.12 with 1
                                          # (tools/ab_engine_attr.py TL_SPLIT 4 2, round 5; lx_gemm4_kernel sums at most four slabs)
        # precise mode writes one slab per cross term (up to 3: hi.A, lo.A, hi.A_lo) whatever the K-split of the bf16 path is
        self.TLs = torch.zeros(max(self.TL_SPLIT, 3), M, tl_w, dtype=f32, device=dev)
        self.TL = self.TLs[0]
        self.lat16 = torch.zeros(B * N, cfg.in_channels, dtype=bf16, device=dev)
        self.lat16h = self.lat16.view(torch.float16)
        self.out = torch.zeros(B * N, cfg.in_channels, dtype=f32, device=dev)
        self.temb = torch.zeros(B, D, dtype=f32, device=dev)
        self.temb_base = torch.zeros(B, D, dtype=f32, device=dev)
        self.cond_temb = torch.zeros(B, D, dtype=f32, device=dev)
        self.tproj = torch.zeros(B, 256, dtype=f32, device=dev)
        self.thid = torch.zeros(B, D, dtype=f32, device=dev)
        self.t1000 = torch.zeros(B, dtype=f32, device=dev)
        self.mods = torch.zeros(B, cfg.n_mod, dtype=f32, device=dev)
        self.cmods = torch.zeros(B, cfg.n_mod, dtype=f32, device=dev)
        self.streams = [Stream("txt", T, self.r_txt, self.vt0["txt"], self.mods), Stream("img", N, self.r_img, self.vt0["img"], self.mods),
                        Stream("cond", C, self.r_cond, self.vt0["cond"], self.cmods)]
        self.stream = {s.name: s for s in self.streams}
        nb = cfg.num_layers + cfg.num_single_layers
        self.tmod = torch.zeros(B, max(nb * cfg.lora_r, 4), dtype=f32, device=dev)
        self.X_txt_init = torch.zeros(max(B * T, 1), D, dtype=f32, device=dev)
        self.X_cond_init = torch.zeros(max(B * C, 1), D, dtype=f32, device=dev)
        rd = sum(cfg.axes_dims_rope)
        self.rope_main = torch.zeros(2, T + N, rd, dtype=f32, device=dev)
        self.rope_cond = torch.zeros(2, max(C, 1), rd, dtype=f32, device=dev)
        # the same tables as (cos, sin) per rotary pair, for the projection GEMM's fused RMSNorm + RoPE epilogue (LX_EPI_QKV)
        self.rope_cs_main = torch.zeros(T + N, rd, dtype=f32, device=dev)
        self.rope_cs_cond = torch.zeros(max(C, 1), rd, dtype=f32, device=dev)
        self.qkv_fused = False
        self.g_lat = torch.zeros(B, N, cfg.in_channels, dtype=f32, device=dev)
        self.g_t = torch.zeros(B, dtype=f32, device=dev)
        self.graphs = {}
        self.shape = (B, T, N, C)
        self.cond_ready = False
        self.KC = self.VTC = self.KC2 = self.VTC2 = self.KC8 = self.VTC8 = None      # per-layer key / V^T images of the condition cache: shape-bound
        self.cond_cache = self.cond_cached = False
        self.step_cache = None
        self.sc_m = self.sc_R = self.sc_rows = self.sc_sums = None      # the step cache's buffers: shape-bound
        self.XN2 = self.Y32 = self.YA = self.lat2 = None          # precise-mode buffers, allocated by _setup_precise()
        self.XN8 = self.Y8 = None                                  # fp8-GEMM operand images, allocated by _setup_fp8()

    def _setup_precise(self) -> None:
        """The split mode's operand buffers -- XN2 bf16 [M, 2D], Y32 fp32 [M, 3D], YA bf16 [M, 10D], lat2 for the step's latents -- and the
        precise attention's images; what lives where in them: DESIGN.md section 8.2."""
        if self.XN2 is not None:
            return
        if not self.w.precise_ready:
            raise ValueError("precise mode needs weights packed with precise=True (pack_state_dict / LxFluxTransformer.from_state_dict): "
                             "the bf16 rounding residuals of the weights were not kept")
        D, dev, bf16 = self.cfg.inner_dim, self.device, torch.bfloat16
        self.XN2 = torch.zeros(self.M, 2 * D, dtype=bf16, device=dev)
        self.Y32 = torch.zeros(self.M, 3 * D, dtype=torch.float32, device=dev)
        self.YA = torch.zeros(self.M, 10 * D, dtype=bf16, device=dev)
        self.lat2 = torch.zeros(self.B * self.N, 2 * self.cfg.in_channels, dtype=bf16, device=dev)
        # precise attention on the bf16 matrix pipe (lx_attn_fwd_split): q / k after RMSNorm + RoPE and v^T as bf16 hi / lo pairs
        #   QK2 bf16 [M, 4D] = [k_hi | k_lo | q_hi | q_lo];  VT2 bf16 [2, B, H, 128, slots] = the hi and the lo V^T image
        # LX_PRECISE_ATTN=f32: the exact fp32-MFMA kernel (lx_attn_fwd_f32: 1/16 of the bf16 matrix rate, half of a precise step)
        self.precise_attn_split = os.environ.get("LX_PRECISE_ATTN", "split") != "f32"
        if self.precise_attn_split:
            self.QK2 = torch.zeros(self.M, 4 * D, dtype=bf16, device=dev)
            self.VT2 = torch.zeros((2,) + tuple(self.VT.shape), dtype=bf16, device=dev)

    def _fp8_images(self) -> None:
        """Q8 / K8 u8 [M, D], VT8 u8 [B, H, 128, slots]: the e4m3 operand images of the fp8 attention path (model_config attn_fp8)."""
        if self.Q8 is None:
            u8, D = torch.uint8, self.cfg.inner_dim
            self.Q8 = torch.zeros(self.M, D, dtype=u8, device=self.device)
            self.K8 = torch.zeros(self.M, D, dtype=u8, device=self.device)
            self.VT8 = torch.zeros(self.VT.shape, dtype=u8, device=self.device)

    def _setup_f16(self) -> None:
        """fp16 images of every weight a GEMM of the forward reads (block weights, embedders, final projection: +17 GB at FLUX.1-dev scale,
        resident while the engine is in the fp16 operand mode and released by the first conditioning that selects bf16 operands; the stacked
        modulation weights stay bf16 -- their activations are bf16 hi / lo pairs already) and of the LoRA down-projections, built once
        per weight set (the key holds the weights' version counters: a broadcast or a new adapter rebuilds them at the next conditioning or
        forward). bf16 -> fp16 is exact for 2^-14 <= |w| <= 65504 and to 2^-24 absolute below (fp16 subnormals, which the MFMA honours:
        tests/test_f16_gpu.py); the share of weights that lose bits is kept in `w16_inexact_share`. A weight beyond fp16's range is
        SATURATED to +-65504, never turned into inf, and counted in `w16_clipped` -- which f16_overflow_poll() reports with the activations'
        saturation counter, so the product's f16_overflow policy sees it. One host synchronisation per weight set."""
        if self.f16_ovf is None:
            self.f16_ovf = torch.zeros(1, dtype=torch.int32, device=self.device)
        # Only the adapter set moved (another active set, a new adapter: lora_version): the weight images stay where they are and only the
        # adapters' `.down` images are rebuilt -- switching adapters from image to image must not re-convert 17 GB.
        key = ((id(self.w), getattr(self.w, "weights_version", 0)), (getattr(self.w, "lora_version", 0), len(self.w.lora)))
        if self.w16 and self._w16_key == key:
            return
        full = not self.w16 or self._w16_key is None or self._w16_key[0] != key[0]
        self._w16_gen += 1                                         # part of the step graphs' key: they hold the images' addresses
        stat = torch.zeros(2, 2, dtype=torch.int64, device=self.device)      # weights, adapters: [values that lost bits, values clipped]

        def image(W, st):
            h = W.float().clamp_(-65504.0, 65504.0).to(torch.float16)
            back = h.to(W.dtype)
            st[0] += (back != W).sum()
            st[1] += (W.float().abs() > 65504.0).sum()
            return h

        if full:
            self.w16 = {}
            total = 0
            for name, W in self.w.t.items():
                if not name.endswith(".w") or name.startswith("mod.") or name.startswith("tte.") or W.dtype != torch.bfloat16:
                    continue
                h = image(W, stat[0])
                if getattr(W, "lx_tiled", False):
                    h.lx_tiled = True                          # an elementwise conversion keeps the tiled image
                total += W.numel()
                self.w16[name[:-2]] = h
        else:
            for name in [n for n in self.w16 if n.endswith(".down")]:
                del self.w16[name]
        for name, lo in self.w.lora.items():
            self.w16[name + ".down"] = image(lo.down, stat[1])
        (w_lost, w_clipped), (a_lost, a_clipped) = ([int(v) for v in row] for row in stat.tolist())
        if full:
            self._w16_wstat = (w_lost, w_clipped, total)
        w_lost, w_clipped, total = self._w16_wstat
        self.w16_inexact_share = (w_lost + a_lost) / max(total, 1)
        self.w16_clipped = w_clipped + a_clipped
        self._w16_key = key

    def f16_overflow_count(self, reset: bool = True) -> int:
        """Producer waves that saturated a value to +-65504 since the last reset (fp16 operand mode; synchronises). 0 = every operand
        image is the nearest-even rounding of its fp32 value."""
        if self.f16_ovf is None:
            return 0
        n = int(self.f16_ovf.item())
        if reset:
            self._ovf_word.drop()                              # (an asynchronous read still in flight would report what this call reported)
            self._ovf_seen = 0
            if n:
                self.f16_ovf.zero_()
        return n

    def f16_overflow_poll(self, sync: bool = False) -> int:
        """What the product does with the fp16 mode's saturation counter (generate() applies model_config["f16_overflow"] to the result): the
        number of saturation events not yet reported -- producer waves that clipped an activation to +-65504 (GEMM 16-bit stores, the
        LayerNorm launches, the attention output) plus the weights `_setup_f16` had to clip (those count on every call: every image
        computed with them is affected). The reference clips its fp16 activations silently (block.py:275-276, 336-337); here a clipped
        operand is an event the caller hears about. 0 outside the fp16 operand mode.
        sync=True drains the stream and reads the counter now. sync=False costs no synchronisation -- the check_status(sync=False)
        pattern: it looks at the value copied to pinned host memory by the previous call, if that copy has landed, and enqueues the next
        copy, so an event surfaces at most one call late."""
        if not self.f16 or self.f16_ovf is None:
            return 0
        wclip = int(self.w16_clipped)
        if sync:
            return self.f16_overflow_count(reset=True) + wclip
        n, total = 0, self._ovf_word.take()
        if total is not None:
            n, self._ovf_seen = max(total - self._ovf_seen, 0), total          # the device counter runs on: nothing is reset behind the kernels' back
        self._ovf_word.request(self.f16_ovf)
        return n + wclip

    def set_lora_scale(self, s: float) -> None:
        """Multiplier on every adapter term (reference lora_controller.py: scale_layer). Changes what the captured step graphs
        and the cached condition-stream modulations contain, so both are dropped."""
        s = float(s)
        if s != self.lora_scale:
            self.lora_scale = s
            self._adapters_changed()

    def _adapters_changed(self) -> None:
        """What the adapter terms contribute has changed: the captured step graphs, the prepared schedule and the conditioning (with its
        cached condition stream) go."""
        self.graphs = {}
        self.cond_ready = False
        self.sched = None

    # What the layers above drop by hand: no other file assigns an engine cache field. (Neither group occurs among
    # the engine's own events: _adapters_changed keeps the conditioning's mask, configure() keeps `sched` and the shape.)
    def drop_graphs_and_shape(self) -> None:
        """The pipeline installed or removed an adapter set: setup() must run again, the adapter rank sizes the modulation scratch."""
        self.graphs, self.shape = {}, None

    def drop_conditioning(self) -> None:
        """LxFluxTransformer.invalidate_conditioning: the conditioning is over, its mask and its prepared schedule go with it."""
        self.cond_ready, self.cond_mask, self.sched, self.step_cache = False, None, None, None

    def set_adapter_weights(self, weights: Optional[Dict]) -> None:
        """{adapter name: w}: w a float, or one float per image of the conditioning (a sequence or 1-D tensor of length B, checked by
        set_conditioning). Adapters not named weigh 1; engine.lora_scale multiplies on top. None / {}: every adapter at 1."""
        new = self._checked_adapter_weights(weights)
        if new != self.adapter_weights:
            self.adapter_weights = new
            self._adapters_changed()

    def _checked_adapter_weights(self, weights: Optional[Dict]) -> Dict[str, object]:
        """set_adapter_weights' argument as {name: float | tuple of floats}; ValueError for a name that is not loaded."""
        from .weights import list_adapters
        new = {}
        for name, w in (weights or {}).items():
            if isinstance(w, torch.Tensor):
                w = w.detach().reshape(-1).tolist() if w.dim() else float(w)
            new[str(name)] = tuple(float(v) for v in w) if isinstance(w, (list, tuple)) else float(w)
        unknown = [n for n in new if n not in list_adapters(self.w)]
        if unknown:
            raise ValueError(f"unknown adapter{'s' if len(unknown) > 1 else ''} {', '.join(map(repr, unknown))}: loaded adapters are "
                             f"{list_adapters(self.w)}")
        return new

    def set_adapters(self, names, weights: Optional[Dict] = None) -> None:
        """Run with the loaded adapters `names` (weights.set_active_adapters: a name or a list, stacked in this order) at `weights`
        (set_adapter_weights). A call that raises leaves the active set, the weights and the engine's state as they were."""
        from .weights import active_adapters, set_active_adapters
        names = [names] if isinstance(names, str) else list(names)
        new = self._checked_adapter_weights(weights)
        if names != active_adapters(self.w):
            set_active_adapters(self.w, names)            # (atomic: raises before it changes anything)
            self._adapters_changed()
        if new != self.adapter_weights:
            self.adapter_weights = new
            self._adapters_changed()

    def adapter_weights_key(self):
        """What the adapter weights contribute to a conditioning's identity (tranformer_forward's cache key)."""
        return tuple(sorted(self.adapter_weights.items())) + ((self.adapter_weight_tiles,) if self.adapter_weight_tiles != 1 else ())

    def _lora_tables(self, B: int) -> None:
        """lora_w / lora_w_ns of a conditioning with B images (see __init__), in engine-owned buffers whose address depends on the
        table's shape alone. Raises ValueError for a per-image weight whose length is not B."""
        from .weights import _registry
        self.lora_w = self.lora_w_ns = None
        reg = _registry(self.w)
        rows, ones = [[] for _ in range(B)], True
        for name in self.w.active:
            w = self.adapter_weights.get(name, 1.0)
            if isinstance(w, tuple) and len(w) * self.adapter_weight_tiles == B:
                w = w * self.adapter_weight_tiles
            if isinstance(w, tuple) and len(w) != B:
                raise ValueError(f"adapter {name!r}: {len(w)} per-image weights for a batch of {B} images")
            for b in range(B):
                v = w[b] if isinstance(w, tuple) else w
                ones = ones and v == 1.0
                rows[b] += [v] * reg[name].rank
        if not self.w.active or self.lora_scale == 0.0 or (ones and self.lora_scale == 1.0):
            return
        R = len(rows[0])
        for which, s in (("w", self.lora_scale), ("ns", 1.0)):
            if ones and s == 1.0:
                continue
            buf = self._lora_w_bufs.get((B, R, which))
            if buf is None:
                buf = self._lora_w_bufs[(B, R, which)] = torch.zeros(B, R, dtype=torch.float32, device=self.device)
            buf.copy_(torch.tensor([[s * v for v in row] for row in rows], dtype=torch.float32))
            setattr(self, "lora_w" if which == "w" else "lora_w_ns", buf)

    def _scale_lora(self, T: torch.Tensor, segs, n_slab: int = 1, table: Optional[torch.Tensor] = None) -> None:
        """The adapter weights on freshly written adapter scratch: T [rows, columns] (slab 0; n_slab slabs TLs.stride(0) apart), segs =
        [(first row, rows, rows per image), ...] relative to T's first row. Nothing is launched while every factor is 1."""
        table = self.lora_w if table is None else table
        if table is not None:
            assert table.shape[1] == self.cfg.lora_r and n_slab <= self.TLs.shape[0], (table.shape, self.cfg.lora_r, n_slab)
            ops.lora_scale_rows(T, segs, table, self.cfg.lora_r, n_slab=n_slab, slab_stride=self.TLs.stride(0) if n_slab > 1 else 0)

    def _embed_segs(self, rows: int):
        """An embedder's input rows (B images x tokens, image-major) as the one lx_lora_scale_rows segment they are."""
        return [(0, rows, max(rows // self.B, 1))]

    def _lora_segs(self, r0: int, n: int):
        """The token streams inside rows [r0, r0 + n) of the adapter scratch as lx_lora_scale_rows segments (rows relative to r0)."""
        return [(s.row0 - r0, self.B * s.len, s.len) for s in self.streams if s.len > 0 and r0 <= s.row0 < r0 + n]

    def gemm_ws(self) -> Optional[torch.Tensor]:
        """The caller-owned GEMM workspace of lx_gemm_bf16_ws (what selects the default launch plans: lx_gemm4_kernel and its split form).
        One per stream that may have such a launch in flight: this engine runs on one stream at a time."""
        if not self.pair_plan:
            return None
        if self._gemm_ws is None:
            if torch.cuda.is_current_stream_capturing():
                return None                      # never allocate inside a capture; the eager warm-up pass allocates it
            self._gemm_ws = ops.gemm_workspace(self.device)
        return self._gemm_ws

    def check_status(self, sync: bool = True) -> None:
        """Raises LxError if a split-tile workgroup timed out (the results of that step are invalid); the workspace plans are then
        switched off for this engine, so a retry takes the plain plans. sync=True drains the stream and checks now. sync=False
        costs no synchronisation: it looks at the error word copied to pinned host memory by the previous call (if that copy has
        landed) and enqueues the next copy -- generate() does this once per image, so a time-out surfaces at most one image late."""
        if self._gemm_ws is None:
            return
        if sync:
            try:
                ops.gemm_workspace_status(self._gemm_ws)      # (resets the flags and the error word when it reports)
            except Exception:
                self.pair_plan, self.graphs = False, {}
                self._err_word.drop()
                raise
            return
        if self._err_word.take():
            self.check_status(sync=True)              # resets the workspace and raises
        n = self._gemm_ws.numel()
        self._err_word.request(self._gemm_ws[n - 64 * 4: n - 63 * 4].view(torch.int32))      # [slots | 256 flags | error word + pad]

    # row views ---------------------------------------------------------------------------------------
    def rows(self, buf: torch.Tensor, stream: str) -> torch.Tensor:
        s = self.stream[stream]
        return buf[s.row0:s.row0 + self.B * s.len]

    def _streams(self) -> List[Stream]:
        """Token streams with rows in this forward (cond_skip: the condition stream's keys / values come from the per-layer cache)."""
        return [s for s in self.streams if s.len > 0 and not (self.cond_skip and s.name == "cond")]

    def _all_streams(self) -> List[Stream]:
        return [s for s in self.streams if s.len > 0]

    @staticmethod
    def _w_rows(W: torch.Tensor, rows: Optional[slice]) -> torch.Tensor:
        """A row range of a weight image. Row blocks of 256 are contiguous in the tiled image: the slice is a tiled image too."""
        if rows is None:
            return W
        V = W[rows]
        if getattr(W, "lx_tiled", False):
            V.lx_tiled = True
        return V

    # ------------------------------------------------------------------------------------------ helpers
    def _lin_skinny(self, x, name, out, act_in=0, act_out=0, accumulate=False):
        lo = self.w.t.get(name + ".w_lo") if self.precise else None
        if lo is None:
            ops.linear_skinny(x, self.w.t[name + ".w"], self.w.t[name + ".b"], out, act_in=act_in, act_out=act_out,
                              accumulate=accumulate)
            return
        # precise mode, weight not bf16-representable: a second pass over its rounding residual, activation afterwards
        ops.linear_skinny(x, self.w.t[name + ".w"], self.w.t[name + ".b"], out, act_in=act_in, accumulate=accumulate)
        ops.linear_skinny(x, lo, None, out, act_in=act_in, accumulate=True)
        if act_out == 1:
            torch.nn.functional.silu(out, inplace=True)

    def _time_text_embed(self, t1000: torch.Tensor, out: torch.Tensor, base: torch.Tensor) -> None:
        """out = base + timestep_embedder(sinusoid(t1000))   (CombinedTimestep[Guidance]TextProjEmbeddings)."""
        ops.timestep_embed(t1000, self.tproj)
        self._lin_skinny(self.tproj, "tte.timestep_embedder.linear_1", self.thid, act_out=1)
        out.copy_(base)
        self._lin_skinny(self.thid, "tte.timestep_embedder.linear_2", out, accumulate=True)

    def _compute_mods(self, temb: torch.Tensor, out: torch.Tensor, lora: bool, lora_only: bool = False) -> None:
        """All AdaLN modulation vectors of the model from one weight-streaming launch (+ rank-r LoRA glue)."""
        w = self.w
        if not lora_only:
            ops.linear_skinny(temb, w.t["mod.w"], w.t["mod.b"], out, act_in=1)
            if self.precise and "mod.w_lo" in w.t:
                ops.linear_skinny(temb, w.t["mod.w_lo"], None, out, act_in=1, accumulate=True)
        if lora and "mod.lora_down" in w.t and self.lora_scale != 0.0:
            cfg, r, D = self.cfg, self.cfg.lora_r, self.cfg.inner_dim
            nb = cfg.num_layers + cfg.num_single_layers
            rows = temb.shape[0]
            tm = self.tmod[:, : nb * r] if rows == self.B else torch.zeros(rows, nb * r, dtype=torch.float32, device=self.device)
            ops.linear_skinny(temb, w.t["mod.lora_down"], None, tm, act_in=1)
            if self.precise and "mod.lora_down_lo" in w.t:
                ops.linear_skinny(temb, w.t["mod.lora_down_lo"], None, tm, act_in=1, accumulate=True)
            self._scale_lora(tm, [(0, rows, 1)])          # (rows of a whole schedule are step * B + sample: the table's rows wrap)
            for idx in range(nb):
                if idx < cfg.num_layers:
                    base, width = cfg.mod_base_double(idx), 6 * D
                else:
                    base, width = cfg.mod_base_single(idx - cfg.num_layers), 3 * D
                ops.linear_f32(tm[:, idx * r:], w.t[f"mod.lora_up.{idx}"], None, out[:, base:], M=rows, N=width, K=r,
                               ldx=tm.stride(0), ldy=out.stride(0), accumulate=True)

    def prepare_schedule(self, t_sched) -> None:
        """Timestep embedding and every image/text modulation vector for ALL steps of a schedule in one weight pass.

        The modulation Linears hold 6.5 GB of weights (FLUX.1-dev) and see one row per sample and step; evaluated step by
        step they re-stream those weights from HBM 28 times per image. Rows are independent in the weight-streaming kernel, so
        the batched result is bit-identical to the per-step one. `t_sched`: 1-D, the values later passed as `timestep`
        (0..1). Needs set_conditioning() first (temb_base) and is invalidated by it."""
        if not self.cond_ready:
            raise RuntimeError("call set_conditioning() before prepare_schedule()")
        cfg, dev, f32 = self.cfg, self.device, torch.float32
        host = None if isinstance(t_sched, torch.Tensor) and t_sched.is_cuda else tuple(float(v) for v in torch.as_tensor(t_sched, dtype=f32).reshape(-1).tolist())
        t = torch.as_tensor(t_sched, dtype=f32).reshape(-1).to(dev)
        n, B, D = t.numel(), self.B, cfg.inner_dim
        if n * B * cfg.n_mod * 4 > (4 << 30):        # keep the table (and its hi/lo twin) bounded; the per-step path handles the rest
            self.sched = None
            return
        t1000 = torch.mul(t, 1000.0).repeat_interleave(B).contiguous()          # row = step * B + sample
        tproj = torch.empty(n * B, 256, dtype=f32, device=dev)
        thid = torch.empty(n * B, D, dtype=f32, device=dev)
        temb_all = self.temb_base.repeat(n, 1).contiguous()
        ops.timestep_embed(t1000, tproj)
        self._lin_skinny(tproj, "tte.timestep_embedder.linear_1", thid, act_out=1)
        self._lin_skinny(thid, "tte.timestep_embedder.linear_2", temb_all, accumulate=True)
        # n*B rows are too many for the weight-streaming GEMV kernel (every wave re-loads all x rows: 13.7 ms) and the right size
        # for one 128-row MFMA tile row: the 6.5 GB of modulation weights stream once (~1.5 ms). The activations keep fp32-class
        # accuracy as stacked bf16 hi / lo halves of silu(temb) whose two result halves are added (error ~2^-17 relative).
        xs = torch.nn.functional.silu(temb_all)
        hi = xs.to(torch.bfloat16)
        lo = (xs - hi.float()).to(torch.bfloat16)
        acc2 = torch.empty(2 * n * B, cfg.n_mod, dtype=f32, device=dev)
        ops.gemm([ops.gemm_desc(torch.cat([hi, lo], 0).contiguous(), self.w.t["mod.w"], acc2, epilogue=LX_EPI_STORE_F32)])
        mods_all = acc2[: n * B]
        mods_all += acc2[n * B:]
        if self.precise and "mod.w_lo" in self.w.t:          # + silu(temb)_hi . W_lo^T: the third cross term
            acc3 = torch.empty(n * B, cfg.n_mod, dtype=f32, device=dev)
            ops.gemm([ops.gemm_desc(hi.contiguous(), self.w.t["mod.w_lo"], acc3, epilogue=LX_EPI_STORE_F32)])
            mods_all += acc3
        mods_all += self.w.t["mod.b"]
        if self.latent_lora and "mod.lora_down" in self.w.t:
            self._compute_mods(temb_all, mods_all, lora=True, lora_only=True)
        self.sched = (host if host is not None else tuple(float(v) for v in t.tolist()), mods_all.view(n, B, cfg.n_mod))

    def _setup_nomax(self) -> None:
        """Bounded-score attention (include/lx.h LX_ATTN_Q_LOG2 | LX_ATTN_BOUNDED). q and k leave the per-head RMSNorm (block.py:60-67)
        with |q| <= sqrt(128) max|norm_q|, and RoPE is a rotation, so |q.k| / sqrt(128) * log2 e <= 16.33 max|norm_q| max|norm_k|: when
        that plus the largest finite bias stays under 100 the softmax needs no running maximum (exp2 cannot overflow, nor can a row sum
        leave fp32's normal range), and with scale * log2 e folded into the norm_q weights the kernel's exp2 argument is the score MFMA's
        output itself. Decided PER LAYER (the joint attention of a double block mixes both streams' norms: the larger of each pair
        counts); a layer whose weights break the bound keeps the max-tracking kernel. The scaled weights and the bounds are made once per
        weight set (one host sync, outside any capture); LX_ATTN_NOMAX=0 disables."""
        self.attn_nomax = False
        if self.model_config.get("attn_fp8", False) and not self.precise:
            return                                                 # (e4m3 probabilities need the running maximum: their range is 2^17)
        if (self.precise and not self.precise_attn_split) or os.environ.get("LX_ATTN_NOMAX", "1") == "0":
            return
        w = self.w
        tab = getattr(w, "q_log2", None)
        if tab is None:
            layers = []
            for n in w.t:
                if n.endswith(".wq"):
                    p = n[:-3]
                    layers.append((w.t[n], w.t[p + ".wk"], w.t.get(p + ".wq_txt", w.t[n]), w.t.get(p + ".wk_txt", w.t[p + ".wk"])))
            if not layers:
                return
            mx = torch.stack([torch.stack([torch.maximum(a.abs().max(), c.abs().max()), torch.maximum(b.abs().max(), d.abs().max())])
                              for a, b, c, d in layers]).tolist()
            tab = {}
            for (a, b, c, d), (qm, km) in zip(layers, mx):
                tab[a.data_ptr()] = {"wq": a, "wk": b, "wq_txt": c, "wk_txt": d, "bound": 128.0 * ops.Q_LOG2_FACTOR * qm * km,
                                     "scaled": {a.data_ptr(): (a * ops.Q_LOG2_FACTOR).contiguous(), c.data_ptr(): (c * ops.Q_LOG2_FACTOR).contiguous()}}
            w.q_log2 = tab
            w.q_log2_version = getattr(w, "q_log2_version", 0)
        fin = [abs(v) for row in self.attn_bias.values() for v in row.values() if v > -1e37]
        self._nomax_room = 100.0 - max(fin, default=0.0) * 1.4426950408889634
        self.attn_nomax = any(e["bound"] <= self._nomax_room for e in tab.values())      # (some layer of this forward runs the bounded kernel)

    def _layer_nomax(self, wq: torch.Tensor) -> bool:
        """Does the layer whose image-stream norm_q weight is `wq` run the bounded-score kernel in this forward?"""
        if not self.attn_nomax:
            return False
        e = getattr(self.w, "q_log2", {}).get(wq.data_ptr())
        return e is not None and e["wq"] is wq and e["bound"] <= self._nomax_room       # (an unknown / replaced weight: max tracking)

    def _qn(self, w_q: torch.Tensor, wq: torch.Tensor) -> torch.Tensor:
        """The norm_q weight (`w_q`: the layer's image- or text-stream one) an attention launch of this forward is fed: with scale * log2 e
        folded in when the layer (named by its image-stream weight `wq`) runs the bounded-score kernel."""
        return self.w.q_log2[wq.data_ptr()]["scaled"][w_q.data_ptr()] if self._layer_nomax(wq) else w_q

    def _attn_bias(self) -> Dict[str, Dict[str, float]]:
        """block.py:106-128 as a (query stream, key stream) table: 0, log(c_factor) or -inf."""
        names = ("txt", "img", "cond")
        b = {q: {k: 0.0 for k in names} for q in names}
        mc = self.model_config
        if self.C:
            if not mc.get("union_cond_attn", True):
                for o in ("txt", "img"):
                    b[o]["cond"] = NEG_INF
                    b["cond"][o] = NEG_INF
            elif mc.get("independent_condition", False):
                b["cond"]["txt"] = b["cond"]["img"] = NEG_INF
            if self.c_factor is not None:            # evaluated last in the reference: replaces any boolean mask
                lb = math.log(self.c_factor)
                b = {q: {k: 0.0 for k in names} for q in names}
                for o in ("txt", "img"):
                    b[o]["cond"] = lb
                    b["cond"][o] = lb
        return b

    # --------------------------------------------------------------------------------- the caller's attention mask
    def user_mask(self, mask: torch.Tensor, B: int, S: int, C: int, model_config, c_factor: Optional[float]) -> Optional[torch.Tensor]:
        """The caller's attention_mask as lx_attn_fwd_masked takes it ([Bm, Hm, Sq, S]), or None where the reference replaces it
        (block.py:106-128: union_cond_attn = False or independent_condition with a condition stream, or a c_factor -- the engine's
        segment bias table then carries the reference's own mask)."""
        mc = model_config or {}
        if c_factor is not None or (C and (not mc.get("union_cond_attn", True) or mc.get("independent_condition", False))):
            return None
        if mask.dim() > 4:
            raise ValueError(f"attention_mask: rank {mask.dim()} (expected 2..4)")
        if mask.device.type != self.device.type or (self.device.index is not None and mask.device.index != self.device.index):
            raise ValueError(f"attention_mask: on {mask.device}, the engine runs on {self.device}")
        if mask.dtype not in (torch.bool, torch.float32, torch.bfloat16, torch.float16):
            raise ValueError(f"attention_mask: dtype {mask.dtype} (expected bool, float32, bfloat16 or float16)")
        m = mask
        while m.dim() < 4:
            m = m.unsqueeze(0)
        H = self.cfg.num_attention_heads
        if m.shape[0] not in (1, B) or m.shape[1] not in (1, H) or m.shape[2] not in (1, S) or m.shape[3] != S:
            raise ValueError(f"attention_mask: shape {tuple(mask.shape)} does not broadcast to [B={B}, H={H}, S={S}, S={S}] "
                             "over the concatenated [text | image | condition] sequence")
        return m

    def _attn_segments(self, streams: Sequence[Stream], norms=None):
        """(seg_row0, seg_len, seg_vt0, bias, qsegs) of an attention launch over `streams`, as the mask prep, the q / k / v passes and the
        attention kernels describe them. bias: the 3x3 (query segment, key segment) table. qsegs, given norms = (wq, wk, wq_txt, wk_txt):
        per segment (row0, len, vt0, norm_q weight (_qn), norm_k weight, cos, sin), the RoPE tables sliced to the segment's tokens."""
        bias = [[0.0] * 3 for _ in range(3)]
        for qi, q in enumerate(streams):
            for ki, k in enumerate(streams):
                bias[qi][ki] = self.attn_bias[q.name][k.name]
        return [s.row0 for s in streams], [s.len for s in streams], [s.vt0 for s in streams], bias, self._qsegs(streams, *norms) if norms else []

    def _qsegs(self, streams: Sequence[Stream], wq, wk, wq_txt, wk_txt) -> List:
        qsegs, off = [], 0
        for s in streams:
            if s.name == "cond":
                cos, sin = self.cos_cond, self.sin_cond
            elif self.cos_main is None:
                cos = sin = None
            else:
                cos, sin = self.cos_main[off:off + s.len], self.sin_main[off:off + s.len]
                off += s.len
            qsegs.append((s.row0, s.len, s.vt0, self._qn(wq_txt if s.name == "txt" else wq, wq), wk_txt if s.name == "txt" else wk, cos, sin))
        return qsegs

    def _prep_cond_mask(self) -> None:
        """ONE lx_attn_mask_prep per conditioning, into an engine-owned workspace (allocated here, outside any stream capture; kept while
        it is large enough, so the step graphs that hold its address stay valid from image to image)."""
        _, seg_len, seg_vt0, bias, _ = self._attn_segments(self._all_streams())
        kw = dict(B=self.B, H=self.cfg.num_attention_heads, seg_len=seg_len, seg_vt0=seg_vt0, bias=bias)
        need = ops.attn_mask_workspace_bytes(self.cond_mask, **kw)
        if self._mask_ws is None or self._mask_ws.numel() < need:
            self._mask_ws = torch.empty(max(need, 1), dtype=torch.uint8, device=self.device)
        ops.attn_mask_prep(self.cond_mask, self._mask_ws, **kw)

    # --------------------------------------------------------------------------------- step-invariant part
    def set_conditioning(self, prompt_embeds, pooled, guidance, txt_ids, img_ids, condition_latents=None,
                         condition_ids=None, c_t: float = 0.0, model_config: Optional[Dict] = None,
                         c_factor: Optional[float] = None, attention_mask: Optional[torch.Tensor] = None) -> None:
        """attention_mask: what attn_forward takes (rank 2..4, broadcastable to [1|B, 1|H, 1|S, S] over [text | image | condition], bool or
        additive float, on the device), for every attention launch of the forwards of this conditioning. Used under the reference's rules
        only (user_mask); refused in precise and attn_fp8 modes. A call that raises leaves the engine without a mask and unconditioned."""
        cfg, w, dev = self.cfg, self.w, self.device
        B, T = prompt_embeds.shape[0], prompt_embeds.shape[1]
        N = img_ids.shape[0]
        C = 0 if condition_latents is None else condition_latents.shape[1]
        self.cond_mask, self.cond_ready, self.step_cache = None, False, None
        step_cache = step_cache_config(model_config)          # (a bad threshold or coefficient list: ValueError)
        refuse_wide_lora_modes(w, model_config, self.precise_default)
        self._lora_tables(B)             # (a per-image adapter weight of another length than B: ValueError)
        mask = None
        if attention_mask is not None:
            mask_argument(attention_mask)
            refuse_masked_modes(model_config, self.precise_default)
            mask = self.user_mask(attention_mask, B, T + N + C, C, model_config, c_factor)
        self.setup(B, T, N, C)
        self.gemm_ws()                   # allocated here, outside any stream capture
        self._select_mode(model_config, c_factor)
        normalise_model_config(self.model_config)             # (it goes into the step graphs' key, which is hashed)
        if step_cache is not None:
            self._setup_step_cache()
        if self.model_config.get("add_cond_attn", False) and C and C != N:
            raise ValueError("add_cond_attn adds the condition attention output onto the image stream: needs C == N")
        f32 = torch.float32
        # context_embedder(prompt_embeds) -> cached text rows; x_embedder(condition_latents) with LoRA active -> cached condition rows
        self.mode.embed(prompt_embeds.reshape(B * T, -1), "context_embedder", self.X_txt_init, lora=False)
        if C:
            self.mode.embed(condition_latents.reshape(B * C, -1), "x_embedder", self.X_cond_init, lora=True)
        # RoPE tables: [text; image] and condition (transformer.py:130-134)
        ids = torch.cat([txt_ids.to(dev, f32).reshape(-1, 3), img_ids.to(dev, f32).reshape(-1, 3)], 0)
        # tables live in persistent buffers: the captured step graph holds their addresses
        self.cos_main, self.sin_main = ops.rope_table(ids, cfg.axes_dims_rope, out=(self.rope_main[0], self.rope_main[1]))
        if C:
            self.cos_cond, self.sin_cond = ops.rope_table(condition_ids.to(dev, f32).reshape(-1, 3), cfg.axes_dims_rope,
                                                          out=(self.rope_cond[0], self.rope_cond[1]))
        self._rope_pairs(check=False)
        # temb_base = text_embedder(pooled) [+ guidance_embedder(sinusoid(1000 g))]
        pooled = pooled.to(device=dev, dtype=f32).contiguous()
        self._lin_skinny(pooled, "tte.text_embedder.linear_1", self.thid, act_out=1)
        self._lin_skinny(self.thid, "tte.text_embedder.linear_2", self.temb_base)
        if cfg.guidance_embeds:
            if guidance is None:
                raise ValueError("this transformer has guidance_embeds=True: pass `guidance`")
            g1000 = (guidance.to(device=dev, dtype=f32) * 1000.0).contiguous()
            ops.timestep_embed(g1000, self.tproj)
            self._lin_skinny(self.tproj, "tte.guidance_embedder.linear_1", self.thid, act_out=1)
            self._lin_skinny(self.thid, "tte.guidance_embedder.linear_2", self.temb_base, accumulate=True)
        # cond_temb and all condition-stream modulations (LoRA on norm1.linear / norm.linear)
        if C:
            ct = torch.full((B,), float(c_t) * 1000.0, dtype=f32, device=dev)
            self._time_text_embed(ct, self.cond_temb, self.temb_base)
            self._compute_mods(self.cond_temb, self.cmods, lora=True)
        self.attn_bias = self._attn_bias()
        self._setup_nomax()
        if mask is not None:
            self.cond_mask = mask
            self._prep_cond_mask()
        self.cond_ready = True
        self.cond_cached = False          # a new condition stream: the per-layer key / value images are stale
        self.sched = None
        self.step_cache = StepCacheState(*step_cache) if step_cache is not None else None

    # ------------------------------------------------------------------------------------------ arithmetic mode
    def _select_mode(self, model_config: Optional[Dict], c_factor: Optional[float], gemm_fp8: bool = True) -> None:
        """model_config -> latent_lora / precise / gemm_fp8 / the operand format, the operand mode object (`mode`, modes.py) and the
        buffers and weight images those modes need: all of them allocated here, by set_conditioning() or configure(), never first inside
        a capture. gemm_fp8 = False: the caller has no e4m3 GEMM path (the block-level entry points)."""
        self.model_config = dict(model_config or {})
        self.c_factor = c_factor
        self.latent_lora = bool(self.model_config.get("latent_lora", False))
        self.precise = bool(self.model_config.get("precise", self.precise_default))
        if self.precise:
            self._setup_precise()
        self.gemm_fp8 = gemm_fp8 and bool(self.model_config.get("gemm_fp8", False)) and not self.precise
        if self.gemm_fp8:
            self._setup_fp8()
        self.mode = self.mode_split if self.precise else self.mode8 if self.gemm_fp8 else self.mode16
        self._pick_operands()
        if self.model_config.get("attn_fp8", False) and not self.precise:
            self._fp8_images()

    def _pick_operands(self) -> None:
        """model_config["operands"]: "bf16" (default) | "fp16" -- the 16-bit format of every GEMM operand image of the forward."""
        fmt = str(self.model_config.get("operands", self.operands_default)).lower()
        if fmt not in ("bf16", "fp16", "f16", "float16", "bfloat16"):
            raise ValueError(f'model_config["operands"] = {fmt!r}: "bf16" or "fp16"')
        self.f16 = fmt in ("fp16", "f16", "float16") and not self.precise and not self.gemm_fp8
        if self.f16:
            self._setup_f16()
        elif self.w16:
            self.w16, self.graphs = {}, {}                 # leaving the fp16 operand mode: its 17 GB of weight images (and the graphs that read them) go

    def _op(self, t: torch.Tensor) -> torch.Tensor:
        """a (slice of a) 16-bit operand buffer in the format the GEMMs of this forward read"""
        return t.view(torch.float16) if self.f16 else t

    def _W(self, name: str) -> torch.Tensor:
        return self.w16[name] if self.f16 else self.w.t[name + ".w"]

    def _down(self, name: str, lo) -> torch.Tensor:
        return self.w16[name + ".down"] if self.f16 else lo.down

    def _f16_kw(self) -> Dict:
        return dict(f16=True, f16_ovf=self.f16_ovf) if self.f16 else {}

    # ------------------------------------------------------------------------------------------ building blocks
    def _ln_segs(self, base_by_stream: Dict[str, int], shift_off: int, scale_off: int):
        """The segment list of an AdaLN LayerNorm + modulation launch over every stream of this forward: per stream (first row, rows, rows per
        sample, shift vectors, scale vectors), the vectors `shift_off` / `scale_off` past the stream's modulation base."""
        return [(s.row0, self.B * s.len, s.len, s.mods[:, base_by_stream[s.name] + shift_off:], s.mods[:, base_by_stream[s.name] + scale_off:])
                for s in self._streams()]

    def _lora_rows(self, include_txt: bool):
        """(first row, row count) of the rows that run with the adapter on: the condition stream always; with
        model_config["latent_lora"] also the image stream and, where text shares the module (single blocks), text.
        None: no such rows in this forward (no condition stream or cond_skip, without latent_lora)."""
        end = self.r_cond if self.cond_skip else self.M
        if self.latent_lora:
            r0 = self.r_txt if include_txt else self.r_img
            return r0, end - r0
        if self.cond_skip or self.C == 0:
            return None
        return self.r_cond, self.M - self.r_cond

    # An adapter term is handed to a grouped launch as (adapter, slabs of TLs that hold its down-projection, first row they hold), under the
    # keyword `lora`, in all three modes. (None, 0, 0): nothing to add. Each operand mode (modes.py) computes it from its operand image.
    NO_LORA = (None, 0, 0)

    def _launch_streams(self, desc, workspace, main: str, txt: Optional[str], *, epilogue: int, w_rows: Optional[Dict[str, slice]] = None,
                        t_col0: int = 0, gate_off: Optional[Dict[str, int]] = None, lora_mod_cols: int = 0, lora_toff_max: int = 0,
                        only: Optional[Sequence[str]] = None, lora=None) -> None:
        """One grouped GEMM launch over the token streams, in any operand mode. `main` weights serve image+condition rows, `txt` the text
        rows (None => text rows use `main` too: single blocks). `only` restricts the launch to those streams, `w_rows[s]` to that range of
        the weight's rows (= output columns, written to the first columns of the stream's rows of C) for stream s, and `t_col0` names the
        first column of the adapter slabs that belongs to that range. `gate_off[s]`: the stream's gate vector in its modulation buffer.
        `lora`: see NO_LORA. The mode supplies desc(stream, weight name, row range, **kw) -> GemmDesc: its operand views of A and C, its
        weight lookup and its descriptor factory; and the workspace it launches with."""
        lo, n_slabs, lr0 = lora if lora is not None else self.NO_LORA
        probs = []
        for s in self._streams():
            if only is not None and s.name not in only:
                continue
            name = txt if (s.name == "txt" and txt is not None) else main
            rows = w_rows.get(s.name) if w_rows else None
            bias = self.w.t[name + ".b"]
            kw = dict(bias=bias if rows is None else bias[rows], epilogue=epilogue, rows_per_batch=s.len)
            if gate_off is not None:
                kw["gate"] = s.mods[:, gate_off[s.name]:]
            if lo is not None and name == main and s.row0 >= lr0 and (s.name == "cond" or (s.name == "img" and self.latent_lora) or
                                                                       (s.name == "txt" and self.latent_lora and txt is None)):
                kw.update(lora_t=self.TL[s.row0:s.row0 + self.B * s.len, t_col0:], lora_up=lo.up if rows is None else lo.up[rows],
                          lora_mod_cols=lora_mod_cols, lora_toff_max=lora_toff_max, lora_nsplit=n_slabs, lora_split_stride=self.TLs.stride(0))
            probs.append(desc(s, name, rows, **kw))
        ops.gemm(probs, workspace)

    def _lora_wanted(self, only: Optional[Sequence[str]]) -> bool:
        """Can a launch over `only` have adapter rows at all? (Which rows: _lora_rows.)"""
        return only is None or "cond" in only or self.latent_lora

    def _qkv_kw(self, s: Stream, qkv) -> Dict:
        """What the projection launch's fused epilogue (LX_EPI_QKV) needs for stream s: norm weights, the stream's (cos, sin) pairs and
        where k, q and V^T go."""
        rope = self.rope_cs_cond if s.name == "cond" else (self.rope_cs_main[: self.T] if s.name == "txt" else self.rope_cs_main[self.T:])
        kw = dict(norm_q=self._qn(qkv[2] if s.name == "txt" else qkv[0], qkv[0]), norm_k=qkv[3] if s.name == "txt" else qkv[1], rope=rope,
                  vt=self.VT, vt_pos0=s.vt0, d=self.cfg.inner_dim)
        if self.model_config.get("attn_fp8", False):      # e4m3 q / k / V^T images straight from the accumulators
            self._fp8_images()
            kw.update(q8=self.rows(self.Q8, s.name), k8=self.rows(self.K8, s.name), vt=self.VT8)
            if self.cond_cache and len(qkv) > 4:    # the per-layer e4m3 key / V^T images (q stays in the shared Q8)
                kw.update(k8=self.rows(self.KC8[qkv[4]], s.name), vt=self.VTC8[qkv[4]])
        elif self.cond_cache and len(qkv) > 4:      # per-layer key / V^T images: the condition rows' entries outlive the step
            kw.update(k=self.rows(self.KC[qkv[4]], s.name), vt=self.VTC[qkv[4]])
        return kw

    def _rope_pairs(self, check: bool) -> None:
        """(cos, sin) per rotary pair, [L, 128], for LX_EPI_QKV, and the decision whether the projections of this configuration
        use it (self.qkv_fused): bf16 kernel set, every stream a multiple of 32 tokens, heads in pairs, tables whose two
        entries of a pair agree (FluxPosEmbed's repeat_interleave; `check`: tables handed in by a caller are verified)."""
        D, rd = self.cfg.inner_dim, sum(self.cfg.axes_dims_rope)
        ok = (self.qkv_epilogue and D % 256 == 0 and rd == 128 and self.cos_main is not None
              and all(s.len % 32 == 0 for s in self._all_streams()) and (self.C == 0 or self.cos_cond is not None)
              and self.cos_main.shape[0] == self.T + self.N)
        if ok:
            pairs = [(self.rope_cs_main, self.cos_main, self.sin_main)]
            if self.C:
                pairs.append((self.rope_cs_cond, self.cos_cond, self.sin_cond))
            for dst, cos, sin in pairs:
                if check and not (torch.equal(cos[:, 0::2], cos[:, 1::2]) and torch.equal(sin[:, 0::2], sin[:, 1::2])):
                    ok = False
                    break
                dst[:, 0::2].copy_(cos[:, 0::2])
                dst[:, 1::2].copy_(sin[:, 0::2])
        self.qkv_fused = bool(ok)

    def _qkv_epilogue(self) -> bool:
        """The projection launch normalises / rotates k and q and writes V^T itself (LX_EPI_QKV). With model_config attn_fp8 (and bf16
        GEMMs) the same epilogue emits the e4m3 images the fp8 attention kernel reads instead of the bf16 ones (LX_QKV_FUSED_FP8=0:
        the separate lx_qkv_prep_fp8_segs pass)."""
        if not self.qkv_fused or self.precise or self.gemm_fp8:
            return False
        return True

    # ------------------------------ blocks: written once, against the operand mode's logical operands (modes.py: xn, attn, mlp, attn_mlp)
    def double_block(self, i: int) -> None:
        cfg, w, m = self.cfg, self.w, self.mode
        D = cfg.inner_dim
        b = cfg.mod_base_double(i)
        base = {"img": b, "cond": b, "txt": b + 6 * D}
        p = f"d{i}"
        ready = m.ln(base, 0, D, lora_for=p + ".qkv")                                       # norm1 / norm1_context (+ the q/k/v adapters' down-projection)
        nw = (w.t[p + ".wq"], w.t[p + ".wk"], w.t[p + ".wq_txt"], w.t[p + ".wk_txt"])
        fused = self._qkv_epilogue()
        m.gemm("xn", "qkv", p + ".qkv", p + ".qkv_txt", lora_mod_cols=D, lora_toff_max=2, lora=ready, **(dict(qkv=nw + (i,)) if fused else {}))
        m.attention(*nw, prepped=fused, layer=i)
        gate = {s: base[s] + 2 * D for s in base}
        lo, n_slabs, _ = m.gemm("attn", "x", p + ".out", p + ".out_txt", gate_off=gate)
        if self.C and self.model_config.get("add_cond_attn", False):                          # block.py:233-234
            if self.gemm_fp8:      # known gap: refused here, after the output projection above has been enqueued
                raise NotImplementedError("add_cond_attn is not wired into the fp8 GEMM path (use the bf16 or the precise mode)")
            kw = dict(lora_t=self.rows(self.TL, "cond"), lora_up=lo.up, lora_nsplit=n_slabs, lora_split_stride=self.TLs.stride(0)) if lo is not None else {}
            m.single("attn", "cond", p + ".out", self.rows(self.X, "img"), bias=w.t[p + ".out.b"], epilogue=LX_EPI_RESID_F32,
                     rows_per_batch=self.C, gate=self.cmods[:, gate["cond"]:], **kw)
        ready = m.ln(base, 3 * D, 4 * D, lora_for=p + ".ff1")                               # norm2 + (scale_mlp, shift_mlp)
        m.gemm("xn", "mlp", p + ".ff1", p + ".ff1_txt", lora=ready)                       # (ff.net.0.proj carries no adapter: the loaders refuse one)
        gate = {s: base[s] + 5 * D for s in base}
        m.gemm("mlp", "x", p + ".ff2", p + ".ff2_txt", gate_off=gate)

    def single_block(self, j: int, image_out_only: bool = False) -> None:
        """image_out_only: the caller reads nothing but the image rows of X afterwards (the LAST block of a forward: norm_out /
        proj_out run on the image tokens, transformer.py:243-252). The text and condition rows then still need their keys and
        values (the image queries attend to them) but neither queries, MLP branch nor output projection: 145 + 145 of the
        block's 580 GFLOP of GEMM work are skipped, with bit-identical image rows (how much a mode skips: its fused() / attention())."""
        cfg, w, m = self.cfg, self.w, self.mode
        D = cfg.inner_dim
        b = cfg.mod_base_single(j)
        base = {"img": b, "cond": b, "txt": b}
        p, layer = f"s{j}", cfg.num_layers + j
        ready = m.ln(base, 0, D, lora_for=p + ".fused", include_txt=True)
        nw = (w.t[p + ".wq"], w.t[p + ".wk"], w.t[p + ".wq"], w.t[p + ".wk"])
        fused = self._qkv_epilogue()
        m.fused(p, ready, image_out_only, nw + (layer,) if fused else None)                 # [k | v | q | mlp] of xn
        m.attention(*nw, prepped=fused, layer=layer, img_only=image_out_only)
        gate = {s: b + 2 * D for s in base}
        m.gemm("attn_mlp", "x", p + ".out", None, gate_off=gate, only=("img",) if image_out_only else None)

    # ------------------------------------------------------------------------------------------ fp8 GEMM path
    S_X8, S_Y8 = 16.0, 16.0      # fixed activation scales of the e4m3 images: AdaLN-normalised operand / attention output + MLP hidden

    def _setup_fp8(self) -> None:
        """The e4m3 mode's operand images XN8 u8 [M, D] and Y8 u8 [M, 5D] (what lives where: DESIGN.md section 8.2). Block weights are
        quantised once per weight set (per-output-row scale) from the packed bf16 weights and kept as tiled e4m3 images (+11.9 GB)."""
        if self.XN8 is None:
            D = self.cfg.inner_dim
            self.XN8 = torch.zeros(self.M, D, dtype=torch.uint8, device=self.device)
            self.Y8 = torch.zeros(self.M, 5 * D, dtype=torch.uint8, device=self.device)
        # (the images are quantised from the packed weights: a weight set overwritten in place -- dist.broadcast_packed_weights, which
        # moves weights_version -- gets new ones, like the fp16 images of _setup_f16; the graphs that hold the old ones' addresses go)
        key = (id(self.w), getattr(self.w, "weights_version", 0))
        if self.w8 and self._w8_key == key:
            return
        if self.w8:
            self.w8, self.graphs = {}, {}
        self._w8_key = key
        names = []
        for i in range(self.cfg.num_layers):
            names += [f"d{i}.{n}" for n in ("qkv", "qkv_txt", "out", "out_txt", "ff1", "ff1_txt", "ff2", "ff2_txt")]
        for j in range(self.cfg.num_single_layers):
            names += [f"s{j}.fused", f"s{j}.out"]
        for n in names:
            W = self.w.t[n + ".w"]
            W = ops.untile_weight(W) if getattr(W, "lx_tiled", False) else W
            W8, rs = ops.quantize_weight_fp8(W)
            self.w8[n] = ops.tile_weight(W8) if (W8.shape[0] % 256 == 0 and W8.shape[1] % 128 == 0) else W8
            self.w8[n + ".rs"] = rs

    def _cs(self, name: str, act_scale: float, rows: Optional[slice] = None) -> torch.Tensor:
        """col_scale of an fp8 GEMM: 1 / (activation scale x weight-row scale), cached per (weight, activation scale)."""
        key = f"{name}.cs{act_scale:g}"
        t = self.w8.get(key)
        if t is None:
            t = self.w8[key] = (self.w8[name + ".rs"] / act_scale).contiguous()
        return t if rows is None else t[rows]

    # ------------------------------------------------------------------------------------------ one step
    def embed_step_inputs(self, latents: torch.Tensor, timestep: torch.Tensor, mods_ready: bool = False) -> None:
        """x_embedder(latents), reset text/condition rows, temb(t) and every image/text modulation vector."""
        self.mode.embed(latents.reshape(self.B * self.N, -1), "x_embedder", self.rows(self.X, "img"), lora=self.latent_lora, step=True)
        self.rows(self.X, "txt").copy_(self.X_txt_init)
        if self.C and not self.cond_skip:
            self.rows(self.X, "cond").copy_(self.X_cond_init)
        if mods_ready:                      # self.mods already holds this step's row of the prepare_schedule() table
            return
        torch.mul(timestep.to(device=self.device, dtype=torch.float32), 1000.0, out=self.t1000)
        self._time_text_embed(self.t1000, self.temb, self.temb_base)
        self._compute_mods(self.temb, self.mods, lora=self.latent_lora)

    def final_layer(self) -> torch.Tensor:
        """norm_out (AdaLayerNormContinuous: chunk order scale, shift) + proj_out on the image rows."""
        cfg, w = self.cfg, self.w
        D, o = cfg.inner_dim, cfg.mod_base_out
        shift, scale = self.mods[:, o + D:], self.mods[:, o:]
        # the one LayerNorm that stays mode-specific: 16-bit operands get the plain one-segment kernel, which the modes' ln() does not describe
        if self.precise:
            ops.ln_modulate_split_segs(self.X, [(self.r_img, self.B * self.N, self.N, shift, scale)], self.XN2, self.mods.stride(0), D)
        else:
            ops.ln_modulate(self.rows(self.X, "img"), shift, scale, self._op(self.rows(self.XN, "img")),
                            rows_per_batch=self.N, mod_ld=self.mods.stride(0), **(dict(f16_ovf=self.f16_ovf) if self.f16 else {}))
        self.mode.single("xn", "img", "proj_out", self.out, bias=w.t["proj_out.b"], epilogue=LX_EPI_STORE_F32)
        return self.out.view(self.B, self.N, cfg.in_channels)

    def _forward_eager(self, latents: torch.Tensor, timestep: torch.Tensor, mods_ready: bool = False) -> torch.Tensor:
        self.embed_step_inputs(latents, timestep, mods_ready)
        self._blocks()
        return self.final_layer()

    def _blocks(self) -> None:
        for i in range(self.cfg.num_layers):
            self.double_block(i)
        last = self.cfg.num_single_layers - 1
        for j in range(self.cfg.num_single_layers):
            self.single_block(j, image_out_only=(j == last))

    def forward(self, latents: torch.Tensor, timestep: torch.Tensor, step_index: Optional[int] = None) -> torch.Tensor:
        """latents fp32 [B,N,in_channels], timestep [B] in 0..1 -> velocity fp32 [B,N,in_channels] (engine-owned buffer).

        The ~600 kernel launches of a step are captured ONCE per conditioning into a HIP graph (all of them are enqueued
        on torch's current stream through the C ABI, so stream capture sees them) and replayed for the remaining steps:
        the launch-bound gaps between the short kernels disappear.  LX_GRAPH=0 disables capture.

        `step_index`: position of `timestep` in the schedule given to prepare_schedule(); the step then takes its
        modulation vectors from that table instead of re-streaming the modulation weights. A conditioning with the step cache on
        (model_config step_cache_thresh) needs it: the step then runs as _forward_step_cache's three parts."""
        if not self.cond_ready:
            raise RuntimeError("call set_conditioning() before forward()")
        pre = step_index is not None and self.sched is not None
        if pre and not 0 <= step_index < len(self.sched[0]):
            raise IndexError(f"step_index {step_index} outside the prepared schedule of {len(self.sched[0])} steps")
        if self.f16:
            self._setup_f16()                # (a key comparison: weights broadcast or adapters installed after the conditioning get fresh images)
        timed = ops.TIMER is not None and ops.TIMER.next_call()      # event brackets need the eager launch path
        self.cond_cache = self._cond_cache_ok()
        skip = self.cond_cache and self.cond_cached            # the condition stream's keys / values of this conditioning are cached
        nl = self.cfg.num_layers + self.cfg.num_single_layers
        # (one set at a time: an engine that alternates between bf16 / fp16, attn_fp8 and precise conditionings drops the other mode's images
        #  -- and the step graphs that hold their addresses -- when it allocates this mode's)
        if self.cond_cache:                                    # this mode's per-layer key / V^T images (outside any capture)
            want = "KC2" if self.precise else "KC8" if self.model_config.get("attn_fp8", False) else "KC"
            if getattr(self, want) is None:
                if any(getattr(self, n) is not None for n in ("KC", "KC2", "KC8")):
                    self.KC = self.VTC = self.KC2 = self.VTC2 = self.KC8 = self.VTC8 = None
                    self.graphs = {}
                D, vts, bf16 = self.cfg.inner_dim, tuple(self.VT.shape), torch.bfloat16
                if want == "KC2":                              # key pairs (hi | lo), the hi and the lo V^T image
                    self.KC2 = torch.zeros(nl, self.M, 2 * D, dtype=bf16, device=self.device)
                    self.VTC2 = torch.zeros((nl, 2) + vts, dtype=bf16, device=self.device)
                elif want == "KC8":                            # e4m3 bytes: half the bf16 images
                    self.KC8 = torch.zeros(nl, self.M, D, dtype=torch.uint8, device=self.device)
                    self.VTC8 = torch.zeros((nl,) + vts, dtype=torch.uint8, device=self.device)
                else:
                    self.KC = torch.zeros(nl, self.M, D, dtype=bf16, device=self.device)
                    self.VTC = torch.zeros((nl,) + vts, dtype=bf16, device=self.device)
        if self.step_cache is not None:
            return self._forward_step_cache(latents, step_index, pre, not self.use_graph or timed, skip)
        if not self.use_graph or timed:
            if pre:
                self.mods.copy_(self.sched[1][step_index])
            self.cond_skip = skip
            try:
                out = self._forward_eager(latents, timestep, pre)
            finally:
                self.cond_skip = False
            self.cond_cached = self.cond_cache
            return out
        self.g_lat.copy_(latents.reshape(self.g_lat.shape))
        self.g_t.copy_(timestep.to(device=self.device, dtype=torch.float32).reshape(-1))
        key = self._graph_key(pre, skip)
        g = self.graphs.get(key)
        if g is None:
            mode = self._warm_mode(skip)
            self.cond_skip = skip
            try:
                if mode not in self._warmed:                          # lazy code-object loads / buffer allocations must not happen inside capture
                    self._forward_eager(self.g_lat, self.g_t, False)
                    torch.cuda.synchronize(self.device)
                    self._warmed.add(mode)
                if len(self.graphs) >= 4:
                    self.graphs.clear()
                g = torch.cuda.CUDAGraph()
                with torch.cuda.graph(g):
                    self._forward_eager(self.g_lat, self.g_t, pre)
            finally:
                self.cond_skip = False
            self.graphs[key] = g
        if pre:                                   # AFTER any warm-up pass above, which recomputes the per-step modulations
            self.mods.copy_(self.sched[1][step_index])
        g.replay()
        self.cond_cached = self.cond_cache
        return self.out.view(self.B, self.N, self.cfg.in_channels)

    def _graph_key(self, pre: bool, skip: bool):
        """The captured launches reference only engine-owned buffers, so one graph serves every image with the same shape and code path
        (LoRA rows, attention bias table, add_cond_attn ...): key it on exactly those."""
        return (self.shape, tuple(sorted(self.model_config.items())), self.c_factor, pre, self.pair_plan, self.precise, self.gemm_fp8, self.f16,
                getattr(self.w, "q_log2_version", 0),      # (a weight broadcast refreshes the scaled norm_q tensors and the per-layer bounds)
                getattr(self.w, "weights_version", 0),     # (... and moves this one unconditionally: dist.broadcast_packed_weights)
                self.cond_cache, skip, self.ln_lora, self.qkv_epilogue, self._w16_gen if self.f16 else 0,
                # the adapter set (its tensors' addresses are in the launches) and whether the adapter-weight tables exist (their launches)
                getattr(self.w, "lora_version", 0), tuple(None if t is None else t.data_ptr() for t in (self.lora_w, self.lora_w_ns)),
                # the masked launches hold the workspace's address and the mask's tile geometry (dtype, broadcast dims), never the mask itself:
                # a new mask of the same form is a new prep into the same workspace (set_conditioning), which the same graph then reads
                None if self.cond_mask is None else (self._mask_ws.data_ptr(), self.cond_mask.dtype, tuple(self.cond_mask.shape[:3])),
                self.step_cache is not None)               # (the entry is then the step's three parts: _forward_step_cache)

    def _warm_mode(self, skip: bool):
        """The kernel set of a forward, as the `_warmed` set remembers it."""
        return (self.precise, self.gemm_fp8, self.f16, bool(self.model_config.get("attn_fp8", False)), self.latent_lora, self.C > 0, skip,
                self.lora_w is not None or self.lora_w_ns is not None,
                None if self.cond_mask is None else self.cond_mask.dtype == torch.bool,      # (the bit and the bias form of the masked kernel)
                self.step_cache is not None)

    # ------------------------------------------------------------------------------------------ step cache
    def _setup_step_cache(self) -> None:
        """The step cache's buffers (see __init__), allocated by set_conditioning(), outside any capture."""
        if self.sc_m is None:
            rows, D, dev = self.B * self.N, self.cfg.inner_dim, self.device
            self.sc_m = torch.zeros(rows, D, dtype=torch.float32, device=dev)
            self.sc_R = torch.zeros(rows, D, dtype=torch.float32, device=dev)
            self.sc_rows = torch.zeros(rows, 2, dtype=torch.float32, device=dev)
            self.sc_sums = torch.zeros(2, dtype=torch.float64, device=dev)
        if self.sc_host is None:
            self.sc_host = torch.zeros(2, dtype=torch.float64).pin_memory()

    def _sc_probe(self, latents: torch.Tensor) -> None:
        """Part 1 of a step (self.mods holds the step's row of the schedule table): x_embedder(latents) into the image rows of X, and the
        distance of double block 0's image norm1 input from the previous step's (lx_ln_modulate_delta: sc_m is replaced, sc_sums written)."""
        D, b, x = self.cfg.inner_dim, self.cfg.mod_base_double(0), self.rows(self.X, "img")
        self.mode.embed(latents.reshape(self.B * self.N, -1), "x_embedder", x, lora=self.latent_lora, step=True)
        ops.ln_modulate_delta(x, self.mods[:, b:], self.mods[:, b + D:], self.sc_m, self.N, self.sc_rows, self.sc_sums, mod_ld=self.mods.stride(0))

    def _sc_body(self) -> torch.Tensor:
        """Part 2, a computed step: what _forward_eager runs after the image embed, with X0 = the embedded image rows kept (in sc_R) and
        replaced by the residual R = fl32(X_img - X0) once the blocks are through."""
        x = self.rows(self.X, "img")
        self.rows(self.X, "txt").copy_(self.X_txt_init)
        if self.C and not self.cond_skip:
            self.rows(self.X, "cond").copy_(self.X_cond_init)
        self.sc_R.copy_(x)
        self._blocks()
        torch.sub(x, self.sc_R, out=self.sc_R)
        return self.final_layer()

    def _sc_reuse(self) -> torch.Tensor:
        """Part 2, a skipped step: X_img = fl32(X0 + R) on the freshly embedded image rows. No block runs; the text and condition rows are
        not read by the final layer."""
        x = self.rows(self.X, "img")
        torch.add(x, self.sc_R, out=x)
        return self.final_layer()

    def _sc_rel(self) -> float:
        """The probe's two sums -> rel: one 16-byte synchronous read through the pinned host mirror."""
        self.sc_host.copy_(self.sc_sums, non_blocking=True)
        torch.cuda.current_stream(self.device).synchronize()
        s1, s2 = float(self.sc_host[0]), float(self.sc_host[1])
        return s1 / s2 if s2 > 0.0 else float("inf")

    def _forward_step_cache(self, latents: torch.Tensor, step_index: Optional[int], pre: bool, eager: bool, skip: bool) -> torch.Tensor:
        """forward() with the step cache on: probe, the host's decision (step_cache.py), then the blocks or the cached residual. The three
        parts are launched eagerly (`eager`) or replayed from one graph entry (probe, body, reuse) under the conditioning's graph key."""
        sc = self.step_cache
        if not pre:
            raise ValueError("step_cache_thresh needs the schedule: pass step_index to forward() after prepare_schedule() "
                             "(tranformer_forward: lx_schedule=(i, timesteps))")
        if step_index == 0:
            sc.reset()
        if not eager:
            self.g_lat.copy_(latents.reshape(self.g_lat.shape))
            latents = self.g_lat
        self.mods.copy_(self.sched[1][step_index])
        self.cond_skip = skip
        try:
            parts = None
            if not eager:
                key = self._graph_key(pre, skip)
                parts = self.graphs.get(key)
                if parts is None:
                    mode = self._warm_mode(skip)
                    if mode not in self._warmed:           # all three parts once, eagerly; what the rule carries over (m, R) is put back
                        keep = None if step_index == 0 else (self.sc_m.clone(), self.sc_R.clone())
                        self._sc_probe(latents)
                        self._sc_body()
                        self._sc_probe(latents)
                        self._sc_reuse()
                        torch.cuda.synchronize(self.device)
                        if keep is not None:
                            self.sc_m.copy_(keep[0])
                            self.sc_R.copy_(keep[1])
                        self._warmed.add(mode)
                    if len(self.graphs) >= 4:
                        self.graphs.clear()
                    parts = []
                    for part in (lambda: self._sc_probe(self.g_lat), self._sc_body, self._sc_reuse):
                        g = torch.cuda.CUDAGraph()
                        with torch.cuda.graph(g):
                            part()
                        parts.append(g)
                    parts = self.graphs[key] = tuple(parts)
            if parts is None:
                self._sc_probe(latents)
            else:
                parts[0].replay()
            rel = self._sc_rel() if step_index > 0 else None
            compute = sc.step(step_index, len(self.sched[0]), rel)
            if parts is None:
                self._sc_body() if compute else self._sc_reuse()
            else:
                parts[1 if compute else 2].replay()
        finally:
            self.cond_skip = False
        if compute:
            self.cond_cached = self.cond_cache          # (a skipped step touches none of the per-layer condition images)
        return self.out.view(self.B, self.N, self.cfg.in_channels)

    def step_cache_report(self) -> Optional[Dict]:
        """What the step cache decided for the forwards of this conditioning since its last step 0: steps (forwards seen), indices, computed
        (indices whose blocks ran), rel (per forward, None at step 0), acc (after each forward), thresh, coefficients. None: the cache is off."""
        return None if self.step_cache is None else self.step_cache.report()

    def _cond_cache_ok(self) -> bool:
        """The condition stream is step-invariant and this kernel set can keep its keys / values per layer: condition queries
        masked from text and image keys (block.py:106-120), something that writes the per-layer images -- the fused projection
        epilogue or the separate q / k / v pass (lx_qkv_prep_kv_segs; lx_qkv_prep_fp8_segs with attn_fp8, into e4m3 images), in precise mode the
        split-bf16 attention's prep pass (LX_PRECISE_ATTN=f32 recomputes: that kernel reads fp32 q / k / v from one buffer); not the e4m3
        GEMM path, whose blocks have no per-layer images --, no add_cond_attn (which also needs the condition stream's attention OUTPUT
        every step)."""
        writes = self.precise_attn_split if self.precise else not self.gemm_fp8
        if not (self.cond_cache_enabled and self.C and writes) or self.model_config.get("add_cond_attn", False):
            return False
        ab = self.attn_bias["cond"]
        return ab["txt"] == NEG_INF and ab["img"] == NEG_INF

    # ------------------------------------------------------------------------------------------ block-level entry points
    # (used by the reference-API mirrors in block.py: same arithmetic as forward(), driven one block at a time)
    def load_streams(self, enc: Optional[torch.Tensor], hid: torch.Tensor, cond: Optional[torch.Tensor], dst: str = "X") -> None:
        """Copy [B,L,D] per-stream tensors into the stream-major rows of X (fp32) or XN (the 16-bit operand image of this mode)."""
        self.block_level_entry()
        buf = self.X if dst == "X" else self._op(self.XN)
        for s, t in (("txt", enc), ("img", hid), ("cond", cond)):
            if t is not None:
                self.rows(buf, s).copy_(t.reshape(-1, t.shape[-1]))

    def read_stream(self, s: str, L: int, src: str = "X", cols: Optional[slice] = None) -> torch.Tensor:
        # (Y: the block-level callers read the attention output / MLP columns, which the fp16 operand mode holds as fp16)
        buf = {"X": self.X, "XN": self._op(self.XN), "Y": self._op(self.Y)}[src]
        r = self.rows(buf, s)
        if cols is not None:
            r = r[:, cols]
        return r.float().reshape(self.B, L, -1).clone()

    def block_level_entry(self) -> None:
        """Block-level calls (the reference-API mirrors in block.py) compute all three streams every time: whatever a previous
        forward() left in the per-layer condition cache must not be read, and no row may be skipped."""
        self.cond_cache = self.cond_cached = self.cond_skip = False

    def block_mods(self, kind: str, idx: int, temb: torch.Tensor, cond_temb: Optional[torch.Tensor]) -> None:
        """Modulation vectors of ONE block from explicit temb / cond_temb (block.py:191-207, 301-305)."""
        cfg, w, D, r = self.cfg, self.w, self.cfg.inner_dim, self.cfg.lora_r
        base, width, lw = (cfg.mod_base_double(idx), 12 * D, 6 * D) if kind == "double" else (cfg.mod_base_single(idx), 3 * D, 3 * D)
        li = idx if kind == "double" else cfg.num_layers + idx
        for vec, out, lora in ((temb, self.mods, self.latent_lora), (cond_temb, self.cmods, True)):
            if vec is None:
                continue
            vec = vec.to(device=self.device, dtype=torch.float32).contiguous()
            ops.linear_skinny(vec, w.t["mod.w"][base:base + width], w.t["mod.b"][base:base + width], out[:, base:], act_in=1)
            if self.precise and "mod.w_lo" in w.t:          # the weights' rounding residual, as _compute_mods adds it
                ops.linear_skinny(vec, w.t["mod.w_lo"][base:base + width], None, out[:, base:], act_in=1, accumulate=True)
            if lora and "mod.lora_down" in w.t and self.lora_scale != 0.0:
                tm = self.tmod[:, :r]
                ops.linear_skinny(vec, w.t["mod.lora_down"][li * r:(li + 1) * r], None, tm, act_in=1)
                if self.precise and "mod.lora_down_lo" in w.t:
                    ops.linear_skinny(vec, w.t["mod.lora_down_lo"][li * r:(li + 1) * r], None, tm, act_in=1, accumulate=True)
                self._scale_lora(tm, [(0, self.B, 1)])
                ops.linear_f32(tm, w.t[f"mod.lora_up.{li}"], None, out[:, base:], M=self.B, N=lw, K=r, ldx=tm.stride(0),
                               ldy=out.stride(0), accumulate=True)

    def configure(self, B, T, N, C, model_config=None, c_factor=None, rope_main=None, rope_cond=None) -> None:
        """Shape + config + RoPE tables without the prompt/condition embedders (block-level use)."""
        self._lora_tables(B)
        self.setup(B, T, N, C)
        self.gemm_ws()
        self.graphs = {}
        self.cond_mask = None                                      # (a conditioning's mask does not outlive it; block-level calls bring their own)
        self.cond_cache = self.cond_cached = False                # block-level use: every call computes all three streams
        self.step_cache = None
        self._select_mode(model_config, c_factor, gemm_fp8=False)
        self.attn_bias = self._attn_bias()
        self._setup_nomax()
        f32 = torch.float32
        if rope_main is not None:
            self.cos_main, self.sin_main = (t.to(self.device, f32).contiguous() for t in rope_main)
        else:
            self.cos_main = self.sin_main = None
        if rope_cond is not None:
            self.cos_cond, self.sin_cond = (t.to(self.device, f32).contiguous() for t in rope_cond)
        else:
            self.cos_cond = self.sin_cond = None
        self._rope_pairs(check=True)
        # A block-level configuration is NOT a conditioning: it replaced model_config, c_factor, the attention bias and the RoPE tables of
        # whatever set_conditioning() left, and block_mods() overwrites slices of mods / cmods. forward() and prepare_schedule() must not
        # run on that, and tranformer_forward -- whose key of conditioning tensors cannot see a block-level call on the same engine in
        # between -- conditions again when it finds cond_ready unset. (The block-level entry points themselves never look at it.)
        self.cond_ready = False

    def attention_module(self, kind: str, idx: int, project_out: bool) -> None:
        """attn_forward (block.py:7-176) on the normalised activations already in XN: QKV projections, QK-RMSNorm,
        RoPE, joint attention; double blocks also apply to_out / to_add_out into X (plain store)."""
        w, D, m = self.w, self.cfg.inner_dim, self.mode16          # (the 16-bit kernels whatever the mode: attn_forward has no other path)
        self.block_level_entry()
        if kind == "double":
            p = f"d{idx}"
            m.gemm("xn", "qkv", p + ".qkv", p + ".qkv_txt", lora_mod_cols=D, lora_toff_max=2)
            m.attention(w.t[p + ".wq"], w.t[p + ".wk"], w.t[p + ".wq_txt"], w.t[p + ".wk_txt"])
            if project_out:
                m.launch(m.operand("attn"), self.X, p + ".out", p + ".out_txt", epilogue=LX_EPI_STORE_F32)      # a plain store, no gate
        else:
            p = f"s{idx}"
            m.fused(p, None, False, None)
            m.attention(w.t[p + ".wq"], w.t[p + ".wk"], w.t[p + ".wq"], w.t[p + ".wk"])
