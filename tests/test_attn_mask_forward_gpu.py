"""attention_mask through tranformer_forward / generate, and the query-segment subsets of lx_attn_fwd_masked that the last block needs.

Kernel: every written 256-row tile of every (batch, head) against the float64 restatement below (`_ref64`), relative L2 over rows x 128,
bounded by the 6e-3 test_attn_mask_gpu uses for the same kernel; rows of segments without queries keep the sentinel they started with.

Forward: the tiny transformer against oracle.flux_ref.tranformer_forward whose SDPA receives the same mask (TOL_FWD of test_api_gpu), the
truncation equivalence of a key-padding mask (needs no oracle), graph replay against eager launches bit for bit, the reference's rules that
replace the mask, and the refused modes."""
import math

import pytest
import torch

pytestmark = pytest.mark.gpu

from oracle import flux_modules as fm  # noqa: E402
from oracle import flux_ref as fr  # noqa: E402
from loongx_amd.tolerances import TOLERANCES  # noqa: E402
from tests.helpers import load, relerr, tiny_transformer  # noqa: E402
from tests.test_api_gpu import TOL_FWD, _mk_model  # noqa: E402
from tests.test_attn_mask_gpu import PAD_L, PAD_R, QT, SENT, TOL, _lay, _mask, _MaskedF  # noqa: E402
from tests.test_kernels_gpu import DEV, ops  # noqa: E402,F401

BF16 = torch.bfloat16


# ---- 1. kernel: query-segment subsets ------------------------------------------------------------------------------------------------------
def _ref64(lay, b, mask, bias=None):
    """float64 softmax(q k^T / sqrt(128) + mask) v of batch b over the concatenated segments, head by head -> [H, S, 128]; a row that
    attends to no key is zeros"""
    q, k, v = lay.qkv64(b)
    m = mask
    while m.dim() < 4:
        m = m.unsqueeze(0)
    m = m[b if m.shape[0] > 1 else 0].cpu()
    out = torch.zeros(lay.H, lay.S, 128, dtype=torch.float64)
    for h in range(lay.H):
        s = q[h] @ k[h].t() / math.sqrt(128.0)
        if bias is not None:
            for i in range(len(lay.lens)):
                for j in range(len(lay.lens)):
                    s[lay.edges[i]:lay.edges[i + 1], lay.edges[j]:lay.edges[j + 1]] += bias[i][j]
        mh = m[h if m.shape[0] > 1 else 0]
        s = s.masked_fill(~mh, float("-inf")) if mh.dtype == torch.bool else s + mh.double()
        top = s.max(dim=-1, keepdim=True).values
        dead = torch.isinf(top) & (top < 0)
        p = torch.exp(s - torch.where(dead, torch.zeros_like(top), top))
        den = p.sum(dim=-1, keepdim=True)
        out[h] = torch.where(dead, torch.zeros_like(den), 1.0 / den.clamp_min(1e-300)) * (p @ v[h])
    return out


def _run_subset(ops, lay, mask, *, flags=0, **kw):
    D = lay.H * 128
    O = torch.full((lay.buf.shape[0], PAD_L + D + PAD_R), SENT[BF16], dtype=torch.int16, device=DEV).view(BF16)
    ops.attn_fwd_masked(lay.buf, lay.buf, lay.VT, O, mask, q_col=2 * D, k_col=0, o_col=PAD_L, B=lay.B, H=lay.H, seg_row0=lay.row0,
                        seg_len=list(lay.lens), seg_vt0=lay.vt0, flags=flags, **kw)
    torch.cuda.synchronize()
    return O


def _check_subset(lay, O, mask, qseg_mask):
    """largest per-tile relative error over the segments with queries; asserts the write footprint"""
    D = lay.H * 128
    raw = O.view(torch.int16).cpu()
    sent = SENT[BF16]
    assert (raw[:, :PAD_L] == sent).all() and (raw[:, PAD_L + D:] == sent).all(), "write outside the head columns"
    worst, tiles = 0.0, 0
    for b in range(lay.B):
        ref, got = _ref64(lay, b, mask), lay.out_rows(O, b)
        for s, L in enumerate(lay.lens):
            rows = slice(lay.row0[s] + b * L, lay.row0[s] + (b + 1) * L)
            if not (qseg_mask >> s) & 1:
                assert (raw[rows] == sent).all(), f"segment {s} has no queries but rows of O were written (b={b})"
                continue
            assert (raw[rows, PAD_L:PAD_L + D] != sent).any(dim=1).all(), f"segment {s}: a query row was not written (b={b})"
            for t0 in range(0, L, QT):
                r = ref[:, lay.edges[s] + t0: lay.edges[s] + min(L, t0 + QT)]
                g = got[:, lay.edges[s] + t0: lay.edges[s] + min(L, t0 + QT)]
                assert torch.isfinite(g).all()
                for h in range(lay.H):
                    n = float(r[h].norm())
                    tiles += 1
                    if n == 0.0:
                        assert (g[h] == 0).all(), f"fully masked tile b={b} h={h} seg={s} row {t0} not zero"
                    else:
                        worst = max(worst, float((g[h] - r[h]).norm()) / n)
    return worst, tiles


@pytest.mark.parametrize("qseg_mask", [1, 2, 3, 4, 5, 6, 7])
@pytest.mark.parametrize("kind", ["block_bool", "dense_bool_B1SS", "f32_1HSS"])
def test_masked_kernel_query_segment_subsets(ops, kind, qseg_mask):
    """three ragged segments (40, 300, 90: the last key tile of each is ragged, the 300-row one has two query tiles), every non-empty subset of
    them as the query segments"""
    lay = _lay(ops, "three")
    mask = _mask(lay, kind, seed=17 + qseg_mask)
    O = _run_subset(ops, lay, mask, qseg_mask=qseg_mask)
    worst, tiles = _check_subset(lay, O, mask, qseg_mask)
    want_tiles = lay.B * lay.H * sum(-(-L // QT) for s, L in enumerate(lay.lens) if (qseg_mask >> s) & 1)
    print(f"kind={kind} qseg_mask={qseg_mask}: worst tile rel-L2 {worst:.3e} over {tiles} tiles")
    assert tiles == want_tiles
    assert worst <= TOL


def test_masked_kernel_subset_forms_agree_and_share_one_prep(ops):
    """n_qseg = 2 is qseg_mask = 0b011; and a workspace prepared once, with no query subset, serves the full launch and a subset launch
    (what a forward does: 56 full launches and the last block's image-only one), each bit-equal to its one-call form"""
    lay = _lay(ops, "three")
    mask = _mask(lay, "block_bool", seed=23)
    a = _run_subset(ops, lay, mask, n_qseg=2)
    b = _run_subset(ops, lay, mask, qseg_mask=3)
    assert torch.equal(a.view(torch.int16), b.view(torch.int16))
    ws = ops.attn_mask_workspace(mask, B=lay.B, H=lay.H, seg_len=list(lay.lens), seg_vt0=lay.vt0)
    ops.attn_mask_prep(mask, ws, B=lay.B, H=lay.H, seg_len=list(lay.lens), seg_vt0=lay.vt0)
    for q in (0, 2, 5):
        one = _run_subset(ops, lay, mask, qseg_mask=q)
        two = _run_subset(ops, lay, mask, qseg_mask=q, workspace=ws, prepped=True)
        assert torch.equal(one.view(torch.int16), two.view(torch.int16)), q
    from loongx_amd._lib import LxError
    for bad in (dict(qseg_mask=8), dict(n_qseg=4), dict(qseg_mask=-1)):
        with pytest.raises(LxError):
            _run_subset(ops, lay, mask, **bad)


def test_masked_kernel_image_only_at_the_engine_layout(ops):
    """the last block's launch at 512 x 512: segments (512 text, 1024 image, 1024 condition), 24 heads, image queries only, q in log2 units"""
    lay = _lay(ops, "engine", q_log2=True)
    mask = _mask(lay, "keypad", seed=3)
    O = _run_subset(ops, lay, mask, flags=ops.ATTN_Q_LOG2, qseg_mask=2)
    worst, tiles = _check_subset(lay, O, mask, 2)
    print(f"engine layout, image-only: worst tile rel-L2 {worst:.3e} over {tiles} tiles")
    assert tiles == 4 * 24 and worst <= TOL


# ---- the tiny transformer --------------------------------------------------------------------------------------------------------------------
TINY = dict(num_layers=2, num_single_layers=2, num_attention_heads=2, in_channels=64, joint_attention_dim=64, pooled_projection_dim=32,
            guidance_embeds=True)


@pytest.fixture(scope="module")
def tiny():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from loongx_amd.flux.transformer import LxFluxTransformer
    from loongx_amd.flux.weights import FluxConfig
    tr = tiny_transformer()
    return load("flux_tiny.npz"), tr, LxFluxTransformer.from_state_dict(tr.state_dict(), FluxConfig(**TINY), "cuda")


def _inputs(G):
    return dict(hidden_states=G["in_latents"], encoder_hidden_states=G["in_enc"], pooled_projections=G["in_pooled"], timestep=G["in_timestep"],
                img_ids=G["in_img_ids"], txt_ids=G["in_txt_ids"], guidance=G["in_guidance"])


def _cuda(t):
    return None if t is None else t.cuda()


def _forward(lx, kw, cond, cids, mc=None, **extra):
    from loongx_amd.flux.transformer import tranformer_forward
    out = tranformer_forward(lx, _cuda(cond), _cuda(cids), None, dict(mc or {}), return_dict=False, **{k: v.cuda() for k, v in kw.items()}, **extra)
    return out[0].float().cpu().clone()


def _oracle(monkeypatch, tr, kw, cond, cids, mask, mc=None):
    monkeypatch.setattr(fr, "F", _MaskedF(mask))
    with torch.no_grad():
        want = fr.tranformer_forward(tr, cond, cids, None, dict(mc or {}), **kw)[0]
    monkeypatch.undo()
    return want.float()


def _fwd_mask(kind, B, H, T, S):
    """masks in which every query keeps some key (a row without keys is NaN in the oracle's SDPA and would spread through the layers)"""
    g = torch.Generator().manual_seed(31)
    if kind == "bool_B1SS":
        m = torch.rand(B, 1, S, S, generator=g) < 0.6
        m |= torch.eye(S, dtype=torch.bool)
        return m
    if kind == "keypad":
        from loongx_amd.flux.pipeline_tools import text_padding_mask
        return text_padding_mask([T // 2 - b for b in range(B)], T, S - T, 0)
    m = torch.randn(1, H, S, S, generator=g)                      # additive fp32 [1, H, S, S]
    m[torch.rand(1, H, S, S, generator=g) < 0.25] = float("-inf")
    m[0, :, torch.arange(S), torch.arange(S)] = 0.0
    return m


# ---- 2. tranformer_forward with a mask against the oracle under the same mask ---------------------------------------------------------------
@pytest.mark.parametrize("kind", ["bool_B1SS", "keypad", "f32_1HSS"])
@pytest.mark.parametrize("with_cond", [True, False])
@pytest.mark.parametrize("slot", ["keyword", "joint_attention_kwargs"])
def test_tranformer_forward_with_mask_against_the_oracle(tiny, monkeypatch, kind, with_cond, slot):
    G, tr, lx = tiny
    kw = _inputs(G)
    cond, cids = (G["in_cond"], G["in_cond_ids"]) if with_cond else (None, None)
    B, T, N = kw["hidden_states"].shape[0], kw["encoder_hidden_states"].shape[1], kw["hidden_states"].shape[1]
    S = T + N + (cond.shape[1] if with_cond else 0)
    mask = _fwd_mask(kind, B, TINY["num_attention_heads"], T, S)
    want = _oracle(monkeypatch, tr, kw, cond, cids, mask)
    how = dict(attention_mask=mask.cuda()) if slot == "keyword" else dict(joint_attention_kwargs={"attention_mask": mask.cuda()})
    lx.invalidate_conditioning()
    got = _forward(lx, kw, cond, cids, **how)
    again = _forward(lx, kw, cond, cids, **how)                   # the same conditioning: the captured step graph
    plain = _forward(lx, kw, cond, cids)
    e, e2, ep = relerr(got, want), relerr(again, want), relerr(plain, want)
    print(f"{kind} cond={with_cond} {slot}: masked {e:.3e} (replay {e2:.3e}), unmasked against the masked oracle {ep:.3e}; bound {TOL_FWD:.1e}")
    assert lx.engine.cond_mask is None                            # the unmasked call left no mask behind
    assert e < TOL_FWD and e2 < TOL_FWD
    assert ep > TOL_FWD, "the mask made no difference"


# ---- 3. truncation equivalence -----------------------------------------------------------------------------------------------------------------
def _trunc_case(lx, cfg, B, T, hw, k, with_cond, seed, mc=None):
    """image rows of a forward over T text tokens whose last k are masked as keys, and of a forward over the first T - k"""
    from loongx_amd.flux.pipeline_tools import text_padding_mask
    g = torch.Generator().manual_seed(seed)
    N = hw * hw
    kw = dict(hidden_states=torch.randn(B, N, cfg.in_channels, generator=g), encoder_hidden_states=torch.randn(B, T, cfg.joint_attention_dim, generator=g) * 0.5,
              pooled_projections=torch.randn(B, cfg.pooled_projection_dim, generator=g), timestep=torch.linspace(0.7, 0.35, B),
              img_ids=fm.prepare_latent_image_ids(hw, hw), txt_ids=torch.zeros(T, 3), guidance=torch.full((B,), 3.5))
    cond = cids = None
    if with_cond:
        cond = torch.randn(B, N, cfg.in_channels, generator=g)
        cids = fm.prepare_latent_image_ids(hw, hw)
        cids[:, 2] -= hw
    mask = text_padding_mask([T - k] * B, T, N, N if with_cond else 0).cuda()
    lx.invalidate_conditioning()
    padded = _forward(lx, kw, cond, cids, mc, attention_mask=mask)
    short = dict(kw, encoder_hidden_states=kw["encoder_hidden_states"][:, : T - k].contiguous(), txt_ids=torch.zeros(T - k, 3))
    lx.invalidate_conditioning()
    return padded, _forward(lx, short, cond, cids, mc)


@pytest.mark.parametrize("with_cond", [True, False])
def test_truncation_equivalence_tiny(tiny, with_cond):
    """txt_ids = 0: text tokens carry no position, so masking the last 64 of 128 as keys for every query = a forward over the first 64"""
    from loongx_amd.flux.weights import FluxConfig
    _, _, lx = tiny
    bound = 2 * TOLERANCES["bf16"]["per_forward_max"]             # each side within one tolerance of the same exact value
    padded, short = _trunc_case(lx, FluxConfig(**TINY), 2, 128, 8, 64, with_cond, seed=5)
    e = relerr(padded, short)
    print(f"truncation, tiny, cond={with_cond}: {e:.3e} (bound {bound:.1e})")
    assert e <= bound


def test_truncation_equivalence_full_width():
    """one full-width (24 heads, 3072) double + single block: T = 512 with the last 64 keys masked against T = 448, 32 x 32 latents"""
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from loongx_amd.flux.transformer import LxFluxTransformer
    from loongx_amd.flux.weights import FluxConfig
    cfg = FluxConfig(num_layers=1, num_single_layers=1)
    lx = LxFluxTransformer.synthetic(cfg, "cuda", seed=2)
    bound = 2 * TOLERANCES["bf16"]["per_forward_max"]
    padded, short = _trunc_case(lx, cfg, 1, 512, 32, 64, True, seed=6)
    e = relerr(padded, short)
    print(f"truncation, full width: {e:.3e} (bound {bound:.1e})")
    assert torch.isfinite(padded).all() and e <= bound


# ---- 4. graph replay ---------------------------------------------------------------------------------------------------------------------------
def test_generate_with_mask_graph_equals_eager_and_never_replays_a_stale_prep():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from loongx_amd.flux.condition import Condition
    from loongx_amd.flux.generate import generate
    from loongx_amd.flux.pipeline_tools import text_padding_mask
    tr = fm.FluxTransformer2DModel(num_layers=2, num_single_layers=2, heads=2, head_dim=128, in_channels=64, joint_dim=4096,
                                   pooled_dim=768, guidance_embeds=True, lora=True)
    fm.init_synthetic_(tr, seed=4, std=0.03, bias_std=0.02, norm_jitter=0.1)
    _, model = _mk_model(tr.eval())
    eng = model.flux_pipe.transformer.engine
    g = torch.Generator().manual_seed(3)
    B, hw, T = 1, 4, 512
    lat, cond = torch.randn(B, hw * hw, 64, generator=g), torch.randn(B, hw * hw, 64, generator=g)
    pe, pooled = torch.randn(B, T, 4096, generator=g) * 0.1, torch.randn(B, 768, generator=g)
    mask = text_padding_mask([200], T, hw * hw, hw * hw).cuda()

    def run(graph, **kw):
        eng.use_graph = graph                                     # what LX_GRAPH=1 / 0 sets when the engine is made
        c = Condition("subject", latents=cond.cuda(), latent_hw=(hw, hw), position_delta=[0, -hw])
        out = generate(model, model.flux_pipe, conditions=[c], height=hw * 16, width=hw * 16, num_inference_steps=4, latents=lat.cuda(),
                       prompt_embeds=pe.cuda(), pooled_prompt_embeds=pooled.cuda(), output_type="latent", model_config={}, default_lora=True,
                       use_brain_condition=False, **kw)
        return out.images.float().cpu().clone()

    try:
        jk = {"attention_mask": mask}
        first_graph = run(True, joint_attention_kwargs=jk)
        assert eng.graphs, "the masked step was not captured"
        first_eager = run(False, joint_attention_kwargs=jk)
        assert torch.equal(first_graph, first_eager)
        unmasked = run(True)
        assert relerr(first_graph, unmasked) > 1e-3, "the mask made no difference"
        # a second image: the SAME tensor object, same shape, other content
        mask[..., 40:200] = False
        second_graph = run(True, joint_attention_kwargs=jk)
        second_eager = run(False, joint_attention_kwargs=jk)
        assert not torch.equal(second_graph, first_graph) and relerr(second_graph, first_graph) > 1e-4, "a stale prep was replayed"
        assert torch.equal(second_graph, second_eager)
    finally:
        eng.use_graph = True


# ---- 5. the reference's rules ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("rule", ["no_union", "independent", "cfactor"])
def test_reference_rules_replace_the_mask_in_a_forward(tiny, rule):
    G, tr, lx = tiny
    kw = _inputs(G)
    S = 48
    mask = (torch.rand(S, S, generator=torch.Generator().manual_seed(4)) < 0.5).cuda()
    mc = {"no_union": {"union_cond_attn": False}, "independent": {"independent_condition": True}, "cfactor": {}}[rule]
    try:
        if rule == "cfactor":
            lx.c_factor = 0.5
        lx.invalidate_conditioning()
        with_mask = _forward(lx, kw, G["in_cond"], G["in_cond_ids"], mc, attention_mask=mask)
        assert lx.engine.cond_mask is None
        lx.invalidate_conditioning()
        without = _forward(lx, kw, G["in_cond"], G["in_cond_ids"], mc)
        assert torch.equal(with_mask, without)
    finally:
        lx.c_factor = None
        lx.invalidate_conditioning()


# ---- 6. an all-True mask -----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("with_cond", [True, False])
def test_all_true_mask_matches_the_unmasked_forward(tiny, with_cond):
    G, tr, lx = tiny
    kw = _inputs(G)
    cond, cids = (G["in_cond"], G["in_cond_ids"]) if with_cond else (None, None)
    S = 48 if with_cond else 32
    lx.invalidate_conditioning()
    masked = _forward(lx, kw, cond, cids, attention_mask=torch.ones(S, S, dtype=torch.bool, device="cuda"))
    assert lx.engine.cond_mask is not None
    plain = _forward(lx, kw, cond, cids)
    e = relerr(masked, plain)
    print(f"all-True mask against no mask, cond={with_cond}: {e:.3e}")
    assert e <= TOLERANCES["bf16"]["per_forward_max"]


# ---- 7. fp16 operand mode ----------------------------------------------------------------------------------------------------------------------
def test_fp16_operands_with_key_padding_against_the_oracle(monkeypatch):
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from loongx_amd.flux.pipeline_tools import text_padding_mask
    from tests.test_f16_gpu import _tiny_pair
    tr, lx = _tiny_pair()
    g = torch.Generator().manual_seed(1)
    B, T, hw = 2, 32, 8
    N = hw * hw
    kw = dict(hidden_states=torch.randn(B, N, 64, generator=g), encoder_hidden_states=torch.randn(B, T, 64, generator=g) * 0.5,
              pooled_projections=torch.randn(B, 32, generator=g), timestep=torch.tensor([0.7, 0.35]),
              img_ids=fm.prepare_latent_image_ids(hw, hw), txt_ids=torch.zeros(T, 3), guidance=torch.full((B,), 3.5))
    cond = torch.randn(B, N, 64, generator=g)
    cids = fm.prepare_latent_image_ids(hw, hw)
    cids[:, 2] -= hw
    mask = text_padding_mask([20, 9], T, N, N)
    want = _oracle(monkeypatch, tr, kw, cond, cids, mask)
    got = _forward(lx, kw, cond, cids, {"operands": "fp16"}, attention_mask=mask.cuda())
    assert lx.engine.f16 and lx.engine.cond_mask is not None
    again = _forward(lx, kw, cond, cids, {"operands": "fp16"}, attention_mask=mask.cuda())
    plain = _forward(lx, kw, cond, cids, {"operands": "fp16"})
    e, e2, ep = relerr(got, want), relerr(again, want), relerr(plain, want)
    bound = TOLERANCES["fp16"]["per_forward_max"]
    print(f"fp16 operands, key padding: {e:.3e} (replay {e2:.3e}), unmasked against the masked oracle {ep:.3e}; bound {bound:.1e}")
    assert lx.engine.f16_overflow_count() == 0
    assert e < bound and e2 < bound and ep > bound


# ---- 8. refused modes and arguments ------------------------------------------------------------------------------------------------------------
def test_refused_modes_and_arguments_leave_no_mask(tiny):
    G, tr, lx = tiny
    kw = _inputs(G)
    cond, cids = G["in_cond"], G["in_cond_ids"]
    S = 48
    ok = torch.ones(S, S, dtype=torch.bool, device="cuda")
    eng = lx.engine

    def clean():
        assert eng.attn_mask is None and eng.cond_mask is None and not eng.cond_ready and lx._cond_key is None

    _forward(lx, kw, cond, cids, attention_mask=ok)               # a mask is in place: each refusal below has one to forget
    assert eng.cond_mask is not None
    for mc, word in (({"precise": True}, "precise"), ({"attn_fp8": True}, "attn_fp8")):
        with pytest.raises(NotImplementedError, match=word):
            _forward(lx, kw, cond, cids, mc, attention_mask=ok)
        clean()
    _forward(lx, kw, cond, cids, attention_mask=ok)
    with pytest.raises(ValueError, match="twice"):
        _forward(lx, kw, cond, cids, attention_mask=ok, joint_attention_kwargs={"attention_mask": ok})
    clean()
    for bad in (torch.ones(S, S + 1, dtype=torch.bool, device="cuda"), torch.ones(3, 1, S, S, dtype=torch.bool, device="cuda"),
                torch.ones(1, 5, S, S, dtype=torch.bool, device="cuda"), torch.ones(S, S, dtype=torch.bool),
                torch.ones(S, S, dtype=torch.int32, device="cuda"), torch.ones(1, 1, 1, S, S, dtype=torch.bool, device="cuda")):
        with pytest.raises(ValueError):
            _forward(lx, kw, cond, cids, attention_mask=bad)
        clean()
    with pytest.raises(NotImplementedError):
        _forward(lx, kw, cond, cids, attention_mask=torch.ones(S, device="cuda"))
    clean()
    # and the transformer still works, with and without a mask
    assert torch.isfinite(_forward(lx, kw, cond, cids, attention_mask=ok)).all()
    assert torch.isfinite(_forward(lx, kw, cond, cids)).all() and eng.cond_mask is None
