"""Precise mode's step-invariant condition stream: lx_attn_fwd_split with query-segment subsets and keys / V^T from buffers of their own,
lx_qkv_prep_split_kv_segs writing per-layer images, and the engine that caches the condition stream's key and V^T pairs per layer
(model_config independent_condition / union_cond_attn = False) and runs the last single block's attention for the image queries only."""
import functools
import math
import re

import pytest
import torch

pytestmark = pytest.mark.gpu

from tests.helpers import relerr, tiny_transformer  # noqa: E402

DEV = "cuda"
NINF = float("-inf")
BIAS = {"none": [[0.0] * 3] * 3, "nounion": [[0, 0, NINF], [0, 0, NINF], [NINF, NINF, 0]]}
SENTINEL = 0x5A5B          # a bf16 bit pattern no output of these cases takes in a whole row


@pytest.fixture(scope="module")
def ops():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from loongx_amd import ops as o
    return o


def rnd(*shape, seed=0):
    g = torch.Generator().manual_seed(seed)
    return torch.randn(*shape, generator=g).to(DEV)


def rel(a, b):
    """|a - b| / |b| in float64 (tests/helpers.relerr restated: the kernel checks below call it once per segment and launch)"""
    a, b = a.double(), b.double()
    return float((a - b).norm() / b.norm().clamp_min(1e-30))


def attn_ref(q, k, v, lens, bias):
    """float64 joint attention over segments with a (query segment, key segment) additive bias; q, k, v [B, H, S, 128]"""
    S = sum(lens)
    m = torch.zeros(S, S, dtype=torch.float64, device=q.device)
    e = [0]
    for L in lens:
        e.append(e[-1] + L)
    for i in range(len(lens)):
        for j in range(len(lens)):
            m[e[i]:e[i + 1], e[j]:e[j + 1]] = bias[i][j]
    s = q.double() @ k.double().transpose(-1, -2) / math.sqrt(128.0) + m
    return torch.softmax(s, -1) @ v.double()


def layout(lens, B):
    row0, vt0, r, v = [], [], 0, 0
    for L in lens:
        row0.append(r); vt0.append(v)
        r += B * L
        v += (L + 63) // 64 * 64
    return row0, vt0, v


B_, H_ = 2, 2
D_ = H_ * 128
LDO, O_LO = 2 * D_ + 96, D_ + 64      # hi at [0, D), slack [D, D + 64), lo at [D + 64, 2D + 64), slack behind


@functools.lru_cache(maxsize=None)
def case(lens, mode, bounded):
    """One attention problem: fp32 [k | v | q] rows, their pair images (qkv_prep_split_segs, no norm weights), the float64 reference per
    segment ([B, L, H, 128]), and the all-queries launch every subset launch is compared with. Built once, read-only afterwards."""
    from loongx_amd import ops
    M = B_ * sum(lens)
    buf = rnd(M, 3 * D_, seed=7 + len(mode))
    src = buf
    if bounded:                                                   # q carries scale * log2 e; |q.k| stays far below the bound of 100
        buf[:, 2 * D_:] *= 0.7
        src = buf.clone()
        src[:, 2 * D_:] *= ops.Q_LOG2_FACTOR
    row0, vt0, vt_ld = layout(lens, B_)
    QK2 = torch.zeros(M, 4 * D_, dtype=torch.bfloat16, device=DEV)
    VT2 = torch.zeros(2, B_, H_, 128, vt_ld, dtype=torch.bfloat16, device=DEV)
    segs = [(row0[i], L, vt0[i], None, None, None, None) for i, L in enumerate(lens)]
    ops.qkv_prep_split_segs(src, 2 * D_, 0, D_, segs, B_, H_, QK2, q2_col=2 * D_, k2_col=0, lo_off=D_, VT2=VT2)

    def gather(col):
        parts = [buf[row0[i]:row0[i] + B_ * L, col:col + D_].view(B_, L, H_, 128) for i, L in enumerate(lens)]
        return torch.cat(parts, 1).permute(0, 2, 1, 3)
    ref = attn_ref(gather(2 * D_), gather(0), gather(D_), lens, BIAS[mode]).permute(0, 2, 1, 3)
    refs, e = [], 0
    for L in lens:
        refs.append(ref[:, e:e + L].float())
        e += L
    c = dict(src=src, QK2=QK2, VT2=VT2, row0=row0, vt0=vt0, vt_ld=vt_ld, refs=refs, lens=lens, bias=BIAS[mode],
             flags=(ops.ATTN_Q_LOG2 | ops.ATTN_BOUNDED) if bounded else 0)
    c["full"] = launch(ops, c)
    return c


def launch(ops, c, **kw):
    O = torch.full((B_ * sum(c["lens"]), LDO), SENTINEL, dtype=torch.int16, device=DEV).view(torch.bfloat16)
    ops.attn_fwd_split(c["QK2"], c["VT2"], O, q_col=2 * D_, k_col=kw.pop("k_col", 0), qk_lo_off=D_, o_col=0, o_lo_off=O_LO, B=B_, H=H_,
                       seg_row0=kw.pop("seg_row0", c["row0"]), seg_len=list(c["lens"]), seg_vt0=c["vt0"], bias=kw.pop("bias", c["bias"]),
                       flags=c["flags"], **kw)
    return O


def check_subset(c, O, qmask):
    bits, full = O.view(torch.int16), c["full"].view(torch.int16)
    for i, L in enumerate(c["lens"]):
        rows = slice(c["row0"][i], c["row0"][i] + B_ * L)
        if (qmask >> i) & 1:
            got = (O[rows, :D_].float() + O[rows, O_LO:O_LO + D_].float()).view(B_, L, H_, 128)
            e = rel(got, c["refs"][i])
            print(f"segment {i}: relerr vs float64 = {e:.3e}")
            assert e < 3e-5, (i, e)                                                    # (a)
            assert torch.equal(bits[rows], full[rows]), f"segment {i}: differs from the all-queries launch"      # (b): hi, lo and the slack
            assert bool((bits[rows, D_:O_LO] == SENTINEL).all()) and bool((bits[rows, O_LO + D_:] == SENTINEL).all())
        else:
            assert bool((bits[rows] == SENTINEL).all()), f"segment {i} has no queries: its rows of O were written"      # (c)


CASES = [(40, 100, 70), (300, 520, 260)]
SUBSETS = [dict(n_qseg=2), dict(qseg_mask=0b010), dict(qseg_mask=0b101)]


def _qmask(kw):
    return kw.get("qseg_mask") or (1 << kw["n_qseg"]) - 1


@pytest.mark.parametrize("bounded", [False, True])
@pytest.mark.parametrize("mode", ["none", "nounion"])
@pytest.mark.parametrize("lens", CASES)
def test_attn_split_query_segment_subsets(ops, lens, mode, bounded):
    """Only the query tiles of the query segments are decoded; their rows agree with float64 within the kernel's bound, are bit-identical to
    the all-queries launch (hi and lo image), and the rows of the other segments keep the sentinel O was filled with, slack columns included.
    (300, 520, 260): ragged 256-row query tiles, several tiles per segment, ragged 64-key tiles."""
    c = case(lens, mode, bounded)
    check_subset(c, c["full"], 0b111)
    for kw in SUBSETS:
        check_subset(c, launch(ops, c, **kw), _qmask(kw))
    check_subset(c, launch(ops, c, n_qseg=1, qseg_mask=0b110), 0b110)                  # qseg_mask wins over n_qseg


def _kv_images(ops, c, src, segs_idx, K2, VTb, Q2, k2_col=8):
    segs = [(c["row0"][i], c["lens"][i], c["vt0"][i], None, None, None, None) for i in segs_idx]
    ops.qkv_prep_split_kv_segs(src, 2 * D_, 0, D_, segs, B_, H_, Q2, 2 * D_, K2, k2_col, D_, VTb)


@pytest.mark.parametrize("bounded", [False, True])
def test_attn_split_reads_keys_and_vt_from_buffers_of_their_own(ops, bounded):
    """K and V^T from separate buffers (another ldk, another key column, another vt_ld), written by lx_qkv_prep_split_kv_segs; Q from the
    buffer lx_qkv_prep_split_segs filled: bit-identical to the single-buffer launch, for every query subset."""
    c = case((300, 520, 260), "nounion", bounded)
    M = c["QK2"].shape[0]
    K2 = torch.zeros(M, 2 * D_ + 24, dtype=torch.bfloat16, device=DEV)
    VTb = torch.zeros(2, B_, H_, 128, c["vt_ld"] + 128, dtype=torch.bfloat16, device=DEV)
    Q2 = torch.zeros(M, 4 * D_, dtype=torch.bfloat16, device=DEV)
    _kv_images(ops, c, c["src"], (0, 1, 2), K2, VTb, Q2)
    assert torch.equal(Q2[:, 2 * D_:], c["QK2"][:, 2 * D_:]) and torch.equal(K2[:, 8:8 + 2 * D_], c["QK2"][:, :2 * D_])
    assert torch.equal(launch(ops, c, K=K2, VT=VTb, k_col=8).view(torch.int16), c["full"].view(torch.int16))
    for kw in SUBSETS:
        want = launch(ops, c, **kw)
        assert torch.equal(launch(ops, c, K=K2, VT=VTb, k_col=8, **kw).view(torch.int16), want.view(torch.int16))


def test_attn_split_bad_arguments_are_refused_before_any_launch(ops):
    from loongx_amd._lib import LxError
    c = case((40, 100, 70), "none", False)
    r = c["row0"]
    dead2 = [[0, 0, 0], [0, 0, 0], [NINF, NINF, NINF]]
    bad = [(dict(n_qseg=4), "n_qseg=4 must be 0..n_seg"),
           (dict(qseg_mask=8), "qseg_mask=8 names a segment >= n_seg"),
           (dict(n_qseg=2, seg_row0=[r[0], r[1], r[1] + 10]), "leave segment 2 without queries, but its rows"),
           (dict(bias=dead2), "query segment 2 is masked from every key segment"),
           (dict(n_qseg=2, VT=c["VT2"][..., : c["vt_ld"] - 64].contiguous()), "segment 2's V^T tiles end at")]
    O = torch.full((c["QK2"].shape[0], LDO), SENTINEL, dtype=torch.int16, device=DEV)
    for kw, text in bad:
        kw = dict(kw)
        with pytest.raises(LxError, match=re.escape(text)):
            ops.attn_fwd_split(c["QK2"], c["VT2"], O.view(torch.bfloat16), q_col=2 * D_, k_col=0, qk_lo_off=D_, o_col=0, o_lo_off=O_LO, B=B_, H=H_,
                               seg_row0=kw.pop("seg_row0", r), seg_len=list(c["lens"]), seg_vt0=c["vt0"], bias=kw.pop("bias", c["bias"]), **kw)
    torch.cuda.synchronize()
    assert bool((O == SENTINEL).all())
    # a segment masked from every key is fine as long as it has no queries
    check_subset(dict(c, bias=dead2), launch(ops, c, bias=dead2, n_qseg=2), 0b011)
    # the new prep entry point: a key image too narrow for the pair, V^T tiles past vt_ld
    K2 = torch.zeros(c["QK2"].shape[0], 2 * D_, dtype=torch.bfloat16, device=DEV)
    Q2 = torch.zeros_like(c["QK2"])
    with pytest.raises(LxError, match="must fit ldq2="):
        _kv_images(ops, c, c["src"], (0, 1, 2), K2, c["VT2"].clone(), Q2, k2_col=8)
    with pytest.raises(LxError, match="segment 2's V\\^T tiles end at"):
        _kv_images(ops, c, c["src"], (0, 1, 2), K2, c["VT2"][..., : c["vt_ld"] - 64].contiguous(), Q2, k2_col=0)
    torch.cuda.synchronize()
    assert not bool(K2.any()) and not bool(Q2.any())


def test_prep_into_per_layer_images_leaves_other_segments_alone(ops):
    """A launch over all three segments, then one over segments 0 and 1 with other inputs: segment 2's key rows and its columns of both V^T
    images stay bit for bit, segments 0 and 1 hold what lx_qkv_prep_split_segs writes for the new inputs."""
    lens = (300, 520, 260)
    c = case(lens, "none", False)
    M, r, v = c["QK2"].shape[0], c["row0"], c["vt0"]
    wq, wk = rnd(128, seed=4).abs() + 0.5, rnd(128, seed=5).abs() + 0.5

    def segs(idx):
        return [(r[i], lens[i], v[i], wq, wk, None, None) for i in idx]
    K2 = torch.zeros(M, 2 * D_ + 24, dtype=torch.bfloat16, device=DEV)
    VTb = torch.zeros(2, B_, H_, 128, c["vt_ld"], dtype=torch.bfloat16, device=DEV)
    Q2 = torch.zeros(M, 4 * D_, dtype=torch.bfloat16, device=DEV)
    ops.qkv_prep_split_kv_segs(c["src"], 2 * D_, 0, D_, segs((0, 1, 2)), B_, H_, Q2, 2 * D_, K2, 8, D_, VTb)
    k_before, vt_before, q_before = K2.clone(), VTb.clone(), Q2.clone()
    assert bool(k_before[r[2]:].any()) and bool(vt_before[..., v[2]:].any())
    other = rnd(M, 3 * D_, seed=99)
    ops.qkv_prep_split_kv_segs(other, 2 * D_, 0, D_, segs((0, 1)), B_, H_, Q2, 2 * D_, K2, 8, D_, VTb)
    assert torch.equal(K2[r[2]:], k_before[r[2]:])                                   # segment 2's key rows (hi, lo, slack columns)
    assert torch.equal(VTb[..., v[2]:], vt_before[..., v[2]:])                       # its columns of the hi and the lo V^T image
    assert torch.equal(Q2[r[2]:], q_before[r[2]:])
    QKo = torch.zeros(M, 4 * D_, dtype=torch.bfloat16, device=DEV)
    VTo = torch.zeros_like(VTb)
    ops.qkv_prep_split_segs(other, 2 * D_, 0, D_, segs((0, 1)), B_, H_, QKo, q2_col=2 * D_, k2_col=0, lo_off=D_, VT2=VTo)
    assert torch.equal(K2[:r[2], 8:8 + 2 * D_], QKo[:r[2], :2 * D_]) and torch.equal(Q2[:r[2], 2 * D_:], QKo[:r[2], 2 * D_:])
    assert torch.equal(VTb[..., :v[2]], VTo[..., :v[2]])
    assert not bool(K2[:, :8].any()) and not bool(K2[:, 8 + 2 * D_:].any())          # nothing outside the pair's columns
    assert not torch.equal(K2[:r[2]], k_before[:r[2]])


# ---------------------------------------------------------------------------------------------------- engine
TOL_P = 2e-4      # the project's precise bound at this size (tests/test_precise_gpu.py)


def _engine(tr, precise=True):
    from loongx_amd.flux.engine import DiTEngine
    from loongx_amd.flux.weights import FluxConfig, pack_state_dict
    c = tr.config
    cfg = FluxConfig(num_layers=c.num_layers, num_single_layers=c.num_single_layers, num_attention_heads=c.num_attention_heads,
                     attention_head_dim=c.attention_head_dim, in_channels=c.in_channels, joint_attention_dim=c.joint_attention_dim,
                     pooled_projection_dim=c.pooled_projection_dim, guidance_embeds=c.guidance_embeds, axes_dims_rope=c.axes_dims_rope)
    eng = DiTEngine(pack_state_dict(tr.state_dict(), cfg, "cuda", precise=precise), "cuda")
    eng.precise_default = precise
    return eng


@functools.lru_cache(maxsize=None)
def setup():
    """The inputs of test_step_invariant_condition_stream_is_cached (tests/test_engine_gpu.py): two conditionings, three steps."""
    from oracle import flux_modules as fm
    tr = tiny_transformer(seed=5)
    g = torch.Generator().manual_seed(11)
    B, T, hw = 2, 32, 8
    N = hw * hw
    s = dict(tr=tr, B=B, T=T, N=N, enc=torch.randn(B, T, 64, generator=g) * 0.5, pooled=torch.randn(B, 32, generator=g),
             ids=fm.prepare_latent_image_ids(hw, hw), tids=torch.zeros(T, 3))
    s["cids"] = s["ids"].clone()
    s["cids"][:, 2] -= hw
    s["conds"] = [torch.randn(B, N, 64, generator=g) for _ in range(2)]
    s["lats"] = [torch.randn(B, N, 64, generator=g) for _ in range(3)]
    s["ts"] = [torch.tensor([0.9, 0.8]), torch.tensor([0.55, 0.5]), torch.tensor([0.2, 0.1])]
    s["guid"] = torch.full((B,), 3.5)
    return s


@functools.lru_cache(maxsize=None)
def oracle(mc_items, ci, k):
    from oracle import flux_ref as fr
    s = setup()
    with torch.no_grad():
        return fr.tranformer_forward(s["tr"], s["conds"][ci], s["cids"], None, dict(mc_items), hidden_states=s["lats"][k],
                                     encoder_hidden_states=s["enc"], pooled_projections=s["pooled"], timestep=s["ts"][k], img_ids=s["ids"],
                                     txt_ids=s["tids"], guidance=s["guid"])[0]


def _condition(eng, s, ci, mc):
    d = DEV
    eng.set_conditioning(s["enc"].to(d), s["pooled"].to(d), s["guid"].to(d), s["tids"].to(d), s["ids"].to(d), s["conds"][ci].to(d), s["cids"].to(d),
                         c_t=0.0, model_config=mc)


def _step(eng, s, k):
    return eng.forward(s["lats"][k].to(DEV), s["ts"][k].to(DEV)).float().cpu().clone()


@pytest.mark.parametrize("mc", [{"independent_condition": True}, {"union_cond_attn": False}, {"independent_condition": True, "latent_lora": True}])
def test_precise_condition_stream_is_cached(ops, monkeypatch, mc):
    """The condition stream repeats itself every step: the first forward of a conditioning leaves its key / V^T pairs in per-layer images,
    the following forwards run the text and image rows only. Against the fp32 oracle (which recomputes everything) and against
    LX_COND_CACHE=0; a new conditioning refreshes the cache."""
    s = setup()
    res = {}
    for cache in ("1", "0"):
        monkeypatch.setenv("LX_COND_CACHE", cache)
        eng = _engine(s["tr"])
        outs = []
        for ci in range(2):
            _condition(eng, s, ci, mc)
            for k in range(3):
                assert eng.cond_cached == (cache == "1" and k > 0)
                outs.append(_step(eng, s, k))
                assert eng.cond_cache == (cache == "1")
        assert (eng.KC2 is not None) == (cache == "1") and eng.KC is None
        res[cache] = outs
    for ci in range(2):
        for k in range(3):
            want = oracle(tuple(sorted(mc.items())), ci, k)
            e1, e0 = relerr(res["1"][ci * 3 + k], want), relerr(res["0"][ci * 3 + k], want)
            print(f"conditioning {ci} step {k}: cached {e1:.3e} recomputed {e0:.3e}")
            assert e1 < TOL_P and e0 < TOL_P, (ci, k, e1, e0)
            e10 = relerr(res["1"][ci * 3 + k], res["0"][ci * 3 + k])              # (logged under LX_TEST_RECORD by relerr)
            print(f"    cached vs recomputed {e10:.3e}")
            assert e10 < 2 * TOL_P
    if mc.get("union_cond_attn", True):                        # (without union attention the image never sees the condition at all)
        assert relerr(res["1"][0], res["1"][3]) > 1e-3        # the two conditionings differ: the cache really was refreshed


def test_cached_forward_touches_no_condition_row(ops, monkeypatch):
    """After the first forward of a conditioning the condition rows of every activation buffer and the condition queries are poison: the
    next forward neither reads them (finite output, bit-equal to the unpoisoned run) nor writes the images' condition rows."""
    monkeypatch.setenv("LX_COND_CACHE", "1")
    s = setup()
    mc = {"independent_condition": True, "latent_lora": True}
    outs = []
    for poison in (False, True):
        eng = _engine(s["tr"])
        eng.use_graph = False
        _condition(eng, s, 0, mc)
        _step(eng, s, 0)
        assert eng.cond_cached
        D = eng.cfg.inner_dim
        kc, vtc = eng.rows(eng.KC2.transpose(0, 1), "cond").clone(), eng.VTC2[..., eng.vt0["cond"]:].clone()
        assert bool(kc.any()) and bool(vtc.any())
        if poison:
            for buf in (eng.X, eng.XN2, eng.Y32, eng.YA):
                eng.rows(buf, "cond").fill_(float("nan"))
            eng.rows(eng.QK2, "cond")[:, 2 * D:].fill_(float("nan"))
        out = _step(eng, s, 1)
        assert bool(torch.isfinite(out).all())
        assert torch.equal(eng.rows(eng.KC2.transpose(0, 1), "cond"), kc) and torch.equal(eng.VTC2[..., eng.vt0["cond"]:], vtc)
        if poison:
            for buf in (eng.X, eng.XN2, eng.Y32, eng.YA):                      # nothing wrote them either
                assert bool(torch.isnan(eng.rows(buf, "cond").float()).all())
            assert bool(torch.isnan(eng.rows(eng.QK2, "cond")[:, 2 * D:].float()).all())
        outs.append(out)
    assert torch.equal(outs[0], outs[1])


def test_cached_graph_replay_equals_eager(ops, monkeypatch):
    """A first forward and a cached forward of one conditioning are two graphs; three steps through them give the eager launches' latents."""
    monkeypatch.setenv("LX_COND_CACHE", "1")
    s = setup()
    mc = {"independent_condition": True}
    lat = {}
    for graph in (True, False):
        eng = _engine(s["tr"])
        eng.use_graph = graph
        _condition(eng, s, 0, mc)
        x = s["lats"][0].clone()
        for k in range(3):
            v = eng.forward(x.to(DEV), s["ts"][k].to(DEV)).float().cpu()
            x = x - 0.3 * v
            assert eng.cond_cached
        lat[graph] = x
        if graph:
            assert len(eng.graphs) == 2                       # one with the condition rows, one without
    assert torch.equal(lat[True], lat[False])


@pytest.mark.parametrize("mc,env", [({}, {}), ({"independent_condition": True, "add_cond_attn": True}, {}),
                                    ({"independent_condition": True}, {"LX_PRECISE_ATTN": "f32"})])
def test_cache_stays_off_where_the_condition_stream_is_not_invariant_or_cannot_be_kept(ops, monkeypatch, mc, env):
    monkeypatch.setenv("LX_COND_CACHE", "1")
    for k_, v_ in env.items():
        monkeypatch.setenv(k_, v_)
    s = setup()
    eng = _engine(s["tr"])
    _condition(eng, s, 0, mc)
    for k in range(2):
        got = _step(eng, s, k)
        assert not eng.cond_cache and not eng.cond_cached and eng.KC2 is None and eng.VTC2 is None and eng.KC is None
        assert relerr(got, oracle(tuple(sorted(mc.items())), 0, k)) < TOL_P


@pytest.mark.parametrize("mc", [{}, {"independent_condition": True}])
def test_last_block_attention_for_image_queries_only(ops, monkeypatch, mc):
    """The last single block's attention runs the image queries only (qseg_mask): the forward's output is bit-identical to the one with
    that launch forced to all queries, with and without the condition cache."""
    monkeypatch.setenv("LX_COND_CACHE", "1")
    from loongx_amd.flux.modes import SplitMode
    s = setup()
    assert s["tr"].config.num_single_layers >= 1
    seen = []
    real = ops.attn_fwd_split

    def spy(*a, **kw):
        seen.append((kw.get("qseg_mask", 0), kw.get("n_qseg", 0), len(kw["seg_len"])))
        return real(*a, **kw)
    monkeypatch.setattr(ops, "attn_fwd_split", spy)
    outs = {}
    for forced in (False, True):
        with monkeypatch.context() as m:
            if forced:
                orig = SplitMode.attention
                m.setattr(SplitMode, "attention", lambda self, *a, **kw: orig(self, *a, **dict(kw, img_only=False)))
            eng = _engine(s["tr"])
            eng.use_graph = False
            _condition(eng, s, 0, mc)
            del seen[:]
            outs[forced] = [_step(eng, s, k) for k in range(2)]
            nb = eng.cfg.num_layers + eng.cfg.num_single_layers
            assert len(seen) == 2 * nb
            assert [q for q, _, _ in seen[nb - 1::nb]] == ([0, 0] if forced else [0b010, 0b010])      # the image segment of [txt, img, cond]
            assert all(q == 0 for i, (q, _, _) in enumerate(seen) if i % nb != nb - 1)
            if mc and not forced:                                        # the cached step: keys of three segments, queries of two
                assert seen[nb] == (0, 2, 3)
    for k in range(2):
        assert torch.equal(outs[False][k], outs[True][k])
