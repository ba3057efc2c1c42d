"""The step-invariant condition stream's per-layer key / V^T images in the modes that had none: model_config attn_fp8 (e4m3 images) and every
shape or setting the fused projection epilogue does not take (ragged stream lengths, bf16 or fp16 operands).
Kernel level: lx_qkv_prep_kv_segs (the 16-bit q / k / v pass with the keys in an image of their own) against lx_qkv_prep_segs, the
same write-only-your-own-segments contract for lx_qkv_prep_fp8_segs, and lx_attn_fwd / lx_attn_fwd_fp8 reading such images with a
query-segment subset. Engine level: the cache is on (and refreshed, skipped rows really skipped, graph replay = eager) in every new
combination and stays off where the condition stream is not step-invariant."""
import functools

import pytest
import torch

pytestmark = pytest.mark.gpu

from tests.helpers import relerr, tiny_transformer  # noqa: E402
from tests.test_engine_gpu import TOL, _engine  # noqa: E402
from tests.test_fp8_gpu import TOL_FP8  # noqa: E402
from tests.test_kernels_gpu import BIASES, DEV, _attn_reference, _qkv_buffer, _segments, ops, rnd  # noqa: E402,F401

# ---------------------------------------------------------------------------------------------------- kernels
LENS, B_, H_ = (40, 300, 90), 2, 3          # ragged 64-slot tiles everywhere, several tiles in segment 1
D_ = H_ * 128
S16 = 0x5A5B                                # a bf16 bit pattern / byte no output of these cases takes in a whole row
S8 = 0x5A


def bits(t):
    return t.view(torch.int16)


def sent16(*shape):
    return torch.full(shape, S16, dtype=torch.int16, device=DEV).view(torch.bfloat16)


def sent8(*shape):
    return torch.full(shape, S8, dtype=torch.uint8, device=DEV)


def _ropes():
    from oracle.flux_modules import rope_tables
    out = []
    for i, Ls in enumerate(LENS):
        ids = torch.zeros(Ls, 3)
        ids[:, 1] = torch.arange(Ls) // 8 + i
        ids[:, 2] = torch.arange(Ls) % 8 - 3
        cos, sin = rope_tables(ids)
        out.append((cos.to(DEV).contiguous(), sin.to(DEV).contiguous()))
    return out


def _segs(idx, normed):
    row0, vt0, _ = _segments(B_, LENS)
    wq, wk = (1 + 0.1 * rnd(128, seed=2), 1 + 0.1 * rnd(128, seed=3)) if normed else (None, None)
    ropes = _ropes() if normed else [(None, None)] * 3
    return [(row0[i], LENS[i], vt0[i], wq, wk, ropes[i][0], ropes[i][1]) for i in idx]


def _input(fmt, seed=5):
    buf = _qkv_buffer(B_, LENS, H_, seed=seed)                  # bf16 [M, 3D] = [k | v | q]
    return buf.to(torch.float16) if fmt == "fp16" else buf


@pytest.mark.parametrize("k2_col,ldk2", [(0, D_), (16, D_ + 40)])
@pytest.mark.parametrize("normed", [True, False])
@pytest.mark.parametrize("fmt", ["bf16", "fp16"])
def test_prep_with_a_key_image_of_its_own_equals_the_in_place_pass(ops, fmt, normed, k2_col, ldk2):
    """lx_qkv_prep_kv_segs against lx_qkv_prep_segs on copies of one buffer (bf16 and fp16 input; with norm weights and RoPE tables -- the
    FAST body for bf16 -- and without): q in place, the key image and the V^T tiles bit for bit; the k columns of QKV unmodified; every
    entry outside the launched segments' rows, key columns and V^T tiles still the sentinel. Then a launch over segments {0, 1} only."""
    row0, vt0, vt_len = _segments(B_, LENS)
    src = _input(fmt)
    M = src.shape[0]
    vt_ld = vt_len + 64                                           # a tile behind the last segment's that nobody may write
    f16 = fmt == "fp16"
    ref, VTr = src.clone(), sent16(B_, H_, 128, vt_ld)
    ops.qkv_prep_segs(ref, 2 * D_, 0, D_, _segs((0, 1, 2), normed), B_, H_, VTr, in_f16=f16)
    got = {}
    for idx in ((0, 1, 2), (0, 1)):
        buf, K2, VT = src.clone(), sent16(M, ldk2), sent16(B_, H_, 128, vt_ld)
        ops.qkv_prep_kv_segs(buf, 2 * D_, 0, D_, _segs(idx, normed), B_, H_, K2, k2_col, VT, in_f16=f16)
        rows = row0[2] if idx == (0, 1) else M                    # the launched segments' rows are the first `rows`
        slots = vt0[2] if idx == (0, 1) else vt_len
        assert torch.equal(bits(buf)[:rows, 2 * D_:], bits(ref)[:rows, 2 * D_:])                 # q in place
        assert torch.equal(bits(buf)[:, :2 * D_], bits(src)[:, :2 * D_])                          # k (and v) columns of QKV as they were
        assert torch.equal(bits(buf)[rows:], bits(src)[rows:])                                    # rows of segments not launched
        assert torch.equal(bits(K2)[:rows, k2_col:k2_col + D_], bits(ref)[:rows, :D_])            # the key image = the in-place k
        assert torch.equal(bits(VT)[..., :slots], bits(VTr)[..., :slots])                         # V^T tiles (zero-filled tails included)
        assert bool((bits(K2)[rows:] == S16).all()) and bool((bits(VT)[..., slots:] == S16).all())
        assert bool((bits(K2)[:, :k2_col] == S16).all()) and bool((bits(K2)[:, k2_col + D_:] == S16).all())
        got[idx] = (K2, VT)
    r, v = row0[2], vt0[2]
    assert torch.equal(bits(got[(0, 1)][0])[:r], bits(got[(0, 1, 2)][0])[:r])                     # segments 0, 1: what the full launch wrote
    assert torch.equal(bits(got[(0, 1)][1])[..., :v], bits(got[(0, 1, 2)][1])[..., :v])
    if normed:
        assert not torch.equal(bits(ref)[:, :D_], bits(src)[:, :D_])                              # (the pass does change k)


def test_fp8_prep_over_a_segment_subset_writes_only_its_own_rows_and_tiles(ops):
    """lx_qkv_prep_fp8_segs over segments {0, 1} into sentinel-filled K8 / VT8 that live in allocations other than Q8's: segment 2's key
    rows and V^T columns (and the tile behind them) keep the sentinel, segments 0 and 1 hold what the launch over all segments writes."""
    row0, vt0, vt_len = _segments(B_, LENS)
    src = _input("bf16")
    M = src.shape[0]
    full = (torch.zeros(M, D_, dtype=torch.uint8, device=DEV), torch.zeros(M, D_, dtype=torch.uint8, device=DEV),
            torch.zeros(B_, H_, 128, vt_len, dtype=torch.uint8, device=DEV))
    ops.qkv_prep_fp8_segs(src, 2 * D_, 0, D_, _segs((0, 1, 2), True), B_, H_, *full)
    Q8, K8, VT8 = sent8(M, D_), sent8(M, D_), sent8(B_, H_, 128, vt_len + 64)
    before = src.clone()
    ops.qkv_prep_fp8_segs(src, 2 * D_, 0, D_, _segs((0, 1), True), B_, H_, Q8, K8, VT8)
    r, v = row0[2], vt0[2]
    assert torch.equal(src, before)
    assert torch.equal(Q8[:r], full[0][:r]) and torch.equal(K8[:r], full[1][:r]) and torch.equal(VT8[..., :v], full[2][..., :v])
    assert bool((Q8[r:] == S8).all()) and bool((K8[r:] == S8).all()) and bool((VT8[..., v:] == S8).all())
    assert not bool((K8[:r] == S8).all(1).any())


@functools.lru_cache(maxsize=None)
def _layer_images(fp8):
    """What the engine's per-layer images hold in a cached step: one prep launch over all segments (input a: the first forward of a
    conditioning), then one over segments {0, 1} with other data (input b: a later step). q of b in place / in Q8. Read-only afterwards."""
    from loongx_amd import ops
    row0, vt0, vt_len = _segments(B_, LENS)
    a, b = _input("bf16", seed=5), _input("bf16", seed=6)
    M = a.shape[0]
    mixed = b.clone()                                             # the rows the attention sees: segments 0, 1 of b, segment 2 of a
    mixed[row0[2]:] = a[row0[2]:]
    if fp8:
        Q8, K8, VT8 = sent8(M, D_), sent8(M, D_), torch.zeros(B_, H_, 128, vt_len, dtype=torch.uint8, device=DEV)
        ops.qkv_prep_fp8_segs(a, 2 * D_, 0, D_, _segs((0, 1, 2), False), B_, H_, Q8, K8, VT8)
        ops.qkv_prep_fp8_segs(b, 2 * D_, 0, D_, _segs((0, 1), False), B_, H_, Q8, K8, VT8)
        return dict(Q=Q8, K=K8, VT=VT8, mixed=mixed)
    K2, VT = sent16(M, D_ + 40), torch.zeros(B_, H_, 128, vt_len + 64, dtype=torch.bfloat16, device=DEV)
    qa, qb = a.clone(), b.clone()
    ops.qkv_prep_kv_segs(qa, 2 * D_, 0, D_, _segs((0, 1, 2), False), B_, H_, K2, 16, VT)
    ops.qkv_prep_kv_segs(qb, 2 * D_, 0, D_, _segs((0, 1), False), B_, H_, K2, 16, VT)
    return dict(Q=qb, K=K2, VT=VT, mixed=mixed)


@pytest.mark.parametrize("mode", ["none", "no_union"])
@pytest.mark.parametrize("fp8", [False, True])
def test_attention_reads_keys_and_vt_from_images_of_their_own(ops, fp8, mode):
    """lx_attn_fwd / lx_attn_fwd_fp8 with K and V^T from the images the prep passes above wrote (another buffer, row stride and key column than
    Q's) and n_qseg = 2: the query segments' rows of O are bit-equal to the launch with every segment a query segment on the same images (a
    row's tile, wave and lane depend only on its position in its own segment), segment 2's rows keep their sentinel, and the result is the
    attention of segments 0 and 1 of the later input over their own keys and segment 2's keys of the first input, within the kernel's bound."""
    c = _layer_images(fp8)
    row0, vt0, _ = _segments(B_, LENS)
    M = c["mixed"].shape[0]
    bias = BIASES[mode]
    kw = dict(o_col=0, B=B_, H=H_, seg_row0=row0, seg_len=list(LENS), seg_vt0=vt0, bias=bias)
    outs = {}
    for nq in (0, 2):
        O = sent16(M, D_)
        if fp8:
            ops.attn_fwd_fp8(c["Q"], c["K"], c["VT"], O, n_qseg=nq, **kw)
        else:
            ops.attn_fwd(c["Q"], c["K"], c["VT"], O, q_col=2 * D_, k_col=16, n_qseg=nq, **kw)
        outs[nq] = O
    r = row0[2]
    assert torch.equal(bits(outs[2])[:r], bits(outs[0])[:r])
    assert bool((bits(outs[2])[r:] == S16).all()) and not bool((bits(outs[0])[r:] == S16).all(1).any())
    ref, edges = _attn_reference(c["mixed"], B_, H_, LENS, bias, 2 * D_, 0, D_)
    got = outs[2].float().cpu()
    for s in range(2):
        e = relerr(got[row0[s]: row0[s] + B_ * LENS[s]].view(B_, LENS[s], H_, 128), ref[:, edges[s]:edges[s + 1]])
        print(f"fp8={fp8} {mode} segment {s}: relerr {e:.3e}")
        assert e < (TOL_FP8 if fp8 else 6e-3), (s, e)           # the bounds of test_fp8_attention_segments / test_attention_segments


# ---------------------------------------------------------------------------------------------------- engine
SHAPES = {"aligned": (32, 8, 8), "ragged": (24, 6, 10)}      # (T, h, w): N = C = 64 (the fused projection epilogue) | 60 (no stream a multiple of 32)
MODES = {"bf16": {}, "fp16": {"operands": "fp16"}, "attn_fp8": {"attn_fp8": True}}
COMBOS = [("aligned", "attn_fp8"), ("ragged", "bf16"), ("ragged", "fp16"), ("ragged", "attn_fp8")]
RULES = [{"independent_condition": True}, {"union_cond_attn": False}]
IMAGES = {"bf16": "KC", "fp16": "KC", "attn_fp8": "KC8"}


@functools.lru_cache(maxsize=None)
def setup(shape):
    """Two conditionings, three steps with different latents and timesteps (test_step_invariant_condition_stream_is_cached's inputs)."""
    from oracle import flux_modules as fm
    T, h, w = SHAPES[shape]
    N = h * w
    g = torch.Generator().manual_seed(11)
    B = 2
    s = dict(tr=tiny_transformer(seed=5), B=B, T=T, N=N, enc=torch.randn(B, T, 64, generator=g) * 0.5, pooled=torch.randn(B, 32, generator=g),
             ids=fm.prepare_latent_image_ids(h, w), tids=torch.zeros(T, 3))
    s["cids"] = s["ids"].clone()
    s["cids"][:, 2] -= w
    s["conds"] = [torch.randn(B, N, 64, generator=g) for _ in range(2)]
    s["lats"] = [torch.randn(B, N, 64, generator=g) for _ in range(3)]
    s["ts"] = [torch.tensor([0.9, 0.8]), torch.tensor([0.55, 0.5]), torch.tensor([0.2, 0.1])]
    s["guid"] = torch.full((B,), 3.5)
    return s


def _key(mc):
    return tuple(sorted(mc.items()))


@functools.lru_cache(maxsize=None)
def oracle(shape, mc_items, ci, k):
    from oracle import flux_ref as fr
    s = setup(shape)
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


@functools.lru_cache(maxsize=None)
def bf16_path(shape, mc_items):
    """The same six forwards on the bf16 path (what test_fp8_gpu.py compares an attn_fp8 engine forward with). Computed once."""
    s = setup(shape)
    eng = _engine(s["tr"])
    outs = []
    for ci in range(2):
        _condition(eng, s, ci, dict(mc_items))
        outs += [_step(eng, s, k) for k in range(3)]
    return outs


def _images(eng):
    return {n for n in ("KC", "KC2", "KC8") if getattr(eng, n) is not None}


@pytest.mark.parametrize("rule", RULES, ids=["independent", "no_union"])
@pytest.mark.parametrize("shape,mode", COMBOS)
def test_condition_stream_is_cached_in_every_mode(monkeypatch, shape, mode, rule):
    """Three steps of two conditionings with LX_COND_CACHE = 1 and 0: the flags as in test_step_invariant_condition_stream_is_cached, this
    mode's image set (and only it) allocated, every output within the mode's bound of the fp32 oracle (attn_fp8: the fp8 bound, also against
    the bf16 path), cached within 5e-3 of recomputed, the second conditioning's outputs different from the first's.
    On the commit before the feature these combinations fail at eng.cond_cache."""
    s = setup(shape)
    mc = dict(rule, **MODES[mode])
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
        assert eng.qkv_fused == (shape == "aligned")
        assert _images(eng) == ({IMAGES[mode]} if cache == "1" else set())
        if cache == "1" and mode == "attn_fp8":
            assert eng.KC8 is not None and eng.KC is None and eng.KC8.dtype == torch.uint8 and eng.VTC8.shape[1:] == eng.VT.shape
        if mode == "fp16":
            assert eng.f16 and eng.f16_overflow_count() == 0
        res[cache] = outs
    fp8 = mode == "attn_fp8"
    tol = TOL_FP8 if fp8 else TOL
    ref16 = bf16_path(shape, _key(rule)) if fp8 else None
    for ci in range(2):
        for k in range(3):
            i = ci * 3 + k
            want = oracle(shape, _key(rule), ci, k)
            e1, e0 = relerr(res["1"][i], want), relerr(res["0"][i], want)
            e10 = relerr(res["1"][i], res["0"][i])
            print(f"{shape} {mode} conditioning {ci} step {k}: cached {e1:.3e} recomputed {e0:.3e} cached vs recomputed {e10:.3e}")
            assert e1 < tol and e0 < tol, (ci, k, e1, e0)
            if fp8:
                eb = relerr(res["1"][i], ref16[i])
                print(f"    against the bf16 path {eb:.3e}")
                assert eb < TOL_FP8, (ci, k, eb)
            assert e10 < 5e-3, (ci, k, e10)                    # the bound of test_step_invariant_condition_stream_is_cached
    if rule.get("union_cond_attn", True):                      # (without union attention the image never sees the condition at all)
        assert relerr(res["1"][0], res["1"][3]) > 1e-3        # the two conditionings differ: the cache really was refreshed


@pytest.mark.parametrize("shape,mode", COMBOS)
def test_cached_step_launches_no_condition_row(ops, monkeypatch, shape, mode):
    """A spy on ops.gemm and on the prep passes, eager launches: in the first forward of a conditioning the block GEMMs cover B (T + N + C)
    rows and the prep pass (where there is one) gets three segments; in the cached step no launch covers more than the B (T + N) text and
    image rows, the projections cover exactly those, and the prep pass gets the text and image segments only."""
    monkeypatch.setenv("LX_COND_CACHE", "1")
    s = setup(shape)
    B, T, N = s["B"], s["T"], s["N"]
    gemms, preps = [], []
    real_gemm = ops.gemm
    monkeypatch.setattr(ops, "gemm", lambda probs, *a, **k: (gemms.append(sum(p.M for p in probs)), real_gemm(probs, *a, **k))[1])
    for name in ("qkv_prep_kv_segs", "qkv_prep_fp8_segs", "qkv_prep_segs"):
        real = getattr(ops, name)
        monkeypatch.setattr(ops, name, lambda QKV, qc, kc, vc, segs, *a, _real=real, _n=name, **k: (preps.append((_n, [g[0] for g in segs])),
                                                                                                  _real(QKV, qc, kc, vc, segs, *a, **k))[1])
    eng = _engine(s["tr"])
    eng.use_graph = False
    _condition(eng, s, 0, dict({"independent_condition": True}, **MODES[mode]))
    nb = eng.cfg.num_layers + eng.cfg.num_single_layers
    want_prep = None if shape == "aligned" else ("qkv_prep_fp8_segs" if mode == "attn_fp8" else "qkv_prep_kv_segs")
    for k, rows in ((0, B * (T + 2 * N)), (1, B * (T + N))):
        del gemms[:], preps[:]
        _step(eng, s, k)
        assert eng.cond_cached
        assert max(gemms) == rows and gemms.count(rows) >= nb, (k, rows, sorted(set(gemms)))
        if want_prep is None:
            assert preps == []
        else:
            r = [eng.r_txt, eng.r_img, eng.r_cond][: 3 if k == 0 else 2]
            assert preps == [(want_prep, r)] * nb, preps


@pytest.mark.parametrize("shape,mode", [("ragged", "bf16"), ("aligned", "attn_fp8")])
def test_cached_graph_replay_equals_eager(monkeypatch, shape, mode):
    """A first forward and a cached forward of one conditioning are two graphs; three steps through them give the eager launches' latents."""
    monkeypatch.setenv("LX_COND_CACHE", "1")
    s = setup(shape)
    mc = dict({"independent_condition": True}, **MODES[mode])
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


@pytest.mark.parametrize("shape,mc", [("aligned", {"attn_fp8": True}), ("ragged", {"independent_condition": True, "add_cond_attn": True})],
                         ids=["union_attn_fp8", "add_cond_attn_ragged"])
def test_cache_stays_off_where_the_condition_stream_is_not_invariant(monkeypatch, shape, mc):
    monkeypatch.setenv("LX_COND_CACHE", "1")
    s = setup(shape)
    eng = _engine(s["tr"])
    _condition(eng, s, 0, mc)
    rule = {k: v for k, v in mc.items() if k != "attn_fp8"}
    for k in range(2):
        got = _step(eng, s, k)
        assert not eng.cond_cache and not eng.cond_cached and _images(eng) == set()
        e = relerr(got, oracle(shape, _key(rule), 0, k))
        print(f"{shape} {mc} step {k}: {e:.3e}")
        assert e < (TOL_FP8 if mc.get("attn_fp8") else TOL), (k, e)
