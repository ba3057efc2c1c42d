"""LoRA adapters of rank > 4 per module: the wide down-projection (lx_lora_down with 16 < R <= 256), the 8-wave GEMMs' LoRA step at
ranks up to 64, and the engine with rank-16 / rank-64 adapter sets.

Bounds. The down-projection multiplies 16-bit operands exactly into fp32 and adds K products in some order, so per element
|got - ref| <= gamma_K sum_k |x||a| + u |ref| (u = 2^-24, gamma_n = n u / (1 - n u): tests/helpers.gamma_n, the bound
tests/test_cs3_tiles_gpu.py derives for fp32 dot products of any summation order), and per row the constant tests/test_rowops_gpu.py
holds this kernel family to (BOUND["lora"], relative to sum |x||a|). The GEMM's LoRA step splits t and up into bf16 hi + lo parts
(2^-16 relative per product, csrc/gemm8.h), so with fp32 outputs |got - ref| <= |gate| (gamma_(K+4r+ns+3) (mag_main + |bias| +
mag_lora) + 2^-16 mag_lora) + 2u (|gate||y| + |x0|) + u |ref|, and every output also meets tests/test_gemm_tiles_gpu.py's worst-tile
bounds."""
import pytest
import torch

pytestmark = pytest.mark.gpu

from tests.helpers import U24, gamma_n, relerr, tiny_transformer  # noqa: E402
from tests.test_engine_gpu import TOL  # noqa: E402
from tests.test_gemm_tiles_gpu import BOUND as GEMM_BOUND, tile_worst  # noqa: E402
from tests.test_lora_rank_cpu import _cfg, _lora_only, with_rank  # noqa: E402
from tests.test_rowops_gpu import BOUND as ROW_BOUND, check_footprint, randn, row_worst, sentinel  # noqa: E402

DEV = "cuda"


@pytest.fixture(scope="module")
def ops():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from loongx_amd import ops as o
    return o


# ================================================================================================ the wide down-projection
_DOWN_IN = {}


def _down_inputs(fmt, M, K):
    """X [M, K] (a strided view, ldx = K + 24) and A [256, K] in the operand format, with their float64 images; shared by all R."""
    key = (fmt, M, K)
    if key not in _DOWN_IN:
        dt = torch.float16 if fmt == "f16" else torch.bfloat16
        X = torch.empty(M, K + 24, dtype=dt, device=DEV)[:, :K]
        X.copy_(randn(M, K, seed=1).to(dt))
        A = randn(256, K, seed=2, scale=K ** -0.5, dtype=dt)
        _DOWN_IN[key] = (X, A, X.double(), A.double())
    return _DOWN_IN[key]


@pytest.mark.parametrize("fmt", ["bf16", "f16"])
@pytest.mark.parametrize("R", [18, 24, 64, 256])
def test_wide_lora_down_against_fp64(ops, fmt, R):
    for M in (1, 70, 513):
        for K in (32, 96, 3072):
            X, A, X64, A64 = _down_inputs(fmt, M, K)
            A_r, A64_r = A[:R].contiguous(), A64[:R]
            for n_split in (1, 4):
                what = f"lora_down {fmt} M={M} K={K} R={R} n_split={n_split}"
                ldt = R + 4                                          # R = 18: ldt % 4 != 0, element stores
                stride = ((M - 1) * ldt + R + 8 + 3) // 4 * 4       # sentinel elements between the slabs and after the last row
                buf = sentinel((n_split * stride + 32,), torch.float32)
                T = buf[16:].as_strided((M, R), (ldt, 1))
                ops.lora_down(X, A_r, T, n_split=n_split, split_stride=stride)
                torch.cuda.synchronize()
                ks = ((K // 32 + n_split - 1) // n_split) * 32
                inside = torch.zeros(buf.shape, dtype=torch.bool, device=DEV)
                tot = 0
                for s in range(n_split):
                    k0, k1 = min(K, s * ks), min(K, (s + 1) * ks)
                    Ts = buf[16 + s * stride:].as_strided((M, R), (ldt, 1))
                    inside[16 + s * stride:].as_strided((M, R), (ldt, 1)).fill_(True)
                    if k0 == k1:
                        assert bool((Ts == 0).all()), f"{what}: slab {s} has an empty K range and must be zeros"
                        continue
                    ref = X64[:, k0:k1] @ A64_r[:, k0:k1].T
                    mag = X64[:, k0:k1].abs() @ A64_r[:, k0:k1].abs().T
                    err = (Ts.double() - ref).abs()
                    lim = gamma_n(k1 - k0) * mag + U24 * ref.abs()
                    over = err > lim
                    assert not bool(over.any()), (f"{what}: slab {s}: {int(over.sum())} elements beyond gamma_K sum|x||a| + u|ref| "
                                                  f"(worst ratio {float((err / lim.clamp_min(1e-300)).max()):.3g})")
                    assert row_worst(Ts, ref, mag) < ROW_BOUND["lora"], f"{what}: slab {s}"
                    tot = tot + Ts.double()
                ref, mag = X64 @ A64_r.T, X64.abs() @ A64_r.abs().T
                err = (tot - ref).abs()
                assert bool((err <= gamma_n(K + n_split) * mag + U24 * ref.abs()).all()), f"{what}: the sum of the slabs"
                check_footprint(what, buf, inside)                 # nothing past R inside a row, past row M, or between the slabs


@pytest.mark.parametrize("fmt", ["bf16", "f16"])
def test_narrow_lora_down_is_unchanged_and_deterministic(ops, fmt):
    """R = 16 stays on the narrow kernel: two calls with the same inputs agree bit for bit, and the wide kernel computes the same
    columns from the same operands (another split of K among the waves: fp32 summation order only)."""
    for M, K, n_split in ((70, 3072, 4), (513, 96, 1)):
        X, A, X64, A64 = _down_inputs(fmt, M, K)
        out = []
        for R in (16, 16, 32):
            T = torch.zeros(n_split, M, R, dtype=torch.float32, device=DEV)
            ops.lora_down(X, A[:R].contiguous(), T[0], n_split=n_split, split_stride=T.stride(0))
            out.append(T)
        assert torch.equal(out[0], out[1])
        mag = X64.abs() @ A64[:16].abs().T
        assert row_worst(out[2].sum(0)[:, :16], out[0].sum(0), mag) < ROW_BOUND["lora"]


def test_lora_down_rank_limits(ops):
    from loongx_amd._lib import LxError
    X, A, _, _ = _down_inputs("bf16", 70, 96)
    A2 = torch.cat([A, A[:8]], 0).contiguous()
    with pytest.raises(LxError):
        ops.lora_down(X, A2, torch.zeros(70, 264, dtype=torch.float32, device=DEV))          # R = 264 > 256
    with pytest.raises(LxError):                                                              # the multi-term form keeps R <= 16
        ops.lora_down_terms([(X.contiguous(), A[:24].contiguous())], torch.zeros(70, 24, dtype=torch.float32, device=DEV), 70 * 24)


# ================================================================================================ the GEMM's LoRA step
GM, GN, GK, MOD_COLS, TOFF_MAX, RPB = 300, 512, 128, 256, 1, 100
_GEMM_IN = {}


def _gemm_inputs(fmt):
    if fmt not in _GEMM_IN:
        dt = torch.float16 if fmt == "f16" else torch.bfloat16
        A, W = randn(GM, GK, seed=11).to(dt), randn(GN, GK, seed=12, scale=0.02).to(dt)
        d = dict(A=A, W=W, bias=randn(GN, seed=13, scale=0.1), gate=randn(GM // RPB, GN, seed=14), X0=randn(GM, GN, seed=15),
                 slabs=randn(4, GM, 2 * 64, seed=16, scale=0.5).contiguous(), up=randn(GN, 64, seed=17, scale=0.1))
        d["main"] = A.double() @ W.double().T
        d["main_mag"] = A.double().abs() @ W.double().abs().T
        _GEMM_IN[fmt] = d
    return _GEMM_IN[fmt]


@pytest.mark.parametrize("g4", ["0", None])
@pytest.mark.parametrize("fmt", ["bf16", "f16"])
def test_gemm_lora_step_ranks(ops, monkeypatch, fmt, g4):
    """One grouped launch (a 16-bit GELU store and a gated fp32 residual, both with the adapter term) per rank and slab count, two
    modules of 256 columns (toff = r for the second)."""
    if g4 is None:
        monkeypatch.delenv("LX_GEMM4", raising=False)
    else:
        monkeypatch.setenv("LX_GEMM4", g4)
    ops.lib.lx_gemm_reload_env()
    d = _gemm_inputs(fmt)
    ws = ops.gemm_workspace(DEV)
    dt16 = torch.float16 if fmt == "f16" else torch.bfloat16
    ovf = torch.zeros(1, dtype=torch.int32, device=DEV)
    fkw = dict(f16=True, f16_ovf=ovf) if fmt == "f16" else {}
    for r in (6, 16, 18, 32, 64):
        up = d["up"][:, :r].contiguous()
        for ns in (1, 4):
            what = f"gemm lora {fmt} LX_GEMM4={g4} r={r} nsplit={ns}"
            slabs = d["slabs"][:ns, :, :2 * r].contiguous()
            t = slabs.double().sum(0)
            tmag = slabs.double().abs().sum(0)
            lora, lmag = torch.zeros_like(d["main"]), torch.zeros_like(d["main"])
            for b in range(GN // MOD_COLS):
                c, o = slice(b * MOD_COLS, (b + 1) * MOD_COLS), min(b, TOFF_MAX) * r
                lora[:, c] = t[:, o:o + r] @ up[c].double().T
                lmag[:, c] = tmag[:, o:o + r] @ up[c].double().abs().T
            y = d["main"] + lora + d["bias"].double()
            C16 = sentinel((GM + 4, GN + 24), dt16)
            C32 = sentinel((GM + 4, GN + 24), torch.float32)
            C32[2:2 + GM, :GN] = d["X0"]
            init32 = C32.clone()
            lkw = dict(lora_t=slabs[0], lora_up=up, lora_nsplit=ns, lora_split_stride=slabs.stride(0), lora_mod_cols=MOD_COLS,
                       lora_toff_max=TOFF_MAX)
            descs = [ops.gemm_desc(d["A"], d["W"], C16[2:2 + GM, :GN], bias=d["bias"], epilogue=ops.LX_EPI_STORE_BF16 | ops.LX_EPI_GELU,
                                   **lkw, **fkw),
                     ops.gemm_desc(d["A"], d["W"], C32[2:2 + GM, :GN], bias=d["bias"], epilogue=ops.LX_EPI_RESID_F32, gate=d["gate"],
                                   rows_per_batch=RPB, **lkw, **fkw)]
            ops.gemm(descs, ws)
            torch.cuda.synchronize()
            inside = torch.zeros(C16.shape, dtype=torch.bool, device=DEV)
            inside[2:2 + GM, :GN] = True
            check_footprint(what + " store", C16, inside)
            check_footprint(what + " resid", C32, inside, init=init32)
            # 16-bit GELU store: the tile tests' worst-tile bound for this format
            e16, at = tile_worst(C16[2:2 + GM, :GN], torch.nn.functional.gelu(y, approximate="tanh"))
            assert e16 < GEMM_BOUND[(fmt, "store")], f"{what}: store tile at {at}: {e16:.3e}"
            # gated fp32 residual: the tile bound, and the derived per-element bound
            g = d["gate"].double().repeat_interleave(RPB, 0)[:GM]
            ref = d["X0"].double() + g * y
            got = C32[2:2 + GM, :GN].double()
            e32, at = tile_worst(got - d["X0"].double(), g * y)
            assert e32 < GEMM_BOUND[(fmt, "f32")], f"{what}: residual tile at {at}: {e32:.3e}"
            # one fp32 chain over everything the accumulator receives (K products, bias, the slab sums and the 4 r hi / lo products)
            lim = g.abs() * (gamma_n(GK + 4 * r + ns + 3) * (d["main_mag"] + d["bias"].double().abs() + lmag) + 2.0 ** -16 * lmag) \
                + 2 * U24 * (g.abs() * y.abs() + d["X0"].double().abs()) + U24 * ref.abs()
            err = (got - ref).abs()
            over = err > lim
            assert not bool(over.any()), (f"{what}: {int(over.sum())} residual elements beyond the derived bound "
                                          f"(worst ratio {float((err / lim).max()):.3g})")
    assert int(ovf) == 0


# ================================================================================================ engine level
_ENG_IN = {}


def _inputs():
    if not _ENG_IN:
        from oracle import flux_modules as fm
        g = torch.Generator().manual_seed(7)
        B, T, hw = 2, 32, 8
        N = hw * hw
        kw = dict(hidden_states=torch.randn(B, N, 64, generator=g), encoder_hidden_states=torch.randn(B, T, 64, generator=g) * 0.5,
                  pooled_projections=torch.randn(B, 32, generator=g), timestep=torch.tensor([0.8, 0.3]),
                  img_ids=fm.prepare_latent_image_ids(hw, hw), txt_ids=torch.zeros(T, 3), guidance=torch.full((B,), 3.5))
        cond = torch.randn(B, N, 64, generator=g)
        cids = fm.prepare_latent_image_ids(hw, hw)
        cids[:, 2] -= hw
        _ENG_IN.update(kw=kw, cond=cond, cids=cids)
    return _ENG_IN["kw"], _ENG_IN["cond"], _ENG_IN["cids"]


_MODELS = {}


def rank_model(r):
    """(oracle module, its state dict) of the tiny model (D = 256) with every adapter -- q/k/v/out, ff, proj_mlp / proj_out, x_embedder and
    the norm*.linear modulation Linears -- redrawn at rank r, N(0, 0.02^2) down and up, scaling 1. Oracle outputs are cached per mode."""
    if r not in _MODELS:
        from oracle import flux_modules as fm
        tr = tiny_transformer(seed=5)
        sd = with_rank({k: v.detach().clone() for k, v in tr.state_dict().items()}, r, seed=r) if r != 4 else tr.state_dict()
        n = 0
        for m in tr.modules():
            if isinstance(m, fm.LoraLinear) and r != 4:
                m.lora_A["default"] = torch.nn.Linear(m.in_features, r, bias=False)
                m.lora_B["default"] = torch.nn.Linear(r, m.out_features, bias=False)
                m.scaling["default"], m.r = 1.0, r
                n += 1
        assert r == 4 or n == 25
        tr.load_state_dict(sd)
        _MODELS[r] = (tr.eval(), {k: v.detach().clone() for k, v in sd.items()}, {})
    return _MODELS[r]


def oracle_out(r, mc):
    from oracle import flux_ref as fr
    tr, _, cache = rank_model(r)
    key = tuple(sorted(mc.items()))
    if key not in cache:
        kw, cond, cids = _inputs()
        with torch.no_grad():
            cache[key] = fr.tranformer_forward(tr, cond, cids, None, dict(mc), **kw)[0]
    return cache[key]


def make_engine(r):
    from loongx_amd.flux.engine import DiTEngine
    from loongx_amd.flux.weights import pack_state_dict
    tr, sd, _ = rank_model(r)
    return DiTEngine(pack_state_dict(sd, _cfg(tr), "cuda"), "cuda")


def condition(eng, mc):
    kw, cond, cids = _inputs()
    d = DEV
    eng.set_conditioning(kw["encoder_hidden_states"].to(d), kw["pooled_projections"].to(d), kw["guidance"].to(d), kw["txt_ids"].to(d),
                         kw["img_ids"].to(d), cond.to(d), cids.to(d), c_t=0.0, model_config=mc)


def forward(eng):
    kw, _, _ = _inputs()
    return eng.forward(kw["hidden_states"].to(DEV), kw["timestep"].to(DEV)).float().cpu().clone()


@pytest.mark.parametrize("operands", ["bf16", "fp16"])
@pytest.mark.parametrize("mc", [{}, {"latent_lora": True}, {"independent_condition": True}, {"attn_fp8": True}])
@pytest.mark.parametrize("r", [16, 64])
def test_engine_forward_wide_ranks_against_the_oracle(ops, r, mc, operands):
    eng = make_engine(r)
    assert eng.cfg.lora_r == r
    condition(eng, dict(mc, operands=operands))
    assert eng.TLs.shape[2] == 4 * r and eng.tmod.shape[1] == 4 * r
    a = forward(eng)
    b = forward(eng)                            # captured / replayed (with independent_condition: the cached condition stream)
    want = oracle_out(r, {k: v for k, v in mc.items() if k != "attn_fp8"})
    if mc.get("attn_fp8"):
        # e4m3 attention operands dominate this mode's error (tests/test_f16_gpu.py holds the rank-4 forward to 7e-2)
        assert relerr(a, want) < 7e-2 and relerr(b, want) < 7e-2
    else:
        assert relerr(a, want) < TOL and relerr(b, want) < TOL, (relerr(a, want), relerr(b, want))
    # the adapters matter: the rank-r set moves the result away from the rank-4 model's
    assert relerr(a, oracle_out(4, {k: v for k, v in mc.items() if k != "attn_fp8"})) > 1e-3


@pytest.mark.parametrize("r", [16, 64])
def test_engine_graph_replay_equals_eager_launches(ops, r):
    eng = make_engine(r)
    condition(eng, {})
    eng.use_graph = False
    eager = forward(eng)
    eng.use_graph = True
    captured, replayed = forward(eng), forward(eng)
    assert torch.equal(eager, captured) and torch.equal(captured, replayed)


def test_load_lora_weights_changes_the_rank_and_back(ops, tmp_path):
    """An r = 16 file over an r = 4 model, then the r = 4 file again: each time the forward equals a freshly packed model's, bit for bit."""
    from safetensors.torch import save_file
    from loongx_amd.flux.pipeline import LxFluxPipeline
    from loongx_amd.flux.transformer import LxFluxTransformer
    tr, sd4, _ = rank_model(4)
    _, sd16, _ = rank_model(16)
    for r, sd in ((4, sd4), (16, sd16)):
        (tmp_path / f"r{r}").mkdir()
        save_file(_lora_only(sd), str(tmp_path / f"r{r}" / "pytorch_lora_weights.safetensors"))
    fresh = {}
    for r in (4, 16):
        e = make_engine(r)
        condition(e, {})
        fresh[r] = forward(e)
    base = {k.replace(".base_layer.", "."): v for k, v in sd4.items() if ".lora_" not in k}
    lxt = LxFluxTransformer.from_state_dict(base, _cfg(tr), "cuda")
    pipe, eng = LxFluxPipeline(lxt), lxt.engine
    for r in (4, 16, 4):
        assert pipe.load_lora_weights(str(tmp_path / f"r{r}")) == 25
        assert eng.cfg.lora_r == r
        condition(eng, {})
        assert eng.TLs.shape[2] == max(16, 4 * r)
        assert torch.equal(forward(eng), fresh[r]), f"after loading the rank-{r} file"


def test_gemm_fp8_refuses_wide_ranks_and_leaves_the_engine_usable(ops):
    eng = make_engine(16)
    condition(eng, {})
    want = forward(eng)
    with pytest.raises(ValueError, match="gemm_fp8.*16|16.*gemm_fp8"):
        condition(eng, {"gemm_fp8": True})
    assert not eng.cond_ready                                     # no conditioning left behind
    condition(eng, {})
    assert torch.equal(forward(eng), want)
