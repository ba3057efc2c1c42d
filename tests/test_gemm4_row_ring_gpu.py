"""lx_gemm4_kernel's row ring (csrc/gemm4.h): the residual rows of the gated-residual epilogue and the RoPE rows of the q / k tiles reach
the lanes through LDS-DMA slots that are filled one and two 16-row blocks ahead. Every form that takes a different path through the ring,
at the smallest shape that reaches it, against a float64 product of the operands the kernel read (the worst 128 x 256 tile at the bounds of
tests/test_gemm_tiles_gpu.py, whose problem / sentinel-buffer helpers this file uses), with the write footprint held by sentinels around C
and two launches giving the same bits:

  * the two-way split form (every tile split; K = 6144, the planner's minimum for a launch of fewer tiles than CUs): M = 256 (whole
    blocks), 272 (the second tile row is one block), 130 (a partial block 8 of the upper waves, absent blocks behind it);
  * the gate row: per tile (rows_per_batch = 256, or one batch), per row (rows_per_batch = 128: it changes inside a tile), and no gate;
  * whole tiles, M = 512, N = 256, K = 256: eight blocks per wave, the two slots are refilled three times;
  * the three-way split form at the shape of test_kernels_gpu.py::test_gemm_three_way_split_form;
  * q / k tiles (two heads, a RoPE table whose rows all differ: a row fetched for the wrong block is a wrong rotation), M = 64 and
    M = 288 = three batch elements of 96 rows inside one tile, whole tiles and the two-way split form;
  * the fp16-operand and the split-bf16 instantiations, once each on the first split shape."""
import pytest
import torch

from tests.test_gemm_tiles_gpu import BOUND, DEV, PAD, XCOLS, Buf, Prob, _p, randn, run, set_env, tile_worst, workspace

pytestmark = pytest.mark.gpu

K_SPLIT = 6144            # 96 K tiles: from here a launch of fewer tiles than CUs runs entirely in the split form (csrc/gemm.hip)
SPLIT2 = {"LX_GEMM4": "2", "LX_GEMM4_SK": "2"}
WHOLE = {"LX_GEMM4": "2", "LX_GEMM4_SK": "0"}


@pytest.fixture(scope="module")
def ops():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from loongx_amd import ops as o
    return o


class ProbNoGate(Prob):
    """The residual epilogue without a gate: C = X0 + (A W^T + bias)."""

    def __init__(self, fmt, M, N, K, seed):
        super().__init__(fmt, M, N, K, "res", seed, rpb=M)

    def y(self):
        if self._ref is None:
            self._ref = self.X0.double() + self.A64 @ self.W64.T + self.bias.double()
        return self._ref

    def desc(self, ops, C_, r0=0, r1=None):
        kw = dict(f16=True, f16_ovf=self.ovf) if self.fmt == "f16" else {}
        return ops.gemm_desc(self.A, self.W, C_, bias=self.bias, epilogue=ops.LX_EPI_RESID_F32, M=self.M, N=self.N, K=self.K, **kw)


_PROBS = {}


def prob(fmt, M, N, K, rpb):
    """rpb = None: no gate. One problem (operands and float64 reference) per shape, shared by the cases that use it."""
    key = (fmt, M, N, K, rpb)
    if key not in _PROBS:
        seed = 100 + len(_PROBS)
        _PROBS[key] = ProbNoGate(fmt, M, N, K, seed) if rpb is None else Prob(fmt, M, N, K, "res", seed, rpb=rpb)
    return _PROBS[key]


@pytest.mark.parametrize("M", [256, 272, 130])
def test_split_form_gated_residual(ops, monkeypatch, M):
    set_env(ops, monkeypatch, SPLIT2)
    run(ops, [prob("bf16", M, 512, K_SPLIT, M)], workspace(ops), _p("G4_SPLIT2"), f"ring/split2/M{M}")


@pytest.mark.parametrize("rpb", [128, None])
def test_split_form_gate_paths(ops, monkeypatch, rpb):
    """(rows_per_batch = M, the per-tile gate of a split tile, is test_split_form_gated_residual's M = 256)"""
    set_env(ops, monkeypatch, SPLIT2)
    run(ops, [prob("bf16", 256, 512, K_SPLIT, rpb)], workspace(ops), _p("G4_SPLIT2"), f"ring/split2/rpb{rpb}")


@pytest.mark.parametrize("rpb", [256, 128, 512, None])
def test_whole_tile_residual_gate_paths(ops, monkeypatch, rpb):
    """Two tile rows of eight blocks per wave. rows_per_batch = 256: one gate row per tile, another one for the second tile row; 128: the
    gate row changes inside every tile; 512: one batch element; None: no gate."""
    set_env(ops, monkeypatch, WHOLE)
    run(ops, [prob("bf16", 512, 256, 256, rpb)], workspace(ops), _p("G4"), f"ring/whole/rpb{rpb}")


def test_whole_tile_residual_ragged_rows_and_columns(ops, monkeypatch):
    """M = 300: the second tile row has two whole blocks and one of 12 rows in its upper waves, none in its lower waves; N = 200: the
    right-hand waves have 72 columns (clamped column offsets of the ring's pieces, stores with and without active lanes)."""
    set_env(ops, monkeypatch, WHOLE)
    run(ops, [prob("bf16", 300, 200, 256, 300)], workspace(ops), _p("G4"), "ring/whole/ragged")


def test_three_way_split_form(ops, monkeypatch):
    set_env(ops, monkeypatch, {})
    run(ops, [prob("bf16", 1536, 3072, 12288, 1536)], workspace(ops), _p("G4_SPLIT3"), "ring/split3")


@pytest.mark.parametrize("fmt", ["f16", "split2"])
def test_split_form_other_instantiations(ops, monkeypatch, fmt):
    set_env(ops, monkeypatch, SPLIT2)
    run(ops, [prob(fmt, 256, 512, K_SPLIT, 256)], workspace(ops), _p("G4_SPLIT2"), f"ring/split2/{fmt}")


# ------------------------------------------------------------------------------------------------ q / k tiles
VT_PERM = (0, 1, 2, 3, 8, 9, 10, 11, 4, 5, 6, 7, 12, 13, 14, 15)


class QkvProb:
    """[k | v | q] projection with LX_EPI_QKV, H = 2 heads: operands, a RoPE table of L distinct rows and the float64 reference."""
    H = 2

    def __init__(self, M, L, K, seed):
        D = self.H * 128
        self.M, self.L, self.K, self.D, self.N, self.B = M, L, K, D, 3 * D, M // L
        self.A = randn(M, K, seed=seed + 1).to(torch.bfloat16)
        self.W = randn(self.N, K, seed=seed + 2, scale=K ** -0.5).to(torch.bfloat16)
        self.bias = randn(self.N, seed=seed + 3, scale=0.3)
        self.wq, self.wk = 1 + 0.1 * randn(128, seed=seed + 4), 1 + 0.1 * randn(128, seed=seed + 5)
        th = randn(L, 64, seed=seed + 6, scale=2.0)                   # an angle per (position, pair): every row of the table differs
        self.cs = torch.empty(L, 128, device=DEV)
        self.cs[:, 0::2], self.cs[:, 1::2] = th.cos(), th.sin()
        y = self.A.double() @ self.W.double().T + self.bias.double()
        co, si = self.cs[:, 0::2].double().repeat(self.B, 1), self.cs[:, 1::2].double().repeat(self.B, 1)      # [M, 64]

        def norm_rope(x, w):                                          # [M, D] -> RMSNorm over each head, pairs (2j, 2j + 1) rotated
            x = x.view(M, self.H, 128)
            x = x * torch.rsqrt(x.pow(2).mean(-1, keepdim=True) + 1e-6) * w.double()
            e, o = x[..., 0::2], x[..., 1::2]
            out = torch.empty_like(x)
            out[..., 0::2] = e * co[:, None] - o * si[:, None]
            out[..., 1::2] = o * co[:, None] + e * si[:, None]
            return out.view(M, D)
        self.ref_k, self.ref_q, self.ref_v = norm_rope(y[:, :D], self.wk), norm_rope(y[:, 2 * D:], self.wq), y[:, D:2 * D]


_QKV = {}


def qkv_prob(M, L, K):
    if (M, L, K) not in _QKV:
        _QKV[(M, L, K)] = QkvProb(M, L, K, seed=700 + 10 * len(_QKV))
    return _QKV[(M, L, K)]


@pytest.mark.parametrize("M,L,K,env,plan", [(64, 64, 256, WHOLE, "G4"), (288, 96, 256, WHOLE, "G4"), (288, 96, K_SPLIT, SPLIT2, "G4_SPLIT2")])
def test_qk_tiles_rope_rows(ops, monkeypatch, M, L, K, env, plan):
    set_env(ops, monkeypatch, env)
    p = qkv_prob(M, L, K)
    buf = Buf(torch.bfloat16, M + 2 * PAD, p.N + XCOLS)
    buf.block(PAD, M, 0, p.D)                                         # k and q columns; the v columns of C are not written: sentinels
    buf.block(PAD, M, 2 * p.D, p.D)
    C = buf.buf[PAD:PAD + M, :p.N]
    buf.snapshot()
    vt_ld = (L + 63) // 64 * 64
    VT = torch.zeros(p.B, p.H, 128, vt_ld, dtype=torch.bfloat16, device=DEV)
    d = ops.gemm_desc(p.A, p.W, C, bias=p.bias, epilogue=ops.LX_EPI_STORE_BF16, rows_per_batch=L, gelu_col_start=p.N,
                      qkv=dict(norm_q=p.wq, norm_k=p.wk, rope=p.cs, vt=VT, vt_pos0=0, d=p.D))
    ws = workspace(ops)
    outs = []
    for _ in range(2):
        buf.reset()
        VT.zero_()
        ops.gemm([d], ws)
        assert ops.gemm_last_plan() == _p(plan)
        assert ops.lib.lx_gemm_workspace_status(ws.data_ptr(), torch.cuda.current_stream().cuda_stream) == 0
        torch.cuda.synchronize()
        outs.append((buf.buf.clone(), VT.clone()))
    assert torch.equal(outs[0][0].view(torch.int16), outs[1][0].view(torch.int16)) and torch.equal(outs[0][1].view(torch.int16), outs[1][1].view(torch.int16))
    buf.check_footprint(f"ring/qk/M{M}/{plan}")
    bound = BOUND[("bf16", "store")]
    for name, got, ref in (("k", C[:, :p.D], p.ref_k), ("q", C[:, 2 * p.D:], p.ref_q)):
        err, at = tile_worst(got, ref)
        print(f"ring/qk M={M} K={K} {plan} {name}: worst tile {err:.3e} (bound {bound:.0e})")
        assert err < bound, f"{name} of M={M} K={K} {plan}: worst tile at {at}: rel err {err:.3e} >= {bound:.0e}"
    perm = torch.tensor(VT_PERM, device=DEV)
    pos = torch.arange(L, device=DEV)
    slots = (pos // 16) * 16 + perm[pos % 16]
    want = p.ref_v.view(p.B, L, p.H, 128)[:, slots].permute(0, 2, 3, 1)                   # [B, H, d, slot]
    err, _ = tile_worst(VT[..., :L].reshape(-1, L), want.reshape(-1, L))
    assert err < bound, f"V^T image of M={M} K={K} {plan}: rel err {err:.3e} >= {bound:.0e}"
    assert not bool(VT[..., L:].any())
