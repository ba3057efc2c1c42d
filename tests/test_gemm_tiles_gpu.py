"""The GEMM's launch plans, tile by tile: every plan the planner of csrc/gemm.hip can choose (asserted through lx_gemm_last_plan after every
launch), on ragged shapes and multi-problem launches whose tile decode (XCD map -> tile_group -> tile_coords, split parts -> K ranges,
the mixed plan's peeled tail and its m_base) has edges, against a float64 product of the operands the kernel read:

  * each problem is cut into 128 x 256 tiles and the worst tile's relative L2 error is held to the format's bound;
  * C lives inside a sentinel-filled buffer (rows above and below, ldc = N + 24): everything outside [M, N] keeps its bits, everything
    inside is finite (a tile the decode never reached stays NaN);
  * the LoRA slabs (an input; rank, slab count, row stride and first column per problem: Prob.set_lora, defaults r = 4 and 2 slabs) lie
    inside NaN sentinels too -- a row or rank read out of range makes the output non-finite -- and keep their bits;
  * the same launch twice gives the same bits; the plans without a workspace give the same bits whichever of them runs, for a problem
    alone, inside its group, or as a row slice (include/lx.h: a data-parallel shard reproduces the batch bit for bit); lx_gemm4_kernel
    and its split forms agree with the 8-wave kernels within one fp32 rounding per element.

Tile counts that select a plan are derived from the device's CU count (the planner rounds by it). Run with -s to see the worst tile of
every arm."""
import json
import os

import pytest
import torch

pytestmark = pytest.mark.gpu

DEV = "cuda"
PAD = 2                   # sentinel rows above and below every output block
XCOLS = 24                # ldc = N + XCOLS (a multiple of 8)
GAP = 3                   # sentinel rows between blocks of a shared buffer

# sentinel bit patterns: NaNs for the stores (a tile nobody wrote stays NaN), a finite value around the gated residual's block
SENT = {torch.bfloat16: 0x7FA5, torch.float16: 0x7E5A, torch.float32: 0x7FC0BEEF, torch.uint8: 0x7F}
RES_SENT = 0x449A5000    # 1234.5f
IVIEW = {torch.bfloat16: torch.int16, torch.float16: torch.int16, torch.float32: torch.int32, torch.uint8: torch.uint8}

# worst-tile bounds = the whole-matrix bounds of test_kernels_gpu.py / test_fp8_gemm_gpu.py / test_precise_gpu.py
BOUND = {("bf16", "store"): 4e-3, ("f16", "store"): 5e-4, ("bf16", "f32"): 2e-5, ("f16", "f32"): 2e-5,
         ("fp8", "f32"): 2e-5, ("fp8", "lora"): 1e-4, ("fp8", "fp8out"): 2e-2,
         ("split", "f32"): 3e-5, ("split", "pair"): 5e-5, ("split", "hi"): 4e-3}
XPLAN_TOL = 2e-6          # lx_gemm4 / split forms against the 8-wave kernels, fp32 outputs (one more fp32 rounding per element)
XPLAN_TOL16 = {"bf16": 2e-3, "f16": 2.5e-4}   # ... 16-bit stores: an ulp flip where the two sums straddle a rounding boundary

REPORT = []               # (arm, plan, worst tile error, bound) per checked output


@pytest.fixture(scope="module")
def ops():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from loongx_amd import ops as o
    yield o
    if REPORT:
        rows = {}
        for arm, plan, err, bound in REPORT:
            k = (arm, plan)
            if k not in rows or err / bound > rows[k][0] / rows[k][1]:
                rows[k] = (err, bound)
        print("\nGEMM_TILES worst tile per arm:")
        for (arm, plan), (err, bound) in sorted(rows.items()):
            print(f"  {arm:34s} plan {plan}  worst {err:.3e}  bound {bound:.0e}")
        out = os.environ.get("LX_GEMM_TILES_REPORT")
        if out:
            with open(out, "a") as f:
                for (arm, plan), (err, bound) in sorted(rows.items()):
                    f.write(json.dumps({"arm": arm, "plan": plan, "worst": err, "bound": bound}) + "\n")


def ncu():
    return torch.cuda.get_device_properties(0).multi_processor_count


_WS = []


def workspace(ops):
    if not _WS:
        _WS.append(ops.gemm_workspace(DEV))
    return _WS[0]


def set_env(ops, monkeypatch, env):
    for k in ("LX_GEMM_BM", "LX_GEMM4", "LX_GEMM4_SK", "LX_GEMM4_FAULT"):
        monkeypatch.delenv(k, raising=False)
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    ops.lib.lx_gemm_reload_env()


def randn(*shape, seed, scale=1.0):
    g = torch.Generator(device=DEV).manual_seed(seed)
    return torch.randn(*shape, generator=g, device=DEV) * scale


def deq(u8):
    return u8.view(torch.float8_e4m3fn).float()


def q8(x, scale):
    return (x.float() * scale).clamp(-448, 448).to(torch.float8_e4m3fn).view(torch.uint8)


# ------------------------------------------------------------------------------------------------ outputs inside sentinel buffers
class Buf:
    """One sentinel-filled buffer holding one or more output blocks (rows apart by GAP, PAD above the first and below the last)."""

    def __init__(self, dtype, rows, ldc, resid=False):
        self.dtype, self.resid = dtype, resid
        self.buf = torch.empty(rows, ldc, dtype=dtype, device=DEV)
        self.sent = RES_SENT if resid else SENT[dtype]
        self.iv = IVIEW[dtype]
        self.buf.view(self.iv).fill_(self.sent if self.sent < 2 ** 31 else self.sent - 2 ** 32)
        self.blocks = []          # (r0, M, c0, N)
        self.init = None

    def block(self, r0, M, c0, N):
        self.blocks.append((r0, M, c0, N))
        return self.buf[r0:r0 + M, c0:c0 + N]

    def snapshot(self):           # the state every launch starts from (the residual's X0 inside, sentinels outside)
        self.init = self.buf.clone()

    def reset(self):
        self.buf.copy_(self.init)

    def check_footprint(self, what):
        bits = self.buf.view(self.iv)
        s = self.sent if self.sent < 2 ** 31 or self.iv != torch.int32 else self.sent - 2 ** 32
        outside = bits != s
        for r0, M, c0, N in self.blocks:
            blk = self.buf[r0:r0 + M, c0:c0 + N]
            if self.dtype == torch.uint8:
                bad = (blk & 0x7F) == 0x7F
            else:
                bad = ~torch.isfinite(blk.float())
            assert not bool(bad.any()), f"{what}: {int(bad.sum())} non-finite elements inside block rows {r0}.. cols {c0}.. (first at " \
                                        f"{bad.nonzero()[0].tolist()})"
            outside[r0:r0 + M, c0:c0 + N] = False
        assert not bool(outside.any()), f"{what}: {int(outside.sum())} elements outside the [M, N] blocks changed (first at {outside.nonzero()[0].tolist()})"


def tile_worst(got, ref):
    """max over 128 x 256 tiles of ||got - ref|| / ||ref||, and the worst tile's (row, col) origin."""
    got, ref = got.double(), ref.double()
    M, N = ref.shape
    tm, tn = -(-M // 128), -(-N // 256)
    d = torch.zeros(tm * 128, tn * 256, dtype=torch.float64, device=ref.device)
    r = torch.zeros_like(d)
    d[:M, :N] = (got - ref) ** 2
    r[:M, :N] = ref ** 2
    d = d.view(tm, 128, tn, 256).sum((1, 3))
    r = r.view(tm, 128, tn, 256).sum((1, 3))
    e = (d / r.clamp_min(1e-300)).sqrt()
    i = int(e.argmax())
    return float(e.view(-1)[i]), (i // tn * 128, i % tn * 256)


# ------------------------------------------------------------------------------------------------ problems
def lora_term64(slabs, up, R, mod_cols, toff_max):
    """float64 adapter term of a GEMM: out[m, n] = sum_r t[m, toff(n) + r] up[n, r] with t the sum of the slabs [nsplit, M, >= (toff_max
    + 1) R] and toff(n) = R min(n // mod_cols, toff_max) -- the module a column belongs to picks its R columns of t."""
    t = slabs.double().sum(0)
    N = up.shape[0]
    out = torch.zeros(t.shape[0], N, dtype=torch.float64, device=t.device)
    for b in range(-(-N // mod_cols)):
        m = min(b, toff_max) * R
        c = slice(b * mod_cols, min(N, (b + 1) * mod_cols))
        out[:, c] = t[:, m:m + R] @ up[c].double().T
    return out


class Prob:
    """One GEMM problem: operands in the launch's format, its output block, and its float64 reference.
    fmt: bf16 | f16 | fp8 | split2 | split3.  epi: store (16-bit store + GELU) | f32 | lora (fp32 store + LoRA) | res (gated residual) |
    fp8out (e4m3 store + GELU) | pair (LX_EPI_SPLIT_BF16 + GELU)."""
    R, NSPLIT, MOD_COLS, TOFF_MAX, GELU_COL = 4, 2, 256, 1, 200

    def __init__(self, fmt, M, N, K, epi, seed, rpb=None, lora=False, R=None, nsplit=None, ldt=None, t_col0=0):
        self.fmt, self.M, self.N, self.K, self.epi, self.rpb, self.seed = fmt, M, N, K, epi, rpb, seed
        self.lora = lora or epi == "lora"
        g = seed * 10
        A = randn(M, K, seed=g + 1)
        W = randn(N, K, seed=g + 2, scale=0.02)
        self.bias = randn(N, seed=g + 3, scale=0.1)
        if fmt == "fp8":
            self.A = q8(A, 16.0)
            self.W, rs = Prob._wq(W)
            self.cs = (rs / 16.0).contiguous()
            self.A64, self.W64 = deq(self.A).double(), deq(self.W).double()
        elif fmt.startswith("split"):
            segs = int(fmt[-1])
            self.segs, self.a_lo = segs, K + 64
            hi = A.to(torch.bfloat16)
            self.A = torch.zeros(M, 2 * K + 128, dtype=torch.bfloat16, device=DEV)
            self.A[:, :K] = hi
            self.A[:, K + 64:2 * K + 64] = (A - hi.float()).to(torch.bfloat16)
            self.A64 = self.A[:, :K].double() + self.A[:, K + 64:2 * K + 64].double()
            Wh = W.to(torch.bfloat16)
            if segs == 2:
                self.W, self.W64 = Wh, Wh.double()
            else:
                Wl = (W - Wh.float()).to(torch.bfloat16)
                self.W = torch.cat([Wh, Wl], 1).contiguous()
                self.W64 = Wh.double() + Wl.double()
        else:
            dt = torch.float16 if fmt == "f16" else torch.bfloat16
            self.A, self.W = A.to(dt), W.to(dt)
            self.A64, self.W64 = self.A.double(), self.W.double()
        if epi == "res":
            nb = -(-M // rpb)
            self.gate = randn(nb, N, seed=g + 4)
            self.X0 = randn(M, N, seed=g + 5)
        self._main = self._ref = None
        if self.lora:
            self.set_lora(R, nsplit, ldt, t_col0)

    def set_lora(self, R=None, nsplit=None, ldt=None, t_col0=0):
        """(Re)draw the adapter inputs -- rank R, nsplit slabs, row stride ldt (default 2 R), lora_t at column t_col0 of the slab rows --
        and drop the cached reference (the operands' float64 product is kept). Each slab lies inside sentinels: PAD NaN rows above and
        below it and NaN in the columns the step never reads (ldt > t_col0 + (TOFF_MAX + 1) R), so a row or rank read out of range
        shows as a non-finite output, and the whole buffer must keep its bits."""
        assert self.lora
        self.R, self.NSPLIT, self.t_col0 = R or Prob.R, nsplit or Prob.NSPLIT, t_col0
        w = (self.TOFF_MAX + 1) * self.R
        self.ldt = 2 * self.R if ldt is None else ldt
        assert self.ldt >= t_col0 + w, (self.ldt, t_col0, w)
        g = self.seed * 10
        self.tbuf = torch.empty(self.NSPLIT, self.M + 2 * PAD, self.ldt, dtype=torch.float32, device=DEV)
        self.tbuf.view(torch.int32).fill_(SENT[torch.float32])
        self.slabs = self.tbuf[:, PAD:PAD + self.M, t_col0:t_col0 + w]
        self.slabs.copy_(randn(self.NSPLIT, self.M, w, seed=g + 6, scale=0.5))
        self.up = randn(self.N, self.R, seed=g + 7, scale=0.1).contiguous()
        self.tinit = self.tbuf.clone()
        self._ref = None

    def check_inputs(self, what):
        if self.lora:
            assert torch.equal(self.tbuf.view(torch.int32), self.tinit.view(torch.int32)), f"{what}: the launch changed its input lora_t"

    @staticmethod
    def _wq(W):
        from loongx_amd import ops
        return ops.quantize_weight_fp8(W)

    # -- reference (float64, from the operands the kernel reads), rows [r0, r1) --
    def y(self):
        if self._ref is None:
            if self._main is None:
                y = self.A64 @ self.W64.T
                if self.fmt == "fp8":
                    y = y * self.cs.double()
                self._main = y + self.bias.double()
            y = self._main.clone()
            if self.lora:
                y += lora_term64(self.slabs, self.up, self.R, self.MOD_COLS, self.TOFF_MAX)
            if self.epi in ("store", "fp8out", "pair"):
                c = self.GELU_COL
                y[:, c:] = torch.nn.functional.gelu(y[:, c:], approximate="tanh")
            if self.epi == "res":
                y = self.X0.double() + self.gate.double().repeat_interleave(self.rpb, 0)[:self.M] * y
            self._ref = y
        return self._ref

    # -- output buffer and descriptor --
    def out_dtype(self):
        if self.epi == "store":
            return torch.float16 if self.fmt == "f16" else torch.bfloat16
        return {"fp8out": torch.uint8, "pair": torch.bfloat16}.get(self.epi, torch.float32)

    def ldc(self):
        return (2 * self.N + 8 + XCOLS) if self.epi == "pair" else self.N + XCOLS

    def own_buf(self, r0=0, r1=None):
        """A private sentinel buffer for rows [r0, r1) of this problem."""
        r1 = self.M if r1 is None else r1
        b = Buf(self.out_dtype(), (r1 - r0) + 2 * PAD, self.ldc(), resid=self.epi == "res")
        self.place(b, PAD, r0, r1)
        b.snapshot()
        return b

    def place(self, b, row, r0=0, r1=None):
        r1 = self.M if r1 is None else r1
        blk = b.block(row, r1 - r0, 0, self.N)
        if self.epi == "pair":
            b.block(row, r1 - r0, self.N + 8, self.N)
        if self.epi == "res":
            blk.copy_(self.X0[r0:r1])
        return blk

    def desc(self, ops, C_, r0=0, r1=None):
        r1 = self.M if r1 is None else r1
        kw = dict(bias=self.bias, M=r1 - r0, N=self.N, K=self.K)
        epi = {"store": ops.LX_EPI_STORE_BF16 | ops.LX_EPI_GELU, "f32": ops.LX_EPI_STORE_F32, "lora": ops.LX_EPI_STORE_F32,
               "res": ops.LX_EPI_RESID_F32, "fp8out": ops.LX_EPI_STORE_FP8 | ops.LX_EPI_GELU,
               "pair": ops.LX_EPI_STORE_BF16 | ops.LX_EPI_GELU}[self.epi]
        if self.epi in ("store", "fp8out", "pair"):
            kw["gelu_col_start"] = self.GELU_COL
        if self.epi == "res":
            assert r0 % self.rpb == 0
            kw.update(gate=self.gate[r0 // self.rpb:], rows_per_batch=self.rpb)
        if self.lora:
            kw.update(lora_t=self.tbuf[0, PAD + r0:, self.t_col0:], lora_up=self.up, lora_nsplit=self.NSPLIT, lora_split_stride=self.tbuf.stride(0),
                      lora_mod_cols=self.MOD_COLS, lora_toff_max=self.TOFF_MAX)
        if self.fmt == "fp8":
            kw.update(fp8=True, col_scale=self.cs)
            if self.epi == "fp8out":
                kw["out_scale"] = 16.0
        elif self.fmt == "f16":
            kw.update(f16=True, f16_ovf=self.ovf)
        elif self.fmt.startswith("split"):
            kw.update(k_segs=self.segs, a_lo_off=self.a_lo)
            if self.epi == "pair":
                kw["c_lo_off"] = self.N + 8
        return ops.gemm_desc(self.A[r0:r1], self.W, C_, epilogue=epi, **kw)

    ovf = None

    # -- tile-by-tile check of this problem's rows [r0, r1) in buffer b at buffer row `row` --
    def check(self, b, row, arm, plan, r0=0, r1=None):
        r1 = self.M if r1 is None else r1
        ref = self.y()[r0:r1]
        got = b.buf[row:row + (r1 - r0), :self.N]
        fmt = "split" if self.fmt.startswith("split") else self.fmt
        where = f"{arm} {self.fmt} {self.epi} M={self.M} N={self.N} K={self.K} rows [{r0}, {r1})"
        checks = []
        if self.epi == "fp8out":
            want = deq(q8(ref * 16.0, 1.0))
            checks.append(("fp8out", deq(got), want))
            miss = float((deq(got) != want).float().mean())
            assert miss < 0.02, f"{where}: {miss:.4f} of the e4m3 bytes differ from the rounded reference"
        elif self.epi == "pair":
            hi, lo = got.double(), b.buf[row:row + (r1 - r0), self.N + 8:2 * self.N + 8].double()
            checks += [("pair", hi + lo, ref), ("hi", hi, ref)]
        elif self.epi == "store":
            checks.append(("store", got, ref))
        else:
            checks.append(("lora" if self.lora and fmt == "fp8" else "f32", got, ref))
        for kind, g, w in checks:
            bound = BOUND[(fmt, kind)]
            err, at = tile_worst(g, w)
            REPORT.append((f"{fmt}/{arm}/{kind}", plan, err, bound))
            assert err < bound, f"{where}: worst {kind} tile at {at}: rel err {err:.3e} >= {bound:.0e}"


# ------------------------------------------------------------------------------------------------ the four-problem launch
def group(fmt, K, rows0, seed=0, lora_p3=False, **lora):
    """Four problems of one K, different M and N, mixed epilogues:
      p0  M = 256 (rows0 - 1) + 1 (or 20 for rows0 = 1), N = 2040: a 16-bit / e4m3 / hi-lo store with GELU from column 200 (inside a tile)
      p1  M = 2303 (9 tile rows, M % 256 = 255), N = 776 (3 x 256 + 8): fp32 store + LoRA (2 slabs, modules of 256 columns, toff_max 1)
      p2  M = 1055 (5 tile rows, M % 256 = 31), N = 264: fp32 store
      p3  M = 641 (M % 256 = 129), N = 64 (proj_out): gated fp32 residual, 100 rows per batch
    49 + 8 rows0 tiles of 256 x 256; the last ones in launch order are p3, p2 and p1's ragged last tile row.
    lora = R, nsplit, ldt, t_col0 of p1's adapter inputs (Prob.set_lora); lora_p3 gives p3 the adapter term with the same parameters."""
    store = {"fp8": "fp8out", "split2": "pair", "split3": "pair"}.get(fmt, "store")
    M0 = 20 if rows0 == 1 else 256 * (rows0 - 1) + 1
    return [Prob(fmt, M0, 2040, K, store, seed + 1), Prob(fmt, 2303, 776, K, "lora", seed + 2, **lora), Prob(fmt, 1055, 264, K, "f32", seed + 3),
            Prob(fmt, 641, 64, K, "res", seed + 4, rpb=100, lora=lora_p3, **(lora if lora_p3 else {}))]


def tiles256(probs):
    return sum(-(-p.M // 256) * -(-p.N // 256) for p in probs)


SLICES = [(100, None), (1000, None), (520, 1000), (300, None)]      # per problem of group(): r0 % 32 != 0 (p3: whole batches)


def descs_of(ops, probs, bufs):
    return [p.desc(ops, b.buf[b.blocks[0][0]:b.blocks[0][0] + p.M, :b.buf.shape[1]] if p.epi == "pair" else
                   b.buf[b.blocks[0][0]:b.blocks[0][0] + p.M, :p.N]) for p, b in zip(probs, bufs)]


def run(ops, probs, ws, plan, arm, bufs=None, check=True):
    """Launch the problems (each in its own sentinel buffer unless given) twice; check plan, footprint, tiles and run-to-run bits.
    plan: the plan the planner must choose, or a tuple of them where the choice between the two 8-wave tile heights is the planner's.
    Returns the buffers (contents of the first run)."""
    if bufs is None:
        bufs = [p.own_buf() for p in probs]
    for p in probs:
        if p.fmt == "f16":
            p.ovf = torch.zeros(1, dtype=torch.int32, device=DEV)
    descs = descs_of(ops, probs, bufs)
    first = None
    for rep in range(2):
        for b in {id(b): b for b in bufs}.values():
            b.reset()
        ops.gemm(descs, ws)
        got = ops.gemm_last_plan()
        assert got in (plan if isinstance(plan, tuple) else (plan,)), \
            f"{arm}: the planner chose plan {got}, not {plan} ({tiles256(probs)} tiles of 256 x 256, {ncu()} CUs)"
        if ws is not None:
            assert ops.lib.lx_gemm_workspace_status(ws.data_ptr(), torch.cuda.current_stream().cuda_stream) == 0
        torch.cuda.synchronize()
        if rep == 0:
            first = [b.buf.clone() for b in bufs]
    for b, f in zip(bufs, first):
        assert torch.equal(b.buf.view(b.iv), f.view(b.iv)), f"{arm}: two runs of the same launch differ"
    for p in probs:
        p.check_inputs(arm)
    if check:
        for b in {id(b): b for b in bufs}.values():
            b.check_footprint(arm)
        for p, b in zip(probs, bufs):
            p.check(b, b.blocks[0][0], arm, got)
            if p.ovf is not None:
                assert int(p.ovf) == 0
    return bufs


def block_of(p, b):
    r = b.blocks[0][0]
    return b.buf[r:r + p.M, :p.ldc()]


def close(p, a, b):
    """relative difference of two results of problem p (a gated residual's without X0: the product is what the plans compute)"""
    a, b = a[:, :p.N].double(), b[:, :p.N].double()
    if p.epi == "res":
        a, b = a - p.X0.double(), b - p.X0.double()
    return float((a - b).norm() / b.norm())


# ------------------------------------------------------------------------------------------------ bf16 / fp16 operands: every plan
def _p(name):
    from loongx_amd import _lib
    return getattr(_lib, "LX_GEMM_PLAN_" + name)


# arm -> (environment, workspace?, expected plan, launch size)
ARMS16 = {
    "w256": ({"LX_GEMM_BM": "256"}, False, "8WAVE_256", "main"),
    "w128": ({"LX_GEMM_BM": "128"}, False, "8WAVE_128", "main"),
    "mixed": ({}, False, "MIXED", "main"),
    "g4": ({"LX_GEMM4": "2", "LX_GEMM4_SK": "0"}, True, "G4", "main"),
    "sk2": ({"LX_GEMM4_SK": "2"}, True, "G4_SPLIT2", "main"),
    "sk3": ({}, True, "G4_SPLIT3", "main"),
    "splitall2": ({"LX_GEMM4_SK": "2"}, True, "G4_SPLIT2", "long"),
    "splitall3": ({}, True, "G4_SPLIT3", "long"),
}
K_MAIN, K_LONG = 1536, 6144        # 24 K tiles: the smallest K of the three-way split tail; 96: the split-all form


def main_rows0():
    """p0's tile rows for the 'main' launch: NCU + tail tiles, tail in [17, 24] -- one full round and a partial one whose tiles span
    p3, p2 and p1's ragged last row: the mixed plan peels p3 and p2 whole and p1 partly, and the tail is small enough (<= a sixth of
    a round) for the three-way split form."""
    n = ncu()
    for tail in range(17, 25):
        if (n + tail - 49) % 8 == 0 and tail * 6 <= n:
            return (n + tail - 49) // 8
    pytest.skip(f"no main launch shape for {n} CUs")


_GROUPS = {}


def cached_group(fmt, K, rows0):
    key = (fmt, K, rows0)
    if key not in _GROUPS:
        _GROUPS[key] = group(fmt, K, rows0)
    return _GROUPS[key]


@pytest.mark.parametrize("arm", list(ARMS16))
@pytest.mark.parametrize("fmt", ["bf16", "f16"])
def test_gemm_tiles_16bit_operands(ops, monkeypatch, fmt, arm):
    env, use_ws, plan, size = ARMS16[arm]
    if size == "long":
        probs = cached_group(fmt, K_LONG, 1)
        t = tiles256(probs)
        assert t <= 128 and (arm == "splitall2" or 3 * t <= min(256, ncu())), t
    else:
        probs = cached_group(fmt, K_MAIN, main_rows0())
    ws = workspace(ops) if use_ws else None
    set_env(ops, monkeypatch, env)
    bufs = run(ops, probs, ws, _p(plan), arm)
    if arm in ("g4", "sk2", "sk3", "splitall2", "splitall3"):
        # against the 8-wave kernels on the same inputs: the same products, another fp32 summation order
        set_env(ops, monkeypatch, {"LX_GEMM_BM": "256"})
        ref = run(ops, probs, None, _p("8WAVE_256"), arm + "/w256", check=False)
        for p, b, r in zip(probs, bufs, ref):
            e = close(p, block_of(p, b), block_of(p, r))
            tol = XPLAN_TOL16[fmt] if p.epi == "store" else XPLAN_TOL
            assert e < tol, f"{arm} vs 8-wave: {p.epi} rel err {e:.3e} >= {tol:.0e}"
    if arm in ("w256", "w128", "g4"):          # the small launch (p0 with 20 rows): every plan that takes it
        set_env(ops, monkeypatch, env)
        small = group(fmt, K_MAIN, 1, seed=20)
        run(ops, small, ws, _p(plan), arm + "/small")


def _no_ws_bits(ops, monkeypatch, fmt, K, arms, **lora):
    """The no-workspace plans agree bit for bit: each arm's group launch, each problem launched alone, and a row slice of each."""
    probs = group(fmt, K, main_rows0(), seed=40, **lora)
    res = {}
    for arm, env, plan in arms:
        set_env(ops, monkeypatch, env)
        bufs = run(ops, probs, None, _p(plan), arm)
        res[arm] = [block_of(p, b).clone() for p, b in zip(probs, bufs)]
    set_env(ops, monkeypatch, {})
    no_ws = {_p(n) for n in ("8WAVE_256", "8WAVE_128", "MIXED", "MIXED_2L")}
    base = arms[0][0]
    for i, p in enumerate(probs):
        b = p.own_buf()
        if p.fmt == "f16":
            p.ovf = torch.zeros(1, dtype=torch.int32, device=DEV)
        ops.gemm([p.desc(ops, b.buf[PAD:PAD + p.M, :p.N])])
        assert ops.gemm_last_plan() in no_ws
        torch.cuda.synchronize()
        b.check_footprint(f"{fmt} p{i} alone")
        alone = block_of(p, b)
        r0, r1 = SLICES[i]
        r1 = p.M if r1 is None else r1
        s = p.own_buf(r0, r1)
        ops.gemm([p.desc(ops, s.buf[PAD:PAD + r1 - r0, :p.N], r0, r1)])
        assert ops.gemm_last_plan() in no_ws
        torch.cuda.synchronize()
        s.check_footprint(f"{fmt} p{i} rows [{r0}, {r1})")
        p.check_inputs(f"{fmt} p{i} alone / rows [{r0}, {r1})")
        p.check(s, PAD, "slice", ops.gemm_last_plan(), r0, r1)
        sl = s.buf[PAD:PAD + r1 - r0, :p.ldc()]
        iv = IVIEW[alone.dtype]
        for arm, _, _ in arms:
            assert torch.equal(res[arm][i].view(iv), res[base][i].view(iv)), f"{fmt} p{i} ({p.epi}): plan {arm} differs from {base}"
        assert torch.equal(alone.view(iv), res[base][i].view(iv)), f"{fmt} p{i} ({p.epi}): launched alone it differs from the group"
        assert torch.equal(sl.view(iv), res[base][i][r0:r1].view(iv)), f"{fmt} p{i} ({p.epi}): rows [{r0}, {r1}) alone differ"


@pytest.mark.parametrize("fmt", ["bf16", "f16"])
def test_gemm_no_workspace_plans_are_bit_identical(ops, monkeypatch, fmt):
    _no_ws_bits(ops, monkeypatch, fmt, K_MAIN, [("w256", {"LX_GEMM_BM": "256"}, "8WAVE_256"), ("w128", {"LX_GEMM_BM": "128"}, "8WAVE_128"),
                                                 ("mixed", {}, "MIXED")])


# ------------------------------------------------------------------------------------------------ e4m3 operands
K_FP8 = 256


@pytest.mark.parametrize("arm", ["w256", "w128"])
def test_gemm_tiles_fp8_operands(ops, monkeypatch, arm):
    set_env(ops, monkeypatch, {"LX_GEMM_BM": arm[1:]})
    plan = _p("8WAVE_" + arm[1:])
    run(ops, group("fp8", K_FP8, main_rows0(), seed=60), None, plan, arm)
    run(ops, group("fp8", K_FP8, 1, seed=70), None, plan, arm + "/small")


def test_gemm_fp8_plans_are_bit_identical(ops, monkeypatch):
    _no_ws_bits(ops, monkeypatch, "fp8", K_FP8, [("w256", {"LX_GEMM_BM": "256"}, "8WAVE_256"), ("w128", {"LX_GEMM_BM": "128"}, "8WAVE_128")])


# ------------------------------------------------------------------------------------------------ split-bf16 (precise) operands
ARMS_SPLIT = {
    "w256": ({"LX_GEMM_BM": "256"}, False, "8WAVE_256"),
    "w128": ({"LX_GEMM_BM": "128"}, False, "8WAVE_128"),
    "g4": ({"LX_GEMM4": "2", "LX_GEMM4_SK": "0"}, True, "G4"),
    "g4sk": ({"LX_GEMM4": "2", "LX_GEMM4_SK": "1"}, True, "G4_SPLIT2"),      # 57 tiles, 16 / 24 K tiles: every tile split
}
K_SPLIT = 512


@pytest.mark.parametrize("arm", list(ARMS_SPLIT))
@pytest.mark.parametrize("segs", [2, 3])
def test_gemm_tiles_split_bf16(ops, monkeypatch, segs, arm):
    env, use_ws, plan = ARMS_SPLIT[arm]
    probs = cached_group(f"split{segs}", K_SPLIT, 1)
    set_env(ops, monkeypatch, env)
    ws = workspace(ops) if use_ws else None
    bufs = run(ops, probs, ws, _p(plan), arm)
    if arm != "w256":
        set_env(ops, monkeypatch, {"LX_GEMM_BM": "256"})
        ref = run(ops, probs, None, _p("8WAVE_256"), arm + "/w256", check=False)
        for p, b, r in zip(probs, bufs, ref):
            if p.epi != "pair":
                e = close(p, block_of(p, b), block_of(p, r))
                assert e < XPLAN_TOL, f"{arm} vs 8-wave: {p.epi} rel err {e:.3e}"


# ------------------------------------------------------------------------------------------------ the mixed plan's peel
@pytest.mark.parametrize("fmt", ["bf16", "f16"])
def test_gemm_mixed_plan_peel_into_a_shared_buffer(ops, monkeypatch, fmt):
    peel_into_a_shared_buffer(ops, monkeypatch, fmt)


def peel_into_a_shared_buffer(ops, monkeypatch, fmt, **lora):
    """Four gated-residual problems with LoRA in ONE fp32 buffer (GAP sentinel rows between them), NCU + 11 tiles: the mixed plan peels
    q3 (641 rows) entirely and q2's last two tile rows (287 of 1055 rows) into its 128-row tail, so q2's tail starts at m_base = 768,
    inside batch 7 of 100-row batches -- the gate's batch index and the LoRA rows there come from m_base. Against float64 tile by tile,
    the footprint, and bit for bit against the 8-wave plans and each problem alone. lora = the adapter inputs of all four (Prob.set_lora).
    Returns the problems and the shared buffer's contents."""
    n = ncu()
    r1 = next((r for r in range(6, 10) if (n - 12 - 2 * r) % 8 == 0 and n - 12 - 2 * r > 0), None)
    if r1 is None:
        pytest.skip(f"no peel shape for {n} CUs")
    K = 128
    rows0 = (n - 12 - 2 * r1) // 8
    probs = [Prob(fmt, 256 * (rows0 - 1) + 255, 2040, K, "res", 81, rpb=700, lora=True, **lora),
             Prob(fmt, 256 * (r1 - 1) + 129, 264, K, "res", 82, rpb=300, lora=True, **lora),
             Prob(fmt, 1055, 776, K, "res", 83, rpb=100, lora=True, **lora),
             Prob(fmt, 641, 64, K, "res", 84, rpb=160, lora=True, **lora)]
    assert tiles256(probs) == n + 11
    rows = sum(p.M for p in probs) + GAP * (len(probs) + 1)
    b = Buf(torch.float32, rows, 2040 + XCOLS, resid=True)
    row = GAP
    for p in probs:
        p.place(b, row)
        row += p.M + GAP
    b.snapshot()
    # every problem's descriptor points at its own block; run() takes its row from blocks[i]
    views = []
    for i, p in enumerate(probs):
        v = Buf.__new__(Buf)
        v.__dict__.update(b.__dict__)
        v.blocks = [b.blocks[i]]
        views.append(v)
    out = {}
    for arm, env, plan in (("mixed", {}, "MIXED"), ("w256", {"LX_GEMM_BM": "256"}, "8WAVE_256"), ("w128", {"LX_GEMM_BM": "128"}, "8WAVE_128")):
        set_env(ops, monkeypatch, env)
        run(ops, probs, None, _p(plan), "peel/" + arm, bufs=views, check=False)
        b.check_footprint("peel/" + arm)
        for p, v in zip(probs, views):
            p.check(b, v.blocks[0][0], "peel/" + arm, _p(plan))
        out[arm] = b.buf.clone()
    assert torch.equal(out["mixed"].view(torch.int32), out["w256"].view(torch.int32)), "mixed plan differs from the 256-row plan"
    assert torch.equal(out["mixed"].view(torch.int32), out["w128"].view(torch.int32)), "mixed plan differs from the 128-row plan"
    set_env(ops, monkeypatch, {})
    for p, v in zip(probs, views):
        a = p.own_buf()
        ops.gemm([p.desc(ops, a.buf[PAD:PAD + p.M, :p.N])])
        torch.cuda.synchronize()
        r = v.blocks[0][0]
        assert torch.equal(a.buf[PAD:PAD + p.M, :p.N].view(torch.int32), out["mixed"][r:r + p.M, :p.N].view(torch.int32))
        a.check_footprint("peel/alone")
        p.check_inputs("peel/alone")
    return probs, views, out["mixed"]
