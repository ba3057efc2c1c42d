"""LX_EPI_QKV, the q/k/v projection epilogue (csrc/gemm8.h gemm_epilogue_qkv, csrc/gemm4.h), tile by tile under every launch plan that
can carry it (asserted through lx_gemm_last_plan), against a float64 restatement (tests/helpers.py, pinned on the CPU by
tests/test_qkv_epilogue_ref_cpu.py) of what it does to the fp32 sums: RMSNorm(128) + RoPE on k and q, the single bf16 / e4m3 rounding, the
transposed 16-key-interleaved scatter of v into the attention kernel's V^T image. H = 2 heads, every stream with its own norm weights and
a RoPE table whose rows all differ (a row fetched for the wrong position is a wrong rotation).

  double-block launch  p0 [k|v|q], 416 rows per batch element (tiles straddle elements, the last 64-key V^T tile is half full), batch count
                       from the CU count: NCU + 17..24 tiles; p1 [k|v|q], 96 rows per element, keys in a separate image; p2 [k|v] (N = 3 D -
                       256) with a LoRA term of rank 4 (tile prologue) or 8 (epilogue; lx_gemm4_kernel's largest); p3 a plain fp32 store.
                       One shared V^T image, 64 sentinel slots between the streams. The mixed plan peels p3, p2 and p1's last tile rows:
                       p1's tail starts at m_base > 0 inside a batch element (asserted from the planner's arithmetic).
  single-block launch  one [k|v|q|mlp] problem, N = 3 D + 520, GELU from column 3 D, LoRA (rank 4, four modules), 160 rows per element;
                       the mixed plan's tail starts at m_base > 0 (with 256 CUs inside a batch element here too).
  long-K launch        288 = 3 x 96 rows + the fp32 problem at K = 6144: every tile in the two-way split form.

Per launch: two runs give the same bits; the worst 128 x 256 tile of k, q and the de-interleaved V^T against float64; every element between
rne(ref - E) and rne(ref + E) with at most NEIGHBOUR_FRAC of them not rne(ref); sentinels around and between everything the epilogue may
not write (C's v columns, C's k columns with a key image, all of bf16 with e4m3 outputs, the V^T pad slots, gaps and other streams). The
plans without a workspace agree bit for bit, one batch element launched alone reproduces its rows of the batch, lx_gemm4_kernel and its
split forms agree with the 8-wave kernels within an ulp flip. Run with -s to see the worst tile and the neighbour share of every arm."""
import json
import os

import pytest
import torch

from tests.helpers import (QKV_D, QKV_DOUBLE, QKV_SINGLE, U32, mixed_plan_keep_rows, qk_norm_rope_ref, qkv_double_shapes, qkv_single_shape,
                           vt8_slot_keys, vt_slot_keys, vt_stream_deinterleave)
from tests.test_gemm_tiles_gpu import BOUND, DEV, IVIEW, PAD, SENT, XCOLS, XPLAN_TOL, XPLAN_TOL16, Buf, Prob, _p, ncu, randn, set_env, tile_worst, workspace
from tests.test_rowops_gpu import NEIGHBOUR_FRAC, check_rounding

pytestmark = pytest.mark.gpu

H, D = 2, QKV_D
K_MAIN, K_LONG = 1536, 6144        # 24 K tiles: the smallest K of the three-way split tail; 96: the split-all form
VT_GAP = 64                        # sentinel slots between two streams of the shared V^T image
E4M3_TILE_BOUND = 4e-2             # worst e4m3 tile: tests/test_rowops_gpu.py's bound (3 significand bits: ~2.6e-2 rms of one rounding)

# arm -> (environment, workspace?, expected plan)
ARMS = {
    "w256": ({"LX_GEMM_BM": "256"}, False, "8WAVE_256"),
    "w128": ({"LX_GEMM_BM": "128"}, False, "8WAVE_128"),
    "mixed": ({}, False, "MIXED"),
    "g4": ({"LX_GEMM4": "2", "LX_GEMM4_SK": "0"}, True, "G4"),
    "sk2": ({"LX_GEMM4_SK": "2"}, True, "G4_SPLIT2"),
    "sk3": ({}, True, "G4_SPLIT3"),
    "splitall2": ({"LX_GEMM4_SK": "2"}, True, "G4_SPLIT2"),
}
NO_WS_ARMS = ("w256", "w128", "mixed")
G4_ARMS = ("g4", "sk2", "sk3", "splitall2")

REPORT = []               # (arm, output, worst tile error, bound, neighbour share or None)


@pytest.fixture(scope="module")
def ops():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from loongx_amd import ops as o
    yield o
    if REPORT:
        rows = {}
        for arm, what, err, bound, nb in REPORT:
            k = (arm, what)
            e, _, n = rows.get(k, (0.0, bound, None))
            rows[k] = (max(e, err), bound, nb if n is None else (n if nb is None else max(n, nb)))
        print(f"\nQKV_TILES worst tile and neighbour share (cap {NEIGHBOUR_FRAC:.0e}) per arm and output:")
        for (arm, what), (err, bound, nb) in sorted(rows.items()):
            print(f"  {arm:28s} {what:6s} worst {err:.3e}  bound {bound:.0e}  neighbours {'-' if nb is None else format(nb, '.2e')}")
        out = os.environ.get("LX_QKV_TILES_REPORT")
        if out:
            with open(out, "a") as f:
                for (arm, what), (err, bound, nb) in sorted(rows.items()):
                    f.write(json.dumps({"arm": arm, "output": what, "worst": err, "bound": bound, "neighbours": nb}) + "\n")


# ------------------------------------------------------------------------------------------------ one token stream = one QKV problem
class Stream:
    """A [k | v | q (| mlp)] projection of B batch elements of L rows: operands in the launch's format, norm weights, a RoPE table of L
    distinct rows, an optional LoRA term (2 slabs, modules of D columns) and the float64 reference with its fp32 error bounds."""

    def __init__(self, name, fmt, B, L, N, K, seed, R=0, toff_max=2, kimg=False, gelu=False):
        self.name, self.fmt, self.B, self.L, self.N, self.K, self.R, self.toff_max, self.kimg, self.gelu = name, fmt, B, L, N, K, R, toff_max, kimg, gelu
        self.M = M = B * L
        dt = torch.float16 if fmt == "f16" else torch.bfloat16
        self.A = randn(M, K, seed=seed + 1).to(dt)
        self.W = randn(N, K, seed=seed + 2, scale=K ** -0.5).to(dt)
        self.bias = randn(N, seed=seed + 3, scale=0.3)
        self.wq, self.wk = 1 + 0.1 * randn(128, seed=seed + 4), 1 + 0.1 * randn(128, seed=seed + 5)
        th = randn(L, 64, seed=seed + 6, scale=2.0)                   # an angle per (position, pair): every row of the table differs
        self.cs = torch.empty(L, 128, device=DEV)
        self.cs[:, 0::2], self.cs[:, 1::2] = th.cos(), th.sin()
        if R:
            self.slabs = randn(2, M, (toff_max + 1) * R, seed=seed + 7, scale=0.5).contiguous()
            self.up = randn(N, R, seed=seed + 8, scale=0.1).contiguous()
        self.ovf = torch.zeros(1, dtype=torch.int32, device=DEV) if fmt == "f16" else None
        self._ref = {}

    def rows(self, r0, r1):
        """rows [r0, r1) (whole batch elements) as a stream of their own: the same weights and table, no reference of its own"""
        assert r0 % self.L == 0 and r1 % self.L == 0
        s = Stream.__new__(Stream)
        s.__dict__.update(self.__dict__)
        s.A, s.M, s.B, s._ref = self.A[r0:r1], r1 - r0, (r1 - r0) // self.L, None
        if self.R:
            s.slabs = self.slabs[:, r0:r1]
        return s

    def ref(self):
        """name -> (float64 reference [M, cols], E or None): k, v, q (when N reaches them), mlp (GELU columns). E = the fp32 error bound
        of the kernel's expression: the K-term of the fp32 accumulation ((K + 8) U32 sum |a||w|: U32 is twice the unit roundoff, the 8
        covers bias, split parts and slab sums; the LoRA step's bf16 hi/lo products add 2^-15 sum |t||up|) carried through the norm and
        the rotation, plus their own roundings (tests/helpers.py qk_norm_rope_ref)."""
        if not self._ref:
            A, W = self.A.double(), self.W.double()
            y = A @ W.T + self.bias.double()
            mag = A.abs() @ W.abs().T + self.bias.double().abs()
            Ey = (self.K + 8) * U32 * mag
            del mag
            if self.R:
                t, ta = self.slabs.double().sum(0), self.slabs.double().abs().sum(0)
                for b in range(-(-self.N // D)):
                    m = min(b, self.toff_max) * self.R
                    c = slice(b * D, min(self.N, (b + 1) * D))
                    up = self.up[c].double()
                    y[:, c] += t[:, m:m + self.R] @ up.T
                    Ey[:, c] += (2.0 ** -15 + 8 * U32) * (ta[:, m:m + self.R] @ up.abs().T)
            r = self._ref
            r["k"] = qk_norm_rope_ref(y[:, :D], self.wk, self.cs, self.L, 0, Ey[:, :D])
            r["v"] = (y[:, D:2 * D].clone(), Ey[:, D:2 * D].clone())
            if self.N >= 3 * D:
                r["q"] = qk_norm_rope_ref(y[:, 2 * D:3 * D], self.wq, self.cs, self.L, 0, Ey[:, 2 * D:3 * D])
            if self.N > 3 * D:
                r["mlp"] = (torch.nn.functional.gelu(y[:, 3 * D:], approximate="tanh"), None)
        return self._ref


_STREAMS = {}


def stream(name, fmt, B, L, N, K, seed, **kw):
    key = (name, fmt, B, L, N, K, tuple(sorted(kw.items())))
    if key not in _STREAMS:
        _STREAMS[key] = Stream(name, fmt, B, L, N, K, seed, **kw)
    return _STREAMS[key]


_P3 = {}


def plain_problem(fmt, K):
    """p3: an fp32 store without the flag (M = 300, N = 264) -- the per-problem `n0 < 3 qkv_d` decision"""
    if (fmt, K) not in _P3:
        _P3[(fmt, K)] = Prob(fmt, QKV_DOUBLE["M3"], QKV_DOUBLE["N3"], K, "f32", 900 + len(_P3))
        if fmt == "f16":
            _P3[(fmt, K)].ovf = torch.zeros(1, dtype=torch.int32, device=DEV)
    return _P3[(fmt, K)]


def sentinel_image(shape, dtype):
    t = torch.empty(*shape, dtype=dtype, device=DEV)
    t.view(IVIEW[dtype]).fill_(SENT[dtype])
    return t


# ------------------------------------------------------------------------------------------------ a launch and its outputs
class Launch:
    """Up to three QKV streams writing into ONE V^T image at different vt_pos0 (VT_GAP sentinel slots apart), and an optional plain problem.
    f8: the e4m3 form (q8 / k8 / byte V^T image; a stream's separate key image is then left out: the two exclude each other)."""

    def __init__(self, name, streams, p3=None, f8=False):
        self.name, self.streams, self.p3, self.f8 = name, streams, p3, f8
        self.pos0, p = [], 0
        for s in streams:
            self.pos0.append(p)
            p += (s.L + 63) // 64 * 64 + VT_GAP
        self.vt_ld = p
        self.Bmax = max(s.B for s in streams)
        self.fmt = streams[0].fmt

    def shapes(self):
        return [(s.M, s.N) for s in self.streams] + ([(self.p3.M, self.p3.N)] if self.p3 else [])

    def new_outputs(self):
        o = {"C": [], "kimg": [], "q8": [], "k8": []}
        for s in self.streams:
            c = Buf(torch.bfloat16, s.M + 2 * PAD, s.N + XCOLS)
            if not self.f8:                          # what the epilogue writes of C: k (unless it has an image of its own) and q, never v
                if not s.kimg:
                    c.block(PAD, s.M, 0, D)
                if s.N >= 3 * D:
                    c.block(PAD, s.M, 2 * D, D)
            if s.N > 3 * D:
                c.block(PAD, s.M, 3 * D, s.N - 3 * D)
            c.snapshot()
            o["C"].append(c)
            kb = None
            if s.kimg and not self.f8:
                kb = Buf(torch.bfloat16, s.M + 2 * PAD, D + 8)
                kb.block(PAD, s.M, 0, D)
                kb.snapshot()
            o["kimg"].append(kb)
            for nm in ("q8", "k8"):
                b8 = None
                if self.f8 and (nm == "k8" or s.N >= 3 * D):
                    b8 = Buf(torch.uint8, s.M + 2 * PAD, D + 16)
                    b8.block(PAD, s.M, 0, D)
                    b8.snapshot()
                elif self.f8:                        # (N = 3 D - 256: no q tile runs, the pointer only has to be valid)
                    b8 = Buf(torch.uint8, s.M + 2 * PAD, D + 16)
                    b8.snapshot()
                o[nm].append(b8)
        o["VT"] = sentinel_image((self.Bmax, H, 128, self.vt_ld), torch.uint8 if self.f8 else torch.bfloat16)
        o["VT16"] = sentinel_image((self.Bmax, H, 128, self.vt_ld), torch.bfloat16) if self.f8 else None   # qkv_vt beside the byte image: never written
        o["p3"] = self.p3.own_buf() if self.p3 else None
        return o

    def reset(self, o):
        for b in o["C"] + o["kimg"] + o["q8"] + o["k8"] + [o["p3"]]:
            if b is not None:
                b.reset()
        for nm in ("VT", "VT16"):
            if o[nm] is not None:
                o[nm].view(IVIEW[o[nm].dtype]).fill_(SENT[o[nm].dtype])

    def descs(self, ops, o):
        ds = []
        for i, s in enumerate(self.streams):
            rows = slice(PAD, PAD + s.M)
            q = dict(norm_q=s.wq, norm_k=s.wk, rope=s.cs, vt=o["VT"], vt_pos0=self.pos0[i], d=D)
            if self.f8:
                q.update(q8=o["q8"][i].buf[rows, :D], k8=o["k8"][i].buf[rows, :D])
            elif s.kimg:
                q["k"] = o["kimg"][i].buf[rows, :D]
            kw = dict(bias=s.bias, epilogue=ops.LX_EPI_STORE_BF16 | (ops.LX_EPI_GELU if s.gelu else 0), rows_per_batch=s.L,
                      gelu_col_start=3 * D if s.gelu else s.N, qkv=q)
            if s.R:
                kw.update(lora_t=s.slabs[0], lora_up=s.up, lora_nsplit=2, lora_split_stride=s.slabs.stride(0), lora_mod_cols=D, lora_toff_max=s.toff_max)
            if s.fmt == "f16":
                kw.update(f16=True, f16_ovf=s.ovf)
            d = ops.gemm_desc(s.A, s.W, o["C"][i].buf[rows, :s.N], **kw)
            if self.f8:
                d.qkv_vt = o["VT16"].data_ptr()
            ds.append(d)
        if self.p3:
            ds.append(self.p3.desc(ops, o["p3"].buf[PAD:PAD + self.p3.M, :self.p3.N]))
        return ds

    def bits(self, o):
        """every output buffer of the launch as integer bit patterns, in a fixed order"""
        bufs = [b.buf for b in o["C"] + o["kimg"] + o["q8"] + o["k8"] + [o["p3"]] if b is not None] + [t for t in (o["VT"], o["VT16"]) if t is not None]
        return [t.view(IVIEW[t.dtype]) for t in bufs]

    # -- what stream i wrote, as (16-bit or byte tensor [M, cols], dequantising scale) per output --
    def got(self, ops, o, i):
        s, rows = self.streams[i], slice(PAD, PAD + self.streams[i].M)
        C = o["C"][i].buf[rows]
        g = {}
        if self.f8:
            g["k"] = (o["k8"][i].buf[rows, :D], ops.FP8_K_SCALE)
            if s.N >= 3 * D:
                g["q"] = (o["q8"][i].buf[rows, :D], ops.FP8_Q_SCALE)
        else:
            g["k"] = (o["kimg"][i].buf[rows, :D] if s.kimg else C[:, :D], 1.0)
            if s.N >= 3 * D:
                g["q"] = (C[:, 2 * D:3 * D], 1.0)
        v, _ = vt_stream_deinterleave(o["VT"][:s.B], s.L, self.pos0[i], fp8=self.f8)       # [B, H, L, 128]
        g["v"] = (v.permute(0, 2, 1, 3).reshape(s.M, D), ops.FP8_V_SCALE if self.f8 else 1.0)
        if s.N > 3 * D:
            mlp = C[:, 3 * D:s.N]
            g["mlp"] = (mlp.view(torch.float16) if s.fmt == "f16" else mlp, 1.0)
        return g

    def check(self, ops, o, arm, plan):
        tag = f"{self.name}/{arm}"
        fmt8 = "e4m3" if self.f8 else "bf16"
        for i, s in enumerate(self.streams):
            where = f"{tag} {s.name} (M={s.M} N={s.N} K={s.K} L={s.L})"
            for nm in ("C", "kimg", "q8", "k8"):
                if o[nm][i] is not None:
                    o[nm][i].check_footprint(f"{where} {nm}")
            ref = s.ref()
            for what, (got, scale) in self.got(ops, o, i).items():
                want, E = ref[what]
                if what == "mlp":                                     # the GELU columns behind the projections, as Prob.check does
                    bound = BOUND[(s.fmt, "store")]
                    err, at = tile_worst(got, want)
                    REPORT.append((tag, what, err, bound, None))
                    assert err < bound, f"{where}: worst mlp tile at {at}: rel err {err:.3e} >= {bound:.0e}"
                    continue
                assert float(want.abs().max()) * scale < 448.0, f"{where}: the reference of {what} would saturate e4m3"
                val = got.view(torch.float8_e4m3fn).double() / scale if self.f8 else got
                bound = E4M3_TILE_BOUND if self.f8 else BOUND[("bf16", "store")]
                err, at = tile_worst(val, want)
                print(f"{where} {what}: worst tile {err:.3e} (bound {bound:.0e})")
                assert err < bound, f"{where}: worst {what} tile at {at}: rel err {err:.3e} >= {bound:.0e}"
                # the scaling before the e4m3 rounding is one more fp32 product
                nb = check_rounding(f"{where} {what}", got, want * scale, E * scale + (U32 * scale * want.abs() if self.f8 else 0.0), fmt8)
                REPORT.append((tag, what, err, bound, nb))
            if s.ovf is not None:
                assert int(s.ovf) == 0
        # V^T footprint: exactly the slots of keys that exist, of the batch elements that exist, are written; everything else keeps the sentinel
        written = torch.zeros(self.Bmax, self.vt_ld, dtype=torch.bool)
        for i, s in enumerate(self.streams):
            n = (s.L + 63) // 64 * 64
            written[:s.B, self.pos0[i]:self.pos0[i] + n] = (vt8_slot_keys(n) if self.f8 else vt_slot_keys(n)) < s.L
        written = written.to(DEV)[:, None, None, :].expand_as(o["VT"])
        vt = o["VT"]
        kept = vt.view(IVIEW[vt.dtype]) == SENT[vt.dtype]
        nan = (vt & 0x7F) == 0x7F if self.f8 else ~torch.isfinite(vt.float())
        bad = ~kept & ~written
        assert not bool(bad.any()), f"{tag}: {int(bad.sum())} V^T slots outside the streams' keys were written (pad slots, gaps, other batch " \
                                    f"elements; first at {bad.nonzero()[0].tolist()})"
        bad = nan & written
        assert not bool(bad.any()), f"{tag}: {int(bad.sum())} V^T slots of existing keys were not written (first at {bad.nonzero()[0].tolist()})"
        if o["VT16"] is not None:
            assert bool((o["VT16"].view(torch.int16) == SENT[torch.bfloat16]).all()), f"{tag}: the bf16 V^T image was written beside the e4m3 one"
        if self.p3:
            o["p3"].check_footprint(f"{tag} p3")
            self.p3.check(o["p3"], PAD, tag, plan)
            if self.p3.ovf is not None:
                assert int(self.p3.ovf) == 0


_RUNS = {}


def run(ops, monkeypatch, launch, arm, env=None, plan=None, use_ws=None, check=True):
    """The launch under the arm's plan, twice with identical bits, checked; the outputs of each (launch, arm) are computed once and shared."""
    key = (launch.name, arm)
    if key in _RUNS:
        return _RUNS[key]
    a_env, a_ws, a_plan = ARMS.get(arm, ({}, False, None))
    env, use_ws, plan = a_env if env is None else env, a_ws if use_ws is None else use_ws, _p(a_plan) if plan is None else plan
    set_env(ops, monkeypatch, env)
    ws = workspace(ops) if use_ws else None
    o = launch.new_outputs()
    descs = launch.descs(ops, o)
    first = None
    for rep in range(2):
        launch.reset(o)
        ops.gemm(descs, ws)
        got = ops.gemm_last_plan()
        ok = got in plan if isinstance(plan, (set, tuple)) else got == plan
        assert ok, f"{launch.name}/{arm}: the planner chose plan {got}, not {plan} ({launch.shapes()}, {ncu()} CUs)"
        if ws is not None:
            assert ops.lib.lx_gemm_workspace_status(ws.data_ptr(), torch.cuda.current_stream().cuda_stream) == 0
        torch.cuda.synchronize()
        if rep == 0:
            first = [t.clone() for t in launch.bits(o)]
    for a, b in zip(first, launch.bits(o)):
        assert torch.equal(a, b), f"{launch.name}/{arm}: two runs of the same launch differ"
    if check:
        launch.check(ops, o, arm, ops.gemm_last_plan())
    _RUNS[key] = o
    return o


def same_bits(launch, a, b, what):
    for x, y in zip(launch.bits(a), launch.bits(b)):
        assert torch.equal(x, y), f"{launch.name}: {what}"


def close_to(ops, launch, o, base, arm):
    """lx_gemm4_kernel and its split forms against the 8-wave kernels on the same inputs: the same products, another fp32 summation order --
    an ulp flip of the 16-bit store where the two sums straddle a rounding boundary, per problem and output (the V^T image included)"""
    for i, s in enumerate(launch.streams):
        ga, gb = launch.got(ops, o, i), launch.got(ops, base, i)
        for what in ga:
            x, y = ga[what][0].double(), gb[what][0].double()
            e = float((x - y).norm() / y.norm())
            tol = XPLAN_TOL16["f16" if what == "mlp" and s.fmt == "f16" else "bf16"]
            assert e < tol, f"{launch.name}/{arm} vs 8-wave: {s.name} {what} rel err {e:.3e} >= {tol:.0e}"
    if launch.p3:
        x, y = (b.buf[PAD:PAD + launch.p3.M, :launch.p3.N].double() for b in (o["p3"], base["p3"]))
        e = float((x - y).norm() / y.norm())
        assert e < XPLAN_TOL, f"{launch.name}/{arm} vs 8-wave: p3 rel err {e:.3e} >= {XPLAN_TOL:.0e}"


# ------------------------------------------------------------------------------------------------ the launch shapes
_LAUNCHES = {}


def double_launch(fmt, R, f8=False):
    key = ("double", fmt, R, f8)
    if key not in _LAUNCHES:
        shapes = qkv_double_shapes(ncu())
        if shapes is None:
            pytest.skip(f"no double-block launch shape for {ncu()} CUs")
        d = QKV_DOUBLE
        B0 = shapes[0][0] // d["L"][0]
        st = [stream("p0", fmt, B0, d["L"][0], d["N"][0], K_MAIN, 1000),
              stream("p1", fmt, d["B"][1], d["L"][1], d["N"][1], K_MAIN, 1100, kimg=True),
              stream("p2", fmt, d["B"][2], d["L"][2], d["N"][2], K_MAIN, 1200 + R, R=R, toff_max=2)]
        assert [(s.M, s.N) for s in st] == shapes[:3]
        _LAUNCHES[key] = Launch(f"double/{fmt}/R{R}" + ("/e4m3" if f8 else ""), st, plain_problem(fmt, K_MAIN), f8)
    return _LAUNCHES[key]


def single_launch(fmt, f8=False):
    key = ("single", fmt, f8)
    if key not in _LAUNCHES:
        shapes = qkv_single_shape(ncu())
        if shapes is None:
            pytest.skip(f"no single-block launch shape for {ncu()} CUs")
        d = QKV_SINGLE
        st = [stream("s0", fmt, shapes[0][0] // d["L"], d["L"], d["N"], K_MAIN, 1300, R=4, toff_max=3, gelu=True)]
        _LAUNCHES[key] = Launch(f"single/{fmt}" + ("/e4m3" if f8 else ""), st, None, f8)
    return _LAUNCHES[key]


def assert_peel(launch, inside_an_element):
    """The mixed plan's 128-row tail holds QKV rows that start at m_base > 0 and, for the double-block launch, inside a batch element
    (m_base % rows_per_batch != 0) -- from the planner's arithmetic, restated in tests/helpers.py and pinned by
    tests/test_qkv_epilogue_ref_cpu.py: the case cannot disappear on a device with another CU count. The single-block launch keeps a
    multiple of 256 rows of 160-row elements: inside an element unless that is a multiple of 1280 (it is inside one with 256 CUs, not
    with 304), so only m_base > 0 is required of it."""
    keep = mixed_plan_keep_rows(launch.shapes(), ncu())
    assert keep is not None, (launch.shapes(), ncu())
    hit = [s.name for s, k in zip(launch.streams, keep) if 0 < k < s.M and (k % s.L != 0 or not inside_an_element)]
    assert hit, f"{launch.name}: no QKV problem is peeled at m_base > 0{' inside a batch element' if inside_an_element else ''} " \
                f"(keep_rows {keep}, {ncu()} CUs)"


def launch_under(ops, monkeypatch, launch, arm):
    if arm == "mixed":
        assert_peel(launch, inside_an_element=launch.p3 is not None)
    o = run(ops, monkeypatch, launch, arm)
    if arm in G4_ARMS:
        close_to(ops, launch, o, run(ops, monkeypatch, launch, "w256"), arm)


CASES16 = [("bf16", a) for a in ("w256", "w128", "mixed", "g4", "sk2", "sk3")] + [("f16", a) for a in ("mixed", "g4", "sk2")]


@pytest.mark.parametrize("R", [4, 8])
@pytest.mark.parametrize("fmt,arm", CASES16)
def test_double_block_launch(ops, monkeypatch, fmt, arm, R):
    launch_under(ops, monkeypatch, double_launch(fmt, R), arm)


@pytest.mark.parametrize("fmt,arm", CASES16)
def test_single_block_launch(ops, monkeypatch, fmt, arm):
    launch_under(ops, monkeypatch, single_launch(fmt), arm)


def test_long_k_launch_in_the_split_form(ops, monkeypatch):
    """K = 6144, fewer tiles than CUs: every tile is shared by two workgroups (three batch elements of 96 rows inside the first tile row)"""
    st = [stream("l0", "bf16", 3, 96, 3 * D, K_LONG, 1400)]
    launch = Launch("long/bf16", st, plain_problem("bf16", K_LONG))
    t = sum(-(-M // 256) * -(-N // 256) for M, N in launch.shapes())
    assert t <= 128 and 2 * t <= ncu(), t
    launch_under(ops, monkeypatch, launch, "splitall2")


@pytest.mark.parametrize("arm", NO_WS_ARMS)
@pytest.mark.parametrize("shape", ["double", "single"])
def test_e4m3_images(ops, monkeypatch, shape, arm):
    """q8 / k8 / the byte V^T image (scales ops.FP8_*_SCALE): the form that lives on the 8-wave kernels. Nothing in bf16 is written."""
    launch = double_launch("bf16", 4, f8=True) if shape == "double" else single_launch("bf16", f8=True)
    if arm == "mixed":
        assert_peel(launch, inside_an_element=shape == "double")
    run(ops, monkeypatch, launch, arm)


@pytest.mark.parametrize("shape", ["double", "single"])
def test_e4m3_images_never_take_a_g4_plan(ops, monkeypatch, shape):
    """With a workspace and LX_GEMM4 = 2 the planner still keeps the e4m3 form off lx_gemm4_kernel (csrc/gemm.hip), and what it runs instead
    is the no-workspace plan's result bit for bit."""
    launch = double_launch("bf16", 4, f8=True) if shape == "double" else single_launch("bf16", f8=True)
    no_ws = (_p("8WAVE_256"), _p("8WAVE_128"), _p("MIXED"), _p("MIXED_2L"))
    o = run(ops, monkeypatch, launch, "g4-asked", env={"LX_GEMM4": "2"}, plan=no_ws, use_ws=True)
    same_bits(launch, o, run(ops, monkeypatch, launch, "mixed"), "with a workspace and LX_GEMM4 = 2 the e4m3 form differs from the mixed plan")


@pytest.mark.parametrize("kind", ["double/bf16", "double/f16", "double/e4m3", "single/bf16", "single/e4m3"])
def test_no_workspace_plans_are_bit_identical(ops, monkeypatch, kind):
    """include/lx.h: without a workspace the plans do not depend on the batch size -- k, q, V^T and the e4m3 images are the same bits
    whichever of the three runs (the mixed plan's tail decodes position and batch element from m_base + m)."""
    shape, f = kind.split("/")
    fmt, f8 = ("bf16", True) if f == "e4m3" else (f, False)
    launch = double_launch(fmt, 4, f8) if shape == "double" else single_launch(fmt, f8)
    base = run(ops, monkeypatch, launch, "w256")
    for arm in ("w128", "mixed"):
        same_bits(launch, run(ops, monkeypatch, launch, arm), base, f"plan {arm} differs from w256")


@pytest.mark.parametrize("f8", [False, True])
def test_one_batch_element_alone_reproduces_its_rows(ops, monkeypatch, f8):
    """The data-parallel-shard property: a batch element of p0 (one that starts inside a tile of the big launch) launched alone, B = 1,
    with the same table and a V^T image of its own, gives its rows of k / q and its V^T rows of the big launch bit for bit."""
    big = double_launch("bf16", 4, f8)
    p0 = big.streams[0]
    b = next(b for b in range(p0.B // 3, p0.B) if (b * p0.L) % 256 not in (0, 128))
    alone = Launch(f"alone/b{b}" + ("/e4m3" if f8 else ""), [p0.rows(b * p0.L, (b + 1) * p0.L)], None, f8)
    no_ws = (_p("8WAVE_256"), _p("8WAVE_128"), _p("MIXED"), _p("MIXED_2L"))
    oa = run(ops, monkeypatch, alone, "alone", env={}, plan=no_ws, use_ws=False, check=False)
    ob = run(ops, monkeypatch, big, "mixed")
    ga, gb = alone.got(ops, oa, 0), big.got(ops, ob, 0)
    for what in ga:
        x, y = ga[what][0], gb[what][0][b * p0.L:(b + 1) * p0.L]
        assert torch.equal(x.view(IVIEW[x.dtype]), y.view(IVIEW[y.dtype])), f"batch element {b} alone: {what} differs from the batch"
    n = (p0.L + 63) // 64 * 64
    x, y = oa["VT"][0, :, :, :n], ob["VT"][b, :, :, :n]
    assert torch.equal(x.view(IVIEW[x.dtype]), y.view(IVIEW[y.dtype])), f"batch element {b} alone: its V^T rows differ from the batch"
