"""The row kernels of the denoise step, row by row, against a float64 reference of the exact inputs each kernel read (the 16-bit and e4m3
images as stored, the fp32 tables): AdaLN LayerNorm + modulation in every form (csrc/rowops.hip, fp8.hip, precise.hip), per-head RMSNorm +
RoPE with its V^T images, the LoRA down-projections, the RoPE tables, the skinny linear and the grid-stride converters.

Every launch is held to:
  * worst row: the relative L2 error of the worst output row -- per (row, head) 128-vector for q / k -- within the format's bound. fp32
    dot-product outputs (LoRA T, the skinny linear) are normalised by the row's absolute sum |x| . |w|, since a single output can cancel;
  * rounding: every 16-bit or e4m3 element is the correctly rounded float64 value, up to the fp32 arithmetic error E of the kernel's own
    expression: it must lie between rne(ref - E) and rne(ref + E), and only a small fraction may differ from rne(ref) at all. E is
    derived per element from the fp32 error of the summands (ln_ref / qk_ref below), so cancelling elements get what they need;
  * footprint: outputs live in sentinel-filled buffers (rows around and between segments, leading dimensions wider than the data,
    foreign columns, V^T slots outside [vt_pos0, vt_pos0 + pad64(L)), T rows / columns past R, every K-split slab): nothing outside the
    documented outputs changes, nothing inside stays at the sentinel or is non-finite, V^T padding slots are zero;
  * determinism: the same launch twice gives the same bits;
  * row-position invariance: a row gives the same bits launched alone or inside a three-segment launch (include/lx.h: one wave per
    LayerNorm row with a fixed reduction order, 16 lanes per (row, head) with fixed shuffles).

Run with -s to see the worst row of every arm against its bound."""
import pytest
import torch

pytestmark = pytest.mark.gpu

DEV = "cuda"
PAD, GAP = 2, 3           # sentinel rows above / below every output block, and between segments
U32 = 2.0 ** -23          # fp32 ulp at 1 (twice the unit roundoff: the error terms below are upper bounds)
NEIGHBOUR_FRAC = 1e-3     # elements that may be the neighbour of rne(ref) (fp32 error near a rounding tie, ~1e-7 relative)

SENT = {torch.bfloat16: 0x7FA5, torch.float16: 0x7E5A, torch.float32: 0x7FC0BEEF, torch.uint8: 0x7F}
IVIEW = {torch.bfloat16: torch.int16, torch.float16: torch.int16, torch.float32: torch.int32, torch.uint8: torch.uint8}
E4M3 = torch.float8_e4m3fn

# worst-row bounds: the whole-tensor bounds of test_kernels_gpu.py / test_f16_gpu.py / test_precise_gpu.py / test_fp8_gemm_gpu.py
BOUND = {"bf16": 4e-3, "f16": 5e-4, "f32": 4e-6, "lora": 2e-6, "split_qk": 5e-6, "split_ln": 2e-5, "e4m3": 4e-2, "skinny": 1e-5}

REPORT = []               # (arm, output, worst, bound, neighbour fraction)


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
            if k not in rows or err / bound > rows[k][0] / rows[k][1]:
                rows[k] = (err, bound, max(nb, rows.get(k, (0, 0, 0))[2]))
        print("\nROWOPS worst row per arm:")
        for (arm, what), (err, bound, nb) in sorted(rows.items()):
            print(f"  {arm:28s} {what:10s} worst {err:.3e}  bound {bound:.0e}  neighbours {nb:.1e}")


def report(arm, what, err, bound, nb=0.0):
    REPORT.append((arm, what, float(err), bound, float(nb)))
    assert err < bound, f"{arm} {what}: worst row {err:.3e} >= {bound:.0e}"


def randn(*shape, seed, scale=1.0, dtype=torch.float32):
    g = torch.Generator(device=DEV).manual_seed(seed)
    return (torch.randn(*shape, generator=g, device=DEV) * scale).to(dtype)


def sentinel(shape, dtype):
    t = torch.empty(*shape, dtype=dtype, device=DEV)
    t.view(IVIEW[dtype]).fill_(SENT[dtype])      # (every pattern is positive in its integer view)
    return t


def bits(t):
    return t.view(IVIEW[t.dtype])


def check_footprint(what, buf, inside, init=None):
    """buf outside the boolean mask `inside` keeps the bits of init (default: the sentinel); inside is finite and not the sentinel."""
    b = bits(buf)
    ref = bits(init) if init is not None else bits(sentinel((1,), buf.dtype))[0]
    changed = b != ref
    out = changed & ~inside
    assert not bool(out.any()), f"{what}: {int(out.sum())} elements outside the outputs changed (first at {out.nonzero()[0].tolist()})"
    vals = buf[inside]
    if buf.dtype == torch.uint8:
        bad = (vals & 0x7F) == 0x7F
    else:
        bad = ~torch.isfinite(vals.float())
        if init is None:
            bad |= bits(vals) == bits(sentinel((1,), buf.dtype))[0]
    assert not bool(bad.any()), f"{what}: {int(bad.sum())} elements inside the outputs are non-finite / unwritten"


def row_worst(got, ref, denom=None):
    """max over rows (last dim) of ||got - ref|| / ||denom|| (denom defaults to ref)"""
    got, ref = got.double(), ref.double()
    d = (got - ref).flatten(0, -2).norm(dim=-1)
    n = (ref if denom is None else denom).double().flatten(0, -2).norm(dim=-1)
    return float((d / n.clamp_min(1e-300)).max()) if d.numel() else 0.0


def rne(x64, fmt):
    if fmt == "e4m3":
        return x64.clamp(-448.0, 448.0).to(E4M3).view(torch.uint8)
    return x64.to(torch.bfloat16 if fmt == "bf16" else torch.float16)


def codes(t):
    """ordered integer code of 16-bit / e4m3 bit patterns (rounding is monotonic in it; +0 and -0 are both 0)"""
    if t.dtype == torch.uint8:
        b = t.to(torch.int32)
        m, s = b & 0x7F, b >> 7
    else:
        b = t.view(torch.int16).to(torch.int32) & 0xFFFF
        m, s = b & 0x7FFF, b >> 15
    return torch.where(s == 1, -m, m)


def check_rounding(what, got, ref, E, fmt, frac=NEIGHBOUR_FRAC, frac_mask=None):
    """got (16-bit tensor, or uint8 e4m3 codes) between rne(ref - E) and rne(ref + E); returns the fraction that is not rne(ref)."""
    g, lo, hi, c = codes(got), codes(rne(ref - E, fmt)), codes(rne(ref + E, fmt)), codes(rne(ref, fmt))
    bad = (g < lo) | (g > hi)
    if bool(bad.any()):
        i = tuple(bad.nonzero()[0].tolist())
        raise AssertionError(f"{what}: {int(bad.sum())} of {g.numel()} elements are not the rounded reference (first at {list(i)}: got "
                             f"code {int(g[i])}, reference {float(ref[i]):.9g} +- {float(E[i]):.3g} -> codes {int(lo[i])}..{int(hi[i])})")
    nb = g != c
    if frac_mask is not None:
        nb = nb[frac_mask]
    f = float(nb.double().mean()) if nb.numel() else 0.0
    assert f <= frac, f"{what}: {f:.2e} of the elements are a neighbour of the rounded reference (> {frac:.0e}): truncating pack?"
    return f


def deq8(u8):
    return u8.view(E4M3).double()


# ================================================================================================ AdaLN LayerNorm + modulation
LN_FORMS = ["plain", "segs", "f16", "lora", "lora_f16", "fp8_y", "fp8_noy", "split"]
LN_D = [3072, 256, 1024, 520, 4, 16384]
LN_SEGS = {3072: [(7, 2), (3, 5), (9, 1)], 256: [(5, 3), (2, 4), (12, 1)], 1024: [(4, 5), (3, 3), (8, 2)],   # (rows_per_batch, batches)
           520: [(6, 2), (1, 5), (9, 1)], 4: [(3, 3), (7, 1), (2, 5)], 16384: [(2, 2), (1, 3), (4, 1)]}     # M % 4 = 2, 3, 1, 2, 3, 3
LN_Y8_SCALE = 64.0        # a power of two (o * s8 is exact); |o| > 7 saturates


def _ln_params():
    out = []
    for form in LN_FORMS:
        for D in LN_D:
            if form.startswith("lora"):
                if D in (3072, 256):
                    out += [pytest.param(form, D, R, id=f"{form}-D{D}-R{R}") for R in (1, 3, 4, 5, 12, 16)]
            else:
                out.append(pytest.param(form, D, 0, id=f"{form}-D{D}"))
    return out


class LnCase:
    def __init__(self, form, D):
        self.form, self.D = form, D
        self.eps = 1e-5 if D in (520, 256) else 1e-6
        segs = LN_SEGS[D] if form != "plain" else [(7, 3)]
        self.n = [L * B for L, B in segs]
        # physical order: segment 2, segment 0, segment 1 (row0 out of launch order, GAP untouched rows between them)
        order = [2, 0, 1] if len(segs) == 3 else [0]
        self.row0, r = [0] * len(segs), PAD
        for i in order:
            self.row0[i] = r
            r += self.n[i] + GAP
        self.Mphys = r - GAP + PAD
        self.ldx, self.ldy, self.ldy8 = D + 8, D + 12, D + 20
        self.mod_ld = 6 * D + 8
        self.X = randn(self.Mphys, self.ldx, seed=D + 1, scale=2.0) + 0.3
        rows = [self.row0[i] + j for i in range(len(segs)) for j in range(self.n[i])]
        self.phys = torch.tensor(rows, device=DEV)                     # launch order -> physical row
        kind = torch.arange(len(rows), device=DEV)
        self.offset_rows = self.phys[kind % 7 == 3]                    # 1e3 + N(0, 1): the variance must stay two-pass
        self.const_rows = self.phys[kind % 11 == 5]                    # constant: every partial sum exact, variance 0 -> y = shift
        self.X[self.offset_rows] = 1e3 + randn(len(self.offset_rows), self.ldx, seed=D + 2)
        for j, r_ in enumerate(self.const_rows.tolist()):
            self.X[r_] = 0.5 if j % 2 == 0 else 3.0
        # one wide [B, mod_ld] table (shift / scale at column offsets), a second one for the last segment (the engine's cmods);
        # batch 2's shift is large: its rows saturate the e4m3 image
        self.tabs = [randn(5, self.mod_ld, seed=D + 3, scale=0.5), randn(5, self.mod_ld, seed=D + 4, scale=0.5)]
        for t in self.tabs:
            t[2, D + 4:2 * D + 4] *= 20.0
        self.segs = []
        for i, (L, B) in enumerate(segs):
            t = self.tabs[1] if i == 2 else self.tabs[0]
            self.segs.append((self.row0[i], self.n[i], L, t[:, D + 4:], t[:, 3 * D + 4:]))
        # float64 reference per launched row
        b_of = torch.cat([torch.arange(n_, device=DEV) // L for n_, (L, B) in zip(self.n, segs)])
        tab_of = torch.cat([torch.full((n_,), 1 if i == 2 else 0, device=DEV) for i, n_ in enumerate(self.n)])
        tabs64 = torch.stack(self.tabs).double()
        self.shift = tabs64[tab_of, b_of, D + 4:2 * D + 4]
        self.scale = tabs64[tab_of, b_of, 3 * D + 4:4 * D + 4]
        self.o, self.E = self.ln_ref()

    def ln_ref(self):
        """o = (x - mean) * rstd * (1 + scale) + shift in float64, and E, a bound on |o_fp32 - o| of the kernel's fp32 evaluation:
          mean: D fp32 additions in a tree of depth D / 256 + 2 per lane plus 6 shuffle levels, error <= c U32 mean|x| with
                c = D / 256 + 9 (U32 is two unit roundoffs: twice the worst-case depth bound);
          x - mean, (.)^2, the variance sum (same c) and rsqrtf (<= 2 ulp): rstd relative error <= (c / 2 + 3) U32;
          t = (x - mean) * rstd * (1 + scale): three more roundings; its error is
              |t| (c / 2 + 6) U32 + rstd |1 + scale| c U32 mean|x|      (the second term: the mean's error times rstd);
          o = t + shift: one more rounding, <= U32 (|t| + |shift|)."""
        D = self.D
        x = self.X[self.phys, :D].double()
        eps = float(torch.tensor(self.eps, dtype=torch.float32))
        m = x.mean(1, keepdim=True)
        rstd = 1.0 / torch.sqrt(((x - m) ** 2).mean(1, keepdim=True) + eps)
        t = (x - m) * rstd * (1.0 + self.scale)
        o = t + self.shift
        c = D / 256 + 9
        E = t.abs() * (c / 2 + 6) * U32 + rstd * (1.0 + self.scale).abs() * c * U32 * x.abs().mean(1, keepdim=True) \
            + U32 * (t.abs() + self.shift.abs())
        return o, E

    def outputs(self, lora=None):
        D, fm = self.D, self.form
        out = {}
        if fm in ("plain", "segs", "lora", "fp8_y"):
            out["Y"] = sentinel((self.Mphys, self.ldy), torch.bfloat16)
        if fm in ("f16", "lora_f16"):
            out["Y"] = sentinel((self.Mphys, self.ldy), torch.float16)
        if fm.startswith("fp8"):
            out["Y8"] = sentinel((self.Mphys, self.ldy8), torch.uint8)
        if fm == "split":
            out["Y"] = sentinel((self.Mphys, 2 * D + 24), torch.bfloat16)
        if fm.startswith("lora"):
            out["T"] = sentinel((lora["rows"] + 2 * PAD, lora["ldt"]), torch.float32)
        out["ovf"] = torch.zeros(1, dtype=torch.int32, device=DEV)
        return out

    def launch(self, ops, out, seg_idx=None, lora=None):
        D, fm = self.D, self.form
        segs = self.segs if seg_idx is None else [self.segs[i] for i in seg_idx]
        if fm == "plain":
            r0, n, L, sh, sc = self.segs[0]
            ops.ln_modulate(self.X[r0:r0 + n, :D], sh, sc, out["Y"][r0:r0 + n, :D], rows_per_batch=L, eps=self.eps, mod_ld=self.mod_ld)
        elif fm in ("segs", "f16"):
            ops.ln_modulate_segs(self.X[:, :D], segs, out["Y"][:, :D], self.mod_ld, eps=self.eps, f16_ovf=out["ovf"] if fm == "f16" else None)
        elif fm.startswith("lora"):
            T = out["T"][PAD:PAD + lora["rows"], :lora["R"]]
            ops.ln_modulate_segs(self.X[:, :D], segs, out["Y"][:, :D], self.mod_ld, eps=self.eps, lora=(lora["A"], T, lora["row0"], lora["rows"]),
                                 f16_ovf=out["ovf"] if fm == "lora_f16" else None)
        elif fm.startswith("fp8"):
            ops.ln_modulate_fp8_segs(self.X[:, :D], segs, out["Y"][:, :D] if "Y" in out else None, out["Y8"][:, :D], self.mod_ld, LN_Y8_SCALE,
                                     eps=self.eps)
        else:
            ops.ln_modulate_split_segs(self.X[:, :D], segs, out["Y"][:, :2 * D + 24], self.mod_ld, D + 8, eps=self.eps)
        torch.cuda.synchronize()


@pytest.mark.parametrize("form,D,R", _ln_params())
def test_ln_modulate_rows(ops, form, D, R):
    c = LnCase(form, D)
    arm = f"ln {form} D={D}" + (f" R={R}" if R else "")
    lora = None
    if form.startswith("lora"):
        # adapter rows: from the middle of segment 0's first workgroup, across the gap rows, into segment 1
        r0 = c.row0[0] + 1
        rows = c.row0[1] + 3 - r0
        A = randn(R, D, seed=D + 9, scale=D ** -0.5).to(torch.float16 if form == "lora_f16" else torch.bfloat16)
        lora = {"A": A, "R": R, "row0": r0, "rows": rows, "ldt": R + 3 if R % 2 else 17}
    out = c.outputs(lora)
    c.launch(ops, out, lora=lora)
    fmt = {"plain": "bf16", "segs": "bf16", "f16": "f16", "lora": "bf16", "lora_f16": "f16", "fp8_y": "bf16", "split": "bf16"}.get(form)
    phys, o, E = c.phys, c.o, c.E
    rand_rows = ~torch.isin(phys, torch.cat([c.offset_rows, c.const_rows]))
    inside = {}
    # ---- the 16-bit image (or the hi half of the split pair)
    if "Y" in out:
        Y = out["Y"][phys, :D]
        nb = check_rounding(f"{arm} Y", Y, o, E, fmt, frac_mask=rand_rows)
        report(arm, "Y" if form != "split" else "hi", row_worst(Y, o), BOUND[fmt], nb)
        const = torch.isin(phys, c.const_rows)
        assert torch.equal(bits(Y[const]), bits(rne(c.shift[const], fmt))), f"{arm}: a constant row is not shift rounded to {fmt}"
        m = torch.zeros(out["Y"].shape, dtype=torch.bool, device=DEV)
        m[phys, :D] = True
        if form == "split":
            lo = out["Y"][phys, D + 8:2 * D + 8]
            check_rounding(f"{arm} lo", lo, o - Y.double(), E, "bf16", frac=1.0)
            # the pair carries 16 bits; on the 1e3-offset rows the fp32 mean alone is off by ~1e3 U32 (E above), so the pair bound holds
            # on the other rows and the offset rows are held element by element by the hi / lo rounding checks against E
            report(arm, "pair", row_worst((Y.double() + lo.double())[rand_rows | const], o[rand_rows | const]), BOUND["split_ln"])
            m[phys, D + 8:2 * D + 8] = True
        inside["Y"] = m
    # ---- the e4m3 image
    if "Y8" in out:
        Y8 = out["Y8"][phys, :D]
        s = LN_Y8_SCALE
        nb = check_rounding(f"{arm} Y8", Y8, o * s, E * s + U32 * (o * s).abs(), "e4m3", frac_mask=rand_rows)
        # (a row of 4 correctly rounded e4m3 values can be off by up to the format's half ulp, 2^-4: the 4e-2 bound needs longer rows)
        report(arm, "Y8", row_worst(deq8(Y8), (o * s).clamp(-448, 448)), BOUND["e4m3"] if D >= 128 else 2.0 ** -4, nb)
        assert bool((Y8.view(E4M3).float().abs() == 448).any()), f"{arm}: no row reached e4m3 saturation"
        m = torch.zeros(out["Y8"].shape, dtype=torch.bool, device=DEV)
        m[phys, :D] = True
        inside["Y8"] = m
    # ---- the fused LoRA down-projection: T[pr - row0] = Y_row . A^T for the launched adapter rows, gap rows keep the sentinel
    if lora is not None:
        f16 = form == "lora_f16"
        base = out["Y"]
        ref_out = c.outputs(lora)                                     # the plain form of the same launch: Y bit for bit
        c.form = "f16" if f16 else "segs"
        c.launch(ops, ref_out)
        c.form = form
        assert torch.equal(bits(base), bits(ref_out["Y"])), f"{arm}: Y differs from the form without the adapter"
        ad = [p for p in phys.tolist() if lora["row0"] <= p < lora["row0"] + lora["rows"]]
        ad_t = torch.tensor(ad, device=DEV)
        Ys, A64 = out["Y"][ad_t, :D].double(), lora["A"].double()
        T = out["T"][PAD + ad_t - lora["row0"], :R]
        report(arm, "T", row_worst(T, Ys @ A64.T, Ys.abs() @ A64.abs().T), BOUND["lora"])
        m = torch.zeros(out["T"].shape, dtype=torch.bool, device=DEV)
        m[PAD + ad_t - lora["row0"], :R] = True
        inside["T"] = m
        assert len(ad) < lora["rows"], "the adapter rows must cover a gap row"
    if form in ("f16", "lora_f16"):
        assert int(out["ovf"]) == 0, f"{arm}: f16_ovf counted a clipped wave in range"
    for k, m in inside.items():
        check_footprint(f"{arm} {k}", out[k], m)
    # ---- determinism
    again = c.outputs(lora)
    c.launch(ops, again, lora=lora)
    for k in inside:
        assert torch.equal(bits(out[k]), bits(again[k])), f"{arm}: {k} differs between two identical launches"
    # ---- row-position invariance: segment 0 alone, segments 1 and 2 as a two-segment launch
    if form != "plain":
        for idx in ([0], [1, 2]):
            alone = c.outputs(lora)
            c.launch(ops, alone, seg_idx=idx, lora=lora)
            rows = torch.cat([torch.arange(c.row0[i], c.row0[i] + c.n[i], device=DEV) for i in idx])
            for k in inside:
                if k == "T":
                    tr = rows[(rows >= lora["row0"]) & (rows < lora["row0"] + lora["rows"])] - lora["row0"] + PAD
                    assert torch.equal(bits(out[k][tr]), bits(alone[k][tr])), f"{arm}: T rows of segments {idx} depend on the launch"
                else:
                    assert torch.equal(bits(out[k][rows]), bits(alone[k][rows])), f"{arm}: {k} rows of segments {idx} depend on the launch"


# ================================================================================================ q / k prep
QK_CFG = {"h1": (1, [65, 1, 200], 5), "h3": (3, [64, 512, 63], 2), "h24": (24, [1, 63, 65], 1)}       # H, segment lengths, n_batches
QK_FORMS = ["single", "fast", "general", "f16in", "fp8", "fp8_f16in", "f32", "split"]
PARTIAL = {"general", "f16in", "fp8", "f32"}            # segment 1 without RoPE tables, segment 2 without norm_q: the general body
PERM16 = [0, 1, 2, 3, 8, 9, 10, 11, 4, 5, 6, 7, 12, 13, 14, 15]


def pad64(n):
    return (n + 63) // 64 * 64


def vt_key(j):            # V^T slot within a segment's image -> source key (16-key interleave, qkv_prep_kernel)
    return (j // 16) * 16 + torch.tensor(PERM16, device=DEV)[j % 16]


def vt8_key(j):           # VT8 byte position -> key (qkv_prep_fp8_kernel, the f8f6f4 MFMA B-operand order)
    t, q = j // 64, j % 64
    g, p = q // 32, q % 32
    return t * 64 + (p // 16) * 32 + 8 * ((p % 16) // 4) + 4 * g + (p % 4)


class QkCase:
    def __init__(self, ops, form, cfg):
        self.form = form
        H, lens, B = QK_CFG[cfg]
        if form == "single":
            lens = lens[:1]
        self.H, self.lens, self.B, self.D = H, lens, B, H * 128
        D = self.D
        ns = len(lens)
        order = [1, 2, 0][:ns] if ns == 3 else [0]
        self.row0, r = [0] * ns, PAD
        for i in order:
            self.row0[i] = r
            r += B * lens[i] + GAP
        self.Mphys = r - GAP + PAD
        vorder = [2, 0, 1] if ns == 3 else [0]
        self.vt0, p = [0] * ns, 64
        for i in vorder:
            self.vt0[i] = p
            p += pad64(lens[i]) + 64
        self.vt_ld = p + 64
        # columns: [16 foreign | k | 8 foreign | v | q | 32 foreign] (the single blocks' layout: k, v, q in a non-default order)
        self.k_col, self.v_col, self.q_col, self.ld = 16, 24 + D, 24 + 2 * D, 3 * D + 56
        f32in = form in ("f32", "split")
        src = randn(self.Mphys, self.ld, seed=7 * H + 1)
        if not f32in:    # values exactly representable in bf16 and fp16 (|x| >= 2^-14 or 0)
            src = src.to(torch.bfloat16).float()
            src[src.abs() < 2 ** -14] = 0.0
        self.x = src
        self.buf = src.to(torch.float16 if form in ("f16in", "fp8_f16in") else (torch.float32 if f32in else torch.bfloat16))
        # RoPE tables: one cos_main over all streams, sliced per segment (the engine slices it per stream)
        Lt = sum(lens) + 5
        ids = torch.zeros(Lt, 3, device=DEV)
        ids[:, 1] = torch.arange(Lt, device=DEV) // 11
        ids[:, 2] = torch.arange(Lt, device=DEV) % 11 - 4
        self.cos, self.sin = ops.rope_table(ids)
        offs, o = [], 5
        for L in lens:
            offs.append(o)
            o += L
        self.segs = []
        for i, L in enumerate(lens):
            wq, wk = 1 + 0.2 * randn(128, seed=50 + i), 1 + 0.2 * randn(128, seed=60 + i)
            ct, st = self.cos[offs[i]:offs[i] + L], self.sin[offs[i]:offs[i] + L]
            if form in PARTIAL and i == 1:
                ct = st = None
            if form in PARTIAL and i == 2:
                wq = None
            self.segs.append((self.row0[i], L, self.vt0[i], wq, wk, ct, st))

    def qk_ref(self, i, which):
        """q or k of segment i, [B, L, H, 128] float64, and E, a bound on the fp32 error of the kernel's evaluation:
        RMSNorm: 128 squares summed (8 per lane, then 4 shuffles), rsqrtf and two products: relative <= 12 U32 on x r w;
        RoPE x c - x' s: two products and a difference, <= 4 U32 (|x c| + |x' s|) on top."""
        r0, L, _, wq, wk, ct, st = self.segs[i]
        col = self.q_col if which == "q" else self.k_col
        w = wq if which == "q" else wk
        B, H = self.B, self.H
        x = self.x[r0:r0 + B * L, col:col + H * 128].double().view(B, L, H, 128)
        if w is not None:
            x = x * torch.rsqrt((x * x).mean(-1, keepdim=True) + 1e-6) * w.double()
        if ct is None:
            return x, 12 * U32 * x.abs()
        c, s = ct.double()[None, :, None], st.double()[None, :, None]
        xr = torch.stack([-x[..., 1::2], x[..., 0::2]], -1).flatten(-2)
        y = x * c + xr * s
        return y, 16 * U32 * ((x * c).abs() + (xr * s).abs())

    def v_in(self, i):
        r0, L = self.segs[i][0], self.segs[i][1]
        return self.buf[r0:r0 + self.B * L, self.v_col:self.v_col + self.D].view(self.B, L, self.H, 128)

    def new_outputs(self):
        fm, D = self.form, self.D
        out = {}
        if fm in ("single", "fast", "general", "f16in"):
            out["QKV"] = self.buf.clone()
            out["VT"] = sentinel((self.B, self.H, 128, self.vt_ld), torch.bfloat16)
        elif fm.startswith("fp8"):
            out["QKV"] = self.buf.clone()
            out["Q8"] = sentinel((self.Mphys, D + 32), torch.uint8)
            out["K8"] = sentinel((self.Mphys, D + 32), torch.uint8)
            out["VT8"] = sentinel((self.B, self.H, 128, self.vt_ld), torch.uint8)
        elif fm == "f32":
            out["QKV"] = self.buf.clone()
        else:
            out["QKV"] = self.buf.clone()
            out["QK2"] = sentinel((self.Mphys, 4 * D + 48), torch.bfloat16)
            out["VT2"] = sentinel((2, self.B, self.H, 128, self.vt_ld), torch.bfloat16)
        return out

    def launch(self, ops, out, seg_idx=None):
        fm, H, B = self.form, self.H, self.B
        segs = self.segs if seg_idx is None else [self.segs[i] for i in seg_idx]
        a = (out["QKV"], self.q_col, self.k_col, self.v_col)
        if fm == "single":
            r0, L, vt0, wq, wk, ct, st = segs[0]
            ops.qkv_prep(*a, row0=r0, n_rows=B * L, rows_per_batch=L, H=H, wq=wq, wk=wk, cos=ct, sin=st, VT=out["VT"], vt_pos0=vt0)
        elif fm in ("fast", "general", "f16in"):
            ops.qkv_prep_segs(*a, segs, B, H, out["VT"], in_f16=fm == "f16in")
        elif fm.startswith("fp8"):
            ops.qkv_prep_fp8_segs(*a, segs, B, H, out["Q8"], out["K8"], out["VT8"], in_f16=fm == "fp8_f16in")
        elif fm == "f32":
            ops.qkv_prep_f32_segs(out["QKV"], self.q_col, self.k_col, segs, B, H)
        else:
            D = self.D
            ops.qkv_prep_split_segs(*a, segs, B, H, out["QK2"], 8, 2 * D + 24, D + 8, out["VT2"])
        torch.cuda.synchronize()

    def expected_vt(self, i, kind):
        """the V^T image of segment i over its slots [0, pad64(L)): bf16 bits / e4m3 codes / (hi, lo) bf16 pair"""
        L = self.lens[i]
        P = pad64(L)
        v = self.v_in(i)
        vp = torch.zeros(self.B, P, self.H, 128, dtype=v.dtype, device=DEV)
        vp[:, :L] = v
        j = torch.arange(P, device=DEV)
        if kind == "bf16":
            return vp.to(torch.bfloat16)[:, vt_key(j)].permute(0, 2, 3, 1)
        if kind == "e4m3":
            from loongx_amd.ops import FP8_V_SCALE
            e = (vp.to(torch.bfloat16).float() * FP8_V_SCALE).clamp(-448, 448).to(E4M3).view(torch.uint8)
            return e[:, vt8_key(j)].permute(0, 2, 3, 1)
        hi = vp.to(torch.bfloat16)
        lo = (vp - hi.float()).to(torch.bfloat16)
        return hi[:, vt_key(j)].permute(0, 2, 3, 1), lo[:, vt_key(j)].permute(0, 2, 3, 1)


@pytest.mark.parametrize("cfg", list(QK_CFG))
@pytest.mark.parametrize("form", QK_FORMS)
def test_qkv_prep_rows(ops, form, cfg):
    c = QkCase(ops, form, cfg)
    arm = f"qk {form} {cfg}"
    out = c.new_outputs()
    c.launch(ops, out)
    D, H, B = c.D, c.H, c.B
    ns = len(c.segs)
    qkv_in = torch.zeros(out["QKV"].shape, dtype=torch.bool, device=DEV)       # columns / rows the launch may change in place
    vt_in = None
    for i in range(ns):
        r0, L, vt0 = c.segs[i][:3]
        rows = slice(r0, r0 + B * L)
        for which, col in (("q", c.q_col), ("k", c.k_col)):
            y, E = c.qk_ref(i, which)
            if form in ("single", "fast", "general", "f16in"):
                got = out["QKV"][rows, col:col + D].view(torch.bfloat16).view(B, L, H, 128)      # (bf16 written over fp16 in f16in)
                nb = check_rounding(f"{arm} seg{i} {which}", got, y, E, "bf16")
                report(arm, which, row_worst(got, y), BOUND["bf16"], nb)
                qkv_in[rows, col:col + D] = True
            elif form.startswith("fp8"):
                from loongx_amd.ops import FP8_Q_SCALE, FP8_K_SCALE
                s = FP8_Q_SCALE if which == "q" else FP8_K_SCALE
                got = out["Q8" if which == "q" else "K8"][rows, :D].view(B, L, H, 128)
                nb = check_rounding(f"{arm} seg{i} {which}8", got, y * s, (E + U32 * y.abs()) * s, "e4m3")
                report(arm, which + "8", row_worst(deq8(got), (y * s).clamp(-448, 448)), BOUND["e4m3"], nb)
            elif form == "f32":
                got = out["QKV"][rows, col:col + D].view(B, L, H, 128)
                report(arm, which, row_worst(got, y), BOUND["f32"])
                qkv_in[rows, col:col + D] = True
            else:
                col2 = 8 if which == "q" else 2 * D + 24
                hi = out["QK2"][rows, col2:col2 + D].view(B, L, H, 128)
                lo = out["QK2"][rows, col2 + D + 8:col2 + 2 * D + 8].view(B, L, H, 128)
                nb = check_rounding(f"{arm} seg{i} {which} hi", hi, y, E, "bf16")
                check_rounding(f"{arm} seg{i} {which} lo", lo, y - hi.double(), E, "bf16", frac=1.0)
                report(arm, which + " pair", row_worst(hi.double() + lo.double(), y), BOUND["split_qk"], nb)
    # ---- V^T images, slot by slot; everything outside [vt_pos0, vt_pos0 + pad64(L)) keeps the sentinel
    if "VT" in out or "VT8" in out or "VT2" in out:
        key = "VT" if "VT" in out else ("VT8" if "VT8" in out else "VT2")
        vt = out[key]
        vt_in = torch.zeros(vt.shape, dtype=torch.bool, device=DEV)
        for i in range(ns):
            L, vt0 = c.lens[i], c.vt0[i]
            P = pad64(L)
            if key == "VT":
                got, exp = vt[..., vt0:vt0 + P], c.expected_vt(i, "bf16")
                assert torch.equal(bits(got), bits(exp)), f"{arm}: V^T of segment {i} is not the interleaved V ({int((bits(got) != bits(exp)).sum())} slots)"
            elif key == "VT8":
                got, exp = vt[..., vt0:vt0 + P], c.expected_vt(i, "e4m3")
                assert torch.equal(got, exp), f"{arm}: VT8 of segment {i} is not e4m3(bf16(v) * v_scale) in vt8_key order"
            else:
                hi, lo = c.expected_vt(i, "pair")
                assert torch.equal(bits(vt[0, ..., vt0:vt0 + P]), bits(hi)) and torch.equal(bits(vt[1, ..., vt0:vt0 + P]), bits(lo)), \
                    f"{arm}: VT2 of segment {i} is not the (hi, lo) pair of V"
            j = torch.arange(P, device=DEV)
            pad_slots = vt0 + j[(vt8_key(j) if key == "VT8" else vt_key(j)) >= L]     # the slots that hold keys [L, pad64(L))
            pz = vt[..., pad_slots]
            assert bool((pz.float() == 0).all()) if key != "VT8" else bool((pz == 0).all()), f"{arm}: V^T padding slots of segment {i} not zero"
            vt_in[..., vt0:vt0 + P] = True
        check_footprint(f"{arm} {key}", vt, vt_in)
    # ---- in place: nothing but q / k of the launched rows changes (V stays, in fp16 in the f16in form); fp8 / split leave QKV alone
    check_footprint(f"{arm} QKV", out["QKV"], qkv_in, init=c.buf)
    if form.startswith("fp8"):
        for k in ("Q8", "K8"):
            m = torch.zeros(out[k].shape, dtype=torch.bool, device=DEV)
            for i in range(ns):
                m[c.segs[i][0]:c.segs[i][0] + B * c.lens[i], :D] = True
            check_footprint(f"{arm} {k}", out[k], m)
    if form == "split":
        m = torch.zeros(out["QK2"].shape, dtype=torch.bool, device=DEV)
        for i in range(ns):
            rows = slice(c.segs[i][0], c.segs[i][0] + B * c.lens[i])
            for c0 in (8, D + 16, 2 * D + 24, 3 * D + 32):
                m[rows, c0:c0 + D] = True
        check_footprint(f"{arm} QK2", out["QK2"], m)
    # ---- determinism (from a fresh copy of the inputs: the bf16 / f32 forms work in place)
    again = c.new_outputs()
    c.launch(ops, again)
    for k in out:
        assert torch.equal(bits(out[k]), bits(again[k])), f"{arm}: {k} differs between two identical launches"
    # ---- row-position invariance: segment 0 alone
    if ns == 3:
        alone = c.new_outputs()
        c.launch(ops, alone, seg_idx=[0])
        r0, L, vt0 = c.segs[0][:3]
        rows = slice(r0, r0 + B * L)
        for k in out:
            if k.startswith("VT"):
                assert torch.equal(bits(out[k][..., vt0:vt0 + pad64(L)]), bits(alone[k][..., vt0:vt0 + pad64(L)])), f"{arm}: {k} depends on the launch"
            else:
                assert torch.equal(bits(out[k][rows]), bits(alone[k][rows])), f"{arm}: {k} rows of segment 0 depend on the launch"
    # ---- cross-form identities
    if form == "general":         # segment 0 has norm weights and tables: the FAST body on the same segment gives the same bits
        f = QkCase(ops, "fast", cfg)
        fo = f.new_outputs()
        f.launch(ops, fo, seg_idx=[0])
        r0, L, vt0 = c.segs[0][:3]
        for col in (c.q_col, c.k_col):
            assert torch.equal(bits(out["QKV"][r0:r0 + B * L, col:col + D]), bits(fo["QKV"][r0:r0 + B * L, col:col + D])), \
                f"{arm}: the general and the FAST body disagree on a complete segment"
        assert torch.equal(bits(out["VT"][..., vt0:vt0 + pad64(L)]), bits(fo["VT"][..., vt0:vt0 + pad64(L)]))
    if form == "f16in":           # inputs exact in both formats: bit-equal to the bf16-input general body
        g = QkCase(ops, "general", cfg)
        go = g.new_outputs()
        g.launch(ops, go)
        assert torch.equal(bits(out["VT"]), bits(go["VT"])), f"{arm}: V^T differs from the bf16-input launch"
        for i in range(ns):
            r0, L = c.segs[i][:2]
            for col in (c.q_col, c.k_col):
                assert torch.equal(bits(out["QKV"][r0:r0 + B * L, col:col + D]), bits(go["QKV"][r0:r0 + B * L, col:col + D])), \
                    f"{arm}: q / k of segment {i} differ from the bf16-input launch"
            v = out["QKV"][r0:r0 + B * L, c.v_col:c.v_col + D]
            assert v.dtype == torch.float16 and torch.equal(bits(v), bits(c.buf[r0:r0 + B * L, c.v_col:c.v_col + D]))


# ================================================================================================ LoRA down-projection
# (M, K, n_split, R, ldt): K / 256 steps per wave 1, 4, 5, 8, 9, 16, 17, 60; n_split 3, 4, 16 with empty slabs (K=256 / 16: slabs 8..15,
# K=96 / 4: slab 3, K=1280 / 16: slabs 14, 15); ldt = R, 16, 17 (scalar stores when ldt % 4 or R % 4)
LORA_CASES = [(1, 256, 1, 1, 1), (15, 1024, 1, 3, 16), (17, 1280, 1, 4, 4), (300, 2048, 1, 5, 17), (17, 2304, 3, 16, 16),
              (15, 4096, 4, 16, 17), (300, 4352, 1, 4, 16), (1, 15360, 1, 16, 17), (17, 256, 16, 5, 5), (300, 96, 4, 3, 17),
              (15, 1280, 16, 16, 16)]


def _lora_ids():
    return [f"M{m}-K{k}-s{s}-R{r}-ldt{l}" for m, k, s, r, l in LORA_CASES]


@pytest.mark.parametrize("entry", ["bf16", "f16", "fp8", "terms"])
@pytest.mark.parametrize("M,K,n_split,R,ldt", LORA_CASES, ids=_lora_ids())
def test_lora_down_slabs(ops, entry, M, K, n_split, R, ldt):
    arm = f"lora_down {entry}"
    if entry == "terms":
        n_split = min(max(n_split, 1), 4)          # one slab per term
    stride = ((M - 1) * ldt + R + 8 + 3) // 4 * 4      # sentinel elements between slabs
    buf = sentinel((n_split * stride + 2 * 16,), torch.float32)
    T = buf[16:].as_strided((M, R), (ldt, 1))
    ks = ((K // 32 + n_split - 1) // n_split) * 32
    descale = 1.0
    if entry == "terms":
        Xs = [randn(M, K + 40, seed=s + 1, dtype=torch.bfloat16)[:, 8:8 + K] for s in range(n_split)]
        As = [randn(R, K, seed=s + 20, scale=K ** -0.5, dtype=torch.bfloat16) for s in range(n_split)]
        ops.lora_down_terms(list(zip(Xs, As)), T, stride)
        slabs = [(Xs[s].double() @ As[s].double().T, Xs[s].double().abs() @ As[s].double().abs().T) for s in range(n_split)]
    else:
        X = randn(M, K + 24, seed=1)[:, :K]
        A = randn(R, K, seed=2, scale=K ** -0.5, dtype=torch.bfloat16)
        if entry == "fp8":
            descale = 1.0 / 16.0
            X8 = (X * 16.0).clamp(-448, 448).to(E4M3).view(torch.uint8)
            ops.lora_down_fp8(X8, descale, A, T, n_split=n_split, split_stride=stride)
            X64 = deq8(X8) * descale
        else:
            dt = torch.float16 if entry == "f16" else torch.bfloat16
            Xb = torch.empty(M, K + 24, dtype=dt, device=DEV)[:, :K]
            Xb.copy_(X.to(dt))
            A = A.to(dt)
            ops.lora_down(Xb, A, T, n_split=n_split, split_stride=stride)
            X64 = Xb.double()
        A64 = A.double()
        slabs = []
        for s in range(n_split):
            k0, k1 = min(K, s * ks), min(K, (s + 1) * ks)
            slabs.append((X64[:, k0:k1] @ A64[:, k0:k1].T, X64[:, k0:k1].abs() @ A64[:, k0:k1].abs().T))
    torch.cuda.synchronize()
    inside = torch.zeros(buf.shape, dtype=torch.bool, device=DEV)
    tot, tot_abs, worst = 0, 0, 0.0
    for s in range(n_split):
        Ts = buf[16 + s * stride:].as_strided((M, R), (ldt, 1))
        ref, ab = slabs[s]
        if entry != "terms" and s * ks >= K:
            assert bool((Ts == 0).all()), f"{arm}: slab {s} has an empty K range and must be written as zeros"
        else:
            worst = max(worst, row_worst(Ts, ref, ab))
        inside[16 + s * stride:].as_strided((M, R), (ldt, 1)).fill_(True)
        tot, tot_abs = tot + Ts.double(), tot_abs + ab
    report(arm, "slab", worst, BOUND["lora"])
    report(arm, "sum", row_worst(tot, sum(r for r, _ in slabs), tot_abs), BOUND["lora"])
    check_footprint(arm, buf, inside)


# ================================================================================================ small producers
def rope_ref(ids, axes, theta=10000.0):
    """float64 restatement of FluxPosEmbed's tables: freq_j = 1 / theta^(2j / d), angle = id * freq, each value twice (pair layout)"""
    cs, ss = [], []
    for a, d in enumerate(axes):
        f = 1.0 / theta ** (torch.arange(0, d, 2, dtype=torch.float64, device=ids.device) / d)
        ang = ids[:, a].double()[:, None] * f
        cs.append(ang.cos().repeat_interleave(2, 1))
        ss.append(ang.sin().repeat_interleave(2, 1))
    return torch.cat(cs, 1), torch.cat(ss, 1)


@pytest.mark.parametrize("axes", [(16, 56, 56), (20, 54, 54)])
@pytest.mark.parametrize("L", [1, 77, 4096])
def test_rope_table_against_fp64(ops, L, axes):
    hw = 64                                    # 1024 x 1024 image: 64 x 64 packed latent tokens
    n_img = min(L, hw * hw)
    ids = torch.zeros(L, 3, device=DEV)
    t = torch.arange(n_img, device=DEV)
    ids[:n_img, 1] = (t // hw).float()
    ids[:n_img, 2] = (t % hw).float() - (hw if L == 77 else 0)       # negative ids: the condition stream's shifted grid
    ids[0, 0] = 3.0
    tot = sum(axes)
    cb, sb = sentinel((L + 2, tot), torch.float32), sentinel((L + 2, tot), torch.float32)
    ops.rope_table(ids, axes=axes, out=(cb[:L], sb[:L]))
    torch.cuda.synchronize()
    rc, rs = rope_ref(ids, axes)
    def code32(t):
        b = t.view(torch.int32).long()
        return torch.where(b < 0, -(b & 0x7FFFFFFF), b)
    for name, got, ref in (("cos", cb[:L], rc), ("sin", sb[:L], rs)):
        ulps = (code32(got) - code32(ref.float())).abs()
        assert bool((ulps <= 1).all()), f"rope_table {axes} L={L} {name}: {int((ulps > 1).sum())} values more than 1 fp32 ulp from float64"
    m = torch.zeros(cb.shape, dtype=torch.bool, device=DEV)
    m[:L] = True
    check_footprint("rope cos", cb, m)
    check_footprint("rope sin", sb, m)


@pytest.mark.parametrize("M", [1, 4, 7, 16])
@pytest.mark.parametrize("N,K", [(5, 8), (18, 520), (515, 3080), (1027, 520)])
def test_linear_skinny_edges(ops, M, N, K):
    X = randn(M, K + 12, seed=1)[:, :K]
    W = randn(N, K + 8, seed=2, scale=K ** -0.5, dtype=torch.bfloat16)[:, :K]
    b = randn(N, seed=3)
    x64, w64, b64 = X.double(), W.double(), b.double()
    silu = lambda v: v / (1 + torch.exp(-v))          # noqa: E731
    for act_in, act_out, acc in ((1, 0, False), (0, 1, True), (0, 0, False)):
        Yb = sentinel((M + 2, N + 5), torch.float32)
        Y = Yb[1:M + 1, :N]
        y0 = randn(M, N, seed=4)
        if acc:
            Y.copy_(y0)
        init = Yb.clone()
        ops.linear_skinny(X, W, b if act_out == 0 else None, Y, act_in=act_in, act_out=act_out, accumulate=acc)
        torch.cuda.synchronize()
        xa = silu(x64) if act_in else x64
        s = xa @ w64.T + (b64 if act_out == 0 else 0)
        ab = xa.abs() @ w64.abs().T + (b64.abs() if act_out == 0 else 0)
        ref = (silu(s) if act_out else s) + (y0.double() if acc else 0)
        report("linear_skinny", f"act{act_in}{act_out}{int(acc)}", row_worst(Y, ref, ab + (y0.double().abs() if acc else 0)), BOUND["skinny"])
        m = torch.zeros(Yb.shape, dtype=torch.bool, device=DEV)
        m[1:M + 1, :N] = True
        check_footprint(f"linear_skinny M{M} N{N} K{K}", Yb, m, init=init if acc else None)


def test_grid_stride_converters_past_their_grid_caps(ops):
    """lx_euler_step (grid cap 2048 x 256), lx_convert (4096 x 256), lx_convert_fp8 and lx_split_bf16 (4096 x 256 groups): sizes that make
    every grid-stride loop go round more than once; the 2-D ones on strided rows; each output inside a sentinel tail."""
    n = 2048 * 256 * 2 + 777
    x = randn(n, seed=1)
    for vdt in (torch.bfloat16, torch.float32):
        v = randn(n, seed=2, dtype=vdt)
        xb = sentinel((n + 64,), torch.float32)
        xb[:n] = x
        ops.euler_step(xb[:n], v, -0.0625)
        torch.cuda.synchronize()
        ref = (x.double() - 0.0625 * v.double()).float()          # fmaf: one rounding of the exact x + ds v (ds a power of two)
        assert torch.equal(bits(xb[:n]), bits(ref)), f"euler_step {vdt}: {int((xb[:n] != ref).sum())} elements differ"
        assert bool((bits(xb[n:]) == bits(sentinel((1,), torch.float32))[0]).all()), "euler_step wrote past n"
    n = 4096 * 256 * 2 + 333
    src32 = randn(n, seed=3, scale=3e4)                 # |x| > 65504 saturates in the fp16 image
    src16 = randn(n, seed=4, dtype=torch.bfloat16)
    for dst_dt, src, exp in ((torch.bfloat16, src32, src32.to(torch.bfloat16)),
                             (torch.float16, src32, src32.clamp(-65504, 65504).to(torch.float16)),
                             (torch.float32, src16, src16.float()),
                             (torch.float32, src32, src32)):
        db = sentinel((n + 64,), dst_dt)
        ops.convert(db[:n], src)
        torch.cuda.synchronize()
        assert torch.equal(bits(db[:n]), bits(exp)), f"convert {src.dtype} -> {dst_dt}: {int((bits(db[:n]) != bits(exp)).sum())} elements differ"
        assert bool((bits(db[n:]) == bits(sentinel((1,), dst_dt))[0]).all()), f"convert -> {dst_dt} wrote past n"
    M, K = 1100, 8192
    for sdt in (torch.float32, torch.bfloat16):
        src = randn(M, K + 8, seed=5, scale=40.0, dtype=sdt)[:, :K]
        db = sentinel((M + 1, K + 16), torch.uint8)
        ops.convert_fp8(src, db[:M, :K], 4.0)
        torch.cuda.synchronize()
        exp = (src.float() * 4.0).clamp(-448, 448).to(E4M3).view(torch.uint8)
        assert torch.equal(db[:M, :K], exp), f"convert_fp8 {sdt}: {int((db[:M, :K] != exp).sum())} bytes differ"
        m = torch.zeros(db.shape, dtype=torch.bool, device=DEV)
        m[:M, :K] = True
        check_footprint(f"convert_fp8 {sdt}", db, m)
    M, K = 600, 7200
    src = randn(M, K + 4, seed=6)[:, :K]
    db = sentinel((M + 1, 2 * K + 16), torch.bfloat16)
    ops.split_bf16(src, db[:M], K + 8)
    torch.cuda.synchronize()
    hi = src.to(torch.bfloat16)
    lo = (src - hi.float()).to(torch.bfloat16)
    assert torch.equal(bits(db[:M, :K]), bits(hi)) and torch.equal(bits(db[:M, K + 8:2 * K + 8]), bits(lo)), "split_bf16: pair differs"
    m = torch.zeros(db.shape, dtype=torch.bool, device=DEV)
    m[:M, :K] = True
    m[:M, K + 8:2 * K + 8] = True
    check_footprint("split_bf16", db, m)
