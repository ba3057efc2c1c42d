"""Named LoRA adapters on the host side: the registry of PackedWeights (install_lora(adapter_name=...), set_active_adapters,
delete_adapters), the stacked image the engine reads, what lx_lora_scale_rows refuses before it launches, and the broadcast of a model
with two adapters. The test adapters are slices of tests/test_lora_wide_gpu.rank_model's sets: rows lo:hi of every down matrix and the
same columns of every up matrix, so that adapters [0:4] + [4:16] stacked ARE the rank-16 set."""
import copy
import ctypes as C
import os
import socket
import sys

import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

from tests.test_lora_rank_cpu import _cfg, _lora_only, with_rank
from tests.test_lora_wide_gpu import _inputs, oracle_out, rank_model

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def lora_slice(sd, lo, hi):
    """LoRA-only state dict (install_lora's input) of the adapter made of rank rows lo:hi of every module of `sd`."""
    return {k: (v[lo:hi] if ".lora_A." in k else v[:, lo:hi]).contiguous() for k, v in _lora_only(sd).items()}


def base_sd(sd):
    """The state dict without any adapter (plain Linear names)."""
    return {k.replace(".base_layer.", "."): v for k, v in sd.items() if ".lora_" not in k}


def packed_with(r, parts, precise=False, device="cpu"):
    """The tiny model packed without adapters, then the named slices `parts` = [(name, lo, hi), ...] of the rank-r set installed."""
    from loongx_amd.flux.weights import install_lora, pack_state_dict
    tr, sd, _ = rank_model(r)
    pw = pack_state_dict(base_sd(sd), _cfg(tr), device, precise=precise)
    for name, lo, hi in parts:
        assert install_lora(pw, lora_slice(sd, lo, hi), adapter_name=name) == 25
    return pw


def split_oracle(r, parts, scalings):
    """A copy of the rank-r oracle model whose every LoraLinear carries the adapters `parts` = [(name, lo, hi), ...] (slices of its
    "default" adapter) with `scalings` = {name: s}, all active, in this order -- the unmodified oracle.flux_modules.LoraLinear loops
    over active_adapters with its scaling dict."""
    from oracle import flux_modules as fm
    tr = copy.deepcopy(rank_model(r)[0])
    for m in tr.modules():
        if isinstance(m, fm.LoraLinear):
            A, B = m.lora_A["default"].weight.detach(), m.lora_B["default"].weight.detach()
            for name, lo, hi in parts:
                m.lora_A[name] = torch.nn.Linear(m.in_features, hi - lo, bias=False)
                m.lora_B[name] = torch.nn.Linear(hi - lo, m.out_features, bias=False)
                m.lora_A[name].weight.data.copy_(A[lo:hi])
                m.lora_B[name].weight.data.copy_(B[:, lo:hi])
                m.scaling[name] = float(scalings[name]) * m.scaling["default"]
            m.active_adapters = [name for name, _, _ in parts]
    return tr.eval()


def split_oracle_out(r, parts, scalings, mc):
    from oracle import flux_ref as fr
    kw, cond, cids = _inputs()
    with torch.no_grad():
        return fr.tranformer_forward(split_oracle(r, parts, scalings), cond, cids, None, dict(mc), **kw)[0]


AB = [("a", 0, 4), ("b", 4, 16)]


def _lora_tensors(pw):
    out = {k: v for k, v in pw.t.items() if k.startswith("mod.lora_")}
    for k, lo in pw.lora.items():
        out[k + ".down"], out[k + ".up"] = lo.down, lo.up
        if lo.down_lo is not None:
            out[k + ".down_lo"] = lo.down_lo
    return out


# ---------------------------------------------------------------------------------------------------------------- stacking
@pytest.mark.parametrize("r,parts,precise", [(16, AB, False), (4, [("a", 0, 2), ("b", 2, 4)], True)])
def test_stacked_adapters_are_the_whole_set(r, parts, precise):
    from loongx_amd.flux.weights import active_adapters, pack_state_dict, set_active_adapters
    tr, sd, _ = rank_model(r)
    pw = packed_with(r, parts, precise)
    assert active_adapters(pw) == ["a"] and pw.cfg.lora_r == parts[0][2]          # the first one loaded became active, the second did not
    set_active_adapters(pw, ["a", "b"])
    ref = pack_state_dict(sd, _cfg(tr), "cpu", precise=precise)
    got, want = _lora_tensors(pw), _lora_tensors(ref)
    assert set(got) == set(want) and set(pw.lora) == set(ref.lora) and len(ref.lora) > 8
    for k in want:
        assert torch.equal(got[k], want[k]), k
    assert pw.cfg.lora_r == r
    if precise:
        assert any(k.endswith(".down_lo") for k in got) and "mod.lora_down_lo" in got
    # the other order stacks the other way round
    set_active_adapters(pw, ["b", "a"])
    cut = parts[1][2] - parts[1][1]
    assert torch.equal(pw.lora["x_embedder"].down[:cut], ref.lora["x_embedder"].down[parts[1][1]:])
    assert torch.equal(pw.lora["d0.out"].up[:, cut:], ref.lora["d0.out"].up[:, :parts[0][2]])


def test_an_adapter_without_a_module_contributes_zeros():
    from loongx_amd.flux.weights import install_lora, pack_state_dict, set_active_adapters
    tr, sd, _ = rank_model(16)
    pw = pack_state_dict(base_sd(sd), _cfg(tr), "cpu")
    a = lora_slice(sd, 0, 4)
    b = {k: v for k, v in lora_slice(sd, 4, 16).items() if ".x_embedder." not in k and "norm" not in k}     # no x_embedder, no modulation adapters
    install_lora(pw, a, adapter_name="a")
    install_lora(pw, b, adapter_name="b")
    set_active_adapters(pw, ["a", "b"])
    ref = pack_state_dict(sd, _cfg(tr), "cpu")
    xe = pw.lora["x_embedder"]
    assert xe.down.shape == (16, 64) and torch.equal(xe.down[:4], ref.lora["x_embedder"].down[:4]) and not bool(xe.down[4:].any())
    assert torch.equal(xe.up[:, :4], ref.lora["x_embedder"].up[:, :4]) and not bool(xe.up[:, 4:].any())
    md = pw.t["mod.lora_down"].view(4, 16, 256)
    assert torch.equal(md[:, :4], ref.t["mod.lora_down"].view(4, 16, 256)[:, :4]) and not bool(md[:, 4:].any())
    assert not bool(pw.t["mod.lora_up.3"][:, 4:].any()) and torch.equal(pw.lora["s1.fused"].down, ref.lora["s1.fused"].down)


# ---------------------------------------------------------------------------------------------------------------- registry
def test_registry_operations():
    from loongx_amd.flux.weights import (active_adapters, delete_adapters, install_lora, list_adapters, pack_state_dict,
                                         set_active_adapters)
    tr, sd, _ = rank_model(16)
    pw = pack_state_dict(rank_model(4)[1], _cfg(tr), "cpu")              # packed WITH its rank-4 adapter: adopted as "default"
    down0, v0 = pw.lora["d0.qkv"].down, pw.lora_version
    assert list_adapters(pw) == ["default"] and active_adapters(pw) == ["default"]
    assert pw.adapters["default"].lora["d0.qkv"].down is down0 and pw.lora_version == v0          # shared storage, nothing restacked
    install_lora(pw, lora_slice(sd, 0, 4), adapter_name="a")
    install_lora(pw, lora_slice(sd, 4, 16), adapter_name="b")
    assert list_adapters(pw) == ["default", "a", "b"] and active_adapters(pw) == ["default"]
    assert pw.lora["d0.qkv"].down is down0 and pw.lora_version == v0 and pw.cfg.lora_r == 4      # loading beside an active set changes nothing
    set_active_adapters(pw, "b")
    assert active_adapters(pw) == ["b"] and pw.cfg.lora_r == 12 and pw.lora_version == v0 + 1
    assert pw.lora["d0.qkv"].down.shape == (36, 256) and pw.t["mod.lora_down"].shape == (48, 256)
    only_b = packed_with(16, [("b", 4, 16)])
    for k, v in _lora_tensors(only_b).items():
        assert torch.equal(_lora_tensors(pw)[k], v), k
    set_active_adapters(pw, ["b", "a"])
    assert active_adapters(pw) == ["b", "a"] and pw.cfg.lora_r == 16
    # replace an ACTIVE entry: the stacked image follows
    install_lora(pw, lora_slice(sd, 0, 2), adapter_name="a")
    assert pw.adapters["a"].rank == 2 and pw.cfg.lora_r == 14 and pw.lora["x_embedder"].down.shape[0] == 14
    # delete an active and an inactive one
    delete_adapters(pw, ["b", "default"])
    assert list_adapters(pw) == ["a"] and active_adapters(pw) == ["a"] and pw.cfg.lora_r == 2
    delete_adapters(pw, "a")
    assert list_adapters(pw) == [] and active_adapters(pw) == [] and not pw.lora and "mod.lora_down" not in pw.t
    # with nothing active, the next named adapter becomes active
    install_lora(pw, lora_slice(sd, 4, 16), adapter_name="b")
    assert active_adapters(pw) == ["b"] and pw.cfg.lora_r == 12
    # adapter_name=None still replaces everything
    install_lora(pw, lora_slice(sd, 0, 4), adapter_name="a")
    assert install_lora(pw, _lora_only(rank_model(4)[1])) == 25
    assert list_adapters(pw) == ["default"] and active_adapters(pw) == ["default"] and pw.cfg.lora_r == 4
    fresh = pack_state_dict(rank_model(4)[1], _cfg(tr), "cpu")
    for k, v in _lora_tensors(fresh).items():
        assert torch.equal(_lora_tensors(pw)[k], v), k


def _state(pw):
    return (pw.lora_version, pw.cfg.lora_r, list(pw.active), list(pw.adapters), {k: id(v) for k, v in _lora_tensors(pw).items()})


def test_refusals_leave_the_model_as_it_was():
    from loongx_amd.flux.weights import install_lora, set_active_adapters
    tr, sd, _ = rank_model(16)
    pw = packed_with(16, AB)
    set_active_adapters(pw, ["a", "b"])
    before = _state(pw)
    with pytest.raises(ValueError, match=r"'nope'.*\['a', 'b'\]"):
        set_active_adapters(pw, ["a", "nope"])
    assert _state(pw) == before
    # 64 + 2: past the wide limit; the message names the adapters and the total
    sd64 = rank_model(64)[1]
    install_lora(pw, lora_slice(sd64, 0, 64), adapter_name="wide")
    install_lora(pw, lora_slice(sd, 0, 2), adapter_name="two")
    before = _state(pw)
    with pytest.raises(ValueError, match=r"'wide' \(rank 64\).*'two' \(rank 2\).*66.*64"):
        set_active_adapters(pw, ["wide", "two"])
    assert _state(pw) == before
    # 3 + 4 = 7: odd and above the narrow limit (4 modules x 7 > 16)
    install_lora(pw, lora_slice(sd, 0, 3), adapter_name="three")
    before = _state(pw)
    with pytest.raises(ValueError, match=r"'three' \(rank 3\).*'a' \(rank 4\).*rank 7"):
        set_active_adapters(pw, ["three", "a"])
    assert _state(pw) == before
    # one adapter, one rank
    mixed = _lora_only(with_rank(rank_model(4)[1], 8, only="single_transformer_blocks.1.proj_out"))
    with pytest.raises(ValueError, match="share one rank"):
        install_lora(pw, mixed, adapter_name="mixed")
    assert _state(pw) == before
    # replacing an ACTIVE adapter by one that no longer fits keeps the old entry
    with pytest.raises(ValueError, match=r"'a' \(rank 62\).*'b' \(rank 12\).*rank 74"):
        install_lora(pw, lora_slice(sd64, 0, 62), adapter_name="a")
    assert _state(pw) == before and pw.adapters["a"].rank == 4


def test_precise_weights_keep_the_narrow_limit_for_the_stack():
    from loongx_amd.flux.weights import install_lora, pack_state_dict, set_active_adapters
    tr, sd, _ = rank_model(16)
    pw = pack_state_dict(base_sd(sd), _cfg(tr), "cpu", precise=True)
    install_lora(pw, lora_slice(sd, 0, 4), adapter_name="a")
    install_lora(pw, lora_slice(sd, 4, 8), adapter_name="b")
    before = _state(pw)
    with pytest.raises(ValueError, match=r"'a' \(rank 4\).*'b' \(rank 4\).*rank 8.*precise"):
        set_active_adapters(pw, ["a", "b"])
    assert _state(pw) == before
    set_active_adapters(pw, "b")                                         # each alone fits
    assert pw.cfg.lora_r == 4


# ---------------------------------------------------------------------------------------------------------------- the oracle side
def test_the_split_oracle_is_the_rank16_oracle():
    from tests.helpers import relerr
    assert relerr(split_oracle_out(16, AB, {"a": 1.0, "b": 1.0}, {}), oracle_out(16, {})) < 1e-6
    assert relerr(split_oracle_out(16, AB, {"a": 0.5, "b": 2.0}, {}), oracle_out(16, {})) > 1e-3


# ---------------------------------------------------------------------------------------------------------------- host validation
A16 = 0x10000          # 16-byte aligned, never dereferenced


def _segs(rows):
    from loongx_amd import _lib
    arr = (_lib.RowScaleSeg * max(len(rows), 1))()
    for i, (row0, n_rows, rpb) in enumerate(rows):
        arr[i].row0, arr[i].n_rows, arr[i].rows_per_batch = row0, n_rows, rpb
    return arr


SCALE_DEFAULTS = dict(T=A16, ldt=16, R=16, n_slab=1, slab_stride=0, rows=[(0, 8, 4), (8, 8, 2)], seg=True, n_seg=2, W=A16, w_ld=16,
                      n_batches=2, period=16)


def _scale_call(**over):
    from loongx_amd import _lib
    a = dict(SCALE_DEFAULTS, **over)
    return _lib.lib.lx_lora_scale_rows(a["T"], a["ldt"], a["R"], a["n_slab"], a["slab_stride"], _segs(a["rows"]) if a["seg"] else None,
                                       a["n_seg"], a["W"], a["w_ld"], a["n_batches"], a["period"], None)


@pytest.mark.parametrize("over,text", [
    (dict(T=None), "lx_lora_scale_rows: NULL operand"),
    (dict(W=None), "lx_lora_scale_rows: NULL operand"),
    (dict(seg=False), "lx_lora_scale_rows: NULL operand"),
    (dict(R=0), "lx_lora_scale_rows: R=0 must be in [1,16384]"),
    (dict(R=16385, ldt=16400), "lx_lora_scale_rows: R=16385 must be in [1,16384]"),
    (dict(period=0), "lx_lora_scale_rows: period=0, n_batches=2 and n_slab=1 must be >= 1"),
    (dict(n_batches=0), "lx_lora_scale_rows: period=16, n_batches=0 and n_slab=1 must be >= 1"),
    (dict(n_slab=0), "lx_lora_scale_rows: period=16, n_batches=2 and n_slab=0 must be >= 1"),
    (dict(n_seg=0), "lx_lora_scale_rows: 1..3 segments"),
    (dict(n_seg=4), "lx_lora_scale_rows: 1..3 segments"),
    (dict(w_ld=15), "lx_lora_scale_rows: w_ld=15 must be >= min(period, R)"),
    (dict(period=64, w_ld=15), "lx_lora_scale_rows: w_ld=15 must be >= min(period, R)"),
    (dict(period=4, R=16, w_ld=3), "lx_lora_scale_rows: w_ld=3 must be >= min(period, R)"),
    (dict(ldt=15), "lx_lora_scale_rows: ldt=15 must be >= R=16"),
    (dict(n_slab=2, slab_stride=0), "lx_lora_scale_rows: bad slab_stride=0"),
    (dict(T=A16 + 2), "lx_lora_scale_rows: operands must be 4-byte aligned"),
    (dict(rows=[(0, 8, 4), (8, 8, 0)]), "lx_lora_scale_rows: bad segment 1"),
    (dict(rows=[(0, 8, 0), (8, 8, 2)]), "lx_lora_scale_rows: bad segment 0"),
    (dict(rows=[(0, 8, 4), (8, 0, 2)]), "lx_lora_scale_rows: bad segment 1"),
    (dict(rows=[(-1, 8, 4), (8, 8, 2)]), "lx_lora_scale_rows: bad segment 0"),
])
def test_scale_rows_refusals(over, text):
    """Every call is refused before anything is launched (fake, aligned addresses: nothing dereferences them)."""
    from loongx_amd import _lib
    assert _scale_call(**over) == -1                     # LX_ERR_INVALID
    assert _lib.lib.lx_last_error().decode() == text


def test_abi_is_additive():
    from loongx_amd import _lib
    assert "lx_lora_scale_rows" in _lib.EXPORTS and _lib.lib.lx_version() == 404
    assert C.sizeof(_lib.RowScaleSeg) == 16


# ---------------------------------------------------------------------------------------------------------------- engine bookkeeping
def test_engine_adapter_weight_bookkeeping_without_a_gpu():
    """set_adapter_weights / set_adapters: what they accept, what they drop and that a refused call changes nothing (no kernel involved)."""
    from loongx_amd.flux.engine import DiTEngine
    pw = packed_with(16, AB)
    eng = DiTEngine(pw, "cpu")
    eng.graphs, eng.cond_ready, eng.sched = {"k": 1}, True, ("s",)
    eng.set_adapter_weights({"a": 1.0})                   # recorded, and the cached state goes: the weights are part of it
    assert eng.adapter_weights == {"a": 1.0} and eng.graphs == {} and not eng.cond_ready and eng.sched is None
    eng.graphs, eng.cond_ready = {"k": 1}, True
    eng.set_adapter_weights({"a": 1.0})                   # the same again: nothing to drop
    assert eng.graphs == {"k": 1} and eng.cond_ready
    eng.set_adapter_weights({"a": torch.tensor([1.0, 0.0]), "b": [0.0, 1.0]})
    assert eng.adapter_weights == {"a": (1.0, 0.0), "b": (0.0, 1.0)} and eng.graphs == {} and not eng.cond_ready
    key = eng.adapter_weights_key()
    eng.graphs, eng.cond_ready = {"k": 1}, True
    with pytest.raises(ValueError, match=r"'c'.*\['a', 'b'\]"):
        eng.set_adapter_weights({"c": 2.0})
    with pytest.raises(ValueError, match=r"'c'.*\['a', 'b'\]"):
        eng.set_adapters(["a", "c"], {"a": 3.0})
    with pytest.raises(ValueError, match=r"'c'.*\['a', 'b'\]"):
        eng.set_adapters(["a", "b"], {"c": 3.0})
    assert eng.adapter_weights_key() == key and pw.active == ["a"] and eng.graphs == {"k": 1} and eng.cond_ready      # refused: nothing moved
    v = pw.lora_version
    eng.graphs = {"k": 1}
    eng.set_adapters(["a", "b"], {"a": 0.5, "b": 2.0})
    assert pw.active == ["a", "b"] and pw.lora_version == v + 1 and eng.graphs == {} and eng.adapter_weights == {"a": 0.5, "b": 2.0}
    assert eng.adapter_weights_key() != key


# ---------------------------------------------------------------------------------------------------------------- broadcast
def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


def _bcast_worker(rank, world, port, q):
    sys.path.insert(0, ROOT)
    os.environ.update(RANK=str(rank), LOCAL_RANK=str(rank), WORLD_SIZE=str(world), MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
    from loongx_amd import dist as lxd
    from loongx_amd.flux.weights import set_active_adapters
    lxd.init("gloo", timeout_s=120)
    truth = packed_with(16, AB)
    set_active_adapters(truth, ["a", "b"])
    want = {k: v.clone() for k, v in _lora_tensors(truth).items()}
    if rank == 0:
        pw = truth
    else:                                   # the same names and ranks, other contents, and only "a" active
        pw = packed_with(16, AB)
        for ad in pw.adapters.values():
            for t in ad.tensors().values():
                t.mul_(3.0)
    set_active_adapters(pw, ["a"])
    nb = lambda ts: sum(t.numel() * t.element_size() for t in ts)
    # what the engine reads (pw.t and the stacked adapter image, here "a" alone) and, beside it, both adapters of the registry
    expect = nb(pw.t.values()) + nb(_lora_tensors(pw).values()) - nb(v for k, v in pw.t.items() if k.startswith("mod.lora_")) \
        + nb(t for ad in pw.adapters.values() for t in ad.tensors().values())
    moved = lxd.broadcast_packed_weights(pw, src=0)
    set_active_adapters(pw, ["a", "b"])     # the receiving rank switches adapters from what arrived
    got = _lora_tensors(pw)
    ok = set(got) == set(want) and all(torch.equal(got[k], want[k]) for k in want) and moved == expect
    dist.barrier()
    dist.destroy_process_group()
    q.put((rank, bool(ok)))


def test_gloo_world2_broadcast_carries_the_registry():
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = _free_port()
    procs = [ctx.Process(target=_bcast_worker, args=(r, 2, port, q)) for r in range(2)]
    for p in procs:
        p.start()
    res = [q.get(timeout=180) for _ in procs]
    for p in procs:
        p.join(timeout=60)
    assert sorted(res) == [(0, True), (1, True)]
