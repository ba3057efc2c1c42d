"""Which LoRA ranks a checkpoint may carry (weights._check_lora_ranks through pack_state_dict and install_lora), on the tiny config:
one rank per checkpoint; r * (modules behind one GEMM) <= 16 as before, or an even r <= 64 outside precise mode."""
import pytest
import torch

from tests.helpers import tiny_transformer


def _cfg(tr):
    from loongx_amd.flux.weights import FluxConfig
    c = tr.config
    return FluxConfig(num_layers=c.num_layers, num_single_layers=c.num_single_layers, num_attention_heads=c.num_attention_heads,
                      attention_head_dim=c.attention_head_dim, in_channels=c.in_channels, joint_attention_dim=c.joint_attention_dim,
                      pooled_projection_dim=c.pooled_projection_dim, guidance_embeds=c.guidance_embeds, axes_dims_rope=c.axes_dims_rope)


def with_rank(sd, r, seed=0, only=None):
    """The state dict with every adapter (or those whose key contains `only`) redrawn at rank r: N(0, 0.02^2) down and up."""
    g = torch.Generator().manual_seed(seed)
    out = {}
    for k, v in sd.items():
        if ".lora_A." in k and (only is None or only in k):
            v = torch.randn(r, v.shape[1], generator=g) * 0.02
        elif ".lora_B." in k and (only is None or only in k):
            v = torch.randn(v.shape[0], r, generator=g) * 0.02
        out[k] = v
    return out


@pytest.fixture(scope="module")
def tiny():
    tr = tiny_transformer(seed=0)
    return tr, {k: v.detach().clone() for k, v in tr.state_dict().items()}


def _lora_only(sd):
    return {"transformer." + k.replace(".default.", "."): v.contiguous() for k, v in sd.items() if ".lora_" in k}


@pytest.mark.parametrize("r", [2, 3, 4, 8, 16, 64])
def test_pack_and_install_accept_the_rank(tiny, r):
    from loongx_amd.flux.weights import install_lora, pack_state_dict
    tr, sd = tiny
    wide = with_rank(sd, r)
    pw = pack_state_dict(wide, _cfg(tr), "cpu")
    assert pw.cfg.lora_r == r
    assert pw.lora["s0.fused"].down.shape == (4 * r, 256) and pw.lora["s0.fused"].up.shape == (7 * 256, r)
    assert pw.lora["d0.qkv"].down.shape[0] == 3 * r and pw.lora["x_embedder"].down.shape[0] == r
    nb = 4
    assert pw.t["mod.lora_down"].shape == (nb * r, 256) and pw.t["mod.lora_up.0"].shape == (6 * 256, r)
    # the same adapters installed over a rank-4 model: the same tensors
    pw4 = pack_state_dict(sd, _cfg(tr), "cpu")
    assert pw4.cfg.lora_r == 4
    assert install_lora(pw4, _lora_only(wide)) == 25
    assert pw4.cfg.lora_r == r
    for name, lo in pw.lora.items():
        assert torch.equal(lo.down, pw4.lora[name].down) and torch.equal(lo.up, pw4.lora[name].up), name
    assert torch.equal(pw.t["mod.lora_down"], pw4.t["mod.lora_down"])


@pytest.mark.parametrize("r", [66, 7, 128])
def test_pack_and_install_refuse_the_rank(tiny, r):
    from loongx_amd.flux.weights import install_lora, pack_state_dict
    tr, sd = tiny
    bad = with_rank(sd, r)
    with pytest.raises(ValueError, match="64"):                   # the message names the real limit
        pack_state_dict(bad, _cfg(tr), "cpu")
    pw = pack_state_dict(sd, _cfg(tr), "cpu")
    before = {k: v.down.clone() for k, v in pw.lora.items()}
    with pytest.raises(ValueError, match="64"):
        install_lora(pw, _lora_only(bad))
    assert pw.cfg.lora_r == 4 and all(torch.equal(pw.lora[k].down, v) for k, v in before.items())      # a refused set installs nothing


def test_mixed_ranks_raise(tiny):
    from loongx_amd.flux.weights import install_lora, pack_state_dict
    tr, sd = tiny
    mixed = with_rank(sd, 8, only="single_transformer_blocks.1.proj_out")
    with pytest.raises(ValueError, match="share one rank"):
        pack_state_dict(mixed, _cfg(tr), "cpu")
    pw = pack_state_dict(sd, _cfg(tr), "cpu")
    with pytest.raises(ValueError, match="share one rank"):
        install_lora(pw, _lora_only(mixed))


def test_precise_packing_keeps_the_narrow_limit(tiny):
    from loongx_amd.flux.weights import install_lora, pack_state_dict
    tr, sd = tiny
    with pytest.raises(ValueError, match="precise"):
        pack_state_dict(with_rank(sd, 16), _cfg(tr), "cpu", precise=True)
    pw = pack_state_dict(sd, _cfg(tr), "cpu", precise=True)      # rank 4: accepted as before
    assert pw.cfg.lora_r == 4 and pw.precise_ready
    with pytest.raises(ValueError, match="precise.*16|16.*precise"):
        install_lora(pw, _lora_only(with_rank(sd, 16)))
    assert pw.cfg.lora_r == 4
