"""The host side of generate(image= | image_latents=, mask_image= | latent_mask=, strength=): the schedule tail that `strength` leaves
(diffusers' get_timesteps), the packed latent mask (diffusers' mask_processor + prepare_mask_latents order) and the refusals that need no
device. No GPU: the scheduler's schedule lives on the host, pack_mask is torch on the CPU, and the entry points validate before launching."""
import ctypes
from types import SimpleNamespace

import numpy as np
import pytest
import torch


def _pipe():
    from loongx_amd.flux.pipeline import LxFluxPipeline
    return LxFluxPipeline(SimpleNamespace(device="cpu", config=SimpleNamespace(in_channels=64, guidance_embeds=True)))


def _schedule(pipe, n):
    from loongx_amd.flux.pipeline import calculate_shift, retrieve_timesteps
    cfg = pipe.scheduler.config
    mu = calculate_shift(16, cfg.base_image_seq_len, cfg.max_image_seq_len, cfg.base_shift, cfg.max_shift)
    return retrieve_timesteps(pipe.scheduler, n, "cpu", None, np.linspace(1.0, 1 / n, n), mu=mu)


@pytest.mark.parametrize("n,strength", [(4, 1.0), (4, 0.5), (4, 0.3), (28, 0.6)])
def test_get_timesteps_is_diffusers_arithmetic(n, strength):
    """diffusers: init_timestep = min(n * strength, n); t_start = int(max(n - init_timestep, 0)); timesteps[t_start * order:], n - t_start,
    scheduler.set_begin_index(t_start * order) -- restated here with the numbers written out."""
    t_start = {(4, 1.0): 0, (4, 0.5): 2, (4, 0.3): 2, (28, 0.6): 11}[(n, strength)]       # int(4 - 1.2) = 2; int(28 - 16.8) = int(11.2) = 11
    assert t_start == int(max(n - min(n * strength, n), 0))
    pipe = _pipe()
    full, n_full = _schedule(pipe, n)
    assert n_full == n and pipe.scheduler._step_index == 0
    full_host = pipe.scheduler.timesteps_host.copy()
    ts, left, th = pipe.get_timesteps(n, strength, "cpu")
    assert left == n - t_start and len(ts) == left
    assert torch.equal(ts, full[t_start:])
    assert isinstance(th, np.ndarray) and th.dtype == np.float32 and np.array_equal(th, full_host[t_start:])
    assert np.array_equal(th, ts.numpy())                            # the host slice holds the device slice's values: no read needed
    assert pipe.scheduler._begin_index == t_start and pipe.scheduler._step_index == t_start
    _schedule(pipe, n)                                               # a new schedule starts at its beginning again
    assert pipe.scheduler._begin_index == 0 and pipe.scheduler._step_index == 0


def test_get_timesteps_refuses_a_strength_that_leaves_no_step():
    pipe = _pipe()
    _schedule(pipe, 28)
    with pytest.raises(ValueError, match="< 1"):
        pipe.get_timesteps(28, 0.0, "cpu")
    assert pipe.scheduler._step_index == 0
    with pytest.raises(ValueError):
        pipe.scheduler.set_begin_index(28)
    from loongx_amd.flux.pipeline import FlowMatchEulerDiscreteScheduler
    with pytest.raises(ValueError, match="set_timesteps"):
        FlowMatchEulerDiscreteScheduler().set_begin_index(0)


def test_scale_noise_reads_sigma_on_the_host():
    """An index or a timestep of the schedule names the sigma; anything else is refused. (The launch itself: test_inpaint_kernels_gpu.py.)"""
    pipe = _pipe()
    _schedule(pipe, 4)
    sch = pipe.scheduler
    assert [sch._sigma_index(i) for i in (0, np.int64(3), 4)] == [0, 3, 4]
    assert sch._sigma_index(sch.timesteps[2]) == 2 and sch._sigma_index(float(sch.timesteps_host[1])) == 1
    for bad in (5, -1, 123.456):
        with pytest.raises(ValueError):
            sch._sigma_index(bad)


def _restated_pack(mask01, batch, height, width):
    """binarise, nearest resize (source index floor(dst * in / out)), repeat over 16 channels, 2x2 pack -- written with loops and indexing,
    nothing shared with the product's code"""
    m = (np.asarray(mask01, np.float32) >= 0.5).astype(np.float32)
    h, w = 2 * (height // 16), 2 * (width // 16)
    small = np.zeros((h, w), np.float32)
    for i in range(h):
        for j in range(w):
            small[i, j] = m[(i * m.shape[0]) // h, (j * m.shape[1]) // w]
    out = np.zeros((batch, (h // 2) * (w // 2), 64), np.float32)
    for i in range(h // 2):
        for j in range(w // 2):
            for c in range(16):
                for di in range(2):
                    for dj in range(2):
                        out[:, i * (w // 2) + j, c * 4 + di * 2 + dj] = small[2 * i + di, 2 * j + dj]
    return torch.from_numpy(out)


def test_pack_mask_on_a_rectangle_with_edges_inside_the_cells():
    """64 wide, 48 high (a 6 x 8 unpacked latent grid, 3 x 4 = 12 tokens); the rectangle's edges at rows 13 / 37 and columns 11 / 52 fall
    inside 8-pixel cells, so the sampled pixel -- the cell's first -- decides, and 2x2 groups of one token are split."""
    from PIL import Image
    H, W = 48, 64
    m = np.zeros((H, W), np.float32)
    m[13:37, 11:52] = 1.0
    m[0, 0] = 0.49                                                    # below the threshold; m[8, 8] exactly on it: >= 0.5 is white
    m[8, 8] = 0.5
    pipe = _pipe()
    want = _restated_pack(m, 2, H, W)
    assert want.shape == (2, 12, 64) and 0 < float(want.mean()) < 1
    assert any(0 < float(want[0, t].mean()) < 1 for t in range(12)), "the fixture should split a token's 2x2 group"
    t = torch.from_numpy(m)
    for given in (m, t, t[None], t[None, None], t[None, None].expand(2, 1, H, W), m[None]):
        got = pipe.pack_mask(given, 2, H, W)
        assert got.dtype == torch.float32 and got.is_contiguous() and torch.equal(got, want), type(given)
    # 0..255 images: PIL "L", PIL "RGB" (converted to "L"), uint8 arrays, bool
    m8 = (np.asarray(m >= 0.5) * 255).astype(np.uint8)
    m8[20, 20] = 127                                                   # 127 / 255 < 0.5 <= 128 / 255; neither pixel is a sampled one ...
    m8[16, 16], want8 = 128, want.clone()                              # ... but (16, 16) is, and stays white
    for given in (Image.fromarray(m8), Image.fromarray(m8).convert("RGB"), m8, torch.from_numpy(m8), torch.from_numpy(m8 >= 128)):
        assert torch.equal(pipe.pack_mask(given, 2, H, W), want8), type(given)
    m8[16, 16] = 127                                                   # the sampled pixel of cell (2, 2) turns black
    got = pipe.pack_mask(Image.fromarray(m8), 1, H, W)
    assert not torch.equal(got, want8[:1]) and torch.equal(got, _restated_pack(m8 / 255.0, 1, H, W))
    for bad in (t[None, None].expand(3, 1, H, W), t[None, None].expand(1, 2, H, W), torch.zeros(2, H, W), torch.zeros(5)):
        with pytest.raises(ValueError):
            pipe.pack_mask(bad, 2, H, W)


def test_prepare_params_names_the_new_keywords_and_keeps_its_tuple():
    from loongx_amd.flux.generate import prepare_inpaint_params, prepare_params
    kw = dict(prompt="p", image="i", image_latents="l", mask_image="m", latent_mask="k", strength=0.25, height=64, unknown=1)
    assert len(prepare_params(**kw)) == 18 and prepare_params(**kw)[:3] == ("p", None, 64)
    assert prepare_inpaint_params(**kw) == ("i", "l", "m", "k", 0.25)
    assert prepare_inpaint_params(prompt="p") == (None, None, None, None, 1.0)


N = 16
_x0, _half = torch.zeros(1, N, 64), torch.ones(1, N, 1)
HOST_ERRORS = {
    "strength_above": dict(image_latents=_x0, strength=1.5),
    "strength_below": dict(image_latents=_x0, strength=-0.1),
    "strength_nan": dict(image_latents=_x0, strength=float("nan")),
    "no_step_left": dict(image_latents=_x0, strength=0.0, num_inference_steps=28),
    "image_and_latents": dict(image=object(), image_latents=_x0),
    "both_masks": dict(image_latents=_x0, mask_image=np.ones((64, 64), np.float32), latent_mask=_half),
    "mask_without_source": dict(latent_mask=_half),
    "pixel_mask_without_source": dict(mask_image=np.ones((64, 64), np.float32)),
    "strength_without_source": dict(strength=0.5),
    "source_tokens": dict(image_latents=torch.zeros(1, N + 1, 64)),
    "source_batch": dict(image_latents=torch.zeros(3, N, 64)),
    "source_channels": dict(image_latents=torch.zeros(1, N, 16)),
    "mask_tokens": dict(image_latents=_x0, latent_mask=torch.ones(1, N - 1, 64)),
    "mask_batch": dict(image_latents=_x0, latent_mask=torch.ones(2, N, 1)),
    "mask_channels": dict(image_latents=_x0, latent_mask=torch.ones(1, N, 2)),
    "mask_above_one": dict(image_latents=_x0, latent_mask=_half * 1.5),
    "mask_negative": dict(image_latents=_x0, latent_mask=_half * -0.25),
    "mask_nan": dict(image_latents=_x0, latent_mask=_half * float("nan")),
}


@pytest.mark.parametrize("case", list(HOST_ERRORS))
def test_generate_refuses_before_it_touches_the_pipeline(case):
    """Every refusal is a ValueError raised before the pipeline, its transformer or its scheduler is used: the stand-in transformer here has
    no engine, no conditioning cache and no c_factor to lose, and the scheduler is as new afterwards."""
    from loongx_amd.flux.generate import generate
    pipe = _pipe()
    kw = dict(height=64, width=64, num_inference_steps=4, prompt_embeds=torch.zeros(1, 8, 32), pooled_prompt_embeds=torch.zeros(1, 32),
              output_type="latent", model_config={}, condition_scale=2.0)
    kw.update(HOST_ERRORS[case])
    with pytest.raises(ValueError):
        generate(None, pipe, **kw)
    assert not hasattr(pipe.transformer, "c_factor") and pipe.scheduler.timesteps is None and pipe.scheduler._step_index is None


def test_entry_points_validate_without_a_gpu():
    """NULL operands, and x0 / z / m on (or overlapping) x, return the error status with the entry point's name; nothing is launched."""
    from loongx_amd._lib import lib
    a, n = 0x10000, 1024                                                     # (fake, aligned addresses: nothing dereferences them)

    def blend(p):
        return lib.lx_euler_step_blend(p[0], p[1], 0, ctypes.c_float(-0.1), p[2], p[3], p[4], ctypes.c_float(0.5), n, None)
    for null in range(5):
        p = [a + i * 0x10000 for i in range(5)]
        p[null] = None
        assert blend(p) == -1 and b"lx_euler_step_blend" in lib.lx_last_error(), null
    for alias in (2, 3, 4):
        for delta in (0, 4 * (n - 1), -4 * (n - 1)):
            p = [a + i * 0x10000 for i in range(5)]
            p[alias] = p[0] + delta
            assert blend(p) == -1 and b"lx_euler_step_blend" in lib.lx_last_error(), (alias, delta)
    for null in range(3):
        p = [a, a + 0x10000, a + 0x20000]
        p[null] = None
        assert lib.lx_scale_noise(*p, ctypes.c_float(0.5), n, None) == -1 and b"lx_scale_noise" in lib.lx_last_error(), null
    assert lib.lx_scale_noise(a, a, a + 0x10000, ctypes.c_float(0.5), n, None) == -1 and b"lx_scale_noise" in lib.lx_last_error()


def test_cli_flags_reach_generate_only_when_given(tmp_path, monkeypatch):
    """inference.py --strength / --mask_dir: the input image, resized to the target size, becomes generate()'s `image`, the mask of the
    same file name its `mask_image`; without the flags no keyword is added (tests/test_inference_cli_cpu.py holds the recorded calls)."""
    from PIL import Image
    import inference as inf
    src = Image.fromarray((np.random.default_rng(0).random((16, 24, 3)) * 255).astype("uint8"))
    assert inf.edit_kwargs(src, 64) == {}
    kw = inf.edit_kwargs(src, 64, strength=0.5)
    assert set(kw) == {"image", "strength"} and kw["image"].size == (64, 64) and kw["strength"] == 0.5
    idir, mdir, odir = tmp_path / "in", tmp_path / "masks", tmp_path / "out"
    for d in (idir, mdir, odir):
        d.mkdir()
    src.save(idir / "a.png")
    Image.fromarray(np.full((16, 24), 255, np.uint8)).save(mdir / "a.png")
    seen = []

    def fake(model, condition_img, prompt, **kw):
        seen.append(kw)
        return src
    monkeypatch.setattr(inf, "inference_single_image", fake)
    model = SimpleNamespace(device=torch.device("cpu"))
    inf.process_image_batch(0, 1, model, ["a.png"], str(idir), str(odir), {}, {}, "subject", [0, -4], 64, 1)
    assert not {"image", "mask_image", "strength"} & set(seen[-1])
    inf.process_image_batch(0, 1, model, ["a.png"], str(idir), str(odir), {}, {}, "subject", [0, -4], 64, 1, mask_dir=str(mdir))
    assert seen[-1]["image"].size == (64, 64) and seen[-1]["mask_image"].mode == "L" and "strength" not in seen[-1]
    with pytest.raises(FileNotFoundError, match="b.png"):
        inf.edit_kwargs(src, 64, mask_path=str(mdir / "b.png"))
    with pytest.raises(SystemExit):
        inf.main(["--synthetic", "--strength", "0.5"])
