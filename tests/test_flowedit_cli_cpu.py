"""inference.py's FlowEdit flags on the host, without a GPU: --source_prompt, --source_guidance_scale, --flowedit_n_max and
--flowedit_n_avg reach generate()'s keywords of the same names, each only when given, with the input image as the source; nothing else that
reaches generate() changes."""
import pytest

from tests.test_inference_cli_cpu import case  # noqa: F401  (the fixture: the recorder, the stand-in model and the recorded calls)

KEYS = ("source_prompt", "source_guidance_scale", "flowedit_n_max", "flowedit_n_avg")


def _run(case, tag, **flags):  # noqa: F811
    """batch_inference as the recorded call made it; returns (the recorder's calls, the keyword names generate() received per call, the
    FlowEdit keywords of each, the size of the `image` each got)"""
    inf, rec, model, idir, cap, pkl, want, tmp = case
    import src.flux.generate as sg
    inner, names, given, sizes = sg.generate, [], [], []

    def generate(model, pipeline, **kw):
        names.append(set(kw))
        given.append({k: kw[k] for k in KEYS if k in kw})
        sizes.append(kw["image"].size if "image" in kw else None)
        return inner(model, pipeline, **kw)
    sg.generate = generate                    # (the fixture's monkeypatch puts the module's own back)
    rec.calls = []
    try:
        inf.batch_inference(model, idir, str(tmp / tag), caption_path=cap, condition_type="subject", target_size=256, position_delta=[0, -16],
                            seed=7, brain_data_path=pkl, **flags)
    finally:
        sg.generate = inner
    return list(rec.calls), names, given, sizes


def test_the_flags_reach_generate_only_when_given(case):  # noqa: F811
    inf, want = case[0], case[6]["batch"]["calls"]
    plain, plain_names, plain_given, plain_sizes = _run(case, "plain")
    assert plain == want and all(g == {} for g in plain_given) and all(s is None for s in plain_sizes)
    # the description alone: the input image, at the target size, is the source
    calls, names, given, sizes = _run(case, "source", flowedit=inf.flowedit_kwargs("a cat on a sofa"))
    assert calls == want, "the flag changed something else that reaches generate()"
    assert all(g == {"source_prompt": "a cat on a sofa"} for g in given) and len(given) == len(plain_given) > 0
    assert [n - p for n, p in zip(names, plain_names)] == [{"source_prompt", "image"}] * len(names) and all(s == (256, 256) for s in sizes)
    # all four
    full = dict(source_prompt="a cat", source_guidance_scale=2.0, flowedit_n_max=20, flowedit_n_avg=2)
    calls, names, given, sizes = _run(case, "all", flowedit=inf.flowedit_kwargs(**full))
    assert calls == want and all(g == full for g in given)
    assert [n - p for n, p in zip(names, plain_names)] == [set(KEYS) | {"image"}] * len(names)
    # with a strength as well the image is passed once, and generate() is the one that refuses the pair
    calls, names, given, sizes = _run(case, "strength", strength=0.5, flowedit=inf.flowedit_kwargs("a cat"))
    assert [n - p for n, p in zip(names, plain_names)] == [{"source_prompt", "image", "strength"}] * len(names)


def test_flowedit_kwargs_and_edit_kwargs():
    import inference as inf
    assert inf.flowedit_kwargs() == {} and inf.edit_kwargs(None, 64) == {} and inf.edit_kwargs(None, 64, flowedit={}) == {}
    assert inf.flowedit_kwargs("a dog", None, 12) == {"source_prompt": "a dog", "flowedit_n_max": 12}
    assert inf.flowedit_kwargs(flowedit_n_avg=0) == {"flowedit_n_avg": 0}          # (passed as given: generate() is what refuses it)
    # numbers without a description go along untouched and bring no image with them: generate() checks them and runs the plain call
    assert inf.edit_kwargs(None, 64, flowedit={"flowedit_n_avg": 2}) == {"flowedit_n_avg": 2}
    from PIL import Image
    kw = inf.edit_kwargs(Image.new("L", (32, 48)), 64, flowedit=inf.flowedit_kwargs("a dog", 1.0))
    assert set(kw) == {"image", "source_prompt", "source_guidance_scale"} and kw["image"].size == (64, 64) and kw["image"].mode == "RGB"


def test_the_parser(monkeypatch, tmp_path):
    import inference as inf
    with pytest.raises(SystemExit):
        inf.main(["--flowedit_n_max", "many"])
    with pytest.raises(SystemExit):
        inf.main(["--synthetic", "--source_prompt", "a cat"])
    seen = {}

    def stop(model, input_dir, output_dir, caption_path=None, **kw):
        seen.update(kw)
    monkeypatch.setattr(inf, "load_model", lambda *a, **k: None)
    monkeypatch.setattr(inf, "batch_inference", stop)
    base = ["--input_dir", str(tmp_path), "--output_dir", str(tmp_path / "o"), "--num_gpus", "1"]
    inf.main(base + ["--source_prompt", "a cat", "--source_guidance_scale", "2.5", "--flowedit_n_max", "20", "--flowedit_n_avg", "3"])
    assert seen["flowedit"] == {"source_prompt": "a cat", "source_guidance_scale": 2.5, "flowedit_n_max": 20, "flowedit_n_avg": 3}
    seen.clear()
    inf.main(base + ["--source_prompt", "a cat"])
    assert seen["flowedit"] == {"source_prompt": "a cat"}
    seen.clear()
    inf.main(base)
    assert seen["flowedit"] == {}
