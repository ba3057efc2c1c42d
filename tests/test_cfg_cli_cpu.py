"""inference.py --true_cfg_scale / --negative_prompt: accepted by the parser, handed to generate() only when given. Under the recording
stub of tests/test_inference_cli_cpu.py a run without them records the calls of tests/golden/inference_cli.json, a run with them the same
calls with exactly the two keywords more."""
import pytest

from tests.test_inference_cli_cpu import case  # noqa: F401  (the fixture: the recorder, the stand-in model and the recorded calls)


def _run(case, tag, **flags):  # noqa: F811
    """batch_inference as the recorded call made it; returns (the recorder's calls, the keyword names generate() received per call)"""
    inf, rec, model, idir, cap, pkl, want, tmp = case
    import src.flux.generate as sg
    inner, names, given = sg.generate, [], []

    def generate(model, pipeline, **kw):
        names.append(set(kw))
        given.append({k: kw[k] for k in ("true_cfg_scale", "negative_prompt") if k in kw})
        return inner(model, pipeline, **kw)
    sg.generate = generate                    # (the fixture's monkeypatch puts the module's own back)
    rec.calls = []
    try:
        inf.batch_inference(model, idir, str(tmp / tag), caption_path=cap, condition_type="subject", target_size=256, position_delta=[0, -16],
                            seed=7, brain_data_path=pkl, **flags)
    finally:
        sg.generate = inner
    return list(rec.calls), names, given


def test_the_flags_reach_generate_only_when_given(case):  # noqa: F811
    want = case[6]["batch"]["calls"]
    plain, plain_names, plain_given = _run(case, "plain")
    assert plain == want and len(plain) == 7
    assert all(g == {} for g in plain_given)
    guided, names, given = _run(case, "guided", true_cfg_scale=3.5, negative_prompt="blurry")
    assert guided == want, "the flags changed something else that reaches generate()"
    assert all(g == {"true_cfg_scale": 3.5, "negative_prompt": "blurry"} for g in given) and len(given) == 7
    assert [n - p for n, p in zip(names, plain_names)] == [{"true_cfg_scale", "negative_prompt"}] * 7
    assert all(p <= n for n, p in zip(names, plain_names))
    _, _, only_scale = _run(case, "scale", true_cfg_scale=2.0)
    assert all(g == {"true_cfg_scale": 2.0} for g in only_scale)


def test_cfg_kwargs_and_the_parser():
    import inference as inf
    assert inf.cfg_kwargs() == {} and inf.cfg_kwargs(None, None) == {}
    assert inf.cfg_kwargs(2.0) == {"true_cfg_scale": 2.0} and inf.cfg_kwargs(negative_prompt="n") == {"negative_prompt": "n"}
    with pytest.raises(SystemExit):                       # (synthetic runs have no text encoder for a negative prompt)
        inf.main(["--synthetic", "--true_cfg_scale", "2.0", "--negative_prompt", "blurry"])
    with pytest.raises(SystemExit):
        inf.main(["--true_cfg_scale", "much"])


def test_the_parser_accepts_the_flags(monkeypatch, tmp_path):
    """main() with the two flags gets as far as loading the model: the stub there sees what the parser made of them"""
    import inference as inf
    seen = {}

    def stop(model, input_dir, output_dir, caption_path=None, **kw):
        seen.update(kw)
    monkeypatch.setattr(inf, "load_model", lambda *a, **k: None)
    monkeypatch.setattr(inf, "batch_inference", stop)
    inf.main(["--input_dir", str(tmp_path), "--output_dir", str(tmp_path / "o"), "--num_gpus", "1", "--true_cfg_scale", "2.5",
              "--negative_prompt", "low quality"])
    assert seen["true_cfg_scale"] == 2.5 and seen["negative_prompt"] == "low quality"
    seen.clear()
    inf.main(["--input_dir", str(tmp_path), "--output_dir", str(tmp_path / "o"), "--num_gpus", "1"])
    assert seen["true_cfg_scale"] is None and seen["negative_prompt"] is None
