"""Host side of the top-k samplers and of the generation-config defaults (no GPU): the float64 restatement of
tests/topk_case.py against the installed transformers' own warpers, the two new C-ABI entry points' declarations and argument
refusals, rlaif_v_amd.genconfig.resolve_sampling's precedence, and what the three command lines resolve to with and without
--hf_defaults."""
import inspect
import json
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import generate_case as GC  # noqa: E402
import topk_case as TK  # noqa: E402

P = 0x1000        # a non-NULL stand-in pointer: every call below is refused before anything is launched or dereferenced
REG, WIDE = "rv_sample_token_topk", "rv_sample_token_wide_topk"


def _lib():
    from rlaif_v_amd import hip
    return hip.lib()


# ------------------------------------------------------------------------------------------------ the restatement
@pytest.mark.parametrize("V,seed,scale", [(512, 3, 4.0), (1000, 8, 2.0), (4099, 10, 8.0)])
def test_restatement_equals_the_transformers_warpers(V, seed, scale):
    """softmax(TopP(TopK(Temperature(x)))) of the installed transformers to 1e-12, over rows, temperatures, top_k and top_p"""
    row = GC.peaked_row(V, seed=seed, scale=scale)
    worst = 0.0
    for temperature in (0.2, 0.7, 1.0):
        for top_k in (1, 2, 50, V, V + 100):
            for top_p in (1.0, 0.9):
                p, _, gap = TK.sampler_probs64_topk(row, temperature, top_p, top_k)
                worst = max(worst, float(np.abs(p - TK.hf_warped_probs_topk(row, temperature, top_p, top_k)).max()))
                assert int((p > 0).sum()) <= min(top_k, V)
                assert (gap == np.inf) == (top_k >= V)
                if top_k >= V:            # off: the restatement without top-k
                    assert np.array_equal(p, GC.sampler_probs64(row, temperature, top_p)[0])
    print(f"[topk] V={V}: max |restatement - transformers| = {worst:.2e}")
    assert worst <= 1e-12


def test_restatement_keeps_everything_tied_with_the_kth_as_transformers_does():
    row = np.asarray([1, 3, 2, 2, 2, .5, -1], dtype=np.float32)
    p, edge, gap = TK.sampler_probs64_topk(row, 1.0, 1.0, 2)
    assert np.nonzero(p > 0)[0].tolist() == [1, 2, 3, 4] and edge == np.inf
    assert abs(gap - 0.5) < 1e-12                                   # 2 against 1, relative to 2
    assert np.abs(p - TK.hf_warped_probs_topk(row, 1.0, 1.0, 2)).max() <= 1e-12
    zeros = np.asarray([2, 0.0, -0.0, -1, 0.0], dtype=np.float32)   # -0.0 and +0.0 tie by value
    p, _, _ = TK.sampler_probs64_topk(zeros, 1.0, 1.0, 2)
    assert np.nonzero(p > 0)[0].tolist() == [0, 1, 2, 4]
    assert np.abs(p - TK.hf_warped_probs_topk(zeros, 1.0, 1.0, 2)).max() <= 1e-12
    # a penalty moves the cut: the top token, penalised, leaves the top 1
    p, _, _ = TK.sampler_probs64_topk(row, 1.0, 1.0, 1, seen_ids=[1], penalty=2.0)
    assert np.nonzero(p > 0)[0].tolist() == [2, 3, 4]
    # temperature 0: the distribution greedy's logp refers to, top_k ignored
    assert np.array_equal(TK.sampler_probs64_topk(row, 0.0, 0.5, 2)[0], GC.sampler_probs64(row, 0.0, 0.5)[0])


# ------------------------------------------------------------------------------------------------ C ABI
def test_topk_samplers_declared_and_exported_in_abi_7():
    lib = _lib()
    assert lib.lib.rv_abi_version() == 7
    for name, base in ((REG, "rv_sample_token"), (WIDE, "rv_sample_token_wide")):
        ret, args = lib.decls[name]
        names = [n for _, n in lib.decls[base][1]]
        at = names.index("top_p") + 1
        assert ret == "int" and [n for _, n in args] == names[:at] + ["top_k"] + names[at:]
        assert dict((n, t) for t, n in args)["top_k"] == "int"
        assert [t for t, n in args if n != "top_k"] == [t for t, _ in lib.decls[base][1]]
        assert hasattr(lib.lib, name)


def _reg(temperature=0.7, top_p=0.9, top_k=50, M=2, V=32000, ldl=None, penalty=1.0, u=P, logits=P, token=P, logp=P, seen_off=None,
         seen_ids=None):
    return _lib().lib.rv_sample_token_topk(logits, V if ldl is None else ldl, M, V, seen_off, seen_ids, penalty, temperature, top_p,
                                           top_k, u, token, logp, None)


def _wide(temperature=0.7, top_p=0.9, top_k=50, M=2, V=128256, ldl=None, penalty=1.0, u=P, logits=P, token=P, logp=P, seen_off=None,
          seen_ids=None, ws=P, ws_floats=None):
    lib = _lib().lib
    if ws_floats is None:
        ws_floats = max(int(lib.rv_sample_token_wide_workspace_floats(M, V)), 1)
    return lib.rv_sample_token_wide_topk(logits, V if ldl is None else ldl, M, V, seen_off, seen_ids, penalty, temperature, top_p,
                                         top_k, u, token, logp, ws, ws_floats, None)


_IDS = dict(ids=lambda v: "-".join(f"{k}={x}" for k, x in v.items()) if isinstance(v, dict) else None)


@pytest.mark.parametrize("kw,reason", [
    (dict(top_k=-1), "top_k must be >= 0"),
    (dict(top_k=-50, temperature=0.0), "top_k must be >= 0"),
    (dict(V=0), "M, V_valid > 0, ldl >= V_valid"),
    (dict(M=0), "M, V_valid > 0, ldl >= V_valid"),
    (dict(V=512, ldl=511), "M, V_valid > 0, ldl >= V_valid"),
    (dict(V=65537), "V_valid <= 65536"),
    (dict(logits=None), "NULL buffer"),
    (dict(token=None), "NULL buffer"),
    (dict(logp=None), "NULL buffer"),
    (dict(temperature=-0.5), "temperature must be >= 0"),
    (dict(top_p=0.0), "top_p must be > 0"),
    (dict(penalty=0.0), "penalty must be positive"),
    (dict(u=None), "sampling needs the uniforms"),
    (dict(seen_off=P, penalty=1.3), "seen_off without seen_ids"),
], **_IDS)
def test_register_topk_sampler_refuses_bad_arguments(kw, reason):
    lib = _lib()
    assert _reg(**kw) == 1
    err = lib.last_error()
    assert err.startswith(REG + ":") and reason in err, err


@pytest.mark.parametrize("kw,reason", [
    (dict(top_k=-1), "top_k must be >= 0"),
    (dict(top_k=-50, temperature=0.0), "top_k must be >= 0"),
    (dict(V=0), "1 <= V_valid <= 262144"),
    (dict(V=262145), "1 <= V_valid <= 262144"),
    (dict(V=70000, ldl=69999), "ldl >= V_valid"),
    (dict(logits=None), "NULL buffer"),
    (dict(token=None), "NULL buffer"),
    (dict(logp=None), "NULL buffer"),
    (dict(ws=None), "NULL buffer"),
    (dict(logits=P + 2), "4-byte aligned"),
    (dict(temperature=-0.5), "temperature must be >= 0"),
    (dict(top_p=0.0), "top_p must be > 0"),
    (dict(top_p=-1.0), "top_p must be > 0"),
    (dict(penalty=0.0), "penalty must be positive"),
    (dict(penalty=-2.0), "penalty must be positive"),
    (dict(u=None), "sampling needs the uniforms"),
    (dict(seen_off=P, penalty=1.3), "seen_off without seen_ids"),
    (dict(ws_floats=2 * 16 * 8192 - 1), "workspace smaller than rv_sample_token_wide_workspace_floats"),
    (dict(M=0), "M must be >= 1"),
], **_IDS)
def test_streamed_topk_sampler_refuses_bad_arguments(kw, reason):
    lib = _lib()
    assert _wide(**kw) == 1
    err = lib.last_error()
    assert err.startswith(WIDE + ":") and reason in err, err


def test_ops_take_top_k_last_and_refuse_a_negative_one():
    from rlaif_v_amd import ops
    from rlaif_v_amd.model import LlavaDPOModel
    for fn in (ops.sample_token, ops.sample_token_wide):
        par = inspect.signature(fn).parameters
        assert list(par)[-1] == "top_k" and par["top_k"].default == 0
        for bad in (-1, 2.5):
            with pytest.raises(ValueError, match="top_k must be an integer >= 0"):
                fn(torch.zeros(2, 8), 2, 8, None, top_k=bad)
    par = inspect.signature(LlavaDPOModel.generate).parameters
    names = list(par)
    assert names[names.index("num_beams") + 1] == "top_k" and par["top_k"].default == 0
    assert par["top_k"].kind == inspect.Parameter.POSITIONAL_OR_KEYWORD
    assert "top_k" not in inspect.signature(LlavaDPOModel.beam_search).parameters
    assert ops.sampler_for(32000) == (ops.sample_token, False) and ops.sampler_for(128256) == (ops.sample_token_wide, True)


# ------------------------------------------------------------------------------------------------ generation_config.json
def _ckpt(tmp_path, name, cfg=None):
    d = tmp_path / name
    d.mkdir()
    if cfg is not None:
        (d / "generation_config.json").write_text(json.dumps(cfg))
    return str(d)


def test_resolve_sampling_precedence(tmp_path):
    from rlaif_v_amd.genconfig import HF_4_35_DEFAULTS, resolve_sampling
    lib_defaults = dict(temperature=1.0, top_p=1.0, top_k=50, repetition_penalty=1.0)      # transformers 4.35, the reference's pin
    assert HF_4_35_DEFAULTS == lib_defaults
    none = _ckpt(tmp_path, "no_file")
    assert resolve_sampling(none) == lib_defaults
    assert resolve_sampling(None) == lib_defaults and resolve_sampling(str(tmp_path / "missing")) == lib_defaults
    some = _ckpt(tmp_path, "some", {"top_p": 0.6, "temperature": 0.9, "bos_token_id": 1, "transformers_version": "4.31.0"})
    assert resolve_sampling(some) == dict(temperature=0.9, top_p=0.6, top_k=50, repetition_penalty=1.0)
    nulls = _ckpt(tmp_path, "nulls", {"top_p": None, "top_k": None, "temperature": 0.6, "repetition_penalty": 1.1})
    assert resolve_sampling(nulls) == dict(temperature=0.6, top_p=1.0, top_k=50, repetition_penalty=1.1)
    off = _ckpt(tmp_path, "off", {"top_k": 0, "top_p": 0.9})
    assert resolve_sampling(off) == dict(temperature=1.0, top_p=0.9, top_k=0, repetition_penalty=1.0)
    # explicit values win over the file and the defaults, one by one; an explicit 0 is a value (off), not absence
    assert resolve_sampling(some, temperature=0.7) == dict(temperature=0.7, top_p=0.6, top_k=50, repetition_penalty=1.0)
    assert resolve_sampling(some, top_p=0.95, top_k=30) == dict(temperature=0.9, top_p=0.95, top_k=30, repetition_penalty=1.0)
    assert resolve_sampling(nulls, top_k=0, repetition_penalty=1.0) == dict(temperature=0.6, top_p=1.0, top_k=0, repetition_penalty=1.0)
    assert resolve_sampling(none, 0.2, 0.9, 5, 1.3) == dict(temperature=0.2, top_p=0.9, top_k=5, repetition_penalty=1.3)
    r = resolve_sampling(some)
    assert isinstance(r["top_k"], int) and all(isinstance(r[k], float) for k in ("temperature", "top_p", "repetition_penalty"))
    with pytest.raises(ValueError, match="top_k"):
        resolve_sampling(none, top_k=-1)
    with pytest.raises(ValueError, match="top_k"):
        resolve_sampling(_ckpt(tmp_path, "bad", {"top_k": -3}))


# ------------------------------------------------------------------------------------------------ the command lines
def test_gen_data_command_line(tmp_path):
    from rlaif_v_amd import gen_data
    ck = _ckpt(tmp_path, "llava", {"top_p": 0.6, "temperature": 0.9, "top_k": None})
    base = ["--checkpoint", ck, "--ds_name", "q.jsonl", "--answer_file", "a.jsonl"]
    ap = gen_data.build_parser()
    today = dict(temperature=0.7, top_p=1.0, top_k=0, repetition_penalty=1.0)
    assert gen_data.sampling_args(ap.parse_args(base)) == today
    assert gen_data.sampling_args(ap.parse_args(base + ["--temperature", "0.5", "--top_p", "0.8"])) == dict(today, temperature=0.5, top_p=0.8)
    assert gen_data.sampling_args(ap.parse_args(base + ["--top_k", "50"])) == dict(today, top_k=50)
    # --hf_defaults: what is not on the command line comes from the file, then from transformers 4.35
    assert gen_data.sampling_args(ap.parse_args(base + ["--hf_defaults"])) == dict(temperature=0.9, top_p=0.6, top_k=50, repetition_penalty=1.0)
    assert gen_data.sampling_args(ap.parse_args(base + ["--hf_defaults", "--temperature", "0.7"])) == \
        dict(temperature=0.7, top_p=0.6, top_k=50, repetition_penalty=1.0)
    assert gen_data.sampling_args(ap.parse_args(base + ["--hf_defaults", "--top_k", "0", "--top_p", "1.0"])) == \
        dict(temperature=0.9, top_p=1.0, top_k=0, repetition_penalty=1.0)
    with pytest.raises(ValueError, match="top_k"):
        gen_data.sampling_args(ap.parse_args(base + ["--top_k", "-2"]))
    par = inspect.signature(gen_data.generate_answers).parameters
    assert par["top_k"].default == 0 and par["temperature"].default == 0.7 and par["top_p"].default == 1.0


def test_vqa_command_line(tmp_path):
    from rlaif_v_amd import vqa
    ck = _ckpt(tmp_path, "llava", {"top_p": 0.6, "repetition_penalty": 1.2})
    base = ["--model-path", ck, "--question-file", "q.jsonl", "--answers-file", "a.jsonl"]
    ap = vqa.build_parser()
    today = dict(temperature=0.2, top_p=1.0, top_k=0, repetition_penalty=1.0)
    assert vqa.sampling_args(ap.parse_args(base)) == today
    assert vqa.sampling_args(ap.parse_args(base + ["--temperature", "0", "--num_beam", "3"])) == dict(today, temperature=0.0)
    assert vqa.sampling_args(ap.parse_args(base + ["--top_k", "30", "--top_p", "0.9"])) == dict(today, top_k=30, top_p=0.9)
    # beam search (the default --num_beams 3) samples nothing: --hf_defaults resolves nothing there
    assert vqa.sampling_args(ap.parse_args(base + ["--hf_defaults"])) == today
    assert vqa.sampling_args(ap.parse_args(base + ["--hf_defaults", "--temperature", "0", "--num_beam", "3"])) == dict(today, temperature=0.0)
    base = base + ["--num_beams", "1"]
    assert vqa.sampling_args(ap.parse_args(base + ["--hf_defaults", "--temperature", "0.2"])) == \
        dict(temperature=0.2, top_p=0.6, top_k=50, repetition_penalty=1.2)
    assert vqa.sampling_args(ap.parse_args(base + ["--hf_defaults"])) == dict(temperature=1.0, top_p=0.6, top_k=50, repetition_penalty=1.2)
    assert vqa.sampling_args(ap.parse_args(base + ["--hf_defaults", "--top_k", "30", "--top_p", "0.95", "--temperature", "0.5"])) == \
        dict(temperature=0.5, top_p=0.95, top_k=30, repetition_penalty=1.2)
    par = inspect.signature(vqa.answer_questions).parameters
    assert par["top_k"].default == 0 and par["repetition_penalty"].default == 1.0 and par["top_p"].default is None


def test_divide_command_line_resolves_each_checkpoint(tmp_path):
    from rlaif_v_amd import divide
    div = _ckpt(tmp_path, "divide", {"top_k": 40, "temperature": 0.6, "top_p": 0.5})
    gq = _ckpt(tmp_path, "changeq", {"repetition_penalty": 1.1, "top_k": None})
    fixed = dict(temperature=0.2, top_p=0.9)                         # the explicit values of the reference's pipeline call
    assert (divide.TEMPERATURE, divide.TOP_P) == (0.2, 0.9)
    assert divide.stage_sampling(div) == dict(fixed, top_k=0, repetition_penalty=1.0)
    assert divide.stage_sampling(div, top_k=7) == dict(fixed, top_k=7, repetition_penalty=1.0)
    assert divide.stage_sampling(div, hf_defaults=True) == dict(fixed, top_k=40, repetition_penalty=1.0)
    assert divide.stage_sampling(gq, hf_defaults=True) == dict(fixed, top_k=50, repetition_penalty=1.1)
    assert divide.stage_sampling(gq, top_k=0, hf_defaults=True) == dict(fixed, top_k=0, repetition_penalty=1.1)
    with pytest.raises(ValueError, match="top_k"):
        divide.stage_sampling(div, top_k=-1)
    ap = divide.build_parser()
    base = ["--path", "x.jsonl", "--divide_model", div, "--changeq_model", gq]
    a = ap.parse_args(base)
    from rlaif_v_amd.genconfig import given_on_command_line
    assert a.top_k == 0 and given_on_command_line(a)["top_k"] is None and a.hf_defaults is False
    a = ap.parse_args(base + ["--hf_defaults", "--top_k", "5"])
    assert a.top_k == 5 and given_on_command_line(a)["top_k"] == 5 and a.hf_defaults is True
    a = ap.parse_args(base + ["--hf_defaults", "--top_k", "0"])
    assert given_on_command_line(a)["top_k"] == 0, "an explicit 0 is a value: off for both checkpoints"

    # run() hands every stage its own checkpoint's values
    calls = []

    class Model:
        class cfg:
            arch = "text"

        def generate(self, prompts, images, **kw):
            calls.append((kw["temperature"], kw["top_p"], kw.get("top_k", 0), kw.get("repetition_penalty", 1.0)))
            return [[[9]] for _ in prompts]
    src = tmp_path / "answers.jsonl"
    src.write_text(json.dumps({"question_id": 0, "raw_question": "q", "answer": "a", "metainfos": {"image_path": "i", "ds_question_id": 1}}) + "\n")
    sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
    import divide_case as DC
    load = lambda name: (Model(), DC.StubTokenizer())                # noqa: E731
    divide.run(str(src), load, div, gq, hf_defaults=True)
    assert calls == [(0.2, 0.9, 40, 1.0), (0.2, 0.9, 50, 1.1)]
    del calls[:]
    for f in tmp_path.glob("answers.s*"):
        f.unlink()
    divide.run(str(src), load, div, gq)
    assert calls == [(0.2, 0.9, 0, 1.0), (0.2, 0.9, 0, 1.0)]
