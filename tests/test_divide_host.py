"""Host side of the claim-splitting stage: the wide sampler's C-ABI entry points (declared, exported, bad arguments refused before
any launch), rlaif_v_amd.divide against values recorded from the reference's own functions (tests/golden/divide_host.json,
make_divide_golden.py), resume, the text-only configuration and the two-EOS cut rule.  No GPU."""
import json
import os
import sys
import types

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import divide_case as DC  # noqa: E402

P = 0x1000        # a non-NULL stand-in pointer: every call below is refused before anything is launched or dereferenced
WIDE = "rv_sample_token_wide"


def _lib():
    from rlaif_v_amd import hip
    return hip.lib()


# ------------------------------------------------------------------------------------------------ C ABI
def test_wide_sampler_declared_and_exported_in_abi_7():
    lib = _lib()
    assert lib.lib.rv_abi_version() == 7
    ret, args = lib.decls[WIDE]
    base = [n for _, n in lib.decls["rv_sample_token"][1]]
    assert ret == "int" and [n for _, n in args] == base[:-1] + ["workspace", "workspace_floats", "stream"]
    ret, args = lib.decls[WIDE + "_workspace_floats"]
    assert ret == "long" and [n for _, n in args] == ["M", "V_valid"]
    for name in (WIDE, WIDE + "_workspace_floats"):
        assert hasattr(lib.lib, name)
    ws = lib.lib.rv_sample_token_wide_workspace_floats
    assert ws(1, 128256) == 16 * 8192 and ws(3, 1) == 3 * 16 * 256 and ws(2, 262144) == 2 * 16 * 16384
    assert ws(0, 512) == 0 and ws(1, 0) == 0 and ws(1, 262145) == 0


def _wide(temperature=0.7, top_p=0.9, M=2, V=128256, ldl=None, penalty=1.0, u=P, logits=P, token=P, logp=P, seen_off=None,
          seen_ids=None, ws=P, ws_floats=None):
    lib = _lib().lib
    if ws_floats is None:
        ws_floats = max(int(lib.rv_sample_token_wide_workspace_floats(M, V)), 1)
    return lib.rv_sample_token_wide(logits, V if ldl is None else ldl, M, V, seen_off, seen_ids, penalty, temperature, top_p, u, token,
                                    logp, ws, ws_floats, None)


@pytest.mark.parametrize("kw,reason", [
    (dict(V=0), "1 <= V_valid <= 262144"),
    (dict(V=262145), "1 <= V_valid <= 262144"),
    (dict(V=70000, ldl=69999), "ldl >= V_valid"),
    (dict(logits=None), "NULL buffer"),
    (dict(token=None), "NULL buffer"),
    (dict(logp=None), "NULL buffer"),
    (dict(ws=None), "NULL buffer"),
    (dict(temperature=-0.5), "temperature must be >= 0"),
    (dict(top_p=0.0), "top_p must be > 0"),
    (dict(top_p=-1.0), "top_p must be > 0"),
    (dict(penalty=0.0), "penalty must be positive"),
    (dict(penalty=-2.0), "penalty must be positive"),
    (dict(u=None), "sampling needs the uniforms"),
    (dict(seen_off=P, penalty=1.3), "seen_off without seen_ids"),
    (dict(ws_floats=2 * 16 * 8192 - 1), "workspace smaller than rv_sample_token_wide_workspace_floats"),
    (dict(M=0), "M must be >= 1"),
], ids=lambda v: "-".join(f"{k}={x}" for k, x in v.items()) if isinstance(v, dict) else None)
def test_wide_sampler_refuses_bad_arguments(kw, reason):
    lib = _lib()
    assert _wide(**kw) == 1
    err = lib.last_error()
    assert err.startswith(WIDE + ":") and reason in err, err


def test_register_sampler_still_refuses_a_wide_row():
    lib = _lib()
    rc = lib.lib.rv_sample_token(P, 70000, 1, 70000, None, None, 1.0, 0.7, 0.9, P, P, P, None)
    assert rc == 1 and lib.last_error() == "rv_sample_token: V_valid <= 65536 (the row is held in registers)"


def test_ops_chooser_routes_by_vocabulary():
    from rlaif_v_amd import ops
    assert ops.sampler_for(1) == (ops.sample_token, False) and ops.sampler_for(65536) == (ops.sample_token, False)
    assert ops.sampler_for(65537) == (ops.sample_token_wide, True) and ops.sampler_for(262144) == (ops.sample_token_wide, True)
    with pytest.raises(ValueError, match="262144"):
        ops.sampler_for(262145)
    with pytest.raises(ValueError, match="sample_token_wide: logits"):
        ops.sample_token_wide(torch.zeros(2, 8), 2, 8, None)


# ------------------------------------------------------------------------------------------------ the stage's host logic
@pytest.fixture(scope="module")
def gold():
    with open(DC.GOLD_HOST) as f:
        return json.load(f)


def test_get_facts_matches_the_reference(gold):
    from rlaif_v_amd import divide
    assert len(gold["get_facts"]) >= 7
    for case in gold["get_facts"]:
        assert divide.get_facts(case["in"]) == case["out"], case["in"]
    outs = [c["out"] for c in gold["get_facts"]]
    assert [] in outs and any("" in o for o in outs) and any(o and not o[0].startswith("T") for o in outs)     # the edge cases are in


def test_prompt_wrappers_match_the_reference(gold):
    from rlaif_v_amd import divide
    for case in gold["divide"]:
        assert divide.divide_messages(dict(case["item"])) == case["messages"]
    assert any(len(c["messages"][0]["content"].split(" ")) == 300 for c in gold["divide"]), "an answer cut at 300 words"
    keys = [next(k for k in ("raw_question", "prompt", "question") if k in c["item"]) for c in gold["divide"]]
    assert set(keys) == {"raw_question", "prompt", "question"} and any("answer" not in c["item"] for c in gold["divide"])
    for case in gold["changeq"]:
        assert divide.changeq_messages(dict(case["item"])) == case["messages"]
    assert any(isinstance(c["item"]["facts"], str) for c in gold["changeq"])


def test_construct_question_yesno_matches_the_reference(gold, tmp_path):
    from rlaif_v_amd import divide
    src, dst = tmp_path / "in.gq.jsonl", tmp_path / "in.gq.qas.jsonl"
    src.write_text("".join(json.dumps(r) + "\n" for r in gold["yesno"]["records"]))
    got = divide.construct_question_yesno(str(src), str(dst))
    want = gold["yesno"]["out"]
    assert got == want and [json.loads(line) for line in dst.read_text().splitlines()] == want
    assert [list(r) for r in got] == [list(r) for r in want], "key order"
    assert len(want) == 4 and want[2]["image_path"] == "img/1.jpg" and want[2]["ds_question_id"] == 71
    bad = tmp_path / "bad.jsonl"
    bad.write_text(json.dumps({"question_id": 9, "facts": [], "changed_facts": [], "metainfos": {}}) + "\n")
    with pytest.raises(ValueError) as e:
        divide.construct_question_yesno(str(bad), str(dst))
    assert str(e.value) == gold["yesno"]["no_image_path_raises"]


def test_output_file_names_match_the_reference(gold):
    from rlaif_v_amd import divide
    for case in gold["paths"]:
        ap = dict(zip(case["argv"][::2], case["argv"][1::2]))
        got = divide.output_paths(ap["--path"], int(ap.get("--start", 0)), int(ap.get("--end", -1)), int(ap.get("--chunk-num", 1)),
                                  int(ap.get("--chunk-idx", 0)), ap.get("--divide_suffix", "llama3-8b_divide"))
        assert list(got) == case["files"], case["argv"]
    assert gold["paths"][0]["files"][0] == "data/answers.s0-e-1.chunk1-0.llama3-8b_divide.jsonl"


def test_select_items_and_input_formats(tmp_path):
    from rlaif_v_amd import divide
    data = [{"i": i} for i in range(10)]
    assert divide.select_items(data) == data and divide.select_items(data, 2, 7) == data[2:7]
    assert divide.select_items(data, 0, 99) == data and divide.select_items(data, 0, -1, 3, 1) == data[4:8]
    assert divide.select_items(data, 0, -1, 3, 2) == data[8:] and divide.select_items(data, 1, -2) == data[1:-2]
    assert divide.select_items([], 0, -1, 2, 0) == []
    for name, text in (("a.json", json.dumps(data)), ("b.jsonl", "".join(json.dumps(d) + "\n" for d in data)),
                       ("c.json", json.dumps(data[0]))):
        (tmp_path / name).write_text(text)
    assert divide.read_items(str(tmp_path / "a.json")) == data and divide.read_items(str(tmp_path / "b.jsonl")) == data
    assert divide.read_items(str(tmp_path / "c.json")) == [data[0]]


def _stub_model(calls):
    def generate(prompts, images, max_new_tokens, temperature=0.0, top_p=1.0, eos_token_id=None, generator=None):
        assert images is None and all(int(p[0]) == 1 and int(p[1]) == 1 and int(p[2]) != 1 for p in prompts), "two BOS ids"
        calls.append(dict(n=len(prompts), max_new_tokens=max_new_tokens, temperature=temperature, top_p=top_p, eos=eos_token_id,
                          u=float(torch.rand(1, generator=generator))))
        return [[[11 + len(calls), 15, 12 + k, 20, 13, 3]] for k in range(len(prompts))]
    return types.SimpleNamespace(cfg=types.SimpleNamespace(arch="text"), generate=generate)


def test_batch_inference_records_and_resume(tmp_path):
    from rlaif_v_amd import divide
    items = [{"question_id": i, "raw_question": f"q {i}?", "answer": f"answer {i}.", "metainfos": {"n": i}} for i in range(5)]
    src, ans = tmp_path / "in.jsonl", tmp_path / "out" / "in.div.jsonl"
    src.write_text("".join(json.dumps(d) + "\n" for d in items))
    # a pre-filled answer file of 2 lines: 2 items are skipped, 3 records are appended behind them
    ans.parent.mkdir()
    old = [dict(items[0], raw_facts="kept", facts=["kept"]), dict(items[1], raw_facts="kept too", facts=[])]
    ans.write_text("".join(json.dumps(d) + "\n" for d in old))
    calls, tok = [], DC.StubTokenizer()
    recs = divide.batch_inference(_stub_model(calls), tok, str(src), str(ans), "facts", divide.divide_messages, batch_size=2, seed=7)
    assert [c["n"] for c in calls] == [2, 1] and len(tok.templated) == 3 and "q 2?" in tok.templated[0]
    assert all(c["max_new_tokens"] == 256 and c["temperature"] == 0.2 and c["top_p"] == 0.9 and c["eos"] == [2, 3] for c in calls)
    assert calls[0]["u"] == float(torch.rand(1, generator=torch.Generator().manual_seed(7)))
    lines = [json.loads(line) for line in ans.read_text().splitlines()]
    assert lines[:2] == old and lines == recs and [r["question_id"] for r in lines] == [0, 1, 2, 3, 4]
    assert list(lines[2]) == ["question_id", "raw_question", "answer", "metainfos", "raw_facts", "facts"]
    assert lines[2]["raw_facts"] == "### Facts:\n- w12 \n- w12 \n- w13" and lines[2]["facts"] == ["w12", "w12", "w13"]
    assert lines[4]["facts"] == ["w13", "w12", "w13"]
    # complete file: nothing is generated, nothing appended
    n = len(calls)
    assert divide.batch_inference(_stub_model(calls), tok, str(src), str(ans), "facts", divide.divide_messages) == lines
    assert len(calls) == n and len(ans.read_text().splitlines()) == 5
    with pytest.raises(ValueError, match="input file"):
        divide.batch_inference(_stub_model(calls), tok, str(src), str(src), "facts", divide.divide_messages)
    with pytest.raises(NotImplementedError, match="text-only"):
        divide.batch_inference(types.SimpleNamespace(cfg=types.SimpleNamespace(arch="llava")), tok, str(src), str(ans), "facts",
                               divide.divide_messages)


def test_run_writes_the_three_files_with_stubbed_models(tmp_path):
    from rlaif_v_amd import divide
    items = [{"question_id": i, "question": f"q {i}?", "answer": f"a {i}.", "metainfos": {"image_path": f"{i}.jpg", "ds_question_id": 9 + i}}
             for i in range(3)]
    src = tmp_path / "ans.jsonl"
    src.write_text("".join(json.dumps(d) + "\n" for d in items))
    loaded, calls = [], []

    def load(name):
        loaded.append(name)
        return _stub_model(calls), DC.StubTokenizer()
    paths = divide.run(str(src), load, "DIV", "CHG", bs=2, seed=3)
    assert loaded == ["DIV", "CHG"] and [os.path.basename(p) for p in paths] == [
        "ans.s0-e-1.chunk1-0.llama3-8b_divide.jsonl", "ans.s0-e-1.chunk1-0.llama3-8b_divide.gq.jsonl",
        "ans.s0-e-1.chunk1-0.llama3-8b_divide.gq.qas.jsonl"]
    gq = [json.loads(line) for line in open(paths[1])]
    assert list(gq[0]) == ["question_id", "question", "answer", "metainfos", "raw_facts", "facts", "raw_changed_facts", "changed_facts"]
    qas = [json.loads(line) for line in open(paths[2])]
    assert len(qas) == sum(min(len(r["facts"]), len(r["changed_facts"])) for r in gq) > 0
    assert qas[0]["question"].endswith(" Please answer yes or no.") and qas[0]["image_path"] == "0.jpg" and qas[0]["ds_question_id"] == 9


# ------------------------------------------------------------------------------------------------ text-only configuration
LLAMA3 = {"architectures": ["LlamaForCausalLM"], "model_type": "llama", "hidden_size": 4096, "intermediate_size": 14336,
          "num_hidden_layers": 32, "num_attention_heads": 32, "num_key_value_heads": 8, "vocab_size": 128256, "rms_norm_eps": 1e-5,
          "rope_theta": 500000.0, "rope_scaling": None, "max_position_embeddings": 8192, "tie_word_embeddings": False,
          "bos_token_id": 128000, "eos_token_id": 128009, "attention_bias": False, "hidden_act": "silu"}


def test_text_config_from_a_llama_config_json(tmp_path):
    from rlaif_v_amd.checkpoint import config_from_hf, hf_config_dict
    from rlaif_v_amd.model import ParamStore
    from rlaif_v_amd.textlm import TextLMConfig, TextLMModel
    (tmp_path / "config.json").write_text(json.dumps(LLAMA3))
    cfg = config_from_hf(json.loads((tmp_path / "config.json").read_text()))
    assert isinstance(cfg, TextLMConfig) and cfg.arch == "text" and cfg == TextLMConfig()
    assert (cfg.hidden, cfg.layers, cfg.heads, cfg.n_kv_heads, cfg.kv_group, cfg.ffn, cfg.vocab, cfg.head_dim) == \
        (4096, 32, 32, 8, 4, 14336, 128256, 128)
    assert cfg.rope_theta == 500000.0 and cfg.n_image_tokens == 0 and cfg.vision_param_entries() == ([], [])
    assert cfg.vocab_padded == 128256
    assert config_from_hf(hf_config_dict(cfg)) == cfg
    with pytest.raises(NotImplementedError, match="rope_scaling"):
        config_from_hf(dict(LLAMA3, rope_scaling={"rope_type": "llama3", "factor": 8.0}))
    with pytest.raises(NotImplementedError, match="tie_word_embeddings"):
        config_from_hf(dict(LLAMA3, tie_word_embeddings=True))
    # the store: the language model alone, nothing trainable, no vision key
    tiny = DC.tiny_text_cfg()
    st = ParamStore(tiny, "cpu", with_optimizer=False)
    assert st.vision_keys == [] and st.n_train == 0 and st.flat_g.numel() == 0 and st.flat_master is None
    assert not any("mm_projector" in k or "vision" in k for k in st.offsets)
    assert set(st.hf_slices(tiny)) == set(DC.tiny_text_weights(1024, 0))
    with pytest.raises(NotImplementedError, match="text-only"):
        ParamStore(tiny, "cpu", with_optimizer=True)
    if not torch.cuda.is_available():
        with pytest.raises(RuntimeError, match="no CPU fallback"):
            TextLMModel(tiny)
    with pytest.raises(NotImplementedError, match="training a text-only model"):
        TextLMModel(tiny, with_optimizer=True)
    with pytest.raises(NotImplementedError, match="TextLMModel.forward_logps: training"):
        TextLMModel.forward_logps(object())


def test_eos_ids_and_the_cut_rule():
    from rlaif_v_amd.splice import cut_behind_eos, eos_id_set
    assert eos_id_set(None) is None and eos_id_set(2) == (2,) and eos_id_set([2, 3]) == (2, 3) and eos_id_set((128001, 128009, 128001)) == (128001, 128009)
    assert eos_id_set(torch.tensor([7, 9])) == (7, 9)
    for bad in ([], "2", [2.5], True, [True], 2.0):
        with pytest.raises(ValueError, match="eos_token_id"):
            eos_id_set(bad)
    seq = [5, 9, 3, 7, 2, 3]
    assert cut_behind_eos(seq, None) == seq and cut_behind_eos(seq, (2,)) == [5, 9, 3, 7, 2]
    assert cut_behind_eos(seq, (2, 3)) == [5, 9, 3] and cut_behind_eos(seq, (3, 2)) == [5, 9, 3]
    assert cut_behind_eos(seq, (11, 12)) == seq and cut_behind_eos([2], (2, 3)) == [2] and cut_behind_eos([], (2,)) == []
