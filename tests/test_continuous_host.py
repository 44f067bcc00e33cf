"""Host side of continuous batching: the two C-ABI entry points of csrc/decode_state.hip (declared, exported, bad arguments
refused before any launch), the slot scheduler's step counts on seeded workloads, the per-request uniforms, and the
``--continuous`` option of rlaif_v_amd.gen_data on a stubbed model.  No GPU."""
import ctypes
import math
import os
import sys
import types

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

P = 0x7F0000010000          # a "device operand": 64 KiB aligned, never dereferenced (every call below is refused before any launch)


def _lib():
    from rlaif_v_amd import hip
    return hip.lib()


# ------------------------------------------------------------------------------------------------ the C ABI
_TAIL = ["len", "budget", "done", "pre_off", "pre_len", "own_off", "eos_ids", "n_eos", "out_tokens", "seen_ids", "u_table", "ld_t", "S",
         "T", "tok_in", "pos", "dst", "pre_len_eff", "own_len", "u_next", "stream"]


def test_entry_points_declared_and_exported_in_abi_7():
    lib = _lib()
    assert lib.lib.rv_abi_version() == 7
    ret, args = lib.decls["rv_decode_advance"]
    assert ret == "int" and [n for _, n in args] == ["token"] + _TAIL
    ret, args = lib.decls["rv_decode_admit"]
    assert ret == "int" and [n for _, n in args] == ["slots", "new_pre_off", "new_pre_len", "new_budget", "n", "token"] + _TAIL
    assert hasattr(lib.lib, "rv_decode_advance") and hasattr(lib.lib, "rv_decode_admit")
    from rlaif_v_amd import ops, schedule
    from rlaif_v_amd.model import LlavaDPOModel
    assert all(hasattr(ops, n) for n in ("DecodeState", "decode_advance", "decode_admit"))
    assert all(hasattr(schedule, n) for n in ("SlotRows", "SlotScheduler", "uniform_table"))
    assert hasattr(LlavaDPOModel, "generate_continuous")


def _ints(*v):
    return (ctypes.c_int * len(v))(*v)


_EOS = _ints(2, 7)


def _host_ptr(a):
    return None if a is None else ctypes.cast(a, ctypes.c_void_p)


def _advance(**kw):
    a = dict(token=P, len=P, budget=P, done=P, pre_off=P, pre_len=P, own_off=P, eos_ids=_EOS, n_eos=2, out_tokens=P, seen_ids=P,
             u_table=P, ld_t=16, S=200, T=16, tok_in=P, pos=P, dst=P, pre_len_eff=P, own_len=P, u_next=P)
    a.update(kw)
    a["eos_ids"] = _host_ptr(a["eos_ids"])
    return _lib().lib.rv_decode_advance(*a.values(), None)


def _admit(**kw):
    a = dict(slots=_ints(3, 0, 199), new_pre_off=_ints(0, 40, 80), new_pre_len=_ints(9, 12, 1), new_budget=_ints(16, 1, 7), n=3,
             token=P, len=P, budget=P, done=P, pre_off=P, pre_len=P, own_off=P, eos_ids=_EOS, n_eos=2, out_tokens=P, seen_ids=P,
             u_table=P, ld_t=16, S=200, T=16, tok_in=P, pos=P, dst=P, pre_len_eff=P, own_len=P, u_next=P)
    a.update(kw)
    for k in ("slots", "new_pre_off", "new_pre_len", "new_budget", "eos_ids"):
        a[k] = _host_ptr(a[k])
    return _lib().lib.rv_decode_admit(*a.values(), None)


_DEVICE_ARRAYS = ("token", "len", "budget", "done", "pre_off", "pre_len", "own_off", "out_tokens", "seen_ids", "u_table", "tok_in",
                  "pos", "dst", "pre_len_eff", "own_len", "u_next")


@pytest.mark.parametrize("call,who", [(_advance, "rv_decode_advance"), (_admit, "rv_decode_admit")])
def test_decode_state_entries_refuse_bad_arguments(call, who):
    lib = _lib()
    assert call(S=0) == 1 and "S >= 1" in lib.last_error() and lib.last_error().startswith(who + ":")
    assert call(T=0) == 1 and "T >= 1" in lib.last_error()
    assert call(ld_t=15) == 1 and "ld_t >= T" in lib.last_error()
    assert call(S=4000000, ld_t=1024) == 1 and "int32" in lib.last_error()
    assert call(n_eos=9) == 1 and "8 EOS ids" in lib.last_error()
    assert call(n_eos=-1) == 1
    assert call(eos_ids=None) == 1 and "eos_ids" in lib.last_error()
    for name in _DEVICE_ARRAYS:
        assert call(**{name: None}) == 1 and "NULL" in lib.last_error() and lib.last_error().startswith(who + ":"), name
        assert call(**{name: P + 2}) == 1 and "aligned" in lib.last_error(), name
    for name in ("out_tokens", "seen_ids", "u_table"):
        assert call(**{name: None}) == 1 and "NULL table" in lib.last_error(), name


def test_decode_admit_refuses_bad_lists():
    lib = _lib()
    assert _admit(n=0) == 1 and "1 <= n <= 64" in lib.last_error() and lib.last_error().startswith("rv_decode_admit:")
    assert _admit(n=65) == 1 and "1 <= n <= 64" in lib.last_error()
    for name in ("slots", "new_pre_off", "new_pre_len", "new_budget"):
        assert _admit(**{name: None}) == 1 and "NULL host list" in lib.last_error(), name
    assert _admit(slots=_ints(3, 200, 1)) == 1 and "outside [0, S)" in lib.last_error()
    assert _admit(slots=_ints(3, -1, 1)) == 1 and "outside [0, S)" in lib.last_error()
    assert _admit(slots=_ints(3, 0, 3)) == 1 and "twice" in lib.last_error()
    assert _admit(new_budget=_ints(16, 17, 7)) == 1 and "budget" in lib.last_error()             # budget > T
    assert _admit(new_budget=_ints(16, 0, 7)) == 1 and "budget" in lib.last_error()
    assert _admit(new_pre_len=_ints(9, -1, 1)) == 1 and "span" in lib.last_error()
    assert _admit(new_pre_off=_ints(-4, 0, 1)) == 1 and "span" in lib.last_error()


# ------------------------------------------------------------------------------------------------ cache rows
def test_slot_rows_layout():
    from rlaif_v_amd.schedule import SlotRows
    rows = SlotRows(regions=3, max_prompt_tokens=20, slots=70, max_new=5)
    assert rows.own_base == 60 and rows.n_rows == 60 + 70 * 5 and rows.chunks == [(0, 64), (64, 70)]
    assert rows.own_off.dtype == torch.int32 and rows.own_off.tolist() == [60 + 5 * s for s in range(70)]
    t = rows.prefill_rows([2, 0], [7, 20])
    assert t.dtype == torch.int32 and t.tolist() == list(range(40, 47)) + list(range(0, 20))
    for bad in (([0, 0], [3, 3]), ([0], [21]), ([3], [4]), ([0], [0]), ([0, 1], [3])):
        with pytest.raises(ValueError):
            rows.prefill_rows(*bad)
    with pytest.raises(ValueError):
        SlotRows(regions=0, max_prompt_tokens=20, slots=4, max_new=5)


# ------------------------------------------------------------------------------------------------ the scheduler
WORKLOADS = [(60, 10), (600, 1), (60, 4)]


def _lengths(n, repeat, seed):
    from rlaif_v_amd.schedule import length_table
    flat = length_table(n * repeat, seed)
    assert all(1 <= x <= 512 for x in flat)
    return [flat[i * repeat:(i + 1) * repeat] for i in range(n)]


@pytest.mark.parametrize("seed", [0, 1, 2])
@pytest.mark.parametrize("n,repeat", WORKLOADS)
def test_scheduler_step_counts_on_the_seeded_workloads(n, repeat, seed):
    """64 slots, flags read every 8 steps, answer lengths log-normal (median 90, sigma 0.6) clipped to [1, 512] - an assumed
    distribution.  The static scheme is generate() on 64 // repeat prompts per call."""
    from rlaif_v_amd import schedule
    lengths = _lengths(n, repeat, seed)
    trace = []
    sched = schedule.simulate(lengths, slots=64, repeat=repeat, poll_every=8, trace=trace)
    assert [q for q, _, _ in sched.history] == list(range(n)), "every request is admitted exactly once (here: in order)"
    assert not sched.live and sorted(sched.free_slots) == list(range(64)) and sorted(sched.free_regions) == list(range(sched.regions))
    for _, owner, regions in trace:
        held = [o for o in owner if o is not None]
        assert len(set(held)) == len(held), "a (request, sample) holds one slot"
        assert {q for q, _ in held} <= set(regions), "a slot is held by a live request only"
        assert len(set(regions.values())) == len(regions), "no region is held by two live requests"
        for q in regions:
            assert sum(1 for o in held if o[0] == q) <= repeat
    tokens = sum(map(sum, lengths))
    static = schedule.static_decode_steps(lengths, 64 // repeat, 512, 8)
    print(f"[{n} x {repeat}, seed {seed}] {tokens} tokens: static {static} decode steps, continuous {sched.steps_executed} "
          f"({static / sched.steps_executed:.2f} x fewer), floor {math.ceil(tokens / 64)}, {sched.polls} polls")
    assert sched.steps_executed < static
    assert sched.steps_executed >= math.ceil(tokens / 64)


def test_scheduler_rules():
    from rlaif_v_amd.schedule import SlotScheduler, simulate
    s = SlotScheduler(slots=4, repeat=2, regions=3, poll_every=8)
    assert s.room() == 2
    assert s.admit(10, budget=5) == (0, [0, 1]) and s.admit(11, budget=3) == (1, [2, 3]) and s.room() == 0
    with pytest.raises(RuntimeError):
        s.admit(12, budget=5)
    assert s.steps_to_poll() == 4                      # the longest live budget: 5 tokens = the prefill's + 4 steps
    for _ in range(2):
        s.step()
    fin, comp = s.poll([0, 1, 1, 1])                   # request 11 whole, sample 1 of request 10
    assert fin == [(1, 10, 1), (2, 11, 0), (3, 11, 1)] and comp == [11]
    assert s.room() == 1 and s.chunk_live(0, 1) and not s.chunk_live(1, 4)
    assert s.admit(12, budget=9) == (1, [1, 2])        # the lowest free slots, the freed region
    assert s.steps_to_poll() == 8
    t = SlotScheduler(slots=4, repeat=1)
    t.admit(12, budget=2)
    with pytest.raises(ValueError):
        t.admit(12, budget=2)                          # a live request is not admitted again
    for _ in range(2):
        s.step()
    with pytest.raises(RuntimeError, match="not flagged done"):
        s.poll([0, 0, 0, 1])                           # slot 0 has used its 5 tokens: the device must have flagged it
    assert s.steps_executed == 4
    for bad in (dict(slots=0), dict(repeat=0), dict(poll_every=0), dict(slots=4, repeat=5), dict(regions=0)):
        with pytest.raises(ValueError):
            SlotScheduler(**{**dict(slots=4, repeat=1), **bad})
    # a budget of one token costs no decode step at all
    assert simulate([[1], [1], [1]], slots=2, repeat=1).steps_executed == 0


# ------------------------------------------------------------------------------------------------ uniforms
def test_uniforms_are_a_function_of_seed_request_sample_and_step():
    from rlaif_v_amd.schedule import uniform_table
    T, R, n = 12, 3, 9
    whole = [uniform_table(4, i, T, R) for i in range(n)]                   # a run over [0, n)
    for i in (0, 5, 8):
        alone = uniform_table(4, i, T, R)                                   # a run over [i, i + 1)
        assert torch.equal(alone, whole[i])
    t = whole[5]
    assert t.dtype == torch.float32 and tuple(t.shape) == (T, R) and bool(((t >= 0) & (t < 1)).all())
    assert torch.equal(uniform_table(4, 5, 2 * T, R + 2)[:T, :R], t), "neither max_new_tokens nor repeat moves a sample's stream"
    assert not torch.equal(uniform_table(5, 5, T, R), t), "another seed, other uniforms"
    assert not torch.equal(whole[4], t) and not torch.equal(t[:, 0], t[:, 1])
    flat = torch.cat([w.reshape(-1) for w in whole])
    assert flat.unique().numel() >= flat.numel() - 1 and 0.4 < float(flat.mean()) < 0.6


# ------------------------------------------------------------------------------------------------ gen_data
def _tok():
    sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden"))
    from toy_tokenizer import ToyTokenizer

    class Tok(ToyTokenizer):
        def decode(self, ids, skip_special_tokens=True):
            return " " + " ".join(f"t{int(i)}" for i in ids if not (skip_special_tokens and int(i) in (0, 1, 2))) + " "
    return Tok()


def _stub():
    calls = []

    def generate(prompts, images, max_new_tokens, repeat=1, temperature=0.0, top_p=1.0, repetition_penalty=1.0, eos_token_id=None,
                 generator=None, return_scores=False):
        calls.append(dict(kind="generate", n=len(prompts)))
        return [[[100 + r, 2] for r in range(repeat)] for _ in prompts]

    def generate_continuous(requests, max_new_tokens, slots=64, repeat=1, temperature=0.0, top_p=1.0, top_k=0,
                            repetition_penalty=1.0, eos_token_id=None, seed=0, max_prompt_tokens=None, poll_every=8,
                            request_indices=None):
        reqs = list(zip(request_indices, requests))
        calls.append(dict(kind="continuous", n=len(reqs), slots=slots, repeat=repeat, seed=seed, eos=eos_token_id,
                          max_prompt_tokens=max_prompt_tokens, max_new_tokens=max_new_tokens, indices=[i for i, _ in reqs]))
        assert all(int((p == -200).sum()) == 1 and int(p[0]) == 1 and im is not None for _, (p, im) in reqs)
        for index, _ in reversed(reqs):                # completion order is not item order
            yield index, [[10 * index + r + 3, 2] for r in range(repeat)]
    model = types.SimpleNamespace(cfg=types.SimpleNamespace(arch="llava", n_image_tokens=2), generate=generate,
                                  generate_continuous=generate_continuous)
    return model, calls


def _items():
    img = torch.zeros(3, 4, 4)
    return [dict(question="What is shown ?", image=img, question_id="q0", metainfos={"ds_question_id": 70, "origin": "a"}),
            dict(question="Describe the scene .", image=img, metainfos={"origin": "b"}),
            dict(question="How many apples ?", image=img, question_id=12)]


def test_continuous_stage_gives_todays_record_keys_and_item_order():
    from rlaif_v_amd import autocheck, gen_data
    tok, items = _tok(), _items()
    model, calls = _stub()
    today = gen_data.generate_answers(model, tok, items, repeat=3, temperature=0.7, max_tokens=8, seed=5, model_path="ckpt")
    assert [c["kind"] for c in calls] == ["generate"], "without the option generate_continuous is never called"
    model, calls = _stub()
    recs = gen_data.generate_answers(model, tok, items, repeat=3, temperature=0.7, max_tokens=8, seed=5, model_path="ckpt",
                                     continuous=True, slots=16, index_base=40)
    assert [c["kind"] for c in calls] == ["continuous"]
    c = calls[0]
    assert (c["n"], c["slots"], c["repeat"], c["seed"], c["eos"], c["max_new_tokens"]) == (3, 16, 3, 5, 2, 8)
    assert c["indices"] == [40, 41, 42], "the request index is the item's absolute index in the question file"
    longest = max(int(autocheck.wrap_question_for_llava15(it["question"], tok).numel()) for it in items) + 2 - 1
    assert c["max_prompt_tokens"] == longest
    assert len(recs) == len(today) == 9
    assert [list(r) for r in recs] == [list(r) for r in today]
    for key in ("question_id", "raw_question", "metainfos", "model_path"):
        assert [r[key] for r in recs] == [r[key] for r in today], key
    assert [r.get("ds_question_id") for r in recs] == [r.get("ds_question_id") for r in today]
    assert [r["answer"] for r in recs] == [f"t{10 * (40 + n) + r + 3}" for n in range(3) for r in range(3)]
    assert gen_data.generate_answers(model, tok, [], continuous=True) == []


def test_command_line_leaves_the_option_off_by_default():
    from rlaif_v_amd import gen_data
    base = ["--checkpoint", "c", "--ds_name", "q", "--answer_file", "a"]
    args = gen_data.build_parser().parse_args(base)
    assert args.continuous is False and args.slots == 64
    args = gen_data.build_parser().parse_args(base + ["--continuous", "--slots", "32", "--start", "100"])
    assert args.continuous is True and args.slots == 32 and args.start == 100


def test_generate_continuous_refuses_by_name_before_any_launch():
    """the checks run at the call, not at the first next(): no device is touched (this test has none)"""
    from rlaif_v_amd.model import LlavaDPOModel

    def model(**kw):
        cfg = dict(arch="llava", head_dim=128, model_max_length=64, vocab=512)
        cfg.update(kw.pop("cfg", {}))
        m = types.SimpleNamespace(cfg=types.SimpleNamespace(**cfg), lora=kw.pop("lora", None), _row_splicer=lambda: kw.get("splicer"))
        return m
    call = LlavaDPOModel.generate_continuous
    reqs = [(torch.tensor([1, -200, 5]), torch.zeros(3, 4, 4))]
    with pytest.raises(NotImplementedError, match="LoRA"):
        call(model(lora=object()), reqs, 4)
    with pytest.raises(NotImplementedError, match="OmniLMM"):
        call(model(cfg=dict(arch="omnilmm")), reqs, 4)
    with pytest.raises(NotImplementedError, match="OmniLMM"):
        call(model(splicer=object()), reqs, 4)
    with pytest.raises(NotImplementedError, match="head_dim 128"):
        call(model(cfg=dict(head_dim=64)), reqs, 4)
    with pytest.raises(NotImplementedError, match="num_beams"):
        call(model(), reqs, 4, num_beams=3)
    with pytest.raises(ValueError, match="repeat 5 > slots 4"):
        call(model(), reqs, 4, slots=4, repeat=5)
    with pytest.raises(ValueError, match="8 EOS ids"):
        call(model(), reqs, 4, eos_token_id=list(range(9)))
    with pytest.raises(ValueError):
        call(model(), reqs, 0)
