"""Host side of KV-cached candidate generation: the three new C-ABI entry points (declared, exported, bad shapes refused before
any launch), the float64 restatement of the sampler against transformers' own warpers, the cache-row planner and the record
format of rlaif_v_amd.gen_data on a stubbed model.  No GPU."""
import os
import sys
import types

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import generate_case as GC  # noqa: E402

P = 0x1000        # a non-NULL stand-in pointer: every call below is refused before anything is launched or dereferenced


def _lib():
    from rlaif_v_amd import hip
    return hip.lib()


def test_entry_points_declared_and_exported_in_abi_7():
    lib = _lib()
    assert lib.lib.rv_abi_version() == 7
    ret, args = lib.decls["rv_gemm_nt_skinny_bf16"]
    assert ret == "int" and [n for _, n in args] == ["A", "lda", "W", "ldw", "C", "ldc", "M", "N", "K", "residual", "ldr", "out_f32",
                                                     "stream"]
    ret, args = lib.decls["rv_attn_decode"]
    assert ret == "int" and [n for _, n in args] == ["q", "ldq", "kv", "ldkv", "k_col0", "v_col0", "pre_off", "pre_len", "own_off",
                                                     "own_len", "out", "ldo", "lse", "M", "H", "hd", "kv_group", "scale", "n_split",
                                                     "workspace", "workspace_floats", "stream"]
    ret, args = lib.decls["rv_attn_decode_workspace_floats"]
    assert ret == "long" and [n for _, n in args] == ["M", "H", "n_split"]
    ret, args = lib.decls["rv_sample_token"]
    assert ret == "int" and [n for _, n in args] == ["logits", "ldl", "M", "V_valid", "seen_off", "seen_ids", "penalty", "temperature",
                                                     "top_p", "u", "token", "logp", "stream"]
    for name in ("rv_gemm_nt_skinny_bf16", "rv_attn_decode", "rv_attn_decode_workspace_floats", "rv_sample_token"):
        assert hasattr(lib.lib, name)
    header = open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "include", "rlaifv_hip.h")).read()
    block = header[header.index("KV-cached candidate generation"):]
    assert block.count("ROUNDING") >= 1 and "Containment" in block and "bit-identical" in block


def _skinny(M, N, K, lda=None, out_f32=0):
    return _lib().lib.rv_gemm_nt_skinny_bf16(P, lda or K, P, K, P, N, M, N, K, None, 0, out_f32, None)


def test_skinny_gemm_refuses_bad_shapes():
    lib = _lib()
    assert _skinny(0, 64, 64) == 1 and "1 <= M <= 64" in lib.last_error()
    assert _skinny(65, 64, 64) == 1 and "1 <= M <= 64" in lib.last_error()
    assert _skinny(4, 64, 96) == 1 and "multiple of 64" in lib.last_error()
    assert _skinny(4, 64, 0) == 1
    assert _skinny(4, 66, 64) == 1 and "multiple of 4" in lib.last_error()
    assert _skinny(4, 64, 64, lda=60) == 1
    assert _skinny(4, 64, 64, out_f32=2) == 1
    assert lib.lib.rv_gemm_nt_skinny_bf16(None, 64, P, 64, P, 64, 4, 64, 64, None, 0, 0, None) == 1 and "NULL" in lib.last_error()


def _attn(hd=128, n_split=1, M=2, H=4, kv_group=2, ws=None):
    lib = _lib().lib
    need = ws if ws is not None else max(int(lib.rv_attn_decode_workspace_floats(M, H, n_split)), 1)
    return lib.rv_attn_decode(P, H * hd, P, 2 * H * hd, 0, H * hd, P, P, P, P, P, H * hd, None, M, H, hd, kv_group, 0.1, n_split, P,
                              need, None)


def test_attn_decode_refuses_bad_shapes():
    lib = _lib()
    assert _attn(hd=64) == 1 and "hd must be 128" in lib.last_error()
    assert _attn(n_split=0) == 1 and "n_split" in lib.last_error()
    assert _attn(M=0) == 1
    assert _attn(kv_group=3) == 1
    assert _attn(H=4, kv_group=8) == 1
    assert _attn(ws=7) == 1 and "workspace" in lib.last_error()
    assert lib.lib.rv_attn_decode_workspace_floats(2, 4, 3) == 2 * 4 * 3 * 132
    assert lib.lib.rv_attn_decode_workspace_floats(2, 4, 0) == 0 and lib.lib.rv_attn_decode_workspace_floats(0, 4, 1) == 0


def _sample(temperature=0.7, top_p=0.9, M=1, V=512, ldl=576, penalty=1.0, u=P):
    return _lib().lib.rv_sample_token(P, ldl, M, V, None, None, penalty, temperature, top_p, u, P, P, None)


def test_sample_token_refuses_bad_arguments():
    lib = _lib()
    assert _sample(top_p=0.0) == 1 and "top_p" in lib.last_error()
    assert _sample(top_p=-0.5) == 1 and "top_p" in lib.last_error()
    assert _sample(temperature=-1.0) == 1 and "temperature" in lib.last_error()
    assert _sample(M=0) == 1
    assert _sample(V=600, ldl=576) == 1 and "ldl >= V_valid" in lib.last_error()
    assert _sample(V=70000, ldl=70000) == 1 and "65536" in lib.last_error()
    assert _sample(penalty=0.0) == 1
    assert _sample(u=None) == 1 and "uniforms" in lib.last_error()


# ------------------------------------------------------------------------------------------------ sampler restatement
@pytest.mark.parametrize("top_p", [1.0, 0.9, 0.5, 1e-6])
@pytest.mark.parametrize("temperature", [0.2, 0.7, 1.0])
def test_restatement_matches_the_installed_transformers_warpers(temperature, top_p):
    """kept set and renormalised probabilities of generate_case.sampler_probs64 = softmax of TemperatureLogitsWarper +
    TopPLogitsWarper of the installed transformers, on random rows (flat and peaked)"""
    for seed, scale in ((0, 1.0), (1, 2.5), (2, 4.0), (3, 0.3)):
        row = GC.peaked_row(512, seed, scale)
        p, edge = GC.sampler_probs64(row, temperature, top_p)
        if not edge > 1e-9:
            continue                                        # a nucleus edge on a tie decides nothing
        hf = GC.hf_warped_probs(row, temperature, top_p)
        assert np.array_equal(p > 0, hf > 0), (seed, scale)
        assert np.abs(p - hf).max() <= 1e-12
        assert abs(p.sum() - 1.0) <= 1e-12 and p[int(np.argmax(row))] > 0


def test_restatement_draw_and_penalty():
    p = np.array([0.0, 0.25, 0.0, 0.5, 0.25])
    tok, dist = GC.sampler_choice64(p, np.array([0.0, 0.2499, 0.25, 0.7499, 0.75, 0.999999]))
    assert tok.tolist() == [1, 1, 3, 3, 4, 4]
    assert np.allclose(dist, [0.25, 0.0001, 0.0, 0.0001, 0.0, 0.249999])
    x = GC.penalised(np.array([2.0, -2.0, 1.0, -1.0]), [0, 1, 1, 9, -3], 2.0)
    assert x.tolist() == [1.0, -4.0, 1.0, -1.0]
    sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
    import autocheck_case as AC
    row = torch.tensor(GC.peaked_row(64, 5, 2.0))
    assert np.allclose(GC.penalised(row.numpy(), [3, 9, 9], 1.3), AC.hf_repetition_penalty(row, [3, 9], 1.3).numpy())


# ------------------------------------------------------------------------------------------------ cache rows
def test_plan_decode_rows_ragged_prompts_times_repeat():
    from rlaif_v_amd.splice import IMAGE_TOKEN_INDEX, build_branch_plan, plan_decode_rows
    n_img, T, R = 6, 5, 3
    prompts = [torch.tensor([1, 7, IMAGE_TOKEN_INDEX, 9]), torch.tensor([1, IMAGE_TOKEN_INDEX, 4, 5, 6, 8, 3]),
               torch.tensor([1, 2, 3, IMAGE_TOKEN_INDEX])]
    plan = build_branch_plan([[p] for p in prompts], n_img, 256, pad_free=True, packed=False)
    lens = [p.numel() - 1 + n_img for p in prompts]                   # the placeholder expands to n_img rows
    assert plan.row_len.tolist() == lens and plan.row_off.tolist() == [0, lens[0], lens[0] + lens[1]]
    rows = plan_decode_rows(plan.row_off.tolist(), plan.row_len.tolist(), R, T)
    n_pre = sum(lens)
    assert rows.n_seq == 9 and rows.n_rows == n_pre + 9 * T
    assert rows.prompt_of.tolist() == [0, 0, 0, 1, 1, 1, 2, 2, 2]
    assert rows.pre_off.tolist() == [0] * 3 + [lens[0]] * 3 + [lens[0] + lens[1]] * 3     # one stored prompt per sample group
    assert rows.pre_len.tolist() == [lens[0]] * 3 + [lens[1]] * 3 + [lens[2]] * 3
    assert rows.own_off.tolist() == [n_pre + m * T for m in range(9)]
    assert rows.chunks == [(0, 9)]
    # brute force: every cache row has at most one owner, every sequence reads its prompt followed by its own tokens
    owner = {}
    for m in range(9):
        for j in range(T):
            pos, dst, own_len = rows.step(j)
            assert int(pos[m]) == lens[m // R] + j and int(own_len[m]) == j + 1
            r = int(dst[m])
            assert r >= n_pre and owner.setdefault(r, (m, j)) == (m, j)
            assert r == int(rows.own_off[m]) + j < rows.n_rows
    assert len(owner) == 9 * T
    for t in (rows.prompt_of, rows.pre_off, rows.pre_len, rows.own_off):
        assert t.dtype == torch.int32
    big = plan_decode_rows([0, 40], [40, 30], 70, 2)
    assert big.chunks == [(0, 64), (64, 128), (128, 140)] and big.n_rows == 70 + 140 * 2
    for bad in (dict(repeat=0), dict(max_new=0)):
        with pytest.raises(ValueError):
            plan_decode_rows([0], [4], **{**dict(repeat=1, max_new=1), **bad})
    with pytest.raises(ValueError):
        plan_decode_rows([0], [0], 1, 1)


# ------------------------------------------------------------------------------------------------ gen_data records
def _tok():
    sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden"))
    from toy_tokenizer import ToyTokenizer

    class Tok(ToyTokenizer):
        def decode(self, ids, skip_special_tokens=True):
            return " " + " ".join(f"t{int(i)}" for i in ids if not (skip_special_tokens and int(i) in (0, 1, 2))) + " "
    return Tok()


def test_generate_answers_records_on_a_stubbed_model():
    from rlaif_v_amd import gen_data
    calls = []

    def generate(prompts, images, max_new_tokens, repeat=1, temperature=0.0, top_p=1.0, repetition_penalty=1.0, eos_token_id=None,
                 generator=None, return_scores=False):
        calls.append(dict(n=len(prompts), max_new_tokens=max_new_tokens, repeat=repeat, temperature=temperature, eos=eos_token_id,
                          u=float(torch.rand(1, generator=generator))))
        assert all(int((p == -200).sum()) == 1 and int(p[0]) == 1 for p in prompts)
        return [[[10 * (len(calls) - 1) + 3 * k + r + 3, 2][:max_new_tokens] for r in range(repeat)] for k in range(len(prompts))]
    model = types.SimpleNamespace(cfg=types.SimpleNamespace(arch="llava", n_image_tokens=2), generate=generate)
    img = torch.zeros(3, 4, 4)
    items = [dict(question="What is shown ?", image=img, question_id="q0", metainfos={"ds_question_id": 70, "origin": "a"}),
             dict(question="Describe the scene .", image=img, metainfos={"origin": "b"}),
             dict(question="How many apples ?", image=img, question_id=12)]
    recs = gen_data.generate_answers(model, _tok(), items, repeat=3, temperature=0.7, max_tokens=8, seed=5, prompts_per_call=2,
                                     model_path="ckpt")
    assert [c["n"] for c in calls] == [2, 1] and all(c["repeat"] == 3 and c["max_new_tokens"] == 8 and c["eos"] == 2 for c in calls)
    assert calls[0]["u"] == float(torch.rand(1, generator=torch.Generator().manual_seed(5)))        # the seeded CPU generator
    assert len(recs) == 9
    assert [r["question_id"] for r in recs] == ["q0"] * 3 + [1] * 3 + [12] * 3             # the copies of an item in a row
    assert list(recs[0]) == ["question_id", "ds_question_id", "raw_question", "answer", "metainfos", "model_path"]
    assert list(recs[3]) == ["question_id", "raw_question", "answer", "metainfos", "model_path"]
    assert recs[0]["ds_question_id"] == 70 and recs[0]["metainfos"] == {"ds_question_id": 70, "origin": "a"} and recs[8]["metainfos"] == {}
    assert [r["answer"] for r in recs] == ["t3", "t4", "t5", "t6", "t7", "t8", "t13", "t14", "t15"]    # eos skipped, stripped
    assert all(r["model_path"] == "ckpt" for r in recs) and recs[4]["raw_question"] == "Describe the scene ."
    with pytest.raises(NotImplementedError):
        gen_data.generate_answers(types.SimpleNamespace(cfg=types.SimpleNamespace(arch="omnilmm")), _tok(), items)
    with pytest.raises(NotImplementedError):
        gen_data.main(["--checkpoint", "x", "--ds_name", "y", "--answer_file", "z", "--num_beam", "3"])
