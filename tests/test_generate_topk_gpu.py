"""top_k through generate() on the GPU: the tiny LLaVA model of tests/golden/generate_tiny.pt (rv_sample_token_topk), the tiny
text model of tests/golden/text_generate_tiny.pt (the same sampler behind images=None) and a tiny text model with 66048 ids
(rv_sample_token_wide_topk), with planted uniforms and return_scores.  The fixtures are read only.

Every step's token must be what ops.sample_token[_wide](scores[j], ..., top_k=) gives alone on that step's logits, and the
float64 restatement's (tests/topk_case.py) wherever fp32 can decide it; top_k = 1 at temperature 0.7 is greedy; top_k = 0 is
the call without the keyword."""
import os
import sys

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import divide_case as DC  # noqa: E402
import generate_case as GC  # noqa: E402
import topk_case as TK  # noqa: E402
from oracle import dpo_oracle as O  # noqa: E402

_STATE = {}
WIDE_V = 66048
T_SAMPLE, TOP_P = 0.7, 0.9


def _model(name):
    """(model, prompts, images, steps, vocab): built once, shared, never modified"""
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    if name not in _STATE:
        if name == "llava":
            from rlaif_v_amd.model import LlavaConfig, LlavaDPOModel
            gold = GC.load_case()
            case, cfg = gold["mha"], O.tiny_cfg()
            model = LlavaDPOModel(LlavaConfig(**O.asdict(cfg)), with_optimizer=False)
            model.load_state_dict(O.make_weights(cfg, seed=case["seed"], std=gold["std"]))
            _STATE[name] = (model, case["prompts"], case["pixels"], gold["steps"], cfg.vocab)
        elif name == "text":
            gold = torch.load(DC.GOLD_TEXT, weights_only=True)
            W = DC.tiny_text_weights(1024, gold["seed"], gold["std"], gold["head_scale"])
            _STATE[name] = (DC.tiny_text_model(W, 1024), gold["prompts"], None, gold["steps"], 1024)
        else:
            W = DC.tiny_text_weights(WIDE_V, seed=5, std=0.05, head_scale=4.0)
            g = torch.Generator().manual_seed(9)
            prompts = [torch.cat([torch.tensor([1]), torch.randint(8, WIDE_V, (n,), generator=g)]) for n in (4, 11, 7)]
            _STATE[name] = (DC.tiny_text_model(W, WIDE_V), prompts, None, 6, WIDE_V)
    return _STATE[name]


def _uniforms(T, n, seed):
    return torch.rand(T, n, generator=torch.Generator().manual_seed(seed))


def _alone(ops, V, scores_j, u_j, top_k, **kw):
    fn = ops.sample_token if V <= ops.SAMPLE_REG_MAX_V else ops.sample_token_wide
    tok, _ = fn(scores_j.contiguous(), scores_j.shape[0], V, u_j.contiguous(), T_SAMPLE, TOP_P, top_k=top_k, **kw)
    return tok.cpu().tolist()


@pytest.mark.parametrize("name", ["llava", "text", "wide"])
def test_every_step_is_the_sampler_alone_and_the_restatement(name):
    from rlaif_v_amd import ops
    model, prompts, images, T, V = _model(name)
    n, top_k = len(prompts), 3
    U = _uniforms(T, n, seed=21)
    out, scores = model.generate(prompts, images, T, temperature=T_SAMPLE, top_p=TOP_P, top_k=top_k, _uniforms=U, return_scores=True)
    assert scores.shape[0] == T and all(len(out[k][0]) == T for k in range(n))
    bound, decided = V * TK.U32, 0
    for j in range(T):
        got = [out[k][0][j] for k in range(n)]
        assert got == _alone(ops, V, scores[j], U[j].to(scores.device), top_k), f"step {j}"
        for k in range(n):
            row = scores[j, k].cpu().numpy()
            p, edge, gap = TK.sampler_probs64_topk(row, T_SAMPLE, TOP_P, top_k)
            want, dist = GC.sampler_choice64(p, np.asarray([np.float32(U[j, k])], dtype=np.float64))
            if edge > 4 * bound and gap > TK.GAP_MIN and dist[0] > bound:
                decided += 1
                assert got[k] == int(want[0]), f"step {j} prompt {k}: token {got[k]}, the restatement draws {int(want[0])}"
            if gap > TK.GAP_MIN:
                assert row[got[k]] >= np.sort(row)[-top_k], f"step {j} prompt {k}: token {got[k]} is not among the top {top_k}"
    print(f"[{name}] top_k={top_k}: {decided} of {T * n} draws decidable in float64")
    assert decided >= (T * n) // 2, "too few decidable draws: pick other uniforms"


@pytest.mark.parametrize("name", ["llava", "text", "wide"])
def test_top_k_1_is_greedy_and_top_k_0_is_the_call_without_it(name):
    from rlaif_v_amd import ops
    model, prompts, images, T, V = _model(name)
    n = len(prompts)
    U = _uniforms(T, n, seed=22)
    greedy = model.generate(prompts, images, T)
    assert model.generate(prompts, images, T, temperature=T_SAMPLE, top_k=1, _uniforms=U) == greedy
    assert model.generate(prompts, images, T, temperature=T_SAMPLE, top_p=0.5, top_k=1, _uniforms=U) == greedy
    before, s0 = model.generate(prompts, images, T, temperature=T_SAMPLE, top_p=TOP_P, _uniforms=U, return_scores=True)
    off, s1 = model.generate(prompts, images, T, temperature=T_SAMPLE, top_p=TOP_P, top_k=0, _uniforms=U, return_scores=True)
    assert off == before and torch.equal(s0, s1)
    for j in range(T):                                        # and both are the base entry point on that step's logits
        assert [off[k][0][j] for k in range(n)] == _alone(ops, V, s1[j], U[j].to(s1.device), 0), f"step {j}"
    big = model.generate(prompts, images, T, temperature=T_SAMPLE, top_p=TOP_P, top_k=V + 5, _uniforms=U)
    assert big == before, "top_k >= the vocabulary is off"


def test_generate_refuses_a_negative_top_k():
    model, prompts, images, T, _ = _model("text")
    with pytest.raises(ValueError, match="top_k"):
        model.generate(prompts, images, T, temperature=T_SAMPLE, top_k=-1)
