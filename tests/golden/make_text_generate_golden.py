"""Record tests/golden/text_generate_tiny.pt with the installed transformers' own ``LlamaForCausalLM.generate`` on the CPU (fp32):
greedy decoding of a LEFT-PADDED batch of three prompts of different lengths - what the text-generation pipeline of the
reference's utils/llama3_8b_inference.py feeds its models - once without an end-of-sequence id (12 steps each: the sequences the
tests teacher-force, with the logits of every step and their top-1 / top-2 gaps) and once with TWO end-of-sequence ids chosen
from those sequences, so that two prompts stop at different ids at different steps and the third runs on.

    python tests/golden/make_text_generate_golden.py

The tiny model: hidden 256, 2 heads of 128, 1 kv head, 2 layers, ffn 512, rope_theta 500000, vocabulary 1024.  Its weights are
tests/divide_case.tiny_text_weights(1024, seed, STD, HEAD_SCALE): the fixture stores that recipe, not the tensors (3.4 MB), and
this script checks that ``oracle.dpo_oracle.llama_logits`` on those weights reproduces the HF model's logits to 1e-4 before it
records anything.  The seed is the one of SEEDS with the largest smallest gap over the steps of the run with two EOS ids (the
steps a greedy comparison looks at); it must exceed 2 x GAP_BAR.  Data only."""
import os
import sys

import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))

import divide_case as DC  # noqa: E402
from oracle import dpo_oracle as O  # noqa: E402

VOCAB, STEPS, STD, HEAD_SCALE = 1024, 12, 0.05, 4.0
SEEDS = range(300)
GAP_BAR = 0.08          # the no-cache bf16 forward's logit error at this logit scale (|logit| up to 14), measured on an MI355X: 0.077
PAD = 0
LENS = (5, 9, 14)


def hf_model(W):
    import transformers
    cfg = transformers.LlamaConfig(hidden_size=DC.TINY["hidden"], intermediate_size=DC.TINY["ffn"], num_hidden_layers=DC.TINY["layers"],
                                   num_attention_heads=DC.TINY["heads"], num_key_value_heads=DC.TINY["kv_heads"], vocab_size=VOCAB,
                                   rms_norm_eps=DC.TINY["rms_eps"], rope_theta=DC.TINY["rope_theta"], max_position_embeddings=2048,
                                   tie_word_embeddings=False, attention_bias=False, pad_token_id=PAD, bos_token_id=1, eos_token_id=2)
    model = transformers.LlamaForCausalLM(cfg).float().eval()
    missing, unexpected = model.load_state_dict(W, strict=False)
    assert not unexpected and all("rotary" in k or "inv_freq" in k for k in missing), (missing, unexpected)
    return model


def make_prompts(seed):
    g = torch.Generator().manual_seed(1000 + seed)
    return [torch.cat([torch.tensor([1]), torch.randint(8, VOCAB, (n - 1,), generator=g)]) for n in LENS]


def left_padded(prompts):
    L = max(p.numel() for p in prompts)
    ids = torch.full((len(prompts), L), PAD, dtype=torch.long)
    mask = torch.zeros(len(prompts), L, dtype=torch.long)
    for k, p in enumerate(prompts):
        ids[k, L - p.numel():] = p
        mask[k, L - p.numel():] = 1
    return ids, mask


def generate(model, prompts, eos):
    ids, mask = left_padded(prompts)
    with torch.no_grad():
        out = model.generate(input_ids=ids, attention_mask=mask, do_sample=False, num_beams=1, max_new_tokens=STEPS, use_cache=True,
                             eos_token_id=eos, pad_token_id=PAD, output_logits=True, return_dict_in_generate=True)
    return out.sequences[:, ids.shape[1]:], torch.stack(out.logits, 1).float()                # [3, <= T], [3, <= T, V]


def pick_eos(free):
    """two ids: the first stops prompt 0 mid-way, the second prompt 1 at a later step; neither occurs earlier anywhere"""
    seqs = free.tolist()
    for j0 in range(3, STEPS - 4):
        e1 = seqs[0][j0]
        if e1 in seqs[0][:j0]:
            continue
        for j1 in range(j0 + 2, STEPS - 1):
            e2 = seqs[1][j1]
            if e2 == e1 or e2 in seqs[1][:j1] or e1 in seqs[1][:j1] or e2 in seqs[0][:j0] or e1 in seqs[2] or e2 in seqs[2]:
                continue
            return (e1, e2), (j0, j1)
    return None, None


def main():
    ocfg = O.LlavaCfg(vocab=VOCAB, **DC.TINY)
    best = None
    for seed in SEEDS:
        W = DC.tiny_text_weights(VOCAB, seed, STD, HEAD_SCALE)
        prompts = make_prompts(seed)
        free, logits = generate(hf_model(W), prompts, None)
        top2 = logits.topk(2, -1).values
        gaps = top2[..., 0] - top2[..., 1]
        eos, at = pick_eos(free)
        if eos is None:
            continue
        used = min(float(gaps[0, :at[0] + 1].min()), float(gaps[1, :at[1] + 1].min()), float(gaps[2].min()))
        print("seed", seed, "min gap %.4f" % float(gaps.min()), "over the compared steps %.4f" % used, "eos", eos, at, flush=True)
        if best is None or used > best[0]:
            best = (used, seed)
    assert best is not None and best[0] > 2 * GAP_BAR, best
    seed = best[1]
    W = DC.tiny_text_weights(VOCAB, seed, STD, HEAD_SCALE)
    prompts = make_prompts(seed)
    model = hf_model(W)
    free, logits = generate(model, prompts, None)
    assert free.shape == (3, STEPS)
    top2 = logits.topk(2, -1).values
    gaps = top2[..., 0] - top2[..., 1]
    eos, at = pick_eos(free)
    cut, _ = generate(model, prompts, list(eos))
    sequences = []
    for k in range(3):
        seq = cut[k].tolist()
        stop = [j for j, t in enumerate(seq) if t in eos]
        sequences.append(seq[:stop[0] + 1] if stop else seq)
    assert len(sequences[0]) == at[0] + 1 and len(sequences[1]) == at[1] + 1 and len(sequences[2]) == STEPS
    assert sequences[0][-1] == eos[0] and sequences[1][-1] == eos[1]
    assert all(sequences[k] == free[k].tolist()[:len(sequences[k])] for k in range(3))
    # the oracle on prompt + tokens so far against HF's per-step logits
    worst = 0.0
    with torch.no_grad():
        for k, p in enumerate(prompts):
            ids = torch.cat([p, free[k, :STEPS - 1]])
            lg = O.llama_logits(W["model.embed_tokens.weight"][ids][None], W, ocfg)[0]
            worst = max(worst, float((lg[p.numel() - 1:] - logits[k]).abs().max()))
    print("oracle against LlamaForCausalLM.generate logits: max abs diff %.3e, |logit| max %.2f" % (worst, float(logits.abs().max())))
    assert worst <= 1e-4
    compared = min(float(gaps[k, :len(sequences[k])].min()) for k in range(3))
    out = dict(min_compared_gap=compared, cfg=dict(DC.TINY, vocab=VOCAB), seed=seed, std=STD, head_scale=HEAD_SCALE, steps=STEPS, gap_bar=GAP_BAR, pad=PAD,
               prompts=prompts, eos_ids=list(eos), eos_steps=list(at), free_sequences=free.to(torch.int32), scores=logits,
               gaps=gaps, sequences=sequences, oracle_vs_hf=worst)
    path = os.path.join(HERE, "text_generate_tiny.pt")
    torch.save(out, path)
    print("seed", seed, "eos", eos, "at", at, "min gap %.4f" % float(gaps.min()), "->", path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
