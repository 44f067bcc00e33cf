"""Generate tests/golden/autocheck_tiny.pt by executing the REFERENCE ITSELF (the read-only checkout make_golden.py puts on sys.path) on CPU: the
yes / no feedback stage of muffin/llava15_gen_data.py:280-313 on the tiny configuration.

Run where the reference checkout exists (the build container; the GPU box has none):

    python tests/golden/make_autocheck_golden.py

What runs: the reference's ``LlavaLlamaForCausalLM`` (built as in make_golden.py, weights from
``oracle.dpo_oracle.make_weights``) and, per question, its own
``generate(inputs, images, image_sizes, do_sample=False, num_beams=1, max_new_tokens=1, use_cache=True, output_scores=True,
return_dict_in_generate=True)``; then ``softmax(scores[0])`` at the four wanted ids and the new token, exactly as the
script reads them.  The reference model's last-position forward logits (prepare_inputs_labels_for_multimodal + forward, the
two calls make_golden.py uses) are stored next to them: for greedy decoding without logits processors ``scores[0]`` IS that
row, and the script asserts it.  If ``generate`` cannot run under the installed transformers (the reference pins 4.35), the
forward logits alone are stored and ``generate_ran`` is False.

The fixture is data only: the pixel tensors, the prompts (input ids with the -200 image placeholder), the wanted ids, the
weight recipe (seed, std) and the recorded results.
"""
import os
import sys

import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)

from make_golden import O, build_reference_model  # noqa: E402  (sets up sys.path, the wandb stub and the reference imports)

IMAGE_TOKEN_INDEX = -200
SEED, STD = 23, 0.04
WANT = [17, 101, 250, 399]                 # stand-ins for the ids of yes / Yes / no / No in the 512-token toy vocabulary
N_QUESTIONS = [1, 4, 7]
TAILS = [[9], [44, 51, 39, 48], [55, 42, 49, 38, 53, 46, 41]]


def make_case(cfg):
    """Three images with 1, 4 and 7 questions: [bos, system.., <image>, shared question words.., own tail..]."""
    g = torch.Generator().manual_seed(SEED)
    pixels = torch.randn(len(N_QUESTIONS), 3, cfg.image_size, cfg.image_size, generator=g)
    prompts = []
    for k, tails in enumerate(TAILS):
        head = torch.cat([torch.tensor([1]), torch.randint(3, cfg.vocab, (5 + k,), generator=g)])
        shared = torch.randint(3, cfg.vocab, (3,), generator=g)
        prompts.append([torch.cat([head, torch.tensor([IMAGE_TOKEN_INDEX]), shared, torch.randint(3, cfg.vocab, (t,), generator=g)])
                        for t in tails])
    return pixels, prompts


def main():
    torch.set_num_threads(8)
    torch.manual_seed(0)
    cfg = O.tiny_cfg()
    W = O.make_weights(cfg, seed=SEED, std=STD)
    model = build_reference_model(cfg, {k: v.clone() for k, v in W.items()})
    model.eval()
    pixels, prompts = make_case(cfg)
    probs, tokens, logits_last, generate_ran = [], [], [], True
    with torch.no_grad():
        for k, plist in enumerate(prompts):
            for ids in plist:
                (_, _, _, _, emb, _) = model.prepare_inputs_labels_for_multimodal(
                    input_ids=ids[None], position_ids=None, attention_mask=None, past_key_values=None, labels=None,
                    images=pixels[k:k + 1])
                fwd = model.forward(inputs_embeds=emb, labels=None).logits[0, -1].float()
                logits_last.append(fwd)
                scores = fwd
                if generate_ran:
                    try:
                        out = model.generate(inputs=ids[None], images=pixels[k:k + 1], image_sizes=[(cfg.image_size, cfg.image_size)],
                                             do_sample=False, num_beams=1, max_new_tokens=1, use_cache=True, output_scores=True,
                                             return_dict_in_generate=True)
                        scores = out.scores[0][0].float()
                        assert torch.allclose(scores, fwd, atol=1e-5, rtol=1e-5), float((scores - fwd).abs().max())
                        assert int(out.sequences[0, -1]) == int(scores.argmax())
                    except AssertionError:
                        raise
                    except Exception as e:                      # noqa: BLE001
                        print("generate() does not run under the installed transformers:", type(e).__name__, str(e)[:300])
                        generate_ran = False
                        scores = fwd
                sm = torch.softmax(scores, 0)
                probs.append(sm[WANT].clone())
                tokens.append(int(sm.argmax()))
    out = dict(cfg=O.asdict(cfg), seed=SEED, std=STD, want_ids=WANT, pixels=pixels, prompts=prompts,
               probs=torch.stack(probs), new_token=torch.tensor(tokens), logits_last=torch.stack(logits_last),
               generate_ran=generate_ran)
    path = os.path.join(HERE, "autocheck_tiny.pt")
    torch.save(out, path)
    print("generate_ran", generate_ran, "probs", out["probs"][:3].tolist(), "->", path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
