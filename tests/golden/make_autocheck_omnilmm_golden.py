"""Generate tests/golden/autocheck_omnilmm_tiny.pt by executing the REFERENCE ITSELF on CPU: the yes / no feedback stage of
omnilmm/omnilmm_gen_data.py:248-282 on the tiny OmniLMM configuration of make_omnilmm_golden.py (its stand-in tower and stubs).

Run where the reference checkout exists (the build container; the GPU box has none):

    python tests/golden/make_autocheck_omnilmm_golden.py

What runs, per question: the reference's own ``OmniLMMForCausalLM.generate_vllm(input_ids, images, max_new_tokens=1,
num_beams=1, return_dict_in_generate=True, repetition_penalty=1.1, output_scores=True)``, then ``softmax(scores[0])`` at the
four wanted ids and the new token, as the script reads them.  ``generate_vllm`` turns the prompt into ``inputs_embeds`` and
calls ``generate`` WITHOUT input ids (omnilmm/model/omnilmm.py:371-396), so the repetition penalty has no token to act on at
the one step taken and ``scores[0]`` are the model's raw last-position logits; where ``generate_vllm`` runs, the script
asserts that.  A prompt of the first image contains a wanted id, so a penalty over the prompt ids would show.

Under the installed transformers (the reference pins 4.35) ``generate_vllm`` does NOT run: the reference's
``prepare_inputs_for_generation`` (omnilmm.py:349-369) tests ``past_key_values is None``, today's ``generate`` hands it an empty
cache object instead, and the model is called with the EMPTY [1, 0] id tensor ``generate`` started from - which is itself the
point above.  As for the LLaVA fixture, the reference model's last-position forward logits are stored instead
(``get_vllm_embedding`` + ``forward(inputs_embeds=)``, the two calls ``generate_vllm`` makes), and ``generate_ran`` is False.

The fixture is data only: the stand-in tower's tokens for three images, the prompts, the wanted ids, the weight recipe and the
recorded results.
"""
import os
import sys

import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)

import make_omnilmm_golden as MG  # noqa: E402  (installs the stubs, sets up sys.path and imports the reference classes)

O, OO = MG.O, MG.OO
SEED, STD = 31, 0.04
WANT = [17, 101, 250, 300]
TAILS = [[9], [14, 21, 9, 18], [25, 12, 19, 8, 23, 16, 11]]


def make_prompts():
    pt, st, en = MG.TOKENS
    g = torch.Generator().manual_seed(SEED)
    prompts = []
    for k, tails in enumerate(TAILS):
        head = torch.cat([torch.tensor([1]), torch.randint(3, pt, (4 + k,), generator=g)])
        img = torch.tensor([st] + [pt] * MG.NUM_QUERY + [en])
        shared = torch.randint(3, pt, (3,), generator=g)
        prompts.append([torch.cat([head, img, shared, torch.randint(3, pt, (t,), generator=g)]) for t in tails])
    prompts[0][0][2] = WANT[0]                     # a wanted id inside a prompt
    return prompts, torch.randn(len(TAILS), 3, MG.IMG, MG.IMG, generator=g)


def main():
    torch.set_num_threads(8)
    torch.manual_seed(0)
    cfg = MG.tiny_cfg()
    ocfg = MG.OmniLMMConfig(hidden_size=cfg.hidden, intermediate_size=cfg.ffn, num_hidden_layers=cfg.layers,
                            num_attention_heads=cfg.heads, num_key_value_heads=cfg.n_kv_heads, vocab_size=cfg.vocab,
                            rms_norm_eps=cfg.rms_eps, rope_theta=cfg.rope_theta, max_position_embeddings=4096,
                            sliding_window=None, pad_token_id=None, attn_implementation="eager",
                            mm_vision_tower="stub", num_query=MG.NUM_QUERY, image_size=MG.IMG)
    model = MG.OmniLMMForCausalLM(ocfg).float()
    W = {k: v for k, v in O.make_weights(cfg, seed=3, std=STD).items() if "vision_tower" not in k and "mm_projector" not in k}
    W.update(OO.make_resampler_weights(cfg.hidden, MG.KV_DIM, MG.NUM_QUERY))
    missing, unexpected = model.load_state_dict(dict(W), strict=False)
    assert not unexpected, unexpected
    assert all(("vision_tower" in m) or m.endswith("resampler.pos_embed") for m in missing), missing
    vc = model.model.vision_config
    vc.im_patch_token, vc.im_start_token, vc.im_end_token = MG.TOKENS
    vc.use_im_start_end = True
    model.eval()
    prompts, images = make_prompts()
    probs, tokens, logits_last, generate_ran = [], [], [], True
    with torch.no_grad():
        tower = model.model.vision_tower.forward_features(images)[:, 1:]
        for k, plist in enumerate(prompts):
            for ids in plist:
                emb, _ = model.model.get_vllm_embedding({"input_ids": ids[None], "pixel_values": images[k:k + 1]})
                fwd = model(inputs_embeds=emb).logits[0, -1].float()
                scores = fwd
                if generate_ran:
                    try:
                        out = model.generate_vllm(input_ids=ids[None], images=images[k:k + 1], max_new_tokens=1, num_beams=1,
                                                  return_dict_in_generate=True, repetition_penalty=1.1, output_scores=True)
                        scores = out.scores[0][0].float()
                        assert torch.allclose(scores, fwd, atol=1e-5, rtol=1e-5), float((scores - fwd).abs().max())
                        assert int(out.sequences[0, -1]) == int(scores.argmax())
                    except AssertionError:
                        raise
                    except Exception as e:                      # noqa: BLE001
                        print("generate_vllm() does not run under the installed transformers:", type(e).__name__, str(e)[:200])
                        generate_ran = False
                        scores = fwd
                logits_last.append(fwd)
                sm = torch.softmax(scores, 0)
                probs.append(sm[WANT].clone())
                tokens.append(int(sm.argmax()))
    out = dict(cfg=O.asdict(cfg), weight_seed=3, std=STD, want_ids=WANT, tokens=list(MG.TOKENS), num_query=MG.NUM_QUERY,
               kv_dim=MG.KV_DIM, tower=tower.clone(), prompts=prompts, probs=torch.stack(probs), new_token=torch.tensor(tokens),
               logits_last=torch.stack(logits_last), penalty_passed=1.1,
               generate_ran=generate_ran)
    path = os.path.join(HERE, "autocheck_omnilmm_tiny.pt")
    torch.save(out, path)
    print("generate_ran", generate_ran, "probs", out["probs"][:2].tolist(), "->", path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
