"""Shared pieces of the yes / no feedback scoring tests (tests/test_autocheck_host.py, tests/test_autocheck_gpu.py): the case
stored in tests/golden/autocheck_tiny.pt (three images with 1, 4 and 7 questions, written by make_autocheck_golden.py next to
what the reference's own ``generate`` returned for it) and the CPU oracle of one question = ``oracle.dpo_oracle.llama_logits``
on its stand-alone spliced sequence, log-softmax at the last position, fp32."""
import os

import torch
import torch.nn.functional as F

from oracle import dpo_oracle as O
from oracle import omnilmm_oracle as OO

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "autocheck_tiny.pt")
OMNI_TOKENS = (322, 323, 324)            # <im_patch>, <im_start>, <im_end> of the tiny OmniLMM configuration
OMNI_NQ, OMNI_KV, OMNI_RS_HEADS = 16, 192, 4


def load_case():
    return torch.load(GOLD, weights_only=True)


def load_omni_case():
    """tests/golden/autocheck_omnilmm_tiny.pt (make_autocheck_omnilmm_golden.py): the reference OmniLMM model's scores for
    1 + 4 + 7 questions about three images, from its stand-in tower's tokens on."""
    return torch.load(GOLD.replace("autocheck_tiny", "autocheck_omnilmm_tiny"), weights_only=True)


def n_prefix(k):
    """Length of the spliced shared prefix of image k of the stored case: bos + (5 + k) words + 16 image tokens + 3 words."""
    return 1 + 5 + k + 16 + 3


def question_embeds(cfg, W, prompts, pixels):
    """Per image, per question: the stand-alone spliced input embeddings [1, L, d] (fp32)."""
    feats = O.encode_images(pixels, W, cfg)
    emb_w = W["model.embed_tokens.weight"]
    return [[O.prepare_inputs_labels_for_multimodal(p[None], torch.full_like(p[None], -100), feats[k:k + 1], emb_w, None)[0]
             for p in plist] for k, plist in enumerate(prompts)]


def oracle_logits(cfg, W, embeds):
    """[n_q, V] last-position logits, questions in input order."""
    with torch.no_grad():
        return torch.stack([O.llama_logits(e, W, cfg)[0, -1] for img in embeds for e in img])


def leaked_logits(cfg, W, embeds):
    """The same questions under a WRONG mask: every question of a multi-question image also sees the tail of the question
    packed in front of it (the first one: the last one's), every token keeping its own position - what a branch mask that
    starts one branch too early computes.  [n_multi, V] and the indices of those questions."""
    out, idx, n = [], [], 0
    with torch.no_grad():
        for k, img in enumerate(embeds):
            sh = n_prefix(k)
            for i, e in enumerate(img):
                if len(img) > 1:
                    other = img[(i - 1) % len(img)][:, sh:]
                    x = torch.cat([e[:, :sh], other, e[:, sh:]], 1)
                    pos = torch.cat([torch.arange(sh), torch.arange(sh, sh + other.shape[1]), torch.arange(sh, e.shape[1])])
                    cos, sin = O.rope_tables(int(pos.max()) + 1, cfg.head_dim, cfg.rope_theta, x.dtype)
                    mask = torch.full((x.shape[1], x.shape[1]), float("-inf")).triu(1)
                    for layer in range(cfg.layers):
                        x = O.llama_layer(x, W, cfg, layer, cos[pos], sin[pos], mask)
                    h = O.rms_norm(x, W["model.norm.weight"], cfg.rms_eps)
                    out.append(F.linear(h, W["lm_head.weight"]).float()[0, -1])
                    idx.append(n)
                n += 1
    return torch.stack(out), idx


def hf_repetition_penalty(logits, prompt_ids, penalty):
    """transformers RepetitionPenaltyLogitsProcessor.__call__ restated: score = gather(scores, input_ids);
    score = where(score < 0, score * penalty, score / penalty); scores.scatter(input_ids, score).  One row."""
    ids = torch.as_tensor(prompt_ids).long()
    score = logits[ids]
    out = logits.clone()
    out[ids] = torch.where(score < 0, score * penalty, score / penalty)
    return out


# ------------------------------------------------------------------------------------------------ OmniLMM
def omni_cfgs():
    from rlaif_v_amd.omnilmm import OmniLMMConfig
    pt, st, en = OMNI_TOKENS
    cfg = OmniLMMConfig(hidden=512, layers=2, heads=4, kv_heads=2, ffn=768, vocab=325, model_max_length=256, num_query=OMNI_NQ,
                        vision_width=OMNI_KV, image_size=84, im_patch_token=pt, im_start_token=st, im_end_token=en)
    ocfg = O.LlavaCfg(hidden=512, layers=2, heads=4, kv_heads=2, ffn=768, vocab=325, model_max_length=256)
    return cfg, ocfg


def omni_weights(ocfg, std):
    W = {k: v for k, v in O.make_weights(ocfg, seed=3, std=std).items() if "vision_tower" not in k and "mm_projector" not in k}
    W.update(OO.make_resampler_weights(512, OMNI_KV, OMNI_NQ))
    return W


def omni_case(ocfg, seed=31):
    """Tower tokens [3, 36, width] and prompts [bos, words.., <im_start>, <im_patch> x nq, <im_end>, shared.., tail..] with
    1, 4 and 7 questions; text ids stay below the three image tokens."""
    pt, st, en = OMNI_TOKENS
    g = torch.Generator().manual_seed(seed)
    tower = torch.randn(3, 36, OMNI_KV, generator=g).bfloat16().float()
    prompts = []
    for k, tails in enumerate([[9], [14, 21, 9, 18], [25, 12, 19, 8, 23, 16, 11]]):
        head = torch.cat([torch.tensor([1]), torch.randint(3, pt, (4 + k,), generator=g)])
        img = torch.tensor([st] + [pt] * OMNI_NQ + [en])
        shared = torch.randint(3, pt, (3,), generator=g)
        prompts.append([torch.cat([head, img, shared, torch.randint(3, pt, (t,), generator=g)]) for t in tails])
    return tower, prompts


def omni_oracle_logits(ocfg, W, tower, prompts):
    with torch.no_grad():
        feats = OO.resampler_forward(tower, W, OMNI_RS_HEADS)
        rows = []
        for k, plist in enumerate(prompts):
            for p in plist:
                emb = OO.omnilmm_splice(p[None], W["model.embed_tokens.weight"], feats[k:k + 1], *OMNI_TOKENS)
                rows.append(O.llama_logits(emb, W, ocfg)[0, -1])
    return torch.stack(rows)
