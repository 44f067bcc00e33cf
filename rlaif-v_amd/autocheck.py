"""Yes / no feedback scoring: the labeler side of the AI-feedback stage that makes the preference pairs.

Mirrors (paths relative to the reference checkout) the ``--is_yesno`` branch of
  muffin/llava15_gen_data.py:266-333   (LLaVA-1.5 labeler, conv_llava_v1 prompts, ids from ``tokenizer.encode('<s> yes')[-1]``)
  omnilmm/omnilmm_gen_data.py:236-303  (OmniLMM labeler, Zephyr chat template, ids from
                                        ``tokenizer.encode('\\n<|assistant|>\\nyes')[-1]``)
started by script/data_gen/omnilmm/omnilmm_autocheck.sh: one short yes / no question per atomic claim of a candidate answer,
``generate(max_new_tokens=1, output_scores=True)`` per question, and the only things kept are softmax(scores[0]) at the ids
of ``yes`` / ``Yes`` / ``no`` / ``No`` and the greedy token.  That is one prefill per question: no cache, no decode loop.

Repetition penalty: omnilmm_gen_data.py:249-256 passes ``repetition_penalty=1.1``, but ``generate_vllm``
(omnilmm/model/omnilmm.py:371-396) hands ``generate`` the prompt as ``inputs_embeds`` only, so HF starts from an EMPTY id tensor
and RepetitionPenaltyLogitsProcessor has nothing to gather at the one step taken: ``scores[0]`` are the raw last-position logits.
llava15_gen_data.py sets no penalty.  The default here is therefore no penalty for both labelers; ``repetition_penalty=`` applies
HF's processor over each question's prompt ids (what ``generate(input_ids=..., repetition_penalty=...)`` does) on request.

The reference runs one full sequence (system prompt + image tokens + question) and one tower pass per question.  Here the
consecutive items that show the same image form a group: the tower runs once per image and the group's shared prefix once
(LlavaDPOModel.forward_next_token_scores, splice.build_branch_plan, rv_attn_fwd_branches, rv_next_token_scores).

Command line (the jsonl format of the reference's GenDataset in, one record per line out):
    python -m rlaif_v_amd.autocheck --checkpoint CKPT --ds_name questions.jsonl --answer_file out.jsonl --is_yesno
"""
from __future__ import annotations

import argparse
import base64
import io
import json
import os
from typing import Dict, List, Optional, Sequence

import torch

from .dataset import IMAGE_TOKEN_INDEX, llava_v1_prompt, tokenizer_image_token

DEFAULT_IMAGE_TOKEN = "<image>"
YESNO_KEYS = ("yes", "Yes", "no", "No")


def wrap_question_for_llava15(question: str, tokenizer, mm_use_im_start_end: bool = False) -> torch.Tensor:
    """llava15_gen_data.py:152-169 with conv_mode llava_v1: ``SYSTEM USER: <image>\\nquestion ASSISTANT:`` -> input ids."""
    qs = question.replace(DEFAULT_IMAGE_TOKEN, "")
    qs = ("<im_start>" + DEFAULT_IMAGE_TOKEN + "<im_end>" if mm_use_im_start_end else DEFAULT_IMAGE_TOKEN) + "\n" + qs
    prompt = llava_v1_prompt([{"from": "human", "value": qs}, {"from": "gpt", "value": None}])
    return tokenizer_image_token(prompt, tokenizer, IMAGE_TOKEN_INDEX, return_tensors="pt")


def yesno_ids(tokenizer, omnilmm: bool) -> List[int]:
    """The ids of yes / Yes / no / No as the reference takes them (llava15_gen_data.py:266-269, omnilmm_gen_data.py:236-239)."""
    lead = "\n<|assistant|>\n" if omnilmm else "<s> "
    return [int(tokenizer.encode(lead + w)[-1]) for w in YESNO_KEYS]


def _same_image(a, b) -> bool:
    if a is b:
        return True
    if torch.is_tensor(a) and torch.is_tensor(b):
        return a.shape == b.shape and a.dtype == b.dtype and bool(torch.equal(a, b))
    return False


def group_by_image(items: Sequence[Dict]) -> List[List[int]]:
    """Runs of consecutive items with the same image: the same ``image_id`` when both carry one, else the same image object
    or equal image tensors."""
    groups: List[List[int]] = []
    for i, it in enumerate(items):
        if groups:
            prev = items[groups[-1][0]]
            same = (it["image_id"] == prev["image_id"]) if ("image_id" in it and "image_id" in prev) \
                else _same_image(it["image"], prev["image"])
            if same:
                groups[-1].append(i)
                continue
        groups.append([i])
    return groups


def score_yesno(model, tokenizer, items: Sequence[Dict], packed: bool = True, repetition_penalty: Optional[float] = None,
                images_per_call: int = 8, model_path: Optional[str] = None, max_row_tokens: Optional[int] = None) -> List[Dict]:
    """``items``: dicts with ``question`` (text), ``image`` (what the model's ``encode_images`` takes for ONE image: a
    preprocessed [3, H, W] tensor or a raw uint8 [H, W, 3] image for LLaVA-1.5, tower tokens [N, width] or pixels for OmniLMM),
    optionally ``question_id`` (default: the item's index), ``image_id`` and ``metainfos``.  Returns one record per item, in
    input order, with the reference's keys: question_id, ds_question_id (when metainfos carries one), raw_question, answer (the
    decoded greedy token, stripped), scores {yes, Yes, no, No}, metainfos (and model_path when given).
    ``repetition_penalty``: None = what the reference's scores amount to for both labelers: no token is penalised (module
    docstring); a value penalises each question's own prompt ids, as HF does when ``generate`` is given ``input_ids``."""
    omnilmm = getattr(model.cfg, "arch", "llava") == "omnilmm"
    if repetition_penalty is None:
        repetition_penalty = 1.0
    if omnilmm:
        from .omni_data import wrap_question_for_omni_lmm

        def question_process(q):
            return torch.as_tensor(wrap_question_for_omni_lmm(q, model.cfg.n_image_tokens, tokenizer)["input_ids"])
    else:
        def question_process(q):
            return wrap_question_for_llava15(q, tokenizer, getattr(model.cfg, "mm_use_im_start_end", False))
    want = yesno_ids(tokenizer, omnilmm)
    groups = group_by_image(items)
    records: List[Dict] = []
    for g0 in range(0, len(groups), max(1, images_per_call)):
        chunk = groups[g0:g0 + max(1, images_per_call)]
        prompts = [[question_process(items[i]["question"]) for i in g] for g in chunk]
        images = [items[g[0]]["image"] for g in chunk]
        if all(torch.is_tensor(im) for im in images) and len({(im.shape, im.dtype) for im in images}) == 1 \
                and images[0].dtype != torch.uint8:
            images = torch.stack(images)
        probs, _, argmax, _ = model.forward_next_token_scores(prompts, images, want, packed=packed,
                                                              repetition_penalty=repetition_penalty,
                                                              max_row_tokens=max_row_tokens)
        probs, argmax = probs.cpu(), argmax.cpu()
        for n, i in enumerate(i for g in chunk for i in g):
            it = items[i]
            meta = it.get("metainfos", {})
            rec = {"question_id": it.get("question_id", i)}
            if "ds_question_id" in meta:
                rec["ds_question_id"] = meta["ds_question_id"]
            rec.update(raw_question=it["question"], answer=tokenizer.decode([int(argmax[n])], skip_special_tokens=True).strip(),
                       scores={k: float(probs[n, j]) for j, k in enumerate(YESNO_KEYS)}, metainfos=meta)
            if model_path is not None:
                rec["model_path"] = model_path
            records.append(rec)
    return records


def expand2square(img: torch.Tensor, background) -> torch.Tensor:
    """llava/mm_utils.py:152-163 on a raw uint8 [H, W, 3] image: pad the shorter side to a square with ``background``, the image
    centred ((longer - shorter) // 2 pixels in front of it)."""
    h, w = img.shape[:2]
    if h == w:
        return img
    n = max(h, w)
    out = torch.tensor(background, dtype=torch.uint8).expand(n, n, 3).clone()
    y0, x0 = ((n - h) // 2, 0) if w > h else (0, (n - w) // 2)
    out[y0:y0 + h, x0:x0 + w] = img
    return out


def read_gen_dataset(qa_file: str, start: int = 0, end: int = -1, image_aspect_ratio: Optional[str] = None) -> List[Dict]:
    """GenDataset (llava15_gen_data.py:64-147): a jsonl (or one-line json list, or json) file of {image | image_path |
    metainfos.image_path, question, question_id?, image_id?, ...}; everything but image_id / question / image is metainfos.
    Images come back as raw uint8 [H, W, 3] arrays (the device does CLIP's resize / crop / normalise).
    ``image_aspect_ratio`` = the checkpoint's config value, as the reference's collator honours it (process_images,
    llava/mm_utils.py:166-182): 'pad' (what LLaVA-1.5 checkpoints carry) squares the image with the processor's mean colour
    first; None / 'square' leaves it to the resize + centre crop; 'anyres' is not a LLaVA-1.5 mode and raises."""
    if image_aspect_ratio == "anyres":
        raise NotImplementedError("image_aspect_ratio='anyres' (LLaVA-NeXT grids) is not implemented")
    from .image import CLIP_MEAN
    background = tuple(int(x * 255) for x in CLIP_MEAN)
    import numpy as np
    from PIL import Image
    try:
        data = [json.loads(line) for line in open(qa_file)]
        if isinstance(data[0], list):
            data = data[0]
    except Exception:
        try:
            with open(qa_file) as f:
                data = json.load(f)
        except Exception:
            raise ValueError("Wrong input data format!")
    data = data[start:] if end < 0 or end > len(data) else data[start:end]
    items, last_key, last_img = [], None, None
    for idx, item in enumerate(data):
        if "image" in item:
            key = item["image"]
            src = io.BytesIO(base64.b64decode(key)) if len(key) > 100 else key
        elif "image_path" in item:
            key = src = item["image_path"]
        else:
            key = src = item["metainfos"]["image_path"]
        if key != last_key:                       # consecutive questions about one image share the decoded object
            last_key, last_img = key, torch.from_numpy(np.asarray(Image.open(src).convert("RGB")).copy())
            if image_aspect_ratio == "pad":
                last_img = expand2square(last_img, background)
        out = dict(question=item["question"], image=last_img, question_id=item.get("question_id", start + idx),
                   metainfos={k: v for k, v in item.items() if k not in ("image_id", "question", "image")})
        if "image_id" in item:
            out["image_id"] = item["image_id"]
        items.append(out)
    return items


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--checkpoint", type=str, required=True)
    ap.add_argument("--ds_name", type=str, required=True, help="question file in the jsonl format of the reference's GenDataset")
    ap.add_argument("--answer_file", type=str, required=True)
    ap.add_argument("--is_yesno", action="store_true", default=False)
    ap.add_argument("--start", "--start_pos", dest="start", type=int, default=0)
    ap.add_argument("--end", "--end_pos", dest="end", type=int, default=-1)
    ap.add_argument("--unpacked", action="store_true", help="one plain causal row per question (the comparison path)")
    args = ap.parse_args(argv)
    if not args.is_yesno:
        raise NotImplementedError("only --is_yesno (next-token scores) is implemented here: candidate answers come from "
                                  "python -m rlaif_v_amd.gen_data")
    import transformers
    from .checkpoint import from_pretrained
    model = from_pretrained(args.checkpoint, with_optimizer=False)
    tokenizer = transformers.AutoTokenizer.from_pretrained(args.checkpoint, use_fast=False)
    omnilmm = getattr(model.cfg, "arch", "llava") == "omnilmm"      # its collator applies the image transform alone
    with open(os.path.join(args.checkpoint, "config.json")) as f:
        aspect = None if omnilmm else json.load(f).get("image_aspect_ratio")
    items = read_gen_dataset(args.ds_name, args.start, args.end, image_aspect_ratio=aspect)
    records = score_yesno(model, tokenizer, items, packed=not args.unpacked, model_path=args.checkpoint)
    with open(args.answer_file, "w") as f:
        for rec in records:
            f.write(json.dumps(rec) + "\n")
    print(f"{len(records)} records -> {args.answer_file}")


if __name__ == "__main__":
    main()
