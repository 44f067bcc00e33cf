"""Answer files for the evaluation stage: one answer per question, by beam search, in the reference's record format.

Mirrors (paths relative to the reference checkout) the answer-file stage of
  muffin/eval/muffin_vqa.py:31-95        (Object-HalBench / MMHal: script/eval/eval_rlaifv_objhal.sh, eval_rlaifv_mmhal.sh run it
                                          with ``--temperature 0 --num_beam 3``)
  muffin/eval/llava15_chair.py           (the same loop with its own defaults)
which call ``model.generate(do_sample=temperature > 0, num_beams=3, max_new_tokens=1024, use_cache=True)`` once per question.
Here ``num_beams > 1`` is LlavaDPOModel.beam_search (rv_attn_decode_indexed, rv_beam_topk, rv_beam_step) and ``num_beams == 1``
the existing LlavaDPOModel.generate (greedy at temperature 0, else sampling).  Beams with ``temperature > 0`` is HF's
beam-sample mode; it is not implemented and refused by name.  The GPT-4 scoring half of the evaluation scripts is not part of
this project.

Sampling (``--num_beams 1 --temperature > 0``): ``--top_k`` is HF's TopKLogitsWarper (0 = off, the default).  ``--hf_defaults``
takes every sampling parameter that is not on the command line from the checkpoint's generation_config.json, else from
transformers 4.35's defaults (top_k = 50) - what a reference ``generate`` call that leaves them unsaid runs with
(genconfig.resolve_sampling); without it nothing changes.  It concerns ``--num_beams 1`` alone: beam search samples nothing, so with
``--num_beams > 1`` nothing is resolved.

Question lines carry ``question`` and a base64 ``image`` or an ``image_path`` (autocheck.read_gen_dataset decodes them and
applies the checkpoint's image_aspect_ratio).  Records: question_id (the running index), image_id (the line's ``image_id``, else
its ``image_url``), prompt (the question as given), text (the decoded new tokens, special tokens skipped, stripped), model_id.

Command line (``--num_beam``, as the evaluation scripts spell it, is accepted through argparse's prefix matching):
    python -m rlaif_v_amd.vqa --model-path CKPT --question-file q.jsonl --answers-file a.jsonl --temperature 0 --num_beam 3
"""
from __future__ import annotations

import argparse
import json
import math
import os
from typing import Dict, List, Optional, Sequence

import torch

from .autocheck import read_gen_dataset, wrap_question_for_llava15
from .genconfig import StoreGiven, cli_sampling, given_on_command_line

DEFAULTS = {"temperature": 0.2, "top_p": 1.0, "top_k": 0, "repetition_penalty": 1.0}     # without --hf_defaults

MODEL_ID = "llava-v1.5-7b"          # muffin_vqa.py:35 writes this name whatever the checkpoint


def get_chunk(lst: Sequence, n: int, k: int):
    """muffin_vqa.py:20-28: chunk k of n (roughly) equal chunks"""
    size = math.ceil(len(lst) / n)
    return [lst[i:i + size] for i in range(0, len(lst), size)][k]


def answer_questions(model, tokenizer, lines: Sequence[Dict], num_beams: int = 3, temperature: float = 0.0,
                     top_p: Optional[float] = None, max_new_tokens: int = 1024, prompts_per_call: int = 4, seed: Optional[int] = 0,
                     model_id: str = MODEL_ID, length_penalty: float = 1.0, top_k: int = 0,
                     repetition_penalty: float = 1.0) -> List[Dict]:
    """``lines``: dicts with ``question``, ``image`` (what ``encode_images`` takes for ONE image) and ``image_id`` or
    ``image_url`` (read_gen_dataset keeps ``image_url`` under ``metainfos``).  ``prompts_per_call`` questions share one call;
    an answer does not depend on the questions next to it."""
    if getattr(model.cfg, "arch", "llava") == "omnilmm":
        raise NotImplementedError("vqa: OmniLMM generation is not implemented (LlavaDPOModel.beam_search is LLaVA-1.5 only)")
    if num_beams < 1:
        raise ValueError("vqa: num_beams must be >= 1")
    if num_beams > 1 and temperature > 0:
        raise NotImplementedError("vqa: num_beams > 1 with temperature > 0 is HF's beam-sample mode, which is not implemented - "
                                  "pass --temperature 0 (as the evaluation scripts do)")
    eos = getattr(tokenizer, "eos_token_id", None)
    mm = getattr(model.cfg, "mm_use_im_start_end", False)
    gen = torch.Generator().manual_seed(int(seed)) if seed is not None else None
    records: List[Dict] = []
    step = max(1, prompts_per_call)
    for i0 in range(0, len(lines), step):
        chunk = lines[i0:i0 + step]
        prompts = [wrap_question_for_llava15(it["question"], tokenizer, mm) for it in chunk]
        images = [it["image"] for it in chunk]
        if all(torch.is_tensor(im) for im in images) and len({(im.shape, im.dtype) for im in images}) == 1 \
                and images[0].dtype != torch.uint8:
            images = torch.stack(images)
        if num_beams > 1:
            answers, _ = model.beam_search(prompts, images, max_new_tokens=max_new_tokens, num_beams=num_beams, eos_token_id=eos,
                                           length_penalty=length_penalty)
        else:
            extra = {}                                        # the call of before when neither is asked for
            if top_k:
                extra["top_k"] = int(top_k)
            if repetition_penalty != 1.0:
                extra["repetition_penalty"] = float(repetition_penalty)
            out = model.generate(prompts, images, max_new_tokens=max_new_tokens, repeat=1, temperature=temperature,
                                 top_p=1.0 if top_p is None else top_p, eos_token_id=eos, generator=gen, **extra)
            answers = [o[0] for o in out]
        for n, it in enumerate(chunk):
            image_id = it["image_id"] if "image_id" in it else it.get("image_url", it.get("metainfos", {}).get("image_url"))
            records.append({"question_id": i0 + n, "image_id": image_id, "prompt": it["question"],
                            "text": tokenizer.decode(answers[n], skip_special_tokens=True).strip(), "model_id": model_id})
    return records


def build_parser() -> argparse.ArgumentParser:
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])        # allow_abbrev stays on: --num_beam means --num_beams
    ap.add_argument("--model-path", type=str, required=True)
    ap.add_argument("--model-base", type=str, default=None, help="accepted for the reference's command lines; unused")
    ap.add_argument("--image-folder", type=str, default="", help="accepted for the reference's command lines; unused")
    ap.add_argument("--question-file", type=str, required=True)
    ap.add_argument("--answers-file", type=str, required=True)
    ap.add_argument("--conv-mode", type=str, default="llava_v1")
    ap.add_argument("--num-chunks", type=int, default=1)
    ap.add_argument("--chunk-idx", type=int, default=0)
    ap.add_argument("--temperature", type=float, default=0.2, action=StoreGiven)
    ap.add_argument("--top_p", type=float, default=None, action=StoreGiven)
    ap.add_argument("--top_k", type=int, default=0, action=StoreGiven, help="0 = off; sampling only")
    ap.add_argument("--hf_defaults", action="store_true",
                    help="sampling (--num_beams 1) only: take every sampling parameter not given here from the checkpoint's "
                         "generation_config.json, else from transformers 4.35's defaults (top_k 50); with --num_beams > 1 "
                         "nothing is sampled and nothing is resolved")
    ap.add_argument("--num_beams", type=int, default=3)
    ap.add_argument("--max_new_tokens", type=int, default=1024, help="the reference hard-codes 1024")
    ap.add_argument("--batch_size", type=int, default=4, help="questions per call")
    ap.add_argument("--seed", type=int, default=0, help="the sampling generator of --num_beams 1 --temperature > 0")
    return ap


def sampling_args(args) -> Dict:
    """{temperature, top_p, top_k, repetition_penalty} of the parsed command line"""
    # beam search samples nothing: --hf_defaults then must not turn the default temperature into the file's (beam-sample mode)
    s = cli_sampling(os.path.expanduser(args.model_path), args.hf_defaults and args.num_beams == 1, given_on_command_line(args),
                     DEFAULTS)
    if s["top_k"] < 0:
        raise ValueError("--top_k must be >= 0 (0 = off)")
    return s


def main(argv=None):
    args = build_parser().parse_args(argv)
    sampling = sampling_args(args)
    args.temperature = sampling["temperature"]
    if args.conv_mode != "llava_v1":
        raise NotImplementedError(f"--conv-mode {args.conv_mode}: only llava_v1 (conv_llava_v1) prompts are built")
    if args.num_beams > 1 and args.temperature > 0:
        raise NotImplementedError("--num_beams > 1 with --temperature > 0 is HF's beam-sample mode, which is not implemented - "
                                  "pass --temperature 0 (as the evaluation scripts do)")
    import transformers
    from .checkpoint import from_pretrained
    model_path = os.path.expanduser(args.model_path)
    model = from_pretrained(model_path, with_optimizer=False)
    tokenizer = transformers.AutoTokenizer.from_pretrained(model_path, use_fast=False)
    with open(os.path.join(model_path, "config.json")) as f:
        aspect = json.load(f).get("image_aspect_ratio")
    lines = get_chunk(read_gen_dataset(os.path.expanduser(args.question_file), image_aspect_ratio=aspect), args.num_chunks,
                      args.chunk_idx)
    records = answer_questions(model, tokenizer, lines, num_beams=args.num_beams, temperature=args.temperature,
                               top_p=sampling["top_p"], max_new_tokens=args.max_new_tokens, prompts_per_call=args.batch_size,
                               seed=args.seed, top_k=sampling["top_k"], repetition_penalty=sampling["repetition_penalty"])
    answers_file = os.path.expanduser(args.answers_file)
    os.makedirs(os.path.dirname(os.path.abspath(answers_file)), exist_ok=True)
    with open(answers_file, "w") as f:
        for rec in records:
            f.write(json.dumps(rec) + "\n")
    print(f"{len(records)} records -> {answers_file}")


if __name__ == "__main__":
    main()
