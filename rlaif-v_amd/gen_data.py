"""Candidate answers for the AI-feedback stage: the sampling side of the loop that makes the preference pairs.

Mirrors (paths relative to the reference checkout) the non-``--is_yesno`` branch of
  muffin/llava15_gen_data.py:335-381   (LLaVA-1.5, conv_llava_v1 prompts)
started by script/data_gen/llava15/llava15_diverse_gen.sh with ``--repeat N --temperature 0.7 --max_tokens ...``: the dataset
repeats every (image, question) item N times in a row (GenDataset, :102-106) and ``generate(do_sample=True, temperature=,
max_new_tokens=, use_cache=True)`` answers each copy on its own - N prefills of the same prompt.  Here the N copies of an item
are ONE prompt with ``repeat=N`` samples: the tower and the prefill run once, the prompt's keys and values are stored once and the
N decode rows share them (LlavaDPOModel.generate, rv_gemm_nt_skinny_bf16, rv_attn_decode, rv_sample_token).

Sampling: HF's processors (temperature, then top_k and top_p when given), drawn from uniforms of a seeded CPU generator -
``--seed`` fixes the output, but the stream is not torch.multinomial's, so the reference's exact samples are not reproduced (no
two seeds of the reference agree either).  The reference's call names neither top_k nor top_p, so under its transformers 4.35 it
samples with the checkpoint's generation_config.json and the library defaults (top_k = 50): ``--hf_defaults`` resolves every
sampling parameter that is not on the command line that way (genconfig.resolve_sampling) and is what reproduces the reference's
DISTRIBUTION; without it the defaults below apply (no top-k, top_p 1) as before.  ``--num_beam`` >= 1 (the reference's beam-search branch) is not implemented.

Records, one per repeat in the reference's order (item by item, the copies of an item in a row): question_id, ds_question_id (when
metainfos carries one), raw_question, answer (the decoded new tokens, special tokens skipped, stripped), metainfos, model_path.

Command line (the jsonl format of the reference's GenDataset in; one record per line out):
    python -m rlaif_v_amd.gen_data --checkpoint CKPT --ds_name questions.jsonl --answer_file out.jsonl \\
        --repeat 10 --temperature 0.7 --max_tokens 512 --seed 0 --hf_defaults
``--continuous --slots 64`` runs the same stage with continuous batching (generate_continuous): the same records in the same
order, other samples (the uniforms are then a hash of the seed and the item's index), fewer decode steps.
"""
from __future__ import annotations

import argparse
import json
import os
from typing import Dict, List, Optional, Sequence

import torch

from .autocheck import read_gen_dataset, wrap_question_for_llava15
from .genconfig import StoreGiven, cli_sampling, given_on_command_line

DEFAULTS = {"temperature": 0.7, "top_p": 1.0, "top_k": 0, "repetition_penalty": 1.0}     # without --hf_defaults


def generate_answers(model, tokenizer, items: Sequence[Dict], repeat: int = 1, temperature: float = 0.7, top_p: float = 1.0,
                     max_tokens: int = 10, seed: Optional[int] = 0, prompts_per_call: int = 6, model_path: Optional[str] = None,
                     repetition_penalty: float = 1.0, top_k: int = 0, continuous: bool = False, slots: int = 64,
                     index_base: int = 0) -> List[Dict]:
    """``items``: dicts with ``question`` (text), ``image`` (what ``encode_images`` takes for ONE image: a preprocessed
    [3, H, W] tensor or a raw uint8 [H, W, 3] image), optionally ``question_id`` (default: the item's index) and ``metainfos``.
    ``repeat`` samples per item at ``temperature`` (0 = greedy: the copies are then equal); ``seed``: the CPU generator the
    uniforms come from (None: torch's default generator).  ``prompts_per_call`` items share one ``generate`` call.
    ``continuous``: the items go through ``generate_continuous`` with ``slots`` decode rows instead (a finished row is given to
    the next item; ``prompts_per_call`` then plays no part), item n under the request index ``index_base`` + n - its absolute
    index in the question file when ``index_base`` is the shard's --start - so that its samples depend on ``seed`` and that
    index alone, not on the shard or the other items.  The records are the same, in item order."""
    if getattr(model.cfg, "arch", "llava") == "omnilmm":
        raise NotImplementedError("gen_data: OmniLMM generation is not implemented (LlavaDPOModel.generate is LLaVA-1.5 only)")
    if continuous:
        return _generate_answers_continuous(model, tokenizer, items, repeat, temperature, top_p, max_tokens, seed, model_path,
                                            repetition_penalty, top_k, slots, index_base)
    gen = torch.Generator().manual_seed(int(seed)) if seed is not None else None
    eos = getattr(tokenizer, "eos_token_id", None)
    mm = getattr(model.cfg, "mm_use_im_start_end", False)
    records: List[Dict] = []
    step = max(1, prompts_per_call)
    for i0 in range(0, len(items), step):
        chunk = items[i0:i0 + step]
        prompts = [wrap_question_for_llava15(it["question"], tokenizer, mm) for it in chunk]
        images = [it["image"] for it in chunk]
        if all(torch.is_tensor(im) for im in images) and len({(im.shape, im.dtype) for im in images}) == 1 \
                and images[0].dtype != torch.uint8:
            images = torch.stack(images)
        out = model.generate(prompts, images, max_new_tokens=max_tokens, repeat=repeat, temperature=temperature, top_p=top_p,
                             repetition_penalty=repetition_penalty, eos_token_id=eos, generator=gen,
                             **({"top_k": int(top_k)} if top_k else {}))
        for n, it in enumerate(chunk):
            meta = it.get("metainfos", {})
            for r in range(repeat):
                rec = {"question_id": it.get("question_id", i0 + n)}
                if "ds_question_id" in meta:
                    rec["ds_question_id"] = meta["ds_question_id"]
                rec.update(raw_question=it["question"], answer=tokenizer.decode(out[n][r], skip_special_tokens=True).strip(),
                           metainfos=meta, model_path=model_path)
                records.append(rec)
    return records


def _record(it: Dict, default_id, answer: str, model_path: Optional[str]) -> Dict:
    meta = it.get("metainfos", {})
    rec = {"question_id": it.get("question_id", default_id)}
    if "ds_question_id" in meta:
        rec["ds_question_id"] = meta["ds_question_id"]
    rec.update(raw_question=it["question"], answer=answer, metainfos=meta, model_path=model_path)
    return rec


def _generate_answers_continuous(model, tokenizer, items, repeat, temperature, top_p, max_tokens, seed, model_path,
                                 repetition_penalty, top_k, slots, index_base) -> List[Dict]:
    from .splice import IMAGE_TOKEN_INDEX
    eos = getattr(tokenizer, "eos_token_id", None)
    mm = getattr(model.cfg, "mm_use_im_start_end", False)
    prompts = [torch.as_tensor(wrap_question_for_llava15(it["question"], tokenizer, mm)) for it in items]
    if not prompts:
        return []
    n_img = int(model.cfg.n_image_tokens)
    longest = max(int(p.numel()) + (n_img - 1) * int((p == IMAGE_TOKEN_INDEX).sum()) for p in prompts)     # spliced lengths
    out = dict(model.generate_continuous(((p, it["image"]) for p, it in zip(prompts, items)), max_new_tokens=max_tokens,
                                         slots=max(int(slots), int(repeat)), repeat=repeat, temperature=temperature, top_p=top_p,
                                         top_k=int(top_k), repetition_penalty=repetition_penalty, eos_token_id=eos,
                                         seed=0 if seed is None else int(seed), max_prompt_tokens=longest,
                                         request_indices=range(index_base, index_base + len(items))))
    records: List[Dict] = []
    for n, it in enumerate(items):
        for r in range(repeat):
            answer = tokenizer.decode(out[index_base + n][r], skip_special_tokens=True).strip()
            records.append(_record(it, n, answer, model_path))
    return records


def build_parser() -> argparse.ArgumentParser:
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--checkpoint", type=str, required=True)
    ap.add_argument("--ds_name", type=str, required=True, help="question file in the jsonl format of the reference's GenDataset")
    ap.add_argument("--answer_file", type=str, required=True)
    ap.add_argument("--repeat", type=int, default=1)
    ap.add_argument("--temperature", type=float, default=0.7, action=StoreGiven)
    ap.add_argument("--top_p", type=float, default=1.0, action=StoreGiven)
    ap.add_argument("--top_k", type=int, default=0, action=StoreGiven, help="0 = off")
    ap.add_argument("--hf_defaults", action="store_true",
                    help="take every sampling parameter not given here from the checkpoint's generation_config.json, else "
                         "from transformers 4.35's defaults (top_k 50): the values the reference's generate call runs with")
    ap.add_argument("--max_tokens", type=int, default=10)
    ap.add_argument("--num_beam", type=int, default=-1)
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--batch_size", type=int, default=6, help="items per generate call (x --repeat decode rows)")
    ap.add_argument("--continuous", action="store_true",
                    help="continuous batching: --slots decode rows, a finished row is given to the next item "
                         "(LlavaDPOModel.generate_continuous); an item's samples then depend on --seed and its index in the "
                         "question file alone")
    ap.add_argument("--slots", type=int, default=64, help="decode rows of --continuous")
    ap.add_argument("--start", "--start_pos", dest="start", type=int, default=0)
    ap.add_argument("--end", "--end_pos", dest="end", type=int, default=-1)
    return ap


def sampling_args(args) -> Dict:
    """{temperature, top_p, top_k, repetition_penalty} of the parsed command line"""
    s = cli_sampling(args.checkpoint, args.hf_defaults, given_on_command_line(args), DEFAULTS)
    if s["top_k"] < 0:
        raise ValueError("--top_k must be >= 0 (0 = off)")
    return s


def main(argv=None):
    args = build_parser().parse_args(argv)
    sampling = sampling_args(args)
    if args.num_beam >= 1:
        raise NotImplementedError("--num_beam >= 1 (beam search) is not implemented: only the sampling branch is")
    import transformers
    from .checkpoint import from_pretrained
    model = from_pretrained(args.checkpoint, with_optimizer=False)
    tokenizer = transformers.AutoTokenizer.from_pretrained(args.checkpoint, use_fast=False)
    with open(os.path.join(args.checkpoint, "config.json")) as f:
        aspect = json.load(f).get("image_aspect_ratio")
    items = read_gen_dataset(args.ds_name, args.start, args.end, image_aspect_ratio=aspect)
    records = generate_answers(model, tokenizer, items, repeat=args.repeat, temperature=sampling["temperature"],
                               top_p=sampling["top_p"], max_tokens=args.max_tokens, seed=args.seed,
                               prompts_per_call=args.batch_size, model_path=args.checkpoint,
                               repetition_penalty=sampling["repetition_penalty"], top_k=sampling["top_k"],
                               **(dict(continuous=True, slots=args.slots, index_base=max(args.start, 0)) if args.continuous else {}))
    with open(args.answer_file, "w") as f:
        for rec in records:
            f.write(json.dumps(rec) + "\n")
    print(f"{len(records)} records -> {args.answer_file}")


if __name__ == "__main__":
    main()
