"""Candidate answers of OmniLMM-12B for the AI-feedback stage (BASELINE config 4): what the model is then trained on.

Mirrors (paths relative to the reference checkout) the non-``--is_yesno`` branches of
  omnilmm/omnilmm_gen_data.py:305-349
started by script/data_gen/omnilmm/omnilmm_diverse_gen.sh with ``--repeat 10 --max_tokens 512 --temperature 0.7``, as gen_data.py
mirrors the LLaVA-1.5 script.  Prompts are omni_data.wrap_question_for_omni_lmm's (``<im_start> <im_patch> x 64 <im_end>`` + the
question in the Zephyr template); the image is whatever ``OmniLMMDPOModel.encode_images`` takes for one image.

  * Sampling branch (:316-323, ``do_sample=True, temperature=, repetition_penalty=1.1``): OmniLMMDPOModel.generate - the N
    ``--repeat`` copies of an item are ONE prompt with N samples that share its prefill and cache rows - or, with
    ``--continuous``, generate_continuous.  The reference hard-codes the penalty 1.1; ``generate_vllm`` decodes from
    ``inputs_embeds``, so the processor sees the generated ids only, which is ``generate``'s meaning of the keyword.
  * Beam branch (:306-314, ``--num_beam >= 1``: ``num_beams=, repetition_penalty=1.1``): OmniLMMDPOModel.beam_search with the
    penalty inside the candidate selection (rv_beam_topk_penalty).  Beam search is deterministic, so the ``--repeat`` copies of an
    item are equal: the answer is computed once and written ``repeat`` times.  ``--num_beam`` <= 8 (rv_beam_topk).

Sampling parameters as in gen_data.py: ``--hf_defaults`` resolves what the command line leaves open from the checkpoint's
generation_config.json and transformers 4.35's defaults (top_k = 50), which is what the reference's call samples with.

Records, the reference's keys in its order (:326-349), one per repeat, item by item: question_id, ds_question_id (when metainfos
carries one), raw_question, answer (the decoded new tokens, special tokens skipped, stripped), metainfos, model_path.

    python -m rlaif_v_amd.omnilmm_gen_data --checkpoint CKPT --ds_name questions.jsonl --answer_file out.jsonl \\
        --repeat 10 --temperature 0.7 --max_tokens 512 --seed 0 --hf_defaults [--continuous --slots 64 | --num_beam 3]
``--is_yesno`` (the labeler's scores) is python -m rlaif_v_amd.autocheck.
"""
from __future__ import annotations

import argparse
import json
from typing import Dict, List, Optional, Sequence

import torch

from .gen_data import _record
from .genconfig import StoreGiven, cli_sampling, given_on_command_line

REPETITION_PENALTY = 1.1                # omnilmm_gen_data.py:314, :323 - not a command-line option of the reference
MAX_BEAMS = 8                           # rv_beam_topk keeps 2 K candidates per row in a wave pair: 1 <= K <= 8
DEFAULTS = {"temperature": 0.7, "top_p": 1.0, "top_k": 0, "repetition_penalty": REPETITION_PENALTY}     # without --hf_defaults


def _stack_images(images):
    if all(torch.is_tensor(im) for im in images) and len({(im.shape, im.dtype) for im in images}) == 1 \
            and images[0].dtype != torch.uint8:
        return torch.stack(images)
    return images


def generate_answers(model, tokenizer, items: Sequence[Dict], repeat: int = 1, temperature: float = 0.7, top_p: float = 1.0,
                     max_tokens: int = 10, seed: Optional[int] = 0, prompts_per_call: int = 6, model_path: Optional[str] = None,
                     repetition_penalty: float = REPETITION_PENALTY, top_k: int = 0, num_beam: int = -1,
                     continuous: bool = False, slots: int = 64, index_base: int = 0) -> List[Dict]:
    """``items``: dicts with ``question`` (text), ``image`` (tower tokens [N, width], or pixels when the model has a tower
    registered), optionally ``question_id`` (default: the item's index) and ``metainfos``.  ``num_beam`` >= 1: one beam search
    per item, its answer written ``repeat`` times; else ``repeat`` samples per item at ``temperature`` as gen_data.generate_answers
    draws them (``seed``, ``prompts_per_call``, ``continuous`` / ``slots`` / ``index_base`` as there).  Records in item order."""
    if getattr(model.cfg, "arch", "llava") != "omnilmm":
        raise NotImplementedError("omnilmm_gen_data: an OmniLMM model is needed (LLaVA-1.5 answers come from rlaif_v_amd.gen_data)")
    if num_beam > MAX_BEAMS:
        raise NotImplementedError(f"omnilmm_gen_data: --num_beam <= {MAX_BEAMS} (rv_beam_topk), got {num_beam}")
    if repeat < 1:
        raise ValueError("omnilmm_gen_data: repeat must be >= 1")
    from .omni_data import wrap_question_for_omni_lmm
    eos = getattr(tokenizer, "eos_token_id", None)
    prompts = [torch.as_tensor(wrap_question_for_omni_lmm(it["question"], model.cfg.n_image_tokens, tokenizer)["input_ids"])
               for it in items]
    if not prompts:
        return []
    answers: List[List[List[int]]] = []                 # [item][copy] -> new token ids
    step = max(1, prompts_per_call)
    if num_beam >= 1:
        for i0 in range(0, len(items), step):
            images = _stack_images([it["image"] for it in items[i0:i0 + step]])
            tokens, _ = model.beam_search(prompts[i0:i0 + step], images, max_new_tokens=max_tokens, num_beams=int(num_beam),
                                          eos_token_id=eos, repetition_penalty=repetition_penalty)
            answers.extend([t] * repeat for t in tokens)
    elif continuous:
        longest = max(int(p.numel()) for p in prompts)           # the replacement splice keeps a prompt's length
        out = dict(model.generate_continuous(((p, it["image"]) for p, it in zip(prompts, items)), max_new_tokens=max_tokens,
                                             slots=max(int(slots), int(repeat)), repeat=repeat, temperature=temperature,
                                             top_p=top_p, top_k=int(top_k), repetition_penalty=repetition_penalty,
                                             eos_token_id=eos, seed=0 if seed is None else int(seed), max_prompt_tokens=longest,
                                             request_indices=range(index_base, index_base + len(items))))
        answers = [out[index_base + n] for n in range(len(items))]
    else:
        gen = torch.Generator().manual_seed(int(seed)) if seed is not None else None
        for i0 in range(0, len(items), step):
            images = _stack_images([it["image"] for it in items[i0:i0 + step]])
            answers.extend(model.generate(prompts[i0:i0 + step], images, max_new_tokens=max_tokens, repeat=repeat,
                                          temperature=temperature, top_p=top_p, repetition_penalty=repetition_penalty,
                                          eos_token_id=eos, generator=gen, **({"top_k": int(top_k)} if top_k else {})))
    records: List[Dict] = []
    for n, it in enumerate(items):
        for r in range(repeat):
            records.append(_record(it, n, tokenizer.decode(answers[n][r], skip_special_tokens=True).strip(), model_path))
    return records


def build_parser() -> argparse.ArgumentParser:
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--checkpoint", type=str, required=True)
    ap.add_argument("--ds_name", type=str, required=True, help="question file in the jsonl format of the reference's GenDataset")
    ap.add_argument("--answer_file", type=str, required=True)
    ap.add_argument("--is_yesno", action="store_true", default=False)
    ap.add_argument("--max_sample", type=int, default=-1, help="at most this many items of the file (-1: all)")
    ap.add_argument("--start_pos", "--start", dest="start", type=int, default=0)
    ap.add_argument("--end_pos", "--end", dest="end", type=int, default=-1)
    ap.add_argument("--repeat", type=int, default=1)
    ap.add_argument("--temperature", type=float, default=0.7, action=StoreGiven)
    ap.add_argument("--top_p", type=float, default=1.0, action=StoreGiven)
    ap.add_argument("--top_k", type=int, default=0, action=StoreGiven, help="0 = off")
    ap.add_argument("--hf_defaults", action="store_true",
                    help="take every sampling parameter not given here from the checkpoint's generation_config.json, else "
                         "from transformers 4.35's defaults (top_k 50): the values the reference's generate call runs with")
    ap.add_argument("--num_beam", type=int, default=-1, help=f">= 1: beam search with that many beams (<= {MAX_BEAMS})")
    ap.add_argument("--max_tokens", type=int, default=10)
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--batch-size", "--batch_size", dest="batch_size", type=int, default=1,
                    help="items per generate / beam_search call (x --repeat or --num_beam decode rows)")
    ap.add_argument("--num-workers", "--num_workers", dest="num_workers", type=int, default=1, help="accepted, unused")
    ap.add_argument("--continuous", action="store_true",
                    help="continuous batching: --slots decode rows, a finished row is given to the next item "
                         "(generate_continuous); an item's samples then depend on --seed and its index in the file alone")
    ap.add_argument("--slots", type=int, default=64, help="decode rows of --continuous")
    return ap


def sampling_args(args) -> Dict:
    """{temperature, top_p, top_k, repetition_penalty} of the parsed command line; the penalty is the reference's 1.1, which its
    call names itself - no generation_config.json replaces it"""
    given = given_on_command_line(args)
    given["repetition_penalty"] = REPETITION_PENALTY
    s = cli_sampling(args.checkpoint, args.hf_defaults, given, DEFAULTS)
    if s["top_k"] < 0:
        raise ValueError("--top_k must be >= 0 (0 = off)")
    return s


def main(argv=None):
    args = build_parser().parse_args(argv)
    if args.is_yesno:
        raise NotImplementedError("--is_yesno (next-token scores) is python -m rlaif_v_amd.autocheck")
    if args.num_beam > MAX_BEAMS:
        raise NotImplementedError(f"--num_beam <= {MAX_BEAMS} (rv_beam_topk), got {args.num_beam}")
    if args.num_beam >= 1 and args.continuous:
        raise NotImplementedError("--continuous is the sampling branch's: beam search runs --batch-size items per call")
    sampling = sampling_args(args)
    import transformers
    from .autocheck import read_gen_dataset
    from .checkpoint import from_pretrained
    model = from_pretrained(args.checkpoint, with_optimizer=False)
    tokenizer = transformers.AutoTokenizer.from_pretrained(args.checkpoint, use_fast=False)
    items = read_gen_dataset(args.ds_name, args.start, args.end)         # OmniLMM's collator applies the image transform alone
    if args.max_sample >= 0:
        items = items[:args.max_sample]
    records = generate_answers(model, tokenizer, items, repeat=args.repeat, temperature=sampling["temperature"],
                               top_p=sampling["top_p"], max_tokens=args.max_tokens, seed=args.seed,
                               prompts_per_call=args.batch_size, model_path=args.checkpoint,
                               repetition_penalty=sampling["repetition_penalty"], top_k=sampling["top_k"],
                               num_beam=args.num_beam,
                               **(dict(continuous=True, slots=args.slots, index_base=max(args.start, 0)) if args.continuous else {}))
    with open(args.answer_file, "w") as f:
        for rec in records:
            f.write(json.dumps(rec) + "\n")
    print(f"{len(records)} records -> {args.answer_file}")


if __name__ == "__main__":
    main()
