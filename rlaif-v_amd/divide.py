"""Claim splitting: step 2 of the reference's data pipeline (script/data_gen/run_data_pipline_llava15_omni.sh), between the
candidate answers of ``rlaif_v_amd.gen_data`` and the labeler's yes / no scoring of ``rlaif_v_amd.autocheck``.

Restates utils/llama3_8b_inference.py of the reference: every (question, answer) record is split into atomic claims by one
Llama-3-8B fine-tune ("divide"), every claim is rewritten as a general question by a second one ("changeq"), and each
(claim, question) pair becomes one yes / no item for the labeler.  The reference runs both models behind
``transformers.pipeline("text-generation")(prompts, eos_token_id=[eos, <|eot_id|>], max_new_tokens=256, do_sample=True,
temperature=0.2, top_p=0.9)``; here they are text-only models of this library (textlm.py, checkpoint.from_pretrained on an HF
``LlamaForCausalLM`` directory) and the decoding is ``generate(prompts, None, ...)`` - pad-free prefill, KV-cached decode steps,
rv_sample_token_wide over Llama-3's 128256 ids.  The pipeline's left padding needs no counterpart: HF derives the positions from
the attention mask, so every prompt is decoded as if alone, which is what the pad-free row per prompt does.

Prompt: ``tokenizer.apply_chat_template(messages, tokenize=False, add_generation_prompt=True)``, then tokenised as the
installed transformers' text-generation pipeline tokenises a string prompt - ``tokenizer(prompt)`` with the tokenizer's own
defaults, i.e. add_special_tokens=True.  BOS: Llama-3's template already writes ``<|begin_of_text|>`` into the text and its
tokenizer prepends the BOS id once more, so the ids start with TWO BOS tokens, exactly what the reference's models see.
Answer text: ``tokenizer.decode(new_tokens, skip_special_tokens=True)``.

Sampling: HF's processors (temperature 0.2, top_k when given, then top_p 0.9) drawn from the uniforms of a seeded CPU generator -
``--seed`` fixes the output (the changeq stage uses seed + 1), but as in gen_data the stream is not torch.multinomial's.  The
reference's pipeline call names temperature and top_p only, so under its transformers 4.35 top_k and the repetition penalty come
from each checkpoint's generation_config.json, else from the library defaults (top_k = 50): ``--hf_defaults`` resolves them that
way for each of the two checkpoints (genconfig.resolve_sampling) and is what reproduces the reference's DISTRIBUTION; without it
there is no top-k, as before.  ``--top_k`` sets it by hand for both stages.  A resumed run draws its
uniforms afresh for the items that are left, so it does not repeat the samples of an uninterrupted one.

Files (the reference's names): with ``--path X.jsonl`` the divide stage writes
``X.s{start}-e{end}.chunk{chunk_num}-{chunk_idx}.{divide_suffix}.jsonl`` (records + ``raw_facts`` / ``facts``), the changeq stage
``....gq.jsonl`` (+ ``raw_changed_facts`` / ``changed_facts``) and ``construct_question_yesno`` ``....gq.qas.jsonl``.  An answer
file that already exists is resumed: as many items as it has lines are skipped, new records are appended.

    python -m rlaif_v_amd.divide --path answers.jsonl --divide_model DIR --changeq_model DIR --bs 8 --seed 0 --hf_defaults
"""
from __future__ import annotations

import argparse
import copy
import json
import math
import os
from typing import Callable, Dict, List, Optional, Sequence

import torch

from .genconfig import StoreGiven, cli_sampling, given_on_command_line

TEMPERATURE, TOP_P, MAX_NEW_TOKENS = 0.2, 0.9, 256
DIVIDE_WORDS = 300          # the divide prompt is cut to its first 300 space-separated pieces
EOT = "<|eot_id|>"

DIVIDE_HEAD = ("You are an expert in extracting facts from the given question-answer pair for an image. Your task is to extract and "
               "rewrite the facts mentioned in the question-answer pair into self-contained sentences. Exclude opinions or "
               "subjective statements.\n\nYou should present your result in the following format:\n### Facts:\n- {Extracted fact 1}"
               "\n- {Extracted fact 2}\n- ...\n\n### Question-answer pair:\nQuestion: ")
CHANGEQ_HEAD = ("You are an expert at modifying a given declarative sentence into a general question sentence. Your task is to "
                "modify the given declarative sentences one by one into a general question form. Do not change tenses or add extra "
                "content.\n    If the given declarative sentence contains not, no or negative meaning words, you need to check the "
                "modified general interrogative sentence to make sure that the generated general question sentence retains words "
                "with not , no or negative meaning words.\n\nYou should present your result in the following format:\n### Modified "
                "sentences:\n- {Modified sentence 1}\n- {Modified sentence 2}\n- ...\n\n### Declarative sentences:")


# ------------------------------------------------------------------------------------------------ text in, text out
def get_facts(result: str) -> List[str]:
    """The bullet list of a model answer: every line that is not empty and holds no ``###``, WITHOUT its first character (the
    bullet - a line without one loses a letter, as in the reference) and stripped.  A line of blanks only yields ''."""
    facts = []
    for line in result.strip().split("\n"):
        if line == "" or "###" in line:
            continue
        facts.append(line[1:].strip())
    return facts


def divide_messages(item: Dict) -> List[Dict]:
    """The divide model's user turn.  Question: ``raw_question``, else ``prompt``, else ``question``; answer: ``answer``, else
    ``text``.  The content is cut to its first 300 pieces between single spaces (newlines do not split)."""
    question = item["raw_question"] if "raw_question" in item else item["prompt"] if "prompt" in item else item["question"]
    answer = item["answer"] if "answer" in item else item["text"]
    content = DIVIDE_HEAD + question + "\nAnswer: " + answer
    return [{"role": "user", "content": " ".join(content.split(" ")[:DIVIDE_WORDS])}]


def changeq_messages(item: Dict) -> List[Dict]:
    """The changeq model's user turn: one ``\\n- fact\\n`` per entry of ``facts`` (a string is walked character by character, as
    the reference does; construct_question_yesno drops such items)."""
    return [{"role": "user", "content": CHANGEQ_HEAD + "".join("\n- {}\n".format(f) for f in item["facts"])}]


def output_paths(path: str, start: int, end: int, chunk_num: int, chunk_idx: int, divide_suffix: str):
    """(divide, changeq, yes / no) file names: every ``.jsonl`` of the name is replaced, as str.replace does"""
    divide = path.replace(".jsonl", f".s{start}-e{end}.chunk{chunk_num}-{chunk_idx}.{divide_suffix}.jsonl")
    gq = divide.replace(".jsonl", ".gq.jsonl")
    return divide, gq, gq.replace(".jsonl", ".qas.jsonl")


def read_items(path: str) -> List[Dict]:
    """one json document (a list, or a single record) or json lines"""
    with open(path, "r") as f:
        text = f.read()
    try:
        data = json.loads(text)
    except ValueError:
        data = [json.loads(line) for line in text.split("\n") if line.strip()]
    return [data] if isinstance(data, dict) else data


def select_items(data: List[Dict], start: int = 0, end: int = -1, chunk_num: int = 1, chunk_idx: int = 0) -> List[Dict]:
    """``data[start:end]`` (end > 0: clipped to the length, -1: the length, any other value: Python's slice) and of that the
    ``chunk_idx``-th of ``chunk_num`` chunks of ceil(n / chunk_num) items"""
    if end > 0:
        end = min(end, len(data))
    elif end == -1:
        end = len(data)
    data = data[start:end]
    if not data:
        return []
    size = math.ceil(len(data) / chunk_num)
    return [data[i:i + size] for i in range(0, len(data), size)][chunk_idx]


def construct_question_yesno(path: str, save_path: str) -> List[Dict]:
    """One labeler item per (fact, changed fact) pair of every record of the changeq file: the question is the changed fact +
    ' Please answer yes or no.', metainfos carries the origin.  ``image_path`` is the record's or its metainfos'; a record whose
    ``facts`` is a string is skipped; zip() drops the facts without a partner."""
    with open(path, "r") as f:
        data = [json.loads(line) for line in f]
    out = []
    for item in data:
        if "image_path" in item:
            image_path = item["image_path"]
        elif isinstance(item.get("metainfos"), dict) and "image_path" in item["metainfos"]:
            image_path = item["metainfos"]["image_path"]
        else:
            raise ValueError("Do not have 'image_path' in the data!")
        if isinstance(item["facts"], str):
            continue
        for fact, changed in zip(item["facts"], item["changed_facts"]):
            meta = copy.deepcopy(item["metainfos"])
            meta["origin_question"] = item["raw_question"] if "raw_question" in item else item["question"]
            meta["origin_answer"] = item["answer"]
            meta["origin_fact"] = fact
            meta["origin_changed_fact"] = changed
            meta["origin_all_facts"] = item["facts"]
            meta["origin_changed_all_facts"] = item["changed_facts"]
            out.append({"question_id": item["question_id"],
                        "ds_question_id": item["ds_question_id"] if "ds_question_id" in item else item["metainfos"]["ds_question_id"],
                        "image_path": image_path, "question": f"{changed} Please answer yes or no.", "metainfos": meta})
    with open(save_path, "w") as f:
        for rec in out:
            f.write(json.dumps(rec) + "\n")
    return out


# ------------------------------------------------------------------------------------------------ one stage
def terminators(tokenizer) -> List[int]:
    return [int(tokenizer.eos_token_id), int(tokenizer.convert_tokens_to_ids(EOT))]


def prompt_ids(tokenizer, messages: List[Dict]) -> torch.Tensor:
    text = tokenizer.apply_chat_template(messages, tokenize=False, add_generation_prompt=True)
    return torch.as_tensor(list(tokenizer(text)["input_ids"]), dtype=torch.int64).reshape(-1)


def stage_sampling(checkpoint_dir: Optional[str], top_k: Optional[int] = None, hf_defaults: bool = False) -> Dict:
    """{temperature, top_p, top_k, repetition_penalty} of one stage: temperature 0.2 and top_p 0.9 are the explicit values of the
    reference's call; ``top_k`` as given, else (``hf_defaults``) what that checkpoint's generation_config.json or transformers
    4.35 says, else off; the repetition penalty likewise."""
    given = {"temperature": TEMPERATURE, "top_p": TOP_P, "top_k": top_k, "repetition_penalty": None}
    s = cli_sampling(checkpoint_dir, hf_defaults, given, {"temperature": TEMPERATURE, "top_p": TOP_P, "top_k": 0,
                                                          "repetition_penalty": 1.0})
    if s["top_k"] < 0:
        raise ValueError("divide: top_k must be >= 0 (0 = off)")
    return s


def batch_inference(model, tokenizer, path: str, ans_file: str, key: str, wrap: Callable[[Dict], List[Dict]], batch_size: int = 8,
                    chunk_num: int = 1, chunk_idx: int = 0, max_tokens: int = MAX_NEW_TOKENS, start: int = 0, end: int = -1,
                    seed: Optional[int] = 0, top_k: int = 0, repetition_penalty: float = 1.0) -> List[Dict]:
    """One stage over the selected items of ``path``: per item ``raw_{key}`` (the answer text) and ``{key}`` (get_facts of it)
    are added and the record is appended to ``ans_file`` at once.  Returns the records of the file, earlier ones included."""
    if getattr(model.cfg, "arch", "llava") != "text":
        raise NotImplementedError("divide: the claim-splitting stage runs text-only models (TextLMConfig)")
    if os.path.abspath(ans_file) == os.path.abspath(path):
        raise ValueError(f"divide: the answer file would be the input file {path} (the input's name must hold '.jsonl')")
    data = select_items(read_items(path), start, end, chunk_num, chunk_idx)
    done: List[Dict] = []
    if os.path.exists(ans_file):
        with open(ans_file, "r") as f:
            done = [json.loads(line) for line in f.readlines()]
        data = data[len(done):]
    elif os.path.dirname(ans_file):
        os.makedirs(os.path.dirname(ans_file), exist_ok=True)
    gen = torch.Generator().manual_seed(int(seed)) if seed is not None else None
    stop = terminators(tokenizer)
    extra = {}                                                    # the call of before when neither is asked for
    if top_k:
        extra["top_k"] = int(top_k)
    if repetition_penalty != 1.0:
        extra["repetition_penalty"] = float(repetition_penalty)
    with open(ans_file, "a" if done else "w") as out:
        for i0 in range(0, len(data), max(1, batch_size)):
            chunk = data[i0:i0 + max(1, batch_size)]
            prompts = [prompt_ids(tokenizer, wrap(it)) for it in chunk]
            toks = model.generate(prompts, None, max_new_tokens=max_tokens, temperature=TEMPERATURE, top_p=TOP_P,
                                  eos_token_id=stop, generator=gen, **extra)
            for it, new in zip(chunk, toks):
                resp = tokenizer.decode(new[0], skip_special_tokens=True)
                it[f"raw_{key}"] = resp
                it[key] = get_facts(resp)
                done.append(it)
                out.write(json.dumps(it, ensure_ascii=False) + "\n")
                out.flush()
    return done


def run(path: str, load: Callable[[str], tuple], divide_model: str, changeq_model: str, divide_suffix: str = "llama3-8b_divide",
        chunk_num: int = 1, chunk_idx: int = 0, bs: int = 4, start: int = 0, end: int = -1, seed: Optional[int] = 0,
        top_k: Optional[int] = None, hf_defaults: bool = False):
    """The whole stage.  ``load(name) -> (model, tokenizer)``; the two checkpoints are loaded one after the other, the first is
    released before the second is built.  ``top_k`` / ``hf_defaults``: stage_sampling, per checkpoint.  Returns the three file
    names."""
    p_div, p_gq, p_qas = output_paths(path, start, end, chunk_num, chunk_idx, divide_suffix)
    s_div, s_gq = stage_sampling(divide_model, top_k, hf_defaults), stage_sampling(changeq_model, top_k, hf_defaults)
    model, tokenizer = load(divide_model)
    batch_inference(model, tokenizer, path, p_div, "facts", divide_messages, bs, chunk_num, chunk_idx, MAX_NEW_TOKENS, start, end, seed,
                    top_k=s_div["top_k"], repetition_penalty=s_div["repetition_penalty"])
    del model, tokenizer
    if torch.cuda.is_available():
        torch.cuda.empty_cache()
    model, tokenizer = load(changeq_model)
    batch_inference(model, tokenizer, p_div, p_gq, "changed_facts", changeq_messages, bs, max_tokens=MAX_NEW_TOKENS,
                    seed=None if seed is None else int(seed) + 1, top_k=s_gq["top_k"],
                    repetition_penalty=s_gq["repetition_penalty"])
    del model, tokenizer
    construct_question_yesno(p_gq, p_qas)
    return p_div, p_gq, p_qas


def load_text_model(ckpt_dir: str):
    import transformers
    from .checkpoint import from_pretrained
    model = from_pretrained(ckpt_dir, with_optimizer=False)
    if getattr(model.cfg, "arch", "llava") != "text":
        raise ValueError(f"{ckpt_dir}: not a text-only checkpoint (config.json model_type must be 'llama')")
    return model, transformers.AutoTokenizer.from_pretrained(ckpt_dir, padding_side="left")


def build_parser() -> argparse.ArgumentParser:
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--path", type=str, required=True)
    ap.add_argument("--divide_model", type=str, required=True, help="HF LlamaForCausalLM directory of the claim splitter")
    ap.add_argument("--changeq_model", type=str, required=True, help="HF LlamaForCausalLM directory of the question rewriter")
    ap.add_argument("--divide_suffix", type=str, default="llama3-8b_divide")
    ap.add_argument("--chunk-num", type=int, default=1)
    ap.add_argument("--chunk-idx", type=int, default=0)
    ap.add_argument("--bs", type=int, default=4)
    ap.add_argument("--start", type=int, default=0)
    ap.add_argument("--end", type=int, default=-1)
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--top_k", type=int, default=0, action=StoreGiven,
                    help="0 = off; when not given, --hf_defaults takes each checkpoint's own")
    ap.add_argument("--hf_defaults", action="store_true",
                    help="take top_k and the repetition penalty, when not given here, from each checkpoint's "
                         "generation_config.json, else from transformers 4.35's defaults (top_k 50)")
    return ap


def main(argv: Optional[Sequence[str]] = None):
    args = build_parser().parse_args(argv)
    paths = run(args.path, load_text_model, args.divide_model, args.changeq_model, args.divide_suffix, args.chunk_num,
                args.chunk_idx, args.bs, args.start, args.end, args.seed, top_k=given_on_command_line(args)["top_k"],
                hf_defaults=args.hf_defaults)
    for p in paths:
        print(p)
    return paths


if __name__ == "__main__":
    main()
