"""Record tests/golden/divide_host.json by calling the REFERENCE'S OWN functions (utils/llama3_8b_inference.py of the read-only
checkout at /root/reference) on a dozen hand-written items.  The fixture is data only: inputs and what the reference returned.

    python tests/golden/make_divide_golden.py

  * get_facts on answers with ``###`` lines, blank lines, lines of blanks and lines without a bullet;
  * wrap_prompt_divide_to_list / wrap_prompt_changeq_to_list: the question-key fallbacks (raw_question, prompt, question), the
    answer-key fallback (answer, text), an answer longer than 300 words, ``facts`` given as a string;
  * construct_question_yesno on a changeq file: ``image_path`` in the record or only in metainfos, ``ds_question_id`` in the
    record or only in metainfos, an item whose ``facts`` is a string, more facts than changed facts;
  * the three file names: the reference computes them inside main(), so main() itself runs here with its pipelines and its
    batch_inference replaced by recorders."""
import importlib.util
import json
import os
import sys
import tempfile

HERE = os.path.dirname(os.path.abspath(__file__))
REF = "/root/reference/utils/llama3_8b_inference.py"

ANSWERS = [
    "### Facts:\n- The cat sits on a red sofa.\n- A lamp stands next to the sofa.\n",
    "\n\n### Facts:\n\n- There are two dogs.\n\n-   One dog is black.  \n### End\n- The grass is green.",
    "The picture shows a street.\nIt is raining.",
    "- single fact",
    "### Facts:\n   \n- A man rides a bike.\n* He wears a helmet.\n-No space after the bullet.",
    "",
    "### only a header ###",
]
LONG = " ".join(f"word{i}" for i in range(400))
DIVIDE_ITEMS = [
    {"raw_question": "What is on the sofa?", "prompt": "ignored", "question": "ignored too", "answer": "A cat is on the sofa.", "text": "no"},
    {"prompt": "Describe the image.", "question": "ignored", "answer": "Two dogs play on the grass.\nOne is black."},
    {"question": "How many people are there?", "text": "There are three people."},
    {"raw_question": "Describe in detail.", "answer": LONG},
    {"question": "Short  double  spaces ?", "answer": "yes  it  has"},
]
CHANGEQ_ITEMS = [
    {"facts": ["The cat sits on a red sofa.", "A lamp stands next to the sofa."]},
    {"facts": []},
    {"facts": ["There is no dog."]},
    {"facts": "abc"},
]
GQ_RECORDS = [
    {"question_id": 0, "ds_question_id": 70, "image_path": "img/0.jpg", "raw_question": "What is on the sofa?", "question": "q0",
     "answer": "A cat is on the sofa.", "metainfos": {"origin": "a"}, "facts": ["The cat sits on a sofa.", "The sofa is red."],
     "changed_facts": ["Does the cat sit on a sofa?", "Is the sofa red?"]},
    {"question_id": "q1", "question": "Describe the image.", "answer": "Two dogs.",
     "metainfos": {"image_path": "img/1.jpg", "ds_question_id": 71}, "facts": ["There are two dogs.", "One is black.", "Extra."],
     "changed_facts": ["Are there two dogs?", "Is one black?"]},
    {"question_id": 2, "ds_question_id": 72, "image_path": "img/2.jpg", "question": "Skipped?", "answer": "x", "metainfos": {},
     "facts": "a string", "changed_facts": ["A?"]},
    {"question_id": 3, "ds_question_id": 73, "image_path": "img/3.jpg", "question": "Empty?", "answer": "y", "metainfos": {"k": [1, 2]},
     "facts": [], "changed_facts": []},
]
MAIN_ARGS = [
    ["--path", "data/answers.jsonl"],
    ["--path", "out.jsonl/run.jsonl", "--start", "5", "--end", "40", "--chunk-num", "4", "--chunk-idx", "2", "--divide_suffix", "sfx"],
    ["--path", "plain.json", "--bs", "2"],
]


def load_reference():
    spec = importlib.util.spec_from_file_location("ref_llama3_8b_inference", REF)
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def main():
    R = load_reference()
    out = {"get_facts": [{"in": a, "out": R.get_facts(a)} for a in ANSWERS],
           "divide": [{"item": it, "messages": R.wrap_prompt_divide_to_list(dict(it))} for it in DIVIDE_ITEMS],
           "changeq": [{"item": it, "messages": R.wrap_prompt_changeq_to_list(dict(it))} for it in CHANGEQ_ITEMS]}
    with tempfile.TemporaryDirectory() as d:
        src, dst = os.path.join(d, "in.gq.jsonl"), os.path.join(d, "out.qas.jsonl")
        R.write_jsonlines(src, GQ_RECORDS)
        R.construct_question_yesno(src, dst)
        out["yesno"] = {"records": GQ_RECORDS, "out": R.read_jsonlines(dst)}
        bad = os.path.join(d, "bad.jsonl")
        R.write_jsonlines(bad, [{"question_id": 9, "facts": [], "changed_facts": [], "metainfos": {}}])
        try:
            R.construct_question_yesno(bad, dst)
            out["yesno"]["no_image_path_raises"] = None
        except ValueError as e:
            out["yesno"]["no_image_path_raises"] = str(e)
    # the file names: main() with everything that needs a model replaced by recorders
    out["paths"] = []
    R.init_divide_pipline = R.init_changeq_pipline = lambda: (None, None)
    for argv in MAIN_ARGS:
        seen = []
        R.batch_inference = lambda path, ans_file, *a, **kw: seen.append(ans_file)
        R.construct_question_yesno = lambda path, save_path: seen.append(save_path)
        old = sys.argv
        sys.argv = ["llama3_8b_inference.py"] + argv
        try:
            R.main()
        finally:
            sys.argv = old
        out["paths"].append({"argv": argv, "files": seen})
    with open(os.path.join(HERE, "divide_host.json"), "w") as f:
        json.dump(out, f, indent=1, ensure_ascii=False)
        f.write("\n")
    print({k: len(v) for k, v in out.items()})


if __name__ == "__main__":
    main()
