"""The sampling parameters a reference ``generate(do_sample=True, ...)`` call really runs with.

The reference pins transformers==4.35.0 (its pyproject.toml).  In that version every sampling parameter a ``generate`` call does
not name is taken from the checkpoint's ``generation_config.json``, and where the file is silent from the library's
GenerationConfig defaults: ``top_k=50``, ``top_p=1.0``, ``temperature=1.0``, ``repetition_penalty=1.0``.  None of the reference's
sampling calls (muffin/llava15_gen_data.py:351-356, omnilmm/omnilmm_gen_data.py:318-323, utils/llama3_8b_inference.py:174-180)
names ``top_k``, so all of them sample behind a top-50 filter, and the LLaVA call takes its ``top_p`` from the file as well.
Later transformers releases construct GenerationConfig() with None defaults, so the 4.35 values are written down here, not read
from the installed package; the file is read with ``json`` alone."""
from __future__ import annotations

import argparse
import json
import os
from typing import Dict, Optional

HF_4_35_DEFAULTS = {"temperature": 1.0, "top_p": 1.0, "top_k": 50, "repetition_penalty": 1.0}
GENERATION_CONFIG = "generation_config.json"


def read_generation_config(checkpoint_dir: Optional[str]) -> Dict:
    """The checkpoint's generation_config.json as a dict; {} when there is no directory or no file."""
    if not checkpoint_dir:
        return {}
    path = os.path.join(os.path.expanduser(str(checkpoint_dir)), GENERATION_CONFIG)
    if not os.path.isfile(path):
        return {}
    with open(path, "r") as f:
        cfg = json.load(f)
    if not isinstance(cfg, dict):
        raise ValueError(f"{path}: not a JSON object")
    return cfg


def resolve_sampling(checkpoint_dir: Optional[str], temperature: Optional[float] = None, top_p: Optional[float] = None,
                     top_k: Optional[int] = None, repetition_penalty: Optional[float] = None) -> Dict:
    """{temperature, top_p, top_k, repetition_penalty}: per parameter the explicit value (not None), else the value in the
    checkpoint's generation_config.json (``null`` counts as absent), else transformers 4.35's default.  ``top_k`` 0 - given or
    in the file - means off, as in HF and in ops.sample_token."""
    cfg = read_generation_config(checkpoint_dir)
    given = {"temperature": temperature, "top_p": top_p, "top_k": top_k, "repetition_penalty": repetition_penalty}
    out = {}
    for name, default in HF_4_35_DEFAULTS.items():
        v = given[name]
        if v is None:
            v = cfg.get(name)
        if v is None:
            v = default
        out[name] = int(v) if name == "top_k" else float(v)
        if name == "top_k" and out[name] != v:
            raise ValueError(f"top_k must be an integer, got {v!r}")
    if out["top_k"] < 0:
        raise ValueError(f"top_k must be >= 0 (0 = off), got {out['top_k']}")
    return out


class StoreGiven(argparse.Action):
    """``store`` that also notes the option's dest in ``namespace.given``: an option with a default of its own can then be told
    from one the user wrote on the command line."""

    def __call__(self, parser, namespace, values, option_string=None):
        setattr(namespace, self.dest, values)
        namespace.given = tuple(getattr(namespace, "given", None) or ()) + (self.dest,)


def given_on_command_line(args, names=("temperature", "top_p", "top_k")) -> Dict:
    """{name: the parsed value if the user gave the option, else None} (``repetition_penalty``: no command line has it)"""
    given = getattr(args, "given", None) or ()
    out = {n: (getattr(args, n) if n in given else None) for n in names}
    out["repetition_penalty"] = None
    return out


def cli_sampling(checkpoint_dir: Optional[str], hf_defaults: bool, given: Dict, fallback: Dict) -> Dict:
    """What a command line samples with.  ``given``: the four parameters as the user gave them (None = not given);
    ``fallback``: the command's own defaults.  Without ``hf_defaults`` a parameter that was not given is the command's default -
    the behaviour of before; with it, resolve_sampling's value for that checkpoint."""
    if hf_defaults:
        return resolve_sampling(checkpoint_dir, **{k: given.get(k) for k in HF_4_35_DEFAULTS})
    out = {k: (given.get(k) if given.get(k) is not None else fallback[k]) for k in HF_4_35_DEFAULTS}
    out["top_k"] = int(out["top_k"])
    return out
