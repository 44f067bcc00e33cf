"""A text-only language model: the Llama decoder of LlavaDPOModel without tower, projector or image tokens - what the
claim-splitting stage of the data pipeline runs (utils/llama3_8b_inference.py of the reference: two Llama-3-8B fine-tunes behind
``transformers.pipeline("text-generation")``).  Inference only: prefill through the training forward's stack, KV-cached decoding
through ``generate(prompts, None, ...)``; at Llama-3's 128256 ids the sampler is rv_sample_token_wide (ops.sampler_for).

The store holds the language model alone (ParamStore: every tensor frozen, no gradient, master or moment buffers), loaded from
an HF ``LlamaForCausalLM`` directory by checkpoint.from_pretrained (``model_type: "llama"``)."""
from __future__ import annotations

from dataclasses import dataclass
from typing import Dict, Optional

import torch

from .model import BF16, LlavaConfig, LlavaDPOModel


@dataclass
class TextLMConfig(LlavaConfig):
    """LlavaConfig's language-model fields; the vision fields are unused.  Defaults: Llama-3-8B."""
    hidden: int = 4096
    layers: int = 32
    heads: int = 32
    ffn: int = 14336
    vocab: int = 128256
    rope_theta: float = 500000.0
    model_max_length: int = 8192
    kv_heads: Optional[int] = 8

    arch = "text"

    @property
    def n_image_tokens(self) -> int:
        return 0

    def vision_param_entries(self):
        return [], []


def _no_training(what: str):
    raise NotImplementedError(f"TextLMModel.{what}: training a text-only model is not supported (inference only)")


class TextLMModel(LlavaDPOModel):
    def __init__(self, cfg: TextLMConfig, device="cuda:0", with_optimizer: bool = False, lora=None):
        if getattr(cfg, "arch", None) != "text":
            raise ValueError("TextLMModel needs a TextLMConfig")
        if with_optimizer or lora is not None:
            _no_training("__init__(with_optimizer=True / lora)")
        super().__init__(cfg, device=device, with_optimizer=False, lora=None)
        self.training = False

    # ---- no vision side
    def _load_tower(self, sd: Dict[str, torch.Tensor]):
        pass

    def _init_tower(self, g: torch.Generator, std: float):
        pass

    def clip_state_dict(self) -> Dict[str, torch.Tensor]:
        return {}

    def encode_images(self, pixels=None, ctx: Optional[dict] = None) -> torch.Tensor:
        """No image, no feature row: an empty [0, hidden] block (the splice then copies embedding rows only)."""
        if pixels is not None:
            raise ValueError("TextLMModel.encode_images: a text-only model takes no images")
        return torch.empty(0, self.cfg.hidden, dtype=BF16, device=self.device)

    # ---- inference only
    def train(self, mode: bool = True):
        if mode:
            _no_training("train")
        return super().train(False)

    def forward_logps(self, *a, **kw):
        _no_training("forward_logps")

    def backward(self, *a, **kw):
        _no_training("backward")

    def forward(self, *a, **kw):
        _no_training("forward")

    def forward_next_token_scores(self, *a, **kw):
        raise NotImplementedError("TextLMModel.forward_next_token_scores: the labeler's stage scores questions about an image")

    def beam_search(self, *a, **kw):
        raise NotImplementedError("TextLMModel.beam_search: beam search is not supported on a text-only model")
