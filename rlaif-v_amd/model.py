"""LLaVA-1.5 policy for the DPO step, executed entirely by the gfx950 kernels of librlaifv_hip.so.

This is the host-side mirror of the reference's model surface for the DPO path
(/root/reference llava/model/language_model/llava_llama.py:41-102, llava/model/llava_arch.py:141-330,
llava/model/multimodal_encoder/clip_encoder.py:36-58, llava/model/multimodal_projector/builder.py:39-46)
with a hand-written forward AND backward (no autograd): torch only owns device memory and streams.

Data layout in HBM:
  * all trainable parameters live in ONE flat bf16 buffer (``flat_p``) in *backward-completion order*
    (lm_head, layer L-1 .. layer 0, embed_tokens, projector, then the no-decay tail: norm gains and
    biases); ``flat_g`` (bf16 grads), ``flat_master``/``flat_m``/``flat_v`` (fp32) mirror it, so AdamW is
    two launches (decay / no-decay range) and data-parallel all-reduce buckets are contiguous slices
    that become ready in address order while backward is still running;
  * q/k/v and gate/up projections are stored adjacent so each is ONE GEMM ([3d,d] and [2f,d]);
  * every weight that a dgrad GEMM needs K-contiguous has a transposed bf16 copy in ``flat_pT``
    (refreshed after each optimizer step by rv_transpose), so every contraction is the NT kernel;
  * activations are token-major [S*L, features] bf16; per layer we keep x, qkv (post-RoPE), attention
    output, x_mid, gate/up and the fp32 rstd/lse rows; normalised inputs and SwiGLU outputs are
    recomputed in backward (HBM-cheap) rather than stored.
"""
from __future__ import annotations

import math
import os
from contextlib import contextmanager
from dataclasses import dataclass, field, replace
from typing import Dict, List, NamedTuple, Optional, Tuple

import torch

from . import ops
from .splice import (IMAGE_TOKEN_INDEX, SplicePlan, build_branch_plan, build_packed_plan, build_splice_plan, cut_behind_eos,
                     eos_id_set)

BF16 = torch.bfloat16
VT = "model.vision_tower.vision_tower.vision_model."


@dataclass
class LlavaConfig:
    """Same fields as the reference's checkpoint config (SURVEY.md section 8a notes)."""
    hidden: int = 4096
    layers: int = 32
    heads: int = 32
    ffn: int = 11008
    vocab: int = 32000
    rms_eps: float = 1e-5
    rope_theta: float = 10000.0
    clip_hidden: int = 1024
    clip_layers: int = 24
    clip_heads: int = 16
    clip_ffn: int = 4096
    image_size: int = 336
    patch: int = 14
    clip_eps: float = 1e-5
    select_layer: int = -2
    model_max_length: int = 2048
    pad_token_id: int = 0
    kv_heads: Optional[int] = None      # num_key_value_heads (Mistral / Llama-3 style GQA); None = heads (LLaVA-1.5: MHA)

    arch = "llava"                      # class attribute: "llava" (CLIP + mlp2x_gelu projector) | "omnilmm" (omnilmm.py)

    @property
    def vocab_padded(self) -> int:
        """Rows of embed_tokens / lm_head as stored: the tokenizer's vocabulary rounded up to the fused LM head's 64-column
        blocks.  The padding rows are zero, are never indexed, never enter the softmax (rv_lmhead_logp_* V_valid) and get
        zero gradient, so they stay zero under AdamW; HF tensors map to the first ``vocab`` rows."""
        return ops.round_up(self.vocab, 64)

    @property
    def n_image_tokens(self) -> int:
        """Sequence positions one image occupies after the splice."""
        return self.n_patches

    def vision_param_entries(self):
        """(decay weights, no-decay tensors) of the trainable vision-to-language adapter, each (key, shape, transposed copy),
        in backward-completion order.  LLaVA-1.5: the mlp2x_gelu projector (llava/model/multimodal_projector/builder.py)."""
        d, cd = self.hidden, self.clip_hidden
        return ([("model.mm_projector.2.weight", (d, d), True), ("model.mm_projector.0.weight", (d, cd), False)],
                [("model.mm_projector.2.bias", (d,), False), ("model.mm_projector.0.bias", (d,), False)])

    @property
    def head_dim(self) -> int:
        return self.hidden // self.heads

    @property
    def n_kv_heads(self) -> int:
        return self.heads if self.kv_heads is None else self.kv_heads

    @property
    def kv_dim(self) -> int:
        return self.n_kv_heads * self.head_dim

    @property
    def kv_group(self) -> int:
        return self.heads // self.n_kv_heads

    @property
    def clip_head_dim(self) -> int:
        return self.clip_hidden // self.clip_heads

    @property
    def n_patches(self) -> int:
        return (self.image_size // self.patch) ** 2

    @property
    def clip_layers_used(self) -> int:
        return self.select_layer if self.select_layer >= 0 else self.clip_layers + 1 + self.select_layer

    @property
    def patch_k(self) -> int:
        return ops.round_up(3 * self.patch * self.patch, 64)


@dataclass
class LoraConfig:
    """peft.LoraConfig as built by the reference's LoRA entry point (muffin/train/train_llava15_lora.py:304-318,
    flag defaults :111-116): every nn.Linear of the language model except lm_head (find_all_linear_names, :120-134)."""
    r: int = 64
    lora_alpha: int = 16
    lora_dropout: float = 0.05
    bias: str = "none"
    target_modules: Tuple[str, ...] = ("q_proj", "k_proj", "v_proj", "o_proj", "gate_proj", "up_proj", "down_proj")

    def __post_init__(self):
        if set(self.target_modules) != {"q_proj", "k_proj", "v_proj", "o_proj", "gate_proj", "up_proj", "down_proj"}:
            raise NotImplementedError("LoRA is applied to all seven decoder projections (find_all_linear_names)")
        if self.bias != "none":
            raise NotImplementedError("lora_bias other than 'none' (the reference's default) is not supported")

    @property
    def scaling(self) -> float:
        return self.lora_alpha / self.r

    @property
    def r_pad(self) -> int:
        """Stored rank: r rounded up to the GEMM K step (64); the padding rows/columns are zero and stay zero."""
        return ops.round_up(self.r, 64)


# fused projection -> (store suffix, peft module names in stacking order)
LORA_GROUPS = {"qkv": ("self_attn.q_proj", "self_attn.k_proj", "self_attn.v_proj"), "o": ("self_attn.o_proj",),
               "gu": ("mlp.gate_proj", "mlp.up_proj"), "down": ("mlp.down_proj",)}


def lora_group_rows(cfg: "LlavaConfig", grp: str) -> List[Tuple[int, int]]:
    """(first output row, rows) of every peft module inside a fused projection: q | k | v have widths hidden, kv_dim, kv_dim
    (grouped-query attention: kv_dim < hidden), gate | up are ffn each."""
    d, kvd, f = cfg.hidden, cfg.kv_dim, cfg.ffn
    return {"qkv": [(0, d), (d, kvd), (d + kvd, kvd)], "o": [(0, d)], "gu": [(0, f), (f, f)], "down": [(0, d)]}[grp]


# fused projection -> the slots (LlavaDPOModel._dropout_seed) of its adapter dropout masks: first the one of the mask the projection
# shares (under RV_LORA_PEFT_MASKS: of its first peft module - q, o, gate, down), then the layer's spare slots that k, v and up take then
LORA_SEED_SLOTS = {"qkv": (0, 4, 5), "o": (1,), "gu": (2, 6), "down": (3,)}


class LoraDrop(NamedTuple):       # the pass state: the adapter-dropout mode of ONE forward and of the backward that differentiates it
    p: float = 0.0               # peft lora_dropout in effect; 0.0 = no dropout (full fine-tune, eval mode, lora_dropout = 0)
    per_module: bool = False     # one mask per peft module (RV_LORA_PEFT_MASKS) instead of one per fused projection
    fused: bool = False          # the kernels that produce a projection's input also write its dropped copy
    step: int = 0                # the model's _dropout_step the pass ran at: seeds its masks (filled with or without dropout)


class ProjSaved(NamedTuple):      # what an adapter projection keeps for its backward
    t: torch.Tensor              # (alpha / r) dropout(x) A^T, the modules' blocks side by side
    xd: Optional[torch.Tensor]   # the dropped input under a shared mask (keep_dropped_inputs), else None: regenerated from the seed


def _is_decay(name: str) -> bool:
    return not (name.endswith("bias") or "norm" in name)


class ParamStore:
    """Flat parameter / gradient / optimizer-state buffers with named views."""

    def __init__(self, cfg: LlavaConfig, device, with_optimizer: bool = True, lora: Optional[LoraConfig] = None):
        d, f, V, cd, kvd = cfg.hidden, cfg.ffn, cfg.vocab_padded, cfg.clip_hidden, cfg.kv_dim
        if cfg.heads % cfg.n_kv_heads != 0:
            raise ValueError("kv_heads must divide heads")
        Entry = Tuple[str, Tuple[int, ...], bool]        # (key, shape, needs transposed copy); fused keys map to HF names
        self.lora = lora
        # Full fine-tune: the fused gate|up weight stores its rows INTERLEAVED (row 2j = gate_j, 2j+1 = up_j) so that the GEMM
        # epilogues can apply SwiGLU and its backward in registers (ops.linear_swiglu / linear_swiglu_bwd).  LoRA keeps
        # [gate | up] blocks (its adapter column groups address them).  RV_FUSE_SWIGLU=0: block layout + separate kernels.
        fuse = os.environ.get("RV_FUSE_SWIGLU", "1") != "0"
        # Round 6: adapter models can take the fused SwiGLU epilogues too (RV_LORA_FUSE_SWIGLU=1): the frozen gate|up weight AND the
        # rows of the gate|up adapter lora_B are stored interleaved, and the fused GEMM's adapter segment runs over BOTH modules'
        # t = x A^T columns against an EXPANDED lora_B^T whose zeros keep t_gate out of the up columns (``gu_bexp``).
        self.lora_il = lora is not None and fuse and os.environ.get("RV_LORA_FUSE_SWIGLU", "0") == "1"
        self.interleave_gu = fuse and (lora is None or self.lora_il)
        self.gu_bexp: Dict[int, torch.Tensor] = {}      # layer -> [2 r_pad, 2 ffn] expanded transposed gate|up adapter (lora_il only)
        proj_w, proj_b = cfg.vision_param_entries()
        self.vision_keys = [k for k, _, _ in proj_w + proj_b]
        base_w: List[Entry] = [("lm_head.weight", (V, d), True)]
        for i in reversed(range(cfg.layers)):
            base_w += [(f"layers.{i}.wdown", (d, f), True), (f"layers.{i}.wgu", (2 * f, d), True),
                       (f"layers.{i}.wo", (d, d), True), (f"layers.{i}.wqkv", (d + 2 * kvd, d), True)]
        base_w += [("model.embed_tokens.weight", (V, d), False)]
        norms: List[Entry] = [("model.norm.weight", (d,), False)]
        for i in reversed(range(cfg.layers)):
            norms += [(f"layers.{i}.ln2", (d,), False), (f"layers.{i}.ln1", (d,), False)]
        text_only = getattr(cfg, "arch", "llava") == "text"
        if text_only:
            # a text-only language model (textlm.py) is inference-only: nothing trainable, so no gradient or optimizer slot
            if lora is not None or with_optimizer:
                raise NotImplementedError("a text-only model (TextLMConfig) cannot be trained: build it with with_optimizer=False "
                                          "and without LoRA")
            frozen: List[Entry] = base_w + norms
            decay, nodecay = [], []
        elif lora is None:
            # full fine-tune: everything trainable, laid out in backward-completion order
            frozen = []
            decay = base_w + proj_w
            nodecay = norms + proj_b
        else:
            # LoRA: base language model frozen; adapters (backward-completion order) + projector trainable
            rp = lora.r_pad
            frozen = base_w + norms
            decay = []
            for i in reversed(range(cfg.layers)):
                decay += [(f"layers.{i}.lora_down.B", (d, rp), True), (f"layers.{i}.lora_down.A", (rp, f), True),
                          (f"layers.{i}.lora_gu.B", (2 * f, rp), True), (f"layers.{i}.lora_gu.A", (2 * rp, d), True),
                          (f"layers.{i}.lora_o.B", (d, rp), True), (f"layers.{i}.lora_o.A", (rp, d), True),
                          (f"layers.{i}.lora_qkv.B", (d + 2 * kvd, rp), True), (f"layers.{i}.lora_qkv.A", (3 * rp, d), True)]
            decay += proj_w
            nodecay = proj_b
        self.entries = frozen + decay + nodecay
        self.offsets: Dict[str, Tuple[int, Tuple[int, ...]]] = {}
        off = 0
        for k, shp, _ in self.entries:
            n = math.prod(shp)
            assert n % 8 == 0, (k, shp)
            self.offsets[k] = (off, shp)
            off += n
        self.n_total = off
        self.t0 = sum(math.prod(shp) for _, shp, _ in frozen)            # first trainable element of flat_p
        self.n_decay = sum(math.prod(shp) for _, shp, _ in decay)        # trainable elements with weight decay
        self.n_train = self.n_total - self.t0
        self.trainable = {k for k, _, _ in decay + nodecay}
        self.device = device
        self.flat_p = torch.zeros(self.n_total, dtype=BF16, device=device)
        self.train_p = self.flat_p[self.t0:]                             # the slice the optimizer owns
        self.flat_g = torch.zeros(self.n_train, dtype=BF16, device=device)
        if with_optimizer:
            self.flat_master = torch.zeros(self.n_train, dtype=torch.float32, device=device)
            self.flat_m = torch.zeros(self.n_train, dtype=torch.float32, device=device)
            self.flat_v = torch.zeros(self.n_train, dtype=torch.float32, device=device)
        else:
            self.flat_master = self.flat_m = self.flat_v = None
        # transposed copies: W [out, in] -> W^T [in, out]   (out is a multiple of 64 for every entry)
        self.t_offsets: Dict[str, Tuple[int, Tuple[int, int]]] = {}
        toff = 0
        for k, shp, tr in self.entries:
            if tr:
                assert shp[0] % 64 == 0, (k, shp)
                self.t_offsets[k] = (toff, (shp[1], shp[0]))
                toff += shp[0] * shp[1]
        self.flat_pT = torch.zeros(toff, dtype=BF16, device=device)
        # gradient buckets for data parallelism: contiguous slices of flat_g in the order backward finishes them
        self.buckets: Dict[str, Tuple[int, int]] = {}
        if text_only:
            pass
        elif lora is None:
            self.buckets["lm_head"] = self.grad_range("lm_head.weight", "lm_head.weight")
            for i in reversed(range(cfg.layers)):
                self.buckets[f"layer{i}"] = self.grad_range(f"layers.{i}.wdown", f"layers.{i}.wqkv")
            self.buckets["embed_proj"] = self.grad_range("model.embed_tokens.weight", proj_w[-1][0])
        else:
            for i in reversed(range(cfg.layers)):
                self.buckets[f"layer{i}"] = self.grad_range(f"layers.{i}.lora_down.B", f"layers.{i}.lora_qkv.A")
            self.buckets["embed_proj"] = self.grad_range(proj_w[0][0], proj_w[-1][0])
        self.buckets["nodecay"] = (self.n_decay, self.n_train)

    def bucket_schedule(self) -> List[Tuple[str, int, int]]:
        """(name, start, end) in the order LlavaDPOModel.backward fires grad_ready_hook; covers flat_g exactly."""
        return [(k, a, b) for k, (a, b) in self.buckets.items()]

    def p(self, key: str) -> torch.Tensor:
        off, shp = self.offsets[key]
        return self.flat_p[off:off + math.prod(shp)].view(*shp)

    def g(self, key: str) -> torch.Tensor:
        off, shp = self.offsets[key]
        if key not in self.trainable:
            raise KeyError(f"{key} is frozen: it has no gradient slot")
        off -= self.t0
        return self.flat_g[off:off + math.prod(shp)].view(*shp)

    def pT(self, key: str) -> torch.Tensor:
        off, shp = self.t_offsets[key]
        return self.flat_pT[off:off + shp[0] * shp[1]].view(*shp)

    def grad_range(self, first_key: str, last_key: str) -> Tuple[int, int]:
        """[start, end) inside flat_g (offsets relative to the first trainable element)."""
        a = self.offsets[first_key][0]
        off, shp = self.offsets[last_key]
        return a - self.t0, off + math.prod(shp) - self.t0

    def refresh_transposes(self, trainable_only: bool = False):
        """W^T copies; after an optimizer step only the trainable ones moved (LoRA: 160 MB instead of 13 GB)."""
        for k in self.t_offsets:
            if not trainable_only or k in self.trainable:
                ops.transpose(self.p(k), out=self.pT(k))
        if self.lora_il:
            self.refresh_gu_bexp()

    def refresh_gu_bexp(self):
        """lora_il: the expanded transposed gate|up adapter of every layer from its (row-interleaved) lora_B: rows 0..rp-1 =
        lora_B(gate)^T on the even columns, rows rp..2rp-1 = lora_B(up)^T on the odd columns, zeros elsewhere (plumbing: 64
        strided device copies of 2.8 MB per optimizer step)."""
        rp = self.lora.r_pad
        for key in self.t_offsets:
            if not key.endswith("lora_gu.B"):
                continue
            i = int(key.split(".")[1])
            BT = self.pT(key)                                   # [rp, 2f]: column 2j = lora_B(gate)[j], 2j + 1 = lora_B(up)[j]
            e = self.gu_bexp.get(i)
            if e is None:
                e = self.gu_bexp[i] = torch.zeros(2 * rp, BT.shape[1], dtype=BT.dtype, device=BT.device)
            e[:rp, 0::2].copy_(BT[:, 0::2])
            e[rp:, 1::2].copy_(BT[:, 1::2])

    def sync_master_from_params(self):
        if self.flat_master is not None:
            self.flat_master.copy_(self.train_p)     # bf16 -> fp32 (device copy, plumbing)
        if getattr(self, "sharded_optimizer", None) is not None:
            self.sharded_optimizer.sync_master_from_params()      # opt-in ZeRO-1: the fp32 masters live in the trainer's shards

    # ---- HF state-dict mapping ------------------------------------------------------------
    def hf_slices(self, cfg: LlavaConfig) -> Dict[str, Tuple[str, int, int, int]]:
        """HF name -> (store key, first row, n rows, row step) for the language model + projector: the HF tensor is
        ``rows(view(key), r0, n, step)`` (step 2 = the interleaved gate / up rows of the fused MLP weight)."""
        d, f, kvd = cfg.hidden, cfg.ffn, cfg.kv_dim
        m: Dict[str, Tuple[str, int, int, int]] = {}
        il = self.interleave_gu
        for i in range(cfg.layers):
            p = f"model.layers.{i}."
            m[p + "self_attn.q_proj.weight"] = (f"layers.{i}.wqkv", 0, d, 1)
            m[p + "self_attn.k_proj.weight"] = (f"layers.{i}.wqkv", d, kvd, 1)
            m[p + "self_attn.v_proj.weight"] = (f"layers.{i}.wqkv", d + kvd, kvd, 1)
            m[p + "self_attn.o_proj.weight"] = (f"layers.{i}.wo", 0, d, 1)
            m[p + "mlp.gate_proj.weight"] = (f"layers.{i}.wgu", 0, f, 2) if il else (f"layers.{i}.wgu", 0, f, 1)
            m[p + "mlp.up_proj.weight"] = (f"layers.{i}.wgu", 1, f, 2) if il else (f"layers.{i}.wgu", f, f, 1)
            m[p + "mlp.down_proj.weight"] = (f"layers.{i}.wdown", 0, d, 1)
            m[p + "input_layernorm.weight"] = (f"layers.{i}.ln1", 0, d, 1)
            m[p + "post_attention_layernorm.weight"] = (f"layers.{i}.ln2", 0, d, 1)
        for k in ["lm_head.weight", "model.embed_tokens.weight", "model.norm.weight"] + self.vision_keys:
            m[k] = (k, 0, cfg.vocab if k in ("lm_head.weight", "model.embed_tokens.weight") else self.offsets[k][1][0], 1)
        return m

    @staticmethod
    def rows(view: torch.Tensor, r0: int, n: int, step: int = 1) -> torch.Tensor:
        """Rows r0, r0 + step, ... (n of them) of a store view."""
        return view[r0:r0 + n * step:step]


    @staticmethod
    def lora_view(t: torch.Tensor, r0: int, n: int, ncol: int, step: int = 1) -> torch.Tensor:
        """The peft tensor inside a store view: rows r0, r0 + step, ... (n of them), first ncol columns."""
        return t[r0:r0 + n * step:step, :ncol]

    def lora_slices(self, cfg: LlavaConfig) -> Dict[str, Tuple[str, int, int, int, int]]:
        """peft adapter name (without the 'base_model.model.' prefix) -> (store key, first row, n rows, n cols, row step); the
        tensor is ``lora_view(view(key), r0, n, ncol, step)`` (step 2 = the interleaved gate / up rows of lora_il's lora_gu.B)."""
        m: Dict[str, Tuple[str, int, int, int, int]] = {}
        if self.lora is None:
            return m
        r, rp, d, f = self.lora.r, self.lora.r_pad, cfg.hidden, cfg.ffn
        in_cols = {"qkv": d, "o": d, "gu": d, "down": f}
        for i in range(cfg.layers):
            for grp, mods in LORA_GROUPS.items():
                for gi, (mod, (r0, rows)) in enumerate(zip(mods, lora_group_rows(cfg, grp))):
                    p = f"model.layers.{i}.{mod}."
                    m[p + "lora_A.weight"] = (f"layers.{i}.lora_{grp}.A", gi * rp, r, in_cols[grp], 1)
                    if grp == "gu" and self.lora_il:
                        m[p + "lora_B.weight"] = (f"layers.{i}.lora_{grp}.B", gi, rows, r, 2)
                    else:
                        m[p + "lora_B.weight"] = (f"layers.{i}.lora_{grp}.B", r0, rows, r, 1)
        return m


@dataclass
class StepOutput:
    """What one DPO forward produced (all device tensors; nothing is synced to the host)."""
    loss: torch.Tensor                 # 0-d fp32
    scalars: torch.Tensor              # [8] see rv_dpo_loss
    per_pair: torch.Tensor             # [5, B]
    seq_logp: torch.Tensor             # [2B] sum of target log-probs (log_prob of get_batch_logps)
    seq_cnt: torch.Tensor              # [2B] number of targets
    per_token_logp: torch.Tensor       # [n_sel] fp32, selected rows only
    plan: SplicePlan = None
    ctx: dict = field(default_factory=dict)


class LlavaDPOModel:
    """Mirror of ``LlavaLlamaForCausalLM`` for the DPO call pattern of
    ``get_beta_and_logps`` (muffin/train/trainers.py:161-275): images -> CLIP (frozen) -> projector ->
    splice -> Llama stack -> fused LM-head log-probs -> DPO loss, plus the matching backward."""

    def __init__(self, cfg: LlavaConfig, device="cuda:0", with_optimizer: bool = True,
                 lora: Optional[LoraConfig] = None):
        if not torch.cuda.is_available():
            raise RuntimeError("LlavaDPOModel needs an MI355X (HIP) device; there is no CPU fallback")
        self.cfg = cfg
        self.device = torch.device(device)
        self.lora = lora
        self.store = ParamStore(cfg, self.device, with_optimizer, lora)
        self._dropout_step = 0          # advances once per training forward: seeds the LoRA dropout masks
        self._cur_drop = LoraDrop()     # the pass state of the forward / backward in flight (_begin_pass)
        # keep the dropped adapter inputs for backward (+1.3 GB per layer at 27 k tokens) instead of regenerating them
        self.keep_dropped_inputs = os.environ.get("RV_LORA_KEEP_DROPPED", "1") != "0"
        # keep normalised inputs and SwiGLU outputs for backward instead of recomputing them (RV_KEEP_RECOMPUTABLE=0:
        # the lean layout, 1.05 GB / layer less at 27 k tokens)
        self.keep_recomputable = os.environ.get("RV_KEEP_RECOMPUTABLE", "1") != "0"
        # --gradient_checkpointing (script/train/llava15_train.sh:39): keep only each decoder layer's input and re-run the
        # layer in backward.  Off by default: 288 GB holds 8 pairs x 2048 tokens without it.
        self.gradient_checkpointing = False
        self.clip: Dict[str, torch.Tensor] = {}
        self.training = True
        self._rope_cache: Optional[Tuple[int, torch.Tensor, torch.Tensor]] = None     # ONE table, grown geometrically
        self.dropout_rank = 0           # data-parallel rank: mixed into the LoRA dropout seeds (set by the trainer)
        self.grad_ready_hook = None     # callable(name, start, end) fired when a slice of flat_g is final
        # compute the prefix shared by the chosen and rejected sequence of a pair once (splice.build_packed_plan)
        self.share_prefix = os.environ.get("RV_SHARE_PREFIX", "1") != "0"
        # packed rows are concatenated without inter-row padding (splice.build_packed_plan pad_free; RV_PAD_FREE=0: every packed
        # row right-padded to the longest, the round-1..4 layout).  Log-probs are bit-identical either way (SURVEY 8a property (i))
        self.pad_free = os.environ.get("RV_PAD_FREE", "1") != "0"
        # The DECODER's residual stream in fp32 - DEFAULT for the full fine-tune since round 6 (RV_RESID_FP32=0 restores the bf16
        # stream; LoRA runs keep bf16: their fixtures were validated that way and the producer-side dropout kernels write bf16).
        # o_proj / down_proj write their branch in bf16 without the residual operand; rv_rmsnorm_fwd_f32 adds it to the fp32 stream
        # and normalises in one pass.  Decided on round 6's evidence (profiles/r06_cfg1_step_numerics.json): with
        # SwiGLU and RoPE taken from fp32 accumulators the stream is what is left - per-token RMS error 0.035 -> 0.027 at 32 layers
        # (the HF-style bf16 emulation: 0.053), and BASELINE config 1's literal batch - whose 1e-3 loss bar is a fraction of a sigma
        # of ANY bf16 forward - lands at 4.2e-4 with it and at 2.6e-3 ... 3.9e-3 without.  Price: +1.1 % step time, +14 GB.
        env = os.environ.get("RV_RESID_FP32")
        self.resid_fp32 = (env != "0") if env not in (None, "") else (lora is None)
        # OPT-IN: peft's dropout semantics to the letter (RV_LORA_PEFT_MASKS=1): peft wraps every nn.Linear in its own lora.Linear with
        # its OWN nn.Dropout, so q / k / v (and gate / up) draw INDEPENDENT masks of the same input.  The default fuses them: one
        # dropped input per fused projection (same marginals, one pass over the activation instead of three).  See LORA_SEED_SLOTS.
        self.lora_peft_masks = os.environ.get("RV_LORA_PEFT_MASKS", "0") != "0"
        # LoRA under a shared adapter-dropout mask: the kernels that produce a projection's input also write its dropped copy (one
        # pass less over the activation per projection; the attention output keeps the stand-alone rv_dropout)
        self.lora_fused_dropout = os.environ.get("RV_LORA_FUSED_DROPOUT", "1") != "0"
        self.clip_fp32_resid = os.environ.get("RV_CLIP_FP32_RESID", "1") != "0"      # default ON since round 5, see clip_features
        self.fuse_rope_bwd = os.environ.get("RV_FUSE_ROPE_BWD", "1") != "0"
        self.fuse_rope_fwd = os.environ.get("RV_FUSE_ROPE_FWD", "1") != "0"      # RoPE in the q|k|v GEMM epilogue (ops.linear_rope)

    # ------------------------------------------------------------------ weights
    def load_state_dict(self, sd: Dict[str, torch.Tensor]):
        """HF-named fp32/bf16 CPU tensors (the reference's checkpoint layout, 4.35 CLIP key names)."""
        cfg, st = self.cfg, self.store
        for name, (key, r0, n, step) in st.hf_slices(cfg).items():
            st.rows(st.p(key), r0, n, step).copy_(sd[name].to(BF16))
        if self.lora is not None:
            self.load_lora_state_dict(sd, strict=False, _refresh=False)
        st.sync_master_from_params()
        st.refresh_transposes()
        self._load_tower(sd)

    def _load_tower(self, sd: Dict[str, torch.Tensor]):
        """The frozen CLIP-ViT-L/14 tower (llava/model/multimodal_encoder/clip_encoder.py) into device tensors."""
        cfg = self.cfg
        self._clip_raw = {k: v.detach().to(BF16).cpu() for k, v in sd.items() if k.startswith(VT)}
        cd, Kp = cfg.clip_hidden, cfg.patch_k

        def dev(t):
            return t.to(BF16).to(self.device).contiguous()

        c = self.clip
        pw = torch.zeros(cd, Kp, dtype=BF16)
        pw[:, :3 * cfg.patch * cfg.patch] = sd[VT + "embeddings.patch_embedding.weight"].reshape(cd, -1).to(BF16)
        c["patch_w"] = pw.to(self.device)
        c["cls"] = dev(sd[VT + "embeddings.class_embedding"])
        c["pos"] = dev(sd[VT + "embeddings.position_embedding.weight"])
        c["pre_ln_w"], c["pre_ln_b"] = dev(sd[VT + "pre_layrnorm.weight"]), dev(sd[VT + "pre_layrnorm.bias"])
        for i in range(cfg.clip_layers_used):
            p = VT + f"encoder.layers.{i}."
            c[f"{i}.wqkv"] = dev(torch.cat([sd[p + f"self_attn.{n}_proj.weight"] for n in "qkv"], 0))
            c[f"{i}.bqkv"] = dev(torch.cat([sd[p + f"self_attn.{n}_proj.bias"] for n in "qkv"], 0))
            c[f"{i}.wo"], c[f"{i}.bo"] = dev(sd[p + "self_attn.out_proj.weight"]), dev(sd[p + "self_attn.out_proj.bias"])
            for ln in ("layer_norm1", "layer_norm2"):
                c[f"{i}.{ln}.w"], c[f"{i}.{ln}.b"] = dev(sd[p + ln + ".weight"]), dev(sd[p + ln + ".bias"])
            c[f"{i}.fc1.w"], c[f"{i}.fc1.b"] = dev(sd[p + "mlp.fc1.weight"]), dev(sd[p + "mlp.fc1.bias"])
            c[f"{i}.fc2.w"], c[f"{i}.fc2.b"] = dev(sd[p + "mlp.fc2.weight"]), dev(sd[p + "mlp.fc2.bias"])

    def init_random(self, seed: int = 0, std: float = 0.02, lora_b_std: Optional[float] = None):
        """HF-default style random init directly on the device (no checkpoints exist offline)."""
        cfg, st = self.cfg, self.store
        g = torch.Generator(device=self.device).manual_seed(seed)
        chunk = 1 << 26
        for k, shp, _ in st.entries:
            off, n = st.offsets[k][0], math.prod(shp)
            if ".lora_" in k or k.endswith("bias"):
                continue                                        # adapters: reset_lora_parameters below; biases stay 0
            if len(shp) == 1:
                st.flat_p[off:off + n] = 1.0                    # norm gains
                continue
            for a in range(off, off + n, chunk):
                b = min(off + n, a + chunk)
                st.flat_p[a:b] = (torch.randn(b - a, device=self.device, generator=g) * std).to(BF16)
        if self.lora is not None:
            self.reset_lora_parameters(seed + 1, lora_b_std)
        if cfg.vocab_padded != cfg.vocab:                       # vocabulary padding rows are zero (LlavaConfig.vocab_padded)
            st.p("lm_head.weight")[cfg.vocab:].zero_()
            st.p("model.embed_tokens.weight")[cfg.vocab:].zero_()
        st.sync_master_from_params()
        st.refresh_transposes()
        self._init_tower(g, std)

    def _init_tower(self, g: torch.Generator, std: float):
        cfg = self.cfg
        cd, Kp = cfg.clip_hidden, cfg.patch_k

        def rn(*shape, s=std):
            return (torch.randn(*shape, device=self.device, generator=g) * s).to(BF16)

        c = self.clip
        c["patch_w"] = rn(cd, Kp)
        c["patch_w"][:, 3 * cfg.patch * cfg.patch:] = 0
        c["cls"], c["pos"] = rn(cd), rn(cfg.n_patches + 1, cd)
        c["pre_ln_w"], c["pre_ln_b"] = torch.ones(cd, dtype=BF16, device=self.device), torch.zeros(cd, dtype=BF16, device=self.device)
        for i in range(cfg.clip_layers_used):
            c[f"{i}.wqkv"], c[f"{i}.bqkv"] = rn(3 * cd, cd), rn(3 * cd)
            c[f"{i}.wo"], c[f"{i}.bo"] = rn(cd, cd), rn(cd)
            for ln in ("layer_norm1", "layer_norm2"):
                c[f"{i}.{ln}.w"] = torch.ones(cd, dtype=BF16, device=self.device)
                c[f"{i}.{ln}.b"] = torch.zeros(cd, dtype=BF16, device=self.device)
            c[f"{i}.fc1.w"], c[f"{i}.fc1.b"] = rn(cfg.clip_ffn, cd), rn(cfg.clip_ffn)
            c[f"{i}.fc2.w"], c[f"{i}.fc2.b"] = rn(cd, cfg.clip_ffn), rn(cd)

    def state_dict(self) -> Dict[str, torch.Tensor]:
        """HF-named CPU bf16 tensors of the trainable part (safe_save_model_for_hf_trainer layout,
        muffin/train/train_llava15.py:102-112)."""
        out = {}
        for name, (key, r0, n, step) in self.store.hf_slices(self.cfg).items():
            out[name] = self.store.rows(self.store.p(key), r0, n, step).detach().cpu().clone()
        return out

    # ---- LoRA adapters (peft naming, muffin/train/train_llava15_lora.py:152-197) ----------------
    def reset_lora_parameters(self, seed: int = 1, b_std: Optional[float] = None):
        """peft LoraLayer.reset_lora_parameters: lora_A ~ kaiming_uniform(a=sqrt(5)) = U(-1/sqrt(in), 1/sqrt(in)),
        lora_B = 0 (b_std: draw B ~ N(0, b_std) instead - tests and benchmarks that want a non-trivial adapter)."""
        st, g = self.store, torch.Generator(device=self.device).manual_seed(seed)
        for name, (key, r0, n, ncol, step) in st.lora_slices(self.cfg).items():
            view = st.lora_view(st.p(key), r0, n, ncol, step)
            if name.endswith("lora_A.weight"):
                bound = 1.0 / math.sqrt(ncol)
                view.copy_(((torch.rand(n, ncol, device=self.device, generator=g) * 2 - 1) * bound).to(BF16))
            elif b_std is None:
                view.zero_()
            else:
                view.copy_((torch.randn(n, ncol, device=self.device, generator=g) * b_std).to(BF16))

    def load_lora_state_dict(self, sd: Dict[str, torch.Tensor], strict: bool = True, _refresh: bool = True):
        """Adapter tensors under peft names, with or without the 'base_model.model.' prefix / '.default' infix."""
        st = self.store
        norm = {k.replace("base_model.model.", "").replace(".default.", "."): v for k, v in sd.items() if ".lora_" in k}
        found = 0
        for name, (key, r0, n, ncol, step) in st.lora_slices(self.cfg).items():
            if name in norm:
                st.lora_view(st.p(key), r0, n, ncol, step).copy_(norm[name].to(BF16))
                found += 1
            elif strict:
                raise KeyError(f"adapter tensor {name} missing")
        if found == 0 and not strict:
            self.reset_lora_parameters()
        if _refresh:
            st.sync_master_from_params()
            st.refresh_transposes(trainable_only=True)

    def lora_state_dict(self, grads: bool = False) -> Dict[str, torch.Tensor]:
        """What get_peft_state_maybe_zero_3(named_parameters(), 'none') collects: 'base_model.model.<module>.lora_X.weight'."""
        st, out = self.store, {}
        for name, (key, r0, n, ncol, step) in st.lora_slices(self.cfg).items():
            src = st.g(key) if grads else st.p(key)
            t = st.lora_view(src, r0, n, ncol, step).detach()
            out["base_model.model." + name] = t.float().cpu() if grads else t.cpu().clone()
        return out

    def non_lora_trainables(self) -> Dict[str, torch.Tensor]:
        """get_peft_state_non_lora_maybe_zero_3: the trainable non-adapter tensors = the projector."""
        return {"base_model.model." + k: self.store.p(k).detach().cpu().clone() for k in self.store.trainable
                if "mm_projector" in k}

    def merge_lora(self):
        """peft merge_and_unload (llava/model/builder.py:81-85): W += (alpha/r) B A for every adapted projection, on
        the device; the adapters are zeroed afterwards (B = 0 makes them the identity)."""
        if self.lora is None:
            return
        st, cfg, rp, sc = self.store, self.cfg, self.lora.r_pad, self.lora.scaling
        for i in range(cfg.layers):
            for grp in LORA_GROUPS:
                W, B, AT = st.p(f"layers.{i}.w{grp}"), st.p(f"layers.{i}.lora_{grp}.B"), st.pT(f"layers.{i}.lora_{grp}.A")
                if grp == "gu" and st.lora_il:
                    # interleaved rows: W[2j + gi] += sc B[2j + gi] A_gi - one GEMM per module on contiguous copies (a one-off)
                    for gi in range(2):
                        Wg = W[gi::2].contiguous()
                        ops.gemm_nt(B[gi::2].contiguous(), AT[:, gi * rp:(gi + 1) * rp].contiguous(), out=Wg, residual=Wg, alpha=sc)
                        W[gi::2].copy_(Wg)
                    B.zero_()
                    continue
                for gi, (r0, rows) in enumerate(lora_group_rows(cfg, grp)):
                    Wg = W[r0:r0 + rows]
                    ops.gemm_nt(B[r0:r0 + rows], AT[:, gi * rp:(gi + 1) * rp], out=Wg, residual=Wg, alpha=sc)
                B.zero_()
        st.sync_master_from_params()
        st.refresh_transposes()

    def clip_state_dict(self) -> Dict[str, torch.Tensor]:
        """The frozen tower under its checkpoint key names (kept from load_state_dict; empty after init_random)."""
        return dict(getattr(self, "_clip_raw", {}))

    def grads_state_dict(self) -> Dict[str, torch.Tensor]:
        out = {}
        for name, (key, r0, n, step) in self.store.hf_slices(self.cfg).items():
            if key in self.store.trainable:
                out[name] = self.store.rows(self.store.g(key), r0, n, step).detach().float().cpu()
        for name, t in self.lora_state_dict(grads=True).items():
            out[name.replace("base_model.model.", "")] = t
        return out

    def train(self, mode: bool = True):
        self.training = mode
        return self

    def eval(self):
        return self.train(False)

    # ------------------------------------------------------------------ vision
    def _rope(self, L: int):
        """cos/sin rows 0..L-1.  The kernels index the table by position, so one table for the largest length seen so far
        serves every batch (a table per distinct L would grow without bound with ragged / packed batches)."""
        if self._rope_cache is None or self._rope_cache[0] < L:
            n = max(L, self.cfg.model_max_length, 2 * self._rope_cache[0] if self._rope_cache else 0)
            self._rope_cache = (n,) + ops.rope_tables(n, self.cfg.head_dim, self.cfg.rope_theta, self.device)
        return self._rope_cache[1], self._rope_cache[2]

    def clip_features(self, pixels: torch.Tensor) -> torch.Tensor:
        """CLIPVisionTower.forward + feature_select('patch') (clip_encoder.py:36-58): [B*P, clip_hidden]."""
        cfg, c = self.cfg, self.clip
        if isinstance(pixels, (list, tuple)) or pixels.dtype == torch.uint8:
            # raw decoded images (uint8 HWC, any sizes): CLIPImageProcessor's resize / crop / normalise on the device
            from .image import clip_preprocess_batch
            pixels = clip_preprocess_batch(pixels, size=cfg.image_size, device=self.device)
        B = pixels.shape[0]
        P, T, cd, H, hd = cfg.n_patches, cfg.n_patches + 1, cfg.clip_hidden, cfg.clip_heads, cfg.clip_head_dim
        px = pixels.to(self.device, dtype=torch.float32).contiguous()
        cols = ops.im2col_patches(px, cfg.patch, cfg.patch_k)
        pe = ops.gemm_nt(cols, c["patch_w"])
        x = ops.clip_assemble(pe, c["cls"], c["pos"], B, P)
        x = ops.layernorm_fwd(x, c["pre_ln_w"], c["pre_ln_b"], cfg.clip_eps)
        if self.clip_fp32_resid:
            # The frozen tower's RESIDUAL STREAM in fp32 (default since round 5; RV_CLIP_FP32_RESID=0 = the bf16 stream): the 47 bf16 roundings of x on the way
            # through 23 layers are 84 % of the vision front's share - 27 % of the whole - of the per-token log-prob error variance
            # (profiles/r05_rounding_attribution.json), and the tower is 0.6 % of the step.  Every MFMA operand stays
            # bf16 (LayerNorm outputs, q / k / v, attention output, quick_gelu(fc1)); only out_proj / fc2 accumulate into an fp32 x.
            x = ops.cast_bf16_to_f32(x)
            norm = ops.layernorm_fwd_f32in
            add_branch = ops.gemm_nt_f32res                     # x += a W^T + bias, in place
        else:
            norm = ops.layernorm_fwd

            def add_branch(a, w, bias, x):
                return ops.gemm_nt(a, w, bias=bias, residual=x)
        for i in range(cfg.clip_layers_used):
            h = norm(x, c[f"{i}.layer_norm1.w"], c[f"{i}.layer_norm1.b"], cfg.clip_eps)
            qkv = ops.gemm_nt(h, c[f"{i}.wqkv"], bias=c[f"{i}.bqkv"])
            a, _ = ops.attn_fwd(qkv, B, T, H, hd, False, 0, cd, 2 * cd)
            x = add_branch(a, c[f"{i}.wo"], c[f"{i}.bo"], x)
            h = norm(x, c[f"{i}.layer_norm2.w"], c[f"{i}.layer_norm2.b"], cfg.clip_eps)
            h = ops.gemm_nt(h, c[f"{i}.fc1.w"], bias=c[f"{i}.fc1.b"], act=ops.ACT_QUICK_GELU)
            x = add_branch(h, c[f"{i}.fc2.w"], c[f"{i}.fc2.b"], x)
        if self.clip_fp32_resid:
            x = ops.cast_f32_to_bf16(x)              # hidden_states[-2] as the projector's bf16 GEMM operand: one rounding
        idx = (torch.arange(B, device=self.device)[:, None] * T + 1 + torch.arange(P, device=self.device)[None]).reshape(-1)
        return ops.gather_rows(x, idx.to(torch.int32))

    def encode_images(self, pixels: torch.Tensor, ctx: Optional[dict] = None) -> torch.Tensor:
        """llava_arch.py:141-148.  One pass per PAIR (the reference encodes [images, images],
        trainers.py:190; rows i and B+i are identical, so the pair shares one feature block)."""
        st = self.store
        f_clip = self.clip_features(pixels)
        z1 = ops.gemm_nt(f_clip, st.p("model.mm_projector.0.weight"), bias=st.p("model.mm_projector.0.bias"))
        h1 = ops.gelu_fwd(z1)
        feats = ops.gemm_nt(h1, st.p("model.mm_projector.2.weight"), bias=st.p("model.mm_projector.2.bias"))
        if ctx is not None:
            ctx.update(f_clip=f_clip, z1=z1, h1=h1)
        return feats

    def _vision_backward(self, dfeat: torch.Tensor, ctx: dict):
        """Autograd of the mlp2x_gelu projector (the CLIP tower is frozen: llava_arch.py:141-148, train_llava15.py:268)."""
        st = self.store
        ops.colsum(dfeat, out=st.g("model.mm_projector.2.bias"))
        ops.gemm_tn(dfeat, ctx["h1"], out=st.g("model.mm_projector.2.weight"))
        dh1 = ops.gemm_nt(dfeat, st.pT("model.mm_projector.2.weight"))
        dz1 = ops.gelu_bwd(dh1, ctx["z1"])
        ops.colsum(dz1, out=st.g("model.mm_projector.0.bias"))
        ops.gemm_tn(dz1, ctx["f_clip"], out=st.g("model.mm_projector.0.weight"))

    def _row_splicer(self):
        """Row-level splice rule handed to the planners (None = LLaVA's expanding <image> splice, splice._splice_rows)."""
        return None

    @property
    def splice_keeps_positions(self) -> bool:
        """True when the image splice leaves every text token at its position (OmniLMM replaces the <im_patch> embeddings in
        place): the precondition of the generic get_beta_and_logps branch and of token-weighted DPO."""
        return bool(getattr(self._row_splicer(), "keeps_positions", False))

    # ------------------------------------------------------------------ decoder projections (+ LoRA)
    def _lora_grouping(self, grp: str) -> Tuple[int, int]:
        """(group_cols, group0) of the fused LoRA GEMM for a fused projection (rv_gemm_nt_lora_bf16)."""
        cfg = self.cfg
        if grp == "qkv":
            return cfg.kv_dim, (cfg.hidden if cfg.kv_dim != cfg.hidden else 0)
        return (cfg.ffn, 0) if grp == "gu" else (0, 0)

    def _begin_pass(self, advance: bool = False) -> LoraDrop:
        """The state of the forward that starts now, stored as ``_cur_drop``: the dropout step (``advance``: of a new training step)
        and the adapter-dropout mode (peft lora_dropout: adapter models in training mode only).  It travels in the forward's context:
        backward and a checkpointed layer's re-run follow it, whatever happened to the model in between."""
        if advance:
            self._dropout_step += 1
        drop = LoraDrop(step=self._dropout_step)
        if self.lora is not None and self.training and self.lora.lora_dropout > 0.0:
            fused = self.lora_fused_dropout and not self.lora_peft_masks
            if fused and self.resid_fp32:
                raise NotImplementedError("RV_RESID_FP32 with the producer-side LoRA dropout kernels (set RV_LORA_FUSED_DROPOUT=0)")
            drop = drop._replace(p=self.lora.lora_dropout, per_module=self.lora_peft_masks, fused=fused)
        self._cur_drop = drop
        return drop

    @contextmanager
    def _eval_mode(self):
        """Eval mode for a forward-only surface; the caller's mode comes back afterwards."""
        was_training = self.training
        self.eval()
        try:
            yield
        finally:
            self.train(was_training)

    def _dropout_seed(self, layer: int, slot: int) -> int:
        return (self._cur_drop.step * 1000003 + self.dropout_rank * 7919 + layer * 8 + slot) & 0x7FFFFFFF

    def _lora_mask(self, layer: int, grp: str) -> Tuple[float, int]:
        """(p, seed) of the mask a fused projection's adapter input shares; (0.0, 0) without dropout."""
        p = self._cur_drop.p
        return (p, self._dropout_seed(layer, LORA_SEED_SLOTS[grp][0])) if p else (0.0, 0)

    def _module_seeds(self, layer: int, grp: str) -> List[int]:
        """RV_LORA_PEFT_MASKS: the seed of every peft module of a fused projection, in stacking order."""
        return [self._dropout_seed(layer, slot) for slot in LORA_SEED_SLOTS[grp]]

    def _proj_fwd(self, x: torch.Tensor, i: int, grp: str, residual: Optional[torch.Tensor] = None, xd: Optional[torch.Tensor] = None):
        """y = x W^T (+ residual); with adapters  y = x W^T + t B^T,  t = (alpha/r) dropout(x) A^T  (peft
        lora.Linear.forward) - the adapter term rides in the same K loop (rv_gemm_nt_lora_bf16).  Returns (y, ProjSaved or None).
        ``xd``: dropout(x) under the projection's shared mask when the kernel that produced x wrote it already (LoraDrop.fused)."""
        st = self.store
        W = st.p(f"layers.{i}.w{grp}")
        if self.lora is None:
            return ops.linear(x, W, st.pT(f"layers.{i}.w{grp}"), residual=residual), None
        saved = self._lora_t(x, i, grp, xd)
        gc, g0 = self._lora_grouping(grp)
        y = ops.linear_lora(x, W, st.pT(f"layers.{i}.w{grp}"), saved.t, st.p(f"layers.{i}.lora_{grp}.B"),
                            st.pT(f"layers.{i}.lora_{grp}.B"), group_cols=gc, residual=residual, group0=g0)
        return y, saved

    def _lora_t(self, x: torch.Tensor, i: int, grp: str, xd: Optional[torch.Tensor] = None) -> ProjSaved:
        """t = [t_0 | .. | t_{G-1}], t_g = (alpha / r) dropout(x) A_g^T, of a fused projection in any dropout mode (+ what backward keeps)."""
        drop, rp, sc = self._cur_drop, self.lora.r_pad, self.lora.scaling
        A = self.store.p(f"layers.{i}.lora_{grp}.A")
        if not drop.per_module:
            if xd is None and drop.p:
                xd = ops.dropout(x, *self._lora_mask(i, grp))
            t = ops.gemm_nt(x if xd is None else xd, A, alpha=sc)
            return ProjSaved(t, xd if self.keep_dropped_inputs else None)
        # one independent mask per peft module: one kernel that reads x once and draws every module's mask on the operand it holds
        # (rv_gemm_nt_lora_masks_bf16).  Shapes it does not serve: a dropped copy and a skinny GEMM per module.
        seeds = self._module_seeds(i, grp)
        if ops.lora_module_masks_ok(x.shape[1], rp):
            return ProjSaved(ops.lora_down_module_masks(x, A, drop.p, seeds, alpha=sc), None)
        t = torch.empty(x.shape[0], len(seeds) * rp, dtype=BF16, device=self.device)
        for g, seed in enumerate(seeds):
            ops.gemm_nt(ops.dropout(x, drop.p, seed), A[g * rp:(g + 1) * rp], out=t[:, g * rp:(g + 1) * rp], alpha=sc)
        return ProjSaved(t, None)

    def _proj_bwd(self, dy: torch.Tensor, xin: torch.Tensor, saved: Optional[ProjSaved], i: int, grp: str) -> torch.Tensor:
        """Input gradient of _proj_fwd; writes the weight gradients that exist (full fine-tune: dW = dy^T x by the TN
        GEMM; LoRA: dA = dt^T x_d, dB = dy^T t by the split-K TN GEMM, base weight frozen)."""
        st = self.store
        wkey, akey = f"layers.{i}.w{grp}", f"layers.{i}.lora_{grp}.A"
        if self.lora is None:
            dx = ops.linear(dy, st.pT(wkey), st.p(wkey))        # dx = dy @ W: "weight" = W^T, its transpose = W itself
            ops.gemm_tn(dy, xin, out=st.g(wkey))
            return dx
        drop = self._cur_drop
        dt = self._lora_dt(dy, i, grp)
        if drop.per_module:
            # dx = dy W + sum_g mask_g * (dt_g A_g) / (1 - p): _lora_wgrads adds the adapter terms, next to the dA that shares their masks
            dx = ops.linear(dy, st.pT(wkey), st.p(wkey))
        elif drop.p:
            # dropout sits on the adapter branch only: dx = dy W + mask * (dt A) / (1 - p)
            dx = ops.lora_dgrad_dropout(dy, st.p(wkey), st.pT(wkey), dt, st.p(akey), st.pT(akey), *self._lora_mask(i, grp))
        else:
            dx = ops.linear_lora(dy, st.pT(wkey), st.p(wkey), dt, st.pT(akey), st.p(akey), group_cols=0)
        self._lora_wgrads(dy, dt, xin, saved, i, grp, dx=dx if drop.per_module else None)
        return dx

    def _lora_dt(self, dy: torch.Tensor, i: int, grp: str) -> torch.Tensor:
        """dt = [dt_0 | .. | dt_{G-1}], dt_g = (alpha / r) dy_g B_g: the gradient of _lora_t's t."""
        st, rp, sc = self.store, self.lora.r_pad, self.lora.scaling
        if grp == "gu" and st.lora_il:
            # interleaved gate / up columns, the modules are column PARITIES: dt = (alpha/r) dy bexp^T, the expanded adapter's zeros
            # keep the gate columns of dy out of dt_up and vice versa
            return ops.gemm_nt(dy, st.gu_bexp[i], alpha=sc)
        groups = lora_group_rows(self.cfg, grp)                       # (first output column, width) per peft module
        BT = st.pT(f"layers.{i}.lora_{grp}.B")                        # [rp, total output width]
        dt = torch.empty(dy.shape[0], len(groups) * rp, dtype=BF16, device=self.device)
        for g, (c0, og) in enumerate(groups):
            ops.gemm_nt(dy[:, c0:c0 + og], BT[:, c0:c0 + og], out=dt[:, g * rp:(g + 1) * rp], alpha=sc)
        return dt

    def _lora_wgrads(self, dy: torch.Tensor, dt: torch.Tensor, xin: torch.Tensor, saved: ProjSaved, i: int, grp: str,
                     dx: Optional[torch.Tensor] = None):
        """The adapter weight gradients of a fused projection in any dropout mode and either gate|up layout: dA_g = dt_g^T dropout_g(x),
        dB_g = dy_g^T t_g.  ``dx`` (per-module masks, where the caller's input gradient holds dy W only so far): the adapter terms
        sum_g mask_g * (dt_g A_g) / (1 - p) are added to it here, from the same seeds."""
        st, rp, drop = self.store, self.lora.r_pad, self._cur_drop
        gA, gB = st.g(f"layers.{i}.lora_{grp}.A"), st.g(f"layers.{i}.lora_{grp}.B")
        if not drop.per_module:
            if drop.p:
                # the dropped adapter input: kept from forward (288 GB HBM) or regenerated from the seed
                xin = saved.xd if saved.xd is not None else ops.dropout(xin, *self._lora_mask(i, grp))
            ops.gemm_tn_skinny(dt, xin, out=gA)
        else:
            # both from kernels that draw the G masks themselves: one pass over dx, one over the adapter input, no dropped copy
            seeds, AT = self._module_seeds(i, grp), st.pT(f"layers.{i}.lora_{grp}.A")
            if ops.lora_module_masks_ok(xin.shape[1], rp):
                if dx is not None:
                    ops.lora_dgrad_module_masks(dt, AT[:, :len(seeds) * rp], drop.p, seeds, out=dx, residual=dx)
                ops.lora_wgrad_module_masks(dt, xin, drop.p, seeds, out=gA)
            else:
                for g, seed in enumerate(seeds):
                    dtg = dt[:, g * rp:(g + 1) * rp]
                    if dx is not None:
                        ops.gemm_nt_dropout(dtg, AT[:, g * rp:(g + 1) * rp], drop.p, seed, out=dx, residual=dx)
                    ops.gemm_tn_skinny(dtg, ops.dropout(xin, drop.p, seed), out=gA[g * rp:(g + 1) * rp])
        if grp == "gu" and st.lora_il:
            # dB of both modules from ONE product dy^T [t_gate | t_up] -> [2f, 2 rp]; row 2j keeps its first rp columns (gate),
            # row 2j + 1 its last rp (up): the other halves are the cross terms the expanded adapter's zeros stand for
            full = ops.gemm_tn_skinny(dy, saved.t)
            gB[0::2].copy_(full[0::2, :rp])
            gB[1::2].copy_(full[1::2, rp:])
        else:
            for g, (c0, og) in enumerate(lora_group_rows(self.cfg, grp)):
                ops.gemm_tn_skinny(dy[:, c0:c0 + og], saved.t[:, g * rp:(g + 1) * rp], out=gB[c0:c0 + og])

    # ---- adapter models with interleaved gate|up layout (ParamStore.lora_il; RV_LORA_FUSE_SWIGLU=1, round 6) -----------------------
    def _lora_gu_fwd(self, xn2: torch.Tensor, i: int, xn2d: Optional[torch.Tensor]):
        """(gu, act, actd, ProjSaved) of the gate|up projection + SwiGLU of an adapter model: the fused-LoRA GEMM with the SwiGLU
        epilogue (and the dropped activation for the down projection's adapter written by the same epilogue) at chip-filling
        shapes, the unfused composition on the same layout otherwise."""
        st, cfg = self.store, self.cfg
        saved = self._lora_t(xn2, i, "gu", xn2d)
        # the producer-side dropped copy only when the fused-dropout path wants it, as swiglu_fwd_dropout does (per-module masks: the
        # down projection's adapter input is masked in its own kernel, so none is requested)
        fused, (p3, seed3), bexp = self._cur_drop.fused, self._lora_mask(i, "down"), st.gu_bexp[i]
        if ops.linear_lora_swiglu_ok(xn2.shape[0], cfg.ffn, cfg.hidden, self.lora.r_pad):
            return ops.linear_lora_swiglu(xn2, st.pT(f"layers.{i}.wgu"), saved.t, bexp, p3 if fused else 0.0, seed3) + (saved,)
        gu = ops.linear(xn2, st.p(f"layers.{i}.wgu"), st.pT(f"layers.{i}.wgu"))
        ops.gemm_nn(saved.t, bexp, out=gu, residual=gu)
        act = ops.swiglu_fwd(gu, interleaved=True)
        return gu, act, (ops.dropout(act, p3, seed3) if fused else None), saved

    def _lora_down_bwd_swiglu(self, dy: torch.Tensor, act: torch.Tensor, saved: ProjSaved, i: int, gu: torch.Tensor) -> torch.Tensor:
        """d(gate|up) of an adapter model: the down projection's backward (_proj_bwd "down": dA, dB, input gradient) with the SwiGLU
        backward in the epilogue of its input-gradient GEMM (chip-filling shapes: ops.linear_lora_swiglu_ok)."""
        st = self.store
        dt = self._lora_dt(dy, i, "down")
        # (down_proj is one peft module: its mask is the same in both modes, so the fused kernel is exact under per-module masks too)
        dgu = ops.linear_lora_swiglu_bwd(dy, st.p(f"layers.{i}.wdown"), dt, st.p(f"layers.{i}.lora_down.A"), gu,
                                         *self._lora_mask(i, "down"))
        self._lora_wgrads(dy, dt, act, saved, i, "down")
        return dgu

    def _layer_fwd(self, i: int, x: torch.Tensor, pending: Optional[torch.Tensor], plan: SplicePlan, cos, sin, save: bool):
        """One decoder layer (HF LlamaDecoderLayer: RMSNorm, QKV, RoPE, causal attention, O + residual, RMSNorm, SwiGLU
        + residual).  ``pending``: on the fp32 stream (RV_RESID_FP32) the previous layer's bf16 down-projection branch, not yet
        added to ``x``; None on the bf16 stream and in front of layer 0.  Returns (x_next, pending_next, context for backward or None)."""
        cfg, st = self.cfg, self.store
        d, H, hd = cfg.hidden, cfg.heads, cfg.head_dim
        S, L = plan.S, plan.L
        drop = self._cur_drop.fused   # this layer's norms and SwiGLU write the dropped copies their consumers' adapters read
        xnd = xn2d = actd = s_qkv = s_gu = None
        if pending is not None:       # the add rides in this layer's first norm: x = stream + branch, xn = rmsnorm(x), one pass
            x, xn, rstd1 = ops.add_rmsnorm_fwd(x, pending, st.p(f"layers.{i}.ln1"), cfg.rms_eps)
        elif drop:
            xn, rstd1, xnd = ops.rmsnorm_fwd_dropout(x, st.p(f"layers.{i}.ln1"), cfg.rms_eps, *self._lora_mask(i, "qkv"))
        else:
            xn, rstd1 = ops.rmsnorm_fwd(x, st.p(f"layers.{i}.ln1"), cfg.rms_eps)
        rope_cols = (H + cfg.n_kv_heads) * hd
        if (self.lora is None and self.fuse_rope_fwd
                and ops.linear_rope_ok(xn.shape[0], rope_cols + cfg.kv_dim, xn.shape[1], rope_cols, hd)):
            # RoPE in the epilogue of the q|k|v projection, from the fp32 accumulators (round 6): no rope pass, one rounding less on Q / K
            qkv = ops.linear_rope(xn, st.pT(f"layers.{i}.wqkv")[:, :rope_cols + cfg.kv_dim], cos, sin, plan.pos, L, rope_cols, hd)
        else:
            qkv, s_qkv = self._proj_fwd(xn, i, "qkv", xd=xnd)
            ops.rope_inplace(qkv, cos, sin, L, H + cfg.n_kv_heads, hd, pos=plan.pos)      # q heads then k heads
        attn, lse = ops.attn_fwd(qkv, S, L, H, hd, True, 0, d, d + cfg.kv_dim, seg=plan.seg, kv_group=cfg.kv_group, rows=plan.rows,
                                 branches=plan.branches)
        if self.resid_fp32:
            o, s_o = self._proj_fwd(attn, i, "o", residual=None)          # the BRANCH, bf16
            x_mid, xn2, rstd2 = ops.add_rmsnorm_fwd(x, o, st.p(f"layers.{i}.ln2"), cfg.rms_eps)   # fp32 stream + norm, one pass
            del o
        else:
            x_mid, s_o = self._proj_fwd(attn, i, "o", residual=x)
            if drop:
                xn2, rstd2, xn2d = ops.rmsnorm_fwd_dropout(x_mid, st.p(f"layers.{i}.ln2"), cfg.rms_eps, *self._lora_mask(i, "gu"))
            else:
                xn2, rstd2 = ops.rmsnorm_fwd(x_mid, st.p(f"layers.{i}.ln2"), cfg.rms_eps)
        if st.interleave_gu and self.lora is None:   # full fine-tune: SwiGLU in the epilogue of the gate|up GEMM (interleaved weight rows)
            gu, act = ops.linear_swiglu(xn2, st.pT(f"layers.{i}.wgu"))
        elif st.lora_il:              # adapter model, interleaved layout (RV_LORA_FUSE_SWIGLU=1): the same epilogue on the fused-LoRA GEMM
            gu, act, actd, s_gu = self._lora_gu_fwd(xn2, i, xn2d)
        else:
            gu, s_gu = self._proj_fwd(xn2, i, "gu", xd=xn2d)
            if drop:
                act, actd = ops.swiglu_fwd_dropout(gu, *self._lora_mask(i, "down"))
            else:
                act = ops.swiglu_fwd(gu)
        if self.resid_fp32:           # the NEXT layer's first norm (or _run_stack, after the last layer) adds the branch to the stream
            x_next = x_mid
            branch, s_down = self._proj_fwd(act, i, "down", residual=None, xd=actd)
        else:
            branch = None
            x_next, s_down = self._proj_fwd(act, i, "down", residual=x_mid, xd=actd)
        if not save:
            return x_next, branch, None
        keep = self.keep_recomputable
        lctx = dict(x=x, rstd1=rstd1, qkv=qkv, attn=attn, lse=lse, x_mid=x_mid, rstd2=rstd2, gu=gu,
                    lora_qkv=s_qkv, lora_o=s_o, lora_gu=s_gu, lora_down=s_down,      # ProjSaved per projection (None: no adapters)
                    # 288 GB of HBM: keep the cheap-to-recompute operands too (+1.05 GB / layer at 27 k tokens)
                    # instead of re-running RMSNorm / SwiGLU in backward
                    xn=xn if keep else None, xn2=xn2 if keep else None, act=act if keep else None)
        return x_next, branch, lctx

    def _run_stack(self, x: torch.Tensor, plan, save: bool = False, caches: Optional[List[torch.Tensor]] = None,
                   cache_rows: Optional[torch.Tensor] = None):
        """The decoder stack over the spliced bf16 embeddings ``x`` [n_tokens, hidden] under the pass state of _begin_pass: every
        surface's driver.  Returns (the final residual stream, the layers' backward contexts - empty unless ``save``).
        ``save`` under --gradient_checkpointing keeps only each layer's INPUT (fp32 stream: with its pending branch added) and
        backward runs the layer again.  ``caches``: per layer a [rows, 2 kv_dim] bf16 buffer whose first n_tokens rows receive the
        layer's roped K | V columns; with ``cache_rows`` (int32 [n_tokens], generate_continuous) token t goes to row cache_rows[t]
        instead."""
        cfg = self.cfg
        if self.resid_fp32:
            x = ops.cast_bf16_to_f32(x)          # embedding / feature rows are bf16 values: exact
        cos, sin = self._rope(plan.L)
        keep = save and not self.gradient_checkpointing
        pending, layers_ctx = None, []
        for i in range(cfg.layers):
            x_next, branch, lctx = self._layer_fwd(i, x, pending, plan, cos, sin, keep or caches is not None)
            if caches is not None and cache_rows is None:
                caches[i][:plan.n_tokens].copy_(lctx["qkv"][:, cfg.hidden:])      # device copy of the roped K | V columns (plumbing)
            elif caches is not None:
                ops.scatter_rows(lctx["qkv"][:, cfg.hidden:], cache_rows, caches[i])
            if keep:
                layers_ctx.append(lctx)
            elif save:
                layers_ctx.append(dict(x=x if pending is None else ops.add_f32_bf16(x, pending), recompute=True))
            del lctx
            x, pending = x_next, branch
        if pending is not None:
            x = ops.add_f32_bf16(x, pending)     # the last layer's branch joins the fp32 stream
        return x, layers_ctx

    def _last_position_logits(self, plan: SplicePlan, images, caches: Optional[List[torch.Tensor]] = None,
                              cache_rows: Optional[torch.Tensor] = None) -> torch.Tensor:
        """Forward-only read-out behind every row's last token: embed + splice, the stack, the final norm at ``plan.last_idx`` and
        the LM head in fp32.  Returns [round_up(n_seq, 64), vocab_padded] logits (rows >= n_seq are the LM head of zero rows)."""
        cfg, st = self.cfg, self.store
        self._begin_pass()
        feats = self.encode_images(images)
        x = ops.splice_fwd(plan.src, st.p("model.embed_tokens.weight"), feats, cfg.hidden)
        x, _ = self._run_stack(x, plan, caches=caches, cache_rows=cache_rows)
        n = plan.n_seq
        hsel = torch.zeros(max(64, ops.round_up(n, 64)), cfg.hidden, dtype=BF16, device=self.device)
        ops.rmsnorm_fwd(x, st.p("model.norm.weight"), cfg.rms_eps, row_idx=plan.last_idx, out=hsel[:n], want_rstd=False)
        return ops.gemm_nt_f32(hsel, st.p("lm_head.weight"))

    # ------------------------------------------------------------------ forward
    def _logps_plan(self, input_ids, labels, B: int, all_rows: bool, label_shift: int, token_weight, packed: bool):
        """The plan of a forward_logps call, on the device, and the weights rv_seq_sum applies to its selected rows (or None)."""
        cfg = self.cfg
        args = (input_ids, labels, cfg.n_image_tokens, B, cfg.model_max_length)
        if packed or (not all_rows and label_shift == 1 and self.share_prefix and input_ids.shape[0] == 2 * B):
            plan = build_packed_plan(*args, cfg.pad_token_id, splicer=self._row_splicer(), pad_free=self.pad_free,
                                     token_weight=token_weight, all_rows=packed)
        else:
            # label_shift != 1: the get_batch_logps_minicpm convention (labels pre-shifted, muffin_inference_logp.py:21-52),
            # reference layout only
            plan = build_splice_plan(*args, label_shift=1 if all_rows else label_shift, splicer=self._row_splicer(),
                                     token_weight=token_weight)
        w_rows = None
        if all_rows and not packed:       # every position of the reference layout; masked ones take token id 0
            nxt = plan.labels[:, 1:]
            S_, Lm1 = nxt.shape
            plan.sel_idx = (torch.arange(S_)[:, None] * plan.L + torch.arange(Lm1)[None]).reshape(-1).to(torch.int32)
            plan.tgt = torch.where(nxt != -100, nxt, torch.zeros_like(nxt)).reshape(-1).to(torch.int32)
            plan.seq_off = (torch.arange(S_ + 1) * Lm1).to(torch.int32)
            plan.seq_of_row = torch.arange(S_).repeat_interleave(Lm1).to(torch.int32)
            plan.n_sel = int(plan.sel_idx.numel())
            w_rows = (nxt != -100).reshape(-1).to(torch.float32).to(self.device)     # loss_mask of get_batch_logps
        plan = plan.to(self.device)
        if token_weight is not None:
            w_rows = plan.w_sel          # [n_sel] fp32: rv_seq_sum weighs the sums / counts, rv_row_coef the row coefficients
        return plan, w_rows

    def forward_logps(self, input_ids: torch.Tensor, labels: torch.Tensor, images: torch.Tensor,
                      save_for_backward: bool = True, all_rows: bool = False, label_shift: int = 1,
                      token_weight: Optional[torch.Tensor] = None, packed: bool = False) -> StepOutput:
        """Everything of get_beta_and_logps up to ``get_batch_logps``: returns per-sequence log-prob sums
        and counts (muffin/eval/muffin_inference_logp.py:82-115) without materialising logits.
        ``all_rows`` (forward only, reference layout): evaluate EVERY position like
        ``get_batch_logps(return_all=True)`` does - masked positions get the log-prob of token id 0, exactly what
        the reference stores in its ``logps`` parquet column.
        ``token_weight`` [2B, T-1] (token-weighted DPO, position-keeping splices only): the plan gathers it onto the selected
        rows, ``seq_logp`` / ``seq_cnt`` become the weighted sum and the weighted count (compute_weighted_logp,
        trainers.py:128-137) and backward scales each row's coefficient by its weight.
        ``packed`` (with ``all_rows``; input_ids / labels [2B, T] wins then rejects, B images): the all-positions evaluation on
        the packed TRAINING layout - the same plan, layer stack and launches as the training forward, so the values are the
        training step's bit for bit.  ``per_token_logp`` is the [2B, ld] matrix (row s owns its first ``plan.ev_len[s]``
        entries, the rest keep the fill 0), ``seq_logp`` / ``seq_cnt`` are rv_seq_sum over the compact vector of selected rows."""
        B = len(images)                  # tensor [B, 3, H, W] or a list of raw uint8 [H, W, 3] images
        if packed and not all_rows:
            raise ValueError("packed=True is the all-positions precompute on the packed layout: pass all_rows=True")
        if all_rows:
            if save_for_backward:
                raise ValueError("all_rows is a forward-only mode")
            if packed and label_shift != 1:
                raise ValueError("packed=True needs the label_shift=1 convention (the packed layout has no MiniCPM variant)")
            if token_weight is not None:
                raise ValueError("all_rows returns per-token log-probs; token weights apply to the selected-row step")
            if packed and input_ids.shape[0] != 2 * B:
                raise ValueError("packed=True takes [2B, T] wins-then-rejects rows and B images")
        cfg, st = self.cfg, self.store
        d = cfg.hidden
        # evaluation passes between steps must not shift the dropout seeds of later steps
        ctx: dict = {"lora_drop": self._begin_pass(advance=self.training)}
        plan, w_rows = self._logps_plan(input_ids, labels, B, all_rows, label_shift, token_weight, packed)
        feats = self.encode_images(images, ctx if save_for_backward else None)
        x = ops.splice_fwd(plan.src, st.p("model.embed_tokens.weight"), feats, d)
        x, layers_ctx = self._run_stack(x, plan, save=save_for_backward)
        if packed:
            return self._packed_all_rows_logps(x, plan)
        n_sel = plan.n_sel
        n_pad = max(64, ops.round_up(n_sel, 64))
        hsel = torch.zeros(n_pad, d, dtype=BF16, device=self.device)
        if n_sel > 0:
            _, rstd_f = ops.rmsnorm_fwd(x, st.p("model.norm.weight"), cfg.rms_eps, row_idx=plan.sel_idx, out=hsel[:n_sel])
            logp, lse_v = ops.lmhead_logp_fwd(hsel, st.p("lm_head.weight"), plan.tgt, n_sel, v_valid=cfg.vocab)
        else:
            rstd_f = torch.empty(0, dtype=torch.float32, device=self.device)
            logp = torch.empty(0, dtype=torch.float32, device=self.device)
            lse_v = logp
        seq_logp, seq_cnt = ops.seq_sum(logp, plan.seq_off, plan.n_seq, weight=w_rows)
        out = StepOutput(loss=None, scalars=None, per_pair=None, seq_logp=seq_logp, seq_cnt=seq_cnt,
                         per_token_logp=logp, plan=plan)
        if save_for_backward:
            # N: S * L in the rectangular layouts, the sum of the packed rows' lengths when pad-free
            ctx.update(layers=layers_ctx, x_final=x, hsel=hsel, rstd_f=rstd_f, lse_v=lse_v, w_rows=w_rows, N=plan.n_tokens, B=B)
            out.ctx = ctx
        return out

    def _packed_all_rows_logps(self, x: torch.Tensor, plan: SplicePlan) -> StepOutput:
        """Final norm + LM head on every evaluated row of the packed layout (plan.ev_*), then rv_logp_finish_unpack: one launch
        writes each log-prob to its per-token slot(s) and, for the rows the training step selects, to the compact vector that
        rv_seq_sum reduces with the plan's own seq_off - the training step's sums.  A row's LM-head result does not depend on
        the other rows of the launch as long as the GEMM kernel is the same, and the library picks that kernel by row count:
        the launch here is given the kernel the training step's n_sel rows would get."""
        cfg, st = self.cfg, self.store
        n_ev, n_sel, ld = plan.n_ev, plan.n_sel, plan.ev_ld
        per_token = torch.zeros(plan.n_seq, ld, dtype=torch.float32, device=self.device)
        compact = torch.zeros(n_sel, dtype=torch.float32, device=self.device)
        if n_ev > 0:
            hev = torch.zeros(max(64, ops.round_up(n_ev, 64)), cfg.hidden, dtype=BF16, device=self.device)
            ops.rmsnorm_fwd(x, st.p("model.norm.weight"), cfg.rms_eps, row_idx=plan.ev_idx, out=hev[:n_ev], want_rstd=False)
            W = st.p("lm_head.weight")
            v_train = ops.gemm_auto_variant(n_sel, W.shape[0]) if n_sel > 0 else -1
            variant = -1 if v_train == ops.gemm_auto_variant(n_ev, W.shape[0]) else v_train
            ops.lmhead_logp_unpack(hev, W, plan.ev_tgt, n_ev, plan.ev_dst_a, plan.ev_dst_b, plan.ev_dst_c, per_token, compact,
                                   v_valid=cfg.vocab, variant=variant)
        seq_logp, seq_cnt = ops.seq_sum(compact, plan.seq_off, plan.n_seq)
        return StepOutput(loss=None, scalars=None, per_pair=None, seq_logp=seq_logp, seq_cnt=seq_cnt,
                          per_token_logp=per_token, plan=plan)

    # ------------------------------------------------------------------ yes / no feedback scoring
    def forward_next_token_scores(self, prompts, images, want_ids, packed: bool = True, repetition_penalty: float = 1.0,
                                  max_row_tokens: Optional[int] = None):
        """The labeler's side of the AI-feedback stage (muffin/llava15_gen_data.py:266-333, omnilmm/omnilmm_gen_data.py:245-300
        with --is_yesno): ``generate(max_new_tokens=1, output_scores=True)`` per question, of which only softmax(scores[0]) at a
        few token ids and the greedy token are kept - one prefill per question, no cache, no decode loop.
        ``prompts[k]``: the full prompts (1-D input_ids with the image placeholder, as ``question_process`` builds them) of the
        questions about ``images[k]``.  ``encode_images`` runs once per image.  ``packed``: the questions of an image share its
        [system prompt | image | ...] prefix, computed once (splice.build_branch_plan, rv_attn_fwd_branches); ``packed=False``:
        one plain causal pad-free row per question on the existing attention kernel (the comparison path).
        ``repetition_penalty``: HF's RepetitionPenaltyLogitsProcessor over each question's own prompt ids - what
        ``generate(input_ids=..., repetition_penalty=...)`` applies at the first step.  The reference's scripts end up WITHOUT it:
        llava15_gen_data.py sets none, omnilmm_gen_data.py passes 1.1 to ``generate_vllm``, which generates from ``inputs_embeds``
        alone (omnilmm/model/omnilmm.py:371-396), i.e. from an empty id tensor with nothing to penalise.  Default 1.0 = off.
        Forward only, eval mode.  Returns (probs [n_q, K], logp [n_q, K], argmax int32 [n_q], lse [n_q]) on the
        device, questions in input order (image by image)."""
        cfg = self.cfg
        if len(prompts) != len(images):
            raise ValueError(f"{len(prompts)} prompt lists for {len(images)} images")
        with self._eval_mode():
            plan = build_branch_plan(prompts, cfg.n_image_tokens, cfg.model_max_length, splicer=self._row_splicer(),
                                     pad_free=self.pad_free or not packed, max_row_tokens=max_row_tokens, packed=packed)
            logits = self._last_position_logits(plan.to(self.device), images)
            n_q = plan.n_seq
            seen = None
            if repetition_penalty != 1.0:
                uniq = [torch.unique(ids.cpu().long()) for plist in prompts for ids in plist]
                uniq = [u[(u >= 0) & (u < cfg.vocab)] for u in uniq]
                off = torch.zeros(n_q + 1, dtype=torch.int32)
                off[1:] = torch.cumsum(torch.tensor([u.numel() for u in uniq]), 0).to(torch.int32)
                seen = (off.to(self.device), torch.cat(uniq).to(torch.int32).to(self.device))
            want = torch.as_tensor(want_ids, dtype=torch.int32).reshape(-1).to(self.device)
            return ops.next_token_scores(logits, n_q, cfg.vocab, want, seen=seen, penalty=float(repetition_penalty))

    # ------------------------------------------------------------------ KV-cached candidate generation
    def _prefill(self, prompts, images, caches: Optional[List[torch.Tensor]] = None, cache_rows: Optional[torch.Tensor] = None):
        """One plain causal pad-free row per prompt through the training forward's stack (_last_position_logits: its bits).  Returns fp32 last-position logits [round_up(n, 64), vocab_padded] (rows >= n are the LM head of zero rows).
        ``caches``: per layer a [rows, 2 kv_dim] bf16 buffer; the layer's roped K | V rows are copied to its first n_tokens rows,
        or with ``cache_rows`` (int32 [n_tokens] on the device) scattered to the rows it names."""
        cfg = self.cfg
        plan = build_branch_plan([[p] for p in prompts], cfg.n_image_tokens, cfg.model_max_length, splicer=self._row_splicer(),
                                 pad_free=True, packed=False).to(self.device)
        return self._last_position_logits(plan, images, caches, cache_rows)

    def _decode_step(self, tok: torch.Tensor, pos: torch.Tensor, dst: torch.Tensor, spans, caches: List[torch.Tensor],
                     n_split: int, out: torch.Tensor, own_rows: Optional[torch.Tensor] = None, cur_own_len: int = 0):
        """One decode step of at most 64 sequences: token ids ``tok`` at RoPE positions ``pos``, their K | V appended at cache
        rows ``dst``, attention over ``spans`` (current token included), fp32 logits into ``out`` [M, vocab_padded].
        ``own_rows`` (beam search): the sequences' own keys are the rows this int32 [M, T] table names, ``cur_own_len`` of them,
        and ``spans`` = (pre_off, pre_len, own_len); without it ``spans`` = (pre_off, pre_len, own_off, own_len)."""
        cfg, st = self.cfg, self.store
        d, H, hd, kvd = cfg.hidden, cfg.heads, cfg.head_dim, cfg.kv_dim
        cos, sin = self._rope_cache[1], self._rope_cache[2]
        x = ops.gather_rows(st.p("model.embed_tokens.weight"), tok)
        pending = None
        if self.resid_fp32:
            x = ops.cast_bf16_to_f32(x)
        for i in range(cfg.layers):
            if pending is not None:
                x, xn, _ = ops.add_rmsnorm_fwd(x, pending, st.p(f"layers.{i}.ln1"), cfg.rms_eps)
            else:
                xn, _ = ops.rmsnorm_fwd(x, st.p(f"layers.{i}.ln1"), cfg.rms_eps, want_rstd=False)
            qkv = ops.gemm_nt_skinny(xn, st.p(f"layers.{i}.wqkv"))
            ops.rope_inplace(qkv, cos, sin, 1, H + cfg.n_kv_heads, hd, pos=pos)           # q heads then k heads
            ops.scatter_rows(qkv[:, d:], dst, caches[i])
            if own_rows is None:
                attn, _ = ops.attn_decode(qkv, caches[i], H, hd, 0, kvd, spans, kv_group=cfg.kv_group, n_split=n_split)
            else:
                attn, _ = ops.attn_decode_indexed(qkv, caches[i], H, hd, 0, kvd, spans, own_rows, cur_own_len,
                                                  kv_group=cfg.kv_group, n_split=n_split)
            if self.resid_fp32:
                o = ops.gemm_nt_skinny(attn, st.p(f"layers.{i}.wo"))
                x, xn2, _ = ops.add_rmsnorm_fwd(x, o, st.p(f"layers.{i}.ln2"), cfg.rms_eps)
            else:
                x = ops.gemm_nt_skinny(attn, st.p(f"layers.{i}.wo"), residual=x)
                xn2, _ = ops.rmsnorm_fwd(x, st.p(f"layers.{i}.ln2"), cfg.rms_eps, want_rstd=False)
            gu = ops.gemm_nt_skinny(xn2, st.p(f"layers.{i}.wgu"))
            act = ops.swiglu_fwd(gu, interleaved=st.interleave_gu)
            if self.resid_fp32:
                pending = ops.gemm_nt_skinny(act, st.p(f"layers.{i}.wdown"))
            else:
                x = ops.gemm_nt_skinny(act, st.p(f"layers.{i}.wdown"), residual=x)
        if pending is not None:
            x = ops.add_f32_bf16(x, pending)
        h, _ = ops.rmsnorm_fwd(x, st.p("model.norm.weight"), cfg.rms_eps, want_rstd=False)
        ops.gemm_nt_skinny(h, st.p("lm_head.weight"), out=out, out_f32=True)

    def generate(self, prompts, images, max_new_tokens: int, repeat: int = 1, temperature: float = 0.0, top_p: float = 1.0,
                 repetition_penalty: float = 1.0, eos_token_id=None,
                 generator: Optional[torch.Generator] = None, return_scores: bool = False, num_beams: int = 1,
                 top_k: int = 0, *, _uniforms: Optional[torch.Tensor] = None, _forced_tokens: Optional[torch.Tensor] = None):
        """The sampling branch of the AI-feedback stage (muffin/llava15_gen_data.py:335-357: ``generate(do_sample=True,
        temperature=, max_new_tokens=, use_cache=True)`` on a dataset that repeats every item ``--repeat`` times): ``repeat``
        candidate answers per (image, prompt) with a KV cache.  ``prompts[k]``: 1-D input_ids with the image placeholder,
        about ``images[k]``.  Prefill (_prefill) = the training forward's stack, one pad-free causal row per prompt, whose roped K | V rows become
        the first rows of every layer's cache - stored ONCE per prompt, the ``repeat`` samples attend the same rows
        (splice.plan_decode_rows).  Each decode step runs len(prompts) * repeat sequences (chunks of <= 64 rows) through
        norm, rv_gemm_nt_skinny_bf16, RoPE, scatter into the cache, rv_attn_decode, SwiGLU and rv_sample_token; the loop is a
        host ``for`` over at most ``max_new_tokens`` steps and the finished flags are read back every 8 steps.  A finished
        sequence keeps its row and is decoded on until all are finished (its later tokens are dropped): with long answers of
        very different lengths that is work for nothing, the price of fixed chunks and no device-side waiting.
        ``temperature`` 0 = greedy; else HF's processor order (repetition penalty, temperature, top_k, top_p) with uniforms drawn on
        the host from ``generator`` (a CPU torch.Generator; None = the default one): [max_new_tokens, n_seq] in one draw, so a
        seed fixes the output.  The distribution is HF's, the stream is not torch.multinomial's.  The repetition penalty
        covers the ids a sequence has GENERATED so far, no prompt id - the reference's generate starts from inputs_embeds, so
        its processor sees no prompt id either (as forward_next_token_scores documents for the first token).  ``top_p`` < 1
        keeps the smallest set of tokens whose mass reaches top_p; ``top_k`` > 0 first keeps the top_k highest scores and
        everything tied with the last of them (HF's TopKLogitsWarper; rv_sample_token_topk / rv_sample_token_wide_topk), 0 =
        off.  The reference's sampling calls name no top_k and so run with transformers 4.35's default of 50, or the value in the
        checkpoint's generation_config.json: genconfig.resolve_sampling gives the values such a call runs with.  ``num_beams``
        exists to refuse beam search by name.  Test hooks, keyword-only: ``_uniforms`` (fp32 [max_new_tokens, n_seq]) plants
        the uniforms; ``_forced_tokens`` (int32 [n_seq, max_new_tokens]) feeds given tokens instead of the sampled ones
        (teacher forcing).
        ``eos_token_id``: an int, or a sequence of ints (HF's ``eos_token_id=[eos, <|eot_id|>]``): a sequence is finished by the
        first id of the set.  A text-only model (textlm.py) takes ``images=None`` and prompts without the image placeholder.
        The sampler is ops.sampler_for(vocab): rv_sample_token up to 65536 ids, rv_sample_token_wide above.
        Returns tokens[k][r] = the new token ids of sample r of prompt k, cut behind the first ``eos_token_id``; with
        ``return_scores`` (test only) also the fp32 logits [steps, n_seq, vocab] every step sampled from."""
        cfg, st = self.cfg, self.store
        if self.lora is not None:
            raise NotImplementedError("generate(): un-merged LoRA adapters are not supported - merge_lora() first")
        if not getattr(self, "_decodes_spliced_rows", False) and (getattr(cfg, "arch", "llava") == "omnilmm"
                                                                  or self._row_splicer() is not None):
            raise NotImplementedError("generate(): OmniLMM (resampler splice) is not supported")
        if num_beams != 1:
            raise NotImplementedError("generate(): beam search (num_beams > 1) is not supported here - use beam_search()")
        if int(top_k) != top_k or top_k < 0:
            raise ValueError("generate(): top_k must be an integer >= 0 (0 = off)")
        if cfg.head_dim != 128:
            raise NotImplementedError("generate(): rv_attn_decode needs head_dim 128")
        text_only = getattr(cfg, "arch", "llava") == "text"
        if text_only:
            if images is not None:
                raise ValueError("generate(): a text-only model (TextLMConfig) takes images=None")
            if len(prompts) == 0:
                raise ValueError("generate(): no prompts")
            if any(bool((torch.as_tensor(p) == IMAGE_TOKEN_INDEX).any()) for p in prompts):
                raise ValueError("generate(): a prompt of a text-only model (TextLMConfig) holds the image placeholder")
        elif images is None:
            raise ValueError(f"generate(): images=None needs a text-only model (TextLMConfig), this one is '{cfg.arch}'")
        elif len(prompts) != len(images) or len(prompts) == 0:
            raise ValueError(f"{len(prompts)} prompts for {len(images)} images")
        if max_new_tokens < 1 or repeat < 1:
            raise ValueError("generate(): max_new_tokens and repeat must be >= 1")
        eos_ids = eos_id_set(eos_token_id)
        sampler, wide = ops.sampler_for(cfg.vocab)
        from .splice import plan_decode_rows
        T, dev = int(max_new_tokens), self.device
        with self._eval_mode():
            cpu_plan = build_branch_plan([[p] for p in prompts], cfg.n_image_tokens, cfg.model_max_length,
                                         splicer=self._row_splicer(), pad_free=True, packed=False)
            rows = plan_decode_rows(cpu_plan.row_off.tolist(), cpu_plan.row_len.tolist(), repeat, T)
            M = rows.n_seq
            self._rope(cpu_plan.L + T)
            n_split = min(8, max(1, (cpu_plan.L + T) // 256))       # a function of the lengths only: the same bits at any repeat
            caches = [torch.empty(rows.n_rows, 2 * cfg.kv_dim, dtype=BF16, device=dev) for _ in range(cfg.layers)]
            logits = self._prefill(prompts, images, caches)[rows.prompt_of.long().to(dev)]       # [M, vocab_padded]
            pre_off, pre_len, own_off = rows.pre_off.to(dev), rows.pre_len.to(dev), rows.own_off.to(dev)
            rows = replace(rows, pre_len=pre_len, own_off=own_off)               # step() then computes on the device
            sampling = temperature != 0.0
            uniforms, forced_tokens = _uniforms, _forced_tokens
            if sampling and uniforms is None:
                uniforms = torch.rand(T, M, generator=generator, dtype=torch.float32)
            if uniforms is not None:
                if tuple(uniforms.shape) != (T, M):
                    raise ValueError(f"generate(): _uniforms must be [{T}, {M}]")
                uniforms = uniforms.to(dev, torch.float32).contiguous()
            if forced_tokens is not None:
                forced_tokens = torch.as_tensor(forced_tokens).to(dev, torch.int32).reshape(M, T)
            seen = None
            if repetition_penalty != 1.0:
                seen_ids = torch.full((M, T), -1, dtype=torch.int32, device=dev)      # row m: its generated ids; -1 = none yet
                seen = (torch.arange(M + 1, dtype=torch.int32, device=dev) * T, seen_ids.view(-1))
            tokens = torch.zeros(M, T, dtype=torch.int32, device=dev)
            done = torch.zeros(M, dtype=torch.bool, device=dev)
            eos_t = torch.tensor(eos_ids, dtype=torch.int32, device=dev) if eos_ids is not None and len(eos_ids) > 1 else None
            extra = {}
            if wide:
                extra["workspace"] = torch.empty(ops.sample_token_wide_workspace_floats(M, cfg.vocab), dtype=torch.float32, device=dev)
            scores = []
            n_steps = 0
            for j in range(T):
                if j > 0:
                    logits = torch.empty(M, cfg.vocab_padded, dtype=torch.float32, device=dev)
                    pos, dst, own_len = rows.step(j - 1)      # feeds token j - 1, generated last step
                    for c0, c1 in rows.chunks:
                        self._decode_step(tokens[c0:c1, j - 1].contiguous(), pos[c0:c1], dst[c0:c1],
                                          (pre_off[c0:c1], pre_len[c0:c1], own_off[c0:c1], own_len[c0:c1]), caches, n_split,
                                          logits[c0:c1])
                tok, _ = sampler(logits, M, cfg.vocab, uniforms[j] if sampling else None, float(temperature),
                                 float(top_p), seen=seen, penalty=float(repetition_penalty), top_k=int(top_k), **extra)
                if forced_tokens is not None:
                    tok = forced_tokens[:, j]
                tokens[:, j] = tok
                if seen is not None:
                    seen_ids[:, j] = tok
                if return_scores:
                    scores.append(logits[:, :cfg.vocab].clone())
                n_steps = j + 1
                if eos_ids is not None:
                    done |= (tok == eos_ids[0]) if eos_t is None else torch.isin(tok, eos_t)
                    if j % 8 == 7 and bool(done.all()):            # the one read-back of the loop, every 8 steps
                        break
            host = tokens[:, :n_steps].cpu().tolist()
            out = []
            for k in range(len(prompts)):
                out.append([])
                for r in range(repeat):
                    out[-1].append(cut_behind_eos(host[k * repeat + r], eos_ids))
            return (out, torch.stack(scores)) if return_scores else out

    # ------------------------------------------------------------------ continuous batching of candidate generation
    def generate_continuous(self, requests, max_new_tokens: int, slots: int = 64, repeat: int = 1, temperature: float = 0.0,
                            top_p: float = 1.0, top_k: int = 0, repetition_penalty: float = 1.0, eos_token_id=None, seed: int = 0,
                            max_prompt_tokens: Optional[int] = None, poll_every: int = 8, num_beams: int = 1,
                            request_indices=None, prefill_prompts: int = 8, regions: Optional[int] = None, *,
                            _uniforms=None, _scores=None, _scheduler: Optional[list] = None):
        """``generate()``'s sampling with the finished rows refilled: a GENERATOR over ``requests``, any iterable of
        ``(prompt_ids, image[, max_new_tokens_i])`` consumed lazily (a DataLoader can feed it), that yields
        ``(request_index, [tokens of sample 0 .. repeat - 1])`` in completion order.  ``request_indices``: an iterable of ints
        consumed in step with ``requests`` (default 0, 1, ...) - the index a request is reported and seeded under.
        The decode step has ``slots`` rows, each at a step of its own (ops.DecodeState, rv_decode_advance): _decode_step per
        chunk of <= 64 slots, the sampler over all slots, rv_decode_advance; a finished or unused slot is parked on the first
        row of its own cache region.  The done flags are read back when schedule.SlotScheduler says so (every ``poll_every``
        steps, sooner when every live budget ends sooner); a request is admitted whole - ``repeat`` free slots and one of
        ``regions`` (default min(slots, 3 * (slots // repeat))) prompt regions of ``max_prompt_tokens`` rows (default model_max_length; a
        region is what the cache reserves per live prompt, so pass the longest spliced prompt when it is known) - at most
        ``prefill_prompts`` per _prefill call, whose K | V rows are scattered to their regions (schedule.SlotRows) and whose
        last-position logits give each sample's first token (rv_decode_admit).
        BITS: every kernel of a sequence's path is ``generate()``'s and none of them lets a row see its neighbours, and
        n_split = min(8, max(1, (max_prompt_tokens + max_new_tokens) // 256)) is a function of the engine's capacity only: a
        sequence's tokens do not depend on ``slots``, on who shares the step with it or on the order of arrival, and equal
        ``generate([prompt], [image], budget, repeat)`` with the same uniforms whenever that call's n_split is the same.
        UNIFORMS: step t of sample r of request i draws schedule.uniform_table(seed, i, max_new_tokens, repeat)[t, r], a hash
        of (seed, i, r, t) alone - no generator is consumed in call order, so a shard that starts at another item draws the
        same numbers for it.  ``max_new_tokens_i`` (<= max_new_tokens) is a request's own budget: one int, or ``repeat`` ints, one per
        sample.
        Test hooks, keyword-only: ``_uniforms`` (callable index -> fp32 [max_new_tokens, repeat]) replaces the table;
        ``_scores`` (callable (index, sample, step, fp32 logits [vocab])) sees every row a live slot is sampled from (rows
        behind a sequence's end included, until the poll that frees the slot); ``_scheduler`` (a list) receives the
        SlotScheduler.  Refused by name before anything is launched: a row splicer the class does not decode with
        (``_decodes_spliced_rows``; OmniLMMDPOModel sets it), un-merged LoRA, head_dim != 128,
        num_beams != 1, repeat > slots; a prompt longer than ``max_prompt_tokens`` when its request is reached."""
        cfg = self.cfg
        if self.lora is not None:
            raise NotImplementedError("generate_continuous(): un-merged LoRA adapters are not supported - merge_lora() first")
        if not getattr(self, "_decodes_spliced_rows", False) and (getattr(cfg, "arch", "llava") == "omnilmm"
                                                                  or self._row_splicer() is not None):
            raise NotImplementedError("generate_continuous(): OmniLMM (resampler splice) is not supported")
        if num_beams != 1:
            raise NotImplementedError("generate_continuous(): beam search (num_beams > 1) is not supported - use beam_search()")
        if cfg.head_dim != 128:
            raise NotImplementedError("generate_continuous(): rv_attn_decode needs head_dim 128")
        if int(top_k) != top_k or top_k < 0:
            raise ValueError("generate_continuous(): top_k must be an integer >= 0 (0 = off)")
        if max_new_tokens < 1 or repeat < 1 or slots < 1 or poll_every < 1 or prefill_prompts < 1:
            raise ValueError("generate_continuous(): max_new_tokens, repeat, slots, poll_every and prefill_prompts must be >= 1")
        if repeat > slots:
            raise ValueError(f"generate_continuous(): repeat {repeat} > slots {slots} (a request is admitted whole)")
        max_prompt = int(cfg.model_max_length if max_prompt_tokens is None else max_prompt_tokens)
        if max_prompt < 1:
            raise ValueError("generate_continuous(): max_prompt_tokens must be >= 1")
        eos_ids = eos_id_set(eos_token_id)
        if eos_ids is not None and len(eos_ids) > 8:
            raise ValueError("generate_continuous(): at most 8 EOS ids (rv_decode_advance)")
        ops.sampler_for(cfg.vocab)
        return self._continuous(requests, int(max_new_tokens), int(slots), int(repeat), float(temperature), float(top_p), int(top_k),
                                float(repetition_penalty), eos_ids, int(seed), max_prompt, int(poll_every), request_indices,
                                int(prefill_prompts), regions, _uniforms, _scores, _scheduler)

    def _continuous(self, requests, T, S, repeat, temperature, top_p, top_k, penalty, eos_ids, seed, max_prompt, poll_every,
                    request_indices, prefill_prompts, regions, uniforms_of, scores_hook, sched_out):
        """The loop of generate_continuous (a generator: the checks above run at the call, this at the first ``next``)."""
        from .schedule import SlotRows, SlotScheduler, uniform_table
        cfg, dev = self.cfg, self.device
        text_only = getattr(cfg, "arch", "llava") == "text"
        sampler, wide = ops.sampler_for(cfg.vocab)
        sched = SlotScheduler(S, repeat, regions, poll_every)
        if sched_out is not None:
            sched_out.append(sched)
        rows = SlotRows(sched.regions, max_prompt, S, T)
        sampling = temperature != 0.0
        feed = iter(requests)
        index_feed = iter(request_indices) if request_indices is not None else None
        with self._eval_mode():
            self._rope(max_prompt + T)
            n_split = min(8, max(1, (max_prompt + T) // 256))        # the engine's capacity only: the same bits whoever shares the step
            caches = [torch.empty(rows.n_rows, 2 * cfg.kv_dim, dtype=BF16, device=dev) for _ in range(cfg.layers)]
            state = ops.DecodeState(S, T, rows.own_off, dev, eos_ids)
            seen = state.seen if penalty != 1.0 else None
            extra = {}
            if wide:
                extra["workspace"] = torch.empty(ops.sample_token_wide_workspace_floats(S, cfg.vocab), dtype=torch.float32, device=dev)
            logits = torch.zeros(S, cfg.vocab_padded, dtype=torch.float32, device=dev)
            chunks = rows.chunks
            age = [0] * S                  # sampler rounds a slot's sequence has had (host count, for the scores hook)
            results: Dict[int, list] = {}
            position, exhausted = 0, False
            while True:
                # ---- admission: whole requests, at most prefill_prompts per prefill
                while not exhausted and sched.room() > 0:
                    batch, cap = [], min(sched.room(), prefill_prompts)
                    while len(batch) < cap:
                        try:
                            req = next(feed)
                        except StopIteration:
                            exhausted = True
                            break
                        index = position if index_feed is None else int(next(index_feed))
                        position += 1
                        prompt, image = req[0], req[1]
                        budget = req[2] if len(req) > 2 and req[2] is not None else T
                        budget = [int(b) for b in budget] if isinstance(budget, (list, tuple)) else [int(budget)] * repeat
                        if len(budget) != repeat or not all(1 <= b <= T for b in budget):
                            raise ValueError(f"generate_continuous(): request {index}: max_new_tokens {budget} outside [1, {T}] "
                                             f"(one value, or one per sample)")
                        if text_only:
                            if image is not None:
                                raise ValueError(f"generate_continuous(): request {index}: a text-only model (TextLMConfig) takes image=None")
                            if bool((torch.as_tensor(prompt) == IMAGE_TOKEN_INDEX).any()):
                                raise ValueError(f"generate_continuous(): request {index}: a prompt of a text-only model holds the image placeholder")
                        elif image is None:
                            raise ValueError(f"generate_continuous(): request {index}: image=None needs a text-only model (TextLMConfig)")
                        if index in results or any(index == b[0] for b in batch):
                            raise ValueError(f"generate_continuous(): request index {index} is used twice")
                        batch.append((index, prompt, image, budget))
                    if not batch:
                        break
                    prompts = [b[1] for b in batch]
                    cpu_plan = build_branch_plan([[p] for p in prompts], cfg.n_image_tokens, cfg.model_max_length,
                                                 splicer=self._row_splicer(), pad_free=True, packed=False)
                    lens = cpu_plan.row_len.tolist()
                    for (index, _, _, _), n in zip(batch, lens):
                        if n > max_prompt:
                            raise ValueError(f"generate_continuous(): request {index}: a spliced prompt of {n} tokens is longer than "
                                             f"max_prompt_tokens = {max_prompt}")
                    images = None
                    if not text_only:
                        images = [b[2] for b in batch]
                        if all(torch.is_tensor(im) for im in images) and len({(im.shape, im.dtype) for im in images}) == 1 \
                                and images[0].dtype != torch.uint8:
                            images = torch.stack(images)
                    ad_slots, ad_off, ad_len, ad_budget, prompt_of, regs = [], [], [], [], [], []
                    for k, (index, _, _, budget) in enumerate(batch):
                        region, ss = sched.admit(index, budget)
                        regs.append(region)
                        if sampling:
                            table = uniforms_of(index) if uniforms_of is not None else uniform_table(seed, index, T, repeat)
                            table = torch.as_tensor(table, dtype=torch.float32)
                            if tuple(table.shape) != (T, repeat):
                                raise ValueError(f"generate_continuous(): the uniforms of a request must be [{T}, {repeat}]")
                            state.u_table[torch.tensor(ss, device=dev)] = table.t().contiguous().to(dev)
                        results[index] = [None] * repeat
                        for r, s in enumerate(ss):
                            ad_slots.append(s), ad_off.append(rows.region_off(region)), ad_len.append(lens[k])
                            ad_budget.append(budget[r]), prompt_of.append(k)
                    first = self._prefill(prompts, images, caches, rows.prefill_rows(regs, lens).to(dev))
                    first = first[torch.tensor(prompt_of, device=dev)]                  # [admitted slots, vocab_padded]
                    slot_t = torch.tensor(ad_slots, device=dev)
                    n_new = len(ad_slots)
                    x = {"workspace": torch.empty(ops.sample_token_wide_workspace_floats(n_new, cfg.vocab), dtype=torch.float32,
                                                  device=dev)} if wide else {}
                    tok, _ = sampler(first, n_new, cfg.vocab, state.u_table[slot_t, 0].contiguous() if sampling else None, temperature,
                                     top_p, seen=None, penalty=1.0, top_k=top_k, **x)        # nothing generated yet: nothing to penalise
                    if scores_hook is not None:
                        for n, s in enumerate(ad_slots):
                            scores_hook(*sched.owner[s], 0, first[n, :cfg.vocab].clone())
                    for s in ad_slots:
                        age[s] = 1
                    ops.decode_admit(state, ad_slots, ad_off, ad_len, ad_budget, tok)
                if not sched.live:
                    if exhausted:
                        return
                    continue
                # ---- decode steps until the next look at the flags
                for _ in range(sched.steps_to_poll()):
                    for c0, c1 in chunks:
                        if sched.chunk_live(c0, c1):
                            self._decode_step(state.tok_in[c0:c1], state.pos[c0:c1], state.dst[c0:c1],
                                              (state.pre_off[c0:c1], state.pre_len_eff[c0:c1], state.own_off[c0:c1],
                                               state.own_len[c0:c1]), caches, n_split, logits[c0:c1])
                    tok, _ = sampler(logits, S, cfg.vocab, state.u_next if sampling else None, temperature, top_p, seen=seen,
                                     penalty=penalty, top_k=top_k, **extra)
                    if scores_hook is not None:
                        for s, o in enumerate(sched.owner):
                            if o is not None:
                                scores_hook(*o, age[s], logits[s, :cfg.vocab].clone())
                                age[s] += 1
                    ops.decode_advance(state, tok)
                    sched.step()
                # ---- the read-back: lengths and flags, then the rows of the slots that have finished
                lens_h, done_h = state.flags()
                finished, complete = sched.poll(done_h)
                if finished:
                    got = state.out_tokens[torch.tensor([s for s, _, _ in finished], device=dev)].cpu().tolist()
                    for (s, index, sample), row in zip(finished, got):
                        results[index][sample] = cut_behind_eos(row[:lens_h[s]], eos_ids)
                for index in complete:
                    yield index, results.pop(index)

    # ------------------------------------------------------------------ beam-search decoding (the evaluation stage)
    def beam_search(self, prompts, images, max_new_tokens: int, num_beams: int = 3, eos_token_id: Optional[int] = None,
                    length_penalty: float = 1.0, return_trace: bool = False, repetition_penalty: float = 1.0, *, _forced=None):
        """One answer per (image, prompt) the way the reference's evaluation produces it (muffin/eval/muffin_vqa.py,
        llava15_chair.py, chat.py: ``generate(do_sample=False, num_beams=3, max_new_tokens=)`` from inputs_embeds): HF's
        GenerationMixin._beam_search with early_stopping=False and one EOS id.  Prefill is ``generate``'s (_prefill); its
        last-position logits serve the ``num_beams`` beams of a prompt, which share the prompt's cache rows
        (splice.plan_beam_rows).  A step is ``generate``'s decode step with rv_attn_decode_indexed in place of rv_attn_decode,
        then rv_beam_topk (the 2K best of log_softmax + beam score per prompt) and rv_beam_step (running beams, finished
        hypotheses, stop rule, and the per-beam token history and cache-row table for the next step) - all on the device; the
        loop is a host ``for`` and the done flags are read back every 8 steps.  Step j's K | V go to fresh cache rows; a
        reselection of beams changes table entries only, no cache row is ever copied or reordered.  A prompt that is done keeps
        its rows and is decoded on until all are (its finished set is frozen), as in ``generate``.
        Returns (tokens, scores): tokens[k] = the new token ids of prompt k's best hypothesis (it ends with ``eos_token_id`` if
        it finished on it), scores[k] = its ``sequences_scores`` = sum of log-probs / length ** length_penalty.
        ``repetition_penalty`` != 1 (omnilmm/omnilmm_gen_data.py:306-314): HF's RepetitionPenaltyLogitsProcessor where beam search
        runs it, on the log-softmax before the beam score is added, over the tokens the beam has GENERATED (its row of the token
        history; no prompt id, as in ``generate``) - rv_beam_topk_penalty.  The summed scores are then sums of penalised
        log-probs, as HF's are.  1.0 = rv_beam_topk, today's bits.
        ``return_trace`` (tests): a third value, a dict of per-step tensors - ``logits`` [steps, M, vocab] fp32, the device's
        candidates ``cand_val`` / ``cand_parent`` / ``cand_tok`` [steps, G, 2K], its running beams ``parent`` / ``token`` /
        ``score`` [steps, M], and ``done`` [steps, G], ``n_hyp`` [steps, G], ``hyp_score`` / ``hyp_len`` [steps, G, K] after each
        step, plus the final ``hyp_tokens`` [G, K, T].  ``_forced`` (test hook, keyword-only) = (parent, token[, score]), each
        [steps, M]: follow these beams instead of the device's selection (teacher forcing for beams) for ``steps`` steps; no
        hypothesis is collected and tokens / scores are None."""
        cfg = self.cfg
        if self.lora is not None:
            raise NotImplementedError("beam_search(): un-merged LoRA adapters are not supported - merge_lora() first")
        if not getattr(self, "_decodes_spliced_rows", False) and (getattr(cfg, "arch", "llava") == "omnilmm"
                                                                  or self._row_splicer() is not None):
            raise NotImplementedError("beam_search(): OmniLMM (resampler splice) is not supported")
        if cfg.head_dim != 128:
            raise NotImplementedError("beam_search(): rv_attn_decode_indexed needs head_dim 128")
        if not 1 <= num_beams <= 8:
            raise NotImplementedError(f"beam_search(): num_beams must be 1..8 (rv_beam_topk), got {num_beams}")
        if len(prompts) != len(images) or len(prompts) == 0:
            raise ValueError(f"{len(prompts)} prompts for {len(images)} images")
        if max_new_tokens < 1:
            raise ValueError("beam_search(): max_new_tokens must be >= 1")
        if not repetition_penalty > 0:
            raise ValueError("beam_search(): repetition_penalty must be > 0 (1.0 = off)")
        from .splice import plan_beam_rows
        T, K, G, dev = int(max_new_tokens), int(num_beams), len(prompts), self.device
        with self._eval_mode():
            cpu_plan = build_branch_plan([[p] for p in prompts], cfg.n_image_tokens, cfg.model_max_length,
                                         splicer=self._row_splicer(), pad_free=True, packed=False)
            rows = plan_beam_rows(cpu_plan.row_off.tolist(), cpu_plan.row_len.tolist(), K, T)
            M = rows.n_seq
            self._rope(cpu_plan.L + T)
            n_split = min(8, max(1, (cpu_plan.L + T) // 256))       # generate()'s rule: a function of the lengths only
            caches = [torch.empty(rows.n_rows, 2 * cfg.kv_dim, dtype=BF16, device=dev) for _ in range(cfg.layers)]
            logits = self._prefill(prompts, images, caches)[rows.prompt_of.long().to(dev)]       # [M, vocab_padded]
            pre_off = rows.pre_off.to(dev)
            rows = replace(rows, pre_len=rows.pre_len.to(dev), seq_idx=rows.seq_idx.to(dev))
            state = ops.BeamState(G, K, T, rows.own_base, dev)
            forced, n_max = None, T
            if _forced is not None:
                forced = [torch.as_tensor(t).to(dev) for t in _forced]
                if len(forced) == 2:
                    forced.append(torch.zeros(forced[0].shape, dtype=torch.float32, device=dev))
                n_max = int(forced[0].shape[0])
                if len(forced) != 3 or not 1 <= n_max <= T or any(tuple(t.shape) != (n_max, M) for t in forced):
                    raise ValueError(f"beam_search(): _forced = (parent, token[, score]), each [steps <= {T}, {M}]")
                forced = [forced[0].to(torch.int32).contiguous(), forced[1].to(torch.int32).contiguous(),
                          forced[2].to(torch.float32).contiguous()]
            keys = ("logits", "cand_val", "cand_parent", "cand_tok", "parent", "token", "score", "done", "n_hyp", "hyp_score",
                    "hyp_len")
            trace = {k: [] for k in keys}
            for j in range(n_max):
                if j > 0:
                    logits = torch.empty(M, cfg.vocab_padded, dtype=torch.float32, device=dev)
                    pos, dst, own_len = rows.step(j - 1)      # feeds token j - 1, chosen last step
                    for c0, c1 in rows.chunks:
                        self._decode_step(state.token[c0:c1], pos[c0:c1], dst[c0:c1], (pre_off[c0:c1], rows.pre_len[c0:c1],
                                          own_len[c0:c1]), caches, n_split, logits[c0:c1], own_rows=state.own_rows[c0:c1],
                                          cur_own_len=j)
                if repetition_penalty != 1.0:
                    cand = ops.beam_topk(logits, state.run_score, G, K, cfg.vocab, hist=state.hist, n_hist=j,
                                         penalty=float(repetition_penalty))[:3]
                else:
                    cand = ops.beam_topk(logits, state.run_score, G, K, cfg.vocab)[:3]
                ops.beam_step(state, cand, j, eos_token_id, length_penalty,
                              forced=None if forced is None else (forced[0][j], forced[1][j], forced[2][j]))
                if return_trace:
                    for k, t in zip(keys, (logits[:, :cfg.vocab], *cand, state.parent, state.token, state.run_score, state.done,
                                           state.n_hyp, state.hyp_score, state.hyp_len)):
                        trace[k].append(t.clone())
                if eos_token_id is not None and forced is None and j % 8 == 7 and bool(state.done.all()):
                    break                                      # the one read-back of the loop, every 8 steps
            tokens = scores = None
            if forced is None:
                n_hyp, hyp_len = state.n_hyp.cpu().tolist(), state.hyp_len.cpu().tolist()
                hyp_score, hyp_tokens = state.hyp_score.cpu(), state.hyp_tokens.cpu()
                tokens, scores = [], []
                for g in range(G):                             # the best finished hypothesis wins (the lower slot among equals)
                    best = int(torch.argmax(hyp_score[g, :n_hyp[g]]))
                    tokens.append(hyp_tokens[g, best, :hyp_len[g][best]].tolist())
                    scores.append(float(hyp_score[g, best]))
            if not return_trace:
                return tokens, scores
            out = {k: torch.stack(v) for k, v in trace.items()}
            out["hyp_tokens"] = state.hyp_tokens.clone()
            return tokens, scores, out

    # ------------------------------------------------------------------ backward
    def backward(self, out: StepOutput, coef: torch.Tensor):
        """coef[2B] = d loss / d seq_logp (rv_dpo_loss).  Fills ``store.flat_g`` (overwrites)."""
        cfg, st = self.cfg, self.store
        d, H, hd, f = cfg.hidden, cfg.heads, cfg.head_dim, cfg.ffn
        ctx, plan = out.ctx, out.plan
        S, L, N = plan.S, plan.L, ctx["N"]
        cos, sin = self._rope(L)
        hook = self.grad_ready_hook

        lora = self.lora is not None
        self._cur_drop = ctx.get("lora_drop", LoraDrop())      # the pass state of the forward being differentiated
        scratch_dw = torch.empty(d, dtype=BF16, device=self.device) if lora else None   # gains are frozen under LoRA

        def wgrad(dy: torch.Tensor, xin: torch.Tensor, key: str):
            """dW[key] = dy^T @ xin: TN GEMM (operands transposed on the fly by ds_read_b64_tr_b16)."""
            ops.gemm_tn(dy, xin, out=st.g(key))

        def gain_grad(key: str) -> torch.Tensor:
            return scratch_dw if lora else st.g(key)

        # ---- LM head + final norm
        n_sel = plan.n_sel
        dx = torch.zeros(N, d, dtype=BF16, device=self.device)
        if n_sel > 0:
            rc = ops.row_coef(coef, plan.seq_of_row, ctx["w_rows"])
            dlog = ops.lmhead_logp_bwd(ctx["hsel"], st.p("lm_head.weight"), plan.tgt, ctx["lse_v"], rc, n_sel,
                                       v_valid=cfg.vocab)
            dh = ops.linear(dlog, st.pT("lm_head.weight"), st.p("lm_head.weight"))
            if not lora:
                wgrad(dlog, ctx["hsel"], "lm_head.weight")
            del dlog
            ops.rmsnorm_bwd(dh[:n_sel], ctx["x_final"], st.p("model.norm.weight"), ctx["rstd_f"],
                            gain_grad("model.norm.weight"), row_idx=plan.sel_idx, dx=dx)
        elif not lora:
            st.g("lm_head.weight").zero_()
            st.g("model.norm.weight").zero_()
        if hook and not lora:
            hook("lm_head", *st.buckets["lm_head"])

        # ---- decoder layers, last to first
        for i in reversed(range(cfg.layers)):
            c = ctx["layers"][i]
            if c.get("recompute"):      # --gradient_checkpointing: only the layer input was kept; run the layer again
                _, _, c = self._layer_fwd(i, c["x"], None, plan, cos, sin, True)
            act = c["act"] if c["act"] is not None else ops.swiglu_fwd(c["gu"], interleaved=st.interleave_gu)
            c["act"] = None
            if st.interleave_gu and self.lora is None:
                # d(gate|up) straight out of the down projection's input-gradient GEMM (SwiGLU backward in its epilogue)
                dgu = ops.linear_swiglu_bwd(dx, st.p(f"layers.{i}.wdown"), c["gu"])
                ops.gemm_tn(dx, act, out=st.g(f"layers.{i}.wdown"))
                del act
            elif st.lora_il and ops.linear_lora_swiglu_ok(dx.shape[0], f, d, self.lora.r_pad):
                dgu = self._lora_down_bwd_swiglu(dx, act, c["lora_down"], i, c["gu"])
                del act
            else:
                dact = self._proj_bwd(dx, act, c["lora_down"], i, "down")
                del act
                dgu = ops.swiglu_bwd(dact, c["gu"], interleaved=st.interleave_gu)
                del dact
            xn2 = c["xn2"] if c["xn2"] is not None else \
                ops.rmsnorm_fwd(c["x_mid"], st.p(f"layers.{i}.ln2"), cfg.rms_eps, want_rstd=False)[0]
            c["xn2"] = None
            dxn2 = self._proj_bwd(dgu, xn2, c["lora_gu"], i, "gu")
            del dgu, xn2
            dx_mid = ops.rmsnorm_bwd(dxn2, c["x_mid"], st.p(f"layers.{i}.ln2"), c["rstd2"], gain_grad(f"layers.{i}.ln2"),
                                     dres=dx)
            del dxn2
            dattn = self._proj_bwd(dx_mid, c["attn"], c["lora_o"], i, "o")
            # dQ / dK leave the attention backward already rotated back (RV_FUSE_ROPE_BWD=0: separate rv_rope_inplace pass)
            dqkv = ops.attn_bwd(c["qkv"], c["attn"], dattn, c["lse"], S, L, H, hd, True, 0, d, d + cfg.kv_dim,
                                seg=plan.seg, kv_group=cfg.kv_group, rope=(cos, sin, plan.pos) if self.fuse_rope_bwd else None,
                                rows=plan.rows)
            del dattn
            if not self.fuse_rope_bwd:
                ops.rope_inplace(dqkv, cos, sin, L, H + cfg.n_kv_heads, hd, backward=True, pos=plan.pos)
            xn = c["xn"] if c["xn"] is not None else \
                ops.rmsnorm_fwd(c["x"], st.p(f"layers.{i}.ln1"), cfg.rms_eps, want_rstd=False)[0]
            c["xn"] = None
            dxn = self._proj_bwd(dqkv, xn, c["lora_qkv"], i, "qkv")
            del dqkv, xn
            dx = ops.rmsnorm_bwd(dxn, c["x"], st.p(f"layers.{i}.ln1"), c["rstd1"], gain_grad(f"layers.{i}.ln1"),
                                 dres=dx_mid)
            del dxn, dx_mid
            ctx["layers"][i] = None          # free this layer's activations
            if hook:
                hook(f"layer{i}", *st.buckets[f"layer{i}"])

        # ---- embedding (deterministic segmented sum; frozen under LoRA) and projector
        if not lora:
            ge = st.g("model.embed_tokens.weight")
            ge.zero_()
            ops.embed_bwd(plan.uniq_ids, plan.seg_off, plan.pos_sorted, dx, ge)
        dfeat = ops.feat_grad(plan.feat_src_a, plan.feat_src_b, dx, d)
        self._vision_backward(dfeat, ctx)
        if hook:
            hook("embed_proj", *st.buckets["embed_proj"])
            hook("nodecay", *st.buckets["nodecay"])
        out.ctx = {}

    # ------------------------------------------------------------------ reference-style surface
    def forward(self, input_ids=None, attention_mask=None, position_ids=None, past_key_values=None, inputs_embeds=None,
                labels=None, images=None, **kwargs):
        """``LlavaLlamaForCausalLM.forward(inputs_embeds=, labels=None).logits`` - the call get_beta_and_logps makes after
        the splice (muffin/train/trainers.py:221-225, llava/model/language_model/llava_llama.py:57-102).  Debug / evaluation
        surface for SMALL inputs: it materialises [S, L, V] logits, which the training path never does (forward_logps fuses
        the LM head with the log-softmax).  Forward only; pure causal mask, positions 0..L-1, like the reference call."""
        from types import SimpleNamespace
        if inputs_embeds is None:
            raise NotImplementedError("forward() takes inputs_embeds (prepare_inputs_labels_for_multimodal builds them)")
        if labels is not None or attention_mask is not None or past_key_values is not None:
            raise NotImplementedError("the DPO call site passes labels=None, attention_mask=None, no cache")
        cfg, st = self.cfg, self.store
        S, L, d = inputs_embeds.shape
        if S * L * cfg.vocab * 2 > (16 << 30):
            raise ValueError("forward(): logits would exceed 16 GB - use forward_logps (fused LM head) for training shapes")
        x = inputs_embeds.to(self.device, BF16).reshape(S * L, d).contiguous()
        self._begin_pass()
        x, _ = self._run_stack(x, SimpleNamespace(S=S, L=L, pos=None, seg=None, rows=None, branches=None))
        h, _ = ops.rmsnorm_fwd(x, st.p("model.norm.weight"), cfg.rms_eps, want_rstd=False)
        logits = ops.gemm_nt(h, st.p("lm_head.weight"))[:, :cfg.vocab]          # drop the vocabulary padding columns
        return SimpleNamespace(logits=logits.reshape(S, L, cfg.vocab), loss=None)

    __call__ = forward

    def prepare_inputs_labels_for_multimodal(self, input_ids, position_ids, attention_mask, past_key_values, labels,
                                             images):
        """Same 6-tuple contract as llava_arch.py:150-330 (embeds materialised by rv_splice_fwd)."""
        if attention_mask is not None:
            raise NotImplementedError("the DPO path passes attention_mask=None (trainers.py:199)")
        feats = self.encode_images(images)      # one feature block per row of `images`, like the reference
        n_img = len(images)
        plan = build_splice_plan(input_ids, labels, self.cfg.n_image_tokens, n_img, self.cfg.model_max_length,
                                 splicer=self._row_splicer()).to(self.device)
        emb = ops.splice_fwd(plan.src, self.store.p("model.embed_tokens.weight"), feats, self.cfg.hidden)
        return None, None, None, past_key_values, emb.view(plan.S, plan.L, -1), plan.labels.to(self.device)
