"""Host-side integer planning for the image splice and the label-driven row selection.

Mirrors ``LlavaMetaForCausalLM.prepare_inputs_labels_for_multimodal``
(/root/reference llava/model/llava_arch.py:150-330) for the DPO call site, where
``attention_mask=None`` (muffin/train/trainers.py:199, so pads are kept: llava_arch.py:220-231) and
``get_batch_logps``' shift / mask (muffin/eval/muffin_inference_logp.py:93-96).  Everything here is
int64/int32 index arithmetic on the CPU side of the batch (it replaces the reference's per-row
Python loop with its ``.tolist()`` device syncs); the tables are then consumed by the HIP kernels
``rv_splice_fwd`` / ``rv_embed_bwd`` / ``rv_feat_grad`` / ``rv_rmsnorm_*`` (row gather).

Two layouts:
  * ``build_splice_plan``  - the reference layout: 2B rows (wins then rejects), right padded to L;
  * ``build_packed_plan``  - one row per PAIR, ``[shared prefix | chosen branch | rejected branch]``.
    The chosen and rejected sequences of a pair start with the same system prompt + image + question
    (muffin/data/datasets.py:61-63), a causal model gives those positions identical hidden states in both
    rows, so they are computed once: the rejected branch attends the shared prefix but not the chosen branch
    (rv_attn_* ``seg_sh/seg_e1``) and keeps its own RoPE positions (``pos``).  Pads are dropped (they sit to
    the right of every counted token and never influence a log-prob).  The per-sequence outputs are
    mathematically identical to the reference layout.
"""
from __future__ import annotations

import numbers
from dataclasses import dataclass
from typing import List, Optional, Sequence, Tuple

import torch

IGNORE_INDEX = -100
IMAGE_TOKEN_INDEX = -200


@dataclass
class SplicePlan:
    S: int                     # physical rows of the activation matrix
    L: int                     # row length (right padded)
    n_seq: int                 # logical sequences (2B: wins then rejects)
    src: torch.Tensor          # int32 [S*L]  >=0 embed row | -1 zero pad | <=-2 feature row (-2 - r)
    labels: Optional[torch.Tensor]   # int64 [S, L] new labels in the reference layout (None when packed)
    sel_idx: torch.Tensor      # int32 [n_sel] flat row n whose NEXT label is a target, ordered by (sequence, position)
    tgt: torch.Tensor          # int32 [n_sel] that target id
    seq_off: torch.Tensor      # int32 [n_seq+1] selected rows of sequence s are seq_off[s]..seq_off[s+1]
    seq_of_row: torch.Tensor   # int32 [n_sel]
    uniq_ids: torch.Tensor     # int32 [U]     distinct embedded token ids
    seg_off: torch.Tensor      # int32 [U+1]
    pos_sorted: torch.Tensor   # int32 [n_text] flat rows grouped by token id (stable order)
    feat_src_a: torch.Tensor   # int32 [n_feat_rows] flat row fed by feature row r (first user) or -1
    feat_src_b: torch.Tensor   # int32 [n_feat_rows] second user or -1
    n_sel: int
    pos: Optional[torch.Tensor] = None        # int32 [S*L] RoPE position of every row (packed layout only)
    seg_sh: Optional[torch.Tensor] = None     # int32 [S] end of the shared prefix
    seg_e1: Optional[torch.Tensor] = None     # int32 [S] end of the chosen branch
    shared_len: Optional[List[int]] = None    # per pair (accounting)
    n_real_tokens: int = 0                    # rows that carry a real token / image feature
    row_off: Optional[torch.Tensor] = None    # int32 [S] PAD-FREE packed layout: first token row of packed row s (None: s * L)
    row_len: Optional[torch.Tensor] = None    # int32 [S] ... and its length; L is then the LONGEST row (grid / lse stride / RoPE table)
    n_tokens: int = 0                         # rows of the token-major activation buffers (S * L when rectangular)
    w_sel: Optional[torch.Tensor] = None      # fp32 [n_sel] token weight of each selected row (token-weighted DPO), else None
    # all-positions evaluation of the packed layout (build_packed_plan(all_rows=True), the packed log-prob precompute): every
    # packed row with a successor in its own sequence, pair by pair in buffer order [prefix | chosen | rejected]
    ev_idx: Optional[torch.Tensor] = None     # int32 [n_ev] flat row n that is evaluated
    ev_tgt: Optional[torch.Tensor] = None     # int32 [n_ev] its next label, token id 0 where that label is -100 (return_all=True)
    ev_dst_a: Optional[torch.Tensor] = None   # int32 [n_ev] slot s * ev_ld + t of the per-token matrix [n_seq, ev_ld]
    ev_dst_b: Optional[torch.Tensor] = None   # int32 [n_ev] second slot (prefix rows: the rejected sequence's copy), else -1
    ev_dst_c: Optional[torch.Tensor] = None   # int32 [n_ev] slot in the compact vector = its index in sel_idx / tgt, else -1
    ev_len: Optional[List[int]] = None        # per sequence n_s - 1: the per-token entries it owns (n_s: spliced, truncated, pads dropped)
    ev_ld: int = 0                            # columns of the per-token matrix
    n_ev: int = 0
    # N-branch rows of the yes / no feedback stage (build_branch_plan): row s = [shared prefix | tail 0 | tail 1 | ...]
    q_lo: Optional[torch.Tensor] = None       # int32 [n_tokens] first key (relative to its row) of the token's own branch
    last_idx: Optional[torch.Tensor] = None   # int32 [n_seq] buffer row of each question's last token, in input order

    def to(self, device) -> "SplicePlan":
        kw = {}
        for k, v in self.__dict__.items():
            kw[k] = v.to(device, non_blocking=True) if torch.is_tensor(v) else v
        return SplicePlan(**kw)

    @property
    def seg(self):
        return (self.seg_sh, self.seg_e1) if self.seg_sh is not None and self.q_lo is None else None

    @property
    def branches(self):
        """(seg_sh, q_lo) for rv_attn_fwd_branches, None for every other layout."""
        return (self.seg_sh, self.q_lo) if self.q_lo is not None else None

    @property
    def rows(self):
        """(row_off, row_len) for the attention kernels, None in the rectangular layouts."""
        return (self.row_off, self.row_len) if self.row_off is not None else None


def _splice_rows(input_ids: torch.Tensor, labels: torch.Tensor, n_img_tokens: int, n_images: int,
                 max_len: Optional[int]) -> Tuple[List[torch.Tensor], List[torch.Tensor]]:
    """Per-row spliced sources / labels before padding (llava_arch.py:237-283).  Sequence row r uses image
    ``cur_image_idx % n_images`` where cur_image_idx advances exactly like llava_arch.py:241-266 (one per image
    token, and one for a row without any image token)."""
    S, T = input_ids.shape
    P = n_img_tokens
    rows_src, rows_lab = [], []
    cur_image_idx = 0
    for r in range(S):
        ids, lab = input_ids[r], labels[r]
        is_img = ids == IMAGE_TOKEN_INDEX
        n_img = int(is_img.sum())
        counts = torch.where(is_img, torch.full_like(ids, P), torch.ones_like(ids))
        tok_of = torch.repeat_interleave(torch.arange(T), counts)           # source token of each output slot
        start = torch.cumsum(counts, 0) - counts                           # first output slot of each token
        within = torch.arange(tok_of.numel()) - start[tok_of]              # offset inside an image span
        src_tok = ids[tok_of]
        out_is_img = is_img[tok_of]
        img_rank = (torch.cumsum(is_img.long(), 0) - 1)[tok_of]            # 0-based within the row
        img_global = (cur_image_idx + img_rank) % max(n_images, 1)
        src = torch.where(out_is_img, -2 - (img_global * P + within), src_tok)
        new_lab = torch.where(out_is_img, torch.full_like(src_tok, IGNORE_INDEX), lab[tok_of])
        cur_image_idx += n_img if n_img > 0 else 1
        if max_len is not None:                                            # llava_arch.py:280-283
            src, new_lab = src[:max_len], new_lab[:max_len]
        rows_src.append(src)
        rows_lab.append(new_lab)
    return rows_src, rows_lab


def _check_token_weight(token_weight: Optional[torch.Tensor], splicer, n_seq: int) -> Optional[torch.Tensor]:
    """The collator's ``token_weight [n_seq, T-1]`` (column t weighs the row that predicts label t+1) as fp32 on the CPU.
    Token weights index TEXT positions, so they only apply to a splice that keeps every token at its position (OmniLMM's
    in-place replacement); a length-changing splice (LLaVA-1.5) raises like the reference (trainers.py:246-248)."""
    if token_weight is None:
        return None
    if not getattr(splicer, "keeps_positions", False):
        raise NotImplementedError("token-weighted DPO needs a splice that keeps text positions (OmniLMM): the LLaVA-1.5 splice "
                                  "changes the sequence length, so the text-length token weights do not line up with its "
                                  "rows (the reference raises here too, muffin/train/trainers.py:246-248)")
    token_weight = token_weight.detach().cpu().to(torch.float32)
    if token_weight.dim() != 2 or token_weight.shape[0] != n_seq:
        raise ValueError(f"token_weight must be [{n_seq}, T-1], got {tuple(token_weight.shape)}")
    return token_weight


def _gather_weight(token_weight: torch.Tensor, s: int, cols: torch.Tensor) -> torch.Tensor:
    if cols.numel() and int(cols.max()) >= token_weight.shape[1]:
        raise ValueError(f"token_weight has {token_weight.shape[1]} columns, sequence {s} selects column {int(cols.max())}")
    return token_weight[s, cols]


def make_omnilmm_splicer(im_patch: int, im_start: int, im_end: int):
    """Row splicer for the OmniLMM convention (omnilmm/model/omnilmm.py:221-257, use_im_start_end): the ``num_query``
    <im_patch> embeddings behind an <im_start> are REPLACED by the image's resampler features - no length change, labels
    untouched (the data pipeline already masks them).  ``cur_image_idx`` advances once per <im_start> and not at all for
    a row without <im_patch> tokens; the reference's batch carries cat([images, images]) (trainers.py:190), so global
    image k is distinct image k % n_images.  The reference restarts every replacement from the ORIGINAL row, so a row
    with several images keeps only the last one - reproduced here (one image per sample is the DPO data format)."""
    def splicer(input_ids, labels, n_img_tokens, n_images, max_len):
        rows_src, rows_lab = [], []
        cur = 0
        P = n_img_tokens
        for ids, lab in zip(input_ids, labels):
            src = ids.clone()
            if int((ids == im_patch).sum()) > 0:
                starts = torch.nonzero(ids == im_start, as_tuple=True)[0]
                if starts.numel() != int((ids == im_end).sum()):
                    raise ValueError("The number of image start tokens and image end tokens should be the same.")
                for p in starts.tolist():
                    if p + P + 1 >= ids.numel() or int(ids[p + P + 1]) != im_end:
                        raise ValueError("The image end token should follow the image start token.")
                    src = ids.clone()
                    src[p + 1:p + 1 + P] = -2 - ((cur % max(n_images, 1)) * P + torch.arange(P))
                    cur += 1
            if max_len is not None:
                src, lab = src[:max_len], lab[:max_len]
            rows_src.append(src)
            rows_lab.append(lab.clone())
        return rows_src, rows_lab
    splicer.keeps_positions = True          # row position = text position: token weights apply (build_*_plan token_weight)
    return splicer


def _tables(flat: torch.Tensor, n_feat_rows: int, strict: bool = True):
    """Embedding-backward segments and feature-gradient sources from the flat source table.  ``strict=False`` (forward-only
    plans whose rows may repeat an image): a feature row with more than two users keeps its first two."""
    text_rows = torch.nonzero(flat >= 0, as_tuple=True)[0]
    text_ids = flat[text_rows]
    order = torch.sort(text_ids, stable=True).indices
    sorted_ids = text_ids[order]
    pos_sorted = text_rows[order].to(torch.int32)
    uniq, counts_u = torch.unique_consecutive(sorted_ids, return_counts=True)
    seg_off = torch.zeros(uniq.numel() + 1, dtype=torch.int32)
    seg_off[1:] = torch.cumsum(counts_u, 0).to(torch.int32)

    feat_rows = torch.nonzero(flat <= -2, as_tuple=True)[0]
    feat_ids = (-2 - flat[feat_rows])
    a = torch.full((n_feat_rows,), -1, dtype=torch.int32)
    b = torch.full((n_feat_rows,), -1, dtype=torch.int32)
    if feat_rows.numel():
        # users of a feature row appear in increasing flat order; with one image per sample there are at most
        # two (the chosen and the rejected sequence of the pair; one when the image lies in the shared prefix)
        order_f = torch.sort(feat_ids, stable=True).indices
        fid_s, frow_s = feat_ids[order_f], feat_rows[order_f]
        first = torch.ones_like(fid_s, dtype=torch.bool)
        first[1:] = fid_s[1:] != fid_s[:-1]
        second = torch.zeros_like(first)
        second[1:] = (~first[1:]) & first[:-1]
        if strict and bool((~(first | second)).any()):
            raise ValueError("an image feature row is used by more than two sequence positions; "
                             "the DPO path expects one image per (chosen, rejected) pair")
        a[fid_s[first]] = frow_s[first].to(torch.int32)
        b[fid_s[second]] = frow_s[second].to(torch.int32)
    return uniq.to(torch.int32), seg_off, pos_sorted, a, b


def build_splice_plan(input_ids: torch.Tensor, labels: torch.Tensor, n_img_tokens: int, n_images: int,
                      max_len: Optional[int], label_shift: int = 1, splicer=None,
                      token_weight: Optional[torch.Tensor] = None) -> SplicePlan:
    """Reference layout.  input_ids/labels: int64 [S, T] (the collator's ``concatenated_*`` tensors);
    ``n_images`` distinct images were encoded (one per pair).  label_shift = 1: get_batch_logps
    (labels[:, 1:] vs logits[:, :-1], muffin_inference_logp.py:93-94); 0: get_batch_logps_minicpm (labels already
    shifted by the data pipeline: labels[:, :-1] vs logits[:, :-1], :32-33).
    ``token_weight`` [S, T-1] (token-weighted DPO, position-keeping splicers only): selected row (s, t) takes
    token_weight[s, t]; returned in selection order as ``w_sel``."""
    if label_shift not in (0, 1):
        raise ValueError("label_shift must be 0 (minicpm) or 1 (llava / omnilmm)")
    token_weight = _check_token_weight(token_weight, splicer, input_ids.shape[0])
    if token_weight is not None and label_shift != 1:
        raise NotImplementedError("token weights under the minicpm label convention (label_shift=0)")
    input_ids = input_ids.cpu().long()
    labels = labels.cpu().long()
    S = input_ids.shape[0]
    rows_src, rows_lab = (splicer or _splice_rows)(input_ids, labels, n_img_tokens, n_images, max_len)
    L = max(int(x.numel()) for x in rows_src)                              # :286
    src_full = torch.full((S, L), -1, dtype=torch.int64)                   # zero-embedding right pad (:305-313)
    lab_full = torch.full((S, L), IGNORE_INDEX, dtype=torch.int64)
    for r in range(S):
        n = rows_src[r].numel()
        src_full[r, :n] = rows_src[r]
        lab_full[r, :n] = rows_lab[r]

    # rows whose next-position label is a target (labels[:,1:] vs logits[:,:-1]; minicpm: labels[:,:-1])
    nxt = lab_full[:, 1:] if label_shift == 1 else lab_full[:, :-1]
    mask = nxt != IGNORE_INDEX                                             # [S, L-1]
    s_idx, l_idx = torch.nonzero(mask, as_tuple=True)                      # row-major order: by s then l
    sel = (s_idx * L + l_idx).to(torch.int32)
    tgt = nxt[mask].to(torch.int32)
    seq_off = torch.zeros(S + 1, dtype=torch.int32)
    seq_off[1:] = torch.cumsum(mask.sum(1), 0).to(torch.int32)

    w_sel = None
    if token_weight is not None:
        if l_idx.numel() and int(l_idx.max()) >= token_weight.shape[1]:
            raise ValueError(f"token_weight has {token_weight.shape[1]} columns, a target sits at column {int(l_idx.max())}")
        w_sel = token_weight[s_idx, l_idx].contiguous()

    flat = src_full.reshape(-1)
    uniq, seg_off, pos_sorted, a, b = _tables(flat, max(n_images, 1) * n_img_tokens)
    return SplicePlan(S=S, L=L, n_seq=S, src=flat.to(torch.int32), labels=lab_full, sel_idx=sel, tgt=tgt,
                      seq_off=seq_off, seq_of_row=s_idx.to(torch.int32), uniq_ids=uniq, seg_off=seg_off,
                      pos_sorted=pos_sorted, feat_src_a=a, feat_src_b=b, n_sel=int(sel.numel()),
                      n_real_tokens=int(sum(x.numel() for x in rows_src)), n_tokens=S * L, w_sel=w_sel)


def _eval_rows(cl: torch.Tensor, rl: torch.Tensor, sh: int):
    """The evaluated rows of one pair (build_packed_plan(all_rows=True)) from its chosen / rejected labels and shared length:
    (row offset in the packed row, position t, branch 0 | 1, target, rank among its sequence's real targets or -1)."""
    Lc, Lr = cl.numel(), rl.numel()
    assert sh <= min(Lc, Lr) - 1
    # prefix rows are evaluated once for both sequences: both must ask for the masked-position target there
    assert bool((cl[1:sh + 1] == IGNORE_INDEX).all()) and bool((rl[1:sh + 1] == IGNORE_INDEX).all()), \
        "a shared-prefix row predicts a real target"
    tc, tr = torch.arange(0, Lc - 1), torch.arange(sh, Lr - 1)
    t = torch.cat([tc, tr])
    row = torch.cat([tc, Lc + (tr - sh)])
    br = torch.cat([torch.zeros_like(tc), torch.ones_like(tr)])
    nxt = torch.cat([cl[1:], rl[sh + 1:]])
    real = nxt != IGNORE_INDEX
    rank_c = torch.cumsum(real[:Lc - 1].long(), 0) - 1
    rank_r = torch.cumsum(real[Lc - 1:].long(), 0) - 1
    rank = torch.where(real, torch.cat([rank_c, rank_r]), torch.full_like(t, -1))
    return row, t, br, torch.where(real, nxt, torch.zeros_like(nxt)), rank


def build_packed_plan(input_ids: torch.Tensor, labels: torch.Tensor, n_img_tokens: int, n_images: int,
                      max_len: Optional[int], pad_token_id: int = 0, splicer=None, pad_free: bool = False,
                      token_weight: Optional[torch.Tensor] = None, all_rows: bool = False) -> SplicePlan:
    """One row per pair: [shared prefix | chosen branch | rejected branch] (module docstring).
    input_ids / labels: [2B, T], wins then rejects.
    ``pad_free``: the B packed rows are CONCATENATED (row b starts at row_off[b], no inter-row padding) instead of being
    right-padded to the longest - the reference pads every row to the batch maximum (llava/model/llava_arch.py:305-313) and
    SURVEY 8a property (i) (a sequence's log-prob does not depend on its padding or its batch mates) makes dropping those rows
    exact.  Everything token-major (GEMMs, norms, SwiGLU, LM head, splice, embedding gradient) simply sees fewer rows; the
    attention kernels take (row_off, row_len) and the RoPE position table is indexed by buffer row.  Identical index tables up
    to the row renumbering: selected rows / targets / sequence offsets keep their (sequence, position) order.
    ``token_weight`` [2B, T-1]: chosen rows take token_weight[b, i], rejected rows token_weight[B+b, i] for the text position
    i of the row (``w_sel``, same order as ``tgt``).
    ``all_rows``: the same plan plus the ``ev_*`` tables of the all-positions evaluation (get_batch_logps(return_all=True),
    muffin_inference_logp.py:93-115, on the packed row): position t of sequence s, t < n_s - 1, is packed row t of its pair when
    it is chosen or lies in the shared prefix, row Lc + (t - sh) when it is rejected; its target is label[s][t + 1] or token
    id 0.  A prefix row is evaluated ONCE and lands in both sequences' per-token rows (sh <= first target - 1: both want
    target 0 there); the rows with a real target also land in the compact vector, at their index in ``sel_idx``."""
    input_ids = input_ids.cpu().long()
    labels = labels.cpu().long()
    S2 = input_ids.shape[0]
    if all_rows and token_weight is not None:
        raise ValueError("all_rows returns per-token log-probs; token weights apply to the selected-row step")
    token_weight = _check_token_weight(token_weight, splicer, S2)
    if S2 % 2:
        raise ValueError("packed layout needs wins followed by the same number of rejects")
    B = S2 // 2
    rows_src, rows_lab = (splicer or _splice_rows)(input_ids, labels, n_img_tokens, n_images, max_len)
    for r in range(S2):        # drop the collator's right padding (pad id with label -100 at the very end)
        pad = (rows_src[r] == pad_token_id) & (rows_lab[r] == IGNORE_INDEX)
        keep = int(torch.nonzero(~pad)[-1]) + 1 if bool((~pad).any()) else 1
        rows_src[r], rows_lab[r] = rows_src[r][:keep], rows_lab[r][:keep]

    def first_target(lab):
        nz = torch.nonzero(lab != IGNORE_INDEX)
        return int(nz[0]) if nz.numel() else int(lab.numel())

    packed_src, packed_pos, shs, e1s = [], [], [], []
    sel_rows: List[List[torch.Tensor]] = [[None] * B, [None] * B]          # [branch][pair] -> row offsets in the packed row
    sel_tgts: List[List[torch.Tensor]] = [[None] * B, [None] * B]
    sel_w: List[List[torch.Tensor]] = [[None] * B, [None] * B]
    ev: List[Tuple[torch.Tensor, ...]] = []                                # per pair (all_rows)
    for b in range(B):
        cs, cl, rs, rl = rows_src[b], rows_lab[b], rows_src[B + b], rows_lab[B + b]
        n = min(cs.numel(), rs.numel())
        eq = (cs[:n] == rs[:n]) & (cl[:n] == rl[:n])
        ne = torch.nonzero(~eq)
        lcp = int(ne[0]) if ne.numel() else n
        sh = max(0, min(lcp - 1, min(first_target(cl), first_target(rl)) - 1))
        Lc, Lr = cs.numel(), rs.numel()
        packed_src.append(torch.cat([cs, rs[sh:]]))
        packed_pos.append(torch.cat([torch.arange(Lc), torch.arange(sh, Lr)]))
        shs.append(sh)
        e1s.append(Lc)
        ci = torch.nonzero(cl[1:] != IGNORE_INDEX, as_tuple=True)[0]       # row i predicts label i+1
        ri = torch.nonzero(rl[1:] != IGNORE_INDEX, as_tuple=True)[0]
        assert (ri >= sh).all() and (ci >= sh).all() or sh == 0
        sel_rows[0][b], sel_tgts[0][b] = ci, cl[1:][ci]
        sel_rows[1][b], sel_tgts[1][b] = Lc + (ri - sh), rl[1:][ri]
        if token_weight is not None:
            sel_w[0][b], sel_w[1][b] = _gather_weight(token_weight, b, ci), _gather_weight(token_weight, B + b, ri)
        if all_rows:
            ev.append(_eval_rows(cl, rl, sh))
    L = max(int(x.numel()) for x in packed_src)
    lens = [int(x.numel()) for x in packed_src]
    if pad_free:
        starts = [0] * B
        for b in range(1, B):
            starts[b] = starts[b - 1] + lens[b - 1]
        n_tokens = starts[-1] + lens[-1]
        flat = torch.cat(packed_src)
        pos_flat = torch.cat(packed_pos)
    else:
        starts = [b * L for b in range(B)]
        n_tokens = B * L
        src_full = torch.full((B, L), -1, dtype=torch.int64)
        pos_full = torch.zeros((B, L), dtype=torch.int64)
        for b in range(B):
            n = packed_src[b].numel()
            src_full[b, :n] = packed_src[b]
            pos_full[b, :n] = packed_pos[b]
        flat, pos_flat = src_full.reshape(-1), pos_full.reshape(-1)
    sel, tgt, seq_of, counts, ws = [], [], [], [], []
    for br in range(2):
        for b in range(B):
            if token_weight is not None:
                ws.append(sel_w[br][b])
            sel.append(starts[b] + sel_rows[br][b])
            tgt.append(sel_tgts[br][b])
            seq_of.append(torch.full((sel_rows[br][b].numel(),), br * B + b, dtype=torch.int64))
            counts.append(sel_rows[br][b].numel())
    sel = torch.cat(sel).to(torch.int32)
    tgt = torch.cat(tgt).to(torch.int32)
    seq_of = torch.cat(seq_of).to(torch.int32)
    seq_off = torch.zeros(S2 + 1, dtype=torch.int32)
    seq_off[1:] = torch.cumsum(torch.tensor(counts), 0).to(torch.int32)
    uniq, seg_off, pos_sorted, a, bb = _tables(flat, max(n_images, 1) * n_img_tokens)
    evkw = {}
    if all_rows:
        ev_len = [int(x.numel()) - 1 for x in rows_src]
        ld = max(ev_len)
        if getattr(splicer, "keeps_positions", False):
            # row position = text position: the per-token rows keep the collator's T - 1 columns (its token weights' layout)
            ld = max(ld, min(input_ids.shape[1], max_len or input_ids.shape[1]) - 1)
        rows, tg, da, db, dc = [], [], [], [], []
        for b, (row, t, br, tgt_b, rank) in enumerate(ev):
            s = b + br * B                                                 # the sequence that owns the row (prefix: chosen)
            rows.append(starts[b] + row)
            tg.append(tgt_b)
            da.append(s * ld + t)
            db.append(torch.where(t < shs[b], (B + b) * ld + t, torch.full_like(t, -1)))
            dc.append(torch.where(rank >= 0, seq_off[s.long()].long() + rank, torch.full_like(rank, -1)))
        i32 = lambda xs: torch.cat(xs).to(torch.int32)                     # noqa: E731
        evkw = dict(ev_idx=i32(rows), ev_tgt=i32(tg), ev_dst_a=i32(da), ev_dst_b=i32(db), ev_dst_c=i32(dc), ev_len=ev_len,
                    ev_ld=ld, n_ev=int(sum(x.numel() for x in rows)))
    return SplicePlan(**evkw, S=B, L=L, n_seq=S2, src=flat.to(torch.int32), labels=None, sel_idx=sel, tgt=tgt, seq_off=seq_off,
                      seq_of_row=seq_of, uniq_ids=uniq, seg_off=seg_off, pos_sorted=pos_sorted, feat_src_a=a,
                      feat_src_b=bb, n_sel=int(sel.numel()), pos=pos_flat.to(torch.int32),
                      seg_sh=torch.tensor(shs, dtype=torch.int32), seg_e1=torch.tensor(e1s, dtype=torch.int32),
                      shared_len=shs, n_real_tokens=int(sum(lens)), n_tokens=n_tokens,
                      row_off=torch.tensor(starts, dtype=torch.int32) if pad_free else None,
                      row_len=torch.tensor(lens, dtype=torch.int32) if pad_free else None,
                      w_sel=torch.cat(ws).contiguous() if token_weight is not None else None)


def check_branch_rows(seg_sh: torch.Tensor, q_lo: torch.Tensor, starts: List[int], lens: List[int]) -> None:
    """The conditions rv_attn_fwd_branches relies on and does not check: for every query i >= seg_sh[s] of row s (token row
    starts[s] + i, i < lens[s]),  seg_sh[s] <= q_lo[i] <= i,  and q_lo does not decrease inside a row."""
    n = int(q_lo.numel())
    for s, (a, ln) in enumerate(zip(starts, lens)):
        sh = int(seg_sh[s])
        if not (ln >= 1 and 0 <= a and a + ln <= n):
            raise ValueError(f"branch row {s}: token rows [{a}, {a + ln}) do not fit the q_lo table of {n} entries")
        if not 0 <= sh <= ln:
            raise ValueError(f"branch row {s}: shared prefix {sh} outside [0, {ln}]")
        q = q_lo[a + sh:a + ln].long()
        i = torch.arange(sh, ln)
        if bool((q < sh).any()) or bool((q > i).any()):
            raise ValueError(f"branch row {s}: q_lo must satisfy seg_sh <= q_lo[i] <= i for every query behind the prefix")
        if bool((q[1:] < q[:-1]).any()):
            raise ValueError(f"branch row {s}: q_lo decreases inside the row")


def _splice_one(ids: torch.Tensor, image: int, n_img_tokens: int, splicer) -> torch.Tensor:
    """One prompt spliced on its own (no truncation); its image-feature sources re-pointed at feature block ``image``."""
    ids = ids.cpu().long().reshape(1, -1)
    rows, _ = (splicer or _splice_rows)(ids, torch.full_like(ids, IGNORE_INDEX), n_img_tokens, 1, None)
    src = rows[0]
    return torch.where(src <= -2, src - image * n_img_tokens, src)


def _shared_len(rows: List[torch.Tensor]) -> int:
    """Longest common prefix of the spliced rows that leaves every row a token of its own and does not end inside an image
    block (a run of consecutive feature sources).  A single row shares nothing: it is a plain causal row."""
    if len(rows) == 1:
        return 0
    n = min(int(r.numel()) for r in rows)
    eq = torch.ones(n, dtype=torch.bool)
    for r in rows[1:]:
        eq &= r[:n] == rows[0][:n]
    ne = torch.nonzero(~eq)
    sh = min(int(ne[0]) if ne.numel() else n, n - 1)

    def cuts(k):       # the cut between k - 1 and k separates two features of one block in some row
        return k > 0 and any(int(r[k - 1]) <= -2 and int(r[k]) == int(r[k - 1]) - 1 for r in rows)
    while cuts(sh):
        sh -= 1
    return sh


def build_branch_plan(prompts: List[List[torch.Tensor]], n_img_tokens: int, model_max_length: Optional[int], splicer=None,
                      pad_free: bool = True, max_row_tokens: Optional[int] = None, packed: bool = True) -> SplicePlan:
    """Forward-only plan of the yes / no feedback stage (muffin/llava15_gen_data.py:266-333, omnilmm/omnilmm_gen_data.py:245-300:
    one prefill per question, only the next-token distribution behind the prompt is kept).
    ``prompts[k]``: the full prompts (1-D input_ids with the image placeholder) of the questions about image k; image k's
    features are feature rows [k * n_img_tokens, (k + 1) * n_img_tokens).
    ``packed``: per image every prompt is spliced on its own, the rows' longest common prefix (never cutting an image block) is
    kept once and the row is [prefix | tail 0 | tail 1 | ...]: under a causal mask a prefix position sees the same keys in every
    stand-alone sequence, so its hidden states are shared; a tail token attends the prefix and its own tail (``seg_sh`` /
    ``q_lo``, rv_attn_fwd_branches) and keeps the position it has in its stand-alone sequence (``pos``).  A row that would
    exceed ``max_row_tokens`` is continued in a new row that carries the prefix again (a row always takes at least one tail).
    ``packed=False``: one plain causal row per question (no seg_sh / q_lo: the existing attention kernel).
    ``last_idx``: the buffer row of each question's last token, questions in input order (image by image).  A stand-alone
    sequence longer than ``model_max_length`` raises ValueError (the stage scores complete prompts)."""
    P = n_img_tokens
    packed_src, packed_pos, packed_qlo, shs = [], [], [], []
    last_rel: List[Tuple[int, int]] = []                                   # per question: (row, offset in the row)
    for k, plist in enumerate(prompts):
        if len(plist) == 0:
            raise ValueError(f"image {k} has no question")
        rows = [_splice_one(ids, k, P, splicer) for ids in plist]
        for r in rows:
            if r.numel() == 0:
                raise ValueError(f"image {k}: empty prompt")
            if model_max_length is not None and r.numel() > model_max_length:
                raise ValueError(f"image {k}: a spliced prompt has {r.numel()} tokens, model_max_length is {model_max_length}")
        if not packed:
            for r in rows:
                last_rel.append((len(packed_src), int(r.numel()) - 1))
                packed_src.append(r)
                packed_pos.append(torch.arange(r.numel()))
            continue
        sh = _shared_len(rows)
        j = 0
        while j < len(rows):
            src, pos, qlo = [rows[0][:sh]], [torch.arange(sh)], [torch.zeros(sh, dtype=torch.int64)]
            n = sh
            while j < len(rows) and (n == sh or max_row_tokens is None or n + rows[j].numel() - sh <= max_row_tokens):
                t = int(rows[j].numel()) - sh
                src.append(rows[j][sh:])
                pos.append(torch.arange(sh, sh + t))
                qlo.append(torch.full((t,), n, dtype=torch.int64))
                n += t
                last_rel.append((len(packed_src), n - 1))
                j += 1
            packed_src.append(torch.cat(src))
            packed_pos.append(torch.cat(pos))
            packed_qlo.append(torch.cat(qlo))
            shs.append(sh)
    S = len(packed_src)
    lens = [int(x.numel()) for x in packed_src]
    L = max(lens)
    if pad_free:
        starts = [0] * S
        for b in range(1, S):
            starts[b] = starts[b - 1] + lens[b - 1]
        n_tokens = starts[-1] + lens[-1]
        flat, pos_flat = torch.cat(packed_src), torch.cat(packed_pos)
        qlo_flat = torch.cat(packed_qlo) if packed else None
    else:
        starts = [b * L for b in range(S)]
        n_tokens = S * L
        src_full = torch.full((S, L), -1, dtype=torch.int64)
        pos_full = torch.zeros((S, L), dtype=torch.int64)
        qlo_full = torch.zeros((S, L), dtype=torch.int64)
        for b in range(S):
            src_full[b, :lens[b]], pos_full[b, :lens[b]] = packed_src[b], packed_pos[b]
            if packed:                       # the pad queries behind a row continue its last branch (their results are not read)
                qlo_full[b, :lens[b]] = packed_qlo[b]
                qlo_full[b, lens[b]:] = packed_qlo[b][-1]
        flat, pos_flat = src_full.reshape(-1), pos_full.reshape(-1)
        qlo_flat = qlo_full.reshape(-1) if packed else None
    seg_sh = torch.tensor(shs, dtype=torch.int32) if packed else None
    q_lo = qlo_flat.to(torch.int32) if packed else None
    if packed:
        check_branch_rows(seg_sh, q_lo, starts, lens if pad_free else [L] * S)
    last_idx = torch.tensor([starts[r] + o for r, o in last_rel], dtype=torch.int32)
    uniq, seg_off, pos_sorted, a, bb = _tables(flat, max(len(prompts), 1) * P, strict=False)
    e32 = torch.zeros(0, dtype=torch.int32)
    n_q = len(last_rel)
    return SplicePlan(S=S, L=L, n_seq=n_q, src=flat.to(torch.int32), labels=None, sel_idx=e32, tgt=e32,
                      seq_off=torch.zeros(n_q + 1, dtype=torch.int32), seq_of_row=e32, uniq_ids=uniq, seg_off=seg_off,
                      pos_sorted=pos_sorted, feat_src_a=a, feat_src_b=bb, n_sel=0, pos=pos_flat.to(torch.int32), seg_sh=seg_sh,
                      shared_len=shs if packed else None, n_real_tokens=int(sum(lens)), n_tokens=n_tokens,
                      row_off=torch.tensor(starts, dtype=torch.int32) if pad_free else None,
                      row_len=torch.tensor(lens, dtype=torch.int32) if pad_free else None, q_lo=q_lo, last_idx=last_idx)


# ------------------------------------------------------------------------------------------------ KV-cached generation
@dataclass
class DecodeRows:
    """Cache rows of ``LlavaDPOModel.generate``: every layer's cache is one [n_rows][2 kv_dim] buffer.  Rows [0, n_prefill) hold
    the prompts exactly where the pad-free prefill put them; sequence m = prompt * repeat + sample then owns ``max_new`` rows of
    its own behind them.  The samples of one prompt name the same prompt span (``pre_off`` / ``pre_len``): it is stored once."""
    n_seq: int
    n_rows: int                # rows of one layer's cache
    prompt_of: torch.Tensor    # int32 [n_seq] the prompt (= prefill row) a sequence continues
    pre_off: torch.Tensor      # int32 [n_seq] first cache row of its prompt
    pre_len: torch.Tensor      # int32 [n_seq] tokens of the spliced prompt
    own_off: torch.Tensor      # int32 [n_seq] first cache row of its generated tokens
    chunks: List[Tuple[int, int]]   # [c0, c1) sequence ranges of at most ``max_rows`` rows: one launch set per chunk and step

    def step(self, j: int) -> Tuple[torch.Tensor, torch.Tensor, torch.Tensor]:
        """Decode step j (it feeds generated token j, j = 0 the token sampled from the prefill): (RoPE position of that token,
        the cache row its K | V go to, own_len INCLUDING it), int32 [n_seq] each."""
        return self.pre_len + j, self.own_off + j, torch.full_like(self.pre_len, j + 1)


def plan_decode_rows(row_off: Sequence[int], row_len: Sequence[int], repeat: int, max_new: int, max_rows: int = 64) -> DecodeRows:
    """``row_off`` / ``row_len``: the pad-free prefill rows of the prompts (build_branch_plan(packed=False)), in prompt order."""
    if repeat < 1 or max_new < 1 or max_rows < 1:
        raise ValueError("plan_decode_rows: repeat, max_new and max_rows must be >= 1")
    if len(row_off) != len(row_len) or len(row_off) == 0:
        raise ValueError("plan_decode_rows: one (row_off, row_len) pair per prompt, at least one prompt")
    off, ln = [int(x) for x in row_off], [int(x) for x in row_len]
    if any(n < 1 for n in ln):
        raise ValueError("plan_decode_rows: empty prompt")
    n_prefill = max(o + n for o, n in zip(off, ln))
    n_seq = len(off) * repeat
    prompt_of = torch.arange(len(off), dtype=torch.int32).repeat_interleave(repeat)
    i32 = lambda v: torch.tensor(v, dtype=torch.int32)                   # noqa: E731
    return DecodeRows(n_seq=n_seq, n_rows=n_prefill + n_seq * max_new, prompt_of=prompt_of,
                      pre_off=i32(off)[prompt_of.long()], pre_len=i32(ln)[prompt_of.long()],
                      own_off=n_prefill + torch.arange(n_seq, dtype=torch.int32) * max_new,
                      chunks=[(c, min(c + max_rows, n_seq)) for c in range(0, n_seq, max_rows)])


@dataclass
class BeamRows:
    """Cache rows of ``LlavaDPOModel.beam_search``, the beam counterpart of ``DecodeRows``: sequence m = prompt * num_beams + beam;
    the beams of a prompt share its prompt span.  No beam owns rows: step j writes the K | V of sequence m to the fresh row
    ``own_base + j * n_seq + m`` (step-major) and a per-beam row table (rv_beam_step) names the rows of its ancestry, so a
    reselection of beams moves table entries, never cache rows."""
    n_seq: int
    n_rows: int                # rows of one layer's cache
    num_beams: int
    prompt_of: torch.Tensor    # int32 [n_seq] the prompt (= prefill row) a sequence continues
    pre_off: torch.Tensor      # int32 [n_seq] first cache row of its prompt
    pre_len: torch.Tensor      # int32 [n_seq] tokens of the spliced prompt
    own_base: int              # first cache row behind the prompts
    seq_idx: torch.Tensor      # int32 [n_seq] 0 .. n_seq - 1
    chunks: List[Tuple[int, int]]   # [c0, c1) sequence ranges of at most ``max_rows`` rows, whole groups only

    def step(self, j: int) -> Tuple[torch.Tensor, torch.Tensor, torch.Tensor]:
        """Decode step j (it feeds generated token j): (RoPE position of that token, the cache row its K | V go to, own_len
        INCLUDING it), int32 [n_seq] each."""
        return self.pre_len + j, self.seq_idx + (self.own_base + j * self.n_seq), torch.full_like(self.pre_len, j + 1)


def plan_beam_rows(row_off: Sequence[int], row_len: Sequence[int], num_beams: int, max_new: int, max_rows: int = 64) -> BeamRows:
    """``row_off`` / ``row_len``: the pad-free prefill rows of the prompts (build_branch_plan(packed=False)), in prompt order."""
    if num_beams < 1 or max_new < 1 or max_rows < 1:
        raise ValueError("plan_beam_rows: num_beams, max_new and max_rows must be >= 1")
    if num_beams > max_rows:
        raise ValueError("plan_beam_rows: a chunk of max_rows rows must hold a whole group of num_beams beams")
    if len(row_off) != len(row_len) or len(row_off) == 0:
        raise ValueError("plan_beam_rows: one (row_off, row_len) pair per prompt, at least one prompt")
    off, ln = [int(x) for x in row_off], [int(x) for x in row_len]
    if any(n < 1 for n in ln) or any(o < 0 for o in off):
        raise ValueError("plan_beam_rows: empty prompt or negative row offset")
    n_prefill = max(o + n for o, n in zip(off, ln))
    n_seq = len(off) * num_beams
    if n_prefill + n_seq * max_new > 2 ** 31 - 1:
        raise ValueError("plan_beam_rows: the cache rows do not fit int32")
    prompt_of = torch.arange(len(off), dtype=torch.int32).repeat_interleave(num_beams)
    i32 = lambda v: torch.tensor(v, dtype=torch.int32)                   # noqa: E731
    per = (max_rows // num_beams) * num_beams
    return BeamRows(n_seq=n_seq, n_rows=n_prefill + n_seq * max_new, num_beams=num_beams, prompt_of=prompt_of,
                    pre_off=i32(off)[prompt_of.long()], pre_len=i32(ln)[prompt_of.long()], own_base=n_prefill,
                    seq_idx=torch.arange(n_seq, dtype=torch.int32),
                    chunks=[(c, min(c + per, n_seq)) for c in range(0, n_seq, per)])


# ------------------------------------------------------------------------------------------------ end-of-sequence ids
def eos_id_set(eos_token_id) -> Optional[Tuple[int, ...]]:
    """``generate(eos_token_id=...)`` as a tuple of distinct ids in the caller's order: None stays None, an int is a set of one,
    a sequence of ints (HF's ``eos_token_id=[eos, <|eot_id|>]``) is taken as it is.  Anything else raises ValueError."""
    if eos_token_id is None:
        return None
    if isinstance(eos_token_id, bool):
        raise ValueError("eos_token_id must be an int or a sequence of ints")
    if isinstance(eos_token_id, numbers.Integral):
        return (int(eos_token_id),)
    if torch.is_tensor(eos_token_id):
        eos_token_id = eos_token_id.reshape(-1).tolist()
    try:
        ids = [i for i in eos_token_id]
    except TypeError:
        raise ValueError("eos_token_id must be an int or a sequence of ints") from None
    if len(ids) == 0 or any(isinstance(i, bool) or not isinstance(i, numbers.Integral) for i in ids):
        raise ValueError("eos_token_id must be an int or a non-empty sequence of ints")
    return tuple(dict.fromkeys(int(i) for i in ids))


def cut_behind_eos(seq: List[int], eos_ids: Optional[Tuple[int, ...]]) -> List[int]:
    """The generated ids up to and including the first one that is in ``eos_ids`` (all of them when there is none)."""
    if eos_ids:
        for n, t in enumerate(seq):
            if t in eos_ids:
                return seq[:n + 1]
    return seq
