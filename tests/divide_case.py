"""Shared pieces of the claim-splitting tests (tests/test_divide_host.py, tests/test_sample_wide_gpu.py,
tests/test_text_generate_gpu.py; a plain helper module like generate_case.py):

  * the planted logits rows of the wide sampler's tests - a background of probability <= 1e-13 per token and seven planted
    tokens that carry the mass, so that the float64 restatement (generate_case.sampler_probs64 / sampler_choice64) decides every
    planted uniform even at V = 128256, where the fp32 error of a V-term sum (V 2^-24 = 7.6e-3) is coarse;
  * the runner that calls rv_sample_token_wide on tests/guarded.py windows;
  * the fp32 evaluation bound of logp (test_decode_kernels_gpu.py::_logp_bound restated);
  * the tiny text model and the stub tokenizer of the end-to-end tests."""
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import accuracy as A  # noqa: E402
import generate_case as GC  # noqa: E402
from guarded import Guarded  # noqa: E402

HERE = os.path.dirname(os.path.abspath(__file__))
GOLD_HOST = os.path.join(HERE, "golden", "divide_host.json")
GOLD_TEXT = os.path.join(HERE, "golden", "text_generate_tiny.pt")
U32 = 2.0 ** -24
U_LAST = float(np.nextafter(np.float32(1.0), np.float32(0.0)))
F32, I32 = torch.float32, torch.int32
PLANTED_D = (0.30, 0.22, 0.18, 0.14, 0.11, 0.03, 0.02)


# ------------------------------------------------------------------------------------------------ planted rows
def planted_ids(V):
    """0, 4095, 4096, 65535, 65536, V // 2 + 1 and V - 1, clipped to the row (those inside it, each once, ascending)"""
    return sorted({i for i in (0, 4095, 4096, 65535, 65536, V // 2 + 1, V - 1) if 0 <= i < V})


def planted_row(V, temperature, seed):
    """fp32 [V]: background T (log 1e-13 - 3 rand), planted logits T log d for a seeded permutation of PLANTED_D (T = 1 in the
    greedy case): after the division by T the planted tokens hold all but 1e-8 of the mass in the proportions d."""
    T = temperature if temperature else 1.0
    g = np.random.default_rng(seed)
    row = T * (np.log(1e-13) - 3.0 * g.random(V))
    ids = planted_ids(V)
    d = g.permutation(np.asarray(PLANTED_D))[:len(ids)]
    row[ids] = T * np.log(d)
    return row.astype(np.float32)


def planted_seen(V, row):
    """the top id twice, 5, V - 1, -1 and V + 7: duplicates and ids outside the row among them"""
    top = int(np.argmax(row))
    return [top, top, 5, V - 1, -1, V + 7]


def planted_uniforms(p, bound):
    """0, the largest float below 1 and the middle of every CDF interval (vocabulary order) wider than 8 bounds"""
    kept = np.nonzero(p > 0)[0]
    hi = np.cumsum(p[kept])
    wide = np.nonzero(p[kept] > 8 * bound)[0]
    return [0.0, U_LAST] + [float(np.float32(hi[i] - 0.5 * p[kept][i])) for i in wide]


def logp_bound(row, p, temperature, seen=None, penalty=1.0):
    """|logp - log p_tok| of the fp32 evaluation (x_t - max) - log(sum exp(x_i - max)): the division by the temperature and the
    penalty (2^-24 |x| each, on x_t and on the maximum), the subtraction, per term exp's (|x_i - max| + 2) 2^-23 and the two
    operand roundings weighted by the term's share, the V-term sum, logf (FEW) and the last subtraction."""
    x = GC.penalised(row, seen, penalty) / (float(np.float32(temperature)) if temperature else 1.0)
    mx = x.max()
    kept = p > 0
    rel = ((np.abs(x - mx) + 2.0) * 2.0 * U32 + 2.0 * U32 * (np.abs(x) + abs(mx)))
    zerr = float((p * rel)[kept].sum()) + int(kept.sum()) * U32
    lz = np.log(np.exp(x[kept] - mx).sum())
    return lambda t: (2.0 * U32 * (abs(x[t]) + abs(mx)) + U32 * abs(x[t] - mx) + zerr + A.FEW * U32 * abs(lz)
                      + U32 * abs(np.log(p[t])) + 2.0 * U32)


# ------------------------------------------------------------------------------------------------ the kernel on guarded windows
def call(name, *args):
    import pytest
    from rlaif_v_amd import hip
    try:
        hip.call(name, *args)
        torch.cuda.synchronize()
    except RuntimeError as e:
        if "HIP error" in str(e) or "illegal memory access" in str(e):      # a faulted device: start nothing more on it
            pytest.exit(f"GPU fault in {name}: {e}", returncode=3)
        raise


def run_wide(dev, rows, V, ldl, us, temperature, top_p, seens=None, penalty=1.0):
    """rv_sample_token_wide on n = len(us) rows.  rows: fp32 [V] (every row the same logits) or [n][V]; seens: None, one list
    (every row names it) or n lists.  The columns behind V (ldl > V), the rows around the window and the band around the
    workspace are poisoned and checked.  -> (token int64 [n], logp float64 [n], logp bits int32 [n])"""
    from rlaif_v_amd import hip
    n = len(us)
    rows = np.asarray(rows, dtype=np.float32)
    fill = torch.zeros(n, ldl)
    fill[:, :V] = torch.from_numpy(rows).reshape(-1, V)
    inner = torch.zeros(n, ldl, dtype=torch.bool)
    inner[:, V:] = True
    gl = Guarded(n, ldl, F32, dev, fill=fill, name="logits", inner=inner, guard_cols=0, guard_rows=4)
    assert gl.ld == ldl
    gu = Guarded(1, n, F32, dev, fill=torch.tensor(us, dtype=F32)[None], name="u", guard_rows=0)
    gt = Guarded(1, n, I32, dev, name="token", guard_rows=0)
    gp = Guarded(1, n, F32, dev, name="logp", guard_rows=0)
    need = int(hip.lib().lib.rv_sample_token_wide_workspace_floats(n, V))
    assert need > 0
    gws = Guarded(1, need, F32, dev, name="workspace", guard_rows=0)
    so = si = None
    if seens is not None:
        if not isinstance(seens[0], (list, tuple)):
            seens = [seens] * n
        si = torch.tensor([i for s in seens for i in s], dtype=I32, device=dev)
        so = torch.tensor(np.concatenate([[0], np.cumsum([len(s) for s in seens])]), dtype=I32, device=dev)
    call("rv_sample_token_wide", gl.view, gl.ld, n, V, so, si, float(penalty), float(temperature), float(top_p), gu.view, gt.view,
         gp.view, gws.view, need)
    gl.check(), gu.check(), gws.check()
    gt.check(written=True), gp.check(written=True)
    return gt.view[0].cpu().numpy().astype(np.int64), gp.view[0].cpu().double().numpy(), gp.bits()[0].cpu().numpy()


def check_against_restatement(row, V, us, tok, logp, temperature, top_p, seen, penalty, max_undecidable=0.0, planted_from=2):
    """every decidable token is the restatement's, every token is in the kept set, logp inside the fp32 evaluation bound"""
    bound = V * U32
    p, edge = GC.sampler_probs64(row, temperature, top_p, seen, penalty)
    assert edge > 4 * bound, f"the nucleus edge is {edge:.3e} from a tie (4 x bound = {4 * bound:.3e}): pick another row"
    if temperature == 0.0:
        want = np.full(len(us), int(np.argmax(GC.penalised(row, seen, penalty))))
        dist = np.full(len(us), np.inf)
    else:
        want, dist = GC.sampler_choice64(p, np.asarray(np.float32(us), dtype=np.float64))
    ok = dist > bound
    if max_undecidable == 0.0:
        assert ok[planted_from:].all(), "every planted interval middle is decidable by construction"
    else:
        assert 1.0 - ok.mean() <= max_undecidable, "the row leaves too many of the planted uniforms undecidable"
    assert (p[tok] > 0).all(), "a token outside the kept set was drawn"
    bad = np.nonzero(ok & (tok != want))[0]
    assert bad.size == 0, f"{bad.size} draws differ from the restatement, first u = {us[bad[0]]!r}: {tok[bad[0]]} vs {want[bad[0]]}"
    eb = logp_bound(row, p, temperature, seen, penalty)
    for t in np.unique(tok):
        err = np.abs(logp[tok == t] - np.log(p[t])).max()
        assert err <= eb(t), f"logp of token {t}: error {err:.3e} > bound {eb(t):.3e}"
    return p, want, ok


# ------------------------------------------------------------------------------------------------ tiny text model, stub tokenizer
TINY = dict(hidden=256, layers=2, heads=2, kv_heads=1, ffn=512, rope_theta=500000.0, rms_eps=1e-5, model_max_length=2048)


def tiny_text_cfg(vocab=1024):
    from rlaif_v_amd.textlm import TextLMConfig
    return TextLMConfig(vocab=vocab, **TINY)


def tiny_text_weights(vocab, seed, std=0.05, head_scale=1.0):
    """HF-named fp32 CPU tensors of the tiny Llama (values on the bf16 grid, so every consumer sees the same numbers);
    ``head_scale`` stretches the LM head so that the logits spread over several units."""
    g = torch.Generator().manual_seed(seed)
    d, f, L = TINY["hidden"], TINY["ffn"], TINY["layers"]
    kvd = d // TINY["heads"] * TINY["kv_heads"]

    def rn(*shape, s=std):
        return (torch.randn(*shape, generator=g) * s).bfloat16().float()
    W = {"model.embed_tokens.weight": rn(vocab, d, s=0.5), "model.norm.weight": (1.0 + rn(d, s=0.1)),
         "lm_head.weight": rn(vocab, d, s=std * head_scale)}
    for i in range(L):
        p = f"model.layers.{i}."
        W[p + "self_attn.q_proj.weight"], W[p + "self_attn.o_proj.weight"] = rn(d, d), rn(d, d)
        W[p + "self_attn.k_proj.weight"], W[p + "self_attn.v_proj.weight"] = rn(kvd, d), rn(kvd, d)
        W[p + "mlp.gate_proj.weight"], W[p + "mlp.up_proj.weight"], W[p + "mlp.down_proj.weight"] = rn(f, d), rn(f, d), rn(d, f)
        W[p + "input_layernorm.weight"], W[p + "post_attention_layernorm.weight"] = 1.0 + rn(d, s=0.1), 1.0 + rn(d, s=0.1)
    return W


def tiny_text_model(W, vocab, device="cuda:0"):
    from rlaif_v_amd.textlm import TextLMModel
    model = TextLMModel(tiny_text_cfg(vocab), device=device)
    model.load_state_dict(W)
    return model


class StubTokenizer:
    """What rlaif_v_amd.divide asks of a tokenizer, over a vocabulary of ``vocab`` ids: 0 pad, 1 bos, 2 eos, 3 <|eot_id|>, 4 / 5 the
    role headers.  Like Llama-3's, the chat template writes the BOS into the text AND __call__ prepends one: two BOS ids."""
    bos_token_id, eos_token_id, eot_id = 1, 2, 3
    pad_token_id = None

    def __init__(self, vocab=1024):
        self.vocab = vocab
        self.templated = []

    def apply_chat_template(self, messages, tokenize=False, add_generation_prompt=True):
        assert tokenize is False and add_generation_prompt is True
        text = "<bos>" + "".join(f" <{m['role']}> {m['content']} <eot>" for m in messages) + " <assistant>"
        self.templated.append(text)
        return text

    def convert_tokens_to_ids(self, token):
        return {"<|eot_id|>": self.eot_id}[token]

    def __call__(self, text):
        import zlib
        special = {"<bos>": 1, "<eot>": 3, "<user>": 4, "<assistant>": 5}
        ids = [self.bos_token_id]
        for w in text.replace("<bos>", "<bos> ").split():
            ids.append(special[w] if w in special else 8 + zlib.crc32(w.encode()) % (self.vocab - 8))
        return {"input_ids": ids}

    def decode(self, ids, skip_special_tokens=True):
        assert skip_special_tokens is True
        out = []
        for i in ids:
            i = int(i)
            if i < 8:
                continue
            out.append("\n-" if i % 5 == 0 else f"w{i}")
        return "### Facts:\n- " + " ".join(out)
