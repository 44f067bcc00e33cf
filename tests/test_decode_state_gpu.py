"""rv_decode_advance / rv_decode_admit (csrc/decode_state.hip) through the C ABI against a Python restatement: 40 steps of random
tokens over S slots of T = 16 columns, budgets 1..16, two EOS ids, slots admitted at different steps and admitted again after
they have finished.  Every operand is a tests/guarded.py window (tables with ld_t > T), so after every launch all state arrays,
output arrays and tables must equal the restatement's - which writes the contract's cells only - and at the end no guard
may have changed.  Every emitted cache row stays inside its slot's region, for parked slots too."""
import os
import sys

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import guarded as G  # noqa: E402

T, STEPS, VOCAB, EOS = 16, 40, 24, (3, 11)
INT_STATE = ("len", "budget", "done", "pre_off", "pre_len", "own_off")
INT_OUT = ("tok_in", "pos", "dst", "pre_len_eff", "own_len")


class Restated:
    """The contract of include/rlaifv_hip.h in numpy, one slot at a time."""

    def __init__(self, S, own_off, u_table, fill):
        self.S = S
        z = lambda: np.zeros(S, dtype=np.int64)                                       # noqa: E731
        self.len, self.budget, self.pre_off, self.pre_len = z(), z(), z(), z()
        self.done = np.ones(S, dtype=np.int64)
        self.own_off = np.asarray(own_off, dtype=np.int64)
        self.out_tokens, self.seen_ids = fill["out_tokens"].copy(), fill["seen_ids"].copy()
        self.u_table = u_table
        self.tok_in, self.pos, self.dst, self.pre_len_eff, self.own_len = (fill[k].copy() for k in INT_OUT)
        self.u_next = fill["u_next"].copy()
        self.ended = {"eos": 0, "budget": 0}

    def advance(self, s, tok):
        if not self.done[s]:
            n = self.len[s]
            self.out_tokens[s, n] = self.seen_ids[s, n] = tok
            self.len[s] = n + 1
            if tok in EOS or n + 1 == self.budget[s]:
                self.done[s] = 1
                self.ended["eos" if tok in EOS else "budget"] += 1
        if not self.done[s]:
            n = self.len[s]
            self.tok_in[s], self.pos[s], self.dst[s] = tok, self.pre_len[s] + n - 1, self.own_off[s] + n - 1
            self.pre_len_eff[s], self.own_len[s], self.u_next[s] = self.pre_len[s], n, self.u_table[s, n]
        else:
            self.tok_in[s], self.pos[s], self.dst[s] = 0, 0, self.own_off[s]
            self.pre_len_eff[s], self.own_len[s], self.u_next[s] = 0, 1, np.float32(0.5)

    def admit(self, s, pre_off, pre_len, budget, tok):
        self.seen_ids[s, :] = -1
        self.len[s], self.done[s], self.pre_off[s], self.pre_len[s], self.budget[s] = 0, 0, pre_off, pre_len, budget
        self.advance(s, tok)


def scenario(S, rng, ref):
    """The run as events the caller applies to ``ref`` (and to the device) before asking for the next one:
    ("admit", step, slots, pre_off, pre_len, budget, token) with at most 64 slots, or ("advance", step, token).  No slot is
    admitted in the last T steps, so every sequence has ended when the run has."""
    for step in range(STEPS):
        free = np.nonzero(ref.done)[0]
        want = free[rng.random(free.size) < (0.9 if step == 0 else 0.35)] if step < STEPS - T else free[:0]
        if step == 3:                                      # everything that is free at once: more than 64 slots in one go at S = 200
            want = free
        want = rng.permutation(want)
        for c in range(0, want.size, 64):
            part = want[c:c + 64]
            n = part.size
            yield ("admit", step, part, rng.integers(0, 4000, n), rng.integers(0, 700, n), rng.integers(1, T + 1, n),
                   rng.integers(0, VOCAB, n))
        yield ("advance", step, rng.integers(0, VOCAB, S))


def make_case(S):
    rng = np.random.default_rng(100 + S)
    own_off = 5000 + np.arange(S) * T
    fill = {k: rng.integers(-9, 9, S) for k in INT_OUT}                               # the outputs start as junk: all are rewritten
    fill["u_next"] = rng.random(S).astype(np.float32)
    fill["out_tokens"] = rng.integers(100, 200, (S, T))
    fill["seen_ids"] = rng.integers(100, 200, (S, T))
    u_table = rng.random((S, T)).astype(np.float32)
    return rng, own_off, fill, u_table, Restated(S, own_off, u_table, fill)


def apply_to_restatement(ref, ev):
    if ev[0] == "admit":
        _, _, part, p_off, p_len, budget, tok = ev
        for i, s in enumerate(part):
            ref.admit(s, p_off[i], p_len[i], budget[i], tok[i])
    else:
        for s in range(ref.S):
            ref.advance(s, ev[2][s])


@pytest.mark.parametrize("S", [1, 64, 200])
def test_admit_and_advance_equal_the_restatement_and_stay_in_their_cells(S):
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    from rlaif_v_amd import hip
    dev = torch.device("cuda:0")
    rng, own_off, fill, u_table, ref = make_case(S)

    ops, checks = {}, []

    def operand(name, value, dtype, role, two_d=False):
        if two_d:
            g = G.Guarded(S, T, dtype, dev, fill=torch.as_tensor(value), name=name, role=role)
        else:
            g = G.guarded_1d_obj(S, dtype, dev, fill=torch.as_tensor(value), name=name, role=role)
        ops[name] = g.view if two_d else g.flat
        checks.append(g.check)

    for name in INT_STATE:
        operand(name, getattr(ref, name), torch.int32, "in" if name == "own_off" else "io")
    for name in INT_OUT:
        operand(name, fill[name], torch.int32, "io")
    operand("u_next", fill["u_next"], torch.float32, "io")
    operand("out_tokens", fill["out_tokens"], torch.int32, "io", two_d=True)
    operand("seen_ids", fill["seen_ids"], torch.int32, "io", two_d=True)
    operand("u_table", u_table, torch.float32, "in", two_d=True)
    ld_t = ops["out_tokens"].stride(0)
    assert ld_t > T and ops["seen_ids"].stride(0) == ld_t and ops["u_table"].stride(0) == ld_t
    eos = torch.tensor(EOS, dtype=torch.int32)
    tail = lambda: (ops["len"], ops["budget"], ops["done"], ops["pre_off"], ops["pre_len"], ops["own_off"], eos, len(EOS),    # noqa: E731
                    ops["out_tokens"], ops["seen_ids"], ops["u_table"], ld_t, S, T, ops["tok_in"], ops["pos"], ops["dst"],
                    ops["pre_len_eff"], ops["own_len"], ops["u_next"])

    def compare(what):
        for name in INT_STATE + INT_OUT + ("out_tokens", "seen_ids"):
            got = ops[name].cpu().numpy().astype(np.int64)
            assert np.array_equal(got, getattr(ref, name)), f"{what}: {name}"
        assert np.array_equal(ops["u_next"].cpu().numpy(), ref.u_next), f"{what}: u_next"
        dst, budget = ops["dst"].cpu().numpy(), np.maximum(ref.budget, 1)
        inside = (dst >= own_off) & (dst < own_off + budget)
        assert np.all(inside[emitted]), f"{what}: a cache row outside its slot's region"

    admissions = np.zeros(S, dtype=np.int64)
    emitted = np.zeros(S, dtype=bool)          # slots a launch has emitted a cache row for (before that, dst holds the junk fill)
    for ev in scenario(S, rng, ref):
        if ev[0] == "admit":
            _, step, part, p_off, p_len, budget, tok = ev
            host = [torch.as_tensor(v, dtype=torch.int32).contiguous() for v in (part, p_off, p_len, budget)]
            hip.call("rv_decode_admit", *host, part.size, torch.as_tensor(tok, dtype=torch.int32).to(dev), *tail())
            admissions[part] += 1
            emitted[part] = True
        else:
            emitted[:] = True
            hip.call("rv_decode_advance", torch.as_tensor(ev[2], dtype=torch.int32).to(dev), *tail())
        apply_to_restatement(ref, ev)
        compare(f"step {ev[1]}, after the {ev[0]}")
    torch.cuda.synchronize()
    for check in checks:
        check()
    assert bool(ref.done.all()), "40 steps end every sequence of at most 16 tokens"
    assert admissions.min() >= 2, "every slot was handed on after its first sequence finished"
    assert ref.ended["eos"] > 0 and ref.ended["budget"] > 0, "sequences ended on EOS and on their budget"
