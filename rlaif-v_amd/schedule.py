"""Host side of continuous batching (LlavaDPOModel.generate_continuous): the cache layout, the slot scheduler, the uniforms
and the host step counts.  Pure Python / CPU torch: nothing here touches a GPU, so the scheduler's claims are tests
(tests/test_continuous_host.py).

``generate()`` decodes a fixed set of rows until the longest of them ends.  Here the decode step has ``slots`` rows, each at a
step of its own (rv_decode_advance); a request - one prompt and its ``repeat`` samples - is admitted whole when ``repeat``
slots and one prompt region are free, and a slot found finished at a poll goes back to the free list at once."""
from __future__ import annotations

import heapq
import math
from dataclasses import dataclass
from typing import Dict, List, Optional, Sequence, Tuple

import numpy as np
import torch


# ------------------------------------------------------------------------------------------------ cache rows
@dataclass
class SlotRows:
    """Cache rows of ``generate_continuous``, the counterpart of ``splice.DecodeRows``: every layer's cache is one
    [n_rows][2 kv_dim] buffer of ``regions`` prompt regions of ``max_prompt_tokens`` rows followed by ``slots`` slot regions of
    ``max_new`` rows.  A prompt's K | V is stored once in its region and named by all its samples' spans; the region is free
    again when the last of them has finished.  Slot s owns rows [own_off(s), own_off(s) + max_new) for good."""
    regions: int
    max_prompt_tokens: int
    slots: int
    max_new: int
    max_rows: int = 64

    def __post_init__(self):
        if min(self.regions, self.max_prompt_tokens, self.slots, self.max_new, self.max_rows) < 1:
            raise ValueError("SlotRows: regions, max_prompt_tokens, slots, max_new and max_rows must be >= 1")
        if self.n_rows > 2 ** 31 - 1:
            raise ValueError("SlotRows: the cache rows do not fit int32")

    @property
    def own_base(self) -> int:
        return self.regions * self.max_prompt_tokens

    @property
    def n_rows(self) -> int:
        return self.own_base + self.slots * self.max_new

    @property
    def own_off(self) -> torch.Tensor:
        return self.own_base + torch.arange(self.slots, dtype=torch.int32) * self.max_new

    def region_off(self, region: int) -> int:
        if not 0 <= region < self.regions:
            raise ValueError(f"SlotRows: region {region} outside [0, {self.regions})")
        return region * self.max_prompt_tokens

    @property
    def chunks(self) -> List[Tuple[int, int]]:
        """[c0, c1) slot ranges of at most ``max_rows`` rows: one launch set per chunk and step."""
        return [(c, min(c + self.max_rows, self.slots)) for c in range(0, self.slots, self.max_rows)]

    def prefill_rows(self, regions: Sequence[int], lens: Sequence[int]) -> torch.Tensor:
        """int32 [sum(lens)]: the cache row of every token of a pad-free prefill of prompts of ``lens`` tokens, prompt k going
        to region ``regions[k]``."""
        if len(regions) != len(lens) or len(set(regions)) != len(regions):
            raise ValueError("SlotRows.prefill_rows: one distinct region per prompt")
        out = []
        for r, n in zip(regions, lens):
            if not 1 <= n <= self.max_prompt_tokens:
                raise ValueError(f"SlotRows.prefill_rows: a prompt of {n} tokens does not fit a region of {self.max_prompt_tokens}")
            out.append(self.region_off(r) + torch.arange(n, dtype=torch.int32))
        return torch.cat(out)


# ------------------------------------------------------------------------------------------------ the scheduler
class SlotScheduler:
    """Which slots and prompt regions are free, which request holds which, and when to look at the device's done flags.

    ``room()`` requests can be admitted now; ``admit(request, budget)`` takes ``repeat`` slots (the lowest free ones) and one
    region; ``steps_to_poll()`` decode steps may run before the done flags must be read - ``poll_every``, or fewer when every
    live slot's budget ends sooner (budgets are known on the host, EOS is not); ``step()`` counts one executed decode step;
    ``poll(done)`` frees what the flags show finished.  ``steps_executed`` is the number of decode steps - passes over the
    weights - the schedule cost."""

    def __init__(self, slots: int, repeat: int = 1, regions: Optional[int] = None, poll_every: int = 8):
        if slots < 1 or repeat < 1 or poll_every < 1:
            raise ValueError("SlotScheduler: slots, repeat and poll_every must be >= 1")
        if repeat > slots:
            raise ValueError(f"SlotScheduler: repeat {repeat} > slots {slots}: a request is admitted whole")
        # A region outlives its request's shortest samples, so more requests are live than slots // repeat: with only that many
        # regions a request could start only when a whole earlier one has ended, which is the static scheme again (2,320 - 2,720
        # steps instead of 1,312 - 1,472 on the 60 x 10 workload of tests/test_continuous_host.py; 3 x saturates it).  A live
        # request holds at least one slot, so ``slots`` regions are always enough.
        regions = min(slots, 3 * (slots // repeat)) if regions is None else int(regions)
        if regions < 1:
            raise ValueError("SlotScheduler: regions must be >= 1")
        self.slots, self.repeat, self.regions, self.poll_every = int(slots), int(repeat), regions, int(poll_every)
        self.free_slots = list(range(self.slots))
        self.free_regions = list(range(regions))
        self.owner: List[Optional[Tuple[int, int]]] = [None] * self.slots       # slot -> (request, sample)
        self.left: List[int] = [0] * self.slots       # decode steps until the slot's budget is used up (host upper bound)
        self.live: Dict[int, dict] = {}               # request -> dict(region=, slots=, open=)
        self.steps_executed = 0
        self.polls = 0
        self.history: List[Tuple[int, int, List[int]]] = []       # (request, region, slots) of every admission, in order

    def room(self) -> int:
        return min(len(self.free_slots) // self.repeat, len(self.free_regions))

    def admit(self, request: int, budget) -> Tuple[int, List[int]]:
        """``budget``: the most tokens a sample of the request may have - one int, or ``repeat`` ints, one per sample."""
        if self.room() < 1:
            raise RuntimeError("SlotScheduler.admit: no room")
        if request in self.live:
            raise ValueError(f"SlotScheduler.admit: request {request} is live")
        budgets = [int(b) for b in budget] if hasattr(budget, "__len__") else [int(budget)] * self.repeat
        if len(budgets) != self.repeat or min(budgets) < 1:
            raise ValueError("SlotScheduler.admit: one budget >= 1, or one per sample")
        region = heapq.heappop(self.free_regions)
        slots = [heapq.heappop(self.free_slots) for _ in range(self.repeat)]
        for r, s in enumerate(slots):
            self.owner[s] = (request, r)
            self.left[s] = budgets[r] - 1             # the first token comes from the prefill
        self.live[request] = dict(region=region, slots=slots, open=self.repeat)
        self.history.append((request, region, list(slots)))
        return region, slots

    def chunk_live(self, c0: int, c1: int) -> bool:
        return any(o is not None for o in self.owner[c0:c1])

    def steps_to_poll(self) -> int:
        left = [self.left[s] for s in range(self.slots) if self.owner[s] is not None]
        return min(self.poll_every, max(left)) if left else 0

    def step(self) -> None:
        self.steps_executed += 1
        for s in range(self.slots):
            if self.left[s] > 0:
                self.left[s] -= 1

    def poll(self, done: Sequence[int]) -> Tuple[List[Tuple[int, int, int]], List[int]]:
        """``done``: the device's flag per slot.  Returns (finished (slot, request, sample) triples, requests now complete).
        The finished slots and the complete requests' regions are free on return."""
        self.polls += 1
        finished, complete = [], []
        for s in range(self.slots):
            if self.owner[s] is None:
                continue
            if not done[s]:
                if self.left[s] == 0:
                    raise RuntimeError(f"slot {s} has used its budget and is not flagged done: the device state is inconsistent")
                continue
            request, sample = self.owner[s]
            finished.append((s, request, sample))
            self.owner[s] = None
            self.left[s] = 0
            heapq.heappush(self.free_slots, s)
            rec = self.live[request]
            rec["open"] -= 1
            if rec["open"] == 0:
                heapq.heappush(self.free_regions, rec["region"])
                del self.live[request]
                complete.append(request)
        return finished, complete


# ------------------------------------------------------------------------------------------------ host step counts
def length_table(n: int, seed: int, median: float = 90.0, sigma: float = 0.6, lo: int = 1, hi: int = 512) -> List[int]:
    """``n`` answer lengths drawn log-normal (median, sigma), rounded and clipped to [lo, hi]: an ASSUMED distribution - nobody
    has measured RLAIF-V's answer lengths in this project."""
    z = torch.randn(n, generator=torch.Generator().manual_seed(int(seed)), dtype=torch.float64)
    return torch.clamp(torch.round(torch.exp(math.log(median) + sigma * z)), lo, hi).long().tolist()


def static_decode_steps(lengths: Sequence[Sequence[int]], prompts_per_call: int, max_new: int, poll_every: int = 8) -> int:
    """Decode steps of ``generate()`` called on ``prompts_per_call`` requests at a time: a call runs until its longest sequence
    has ended AND the flags are read (every ``poll_every`` sampler rounds), or ``max_new`` rounds; its first round is the
    prefill's, the others are decode steps.  ``lengths[i]``: the sample lengths of request i."""
    total = 0
    for i0 in range(0, len(lengths), prompts_per_call):
        longest = max(max(ls) for ls in lengths[i0:i0 + prompts_per_call])
        rounds = min(int(max_new), -(-longest // poll_every) * poll_every)
        total += rounds - 1
    return total


def simulate(lengths: Sequence[Sequence[int]], slots: int, repeat: int, regions: Optional[int] = None, poll_every: int = 8,
             trace: Optional[list] = None, known: bool = False) -> SlotScheduler:
    """Runs ``SlotScheduler`` over requests 0 .. n - 1 in order with the given sample lengths (the loop of
    generate_continuous with the device replaced by a counter) and returns it.  The scheduler does not know a length: it
    sees a budget of max(lengths) and the done flags at its polls, as with sequences that end on EOS.  ``trace`` receives a
    (steps_executed, owner list, {live request: region}) snapshot after every admission round.  ``known``: the lengths are
    given to the scheduler as per-sample budgets (sequences that end on their budget, as with a model that never emits EOS)."""
    sched = SlotScheduler(slots, repeat, regions, poll_every)
    budget = max(max(ls) for ls in lengths)
    age = [0] * slots              # tokens the slot's sequence has
    want = [0] * slots
    nxt, n = 0, len(lengths)
    while True:
        while nxt < n and sched.room() > 0:
            _, ss = sched.admit(nxt, [int(x) for x in lengths[nxt]] if known else budget)
            for r, s in enumerate(ss):
                age[s], want[s] = 1, int(lengths[nxt][r])
            nxt += 1
        if trace is not None:
            trace.append((sched.steps_executed, list(sched.owner), {q: rec["region"] for q, rec in sched.live.items()}))
        if not sched.live:
            if nxt >= n:
                return sched
            continue
        for _ in range(sched.steps_to_poll()):
            sched.step()
            for s in range(slots):
                if sched.owner[s] is not None and age[s] < want[s]:
                    age[s] += 1
        sched.poll([sched.owner[s] is None or age[s] >= want[s] for s in range(slots)])


# ------------------------------------------------------------------------------------------------ uniforms
_M64 = (1 << 64) - 1


def _mix64(z: np.ndarray) -> np.ndarray:
    """splitmix64's finaliser on uint64 arrays (wrapping arithmetic)."""
    z = (z ^ (z >> np.uint64(30))) * np.uint64(0xBF58476D1CE4E5B9)
    z = (z ^ (z >> np.uint64(27))) * np.uint64(0x94D049BB133111EB)
    return z ^ (z >> np.uint64(31))


def uniform_table(seed: int, index: int, max_new: int, repeat: int) -> torch.Tensor:
    """fp32 [max_new, repeat]: the uniform of step t of sample r of request ``index`` under ``seed`` - a function of these four
    integers alone (no generator is consumed, no other request matters):

        k = mix64(mix64(mix64(seed mod 2^64 + G) ^ index) ^ r) + t G  (mod 2^64),    u = (mix64(k) >> 40) * 2^-24

    mix64 = splitmix64's finaliser, G = 0x9E3779B97F4A7C15.  u is a multiple of 2^-24 in [0, 1), exact in fp32."""
    g = np.uint64(0x9E3779B97F4A7C15)
    with np.errstate(over="ignore"):
        base = _mix64(np.array([(int(seed) & _M64)], dtype=np.uint64) + g)
        base = _mix64(base ^ np.uint64(int(index) & _M64))
        per_r = _mix64(base[None, :] ^ np.arange(repeat, dtype=np.uint64)[None, :])                      # [1, repeat]
        k = per_r + np.arange(max_new, dtype=np.uint64)[:, None] * g                                    # [max_new, repeat]
        bits = _mix64(k) >> np.uint64(40)
    return torch.from_numpy((bits.astype(np.float64) * 2.0 ** -24).astype(np.float32))
