"""``DecodePool``: continuous batching on one ``row_params`` decode session (decode.py) -- requests are admitted into free rows of
a RUNNING batch and their rows are released when they finish, instead of a fixed set of rows per call (``generate_ragged``).

Why: a decoded event costs the same ~210 launches for 1 row as for 64, and two sessions do not overlap on this runtime (DESIGN 7.5,
7.6), so a serving caller's throughput is the number of USEFUL rows per event step.  ``generate_ragged`` parks a row that has
reached its ``max_len`` until the longest row of the call finishes -- ``sum_b (L_max - L_b)`` parked row-events per call -- and a
request that arrives one event after a call began waits for the whole call.  Here it waits for a free row.

The pool is a single-threaded object that the caller drives:

    with model.decode_pool(rows=64, capacity=1025, generator=g) as pool:
        a = pool.submit(prompt_a, max_len=300, temp=0.9)
        b = pool.submit(prompt_b, max_len=1024, top_k=1, disable_channels=[9])
        while pool.pending():
            for rid, event, done in pool.step():   # one event per occupied row
                ...                                 # (submit() more whenever they arrive)
        out_a = pool.result(a)

One ``step()``: queued requests are admitted into free rows, lowest row first, FIFO, as many as fit, with ONE packed prefill for the
group (DecodeSession.admit); one event is sampled for every row (``sample_event(live=occupied)``: the break rule runs over the
occupied rows, free rows are sampled and dropped); a request that sampled EOS (its last event, as in ``generate``) or holds
``max_len`` events is done and its row is released; if any request continues, the next event's noise and the net step follow, in
``generate_ragged``'s order.  Device work per step is that of a ``generate_ragged`` step; an admission adds its prefill and about a
dozen tiny copies, a release two.  No graph is recaptured: the session's graphs read every per-row value from device
memory.

A SEED PER REQUEST (``model.decode_pool(rows, capacity, seeded=True)``, ``submit(..., seed=s)``, s an int in [0, 2^64)).  An
unseeded pool's rows share the ``[8, B, V]`` noise of an event, so a sampled request's draws depend on its row and on the step it
runs at: that pool is reproducible for the same generator seed AND the same submit / step schedule.  A seeded pool runs on a
``seeded`` session (decode.py): no noise buffer, no noise graph, no generator; the sampler computes the variate of (request seed,
index of the event in the request's result, token position, rank) with a counter-based generator (Philox4x32-10,
``mh_sample_top_p_k_seeded``).  A request's ids are then a function of the weights, its prompt, its sampling settings, its seed
and the SHAPES of the launches it runs in -- not of its row, the step it was admitted at, its neighbours, or what its row held
before.  The stated limits of that promise:
  * a request's prefill depends on its admission group through the packed forward's own shape dispatch (DecodeSession.admit);
  * its decode steps depend on the session's row count through the projection kernels' dispatch;
  * so the promise holds at equal launch shapes: the same pool size, and the same admission grouping or admitted alone.  At equal
    shapes the kernels are bit-equal per row; nothing wider is claimed.
Every request of a seeded pool needs a seed, an unseeded pool refuses one, and ``generator`` with ``seeded=True`` is refused.  Free
and parked rows keep being sampled and dropped; their seeds are whatever the row last held.  Measured: DESIGN 7.8.

Out of scope:
  * a background thread or server loop -- the caller owns the loop (and the thread: one pool, one thread);
  * ``share_prompt`` inside the pool;
  * chunking a long admission: a 4096-event prefill on tv2o-medium is 4096 x 0.4 GFLOP of projections (12 layers x 16.8 M
    weights x 2) plus ~0.8 TFLOP of causal attention, about 2.5 TFLOP -- 2.5 to 5 ms at the 500 to 1000 TFLOP/s the block
    forward runs at, i.e. about one or two decoded events -- arithmetic, not a measurement;
  * ``generate``, ``generate_stream``, ``generate_ragged`` and their sessions: they run what they ran.

Measured (one MI355X, ``profiles/pool_ab.txt``): ``tools/bench_pool.py`` -- tv2o-medium bf16, 256 requests arriving
together, prompts of 16 to 512 events, 32 to 512 events to generate, 64 rows -- gives 28.1 k useful events/s for one pool against
22.3 k for ``generate_ragged`` over consecutive groups of 64, 1.26 x, and the last request's first event after 1.8 s instead of
2.35 s.  The static form's parked row-events predict 1.86 x for a pool that is never short of requests; this finite list drains
(1382 event steps where 1088 would be full, against the groups' 2022: 1.46 x in steps), and an admission costs 1.9 ms of host launch
time (the packed forward's ~100 launches for one short prompt), about 1.35 decode steps, 177 times.  ``bench.py --mode generate``
at 64 x 1024, this commit against its parent alternating on one box: 41.4 k against 41.2 k events/s, inside the parent's own
2.3 % spread -- the plain path runs no new code.
"""
from __future__ import annotations

from collections import deque
from typing import Dict, List, Optional, Tuple

import numpy as np
import torch


class _Request:
    __slots__ = ("prompt", "max_len", "rp", "events", "row", "done")  # (rp["seed"]: a seeded pool's request)

    def __init__(self, prompt: np.ndarray, rp: dict):
        self.prompt, self.rp, self.max_len = prompt, rp, rp["max_len"][0]
        self.events: List[np.ndarray] = []
        self.row: Optional[int] = None
        self.done = False


class DecodePool:
    """see the module docstring; made by ``MIDIModel.decode_pool(rows, capacity, generator, seeded)``"""

    def __init__(self, model, rows: int, capacity: int, generator=None, seeded: bool = False):
        if int(rows) != rows or rows < 1 or int(capacity) != capacity or capacity < 2:
            raise ValueError(f"decode_pool: {rows} rows of capacity {capacity}")
        if seeded and generator is not None:
            raise ValueError("decode_pool: seeded=True together with a generator -- a seeded pool draws nothing from a generator")
        self.model, self.rows, self.capacity, self.generator = model, int(rows), int(capacity), generator
        self.seeded = bool(seeded)
        self.ses = None                                  # taken from the model's pool at the first admission
        self.free: List[int] = list(range(self.rows))    # ascending: the lowest free row is taken first
        self.queue: deque = deque()                      # request ids, FIFO
        self.occupied: Dict[int, int] = {}               # row -> request id
        self.requests: Dict[int, _Request] = {}
        self._next_id = 0
        self._closed = False

    # ---- the caller's side ----------------------------------------------------------------------------------------------
    def submit(self, prompt, max_len=512, temp=1.0, top_p=0.98, top_k=20, ban_eos=False, disable_patch_change=False,
               disable_control_change=False, disable_channels=None, seed=None) -> int:
        """queue one request; -> its id.  Checked as ``generate_ragged`` checks a row with values of its own (the same code, the
        same ``ValueError``s), plus ``max_len + 1 > capacity``; the prompt is cropped to its last 4096 events, as the stream forms
        crop.  ``seed``: required in a seeded pool (an int in [0, 2^64)), refused in an unseeded one.  Nothing is launched here."""
        if self._closed:
            raise ValueError("DecodePool.submit: the pool is closed")
        if self.seeded and seed is None:
            raise ValueError("DecodePool.submit: every request of a seeded pool needs a seed (an integer in [0, 2^64))")
        if not self.seeded and seed is not None:
            raise ValueError("DecodePool.submit: this pool shares one noise stream among its rows; a seed per request needs "
                             "decode_pool(..., seeded=True)")
        p, rp = self.model._check_request(prompt, max_len, temp, top_p, top_k, ban_eos, disable_patch_change,
                                          disable_control_change, disable_channels, seed=seed)
        if rp["max_len"][0] + 1 > self.capacity:
            raise ValueError(f"DecodePool.submit: max_len {rp['max_len'][0]} in a pool of capacity {self.capacity} (max_len + 1 "
                             f"rows are needed)")
        rid = self._next_id
        self._next_id += 1
        self.requests[rid] = _Request(p, rp)
        self.queue.append(rid)
        return rid

    def pending(self) -> int:
        """requests queued or running"""
        return len(self.queue) + len(self.occupied)

    def result(self, rid: int, forget: bool = False) -> np.ndarray:
        """request ``rid``'s events so far, ``(<= max_len, 8) int64`` with its (cropped, padded) prompt in front; ``forget``: drop a
        finished request from the pool's books"""
        r = self.requests[rid]
        out = np.concatenate([r.prompt] + [e[None] for e in r.events], axis=0)
        if forget and r.done:
            del self.requests[rid]
        return out

    def results(self) -> Dict[int, np.ndarray]:
        """{id: result(id)} of every finished request the pool still knows"""
        return {rid: self.result(rid) for rid, r in self.requests.items() if r.done}

    def close(self) -> None:
        """hand the advanced random stream back to the generator and the session back to the model's pool; requests still queued
        or running stay as far as they got"""
        if self._closed:
            return
        self._closed = True
        if self.ses is not None:
            ses, self.ses = self.ses, None
            ses.end()
            self.model._return_session(ses)

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()
        return False

    # ---- one event step ---------------------------------------------------------------------------------------------------
    def _session(self):
        if self.ses is None:
            # (1.0, 0.98, 1 fill a NEW session's buffers through its warm-up pass; every admission overwrites its rows')
            ses = self.model._checkout_session(self.rows, self.capacity, 1.0, 0.98, 1, ragged=True, row_params=True,
                                                seeded=self.seeded)
            ses.reset()                      # every row free: pos = pos_limit = 0
            ses.begin(self.generator)
            self.ses = ses
        return self.ses

    def _admit_queued(self) -> None:
        k = min(len(self.free), len(self.queue))
        if k == 0:
            return
        rows, rids = self.free[:k], [self.queue.popleft() for _ in range(k)]
        reqs = [self.requests[rid] for rid in rids]
        del self.free[:k]
        rp = {name: [r.rp[name][0] for r in reqs] for name in reqs[0].rp}
        first, ban = self.model._mask_rows(rp)
        tokens = torch.from_numpy(np.concatenate([r.prompt for r in reqs], axis=0))
        self._session().admit(rows, tokens, [len(r.prompt) for r in reqs], rp["max_len"], rp["temp"], rp["top_p"], rp["top_k"],
                              first, ban, seeds=rp.get("seed"))
        for row, rid, r in zip(rows, rids, reqs):
            r.row = row
            self.occupied[row] = rid

    def step(self) -> List[Tuple[int, np.ndarray, bool]]:
        """admit what fits, sample one event for every row, -> [(request id, event np.int64 (8,), done)] for the occupied rows,
        by request id.  With nothing occupied and nothing queued: ``[]``, and nothing is launched."""
        from .model import _SPECULATIVE_NET
        if self._closed:
            raise ValueError("DecodePool.step: the pool is closed")
        if not self.queue and not self.occupied:
            return []
        eos = self.model.tokenizer.eos_id
        with torch.inference_mode():
            self._admit_queued()
            ses = self.ses
            live = [row in self.occupied for row in range(self.rows)]
            running = [self.requests[rid] for rid in self.occupied.values()]
            more = any(len(r.prompt) + len(r.events) + 1 < r.max_len for r in running)
            speculative = more and ses.g_steps is not None and _SPECULATIVE_NET
            event, _ = ses.sample_event(then_net=speculative, live=live)
            out, finished = [], []
            for row, rid in sorted(self.occupied.items(), key=lambda kv: kv[1]):
                r = self.requests[rid]
                ev = event[row].copy()
                r.events.append(ev)
                r.done = bool(ev[0] == eos) or len(r.prompt) + len(r.events) >= r.max_len
                if r.done:
                    finished.append(row)
                out.append((rid, ev, r.done))
            if len(finished) < len(out):  # a request continues: the next event's draws, under the net step over this event
                ses.draw_noise()
                if not speculative:
                    ses.net_step()
            if finished:  # (behind the net step, which advanced these rows with the rest)
                ses.release(finished)
                for row in finished:
                    self.requests[self.occupied.pop(row)].row = None
                self.free = sorted(self.free + finished)
        return out
