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

FORKS.  A row can be DUPLICATED into free rows without a second prefill: its K/V rows [0, L) of every layer are
copied by one kernel launch (``mh_kv_fork_rows``) and its ``hidden`` row, position and a new set of per-row values are scattered as
an admission scatters them (``DecodeSession.fork``).  Three entry points share that:
  * ``submit(prompt, ..., n=k)`` -> k ids, SIBLINGS on one prompt and one set of settings (a seeded pool: k seeds).  The group is
    admitted whole -- it waits at the head of the FIFO until k rows are free -- its leader is prefilled in the admission's one packed
    forward, the other k - 1 rows are filled by one fork right behind it.  One prompt's prefill instead of k.
  * ``submit(..., hold=True)``: a request that finishes by reaching ``max_len`` KEEPS its row (``held()`` lists such requests,
    ``drop(rid)`` releases the row; they do not count in ``pending()``).  ``step()`` then runs the net step over the request's final
    event as well -- without ``hold`` it is skipped when nothing continues -- and ``DecodeSession.hold`` keeps the row's ``hidden``:
    the parked row keeps being sampled and net-stepped with the batch, which overwrites ``hidden`` and cache row ``max_len``, never
    cache rows [0, max_len).  A held request that ends on EOS is released as usual.
  * ``fork(rid, count, max_len=..., seed=...)`` -> ``count`` new requests that continue a running or held request from where it
    stands, in the lowest free rows, taken at once and ahead of the queue; their first event comes with the next ``step()``, and
    ``result()`` of a child has the inherited events in front.
In a seeded pool the variate counter is ``pos``, the index of the event in the result, and a child continues its parent's counter
under its own seed: a child given the parent's seed and settings repeats the parent, and a held request forked under its own seed
with a larger ``max_len`` gives exactly what an uninterrupted request with that ``max_len`` gives -- at equal launch shapes, the
limit stated above.  ``n == 1`` without ``hold`` runs exactly what it ran.  Measured (one MI355X, ``profiles/fork_ab.txt``, DESIGN
7.9; ``tools/bench_fork.py``, tv2o-medium bf16, 64 rows): admitting ``n=4`` siblings against four ``submit``s of the prompt, the
admitting step takes 5.58 against 10.75 ms at 4000 prompt events, 4.29 against 6.46 ms at 2048, and 3.50 against 3.32 ms at 64 (no
gain: a short admission is its launches); the copy kernel alone runs at 0.85 to 0.97 of the chip's copy rate at those lengths.

PREFIX SLOTS.  ``model.decode_pool(rows, capacity, prefix_slots=G, prefix_capacity=Pmax)`` runs on a session that keeps
G prefix slots of Pmax events beside the rows' caches, and ``submit(prompt, ..., share_prefix=True)`` stores the prompt's K/V ONCE, in
a slot: every row that continues it reads that copy, once per head and event for all of them (``mh_attn_prefix_partial_slots``), and
its own cache holds only the events behind the prompt (``mh_attn_decode_append_rows_shared``).  With ``n=k`` the k - 1 siblings JOIN
the leader's slot with no K/V copy at all -- they get the scatter of ``hidden``, position and settings; ``fork`` of a sharing request
makes children that join its slot and copy only its own events behind the prompt; ``fork`` of any other request is what it was.  A
slot is counted by the rows that name it, running and held, and is free again when the last of them leaves (``release``, ``drop``,
``close``).  A sharing group waits at the head of the queue for a free slot as a group waits for rows.  The stated limits:
  * numerics: the prefix half rounds probabilities to bf16 for its P V product, so a sharing request's ids may differ
    from the same request unshared -- bit equality with the non-sharing pool is NOT promised for sharing rows;
  * a seeded pool's promise holds for them as it stands -- "not its row, its neighbours": a sharing request's ids do not depend on how
    many rows share its slot, on which rows they sit in, or on the other slots, at equal launch shapes (per row the slot kernels are
    bit-equal to the one-prompt kernels, whatever shares a query tile: tests/test_poolshare_kernels_gpu.py);
  * cost to the others: every row of a pool with slots pays one more launch per layer and event, sharing or not (measured below);
  * an admission stores into slots or into rows: sharing leaders and other requests admitted in one ``step()`` take a packed forward
    each, so a request's admission group is the requests of its own kind admitted with it;
  * the slot caches come on top of the row caches, which are not shrunk; a prompt must fit ``prefix_capacity`` after the 4096 crop.
A pool made without ``prefix_slots`` takes the session, the graphs and the launches it took.  Measured (one MI355X,
``profiles/pool_share_ab.txt``; ``tools/bench_pool_share.py``, tv2o-medium bf16, 64 rows, a group of k siblings alone in
the pool, median decode step over 64 events): k = 8 behind 4000 events 1.455 against 1.637 ms (1.13 x), 2048: 1.412 against 1.459
(1.03 x), 512: 1.374 against 1.301 and 64: 1.351 against 1.256 -- sharing LOSES below a prompt of about a thousand events (between
the measured 512 and 2048), where a step is its launches; k = 4: 1.11 x at 4000, 1.02 x at 2048, the same crossover.  Rows that share
nothing pay 25 to 45 us a step (2 to 3 %) in a pool with slots.

FP8 K/V.  ``model.decode_pool(rows, capacity, kv_dtype="fp8")`` runs on a session whose event-level cache holds OCP e4m3
codes with one fp32 scale per (row, head, event) for K and one for V -- 136 bytes where the bf16 cache holds 256, per decoded event
and per row of capacity -- for EVERY row, prompts of their own included.  The admission's store quantizes
(``mh_kv_store_seqs_rows_fp8``), decode attention dequantizes in registers and attends to the new event's row as the cache holds it
(``mh_attn_decode_append_rows_fp8``), a fork copies codes and scales bit for bit (``mh_kv_fork_rows_fp8``).  The stated limits:
  * a request's ids may differ from the same request in a bf16-cache pool (the quantization moves the hidden state by about what the
    reference's own fp8 restatement says: DESIGN 7.11);
  * the seeded pool's promise holds as it stands: quantization is per (row, head, event), a row's keys do not depend on its row
    number, its neighbours or what the row held before, and the new row is attended to quantized -- so a child on its parent's seed
    repeats the parent and a held-then-forked request equals an uninterrupted one, at equal launch shapes and nothing wider;
  * a bf16 model and at most 256 rows (``ValueError`` at construction otherwise); not available with prefix slots, nor with
    ``generate``, ``generate_ragged`` or ``share_prompt``; the token-level cache is what it was.
A pool made without ``kv_dtype`` takes the session, the graphs and the launches it took.  Measured (one MI355X,
``profiles/pool_kvq_ab.txt``; ``tools/bench_pool_kvq.py``, tv2o-medium bf16, 64 rows all behind P events, median decode step, fp8
against bf16): P = 4000: 2.43 against 3.34 ms (1.37 x), 2048: 1.95 against 2.36 (1.21 x), 512: 1.51 against 1.56 (1.03 x), 64: 1.34
against 1.31 -- fp8 is SLOWER below a few hundred cached events (between the measured 64 and 512), where a step is its launches and
the kernel converts twice the elements per byte; the attention launch alone gains 1.78 x at 4000 events, under the 1.88 x byte ratio.
The admitting step is within 0.15 ms either way.  64 rows x 4096 events: 6.85 GB of cache against 12.88 GB.

LOG-LIKELIHOODS.  ``model.decode_pool(rows, capacity, logprobs=True)`` -- with any of the options above -- runs on a
session whose token steps call the ``_logp`` form of their sampler (``mh_sample_top_p_k_rows_logp`` /
``mh_sample_top_p_k_seeded_logp``): the same ids bit for bit, plus the MODEL's log-probability ``z_c - log sum_v exp(z_v)`` of every
token drawn, over the raw logits -- independent of temperature, top-p, top-k, the masks, the seed and the row, so values of requests
with different settings compare, and it is what the training loss sums.  ``pool.logprobs(rid)`` -> ``np.float32 [len(result(rid)) -
len(prompt)]``: ``ll`` of every event the request generated, aligned with ``result(rid)[len(prompt):]``; an event's ``ll`` is the sum
over its token positions 0..arity (the host sums them in fp32 with the grammar's arity table; EOS counts position 0 alone, the pad
positions behind an event's parameters count nothing).  A fork child's array covers its own events -- the inherited ones are its
prompt; a held request keeps its array; a row handed to a later request starts empty.  ``step()`` and ``result()`` are unchanged, and
``MIDIModel.score(x)`` gives the same quantity for given sequences.  The stated limits:
  * the values are exact on the logits the decode path produced (fp32 sums, error bound derived in tests/ref_logp.py); what bf16
    activations do to the logits themselves is the decode path's, as for the ids;
  * the seeded pool's promise extends as it stands: a request's log-likelihoods are a function of what its ids are a function of;
  * not the probability under the filtered (temperature / top-p / top-k / masked) distribution, and no top-n alternatives;
  * ``generate``, ``generate_ragged`` and ``share_prompt`` report none; ``logprobs()`` on a pool made without the option is a
    ``ValueError``.
A pool made without ``logprobs`` takes the session, the graphs and the launches it took.  Measured: DESIGN 7.12
(``tools/bench_pool_logp.py``, ``profiles/pool_logp_ab.txt``).

LORA ADAPTERS.  ``model.decode_pool(rows, capacity, lora_slots=G, lora_rank=R)`` -- with any of the options above --
runs on a session that keeps G adapter slots of rank R beside the base weights (27 MB an adapter at r = 64 for tv2o-medium, against
467 MB for a merged copy), and ``submit(..., adapter=id)`` decodes a request under the adapter ``load_adapter(src)`` returned that id
for: every row's projection is ``x W^T + s (x A^T) B^T`` with A, B, s of the row's own slot, unmerged (``mh_lora_shrink_rows`` ahead of
each of a layer's four projections, the expand inside ``mh_gemm_skinny_ext``), so requests on different adapters and on none share one
batch and one copy of the weights.  The stated limits:
  * the PROMPT is prefilled against the adapter's MERGED event-level weights (W + s B A in bf16, a second copy of those matrices
    that the session re-materialises when the adapter of an admission changes): the prompt's K/V come from the merged weights, which
    is how the reference serves an adapter (``load_merge_lora``), and the decoded events come from the unmerged form.  The two differ
    by bf16 roundings, as a merged bf16 model differs from float arithmetic on W + s B A;
  * an admission is split into one ``admit`` per adapter, in the order the adapters first appear in it, so a request's admission
    group is the requests on its own adapter admitted with it;
  * a fork child keeps its parent's adapter (its K/V were computed under it); ``unload_adapter`` is refused while a queued,
    running or held request names the adapter; adapters are never evicted on their own;
  * every row of such a pool pays the four extra launches per layer, adapted or not (DESIGN 7.13 has the numbers);
  * a bf16 model, at most 256 rows, ``G R`` a multiple of 256 (``ValueError`` at construction otherwise).
A pool made without ``lora_slots`` takes the session, the graphs and the launches it took.

LOOKAHEAD.  ``model.decode_pool(rows=R, capacity=C, seeded=True, lookahead=k)`` makes one request finish in FEWER steps: a
step costs its launches whether it carries 1 row or 64, so each of the R requests owns a GROUP of k + 1 consecutive session rows (the
session has R (k + 1) <= 256), row 0 its LEADER, rows 1..k carrying DRAFTS -- guessed events for the next k positions -- and every
``step()`` verifies the guesses of the step before.  The seeded sampler's variate is a function of (request seed, index of the event,
token position, rank), not of the row or the step, so what draft row j samples for index t + j behind a guessed prefix IS the event
the request would have sampled there if the prefix was right.  One ``step()``:
  1. ``sample_event`` over all rows: row j of a group samples s_j for event index t + j;
  2. acceptance, on the host (``DecodePool.accept``): s_0 is true; m is the largest number such that for every 1 <= i <= m the draft
     row i consumed in the previous net step equals s_(i-1) in all 8 tokens; s_0 .. s_m are reported, in order -- one request id
     may appear several times in a step's list -- and an EOS or ``max_len`` inside the run ends the request there;
  3. ``pool.proposer(history, k)`` -> up to k drafts for the next indices, ``np.ndarray [<= k, 8]``; the built-in one
     (``propose_ngram``) finds the most recent earlier occurrence of the last n events of prompt + result (n = 3, then 2; exact
     8-token equality) and proposes what followed it.  It is an attribute: assign any callable.  Drafts that could only sample
     events at or past ``max_len`` are cut off; rows without a draft sit the step out (no K/V written, nothing read);
  4. one pinned-block scatter (``DecodeSession.set_inputs``: seq[leader] = s_m, seq[leader + j] = draft j, their positions and
     cache entries), then the net step.  Lookahead pools never queue the net step ahead of the host's decision.
The K/V of a group live once, in its leader's cache sequence (``kv1`` holds R sequences, not R (k + 1)); attention is the pair
``mh_kv_append_rows_via`` + ``mh_attn_decode_rows_via``, 6 launches per layer instead of 5.  ``submit(n=)``, ``fork``, ``hold``,
``held``, ``drop`` and ``logprobs`` work, in units of groups; an accepted event's log-likelihood is read from the row that sampled it.
THE PROMISE: a request's ids and log-likelihoods do NOT depend on what the drafts were -- all right, all wrong, none, or anything
between gives the same ids -- at equal launch shapes (the same session row count), the seeded pool's own limit.  The stated limits:
  * equality with a pool made WITHOUT ``lookahead`` is NOT promised: the attention pair may order its additions differently from
    the fused ``mh_attn_decode_append_rows``, and the session row count differs;
  * ``ValueError`` at construction, before any launch: ``lookahead`` without ``seeded=True``; together with ``prefix_slots``,
    ``kv_dtype`` or ``lora_slots``; R (k + 1) > 256; k < 1;
  * a proposer must be a pure guess: whatever it returns changes the number of steps, never the result; one that returns anything
    but ``[<= k, 8]`` token ids inside the vocabulary is a ``ValueError`` in ``step()``, before the scatter;
  * what it buys on a real checkpoint is unmeasured here (no pretrained weights in the repository): DESIGN 7.14 has the mechanism's
    overhead and its ceiling, and where it loses.
Measured (one MI355X, ``profiles/pool_lookahead_ab.txt``; ``tools/bench_pool_lookahead.py``, tv2o-medium bf16, 64 prompt
events, 128 generated, median steps): one request, k = 3: a step of 1.17 ms against the plain pool's 0.99 (no drafts: the overhead,
861 against 1002 events/s) and 3390 events/s with every guess right (3.4 x; 3.97 events a step); k = 7: 1.19 ms, 6654 events/s (6.5
x); eight requests: steps 1.33 x and 1.37 x the plain pool's, ceilings 2.8 x and 5.2 x.  A plain pool of the same R (k + 1) rows
beats even the ceiling once 80 to 90 % of its rows hold requests: the option is for mostly empty pools.  The built-in proposer on
the trained toy model of the parity tests guessed 6 times in 2040 events and was never right (it lost 7 %): a toy, not a checkpoint.
A pool made without ``lookahead`` takes the session, the key, the graphs and the launches it took.

Out of scope:
  * a background thread or server loop -- the caller owns the loop (and the thread: one pool, one thread);
  * shrinking the row caches of a pool with prefix slots, or a prompt shared ACROSS pools;
  * a held row's K/V outliving its pool, or moving to another pool: ``close()`` ends every hold;
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


_SETTINGS = ("max_len", "temp", "top_p", "top_k", "ban_eos", "disable_patch_change", "disable_control_change", "disable_channels")


def propose_ngram(history: np.ndarray, k: int) -> np.ndarray:
    """the built-in proposer of a lookahead pool: ``history`` [N, 8] (prompt + result so far) -> up to k guessed next events, [<= k,
    8] int64.  The most recent EARLIER occurrence of the last n events (exact 8-token equality), n = 3 then 2; the guess is what
    followed it, as far as the history goes.  No occurrence, or a history of at most n events: no guess."""
    history = np.asarray(history)
    N = len(history)
    for n in (3, 2):
        if N <= n:
            continue
        ok = np.ones(N - n, dtype=bool)   # ok[i]: history[i : i + n] equals the last n events (i < N - n: an earlier occurrence)
        for j in range(n):
            ok &= (history[j:N - n + j] == history[N - n + j]).all(axis=1)
        hits = np.nonzero(ok)[0]
        if hits.size:
            at = int(hits[-1]) + n
            return history[at:at + k].astype(np.int64, copy=True)
    return np.zeros((0, history.shape[1] if history.ndim == 2 else 8), dtype=np.int64)


class _Request:
    # (rp["seed"]: a seeded pool's request; prompt: a child's holds its parent's result at the fork; group: the size of the sibling
    #  group this request LEADS in the queue, 0 for the siblings behind it; kw: the settings as given, a child's defaults)
    #  share: the request continues a prompt that sits in a prefix slot -- a share_prefix submit, its siblings, their fork children)
    #  logp: ll of every event the request generated itself, beside ``events`` (a pool with logprobs=True; empty otherwise)
    #  drafts: (a lookahead pool) the guessed events the request's draft rows consumed in the last net step, [<= k, 8]
    __slots__ = ("prompt", "max_len", "rp", "events", "row", "done", "hold", "held", "eos", "group", "kw", "share", "logp", "adapter",
                 "drafts")

    def __init__(self, prompt: np.ndarray, rp: dict, kw: dict, hold: bool = False, group: int = 1, share: bool = False):
        self.prompt, self.rp, self.max_len, self.kw, self.share = prompt, rp, rp["max_len"][0], kw, bool(share)
        self.events: List[np.ndarray] = []
        self.logp: List[float] = []
        self.row: Optional[int] = None
        self.done = False
        self.hold, self.held, self.eos, self.group = bool(hold), False, False, group
        self.adapter: Optional[int] = None   # the adapter id the request decodes under (a pool with lora_slots)
        self.drafts = np.zeros((0, 8), dtype=np.int64)


class DecodePool:
    """see the module docstring; made by ``MIDIModel.decode_pool(rows, capacity, generator, seeded, prefix_slots, prefix_capacity,
    kv_dtype, logprobs)``"""

    def __init__(self, model, rows: int, capacity: int, generator=None, seeded: bool = False, prefix_slots: int = 0,
                 prefix_capacity: int = 0, kv_dtype: Optional[str] = None, logprobs: bool = False, lora_slots: int = 0,
                 lora_rank: int = 64, lookahead: Optional[int] = None):
        if int(rows) != rows or rows < 1 or int(capacity) != capacity or capacity < 2:
            raise ValueError(f"decode_pool: {rows} rows of capacity {capacity}")
        if lookahead is not None:
            if isinstance(lookahead, bool) or not isinstance(lookahead, (int, np.integer)) or lookahead < 1:
                raise ValueError(f"decode_pool: lookahead={lookahead!r} -- an integer k >= 1, the draft rows of every request")
            if not seeded:
                raise ValueError("decode_pool: lookahead needs seeded=True -- exact verification rests on the seeded sampler, whose "
                                 "draws depend on the request's seed and the event's index, not on the row or the step")
            if prefix_slots or prefix_capacity or kv_dtype is not None or lora_slots:
                raise ValueError("decode_pool: lookahead is not available together with prefix_slots, kv_dtype or lora_slots")
            if rows * (int(lookahead) + 1) > 256:
                raise ValueError(f"decode_pool: {rows} requests with lookahead={lookahead} need {rows * (int(lookahead) + 1)} session "
                                 f"rows (rows x (lookahead + 1)); at most 256")
        self.lookahead = int(lookahead) if lookahead is not None else 0
        self.proposer = propose_ngram   # (a lookahead pool) history [N, 8], k -> up to k guessed next events; replaceable
        self.steps = 0                  # step() calls that launched something (tools and tests count them)
        self.drafted = self.accepted = 0   # (a lookahead pool) guesses that a draft row consumed, and those that proved right
        if kv_dtype is not None:
            if kv_dtype != "fp8":
                raise ValueError(f"decode_pool: kv_dtype={kv_dtype!r} -- None (the cache in the model's dtype) or \"fp8\"")
            if prefix_slots or prefix_capacity:
                raise ValueError("decode_pool: kv_dtype=\"fp8\" is not available together with prefix slots")
            if rows > 256 or model.dtype != torch.bfloat16:
                raise ValueError(f"decode_pool: kv_dtype=\"fp8\" needs a bf16 model and at most 256 rows: {model.dtype}, {rows} rows")
        self.kv_dtype = kv_dtype
        self.want_logprobs = bool(logprobs)
        if lora_slots:
            if any(isinstance(x, bool) or not isinstance(x, (int, np.integer)) for x in (lora_slots, lora_rank)) or lora_slots < 1 \
                    or lora_rank < 8 or lora_rank % 8 or (lora_slots * lora_rank) % 256:
                raise ValueError(f"decode_pool: lora_slots={lora_slots!r}, lora_rank={lora_rank!r} -- the rank a multiple of 8 and "
                                 f"slots x rank a multiple of 256")
            if rows > 256 or model.dtype != torch.bfloat16:
                raise ValueError(f"decode_pool: lora_slots needs a bf16 model and at most 256 rows: {model.dtype}, {rows} rows")
        self.lora_slots, self.lora_rank = int(lora_slots), int(lora_rank)
        self.adapters: Dict[int, int] = {}               # adapter id -> the session's slot
        self._next_adapter = 0
        if (prefix_slots or prefix_capacity) and not (
                all(isinstance(x, (int, np.integer)) and not isinstance(x, bool) for x in (prefix_slots, prefix_capacity))
                and prefix_slots >= 1 and prefix_capacity >= 1):
            raise ValueError(f"decode_pool: prefix_slots={prefix_slots!r}, prefix_capacity={prefix_capacity!r} -- both 0 (no prefix "
                             "slots), or at least one slot of at least one event")
        self.prefix_slots, self.prefix_capacity = int(prefix_slots), int(prefix_capacity)
        if seeded and generator is not None:
            raise ValueError("decode_pool: seeded=True together with a generator -- a seeded pool draws nothing from a generator")
        self.model, self.rows, self.capacity, self.generator = model, int(rows), int(capacity), generator
        self.seeded = bool(seeded)
        self.ses = None                                  # taken from the model's pool at the first admission
        self.free: List[int] = list(range(self.rows))    # ascending: the lowest free row is taken first
        self.queue: deque = deque()                      # request ids, FIFO
        self.occupied: Dict[int, int] = {}               # row -> request id (running)
        self.held_rows: Dict[int, int] = {}              # row -> request id (finished at max_len with hold=True: the row is kept)
        self.requests: Dict[int, _Request] = {}
        self._next_id = 0
        self._closed = False

    # ---- the caller's side ----------------------------------------------------------------------------------------------
    def submit(self, prompt, max_len=512, temp=1.0, top_p=0.98, top_k=20, ban_eos=False, disable_patch_change=False,
               disable_control_change=False, disable_channels=None, seed=None, n=1, hold=False, share_prefix=False, adapter=None):
        """queue one request; -> its id.  Checked as ``generate_ragged`` checks a row with values of its own (the same code, the
        same ``ValueError``s), plus ``max_len + 1 > capacity``; the prompt is cropped to its last 4096 events, as the stream forms
        crop.  ``seed``: required in a seeded pool (an int in [0, 2^64)), refused in an unseeded one.  Nothing is launched here.
        ``n`` > 1 (an int in [1, rows]): n SIBLINGS, continuations of the one prompt that share every setting; -> the list of their n
        ids.  In a seeded pool ``seed`` is then a sequence of n ints.  The group is admitted whole -- it waits at the head of the
        queue until n rows are free, and later requests wait behind it; its leader is prefilled in the admission's one packed
        forward, the other n - 1 rows are filled by one ``DecodeSession.fork`` right behind it: one prefill and one K/V copy per
        sibling instead of n prefills.  ``n == 1`` runs exactly what it ran, and its id is a plain int.
        ``hold``: when the request finishes by reaching ``max_len`` its row is kept (``held()``, ``fork()``, ``drop()``); one that
        ends on EOS is released as usual.
        ``share_prefix`` (a pool made with ``prefix_slots``): the prompt's K/V is stored ONCE, in a prefix slot, and every row that
        continues it reads that copy -- the request itself, its ``n - 1`` siblings, which then join the slot with no K/V copy at
        all, and their fork children.  The request waits at the head of the queue for a free slot as a group waits for rows.
        ``ValueError``, before any launch: a pool without slots; a prompt of more than ``prefix_capacity`` events (after the crop)."""
        if self._closed:
            raise ValueError("DecodePool.submit: the pool is closed")
        if adapter is not None and adapter not in self.adapters:
            raise ValueError(f"DecodePool.submit: adapter {adapter!r} is not loaded in this pool (load_adapter returns the ids: "
                             f"{sorted(self.adapters)})")
        if share_prefix and not self.prefix_slots:
            raise ValueError("DecodePool.submit: share_prefix needs a pool with prefix slots -- decode_pool(..., prefix_slots=G, "
                             "prefix_capacity=Pmax)")
        if isinstance(n, bool) or not isinstance(n, (int, np.integer)) or not 1 <= n <= self.rows:
            raise ValueError(f"DecodePool.submit: n = {n!r} is not an integer in [1, {self.rows}] (the pool's rows)")
        n = int(n)
        seeds = self._seeds(seed, n, "submit", "n")
        kw = dict(zip(_SETTINGS, (max_len, temp, top_p, top_k, ban_eos, disable_patch_change, disable_control_change,
                                  disable_channels)))
        checked = [self._checked(prompt, kw, s, "submit") for s in seeds]
        if share_prefix and len(checked[0][0]) > self.prefix_capacity:
            raise ValueError(f"DecodePool.submit: share_prefix with a prompt of {len(checked[0][0])} events in a pool whose prefix "
                             f"slots hold {self.prefix_capacity}")
        rids = []
        for i, (p, rp) in enumerate(checked):
            rids.append(self._next_id)
            self._next_id += 1
            self.requests[rids[-1]] = _Request(p, rp, kw, hold=hold, group=n if i == 0 else 0, share=share_prefix)
            self.requests[rids[-1]].adapter = adapter
            self.queue.append(rids[-1])
        return rids[0] if n == 1 else rids

    def load_adapter(self, src) -> int:
        """(a pool made with ``lora_slots``) load one LoRA adapter into a free slot; -> its id, for ``submit(adapter=id)``.  ``src``: a
        directory in peft's layout, as ``MIDIModel.load_merge_lora`` reads it (rsLoRA scaling as there), or a ``lora.LoraAdapter``.
        Stream-ordered copies into the session's fixed buffers: rows that run are untouched.  ``ValueError`` before any copy: a pool
        without slots, a rank above ``lora_rank``, a target that is no projection of a decoder layer, no free slot."""
        from .lora import adapter_layers
        if self._closed or not self.lora_slots:
            raise ValueError("DecodePool.load_adapter: " + ("the pool is closed" if self._closed else
                             "this pool has no adapter slots -- decode_pool(..., lora_slots=G, lora_rank=R)"))
        net, tok, scale, r = adapter_layers(self.model, src)
        if r > self.lora_rank or any(A.shape[0] > self.lora_rank for layers in (net, tok) for mods in layers for A, _ in mods.values()):
            raise ValueError(f"DecodePool.load_adapter: an adapter of rank {r} in slots of rank {self.lora_rank}")
        free = [g for g in range(self.lora_slots) if g not in self.adapters.values()]
        if not free:
            raise ValueError(f"DecodePool.load_adapter: all {self.lora_slots} adapter slots are taken -- unload_adapter one")
        with torch.inference_mode():
            self._session().load_adapter(free[0], net, tok, scale)
        aid = self._next_adapter
        self._next_adapter += 1
        self.adapters[aid] = free[0]
        return aid

    def unload_adapter(self, aid: int) -> None:
        """free the slot of adapter ``aid``; refused (``ValueError``) while a queued, running or held request names it"""
        if self._closed or aid not in self.adapters:
            raise ValueError(f"DecodePool.unload_adapter: no adapter {aid!r} in this pool")
        users = [rid for rid, r in self.requests.items() if r.adapter == aid and (r.row is not None or rid in self.queue)]
        if users:
            raise ValueError(f"DecodePool.unload_adapter: adapter {aid} is named by requests {users} (queued, running or held)")
        with torch.inference_mode():
            self.ses.unload_adapter(self.adapters.pop(aid))

    def _seeds(self, seed, n: int, what: str, count_name: str) -> list:
        """the seed argument of submit(n=) / fork(count=) -> n seeds (None each in an unseeded pool); one request takes a scalar,
        several take a sequence of that many (each is checked as one seed is, by _check_request)"""
        if self.seeded and seed is None:
            raise ValueError(f"DecodePool.{what}: every request of a seeded pool needs a seed (an integer in [0, 2^64))")
        if not self.seeded and seed is not None:
            raise ValueError(f"DecodePool.{what}: this pool shares one noise stream among its rows; a seed per request needs "
                             "decode_pool(..., seeded=True)")
        if seed is None or n == 1:
            return [seed] * n
        per_row = self.model._per_row(seed)
        if not per_row or len(seed) != n:
            raise ValueError(f"DecodePool.{what}: {count_name} = {n} takes a sequence of {n} seeds, one per request"
                             + (f": it holds {len(seed)}" if per_row else f", not the scalar {seed!r}"))
        return seed.tolist() if isinstance(seed, (np.ndarray, torch.Tensor)) else list(seed)

    def _checked(self, prompt, kw: dict, seed, what: str, crop=4096):
        """_check_request on the settings ``kw`` + the pool's capacity rule -> (prompt, the one-row dict)"""
        p, rp = self.model._check_request(prompt, *(kw[name] for name in _SETTINGS), crop=crop, seed=seed)
        if rp["max_len"][0] + 1 > self.capacity:
            raise ValueError(f"DecodePool.{what}: max_len {rp['max_len'][0]} in a pool of capacity {self.capacity} (max_len + 1 "
                             f"rows are needed)")
        return p, rp

    def pending(self) -> int:
        """requests queued or running (a held request is neither)"""
        return len(self.queue) + len(self.occupied)

    def held(self) -> List[int]:
        """ids of the requests that finished with ``hold=True`` and still keep their row"""
        return sorted(self.held_rows.values())

    def drop(self, rid: int) -> None:
        """release the row of held request ``rid`` (its result stays)"""
        r = self.requests.get(rid)
        if self._closed or r is None or not r.held:
            raise ValueError(f"DecodePool.drop: request {rid!r} holds no row of this pool")
        with torch.inference_mode():
            self.ses.release([r.row])
        del self.held_rows[r.row]
        self.free = sorted(self.free + [r.row])
        r.row, r.held = None, False

    def fork(self, rid: int, count: int = 1, max_len=None, temp=None, top_p=None, top_k=None, ban_eos=None,
             disable_patch_change=None, disable_control_change=None, disable_channels=None, seed=None, hold=False) -> List[int]:
        """``count`` new requests that CONTINUE request ``rid`` from where it stands: their prompt is ``result(rid)`` as it is now
        (inherited events in front of their own in ``result()``), their first event is reported by the next ``step()``; -> their
        ids.  The parent is running or held (``submit(hold=True)``); it runs on, or stays held, untouched.  No prefill: the
        parent's K/V is copied into ``count`` free rows and the rows' state set in one ``DecodeSession.fork`` -- one kernel launch
        and the scatter of an admission.  The children of a parent that shares its prompt (``share_prefix``) JOIN its prefix slot:
        only the parent's own events behind the prompt are copied, and they are share requests themselves.  The rows are taken NOW,
        the lowest first and ahead of the queue.  A setting left at None is the parent's; ``max_len`` must exceed
        ``len(result(rid))`` (so a held parent's children need one).  In a seeded pool ``seed`` is an int for one child, a sequence
        of ``count`` ints for several.
        Seeded pools: the variate counter of an event is its index in the result, so a child continues the parent's counter under
        its own seed -- a child given the parent's seed and settings repeats the parent event for event, and a held request forked
        under its own seed with a larger ``max_len`` gives exactly what an uninterrupted request with that ``max_len`` gives.  The
        limit is the module docstring's: equal launch shapes (the same pool size; the parent's prefill in the same admission
        grouping) -- the copy itself is bit-exact and the decode kernels treat rows independently.
        ``ValueError`` before any launch: an unknown, queued, released or EOS-ended parent, fewer than ``count`` free rows,
        ``max_len <= len(result(rid))``, ``max_len + 1 > capacity``, and every refusal of ``submit``'s settings."""
        if self._closed:
            raise ValueError("DecodePool.fork: the pool is closed")
        r = self.requests.get(rid) if isinstance(rid, (int, np.integer)) and not isinstance(rid, bool) else None
        if r is None:
            raise ValueError(f"DecodePool.fork: no request {rid!r}")
        if r.eos:
            raise ValueError(f"DecodePool.fork: request {rid} ended on EOS: there is nothing to continue")
        if r.row is None:
            raise ValueError(f"DecodePool.fork: request {rid} is {'released: its row is gone' if r.done else 'still queued'} -- a "
                             f"parent is running, or held (submit(hold=True))")
        if isinstance(count, bool) or not isinstance(count, (int, np.integer)) or not 1 <= count <= self.rows:
            raise ValueError(f"DecodePool.fork: count = {count!r} is not an integer in [1, {self.rows}] (the pool's rows)")
        count = int(count)
        if count > len(self.free):
            raise ValueError(f"DecodePool.fork: {count} rows are needed, {len(self.free)} are free")
        seeds = self._seeds(seed, count, "fork", "count")
        given = (max_len, temp, top_p, top_k, ban_eos, disable_patch_change, disable_control_change, disable_channels)
        kw = {name: r.kw[name] if v is None else v for name, v in zip(_SETTINGS, given)}
        prompt = self.result(rid)
        checked = [self._checked(prompt, kw, s, "fork", crop=None) for s in seeds]
        rows = self.free[:count]
        rp = {name: [c[1][name][0] for c in checked] for name in checked[0][1]}
        first, ban = self.model._mask_rows(rp)
        with torch.inference_mode():
            join = {"join": [True] * count} if r.share else {}
            self.ses.fork([r.row] * count, rows, [len(prompt)] * count, rp["max_len"], rp["temp"], rp["top_p"], rp["top_k"],
                          first, ban, seeds=rp.get("seed"), from_held=[r.held] * count, **join)
        del self.free[:count]
        rids = []
        for row, (p, one) in zip(rows, checked):
            rids.append(self._next_id)
            self._next_id += 1
            child = self.requests[rids[-1]] = _Request(p, one, kw, hold=hold, share=r.share)
            child.adapter = r.adapter   # (the session's fork copies row_adapter with the row)
            child.row = row
            self.occupied[row] = rids[-1]
        return rids

    def result(self, rid: int, forget: bool = False) -> np.ndarray:
        """request ``rid``'s events so far, ``(<= max_len, 8) int64`` with its (cropped, padded) prompt in front; ``forget``: drop a
        finished request from the pool's books"""
        r = self.requests[rid]
        out = np.concatenate([r.prompt] + [e[None] for e in r.events], axis=0)
        if forget and r.done:
            del self.requests[rid]
        return out

    def logprobs(self, rid: int) -> np.ndarray:
        """(a pool made with ``logprobs=True``) request ``rid``'s log-likelihoods so far: ``np.float32 [len(result(rid)) -
        len(prompt)]``, entry j the model's ll of the j-th event the request generated -- aligned with
        ``result(rid)[len(prompt):]`` (a fork child's prompt is what it inherited: its array covers its own events).  See the module
        docstring, "LOG-LIKELIHOODS".  ``ValueError`` on a pool made without the option."""
        if not self.want_logprobs:
            raise ValueError("DecodePool.logprobs: this pool keeps no log-likelihoods -- decode_pool(..., logprobs=True)")
        return np.asarray(self.requests[rid].logp, dtype=np.float32)

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
            if self.prefix_slots:  # every row leaves its slot and every slot is emptied: nothing outlives the pool
                with torch.inference_mode():
                    ses.reset()
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
            slots = dict(prefix_slots=self.prefix_slots, prefix_capacity=self.prefix_capacity) if self.prefix_slots else {}
            if self.kv_dtype is not None:
                slots = dict(kv_dtype=self.kv_dtype)
            if self.want_logprobs:  # (the call without the option is the call it was)
                slots["logprobs"] = True
            if self.lora_slots:  # (likewise)
                slots.update(lora_slots=self.lora_slots, lora_rank=self.lora_rank)
            if self.lookahead:  # (likewise) a group of lookahead + 1 session rows per request
                slots["lookahead"] = self.lookahead
            ses = self.model._checkout_session(self.rows * (self.lookahead + 1), self.capacity, 1.0, 0.98, 1, ragged=True,
                                                row_params=True, seeded=self.seeded, **slots)
            ses.reset()                      # every row free: pos = pos_limit = 0
            ses.begin(self.generator)
            self.ses = ses
        return self.ses

    def _admit_queued(self) -> None:
        # FIFO, whole sibling groups: the request at the head leads a group of r.group rows (1: a lone request); a group that
        # does not fit waits there, and what is queued behind it waits with it
        # (a share_prefix group needs a free prefix slot as well, and waits in the same place for one)
        groups, k, slots = [], 0, self._free_slots()
        while self.queue and k + self.requests[self.queue[0]].group <= len(self.free):
            head = self.requests[self.queue[0]]
            if head.share and not slots:
                break
            g = head.group
            groups.append([self.queue.popleft() for _ in range(g)])
            k += g
            if head.share:
                slots.pop(0)
        if k == 0:
            return
        taken = self.free[:k]
        del self.free[:k]
        lead = {True: [], False: []}  # share -> [(row, request id)] of the group leaders
        forks, at = [], 0             # (leader's row, sibling's row, sibling's id, the sibling joins the leader's slot)
        for grp in groups:
            share = self.requests[grp[0]].share
            lead[share].append((taken[at], grp[0]))
            forks += [(taken[at], taken[at + i], rid, share) for i, rid in enumerate(grp) if i > 0]
            at += len(grp)
        ses = self._session()
        # an admission stores into slots or into rows: the sharing leaders take a packed forward of their own, K/V into free slots
        for share in (True, False):
            if not lead[share]:
                continue
            # ... and one admit per adapter, in the order the adapters first appear (a pool without adapter slots: one admit)
            order = []
            for _, i in lead[share]:
                if self.requests[i].adapter not in order:
                    order.append(self.requests[i].adapter)
            for aid in order:
                mine = [(r, i) for r, i in lead[share] if self.requests[i].adapter == aid]
                rows, rids = [r for r, _ in mine], [i for _, i in mine]
                reqs = [self.requests[rid] for rid in rids]
                rp = {name: [r.rp[name][0] for r in reqs] for name in reqs[0].rp}
                first, ban = self.model._mask_rows(rp)
                tokens = torch.from_numpy(np.concatenate([r.prompt for r in reqs], axis=0))
                into = {"slots": ses.free_slots()[:len(rows)]} if share else {}
                if self.lora_slots:
                    into["adapter"] = None if aid is None else self.adapters[aid]
                ses.admit(rows, tokens, [len(r.prompt) for r in reqs], rp["max_len"], rp["temp"], rp["top_p"], rp["top_k"], first,
                          ban, seeds=rp.get("seed"), **into)
                for row, rid, r in zip(rows, rids, reqs):
                    r.row = row
                    self.occupied[row] = rid
        if forks:  # the siblings, right behind the prefills that made their leaders: the leaders' K/V and last hidden rows -- a
            #        sharing group's siblings JOIN the leader's slot instead and copy nothing
            sibs = [self.requests[rid] for _, _, rid, _ in forks]
            rp = {name: [r.rp[name][0] for r in sibs] for name in sibs[0].rp}
            first, ban = self.model._mask_rows(rp)
            join = {"join": [j for _, _, _, j in forks]} if any(j for _, _, _, j in forks) else {}
            ses.fork([s for s, _, _, _ in forks], [d for _, d, _, _ in forks], [len(r.prompt) for r in sibs], rp["max_len"],
                     rp["temp"], rp["top_p"], rp["top_k"], first, ban, seeds=rp.get("seed"), **join)
            for (_, row, rid, _), r in zip(forks, sibs):
                r.row = row
                self.occupied[row] = rid

    def _free_slots(self) -> List[int]:
        if self.ses is None:
            return list(range(self.prefix_slots))
        return self.ses.free_slots()

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
            if not self.occupied:  # (a sibling group at the head of the queue, and held requests on the rows it waits for)
                head = self.requests[self.queue[0]]
                slots = f", {len(self._free_slots())} of {self.prefix_slots} prefix slots (it needs one)" if head.share else ""
                raise RuntimeError(f"DecodePool.step: nothing runs and the group of {head.group} requests "
                                   f"at the head of the queue cannot be admitted: {len(self.free)} rows are free{slots}, "
                                   f"{len(self.held_rows)} held -- drop() a held request")
            ses = self.ses
            self.steps += 1
            if self.lookahead:
                return self._step_lookahead(eos)
            live = [row in self.occupied for row in range(self.rows)]
            running = [self.requests[rid] for rid in self.occupied.values()]
            # (a request that is to be held needs the net step over its LAST event too: its K/V row max_len - 1 and the hidden row
            #  that hold() keeps)
            more = any(len(r.prompt) + len(r.events) + 1 < r.max_len or r.hold for r in running)
            speculative = more and ses.g_steps is not None and _SPECULATIVE_NET
            event, _ = ses.sample_event(then_net=speculative, live=live)
            if self.want_logprobs:  # ll of an event: its token positions 0..arity, summed here in fp32 (one running sum over the
                #                     block, position by position); EOS is position 0 alone
                logp, arity = np.cumsum(ses.last_logp, axis=1, dtype=np.float32), self.model._grammar()[3]
            out, finished, keep = [], [], []
            for row, rid in sorted(self.occupied.items(), key=lambda kv: kv[1]):
                r = self.requests[rid]
                ev = event[row].copy()
                r.events.append(ev)
                r.eos = bool(ev[0] == eos)
                if self.want_logprobs:
                    r.logp.append(logp[row, 0 if r.eos else arity[int(ev[0])]])
                r.done = r.eos or len(r.prompt) + len(r.events) >= r.max_len
                if r.done:
                    (keep if r.hold and not r.eos else finished).append(row)
                out.append((rid, ev, r.done))
            if len(finished) + len(keep) < len(out):  # a request continues: the next event's draws, under the net step over this event
                ses.draw_noise()
            if (len(finished) < len(out)) and not speculative:  # ... or is to be held
                ses.net_step()
            if keep:  # (behind the net step over their last event: the rows stay parked at max_len, nothing is released)
                ses.hold(keep)
                for row in keep:
                    rid = self.held_rows[row] = self.occupied.pop(row)
                    self.requests[rid].held = True
            if finished:  # (behind the net step, which advanced these rows with the rest)
                ses.release(finished)
                for row in finished:
                    self.requests[self.occupied.pop(row)].row = None
                self.free = sorted(self.free + finished)
        return out

    # ---- lookahead (the module docstring, "LOOKAHEAD") --------------------------------------------------------------------------
    @staticmethod
    def accept(samples: np.ndarray, drafts: np.ndarray, t: int, max_len: int, eos_id: int) -> int:
        """the acceptance rule -> the number of TRUE events at the head of ``samples`` (>= 1).  samples [k + 1, 8]: row j of the
        group sampled samples[j] for event index t + j; drafts [<= k, 8]: drafts[i - 1] is what row i consumed as event t + i - 1 in
        the previous net step.  samples[0] is true; samples[i] is true iff samples[i - 1] is and drafts[i - 1] equals it in all 8
        tokens.  The run ends behind an EOS and behind the event that brings the request to ``max_len`` events."""
        n = 1
        while not (samples[n - 1][0] == eos_id or t + n >= max_len or n > len(drafts) or n >= len(samples)
                   or not np.array_equal(drafts[n - 1], samples[n - 1])):
            n += 1
        return n

    def _drafts(self, r: _Request, history: np.ndarray) -> np.ndarray:
        """the proposer's guess for the events behind ``history`` (request r's prompt + result), checked, and cut to the rows that can
        sample an event below ``max_len`` (draft row j samples index len(history) + j)"""
        k = self.lookahead
        T, V = self.model.tokenizer.max_token_seq, self.model.tokenizer.vocab_size
        room = min(k, r.max_len - 1 - len(history))
        if room < 1:
            return np.zeros((0, T), dtype=np.int64)
        d = np.asarray(self.proposer(history, k))
        if d.size == 0:
            return np.zeros((0, T), dtype=np.int64)
        if d.ndim != 2 or d.shape[1] != T or len(d) > k or d.dtype.kind not in "iu" or d.min() < 0 or d.max() >= V:
            raise ValueError(f"DecodePool.step: the proposer returned {d.dtype} {tuple(d.shape)}: at most {k} events of {T} token ids "
                             f"in [0, {V}) are a guess")
        return d[:room].astype(np.int64)

    def _step_lookahead(self, eos: int) -> List[Tuple[int, np.ndarray, bool]]:
        """steps 1 to 4 of the module docstring, behind the admissions; ``row`` of a request is its GROUP here.  The host part is
        planned first and committed afterwards, so that a proposer that raises, or returns what is no guess, leaves every request as
        it was: the next ``step()`` samples the same events again (the seeded sampler's draws are a function of the state)."""
        ses, gw = self.ses, self.lookahead + 1
        live = [False] * (self.rows * gw)   # (the break rule of the step-by-step form: every row whose sample may be accepted)
        for g, rid in self.occupied.items():
            for j in range(len(self.requests[rid].drafts) + 1):
                live[g * gw + j] = True
        event, _ = ses.sample_event(then_net=False, live=live)
        if self.want_logprobs:
            logp, arity = np.cumsum(ses.last_logp, axis=1, dtype=np.float32), self.model._grammar()[3]
        plan = []   # (group, request, true events, their ll, eos, done, the drafts for the next net step)
        for g, rid in sorted(self.occupied.items(), key=lambda kv: kv[1]):
            r = self.requests[rid]
            t = len(r.prompt) + len(r.events)
            samples = event[g * gw:(g + 1) * gw]
            n = self.accept(samples, r.drafts, t, r.max_len, eos)
            evs = [samples[i].copy() for i in range(n)]
            is_eos = bool(evs[-1][0] == eos)
            # an accepted event's ll comes from the row that sampled it
            ll = [logp[g * gw + i, 0 if evs[i][0] == eos else arity[int(evs[i][0])]] for i in range(n)] if self.want_logprobs else []
            done = is_eos or t + n >= r.max_len
            drafts = r.drafts[:0] if done else self._drafts(r, np.concatenate([r.prompt] + [e[None] for e in r.events + evs], axis=0))
            plan.append((g, rid, r, evs, ll, is_eos, done, drafts))
        out, finished, keep = [], [], []
        rows, inputs, poss, caches = [], [], [], []
        for g, rid, r, evs, ll, is_eos, done, drafts in plan:
            r.events += evs
            r.logp += ll
            self.drafted, self.accepted = self.drafted + len(r.drafts), self.accepted + len(evs) - 1
            r.eos, r.done, r.drafts = is_eos, done, drafts
            out += [(rid, ev, done and i == len(evs) - 1) for i, ev in enumerate(evs)]
            if done and not (r.hold and not is_eos):
                finished.append(g)
                continue
            if done:  # to be held: the net step over its final event, the draft rows inactive
                keep.append(g)
            # the group's inputs for the net step: the leader consumes the last true event, draft row j the j-th guess behind it
            t, m = len(r.prompt) + len(r.events), len(drafts)
            rows += [g * gw + j for j in range(gw)]
            inputs += [evs[-1]] + list(drafts) + [evs[-1]] * (gw - 1 - m)
            poss += [t - 1 + j for j in range(m + 1)] + [0] * (gw - 1 - m)
            caches += [g] * (m + 1) + [-1] * (gw - 1 - m)
        if rows:  # a request continues, or is to be held
            ses.set_inputs(rows, np.stack(inputs), poss, caches)
            ses.net_step()
        if keep:  # (behind the net step over their last event: the leaders stay parked at max_len, nothing is released)
            ses.hold(keep)
            for g in keep:
                rid = self.held_rows[g] = self.occupied.pop(g)
                self.requests[rid].held = True
        if finished:
            ses.release(finished)
            for g in finished:
                self.requests[self.occupied.pop(g)].row = None
            self.free = sorted(self.free + finished)
        return out
