"""KV-cached decode driver for ``MIDIModel.generate`` (midi_model.py:167-250).

The reference spends a generated event in ~1000 launches and B host syncs.  Here one event is THREE graph replays and
ONE device->host copy:

    noise graph  (side stream, overlapping the previous event's net step): the Exp(1) variates torch.multinomial would draw
                 inside sample_top_p_k for the 8 token positions, [8, B, vocab], from a session generator that carries the
                 caller's generator state in and out
    steps graph  all 8 token steps back to back: (embedding of the token just sampled ->) 3 decoder layers at position i ->
                 lm_head -> fused grammar-masked softmax + top-p/top-k + draw (mh_sample_top_p_k) on that noise
    [copy]       the event's 8 tokens to the host; the reference's break rule (midi_model.py:232-235) is evaluated on them
                 AFTERWARDS: positions past an event's arity sample PAD whether or not the loop runs them, so running all 8
                 changes nothing but the number of draws -- and the generator is wound back to exactly the draws the
                 reference would have made (philox offset arithmetic), so a seeded torch.Generator still yields the
                 reference loop's stream (tests/test_decode_gpu.py drives app.py's loop against generate())
    net graph    embedding sum of the event's 8 tokens -> 12 decoder layers on one position per sequence -> final norm;
                 K/V appended to preallocated caches at a position kept in DEVICE memory

Samplers the fused kernel does not cover (top_k > 64) and the eager mode (MH_DECODE_GRAPHS=0, the CPU fake backend of the
tests) keep the step-by-step form: one graph / call per token step with the reference's own sampling ops inside.

The graphs are hipGraphs captured through torch.cuda.CUDAGraph from the same Python schedule the eager path runs
(``engine.stack_decode``), so there is one implementation of the step.  A session owns every buffer the graphs touch and
is keyed by (parameter buffer, batch, capacity, temperature, top_p, top_k) -- a ``row_params`` session, below, by the first
three alone; ``MIDIModel`` keeps a pool of them and hands one to each ``generate`` call, so concurrent generators on one model
(app.py:496) never share scratch.

``shared_capacity`` > 0 (generate(share_prompt=True), shared.py): the B rows continue ONE prompt.  ``kvp`` (one sequence,
shared_capacity rows) holds the prompt's K/V, ``kv1`` only the generated suffix, a device int32 ``pre_len`` sits beside ``pos``,
and the net step's attention is the two launches of shared.py.  The captured graph reads ``pos`` and ``pre_len`` from device
memory and its launch geometry depends on the capacities only, so one session serves every prompt length <= shared_capacity.

``ragged`` (generate_ragged): the B rows continue B DIFFERENT prompts of B different lengths, in lockstep.  ``pos`` is then int32 [B]
-- every row's own position -- the net step's attention runs the per-row kernels on it (engine.stack_decode(row_pos=...)), and
the net body advances it on the device as pos = min(pos + 1, pos_limit), pos_limit = the call's max_len: a row that has reached
max_len is PARKED there, keeps overwriting cache row max_len (capacity max_len + 1, the plain rule) and keeps being sampled; the
host drops what it samples.  No per-row host state, no extra sync; the graphs' geometry depends on B and the capacity only, so
one pooled session serves any mix of lengths.  The token level, the sampler and the noise graph are row-uniform and unchanged.

``row_params`` (ragged only; generate_ragged with a value per row): temperature, top-p, top-k, the two masks and the parking position
live in session buffers with one entry per row -- ``temp_rows``, ``top_p_rows``, ``top_k_rows`` [B], ``first_mask`` and ``ban`` [B, V],
``pos_limit`` [B] -- and the token steps call mh_sample_top_p_k_rows, which reads them on the device.  The captured graphs hold
addresses, not values, and the pool key holds no sampling parameter: one session serves every setting of its (B, capacity), and
a new setting is B-element copies (set_row_params, set_limit) instead of a new K/V cache and three captures.  The form has no
op-by-op sampler behind it: it needs the fused kernel (grammar spans of at most 2048 ids, top_k <= 64).

``seeded`` (row_params only; generate_ragged(seed=...), decode_pool(seeded=True)): a seed per row in ``seed_rows`` (int64 [B]: the 64
bits), and the token steps call mh_sample_top_p_k_seeded with ``seed_rows`` and ``pos`` -- row b's variate at token position i for
rank j is Philox4x32-10 of (pos[b], i, j) under seed_rows[b], computed by the lanes that need one.  ``pos[b]`` is the index of the
event being sampled in row b's result (prompt events + events generated so far): the token steps of an event run before the net
body advances it.  Such a session has no ``q_all``, no noise graph, no noise stream and no generator (``gen is None``):
``draw_noise`` / ``consumed`` do nothing, ``begin`` / ``end`` touch no generator, one event is TWO graph replays.  The graphs read
both arrays at replay time, so a new seed is a B-element copy (``set_row_seeds``) or one more section of an admission's block.  Its
pool key carries "seeded": an unseeded session is never handed out in its place, and no existing key changes.

``admit`` / ``release`` (row_params sessions; pool.DecodePool drives them): rows of a RUNNING batch change hands between two
events.  ``admit(rows, ...)`` runs one packed forward over the new prompts alone, stores their K/V into cache rows ``rows``
(mh_kv_store_seqs_rows) and overwrites those rows of ``hidden``, ``pos``, ``pos_limit``, the three sampler arrays and the two masks;
``release(rows)`` sets pos = pos_limit = 0 there, so that a free row attends to one key.  STREAM ORDER is the correctness argument:
  1. the net step over the event just sampled runs for ALL rows first -- with ``then_net`` it is already queued behind the token
     steps, otherwise the caller queues it before it admits; it reads and advances ``pos`` and writes ``hidden`` of every row;
  2. the admission follows ON THE SAME STREAM and overwrites ``hidden``, ``pos`` and cache rows [0, L) of the admitted rows, so
     what step 1 left there (the continuation of a request that has finished, or of nothing) is gone before anything reads it;
  3. the next token steps, on the same stream again, sample every row from ``hidden``, the admitted rows from their prompts' last
     positions.
Stale K/V at cache rows >= L of a reused row is never read: attention reads rows [0, pos] and every one of them has been written
since the admission -- [0, L) by the prefill, row p by the net step that stood at p.  The noise graph runs on its own stream and
touches ``q_all`` alone, the copy stream reads ``seq`` alone; an admission writes neither.  No graph is recaptured and no graph
body changes: every buffer named above sits at the address the captures hold.

``fork`` / ``hold`` (row_params sessions; pool.DecodePool drives them): a row is DUPLICATED into free rows between two events, without
a second prefill.  ``fork(src, dst, lengths, ...)`` is one mh_kv_fork_rows launch over the whole of ``kv1`` (every layer, K and V, rows
[0, lengths[p]) of sequence src[p] into sequence dst[p]) and the scatter of an admission with ``hidden[dst] = hidden[src]`` and
``pos[dst] = lengths``; it runs no forward.  The same stream order carries it:
  1. the net step over the source's last event runs first, on the session's stream: it wrote the source's K/V row lengths[p] - 1 and
     its ``hidden``, and advanced its ``pos`` to lengths[p] -- so the source's cache rows [0, lengths[p]) and ``hidden`` are exactly
     the state from which event lengths[p] is sampled;
  2. the fork follows ON THE SAME STREAM: the copy reads that state and overwrites cache rows [0, lengths[p]), ``hidden``, ``pos`` and
     the settings of the destination rows -- free rows, whose own state nothing reads; the source rows are only read;
  3. the next token steps, on the same stream again, sample the destination rows from the copied ``hidden``; the net step behind them
     appends at row lengths[p] of each sequence on its own.
Stale K/V at cache rows >= lengths[p] of a destination is never read, by the argument above.  A source that has reached its max_len is
PARKED: the net steps that follow keep writing its cache row max_len and its ``hidden``, never rows [0, max_len).  ``hold(rows)``
therefore copies ``hidden[rows]`` into ``held_hidden`` right behind the net step over the row's last event, and a later
``fork(from_held=...)`` takes ``hidden`` from there: a held row can be continued any number of steps later.

``prefix_slots`` = G > 0 with ``prefix_capacity`` = Pmax (row_params sessions; decode_pool(prefix_slots=...)): rows may
SHARE a prompt's K/V.  ``kvs`` holds G prefix slots of Pmax rows per layer ([G, H, Pmax, 64]), ``slot_len`` (int32 [G]; 0: empty)
their lengths and ``row_slot`` (int32 [B]; -1: none) the slot each row continues; a sharing row's own cache ``kv1`` holds only what
lies BEHIND its slot's prompt -- cache row j is absolute position slot_len[row_slot[b]] + j -- while ``pos`` and ``pos_limit`` stay
absolute.  The net step's attention is the two launches of ops_share.py for EVERY row (a row without a slot merges no partial and
does the per-row kernel's arithmetic).  The graphs read the three arrays at replay time and their geometry depends on (B, capacity,
G, Pmax) only: nothing is recaptured.  ``admit(slots=...)`` stores the admitted prompts' K/V into slots instead of rows;
``fork(join=...)`` lets a destination join its source's slot and copies only the source's own cache rows [0, pos - pre) -- nothing
when that is empty; ``release`` frees a slot (slot_len = 0, in stream order) when its last row leaves, a held row keeping its slot.
The host keeps the slot of every row, every slot's length and its reference count (``slot_refs``): it decides which slot is free.
``prefix_slots=0`` is the session as it was: no new buffer, no new key, the same launches.

``kv_dtype="fp8"`` (row_params sessions, seeded or not; a bf16 model, at most 256 rows; decode_pool(kv_dtype="fp8")):
``kv1`` is an ``engine.KVStateQ`` -- e4m3fn codes with an fp32 scale per (row, head, event) for K and for V, 136 bytes where the
bf16 cache holds 256.  ``admit`` stores through mh_kv_store_seqs_rows_fp8, the net step attends through
mh_attn_decode_append_rows_fp8 (the new row is quantized first and attended to as the cache holds it, so a fork or a
held-then-forked request sees the keys an uninterrupted one saw) and ``fork`` copies through mh_kv_fork_rows_fp8.  The graphs are
captured from the same schedule and nothing is recaptured.  Not with prefix slots or a shared prompt; ``prefill`` and
``prefill_ragged`` refuse such a session.  ``kv_dtype=None`` is the session as it was: the same key, buffers and launches.

``logprobs`` (row_params sessions; seeded or not, with or without prefix slots or the fp8 cache; decode_pool(logprobs=True), DESIGN
7.12): the token steps call the ``_logp`` form of their sampler (mh_sample_top_p_k_rows_logp / mh_sample_top_p_k_seeded_logp) -- the
same ids bit for bit -- which also writes ``logp_rows[:, i]`` (fp32 [B, T]): the model's own log-probability z_c - log sum exp z of
the id each row drew at token position i, whatever the row's temperature, top-p, top-k and masks.  ``sample_event`` copies the buffer
to a pinned host block on the copy stream beside ``seq``, under the same one synchronise, and leaves the event's values in
``last_logp`` (np.float32 [B, T]; positions past an event's arity hold the pad token's value or, in the step-by-step form, what an
earlier event left: the caller sums positions 0..arity).  Only the sampler call changes: admissions, forks and releases recapture
nothing.  The key's form gains ``("logp",)`` at its end; ``logprobs=False`` is the session as it was: the same key, buffers and launches.

``lookahead`` = k > 0 (seeded row_params sessions, bf16 cache, no prefix slots, no adapters; decode_pool(lookahead=k)): the
B rows are B / (k + 1) GROUPS of k + 1 consecutive rows -- row 0 of a group its LEADER, rows 1..k its DRAFT rows -- and the K/V of a
group live ONCE, in cache sequence g of ``kv1``, which is allocated for B / (k + 1) sequences (``kv2``, the token level, stays per
row).  ``row_cache`` (device int32 [B], a fixed buffer the captured net graph reads; -1: the row is inactive) names the cache sequence
of every row, and the net step's attention is the pair of ops_lookahead.py: every active row stores its K/V at ``pos[b]`` of its
group's sequence, then every active row attends to rows [0, pos[b]] of it -- so a draft row at position p + j sees what the leader
(at p) and the draft rows below it stored in the same layer.  ``set_inputs`` scatters the rows' inputs (``seq``), positions and
``row_cache`` entries between the token steps and the net step, in one pinned block; the sampler's counter is ``pos[b]`` as in
every seeded session, so draft row j samples the event of index p + j + 1 under its request's seed.  ``admit`` / ``fork`` /
``hold`` / ``release`` then take GROUP indices where they take rows: a prompt's K/V goes into the group's cache sequence, the
leader's hidden row, position and settings are written as a row's are, and the leader's settings (limit, temperature, top-p, top-k,
both masks, seed) are copied into the group's draft rows, which start inactive.  Stale K/V of rejected drafts lie at or above the
leader's next position, and the next net step overwrites the rows it reads before it reads them.  Nothing is recaptured per step,
admission, fork or release.  The key's form gains ``("lookahead", k)``; ``lookahead=0`` is the session as it was: the same key,
buffers and launches.
"""
from __future__ import annotations

import os
import threading
from typing import List, Optional

import numpy as np
import torch

from . import engine, ops
from .engine import KVState, KVStateQ, RopeTable


# One capture at a time per process, and in thread-local error mode: generators of other threads (app.py runs up to 10 on
# one model) keep launching and allocating while a new session is being captured.
# Replays of graphs that carry a registered generator state (the noise graph; the per-step graphs of the unfused sampler) take the
# same lock: torch's replay prologue asserts that NO capture is active, and under HIP a capture on another thread's stream makes
# that check fire ("Cannot prepare for replay during capturing stage", seen once in ~3 runs of the whole GPU suite in
# test_concurrent_generators_on_one_model, r04).  Captures are rare (a session is captured once and pooled), so the replays of
# other generators wait a few hundred milliseconds at most.
_CAPTURE_LOCK = threading.RLock()
_NOISE_INLINE = os.environ.get("MH_DECODE_NOISE_INLINE", "0") == "1"
_COPY_PAGEABLE = os.environ.get("MH_DECODE_COPY_PAGEABLE", "0") == "1"


def graphs_enabled(device: torch.device) -> bool:
    return device.type == "cuda" and os.environ.get("MH_DECODE_GRAPHS", "1") != "0"


class DecodeSession:
    def __init__(self, model, B: int, capacity: int, temp: float, top_p: float, top_k: int, shared_capacity: int = 0,
                 ragged: bool = False, row_params: bool = False, seeded: bool = False, prefix_slots: int = 0,
                 prefix_capacity: int = 0, kv_dtype: Optional[str] = None, logprobs: bool = False, lora_slots: int = 0,
                 lora_rank: int = 64, lookahead: int = 0):
        tok = model.tokenizer
        self.model, self.B, self.cap, self.temp = model, B, capacity, float(temp)
        self.top_p, self.top_k = float(top_p), int(top_k)
        self.shared_capacity = int(shared_capacity)
        self.ragged = bool(ragged)
        self.row_params = bool(row_params)
        self.seeded = bool(seeded)
        self.prefix_slots, self.prefix_capacity = int(prefix_slots), int(prefix_capacity)
        self.kv_dtype = kv_dtype
        self.logprobs = bool(logprobs)
        self.lora_slots, self.lora_rank = int(lora_slots), int(lora_rank)
        self.lookahead = int(lookahead) if lookahead else 0
        self.gw = self.lookahead + 1          # rows per group (1: every row is its own group, the session as it was)
        self.groups = B // self.gw            # ... and the sequences of the event-level cache
        if lookahead:  # (the call without the option is the call it was)
            self.key = self.make_key(model, B, capacity, temp, top_p, top_k, shared_capacity, ragged, row_params, seeded,
                                     prefix_slots, prefix_capacity, kv_dtype, logprobs, lora_slots, lora_rank, lookahead)
        elif lora_slots:
            self.key = self.make_key(model, B, capacity, temp, top_p, top_k, shared_capacity, ragged, row_params, seeded,
                                     prefix_slots, prefix_capacity, kv_dtype, logprobs, lora_slots, lora_rank)
        else:
            self.key = self.make_key(model, B, capacity, temp, top_p, top_k, shared_capacity, ragged, row_params, seeded,
                                     prefix_slots, prefix_capacity, kv_dtype, logprobs)
        dev, dt = model.device, model.dtype
        self.T, self.V, self.Vp = tok.max_token_seq, tok.vocab_size, model.vocab_padded
        spec, tspec = model._specs["net"], model._specs["net_token"]
        if kv_dtype == "fp8":  # codes and a scale pair per (row, head, event); never grown
            self.kv1 = KVStateQ(spec, B, capacity, model._flat)
        else:  # (lookahead: a sequence per GROUP)
            self.kv1 = KVState(spec, self.groups, capacity, model._flat)  # (shared: the generated suffix only)
        self.kv2 = KVState(tspec, B, self.T, model._flat)
        self.kvp = self.pre_len = self.ws = None
        if self.shared_capacity > 0:
            from . import shared
            self.kvp = KVState(spec, 1, self.shared_capacity, model._flat)  # the prompt, once
            self.pre_len = torch.zeros(1, dtype=torch.int32, device=dev)      # its length (device side, beside pos)
            self.ws = torch.empty(shared.workspace_floats(B, spec.H, self.shared_capacity), dtype=torch.float32, device=dev)
        # (lookahead) the cache sequence of every row, -1: inactive; read by the captured net graph
        self.row_cache = torch.full((B,), -1, dtype=torch.int32, device=dev) if self.lookahead else None
        self._look_stage = None    # the pinned host block of the last set_inputs
        self.kvs = self.slot_len = self.row_slot = None
        if self.prefix_slots > 0:
            from .ops_share import workspace_floats
            G, Pmax = self.prefix_slots, self.prefix_capacity
            self.kvs = KVState(spec, G, Pmax, model._flat)                        # the G shared prompts, once each
            self.slot_len = torch.zeros(G, dtype=torch.int32, device=dev)        # their lengths (0: the slot is empty)
            self.row_slot = torch.full((B,), -1, dtype=torch.int32, device=dev)  # the slot each row continues (-1: none)
            self.ws = torch.empty(workspace_floats(B, spec.H, Pmax), dtype=torch.float32, device=dev)
            self._reset_slots_host()
        # rope tables private to the session: a captured graph keeps their addresses
        self.rope1 = RopeTable(spec.hd, spec.theta, dev, capacity + self.shared_capacity)
        self.rope2 = RopeTable(tspec.hd, tspec.theta, dev, self.T)
        first, lo, hi, _ = model._grammar()
        self.first_mask = first.clone()           # generate() overwrites it (ban_eos, disable_patch/control_change)
        self.ban = torch.zeros_like(first)        # ids removed from every mask (disable_channels); generate() fills it
        self.lo_tab, self.hi_tab = lo, hi
        self.first_span, self.max_range = ops.mask_spans(first, lo, hi)  # (generate() only ever clears bits of first_mask)
        self.fused_sampler = (1 <= self.top_k <= min(ops.SAMPLE_MAX_K, self.V) and max(self.max_range) <= ops.SAMPLE_MAX_RANGE
                              and self.first_span[1] - self.first_span[0] <= ops.SAMPLE_MAX_RANGE)
        self.temp_rows = self.top_p_rows = self.top_k_rows = None
        if self.row_params:
            if not self.fused_sampler:
                raise ValueError(f"DecodeSession(row_params=True) needs the fused sampler: top_k {self.top_k} outside [1, "
                                 f"{min(ops.SAMPLE_MAX_K, self.V)}] or a grammar mask of more than {ops.SAMPLE_MAX_RANGE} ids")
            # one entry per row at fixed addresses (the arguments fill them until set_row_params / generate_ragged does)
            self.temp_rows = torch.full((B,), self.temp, dtype=torch.float32, device=dev)
            self.top_p_rows = torch.full((B,), self.top_p, dtype=torch.float32, device=dev)
            self.top_k_rows = torch.full((B,), self.top_k, dtype=torch.int32, device=dev)
            self.first_mask = first[None, :].repeat(B, 1)
            self.ban = torch.zeros_like(self.first_mask)
        # (seeded) row b's seed, the 64 bits in int64 storage; zeros until set_row_seeds / admit writes a request's
        self.seed_rows = torch.zeros((B,), dtype=torch.int64, device=dev) if self.seeded else None
        # cached events so far (device side); ragged: per row, and the position a row is parked at (the call's max_len)
        self.pos = torch.zeros(B if self.ragged else 1, dtype=torch.int32, device=dev)
        self.pos_limit = torch.zeros(B if self.row_params else 1, dtype=torch.int32, device=dev) if self.ragged else None
        self.hidden = torch.zeros((B, spec.D), dtype=dt, device=dev)
        self.seq = torch.zeros((B, self.T), dtype=torch.long, device=dev)  # tokens of the event being sampled
        self.samples_in = torch.zeros((B,), dtype=torch.long, device=dev)  # token sampled at the previous position
        # (logprobs) the model's log-probability of every token of the event being sampled, written by the token steps' samplers
        self.logp_rows = torch.zeros((B, self.T), dtype=torch.float32, device=dev) if self.logprobs else None
        self.last_logp = None  # ... and the host copy sample_event() leaves: np.float32 [B, T] of the event it returned
        self.ev = torch.zeros((B,), dtype=torch.long, device=dev)          # event id (token 0) of the current event
        self.pad_id = tok.pad_id
        self.neg1 = torch.full((B,), -1, dtype=torch.int32, device=dev)
        self.probs = torch.zeros((B, 1, self.V), dtype=torch.float32, device=dev)
        # Exp(1) noise of the sampler, one [B, V] slice per token position (ones: a step sampled before any draw is greedy-safe)
        # (a seeded session has none: its sampler computes the variates it needs)
        self.q_all = None if self.seeded else torch.ones((self.T, B, self.V), dtype=torch.float32, device=dev)
        self.q = None if self.seeded else self.q_all[0]
        self.logits = torch.zeros((B, self.Vp), dtype=dt, device=dev)
        # RMSNorm weights folded into the projections that follow them (one launch for norm + projection)
        self.fold1 = self.fold2 = self.lm_fold = None
        # (lora_slots) G adapter slots per stack, unmerged in the decode step (engine.LoraStack); one row_adapter / slot_scale for both
        self.lora1 = self.lora2 = self.row_adapter = None
        self._lora_loaded = {}      # slot -> (event-level layers, scale): what admit() merges for the prompt's prefill
        self._merged = None         # the second copy of the event-level matrices, W + s B A of slot _merged_of
        self._merged_of = None
        probe = torch.empty((B, 1), dtype=dt, device=dev)
        # 65 to 256 rows: the same folded layer on mh_gemm_skinny_wide, unless MH_DECODE_WIDE=0 (read here, once) keeps the general form
        self.wide = ops.decode_wide_enabled() and ops.skinny_wide_ok(probe, spec.D)
        served = ops.skinny_wide_ok if self.wide else ops.skinny_ok
        if served(probe, spec.D) and served(probe, spec.I) and served(probe, tspec.I) \
                and os.environ.get("MH_DECODE_FOLD", "1") != "0":
            self.fold1 = engine.fold_norm_weights(model._W["net"])
            self.fold2 = engine.fold_norm_weights(model._W["net_token"])
            self.lm_fold = torch.empty_like(model.lm_head.weight.data)
            if self.lora_slots:
                self.lora1 = engine.LoraStack(spec, len(model._W["net"].layers), self.lora_slots, self.lora_rank, B, model._flat)
                self.lora2 = engine.LoraStack(tspec, len(model._W["net_token"].layers), self.lora_slots, self.lora_rank, B, model._flat)
                self.lora2.row_adapter, self.lora2.slot_scale = self.lora1.row_adapter, self.lora1.slot_scale
                self.row_adapter = self.lora1.row_adapter
            self.refresh()
        if self.lora_slots and self.lora1 is None:
            raise ValueError("DecodeSession: lora_slots needs the fused folded decode form (hidden and MLP widths that are multiples of "
                             "256, MH_DECODE_FOLD not 0)")
        self.g_net = None
        self.g_tok: List[Optional[torch.cuda.CUDAGraph]] = [None] * self.T
        self.g_noise = self.g_steps = None
        self.use_graphs = graphs_enabled(dev)
        # the generator the captured sampler draws from (a seeded session draws from none)
        self.gen = torch.Generator(device=dev) if self.use_graphs and not self.seeded else None
        self._user_gen = None
        self._admit_stage = None   # the pinned host block of the last admission (admit)
        self._fork_stage = None    # ... and of the last fork
        self.held_hidden = None    # [B, D]: hidden rows kept by hold(), allocated at first use
        self._pool = None
        self._off = 0          # philox offset of the next draw the reference loop would make
        self._draw_inc = 0     # philox offset consumed by one [B, V] exponential_ call
        self._noise_pending = False
        self._noise_read = False   # the pending variates have been read by a tok_step (step-by-step form)
        self._steps_recorded = False
        self.noise_stream = self.noise_done = self.copy_stream = self.steps_done = self.seq_host = None
        if self.use_graphs:
            self._capture()

    @staticmethod
    def make_key(model, B, capacity, temp, top_p, top_k, shared_capacity=0, ragged=False, row_params=False, seeded=False,
                 prefix_slots=0, prefix_capacity=0, kv_dtype=None, logprobs=False, lora_slots=0, lora_rank=64, lookahead=0):
        if lookahead:
            if isinstance(lookahead, bool) or not isinstance(lookahead, (int, np.integer)) or lookahead < 1:
                raise ValueError(f"DecodeSession: lookahead={lookahead!r} -- an integer >= 1 (draft rows per group), or 0 for none")
            if not (ragged and row_params and seeded):
                raise ValueError("DecodeSession: lookahead is a form of the per-row seeded session -- it needs ragged=True, "
                                 "row_params=True, seeded=True (exact verification rests on the seeded sampler's counter)")
            if prefix_slots or prefix_capacity or kv_dtype is not None or lora_slots or shared_capacity:
                raise ValueError("DecodeSession: lookahead is not available together with prefix slots, kv_dtype or lora_slots")
            if B % (int(lookahead) + 1) or B > 256:
                raise ValueError(f"DecodeSession: lookahead={lookahead} needs whole groups of {int(lookahead) + 1} rows and at most "
                                 f"256 rows in all: {B} rows")
        if lora_slots:
            if not (ragged and row_params):
                raise ValueError("DecodeSession: lora_slots is a form of the per-row session -- it needs ragged=True, row_params=True")
            if model._flat.dtype != torch.bfloat16 or B > 256:
                raise ValueError(f"DecodeSession: lora_slots needs a bf16 model and at most 256 rows (the skinny projections are the "
                                 f"one form that takes the second operand pair): {model._flat.dtype}, {B} rows")
            if int(lora_slots) != lora_slots or int(lora_rank) != lora_rank or lora_slots < 1 or lora_rank < 8 or lora_rank % 8 \
                    or (lora_slots * lora_rank) % 256:
                raise ValueError(f"DecodeSession: lora_slots={lora_slots!r}, lora_rank={lora_rank!r} -- the rank a multiple of 8 and "
                                 f"slots x rank a multiple of 256")
        if logprobs and not (ragged and row_params):
            raise ValueError("DecodeSession: logprobs is a form of the per-row session -- it needs ragged=True, row_params=True")
        if kv_dtype is not None:
            if kv_dtype != "fp8":
                raise ValueError(f"DecodeSession: kv_dtype={kv_dtype!r} -- None (the cache in the model's dtype) or \"fp8\"")
            if not (ragged and row_params):
                raise ValueError("DecodeSession: kv_dtype=\"fp8\" is a form of the per-row session -- it needs ragged=True, "
                                 "row_params=True")
            if prefix_slots or prefix_capacity or shared_capacity:
                raise ValueError("DecodeSession: kv_dtype=\"fp8\" is not available with prefix slots or a shared prompt (their "
                                 "caches and kernels are bf16)")
            if model._flat.dtype != torch.bfloat16 or B > 256:
                raise ValueError(f"DecodeSession: kv_dtype=\"fp8\" needs a bf16 model and at most 256 rows (the fused per-row "
                                 f"attention is the one form that reads the fp8 cache): {model._flat.dtype}, {B} rows")
        if prefix_slots or prefix_capacity:
            if not (ragged and row_params) or int(prefix_slots) != prefix_slots or int(prefix_capacity) != prefix_capacity \
                    or prefix_slots < 1 or prefix_capacity < 1:
                raise ValueError(f"DecodeSession: prefix_slots={prefix_slots!r}, prefix_capacity={prefix_capacity!r} -- prefix slots "
                                 "are a form of the per-row session (ragged=True, row_params=True) and need at least one slot of "
                                 "at least one row")
        if ragged and shared_capacity:
            raise ValueError("DecodeSession: ragged rows have prompts of their own -- not together with a shared prompt")
        if seeded and not (ragged and row_params):
            raise ValueError("DecodeSession: seeded is a form of the per-row session -- it needs ragged=True, row_params=True")
        if row_params:
            if shared_capacity or not ragged:
                raise ValueError("DecodeSession: row_params is a form of the ragged session -- not with a shared prompt, not "
                                 "without ragged=True")
            # no temperature, top-p or top-k: they are buffer contents of this form, not facts of its graphs (nor is a seed)
            form = ("ragged", "row_params", "seeded") if seeded else ("ragged", "row_params")
            if prefix_slots:  # (no existing key changes: a session without slots keeps the key it had)
                form += (("slots", int(prefix_slots), int(prefix_capacity)),)
            if kv_dtype is not None:  # (likewise: only an fp8 session carries it)
                form += (("kv", "fp8"),)
            if logprobs:  # (likewise, at the end: only a session whose samplers write log-probabilities carries it)
                form += (("logp",),)
            if lora_slots:  # (likewise)
                form += (("lora", int(lora_slots), int(lora_rank)),)
            if lookahead:  # (likewise)
                form += (("lookahead", int(lookahead)),)
            return (model._flat.data_ptr(), model._flat.dtype, B, capacity, form)
        key = (model._flat.data_ptr(), model._flat.dtype, B, capacity, float(temp), float(top_p), int(top_k))
        if ragged:
            return key + (("ragged",),)
        return key + (("shared", int(shared_capacity)),) if shared_capacity else key

    def refresh(self) -> None:
        """Re-derive the folded weights (norm weight x projection) IN PLACE from the live parameters.  The training
        kernels write the flat parameter buffer through raw pointers (AdamW, LoRA materialisation), which no tensor version
        counter sees, so a pooled session refreshes every time it is handed out (model._checkout_session): ~0.3 GB of
        elementwise traffic per generate() call, and the captured graphs keep their addresses."""
        if self.fold1 is None:
            return
        m = self.model
        engine.fold_norm_weights(m._W["net"], out=self.fold1)
        engine.fold_norm_weights(m._W["net_token"], out=self.fold2)
        lm_w = m.lm_head.weight.data
        self.lm_fold.copy_(lm_w.float() * m._W["net_token"].norm.float()[None, :])
        if self.lora1 is not None:  # the norm-folded A stacks follow the norm weights; the merged copy follows the base weights
            self.lora1.refresh(m._W["net"])
            self.lora2.refresh(m._W["net_token"])
            self._merged_of = None

    # ---- the step bodies (run eagerly, or once under capture) ---------------------------------------------
    def _net_body(self):
        m = self.model
        spec = m._specs["net"]
        e = torch.empty((self.B, spec.D), dtype=m.dtype, device=m.device)
        ops.embed_sum_fwd(self.seq, m._W["net"].embed, e)  # the event sampled last
        if self.ragged:  # every row at its own position; a row at pos_limit stays there
            sh = None
            if self.kvs is not None:  # ... and behind the prompt of its slot, if it names one
                from .ops_share import SlotPrefix
                sh = SlotPrefix(self.kvs, self.slot_len, self.row_slot, self.ws)
            if self.row_cache is not None:  # the rows of a group on their leader's cache sequence
                engine.stack_decode(spec, m._W["net"], e, self.rope1, self.kv1, folded=self.fold1, out=self.hidden, row_pos=self.pos,
                                    wide=self.wide, row_cache=self.row_cache)
            elif self.lora1 is not None:
                engine.stack_decode(spec, m._W["net"], e, self.rope1, self.kv1, folded=self.fold1, out=self.hidden, row_pos=self.pos,
                                    wide=self.wide, shared=sh, lora=self.lora1)
            else:
                engine.stack_decode(spec, m._W["net"], e, self.rope1, self.kv1, folded=self.fold1, out=self.hidden, row_pos=self.pos,
                                    wide=self.wide, shared=sh)
            self.pos.add_(1)
            torch.minimum(self.pos, self.pos_limit, out=self.pos)
            return
        sh = None
        if self.kvp is not None:
            from .shared import SharedPrefix
            sh = SharedPrefix(self.kvp, self.pre_len, self.ws)
        engine.stack_decode(spec, m._W["net"], e, self.rope1, self.kv1, pos_dev=self.pos, folded=self.fold1, out=self.hidden,
                            shared=sh, wide=self.wide)
        self.pos.add_(1)

    def _noise_body(self, generator=None):
        """the draws of one event: what torch.multinomial(probs_sort [B, V]) would draw at each of the T token positions"""
        for i in range(self.T):
            self.q_all[i].exponential_(1.0, generator=generator)

    def _tok_body(self, i: int, generator=None, draw: bool = True):
        m = self.model
        tspec, Wt = m._specs["net_token"], m._W["net_token"]
        self.kv2.len = i
        lm_w = m.lm_head.weight.data
        skinny = ops.gemm_skinny_wide if self.wide else ops.gemm_skinny
        if self.lm_fold is not None:  # the stack's final RMSNorm rides on the lm_head projection
            more = dict(lora=self.lora2) if self.lora2 is not None else {}
            if i == 0:
                h = engine.stack_decode(tspec, Wt, self.hidden, self.rope2, self.kv2, folded=self.fold2, final_norm=False,
                                        wide=self.wide, **more)
            else:  # the embedding of the token just sampled is looked up inside the first projections
                h = engine.stack_decode(tspec, Wt, Wt.embed, self.rope2, self.kv2, folded=self.fold2, final_norm=False,
                                        x_ids=self.samples_in, wide=self.wide, **more)
            skinny(h, self.lm_fold, self.logits[:, : self.V], norm_eps=tspec.eps)
        else:
            x = self.hidden if i == 0 else Wt.embed.index_select(0, self.samples_in)
            h = engine.stack_decode(tspec, Wt, x, self.rope2, self.kv2, wide=self.wide)
            if (ops.skinny_wide_ok if self.wide else ops.skinny_ok)(h, tspec.D):
                skinny(h, lm_w, self.logits[:, : self.V])
            else:
                ops.gemm_nt(h, lm_w, self.logits[:, : self.V])
        if i == 0 and not self.fused_sampler:
            self.seq.fill_(self.pad_id)
        if self.fused_sampler:
            # one launch instead of sample_top_p_k's ~25: the Exp(1) noise torch.multinomial would draw internally
            # (empty_like(probs).exponential_(1, generator)) is drawn here (eager form) or by the noise graph ahead of the
            # step (draw=False), the rest is mh_sample_top_p_k
            # (logprobs) the ``_logp`` form of the row's sampler: the same ids, and logp_rows[:, i] = the model's log-probability of
            # the id each row drew, handed over behind the ban mask; without the option the call is the plain form's as it was
            lp = (self.logp_rows[:, i],) if self.logprobs else ()
            tail = dict(out_b=self.samples_in, out_c=self.ev if i == 0 else None, first_span=self.first_span,
                        max_range=self.max_range[i], fill_rest=self.T - 1 if i == 0 else 0, fill_id=self.pad_id)
            if self.seeded:  # nothing is drawn: row b's variates follow from seed_rows[b] and pos[b], the index of this event
                op = ops.sample_top_p_k_seeded_logp if self.logprobs else ops.sample_top_p_k_seeded
                op(self.logits, self.first_mask, self.lo_tab, self.hi_tab, self.ev, i, self.seed_rows, self.pos, self.seq[:, i], self.V,
                   self.temp_rows, self.top_p_rows, self.top_k_rows, self.ban, *lp, **tail)
                return
            if draw:
                self.q_all[i].exponential_(1.0, generator=generator)
            if self.row_params:  # the same kernel, row b on temp_rows[b], top_p_rows[b], top_k_rows[b] and its own two masks
                op = ops.sample_top_p_k_rows_logp if self.logprobs else ops.sample_top_p_k_rows
                op(self.logits, self.first_mask, self.lo_tab, self.hi_tab, self.ev, i, self.q_all[i], self.seq[:, i], self.V,
                   self.temp_rows, self.top_p_rows, self.top_k_rows, self.ban, *lp, **tail)
                return
            ops.sample_top_p_k(self.logits, self.first_mask, self.lo_tab, self.hi_tab, self.ev, i, self.q_all[i], self.seq[:, i],
                               self.V, self.temp, self.top_p, self.top_k, out_b=self.samples_in,
                               out_c=self.ev if i == 0 else None, first_span=self.first_span, max_range=self.max_range[i],
                               ban_mask=self.ban, fill_rest=self.T - 1 if i == 0 else 0, fill_id=self.pad_id)
            return
        if i == 0:
            lo, hi = self.neg1, self.neg1
        else:
            lo, hi = self.lo_tab[self.ev, i].contiguous(), self.hi_tab[self.ev, i].contiguous()
        ops.masked_softmax(self.logits, lo, hi, self.first_mask, self.probs.view(self.B, self.V), self.V, self.temp)
        self.probs.mul_((self.ban == 0).view(1, 1, self.V))
        samples = m.sample_top_p_k(self.probs, self.top_p, self.top_k, generator=generator)  # (B, 1)
        self.seq[:, i] = samples[:, 0]
        if i == 0:
            self.ev.copy_(self.seq[:, 0])
        self.samples_in.copy_(self.seq[:, i])

    def _capture(self):
        with _CAPTURE_LOCK:
            self._capture_locked()

    def _capture_locked(self):
        # one eager pass on a side stream first: lazy initialisation (kernel attributes, allocator pools) must not
        # happen inside a capture
        cur = torch.cuda.current_stream()
        side = torch.cuda.Stream()
        side.wait_stream(cur)
        with torch.cuda.stream(side):
            self._net_body()
            for i in range(self.T):
                self._tok_body(i, self.gen)
        cur.wait_stream(side)
        torch.cuda.synchronize()
        self._pool = pool = torch.cuda.graph_pool_handle()
        self.g_net = torch.cuda.CUDAGraph()
        with torch.cuda.graph(self.g_net, pool=pool, capture_error_mode="thread_local"):
            self._net_body()
        if self.seeded:
            # all T token steps in one graph; no noise graph, no noise stream: the sampler computes its variates
            self.g_steps = torch.cuda.CUDAGraph()
            with torch.cuda.graph(self.g_steps, pool=pool, capture_error_mode="thread_local"):
                for i in range(self.T):
                    self._tok_body(i, draw=False)
            self.copy_stream = torch.cuda.Stream()
            self.steps_done = torch.cuda.Event()
            self.seq_host = torch.empty((self.B, self.T), dtype=torch.long).pin_memory()
            self._pin_logp()
        elif self.fused_sampler:
            # the event's draws in one graph (the only one that touches the generator) ...
            self.g_noise = torch.cuda.CUDAGraph()
            self.g_noise.register_generator_state(self.gen)  # philox seed/offset are read at replay time, offsets advance per replay
            # (its own memory pool: it replays on the noise stream WHILE the net graph runs on the caller's stream)
            with torch.cuda.graph(self.g_noise, capture_error_mode="thread_local"):
                self._noise_body(self.gen)
            # ... and all T token steps in another
            self.g_steps = torch.cuda.CUDAGraph()
            with torch.cuda.graph(self.g_steps, pool=pool, capture_error_mode="thread_local"):
                for i in range(self.T):
                    self._tok_body(i, draw=False)
            o0 = self.gen.get_offset()
            self.g_noise.replay()
            torch.cuda.synchronize()
            self._draw_inc = (self.gen.get_offset() - o0) // self.T
            assert self._draw_inc > 0 and self._draw_inc * self.T == self.gen.get_offset() - o0
            self.noise_stream = torch.cuda.Stream()
            self.noise_done = torch.cuda.Event()
            self.copy_stream = torch.cuda.Stream()
            self.steps_done = torch.cuda.Event()
            self.seq_host = torch.empty((self.B, self.T), dtype=torch.long).pin_memory()
            self._pin_logp()
        else:
            for i in range(self.T):
                self._capture_step(i)
        self.reset()

    def _pin_logp(self) -> None:
        """(logprobs) the pinned host block logp_rows is copied to beside seq, under the event's one synchronise"""
        self.logp_host = torch.empty((self.B, self.T), dtype=torch.float32).pin_memory() if self.logprobs else None

    def _capture_step(self, i: int):
        """a graph of token step i alone (the step-by-step form; with the fused sampler only tests / debugging use it: the
        noise then comes from draw_noise())"""
        g = torch.cuda.CUDAGraph()
        if not self.fused_sampler:
            g.register_generator_state(self.gen)
        with torch.cuda.graph(g, pool=self._pool, capture_error_mode="thread_local"):
            self._tok_body(i, self.gen, draw=not self.fused_sampler)
        self.g_tok[i] = g

    # ---- driver interface ---------------------------------------------------------------------------------
    def reset(self):
        self.kv1.len = 0
        self.kv2.len = 0
        self.pos.zero_()
        if self.pos_limit is not None:
            self.pos_limit.zero_()
        if self.kvp is not None:
            self.kvp.len = 0
            self.pre_len.zero_()
        if self.kvs is not None:
            self.slot_len.zero_()
            self.row_slot.fill_(-1)
            self._reset_slots_host()
        if self.row_cache is not None:  # every row inactive
            self.row_cache.fill_(-1)
        if self.row_adapter is not None:  # no row names an adapter and every slot is empty: nothing outlives the session's user
            self.row_adapter.fill_(-1)
            for g in list(self._lora_loaded):
                self.unload_adapter(g)

    def load_adapter(self, slot: int, layers_net, layers_tok, scale: float) -> None:
        """(lora_slots) adapter slot ``slot`` <- one adapter: per stack a list over its layers of {target module: (A [r, in], B [out,
        r])} and the scale alpha / r.  Stream-ordered copies into the fixed buffers the captured graphs read, zero-padded for r < R
        and for targets the adapter lacks, then the norm fold of the A stacks.  ``ValueError`` before any copy: no such slot, a rank
        above R, an unknown target."""
        if self.lora1 is None:
            raise ValueError("DecodeSession.load_adapter: not a lora_slots session")
        self.lora1.check_slot(slot, layers_net)
        self.lora2.check_slot(slot, layers_tok)
        m = self.model
        self.lora1.load_slot(slot, layers_net, scale)
        self.lora2.load_slot(slot, layers_tok, scale)
        self.lora1.refresh(m._W["net"])
        self.lora2.refresh(m._W["net_token"])
        self._lora_loaded[slot] = (layers_net, float(scale))
        if self._merged_of == slot:
            self._merged_of = None

    def unload_adapter(self, slot: int) -> None:
        """(lora_slots) empty slot ``slot``: zeros in its blocks of the stacks, scale 0"""
        if self.lora1 is None or not 0 <= slot < self.lora_slots:
            raise ValueError(f"DecodeSession.unload_adapter: slot {slot!r}")
        self.load_adapter(slot, [{} for _ in self.lora1.a], [{} for _ in self.lora2.a], 0.0)
        del self._lora_loaded[slot]

    def _merged_weights(self, slot: int):
        """the event-level matrices with adapter ``slot`` merged, W + s B A per target by ops.gemm_nt as LoraAdapter.materialize
        does it, in a second copy of those matrices (allocated at the first adapted admission, re-materialised when the adapter
        or the base weights change)"""
        W = self.model._W["net"]
        if self._merged is None:
            self._merged = engine.StackTensors(embed=W.embed, norm=W.norm, layers=[
                engine.LayerTensors(wqkv=torch.empty_like(lw.wqkv), wo=torch.empty_like(lw.wo), wgu=torch.empty_like(lw.wgu),
                                    wd=torch.empty_like(lw.wd), n1=lw.n1, n2=lw.n2) for lw in W.layers])
        if self._merged_of != slot:
            layers, scale = self._lora_loaded[slot]
            names = {"qkv": "wqkv", "o": "wo", "gu": "wgu", "d": "wd"}
            for lw, lm, mods in zip(W.layers, self._merged.layers, layers):
                for nm in names.values():
                    getattr(lm, nm).copy_(getattr(lw, nm))
                for t, (A, Bm) in mods.items():
                    proj, part = engine.LORA_PROJ[t]
                    n = Bm.shape[0]
                    base, out = getattr(lw, names[proj])[part * n:(part + 1) * n], getattr(lm, names[proj])[part * n:(part + 1) * n]
                    ops.gemm_nt(Bm, A, out, K=A.shape[0], alpha=scale, beta=1.0, res=base, tb=True)
            self._merged_of = slot
        return self._merged

    def _reset_slots_host(self) -> None:
        """(prefix slots) the host's books: no row names a slot, every slot is empty and free"""
        self.row_slot_host = [-1] * self.B                 # row -> its slot
        self.slot_len_host = [0] * self.prefix_slots       # slot -> the length of its prompt
        self.slot_refs = [0] * self.prefix_slots           # slot -> rows that name it (running and held)

    def free_slots(self) -> List[int]:
        """(prefix slots) the slots no row names, ascending"""
        return [g for g, n in enumerate(self.slot_refs) if n == 0] if self.kvs is not None else []

    def prefill(self, tokens: torch.Tensor) -> None:
        """tokens [B, S, T]: causal forward over the prompt from an empty cache; leaves hidden = last position.
        A shared session runs ROW 0 alone (the caller has checked that the rows are equal) into ``kvp`` and hands its last hidden
        row to all B rows; the suffix cache starts empty."""
        if self.kv_dtype is not None or self.lookahead:
            raise ValueError("DecodeSession.prefill: an fp8-cache or lookahead session is filled by admit() alone")
        m = self.model
        spec = m._specs["net"]
        B, S, T = tokens.shape
        if self.kvp is not None:
            if S > self.shared_capacity:
                raise ValueError(f"prompt of {S} events in a session whose shared capacity is {self.shared_capacity}")
            e = torch.empty((S, spec.D), dtype=m.dtype, device=m.device)
            ops.embed_sum_fwd(tokens[0].contiguous().view(S, T), m._W["net"].embed, e)
            self.kvp.len = 0
            self.kv1.len = 0
            y = engine.stack_prefill(spec, m._W["net"], e, 1, S, self.rope1, self.kvp, folded=self.fold1)
            self.hidden.copy_(y[S - 1:S].expand(self.B, -1))
            self.pre_len.fill_(S)
            self.pos.fill_(S)
            return
        e = torch.empty((B * S, spec.D), dtype=m.dtype, device=m.device)
        ops.embed_sum_fwd(tokens.contiguous().view(B * S, T), m._W["net"].embed, e)
        self.kv1.len = 0
        y = engine.stack_prefill(spec, m._W["net"], e, B, S, self.rope1, self.kv1, folded=self.fold1)
        self.hidden.copy_(y.view(B, S, spec.D)[:, -1])
        self.pos.fill_(S)

    def set_limit(self, max_len) -> None:
        """(ragged) the position rows are parked at, for this call: cache row max_len must exist.  A row_params session also takes
        a sequence of B limits, row b parked at max_len[b]."""
        if isinstance(max_len, (int, np.integer)):
            if max_len + 1 > self.cap:
                raise ValueError(f"max_len {max_len} in a ragged session of capacity {self.cap} (max_len + 1 rows are needed)")
            self.pos_limit.fill_(int(max_len))
            return
        lim = [int(n) for n in max_len]
        if not self.row_params or len(lim) != self.B:
            raise ValueError(f"set_limit: {len(lim)} limits for a session of {self.B} rows (row_params: {self.row_params})")
        if max(lim) + 1 > self.cap:
            raise ValueError(f"max_len {max(lim)} in a ragged session of capacity {self.cap} (max_len + 1 rows are needed)")
        self.pos_limit.copy_(torch.tensor(lim, dtype=torch.int32))

    def set_row_params(self, temp, top_p, top_k) -> None:
        """(row_params) row b samples at temp[b], top_p[b], top_k[b] from now on: three B-element copies into the buffers the
        captured sampler reads.  The values are the caller's to validate (model._row_params does); a top_k outside
        [1, min(64, V)] is refused here as well, since this form has no sampler for it."""
        if not self.row_params:
            raise ValueError("set_row_params: not a row_params session")
        vals = [list(np.asarray(x).reshape(-1).tolist()) for x in (temp, top_p, top_k)]
        if any(len(v) != self.B for v in vals):
            raise ValueError(f"set_row_params: {[len(v) for v in vals]} values for a session of {self.B} rows")
        kmax = min(ops.SAMPLE_MAX_K, self.V)
        if any(int(k) != k or not 1 <= k <= kmax for k in vals[2]):
            raise ValueError(f"set_row_params: top_k {vals[2]} outside [1, {kmax}]")
        self.temp_rows.copy_(torch.tensor(vals[0], dtype=torch.float32))
        self.top_p_rows.copy_(torch.tensor(vals[1], dtype=torch.float32))
        self.top_k_rows.copy_(torch.tensor(vals[2], dtype=torch.int32))

    @staticmethod
    def _seed_values(seeds, n: int, what: str) -> list:
        """n Python ints in [0, 2^64) -> their int64 storage values (the same 64 bits); ValueError otherwise"""
        seeds = list(seeds) if seeds is not None else None
        if seeds is None or len(seeds) != n:
            raise ValueError(f"{what}: {'no' if seeds is None else len(seeds)} seeds for {n} rows")
        for s in seeds:
            if isinstance(s, bool) or not isinstance(s, (int, np.integer)) or not 0 <= int(s) < (1 << 64):
                raise ValueError(f"{what}: seed {s!r} is not an integer in [0, 2^64)")
        from .ops_seeded import seed_storage
        return seed_storage(seeds)

    def set_row_seeds(self, seeds) -> None:
        """(seeded) row b samples on seeds[b] from now on: one B-element copy into the buffer the captured sampler reads"""
        if not self.seeded:
            raise ValueError("set_row_seeds: not a seeded session")
        self.seed_rows.copy_(torch.tensor(self._seed_values(seeds, self.B, "set_row_seeds"), dtype=torch.int64))

    def prefill_ragged(self, tokens: torch.Tensor, lengths) -> None:
        """tokens [M, T]: the B prompts laid end to end, prompt b of lengths[b] events.  One packed causal forward from empty
        caches (engine.stack_prefill_seqs); leaves hidden[b] = prompt b's last position and pos[b] = lengths[b].  Prompts of one
        length take prefill()'s uniform forward instead, so that generate_ragged continues them exactly as generate() does."""
        if self.kv_dtype is not None or self.lookahead:
            raise ValueError("DecodeSession.prefill_ragged: an fp8-cache or lookahead session is filled by admit() alone")
        m = self.model
        spec = m._specs["net"]
        lengths = [int(n) for n in lengths]
        M, T = tokens.shape
        if not self.ragged or len(lengths) != self.B or min(lengths) < 1 or sum(lengths) != M:
            raise ValueError(f"prefill_ragged: {len(lengths)} lengths summing to {sum(lengths)} for {M} rows in a session of "
                             f"{self.B} rows (ragged: {self.ragged})")
        if max(lengths) >= self.cap:
            raise ValueError(f"prompt of {max(lengths)} events in a ragged session of capacity {self.cap}")
        if min(lengths) == max(lengths):
            # prompts of ONE length are a uniform batch: the forward prefill() runs (RoPE in the q|k|v epilogue, no table), so the
            # state handed to the decode steps is prefill()'s bit for bit -- the packed forward rotates the ROUNDED product in a
            # launch of its own and lands a bf16 rounding away (hidden by up to 7.8e-2 on tv2o-medium), enough to part sampled ids
            S = lengths[0]
            e = torch.empty((M, spec.D), dtype=m.dtype, device=m.device)
            ops.embed_sum_fwd(tokens.contiguous(), m._W["net"].embed, e)
            self.kv1.len = 0
            y = engine.stack_prefill(spec, m._W["net"], e, self.B, S, self.rope1, self.kv1, folded=self.fold1)
            self.kv1.len = 0  # (ragged: the rows' positions live in `pos` alone)
            self.hidden.copy_(y.view(self.B, S, spec.D)[:, -1])
            self.pos.fill_(S)
            return
        plan = ops.attn_seq_plan(lengths, spec.H).upload(m.device)
        e = torch.empty((M, spec.D), dtype=m.dtype, device=m.device)
        ops.embed_sum_fwd(tokens.contiguous(), m._W["net"].embed, e)
        y = engine.stack_prefill_seqs(spec, m._W["net"], e, plan, self.rope1, self.kv1, folded=self.fold1)
        self.hidden.copy_(y.index_select(0, plan.seq_start[1:].long() - 1))
        self.pos.copy_(plan.seq_start[1:] - plan.seq_start[:-1])

    def admit(self, rows, tokens: torch.Tensor, lengths, limits, temp, top_p, top_k, first_masks, bans, seeds=None,
              slots=None, adapter=None) -> None:
        """(row_params) n new requests into rows ``rows`` of the running batch, between two events (the header has the stream-order
        argument).  tokens [M, T]: the n prompts laid end to end, prompt s of lengths[s] events; limits[s]: the position row
        rows[s] is parked at (its max_len); temp / top_p / top_k: n values; first_masks / bans: uint8 [n, V] (host).  ONE packed
        forward over the admitted prompts alone -- always the packed form, also for one prompt or equal lengths, so that a
        request's prefill depends on its admission group through that forward's own shape dispatch and through nothing else --
        K/V into cache rows ``rows``, hidden[rows] = each prompt's last position, pos[rows] = lengths, and pos_limit, the sampler
        arrays and both masks of those rows overwritten.  The per-row values travel in ONE pinned host block and are scattered by
        eight index_copy_ calls (and one index_select for the last positions): no kernel of their own.  A seeded session takes
        ``seeds`` as well, n ints in [0, 2^64): one more int64 section of the block and a ninth index_copy_ into ``seed_rows``; an
        unseeded session refuses them.
        ``slots`` (a prefix_slots session; n distinct FREE slots, one per sequence -- an admission stores all of its prompts in
        slots or none, so that either cache takes the one packed store per layer): prompt s's K/V goes into slot slots[s]
        (mh_kv_store_seqs_rows over the slot cache, the slot ids as the row map) and NOT into cache row rows[s], whose own cache
        starts empty behind it; ``row_slot[rows]`` = slots and ``slot_len[slots]`` = lengths travel in the same block (two more
        index_copy_ calls).  Without ``slots`` such a session sets ``row_slot[rows]`` = -1.
        ``adapter`` (a lora_slots session; one loaded slot for the whole admission, or None): ``row_adapter[rows]`` = the slot (-1 for
        None) travels in the same block, and the prompts are prefilled against that adapter's MERGED event-level weights
        (``_merged_weights``; the unfolded forward) -- so the prompt's K/V come from W + s B A in bf16, which is how the reference
        serves an adapter, and the decoded events from the unmerged form.
        A lookahead session: ``rows`` are GROUP indices -- prompt s's K/V goes into cache sequence rows[s], the LEADER row
        rows[s] (k + 1) takes hidden, position and the settings, ``row_cache`` names the sequence for it, and the group's draft rows
        take a copy of the leader's settings and start inactive (``_spread_group``).
        Everything is checked on the host first; ``ValueError`` before any launch."""
        if not (self.ragged and self.row_params):
            raise ValueError("DecodeSession.admit: rows are admitted into a ragged=True, row_params=True session only")
        from .ops_pool import check_rows
        m = self.model
        spec = m._specs["net"]
        lengths, limits = [int(n) for n in lengths], [int(n) for n in limits]
        n, V = len(lengths), self.V
        ids = check_rows(rows, n, self.groups)   # (cache sequences: the rows themselves unless the session has groups)
        lead = [g * self.gw for g in ids] if self.lookahead else ids   # ... and the rows that take the state
        vals = [list(np.asarray(x).reshape(-1).tolist()) for x in (temp, top_p, top_k)]
        first_masks, bans = torch.as_tensor(first_masks), torch.as_tensor(bans)
        M, T = tokens.shape
        if n < 1 or min(lengths) < 1 or sum(lengths) != M or T != self.T or len(limits) != n or any(len(v) != n for v in vals):
            raise ValueError(f"admit: {n} lengths summing to {sum(lengths)} for {M} rows of {T} tokens, {len(limits)} limits, "
                             f"{[len(v) for v in vals]} sampler values")
        if any(L > lim or lim + 1 > self.cap for L, lim in zip(lengths, limits)):
            raise ValueError(f"admit: prompts of {lengths} events, limits {limits}, in a session of capacity {self.cap} (a prompt "
                             f"may not exceed its limit, and limit + 1 rows are needed)")
        kmax = min(ops.SAMPLE_MAX_K, V)
        if any(int(k) != k or not 1 <= k <= kmax for k in vals[2]):
            raise ValueError(f"admit: top_k {vals[2]} outside [1, {kmax}]")
        for name, t in (("first_masks", first_masks), ("bans", bans)):
            if t.dtype != torch.uint8 or t.shape != (n, V) or t.device.type != "cpu":
                raise ValueError(f"admit: {name} must be a host uint8 tensor [{n}, {V}]: {t.dtype} {tuple(t.shape)} on {t.device}")
        if self.seeded:
            seed_vals = self._seed_values(seeds, n, "admit")
        elif seeds is not None:
            raise ValueError("admit: seeds are taken by a seeded=True session only")
        if adapter is not None and (self.lora1 is None or isinstance(adapter, bool) or not isinstance(adapter, (int, np.integer))
                                    or adapter not in self._lora_loaded):
            raise ValueError(f"admit: adapter {adapter!r} -- a loaded slot of a lora_slots session (loaded: {sorted(self._lora_loaded)})")
        slot_ids = None
        if slots is not None:
            if self.kvs is None:
                raise ValueError("admit: slots are taken by a session with prefix slots only (prefix_slots=G, prefix_capacity=Pmax)")
            from .ops_share import check_slots
            slot_ids = check_slots(slots, n, self.prefix_slots)
            if any(self.slot_refs[g] for g in slot_ids):
                raise ValueError(f"admit: slots {[g for g in slot_ids if self.slot_refs[g]]} are in use")
            if max(lengths) > self.prefix_capacity:
                raise ValueError(f"admit: a prompt of {max(lengths)} events into a prefix slot of {self.prefix_capacity}")
        if self.kvs is not None and any(self.row_slot_host[r] >= 0 for r in ids):
            raise ValueError(f"admit: rows {[r for r in ids if self.row_slot_host[r] >= 0]} still name a prefix slot: release them first")
        # ---- the one host block: [idx i64 | last i64 | rows i32 | lengths i32 | limits i32 | top_k i32 | temp f32 | top_p f32 |
        #      first u8 | ban u8 (| seeds i64)], every section on a multiple of 16 bytes
        sections = [(np.int64, lead), (np.int64, np.cumsum(lengths) - 1), (np.int32, ids), (np.int32, lengths), (np.int32, limits),
                    (np.int32, vals[2]), (np.float32, vals[0]), (np.float32, vals[1]),
                    (np.uint8, first_masks.numpy().reshape(-1)), (np.uint8, bans.numpy().reshape(-1))]
        if self.seeded:
            sections.append((np.int64, seed_vals))
        if self.lora1 is not None:  # (| adapter i32)
            sections.append((np.int32, [-1 if adapter is None else int(adapter)] * n))
        if slot_ids is not None:  # (| slots i64 | slots i32), behind everything a session without slots stages
            sections += [(np.int64, slot_ids), (np.int32, slot_ids)]
        dev = m.device
        idx, last, rows_dev, len_dev, lim_dev, k_dev, t_dev, p_dev, first_dev, ban_dev, *more_dev = \
            self._stage_block(sections, "_admit_stage")
        seed_dev = more_dev[:1] if self.seeded else []
        # ---- one packed forward over the admitted prompts alone, K/V into the chosen cache rows
        plan = ops.attn_seq_plan(lengths, spec.H).upload(dev)
        e = torch.empty((M, spec.D), dtype=m.dtype, device=dev)
        ops.embed_sum_fwd(tokens.to(dev).contiguous(), m._W["net"].embed, e)
        Wp, foldp = (m._W["net"], self.fold1) if adapter is None else (self._merged_weights(int(adapter)), None)
        if slot_ids is not None:  # the prompts' K/V into their slots; the rows' own caches start empty behind them
            slot_idx, slots_dev = more_dev[-2:]
            y = engine.stack_prefill_seqs(spec, Wp, e, plan, self.rope1, self.kvs, folded=foldp, rows=slot_ids, rows_dev=slots_dev)
        else:
            y = engine.stack_prefill_seqs(spec, Wp, e, plan, self.rope1, self.kv1, folded=foldp, rows=ids, rows_dev=rows_dev)
        # ---- the rows' state
        self.hidden.index_copy_(0, idx, y.index_select(0, last))
        self.pos.index_copy_(0, idx, len_dev)
        self.pos_limit.index_copy_(0, idx, lim_dev)
        self.temp_rows.index_copy_(0, idx, t_dev)
        self.top_p_rows.index_copy_(0, idx, p_dev)
        self.top_k_rows.index_copy_(0, idx, k_dev)
        self.first_mask.index_copy_(0, idx, first_dev.view(n, V))
        self.ban.index_copy_(0, idx, ban_dev.view(n, V))
        if self.seeded:
            self.seed_rows.index_copy_(0, idx, seed_dev[0])
        if self.lora1 is not None:
            self.row_adapter.index_copy_(0, idx, more_dev[1 if self.seeded else 0])
        if slot_ids is not None:
            self.row_slot.index_copy_(0, idx, slots_dev)
            self.slot_len.index_copy_(0, slot_idx, len_dev)
            for r, g, L in zip(ids, slot_ids, lengths):
                self.row_slot_host[r], self.slot_len_host[g], self.slot_refs[g] = g, L, 1
        elif self.kvs is not None:
            self.row_slot.index_fill_(0, idx, -1)
        if self.lookahead:
            self.row_cache.index_copy_(0, idx, rows_dev)
            self._spread_group(ids)

    def _spread_group(self, groups) -> None:
        """(lookahead) the draft rows of ``groups`` <- their leader's limit, temperature, top-p, top-k, masks and seed; inactive
        (``row_cache`` = -1) at position 0.  Device-side row copies behind the scatter that wrote the leaders."""
        k, gw = self.lookahead, self.gw
        dev = self.model.device
        drafts = torch.tensor([g * gw + j for g in groups for j in range(1, gw)], dtype=torch.int64).to(dev)
        leads = torch.tensor([g * gw for g in groups for _ in range(k)], dtype=torch.int64).to(dev)
        for buf in (self.pos_limit, self.temp_rows, self.top_p_rows, self.top_k_rows, self.first_mask, self.ban, self.seed_rows):
            buf.index_copy_(0, drafts, buf.index_select(0, leads))
        self.pos.index_fill_(0, drafts, 0)
        self.row_cache.index_fill_(0, drafts, -1)

    def set_inputs(self, rows, events, positions, caches) -> None:
        """(lookahead) between the token steps and the net step: ``seq[rows]`` = events (int64 [n, T]: the event each row consumes),
        ``pos[rows]`` = positions and ``row_cache[rows]`` = caches (the row's group, or -1 for a row that sits the step out), in ONE
        pinned host block (``_stage_block``) and three index_copy_ calls.  The caller keeps two rows of one group off one position
        and every position inside the capacity (checked here on the host; ``ValueError`` before any copy)."""
        if not self.lookahead:
            raise ValueError("DecodeSession.set_inputs: not a lookahead session")
        from .ops_pool import check_rows
        ids = check_rows(rows, len(rows), self.B)
        n = len(ids)
        events = np.asarray(events, dtype=np.int64).reshape(n, self.T) if n else np.zeros((0, self.T), dtype=np.int64)
        positions, caches = [int(p) for p in positions], [int(c) for c in caches]
        if len(positions) != n or len(caches) != n:
            raise ValueError(f"set_inputs: {n} rows, {len(positions)} positions, {len(caches)} cache sequences")
        if not n:
            return
        for r, p, c in zip(ids, positions, caches):
            if c != -1 and (c != r // self.gw or not 0 <= p < self.cap):
                raise ValueError(f"set_inputs: row {r} at position {p} of cache sequence {c}: an active row belongs to its own group "
                                 f"({r // self.gw}) and stands inside the capacity {self.cap}")
        taken = [(c, p) for p, c in zip(positions, caches) if c != -1]
        if len(set(taken)) != len(taken):
            raise ValueError(f"set_inputs: two rows of one group at one position: {sorted(taken)}")
        if events.min() < 0 or events.max() >= self.V:
            raise ValueError(f"set_inputs: a token id outside [0, {self.V})")
        idx, ev_dev, pos_dev, cache_dev = self._stage_block(
            [(np.int64, ids), (np.int64, events.reshape(-1)), (np.int32, positions), (np.int32, caches)], "_look_stage")
        self.seq.index_copy_(0, idx, ev_dev.view(n, self.T))
        self.pos.index_copy_(0, idx, pos_dev)
        self.row_cache.index_copy_(0, idx, cache_dev)

    _STAGE_TYPES = {np.int64: torch.int64, np.int32: torch.int32, np.float32: torch.float32, np.uint8: torch.uint8}

    def _stage_block(self, sections, slot: str) -> list:
        """(admit, fork) ``sections`` [(numpy type, values)] laid into ONE host block, every section on a multiple of 16 bytes, and
        uploaded once; -> the sections as typed views of the device copy.  On a GPU the block is pinned and the copy non-blocking
        (as SeqPlan.upload); the pinned block is kept alive under ``slot`` until the next call that names it."""
        parts, offs, at = [], [], 0
        for ty, v in sections:
            a = np.ascontiguousarray(np.asarray(v, dtype=ty)).view(np.uint8)
            parts.append(a)
            offs.append((at, a.size))
            at += (a.size + 15) // 16 * 16
        host = np.zeros(at, dtype=np.uint8)
        for a, (o, sz) in zip(parts, offs):
            host[o:o + sz] = a
        block = torch.from_numpy(host)
        if self.model.device.type == "cuda":
            setattr(self, slot, block.pin_memory())
            block = getattr(self, slot).to(self.model.device, non_blocking=True)
        return [block[o:o + sz].view(self._STAGE_TYPES[ty]) for (ty, _), (o, sz) in zip(sections, offs)]

    def fork(self, src_rows, dst_rows, lengths, limits, temp, top_p, top_k, first_masks, bans, seeds=None, from_held=None,
             join=None) -> None:
        """(row_params) n rows of the running batch become continuations of other rows, between two events, WITHOUT a forward (the
        header has the stream-order argument).  For pair p: cache rows [0, lengths[p]) of every layer of sequence src_rows[p] are
        copied to sequence dst_rows[p] -- ONE mh_kv_fork_rows launch over the whole of ``kv1`` -- and row dst_rows[p] takes
        hidden[src_rows[p]] (``from_held[p]`` set: held_hidden[src_rows[p]], what ``hold`` kept), pos = lengths[p], pos_limit =
        limits[p], and the sampler arrays, both masks and, in a seeded session, the seed from the arguments (as ``admit`` takes
        them).  lengths[p] is the number of events whose K/V the source row holds: the caller's to know -- the session keeps no
        host copy of ``pos``.  Several pairs may name one source; the dst rows are distinct and no row stands on both sides.
        The per-row values travel in ONE pinned host block and are scattered by index_copy_ calls, as in ``admit``.  No forward,
        no capture, no recapture: every buffer sits at the address the graphs hold.
        ``join`` (a prefix_slots session; a bool per pair): dst_rows[p] JOINS the slot of src_rows[p] -- ``row_slot[dst]`` = the
        source's slot, one more reference to it -- and only the source's own cache rows [0, lengths[p] - pre), pre the slot's
        length, are copied: the launch covers the pairs with a row to copy, and when there is none it is not made.  A source that
        names a slot can only be forked with ``join``; a source that names none only without.
        ``ValueError`` before any launch."""
        if not (self.ragged and self.row_params):
            raise ValueError("DecodeSession.fork: rows are forked in a ragged=True, row_params=True session only")
        from .ops_fork import check_pairs
        V = self.V
        limits = [int(n) for n in limits]
        src, dst, lengths = check_pairs(src_rows, dst_rows, lengths, self.groups, self.cap)   # (lookahead: GROUP indices)
        n = len(src)
        gw = self.gw   # the rows that give and take the state: the groups' leaders (gw == 1: the rows themselves)
        vals = [list(np.asarray(x).reshape(-1).tolist()) for x in (temp, top_p, top_k)]
        first_masks, bans = torch.as_tensor(first_masks), torch.as_tensor(bans)
        if len(limits) != n or any(len(v) != n for v in vals):
            raise ValueError(f"fork: {n} pairs, {len(limits)} limits, {[len(v) for v in vals]} sampler values")
        if any(L > lim or lim + 1 > self.cap for L, lim in zip(lengths, limits)):
            raise ValueError(f"fork: rows of {lengths} events, limits {limits}, in a session of capacity {self.cap} (a row may not "
                             f"exceed its limit, and limit + 1 rows are needed)")
        kmax = min(ops.SAMPLE_MAX_K, V)
        if any(int(k) != k or not 1 <= k <= kmax for k in vals[2]):
            raise ValueError(f"fork: top_k {vals[2]} outside [1, {kmax}]")
        for name, t in (("first_masks", first_masks), ("bans", bans)):
            if t.dtype != torch.uint8 or t.shape != (n, V) or t.device.type != "cpu":
                raise ValueError(f"fork: {name} must be a host uint8 tensor [{n}, {V}]: {t.dtype} {tuple(t.shape)} on {t.device}")
        if self.seeded:
            seed_vals = self._seed_values(seeds, n, "fork")
        elif seeds is not None:
            raise ValueError("fork: seeds are taken by a seeded=True session only")
        held = [bool(x) for x in from_held] if from_held is not None else [False] * n
        if len(held) != n:
            raise ValueError(f"fork: from_held holds {len(held)} values for {n} pairs")
        if any(held) and self.held_hidden is None:
            raise ValueError("fork: from_held names a row, and hold() has kept none")
        copies = None  # (join) the pairs with rows of their own to copy, as (src, dst, rows); None: every pair, lengths[p] rows
        if join is not None or self.kvs is not None:
            joins = [bool(x) for x in join] if join is not None else [False] * n
            if len(joins) != n:
                raise ValueError(f"fork: join holds {len(joins)} values for {n} pairs")
            if any(joins) and self.kvs is None:
                raise ValueError("fork: join is taken by a session with prefix slots only")
            if self.kvs is not None:
                src_slot = [self.row_slot_host[s] for s in src]
                if any((g >= 0) != j for g, j in zip(src_slot, joins)):
                    raise ValueError(f"fork: sources {src} name the slots {src_slot} and join is {joins}: a child of a row that shares "
                                     "a prompt joins its slot, and no other child does")
                if any(self.row_slot_host[d] >= 0 for d in dst):
                    raise ValueError(f"fork: destination rows {[d for d in dst if self.row_slot_host[d] >= 0]} still name a prefix "
                                     "slot: release them first")
                pre = [self.slot_len_host[g] if g >= 0 else 0 for g in src_slot]
                if any(L < p for L, p in zip(lengths, pre)):
                    raise ValueError(f"fork: rows of {lengths} events behind prompts of {pre}")
                if any(joins):
                    copies = [(s, d, L - p) for s, d, L, p in zip(src, dst, lengths, pre) if L - p > 0]
        # ---- the one host block: [dst i64 | src i64 | src, dst, lengths i32 [3, n] | limits i32 | top_k i32 | temp f32 | top_p f32 |
        #      first u8 | ban u8 | held u8 (| seeds i64)]
        sections = [(np.int64, [d * gw for d in dst]), (np.int64, [s * gw for s in src]), (np.int32, src + dst + lengths),
                    (np.int32, limits), (np.int32, vals[2]),
                    (np.float32, vals[0]), (np.float32, vals[1]), (np.uint8, first_masks.numpy().reshape(-1)),
                    (np.uint8, bans.numpy().reshape(-1)), (np.uint8, held)]
        if self.seeded:
            sections.append((np.int64, seed_vals))
        if self.kvs is not None:  # (| slots i32 (| src, dst, rows i32 [3, m] of the pairs to copy)), behind the rest
            sections.append((np.int32, src_slot))
            if copies:
                sections.append((np.int32, [c[k] for k in range(3) for c in copies]))
        idx, from_idx, pairs, lim_dev, k_dev, t_dev, p_dev, first_dev, ban_dev, held_dev, *more_dev = \
            self._stage_block(sections, "_fork_stage")
        seed_dev = more_dev[:1] if self.seeded else []
        pairs = pairs.view(3, n)
        # ---- the K/V of every layer, one launch
        if self.kv_dtype is not None:  # (no prefix slots with it: every pair copies lengths[p] rows) codes and scale pairs
            ops.kv_fork_rows_fp8(self.kv1.k8, self.kv1.v8, self.kv1.sc, src, dst, lengths, dev=pairs)
        elif copies is None:
            ops.kv_fork_rows(self.kv1.k, self.kv1.v, src, dst, lengths, dev=pairs)
        elif copies:
            ops.kv_fork_rows(self.kv1.k, self.kv1.v, *([c[k] for c in copies] for k in range(3)),
                             dev=more_dev[-1].view(3, len(copies)))
        # ---- the rows' state
        h = self.hidden.index_select(0, from_idx)
        if any(held):
            h = torch.where(held_dev.bool()[:, None], self.held_hidden.index_select(0, from_idx), h)
        self.hidden.index_copy_(0, idx, h)
        self.pos.index_copy_(0, idx, pairs[2])
        self.pos_limit.index_copy_(0, idx, lim_dev)
        self.temp_rows.index_copy_(0, idx, t_dev)
        self.top_p_rows.index_copy_(0, idx, p_dev)
        self.top_k_rows.index_copy_(0, idx, k_dev)
        self.first_mask.index_copy_(0, idx, first_dev.view(n, V))
        self.ban.index_copy_(0, idx, ban_dev.view(n, V))
        if self.seeded:
            self.seed_rows.index_copy_(0, idx, seed_dev[0])
        if self.row_adapter is not None:  # a child keeps its parent's adapter: its K/V were computed under it
            self.row_adapter.index_copy_(0, idx, self.row_adapter.index_select(0, from_idx))
        if self.kvs is not None:
            self.row_slot.index_copy_(0, idx, more_dev[1 if self.seeded else 0])
        if self.lookahead:  # the destination groups: the leader on its own cache sequence, the draft rows inactive on its settings
            self.row_cache.index_copy_(0, idx, pairs[1])
            self._spread_group(dst)
        if self.kvs is not None:
            for d, g in zip(dst, src_slot):
                self.row_slot_host[d] = g
                if g >= 0:
                    self.slot_refs[g] += 1

    def hold(self, rows) -> None:
        """(row_params) keep ``hidden[rows]`` -- the net output over those rows' LAST event -- in ``held_hidden`` [B, D] (allocated
        at first use) at the same row indices.  A parked row keeps being sampled and the next net step overwrites its ``hidden``;
        its K/V rows [0, max_len) stay as they are (a parked row writes cache row max_len alone), so the copy is all that a later
        ``fork(..., from_held=...)`` needs to continue the row.  Call it behind the net step over the row's last event."""
        if not (self.ragged and self.row_params):
            raise ValueError("DecodeSession.hold: rows are held on a ragged=True, row_params=True session only")
        from .ops_pool import check_rows
        ids = [g * self.gw for g in check_rows(rows, len(rows), self.groups)]   # (lookahead: groups -> their leaders)
        if not ids:
            return
        if self.held_hidden is None:
            self.held_hidden = torch.zeros_like(self.hidden)
        idx = torch.tensor(ids, dtype=torch.int64).to(self.model.device)
        self.held_hidden.index_copy_(0, idx, self.hidden.index_select(0, idx))

    def release(self, rows) -> None:
        """(row_params) rows whose requests have finished: pos = pos_limit = 0 there.  A free row is still embedded, attended and
        sampled with the rest of the batch, but it now attends to ONE key (the row it overwrites at position 0) instead of
        dragging a finished request's whole cache through the attention kernel; what it samples is the caller's to drop.
        A prefix_slots session: ``row_slot`` = -1 there as well, and a slot whose last row leaves is emptied (``slot_len`` = 0, on
        the same stream) and free again."""
        if not (self.ragged and self.row_params):
            raise ValueError("DecodeSession.release: rows are released on a ragged=True, row_params=True session only")
        from .ops_pool import check_rows
        ids = check_rows(rows, len(rows), self.groups)
        if not ids:
            return
        if self.lookahead:  # groups: every row of them, and all of them inactive
            ids = [g * self.gw + j for g in ids for j in range(self.gw)]
        idx = torch.tensor(ids, dtype=torch.int64).to(self.model.device)
        self.pos.index_fill_(0, idx, 0)
        self.pos_limit.index_fill_(0, idx, 0)
        if self.row_cache is not None:
            self.row_cache.index_fill_(0, idx, -1)
        if self.row_adapter is not None:
            self.row_adapter.index_fill_(0, idx, -1)
        if self.kvs is not None:
            self.row_slot.index_fill_(0, idx, -1)
            emptied = []
            for r in ids:
                g, self.row_slot_host[r] = self.row_slot_host[r], -1
                if g >= 0:
                    self.slot_refs[g] -= 1
                    if self.slot_refs[g] == 0:
                        self.slot_len_host[g] = 0
                        emptied.append(g)
            if emptied:
                self.slot_len.index_fill_(0, torch.tensor(emptied, dtype=torch.int64).to(self.model.device), 0)

    def begin(self, generator) -> None:
        """take over the caller's random stream (None = the device's default generator).  A seeded session has no generator of its
        own (``gen is None``) and takes none: here and in ``end`` nothing reads or writes a generator's state."""
        if self.seeded and generator is not None:
            raise ValueError("DecodeSession.begin: a seeded session draws nothing from a generator")
        self._user_gen = generator
        self._noise_pending = False
        self._noise_read = False
        if self.gen is not None:
            src = generator if generator is not None else torch.cuda.default_generators[self.model.device.index or 0]
            with _CAPTURE_LOCK:
                self.gen.set_state(src.get_state())
                self._off = self.gen.get_offset()

    def end(self) -> None:
        """hand the advanced random stream back to the caller's generator"""
        if self.g_noise is not None:
            if self._noise_pending:  # draws made ahead for an event that was never sampled: not consumed
                self.noise_stream.synchronize()
                self._noise_pending = False
            with _CAPTURE_LOCK:
                self.gen.set_offset(self._off)
        if self.gen is not None:
            dst = self._user_gen if self._user_gen is not None else torch.cuda.default_generators[self.model.device.index or 0]
            with _CAPTURE_LOCK:
                dst.set_state(self.gen.get_state())
        self._user_gen = None

    def net_step(self) -> None:
        """decode the event in ``seq`` (the one just sampled) at the next position; hidden <- net output"""
        if self.g_net is not None:
            self.g_net.replay()
        else:
            self._net_body()
        if not self.ragged:  # (ragged: the rows' positions live in `pos` alone)
            self.kv1.len += 1

    def tok_step(self, i: int) -> None:
        """sample token position i of the current event into seq[:, i] (and ev for i == 0) -- the step-by-step form.
        With the fused sampler the step READS the event's Exp(1) variates instead of drawing them: they come from
        draw_noise() (called here for position 0 when the caller has not done so -- without it the step would sample against
        stale variates and leave the generator where it was), and the caller reports the draws the reference loop would have
        made with consumed(n_steps) once the event is complete (sample_event() does both)."""
        if self.use_graphs:
            if self.g_tok[i] is None:
                with _CAPTURE_LOCK:
                    self._capture_step(i)
            if self.g_noise is not None and i == 0:
                if self._noise_pending and self._noise_read:
                    # the pending variates were already read by an earlier event's steps and never reported with consumed():
                    # sampling against them again would repeat that event's draws and leave the generator where it was
                    raise RuntimeError("DecodeSession.tok_step(0): the previous event's draws were not reported -- call "
                                       "consumed(n_steps) after the last tok_step of an event (sample_event() does both)")
                if not self._noise_pending:
                    self.draw_noise()
            if self.g_noise is not None:
                self._noise_read = True
            if self.g_noise is not None and self._noise_pending:
                torch.cuda.current_stream().wait_event(self.noise_done)
            if self.fused_sampler:
                self.g_tok[i].replay()
            else:  # (the step graph of the unfused sampler carries the generator state)
                with _CAPTURE_LOCK:
                    self.g_tok[i].replay()
            self._steps_recorded = False
        else:
            self._tok_body(i, self._user_gen)

    # ---- one event per call: the form generate() drives ----------------------------------------------------
    def draw_noise(self) -> None:
        """(fused graphs) draw the next event's T x [B, V] variates on the noise stream, starting at the offset the reference
        loop would be at; they overlap whatever the caller queues next on its own stream (the net step)"""
        if self.g_noise is None:
            return
        # the token steps that read the previous draws must be done first: the event recorded right behind the steps graph
        # when there is one (NOT the whole stream: the net step queued after it is what the draws should overlap)
        if _NOISE_INLINE:
            pass
        elif self._steps_recorded:
            self.noise_stream.wait_event(self.steps_done)
        else:
            self.noise_stream.wait_stream(torch.cuda.current_stream())
        self._noise_read = False
        if _NOISE_INLINE:  # (A/B: the draws on the caller's stream, no cross-stream dependency)
            with _CAPTURE_LOCK:  # (generator-state calls assert "not capturing" as well)
                self.gen.set_offset(self._off)
                self.g_noise.replay()
            self.noise_done.record(torch.cuda.current_stream())
        else:
            with torch.cuda.stream(self.noise_stream):
                with _CAPTURE_LOCK:
                    self.gen.set_offset(self._off)
                    self.g_noise.replay()
                self.noise_done.record(self.noise_stream)
        self._noise_pending = True

    def consumed(self, n_steps: int) -> None:
        """the reference loop ran n_steps sampling calls for the event just sampled: its generator stands n_steps draws on"""
        if self.g_noise is not None:
            self._off += n_steps * self._draw_inc
            self._noise_pending = False
            self._noise_read = False

    def n_steps_of(self, ids) -> tuple:
        """(number of sampling calls the reference makes for an event whose first tokens are `ids`, all rows ended?) --
        the break rule of midi_model.py:232-235: the inner loop stops after position i iff every live row's event has
        exactly i parameters (vacuously true at i == 1 when no row is live)"""
        tok = self.model.tokenizer
        arity = self.model._grammar()[3]
        alive = [arity[t] for t in ids if t != tok.eos_id]
        if not alive:
            return 2, True
        return (alive[0] + 1 if all(a == alive[0] for a in alive) else self.T), False

    @staticmethod
    def _live_ids(ids, live):
        return ids if live is None else [t for t, on in zip(ids, live) if on]

    def sample_event(self, then_net: bool = False, live=None):
        """sample the T tokens of the next event from `hidden`; -> (np.ndarray [B, T] int64, all rows ended?).
        ``live`` (ragged; a bool per row): the break rule and "all rows ended" are evaluated over these rows only -- the others
        are retired, sampled all the same, and the caller drops their tokens.
        ``then_net`` (graph form): the net step over the sampled event is queued right behind the token steps, BEFORE the host
        waits for the tokens -- it depends on nothing the host decides -- so the device never idles through the host's
        round trip; the tokens come back through a copy stream that waits for the token steps only.  (If every row turns out
        to have ended, that net step was wasted work on a session about to be reset.)"""
        if self.g_steps is not None:
            if not self._noise_pending:
                self.draw_noise()
            cur = torch.cuda.current_stream()
            if self.g_noise is not None:  # (a seeded session has no noise to wait for)
                cur.wait_event(self.noise_done)
            self.g_steps.replay()
            self.steps_done.record(cur)
            self._steps_recorded = True
            if then_net:
                self.net_step()
                self.copy_stream.wait_event(self.steps_done)
                with torch.cuda.stream(self.copy_stream):
                    if _COPY_PAGEABLE:  # (A/B: a blocking pageable copy on the copy stream instead of pinned + stream sync)
                        event = self.seq.cpu().numpy().copy()
                        if self.logprobs:
                            self.last_logp = self.logp_rows.cpu().numpy().copy()
                    else:
                        self.seq_host.copy_(self.seq, non_blocking=True)
                        if self.logprobs:  # beside seq on the copy stream: the same one synchronise covers both
                            self.logp_host.copy_(self.logp_rows, non_blocking=True)
                if not _COPY_PAGEABLE:
                    self.copy_stream.synchronize()  # the one host sync per event
                    event = self.seq_host.numpy().copy()
                    if self.logprobs:
                        self.last_logp = self.logp_host.numpy().copy()
            else:
                event = self.seq.cpu().numpy().copy()  # the one host sync per event
                if self.logprobs:
                    self.last_logp = self.logp_rows.cpu().numpy().copy()
            n, end_all = self.n_steps_of(self._live_ids(event[:, 0].tolist(), live))
            self.consumed(n)
            return event, end_all
        n_steps, end_all, i = self.T, False, 0
        while i < n_steps:
            self.tok_step(i)  # ... lm_head -> masked softmax -> sample_top_p_k -> seq[:, i]
            if i == 0:
                n_steps, end_all = self.n_steps_of(self._live_ids(self.ev.tolist(), live))  # (a host sync)
            i += 1
        if self.logprobs:  # (step-by-step form: positions the break rule skipped keep what an earlier event left there)
            self.last_logp = self.logp_rows.cpu().numpy().copy()
        return self.seq.cpu().numpy().copy(), end_all  # (a CPU tensor would share memory with the session buffer)
