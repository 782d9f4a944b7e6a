"""``MIDIModel`` with the reference's surface (midi_model.py:99-250) on the HIP kernels.

Same constructor, attributes (``tokenizer, net, net_token, lm_head, config, device, dtype``), the same
140 parameter names/shapes (so ``state_dict`` / ``load_state_dict`` / ``.to()`` interoperate with
reference checkpoints), and the same methods: ``forward``, ``forward_token``, ``sample_top_p_k``,
``generate``.  Underneath, all parameters live in ONE flat buffer (q|k|v and gate|up adjacent, so each pair
is one projection; gradients mirror the layout so the data-parallel reducer and the fused AdamW work on
contiguous ranges), and every tensor op is a launch from ``engine.py`` / ``ops.py``.

There is no CPU implementation: calling the compute methods without a ROCm device raises.
"""
from __future__ import annotations

import json
import math
import os
import threading
from typing import List, Optional, Tuple

import numpy as np
import torch
import torch.nn as nn

from . import engine, ops
from .config import MIDIModelConfig, NetConfig
from .engine import KVState, LayerTensors, RopeTable, StackSpec, StackTensors


# MH_DECODE_SPEC=1: queue the net step of an event BEFORE the host has read its tokens (decode.DecodeSession.sample_event,
# tokens through a copy stream).  Measured slower on the MI355X, same box, interleaved (r02, tools/gpu_r2_13.sh): 1.86 ms per
# event against 1.70 with the plain order (token steps -> host copy -> noise graph + net step), pinned or pageable copy
# alike -- the host's ~40 us round trip is cheaper than what the extra queue traffic costs the dependent chain.  Off.
_SPECULATIVE_NET = os.environ.get("MH_DECODE_SPEC", "0") == "1"


class _SessionPool:
    """Idle decode sessions of one model (buffers + captured graphs).  Copies and pickles of the model start empty."""

    def __init__(self):
        self.lock = threading.Lock()
        self.idle = []

    def __deepcopy__(self, memo):
        return _SessionPool()

    def __reduce__(self):
        return (_SessionPool, ())


class _W(nn.Module):
    """A module that owns one ``weight`` (stands in for nn.Linear / nn.Embedding / RMSNorm in the key tree)."""

    def __init__(self, *shape: int):
        super().__init__()
        self.weight = nn.Parameter(torch.empty(*shape))


class _Attn(nn.Module):
    def __init__(self, D: int):
        super().__init__()
        self.q_proj, self.k_proj, self.v_proj, self.o_proj = _W(D, D), _W(D, D), _W(D, D), _W(D, D)


class _MLP(nn.Module):
    def __init__(self, D: int, I: int):
        super().__init__()
        self.gate_proj, self.up_proj, self.down_proj = _W(I, D), _W(I, D), _W(D, I)


class _Layer(nn.Module):
    def __init__(self, D: int, I: int):
        super().__init__()
        self.self_attn = _Attn(D)
        self.mlp = _MLP(D, I)
        self.input_layernorm = _W(D)
        self.post_attention_layernorm = _W(D)


class _Stack(nn.Module):
    def __init__(self, cfg: NetConfig):
        super().__init__()
        self.config = cfg
        D, I = cfg.hidden_size, cfg.intermediate_size
        self.embed_tokens = _W(cfg.vocab_size, D)
        self.layers = nn.ModuleList([_Layer(D, I) for _ in range(cfg.num_hidden_layers)])
        self.norm = _W(D)


_MATS = ("self_attn.q_proj", "self_attn.k_proj", "self_attn.v_proj", "self_attn.o_proj",
         "mlp.gate_proj", "mlp.up_proj", "mlp.down_proj")


class MIDIModel(nn.Module):
    config_class = MIDIModelConfig

    def __init__(self, config: MIDIModelConfig, *args, **kwargs):
        super().__init__()
        self.config = config
        self.tokenizer = config.tokenizer
        self.net = _Stack(config.net_config)
        self.net_token = _Stack(config.net_token_config)
        self.lm_head = _W(self.tokenizer.vocab_size, config.n_embd)
        self._specs = {
            "net": self._spec("net", config.net_config, "event"),
            "net_token": self._spec("net_token", config.net_token_config, "token"),
        }
        self._flat = None
        self._flat_grad = None
        self._ropes = {}
        self._tables = None
        self._sessions = _SessionPool()  # idle decode sessions (decode.py)
        self._weights_epoch = 0          # bumped by every writer that bypasses torch's version counters (weights_written)
        self._fold_cache = {}            # stack name -> (key, folded weights): folded_weights()
        self._reset_parameters()
        self._repack()

    # ------------------------------------------------------------------------------------------ set-up
    @staticmethod
    def _spec(name: str, c: NetConfig, kind: str) -> StackSpec:
        return StackSpec(name, c.hidden_size, c.num_attention_heads, c.intermediate_size, c.num_hidden_layers,
                         float(c.rms_norm_eps), float(c.rope_theta), kind)

    def _reset_parameters(self):
        """HF LLaMA init for the two stacks (N(0, 0.02), pad row zero, norms one; modeling_llama post_init) and
        torch's default nn.Linear init for lm_head (the reference never calls post_init on MIDIModel itself)."""
        with torch.no_grad():
            for st in (self.net, self.net_token):
                for n, p in st.named_parameters():
                    if p.dim() == 1:
                        p.fill_(1.0)
                    else:
                        p.normal_(0.0, 0.02)
                pad = st.config.pad_token_id
                if pad is not None:
                    st.embed_tokens.weight[pad].zero_()
            bound = 1.0 / math.sqrt(self.lm_head.weight.shape[1])
            self.lm_head.weight.uniform_(-bound, bound)

    def _layout(self) -> List[Tuple[str, nn.Parameter, str]]:
        """Flat order: all matrices in forward order, then all norm vectors (the no-weight-decay group)."""
        named = dict(self.named_parameters())
        mats, norms = [], []
        for pre, st in (("net", self.net), ("net_token", self.net_token)):
            mats.append(f"{pre}.embed_tokens.weight")
            for i in range(len(st.layers)):
                mats += [f"{pre}.layers.{i}.{m}.weight" for m in _MATS]
                norms += [f"{pre}.layers.{i}.input_layernorm.weight", f"{pre}.layers.{i}.post_attention_layernorm.weight"]
            norms.append(f"{pre}.norm.weight")
        mats.append("lm_head.weight")
        assert len(mats) + len(norms) == len(named)
        return [(n, named[n], "mat") for n in mats] + [(n, named[n], "norm") for n in norms]

    def _repack(self):
        """(Re)build the flat parameter buffer on the parameters' current device/dtype and re-point every
        Parameter at its slice.  Runs after construction and after every ``.to()/.cuda()/.bfloat16()``."""
        layout = self._layout()
        p0 = layout[0][1]
        total = sum(p.numel() for _, p, _ in layout)
        flat = torch.empty(total, dtype=p0.dtype, device=p0.device)
        off = 0
        self._offsets = {}
        with torch.no_grad():
            for name, p, grp in layout:
                n = p.numel()
                assert off % 8 == 0, "every tensor must start 16-byte aligned"
                flat[off:off + n].copy_(p.detach().reshape(-1).to(flat.dtype))
                p.data = flat[off:off + n].view(p.shape)
                p.grad = None
                self._offsets[name] = (off, n, grp)
                off += n
        self._flat = flat
        self._n_mat = sum(n for (_, n, g) in self._offsets.values() if g == "mat")
        self._flat_grad = None
        self._ropes = {}
        self._tables = None
        self._sessions = _SessionPool()  # idle decode sessions (decode.py)
        self._W = {k: self._stack_views(k, flat) for k in ("net", "net_token")}
        self._fold_cache = {}
        self._weights_epoch = getattr(self, "_weights_epoch", 0) + 1

    # --------------------------------------------------------------------- derived data of the weights
    def weights_written(self) -> None:
        """Tell the model that its flat parameter buffer was written through a raw pointer (mh_adamw, a LoRA materialisation, a
        broadcast): torch's version counters do not see those writes, the caches of data DERIVED from the weights
        (folded_weights) are keyed on this epoch as well."""
        self._weights_epoch += 1

    def folded_weights(self, pre: str = "net"):
        """engine.fold_norm_weights of stack ``pre`` -- [(wqkv * n1, wgu * n2) per layer], the weights the forward-only blocks with
        folded RMSNorms multiply by (engine.layer_forward_folded) -- kept on the model and re-derived lazily, in place, when a
        parameter changed: keyed on the parameters' version counters (torch-side in-place writes: load_state_dict, an optimizer
        from torch.optim, ``p.mul_()`` under no_grad) and on the epoch raw-pointer writers bump (weights_written; a write through
        ``p.data`` is such a writer too -- torch does not count it).  So the public
        ``forward`` under no_grad reaches the folded blocks from 8192 rows up without paying the fold per call (~0.7 ms of
        elementwise launches for tv2o-medium).  277 MB for tv2o-medium in bf16."""
        st = getattr(self, pre)
        versions = tuple(p._version for lyr in st.layers for p in lyr.parameters())
        key = (self._weights_epoch, self._flat.data_ptr(), versions)
        hit = self._fold_cache.get(pre)
        if hit is not None and hit[0] == key:
            return hit[1]
        with self._sessions.lock:  # (app.py:496 runs up to ten generators on one model: one of them derives, the others wait)
            hit = self._fold_cache.get(pre)
            if hit is None or hit[0] != key:
                with torch.no_grad():
                    folded = engine.fold_norm_weights(self._W[pre], out=hit[1] if hit is not None else None)
                self._fold_cache[pre] = hit = (key, folded)
        return hit[1]

    def _apply(self, fn, recurse=True):
        out = super()._apply(fn, recurse)
        if getattr(self, "_flat", None) is not None or hasattr(self, "_offsets"):
            self._repack()
        return out

    def _stack_views(self, pre: str, flat: torch.Tensor) -> StackTensors:
        spec = self._specs[pre]
        D, I = spec.D, spec.I

        def view(name, rows, cols=None):
            off, _, _ = self._offsets[name]
            n = rows * (cols or 1)
            t = flat[off:off + n]
            return t.view(rows, cols) if cols else t

        V = self.tokenizer.vocab_size
        st = StackTensors(embed=view(f"{pre}.embed_tokens.weight", V, D), norm=view(f"{pre}.norm.weight", D))
        for i in range(spec.L):
            b = f"{pre}.layers.{i}."
            st.layers.append(LayerTensors(
                wqkv=view(b + "self_attn.q_proj.weight", 3 * D, D), wo=view(b + "self_attn.o_proj.weight", D, D),
                wgu=view(b + "mlp.gate_proj.weight", 2 * I, D), wd=view(b + "mlp.down_proj.weight", D, I),
                n1=view(b + "input_layernorm.weight", D), n2=view(b + "post_attention_layernorm.weight", D)))
        return st

    # ------------------------------------------------------------------------------------- properties
    @property
    def device(self) -> torch.device:
        return self._flat.device

    @property
    def dtype(self) -> torch.dtype:
        return self._flat.dtype

    @property
    def vocab_padded(self) -> int:
        return ops.round_up(self.tokenizer.vocab_size, 64)

    def _require_gpu(self):
        if self._flat.device.type != "cuda":
            raise RuntimeError("MIDIModel compute needs a ROCm device: move the model with .to('cuda'). "
                               "This implementation has no CPU path (the reference's CPU path is the oracle's job).")
        if self._flat.dtype not in (torch.float32, torch.bfloat16):
            raise RuntimeError(f"unsupported parameter dtype {self._flat.dtype} (float32 or bfloat16)")

    def _check_ids(self, ids: torch.Tensor) -> None:
        """Token ids still on the host are range-checked for free; ids already on the device are checked by the embedding
        kernels themselves (an id outside [0, vocab) traps the kernel, as torch's embedding raises a device assert)."""
        if not ids.is_cuda and ids.numel():
            lo, hi = int(ids.min()), int(ids.max())
            if lo < 0 or hi >= self.tokenizer.vocab_size:
                raise IndexError(f"token ids outside [0, {self.tokenizer.vocab_size}): min {lo}, max {hi}")

    def rope(self, pre: str) -> RopeTable:
        if pre not in self._ropes:
            spec = self._specs[pre]
            self._ropes[pre] = RopeTable(spec.hd, spec.theta, self.device)
        return self._ropes[pre]

    # ---------------------------------------------------------------- gradients + transposed weights
    def grad_buffer(self) -> torch.Tensor:
        """Flat gradient buffer mirroring the parameter layout; every p.grad is a view of it."""
        if self._flat_grad is None:
            self._flat_grad = torch.zeros_like(self._flat)
            for name, p in self.named_parameters():
                off, n, _ = self._offsets[name]
                p.grad = self._flat_grad[off:off + n].view(p.shape)
            self._G = {k: self._stack_views(k, self._flat_grad) for k in ("net", "net_token")}
            off, n, _ = self._offsets["lm_head.weight"]
            self._g_lm = self._flat_grad[off:off + n].view(self.lm_head.weight.shape)
        return self._flat_grad

    # ------------------------------------------------------------------------------ reference methods
    def load_merge_lora(self, model_id):
        """midi_model.py:109-114 without peft: read a saved LoRA adapter (``adapter_config.json`` +
        ``adapter_model.safetensors`` / ``.bin`` in the directory ``model_id``) and merge it into the weights in place,
        W += scale * B @ A with scale = lora_alpha / r (or / sqrt(r) for rsLoRA), which is what
        ``LoraModel.merge_and_unload`` computes for ``nn.Linear`` targets (train.py:439-449 trains r=64, alpha=128 on
        q,k,v,o,gate,up,down).  Returns self.  The merge is a pure weight transform; nothing else changes."""
        cfg_path = os.path.join(model_id, "adapter_config.json")
        if not os.path.isdir(model_id) or not os.path.exists(cfg_path):
            raise FileNotFoundError(f"{model_id}: not a local LoRA adapter directory (hub ids need network access)")
        with open(cfg_path) as f:
            cfg = json.load(f)
        if cfg.get("peft_type", "LORA") != "LORA":
            raise ValueError(f"unsupported peft_type {cfg.get('peft_type')}")
        r, alpha = int(cfg["r"]), float(cfg.get("lora_alpha", cfg["r"]))
        scale = alpha / math.sqrt(r) if cfg.get("use_rslora") else alpha / r
        st_path = os.path.join(model_id, "adapter_model.safetensors")
        if os.path.exists(st_path):
            from safetensors.torch import load_file
            sd = load_file(st_path)
        else:
            sd = torch.load(os.path.join(model_id, "adapter_model.bin"), map_location="cpu")
        params = dict(self.named_parameters())
        merged = 0
        with torch.no_grad():
            for key, a in sd.items():
                if not key.endswith("lora_A.weight"):
                    continue
                stem = key[: -len(".lora_A.weight")]
                b = sd[stem + ".lora_B.weight"]
                name = stem
                for prefix in ("base_model.model.", "base_model."):
                    if name.startswith(prefix):
                        name = name[len(prefix):]
                        break
                w = params.get(name + ".weight")
                if w is None:
                    raise KeyError(f"adapter targets {name}.weight, which this model does not have")
                delta = (b.float() @ a.float()) * scale  # [out, r] @ [r, in]
                if cfg.get("fan_in_fan_out"):
                    delta = delta.t()
                if delta.shape != w.shape:
                    raise ValueError(f"{name}: adapter delta {tuple(delta.shape)} vs weight {tuple(w.shape)}")
                w.add_(delta.to(device=w.device, dtype=w.dtype))
                merged += 1
        if merged == 0:
            raise ValueError(f"{model_id}: no lora_A/lora_B pairs found")
        return self

    def forward(self, x: torch.Tensor, cache=None) -> torch.Tensor:
        """x (B, S, 8) int64 -> hidden (B, S, n_embd)   [midi_model.py:137-150]

        Without ``cache`` the call is differentiable (an autograd node that runs the explicit backward
        schedule).  With ``cache`` (any object; HF DynamicCache instances are accepted) K/V go to
        preallocated buffers attached to it: an empty cache is prefilled causally, afterwards one event per
        call is decoded, or a chunk of S > 1 events is appended in one pass (``engine.stack_extend``)."""
        self._require_gpu()
        if x.dim() != 3:
            raise ValueError(f"expected (batch, events, tokens) ids, got shape {tuple(x.shape)}")
        B, S, T = x.shape
        self._check_ids(x)
        x = x.to(device=self.device, dtype=torch.long).contiguous()
        if cache is None:
            if not torch.is_grad_enabled():
                # nothing will backpropagate (validation, app.py's no_grad calls): the forward-only schedule -- no activations kept,
                # gate|up never written, and for enough rows the folded-norm blocks.  (Inside an autograd.Function the grad mode is
                # always off and needs_input_grad still reports the parameters' flags, so the decision is taken here.)
                spec = self._specs["net"]
                e = torch.empty((B * S, spec.D), dtype=self.dtype, device=self.device)
                ops.embed_sum_fwd(x.view(B * S, T), self._W["net"].embed, e)
                y, _ = engine.stack_forward(spec, self._W["net"], e, B, S, self.rope("net"), save=False,
                                            folded=self._folded_for(spec, e))
                return y.view(B, S, spec.D)
            from .autograd import NetFn
            params = self._stack_params("net")
            return NetFn.apply(self, x, *params)
        spec = self._specs["net"]
        st = getattr(cache, "_mh_state", None)
        with torch.no_grad():
            e = torch.empty((B * S, spec.D), dtype=self.dtype, device=self.device)
            ops.embed_sum_fwd(x.view(B * S, T), self._W["net"].embed, e)
            if st is None or st.len == 0:
                if st is None:
                    st = KVState(spec, B, max(ops.round_up(S + 64, 64), 256), e)
                    cache._mh_state = st
                y = engine.stack_prefill(spec, self._W["net"], e, B, S, self.rope("net"), st, folded=self._folded_for(spec, e))
                return y.view(B, S, spec.D)
            if st.B != B:
                raise ValueError(f"cache was built for batch {st.B}, got {B}")
            if S == 1:  # one event per call: the decode step
                return engine.stack_decode(spec, self._W["net"], e, self.rope("net"), st).view(B, 1, spec.D)
            # chunked continuation: the S new events attend to the cached ones and causally to each other
            return engine.stack_extend(spec, self._W["net"], e, B, S, self.rope("net"), st).view(B, S, spec.D)

    def _folded_for(self, spec, e: torch.Tensor):
        """the kept folded weights when a forward-only pass over ``e`` [rows, D] will run the folded-norm blocks, else None"""
        return self.folded_weights(spec.name) if engine.runs_folded(spec, e, False, None, True) else None

    def forward_token(self, hidden_state=None, x=None, cache=None) -> torch.Tensor:
        """hidden_state (N, n_embd) and/or x (N, t) int64 -> logits (N, [1]+t, vocab)   [midi_model.py:116-135]"""
        self._require_gpu()
        if hidden_state is None and x is None:
            raise ValueError("forward_token needs hidden_state and/or x")
        if x is not None:
            self._check_ids(x)
            x = x.to(device=self.device, dtype=torch.long)
        if cache is None:
            from .autograd import TokFn
            params = self._stack_params("net_token") + [self.lm_head.weight]
            return TokFn.apply(self, hidden_state, x, *params)
        spec = self._specs["net_token"]
        st = getattr(cache, "_mh_state", None)
        V, Vp = self.tokenizer.vocab_size, self.vocab_padded
        with torch.no_grad():
            rows = []
            N = (hidden_state if hidden_state is not None else x).shape[0]
            if hidden_state is not None:
                rows.append(hidden_state.to(self.dtype).contiguous())
            if x is not None:
                for j in range(x.shape[1]):
                    rows.append(self._W["net_token"].embed[x[:, j]])  # gather of N rows (indexing only)
            if st is None:
                st = KVState(spec, N, self.tokenizer.max_token_seq, rows[0])
                cache._mh_state = st
            outs = []
            for r in rows:
                h = engine.stack_decode(spec, self._W["net_token"], r.contiguous(), self.rope("net_token"), st)
                lg = torch.empty((N, Vp), dtype=self.dtype, device=self.device)
                ops.gemm_nt(h, self.lm_head.weight.data, lg[:, :V])
                outs.append(lg[:, :V])
            return torch.stack(outs, dim=1)

    def _stack_params(self, pre: str) -> List[nn.Parameter]:
        st = getattr(self, pre)
        out = [st.embed_tokens.weight]
        for l in st.layers:
            out += [l.self_attn.q_proj.weight, l.self_attn.k_proj.weight, l.self_attn.v_proj.weight,
                    l.self_attn.o_proj.weight, l.mlp.gate_proj.weight, l.mlp.up_proj.weight, l.mlp.down_proj.weight,
                    l.input_layernorm.weight, l.post_attention_layernorm.weight]
        out.append(st.norm.weight)
        return out

    SCORE_CHUNK_ROWS = 32768  # token rows per lm_head + cross-entropy chunk of score() (the training loss head's default)

    @torch.no_grad()
    def score(self, x: torch.Tensor, lengths=None) -> torch.Tensor:
        """(ours) x (B, S, 8) int64 -> fp32 (B, S - 1) on the device: entry [b, t] is the model's log-likelihood of event t + 1 given
        events <= t -- ll(e) = sum over the event's token positions 0..arity of (z_c - log sum exp z), pad targets ignored: exactly
        the quantity the training loss sums (hidden = forward(x[:, :-1]), the token stack teacher-forced on x[:, 1:]), so
        ``-score(x).sum() / (number of non-pad targets)`` is ``validation_step``'s loss on x.  ``lengths`` (B ints, optional): row b
        holds lengths[b] events; events at index >= lengths[b], and events made of pad only, give exactly 0.  The same quantity
        ``DecodePool.logprobs`` reports for generated events.  Runs on the existing kernels -- mh_cross_entropy
        returns the per-token loss -- chunked over rows as the training loss head is; nothing is kept for a backward."""
        self._require_gpu()
        if x.dim() != 3 or x.shape[1] < 2:
            raise ValueError(f"score: expected (batch, events >= 2, tokens) ids, got shape {tuple(x.shape)}")
        B, S1, T = x.shape
        if lengths is not None:
            lengths = [int(n) for n in lengths]
            if len(lengths) != B or any(not 0 <= n <= S1 for n in lengths):
                raise ValueError(f"score: lengths {lengths} for a batch of {B} rows of {S1} events")
        tok = self.tokenizer
        hidden = self.forward(x[:, :-1])  # (checks the ids; forward-only schedule under no_grad)
        dev, dty = self.device, self.dtype
        y = x[:, 1:].to(device=dev, dtype=torch.long).contiguous()
        S = S1 - 1
        tspec, Wt = self._specs["net_token"], self._W["net_token"]
        D, V, Vp = tspec.D, tok.vocab_size, self.vocab_padded
        N = B * S
        R = N * T
        y_t = y.view(N, T)
        seq = torch.empty((N, T, D), dtype=dty, device=dev)
        ops.concat_tok_fwd(hidden.reshape(N, D), y_t, Wt.embed, seq, T)
        h, _ = engine.stack_forward(tspec, Wt, seq.view(R, D), N, T, self.rope("net_token"), save=False,
                                    folded=self._folded_for(tspec, seq.view(R, D)))
        del seq
        targets = y_t.reshape(R)
        row_loss = torch.empty(R, dtype=torch.float32, device=dev)
        lm_w = self.lm_head.weight.data
        chunk = max(T, (self.SCORE_CHUNK_ROWS // T) * T)
        logits = torch.empty((min(chunk, R), Vp), dtype=dty, device=dev)
        for r0 in range(0, R, chunk):
            r1 = min(R, r0 + chunk)
            lg = logits[: r1 - r0]
            ops.gemm_nt(h[r0:r1], lm_w, lg[:, :V])
            ops.cross_entropy(lg, V, targets[r0:r1], row_loss[r0:r1], None, None, None, tok.pad_id)
        # (a pad target's row_loss is 0: ignore_index; the sum over an event's 8 rows is its ll, negated)
        out = -row_loss.view(B, S, T).sum(-1)
        if lengths is not None:  # event t + 1 exists iff t + 1 < lengths[b]
            keep = torch.arange(1, S1, device=dev)[None, :] < torch.tensor(lengths, device=dev)[:, None]
            out = torch.where(keep, out, torch.zeros_like(out))
        return out

    def sample_top_p_k(self, probs, p, k, generator=None):
        """midi_model.py:152-165, op for op (torch.sort / cumsum / multinomial), so a seeded
        ``torch.Generator`` is consumed exactly as the reference consumes it."""
        probs_sort, probs_idx = torch.sort(probs, dim=-1, descending=True)
        probs_sum = torch.cumsum(probs_sort, dim=-1)
        mask = probs_sum - probs_sort > p
        probs_sort[mask] = 0.0
        mask = torch.zeros(probs_sort.shape[-1], device=probs_sort.device)
        mask[:k] = 1
        probs_sort = probs_sort * mask
        probs_sort.div_(probs_sort.sum(dim=-1, keepdim=True))
        shape = probs_sort.shape
        next_token = torch.multinomial(probs_sort.reshape(-1, shape[-1]), num_samples=1,
                                       generator=generator).reshape(*shape[:-1], 1)
        return torch.gather(probs_idx, -1, next_token).reshape(*shape[:-1])

    # ------------------------------------------------------------------------------------- generation
    def _grammar(self):
        if self._tables is None:
            from .tokenizer import grammar_tables
            first, lo, hi, arity = grammar_tables(self.tokenizer)
            dev = self.device
            self._tables = (torch.tensor(first, dtype=torch.uint8, device=dev),
                            torch.tensor(lo, dtype=torch.int32, device=dev),
                            torch.tensor(hi, dtype=torch.int32, device=dev), arity)
        return self._tables

    def generate(self, prompt=None, batch_size=1, max_len=512, temp=1.0, top_p=0.98, top_k=20, generator=None,
                 ban_eos: bool = False, disable_patch_change: bool = False, disable_control_change: bool = False,
                 disable_channels=None, share_prompt: bool = False):
        """midi_model.py:167-250 with the host-bound parts moved to the device: grammar masks come from
        per-event-id range tables (no Python loop over the batch), K/V live in preallocated buffers, every decode /
        sampling step is a replayed hipGraph (decode.py) and the only device->host traffic is ONE copy of the B sampled
        event ids per event (the reference does B ``.item()`` calls).  The number of sampling calls per event follows
        the reference's break rule exactly, so a seeded generator yields the reference's stream.

        Returns ``np.ndarray (B, <= max_len, 8) int64`` including the prompt.  Extras (ours): ``ban_eos`` removes EOS
        from the first-token mask (throughput runs); ``disable_patch_change`` / ``disable_control_change`` /
        ``disable_channels`` are the mask options of the serving loop (app.py:27-31, 73-86).

        ``batch_size``: bf16 batches of up to 256 rows run the folded 5-launch decoder layer, the three graphs per event and the
        fused sampler -- up to 64 rows on ``mh_gemm_skinny``, 65 to 256 on ``mh_gemm_skinny_wide`` (the same kernel over 64-row
        groups; DESIGN 7.5 has the measured rates).  Larger batches and fp32 keep the general GEMM form (about twice the launches),
        and so does ``MH_DECODE_WIDE=0`` from 65 rows up (read when a session is created).  The same holds for ``generate_stream``,
        ``generate_ragged`` and ``share_prompt``.

        ``share_prompt=True`` (ours; what every caller of the reference does: B continuations of ONE prompt) takes a
        ``(L, T')`` prompt, a ``(1, L, T')`` prompt or a ``(batch_size, L, T')`` prompt whose rows are all equal (checked on the
        host; unequal rows raise ``ValueError`` naming the first row that differs).  The prompt is prefilled once instead of B
        times, its K/V are cached once instead of B times, and every decoded event reads them once per head for all B rows
        (shared.py).  With ``prompt=None`` there is nothing to share and the plain path runs.  Output shape, dtype,
        prompt inclusion, ``max_len``, the break rule and the mask options are those of the plain path, and the same
        ``[8, B, V]`` variates are drawn from ``generator`` in the same order, so a seeded generator is left in the same state.
        The logits are summed in another order than on the plain path (the prompt's keys in chunks of 256, then the suffix), so
        sampled ids may differ from the plain path's where two candidates are within rounding of each other: bit equality with
        the plain path is NOT promised (two shared runs are bit-identical).
        Crossover ((B, P) below which sharing is slower): NOT MEASURED at this commit -- ``tools/bench_shared_prompt.py`` is the
        vehicle and no MI355X run of it exists yet; from bytes alone sharing adds 12 launches per event and saves
        (B - 1) x P x 49,152 bytes of K/V reads, so expect it to lose at short prompts and small B.  Opt-in for that reason."""
        shared = self._shares_prompt(prompt, share_prompt)
        inp = self._prompt_tensor(prompt, batch_size)
        parts = [inp.cpu().numpy()]
        for ev in self._generate_events(inp, batch_size, max_len, temp, top_p, top_k, generator, ban_eos,
                                        disable_patch_change, disable_control_change, disable_channels, shared):
            parts.append(ev[:, None, :])
        return np.concatenate(parts, axis=1)

    def generate_stream(self, prompt=None, batch_size=1, max_len=512, temp=1.0, top_p=0.98, top_k=20,
                        disable_patch_change=False, disable_control_change=False, disable_channels=None, generator=None,
                        share_prompt: bool = False):
        """The serving loop of the reference (app.py:27-120, same arguments): a Python generator that yields every new
        event as ``np.ndarray (B, 8) int64`` as soon as it is sampled; the prompt is cropped to its last 4096 events
        (app.py:53).  Same kernels and sessions as ``generate``; ``share_prompt`` as there (the crop comes first)."""
        shared = self._shares_prompt(prompt, share_prompt)
        inp = self._prompt_tensor(prompt, batch_size)[:, -4096:]
        return self._generate_events(inp, batch_size, max_len, temp, top_p, top_k, generator, False,
                                     disable_patch_change, disable_control_change, disable_channels, shared)

    def generate_ragged(self, prompts, max_len=512, temp=1.0, top_p=0.98, top_k=20, disable_patch_change=False,
                        disable_control_change=False, disable_channels=None, generator=None, ban_eos: bool = False, seed=None):
        """(ours) ``generate`` for B prompts of B DIFFERENT lengths in ONE decode batch: ``prompts`` is a sequence of B arrays, row
        b of shape ``(L_b, T')``, 1 <= T' <= 8, padded and range-checked as ``generate`` pads and checks its prompt.  Returns a
        list of B ``np.ndarray (<= max_len, 8) int64``, row b with its prompt in front.

        The rows decode in lockstep: event step t samples one event for every row, and row b is live while L_b + t < max_len.
        A row that reaches ``max_len`` is retired: the device parks it at position max_len and goes on sampling it (no host
        bookkeeping per row, no extra sync; decode.py), the host drops what it samples.  The reference's break rule and its
        "every row sampled EOS" stop are evaluated over the live rows only, so with equal lengths this is the rule ``generate``
        runs; the noise is still ``[8, B, V]`` per event.  The call ends when no row is live or every live row sampled EOS, so a
        row may come back shorter than ``max_len`` only through EOS.  The set of rows is fixed for the call (``decode_pool`` admits
        and releases rows while the batch runs).  ``ValueError`` before
        any launch: no prompts, an empty prompt, a prompt of ``max_len`` events or more, ids outside the vocabulary, and what the
        mask options refuse in ``generate``.

        A value PER ROW: each of ``temp``, ``top_p``, ``top_k``, ``max_len``, ``ban_eos``, ``disable_patch_change`` and
        ``disable_control_change`` is a scalar (every row's, as in ``generate``) or a sequence of B values, row b's at index b;
        ``disable_channels`` is ``None``, a flat sequence of ints (every row's) or a sequence of B entries, each ``None`` or a
        sequence of ints.  With scalars (and a flat channel list) alone the call runs the path, the session and the kernels it ran
        before per-row values existed.  As soon as ONE argument is a sequence -- equal entries included -- the call runs on a
        ``row_params`` session (decode.py): the values live in device buffers with one entry per row, the sampler is
        ``mh_sample_top_p_k_rows`` (the uniform sampler's kernel, row b on its own values: same arithmetic, same id), and the
        pooled session of a (B, capacity) serves every setting without a new K/V cache or a recapture.  Row b is then live while
        L_b + t < max_len[b], the capacity follows max(max_len) + 1, and the break rule, the all-EOS stop, the ``[8, B, V]`` noise
        per event and the generator's final state follow the rule above.  Further refusals of this form, all ``ValueError`` before
        any launch: a sequence whose length is not B; a temperature that is not finite or not above 0; a NaN ``top_p``; a
        ``top_k`` outside [1, min(64, V)] (the scalar path keeps its op-by-op sampler for larger k, this form has none); row b's
        prompt holding ``max_len[b]`` events or more (the message names the row); per row, what the mask options refuse.
        A SEED per row: ``seed`` is a sequence of B Python ints in [0, 2^64).  The call then runs on a ``seeded`` row_params session
        (decode.py): no ``[8, B, V]`` noise and no generator -- ``seed`` together with ``generator`` is a ``ValueError`` -- the
        sampler computes row b's variates from (seed[b], the index of the event in row b's result, token position, rank)
        (``mh_sample_top_p_k_seeded``), so row b's ids no longer depend on its batch mates' draws or on its row number.  The
        stated limits are pool.py's: the promise holds at equal launch shapes (the same B; the same prompts prefilled together).
        ``bool``, floats, negatives and a wrong length are refused, the message naming the row.  ``seed=None``: everything above.
        Out of scope: per-row values on ``generate`` / ``generate_stream`` / ``share_prompt``.
        Admitting new rows into a running batch is not this call's
        job: ``decode_pool`` / ``generate_pool`` do that (pool.py).
        The prompts are prefilled packed -- no padded event is computed; prompts of ONE length are prefilled by
        ``generate``'s uniform forward, so that for the same seeded generator the call returns exactly ``generate``'s ids.
        Speed against one ``generate`` call per distinct length: NOT MEASURED at this commit -- ``tools/bench_ragged.py`` is the
        vehicle and no MI355X run of it exists yet.  From launches alone: a decoded event costs about the same
        ~210 launches for 1 row as for 64, so B lengths in one batch should approach B times the useful events/s of B batches
        of one; the net graph gains two tiny launches (the position update) and nothing else."""
        rp = self._row_params(prompts, max_len, temp, top_p, top_k, ban_eos, disable_patch_change, disable_control_change,
                              disable_channels, seed, generator)
        rows = self._ragged_prompts(prompts, max_len if rp is None else rp["max_len"], None)
        chans = None if rp is not None else \
            self._check_mask_options(ban_eos, disable_patch_change, disable_control_change, disable_channels)
        outs = [[r] for r in rows]
        for ev, live in self._generate_events_ragged(rows, max_len, temp, top_p, top_k, generator, ban_eos, disable_patch_change,
                                                     disable_control_change, chans, rp):
            for b in np.flatnonzero(live):
                outs[b].append(ev[b][None])
        return [np.concatenate(o, axis=0) for o in outs]

    def generate_stream_ragged(self, prompts, max_len=512, temp=1.0, top_p=0.98, top_k=20, disable_patch_change=False,
                               disable_control_change=False, disable_channels=None, generator=None, ban_eos: bool = False,
                               seed=None):
        """The serving form of ``generate_ragged``: a Python generator that yields, per event step, ``(events np.int64 (B, 8),
        live np.bool_ (B,))`` -- row b of ``events`` counts only where ``live[b]``.  Each prompt is cropped to its last 4096
        events first, as ``generate_stream`` crops.  The arguments are checked HERE, before the generator is handed out."""
        rp = self._row_params(prompts, max_len, temp, top_p, top_k, ban_eos, disable_patch_change, disable_control_change,
                              disable_channels, seed, generator)
        rows = self._ragged_prompts(prompts, max_len if rp is None else rp["max_len"], 4096)
        chans = None if rp is not None else \
            self._check_mask_options(ban_eos, disable_patch_change, disable_control_change, disable_channels)
        return self._generate_events_ragged(rows, max_len, temp, top_p, top_k, generator, ban_eos, disable_patch_change,
                                            disable_control_change, chans, rp)

    @staticmethod
    def _per_row(x) -> bool:
        return isinstance(x, (list, tuple)) or (isinstance(x, (np.ndarray, torch.Tensor)) and x.ndim > 0)

    def _row_params(self, prompts, max_len, temp, top_p, top_k, ban_eos, disable_patch_change, disable_control_change,
                    disable_channels, seed=None, generator=None):
        """The arguments of generate_ragged that take a value per row, checked on the host before any launch.  -> None when every
        one of them is the call's (scalars; a flat list of channels): today's path.  Otherwise a dict of B-element lists -- scalars
        repeated -- under the argument names, ``chans`` holding row b's sorted banned channels; every refusal is a ValueError.
        ``seed`` (not None: B ints in [0, 2^64), row b's seed) always gives the dict, with the checked seeds under ``"seed"``."""
        channels_per_row = self._per_row(disable_channels) and any(c is None or self._per_row(c) for c in disable_channels)
        scalars = dict(max_len=max_len, temp=temp, top_p=top_p, top_k=top_k, ban_eos=ban_eos,
                       disable_patch_change=disable_patch_change, disable_control_change=disable_control_change)
        if seed is None and not channels_per_row and not any(self._per_row(v) for v in scalars.values()):
            return None
        if seed is not None and generator is not None:
            raise ValueError("generate_ragged: seed and generator together -- a seeded call draws nothing from a generator")
        if prompts is None or len(prompts) == 0:
            raise ValueError("generate_ragged: no prompts")
        B = len(prompts)
        rp = {}
        for name, v in scalars.items():
            v = list(v.tolist() if isinstance(v, (np.ndarray, torch.Tensor)) else v) if self._per_row(v) else [v] * B
            if len(v) != B:
                raise ValueError(f"generate_ragged: {name} holds {len(v)} values for {B} prompts")
            rp[name] = v
        chan_rows = list(disable_channels) if channels_per_row else [disable_channels] * B
        if len(chan_rows) != B:
            raise ValueError(f"generate_ragged: disable_channels holds {len(chan_rows)} entries for {B} prompts")
        kmax = min(ops.SAMPLE_MAX_K, self.tokenizer.vocab_size)
        rp["chans"] = []
        for b in range(B):
            t, p, k = rp["temp"][b], rp["top_p"][b], rp["top_k"][b]
            if not (math.isfinite(t) and t > 0):
                raise ValueError(f"generate_ragged: row {b}: temperature {t} is not a finite number above 0")
            if math.isnan(p):
                raise ValueError(f"generate_ragged: row {b}: top_p is NaN")
            if int(k) != k or not 1 <= k <= kmax:
                raise ValueError(f"generate_ragged: row {b}: top_k {k} outside [1, {kmax}] (per-row parameters run on the fused "
                                 f"sampler alone)")
            if int(rp["max_len"][b]) != rp["max_len"][b]:
                raise ValueError(f"generate_ragged: row {b}: max_len {rp['max_len'][b]} is not an integer")
            try:
                rp["chans"].append(self._check_mask_options(rp["ban_eos"][b], rp["disable_patch_change"][b],
                                                            rp["disable_control_change"][b], chan_rows[b]))
            except ValueError as e:
                raise ValueError(f"row {b}: {e}") from None
        rp["max_len"] = [int(n) for n in rp["max_len"]]
        rp["top_k"] = [int(k) for k in rp["top_k"]]
        if seed is not None:
            if not self._per_row(seed) or len(seed) != B:
                raise ValueError(f"generate_ragged: seed must be a sequence of {B} integers, one per prompt"
                                 + (f": it holds {len(seed)}" if self._per_row(seed) else ""))
            seed = seed.tolist() if isinstance(seed, (np.ndarray, torch.Tensor)) else list(seed)
            for b, s in enumerate(seed):
                if isinstance(s, bool) or not isinstance(s, (int, np.integer)) or not 0 <= int(s) < (1 << 64):
                    raise ValueError(f"generate_ragged: row {b}: seed {s!r} is not an integer in [0, 2^64)")
            rp["seed"] = [int(s) for s in seed]
        return rp

    def _ragged_prompts(self, prompts, max_len, crop) -> list:
        """the prompts of generate_ragged as contiguous int64 arrays (L_b, 8): _prompt_tensor's range check and padding per row.
        ``max_len``: the call's, or a list with row b's"""
        self._require_gpu()
        tok = self.tokenizer
        T = tok.max_token_seq
        if prompts is None or len(prompts) == 0:
            raise ValueError("generate_ragged: no prompts")
        rows = []
        for b, p in enumerate(prompts):
            p = np.asarray(p)
            if p.ndim != 2 or p.shape[0] < 1 or p.shape[1] < 1:
                raise ValueError(f"generate_ragged: prompt {b} has shape {p.shape}; (L, T') with L >= 1 and 1 <= T' <= {T} is needed")
            if p.min() < 0 or p.max() >= tok.vocab_size:
                raise ValueError(f"prompt holds token ids outside [0, {tok.vocab_size}): min {p.min()}, max {p.max()}")
            p = p[:, :T]
            if p.shape[1] < T:
                p = np.pad(p, ((0, 0), (0, T - p.shape[1])), mode="constant", constant_values=tok.pad_id)
            if crop is not None:
                p = p[-crop:]
            limit = max_len[b] if isinstance(max_len, list) else max_len
            if p.shape[0] >= limit:
                raise ValueError(f"generate_ragged: prompt {b} has {p.shape[0]} events, max_len is {limit}: nothing to generate")
            rows.append(np.ascontiguousarray(p, dtype=np.int64))
        return rows

    def _generate_events_ragged(self, rows, max_len, temp, top_p, top_k, generator, ban_eos, disable_patch_change,
                                disable_control_change, chans, rp=None):
        """generator over (events (B, 8), live (B,)) of the checked prompts ``rows``; the session goes back to the pool when the
        generator finishes or is closed.  The loop is _generate_events' with the live rows in place of all rows.  ``rp`` (the
        checked per-row arguments of _row_params, or None): the row_params session, row b live while L_b + t < max_len[b]."""
        lengths = np.array([r.shape[0] for r in rows], dtype=np.int64)
        B = len(rows)
        with torch.inference_mode():
            if rp is not None:
                max_len = np.array(rp["max_len"], dtype=np.int64)
                # (1.0, 0.98, 1 fill a NEW session's buffers through its warm-up pass; set_row_params below overwrites them)
                ses = self._checkout_session(B, int(max_len.max()) + 1, 1.0, 0.98, 1, ragged=True, row_params=True,
                                             seeded="seed" in rp)
            else:
                ses = self._checkout_session(B, max_len + 1, float(temp), float(top_p), int(top_k), ragged=True)
        try:
            with torch.inference_mode():
                if rp is not None:
                    self._set_masks_rows(ses, rp)
                    ses.set_row_params(rp["temp"], rp["top_p"], rp["top_k"])
                    if "seed" in rp:
                        ses.set_row_seeds(rp["seed"])
                else:
                    self._set_masks(ses, ban_eos, disable_patch_change, disable_control_change, chans)
                ses.reset()
                ses.begin(generator)
                ses.set_limit(max_len if rp is None else rp["max_len"])
                packed = torch.from_numpy(np.concatenate(rows, axis=0)).to(self.device)
                ses.prefill_ragged(packed, lengths.tolist())  # one packed causal forward; hidden[b] = prompt b's last position
            t = 0
            while True:
                live = lengths + t < max_len          # (row b's next event has index L_b + t)
                with torch.inference_mode():
                    more = bool((lengths + t + 1 < max_len).any())
                    speculative = more and ses.g_steps is not None and _SPECULATIVE_NET
                    event, end_all = ses.sample_event(then_net=speculative, live=live.tolist())
                    t += 1
                    last = end_all or not more
                    if not last:
                        ses.draw_noise()
                        if not speculative:
                            ses.net_step()
                yield event, live
                if last:
                    break
        finally:
            ses.end()
            self._return_session(ses)

    @staticmethod
    def _shares_prompt(prompt, share_prompt: bool) -> bool:
        """share_prompt=True with a prompt: its rows must be equal (host check, before any launch); without one: plain path"""
        if not share_prompt or prompt is None:
            return False
        from .shared import check_equal_rows
        check_equal_rows(prompt)
        return True

    def _prompt_tensor(self, prompt, batch_size: int) -> torch.Tensor:
        """prompt handling of midi_model.py:171-188 (and app.py:35-52): None -> one BOS event per sequence"""
        self._require_gpu()
        tok = self.tokenizer
        T, dev = tok.max_token_seq, self.device
        if prompt is None:
            inp = torch.full((batch_size, 1, T), tok.pad_id, dtype=torch.long, device=dev)
            inp[:, 0, 0] = tok.bos_id
            return inp
        prompt = np.asarray(prompt)
        if prompt.size and (prompt.min() < 0 or prompt.max() >= tok.vocab_size):
            raise ValueError(f"prompt holds token ids outside [0, {tok.vocab_size}): min {prompt.min()}, max {prompt.max()}")
        if prompt.ndim == 2:
            prompt = np.repeat(prompt[None, :], repeats=batch_size, axis=0)
        elif prompt.shape[0] == 1:
            prompt = np.repeat(prompt, repeats=batch_size, axis=0)
        elif prompt.ndim != 3 or prompt.shape[0] != batch_size:
            raise ValueError(f"invalid shape for prompt, {prompt.shape}")
        prompt = prompt[..., :T]
        if prompt.shape[-1] < T:
            prompt = np.pad(prompt, ((0, 0), (0, 0), (0, T - prompt.shape[-1])), mode="constant",
                            constant_values=tok.pad_id)
        return torch.from_numpy(np.ascontiguousarray(prompt)).to(dtype=torch.long, device=dev)

    def _check_mask_options(self, ban_eos, disable_patch_change, disable_control_change, disable_channels) -> list:
        """the mask options of generate / generate_ragged, checked on the host before any launch; -> the banned channels, sorted"""
        tok = self.tokenizer
        # Every grammar mask must keep at least one id.  The reference fails with a (recoverable) multinomial error when a
        # mask is empty (midi_model.py:152-165 on an all-zero row); the fused sampler has no such path -- it would hand a
        # sentinel id to the next embedding lookup, which traps -- so an emptied mask is refused here, before any launch.
        first_ids = {tok.eos_id, *tok.event_ids.values()}
        if ban_eos:
            first_ids.discard(tok.eos_id)
        if disable_patch_change:
            first_ids.discard(tok.event_ids["patch_change"])
        if disable_control_change:
            first_ids.discard(tok.event_ids["control_change"])
        if not first_ids:
            raise ValueError("generate: the options leave no legal event id at token position 0")
        chans = sorted(set(int(c) for c in (disable_channels or [])))
        n_chan = len(tok.parameter_ids["channel"])
        if any(c < 0 or c >= n_chan for c in chans):
            raise ValueError(f"generate: disable_channels holds a channel outside [0, {n_chan}): {chans}")
        if len(chans) >= n_chan:
            raise ValueError("generate: disable_channels bans every channel id: no legal token is left at the channel position")
        return chans

    def _set_masks(self, ses, ban_eos, disable_patch_change, disable_control_change, chans) -> None:
        """write the checked mask options into a session's first-token mask and ban list"""
        tok = self.tokenizer
        ses.first_mask.copy_(self._grammar()[0])
        if ban_eos:
            ses.first_mask[tok.eos_id] = 0
        if disable_patch_change:
            ses.first_mask[tok.event_ids["patch_change"]] = 0
        if disable_control_change:
            ses.first_mask[tok.event_ids["control_change"]] = 0
        ses.ban.zero_()
        for c in chans:
            ses.ban[tok.parameter_ids["channel"][c]] = 1

    def _mask_rows(self, rp):
        """the checked per-row mask options as two host uint8 tensors [B, V]: (first-token mask, banned ids)"""
        tok = self.tokenizer
        B = len(rp["chans"])
        first = self._grammar()[0].cpu()[None, :].repeat(B, 1)
        ban = torch.zeros_like(first)
        for b in range(B):
            if rp["ban_eos"][b]:
                first[b, tok.eos_id] = 0
            if rp["disable_patch_change"][b]:
                first[b, tok.event_ids["patch_change"]] = 0
            if rp["disable_control_change"][b]:
                first[b, tok.event_ids["control_change"]] = 0
            for c in rp["chans"][b]:
                ban[b, tok.parameter_ids["channel"][c]] = 1
        return first, ban

    def _set_masks_rows(self, ses, rp) -> None:
        """_set_masks per row of a row_params session: both [B, V] masks are built on the host and copied once"""
        first, ban = self._mask_rows(rp)
        ses.first_mask.copy_(first)
        ses.ban.copy_(ban)

    def _check_request(self, prompt, max_len, temp, top_p, top_k, ban_eos, disable_patch_change, disable_control_change,
                       disable_channels, crop=4096, seed=None):
        """ONE request of a decode pool, checked as generate_ragged checks a row with values of its own (_row_params,
        _check_mask_options, _ragged_prompts: their code, their ValueErrors, before any launch) -> (prompt (L, 8) int64 cropped to
        its last ``crop`` events, the one-row dict of _row_params)"""
        if any(self._per_row(v) for v in (max_len, temp, top_p, top_k, ban_eos, disable_patch_change, disable_control_change)):
            raise ValueError("a request takes one value per option: a scalar max_len, temp, top_p, top_k and mask option")
        if disable_channels is not None and (not self._per_row(disable_channels) or any(
                c is None or self._per_row(c) for c in disable_channels)):
            raise ValueError("a request's disable_channels is None or a flat sequence of channel numbers")
        if self._per_row(seed):
            raise ValueError("a request takes one seed: an integer in [0, 2^64)")
        rp = self._row_params([prompt], [max_len], [temp], [top_p], [top_k], [ban_eos], [disable_patch_change],
                              [disable_control_change], [disable_channels], None if seed is None else [seed])
        return self._ragged_prompts([prompt], rp["max_len"], crop)[0], rp

    def decode_pool(self, rows: int, capacity: int, generator=None, seeded: bool = False, prefix_slots: int = 0,
                    prefix_capacity: int = 0, kv_dtype: Optional[str] = None, logprobs: bool = False, lora_slots: int = 0,
                    lora_rank: int = 64, lookahead: Optional[int] = None):
        """(ours) a ``pool.DecodePool`` on this model: ``rows`` decode rows that requests are admitted into and released from
        while the batch runs (continuous batching).  ``capacity``: cache rows per decode row; a request needs
        max_len + 1 <= capacity (the session's own capacity is rounded up as every session's is, 256 x 2^k).  The pool takes one
        pooled ``row_params`` session at its first admission and holds it until ``close()`` (it is a context manager); it draws
        from ``generator`` as ``generate_ragged`` does.  ``seeded=True``: every request brings a seed of its own
        (``submit(seed=...)``) and the pool draws from no generator (pool.py has the promise and its limits); ``generator`` is
        then refused.  ``prefix_slots`` = G > 0 with ``prefix_capacity`` = Pmax: the pool's session keeps G prefix slots of Pmax
        events, and ``submit(..., share_prefix=True)`` stores a prompt of at most Pmax events in one, read ONCE per decoded event
        for all the rows that continue it -- siblings (``n=k``) and fork children (pool.py).
        ``kv_dtype="fp8"``: the rows' event-level K/V is cached as e4m3 codes with a scale per head and event, 0.53 x the bytes
        (pool.py "FP8 K/V"); a bf16 model, at most 256 rows, not with prefix slots (``ValueError``).
        ``logprobs=True``: ``pool.logprobs(rid)`` gives the model's log-likelihood of every event a request generated (pool.py
        "LOG-LIKELIHOODS"); with any of the options above.
        ``lora_slots`` = G > 0 with ``lora_rank`` = R: the pool keeps G LoRA adapters of rank at most R beside the base weights
        (``pool.load_adapter``) and ``submit(..., adapter=id)`` decodes a request under one of them, unmerged, in the same batch as
        requests on other adapters and on none (pool.py "LORA ADAPTERS"); a bf16 model, at most 256 rows, G R a
        multiple of 256 (``ValueError``); with any of the options above.
        ``lookahead`` = k >= 1 (``seeded=True`` only; with ``logprobs``, not with prefix slots, ``kv_dtype`` or ``lora_slots``; rows x
        (k + 1) <= 256; ``ValueError`` otherwise): every request owns k + 1 session rows, k of which verify guessed next events
        (``pool.proposer``), so a request whose guesses are right finishes in fewer steps and its ids never depend on the guesses
        (pool.py "LOOKAHEAD").  Nothing is launched here."""
        from .pool import DecodePool
        if lookahead is not None:
            return DecodePool(self, rows, capacity, generator, seeded, prefix_slots, prefix_capacity, kv_dtype=kv_dtype,
                              logprobs=logprobs, lora_slots=lora_slots, lora_rank=lora_rank, lookahead=lookahead)
        if lora_slots:
            return DecodePool(self, rows, capacity, generator, seeded, prefix_slots, prefix_capacity, kv_dtype=kv_dtype,
                              logprobs=logprobs, lora_slots=lora_slots, lora_rank=lora_rank)
        if logprobs:
            return DecodePool(self, rows, capacity, generator, seeded, prefix_slots, prefix_capacity, kv_dtype=kv_dtype,
                              logprobs=True)
        if kv_dtype is not None:
            return DecodePool(self, rows, capacity, generator, seeded, prefix_slots, prefix_capacity, kv_dtype=kv_dtype)
        if prefix_slots or prefix_capacity:
            return DecodePool(self, rows, capacity, generator, seeded, prefix_slots, prefix_capacity)
        return DecodePool(self, rows, capacity, generator, seeded)

    def generate_pool(self, requests, rows: int, capacity: Optional[int] = None, generator=None,
                      kv_dtype: Optional[str] = None, logprobs: bool = False, adapters: Optional[dict] = None,
                      lora_rank: int = 64, lookahead: Optional[int] = None) -> list:
        """(ours) ``requests``: a list of dicts, each the keyword arguments of ``DecodePool.submit`` (``prompt`` and any of max_len,
        temp, top_p, top_k, ban_eos, disable_patch_change, disable_control_change, disable_channels, seed).  If EVERY request
        carries ``"seed"`` the pool is a seeded one; some with and some without is a ``ValueError``.  They are submitted in order
        to one pool of ``rows`` rows and stepped until all are done: a request waits only until a row is free, and a row that
        finishes is handed to the next request at once.  -> a list of ``np.ndarray (<= max_len, 8) int64``, request i's at index
        i, its prompt in front.  ``capacity`` defaults to the largest max_len + 1.  ``kv_dtype``: as ``decode_pool`` takes it.
        ``logprobs=True``: -> a list of ``(events, logprobs)`` pairs instead, ``logprobs`` the request's ``DecodePool.logprobs``
        array (np.float32, one value per generated event, aligned with ``events[len(prompt):]``).
        ``adapters`` = {name: src} (``src`` as ``DecodePool.load_adapter`` takes it): the pool gets a slot for each (as many of rank
        ``lora_rank`` as make slots x rank a multiple of 256) and a request's ``"adapter": name`` decodes it under that adapter.
        ``lookahead``: as ``decode_pool`` takes it (every request then carries a seed); the pool's built-in proposer guesses."""
        requests = list(requests)
        if not requests:
            return []
        if capacity is None:
            capacity = max(int(r.get("max_len", 512)) for r in requests) + 1
        with_seed = sum("seed" in r and r["seed"] is not None for r in requests)
        if with_seed not in (0, len(requests)):
            raise ValueError(f"generate_pool: {with_seed} of {len(requests)} requests carry a seed -- all of them or none")
        kvq = dict(kv_dtype=kv_dtype) if kv_dtype is not None else {}
        if logprobs:
            kvq["logprobs"] = True
        if adapters:
            per = 256 // math.gcd(256, int(lora_rank))   # slots come in steps that keep slots x rank a multiple of 256
            kvq.update(lora_slots=-(-len(adapters) // per) * per, lora_rank=lora_rank)
        elif any(r.get("adapter") is not None for r in requests):
            raise ValueError("generate_pool: a request names an adapter and ``adapters`` is empty")
        if lookahead is not None:
            kvq["lookahead"] = lookahead
        with self.decode_pool(rows, capacity, generator, seeded=with_seed > 0, **kvq) as pool:
            if adapters:
                names = {name: pool.load_adapter(src) for name, src in adapters.items()}
                unknown = [r["adapter"] for r in requests if r.get("adapter") is not None and r["adapter"] not in names]
                if unknown:
                    raise ValueError(f"generate_pool: requests name the adapters {unknown}; given: {sorted(names)}")
                requests = [dict(r, adapter=names[r["adapter"]]) if r.get("adapter") is not None else r for r in requests]
            ids = [pool.submit(**r) for r in requests]
            while pool.pending():
                pool.step()
            if logprobs:
                return [(pool.result(i), pool.logprobs(i)) for i in ids]
            return [pool.result(i) for i in ids]

    def _generate_events(self, inp, batch_size, max_len, temp, top_p, top_k, generator, ban_eos, disable_patch_change,
                         disable_control_change, disable_channels, shared: bool = False):
        """generator over the new events ((B, 8) int64 numpy each); the session is returned to the pool when the
        generator finishes or is closed"""
        tok = self.tokenizer
        T = tok.max_token_seq
        B = batch_size
        cur_len = inp.shape[1]
        if cur_len >= max_len:
            return
        chans = self._check_mask_options(ban_eos, disable_patch_change, disable_control_change, disable_channels)
        with torch.inference_mode():
            if shared:  # the prompt in its own cache; the per-row cache holds the generated suffix only
                ses = self._checkout_session(B, max_len - cur_len + 1, float(temp), float(top_p), int(top_k), shared_need=cur_len)
            else:
                ses = self._checkout_session(B, max(max_len, cur_len) + 1, float(temp), float(top_p), int(top_k))
        try:
            with torch.inference_mode():
                self._set_masks(ses, ban_eos, disable_patch_change, disable_control_change, chans)
                ses.reset()
                ses.begin(generator)
                ses.prefill(inp)  # causal forward over the prompt; hidden = last position
            while cur_len < max_len:
                with torch.inference_mode():
                    more = cur_len + 1 < max_len
                    speculative = more and ses.g_steps is not None and _SPECULATIVE_NET
                    # the event's 8 token steps (one replayed graph, one host copy); in the graph form the net step over
                    # the event is queued behind them before the host waits
                    event, end_all = ses.sample_event(then_net=speculative)
                    cur_len += 1
                    last = end_all or not more
                    if not last:
                        ses.draw_noise()  # the next event's draws, on a side stream under the net step
                        if not speculative:
                            ses.net_step()  # decode the event just sampled; hidden = its net output (overlaps the consumer)
                yield event
                if last:
                    break
        finally:
            ses.end()
            self._return_session(ses)

    # decode sessions: buffers + captured graphs, one per concurrent generate() call (decode.py)
    def _checkout_session(self, B: int, need: int, temp: float, top_p: float, top_k: int, shared_need: int = 0,
                          ragged: bool = False, row_params: bool = False, seeded: bool = False, prefix_slots: int = 0,
                          prefix_capacity: int = 0, kv_dtype: Optional[str] = None, logprobs: bool = False, lora_slots: int = 0,
                          lora_rank: int = 64, lookahead: int = 0):
        """``lookahead`` = k (seeded row_params only): the session of B rows in groups of k + 1 that share a cache sequence
        (DecodeSession); a pooled session of its own kind, 0: the session as it was.
        ``lora_slots`` / ``lora_rank`` (row_params only): the session with that many LoRA adapter slots (DecodeSession); a pooled
        session of its own kind, 0: the session as it was.
        ``logprobs`` (row_params only): the session whose samplers also write the drawn ids' log-probabilities (DecodeSession); a
        pooled session of its own kind, False: the session as it was.
        ``kv_dtype`` = "fp8" (row_params only): the session whose event-level cache holds e4m3 codes and scales (DecodeSession); a
        pooled session of its own kind, None: the session as it was.
        ``prefix_slots`` / ``prefix_capacity`` (row_params only): a session with that many prefix slots of that many rows
        (DecodeSession; the capacity is rounded up by the doubling rule too); 0: the session as it was.
        ``shared_need`` > 0: a shared-prompt session whose prompt cache holds shared_need events (capacities by the same
        doubling rule from 256, so one captured session serves a range of prompt and suffix lengths).  ``ragged``: a session
        with a position per row (generate_ragged), pooled like the others; not together with shared_need.  ``row_params``
        (ragged only): the session that reads temperature, top-p, top-k, masks and limit per row from its own buffers; its key
        holds none of them, so temp / top_p / top_k only fill the buffers of a session built here.  ``seeded`` (row_params only):
        the session whose sampler computes its noise from per-row seeds; a pooled session of its own kind."""
        from .decode import DecodeSession
        cap = 256
        while cap < need:
            cap *= 2
        scap = 0
        if shared_need > 0:
            scap = 256
            while scap < shared_need:
                scap *= 2
        pcap = 0
        if prefix_slots:
            pcap = 256
            while pcap < prefix_capacity:
                pcap *= 2
        if lookahead:
            key = DecodeSession.make_key(self, B, cap, temp, top_p, top_k, scap, ragged, row_params, seeded, prefix_slots, pcap,
                                         kv_dtype, logprobs, lora_slots, lora_rank, lookahead=lookahead)
        elif lora_slots:
            key = DecodeSession.make_key(self, B, cap, temp, top_p, top_k, scap, ragged, row_params, seeded, prefix_slots, pcap,
                                         kv_dtype, logprobs, lora_slots, lora_rank)
        elif logprobs:
            key = DecodeSession.make_key(self, B, cap, temp, top_p, top_k, scap, ragged, row_params, seeded, prefix_slots, pcap,
                                         kv_dtype, True)
        elif kv_dtype is not None:
            key = DecodeSession.make_key(self, B, cap, temp, top_p, top_k, scap, ragged, row_params, seeded, prefix_slots, pcap,
                                         kv_dtype)
        elif prefix_slots:
            key = DecodeSession.make_key(self, B, cap, temp, top_p, top_k, scap, ragged, row_params, seeded, prefix_slots, pcap)
        else:
            key = DecodeSession.make_key(self, B, cap, temp, top_p, top_k, scap, ragged, row_params, seeded)
        pool = self._sessions
        with pool.lock:
            found = None
            for k, ses in enumerate(pool.idle):
                if ses.key == key:
                    found = pool.idle.pop(k)
                    break
            while found is None and len(pool.idle) >= 4:  # bound the memory held by idle sessions
                pool.idle.pop(0)
        if found is not None:
            found.refresh()  # weights may have been trained / merged since the session derived its folded copies
            return found
        if lookahead:
            return DecodeSession(self, B, cap, temp, top_p, top_k, scap, ragged, row_params, seeded, prefix_slots, pcap, kv_dtype,
                                 logprobs=logprobs, lora_slots=lora_slots, lora_rank=lora_rank, lookahead=lookahead)
        if lora_slots:
            return DecodeSession(self, B, cap, temp, top_p, top_k, scap, ragged, row_params, seeded, prefix_slots, pcap, kv_dtype,
                                 logprobs=logprobs, lora_slots=lora_slots, lora_rank=lora_rank)
        if logprobs:
            return DecodeSession(self, B, cap, temp, top_p, top_k, scap, ragged, row_params, seeded, prefix_slots, pcap, kv_dtype,
                                 logprobs=True)
        if kv_dtype is not None:
            return DecodeSession(self, B, cap, temp, top_p, top_k, scap, ragged, row_params, seeded, prefix_slots, pcap, kv_dtype)
        if prefix_slots:
            return DecodeSession(self, B, cap, temp, top_p, top_k, scap, ragged, row_params, seeded, prefix_slots, pcap)
        return DecodeSession(self, B, cap, temp, top_p, top_k, scap, ragged, row_params, seeded)

    def _return_session(self, ses) -> None:
        with self._sessions.lock:
            self._sessions.idle.append(ses)

    # ------------------------------------------------------------------------------------ persistence
    def save_pretrained(self, save_directory: str):
        from safetensors.torch import save_file
        os.makedirs(save_directory, exist_ok=True)
        self.config.save_pretrained(save_directory)
        save_file({k: v.detach().cpu().contiguous() for k, v in self.state_dict().items()},
                  os.path.join(save_directory, "model.safetensors"))

    @classmethod
    def from_pretrained(cls, directory: str):
        from safetensors.torch import load_file
        cfg = MIDIModelConfig.from_json_file(os.path.join(directory, "config.json"))
        model = cls(cfg)
        model.load_checkpoint_state(load_file(os.path.join(directory, "model.safetensors")))
        return model

    # keys a reference-side checkpoint may carry that are not parameters of the model (buffers of older HF versions)
    _BENIGN_EXTRA = ("rotary_emb.inv_freq",)

    def load_checkpoint_state(self, state: dict):
        """Load a reference checkpoint's tensors the way app.py:311-316 / train.py:433-436 do (``strict=False``) but
        WITHOUT its silence: a Lightning ``.ckpt`` payload (``{"state_dict": ...}``) is unwrapped, the prefixes other
        wrappers add (``model.``, ``base_model.model.``, ``module.``) are stripped when they cover every key, known-benign
        extras are dropped, and any parameter the file does not supply -- or any other unexpected key -- raises instead of
        leaving random-initialised weights behind.  Returns self."""
        if "state_dict" in state and not torch.is_tensor(state["state_dict"]):
            state = state["state_dict"]
        own = set(self.state_dict().keys())
        # wrapper prefixes in any order and nesting (torch.compile's _orig_mod., DDP's module., Lightning's model., peft's
        # base_model.model.): stripped, one at a time, until none covers every key or the keys are ours
        prefixes = ("model.", "base_model.model.", "module.", "_orig_mod.")
        for _ in range(8):
            if own & set(state):
                break
            hit = next((p for p in prefixes if state and all(k.startswith(p) for k in state)), None)
            if hit is None:
                break
            state = {k[len(hit):]: v for k, v in state.items()}
        if any(".base_layer." in k or ".lora_A." in k or ".lora_B." in k for k in state):
            raise RuntimeError("this checkpoint holds peft-wrapped modules (base_layer / lora_A / lora_B keys): load the base weights "
                               "with load_checkpoint_state and the adapter with MIDIModel.load_merge_lora(adapter_dir), or merge "
                               "the adapter before saving (merge_and_unload)")
        state = {k: v for k, v in state.items() if not k.endswith(self._BENIGN_EXTRA)}
        res = self.load_state_dict(state, strict=False)
        if res.missing_keys or res.unexpected_keys:
            raise RuntimeError(f"checkpoint does not match the model: missing {sorted(res.missing_keys)[:8]} "
                               f"({len(res.missing_keys)}), unexpected {sorted(res.unexpected_keys)[:8]} "
                               f"({len(res.unexpected_keys)})")
        return self

    @classmethod
    def from_checkpoint(cls, config, path: str, **kwargs):
        """app.py:304-316: a Lightning ``.ckpt`` (torch pickle with ``state_dict``) or a ``.safetensors`` file next to a
        config given by name / object."""
        cfg = config if isinstance(config, MIDIModelConfig) else MIDIModelConfig.from_name(config)
        trust = bool(kwargs.pop("trust_checkpoint", False))
        model = cls(cfg, **kwargs)
        if path.endswith(".safetensors"):
            from safetensors.torch import load_file
            state = load_file(path)
        else:
            import pickle
            try:
                state = torch.load(path, map_location="cpu", weights_only=True)
            except pickle.UnpicklingError as e:
                # the reference calls plain torch.load (app.py:314), which executes whatever the pickle names; a Lightning
                # .ckpt with callback / hyper-parameter objects outside torch's allow-list lands here
                # the trust is per call: the caller vouches for THIS file (no process-wide switch)
                if not trust:
                    raise RuntimeError(f"{path} holds pickled objects beyond tensors ({e}); re-save its state_dict alone, or pass "
                                       "from_checkpoint(..., trust_checkpoint=True) to unpickle it as the reference does (only "
                                       "for a file you trust: unpickling executes what the file names)") from e
                import warnings
                warnings.warn(f"from_checkpoint: unpickling {path} with weights_only=False (trust_checkpoint=True)", stacklevel=2)
                state = torch.load(path, map_location="cpu", weights_only=False)
        return model.load_checkpoint_state(state)
