"""One transformer block per training schedule against float64: the reference, the stand-in yardstick and the slice-wise measure
shared by tests/test_block_bounds_host.py (CPU) and tests/test_block_schedules_gpu.py (MI355X).

* ``block_fp64`` / ``tokfirst_fp64``: one pre-norm LLaMA block in torch float64 with autograd, on the bf16 operand values upcast;
  nothing else is rounded (cos / sin are RopeTable's float32 values upcast).
* ``run_case(case, device)``: the SAME engine.py block functions on ``device`` -- "cpu" under the stand-ins of tests/emu_ops.py /
  emu_packed.py (``standin_run``: fp32 arithmetic, rounded where the kernels store, plus the rounding points of the MFMA
  attention that those files do not model: attn_fwd_event, attn_bwd_event), "cuda" on the HIP kernels, with every operand
  between NaN guard rows and every gradient buffer NaN-filled.
* ``slice_distances``: relative L2 distance of the whole tensor, worst over its rows, worst over its columns (every slice divided
  by the same slice of the reference); vectors: whole distance and max|err| / max|ref|.
* ``check(device, standin, ref, margin)``: every distance of every tensor of the device run is at most ``margin`` x the stand-in's.
  The yardstick is never a device schedule.  MARGIN = 1.5 is the factor DESIGN.md section 2 grants over the reference's own bf16
  drift; the stand-in run, rounding where the kernels round, is that drift for one block.
"""
from __future__ import annotations

import functools
from dataclasses import dataclass
from typing import Dict, Tuple

import torch

from midi_model_amd import engine, ops, tokfirst

BF16, F32, F64 = torch.bfloat16, torch.float32, torch.float64
EPS, THETA = 1e-6, 10000.0
GUARD = 8                    # NaN rows (2-D) / elements (1-D) on either side of a guarded device tensor
MARGIN = 1.5
KEYS = ("wqkv", "wo", "wgu", "wd", "n1", "n2")
GRAD = {"wqkv": "dWqkv", "wo": "dWo", "wgu": "dWgu", "wd": "dWd", "n1": "dn1", "n2": "dn2"}
PAD_ID = 0
# a stand-in schedule's own distance to float64: every stored value passes ~10 bf16 rounding points of half an ulp (2^-9) each, summed
# linearly 10 x 2^-9 = 0.02; 2^-5 bounds it with room and is two orders below what a wrong convention (RoPE layout, mask, residual) gives
STANDIN_CAP = 2.0 ** -5


@dataclass(frozen=True)
class Case:
    name: str
    kind: str                       # "event" (head_dim 64) | "token" (head_dim 256)
    D: int
    H: int
    I: int
    B: int                          # sequences ...
    S: int                          # ... of S rows each (packed: unused)
    lengths: Tuple[int, ...] = ()   # packed batch: the sequences' lengths
    folded: bool = False
    lean: bool = False
    ndy: int = 1                    # 2: the backward runs a second time, accumulating, on a second dy
    chain: bool = False             # two blocks, the second taking parts_in from the first
    fp32: bool = False
    first: Tuple[int, int] = ()     # (N, V): the token-level first block per vocabulary entry (device); its stand-in is dense
    spread: bool = False            # the rows of x at scales 2^u, u uniform in [-1, 1] (overall std 1): rstd far from 1 in most rows
    seed: int = 1

    @property
    def M(self):
        return sum(self.lengths) if self.lengths else self.B * self.S

    @property
    def hd(self):
        return self.D // self.H

    def but(self, **kw):
        d = dict(self.__dict__)
        d.update(kw)
        return Case(**d)


EVENT = Case("event plain", "event", 256, 4, 1024, 2, 100)
TOKEN = Case("token plain", "token", 512, 2, 1024, 52, 8)
PACKED_LENGTHS = (33, 200, 7, 128, 129, 3)
CASES = {c.name: c for c in (
    EVENT,
    EVENT.but(name="event folded", folded=True),
    EVENT.but(name="event folded spread", folded=True, spread=True),
    EVENT.but(name="event folded splitk", folded=True, S=516),
    EVENT.but(name="event folded grouped", folded=True, D=1024, H=16, I=4096, S=132),
    EVENT.but(name="event folded chain", folded=True, chain=True),
    EVENT.but(name="event plain accumulate", ndy=2),
    EVENT.but(name="event folded accumulate", folded=True, ndy=2),
    EVENT.but(name="event plain lean", lean=True),
    EVENT.but(name="event folded lean", folded=True, lean=True),
    EVENT.but(name="packed plain", lengths=PACKED_LENGTHS, B=1, S=sum(PACKED_LENGTHS)),
    EVENT.but(name="packed folded", lengths=PACKED_LENGTHS, B=1, S=sum(PACKED_LENGTHS), folded=True),
    TOKEN,
    TOKEN.but(name="token folded", folded=True),
    TOKEN.but(name="token first", folded=True, B=300, first=(300, 200)),
    EVENT.but(name="event plain fp32", fp32=True),
    TOKEN.but(name="token plain fp32", D=512, fp32=True),
)}


# ------------------------------------------------------------------------------------------------------------------ inputs
def _values_key(case: Case) -> Case:
    """what the operand values and the float64 reference depend on: shapes, seed, accumulation, chaining -- not the schedule"""
    return case.but(name="", folded=False, lean=False, fp32=False)


def inputs(case: Case) -> dict:
    return _inputs(_values_key(case))


@functools.lru_cache(maxsize=None)
def _inputs(case: Case) -> dict:
    """Seeded bf16 values (CPU): weights std 0.02 .. 0.04, norm weights 1 +- 0.1, x std 1, dy std 1/64.  The fp32 cases run on
    the same values upcast.  Never modified by anyone: the runs copy."""
    g = torch.Generator().manual_seed(case.seed)
    D, I = case.D, case.I

    def r(shape, std, mean=0.0):
        return (mean + std * torch.randn(shape, generator=g)).to(BF16)
    ws = [dict(wqkv=r((3 * D, D), 0.04), wo=r((D, D), 0.03), wgu=r((2 * I, D), 0.03), wd=r((D, I), 0.02),
               n1=r((D,), 0.1, 1.0), n2=r((D,), 0.1, 1.0)) for _ in range(2 if case.chain else 1)]
    out = {"w": ws, "dys": [r((case.M, D), 1.0 / 64) for _ in range(case.ndy)]}
    if case.first:
        N, V = case.first
        T = tokfirst.TN
        hidden, table = r((N, D), 1.0), r((V, D), 1.0)
        # 15 ids never occur (V - 15 .. V - 1), id 5 occurs 1100 times (> tokfirst.SEG_OWN), the pad id 3 times, once in mid-sequence
        ids = torch.randint(1, V - 15, (N, T - 1), generator=g)
        flat = ids.view(-1)
        flat[torch.randperm(flat.numel(), generator=g)[:1110]] = 5
        ids[3, 2], ids[3, 3], ids[10, T - 2], ids[299, T - 2] = PAD_ID, 7, PAD_ID, PAD_ID
        assert int((ids == 5).sum()) >= 1100 > tokfirst.SEG_OWN and int((ids == PAD_ID).sum()) == 3
        occurs = torch.bincount(ids.view(-1), minlength=V) > 0
        assert int((~occurs).sum()) >= 10
        zero = ~occurs
        zero[PAD_ID] = True
        x = torch.empty((N, T, D), dtype=BF16)
        x[:, 0], x[:, 1:] = hidden, table[ids]
        out.update(hidden=hidden, table=table, ids=ids, zero_rows=zero, x=x.view(N * T, D))
    elif case.spread:
        # x std 1 in every row gives rstd = 1 +- 0.04: a row scale that is missed somewhere then moves its rows by 4 % of the
        # attention path's share of them, which no measure sees.  Rows at scales 0.5 .. 2 (E[4^u] = 1.352: overall std 1) show it.
        u = 2 * torch.rand((case.M, 1), generator=g) - 1
        out["x"] = (torch.randn((case.M, D), generator=g) * 2.0 ** u / 1.352 ** 0.5).to(BF16)
    else:
        out["x"] = r((case.M, D), 1.0)
    return out


def segments(case: Case):
    if case.lengths:
        a, segs = 0, []
        for n in case.lengths:
            segs.append((a, a + n))
            a += n
        return segs
    return [(b * case.S, (b + 1) * case.S) for b in range(case.B)]


# ------------------------------------------------------------------------------------------------------- float64 reference
def _rope_tables(hd, npos):
    """RopeTable's float32 cos / sin upcast (the values the engine holds), held to a float64 restatement of
    pos * theta^(-2i / hd): the table forms the angle in float32, so position p may be off by p * 2^-22 (+ one rounding) -- a wrong
    theta, pairing or position convention inside RopeTable is off by O(1) and would otherwise be shared by the reference."""
    t = engine.RopeTable(hd, THETA, "cpu", npos)
    ang = torch.arange(t.n, dtype=F64)[:, None] * THETA ** (-torch.arange(0, hd, 2, dtype=F64) / hd)[None, :]
    tol = (torch.arange(t.n, dtype=F64)[:, None] + 1) * 2.0 ** -22
    assert t.cos.shape == ang.shape and bool(((t.cos.double() - ang.cos()).abs() <= tol).all()) \
        and bool(((t.sin.double() - ang.sin()).abs() <= tol).all()), "RopeTable is not cos / sin of pos * theta^(-2i / hd)"
    return t.cos.double(), t.sin.double()


def _block64(w, x, segs, hd):
    """one block on float64 autograd tensors -> (x3, rstd1, rstd2)"""
    M, D = x.shape
    H, I = D // hd, w["wgu"].shape[0] // 2
    lens = [b - a for a, b in segs]
    pos = torch.cat([torch.arange(n) for n in lens])
    cos, sin = _rope_tables(hd, max(lens))
    c, s = cos[pos][:, None, :], sin[pos][:, None, :]

    def norm(v, wn):
        rstd = torch.rsqrt(v.pow(2).mean(-1) + EPS)
        return v * rstd[:, None] * wn, rstd

    def rot(v):
        v = v.reshape(M, H, hd)
        v1, v2 = v[..., : hd // 2], v[..., hd // 2:]
        return torch.cat([v1 * c - v2 * s, v2 * c + v1 * s], -1)

    def attend(q, k, v):          # [..., H, S, hd], causal
        S = q.shape[-2]
        sc = (q @ k.transpose(-1, -2)) * hd ** -0.5
        sc = sc.masked_fill(torch.triu(torch.ones(S, S, dtype=torch.bool), 1), float("-inf"))
        return torch.softmax(sc, -1) @ v

    h1, rstd1 = norm(x, w["n1"])
    qkv = h1 @ w["wqkv"].T
    q, k, v = rot(qkv[:, :D]), rot(qkv[:, D:2 * D]), qkv[:, 2 * D:].reshape(M, H, hd)
    if len(set(lens)) == 1:
        B, S = len(lens), lens[0]
        o = attend(*(t.view(B, S, H, hd).transpose(1, 2) for t in (q, k, v))).transpose(1, 2).reshape(M, D)
    else:
        o = torch.cat([attend(*(t[a:b].transpose(0, 1) for t in (q, k, v))).transpose(0, 1).reshape(b - a, D) for a, b in segs])
    x2 = x + o @ w["wo"].T
    h2, rstd2 = norm(x2, w["n2"])
    gu = h2 @ w["wgu"].T
    x3 = x2 + (torch.nn.functional.silu(gu[:, :I]) * gu[:, I:]) @ w["wd"].T
    return x3, rstd1, rstd2


def _chain64(kind, weights, x, dys, segs, extra_leaves=()):
    """blocks ``weights`` (a list) one after the other; parameter gradients for the SUM of ``dys``, dx for the last of them"""
    hd = 64 if kind == "event" else 256
    ws = [{k: v.double().requires_grad_(True) for k, v in w.items()} for w in weights]
    out, cur = {}, x
    for i, w in enumerate(ws):
        cur, r1, r2 = _block64(w, cur, segs, hd)
        p = f"{i}." if len(ws) > 1 else ""
        out.update({p + "x3": cur.detach(), p + "rstd1": r1.detach(), p + "rstd2": r2.detach()})
    leaves = [w[k] for w in ws for k in KEYS]
    total = sum(d.double() for d in dys)
    grads = torch.autograd.grad(cur, leaves + list(extra_leaves), total, retain_graph=True)
    for i in range(len(ws)):
        p = f"{i}." if len(ws) > 1 else ""
        for j, k in enumerate(KEYS):
            out[p + GRAD[k]] = grads[i * len(KEYS) + j]
    return out, cur, grads[len(leaves):]


def block_fp64(kind, weights, x, dy, B, S, seqs=None) -> Dict[str, torch.Tensor]:
    """One pre-norm LLaMA block in float64 with autograd: RMSNorm (eps 1e-6), q|k|v, half-split RoPE, causal softmax attention,
    o projection + residual, RMSNorm, SwiGLU, down projection + residual.  ``weights``: {wqkv, wo, wgu, wd, n1, n2} (a list of
    such: blocks chained, keys prefixed "0." / "1."); ``dy``: one tensor or a list (accumulation: parameter gradients of the sum,
    dx of the last); ``seqs``: a list of lengths -- attention and positions restart per sequence.
    -> x3, dx, dWqkv, dWo, dWgu, dWd, dn1, dn2, rstd1, rstd2"""
    weights = weights if isinstance(weights, list) else [weights]
    dys = dy if isinstance(dy, list) else [dy]
    case = Case("", kind, x.shape[1], 0, 0, B, S, tuple(seqs or ()))
    xl = x.double().requires_grad_(True)
    out, x3, _ = _chain64(kind, weights, xl, dys, segments(case))
    out["dx"] = torch.autograd.grad(x3, xl, dys[-1].double())[0]
    return out


def tokfirst_fp64(weights, hidden, table, ids, pad_id, dy) -> Dict[str, torch.Tensor]:
    """The same block over the rows  row 8n = hidden[n], row 8n + p = table[ids[n, p - 1]]  with ``hidden`` and ``table`` as
    leaves -> the block's outputs (without dx) + dhidden, dtable (row ``pad_id`` zero: nn.Embedding's padding row)"""
    N, D = hidden.shape
    T = tokfirst.TN
    hl, tl = hidden.double().requires_grad_(True), table.double().requires_grad_(True)
    x = torch.cat([hl[:, None, :], tl[ids[:, : T - 1]]], 1).reshape(N * T, D)
    case = Case("", "token", D, 0, 0, N, T)
    out, _, (dh, dt) = _chain64("token", [weights], x, [dy], segments(case), (hl, tl))
    dt = dt.clone()
    dt[pad_id] = 0
    out.update(dhidden=dh, dtable=dt)
    return out


def reference(case: Case) -> Dict[str, torch.Tensor]:
    """the float64 block on the inputs of ``case``, computed once per set of values and never modified"""
    return _reference(_values_key(case))


@functools.lru_cache(maxsize=None)
def _reference(case: Case) -> Dict[str, torch.Tensor]:
    inp = inputs(case)
    if case.first:
        return tokfirst_fp64(inp["w"][0], inp["hidden"], inp["table"], inp["ids"], PAD_ID, inp["dys"][0])
    return block_fp64(case.kind, inp["w"] if case.chain else inp["w"][0], inp["x"], inp["dys"], case.B, case.S, case.lengths)


# ---------------------------------------------------------------------------------------------------- the engine's schedules
def _guarded(t: torch.Tensor, device, fill_nan=False):
    """-> (whole allocation | None, the view that holds ``t``): on the device between GUARD NaN rows / elements"""
    if device == "cpu":
        return None, (torch.full_like(t, float("nan")) if fill_nan else t.clone())
    whole = torch.full((t.shape[0] + 2 * GUARD,) + tuple(t.shape[1:]), float("nan"), dtype=t.dtype, device=device)
    view = whole[GUARD:GUARD + t.shape[0]]
    if not fill_nan:
        view.copy_(t)
    return whole, view


def run_case(case: Case, device: str, dense: bool = False) -> Dict[str, torch.Tensor]:
    """The engine's block functions for ``case`` on ``device`` (the caller installs the stand-ins for "cpu") -> the tensors
    ``reference(case)`` names, on the CPU in the dtype they were stored in.  ``dense``: a ``first`` case as the dense folded
    schedule over its [8N, D] rows (-> dx in place of dhidden / dtable)."""
    inp = inputs(case)
    dtype = F32 if case.fp32 else BF16
    D, H, I = case.D, case.H, case.I
    nb = len(inp["w"])
    spec = engine.StackSpec("blk", D, H, I, nb, EPS, THETA, case.kind)
    fences = []

    def put(t, nan=False):
        whole, view = _guarded(t.to(dtype) if t.is_floating_point() else t, device, nan)
        if whole is not None:
            fences.append((whole, nan))
        return view
    lws = [engine.LayerTensors(**{k: put(w[k]) for k in KEYS}) for w in inp["w"]]
    lgs = [engine.LayerTensors(**{k: put(w[k], nan=True) for k in KEYS}) for w in inp["w"]]
    B, S = (1, case.M) if case.lengths else (case.B, case.S)
    seqs = ops.attn_seq_plan(case.lengths, H).upload(device) if case.lengths else None
    rope = engine.RopeTable(case.hd, THETA, device, max(case.lengths) if case.lengths else S)
    fold = engine.fold_norm_weights(engine.StackTensors(layers=lws)) if case.folded else None
    x = put(inp["x"])
    out = {}
    if case.first and not dense:
        N, V = case.first
        first = tokfirst.TokFirst(put(inp["hidden"]), inp["ids"].to(device), put(inp["table"]), PAD_ID)
        saved = []
        x3, _ = engine.tok_first_forward(spec, lws[0], fold[0], first, x, N, rope, saved, case.lean)
        keep = saved[0]
        g = engine.tok_first_backward(spec, lws[0], lgs[0], fold[0], keep, first, put(inp["dys"][0]), N, rope, False)
        rstd_rows = torch.cat([keep.rstd1[:N, None], keep.rstd1[N:N + V][first.ids[:, : tokfirst.TN - 1]]], 1).reshape(-1)
        out.update(x3=x3, rstd1=rstd_rows, rstd2=keep.rstd2, dhidden=g.dhidden, dtable=g.dtable32)
    else:
        keeps, cur, parts = [], x, None
        for li in range(nb):
            if case.folded:
                saved = []
                cur, parts = engine.layer_forward_folded(spec, lws[li], fold[li], cur, B, S, rope, parts, None, saved, case.lean, seqs)
                keeps.append(saved[0])
            else:
                cur, keep = engine.layer_forward(spec, lws[li], cur, B, S, rope, None, True, case.lean, seqs)
                keeps.append(keep)
            assert (keeps[-1].a is None) == case.lean and (keeps[-1].h1 is None) == case.folded
            p = f"{li}." if nb > 1 else ""
            out.update({p + "x3": cur, p + "rstd1": keeps[-1].rstd1, p + "rstd2": keeps[-1].rstd2})
        for j, dy in enumerate(inp["dys"]):
            dx = put(dy)
            for li in range(nb - 1, -1, -1):
                if case.folded:
                    dx = engine.layer_backward_folded(spec, lws[li], lgs[li], fold[li], keeps[li], dx, B, S, rope, j > 0, seqs)
                else:
                    dx = engine.layer_backward(spec, lws[li], lgs[li], keeps[li], dx, B, S, rope, j > 0, seqs)
        out["dx"] = dx
    for li in range(nb):
        p = f"{li}." if nb > 1 else ""
        out.update({p + GRAD[k]: getattr(lgs[li], k) for k in KEYS})
    if device != "cpu":
        torch.cuda.synchronize()
        for whole, was_nan in fences:
            w = whole.float()
            assert torch.isnan(w[:GUARD]).all() and torch.isnan(w[-GUARD:]).all(), f"{case.name}: a guard row was written"
            assert not torch.isnan(w[GUARD:-GUARD]).any(), f"{case.name}: NaN between the guards (a gradient never written?)"
    return {k: v.detach().cpu().clone() for k, v in out.items()}


def fold_dx_to_first(case: Case, dx: torch.Tensor):
    """the dense schedule's [8N, D] input gradient folded in float64: rows 8n -> dhidden, the others added by id into dtable, the
    pad row zero"""
    N, V = case.first
    T = tokfirst.TN
    d = dx.double().view(N, T, case.D)
    dtable = torch.zeros((V, case.D), dtype=F64)
    dtable.index_add_(0, inputs(case)["ids"].reshape(-1), d[:, 1:].reshape(-1, case.D))
    dtable[PAD_ID] = 0
    return d[:, 0].clone(), dtable


# Rounding points of the device that tests/emu_ops.py does not model; ``standin_run`` puts these two over it.
def attn_fwd_event(qkv, o, lse, B, S, H, scale):
    """emu_ops.attn_fwd with the MFMA forward's rounding point (bf16 only): the unnormalised P goes into P @ V as bf16, the row
    sum stays fp32"""
    import emu_ops
    if qkv.dtype != BF16:
        return emu_ops.attn_fwd(qkv, o, lse, B, S, H, scale)
    q, k, v = emu_ops._split(qkv, B, S, H, 64)
    s = emu_ops._causal_scores(q, k, scale)
    m = s.max(-1, keepdim=True).values
    p = torch.exp(s - m)
    l = p.sum(-1, keepdim=True)
    o.copy_(((p.to(BF16).float() @ v) / l).transpose(1, 2).reshape(B * S, H * 64).to(o.dtype))
    lse.view(B, H, ops.round_up(S, 64))[:, :, :S] = (m + l.log()).squeeze(-1)
    return o


def attn_bwd_event(qkv, o, dout, lse, dqkv, B, S, H, scale, cos_t=None, sin_t=None, rowscale=None):
    """emu_ops.attn_bwd with the MFMA backward's rounding points (bf16 only; attention_mfma3.hip): P from the stored lse,
    delta = rowsum(dO . O) from the STORED (bf16) O, the unscaled dS = P (dP - delta) and P rounded to bf16 before their products,
    the softmax scale applied to the fp32 sums"""
    import emu_ops
    if qkv.dtype != BF16:
        return emu_ops.attn_bwd(qkv, o, dout, lse, dqkv, B, S, H, scale, cos_t, sin_t, rowscale)
    q, k, v = emu_ops._split(qkv, B, S, H, 64)
    do, of = (t.float().view(B, S, H, 64).transpose(1, 2) for t in (dout, o))
    p = torch.exp(emu_ops._causal_scores(q, k, scale) - lse.view(B, H, ops.round_up(S, 64))[:, :, :S, None])
    ds = (p * (do @ v.transpose(-1, -2) - (do * of).sum(-1, keepdim=True))).to(BF16).float()
    grads = ((ds @ k) * scale, (ds.transpose(-1, -2) @ q) * scale, p.to(BF16).float().transpose(-1, -2) @ do)
    D = H * 64
    for i, t in enumerate(grads):
        t = t.transpose(1, 2).reshape(B * S, D)
        if rowscale is not None:
            t = t * rowscale.float()[:, None]
        dqkv[:, i * D:(i + 1) * D] = t.to(dqkv.dtype)
    if cos_t is not None:
        emu_ops.rope_(dqkv, cos_t, sin_t, S, 0, H, 64, -1)
    return dqkv


def standin_run_uncached(case: Case) -> Dict[str, torch.Tensor]:
    import emu_packed
    import midi_model_amd.ops as real
    g = globals()
    with emu_packed.install():
        over = {} if case.fp32 else {"attn_fwd": "attn_fwd_event", "attn_bwd": "attn_bwd_event"}
        saved = {n: getattr(real, n) for n in over}
        try:
            for n, mine in over.items():
                setattr(real, n, g[mine])        # (looked up now: test_block_bounds_host.py patches wrong kernels over them)
            out = run_case(case, "cpu", dense=True)
        finally:
            for n, f in saved.items():
                setattr(real, n, f)
    if case.first:
        out["dhidden"], out["dtable"] = fold_dx_to_first(case, out.pop("dx"))
    return out


@functools.lru_cache(maxsize=None)
def standin_run(case: Case) -> Dict[str, torch.Tensor]:
    """``case`` through the same engine functions on the CPU under emu_ops / emu_packed (fp32 arithmetic, rounded where the kernels
    store); the context is left before anything else runs.  A ``first`` case: the dense folded schedule, its input gradient folded
    to dhidden / dtable in float64."""
    return standin_run_uncached(case)


# ------------------------------------------------------------------------------------------------------------- the measure
def slice_distances(got: torch.Tensor, ref: torch.Tensor, zero_rows=None) -> Dict[str, float]:
    """2-D: {"all": relative L2 of the whole tensor, "row": worst over rows, "col": worst over columns}, every slice divided by
    the norm of the same slice of ``ref``; vectors: {"all", "max": max|err| / max|ref|}.  No slice is left out and every
    reference slice must have a non-zero norm -- except ``zero_rows`` (bool [rows]: table rows no id names, the pad row), where
    the reference is exactly zero and ``got`` must hold exact zeros."""
    g, r = got.double(), ref.double()
    assert g.shape == r.shape and torch.isfinite(g).all() and torch.isfinite(r).all(), (got.shape, ref.shape)
    e = g - r
    if r.dim() == 1:
        assert zero_rows is None and float(r.abs().max()) > 0
        return {"all": float(e.norm() / r.norm()), "max": float(e.abs().max() / r.abs().max())}
    rows = torch.ones(r.shape[0], dtype=torch.bool) if zero_rows is None else ~zero_rows
    if zero_rows is not None:
        assert float(r[zero_rows].abs().max()) == 0, "zero_rows: the reference is not zero there"
        assert float(g[zero_rows].abs().max()) == 0, "a table row without occurrences (or the pad row) is not exactly zero"
    rn, cn = r[rows].norm(dim=1), r.norm(dim=0)
    assert float(rn.min()) > 0 and float(cn.min()) > 0, "a reference slice with zero norm"
    return {"all": float(e.norm() / r.norm()), "row": float((e[rows].norm(dim=1) / rn).max()), "col": float((e.norm(dim=0) / cn).max())}


def check(device, standin, ref, margin=MARGIN, zero_rows=None, tag="", raise_on_fail=True):
    """For every tensor of ``ref`` and every one of its distances: d(device) <= margin * d(standin).  ``margin``: a number, or
    {tensor name: number} over the default MARGIN.  Every triple is printed.  -> [(tensor, kind, d_device, d_standin, ratio, ok)]"""
    zero_rows = zero_rows or {}
    rows = []
    assert set(ref) <= set(device) and set(ref) <= set(standin), (sorted(ref), sorted(device), sorted(standin))
    for name in sorted(ref):
        m = margin.get(name.split(".")[-1], MARGIN) if isinstance(margin, dict) else margin
        dd = slice_distances(device[name], ref[name], zero_rows.get(name))
        ds = slice_distances(standin[name], ref[name], zero_rows.get(name))
        for kind in dd:
            ratio = dd[kind] / ds[kind] if ds[kind] > 0 else (0.0 if dd[kind] == 0 else float("inf"))
            ok = dd[kind] <= m * ds[kind]
            rows.append((name, kind, dd[kind], ds[kind], ratio, ok))
            print(f"{tag:24s} {name:10s} {kind:3s}  device {dd[kind]:.3e}  stand-in {ds[kind]:.3e}  ratio {ratio:6.3f}  margin {m:.3f}"
                  f"{'' if ok else '   <-- FAILS'}")
    bad = [(n, k, f"{a:.3e}", f"{b:.3e}", f"{q:.3f}") for n, k, a, b, q, ok in rows if not ok]
    if raise_on_fail:
        assert not bad, f"{tag}: (tensor, slice kind, device, stand-in, ratio) over the margin: {bad}"
    return rows


def same_bits(a: Dict[str, torch.Tensor], b: Dict[str, torch.Tensor]):
    assert set(a) == set(b)
    for k in a:
        assert a[k].dtype == b[k].dtype and torch.equal(a[k].view(torch.int16 if a[k].dtype == BF16 else torch.int32),
                                                        b[k].view(torch.int16 if b[k].dtype == BF16 else torch.int32)), k
