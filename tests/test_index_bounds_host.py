"""CPU proof that the checks of tests/test_index_kernels_gpu.py bite: the checks of tests/ref_index.py, at the GPU test's own
inputs (for a grid-cap case a slice from the same generator), accept emu_ops (and the torch stand-ins of
tests/test_tokfirst_host.py for the three entry points emu_ops does not restate) and reject named wrong kernels restated in
torch.  Also: the float64 reference rounded once meets every random-value bound (the bounds were derived, not tuned), and the
augment branch census is complete for both tokenizer versions."""
import pytest
import torch

import emu_ops as emu
import ref_index as R
from ref_index import BF16, F32, F64
from test_tokfirst_host import STANDINS

DTYPES = [BF16, F32]


class Emu:
    """emu_ops behind the backend interface of ref_index's checks; `wrong` names the wrong kernel it plays instead"""
    dev = "cpu"

    def __init__(self, wrong=None):
        self.wrong = wrong

    # ---- embeddings
    def embed_sum(self, tok, table, out):
        w, D = self.wrong, table.shape[1]
        if w == "last token of the octet dropped":
            tok = tok[:, :-1]
        if w == "TT > 8 tail ignored":
            tok = tok[:, :8]
        if w == "bf16 rounding after every add":
            acc = torch.zeros_like(out)
            for j in range(tok.shape[1]):
                acc = (acc.float() + table[tok[:, j]].float()).to(torch.bfloat16).to(out.dtype)
            return out.copy_(acc)
        if w == "columns past the last whole chunk left unwritten":
            Dw = D // (64 * R.NVEC[out.dtype]) * (64 * R.NVEC[out.dtype])
            return out[:, :Dw].copy_(table[tok].float().sum(1).to(out.dtype)[:, :Dw])
        tmp = torch.empty(out.shape, dtype=out.dtype)
        return out.copy_(emu.embed_sum_fwd(tok, table, tmp))

    def concat(self, hidden, tok, table, out, T):
        M, V = hidden.shape[0], table.shape[0]
        if self.wrong == "token column shifted by one":
            tok = torch.as_strided(tok, tok.shape, tok.stride(), tok.storage_offset() + 1) % V
        if self.wrong == "ldtok ignored":
            tok = torch.as_strided(tok, tok.shape, (T - 1, 1), tok.storage_offset()) % V
        return emu.concat_tok_fwd(hidden, tok, table, out, T)

    def scatter(self, tok, T, dout, rpm, js, j0, dtab, pad):
        if self.wrong == "pad row not skipped":
            pad = -1
        if self.wrong == "last partial chunk skipped":
            return self._chunks_only(lambda d: emu.embed_scatter_bwd(tok, T, dout, rpm, js, j0, d, pad), dtab, dout.dtype)
        emu.embed_scatter_bwd(tok, T, dout, rpm, js, j0, dtab, pad)

    @staticmethod
    def _chunks_only(run, tab, dtype):
        D = tab.shape[1]
        Dw = D // (64 * R.NVEC[dtype]) * (64 * R.NVEC[dtype])
        full = tab.clone()
        run(full)
        tab[:, :Dw] = full[:, :Dw]

    def _segment(self, src, seg, x, ld, tab, n_occ, pad):
        """the sum of both segment entry points: x the flat rows (row stride ld), tab a [V, D] view of fp32"""
        w = self.wrong
        V, D = tab.shape
        n_in = min(int(seg[V]), n_occ)                       # (occurrences behind seg_start[V]: skipped)
        if w == "ld taken as D":
            ld = D
        if w == "occurrences behind seg_start[V] added to row V - 1":
            seg = seg.clone()
            seg[V], n_in = n_occ, n_occ
        if w == "one occurrence per 128-piece dropped":
            keep = torch.arange(n_in) % 128 != 5
            cnt = torch.zeros(V + 1, dtype=torch.int64)
            cnt[1:] = torch.cumsum(torch.bincount(torch.repeat_interleave(torch.arange(V), seg[1:] - seg[:-1])[keep], minlength=V), 0)
            src, seg, n_in = src[:n_in][keep], cnt, int(keep.sum())
        src = src[:n_in]
        add = torch.zeros((V, D), dtype=torch.float32)
        if n_in:
            emu.embed_segment_bwd(src, seg, x, ld, add, pad)
        n = seg[1:] - seg[:-1]
        if w == "long segment's middle group written twice":
            for v in torch.nonzero(n > R.SEG_OWN).flatten().tolist():
                a = int(seg[v])
                rows = torch.as_strided(x, (int(src.max()) + 1, D), (ld, 1), x.storage_offset()).float()
                if v != pad:
                    add[v] += rows[src[a + 1024: min(a + 2048, int(seg[v + 1]))]].sum(0)
        if w == "last partial chunk skipped":
            add[:, D // (64 * R.NVEC[x.dtype]) * (64 * R.NVEC[x.dtype]):] = 0
        if w == "owned segment overwrites instead of adds":
            own = (n > 0) & (n <= R.SEG_OWN)
            if pad >= 0:
                own[pad] = False
            tab[own] = 0
        tab += add

    def segment_bwd(self, src, seg, x, ld, tab, n_occ, pad):
        self._segment(src, seg, x, ld, tab, n_occ, -1 if self.wrong == "pad row not skipped" else pad)

    def segment_sum(self, src, seg, rows, tab, n_occ):
        if self.wrong is None:
            assert n_occ == src.numel()
            return STANDINS["segment_sum"](src, seg, rows, tab)
        base = torch.as_strided(rows, (rows.shape[0] * rows.stride(0),), (1,), rows.storage_offset())
        self._segment(src, seg, base, rows.stride(0), tab, n_occ, 0 if self.wrong == "pad skipped in segment_sum" else -1)

    def split_hi_lo(self, s, hi, lo):
        STANDINS["split_hi_lo"](s, hi, lo)
        if self.wrong == "lo not written":
            lo.zero_()
        if self.wrong == "hi truncated":
            hi.copy_((R.bits(s) & -65536).view(F32).to(hi.dtype) if hi.dtype == BF16 else s * (1 - 2.0 ** -23))

    def table_norm_bwd(self, t_hi, t_lo, e, rstd, acc, pad):
        w = self.wrong
        if w == "t_lo ignored":
            t_lo = torch.zeros_like(t_lo)
        if w == "rstd not squared":
            rstd = rstd.sqrt()
        V = e.shape[0]
        ext = lambda t: torch.cat([t, t[:1]])       # one spare row for the stand-in to skip when the entry point skips none
        a = ext(acc)
        STANDINS["table_norm_bwd"](ext(t_hi), ext(t_lo), ext(e), ext(rstd), a, pad if pad >= 0 and w != "pad row not skipped" else V)
        a = a[:V]
        if w == "last partial chunk skipped":
            Dw = e.shape[1] // (64 * R.NVEC[e.dtype]) * (64 * R.NVEC[e.dtype])
            a[:, Dw:] = acc[:, Dw:]
        acc.copy_(a)

    # ---- index preparation
    def token_segments(self, tok, V, row_mul, col_mul, add, src_out, seg_out):
        w = self.wrong
        if w == "row_mul / col_mul swapped":
            row_mul, col_mul = col_mul, row_mul
        bucket = torch.where((tok >= 0) & (tok < V), tok, torch.full_like(tok, V))   # (emu_ops takes in-range ids only)
        src, seg = emu.token_segments(bucket, V, row_mul, col_mul, add)
        if w == "seg_start[V] missing the last bucket":
            seg[V] = seg[V - 1]
        if w == "out-of-range ids dropped":
            src_out[: int(seg[V])] = src[: int(seg[V])]
        else:
            src_out.copy_(src)
        seg_out.copy_(seg)

    def transpose(self, x, out):
        R_, C = x.shape
        nv = R.NVEC[x.dtype]
        tmp = emu.transpose(x, torch.empty((C, R_), dtype=x.dtype))
        scalar = bool(out.stride(0) % nv or out.storage_offset() % nv)
        if self.wrong == "scalar-path last column dropped" and scalar:
            out[:, : R_ - 1] = tmp[:, : R_ - 1]
            return
        out.copy_(tmp)
        if self.wrong == "tail tile zero-filled into the output gap" and R_ % nv:
            torch.as_strided(out, (C, 1), out.stride(), out.storage_offset() + R_).zero_()

    # ---- batch assembly
    def collate(self, tokens, start, length, out, pad_id):
        B, L, T = out.shape
        if self.wrong == "window off by one at the corpus end":
            start = torch.where(start + length == tokens.shape[0], start - 1, start)
        emu.collate_windows(tokens, start, length, out, pad_id)
        if self.wrong == "pad region reads the following events":
            idx = (start[:, None] + torch.arange(L)[None, :]).clamp(max=tokens.shape[0] - 1)
            out.copy_(tokens[idx].long())

    def piece_stats(self, tokens, off, tab, stats):
        if self.wrong == "rule (1) counting drum notes":
            return stats.copy_(R.piece_stats_ref(tokens, off, tab, count_drums=True))
        emu.augment_piece_stats(tokens, off, tab, stats)

    def augment_collate(self, tokens, start, length, piece, sh, stats, tab, out, pad_id):
        if self.wrong in R.AUGMENT_WRONG:
            return out.copy_(R.augment_ref(tokens, start, length, piece, sh, stats, tab, out.shape[1], pad_id, wrong=self.wrong))
        emu.augment_collate_windows(tokens, start, length, piece, sh, stats, tab, out, pad_id)


def rejects(check, wrongs, cases):
    """every case accepted from emu_ops; -> {wrong kernel: number of cases that reject it}"""
    rej = {w: 0 for w in wrongs}
    for case in cases:
        assert check(Emu(), *case) == 0, case
        for w in wrongs:
            rej[w] += check(Emu(w), *case) > 0
    return rej


# ------------------------------------------------------------------------------------------------------------------- embed_sum
EMBED_SUM_WRONG = ["last token of the octet dropped", "TT > 8 tail ignored", "columns past the last whole chunk left unwritten",
                   "bf16 rounding after every add"]


def test_embed_sum_checks_accept_the_emulation_and_reject_wrong_kernels():
    """bf16 rounding after every add keeps every integer partial sum: the exact family cannot see it (asserted), the
    random-value bound does"""
    cases = R.EMBED_SUM_CASES
    exact = rejects(lambda be, *c: R.check_embed_sum(be, *c, True), EMBED_SUM_WRONG, cases)
    rand = rejects(lambda be, *c: R.check_embed_sum(be, *c, False), EMBED_SUM_WRONG, cases)
    n_tail = sum(1 for c in cases if c[1] > 8)
    n_part = sum(1 for c in cases if c[2] % (64 * R.NVEC[c[3]]))
    assert exact["bf16 rounding after every add"] == 0 and rand["bf16 rounding after every add"] >= 4, (exact, rand)
    for r in (exact, rand):
        assert r["last token of the octet dropped"] == len(cases), r
        assert r["TT > 8 tail ignored"] == n_tail, r
        assert r["columns past the last whole chunk left unwritten"] == n_part, r
    M, TT, D = R.EMBED_SUM_CAP
    assert R.check_embed_sum(Emu(), M // 64, TT, D, BF16, True, seed=1) == 0


def test_concat_check_accepts_the_emulation_and_rejects_wrong_kernels():
    rej = rejects(R.check_concat, ["token column shifted by one", "ldtok ignored"], R.CONCAT_CASES)
    n_tok = sum(1 for c in R.CONCAT_CASES if c[1] > 1)
    assert rej["token column shifted by one"] == n_tok and rej["ldtok ignored"] == n_tok, rej
    M, T, D = R.CONCAT_CAP
    assert R.check_concat(Emu(), M // 64, T, D, BF16, seed=1) == 0


# --------------------------------------------------------------------------------------------------------- scatter and segments
@pytest.mark.parametrize("exact", [True, False])
def test_scatter_check_accepts_the_emulation_and_rejects_wrong_kernels(exact):
    rej = rejects(lambda be, *c: R.check_scatter(be, *c, exact), ["pad row not skipped", "last partial chunk skipped"], R.SCATTER_CASES)
    assert rej["pad row not skipped"] == sum(1 for c in R.SCATTER_CASES if c[5] >= 0), rej
    assert rej["last partial chunk skipped"] == sum(1 for c in R.SCATTER_CASES if c[2] % (64 * R.NVEC[c[3]])), rej
    M, T, D, dt, seq, pad, one = R.SCATTER_CAP
    assert R.check_scatter(Emu(), M // 64, T, D, dt, seq, pad, one, exact, seed=1) == 0


SEGMENT_WRONG = ["pad row not skipped", "pad skipped in segment_sum", "one occurrence per 128-piece dropped",
                 "owned segment overwrites instead of adds", "occurrences behind seg_start[V] added to row V - 1", "ld taken as D",
                 "last partial chunk skipped", "long segment's middle group written twice"]


@pytest.mark.parametrize("exact", [True, False])
def test_segment_checks_accept_the_emulation_and_reject_wrong_kernels(exact):
    cases = R.SEG_SMALL_CASES
    rej = rejects(lambda be, *c: R.check_segment(be, *c, exact), SEGMENT_WRONG, cases)
    has = {d: R.seg_distributions(4095)[d] for d in R.SEG_DISTS}
    padded = lambda c: any(v == has[c[1]][2] for v, _ in has[c[1]][0])
    assert rej["pad row not skipped"] == sum(1 for c in cases if c[0] == "bwd" and padded(c)), rej
    assert rej["pad skipped in segment_sum"] == sum(1 for c in cases if c[0] == "sum" and any(v == 0 for v, _ in has[c[1]][0])), rej
    def drops(c):       # a dropped position (5 mod 128) that holds an occurrence the operation adds
        ids = [v for v, n in has[c[1]][0] for _ in range(n)]
        return any(c[0] == "sum" or ids[p] != has[c[1]][2] for p in range(5, len(ids), 128))
    assert rej["one occurrence per 128-piece dropped"] == sum(1 for c in cases if drops(c)), rej
    assert rej["owned segment overwrites instead of adds"] == len(cases), rej
    assert rej["occurrences behind seg_start[V] added to row V - 1"] == sum(1 for c in cases if has[c[1]][1]), rej
    assert rej["ld taken as D"] == sum(1 for c in cases if c[1] != "n1"), rej      # (one occurrence: row 0 lies where it lay)
    assert rej["last partial chunk skipped"] == sum(1 for c in cases if c[3] % (64 * R.NVEC[c[4]])), rej
    assert rej["long segment's middle group written twice"] >= sum(1 for c in cases if c[1] in ("long", "own")), rej


def test_segment_dispatch_class_cases_accept_the_emulation():
    """the wide cases of the GPU test, emulation only (the wrong kernels are shown at the narrow ones)"""
    for c in R.SEG_CLASS_CASES:
        assert R.check_segment(Emu(), *c) == 0, c


class Ref64(Emu):
    """the float64 reference rounded once to the output type: what every random-value bound must admit"""

    def embed_sum(self, tok, table, out):
        out.copy_(table[tok].double().sum(1).to(out.dtype))

    def scatter(self, tok, T, dout, rpm, js, j0, dtab, pad):
        rows = torch.arange(tok.shape[0])[:, None] * rpm + torch.arange(T)[None, :] * js + j0
        keep = tok != pad
        dtab.copy_(dtab.double().index_add_(0, tok[keep], dout.double()[rows[keep]]).float())

    def _segment(self, src, seg, x, ld, tab, n_occ, pad):
        V, D = tab.shape
        n_in = int(seg[V])
        rows = torch.as_strided(x, (x.numel() // ld if x.dim() == 1 else x.shape[0], D), (ld, 1), x.storage_offset()).double()
        ids = torch.repeat_interleave(torch.arange(V), seg[1:] - seg[:-1])
        keep = ids != pad
        tab.copy_(tab.double().index_add_(0, ids[keep], rows[src[:n_in][keep]]).float())

    def segment_sum(self, src, seg, rows, tab, n_occ):
        self._segment(src, seg, torch.as_strided(rows, (rows.shape[0] * rows.stride(0),), (1,), rows.storage_offset()), rows.stride(0), tab, n_occ, -1)

    def table_norm_bwd(self, t_hi, t_lo, e, rstd, acc, pad):
        Tt, e64 = t_hi.double() + t_lo.double(), e.double()
        d = Tt - e64 * (rstd.double() ** 2 * (Tt * e64).sum(-1) / e.shape[1])[:, None]
        if pad >= 0:
            d[pad] = 0
        acc.copy_((acc.double() + d).float())


def test_random_value_bounds_hold_for_the_rounded_float64_reference():
    be = Ref64()
    for c in R.EMBED_SUM_CASES:
        assert R.check_embed_sum(be, *c, False) == 0, c
    for c in R.SCATTER_CASES:
        assert R.check_scatter(be, *c, False) == 0, c
    for c in R.SEG_SMALL_CASES:
        assert R.check_segment(be, *c, False) == 0, c
    for c in R.TABLE_NORM_CASES:
        assert R.check_table_norm(be, *c) == 0, c


# --------------------------------------------------------------------------------------------------- split_hi_lo and table_norm
@pytest.mark.parametrize("dtype", DTYPES)
def test_split_check_accepts_the_emulation_and_rejects_wrong_kernels(dtype):
    cases = [(n, dtype, ex) for n in (4, 1028, R.SPLIT_CAP // 64 // 4 * 4) for ex in (True, False)]
    rej = rejects(R.check_split, ["lo not written", "hi truncated"], cases)
    assert rej["hi truncated"] >= 2 and (dtype == F32 or rej["lo not written"] >= 2), rej


def test_table_norm_check_accepts_the_emulation_and_rejects_wrong_kernels():
    rej = rejects(R.check_table_norm, ["pad row not skipped", "t_lo ignored", "rstd not squared", "last partial chunk skipped"], R.TABLE_NORM_CASES)
    assert rej["pad row not skipped"] == sum(1 for c in R.TABLE_NORM_CASES if c[3] >= 0), rej
    assert rej["t_lo ignored"] == len(R.TABLE_NORM_CASES) and rej["rstd not squared"] == len(R.TABLE_NORM_CASES), rej
    assert rej["last partial chunk skipped"] == sum(1 for c in R.TABLE_NORM_CASES if c[1] % (64 * R.NVEC[c[2]])), rej
    V, D = R.TABLE_NORM_CAP
    for pad in (0, V // 64 - 1, -1):
        assert R.check_table_norm(Emu(), V // 64, D, BF16, pad, seed=1) == 0


# -------------------------------------------------------------------------------------------------- token_segments and transpose
def test_token_segments_check_accepts_the_emulation_and_rejects_wrong_kernels():
    wrongs = ["seg_start[V] missing the last bucket", "out-of-range ids dropped", "row_mul / col_mul swapped"]
    rej = rejects(R.check_token_segments, wrongs, R.TOKSEG_CASES)
    assert rej["seg_start[V] missing the last bucket"] == len(R.TOKSEG_CASES), rej
    assert rej["out-of-range ids dropped"] == sum(1 for c in R.TOKSEG_CASES if c[3] == "mixed" and c[0] * c[1] >= 4), rej
    assert rej["row_mul / col_mul swapped"] == sum(1 for c in R.TOKSEG_CASES if c[0] * c[1] > 1), rej
    assert R.SEG_CH == 2048 and R.SEG_OWN == 1024     # what the case lists above were laid out for; they follow the sources


@pytest.mark.parametrize("dtype", DTYPES)
def test_transpose_check_accepts_the_emulation_and_rejects_wrong_kernels(dtype):
    cases = [(R_, C, dtype, v) for R_, C in R.TRANSPOSE_SHAPES for v in R.TRANSPOSE_VARIANTS]
    rej = rejects(R.check_transpose, ["tail tile zero-filled into the output gap", "scalar-path last column dropped"], cases)
    assert rej["tail tile zero-filled into the output gap"] == sum(1 for c in cases if c[0] % R.NVEC[dtype]), rej
    assert rej["scalar-path last column dropped"] == len(R.TRANSPOSE_SHAPES), rej


# --------------------------------------------------------------------------------------------------------------- batch assembly
def test_collate_check_accepts_the_emulation_and_rejects_wrong_kernels():
    rej = rejects(R.check_collate, ["pad region reads the following events", "window off by one at the corpus end"], R.COLLATE_CASES)
    assert rej["window off by one at the corpus end"] == len(R.COLLATE_CASES), rej
    assert rej["pad region reads the following events"] == sum(1 for c in R.COLLATE_CASES if any(n < c[2] for _, n in c[3])), rej
    T, B, L, wins, pad = R.COLLATE_CAP
    assert R.check_collate(Emu(), T, B, L, wins, pad, slice_b=B // 64) == 0


@pytest.mark.parametrize("ver", ["v1", "v2"])
def test_augment_checks_accept_the_emulation_and_reject_wrong_kernels(orc, ver):
    tok = R.tokenizer(ver)
    assert R.check_piece_stats(Emu(), tok) == 0
    assert R.check_augment(Emu(), tok, orc) == 0
    assert R.check_augment_cap(Emu(), tok, slice_b=R.AUGMENT_CAP_ROWS // 13 // 256) == 0
    for w in R.AUGMENT_WRONG + ("rule (1) counting drum notes",):
        if ver == "v1" and w.startswith("rule (2)"):
            continue                                  # (v1 has no key signatures)
        assert R.check_augment(Emu(w), tok, orc) > 0, w
    assert R.check_piece_stats(Emu("rule (1) counting drum notes"), tok) > 0


@pytest.mark.parametrize("ver", ["v1", "v2"])
def test_augment_branch_census_is_complete(ver):
    tok = R.tokenizer(ver)
    pieces, shifts = R.augment_corpus(tok)
    wins, L = R.augment_windows(pieces)
    c = R.augment_census(tok, pieces, shifts, [w[2] for w in wins], L)
    assert c["unchanged: a pitch below 0"] == 1 and c["unchanged: a pitch above 127"] == 1
    assert sum(len(p) for p in pieces) < 1000
