"""The index-driven kernels on the MI355X at their edges: mh_embed_sum_fwd, mh_concat_tok_fwd, mh_embed_scatter_bwd,
mh_embed_segment_bwd, mh_embed_segment_sum, mh_embed_split_hi_lo, mh_embed_table_norm_bwd, mh_token_segments, mh_transpose,
mh_collate_windows, mh_augment_piece_stats, mh_augment_collate_windows -- together every training step's input batch, its
embedding and the whole embedding-table gradient.  The checks, their references and their bounds are tests/ref_index.py's:
integer operands for which every correct kernel returns the same bits as the int64 reference, random operands against float64
with derived bounds, outputs in fenced views, NaN or a telling id in everything the operation must not read.  Shapes are the
smallest that reach each edge: one lane active, a partial and a whole last chunk, the octet loop and the generic loop of
embed_sum, every chunk count x LDS / global seg_start x 8 / 4 / 1 waves of the segment kernels, pieces of exactly 128 and 1024
occurrences, segments of SEG_OWN - 1 / SEG_OWN / SEG_OWN + 1, ids outside [0, V) behind seg_start[V], the scalar fallbacks of
the transpose, and one launch per grid cap so that every `+= gridDim.x` loop takes its second pass.

Every check is a function of a backend (`Hip` below: the C ABI on the device, every argument spelled out).
tests/test_index_bounds_host.py runs the same checks at the same inputs on the CPU against emu_ops and against named wrong
kernels, which they reject.

Not covered: n_occ >= 2^31 (refused by the entry points; positions are 32-bit) and index arithmetic past 2^31 elements in
general (the largest output here is 268 MB); V >= 16000 for mh_token_segments (refused: the counters of one id per LDS word) and
V >= 2^30 for the segment kernels; the deliberate trap of mh_embed_sum_fwd / mh_concat_tok_fwd on an id outside [0, V), which
no test may provoke; D > 1024 for embed_sum / concat / scatter / table_norm (their column loop is the same code at any trip
count); more than 65535 column slabs or row tiles; tokenizers other than the two versions' tables."""
import pytest
import torch

import ref_index as R
from ref_index import BF16, F32

pytestmark = pytest.mark.gpu


class Hip:
    """the C-ABI of libmidihip.so on the device, every argument spelled out (no wrapper of midi_model_amd.ops in between)"""
    dev = "cuda"

    def __init__(self):
        from midi_model_amd.lib import lib
        self._lib = lib

    def call(self, name, *args):
        self._lib().call(name, *args, torch.cuda.current_stream().cuda_stream)

    @staticmethod
    def p(t):
        return t.data_ptr()

    @staticmethod
    def dt(t):
        return 1 if t.dtype == BF16 else 0

    def embed_sum(self, tok, table, out):
        assert tok.is_contiguous() and table.is_contiguous() and out.is_contiguous()
        self.call("mh_embed_sum_fwd", self.p(tok), self.p(table), self.p(out), tok.shape[0], tok.shape[1], table.shape[0], table.shape[1], self.dt(table))

    def concat(self, hidden, tok, table, out, T):
        assert hidden.is_contiguous() and table.is_contiguous() and out.is_contiguous() and (T == 1 or tok.stride(1) == 1)
        self.call("mh_concat_tok_fwd", self.p(hidden), self.p(tok), tok.stride(0), self.p(table), self.p(out), hidden.shape[0], T, table.shape[0],
                  table.shape[1], self.dt(table))

    def scatter(self, tok, T, dout, rpm, js, j0, dtab, pad):
        assert tok.stride(1) == 1 and dout.is_contiguous() and dtab.is_contiguous() and dtab.dtype == F32
        self.call("mh_embed_scatter_bwd", self.p(tok), tok.stride(0), T, self.p(dout), rpm, js, j0, self.p(dtab), tok.shape[0], dtab.shape[0],
                  dtab.shape[1], pad, self.dt(dout))

    def segment_bwd(self, src, seg, x, ld, tab, n_occ, pad):
        assert tab.is_contiguous() and tab.dtype == F32 and seg.numel() == tab.shape[0] + 1 and src.numel() == n_occ
        self.call("mh_embed_segment_bwd", self.p(src), self.p(seg), self.p(x), ld, self.p(tab), tab.shape[0], tab.shape[1], n_occ, pad, self.dt(x))

    def segment_sum(self, src, seg, rows, tab, n_occ):
        assert rows.stride(1) == 1 and tab.stride(1) == 1 and tab.dtype == F32 and src.numel() == n_occ
        self.call("mh_embed_segment_sum", self.p(src), self.p(seg), self.p(rows), rows.stride(0), self.p(tab), tab.stride(0), tab.shape[0], tab.shape[1],
                  n_occ, self.dt(rows))

    def split_hi_lo(self, s, hi, lo):
        self.call("mh_embed_split_hi_lo", self.p(s), self.p(hi), self.p(lo), s.numel(), self.dt(hi))

    def table_norm_bwd(self, t_hi, t_lo, e, rstd, acc, pad):
        self.call("mh_embed_table_norm_bwd", self.p(t_hi), self.p(t_lo), self.p(e), self.p(rstd), self.p(acc), e.shape[0], e.shape[1], pad, self.dt(e))

    def token_segments(self, tok, V, row_mul, col_mul, add, src, seg):
        n_rows, n_cols = tok.shape
        chunk = self._lib().cdll.mh_token_segments_chunk()
        assert chunk == R.SEG_CH
        wbuf, work = R.fenced(((((n_rows * n_cols + chunk - 1) // chunk) + 1) * (V + 1),), torch.int32, self.dev)
        w0 = wbuf.clone()
        self.call("mh_token_segments", self.p(tok), tok.stride(0), n_rows, n_cols, V, row_mul, col_mul, add, self.p(src), self.p(seg), self.p(work))
        assert R.stray(wbuf, w0, work) == 0, "mh_token_segments wrote outside its scratch"

    def transpose(self, x, out):
        self.call("mh_transpose", self.p(x), x.stride(0), self.p(out), out.stride(0), x.shape[0], x.shape[1], self.dt(x))

    def collate(self, tokens, start, length, out, pad_id):
        B, L, T = out.shape
        assert tokens.is_contiguous() and tokens.shape[1] == T
        self.call("mh_collate_windows", self.p(tokens), tokens.shape[0], self.p(start), self.p(length), self.p(out), B, L, T, pad_id)

    def piece_stats(self, tokens, off, tab, stats):
        self.call("mh_augment_piece_stats", self.p(tokens), self.p(off), off.numel() - 1, self.p(tab), self.p(stats))

    def augment_collate(self, tokens, start, length, piece, sh, stats, tab, out, pad_id):
        B, L, T = out.shape
        assert tokens.is_contiguous() and sh.is_contiguous() and stats.is_contiguous() and sh.shape == (B, 6)
        self.call("mh_augment_collate_windows", self.p(tokens), tokens.shape[0], self.p(start), self.p(length), self.p(piece), self.p(sh), self.p(stats),
                  self.p(tab), self.p(out), B, L, T, pad_id)


@pytest.fixture(scope="module")
def be():
    return Hip()


def run(check, be, cases, *tail):
    """every case; the failing ones with their counts of bad elements"""
    failed = {}
    for c in cases:
        n = check(be, *c, *tail)
        if n:
            failed[str(c)] = n
    assert not failed, failed


# -------------------------------------------------------------------------------------------------------------------- embeddings
@pytest.mark.parametrize("exact", [True, False], ids=["exact", "fp64"])
def test_embed_sum(be, exact):
    """TT in {1, 7, 8} the octet form, {9, 16} the generic loop; D one lane, last chunk partial / whole / one vector over"""
    run(R.check_embed_sum, be, R.EMBED_SUM_CASES, exact)


@pytest.mark.parametrize("dtype", [BF16, F32], ids=["bf16", "f32"])
def test_embed_sum_grid_cap(be, dtype):
    M, TT, D = R.EMBED_SUM_CAP
    assert R.check_embed_sum(be, M, TT, D, dtype, True, seed=1) == 0


def test_concat_tok(be):
    """T in {1, 2, 8}; the ids a column slice of a wider matrix whose other columns no kernel may read"""
    run(R.check_concat, be, R.CONCAT_CASES)


def test_concat_tok_grid_cap(be):
    M, T, D = R.CONCAT_CAP
    assert R.check_concat(be, M, T, D, BF16, seed=1) == 0


@pytest.mark.parametrize("exact", [True, False], ids=["exact", "fp64"])
def test_embed_scatter(be, exact):
    """both addressing modes, pad id 0 / a mid id / none, one id holding nearly every occurrence, partial chunks"""
    run(R.check_scatter, be, R.SCATTER_CASES, exact)


def test_embed_scatter_grid_cap(be):
    assert R.check_scatter(be, *R.SCATTER_CAP, True, seed=1) == 0


@pytest.mark.parametrize("exact", [True, False], ids=["exact", "fp64"])
@pytest.mark.parametrize("op", ["bwd", "sum"])
def test_embed_segment_distributions(be, op, exact):
    """every id distribution of ref_index.seg_distributions, V = 4095 | 4096, ld = D + 8 with NaN in the gap, twice into one table"""
    run(R.check_segment, be, [c for c in R.SEG_SMALL_CASES if c[0] == op], exact)


@pytest.mark.parametrize("op", ["bwd", "sum"])
def test_embed_segment_dispatch_classes(be, op):
    """chunk counts 1 / 2 / 4 / 8 (8 / 8 / 4 / 1 waves) x seg_start in LDS / global, each at its widest D and 8 columns over;
    segment_sum at 1, 2 and 3 slabs with a partial last slab and table rows D + 4 apart"""
    run(R.check_segment, be, [c for c in R.SEG_CLASS_CASES if c[0] == op])


@pytest.mark.parametrize("dtype", [BF16, F32], ids=["bf16", "f32"])
def test_embed_split_hi_lo(be, dtype):
    run(R.check_split, be, [(n, dtype, ex) for n in R.SPLIT_SIZES for ex in (True, False)])


def test_embed_table_norm_bwd(be):
    run(R.check_table_norm, be, R.TABLE_NORM_CASES)


@pytest.mark.parametrize("pad", ["first", "last", "none"])
def test_embed_table_norm_bwd_grid_cap(be, pad):
    V, D = R.TABLE_NORM_CAP
    assert R.check_table_norm(be, V, D, BF16, {"first": 0, "last": V - 1, "none": -1}[pad], seed=1) == 0


# ------------------------------------------------------------------------------------------------------- index preparation, transpose
def test_token_segments(be):
    """V in {1, 255, 256, 257, 15999}, n around one chunk and at three, 1 and 7 columns of a wider matrix, ids outside [0, V)"""
    run(R.check_token_segments, be, R.TOKSEG_CASES)


@pytest.mark.parametrize("dtype", [BF16, F32], ids=["bf16", "f32"])
def test_transpose(be, dtype):
    """vector and scalar paths in and out: aligned, ldi off the vector width, input one element in, ldo odd one element in"""
    run(R.check_transpose, be, [(R_, C, dtype, v) for R_, C in R.TRANSPOSE_SHAPES for v in R.TRANSPOSE_VARIANTS])


# --------------------------------------------------------------------------------------------------------------- batch assembly
def test_collate_windows(be):
    run(R.check_collate, be, R.COLLATE_CASES)


def test_collate_windows_grid_cap(be):
    assert R.check_collate(be, *R.COLLATE_CAP) == 0


@pytest.mark.parametrize("ver", ["v1", "v2"])
def test_augment_piece_stats(be, ver):
    assert R.check_piece_stats(be, R.tokenizer(ver)) == 0


@pytest.mark.parametrize("ver", ["v1", "v2"])
def test_augment_collate_windows(be, orc, ver):
    """the constructed corpus (branch census first) against oracle.augment on whole files, cut afterwards"""
    assert R.check_augment(be, R.tokenizer(ver), orc) == 0


def test_augment_collate_windows_grid_cap(be):
    assert R.check_augment_cap(be, R.tokenizer("v2")) == 0
