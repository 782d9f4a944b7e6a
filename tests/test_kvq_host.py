"""The 8-bit K/V cache on the CPU: DecodeSession(kv_dtype="fp8") / DecodePool(kv_dtype="fp8") (decode.py, pool.py), engine.KVStateQ's
dispatch and refusals, through the fake backend plus the stand-ins of the three fp8 entry points (tests/emu_kvq.py).  Tiny 4-layer
model, bf16 (the fp8 cache takes bf16 activations).  The kernels: test_kvq_kernels_gpu.py; the production session:
test_kvq_pool_gpu.py."""
import pytest
import torch

import midi_model_amd as mm
from midi_model_amd import engine
from midi_model_amd.decode import DecodeSession

import emu_fork
import emu_kvq
import fork_common as fc
import kvq_common as kc
import ragged_common as rc

FP8_OPS = ("kv_store_seqs_rows_fp8", "attn_decode_append_rows_fp8", "kv_fork_rows_fp8")
BF16_OPS = ("kv_store_seqs_rows", "kv_store_seqs", "attn_decode_append_rows", "attn_decode_rows", "kv_append_rows", "kv_fork_rows",
            "attn_decode_append_rows_shared", "attn_prefix_partial_slots")


@pytest.fixture(scope="module")
def tok():
    return mm.MIDITokenizerV2()


@pytest.fixture(scope="module")
def tiny(orc, tok):
    shp = orc.Shape(n_layer=4, n_head=4, n_embd=256, n_inner=512, vocab=tok.vocab_size)
    return shp, orc.make_state_dict(shp, seed=0)


def _model(sd, dtype=torch.bfloat16):
    m = mm.MIDIModel(mm.MIDIModelConfig.get_config("v2", True, 4, 4, 256, 512))
    m.load_state_dict(sd)
    return m.to(dtype)


def test_refusals_come_before_any_launch(orc, tok, tiny):
    p = rc.prompts(orc, tok, (5,), seed0=600)[0]
    with emu_kvq.install() as log:
        m = _model(tiny[1])
        m32 = _model(tiny[1], torch.float32)
        del log[:]
        for kw, match in ((dict(kv_dtype="fp8", prefix_slots=2, prefix_capacity=16), "prefix slots"),
                          (dict(kv_dtype="int8"), "kv_dtype"), (dict(kv_dtype="fp8", rows=257), "256 rows")):
            with pytest.raises(ValueError, match=match):
                m.decode_pool(kw.pop("rows", 4), 64, **kw)
        with pytest.raises(ValueError, match="bf16 model"):
            m32.decode_pool(4, 64, kv_dtype="fp8")
        for args, match in (((m, 4, 256, 1.0, 0.98, 1, 0, True, False), "row_params"), ((m, 4, 256, 1.0, 0.98, 1, 0, False, False), "row_params"),
                            ((m, 4, 256, 1.0, 0.98, 1, 64, False, False), "row_params"),
                            ((m, 4, 256, 1.0, 0.98, 1, 0, True, True, False, 2, 64), "prefix slots"),
                            ((m, 257, 256, 1.0, 0.98, 1, 0, True, True), "256 rows"), ((m32, 4, 256, 1.0, 0.98, 1, 0, True, True), "bf16 model")):
            with pytest.raises(ValueError, match=match):
                DecodeSession.make_key(*args, kv_dtype="fp8")
            with pytest.raises(ValueError, match=match):
                DecodeSession(*args, kv_dtype="fp8")
        assert log == [], log
        # ---- a session of the form: prefill / prefill_ragged refuse it; the engine refuses every form but the two it serves
        ses = DecodeSession(m, 4, 256, 1.0, 0.98, 1, ragged=True, row_params=True, kv_dtype="fp8")
        assert isinstance(ses.kv1, engine.KVStateQ) and ses.kv1.cap == 256 and ses.kv1.B == 4 and not hasattr(ses.kv1, "k")
        assert ses.kv1.k8.dtype == torch.uint8 and ses.kv1.k8.shape == (4, 4, 4, 256, 64) and ses.kv1.sc.shape == (4, 4, 4, 256, 2)
        del log[:]
        toks = torch.from_numpy(p)
        with pytest.raises(ValueError, match="admit"):
            ses.prefill(toks[None].repeat(4, 1, 1))
        with pytest.raises(ValueError, match="admit"):
            ses.prefill_ragged(toks.repeat(4, 1), [5] * 4)
        spec, W, kv = m._specs["net"], m._W["net"], ses.kv1
        x = torch.zeros((4, spec.D), dtype=torch.bfloat16)
        with pytest.raises(ValueError, match="fp8"):
            engine.stack_decode(spec, W, x, ses.rope1, kv)                                        # no row_pos
        with pytest.raises(ValueError, match="fp8"):
            engine.stack_decode(spec, W, x, ses.rope1, kv, pos_dev=ses.pos[:1])
        with pytest.raises(ValueError, match="fp8"):
            engine.stack_decode(spec, W, x, ses.rope1, kv, row_pos=ses.pos, shared=(None, None, None))
        with pytest.raises(ValueError, match="unfused"):                                          # fp32 rows: the unfused pair
            engine.stack_decode(spec, m32._W["net"], x.float(), ses.rope1, kv, row_pos=ses.pos)
        with pytest.raises(ValueError, match="fp8"):
            engine.stack_extend(spec, W, torch.zeros((8, spec.D), dtype=torch.bfloat16), 4, 2, ses.rope1, kv)
        with pytest.raises(ValueError, match="fp8"):
            engine.stack_prefill(spec, W, torch.zeros((8, spec.D), dtype=torch.bfloat16), 4, 2, ses.rope1, kv)
        plan = mm.ops.attn_seq_plan([2] * 4, spec.H).upload(torch.device("cpu"))
        with pytest.raises(ValueError, match="fp8"):
            engine.stack_prefill_seqs(spec, W, torch.zeros((8, spec.D), dtype=torch.bfloat16), plan, ses.rope1, kv)   # no rows
        assert log == [], log


def test_session_keys(orc, tok, tiny):
    with emu_kvq.install():
        m = _model(tiny[1])
        for seeded in (False, True):
            plain = DecodeSession.make_key(m, 4, 256, 1.0, 0.98, 1, 0, True, True, seeded)
            form = ("ragged", "row_params", "seeded") if seeded else ("ragged", "row_params")
            assert plain == (m._flat.data_ptr(), m._flat.dtype, 4, 256, form), "the bf16 key is what it was"
            assert DecodeSession.make_key(m, 4, 256, 1.0, 0.98, 1, 0, True, True, seeded, kv_dtype=None) == plain
            q = DecodeSession.make_key(m, 4, 256, 1.0, 0.98, 1, 0, True, True, seeded, kv_dtype="fp8")
            assert q == plain[:4] + (form + (("kv", "fp8"),),) and q != plain
        p = rc.prompts(orc, tok, (5,), seed0=601)[0]
        keys = []
        for kw in ({}, dict(kv_dtype="fp8")):
            with m.decode_pool(4, 64, **kw) as pool:
                pool.submit(p, max_len=8, top_k=1)
                pool.step()
                keys.append(pool.ses.key)
                assert pool.ses.kv_dtype == kw.get("kv_dtype")
        assert keys[0] != keys[1] and len(m._sessions.idle) == 2, "an fp8 pool never takes a bf16 pool's session, nor the reverse"


def _run(m, orc, tok, **kw):
    p, q = rc.prompts(orc, tok, (7, 4), seed0=560)
    with m.decode_pool(5, 64, seeded=True, **kw) as pool:
        a, b, c = pool.submit(p, max_len=14, seed=[1, 2, 3], n=3, **fc.KW)
        pool.submit(q, max_len=9, seed=4, **fc.KW)
        for _ in range(3):
            pool.step()
        kid, = pool.fork(a, seed=9)   # (the siblings were filled by one fork already; this is a second)
        fc.drain(pool)
        return [pool.result(i) for i in (a, b, c, kid)]


def test_call_log(orc, tok, tiny):
    """an fp8 pool names only the fp8 forms for store, attention and fork; a pool made without kv_dtype logs exactly what it logs
    without this feature's stand-ins installed"""
    with emu_fork.install() as log0:
        m = _model(tiny[1])
        del log0[:]
        a, la = _run(m, orc, tok), list(log0)
    with emu_kvq.install() as log:
        m = _model(tiny[1])
        del log[:]
        b, lb = _run(m, orc, tok), list(log)
        assert la == lb and not any(n in lb for n in FP8_OPS) and all(fc.same(x, y) for x, y in zip(a, b))
        del log[:]
        _run(m, orc, tok, kv_dtype="fp8")
        lq = list(log)
    assert all(n in lq for n in FP8_OPS) and not any(n in lq for n in BF16_OPS), sorted(set(lq))
    swap = {"kv_store_seqs_rows": "kv_store_seqs_rows_fp8", "attn_decode_append_rows": "attn_decode_append_rows_fp8",
            "kv_fork_rows": "kv_fork_rows_fp8"}
    # (the sampled ids differ, and with them the eager token steps an event takes; the admissions, forks and net steps do not)
    for plain, q in swap.items():
        assert lb.count(plain) == lq.count(q) > 0, (plain, lb.count(plain), lq.count(q))


def test_fork_and_hold_scenarios(orc, tok, tiny):
    with emu_kvq.install() as log:
        m = _model(tiny[1])
        kc.child_repeats_parent(m, orc, tok, 64)
        kc.siblings_equal_lone_requests(m, orc, tok, 64)
        for alone in (False, True):
            ses = kc.held_then_forked_equals_uninterrupted(m, orc, tok, 64, 3, alone)
        kc.alone_equals_beside_neighbours(m, orc, tok, 64)
        assert m._sessions.idle == [ses] and "kv_fork_rows_fp8" in log and not any(n in log for n in BF16_OPS)


def test_wrapper_checks(orc):
    """ops.kv_fork_rows_fp8 / kv_store_seqs_rows_fp8 refuse on the host what their bf16 forms refuse, before the library is reached"""
    from midi_model_amd import ops_kvq
    k8 = torch.zeros((2, 4, 2, 16, 64), dtype=torch.uint8)
    sc = torch.zeros((2, 4, 2, 16, 2))
    for src, dst, lens, match in (([0], [4], [3], "outside"), ([0, 3], [1, 1], [3, 3], "twice"), ([0, 1], [1, 2], [3, 3], "at once"),
                                  ([0], [1], [17], "length"), ([0], [1], [0], "length")):
        with pytest.raises(ValueError, match=match):
            ops_kvq.kv_fork_rows_fp8(k8, k8.clone(), sc, src, dst, lens)
    plan = mm.ops.attn_seq_plan([3, 2], 2).upload(torch.device("cpu"))
    qkv = torch.zeros((5, 3 * 2 * 64), dtype=torch.bfloat16)
    for rows, match in (([0, 4], "outside"), ([1, 1], "twice"), ([0], "cache rows")):
        with pytest.raises(ValueError, match=match):
            ops_kvq.kv_store_seqs_rows_fp8(qkv, plan, rows, k8[0], k8[0].clone(), sc[0], 2, 64, 16)
    with pytest.raises(ValueError, match="3 rows in a cache of 2"):
        ops_kvq.kv_store_seqs_rows_fp8(qkv, plan, [0, 1], k8[0, :, :, :2].contiguous(), k8[0, :, :, :2].contiguous(),
                                       sc[0, :, :, :2].contiguous(), 2, 64, 2)
