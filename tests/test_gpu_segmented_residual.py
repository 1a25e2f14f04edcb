"""Error feedback under per-tensor budgets on the device (include/gcow.h "Segmented fields with a residual";
codec.rate_tables_segmented, codec.SegmentedResidualEncoder, codec.PerTensorFittedResidualEncoder,
DeviceCodec.encode_residual_per_tensor, compressed_allgather_hook with error_feedback and per_tensor_budget), bitwise
against the per-tensor oracle model (tests/segmented_residual_inputs.py):

  1. the tables of y per tensor: every list x dtype x e in {None, step 2's e}, tables and workspace poisoned, guard rows
     behind the tables; with e None also equal to rate_tables_tensors; maxprec 12;
  2. the encode: every list x dtype x word set x index stride x e, the whole stream capacity, bit count, index and e'
     against the model, e' between guards, x unchanged; the stream also equals encode_segmented of a torch-made y;
  3. in place (err_out is err) equals separate buffers, with oversized tiles included;
  4. x, e_in and e_out at three different alignments;
  5. NaN / Inf blocks and an overflowing x + e;
  6. the fitted chain over two steps at 8 and 2.5 bits per value;
  7. the chain captured into a graph and replayed on step 2's data, then step 1's;
  8. the hook at world 1 over RCCL, two iterations, fp32 and bf16.
Every test fails on a library without gcow_rate_table_seg_device / gcow_encode_seg_residual_device."""
import os
import sys

import numpy as np
import pytest

torch = pytest.importorskip("torch")

TESTS = os.path.dirname(os.path.abspath(__file__))
if TESTS not in sys.path:
    sys.path.insert(0, TESTS)

import fitted_per_tensor_inputs as FP  # noqa: E402
import mean_codec  # noqa: E402
import segmented_inputs as SI  # noqa: E402
import segmented_residual_inputs as SR  # noqa: E402
from test_gpu_segmented import (BF, BF_IDS, POISON, POISON_I64, _Bucket, _bits_of, _check_encode, _poison,  # noqa: E402
                                _records, _u64, _upload, _words_tensor, gc, nccl_world1)  # noqa: F401

pytestmark = pytest.mark.gpu

SENT = -1234.0  # the guards around e_out
SENT_BITS = np.float32(SENT).view(np.uint32)


def _guarded(n: int, lead: int = 4, tail: int = 4):
    """-> (the allocation, its view of n fp32 values `lead` values in): every value the sentinel."""
    whole = torch.full((n + lead + tail,), SENT, dtype=torch.float32, device="cuda")
    return whole, whole[lead:lead + n]


def _check_guarded(whole, lead, n, want_bits, what=None):
    g = _bits_of(whole)
    assert np.array_equal(g[lead:lead + n], want_bits), what
    assert (g[:lead] == SENT_BITS).all() and (g[lead + n:] == SENT_BITS).all(), what


def _err(name, bf16, step, bpv=8.0):
    e = SR.e_bucket(name, bf16, step, bpv)
    return None if e is None else _upload(e)


def _x_bits(a):
    return a.view(np.uint16 if a.dtype == np.uint16 else np.uint32)


# ------------------------------------------------------------------------------------------------ 1. the tables
def _run_tables(gc, name, bf16, step, maxprec, plan):
    cnts = SI.counts(name)
    S = len(cnts)
    x = _upload(SR.x_bucket(name, bf16, step))
    e = _err(name, bf16, step)
    rt = gc.SegmentedRateTables(cnts, x.dtype, maxprec, "cuda", plan)
    big = torch.full((S + 2, 288), int(POISON_I64), dtype=torch.int64, device="cuda")
    rt.tables = big[:S]
    rt.ws.fill_(int(POISON_I64))
    got = rt(x, e)
    torch.cuda.synchronize()
    want = SR.tables_y(name, bf16, step, maxprec)
    g = big.cpu().numpy()
    for s in range(S):
        assert np.array_equal(g[s], want[s]), (s, cnts[s])
        if not cnts[s]:
            assert not g[s].any()
    assert (g[S:].view(np.uint64) == np.uint64(POISON)).all()
    assert np.array_equal(_bits_of(x), _x_bits(SR.x_bucket(name, bf16, step)))
    return x, got


@pytest.mark.parametrize("bf16", BF, ids=BF_IDS)
@pytest.mark.parametrize("name", SR.LISTS)
def test_tables(gc, orc, name, bf16):
    SR.check_differs(name, bf16)
    cnts = SI.counts(name)
    plan = gc.SegmentPlan(cnts, torch.bfloat16 if bf16 else torch.float32, "cuda")
    for step in SR.STEPS:
        x, got = _run_tables(gc, name, bf16, step, 64, plan)
        if step == 0:  # e None: the per-tensor tables of x from the other plan
            ref = gc.rate_tables_tensors(list(torch.split(x, cnts)), 64)
            torch.cuda.synchronize()
            assert torch.equal(got, ref)
            assert torch.equal(gc.rate_tables_segmented(x, cnts, None, 64, plan), ref)


@pytest.mark.parametrize("bf16", BF, ids=BF_IDS)
@pytest.mark.parametrize("name", ["edges", "special"])
def test_tables_maxprec_12(gc, orc, name, bf16):
    for step in SR.STEPS:
        _run_tables(gc, name, bf16, step, 12, None)


def test_tables_empty_lists(gc):
    x = torch.zeros(0, device="cuda")
    assert gc.rate_tables_segmented(x, []).shape == (0, 288)
    t = gc.rate_tables_segmented(x, [0, 0])
    torch.cuda.synchronize()
    assert t.shape == (2, 288) and not t.any()


# ------------------------------------------------------------------------------------------------ 2. the encode
def _encode_case(gc, enc, name, bf16, step, ws, stride, x, e, lead=4):
    n = x.numel()
    want = SR.model(name, bf16, step, ws)
    whole, out = _guarded(n, lead)
    _poison(enc)
    r = enc(x, e, _words_tensor(SI.words(name, bf16, ws), records=stride == 8), err_out=out)
    _check_encode(enc, r, want[:4], stride)
    _check_guarded(whole, lead, n, want[3].view(np.uint32), (ws, stride, step))
    return want


@pytest.mark.parametrize("bf16", BF, ids=BF_IDS)
@pytest.mark.parametrize("name", SR.LISTS)
def test_encode_every_word_set_stride_and_error(gc, orc, name, bf16):
    cnts = SI.counts(name)
    dt = torch.bfloat16 if bf16 else torch.float32
    plan = gc.SegmentPlan(cnts, dt, "cuda")
    yplan = gc.SegmentPlan(cnts, torch.float32, "cuda")
    for step in SR.STEPS:
        a = SR.x_bucket(name, bf16, step)
        x = _upload(a)
        e = _err(name, bf16, step)
        e_copy = None if e is None else e.clone()
        y = x.float() + (e if e is not None else torch.zeros_like(x, dtype=torch.float32))
        for stride in SR.STRIDES:
            enc = gc.SegmentedResidualEncoder(cnts, dt, 64, "cuda", stride, plan=plan)
            for ws in SR.WORD_SETS:
                want = _encode_case(gc, enc, name, bf16, step, ws, stride, x, e)
                if stride == 16:  # the stream of the fp32 array y
                    ye = gc.encode_segmented(y, cnts, _words_tensor(SI.words(name, bf16, ws), False), 64, 16, plan=yplan)
                    torch.cuda.synchronize()
                    nw = (want[1] + 63) // 64
                    assert ye.bits == want[1]
                    assert np.array_equal(_u64(ye.words)[:nw], _u64(enc.words)[:nw])
                    assert np.array_equal(_u64(ye.index), _u64(enc.index))
        assert np.array_equal(_bits_of(x), _x_bits(a))  # only read
        if e is not None:
            assert torch.equal(e, e_copy)


def test_encode_empty_lists(gc):
    for cnts in ([], [0, 0]):
        x = torch.zeros(0, device="cuda")
        enc = gc.SegmentedResidualEncoder(cnts, torch.float32, 64, "cuda", 16)
        _poison(enc)
        r = enc(x, torch.zeros(0, device="cuda"), torch.zeros(len(cnts), dtype=torch.int32, device="cuda"))
        torch.cuda.synchronize()
        assert r.bits == 0 and (_u64(enc.words) == np.uint64(POISON)).all()
    x = torch.zeros(8, device="cuda")
    w = torch.zeros(2, dtype=torch.int32, device="cuda")
    with pytest.raises(gc.GcowError):
        gc.encode_segmented_residual(x, None, [4, 4], w)  # zeros need err_out
    with pytest.raises(gc.GcowError):
        gc.encode_segmented_residual(x, torch.zeros(7, device="cuda"), [4, 4], w)
    with pytest.raises(gc.GcowError):
        gc.encode_segmented_residual(x, torch.zeros(8, dtype=torch.float64, device="cuda"), [4, 4], w)


# ------------------------------------------------------------------------------------------------ 3. in place
@pytest.mark.parametrize("bf16", BF, ids=BF_IDS)
@pytest.mark.parametrize("name,ws", [("edges", "fit8"), ("small", "lo"), ("edges", "lo")])
def test_in_place_equals_separate_buffers(gc, orc, name, ws, bf16):
    """`lo` codes every block at full precision: every tile is oversized and is read again by the second pass."""
    cnts = SI.counts(name)
    x = _upload(SR.x_bucket(name, bf16, 1))
    words = _words_tensor(SI.words(name, bf16, ws), False)
    want = SR.model(name, bf16, 1, ws)
    enc = gc.SegmentedResidualEncoder(cnts, x.dtype, 64, "cuda", 16)
    err = _err(name, bf16, 1)
    _poison(enc)
    r = enc(x, err, words)  # err_out is err
    _check_encode(enc, r, want[:4], 16)
    assert np.array_equal(_bits_of(err), want[3].view(np.uint32))
    got_words, got_index = _u64(enc.words).copy(), _u64(enc.index).copy()
    e_in, e_out = _err(name, bf16, 1), torch.full((x.numel(),), SENT, device="cuda")
    _poison(enc)
    r = enc(x, e_in, words, err_out=e_out)
    _check_encode(enc, r, want[:4], 16)
    assert torch.equal(e_out, err)
    assert np.array_equal(_u64(enc.words), got_words) and np.array_equal(_u64(enc.index), got_index)
    assert np.array_equal(_bits_of(e_in), SR.e_bucket(name, bf16, 1).view(np.uint32))


# ------------------------------------------------------------------------------------------------ 4. alignment
def _placed(a: np.ndarray, off: bool, fill):
    """`a` inside a larger allocation: one element in (off the row alignment) or four elements in (fp32: aligned)."""
    lead = 1 if off else (8 if a.dtype == np.uint16 else 4)
    pad = np.full(8, fill, a.dtype)
    whole = _upload(np.concatenate([pad[:lead], a, pad[:3]]))
    return whole, whole[lead:lead + a.size], lead


@pytest.mark.parametrize("bf16", BF, ids=BF_IDS)
@pytest.mark.parametrize("offs", [(True, False, False), (False, True, True), (True, True, False)],
                         ids=["x_off", "e_off", "x_ein_off"])
def test_three_alignments(gc, orc, offs, bf16):
    name, ws, step = "edges", "alt", 1
    cnts = SI.counts(name)
    a, e = SR.x_bucket(name, bf16, step), SR.e_bucket(name, bf16, step)
    n = a.size
    xw, x, xl = _placed(a, offs[0], a[0])
    ew, ei, el = _placed(e, offs[1], np.float32(0.5))
    lead = 1 if offs[2] else 4
    ow, eo = _guarded(n, lead, 3)
    for t, off, al in ((x, offs[0], 4 if bf16 else 16), (ei, offs[1], 16), (eo, offs[2], 16)):
        assert (t.data_ptr() % al != 0) == off
    want = SR.model(name, bf16, step, ws)
    enc = gc.SegmentedResidualEncoder(cnts, x.dtype, 64, "cuda", 16)
    _poison(enc)
    r = enc(x, ei, _words_tensor(SI.words(name, bf16, ws), True), err_out=eo)
    _check_encode(enc, r, want[:4], 16)
    _check_guarded(ow, lead, n, want[3].view(np.uint32))
    gx = _bits_of(xw)
    assert np.array_equal(gx[xl:xl + n], _x_bits(a)) and (gx[:xl] == _x_bits(a)[0]).all()
    assert (gx[xl + n:] == _x_bits(a)[0]).all()
    ge = _bits_of(ew)
    half = np.float32(0.5).view(np.uint32)
    assert np.array_equal(ge[el:el + n], e.view(np.uint32)) and (ge[:el] == half).all() and (ge[el + n:] == half).all()
    # the tables read x and e at the same places
    T = gc.rate_tables_segmented(x, cnts, ei, 64)
    torch.cuda.synchronize()
    assert np.array_equal(T.cpu().numpy(), SR.tables_y(name, bf16, step))


# ------------------------------------------------------------------------------------------------ 5. special values
@pytest.mark.parametrize("bf16", BF, ids=BF_IDS)
def test_special_values(gc, orc, bf16):
    """NaN / Inf blocks, the all-NaN block and the tensor where x + e overflows: stream and e' per the model, a
    non-finite residual is +0."""
    name, step = "special", 1
    cnts = SI.counts(name)
    ys = SR.y_tensors(name, bf16, step)
    xs = [SR.widen(t) for t in SI.variant(name, bf16, step)]
    assert any(np.isnan(y).any() for y in ys) and any(np.isinf(y).any() for y in ys)
    assert any(np.isnan(y.reshape(-1, 4)).all(axis=1).any() for y in ys if y.size % 4 == 0 and y.size)
    assert any((np.isinf(y) & np.isfinite(x)).any() for x, y in zip(xs, ys))  # x + e overflows
    x, e = _upload(SR.x_bucket(name, bf16, step)), _err(name, bf16, step)
    for ws in ("fit8", "lo", "alt"):
        want = SR.model(name, bf16, step, ws)
        y = np.concatenate(ys)
        with np.errstate(all="ignore"):
            bad = ~np.isfinite(y - want[4])
        assert bad.any() and not want[3].view(np.uint32)[bad].any()
        enc = gc.SegmentedResidualEncoder(cnts, x.dtype, 64, "cuda", 8)
        _encode_case(gc, enc, name, bf16, step, ws, 8, x, e)


# ------------------------------------------------------------------------------------------------ 6. the fitted chain
def _check_chain(e, fits, err, name, bf16, step, bpv, stride=16):
    cnts = SI.counts(name)
    recs, want = SR.chain(name, bf16, step, bpv)
    torch.cuda.synchronize()
    assert _records(fits) == list(recs), step
    words, total, pos, res, _ = want
    assert e.bits == total == sum(r[2] for r in recs)
    if all(r[1] == 0 for r in recs):
        assert total <= sum(FP.budget_of(bpv, n) for n in cnts)
    assert np.array_equal(_u64(e.words)[:words.size], words)
    ix = SI.index_of(pos, stride)
    assert np.array_equal(_u64(e.index)[:ix.size], ix)
    assert np.array_equal(_bits_of(err), res.view(np.uint32)), step


@pytest.mark.parametrize("bf16", BF, ids=BF_IDS)
@pytest.mark.parametrize("bpv", [8.0, 2.5])
@pytest.mark.parametrize("name", SR.LISTS)
def test_fitted_chain_two_steps(gc, orc, name, bpv, bf16):
    cnts = SI.counts(name)
    x = _upload(SR.x_bucket(name, bf16, 0))
    err = torch.zeros(x.numel(), device="cuda")
    enc = gc.PerTensorFittedResidualEncoder(bpv)
    for step in SR.STEPS:
        x.copy_(_upload(SR.x_bucket(name, bf16, step)))
        e, fits = enc(x, err, cnts, 16)
        _check_chain(e, fits, err, name, bf16, step, bpv)


# ------------------------------------------------------------------------------------------------ 7. captured graph
def test_fitted_chain_graph(gc, orc):
    """Tables of y -> fits -> segmented residual encode captured on one stream, replayed on step 2's data and then on
    step 1's: each replay equals the eager call on that data."""
    name, bf16, bpv = "hook", False, 8.0
    cnts = SI.counts(name)
    x = _upload(SR.x_bucket(name, bf16, 0))
    err = torch.zeros(x.numel(), device="cuda")
    enc = gc.PerTensorFittedResidualEncoder(bpv)
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        enc(x, err, cnts, 16, stream=s)  # plans, allocates and uploads: not capturable, and not needed again
    s.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, stream=s):
        e, fits = enc(x, err, cnts, 16, stream=s)
    for step in (1, 0):
        a, ein = SR.x_bucket(name, bf16, step), SR.e_bucket(name, bf16, step, bpv)
        x.copy_(_upload(a))
        err.copy_(_upload(ein) if ein is not None else torch.zeros_like(err))
        torch.cuda.synchronize()
        g.replay()
        torch.cuda.synchronize()
        ex, eerr = _upload(a), (_upload(ein) if ein is not None else torch.zeros_like(err))
        eager, efits = gc.PerTensorFittedResidualEncoder(bpv)(ex, eerr, cnts, 16)
        torch.cuda.synchronize()
        nw = (eager.bits + 63) // 64
        assert e.bits == eager.bits and _records(fits) == _records(efits)
        assert np.array_equal(_u64(e.words)[:nw], _u64(eager.words)[:nw])
        assert np.array_equal(_u64(e.index), _u64(eager.index))
        assert torch.equal(err, eerr)
        _check_chain(e, fits, err, name, bf16, step, bpv)


# ------------------------------------------------------------------------------------------------ 8. the hook
@pytest.mark.parametrize("bf16", BF, ids=BF_IDS)
def test_allgather_hook_error_feedback_per_tensor_world1(gc, orc, nccl_world1, bf16):
    """One rank over RCCL, one bucket over two iterations: after each the bucket is the model's decode of this rank's
    stream (bf16: rounded to nearest even), the state's error buffer the model's residual and its records the model's."""
    from gcow_amd import ddp
    from gcow_amd import dist as gdist

    calls = []

    class CountingCodec(gdist.DeviceCodec):
        def encode_residual_per_tensor(self, *a, **k):
            calls.append("encode_residual_per_tensor")
            return super().encode_residual_per_tensor(*a, **k)

        def encode_per_tensor(self, *a, **k):
            calls.append("encode_per_tensor")
            return super().encode_per_tensor(*a, **k)

        def decode_mean_per_tensor(self, *a, **k):
            calls.append("decode_mean_per_tensor")
            return super().decode_mean_per_tensor(*a, **k)

    name, bpv = "hook", 8.0
    cnts = SI.counts(name)
    state = ddp.make_hook_state(hook=ddp.compressed_allgather_hook, params=gc.accuracy(1e-3), codec=CountingCodec(),
                                target_bits=bpv, per_tensor_budget=True, error_feedback=True)
    for step in SR.STEPS:
        recs, want = SR.chain(name, bf16, step, bpv)
        mean = mean_codec.mean_of([want[4]])
        bits = SI.bf16_rne(mean) if bf16 else mean.view(np.uint32)
        t = _upload(SR.x_bucket(name, bf16, step))
        out = ddp.compressed_allgather_hook(state, _Bucket(t, 0, cnts)).wait()
        torch.cuda.synchronize()
        out = out[0] if isinstance(out, (list, tuple)) else out
        assert out.data_ptr() == t.data_ptr()
        assert np.array_equal(_bits_of(out), bits), step
        assert np.array_equal(_bits_of(state.error_buffer(0, t)), want[3].view(np.uint32)), step
        assert _records(state.fit_record(0)) == list(recs)
    assert calls == ["encode_residual_per_tensor", "decode_mean_per_tensor"] * 2
    state.reset_error_feedback()
    assert not state.error_buffer(0, t).any()
