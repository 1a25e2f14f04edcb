"""GPU parity of the bit budget over a tensor list (include/gcow.h: gcow_rate_table_list_device,
gcow_roundtrip_list_fitted_device; codec.TensorListFitted, rate_table_tensors, roundtrip_tensors_fitted,
roundtrip_gradients_fitted), bit for bit:

  1. the table of a list against the oracle's 288 encodes of the concatenation and against codec.rate_table(cat): the
     seam lists of tests/roundtrip_list_inputs.py (crafted zero / subnormal / NaN / Inf / 3e38 blocks across one- to
     three-value tensors, and inside a long tensor at offset 1 mod 4), fp32 and bf16, carved at 16-byte aligned bases
     and at odd element offsets, maxprec 64 and 12; single tensors around the chunk of C = 8192 values; empty lists;
     maxprec 0;
  2. a list with more direct chunks than the table kernel's grid, so that its grid-stride loop runs;
  3. the fitted round trip against the oracle's decompress(compress(X)) under the fitted set and against
     codec.roundtrip_fitted(cat), for budgets at and around the table's entries and out-of-range hand-written words,
     four dtype pairs, out of place and in place;
  4. the one call (TensorListFitted), its plan reuse and a stream capture replayed on other contents;
  5. roundtrip_gradients_fitted on a small model;
  6. refusals through Python.

The tensors are carved out of one sentinel-filled buffer with gaps of at least 3 elements and 16 elements of tail:
every test checks that the gaps and the tail still hold the sentinel and, out of place, that the inputs are untouched.
The table and the workspace are filled with a poison pattern before every table call."""
import os
import sys

import numpy as np
import pytest

torch = pytest.importorskip("torch")

TESTS = os.path.dirname(os.path.abspath(__file__))
if TESTS not in sys.path:
    sys.path.insert(0, TESTS)

import list_fitted_inputs as LF  # noqa: E402

pytestmark = pytest.mark.gpu

CH = LF.CHUNK
DTYPES = [(False, False), (True, True), (False, True), (True, False)]
DTYPE_IDS = ["fp32-fp32", "bf16-bf16", "fp32-bf16", "bf16-fp32"]
POISON = LF.POISON


@pytest.fixture(scope="module")
def gc(orc):
    if not torch.cuda.is_available():
        pytest.fail("GPU tests need a device")
    from gcow_amd import codec
    return codec


def _tdtype(bf16):
    return torch.bfloat16 if bf16 else torch.float32


def _bits_of(t):
    """The tensor's values as raw bits (uint32 for fp32, uint16 for bf16)."""
    if t.dtype == torch.bfloat16:
        return t.view(torch.int16).cpu().numpy().view(np.uint16)
    return t.cpu().numpy().view(np.uint32)


def _want(d, bf16_out):
    from roundtrip_inputs import bf16_rne
    return bf16_rne(d) if bf16_out else d.view(np.uint32)


def _carve(sizes, bf16, aligned, x_np=None):
    """-> (buffer, tensors, cover mask): the buffer sentinel-filled, the tensors views into it, filled from x_np."""
    pos, total = LF.layout(sizes, aligned)
    buf = torch.full((total,), LF.SENT, dtype=_tdtype(bf16), device="cuda")
    assert buf.data_ptr() % 16 == 0
    cover = np.zeros(total, bool)
    ts, at = [], 0
    if x_np is not None:
        xt = torch.from_numpy(np.array(x_np)).cuda()  # a writable copy: the cases' arrays are shared and read-only
        xt = xt.view(torch.bfloat16) if bf16 else xt
    for p, n in zip(pos, sizes):
        t = buf[p:p + n]
        if x_np is not None and n:
            t.copy_(xt[at:at + n])
        cover[p:p + n] = True
        ts.append(t)
        at += n
    return buf, ts, cover


def _fill(ts, x_np, bf16):
    """The carved tensors' contents replaced (their addresses stay)."""
    xt = torch.from_numpy(np.array(x_np)).cuda()
    xt = xt.view(torch.bfloat16) if bf16 else xt
    at = 0
    for t in ts:
        if t.numel():
            t.copy_(xt[at:at + t.numel()])
        at += t.numel()


def _covered(buf, cover):
    return _bits_of(buf)[cover]


def _gaps_clean(buf, cover):
    sent = _bits_of(torch.full((1,), LF.SENT, dtype=buf.dtype))[0]
    return bool((_bits_of(buf)[~cover] == sent).all())


def _untouched(buf, cover, x_np):
    """The inputs were only read: every tensor holds its values, every gap and the tail the sentinel."""
    return np.array_equal(_covered(buf, cover), x_np.view(np.uint16 if buf.dtype == torch.bfloat16 else np.uint32)) \
        and _gaps_clean(buf, cover)


def _cat(ts, bf16):
    return torch.cat([t.reshape(-1) for t in ts]) if ts else torch.zeros(0, dtype=_tdtype(bf16), device="cuda")


def _poison(plan, ts):
    """The plan object's table and workspace filled with the poison pattern (allocated by a first call if need be)."""
    if plan.table is None:
        plan.rate_table(ts)
    plan.table.fill_(POISON)
    plan.ws.fill_(POISON)


def _table_of(gc, plan, ts, maxprec):
    _poison(plan, ts)
    t = gc.rate_table_tensors(ts, maxprec, plan=plan)
    assert t is plan.table and t.dtype == torch.int64 and t.numel() == 288
    torch.cuda.synchronize()
    return t.cpu().numpy()


# ------------------------------------------------------------------------------------------------ 1. table parity
@pytest.mark.parametrize("maxprec", [64, 12])
@pytest.mark.parametrize("aligned", [True, False], ids=["aligned16", "odd-element"])
@pytest.mark.parametrize("bf16", [False, True], ids=["fp32", "bf16"])
@pytest.mark.parametrize("r", [0, 1, 2, 3])
def test_table_seam_list(gc, orc, r, bf16, aligned, maxprec):
    sizes = LF.seam_sizes(r)
    x_np = LF.seam_field(r, bf16)
    buf, ts, cover = _carve(sizes, bf16, aligned, x_np)
    plan = gc.TensorListFitted(8.0, maxprec)
    got = _table_of(gc, plan, ts, maxprec)
    assert np.array_equal(got, LF.seam_table(r, bf16, maxprec))
    assert np.array_equal(got, gc.rate_table(_cat(ts, bf16), maxprec).cpu().numpy())
    assert _untouched(buf, cover, x_np)
    s = plan.stats()
    assert s.domain == 1 and s.total_values == x_np.size
    assert s.gather_chunks >= 6  # the chunks with seams and the last block
    if not bf16 or not aligned:
        assert s.direct_chunks >= 2  # bf16 at aligned bases: only the tensors at even flat offsets have aligned rows
    assert s.direct_chunks >= 1  # both kinds are present
    # a second call reuses the plan and gives the same bits
    assert np.array_equal(_table_of(gc, plan, ts, maxprec), got) and plan.rebuilds == 1


@pytest.mark.parametrize("bf16", [False, True], ids=["fp32", "bf16"])
@pytest.mark.parametrize("n", LF.SINGLE_SIZES)
def test_table_single_tensor(gc, orc, n, bf16):
    x_np = np.array(LF.seam_field(1, bf16)[:n])
    for aligned in (True, False):
        buf, ts, cover = _carve([n], bf16, aligned, x_np)
        for maxprec in (64, 12):
            plan = gc.TensorListFitted(8.0, maxprec)
            got = _table_of(gc, plan, ts, maxprec)
            assert np.array_equal(got, LF.single_table(n, bf16, maxprec)), (aligned, maxprec)
            assert np.array_equal(got, gc.rate_table(ts[0].clone(), maxprec).cpu().numpy())
        assert _untouched(buf, cover, x_np)


def test_table_empty_lists_and_maxprec_zero(gc, orc):
    for ts in ([], [torch.zeros(0, device="cuda"), torch.zeros(0, device="cuda")],
               [torch.zeros(0, device="cuda", dtype=torch.bfloat16)]):
        plan = gc.TensorListFitted(8.0)
        assert not _table_of(gc, plan, ts, 64).any()
    # no precision: every block is one bit under every minexp
    x_np = LF.seam_field(2, False)
    buf, ts, cover = _carve(LF.seam_sizes(2), False, False, x_np)
    got = _table_of(gc, gc.TensorListFitted(8.0, 0), ts, 0)
    assert (got == (x_np.size + 3) // 4).all()
    assert _untouched(buf, cover, x_np)


# ------------------------------------------------------------------------------------------------ 2. grid-stride
def test_table_grid_stride(gc, orc):
    """1100 direct chunks and three gather chunks on a grid of 1024: every workgroup takes a chunk, some take two."""
    cap = gc.RATE_TABLE_LIST_MAX_GRID
    sizes = [500 * CH + 1, 300 * CH + 2, 303 * CH + 3]  # two seams and a partial last block
    buf, ts, cover = _carve(sizes, False, True)
    for k, t in enumerate(ts):
        gc.fill_normal(t, 1e-3, seed=11 + k)
    before = buf.clone()
    plan = gc.TensorListFitted(8.0)
    got = _table_of(gc, plan, ts, 64)
    s = plan.stats()
    assert s.direct_chunks > cap and s.gather_chunks >= 3 and s.direct_chunks + s.gather_chunks < 2 * cap
    assert np.array_equal(got, gc.rate_table(_cat(ts, False), 64).cpu().numpy())
    assert torch.equal(buf.view(torch.int32), before.view(torch.int32))  # inputs, gaps and tail


# ------------------------------------------------------------------------------------------------ 3. fitted round trip
def _expect(r, bf16_in, bf16_out, maxprec, m):
    d, bits = LF.seam_roundtrip(r, bf16_in, maxprec, m)
    return _want(d, bf16_out), bits


def _run_fitted(gc, plan, ins, ibuf, icover, x_np, sizes, word, maxprec, bf16_in, bf16_out, aligned, want, bits_ref):
    """Out of place on fresh outputs; the contiguous call on the concatenation; then in place for equal dtypes."""
    obuf, outs, ocover = _carve(sizes, bf16_out, aligned)
    bits = torch.full((1,), -1, dtype=torch.int64, device="cuda")
    word0 = word.clone()
    got = gc.roundtrip_tensors_fitted(ins, word, maxprec, outs=outs, bits=bits, plan=plan)
    torch.cuda.synchronize()
    assert [g.data_ptr() for g in got] == [o.data_ptr() for o in outs]
    assert np.array_equal(_covered(obuf, ocover), want) and _gaps_clean(obuf, ocover)
    assert _untouched(ibuf, icover, x_np)
    assert int(bits.item()) == bits_ref
    assert torch.equal(word, word0)  # d_minexp is read, never written
    ref = gc.roundtrip_fitted(_cat(ins, bf16_in), word, maxprec,
                              out=torch.empty(x_np.size, dtype=_tdtype(bf16_out), device="cuda"))
    torch.cuda.synchronize()
    assert np.array_equal(_bits_of(ref), want)
    if bf16_in != bf16_out:
        return
    bits2 = torch.full((1,), -1, dtype=torch.int64, device="cuda")
    gc.roundtrip_tensors_fitted(ins, word, maxprec, bits=bits2, plan=plan)
    torch.cuda.synchronize()
    assert np.array_equal(_covered(ibuf, icover), want) and _gaps_clean(ibuf, icover)
    assert int(bits2.item()) == bits_ref
    _fill(ins, x_np, bf16_in)


@pytest.mark.parametrize("maxprec", [64, 12])
@pytest.mark.parametrize("aligned", [True, False], ids=["aligned16", "odd-element"])
@pytest.mark.parametrize("bf16_in,bf16_out", DTYPES, ids=DTYPE_IDS)
@pytest.mark.parametrize("r", [0, 1, 2, 3])
def test_roundtrip_fitted_seam_list(gc, orc, r, bf16_in, bf16_out, aligned, maxprec):
    sizes = LF.seam_sizes(r)
    x_np = LF.seam_field(r, bf16_in)
    T = LF.seam_table(r, bf16_in, maxprec)
    d_T = torch.from_numpy(np.array(T)).cuda()
    ibuf, ins, icover = _carve(sizes, bf16_in, aligned, x_np)
    plan = gc.TensorListFitted(8.0, maxprec)
    seen = set()
    for budget in LF.budgets(T, x_np.size):
        rec = gc.fit_device(d_T, budget)
        want_rec = LF.fit_record(T, budget)
        assert gc.read_fit(rec) == want_rec, budget
        m = want_rec[0]
        seen.add(want_rec[:2])
        want, bits_ref = _expect(r, bf16_in, bf16_out, maxprec, m)
        assert bits_ref == int(T[m - LF.MINEXP_LO])
        _run_fitted(gc, plan, ins, ibuf, icover, x_np, sizes, rec, maxprec, bf16_in, bf16_out, aligned, want, bits_ref)
    assert (133, 1) in seen and (132, 0) in seen and (-154, 0) in seen
    # hand-written words outside the table's range behave as its ends
    for w in (-100000, 100000):
        want, bits_ref = _expect(r, bf16_in, bf16_out, maxprec, LF.clamp(w))
        word = torch.tensor([w], dtype=torch.int32, device="cuda")
        _run_fitted(gc, plan, ins, ibuf, icover, x_np, sizes, word, maxprec, bf16_in, bf16_out, aligned, want, bits_ref)
    s = plan.stats()
    assert s.domain == 1 and s.gather_chunks >= 6 and s.direct_chunks >= 1  # both kernels ran


# ------------------------------------------------------------------------------------------------ 4. the one call
@pytest.mark.parametrize("bpv", [8.0, 2.5])
@pytest.mark.parametrize("bf16", [False, True], ids=["fp32", "bf16"])
def test_one_call(gc, orc, bf16, bpv):
    r, maxprec = 1, 64
    sizes = LF.seam_sizes(r)
    x_np = LF.seam_field(r, bf16)
    T = LF.seam_table(r, bf16, maxprec)
    budget = LF.budget_of(bpv, x_np.size)
    want_rec = LF.fit_record(T, budget)
    want, bits_ref = _expect(r, bf16, bf16, maxprec, want_rec[0])
    assert want_rec[1] == 0 and bits_ref == want_rec[2] <= budget
    ibuf, ins, icover = _carve(sizes, bf16, False, x_np)
    obuf, outs, ocover = _carve(sizes, bf16, True)
    plan = gc.TensorListFitted(bpv, maxprec)
    bits = torch.full((1,), -1, dtype=torch.int64, device="cuda")
    assert plan(ins, outs, bits) == outs  # allocates the table and the workspace: poisoned from the second call on
    torch.cuda.synchronize()
    assert np.array_equal(plan.table.cpu().numpy(), T)
    assert gc.read_fit(plan.fit) == want_rec and plan.budget == budget
    assert plan.params().tuple() == (1, 16658, maxprec, want_rec[0])
    assert int(bits.item()) == bits_ref <= budget
    assert np.array_equal(_covered(obuf, ocover), want) and _gaps_clean(obuf, ocover)
    assert _untouched(ibuf, icover, x_np)
    ref = gc.roundtrip_fitted(_cat(ins, bf16), bpv, maxprec)
    torch.cuda.synchronize()
    assert np.array_equal(_bits_of(ref), want)
    # a second call on the same tensors plans nothing; without `bits` the count lands in the object's own word
    obuf.fill_(LF.SENT)
    _poison(plan, ins)
    plan(ins, outs)
    torch.cuda.synchronize()
    assert plan.rebuilds == 1 and int(plan.bits.item()) == bits_ref
    assert np.array_equal(plan.table.cpu().numpy(), T) and gc.read_fit(plan.fit) == want_rec
    assert np.array_equal(_covered(obuf, ocover), want) and _gaps_clean(obuf, ocover)
    # in place
    inplace = gc.TensorListFitted(bpv, maxprec)
    assert inplace(ins) == ins
    torch.cuda.synchronize()
    assert inplace.rebuilds == 1 and np.array_equal(_covered(ibuf, icover), want) and _gaps_clean(ibuf, icover)


def test_one_call_below_one_bit_per_block(gc, orc):
    x_np = LF.seam_field(1, False)
    T = LF.seam_table(1, False, 64)
    ibuf, ins, icover = _carve(LF.seam_sizes(1), False, True, x_np)
    obuf, outs, ocover = _carve(LF.seam_sizes(1), False, True)
    plan = gc.TensorListFitted(0.25)
    _poison(plan, ins)
    plan(ins, outs)
    torch.cuda.synchronize()
    assert gc.read_fit(plan.fit) == (133, 1, int(T[287])) and int(plan.bits.item()) == int(T[287])
    with pytest.raises(gc.GcowError):
        plan.params()
    assert plan.params(allow_coarsest=True).tuple() == (1, 16658, 64, 133)
    want, _ = _expect(1, False, False, 64, 133)
    assert np.array_equal(_covered(obuf, ocover), want) and _gaps_clean(obuf, ocover)
    assert _untouched(ibuf, icover, x_np)


def test_one_call_graph_capture(gc, orc):
    """Table, fit and round trip captured once and replayed on two contents of the same tensors; the second is the
    first scaled by 2^-7, so the fitted minexp moves with the data."""
    sizes = LF.seam_sizes(3)
    x1 = np.array(LF.seam_field(3, False))
    with np.errstate(under="ignore", invalid="ignore"):
        x2 = (x1 * np.float32(2.0 ** -7)).astype(np.float32)
    ibuf, ins, icover = _carve(sizes, False, False, x1)
    obuf, outs, ocover = _carve(sizes, False, True)
    ebuf, eouts, ecover = _carve(sizes, False, True)
    plan = gc.TensorListFitted(8.0)
    bits = torch.full((1,), -1, dtype=torch.int64, device="cuda")
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        plan(ins, outs, bits)  # plans, uploads and allocates outside the capture
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        plan(ins, outs, bits)
    assert plan.rebuilds == 1
    eager = gc.TensorListFitted(8.0)
    recs = []
    for x in (x1, x2):
        _fill(ins, x, False)
        obuf.fill_(LF.SENT)
        bits.fill_(-1)
        plan.table.fill_(POISON)
        plan.ws.fill_(POISON)
        g.replay()
        torch.cuda.synchronize()
        rec = gc.read_fit(plan.fit)
        ebits = torch.full((1,), -1, dtype=torch.int64, device="cuda")
        eager(ins, eouts, ebits)
        torch.cuda.synchronize()
        assert rec == gc.read_fit(eager.fit) and rec[1] == 0 and int(bits.item()) == int(ebits.item()) == rec[2]
        assert torch.equal(plan.table, eager.table)
        assert np.array_equal(_covered(obuf, ocover), _covered(ebuf, ecover)) and _gaps_clean(obuf, ocover)
        assert _untouched(ibuf, icover, x)
        recs.append(rec)
    assert recs[0] == LF.fit_record(LF.seam_table(3, False, 64), LF.budget_of(8.0, x1.size))
    assert recs[1][0] < recs[0][0]  # the fit followed the data


# ------------------------------------------------------------------------------------------------ 5. gradients
def test_gradients_fitted(gc, orc):
    torch.manual_seed(5)
    model = torch.nn.Sequential(torch.nn.Conv2d(3, 16, 3), torch.nn.Conv2d(16, 32, 3), torch.nn.Flatten(),
                                torch.nn.Linear(32 * 4 * 4, 80), torch.nn.Linear(80, 13)).cuda()
    model(torch.randn(4, 3, 8, 8, device="cuda")).square().sum().backward()
    params = list(model.parameters())
    n = sum(q.numel() for q in params)
    assert 40000 < n < 60000 and all(q.grad is not None for q in params)
    grads0 = [q.grad.clone() for q in params]
    bpv = 8.0
    flat = torch.cat([g.view(-1) for g in grads0])
    bits_ref = torch.zeros(1, dtype=torch.int64, device="cuda")
    ref = gc.roundtrip_fitted(flat, bpv, bits=bits_ref)
    cache = {}
    for rep in range(2):  # the second time on poisoned buffers: they exist after the first
        for q, g0 in zip(params, grads0):
            q.grad.copy_(g0)
        if rep:
            plan.table.fill_(POISON)
            plan.ws.fill_(POISON)
        bits = torch.full((1,), -1, dtype=torch.int64, device="cuda")
        plan = gc.roundtrip_gradients_fitted(params, bpv, bits=bits, cache=cache)
        torch.cuda.synchronize()
        got = torch.cat([q.grad.view(-1) for q in params])
        assert np.array_equal(_bits_of(got), _bits_of(ref)) and int(bits.item()) == int(bits_ref.item())
        assert int(bits.item()) <= int(bpv * n) and gc.read_fit(plan.fit)[1] == 0
        assert isinstance(plan, gc.TensorListFitted) and plan.rebuilds == 1 and list(cache.values()) == [plan]
        assert torch.equal(plan.table, gc.rate_table(flat))
    # roundtrip_gradients on the same parameters still works, under a cache entry of its own
    p = gc.accuracy(1e-3)
    for q, g0 in zip(params, grads0):
        q.grad.copy_(g0)
    plain = gc.roundtrip_gradients(params, p, cache=cache)
    torch.cuda.synchronize()
    assert plain is not plan and len(cache) == 2 and type(plain) is gc.TensorListRoundtrip
    assert np.array_equal(_bits_of(torch.cat([q.grad.view(-1) for q in params])), _bits_of(gc.roundtrip(flat, p)))
    # the default cache is the module's
    gc.gradient_plans.clear()
    plan = gc.roundtrip_gradients_fitted(params, bpv)
    torch.cuda.synchronize()
    assert list(gc.gradient_plans.values()) == [plan]
    gc.gradient_plans.clear()


# ------------------------------------------------------------------------------------------------ 6. refusals
def test_refusals(gc, orc):
    import gcow_amd
    assert gcow_amd.TensorListFitted is gc.TensorListFitted
    assert gcow_amd.roundtrip_gradients_fitted is gc.roundtrip_gradients_fitted
    a = torch.zeros(64, device="cuda")
    b = torch.zeros(64, device="cuda", dtype=torch.bfloat16)
    word = torch.tensor([-20], dtype=torch.int32, device="cuda")
    for call in (lambda ts, **kw: gc.roundtrip_tensors_fitted(ts, 8.0, **kw),
                 lambda ts, **kw: gc.roundtrip_tensors_fitted(ts, word, **kw),
                 lambda ts, **kw: gc.TensorListFitted(8.0)(ts, **kw)):
        with pytest.raises(gc.GcowError):
            call([a, b])                                              # mixed dtypes
        with pytest.raises(gc.GcowError):
            call([a, torch.zeros(4)])                                 # a host tensor
        with pytest.raises(gc.GcowError):
            call([torch.zeros(128, device="cuda")[::2]])              # not contiguous
        with pytest.raises(gc.GcowError):
            call([a], outs=[torch.zeros(63, device="cuda")])          # outs of the wrong sizes
        with pytest.raises(gc.GcowError):
            call([a], outs=[a, a])
        with pytest.raises(gc.GcowError):
            call([a], bits=torch.zeros(1, dtype=torch.int32, device="cuda"))   # bits of the wrong dtype
    for ts in ([a, b], [a, torch.zeros(4)], [torch.zeros(128, device="cuda")[::2]], [a.to(torch.float16)]):
        with pytest.raises(gc.GcowError):
            gc.rate_table_tensors(ts)
    other = gc.TensorListFitted(8.0, 12)
    with pytest.raises(gc.GcowError):
        gc.roundtrip_tensors_fitted([a], 8.0, plan=other)             # a plan object of another maxprec
    with pytest.raises(gc.GcowError):
        gc.rate_table_tensors([a], 64, plan=other)
    with pytest.raises(gc.GcowError):
        gc.roundtrip_tensors_fitted([a], 8.0, plan=gc.TensorListRoundtrip(gc.accuracy(1e-3)))
    with pytest.raises(gc.GcowError):
        gc.roundtrip_tensors_fitted([a], torch.tensor([-20], dtype=torch.int32))   # a host word
    with pytest.raises(gc.GcowError):
        gc.roundtrip_tensors_fitted([a], "8")
    assert not a.any() and other.rebuilds == 0
    torch.cuda.synchronize()
