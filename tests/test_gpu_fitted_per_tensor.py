"""GPU parity of the bit budget per tensor (gcow_rate_table_rel_device, gcow_rate_table_fit_batch_device,
gcow_roundtrip_rel_fitted_device; codec.TensorListFittedPerTensor and the functions around it;
DeviceCodec.roundtrip_fitted_per_tensor; roundtrip_hook with per_tensor_budget), bitwise against the per-tensor oracle
expectation of tests/fitted_per_tensor_inputs.py:

  1. every row of the tables against the oracle's table of that tensor as a field of its own, over the lists of
     relative_inputs.py (edges, small, special, hook), fp32 / bf16, maxprec 64 / 12, the tensors carved from one buffer
     at aligned bases and at odd element offsets; tables and workspace poisoned, the words after the last row intact;
  2. the records of the batch fit against the restated rule, at 8, 2.5 and 0.5 bits per value and floors -154 / -94;
  3. the round trip against the oracle's decode of each tensor under its fitted minexp and the summed bit count: the
     whole call, four dtype pairs, in place and out of place, whole allocations compared (sentinels between and after
     the tensors); minexp words at stride 4 (the records) and stride 1 (packed words, some outside [-154, 133]);
  4. a list whose direct chunks outnumber the grid, so that a workgroup's run crosses tensors, against
     codec.rate_table of each tensor; two runs give the same bits;
  5. tables -> fits -> round trip captured into one graph and replayed on changed data;
  6. roundtrip_hook with per_tensor_budget at world 1, and roundtrip_gradients_fitted_per_tensor on a small module."""
import os
import sys

import numpy as np
import pytest

torch = pytest.importorskip("torch")

TESTS = os.path.dirname(os.path.abspath(__file__))
if TESTS not in sys.path:
    sys.path.insert(0, TESTS)

import fitted_per_tensor_inputs as F  # noqa: E402
import list_fitted_inputs as LF  # noqa: E402
from relative_inputs import HOOK_SIZES, tensors  # noqa: E402

pytestmark = pytest.mark.gpu

DTYPES = [(False, False), (True, True), (False, True), (True, False)]
DTYPE_IDS = ["fp32-fp32", "bf16-bf16", "fp32-bf16", "bf16-fp32"]
SENT = {False: np.float32(-1234.5).view(np.uint32), True: np.uint16(0xC49A)}  # sentinel bits (bf16: -1232.0)
POISON = F.POISON


@pytest.fixture(scope="module")
def gc():
    if not torch.cuda.is_available():
        pytest.fail("GPU tests need a device")
    from gcow_amd import codec
    return codec


def _bits_of(t):
    if t.dtype == torch.bfloat16:
        return t.view(torch.int16).cpu().numpy().view(np.uint16)
    return t.cpu().numpy().view(np.uint32)


def _as_bits(a, bf16):
    return a if bf16 else a.view(np.uint32)


def _upload(bits_np, bf16):
    if bf16:
        return torch.from_numpy(bits_np.view(np.int16)).cuda().view(torch.bfloat16)
    return torch.from_numpy(bits_np.view(np.float32)).cuda()


class Carved:
    """Tensors carved out of one sentinel-filled device buffer (list_fitted_inputs.layout: gaps of at least 3 elements,
    16 elements of tail; aligned bases or odd element offsets). `host` is the buffer's expected bits."""

    def __init__(self, sizes, bf16, aligned, arrays=None):
        self.bf16, self.sizes = bf16, list(sizes)
        self.pos, total = LF.layout(self.sizes, aligned)
        self.host = np.full(total, SENT[bf16], np.uint16 if bf16 else np.uint32)
        if arrays is not None:
            self.put(arrays)
        self.buf = _upload(self.host, bf16)
        self.tensors = [self.buf[p:p + n] for p, n in zip(self.pos, self.sizes)]

    def put(self, arrays):
        """Write per-tensor bits into the expected image."""
        for p, n, a in zip(self.pos, self.sizes, arrays):
            self.host[p:p + n] = a

    def same(self):
        """The whole allocation against the expected image."""
        return np.array_equal(_bits_of(self.buf), self.host)


def _want(outs_ref, bf16_out):
    from roundtrip_inputs import bf16_rne
    return [bf16_rne(d) if bf16_out else d.view(np.uint32) for d in outs_ref]


def _inputs(name, bf16, aligned):
    ts_np = tensors(name, bf16)
    return Carved([t.size for t in ts_np], bf16, aligned, [_as_bits(t, bf16) for t in ts_np])


def _records(fits):
    """int64[S, 2] records -> [(minexp, status, bits)]."""
    a = fits.cpu().numpy()
    out = []
    for w0, w1 in a:
        me = int(w0) & 0xFFFFFFFF
        out.append((me - (1 << 32) if me >> 31 else me, (int(w0) >> 32) & 0xFFFFFFFF, int(w1)))
    return out


# ------------------------------------------------------------------------------------------------------- 1. tables
def _poisoned_tables(plan, n):
    """Point the plan object at tables inside a larger poisoned buffer; -> that buffer (S + 1 rows)."""
    big = torch.full(((n + 1) * 288,), POISON, dtype=torch.int64, device="cuda")
    plan.tables = big[:n * 288].view(n, 288)
    plan.ws.fill_(POISON)
    return big


@pytest.mark.parametrize("aligned", [True, False], ids=["aligned", "odd"])
@pytest.mark.parametrize("bf16", [False, True], ids=["fp32", "bf16"])
@pytest.mark.parametrize("name,maxprec", [(n, m) for n in F.LISTS for m in F.maxprecs(n)])
def test_tables(gc, orc, name, maxprec, bf16, aligned):
    ins = _inputs(name, bf16, aligned)
    n = len(ins.sizes)
    plan = gc.TensorListFittedPerTensor(8.0, maxprec)
    assert gc.rate_tables_tensors(ins.tensors, maxprec, plan=plan) is plan.tables  # plans and allocates
    big = _poisoned_tables(plan, n)
    got = plan.rate_tables(ins.tensors)
    torch.cuda.synchronize()
    assert plan.rebuilds == 1 and got.data_ptr() == big.data_ptr()
    want = F.tables(name, bf16, maxprec)
    g = got.cpu().numpy()
    bad = [s for s in range(n) if not np.array_equal(g[s], want[s])]
    assert not bad, (bad[:8], [ins.sizes[s] for s in bad[:8]])
    for s, size in enumerate(ins.sizes):
        if size == 0:
            assert not g[s].any()
    assert bool((big[n * 288:] == POISON).all())  # nothing past the last row
    assert ins.same()                              # the inputs are only read
    st = plan.stats()
    assert st.gather_chunks > 0
    if name == "edges" and aligned:
        assert st.direct_chunks == 7  # 8191, 8192, 8193 values: one chunk each; 24583: 6145 whole blocks, four chunks


# --------------------------------------------------------------------------------------------------------- 2. fits
@pytest.mark.parametrize("floor", F.FLOORS)
@pytest.mark.parametrize("bpv", F.BPVS)
@pytest.mark.parametrize("name,bf16", [("edges", False), ("special", False), ("special", True), ("small", True)])
def test_fits(gc, orc, name, bf16, bpv, floor):
    T = F.tables(name, bf16, 64)
    sizes = [t.size for t in tensors(name, bf16)]
    n = len(sizes)
    tables = torch.from_numpy(np.array(T)).cuda()
    budgets = torch.tensor([F.budget_of(bpv, k) for k in sizes], dtype=torch.int64, device="cuda")
    big = torch.full((2 * (n + 1),), POISON, dtype=torch.int64, device="cuda")
    out = gc.fit_device_batch(tables, budgets, floor, out=big[:2 * n].view(n, 2))
    torch.cuda.synchronize()
    assert _records(out) == list(F.fits(name, bf16, 64, bpv, floor))
    assert np.array_equal(out.cpu().numpy(), F.records_array(F.fits(name, bf16, 64, bpv, floor)))
    assert bool((big[2 * n:] == POISON).all())
    assert np.array_equal(tables.cpu().numpy(), T)  # the tables are only read


def test_fit_batch_of_one_is_the_single_fit(gc, orc):
    T = F.tables("hook", False, 64)
    for s in range(T.shape[0]):
        row = torch.from_numpy(np.array(T[s:s + 1])).cuda()
        for budget in (int(T[s][287]) - 1, int(T[s][287]), F.budget_of(8.0, HOOK_SIZES[s]), int(T[s][0])):
            one = gc.fit_device(row[0], budget)
            many = gc.fit_device_batch(row, torch.tensor([budget], dtype=torch.int64, device="cuda"), -154)
            torch.cuda.synchronize()
            assert gc.read_fit(one) == _records(many)[0]


# --------------------------------------------------------------------------------------------------- 3. round trip
def _whole_call(gc, name, bf16_in, bf16_out, maxprec, bpv, aligned):
    outs_ref, bits_ref, rec = F.expect(name, bf16_in, maxprec, bpv)
    want = _want(outs_ref, bf16_out)
    ins = _inputs(name, bf16_in, aligned)
    outs = Carved(ins.sizes, bf16_out, aligned)
    bits = torch.full((1,), -1, dtype=torch.int64, device="cuda")
    plan = gc.TensorListFittedPerTensor(bpv, maxprec)
    got = gc.roundtrip_tensors_fitted_per_tensor(ins.tensors, bpv, maxprec, outs=outs.tensors, bits=bits, plan=plan)
    torch.cuda.synchronize()
    assert [g.data_ptr() for g in got] == [o.data_ptr() for o in outs.tensors]
    assert _records(plan.fits) == list(rec)
    assert plan.budgets.tolist() == [F.budget_of(bpv, k) for k in ins.sizes]
    outs.put(want)
    assert outs.same() and ins.same()  # whole allocations: sentinels between and after the tensors, inputs only read
    assert int(bits.item()) == bits_ref == sum(r[2] for r, k in zip(rec, ins.sizes) if k)
    assert all(r[2] <= F.budget_of(bpv, k) for r, k in zip(rec, ins.sizes) if r[1] == 0)
    if bf16_in == bf16_out:  # in place, the bit count kept on the plan object
        plan2 = gc.TensorListFittedPerTensor(bpv, maxprec)
        plan2(ins.tensors)
        torch.cuda.synchronize()
        ins.put(want)
        assert ins.same() and int(plan2.bits.item()) == bits_ref and _records(plan2.fits) == list(rec)


@pytest.mark.parametrize("aligned", [True, False], ids=["aligned", "odd"])
@pytest.mark.parametrize("bf16_in,bf16_out", DTYPES, ids=DTYPE_IDS)
@pytest.mark.parametrize("name", ["edges", "small", "special"])
def test_roundtrip_whole_call(gc, orc, name, bf16_in, bf16_out, aligned):
    _whole_call(gc, name, bf16_in, bf16_out, 64, 8.0, aligned)


@pytest.mark.parametrize("bpv,maxprec", [(2.5, 64), (0.5, 64), (8.0, 12)])
@pytest.mark.parametrize("bf16", [False, True], ids=["fp32", "bf16"])
def test_roundtrip_other_budgets(gc, orc, bf16, bpv, maxprec):
    _whole_call(gc, "edges", bf16, bf16, maxprec, bpv, False)
    _whole_call(gc, "special", bf16, not bf16, maxprec, bpv, True)


@pytest.mark.parametrize("bf16_in,bf16_out", DTYPES, ids=DTYPE_IDS)
@pytest.mark.parametrize("stride", [4, 1])
def test_roundtrip_under_given_words(gc, orc, stride, bf16_in, bf16_out):
    """The round trip alone under hand-written words: the records of another budget (stride 4) or packed int32 words
    (stride 1), some outside [-154, 133], which are clamped."""
    name = "edges"
    ins = _inputs(name, bf16_in, False)
    n = len(ins.sizes)
    words = [-1000, -154, -30, 500, 0, -20, -12, 133, -155, 134, -7][:n]
    assert len(words) == n
    if stride == 4:
        rec = np.zeros((n, 2), np.int64)
        rec[:, 0] = [(w & 0xFFFFFFFF) | (1 << 32) for w in words]  # a status word beside it: not read
        rec[:, 1] = POISON
        fits = torch.from_numpy(rec).cuda()
    else:
        fits = torch.tensor(words, dtype=torch.int32, device="cuda")
    keep = fits.clone()
    outs_ref, bits_ref = F.expect_words(name, bf16_in, 64, words)
    outs = Carved(ins.sizes, bf16_out, False)
    bits = torch.full((1,), -1, dtype=torch.int64, device="cuda")
    gc.roundtrip_tensors_fitted_per_tensor(ins.tensors, fits, 64, outs=outs.tensors, bits=bits)
    torch.cuda.synchronize()
    outs.put(_want(outs_ref, bf16_out))
    assert outs.same() and ins.same() and int(bits.item()) == bits_ref
    assert torch.equal(fits, keep)  # the words are only read


def test_equals_roundtrip_fitted_per_tensor(gc, orc):
    """Against the library's own contiguous fitted round trip of each tensor under its record."""
    ins = _inputs("edges", False, True)
    plan = gc.TensorListFittedPerTensor(8.0)
    outs = plan(ins.tensors, outs=[torch.empty_like(t) for t in ins.tensors])
    for s, (t, o) in enumerate(zip(ins.tensors, outs)):
        if t.numel() == 0:
            continue
        ref = gc.roundtrip_fitted(t.clone(), plan.fits[s])
        torch.cuda.synchronize()
        assert np.array_equal(_bits_of(o), _bits_of(ref)), s


# ------------------------------------------------------------------------- 4. a run of chunks over several tensors
def test_runs_cross_tensors_and_are_deterministic(gc, orc):
    """Five tensors of 300 direct chunks each: 1500 chunks for a grid of at most 1024 runs, so runs hold one or two
    chunks and some cross from one tensor into the next. Too large for the oracle: against codec.rate_table of each
    tensor (pinned to the oracle by tests/test_gpu_rate_table.py)."""
    import re
    from gcow_amd import _ffi
    src = open(os.path.join(_ffi.HERE, "csrc", "kernels.h")).read()
    cap = int(re.search(r"constexpr uint32_t kRateTableRelMaxGrid = (\d+);", src).group(1))
    per, n = 300 * 8192, 5
    gen = torch.Generator(device="cuda").manual_seed(5)
    buf = torch.randn(n * per, generator=gen, device="cuda")
    ts = [buf[s * per:(s + 1) * per] for s in range(n)]
    for s, t in enumerate(ts):
        t.mul_(2.0 ** (-12 + 7 * s))
    plan = gc.TensorListFittedPerTensor(8.0)
    first = plan.rate_tables(ts).clone()
    st = plan.stats()
    assert st.direct_chunks == n * 300 > cap and st.gather_chunks == 0
    big = _poisoned_tables(plan, n)
    second = plan.rate_tables(ts)
    torch.cuda.synchronize()
    assert torch.equal(first, second) and bool((big[n * 288:] == POISON).all())
    for s, t in enumerate(ts):
        assert torch.equal(second[s], gc.rate_table(t)), s
    assert len({int(second[s][150]) for s in range(n)}) == n  # the scales tell the rows apart


def test_determinism_on_gather_lists(gc, orc):
    ins = _inputs("small", True, False)
    plan = gc.TensorListFittedPerTensor(8.0)
    a = plan.rate_tables(ins.tensors).clone()
    plan.ws.fill_(POISON)
    b = plan.rate_tables(ins.tensors)
    torch.cuda.synchronize()
    assert torch.equal(a, b)


# --------------------------------------------------------------------------------------------------------- 5. graph
def test_graph_capture_follows_the_data(gc, orc):
    """Tables, fits and round trip captured as one linear chain and replayed on two contents of the same tensors; the
    second is the first with every tensor scaled by another power of two, so every record moves."""
    ts_np = tensors("edges", False)
    ins = _inputs("edges", False, True)
    outs = Carved(ins.sizes, False, True)
    eouts = Carved(ins.sizes, False, True)
    plan = gc.TensorListFittedPerTensor(8.0)
    bits = torch.full((1,), -1, dtype=torch.int64, device="cuda")
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        plan(ins.tensors, outs.tensors, bits)  # plans, uploads and allocates outside the capture
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        plan(ins.tensors, outs.tensors, bits)
    assert plan.rebuilds == 1
    eager = gc.TensorListFittedPerTensor(8.0)
    seen = []
    for rnd in range(2):
        if rnd == 1:
            for s, t in enumerate(ins.tensors):
                t.mul_(2.0 ** (3 + s % 4))
        outs.buf.copy_(_upload(outs.host, False))
        bits.fill_(-1)
        plan.tables.fill_(POISON)
        plan.fits.fill_(POISON)
        plan.ws.fill_(POISON)
        g.replay()
        torch.cuda.synchronize()
        ebits = torch.full((1,), -1, dtype=torch.int64, device="cuda")
        eager(ins.tensors, eouts.tensors, ebits)
        torch.cuda.synchronize()
        assert torch.equal(outs.buf.view(torch.int32), eouts.buf.view(torch.int32)), rnd
        assert torch.equal(plan.fits, eager.fits) and torch.equal(plan.tables, eager.tables), rnd
        assert int(bits.item()) == int(ebits.item()) > 0
        seen.append(_records(plan.fits))
    outs_ref, bits_ref, rec = F.expect("edges", False, 64, 8.0)
    assert seen[0] == list(rec)
    live = [s for s, t in enumerate(ts_np) if t.size]
    assert all(seen[1][s][0] == seen[0][s][0] + 3 + s % 4 for s in live)  # scaled by 2^k: minexp + k, the same bits
    assert all(seen[1][s][2] == seen[0][s][2] for s in live)


# ------------------------------------------------------------------------------------------- 6. hook and gradients
@pytest.fixture
def nccl_world1():
    import torch.distributed as dist
    dist.init_process_group("nccl", store=dist.HashStore(), rank=0, world_size=1, device_id=torch.device("cuda", 0))
    yield
    dist.destroy_process_group()


class _Bucket:
    def __init__(self, t, i, sizes):
        self.t, self.i, self.sizes = t, i, sizes

    def buffer(self):
        return self.t

    def index(self):
        return self.i

    def gradients(self):
        out, at = [], 0
        for n in self.sizes:
            out.append(self.t[at:at + n])
            at += n
        return out


@pytest.mark.parametrize("bf16", [False, True], ids=["fp32", "bf16"])
def test_roundtrip_hook_per_tensor_budget_world1(gc, orc, nccl_world1, bf16):
    """One rank over RCCL: the hook round-trips the bucket's per-parameter views in place, each under its own budget,
    fitted on the device; it neither encodes nor takes the bucket's own table."""
    from gcow_amd import ddp
    from gcow_amd import dist as gdist

    calls = []

    class CountingCodec(gdist.DeviceCodec):
        def roundtrip_fitted_per_tensor(self, *a, **k):
            calls.append("roundtrip_fitted_per_tensor")
            return super().roundtrip_fitted_per_tensor(*a, **k)

        def rate_table(self, *a, **k):
            calls.append("rate_table")
            return super().rate_table(*a, **k)

        def roundtrip(self, *a, **k):
            calls.append("roundtrip")
            return super().roundtrip(*a, **k)

        def encode(self, *a, **k):
            calls.append("encode")
            return super().encode(*a, **k)

    cdc = CountingCodec()
    state = ddp.make_hook_state(hook=ddp.roundtrip_hook, params=gc.accuracy(1e-3), codec=cdc, target_bits=8,
                                per_tensor_budget=True)
    ts_np = tensors("hook", bf16)
    outs_ref, bits_ref, rec = F.expect("hook", bf16, 64, 8.0)
    want = np.concatenate(_want(outs_ref, bf16))
    flat = np.concatenate([_as_bits(t, bf16) for t in ts_np])
    for i in range(2):  # the second bucket index gets a plan of its own
        t = _upload(flat.copy(), bf16)
        out = ddp.roundtrip_hook(state, _Bucket(t, i, HOOK_SIZES)).wait()
        torch.cuda.synchronize()
        out = out[0] if isinstance(out, (list, tuple)) else out
        assert out.data_ptr() == t.data_ptr()
        assert np.array_equal(_bits_of(out), want), i
        assert _records(state.fit_record(i)) == list(rec)
        assert sum(r[2] for r in _records(state.fit_record(i))) == bits_ref <= sum(F.budget_of(8.0, k) for k in HOOK_SIZES)
    assert calls == ["roundtrip_fitted_per_tensor"] * 2 and not state._fits


def test_gradients_end_to_end(gc, orc):
    import gcow_amd
    assert gcow_amd.roundtrip_gradients_fitted_per_tensor is gc.roundtrip_gradients_fitted_per_tensor
    torch.manual_seed(3)
    model = torch.nn.Sequential(torch.nn.Linear(96, 128), torch.nn.LayerNorm(128), torch.nn.Linear(128, 10)).cuda()
    model(torch.randn(32, 96, device="cuda")).square().sum().backward()
    params = list(model.parameters())
    before = [q.grad.clone() for q in params]
    cache = {}
    bits = torch.zeros(1, dtype=torch.int64, device="cuda")
    plan = gc.roundtrip_gradients_fitted_per_tensor(params, 8.0, bits=bits, cache=cache)
    torch.cuda.synchronize()
    rec = _records(plan.fits)
    assert list(cache.values()) == [plan] and plan.rebuilds == 1 and len(rec) == len(params)
    assert int(bits.item()) == sum(r[2] for r in rec) <= sum(F.budget_of(8.0, g.numel()) for g in before)
    for s, (g0, q) in enumerate(zip(before, params)):
        ref = gc.roundtrip_fitted(g0.view(-1), plan.fits[s]).view_as(g0)
        assert torch.equal(ref, q.grad), s
        assert rec[s][1] == 0 and rec[s][0] >= -94
        assert float((q.grad - g0).abs().max()) <= 2.0 ** rec[s][0]
    for q, g0 in zip(params, before):
        q.grad.copy_(g0)
    assert gc.roundtrip_gradients_fitted_per_tensor(params, 8.0, cache=cache) is plan and plan.rebuilds == 1
    assert gc.roundtrip_gradients_fitted_per_tensor(params, 4.0, cache=cache) is not plan
    torch.cuda.synchronize()


def test_refusals_and_empty_lists(gc, orc):
    a = torch.zeros(64, device="cuda")
    with pytest.raises(gc.GcowError):
        gc.roundtrip_tensors_fitted_per_tensor([a.to(torch.float16)], 8.0)
    with pytest.raises(gc.GcowError):
        gc.roundtrip_tensors_fitted_per_tensor([a], torch.zeros(2, dtype=torch.int32, device="cuda"))  # two words for one
    with pytest.raises(gc.GcowError):
        gc.roundtrip_tensors_fitted_per_tensor([a], 8.0, plan=gc.TensorListFittedPerTensor(4.0))
    with pytest.raises(gc.GcowError):
        gc.rate_tables_tensors([a], 12, plan=gc.TensorListFittedPerTensor(4.0, 64))
    bits = torch.full((1,), -1, dtype=torch.int64, device="cuda")
    assert gc.roundtrip_tensors_fitted_per_tensor([], 8.0, bits=bits) == []
    torch.cuda.synchronize()
    assert int(bits.item()) == 0
    bits.fill_(-1)
    plan = gc.TensorListFittedPerTensor(8.0)
    plan([torch.zeros(0, device="cuda")] * 2, bits=bits)
    torch.cuda.synchronize()
    assert int(bits.item()) == 0 and not plan.tables.any() and _records(plan.fits) == [(-94, 0, 0)] * 2
    assert gc.rate_tables_tensors([]).shape == (0, 288)
