"""GPU checks of the fit on the device and of the calls that take minexp from device memory (include/gcow.h:
gcow_rate_table_fit_device, gcow_encode_fitted_device, gcow_roundtrip_fitted_device; codec.FittedEncoder), bit for bit:

  - the fit kernel on uploaded tables against the host gcow_rate_table_fit (or the status = 1 rule), with a sentinel
    after every record;
  - the fitted encode against codec.encode under the clamped set, for in-range and out-of-range device words, fp32 and
    bf16, maxprec 64 / 20 / 0, index strides 0 / 8 / 16, and against the oracle; oversized tiles; dirty buffers;
  - the fitted round trip against codec.roundtrip under the clamped set, in and out of place, mixed dtypes;
  - FittedEncoder against codec.encode_fitted; a stream capture of table + fit + encode replayed on other data;
  - argument checks; the hooks' fit_on_device over a one-rank RCCL group.

Sizes follow the tile encoder's geometry: a tile is 4096 values, a count workgroup covers 8 tiles (32768 values), a
round-trip chunk is 8192 values."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

torch = pytest.importorskip("torch")

TESTS = os.path.dirname(os.path.abspath(__file__))
if TESTS not in sys.path:
    sys.path.insert(0, TESTS)

import fit_device_inputs as FI  # noqa: E402

pytestmark = pytest.mark.gpu

TILE, COUNT_WG = 4096, 32768
SIZES = [1, 3, 5, 4095, 4096, 4097, 8191, 8192, 8197, COUNT_WG + 5, 3 * COUNT_WG + TILE + 7]
BIG = 3 * TILE + 7
WORDS = [-154, -40, -20, -10, 0, 100, 133, -155, 134, -2 ** 31, 2 ** 31 - 1]
MAXPRECS = [64, 20, 0]
STRIDES = [0, 8, 16]
SENT = 0x5A5A5A5A5A5A5A5A


@pytest.fixture(scope="module")
def gc(orc):
    if not torch.cuda.is_available():
        pytest.fail("GPU tests need a device")
    from gcow_amd import codec
    return codec


def _stream():
    return torch.cuda.current_stream().cuda_stream


def _dev(a):
    t = torch.from_numpy(np.array(a)).cuda()  # a writable copy: the cases' arrays are shared and read-only
    return t.view(torch.bfloat16) if a.dtype == np.uint16 else t


def _word(v):
    return torch.tensor([v], dtype=torch.int32, device="cuda")


def _same_stream(a, b, what):
    """Two Encoded: the bit count, the flushed stream words and the index."""
    assert a.bits == b.bits, what
    nw = (a.bits + 63) // 64
    assert torch.equal(a.words[:nw], b.words[:nw]), what
    assert (a.index is None) == (b.index is None), what
    if a.index is not None:
        ne = ((a.shape[0] + 3) // 4 + a.index_stride - 1) // a.index_stride
        assert torch.equal(a.index[:ne], b.index[:ne]), what


# ------------------------------------------------------------------------------------------------ the fit kernel
def _tables():
    import rate_table_inputs as RT
    out = [("plateau", FI.plateau_table()), ("constant", FI.constant_table()), ("decreasing", FI.decreasing_table()),
           ("huge", FI.huge_table())]
    for n in (5, BIG):
        out.append(("crafted%d" % n, np.array(RT.crafted_table(n, False, 64)[1])))
    return out


@pytest.mark.parametrize("name", ["plateau", "constant", "decreasing", "huge", "crafted5", "crafted%d" % BIG])
def test_fit_kernel_matches_host_fit(gc, orc, name):
    L = gc.load()
    table = dict(_tables())[name].astype(np.int64)
    tu = table.view(np.uint64)
    budgets = FI.budgets(tu)
    d_table = torch.from_numpy(table.copy()).cuda()
    h_table = (C.c_uint64 * 288)(*[int(v) for v in tu])
    # one record and 16 bytes of sentinel per budget, all launched before one synchronise
    buf = torch.full((len(budgets), 4), SENT, dtype=torch.int64, device="cuda")
    for k, b in enumerate(budgets):
        assert L.gcow_rate_table_fit_device(d_table.data_ptr(), b, buf[k].data_ptr(), _stream()) == 0
    torch.cuda.synchronize()
    got = buf.cpu().numpy()
    assert (got[:, 2:] == SENT).all(), "the 16 bytes after a record were written"
    assert np.array_equal(d_table.cpu().numpy(), table)
    nfail = 0
    for k, b in enumerate(budgets):
        me, bits = C.c_int(0), C.c_uint64(0)
        st = L.gcow_rate_table_fit(h_table, b, C.byref(me), C.byref(bits))
        want = (me.value, 0, bits.value) if st == 0 else (FI.MINEXP_HI, 1, int(tu[287]))
        nfail += st != 0
        assert gc.read_fit(torch.from_numpy(got[k, :2].copy())) == want, (name, b)
        assert want == FI.model_fit(tu, b)
    assert nfail >= 1  # budget 0 is below every table's last entry


# ------------------------------------------------------------------------------------------------ the fitted encode
@pytest.mark.parametrize("bf16", [False, True], ids=["fp32", "bf16"])
@pytest.mark.parametrize("n", SIZES)
def test_encode_fitted_matches_host_params(gc, orc, n, bf16):
    import roundtrip_inputs as RI
    x = _dev(RI.inputs(n, bf16))
    ref = {}
    for maxprec in MAXPRECS:
        for stride in STRIDES:
            for w in WORDS:
                m = FI.clamp(w)
                key = (maxprec, stride, m)
                if key not in ref:
                    ref[key] = gc.encode(x, gc.expert(1, 16658, maxprec, m), stride)
                word = _word(w)
                got = gc.encode_fitted_device(x, word, maxprec, stride)
                torch.cuda.synchronize()
                _same_stream(got, ref[key], (n, bf16, maxprec, stride, w))
                assert int(word.item()) == w  # d_minexp is read, never written


@pytest.mark.parametrize("n", SIZES)
def test_encode_fitted_matches_oracle(gc, orc, n):
    import roundtrip_inputs as RI
    O = orc
    x_np = RI.inputs(n, False)
    x = _dev(x_np)
    for w in (-155, -20, 100):
        got = gc.encode_fitted_device(x, _word(w), 64, 8)
        torch.cuda.synchronize()
        op = O.expert(1, 16658, 64, FI.clamp(w))
        w_ref, bits_ref = O.compress(x_np, op)
        assert got.bits == bits_ref and got.to_bytes() == w_ref.tobytes(), (n, w)
        lens = O.block_bits(x_np, op).astype(np.uint64)
        offs = np.concatenate([[0], np.cumsum(lens)[:-1]]).astype(np.uint64)[::8]
        assert np.array_equal(got.index[:offs.size].cpu().numpy().view(np.uint64), offs), (n, w)


def test_encode_fitted_unaligned_input(gc, orc):
    """A view one element off 16-byte alignment: the gather path of the count and tile kernels."""
    import roundtrip_inputs as RI
    for bf16 in (False, True):
        a = RI.inputs(TILE + 9, bf16)
        base = _dev(np.concatenate([a[:1], a]))
        x = base[1:]
        assert x.data_ptr() % 16 != 0
        got = gc.encode_fitted_device(x, _word(-20), 64, 16)
        ref = gc.encode(x, gc.expert(1, 16658, 64, -20), 16)
        torch.cuda.synchronize()
        _same_stream(got, ref, bf16)


def _all_exponents(n):
    """Block b holds values of biased exponent b mod 255 with random mantissas and signs (test_contention_all_bins of
    test_gpu_rate_table.py): at full precision most blocks take well over 95 bits."""
    rng = np.random.default_rng(77)
    nb = (n + 3) // 4
    e = (np.arange(nb, dtype=np.uint32) % 255).repeat(4)[:n]
    bits = (e << 23) | rng.integers(0, 1 << 23, n, dtype=np.uint32) | (rng.integers(0, 2, n, dtype=np.uint32) << 31)
    x = bits.astype(np.uint32).view(np.float32)
    assert np.isfinite(x).all()
    return x


def test_encode_fitted_oversized_tiles(gc, orc):
    O = orc
    n = 3 * TILE + 7
    x_np = _all_exponents(n)
    op = O.expert(1, 16658, 64, -154)
    lens = O.block_bits(x_np, op).astype(np.int64)
    tiles = [int(lens[t:t + TILE // 4].sum()) for t in range(0, lens.size, TILE // 4)]
    # the small window holds 1500 qwords = 96000 bits, 128 of which the tile's start may take
    assert max(tiles[:3]) > 96 * (TILE // 4), tiles  # at least one whole tile is coded by the _big kernel
    x = _dev(x_np)
    for stride in (0, 8):
        got = gc.encode_fitted_device(x, _word(-154), 64, stride)
        ref = gc.encode(x, gc.expert(1, 16658, 64, -154), stride)
        torch.cuda.synchronize()
        _same_stream(got, ref, stride)
    w_ref, bits_ref = O.compress(x_np, op)
    assert got.bits == bits_ref and got.to_bytes() == w_ref.tobytes()


def _raw_encode(gc, f, maxprec, word_ptr, words, cap, bits, ws, wsb, index, stride):
    return gc.load().gcow_encode_fitted_device(C.byref(f), maxprec, word_ptr, words.data_ptr() if words is not None
                                               else None, cap, bits.data_ptr(), ws.data_ptr() if ws is not None
                                               else None, wsb, index.data_ptr() if index is not None else None,
                                               stride, _stream())


@pytest.mark.parametrize("n", [5, 8197, COUNT_WG + 5])
def test_encode_fitted_dirty_buffers(gc, orc, n):
    """Sentinel-filled stream, index, workspace and bit count; a second input with a shorter stream into the same
    buffers; the bytes past gcow_max_output_bytes and the minexp word stay as they were."""
    import roundtrip_inputs as RI
    L = gc.load()
    x1 = _dev(RI.inputs(n, False))
    x2 = _dev(RI.inputs(n, False, seed=77) * np.float32(2.0 ** -8))
    hp = gc.fitted_params(64, 0)
    f = gc.field_of(x1)
    cap = L.gcow_max_output_bytes(C.byref(f), C.byref(hp))
    wsb = L.gcow_encode_workspace_bytes(C.byref(f), C.byref(hp))
    for me in (-154, 133):  # neither query depends on minexp
        q = gc.fitted_params(64, me)
        assert L.gcow_max_output_bytes(C.byref(f), C.byref(q)) == cap
        assert L.gcow_encode_workspace_bytes(C.byref(f), C.byref(q)) == wsb
    ne = L.gcow_index_entries(C.byref(f), 8)
    for fill in (-1, SENT):
        words = torch.full((cap // 8 + 4,), fill, dtype=torch.int64, device="cuda")
        ws = torch.full((wsb // 8 + 1,), fill, dtype=torch.int64, device="cuda")
        index = torch.full((ne + 4,), fill, dtype=torch.int64, device="cuda")
        bits = torch.full((1,), fill, dtype=torch.int64, device="cuda")
        rec = torch.tensor([-20, 0x5A5A5A5A, 7, 7], dtype=torch.int32, device="cuda")
        for x in (x1, x2):
            assert _raw_encode(gc, gc.field_of(x), 64, rec.data_ptr(), words, cap, bits, ws, wsb, index, 8) == 0
            ref = gc.encode(x, gc.expert(1, 16658, 64, -20), 8)
            torch.cuda.synchronize()
            assert int(bits.item()) == ref.bits
            nw = (ref.bits + 63) // 64
            assert torch.equal(words[:nw], ref.words[:nw])
            assert bool((words[cap // 8:] == fill).all()), "the words after the capacity were written"
            assert torch.equal(index[:ne], ref.index[:ne]) and bool((index[ne:] == fill).all())
            assert rec.tolist() == [-20, 0x5A5A5A5A, 7, 7]


# ------------------------------------------------------------------------------------------------ the fitted round trip
DT = {"fp32": torch.float32, "bf16": torch.bfloat16}


@pytest.mark.parametrize("io", ["fp32-fp32", "bf16-bf16", "fp32-bf16"])
@pytest.mark.parametrize("n", SIZES)
def test_roundtrip_fitted_matches_host_params(gc, orc, n, io):
    import roundtrip_inputs as RI
    din, dout = (DT[s] for s in io.split("-"))
    x = _dev(RI.inputs(n, din == torch.bfloat16))
    bits_a = torch.zeros(1, dtype=torch.int64, device="cuda")
    bits_b = torch.full((1,), SENT, dtype=torch.int64, device="cuda")
    for maxprec in (64, 20):
        table = gc.rate_table(x, maxprec).cpu().numpy()
        for w in WORDS:
            m = FI.clamp(w)
            p = gc.expert(1, 16658, maxprec, m)
            want = gc.roundtrip(x, p, out=torch.empty(n, dtype=dout, device="cuda"), bits=bits_a)
            got = gc.roundtrip_fitted(x, _word(w), maxprec, out=torch.empty(n, dtype=dout, device="cuda"), bits=bits_b)
            torch.cuda.synchronize()
            assert torch.equal(got.view(torch.int16 if dout == torch.bfloat16 else torch.int32),
                               want.view(torch.int16 if dout == torch.bfloat16 else torch.int32)), (n, io, maxprec, w)
            assert int(bits_b.item()) == int(bits_a.item()) == int(table[m - FI.MINEXP_LO]), (n, io, maxprec, w)
            if din == dout:  # in place
                y = x.clone()
                assert gc.roundtrip_fitted(y, _word(w), maxprec, out=y) is y
                torch.cuda.synchronize()
                assert torch.equal(y.view(torch.int16 if dout == torch.bfloat16 else torch.int32),
                                   want.view(torch.int16 if dout == torch.bfloat16 else torch.int32)), (n, io, w)


def test_roundtrip_fitted_unaligned(gc, orc):
    """Buffers off 16-byte alignment: the generic kernel throughout, under the device word."""
    import roundtrip_inputs as RI
    a = RI.inputs(TILE + 9, False)
    x = _dev(np.concatenate([a[:1], a]))[1:]
    p = gc.expert(1, 16658, 64, -20)
    want = gc.roundtrip(x, p)
    got = gc.roundtrip_fitted(x, _word(-20), 64)
    base = torch.zeros(x.numel() + 1, device="cuda")
    base[1:] = x
    gc.roundtrip_fitted(base[1:], _word(-20), 64, out=base[1:])
    torch.cuda.synchronize()
    assert torch.equal(got.view(torch.int32), want.view(torch.int32))
    assert torch.equal(base[1:].view(torch.int32), want.view(torch.int32))


def test_roundtrip_fitted_bits_per_value(gc, orc):
    """The one-shot form: table, fit and round trip launched from a number of bits per value."""
    import rate_table_inputs as RT
    x_np, _ = RT.crafted_table(BIG, False, 64)
    x = _dev(x_np)
    for bpv in (2, 8):
        p = gc.fit_accuracy(x, bpv)
        bits = torch.zeros(1, dtype=torch.int64, device="cuda")
        got = gc.roundtrip_fitted(x, bpv, bits=bits)
        want = gc.roundtrip(x, p)
        torch.cuda.synchronize()
        assert torch.equal(got.view(torch.int32), want.view(torch.int32))
        assert int(bits.item()) <= bpv * BIG


# ------------------------------------------------------------------------------------------------ end to end
@pytest.mark.parametrize("bpv", [2, 4, 8, 16])
def test_fitted_encoder_matches_encode_fitted(gc, orc, bpv):
    import rate_table_inputs as RT
    x_np, _ = RT.crafted_table(BIG, False, 64)
    x = _dev(x_np)
    fe = gc.FittedEncoder(BIG, torch.float32, bpv, index_stride=8)
    got = fe(x)
    ref, p = gc.encode_fitted(x, bpv, index_stride=8)
    torch.cuda.synchronize()
    assert got.params is None
    _same_stream(got, ref, bpv)
    assert got.to_bytes() == ref.to_bytes()
    assert fe.params() == p == gc.fit_accuracy(x, bpv)
    assert got.bits <= bpv * BIG and gc.read_fit(fe.fit) == (p.minexp, 0, got.bits)
    d = gc.decode(got, params=fe.params())
    torch.cuda.synchronize()
    assert torch.equal(d.view(torch.int32), gc.decode(ref).view(torch.int32))


def test_fitted_encoder_coarsest(gc):
    x = torch.ones(64, device="cuda")
    fe = gc.FittedEncoder(64, torch.float32, 0.2)  # below one bit per block
    got = fe(x)
    torch.cuda.synchronize()
    assert gc.read_fit(fe.fit) == (133, 1, 16) and got.bits == 16
    with pytest.raises(gc.GcowError):
        fe.params()
    assert fe.params(allow_coarsest=True) == gc.fitted_params(64, 133)


def test_stream_capture(gc, orc):
    """What the feature is for: table, fit and encode captured once follow the data they are replayed on -- input B's
    scale differs, so does its fitted minexp, and the replay codes B under B's own fit."""
    import rate_table_inputs as RT
    import roundtrip_inputs as RI
    O = orc
    bpv = 6
    a, table_a = RT.crafted_table(BIG, False, 64)
    with np.errstate(over="ignore"):  # 3e38 * 1024: Inf members, which the coder has a rule for
        b = RI.inputs(BIG, False, seed=1234) * np.float32(1024.0)
    table_b = RT.oracle_table(b, 64)
    fit_a, fit_b = RT.fit(table_a, bpv * BIG), RT.fit(table_b, bpv * BIG)
    assert fit_a[0] != fit_b[0]

    def check(x_np, fit):
        op = O.expert(1, 16658, 64, fit[0])
        w_ref, bits_ref = O.compress(x_np, op)
        assert bits_ref == fit[1]
        assert gc.read_fit(fe.fit) == (fit[0], 0, fit[1])
        assert enc.bits == bits_ref and enc.to_bytes() == w_ref.tobytes()

    fe = gc.FittedEncoder(BIG, torch.float32, bpv)
    x = _dev(a)
    enc = fe(x)  # the kernels are loaded before the capture
    torch.cuda.synchronize()
    check(a, fit_a)
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        enc = fe(x)
    x.copy_(torch.from_numpy(b))
    g.replay()
    torch.cuda.synchronize()
    check(b, fit_b)
    x.copy_(torch.from_numpy(np.array(a)))
    g.replay()
    torch.cuda.synchronize()
    check(a, fit_a)


# ------------------------------------------------------------------------------------------------ argument checks
def test_argument_checks(gc):
    from gcow_amd import _ffi
    L = gc.load()
    x = torch.zeros(64, dtype=torch.float32, device="cuda")
    hp = gc.fitted_params(64, 0)
    f0 = gc.field_of(x)
    cap = L.gcow_max_output_bytes(C.byref(f0), C.byref(hp))
    wsb = L.gcow_encode_workspace_bytes(C.byref(f0), C.byref(hp))
    words = torch.full((cap // 8,), SENT, dtype=torch.int64, device="cuda")
    ws = torch.full((wsb // 8 + 1,), SENT, dtype=torch.int64, device="cuda")
    bits = torch.full((1,), SENT, dtype=torch.int64, device="cuda")
    out = torch.full((64,), 7.0, device="cuda")
    word = torch.tensor([-20, 0], dtype=torch.int32, device="cuda")
    byte_off = word.data_ptr() + 2

    def field(**kw):
        f = gc.field_of(x)
        for k, v in kw.items():
            setattr(f, k, v)
        return f

    INVALID, CAPACITY, UNSUPPORTED = 1, 2, 5
    cases = [(field(nx=8, ny=8), word.data_ptr(), cap, wsb, UNSUPPORTED),                  # 2-D
             (field(nx=32, sx=2), word.data_ptr(), cap, wsb, UNSUPPORTED),                 # a strided view
             (field(dtype=_ffi.DTYPE_INT32), word.data_ptr(), cap, wsb, UNSUPPORTED),      # an int32 tensor
             (field(), None, cap, wsb, INVALID),                                           # NULL d_minexp
             (field(), byte_off, cap, wsb, INVALID),                                       # misaligned d_minexp
             (field(), word.data_ptr(), cap - 8, wsb, CAPACITY),                           # short capacity
             (field(), word.data_ptr(), cap, wsb - 8, INVALID)]                            # short workspace
    for f, wp, c, wb, want in cases:
        assert _raw_encode(gc, f, 64, wp, words, c, bits, ws, wb, None, 0) == want, L.gcow_last_error()
    for f, wp, _, _, want in cases[:5]:
        st = L.gcow_roundtrip_fitted_device(C.byref(f), 64, wp, out.data_ptr(), _ffi.DTYPE_FLOAT, bits.data_ptr(),
                                            _stream())
        assert st == want, L.gcow_last_error()
    assert L.gcow_roundtrip_fitted_device(C.byref(f0), 64, word.data_ptr(), out.data_ptr(), _ffi.DTYPE_INT32,
                                          None, _stream()) == UNSUPPORTED
    table = torch.zeros(288, dtype=torch.int64, device="cuda")
    rec = torch.full((2,), SENT, dtype=torch.int64, device="cuda")
    for tp, rp in [(None, rec.data_ptr()), (table.data_ptr(), None), (table.data_ptr() + 4, rec.data_ptr()),
                   (table.data_ptr(), rec.data_ptr() + 4)]:
        assert L.gcow_rate_table_fit_device(tp, 100, rp, _stream()) == INVALID
    torch.cuda.synchronize()
    for t in (words, ws, bits, rec):
        assert bool((t == SENT).all())
    assert bool((out == 7.0).all()) and word.tolist() == [-20, 0]
    with pytest.raises(gc.GcowError):
        gc.encode_fitted_device(torch.zeros(8, 8, device="cuda"), word)
    with pytest.raises(gc.GcowError):
        gc.encode_fitted_device(torch.zeros(64, device="cuda")[::2], word)
    with pytest.raises(gc.GcowError):
        gc.encode_fitted_device(torch.zeros(64, dtype=torch.int32, device="cuda"), word)
    with pytest.raises(gc.GcowError):
        gc.encode_fitted_device(x, torch.zeros(1, dtype=torch.int32))  # a host word
    with pytest.raises(gc.GcowError):
        gc.fit_device(torch.zeros(288, dtype=torch.int64), 100)  # a host table
    with pytest.raises(gc.GcowError):
        gc.roundtrip_fitted(x, torch.zeros(1, dtype=torch.float32, device="cuda"))


# ---------------------------------------------------------------------------------------------- hooks, RCCL world 1
@pytest.fixture
def nccl_world1():
    import torch.distributed as dist
    dist.init_process_group("nccl", store=dist.HashStore(), rank=0, world_size=1, device_id=torch.device("cuda", 0))
    yield
    dist.destroy_process_group()


class _Bucket:
    def __init__(self, t, i):
        self.t, self.i = t, i

    def buffer(self):
        return self.t

    def index(self):
        return self.i


def test_roundtrip_hook_fit_on_device_world1(gc, orc, nccl_world1):
    import roundtrip_inputs as RI
    from gcow_amd import ddp
    x = _dev(RI.inputs(BIG, False))
    state = ddp.make_hook_state(hook=ddp.roundtrip_hook, params=gc.accuracy(1e-3), target_bits=4, fit_on_device=True)
    t = x.clone()
    ddp.roundtrip_hook(state, _Bucket(t, 0)).wait()
    torch.cuda.synchronize()
    p = gc.fit_accuracy(x, 4)
    want = gc.roundtrip(x, p)
    torch.cuda.synchronize()
    assert np.array_equal(t.cpu().numpy().view(np.uint32), want.cpu().numpy().view(np.uint32))
    assert not state._fits and gc.read_fit(state.fit_record(0))[:2] == (p.minexp, 0)


def test_allgather_hook_fit_on_device_world1(gc, orc, nccl_world1):
    import roundtrip_inputs as RI
    from gcow_amd import ddp
    x = _dev(RI.inputs(BIG, False))
    p0 = gc.accuracy(1e-6)
    state = ddp.make_hook_state(hook=ddp.compressed_allgather_hook, params=p0, target_bits=4, fit_on_device=True)
    p = gc.fit_accuracy(x, 4)
    assert p != p0
    for _ in range(2):  # the first step is fitted like every other
        t = x.clone()
        ddp.compressed_allgather_hook(state, _Bucket(t, 0)).wait()
        torch.cuda.synchronize()
        # the mean of one stream is 0 + decode, so a -0 of the decode arrives as +0
        want = gc.roundtrip(x, p) + 0.0
        assert np.array_equal(t.cpu().numpy().view(np.uint32), want.cpu().numpy().view(np.uint32))
        me, status, bits = gc.read_fit(state.fit_record(0))
        assert (me, status) == (p.minexp, 0) and bits == gc.encode(x, p).bits <= 4 * BIG
    assert not state._fits


def test_hook_value_errors(gc):
    from gcow_amd import ddp
    acc = gc.accuracy(1e-3)
    b = _Bucket(torch.zeros(64, device="cuda"), 0)
    S = ddp.GcowHookState
    with pytest.raises(ValueError, match="compressed_sharded_hook"):
        ddp.compressed_sharded_hook(S(params=acc, target_bits=4.0, fit_on_device=True, sharded=True), b)
    with pytest.raises(ValueError, match="error_feedback"):
        ddp.compressed_allgather_hook(S(params=acc, target_bits=4.0, fit_on_device=True, error_feedback=True), b)
    with pytest.raises(ValueError, match="compress_mean"):
        ddp.compressed_sharded_hook(S(params=acc, target_bits=4.0, fit_on_device=True, sharded=True,
                                      compress_mean=True), b)
    with pytest.raises(ValueError, match="target_bits"):
        ddp.roundtrip_hook(S(params=acc, fit_on_device=True), b)
