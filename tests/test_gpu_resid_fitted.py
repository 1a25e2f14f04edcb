"""GPU checks of error feedback under a bit budget (include/gcow.h: gcow_rate_table_residual_device,
gcow_encode_residual_fitted_device; codec.FittedResidualEncoder), bit for bit:

  - the rate table of y = x + e against codec.rate_table of y made by torch, against the bits codec.encode_residual
    reports at a handful of entries, against the oracle's table on the small sizes, err = None against the table of x,
    rows off 16-byte alignment, and more than 1024 tiles (the grid-stride loop's second iteration); a sentinel follows
    every table;
  - the fitted residual encode against codec.encode_residual under the clamped set: stream, bits, index and the whole
    e_out, out of place (sentinels past e_out[n - 1] and past the stream), in place and with e_in = NULL; fp32 and bf16,
    maxprec 64 / 20 / 0, strides 0 / 8 / 16, in-range and out-of-range device words; dirty buffers; oversized tiles;
    the numpy model on small sizes;
  - FittedResidualEncoder against host table -> fit_minexp -> encode_residual; one captured graph of table + fit +
    encode replayed on other x and e;
  - argument checks; compressed_allgather_hook with fit_on_device and error_feedback over a one-rank RCCL group.

Sizes follow the tile encoder's geometry: a tile is 4096 values, a count workgroup covers 8 tiles (32768 values). x is
the crafted bucket of tests/roundtrip_inputs.py (zero, subnormal, NaN, +-Inf, 3e38 blocks); e is random at x's
magnitude, and 3e38 where x is, so that x + e overflows."""
import ctypes as C
import functools
import os
import sys

import numpy as np
import pytest

torch = pytest.importorskip("torch")

TESTS = os.path.dirname(os.path.abspath(__file__))
if TESTS not in sys.path:
    sys.path.insert(0, TESTS)

import fit_device_inputs as FI  # noqa: E402
from test_gpu_fit_device import MAXPRECS, SENT, SIZES, STRIDES, TILE, WORDS, _all_exponents  # noqa: E402

pytestmark = pytest.mark.gpu

BIG = 3 * TILE + 7
MANY_TILES = (1024 + 3) * TILE + 5  # the table's grid is at most 1024 workgroups of one tile per iteration
SENT_F = 1234.5
INVALID, CAPACITY, UNSUPPORTED = 1, 2, 5


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


def _i32(t):
    return t.view(torch.int32)


@functools.lru_cache(maxsize=None)
def _inputs(n, bf16, seed=901):
    """(x, e): computed once per case, read-only."""
    import roundtrip_inputs as RI
    from oracle import oracle as O
    x = RI.inputs(n, bf16, seed)
    xf = RI.widen(x)
    e = O.gen_normal(n, 1e-3, seed + 76, True).copy()
    with np.errstate(invalid="ignore"):
        huge = np.isfinite(xf) & (np.abs(xf) > 1e38)
    e[huge] = np.copysign(np.float32(3e38), xf[huge])
    x.setflags(write=False)
    e.setflags(write=False)
    return x, e


def test_inputs_have_the_crafted_cases():
    import roundtrip_inputs as RI
    x, e = _inputs(4097, False)
    xf = RI.widen(x)
    with np.errstate(over="ignore", invalid="ignore"):
        y = xf + e
    assert np.isnan(xf).any() and np.isinf(xf).any()
    assert (np.isinf(y) & np.isfinite(xf)).any()  # x + e overflows


# ------------------------------------------------------------------------------------------------ the table
def _raw_table(gc, x, e, maxprec):
    """gcow_rate_table_residual_device through the C ABI into a sentinel-filled table with 4 sentinel words behind."""
    L = gc.load()
    f = gc.field_of(x)
    wsb = L.gcow_rate_table_workspace_bytes(C.byref(f))
    ws = torch.full((wsb // 8 + 2,), SENT, dtype=torch.int64, device="cuda")
    table = torch.full((288 + 4,), SENT, dtype=torch.int64, device="cuda")
    st = L.gcow_rate_table_residual_device(C.byref(f), e.data_ptr() if e is not None else None, maxprec,
                                           table.data_ptr(), ws.data_ptr(), wsb, _stream())
    assert st == 0, L.gcow_last_error()
    torch.cuda.synchronize()
    assert bool((table[288:] == SENT).all()) and bool((ws[wsb // 8:] == SENT).all())
    return table[:288]


@pytest.mark.parametrize("bf16", [False, True], ids=["fp32", "bf16"])
@pytest.mark.parametrize("n", SIZES)
def test_table_of_y(gc, orc, n, bf16):
    x_np, e_np = _inputs(n, bf16)
    x, e = _dev(x_np), _dev(e_np)
    y = x.float() + e
    keep_x, keep_e = x.clone(), e.clone()
    for maxprec in MAXPRECS:
        got = _raw_table(gc, x, e, maxprec)
        assert torch.equal(got, gc.rate_table(y, maxprec)), (n, bf16, maxprec)
        assert torch.equal(gc.rate_table_residual(x, e, maxprec), got)
        assert torch.equal(_raw_table(gc, x, None, maxprec), gc.rate_table(x, maxprec)), (n, bf16, maxprec)
        assert torch.equal(gc.rate_table_residual(x, None, maxprec), gc.rate_table(x, maxprec))
        h = got.cpu().tolist()
        for t in (0, 100, 134, 140, 150, 287):  # the encoder's own bit count, on the array it encodes
            enc = gc.encode_residual(x, e.clone(), gc.expert(1, 16658, maxprec, FI.MINEXP_LO + t))
            torch.cuda.synchronize()
            assert enc.bits == h[t], (n, bf16, maxprec, t)
    assert torch.equal(_i32(keep_e), _i32(e)) and torch.equal(keep_x.view(torch.uint8), x.view(torch.uint8))


@pytest.mark.parametrize("bf16", [False, True], ids=["fp32", "bf16"])
@pytest.mark.parametrize("n", [1, 3, 5, 4097])
def test_table_matches_oracle(gc, orc, n, bf16):
    import rate_table_inputs as RT
    import roundtrip_inputs as RI
    x_np, e_np = _inputs(n, bf16)
    with np.errstate(over="ignore", invalid="ignore"):
        y_np = (RI.widen(x_np) + e_np).astype(np.float32)
    for maxprec in (64, 20):
        got = _raw_table(gc, _dev(x_np), _dev(e_np), maxprec)
        assert np.array_equal(got.cpu().numpy(), RT.oracle_table(y_np, maxprec)), (n, bf16, maxprec)


@pytest.mark.parametrize("off_x,off_e", [(1, 0), (0, 1), (1, 1), (2, 3)])
@pytest.mark.parametrize("bf16", [False, True], ids=["fp32", "bf16"])
def test_table_unaligned_rows(gc, orc, bf16, off_x, off_e):
    """Either row off 16-byte alignment: the element path for every tile, the partial last block padded from y."""
    n = 2 * TILE + 9
    x_np, e_np = _inputs(n, bf16)
    x = _dev(np.concatenate([x_np[:off_x], x_np]))[off_x:]
    e = _dev(np.concatenate([e_np[:off_e], e_np]))[off_e:]
    assert x.data_ptr() % 16 != 0 or e.data_ptr() % 16 != 0
    y = x.float() + e
    for maxprec in (64, 20):
        assert torch.equal(_raw_table(gc, x, e, maxprec), gc.rate_table(y, maxprec)), (bf16, off_x, off_e, maxprec)


@pytest.mark.parametrize("bf16", [False, True], ids=["fp32", "bf16"])
def test_table_more_tiles_than_workgroups(gc, bf16):
    """More than 1024 tiles: the two-row prefetch of the grid-stride loop runs a second iteration."""
    g = torch.Generator(device="cuda").manual_seed(5)
    x = torch.randn(MANY_TILES, device="cuda", generator=g) * 1e-3
    e = torch.randn(MANY_TILES, device="cuda", generator=g) * 1e-3
    if bf16:
        x = x.to(torch.bfloat16)
    y = x.float() + e
    got = _raw_table(gc, x, e, 64)
    assert torch.equal(got, gc.rate_table(y, 64))
    assert not torch.equal(got, gc.rate_table(x, 64))


# ------------------------------------------------------------------------------------------------ the fitted encode
def _raw_encode(gc, x, e_in, e_out, word, maxprec, stride, fill=SENT, cap=None, wsb=None):
    """gcow_encode_residual_fitted_device through the C ABI into filled buffers: the capacity and the workspace are
    exactly the queries of the fp32 field of n values, with 4 / 8 filled words behind them, the index with 2.
    -> (status, words, bits, index or None). The words behind each buffer are checked here."""
    L = gc.load()
    n = x.numel()
    hp = gc.fitted_params(maxprec, 0)
    yf = gc.field_of_shape((n,), torch.float32)
    cap_q = L.gcow_max_output_bytes(C.byref(yf), C.byref(hp))
    wsb_q = L.gcow_encode_workspace_bytes(C.byref(yf), C.byref(hp))
    words = torch.full((cap_q // 8 + 4,), fill, dtype=torch.int64, device="cuda")
    ws = torch.full((wsb_q // 8 + 8,), fill, dtype=torch.int64, device="cuda")
    bits = torch.full((1,), fill, dtype=torch.int64, device="cuda")
    ne = L.gcow_index_entries(C.byref(yf), stride) if stride else 0
    index = torch.full((ne + 2,), fill, dtype=torch.int64, device="cuda") if stride else None
    f = gc.field_of(x)
    st = L.gcow_encode_residual_fitted_device(C.byref(f), maxprec, word.data_ptr(),
                                              e_in.data_ptr() if e_in is not None else None, e_out.data_ptr(),
                                              words.data_ptr(), cap_q if cap is None else cap, bits.data_ptr(),
                                              ws.data_ptr(), wsb_q if wsb is None else wsb,
                                              index.data_ptr() if index is not None else None, stride, _stream())
    torch.cuda.synchronize()
    assert bool((words[cap_q // 8:] == fill).all()), "the words after the capacity were written"
    assert bool((ws[wsb_q // 8:] == fill).all()), "the words after the workspace were written"
    if index is not None:
        assert bool((index[ne:] == fill).all())
        index = index[:ne]
    return st, words, int(bits.item()), index


def _ebuf(n, init):
    """An error buffer of n floats inside a 16-byte aligned allocation with 16 sentinel floats on either side."""
    buf = torch.full((16 + n + 16,), SENT_F, dtype=torch.float32, device="cuda")
    if init is not None:
        buf[16:16 + n] = init
    return buf, buf[16:16 + n]


def _intact(buf, n):
    return bool((buf[:16] == SENT_F).all() and (buf[16 + n:] == SENT_F).all())


def _same(got, ref, e_got, e_ref, what):
    """(status, words, bits, index) of _raw_encode against an Encoded of codec.encode_residual, and the errors."""
    st, words, bits, index = got
    assert st == 0, what
    assert bits == ref.bits, what
    nw = (bits + 63) // 64
    assert torch.equal(words[:nw], ref.words[:nw]), what
    assert (index is None) == (ref.index is None), what
    if index is not None:
        assert torch.equal(index, ref.index[:index.numel()]), what
    assert torch.equal(_i32(e_got), _i32(e_ref)), what


@pytest.mark.parametrize("has_e", [True, False], ids=["e", "null"])
@pytest.mark.parametrize("bf16", [False, True], ids=["fp32", "bf16"])
@pytest.mark.parametrize("n", SIZES)
def test_encode_matches_host_params(gc, orc, n, bf16, has_e):
    x_np, e_np = _inputs(n, bf16)
    x = _dev(x_np)
    e0 = _dev(e_np) if has_e else torch.zeros(n, device="cuda")
    ref = {}
    k = 0
    for maxprec in MAXPRECS:
        for w in WORDS:
            stride = STRIDES[k % len(STRIDES)]  # every stride meets every maxprec and most words
            k += 1
            m = FI.clamp(w)
            key = (maxprec, stride, m)
            if key not in ref:
                e_ref = e0.clone()
                ref[key] = (gc.encode_residual(x, e_ref, gc.expert(1, 16658, maxprec, m), stride), e_ref)
                torch.cuda.synchronize()
            what = (n, bf16, has_e, maxprec, stride, w)
            word = _word(w)
            # out of place: e_in only read, sentinels around e_out
            buf_in, e_in = _ebuf(n, e0) if has_e else (None, None)
            buf_out, e_out = _ebuf(n, None)
            got = _raw_encode(gc, x, e_in, e_out, word, maxprec, stride)
            _same(got, ref[key][0], e_out, ref[key][1], what)
            assert _intact(buf_out, n), what
            if has_e:
                assert torch.equal(_i32(e_in), _i32(e0)) and _intact(buf_in, n), what
                # in place: the same result
                buf2, e2 = _ebuf(n, e0)
                got = _raw_encode(gc, x, e2, e2, word, maxprec, stride)
                _same(got, ref[key][0], e2, ref[key][1], what)
                assert _intact(buf2, n), what
            assert int(word.item()) == w  # d_minexp is read, never written


@pytest.mark.parametrize("bf16", [False, True], ids=["fp32", "bf16"])
def test_codec_entry_point(gc, orc, bf16):
    """codec.encode_residual_fitted_device: err updated in place, the word a gcow_fit record."""
    n = 8197
    x_np, e_np = _inputs(n, bf16)
    x, e, e_ref = _dev(x_np), _dev(e_np), _dev(e_np)
    rec = gc.fit_device(gc.rate_table_residual(x, e), 6 * n)
    me, status, bits = gc.read_fit(rec)
    assert status == 0 and bits <= 6 * n
    enc = gc.encode_residual_fitted_device(x, e, rec, index_stride=16)
    ref = gc.encode_residual(x, e_ref, gc.fitted_params(64, me), 16)
    torch.cuda.synchronize()
    assert enc.params is None and enc.bits == ref.bits == bits and enc.to_bytes() == ref.to_bytes()
    ne = ((n + 3) // 4 + 15) // 16
    assert torch.equal(enc.index[:ne], ref.index[:ne]) and torch.equal(_i32(e), _i32(e_ref))


@pytest.mark.parametrize("bf16", [False, True], ids=["fp32", "bf16"])
@pytest.mark.parametrize("n", [1, 3, 5, 4095, 4097])
def test_encode_matches_model(gc, orc, n, bf16):
    from residual_model import model_step
    O = orc
    x_np, e_np = _inputs(n, bf16)
    x = _dev(x_np)
    for w in (-155, -20, 100):
        op = O.expert(1, 16658, 64, FI.clamp(w))
        for e_init in (e_np, None):
            _, w_ref, bits_ref, _, r_ref = model_step(x_np, None if e_init is None else np.array(e_init), op)
            buf, e_out = _ebuf(n, None)
            st, words, bits, _ = _raw_encode(gc, x, None if e_init is None else _dev(e_init), e_out, _word(w), 64, 8)
            assert st == 0 and bits == bits_ref, (n, bf16, w)
            assert words[:w_ref.size].cpu().numpy().view(np.uint64).tobytes() == w_ref.tobytes(), (n, bf16, w)
            assert np.array_equal(e_out.cpu().numpy().view(np.uint32), r_ref.view(np.uint32)), (n, bf16, w)
            assert _intact(buf, n)


@pytest.mark.parametrize("n", [5, 8197, 32768 + 5])
def test_encode_dirty_buffers(gc, orc, n):
    """All-ones and patterned stream, index, workspace, bit count and e_out; a second input with a shorter stream into
    the same kind of buffers; the minexp record stays as it was."""
    x1_np, e_np = _inputs(n, False)
    x2_np, _ = _inputs(n, False, 77)
    x1, x2 = _dev(x1_np), _dev(x2_np) * (2.0 ** -8)
    e0 = _dev(e_np)
    for fill in (-1, SENT):
        rec = torch.tensor([-20, 0x5A5A5A5A, 7, 7], dtype=torch.int32, device="cuda")
        for x in (x1, x2):
            e_ref = e0.clone()
            ref = gc.encode_residual(x, e_ref, gc.expert(1, 16658, 64, -20), 8)
            e_out = torch.full((n,), float("nan"), device="cuda")
            got = _raw_encode(gc, x, e0, e_out, rec, 64, 8, fill=fill)
            _same(got, ref, e_out, e_ref, (n, fill))
            assert rec.tolist() == [-20, 0x5A5A5A5A, 7, 7]


def test_encode_oversized_tiles(gc, orc):
    """Tiles whose code exceeds the small LDS window are listed by the main kernel and coded by the _big one. Two
    inputs: the 65559-value bucket of residual_var_inputs (every odd tile times 2^20, scale_odd_tiles) at accuracy
    1e-3 = minexp -10, where only those tiles are oversized and both kernels code tiles in one call; and a bucket of
    all exponents at full precision, where every whole tile is."""
    from residual_model import model_step
    from residual_var_inputs import case
    O = orc
    window = 1500 * 64 - 128  # the small window, less what the tile's start may take
    c = case(65559, False, "acc1e-3")
    assert c["op"].tuple() == (1, 16658, 64, -10)
    mixed = (np.array(c["xs"][0]), np.array(c["e0"]), -10)
    allexp = (_all_exponents(BIG), (_all_exponents(BIG)[::-1] * np.float32(2.0 ** -12)).astype(np.float32), -154)
    for name, (x_np, e_np, me) in (("mixed", mixed), ("all", allexp)):
        n = x_np.size
        op = O.expert(1, 16658, 64, me)
        y, w_ref, bits_ref, _, r_ref = model_step(x_np, e_np, op)
        lens = O.block_bits(y, op).astype(np.int64)
        tiles = [int(lens[t:t + TILE // 4].sum()) for t in range(0, lens.size, TILE // 4)]
        assert tiles[1] > 96 * (TILE // 4), (name, tiles)  # above the window wherever the tile starts
        assert name != "mixed" or max(tiles[0], tiles[2]) < window, (name, tiles)
        x, e0 = _dev(x_np), _dev(e_np)
        for stride in (0, 8):
            e_ref = e0.clone()
            ref = gc.encode_residual(x, e_ref, gc.expert(1, 16658, 64, me), stride)
            buf, e_out = _ebuf(n, None)
            got = _raw_encode(gc, x, e0, e_out, _word(me), 64, stride)
            _same(got, ref, e_out, e_ref, (name, stride))
            assert _intact(buf, n)
            e2 = e0.clone()
            got = _raw_encode(gc, x, e2, e2, _word(me if name == "mixed" else -2 ** 31), 64, stride)  # in place
            _same(got, ref, e2, e_ref, (name, stride))
        assert got[2] == bits_ref
        assert got[1][:w_ref.size].cpu().numpy().view(np.uint64).tobytes() == w_ref.tobytes()
        assert np.array_equal(e2.cpu().numpy().view(np.uint32), r_ref.view(np.uint32))


# ------------------------------------------------------------------------------------------------ end to end
def _eager_step(gc, x, e, budget, maxprec=64, stride=8):
    """The form with host reads: the table of y, fit_minexp on the host, encode_residual (e updated in place)."""
    me, bits = gc.fit_minexp(gc.rate_table_residual(x, e, maxprec), budget)
    enc = gc.encode_residual(x, e, gc.fitted_params(maxprec, me), stride)
    torch.cuda.synchronize()
    assert enc.bits == bits <= budget
    return enc, me


@pytest.mark.parametrize("bf16", [False, True], ids=["fp32", "bf16"])
@pytest.mark.parametrize("bpv", [2, 4, 8, 16])
def test_fitted_residual_encoder_matches_host_fit(gc, orc, bpv, bf16):
    x_np, e_np = _inputs(BIG, bf16)
    x = _dev(x_np)
    e, e_ref = _dev(e_np), _dev(e_np)
    fe = gc.FittedResidualEncoder(BIG, x.dtype, bpv, index_stride=8)
    for step in range(2):  # the second step codes x + the first step's residual
        got = fe(x, e)
        ref, me = _eager_step(gc, x, e_ref, int(bpv * BIG))
        torch.cuda.synchronize()
        assert got.params is None
        assert got.bits == ref.bits <= bpv * BIG and got.to_bytes() == ref.to_bytes(), (bpv, step)
        ne = ((BIG + 3) // 4 + 7) // 8
        assert torch.equal(got.index[:ne], ref.index[:ne])
        assert torch.equal(_i32(e), _i32(e_ref)), (bpv, step)
        assert gc.read_fit(fe.fit) == (me, 0, got.bits) and fe.params() == gc.fitted_params(64, me)


def test_fitted_residual_encoder_coarsest(gc):
    x = torch.ones(64, device="cuda")
    e = torch.full((64,), 0.5, device="cuda")
    fe = gc.FittedResidualEncoder(64, torch.float32, 0.2)  # below one bit per block
    got = fe(x, e)
    torch.cuda.synchronize()
    assert gc.read_fit(fe.fit) == (133, 1, 16) and got.bits == 16
    assert bool((e == 1.5).all())  # nothing was sent: the whole of y is carried
    with pytest.raises(gc.GcowError):
        fe.params()
    assert fe.params(allow_coarsest=True) == gc.fitted_params(64, 133)


def test_stream_capture(gc, orc):
    """Table of y, fit and residual encode captured once on one stream; three replays on other x and e follow their
    data, and e evolves as in the eager sequence."""
    bpv = 6
    budget = bpv * BIG
    xs = [_inputs(BIG, False, s)[0] for s in (901, 1234, 77)]
    scales = [1.0, 1024.0, 2.0 ** -6]  # other scales, so other fitted sets
    e_start = _inputs(BIG, False, 1234)[1]
    fe = gc.FittedResidualEncoder(BIG, torch.float32, bpv, index_stride=8)
    x = _dev(xs[0])
    e = torch.zeros(BIG, device="cuda")
    fe(x, e)  # the kernels are loaded before the capture
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        enc = fe(x, e)
    e.copy_(_dev(e_start))
    e_ref = _dev(e_start)
    fits = []
    for k in range(3):
        xk = _dev(xs[k]) * scales[k]
        x.copy_(xk)
        g.replay()
        torch.cuda.synchronize()
        ref, me = _eager_step(gc, xk, e_ref, budget)
        assert gc.read_fit(fe.fit) == (me, 0, ref.bits), k
        assert enc.bits == ref.bits and enc.to_bytes() == ref.to_bytes(), k
        assert torch.equal(_i32(e), _i32(e_ref)), k
        fits.append(me)
    assert len(set(fits)) > 1  # the replays did not all code under one set


# ------------------------------------------------------------------------------------------------ argument checks
def test_argument_checks(gc):
    L = gc.load()
    n = 64
    x = torch.zeros(n + 4, device="cuda")
    word = torch.tensor([-20, 0], dtype=torch.int32, device="cuda")
    buf_in, e_in = _ebuf(n + 4, torch.ones(n + 4, device="cuda"))
    buf_out, e_out = _ebuf(n + 4, None)

    def untouched():
        return bool((e_in == 1.0).all() and (e_out == SENT_F).all() and _intact(buf_in, n + 4)
                    and _intact(buf_out, n + 4) and (x == 0).all())

    def call(xv=x[:n], ei=e_in[:n], eo=e_out[:n], wd=word, **kw):
        st, words, bits, _ = _raw_encode(gc, xv, ei, eo, wd, 64, 0, **kw)
        assert bool((words == SENT).all()) and bits == SENT and untouched(), L.gcow_last_error()
        return st

    # off 16-byte alignment: no composed fallback
    assert call(xv=x[1:n + 1]) == UNSUPPORTED
    assert call(ei=e_in[1:n + 1]) == UNSUPPORTED
    assert call(eo=e_out[2:n + 2]) == UNSUPPORTED
    xb = torch.zeros(n + 8, dtype=torch.bfloat16, device="cuda")
    assert call(xv=xb[4:n + 4]) == UNSUPPORTED  # 8 bytes in
    with pytest.raises(gc.GcowError):
        gc.encode_residual_fitted_device(x[1:n + 1], e_out[:n], word)
    # the word
    assert call(wd=word.view(torch.int16)[1:]) == INVALID  # 2 bytes in
    # short capacity, short workspace
    hp = gc.fitted_params(64, 0)
    yf = gc.field_of_shape((n,), torch.float32)
    cap = L.gcow_max_output_bytes(C.byref(yf), C.byref(hp))
    wsb = L.gcow_encode_workspace_bytes(C.byref(yf), C.byref(hp))
    assert call(cap=cap - 8) == CAPACITY
    assert call(wsb=wsb - 8) == INVALID
    # NULL d_err_out, NULL d_minexp
    f = gc.field_of(x[:n])
    words = torch.full((cap // 8,), SENT, dtype=torch.int64, device="cuda")
    ws = torch.full((wsb // 8 + 1,), SENT, dtype=torch.int64, device="cuda")
    bits = torch.full((1,), SENT, dtype=torch.int64, device="cuda")
    args = (words.data_ptr(), cap, bits.data_ptr(), ws.data_ptr(), wsb, None, 0, _stream())
    assert L.gcow_encode_residual_fitted_device(C.byref(f), 64, word.data_ptr(), e_in.data_ptr(), None, *args) == INVALID
    assert L.gcow_encode_residual_fitted_device(C.byref(f), 64, None, e_in.data_ptr(), e_out.data_ptr(),
                                                *args) == INVALID
    torch.cuda.synchronize()
    assert bool((words == SENT).all()) and bool((ws == SENT).all()) and int(bits.item()) == SENT
    # nx = 0 writes a zero bit count and nothing else
    f0 = gc.field_of_shape((0,), torch.float32)
    assert L.gcow_encode_residual_fitted_device(C.byref(f0), 64, word.data_ptr(), e_in.data_ptr(), e_out.data_ptr(),
                                                *args) == 0
    torch.cuda.synchronize()
    assert int(bits.item()) == 0 and bool((words == SENT).all()) and untouched()
    # the table: e off 4 bytes is refused, the sentinel-filled table untouched
    table = torch.full((288,), SENT, dtype=torch.int64, device="cuda")
    tws = torch.zeros(L.gcow_rate_table_workspace_bytes(C.byref(f)) // 8, dtype=torch.int64, device="cuda")
    assert L.gcow_rate_table_residual_device(C.byref(f), e_in.data_ptr() + 2, 64, table.data_ptr(), tws.data_ptr(),
                                             tws.numel() * 8, _stream()) == INVALID
    torch.cuda.synchronize()
    assert bool((table == SENT).all()) and word.tolist() == [-20, 0]
    with pytest.raises(gc.GcowError):
        gc.rate_table_residual(x[:n], torch.zeros(n, device="cuda", dtype=torch.float64))
    with pytest.raises(gc.GcowError):
        gc.rate_table_residual(x[:n], torch.zeros(n + 1, device="cuda"))


# ---------------------------------------------------------------------------------------------- the hook, RCCL world 1
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


@pytest.mark.parametrize("bf16", [False, True], ids=["fp32", "bf16"])
def test_allgather_hook_error_feedback_fit_on_device_world1(gc, orc, nccl_world1, bf16):
    from gcow_amd import ddp
    from oracle import oracle as O
    bpv = 4
    budget = bpv * BIG
    state = ddp.make_hook_state(hook=ddp.compressed_allgather_hook, params=gc.accuracy(1e-6), target_bits=bpv,
                                fit_on_device=True, error_feedback=True)
    e_ref = torch.zeros(BIG, device="cuda")
    fits = []
    for step in range(3):
        x = torch.from_numpy(O.gen_normal(BIG, 1e-3 * 8.0 ** step, 4100 + step, False).copy()).cuda()
        if bf16:
            x = x.to(torch.bfloat16)
        y = x.float() + e_ref  # what is encoded and sent
        ref, me = _eager_step(gc, x, e_ref, budget)
        p = gc.fitted_params(64, me)
        t = x.clone()
        ddp.compressed_allgather_hook(state, _Bucket(t, 0)).wait()
        torch.cuda.synchronize()
        rec = gc.read_fit(state.fit_record(0))
        assert rec == (me, 0, ref.bits) and rec[2] <= budget, (step, rec)
        # the mean of one stream is 0 + decode, so a -0 of the decode arrives as +0; a bf16 bucket gets it rounded
        want = (gc.roundtrip(y, p) + 0.0).to(t.dtype)
        assert torch.equal(t.view(torch.int16 if bf16 else torch.int32),
                           want.view(torch.int16 if bf16 else torch.int32)), step
        assert torch.equal(_i32(state.error_buffer(0, t)), _i32(e_ref)), step
        fits.append(me)
    assert not state._fits and bool((e_ref != 0).any()) and len(set(fits)) > 1
