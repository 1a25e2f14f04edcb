"""The segmented codec on the device (include/gcow.h "Segmented fields"; codec.SegmentedEncoder,
codec.decode_mean_segmented, codec.PerTensorFittedEncoder, DeviceCodec.encode_per_tensor / decode_mean_per_tensor,
compressed_allgather_hook with per_tensor_budget), bitwise against the per-tensor oracle (tests/segmented_inputs.py):

  1. the encode: every list x dtype x word set x index stride, packed words and gcow_fit records, output / workspace /
     index poisoned beforehand and the whole capacity compared; a bucket at an address off the row alignment; maxprec 12;
  2. the encode equals the device encode_append chain;
  3. the decode-mean: W = 1, 2, 3 with different data per stream, one word set for all streams and one per stream,
     odd and even stream_words, poisoned tails, strides 8 and 16, fp32 and bf16 output inside a guarded allocation at
     aligned and unaligned addresses, the all -154 streams (spans past the stage) included;
  4. PerTensorFittedEncoder: eager against the oracle's records and stream, and captured into a graph on one stream and
     replayed on new data;
  5. the hook at world 1 over RCCL, fp32 and bf16 buckets.
Every test fails on a library without the gcow_*_seg_* symbols."""
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

pytestmark = pytest.mark.gpu

POISON = 0x5A5A5A5A5A5A5A5A
POISON_I64 = np.uint64(POISON).astype(np.int64)
JUNK = 0x7777777700000000  # the upper half of a record's word 0 (status) and its word 1: never read
BF = [False, True]
BF_IDS = ["fp32", "bf16"]


@pytest.fixture(scope="module")
def gc():
    if not torch.cuda.is_available():
        pytest.fail("GPU tests need a device")
    from gcow_amd import codec
    return codec


def _upload(a: np.ndarray):
    t = torch.from_numpy(np.ascontiguousarray(a).copy())
    if a.dtype == np.uint16:
        return t.view(torch.int16).cuda().view(torch.bfloat16)
    return t.cuda()


def _bits_of(t):
    if t.dtype == torch.bfloat16:
        return t.view(torch.int16).cpu().numpy().view(np.uint16)
    return t.cpu().numpy().view(np.uint32)


def _u64(t):
    return t.cpu().numpy().view(np.uint64)


def _words_tensor(ws, records: bool):
    """The minexp words as int32[S], or as gcow_fit records int64[S, 2] with junk in everything but word 0's low half."""
    if not records:
        return torch.tensor(list(ws), dtype=torch.int32, device="cuda")
    a = np.zeros((len(ws), 2), np.uint64)
    for s, w in enumerate(ws):
        a[s, 0] = np.uint64((int(w) & 0xFFFFFFFF) | JUNK)
        a[s, 1] = np.uint64(POISON)
    return torch.from_numpy(a.view(np.int64)).cuda()


def _poison(enc):
    enc.words.fill_(int(POISON_I64))
    enc.ws.fill_(int(POISON_I64))
    enc.bits_dev.fill_(-1)
    if enc.index is not None:
        enc.index.fill_(int(POISON_I64))


def _check_encode(enc, e, want, stride):
    words, total, pos, _ = want
    torch.cuda.synchronize()
    assert e.bits == total
    got = _u64(enc.words)
    nw = (total + 63) // 64
    assert np.array_equal(got[:nw], words)
    assert (got[nw:] == np.uint64(POISON)).all()  # nothing past the flushed words, up to the whole capacity
    if stride:
        ix = SI.index_of(pos, stride)
        gi = _u64(enc.index)
        assert np.array_equal(gi[:ix.size], ix)
        assert (gi[ix.size:] == np.uint64(POISON)).all()


# ------------------------------------------------------------------------------------------------ 1. the encode
@pytest.mark.parametrize("bf16", BF, ids=BF_IDS)
@pytest.mark.parametrize("name", SI.LISTS)
def test_encode_every_word_set_and_stride(gc, orc, name, bf16):
    cnts = SI.counts(name)
    x = _upload(SI.bucket(name, bf16))
    plan = gc.SegmentPlan(cnts, x.dtype, "cuda")
    for stride in SI.STRIDES:
        enc = gc.SegmentedEncoder(cnts, x.dtype, 64, "cuda", stride, plan=plan)
        assert enc.words.numel() * 8 >= plan.max_output_bytes()
        for k, ws in enumerate(SI.WORD_SETS):
            _poison(enc)
            e = enc(x, _words_tensor(SI.words(name, bf16, ws), records=(k + stride // 8) % 2 == 1))
            _check_encode(enc, e, SI.stream(name, bf16, ws), stride)


@pytest.mark.parametrize("bf16", BF, ids=BF_IDS)
@pytest.mark.parametrize("name", ["edges", "special"])
def test_encode_off_the_row_alignment_and_maxprec_12(gc, orc, name, bf16):
    """The bucket one element into an allocation (fp32: rows 4 bytes off 16; bf16: rows at odd element offsets, 2
    bytes off 4), and a second maxprec."""
    cnts = SI.counts(name)
    a = SI.bucket(name, bf16)
    big = _upload(np.concatenate([a[:1], a, a[:3]]))
    x = big[1:1 + a.size]
    assert x.data_ptr() % (4 if bf16 else 16) != 0
    ws = SI.words(name, bf16, "alt")
    for maxprec in (64, 12):
        enc = gc.SegmentedEncoder(cnts, x.dtype, maxprec, "cuda", 16)
        _poison(enc)
        e = enc(x, _words_tensor(ws, records=maxprec == 12))
        _check_encode(enc, e, SI.stream(name, bf16, ws, maxprec), 16)
    assert np.array_equal(_bits_of(big[1:1 + a.size]), a.view(np.uint16 if bf16 else np.uint32))  # only read


def test_encode_empty_lists(gc):
    for cnts in ([], [0, 0]):
        x = torch.zeros(0, device="cuda")
        enc = gc.SegmentedEncoder(cnts, torch.float32, 64, "cuda", 16)
        _poison(enc)
        e = enc(x, torch.zeros(len(cnts), dtype=torch.int32, device="cuda"))
        torch.cuda.synchronize()
        assert e.bits == 0 and (_u64(enc.words) == np.uint64(POISON)).all()
    with pytest.raises(gc.GcowError):
        gc.encode_segmented(torch.zeros(8, device="cuda"), [4, 4], torch.zeros(3, dtype=torch.int32, device="cuda"))
    with pytest.raises(gc.GcowError):
        gc.encode_segmented(torch.zeros(9, device="cuda"), [4, 4], torch.zeros(2, dtype=torch.int32, device="cuda"))


# ------------------------------------------------------------------------------------------------ 2. the append chain
@pytest.mark.parametrize("bf16", BF, ids=BF_IDS)
def test_encode_equals_the_append_chain(gc, orc, bf16):
    name = "edges"
    cnts = SI.counts(name)
    ws = SI.words(name, bf16, "alt")
    x = _upload(SI.bucket(name, bf16))
    e = gc.encode_segmented(x, cnts, _words_tensor(ws, False), 64)
    words = torch.zeros(e.words.numel() + 4, dtype=torch.int64, device="cuda")
    live = [(o, n, w) for o, n, w in zip(np.cumsum([0] + cnts[:-1]), cnts, ws) if n]
    bits = torch.zeros(len(live) + 1, dtype=torch.int64, device="cuda")
    for i, (o, n, w) in enumerate(live):
        gc.encode_append(x[o:o + n], gc.fitted_params(64, SI.clamp(w)), words, bits[i:i + 1], bits[i + 1:i + 2])
    torch.cuda.synchronize()
    assert int(bits[-1]) == e.bits == SI.stream(name, bf16, "alt")[1]
    nw = (e.bits + 63) // 64
    assert np.array_equal(_u64(words)[:nw], _u64(e.words)[:nw])


# ------------------------------------------------------------------------------------------------ 3. the decode-mean
def _stream_buffer(name, sets, stride, odd):
    """W streams of fp32 data variants 0 .. W - 1 under sets[r] in one poisoned buffer: every slot holds garbage from
    its stream's last bit on, and so do the two words after the last slot -> (words, stream_words, index, index_words,
    the expected mean as fp32)."""
    W = len(sets)
    st = [SI.stream(name, False, sets[r], 64, r) for r in range(W)]
    sw = max(1, max(s[0].size for s in st)) + 1
    if (sw % 2 == 1) != odd:
        sw += 1
    buf = np.full(W * sw + 2, POISON, np.uint64)
    ne = max(1, max(SI.index_of(s[2], stride).size for s in st))
    iw = ne + 1
    idx = np.full(W * iw, POISON, np.uint64)
    for r, (w, total, pos, _) in enumerate(st):
        buf[r * sw:r * sw + w.size] = w
        if total % 64:  # the bits of the last word above the stream's last bit are garbage too
            buf[r * sw + w.size - 1] |= np.uint64((POISON << (total % 64)) & 0xFFFFFFFFFFFFFFFF)
        ix = SI.index_of(pos, stride)
        idx[r * iw:r * iw + ix.size] = ix
    mean = mean_codec.mean_of([s[3] for s in st])
    return (torch.from_numpy(buf.view(np.int64)).cuda(), sw, torch.from_numpy(idx.view(np.int64)).cuda(), iw, mean)


def _set_tensor(name, sets, shared: bool, records: bool):
    if shared:
        return _words_tensor(SI.words(name, False, sets[0]), records)
    rows = [_words_tensor(SI.words(name, False, s), records) for s in sets]
    return torch.stack(rows).contiguous()


CASES = [  # (word set per stream, one set for all, records, index stride, odd stream_words, guard elements)
    (("alt",), True, False, 16, True, 4),
    (("lo", "lo"), True, True, 8, False, 3),
    (("fit8", "lo", "clamp"), False, True, 16, True, 3),
    (("fit2.5", "hi"), False, False, 8, False, 4),
    (("lo", "fit0.5", "alt"), False, False, 16, False, 1),
]


@pytest.mark.parametrize("bf16_out", BF, ids=BF_IDS)
@pytest.mark.parametrize("name", SI.LISTS)
def test_decode_mean(gc, orc, name, bf16_out):
    cnts = SI.counts(name)
    n = sum(cnts)
    dt = torch.bfloat16 if bf16_out else torch.float32
    for sets, shared, records, stride, odd, guard in CASES:
        W = len(sets)
        buf, sw, idx, iw, mean = _stream_buffer(name, sets, stride, odd)
        assert sw % 2 == (1 if odd else 0)
        mx = _set_tensor(name, sets, shared, records)
        whole = torch.full((n + 2 * guard,), -1234.0, dtype=dt, device="cuda")
        sent = _bits_of(whole[:1])[0]
        out = whole[guard:guard + n]
        got = gc.decode_mean_segmented(buf, sw, W, cnts, mx, 64, idx, iw, stride, out=out)
        torch.cuda.synchronize()
        assert got.data_ptr() == out.data_ptr()
        want = SI.bf16_rne(mean) if bf16_out else mean.view(np.uint32)
        g = _bits_of(whole)
        assert np.array_equal(g[guard:guard + n], want), (sets, stride)
        assert (g[:guard] == sent).all() and (g[guard + n:] == sent).all(), (sets, stride)


def test_decode_mean_w1_is_the_plain_decode(gc, orc):
    """W = 1 under one word set: the oracle's decode itself (the mean of one stream adds +0 and divides by 1)."""
    name = "hook"
    cnts = SI.counts(name)
    x = _upload(SI.bucket(name, False))
    ws = SI.words(name, False, "fit8")
    e = gc.encode_segmented(x, cnts, _words_tensor(ws, True), 64, 16)
    torch.cuda.synchronize()
    nw = (e.bits + 63) // 64
    out = gc.decode_mean_segmented(e.words, nw, 1, cnts, _words_tensor(ws, False), 64, e.index, e.index.numel(), 16)
    torch.cuda.synchronize()
    dec = SI.stream(name, False, "fit8")[3]
    assert np.array_equal(_bits_of(out), mean_codec.mean_of([dec]).view(np.uint32))


# ------------------------------------------------------------------------------------------------ 4. fitted encoder
def _records(fits):
    return [_read_rec(r) for r in fits.cpu().numpy().view(np.uint64).reshape(-1, 2)]


def _read_rec(r):
    me = int(r[0]) & 0xFFFFFFFF
    return (me - (1 << 32) if me >> 31 else me), (int(r[0]) >> 32) & 0xFFFFFFFF, int(r[1])


@pytest.mark.parametrize("bf16", BF, ids=BF_IDS)
@pytest.mark.parametrize("name", ["edges", "hook"])
def test_per_tensor_fitted_encoder(gc, orc, name, bf16):
    cnts = SI.counts(name)
    x = _upload(SI.bucket(name, bf16))
    enc = gc.PerTensorFittedEncoder(8.0)
    for _ in range(2):  # the second call reuses every buffer
        e, fits = enc(x, cnts, 16)
        torch.cuda.synchronize()
        rec = FP.fits(name, bf16, 64, 8.0, FP.FLOOR)
        assert _records(fits) == list(rec)
        words, total, pos, _ = SI.stream(name, bf16, "fit8")
        assert e.bits == total == sum(r[2] for r in rec) <= sum(FP.budget_of(8.0, n) for n in cnts)
        assert np.array_equal(_u64(e.words)[:words.size], words)
        ix = SI.index_of(pos, 16)
        assert np.array_equal(_u64(e.index)[:ix.size], ix)
    assert enc.lst.rebuilds == 1


def test_per_tensor_fitted_encoder_graph(gc, orc):
    """The chain tables -> fits -> segmented encode captured on one stream and replayed on new data: the replay equals
    the eager call on that data (and so the oracle, by the test above)."""
    name = "hook"
    cnts = SI.counts(name)
    a0, a1 = SI.bucket(name, False, 0), SI.bucket(name, False, 1)
    x = _upload(a0)
    enc = gc.PerTensorFittedEncoder(8.0)
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        enc(x, cnts, 16, stream=s)  # plans, allocates and uploads: not capturable, and not needed again
    s.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, stream=s):
        e, fits = enc(x, cnts, 16, stream=s)
    assert enc.lst.rebuilds == 1
    x.copy_(_upload(a1))
    torch.cuda.synchronize()
    g.replay()
    torch.cuda.synchronize()
    got_bits, got_words, got_fits, got_index = e.bits, _u64(e.words).copy(), _records(fits), _u64(e.index).copy()
    eager, efits = gc.PerTensorFittedEncoder(8.0)(_upload(a1), cnts, 16)
    torch.cuda.synchronize()
    nw = (eager.bits + 63) // 64
    assert got_bits == eager.bits and got_fits == _records(efits)
    assert np.array_equal(got_words[:nw], _u64(eager.words)[:nw])
    assert np.array_equal(got_index, _u64(eager.index))
    w0 = SI.stream(name, False, "fit8")[0]  # the captured call's own data gave another stream: the replay followed x
    assert not np.array_equal(got_words[:w0.size], w0)


# ------------------------------------------------------------------------------------------------ 5. the hook
@pytest.fixture
def nccl_world1():
    import torch.distributed as dist
    dist.init_process_group("nccl", store=dist.HashStore(), rank=0, world_size=1, device_id=torch.device("cuda", 0))
    yield
    dist.destroy_process_group()


class _Bucket:
    def __init__(self, t, i, sizes):
        self.t, self.i, self.sizes = t, i, list(sizes)

    def buffer(self):
        return self.t

    def index(self):
        return self.i

    def gradients(self):
        return list(torch.split(self.t, self.sizes))


@pytest.mark.parametrize("bf16", BF, ids=BF_IDS)
def test_allgather_hook_per_tensor_budget_world1(gc, orc, nccl_world1, bf16):
    """One rank over RCCL, two buckets, the device codec: each bucket ends as the mean of one stream -- every gradient's
    oracle decode under its own fitted minexp (bf16: rounded to nearest even) -- and the state holds the records."""
    from gcow_amd import ddp
    from gcow_amd import dist as gdist

    calls = []

    class CountingCodec(gdist.DeviceCodec):
        def encode_per_tensor(self, *a, **k):
            calls.append("encode_per_tensor")
            return super().encode_per_tensor(*a, **k)

        def decode_mean_per_tensor(self, *a, **k):
            calls.append("decode_mean_per_tensor")
            return super().decode_mean_per_tensor(*a, **k)

        def encode(self, *a, **k):
            calls.append("encode")
            return super().encode(*a, **k)

    name = "hook"
    cnts = SI.counts(name)
    cdc = CountingCodec()
    state = ddp.make_hook_state(hook=ddp.compressed_allgather_hook, params=gc.accuracy(1e-3), codec=cdc, target_bits=8,
                                per_tensor_budget=True)
    rec = FP.fits(name, bf16, 64, 8.0, FP.FLOOR)
    mean = mean_codec.mean_of([SI.stream(name, bf16, "fit8")[3]])
    want = SI.bf16_rne(mean) if bf16 else mean.view(np.uint32)
    for i in range(2):
        t = _upload(SI.bucket(name, bf16))
        out = ddp.compressed_allgather_hook(state, _Bucket(t, i, cnts)).wait()
        torch.cuda.synchronize()
        out = out[0] if isinstance(out, (list, tuple)) else out
        assert out.data_ptr() == t.data_ptr()
        assert np.array_equal(_bits_of(out), want), i
        assert _records(state.fit_record(i)) == list(rec)
        assert sum(r[2] for r in rec) <= sum(FP.budget_of(8.0, n) for n in cnts)
    assert calls == ["encode_per_tensor", "decode_mean_per_tensor"] * 2 and not state._fits
