"""Relative tolerance on the wire, on the device (include/gcow.h "Relative tolerance over a segmented field";
codec.relative_minexp_segmented, codec.PerTensorRelativeEncoder / PerTensorRelativeResidualEncoder,
DeviceCodec.encode_relative / encode_residual_relative, compressed_allgather_hook with relative_bits). Everything is
compared bitwise, and every expectation comes from numpy (the fp32 add, the finite maximum), the rule restated in
tests/relative_inputs.py (minexp_of), the per-tensor oracle streams (tests/segmented_inputs.py, tests/residual_model.py)
or the older gcow_roundtrip_rel_device -- never from the call under test:

  1. words and maxima of the lists of relative_inputs as one flat bucket, at three offsets into its allocation;
  2. seams: neighbours 2^40 apart in scale, every tensor's maximum planted next to its seams;
  3. with a carried error: cancellation, overflow, a moved maximum, NaN, the top binade, mixed alignments;
  4. more tiles than workgroups;
  5. strides, guards and the ends of rel_bits;
  6. the encoder against the oracle streams, the decode and the list round trip;
  7. the residual encoder over two steps, in place;
  8. the chain captured into a graph;
  9. the receive side under int32[W, S] words;
  10. the hook at world 1 over RCCL, with and without error feedback, three buckets in flight;
  11. refusals with device pointers: the code, and nothing written.
Every test fails on a library without gcow_seg_rel_minexp_device."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

torch = pytest.importorskip("torch")

TESTS = os.path.dirname(os.path.abspath(__file__))
if TESTS not in sys.path:
    sys.path.insert(0, TESTS)

import mean_codec  # noqa: E402
import relative_inputs as RI  # noqa: E402
import segmented_inputs as SI  # noqa: E402
from residual_model import model_step, widen  # noqa: E402
from roundtrip_inputs import bf16_rne, bf16_trunc  # noqa: E402

pytestmark = pytest.mark.gpu

POISON32 = 0x5A5A5A5A
POISON64 = np.uint64(0x5A5A5A5A5A5A5A5A).astype(np.int64)
BF = [False, True]
BF_IDS = ["fp32", "bf16"]
K = 8


@pytest.fixture(scope="module")
def gc():
    if not torch.cuda.is_available():
        pytest.fail("GPU tests need a device")
    from gcow_amd import codec
    return codec


def _upload(a: np.ndarray, off: int = 0):
    """a on the device, `off` elements into its allocation (torch allocations are 256-byte aligned)."""
    t = torch.from_numpy(np.ascontiguousarray(a).copy())
    if a.dtype == np.uint16:
        t = t.view(torch.int16)
    buf = torch.zeros(t.numel() + off, dtype=t.dtype, device="cuda")
    buf[off:].copy_(t)
    v = buf[off:]
    return v.view(torch.bfloat16) if a.dtype == np.uint16 else v


def _u32(t):
    return t.cpu().numpy().view(np.uint32)


def _u64(t):
    return t.cpu().numpy().view(np.uint64)


def _bits_of(t):
    if t.dtype == torch.bfloat16:
        return t.view(torch.int16).cpu().numpy().view(np.uint16)
    return t.cpu().numpy().view(np.uint32)


def _as_input(ts, bf16):
    return [bf16_trunc(np.ascontiguousarray(t, np.float32)) if bf16 else np.ascontiguousarray(t, np.float32) for t in ts]


def _y_of(ts, es=None):
    """numpy's fp32 add, tensor by tensor (x widened exactly)."""
    with np.errstate(over="ignore", invalid="ignore"):
        return [(widen(t) + (np.zeros(t.size, np.float32) if es is None else es[s])).astype(np.float32)
                for s, t in enumerate(ts)]


def _expect(ys, k):
    amax = np.array([RI.absmax_of(y) for y in ys], np.float32)
    return amax, np.array([RI.minexp_of(a, k) for a in amax], np.int32)


def _run_words(gc, x, cnts, k, err=None):
    am = torch.full((len(cnts),), float("nan"), dtype=torch.float32, device="cuda")
    w = gc.relative_minexp_segmented(x, cnts, k, err=err, absmax=am)
    torch.cuda.synchronize()
    assert w.dtype == torch.int32 and w.numel() == len(cnts)
    return _u32(am), w.cpu().numpy()


def _check_words(gc, ts, k, es=None, xoff=0, eoff=0):
    cnts = [int(t.size) for t in ts]
    x = _upload(np.concatenate(ts), xoff)
    e = _upload(np.concatenate(es), eoff) if es is not None else None
    am, w = _run_words(gc, x, cnts, k, e)
    wa, ww = _expect(_y_of(ts, es), k)
    assert np.array_equal(am, wa.view(np.uint32)), (k, np.nonzero(am != wa.view(np.uint32))[0][:8])
    assert np.array_equal(w, ww), (k, np.nonzero(w != ww)[0][:8])
    return wa, ww


# ------------------------------------------------------------------------------------------------ 1. words and maxima
@pytest.mark.parametrize("off", [0, 1, 3])
@pytest.mark.parametrize("bf16", BF, ids=BF_IDS)
@pytest.mark.parametrize("name", RI.LISTS)
def test_words_and_maxima(gc, orc, name, bf16, off):
    ts = RI.tensors(name, bf16)
    cnts = [int(t.size) for t in ts]
    x = _upload(np.concatenate(ts), off)
    esz = 2 if bf16 else 4
    assert x.data_ptr() % 256 == off * esz
    for k in RI.KS:
        want = RI.expect(name, bf16, k, 64)[1]
        am, w = _run_words(gc, x, cnts, k)
        assert np.array_equal(am, want.view(np.uint32)), k
        assert np.array_equal(w, np.array([RI.minexp_of(a, k) for a in want], np.int32)), k
        # the older call on the same views, wherever they lie, leaves the same maxima
        views = list(torch.split(x, cnts))
        outs = [torch.empty(n, dtype=torch.float32, device="cuda") for n in cnts]
        old = torch.full((len(cnts),), float("nan"), dtype=torch.float32, device="cuda")
        gc.roundtrip_tensors_relative(views, k, outs=outs, absmax=old)
        torch.cuda.synchronize()
        assert views[0].data_ptr() == x.data_ptr()
        assert np.array_equal(_u32(old), want.view(np.uint32)), k
        assert np.array_equal(_u32(old), am), k


# ------------------------------------------------------------------------------------------------ 2. seams
SEAM_SIZES = [5, 3, 4091, 4096, 4097, 12295, 1, 0, 2]


def _seam_base():
    rng = np.random.default_rng(31)
    scales = [2.0 ** (20 if s % 2 == 0 else -20) for s in range(len(SEAM_SIZES))]
    ts = [(rng.uniform(0.5, 1.0, n) * rng.choice([-1.0, 1.0], n) * sc).astype(np.float32)
          for n, sc in zip(SEAM_SIZES, scales)]
    return ts, scales


@pytest.mark.parametrize("bf16", BF, ids=BF_IDS)
def test_seams(gc, bf16):
    """6151 virtual blocks in 7 tiles, seams at blocks 2, 3, 1026, 2050, 3075, 6149 and 6150: inside a lane's four
    blocks, in a tile's first and last lanes, a tensor of one tile's worth of blocks, uniform tiles in a row and an
    empty tensor. A value that leaked across a seam (2^40 away in scale, or the planted maximum, two binades up)
    changes a maximum and a word."""
    base, scales = _seam_base()
    places = {"first": lambda n: 0, "last": lambda n: n - 1, "before the partial block": lambda n: max(n // 4 * 4 - 1, 0)}
    _check_words(gc, _as_input(base, bf16), K)
    for s, n in enumerate(SEAM_SIZES):
        if not n:
            continue
        for what, at in places.items():
            ts = [t.copy() for t in base]
            ts[s][at(n)] = np.float32(-3.5 * scales[s])
            wa, _ = _check_words(gc, _as_input(ts, bf16), K)
            assert wa[s] == np.float32(3.5 * scales[s]), (s, what)


# ------------------------------------------------------------------------------------------------ 3. with e
def _err_cases(bf16):
    rng = np.random.default_rng(32)
    f32 = np.float32
    xs, es = [], []

    def add(x, e):
        x = _as_input([x], bf16)[0]
        xs.append(x)
        es.append(np.ascontiguousarray(e, f32))
        return widen(x)

    # e = -x exactly: a = 0, the word is the floor
    x = (rng.standard_normal(4100) * 3.0).astype(f32)
    xw = add(x, np.zeros(4100, f32))
    es[-1] = (-xw).astype(f32)
    # x + e overflows at some values (masked); the others decide
    x = (rng.uniform(0.5, 1.0, 64) * 2.0 ** 100).astype(f32)
    e = np.zeros(64, f32)
    x[[3, 17, 63]] = f32(3e38)
    e[[3, 17, 63]] = f32(3e38)
    add(x, e)
    # e moves the maximum to another position and another binade
    x = (rng.standard_normal(1030) * 1e-3).astype(f32)
    x[5] = f32(0.25)
    e = (rng.standard_normal(1030) * 1e-4).astype(f32)
    e[5] = f32(-0.25)
    e[1027] = f32(5.0)
    add(x, e)
    # NaN in e
    x = rng.standard_normal(37).astype(f32)
    e = (rng.standard_normal(37) * 0.1).astype(f32)
    e[[0, 20, 36]] = np.nan
    add(x, e)
    # y in the top binade: the cap applies
    x = np.full(9, 1.5e38, f32)
    e = np.full(9, 1.0e38, f32)
    x[4], e[4] = f32(1.7e38), f32(1.69e38)
    add(x, e)
    # an empty tensor and a short one with -0 + 0
    add(np.zeros(0, f32), np.zeros(0, f32))
    add(np.full(3, -0.0, f32), np.zeros(3, f32))
    return xs, es


@pytest.mark.parametrize("align", [(0, 0), (0, 1), (1, 0), (3, 2)], ids=["aligned", "e-off", "x-off", "both-off"])
@pytest.mark.parametrize("bf16", BF, ids=BF_IDS)
def test_words_with_carried_error(gc, bf16, align):
    xs, es = _err_cases(bf16)
    ys = _y_of(xs, es)
    wa, ww = _expect(ys, K)
    # the cases are what they claim to be
    assert wa[0] == 0 and ww[0] == RI.MINEXP_FLOOR
    assert np.isinf(ys[1]).sum() == 3 and 0 < wa[1] < 2.0 ** 101
    assert wa[2] > 4.0 and np.argmax(np.abs(ys[2])) == 1027
    assert np.isnan(ys[3]).sum() == 3 and wa[3] > 0
    assert wa[4] >= 2.0 ** 127 and ww[4] < 128 - K
    for k in RI.KS:
        _check_words(gc, xs, k, es, *align)


# ------------------------------------------------------------------------------------------------ 4. many tiles
def test_more_tiles_than_workgroups(gc):
    """1.31 M virtual blocks = 1282 tiles over 1024 workgroups: runs of one and two tiles, and runs that change tensor."""
    rng = np.random.default_rng(33)
    sizes = [1_800_001, 1_700_003, 1_750_000]
    ts = [(rng.standard_normal(n) * 2.0 ** sc).astype(np.float32) for n, sc in zip(sizes, (-10, 30, -25))]
    assert sum((n + 3) // 4 for n in sizes) > 1024 * 1024
    ts[0][sizes[0] - 5] = np.float32(0.75)  # the first tensor's maximum, in its last tile
    wa, _ = _check_words(gc, ts, K)
    assert wa[0] == np.float32(0.75)


# ------------------------------------------------------------------------------------------------ 5. strides, bounds
@pytest.mark.parametrize("k", [0, 24])
@pytest.mark.parametrize("bf16", BF, ids=BF_IDS)
def test_strides_and_guards(gc, bf16, k):
    ts = RI.tensors("edges", bf16)
    cnts = [int(t.size) for t in ts]
    S = len(cnts)
    x = _upload(np.concatenate(ts))
    wa, ww = _expect(_y_of(ts), k)
    # stride 4: word 0 of each record, nothing else
    recs = torch.full((S, 2), int(POISON64), dtype=torch.int64, device="cuda")
    assert gc.relative_minexp_segmented(x, cnts, k, out=recs) is recs
    torch.cuda.synchronize()
    got = recs.cpu().numpy().view(np.uint32).reshape(S, 4)
    assert np.array_equal(got[:, 0].view(np.int32), ww)
    assert (got[:, 1:] == POISON32).all()
    # stride 1 and the maxima, inside guarded allocations
    G = 8
    wbuf = torch.full((S + 2 * G,), POISON32, dtype=torch.int32, device="cuda")
    abuf = torch.full((S + 2 * G,), POISON32, dtype=torch.int32, device="cuda")
    gc.relative_minexp_segmented(x, cnts, k, absmax=abuf[G:G + S].view(torch.float32), out=wbuf[G:G + S])
    torch.cuda.synchronize()
    w, a = wbuf.cpu().numpy(), abuf.cpu().numpy()
    assert np.array_equal(w[G:G + S], ww) and np.array_equal(a[G:G + S].view(np.uint32), wa.view(np.uint32))
    for g in (w, a):
        assert (g[:G] == POISON32).all() and (g[G + S:] == POISON32).all()


# ------------------------------------------------------------------------------------------------ 6. the encoder
def _index_equal(e, pos, stride):
    if not stride:
        assert e.index is None
        return
    ix = SI.index_of(pos, stride)
    assert np.array_equal(_u64(e.index)[:ix.size], ix)


@pytest.mark.parametrize("maxprec", [64, 12])
@pytest.mark.parametrize("bf16", BF, ids=BF_IDS)
@pytest.mark.parametrize("name", ["edges", "hook"])
def test_relative_encoder(gc, orc, name, bf16, maxprec):
    ts = RI.tensors(name, bf16)
    cnts = [int(t.size) for t in ts]
    decs, amax, bits = RI.expect(name, bf16, K, maxprec)
    ww = tuple(RI.minexp_of(a, K) for a in amax)
    words, total, pos, dec = SI.stream(name, bf16, ww, maxprec)
    assert total == bits and np.array_equal(dec.view(np.uint32), np.concatenate(decs).view(np.uint32))
    x = _upload(np.concatenate(ts))
    # the older call on the same views: outputs and bit count
    outs = [torch.empty(n, dtype=torch.float32, device="cuda") for n in cnts]
    rbits = torch.zeros(1, dtype=torch.int64, device="cuda")
    gc.roundtrip_tensors_relative(list(torch.split(x, cnts)), K, outs=outs, bits=rbits, maxprec=maxprec)
    torch.cuda.synchronize()
    old = np.concatenate([_u32(o) for o in outs])
    assert np.array_equal(old, dec.view(np.uint32)) and int(rbits.item()) == total
    for stride in SI.STRIDES:
        enc = gc.PerTensorRelativeEncoder(K, maxprec)
        e, w = enc(x, cnts, stride)
        torch.cuda.synchronize()
        assert np.array_equal(w.cpu().numpy(), np.array(ww, np.int32))
        assert np.array_equal(_u32(enc.absmax), amax.view(np.uint32))
        assert e.bits == total == int(rbits.item())
        assert np.array_equal(_u64(e.words)[:words.size], words)
        _index_equal(e, pos, stride)
        if stride:
            nw = (total + 63) // 64
            got = gc.decode_mean_segmented(e.words, nw, 1, cnts, w, maxprec, e.index, e.index.numel(), stride)
            torch.cuda.synchronize()
            want = mean_codec.mean_of([dec])
            assert np.array_equal(_u32(got), want.view(np.uint32))
            assert np.array_equal(_u32(got), mean_codec.mean_of([old.view(np.float32)]).view(np.uint32))


# ------------------------------------------------------------------------------------------------ 7. the residual form
def _model(ts, carried, k, maxprec):
    """One step of every tensor under the word of its y: -> (words, stream, bits, block positions, decode, residuals)."""
    from oracle import oracle as O
    ww, pieces, lens, decs, res = [], [], [], [], []
    ys = _y_of(ts, carried)
    for s, t in enumerate(ts):
        m = RI.minexp_of(RI.absmax_of(ys[s]), k)
        ww.append(m)
        if not t.size:
            res.append(np.zeros(0, np.float32))
            decs.append(np.zeros(0, np.float32))
            continue
        p = O.expert(1, 16658, maxprec, m)
        y, w, b, d, r = model_step(t, carried[s] if carried is not None else None, p)
        pieces.append((w, b))
        lens.append(O.block_bits(y, p).astype(np.uint64))
        decs.append(d)
        res.append(r.astype(np.float32))
    stream, total, _ = SI.concat_bits(pieces)
    lens = np.concatenate(lens)
    pos = np.concatenate([[0], np.cumsum(lens)[:-1]]).astype(np.uint64)
    return np.array(ww, np.int32), stream, total, pos, np.concatenate(decs), res


@pytest.mark.parametrize("bf16", BF, ids=BF_IDS)
def test_relative_residual_encoder_two_steps(gc, orc, bf16):
    name = "hook"
    cnts = SI.counts(name)
    enc = gc.PerTensorRelativeResidualEncoder(K)
    err = torch.zeros(sum(cnts), dtype=torch.float32, device="cuda")
    carried = [np.zeros(n, np.float32) for n in cnts]
    for step in range(2):
        ts = SI.variant(name, bf16, step)
        ww, stream, total, pos, _, res = _model(ts, carried, K, 64)
        x = _upload(np.concatenate(ts))
        keep = _bits_of(x).copy()
        e, w = enc(x, err, cnts, 16)
        torch.cuda.synchronize()
        assert np.array_equal(w.cpu().numpy(), ww), step
        assert e.bits == total and np.array_equal(_u64(e.words)[:stream.size], stream), step
        _index_equal(e, pos, 16)
        assert np.array_equal(_u32(err), np.concatenate(res).view(np.uint32)), step  # in place
        assert np.array_equal(_bits_of(x), keep)
        # the stream is the segmented encode of the fp32 array y under the words of y
        y = np.concatenate(_y_of(ts, carried))
        plain = gc.encode_segmented(_upload(y), cnts, w, 64, 16)
        torch.cuda.synchronize()
        assert plain.bits == total and np.array_equal(_u64(plain.words)[:stream.size], stream), step
        carried = res
    assert np.concatenate(carried).any()


# ------------------------------------------------------------------------------------------------ 8. the graph
def test_relative_encoder_graph(gc, orc):
    """The chain words -> segmented encode captured on one stream and replayed on new data: the replay equals the eager
    call on that data (and so the oracle, by the tests above)."""
    name = "hook"
    cnts = SI.counts(name)
    a0 = SI.bucket(name, False, 0)
    a1 = (SI.bucket(name, False, 1) * np.float32(2.0 ** 7)).astype(np.float32)  # other words as well as another stream
    x = _upload(a0)
    enc = gc.PerTensorRelativeEncoder(K)
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        enc(x, cnts, 16, stream=s)  # plans and allocates: not capturable, and not needed again
    s.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, stream=s):
        e, w = enc(x, cnts, 16, stream=s)
    x.copy_(_upload(a1))
    torch.cuda.synchronize()
    g.replay()
    torch.cuda.synchronize()
    got_bits, got_words, got_w, got_index = e.bits, _u64(e.words).copy(), w.cpu().numpy().copy(), _u64(e.index).copy()
    eager, ew = gc.PerTensorRelativeEncoder(K)(_upload(a1), cnts, 16)
    torch.cuda.synchronize()
    nw = (eager.bits + 63) // 64
    assert got_bits == eager.bits and np.array_equal(got_w, ew.cpu().numpy())
    assert np.array_equal(got_words[:nw], _u64(eager.words)[:nw])
    assert np.array_equal(got_index, _u64(eager.index))
    ts0 = RI.tensors(name, False)
    assert not np.array_equal(got_w, _expect(_y_of(ts0), K)[1])  # the replay followed x, words included


# ------------------------------------------------------------------------------------------------ 9. the receive side
@pytest.mark.parametrize("bf16_out", BF, ids=["out-fp32", "out-bf16"])
@pytest.mark.parametrize("bf16", BF, ids=BF_IDS)
def test_receive_under_int32_words(gc, orc, bf16, bf16_out):
    from gcow_amd import dist as gdist
    name, W = "hook", 3
    cnts = SI.counts(name)
    S = len(cnts)
    sets, streams = [], []
    for r, k in enumerate(RI.KS):
        amax = _expect(_y_of(SI.variant(name, bf16, r)), k)[0]
        ww = tuple(RI.minexp_of(a, k) for a in amax)
        sets.append(ww)
        streams.append(SI.stream(name, bf16, ww, 64, r))
    assert len(set(sets)) == W
    sw = max(st[0].size for st in streams)
    ni = (sum((n + 3) // 4 for n in cnts) + 15) // 16
    buf = np.full(W * sw + 2, np.uint64(0x5A5A5A5A5A5A5A5A), np.uint64)
    idx = np.zeros(W * ni, np.uint64)
    for r, (words, _, pos, _) in enumerate(streams):
        buf[r * sw:r * sw + words.size] = words
        idx[r * ni:(r + 1) * ni] = SI.index_of(pos, 16)
    fits = torch.tensor(sets, dtype=torch.int32, device="cuda")
    assert tuple(fits.shape) == (W, S)
    out = torch.empty(sum(cnts), dtype=torch.bfloat16 if bf16_out else torch.float32, device="cuda")
    gdist.DeviceCodec().decode_mean_per_tensor(torch.from_numpy(buf.view(np.int64)).cuda(), sw, W, cnts, fits, 64,
                                               torch.from_numpy(idx.view(np.int64)).cuda(), ni, 16, out=out)
    torch.cuda.synchronize()
    mean = mean_codec.mean_of([st[3] for st in streams])
    assert np.array_equal(_bits_of(out), bf16_rne(mean) if bf16_out else mean.view(np.uint32))


# ------------------------------------------------------------------------------------------------ 10. the hook
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


@pytest.mark.parametrize("feedback", [False, True], ids=["plain", "feedback"])
@pytest.mark.parametrize("bf16", BF, ids=BF_IDS)
def test_allgather_hook_relative_world1(gc, orc, nccl_world1, bf16, feedback):
    """One rank over RCCL, the device codec, two steps with three buckets in flight: each bucket ends as the mean of one
    stream -- every gradient's oracle decode under the word of its own y (bf16: rounded to nearest even) -- and with
    error feedback the state's buffers hold the model's y - decode."""
    from gcow_amd import ddp
    from gcow_amd import dist as gdist

    calls = []

    class CountingCodec(gdist.DeviceCodec):
        pass

    def counted(name):
        def f(self, *a, **k):
            calls.append(name)
            return getattr(gdist.DeviceCodec, name)(self, *a, **k)
        return f

    for m in ("encode_relative", "encode_residual_relative", "decode_mean_per_tensor", "roundtrip_relative", "encode"):
        setattr(CountingCodec, m, counted(m))

    name, NB = "hook", 3
    cnts = SI.counts(name)
    state = ddp.make_hook_state(hook=ddp.compressed_allgather_hook, params=gc.accuracy(1e-3), codec=CountingCodec(),
                                relative_bits=K, error_feedback=feedback)
    carried = [[np.zeros(n, np.float32) for n in cnts] for _ in range(NB)]
    for step in range(2):
        bufs, futs, wants = [], [], []
        for i in range(NB):
            ts = SI.variant(name, bf16, (i + step) % 3)
            _, _, _, _, dec, res = _model(ts, carried[i] if feedback else None, K, 64)
            if feedback:
                carried[i] = res
            mean = mean_codec.mean_of([dec])
            wants.append(bf16_rne(mean) if bf16 else mean.view(np.uint32))
            bufs.append(_upload(np.concatenate(ts)))
        for i in range(NB):
            futs.append(ddp.compressed_allgather_hook(state, _Bucket(bufs[i], i, cnts)))
        for i in range(NB):
            out = futs[i].wait()
            torch.cuda.synchronize()
            out = out[0] if isinstance(out, (list, tuple)) else out
            assert out.data_ptr() == bufs[i].data_ptr()
            assert np.array_equal(_bits_of(out), wants[i]), (step, i)
            if feedback:
                got = _u32(state.error_buffer(i, bufs[i]))
                assert np.array_equal(got, np.concatenate(carried[i]).view(np.uint32)), (step, i)
    enc = "encode_residual_relative" if feedback else "encode_relative"
    assert sorted(calls) == sorted([enc, "decode_mean_per_tensor"] * (2 * NB))
    assert "roundtrip_relative" not in calls
    assert feedback or not state._errors
    assert not feedback or np.concatenate(carried[0]).any()


# ------------------------------------------------------------------------------------------------ 11. refusals
@pytest.mark.parametrize("bf16", BF, ids=BF_IDS)
def test_device_side_refusals_write_nothing(gc, bf16):
    from gcow_amd import _ffi
    L = _ffi.load()
    cnts = [5, 0, 4100]
    dtype = torch.bfloat16 if bf16 else torch.float32
    pl = gc.SegmentPlan(cnts, dtype, "cuda")
    x = torch.ones(sum(cnts), dtype=dtype, device="cuda")
    e = torch.ones(sum(cnts) + 1, dtype=torch.float32, device="cuda")
    am = torch.full((4,), POISON32, dtype=torch.int32, device="cuda")
    w = torch.full((4,), POISON32, dtype=torch.int32, device="cuda")
    INVALID = 1

    def call(h=pl.h.data_ptr(), hb=pl.used, d=pl.d.data_ptr(), xp=x.data_ptr(), ep=None, k=K, a=am.data_ptr(),
             m=w.data_ptr(), ms=1):
        return L.gcow_seg_rel_minexp_device(h, d, hb, xp, ep, k, a, m, ms, None)

    junk = (C.c_uint64 * 16)()
    for bad in (dict(h=None), dict(h=junk, hb=128), dict(hb=pl.used - 8), dict(k=25), dict(a=None),
                dict(a=am.data_ptr() + 2), dict(m=None), dict(m=w.data_ptr() + 2), dict(ms=0), dict(d=None),
                dict(d=pl.d.data_ptr() + 4), dict(xp=None), dict(xp=x.data_ptr() + (1 if bf16 else 2)), dict(ep=e.data_ptr() + 2)):
        assert call(**bad) == INVALID, bad
    torch.cuda.synchronize()
    assert (am.cpu().numpy() == POISON32).all() and (w.cpu().numpy() == POISON32).all()
    # and the good call through the same pointers, an error array off 16 bytes included
    assert call(ep=e.data_ptr() + 4) == 0
    torch.cuda.synchronize()
    assert np.array_equal(am.cpu().numpy()[:3].view(np.float32), np.array([2.0, 0.0, 2.0], np.float32))
    assert np.array_equal(w.cpu().numpy()[:3], np.array([2 - K, RI.MINEXP_FLOOR, 2 - K], np.int32))
    assert am.cpu().numpy()[3] == POISON32 and w.cpu().numpy()[3] == POISON32
