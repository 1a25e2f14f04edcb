"""GPU parity of decode + mean + encode (gcow_decode_mean_encode_device, include/gcow.h), bitwise, against the
reference model (tests/mean_codec.py: numpy over the oracle) and against the composition of the existing device calls
(decode_mean into an fp32 tensor, then encode / encode_residual): the stream and its bit count, the new error,
e_in = NULL, in place, chained steps, the bytes after both outputs, argument checks, compressed_sharded_hook with
`compress_mean` over a one-rank RCCL group, and three processes sharing the GPU over gloo.

Sizes: one value, partial and whole single blocks, and the fused kernel's workgroup chunk C = 256 lanes x U blocks
(U = GCOW_MEANENC_U = 2: 512 blocks): 4 C - 1, 4 C, 4 C + 1 and 12 C + 5 values. nstreams 3 takes mean_scale's
division, the others its reciprocal. rate 16 / 8 run the fused kernel; rate 12, expert(64, 64, 20, -1074) and
rate 16 -> rate 8 the composed path at fixed rate; accuracy / precision the composed path at variable rate with the
input index every 8 blocks, accuracy also with the packed 16-block index."""
import ctypes as C
import functools
import os
import sys
import tempfile

import numpy as np
import pytest

torch = pytest.importorskip("torch")

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
U = 2  # gcow_amd/csrc/mean_enc1d.hip GCOW_MEANENC_U
CHUNK = 256 * U
SIZES = [1, 3, 4, 5, 4 * CHUNK - 1, 4 * CHUNK, 4 * CHUNK + 1, 12 * CHUNK + 5]
NSTREAMS = [1, 2, 3, 8]
FUSED = ["rate16", "rate8"]
MODES = FUSED + ["rate12", "expert64_prec20", "rate16to8", "acc1e-3", "prec12", "acc1e-3_pk"]
PACKED16 = 0x1010
SENT_F = 1234.5
SENT_W = 0x5A5A5A5A5A5A5A5A


@pytest.fixture(scope="module")
def gc():
    if not torch.cuda.is_available():
        pytest.fail("GPU tests need a device")
    from gcow_amd import codec
    return codec


def _ops(O, mode):
    """(input set, output set, input index stride) of a mode."""
    one = {"rate16": O.rate(16, 1), "rate8": O.rate(8, 1), "rate12": O.rate(12, 1),
           "expert64_prec20": O.expert(64, 64, 20, -1074), "acc1e-3": O.accuracy(1e-3), "prec12": O.precision(12)}
    if mode == "rate16to8":
        return one["rate16"], one["rate8"], 0
    if mode == "acc1e-3_pk":
        return one["acc1e-3"], one["acc1e-3"], PACKED16
    p = one[mode]
    return p, p, (0 if p.minbits == p.maxbits else 8)


def _index(O, x, op, stride):
    lens = O.block_bits(x, op).astype(np.uint64)
    off = np.concatenate([[0], np.cumsum(lens)[:-1]]).astype(np.uint64)
    return off[::stride]


@functools.lru_cache(maxsize=None)
def _case(n, nstreams, mode):
    """W gradient-like buckets with different seeds and test_gpu_residual's crafted blocks at the same places in every
    one (long group phases and budget-crossing planes for the decoders' and the coder's special lanes, subnormal
    blocks, NaN / Inf, and a block of 3e38 whose sum over two or more streams overflows: the mean is Inf, the coder
    takes its special path and the residual is +0), coded by the oracle; the model's plain encode of their mean, its
    three chained error-feedback steps from e0, and the step from e = NULL. Computed once per case, never modified."""
    from mean_codec import mean_of
    from oracle import oracle as O
    from residual_model import model_step
    from test_gpu_residual import _inputs
    op_in, op_out, istride = _ops(O, mode)
    x0, e0 = _inputs(n, False, op_out)
    # the subnormal block decodes to zeros in every received stream: its carried error is subnormal instead, so that
    # y is, and with it the residual
    e0 = e0.copy()
    at = 4 if n >= 64 else 0
    e0[at:at + 4] = np.array([1e-40, 2e-40, -3e-41, 0.0], np.float32)[: min(4, n - at)]
    base = O.gen_normal(n, 1e-3, 501, True)
    plain = x0.view(np.uint32) == base.view(np.uint32)  # outside the crafted blocks
    streams, decs, idx = [], [], []
    for r in range(nstreams):
        x = x0.copy()
        x[plain] = O.gen_normal(n, 1e-3, 900 + r, True)[plain]
        w, _ = O.compress(x, op_in)
        streams.append(w)
        decs.append(O.decompress(w, (n,), op_in))
        if istride:
            i8 = _index(O, x, op_in, 8)
            if istride == PACKED16:  # include/gcow.h GCOW_INDEX_PACKED16
                a, b = i8[0::2], np.zeros_like(i8[0::2])
                b[: len(i8[1::2])] = i8[1::2] - a[: len(i8[1::2])]
                i8 = a | (b << np.uint64(48))
            idx.append(i8)
    sw = max(len(w) for w in streams)
    buf = np.zeros(nstreams * sw + 2, np.uint64)
    for r, w in enumerate(streams):
        buf[r * sw:r * sw + len(w)] = w
    iw = len(idx[0]) if idx else 0
    m = mean_of(decs)
    w_plain, bits_plain = O.compress(m, op_out)
    steps, e = [], e0
    for _ in range(3):
        _, w, bits, _, e = model_step(m, e, op_out)
        steps.append((w, bits, e))
    null = model_step(m, None, op_out)
    out_index = None if op_out.minbits == op_out.maxbits else _index(O, m, op_out, 16)
    for a in [buf, m, e0, w_plain] + [s[2] for s in steps]:
        a.setflags(write=False)
    return {"op_in": op_in, "op_out": op_out, "istride": istride, "streams": buf, "sw": sw,
            "index": np.concatenate(idx) if idx else None, "iw": iw, "m": m, "e0": e0, "plain": (w_plain, bits_plain),
            "steps": steps, "null": (null[1], null[2], null[4]), "out_index": out_index}


def _dev(a):
    return torch.from_numpy(np.array(a).view(np.int64) if a.dtype == np.uint64 else np.array(a)).cuda()


def _bits_eq(t, ref):
    return np.array_equal(t.cpu().numpy().view(np.uint32), ref.view(np.uint32))


def _call(gc, c, n, nstreams, e_in, e_out, nwords, streams=None, cap=None, wsb=None):
    """gcow_decode_mean_encode_device through the C ABI into sentinel-filled buffers: -> (status, stream words, bits,
    the 4 words after the stream, the output index)."""
    from gcow_amd._ffi import load
    L = load()
    p_in, p_out = gc.expert(*c["op_in"].tuple()), gc.expert(*c["op_out"].tuple())
    f = gc.field_of_shape((n,), torch.float32)
    need = L.gcow_max_output_bytes(C.byref(f), C.byref(p_out))
    words = torch.full((max((need + 7) // 8, nwords + 4),), SENT_W, dtype=torch.int64, device="cuda")
    bits = torch.full((1,), -1, dtype=torch.int64, device="cuda")
    if wsb is None:
        wsb = L.gcow_decode_mean_encode_workspace_bytes(C.byref(f), C.byref(p_in), C.byref(p_out))
    ws = torch.empty(max(wsb // 8, 1), dtype=torch.int64, device="cuda")
    streams = _dev(c["streams"]) if streams is None else streams
    index = _dev(c["index"]) if c["index"] is not None else None
    ostride = 0 if gc.is_fixed(p_out) else 16
    oindex = torch.full((max((n + 63) // 64, 1),), -1, dtype=torch.int64, device="cuda") if ostride else None
    st = L.gcow_decode_mean_encode_device(
        C.byref(f), C.byref(p_in), streams.data_ptr(), streams.numel() * 8, c["sw"], nstreams,
        index.data_ptr() if index is not None else None, c["iw"], c["istride"], C.byref(p_out),
        e_in.data_ptr() if e_in is not None else None, e_out.data_ptr() if e_out is not None else None,
        words.data_ptr(), words.numel() * 8 if cap is None else cap, bits.data_ptr(), ws.data_ptr(), wsb,
        oindex.data_ptr() if oindex is not None else None, ostride, torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    return (st, words[:nwords].cpu().numpy().view(np.uint64), int(bits.item()),
            words[nwords:nwords + 4].cpu().numpy().view(np.uint64), oindex)


def _path(gc, c, n, residual):
    from gcow_amd._ffi import load
    f = gc.field_of_shape((n,), torch.float32)
    p_in, p_out = gc.expert(*c["op_in"].tuple()), gc.expert(*c["op_out"].tuple())
    e = torch.zeros(4, device="cuda").data_ptr() if residual else None
    return load().gcow_decode_mean_encode_path(C.byref(f), C.byref(p_in), C.byref(p_out), e, e,
                                               1 if c["istride"] else None, None if gc.is_fixed(p_out) else 1)


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("nstreams", NSTREAMS)
@pytest.mark.parametrize("n", SIZES)
def test_decode_mean_encode_matches_model(gc, orc, n, nstreams, mode):
    c = _case(n, nstreams, mode)
    for residual in (False, True):
        assert _path(gc, c, n, residual) == (gc.MEANENC_FUSED_FIXED if mode in FUSED else gc.MEANENC_COMPOSED)
    # no error feedback: the stream of the mean, 4 sentinel words after it
    w_ref, bits_ref = c["plain"]
    st, w, bits, after, oindex = _call(gc, c, n, nstreams, None, None, w_ref.size)
    assert st == 0
    assert bits == bits_ref and w.tobytes() == w_ref.tobytes()
    assert np.all(after == SENT_W)
    if oindex is not None:
        assert np.array_equal(oindex.cpu().numpy().view(np.uint64), c["out_index"])
    # the composition of the existing device calls gives the same stream (and the model's mean)
    p_in, p_out = gc.expert(*c["op_in"].tuple()), gc.expert(*c["op_out"].tuple())
    streams = _dev(c["streams"])
    index = _dev(c["index"]) if c["index"] is not None else None
    m = gc.decode_mean(streams, c["sw"], nstreams, n, p_in, index, c["iw"], c["istride"])
    e = gc.encode(m, p_out)
    torch.cuda.synchronize()
    assert _bits_eq(m, c["m"])
    assert e.bits == bits and e.to_bytes() == w.tobytes()
    # with e_in, out of place: 16 sentinel floats after e_out[n - 1]
    w_ref, bits_ref, e_ref = c["steps"][0]
    e_in = _dev(c["e0"])
    buf = torch.full((n + 16,), SENT_F, dtype=torch.float32, device="cuda")
    st, w, bits, after, _ = _call(gc, c, n, nstreams, e_in, buf[:n], w_ref.size)
    assert st == 0 and bits == bits_ref and w.tobytes() == w_ref.tobytes()
    assert _bits_eq(buf[:n], e_ref)
    assert torch.all(buf[n:] == SENT_F) and np.all(after == SENT_W)
    assert _bits_eq(e_in, c["e0"])  # the input error is only read
    err = _dev(c["e0"]).clone()
    e2 = gc.encode_residual(m, err, p_out)
    torch.cuda.synchronize()
    assert e2.to_bytes() == w.tobytes() and _bits_eq(err, e_ref)
    # in place: the same result
    buf2 = torch.full((n + 16,), SENT_F, dtype=torch.float32, device="cuda")
    buf2[:n] = _dev(c["e0"])
    st, w, bits, after, _ = _call(gc, c, n, nstreams, buf2[:n], buf2[:n], w_ref.size)
    assert st == 0 and bits == bits_ref and w.tobytes() == w_ref.tobytes()
    assert _bits_eq(buf2[:n], e_ref)
    assert torch.all(buf2[n:] == SENT_F) and np.all(after == SENT_W)
    # e_in = NULL is e_in = zeros
    wn_ref, bitsn_ref, en_ref = c["null"]
    buf3 = torch.full((n + 16,), SENT_F, dtype=torch.float32, device="cuda")
    st, w, bits, after, _ = _call(gc, c, n, nstreams, None, buf3[:n], wn_ref.size)
    assert st == 0 and bits == bitsn_ref and w.tobytes() == wn_ref.tobytes()
    assert _bits_eq(buf3[:n], en_ref)
    assert torch.all(buf3[n:] == SENT_F) and np.all(after == SENT_W)


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("nstreams", [2, 3])
@pytest.mark.parametrize("n", [5, 4 * CHUNK + 1, 12 * CHUNK + 5])
def test_three_chained_steps(gc, orc, n, nstreams, mode):
    """The preallocated ReduceEncoder three times on one err tensor, and the one-call forms."""
    c = _case(n, nstreams, mode)
    p_in, p_out = gc.expert(*c["op_in"].tuple()), gc.expert(*c["op_out"].tuple())
    streams = _dev(c["streams"])
    index = _dev(c["index"]) if c["index"] is not None else None
    err = _dev(c["e0"]).clone()
    enc = gc.ReduceEncoder(n, p_in, nstreams, p_out, "cuda", residual=True,
                           index_stride_out=0 if gc.is_fixed(p_out) else 16)
    assert enc.path == (gc.MEANENC_FUSED_FIXED if mode in FUSED else gc.MEANENC_COMPOSED)
    for w_ref, bits_ref, e_ref in c["steps"]:
        e = enc(streams, c["sw"], index, c["iw"], c["istride"], err=err)
        torch.cuda.synchronize()
        assert e.bits == bits_ref and e.to_bytes() == w_ref.tobytes()
        assert _bits_eq(err, e_ref)
    if not gc.is_fixed(p_out):  # the index written is the stream's: the decoder finds every chunk through it
        d = gc.decode(e).cpu().numpy()
        ref = orc.decompress(c["steps"][2][0], (n,), c["op_out"])
        assert np.array_equal(d.view(np.uint32), ref.view(np.uint32))
    e = gc.decode_mean_encode(streams, c["sw"], nstreams, n, p_in, index, c["iw"], c["istride"], out_params=p_out)
    torch.cuda.synchronize()
    assert e.bits == c["plain"][1] and e.to_bytes() == c["plain"][0].tobytes()
    from gcow_amd.dist import DeviceCodec
    cdc = DeviceCodec()
    for _ in range(2):  # the second call reuses the cached encoder
        err2 = _dev(c["e0"]).clone()
        words, bits, _ = cdc.decode_mean_encode(streams, c["sw"], nstreams, n, p_in, index, c["iw"], c["istride"],
                                                out_params=p_out, err=err2, slot="s")
        torch.cuda.synchronize()
        nw = c["steps"][0][0].size
        assert int(bits.item()) == c["steps"][0][1]
        assert words[:nw].cpu().numpy().view(np.uint64).tobytes() == c["steps"][0][0].tobytes()
        assert _bits_eq(err2, c["steps"][0][2])
    assert len(cdc._enc) == 1


def test_argument_checks(gc, orc):
    from gcow_amd._ffi import load
    L = load()
    n = 4 * CHUNK + 1
    for mode in ("rate16", "rate12", "acc1e-3"):
        c = _case(n, 2, mode)
        nw = c["plain"][0].size
        assert _call(gc, c, n, 2, None, None, nw)[0] == 0
        short = _dev(c["streams"])[:-2].contiguous()  # without the two slack words
        assert _call(gc, c, n, 2, None, None, nw, streams=short)[0] == 1           # GCOW_ERR_INVALID
        assert _call(gc, c, n, 2, None, None, nw, cap=8 * nw - 8)[0] == 2          # GCOW_ERR_CAPACITY, the encoder's
        e = torch.zeros(n, device="cuda")
        assert _call(gc, c, n, 2, e, None, nw)[0] == 1                             # d_err_in without d_err_out
        if mode != "rate16":  # the composed path needs its workspace
            assert _call(gc, c, n, 2, None, None, nw, wsb=4 * n)[0] == 1           # the encoder's workspace error
            assert _call(gc, c, n, 2, None, e, nw, wsb=4 * n)[0] == 1
        else:
            f = gc.field_of_shape((n,), torch.float32)
            p = gc.rate(16, 1)
            assert L.gcow_decode_mean_encode_workspace_bytes(C.byref(f), C.byref(p), C.byref(p)) == 0
            # a misaligned error buffer sends the call to the composed path
            assert L.gcow_decode_mean_encode_path(C.byref(f), C.byref(p), C.byref(p), None, 16 + 4, None, None) == 0
            assert L.gcow_decode_mean_encode_path(C.byref(f), C.byref(p), C.byref(p), None, 16 + 2, None, None) == -1
    # n = 0 writes a zero bit count
    c = _case(5, 2, "rate16")
    st, _, bits, after, _ = _call(gc, c, 0, 2, None, None, 0)
    assert st == 0 and bits == 0 and np.all(after == SENT_W)
    f2 = gc.field_of(torch.zeros(8, 8, device="cuda"))
    p = gc.rate(16, 1)
    assert L.gcow_decode_mean_encode_path(C.byref(f2), C.byref(p), C.byref(p), None, None, None, None) == -1
    with pytest.raises(gc.GcowError):
        gc.ReduceEncoder(64, p, 2, residual=True)(torch.zeros(66, dtype=torch.int64, device="cuda"), 32)  # no err


# ---------------------------------------------------------------------------------------------- the hook, RCCL
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


def _hook_modes(gc):
    return {"rate16": gc.rate(16, 1), "acc1e-3": gc.accuracy(1e-3)}


@pytest.mark.parametrize("mode", ["rate16", "acc1e-3"])
@pytest.mark.parametrize("bf16", [False, True], ids=["fp32", "bf16"])
@pytest.mark.parametrize("variant", ["plain", "ef", "ef_coarse_mean"])
def test_compress_mean_hook_world1(gc, orc, nccl_world1, variant, bf16, mode):
    """One rank over RCCL, two buckets, two steps, the device codec: every bucket comes back as the model's
    decode(encode((0 + yhat) / 1 + e2)) (a bf16 bucket: rounded to nearest even) and the state holds both errors.
    With one rank the mean is a decode, which the same parameter set codes again without loss (e2 stays zero), so
    "ef_coarse_mean" codes the mean under a coarser set (mean_params: rate 8, accuracy 1e-2) and carries a real e2."""
    from gcow_amd import ddp
    from mean_codec import mean_model_step
    from residual_model import model_step, widen
    p = _hook_modes(gc)[mode]
    op = orc.expert(*p.tuple())
    ef = variant != "plain"
    mp = {"rate16": gc.rate(8, 1), "acc1e-3": gc.accuracy(1e-2)}[mode] if variant == "ef_coarse_mean" else None
    omp = orc.expert(*(mp or p).tuple())
    sizes = [12 * CHUNK + 5, 4 * CHUNK + 1]
    state = ddp.make_hook_state(hook=ddp.compressed_sharded_hook, params=p, compress_mean=True, error_feedback=ef,
                                mean_params=mp)
    e1, e2 = [None, None], [None, None]
    for step in range(2):
        for i, n in enumerate(sizes):
            a = orc.gen_normal(n, 1e-3, 700 + 8 * step + i, True)
            x = (a.view(np.uint32) >> 16).astype(np.uint16) if bf16 else a
            if ef:
                _, _, _, d, e1[i] = model_step(x, e1[i], op)
                _, _, _, want, e2[i] = mean_model_step([d], e2[i], omp)
            else:
                xf = widen(x)
                d = orc.decompress(orc.compress(xf, op)[0], (n,), op)
                m = mean_model_step([d], None, omp)[0]
                want = orc.decompress(orc.compress(m, omp)[0], (n,), omp)
            t = torch.from_numpy(np.array(x)).cuda()
            t = t.view(torch.bfloat16) if bf16 else t
            out = ddp.compressed_sharded_hook(state, _Bucket(t, i)).wait()
            torch.cuda.synchronize()
            out = out[0] if isinstance(out, (list, tuple)) else out
            if bf16:
                got = out.float().cpu().numpy()
                ref = torch.from_numpy(want).to(torch.bfloat16).float().numpy()
                assert np.array_equal(got.view(np.uint32), ref.view(np.uint32)), (step, i)
            else:
                assert _bits_eq(out, want), (step, i)
            if ef:
                assert _bits_eq(state.error_buffer(i, t), e1[i]), (step, i)
                assert _bits_eq(state.mean_error_buffer(i, n, t.device), e2[i]), (step, i)
    assert variant != "ef_coarse_mean" or all(np.any(e) for e in e2)


# ---------------------------------------------------------------------------------------------- multi-process
def _host_staged_codec():
    from test_gpu_exchange import HostStagedDeviceCodec

    class HostStagedMeanCodec(HostStagedDeviceCodec):
        def decode_mean_encode(self, streams, stream_words, nstreams, n, params, index=None, index_words=0,
                               index_stride=0, out_params=None, err=None, out_index_stride=0, slot=None):
            w, b, i = self.d.decode_mean_encode(streams.cuda(), stream_words, nstreams, n, params,
                                                index.cuda() if index is not None else None, index_words,
                                                index_stride, out_params=out_params, err=err,
                                                out_index_stride=out_index_stride, slot=slot)
            self.calls.append("decode_mean_encode")
            return w.cpu(), b.cpu(), (i.cpu() if i is not None else None)

    return HostStagedMeanCodec()


MP_N = 4 * (2 * 64 + 20) + 3  # world 3: two full 64-block shards and a ragged one ending in a partial block


def _mp_worker(rank, world, port, q):
    import torch.distributed as dist
    for p in (ROOT, os.path.join(ROOT, "tests")):
        if p not in sys.path:
            sys.path.insert(0, p)
    dist.init_process_group("gloo", init_method=port, rank=rank, world_size=world)  # a file:// rendezvous
    try:
        from gcow_amd import codec, ddp
        from gcow_amd import dist as gdist
        from mean_codec import mean_of
        from oracle import oracle as O
        bad = None
        for mode, p in (("rate16", codec.rate(16, 1)), ("acc1e-3", codec.accuracy(1e-3))):
            op = O.expert(*p.tuple())
            cdc = _host_staged_codec()
            state = ddp.make_hook_state(hook=ddp.compressed_sharded_hook, params=p, codec=cdc, compress_mean=True)
            grads = [O.gen_normal(MP_N, 1e-3, 40 + r, True) for r in range(world)]
            m = mean_of([O.decompress(O.compress(g, op)[0], (MP_N,), op) for g in grads])
            want = np.zeros(MP_N, np.float32)
            bounds = gdist.shard_plan(MP_N, world)[0]
            for lo, hi in bounds:
                want[lo:hi] = O.decompress(O.compress(m[lo:hi], op)[0], (hi - lo,), op)
            out = ddp.compressed_sharded_hook(state, _Bucket(torch.from_numpy(grads[rank].copy()), 0)).wait()
            got = (out[0] if isinstance(out, (list, tuple)) else out).numpy()
            allg = [torch.empty(MP_N) for _ in range(world)]
            dist.all_gather(allg, torch.from_numpy(got.copy()))
            if not np.array_equal(got.view(np.uint32), want.view(np.uint32)):
                bad = bad or "%s: bucket != the model's" % mode
            if any(not np.array_equal(t.numpy().view(np.uint32), got.view(np.uint32)) for t in allg):
                bad = bad or "%s: ranks hold different bits" % mode
            lo, hi = bounds[rank]
            if ("decode_mean_encode" in cdc.calls) != (hi > lo) or "decode_mean" in cdc.calls:
                bad = bad or "%s: codec calls %r" % (mode, cdc.calls)
        q.put((rank, True if bad is None else bad))
    except Exception as ex:  # pragma: no cover
        q.put((rank, repr(ex)))
    finally:
        dist.destroy_process_group()


def test_compress_mean_multiprocess_device_codec_world3(gc):
    """Three processes sharing the one GPU, every codec call on the gfx950 kernels, the collectives over gloo: rate 16
    and accuracy 1e-3, a ragged last shard; all ranks hold identical bits, equal to the model."""
    import torch.multiprocessing as mp
    from gcow_amd import dist as gdist
    assert [hi - lo for lo, hi in gdist.shard_plan(MP_N, 3)[0]] == [256, 256, 83]
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    with tempfile.TemporaryDirectory() as d:  # a file rendezvous: no port to race other jobs on the box for
        init = "file://" + os.path.join(d, "rdv")
        procs = [ctx.Process(target=_mp_worker, args=(r, 3, init, q)) for r in range(3)]
        for pr in procs:
            pr.start()
        try:
            res = [q.get(timeout=100) for _ in procs]
        finally:
            for pr in procs:
                pr.join(timeout=60)
                if pr.is_alive():
                    pr.kill()
    assert all(ok is True for _, ok in res), res
