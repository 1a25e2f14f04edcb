"""Relative tolerance on the wire (include/gcow.h "Relative tolerance over a segmented field") as far as it can be
checked without a GPU:

  1. the symbol, its declaration and the Python entry points;
  2. every refusal of gcow_seg_rel_minexp_device that returns before a launch, and the empty list (the pointers are
     fake and never dereferenced);
  3. the check matrix of compressed_allgather_hook with relative_bits against a codec that records its calls: every
     refusal is a ValueError naming relative_bits and no codec call is made; the two cases other files pin are here too;
  4. the hook over gloo at worlds 2 and 3 with an oracle-backed codec that implements encode_relative,
     encode_residual_relative and decode_mean_per_tensor from the definition: every rank ends with the rank-order mean
     of every rank's per-tensor oracle decode under that rank's own words, the words the decode saw are all ranks' in
     rank order and differ between ranks, and with error_feedback, over two steps, the carried error is the model's."""
import ctypes as C
import os
import sys

import numpy as np
import pytest
import torch
import torch.distributed as dist

TESTS = os.path.dirname(os.path.abspath(__file__))
if TESTS not in sys.path:
    sys.path.insert(0, TESTS)

from test_dist_cpu import _init, _run  # noqa: E402
from test_segmented_cpu import _Bucket, _plan, _rank_data  # noqa: E402

INVALID = 1
K, MAXPREC = 8, 64


# ------------------------------------------------------------------------------------------------ 1. the surface
def test_symbol_exported_and_declared():
    from gcow_amd import _ffi
    L = _ffi.load()
    assert hasattr(L, "gcow_seg_rel_minexp_device")
    assert "gcow_seg_rel_minexp_device" in _ffi.header_functions()
    assert len(L.gcow_seg_rel_minexp_device.argtypes) == 10


def test_python_entry_points():
    from gcow_amd import codec, ddp, dist as gdist
    for name in ("relative_minexp_segmented", "PerTensorRelativeEncoder", "PerTensorRelativeResidualEncoder"):
        assert hasattr(codec, name), name
    for name in ("encode_relative", "encode_residual_relative", "decode_mean_per_tensor"):
        assert hasattr(gdist.DeviceCodec, name), name
    assert hasattr(ddp, "_allgather_relative")
    for bad in (-1, 25, 2.5, 8.0, True, None):  # the hook's test of an integer: no bool, no integral float
        assert not codec.valid_rel_bits(bad)
        with pytest.raises(codec.GcowError):
            codec.PerTensorRelativeEncoder(bad)
    assert all(codec.valid_rel_bits(k) for k in (0, 24, np.int64(8)))


# ------------------------------------------------------------------------------------------------ 2. refusals
def test_words_call_refusals():
    from gcow_amd import _ffi
    L = _ffi.load()
    st, plan, used = _plan([5, 0, 4100])
    assert st == 0
    DP, X, E, A, M = 0x10000, 0x20000, 0x30000, 0x40000, 0x50000

    def call(h=plan, hb=used, d=DP, x=X, e=E, k=8, a=A, m=M, ms=1):
        return L.gcow_seg_rel_minexp_device(h, d, hb, x, e, k, a, m, ms, None)

    junk = (C.c_uint64 * 16)()
    assert call(h=None) == INVALID and call(h=junk, hb=128) == INVALID and call(hb=used - 8) == INVALID
    assert call(k=25) == INVALID
    assert "24" in L.gcow_last_error().decode()
    assert call(a=None) == INVALID and call(a=A + 2) == INVALID
    assert call(m=None) == INVALID and call(m=M + 2) == INVALID and call(ms=0) == INVALID
    assert call(d=None) == INVALID and call(d=DP + 4) == INVALID
    assert call(x=None) == INVALID and call(x=X + 2) == INVALID
    assert call(e=E + 2) == INVALID
    st, bplan, bused = _plan([5, 0, 4100], _ffi.DTYPE_BF16)
    assert call(h=bplan, hb=bused, x=X + 1) == INVALID  # bf16: element alignment is 2 bytes
    # an empty list is accepted and writes nothing; rel_bits is still checked
    st, eplan, eused = _plan([])
    assert call(h=eplan, hb=eused, d=None, x=None, e=None, a=None, m=None, ms=0) == 0
    assert call(h=eplan, hb=eused, d=None, x=None, e=None, a=None, m=None, k=25) == INVALID


# ------------------------------------------------------------------------------------------------ 3. the hook's checks
class _Recording:
    """A codec with every method the relative path asks for; any call is recorded (none may happen)."""

    def __init__(self, without=()):
        self.records = []
        for name in ("encode_relative", "encode_residual_relative", "decode_mean_per_tensor"):
            if name not in without:
                setattr(self, name, self._rec(name))

    def _rec(self, name):
        def f(*a, **k):
            self.records.append(name)
            raise AssertionError("codec call %s" % name)
        return f


def test_hook_check_matrix(orc):
    """All before any codec call or collective: there is no process group here."""
    from gcow_amd import codec, ddp
    from test_segmented_cpu import _oracle_per_tensor_codec
    acc = codec.accuracy(1e-3)
    S = ddp.GcowHookState
    hook = ddp.compressed_allgather_hook
    b = _Bucket(torch.zeros(64), [60, 4])
    full = _Recording()

    def refused(bucket=b, **kw):
        kw.setdefault("codec", full)
        with pytest.raises(ValueError, match="relative_bits") as ei:
            hook(S(params=acc, relative_bits=kw.pop("relative_bits", K), **kw), bucket)
        return str(ei.value)

    # 1. the combinations
    assert "compress_mean" in refused(compress_mean=True)
    assert "target_bits" in refused(target_bits=8.0)
    assert "target_bits" in refused(target_bits=8.0, per_tensor_budget=True)
    assert "per_tensor_budget" in refused(per_tensor_budget=True)  # check_target: it wants target_bits
    # 2. the range, ahead of the codec's methods
    for bad in (-1, 25, 2.5, 8.0, True):
        assert "0..24" in refused(relative_bits=bad, codec=_Recording(without=("encode_relative",)))
    # 3. the codec, ahead of the process group
    assert "encode_relative" in refused(codec=_Recording(without=("encode_relative",)))
    assert "decode_mean_per_tensor" in refused(codec=_Recording(without=("decode_mean_per_tensor",)))
    lacks = _Recording(without=("encode_residual_relative",))
    assert "encode_residual_relative" in refused(codec=lacks, error_feedback=True)
    assert "process group" in refused(codec=lacks)  # without error feedback that codec will do
    # 4. the process group, ahead of dtype and layout
    assert "process group" in refused()
    assert "process group" in refused(error_feedback=True)
    assert "process group" in refused(bucket=_Bucket(torch.zeros(64, dtype=torch.float16), [60, 4]))
    for k in (0, 24):
        assert "process group" in refused(relative_bits=k)
    assert not full.records and not lacks.records
    # the sharded hook keeps refusing
    with pytest.raises(ValueError, match="relative_bits"):
        ddp.compressed_sharded_hook(S(params=acc, relative_bits=K, sharded=True, codec=full), b)
    # the two pinned cases: the default state (tests/test_gpu_roundtrip_rel.py, there on the device) ...
    for h in (hook, ddp.compressed_sharded_hook):
        with pytest.raises(ValueError, match="relative_bits"):
            h(S(relative_bits=8), _Bucket(torch.zeros(64), [64]))
    # ... and a codec that lacks the new methods (tests/test_segmented_cpu.py)
    old = _oracle_per_tensor_codec()()
    with pytest.raises(ValueError, match="relative_bits"):
        hook(S(params=acc, codec=old, target_bits=8.0, per_tensor_budget=True, relative_bits=8), b)
    with pytest.raises(ValueError, match="relative_bits"):
        hook(S(params=acc, codec=old, relative_bits=8), b)
    assert not old.records


def _layout_worker(rank, world, port, q):
    _init(rank, world, port)
    try:
        from gcow_amd import codec, ddp
        full = _Recording()
        state = ddp.GcowHookState(params=codec.accuracy(1e-3), codec=full, relative_bits=K)
        hook = ddp.compressed_allgather_hook
        t = torch.zeros(64)
        with pytest.raises(ValueError, match="relative_bits.*fp32 or bf16"):
            hook(state, _Bucket(t.to(torch.float16), [60, 4]))

        class Odd(_Bucket):
            def gradients(self):
                return [self.t[4:64], self.t[0:4]]

        with pytest.raises(ValueError, match="relative_bits.*tile"):
            hook(state, Odd(t, [60, 4]))
        assert not full.records
        q.put((rank, True))
    except Exception as ex:  # pragma: no cover - reported through the queue
        import traceback
        q.put((rank, repr(ex) + traceback.format_exc()))
    finally:
        dist.destroy_process_group()


def test_hook_dtype_and_layout_checks_with_a_process_group(orc):
    _run(_layout_worker, 1)


# ------------------------------------------------------------------------------------------------ 4. gloo runs
def _oracle_relative_codec():
    import mean_codec
    import relative_inputs as RI
    import segmented_inputs as SI
    from oracle import oracle as O
    from oracle_codec import OracleCodec, _np_values, _u64
    from residual_model import model_step, widen

    class OracleRelativeCodec(OracleCodec):
        """encode_relative / encode_residual_relative / decode_mean_per_tensor from the definition: per tensor the
        word minexp_of(absmax_of(y_s), k), y = x (+ e), the oracle stream of y_s under it (model_step with a carried
        error), the streams concatenated bit by bit; the decode of tensor s of stream r under word (r, s)."""

        def _encode(self, kind, x, err, counts, k, maxprec, index_stride):
            a = _np_values(x)
            e = err.numpy().copy() if err is not None else None
            mx, pieces, lens, res = [], [], [], []
            o = 0
            for n in counts:
                t = a[o:o + n]
                es = e[o:o + n] if e is not None else np.zeros(n, np.float32)
                o += n
                with np.errstate(over="ignore", invalid="ignore"):
                    y0 = (widen(t) + es).astype(np.float32)
                m = RI.minexp_of(RI.absmax_of(y0), k)
                mx.append(m)
                if not n:
                    continue
                p = O.expert(1, 16658, maxprec, m)
                y, w, b, _, r = model_step(t, es, p)
                pieces.append((w, b))
                lens.append(O.block_bits(y, p).astype(np.uint64))
                res.append(r)
            words, total, _ = SI.concat_bits(pieces)
            lens = np.concatenate(lens)
            pos = np.concatenate([[0], np.cumsum(lens)[:-1]]).astype(np.uint64)
            index = torch.from_numpy(pos[::index_stride].view(np.int64).copy()) if index_stride else None
            if err is not None:
                err.copy_(torch.from_numpy(np.concatenate(res).astype(np.float32)))
            self.records.append((kind, list(mx), total))
            wt = torch.from_numpy(np.concatenate([words, np.zeros(2, np.uint64)]).view(np.int64).copy())
            return wt, torch.tensor([total], dtype=torch.int64), index, torch.tensor(mx, dtype=torch.int32)

        def encode_relative(self, x, counts, rel_bits, maxprec=64, index_stride=0, slot=None):
            return self._encode("encode_relative", x, None, counts, rel_bits, maxprec, index_stride)

        def encode_residual_relative(self, x, err, counts, rel_bits, maxprec=64, index_stride=0, slot=None):
            assert err.dtype == torch.float32 and err.numel() == x.numel()
            return self._encode("encode_residual_relative", x, err, counts, rel_bits, maxprec, index_stride)

        def roundtrip_relative(self, *a, **k):
            raise AssertionError("the wire hook does not round-trip")

        def decode_mean_per_tensor(self, streams, stream_words, nstreams, counts, fits, maxprec=64, index=None,
                                   index_words=0, index_stride=16, out=None, slot=None):
            s = _u64(streams)
            S = len(counts)
            assert fits.dtype == torch.int32 and fits.numel() == nstreams * S  # 4 bytes per tensor on the wire
            f = fits.numpy().reshape(nstreams, S)
            decs = []
            for r in range(nstreams):
                w = np.concatenate([s[r * stream_words:(r + 1) * stream_words], np.zeros(2, np.uint64)])
                ix = index.numpy()[r * index_words:(r + 1) * index_words].view(np.uint64)
                d = np.zeros(sum(counts), np.float32)
                bit, o, vb = 0, 0, 0
                for j, n in enumerate(counts):
                    if not n:
                        continue
                    if vb % index_stride == 0:
                        assert int(ix[vb // index_stride]) == bit  # the gathered index agrees with the stream
                    p = O.expert(1, 16658, maxprec, SI.clamp(int(f[r, j])))
                    t = np.zeros(n, np.float32)
                    dims, nn = O._shape((n,))
                    end = O.lib().orc_decompress_at(O._p(t, O.C.c_float), dims, nn, None, O.C.byref(p),
                                                    O._p(w, O.C.c_uint64), len(w), bit)
                    d[o:o + n] = t
                    bit, o, vb = int(end), o + n, vb + (n + 3) // 4
                decs.append(d)
            self.records.append(("decode_mean_per_tensor", nstreams, f.copy()))
            out.copy_(torch.from_numpy(mean_codec.mean_of(decs)).to(out.dtype))
            return out

    return OracleRelativeCodec


def _iteration_data(world, it):
    data = _rank_data(world)  # rank r's data scaled by 2^(r - 1)
    return data if it == 0 else [[np.ascontiguousarray(t[::-1]) for t in ts] for ts in data]


def _hook_worker(rank, world, port, q, feedback, default_params=False):
    _init(rank, world, port)
    try:
        import mean_codec
        import relative_inputs as RI
        from gcow_amd import codec, ddp
        from oracle import oracle as O
        from residual_model import model_step
        cdc = _oracle_relative_codec()()
        hook = ddp.compressed_allgather_hook
        # `params` contributes only its maxprec: the default fixed-rate set must do as well as a variable-rate one
        kw = {} if default_params else {"params": codec.accuracy(1e-3)}
        state = ddp.make_hook_state(hook=hook, codec=cdc, relative_bits=K, error_feedback=feedback, **kw)
        assert codec.is_fixed(state.params) == default_params and state.params.maxprec == MAXPREC
        carried = None  # the model's carried error of every rank, per tensor (zeros throughout without feedback)
        for it in range(2):
            data = _iteration_data(world, it)
            sizes = [t.size for t in data[0]]
            if carried is None or not feedback:
                carried = [[np.zeros(n, np.float32) for n in sizes] for _ in range(world)]
            g = torch.from_numpy(np.concatenate(data[rank]).copy())
            hook(state, _Bucket(g, sizes)).wait()
            decs, words_all = [], []
            for r in range(world):
                d, ws = [], []
                for s, t in enumerate(data[r]):
                    y0 = (t + carried[r][s]).astype(np.float32)
                    m = RI.minexp_of(RI.absmax_of(y0), K)
                    _, _, _, dec, res = model_step(t, carried[r][s], O.expert(1, 16658, MAXPREC, m))
                    d.append(dec)
                    ws.append(m)
                    carried[r][s] = res
                decs.append(np.concatenate(d))
                words_all.append(ws)
            want = mean_codec.mean_of(decs)
            assert np.array_equal(g.numpy().view(np.uint32), want.view(np.uint32)), it
            wire = cdc.records[-1][2]  # what the decode saw: every rank's words, in rank order
            assert wire.dtype == np.int32 and np.array_equal(wire, np.array(words_all, np.int32)), it
            assert len({tuple(w) for w in words_all}) == world  # the ranks do code under different words
            assert cdc.records[-2][1] == words_all[rank]
            if feedback:
                mine = np.concatenate(carried[rank])
                assert np.array_equal(state.error_buffer(0, g).numpy().view(np.uint32), mine.view(np.uint32)), it
                assert mine.any()
        kinds = [r[0] for r in cdc.records]
        enc = "encode_residual_relative" if feedback else "encode_relative"
        assert kinds == [enc, "decode_mean_per_tensor"] * 2
        if not feedback:
            assert not state._errors
        q.put((rank, True))
    except Exception as ex:  # pragma: no cover - reported through the queue
        import traceback
        q.put((rank, repr(ex) + traceback.format_exc()))
    finally:
        dist.destroy_process_group()


@pytest.mark.parametrize("world", [2, 3])
def test_allgather_hook_relative(orc, world):
    _run(_hook_worker, world, False)


@pytest.mark.parametrize("world", [2, 3])
def test_allgather_hook_relative_error_feedback(orc, world):
    _run(_hook_worker, world, True)


@pytest.mark.parametrize("feedback", [False, True], ids=["plain", "feedback"])
def test_allgather_hook_relative_default_params(orc, feedback):
    """The state's default `params` is fixed rate (rate 16): make_hook_state still creates the exchange group, and the
    hook runs as under a variable-rate set."""
    _run(_hook_worker, 2, feedback, True)
