"""The segmented codec (include/gcow.h "Segmented fields") as far as it can be checked without a GPU:

  1. the expectation itself (tests/segmented_inputs.py): with equal words and every n_s a multiple of 4 the bit
     concatenation reproduces O.compress of the concatenated bucket, and the oracle decodes every tensor back from the
     concatenated stream at its bit position;
  2. the plan through the C ABI: vb0 / off / n of every tensor and the tile words against a numpy restatement on all
     four lists, the size bound and used_bytes, one plan per shape whatever the dtype's alignment;
  3. every refusal that returns before a launch (the pointers are fake and never dereferenced);
  4. compressed_allgather_hook with per_tensor_budget over gloo at worlds 2 and 3 with an oracle-backed codec that
     implements encode_per_tensor / decode_mean_per_tensor: every rank ends with the model's mean bit for bit, each
     rank's stream is within its budget, and the records on the wire are each rank's own."""
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

INVALID, CAPACITY, UNSUPPORTED = 1, 2, 5
NEW = {"gcow_seg_plan_bytes": 2, "gcow_seg_plan": 6, "gcow_seg_plan_stats": 3, "gcow_seg_plan_segment": 6,
       "gcow_seg_plan_tile": 5, "gcow_encode_seg_max_output_bytes": 2, "gcow_encode_seg_workspace_bytes": 2,
       "gcow_encode_seg_index_entries": 3, "gcow_encode_seg_device": 15, "gcow_decode_mean_seg_device": 17}
TARGET, MAXPREC = 6.0, 64


def test_symbols_exported_and_declared():
    from gcow_amd import _ffi
    L = _ffi.load()
    declared = _ffi.header_functions()
    for name, nargs in NEW.items():
        assert hasattr(L, name), name
        assert name in declared, name
        assert len(getattr(L, name).argtypes) == nargs, name


def test_python_entry_points():
    from gcow_amd import codec, dist as gdist
    for name in ("SegmentPlan", "SegmentedEncoder", "encode_segmented", "decode_mean_segmented",
                 "PerTensorFittedEncoder"):
        assert hasattr(codec, name), name
    for name in ("encode_per_tensor", "decode_mean_per_tensor"):
        assert hasattr(gdist.DeviceCodec, name), name


# ------------------------------------------------------------------------------------------------ 1. the expectation
def test_concatenation_of_whole_block_tensors_is_the_plain_stream(orc):
    import segmented_inputs as SI
    rng = np.random.default_rng(5)
    sizes = [4, 64, 0, 8, 4096, 12]
    ts = [(rng.standard_normal(n) * 2.0 ** int(rng.integers(-20, 4))).astype(np.float32) for n in sizes]
    for minexp in (-154, -30, 133):
        p = orc.expert(1, 16658, 64, minexp)
        out, total, starts = SI.concat_bits([orc.compress(t, p) for t in ts if t.size])
        w, bits = orc.compress(np.concatenate(ts), p)
        assert total == bits and np.array_equal(out, w)
        assert starts[0] == 0 and all(a < b for a, b in zip(starts, starts[1:]))


@pytest.mark.parametrize("bf16", [False, True], ids=["fp32", "bf16"])
@pytest.mark.parametrize("name", ["edges", "special", "hook"])
def test_oracle_decodes_every_tensor_at_its_bit_position(orc, name, bf16):
    import segmented_inputs as SI
    words, total, pos, dec = SI.stream(name, bf16, "alt")
    ws = SI.words(name, bf16, "alt")
    w = np.concatenate([words, np.zeros(2, np.uint64)])
    cnts = SI.counts(name)
    vb0, off, _, _, nvb, nvals = SI.plan_model(cnts)
    assert pos.size == nvb and dec.size == nvals and (total + 63) // 64 == words.size
    for s, n in enumerate(cnts):
        if not n:
            continue
        p = orc.expert(1, 16658, 64, SI.clamp(ws[s]))
        d = np.zeros(n, np.float32)
        dims, nn = orc._shape((n,))
        end = orc.lib().orc_decompress_at(orc._p(d, orc.C.c_float), dims, nn, None, orc.C.byref(p),
                                          orc._p(w, orc.C.c_uint64), len(w), int(pos[vb0[s]]))
        assert np.array_equal(d.view(np.uint32), dec[off[s]:off[s] + n].view(np.uint32)), s
        nxt = vb0[s] + (n + 3) // 4
        assert end == (int(pos[nxt]) if nxt < nvb else total), s


# ------------------------------------------------------------------------------------------------ 2. the plan
@pytest.mark.parametrize("name", ["edges", "small", "special", "hook"])
def test_plan_against_the_restatement(name):
    import segmented_inputs as SI
    from gcow_amd import codec
    cnts = SI.counts(name)
    vb0, off, n, tiles, nvb, nvals = SI.plan_model(cnts)
    for dtype in (torch.float32, torch.bfloat16):
        pl = codec.SegmentPlan(cnts, dtype)
        st = pl.stats()
        assert (st.total_values, st.virtual_blocks, st.tiles) == (nvals, nvb, len(tiles))
        assert st.segments == sum(1 for c in cnts if c) and st.uniform_tiles == sum(1 for _, u in tiles if u)
        assert st.used_bytes == pl.used <= pl.L.gcow_seg_plan_bytes(len(cnts), nvals) and pl.used % 8 == 0
        nxt_vb, nxt_off = nvb, nvals  # an empty tensor reports the next non-empty one's
        want = [None] * len(cnts)
        for s in range(len(cnts) - 1, -1, -1):
            if cnts[s]:
                nxt_vb, nxt_off = vb0[s], off[s]
            want[s] = (nxt_vb, nxt_off, cnts[s])
        for s in range(len(cnts)):
            assert pl.segment(s) == want[s], s
        for t, (seg, uni) in enumerate(tiles):
            assert pl.tile(t) == (seg, uni), t
        assert pl.max_output_bytes() == (nvb * 140 + 63) // 64 * 8 + 8
        assert pl.workspace_bytes() > 0 and pl.workspace_bytes() % 8 == 0
        assert [pl.index_entries(k) for k in (0, 1, 8, 16, 256)] == [0, nvb, (nvb + 7) // 8, (nvb + 15) // 16,
                                                                     (nvb + 255) // 256]
    if name == "edges":  # 49 181 values: 13 tiles, seams inside tiles, and whole tiles of one tensor
        assert len(tiles) == 13 and 0 < sum(1 for _, u in tiles if u) < 13


def test_plan_is_the_same_for_both_dtypes_but_for_the_dtype_word():
    from gcow_amd import codec
    a = codec.SegmentPlan([5, 0, 4100], torch.float32)
    b = codec.SegmentPlan([5, 0, 4100], torch.bfloat16)
    ha, hb = a.h.numpy().copy(), b.h.numpy().copy()
    assert a.used == b.used and not np.array_equal(ha[:1], hb[:1]) and np.array_equal(ha[1:], hb[1:])


def test_empty_plans():
    from gcow_amd import codec
    for cnts in ([], [0], [0, 0, 0]):
        pl = codec.SegmentPlan(cnts, torch.float32)
        st = pl.stats()
        assert (st.total_values, st.virtual_blocks, st.tiles, st.segments) == (0, 0, 0, 0)
        assert pl.index_entries(16) == 0
        for s in range(len(cnts)):
            assert pl.segment(s) == (0, 0, 0)


# ------------------------------------------------------------------------------------------------ 3. refusals
def _plan(cnts, dtype=None):
    from gcow_amd import _ffi
    L = _ffi.load()
    n = len(cnts)
    need = L.gcow_seg_plan_bytes(n, sum(cnts))
    buf = (C.c_uint64 * ((need + 7) // 8))()
    used = C.c_size_t(0)
    arr = (C.c_uint64 * max(n, 1))(*cnts)
    st = L.gcow_seg_plan(arr, n, _ffi.DTYPE_FLOAT if dtype is None else dtype, buf, need, C.byref(used))
    return st, buf, used.value


def test_plan_refusals():
    from gcow_amd import _ffi
    L = _ffi.load()
    cnts = [5, 0, 4100]
    arr = (C.c_uint64 * 3)(*cnts)
    need = L.gcow_seg_plan_bytes(3, sum(cnts))
    buf = (C.c_uint64 * (need // 8 + 1))()
    used = C.c_size_t(0)
    assert L.gcow_seg_plan(arr, 3, _ffi.DTYPE_FLOAT, buf, need, C.byref(used)) == 0 and used.value <= need
    tmp = (C.c_uint64 * (need // 8 + 1))()  # the refused (and the empty) plans go here: buf keeps the good one
    assert L.gcow_seg_plan(arr, 3, _ffi.DTYPE_FLOAT, None, need, None) == INVALID
    assert L.gcow_seg_plan(None, 3, _ffi.DTYPE_FLOAT, tmp, need, None) == INVALID
    assert L.gcow_seg_plan(None, 0, _ffi.DTYPE_FLOAT, tmp, need, None) == 0          # an empty list needs no counts
    assert L.gcow_seg_plan(arr, 3, _ffi.DTYPE_DOUBLE, tmp, need, None) == UNSUPPORTED
    assert L.gcow_seg_plan(arr, 3, _ffi.DTYPE_INT32, tmp, need, None) == UNSUPPORTED
    assert L.gcow_seg_plan(arr, 3, _ffi.DTYPE_FLOAT, tmp, used.value - 8, None) == INVALID
    assert L.gcow_seg_plan(arr, 3, _ffi.DTYPE_FLOAT, C.c_void_p(C.addressof(tmp) + 4), need, None) == INVALID
    big = (C.c_uint64 * 2)((1 << 33), (1 << 33))                                     # 2^32 virtual blocks
    assert L.gcow_seg_plan(big, 2, _ffi.DTYPE_FLOAT, tmp, need, None) == UNSUPPORTED
    assert "2^32" in L.gcow_last_error().decode()
    one = (C.c_uint64 * 1)(1 << 34)
    assert L.gcow_seg_plan(one, 1, _ffi.DTYPE_FLOAT, tmp, need, None) == UNSUPPORTED
    # the queries and the readers refuse what is no plan
    junk = (C.c_uint64 * 16)()
    for q in (L.gcow_encode_seg_max_output_bytes, L.gcow_encode_seg_workspace_bytes):
        assert q(None, 128) == 0 and q(junk, 128) == 0 and q(buf, 8) == 0 and q(buf, used.value) > 0
    assert L.gcow_encode_seg_index_entries(junk, 128, 16) == 0
    stats = _ffi.SegStats()
    assert L.gcow_seg_plan_stats(junk, 128, C.byref(stats)) == INVALID
    assert L.gcow_seg_plan_stats(buf, used.value - 8, C.byref(stats)) == INVALID
    assert L.gcow_seg_plan_stats(buf, used.value, None) == INVALID
    a, b, c, u = C.c_uint64(), C.c_uint64(), C.c_uint64(), C.c_int()
    assert L.gcow_seg_plan_segment(buf, used.value, 3, C.byref(a), C.byref(b), C.byref(c)) == INVALID
    assert L.gcow_seg_plan_tile(buf, used.value, 2, C.byref(a), C.byref(u)) == INVALID


def test_encode_refusals():
    from gcow_amd import _ffi
    L = _ffi.load()
    st, plan, used = _plan([5, 0, 4100])
    assert st == 0
    DP, X, M, OUT, BITS, WS, IDX = 0x10000, 0x20000, 0x30000, 0x40000, 0x50000, 0x60000, 0x70000
    cap = L.gcow_encode_seg_max_output_bytes(plan, used)
    wsb = L.gcow_encode_seg_workspace_bytes(plan, used)

    def call(h=plan, hb=used, d=DP, x=X, maxprec=64, m=M, ms=1, out=OUT, c=cap, bits=BITS, ws=WS, wb=wsb, idx=None,
             stride=0):
        return L.gcow_encode_seg_device(h, d, hb, x, maxprec, m, ms, out, c, bits, ws, wb, idx, stride, None)

    junk = (C.c_uint64 * 16)()
    assert call(h=None) == INVALID and call(h=junk, hb=128) == INVALID and call(hb=used - 8) == INVALID
    assert call(d=None) == INVALID and call(d=DP + 4) == INVALID
    assert call(x=None) == INVALID and call(x=X + 2) == INVALID
    assert call(m=None) == INVALID and call(m=M + 2) == INVALID and call(ms=0) == INVALID
    assert call(out=None) == INVALID and call(out=OUT + 4) == INVALID
    assert call(c=cap - 8) == CAPACITY
    assert call(bits=BITS + 4) == INVALID
    assert call(ws=None) == INVALID and call(ws=WS + 4) == INVALID and call(wb=wsb - 8) == INVALID
    assert call(idx=IDX + 4, stride=16) == INVALID
    for bad in (0, 3, 24, 512):
        assert call(idx=IDX, stride=bad) == INVALID
    st, bplan, bused = _plan([5, 0, 4100], _ffi.DTYPE_BF16)
    assert call(h=bplan, hb=bused, x=X + 1) == INVALID  # bf16: element alignment is 2 bytes
    # an empty list and no bit count: nothing to do, nothing launched
    st, eplan, eused = _plan([0, 0])
    assert call(h=eplan, hb=eused, d=None, x=None, m=None, out=None, c=0, bits=None, ws=None, wb=0) == 0


def test_decode_mean_refusals():
    from gcow_amd import _ffi
    L = _ffi.load()
    st, plan, used = _plan([5, 0, 4100])
    DP, M, S, IDX, OUT = 0x10000, 0x30000, 0x40000, 0x70000, 0x80000
    nvb = 2 + 1025
    iw = (nvb + 15) // 16
    sw = 100

    def call(h=plan, hb=used, d=DP, maxprec=64, m=M, ms=4, mss=12, s=S, sb=(2 * sw + 2) * 8, words=sw, n=2, idx=IDX,
             iwords=iw, stride=16, out=OUT, odt=_ffi.DTYPE_FLOAT):
        return L.gcow_decode_mean_seg_device(h, d, hb, maxprec, m, ms, mss, s, sb, words, n, idx, iwords, stride, out,
                                             odt, None)

    junk = (C.c_uint64 * 16)()
    assert call(h=None) == INVALID and call(h=junk, hb=128) == INVALID and call(hb=used - 8) == INVALID
    assert call(d=None) == INVALID and call(d=DP + 4) == INVALID
    assert call(m=None) == INVALID and call(m=M + 2) == INVALID and call(ms=0) == INVALID
    assert call(s=None) == INVALID and call(s=S + 4) == INVALID and call(n=0) == INVALID
    assert call(sb=(2 * sw + 1) * 8) == INVALID                     # the two words after the last slot
    assert call(idx=None) == INVALID and call(idx=IDX + 4) == INVALID and call(iwords=iw - 1) == INVALID
    for bad in (0, 4, 32, 0x1010):                                  # 8 or 16; the packed16 index is not taken
        assert call(stride=bad) == INVALID
    assert call(iwords=(nvb + 7) // 8 - 1, stride=8) == INVALID
    assert call(out=None) == INVALID and call(out=OUT + 2) == INVALID
    assert call(out=OUT + 1, odt=_ffi.DTYPE_BF16) == INVALID
    assert call(odt=_ffi.DTYPE_DOUBLE) == UNSUPPORTED
    st, eplan, eused = _plan([0])
    assert call(h=eplan, hb=eused, d=None, m=None, s=None, idx=None, out=None) == 0  # an empty list does nothing


# ------------------------------------------------------------------------------------------------ 4. the hook, gloo
class _Bucket:
    """The GradBucket methods the hook uses; the gradients are views that tile the buffer in order."""

    def __init__(self, t, sizes, i=0):
        self.t, self.sizes, self.i = t, list(sizes), i

    def buffer(self):
        return self.t

    def index(self):
        return self.i

    def gradients(self):
        return list(torch.split(self.t, self.sizes))


def _oracle_per_tensor_codec():
    import fitted_per_tensor_inputs as FP
    import segmented_inputs as SI
    from oracle import oracle as O
    from oracle_codec import OracleCodec, _np_values, _u64
    from rate_table_inputs import oracle_table

    class OraclePerTensorCodec(OracleCodec):
        """encode_per_tensor / decode_mean_per_tensor from the definition: per-tensor oracle tables, the fit rule with
        the floor, per-tensor oracle streams concatenated bit by bit; the decode of tensor s of stream r under record
        (r, s) at the bit position the records' lengths give."""

        def encode_per_tensor(self, x, counts, bits_per_value, maxprec=64, index_stride=0, slot=None):
            a = _np_values(x)
            recs, pieces, lens = [], [], []
            o = 0
            for n in counts:
                t = a[o:o + n]
                o += n
                if not n:
                    recs.append(FP.fit_floor(np.zeros(288, np.int64), 0, FP.FLOOR))
                    continue
                rec = FP.fit_floor(oracle_table(t, maxprec), FP.budget_of(bits_per_value, n), FP.FLOOR)
                p = O.expert(1, 16658, maxprec, rec[0])
                w, b = O.compress(t, p)
                assert b == rec[2]
                recs.append(rec)
                pieces.append((w, b))
                lens.append(O.block_bits(t, p).astype(np.uint64))
            words, total, _ = SI.concat_bits(pieces)
            lens = np.concatenate(lens)
            pos = np.concatenate([[0], np.cumsum(lens)[:-1]]).astype(np.uint64)
            index = torch.from_numpy(pos[::index_stride].view(np.int64).copy()) if index_stride else None
            self.records.append(("encode_per_tensor", recs, total))
            fits = torch.from_numpy(FP.records_array(recs))
            wt = torch.from_numpy(np.concatenate([words, np.zeros(2, np.uint64)]).view(np.int64).copy())
            return wt, torch.tensor([total], dtype=torch.int64), index, fits

        def decode_mean_per_tensor(self, streams, stream_words, nstreams, counts, fits, maxprec=64, index=None,
                                   index_words=0, index_stride=16, out=None, slot=None):
            import mean_codec
            s = _u64(streams)
            S = len(counts)
            f = fits.numpy().reshape(nstreams, S, 2)
            decs = []
            for r in range(nstreams):
                w = np.concatenate([s[r * stream_words:(r + 1) * stream_words], np.zeros(2, np.uint64)])
                ix = index.numpy()[r * index_words:(r + 1) * index_words].view(np.uint64)
                d = np.zeros(sum(counts), np.float32)
                bit, o, vb = 0, 0, 0
                for k, n in enumerate(counts):
                    if not n:
                        continue
                    me = int(np.int32(f[r, k, 0] & 0xFFFFFFFF))
                    if vb % index_stride == 0:
                        assert int(ix[vb // index_stride]) == bit  # the gathered index agrees with the records
                    p = O.expert(1, 16658, maxprec, SI.clamp(me))
                    t = np.zeros(n, np.float32)
                    dims, nn = O._shape((n,))
                    end = O.lib().orc_decompress_at(O._p(t, O.C.c_float), dims, nn, None, O.C.byref(p),
                                                    O._p(w, O.C.c_uint64), len(w), bit)
                    assert end - bit == int(f[r, k, 1])  # the record's bit count is the tensor's stream length
                    d[o:o + n] = t
                    bit, o, vb = int(end), o + n, vb + (n + 3) // 4
                decs.append(d)
            m = mean_codec.mean_of(decs)
            self.records.append(("decode_mean_per_tensor", nstreams, f.copy()))
            got = torch.from_numpy(m)
            out.copy_(got.to(out.dtype))
            return out

    return OraclePerTensorCodec


def _rank_data(world):
    import relative_inputs as RI
    base = RI.tensors("hook", False)
    out = []
    for r in range(world):
        rng = np.random.default_rng(100 + r)
        out.append([(t * np.float32(2.0 ** (r - 1)) + (rng.standard_normal(t.size) * 1e-6).astype(np.float32))
                    .astype(np.float32) for t in base])
    return out


def _hook_worker(rank, world, port, q):
    _init(rank, world, port)
    try:
        import fitted_per_tensor_inputs as FP
        import mean_codec
        from gcow_amd import codec, ddp
        from oracle import oracle as O
        from rate_table_inputs import oracle_table
        data = _rank_data(world)
        sizes = [t.size for t in data[0]]
        cdc = _oracle_per_tensor_codec()()
        hook = ddp.compressed_allgather_hook
        state = ddp.make_hook_state(hook=hook, params=codec.accuracy(1e-3), codec=cdc, target_bits=TARGET,
                                    per_tensor_budget=True)
        g = torch.from_numpy(np.concatenate(data[rank]).copy())
        hook(state, _Bucket(g, sizes)).wait()
        # the model: every rank's tensors under that rank's own fits, averaged in rank order
        decs, recs_all = [], []
        for r in range(world):
            d, recs = [], []
            for t in data[r]:
                rec = FP.fit_floor(oracle_table(t, MAXPREC), FP.budget_of(TARGET, t.size), FP.FLOOR)
                p = O.expert(1, 16658, MAXPREC, rec[0])
                d.append(O.decompress(O.compress(t, p)[0], (t.size,), p))
                recs.append(rec)
            decs.append(np.concatenate(d))
            recs_all.append(recs)
        want = mean_codec.mean_of(decs)
        assert np.array_equal(g.numpy().view(np.uint32), want.view(np.uint32))
        mine = recs_all[rank]
        assert all(st == 0 for _, st, _ in mine)
        sent = cdc.records[0][2]
        assert sent == sum(b for _, _, b in mine) <= sum(FP.budget_of(TARGET, n) for n in sizes)
        assert np.array_equal(state.fit_record(0).numpy(), FP.records_array(mine))
        wire = cdc.records[-1][2]  # what the decode saw: every rank's records, in rank order
        assert np.array_equal(wire, np.stack([FP.records_array(r) for r in recs_all]))
        assert len({tuple(m for m, _, _ in r) for r in recs_all}) == world  # the ranks do code under different words
        q.put((rank, True))
    except Exception as ex:  # pragma: no cover - reported through the queue
        import traceback
        q.put((rank, repr(ex) + traceback.format_exc()))
    finally:
        dist.destroy_process_group()


@pytest.mark.parametrize("world", [2, 3])
def test_allgather_hook_per_tensor_budget(orc, world):
    _run(_hook_worker, world)


def test_hook_refusals(orc):
    """Raised before any codec call or collective: no process group here."""
    from gcow_amd import codec, ddp
    from oracle_codec import OracleCodec
    acc = codec.accuracy(1e-3)
    full = _oracle_per_tensor_codec()()
    S = ddp.GcowHookState
    t = torch.zeros(64)
    b = _Bucket(t, [60, 4])
    ok = dict(params=acc, codec=full, target_bits=8.0, per_tensor_budget=True)
    hook = ddp.compressed_allgather_hook
    with pytest.raises(ValueError, match="per_tensor_budget"):
        hook(S(**dict(ok, codec=OracleCodec())), b)
    with pytest.raises(ValueError, match="error_feedback"):
        hook(S(**dict(ok, error_feedback=True)), b)
    with pytest.raises(ValueError, match="compress_mean"):
        hook(S(**dict(ok, compress_mean=True)), b)
    with pytest.raises(ValueError, match="relative_bits"):
        hook(S(**dict(ok, relative_bits=8)), b)
    with pytest.raises(ValueError, match="target_bits"):
        hook(S(**dict(ok, target_bits=None)), b)
    with pytest.raises(ValueError, match="per_tensor_budget"):
        ddp.compressed_sharded_hook(S(**dict(ok, sharded=True)), b)
    with pytest.raises(ValueError, match="relative_bits"):
        hook(S(params=acc, codec=full, relative_bits=8), b)
    assert not full.records
    # with a process group the layout checks run; without one the hook says so first
    with pytest.raises(ValueError, match="process group"):
        hook(S(**ok), b)


def test_bucket_layout_check():
    from gcow_amd import ddp
    t = torch.zeros(64)
    assert ddp._bucket_counts(_Bucket(t, [60, 0, 4]), t) == [60, 0, 4]

    class Odd(_Bucket):
        def __init__(self, t, grads):
            super().__init__(t, [])
            self.g = grads

        def gradients(self):
            return self.g

    with pytest.raises(ValueError, match="tile"):
        ddp._bucket_counts(Odd(t, [t[4:64], t[0:4]]), t)        # out of order
    with pytest.raises(ValueError, match="cover"):
        ddp._bucket_counts(Odd(t, [t[0:60]]), t)                # a tail left out
    with pytest.raises(ValueError, match="tile"):
        ddp._bucket_counts(Odd(t, [t[0:60:2], t[60:64]]), t)    # a strided view
    with pytest.raises(ValueError, match="tile"):
        ddp._bucket_counts(Odd(t, [torch.zeros(60), t[60:64]]), t)  # a gradient that lies elsewhere
