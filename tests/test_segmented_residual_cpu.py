"""Error feedback under per-tensor budgets (include/gcow.h "Segmented fields with a residual") as far as it can be
checked without a GPU:

  1. the symbols, their declarations and every refusal of gcow_rate_table_seg_device, gcow_encode_seg_residual_device
     and the workspace query that returns before a launch (the pointers are fake and never dereferenced);
  2. compressed_allgather_hook with error_feedback and per_tensor_budget over gloo at worlds 2 and 3 over two
     iterations, with an oracle-backed codec whose encode_residual_per_tensor is written from the definition: every
     rank's bucket is the mean of the ranks' model decodes and its carried error its own model residual;
  3. the hook refusals: a codec without encode_residual_per_tensor (no codec call made), roundtrip_hook with
     error_feedback, compressed_sharded_hook with per_tensor_budget;
  4. the model helper's own assertions: the tables and fits of y differ from those of x.
Items 1 to 3 fail on a library or a package without the two calls and encode_residual_per_tensor; item 4 runs the
oracle and the test helper only, so it passes without the feature: it guards the expectations, not the code."""
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
from test_segmented_cpu import _Bucket, _oracle_per_tensor_codec, _rank_data  # noqa: E402

INVALID, CAPACITY, UNSUPPORTED = 1, 2, 5
NEW = {"gcow_rate_table_seg_workspace_bytes": 2, "gcow_rate_table_seg_device": 10,
       "gcow_encode_seg_residual_device": 17}
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
    for name in ("rate_tables_segmented", "SegmentedRateTables", "SegmentedResidualEncoder",
                 "encode_segmented_residual", "PerTensorFittedResidualEncoder"):
        assert hasattr(codec, name), name
    assert hasattr(gdist.DeviceCodec, "encode_residual_per_tensor")


# ------------------------------------------------------------------------------------------------ 1. host refusals
def _plan(counts, bf16=False):
    from gcow_amd import _ffi
    L = _ffi.load()
    ns = len(counts)
    need = L.gcow_seg_plan_bytes(ns, sum(counts))
    buf = (C.c_uint64 * ((need + 7) // 8))()
    used = C.c_size_t(0)
    cnt = (C.c_uint64 * max(ns, 1))(*counts)
    assert L.gcow_seg_plan(cnt, ns, _ffi.DTYPE_BF16 if bf16 else _ffi.DTYPE_FLOAT, buf, need, C.byref(used)) == 0
    return L, buf, used.value


def test_workspace_query():
    L, h, used = _plan([60, 0, 4])
    q = L.gcow_rate_table_seg_workspace_bytes
    w3 = q(h, used)
    assert w3 > 0 and w3 % 8 == 0
    assert q(None, used) == 0 and q(h, 8) == 0 and q(h, used - 8) == 0
    foreign = (C.c_uint64 * 64)()
    assert q(foreign, 512) == 0
    # a function of S only: other counts and another dtype, the same S
    L2, h2, used2 = _plan([1, 100000, 7], bf16=True)
    assert q(h2, used2) == w3
    _, h5, used5 = _plan([4] * 5)
    assert q(h5, used5) > w3
    # the encode's queries do not depend on the plan's dtype: the residual call takes the plan's own
    Lf, hf, uf = _plan([1, 100000, 7], bf16=False)
    for name in ("gcow_encode_seg_max_output_bytes", "gcow_encode_seg_workspace_bytes"):
        assert getattr(L, name)(h2, used2) == getattr(L, name)(hf, uf) > 0


def test_rate_table_seg_argument_checks():
    L, h, used = _plan([60, 0, 4])
    D, X, E, T, W = 0x10000, 0x20000, 0x30000, 0x40000, 0x50000  # fake device addresses
    wsb = L.gcow_rate_table_seg_workspace_bytes(h, used)

    def call(hp=h, nb=used, d=D, x=X, e=E, maxprec=64, t=T, w=W, wb=wsb):
        return L.gcow_rate_table_seg_device(hp, d, nb, x, e, maxprec, t, w, wb, None)

    assert call(hp=None) == INVALID
    assert call(nb=8) == INVALID
    assert call(hp=(C.c_uint64 * 64)(), nb=512) == INVALID     # foreign
    assert call(d=None) == INVALID
    assert call(d=D + 4) == INVALID
    assert call(x=None) == INVALID
    assert call(x=X + 2) == INVALID                             # fp32 x off 4 bytes
    assert call(e=E + 2) == INVALID                             # an error pointer off 4 bytes
    assert "d_err_in" in L.gcow_last_error().decode()
    assert call(t=None) == INVALID
    assert call(t=T + 4) == INVALID
    assert call(w=None) == INVALID
    assert call(w=W + 4) == INVALID
    assert call(wb=wsb - 8) == INVALID
    assert call(maxprec=65) != 0
    Lb, hb, ub = _plan([60, 0, 4], bf16=True)
    assert Lb.gcow_rate_table_seg_device(hb, D, ub, X + 1, E, 64, T, W, wsb, None) == INVALID  # bf16 x off 2 bytes
    # no tensors: nothing to write, no pointer needed
    L0, h0, u0 = _plan([])
    assert L0.gcow_rate_table_seg_device(h0, None, u0, None, None, 64, None, None, 0, None) == 0


def test_encode_seg_residual_argument_checks():
    L, h, used = _plan([60, 0, 4])
    D, X, EI, EO, M, OUT, BITS, WS, IX = (0x10000 * k for k in range(1, 10))
    cap = L.gcow_encode_seg_max_output_bytes(h, used)
    wsb = L.gcow_encode_seg_workspace_bytes(h, used)

    def call(hp=h, nb=used, d=D, x=X, ei=EI, eo=EO, maxprec=64, m=M, ms=1, out=OUT, c=cap, bits=BITS, ws=WS, wb=wsb,
             ix=None, stride=0):
        return L.gcow_encode_seg_residual_device(hp, d, nb, x, ei, eo, maxprec, m, ms, out, c, bits, ws, wb, ix, stride,
                                                 None)

    # gcow_encode_seg_device's refusals
    assert call(hp=None) == INVALID
    assert call(nb=8) == INVALID
    assert call(hp=(C.c_uint64 * 64)(), nb=512) == INVALID
    assert call(d=None) == INVALID and call(d=D + 4) == INVALID
    assert call(x=None) == INVALID and call(x=X + 2) == INVALID
    assert call(m=None) == INVALID and call(m=M + 2) == INVALID
    assert call(ms=0) == INVALID
    assert call(out=None) == INVALID and call(out=OUT + 4) == INVALID
    assert call(c=cap - 8) == CAPACITY
    assert call(bits=BITS + 4) == INVALID
    assert call(ws=None) == INVALID and call(ws=WS + 4) == INVALID
    assert call(wb=wsb - 8) == INVALID
    assert call(ix=IX, stride=3) == INVALID and call(ix=IX, stride=512) == INVALID and call(ix=IX + 4, stride=8) == INVALID
    assert call(maxprec=65) != 0
    # and the error arrays'
    assert call(eo=None) == INVALID
    assert "d_err_out" in L.gcow_last_error().decode()
    assert call(eo=EO + 2) == INVALID
    assert call(ei=EI + 2) == INVALID
    # an empty list and no bit count: nothing to write
    L0, h0, u0 = _plan([0, 0])
    assert L0.gcow_encode_seg_residual_device(h0, None, u0, None, None, None, 64, None, 1, None, 0, None, None, 0, None,
                                              0, None) == 0


# ------------------------------------------------------------------------------------------------ 2. gloo runs
def _oracle_residual_per_tensor_codec():
    import fitted_per_tensor_inputs as FP
    import segmented_inputs as SI
    from oracle import oracle as O
    from oracle_codec import _np_values
    from rate_table_inputs import oracle_table
    from residual_model import model_step, widen

    class OracleResidualPerTensorCodec(_oracle_per_tensor_codec()):
        """encode_residual_per_tensor from the definition: per tensor y = x + e, the oracle table of y, the fit rule
        with the floor, model_step under the fitted set; the streams concatenated bit by bit, err updated in place."""

        def encode_residual_per_tensor(self, x, err, counts, bits_per_value, maxprec=64, index_stride=0, slot=None):
            assert err.dtype == torch.float32 and err.numel() == x.numel()
            a, e = _np_values(x), err.numpy().copy()
            recs, pieces, lens, res = [], [], [], []
            o = 0
            for n in counts:
                t, es = a[o:o + n], e[o:o + n]
                o += n
                if not n:
                    recs.append(FP.fit_floor(np.zeros(288, np.int64), 0, FP.FLOOR))
                    continue
                y0 = (widen(t) + es).astype(np.float32)
                rec = FP.fit_floor(oracle_table(y0, maxprec), FP.budget_of(bits_per_value, n), FP.FLOOR)
                p = O.expert(1, 16658, maxprec, rec[0])
                y, w, b, _, r = model_step(t, es, p)
                assert b == rec[2]
                recs.append(rec)
                pieces.append((w, b))
                lens.append(O.block_bits(y, p).astype(np.uint64))
                res.append(r)
            words, total, _ = SI.concat_bits(pieces)
            lens = np.concatenate(lens)
            pos = np.concatenate([[0], np.cumsum(lens)[:-1]]).astype(np.uint64)
            index = torch.from_numpy(pos[::index_stride].view(np.int64).copy()) if index_stride else None
            err.copy_(torch.from_numpy(np.concatenate(res).astype(np.float32)))
            self.records.append(("encode_residual_per_tensor", recs, total))
            fits = torch.from_numpy(FP.records_array(recs))
            wt = torch.from_numpy(np.concatenate([words, np.zeros(2, np.uint64)]).view(np.int64).copy())
            return wt, torch.tensor([total], dtype=torch.int64), index, fits

    return OracleResidualPerTensorCodec


def _iteration_data(world, it):
    data = _rank_data(world)
    return data if it == 0 else [[np.ascontiguousarray(t[::-1]) for t in ts] for ts in data]


def _hook_worker(rank, world, port, q):
    _init(rank, world, port)
    try:
        import fitted_per_tensor_inputs as FP
        import mean_codec
        from gcow_amd import codec, ddp
        from oracle import oracle as O
        from rate_table_inputs import oracle_table
        from residual_model import model_step
        cdc = _oracle_residual_per_tensor_codec()()
        hook = ddp.compressed_allgather_hook
        state = ddp.make_hook_state(hook=hook, params=codec.accuracy(1e-3), codec=cdc, target_bits=TARGET,
                                    per_tensor_budget=True, error_feedback=True)
        carried = None  # the model's carried error of every rank, per tensor
        for it in range(2):
            data = _iteration_data(world, it)
            sizes = [t.size for t in data[0]]
            if carried is None:
                carried = [[np.zeros(n, np.float32) for n in sizes] for _ in range(world)]
            g = torch.from_numpy(np.concatenate(data[rank]).copy())
            hook(state, _Bucket(g, sizes)).wait()
            decs, recs_all = [], []
            for r in range(world):
                d, recs = [], []
                for s, t in enumerate(data[r]):
                    y0 = (t + carried[r][s]).astype(np.float32)
                    rec = FP.fit_floor(oracle_table(y0, MAXPREC), FP.budget_of(TARGET, t.size), FP.FLOOR)
                    _, _, b, dec, res = model_step(t, carried[r][s], O.expert(1, 16658, MAXPREC, rec[0]))
                    assert b == rec[2]
                    d.append(dec)
                    recs.append(rec)
                    carried[r][s] = res
                decs.append(np.concatenate(d))
                recs_all.append(recs)
            want = mean_codec.mean_of(decs)
            assert np.array_equal(g.numpy().view(np.uint32), want.view(np.uint32)), it
            mine = np.concatenate(carried[rank])
            assert np.array_equal(state.error_buffer(0, g).numpy().view(np.uint32), mine.view(np.uint32)), it
            assert mine.any()
            assert np.array_equal(state.fit_record(0).numpy(), FP.records_array(recs_all[rank]))
            wire = cdc.records[-1][2]  # what the decode saw: every rank's records, in rank order
            assert np.array_equal(wire, np.stack([FP.records_array(r) for r in recs_all]))
        kinds = [r[0] for r in cdc.records]
        assert kinds == ["encode_residual_per_tensor", "decode_mean_per_tensor"] * 2
        q.put((rank, True))
    except Exception as ex:  # pragma: no cover - reported through the queue
        import traceback
        q.put((rank, repr(ex) + traceback.format_exc()))
    finally:
        dist.destroy_process_group()


@pytest.mark.parametrize("world", [2, 3])
def test_allgather_hook_error_feedback_per_tensor(orc, world):
    _run(_hook_worker, world)


# ------------------------------------------------------------------------------------------------ 3. hook refusals
def test_hook_refusals(orc):
    """Raised before any codec call or collective: no process group here."""
    from gcow_amd import codec, ddp
    acc = codec.accuracy(1e-3)
    plain = _oracle_per_tensor_codec()()             # encode_per_tensor only
    full = _oracle_residual_per_tensor_codec()()
    S = ddp.GcowHookState
    b = _Bucket(torch.zeros(64), [60, 4])
    ok = dict(params=acc, target_bits=8.0, per_tensor_budget=True, error_feedback=True)
    with pytest.raises(ValueError) as ei:
        ddp.compressed_allgather_hook(S(codec=plain, **ok), b)
    for word in ("error_feedback", "per_tensor_budget", "encode_residual_per_tensor"):
        assert word in str(ei.value), word
    assert not plain.records
    with pytest.raises(ValueError, match="error_feedback"):
        ddp.roundtrip_hook(S(codec=full, **ok), b)
    with pytest.raises(ValueError, match="error_feedback"):
        ddp.roundtrip_hook(S(codec=full, params=acc, error_feedback=True), b)
    with pytest.raises(ValueError, match="per_tensor_budget"):
        ddp.compressed_sharded_hook(S(codec=full, sharded=True, **ok), b)
    with pytest.raises(ValueError, match="per_tensor_budget"):
        ddp.compressed_sharded_hook(S(codec=full, sharded=True, **dict(ok, error_feedback=False)), b)
    assert not full.records
    # with the method the combination is accepted: without a process group the hook says so, as before
    with pytest.raises(ValueError, match="process group"):
        ddp.compressed_allgather_hook(S(codec=full, **ok), b)
    state = S(codec=full, **ok)
    state.error_buffer(0, torch.zeros(64)).fill_(1.0)
    state.reset_error_feedback()
    assert not state.error_buffer(0, torch.zeros(64)).any()


# ------------------------------------------------------------------------------------------------ 4. the model helper
@pytest.mark.parametrize("name", ["edges", "hook", "special", "small"])
def test_model_tables_and_fits_of_y_differ_from_x(orc, name):
    import segmented_inputs as SI
    import segmented_residual_inputs as SR
    for bf16 in (False, True):
        rows, nfits = SR.check_differs(name, bf16)
        assert rows >= 1
        # step 1 carries nothing: its records are the "fit8" words, and step 2's error is its residual
        assert [r[0] for r in SR.fits_y(name, bf16, 0)] == list(SI.words(name, bf16, "fit8"))
        e = SR.e_bucket(name, bf16, 1)
        assert e.dtype == np.float32 and e.size == sum(SI.counts(name)) and np.isfinite(e).all() and e.any()
        assert np.array_equal(e.view(np.uint32), SR.model(name, bf16, 0, "fit8")[3].view(np.uint32))
    if name == "special":  # x + e overflows to Inf in one tensor
        xs = [SR.widen(t) for t in SI.variant(name, False, 1)]
        assert any((np.isinf(y) & np.isfinite(x)).any() for x, y in zip(xs, SR.y_tensors(name, False, 1)))
