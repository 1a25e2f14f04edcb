"""The bit budget per tensor without a device (include/gcow.h: gcow_rate_table_rel_workspace_bytes,
gcow_rate_table_rel_device, gcow_rate_table_fit_batch_device, gcow_roundtrip_rel_fitted_device): the symbols are
exported, declared and bound; the workspace query; every refusal the contract decides on the host returns its status
before any launch, over plans built from made-up addresses; the restated fit rule against rate_table_inputs.fit; the
hook option's ValueError combinations against a fake codec; and the conditions on the oracle's tables without which
the GPU tests could pass vacuously."""
import ctypes as C
import os
import sys

import pytest

TESTS = os.path.dirname(os.path.abspath(__file__))
if TESTS not in sys.path:
    sys.path.insert(0, TESTS)

from gcow_amd import _ffi  # noqa: E402
from gcow_amd._ffi import DTYPE_BF16, DTYPE_FLOAT  # noqa: E402

NAMES = ["gcow_rate_table_rel_workspace_bytes", "gcow_rate_table_rel_device", "gcow_rate_table_fit_batch_device",
         "gcow_roundtrip_rel_fitted_device"]
INVALID = 1
A = 1 << 40  # made-up device addresses: nothing below is ever dereferenced


@pytest.fixture(scope="module")
def L():
    return _ffi.load()


def _plan(L, sizes=(8192 * 3 + 5, 7, 0, 1024), in_dt=DTYPE_FLOAT, out_dt=DTYPE_FLOAT):
    from test_roundtrip_rel_cpu import make_plan
    ins = [A + (1 << 30) * k for k in range(len(sizes))]
    st, buf, used = make_plan(L, ins, None if in_dt == out_dt else [a + (1 << 36) for a in ins], list(sizes), in_dt,
                              out_dt)
    assert st == 0
    return buf, C.cast(buf, C.c_void_p), used


def test_symbols_exported_declared_and_bound(L):
    declared = _ffi.header_functions()
    for name in NAMES:
        assert name in declared, name
        f = getattr(L, name)
        assert f.argtypes is not None and len(f.argtypes) >= 2, name
    assert L.gcow_rate_table_rel_workspace_bytes.restype is C.c_size_t
    src = open(os.path.join(_ffi.HERE, "..", "include", "gcow.h")).read()
    assert "a table per tensor\n * is not offered" not in src


def test_workspace_query(L):
    import fitted_per_tensor_inputs as F
    buf, h, used = _plan(L)
    ws = L.gcow_rate_table_rel_workspace_bytes(h, used)
    assert ws == 4 * F.WS_WORDS * 8  # the two arrays and the block count per tensor, empty ones included
    # a function of nsegs only: other sizes, other dtypes, the same number of tensors
    buf2, h2, used2 = _plan(L, sizes=(1, 2, 3, 100000), in_dt=DTYPE_BF16, out_dt=DTYPE_FLOAT)
    assert L.gcow_rate_table_rel_workspace_bytes(h2, used2) == ws
    buf3, h3, used3 = _plan(L, sizes=(5,) * 9)
    assert L.gcow_rate_table_rel_workspace_bytes(h3, used3) == 9 * F.WS_WORDS * 8
    buf0, h0, used0 = _plan(L, sizes=())
    assert L.gcow_rate_table_rel_workspace_bytes(h0, used0) > 0
    assert L.gcow_rate_table_rel_workspace_bytes(None, used) == 0
    assert L.gcow_rate_table_rel_workspace_bytes(h, used - 8) == 0
    assert L.gcow_rate_table_rel_workspace_bytes(h, 16) == 0
    foreign = (C.c_uint64 * (used // 8 + 1))()
    assert L.gcow_rate_table_rel_workspace_bytes(C.cast(foreign, C.c_void_p), used) == 0
    # a plan of the list form is foreign here
    from gcow_amd._ffi import GcowParams
    from roundtrip_list_inputs import make_plan
    st, lbuf, lused = make_plan(L, [A], None, [64], DTYPE_FLOAT, DTYPE_FLOAT, GcowParams(1, 16658, 64, 0))
    assert st == 0 and L.gcow_rate_table_rel_workspace_bytes(C.cast(lbuf, C.c_void_p), lused) == 0


def _table(L, h, d_plan, nbytes, maxprec=64, tables=A, ws=A + (1 << 20), wsb=None):
    if wsb is None:
        wsb = 1 << 20
    return L.gcow_rate_table_rel_device(h, d_plan, nbytes, maxprec, tables, ws, wsb, None)


def _rt(L, h, d_plan, nbytes, maxprec=64, word=A, stride=4, total=A + 64):
    return L.gcow_roundtrip_rel_fitted_device(h, d_plan, nbytes, maxprec, word, stride, total, None)


@pytest.mark.parametrize("in_dt,out_dt", [(DTYPE_FLOAT, DTYPE_FLOAT), (DTYPE_BF16, DTYPE_FLOAT)])
def test_refusals_decided_on_the_host(L, in_dt, out_dt):
    buf, h, used = _plan(L, in_dt=in_dt, out_dt=out_dt)
    d = A + (1 << 24)
    wsb = L.gcow_rate_table_rel_workspace_bytes(h, used)
    foreign = (C.c_uint64 * (used // 8 + 1))()
    hf = C.cast(foreign, C.c_void_p)
    for call in (_table, _rt):
        assert call(L, None, d, used) == INVALID          # NULL h_plan
        assert call(L, h, d, used - 8) == INVALID         # short
        assert call(L, h, d, 16) == INVALID               # shorter than a header
        assert call(L, hf, d, used) == INVALID            # not a plan
        assert call(L, h, None, used) == INVALID          # NULL d_plan
        assert call(L, h, d + 4, used) == INVALID         # d_plan off 8 bytes
    assert _table(L, h, d, used, tables=None) == INVALID
    assert _table(L, h, d, used, tables=A + 4) == INVALID
    assert _table(L, h, d, used, ws=None) == INVALID
    assert _table(L, h, d, used, ws=A + 4100) == INVALID
    assert _table(L, h, d, used, wsb=wsb - 8) == INVALID
    assert _table(L, h, d, used, wsb=0) == INVALID
    assert b"workspace" in L.gcow_last_error()
    assert _rt(L, h, d, used, word=None) == INVALID
    assert _rt(L, h, d, used, word=A + 2) == INVALID
    assert b"d_minexp" in L.gcow_last_error()
    assert _rt(L, h, d, used, stride=0) == INVALID
    assert b"stride" in L.gcow_last_error()
    assert _rt(L, h, d, used, total=A + 68) == INVALID
    assert b"d_total_bits" in L.gcow_last_error()


def test_fit_batch_refusals(L):
    fit = L.gcow_rate_table_fit_batch_device
    T, B, R = A, A + (1 << 20), A + (1 << 21)
    assert fit(None, 3, B, -94, R, None) == INVALID
    assert fit(T + 4, 3, B, -94, R, None) == INVALID
    assert fit(T, 3, None, -94, R, None) == INVALID
    assert fit(T, 3, B + 4, -94, R, None) == INVALID
    assert fit(T, 3, B, -94, None, None) == INVALID
    assert fit(T, 3, B, -94, R + 4, None) == INVALID
    assert b"fit" in L.gcow_last_error()
    assert fit(None, 0, None, -94, None, None) == 0  # no table: nothing to do, nothing launched


def test_empty_list_without_a_bit_count_launches_nothing(L):
    buf, h, used = _plan(L, sizes=())
    assert _rt(L, h, None, used, word=None, total=None) == 0
    assert _table(L, h, None, used, tables=None, ws=None, wsb=0) == 0


def test_fit_restatement_agrees_with_the_single_fit(orc):
    import fitted_per_tensor_inputs as F
    from rate_table_inputs import fit
    for name, bf16 in (("edges", False), ("special", True)):
        T = F.tables(name, bf16, 64)
        for row in T:
            for budget in (0, int(row[287]) - 1, int(row[287]), int(row[200]), int(row[100]), int(row[0]), 1 << 62):
                got = fit(row, budget)
                want = (got[0], 0, got[1]) if got is not None else (133, 1, int(row[287]))
                assert F.fit_floor(row, budget, -154) == want
                assert F.fit_floor(row, budget, -1000) == want
                lo = F.fit_floor(row, budget, -94)
                assert lo[0] >= -94 and lo[0] >= want[0] and (lo[0] == want[0] or want[0] < -94)
    # a floor above the range: nothing fits
    assert F.fit_floor(T[0], 1 << 62, 134) == (133, 1, int(T[0][287]))


def test_inputs_cannot_pass_vacuously(orc):
    """On the oracle's tables: the edges list needs at least three different minexp at 8 bits per value (one global
    fit cannot pass); the floor moves the fit of the 1e-40 tensor; at 0.5 bits per value a tensor of one value has no
    entry that fits (status 1)."""
    import fitted_per_tensor_inputs as F
    from relative_inputs import tensors
    for bf16 in (False, True):
        rec = F.fits("edges", bf16, 64, 8.0, F.FLOOR)
        sizes = [t.size for t in tensors("edges", bf16)]
        assert len({r[0] for r, n in zip(rec, sizes) if n}) >= 3
        assert all(r[1] == 0 and r[2] <= F.budget_of(8.0, n) for r, n in zip(rec, sizes))
        assert rec[sizes.index(0)] == (F.FLOOR, 0, 0)  # an empty tensor: an all-zero row fits at the floor
        lo, hi = F.fits("special", bf16, 64, 8.0, -154), F.fits("special", bf16, 64, 8.0, -94)
        assert lo[3][0] < -94 and hi[3][0] == -94  # the tensor of scale 1e-40
        half = F.fits("edges", bf16, 64, 0.5, F.FLOOR)
        ones = [s for s, n in enumerate(sizes) if n == 1]
        assert ones and all(half[s] == (133, 1, 1) for s in ones)
        assert any(r[1] == 0 for r in half)


# ---------------------------------------------------------------------------------------------- the hook option
class _Bucket:
    def __init__(self, t, sizes):
        self.t, self.sizes = t, sizes

    def buffer(self):
        return self.t

    def index(self):
        return 0

    def gradients(self):
        out, at = [], 0
        for n in self.sizes:
            out.append(self.t[at:at + n])
            at += n
        return out


class _FakeCodec:
    """What check_fit_on_device and the hooks look for, and the per-tensor call; nothing here is ever run."""

    def roundtrip_fitted_per_tensor(self, *a, **k):
        raise AssertionError("the refusals come before any codec call")

    rate_table = fit_device = encode_fitted = roundtrip_fitted = roundtrip_relative = roundtrip_fitted_per_tensor


class _NoPerTensor:
    def roundtrip_relative(self, *a, **k):
        raise AssertionError


def test_hook_option_validation():
    import torch
    from gcow_amd import codec, ddp
    acc = codec.accuracy(1e-3)
    t = torch.zeros(64)
    b = _Bucket(t, [60, 4])
    ok = dict(params=acc, codec=_FakeCodec(), target_bits=8.0, per_tensor_budget=True)
    assert ddp.GcowHookState().per_tensor_budget is False
    bad = [dict(ok, relative_bits=8), dict(ok, error_feedback=True), dict(ok, compress_mean=True),
           dict(ok, target_bits=None), dict(ok, codec=_NoPerTensor()), dict(ok, params=codec.rate(16, 1))]
    for kw in bad:
        with pytest.raises(ValueError):
            ddp.roundtrip_hook(ddp.GcowHookState(**kw), b)
    with pytest.raises(ValueError, match="per_tensor_budget"):
        ddp.roundtrip_hook(ddp.GcowHookState(**dict(ok, target_bits=None)), b)
    with pytest.raises(ValueError, match="roundtrip_fitted_per_tensor"):
        ddp.roundtrip_hook(ddp.GcowHookState(**dict(ok, codec=_NoPerTensor())), b)
    with pytest.raises(ValueError, match="fp32 or bf16"):
        ddp.roundtrip_hook(ddp.GcowHookState(**ok), _Bucket(t.to(torch.float16), [64]))
    for hook in (ddp.compressed_allgather_hook, ddp.compressed_sharded_hook):  # the wire hooks
        with pytest.raises(ValueError, match="per_tensor_budget"):
            hook(ddp.GcowHookState(**ok), b)
        with pytest.raises(ValueError, match="per_tensor_budget"):
            hook(ddp.GcowHookState(**dict(ok, fit_on_device=True)), b)
