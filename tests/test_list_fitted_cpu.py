"""The bit budget over a tensor list without a device (include/gcow.h: gcow_rate_table_list_workspace_bytes,
gcow_rate_table_list_device, gcow_roundtrip_list_fitted_device): the three symbols are exported, declared and bound;
every refusal the contract decides on the host returns its status before any launch, over plans built from made-up
addresses (a no-budget plan, and plans of the lean and generic domains, which both calls refuse); the workspace query;
the constant the grid-stride test reads; and the fit rule on the oracle's table of the seam list, whose entries the GPU
tests pin the kernels to."""
import ctypes as C
import os
import re
import sys

import pytest

TESTS = os.path.dirname(os.path.abspath(__file__))
if TESTS not in sys.path:
    sys.path.insert(0, TESTS)

from gcow_amd import _ffi  # noqa: E402
from gcow_amd._ffi import DTYPE_BF16, DTYPE_FLOAT, GcowParams  # noqa: E402

NAMES = ["gcow_rate_table_list_workspace_bytes", "gcow_rate_table_list_device", "gcow_roundtrip_list_fitted_device"]
NOBUDGET = GcowParams(1, 16658, 64, 0)
LEAN = GcowParams(64, 64, 64, -1074)
GENERIC = GcowParams(48, 48, 64, -1074)
INVALID = 1
A = 1 << 40  # made-up device addresses: nothing below is ever dereferenced


@pytest.fixture(scope="module")
def L():
    return _ffi.load()


def _plan(L, p, sizes=(8192 * 3 + 5, 7), in_dt=DTYPE_FLOAT, out_dt=DTYPE_FLOAT):
    from roundtrip_list_inputs import make_plan
    ins = [A + (1 << 30) * k for k in range(len(sizes))]
    st, buf, used = make_plan(L, ins, None if in_dt == out_dt else [a + (1 << 36) for a in ins], list(sizes), in_dt,
                              out_dt, p)
    assert st == 0
    return buf, C.cast(buf, C.c_void_p), used


def test_symbols_exported_declared_and_bound(L):
    declared = _ffi.header_functions()
    for name in NAMES:
        assert name in declared, name
        f = getattr(L, name)
        assert f.argtypes is not None and len(f.argtypes) >= 2, name
    assert L.gcow_rate_table_list_workspace_bytes.restype is C.c_size_t


def test_grid_cap_is_the_one_kernels_h_states():
    from gcow_amd import codec
    src = open(os.path.join(_ffi.HERE, "csrc", "kernels.h")).read()
    m = re.search(r"constexpr uint32_t kRateTableListMaxGrid = (\d+);", src)
    assert m and int(m.group(1)) == codec.RATE_TABLE_LIST_MAX_GRID == 1024


def test_workspace_query(L):
    buf, h, used = _plan(L, NOBUDGET)
    ws = L.gcow_rate_table_list_workspace_bytes(h, used)
    assert ws > 0 and ws % 8 == 0
    assert ws == L.gcow_rate_table_workspace_bytes(None)  # the two 288-bin arrays, whatever the list
    buf0, h0, used0 = _plan(L, NOBUDGET, sizes=())
    assert L.gcow_rate_table_list_workspace_bytes(h0, used0) == ws
    assert L.gcow_rate_table_list_workspace_bytes(None, used) == 0
    assert L.gcow_rate_table_list_workspace_bytes(h, used - 8) == 0


def _table(L, h, d_plan, nbytes, maxprec=64, table=A, ws=A + 4096, wsb=None):
    if wsb is None:
        wsb = L.gcow_rate_table_workspace_bytes(None)
    return L.gcow_rate_table_list_device(h, d_plan, nbytes, maxprec, table, ws, wsb, None)


def _rt(L, h, d_plan, nbytes, maxprec=64, word=A, total=A + 64):
    return L.gcow_roundtrip_list_fitted_device(h, d_plan, nbytes, maxprec, word, total, None)


@pytest.mark.parametrize("in_dt,out_dt", [(DTYPE_FLOAT, DTYPE_FLOAT), (DTYPE_BF16, DTYPE_FLOAT)])
def test_refusals_decided_on_the_host(L, in_dt, out_dt):
    buf, h, used = _plan(L, NOBUDGET, in_dt=in_dt, out_dt=out_dt)
    d = A + (1 << 20)
    wsb = L.gcow_rate_table_workspace_bytes(None)
    foreign = (C.c_uint64 * (used // 8 + 1))()
    hf = C.cast(foreign, C.c_void_p)
    for call in (_table, _rt):
        assert call(L, None, d, used) == INVALID          # NULL h_plan
        assert call(L, h, d, used - 8) == INVALID         # short
        assert call(L, h, d, 16) == INVALID               # shorter than a header
        assert call(L, hf, d, used) == INVALID            # not a plan
        assert call(L, h, None, used) == INVALID          # NULL d_plan
        assert call(L, h, d + 4, used) == INVALID         # d_plan off 8 bytes
    assert _table(L, h, d, used, table=None) == INVALID
    assert _table(L, h, d, used, table=A + 4) == INVALID
    assert _table(L, h, d, used, ws=None) == INVALID
    assert _table(L, h, d, used, ws=A + 4100) == INVALID
    assert _table(L, h, d, used, wsb=wsb - 8) == INVALID
    assert _table(L, h, d, used, wsb=0) == INVALID
    assert _rt(L, h, d, used, word=None) == INVALID
    assert _rt(L, h, d, used, word=A + 2) == INVALID
    assert _rt(L, h, d, used, total=None) == INVALID
    assert _rt(L, h, d, used, total=A + 68) == INVALID
    assert b"d_total_bits" in L.gcow_last_error()


@pytest.mark.parametrize("p", [LEAN, GcowParams(32, 32, 64, -1074), GENERIC, GcowParams(1, 100, 64, -30)],
                         ids=["lean64", "lean32", "rate12", "expert_trunc"])
def test_plans_of_other_domains_are_refused(L, p):
    from gcow_amd._ffi import RoundtripListStats
    buf, h, used = _plan(L, p)
    s = RoundtripListStats()
    assert L.gcow_roundtrip_list_plan_stats(h, used, C.byref(s)) == 0 and s.domain != 1
    assert _table(L, h, A + (1 << 20), used) == INVALID
    assert b"block budget" in L.gcow_last_error()
    assert _rt(L, h, A + (1 << 20), used) == INVALID


def test_any_nobudget_plan_is_taken_whatever_its_maxprec_and_minexp(L):
    """The plan's own maxprec / minexp are not read: the domain alone decides, so the argument checks that follow it
    are reached (here: the NULL table and the NULL word)."""
    from gcow_amd._ffi import RoundtripListStats
    for p in (NOBUDGET, GcowParams(1, 16658, 12, -30), GcowParams(0, 160, 20, 5)):
        buf, h, used = _plan(L, p)
        s = RoundtripListStats()
        assert L.gcow_roundtrip_list_plan_stats(h, used, C.byref(s)) == 0 and s.domain == 1
        assert _table(L, h, A + (1 << 20), used, maxprec=33, table=None) == INVALID
        assert b"table" in L.gcow_last_error()
        assert _rt(L, h, A + (1 << 20), used, maxprec=33, word=None) == INVALID
        assert b"d_minexp" in L.gcow_last_error()


def test_fit_on_the_seam_table(orc):
    """The budgets the GPU tests fit: entry 287 is the block count, one bit below it nothing fits; the fitted minexp at
    0.3 .. 16 bits per value; from 33 bits per value on every block keeps its full precision."""
    import list_fitted_inputs as LF
    from rate_table_inputs import fit
    n = sum(LF.seam_sizes(1))
    T = LF.seam_table(1, False, 64)
    assert n == 81929 and int(T[287]) == (n + 3) // 4 == 20483
    # entries 286 and 287 are equal (include/gcow.h): the fit takes the plateau's first index
    assert fit(T, int(T[287]) - 1) is None and fit(T, int(T[287])) == (132, 20483)
    assert LF.fit_record(T, int(T[287]) - 1) == (133, 1, 20483)
    assert LF.budget_of(0.25, n) == 20482 and fit(T, LF.budget_of(0.25, n)) is None
    want = {0.3: 7, 1: -2, 2.5: -5, 4: -7, 8: -11, 16: -20}
    assert {b: fit(T, LF.budget_of(b, n))[0] for b in want} == want
    for b in (33, 40, 64):
        assert fit(T, LF.budget_of(b, n)) == (-154, int(T[0]))
    assert all(int(T[t]) >= int(T[t + 1]) for t in range(287))
    bl = LF.budgets(T, n)
    assert len(bl) == 6 and bl[2] == int(T[-11 + 154]) and LF.fit_record(T, bl[5])[0] == -154
