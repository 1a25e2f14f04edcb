"""The rate table (gcow_rate_table_device, include/gcow.h) on the CPU: the one-pass construction the kernel implements
(DESIGN.md 5.10), restated in numpy (tests/rate_table_inputs.model_table), equals the oracle's stream length under
expert(1, 16658, maxprec, minexp) for every one of the 288 values of minexp, on the crafted buckets of
tests/roundtrip_inputs.py (zero, subnormal, NaN / Inf, 3e38, wide-exponent, sparse and ramp blocks), fp32 and bf16; the
table is non-increasing and complete (nothing changes below minexp -154, one bit per block from 132 on); and the host
fit rule gcow_rate_table_fit on a hand-made table."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

TESTS = os.path.dirname(os.path.abspath(__file__))
if TESTS not in sys.path:
    sys.path.insert(0, TESTS)

SIZES = [4, 4096, 8192]
MAXPRECS = [64, 32, 31, 20, 12, 1, 0]


@pytest.mark.parametrize("bf16", [False, True], ids=["fp32", "bf16"])
@pytest.mark.parametrize("n", SIZES)
def test_model_matches_oracle_table(orc, n, bf16):
    import rate_table_inputs as RT
    for maxprec in MAXPRECS:
        x, want = RT.crafted_table(n, bf16, maxprec)
        got = RT.model_table(x, maxprec)
        bad = np.nonzero(got != want)[0]
        assert bad.size == 0, (maxprec, bad[:8].tolist(), got[bad[:8]].tolist(), want[bad[:8]].tolist())


@pytest.mark.parametrize("bf16", [False, True], ids=["fp32", "bf16"])
@pytest.mark.parametrize("n", SIZES)
def test_table_monotone_and_complete(orc, n, bf16):
    import rate_table_inputs as RT
    for maxprec in (64, 20, 1):
        x, t = RT.crafted_table(n, bf16, maxprec)
        assert np.all(np.diff(t) <= 0)
        assert t[286] == t[287] == n // 4
        for minexp in (-156, -155):
            assert RT.oracle_bits(x, maxprec, minexp) == t[0]


def _fit(table, budget):
    from gcow_amd import _ffi
    L = _ffi.load()
    h = (C.c_uint64 * 288)(*[int(v) for v in table])
    me, bits = C.c_int(12345), C.c_uint64(777)
    st = L.gcow_rate_table_fit(h, budget, C.byref(me), C.byref(bits))
    return st, me.value, bits.value


def test_fit_rule():
    import rate_table_inputs as RT
    # a hand-made non-increasing table with plateaus: 10000 for t < 40, then 9000 - 40 (t - 40) down to 100 blocks
    table = [10000 if t < 40 else max(100, 9000 - 40 * (t - 40)) for t in range(288)]
    assert table[287] == 100
    for budget in (1 << 40, 10000, 9999, 9000, 8999, 8961, 8960, 8959, 4567, 101, 100):
        st, me, bits = _fit(table, budget)
        want = RT.fit(table, budget)
        assert st == 0 and (me, bits) == want, (budget, st, me, bits, want)
        t = me + 154
        assert table[t] <= budget and (t == 0 or table[t - 1] > budget)  # the smallest minexp under the budget
    assert _fit(table, 10000)[1] == -154          # the whole table fits: full precision
    assert _fit(table, 8960)[1:] == (-154 + 41, 8960)  # budget == table[t] exactly picks t
    assert _fit(table, 8959)[1] == -154 + 42
    st, me, bits = _fit(table, 99)                # below one bit per block: no accuracy-mode stream is that short
    assert st == 1 and (me, bits) == (12345, 777)
    assert RT.fit(table, 99) is None


def test_fit_python_wrapper():
    from gcow_amd import codec
    table = np.array([5000 - 10 * t if t < 286 else 64 for t in range(288)], np.int64)
    assert codec.fit_minexp(table, 5000) == (-154, 5000)
    assert codec.fit_minexp(table.tolist(), 4995) == (-153, 4990)
    with pytest.raises(codec.GcowError):
        codec.fit_minexp(table, 63)
    with pytest.raises(codec.GcowError):
        codec.fit_minexp(table[:100], 5000)
