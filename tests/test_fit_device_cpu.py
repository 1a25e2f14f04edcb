"""The device fit's rule without a device (gcow_rate_table_fit_device, include/gcow.h): the numpy model of the kernel
(tests/fit_device_inputs.model_fit: a min over the indices whose entry fits, the coarsest entry with status 1 when none
does) against the host rule restated in tests/rate_table_inputs.fit, over tables with plateau ties, a constant table, a
strictly decreasing one, entries above 2^63 and an oracle table; budgets are every entry, each +- 1, 0 and 2^64 - 1.
The clamp of the minexp word: the model, and the claim it rests on -- outside [-154, 133] the oracle's stream no longer
changes. No call into libgcow."""
import os
import sys

import numpy as np
import pytest

TESTS = os.path.dirname(os.path.abspath(__file__))
if TESTS not in sys.path:
    sys.path.insert(0, TESTS)

import fit_device_inputs as FI  # noqa: E402


def _check(table):
    import rate_table_inputs as RT
    tu = np.asarray(table).view(np.uint64) if np.asarray(table).dtype == np.int64 else np.asarray(table)
    for b in FI.budgets(tu):
        me, status, bits = FI.model_fit(tu, b)
        host = RT.fit(tu, b)
        if host is None:  # the host call fails: the device takes the coarsest set and says so
            assert b < int(tu[-1])
            assert (me, status, bits) == (FI.MINEXP_HI, 1, int(tu[-1])), b
        else:
            assert (me, bits) == host and status == 0 and bits <= b, b
            t = me - FI.MINEXP_LO
            assert t == 0 or int(tu[t - 1]) > b  # the finest that fits: a plateau's first index


@pytest.mark.parametrize("name", ["plateau_table", "constant_table", "decreasing_table", "huge_table"])
def test_model_matches_host_rule(orc, name):
    _check(getattr(FI, name)())


def test_model_on_an_oracle_table(orc):
    import rate_table_inputs as RT
    _, table = RT.crafted_table(1027, False, 24)
    assert table[286] == table[287]  # a real plateau
    _check(np.array(table))


def test_plateau_takes_its_first_index():
    t = FI.plateau_table()
    runs = np.nonzero(np.diff(t) == 0)[0]
    assert runs.size > 50
    for i in runs[:40]:
        first = int(np.nonzero(t == t[i])[0][0])
        assert FI.model_fit(t, int(t[i]))[0] == FI.MINEXP_LO + first


def test_record_layout():
    r = FI.pack_record(-20, 0, 12345)
    assert r.dtype == np.int64 and r.tobytes()[:4] == np.array([-20], np.int32).tobytes()
    assert FI.pack_record(133, 1, 7).view(np.uint64)[0] == (1 << 32) | 133


def test_clamp_model():
    for w, want in [(-154, -154), (-155, -154), (-2 ** 31, -154), (0, 0), (-20, -20), (133, 133), (134, 133),
                    (2 ** 31 - 1, 133)]:
        assert FI.clamp(w) == want


@pytest.mark.parametrize("bf16", [False, True], ids=["fp32", "bf16"])
def test_clamp_loses_nothing(orc, bf16):
    """Below -154 and above 133 the oracle's stream is the one at the bound, for a bucket with subnormal, huge,
    non-finite and zero blocks."""
    import roundtrip_inputs as RI
    O = orc
    x = RI.inputs(1027, bf16)
    for maxprec in (64, 20):
        lo = O.compress(x, O.expert(1, 16658, maxprec, FI.MINEXP_LO))
        hi = O.compress(x, O.expert(1, 16658, maxprec, FI.MINEXP_HI))
        for me in (-155, -300, -1074):
            w, bits = O.compress(x, O.expert(1, 16658, maxprec, me))
            assert bits == lo[1] and w.tobytes() == lo[0].tobytes(), (maxprec, me)
        for me in (134, 200, 1000):
            w, bits = O.compress(x, O.expert(1, 16658, maxprec, me))
            assert bits == hi[1] and w.tobytes() == hi[0].tobytes(), (maxprec, me)
