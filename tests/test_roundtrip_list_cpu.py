"""The host plan of the round trip over a tensor list (gcow_roundtrip_list_plan, include/gcow.h) against a brute-force
classification of every chunk (tests/roundtrip_list_inputs.py classify): chunk kind, the row addresses of direct chunks,
the first and last tensor of gather chunks, empty tensors dropped; for the seam list of the GPU test and for random
lists, both element types, all three domains. Needs no GPU: the plan is host arithmetic over made-up addresses."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

TESTS = os.path.dirname(os.path.abspath(__file__))
if TESTS not in sys.path:
    sys.path.insert(0, TESTS)

from gcow_amd import _ffi  # noqa: E402
from gcow_amd._ffi import DTYPE_BF16, DTYPE_FLOAT, GcowParams  # noqa: E402

PARAMS = {"rate16": GcowParams(64, 64, 64, -1074), "rate8": GcowParams(32, 32, 64, -1074),
          "acc1e-3": GcowParams(1, 16658, 64, -10), "rate12": GcowParams(48, 48, 64, -1074)}
ESZ = {DTYPE_FLOAT: 4, DTYPE_BF16: 2}


@pytest.fixture(scope="module")
def L():
    return _ffi.load()


def _addresses(sizes, esz, rng, mode):
    """Made-up device addresses for the tensors, none overlapping: "aligned" 256-byte aligned, "element" at odd
    element offsets, "random" at any element offset."""
    at, out = 1 << 40, []
    for n in sizes:
        if mode == "aligned":
            at = (at + 255) // 256 * 256
        elif mode == "element":
            at = (at + 255) // 256 * 256 + esz
        else:
            at += esz * int(rng.integers(0, 9))
        out.append(at)
        at += n * esz + 3 * esz
    return out


def _check(L, sizes, in_dt, out_dt, p, rng, mode, inplace):
    from roundtrip_list_inputs import classify, domain_of, make_plan, plan_chunks
    ins = _addresses(sizes, ESZ[in_dt], rng, mode)
    outs = None if inplace else [a + (1 << 36) for a in _addresses(sizes, ESZ[out_dt], rng, mode)]
    st, buf, used = make_plan(L, ins, outs, sizes, in_dt, out_dt, p)
    assert st == 0
    s, direct, gather = plan_chunks(L, C.cast(buf, C.c_void_p), used)
    assert s.total_values == sum(sizes) and s.segments == sum(1 for n in sizes if n)  # empty tensors dropped
    assert s.domain == domain_of(p) and s.used_bytes == used
    want = classify(ins, outs if outs is not None else ins, sizes, ESZ[in_dt], ESZ[out_dt], s.domain, s.row_rule)
    assert direct == [w for w in want if w[0] == "d"]
    assert gather == [w for w in want if w[0] == "g"]
    return s


@pytest.mark.parametrize("pname", list(PARAMS))
@pytest.mark.parametrize("in_dt,out_dt", [(DTYPE_FLOAT, DTYPE_FLOAT), (DTYPE_BF16, DTYPE_BF16),
                                          (DTYPE_FLOAT, DTYPE_BF16), (DTYPE_BF16, DTYPE_FLOAT)])
@pytest.mark.parametrize("mode", ["aligned", "element"])
@pytest.mark.parametrize("r", [0, 1, 2, 3])
def test_seam_list_plan(L, r, mode, in_dt, out_dt, pname):
    from roundtrip_list_inputs import seam_sizes
    rng = np.random.default_rng(5)
    s = _check(L, seam_sizes(r), in_dt, out_dt, PARAMS[pname], rng, mode, in_dt == out_dt)
    assert s.direct_chunks + s.gather_chunks == 11
    if s.domain == 2:
        assert s.direct_chunks == 0
    elif in_dt == out_dt == DTYPE_FLOAT and s.row_rule == 0:
        # chunks 1, 3, 5 and 7 lie inside the four long tensors (which start at offsets 2, 1, 0, 3 mod 4) and 9 inside
        # the tensor that starts on the chunk boundary; the others hold seams or the last block
        assert s.direct_chunks == 5 and s.gather_chunks == 6


@pytest.mark.parametrize("seed", range(12))
def test_random_list_plan(L, seed):
    rng = np.random.default_rng(100 + seed)
    kinds = rng.integers(0, 4, 40)
    sizes = [int(v) for k in kinds for v in
             ([0], rng.integers(1, 5, 6), [int(rng.integers(5, 3000))], [int(rng.integers(8192, 40000))])[k]]
    in_dt, out_dt = [(DTYPE_FLOAT, DTYPE_FLOAT), (DTYPE_BF16, DTYPE_BF16), (DTYPE_FLOAT, DTYPE_BF16),
                     (DTYPE_BF16, DTYPE_FLOAT)][seed % 4]
    p = list(PARAMS.values())[(seed // 4) % 3]
    _check(L, sizes, in_dt, out_dt, p, rng, "random", inplace=in_dt == out_dt and seed % 2 == 0)


def test_empty_and_refusals(L):
    from roundtrip_list_inputs import make_plan, plan_chunks
    p = PARAMS["rate16"]
    st, buf, used = make_plan(L, [], None, [], DTYPE_FLOAT, DTYPE_FLOAT, p)
    assert st == 0
    s, direct, gather = plan_chunks(L, C.cast(buf, C.c_void_p), used)
    assert (s.total_values, s.segments, direct, gather) == (0, 0, [], [])
    st, buf, used = make_plan(L, [0, 0], None, [0, 0], DTYPE_FLOAT, DTYPE_FLOAT, p)  # NULL with a zero count
    assert st == 0 and plan_chunks(L, C.cast(buf, C.c_void_p), used)[0].segments == 0
    a = 1 << 40
    assert make_plan(L, [a], None, [8], 4, DTYPE_FLOAT, p)[0] == 5            # dtype_double in
    assert make_plan(L, [a], [a + 4096], [8], DTYPE_FLOAT, 1, p)[0] == 5      # dtype_int32 out
    assert make_plan(L, [a], None, [1 << 34], DTYPE_FLOAT, DTYPE_FLOAT, p)[0] == 5   # 2^32 blocks
    assert make_plan(L, [a, 0], None, [8, 8], DTYPE_FLOAT, DTYPE_FLOAT, p)[0] == 1   # NULL with a count
    assert make_plan(L, [a + 2], None, [8], DTYPE_FLOAT, DTYPE_FLOAT, p)[0] == 1     # fp32 off 4 bytes
    assert make_plan(L, [a + 1], None, [8], DTYPE_BF16, DTYPE_BF16, p)[0] == 1       # bf16 off 2 bytes
    assert make_plan(L, [a], None, [8], DTYPE_FLOAT, DTYPE_BF16, p)[0] == 1          # in place, unequal dtypes
    assert make_plan(L, [a], None, [8], DTYPE_FLOAT, DTYPE_FLOAT, GcowParams(8, 4, 64, -1074))[0] == 1  # check_params
    assert make_plan(L, [a], None, [8], DTYPE_FLOAT, DTYPE_FLOAT, p, slack=-8)[0] == 1  # short plan_bytes
    st, buf, used = make_plan(L, [a], None, [8], DTYPE_FLOAT, DTYPE_FLOAT, p)
    from gcow_amd._ffi import RoundtripListStats
    assert st == 0
    assert L.gcow_roundtrip_list_plan_stats(C.cast(buf, C.c_void_p), used - 8, C.byref(RoundtripListStats())) == 1
