"""The host plan of the round trip with a tolerance relative to each tensor (gcow_roundtrip_rel_plan, include/gcow.h)
on made-up addresses -- stats, every block covered exactly once by a direct chunk or a gather piece, which tensors run
direct -- its refusals, and the documented bound |d - t| <= 2^minexp_s checked on the oracle model of
tests/relative_inputs.py. Needs no GPU."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

TESTS = os.path.dirname(os.path.abspath(__file__))
if TESTS not in sys.path:
    sys.path.insert(0, TESTS)

from gcow_amd import _ffi  # noqa: E402
from gcow_amd._ffi import DTYPE_BF16, DTYPE_FLOAT  # noqa: E402

ESZ = {DTYPE_FLOAT: 4, DTYPE_BF16: 2}
PAIRS = [(DTYPE_FLOAT, DTYPE_FLOAT), (DTYPE_BF16, DTYPE_BF16), (DTYPE_FLOAT, DTYPE_BF16), (DTYPE_BF16, DTYPE_FLOAT)]
CHUNK_BLOCKS, GATHER_BLOCKS, MIN_DIRECT = 2048, 256, 256


@pytest.fixture(scope="module")
def L():
    return _ffi.load()


def make_plan(L, in_ptrs, out_ptrs, counts, in_dt, out_dt, slack=0):
    n = len(counts)
    ins = (C.c_void_p * max(n, 1))(*[int(a) or None for a in in_ptrs])
    ous = (C.c_void_p * max(n, 1))(*[int(a) or None for a in out_ptrs]) if out_ptrs is not None else None
    cnt = (C.c_uint64 * max(n, 1))(*[int(c) for c in counts])
    need = L.gcow_roundtrip_rel_plan_bytes(n, int(sum(int(c) for c in counts))) + slack
    buf = (C.c_uint64 * max((need + 7) // 8, 1))()
    used = C.c_size_t(0)
    st = L.gcow_roundtrip_rel_plan(ins, ous, cnt, n, in_dt, out_dt, C.cast(buf, C.c_void_p), need, C.byref(used))
    return st, buf, int(used.value)


def plan_chunks(L, buf, used):
    """(stats, direct chunks, gather pieces), each a list of (tensor, first block, blocks)."""
    h = C.cast(buf, C.c_void_p)
    s = _ffi.RoundtripRelStats()
    assert L.gcow_roundtrip_rel_plan_stats(h, used, C.byref(s)) == 0
    a, b, c = C.c_uint64(), C.c_uint64(), C.c_uint64()
    direct = []
    for i in range(s.direct_chunks):
        assert L.gcow_roundtrip_rel_plan_chunk(h, used, 0, i, C.byref(a), C.byref(b), C.byref(c)) == 0
        direct.append((int(a.value), int(b.value), int(c.value)))
    pieces, i = [], 0
    while L.gcow_roundtrip_rel_plan_chunk(h, used, 1, i, C.byref(a), C.byref(b), C.byref(c)) == 0:
        pieces.append((int(a.value), int(b.value), int(c.value)))
        i += 1
    return s, direct, pieces


def _addresses(sizes, esz, offset_elems):
    """Made-up device addresses, none overlapping: 256-byte aligned bases plus offset_elems elements."""
    at, out = 1 << 40, []
    for n in sizes:
        at = (at + 255) // 256 * 256
        out.append(at + offset_elems * esz)
        at += (n + offset_elems + 3) * esz
    return out


def _check(L, sizes, in_dt, out_dt, offset_elems, inplace):
    ins = _addresses(sizes, ESZ[in_dt], offset_elems)
    outs = None if inplace else [a + (1 << 36) for a in _addresses(sizes, ESZ[out_dt], offset_elems)]
    st, buf, used = make_plan(L, ins, outs, sizes, in_dt, out_dt)
    assert st == 0
    s, direct, pieces = plan_chunks(L, buf, used)
    nblocks = [(n + 3) // 4 for n in sizes]
    assert s.total_values == sum(sizes) and s.total_blocks == sum(nblocks)
    assert s.segments == sum(1 for n in sizes if n) and s.used_bytes == used   # empty tensors dropped
    # every block of every tensor exactly once
    seen = [np.zeros(nb, np.int32) for nb in nblocks]
    for t, b0, nb in direct:
        assert 0 < nb <= CHUNK_BLOCKS and b0 + nb <= sizes[t] // 4   # whole blocks only
        seen[t][b0:b0 + nb] += 1
    for t, b0, nb in pieces:
        assert nb > 0 and b0 + nb == nblocks[t]
        seen[t][b0:] += 1
    assert all((c == 1).all() for c in seen)
    assert s.direct_chunks == len(direct)
    assert s.gather_chunks == (sum(nb for _, _, nb in pieces) + GATHER_BLOCKS - 1) // GATHER_BLOCKS
    # which tensors run direct: at least MIN_DIRECT whole blocks, input and output at 4-byte aligned addresses
    out_ptrs = outs if outs is not None else ins
    has_direct = {t for t, _, _ in direct}
    for t, n in enumerate(sizes):
        want = n // 4 >= MIN_DIRECT and ins[t] % 4 == 0 and out_ptrs[t] % 4 == 0
        assert (t in has_direct) == want, (t, n)
    return s, direct, pieces


@pytest.mark.parametrize("in_dt,out_dt", PAIRS)
@pytest.mark.parametrize("offset_elems", [0, 1], ids=["aligned", "one-element"])
@pytest.mark.parametrize("name", ["edges", "small"])
def test_plan_covers_every_block(L, name, offset_elems, in_dt, out_dt):
    from relative_inputs import EDGE_SIZES, SMALL_SIZES
    sizes = EDGE_SIZES if name == "edges" else SMALL_SIZES
    s, direct, pieces = _check(L, sizes, in_dt, out_dt, offset_elems, in_dt == out_dt)
    bf16_any = DTYPE_BF16 in (in_dt, out_dt)
    if offset_elems == 1 and bf16_any:
        assert not direct      # bf16 tensors at odd element offsets have no direct chunk
    else:
        assert direct          # fp32 tensors at 4-byte but not 16-byte aligned addresses do
        if name == "edges":    # 8191, 8192, 8193 -> one chunk each; 24583 -> three chunks and a partial block
            assert [(t, nb) for t, _, nb in direct] == [(5, 2047), (6, 2048), (7, 2048), (8, 2048), (8, 2048), (8, 2048),
                                                        (8, 1)]
            assert [t for t, _, _ in pieces] == [0, 1, 2, 3, 5, 7, 8, 9, 10]


@pytest.mark.parametrize("seed", range(8))
def test_random_lists(L, seed):
    rng = np.random.default_rng(300 + seed)
    kinds = rng.integers(0, 4, 30)
    sizes = [int(v) for k in kinds for v in
             ([0], rng.integers(1, 9, 5), [int(rng.integers(900, 1100))], [int(rng.integers(8000, 30000))])[k]]
    in_dt, out_dt = PAIRS[seed % 4]
    _check(L, sizes, in_dt, out_dt, seed // 4, inplace=in_dt == out_dt and seed % 2 == 0)


def test_empty_and_refusals(L):
    st, buf, used = make_plan(L, [], None, [], DTYPE_FLOAT, DTYPE_FLOAT)
    assert st == 0
    s, direct, pieces = plan_chunks(L, buf, used)
    assert (s.total_values, s.total_blocks, s.segments, direct, pieces) == (0, 0, 0, [], [])
    # an empty list runs without a device: nothing to launch when no bit count is asked for
    assert L.gcow_roundtrip_rel_device(C.cast(buf, C.c_void_p), None, used, 8, 64, None, None, None) == 0
    st, buf, used = make_plan(L, [0, 0], None, [0, 0], DTYPE_FLOAT, DTYPE_FLOAT)   # NULL with a zero count
    assert st == 0 and plan_chunks(L, buf, used)[0].segments == 0
    a = 1 << 40
    assert make_plan(L, [a], None, [8], 4, DTYPE_FLOAT)[0] == 5               # dtype_double in
    assert make_plan(L, [a], [a + 4096], [8], DTYPE_FLOAT, 1)[0] == 5         # dtype_int32 out
    assert make_plan(L, [a], None, [1 << 34], DTYPE_FLOAT, DTYPE_FLOAT)[0] == 5      # 2^32 blocks in one tensor
    many = [(1 << 33) + 1] * 2                                                       # ... and summed over two
    assert make_plan(L, [a, a + (1 << 37)], None, many, DTYPE_FLOAT, DTYPE_FLOAT)[0] == 5
    assert make_plan(L, [a, 0], None, [8, 8], DTYPE_FLOAT, DTYPE_FLOAT)[0] == 1      # NULL with a count
    assert make_plan(L, [a + 2], None, [8], DTYPE_FLOAT, DTYPE_FLOAT)[0] == 1        # fp32 off 4 bytes
    assert make_plan(L, [a + 1], None, [8], DTYPE_BF16, DTYPE_BF16)[0] == 1          # bf16 off 2 bytes
    assert make_plan(L, [a], None, [8], DTYPE_FLOAT, DTYPE_BF16)[0] == 1             # in place, unequal dtypes
    assert make_plan(L, [a], None, [8], DTYPE_FLOAT, DTYPE_FLOAT, slack=-8)[0] == 1  # short plan_bytes
    st, buf, used = make_plan(L, [a], None, [8], DTYPE_FLOAT, DTYPE_FLOAT)
    assert st == 0
    h = C.cast(buf, C.c_void_p)
    assert L.gcow_roundtrip_rel_plan_stats(h, used - 8, C.byref(_ffi.RoundtripRelStats())) == 1
    # the device call's own refusals come before any launch (made-up device addresses are never touched)
    d_plan, d_abs = 1 << 41, 1 << 42
    assert L.gcow_roundtrip_rel_device(h, d_plan, used - 8, 8, 64, d_abs, None, None) == 1   # short plan_bytes
    assert L.gcow_roundtrip_rel_device(h, d_plan, used, 25, 64, d_abs, None, None) == 1      # rel_bits > 24
    assert L.gcow_roundtrip_rel_device(h, d_plan, used, 8, 64, None, None, None) == 1        # NULL d_absmax
    assert L.gcow_roundtrip_rel_device(h, d_plan, used, 8, 64, d_abs + 2, None, None) == 1   # misaligned d_absmax
    assert L.gcow_roundtrip_rel_device(h, d_plan, used, 8, 64, d_abs, d_abs + 4, None) == 1  # misaligned bit count
    assert L.gcow_roundtrip_rel_device(h, None, used, 8, 64, d_abs, None, None) == 1         # NULL device plan
    # a list plan is not a relative plan
    from gcow_amd._ffi import GcowParams
    need = L.gcow_roundtrip_list_plan_bytes(1, 8)
    lbuf = (C.c_uint64 * ((need + 7) // 8))()
    ins = (C.c_void_p * 1)(a)
    cnt = (C.c_uint64 * 1)(8)
    assert L.gcow_roundtrip_list_plan(ins, None, cnt, 1, DTYPE_FLOAT, DTYPE_FLOAT, C.byref(GcowParams(1, 16658, 64, -10)),
                                      C.cast(lbuf, C.c_void_p), need, None) == 0
    assert L.gcow_roundtrip_rel_device(C.cast(lbuf, C.c_void_p), d_plan, need, 8, 64, d_abs, None, None) == 1


@pytest.mark.parametrize("k", [0, 8, 24])
@pytest.mark.parametrize("bf16", [False, True], ids=["fp32", "bf16"])
@pytest.mark.parametrize("name", ["edges", "small", "special"])
def test_model_meets_the_documented_bound(orc, name, bf16, k):
    """|d - t| <= 2^minexp_s for every finite value of the three lists: a property of the oracle under the definition,
    checked as the header states it (blocks holding an Inf or a NaN are left out: their own values are spoiled).

    The tensor of scale 3e38 has its maximum in the top binade (a_s = 2.99e38, emax_s = 128). Under
    minexp_s = emax_s - k alone, at k = 0 a block keeps 4 planes and 5 of the 64 values (2.43e38, 2.56e38, 2.99e38,
    -2.74e38, ...) round up to +-2^128, which fp32 stores as Inf, and at k = 1 the maximum still does. The headroom
    cap (minexp_s <= floor(log2(2^128 - a_s)) - 2 = 122 here) is what keeps these cases inside the bound; the test
    also asserts that every decode of a finite block is finite."""
    from relative_inputs import absmax_of, expect, minexp_of, tensors
    from roundtrip_inputs import widen
    outs, amax, bits = expect(name, bf16, k, 64)
    ts = tensors(name, bf16)
    assert len(outs) == len(ts) == amax.size
    checked = 0
    for t, d, a in zip(ts, outs, amax):
        x = widen(t).astype(np.float64)
        fin = np.isfinite(x)
        # Inf / NaN members spoil their own block only: the bound is for the blocks without one
        blk_ok = np.repeat(np.add.reduceat(~fin, np.arange(0, x.size, 4)) == 0, 4)[:x.size] if x.size else fin
        assert a == absmax_of(t)
        assert np.isfinite(d[blk_ok]).all()
        err = np.abs(d.astype(np.float64) - x)[blk_ok]
        assert (err <= 2.0 ** minexp_of(a, k)).all(), (name, k, float(err.max()), minexp_of(a, k))
        checked += int(blk_ok.sum())
    assert checked > 0 and bits > 0
