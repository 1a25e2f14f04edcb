"""TEST INFRASTRUCTURE ONLY -- the seam list, its field and a brute-force model of the host plan, shared by
tests/test_roundtrip_list_cpu.py and tests/test_gpu_roundtrip_list.py (the round trip over a tensor list,
gcow_roundtrip_list_* in include/gcow.h)."""
from __future__ import annotations

import ctypes as C
import functools

import numpy as np

from oracle import oracle as O
from roundtrip_inputs import MODES, inputs

CHUNK = 8192  # values per plan chunk: 256 lanes x 8 blocks x 4 values
LONG = 2 * CHUNK + 3
TAILS = {0: [3], 1: [4], 2: [1], 3: [2]}  # total % 4 -> the last tensors


def seam_sizes(r: int) -> list[int]:
    """The seam list whose total is r (mod 4). Flat offsets, C = CHUNK:
      0            6 values, then ten one-value tensors, then 2 3 1 1 2 3 1 3 3 3 3 3 2 (to 46) with empty tensors
                   among them: blocks 1 .. 11 -- the crafted zero, subnormal, NaN, Inf and 3e38 blocks of
                   roundtrip_inputs.inputs -- take their values from two, three and four tensors
      46           four long tensors of 2 C + 3 values, starting at offsets = 2, 1, 0 and 3 (mod 4)
      8 C + 58     a filler that ends exactly on the chunk boundary 9 C
      9 C          C + 5 values (to 10 C + 5: one value of the last whole-or-partial block)
      10 C + 5     the tail: 3, 4, 1 or 2 values, so the totals are 0, 1, 2, 3 (mod 4); with the tail of 1 the partial
                   last block's two real values come from two tensors."""
    s = [6] + [1] * 10 + [0, 2, 3, 1, 1, 0, 0, 2, 3, 1, 3, 3, 3, 3, 3, 2, 0]
    assert sum(s) == 46
    s += [LONG] * 4 + [0]
    s += [9 * CHUNK - sum(s)]
    s += [CHUNK + 5] + TAILS[r] + [0]
    assert sum(s) % 4 == r and sum(s) // CHUNK == 10
    return s


def seam_starts(sizes) -> np.ndarray:
    return np.concatenate([[0], np.cumsum(sizes)]).astype(np.int64)


@functools.lru_cache(maxsize=None)
def seam_field(r: int, bf16: bool) -> np.ndarray:
    """The seam list's concatenation: roundtrip_inputs.inputs, whose crafted blocks (from block 1 on: the special
    values, then wide-exponent, sparse, constant, alternating, ramp, subnormal, zero and tiny blocks -- the long group
    phases) lie across the small tensors of chunk 0, copied once more to chunk 3, which lies inside the long tensor
    that starts at an offset of 1 (mod 4): the direct kernels code them too."""
    n = sum(seam_sizes(r))
    x = inputs(n, bf16).copy()
    x[3 * CHUNK + 4:3 * CHUNK + 7604] = x[4:7604]
    x.setflags(write=False)
    return x


@functools.lru_cache(maxsize=None)
def seam_case(r: int, bf16: bool, mode: str):
    """-> (X, the oracle's decompress(compress(X)) as fp32, the stream's bit count); computed once, read-only."""
    op = MODES[mode]()
    x = seam_field(r, bf16)
    w, bits = O.compress(x, op)
    d = O.decompress(w, (x.size,), op)
    d.setflags(write=False)
    return x, d, bits


# ------------------------------------------------------------------------------------------------ the plan, by brute force
def domain_of(p) -> int:
    """0 whole-word fixed rate, 1 no budget, 2 generic: the predicates of gcow_roundtrip_device."""
    minbits, maxbits, maxprec, minexp = p.tuple()
    if minbits == maxbits and maxbits in (32, 64) and maxprec >= 32 and minexp <= -154:
        return 0
    if minbits <= 1 and maxbits >= 160:
        return 1
    return 2


def classify(in_ptrs, out_ptrs, counts, esz_in, esz_out, domain, rule):
    """Every chunk of the list by looking at every value: ('d', in address, out address, blocks) for a chunk whose
    values all come from one tensor, that holds whole blocks only and whose first row's two addresses are multiples of
    4 (rule 0) or of the row's size (rule 1); ('g', first block, first tensor, last tensor) otherwise, the tensors
    numbered among the non-empty ones. The generic domain has gather chunks only."""
    live = [(int(i), int(o), int(n)) for i, o, n in zip(in_ptrs, out_ptrs, counts) if n]
    cnt = np.array([n for _, _, n in live], np.int64)
    nvals = int(cnt.sum())
    seg_of = np.repeat(np.arange(len(live)), cnt)
    start = np.concatenate([[0], np.cumsum(cnt)])
    ain = 4 if rule == 0 else 4 * esz_in
    aout = 4 if rule == 0 else 4 * esz_out
    out = []
    for v0 in range(0, nvals, CHUNK):
        v1 = min(v0 + CHUNK, nvals)
        ids = seg_of[v0:v1]
        s = int(ids[0])
        ia = live[s][0] + (v0 - int(start[s])) * esz_in
        oa = live[s][1] + (v0 - int(start[s])) * esz_out
        if (domain != 2 and int(ids.min()) == int(ids.max()) and (v1 - v0) % 4 == 0 and ia % ain == 0
                and oa % aout == 0):
            out.append(("d", ia, oa, (v1 - v0) // 4))
        else:
            out.append(("g", v0 // 4, s, int(ids[-1])))
    return out


def make_plan(L, in_ptrs, out_ptrs, counts, in_dt, out_dt, p, slack=0):
    """gcow_roundtrip_list_plan into a ctypes buffer -> (status, buffer, used bytes)."""
    n = len(counts)
    ins = (C.c_void_p * max(n, 1))(*[int(a) or None for a in in_ptrs])
    ous = (C.c_void_p * max(n, 1))(*[int(a) or None for a in out_ptrs]) if out_ptrs is not None else None
    cnt = (C.c_uint64 * max(n, 1))(*[int(c) for c in counts])
    need = L.gcow_roundtrip_list_plan_bytes(n, int(sum(int(c) for c in counts))) + slack
    buf = (C.c_uint64 * max((need + 7) // 8, 1))()
    used = C.c_size_t(0)
    st = L.gcow_roundtrip_list_plan(ins, ous, cnt, n, in_dt, out_dt, C.byref(p), C.cast(buf, C.c_void_p), need,
                                    C.byref(used))
    return st, buf, int(used.value)


def plan_chunks(L, h_plan, nbytes):
    """(stats, the plan's direct descriptors, its gather descriptors), each list in the plan's order."""
    from gcow_amd._ffi import RoundtripListStats
    s = RoundtripListStats()
    assert L.gcow_roundtrip_list_plan_stats(h_plan, nbytes, C.byref(s)) == 0
    a, b, c = C.c_uint64(), C.c_uint64(), C.c_uint64()
    out = []
    for gather, count, tag in ((0, s.direct_chunks, "d"), (1, s.gather_chunks, "g")):
        lst = []
        for i in range(count):
            assert L.gcow_roundtrip_list_plan_chunk(h_plan, nbytes, gather, i, C.byref(a), C.byref(b), C.byref(c)) == 0
            lst.append((tag, int(a.value), int(b.value), int(c.value)))
        out.append(lst)
    return s, out[0], out[1]
