"""TEST INFRASTRUCTURE ONLY -- the tensor lists of the bit budget per tensor (include/gcow.h: gcow_rate_table_rel_device,
gcow_rate_table_fit_batch_device, gcow_roundtrip_rel_fitted_device) and their expectation, computed tensor by tensor
with the oracle from the definition: table_s = oracle_table(t_s, maxprec) (288 encodes of the tensor as a field of its
own), the fit rule with the floor restated below, out_s = decompress(compress(t_s, expert(1, 16658, maxprec, minexp_s)))
and its bit count. The lists are relative_inputs.tensors ("edges", "small", "special", "hook"), fp32 and bf16; every
oracle result is computed once and shared. Shared by tests/test_fitted_per_tensor_cpu.py and
tests/test_gpu_fitted_per_tensor.py."""
from __future__ import annotations

import functools
import math

import numpy as np

from oracle import oracle as O
from rate_table_inputs import ENTRIES, MINEXP_LO, oracle_table
from relative_inputs import tensors

MINEXP_HI = MINEXP_LO + ENTRIES - 1  # 133
FLOOR = -94                          # the Python layer's default floor (codec.MINEXP_FLOOR)
LISTS = ["edges", "small", "special", "hook"]
BPVS = [8.0, 2.5, 0.5]
FLOORS = [-154, -94]
POISON = 0x5A5A5A5A5A5A5A5A  # fills the tables and the workspace before every table call
WS_WORDS = 2 * ENTRIES + 1   # workspace words per tensor: the two arrays and the block count


def maxprecs(name: str):
    """The 300-tensor list's tables take the oracle 86 400 encodes per maxprec: one maxprec for it."""
    return [64] if name == "small" else [64, 12]


def budget_of(bits_per_value: float, n: int) -> int:
    return int(math.floor(bits_per_value * n))


def fit_floor(table, budget_bits: int, floor: int = MINEXP_LO):
    """gcow_rate_table_fit_batch_device restated -> (minexp, status, bits): the smallest minexp in
    [max(floor, -154), 133] whose entry is <= budget_bits, with status 0; none: (133, 1, table[287])."""
    for t in range(max(floor, MINEXP_LO) - MINEXP_LO, ENTRIES):
        if int(table[t]) <= budget_bits:
            return MINEXP_LO + t, 0, int(table[t])
    return MINEXP_HI, 1, int(table[ENTRIES - 1])


@functools.lru_cache(maxsize=None)
def tables(name: str, bf16: bool, maxprec: int) -> np.ndarray:
    """int64[S, 288]: row s = oracle_table(t_s, maxprec), zeros for an empty tensor; read-only."""
    T = np.stack([oracle_table(np.array(t), maxprec) for t in tensors(name, bf16)])
    T.setflags(write=False)
    return T


@functools.lru_cache(maxsize=None)
def fits(name: str, bf16: bool, maxprec: int, bpv: float, floor: int):
    """The records per tensor, (minexp, status, bits), against floor(bpv * n_s) bits."""
    T = tables(name, bf16, maxprec)
    return tuple(fit_floor(T[s], budget_of(bpv, t.size), floor) for s, t in enumerate(tensors(name, bf16)))


@functools.lru_cache(maxsize=None)
def _decode(name: str, bf16: bool, s: int, maxprec: int, minexp: int):
    t = tensors(name, bf16)[s]
    if t.size == 0:
        return np.zeros(0, np.float32), 0
    p = O.expert(1, 16658, maxprec, minexp)
    w, b = O.compress(t, p)
    d = O.decompress(w, (t.size,), p)
    d.setflags(write=False)
    return d, int(b)


def expect_words(name: str, bf16: bool, maxprec: int, words):
    """-> (per-tensor decodes as fp32 arrays, the summed bit count) under minexp_s = clamp(words[s], -154, 133)."""
    outs, bits = [], 0
    for s, w in enumerate(words):
        d, b = _decode(name, bf16, s, maxprec, min(max(int(w), MINEXP_LO), MINEXP_HI))
        outs.append(d)
        bits += b
    return outs, bits


def expect(name: str, bf16: bool, maxprec: int, bpv: float, floor: int = FLOOR):
    """-> (decodes, summed bit count, records) of the whole call: tables -> fits -> round trip."""
    rec = fits(name, bf16, maxprec, bpv, floor)
    outs, bits = expect_words(name, bf16, maxprec, [r[0] for r in rec])
    return outs, bits, rec


def records_array(rec) -> np.ndarray:
    """gcow_fit records as the int64[S, 2] the Python layer holds: word 0 = minexp | status << 32, word 1 = bits."""
    a = np.zeros((len(rec), 2), np.int64)
    for s, (me, st, b) in enumerate(rec):
        a[s, 0] = (me & 0xFFFFFFFF) | (st << 32)
        a[s, 1] = b
    return a
