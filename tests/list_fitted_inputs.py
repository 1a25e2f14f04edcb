"""TEST INFRASTRUCTURE ONLY -- inputs and oracle expectations shared by tests/test_list_fitted_cpu.py and
tests/test_gpu_list_fitted.py (the bit budget over a tensor list: gcow_rate_table_list_device and
gcow_roundtrip_list_fitted_device in include/gcow.h). The lists are the seam lists of roundtrip_list_inputs.py, the
tables and the fit rule those of rate_table_inputs.py; everything the oracle computes is computed once and shared."""
from __future__ import annotations

import functools
import math

import numpy as np

from oracle import oracle as O
from rate_table_inputs import ENTRIES, MINEXP_LO, fit, oracle_table
from roundtrip_list_inputs import CHUNK, seam_field, seam_sizes  # noqa: F401  (re-exported for the tests)

MINEXP_HI = MINEXP_LO + ENTRIES - 1  # 133
SENT = -1234.5  # exact in bf16 too
TAIL = 16
POISON = 0x5A5A5A5A5A5A5A5A  # fills the table and the workspace before every table call
SINGLE_SIZES = [1, 3, 4, 5, CHUNK - 1, CHUNK, CHUNK + 1, 3 * CHUNK + 5]


def clamp(w: int) -> int:
    return min(max(int(w), MINEXP_LO), MINEXP_HI)


def layout(sizes, aligned: bool):
    """Element positions of the tensors in one buffer (test_gpu_roundtrip_list.py's carve): gaps of at least 3
    elements; aligned: every base a multiple of 8 elements (16 bytes for bf16, 32 for fp32), else every base at an odd
    element offset (for bf16: off 4 bytes). -> (positions, buffer length with TAIL elements after the last tensor)."""
    pos, at = [], 8 if aligned else 1
    for n in sizes:
        pos.append(at)
        at += n + 3
        at = (at + 7) // 8 * 8 if aligned else at | 1
    return pos, at + TAIL


@functools.lru_cache(maxsize=None)
def seam_table(r: int, bf16: bool, maxprec: int) -> np.ndarray:
    """oracle_table(seam_field(r, bf16), maxprec): about a second of oracle time, computed once, read-only."""
    t = oracle_table(seam_field(r, bf16), maxprec)
    t.setflags(write=False)
    return t


@functools.lru_cache(maxsize=None)
def single_table(n: int, bf16: bool, maxprec: int) -> np.ndarray:
    """The oracle's table of the first n values of seam_field(1, bf16)."""
    t = oracle_table(np.array(seam_field(1, bf16)[:n]), maxprec)
    t.setflags(write=False)
    return t


@functools.lru_cache(maxsize=None)
def seam_roundtrip(r: int, bf16: bool, maxprec: int, minexp: int):
    """-> (the oracle's decompress(compress(X, expert(1, 16658, maxprec, minexp))) as fp32, the stream's bit count)."""
    op = O.expert(1, 16658, maxprec, minexp)
    x = seam_field(r, bf16)
    w, bits = O.compress(x, op)
    d = O.decompress(w, (x.size,), op)
    d.setflags(write=False)
    return d, int(bits)


def fit_record(table, budget_bits: int):
    """The gcow_fit record gcow_rate_table_fit_device writes: (minexp, status, bits)."""
    got = fit(table, budget_bits)
    return (got[0], 0, got[1]) if got is not None else (MINEXP_HI, 1, int(table[ENTRIES - 1]))


def budget_of(bits_per_value: float, n: int) -> int:
    return int(math.floor(bits_per_value * n))


def budgets(table, n: int) -> list[int]:
    """The budgets of the fitted round trip's parity test: one below the last entry (no fit), the last entry, the
    entry fitted at 8 bits per value and one bit below it (which moves the fit to the next distinct entry),
    2.5 bits per value, and the first entry (minexp -154)."""
    tstar = fit(table, budget_of(8.0, n))[0] - MINEXP_LO
    at, below = int(table[tstar]), int(table[tstar]) - 1
    assert fit(table, at)[0] == MINEXP_LO + tstar
    nxt = fit(table, below)
    assert nxt is not None and nxt[0] > MINEXP_LO + tstar and nxt[1] < at  # the next distinct entry
    return [int(table[ENTRIES - 1]) - 1, int(table[ENTRIES - 1]), at, below, budget_of(2.5, n), int(table[0])]
