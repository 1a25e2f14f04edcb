"""TEST INFRASTRUCTURE ONLY -- the oracle's rate table, a numpy model of its one-pass construction and
the fit rule, shared by tests/test_rate_table_cpu.py, tests/test_rate_fit_hooks_cpu.py and tests/test_gpu_rate_table.py
(gcow_rate_table_device / gcow_rate_table_fit in include/gcow.h)."""
from __future__ import annotations

import functools

import numpy as np

import roundtrip_inputs as RI
from oracle import oracle as O

MINEXP_LO, ENTRIES = -154, 288


def params_at(t: int, maxprec: int) -> O.Params:
    return O.expert(1, 16658, maxprec, MINEXP_LO + t)


def oracle_bits(x: np.ndarray, maxprec: int, minexp: int) -> int:
    return int(O.compress(x, O.expert(1, 16658, maxprec, minexp))[1])


def oracle_table(x: np.ndarray, maxprec: int) -> np.ndarray:
    """table[t] = the oracle's unflushed stream length of x under expert(1, 16658, maxprec, -154 + t): 288 encodes."""
    if x.size == 0:
        return np.zeros(ENTRIES, np.int64)
    return np.array([oracle_bits(x, maxprec, MINEXP_LO + t) for t in range(ENTRIES)], np.int64)


@functools.lru_cache(maxsize=None)
def crafted_table(n: int, bf16: bool, maxprec: int):
    """(x, oracle_table(x, maxprec)) for the crafted bucket roundtrip_inputs.inputs(n, bf16); computed once, read-only."""
    x = RI.inputs(n, bf16)
    t = oracle_table(x, maxprec)
    x.setflags(write=False)
    t.setflags(write=False)
    return x, t


def _clz(v: int) -> int:
    return 32 - int(v).bit_length()


def model_table(x: np.ndarray, maxprec: int) -> np.ndarray:
    """The construction the kernel implements, block by block: two 288-bin histograms (steps and impulses of the first
    difference of each block's length over the table index), then two suffix sums. x: fp32 or bf16 bits, a multiple of
    4 values."""
    f = RI.widen(x)
    assert f.size % 4 == 0
    nb = f.size // 4
    step = np.zeros(ENTRIES, np.int64)
    imp = np.zeros(ENTRIES, np.int64)
    pmax = min(maxprec, 32)

    def add(h, t, v):
        if t >= 0:  # updates below the table are dropped (the step end of an emax = -126 block, at -1)
            h[t] += v

    for b in range(nb):
        blk = f[4 * b:4 * b + 4]
        e = O.block_exponent(blk)
        if e == -127 or pmax == 0:
            continue  # one bit under every minexp
        a = e + 158
        u = [int(v) for v in O.fwd_reorder(O.fwd_xform(O.fwd_cast(blk, e), 1), 1)]
        S = [u[0] | u[1] | u[2] | u[3], u[1] | u[2] | u[3], u[2] | u[3]]
        z = [_clz(s) for s in S]
        bit = [(u[j] >> (31 - z[j])) & 1 if z[j] < 32 else 0 for j in range(3)]
        l1 = 13 - sum(min(zj, 1) for zj in z) + sum(bit[j] for j in range(3) if z[j] <= 0)
        add(imp, a - 1, l1 - 1)
        start = 1 + sum(1 for zj in z if zj <= 1)
        add(step, a - 2, start)
        level = start
        for j in range(3):
            if 1 <= z[j] <= pmax - 1:
                add(imp, a - 1 - z[j], bit[j])
            if 2 <= z[j] <= pmax - 1:
                add(step, a - 1 - z[j], 1)
                level += 1
        add(step, a - 1 - pmax, -level)
    F = np.cumsum(step[::-1])[::-1] + imp
    return nb + np.cumsum(F[::-1])[::-1]


def fit(table, budget_bits: int):
    """gcow_rate_table_fit restated: the smallest minexp in [-154, 133] whose entry is <= budget_bits, and the entry;
    None when even the last entry (one bit per block) is above the budget."""
    for t in range(ENTRIES):
        if int(table[t]) <= budget_bits:
            return MINEXP_LO + t, int(table[t])
    return None
