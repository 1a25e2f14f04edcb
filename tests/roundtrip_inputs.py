"""TEST INFRASTRUCTURE ONLY -- inputs and oracle expectations shared by tests/test_roundtrip_cpu.py and
tests/test_gpu_roundtrip.py (the fused round trip, gcow_roundtrip_device in include/gcow.h)."""
from __future__ import annotations

import functools

import numpy as np

from oracle import oracle as O

MODES = {
    # the lean fixed-rate kernel
    "rate16": lambda: O.rate(16, 1), "rate8": lambda: O.rate(8, 1),
    # the no-budget kernel
    "acc1e-3": lambda: O.accuracy(1e-3), "acc1e-6": lambda: O.accuracy(1e-6), "acc0": lambda: O.accuracy(0.0),
    "prec12": lambda: O.precision(12), "expert_nobudget": lambda: O.expert(1, 160, 20, -30),
    # the generic kernel
    "rate12": lambda: O.rate(12, 1), "expert64_prec20": lambda: O.expert(64, 64, 20, -1074),
    "expert_minbits_pad": lambda: O.expert(8, 512, 32, -1074), "expert_trunc": lambda: O.expert(1, 100, 64, -30),
}
VAR_MODES = ["acc1e-3", "acc1e-6", "acc0", "prec12", "expert_nobudget"]


def bf16_trunc(a: np.ndarray) -> np.ndarray:
    """fp32 -> bf16 bits by truncation (how the test inputs are made)."""
    return (a.view(np.uint32) >> 16).astype(np.uint16)


def bf16_rne(a: np.ndarray) -> np.ndarray:
    """fp32 -> bf16 bits, round to nearest even, NaN -> 0x7fc0 (torch's conversion)."""
    u = a.view(np.uint32).astype(np.uint64)
    r = ((u + 0x7FFF + ((u >> 16) & 1)) >> 16).astype(np.uint16)
    r[(u & 0x7FFFFFFF) > 0x7F800000] = 0x7FC0
    return r


def widen(x: np.ndarray) -> np.ndarray:
    return (x.astype(np.uint32) << 16).view(np.float32) if x.dtype == np.uint16 else x


def inputs(n: int, bf16: bool, seed: int = 901) -> np.ndarray:
    """A gradient-like bucket of n values (float32, or bf16 bits as uint16) with crafted blocks spliced in from block 1
    on (from block 0, cut to n, when the bucket is a few values): all-zero blocks, subnormal maxima, NaN and +-Inf
    members, 3e38, wide-exponent and sparse blocks, and constant / alternating-sign / near-1 ramp blocks, whose long
    group phases and plane codes that cross the budget are the decoders' special lanes."""
    x = O.gen_normal(n, 1e-3, seed, True).copy()
    rng = np.random.default_rng(seed)
    blocks = [
        [0.0, 0.0, 0.0, 0.0],
        [0.0, -0.0, 0.0, -0.0],
        [1e-40, 2e-40, -3e-41, 0.0],
        [-1e-45, 0.0, 0.0, 1e-45],
        [np.nan, 1e-3, -2e-3, 3e-3],
        [1e-3, np.nan, np.nan, -1.0],
        [np.inf, -np.inf, 1e-3, 0.0],
        [1.0, 2.0, -np.inf, 4.0],
        [3e38, 3e38, 3e38, 3e38],
        [3e38, -3e38, 1.0, -1e-30],
        [1.0, 1.0, 1.0, 1.0],
        [2.0 ** -126, -(2.0 ** -126), 2.0 ** -127, 0.0],
    ]
    nbw = max(0, min(256, (n // 4 - 16) // 10))
    if nbw:
        sign = np.where(rng.random((nbw, 4)) < 0.5, -1.0, 1.0)
        wide = sign * 2.0 ** rng.uniform(-60, 10, (nbw, 4))
        sparse = np.zeros((nbw, 4))
        hit = rng.random((nbw, 4)) < 0.2
        sparse[hit] = rng.standard_normal(int(hit.sum()))
        const = np.repeat(rng.standard_normal((nbw, 1)), 4, axis=1)
        alt = np.repeat(rng.standard_normal((nbw, 1)), 4, axis=1) * np.array([1, -1, 1, -1])
        ramp = np.cumsum(rng.standard_normal((nbw, 4)) * 1e-6, axis=1) + 1.0
        sub = rng.standard_normal((nbw, 4)) * 1e-40
        zero = np.zeros((nbw // 4 + 1, 4))
        tiny = rng.standard_normal((nbw, 4)) * 2.0 ** rng.integers(-126, -90, (nbw, 1))
        with np.errstate(over="ignore", under="ignore"):
            for b in np.concatenate([wide, sparse, const, alt, ramp, sub, zero, tiny]).astype(np.float32):
                blocks.append(list(b))
    at = 4 if n >= 64 else 0
    for xb in blocks:
        m = min(4, n - at)
        if m <= 0:
            break
        x[at:at + m] = np.array(xb, np.float32)[:m]
        at += 4
    return bf16_trunc(x) if bf16 else x


@functools.lru_cache(maxsize=None)
def case(n: int, bf16: bool, mode: str):
    """-> (x, the oracle's decompress(compress(x)) as fp32, the stream's bit count); computed once, read-only."""
    op = MODES[mode]()
    x = inputs(n, bf16)
    w, bits = O.compress(x, op)
    d = O.decompress(w, (n,), op)
    x.setflags(write=False)
    d.setflags(write=False)
    return x, d, bits


def mask_identity(x: np.ndarray, op) -> np.ndarray:
    """The round trip of a stream whose budget truncates no block (minbits <= 1, maxbits >= 160), without a coder: per
    block of 4 values, the forward transform's negabinary coefficients with the planes below kmin = 32 - precision
    cleared, the inverse map and transform, then dequantisation as scale first, one fp32 multiply. x: float32, a
    multiple of 4 values."""
    assert op.minbits <= 1 and op.maxbits >= 160 and x.size % 4 == 0
    out = np.zeros(x.size, np.float32)
    NB = np.uint32(0xAAAAAAAA)
    for b in range(x.size // 4):
        f = x[4 * b:4 * b + 4]
        emax = O.block_exponent(f)
        prec = min(op.maxprec, max(0, emax - op.minexp + 4))
        if prec == 0 or emax == -127:
            continue  # the block is a single '0' bit: +0
        u = O.fwd_reorder(O.fwd_xform(O.fwd_cast(f, emax), 1), 1)
        kmin = 32 - prec if prec < 32 else 0
        u = u & np.uint32((0xFFFFFFFF << kmin) & 0xFFFFFFFF)
        q = O.inv_xform(((u ^ NB) - NB).view(np.int32), 1)
        e = emax - 30
        s = np.float32(np.ldexp(1.0, e)) if e >= -149 else np.float32(0.0)
        out[4 * b:4 * b + 4] = s * q.astype(np.float32)
    return out
