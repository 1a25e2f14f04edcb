"""TEST INFRASTRUCTURE ONLY -- a numpy model of the device fit (gcow_rate_table_fit_device, include/gcow.h), of the
clamp the fitted calls apply to their minexp word, synthetic rate tables and the budget sweep, shared by
tests/test_fit_device_cpu.py, tests/test_fit_on_device_hooks_cpu.py and tests/test_gpu_fit_device.py."""
from __future__ import annotations

import numpy as np

MINEXP_LO, MINEXP_HI, ENTRIES = -154, 133, 288
U64_MAX = (1 << 64) - 1


def model_fit(table, budget_bits: int):
    """The kernel's rule: a min over the indices whose entry fits; none fits -> the last entry, status 1.
    -> (minexp, status, bits)."""
    t = np.asarray(table).astype(np.uint64)
    assert t.size == ENTRIES
    fits = np.nonzero(t <= np.uint64(budget_bits))[0]
    best = int(fits.min()) if fits.size else ENTRIES
    status = int(best == ENTRIES)
    best = min(best, ENTRIES - 1)
    return MINEXP_LO + best, status, int(t[best])


def clamp(word: int) -> int:
    """The minexp the fitted kernels use for a device word."""
    return min(max(int(word), MINEXP_LO), MINEXP_HI)


def pack_record(minexp: int, status: int, bits: int) -> np.ndarray:
    """A gcow_fit record as two little-endian int64 words."""
    w0 = (minexp & 0xFFFFFFFF) | (status << 32)
    return np.array([w0, bits], np.uint64).view(np.int64)


def plateau_table() -> np.ndarray:
    """Non-increasing, with runs of equal entries of lengths 1 .. 7 (ties: the fit takes a run's first index), ending
    in a plateau like a real table's last two entries."""
    rng = np.random.default_rng(288)
    vals, v = [], 5_000_000
    while len(vals) < ENTRIES:
        run = int(rng.integers(1, 8))
        vals += [v] * run
        v -= int(rng.integers(1, 40_000))
    t = np.array(vals[:ENTRIES], np.int64)
    t[-2:] = t[-1]
    assert np.all(np.diff(t) <= 0) and t[-1] > 1
    return t


def constant_table() -> np.ndarray:
    return np.full(ENTRIES, 4099, np.int64)


def decreasing_table() -> np.ndarray:
    return (np.arange(ENTRIES, 0, -1, dtype=np.int64) * 1013 + 7)


def huge_table() -> np.ndarray:
    """Entries above 2^63: the comparison is unsigned."""
    t = (np.arange(ENTRIES, 0, -1, dtype=np.uint64) << np.uint64(55)) + np.uint64(3)
    assert int(t[0]) > 1 << 63
    return t.view(np.int64)


def budgets(table) -> list[int]:
    """Every entry, each +- 1, 0 and 2^64 - 1 (within uint64)."""
    out = {0, U64_MAX}
    for v in np.asarray(table).astype(np.uint64).tolist():
        for b in (v - 1, v, v + 1):
            if 0 <= b <= U64_MAX:
                out.add(int(b))
    return sorted(out)
