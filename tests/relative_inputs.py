"""TEST INFRASTRUCTURE ONLY -- the tensor lists of the round trip with a tolerance relative to each tensor
(gcow_roundtrip_rel_* in include/gcow.h) and their expectation, computed tensor by tensor with the oracle from the
definition: a_s = the largest finite |t_s|, emax_s = (bits(a_s) >> 23) - 126, minexp_s = max(emax_s - k, -94) (capped
for emax_s = 128 so that the decode stays finite: minexp_of),
p_s = expert(1, 16658, maxprec, minexp_s), out_s = decompress(compress(t_s, p_s)). Shared by
tests/test_roundtrip_rel_cpu.py and tests/test_gpu_roundtrip_rel.py."""
from __future__ import annotations

import functools

import numpy as np

from oracle import oracle as O
from roundtrip_inputs import bf16_trunc, widen

CHUNK = 8192       # values per direct chunk: 256 lanes x 8 blocks x 4 values
MIN_DIRECT = 256   # whole blocks below which a tensor has no direct chunk
MINEXP_FLOOR = -94
HEADROOM = 2
KS = [0, 8, 24]
MAXPRECS = [64, 12]
LISTS = ["edges", "small", "special"]

EDGE_SIZES = [1, 3, 4, 5, 0, 8191, 8192, 8193, 24583, 2, 7]
HOOK_SIZES = [8193, 5, 24583]
SMALL_SIZES =[1 + i % 9 for i in range(150)] + [8192] + [1 + i % 9 for i in range(150, 299)]


def _scaled(rng, n, lo=-40, hi=10):
    """n normal values times the tensor's own power of two: a wrong tensor's exponent changes bits."""
    return (rng.standard_normal(n) * 2.0 ** int(rng.integers(lo, hi + 1))).astype(np.float32)


@functools.lru_cache(maxsize=None)
def tensors(name: str, bf16: bool):
    """The list as read-only arrays: float32, or bf16 bits as uint16 (made by truncation)."""
    rng = np.random.default_rng({"edges": 11, "small": 12, "special": 13, "hook": 14}[name])
    if name == "edges":
        ts = [_scaled(rng, n) for n in EDGE_SIZES]
    elif name == "hook":  # a gradient bucket's per-parameter views (test_gpu_roundtrip_rel.py)
        ts = [_scaled(rng, n) for n in HOOK_SIZES]
    elif name == "small":
        assert len(SMALL_SIZES) == 300
        ts = [_scaled(rng, n) for n in SMALL_SIZES]
    else:
        spliced = _scaled(rng, 4100)
        spliced[[0, 5, 1030, 4099]] = np.inf, -np.inf, np.nan, np.nan   # whole blocks 0, 1, 257 and the partial last
        spliced[2048:2052] = np.nan                                      # a block of NaN only
        # the largest finite value among values of scale 3e38: the headroom cap at its tightest (minexp_s = 102)
        top = (rng.uniform(-1.0, 1.0, 64) * 3e38).astype(np.float32)
        top[[3, 40]] = np.finfo(np.float32).max, -np.finfo(np.float32).max
        with np.errstate(over="ignore", under="ignore"):
            ts = [np.zeros(64, np.float32),
                  np.full(8, np.nan, np.float32),
                  spliced,
                  (rng.standard_normal(16) * 1e-40).astype(np.float32),
                  (rng.standard_normal(64) * 2.0 ** -100).astype(np.float32),
                  (rng.uniform(-1.0, 1.0, 64) * 3e38).astype(np.float32),
                  np.full(64, -0.0, np.float32),
                  top]
    out = []
    for t in ts:
        t = bf16_trunc(t) if bf16 else t
        t.setflags(write=False)
        out.append(t)
    return out


def absmax_of(t: np.ndarray) -> np.float32:
    """The largest finite magnitude (+0 if there is none)."""
    a = np.abs(widen(t))
    a = a[np.isfinite(a)]
    return np.float32(a.max()) if a.size else np.float32(0.0)


def minexp_of(a: np.float32, k: int) -> int:
    """minexp_s of a tensor whose largest finite magnitude is a. For a maximum in the top binade (emax_s = 128) it is
    capped at floor(log2(2^128 - a)) - 2, so that a + 2^minexp_s stays below fp32's rounding boundary to Inf."""
    bits = int(np.array([a], np.float32).view(np.uint32)[0])
    emax = (bits >> 23) - 126
    m = max(emax - k, MINEXP_FLOOR)
    if emax == 128:
        gap = (1 << 24) - ((bits & 0x7FFFFF) | 0x800000)   # 2^128 - a in units of 2^104
        m = min(m, 104 + gap.bit_length() - 1 - HEADROOM)
    return m


@functools.lru_cache(maxsize=None)
def expect(name: str, bf16: bool, k: int, maxprec: int):
    """-> (per-tensor decodes as fp32 arrays, absmax as a float32 array, the summed bit count); read-only."""
    outs, amax, bits = [], [], 0
    for t in tensors(name, bf16):
        a = absmax_of(t)
        amax.append(a)
        if t.size == 0:
            outs.append(np.zeros(0, np.float32))
            continue
        p = O.expert(1, 16658, maxprec, minexp_of(a, k))
        w, b = O.compress(t, p)
        d = O.decompress(w, (t.size,), p)
        d.setflags(write=False)
        outs.append(d)
        bits += b
    return outs, np.array(amax, np.float32), bits
