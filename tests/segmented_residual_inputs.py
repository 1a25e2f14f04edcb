"""TEST INFRASTRUCTURE ONLY -- error feedback under per-tensor budgets (include/gcow.h "Segmented fields with a
residual": gcow_rate_table_seg_device, gcow_encode_seg_residual_device) and its expectation, from the oracle and the
definition alone: tensor s of the bucket with its slice e_s of the carried error is residual_model.model_step(t_s, e_s,
expert(1, 16658, maxprec, clamp(word_s, -154, 133))) -- y = x + e by one fp32 add, the oracle's stream of the fp32 y,
e' = y - decode with non-finite results +0 --, the stream is the tensors' streams concatenated by
segmented_inputs.concat_bits, table row s is rate_table_inputs.oracle_table(y_s, maxprec), and a record is
fitted_per_tensor_inputs.fit_floor of that row against budget_of(bits_per_value, n_s).

The two steps. Step 1 (step = 0): segmented_inputs.variant(name, bf16, 0) with no carried error. Step 2 (step = 1):
variant(name, bf16, 1) -- every tensor reversed -- with e = step 1's residual under the "fit8" words. A chain at another
budget (chain()) carries its own residual instead. Every oracle result is computed once; arrays are read-only. Shared
by tests/test_segmented_residual_cpu.py and tests/test_gpu_segmented_residual.py."""
from __future__ import annotations

import functools

import numpy as np

import fitted_per_tensor_inputs as FP
import segmented_inputs as SI
from oracle import oracle as O
from rate_table_inputs import oracle_table
from residual_model import model_step, widen

LISTS = SI.LISTS
WORD_SETS = ["fit8", "lo", "hi", "alt", "clamp"]
STRIDES = SI.STRIDES
STEPS = [0, 1]


def offsets(name: str):
    c = SI.counts(name)
    return [int(o) for o in np.cumsum([0] + c[:-1])]


def _ro(a):
    a.setflags(write=False)
    return a


@functools.lru_cache(maxsize=None)
def _tensor(x_key, e_key, maxprec: int, minexp: int):
    """model_step of one tensor; the keys are (name, bf16, variant, s) and a hashable handle of e (None: zeros)."""
    name, bf16, r, s = x_key
    x = SI.variant(name, bf16, r)[s]
    e = None if e_key is None else _error_of(e_key)[s]
    p = O.expert(1, 16658, maxprec, minexp)
    y, w, bits, d, res = model_step(x, e, p)
    with np.errstate(all="ignore"):
        lens = O.block_bits(y, p).astype(np.uint64)
    assert int(lens.sum()) == bits
    return _ro(y), w, int(bits), lens, _ro(d), _ro(res)


@functools.lru_cache(maxsize=None)
def _error_of(e_key):
    """e_key = (name, bf16, bpv): the per-tensor residuals step 1 leaves under the records fitted at bpv bits per value
    (8.0: the "fit8" words -- y = x + 0 has x's tables)."""
    name, bf16, bpv = e_key
    recs = fits_y(name, bf16, 0, bpv)
    out = []
    for s, n in enumerate(SI.counts(name)):
        out.append(_tensor((name, bf16, 0, s), None, 64, SI.clamp(recs[s][0]))[5] if n else np.zeros(0, np.float32))
    return tuple(out)


def _ekey(name, bf16, step, bpv=8.0):
    return None if step == 0 else (name, bf16, float(bpv))


def x_bucket(name: str, bf16: bool, step: int) -> np.ndarray:
    return SI.bucket(name, bf16, step)


def e_bucket(name: str, bf16: bool, step: int, bpv: float = 8.0):
    """The carried error a step starts from: None for step 1, step 1's residual for step 2."""
    if step == 0:
        return None
    return _ro(np.concatenate(_error_of(_ekey(name, bf16, 1, bpv))).astype(np.float32))


@functools.lru_cache(maxsize=None)
def y_tensors(name: str, bf16: bool, step: int, bpv: float = 8.0):
    out = []
    for s, x in enumerate(SI.variant(name, bf16, step)):
        e = None if step == 0 else _error_of(_ekey(name, bf16, 1, bpv))[s]
        with np.errstate(over="ignore", invalid="ignore"):
            out.append(_ro((widen(x) + (0 if e is None else e)).astype(np.float32)))
    return tuple(out)


@functools.lru_cache(maxsize=None)
def tables_y(name: str, bf16: bool, step: int, maxprec: int = 64, bpv: float = 8.0) -> np.ndarray:
    """int64[S, 288]: row s = oracle_table(y_s, maxprec), zeros for an empty tensor."""
    with np.errstate(all="ignore"):
        return _ro(np.stack([oracle_table(np.array(y), maxprec) for y in y_tensors(name, bf16, step, bpv)]))


@functools.lru_cache(maxsize=None)
def fits_y(name: str, bf16: bool, step: int, bpv: float = 8.0, floor: int = FP.FLOOR, maxprec: int = 64):
    """The records per tensor (minexp, status, bits) of y against floor(bpv * n_s) bits; step 2 carries the residual
    of step 1 at the same bpv."""
    if step == 0:  # no recursion: y = x + 0
        ys = y_tensors(name, bf16, 0)
        with np.errstate(all="ignore"):
            T = [oracle_table(np.array(y), maxprec) for y in ys]
    else:
        T = tables_y(name, bf16, 1, maxprec, bpv)
    return tuple(FP.fit_floor(T[s], FP.budget_of(bpv, n), floor) for s, n in enumerate(SI.counts(name)))


@functools.lru_cache(maxsize=None)
def model(name: str, bf16: bool, step: int, wset, maxprec: int = 64, bpv: float = 8.0):
    """wset: a word-set name of segmented_inputs (the words of the bucket x of step 1, as given to the call) or a tuple
    of words -> (stream words, total bits, the bit position of every virtual block, the residual e' of the whole
    bucket, the decode of the whole bucket); read-only."""
    ws = SI.words(name, bf16, wset, maxprec) if isinstance(wset, str) else tuple(wset)
    pieces, lens, res, dec = [], [], [], []
    for s, n in enumerate(SI.counts(name)):
        if not n:
            continue
        _, w, b, ln, d, r = _tensor((name, bf16, step, s), _ekey(name, bf16, step, bpv), maxprec, SI.clamp(ws[s]))
        pieces.append((w, b))
        lens.append(ln)
        res.append(r)
        dec.append(d)
    out, total, _ = SI.concat_bits(pieces)
    lens = np.concatenate(lens) if lens else np.zeros(0, np.uint64)
    pos = np.concatenate([[0], np.cumsum(lens)[:-1]]).astype(np.uint64) if lens.size else np.zeros(0, np.uint64)
    res = np.concatenate(res) if res else np.zeros(0, np.float32)
    dec = np.concatenate(dec) if dec else np.zeros(0, np.float32)
    return _ro(out), total, _ro(pos), _ro(res.astype(np.float32)), _ro(dec.astype(np.float32))


def chain(name: str, bf16: bool, step: int, bpv: float, maxprec: int = 64):
    """PerTensorFittedResidualEncoder's step at bpv bits per value -> (records, model(...) under the records' words)."""
    recs = fits_y(name, bf16, step, bpv, FP.FLOOR, maxprec)
    return recs, model(name, bf16, step, tuple(r[0] for r in recs), maxprec, bpv)


@functools.lru_cache(maxsize=None)
def differing(name: str, bf16: bool):
    """(rows of step 2's table of y that differ from the table of its x alone, fitted minexp at 8 bits per value that
    differ): what a table or an encode that ignored e would get wrong."""
    with np.errstate(all="ignore"):
        Tx = np.stack([oracle_table(np.array(widen(x)), 64) for x in SI.variant(name, bf16, 1)])
    Ty = tables_y(name, bf16, 1)
    rows = int((Tx != Ty).any(axis=1).sum())
    fy = fits_y(name, bf16, 1)
    fx = [FP.fit_floor(Tx[s], FP.budget_of(8.0, n), FP.FLOOR) for s, n in enumerate(SI.counts(name))]
    return rows, sum(1 for a, b in zip(fx, fy) if a[0] != b[0])


def check_differs(name: str, bf16: bool):
    rows, nfits = differing(name, bf16)
    assert rows >= 1, (name, bf16)
    if name in ("edges", "special", "small"):
        assert nfits >= 1, (name, bf16)
    return rows, nfits
