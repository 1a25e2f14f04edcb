"""TEST INFRASTRUCTURE ONLY -- the buckets of the segmented codec (include/gcow.h "Segmented fields":
gcow_encode_seg_device, gcow_decode_mean_seg_device) and their expectation, from the oracle alone and from the
definition: the bucket is np.concatenate(relative_inputs.tensors(name, bf16)); tensor s is coded as a field of its own
under expert(1, 16658, maxprec, clamp(word_s, -154, 133)); the stream is the per-tensor O.compress outputs concatenated
bit by bit and flushed once; index entry j is the bit position of virtual block j * stride; the decode-mean is
mean_codec.mean_of over the per-stream concatenations of the per-tensor O.decompress. Shared by
tests/test_segmented_cpu.py and tests/test_gpu_segmented.py; every oracle result is computed once."""
from __future__ import annotations

import functools

import numpy as np

import fitted_per_tensor_inputs as FP
from oracle import oracle as O
from relative_inputs import tensors
from roundtrip_inputs import bf16_rne  # noqa: F401 -- the decode-mean's bf16 store, for the tests that import this

LISTS = ["edges", "small", "special", "hook"]
MINEXP_LO, MINEXP_HI = -154, 133
TILE = 1024  # virtual blocks per plan tile
# word sets: the fitted records at three budgets, every tensor at the finest / coarsest set, three sets alternating by
# tensor, and words far outside the range (the clamp)
WORD_SETS = ["fit8", "fit2.5", "fit0.5", "lo", "hi", "alt", "clamp"]
STRIDES = [0, 8, 16]


def counts(name: str):
    return [int(t.size) for t in tensors(name, False)]


def variant(name: str, bf16: bool, r: int):
    """The list's tensors as stream r's data: r = 0 as they are, 1 each tensor reversed, 2 every sign flipped."""
    ts = tensors(name, bf16)
    if r == 0:
        return list(ts)
    if r == 1:
        return [np.ascontiguousarray(t[::-1]) for t in ts]
    if bf16:
        return [t ^ np.uint16(0x8000) for t in ts]
    return [(t.view(np.uint32) ^ np.uint32(0x80000000)).view(np.float32) for t in ts]


def bucket(name: str, bf16: bool, r: int = 0) -> np.ndarray:
    return np.concatenate(variant(name, bf16, r))


@functools.lru_cache(maxsize=None)
def words(name: str, bf16: bool, ws: str, maxprec: int = 64):
    """The minexp word of every tensor (as given to the call: unclamped)."""
    n = len(counts(name))
    if ws.startswith("fit"):
        return tuple(r[0] for r in FP.fits(name, bf16, maxprec, float(ws[3:]), FP.FLOOR))
    if ws == "lo":
        return (MINEXP_LO,) * n
    if ws == "hi":
        return (MINEXP_HI,) * n
    if ws == "alt":
        return tuple((MINEXP_LO, -20, MINEXP_HI)[s % 3] for s in range(n))
    assert ws == "clamp"
    return tuple((-1000, 1000)[s % 2] for s in range(n))


def clamp(w: int) -> int:
    return min(max(int(w), MINEXP_LO), MINEXP_HI)


def concat_bits(pieces):
    """[(uint64 words, bits)] -> (the flushed stream as uint64 words, total bits, each piece's first bit): the pieces
    concatenated at bit granularity, no padding between them, zero-padded once to a 64-bit boundary."""
    acc, off, starts = 0, 0, []
    for w, b in pieces:
        starts.append(off)
        if b:
            v = int.from_bytes(np.ascontiguousarray(w, dtype=np.uint64).tobytes(), "little") & ((1 << b) - 1)
            acc |= v << off
            off += b
    nw = (off + 63) // 64
    out = np.frombuffer(acc.to_bytes(8 * nw, "little"), dtype=np.uint64).copy() if nw else np.zeros(0, np.uint64)
    return out, off, starts


@functools.lru_cache(maxsize=None)
def _tensor_stream(name: str, bf16: bool, r: int, s: int, maxprec: int, minexp: int):
    t = variant(name, bf16, r)[s]
    p = O.expert(1, 16658, maxprec, minexp)
    w, b = O.compress(t, p)
    lens = O.block_bits(t, p).astype(np.uint64)
    d = O.decompress(w, (t.size,), p)
    d.setflags(write=False)
    return w, int(b), lens, d


@functools.lru_cache(maxsize=None)
def stream(name: str, bf16: bool, wset, maxprec: int = 64, r: int = 0):
    """wset: a word-set name or a tuple of words -> (stream words, total bits, the bit position of every virtual block
    (uint64), the decode of the whole bucket as fp32); read-only."""
    ws = words(name, bf16, wset, maxprec) if isinstance(wset, str) else tuple(wset)
    pieces, lens, decs = [], [], []
    for s, n in enumerate(counts(name)):
        if not n:
            continue
        w, b, ln, d = _tensor_stream(name, bf16, r, s, maxprec, clamp(ws[s]))
        assert int(ln.sum()) == b
        pieces.append((w, b))
        lens.append(ln)
        decs.append(d)
    out, total, _ = concat_bits(pieces)
    lens = np.concatenate(lens) if lens else np.zeros(0, np.uint64)
    pos = np.concatenate([[0], np.cumsum(lens)[:-1]]).astype(np.uint64) if lens.size else np.zeros(0, np.uint64)
    dec = np.concatenate(decs) if decs else np.zeros(0, np.float32)
    for a in (out, pos, dec):
        a.setflags(write=False)
    return out, total, pos, dec


def index_of(pos: np.ndarray, stride: int) -> np.ndarray:
    return pos[::stride].copy()


def plan_model(cnts):
    """The plan restated -> (vb0[S], off[S], n[S] as gcow_seg_plan_segment reports them, [(tensor of the tile's first
    block, uniform)] per tile of 1024 virtual blocks)."""
    S = len(cnts)
    vb0, off = [0] * S, [0] * S
    v = o = 0
    for s, n in enumerate(cnts):
        vb0[s], off[s] = v, o
        v += (n + 3) // 4
        o += n
    # an empty tensor reports the next non-empty one's (or the totals)
    owner = []  # tensor of every virtual block
    for s, n in enumerate(cnts):
        owner += [s] * ((n + 3) // 4)
    tiles = []
    for t0 in range(0, v, TILE):
        s = owner[t0]
        t1 = min(t0 + TILE, v)
        tiles.append((s, t1 <= vb0[s] + cnts[s] // 4))
    return vb0, off, list(cnts), tiles, v, o
