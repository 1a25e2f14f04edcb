"""TEST INFRASTRUCTURE ONLY -- the case table, inputs and oracle expectations of the encoder contract tests
(test_encode_contract_cpu.py checks what the inputs claim, test_gpu_encode_contract.py runs them): every encoder of
gcow_encode_device / gcow_encode_device_append into buffers that are not zero, called twice on the same buffers, and
every decoder into an output with guard elements around it.

Data of every case (field): N(0, 1e-2) fp32 from the case's seed, about a third of the slowest axis scaled by 1e-3,
every 97th value zero, a few whole all-zero blocks, the tiny and subnormal members of test_random_all_dims; the small
N-D cases also one block each with +Inf, -Inf and NaN. bf16 inputs are the fp32 ones truncated to the upper 16 bits.
The second input of a case has the same shape and a shorter stream: other values, scaled by 2^-3 for accuracy sets, a
quarter of the blocks zeroed otherwise (at fixed rate the length is the shape's; the values differ all the same).

A seed is the crc32 of the input's name plus its entry in SEED_STEPS (0 when it has none); an entry is there because
the stream of the seed before it misses a property test_encode_contract_cpu.py asserts (it ends on an even 32-bit
word, say). That test decides whether a seed is acceptable."""
from __future__ import annotations

import collections
import functools
import zlib

import numpy as np

from oracle import oracle as O

PATTERNS = {"ones": -1, "5a": 0x5A5A5A5A5A5A5A5A}  # int64 fill values: all ones; the project's sentinel word
MULTI_BLOCKS = 2048 * 256        # gcow_api.cpp make_plan: a range has more than one 256-block tile above this
E3V_WIN_WORDS = 64 * 1536 // 32 + 2   # gcow_blocks.hip: the LDS window of k_encode3d_var
TINY = np.array([1e-36, -2e-38, 7e-39, 0], np.float32)

PSETS = {
    "rate16": lambda d: O.rate(16, d), "rate8": lambda d: O.rate(8, d), "rate12": lambda d: O.rate(12, d),
    "rate2.5": lambda d: O.rate(2.5, d), "rate32": lambda d: O.rate(32, d), "rate1": lambda d: O.rate(1, d),
    "rate3.0625": lambda d: O.rate(3.0625, d), "rate2.51": lambda d: O.rate(2.51, d),
    "acc1e-3": lambda d: O.accuracy(1e-3), "acc1e-4": lambda d: O.accuracy(1e-4),
    "prec20": lambda d: O.precision(20), "prec32": lambda d: O.precision(32),
    "expert20_160": lambda d: O.expert(20, 160, 20, -30), "expert1_80": lambda d: O.expert(1, 80, 20, -30),
}

# id: the test id. field: the name of the input (cases that share it share the oracle's work). view: how the device
# tensor is laid out ("stride3": every third element of a 1-D buffer; "transposed": the 2-D field stored column by
# column). form: the 1-D variable-rate encoder's form (codec.var1d_variant). strides: the index strides the case runs
# with (0: no index). patterns: the fills of the buffers before the first call.
Case = collections.namedtuple("Case", "id field shape pset dtype view form strides patterns multi")

N_MULTI_1D = 4 * 524289 + 3
SHAPE_MULTI_2D = (2898, 2899)
SHAPE_OVERSIZED_3D = (24, 40, 64)


def _case(group, shape, pset, dtype="f32", view=None, form=None, index=None, patterns=("ones", "5a"), multi=False):
    fixed = pset.startswith("rate")
    strides = (1, 2) if (not fixed or index) else (0,)
    dims = "x".join(str(s) for s in shape)
    # fixed-rate cases of a shape share one input; a variable-rate case has its own, so that its seed can be chosen
    # for its stream (module docstring); a view shares the input of the dense case
    field = "%s-%s" % (group, dims) if fixed else "%s-%s-%s-%s" % (group, dims, pset, dtype)
    cid = "-".join([group, dims, pset, dtype] + [v for v in (view, form, "index" if fixed and index else None) if v])
    return Case(cid, field, tuple(shape), pset, dtype, view, form, strides, tuple(patterns), multi)


def _table():
    c = []
    # fast 1-D fixed rate (enc_fixed1d.hip): 1 and 2049 blocks are odd counts (rate 8 clears half a word), 2 and 2050
    # even ones
    for r in ("rate16", "rate8"):
        for n in (1, 5, 4 * 2048 + 3, 4 * 2049 + 3):
            for dt in ("f32", "bf16"):
                c.append(_case("fast1d", (n,), r, dt))
    # 1-D fixed rate through k_encode_tiles: two ranges of 256 blocks
    n = 4 * 257 + 1
    for r in ("rate12", "rate2.5", "rate32"):
        c.append(_case("tiles1d", (n,), r))
    c.append(_case("tiles1d", (n,), "rate16", index=True))
    c.append(_case("tiles1d", (n,), "rate16", view="stride3"))
    # 1-D variable rate without a budget (var1d.hip, enc1d_range.hip): three tiles of 1024 blocks and a ragged fourth
    n = 4 * (3 * 1024 + 5) + 1
    for ps in ("acc1e-3", "prec20"):
        for dt in ("f32", "bf16"):
            for form in (None, "range", "single_pass"):
                c.append(_case("var1d", (n,), ps, dt, form=form))
    # 1-D generic variable rate (k_count, k_scan_ranges, k_encode_tiles)
    n = 4 * 257 + 1
    c.append(_case("gen1d", (n,), "expert20_160"))
    c.append(_case("gen1d", (n,), "expert20_160", "bf16"))
    c.append(_case("gen1d", (n,), "expert1_80"))
    c.append(_case("multi1d", (N_MULTI_1D,), "expert20_160", multi=True))
    c.append(_case("multi1d", (N_MULTI_1D,), "expert1_80", multi=True))
    # 2-D: one range (140 blocks) and two (306 blocks)
    for shape in ((37, 53), (66, 70)):
        for ps in ("acc1e-3", "prec20", "prec32", "expert20_160", "rate8", "rate2.5", "rate1", "rate3.0625"):
            c.append(_case("d2", shape, ps))
            c.append(_case("d2", shape, ps, "bf16"))
            c.append(_case("d2", shape, ps, view="transposed"))
    for ps in ("acc1e-3", "prec20"):
        c.append(_case("multi2d", SHAPE_MULTI_2D, ps, patterns=("ones",), multi=True))
    # 3-D: the word path, the generic fixed-rate path, fixed rate with an index, 64-block tiles, oversized tiles
    c.append(_case("d3", (13, 17, 21), "rate8"))
    c.append(_case("d3", (13, 17, 21), "rate2.5"))
    c.append(_case("d3", (13, 17, 21), "rate8", index=True))
    c.append(_case("d3", (13, 17, 21), "acc1e-3"))
    c.append(_case("oversized3d", SHAPE_OVERSIZED_3D, "prec32"))
    # 4-D: one wave per block. Rate 2.5 is 640 bits, whole words; rate 2.51 is 643 bits, so that blocks share words
    # (the encoder clears the whole bound first)
    for ps in ("rate8", "rate2.5", "rate2.51", "acc1e-4", "prec20"):
        c.append(_case("d4", (6, 5, 7, 10), ps))
    c.append(_case("d4", (6, 5, 7, 10), "acc1e-3", "bf16"))
    return c


CASES = _table()
SMALL_CASES = [c for c in CASES if not c.multi]
MULTI_CASES = [c for c in CASES if c.multi]

# gcow_encode_device_append: (id, field name, shape, parameter set, cuts along the slowest axis, zero_start). Every
# list of cuts has an empty chunk and a chunk of one row of blocks. zero_start: the cut (or None) whose chunk begins
# with all-zero blocks, one bit each, at a base inside a 32-bit word: the chunk's second block then starts in the word
# that holds the end of the stream before the chunk, which the scan of a 4-D chunk (one range per block) must not zero.
AppendCase = collections.namedtuple("AppendCase", "id field shape pset cuts zero_start")
APPEND_CASES = [
    AppendCase("append1d", "append1d", (4 * 3001 + 2,), "expert20_160",
               (0, 4 * 700, 4 * 701, 4 * 701, 4 * 2500, 4 * 3001 + 2), None),
    AppendCase("append2d", "append2d", (66, 70), "acc1e-3", (0, 4, 4, 36, 66), None),
    AppendCase("append3d", "oversized3d-append", SHAPE_OVERSIZED_3D, "prec32", (0, 4, 4, 12, 20, 24), 4),
    AppendCase("append4d", "append4d", (6, 5, 7, 12), "acc1e-4", (0, 4, 4, 6), None),
    AppendCase("append4d_zero", "append4d-zerostart", (6, 5, 7, 12), "acc1e-4", (0, 4, 4, 6), 4),
]

# added to crc32(name): see the module's docstring. To re-derive an entry after a rename or a change of a shape or
# a parameter set: drop it, run test_encode_contract_cpu.py, and for every input whose tests fail count the step up
# from 0 until they pass (the properties are the oracle's, so the search needs no GPU).
SEED_STEPS = {
    "var1d-12309-acc1e-3-f32": 2, "var1d-12309-prec20-f32": 1, "gen1d-1029-expert1_80-f32": 8,
    "multi1d-2097159-expert20_160-f32": 4, "d2-37x53-acc1e-3-bf16": 1, "d2-37x53-prec32-bf16": 3,
    "d2-37x53-expert20_160-f32": 64, "d2-37x53-expert20_160-bf16": 18, "d2-66x70-acc1e-3-f32": 3,
    "d2-66x70-acc1e-3-bf16": 1, "d2-66x70-prec32-f32": 3, "d2-66x70-prec32-bf16": 3, "d3-13x17x21-acc1e-3-f32": 1,
    "d4-6x5x7x10-acc1e-4-f32": 1, "d4-6x5x7x10-acc1e-3-bf16": 4, "multi2d-2898x2899-prec20-f32": 1,
    "oversized3d-24x40x64-prec32-f32": 2, "append1d": 2,
}


def params(pset, dims):
    return PSETS[pset](dims)


def is_fixed(pset):
    return pset.startswith("rate")


def bf16_trunc(a):
    return (a.view(np.uint32) >> 16).astype(np.uint16)


def nblocks(shape):
    n = 1
    for s in shape:
        n *= (s + 3) // 4
    return n


def block_ids(shape):
    """The stream-order block number (the last axis fastest) of every element, as an array of the field's shape."""
    bid = np.zeros(shape, np.int64)
    mul = 1
    for ax in range(len(shape) - 1, -1, -1):
        idx = np.arange(shape[ax]) // 4 * mul
        bid += idx.reshape([-1 if a == ax else 1 for a in range(len(shape))])
        mul *= (shape[ax] + 3) // 4
    return bid


def range_blocks(shape, pset):
    """Blocks per range of the variable-rate encoders (gcow_api.cpp make_plan; 4-D scans every block)."""
    dims = len(shape)
    if dims == 4:
        return 1
    if dims == 3:
        return 64
    r = (nblocks(shape) + 2047) // 2048
    return max((r + 255) // 256 * 256, 256)


def seed_of(name, second=False):
    return zlib.crc32((name + ("#2" if second else "")).encode()) + (0 if second else SEED_STEPS.get(name, 0))


def _zero_runs(name, nb):
    if name.startswith("multi"):
        return [(1000, 1300), (300000, 300700)]
    if name == "append4d-zerostart":  # the first two blocks of the chunk that starts at row 4 (12 blocks per row)
        return [(12, 14)]
    return []


@functools.lru_cache(maxsize=None)
def field(name, shape, shrink=None):
    """The fp32 input `name` of `shape` (read-only). shrink: None for the first input, "scale" / "zero" for the
    second (module docstring)."""
    shape = tuple(shape)
    rng = np.random.default_rng(seed_of(name, shrink is not None))
    if name.startswith("oversized3d"):
        # the field of test_3d_var_oversized_tiles: zero slabs between near-lossless noise
        a = (rng.standard_normal(shape) * 1e-2).astype(np.float32)
        a[4:12] = 0
        a[16:20, :, :32] = 0
    else:
        a = (rng.standard_normal(shape) * 1e-2).astype(np.float32)
        s0 = shape[0]
        a[s0 // 3: s0 // 3 + (s0 + 2) // 3] *= np.float32(1e-3)
        flat = a.reshape(-1)
        flat[96::97] = 0
        k = max(0, min(4, flat.size - 5))
        flat[5:5 + k] = TINY[:k]
        nb = nblocks(shape)
        bid = block_ids(shape)
        pick = rng.choice(nb, size=min(nb, 6), replace=False)
        for b in pick[:min(3, nb // 8)]:
            a[bid == b] = 0
        if len(shape) >= 2 and nb >= 16 and not name.startswith("multi"):
            for b, v in zip(pick[3:6], (np.inf, -np.inf, np.nan)):
                at = np.argwhere(bid == b)
                a[tuple(at[len(at) // 2])] = v
        for lo, hi in _zero_runs(name, nb):
            a[(bid >= lo) & (bid < hi)] = 0
    if shrink == "scale":
        a *= np.float32(0.125)
    elif shrink == "zero":
        a[block_ids(shape) % 4 == 1] = 0
    a.setflags(write=False)
    return a


def case_input(c, second=False):
    """The host array of a case's first or second input: float32, or bf16 bits as uint16."""
    shrink = None if not second else ("scale" if c.pset.startswith("acc") else "zero")
    a = field(c.field, c.shape, shrink)
    return _typed(a, c.dtype)


def _typed(a, dtype):
    if dtype == "f32":
        return a
    b = bf16_trunc(a)
    b.setflags(write=False)
    return b


Ref = collections.namedtuple("Ref", "words bits lens offs")


@functools.lru_cache(maxsize=None)
def _reference(name, shape, shrink, dtype, pset):
    a = _typed(field(name, shape, shrink), dtype)
    op = params(pset, len(shape))
    w, bits = O.compress(a, op)
    lens = O.block_bits(a, op).astype(np.uint64)
    offs = np.concatenate([[0], np.cumsum(lens)]).astype(np.uint64)
    assert int(offs[-1]) == bits
    for x in (w, lens, offs):
        x.setflags(write=False)
    return Ref(w, bits, lens, offs)


def reference(c, second=False):
    """The oracle's flushed stream, bit count, block lengths and cumulative block offsets (nblocks + 1 entries) of a
    case's first or second input. Computed once, read-only."""
    shrink = None if not second else ("scale" if c.pset.startswith("acc") else "zero")
    return _reference(c.field, c.shape, shrink, c.dtype, c.pset)


def append_reference(ac):
    return _reference(ac.field, ac.shape, None, "f32", ac.pset)


@functools.lru_cache(maxsize=None)
def decoded(name, shape, dtype, pset):
    """oracle.decompress of the first input's oracle stream (read-only)."""
    r = _reference(name, shape, None, dtype, pset)
    d = O.decompress(r.words, shape, params(pset, len(shape)))
    d.setflags(write=False)
    return d
