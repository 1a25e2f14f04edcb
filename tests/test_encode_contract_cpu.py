"""What the inputs of the encoder contract tests (encode_contract_inputs.py, run by test_gpu_encode_contract.py) claim,
checked with the oracle and without a GPU, so that a later edit of a shape, a seed or a parameter set cannot turn a
case into one that no longer reaches its path: ranges of more than one tile with tile boundaries and range starts on
both sides of 32-bit alignment, blocks padded to minbits and clipped at maxbits, range boundaries inside 32-bit
words, streams that end on an odd 32-bit word (the encoders' flush store), an odd block count for the rate-8 fast
path, 3-D tiles on both sides of the LDS window that share words, second inputs with shorter streams, and the chunk
lists of the append cases."""
import os
import sys

import numpy as np
import pytest

TESTS = os.path.dirname(os.path.abspath(__file__))
if TESTS not in sys.path:
    sys.path.insert(0, TESTS)

import encode_contract_inputs as I  # noqa: E402


@pytest.fixture(scope="module", autouse=True)
def _oracle(orc):
    return orc


def _ids(cases):
    return [c.id for c in cases]


def _var(cases):
    return [c for c in cases if not I.is_fixed(c.pset)]


def _odd_end(bits):
    """The stream's last 32-bit word has an even index: the encoder stores a zero word after it to flush."""
    return ((bits + 31) // 32) % 2 == 1


def test_table():
    assert len(set(_ids(I.CASES))) == len(I.CASES)
    groups = {}
    for c in I.CASES:
        groups.setdefault(c.id.split("-")[0], []).append(c)
    assert {g: len(v) for g, v in groups.items()} == {"fast1d": 16, "tiles1d": 5, "var1d": 12, "gen1d": 3, "multi1d": 2,
                                                      "d2": 48, "multi2d": 2, "d3": 4, "oversized3d": 1, "d4": 6}
    for c in I.CASES:
        fixed = I.is_fixed(c.pset)
        p = I.params(c.pset, len(c.shape))
        assert (p.minbits == p.maxbits) == fixed
        assert c.strides == ((1, 2) if (not fixed or c.id.endswith("index")) else (0,))
        assert c.patterns == (("ones",) if c.field.startswith("multi2d") else ("ones", "5a"))
        assert c.multi == (I.nblocks(c.shape) > I.MULTI_BLOCKS)
    # the parameter sets' 1-D domains: lean (whole words, no index), var1d (no budget), everything else generic
    assert I.params("rate3.0625", 2).maxbits == 49 and I.params("rate2.51", 4).maxbits % 32 != 0
    for ps in ("expert20_160", "expert1_80"):
        p = I.params(ps, 1)
        assert p.minbits != p.maxbits and not (p.minbits <= 1 and p.maxbits >= 160)
    for ps in ("acc1e-3", "prec20"):
        p = I.params(ps, 1)
        assert p.minbits <= 1 and p.maxbits >= 160
    assert I.block_ids((5, 9)).tolist()[4] == [3, 3, 3, 3, 4, 4, 4, 4, 5] and I.block_ids((9,))[8] == 2


@pytest.mark.parametrize("c", I.CASES, ids=_ids(I.CASES))
def test_inputs_are_what_they_claim(c):
    a = I.field(c.field, c.shape)
    assert a.shape == c.shape and a.dtype == np.float32 and not a.flags.writeable
    x = I.case_input(c)
    assert x.dtype == (np.uint16 if c.dtype == "bf16" else np.float32)
    flat = a.reshape(-1)
    if flat.size > 96 and not c.field.startswith("oversized3d"):
        z = flat[96::97]
        assert not z[np.isfinite(z)].any()  # an Inf / NaN member may have landed on one
    if flat.size >= 9 and not c.field.startswith("oversized3d"):
        assert np.array_equal(flat[5:9], I.TINY)
    nb = I.nblocks(c.shape)
    bid = I.block_ids(c.shape)
    if nb >= 24:  # whole all-zero blocks
        absmax = np.zeros(nb)
        np.maximum.at(absmax, bid.reshape(-1), np.nan_to_num(np.abs(flat), nan=1.0, posinf=1.0))
        assert (absmax == 0).sum() >= 3
    if len(c.shape) >= 2 and not c.multi and not c.field.startswith("oversized3d"):
        for hit in (np.isposinf(a), np.isneginf(a), np.isnan(a)):  # one block each
            assert hit.sum() == 1
        assert len({int(bid[np.isposinf(a)][0]), int(bid[np.isneginf(a)][0]), int(bid[np.isnan(a)][0])}) == 3
    else:
        assert np.isfinite(a).all()


@pytest.mark.parametrize("c", I.CASES, ids=_ids(I.CASES))
def test_second_input_is_shorter(c):
    r1, r2 = I.reference(c), I.reference(c, second=True)
    assert r1.lens.size == r2.lens.size == I.nblocks(c.shape)
    assert not np.array_equal(I.case_input(c), I.case_input(c, second=True))
    if I.is_fixed(c.pset):
        assert r1.bits == r2.bits == I.nblocks(c.shape) * I.params(c.pset, len(c.shape)).maxbits
        assert r1.words.tobytes() != r2.words.tobytes()
    else:  # the first stream's tail stays in the buffer past the second stream's end
        assert r2.bits < r1.bits and r2.words.size < r1.words.size


@pytest.mark.parametrize("c", I.MULTI_CASES, ids=_ids(I.MULTI_CASES))
def test_multi_tile_ranges(c):
    nb = I.nblocks(c.shape)
    assert nb > I.MULTI_BLOCKS and int(np.prod(c.shape)) < 8.45e6
    rb = I.range_blocks(c.shape, c.pset)
    assert rb == 512  # two tiles of 256 blocks: k_encode_tiles' loop runs twice, with a carry word between
    r = I.reference(c)
    inner = r.offs[256:nb:rb] % 32   # tile boundaries strictly inside a range
    starts = r.offs[rb:nb:rb] % 32   # range starts (the scan zeroes the words they share)
    for at in (inner, starts):
        assert (at != 0).any() and (at == 0).any(), (int((at != 0).sum()), int((at == 0).sum()))
    assert r.bits % 64 != 0 and _odd_end(r.bits)  # a flush, and one the encoder has to store


@pytest.mark.parametrize("c", [c for c in I.CASES if c.pset == "expert20_160"],
                         ids=_ids([c for c in I.CASES if c.pset == "expert20_160"]))
def test_minbits_pads_some_blocks(c):
    p = I.params(c.pset, len(c.shape))
    lens = I.reference(c).lens
    assert lens.min() == p.minbits and (lens == p.minbits).sum() > 0
    assert (lens > p.minbits).sum() > lens.size // 2
    assert lens.max() <= p.maxbits


@pytest.mark.parametrize("c", [c for c in I.CASES if c.pset == "expert1_80"],
                         ids=_ids([c for c in I.CASES if c.pset == "expert1_80"]))
def test_maxbits_clips_some_blocks(c):
    p = I.params(c.pset, len(c.shape))
    lens = I.reference(c).lens
    assert lens.max() == p.maxbits
    assert (lens == p.maxbits).sum() >= 0.05 * lens.size and (lens < p.maxbits).sum() >= 0.05 * lens.size


@pytest.mark.parametrize("c", _var(I.SMALL_CASES), ids=_ids(_var(I.SMALL_CASES)))
def test_small_variable_rate_edges(c):
    nb = I.nblocks(c.shape)
    r = I.reference(c)
    rb = I.range_blocks(c.shape, c.pset)
    if nb > rb:
        assert (r.offs[rb:nb:rb] % 32 != 0).any()
    if c.field.startswith("var1d"):  # the tile form's tiles of 1024 blocks
        assert nb > 3 * 1024 and (r.offs[1024:nb:1024] % 32 != 0).any()
    assert _odd_end(r.bits), r.bits
    assert r.bits % 32 != 0  # the last word is partial as well


def test_fast1d_rate8_odd_block_count():
    cs = [c for c in I.CASES if c.field.startswith("fast1d") and c.pset == "rate8"]
    assert any(I.nblocks(c.shape) > 2048 and I.nblocks(c.shape) % 2 == 1 for c in cs)
    assert {c.shape[0] for c in cs} == {1, 5, 4 * 2048 + 3, 4 * 2049 + 3}


def _tile_kinds(offs, nb):
    """Per 64-block tile: its stream words as k_encode3d_var counts them, and whether they exceed the window."""
    t0 = offs[0:nb:64].astype(np.int64)
    t1 = np.append(t0[1:], np.int64(offs[nb]))
    words = ((t0 % 32) + (t1 - t0) + 31) // 32
    return t0, words, words + 2 > I.E3V_WIN_WORDS


def test_3d_oversized_tiles():
    (c,) = [c for c in I.CASES if c.field.startswith("oversized3d")]
    nb = I.nblocks(c.shape)
    t0, words, big = _tile_kinds(I.reference(c).offs, nb)
    assert (words > I.E3V_WIN_WORDS - 2).any() and (words < I.E3V_WIN_WORDS - 2).any()
    shared = (t0[1:] % 32 != 0) & (big[1:] != big[:-1])  # a fitting tile and an oversized one share a word
    assert shared.any()
    # the second input fits the window everywhere: the second call takes the other kernel path over the same words
    assert not _tile_kinds(I.reference(c, second=True).offs, nb)[2].any()


@pytest.mark.parametrize("ac", I.APPEND_CASES, ids=[a.id for a in I.APPEND_CASES])
def test_append_chunks(ac):
    cuts = ac.cuts
    assert cuts[0] == 0 and cuts[-1] == ac.shape[0] and list(cuts) == sorted(cuts)
    assert all(c % 4 == 0 for c in cuts[:-1])
    sizes = [b - a for a, b in zip(cuts, cuts[1:])]
    assert 0 in sizes and 4 in sizes  # an empty chunk, a chunk of one row of blocks
    p = I.params(ac.pset, len(ac.shape))
    assert p.minbits != p.maxbits
    r = I.append_reference(ac)
    per_row = I.nblocks(ac.shape) // ((ac.shape[0] + 3) // 4)
    starts = [int(r.offs[c // 4 * per_row]) for c in cuts[1:-1]]
    assert any(s % 32 for s in starts)  # a chunk ORs its first word into the bits before it
    assert _odd_end(r.bits)
    if ac.zero_start is not None:  # the chunk's second block starts in the word that holds the earlier stream's end
        b = ac.zero_start // 4 * per_row
        base = int(r.offs[b])
        assert ac.zero_start in cuts[1:-1] and 1 <= base % 32 <= 30
        assert r.lens[b] == 1 and int(r.offs[b + 1]) >> 5 == base >> 5
    if len(ac.shape) == 3:  # a chunk boundary inside a word, next to an oversized tile on either side of it
        hit = False
        for lo, mid, hi in zip(cuts, cuts[1:], cuts[2:]):
            if lo == mid or mid == hi or r.offs[mid // 4 * per_row] % 32 == 0:
                continue
            b0, b1, b2 = (x // 4 * per_row for x in (lo, mid, (hi + 3) // 4 * 4))
            before = _tile_kinds(r.offs[b0:b1 + 1], b1 - b0)[2]  # the tiles of the chunk that ends there
            after = _tile_kinds(r.offs[b1:b2 + 1], b2 - b1)[2]   # and of the one that starts there
            hit = hit or bool(before[-1]) or bool(after[0])
        assert hit


def test_decode_references():
    for c in I.SMALL_CASES:
        if c.view or c.form:
            continue
        d = I.decoded(c.field, c.shape, c.dtype, c.pset)
        assert d.shape == c.shape and d.dtype == np.float32
