"""What the inputs of the decoder contract tests (decode_contract_inputs.py, run by test_gpu_decode_contract.py) claim,
checked with the oracle and without a GPU, so that a later edit of a shape, a seed, an offset or a cut cannot turn a
case into one that no longer reaches its decoder: every route of decode_impl has a dirty-tail case and an offset case
(decided by decode_impl's rules as the inputs module restates them, from the oracle's block offsets), the poison sets
bits above the stream's end, a decoder that drops or misplaces a bit offset or enters a sub-field at the wrong block
cannot produce the expectation, the shifted-stream builder round-trips, the output views are what they are named
for, and no expectation holds a NaN (the GPU test compares every element bit for bit)."""
import os
import sys

import numpy as np
import pytest

TESTS = os.path.dirname(os.path.abspath(__file__))
if TESTS not in sys.path:
    sys.path.insert(0, TESTS)

import decode_contract_inputs as D  # noqa: E402
import encode_contract_inputs as E  # noqa: E402


@pytest.fixture(scope="module", autouse=True)
def _oracle(orc):
    return orc


def _same(a, b):
    return np.array_equal(np.ascontiguousarray(a).view(np.uint32), np.ascontiguousarray(b).view(np.uint32))


def test_table():
    assert len(D.CASES) == 72 and len(D.BY_ID) == 72  # 69 distinct small cases of the encoder contract, 3 dense 1-D
    assert len({(c.field, c.shape, c.dtype, c.pset) for c in D.CASES}) == 72
    assert [c.pset for c in D.CASES if c.field == "dense1d"] == ["acc1e-8", "acc1e-3", "acc2.5e-4"]
    assert D.N_DENSE == 18774 == max(c.shape[0] for c in D.CASES if len(c.shape) == 1)
    assert max(int(np.prod(c.shape)) for c in D.CASES) == 24 * 40 * 64  # every field is small
    for c in D.CASES:
        p = D.params(c)
        assert (p.minbits == p.maxbits) == D.is_fixed(c)
        assert D.cap_words(c.shape, p) >= D.stream_words(D.reference(c).bits) + (0 if D.is_fixed(c) else 1)
    for table in (D.OFFSET_TABLE, D.SUBFIELD_TABLE):
        assert len({(row[0], row[1]) for row in table}) == len(table)
    for k in D.OFFSETS:  # both sides of 32- and 64-bit alignment, the zfp header lengths, and past several words
        assert k > 0
    assert {k % 32 == 0 for k in D.OFFSETS} == {True, False} and {k % 64 == 0 for k in D.OFFSETS} == {True, False}
    assert max(D.OFFSETS) > 64 * 5 and {96, 148} <= set(D.OFFSETS)


def test_dense_cases_reach_the_second_pass_and_the_32_bit_tier():
    c8, c3 = (D.BY_ID["dense1d-%d-%s-f32" % (D.N_DENSE, ps)] for ps in ("acc1e-8", "acc1e-3"))
    r = D.reference(c8)
    nb = r.lens.size
    assert nb == (D.N_DENSE + 3) // 4 and D.N_DENSE % 4 == 2
    nchunks = (nb + 15) // 16
    assert nchunks // D.LEAN_GROUP == 2 and nchunks % D.LEAN_GROUP and nb % 16  # two whole groups, a partial one
    assert 90 < r.bits / nb < 91
    group0 = (int(r.offs[16 * D.LEAN_GROUP]) + 63) // 64
    assert group0 == 2888 > D.vdec_cap(64) == 2048
    for size in ("exact", "cap"):
        assert "lean_second_pass" in D.routes(c8, 16, 0, D.buffer_words(c8, size)[0])
    r3 = D.reference(c3)
    assert r3.bits * 5 <= nb * 32 * 4  # the 32-bit tier holds 1.25 x the average
    for size, tier in (("exact", "lean:stage32"), ("cap", "lean:gated32")):
        assert D.routes(c3, 16, 0, D.buffer_words(c3, size)[0]) == {tier, "lean_main_staged", "lean_general"}
    # every stage tier of launch_decode1d_var: 32 / 48 / 64 bits per block from the size of a buffer that is the
    # stream's own, and the 32- and 64-bit tiers gated on the device for a buffer of the encoder's capacity
    tiers = set()
    for c, s in D.DIRTY_RUNS:
        if s == 16 and len(c.shape) == 1:
            for size in ("own", "exact", "cap"):
                tiers |= {r for r in D.routes(c, s, 0, D.buffer_words(c, size)[0]) if r.startswith("lean:")}
    assert tiers == {"lean:stage32", "lean:stage48", "lean:stage64", "lean:gated32", "lean:gated64"}
    c4 = D.BY_ID["dense1d-%d-acc2.5e-4-f32" % D.N_DENSE]
    assert all("lean:stage48" in D.routes(c4, 16, k, D.buffer_words(c4, "exact", k)[0]) for k in (0, 33, 64 * 5 + 17))
    # the small 1-D variable-rate case has one whole group only
    small = D.BY_ID["var1d-12309-acc1e-3-f32"]
    assert (E.nblocks(small.shape) + 15) // 16 // D.LEAN_GROUP == 1


def test_no_expectation_holds_a_nan():
    for c in D.CASES:
        d = D.decoded(c)
        assert d.shape == c.shape and d.dtype == np.float32
        assert not np.isnan(d).any(), c.id
    for ps in D.MEAN_PSETS:
        assert not np.isnan(D.mean_reference(ps)[1]).any()


@pytest.mark.parametrize("c", D.CASES, ids=[c.id for c in D.CASES])
def test_poison_sets_bits_above_the_end(c):
    r = D.reference(c)
    nw = D.stream_words(r.bits)
    assert nw == r.words.size
    if not D.is_fixed(c):
        assert r.bits % 64  # a variable-rate stream ends inside a word
    for pat, fill in D.PATTERNS.items():
        word = np.array([fill], np.int64).view(np.uint64)[0]
        w = D.dirty_stream(r, pat, nw + D.POISON_WORDS)
        assert np.array_equal(w[:nw - 1], r.words[:nw - 1])
        assert (w[nw:] == word).all() and w.size - nw >= 4
        if r.bits % 64:  # fixed-rate streams of whole 64-bit words have no such bits: the poison starts a word later
            low = np.uint64((1 << (r.bits % 64)) - 1)
            assert w[nw - 1] & low == r.words[nw - 1] & low
            assert w[nw - 1] & ~low != 0 and r.words[nw - 1] & ~low == 0
        else:
            assert w[nw - 1] == r.words[nw - 1]
        # and the prefix below an offset
        w = D.dirty_stream(r, pat, nw + 2 + D.POISON_WORDS, k=64 + 17)
        assert w[0] == word and (w[1] ^ word) & np.uint64((1 << 17) - 1) == 0


@pytest.mark.parametrize("item", ["dirty-tail", "offsets"])
def test_every_route_has_a_case(item):
    seen = {}
    if item == "dirty-tail":
        for c, s in D.DIRTY_RUNS:
            for size in ("exact", "cap"):
                for r in D.routes(c, s, 0, D.buffer_words(c, size)[0]):
                    seen.setdefault(r, []).append((c.id, s, size))
    else:
        for c, s, ks, sizes in D.OFFSET_RUNS:
            for k in ks:
                for size in sizes:
                    for r in D.routes(c, s, k, D.buffer_words(c, size, k)[0]):
                        seen.setdefault(r, []).append((c.id, s, k, size))
    missing = [r for r in D.ROUTES if r not in seen]
    assert not missing, missing
    extra = {r for r in set(seen) - set(D.ROUTES) if not r.startswith("lean:")}  # lean:*: the stage tier, see above
    assert extra == {"k_decode_staged<2>", "k_decode_staged<3>"}


def test_routing_rules_on_known_cases():
    """The restated rules against cases whose kernel the sources name outright."""
    f16 = D.BY_ID["fast1d-8199-rate16-f32"]
    assert D.routes(f16, 0, 0, 100) == {"lean_fixed64", "tail_block"} == D.routes(f16, 0, 96, 100)
    assert D.routes(f16, 0, 33, 100) == {"k_decode<1>"} == D.routes(f16, 0, 0, 100, vec=False)
    assert D.routes(D.BY_ID["fast1d-1-rate8-f32"], 0, 0, 3) == {"tail_block"}
    d3 = D.BY_ID["d3-13x17x21-rate8-f32"]
    assert D.routes(d3, 0, 64, 4000) == {"k_decode3d_fixed"}
    assert "k_decode_staged<3>" in D.routes(d3, 0, 63, 4000)
    d4 = D.BY_ID["d4-6x5x7x10-acc1e-4-f32"]
    assert [D.routes(d4, s, 0, 9000) for s in (0, 1, 4)] == [{"k_decode4d_seq"}, {"k_decode4d"}, {"k_decode4d_seq"}]
    v = D.BY_ID["var1d-12309-acc1e-3-f32"]
    assert D.routes(v, 1, 0, 9000) == {"k_decode1d_var"} == D.routes(v, 16, 0, 0)
    assert D.routes(v, 16, 0, 9000, vec=False) == {"k_decode<1>"}
    assert D.routes(D.BY_ID["gen1d-1029-expert20_160-f32"], 16, 0, 9000) == {"k_decode<1>"}
    assert D.routes(D.BY_ID["d2-37x53-acc1e-3-f32"], 16, 0, 9000) == {"k_decode<2>"}


_OFFSET_CASES = sorted({(c.id, ks) for c, _, ks, _ in D.OFFSET_RUNS})


@pytest.mark.parametrize("cid,ks", _OFFSET_CASES, ids=[i for i, _ in _OFFSET_CASES])
def test_offsets_round_trip_and_matter(cid, ks):
    c = D.BY_ID[cid]
    r, want = D.reference(c), D.decoded(c)
    for k in ks:
        nw = D.stream_words(r.bits, k) + D.POISON_WORDS
        for pat in D.PATTERNS:
            w = D.dirty_stream(r, pat, nw, k)
            mask = (1 << r.bits) - 1
            assert (D.to_int(w) >> k) & mask == D.to_int(r.words) & mask
            clean = D.to_words((D.to_int(w) >> k) & mask, nw)
            assert _same(D.oracle_decode_at(clean, 0, c), want)
            # the neighbours of k decode to something else, whatever lies below bit k and after the stream
            for other in (k - 1, k + 1):
                assert not _same(D.oracle_decode_at(w, other, c), want), (k, other, pat)


@pytest.mark.parametrize("c,stride,cuts", D.SUBFIELD_RUNS, ids=[c.id for c, _, _ in D.SUBFIELD_RUNS])
def test_subfields(c, stride, cuts):
    assert cuts[0] == 0 and cuts[-1] == c.shape[0] and list(cuts) == sorted(set(cuts))
    assert all(x % 4 == 0 for x in cuts[:-1]) and c.shape[0] % 4  # the last rows are ragged
    per_row = E.nblocks(c.shape) // ((c.shape[0] + 3) // 4)
    parts = D.subfield_parts(c, stride, cuts)
    row = 4 if not (len(c.shape) == 1 and stride) else 4 * stride  # 1-D with an index: one index chunk
    assert any(hi - lo == row for lo, hi, *_ in parts)
    r, want = D.reference(c), D.decoded(c)
    p = D.params(c)
    starts = []
    for lo, hi, first, bit_offset, entry in parts:
        assert first == lo // 4 * per_row
        start = int(r.offs[first])
        if D.is_fixed(c):
            assert start == bit_offset == first * p.maxbits and entry == 0
        else:
            assert bit_offset == 0 and int(r.offs[:-1][::stride][entry]) == start
        shape = (hi - lo,) + c.shape[1:]
        assert _same(D.oracle_decode_at(r.words, start, c, shape), want[lo:hi])
        if starts:  # entered at the part before it, the decoder gives something else
            assert not _same(D.oracle_decode_at(r.words, starts[-1], c, shape), want[lo:hi])
        starts.append(start)
    assert len(set(starts)) == len(starts)


def _offsets_of(layout, shape):
    off = np.full(shape, layout.offset, np.int64)
    for ax, st in enumerate(layout.strides):
        off += (np.arange(shape[ax]) * st).reshape([-1 if a == ax else 1 for a in range(len(shape))])
    return off


@pytest.mark.parametrize("dims", [1, 2, 3, 4])
def test_layouts(dims):
    fixed, var = (D.BY_ID[i] for i, _ in D.LAYOUT_CASES[dims])
    assert D.is_fixed(fixed) and not D.is_fixed(var) and fixed.shape == var.shape or dims == 1
    for cid, stride in D.LAYOUT_CASES[dims]:
        c = D.BY_ID[cid]
        assert len(c.shape) == dims and (stride == 0) == D.is_fixed(c)
        ls = D.layouts(c.shape)
        for lay in ls:
            off = _offsets_of(lay, c.shape)
            assert off.min() >= 0 and off.max() < lay.alloc and np.unique(off).size == off.size
            assert off.size < lay.alloc  # elements outside the view: the fill must survive there
            want = D.as_bits(D.decoded(c), lay.out)
            img = D.image(lay, want, want.dtype.type(0x5A5A5A5A & (0xFFFF if lay.out == "bf16" else 0xFFFFFFFF)))
            assert np.array_equal(img[off.reshape(-1)], want.reshape(-1))
        vec = {lay.name: D.layout_is_vec(lay, c.shape) for lay in ls}
        if dims == 1:
            assert not any(vec.values())  # value stores: store_block1d / scatter_block<1> off the vector path
            assert {lay.offset % 4 for lay in ls if lay.name.startswith("f32-off")} == {1, 2, 3}
        elif dims == 2:
            # one padded pitch keeps 16-byte rows (vector stores with gaps), the other does not
            assert {vec["rows+4"], vec["rows+3"]} == {True, False}
            assert not vec["transposed"] and not vec["window"] and not vec["negative-sy"]
            assert [lay for lay in ls if lay.name == "negative-sy"][0].strides[0] < 0
        else:
            assert not any(vec.values())


def test_index_strides():
    assert D.INDEX_STRIDES == tuple(1 << i for i in range(9))  # every stride decode_impl accepts
    for cid in D.STRIDE_CASES:
        c = D.BY_ID[cid]
        assert not D.is_fixed(c)
        nb = E.nblocks(c.shape) if len(c.shape) > 1 else D.PREFIX_1D // 4
        assert max(D.INDEX_STRIDES) > nb  # one index entry: the whole field in one lane
    assert {len(D.BY_ID[cid].shape) for cid in D.STRIDE_CASES} == {1, 2, 3}


def test_mean_inputs():
    for ps in D.MEAN_PSETS:
        refs, mean = D.mean_reference(ps)
        assert len(refs) == D.MEAN_W == 3 and mean.shape == (D.MEAN_N,)
        fixed = E.is_fixed(ps)
        assert (len({r.bits for r in refs}) == 1) == fixed  # variable rate: three lengths
        w, sw = D.mean_streams(ps, "5a")
        assert sw % 2 == 1 and w.size == 3 * sw + 2  # streams 1 and 2 start on either side of 16 bytes
        for i, r in enumerate(refs):
            nw = D.stream_words(r.bits)
            assert nw < sw and np.array_equal(w[i * sw:i * sw + nw - 1], r.words[:nw - 1])
            assert (w[i * sw + nw:(i + 1) * sw] == np.uint64(0x5A5A5A5A5A5A5A5A)).all()
    nb = (D.MEAN_N + 3) // 4
    assert nb // 16 > 128 and nb % 16 and D.MEAN_N % 4  # a whole lean workgroup, partial chunks, a partial block


def test_odd_word_runs():
    for cid, stride in D.ODD_WORD_RUNS:
        assert (stride == 0) == D.is_fixed(D.BY_ID[cid])
    kinds = {(len(D.BY_ID[cid].shape), D.is_fixed(D.BY_ID[cid])) for cid, _ in D.ODD_WORD_RUNS}
    assert {(1, False), (1, True), (3, False)} <= kinds
