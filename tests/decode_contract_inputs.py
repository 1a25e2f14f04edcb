"""TEST INFRASTRUCTURE ONLY -- the case table, the streams as the decoder receives them and the oracle's expectations
of the decoder contract tests (test_decode_contract_cpu.py checks what the inputs claim, test_gpu_decode_contract.py
runs them): gcow_decode_device, gcow_decode_device_at and gcow_decode_mean_device on streams that are followed by
anything but zeros, that start at a bit offset, that are entered in the middle, and into outputs that are neither
contiguous nor 16-byte aligned.

Cases: the small cases of the encoder contract tests (encode_contract_inputs.SMALL_CASES, one per distinct
(field, shape, dtype, parameter set)), and three 1-D cases on N_DENSE values of the oracle's gen_normal: at accuracy
1e-8 (about 90 bits per block, so that whole 128-chunk groups of the 1-D variable-rate decoder exceed the 64-bit stage
and go to its second pass), at accuracy 1e-3 (the 32-bit stage tier) and at accuracy 2.5e-4 (31.5 bits per block: the
48-bit tier, which only a buffer of the stream's own size selects).

Every expectation is oracle.decompress of the oracle's clean stream. A stream as the decoder gets it is built here as a
Python integer: (stream << k) | poison below bit k | poison from the stream's last bit on."""
from __future__ import annotations

import collections
import functools

import numpy as np

from oracle import oracle as O

import encode_contract_inputs as E
from roundtrip_inputs import bf16_rne

PATTERNS = E.PATTERNS
OFFSETS = (1, 31, 32, 33, 63, 64, 96, 148, 64 * 5 + 17)
N_DENSE = 4 * 16 * 128 * 2 + 4 * 16 * 37 + 4 * 5 + 2  # two whole groups of 128 chunks of 16 blocks, a partial one
DENSE_SEED = 0x51A6E
DENSE_PSETS = ("acc1e-8", "acc1e-3", "acc2.5e-4")
POISON_WORDS = 4  # allocated (and poisoned) past the stream's last word, whatever in_bytes says

DCase = collections.namedtuple("DCase", "id field shape pset dtype")


def _table():
    out, seen = [], set()
    for c in E.SMALL_CASES:
        key = (c.field, c.shape, c.dtype, c.pset)
        if key in seen:  # a view, an encoder form or an index of the same stream
            continue
        seen.add(key)
        out.append(DCase(c.id, c.field, c.shape, c.pset, c.dtype))
    for ps in DENSE_PSETS:
        out.append(DCase("dense1d-%d-%s-f32" % (N_DENSE, ps), "dense1d", (N_DENSE,), ps, "f32"))
    return out


CASES = _table()
BY_ID = {c.id: c for c in CASES}


def params(c):
    return O.accuracy(float(c.pset[3:])) if c.field == "dense1d" else E.params(c.pset, len(c.shape))


def is_fixed(c):
    return E.is_fixed(c.pset)


@functools.lru_cache(maxsize=None)
def reference(c):
    """The oracle's flushed stream, bit count, block lengths and cumulative block offsets (E.Ref), read-only."""
    if c.field != "dense1d":
        return E._reference(c.field, c.shape, None, c.dtype, c.pset)
    a = O.gen_normal(N_DENSE, 1e-3, DENSE_SEED, True)
    w, bits = O.compress(a, params(c))
    lens = O.block_bits(a, params(c)).astype(np.uint64)
    offs = np.concatenate([[0], np.cumsum(lens)]).astype(np.uint64)
    assert int(offs[-1]) == bits
    for x in (w, lens, offs):
        x.setflags(write=False)
    return E.Ref(w, bits, lens, offs)


@functools.lru_cache(maxsize=None)
def decoded(c):
    """oracle.decompress of the clean stream: fp32 of the case's shape, read-only."""
    d = O.decompress(reference(c).words, c.shape, params(c))
    d.setflags(write=False)
    return d


def as_bits(a, out):
    """What the decoder stores for the fp32 values a: their bits (uint32), or (out "bf16") the bf16 bits of each value
    rounded to nearest even (uint16)."""
    a = np.ascontiguousarray(a, np.float32)
    return a.view(np.uint32) if out == "f32" else bf16_rne(a.reshape(-1)).reshape(a.shape)


# ------------------------------------------------------------------------------------------------ streams
def to_int(words):
    return int.from_bytes(np.ascontiguousarray(words, "<u8").tobytes(), "little")


def to_words(v, nwords):
    return np.frombuffer(v.to_bytes(8 * nwords, "little"), "<u8").copy()


def stream_words(bits, k=0):
    """64-bit words a stream of `bits` bits that starts at bit k reaches into."""
    return (k + bits + 63) // 64


def dirty_stream(ref, pattern, nwords, k=0):
    """nwords 64-bit words: poison below bit k, the stream's ref.bits bits from bit k on, poison from the stream's last
    bit to the end (the rest of its last word included). The flush zeros of the oracle's stream are not part of it.
    Where the pattern has no one-bit among the bits of the last word above the stream's end (0x5A...: bit 63 alone),
    those bits take the pattern's complement, so that they never equal the flush."""
    word = int(np.array([PATTERNS[pattern]], np.int64).view(np.uint64)[0])
    fill = to_int(np.full(nwords, word, np.uint64))
    mask = ((1 << ref.bits) - 1) << k
    assert stream_words(ref.bits, k) <= nwords
    v = (fill & ~mask) | ((to_int(ref.words) << k) & mask)
    end = k + ref.bits
    rest = ((1 << (-end % 64)) - 1) << end  # the bits of the stream's last word above its end
    if rest and not v & rest:
        v |= ~fill & rest
    return to_words(v, nwords)


def oracle_decode_at(words, k, c, shape=None):
    """oracle.decompress of the bits of `words` from bit k on, padded with zeros to the capacity of the shape."""
    shape = c.shape if shape is None else shape
    w = to_words(to_int(words) >> k, max(len(words), cap_words(shape, params(c))) + 4)
    return O.decompress(w, shape, params(c))


# ------------------------------------------------------------------------------------------------ decode_impl's rules
# Restated once, from gcow_amd/csrc: gcow_api.cpp decode_impl (the order of the tests below is its order),
# block_bits_bound and gcow_max_output_bytes; dec1d.hip launch_decode1d_var (the stage tier from `avail`), vdec_tier,
# vdec_left_to_big_w and vdec_group (a group is 128 index chunks of 16 blocks); gcow_blocks.hip launch_decode,
# k_decode_staged (a workgroup is 64 blocks, CAPW = 2048 32-bit words) and fixed3d_ok.
LEAN_GROUP = 128
STAGED_CAPW32 = 64 * 1024 // 32


def block_bound(p, dims):
    B = 1 << (2 * dims)
    mb = min(9 + (B - 1) + B * min(p.maxprec, 32), p.maxbits)
    return max(mb, p.minbits, 1)


def cap_words(shape, p):
    """gcow_max_output_bytes / 8."""
    return (E.nblocks(shape) * block_bound(p, len(shape)) + 63) // 64 + 1


def vdec_cap(capb):
    return LEAN_GROUP * 16 * capb // 64


def _lean_routes(n, idx, k, in_words):
    nb = (n + 3) // 4
    nchunks = (nb + 15) // 16
    avail = in_words * 64 - min(k, in_words * 64)
    gated = avail >= nb * 128
    if gated:  # a capacity-sized buffer: the 32- and 64-bit tiers launched, gated on the index (vdec_tier)
        capb = 32
        if nchunks >= 2 and int(idx[nchunks - 1] - idx[0]) * 5 > (nchunks - 1) * 16 * 32 * 4:
            capb = 64
    elif avail * 5 <= nb * 32 * 4:
        capb = 32
    elif avail * 5 <= nb * 48 * 4:
        capb = 48
    else:
        capb = 64
    cap, out = vdec_cap(capb), {"lean:%s%d" % ("gated" if gated else "stage", capb)}
    for c0 in range(0, nchunks, LEAN_GROUP):
        w0 = ((k + int(idx[c0])) >> 6) & ~1
        inner = c0 + LEAN_GROUP < nchunks
        wend = ((k + int(idx[c0 + LEAN_GROUP]) + 63) >> 6) if inner else in_words
        span = min(wend, in_words) - w0
        if inner and 16 * (c0 + LEAN_GROUP) <= n // 4 and span > cap:
            out.add("lean_second_pass")
            continue
        whole = c0 + LEAN_GROUP <= nchunks and 16 * (c0 + LEAN_GROUP) <= n // 4
        out.add("lean_main_staged" if span <= cap and whole else "lean_general")
    return out


def _staged_routes(dims, nb, start_of, in_words):
    out = {"k_decode_staged<%d>" % dims}
    b0 = (nb - 1) // 64 * 64  # the last workgroup: its span runs to in_words
    w0 = (start_of(b0) >> 5) & ~3
    out.add("k_decode_staged<%d>:last_%s" % (dims, "staged" if 2 * in_words - w0 <= STAGED_CAPW32 else "unstaged"))
    return out


def routes(c, stride, k, in_words, vec=True):
    """The decoder kernels (and, for the staged ones, the paths inside them) that gcow_decode_device_at takes for the
    whole field of case c, a contiguous aligned fp32 output (vec), the oracle's index at `stride` (0: none)."""
    p, dims, nb = params(c), len(c.shape), E.nblocks(c.shape)
    fixed = p.minbits == p.maxbits
    offs = reference(c).offs
    if fixed and dims == 1 and vec and p.maxbits in (32, 64) and p.maxprec >= 32 and p.minexp <= -154 and k % 32 == 0:
        out = {"lean_fixed%d" % p.maxbits} if c.shape[0] >= 4 else set()
        return out | ({"tail_block"} if c.shape[0] % 4 else set())
    if dims == 4:
        return {"k_decode4d_seq" if not fixed and stride != 1 else "k_decode4d"}
    if fixed and dims == 3 and k % 32 == 0 and p.maxbits % 32 == 0 and p.maxbits // 32 in (2, 4, 8, 16, 32, 64):
        return {"k_decode3d_fixed"}
    chunk = 1 if fixed else (stride if stride else nb)
    if not fixed and dims == 1 and vec and p.minbits <= 1 and p.maxbits >= 160:
        if stride == 16 and in_words:
            return _lean_routes(c.shape[0], offs[:-1][::16], k, in_words)
        return {"k_decode1d_var"}
    if chunk == 1 and in_words and (fixed or stride) and dims >= 2:
        start = (lambda b: k + b * p.maxbits) if fixed else (lambda b: k + int(offs[b]))
        return _staged_routes(dims, nb, start, in_words)
    return {"k_decode<%d>" % dims}


ROUTES = ("lean_fixed64", "lean_fixed32", "tail_block", "k_decode<1>", "k_decode1d_var", "lean_main_staged",
          "lean_general", "lean_second_pass", "k_decode_staged<2>:last_staged", "k_decode_staged<2>:last_unstaged",
          "k_decode_staged<3>:last_staged", "k_decode_staged<3>:last_unstaged", "k_decode<2>", "k_decode<3>",
          "k_decode3d_fixed", "k_decode4d", "k_decode4d_seq")


def buffer_words(c, size, k=0):
    """(in_words, allocated words) of a run: "exact" says the stream's words plus 2, "cap" the encoder's capacity
    (gcow_max_output_bytes, after the words the offset takes), "own" the stream's words and no more (the header allows
    in_bytes to be the stream's own length). POISON_WORDS more are allocated past the stream."""
    nw = stream_words(reference(c).bits, k)
    in_words = {"own": nw, "exact": nw + 2}.get(size, (k + 63) // 64 + cap_words(c.shape, params(c)))
    assert in_words >= nw
    return in_words, max(in_words, nw + POISON_WORDS)


def var_strides(c):
    """Index strides of a variable-rate case in the dirty-tail and offset runs (a 4-D index at a stride other than 1
    is ignored: the stream is walked in order, as without one)."""
    return (0, 1) if len(c.shape) == 4 else (0, 1, 16)


# ------------------------------------------------------------------------------------------------ the runs
# item 1: every case
DIRTY_RUNS = [(c, s) for c in CASES for s in ((0,) if is_fixed(c) else var_strides(c))]

# item 2: (case id, strides, offsets, buffer sizes)
_ALL = OFFSETS
OFFSET_TABLE = [
    ("fast1d-8199-rate16-f32", (0,), _ALL, ("exact",)),   # lean 64 at k % 32 == 0, else k_decode<1>; a tail block
    ("fast1d-8199-rate8-f32", (0,), _ALL, ("exact",)),    # lean 32
    ("fast1d-8195-rate16-bf16", (0,), _ALL, ("exact",)),
    ("fast1d-5-rate8-f32", (0,), _ALL, ("exact",)),
    ("tiles1d-1029-rate12-f32", (0,), _ALL, ("exact",)),
    ("tiles1d-1029-rate2.5-f32", (0,), _ALL, ("exact",)),
    ("d2-37x53-rate8-f32", (0,), _ALL, ("exact", "cap")),
    ("d2-66x70-rate3.0625-f32", (0,), _ALL, ("exact",)),
    ("d3-13x17x21-rate8-f32", (0,), _ALL, ("exact", "cap")),  # the word path at k % 32 == 0, else k_decode_staged<3>
    ("d3-13x17x21-rate2.5-f32", (0,), _ALL, ("exact",)),
    ("d4-6x5x7x10-rate8-f32", (0,), _ALL, ("exact",)),
    ("d4-6x5x7x10-rate2.51-f32", (0,), _ALL, ("exact",)),
    ("var1d-12309-acc1e-3-f32", (0, 1, 16), _ALL, ("exact", "cap")),
    ("var1d-12309-prec20-bf16", (16,), _ALL, ("exact",)),
    ("gen1d-1029-expert20_160-f32", (0, 1, 16), _ALL, ("exact",)),
    ("gen1d-1029-expert1_80-f32", (1,), _ALL, ("exact",)),
    ("d2-37x53-acc1e-3-f32", (0, 1, 16), _ALL, ("exact", "cap")),
    ("d2-66x70-acc1e-3-f32", (1,), _ALL, ("exact", "cap")),
    ("d2-66x70-expert20_160-f32", (1, 16), _ALL, ("exact",)),
    ("d3-13x17x21-acc1e-3-f32", (0, 1, 16), _ALL, ("exact", "cap")),
    ("oversized3d-24x40x64-prec32-f32", (1,), (33, 64, 64 * 5 + 17), ("exact",)),
    ("d4-6x5x7x10-acc1e-4-f32", (0, 1), _ALL, ("exact",)),
    ("d4-6x5x7x10-prec20-f32", (1,), _ALL, ("exact",)),
    ("dense1d-%d-acc1e-8-f32" % N_DENSE, (16,), (33, 64 * 5 + 17), ("exact", "cap")),
    ("dense1d-%d-acc1e-3-f32" % N_DENSE, (16,), (33, 64 * 5 + 17), ("exact", "cap")),
    ("dense1d-%d-acc2.5e-4-f32" % N_DENSE, (16,), (33, 64 * 5 + 17), ("exact", "cap")),
]
OFFSET_RUNS = [(BY_ID[i], s, ks, sizes) for i, strides, ks, sizes in OFFSET_TABLE for s in strides]

# item 3: (case id, index stride, cuts along the slowest axis). Every list has a part of one row of blocks (1-D at
# stride 16: one index chunk, 64 values) and the ragged last rows.
SUBFIELD_TABLE = [
    ("fast1d-8199-rate16-f32", 0, (0, 4, 4 * 700, 4 * 2048, 8199)),
    ("fast1d-8199-rate8-f32", 0, (0, 4, 4 * 701, 4 * 2049, 8199)),  # parts that start on an odd 32-bit word
    ("tiles1d-1029-rate12-f32", 0, (0, 4, 4 * 100, 1028, 1029)),
    ("var1d-12309-acc1e-3-f32", 16, (0, 64, 64 * 33, 64 * 150, 64 * 192, 12309)),
    ("gen1d-1029-expert20_160-f32", 16, (0, 64, 64 * 7, 64 * 16, 1029)),
    ("dense1d-%d-acc1e-8-f32" % N_DENSE, 16, (0, 64 * 5, 64 * 140, 64 * 141, N_DENSE)),
    ("d2-66x70-rate8-f32", 0, (0, 4, 36, 64, 66)),
    ("d2-66x70-acc1e-3-f32", 1, (0, 4, 36, 64, 66)),
    ("d3-13x17x21-rate8-f32", 0, (0, 4, 8, 13)),
    ("d3-13x17x21-rate2.5-f32", 0, (0, 4, 12, 13)),
    ("d3-13x17x21-acc1e-3-f32", 1, (0, 4, 8, 13)),
    ("d4-6x5x7x10-rate2.51-f32", 0, (0, 4, 6)),
    ("d4-6x5x7x10-acc1e-4-f32", 1, (0, 4, 6)),
]
SUBFIELD_RUNS = [(BY_ID[i], s, cuts) for i, s, cuts in SUBFIELD_TABLE]


def subfield_parts(c, stride, cuts):
    """Per part: (lo, hi, first block, bit_offset, first index entry). Fixed rate enters at first_block * maxbits;
    variable rate at bit 0 with the index pointer advanced (absolute entries)."""
    per_row = E.nblocks(c.shape) // ((c.shape[0] + 3) // 4)
    p, parts = params(c), []
    for lo, hi in zip(cuts, cuts[1:]):
        first = lo // 4 * per_row
        if is_fixed(c):
            parts.append((lo, hi, first, first * p.maxbits, 0))
        else:
            assert first % stride == 0
            parts.append((lo, hi, first, 0, first // stride))
    return parts


# item 4: (case id, index stride) per dimension, one fixed-rate and one variable-rate set
LAYOUT_CASES = {
    1: [("fast1d-8199-rate16-f32", 0), ("var1d-12309-acc1e-3-f32", 16)],
    2: [("d2-37x53-rate8-f32", 0), ("d2-37x53-acc1e-3-f32", 1)],
    3: [("d3-13x17x21-rate8-f32", 0), ("d3-13x17x21-acc1e-3-f32", 1)],
    4: [("d4-6x5x7x10-rate2.51-f32", 0), ("d4-6x5x7x10-acc1e-4-f32", 1)],
}

# An output view inside one allocation: `alloc` elements, element (i0, i1, ...) of the field (numpy order, the slowest
# axis first) at offset + sum(i * stride).
Layout = collections.namedtuple("Layout", "name out alloc offset strides")


def _dense(shape):
    st, m = [], 1
    for s in reversed(shape):
        st.append(m)
        m *= s
    return tuple(reversed(st))


def _window(name, shape, before, after):
    parent = tuple(s + b + a for s, b, a in zip(shape, before, after))
    st = _dense(parent)
    return Layout(name, "f32", int(np.prod(parent)), sum(b * s for b, s in zip(before, st)), st)


def _permuted(name, shape, order):
    """The field stored densely with its axes in `order` (slowest first), viewed in the field's own order."""
    st, m = [0] * len(shape), 1
    for ax in reversed(order):
        st[ax] = m
        m *= shape[ax]
    return Layout(name, "f32", m + 8, 4, tuple(st))  # four guard elements on either side


def layouts(shape):
    n = int(np.prod(shape))
    if len(shape) == 1:
        return ([Layout("f32-off%d" % o, "f32", n + 8, o, (1,)) for o in (1, 2, 3)] +
                [Layout("f32-stride%d" % s, "f32", s * n + 5, 2, (s,)) for s in (2, 3)] +
                [Layout("bf16-off%d" % o, "bf16", n + 8, o, (1,)) for o in (1, 3)])
    if len(shape) == 2:
        ny, nx = shape
        return [_permuted("transposed", shape, (1, 0)),
                Layout("rows+4", "f32", ny * (nx + 4) + 8, 4, (nx + 4, 1)),   # 16-byte aligned rows with gaps
                Layout("rows+3", "f32", ny * (nx + 3) + 8, 4, (nx + 3, 1)),   # rows off 16 bytes: value stores
                _window("window", shape, (3, 5), (2, 1)),
                Layout("negative-sy", "f32", ny * nx + 8, 4 + (ny - 1) * nx, (-nx, 1))]
    if len(shape) == 3:
        return [_permuted("permuted", shape, (2, 0, 1)), _window("window", shape, (1, 2, 4), (1, 1, 1))]
    return [_permuted("permuted", shape, (1, 3, 0, 2))]


def image(layout, want_bits, fill):
    """The whole allocation after the decode: `fill` everywhere but in the view, which holds want_bits."""
    img = np.full(layout.alloc, fill, want_bits.dtype)
    isz = img.itemsize
    view = np.lib.stride_tricks.as_strided(img[layout.offset:], want_bits.shape, tuple(s * isz for s in layout.strides))
    view[...] = want_bits
    return img


def layout_is_vec(layout, shape):
    """make_field's F.vec for the view in an allocation whose base is 16-byte aligned."""
    esz = 2 if layout.out == "bf16" else 4
    st = layout.strides
    return st[-1] == 1 and (layout.offset * esz) % (4 * esz) == 0 and all(s % 4 == 0 for s in st[:-1])


# item 5
INDEX_STRIDES = (1, 2, 4, 8, 16, 32, 64, 128, 256)
STRIDE_CASES = ["var1d-12309-acc1e-3-f32", "gen1d-1029-expert20_160-f32", "d2-37x53-acc1e-3-f32",
                "d3-13x17x21-acc1e-3-f32"]
PREFIX_1D = 4 * 100  # the first 100 blocks of the 1-D streams decoded alone: strides 128 and 256 exceed the block count

# item 6
ODD_WORD_RUNS = [("var1d-12309-acc1e-3-f32", 16), ("dense1d-%d-acc1e-8-f32" % N_DENSE, 16),
                 ("fast1d-8199-rate16-f32", 0), ("d3-13x17x21-acc1e-3-f32", 1), ("d3-13x17x21-rate8-f32", 0)]

# decode_mean: W streams of n values, of different lengths at variable rate
MEAN_N = 4 * (16 * 128 + 16 * 37 + 5) + 2
MEAN_W = 3
MEAN_PSETS = ("rate16", "rate2.5", "acc1e-3")
MEAN_INDEXES = (8, 16, "packed16")


@functools.lru_cache(maxsize=None)
def mean_reference(pset):
    """Per stream the oracle's E.Ref, and the fp32 mean of the oracle's decodes in rank order:
    ((0 + x_0) + x_1 + x_2) / 3, as gcow_decode_mean_device defines it."""
    p = E.params(pset, 1)
    refs, acc = [], np.zeros(MEAN_N, np.float32)
    for r in range(MEAN_W):
        a = np.array(E.field("mean1d-%d" % r, (MEAN_N,))) * np.float32(2.0 ** (-3 * r))
        w, bits = O.compress(a, p)
        offs = np.concatenate([[0], np.cumsum(O.block_bits(a, p).astype(np.uint64))]).astype(np.uint64)
        refs.append(E.Ref(w, bits, None, offs))
        acc = acc + O.decompress(w, (MEAN_N,), p)
    mean = acc / np.float32(MEAN_W)
    mean.setflags(write=False)
    return tuple(refs), mean


def mean_streams(pset, pattern):
    """(words, stream_words): the W streams stream_words apart (an odd spacing, one word more than the longest stream
    at least), every slot poisoned from its own stream's last bit on, and the 2 words after the last slot."""
    refs, _ = mean_reference(pset)
    sw = max(stream_words(r.bits) for r in refs) + 1
    sw += 1 - sw % 2
    out = np.concatenate([dirty_stream(r, pattern, sw) for r in refs] +
                         [np.full(2, PATTERNS[pattern], np.int64).view(np.uint64)])
    return out, sw
