"""The contract of gcow_decode_device, gcow_decode_device_at and gcow_decode_mean_device (include/gcow.h) under the
conditions the parity suite never sets up, bit for bit against oracle.decompress of the clean stream, through the C
ABI:

  1. the stream is followed by poison, not zeros: the bits of its last word above its end and every word after it,
     in a buffer whose in_bytes is the stream's own size (its words; its words plus 2) and in one of the encoder's
     capacity; the same for every slot of decode_mean's W streams;
  2. the stream starts at a bit offset (gcow_decode_device_at), below which lies poison, with no index and with the
     oracle's index, whose entries are relative to the offset;
  3. a part of a field cut along its slowest axis is decoded alone from the whole stream: fixed rate at the bit
     offset of its first block, variable rate through the index pointer advanced to its first entry;
  4. the output is a view inside a poison-filled allocation -- off 16 bytes, strided, transposed, padded, a window,
     rows stored backwards, permuted -- and nothing outside the view is written;
  5. every index stride decode_impl accepts, and one that exceeds the block count;
  6. the stream pointer is 8 bytes off a 16-byte boundary.

Cases, streams and expectations: decode_contract_inputs.py (test_decode_contract_cpu.py proves on the CPU which decoder
kernels and paths they reach). Every comparison is bit equality of the whole output allocation; no element is left
out."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

torch = pytest.importorskip("torch")

pytestmark = pytest.mark.gpu

TESTS = os.path.dirname(os.path.abspath(__file__))
if TESTS not in sys.path:
    sys.path.insert(0, TESTS)

import decode_contract_inputs as D  # noqa: E402
import encode_contract_inputs as E  # noqa: E402

GUARD_ELEMS = 16
INDEX_PACKED16 = 0x1010


@pytest.fixture(scope="module")
def gc(orc):
    if not torch.cuda.is_available():
        pytest.fail("GPU tests need a device")
    from gcow_amd import codec
    return codec


def _lib():
    from gcow_amd._ffi import load
    return load()


def _stream():
    return torch.cuda.current_stream().cuda_stream


def _sync(L, st, what):
    """Wait for the call's kernels. A device fault ends the session: nothing more is started on a faulted device."""
    try:
        torch.cuda.synchronize()
    except RuntimeError as e:
        pytest.exit("the device faulted (%s): %s" % (what, e), returncode=3)
    if st == 3:  # GCOW_ERR_HIP
        pytest.exit("HIP error (%s): %s" % (what, L.gcow_last_error().decode()), returncode=3)
    assert st == 0, "%s: %s" % (what, L.gcow_last_error().decode())


def _dev(a):
    """A uint64 host array on the device (16-byte aligned, as every torch allocation)."""
    t = torch.from_numpy(np.array(a, np.uint64).view(np.int64)).cuda()
    assert t.data_ptr() % 16 == 0
    return t


def _field(ptr, out, shape, strides=None):
    """A zfp_input filled by hand: shape and element strides in numpy order (the slowest axis first)."""
    from gcow_amd._ffi import DTYPE_BF16, DTYPE_FLOAT, ZfpInput
    f = ZfpInput()
    f.dtype, f.data = (DTYPE_BF16 if out == "bf16" else DTYPE_FLOAT), ptr
    for i, n in enumerate(reversed(shape)):
        setattr(f, ("nx", "ny", "nz", "nw")[i], int(n))
        if strides is not None:
            setattr(f, ("sx", "sy", "sz", "sw")[i], int(strides[len(shape) - 1 - i]))
    return f


def _params(gc, c):
    return gc.expert(*D.params(c).tuple())


def _dense(shape, out="f32"):
    n = int(np.prod(shape))
    return D.Layout("dense", out, n + 2 * GUARD_ELEMS, GUARD_ELEMS, D._dense(shape))


def _fill_of(pattern, ndt):
    return np.array([D.PATTERNS[pattern]], np.int64).view(ndt)[0]


def _check_image(buf, lay, want_bits, fill, what):
    got = buf.cpu().numpy().view(want_bits.dtype)
    exp = D.image(lay, want_bits, fill)
    if not np.array_equal(got, exp):
        bad = np.flatnonzero(got != exp)
        inside = np.zeros(lay.alloc, bool)
        inside[np.flatnonzero(D.image(lay, np.ones_like(want_bits), 0))] = True
        pytest.fail("%s: %d of %d elements of the allocation differ (%d of them outside the view), the first at %d: "
                    "got %x, expected %x" % (what, bad.size, lay.alloc, int((~inside[bad]).sum()), bad[0],
                                             got[bad[0]], exp[bad[0]]))


def _decode_into(L, p, lay, shape, want_bits, pattern, d_in, in_bytes, k, d_index, stride, what):
    """One decode into the view `lay` of an allocation filled with the pattern; the whole allocation is compared."""
    ndt = want_bits.dtype
    fill = _fill_of(pattern, ndt)
    buf = torch.from_numpy(np.full(lay.alloc, fill, ndt).view(np.int32 if ndt == np.uint32 else np.int16)).cuda()
    assert buf.data_ptr() % 16 == 0
    f = _field(buf.data_ptr() + lay.offset * ndt.itemsize, lay.out, shape, lay.strides)
    if k == 0:
        st = L.gcow_decode_device(C.byref(f), C.byref(p), d_in, in_bytes, d_index, stride, _stream())
    else:
        st = L.gcow_decode_device_at(C.byref(f), C.byref(p), d_in, in_bytes, k, d_index, stride, _stream())
    _sync(L, st, what)
    _check_image(buf, lay, want_bits, fill, what)


def _index_of(c, stride):
    return _dev(D.reference(c).offs[:-1][::stride]) if stride else None


def _outs(c):
    return ("f32", "bf16") if len(c.shape) == 1 else ("f32",)


# ------------------------------------------------------------------------------------------------ 1. dirty tail
@pytest.mark.parametrize("c,stride", D.DIRTY_RUNS, ids=["%s-s%d" % (c.id, s) for c, s in D.DIRTY_RUNS])
def test_dirty_tail(gc, c, stride):
    L, p, r = _lib(), _params(gc, c), D.reference(c)
    assert L.gcow_max_output_bytes(C.byref(_field(None, "f32", c.shape)), C.byref(p)) == 8 * D.cap_words(c.shape, D.params(c))
    index = _index_of(c, stride)
    for pat in D.PATTERNS:
        for size in ("own", "exact", "cap"):  # in_bytes: the stream's words, those plus 2, the encoder's capacity
            in_words, alloc = D.buffer_words(c, size)
            words = _dev(D.dirty_stream(r, pat, alloc))
            for out in _outs(c):
                _decode_into(L, p, _dense(c.shape, out), c.shape, D.as_bits(D.decoded(c), out), pat, words.data_ptr(),
                             8 * in_words, 0, index.data_ptr() if stride else None, stride,
                             "%s buffer, %s poison, %s output" % (size, pat, out))


MEAN_RUNS = [(ps, ix) for ps in D.MEAN_PSETS for ix in ((None,) if E.is_fixed(ps) else D.MEAN_INDEXES)]
MEAN_LAYOUTS = [_dense((D.MEAN_N,)), D.Layout("f32-off1", "f32", D.MEAN_N + 8, 1, (1,)),
                D.Layout("f32-stride2", "f32", 2 * D.MEAN_N + 5, 2, (2,))]


def _mean_index(L, p, refs, form):
    """(device index, entries per stream, index_stride) of the W streams in the form 8, 16 or "packed16" (built on the
    device from the oracle's index every 8 blocks)."""
    if form != "packed16":
        per = [r.offs[:-1][::form] for r in refs]
        return _dev(np.concatenate(per)), per[0].size, form
    f = _field(None, "f32", (D.MEAN_N,))
    ne = L.gcow_index_entries(C.byref(f), 16)
    out = torch.full((len(refs) * ne,), -1, dtype=torch.int64, device="cuda")
    for i, r in enumerate(refs):
        idx8 = _dev(r.offs[:-1][::8])
        assert idx8.numel() == L.gcow_index_entries(C.byref(f), 8)
        st = L.gcow_index_pack16_device(C.byref(f), C.byref(p), idx8.data_ptr(), out[i * ne:].data_ptr(), _stream())
        _sync(L, st, "gcow_index_pack16_device")
    return out, ne, INDEX_PACKED16


@pytest.mark.parametrize("pset,form", MEAN_RUNS, ids=["%s-%s" % (ps, ix) for ps, ix in MEAN_RUNS])
def test_decode_mean_dirty_slots(gc, pset, form):
    """W = 3 streams an odd number of words apart, every slot poisoned from its own stream's end on; into a contiguous
    output, one whose base is 4 bytes off 16, and one at stride 2."""
    L = _lib()
    p = gc.expert(*E.params(pset, 1).tuple())
    refs, mean = D.mean_reference(pset)
    index, index_words, index_stride = (None, 0, 0) if form is None else _mean_index(L, p, refs, form)
    want = D.as_bits(mean, "f32")
    for pat in D.PATTERNS:
        words, sw = D.mean_streams(pset, pat)
        d_words = _dev(words)
        fill = _fill_of(pat, np.dtype(np.uint32))
        for lay in MEAN_LAYOUTS:
            buf = torch.from_numpy(np.full(lay.alloc, fill, np.uint32).view(np.int32)).cuda()
            f = _field(buf.data_ptr() + 4 * lay.offset, "f32", (D.MEAN_N,), lay.strides)
            st = L.gcow_decode_mean_device(C.byref(f), C.byref(p), d_words.data_ptr(), 8 * words.size, sw, D.MEAN_W,
                                           index.data_ptr() if index is not None else None, index_words, index_stride,
                                           _stream())
            _sync(L, st, "gcow_decode_mean_device, %s" % lay.name)
            _check_image(buf, lay, want, fill, "%s poison, %s" % (pat, lay.name))


# ------------------------------------------------------------------------------------------------ 2. bit offsets
@pytest.mark.parametrize("c,stride,ks,sizes", D.OFFSET_RUNS, ids=["%s-s%d" % (c.id, s) for c, s, _, _ in D.OFFSET_RUNS])
def test_bit_offsets(gc, c, stride, ks, sizes):
    L, p, r = _lib(), _params(gc, c), D.reference(c)
    index = _index_of(c, stride)  # unshifted: entries are relative to bit_offset
    for k in ks:
        for pat in D.PATTERNS:
            for size in sizes:
                in_words, alloc = D.buffer_words(c, size, k)
                words = _dev(D.dirty_stream(r, pat, alloc, k))
                for out in _outs(c):
                    _decode_into(L, p, _dense(c.shape, out), c.shape, D.as_bits(D.decoded(c), out), pat,
                                 words.data_ptr(), 8 * in_words, k, index.data_ptr() if stride else None, stride,
                                 "bit_offset %d, %s buffer, %s poison, %s output" % (k, size, pat, out))


# ------------------------------------------------------------------------------------------------ 3. sub-fields
@pytest.mark.parametrize("c,stride,cuts", D.SUBFIELD_RUNS, ids=[c.id for c, _, _ in D.SUBFIELD_RUNS])
def test_subfield_random_access(gc, c, stride, cuts):
    L, p, r = _lib(), _params(gc, c), D.reference(c)
    in_words, alloc = D.buffer_words(c, "exact")
    words = _dev(D.dirty_stream(r, "5a", alloc))
    index = _index_of(c, stride)
    whole = D.decoded(c)
    for lo, hi, first, bit_offset, entry in D.subfield_parts(c, stride, cuts):
        shape = (hi - lo,) + c.shape[1:]
        _decode_into(L, p, _dense(shape), shape, D.as_bits(whole[lo:hi], "f32"), "5a", words.data_ptr(), 8 * in_words,
                     bit_offset, index.data_ptr() + 8 * entry if stride else None, stride,
                     "rows %d..%d from block %d" % (lo, hi, first))


# ------------------------------------------------------------------------------------------------ 4. output layouts
LAYOUT_RUNS = [(D.BY_ID[cid], s, lay) for dims in sorted(D.LAYOUT_CASES) for cid, s in D.LAYOUT_CASES[dims]
               for lay in D.layouts(D.BY_ID[cid].shape)]


@pytest.mark.parametrize("c,stride,lay", LAYOUT_RUNS, ids=["%s-%s" % (c.id, lay.name) for c, _, lay in LAYOUT_RUNS])
def test_output_layouts(gc, c, stride, lay):
    L, p, r = _lib(), _params(gc, c), D.reference(c)
    in_words, alloc = D.buffer_words(c, "exact")
    words = _dev(D.dirty_stream(r, "ones", alloc))
    index = _index_of(c, stride)
    for pat in D.PATTERNS:
        _decode_into(L, p, lay, c.shape, D.as_bits(D.decoded(c), lay.out), pat, words.data_ptr(), 8 * in_words, 0,
                     index.data_ptr() if stride else None, stride, "%s fill" % pat)


# ------------------------------------------------------------------------------------------------ 5. index strides
@pytest.mark.parametrize("cid", D.STRIDE_CASES)
def test_index_strides(gc, cid):
    c = D.BY_ID[cid]
    L, p, r = _lib(), _params(gc, c), D.reference(c)
    in_words, alloc = D.buffer_words(c, "exact")
    words = _dev(D.dirty_stream(r, "5a", alloc))
    whole = D.decoded(c)
    for s in D.INDEX_STRIDES:
        index = _index_of(c, s)
        _decode_into(L, p, _dense(c.shape), c.shape, D.as_bits(whole, "f32"), "5a", words.data_ptr(), 8 * in_words, 0,
                     index.data_ptr(), s, "index stride %d" % s)
        if len(c.shape) == 1:  # the first blocks alone: the largest strides exceed their count
            shape = (D.PREFIX_1D,)
            _decode_into(L, p, _dense(shape), shape, D.as_bits(whole[:D.PREFIX_1D], "f32"), "5a", words.data_ptr(),
                         8 * in_words, 0, index.data_ptr(), s, "index stride %d, the first %d values" % (s, D.PREFIX_1D))


def test_index_stride_4d(gc):
    """A 4-D index is used at stride 1; at any other stride it is ignored (never read: here it holds poison) and the
    stream is walked in order."""
    c = D.BY_ID["d4-6x5x7x10-acc1e-4-f32"]
    L, p, r = _lib(), _params(gc, c), D.reference(c)
    in_words, alloc = D.buffer_words(c, "exact")
    words = _dev(D.dirty_stream(r, "ones", alloc))
    poison = torch.full((E.nblocks(c.shape),), -1, dtype=torch.int64, device="cuda")
    for s, index in ((1, _index_of(c, 1)), (4, poison)):
        _decode_into(L, p, _dense(c.shape), c.shape, D.as_bits(D.decoded(c), "f32"), "ones", words.data_ptr(),
                     8 * in_words, 0, index.data_ptr(), s, "index stride %d" % s)


# ------------------------------------------------------------------------------------------------ 6. d_in at 8 mod 16
@pytest.mark.parametrize("cid,stride", D.ODD_WORD_RUNS, ids=[i for i, _ in D.ODD_WORD_RUNS])
def test_stream_pointer_at_an_odd_word(gc, cid, stride):
    """d_in needs the alignment of its 64-bit words, no more: the staged kernels round a span's start down to 16 bytes
    relative to d_in, and their 16-byte loads are buffer loads, which need 4-byte alignment."""
    c = D.BY_ID[cid]
    L, p, r = _lib(), _params(gc, c), D.reference(c)
    index = _index_of(c, stride)
    for size in ("exact", "cap"):
        in_words, alloc = D.buffer_words(c, size)
        host = np.concatenate([np.full(1, D.PATTERNS["5a"], np.int64).view(np.uint64), D.dirty_stream(r, "5a", alloc)])
        words = _dev(host)
        d_in = words.data_ptr() + 8
        assert d_in % 16 == 8
        for out in _outs(c):
            _decode_into(L, p, _dense(c.shape, out), c.shape, D.as_bits(D.decoded(c), out), "5a", d_in, 8 * in_words, 0,
                         index.data_ptr() if stride else None, stride, "%s buffer, %s output" % (size, out))
