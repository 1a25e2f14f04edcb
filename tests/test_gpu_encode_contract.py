"""The contract of gcow_encode_device, gcow_encode_device_append and gcow_decode_device (include/gcow.h) under the
conditions the parity suite never sets up, bit for bit against the oracle:

  - every encoder writes into buffers that are NOT zero: the stream buffer (gcow_max_output_bytes plus 4 guard
    words), the workspace, the block index (plus 4 guard entries) and the bit count are filled with all ones or with
    0x5A5A5A5A5A5A5A5A before the call. The header asks for zeroed memory only in gcow_stitch_device, so every word the
    encoders OR into has to be cleared by them (the words two ranges share, by the scans), and the stream's flush word
    has to be stored. Then the same buffers take a second input with a shorter stream, as a preallocated
    codec.Encoder does every step;
  - ranges of more than one 256-block tile (k_encode_tiles' loop, its carry word and its cut at a partial word), which
    need more than 524288 blocks;
  - gcow_encode_device_append for the generic 1-D coder, 2-D, 3-D (next to an oversized tile) and 4-D, with an empty
    chunk and a chunk of one row of blocks, chained through the device bit counts;
  - every decoder into an output with 16 guard elements on either side, from the oracle's stream and index.

Cases, inputs and expectations: encode_contract_inputs.py (test_encode_contract_cpu.py checks that each input reaches
what it is there for)."""
import contextlib
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

import encode_contract_inputs as I  # noqa: E402

GUARD_WORDS = 4
GUARD_ELEMS = 16


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


def _u64(fill):
    return np.array([fill], np.int64).view(np.uint64)[0]


def _device_input(c, a):
    """The case's input on the device, laid out as the case says; a view keeps its storage alive."""
    a = np.array(a)
    if c.view == "stride3":
        base = np.zeros(3 * a.size, a.dtype)
        base[::3] = a
        x = torch.from_numpy(base).cuda()
        x = (x.view(torch.bfloat16) if a.dtype == np.uint16 else x)[::3]
    elif c.view == "transposed":
        x = torch.from_numpy(np.ascontiguousarray(a.T)).cuda()
        x = (x.view(torch.bfloat16) if a.dtype == np.uint16 else x).t()
    else:
        x = torch.from_numpy(a).cuda()
        x = x.view(torch.bfloat16) if a.dtype == np.uint16 else x
    assert tuple(x.shape) == c.shape
    return x


class _Buffers:
    """Stream, workspace, index and bit count of one field, filled with `fill`."""

    def __init__(self, L, f, p, stride, fill, nbits=1, wsb=None):
        self.fill = fill
        self.cap = L.gcow_max_output_bytes(C.byref(f), C.byref(p))
        assert self.cap and self.cap % 8 == 0
        self.capw = self.cap // 8
        self.words = torch.full((self.capw + GUARD_WORDS,), fill, dtype=torch.int64, device="cuda")
        self.wsb = L.gcow_encode_workspace_bytes(C.byref(f), C.byref(p)) if wsb is None else wsb
        self.ws = torch.full(((self.wsb + 7) // 8 + 1,), fill, dtype=torch.int64, device="cuda")
        self.stride = stride
        self.ne = L.gcow_index_entries(C.byref(f), stride) if stride else 0
        self.index = torch.full((self.ne + GUARD_WORDS,), fill, dtype=torch.int64, device="cuda") if stride else None
        self.bits = torch.full((nbits,), fill, dtype=torch.int64, device="cuda")

    def check(self, ref, what):
        """The buffers against the oracle after a synchronise: words [0, ceil(bits / 64)) (the words between the
        stream's end and the capacity are unspecified), the guard words, the index and its guard entries."""
        nw = (ref.bits + 63) // 64
        assert nw == ref.words.size <= self.capw
        got = self.words[:nw].cpu().numpy().view(np.uint64)
        if not np.array_equal(got, ref.words):
            bad = np.flatnonzero(got != ref.words)
            pytest.fail("%s: %d of %d stream words differ, the first at word %d (got %016x, oracle %016x)"
                        % (what, bad.size, nw, bad[0], got[bad[0]], ref.words[bad[0]]))
        guard = self.words[self.capw:].cpu().numpy().view(np.uint64)
        assert (guard == _u64(self.fill)).all(), "%s: the words after the capacity were written" % what
        if self.stride:
            want = ref.offs[:-1][::self.stride]
            assert self.ne == want.size
            idx = self.index.cpu().numpy().view(np.uint64)
            assert np.array_equal(idx[:self.ne], want), "%s: block index" % what
            assert (idx[self.ne:] == _u64(self.fill)).all(), "%s: the entries after the index were written" % what


def _encode_and_check(gc, L, x, p, bufs, ref, what):
    f = gc.field_of(x)
    st = L.gcow_encode_device(C.byref(f), C.byref(p), bufs.words.data_ptr(), bufs.cap, bufs.bits.data_ptr(),
                              bufs.ws.data_ptr(), bufs.wsb, bufs.index.data_ptr() if bufs.stride else None,
                              bufs.stride, _stream())
    torch.cuda.synchronize()
    assert st == 0, "%s: %s" % (what, L.gcow_last_error().decode())
    assert int(bufs.bits.item()) == ref.bits, what  # fixed rate: nblocks * maxbits, the oracle's count as well
    bufs.check(ref, what)


RUNS = [(c, pat, s) for c in I.CASES for pat in c.patterns for s in c.strides]


@pytest.mark.parametrize("c,pat,stride", RUNS, ids=["%s-%s-s%d" % (c.id, pat, s) for c, pat, s in RUNS])
def test_encode_into_dirty_buffers(gc, c, pat, stride):
    L = _lib()
    op = I.params(c.pset, len(c.shape))
    p = gc.expert(*op.tuple())
    x1 = _device_input(c, I.case_input(c))
    x2 = _device_input(c, I.case_input(c, second=True))
    r1, r2 = I.reference(c), I.reference(c, second=True)
    if I.is_fixed(c.pset):
        assert r1.bits == I.nblocks(c.shape) * op.maxbits
    bufs = _Buffers(L, gc.field_of(x1), p, stride, I.PATTERNS[pat])
    with (gc.var1d_variant(c.form) if c.form else contextlib.nullcontext()):
        _encode_and_check(gc, L, x1, p, bufs, r1, "first call")
        # the Encoder reuse of every training step: the same buffers, as the first call left them
        _encode_and_check(gc, L, x2, p, bufs, r2, "second call")


APPEND_RUNS = [(ac, pat) for ac in I.APPEND_CASES for pat in I.PATTERNS]


@pytest.mark.parametrize("ac,pat", APPEND_RUNS, ids=["%s-%s" % (ac.id, pat) for ac, pat in APPEND_RUNS])
def test_append_into_dirty_buffers(gc, ac, pat):
    """The field cut along its slowest axis, every chunk appended at the device-side end of the one before it: the
    oracle's single stream and its absolute block index. An empty chunk (a field without extents) appends nothing."""
    from gcow_amd._ffi import DTYPE_FLOAT, ZfpInput
    L = _lib()
    op = I.params(ac.pset, len(ac.shape))
    p = gc.expert(*op.tuple())
    ref = I.append_reference(ac)
    x = torch.from_numpy(np.array(I.field(ac.field, ac.shape))).cuda()
    chunks = list(zip(ac.cuts, ac.cuts[1:]))
    # one workspace for all chunks, of the largest chunk's size
    wsb = max(L.gcow_encode_workspace_bytes(C.byref(gc.field_of(x[lo:hi])), C.byref(p)) for lo, hi in chunks if hi > lo)
    bufs = _Buffers(L, gc.field_of(x), p, 1, I.PATTERNS[pat], nbits=len(chunks) + 1, wsb=wsb)
    bufs.bits[0] = 0
    per_row = I.nblocks(ac.shape) // ((ac.shape[0] + 3) // 4)
    ends = []
    for i, (lo, hi) in enumerate(chunks):
        if hi > lo:
            f = gc.field_of(x[lo:hi])
        else:  # zfp_input has no zero extent on a slow axis: the empty chunk is the field without extents
            f = ZfpInput()
            f.dtype, f.data = DTYPE_FLOAT, x.data_ptr()
        before = lo // 4 * per_row
        st = L.gcow_encode_device_append(C.byref(f), C.byref(p), bufs.words.data_ptr(), bufs.cap,
                                         bufs.bits[i:].data_ptr(), bufs.bits[i + 1:].data_ptr(), bufs.ws.data_ptr(), wsb,
                                         bufs.index.data_ptr() + 8 * before, 1, _stream())
        assert st == 0, "chunk %d: %s" % (i, L.gcow_last_error().decode())
        ends.append(int(ref.offs[min((hi + 3) // 4 * per_row, ref.offs.size - 1)]))
    torch.cuda.synchronize()
    assert bufs.bits.cpu().tolist() == [0] + ends and ends[-1] == ref.bits
    bufs.check(ref, "appended stream")


def _decode_runs():
    runs, seen = [], set()
    for c in I.SMALL_CASES:
        key = (c.field, c.shape, c.dtype, c.pset)
        if key in seen:  # a view, an encoder form or an index of the same stream
            continue
        seen.add(key)
        strides = (0,) if I.is_fixed(c.pset) else (1, 2)
        for s in strides:
            for out in (("f32", "bf16") if len(c.shape) == 1 else ("f32",)):
                runs.append((c, s, out))
    return runs


DECODE_RUNS = _decode_runs()


@pytest.mark.parametrize("c,stride,out", DECODE_RUNS, ids=["%s-s%d-%s" % (c.id, s, o) for c, s, o in DECODE_RUNS])
def test_decode_into_guarded_output(gc, c, stride, out):
    """The oracle's stream and index (not the encoder's) decoded into a pattern-filled buffer with guard elements on
    either side of the field: oracle.decompress bit for bit, the guards untouched."""
    from roundtrip_inputs import bf16_rne
    L = _lib()
    op = I.params(c.pset, len(c.shape))
    p = gc.expert(*op.tuple())
    r = I.reference(c)
    want = I.decoded(c.field, c.shape, c.dtype, c.pset).reshape(-1)
    words = torch.from_numpy(np.concatenate([r.words, np.zeros(2, np.uint64)]).view(np.int64)).cuda()
    index = torch.from_numpy(r.offs[:-1][::stride].astype(np.int64)).cuda() if stride else None
    n = want.size
    tdt, ndt, edt = ((torch.int32, np.uint32, torch.float32) if out == "f32"
                     else (torch.int16, np.uint16, torch.bfloat16))
    want_bits = want.view(np.uint32) if out == "f32" else bf16_rne(want)
    nan = np.isnan(want)  # a NaN's payload is the device's
    for fill in I.PATTERNS.values():
        fill = fill & 0xFFFFFFFF if out == "f32" else fill & 0xFFFF
        fill_t = int(np.array([fill], ndt).view(np.int32 if out == "f32" else np.int16)[0])
        buf = torch.full((n + 2 * GUARD_ELEMS,), fill_t, dtype=tdt, device="cuda")
        dst = buf.view(edt)[GUARD_ELEMS:GUARD_ELEMS + n].view(c.shape)
        f = gc.field_of(dst)
        st = L.gcow_decode_device(C.byref(f), C.byref(p), words.data_ptr(), words.numel() * 8,
                                  index.data_ptr() if stride else None, stride, _stream())
        torch.cuda.synchronize()
        assert st == 0, L.gcow_last_error().decode()
        got = buf.cpu().numpy().view(ndt)
        assert (got[:GUARD_ELEMS] == fill).all() and (got[GUARD_ELEMS + n:] == fill).all(), "guard elements written"
        body = got[GUARD_ELEMS:GUARD_ELEMS + n]
        got_nan = np.isnan(body.view(np.float32)) if out == "f32" else (body & 0x7FFF) > 0x7F80
        assert np.array_equal(got_nan, nan)
        assert np.array_equal(body[~nan], want_bits[~nan])
