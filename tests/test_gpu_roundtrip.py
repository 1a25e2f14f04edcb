"""GPU parity of the fused round trip (gcow_roundtrip_device, include/gcow.h), bitwise: the output equals the oracle's
decompress(compress(x)) (a bf16 output: that, rounded to nearest even) and the device's own decode(encode(x)); the bit
count equals the oracle's; out of place, in place, 16-byte-misaligned views, the bytes after the output, argument
checks, and roundtrip_hook over a one-rank RCCL group.

Sizes: one value, partial and whole single blocks, and the fused kernels' workgroup chunk (256 lanes x 8 blocks = 8192
values, the same for the fixed-rate and the no-budget kernel) - 1, + 0, + 1, and three chunks plus a partial block.
Modes (tests/roundtrip_inputs.py): rate 16 / 8 run the lean fixed-rate kernel; accuracy 1e-3 / 1e-6 / 0, precision 12
and expert(1, 160, 20, -30) the no-budget kernel; rate 12, expert(64, 64, 20, -1074), expert(8, 512, 32, -1074) (the
minbits pad) and expert(1, 100, 64, -30) (the budget truncates) the generic kernel."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

torch = pytest.importorskip("torch")

TESTS = os.path.dirname(os.path.abspath(__file__))
if TESTS not in sys.path:
    sys.path.insert(0, TESTS)

pytestmark = pytest.mark.gpu

SIZES = [1, 3, 4, 5, 8191, 8192, 8193, 24583]
MODE_NAMES = ["rate16", "rate8", "acc1e-3", "acc1e-6", "acc0", "prec12", "expert_nobudget", "rate12",
              "expert64_prec20", "expert_minbits_pad", "expert_trunc"]
DTYPES = [(False, False), (False, True), (True, False), (True, True)]
DTYPE_IDS = ["fp32-fp32", "fp32-bf16", "bf16-fp32", "bf16-bf16"]
SENT = -1234.5  # exact in bf16 too
SENT_BITS = 0x5A5A5A5A5A5A5A5A


@pytest.fixture(scope="module")
def gc():
    if not torch.cuda.is_available():
        pytest.fail("GPU tests need a device")
    from gcow_amd import codec
    return codec


def _dev(a):
    t = torch.from_numpy(np.array(a)).cuda()  # a writable copy: the cases' arrays are shared and read-only
    return t.view(torch.bfloat16) if a.dtype == np.uint16 else t


def _bits_of(t):
    """The tensor's values as raw bits (uint32 for fp32, uint16 for bf16)."""
    if t.dtype == torch.bfloat16:
        return t.view(torch.int16).cpu().numpy().view(np.uint16)
    return t.cpu().numpy().view(np.uint32)


def _want(d, bf16_out):
    from roundtrip_inputs import bf16_rne
    return bf16_rne(d) if bf16_out else d.view(np.uint32)


def _tdtype(bf16):
    return torch.bfloat16 if bf16 else torch.float32


@pytest.mark.parametrize("mode", MODE_NAMES)
@pytest.mark.parametrize("bf16_in,bf16_out", DTYPES, ids=DTYPE_IDS)
@pytest.mark.parametrize("n", SIZES)
def test_roundtrip_matches_oracle(gc, orc, n, bf16_in, bf16_out, mode):
    from roundtrip_inputs import MODES, case
    x_np, d_ref, bits_ref = case(n, bf16_in, mode)
    p = gc.expert(*MODES[mode]().tuple())
    want = _want(d_ref, bf16_out)
    x = _dev(x_np)
    # out of place into a sentinel-filled buffer, with the bit count
    buf = torch.full((n + 16,), SENT, dtype=_tdtype(bf16_out), device="cuda")
    bits = torch.full((1,), -1, dtype=torch.int64, device="cuda")
    got = gc.roundtrip(x, p, out=buf[:n], bits=bits)
    torch.cuda.synchronize()
    assert got.data_ptr() == buf.data_ptr()
    assert np.array_equal(_bits_of(buf[:n]), want)
    assert bool((buf[n:] == SENT).all())
    assert np.array_equal(_bits_of(x), x_np.view(np.uint16 if bf16_in else np.uint32))  # the input is only read
    assert int(bits.item()) == bits_ref
    # bits=None: a new tensor of x's dtype, and nothing writes a bit counter
    counter = torch.full((1,), SENT_BITS, dtype=torch.int64, device="cuda")
    got2 = gc.roundtrip(x, p)
    torch.cuda.synchronize()
    assert got2.dtype == x.dtype and got2.data_ptr() != x.data_ptr()
    assert np.array_equal(_bits_of(got2), _want(d_ref, bf16_in))
    assert int(counter.item()) == SENT_BITS
    # in place (equal dtypes): the same result
    if bf16_in == bf16_out:
        buf2 = torch.full((n + 16,), SENT, dtype=_tdtype(bf16_out), device="cuda")
        buf2[:n] = x
        bits2 = torch.full((1,), -1, dtype=torch.int64, device="cuda")
        gc.roundtrip(buf2[:n], p, out=buf2[:n], bits=bits2)
        torch.cuda.synchronize()
        assert np.array_equal(_bits_of(buf2[:n]), want)
        assert bool((buf2[n:] == SENT).all()) and int(bits2.item()) == bits_ref
    # "what encode followed by decode leaves": the device's own composition
    e = gc.encode(x, p, index_stride=0 if gc.is_fixed(p) else 16)
    comp = gc.decode(e, out=torch.empty(n, dtype=_tdtype(bf16_out), device="cuda"))
    torch.cuda.synchronize()
    assert e.bits == bits_ref
    assert np.array_equal(_bits_of(comp), want)


@pytest.mark.parametrize("mode", ["rate16", "acc1e-3"])
@pytest.mark.parametrize("bf16_in,bf16_out", DTYPES, ids=DTYPE_IDS)
@pytest.mark.parametrize("n", [5, 8193])
def test_roundtrip_misaligned_views(gc, orc, n, bf16_in, bf16_out, mode):
    """x_big[1 : n + 1] into out_big[1 : n + 1]: one element off 16-byte alignment, the generic kernel."""
    from roundtrip_inputs import MODES, case
    x_np, d_ref, bits_ref = case(n, bf16_in, mode)
    p = gc.expert(*MODES[mode]().tuple())
    x_big = torch.zeros(n + 17, dtype=_tdtype(bf16_in), device="cuda")
    x_big[1:n + 1] = _dev(x_np)
    out_big = torch.full((n + 17,), SENT, dtype=_tdtype(bf16_out), device="cuda")
    bits = torch.full((1,), -1, dtype=torch.int64, device="cuda")
    assert x_big[1:].data_ptr() % 16 and out_big[1:].data_ptr() % 16
    gc.roundtrip(x_big[1:n + 1], p, out=out_big[1:n + 1], bits=bits)
    torch.cuda.synchronize()
    assert np.array_equal(_bits_of(out_big[1:n + 1]), _want(d_ref, bf16_out))
    assert bool((out_big[:1] == SENT).all()) and bool((out_big[n + 1:] == SENT).all())
    assert int(bits.item()) == bits_ref


def test_flattened_contiguous_input(gc, orc):
    """A contiguous 2-D tensor is taken as its flattening (a DDP bucket view)."""
    a = orc.gen_normal(64 * 33, 1e-3, 3, True)
    op = orc.accuracy(1e-3)
    want = orc.decompress(orc.compress(a, op)[0], a.shape, op)
    got = gc.roundtrip(torch.from_numpy(a).cuda().view(64, 33), gc.accuracy(1e-3))
    torch.cuda.synchronize()
    assert got.shape == (64, 33)
    assert np.array_equal(got.cpu().numpy().reshape(-1).view(np.uint32), want.view(np.uint32))


def test_argument_checks(gc, orc):
    from gcow_amd._ffi import load
    L = load()
    p = gc.rate(16, 1)
    st = torch.cuda.current_stream().cuda_stream
    out = torch.zeros(64, device="cuda")
    x2 = torch.zeros(8, 8, device="cuda")
    assert L.gcow_roundtrip_device(C.byref(gc.field_of(x2)), C.byref(p), out.data_ptr(), 3, None, st) == 5  # 2-D
    xs = torch.zeros(128, device="cuda")[::2]
    for q in (p, gc.accuracy(1e-3)):
        assert L.gcow_roundtrip_device(C.byref(gc.field_of(xs)), C.byref(q), out.data_ptr(), 3, None, st) == 5  # strided
    x = torch.zeros(64, device="cuda")
    f = gc.field_of(x)
    f.dtype = 4  # dtype_double
    assert L.gcow_roundtrip_device(C.byref(f), C.byref(p), out.data_ptr(), 3, None, st) == 5
    assert L.gcow_roundtrip_device(C.byref(gc.field_of(x)), C.byref(p), out.data_ptr(), 4, None, st) == 5  # out_dtype
    assert L.gcow_roundtrip_device(C.byref(gc.field_of(x)), C.byref(p), None, 3, None, st) == 1            # NULL d_out
    # nx = 0: OK, bits = 0, for a fixed and a variable rate
    for q in (p, gc.accuracy(1e-3)):
        f0 = gc.field_of(x)
        f0.nx = 0
        bits = torch.full((1,), -1, dtype=torch.int64, device="cuda")
        assert L.gcow_roundtrip_device(C.byref(f0), C.byref(q), out.data_ptr(), 3, bits.data_ptr(), st) == 0
        torch.cuda.synchronize()
        assert int(bits.item()) == 0
    with pytest.raises(gc.GcowError):
        gc.roundtrip(x, p, out=torch.zeros(63, device="cuda"))
    with pytest.raises(gc.GcowError):
        gc.roundtrip(x, p, out=torch.zeros(64, device="cuda", dtype=torch.float16))
    with pytest.raises(gc.GcowError):
        gc.roundtrip(x.to(torch.float16), p)
    with pytest.raises(gc.GcowError):
        gc.roundtrip(xs, p)


# ---------------------------------------------------------------------------------------------- roundtrip_hook, RCCL
@pytest.fixture
def nccl_world1():
    import torch.distributed as dist
    dist.init_process_group("nccl", store=dist.HashStore(), rank=0, world_size=1, device_id=torch.device("cuda", 0))
    yield
    dist.destroy_process_group()


class _Bucket:
    def __init__(self, t, i):
        self.t, self.i = t, i

    def buffer(self):
        return self.t

    def index(self):
        return self.i


@pytest.mark.parametrize("mode", ["rate16", "acc1e-3", "rate12"])
@pytest.mark.parametrize("bf16", [False, True], ids=["fp32", "bf16"])
def test_roundtrip_hook_world1(gc, orc, nccl_world1, bf16, mode):
    """One rank over RCCL, two buckets, the device codec: the hook calls roundtrip and never encode, and every bucket
    comes back as the oracle's decode (a bf16 bucket: rounded to nearest even)."""
    from gcow_amd import ddp
    from gcow_amd import dist as gdist
    from roundtrip_inputs import MODES, case

    calls = []

    class CountingCodec(gdist.DeviceCodec):
        def roundtrip(self, *a, **k):
            calls.append("roundtrip")
            return super().roundtrip(*a, **k)

        def encode(self, *a, **k):
            calls.append("encode")
            return super().encode(*a, **k)

    p = gc.expert(*MODES[mode]().tuple())
    state = ddp.make_hook_state(hook=ddp.roundtrip_hook, params=p, codec=CountingCodec())
    for i, n in enumerate((24583, 8193)):
        x_np, d_ref, _ = case(n, bf16, mode)
        t = _dev(x_np).clone()
        out = ddp.roundtrip_hook(state, _Bucket(t, i)).wait()
        torch.cuda.synchronize()
        out = out[0] if isinstance(out, (list, tuple)) else out
        assert out.data_ptr() == t.data_ptr()
        assert np.array_equal(_bits_of(out), _want(d_ref, bf16)), i
    assert calls == ["roundtrip", "roundtrip"]
