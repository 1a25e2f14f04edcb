"""The fused round trip (gcow_roundtrip_device, include/gcow.h) as far as it can be checked without a GPU: the symbol
and its argument checks (decided before any device call), the Python entry points, roundtrip_hook's choice between one
`roundtrip` call and encode -> decode (over a one-rank gloo group with oracle-backed codecs), and a numpy restatement
of the identity behind the no-budget kernel -- decoded coefficients = coded coefficients with the planes below the
block's precision cleared -- against the oracle's decompress(compress(x))."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

torch = pytest.importorskip("torch")
import torch.distributed as dist  # noqa: E402

TESTS = os.path.dirname(os.path.abspath(__file__))
if TESTS not in sys.path:
    sys.path.insert(0, TESTS)

GCOW_ERR_INVALID, GCOW_ERR_UNSUPPORTED = 1, 5


def _field(nx, ny=0, dtype=3, data=0x1000):
    from gcow_amd._ffi import ZfpInput
    f = ZfpInput()
    f.dtype, f.data, f.nx, f.ny = dtype, data, nx, ny
    return f


def test_symbol_exported_and_declared():
    from gcow_amd import _ffi
    L = _ffi.load()
    assert hasattr(L, "gcow_roundtrip_device")
    assert "gcow_roundtrip_device" in _ffi.header_functions()
    assert L.gcow_roundtrip_device.argtypes is not None and len(L.gcow_roundtrip_device.argtypes) == 6


def test_argument_checks_before_any_device_call():
    from gcow_amd import _ffi, codec
    L = _ffi.load()
    p = codec.rate(16, 1)
    f = _field(64)
    out = 0x2000  # never dereferenced: every call below is refused on the host
    assert L.gcow_roundtrip_device(None, C.byref(p), out, 3, None, None) == GCOW_ERR_INVALID
    assert L.gcow_roundtrip_device(C.byref(f), None, out, 3, None, None) == GCOW_ERR_INVALID
    assert L.gcow_roundtrip_device(C.byref(f), C.byref(p), None, 3, None, None) == GCOW_ERR_INVALID
    assert L.gcow_roundtrip_device(C.byref(_field(8, 8)), C.byref(p), out, 3, None, None) == GCOW_ERR_UNSUPPORTED
    fs = _field(64)
    fs.sx = 2
    assert L.gcow_roundtrip_device(C.byref(fs), C.byref(p), out, 3, None, None) == GCOW_ERR_UNSUPPORTED
    assert L.gcow_roundtrip_device(C.byref(_field(64, dtype=4)), C.byref(p), out, 3, None, None) == GCOW_ERR_UNSUPPORTED
    assert L.gcow_roundtrip_device(C.byref(f), C.byref(p), out, 4, None, None) == GCOW_ERR_UNSUPPORTED
    assert L.gcow_roundtrip_device(C.byref(f), C.byref(p), out + 2, 3, None, None) == GCOW_ERR_INVALID  # fp32 at 2 mod 4
    assert L.gcow_roundtrip_device(C.byref(_field(64, data=0x1001, dtype=5)), C.byref(p), out, 5, None,
                                   None) == GCOW_ERR_INVALID                                           # bf16 at 1 mod 2
    bad = codec.expert(8, 4, 32, -1074)  # check_params: maxbits < 9
    assert L.gcow_roundtrip_device(C.byref(f), C.byref(bad), out, 3, None, None) == GCOW_ERR_INVALID


def test_python_entry_points_exist():
    from gcow_amd import codec
    from gcow_amd import dist as gdist
    assert callable(codec.roundtrip)
    assert callable(gdist.DeviceCodec.roundtrip)
    with pytest.raises(codec.GcowError):
        codec.roundtrip(torch.zeros(16), codec.rate(16, 1))  # a host tensor


# ---------------------------------------------------------------------------------------------- the hook's choice
@pytest.fixture
def gloo_world1():
    dist.init_process_group("gloo", store=dist.HashStore(), rank=0, world_size=1)
    yield
    dist.destroy_process_group()


class _Bucket:
    def __init__(self, t, i):
        self.t, self.i = t, i

    def buffer(self):
        return self.t

    def index(self):
        return self.i


def _roundtrip_codec():
    from oracle import oracle as O
    from oracle_codec import OracleCodec, _np_values, _params

    class OracleRoundtripCodec(OracleCodec):
        def roundtrip(self, x, params, out=None):
            a = _np_values(x)
            p = _params(params)
            d = torch.from_numpy(O.decompress(O.compress(a, p)[0], (a.size,), p))
            self.records.append(("roundtrip", a))
            if out is None:
                return d.to(x.dtype)
            out.copy_(d)
            return out

    return OracleRoundtripCodec()


@pytest.mark.parametrize("mode", ["rate16", "acc1e-3", "rate12"])
@pytest.mark.parametrize("bf16", [False, True], ids=["fp32", "bf16"])
def test_roundtrip_hook_uses_roundtrip_when_the_codec_has_it(orc, gloo_world1, mode, bf16):
    from gcow_amd import codec, ddp
    from oracle_codec import OracleCodec
    from roundtrip_inputs import MODES, bf16_rne, inputs
    op = MODES[mode]()
    p = codec.expert(*op.tuple())
    for cdc, used in ((_roundtrip_codec(), "roundtrip"), (OracleCodec(), "encode")):
        state = ddp.make_hook_state(hook=ddp.roundtrip_hook, params=p, codec=cdc)
        for i, n in enumerate((1027, 64)):
            x = inputs(n, bf16, seed=40 + i)
            d = orc.decompress(orc.compress(x, op)[0], (n,), op)
            t = torch.from_numpy(x.copy())
            t = t.view(torch.bfloat16) if bf16 else t
            out = ddp.roundtrip_hook(state, _Bucket(t, i)).wait()
            out = out[0] if isinstance(out, (list, tuple)) else out
            assert out.data_ptr() == t.data_ptr()  # the bucket, in place
            if bf16:
                assert np.array_equal(out.view(torch.int16).numpy().view(np.uint16), bf16_rne(d))
            else:
                assert np.array_equal(out.numpy().view(np.uint32), d.view(np.uint32))
        names = [r[0] for r in cdc.records]
        assert names.count(used) == 2
        if used == "roundtrip":
            assert "encode" not in names


def test_roundtrip_hook_other_dtypes_keep_the_composed_path(orc, gloo_world1):
    """An fp16 bucket is not a roundtrip field: encode -> decode through an fp32 copy, as before."""
    from gcow_amd import codec, ddp
    cdc = _roundtrip_codec()
    state = ddp.make_hook_state(hook=ddp.roundtrip_hook, params=codec.rate(16, 1), codec=cdc)
    a = orc.gen_normal(256, 1e-3, 5, False)
    t = torch.from_numpy(a).to(torch.float16)
    want = orc.decompress(orc.compress(t.float().numpy(), orc.rate(16, 1))[0], (256,), orc.rate(16, 1))
    out = ddp.roundtrip_hook(state, _Bucket(t, 0)).wait()
    out = out[0] if isinstance(out, (list, tuple)) else out
    assert torch.equal(out, torch.from_numpy(want).to(torch.float16))
    names = [r[0] for r in cdc.records]
    assert "encode" in names and "roundtrip" not in names


# ---------------------------------------------------------------------------------------------- the mask identity
@pytest.mark.parametrize("mode", ["acc1e-3", "acc1e-6", "acc0", "prec12", "expert_nobudget"])
@pytest.mark.parametrize("bf16", [False, True], ids=["fp32", "bf16"])
def test_mask_identity_matches_oracle(orc, mode, bf16):
    """~2000 blocks of the GPU tests' generator (gradient-like, zero, subnormal, NaN / Inf, 3e38, wide-exponent,
    sparse, constant, alternating, ramp): clearing the planes below kmin is the whole round trip."""
    from roundtrip_inputs import MODES, inputs, mask_identity, widen
    op = MODES[mode]()
    x = inputs(8192, bf16)
    want = orc.decompress(orc.compress(x, op)[0], (x.size,), op)
    got = mask_identity(widen(x), op)
    assert np.array_equal(got.view(np.uint32), want.view(np.uint32))
    assert np.any(want != widen(x)) and np.any(want)  # lossy and not all zero: the check shows something
