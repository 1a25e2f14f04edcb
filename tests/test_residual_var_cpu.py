"""Error feedback at variable rate (gcow_encode_residual_device's GCOW_RESID_FUSED_VAR path, include/gcow.h) as far as
it can be checked without a GPU: the path query and the workspace size, both decided on the host from the arguments
alone (pointers are looked at for alignment, never dereferenced), and that the shared inputs of the GPU tests
(residual_var_inputs.py) reach what they claim: tiles on both sides of the tile coder's 1500-qword window, an Inf / NaN
block, a block that decodes to -0."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

torch = pytest.importorskip("torch")

TESTS = os.path.dirname(os.path.abspath(__file__))
if TESTS not in sys.path:
    sys.path.insert(0, TESTS)

COMPOSED, FUSED_FIXED, FUSED_VAR = 0, 1, 2
SIZES = [24583, 1 << 20]
DTYPES = [3, 5]  # dtype_float, dtype_bf16
X, E = 0x7F0000001000, 0x7F0000100000  # 16-byte aligned pointer values, never dereferenced


def _field(nx, ny=0, dtype=3, data=X):
    from gcow_amd._ffi import ZfpInput
    f = ZfpInput()
    f.dtype, f.data, f.nx, f.ny = dtype, data, nx, ny
    return f


def _sets():
    from gcow_amd import codec
    return [(codec.accuracy(1e-3), FUSED_VAR), (codec.accuracy(1e-6), FUSED_VAR), (codec.precision(12), FUSED_VAR),
            (codec.precision(32), FUSED_VAR), (codec.expert(1, 4096, 24, -40), FUSED_VAR),
            (codec.rate(16, 1), FUSED_FIXED), (codec.rate(12, 1), COMPOSED),
            (codec.expert(1, 100, 32, -1074), COMPOSED)]


def test_symbol_exported_and_declared():
    from gcow_amd import _ffi
    L = _ffi.load()
    assert hasattr(L, "gcow_encode_residual_path")
    assert "gcow_encode_residual_path" in _ffi.header_functions()
    assert len(L.gcow_encode_residual_path.argtypes) == 5


@pytest.mark.parametrize("dtype", DTYPES, ids=["fp32", "bf16"])
@pytest.mark.parametrize("n", SIZES)
def test_path_query(n, dtype):
    from gcow_amd import _ffi
    L = _ffi.load()
    f = _field(n, dtype=dtype)
    for p, want in _sets():
        q = lambda *a: L.gcow_encode_residual_path(C.byref(f), C.byref(p), *a)  # noqa: E731
        assert q(E, E, None) == want, p.tuple()
        assert q(None, E, None) == want               # no input error: nothing to misalign
        assert q(None, None, None) == want            # NULL: assume aligned
        # the coder writes the caller's index on the variable-rate path; the fixed-rate kernel has none
        assert q(E, E, 0x7F0000200000) == (want if want != FUSED_FIXED else COMPOSED)
        # an e pointer at 4 mod 16: composed at every parameter set
        assert q(E + 4, E + 4, None) == COMPOSED
        assert q(E, E + 4, None) == COMPOSED
        assert q(E + 4, E, None) == COMPOSED
        assert q(E + 2, E, None) == -1                # not a float pointer: refused
        # the bucket off 16-byte alignment: composed for the variable-rate sets
        g = _field(n, dtype=dtype, data=X + 8)
        got = L.gcow_encode_residual_path(C.byref(g), C.byref(p), E, E, None)
        assert got == (COMPOSED if want == FUSED_VAR or dtype == 3 else want)
        # refused calls
        assert L.gcow_encode_residual_path(C.byref(_field(64, 64, dtype)), C.byref(p), E, E, None) == -1
        fs = _field(n, dtype=dtype)
        fs.sx = 2
        assert L.gcow_encode_residual_path(C.byref(fs), C.byref(p), E, E, None) == -1
        assert L.gcow_encode_residual_path(C.byref(_field(n, dtype=4)), C.byref(p), E, E, None) == -1
    assert L.gcow_encode_residual_path(C.byref(f), None, E, E, None) == -1
    assert L.gcow_encode_residual_path(None, C.byref(_sets()[0][0]), E, E, None) == -1


@pytest.mark.parametrize("dtype", DTYPES, ids=["fp32", "bf16"])
@pytest.mark.parametrize("n", SIZES)
def test_workspace(n, dtype):
    """The fused variable-rate path needs the encoder's workspace for the fp32 field and nothing else: no y (4 n bytes),
    no private index."""
    from gcow_amd import _ffi, codec
    L = _ffi.load()
    yf = _field(n, dtype=3, data=0)
    for data in (X, 0):
        f = _field(n, dtype=dtype, data=data)
        for p, want in _sets():
            ws = L.gcow_encode_residual_workspace_bytes(C.byref(f), C.byref(p))
            enc = L.gcow_encode_workspace_bytes(C.byref(yf), C.byref(p))
            if want == FUSED_VAR:
                assert ws == enc and 0 < ws < 4 * n, p.tuple()
            elif want == FUSED_FIXED:
                assert ws == 0
            else:
                assert ws >= 4 * n + enc
    # off 16-byte alignment the function answers for the composed path
    f = _field(n, dtype=dtype, data=X + 4)
    assert L.gcow_encode_residual_workspace_bytes(C.byref(f), C.byref(codec.accuracy(1e-3))) >= 4 * n
    # the assertion of test_gpu_residual.test_argument_checks
    f64 = _field(64)
    assert L.gcow_encode_residual_workspace_bytes(C.byref(f64), C.byref(codec.accuracy(1e-3))) >= 64 * 4 + 8
    assert L.gcow_encode_residual_workspace_bytes(C.byref(f64), C.byref(codec.rate(16, 1))) == 0


def test_residual_encoder_path_attribute_is_declared():
    from gcow_amd import codec
    assert (codec.RESID_COMPOSED, codec.RESID_FUSED_FIXED, codec.RESID_FUSED_VAR) == (COMPOSED, FUSED_FIXED, FUSED_VAR)


def _tile_totals(orc, y, op):
    from residual_var_inputs import TILE
    bits = orc.block_bits(np.ascontiguousarray(y), op).astype(np.int64)
    nb = TILE // 4
    nfull = bits.size // nb
    return bits[:nfull * nb].reshape(nfull, nb).sum(axis=1), int(bits[nfull * nb:].sum())


@pytest.mark.parametrize("bf16", [False, True], ids=["fp32", "bf16"])
def test_inputs_reach_both_code_kernels(orc, bf16):
    """A tile whose code, placed at the worst bit offset below a 16-byte stream boundary (127), needs more than the
    window's 1500 qwords goes to the _big kernel: total > 1500 * 64 bits is certainly one, total < 1497 * 64 - 127
    certainly not (the window keeps two qwords past the last bit)."""
    from residual_var_inputs import WINDOW_BITS, case
    lo = 1497 * 64 - 127
    c = case(65559, bf16, "acc1e-3")
    tot, _ = _tile_totals(orc, c["steps"][0][3], c["op"])
    assert np.any(tot > WINDOW_BITS) and np.any(tot < lo), tot
    assert np.all(tot[1::2] > WINDOW_BITS) and np.all(tot[0::2] < lo), tot  # the odd tiles are the scaled ones
    c = case(65559, bf16, "prec32")
    tot, _ = _tile_totals(orc, c["steps"][0][3], c["op"])
    assert np.all(tot > WINDOW_BITS), tot
    c = case(65559, bf16, "prec12")
    tot, _ = _tile_totals(orc, c["steps"][0][3], c["op"])
    assert not np.any(tot > WINDOW_BITS), tot


@pytest.mark.parametrize("bf16", [False, True], ids=["fp32", "bf16"])
def test_inputs_hold_special_blocks(orc, bf16):
    from residual_var_inputs import case
    c = case(65559, bf16, "acc1e-3")
    _, _, _, y, d = c["steps"][0]
    yb = y[:y.size // 4 * 4].reshape(-1, 4)
    assert np.any(~np.isfinite(yb).all(axis=1))                 # an Inf / NaN block
    assert np.any(np.isnan(y)) and np.any(np.isposinf(y)) and np.any(np.isneginf(y))
    # a value that decodes to -0: where the subnormal block has precision left (at accuracy 1e-3 it is one '0' bit)
    for mode in ("prec12", "prec32"):
        d = case(65559, bf16, mode)["steps"][0][4]
        assert np.any((d == 0) & np.signbit(d)), mode
