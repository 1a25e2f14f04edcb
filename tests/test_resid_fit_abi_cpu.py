"""gcow_rate_table_residual_device and gcow_encode_residual_fitted_device (include/gcow.h) as far as they can be checked
without a GPU: the symbols, their declarations, and the argument checks that are decided before any device call (the
pointers below are never dereferenced: every call returns ahead of its first launch)."""
import ctypes as C

INVALID, CAPACITY, UNSUPPORTED = 1, 2, 5
NEW = {"gcow_rate_table_residual_device": 7, "gcow_encode_residual_fitted_device": 13}


def _field(dtype, data, nx, ny=0, sx=0):
    from gcow_amd._ffi import ZfpInput
    f = ZfpInput()
    f.dtype, f.data, f.nx, f.ny, f.sx = dtype, data, nx, ny, sx
    return f


def test_symbols_exported_and_declared():
    from gcow_amd import _ffi
    L = _ffi.load()
    declared = _ffi.header_functions()
    for name, nargs in NEW.items():
        assert hasattr(L, name), name
        assert name in declared, name
        assert len(getattr(L, name).argtypes) == nargs, name


def test_python_entry_points():
    from gcow_amd import codec, dist
    for name in ("rate_table_residual", "encode_residual_fitted_device", "FittedResidualEncoder"):
        assert hasattr(codec, name), name
    for name in ("rate_table_residual", "encode_residual_fitted"):
        assert hasattr(dist.DeviceCodec, name), name


def test_rate_table_residual_argument_checks():
    from gcow_amd import _ffi
    L = _ffi.load()
    X, E, T, W = 0x10000, 0x20000, 0x30000, 0x40000  # fake device addresses
    f = _field(_ffi.DTYPE_FLOAT, X, 64)
    wsb = L.gcow_rate_table_workspace_bytes(C.byref(f))
    call = L.gcow_rate_table_residual_device
    assert call(None, E, 64, T, W, wsb, None) == INVALID
    assert call(C.byref(_field(_ffi.DTYPE_FLOAT, X, 8, ny=8)), E, 64, T, W, wsb, None) == INVALID   # 2-D
    assert call(C.byref(_field(_ffi.DTYPE_FLOAT, X, 32, sx=2)), E, 64, T, W, wsb, None) == INVALID  # strided
    assert call(C.byref(_field(_ffi.DTYPE_INT32, X, 64)), E, 64, T, W, wsb, None) == UNSUPPORTED
    assert call(C.byref(f), E, 64, None, W, wsb, None) == INVALID
    assert call(C.byref(f), E, 64, T + 4, W, wsb, None) == INVALID
    assert call(C.byref(f), E, 64, T, None, wsb, None) == INVALID
    assert call(C.byref(f), E, 64, T, W, wsb - 8, None) == INVALID
    assert call(C.byref(_field(_ffi.DTYPE_FLOAT, None, 64)), E, 64, T, W, wsb, None) == INVALID
    assert call(C.byref(_field(_ffi.DTYPE_FLOAT, X + 2, 64)), E, 64, T, W, wsb, None) == INVALID
    assert call(C.byref(f), E + 2, 64, T, W, wsb, None) == INVALID                                  # e off 4 bytes
    assert "error buffer" in L.gcow_last_error().decode()


def test_encode_residual_fitted_argument_checks():
    from gcow_amd import _ffi, codec
    L = _ffi.load()
    X, EI, EO, M, OUT, BITS, WS = 0x10000, 0x20000, 0x30000, 0x40000, 0x50000, 0x60000, 0x70000
    hp = codec.fitted_params(64, 0)
    yf = _field(_ffi.DTYPE_FLOAT, None, 64)
    cap = L.gcow_max_output_bytes(C.byref(yf), C.byref(hp))
    wsb = L.gcow_encode_workspace_bytes(C.byref(yf), C.byref(hp))
    for me in (-154, 133):  # neither query depends on minexp
        q = codec.fitted_params(64, me)
        assert L.gcow_max_output_bytes(C.byref(yf), C.byref(q)) == cap
        assert L.gcow_encode_workspace_bytes(C.byref(yf), C.byref(q)) == wsb

    def call(f=None, m=M, ei=EI, eo=EO, out=OUT, c=cap, ws=WS, wb=wsb, index=None, stride=0):
        f = f if f is not None else _field(_ffi.DTYPE_FLOAT, X, 64)
        return L.gcow_encode_residual_fitted_device(C.byref(f), 64, m, ei, eo, out, c, BITS, ws, wb, index, stride,
                                                    None)

    assert call(_field(_ffi.DTYPE_FLOAT, X, 8, ny=8)) == UNSUPPORTED
    assert call(_field(_ffi.DTYPE_FLOAT, X, 32, sx=2)) == UNSUPPORTED
    assert call(_field(_ffi.DTYPE_INT32, X, 64)) == UNSUPPORTED
    assert call(m=None) == INVALID
    assert call(m=M + 2) == INVALID
    assert call(eo=None) == INVALID
    assert "d_err_out" in L.gcow_last_error().decode()
    assert call(out=None) == INVALID
    assert call(index=0x80000, stride=3) == INVALID
    assert call(_field(_ffi.DTYPE_FLOAT, None, 64)) == INVALID
    # no composed fallback: anything off 16 bytes is refused, for fp32 and bf16 x
    assert call(_field(_ffi.DTYPE_FLOAT, X + 4, 64)) == UNSUPPORTED
    assert call(_field(_ffi.DTYPE_BF16, X + 8, 64)) == UNSUPPORTED
    assert call(ei=EI + 4) == UNSUPPORTED
    assert call(eo=EO + 8) == UNSUPPORTED
    assert call(c=cap - 8) == CAPACITY
    assert call(wb=wsb - 8) == INVALID
    assert call(ws=None) == INVALID
