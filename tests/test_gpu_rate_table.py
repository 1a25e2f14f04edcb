"""GPU parity of the rate table (gcow_rate_table_device, include/gcow.h) and of what is built on it: all 288 entries
equal the oracle's stream lengths (288 oracle encodes, tests/rate_table_inputs.oracle_table); entries equal the bits
the product's own encode and fused round trip report; fields that put every update on the same bins, or on all of
them; dirty table / workspace buffers and the bytes after the table; codec.encode_fitted against the oracle; argument
checks; a stream capture; and the hooks' target_bits over a one-rank RCCL group.

Sizes: one value, partial and whole single blocks, and C = 4096 values -- what one workgroup covers per iteration of its
loop (codec.RATE_TABLE_TILE_VALUES, csrc/kernels.h kRateTableTileValues) -- minus one, exactly, plus one (a second
workgroup with one block), and three tiles plus a partial block."""
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

TILE = 4096
SIZES = [1, 3, 4, 5, TILE - 1, TILE, TILE + 1, 3 * TILE + 7]
BIG = 3 * TILE + 7
MAXPRECS = [64, 20, 1, 0]
SENT = 0x5A5A5A5A5A5A5A5A


@pytest.fixture(scope="module")
def gc():
    if not torch.cuda.is_available():
        pytest.fail("GPU tests need a device")
    from gcow_amd import codec
    assert codec.RATE_TABLE_TILE_VALUES == TILE
    return codec


def _dev(a):
    t = torch.from_numpy(np.array(a)).cuda()  # a writable copy: the cases' arrays are shared and read-only
    return t.view(torch.bfloat16) if a.dtype == np.uint16 else t


def _table(gc, x, maxprec=64):
    t = gc.rate_table(x, maxprec)
    torch.cuda.synchronize()
    return t.cpu().numpy()


def _diff(got, want):
    bad = np.nonzero(got != want)[0]
    return bad[:6].tolist(), got[bad[:6]].tolist(), np.asarray(want)[bad[:6]].tolist()


@pytest.mark.parametrize("bf16", [False, True], ids=["fp32", "bf16"])
@pytest.mark.parametrize("n", SIZES)
def test_table_matches_oracle(gc, orc, n, bf16):
    import rate_table_inputs as RT
    for maxprec in MAXPRECS:
        x_np, want = RT.crafted_table(n, bf16, maxprec)
        got = _table(gc, _dev(x_np), maxprec)
        assert np.array_equal(got, want), (maxprec,) + _diff(got, want)


@pytest.mark.parametrize("n", [TILE + 1, BIG])
def test_table_matches_encode_and_roundtrip(gc, orc, n):
    import roundtrip_inputs as RI
    x = _dev(RI.inputs(n, False))
    table = _table(gc, x)
    bits = torch.zeros(1, dtype=torch.int64, device="cuda")
    for t in (0, 100, 134, 144, 200, 287):  # 134: accuracy 1e-6, 144: accuracy 1e-3
        p = gc.expert(1, 16658, 64, -154 + t)
        assert gc.encode(x, p).bits == table[t], t
        gc.roundtrip(x, p, bits=bits)
        assert int(bits.item()) == table[t], t
    assert gc.accuracy(1e-6).minexp == -154 + 134 and gc.accuracy(1e-3).minexp == -154 + 144


def test_contention_one_bin(gc, orc):
    """3C + 7 values of 1.0: every block has the same exponent and leading planes, so all updates of a workgroup land
    on the same bins."""
    import rate_table_inputs as RT
    x = np.ones(BIG, np.float32)
    got = _table(gc, _dev(x))
    want = RT.oracle_table(x, 64)
    assert np.array_equal(got, want), _diff(got, want)


def test_contention_all_bins(gc, orc):
    """Block b holds values of biased exponent b mod 255 (0: subnormals) with random mantissas and signs: every bin of
    both arrays is touched."""
    import rate_table_inputs as RT
    rng = np.random.default_rng(77)
    nb = (BIG + 3) // 4
    e = (np.arange(nb, dtype=np.uint32) % 255).repeat(4)[:BIG]
    bits = (e << 23) | rng.integers(0, 1 << 23, BIG, dtype=np.uint32) | (rng.integers(0, 2, BIG, dtype=np.uint32) << 31)
    x = bits.astype(np.uint32).view(np.float32)
    assert np.isfinite(x).all()
    got = _table(gc, _dev(x))
    want = RT.oracle_table(x, 64)
    assert np.array_equal(got, want), _diff(got, want)
    assert np.all(np.diff(got) <= 0) and got[287] == nb


def _call(gc, field, maxprec, table_ptr, ws_ptr, ws_bytes):
    return gc.load().gcow_rate_table_device(C.byref(field), maxprec, table_ptr, ws_ptr, ws_bytes,
                                            torch.cuda.current_stream().cuda_stream)


@pytest.mark.parametrize("n", [5, BIG])
def test_dirty_buffers(gc, orc, n):
    import rate_table_inputs as RT
    x_np, want = RT.crafted_table(n, False, 64)
    x = _dev(x_np)
    f = gc.field_of(x)
    ws_bytes = gc.load().gcow_rate_table_workspace_bytes(C.byref(f))
    buf = torch.full((288 + 8,), SENT, dtype=torch.int64, device="cuda")  # the table and 64 bytes past it
    ws = torch.full((ws_bytes // 8,), SENT, dtype=torch.int64, device="cuda")
    for _ in range(2):  # the second call finds the first one's workspace and table
        assert _call(gc, f, 64, buf.data_ptr(), ws.data_ptr(), ws_bytes) == 0
        torch.cuda.synchronize()
        got = buf.cpu().numpy()
        assert np.array_equal(got[:288], want), _diff(got[:288], want)
        assert np.all(got[288:] == SENT)


@pytest.mark.parametrize("bpv", [2, 4, 8, 16])
def test_encode_fitted(gc, orc, bpv):
    import rate_table_inputs as RT
    from oracle import oracle as O
    x_np, _ = RT.crafted_table(BIG, False, 64)
    budget = bpv * BIG
    enc, p = gc.encode_fitted(_dev(x_np), bpv)
    torch.cuda.synchronize()
    assert p.tuple()[:3] == (1, 16658, 64) and p == gc.fit_accuracy(_dev(x_np), bpv)
    assert enc.bits <= budget
    assert p.minexp == -154 or RT.oracle_bits(x_np, 64, p.minexp - 1) > budget  # the finest tolerance that fits
    op = O.expert(*p.tuple())
    w_ref, bits_ref = O.compress(x_np, op)
    assert enc.bits == bits_ref and enc.to_bytes() == w_ref.tobytes()
    d = gc.decode(enc).cpu().numpy()
    assert np.array_equal(d.view(np.uint32), O.decompress(w_ref, x_np.shape, op).view(np.uint32))


def test_empty_field(gc):
    t = _table(gc, torch.empty(0, dtype=torch.float32, device="cuda"))
    assert t.shape == (288,) and not t.any()


def test_argument_checks(gc):
    from gcow_amd import _ffi
    x = torch.zeros(64, dtype=torch.float32, device="cuda")
    table = torch.full((288,), SENT, dtype=torch.int64, device="cuda")
    ws_bytes = gc.load().gcow_rate_table_workspace_bytes(C.byref(gc.field_of(x)))
    ws = torch.zeros(ws_bytes // 8, dtype=torch.int64, device="cuda")

    def field(**kw):
        f = gc.field_of(x)
        for k, v in kw.items():
            setattr(f, k, v)
        return f

    cases = [(field(nx=8, ny=8), ws_bytes, 1),                    # 2-D
             (field(nx=32, sx=2), ws_bytes, 1),                   # a strided view
             (field(), ws_bytes - 8, 1),                          # a short workspace
             (field(dtype=_ffi.DTYPE_INT32), ws_bytes, 5)]        # an int32 tensor
    for f, wb, want in cases:
        assert _call(gc, f, 64, table.data_ptr(), ws.data_ptr(), wb) == want
    torch.cuda.synchronize()
    assert bool((table == SENT).all())
    with pytest.raises(gc.GcowError):
        gc.rate_table(torch.zeros(8, 8, device="cuda"))
    with pytest.raises(gc.GcowError):
        gc.rate_table(torch.zeros(64, device="cuda")[::2])
    with pytest.raises(gc.GcowError):
        gc.rate_table(torch.zeros(64, dtype=torch.int32, device="cuda"))
    with pytest.raises(gc.GcowError):
        gc.encode_fitted(torch.ones(64, device="cuda"), 0.2)  # below one bit per block


def test_stream_capture(gc, orc):
    """The call is a memset node and two kernels: captured once, replayed on new data."""
    import rate_table_inputs as RT
    a, want_a = RT.crafted_table(TILE + 1, False, 64)
    b = np.ones(TILE + 1, np.float32)
    rt = gc.RateTable(TILE + 1, torch.float32, "cuda")
    x = _dev(a)
    rt(x)  # the kernels are loaded before the capture
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        rt(x)
    x.copy_(torch.from_numpy(b))
    g.replay()
    torch.cuda.synchronize()
    assert np.array_equal(rt.table.cpu().numpy(), RT.oracle_table(b, 64))
    x.copy_(torch.from_numpy(np.array(a)))
    g.replay()
    torch.cuda.synchronize()
    assert np.array_equal(rt.table.cpu().numpy(), want_a)


# ---------------------------------------------------------------------------------------------- hooks, RCCL world 1
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


def test_roundtrip_hook_target_world1(gc, orc, nccl_world1):
    import roundtrip_inputs as RI
    from gcow_amd import ddp
    x = _dev(RI.inputs(BIG, False))
    state = ddp.make_hook_state(hook=ddp.roundtrip_hook, params=gc.accuracy(1e-3), target_bits=4)
    t = x.clone()
    ddp.roundtrip_hook(state, _Bucket(t, 0)).wait()
    torch.cuda.synchronize()
    p = gc.fit_accuracy(x, 4)
    want = gc.roundtrip(x, p)
    torch.cuda.synchronize()
    assert np.array_equal(t.cpu().numpy().view(np.uint32), want.cpu().numpy().view(np.uint32))
    assert gc.encode(x, p).bits <= 4 * BIG


def test_allgather_hook_target_world1(gc, orc, nccl_world1):
    import roundtrip_inputs as RI
    from gcow_amd import ddp
    x = _dev(RI.inputs(BIG, False))
    p0 = gc.accuracy(1e-6)
    state = ddp.make_hook_state(hook=ddp.compressed_allgather_hook, params=p0, target_bits=4)
    assert state.step_params(0, BIG) == p0
    t = x.clone()
    ddp.compressed_allgather_hook(state, _Bucket(t, 0)).wait()
    torch.cuda.synchronize()
    # step 1 ran under state.params; the mean of one stream is 0 + decode, so a -0 of the decode arrives as +0
    want = gc.roundtrip(x, p0) + 0.0
    assert np.array_equal(t.cpu().numpy().view(np.uint32), want.cpu().numpy().view(np.uint32))
    p1 = state.step_params(0, BIG)  # step 2's set: the fit of step 1's table
    assert p1 == gc.fit_accuracy(x, 4) and p1 != p0
    t = x.clone()
    ddp.compressed_allgather_hook(state, _Bucket(t, 0)).wait()
    torch.cuda.synchronize()
    want = gc.roundtrip(x, p1) + 0.0
    assert np.array_equal(t.cpu().numpy().view(np.uint32), want.cpu().numpy().view(np.uint32))
    assert gc.encode(x, p1).bits <= 4 * BIG  # the stream step 2 gathered
