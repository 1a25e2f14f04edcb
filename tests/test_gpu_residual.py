"""GPU parity of error feedback (gcow_encode_residual_device, include/gcow.h) against the reference model
(tests/residual_model.py: numpy over the oracle), bitwise: the stream and its bit count, the new error, e_in = NULL,
in place, chained steps, the bytes after both outputs, argument checks, and the wire hooks over a one-rank RCCL group.

Sizes: one value, partial and whole single blocks, and the fused kernel's workgroup chunk (256 lanes x 8 blocks = 8192
values) - 1, + 0, + 1, and three chunks plus a partial block. rate 16 / 8 run the fused kernel, rate 12 and
expert(64, 64, 20, -1074) the composed path at fixed rate, accuracy / precision the composed path at variable rate."""
import ctypes as C
import functools

import numpy as np
import pytest

torch = pytest.importorskip("torch")

pytestmark = pytest.mark.gpu

SIZES = [1, 3, 4, 5, 8191, 8192, 8193, 24583]
MODES = ["rate16", "rate8", "rate12", "expert64_prec20", "acc1e-3", "prec12"]
SENT_F = 1234.5
SENT_W = 0x5A5A5A5A5A5A5A5A


@pytest.fixture(scope="module")
def gc():
    if not torch.cuda.is_available():
        pytest.fail("GPU tests need a device")
    from gcow_amd import codec
    return codec


def _op(orc, mode):
    return {"rate16": orc.rate(16, 1), "rate8": orc.rate(8, 1), "rate12": orc.rate(12, 1),
            "expert64_prec20": orc.expert(64, 64, 20, -1074), "acc1e-3": orc.accuracy(1e-3),
            "prec12": orc.precision(12)}[mode]


def _bf16(a):
    return (a.view(np.uint32) >> 16).astype(np.uint16)


def _inputs(n, bf16, op):
    """The bucket x (float32, or bf16 bits) and the carried error e: a gradient-like bucket with a residual-scale e,
    and crafted blocks spliced in (from block 1 on; from block 0, cut to n, when the bucket is a few values)."""
    from oracle import oracle as O
    from residual_model import model_step, widen
    x = O.gen_normal(n, 1e-3, 501, True).copy()
    e = model_step(O.gen_normal(n, 1e-3, 777, True), None, op)[4].copy()
    rng = np.random.default_rng(7)
    blocks = [
        ([1e-40, 2e-40, -3e-41, 0.0], [0.0] * 4),             # decodes to -0: a subnormal residual
        ([np.nan, 1e-3, -2e-3, 3e-3], None),                  # NaN gradient
        ([np.inf, -np.inf, 1e-3, 0.0], None),                 # +-Inf gradient
        ([3e38] * 4, [3e38] * 4),                             # x + e overflows
        ([1e-3, -2.5e-3, 3.25e-4, 7e-3], "neg"),              # x = -e exactly
    ]
    nbw = max(0, min(512, (n // 4 - 16) // 8))
    if nbw:
        sign = np.where(rng.random((nbw, 4)) < 0.5, -1.0, 1.0)
        wide = sign * 2.0 ** rng.uniform(-60, 10, (nbw, 4))   # test_gpu_parity._adversarial_1d: long group phases
        wide2 = rng.standard_normal((nbw, 4)) * 2.0 ** rng.integers(-40, 40, (nbw, 4))  # test_dec_pair_fastpath._blocks
        pow2 = 2.0 ** rng.integers(-60, 30, (nbw, 4)) * np.where(rng.random((nbw, 4)) < 0.5, -1.0, 1.0)
        sparse = np.zeros((nbw, 4))
        hit = rng.random((nbw, 4)) < 0.2
        sparse[hit] = rng.standard_normal(int(hit.sum()))
        # one or two coefficients significant over many planes: group phases past the decoders' 16-plane window and
        # plane codes that cross the budget (their special lanes; e = 0 keeps the blocks as built)
        const = np.repeat(rng.standard_normal((nbw, 1)), 4, axis=1)
        alt = np.repeat(rng.standard_normal((nbw, 1)), 4, axis=1) * np.array([1, -1, 1, -1])
        ramp = np.cumsum(rng.standard_normal((nbw, 4)) * 1e-6, axis=1) + 1.0
        with np.errstate(over="ignore"):
            for b in np.concatenate([wide, wide2, pow2, sparse]).astype(np.float32):
                blocks.append((list(b), None))
            for b in np.concatenate([const, alt, ramp]).astype(np.float32):
                blocks.append((list(b), [0.0] * 4))
    neg = []
    at = 4 if n >= 64 else 0
    for xb, eb in blocks:
        m = min(4, n - at)
        if m <= 0:
            break
        x[at:at + m] = np.array(xb, np.float32)[:m]
        if eb == "neg":
            neg.append((at, m))
        elif eb is not None:
            e[at:at + m] = np.array(eb, np.float32)[:m]
        at += 4
    if bf16:
        x = _bf16(x)
    for at, m in neg:
        e[at:at + m] = -widen(x)[at:at + m]
    return x, e


@functools.lru_cache(maxsize=None)
def _case(n, bf16, mode):
    """Inputs and the model's three chained steps, computed once per case and shared (never modified)."""
    from oracle import oracle as O
    from residual_model import model_step
    op = _op(O, mode)
    x0, e0 = _inputs(n, bf16, op)
    xs = [x0]
    for t in (1, 2):
        a = O.gen_normal(n, 1e-3, 600 + t, True)
        xs.append(_bf16(a) if bf16 else a)
    steps = []
    e = e0
    for x in xs:
        _, w, bits, _, e = model_step(x, e, op)
        steps.append((w, bits, e))
    null = model_step(x0, None, op)
    for a in xs + [e0] + [s[2] for s in steps]:
        a.setflags(write=False)
    return {"op": op, "xs": xs, "e0": e0, "steps": steps, "null": (null[1], null[2], null[4])}


def _dev(a):
    t = torch.from_numpy(np.array(a)).cuda()  # a writable copy: the cases' arrays are shared and read-only
    return t.view(torch.bfloat16) if a.dtype == np.uint16 else t


def _bits_eq(t, ref):
    return np.array_equal(t.cpu().numpy().view(np.uint32), ref.view(np.uint32))


def _call(gc, x, e_in, e_out, p, nwords, index_stride=0):
    """gcow_encode_residual_device through the C ABI into sentinel-filled buffers: -> (status, stream words, bits,
    the 4 words after the stream)."""
    from gcow_amd._ffi import load
    L = load()
    f = gc.field_of(x)
    cap = L.gcow_max_output_bytes(C.byref(f), C.byref(p))
    words = torch.full((max((cap + 7) // 8, nwords + 4),), SENT_W, dtype=torch.int64, device="cuda")
    bits = torch.full((1,), -1, dtype=torch.int64, device="cuda")
    wsb = L.gcow_encode_residual_workspace_bytes(C.byref(f), C.byref(p))
    ws = torch.empty(max(wsb // 8, 1), dtype=torch.int64, device="cuda")
    ne = L.gcow_index_entries(C.byref(f), index_stride) if index_stride else 0
    index = torch.empty(max(ne, 1), dtype=torch.int64, device="cuda") if index_stride else None
    st = L.gcow_encode_residual_device(C.byref(f), C.byref(p), e_in.data_ptr() if e_in is not None else None,
                                       e_out.data_ptr() if e_out is not None else None, words.data_ptr(),
                                       words.numel() * 8, bits.data_ptr(), ws.data_ptr(), wsb,
                                       index.data_ptr() if index is not None else None, index_stride,
                                       torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    return st, words[:nwords].cpu().numpy().view(np.uint64), int(bits.item()), words[nwords:nwords + 4].cpu().numpy()


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("bf16", [False, True], ids=["fp32", "bf16"])
@pytest.mark.parametrize("n", SIZES)
def test_encode_residual_matches_model(gc, orc, n, bf16, mode):
    c = _case(n, bf16, mode)
    p = gc.expert(*c["op"].tuple())
    x = _dev(c["xs"][0])
    w_ref, bits_ref, e_ref = c["steps"][0]
    # out of place, 16 sentinel floats after e_out[n - 1] and 4 sentinel words after the stream
    e_in = _dev(c["e0"])
    buf = torch.full((n + 16,), SENT_F, dtype=torch.float32, device="cuda")
    st, w, bits, after = _call(gc, x, e_in, buf[:n], p, w_ref.size)
    assert st == 0
    assert bits == bits_ref and w.tobytes() == w_ref.tobytes()
    assert _bits_eq(buf[:n], e_ref)
    assert torch.all(buf[n:] == SENT_F) and np.all(after.view(np.uint64) == SENT_W)
    assert _bits_eq(e_in, c["e0"])  # the input error is only read
    # in place: the same result
    buf2 = torch.full((n + 16,), SENT_F, dtype=torch.float32, device="cuda")
    buf2[:n] = _dev(c["e0"])
    st, w, bits, after = _call(gc, x, buf2[:n], buf2[:n], p, w_ref.size)
    assert st == 0 and bits == bits_ref and w.tobytes() == w_ref.tobytes()
    assert _bits_eq(buf2[:n], e_ref)
    assert torch.all(buf2[n:] == SENT_F) and np.all(after.view(np.uint64) == SENT_W)
    # e_in = NULL is e_in = zeros
    wn_ref, bitsn_ref, en_ref = c["null"]
    buf3 = torch.full((n + 16,), SENT_F, dtype=torch.float32, device="cuda")
    st, w, bits, after = _call(gc, x, None, buf3[:n], p, wn_ref.size)
    assert st == 0 and bits == bitsn_ref and w.tobytes() == wn_ref.tobytes()
    assert _bits_eq(buf3[:n], en_ref)
    assert torch.all(buf3[n:] == SENT_F) and np.all(after.view(np.uint64) == SENT_W)


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("bf16", [False, True], ids=["fp32", "bf16"])
@pytest.mark.parametrize("n", [5, 8193, 24583])
def test_three_chained_steps(gc, orc, n, bf16, mode):
    """codec.encode_residual (the preallocated ResidualEncoder behind it) three times on one err tensor."""
    c = _case(n, bf16, mode)
    p = gc.expert(*c["op"].tuple())
    err = _dev(c["e0"]).clone()
    enc = gc.ResidualEncoder(n, torch.bfloat16 if bf16 else torch.float32, p, "cuda",
                             0 if gc.is_fixed(p) else 16)
    for x, (w_ref, bits_ref, e_ref) in zip(c["xs"], c["steps"]):
        e = enc(_dev(x), err)
        torch.cuda.synchronize()
        assert e.bits == bits_ref and e.to_bytes() == w_ref.tobytes()
        assert _bits_eq(err, e_ref)
    # the one-call form, with the caller's block index at variable rate
    err2 = _dev(c["e0"]).clone()
    e = gc.encode_residual(_dev(c["xs"][0]), err2, p, index_stride=0 if gc.is_fixed(p) else 8)
    torch.cuda.synchronize()
    assert e.to_bytes() == c["steps"][0][0].tobytes() and _bits_eq(err2, c["steps"][0][2])
    if not gc.is_fixed(p):  # the index written is the stream's: the decoder finds every chunk through it
        d = gc.decode(e).cpu().numpy()
        ref = orc.decompress(c["steps"][0][0], (n,), c["op"])
        assert np.array_equal(d.view(np.uint32), ref.view(np.uint32))


def test_argument_checks(gc, orc):
    from gcow_amd._ffi import load
    L = load()
    p = gc.rate(16, 1)
    x2 = torch.zeros(8, 8, device="cuda")
    e2 = torch.zeros(64, device="cuda")
    assert _call(gc, x2, e2, e2, p, 1)[0] == 5          # GCOW_ERR_UNSUPPORTED: a 2-D field
    xs = torch.zeros(128, device="cuda")[::2]
    assert _call(gc, xs, e2, e2, p, 1)[0] == 5          # a strided view
    for q in (p, gc.accuracy(1e-3)):
        assert _call(gc, xs, e2, e2, q, 1)[0] == 5
    x = torch.zeros(64, device="cuda")
    assert _call(gc, x, e2, None, p, 1)[0] == 1         # GCOW_ERR_INVALID: NULL d_err_out
    f = gc.field_of(x)
    f.dtype = 4                                         # dtype_double
    st = L.gcow_encode_residual_device(C.byref(f), C.byref(p), None, e2.data_ptr(), e2.data_ptr(), 1 << 20, None, None,
                                       0, None, 0, None)
    assert st == 5
    with pytest.raises(gc.GcowError):
        gc.encode_residual(x, torch.zeros(63, device="cuda"), p)
    with pytest.raises(gc.GcowError):
        gc.encode_residual(x, torch.zeros(64, device="cuda", dtype=torch.bfloat16), p)
    # fused domain: no workspace; composed: y + the encoder's workspace + the index
    assert L.gcow_encode_residual_workspace_bytes(C.byref(gc.field_of(x)), C.byref(p)) == 0
    assert L.gcow_encode_residual_workspace_bytes(C.byref(gc.field_of(x)), C.byref(gc.accuracy(1e-3))) >= 64 * 4 + 8


# ---------------------------------------------------------------------------------------------- wire hooks, RCCL
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


@pytest.mark.parametrize("mode", ["rate16", "acc1e-3"])
@pytest.mark.parametrize("bf16", [False, True], ids=["fp32", "bf16"])
@pytest.mark.parametrize("hook", ["compressed_allgather_hook", "compressed_sharded_hook"])
def test_wire_hooks_error_feedback_world1(gc, orc, nccl_world1, hook, bf16, mode):
    """One rank over RCCL, two buckets, two steps, the device codec: every bucket comes back as (0 + yhat) / 1 of the
    model's decode (a bf16 bucket: rounded to nearest even) and the state holds the model's error."""
    from gcow_amd import ddp
    from residual_model import model_step
    c = [_case(24583, bf16, mode), _case(8193, bf16, mode)]
    p = gc.expert(*c[0]["op"].tuple())
    fn = getattr(ddp, hook)
    state = ddp.make_hook_state(hook=fn, params=p, error_feedback=True)
    errs = [None, None]
    for step in range(2):
        for i in range(2):
            x = c[i]["xs"][step + 1]  # finite gradients
            _, _, _, d, errs[i] = model_step(x, errs[i], c[i]["op"])
            want = (np.zeros_like(d) + d) / np.float32(1)
            t = _dev(x).clone()
            out = fn(state, _Bucket(t, i)).wait()
            torch.cuda.synchronize()
            out = out[0] if isinstance(out, (list, tuple)) else out
            if bf16:
                got = out.float().cpu().numpy()
                ref = torch.from_numpy(want).to(torch.bfloat16).float().numpy()
                assert np.array_equal(got.view(np.uint32), ref.view(np.uint32)), (step, i)
            else:
                assert _bits_eq(out, want), (step, i)
            assert _bits_eq(state.error_buffer(i, t), errs[i]), (step, i)
    assert any(np.any(e) for e in errs)
