"""GPU parity of error feedback at variable rate (gcow_encode_residual_device's GCOW_RESID_FUSED_VAR path: the tile
encoder on y = x + e, whose code pass writes the residual from its own coefficients) against the reference model
(tests/residual_model.py: numpy over the oracle). Every comparison is bitwise: the stream and its bit count, the new
error, e_in = NULL, in place, the caller's block index, chained steps, the bytes after every output and after the
workspace, the composed path beside it, and the sharded wire hook over a one-rank RCCL group.

Sizes in values: 1, 3, 4, 5 (partial and whole single blocks); one tile of 4096 values -1, +0, +1; the count kernel's
group of 8 tiles (32768 values: its pipelined path runs only with a whole group inside the field) -1, +0, +1; and
65559 = two groups, 5 blocks and 3 values. From three tiles on, every odd tile of x is scaled by 2^20 and goes to the
oversized-tile kernel at accuracy 1e-3 / 1e-6 (residual_var_inputs.py; test_residual_var_cpu.py checks that)."""
import ctypes as C

import numpy as np
import pytest

torch = pytest.importorskip("torch")

pytestmark = pytest.mark.gpu

SIZES = [1, 3, 4, 5, 4095, 4096, 4097, 32767, 32768, 32769, 65559]
MODES = ["acc1e-3", "acc1e-6", "prec12", "prec32", "expert_nobudget"]
SENT_F = 1234.5
SENT_W = 0x5A5A5A5A5A5A5A5A
COMPOSED, FUSED_VAR = 0, 2


@pytest.fixture(scope="module")
def gc():
    if not torch.cuda.is_available():
        pytest.fail("GPU tests need a device")
    from gcow_amd import codec
    return codec


def _dev(a):
    t = torch.from_numpy(np.array(a)).cuda()  # a writable copy: the cases' arrays are shared and read-only
    return t.view(torch.bfloat16) if a.dtype == np.uint16 else t


def _bits_eq(t, ref):
    return np.array_equal(t.cpu().numpy().view(np.uint32), ref.view(np.uint32))


def _call(gc, x, e_in, e_out, p, nwords, want_path, index_stride=0):
    """gcow_encode_residual_device through the C ABI into sentinel-filled buffers, the workspace exactly the size the
    library asks for with 8 sentinel words behind it: -> (status, stream words, bits, the 4 words after the stream,
    index). Asserts the path the library says it takes and that the workspace's sentinels are intact."""
    from gcow_amd._ffi import load
    L = load()
    f = gc.field_of(x)
    cap = L.gcow_max_output_bytes(C.byref(f), C.byref(p))
    words = torch.full((max((cap + 7) // 8, nwords + 4),), SENT_W, dtype=torch.int64, device="cuda")
    bits = torch.full((1,), -1, dtype=torch.int64, device="cuda")
    ne = L.gcow_index_entries(C.byref(f), index_stride) if index_stride else 0
    index = torch.full((max(ne, 1) + 2,), SENT_W, dtype=torch.int64, device="cuda") if index_stride else None
    ptr = lambda t: t.data_ptr() if t is not None else None  # noqa: E731
    path = L.gcow_encode_residual_path(C.byref(f), C.byref(p), ptr(e_in), ptr(e_out), ptr(index))
    assert path == want_path
    fq = gc.field_of(x)
    if want_path == COMPOSED:  # the composed path's size: what the function answers for a bucket off alignment
        fq.data = fq.data + 4
    wsb = L.gcow_encode_residual_workspace_bytes(C.byref(fq), C.byref(p))
    assert wsb % 8 == 0
    if want_path == FUSED_VAR:  # no y: the composed path, which parks y in the workspace, cannot have run in this
        assert wsb < 4 * x.numel() or x.numel() < 4096
        yf = gc.field_of_shape((x.numel(),), torch.float32)
        assert wsb == L.gcow_encode_workspace_bytes(C.byref(yf), C.byref(p))
    ws = torch.full((wsb // 8 + 8,), SENT_W, dtype=torch.int64, device="cuda")
    st = L.gcow_encode_residual_device(C.byref(f), C.byref(p), ptr(e_in), ptr(e_out), words.data_ptr(),
                                       words.numel() * 8, bits.data_ptr(), ws.data_ptr(), wsb, ptr(index), index_stride,
                                       torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    assert torch.all(ws[wsb // 8:] == SENT_W)
    if index is not None:
        assert torch.all(index[ne:] == SENT_W)
        index = index[:ne]
    return st, words[:nwords].cpu().numpy().view(np.uint64), int(bits.item()), words[nwords:nwords + 4].cpu().numpy(), \
        index


def _check_three_ways(gc, c, n, p, want_path, offset=0):
    """Out of place, in place and e_in = NULL against the model; offset: the e buffers start that many floats into a
    16-byte aligned allocation."""
    x = _dev(c["xs"][0])
    w_ref, bits_ref, e_ref = c["steps"][0][:3]

    def ebuf(init):
        buf = torch.full((offset + n + 16,), SENT_F, dtype=torch.float32, device="cuda")
        if init is not None:
            buf[offset:offset + n] = _dev(init)
        return buf, buf[offset:offset + n]

    def intact(buf, after):
        return bool(torch.all(buf[:offset] == SENT_F) and torch.all(buf[offset + n:] == SENT_F)
                    and np.all(after.view(np.uint64) == SENT_W))

    # out of place, 16 sentinel floats after e_out[n - 1] and 4 sentinel words after the stream
    _, e_in = ebuf(c["e0"])
    buf, e_out = ebuf(None)
    st, w, bits, after, _ = _call(gc, x, e_in, e_out, p, w_ref.size, want_path)
    assert st == 0
    assert bits == bits_ref and w.tobytes() == w_ref.tobytes()
    assert _bits_eq(e_out, e_ref)
    assert intact(buf, after)
    assert _bits_eq(e_in, c["e0"])  # the input error is only read
    # in place: the same result
    buf2, e2 = ebuf(c["e0"])
    st, w, bits, after, _ = _call(gc, x, e2, e2, p, w_ref.size, want_path)
    assert st == 0 and bits == bits_ref and w.tobytes() == w_ref.tobytes()
    assert _bits_eq(e2, e_ref)
    assert intact(buf2, after)
    # e_in = NULL is e_in = zeros
    wn_ref, bitsn_ref, en_ref = c["null"]
    buf3, e3 = ebuf(None)
    st, w, bits, after, _ = _call(gc, x, None, e3, p, wn_ref.size, want_path)
    assert st == 0 and bits == bitsn_ref and w.tobytes() == wn_ref.tobytes()
    assert _bits_eq(e3, en_ref)
    assert intact(buf3, after)


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("bf16", [False, True], ids=["fp32", "bf16"])
@pytest.mark.parametrize("n", SIZES)
def test_fused_var_matches_model(gc, orc, n, bf16, mode):
    from residual_var_inputs import case
    c = case(n, bf16, mode)
    _check_three_ways(gc, c, n, gc.expert(*c["op"].tuple()), FUSED_VAR)


@pytest.mark.parametrize("stride", [1, 16, 256])
@pytest.mark.parametrize("mode", ["acc1e-3", "prec32"])
@pytest.mark.parametrize("bf16", [False, True], ids=["fp32", "bf16"])
@pytest.mark.parametrize("n", [4097, 65559])
def test_caller_index(gc, orc, n, bf16, mode, stride):
    """With d_index the path is still the fused one; the index is the one codec.encode writes for the model's y
    uploaded as fp32, and the decoder finds every chunk through it."""
    from residual_var_inputs import case
    c = case(n, bf16, mode)
    p = gc.expert(*c["op"].tuple())
    w_ref, bits_ref, e_ref, y, d = c["steps"][0]
    e = _dev(c["e0"])
    st, w, bits, after, index = _call(gc, _dev(c["xs"][0]), e, e, p, w_ref.size, FUSED_VAR, index_stride=stride)
    assert st == 0 and bits == bits_ref and w.tobytes() == w_ref.tobytes()
    assert _bits_eq(e, e_ref) and np.all(after.view(np.uint64) == SENT_W)
    plain = gc.encode(_dev(y), p, index_stride=stride)
    torch.cuda.synchronize()
    assert plain.to_bytes() == w_ref.tobytes()
    assert torch.equal(index, plain.index[:index.numel()])
    words = torch.from_numpy(w.view(np.int64).copy()).cuda()
    got = gc.decode(words, (n,), p, index=index, index_stride=stride).cpu().numpy()
    assert np.array_equal(got.view(np.uint32), d.view(np.uint32))


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("bf16", [False, True], ids=["fp32", "bf16"])
@pytest.mark.parametrize("n", [5, 32769, 65559])
def test_three_chained_steps(gc, orc, n, bf16, mode):
    """codec.ResidualEncoder three times on one err tensor, on the fused path."""
    from residual_var_inputs import case
    c = case(n, bf16, mode)
    p = gc.expert(*c["op"].tuple())
    err = _dev(c["e0"]).clone()
    enc = gc.ResidualEncoder(n, torch.bfloat16 if bf16 else torch.float32, p, "cuda", 16)
    assert enc.path == gc.RESID_FUSED_VAR == FUSED_VAR
    assert enc.ws_bytes < 4 * n or n < 4096
    for x, (w_ref, bits_ref, e_ref, _, _) in zip(c["xs"], c["steps"]):
        e = enc(_dev(x), err)
        torch.cuda.synchronize()
        assert e.bits == bits_ref and e.to_bytes() == w_ref.tobytes()
        assert _bits_eq(err, e_ref)
    d = gc.decode(e).cpu().numpy()  # through the index of the last step
    assert np.array_equal(d.view(np.uint32), c["steps"][2][4].view(np.uint32))
    assert gc.ResidualEncoder(n, torch.float32, gc.rate(16, 1), "cuda").path == gc.RESID_FUSED_FIXED
    assert gc.ResidualEncoder(n, torch.float32, gc.rate(12, 1), "cuda").path == gc.RESID_COMPOSED


@pytest.mark.parametrize("bf16", [False, True], ids=["fp32", "bf16"])
@pytest.mark.parametrize("n", [4097, 32769])
def test_composed_path_is_alive(gc, orc, n, bf16):
    """An e view one float into its allocation, and a budgeted variable-rate set, take the composed path and still
    match the model."""
    from residual_var_inputs import case
    c = case(n, bf16, "acc1e-3")
    _check_three_ways(gc, c, n, gc.expert(*c["op"].tuple()), COMPOSED, offset=1)
    c = case(n, bf16, "expert_budget")
    _check_three_ways(gc, c, n, gc.expert(*c["op"].tuple()), COMPOSED)


# ---------------------------------------------------------------------------------------------- wire hook, RCCL
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


def test_sharded_hook_bf16_acc1e6_world1(gc, orc, nccl_world1):
    """compressed_sharded_hook with error feedback, bf16 buckets of 65559 and 4097 values (the first with the scaled
    tiles) at accuracy 1e-6, two steps over one rank: every bucket comes back as the model's decode rounded to bf16,
    and the state holds the model's error."""
    from gcow_amd import ddp
    from residual_model import model_step
    from residual_var_inputs import case
    c = [case(65559, True, "acc1e-6"), case(4097, True, "acc1e-6")]
    p = gc.expert(*c[0]["op"].tuple())
    fn = ddp.compressed_sharded_hook
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
            got = out.float().cpu().numpy()
            ref = torch.from_numpy(want).to(torch.bfloat16).float().numpy()
            assert np.array_equal(got.view(np.uint32), ref.view(np.uint32)), (step, i)
            assert _bits_eq(state.error_buffer(i, t), errs[i]), (step, i)
    assert any(np.any(e) for e in errs)
