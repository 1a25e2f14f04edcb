"""GPU parity of the round trip over a tensor list (gcow_roundtrip_list_device, codec.roundtrip_tensors /
roundtrip_gradients), bitwise: every tensor receives its slice of the oracle's decompress(compress(cat)) (a bf16 output:
that, rounded to nearest even) and of codec.roundtrip(torch.cat(...)); the bit count is the oracle's.

The tensors are carved out of one sentinel-filled buffer with gaps of at least 3 elements, at 16-byte aligned bases or
at odd element offsets, so that every gap and the 16 elements after the last tensor show a stray write. C = 8192 values
is the plan's chunk. Single tensors of 1, 3, 4, 5, C - 1, C, C + 1 and 3 C + 5 values; the seam list of
tests/roundtrip_list_inputs.py (long tensors at flat offsets 0, 1, 2, 3 mod 4, a seam on a chunk boundary, runs of
one-, two- and three-value tensors across the crafted zero / subnormal / NaN / Inf / 3e38 blocks, empty tensors, totals
of every residue mod 4) with the plan's chunk kinds checked against a brute-force classification; a small model through
roundtrip_gradients; refusals. Modes: rate 16 / 8 (lean fixed rate), accuracy 1e-3 and precision 12 (no budget),
rate 12 and expert(1, 100, 64, -30) (generic)."""
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

CH = 8192
MODE_NAMES = ["rate16", "rate8", "acc1e-3", "prec12", "rate12", "expert_trunc"]
DTYPES = [(False, False), (True, True), (False, True), (True, False)]
DTYPE_IDS = ["fp32-fp32", "bf16-bf16", "fp32-bf16", "bf16-fp32"]
SENT = -1234.5  # exact in bf16 too
TAIL = 16


@pytest.fixture(scope="module")
def gc():
    if not torch.cuda.is_available():
        pytest.fail("GPU tests need a device")
    from gcow_amd import codec
    return codec


def _tdtype(bf16):
    return torch.bfloat16 if bf16 else torch.float32


def _bits_of(t):
    """The tensor's values as raw bits (uint32 for fp32, uint16 for bf16)."""
    if t.dtype == torch.bfloat16:
        return t.view(torch.int16).cpu().numpy().view(np.uint16)
    return t.cpu().numpy().view(np.uint32)


def _want(d, bf16_out):
    from roundtrip_inputs import bf16_rne
    return bf16_rne(d) if bf16_out else d.view(np.uint32)


def _layout(sizes, aligned):
    """Element positions of the tensors in one buffer: gaps of at least 3 elements; aligned: every base a multiple of
    8 elements (16 bytes for bf16, 32 for fp32), else every base at an odd element offset (for bf16: off 4 bytes)."""
    pos, at = [], 8 if aligned else 1
    for n in sizes:
        pos.append(at)
        at += n + 3
        at = (at + 7) // 8 * 8 if aligned else at | 1
    return pos, at + TAIL


def _carve(sizes, bf16, aligned, x_np=None):
    """-> (buffer, tensors, cover mask): the buffer sentinel-filled, the tensors views into it, filled from x_np."""
    pos, total = _layout(sizes, aligned)
    buf = torch.full((total,), SENT, dtype=_tdtype(bf16), device="cuda")
    assert buf.data_ptr() % 16 == 0
    cover = np.zeros(total, bool)
    ts, at = [], 0
    if x_np is not None:
        xt = torch.from_numpy(np.array(x_np)).cuda()  # a writable copy: the cases' arrays are shared and read-only
        xt = xt.view(torch.bfloat16) if bf16 else xt
    for p, n in zip(pos, sizes):
        t = buf[p:p + n]
        if x_np is not None and n:
            t.copy_(xt[at:at + n])
        cover[p:p + n] = True
        ts.append(t)
        at += n
    return buf, ts, cover


def _covered(buf, cover):
    """The tensors' values in list order, as bits (the tensors lie in the buffer in list order)."""
    return _bits_of(buf)[cover]


def _gaps_clean(buf, cover):
    sent = _bits_of(torch.full((1,), SENT, dtype=buf.dtype))[0]
    return bool((_bits_of(buf)[~cover] == sent).all())


def _run_list(gc, sizes, x_np, d_ref, bits_ref, p, bf16_in, bf16_out, aligned):
    """Out of place (always) and in place (equal dtypes) on carved tensors; returns the in-place plan object, or the
    out-of-place one."""
    want = _want(d_ref, bf16_out)
    in_bits = x_np.view(np.uint16 if bf16_in else np.uint32)
    ibuf, ins, icover = _carve(sizes, bf16_in, aligned, x_np)
    obuf, outs, ocover = _carve(sizes, bf16_out, aligned)
    bits = torch.full((1,), -1, dtype=torch.int64, device="cuda")
    plan = gc.TensorListRoundtrip(p)
    got = gc.roundtrip_tensors(ins, p, outs=outs, bits=bits, plan=plan)
    torch.cuda.synchronize()
    assert [g.data_ptr() for g in got] == [o.data_ptr() for o in outs]
    assert np.array_equal(_covered(obuf, ocover), want)
    assert _gaps_clean(obuf, ocover)
    assert np.array_equal(_covered(ibuf, icover), in_bits) and _gaps_clean(ibuf, icover)  # the inputs are only read
    assert int(bits.item()) == bits_ref
    # the contiguous call on the concatenation gives the same bits
    flat = torch.cat([t.reshape(-1) for t in ins]) if ins else torch.zeros(0, dtype=_tdtype(bf16_in), device="cuda")
    if flat.numel():
        ref = gc.roundtrip(flat, p, out=torch.empty(flat.numel(), dtype=_tdtype(bf16_out), device="cuda"))
        torch.cuda.synchronize()
        assert np.array_equal(_bits_of(ref), _covered(obuf, ocover))
    if bf16_in != bf16_out:
        return plan
    plan2 = gc.TensorListRoundtrip(p)
    bits2 = torch.full((1,), -1, dtype=torch.int64, device="cuda")
    gc.roundtrip_tensors(ins, p, bits=bits2, plan=plan2)
    torch.cuda.synchronize()
    assert np.array_equal(_covered(ibuf, icover), want)
    assert _gaps_clean(ibuf, icover) and int(bits2.item()) == bits_ref
    return plan2


@pytest.mark.parametrize("mode", MODE_NAMES)
@pytest.mark.parametrize("bf16_in,bf16_out", DTYPES, ids=DTYPE_IDS)
@pytest.mark.parametrize("n", [1, 3, 4, 5, CH - 1, CH, CH + 1, 3 * CH + 5])
def test_single_tensor(gc, orc, n, bf16_in, bf16_out, mode):
    from roundtrip_inputs import MODES, case
    x_np, d_ref, bits_ref = case(n, bf16_in, mode)
    p = gc.expert(*MODES[mode]().tuple())
    plan = _run_list(gc, [n], x_np, d_ref, bits_ref, p, bf16_in, bf16_out, aligned=True)
    s = plan.stats()
    assert s.direct_chunks + s.gather_chunks == (n + CH - 1) // CH
    if s.domain != 2:  # an aligned tensor: chunks of whole blocks run direct, the one with the partial block gathers
        assert s.gather_chunks == (1 if n % 4 else 0)


@pytest.mark.parametrize("mode", MODE_NAMES)
@pytest.mark.parametrize("bf16_in,bf16_out", DTYPES, ids=DTYPE_IDS)
@pytest.mark.parametrize("aligned", [True, False], ids=["aligned16", "odd-element"])
@pytest.mark.parametrize("r", [0, 1, 2, 3])
def test_seam_list(gc, orc, r, aligned, bf16_in, bf16_out, mode):
    from gcow_amd._ffi import load
    from roundtrip_inputs import MODES
    from roundtrip_list_inputs import classify, plan_chunks, seam_case, seam_sizes
    sizes = seam_sizes(r)
    x_np, d_ref, bits_ref = seam_case(r, bf16_in, mode)
    p = gc.expert(*MODES[mode]().tuple())
    plan = _run_list(gc, sizes, x_np, d_ref, bits_ref, p, bf16_in, bf16_out, aligned)
    # which path ran: the plan against the brute-force classification of the tensors' own addresses
    key = plan._key
    in_ptrs = [a for a, _ in key[3]]
    out_ptrs = list(key[4]) if key[4] is not None else in_ptrs
    s, direct, gather = plan_chunks(load(), plan._h.data_ptr(), plan._used)
    want = classify(in_ptrs, out_ptrs, sizes, 2 if bf16_in else 4, 2 if bf16_out else 4, s.domain, s.row_rule)
    assert direct == [w for w in want if w[0] == "d"] and gather == [w for w in want if w[0] == "g"]
    assert len(gather) >= 6  # the chunks with seams and the last block
    if mode in ("rate12", "expert_trunc"):
        assert s.domain == 2 and not direct
        return
    assert direct and gather  # both kinds of chunk ran
    # the long tensors start at flat offsets 2, 1, 0, 3 (mod 4): their whole chunks are 1, 3, 5, 7
    long_direct = [w for w in want[1:8:2] if w[0] == "d"]
    if s.row_rule == gc.RTLIST_ROWS_DWORD:
        if not (bf16_in or bf16_out):
            assert len(long_direct) == 4 and len(direct) == 5  # fp32 rows always qualify: misaligned tensors run direct
        elif bf16_in and bf16_out and not aligned:
            # odd base + odd flat offset: the rows of the tensors at offsets 1 and 3 (mod 4) are 4-byte aligned
            assert [w[0] for w in want[1:8:2]] == ["g", "d", "g", "d"]
    else:
        # rows off their own size gather under the fallback rule: at aligned bases the tensors at offsets 2, 1, 3
        # (mod 4); at odd element offsets those at 2 and 0
        mis = [want[1], want[3], want[7]] if aligned else [want[1], want[5]]
        assert all(w[0] == "g" for w in mis)


def test_model_gradients(gc, orc):
    """roundtrip_gradients on a small model with odd sizes leaves what cat -> roundtrip -> copy-back leaves."""
    class Scalar(torch.nn.Module):
        def __init__(self):
            super().__init__()
            self.v = torch.nn.Parameter(torch.tensor(0.5))

    torch.manual_seed(3)
    model = torch.nn.Sequential(torch.nn.Linear(5, 3), torch.nn.Linear(3, 1), Scalar(), torch.nn.Linear(64, 130)).cuda()
    y = model[1](model[0](torch.randn(7, 5, device="cuda"))).sum() * model[2].v
    (y + model[3](torch.randn(2, 64, device="cuda")).sum()).backward()
    params = list(model.parameters())
    assert [q.numel() for q in params] == [15, 3, 3, 1, 1, 8320, 130] and all(q.grad is not None for q in params)
    for p in (gc.rate(16, 1), gc.accuracy(1e-3), gc.rate(12, 1)):
        for q in params:
            q.grad = torch.randn_like(q.grad) * 1e-3
        flat = torch.cat([q.grad.view(-1) for q in params])
        bits_ref = torch.zeros(1, dtype=torch.int64, device="cuda")
        ref = gc.roundtrip(flat, p, bits=bits_ref)
        cache = {}
        bits = torch.zeros(1, dtype=torch.int64, device="cuda")
        plan = gc.roundtrip_gradients(params, p, bits=bits, cache=cache)
        torch.cuda.synchronize()
        got = torch.cat([q.grad.view(-1) for q in params])
        assert np.array_equal(_bits_of(got), _bits_of(ref)) and int(bits.item()) == int(bits_ref.item())
        assert plan.rebuilds == 1 and list(cache.values()) == [plan]
        # a second call on the same .grad tensors reuses the plan (and round-trips the round trip)
        ref2 = gc.roundtrip(ref, p)
        assert gc.roundtrip_gradients(params, p, cache=cache) is plan and plan.rebuilds == 1
        torch.cuda.synchronize()
        assert np.array_equal(_bits_of(torch.cat([q.grad.view(-1) for q in params])), _bits_of(ref2))
        # a .grad replaced by a new tensor: the plan is rebuilt, the result still right
        old = params[5].grad  # kept alive: the new tensor cannot take its address
        params[5].grad = torch.randn_like(old) * 1e-3
        ref3 = gc.roundtrip(torch.cat([q.grad.view(-1) for q in params]), p)
        assert gc.roundtrip_gradients(params, p, cache=cache) is plan and plan.rebuilds == 2
        torch.cuda.synchronize()
        assert np.array_equal(_bits_of(torch.cat([q.grad.view(-1) for q in params])), _bits_of(ref3))
    # the default cache is the module's
    gc.gradient_plans.clear()
    plan = gc.roundtrip_gradients(params, gc.rate(16, 1))
    torch.cuda.synchronize()
    assert list(gc.gradient_plans.values()) == [plan]
    gc.gradient_plans.clear()


def test_refusals(gc, orc):
    import gcow_amd
    from gcow_amd._ffi import load
    from roundtrip_list_inputs import make_plan
    assert gcow_amd.roundtrip_tensors is gc.roundtrip_tensors and gcow_amd.roundtrip_gradients is gc.roundtrip_gradients
    p = gc.rate(16, 1)
    a = torch.zeros(64, device="cuda")
    b = torch.zeros(64, device="cuda", dtype=torch.bfloat16)
    with pytest.raises(gc.GcowError):
        gc.roundtrip_tensors([a, b], p)                           # mixed dtypes
    with pytest.raises(gc.GcowError):
        gc.roundtrip_tensors([a.to(torch.float16)], p)            # fp16
    with pytest.raises(gc.GcowError):
        gc.roundtrip_tensors([torch.zeros(128, device="cuda")[::2]], p)   # not contiguous
    with pytest.raises(gc.GcowError):
        gc.roundtrip_tensors([a], p, outs=[torch.zeros(63, device="cuda")])
    with pytest.raises(gc.GcowError):
        gc.roundtrip_tensors([a], p, outs=[a, a])
    with pytest.raises(gc.GcowError):
        gc.roundtrip_tensors([a, torch.zeros(4)], p)              # a host tensor
    # an empty list, and a list of empty tensors: bit count 0, at a fixed and a variable rate
    for q in (p, gc.accuracy(1e-3)):
        for ts in ([], [torch.zeros(0, device="cuda"), torch.zeros(0, device="cuda")]):
            bits = torch.full((1,), -1, dtype=torch.int64, device="cuda")
            assert gc.roundtrip_tensors(ts, q, bits=bits) == ts
            torch.cuda.synchronize()
            assert int(bits.item()) == 0
    # the C ABI: a short plan_bytes at plan time and at the device call; another parameter set; fp16 has no data_type
    L = load()
    st = torch.cuda.current_stream().cuda_stream
    assert make_plan(L, [a.data_ptr()], None, [64], 3, 3, p, slack=-8)[0] == 1
    rc, buf, used = make_plan(L, [a.data_ptr()], None, [64], 3, 3, p)
    assert rc == 0
    h = C.cast(buf, C.c_void_p)
    d = torch.zeros(used // 8 + 1, dtype=torch.int64, device="cuda")
    assert L.gcow_roundtrip_list_device(h, d.data_ptr(), used - 8, C.byref(p), None, st) == 1
    assert L.gcow_roundtrip_list_device(h, d.data_ptr(), used, C.byref(gc.rate(8, 1)), None, st) == 1
    assert L.gcow_roundtrip_list_device(h, None, used, C.byref(p), None, st) == 1
    assert make_plan(L, [a.data_ptr()], None, [64], 4, 3, p)[0] == 5
    torch.cuda.synchronize()
