"""GPU parity of the round trip with a tolerance relative to each tensor (gcow_roundtrip_rel_device,
codec.roundtrip_tensors_relative / roundtrip_gradients_relative, DeviceCodec.roundtrip_relative, roundtrip_hook with
relative_bits), bitwise against the per-tensor oracle expectation of tests/relative_inputs.py: every output (a bf16
output: the fp32 decode rounded to nearest even), the per-tensor maxima and the summed bit count.

Lists: edges (1, 3, 4, 5, 0, C - 1, C, C + 1, 3 C + 7 values, 2, 7; C = 8192 is a direct chunk), small (300 tensors of
1 .. 9 values around one of 8192: the bisection's depth, many tensors in one gather chunk) and special (all zero, all
NaN, Inf / NaN spliced into finite data, subnormals, scale 2^-100 under the floor, scale 3e38, -0.0). Every tensor has
its own power-of-two scale. Four dtype pairs, rel_bits 0 / 8 / 24, maxprec 64 / 12, and two placements: separate
allocations, and tensors carved back to back out of one buffer one element apart, so that bf16 tensors start at odd
elements and fp32 tensors off 16 bytes. Outputs go into sentinel-filled buffers whose gaps are checked afterwards."""
import os
import sys

import numpy as np
import pytest

torch = pytest.importorskip("torch")

TESTS = os.path.dirname(os.path.abspath(__file__))
if TESTS not in sys.path:
    sys.path.insert(0, TESTS)

pytestmark = pytest.mark.gpu

DTYPES = [(False, False), (True, True), (False, True), (True, False)]
DTYPE_IDS = ["fp32-fp32", "bf16-bf16", "fp32-bf16", "bf16-fp32"]
SENT = {False: np.float32(-1234.5).view(np.uint32), True: np.uint16(0xC49A)}  # sentinel bits (bf16: -1232.0)
PAD = 8  # sentinel elements around a separately allocated tensor; its base stays 16-byte aligned


@pytest.fixture(scope="module")
def gc():
    if not torch.cuda.is_available():
        pytest.fail("GPU tests need a device")
    from gcow_amd import codec
    return codec


def _bits_of(t):
    """The tensor's values as raw bits (uint32 for fp32, uint16 for bf16)."""
    if t.dtype == torch.bfloat16:
        return t.view(torch.int16).cpu().numpy().view(np.uint16)
    return t.cpu().numpy().view(np.uint32)


def _as_bits(a, bf16):
    return a if bf16 else a.view(np.uint32)


def _upload(bits_np, bf16):
    if bf16:
        return torch.from_numpy(bits_np.view(np.int16)).cuda().view(torch.bfloat16)
    return torch.from_numpy(bits_np.view(np.float32)).cuda()


class Placed:
    """Tensors on the device inside sentinel-filled buffers. carved: one buffer, the tensors back to back one element
    apart from element 1 on; else one buffer per tensor with PAD sentinels on either side."""

    def __init__(self, sizes, bf16, carved, arrays=None):
        self.bf16 = bf16
        self.bufs, self.tensors, self.spans = [], [], []  # spans: (buffer index, lo, hi) per tensor
        dt = np.uint16 if bf16 else np.uint32
        if carved:
            pos, at = [], 1
            for n in sizes:
                pos.append(at)
                at += n + 1
            host = [np.full(at + 16, SENT[bf16], dt)]
            self.spans = [(0, p, p + n) for p, n in zip(pos, sizes)]
        else:
            host = [np.full(n + 2 * PAD, SENT[bf16], dt) for n in sizes]
            self.spans = [(i, PAD, PAD + n) for i, n in enumerate(sizes)]
        if arrays is not None:
            for (b, lo, hi), a in zip(self.spans, arrays):
                host[b][lo:hi] = _as_bits(a, bf16)
        self.bufs = [_upload(h, bf16) for h in host]
        self.tensors = [self.bufs[b][lo:hi] for b, lo, hi in self.spans]

    def values(self):
        """Per-tensor bits."""
        host = [_bits_of(b) for b in self.bufs]
        return [host[b][lo:hi] for b, lo, hi in self.spans]

    def gaps_clean(self):
        host = [_bits_of(b) for b in self.bufs]
        cover = [np.zeros(h.size, bool) for h in host]
        for b, lo, hi in self.spans:
            cover[b][lo:hi] = True
        return all(bool((h[~c] == SENT[self.bf16]).all()) for h, c in zip(host, cover))


def _want(outs_ref, bf16_out):
    from roundtrip_inputs import bf16_rne
    return [bf16_rne(d) if bf16_out else d.view(np.uint32) for d in outs_ref]


def _same(got, want):
    return len(got) == len(want) and all(np.array_equal(g, w) for g, w in zip(got, want))


def _run(gc, name, bf16_in, bf16_out, k, maxprec, carved):
    """Out of place (always) and in place (equal dtypes); returns the out-of-place plan object."""
    from relative_inputs import expect, tensors
    ts_np = tensors(name, bf16_in)
    outs_ref, amax_ref, bits_ref = expect(name, bf16_in, k, maxprec)
    sizes = [t.size for t in ts_np]
    want = _want(outs_ref, bf16_out)
    src = [_as_bits(t, bf16_in) for t in ts_np]
    ins = Placed(sizes, bf16_in, carved, ts_np)
    outs = Placed(sizes, bf16_out, carved)
    amax = torch.full((len(sizes),), -1.0, dtype=torch.float32, device="cuda")
    bits = torch.full((1,), -1, dtype=torch.int64, device="cuda")
    plan = gc.TensorListRelative(k, maxprec)
    got = gc.roundtrip_tensors_relative(ins.tensors, k, outs=outs.tensors, absmax=amax, bits=bits, plan=plan,
                                        maxprec=maxprec)
    torch.cuda.synchronize()
    assert [g.data_ptr() for g in got] == [o.data_ptr() for o in outs.tensors]
    assert _same(outs.values(), want)
    assert outs.gaps_clean()
    assert _same(ins.values(), src) and ins.gaps_clean()  # the inputs are only read
    assert np.array_equal(_bits_of(amax), amax_ref.view(np.uint32))
    assert int(bits.item()) == bits_ref
    if bf16_in == bf16_out:
        bits2 = torch.full((1,), -1, dtype=torch.int64, device="cuda")
        plan2 = gc.TensorListRelative(k, maxprec)
        gc.roundtrip_tensors_relative(ins.tensors, k, bits=bits2, plan=plan2, maxprec=maxprec)  # absmax kept on the plan
        torch.cuda.synchronize()
        assert _same(ins.values(), want) and ins.gaps_clean()
        assert np.array_equal(_bits_of(plan2.absmax), amax_ref.view(np.uint32)) and int(bits2.item()) == bits_ref
    return plan


@pytest.mark.parametrize("maxprec", [64, 12])
@pytest.mark.parametrize("k", [0, 8, 24])
@pytest.mark.parametrize("bf16_in,bf16_out", DTYPES, ids=DTYPE_IDS)
@pytest.mark.parametrize("carved", [False, True], ids=["separate", "carved"])
@pytest.mark.parametrize("name", ["edges", "small", "special"])
def test_lists(gc, orc, name, carved, bf16_in, bf16_out, k, maxprec):
    from relative_inputs import tensors
    plan = _run(gc, name, bf16_in, bf16_out, k, maxprec, carved)
    s = plan.stats()
    sizes = [t.size for t in tensors(name, bf16_in)]
    assert s.total_values == sum(sizes) and s.total_blocks == sum((n + 3) // 4 for n in sizes)
    assert s.segments == sum(1 for n in sizes if n) and s.gather_chunks > 0
    if name == "edges":
        # both kinds of chunk ran: carved, the tensors of 8193 and 24583 values start at even elements (4-byte aligned
        # for bf16 too), those of 8191 and 8192 at odd ones
        assert s.direct_chunks == (7 if not carved or not (bf16_in or bf16_out) else 5)
    elif not carved:
        assert s.direct_chunks == 1  # the tensor of 8192 (small) / of 4100 (special) values


@pytest.mark.parametrize("bf16", [False, True], ids=["fp32", "bf16"])
@pytest.mark.parametrize("k", [0, 8, 24])
def test_equals_roundtrip_per_tensor(gc, orc, k, bf16):
    """The edges list against the library's own contiguous round trip of each tensor under its parameter set."""
    from relative_inputs import absmax_of, minexp_of, tensors
    ts_np = tensors("edges", bf16)
    ins = Placed([t.size for t in ts_np], bf16, False, ts_np)
    outs = gc.roundtrip_tensors_relative(ins.tensors, k, outs=[torch.empty_like(t) for t in ins.tensors])
    for t_np, t, o in zip(ts_np, ins.tensors, outs):
        if t_np.size == 0:
            continue
        p = gc.expert(1, 16658, 64, minexp_of(absmax_of(t_np), k))
        ref = gc.roundtrip(t.clone(), p)
        torch.cuda.synchronize()
        assert np.array_equal(_bits_of(o), _bits_of(ref)), t_np.size


def test_plan_reuse_and_gradients(gc, orc):
    from relative_inputs import expect, tensors
    ts_np = tensors("edges", False)
    want = _want(expect("edges", False, 8, 64)[0], False)
    ins = Placed([t.size for t in ts_np], False, False, ts_np)
    work = [t.clone() for t in ins.tensors]
    plan = gc.TensorListRelative(8)
    outs = [torch.empty_like(t) for t in work]
    gc.roundtrip_tensors_relative(work, 8, outs=outs, plan=plan)
    gc.roundtrip_tensors_relative(work, 8, outs=outs, plan=plan)
    torch.cuda.synchronize()
    assert plan.rebuilds == 1 and _same([_bits_of(o) for o in outs], want)   # the same tensors: no new plan
    work[8] = work[8].clone()                                                # a moved tensor: a new plan
    gc.roundtrip_tensors_relative(work, 8, outs=outs, plan=plan)
    torch.cuda.synchronize()
    assert plan.rebuilds == 2 and _same([_bits_of(o) for o in outs], want)
    with pytest.raises(gc.GcowError):
        gc.roundtrip_tensors_relative(work, 9, outs=outs, plan=plan)         # the plan object is another rel_bits'
    # gradients, in place, the plan cached under (rel_bits, maxprec, device)
    params = [torch.nn.Parameter(torch.zeros(t.numel(), device="cuda")) for t in ins.tensors]
    for q, t in zip(params, ins.tensors):
        q.grad = t.clone()
    params.append(torch.nn.Parameter(torch.zeros(3, device="cuda")))         # no .grad: skipped
    cache = {}
    bits = torch.zeros(1, dtype=torch.int64, device="cuda")
    gp = gc.roundtrip_gradients_relative(params, 8, bits=bits, cache=cache)
    torch.cuda.synchronize()
    assert _same([_bits_of(q.grad) for q in params[:-1]], want) and int(bits.item()) == expect("edges", False, 8, 64)[2]
    assert list(cache.values()) == [gp] and gp.rebuilds == 1
    assert gc.roundtrip_gradients_relative(params, 8, cache=cache) is gp and gp.rebuilds == 1
    assert gc.roundtrip_gradients_relative(params, 8, cache=cache, maxprec=12) is not gp
    torch.cuda.synchronize()


def test_refusals(gc, orc):
    import gcow_amd
    assert gcow_amd.roundtrip_tensors_relative is gc.roundtrip_tensors_relative
    a = torch.zeros(64, device="cuda")
    with pytest.raises(gc.GcowError):
        gc.roundtrip_tensors_relative([a], 25)                                  # rel_bits > 24
    with pytest.raises(gc.GcowError):
        gc.roundtrip_tensors_relative([a.to(torch.float16)], 8)                 # fp16
    with pytest.raises(gc.GcowError):
        gc.roundtrip_tensors_relative([a, a.to(torch.bfloat16)], 8)             # mixed dtypes
    with pytest.raises(gc.GcowError):
        gc.roundtrip_tensors_relative([a], 8, absmax=torch.zeros(2, device="cuda"))   # absmax of another length
    with pytest.raises(gc.GcowError):
        gc.roundtrip_tensors_relative([a], 8, outs=[torch.zeros(63, device="cuda")])
    # an empty list and a list of empty tensors: bit count 0, the maxima 0
    bits = torch.full((1,), -1, dtype=torch.int64, device="cuda")
    assert gc.roundtrip_tensors_relative([], 8, bits=bits) == []
    torch.cuda.synchronize()
    assert int(bits.item()) == 0
    amax = torch.full((2,), -1.0, device="cuda")
    bits.fill_(-1)
    gc.roundtrip_tensors_relative([torch.zeros(0, device="cuda")] * 2, 8, absmax=amax, bits=bits)
    torch.cuda.synchronize()
    assert int(bits.item()) == 0 and amax.tolist() == [0.0, 0.0]


# ---------------------------------------------------------------------------------------------- roundtrip_hook, RCCL
@pytest.fixture
def nccl_world1():
    import torch.distributed as dist
    dist.init_process_group("nccl", store=dist.HashStore(), rank=0, world_size=1, device_id=torch.device("cuda", 0))
    yield
    dist.destroy_process_group()


class _Bucket:
    def __init__(self, t, i, sizes):
        self.t, self.i, self.sizes = t, i, sizes

    def buffer(self):
        return self.t

    def index(self):
        return self.i

    def gradients(self):
        out, at = [], 0
        for n in self.sizes:
            out.append(self.t[at:at + n])
            at += n
        return out


@pytest.mark.parametrize("bf16", [False, True], ids=["fp32", "bf16"])
def test_roundtrip_hook_relative_world1(gc, orc, nccl_world1, bf16):
    """One rank over RCCL: with relative_bits the hook round-trips the bucket's per-parameter views in place, each
    under its own tolerance, and never encodes."""
    from gcow_amd import ddp
    from gcow_amd import dist as gdist
    from relative_inputs import HOOK_SIZES, expect, tensors

    calls = []

    class CountingCodec(gdist.DeviceCodec):
        def roundtrip_relative(self, *a, **k):
            calls.append("roundtrip_relative")
            return super().roundtrip_relative(*a, **k)

        def roundtrip(self, *a, **k):
            calls.append("roundtrip")
            return super().roundtrip(*a, **k)

        def encode(self, *a, **k):
            calls.append("encode")
            return super().encode(*a, **k)

    cdc = CountingCodec()
    state = ddp.make_hook_state(hook=ddp.roundtrip_hook, params=gc.accuracy(1e-3), codec=cdc, relative_bits=8)
    ts_np = tensors("hook", bf16)
    want = np.concatenate(_want(expect("hook", bf16, 8, 64)[0], bf16))
    flat = np.concatenate([_as_bits(t, bf16) for t in ts_np])
    for i in range(2):  # the second bucket index gets a plan of its own
        t = _upload(flat.copy(), bf16)
        out = ddp.roundtrip_hook(state, _Bucket(t, i, HOOK_SIZES)).wait()
        torch.cuda.synchronize()
        out = out[0] if isinstance(out, (list, tuple)) else out
        assert out.data_ptr() == t.data_ptr()
        assert np.array_equal(_bits_of(out), want), i
    assert calls == ["roundtrip_relative"] * 2


def test_hooks_refuse_relative_bits(gc, orc):
    """The wire hooks raise with the field set; so does roundtrip_hook for a codec without roundtrip_relative or a
    bucket that is neither fp32 nor bf16. All before any collective: no process group is needed."""
    from gcow_amd import ddp
    t = torch.zeros(64, device="cuda")
    state = ddp.GcowHookState(relative_bits=8)
    for hook in (ddp.compressed_allgather_hook, ddp.compressed_sharded_hook):
        with pytest.raises(ValueError):
            hook(state, _Bucket(t, 0, [64]))

    class Bare:
        pass

    with pytest.raises(ValueError):
        ddp.roundtrip_hook(ddp.GcowHookState(relative_bits=8, codec=Bare()), _Bucket(t, 0, [64]))
    with pytest.raises(ValueError):
        ddp.roundtrip_hook(ddp.GcowHookState(relative_bits=8), _Bucket(t.to(torch.float16), 0, [64]))
