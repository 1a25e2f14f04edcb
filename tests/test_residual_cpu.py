"""Error feedback on the CPU: the reference model (tests/residual_model.py) and the DDP hooks' use of it.

The wire hooks run exactly as written over gloo, with the oracle-backed codec injected; with
`GcowHookState.error_feedback` set every step's bucket must equal the mean, in rank order, of the model's per-rank
decodes of (gradient + carried error), and each rank's state must hold the model's new error, bit for bit."""
import os
import sys

import numpy as np
import pytest
import torch
import torch.distributed as dist

from test_dist_cpu import _Bucket, _init, _run

N = 4099
STEPS = 3


def _modes():
    from gcow_amd import codec
    return {"rate16": codec.rate(16, 1), "acc1e-3": codec.accuracy(1e-3), "rate8": codec.rate(8, 1)}


def _grad(step, rank, n=N):
    from oracle import oracle as O
    return O.gen_normal(n, 1e-3, 1000 + 16 * step + rank, True)


def _ef_hook_worker(rank, world, port, q, hook_name, mode):
    _init(rank, world, port)
    try:
        from gcow_amd import ddp
        from oracle import oracle as O
        from residual_model import OracleResidualCodec, model_step
        p = _modes()[mode]
        op = O.expert(*p.tuple())
        hook = getattr(ddp, hook_name)
        state = ddp.make_hook_state(hook=hook, params=p, codec=OracleResidualCodec(), error_feedback=True)
        errs = [None] * world  # the model's carried error of every rank
        bad = None
        for step in range(STEPS):
            decs = []
            for r in range(world):
                _, _, _, d, errs[r] = model_step(_grad(step, r), errs[r], op)
                decs.append(d)
            acc = np.zeros(N, np.float32)
            for d in decs:  # the hooks' order: 0 + x_0 + x_1 + ..., then / world
                acc = acc + d
            want = acc / np.float32(world)
            g = torch.from_numpy(_grad(step, rank).copy())
            out = hook(state, _Bucket(g, 0)).wait()
            out = out[0] if isinstance(out, (list, tuple)) else out
            got_e = state.error_buffer(0, g).numpy()
            if not np.array_equal(out.numpy().view(np.uint32), want.view(np.uint32)):
                bad = bad or "step %d: bucket != mean of the model's decodes" % step
            if not np.array_equal(got_e.view(np.uint32), errs[rank].view(np.uint32)):
                bad = bad or "step %d: carried error != the model's" % step
        if not np.any(errs[rank]):
            bad = bad or "the model's error is all zero: the test shows nothing"
        q.put((rank, True if bad is None else bad))
    except Exception as ex:  # pragma: no cover - reported through the queue
        q.put((rank, repr(ex)))
    finally:
        dist.destroy_process_group()


@pytest.mark.parametrize("mode", ["rate16", "acc1e-3"])
@pytest.mark.parametrize("hook", ["compressed_allgather_hook", "compressed_sharded_hook"])
def test_wire_hooks_error_feedback_gloo(hook, mode):
    _run(_ef_hook_worker, 2, hook, mode)


# ---------------------------------------------------------------------------------------------- one rank, in process
@pytest.fixture
def gloo_world1():
    tests = os.path.dirname(os.path.abspath(__file__))
    if tests not in sys.path:
        sys.path.insert(0, tests)
    dist.init_process_group("gloo", store=dist.HashStore(), rank=0, world_size=1)
    yield
    dist.destroy_process_group()


def _state(hook, mode, **kw):
    from gcow_amd import ddp
    from residual_model import OracleResidualCodec
    return ddp.make_hook_state(hook=hook, params=_modes()[mode], codec=OracleResidualCodec(), **kw)


@pytest.mark.parametrize("mode", ["rate16", "acc1e-3"])
@pytest.mark.parametrize("hook", ["compressed_allgather_hook", "compressed_sharded_hook"])
def test_flag_unset_never_calls_encode_residual(orc, gloo_world1, hook, mode):
    from gcow_amd import ddp
    op = orc.expert(*_modes()[mode].tuple())
    state = _state(getattr(ddp, hook), mode)
    assert state.error_feedback is False
    for step in range(2):
        a = _grad(step, 0)
        out = getattr(ddp, hook)(state, _Bucket(torch.from_numpy(a.copy()), 0)).wait()
        dec = orc.decompress(orc.compress(a, op)[0], a.shape, op)
        want = (np.zeros_like(dec) + dec) / np.float32(1)
        assert np.array_equal(out.numpy().view(np.uint32), want.view(np.uint32))  # the parent's result, unchanged
    names = [r[0] for r in state.codec.records]
    assert "encode" in names and "encode_residual" not in names
    assert not state._errors


def test_roundtrip_hook_refuses_error_feedback(orc):
    from gcow_amd import ddp
    state = ddp.GcowHookState(error_feedback=True)
    with pytest.raises(ValueError, match="error_feedback"):
        ddp.roundtrip_hook(state, _Bucket(torch.zeros(16), 0))


@pytest.mark.parametrize("hook", ["compressed_allgather_hook", "compressed_sharded_hook"])
def test_changed_bucket_size_starts_from_zeros(orc, gloo_world1, hook):
    from gcow_amd import ddp
    from residual_model import model_step
    mode = "rate8"
    op = orc.expert(*_modes()[mode].tuple())
    state = _state(getattr(ddp, hook), mode, error_feedback=True)
    a = _grad(0, 0)
    getattr(ddp, hook)(state, _Bucket(torch.from_numpy(a.copy()), 0)).wait()
    e1 = state.error_buffer(0, torch.from_numpy(a)).numpy().copy()
    assert np.array_equal(e1.view(np.uint32), model_step(a, None, op)[4].view(np.uint32)) and np.any(e1)
    b = _grad(1, 0, N + 4)  # the same bucket index with another size (DDP's bucket rebuild)
    tb = torch.from_numpy(b.copy())
    out = getattr(ddp, hook)(state, _Bucket(tb, 0)).wait()
    _, _, _, d, e = model_step(b, None, op)  # from zeros, not from e1
    assert np.array_equal(out.numpy().view(np.uint32), ((np.zeros_like(d) + d) / np.float32(1)).view(np.uint32))
    got = state.error_buffer(0, tb)
    assert got.numel() == N + 4 and np.array_equal(got.numpy().view(np.uint32), e.view(np.uint32))
    assert len(state._errors) == 1  # the old buffer is dropped
    state.reset_error_feedback()
    assert not state._errors and not torch.any(state.error_buffer(0, tb))


@pytest.mark.parametrize("mode", ["rate8", "rate16", "acc1e-3"])
def test_model_identity(orc, mode):
    """sum_t yhat_t - sum_t x_t = e_0 - e_T up to the fp32 rounding of the two operations per step: y = fl(x + e) and
    r = fl(y - yhat) are each within 2^-24 relative, |r| <= |y| at these rates, so each step adds at most
    2^-23 max|y| per value; compared in float64 against T 2^-23 max|y|."""
    from residual_model import model_step
    op = orc.expert(*_modes()[mode].tuple())
    T = 20
    e0 = model_step(_grad(99, 0), None, op)[4]  # a real residual to start from
    e = e0.copy()
    sx = np.zeros(N, np.float64)
    sd = np.zeros(N, np.float64)
    ymax = 0.0
    for t in range(T):
        x = _grad(t, 1)
        y, _, _, d, e = model_step(x, e, op)
        assert np.all(np.isfinite(y)) and np.all(np.abs(e) <= np.abs(y).max())
        sx += x
        sd += d
        ymax = max(ymax, float(np.abs(y).max()))
    lhs = sd - sx
    rhs = e0.astype(np.float64) - e.astype(np.float64)
    assert np.abs(lhs - rhs).max() <= T * 2.0 ** -23 * ymax
    # and the point of it: the mean of what was sent is within |e_0 - e_T| / T of the mean of what was meant
    assert np.abs(lhs).max() / T <= (np.abs(e0).max() + np.abs(e).max()) / T + 2.0 ** -23 * ymax


@pytest.mark.parametrize("bf16", [False, True], ids=["fp32", "bf16"])
@pytest.mark.parametrize("n", [8193, 24583])
def test_gpu_case_inputs_reach_the_rare_lanes(orc, n, bf16):
    """The inputs of tests/test_gpu_residual.py do drive what they are built for: words the pair decoder's fast path
    hands to the generic decoder (tests/test_dec_pair_fastpath.py's model of it), non-finite sums (the encoder's
    special lane and the zeroed residual) and subnormal residuals."""
    from residual_model import model_step
    from test_dec_pair_fastpath import fast_pair
    from test_gpu_residual import _case
    c = _case(n, bf16, "rate16")
    w, _, e1 = c["steps"][0]
    assert sum(1 for v in w.tolist() if fast_pair(int(v), True)[0]) >= 100
    y = model_step(c["xs"][0], c["e0"], c["op"])[0]
    bad = ~np.isfinite(y)
    assert bad.sum() >= 5 and not np.any(e1[bad]) and np.all(np.isfinite(e1))
    assert np.any((np.abs(e1) < np.finfo(np.float32).tiny) & (e1 != 0))
