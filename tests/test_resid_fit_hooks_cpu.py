"""compressed_allgather_hook with target_bits, fit_on_device AND error_feedback on gloo process groups on the CPU,
worlds 2 and 3, with the harness of tests/test_fit_on_device_hooks_cpu.py: its FitCodec combined with
residual_model.OracleResidualCodec, plus the two calls the combination needs -- rate_table_residual (the oracle table
of y = x + e) and encode_residual_fitted (the numpy model's step under the record's set).

Three steps: in every step, on every rank, the set used is the fit of the sum over ranks of the oracle tables of
y_r = x_r + e_r, with e_r carried by the numpy model from the step before; the W oracle streams of y_r under that set
total the record's bits and at most world * BUDGET; each rank's error buffer is the model's bit for bit; the bucket is
the mean of the oracle decodes of y_r. A budget below one bit per block; the ValueError for a codec without the two
calls, and the combinations that stay refused."""
import os
import sys

import numpy as np
import pytest
import torch
import torch.distributed as dist

TESTS = os.path.dirname(os.path.abspath(__file__))
if TESTS not in sys.path:
    sys.path.insert(0, TESTS)

import test_fit_on_device_hooks_cpu as F  # noqa: E402
from test_dist_cpu import _Bucket, _init, _run  # noqa: E402

H = F.H
N, TARGET, BUDGET, MAXPREC = H.N, H.TARGET, H.BUDGET, H.MAXPREC


def _resid_fit_codec_class():
    import rate_table_inputs as RT
    import residual_model as RM
    from oracle_codec import _np_values

    class ResidFitCodec(F._fit_codec_class(), RM.OracleResidualCodec):
        """FitCodec + encode_residual + the two calls of fit_on_device with error_feedback."""

        def rate_table_residual(self, x, err, maxprec=64, slot=None):
            self.tables += 1
            y = RM.model_step(_np_values(x), err.numpy().copy(), RM.O.expert(1, 16658, maxprec, 0))[0]
            return torch.from_numpy(RT.oracle_table(y, maxprec).copy())

        def encode_residual_fitted(self, x, err, minexp_word, maxprec=64, index_stride=0, slot=None):
            return self.encode_residual(x, err, self._params(minexp_word, maxprec), index_stride, slot)

    return ResidFitCodec


def _mean(decodes):
    acc = np.zeros(N, np.float32)
    for d in decodes:
        acc = acc + d
    return acc / np.float32(len(decodes))


def _worker(rank, world, port, q):
    _init(rank, world, port)
    try:
        import rate_table_inputs as RT
        import residual_model as RM
        from gcow_amd import codec, ddp
        from oracle import oracle as O
        p0 = codec.expert(1, 16658, MAXPREC, -14)
        cdc = _resid_fit_codec_class()()
        hook = ddp.compressed_allgather_hook
        state = ddp.make_hook_state(hook=hook, params=p0, codec=cdc, target_bits=TARGET, fit_on_device=True,
                                    error_feedback=True)
        errs = [np.zeros(N, np.float32) for _ in range(world)]  # every rank's carried error, by the model
        fits = []
        for step in range(3):
            grads = H._grads(world, step)
            ys = [RM.model_step(grads[r], errs[r], O.expert(1, 16658, MAXPREC, 0))[0] for r in range(world)]
            total = sum(RT.oracle_table(y, MAXPREC) for y in ys)
            me, bits = RT.fit(total, world * BUDGET)
            own = (1, 16658, MAXPREC, me)  # the fit of this step's tables of y
            g = torch.from_numpy(grads[rank].copy())
            hook(state, _Bucket(g, 0)).wait()
            used = cdc.seen[-1]
            everyone = [None] * world
            dist.all_gather_object(everyone, used)
            assert all(u == used for u in everyone), (step, everyone)
            assert used == own, (step, used, own)
            steps = [RM.model_step(grads[r], errs[r], O.expert(*used)) for r in range(world)]
            sent = sum(s[2] for s in steps)  # the W streams of y_r that travelled
            assert sent == bits and sent <= world * BUDGET, (step, sent, bits)
            assert codec.read_fit(state.fit_record(0)) == (me, 0, bits) and cdc.fits[-1] == (me, 0, bits)
            assert not state._fits
            got_e = state.error_buffer(0, g).numpy()
            assert np.array_equal(got_e.view(np.uint32), steps[rank][4].view(np.uint32)), step
            want = _mean([s[3] for s in steps])
            assert np.array_equal(g.numpy().view(np.uint32), want.view(np.uint32)), step
            errs = [s[4] for s in steps]
            fits.append(me)
        assert any(np.any(e != 0) for e in errs)  # the carried error is there: y differs from x
        assert cdc.tables == 3 and len(cdc.seen) == 3 and len(cdc.fits) == 3
        q.put((rank, True))
    except Exception as ex:  # pragma: no cover - reported through the queue
        q.put((rank, repr(ex)))
    finally:
        dist.destroy_process_group()


@pytest.mark.parametrize("world", [2, 3])
def test_allgather_hook_fits_bucket_plus_carried_error(orc, world):
    _run(_worker, world)


def _coarsest_worker(rank, world, port, q):
    """A budget below one bit per block: status 1, the coarsest set, on every rank; the error is y - decode under it."""
    _init(rank, world, port)
    try:
        import residual_model as RM
        from gcow_amd import codec, ddp
        from oracle import oracle as O
        p0 = codec.expert(1, 16658, MAXPREC, -14)
        cdc = _resid_fit_codec_class()()
        hook = ddp.compressed_allgather_hook
        state = ddp.make_hook_state(hook=hook, params=p0, codec=cdc, target_bits=0.1, fit_on_device=True,
                                    error_feedback=True)
        grads = H._grads(world, 0)
        g = torch.from_numpy(grads[rank].copy())
        hook(state, _Bucket(g, 0)).wait()
        assert cdc.seen == [(1, 16658, MAXPREC, 133)]
        assert codec.read_fit(state.fit_record(0)) == (133, 1, world * ((N + 3) // 4))
        steps = [RM.model_step(a, None, O.expert(1, 16658, MAXPREC, 133)) for a in grads]
        assert np.array_equal(g.numpy().view(np.uint32), _mean([s[3] for s in steps]).view(np.uint32))
        assert np.array_equal(state.error_buffer(0, g).numpy().view(np.uint32), steps[rank][4].view(np.uint32))
        q.put((rank, True))
    except Exception as ex:  # pragma: no cover
        q.put((rank, repr(ex)))
    finally:
        dist.destroy_process_group()


def test_budget_below_one_bit_per_block(orc):
    _run(_coarsest_worker, 2)


def test_value_errors(orc):
    """Raised before any collective: no process group here."""
    from gcow_amd import codec, ddp
    acc = codec.accuracy(1e-3)
    b = _Bucket(torch.zeros(N), 0)
    S = ddp.GcowHookState
    kw = dict(params=acc, target_bits=4.0, fit_on_device=True, error_feedback=True)
    # a codec with the fit calls but without the two residual ones: named, with the mode that needs them
    with pytest.raises(ValueError, match="error_feedback.*rate_table_residual, encode_residual_fitted"):
        ddp.compressed_allgather_hook(S(codec=F._fit_codec_class()(), **kw), b)
    # what stays refused, with the full codec
    full = _resid_fit_codec_class()()
    with pytest.raises(ValueError, match="another kernel family"):
        ddp.compressed_sharded_hook(S(codec=full, sharded=True, **kw), b)
    with pytest.raises(ValueError, match="another kernel family"):
        ddp.compressed_sharded_hook(S(codec=full, sharded=True, compress_mean=True, **kw), b)
    with pytest.raises(ValueError, match="error_feedback is for the wire hooks"):
        ddp.roundtrip_hook(S(codec=full, **kw), b)
