"""TEST INFRASTRUCTURE ONLY -- the reference model of error feedback (include/gcow.h gcow_encode_residual_device) in
numpy over the oracle, and an oracle-backed codec with `encode_residual` for running the DDP hooks on CPU tensors.

    y = (x.astype(f32) + e).astype(f32)        one fp32 add
    w, bits = O.compress(y, p)                 the stream of the fp32 array y
    d = O.decompress(w, (n,), p)               libzfp 0.5.5 decode
    r = y - d;  r[~isfinite(r)] = 0            one fp32 subtract, non-finite residuals dropped
"""
from __future__ import annotations

import numpy as np
import torch

from oracle import oracle as O
from oracle_codec import OracleCodec, _np_values, _params


def widen(x: np.ndarray) -> np.ndarray:
    """fp32 values of a bucket given as float32, or as bf16 bit patterns (uint16): exact widening."""
    if x.dtype == np.uint16:
        return (x.astype(np.uint32) << 16).view(np.float32)
    return np.asarray(x, np.float32)


def model_step(x: np.ndarray, e: np.ndarray | None, p):
    """One step: -> (y, words, bits, decode, new error). x: float32 or uint16 (bf16 bits); e: float32 or None (zeros)."""
    xf = widen(x)
    e = np.zeros(xf.size, np.float32) if e is None else e
    with np.errstate(over="ignore", invalid="ignore"):
        y = (xf + e).astype(np.float32)
        w, bits = O.compress(y, p)
        d = O.decompress(w, (y.size,), p)
        r = (y - d).astype(np.float32)
    r[~np.isfinite(r)] = 0
    return y, w, bits, d, r


class OracleResidualCodec(OracleCodec):
    """OracleCodec plus DeviceCodec.encode_residual, every byte the model's."""

    def encode_residual(self, x: torch.Tensor, err: torch.Tensor, params, index_stride: int = 0, slot=None):
        assert err.dtype == torch.float32 and err.numel() == x.numel()
        y, _, bits, _, r = model_step(_np_values(x), err.numpy().copy(), _params(params))
        out = self.encode(torch.from_numpy(y), params, index_stride, slot)  # the stream (and index) of the fp32 y
        assert int(out[1]) == bits
        err.copy_(torch.from_numpy(r))
        self.records.append(("encode_residual", y, r.copy()))
        return out
