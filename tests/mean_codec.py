"""TEST INFRASTRUCTURE ONLY -- the reference model of decode + mean + encode (include/gcow.h
gcow_decode_mean_encode_device) in numpy over the oracle, and oracle-backed codecs with DeviceCodec.decode_mean_encode
for running compressed_sharded_hook with `compress_mean` on CPU tensors.

    m = ((0 + x_0) + x_1 + ...) / W            fp32 sums in rank order, one fp32 division
    y, words, bits, yhat, e' = model_step(m, e, p)   (tests/residual_model.py; e = None and e' unused without feedback)
"""
from __future__ import annotations

import numpy as np
import torch

from oracle_codec import _params
from residual_model import OracleResidualCodec, model_step


def mean_of(decodes) -> np.ndarray:
    """The mean decode_mean forms from the per-rank decodes (fp32 arrays, rank order)."""
    acc = np.zeros(decodes[0].size, np.float32)
    with np.errstate(over="ignore", invalid="ignore"):
        for d in decodes:
            acc = (acc + d).astype(np.float32)
        return (acc / np.float32(len(decodes))).astype(np.float32)


def mean_model_step(decodes, e, p):
    """-> (m, words, bits, yhat, new error): the mean of the decodes coded under p, with carried error e (None: the
    plain encode -- the stream of m itself; a +0 error changes no stream bit, only -0 values of y)."""
    m = mean_of(decodes)
    _, w, bits, d, r = model_step(m, e, p)
    return m, w, bits, d, r


class _RecordingDecode:
    """`decode` that also records what it was given: ("decode", words in the buffer, its dtype, n values)."""

    def decode(self, words, n, params, index=None, index_stride=0, out=None):
        self.records.append(("decode", int(words.numel()), words.dtype, int(n)))
        return super().decode(words, n, params, index=index, index_stride=index_stride, out=out)


class OracleComposedCodec(_RecordingDecode, OracleResidualCodec):
    """No decode_mean_encode: the hook composes decode_mean and encode / encode_residual."""


class OracleMeanCodec(_RecordingDecode, OracleResidualCodec):
    """OracleResidualCodec plus DeviceCodec.decode_mean_encode, every byte the model's."""

    def decode_mean_encode(self, streams, stream_words, nstreams, n, params, index=None, index_words=0,
                           index_stride=0, out_params=None, err=None, out_index_stride=0, slot=None):
        m = self.decode_mean(streams, stream_words, nstreams, n, params, index, index_words, index_stride)
        po = out_params if out_params is not None else params
        if err is not None:
            out = self.encode_residual(m, err, po, out_index_stride, slot)
        else:
            out = self.encode(m, po, out_index_stride, slot)
        self.records.append(("decode_mean_encode", int(n), int(nstreams), _params(po)))
        return out
