#!/usr/bin/env python3
"""Steady-state timing of error feedback under a bit budget on one GPU: n fp32 values (default
256 Mi), x and e normal with sigma 1e-3, a budget of 8 bits per value.

  a  the rate table: gcow_rate_table_device on x alone  |  gcow_rate_table_residual_device on (x, e): twice the bytes
  b  the residual encode under the same fitted minexp, out of place so that every call does the same work:
     gcow_encode_residual_device with host parameters  |  gcow_encode_residual_fitted_device with the device word
  c  the whole step, e carried in place from call to call:
     the form with a host read (torch add into a temporary, rate_table, fit_device, read_fit, encode_residual)  |
     FittedResidualEncoder (table of y in registers, fit_device, fitted residual encode; no host read)

Each pair is timed alternately, ROUNDS times, STEPS calls per window after WARM calls; a window is a host clock around
calls that end in a device synchronise. Prints one JSON line per leg with the median, the minimum and the maximum of
the windows' per-call times in ms. usage: resid_fit_time.py [--n VALUES] [--rounds R] [--steps S]"""
import ctypes as C
import json
import os
import statistics
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
from gcow_amd import codec  # noqa: E402


def arg(name, default):
    return int(sys.argv[sys.argv.index(name) + 1]) if name in sys.argv else default


N = arg("--n", 256 << 20)
ROUNDS, STEPS, WARM = arg("--rounds", 5), arg("--steps", 50), 3
BPV = 8

if not torch.cuda.is_available():
    sys.exit("resid_fit_time.py needs a GPU: nothing is measured without one")


def window(fn, steps=STEPS):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(steps):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3 / steps


def alternate(legs, before=None):
    """legs: {name: fn}; -> {name: [per-call ms of each round]}, the legs taking turns within a round."""
    for k, fn in legs.items():
        if before is not None:
            before(k)
        for _ in range(WARM):
            fn()
    out = {k: [] for k in legs}
    for _ in range(ROUNDS):
        for k, fn in legs.items():
            if before is not None:
                before(k)
            out[k].append(window(fn))
    return out


def report(what, times, **extra):
    for k, v in times.items():
        print(json.dumps({"leg": what, "form": k, "n": N, "ms_median": round(statistics.median(v), 4),
                          "ms_min": round(min(v), 4), "ms_max": round(max(v), 4), "rounds": len(v), "steps": STEPS,
                          **extra}), flush=True)


L = codec.load()
dev = torch.device("cuda")
x = torch.empty(N, dtype=torch.float32, device=dev)
e = torch.empty(N, dtype=torch.float32, device=dev)
codec.fill_normal(x, 1e-3, seed=0x67636F77, inject=False)
codec.fill_normal(e, 1e-3, seed=0x5EED, inject=False)
budget = BPV * N
st = torch.cuda.current_stream().cuda_stream

# ---- a: the table pass
rt = codec.RateTable(N, torch.float32, dev)
a = alternate({"rate_table(x)": lambda: rt(x), "rate_table_residual(x, e)": lambda: rt(x, err=e)})
report("a_table", a)  # 16 against 32 bytes read per block
me, bits = codec.fit_minexp(rt(x, err=e), budget)
print(json.dumps({"fitted_minexp": me, "bits_per_value": round(bits / N, 4)}), flush=True)

# ---- b: the residual encode, out of place (e read, e2 written): the same work every call
p = codec.fitted_params(64, me)
renc = codec.ResidualEncoder(N, torch.float32, p, dev, index_stride=8)
assert renc.path == codec.RESID_FUSED_VAR
fenc = codec.Encoder((N,), torch.float32, codec.fitted_params(64, 0), dev, index_stride=8)
word = torch.tensor([me], dtype=torch.int32, device=dev)
e2 = torch.empty_like(e)
f = codec.field_of(x)


def b_host():
    codec.check(L.gcow_encode_residual_device(C.byref(f), C.byref(p), e.data_ptr(), e2.data_ptr(),
                                              renc.words.data_ptr(), renc.cap, renc.bits_dev.data_ptr(),
                                              renc.ws.data_ptr(), renc.ws_bytes, renc.index.data_ptr(), 8, st), "b0")


def b_fitted():
    codec.check(L.gcow_encode_residual_fitted_device(C.byref(f), 64, word.data_ptr(), e.data_ptr(), e2.data_ptr(),
                                                     fenc.words.data_ptr(), fenc.cap, fenc.bits_dev.data_ptr(),
                                                     fenc.ws.data_ptr(), fenc.ws_bytes, fenc.index.data_ptr(), 8, st),
                "b1")


b = alternate({"encode_residual (host minexp)": b_host, "encode_residual_fitted (device word)": b_fitted})
torch.cuda.synchronize()
nw = (int(renc.bits_dev.item()) + 63) // 64
assert int(renc.bits_dev.item()) == int(fenc.bits_dev.item()) == bits
assert torch.equal(renc.words[:nw], fenc.words[:nw])  # the same stream from both
report("b_encode", b)
del e2

# ---- c: the whole step, e carried in place; each leg on its own copy of e, reset before every window
y = torch.empty_like(x)
ec = {"host read": torch.empty_like(e), "on device": torch.empty_like(e)}
rty = codec.RateTable(N, torch.float32, dev)
rec = codec.new_fit_record(dev)
encs = {}  # the host form needs one encoder per fitted set: cached, as DeviceCodec caches them
fre = codec.FittedResidualEncoder(N, torch.float32, BPV, device=dev, index_stride=8)


def c_host():
    err = ec["host read"]
    torch.add(x, err, out=y)
    codec.fit_device(rty(y), budget, rec)
    m = codec.read_fit(rec)[0]  # the host read
    if m not in encs:
        encs[m] = codec.ResidualEncoder(N, torch.float32, codec.fitted_params(64, m), dev, index_stride=8)
    encs[m](x, err)


def c_device():
    fre(x, ec["on device"])


c = alternate({"host read": c_host, "on device": c_device}, before=lambda k: ec[k].copy_(e))
report("c_step", c, host_form_encoders=len(encs))
