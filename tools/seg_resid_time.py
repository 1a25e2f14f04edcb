#!/usr/bin/env python3
"""Error feedback under per-tensor budgets on the ResNet-50-shaped fp32 bucket of
tools/seg_encode_time.py -- 161 tensors, 25.6 M values, each tensor at a scale of its own -- at --bpv bits per value
(default 8), with a carried error e: the residual one fitted step leaves. That tool's protocol: one process, device
events, every compared form warmed up, the baseline timed before and after the new form ("cold" = 5 untimed + 20 timed
launches, "steady" = 50 launches after 0.25 s of back-to-back launches). One JSON line per measurement:

  a1 encode_segmented_residual (x, e -> stream, e' to a second buffer) against encode_segmented under the same records;
  a2 the same against encode_residual_fitted_device of the bucket under ONE minexp (the nearest stream length not above
     the segmented one): the unsegmented residual tile form;
  b1 rate_tables_segmented with e against TensorListFittedPerTensor.rate_tables on x alone;
  b2 rate_tables_segmented with e None against the same call;
  c  the PerTensorFittedResidualEncoder chain against the PerTensorFittedEncoder chain, eager and as captured graphs.
usage: seg_resid_time.py [--bpv 8] [--only a|b|c]"""
import json
import math
import os
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from gcow_amd import codec  # noqa: E402


def arg(name, default):
    return type(default)(sys.argv[sys.argv.index(name) + 1]) if name in sys.argv else default


def resnet50_counts():
    """The parameter sizes of ResNet-50 in module order (tools/roundtrip_time.py resnet50_shapes)."""
    shapes = [(64, 3, 7, 7), (64,), (64,)]
    inplanes = 64
    for planes, blocks in ((64, 3), (128, 4), (256, 6), (512, 3)):
        for b in range(blocks):
            shapes += [(planes, inplanes, 1, 1), (planes,), (planes,), (planes, planes, 3, 3), (planes,), (planes,),
                       (4 * planes, planes, 1, 1), (4 * planes,), (4 * planes,)]
            if b == 0:
                shapes += [(4 * planes, inplanes, 1, 1), (4 * planes,), (4 * planes,)]
            inplanes = 4 * planes
    return [math.prod(s) for s in shapes + [(1000, 2048), (1000,)]]


st = torch.cuda.current_stream()


def timed(fn, warm, steps):
    for _ in range(warm):
        fn()
    torch.cuda.synchronize()
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(steps + 1)]
    ev[0].record(st)
    for i in range(steps):
        fn()
        ev[i + 1].record(st)
    torch.cuda.synchronize()
    per = [ev[i].elapsed_time(ev[i + 1]) for i in range(steps)]
    return sum(per) / len(per)


def leg(fn):
    cold = timed(fn, 5, 20)
    t0 = time.perf_counter()
    while time.perf_counter() - t0 < 0.25:
        for _ in range(10):
            fn()
        torch.cuda.synchronize()
    return {"cold_ms": round(cold, 4), "steady_ms": round(timed(fn, 0, 50), 4)}


def compare(name, base, new, extra):
    """base, new, base again -> one JSON line with the ratio base / new against the faster base run."""
    t0 = time.perf_counter()
    while time.perf_counter() - t0 < 0.25:  # the clock ramp after the setup's idle time stays out of the first leg
        base()
        torch.cuda.synchronize()
    res = dict(extra, measurement=name)
    res["base_before"] = leg(base)
    res["new"] = leg(new)
    res["base_after"] = leg(base)
    for k in ("cold_ms", "steady_ms"):
        b = min(res["base_before"][k], res["base_after"][k])
        res["base_over_new_" + k] = round(b / res["new"][k], 3)
    print(json.dumps(res), flush=True)


def bucket(counts, seed):
    n = sum(counts)
    x = torch.empty(n, dtype=torch.float32, device="cuda")
    codec.fill_normal(x, 1e-3, seed=seed, inject=False)
    o = 0
    for s, c in enumerate(counts):  # every tensor at a scale of its own, 2^-9 .. 2^3 around the fill's 1e-3
        x[o:o + c] *= 2.0 ** ((s * 7) % 13 - 9)
        o += c
    return x


def main():
    bpv, only = arg("--bpv", 8.0), arg("--only", "")
    counts = resnet50_counts()
    n, S = sum(counts), len(counts)
    x = bucket(counts, 0x67636F77)
    pte = codec.PerTensorFittedEncoder(bpv)
    ptr = codec.PerTensorFittedResidualEncoder(bpv)
    err = torch.zeros(n, dtype=torch.float32, device="cuda")
    ptr(x, err, counts, 16, stream=st)  # err: one step's residual, the carried error of everything below
    torch.cuda.synchronize()
    e0 = err.clone()
    e_out = torch.empty_like(err)
    e, fits = ptr(x, err, counts, 16, stream=st)
    torch.cuda.synchronize()
    fits = fits.clone()
    err.copy_(e0)
    seg_bits = e.bits
    shape = {"values": n, "tensors": S, "bpv": bpv, "segmented_residual_bits": seg_bits,
             "tiles": int(ptr.enc.plan.stats().tiles), "uniform_tiles": int(ptr.enc.plan.stats().uniform_tiles)}
    plain = codec.SegmentedEncoder(counts, torch.float32, 64, "cuda", 16, plan=ptr.enc.plan)

    def seg_resid():
        ptr.enc(x, e0, fits, e_out, st)

    def seg_plain():
        plain(x, fits, st)

    if only in ("", "a"):
        compare("a1_segmented_residual_vs_segmented", seg_plain, seg_resid, shape)
        y = x + e0
        table = codec.rate_table(y, 64, st)
        me, one_bits = codec.fit_minexp(table, seg_bits)
        word = torch.tensor([me], dtype=torch.int32, device="cuda")
        one = codec.Encoder((n,), torch.float32, codec.fitted_params(64, me), "cuda", 16)
        e_one = e0.clone()

        def one_resid():  # in place, as the call is made; the values it codes drift, its work does not
            codec._encode_residual_fitted_into(one, x, e_one, word, st)

        compare("a2_segmented_residual_vs_one_minexp_residual", one_resid, seg_resid,
                dict(shape, one_minexp=me, one_bits=one_bits))
        del y

    if only in ("", "b"):
        views = list(torch.split(x, counts))
        lst = pte.lst
        lst.rate_tables(views, st)
        tab = ptr.tab

        def rel_tables():
            lst.rate_tables(views, st)

        def seg_tables_e():
            tab(x, e0, st)

        def seg_tables():
            tab(x, None, st)

        seg_tables()
        torch.cuda.synchronize()
        same = bool(torch.equal(tab.tables, lst.tables))
        compare("b1_seg_tables_of_y_vs_rel_tables_of_x", rel_tables, seg_tables_e, shape)
        compare("b2_seg_tables_of_x_vs_rel_tables_of_x", rel_tables, seg_tables, dict(shape, same_tables=same))

    if only in ("", "c"):
        def resid_chain(s=st):
            ptr(x, err, counts, 16, stream=s)

        def plain_chain(s=st):
            pte(x, counts, 16, stream=s)

        resid_chain()
        plain_chain()
        torch.cuda.synchronize()
        compare("c_residual_chain_vs_per_tensor_chain_eager", plain_chain, resid_chain, shape)
        side = torch.cuda.Stream()
        graphs = []
        for fn in (resid_chain, plain_chain):
            side.wait_stream(st)
            with torch.cuda.stream(side):
                fn(side)
            side.synchronize()
            g = torch.cuda.CUDAGraph()
            with torch.cuda.graph(g, stream=side):
                fn(side)
            graphs.append(g)
        torch.cuda.synchronize()
        compare("c_residual_chain_vs_per_tensor_chain_graph", graphs[1].replay, graphs[0].replay, shape)


main()
