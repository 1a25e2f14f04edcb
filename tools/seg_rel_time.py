#!/usr/bin/env python3
"""The words pass of a relative tolerance on the wire (gcow_seg_rel_minexp_device) on the
ResNet-50-shaped bucket -- 161 tensors, 25.6 M values, each tensor at a scale of its own, the tensors back to back in
one buffer -- as fp32 and as bf16, at --rel-bits (default 8) against a budget of --bpv bits per value (default 8) for
the per-tensor-budget chains. One process, device events, every compared form warmed up and the baseline timed before
and after the new form (tools/seg_encode_time.py's protocol: "cold" = 5 untimed + 20 timed launches, "steady" = 50
launches after 0.25 s of back-to-back launches). One JSON line per measurement and dtype:

  a  the words pass against gcow_rate_table_seg_device on the same buffers, without and with a carried error;
  b  the chain words -> segmented encode (PerTensorRelativeEncoder) against the per-tensor-budget chain tables -> fit ->
     segmented encode (PerTensorFittedEncoder), eager and as captured graphs;
  c  the residual chains likewise (PerTensorRelativeResidualEncoder against PerTensorFittedResidualEncoder; the carried
     error is restored before every launch by a copy that both sides pay, so the figures are copy + chain; the copy is
     timed alone first, in a line of its own, to be subtracted).
usage: seg_rel_time.py [--rel-bits 8] [--bpv 8] [--only a|b|c] [--dtype fp32|bf16]"""
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


def bucket(counts, seed, dtype):
    n = sum(counts)
    x = torch.empty(n, dtype=torch.float32, device="cuda")
    codec.fill_normal(x, 1e-3, seed=seed, inject=False)
    o = 0
    for s, c in enumerate(counts):  # every tensor at a scale of its own, 2^-9 .. 2^3 around the fill's 1e-3
        x[o:o + c] *= 2.0 ** ((s * 7) % 13 - 9)
        o += c
    return x.to(dtype)


def graphs_of(fns):
    side = torch.cuda.Stream()
    out = []
    for fn in fns:
        side.wait_stream(st)
        with torch.cuda.stream(side):
            fn(side)
        side.synchronize()
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g, stream=side):
            fn(side)
        out.append(g)
    torch.cuda.synchronize()
    return out


def run(dtype, name, k, bpv, only):
    counts = resnet50_counts()
    n, S = sum(counts), len(counts)
    x = bucket(counts, 0x67636F77, dtype)
    e0 = torch.empty(n, dtype=torch.float32, device="cuda")
    codec.fill_normal(e0, 1e-5, seed=0x6572726F, inject=False)
    err = e0.clone()
    plan = codec.SegmentPlan(counts, dtype, "cuda")
    shape = {"dtype": name, "values": n, "tensors": S, "rel_bits": k, "bpv": bpv, "tiles": int(plan.stats().tiles),
             "uniform_tiles": int(plan.stats().uniform_tiles)}

    if only in ("", "a"):
        tab = codec.SegmentedRateTables(counts, dtype, 64, "cuda", plan)
        absmax = torch.zeros(S, dtype=torch.float32, device="cuda")
        words = torch.zeros(S, dtype=torch.int32, device="cuda")
        for what, e in (("a_words_vs_rate_tables", None), ("a_words_vs_rate_tables_with_error", err)):
            compare(what, lambda: tab(x, e, st),
                    lambda: codec.relative_minexp_segmented(x, counts, k, e, absmax, words, plan, st), shape)

    if only in ("", "b"):
        rel, fit = codec.PerTensorRelativeEncoder(k), codec.PerTensorFittedEncoder(bpv)
        er, _ = rel(x, counts, 16, stream=st)
        ef, _ = fit(x, counts, 16, stream=st)
        torch.cuda.synchronize()
        extra = dict(shape, relative_bits_out=er.bits, fitted_bits_out=ef.bits)
        compare("b_relative_chain_vs_budget_chain_eager", lambda: fit(x, counts, 16, stream=st),
                lambda: rel(x, counts, 16, stream=st), extra)
        gr, gf = graphs_of([lambda s: rel(x, counts, 16, stream=s), lambda s: fit(x, counts, 16, stream=s)])
        compare("b_relative_chain_vs_budget_chain_graph", gf.replay, gr.replay, extra)

    if only in ("", "c"):
        rel, fit = codec.PerTensorRelativeResidualEncoder(k), codec.PerTensorFittedResidualEncoder(bpv)

        def rel_step(s):
            err.copy_(e0)
            rel(x, err, counts, 16, stream=s)

        def fit_step(s):
            err.copy_(e0)
            fit(x, err, counts, 16, stream=s)

        rel_step(st)
        fit_step(st)
        torch.cuda.synchronize()
        # what both sides of (c) pay before the chain: the chain times are the figures below minus this
        print(json.dumps(dict(shape, measurement="c_error_restore_copy_alone", copy=leg(lambda: err.copy_(e0)))),
              flush=True)
        compare("c_relative_residual_chain_vs_budget_residual_chain_eager", lambda: fit_step(st), lambda: rel_step(st),
                shape)
        gr, gf = graphs_of([rel_step, fit_step])
        compare("c_relative_residual_chain_vs_budget_residual_chain_graph", gf.replay, gr.replay, shape)


def main():
    k, bpv, only, which = arg("--rel-bits", 8), arg("--bpv", 8.0), arg("--only", ""), arg("--dtype", "")
    for name, dtype in (("fp32", torch.float32), ("bf16", torch.bfloat16)):
        if which in ("", name):
            run(dtype, name, k, bpv, only)


main()
