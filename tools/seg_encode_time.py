#!/usr/bin/env python3
"""The segmented codec (a minexp per tensor on the wire) on the ResNet-50-shaped fp32 bucket -- 161
tensors, 25.6 M values, each tensor at a scale of its own, the tensors back to back in one buffer -- at a budget of
--bpv bits per value (default 8). One process, device events, every compared form warmed up and the baseline timed
before and after the new form (tools/mean_encode_time.py's protocol: "cold" = 5 untimed + 20 timed launches, "steady"
= 50 launches after 0.25 s of back-to-back launches). One JSON line per measurement:

  a  encode_segmented under the fitted records against the chain of 161 codec.encode_append calls under the same
     words (the only way to this stream without the segmented encoder); both must leave the same stream;
  b  encode_segmented against the fitted encode of the same bucket under ONE minexp, chosen from the bucket's own rate
     table for the nearest stream length not above the segmented one: what the per-block lookup and the mixed tiles cost;
  c  decode_mean_segmented at W = 8 against decode_mean over 8 one-minexp streams of the same bucket, 16-block index;
  d  the PerTensorFittedEncoder chain (tables, batch fit, segmented encode) against the one-budget FittedEncoder, eager
     and as a captured graph.
usage: seg_encode_time.py [--bpv 8] [--world 8] [--only a|b|c|d]"""
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
    bpv, world, only = arg("--bpv", 8.0), arg("--world", 8), arg("--only", "")
    counts = resnet50_counts()
    n, S = sum(counts), len(counts)
    x = bucket(counts, 0x67636F77)
    pte = codec.PerTensorFittedEncoder(bpv)
    e, fits = pte(x, counts, 16, stream=st)
    torch.cuda.synchronize()
    seg_bits = e.bits
    seg = pte.enc
    recs = [codec.read_fit(fits[s]) for s in range(S)]
    shape = {"values": n, "tensors": S, "bpv": bpv, "segmented_bits": seg_bits,
             "tiles": int(seg.plan.stats().tiles), "uniform_tiles": int(seg.plan.stats().uniform_tiles)}

    def seg_encode():
        seg(x, fits, st)

    if only in ("", "a"):
        words = torch.zeros(seg.words.numel() + 4, dtype=torch.int64, device="cuda")
        bits = torch.zeros(S + 1, dtype=torch.int64, device="cuda")
        views = list(torch.split(x, counts))
        params = [codec.fitted_params(64, r[0]) for r in recs]
        ws = torch.empty(max(seg.ws.numel(), 1 << 16), dtype=torch.int64, device="cuda")

        def chain():
            for s in range(S):
                codec.encode_append(views[s], params[s], words, bits[s:s + 1], bits[s + 1:s + 2], ws=ws, stream=st)

        chain()
        seg_encode()
        torch.cuda.synchronize()
        nw = (seg_bits + 63) // 64
        same = bool(int(bits[-1]) == seg_bits and torch.equal(words[:nw], seg.words[:nw]))
        compare("a_segmented_vs_append_chain", chain, seg_encode, dict(shape, same_stream=same))

    # one minexp for the nearest stream length not above the segmented one
    table = codec.rate_table(x, 64, st)
    me, one_bits = codec.fit_minexp(table, seg_bits)
    word = torch.tensor([me], dtype=torch.int32, device="cuda")
    one = codec.Encoder((n,), torch.float32, codec.fitted_params(64, me), "cuda", 16)

    def one_encode():
        codec._encode_fitted_into(one, x, word, st)

    if only in ("", "b"):
        compare("b_segmented_vs_one_minexp", one_encode, seg_encode, dict(shape, one_minexp=me, one_bits=one_bits))

    if only in ("", "c"):
        p1 = codec.fitted_params(64, me)
        budget = sum(int(math.floor(bpv * c)) for c in counts)  # every fitted stream is within it
        sw = (int(1.1 * budget) // 64 + 4) // 2 * 2
        ni, nib = seg.index.numel(), one.index.numel()
        a_words = torch.zeros(world * sw + 2, dtype=torch.int64, device="cuda")
        b_words = torch.zeros(world * sw + 2, dtype=torch.int64, device="cuda")
        a_idx = torch.zeros(world * ni, dtype=torch.int64, device="cuda")
        b_idx = torch.zeros(world * nib, dtype=torch.int64, device="cuda")
        all_fits = torch.zeros((world, S, 2), dtype=torch.int64, device="cuda")
        for r in range(world):
            xr = bucket(counts, 0x67636F77 + r)
            er, fr = pte(xr, counts, 16, stream=st)
            torch.cuda.synchronize()
            nw = (er.bits + 63) // 64
            a_words[r * sw:r * sw + nw] = er.words[:nw]
            a_idx[r * ni:(r + 1) * ni] = er.index
            all_fits[r] = fr
            eo = codec._encode_fitted_into(one, xr, word, st)
            torch.cuda.synchronize()
            nw = (eo.bits + 63) // 64
            b_words[r * sw:r * sw + nw] = eo.words[:nw]
            assert nw <= sw
            b_idx[r * nib:(r + 1) * nib] = eo.index
            del xr
        out = torch.empty(n, dtype=torch.float32, device="cuda")
        plan = seg.plan

        def seg_mean():
            codec.decode_mean_segmented(a_words, sw, world, counts, all_fits, 64, a_idx, ni, 16, out=out, stream=st,
                                        plan=plan)

        def one_mean():
            codec.decode_mean(b_words, sw, world, n, p1, b_idx, nib, 16, out=out, stream=st)

        compare("c_decode_mean_segmented_vs_decode_mean", one_mean, seg_mean, dict(shape, world=world))

    if only in ("", "d"):
        fe = codec.FittedEncoder(n, torch.float32, bpv, 64, "cuda", 16)

        def pt_eager():
            pte(x, counts, 16, stream=st)

        def one_eager():
            fe(x, st)

        pt_eager()
        one_eager()
        torch.cuda.synchronize()
        compare("d_per_tensor_chain_vs_fitted_encoder_eager", one_eager, pt_eager, shape)
        side = torch.cuda.Stream()
        graphs = []
        for fn in (lambda: pte(x, counts, 16, stream=side), lambda: fe(x, side)):
            side.wait_stream(st)
            with torch.cuda.stream(side):
                fn()
            side.synchronize()
            g = torch.cuda.CUDAGraph()
            with torch.cuda.graph(g, stream=side):
                fn()
            graphs.append(g)
        torch.cuda.synchronize()
        compare("d_per_tensor_chain_vs_fitted_encoder_graph", graphs[1].replay, graphs[0].replay, shape)


main()
