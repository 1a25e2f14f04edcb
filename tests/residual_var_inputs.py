"""TEST INFRASTRUCTURE ONLY -- shared inputs of the variable-rate error-feedback tests (test_residual_var_cpu.py,
test_gpu_residual_var.py): test_gpu_residual._inputs' bucket (a gradient-like x, a residual-scale e, the crafted
blocks: subnormal, NaN, +-Inf, overflowing x + e, x = -e, wide / sparse / constant / alternating blocks), and in
addition, for buckets of three tiles or more, every odd tile of 4096 values of x multiplied by 2^20 (exact in fp32 and
bf16): those tiles' codes exceed the tile coder's 1500-qword LDS window at accuracy 1e-3 and go to its _big kernel,
while the even tiles stay in the main one. The reference of every comparison is residual_model.model_step."""
import functools

import numpy as np

TILE = 4096           # values per tile of the variable-rate encoder (1024 blocks)
WINDOW_BITS = 1500 * 64

MODES = {
    "acc1e-3": lambda O: O.accuracy(1e-3),
    "acc1e-6": lambda O: O.accuracy(1e-6),
    "prec12": lambda O: O.precision(12),
    "prec32": lambda O: O.precision(32),
    "expert_nobudget": lambda O: O.expert(1, 4096, 24, -40),
    "expert_budget": lambda O: O.expert(1, 100, 32, -1074),   # maxbits < 160: the composed path
}


def bf16_bits(a):
    return (a.view(np.uint32) >> 16).astype(np.uint16)


def scale_odd_tiles(x):
    """x (float32, or bf16 bits) with every odd tile times 2^20, for n >= 3 tiles; otherwise x itself."""
    from residual_model import widen
    n = x.size
    if n < 3 * TILE:
        return x
    f = widen(x).copy()
    with np.errstate(over="ignore", invalid="ignore"):
        for t0 in range(TILE, n, 2 * TILE):
            f[t0:t0 + TILE] *= np.float32(2.0 ** 20)
    return bf16_bits(f) if x.dtype == np.uint16 else f


def inputs(n, bf16, op):
    from test_gpu_residual import _inputs
    x, e = _inputs(n, bf16, op)
    return scale_odd_tiles(x), e


@functools.lru_cache(maxsize=None)
def case(n, bf16, mode):
    """Inputs and the model's three chained steps, computed once per case and shared (read-only)."""
    from oracle import oracle as O
    from residual_model import model_step
    op = MODES[mode](O)
    x0, e0 = inputs(n, bf16, op)
    xs = [x0]
    for t in (1, 2):
        a = O.gen_normal(n, 1e-3, 600 + t, True)
        xs.append(scale_odd_tiles(bf16_bits(a) if bf16 else a))
    steps = []
    e = e0
    for x in xs:
        y, w, bits, d, e = model_step(x, e, op)
        steps.append((w, bits, e, y, d))
    null = model_step(x0, None, op)
    for a in xs + [e0] + [a for s in steps for a in (s[0], s[2], s[3], s[4])]:
        a.setflags(write=False)
    return {"op": op, "xs": xs, "e0": e0, "steps": steps, "null": (null[1], null[2], null[4])}
