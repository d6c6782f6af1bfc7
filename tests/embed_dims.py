"""Embedding sizes shared by tests/test_embed_dims_gpu.py and its CPU companions.

D selects code on the 1:N side (csrc/match.hip: one_term_fits / g1_dims / one_term_frag, the copy addressing, the width
of the key-error band) and it alone shapes NumPy's pairwise-summation tree that the device restates (match_ref.hpp:
SumPlan).  The lists below name one size per class, so that every file tests the same ones."""
import numpy as np

# dif_pairwise: every plan shape.  1..300 = n < 8, the 8-wide body with 0..7 tail terms, the first splits (129, 257).
PAIR_SMALL = tuple(range(1, 301))
PAIR_LARGE = (1000, 1023, 1025, 2047, 4104, 7688, 8000, 8192)
# sizes of [7689, 8191] whose NumPy tree has 65 leaves (441 of the 503 have; tests/test_oracle_golden.py asserts it for
# these): one more than 8192 / 128, the count a power-of-two size gives and the capacity SumPlan had at first
PAIR_65 = (7689, 7690, 7695, 7703, 7777, 7750, 7801, 7919, 8001, 8100, 8185, 8190, 8191)
PAIR_ROWS = 64

# (B, G, D) of the gallery queries: the two-term filter at D % 64 != 0 (96, 160, 288), the one-term row-major filter
# at D % 64 == 0 outside {128, 256, 384, 512} (320, 640, 1024, 2048, 8192); B <= 32, <= 64 and > 64 are the three probe
# tile kinds; every G leaves a tile tail
QUERY_SHAPES = ((3, 129, 96), (65, 257, 160), (130, 1000, 288), (70, 515, 320), (33, 300, 640), (130, 1000, 1024),
                (65, 257, 2048), (5, 130, 8192))
TWO_TERM_DIMS = (96, 160, 288)


def pair_rows(d, n=PAIR_ROWS):
    """Rows scaled by factors in [0.1, 30] and a noisy copy of them (row 0 an exact copy): the generator of
    test_reference_arithmetic_bit_exact, seeded by the size."""
    rng = np.random.default_rng(5000 + d)
    a = (rng.standard_normal((n, d)) * rng.uniform(0.1, 30, (n, 1))).astype(np.float32)
    b = (a + 0.3 * rng.standard_normal((n, d))).astype(np.float32)
    b[0] = a[0]
    return a, b


def pairwise_plan(n):
    """NumPy's pairwise-summation tree over n elements, flattened as the device holds it (match_ref.hpp: SumPlan): the
    leaves (blocks of <= 128 summed by the eight accumulators) in order as [start, length, pops], `pops` = additions of
    the two topmost partial sums after that leaf.  oracle.distance.np_pairwise_sum's recursion without the arithmetic."""
    plan = []

    def rec(off, m):
        if m <= 128:
            plan.append([off, m, 0])
            return
        m2 = m // 2
        m2 -= m2 % 8
        rec(off, m2)
        rec(off + m2, m - m2)
        plan[-1][2] += 1

    rec(0, n)
    return plan


def plan_stack_depth(plan):
    """Most partial sums the stack machine holds at once while it runs `plan`."""
    sp = deepest = 0
    for _, _, pops in plan:
        sp += 1 - pops
        deepest = max(deepest, sp)
    assert sp == 1
    return deepest


def _leaf_sum(x):
    """A leaf as the device sums it, whatever its length (np_sum in match_ref.hpp): eight interleaved accumulators over the
    whole groups of eight, ((r0+r1)+(r2+r3))+((r4+r5)+(r6+r7)), then the rest in order; below eight a plain loop.  x [rows, n]
    float32, every operation a float32 one."""
    n = x.shape[1]
    body = n - n % 8
    if n < 8:
        res, body = np.zeros(x.shape[0], dtype=np.float32), 0
    else:
        r = x[:, :8].copy()
        for i in range(8, body, 8):
            r = r + x[:, i:i + 8]
        res = ((r[:, 0] + r[:, 1]) + (r[:, 2] + r[:, 3])) + ((r[:, 4] + r[:, 5]) + (r[:, 6] + r[:, 7]))
    for i in range(body, n):
        res = res + x[:, i]
    return res


def plan_sum(plan, x):
    """The float32 sums of the rows of x [rows, n] by that stack machine."""
    assert x.dtype == np.float32
    stack = []
    for start, length, pops in plan:
        top = _leaf_sum(x[:, start:start + length])
        for _ in range(pops):
            top = stack.pop() + top
        stack.append(top)
    assert len(stack) == 1 and stack[0].dtype == np.float32
    return stack[0]
