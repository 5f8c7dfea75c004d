"""Test-side statement of the fused chains' window bookkeeping (rustradio_amd/csrc/chain_core.hpp) in Python integers, and of
work() of a chain with an output tail on top of it (blocks.hpp trickle_work), from lengths alone.  Nothing here touches the GPU
library: tests/test_chain_plan_cpu.py holds the C++ plan to plan(), tests/test_gpu_parity.py holds rr.FirFmChain to ChainModel."""
from collections import namedtuple
from math import gcd

from harness import AGAIN, WAIT_DST, WAIT_SRC

UNLIMITED = (1 << 64) - 1
Plan = namedtuple("Plan", "status need early k n_y consumed new_pend produced o_old r_lo r_hi next_block_outputs")


def resampled(y, I, D):
    return -(-y * I // D)


def emitted(y, I, D, lag):
    return max(resampled(y, I, D) - lag, 0)


def plan(S, I, D, lag, front, n1, pend, in_len, out_cap, max_blocks):
    """one call, I : D reduced.  The blocks the room takes are found from the definition by bisection (emitted is monotone), not
    from a bound in closed form."""
    o_old, r_lo = emitted(n1, I, D, lag), resampled(n1, I, D)
    nb = emitted(n1 + S, I, D, lag) - o_old
    if nb > out_cap:
        return Plan(WAIT_DST, nb, 1, 0, 0, 0, pend, 0, o_old, r_lo, r_lo, nb)
    if front and in_len < front + 1:
        return Plan(WAIT_SRC, front + 1, 1, 0, 0, 0, pend, 0, o_old, r_lo, r_lo, nb)
    fits = lambda k: emitted(n1 + k * S, I, D, lag) - o_old <= out_cap
    lo, hi = 1, 2                                                       # fits(lo), and some hi that does not
    while fits(hi):
        lo, hi = hi, 2 * hi
    while hi - lo > 1:
        mid = (lo + hi) // 2
        lo, hi = (mid, hi) if fits(mid) else (lo, mid)
    k_out = min(lo, max_blocks)
    av = in_len - front
    k_in = (pend + av) // S
    if k_in > k_out:
        k, consumed, new_pend, st = k_out, k_out * S - pend, 0, WAIT_DST
        need = emitted(n1 + (k + 1) * S, I, D, lag) - emitted(n1 + k * S, I, D, lag)
    else:
        k, consumed, new_pend, st = k_in, av, pend + av - k_in * S, WAIT_SRC
        need = S - new_pend + front
    n_y = k * S
    return Plan(st, need, 0, k, n_y, consumed, new_pend, emitted(n1 + n_y, I, D, lag) - o_old, o_old, r_lo, resampled(n1 + n_y, I, D), nb)


class ChainModel:
    """(status, consumed, produced, need) of every work() call of FmChain / FirFmChain / AudioChain / FmMulti: pending outputs of
    the tail first (WAIT_DST 1 while some remain), the plan when the window holds the next block's outputs, else ONE block
    through the tail"""

    def __init__(self, S, interp, deci, lag, front=0):
        g = gcd(interp, deci)
        self.shape = (S, interp // g, deci // g, lag, front)
        self.n1 = self.pend = self.tail = 0

    def next_block_outputs(self):
        S, I, D, lag, _ = self.shape
        return emitted(self.n1 + S, I, D, lag) - emitted(self.n1, I, D, lag)

    def _run(self, in_len, out_cap, max_blocks):
        p = plan(*self.shape, self.n1, self.pend, in_len, out_cap, max_blocks)
        self.n1, self.pend = self.n1 + p.n_y, p.new_pend
        return p

    def work(self, in_len, out_cap):
        produced, room = 0, out_cap
        if self.tail:
            produced = min(room, self.tail)
            self.tail -= produced
            room -= produced
            if self.tail:
                return (WAIT_DST, 0, produced, 1)
        nb = self.next_block_outputs()
        if nb <= room:
            p = self._run(in_len, room, UNLIMITED)
            return (p.status, p.consumed, produced + p.produced, p.need)
        p = self._run(in_len, nb, 1)
        if p.produced == 0:
            return (p.status, p.consumed, produced, p.need)
        m = min(room, p.produced)
        self.tail = p.produced - m
        return (WAIT_DST if self.tail else AGAIN, p.consumed, produced + m, 1 if self.tail else 0)
