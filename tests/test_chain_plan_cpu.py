"""No GPU: the window bookkeeping of the fused chains (rustradio_amd/csrc/chain_core.hpp) under the host sanitizers
(tests/cpp/test_chain_hostlogic.cpp): the plan of a call against the protocol stated one filter block at a time, swept over small
shapes; the plan at ratios near 2^31 and positions near 2^40 against Python integers restating the definitions
(tests/chain_model.py); and the receiver's A(k) against tests/receiver_model.py for the shapes of tests/test_fm_receiver_cpu.py."""
import subprocess

import pytest

import fsk_model as fk
import receiver_model as rm
from chain_model import UNLIMITED, plan
from test_fm_receiver_cpu import PROTOCOL_SHAPES

SAN = ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-static-libasan", "-static-libubsan"]


@pytest.fixture(scope="module")
def hostlogic(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("chainhl") / "test_chain_hostlogic")
    fk.build_cpp("test_chain_hostlogic.cpp", exe, SAN)
    return exe


def test_plan_against_the_protocol_block_by_block(hostlogic):
    """the exhaustive sweep (S 1..9, coprime I : D up to 7, lag 0 / 1, front 0 / 1 / 4, block limits 1 / 2 / none) and the receiver's
    two-stage walk; the program fails by itself when more than one call in ten of the sweep ends in an early return"""
    r = subprocess.run([hostlogic], capture_output=True, text=True, timeout=600)
    print(r.stdout)
    assert r.returncode == 0 and "chain hostlogic ok" in r.stdout, r.stdout + r.stderr


P31, Q31 = 2147483647, 2147483629                                       # primes below 2^31
# (S, I, D, lag, front, n1, pend, in_len, out_cap, max_blocks): everything stays below 2^64, as it does behind the constructors'
# limits (ratio parts <= 2^31, stream positions far below 2^63 / 2^31)
BIG = [
    (561, 1, 6, 1, 0, 0, 0, 1000, 100, UNLIMITED),                      # the first call of the bench chain: the lag bites
    (561, 1, 6, 1, 0, 0, 0, 561, 93, UNLIMITED),                        # one block exactly into exactly its outputs: the tie
    (561, 1, 6, 1, 0, 0, 0, 1122, 92, UNLIMITED),                       # ... one output less: early
    (561, P31, Q31, 1, 0, (1 << 40) // 561 * 561, 17, 5 * 561, 1 << 32, UNLIMITED),
    (561, Q31, P31, 0, 0, (1 << 40) // 561 * 561, 560, 1, 1 << 32, UNLIMITED),
    (561, P31, Q31, 1, 0, (1 << 40) // 561 * 561, 0, 1 << 33, 1 << 32, UNLIMITED),   # room for 2^32 outputs runs out first
    (561, P31, Q31, 1, 0, (1 << 40) // 561 * 561, 0, 1 << 33, 1 << 32, 2),
    (623, 1 << 31, P31, 1, 126, (1 << 40) // 623 * 623, 100, 126, 1 << 32, UNLIMITED),   # below the front FIR's minimum
    (623, 1 << 31, P31, 1, 126, (1 << 40) // 623 * 623, 100, 127, 1 << 32, UNLIMITED),
    (623, P31, 1 << 31, 1, 126, (1 << 40) // 623 * 623, 622, 127 + 623, 623, 1),
    (7, 1, 1 << 31, 1, 0, (1 << 40) // 7 * 7, 3, 1000, 0, UNLIMITED),   # blocks that emit nothing need no room
    (7, 1, 1 << 31, 0, 0, (1 << 40) // 7 * 7, 3, 1000, 0, UNLIMITED),
    (7, 1, 1 << 31, 1, 0, ((1 << 31) - 5) // 7 * 7, 0, 1000, 0, UNLIMITED),         # ... until the one that crosses a multiple of D
    (1 << 20, 1, 1 << 31, 0, 4, (1 << 40), 5, (1 << 32), 1 << 32, UNLIMITED),
    (1, 1 << 31, 1, 1, 0, 1 << 20, 0, 9, 1 << 32, UNLIMITED),           # 2^31 outputs per sample: two blocks fit
    (1, 1 << 31, 1, 0, 0, 1 << 20, 0, 9, (1 << 32) - 1, UNLIMITED),     # ... one
    (3, 1 << 31, 1, 0, 0, 1 << 20, 0, 9, 1 << 32, UNLIMITED),           # ... none: early
    (4096, 1 << 31, Q31, 1, 0, (1 << 40), 4095, 1, 0, UNLIMITED),       # no room at all
    (4096, Q31, 1 << 31, 1, 1, (1 << 40), 4095, 2, 4096, 1),
    (9, 7, 3, 1, 4, 0, 0, 4 + 27, 62, UNLIMITED),                       # the first call with a front FIR: 3 blocks make 63 - 1
    (9, 7, 3, 1, 4, 0, 0, 4 + 27, 61, UNLIMITED),
]


@pytest.mark.parametrize("case", BIG, ids=[f"{i}-S{c[0]}-{c[1]}:{c[2]}" for i, c in enumerate(BIG)])
def test_plan_against_python_integers(hostlogic, case):
    r = subprocess.run([hostlogic, "plan", *map(str, case)], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0, r.stderr
    want = list(plan(*case))
    assert max(want) < 1 << 64 and case[5] + (want[3] + 1) * case[0] < 1 << 64       # the case itself fits the program's integers
    assert [int(v) for v in r.stdout.split()] == want, case


@pytest.mark.parametrize("L1,rf,L2,audio,fastfm,n", PROTOCOL_SHAPES)
def test_audio_after_against_the_receiver_model(hostlogic, L1, rf, L2, audio, fastfm, n):
    """receiver_audio_after(k), k = 0 ... 50, against ReceiverModel.A — the model test_fm_receiver_cpu.py holds to the oracle's six
    blocks (FastFM has no lag: the function takes the RF chain's lag like every other count)"""
    m = rm.ReceiverModel(L1, *rf, L2, *audio, fastfm=fastfm)
    args = (m.S1, m.I1, m.D1, 0 if fastfm else 1, m.S2, m.I2, m.D2, 50)
    r = subprocess.run([hostlogic, "audio", *map(str, args)], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0, r.stderr
    assert [int(v) for v in r.stdout.split()] == [m.A(k) for k in range(51)]
