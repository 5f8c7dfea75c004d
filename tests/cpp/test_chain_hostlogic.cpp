// test_chain_hostlogic.cpp — chain_core.hpp's window bookkeeping with no device: the plan of a call against the protocol stated
// one filter block at a time, with no closed form and no division (counts by repeated addition), swept exhaustively over small
// shapes; the receiver's A(k) and stage-2 split against a two-stage walk of the same kind.  tests/test_chain_plan_cpu.py builds it
// with the host sanitizers and runs it as
//   test_chain_hostlogic                                             the sweeps -> "chain hostlogic ok"
//   test_chain_hostlogic plan S I D lag front n1 pend in_len out_cap max_blocks
//       -> "status need early k n_y consumed new_pend produced o_old r_lo r_hi next_block_outputs"
//   test_chain_hostlogic audio S1 I1 D1 lag1 S2 I2 D2 kmax           -> A(0) ... A(kmax)
// (the test holds the last two against Python integers and tests/receiver_model.py)
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>

#include "chain_core.hpp"

using namespace rr;

static int fails = 0;
#define CHECK(c) do { if (!(c)) { if (fails++ < 20) fprintf(stderr, "line %d: %s\n", __LINE__, #c); } } while (0)

static const uint64_t UNLIMITED = ~(uint64_t)0;

// ceil(y I / D) while y grows: r is the smallest count with r D >= y I, both products kept by addition
struct Counter {
    uint64_t I, D, y = 0, yI = 0, r = 0, rD = 0;
    Counter(uint64_t i, uint64_t d) : I(i), D(d) {}
    void add(uint64_t n) {
        for (uint64_t j = 0; j < n; j++) { y++; yI += I; }
        while (rD < yI) { r++; rD += D; }
    }
    uint64_t after(uint64_t n) const { Counter c = *this; c.add(n); return c.r; }
};
static uint64_t lagged(uint64_t r, uint64_t lag) { return r > lag ? r - lag : 0; }

// the protocol, one block at a time: `w` stands behind the filtered samples so far and moves on with the blocks taken
struct Truth { int status; uint64_t need; bool early; uint64_t k, consumed, new_pend, produced; };
static Truth one_call(const ChainShape& c, Counter& w, uint64_t pend, uint64_t in_len, uint64_t out_cap, uint64_t max_blocks) {
    auto next_outputs = [&]() { return lagged(w.after(c.S), c.lag) - lagged(w.r, c.lag); };
    Truth t{0, 0, true, 0, 0, pend, 0};
    if (next_outputs() > out_cap) { t.status = CHAIN_WAIT_DST; t.need = next_outputs(); return t; }
    if (c.front && in_len < c.front + 1) { t.status = CHAIN_WAIT_SRC; t.need = c.front + 1; return t; }
    t.early = false;
    const uint64_t av = in_len - c.front;                 // the front FIR's last samples stay in the window
    uint64_t have = pend + av, room = out_cap;
    while (have >= c.S && next_outputs() <= room && t.k < max_blocks) {
        room -= next_outputs();
        have -= c.S;
        w.add(c.S);
        t.k++;
    }
    t.produced = out_cap - room;
    if (have >= c.S) {                                    // a full block is left where it is: room or the limit ran out first
        t.status = CHAIN_WAIT_DST; t.need = next_outputs();
        t.consumed = av - have; t.new_pend = 0;           // (what is left was all in the window: have - pend < S would have run)
    } else {                                              // input ran out: everything joins the pending samples
        t.status = CHAIN_WAIT_SRC; t.need = c.S - have + c.front;
        t.consumed = av; t.new_pend = have;
    }
    return t;
}

static uint64_t rng_state = 0x9E3779B97F4A7C15ull;        // the committed seed
static uint64_t rnd(uint64_t n) {                         // xorshift64*, [0, n)
    rng_state ^= rng_state >> 12; rng_state ^= rng_state << 25; rng_state ^= rng_state >> 27;
    return ((rng_state * 0x2545F4914F6CDD1Dull) >> 33) % n;
}
static uint64_t gcd(uint64_t a, uint64_t b) { while (b) { const uint64_t t = a % b; a = b; b = t; } return a; }

static long n_calls = 0, n_early = 0, n_dst = 0, n_src = 0, n_tie = 0;

// one stream of n samples through windows and output rooms drawn from the seed; first: 0 drawn, 1 one block exactly into
// exactly the next block's outputs, 2 the same into one output less
static void walk_stream(const ChainShape& c, uint64_t max_blocks, uint64_t n, int first) {
    Counter w((uint64_t)c.I, (uint64_t)c.D);
    uint64_t n1 = 0, pend = 0, pos = 0, blocks = 0, produced = 0;
    for (int call = 0; call < 4000; call++) {
        const uint64_t left = n - pos, nb = chain_next_block_outputs(c, n1), one_block = c.S - pend + c.front;
        CHECK(nb == lagged(w.after(c.S), c.lag) - lagged(w.r, c.lag));
        uint64_t in_len, out_cap;
        const uint64_t di = rnd(100), dr = rnd(100);
        if (di < 3) in_len = 0;                           // (with a front FIR this and the next are the early WAIT_SRC)
        else if (di < 5) in_len = c.front;
        else if (di < 12) in_len = c.front + 1;
        else if (di < 30) in_len = one_block;
        else if (di < 40) in_len = one_block - 1 > c.front ? one_block - 1 : one_block;
        else in_len = c.front + 1 + rnd(4 * c.S + 1);
        if (dr < 4) out_cap = nb ? nb - 1 : 0;            // (early WAIT_DST unless the block makes nothing)
        else if (dr < 25) out_cap = nb;
        else if (dr < 30) out_cap = nb + 1;
        else if (dr < 90) out_cap = nb + rnd(4 * nb + 3);
        else out_cap = (uint64_t)1 << 32;
        if (call == 0 && first) { in_len = one_block; out_cap = first == 1 ? nb : (nb ? nb - 1 : 0); }
        const bool last = left <= c.front || call >= 3000;            // drain: whatever is left, all the room
        if (last) out_cap = (uint64_t)1 << 32;
        if (in_len > left || last) in_len = left;
        const ChainPlan p = chain_plan(c, n1, pend, in_len, out_cap, max_blocks);
        const uint64_t r0 = w.r;
        const Truth t = one_call(c, w, pend, in_len, out_cap, max_blocks);
        n_calls++; n_early += p.early; n_dst += !p.early && p.status == CHAIN_WAIT_DST; n_src += !p.early && p.status == CHAIN_WAIT_SRC;
        CHECK(p.status == t.status && p.need == t.need && p.early == t.early);
        CHECK(p.k == t.k && p.consumed == t.consumed && p.new_pend == t.new_pend && p.produced == t.produced);
        CHECK(p.n_y == p.k * c.S && p.o_old == lagged(r0, c.lag) && p.r_lo == r0 && p.r_hi == w.r);
        CHECK(p.consumed <= in_len && p.produced <= out_cap && p.new_pend < c.S && p.k <= max_blocks);
        if (p.early) CHECK(p.k == 0 && p.consumed == 0 && p.produced == 0 && p.new_pend == pend);
        // a tie: the input's last full block ran and the next one would not have fitted (>= in place of > would answer WAIT_DST)
        if (!p.early && p.status == CHAIN_WAIT_SRC && p.k && chain_emitted(c, n1 + p.n_y + c.S) - p.o_old > out_cap) n_tie++;
        n1 += p.n_y; pend = p.new_pend; pos += p.consumed; blocks += p.k; produced += p.produced;      // the plan's own state
        CHECK(w.y == n1);
        if (last && p.k == 0 && p.consumed == 0) break;
    }
    CHECK(n - pos == (n > c.front ? c.front : n));        // all of the stream but the front FIR's tail was taken in ...
    CHECK(blocks == pos / c.S && pend == pos % c.S);       // ... every whole block of it ran ...
    CHECK(produced == chain_emitted(c, blocks * c.S));     // ... and emitted what the chain emits after that many
}

static void sweep_plan() {
    const uint64_t fronts[3] = {0, 1, 4}, limits[3] = {1, 2, UNLIMITED};
    for (uint64_t S = 1; S <= 9; S++)
        for (int64_t I = 1; I <= 7; I++)
            for (int64_t D = 1; D <= 7; D++) {
                if (gcd((uint64_t)I, (uint64_t)D) != 1) continue;
                for (uint64_t lag = 0; lag <= 1; lag++)
                    for (uint64_t front : fronts)
                        for (uint64_t lim : limits)
                            for (int first = 0; first < 3; first++)
                                walk_stream(ChainShape{S, I, D, lag, front}, lim, 200 + rnd(200), first);
            }
}

// the receiver: RF blocks one at a time into the audio stage, which runs a block whenever it holds one
static void walk_receiver(const ChainShape& rf, const ChainShape& au, int nblocks) {
    Counter w1((uint64_t)rf.I, (uint64_t)rf.D), w2((uint64_t)au.I, (uint64_t)au.D);
    uint64_t held = 0;                                    // demodulated samples the audio stage holds (block at a time: < S2)
    uint64_t n1 = 0, pend = 0, d_call = 0, a_call = 0;    // the split's own state, and the counts at the last call's end
    for (int k = 0; k <= nblocks; k++) {
        CHECK(receiver_audio_after(rf, au, (uint64_t)k) == w2.r);
        if (k && (rnd(3) == 0 || k == nblocks)) {          // a call ends here: its stage 2 takes everything since the last one
            const uint64_t d = lagged(w1.r, rf.lag);
            const ReceiverSplit sp = receiver_split(au, n1, pend, d - d_call);
            CHECK(sp.total == pend + (d - d_call) && sp.n_y == sp.k2 * au.S && sp.new_pend == held && sp.new_pend < au.S);
            CHECK(sp.r_lo == a_call && sp.r_hi == w2.r && n1 + sp.n_y == w2.y);
            n1 += sp.n_y; pend = sp.new_pend; d_call = d; a_call = w2.r;
        }
        const uint64_t d0 = lagged(w1.r, rf.lag);
        w1.add(rf.S);
        held += lagged(w1.r, rf.lag) - d0;
        while (held >= au.S) { held -= au.S; w2.add(au.S); }
    }
}

static void sweep_receiver() {
    const int64_t ratios[6][2] = {{1, 1}, {1, 6}, {3, 2}, {2, 5}, {7, 4}, {3, 7}};
    for (uint64_t S1 = 1; S1 <= 7; S1++)
        for (uint64_t S2 = 1; S2 <= 6; S2++)
            for (auto& a : ratios)
                for (auto& b : ratios)
                    for (uint64_t lag = 0; lag <= 1; lag++)
                        walk_receiver(ChainShape{S1, a[0], a[1], lag, 0}, ChainShape{S2, b[0], b[1], 0, 0}, 60);
}

static uint64_t num(const char* s) { return strtoull(s, nullptr, 10); }

int main(int argc, char** argv) {
    if (argc == 12 && !strcmp(argv[1], "plan")) {
        const ChainShape c{num(argv[2]), (int64_t)num(argv[3]), (int64_t)num(argv[4]), num(argv[5]), num(argv[6])};
        const ChainPlan p = chain_plan(c, num(argv[7]), num(argv[8]), num(argv[9]), num(argv[10]), num(argv[11]));
        printf("%d %llu %d %llu %llu %llu %llu %llu %llu %llu %llu %llu\n", p.status, (unsigned long long)p.need, (int)p.early,
               (unsigned long long)p.k, (unsigned long long)p.n_y, (unsigned long long)p.consumed, (unsigned long long)p.new_pend,
               (unsigned long long)p.produced, (unsigned long long)p.o_old, (unsigned long long)p.r_lo, (unsigned long long)p.r_hi,
               (unsigned long long)chain_next_block_outputs(c, num(argv[7])));
        return 0;
    }
    if (argc == 10 && !strcmp(argv[1], "audio")) {
        const ChainShape rf{num(argv[2]), (int64_t)num(argv[3]), (int64_t)num(argv[4]), num(argv[5]), 0};
        const ChainShape au{num(argv[6]), (int64_t)num(argv[7]), (int64_t)num(argv[8]), 0, 0};
        for (uint64_t k = 0; k <= num(argv[9]); k++) printf("%llu ", (unsigned long long)receiver_audio_after(rf, au, k));
        printf("\n");
        return 0;
    }
    if (argc != 1) { fprintf(stderr, "usage: see the head of tests/cpp/test_chain_hostlogic.cpp\n"); return 2; }
    sweep_plan();
    sweep_receiver();
    // the body of the plan is what the sweep is about: at most one call in ten may end in an early return; both early answers
    // apart, both waits and the tie between them must have been seen
    printf("%ld calls: %ld early (%.1f %%), behind them %ld WAIT_SRC with %ld ties, %ld WAIT_DST\n", n_calls, n_early,
           100.0 * (double)n_early / (double)n_calls, n_src, n_tie, n_dst);
    CHECK(n_early * 10 <= n_calls);
    CHECK(n_early > 0 && n_src > 0 && n_dst > 0 && n_tie > 0);
    if (fails) { fprintf(stderr, "%d checks failed\n", fails); return 1; }
    printf("chain hostlogic ok\n");
    return 0;
}
