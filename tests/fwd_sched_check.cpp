// Host-only check that what plan_fwd (fmha_launch.h) plans is what the forward kernels walk
// (the pure schedule functions of fmha_fwd_sched.h, which fwd_walk calls): every item exactly
// once, and the structure each schedule promises.  Built and run by tests/test_fwd_sched.py.
#include <cstdio>
#include <vector>

#include "fmha_launch.h"

using namespace xfa;

namespace {

struct Case { int nbh, nm, slots, order, ctr, xcdq; FwdQueue queue; };

int g_failures = 0;
#define CHECK(cond, c, what)                                                                              \
    do {                                                                                                  \
        if (!(cond)) {                                                                                    \
            if (g_failures++ < 20)                                                                        \
                std::printf("FAIL %s: nbh %d nm %d slots %d order %d ctr %d xcdq %d queue %d (%s)\n", what, \
                            (c).nbh, (c).nm, (c).slots, (c).order, (c).ctr, (c).xcdq, (int)(c).queue, #cond); \
            return;                                                                                       \
        }                                                                                                 \
    } while (0)

void run_case(const Case& c) {
    static int counters[10];
    FwdParams p{};
    p.b = c.nbh; p.hk = 1; p.h = 1; p.group = 1;
    p.seqlen_q = 256 * c.nm - 100;          // the last row block is partial
    p.num_cus = c.slots; p.persist_per_cu = 1;
    p.order = c.order; p.xcdq = c.xcdq;
    p.work_ctr = c.ctr ? counters : nullptr;
    const FwdPlan s = plan_fwd(p, 256, c.slots, 1, c.queue);
    const FwdParams& pp = s.pp;
    const int nbh = c.nbh, nm = pp.n_mblocks, g = (int)s.grid.x;
    CHECK(nm == c.nm, c, "row blocks");
    std::vector<int> seen(nbh * nm, 0);
    auto produce = [&](int bh, int m_block) {
        if (bh < 0 || bh >= nbh || m_block < 0 || m_block >= nm) return false;
        ++seen[bh * nm + m_block];
        return true;
    };
    if (pp.persistent == 0) {
        // one workgroup per item: fwd_walk maps block (x, y) to (x, grid.y - 1 - y)
        CHECK((int)s.grid.x == nbh && (int)s.grid.y == nm, c, "mode 0 grid");
        for (int x = 0; x < nbh; ++x)
            for (int y = 0; y < nm; ++y) produce(x, nm - 1 - y);
    } else if (pp.persistent == 1 || pp.persistent == 2) {
        CHECK(s.grid.y == 1 && g > 0, c, "persistent grid");
        for (int wg = 0; wg < g; ++wg) {
            int k = 0;
            for (;; ++k) {
                int bh = -1, mb = -1;
                const FwdStep st = pp.persistent == 2 ? fwd_pair_step(k, wg, g, nbh, nm, bh, mb)
                                                       : fwd_snake_step(k, wg, g, nbh, nm, bh, mb);
                if (st == kStepEnd) break;
                CHECK(k < 2 * nbh * nm + 2, c, "static walk ends");
                if (pp.persistent == 2) {
                    // pair i of a unit = row blocks (nm - 1 - i, i) at steps 2j and 2j + 1 of one
                    // workgroup; the middle block of an odd count comes once
                    int bh2 = -1, mb2 = -1;     // the pair's other step
                    const FwdStep st2 = fwd_pair_step(k ^ 1, wg, g, nbh, nm, bh2, mb2);
                    CHECK(st2 != kStepEnd && bh2 == bh && mb + mb2 == nm - 1, c, "pair");
                    CHECK((st == kStepSkip) == ((k & 1) && mb == mb2), c, "odd count skip");
                    if (!(k & 1)) CHECK(st == kStepItem && mb >= mb2, c, "heavier block first");
                } else {
                    CHECK(st == kStepItem, c, "boustrophedon has no skips");
                }
                if (st == kStepItem) CHECK(produce(bh, mb), c, "item in range");
            }
            if (pp.persistent == 2) CHECK(!(k & 1), c, "pairs end on an even step");
        }
    } else {
        CHECK(pp.persistent == 3 && c.queue != kQueueStatic, c, "mode");
        CHECK(s.grid.y == 1 && g > 0, c, "persistent grid");
        const bool xq = c.queue == kQueueXcd && pp.xcd_queues;
        CHECK(c.queue == kQueueXcd || !pp.xcd_queues, c, "only kQueueXcd plans per-XCD queues");
        int next[8] = {};                       // the device counters
        std::vector<int> claims[8];             // per queue, in claim order: bh * nm + m_block
        std::vector<int> active(g);
        for (int i = 0; i < g; ++i) active[i] = i;
        unsigned rng = 12345u + 7u * nbh + 3u * nm + c.slots;
        while (!active.empty()) {               // workgroups finish items in an arbitrary order
            rng = rng * 1664525u + 1013904223u;
            const size_t pick = (rng >> 8) % active.size();
            const int wg = active[pick];
            const int x = fwd_queue_of(xq, wg);
            CHECK(x == (xq ? wg % 8 : 0), c, "workgroup w claims from queue w % 8");
            const int q = next[x]++;
            if (q >= fwd_queue_len(xq, x, nbh, nm)) {   // its last (failed) claim
                active[pick] = active.back();
                active.pop_back();
                continue;
            }
            int bh = -1, mb = -1;
            fwd_queue_item(xq, x, q, nbh, nm, bh, mb);
            CHECK(produce(bh, mb), c, "item in range");
            claims[x].push_back(bh * nm + mb);
        }
        for (int x = 0; x < 8; ++x)
            for (size_t q = 0; q < claims[x].size(); ++q) {
                const int bh = claims[x][q] / nm, mb = claims[x][q] % nm;
                if (xq) {   // unit-major: a unit's row blocks consecutive, the heaviest first
                    CHECK(bh % 8 == x, c, "unit on its XCD's queue");
                    CHECK(mb == nm - 1 - (int)(q % nm), c, "heaviest first within a unit");
                    CHECK(bh == claims[x][q - q % nm] / nm, c, "a unit's row blocks are consecutive");
                } else if (q > 0) {
                    CHECK(x == 0 && mb <= claims[x][q - 1] % nm, c, "global queue: heaviest row blocks first");
                }
            }
    }
    for (int i = 0; i < nbh * nm; ++i) CHECK(seen[i] == 1, c, "every item exactly once");
}

}  // namespace

int main() {
    int cases = 0;
    for (int nbh : {1, 7, 8, 9, 57, 64})
        for (int nm : {1, 2, 3, 5, 8})
            for (int slots : {8, 16, 256, 304})
                for (int order : {0, 1})
                    for (int ctr : {0, 1})
                        for (int xcdq : {0, 1})
                            for (FwdQueue queue : {kQueueStatic, kQueueXcd, kQueueRagged}) {
                                run_case(Case{nbh, nm, slots, order, ctr, xcdq, queue});
                                ++cases;
                            }
    std::printf("%d cases, %d failures\n", cases, g_failures);
    return g_failures ? 1 : 0;
}
