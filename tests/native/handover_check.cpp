// handover_check.cpp -- the host bookkeeping of the tail -> match hand-over (simpleicp_amd/csrc/sicp_handover.h) driven the way
// run_device_tail drives it, with the launchers stubbed out: which stream an iteration goes to, which ticket its match waits for,
// where its record lands.  A stand-alone program for the sanitizers (tests/test_prelaunch_host.py builds it with
// -fsanitize=address,undefined and runs it); exits non-zero with a message at the first broken invariant.
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "../../simpleicp_amd/csrc/sicp_handover.h"

using namespace sicph;

namespace {

struct Launch { int kind; int stream; unsigned long long wait_seq; double seq; int slot; };   // kind 0 match, 1 waiting match, 2 tail

[[noreturn]] void die(const char *what, long a = 0, long b = 0)
{
    std::fprintf(stderr, "handover_check: %s (%ld, %ld)\n", what, a, b);
    std::exit(1);
}

// one run of `max_it` iterations that ends (converges) at record `stop_at` (-1: never), `depth` iterations ahead of the host;
// seq: the context's counter, carried from run to run
void run(bool road, long max_it, long stop_at, int depth, long *seq, long *early_total)
{
    HandOver ho;
    ho.road = road;
    double seqs[HANDOVER_RING];
    std::vector<double> ring(HANDOVER_RING, -1.0);          // the ticket each record slot holds (stub of the pinned ring)
    std::vector<Launch> log;
    long launched = 0, completed = 0;
    bool over = false, event_recorded = false, second_waited = false;
    while (true) {
        while (launched < max_it && launched - completed < depth && !over) {
            const double s = (double)(++*seq);
            const HandOverStep st = ho.next(s);
            if (st.slot != launched % HANDOVER_RING) die("record slot", st.slot, launched);
            if (ring[st.slot] >= 0.0) die("a record slot is reused before its record was taken", st.slot, launched);
            if (!road && (st.stream != 0 || st.wait || st.first_on_second)) die("the single-stream chain left its stream", launched);
            if (road) {
                if (st.stream != (launched & 1)) die("iteration i is not on stream i mod 2", launched, st.stream);
                if (st.wait != (launched > 0)) die("only the first match does not wait", launched);
                if (st.wait && st.wait_seq != (unsigned long long)seqs[(launched - 1) % HANDOVER_RING])
                    die("a match waits for another ticket than the previous tail's", launched, (long)st.wait_seq);
                if (st.first_on_second) {
                    if (second_waited) die("the second stream waits for the setup event twice", launched);
                    if (!event_recorded) die("the second stream waits for an event nobody recorded", launched);
                    second_waited = true;
                }
                if (st.stream == 1 && !second_waited) die("a launch on the second stream before it waited for the setup", launched);
            }
            log.push_back({st.wait ? 1 : 0, st.stream, st.wait_seq, s, st.slot});
            if (launched == 0) event_recorded = true;       // (recorded behind the first match, on stream 0)
            log.push_back({2, st.stream, 0ull, s, st.slot});
            seqs[st.slot] = s;
            ring[st.slot] = s;                              // (the stub tail publishes at once)
            ++launched;
        }
        if (completed == launched) break;
        const int slot = (int)(completed % HANDOVER_RING);
        if (ring[slot] != seqs[slot]) die("the record read is not the launch's", slot, completed);
        ring[slot] = -1.0;
        if (completed == stop_at) over = true;
        ++completed;
    }
    if (ho.launched != launched) die("launch count", (long)ho.launched, launched);
    if (ho.early != (road && launched > 0 ? launched - 1 : 0)) die("early-launch count", (long)ho.early, launched);
    if (ho.second_used != (road && launched > 1)) die("second stream use", launched);
    // tickets grow along the chain, and within a stream the order is match, tail, match, tail
    for (size_t i = 2; i < log.size(); i += 2)
        if (!(log[i].seq > log[i - 1].seq)) die("tickets do not grow", (long)i);
    for (int s = 0; s < 2; ++s) {
        int want = -1;
        for (const Launch &l : log) {
            if (l.stream != s) continue;
            const int kind = l.kind == 2 ? 2 : 0;
            if (want >= 0 && kind != want) die("a stream's launches are not match, tail, match, tail", s);
            want = kind == 2 ? 0 : 2;
        }
    }
    *early_total += ho.early;
}

}  // namespace

int main()
{
    long seq = 0, early = 0;
    for (int road = 0; road < 2; ++road)
        for (long max_it : {1L, 2L, 3L, 9L, 30L, 100L})
            for (long stop_at : {-1L, 0L, 1L, 7L})
                for (int depth : {1, 2, 4, HANDOVER_RING - 1}) {
                    const long before = early;
                    run(road != 0, max_it, stop_at, depth, &seq, &early);
                    if (!road && early != before) die("the single-stream chain launched early");
                }
    std::printf("handover_check OK: %ld launches' tickets, %ld matches launched early\n", seq, early);
    return 0;
}
