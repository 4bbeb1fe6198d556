// sicp_handover.h -- the host's bookkeeping of the tail -> match hand-over ("The tail -> match hand-over"): which stream an
// iteration of a chained run goes to, whether its match is launched early and which ticket it then waits for, and where its record
// lands.  Plain C++ (no HIP): run_device_tail (sicp_icp.cpp) drives the launches with it, tests/native/handover_check.cpp drives
// stubs with it under the sanitizers.
#ifndef SICP_HANDOVER_H
#define SICP_HANDOVER_H

#include <cstdint>

namespace sicph {

constexpr int HANDOVER_RING = 16;       // = REC_RING (sicp_host.h checks): records in flight + being read

// One iteration's place in the chain.
struct HandOverStep {
    int stream = 0;                     // 0: the context's stream, 1: its second one
    bool wait = false;                  // the match is the waiting kernel ...
    unsigned long long wait_seq = 0;    // ... released by the ticket of the tail launched just before it
    bool first_on_second = false;       // the run's first launch on the second stream: it waits (once) for the run's setup event
    int slot = 0;                       // the record's place in the pinned ring
};

// A run's hand-over state.  road: the run launches its matches early (decided once, before the first launch).
struct HandOver {
    bool road = false;
    int64_t launched = 0;               // iterations enqueued so far
    int64_t early = 0;                  // ... of which with a waiting match
    double last_seq = 0.0;              // the ticket of the last tail enqueued
    bool second_used = false;

    // the iteration about to be enqueued; seq: its tail's ticket (unique and growing over the context's life)
    HandOverStep next(double seq)
    {
        HandOverStep s;
        s.slot = (int)(launched % HANDOVER_RING);
        if (road) {
            s.stream = (int)(launched & 1);                    // iteration i, match and tail: stream i mod 2
            s.wait = launched > 0;                             // (the first match follows the setup in stream order)
            s.wait_seq = s.wait ? (unsigned long long)last_seq : 0ull;
            s.first_on_second = s.stream == 1 && !second_used;
            if (s.stream == 1) second_used = true;
            if (s.wait) ++early;
        }
        last_seq = seq;
        ++launched;
        return s;
    }
};

}  // namespace sicph

#endif
