// Host-only check of the pairing rule of a handle's two launch chains (csrc/ndt_host.hpp: lane_step).  No GPU, no HIP
// call: the rule is a pure function of the sequence of events on a handle.  Prints "ok" and returns 0, or says which
// expectation failed.
#include <cstdio>
#include <initializer_list>

#include "ndt_host.hpp"

using ndt::LaneEvent;
using ndt::LanePlan;
using ndt::LaneState;

namespace {

int failures = 0;

struct Want { LaneEvent ev; int lane; bool fork; };

void run(const char* name, int lanes, std::initializer_list<Want> seq) {
  LaneState s;
  s.lanes = lanes;
  int k = 0;
  for (const Want& w : seq) {
    const LanePlan p = ndt::lane_step(s, w.ev);
    const bool wait_both = w.ev == LaneEvent::kWaitStream && lanes == 2;
    if (p.lane != w.lane || p.record_fork != w.fork || p.both_wait != wait_both) {
      std::printf("%s: step %d: lane %d fork %d both_wait %d, expected lane %d fork %d both_wait %d\n", name, k, p.lane,
                  (int)p.record_fork, (int)p.both_wait, w.lane, (int)w.fork, (int)wait_both);
      ++failures;
    }
    ++k;
  }
}

}  // namespace

int main() {
  const LaneEvent A = LaneEvent::kAsyncFixed, W = LaneEvent::kWaitStream, O = LaneEvent::kOther, F = LaneEvent::kFinish;
  run("pairs", 2, {{A, 0, true}, {A, 1, false}, {A, 0, true}, {A, 1, false}, {A, 0, true}});
  // a / a / other / a / a: the other call ends the pair, the next one starts at lane 0 with a fork of its own
  run("other after a pair", 2, {{A, 0, true}, {A, 1, false}, {O, 0, false}, {A, 0, true}, {A, 1, false}});
  // other in the middle of a pair: the saved fork is stale, so the next call is a lane-0 call again (serial, correct)
  run("other inside a pair", 2, {{A, 0, true}, {O, 0, false}, {A, 0, true}, {A, 1, false}});
  // wait_stream between calls keeps the pairing (both lanes wait for the producer)
  run("wait_stream", 2, {{W, 0, false}, {A, 0, true}, {W, 0, false}, {A, 1, false}, {W, 0, false}, {A, 0, true}, {W, 0, false}, {A, 1, false}});
  // finish between calls: both lanes idle, lane 0 next - also in the middle of a pair
  run("finish", 2, {{A, 0, true}, {F, 0, false}, {A, 0, true}, {A, 1, false}, {F, 0, false}, {A, 0, true}, {A, 1, false}});
  // one lane: nothing alternates, no event is recorded
  run("one lane", 1, {{A, 0, false}, {A, 0, false}, {W, 0, false}, {O, 0, false}, {A, 0, false}, {F, 0, false}, {A, 0, false}});
  // the knob changed between calls (a tuning change is an `other` call)
  {
    LaneState s;
    (void)ndt::lane_step(s, A);
    (void)ndt::lane_step(s, O);
    s.lanes = 1;
    const LanePlan p = ndt::lane_step(s, A);
    if (p.lane != 0 || p.record_fork) { std::printf("knob: one-lane call planned on lane %d\n", p.lane); ++failures; }
    s.lanes = 2;
    const LanePlan q = ndt::lane_step(s, A);
    if (q.lane != 0 || !q.record_fork) { std::printf("knob: first two-lane call planned on lane %d\n", q.lane); ++failures; }
  }
  if (failures == 0) std::printf("ok\n");
  return failures == 0 ? 0 : 1;
}
