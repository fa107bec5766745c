// Host-only check of when lane 1 of a handle forks from the handle's stream (csrc/ndt_host.hpp: lane_step, the `mark`
// and `wait` fields of its plan).  No GPU, no HIP call: the rule is a pure function of the sequence of events on a
// handle.  Exact sequences first, then an ordering model over random sequences (fixed seed).  Prints "ok" and returns 0,
// or says which expectation failed.
#include <cstdio>
#include <initializer_list>
#include <random>

#include "ndt_host.hpp"

using ndt::LaneEvent;
using ndt::LanePlan;
using ndt::LaneState;

namespace {

int failures = 0;

struct Want { LaneEvent ev; int lane; bool mark; bool wait; };

void run(const char* name, int lanes, std::initializer_list<Want> seq) {
  LaneState s;
  s.lanes = lanes;
  int k = 0;
  for (const Want& w : seq) {
    const LanePlan p = ndt::lane_step(s, w.ev);
    if (p.lane != w.lane || p.mark != w.mark || p.wait != w.wait) {
      std::printf("%s: step %d: lane %d mark %d wait %d, expected lane %d mark %d wait %d\n", name, k, p.lane, (int)p.mark,
                  (int)p.wait, w.lane, (int)w.mark, (int)w.wait);
      ++failures;
    }
    // a fork is only ever recorded by a lane-0 call and waited for by a lane-1 call
    if ((p.mark && (w.ev != LaneEvent::kAsyncFixed || p.lane != 0)) || (p.wait && (w.ev != LaneEvent::kAsyncFixed || p.lane != 1))) {
      std::printf("%s: step %d: mark / wait on the wrong kind of event\n", name, k);
      ++failures;
    }
    ++k;
  }
}

// The ordering the plans produce.  Positions count the events of a sequence; `other` is the position of the latest
// non-chain work on the handle's stream, `fork` the position the fork event was last recorded at (it covers everything
// on the handle's stream before it), `behind` the position up to which lane 1 is ordered behind the handle's stream.
// A lane-1 call must never be planned with behind < other.
void model(unsigned seed, int sequences, int length) {
  std::mt19937 rng(seed);
  long marks = 0, waits = 0, lane1_calls = 0;
  for (int q = 0; q < sequences; ++q) {
    LaneState s;
    int other = 0, fork = -1, behind = -1;      // position 0: the handle's creation and its first build count as non-chain work
    for (int pos = 1; pos <= length; ++pos) {
      const unsigned r = rng() % 16;
      LaneEvent ev = LaneEvent::kAsyncFixed;
      if (r == 0) ev = LaneEvent::kOther;
      else if (r == 1) ev = LaneEvent::kFinish;
      else if (r == 2) ev = LaneEvent::kWaitStream;
      else if (r == 3) ev = LaneEvent::kOther;
      const int knob = r == 3 ? 1 + (int)(rng() % 2) : s.lanes;      // ndt2d_set_tuning: a kOther event, then the new value
      const LanePlan p = ndt::lane_step(s, ev);
      if (ev == LaneEvent::kOther) other = pos;
      s.lanes = knob;
      if (ev != LaneEvent::kAsyncFixed) {
        if (p.mark || p.wait || p.lane) { std::printf("model %d: position %d: a chain planned for another event\n", q, pos); ++failures; }
        continue;
      }
      if (s.lanes < 2 && (p.lane || p.mark || p.wait)) { std::printf("model %d: one lane, yet lane %d mark %d wait %d\n", q, p.lane, (int)p.mark, (int)p.wait); ++failures; }
      if (p.mark) { fork = pos; ++marks; }
      if (p.lane == 1) {
        ++lane1_calls;
        if (p.wait) { behind = fork > behind ? fork : behind; ++waits; }
        if (behind < other) {
          std::printf("model %d: position %d: a lane-1 call ahead of the non-chain work at %d (lane 1 is behind %d)\n", q, pos, other, behind);
          ++failures;
          return;
        }
      }
    }
  }
  // the model has teeth only if it planned lane-1 calls, and elided most of their waits
  if (lane1_calls < sequences || waits * 2 > lane1_calls || marks < waits) {
    std::printf("model: %ld lane-1 calls, %ld marks, %ld waits: not the traffic it was meant to check\n", lane1_calls, marks, waits);
    ++failures;
  }
}

}  // namespace

int main() {
  const LaneEvent A = LaneEvent::kAsyncFixed, W = LaneEvent::kWaitStream, O = LaneEvent::kOther, F = LaneEvent::kFinish;
  // back-to-back calls: one mark, one wait, then none
  run("back to back", 2, {{A, 0, true, false}, {A, 1, false, true}, {A, 0, false, false}, {A, 1, false, false}, {A, 0, false, false},
                          {A, 1, false, false}, {A, 0, false, false}});
  {
    LaneState s;
    int marks = 0, waits = 0;
    for (int k = 0; k < 50; ++k) { const LanePlan p = ndt::lane_step(s, A); marks += p.mark; waits += p.wait; }
    if (marks != 1 || waits != 1) { std::printf("50 calls: %d marks, %d waits\n", marks, waits); ++failures; }
  }
  // other after a pair, and in steady state: the next pair forks behind it, the one after does not
  run("other after a pair", 2, {{A, 0, true, false}, {A, 1, false, true}, {O, 0, false, false}, {A, 0, true, false}, {A, 1, false, true},
                                {A, 0, false, false}, {A, 1, false, false}});
  run("other in steady state", 2, {{A, 0, true, false}, {A, 1, false, true}, {A, 0, false, false}, {A, 1, false, false}, {A, 0, false, false},
                                   {O, 0, false, false}, {A, 0, true, false}, {A, 1, false, true}, {A, 0, false, false}, {A, 1, false, false}});
  // other inside a pair: the recorded fork is dropped, the next lane-0 call records one behind the other call
  run("other inside a pair", 2, {{A, 0, true, false}, {O, 0, false, false}, {A, 0, true, false}, {A, 1, false, true}, {A, 0, false, false}});
  run("other inside a steady pair", 2, {{A, 0, true, false}, {A, 1, false, true}, {A, 0, false, false}, {O, 0, false, false},
                                        {A, 0, true, false}, {A, 1, false, true}});
  // two others in a row, and an other before the first call, change nothing
  run("others in a row", 2, {{O, 0, false, false}, {O, 0, false, false}, {A, 0, true, false}, {A, 1, false, true}, {O, 0, false, false},
                             {O, 0, false, false}, {A, 0, true, false}, {A, 1, false, true}});
  // finish inside a pair: the fork recorded by the first call is still the one lane 1 has to wait for
  run("finish inside a pair", 2, {{A, 0, true, false}, {F, 0, false, false}, {A, 0, false, false}, {A, 1, false, true}, {A, 0, false, false},
                                  {A, 1, false, false}});
  // finish in steady state, between pairs and inside one: nothing new on the handle's stream, no fork
  run("finish in steady state", 2, {{A, 0, true, false}, {A, 1, false, true}, {F, 0, false, false}, {A, 0, false, false}, {A, 1, false, false},
                                    {A, 0, false, false}, {F, 0, false, false}, {A, 0, false, false}, {A, 1, false, false}});
  // wait_stream keeps the pairing and the state of the fork (begin_align's caller makes lane 1 wait for the producer)
  run("wait_stream", 2, {{W, 0, false, false}, {A, 0, true, false}, {W, 0, false, false}, {A, 1, false, true}, {W, 0, false, false},
                         {A, 0, false, false}, {W, 0, false, false}, {A, 1, false, false}});
  // one lane: nothing alternates, nothing is recorded or waited for
  run("one lane", 1, {{A, 0, false, false}, {A, 0, false, false}, {W, 0, false, false}, {O, 0, false, false}, {A, 0, false, false},
                      {F, 0, false, false}, {A, 0, false, false}});
  // the knob going 2 -> 1 -> 2 (a tuning change is an `other` call): lane 1 is stale when it comes back
  {
    LaneState s;
    for (int k = 0; k < 4; ++k) (void)ndt::lane_step(s, A);
    (void)ndt::lane_step(s, O);
    s.lanes = 1;
    for (int k = 0; k < 3; ++k) {
      const LanePlan p = ndt::lane_step(s, A);
      if (p.lane != 0 || p.mark || p.wait) { std::printf("knob: one-lane call planned on lane %d mark %d wait %d\n", p.lane, (int)p.mark, (int)p.wait); ++failures; }
    }
    (void)ndt::lane_step(s, O);
    s.lanes = 2;
    const LanePlan q0 = ndt::lane_step(s, A), q1 = ndt::lane_step(s, A), q2 = ndt::lane_step(s, A), q3 = ndt::lane_step(s, A);
    if (q0.lane != 0 || !q0.mark || q0.wait || q1.lane != 1 || q1.mark || !q1.wait) { std::printf("knob: the first two-lane pair does not fork\n"); ++failures; }
    if (q2.lane != 0 || q2.mark || q2.wait || q3.lane != 1 || q3.mark || q3.wait) { std::printf("knob: the second two-lane pair forks\n"); ++failures; }
    // and without the `other` event (the state alone, as a one-lane step leaves it)
    LaneState t;
    (void)ndt::lane_step(t, A);
    (void)ndt::lane_step(t, A);
    t.lanes = 1;
    (void)ndt::lane_step(t, A);
    t.lanes = 2;
    const LanePlan r0 = ndt::lane_step(t, A), r1 = ndt::lane_step(t, A);
    if (!r0.mark || r0.lane != 0 || !r1.wait || r1.lane != 1) { std::printf("knob: lane 1 not stale after a one-lane step\n"); ++failures; }
  }
  model(12345u, 200000, 40);
  if (failures == 0) std::printf("ok\n");
  return failures == 0 ? 0 : 1;
}
