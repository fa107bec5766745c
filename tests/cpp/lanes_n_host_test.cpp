// Host-only check of the rotation and fork rule of a handle's launch chains at 1..4 lanes (csrc/ndt_host.hpp:
// lane_step).  No GPU, no HIP call: the rule is a pure function of the sequence of events on a handle.  Exact sequences
// for three and four lanes first, then a model of the streams over random sequences (fixed seed): every stream is an
// ordered queue, an event record copies what the tail of its stream is ordered behind, a wait merges that into the
// waiting stream.  The driver enqueues what ndt2d_api.hip's begin_align, ndt2d_wait_stream and ndt2d_set_tuning enqueue for
// a plan.  Prints "ok" and returns 0, or says which expectation failed.
#include <cstdint>
#include <cstdio>
#include <initializer_list>
#include <random>

#include "ndt_host.hpp"

using ndt::LaneEvent;
using ndt::LanePlan;
using ndt::LaneState;

namespace {

int failures = 0;

// ---- the rule before there were more than two lanes, verbatim ----------------------------------------------------------
struct OldLaneState {
  int lanes = 2;
  int next = 0;
  bool stale = true;
  bool fork_live = false;
};

LanePlan old_lane_step(OldLaneState& s, LaneEvent ev) {
  LanePlan p;
  if (s.lanes < 2) { s.next = 0; s.stale = true; s.fork_live = false; return p; }
  switch (ev) {
    case LaneEvent::kAsyncFixed:
      p.lane = s.next;
      p.record_fork = s.next == 0;
      if (s.next == 0) {
        p.mark = s.stale;
        if (s.stale) { s.fork_live = true; s.stale = false; }
      } else {
        p.wait = s.fork_live;
        s.fork_live = false;
      }
      s.next ^= 1;
      break;
    case LaneEvent::kWaitStream:
      p.both_wait = true;
      break;
    case LaneEvent::kOther:
      s.stale = true;
      s.fork_live = false;
      s.next = 0;
      break;
    case LaneEvent::kFinish:
      s.next = 0;
      break;
  }
  return p;
}

bool same_plan(const LanePlan& a, const LanePlan& b) {
  return a.lane == b.lane && a.record_fork == b.record_fork && a.both_wait == b.both_wait && a.mark == b.mark && a.wait == b.wait;
}

// ---- exact sequences -----------------------------------------------------------------------------------------------------
struct Want { LaneEvent ev; int lane; bool mark; bool wait; };

void run(const char* name, int lanes, std::initializer_list<Want> seq) {
  LaneState s;
  s.lanes = lanes;
  int k = 0;
  for (const Want& w : seq) {
    const LanePlan p = ndt::lane_step(s, w.ev);
    const bool fork = w.ev == LaneEvent::kAsyncFixed && w.lane == 0 && lanes >= 2;
    if (p.lane != w.lane || p.mark != w.mark || p.wait != w.wait || p.record_fork != fork) {
      std::printf("%s: step %d: lane %d mark %d wait %d record_fork %d, expected lane %d mark %d wait %d record_fork %d\n", name, k,
                  p.lane, (int)p.mark, (int)p.wait, (int)p.record_fork, w.lane, (int)w.mark, (int)w.wait, (int)fork);
      ++failures;
    }
    ++k;
  }
}

// ---- the streams ---------------------------------------------------------------------------------------------------------
// What the tail of a stream (or a recorded event) is ordered behind: the position of the latest non-chain item on the
// handle's stream, of the latest producer a wait_stream named, and the set of chains (at most 64 a sequence).
struct Know {
  int other = -1, producer = -1;
  std::uint64_t chains = 0;
  void merge(const Know& k) {
    other = k.other > other ? k.other : other;
    producer = k.producer > producer ? k.producer : producer;
    chains |= k.chains;
  }
};

struct Event {
  bool recorded = false;
  bool fresh = false;          // recorded since the lane it belongs to last waited for it
  Know know;
  void record(const Know& tail) { recorded = true; fresh = true; know = tail; }
};

void wait(Know& stream, const Event& e) { if (e.recorded) stream.merge(e.know); }     // a wait for an event never recorded is a no-op

struct Totals { long calls[ndt::kMaxLanes] = {}, marks = 0, waits = 0, compared = 0, plain_secondary = 0, plain_waits = 0; };

bool model_sequence(std::mt19937& rng, int q, int length, Totals& tot) {
  LaneState s;
  OldLaneState old;
  bool fork_every = false;
  s.lanes = 1 + (int)(rng() % ndt::kMaxLanes);      // set behind the handle's creation (position 0)
  Know main, side[ndt::kMaxLanes];                  // side[k]: lane k's stream, k >= 1
  Event fork[ndt::kMaxLanes], done[ndt::kMaxLanes];
  int last_other = 0, last_producer = -1, chains = 0;
  main.other = 0;                                   // position 0: the handle's creation and its first build
  for (int pos = 1; pos <= length; ++pos) {
    const unsigned r = rng() % 32;
    LaneEvent ev = LaneEvent::kAsyncFixed;
    if (r == 0 || r == 3 || r == 4) ev = LaneEvent::kOther;
    else if (r == 1) ev = LaneEvent::kFinish;
    else if (r == 2) ev = LaneEvent::kWaitStream;
    const int lanes_before = s.lanes;
    const LanePlan p = ndt::lane_step(s, ev);
    // (d) at one and two lanes the plans are those of the rule before
    if (lanes_before <= 2) {
      old.lanes = lanes_before;
      const LanePlan o = old_lane_step(old, ev);
      ++tot.compared;
      if (!same_plan(p, o)) {
        std::printf("model %d: position %d: at %d lanes the plan differs from the two-lane rule's (lane %d / %d, mark %d / %d, wait %d / %d)\n", q,
                    pos, lanes_before, p.lane, o.lane, (int)p.mark, (int)o.mark, (int)p.wait, (int)o.wait);
        ++failures;
        return false;
      }
    } else if (ev == LaneEvent::kOther) {
      (void)old_lane_step(old, ev);
    }
    if (ev != LaneEvent::kAsyncFixed && (p.mark || p.wait || p.lane || p.record_fork)) {
      std::printf("model %d: position %d: a chain planned for another event\n", q, pos);
      ++failures;
      return false;
    }
    switch (ev) {
      case LaneEvent::kOther:
        // the item itself goes into the handle's stream: (b) has put it behind every chain
        main.other = last_other = pos;
        if (r == 3) s.lanes = 1 + (int)(rng() % ndt::kMaxLanes);       // ndt2d_set_tuning: a kOther event, then the new value
        if (r == 4) fork_every = (rng() & 1) != 0;
        break;
      case LaneEvent::kWaitStream: {
        Event producer;
        Know made;
        made.producer = last_producer = pos;
        producer.record(made);
        wait(main, producer);
        if (p.both_wait) for (int l = 1; l < s.lanes; ++l) wait(side[l], producer);
        break;
      }
      case LaneEvent::kFinish:
        break;
      case LaneEvent::kAsyncFixed: {
        if (p.lane < 0 || p.lane >= s.lanes) { std::printf("model %d: position %d: lane %d of %d\n", q, pos, p.lane, s.lanes); ++failures; return false; }
        if ((p.mark && p.lane != 0) || (p.wait && p.lane == 0)) { std::printf("model %d: position %d: mark / wait on the wrong lane\n", q, pos); ++failures; return false; }
        if (fork_every ? p.record_fork : p.mark) {
          for (int l = 1; l < s.lanes; ++l) fork[l].record(main);
          ++tot.marks;
        }
        Know& stream = p.lane ? side[p.lane] : main;
        if (p.lane && (fork_every || p.wait)) {
          // (c) never a wait for a fork that was not recorded since this lane's last wait
          if (!fork[p.lane].fresh) { std::printf("model %d: position %d: lane %d waits for a fork not recorded since its last wait\n", q, pos, p.lane); ++failures; return false; }
          wait(stream, fork[p.lane]);
          fork[p.lane].fresh = false;
          ++tot.waits;
          if (!fork_every) ++tot.plain_waits;
        }
        if (p.lane && !fork_every) ++tot.plain_secondary;
        // (a) every non-chain item and every producer enqueued before this call is ordered before its chain
        if (stream.other < last_other || stream.producer < last_producer) {
          std::printf("model %d: position %d: a lane-%d chain ahead of the work at %d / the producer at %d (its stream is behind %d / %d)\n", q, pos,
                      p.lane, last_other, last_producer, stream.other, stream.producer);
          ++failures;
          return false;
        }
        stream.chains |= std::uint64_t(1) << chains++;
        if (p.lane) { done[p.lane].record(stream); wait(main, done[p.lane]); }
        ++tot.calls[p.lane];
        // (b) the tail of the handle's stream is behind every chain enqueued so far
        if (main.chains != (chains == 64 ? ~std::uint64_t(0) : (std::uint64_t(1) << chains) - 1)) {
          std::printf("model %d: position %d: the handle's stream is not behind every chain (%llx of %d)\n", q, pos, (unsigned long long)main.chains, chains);
          ++failures;
          return false;
        }
        break;
      }
    }
  }
  return true;
}

void model(unsigned seed, int sequences, int length) {
  std::mt19937 rng(seed);
  Totals tot;
  for (int q = 0; q < sequences; ++q)
    if (!model_sequence(rng, q, length, tot)) return;
  // the model has teeth only if it planned calls on every lane, elided most of the secondary lanes' waits, and compared plans
  // (where every round does not fork by order: NDT_TUNE_LANE_FORK = 0)
  if (tot.calls[3] < sequences || tot.calls[2] < sequences || tot.plain_waits * 2 > tot.plain_secondary || tot.plain_waits == 0 ||
      tot.waits == tot.plain_waits || tot.compared < sequences) {
    std::printf("model: calls %ld / %ld / %ld / %ld, %ld marks, %ld waits (%ld of %ld without the fork at every round), %ld plans compared: "
                "not the traffic it was meant to check\n", tot.calls[0], tot.calls[1], tot.calls[2], tot.calls[3], tot.marks, tot.waits,
                tot.plain_waits, tot.plain_secondary, tot.compared);
    ++failures;
  }
}

}  // namespace

int main() {
  const LaneEvent A = LaneEvent::kAsyncFixed, W = LaneEvent::kWaitStream, O = LaneEvent::kOther, F = LaneEvent::kFinish;
  // back-to-back calls: only the first round forks
  run("three lanes back to back", 3, {{A, 0, true, false}, {A, 1, false, true}, {A, 2, false, true}, {A, 0, false, false}, {A, 1, false, false},
                                      {A, 2, false, false}, {A, 0, false, false}, {A, 1, false, false}, {A, 2, false, false}, {A, 0, false, false}});
  run("four lanes back to back", 4, {{A, 0, true, false}, {A, 1, false, true}, {A, 2, false, true}, {A, 3, false, true}, {A, 0, false, false},
                                     {A, 1, false, false}, {A, 2, false, false}, {A, 3, false, false}, {A, 0, false, false}, {A, 1, false, false},
                                     {A, 2, false, false}, {A, 3, false, false}, {A, 0, false, false}});
  for (int lanes = 3; lanes <= 4; ++lanes) {
    LaneState s;
    s.lanes = lanes;
    int marks = 0, waits = 0;
    for (int k = 0; k < 50; ++k) {
      const LanePlan p = ndt::lane_step(s, A);
      if (p.lane != k % lanes) { std::printf("%d lanes: call %d on lane %d\n", lanes, k, p.lane); ++failures; }
      marks += p.mark;
      waits += p.wait;
    }
    if (marks != 1 || waits != lanes - 1) { std::printf("%d lanes, 50 calls: %d marks, %d waits\n", lanes, marks, waits); ++failures; }
  }
  // other inside the first round: the pending forks are dropped, the rotation starts over and every lane forks behind it
  run("other inside the first round", 4, {{A, 0, true, false}, {A, 1, false, true}, {O, 0, false, false}, {A, 0, true, false}, {A, 1, false, true},
                                          {A, 2, false, true}, {A, 3, false, true}, {A, 0, false, false}, {A, 1, false, false}});
  // other in steady state, with lane 2 next
  run("other in steady state", 3, {{A, 0, true, false}, {A, 1, false, true}, {A, 2, false, true}, {A, 0, false, false}, {A, 1, false, false},
                                   {O, 0, false, false}, {A, 0, true, false}, {A, 1, false, true}, {A, 2, false, true}, {A, 0, false, false}});
  // finish inside the first round: the rotation starts over, and the forks recorded by the first call are still the ones
  // lanes 2 and 3 have to wait for when their turn comes
  run("finish inside the first round", 4, {{A, 0, true, false}, {A, 1, false, true}, {F, 0, false, false}, {A, 0, false, false}, {A, 1, false, false},
                                           {A, 2, false, true}, {F, 0, false, false}, {A, 0, false, false}, {A, 1, false, false}, {A, 2, false, false},
                                           {A, 3, false, true}, {A, 0, false, false}, {A, 1, false, false}, {A, 2, false, false}, {A, 3, false, false}});
  // wait_stream keeps the rotation and the state of the forks
  run("wait_stream", 3, {{W, 0, false, false}, {A, 0, true, false}, {W, 0, false, false}, {A, 1, false, true}, {W, 0, false, false},
                         {A, 2, false, true}, {W, 0, false, false}, {A, 0, false, false}, {A, 1, false, false}, {W, 0, false, false}, {A, 2, false, false}});
  // the count going 4 -> 2 -> 3 (a tuning change is an `other` call): every secondary lane is stale when it comes back
  {
    LaneState s;
    s.lanes = 4;
    for (int k = 0; k < 6; ++k) (void)ndt::lane_step(s, A);
    (void)ndt::lane_step(s, O);
    s.lanes = 2;
    const LanePlan a0 = ndt::lane_step(s, A), a1 = ndt::lane_step(s, A), a2 = ndt::lane_step(s, A);
    if (a0.lane != 0 || !a0.mark || a1.lane != 1 || !a1.wait || a2.lane != 0 || a2.mark) { std::printf("knob 4 -> 2: not the two-lane round\n"); ++failures; }
    (void)ndt::lane_step(s, O);
    s.lanes = 3;
    const LanePlan b0 = ndt::lane_step(s, A), b1 = ndt::lane_step(s, A), b2 = ndt::lane_step(s, A), b3 = ndt::lane_step(s, A);
    if (b0.lane != 0 || !b0.mark || b1.lane != 1 || !b1.wait || b2.lane != 2 || !b2.wait || b3.lane != 0 || b3.mark) {
      std::printf("knob 2 -> 3: not the three-lane round\n");
      ++failures;
    }
  }
  model(20261u, 200000, 40);
  if (failures == 0) std::printf("ok\n");
  return failures == 0 ? 0 : 1;
}
