// Host model of the dynamic tile-claiming protocol (hn_tiles.h): W workgroups x two roles (the producer waves,
// one of whose lanes claims, and the MFMA waves) walk the very functions the kernels call, against a mocked
// counter pair, in interleavings chosen by a seeded generator.  A role runs from one workgroup barrier to the
// next; it passes a barrier only when its partner has arrived at the same one.  Checked, for ntiles = 0 ..
// 5 W + 3 and NCC in {2, 4}, over two launches on the same counters:
//   - both roles of a workgroup see the same tile sequence and stop after the same barrier;
//   - what the producers stage for stage s is what the MFMA waves compute at stage s;
//   - a ring word is never read before it is published nor overwritten before its last reader is done;
//   - every tile is run exactly once, and the counters end at zero.
// Built by `make tiles_check` with the address and undefined-behaviour sanitizers.  Stand-alone: links nothing
// of the library and needs no GPU.
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <random>
#include <utility>
#include <vector>

#include "hn_tiles.h"

namespace {

using namespace hn_tiles;

#define CHECK(cond, ...)                       \
  do {                                         \
    if (!(cond)) {                             \
      std::fprintf(stderr, "FAILED %s: ", #cond); \
      std::fprintf(stderr, __VA_ARGS__);       \
      std::fprintf(stderr, "\n");              \
      std::exit(1);                            \
    }                                          \
  } while (0)

struct MockCounter {  // the launch's two words of device memory
  unsigned next = 0, left = 0;
  long takes = 0;
  unsigned take() {
    ++takes;
    return next++;
  }
  unsigned leave() { return left++; }
  void reset() { next = left = 0; }
};

struct Ring {  // the LDS words, each tagged with the iteration it was published for
  int word[kSlots];
  int tag[kSlots];
  Ring() {
    for (int i = 0; i < kSlots; ++i) word[i] = 12345, tag[i] = -1000;
  }
};

using Stage = std::pair<int, int>;  // (tile, channel chunk)

struct Role {
  bool producer = false;
  int rb = 0, nwg = 0, ntiles = 0, ncc = 0;
  Ring* ring = nullptr;
  MockCounter* ctr = nullptr;
  Claimer cl = claimer(false);
  Cursor c{0, 0, 0};
  int arrived = 0;  // barriers arrived at
  bool finished = false;
  int pc = 0, j = 0;       // where the role resumes
  std::vector<int> tiles;  // T_k per iteration
  std::vector<Stage> stages;  // producer: staged for stage s (index s); MFMA: computed at stage s

  // the cursor reads of iteration k: the words must be the ones published for k and k + 1
  void check_tags(int k) {
    CHECK(ring->tag[slot(k)] == k, "rb %d %s: T_%d read, slot holds T_%d", rb, producer ? "producer" : "mfma", k,
          ring->tag[slot(k)]);
    CHECK(ring->tag[slot(k + 1)] == k + 1, "rb %d %s: T_%d read, slot holds T_%d", rb, producer ? "producer" : "mfma",
          k + 1, ring->tag[slot(k + 1)]);
  }
  void stage_for(int s_local) {  // the producers' loads + write of stage s_local of this iteration
    const int t = stage_tile(c, s_local, ncc), cc = stage_chunk(s_local, ncc);
    const size_t s = (size_t)c.k * ncc + s_local;
    if (stages.size() <= s) stages.resize(s + 1, Stage(-7, -7));
    stages[s] = Stage(t, cc);
  }
  // Runs to the next barrier (returns true: arrived) or to the end (false).
  bool step() {
    if (producer) {
      switch (pc) {
        case 0:  // prologue: stages 0 and 1 of T_0 = rb, the ring's first words
          ring_init(ring->word, rb, nwg, ntiles);
          for (int k = 0; k < kAhead; ++k) ring->tag[slot(k)] = k;
          stages.push_back(Stage(rb, 0));
          pc = 1;
          return true;
        case 1:
          check_tags(0);
          cursor_start(c, ring->word);
          pc = 2;
          [[fallthrough]];
        case 2:  // iteration head
          if (cursor_done(c)) {
            claim_finish(cl, *ctr, nwg);
            return false;
          }
          tiles.push_back(c.cur);
          if (c.k == 0) stage_for(1);  // (loaded in the prologue, written in the first body)
          claim_issue(cl, *ctr);
          j = 0;
          [[fallthrough]];
        case 3:  // first half of the two-stage body: loads of stage j + 2, write of stage j + 1
          stage_for(j + 2);
          pc = 4;
          return true;
        case 4: {  // second half: loads of stage j + 3, write of stage j + 2; the last body publishes T_{k+2}
          if (j + 3 < 2 * ncc) stage_for(j + 3);
          const bool last = j + 2 == ncc;
          if (last) {
            const int t = claim_settle(cl, *ctr, nwg, ntiles);
            // the slot's previous word was T_{k-2}: nobody may still need it
            CHECK(ring->tag[slot(c.k + 2)] == c.k + 2 - kSlots || ring->tag[slot(c.k + 2)] == -1000,
                  "rb %d: publishing T_%d over T_%d", rb, c.k + 2, ring->tag[slot(c.k + 2)]);
            ring->word[slot(c.k + 2)] = t;
            ring->tag[slot(c.k + 2)] = c.k + 2;
          }
          j += 2;
          pc = last ? 5 : 3;
          return true;
        }
        case 5:
          check_tags(c.k + 1);
          cursor_advance(c, ring->word);
          pc = 2;
          return step();
      }
    } else {
      switch (pc) {
        case 0:  // bias, prologue barrier
          pc = 1;
          return true;
        case 1:
          check_tags(0);
          cursor_start(c, ring->word);
          pc = 2;
          [[fallthrough]];
        case 2:
          if (cursor_done(c)) return false;
          tiles.push_back(c.cur);
          j = 0;
          [[fallthrough]];
        case 3:  // one stage of the tile, then its barrier
          stages.push_back(Stage(c.cur, j));
          ++j;
          pc = j == ncc ? 5 : 3;
          return true;
        case 5:
          check_tags(c.k + 1);
          cursor_advance(c, ring->word);
          pc = 2;
          return step();
      }
    }
    CHECK(false, "bad pc %d", pc);
    return false;
  }
};

long run_launch(int W, int ntiles, int ncc, MockCounter& ctr, std::mt19937& rng) {
  const int nwg = std::min(W, ntiles);  // the launchers' grid: never more workgroups than tiles
  if (nwg == 0) return 0;
  const long takes0 = ctr.takes;
  std::vector<int> perm(nwg);  // the XCD remap: any bijection
  for (int i = 0; i < nwg; ++i) perm[i] = i;
  std::shuffle(perm.begin(), perm.end(), rng);
  std::vector<Ring> rings(nwg);
  std::vector<Role> roles(2 * nwg);
  for (int w = 0; w < nwg; ++w)
    for (int r = 0; r < 2; ++r) {
      Role& x = roles[2 * w + r];
      x.producer = r == 0;
      x.rb = perm[w];
      x.nwg = nwg;
      x.ntiles = ntiles;
      x.ncc = ncc;
      x.ring = &rings[w];
      x.ctr = &ctr;
      x.cl = claimer(x.producer);
    }
  std::vector<int> runnable;
  for (;;) {
    runnable.clear();
    bool all_done = true;
    for (int i = 0; i < 2 * nwg; ++i) {
      const Role &x = roles[i], &o = roles[i ^ 1];
      if (x.finished) continue;
      all_done = false;
      // waiting at barrier number x.arrived: passes once the partner has arrived at it too
      if (x.arrived <= o.arrived) runnable.push_back(i);
      else CHECK(!o.finished, "rb %d: a role waits at barrier %d, its partner ended after %d", x.rb, x.arrived, o.arrived);
    }
    if (all_done) break;
    CHECK(!runnable.empty(), "deadlock");
    const int i = runnable[rng() % runnable.size()];
    Role& x = roles[i];
    if (x.step()) ++x.arrived;
    else x.finished = true;
  }
  std::vector<int> seen(ntiles, 0);
  for (int w = 0; w < nwg; ++w) {
    const Role &p = roles[2 * w], &m = roles[2 * w + 1];
    CHECK(p.arrived == m.arrived, "rb %d: %d producer barriers, %d MFMA barriers", p.rb, p.arrived, m.arrived);
    CHECK(p.tiles == m.tiles, "rb %d: the roles' tile sequences differ", p.rb);
    CHECK(p.arrived == 1 + ncc * (int)m.tiles.size(), "rb %d: barrier count", p.rb);
    CHECK(p.stages.size() >= m.stages.size(), "rb %d: stages staged", p.rb);
    for (size_t s = 0; s < m.stages.size(); ++s)
      CHECK(p.stages[s] == m.stages[s], "rb %d stage %zu: staged (%d, %d), computed (%d, %d)", p.rb, s, p.stages[s].first,
            p.stages[s].second, m.stages[s].first, m.stages[s].second);
    for (size_t s = m.stages.size(); s < p.stages.size(); ++s)  // staged past the end: from an empty resource
      CHECK(p.stages[s].first == kEnd, "rb %d: stage %zu staged for tile %d and never computed", p.rb, s, p.stages[s].first);
    CHECK(!p.cl.live && p.cl.left, "rb %d: the claimer never checked out", p.rb);
    for (int t : m.tiles) {
      CHECK(t >= 0 && t < ntiles, "rb %d: tile %d of %d", p.rb, t, ntiles);
      ++seen[t];
    }
  }
  for (int t = 0; t < ntiles; ++t) CHECK(seen[t] == 1, "tile %d of %d run %d times (W %d)", t, ntiles, seen[t], W);
  CHECK(ctr.next == 0 && ctr.left == 0, "counters end at %u / %u (W %d, ntiles %d)", ctr.next, ctr.left, W, ntiles);
  return ctr.takes - takes0;
}

}  // namespace

int main() {
  std::mt19937 rng(20240611u);
  long launches = 0, takes = 0;
  for (int W : {1, 2, 3, 5, 8, 13})
    for (int ncc : {2, 4})
      for (int ntiles = 0; ntiles <= 5 * W + 3; ++ntiles)
        for (int rep = 0; rep < 24; ++rep) {
          MockCounter ctr;
          for (int launch = 0; launch < 2; ++launch) {  // the second starts from the first one's reset
            takes += run_launch(W, ntiles, ncc, ctr, rng);
            ++launches;
          }
        }
  std::printf("hn_tiles host check: %ld launches, %ld claims, all invariants held\n", launches, takes);
  return 0;
}
