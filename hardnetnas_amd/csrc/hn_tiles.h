// Dynamic work-tile claiming for the persistent forward kernels.
//
// A static persistent kernel fixes each workgroup's tiles at launch (rb, rb + nwg, rb + 2 nwg, ...), so the
// launch ends when the slowest workgroup ends.  Here a workgroup's first kAhead tiles are the static ones
// (nothing waits for a claim in the prologue) and every later tile is claimed from a global counter: ticket v
// of the launch is tile kAhead * nwg + v.  Tile i means the same patches as in the static kernel.
//
// Per workgroup, ONE lane (the claimer) talks to the counter:
//   iteration k (tile T_k runs):  claim_issue   -- atomic add, result not waited for
//                                 ...the tile's stages...
//                                 claim_settle  -- T_{k+2} from the ticket, published into LDS ring slot
//                                                  slot(k + 2) ahead of the iteration's last barrier
// so the atomic has a whole tile to return.  The first ticket past the last tile is the workgroup's last
// claim: T = kEnd from then on, and the claimer checks out on the launch's second counter (claim_settle issues
// that add; claim_finish, at the role's end, looks at what it returned, so nothing waits for it either).  The
// workgroup that checked out last zeroes both counters -- the next launch on them (stream order) starts from zero
// without a memset.  Only atomics touch the counters and no data is published through them, so the order that
// matters needs no fence: a workgroup checks out after its last ticket has come back (the check-out is control-
// dependent on it), and the zeroing follows the last check-out, hence every ticket of the launch.
//
// Every wave of the workgroup, whatever its role, walks the same Cursor: cursor_start after the prologue
// barrier, cursor_advance after each iteration's last barrier, stop when cursor_done.  The tile index and the
// decision to stop come from the same LDS words behind the same barriers for all of them, so the roles'
// barrier counts cannot differ.  hn_tiles_host_check.cpp runs these functions against a mocked counter.
#pragma once

#if defined(__HIPCC__)
#define HN_TILES_FN __host__ __device__ inline
#else
#define HN_TILES_FN inline
#endif

namespace hn_tiles {

constexpr int kEnd = -1;    // "no more tiles"
constexpr int kAhead = 2;   // tiles known ahead of the running one = static tiles per workgroup = queue depth
constexpr int kSlots = 4;   // LDS ring words (T_k, T_{k+1} live, T_{k+2} being published; a power of two)

HN_TILES_FN int slot(int k) { return k & (kSlots - 1); }

// T_k of workgroup rb (its position after the XCD remap) for k < kAhead
HN_TILES_FN int fixed_tile(int k, int rb, int nwg, int ntiles) {
  const long long t = (long long)rb + (long long)k * nwg;
  return t < ntiles ? (int)t : kEnd;
}
// the tile of ticket v
HN_TILES_FN int claimed_tile(unsigned v, int nwg, int ntiles) {
  const long long t = (long long)kAhead * nwg + v;
  return t < ntiles ? (int)t : kEnd;
}

// The claimer's state.  Ctr has take() (next ticket), leave() (check out; the number of workgroups that had
// checked out before) and reset() (both counters to zero).
struct Claimer {
  bool live;        // false: not the claiming lane, or its last claim is behind it
  unsigned ticket;  // the claim in flight
  bool left;        // checked out: `before` workgroups had done so before
  unsigned before;
};
HN_TILES_FN Claimer claimer(bool claiming_lane) { return Claimer{claiming_lane, 0u, false, 0u}; }
template <class Ctr>
HN_TILES_FN void claim_issue(Claimer& c, Ctr& ctr) {
  if (c.live) c.ticket = ctr.take();
}
// the tile of the claim issued by claim_issue (kEnd after the last claim)
template <class Ctr>
HN_TILES_FN int claim_settle(Claimer& c, Ctr& ctr, int nwg, int ntiles) {
  if (!c.live) return kEnd;
  const int t = claimed_tile(c.ticket, nwg, ntiles);
  if (t == kEnd) {
    c.live = false;
    c.left = true;
    c.before = ctr.leave();
  }
  return t;
}
// at the end of the claimer's role
template <class Ctr>
HN_TILES_FN void claim_finish(Claimer& c, Ctr& ctr, int nwg) {
  if (c.left && c.before == (unsigned)nwg - 1u) ctr.reset();
}
// the claimer fills the ring's first kAhead words ahead of the prologue barrier
HN_TILES_FN void ring_init(int* ring, int rb, int nwg, int ntiles) {
  for (int k = 0; k < kAhead; ++k) ring[slot(k)] = fixed_tile(k, rb, nwg, ntiles);
}

// A wave's position in its workgroup's tile sequence
struct Cursor {
  int k;    // iteration
  int cur;  // T_k
  int nxt;  // T_{k+1}: what the producers stage ahead
};
HN_TILES_FN void cursor_start(Cursor& c, const int* ring) {  // after the prologue barrier
  c.k = 0;
  c.cur = ring[slot(0)];
  c.nxt = ring[slot(1)];
}
HN_TILES_FN bool cursor_done(const Cursor& c) { return c.cur == kEnd; }
HN_TILES_FN void cursor_advance(Cursor& c, const int* ring) {  // after iteration k's last barrier
  ++c.k;
  c.cur = c.nxt;
  c.nxt = ring[slot(c.k + 1)];
}
// Stage j of the iteration, counted from the running tile's first stage (j < 2 ncc): its tile and channel chunk
HN_TILES_FN int stage_tile(const Cursor& c, int j, int ncc) { return j < ncc ? c.cur : c.nxt; }
HN_TILES_FN int stage_chunk(int j, int ncc) { return j < ncc ? j : j - ncc; }

#if defined(__HIPCC__)
// the launch's counters in device memory: [0] next ticket, [1] workgroups checked out
struct DeviceCounter {
  unsigned* p;
  __device__ unsigned take() { return atomicAdd(p, 1u); }
  __device__ unsigned leave() { return atomicAdd(p + 1, 1u); }
  __device__ void reset() {
    atomicExch(p, 0u);
    atomicExch(p + 1, 0u);
  }
};
#endif

}  // namespace hn_tiles
