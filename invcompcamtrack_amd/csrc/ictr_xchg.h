// ictr_xchg.h -- the in-launch exchange protocol, stated once for the host and the device. Its users: the team form of
// k_track1_p8 (ictr_track1.hip), k_level_resident and its sums over the ranks (ictr_resident.hip), k_p2p_allreduce
// (ictr_p2p.hip) and exchange_prepare (ictr_host.hip). The same text compiles as plain C++ under sanitizers for
// tests/cxx/xchg_hd_host.cpp (tests/test_xchg_cpu.py).
//
// The protocol (no flag, no fence: MI355X_MICROARCH.md "Valid forms", R2):
//   * a value travels as ONE naturally aligned 8-byte granule {float bits, tag}, written by one store and polled on its
//     tag: a granule is either old or complete;
//   * tag = launch epoch << kXchgSeqBits | exchange number. The exchange number starts at 1 in every launch and stays
//     <= kXchgMaxSeq (the host refuses a form that could count further); the epoch starts at 1, every launch on a mailbox
//     gets the next one, and the mailbox is cleared when it is made and when the epoch wraps: tag 0 means "nothing yet",
//     and nothing an earlier or failed launch left behind can match. The rank mailbox is shared by two users: k_p2p_allreduce
//     tags with the p2p object's bare sequence number (one exchange per launch, small numbers), the resident form's sums
//     over the ranks with kXchgRankTagBit | the pair's exchange count, the other half of the tag space;
//   * slots are double-buffered by the exchange number's parity: a peer can be at most one exchange ahead (it needs this
//     one's granules of exchange k + 1 before it can finish k + 1 and start k + 2), so slot k & 1 is never overwritten
//     while it is still being read;
//   * every reader adds the slots in the same fixed order: the same bits everywhere, redundant solves stay in lockstep;
//   * polling is bounded by a wall-clock limit. On a time-out the poller raises a sticky flag and never waits again, so
//     every wave reaches the end of its kernel; the host reports the tracking as failed.
// How many requests a poller keeps in flight, which lane owns which granule and how long it sleeps between sweeps is
// tuned per site and stays there.
#pragma once

#include <stddef.h>

#if defined(__HIPCC__)
#include <hip/hip_runtime.h>
#define ICTR_XHD __host__ __device__ __forceinline__
#else
#define ICTR_XHD inline __attribute__((always_inline))
#endif

namespace ictr {

// ---------------------------------------------------------------- tags
constexpr int kXchgSeqBits = 12;    // exchange number of a launch
constexpr int kXchgEpochBits = 20;  // launch epoch of a mailbox
constexpr int kXchgMaxSeq = 4000;   // exchange numbers a launch may use: 1 .. kXchgMaxSeq
static_assert(kXchgMaxSeq < (1 << kXchgSeqBits), "an exchange number must fit its field of the tag");
static_assert(kXchgSeqBits + kXchgEpochBits == 32, "a tag is the upper half of a granule");
constexpr unsigned kXchgRankTagBit = 0x80000000u;  // tags of the sums over the ranks
constexpr long long kWallClockHz = 100000000;      // wall_clock64 ticks per second

ICTR_XHD unsigned xchg_tag0(unsigned epoch) { return epoch << kXchgSeqBits; }
ICTR_XHD unsigned xchg_tag(unsigned tag0, unsigned seq) { return tag0 + seq; }
ICTR_XHD unsigned xchg_rank_tag(unsigned seq) { return kXchgRankTagBit | seq; }
ICTR_XHD unsigned xchg_parity(unsigned seq) { return seq & 1u; }

// the host's step from one launch on a mailbox to the next (a new mailbox is cleared and starts at epoch 0)
struct XchgEpoch {
  unsigned epoch;  // of the next launch
  bool clear;      // the epoch field wrapped: forget every old tag before that launch
};
ICTR_XHD XchgEpoch xchg_next_epoch(unsigned epoch) {
  epoch += 1;
  if (epoch >= (1u << kXchgEpochBits)) return XchgEpoch{1u, true};
  return XchgEpoch{epoch, false};
}

// ---------------------------------------------------------------- granules
ICTR_XHD unsigned long long xchg_pack(unsigned tag, float v) {
  return ((unsigned long long)tag << 32) | (unsigned long long)__builtin_bit_cast(unsigned, v);
}
// "arrived, value +0": what a lane without a granule of its own holds, and what a timed-out poll leaves
ICTR_XHD unsigned long long xchg_empty(unsigned tag) { return (unsigned long long)tag << 32; }
ICTR_XHD bool xchg_miss(unsigned long long g, unsigned tag) { return (unsigned)(g >> 32) != tag; }
ICTR_XHD float xchg_value(unsigned long long g) { return __builtin_bit_cast(float, (unsigned)(g & 0xffffffffu)); }

// ---------------------------------------------------------------- mailbox layouts (in granules), each with its size
// A kernel forms an address in the steps below (box, parity slot, a workgroup's row in the slot, + the granule's number
// in the row); the host allocates the size.
// team form: [B][2][team][kTeamSlot]
constexpr int kTeamSlot = 32;  // granules per workgroup and exchange (21 of H or 6 of b)
ICTR_XHD size_t team_mail_granules(int B, int team) { return (size_t)B * 2 * team * kTeamSlot; }
ICTR_XHD size_t team_mail_box(int b, int team) { return (size_t)b * 2 * team * kTeamSlot; }
ICTR_XHD size_t team_mail_slot(unsigned seq, int team) { return (size_t)xchg_parity(seq) * team * kTeamSlot; }
ICTR_XHD size_t team_mail_row(int part) { return (size_t)part * kTeamSlot; }

// resident form, per pair in flight: gather box [2][parts][kResSlot], then broadcast box [2][kResBcast]
constexpr int kResSlot = 8;    // granules per worker workgroup in the gather box (6 used)
constexpr int kResBcast = 16;  // granules of a broadcast (cpos_G and the loop flag: 13 used)
ICTR_XHD size_t res_slot_granules(int parts) { return (size_t)2 * parts * kResSlot + 2 * kResBcast; }
ICTR_XHD size_t res_mail_granules(int parts, int slots) { return (size_t)slots * res_slot_granules(parts); }
ICTR_XHD size_t res_gather_box(int slot, int parts) { return (size_t)slot * res_slot_granules(parts); }
ICTR_XHD size_t res_bcast_box(int parts) { return (size_t)2 * parts * kResSlot; }  // from the pair's gather box
// (the two parity slots are macros that paste the text k_level_resident was tuned with: as inlined functions of the same
// meaning they change the kernel's register allocation, and the resident form's step was measured 0.4 % slower)
#define res_gather_slot(seq, parts) ((size_t)((seq) & 1u) * (parts) * kResSlot)
ICTR_XHD size_t res_gather_row(int part) { return (size_t)part * kResSlot; }
#define res_bcast_slot(seq) ((size_t)((seq) & 1u) * kResBcast)

// rank mailbox (one per rank, mapped into every peer): [2][world][cap]
ICTR_XHD size_t rank_mail_granules(int world, long long cap) { return (size_t)2 * world * cap; }
ICTR_XHD size_t rank_mail_slot(unsigned seq, int world) { return (size_t)xchg_parity(seq) * world; }  // in units of cap
// slot_rank = rank_mail_slot(seq, world) + the writing rank (a size_t sum: the callers add unrolled loop counters to it)
ICTR_XHD size_t rank_mail_index(size_t slot_rank, long long cap, size_t i) { return slot_rank * cap + i; }

// ---------------------------------------------------------------- one exchange as the host hands it to a launch
// (team form of k_track1, k_level_resident: a kernel-argument member of T1Args and ResArgs, filled by exchange_prepare)
struct Exchange {
  unsigned tag0;             // xchg_tag0(launch epoch); the kernels add the exchange number
  unsigned long long limit;  // polling limit, wall_clock64 ticks
  unsigned long long *mail;  // granules; tag 0 = "nothing yet"
  int *err;                  // sticky time-out flag (pinned host memory as the device sees it)
  int mute;                  // debug (ICTR_VARIANT_DEBUG_MUTE), 0 = off: part (k_track1) / worker (k_level_resident)
                             // `mute - 1` of every problem never posts its values (time-out tests)
};

// ---------------------------------------------------------------- what bounds a poller, and its time-out step
struct XchgPoll {
  unsigned long long limit;
  int *err;
  int dead;  // a poll timed out: never wait again
};
// The time-out step of a poll loop that still misses a granule (wave-uniform; `started` and `t0` are the loop's locals,
// false and 0 before it). The first pass starts the clock: a poll that is answered at once never reads it. When the
// limit has run out, lane 0 raises the flag, p.dead is set and the step leaves the loop it stands in. A macro, not a
// function: as an inlined function the two register-bound kernels (k_level_resident, k_track1_p8's team forms) come out
// with other register allocations and spill counts; this pastes the text they were tuned with.
// (k_p2p_allreduce keeps a variant of its own beside its loop: a device flag, no dead state.)
#define XCHG_TIMEOUT_STEP(p, started, t0, lane)                                                          \
  if (!(started)) {                                                                                      \
    (t0) = wall_clock64();                                                                               \
    (started) = true;                                                                                    \
  } else if (wall_clock64() - (t0) > (p).limit) { /* a peer never arrived: flag it, never wait again */  \
    if ((lane) == 0) __hip_atomic_store((p).err, 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);        \
    (p).dead = 1;                                                                                        \
    break;                                                                                               \
  }

}  // namespace ictr
