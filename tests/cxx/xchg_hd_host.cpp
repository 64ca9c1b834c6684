// Host caller of csrc/ictr_xchg.h as plain C++: the exchange protocol's granule expressions, tag arithmetic, epoch step
// and mailbox layouts. Used by tests/test_xchg_cpu.py, built with the address / undefined-behaviour sanitizers. Takes no
// arguments; prints one line per failed check and returns how many failed (0: all hold).
#include <algorithm>
#include <cfloat>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <vector>

#include "ictr_xchg.h"

using namespace ictr;

static int g_failed = 0;
#define CHECK(cond, ...)                 \
  do {                                   \
    if (!(cond)) {                       \
      if (g_failed < 20) {               \
        printf("FAILED %s: ", #cond);    \
        printf(__VA_ARGS__);             \
        printf("\n");                    \
      }                                  \
      ++g_failed;                        \
    }                                    \
  } while (0)

static float from_bits(uint32_t u) {
  float f;
  memcpy(&f, &u, 4);
  return f;
}
static uint32_t to_bits(float f) {
  uint32_t u;
  memcpy(&u, &f, 4);
  return u;
}

// pack -> value is the identity on the float's bits; the tag test is true exactly for the packed tag
static void granules() {
  const uint32_t vals[] = {0x00000000u, 0x80000000u,               // +-0
                           0x00000001u, 0x807fffffu, 0x00400000u,  // denormals
                           0x7f800000u, 0xff800000u,               // +-inf
                           0x7fc00000u, 0x7f800001u, 0xffc12345u, 0x7fffffffu, 0xffffffffu,  // NaNs with payload
                           to_bits(FLT_MAX), to_bits(-FLT_MAX), to_bits(1.0f), to_bits(FLT_MIN)};
  const unsigned tg[] = {1u, 2u, xchg_tag(xchg_tag0(1), 1), xchg_tag(xchg_tag0((1u << kXchgEpochBits) - 1), kXchgMaxSeq),
                           xchg_rank_tag(1), xchg_rank_tag(0x7fffffffu), 0x7fffffffu, 0xffffffffu};
  for (uint32_t v : vals)
    for (unsigned t : tg) {
      const unsigned long long g = xchg_pack(t, from_bits(v));
      CHECK(to_bits(xchg_value(g)) == v, "value %08x tag %08x", v, t);
      CHECK(!xchg_miss(g, t), "value %08x tag %08x", v, t);
      for (unsigned o : tg) CHECK(xchg_miss(g, o) == (o != t), "value %08x tag %08x other %08x", v, t, o);
      CHECK(xchg_miss(g, t ^ 1u) && xchg_miss(g, t + 1u) && xchg_miss(g, t - 1u) && xchg_miss(g, t ^ 0x80000000u),
            "value %08x tag %08x", v, t);
      CHECK(xchg_miss(g, 0u), "tag 0 is nothing yet: %08x", t);
    }
  for (unsigned t : tg) {
    CHECK(!xchg_miss(xchg_empty(t), t), "empty of %08x", t);
    CHECK(to_bits(xchg_value(xchg_empty(t))) == 0u, "empty of %08x is +0", t);
    CHECK(xchg_empty(t) == xchg_pack(t, 0.0f), "empty of %08x", t);
  }
}

// distinct (epoch, seq) give distinct non-zero tags
static void tags() {
  const unsigned epochs[] = {1u, 2u, 1u << (kXchgEpochBits - 1), (1u << kXchgEpochBits) - 1};
  std::vector<unsigned> all;
  for (unsigned e : epochs) {
    const unsigned t0 = xchg_tag0(e);
    CHECK(t0 != 0u && (t0 >> kXchgSeqBits) == e, "epoch %u", e);
    unsigned prev = t0;
    for (unsigned s = 1; s <= (unsigned)kXchgMaxSeq; ++s) {
      const unsigned t = xchg_tag(t0, s);
      CHECK(t != 0u, "epoch %u seq %u", e, s);
      CHECK(t > prev, "epoch %u seq %u: tags of one epoch ascend, so they are distinct", e, s);
      CHECK((t >> kXchgSeqBits) == e && (t & ((1u << kXchgSeqBits) - 1)) == s, "epoch %u seq %u: fields", e, s);
      CHECK(xchg_parity(s) == (s & 1u), "seq %u", s);
      prev = t;
      all.push_back(t);
    }
  }
  // pairwise, within and across the epochs: no tag twice
  std::sort(all.begin(), all.end());
  CHECK(all.size() == 4 * (size_t)kXchgMaxSeq, "%zu tags", all.size());
  for (size_t i = 1; i < all.size(); ++i) CHECK(all[i - 1] != all[i], "tag %08x twice", all[i]);
  CHECK(xchg_tag(xchg_tag0((1u << kXchgEpochBits) - 1), kXchgMaxSeq) != 0u, "largest tag");
  CHECK((xchg_rank_tag(0) & kXchgRankTagBit) && xchg_rank_tag(5) == (0x80000000u | 5u), "rank tags");
  CHECK(kWallClockHz == 100000000ll, "wall clock");
}

// 0 -> 1 without clearing, n -> n + 1, 2^20 - 1 -> 1 with "clear"
static void epochs() {
  XchgEpoch e = xchg_next_epoch(0);
  CHECK(e.epoch == 1u && !e.clear, "0 -> %u clear %d", e.epoch, (int)e.clear);
  const unsigned last = (1u << kXchgEpochBits) - 1;
  for (unsigned n : {1u, 2u, 4095u, 4096u, 1u << 19, last - 2, last - 1}) {
    e = xchg_next_epoch(n);
    CHECK(e.epoch == n + 1 && !e.clear, "%u -> %u clear %d", n, e.epoch, (int)e.clear);
  }
  e = xchg_next_epoch(last);
  CHECK(e.epoch == 1u && e.clear, "%u -> %u clear %d", last, e.epoch, (int)e.clear);
  // every epoch a mailbox can reach keeps its tags inside 32 bits
  CHECK(((unsigned long long)last << kXchgSeqBits) + kXchgMaxSeq <= 0xffffffffull, "largest tag fits");
}

// marks every granule a layout can address for one parity; checks bounds, that no two addresses coincide, and that the
// two parities do not overlap
struct Marks {
  std::vector<unsigned char> m;
  size_t size;
  explicit Marks(size_t n) : m(n, 0), size(n) {}
  void put(size_t idx, unsigned parity, const char *what) {
    CHECK(idx < size, "%s: index %zu of %zu", what, idx, size);
    if (idx >= size) return;
    CHECK(m[idx] == 0, "%s: granule %zu addressed twice (parity %u, was %u)", what, idx, parity + 1, (unsigned)m[idx]);
    m[idx] = (unsigned char)(parity + 1);
  }
  size_t used() const {
    size_t n = 0;
    for (unsigned char c : m) n += c != 0;
    return n;
  }
};

static void layouts() {
  for (int B : {1, 3})
    for (int team : {2, 3, 63, 64}) {
      Marks mk(team_mail_granules(B, team));
      for (int b = 0; b < B; ++b)
        for (unsigned seq : {1u, 2u})  // one exchange of each parity (seq 3, 4, ... fall on these: parity alone counts)
          for (int part = 0; part < team; ++part)
            for (int k = 0; k < kTeamSlot; ++k)
              mk.put(team_mail_box(b, team) + team_mail_slot(seq, team) + team_mail_row(part) + k, xchg_parity(seq), "team");
      CHECK(mk.used() == mk.size, "team B %d team %d: %zu of %zu", B, team, mk.used(), mk.size);
      CHECK(team_mail_slot(3u, team) == team_mail_slot(1u, team) && team_mail_slot(kXchgMaxSeq, team) == team_mail_slot(2u, team),
            "team %d: the slot is a function of the parity", team);
    }
  for (int slots : {1, 4})
    for (int parts : {1, 2, 253, 254}) {
      Marks mk(res_mail_granules(parts, slots));
      CHECK(res_mail_granules(parts, slots) == (size_t)slots * res_slot_granules(parts), "resident size");
      for (int slot = 0; slot < slots; ++slot)
        for (unsigned seq : {1u, 2u}) {
          const size_t gbox = res_gather_box(slot, parts), bbox = gbox + res_bcast_box(parts);
          for (int part = 0; part < parts; ++part)
            for (int k = 0; k < kResSlot; ++k)
              mk.put(gbox + res_gather_slot(seq, parts) + res_gather_row(part) + k, xchg_parity(seq), "resident gather");
          for (int k = 0; k < kResBcast; ++k) mk.put(bbox + res_bcast_slot(seq) + k, xchg_parity(seq), "resident broadcast");
        }
      CHECK(mk.used() == mk.size, "resident parts %d slots %d: %zu of %zu", parts, slots, mk.used(), mk.size);
    }
  for (long long cap : {32ll, 64ll})
    for (int world : {1, 2, 16}) {
      Marks mk(rank_mail_granules(world, cap));
      for (unsigned seq : {1u, 2u})
        for (int rank = 0; rank < world; ++rank)
          for (long long i = 0; i < cap; ++i)
            mk.put(rank_mail_index(rank_mail_slot(seq, world) + rank, cap, (size_t)i), xchg_parity(seq), "rank");
      CHECK(mk.used() == mk.size, "rank world %d cap %lld: %zu of %zu", world, cap, mk.used(), mk.size);
    }
}

int main() {
  granules();
  tags();
  epochs();
  layouts();
  if (g_failed) printf("%d checks failed\n", g_failed);
  return g_failed ? 1 : 0;
}
