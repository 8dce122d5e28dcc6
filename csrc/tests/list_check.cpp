// Checks of dla::ListBatcher (csrc/include/dla_lists.h), the host code that cuts the optimizer, EMA and pack tensor
// lists into by-value kernel launches, as a standalone executable that runs under AddressSanitizer +
// UndefinedBehaviorSanitizer on the CPU beside host_check: 0, 1, 32, 33 and 65 entries; empty tensors skipped and
// kept; a group change at the first and at the last slot of a list; prefix[ntensors] == blocks in every launch;
// tensor_base / block_base running on across launches; the side values; and the chunk-count overflow.
//
// Build + run: python -m distributed_learning_amd._build --sanitize   (g++ -fsanitize=address,undefined)
#include <cstdio>
#include <string>
#include <vector>

#include "../include/dla_lists.h"

using namespace dla;

namespace {

int g_cases = 0, g_fail = 0;

void check(bool ok, const std::string& what) {
  ++g_cases;
  if (!ok) {
    ++g_fail;
    std::fprintf(stderr, "FAIL %s\n", what.c_str());
  }
}

int64_t chunks_of(int64_t numel) { return (numel + kMTChunk - 1) / kMTChunk; }

// What every set of launches must satisfy, against the sequence of (numel, tag) it was built from: every entry
// that should be there is there once, in order, with its own side value; each launch is consistent in itself;
// the bases continue from launch to launch.
struct In {
  int64_t numel;
  int tag;
};

void verify(const std::string& what, const std::vector<In>& in, bool keep_empty, bool tagged) {
  std::vector<float> side(in.size() + 1);
  ListBatcher<SgdEntry> b("check", keep_empty);
  for (size_t i = 0; i < in.size(); ++i) {
    if (tagged) b.tag(in[i].tag);
    SgdEntry e{};
    e.param = &side[i];  // identifies the entry
    e.numel = in[i].numel;
    b.add(e, &side[i]);
  }
  const auto& launches = b.finish();
  size_t next = 0;  // next input entry expected
  int64_t block_base = 0;
  for (size_t k = 0; k < launches.size(); ++k) {
    const auto& L = launches[k];
    const std::string w = what + " launch " + std::to_string(k);
    check(L.list.ntensors >= 1 && L.list.ntensors <= kMaxList, w + ": 1..kMaxList tensors");
    check(L.block_base == block_base, w + ": block_base continues");
    check(L.list.prefix[0] == 0, w + ": prefix starts at 0");
    check(L.list.prefix[L.list.ntensors] == L.blocks, w + ": prefix[ntensors] is the block count");
    int64_t blocks = 0;
    for (int t = 0; t < L.list.ntensors; ++t) {
      while (next < in.size() && in[next].numel == 0 && !keep_empty) ++next;
      if (next >= in.size()) {
        check(false, w + ": more entries than were added");
        return;
      }
      if (t == 0) check(L.tensor_base == (int)next, w + ": tensor_base is the position of slot 0");
      check(L.list.e[t].param == &side[next] && L.ema.ema[t] == &side[next], w + ": entry and side value in order");
      check(L.list.e[t].numel == in[next].numel, w + ": numel");
      check(L.list.prefix[t] == blocks, w + ": prefix[t] is the blocks before slot t");
      check(!tagged || L.tag == in[next].tag, w + ": one group per launch");
      blocks += chunks_of(in[next].numel);
      ++next;
    }
    check(blocks == L.blocks, w + ": blocks");
    // a launch ends only where it must: full, or the next entry is of another group
    if (k + 1 < launches.size())
      check(L.list.ntensors == kMaxList || (tagged && launches[k + 1].tag != L.tag), w + ": split without a reason");
    block_base += L.blocks;
  }
  while (next < in.size() && in[next].numel == 0 && !keep_empty) ++next;
  check(next == in.size(), what + ": every entry is in a launch");
  check(b.total_blocks() == block_base, what + ": total_blocks");
}

std::vector<In> sizes(int n) {
  static const int64_t kSizes[] = {1, 4095, 4096, 4097, 2 * 4096 + 3, 7};
  std::vector<In> in;
  for (int i = 0; i < n; ++i) in.push_back({kSizes[i % 6], 0});
  return in;
}

void counts() {
  for (int n : {0, 1, 32, 33, 65}) {
    for (bool keep : {false, true}) {
      const std::string what = std::to_string(n) + " entries, keep_empty " + std::to_string(keep);
      verify(what, sizes(n), keep, false);
      ListBatcher<PackEntry> b("check", keep);
      for (const In& e : sizes(n)) b.add(PackEntry{nullptr, e.numel, 0});
      check((int)b.finish().size() == (n + kMaxList - 1) / kMaxList, what + ": ceil(n / kMaxList) launches");
    }
  }
}

void empties() {
  for (int n : {1, 32, 33, 65}) {
    for (int at : {0, n / 2, n - 1}) {
      std::vector<In> in = sizes(n);
      in[at].numel = 0;
      const std::string what = std::to_string(n) + " entries, empty at " + std::to_string(at);
      verify(what + ", skipped", in, false, false);
      verify(what + ", kept", in, true, false);
    }
  }
  std::vector<In> all(40, In{0, 0});
  verify("only empties, skipped", all, false, false);
  verify("only empties, kept", all, true, false);
  ListBatcher<EmaEntry> skip("check"), keep("check", true);
  for (int i = 0; i < 40; ++i) {
    skip.add(EmaEntry{});
    keep.add(EmaEntry{});
  }
  check(skip.finish().empty(), "only empties, skipped: no launch");
  check(keep.finish().size() == 2 && keep.total_blocks() == 0, "only empties, kept: two launches of no block");
}

// the group changes at entry `at`: slot 0, slot 1, the last slot of the first list, the first slot of the second
void splits() {
  for (int at : {0, 1, kMaxList - 1, kMaxList, kMaxList + 1, 64}) {
    for (bool keep : {false, true}) {
      std::vector<In> in = sizes(65);
      for (int i = at; i < 65; ++i) in[i].tag = 1;
      in[40].numel = 0;
      verify("group change at " + std::to_string(at) + ", keep_empty " + std::to_string(keep), in, keep, true);
    }
  }
  // a skipped empty entry of another group between two of one group ends no launch
  verify("empty entry of another group", {{5, 0}, {0, 1}, {5, 0}}, false, true);
  ListBatcher<SgdEntry> b("check");
  b.split();
  check(b.finish().empty(), "split() of nothing makes no launch");
}

void overflow() {
  const int64_t big = ((int64_t)1 << 29) * kMTChunk;  // 2^29 chunks
  ListBatcher<PackEntry> ok("pack");
  ok.add(PackEntry{nullptr, big - 1, 0});
  ok.add(PackEntry{nullptr, big - kMTChunk, 0});
  check(ok.finish().size() == 1 && ok.total_blocks() == ((int64_t)1 << 30) - 1, "2^30 - 1 chunks are accepted");
  for (bool across : {false, true}) {
    ListBatcher<PackEntry> b("pack");
    std::string msg;
    try {
      b.add(PackEntry{nullptr, big, 0});
      if (across) b.split();  // the count runs over all launches: LARS's block_base is an int as well
      b.add(PackEntry{nullptr, big, 0});
    } catch (const std::runtime_error& e) {
      msg = e.what();
    }
    check(msg == "pack: too many chunks", std::string("2^30 chunks raise, ") + (across ? "across" : "within") +
                                              " launches: got '" + msg + "'");
  }
}

}  // namespace

int main() {
  counts();
  empties();
  splits();
  overflow();
  std::printf("list_check: %d cases, %d failed\n", g_cases, g_fail);
  return g_fail ? 1 : 0;
}
