// By-value tensor lists of the multi-tensor kernels (multi_tensor.hip) and the host code that fills them.
// Plain C++ (no HIP, no torch), so csrc/tests/list_check.cpp runs the batcher under the CPU sanitizers.
#pragma once

#include <stddef.h>
#include <stdint.h>

#include <stdexcept>
#include <string>
#include <vector>

namespace dla {

// One 256-thread workgroup owns one chunk of one tensor (16 elements per thread).
constexpr int kMTChunk = 4096;
inline int mt_chunk_elems() { return kMTChunk; }

struct SgdEntry {
  float* param;
  const void* grad;      // float* or bf16*
  float* momentum;       // may be null when momentum == 0
  uint16_t* param_bf16;  // optional bf16 shadow copy of the parameter (null = skip)
  int64_t numel;
};

struct PackEntry {
  void* tensor;    // grad tensor (pack source / unpack destination)
  int64_t numel;
  int64_t offset;  // element offset inside the flat bucket
};

// fp32 tensors the optimizer does not step: ema = fmaf(omd, target - ema, ema) (target read only, shadow
// unused), and the in-place exchange target <-> ema with shadow = bf16(new target) where shadow is non-null.
struct EmaEntry {
  float* target;
  float* ema;
  uint16_t* shadow;
  int64_t numel;
};

// FusedLAMB / FusedAdamW: fp32 parameter (or master), gradient, the two fp32 moments and the optional shadow.
struct AdamEntry {
  float* param;
  const void* grad;      // float* or bf16*; unused (null) by the LAMB apply pass
  float* m;              // exp_avg
  float* v;              // exp_avg_sq
  uint16_t* param_bf16;  // optional bf16 shadow copy of the parameter (null = skip)
  int64_t numel;
};

// By-value tensor lists (kernel arguments, no device table): one launch covers up to kMaxList tensors; used
// when tensor addresses change between steps. Entry t owns blocks [prefix[t], prefix[t + 1]) of the launch,
// so prefix[ntensors] (index kMaxList in a full list, hence the + 1) is the launch's block count.
constexpr int kMaxList = 32;
template <class E>
struct TensorList {
  int ntensors;
  int32_t prefix[kMaxList + 1];
  E e[kMaxList];
};
using SgdList = TensorList<SgdEntry>;
using PackList = TensorList<PackEntry>;
using EmaList = TensorList<EmaEntry>;
using AdamList = TensorList<AdamEntry>;

// Weight EMA (exponential moving average), fused into the list update kernels: slot t is the fp32 average of
// list entry t, advanced from the fp32 value the update just stored, ema = fmaf(omd, p_new - ema, ema) with
// omd = 1 - decay read from device memory (one fp32). Passed by value beside the list.
struct EmaSlots {
  float* ema[kMaxList];
};

struct LarsList {
  SgdList l;        // param may be null for the square-sum pass (norms of the grad slot only)
  int tensor_base;  // table row of l.e[0]
  int block_base;   // partial slot of this launch's block 0
};

// The kernel-argument layouts the kernels were built and profiled with.
static_assert(sizeof(SgdList) == 1416 && offsetof(SgdList, e) == 136, "SgdList layout");
static_assert(sizeof(PackList) == 904 && offsetof(PackList, e) == 136, "PackList layout");
static_assert(sizeof(EmaList) == 1160 && offsetof(EmaList, e) == 136, "EmaList layout");
static_assert(sizeof(LarsList) == 1424 && offsetof(LarsList, tensor_base) == 1416, "LarsList layout");
static_assert(sizeof(AdamEntry) == 48 && offsetof(AdamEntry, v) == 24 && offsetof(AdamEntry, numel) == 40,
              "AdamEntry layout");
static_assert(sizeof(AdamList) == 1672 && offsetof(AdamList, e) == 136, "AdamList layout");
static_assert(sizeof(AdamList) + sizeof(EmaSlots) == 1928, "AdamList + EmaSlots kernel arguments");

// Cuts a sequence of entries into by-value launches. It launches nothing: a caller adds (and so checks) every
// tensor first and runs the launches of finish() afterwards, so a bad tensor anywhere raises with nothing done.
template <class E>
class ListBatcher {
 public:
  struct Launch {
    TensorList<E> list;
    EmaSlots ema;     // add()'s side value per slot
    int blocks;       // the grid: list.prefix[list.ntensors]
    int tensor_base;  // add() calls before slot 0, skipped ones included (LARS: the table row of slot 0)
    int block_base;   // blocks of all earlier launches
    int tag;          // the group the entries were added under
  };

  // keep_empty: zero-element entries take a slot (and no block) instead of being skipped
  explicit ListBatcher(const char* op, bool keep_empty = false) : op_(op), keep_empty_(keep_empty) {}

  // Entries added from now on belong to group t (a dtype): no launch mixes two groups.
  void tag(int t) { tag_ = t; }

  // Ends the open launch, if it holds anything.
  void split() {
    if (cur_.list.ntensors > 0) {
      cur_.list.prefix[cur_.list.ntensors] = cur_.blocks;
      launches_.push_back(cur_);
      blocks_ += cur_.blocks;
    }
    cur_ = Launch{};
  }

  void add(const E& e, float* ema = nullptr) {
    const int row = seen_++;
    if (e.numel == 0 && !keep_empty_) return;
    const int64_t chunks = (e.numel + kMTChunk - 1) / kMTChunk;
    // grid sizes, prefix[] and the LARS partial slots are 32-bit
    if (blocks_ + cur_.blocks + chunks >= (int64_t)1 << 30)
      throw std::runtime_error(std::string(op_) + ": too many chunks");
    if (tag_ != cur_.tag) split();
    int& n = cur_.list.ntensors;
    if (n == 0) {
      cur_.tensor_base = row;
      cur_.block_base = (int)blocks_;
      cur_.tag = tag_;
    }
    cur_.list.prefix[n] = cur_.blocks;
    cur_.ema.ema[n] = ema;
    cur_.list.e[n++] = e;
    cur_.blocks += (int)chunks;
    if (n == kMaxList) split();
  }

  const std::vector<Launch>& finish() {
    split();
    return launches_;
  }
  int64_t total_blocks() const { return blocks_; }  // of the finished launches

 private:
  const char* op_;
  bool keep_empty_;
  Launch cur_{};
  std::vector<Launch> launches_;
  int64_t blocks_ = 0;
  int seen_ = 0, tag_ = 0;
};

}  // namespace dla
